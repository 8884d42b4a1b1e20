"""CPU: the binding table of the packed MXFP4 copies (csrc/mxfp4_bind.h) as a stand-alone program, plain and under AddressSanitizer +
UBSan, and the library's own table through the C ABI (host only: the addresses are never dereferenced)."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

CSRC = os.path.join(ROOT, "spatialrgpt_amd", "csrc")


def _build(out_dir, name, sanitize):
    """tests/<name>.cpp (a header of csrc alone, no HIP) -> a program of its own; sanitize: -fsanitize=address,undefined"""
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "needs a host C++ compiler"
    exe = os.path.join(str(out_dir), name + ("_san" if sanitize else ""))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", *flags, "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"),
                    "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_binding_table(tmp_path, sanitize):
    """bind / rebind / unbind / a lookup with another shape at a recycled address / eight threads"""
    r = subprocess.run([_build(tmp_path, "mxfp4_bind_cli", sanitize)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_library_table_through_the_abi():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    codes, other = 0x10000, 0x20000
    assert lib.srgpt_mxfp4_bound(codes) == 0 and lib.srgpt_mxfp4_unbind(codes) == 0
    assert lib.srgpt_mxfp4_bind(codes, None, 16, 128, 0) == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    assert lib.srgpt_mxfp4_bind(None, 0x20, 16, 128, 0) == _lib.ERR_ARG
    assert lib.srgpt_mxfp4_bind(codes, 0x20, 16, 96, 0) == _lib.ERR_ARG and b"multiple of 128" in lib.srgpt_last_error()
    assert lib.srgpt_mxfp4_bind(codes, 0x20, 24, 128, 1) == _lib.ERR_ARG and b"granule" in lib.srgpt_last_error()
    assert lib.srgpt_mxfp4_bind(codes, 0x20, 0, 128, 0) == _lib.ERR_ARG
    assert lib.srgpt_mxfp4_bound(codes) == 0  # a refused bind leaves nothing behind
    assert lib.srgpt_mxfp4_bind(codes, 0x20, 24, 128, 0) == 0 and lib.srgpt_mxfp4_bind(codes, 0x40, 32, 256, 1) == 0  # rebind
    assert lib.srgpt_mxfp4_bound(codes) == 1 and lib.srgpt_mxfp4_bound(other) == 0
    assert lib.srgpt_mxfp4_unbind(codes) == 1 and lib.srgpt_mxfp4_bound(codes) == 0 and lib.srgpt_mxfp4_unbind(codes) == 0
