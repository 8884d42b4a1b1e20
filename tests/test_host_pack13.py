"""CPU: the lossless 13-bit weight code without a GPU -- the format header (csrc/pack13.h) and the binding table (csrc/pack13_bind.h)
as stand-alone programs, plain and under AddressSanitizer + UBSan; the ABI additions under ABI 9; the packed product's routes."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

from tests.util import ROOT, _build_route_cli

CSRC = os.path.join(ROOT, "spatialrgpt_amd", "csrc")
NEW = ("srgpt_pack13_bytes", "srgpt_pack13", "srgpt_unpack13", "srgpt_gemv_p13", "srgpt_pack13_bind", "srgpt_pack13_unbind",
       "srgpt_pack13_bound")


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
def test_format_round_trips_every_bf16_pattern(tmp_path, sanitize):
    """all 65 536 bit patterns, in windows that code them and in windows that make their row an exception row (below the window,
    zero / denormal, Inf / NaN), and rows of 512, 1024, 2560 and 4096: every row comes back bit for bit"""
    r = subprocess.run([_build(tmp_path, "pack13_cli", sanitize)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    f = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    # 19 filler exponents x 256 exponents + 2 x 4 x 8 random rows; every class occurred
    assert f["rows"] == 19 * 256 + 64 and f["zero"] == 19 and f["special"] == 19 and f["below"] > 1000 and f["coded"] > 1000


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_binding_table(tmp_path, sanitize):
    """bind / rebind / unbind / a lookup with another shape or address / eight threads"""
    r = subprocess.run([_build(tmp_path, "pack13_bind_cli", sanitize)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_abi_additions_under_abi_9():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1)
        assert len(params.split(",")) == len(_lib._SIGNATURES[name][1]), name
    # sizes: ceil(K / 2048) groups of 3328 bytes per row; one flag word per row and the count
    fb = C.c_size_t(0)
    assert lib.srgpt_pack13_bytes(6144, 4096, C.byref(fb)) == 6144 * 6656 and fb.value == 4 * 6145
    assert lib.srgpt_pack13_bytes(4096, 14336, C.byref(fb)) == 4096 * 7 * 3328 and fb.value == 4 * 4097
    assert lib.srgpt_pack13_bytes(10, 512, None) == 10 * 3328 and lib.srgpt_pack13_bytes(10, 2560, None) == 10 * 2 * 3328
    assert lib.srgpt_pack13_bytes(4096, 11008, C.byref(fb)) == 0 and fb.value == 0  # K % 512 != 0: not eligible
    # argument errors are found on the host before any launch
    rc = lib.srgpt_gemv_p13(16, None, 16, 16, None, 0.0, None, 16, 8, 512, 0, 0, None)
    assert rc == _lib.ERR_ARG and b"null" in lib.srgpt_last_error()
    rc = lib.srgpt_gemv_p13(16, 16, 16, 16, None, 0.0, None, 16, 8, 768, 0, 0, None)
    assert rc == _lib.ERR_ARG and b"multiple of 512" in lib.srgpt_last_error()
    rc = lib.srgpt_gemv_p13(16, 16, 16, 16, None, 0.0, 16, 16, 8, 512, 1, 0, None)
    assert rc == _lib.ERR_ARG and b"swiglu" in lib.srgpt_last_error()
    assert lib.srgpt_pack13(16, 8, 768, 16, 16, None) == _lib.ERR_ARG and lib.srgpt_unpack13(16, 16, None, 8, 512, 16, None) == _lib.ERR_ARG
    # the library's table (host only: the addresses are never dereferenced)
    raw, other = 0x10000, 0x20000
    assert lib.srgpt_pack13_bound(raw) == 0 and lib.srgpt_pack13_unbind(raw) == 0
    assert lib.srgpt_pack13_bind(raw, None, 0x30, 8, 512) == _lib.ERR_ARG and lib.srgpt_pack13_bind(raw, 0x20, 0x30, 8, 500) == _lib.ERR_ARG
    assert lib.srgpt_pack13_bound(raw) == 0
    assert lib.srgpt_pack13_bind(raw, 0x20, 0x30, 8, 512) == 0 and lib.srgpt_pack13_bind(raw, 0x40, 0x50, 16, 1024) == 0  # rebind
    assert lib.srgpt_pack13_bound(raw) == 1 and lib.srgpt_pack13_bound(other) == 0
    assert lib.srgpt_pack13_unbind(raw) == 1 and lib.srgpt_pack13_bound(raw) == 0 and lib.srgpt_pack13_unbind(raw) == 0


def test_routes_of_the_four_products(tmp_path):
    """tests/golden/gemv_p13_routes.json: the four streamed products of the decode step (Llama-3-8B geometry) at one row and 256
    CUs, and the shapes that stay raw or get a padded group"""
    exe = _build_route_cli(tmp_path, "gemv_p13_route_cli")
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "gemv_p13_routes.json")))
    assert [t["product"] for t in table[:4]] == ["q/k/v", "gate/up", "down_proj", "lm_head"]
    text = "".join("%d %d %d %d\n" % tuple(t["query"]) for t in table)
    out = subprocess.run([exe, "256"], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert out == [t["answer"] for t in table]


def test_default_products_are_the_measured_ones():
    """what the loader packs by default is what profiles/pack13.txt kept: gate/up and lm_head"""
    from spatialrgpt_amd import weights

    assert weights.PACK13_PRODUCTS == ("wgu", "lm_head") and weights.PACK13_DEFAULT is True
