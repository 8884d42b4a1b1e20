"""CPU: the C surface of prefix reuse (srgpt_rows_match, srgpt_splice_match) -- declared, bound and exported as additions under
ABI 9, and their refusals on the host before any launch (fake non-null pointers that are never dereferenced, in the manner of
tests/test_append_abi.py)."""
import os
import re

from tests.util import ROOT

NEW_SYMBOLS = ("srgpt_rows_match", "srgpt_splice_match")


def test_symbols_are_declared_bound_and_exported():
    import subprocess

    from spatialrgpt_amd import _lib

    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgpt.h")).read(), flags=re.S)
    table = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in table.splitlines() if ln.split()}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and name in exported, name
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert lib.srgpt_abi_version() == _lib.ABI_VERSION == 9  # additions under ABI 9


def test_rows_match_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    ok = dict(a=256, b=512, rows=3, row_bytes=17, out=1024)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.srgpt_rows_match(a["a"], a["b"], a["rows"], a["row_bytes"], a["out"], None)

    for bad in (dict(a=None), dict(b=None), dict(out=None), dict(a=None, rows=0)):
        assert call(**bad) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), bad
    for bad in (dict(rows=-1), dict(rows=-2 ** 31), dict(row_bytes=0), dict(row_bytes=-16), dict(rows=0, row_bytes=0)):
        assert call(**bad) == _lib.ERR_ARG and b"bad shape" in lib.srgpt_last_error(), bad
    assert call(rows=2 ** 31 - 1, row_bytes=2 ** 62) == _lib.ERR_ARG and b"overflows" in lib.srgpt_last_error()


def test_splice_match_refuses_on_the_host():
    from spatialrgpt_amd import _lib

    lib = _lib.load()
    ok = dict(desc_new=256, len_new=5, desc_old=512, n_old_rows=4, gen_old=1024, n_gen_old=3, n_regions_common=1, out=2048)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.srgpt_splice_match(a["desc_new"], a["len_new"], a["desc_old"], a["n_old_rows"], a["gen_old"], a["n_gen_old"],
                                      a["n_regions_common"], a["out"], None)

    for bad in (dict(desc_new=None), dict(desc_old=None), dict(gen_old=None), dict(out=None), dict(desc_new=None, len_new=0)):
        assert call(**bad) == _lib.ERR_ARG and b"null pointer" in lib.srgpt_last_error(), bad
    for bad in (dict(len_new=-1), dict(n_old_rows=-1), dict(n_gen_old=-1), dict(n_regions_common=-1), dict(len_new=-2 ** 31)):
        assert call(**bad) == _lib.ERR_ARG and b"negative length" in lib.srgpt_last_error(), bad
