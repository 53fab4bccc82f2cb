"""cir_check_index / cir_verify_first_dev without a GPU: the declarations in
the header, the ctypes table and INTEGRATION.md's extern block, the argument
checks that need no device, the comparing kernel's resources in the built
code object, and the CLI's usage text.

Reference: commit_image's re-hash loop, src/daemon/disk/commit.rs:51-117.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
from ciruela_amd import _native

NEW = ("cir_verify_first_dev", "cir_check_index")


def _header():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_both():
    text = _header()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
    assert re.search(r"enum cir_check_kind\s*\{\s*CIR_CHECK_OK = 0,\s*CIR_CHECK_CHECKSUM = 1,"
                     r"\s*CIR_CHECK_READ = 2\s*\}", text)
    assert re.search(r"#define CIR_CHECK_STATS_FIELDS 8\b", text)


def test_ctypes_table_binds_both():
    for name in NEW:
        assert name in _native._SIGS
        assert getattr(_native.lib, name).restype is ctypes.c_int
    assert len(_native._SIGS["cir_verify_first_dev"][1]) == 12
    assert len(_native._SIGS["cir_check_index"][1]) == 10
    assert (_native.CIR_CHECK_OK, _native.CIR_CHECK_CHECKSUM, _native.CIR_CHECK_READ) == (0, 1, 2)
    assert _native.CIR_CHECK_STATS_FIELDS == 8


def test_integration_extern_block_names_both():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    assert set(NEW) <= bound


def test_python_interface_exists():
    import ciruela_amd as ca
    assert callable(ca.check_index)
    assert callable(ca.Context.check_index) and callable(ca.Context.verify_first_dev)
    assert "src/daemon/disk/commit.rs:51-117" in ca.__doc__
    r = ca.CheckResult(_native.CIR_CHECK_READ, b"/a", dict(zip(ca.Context.CHECK_STATS_FIELDS,
                                                                [0, 0, 0, 0, 0, 3, 2, 0])))
    assert not r.ok and r.kind == "read" and r.path == b"/a" and r.errno == 2


def _check_index_args():
    kind = ctypes.c_int(77)
    path = ctypes.c_void_p()
    plen = ctypes.c_size_t()
    stats = (ctypes.c_uint64 * 8)()
    return kind, path, plen, stats


def test_check_index_null_arguments():
    lib = _native.lib
    idx = b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n" + b"ab" * 32 + b"\n"
    kind, path, plen, stats = _check_index_args()
    # a null context, before anything else is looked at
    rc = lib.cir_check_index(None, -100, b".", idx, len(idx), 0, ctypes.byref(kind),
                             ctypes.byref(path), ctypes.byref(plen), stats)
    assert rc == _native.CIR_EINVAL
    # (a fake non-null context is never dereferenced before the null checks)
    fake = ctypes.c_void_p(16)
    for args in [
        (fake, -100, b".", None, 0, 0, ctypes.byref(kind), ctypes.byref(path), ctypes.byref(plen),
         stats),
        (fake, -100, b".", idx, len(idx), 0, None, ctypes.byref(path), ctypes.byref(plen), stats),
        (fake, -100, b".", idx, len(idx), 0, ctypes.byref(kind), None, ctypes.byref(plen), stats),
        (fake, -100, b".", idx, len(idx), 0, ctypes.byref(kind), ctypes.byref(path), None, stats),
        (fake, -100, b".", idx, len(idx), 0, ctypes.byref(kind), ctypes.byref(path),
         ctypes.byref(plen), None),
    ]:
        assert lib.cir_check_index(*args) == _native.CIR_EINVAL
        assert b"null" in lib.cir_last_error()


def test_verify_first_dev_argument_checks():
    """The CIR_EINVAL cases of cir_verify_blocks_dev_bounded, all decided
    before any device call: misaligned digest arrays, null pointers."""
    lib = _native.lib
    u64 = (1 << 64) - 1
    ok = dict(ctx=None, ht=1, arena=4096, arena_bytes=u64, off=4096, ln=4096, n=4, exp=4096,
              dig=8192, first=256, nbad=512, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_verify_first_dev(a["ctx"], a["ht"], a["arena"], a["arena_bytes"], a["off"],
                                        a["ln"], a["n"], a["exp"], a["dig"], a["first"],
                                        a["nbad"], a["stream"])
    assert call(exp=4096 + 8) == _native.CIR_EINVAL
    assert b"16-byte aligned" in lib.cir_last_error()
    assert call(dig=8192 + 4) == _native.CIR_EINVAL
    assert call(exp=None) == _native.CIR_EINVAL
    assert call(dig=None) == _native.CIR_EINVAL
    assert call(first=None) == _native.CIR_EINVAL
    assert call(first=260) == _native.CIR_EINVAL
    assert call(ht=9, arena_bytes=1 << 20) == _native.CIR_EINVAL
    assert call(n=1 << 31, arena_bytes=1 << 20) == _native.CIR_EINVAL


@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_first_bad_kernel_resources(tmp_path):
    """k_first_bad is two 16-B loads per operand, a ballot and (in a wave
    with a mismatch) two atomics: no spill, no scratch, no LDS."""
    res = codeobj.resources(str(tmp_path))
    hits = codeobj.find(res, "k_first_bad")
    assert len(hits) == 1, list(hits)
    (k,) = hits.values()
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] == 0
    # k_verify is still one kernel of its own
    assert len(codeobj.find(res, "k_verify")) == 1
    body = next(iter(codeobj.find(codeobj.disassembly(str(tmp_path)), "k_first_bad").values()))
    ops = [ins.split()[0] for ins in body]
    assert sum(o.startswith("global_load_dwordx4") for o in ops) == 4
    assert not any(o.startswith(("scratch_", "ds_")) for o in ops)


def test_cli_usage_lists_check():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index check DIR INDEX_FILE [--disk-threads N]" in p.stderr
    # one positional argument short, and one too many: usage, exit 2
    for args in (["check", "/tmp"], ["check", "/tmp", "a", "b"]):
        p = subprocess.run([cli] + args, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr
