"""cir_check_blocks / cir_verify_bitmap_dev without a GPU: the declarations in
the header, the ctypes table and INTEGRATION.md's extern block, the Python
names, BlocksResult over hand-made inputs, the argument checks that need no
device, the CLI's usage text, k_block_bits' resources in the built code
object, and the bit-run copy (ciruela_amd/csrc/bits.hpp) under
AddressSanitizer and UBSan against a bit-by-bit loop (tools/bits_fuzz.cpp, a
stand-alone program).

Reference: the resume that starts over -- "Resuming download"
(src/daemon/tracking/mod.rs:561-585), start_image's removal of the partial
directory (src/daemon/disk/public.rs:91-93) and fill_blocks
(src/daemon/tracking/progress.rs:129-170).  No expected value comes from the
library: indexes are dirsig_oracle.emit's, digests hashlib's, and expected
bitmaps and missing lists tests/blocks_restate.py's.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import blocks_restate
import codeobj
import dirsig_oracle
from ciruela_amd import _native

NEW = ("cir_verify_bitmap_dev", "cir_check_blocks")


def _header():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_both_and_the_constants():
    text = _header()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
    assert re.search(r"#define CIR_BLOCKS_STATS_FIELDS 10\b", text)
    assert re.search(r"#define CIR_FILE_LONG 0x80\b", text)
    enum = re.search(r"enum cir_file_state \{(.*?)\}", text, flags=re.S).group(1)
    assert [re.sub(r"\s", "", t) for t in enum.split(",") if t.strip()] == \
        ["CIR_FILE_COMPLETE=0", "CIR_FILE_ABSENT=1", "CIR_FILE_PARTIAL=2", "CIR_FILE_BLOCKED=3"]


def test_ctypes_table_binds_both():
    for name in NEW:
        assert name in _native._SIGS
        assert getattr(_native.lib, name).restype is ctypes.c_int
    assert len(_native._SIGS["cir_verify_bitmap_dev"][1]) == 12
    assert len(_native._SIGS["cir_check_blocks"][1]) == 12
    assert _native.CIR_BLOCKS_STATS_FIELDS == 10
    assert (_native.CIR_FILE_COMPLETE, _native.CIR_FILE_ABSENT, _native.CIR_FILE_PARTIAL,
            _native.CIR_FILE_BLOCKED, _native.CIR_FILE_LONG) == (0, 1, 2, 3, 0x80)


def test_integration_extern_block_names_both():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    assert set(NEW) <= bound


BS = 64


def _entry(name, data, exe=False):
    return ("f", name, exe, len(data), dirsig_oracle.block_hashes(data, BS, "blake2b/256"))


def test_python_interface_and_blocks_result():
    import ciruela_amd as ca
    assert callable(ca.check_blocks) and callable(ca.Context.check_blocks)
    assert callable(ca.Context.verify_bitmap_dev)
    for name in ("check_blocks", "BlocksResult"):
        assert name in ca.__all__
    for cite in ("src/daemon/tracking/mod.rs:561-585", "src/daemon/disk/public.rs:91-93",
                 "src/daemon/tracking/progress.rs:129-170"):
        assert cite in ca.__doc__
    assert len(ca.Context.BLOCKS_STATS_FIELDS) == _native.CIR_BLOCKS_STATS_FIELDS
    # escaped names, a size-0 file between two others, a symlink, a subdirectory
    index = dirsig_oracle.emit("blake2b/256", BS, [
        (b"/", [_entry(b"a b", b"x" * 130), ("s", b"l", b"a b"), _entry(b"zero", b"")]),
        (b"/d d", [_entry(b"q\\r", b"y" * 64), _entry(b"\xff", b"z" * 4200)])], keep_empty=True)
    nblk = 3 + 0 + 1 + 66
    bits = [1] * nblk
    for g in (1, 3, 4, 4 + 59, 4 + 60, nblk - 1):   # (4 + 60 is bit 0 of the second word)
        bits[g] = 0
    have = blocks_restate.bitmap_bytes(bits)
    assert len(have) == 16
    states = [_native.CIR_FILE_PARTIAL | _native.CIR_FILE_LONG, _native.CIR_FILE_ABSENT,
              _native.CIR_FILE_BLOCKED, _native.CIR_FILE_PARTIAL]
    stats = dict(zip(ca.Context.BLOCKS_STATS_FIELDS, [nblk - 6, 6, 0, 1, 2, 1, 0, 0, 3, 0]))
    r = ca.BlocksResult(index, nblk, have, states, [0, 0, 13, 0], stats)
    assert r.nblk == nblk and r.have == have
    assert [r.has(g) for g in range(nblk)] == [bool(b) for b in bits]
    with pytest.raises(IndexError):
        r.has(nblk)
    assert r.states == ["partial", "absent", "blocked", "partial"]
    assert r.long == [True, False, False, False]
    assert r.errnos == [0, 0, 13, 0] and not r.complete and not r
    want = [(b"/a b", 64), (b"/d d/q\\r", 0), (b"/d d/\xff", 0), (b"/d d/\xff", 59 * 64),
            (b"/d d/\xff", 60 * 64), (b"/d d/\xff", 65 * 64)]
    assert r.missing() == want == blocks_restate.expected_missing(index, bits)
    assert "64 of 70" in repr(r)
    # everything there: complete, nothing missing; the size-0 file takes no bit
    r = ca.BlocksResult(index, nblk, blocks_restate.bitmap_bytes([1] * nblk), [0, 0, 0, 0],
                        [0] * 4, stats)
    assert r.complete and r and r.missing() == []
    # an index of size-0 files only: no blocks, no bitmap
    index = dirsig_oracle.emit("blake2b/256", BS, [(b"/", [_entry(b"e", b"")])], keep_empty=True)
    r = ca.BlocksResult(index, 0, b"", [1], [0], stats)
    assert r.have == b"" and r.states == ["absent"] and r.missing() == [] and not r.complete


INDEX = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  a f 0\n  b f 0\n" + b"ab" * 32 + b"\n")


def _blocks_args(**kw):
    a = dict(ctx=ctypes.c_void_p(16),  # never dereferenced before the argument checks
             fd=-100, dir=b"/nonexistent/image", index=INDEX, len=len(INDEX), threads=0,
             have=ctypes.pointer(ctypes.c_void_p(1)), nblk=ctypes.pointer(ctypes.c_uint64(7)),
             state=ctypes.pointer(ctypes.c_void_p(1)), errs=ctypes.pointer(ctypes.c_void_p(1)),
             nfiles=ctypes.pointer(ctypes.c_size_t(7)), stats=(ctypes.c_uint64 * 10)())
    a.update(kw)
    return [a[k] for k in ("ctx", "fd", "dir", "index", "len", "threads", "have", "nblk", "state",
                           "errs", "nfiles", "stats")]


def test_check_blocks_argument_checks():
    """CIR_EINVAL / CIR_EPARSE / CIR_EHASHSIZE before any I/O and before the
    context is touched: the root named here does not exist and the non-null
    context is not a context."""
    lib = _native.lib
    for null in ("ctx", "index", "have", "nblk", "state", "nfiles", "stats"):
        assert lib.cir_check_blocks(*_blocks_args(**{null: None})) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    # an index that does not parse, with everything else in order; the
    # outputs are cleared all the same
    a = _blocks_args(index=INDEX[:30], len=30)
    assert lib.cir_check_blocks(*a) == _native.CIR_EPARSE
    assert a[6].contents.value is None and a[7].contents.value == 0
    assert a[8].contents.value is None and a[9].contents.value is None and a[10].contents.value == 0
    # errno_out may be NULL: the parse error is still what comes back
    assert lib.cir_check_blocks(*_blocks_args(index=INDEX[:30], len=30, errs=None)) == \
        _native.CIR_EPARSE
    # 16-byte digests: an unsupported hash size
    short = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  f f 10 " + b"ab" * 16 + b"\n" +
             b"ab" * 32 + b"\n")
    assert lib.cir_check_blocks(*_blocks_args(index=short, len=len(short))) in \
        (_native.CIR_EHASHSIZE, _native.CIR_EPARSE)
    md5 = INDEX.replace(b"blake2b/256", b"md5/128")
    assert lib.cir_check_blocks(*_blocks_args(index=md5, len=len(md5))) in \
        (_native.CIR_EHASHSIZE, _native.CIR_EPARSE)


def test_verify_bitmap_dev_argument_checks():
    """The CIR_EINVAL cases, all decided before any device call."""
    lib = _native.lib
    u64 = (1 << 64) - 1
    ok = dict(ctx=None, ht=1, arena=4096, arena_bytes=u64, off=4096, ln=4096, n=4, exp=4096,
              dig=8192, have=1024, nbad=512, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_verify_bitmap_dev(a["ctx"], a["ht"], a["arena"], a["arena_bytes"], a["off"],
                                         a["ln"], a["n"], a["exp"], a["dig"], a["have"], a["nbad"],
                                         a["stream"])
    assert call(have=None) == _native.CIR_EINVAL
    assert b"null" in lib.cir_last_error()
    assert call(have=None, n=0) == _native.CIR_EINVAL
    for mis in (1024 + 1, 1024 + 4):
        assert call(have=mis) == _native.CIR_EINVAL
        assert b"aligned" in lib.cir_last_error()
    assert call(nbad=514) == _native.CIR_EINVAL
    assert call(exp=4096 + 8) == _native.CIR_EINVAL
    assert b"16-byte aligned" in lib.cir_last_error()
    assert call(dig=8192 + 4) == _native.CIR_EINVAL
    assert call(exp=None) == _native.CIR_EINVAL
    assert call(dig=None) == _native.CIR_EINVAL
    assert call(ht=9, arena_bytes=1 << 20) == _native.CIR_EINVAL
    assert call(n=1 << 31, arena_bytes=1 << 20) == _native.CIR_EINVAL


def test_cli_usage_lists_blocks():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index blocks DIR INDEX_FILE [--list]" in p.stderr
    # no index file, and --list on another command: usage, exit 2
    for args in (["blocks", "/tmp"], ["check", "/tmp", "/tmp/x.ds1", "--list"]):
        p = subprocess.run([cli] + args, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr


@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_block_bits_kernel_resources(tmp_path):
    """k_block_bits is k_first_bad's compare (two 16-B loads per operand, two
    ballots) and, in lane 0 of a wave, one 8-byte vector store and at most one
    atomic add to the count: no spill, no scratch, no LDS, and no atomic on
    the bitmap."""
    res = codeobj.resources(str(tmp_path))
    hits = codeobj.find(res, "k_block_bits")
    assert len(hits) == 1, list(hits)
    (k,) = hits.values()
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] == 0
    body = next(iter(codeobj.find(codeobj.disassembly(str(tmp_path)), "k_block_bits").values()))
    ops = [ins.split()[0] for ins in body]
    assert sum(o.startswith("global_load_dwordx4") for o in ops) == 4
    assert sum(o.startswith("global_store_dwordx2") for o in ops) == 1
    assert sum(o.startswith("global_store") for o in ops) == 1
    assert sum(o.startswith("global_atomic") for o in ops) == 1
    assert not any(o.startswith(("scratch_", "ds_")) for o in ops)


def test_bit_run_copy_under_asan_and_ubsan(tmp_path):
    """tools/bits_fuzz.cpp: a few thousand seeded runs of random source
    offset, destination offset and count (0, 1, 63, 64, 65 and runs spanning
    three words among them) against a bit-by-bit loop, the bits outside the
    destination run unchanged, in buffers of exactly the words a run touches.
    A compile failure fails the test."""
    exe = str(tmp_path / "bits_fuzz")
    cxx = os.environ.get("CXX", "g++")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ciruela_amd", "csrc"),
                        os.path.join(ROOT, "tools", "bits_fuzz.cpp"), "-o", exe],
                       capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"bits_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
