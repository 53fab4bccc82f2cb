"""cir_load_blocks, cir_scatter_runs and cir_scatter_runs_dev without a GPU:
the scatter rule (ciruela_amd/csrc/scatter.hpp) under AddressSanitizer and
UBSan (tools/scatter_fuzz.cpp, a stand-alone program), the host form through
ctypes on the edge table the GPU test uses (tests/scatter_cases.py), the
argument checks that need no device, the Python names, and k_scatter_runs'
resources in the built code object.

The reference has no counterpart: its consumers read committed files from disk
(commit_image, src/daemon/disk/commit.rs:51-117, is the last look at the
bytes).  No expected value comes from the library: the expected buffers are
plain slice copies (scatter_cases.expected), indexes are dirsig_oracle's.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import codeobj
import dirsig_oracle
import scatter_cases
from ciruela_amd import _native

NEW = ("cir_load_blocks", "cir_scatter_runs", "cir_scatter_runs_dev")


def test_declared_bound_and_documented():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _native._SIGS
        assert getattr(_native.lib, name).restype is ctypes.c_int
    assert re.search(r"#define CIR_LOAD_STATS_FIELDS 12\b", text)
    assert re.search(r"#define CIR_SCATTER_RES_FIELDS 1\b", text)
    assert re.search(r"#define CIR_SCATTER_RUN_WORDS 4\b", text)
    assert re.search(r"#define CIR_FILE_SKIPPED 4\b", text)
    assert len(_native._SIGS["cir_load_blocks"][1]) == 15
    assert (_native.CIR_LOAD_STATS_FIELDS, _native.CIR_FILE_SKIPPED) == (12, 4)
    block = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = block[block.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))


def test_python_interface():
    import ciruela_amd as ca
    assert callable(ca.Context.load_blocks) and callable(ca.load_image)
    assert "load_image" in ca.__all__
    assert len(ca.Context.LOAD_STATS_FIELDS) == _native.CIR_LOAD_STATS_FIELDS
    assert ca.Context.LOAD_STATS_FIELDS[:10] == ca.Context.BLOCKS_STATS_FIELDS
    assert ca.Context.LOAD_STATS_FIELDS[10:] == ("scattered_bytes", "skipped")
    stats = dict.fromkeys(ca.Context.LOAD_STATS_FIELDS, 0)
    index = dirsig_oracle.emit("blake2b/256", 64, [
        (b"/", [("f", b"a", False, 70, dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")),
                ("f", b"b", False, 10, dirsig_oracle.block_hashes(b"y" * 10, 64, "blake2b/256"))])])
    r = ca.BlocksResult(index, 3, b"\x03" + bytes(7), [_native.CIR_FILE_COMPLETE,
                                                      _native.CIR_FILE_SKIPPED], [0, 0], stats)
    assert r.states == ["complete", "skipped"] and r.long == [False, False]
    assert not r.complete and r.missing() == [(b"/b", 0)]


def test_short_buffer_is_a_value_error():
    """A span shorter than its entry is refused before the call (no context is
    touched: the object passed as one has no handle)."""
    import ciruela_amd as ca
    index = dirsig_oracle.emit("blake2b/256", 64, [
        (b"/", [("f", b"a", False, 70, dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256"))])])
    with pytest.raises(ValueError):
        ca.Context.load_blocks(object(), "/nowhere", index, [(4096, 69)])
    with pytest.raises(TypeError):
        ca.Context.load_blocks(object(), "/nowhere", index, [b"host bytes"])


# ---- the argument checks that need no device ------------------------------------------------

def _load(ctx, root, index, ptrs, ndata=None):
    n = len(ptrs)
    d_data = (ctypes.c_void_p * max(n, 1))(*ptrs)
    have, state, errs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    nblk, nfiles = ctypes.c_uint64(), ctypes.c_size_t()
    stats = (ctypes.c_uint64 * _native.CIR_LOAD_STATS_FIELDS)(*([77] * 12))
    rc = _native.lib.cir_load_blocks(ctx, -100, root, index, len(index), 1, d_data,
                                     n if ndata is None else ndata, None, ctypes.byref(have),
                                     ctypes.byref(nblk), ctypes.byref(state), ctypes.byref(errs),
                                     ctypes.byref(nfiles), stats)
    assert not have.value and not state.value and not errs.value
    return rc, list(stats)


def test_load_blocks_argument_checks(tmp_path):
    index = dirsig_oracle.emit("blake2b/256", 64, [
        (b"/", [("f", b"a", False, 70, dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")),
                ("f", b"e", False, 0, [])])], keep_empty=True)
    root = os.fsencode(str(tmp_path))
    hex0 = dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")[0].hex().encode()
    assert hex0 in index
    rc, _ = _load(None, root, index, [None, None])
    assert rc == _native.CIR_EINVAL and b"null pointer" in _native.lib.cir_last_error()
    # the parse comes before everything that needs the context's devices: a stand-in
    # handle is enough to see the parse errors and the ndata check (nothing reads it there)
    fake = ctypes.create_string_buffer(4096)
    for bad, code in ((b"", _native.CIR_EPARSE), (index[:40], _native.CIR_EPARSE),
                      (index[:len(index) // 2], _native.CIR_EPARSE),
                      (index.replace(hex0, hex0[:32]), _native.CIR_EHASHSIZE)):
        keep = ctypes.create_string_buffer(bad, max(len(bad), 1))
        d_data = (ctypes.c_void_p * 2)()
        out = [ctypes.c_void_p() for _ in range(3)]
        nblk, nfiles = ctypes.c_uint64(), ctypes.c_size_t()
        stats = (ctypes.c_uint64 * 12)()
        rc = _native.lib.cir_load_blocks(fake, -100, root, keep, len(bad), 1, d_data, 2, None,
                                         ctypes.byref(out[0]), ctypes.byref(nblk),
                                         ctypes.byref(out[1]), ctypes.byref(out[2]),
                                         ctypes.byref(nfiles), stats)
        want = _native.lib.cir_check_blocks(fake, -100, root, keep, len(bad), 1,
                                            ctypes.byref(out[0]), ctypes.byref(nblk),
                                            ctypes.byref(out[1]), ctypes.byref(out[2]),
                                            ctypes.byref(nfiles), stats)
        assert rc == want == code, (bad[:40], rc, want)
    for ndata in (0, 1, 3):
        rc, stats = _load(fake, root, index, [None] * 3, ndata=ndata)
        assert rc == _native.CIR_EINVAL and b"file entries" in _native.lib.cir_last_error()
        assert stats == [0] * 12                  # every stat is written on the way in


def test_scatter_argument_checks():
    lib = _native.lib
    res = (ctypes.c_uint64 * 1)(99)
    runs = (ctypes.c_uint64 * 4)(0, 0, 0, 16)
    src = ctypes.create_string_buffer(64)
    big = 1 << 32
    assert lib.cir_scatter_runs(None, 0, None, 0, 0, None) == _native.CIR_EINVAL
    assert lib.cir_scatter_runs(None, 16, runs, 1, 1, res) == _native.CIR_EINVAL
    assert lib.cir_scatter_runs(src, 16, None, 1, 1, res) == _native.CIR_EINVAL
    assert lib.cir_scatter_runs(src, 16, runs, big, 1, res) == _native.CIR_EINVAL
    assert lib.cir_scatter_runs(src, 16, runs, 1, big, res) == _native.CIR_EINVAL
    assert lib.cir_scatter_runs(None, 0, None, 0, 0, res) == 0 and res[0] == 0
    # the device form decides the same, and the alignments, before any HIP call (there is
    # no device here: a HIP call would not return CIR_EINVAL)
    dev = lib.cir_scatter_runs_dev
    assert dev(None, None, 16, 4096, 1, 1, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 16, None, 1, 1, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 16, 4096, 1, 1, None, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 16, 4096, big, 1, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 16, 4096, 1, big, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096 + 8, 16, 4096, 1, 1, 4096, None) == _native.CIR_EINVAL
    assert b"16-byte" in lib.cir_last_error()
    assert dev(None, 4096, 16, 4096 + 4, 1, 1, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 16, 4096, 1, 1, 4096 + 4, None) == _native.CIR_EINVAL
    assert b"8-byte" in lib.cir_last_error()


# ---- the host form on the edge table -----------------------------------------------------------

@pytest.mark.parametrize("name", scatter_cases.NAMES)
def test_host_form_on_the_edge_tables(name):
    """cir_scatter_runs into one poisoned buffer with guards between the
    destinations: every byte of the buffer is the plain slice copy's, the bad
    records are counted and none of them is written."""
    case = scatter_cases.build(name)
    raw = np.full(case.buf_bytes + 16, scatter_cases.POISON, dtype=np.uint8)
    skew = -raw.ctypes.data % 16                   # (the destinations' alignments are the case's)
    buf = raw[skew:skew + case.buf_bytes]
    table = case.table(buf.ctypes.data)
    res = (ctypes.c_uint64 * 1)(12345)
    rc = _native.lib.cir_scatter_runs(case.src.ctypes.data, case.src_bytes,
                                      table.ctypes.data if len(table) else None, case.nruns,
                                      case.nunits, res)
    assert rc == 0, _native.lib.cir_last_error()
    assert res[0] == case.nbad
    want = scatter_cases.expected(case)
    diff = np.nonzero(buf != want)[0]
    assert diff.size == 0, (name, diff[:8].tolist())


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_scatter_fuzz_under_asan_ubsan(tmp_path):
    """tools/scatter_fuzz.cpp: seeded random files through pack_run and
    cut_pieces, their records through apply_host into destinations of every
    alignment between redzones, against a byte-by-byte copy; damaged tables
    against a sequential restatement.  A compile failure fails the test."""
    exe = str(tmp_path / "scatter_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "scatter_fuzz.cpp"), "-o", exe],
                       capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "1500", "7"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"scatter_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 1500
    m = re.search(rb"(\d+) files, (\d+) batches, (\d+) records, (\d+) units, (\d+) bytes; (\d+) "
                  rb"damaged tables, (\d+) bad records", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "build/scatter_fuzz:" in mk and "scatter.hip" in mk
    assert "scatter_fuzz" not in mk[mk.index("\nall:"):].split("\n", 2)[1]   # not in `all`


# ---- the kernel in the built code object ----------------------------------------------------------

needs_codeobj = pytest.mark.skipif(not codeobj.available(),
                                   reason="needs the built library and llvm-objdump")


@needs_codeobj
def test_kernel_resources(tmp_path):
    res = codeobj.resources(str(tmp_path))
    hits = codeobj.find(res, "k_scatter_runs")
    assert len(hits) == 1, list(hits)
    (k,) = hits.values()
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] == 0


@needs_codeobj
def test_kernel_memory_operations(tmp_path):
    """No scratch, no LDS, no buffer or flat access; the fast path is there (a
    dwordx4 load and a dwordx4 store); the only atomic is the add of the bad
    count."""
    dis = codeobj.disassembly(str(tmp_path))
    hits = codeobj.find(dis, "k_scatter_runs")
    assert len(hits) == 1, list(hits)
    (body,) = hits.values()
    ops = [ins.split()[0] for ins in body]
    assert not [op for op in ops if op.startswith(("scratch_", "ds_", "buffer_", "flat_"))]
    assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops
    assert "global_store_byte" in ops                      # the narrow path of odd destinations
    assert [op for op in ops if "atomic" in op] == ["global_atomic_add_x2"]
