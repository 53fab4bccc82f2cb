"""cir_reload_blocks, cir_copy_runs and cir_copy_runs_dev without a GPU: the
copy and plan rules (ciruela_amd/csrc/copyblk.hpp) under AddressSanitizer and
UBSan (tools/copyblk_fuzz.cpp, a stand-alone program), the host form through
ctypes on the case tables the GPU test uses (tests/reload_restate.py), the
argument checks that need no device, the Python names, and the kernels'
resources in the built code object.

The reference has no counterpart (it holds no image in device memory).  No
expected value comes from the library: the expected buffers are plain slice
copies (reload_restate.CopyCase.expected), indexes are dirsig_oracle's.
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
import reload_restate
from ciruela_amd import _native

NEW = ("cir_reload_blocks", "cir_copy_runs", "cir_copy_runs_dev")


def test_declared_bound_and_documented():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _native._SIGS
        assert getattr(_native.lib, name).restype is ctypes.c_int
    assert re.search(r"#define CIR_RELOAD_STATS_FIELDS 17\b", text)
    assert re.search(r"#define CIR_COPY_RES_FIELDS 1\b", text)
    assert re.search(r"#define CIR_COPY_RUN_WORDS 4\b", text)
    assert re.search(r"#define CIR_FILE_RESIDENT 0x40\b", text)
    assert len(_native._SIGS["cir_reload_blocks"][1]) == 18
    assert (_native.CIR_RELOAD_STATS_FIELDS, _native.CIR_FILE_RESIDENT) == (17, 0x40)
    block = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = block[block.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))


def test_python_interface():
    import ciruela_amd as ca
    assert callable(ca.Context.reload_blocks) and callable(ca.reload_image)
    assert "reload_image" in ca.__all__
    assert len(ca.Context.RELOAD_STATS_FIELDS) == _native.CIR_RELOAD_STATS_FIELDS
    assert ca.Context.RELOAD_STATS_FIELDS[:12] == ca.Context.LOAD_STATS_FIELDS
    assert ca.Context.RELOAD_STATS_FIELDS[12:] == ("copied_blocks", "copied_bytes",
                                                   "resident_blocks", "resident_files",
                                                   "dropped_length")
    stats = dict.fromkeys(ca.Context.RELOAD_STATS_FIELDS, 0)
    index = dirsig_oracle.emit("blake2b/256", 64, [
        (b"/", [("f", b"a", False, 70, dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")),
                ("f", b"b", False, 10, dirsig_oracle.block_hashes(b"y" * 10, 64, "blake2b/256"))])])
    r = ca.BlocksResult(index, 3, b"\x07" + bytes(7),
                        [_native.CIR_FILE_COMPLETE | _native.CIR_FILE_RESIDENT,
                         _native.CIR_FILE_COMPLETE], [0, 0], stats)
    assert r.states == ["complete", "complete"] and r.resident == [True, False]
    assert r.long == [False, False] and r.complete


# ---- the argument checks that need no device ------------------------------------------------

def _reload(ctx, root, index, ptrs, d_have, have_bytes, nhave, ndata=None, stats=True):
    n = len(ptrs)
    d_data = (ctypes.c_void_p * max(n, 1))(*ptrs)
    have, state, errs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    nblk, nfiles = ctypes.c_uint64(), ctypes.c_size_t()
    st = (ctypes.c_uint64 * _native.CIR_RELOAD_STATS_FIELDS)(*([77] * 17))
    keep = ctypes.create_string_buffer(index, max(len(index), 1))
    rc = _native.lib.cir_reload_blocks(ctx, -100, root, keep, len(index), 1, d_data,
                                       n if ndata is None else ndata, d_have, have_bytes, nhave,
                                       None, ctypes.byref(have), ctypes.byref(nblk),
                                       ctypes.byref(state), ctypes.byref(errs),
                                       ctypes.byref(nfiles), st if stats else None)
    assert not have.value and not state.value and not errs.value
    return rc, list(st)


def test_reload_blocks_argument_checks(tmp_path):
    index = dirsig_oracle.emit("blake2b/256", 64, [
        (b"/", [("f", b"a", False, 70, dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")),
                ("f", b"e", False, 0, [])])], keep_empty=True)
    root = os.fsencode(str(tmp_path))
    hex0 = dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")[0].hex().encode()
    # A stand-in handle, as tests/test_load_blocks_cpu.py uses: a context cannot be made without
    # a device, and every case below is decided before the context is read (the header's
    # "before any I/O and any device work").  Zeroed and larger than cir_ctx, so a look at its
    # device list by a reordered check would find an empty list, not foreign memory.
    fake = ctypes.create_string_buffer(4096)
    ptrs = (ctypes.c_void_p * 1)(4096)
    sizes = (ctypes.c_uint64 * 1)(64)
    rc, _ = _reload(fake, root, index, [None, None], None, None, 0, stats=False)
    assert rc == _native.CIR_EINVAL and b"null pointer" in _native.lib.cir_last_error()
    # a resident list without its pointers or without its sizes
    for d_have, have_bytes in ((None, sizes), (ptrs, None), (None, None)):
        rc, stats = _reload(fake, root, index, [None, None], d_have, have_bytes, 1)
        assert rc == _native.CIR_EINVAL and b"null pointer" in _native.lib.cir_last_error()
        assert stats == [0] * 17                   # every stat is written on the way in
    # whatever cir_load_blocks rejects, with the same code: a null context, the parse
    # errors and the ndata check all come before anything asks for a device
    rc, _ = _reload(None, root, index, [None, None], ptrs, sizes, 1)
    assert rc == _native.CIR_EINVAL and b"null pointer" in _native.lib.cir_last_error()
    for bad, code in ((b"", _native.CIR_EPARSE), (index[:40], _native.CIR_EPARSE),
                      (index[:len(index) // 2], _native.CIR_EPARSE),
                      (index.replace(hex0, hex0[:32]), _native.CIR_EHASHSIZE)):
        rc, _ = _reload(fake, root, bad, [None, None], ptrs, sizes, 1)
        assert rc == code, (bad[:40], rc)
    for ndata in (0, 1, 3):
        rc, stats = _reload(fake, root, index, [None] * 3, ptrs, sizes, 1, ndata=ndata)
        assert rc == _native.CIR_EINVAL and b"file entries" in _native.lib.cir_last_error()
        assert stats == [0] * 17


def test_copy_argument_checks():
    lib = _native.lib
    res = (ctypes.c_uint64 * 1)(99)
    src = ctypes.create_string_buffer(64)
    at = ctypes.addressof(src)
    runs = (ctypes.c_uint64 * 4)(0, at, at + 32, 16)
    assert lib.cir_copy_runs(None, 0, 0, None) == _native.CIR_EINVAL
    assert lib.cir_copy_runs(None, 1, 1, res) == _native.CIR_EINVAL
    assert lib.cir_copy_runs(runs, 1 << 32, 1, res) == _native.CIR_EINVAL
    assert lib.cir_copy_runs(runs, 1, (1 << 60) + 1, res) == _native.CIR_EINVAL
    assert res[0] == 99 and src.raw == bytes(64)    # nothing ran
    assert lib.cir_copy_runs(None, 0, 0, res) == 0 and res[0] == 0
    # the device form decides the same, and the alignments, before any HIP call (there is
    # no device here: a HIP call would not return CIR_EINVAL)
    dev = lib.cir_copy_runs_dev
    assert dev(None, None, 1, 1, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 1, 1, None, None) == _native.CIR_EINVAL
    assert dev(None, None, 0, 0, None, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 1 << 32, 1, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096, 1, (1 << 60) + 1, 4096, None) == _native.CIR_EINVAL
    assert dev(None, 4096 + 4, 1, 1, 4096, None) == _native.CIR_EINVAL
    assert b"8-byte" in lib.cir_last_error()
    assert dev(None, 4096, 1, 1, 4096 + 4, None) == _native.CIR_EINVAL
    assert b"8-byte" in lib.cir_last_error()


# ---- the host form on the case tables -------------------------------------------------------

@pytest.mark.parametrize("name", reload_restate.NAMES)
def test_host_form_on_the_case_tables(name):
    """cir_copy_runs inside one buffer with guards between sources and
    destinations: every byte of the buffer is the plain slice copy's (so the
    sources are unchanged and a store outside a run fails), the bad records
    are counted and none of them is written."""
    case = reload_restate.copy_case(name)
    raw = np.full(case.buf_bytes + 16, reload_restate.POISON, dtype=np.uint8)
    skew = -raw.ctypes.data % 16
    buf = raw[skew:skew + case.buf_bytes]
    buf[:] = case.initial
    table = case.table(buf.ctypes.data)
    res = (ctypes.c_uint64 * 1)(12345)
    rc = _native.lib.cir_copy_runs(table.ctypes.data if case.nruns else None, case.nruns,
                                   case.given_nunits, res)
    assert rc == 0, _native.lib.cir_last_error()
    assert res[0] == case.nbad
    diff = np.nonzero(buf != case.expected())[0]
    assert diff.size == 0, (name, diff[:8].tolist())
    assert (raw[:skew] == reload_restate.POISON).all()
    assert (raw[skew + case.buf_bytes:] == reload_restate.POISON).all()


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_copyblk_fuzz_under_asan_ubsan(tmp_path):
    """tools/copyblk_fuzz.cpp: seeded random copy tables over heap buffers of
    exactly their size at every alignment pair, against a byte-by-byte copy;
    damaged tables against a sequential restatement; the plan's rule against a
    block-by-block loop.  A compile failure fails the test."""
    exe = str(tmp_path / "copyblk_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "copyblk_fuzz.cpp"), "-o", exe],
                       capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "1500", "7"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"copyblk_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 1500
    m = re.search(rb"(\d+) records, (\d+) units, (\d+) bytes; (\d+) damaged tables, (\d+) bad "
                  rb"records; (\d+) plan blocks, (\d+) taken, (\d+) dropped", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr


def test_makefile_keeps_the_fuzz_out_of_all():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "build/copyblk_fuzz:" in mk and "copyblk.hip" in mk and "reload.cpp" in mk
    assert "copyblk_fuzz" not in mk[mk.index("\nall:"):].split("\n", 2)[1]
    assert re.search(r"^\.PHONY:.*\bcopyblk_fuzz\b", mk, re.M)


# ---- the kernels in the built code object ---------------------------------------------------

needs_codeobj = pytest.mark.skipif(not codeobj.available(),
                                   reason="needs the built library and llvm-objdump")


@needs_codeobj
def test_kernel_resources(tmp_path):
    res = codeobj.resources(str(tmp_path))
    for name in ("k_copy_runs", "k_copy_plan"):
        hits = codeobj.find(res, name)
        assert len(hits) == 1, (name, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 0, name


@needs_codeobj
def test_kernel_memory_operations(tmp_path):
    """k_copy_runs: no scratch, no LDS, no buffer or flat access; the fast path
    is there (a dwordx4 load and a dwordx4 store) and so are the single-byte
    ends of both ladders; the only atomic is the add of the bad count.
    k_copy_plan: no scratch and no LDS memory; its atomics are counter adds."""
    dis = codeobj.disassembly(str(tmp_path))
    (body,) = codeobj.find(dis, "k_copy_runs").values()
    ops = [ins.split()[0] for ins in body]
    assert not [op for op in ops if op.startswith(("scratch_", "ds_", "buffer_", "flat_"))]
    assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops
    assert "global_load_ubyte" in ops and "global_store_byte" in ops
    assert [op for op in ops if "atomic" in op] == ["global_atomic_add_x2"]
    (body,) = codeobj.find(dis, "k_copy_plan").values()
    ops = [ins.split()[0] for ins in body]
    assert not [op for op in ops if op.startswith(("scratch_", "buffer_", "flat_", "ds_read",
                                                   "ds_write"))]
    assert set(op for op in ops if "atomic" in op) == {"global_atomic_add_x2"}
