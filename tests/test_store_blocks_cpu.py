"""cir_store_blocks, cir_gather_runs and cir_gather_runs_dev without a GPU: the
gather rule (ciruela_amd/csrc/gather.hpp) under AddressSanitizer and UBSan
(tools/gather_fuzz.cpp, a stand-alone program), the host form through ctypes
on the edge tables the GPU test uses (tests/gather_cases.py), the argument
checks that need no device, the Python names, and k_gather_runs' resources in
the built code object.

The reference has no counterpart: an image directory is filled block by block
from the network (write_block, src/daemon/disk/public.rs).  No expected value
comes from the library: the expected buffers are plain slice copies
(gather_cases.expected).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import codeobj
import gather_cases
from ciruela_amd import _native

NEW = ("cir_store_blocks", "cir_gather_runs", "cir_gather_runs_dev")


def test_declared_bound_and_documented():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _native._SIGS
        assert getattr(_native.lib, name).restype is ctypes.c_int
    assert re.search(r"#define CIR_STORE_STATS_FIELDS 6\b", text)
    assert re.search(r"#define CIR_GATHER_RES_FIELDS 1\b", text)
    assert re.search(r"#define CIR_GATHER_RUN_WORDS 4\b", text)
    assert len(_native._SIGS["cir_store_blocks"][1]) == 17
    assert len(_native._SIGS["cir_gather_runs"][1]) == 6
    assert len(_native._SIGS["cir_gather_runs_dev"][1]) == 8
    assert (_native.CIR_STORE_STATS_FIELDS, _native.CIR_GATHER_RUN_WORDS,
            _native.CIR_GATHER_RES_FIELDS) == (6, 4, 1)
    block = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = block[block.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))


def test_covered_by_the_typed_abi_test():
    """tests/test_abi_types.py checks every function of the header against the
    ctypes table and INTEGRATION.md's block by type: the new ones are among
    those it parses."""
    import test_abi_types as t
    protos = t.header_prototypes()
    assert set(NEW) <= set(protos)
    assert set(NEW) <= {name for name, _, _ in t.rust_extern_fns()}
    assert protos["cir_gather_runs"] == ("int", ["uint8_t*", "uint64_t", "const uint64_t*",
                                                 "uint64_t", "uint64_t", "uint64_t*"])
    ret, params = protos["cir_store_blocks"]
    assert ret == "int" and len(params) == 17 and params[10] == "const void* const*"


def test_python_interface():
    import ciruela_amd as ca
    assert callable(ca.Context.store_blocks) and callable(ca.store_image)
    assert "store_image" in ca.__all__
    assert len(ca.Context.STORE_STATS_FIELDS) == _native.CIR_STORE_STATS_FIELDS
    assert ca.Context.STORE_STATS_FIELDS == ("blocks", "files", "dirs_made", "bytes", "batches",
                                             "body_bytes")
    with pytest.raises(ValueError):              # neither a root nor a directory fd
        ca.Context.store_blocks(object(), None, [], 4096, ca.HashType.blake2b_256())
    with pytest.raises(TypeError):               # host bytes are no device span
        ca.Context.store_blocks(object(), "/nowhere", [(b"/a", b"host bytes")], 4096,
                                ca.HashType.blake2b_256())


# ---- the argument checks that need no device ------------------------------------------------

def _store(ctx, root, files, bs=4096, ptrs=None):
    """files: [(path, size)]; ptrs default to a made-up non-null address (nothing
    reads it: every case here is refused before any device work)."""
    n = len(files)
    blob = b"".join(p for p, _ in files)
    offs = [0]
    for p, _ in files:
        offs.append(offs[-1] + len(p))
    paths = ctypes.create_string_buffer(blob, max(len(blob), 1))
    path_off = (ctypes.c_uint64 * (n + 1))(*offs)
    sizes = (ctypes.c_uint64 * max(n, 1))(*[s for _, s in files])
    if ptrs is None:
        ptrs = [4096] * n
    d_data = (ctypes.c_void_p * max(n, 1))(*ptrs)
    out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
    iid = ctypes.create_string_buffer(32)
    stats = (ctypes.c_uint64 * _native.CIR_STORE_STATS_FIELDS)(*([77] * 6))
    rc = _native.lib.cir_store_blocks(ctx, -100, root, _native.CIR_HASH_BLAKE2B_256, bs, paths,
                                      path_off, sizes, None, n, d_data, None, 1,
                                      ctypes.byref(out), ctypes.byref(out_len), iid, stats)
    assert not out.value and out_len.value == 0
    return rc, list(stats)


def test_store_blocks_argument_checks(tmp_path):
    root = os.fsencode(str(tmp_path))
    rc, stats = _store(None, root, [(b"/a", 10)])
    assert rc == _native.CIR_EINVAL and b"null ctx" in _native.lib.cir_last_error()
    assert stats == [0] * 6
    # the list is judged before anything needs the context's devices: a stand-in handle is
    # enough (nothing reads it there), and nothing is created below the root
    fake = ctypes.create_string_buffer(4096)
    cases = {
        "conflict": [(b"/a", 10), (b"/a/b", 10)],
        "twice": [(b"/d/a", 10), (b"/d/a", 3)],
        "empty component": [(b"/d//a", 10)],
        "dotdot": [(b"/d/../a", 10)],
        "relative": [(b"d/a", 10)],
    }
    for what, files in cases.items():
        rc, stats = _store(fake, root, files)
        assert rc == _native.CIR_EINVAL, (what, _native.lib.cir_last_error())
        assert stats == [0] * 6, what                    # every stat is written on the way in
        assert os.listdir(tmp_path) == [], what
    rc, stats = _store(fake, root, [(b"/d/a", 10), (b"/d/b", 10), (b"/e", 0)], ptrs=[4096, None, None])
    assert rc == _native.CIR_EINVAL and b"null device pointer" in _native.lib.cir_last_error()
    assert stats == [0] * 6 and os.listdir(tmp_path) == []
    for bs in (0, 1 << 32):
        rc, stats = _store(fake, root, [(b"/a", 10)], bs=bs)
        assert rc == _native.CIR_EINVAL and b"block_size" in _native.lib.cir_last_error()
        assert stats == [0] * 6 and os.listdir(tmp_path) == []


def test_gather_argument_checks():
    lib = _native.lib
    res = (ctypes.c_uint64 * 1)(99)
    runs = (ctypes.c_uint64 * 4)(0, 0, 0, 16)
    dst = ctypes.create_string_buffer(64)
    big = 1 << 32
    assert lib.cir_gather_runs(None, 0, None, 0, 0, None) == _native.CIR_EINVAL
    assert lib.cir_gather_runs(None, 16, runs, 1, 1, res) == _native.CIR_EINVAL
    assert lib.cir_gather_runs(dst, 16, None, 1, 1, res) == _native.CIR_EINVAL
    assert lib.cir_gather_runs(dst, 16, runs, big, 1, res) == _native.CIR_EINVAL
    assert lib.cir_gather_runs(dst, 16, runs, 1, big, res) == _native.CIR_EINVAL
    assert lib.cir_gather_runs(None, 0, None, 0, 0, res) == 0 and res[0] == 0
    # the device form decides the same, and the alignments, before any HIP call (there is
    # no device here: a HIP call would not return CIR_EINVAL)
    dev = lib.cir_gather_runs_dev
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


# ---- the host form on the edge tables ----------------------------------------------------------

@pytest.mark.parametrize("name", gather_cases.NAMES)
def test_host_form_on_the_edge_tables(name):
    """cir_gather_runs into one poisoned buffer from sources of every alignment:
    every byte of the buffer is the plain slice copy's -- the pad bytes of sound
    records 0, the bytes no unit covers still the poison --, the bad records are
    counted and leave no trace, and the sources are unchanged."""
    case = gather_cases.build(name)
    raw = np.full(len(case.src) + 16, gather_cases.POISON, dtype=np.uint8)
    skew = -raw.ctypes.data % 16                   # (the sources' alignments are the case's)
    src = raw[skew:skew + len(case.src)]
    src[:] = case.src
    table = case.table(src.ctypes.data)
    draw = np.full(case.buf_bytes + 16, gather_cases.POISON, dtype=np.uint8)
    dskew = -draw.ctypes.data % 16
    buf = draw[dskew:dskew + case.buf_bytes]
    res = (ctypes.c_uint64 * 1)(12345)
    rc = _native.lib.cir_gather_runs(buf.ctypes.data if case.nunits else None, case.dst_bytes,
                                     table.ctypes.data if len(table) else None, case.nruns,
                                     case.nunits, res)
    assert rc == 0, _native.lib.cir_last_error()
    assert res[0] == case.nbad
    want = gather_cases.expected(case)
    diff = np.nonzero(buf != want)[0]
    assert diff.size == 0, (name, diff[:8].tolist())
    assert (src == case.src).all()


def test_the_cases_are_not_trivial():
    c = gather_cases.build("mixed")
    assert {r[2] % 16 for r in c.recs} == set(range(16))
    assert {r[3] for r in c.recs} == set(gather_cases.LENS) and c.nunits > 4 * 256
    assert [gather_cases.build(n).nruns for n in ("empty", "one", "two", "hundred", "thousand")] \
        == [0, 1, 2, 128, 1000]
    m = gather_cases.build("malformed")
    want = gather_cases.expected(m)
    assert m.nbad == 12 and (want == 0).any() and (want == gather_cases.POISON).any()


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_gather_fuzz_under_asan_ubsan(tmp_path):
    """tools/gather_fuzz.cpp: seeded random files through pack_run, their
    records through apply_host from sources of every alignment between redzones
    into a slot between redzones, against a byte-by-byte restatement; damaged
    tables against a sequential restatement.  A compile failure fails the
    test."""
    exe = str(tmp_path / "gather_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "gather_fuzz.cpp"), "-o", exe],
                       capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "1500", "7"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"gather_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 1500
    m = re.search(rb"(\d+) files, (\d+) batches, (\d+) records, (\d+) units, (\d+) bytes; (\d+) "
                  rb"damaged tables, (\d+) bad records", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "build/gather_fuzz:" in mk and "gather.hip" in mk and "store.cpp" in mk
    assert "gather_fuzz" not in mk[mk.index("\nall:"):].split("\n", 2)[1]   # not in `all`


# ---- the kernel in the built code object ----------------------------------------------------------

needs_codeobj = pytest.mark.skipif(not codeobj.available(),
                                   reason="needs the built library and llvm-objdump")


@needs_codeobj
def test_kernel_resources(tmp_path):
    res = codeobj.resources(str(tmp_path))
    hits = codeobj.find(res, "k_gather_runs")
    assert len(hits) == 1, list(hits)
    (k,) = hits.values()
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] == 0


@needs_codeobj
def test_kernel_memory_operations(tmp_path):
    """The fast path is there: a dwordx4 load and the dwordx4 store."""
    dis = codeobj.disassembly(str(tmp_path))
    hits = codeobj.find(dis, "k_gather_runs")
    assert len(hits) == 1, list(hits)
    (body,) = hits.values()
    ops = [ins.split()[0] for ins in body]
    assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops
    assert "global_load_ubyte" in ops                      # the narrow path of odd sources
