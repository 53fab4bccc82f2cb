"""cir_update_blocks without a GPU: the rule (ciruela_amd/csrc/update.hpp) under
AddressSanitizer and UBSan (tools/update_fuzz.cpp, a stand-alone program), the
argument checks that need no device, the Python names, and the plan kernels'
resources in the built code object.

The reference has no counterpart (it holds no image in device memory).  No
expected value comes from the library.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
import dirsig_oracle
from ciruela_amd import _native

NAME = "cir_update_blocks"
NSTATS = 22


def test_declared_bound_and_documented():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, text)
    assert NAME in _native._SIGS
    assert getattr(_native.lib, NAME).restype is ctypes.c_int
    assert re.search(r"#define CIR_UPDATE_STATS_FIELDS 22\b", text)
    # cir_reload_blocks' arguments and the scratch cap
    assert len(_native._SIGS[NAME][1]) == len(_native._SIGS["cir_reload_blocks"][1]) + 1 == 19
    assert _native._SIGS[NAME][1][11] is ctypes.c_uint64
    assert _native.CIR_UPDATE_STATS_FIELDS == NSTATS
    block = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    steps = block[block.index("## 3. Call-site changes"):]
    block = block[block.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert NAME in re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block)
    assert NAME in steps


def test_python_interface():
    import ciruela_amd as ca
    assert callable(ca.Context.update_blocks) and callable(ca.update_image)
    assert "update_image" in ca.__all__
    assert len(ca.Context.UPDATE_STATS_FIELDS) == NSTATS
    assert ca.Context.UPDATE_STATS_FIELDS[:17] == ca.Context.RELOAD_STATS_FIELDS
    assert ca.Context.UPDATE_STATS_FIELDS[17:] == ("kept_blocks", "kept_bytes", "staged_blocks",
                                                   "scratch_bytes", "demoted_blocks")
    import inspect
    sig = inspect.signature(ca.Context.update_blocks)
    assert list(sig.parameters) == ["self", "root", "index", "buffers", "resident",
                                    "scratch_bytes", "threads", "dir_fd", "stream"]
    assert sig.parameters["scratch_bytes"].default is None
    sig = inspect.signature(ca.update_image)
    assert list(sig.parameters) == ["root", "index", "held", "context", "only", "threads",
                                    "scratch_bytes"]


# ---- the argument checks that need no device ------------------------------------------------

def _update(ctx, root, index, ptrs, d_have, have_bytes, nhave, ndata=None, stats=True,
            scratch=(1 << 64) - 1):
    n = len(ptrs)
    d_data = (ctypes.c_void_p * max(n, 1))(*ptrs)
    have, state, errs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    nblk, nfiles = ctypes.c_uint64(), ctypes.c_size_t()
    st = (ctypes.c_uint64 * NSTATS)(*([77] * NSTATS))
    keep = ctypes.create_string_buffer(index, max(len(index), 1))
    rc = _native.lib.cir_update_blocks(ctx, -100, root, keep, len(index), 1, d_data,
                                       n if ndata is None else ndata, d_have, have_bytes, nhave,
                                       scratch, None, ctypes.byref(have), ctypes.byref(nblk),
                                       ctypes.byref(state), ctypes.byref(errs),
                                       ctypes.byref(nfiles), st if stats else None)
    assert not have.value and not state.value and not errs.value
    return rc, list(st)


def test_update_blocks_argument_checks(tmp_path):
    index = dirsig_oracle.emit("blake2b/256", 64, [
        (b"/", [("f", b"a", False, 70, dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")),
                ("f", b"b", False, 70, dirsig_oracle.block_hashes(b"y" * 70, 64, "blake2b/256")),
                ("f", b"e", False, 0, [])])], keep_empty=True)
    root = os.fsencode(str(tmp_path))
    hex0 = dirsig_oracle.block_hashes(b"x" * 70, 64, "blake2b/256")[0].hex().encode()
    # A stand-in handle, as tests/test_reload_blocks_cpu.py uses: a context cannot be made
    # without a device.  Zeroed and larger than cir_ctx, so a look at its device list finds an
    # empty list, not foreign memory.
    fake = ctypes.create_string_buffer(4096)
    ptrs = (ctypes.c_void_p * 2)(4096, 8192)
    sizes = (ctypes.c_uint64 * 2)(64, 64)
    none3 = [None, None, None]
    rc, _ = _update(fake, root, index, none3, None, None, 0, stats=False)
    assert rc == _native.CIR_EINVAL and b"null pointer" in _native.lib.cir_last_error()
    # a resident list without its pointers or without its sizes
    for d_have, have_bytes in ((None, sizes), (ptrs, None), (None, None)):
        rc, stats = _update(fake, root, index, none3, d_have, have_bytes, 2)
        assert rc == _native.CIR_EINVAL and b"null pointer" in _native.lib.cir_last_error()
        assert stats == [0] * NSTATS                # every stat is written on the way in
    # whatever cir_load_blocks rejects, with the same code
    rc, _ = _update(None, root, index, none3, ptrs, sizes, 2)
    assert rc == _native.CIR_EINVAL and b"null pointer" in _native.lib.cir_last_error()
    for bad, code in ((b"", _native.CIR_EPARSE), (index[:40], _native.CIR_EPARSE),
                      (index[:len(index) // 2], _native.CIR_EPARSE),
                      (index.replace(hex0, hex0[:32]), _native.CIR_EHASHSIZE)):
        rc, _ = _update(fake, root, bad, none3, ptrs, sizes, 2)
        assert rc == code, (bad[:40], rc)
    for ndata in (0, 2, 4):
        rc, stats = _update(fake, root, index, [None] * 4, ptrs, sizes, 2, ndata=ndata)
        assert rc == _native.CIR_EINVAL and b"file entries" in _native.lib.cir_last_error()
        assert stats == [0] * NSTATS
    # two resident buffers that overlap one another: by one byte, nested, identical -- decided
    # before the index is read, whatever the order of the list; neighbours that touch are fine
    # (the call then goes on to the stand-in's missing device)
    for a, b, over in (((4096, 64), (4159, 64), True), ((4159, 64), (4096, 64), True),
                       ((4096, 640), (4200, 8), True), ((4096, 64), (4096, 64), True),
                       ((4096, 64), (4160, 64), False), ((4096, 0), (4096, 64), False)):
        p2 = (ctypes.c_void_p * 2)(a[0], b[0])
        s2 = (ctypes.c_uint64 * 2)(a[1], b[1])
        rc, stats = _update(fake, root, index, none3, p2, s2, 2)
        assert rc == _native.CIR_EINVAL and stats == [0] * NSTATS
        assert (b"resident buffers overlap" in _native.lib.cir_last_error()) == over, (a, b)
    # two destinations that overlap one another are CIR_EINVAL too.  Which device the stream
    # belongs to is asked first, and the stand-in has none, so here only the code can be
    # seen; the message is tests/test_gpu_update_blocks.py's, and the decision itself
    # (update::spans_overlap) runs against all pairs in tools/update_fuzz.cpp
    rc, stats = _update(fake, root, index, [1 << 20, (1 << 20) + 69, None], ptrs, sizes, 2)
    assert rc == _native.CIR_EINVAL and stats == [0] * NSTATS


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_update_fuzz_under_asan_ubsan(tmp_path):
    """tools/update_fuzz.cpp: seeded random layouts in one heap arena --
    destinations identical to, shifted against, partly over and clear of the
    resident buffers --, update::plan_host and the two copies against a
    block-by-block model from a snapshot.  A compile failure fails the test."""
    exe = str(tmp_path / "update_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "update_fuzz.cpp"), "-o", exe],
                       capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "1500", "7"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"update_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 1500
    m = re.search(rb"(\d+) blocks; (\d+) kept, (\d+) direct, (\d+) staged, (\d+) demoted, (\d+) "
                  rb"dropped", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr


def test_makefile_keeps_the_fuzz_out_of_all():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "build/update_fuzz:" in mk and "update.hip" in mk and "update.cpp" in mk
    assert "update_fuzz" not in mk[mk.index("\nall:"):].split("\n", 2)[1]
    assert re.search(r"^\.PHONY:.*\bupdate_fuzz\b", mk, re.M)
    assert re.search(r"^sanitizers:.*\bupdate_fuzz\b", mk, re.M)


# ---- the kernels in the built code object ---------------------------------------------------

needs_codeobj = pytest.mark.skipif(not codeobj.available(),
                                   reason="needs the built library and llvm-objdump")


@needs_codeobj
def test_kernel_resources(tmp_path):
    res = codeobj.resources(str(tmp_path))
    for name in ("k_update_plan", "k_update_emit"):
        hits = codeobj.find(res, name)
        assert len(hits) == 1, (name, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 0, name
    assert len(codeobj.find(res, "k_update_scan")) == 1
