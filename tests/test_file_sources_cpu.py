"""cir_file_sources / cir_index_files_dev / cir_match_files_dev without a GPU:
the declarations in the header, the ctypes table, INTEGRATION.md's extern
block and the Python interface; the argument checks of the two *_dev calls
(all CIR_EINVAL cases are decided before any device call); cir_file_sources
with ctx = NULL against cir_link_candidates and the restatement of scan_links
(tests/links_restate.py; src/daemon/metadata/hardlink_sources.rs:107-153) on
the families of tests/files_cases.py; a sanitized fuzz of the shared rule
header (tools/files_fuzz.cpp, a stand-alone program); and the new kernels'
resources in the built code object.  No expected value comes from the library.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
import files_cases
import links_restate
from ciruela_amd import _native

NEW = ("cir_index_files_work_bytes", "cir_index_files_dev", "cir_match_files_work_bytes",
       "cir_match_files_dev", "cir_file_sources")
KERNELS = ("k_files_count", "k_files_scan", "k_files_emit", "k_files_tokens", "k_files_fold", "k_files_build",
           "k_files_probe", "k_files_verify")


# ---- declarations and bindings ---------------------------------------------------------

def test_header_declares_the_calls():
    full = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|uint64_t) %s\s*\(" % name, text), name
    assert re.search(r"#define CIR_FILE_WORDS 4\b", text)
    assert re.search(r"#define CIR_FILES_RES_FIELDS 4\b", text)
    assert re.search(r"#define CIR_FILE_SOURCES_STATS_FIELDS 8\b", text)
    assert "CIR_LINKS_MATCH=host" in full[:full.index("#ifndef CIRUELA_BLOCKHASH_H")]


def test_ctypes_table_binds_the_calls():
    for name in NEW:
        assert name in _native._SIGS
    assert len(_native._SIGS["cir_index_files_dev"][1]) == 14
    assert len(_native._SIGS["cir_match_files_dev"][1]) == 24
    assert len(_native._SIGS["cir_file_sources"][1]) == len(_native._SIGS["cir_link_candidates"][1]) + 2
    assert _native.lib.cir_index_files_work_bytes.restype is ctypes.c_uint64
    assert (_native.CIR_FILE_WORDS, _native.CIR_FILES_RES_FIELDS,
            _native.CIR_FILE_SOURCES_STATS_FIELDS) == (4, 4, 8)


def test_integration_extern_block_names_the_calls():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))


def test_python_interface_exists():
    import ciruela_amd as ca
    assert callable(ca.file_sources) and "file_sources" in ca.__all__
    assert callable(ca.Context.index_files_dev) and callable(ca.Context.match_files_dev)
    assert "file_sources" in ca.__doc__


def test_work_bytes_are_pure():
    lib = _native.lib
    tile = lib.cir_debug_index_tile_bytes()
    f = lib.cir_index_files_work_bytes
    assert f(0) == 64 and f(tile) == 96 and f(10 * tile + 1) == 32 * 12
    g = lib.cir_match_files_work_bytes
    assert g(0, 0) == 4 * lib.cir_match_table_slots(0)
    assert g(10, 32) == 16 * 42 + 4 * 64 and g(10, 33) == 16 * 43 + 4 * 128
    assert g(1 << 32, 1) == 0 and g(1, 1 << 31) == 0


def test_index_files_dev_argument_checks():
    lib = _native.lib
    ok = dict(text=1 << 20, len=10000, b0=40, b1=9000, bs=4096, ob=0, bb=0, files=1 << 22,
              cap=1250, work=1 << 23, wb=lib.cir_index_files_work_bytes(10000), res=1 << 24,
              stream=None)
    order = ("text", "len", "b0", "b1", "bs", "ob", "bb", "files", "cap", "work", "wb", "res",
             "stream")

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_index_files_dev(None, *[a[k] for k in order])
    for null in ("text", "files", "work", "res"):
        assert call(**{null: None}) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    for odd in ("text", "files", "work", "res"):
        assert call(**{odd: ok[odd] + 4}) == _native.CIR_EINVAL, odd
        assert b"8-byte aligned" in lib.cir_last_error()
    assert call(b0=9001) == _native.CIR_EINVAL
    assert call(b1=10001) == _native.CIR_EINVAL
    assert call(bs=0) == _native.CIR_EINVAL
    assert call(wb=ok["wb"] - 1) == _native.CIR_EINVAL
    assert b"cir_index_files_work_bytes" in lib.cir_last_error()
    assert call(len=(1 << 36) + 1, b1=9000,
                wb=lib.cir_index_files_work_bytes((1 << 36) + 1)) == _native.CIR_EINVAL
    assert call(cap=(1 << 58) + 1) == _native.CIR_EINVAL


def test_match_files_dev_argument_checks():
    lib = _native.lib
    ok = dict(nt=1 << 20, ntl=5000, nf=1 << 21, nnf=10, nd=1 << 22, nnb=30,
              pt=1 << 20, ptl=5000, pf=1 << 23, pnf=20, pd=1 << 24, pnb=60,
              first=1 << 25, nsrc=2, bs=64, verify=None, seed=1, work=1 << 26,
              wb=lib.cir_match_files_work_bytes(10, 20), csrc=1 << 27, cfile=1 << 28,
              res=1 << 29, stream=None)
    order = tuple(ok)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_match_files_dev(None, *[a[k] for k in order])
    for null in ("nt", "nf", "nd", "pt", "pf", "pd", "first", "work", "csrc", "cfile", "res"):
        assert call(**{null: None}) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    for odd in ("nd", "pd"):
        assert call(**{odd: ok[odd] + 8}) == _native.CIR_EINVAL
        assert b"16-byte aligned" in lib.cir_last_error()
    assert call(verify=(1 << 30) + 8) == _native.CIR_EINVAL
    for odd in ("nf", "pf", "first", "work", "cfile", "res"):
        assert call(**{odd: ok[odd] + 4}) == _native.CIR_EINVAL, odd
    assert call(csrc=ok["csrc"] + 2) == _native.CIR_EINVAL
    assert call(bs=0) == _native.CIR_EINVAL
    assert call(wb=ok["wb"] - 1) == _native.CIR_EINVAL
    assert call(pnf=1 << 31, wb=1 << 62) == _native.CIR_EINVAL
    assert call(nnf=1 << 32, wb=1 << 62) == _native.CIR_EINVAL
    assert call(nnb=1 << 32) == _native.CIR_EINVAL
    # (empty sides need no arrays)
    assert call(nnf=0, nnb=0, nt=None, nf=None, nd=None, csrc=None, cfile=None,
                wb=0) == _native.CIR_EINVAL        # ... but the scratch is never empty
    assert b"work_bytes" in lib.cir_last_error()


# ---- the host path ------------------------------------------------------------------------

def raw_call(index, sources, ctx=None):
    """cir_file_sources through ctypes: (status, pairs, skipped, stats)."""
    lib = _native.lib
    bufs = [ctypes.create_string_buffer(s, max(len(s), 1)) for s in sources]
    n = max(len(sources), 1)
    sp = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * n)(*[len(s) for s in sources])
    f, s, cnt, sk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(77)
    stats = (ctypes.c_uint64 * 8)(*([99] * 8))
    rc = lib.cir_file_sources(ctx, index, len(index), sp, sl, len(sources), ctypes.byref(f),
                              ctypes.byref(s), ctypes.byref(cnt), ctypes.byref(sk), stats)
    pairs = []
    if rc == 0 and cnt.value:
        pairs = list(zip((ctypes.c_uint64 * cnt.value).from_address(f.value),
                         (ctypes.c_uint32 * cnt.value).from_address(s.value)))
    elif rc == 0:
        assert f.value is None and s.value is None
    lib.cir_free(f)
    lib.cir_free(s)
    return rc, pairs, sk.value, list(stats)


def agree(index, sources):
    import ciruela_amd as ca
    want, skipped = links_restate.expected_candidates(index, sources)
    rc, got, sk, stats = raw_call(index, sources)
    assert rc == 0 and got == want and sk == skipped
    assert ca.link_candidates(index, sources) == want
    files = links_restate.file_entries(index)
    used = []
    for s in sources:
        try:
            if links_restate._header(s) == links_restate._header(index):
                used.append(len(links_restate.file_entries(s)))
        except Exception:
            pass
    assert stats == [len(files), len(want), sum(files[i][2] for i, _ in want), sum(used),
                     len(used), 0, 0, 0]
    pairs, st = ca.file_sources(index, sources)
    assert pairs == want and st["skipped"] == skipped and st["on_device"] == 0
    return got


@pytest.mark.parametrize("case", files_cases.families(), ids=lambda c: c[0])
def test_host_path_families(case):
    _, index, sources = case
    agree(index, sources)


def test_host_path_named_answers():
    fam = {name: (i, s) for name, i, s in files_cases.families()}
    assert agree(*fam["dup_first_wins_miss"]) == []
    assert agree(*fam["dup_first_wins_hit"]) == [(0, 0)]
    assert agree(*fam["dup_then_next_source"]) == [(0, 1)]
    assert agree(*fam["spelling_need_escaped"]) == [(0, 0), (1, 0)]
    assert agree(*fam["spelling_pool_escaped"]) == [(0, 0), (1, 0)]
    assert agree(*fam["size0_same"]) == [(i, 0) for i in range(5)]
    assert agree(*fam["size0_vs_nonempty"]) == [(1, 0)]
    assert agree(*fam["exe_flip"]) == []
    assert agree(*fam["other_digests_then_equal"]) == [(0, 1)]
    assert agree(*fam["swapped_digests"]) == []
    assert agree(*fam["skipped_headers"]) == [(i, 2) for i in range(4)]


def test_host_path_random_sweep():
    hits = 0
    for seed in range(300):
        index, sources = files_cases.random_case(seed)
        hits += len(agree(index, sources))
    assert hits > 200


def test_expected_records_helper_matches_the_restatement():
    """The walk the GPU tests compare records with decodes to the
    restatement's paths, flags, sizes and block numbers."""
    for _, index, _ in files_cases.families():
        recs = files_cases.expected_records(index)
        files = links_restate.file_entries(index)
        assert len(recs) == len(files)
        blk = 0
        for (name_off, dir_off, size, first), (path, exe, fsize, dg) in zip(recs.tolist(), files):
            name = links_restate.unescape(index[name_off:index.index(b" ", name_off)])
            d = links_restate.unescape(index[dir_off:index.index(b"\n", dir_off)])
            assert (b"/" if d == b"/" else d + b"/") + name == path
            assert (size, first & ~files_cases.EXE, bool(first >> 63)) == (fsize, blk, exe)
            blk += len(dg)


def test_errors_are_the_host_calls():
    lib = _native.lib
    _, new, sources = files_cases.families()[0]
    f, s, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    st = (ctypes.c_uint64 * 8)()
    out = (ctypes.byref(f), ctypes.byref(s), ctypes.byref(n), None, st)
    assert lib.cir_file_sources(None, None, 0, None, None, 0, *out) == _native.CIR_EINVAL
    assert lib.cir_file_sources(None, new, len(new), None, None, 1, *out) == _native.CIR_EINVAL
    assert lib.cir_file_sources(None, new, len(new), None, None, 0, ctypes.byref(f), ctypes.byref(s),
                                ctypes.byref(n), None, None) == _native.CIR_EINVAL
    for cut in (len(new) // 2, 30):
        rc = lib.cir_file_sources(None, new, cut, None, None, 0, *out)
        text = lib.cir_last_error()
        assert rc == _native.CIR_EPARSE
        assert lib.cir_link_candidates(new, cut, None, None, 0, *out[:4]) == rc
        assert lib.cir_last_error() == text
        assert list(st) == [0] * 8 and n.value == 0
    assert lib.cir_file_sources(None, new, len(new), None, None, 0, *out) == 0 and n.value == 0


def test_cli_usage_lists_candidates():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index candidates INDEX SRCINDEX [SRCINDEX ...] [--host]" in p.stderr
    p = subprocess.run([cli, "candidates", "/tmp/x.ds1"], capture_output=True)
    assert p.returncode == 2 and b"usage" in p.stderr


def test_cli_candidates_on_the_host(tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    _, index, sources = files_cases.families()[0]
    paths = []
    for k, data in enumerate([index] + sources):
        (tmp_path / ("i%d" % k)).write_bytes(data)
        paths.append(str(tmp_path / ("i%d" % k)))
    p = subprocess.run([cli, "candidates"] + paths + ["--host"], capture_output=True)
    assert p.returncode == 0, p.stderr
    want, _ = links_restate.expected_candidates(index, sources)
    files = links_restate.file_entries(index)
    lines = p.stdout.split(b"\n")[:-1]
    assert [tuple(int(x) for x in l.split(b" ")[:2]) for l in lines] == want
    assert [links_restate.unescape(l.split(b" ", 2)[2]) for l in lines] == [files[i][0] for i, _ in want]
    assert b"matched on the host" in p.stderr


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_files_fuzz_under_asan_ubsan(tmp_path):
    """tools/files_fuzz.cpp: a few thousand seeded random indexes; the header's
    host loops against dirsig::parse, and the host form of fold + table +
    probe + verify against candidates_impl, every buffer of exactly its size.
    A compile failure fails the test."""
    exe = str(tmp_path / "files_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                        "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                        "-I", csrc, os.path.join(ROOT, "tools", "files_fuzz.cpp"),
                        os.path.join(csrc, "dirsig.cpp"), os.path.join(csrc, "links.cpp"),
                        "-o", exe], capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"files_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
    m = re.search(rb"(\d+) texts accepted, (\d+) joins, (\d+) candidates, (\d+) collisions", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr


# ---- the kernels' resources ---------------------------------------------------------------

@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_kernel_resources(tmp_path):
    """The eight kernels of files.hip off the code object: no spill and no
    scratch; only the three passes over the text use LDS (their scans)."""
    res = codeobj.resources(str(tmp_path))
    for name in KERNELS:
        hits = codeobj.find(res, name)
        assert len(hits) == 1, (name, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["private_segment_fixed_size"] == 0, name
        if name in ("k_files_tokens", "k_files_fold", "k_files_build", "k_files_probe",
                    "k_files_verify"):
            assert k["group_segment_fixed_size"] == 0, name
        else:
            assert 0 < k["group_segment_fixed_size"] <= 256, name
