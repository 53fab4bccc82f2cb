"""cir_file_copies / cir_match_copies_dev without a GPU: the declarations in the
header, the ctypes table, INTEGRATION.md's extern block and the Python
interface; the argument checks of cir_match_copies_dev (all CIR_EINVAL cases
are decided before any device call); cir_file_copies with ctx = NULL against
the rule restated in plain Python (tests/copies_restate.py) on the families
and the random cases of tests/copies_cases.py; its relation to
cir_link_candidates; the CLI; a sanitized fuzz of the shared rule header
(tools/copies_fuzz.cpp, a stand-alone program); and the new kernels' resources
in the built code object.  No expected value comes from the library.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
import copies_cases
import copies_restate
import files_cases
import links_restate
from ciruela_amd import _native

NEW = ("cir_match_copies_work_bytes", "cir_match_copies_dev", "cir_file_copies",
       "cir_check_links_at")
KERNELS = ("k_copies_build", "k_copies_probe")


# ---- declarations and bindings ---------------------------------------------------------

def test_header_declares_the_calls():
    full = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|uint64_t) %s\s*\(" % name, text), name
    assert re.search(r"#define CIR_FILE_COPIES_STATS_FIELDS 10\b", text)
    assert "cir_file_copies" in full[:full.index("#ifndef CIRUELA_BLOCKHASH_H")]


def test_ctypes_table_binds_the_calls():
    for name in NEW:
        assert name in _native._SIGS
    assert len(_native._SIGS["cir_match_copies_dev"][1]) == 22
    assert len(_native._SIGS["cir_file_copies"][1]) == 15
    assert len(_native._SIGS["cir_check_links_at"][1]) == len(_native._SIGS["cir_check_links"][1]) + 2
    assert _native.lib.cir_match_copies_work_bytes.restype is ctypes.c_uint64
    assert _native.CIR_FILE_COPIES_STATS_FIELDS == 10


def test_integration_extern_block_names_the_calls():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    assert "cir_file_copies(" in text[text.index("\n}\n"):]      # the step of section 3


def test_python_interface_exists():
    import ciruela_amd as ca
    assert callable(ca.file_copies) and "file_copies" in ca.__all__
    assert callable(ca.Context.match_copies_dev)
    assert callable(ca.check_links_at) and callable(ca.Context.check_links_at)
    assert "check_links_at" in ca.__all__ and "check_links_at" in ca.__doc__
    assert "file_copies" in ca.__doc__ and "Context.match_copies_dev" in ca.__doc__
    assert len(ca.FILE_COPIES_STATS) == 10


def test_work_bytes_are_pure():
    g = _native.lib.cir_match_copies_work_bytes
    assert g(0, 0) == 4 * _native.lib.cir_match_table_slots(0)
    assert g(10, 32) == 16 * 42 + 4 * 64 and g(10, 33) == 16 * 43 + 4 * 128
    assert g(10, 33) == g(10, 33)
    assert g(1 << 32, 1) == 0 and g(1, 1 << 31) == 0
    assert g((1 << 32) - 1, (1 << 31) - 1) > 0


def test_match_copies_dev_argument_checks():
    lib = _native.lib
    ok = dict(nf=1 << 21, nnf=10, nd=1 << 22, nnb=30, pf=1 << 23, pnf=20, pd=1 << 24, pnb=60,
              first=1 << 25, nsrc=2, bs=64, skip=1 << 20, verify=None, seed=1, work=1 << 26,
              wb=lib.cir_match_copies_work_bytes(10, 20), csrc=1 << 27, cfile=1 << 28,
              cplace=1 << 30, res=1 << 29, stream=None)
    order = tuple(ok)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_match_copies_dev(None, *[a[k] for k in order])
    for null in ("nf", "nd", "pf", "pd", "first", "work", "csrc", "cfile", "cplace", "res"):
        assert call(**{null: None}) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    for odd in ("nd", "pd"):
        assert call(**{odd: ok[odd] + 8}) == _native.CIR_EINVAL
        assert b"16-byte aligned" in lib.cir_last_error()
    assert call(verify=(1 << 30) + 8) == _native.CIR_EINVAL
    for odd in ("nf", "pf", "first", "skip", "work", "cfile", "cplace", "res"):
        assert call(**{odd: ok[odd] + 4}) == _native.CIR_EINVAL, odd
    assert call(csrc=ok["csrc"] + 2) == _native.CIR_EINVAL
    assert call(bs=0) == _native.CIR_EINVAL
    assert call(wb=ok["wb"] - 1) == _native.CIR_EINVAL
    assert b"cir_match_copies_work_bytes" in lib.cir_last_error()
    assert call(pnf=1 << 31, wb=1 << 62) == _native.CIR_EINVAL
    assert call(nnf=1 << 32, wb=1 << 62) == _native.CIR_EINVAL
    assert call(nnb=1 << 32) == _native.CIR_EINVAL
    assert call(pnb=1 << 32) == _native.CIR_EINVAL
    assert call(nsrc=(1 << 32) - 1) == _native.CIR_EINVAL
    # (empty sides need no arrays) ... but the scratch is never empty
    assert call(nnf=0, nnb=0, nf=None, nd=None, csrc=None, cfile=None, cplace=None,
                wb=0) == _native.CIR_EINVAL
    assert b"work_bytes" in lib.cir_last_error()


# ---- the host rule ------------------------------------------------------------------------

def raw_call(index, sources, skip=None, ctx=None):
    """cir_file_copies through ctypes: (status, candidates, skipped, stats)."""
    lib = _native.lib
    bufs = [ctypes.create_string_buffer(s, max(len(s), 1)) for s in sources]
    n = max(len(sources), 1)
    sp = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * n)(*[len(s) for s in sources])
    bitmap = None
    if skip is not None:
        nfiles = len(links_restate.file_entries(index))
        words = [0] * ((nfiles + 63) // 64)          # exactly the words the contract names
        for i in skip:
            if i < nfiles:
                words[i >> 6] |= 1 << (i & 63)
        bitmap = (ctypes.c_uint64 * max(len(words), 1))(*words)
    outs = [ctypes.c_void_p(1) for _ in range(5)]
    cnt, sk = ctypes.c_size_t(55), ctypes.c_size_t(77)
    stats = (ctypes.c_uint64 * 10)(*([99] * 10))
    rc = lib.cir_file_copies(ctx, index, len(index), sp, sl, len(sources), bitmap,
                             *[ctypes.byref(o) for o in outs], ctypes.byref(cnt), ctypes.byref(sk),
                             stats)
    found = []
    if rc == 0 and cnt.value:
        k = cnt.value
        f = list((ctypes.c_uint64 * k).from_address(outs[0].value))
        s = list((ctypes.c_uint32 * k).from_address(outs[1].value))
        sf = list((ctypes.c_uint64 * k).from_address(outs[2].value))
        off = list((ctypes.c_uint64 * (k + 1)).from_address(outs[3].value))
        assert off[0] == 0 and off == sorted(off)
        paths = ctypes.string_at(outs[4].value, off[k])
        found = [(f[i], s[i], sf[i], paths[off[i]:off[i + 1]]) for i in range(k)]
        assert f == sorted(set(f))                   # strictly increasing
    elif rc == 0:
        assert all(o.value is None for o in outs)
    if rc == 0:
        for o in outs:
            lib.cir_free(o)
    return rc, found, sk.value, list(stats)


def agree(index, sources, skip=None):
    import ciruela_amd as ca
    want, skipped = copies_restate.expected_copies(index, sources, skip)
    rc, got, sk, stats = raw_call(index, sources, skip)
    assert rc == 0 and got == want and sk == skipped, (got, want)
    es = copies_restate.expected_stats(index, sources, skip)
    assert stats == [es[0], es[1], es[2], es[3], es[4], 0, 0, 0, es[8], es[9]]
    found, st = ca.file_copies(index, sources, skip=skip)
    assert found == want and st["skipped"] == skipped and st["on_device"] == 0
    assert st["skipped_files"] == es[8] and st["same_path"] == es[9]
    return got


@pytest.mark.parametrize("case", copies_cases.families(), ids=lambda c: c[0])
def test_host_rule_families(case):
    _, index, sources, skip = case
    agree(index, sources, skip)


def test_host_rule_named_answers():
    fam = {name: rest for name, *rest in copies_cases.families()}
    got = agree(*fam["renamed_dir"])
    assert got == [(0, 0, 0, b"/conf"), (1, 0, 1, b"/app-1.2.3/bin/run"),
                   (2, 0, 2, b"/app-1.2.3/lib/a.so"), (3, 0, 3, b"/app-1.2.3/lib/b.so")]
    assert agree(*fam["renamed_dir_unlinked"]) == got[1:]
    assert agree(*fam["three_paths_one_source"]) == [(0, 0, 1, b"/a/p")]
    assert agree(*fam["sources_0_and_2"]) == [(0, 0, 0, b"/old/moved")]
    assert agree(*fam["sources_2_only"]) == [(0, 2, 0, b"/c/x")]
    assert agree(*fam["exe_flip"]) == []
    assert agree(*fam["last_block_size"]) == []
    assert agree(*fam["empty_files"]) == []
    got = agree(*fam["skip_bits"])
    assert [g[0] for g in got] == [i for i in range(70) if i not in (0, 63, 64, 65)]
    assert len(agree(*fam["skip_none_of_70"])) == 70 and agree(*fam["skip_all_of_70"]) == []
    assert agree(*fam["skipped_sources"]) == [(0, 4, 0, b"/old/moved")]
    assert agree(*fam["no_sources"]) == [] and agree(*fam["no_files"]) == []
    assert agree(*fam["escaped_source_path"]) == \
        [(0, 0, 0, b"/sp ace/\xff\x01dir/back\\slash and space")]
    assert agree(*fam["escaped_root_name"]) == [(0, 0, 0, b"/\x7f top")]
    assert agree(*fam["own_path_and_moved"]) == [(0, 0, 0, b"/conf"), (1, 0, 1, b"/x"),
                                                 (2, 0, 2, b"/d/a.so")]
    assert agree(*fam["big_files"]) == [(0, 0, 1, b"/o/second"), (1, 0, 0, b"/o/first")]


def test_host_rule_random_sweep():
    moved = several = 0
    for seed in range(300):
        index, sources, skip = copies_cases.random_case(seed)
        agree(index, sources, skip)
        # what makes the comparison worth something, from the restatement alone
        want, _ = copies_restate.expected_copies(index, sources, skip)
        files = links_restate.file_entries(index)
        moved += sum(files[f][0] != path for f, _, _, path in want)
        several += sum(c >= 2 for c in copies_restate.equal_pool_files(index, sources))
    assert moved > 200 and several > 50, (moved, several)


def test_relation_to_the_same_path_rule():
    """Every pair cir_link_candidates returns whose file is not empty has a
    candidate here (skip = NULL), from that source or an earlier one."""
    import ciruela_amd as ca
    pairs = 0
    cases = [(i, s) for _, i, s in files_cases.families()]
    cases += [files_cases.random_case(seed) for seed in range(300)]
    cases += [copies_cases.random_case(seed)[:2] for seed in range(100)]
    for index, sources in cases:
        files = links_restate.file_entries(index)
        linked = [(f, s) for f, s in ca.link_candidates(index, sources) if files[f][2] > 0]
        rc, got, _, _ = raw_call(index, sources)
        assert rc == 0
        by_file = {g[0]: g for g in got}
        for f, s in linked:
            assert f in by_file and by_file[f][1] <= s, (f, s, by_file.get(f))
        pairs += len(linked)
    assert pairs > 300


def test_errors_are_the_host_parsers():
    lib = _native.lib
    _, new, sources, _ = copies_cases.families()[0]
    outs = [ctypes.c_void_p() for _ in range(5)]
    n = ctypes.c_size_t()
    st = (ctypes.c_uint64 * 10)()
    refs = [ctypes.byref(o) for o in outs]
    tail = (ctypes.byref(n), None, st)
    assert lib.cir_file_copies(None, None, 0, None, None, 0, None, *refs, *tail) == _native.CIR_EINVAL
    assert lib.cir_file_copies(None, new, len(new), None, None, 1, None, *refs, *tail) == \
        _native.CIR_EINVAL
    assert lib.cir_file_copies(None, new, len(new), None, None, 0, None, *refs, ctypes.byref(n),
                               None, None) == _native.CIR_EINVAL
    for k in range(5):
        bad = list(refs)
        bad[k] = None
        assert lib.cir_file_copies(None, new, len(new), None, None, 0, None, *bad, *tail) == \
            _native.CIR_EINVAL
    f, s = ctypes.c_void_p(), ctypes.c_void_p()
    for cut in (len(new) // 2, 30):
        rc = lib.cir_file_copies(None, new, cut, None, None, 0, None, *refs, *tail)
        text = lib.cir_last_error()
        assert rc == _native.CIR_EPARSE
        assert lib.cir_link_candidates(new, cut, None, None, 0, ctypes.byref(f), ctypes.byref(s),
                                       ctypes.byref(n), None) == rc
        assert lib.cir_last_error() == text
        assert list(st) == [0] * 10 and n.value == 0 and all(o.value is None for o in outs)
    assert lib.cir_file_copies(None, new, len(new), None, None, 0, None, *refs, *tail) == 0
    assert n.value == 0


# ---- cir_check_links_at before any I/O --------------------------------------------------------

INDEX = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  a f 0\n  b f 0\n" + b"ab" * 32 + b"\n")


def _at_args(**kw):
    a = dict(ctx=ctypes.c_void_p(16),  # never dereferenced before the argument checks
             index=INDEX, len=len(INDEX),
             fds=(ctypes.c_int * 2)(-100, -100),
             dirs=(ctypes.c_char_p * 2)(b"/nonexistent/a", b"/nonexistent/b"), nsrc=2,
             lf=(ctypes.c_uint64 * 2)(0, 1), ls=(ctypes.c_uint32 * 2)(0, 1),
             off=(ctypes.c_uint64 * 3)(0, 2, 5), paths=ctypes.c_char_p(b"/x/y/"), n=2, threads=0,
             kinds=(ctypes.c_uint8 * 2)(7, 7), errnos=(ctypes.c_int32 * 2)(),
             stats=(ctypes.c_uint64 * 8)(*([99] * 8)))
    a.update(kw)
    return [a[k] for k in ("ctx", "index", "len", "fds", "dirs", "nsrc", "lf", "ls", "off", "paths",
                           "n", "threads", "kinds", "errnos", "stats")], a


def test_check_links_at_argument_checks():
    """CIR_EINVAL before any I/O and before the context is touched: the roots
    named here do not exist and the non-null context is not a context."""
    lib = _native.lib
    assert lib.cir_check_links_at(*_at_args(ctx=None)[0]) == _native.CIR_EINVAL
    for null in ("index", "fds", "dirs", "lf", "ls", "kinds", "stats", "paths"):
        assert lib.cir_check_links_at(*_at_args(**{null: None})[0]) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    assert lib.cir_check_links_at(*_at_args(lf=(ctypes.c_uint64 * 2)(0, 2))[0]) == _native.CIR_EINVAL
    assert lib.cir_check_links_at(*_at_args(ls=(ctypes.c_uint32 * 2)(0, 2))[0]) == _native.CIR_EINVAL
    assert lib.cir_check_links_at(*_at_args(off=(ctypes.c_uint64 * 3)(0, 3, 2))[0]) == \
        _native.CIR_EINVAL
    assert b"decrease" in lib.cir_last_error()
    for bad in (b"/x/..", b"./y", b"//", b"/", b"a/./b", b".."):
        args, a = _at_args(off=(ctypes.c_uint64 * 3)(0, 2, 2 + len(bad)),
                           paths=ctypes.c_char_p(b"/x" + bad))
        assert lib.cir_check_links_at(*args) == _native.CIR_EINVAL, bad
        assert b"component" in lib.cir_last_error()
        assert list(a["stats"]) == [0] * 8 and list(a["kinds"]) == [7, 7]
    # a parse error is the index parser's, as in cir_check_links
    args, _ = _at_args(len=30)
    assert lib.cir_check_links_at(*args) == _native.CIR_EPARSE


def test_cli_usage_lists_any_path():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2 and b"[--host] [--any-path]" in p.stderr
    p = subprocess.run([cli, "candidates", "/tmp/x.ds1", "/tmp/y.ds1", "--any-path"],
                       capture_output=True)
    assert p.returncode == 2 and b"usage" in p.stderr


# ---- the CLI ---------------------------------------------------------------------------------

def test_cli_usage_lists_copies():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index copies INDEX SRCINDEX [SRCINDEX ...] [--host] [--unlinked]" in p.stderr
    p = subprocess.run([cli, "copies", "/tmp/x.ds1"], capture_output=True)
    assert p.returncode == 2 and b"usage" in p.stderr


@pytest.mark.parametrize("name", ["own_path_and_moved", "escaped_source_path"])
def test_cli_copies_on_the_host(tmp_path, name):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    fam = {n: rest for n, *rest in copies_cases.families()}
    index, sources, _ = fam[name]
    paths = []
    for k, data in enumerate([index] + sources):
        (tmp_path / ("i%d" % k)).write_bytes(data)
        paths.append(str(tmp_path / ("i%d" % k)))
    files = links_restate.file_entries(index)
    linked = [f for f, _ in links_restate.expected_candidates(index, sources)[0]]
    for flags, skip in ((["--host"], None), (["--host", "--unlinked"], linked)):
        p = subprocess.run([cli, "copies"] + paths + flags, capture_output=True)
        assert p.returncode == 0, p.stderr
        want, _ = copies_restate.expected_copies(index, sources, skip)
        lines = [l.split(b" ") for l in p.stdout.split(b"\n")[:-1]]
        assert all(len(l) == 5 for l in lines)
        assert [tuple(int(x) for x in l[:3]) for l in lines] == [w[:3] for w in want]
        assert [links_restate.unescape(l[3]) for l in lines] == [files[w[0]][0] for w in want]
        assert [links_restate.unescape(l[4]) for l in lines] == [w[3] for w in want]
        assert b"matched on the host" in p.stderr
        assert (b"%d left out" % len(skip or ())) in p.stderr
    if name == "own_path_and_moved":
        assert linked == [0, 2] and len(want) == 1


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_copies_fuzz_under_asan_ubsan(tmp_path):
    """tools/copies_fuzz.cpp: a few thousand seeded random cases; the host form
    of fold + build + probe + verify against a brute-force loop over parsed
    indexes, every buffer of exactly its size, and the collision status
    through a second verify array.  A compile failure fails the test."""
    exe = str(tmp_path / "copies_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                        "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                        "-I", csrc, os.path.join(ROOT, "tools", "copies_fuzz.cpp"),
                        os.path.join(csrc, "dirsig.cpp"), "-o", exe], capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"copies_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
    m = re.search(rb"(\d+) joins, (\d+) candidates \((\d+) at another path\), (\d+) collisions; "
                  rb"paths: (\d+) own, (\d+) ok, (\d+) invalid, (\d+) with a NUL", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr


# ---- the kernels' resources ---------------------------------------------------------------

@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_kernel_resources(tmp_path):
    """The two new kernels of files.hip off the code object: one symbol each,
    no spill, no scratch and no LDS."""
    res = codeobj.resources(str(tmp_path))
    for name in KERNELS:
        hits = codeobj.find(res, name)
        assert len(hits) == 1, (name, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 0, name
