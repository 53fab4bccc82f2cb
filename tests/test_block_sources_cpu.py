"""cir_block_sources / cir_match_digests_dev / cir_match_table_slots without a
GPU: the declarations in the header, the ctypes table and INTEGRATION.md's
extern block, the Python names, the table size, the argument checks that need
no device, the host join (ctx = NULL) against a Python restatement of the rule
over families of hand-made and seeded random indexes, the header-only host
side (ciruela_amd/csrc/sources.hpp) under AddressSanitizer and UBSan against a
double loop (tools/sources_fuzz.cpp, a stand-alone program), the two join
kernels' resources in the built code object, and the CLI.

Reference: fill_blocks (src/daemon/tracking/progress.rs:129-170) queues every
block of every file that was not hardlinked whole; scan_links matches whole
files only (src/daemon/metadata/hardlink_sources.rs:131-133, the break at
:143).  No expected value comes from the library: indexes are
dirsig_oracle.emit's over random digests, and the expected arrays are
tests/sources_restate.py's.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
import dirsig_oracle
import sources_cases
import sources_restate
from ciruela_amd import _native

NEW = ("cir_match_table_slots", "cir_match_digests_dev", "cir_block_sources")
CASES = sources_cases.cases()


def _header():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_three_and_the_constant():
    text = _header()
    assert re.search(r"\buint64_t cir_match_table_slots\s*\(", text)
    for name in NEW[1:]:
        assert re.search(r"\bint %s\s*\(" % name, text), name
    assert re.search(r"#define CIR_SOURCES_STATS_FIELDS 8\b", text)


def test_ctypes_table_binds_the_three():
    for name in NEW:
        assert name in _native._SIGS
    assert _native.lib.cir_match_table_slots.restype is ctypes.c_uint64
    assert _native.lib.cir_match_digests_dev.restype is ctypes.c_int
    assert _native.lib.cir_block_sources.restype is ctypes.c_int
    assert len(_native._SIGS["cir_match_table_slots"][1]) == 1
    assert len(_native._SIGS["cir_match_digests_dev"][1]) == 11
    assert len(_native._SIGS["cir_block_sources"][1]) == 13
    assert _native.CIR_SOURCES_STATS_FIELDS == 8


def test_integration_extern_block_names_the_three():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    assert set(NEW) <= bound


def test_python_interface():
    import ciruela_amd as ca
    assert callable(ca.block_sources) and callable(ca.Context.match_digests_dev)
    for name in ("block_sources", "SourcesResult"):
        assert name in ca.__all__
    assert "src/daemon/tracking/progress.rs:129-170" in ca.__doc__
    assert len(ca.SourcesResult.STATS_FIELDS) == _native.CIR_SOURCES_STATS_FIELDS
    for attr in ("found", "bytes_local", "copies", "want_after"):
        assert hasattr(ca.SourcesResult, attr)


def test_match_table_slots():
    """The smallest power of two >= max(64, 2 n)."""
    f = _native.lib.cir_match_table_slots
    assert [f(n) for n in (0, 1, 32, 33, 1 << 20, (1 << 20) + 1)] == \
        [64, 64, 64, 128, 1 << 21, 1 << 22]
    assert f((1 << 31) - 1) == 1 << 32


def test_match_digests_dev_argument_checks():
    """Every CIR_EINVAL case, all decided before any device call (the
    addresses are never dereferenced)."""
    lib = _native.lib
    ok = dict(ctx=None, need=4096, n_need=5, pool=8192, n_pool=40, table=1 << 16, slots=128,
              seed=7, match=1 << 17, nmatch=1 << 18, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_match_digests_dev(a["ctx"], a["need"], a["n_need"], a["pool"], a["n_pool"],
                                         a["table"], a["slots"], a["seed"], a["match"],
                                         a["nmatch"], a["stream"])
    for kw in (dict(need=None), dict(pool=None), dict(match=None), dict(table=None),
               dict(table=None, n_pool=0, n_need=0)):
        assert call(**kw) == _native.CIR_EINVAL, kw
        assert b"null" in lib.cir_last_error()
    for kw in (dict(need=4096 + 8), dict(pool=8192 + 4), dict(need=4096 + 1)):
        assert call(**kw) == _native.CIR_EINVAL, kw
        assert b"16-byte aligned" in lib.cir_last_error()
    # the table: a power of two, at least cir_match_table_slots(n_pool)
    for slots in (0, 64, 96, 127, 129, (1 << 20) + 1):
        assert call(slots=slots) == _native.CIR_EINVAL, slots
        assert b"table_slots" in lib.cir_last_error()
    assert call(n_pool=33, slots=64) == _native.CIR_EINVAL
    # u32 pool ordinals below the empty mark's half
    for n in (1 << 31, (1 << 32) + 3):
        assert call(n_pool=n, slots=1 << 40) == _native.CIR_EINVAL
        assert b"2^31-1" in lib.cir_last_error()
    assert call(n_need=1 << 32) == _native.CIR_EINVAL
    assert call(match=(1 << 17) + 2) == _native.CIR_EINVAL


INDEX = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  a f 10 " + b"cd" * 32 + b"\n" +
         b"ab" * 32 + b"\n")


def _sources_args(**kw):
    srcs = (ctypes.c_void_p * 1)(ctypes.cast(ctypes.c_char_p(INDEX), ctypes.c_void_p))
    lens = (ctypes.c_size_t * 1)(len(INDEX))
    a = dict(ctx=None, index=INDEX, len=len(INDEX), src_index=srcs, src_len=lens, nsrc=1,
             want=None, src=ctypes.pointer(ctypes.c_void_p(1)),
             file=ctypes.pointer(ctypes.c_void_p(1)), block=ctypes.pointer(ctypes.c_void_p(1)),
             nblk=ctypes.pointer(ctypes.c_uint64(7)), skipped=ctypes.pointer(ctypes.c_size_t(7)),
             stats=(ctypes.c_uint64 * 8)())
    a.update(kw)
    return [a[k] for k in ("ctx", "index", "len", "src_index", "src_len", "nsrc", "want", "src",
                           "file", "block", "nblk", "skipped", "stats")]


def _free(args):
    for i in (7, 8, 9):
        if args[i].contents.value:
            _native.lib.cir_free(args[i].contents)
            args[i].contents.value = None


def test_block_sources_argument_checks():
    """CIR_EINVAL / CIR_EPARSE / CIR_EHASHSIZE before any device work: with a
    context that is not a context the checks still come first."""
    lib = _native.lib
    a = _sources_args()
    assert lib.cir_block_sources(*a) == _native.CIR_OK
    assert a[10].contents.value == 1 and a[11].contents.value == 0
    assert list(a[12])[:6] == [1, 1, 10, 1, 1, 0] and a[12][7] == 0
    _free(a)
    for null in ("index", "src", "file", "block", "nblk", "stats", "src_index", "src_len"):
        for ctx in (None, ctypes.c_void_p(16)):
            assert lib.cir_block_sources(*_sources_args(ctx=ctx, **{null: None})) == \
                _native.CIR_EINVAL, null
            assert b"null" in lib.cir_last_error()
    # nskipped_out may be NULL; so may the source arrays when nsrc == 0
    a = _sources_args(skipped=None)
    assert lib.cir_block_sources(*a) == _native.CIR_OK
    _free(a)
    a = _sources_args(src_index=None, src_len=None, nsrc=0)
    assert lib.cir_block_sources(*a) == _native.CIR_OK
    assert a[10].contents.value == 1 and list(a[12])[:5] == [1, 0, 0, 0, 0]
    _free(a)
    # an index that does not parse: the outputs are cleared all the same
    for ctx in (None, ctypes.c_void_p(16)):
        a = _sources_args(ctx=ctx, index=INDEX[:30], len=30)
        assert lib.cir_block_sources(*a) == _native.CIR_EPARSE
        assert a[7].contents.value is None and a[8].contents.value is None
        assert a[9].contents.value is None and a[10].contents.value == 0
        assert a[11].contents.value == 0
    short = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  f f 10 " + b"ab" * 16 + b"\n" +
             b"ab" * 32 + b"\n")
    assert lib.cir_block_sources(*_sources_args(index=short, len=len(short))) in \
        (_native.CIR_EHASHSIZE, _native.CIR_EPARSE)
    md5 = INDEX.replace(b"blake2b/256", b"md5/128")
    assert lib.cir_block_sources(*_sources_args(index=md5, len=len(md5))) in \
        (_native.CIR_EHASHSIZE, _native.CIR_EPARSE)
    # (a pool of 2^31 blocks needs 2^31 digests in the sources' text, 128 GiB:
    # the limit is checked through the header-only helper, in sources_fuzz)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_join_against_the_restatement(case):
    import ciruela_amd as ca
    _, index, sources, bits, tail = case
    want = None if bits is None else sources_restate.want_words(bits, tail_ones=tail)
    exp = sources_restate.expected(index, sources, bits)
    r = ca.block_sources(index, sources, want=want)
    assert sources_restate.same(r, exp)
    assert r.stats["on_device"] == 0
    assert r.found == exp[3]["found"] and r.bytes_local == exp[3]["bytes_local"]
    assert list(r.copies()) == sources_restate.expected_copies(index, sources, *exp[:3])
    after = [1 if (bits is None or bits[g]) and exp[0][g] is None else 0 for g in range(r.nblk)]
    assert r.want_after() == sources_restate.want_words(after)


def test_the_named_families_hold_what_they_are_named_for():
    """The hand-made families do exercise their edge (read off the
    restatement, not the library)."""
    by = {c[0]: c for c in CASES}

    def exp(name):
        _, index, sources, bits, _ = by[name]
        return sources_restate.expected(index, sources, bits)
    src, file, block, stats, _ = exp("first_source_first_place")
    # d0 d1 d2 | d3 d0: d1 first at source 0 file 0 block 1, d3 at source 0 file 2 block 1
    assert (src, file, block) == ([1, 0, 1, 0, 1], [0, 0, 0, 2, 0], [0, 1, 2, 1, 0])
    assert exp("ranking_reversed")[0] == [0, 0, 0, 0, 0]
    assert exp("short_matches_short")[:3] == ([0, None, 0], [0, None, 0], [0, None, 1])
    src, _, _, stats, _ = exp("lying_source_first")
    # (d10 sits in the liar at a 5-byte block: dropped, and the honest copy behind it is not
    # taken; d11 is a whole block in the liar as well)
    assert src == [None, 0, None] and stats["dropped_length"] == 1 and stats["found"] == 1
    assert exp("honest_source_first")[0] == [0, 0, None]
    src, _, _, stats, skipped = exp("skipped_sources")
    assert src == [1, 5, 1] and skipped == 5 and stats["sources_used"] == 2
    assert exp("no_sources")[0] == [None] * 3
    assert exp("no_blocks")[0] == []
    assert exp("sha512_256")[:3] == ([None, 1, 1], [None, 0, 0], [None, 0, 1])
    assert exp("sha512_256")[4] == 1
    assert any(c[0].startswith("random") and sources_restate.expected(c[1], c[2], c[3])[3]
               ["dropped_length"] for c in CASES)


def test_no_blocks_gives_null_arrays():
    _, index, sources, _, _ = next(c for c in CASES if c[0] == "no_blocks")
    srcs = [ctypes.create_string_buffer(s, len(s)) for s in sources]
    sp = (ctypes.c_void_p * len(srcs))(*[ctypes.cast(b, ctypes.c_void_p) for b in srcs])
    sl = (ctypes.c_size_t * len(srcs))(*[len(s) for s in sources])
    a = _sources_args(index=index, len=len(index), src_index=sp, src_len=sl, nsrc=len(srcs))
    assert _native.lib.cir_block_sources(*a) == _native.CIR_OK
    assert a[7].contents.value is None and a[8].contents.value is None
    assert a[9].contents.value is None and a[10].contents.value == 0
    assert a[12][0] == 0 and a[12][4] == 2


def test_skip_files_and_have_fold_into_want():
    import ciruela_amd as ca
    _, index, sources, _, _ = next(c for c in CASES if c[0] == "first_source_first_place")
    # file 0 (blocks 0-2) was hardlinked; block 4 is already there
    r = ca.block_sources(index, sources, skip_files={0}, have=bytes([0b10000]))
    assert sources_restate.same(r, sources_restate.expected(index, sources, [0, 0, 0, 1, 0]))
    assert r.want_after() == sources_restate.want_words([0] * 5)
    r = ca.block_sources(index, sources, want=bytes([0b01111]), skip_files={1})
    assert sources_restate.same(r, sources_restate.expected(index, sources, [1, 1, 1, 0, 0]))


def test_cli_usage_lists_sources():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index sources INDEX SRCINDEX [SRCINDEX ...] [--list] [--host]" in p.stderr
    for args in (["sources", "/tmp/x.ds1"], ["check", "/tmp", "/tmp/x.ds1", "--host"]):
        p = subprocess.run([cli] + args, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr


def test_cli_sources_host(tmp_path):
    """`ciruela-index sources --host --list` prints the restatement's lines,
    paths escaped as in the index, and opens no device."""
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    _, index, sources, _, _ = next(c for c in CASES if c[0] == "sha512_256")
    names = []
    for i, raw in enumerate([index] + list(sources)):
        names.append(str(tmp_path / ("i%d.ds1" % i)))
        with open(names[-1], "wb") as f:
            f.write(raw)
    src, file, block, stats, skipped = sources_restate.expected(index, sources)
    p = subprocess.run([cli, "sources"] + names + ["--list", "--host"], capture_output=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.split(b"\n")
    assert lines[0] == (b"sources: %d blocks, %d found, %d bytes found; %d source index(es) used, "
                        b"%d skipped" % (len(src), stats["found"], stats["bytes_local"],
                                         stats["sources_used"], skipped))
    def esc(path):
        return b"/".join(dirsig_oracle.escape(c) for c in path.split(b"/"))
    want = [b"%s %d %d %d %s %d" % (esc(dp), do, ln, s, esc(sp), so) for dp, do, ln, s, sp, so in
            sources_restate.expected_copies(index, sources, src, file, block)]
    assert want and lines[1:-1] == want and lines[-1] == b""
    assert b"/a\\x20b 64 64 1 /p/\\xffq 0" in lines
    # without --list: the summary alone
    p = subprocess.run([cli, "sources", "--host"] + names, capture_output=True)
    assert p.returncode == 0 and p.stdout.split(b"\n")[1:] == [b""]
    # a new index that does not parse: exit 2
    p = subprocess.run([cli, "sources", "--host", names[2], names[1], names[1] + ".missing"],
                       capture_output=True)
    assert p.returncode == 2


@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_join_kernels_resources(tmp_path):
    """k_join_build and k_join_probe are plain loops over global memory: no
    spill, no scratch, no LDS."""
    res = codeobj.resources(str(tmp_path))
    for short in ("k_join_build", "k_join_probe"):
        hits = codeobj.find(res, short)
        assert len(hits) == 1, (short, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
        assert k["private_segment_fixed_size"] == 0
        assert k["group_segment_fixed_size"] == 0


def test_host_side_under_asan_and_ubsan(tmp_path):
    """tools/sources_fuzz.cpp: a few thousand seeded cases of random small
    indexes through the pool builder, the host join and the mapping against a
    double loop, every buffer of exactly its size; and the pool's limit of
    2^31 - 1 blocks.  A compile failure fails the test."""
    exe = str(tmp_path / "sources_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "sources_fuzz.cpp"),
                        os.path.join(csrc, "dirsig.cpp"), "-o", exe], capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"sources_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
