"""cir_block_repeats / cir_match_repeats_dev without a GPU: the declarations in
the header, the ctypes table and INTEGRATION.md's extern block, the Python
names, the argument checks that return before any HIP call, the host path
(ctx = NULL) against a Python restatement of the rule (tests/repeats_restate.py)
over the families of tests/repeats_cases.py, the rule's two properties on a
random index, the composition with cir_block_extents, the CLI, the shared rule
header and the host path under AddressSanitizer and UBSan against a double loop
(tools/repeats_fuzz.cpp, a stand-alone program), and the kernels' resources in
the built code object.

Reference: fill_blocks (src/daemon/tracking/progress.rs:129-170) queues one
Block per (path, offset), so a digest that occurs twice inside an image is
fetched twice; the reference has no counterpart.  No expected value comes from
the library.
"""
import ctypes
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
import dirsig_oracle
import repeats_cases
import repeats_restate
import sources_restate
from ciruela_amd import _native

NEW = ("cir_match_repeats_dev", "cir_block_repeats")
CASES = repeats_cases.cases()
BY_NAME = {c[0]: c for c in CASES}
B = repeats_cases.BS


def _header():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _words(bits, tail=False):
    return None if bits is None else sources_restate.want_words(bits, tail_ones=tail)


def test_header_declares_the_two_and_the_constants():
    text = _header()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
    assert re.search(r"#define CIR_REPEATS_STATS_FIELDS 10\b", text)
    assert re.search(r"#define CIR_REPEATS_MAX_BLOCKS 0x3FFFFFFF\b", text)
    full = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    assert "are not looked for" not in full and "cir_block_repeats' (below)" in full


def test_ctypes_table_binds_the_two():
    for name in NEW:
        assert name in _native._SIGS
        assert getattr(_native.lib, name).restype is ctypes.c_int
    assert len(_native._SIGS["cir_match_repeats_dev"][1]) == 11
    assert len(_native._SIGS["cir_block_repeats"][1]) == 10
    assert _native.CIR_REPEATS_STATS_FIELDS == 10
    assert _native.CIR_REPEATS_MAX_BLOCKS == (1 << 30) - 1


def test_integration_extern_block_names_the_new_functions():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    assert set(NEW) <= bound
    assert "cir_block_repeats(ctx" in text


def test_python_interface():
    import ciruela_amd as ca
    assert callable(ca.block_repeats) and callable(ca.Context.match_repeats_dev)
    for name in ("block_repeats", "RepeatsResult"):
        assert name in ca.__all__
    assert "block_repeats" in ca.__doc__ and "match_repeats_dev" in ca.__doc__
    assert len(ca.RepeatsResult.STATS_FIELDS) == _native.CIR_REPEATS_STATS_FIELDS
    for attr in ("repeats", "bytes_repeated", "copies"):
        assert hasattr(ca.RepeatsResult, attr)


def test_match_repeats_dev_argument_checks():
    """Every CIR_EINVAL case, all decided before any device call (the
    addresses are never dereferenced)."""
    lib = _native.lib
    slots = lib.cir_match_table_slots(100)
    ok = dict(ctx=None, digests=1 << 12, n=100, want=1 << 13, present=1 << 14, table=1 << 15,
              slots=slots, seed=5, match=1 << 16, nmatch=1 << 17, stream=None)
    order = ("ctx", "digests", "n", "want", "present", "table", "slots", "seed", "match", "nmatch",
             "stream")

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_match_repeats_dev(*[a[k] for k in order])
    for kw in (dict(digests=None), dict(match=None), dict(table=None), dict(table=None, n=0)):
        assert call(**kw) == _native.CIR_EINVAL, kw
        assert b"null" in lib.cir_last_error()
    for kw in (dict(digests=(1 << 12) + 8), dict(want=(1 << 13) + 4), dict(present=(1 << 14) + 4),
               dict(match=(1 << 16) + 2), dict(table=(1 << 15) + 2), dict(nmatch=(1 << 17) + 1)):
        assert call(**kw) == _native.CIR_EINVAL, kw
        assert b"aligned" in lib.cir_last_error()
    for kw in (dict(slots=0), dict(slots=slots - 1), dict(slots=slots // 2), dict(slots=3 * slots)):
        assert call(**kw) == _native.CIR_EINVAL, kw
        assert b"table_slots" in lib.cir_last_error()
    assert call(n=1 << 30, slots=1 << 40) == _native.CIR_EINVAL
    assert b"2^30-1" in lib.cir_last_error()
    # (the limit itself passes this check and fails the next one)
    assert call(n=(1 << 30) - 1, slots=1 << 20) == _native.CIR_EINVAL
    assert b"table_slots" in lib.cir_last_error()


INDEX = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  a f 10 " + b"cd" * 32 + b"\n" +
         b"  b f 10 " + b"cd" * 32 + b"\n" + b"ab" * 32 + b"\n")
ARGS = ("ctx", "index", "len", "want", "present", "extents", "nextents", "fetch", "nblk", "stats")


def _repeats_args(**kw):
    a = dict(ctx=None, index=INDEX, len=len(INDEX), want=None, present=None,
             extents=ctypes.pointer(ctypes.c_void_p(1)), nextents=ctypes.pointer(ctypes.c_size_t(7)),
             fetch=ctypes.pointer(ctypes.c_void_p(1)), nblk=ctypes.pointer(ctypes.c_uint64(7)),
             stats=(ctypes.c_uint64 * 10)(*([9] * 10)))
    a.update(kw)
    return [a[k] for k in ARGS]


def _free(args):
    for i in (5, 7):
        if args[i].contents.value:
            _native.lib.cir_free(args[i].contents)
            args[i].contents.value = None


def test_block_repeats_argument_checks():
    """The errors come before any device work: with a context that is not a
    context the checks still come first."""
    lib = _native.lib
    a = _repeats_args()
    assert lib.cir_block_repeats(*a) == _native.CIR_OK
    assert a[6].contents.value == 1 and a[8].contents.value == 2
    rec = (ctypes.c_uint64 * 8).from_address(a[5].contents.value)
    assert list(rec) == [1, 1, 1, 0, 1, 0, 0, 10]
    assert (ctypes.c_uint64 * 1).from_address(a[7].contents.value)[0] == 1
    assert list(a[9]) == [2, 1, 10, 2, 0, 0, 0, 0, 1, 1]
    _free(a)
    for null in ("index", "extents", "nextents", "fetch", "nblk", "stats"):
        for ctx in (None, ctypes.c_void_p(16)):
            assert lib.cir_block_repeats(*_repeats_args(ctx=ctx, **{null: None})) == \
                _native.CIR_EINVAL, null
            assert b"null" in lib.cir_last_error()
    for ctx in (None, ctypes.c_void_p(16)):
        a = _repeats_args(ctx=ctx, index=INDEX[:30], len=30)
        assert lib.cir_block_repeats(*a) == _native.CIR_EPARSE
        assert a[5].contents.value is None and a[6].contents.value == 0
        assert a[7].contents.value is None and a[8].contents.value == 0
        assert list(a[9]) == [0] * 10
    md5 = INDEX.replace(b"blake2b/256", b"md5/128")
    assert lib.cir_block_repeats(*_repeats_args(index=md5, len=len(md5))) in \
        (_native.CIR_EHASHSIZE, _native.CIR_EPARSE)
    short = INDEX.replace(b"cd" * 32, b"cd" * 16)
    a = _repeats_args(index=short, len=len(short))
    assert lib.cir_block_repeats(*a) == _native.CIR_EHASHSIZE
    assert list(a[9]) == [0] * 10


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_path_against_the_restatement(case):
    import ciruela_amd as ca
    _, index, want, present, tail = case
    exp = repeats_restate.expected(index, want, present)
    r = ca.block_repeats(index, want=_words(want, tail), present=_words(present, tail))
    assert repeats_restate.same(r, exp)
    assert r.stats["on_device"] == 0 and r.stats["table_slots"] == 0
    assert list(r.copies()) == repeats_restate.expected_copies(index, exp[0])
    assert r.repeats == exp[2]["repeats"] and r.bytes_repeated == exp[2]["bytes_repeated"]


def test_the_families_hold_what_they_are_named_for():
    """Read off the restatement, not the library."""
    def exp(name):
        _, index, want, present, _ = BY_NAME[name]
        return repeats_restate.expected(index, want, present)
    ext, fetch, stats = exp("duplicated_file")
    assert ext == [(4, 4, 1, 0, 1, 0, 0, 4 * B)] and fetch == [1] * 4 + [0] * 4
    ext, fetch, _ = exp("duplicated_file_short_tail")
    assert ext == [(4, 4, 1, 0, 1, 0, 0, 3 * B + 9)]
    ext, fetch, stats = exp("zero_filled_file")
    assert ext == [(g, 1, 1, g - 1, 1, 1, 0, B) for g in (2, 3, 4, 5)]
    assert fetch == [1, 1, 0, 0, 0, 0] and stats["repeats"] == 4
    ext, fetch, _ = exp("across_two_directories")
    assert ext == [(7, 3, 4, 0, 1, 1, 0, 3 * B)] and sum(fetch) == 7
    ext, fetch, stats = exp("present_beats_earlier_wanted")
    assert ext == [(0, 2, 0, 0, 0, 1, 0, 2 * B), (4, 2, 2, 0, 0, 1, 0, 2 * B)]
    assert sum(fetch) == 0 and stats["present"] == 2 and stats["took_part"] == 6
    ext, _, _ = exp("two_present_holders")
    assert ext == [(4, 2, 2, 0, 0, 0, 0, 2 * B)]
    for name in ("neither_is_never_a_source", "neither_without_present"):
        ext, fetch, stats = exp(name)
        # a's blocks take no part: b is fetched, and c's one wanted block copies from b
        assert ext == [(4, 1, 2, 0, 1, 1, 0, B)] and fetch == [0, 0, 1, 1, 0, 0]
        assert stats["took_part"] == 3
    ext, fetch, stats = exp("bit_in_both_is_wanted")
    assert ext == [(4, 2, 2, 0, 1, 0, 0, 2 * B)] and fetch == [1, 1, 0, 0, 0, 0]
    assert stats["present"] == 0
    ext, fetch, stats = exp("short_equals_full_dropped")
    assert ext == [(2, 1, 1, 0, 1, 0, 1, B)] and fetch == [1, 1, 0, 1]
    assert stats["dropped_length"] == 1 and stats["left_to_fetch"] == 3
    ext, fetch, stats = exp("want_all_zeros")
    assert ext == [] and sum(fetch) == 0 and stats["wanted"] == 0 and stats["present"] == 6
    ext, fetch, stats = exp("tail_ones_in_both")
    assert ext == [(2, 2, 1, 0, 0, 0, 0, 2 * B), (4, 2, 2, 0, 0, 0, 0, 2 * B)]
    assert exp("tail_ones_nothing_set")[2]["took_part"] == 0
    assert exp("no_blocks")[:2] == ([], [])
    ext, fetch, _ = exp("no_repeats")
    assert ext == [] and fetch == [1] * 6
    ext, fetch, _ = exp("class_change_breaks")
    assert ext == [(2, 1, 1, 0, 0, 0, 0, B), (3, 1, 1, 1, 1, 0, 1, B)] and fetch == [0, 1, 0, 0]


def test_no_blocks_gives_null_outputs():
    _, index, _, _, _ = BY_NAME["no_blocks"]
    a = _repeats_args(index=index, len=len(index))
    assert _native.lib.cir_block_repeats(*a) == _native.CIR_OK
    assert a[5].contents.value is None and a[6].contents.value == 0
    assert a[7].contents.value is None and a[8].contents.value == 0
    assert list(a[9]) == [0] * 10


def test_the_two_properties_on_a_random_index():
    """A few thousand blocks drawn from a few hundred digests, no short
    blocks (nothing can be dropped): no block is both a source and a
    destination, and the blocks left to fetch have pairwise distinct digests,
    none of them a present block's."""
    import ciruela_amd as ca
    rng = random.Random(42)
    universe = [rng.randbytes(32) for _ in range(300)]
    files = []
    for f in range(120):
        nb = rng.choice((1, 5, 20, 64))
        files.append(("f", b"f%03d" % f, False, nb * B, [rng.choice(universe) for _ in range(nb)]))
    index = dirsig_oracle.emit("blake2b/256", B, [(b"/", files)], keep_empty=True)
    digests = repeats_restate.index_digests(index)
    n = len(digests)
    assert 2000 < n < 6000
    want = [1 if rng.random() < 0.8 else 0 for _ in range(n)]
    present = [1 if rng.random() < 0.5 else 0 for _ in range(n)]
    for w, p in ((None, None), (want, None), (want, present)):
        r = ca.block_repeats(index, want=_words(w), present=_words(p))
        assert repeats_restate.same(r, repeats_restate.expected(index, w, p))
        assert r.stats["dropped_length"] == 0 and r.repeats > n // 2
        first = [0]
        for _, _, size, ds in repeats_restate.file_entries(index):
            first.append(first[-1] + len(ds))
        sources, dests = set(), set()
        for e in r.extents:
            for k in range(e.count):
                dests.add(e.first + k)
                sources.add(first[e.src_file] + e.src_block + k)
                assert digests[first[e.src_file] + e.src_block + k] == digests[e.first + k]
        assert not (sources & dests) and len(dests) == r.repeats
        fetch = [g for g in range(n) if r.fetch[g >> 3] >> (g & 7) & 1]
        assert len({digests[g] for g in fetch}) == len(fetch) == r.stats["left_to_fetch"]
        is_present = [g for g in range(n) if (w is not None and not w[g]) and p and p[g]]
        assert not ({digests[g] for g in fetch} & {digests[g] for g in is_present})
        assert all(w is None or w[g] for g in fetch)


def test_composition_with_block_extents():
    """block_extents(v2, [v1]), then block_repeats(v2, want = its fetch,
    present = the complement): the second fetch is a subset of the first, and
    feeding it back as `want` finds nothing more."""
    import ciruela_amd as ca
    rng = random.Random(43)
    d = [rng.randbytes(32) for _ in range(40)]

    def f(name, digests):
        return ("f", name, False, len(digests) * B, list(digests))
    v1 = dirsig_oracle.emit("blake2b/256", B, [(b"/", [f(b"a", d[0:6]), f(b"b", d[6:10])])],
                            keep_empty=True)
    # v2: a with a changed block, b unchanged, a new file twice, and a copy of a
    a2 = d[0:3] + [d[20]] + d[4:6]
    v2 = dirsig_oracle.emit("blake2b/256", B,
                            [(b"/", [f(b"a", a2), f(b"b", d[6:10]), f(b"new", d[21:25])]),
                             (b"/copy", [f(b"a", a2), f(b"new", d[21:25])])], keep_empty=True)
    first = ca.block_extents(v2, [v1])
    n = first.nblk
    assert n == 24
    complement = bytes(~b & 0xFF for b in first.fetch)
    second = ca.block_repeats(v2, want=first.fetch, present=complement)
    fbits = [first.fetch[g >> 3] >> (g & 7) & 1 for g in range(n)]
    assert repeats_restate.same(second, repeats_restate.expected(v2, fbits, [1 - b for b in fbits]))
    assert all(s & ~f1 == 0 for s, f1 in zip(second.fetch, first.fetch))
    # a's changed block and `new` are fetched once; /copy/a's changed block and /copy/new repeat
    assert second.stats["wanted"] == 10 and second.repeats == 5
    assert [(e.first, e.count, e.src) for e in second.extents] == [(17, 1, 1), (20, 4, 1)]
    third = ca.block_repeats(v2, want=second.fetch, present=complement)
    assert third.extents == [] and third.fetch == second.fetch and third.repeats == 0


def test_cli_usage_lists_repeats():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"       ciruela-index repeats INDEX [--host]\n" in p.stderr
    for extra in (["a", "b"], [], ["a", "--list"]):
        p = subprocess.run([cli, "repeats"] + extra, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr, extra


def test_cli_repeats_host(tmp_path):
    """`ciruela-index repeats --host` prints a summary line and one line per
    extent, paths escaped as in the index, and opens no device."""
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    for name in ("across_two_directories", "sha512_256", "zero_filled_file", "no_repeats"):
        _, index, _, _, _ = BY_NAME[name]
        path = str(tmp_path / (name + ".ds1"))
        with open(path, "wb") as f:
            f.write(index)
        ext, fetch, stats = repeats_restate.expected(index)
        p = subprocess.run([cli, "repeats", path, "--host"], capture_output=True)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.split(b"\n")
        assert lines[0] == (b"repeats: %d blocks, %d repeat in %d extent(s), %d bytes, %d left to "
                            b"fetch" % (len(fetch), stats["repeats"], len(ext),
                                        stats["bytes_repeated"], sum(fetch)))

        def esc(p_):
            return b"/".join(dirsig_oracle.escape(c) for c in p_.split(b"/"))
        want = [b"%s %d %d %d %s %d" % (esc(dp), do, ln, s, esc(sp), so) for dp, do, ln, s, sp, so
                in repeats_restate.expected_copies(index, ext)]
        assert lines[1:-1] == want and lines[-1] == b""
    p = subprocess.run([cli, "repeats", "--host", path + ".missing"], capture_output=True)
    assert p.returncode == 2
    bad = str(tmp_path / "bad.ds1")
    with open(bad, "wb") as f:
        f.write(b"garbage\n")
    p = subprocess.run([cli, "repeats", "--host", bad], capture_output=True)
    assert p.returncode == 2


@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_repeat_kernels_resources(tmp_path):
    """The two kernels keep everything in registers: no spill, no scratch, no LDS."""
    res = codeobj.resources(str(tmp_path))
    for short in ("k_repeat_build", "k_repeat_probe"):
        hits = codeobj.find(res, short)
        assert len(hits) == 1, (short, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (short, k)
        assert k["private_segment_fixed_size"] == 0, (short, k)
        assert k["group_segment_fixed_size"] == 0, (short, k)


def test_rule_and_host_path_under_asan_and_ubsan(tmp_path):
    """tools/repeats_fuzz.cpp: a few thousand seeded small cases of the shared
    rule header and of the host path against a double loop, every buffer of
    exactly its size.  A compile failure fails the test."""
    exe = str(tmp_path / "repeats_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "repeats_fuzz.cpp"),
                        os.path.join(csrc, "dirsig.cpp"), "-o", exe], capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"repeats_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
