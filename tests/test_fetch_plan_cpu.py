"""cir_fetch_plan / cir_plan_links_dev / cir_plan_want_dev without a GPU: the
declarations in the header, the ctypes table, INTEGRATION.md's extern block and
the Python interface; the argument checks of the two device-resident calls (all
CIR_EINVAL cases are decided before any device call); cir_fetch_plan with ctx =
NULL against the composition of the four restatements (tests/plan_restate.py)
on the families and the random cases of tests/plan_cases.py, and against the
four existing calls composed through Python; the error cases; the CLI; a
sanitized fuzz of the shared rule header (tools/plan_fuzz.cpp, a stand-alone
program); and the new kernels' resources in the built code object.  No expected
value comes from the library.
"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
import plan_cases
import plan_restate
from ciruela_amd import _native
from sources_restate import want_words

NEW = ("cir_plan_links_dev", "cir_plan_want_dev", "cir_fetch_plan")
KERNELS = ("k_plan_links", "k_plan_want")


# ---- declarations and bindings ---------------------------------------------------------

def test_header_declares_the_calls():
    full = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
    assert re.search(r"#define CIR_PLAN_STATS_FIELDS 44\b", text)
    assert re.search(r"#define CIR_PLAN_WHY_EMPTY 5\b", text)
    assert "cir_fetch_plan" in full[:full.index("#ifndef CIRUELA_BLOCKHASH_H")]


def test_ctypes_table_binds_the_calls():
    for name in NEW:
        assert name in _native._SIGS
    assert len(_native._SIGS["cir_plan_links_dev"][1]) == 8
    assert len(_native._SIGS["cir_plan_want_dev"][1]) == 12
    assert len(_native._SIGS["cir_fetch_plan"][1]) == 25
    assert _native.CIR_PLAN_STATS_FIELDS == 44
    assert _native.CIR_PLAN_WHY_EMPTY not in (_native.CIR_FILE_WHY_DECLINED,
                                              _native.CIR_FILE_WHY_COLLISION,
                                              _native.CIR_FILE_WHY_LIMIT, _native.CIR_FILE_WHY_ENV, 0)


def test_integration_extern_block_names_the_calls():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    assert "cir_fetch_plan(" in text[text.index("\n}\n"):]      # the step of section 3


def test_python_interface_exists():
    import ciruela_amd as ca
    assert callable(ca.fetch_plan) and "fetch_plan" in ca.__all__ and "PlanResult" in ca.__all__
    assert callable(ca.Context.plan_links_dev) and callable(ca.Context.plan_want_dev)
    for name in ("fetch_plan", "Context.plan_links_dev", "Context.plan_want_dev"):
        assert name in ca.__doc__, name
    assert set(ca.PlanResult.__slots__) == {"links", "copies", "extents", "repeats", "fetch",
                                            "nblk", "stats", "skipped"}


# ---- the argument checks of the device-resident calls ------------------------------------

def test_plan_links_dev_argument_checks():
    lib = _native.lib
    ok = dict(deny=1 << 20, n=100, src=1 << 21, file=1 << 22, skip=1 << 23, res=1 << 24,
              stream=None)
    order = tuple(ok)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_plan_links_dev(None, *[a[k] for k in order])
    for null in ("src", "file", "skip", "res"):
        assert call(**{null: None}) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    for odd in ("deny", "file", "skip", "res"):
        assert call(**{odd: ok[odd] + 4}) == _native.CIR_EINVAL, odd
        assert b"8-byte aligned" in lib.cir_last_error()
    assert call(src=ok["src"] + 2) == _native.CIR_EINVAL
    assert b"4-byte aligned" in lib.cir_last_error()
    assert call(n=1 << 32) == _native.CIR_EINVAL
    # (no file needs no arrays, but the result words are always written)
    assert call(n=0, src=None, file=None, skip=None, res=None) == _native.CIR_EINVAL


def test_plan_want_dev_argument_checks():
    lib = _native.lib
    ok = dict(runs=1 << 20, nruns=10, n=100, bs=64, nfiles=12, a=1 << 21, b=1 << 22,
              have=1 << 23, want=1 << 24, res=1 << 25, stream=None)
    order = tuple(ok)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_plan_want_dev(None, *[a[k] for k in order])
    for null in ("runs", "want", "res"):
        assert call(**{null: None}) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    for odd in ("runs", "have", "want", "res"):
        assert call(**{odd: ok[odd] + 4}) == _native.CIR_EINVAL, odd
        assert b"8-byte aligned" in lib.cir_last_error()
    for odd in ("a", "b"):
        assert call(**{odd: ok[odd] + 2}) == _native.CIR_EINVAL, odd
        assert b"4-byte aligned" in lib.cir_last_error()
    assert call(bs=0) == _native.CIR_EINVAL
    assert b"block_size" in lib.cir_last_error()
    for big in ("n", "nruns", "nfiles"):
        assert call(**{big: 1 << 32}) == _native.CIR_EINVAL, big
    assert call(n=0, nruns=0, runs=None, want=None, res=None) == _native.CIR_EINVAL


# ---- the host composition ------------------------------------------------------------------

def raw_call(index, sources, deny=None, have=None, ctx=None, nsrc=None):
    """cir_fetch_plan through ctypes with poisoned outputs: (status, the ten
    pointers, the six counts, stats)."""
    lib = _native.lib
    bufs = [ctypes.create_string_buffer(s, max(len(s), 1)) for s in sources]
    n = max(len(sources), 1)
    sp = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * n)(*[len(s) for s in sources])
    outs = [ctypes.c_void_p(1) for _ in range(10)]
    nl, nc, ne, nr, sk = (ctypes.c_size_t(55) for _ in range(5))
    nblk = ctypes.c_uint64(66)
    stats = (ctypes.c_uint64 * 44)(*([99] * 44))
    ref = ctypes.byref
    rc = lib.cir_fetch_plan(ctx, index, len(index), sp, sl, len(sources) if nsrc is None else nsrc,
                            deny, have, ref(outs[0]), ref(outs[1]), ref(nl), ref(outs[2]),
                            ref(outs[3]), ref(outs[4]), ref(outs[5]), ref(outs[6]), ref(nc),
                            ref(outs[7]), ref(ne), ref(outs[8]), ref(nr), ref(outs[9]), ref(nblk),
                            ref(sk), stats)
    return rc, [o.value for o in outs], [nl.value, nc.value, ne.value, nr.value, nblk.value,
                                         sk.value], list(stats)


def host(index, sources, deny, have):
    import ciruela_amd as ca
    hb = None if have is None else bytes(want_words(have))
    return ca.fetch_plan(index, sources, None, deny=deny, have=hb)


def test_hand_made_counts():
    """The first family's answer, counted by hand (plan_cases.hand_made)."""
    new, olds = plan_cases.hand_made()
    hm = plan_cases.HAND_MADE
    for got in (plan_restate.expected(new, olds), None):
        if got is None:
            r = host(new, olds, None, None)
            got = dict(nblk=r.nblk, links=r.links, copies=r.copies, extents=r.extents,
                       repeats=[tuple(e) for e in r.repeats],
                       fetch=[(r.fetch[g >> 3] >> (g & 7)) & 1 for g in range(r.nblk)])
        assert got["nblk"] == hm["nblk"]
        assert (len(got["links"]), len(got["copies"]), len(got["extents"]),
                len(got["repeats"])) == (hm["links"], hm["copies"], hm["extents"], hm["repeats"])
        assert got["repeats"][0][1] == hm["repeat_blocks"]
        assert got["repeats"][0][4] == hm["repeat_src"]
        assert sum(got["fetch"]) == hm["fetch"]
    denied = plan_restate.expected(new, olds, [0])
    assert (len(denied["links"]), len(denied["extents"])) == (
        plan_cases.HAND_MADE_DENY0["links"], plan_cases.HAND_MADE_DENY0["extents"])
    assert plan_cases.families()[0][0] == "hand_made"


@pytest.mark.parametrize("case", plan_cases.families(), ids=lambda c: c[0])
def test_families_on_the_host(case):
    _, index, sources, deny, have = case
    want = plan_restate.expected(index, sources, deny, have)
    got = host(index, sources, deny, have)
    assert plan_restate.same(got, want, 0), (got, got.stats)
    assert got.stats["why_host"] == 0
    for part in ("sources", "copies", "extents", "repeats"):
        assert got.stats[part]["on_device"] == 0 and got.stats[part]["table_slots"] == 0


def test_named_answers():
    fam = {name: rest for name, *rest in plan_cases.families()}
    got = host(*fam["have_and_its_twin"])
    assert [(e.src, e.count) for e in got.repeats] == [(0, 1)]   # from the block that was there
    assert got.stats["have_blocks"] == 1
    got = host(*fam["denied_with_content_candidate"])
    assert got.links == [] and [c[0] for c in got.copies] == [1] and got.stats["withdrawn"] == 1
    assert [e.need_file for e in got.extents] == [0]
    got = host(*fam["deny_bits"])
    assert [f for f, _ in got.links] == [i for i in range(70) if i not in (0, 63, 64, 65)]
    assert got.stats["withdrawn"] == 4 and sorted({e.need_file for e in got.extents}) == \
        [0, 63, 64, 65]
    got = host(*fam["skipped_sources"])
    assert got.skipped == 3 and got.links == [(0, 2)] and [c[1] for c in got.copies] == [2]
    got = host(*fam["all_linked"])
    assert got.left_to_fetch() == 0 and got.stats["linked_blocks"] == got.nblk == 73
    got = host(*fam["nothing_linked"])
    assert got.left_to_fetch() == got.nblk and got.stats["linked"] == 0


def test_random_cases_on_the_host():
    """The 200 seeds with their random have bitmaps, and how far each reaches:
    the figures the cases were chosen by."""
    none, reach = 0, [0] * 5
    for seed in range(200):
        index, sources, deny, have = plan_cases.random_case(seed)
        want = plan_restate.expected(index, sources, deny, have)
        assert plan_restate.same(host(index, sources, deny, have), want, 0), seed
        plain = plan_restate.expected(index, sources, deny, None)
        if plain["nblk"] == 0 or plain["stats"]["sources"]["sources_used"] == 0:
            none += 1
        else:
            reach = [a + b for a, b in zip(reach, plan_restate.reach(plain))]
    assert none == 42 and reach == [54, 116, 84, 27, 81]


def test_equals_the_four_calls_composed():
    import ciruela_amd as ca
    cases = [c[1:] for c in plan_cases.families()]
    cases += [plan_cases.random_case(seed) for seed in range(0, 200, 5)]
    for index, sources, deny, have in cases:
        got = host(index, sources, deny, have)
        want = plan_restate.composed(ca, index, sources, deny, have)
        assert (got.links, got.copies, [tuple(e) for e in got.extents],
                [tuple(e) for e in got.repeats], got.fetch, got.nblk) == \
            (want["links"], want["copies"], want["extents"], want["repeats"], want["fetch"],
             want["nblk"])


def test_errors_leave_outputs_null_and_stats_zero():
    new, olds = plan_cases.hand_made()
    digest = re.search(rb" ([0-9a-f]{64})\n", new).group(1)
    short_hash = new.replace(digest, digest[:32], 1)          # a token of 16 bytes
    for index, code in ((b"not an index\n", _native.CIR_EPARSE), (new[:200], _native.CIR_EPARSE),
                        (short_hash, _native.CIR_EHASHSIZE)):
        rc, outs, counts, stats = raw_call(index, olds)
        assert rc == code, (index[:20], rc)
        assert outs == [None] * 10 and counts == [0] * 6 and stats == [0] * 44
    # null arguments are refused before anything is written
    lib = _native.lib
    assert lib.cir_fetch_plan(None, None, 0, None, None, 0, None, None, *([None] * 17)) == \
        _native.CIR_EINVAL
    rc, outs, counts, stats = raw_call(new, [], nsrc=0)
    assert rc == 0 and counts[4] == 93 and stats[43] == 0 and stats[42] == 0


def test_success_through_ctypes_matches_the_counts():
    new, olds = plan_cases.hand_made()
    rc, outs, counts, stats = raw_call(new, olds)
    assert rc == 0 and counts == [2, 1, 4, 1, 93, 0]
    assert all(outs), outs
    assert stats[38:44] == [0, 3, 8, 0, 0, 0] and stats[0] == stats[8] == 7
    for p in outs:
        _native.lib.cir_free(ctypes.c_void_p(p))


# ---- the CLI ---------------------------------------------------------------------------------

def test_cli_usage_lists_plan():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index plan INDEX SRCINDEX [SRCINDEX ...] [--host]" in p.stderr
    p = subprocess.run([cli, "plan", "/tmp/x.ds1"], capture_output=True)
    assert p.returncode == 2 and b"usage" in p.stderr


def test_cli_plan_on_the_host(tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    new, olds = plan_cases.hand_made()
    paths = []
    for k, data in enumerate([new] + olds):
        (tmp_path / ("i%d" % k)).write_bytes(data)
        paths.append(str(tmp_path / ("i%d" % k)))
    p = subprocess.run([cli, "plan"] + paths + ["--host"], capture_output=True)
    assert p.returncode == 0, p.stderr
    want = plan_restate.expected(new, olds)
    st = want["stats"]
    size = {f: e[2] for f, e in enumerate(plan_restate.links_restate.file_entries(new))}
    fetch_bytes = sum(size.values()) - sum(size[f] for f, _ in want["links"]) - \
        sum(size[c[0]] for c in want["copies"]) - st["extents"]["bytes_local"] - \
        st["repeats"]["bytes_repeated"]
    assert p.stdout.split(b"\n")[:-1] == [
        b"link 2 files at their own path, %d bytes" % sum(size[f] for f, _ in want["links"]),
        b"link 1 files by content, %d bytes" % sum(size[c[0]] for c in want["copies"]),
        b"copy 4 extents from older images, %d blocks, %d bytes" % (
            st["extents"]["found"], st["extents"]["bytes_local"]),
        b"copy 1 extents inside the image, 5 blocks, %d bytes" % st["repeats"]["bytes_repeated"],
        b"fetch 9 blocks of 93, %d bytes" % fetch_bytes]
    assert b"planned on the host" in p.stderr and b"1 source index(es) used" in p.stderr


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_plan_fuzz_under_asan_ubsan(tmp_path):
    """tools/plan_fuzz.cpp: a few thousand seeded random cases; the host forms
    of the two kernels against loops over files and blocks, lying run tables
    included, and plan_host over stand-in calls, every buffer of exactly its
    size.  A compile failure fails the test."""
    exe = str(tmp_path / "plan_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "plan_fuzz.cpp"), "-o", exe],
                       capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"plan_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
    m = re.search(rb"(\d+) files, (\d+) blocks; (\d+) wanted, (\d+) linked, (\d+) held; (\d+) "
                  rb"lying tables; (\d+) plans, (\d+) failed", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr


# ---- the kernels' resources ---------------------------------------------------------------

@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_kernel_resources(tmp_path):
    """The two kernels of plan.hip off the code object: one symbol each, no
    spill, no scratch and no LDS."""
    res = codeobj.resources(str(tmp_path))
    for name in KERNELS:
        hits = codeobj.find(res, name)
        assert len(hits) == 1, (name, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 0, name
