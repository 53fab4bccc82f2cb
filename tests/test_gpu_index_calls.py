"""The whole-call entry points over index texts on one device flow
(ciruela_amd/csrc/devcall.hpp): cir_block_sources, cir_block_extents,
cir_block_repeats, cir_file_sources, cir_index_digests, cir_file_copies and
cir_fetch_plan.

One child process under CIR_TRACE=1 makes one lazy-staging context and runs
every call on every path -- with the context, under CIR_SOURCES_PARSE=host,
CIR_SOURCES_MAP=host and =device, CIR_LINKS_MATCH=host, and with ctx = NULL --
on the smallest shared cases (cir_fetch_plan: with the context, under
CIR_PLAN=host and with ctx = NULL).  Per path, the trace lines with every number
replaced by N equal literals written from the format strings, and the parsers
the bench tools read those lines with (tools/block_sources_bench.py,
tools/block_repeats_bench.py, tools/file_sources_bench.py,
tools/file_copies_bench.py, tools/fetch_plan_bench.py) find every lap they
name; the results of all paths of a call are equal.

And ctx against NULL on a set of texts on which the two-pass parse's offsets,
the per-text fallback and the retry meet: three sources whose lengths differ
modulo 16, one longer than two 4096-byte tiles, one the device declines (a
doubled space), one with a bad hex digit.
"""
import json
import os
import random
import re
import subprocess
import sys

import pytest

import copies_restate
import files_cases
import plan_restate
import sources_cases
from sources_cases import BS, _emit, _file

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, os, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import ciruela_amd as ca
import copies_cases, files_cases, plan_cases, plan_restate, repeats_cases, sources_cases
_, index, sources, _, _ = next(c for c in sources_cases.cases() if c[0] == "skipped_sources")
_, rep, _, _, _ = next(c for c in repeats_cases.cases() if c[0] == "duplicated_file")
_, fnew, fsrc = next(c for c in files_cases.families() if c[0] == "order_12")
# (moved files, a skip bitmap; and a source that is skipped, in front of the one that counts)
_, cnew, csrc, cskip = next(c for c in copies_cases.families() if c[0] == "renamed_dir_unlinked")
csrc = [b"garbage"] + csrc
pnew, psrc = plan_cases.hand_made()
psrc = psrc + [b"garbage"]
pwant = plan_restate.expected(pnew, psrc)
ctx = ca.Context(device_mask=1, staging_bytes=ca._n.CIR_STAGING_LAZY)
SWITCHES = ("CIR_SOURCES_PARSE", "CIR_SOURCES_MAP", "CIR_LINKS_MATCH", "CIR_PLAN")
PATH_STATS = ("on_device", "table_slots", "why_host")

def ext(r):
    return [r.nblk, [tuple(getattr(e, f) for f in ("first", "count", "need_file", "need_block",
                                                  "src", "src_file", "src_block", "bytes"))
                     for e in r.extents], list(bytes(r.fetch)), sorted(r.stats.items())]

def copies(found):
    return [[f, s, sf, path.hex()] for f, s, sf, path in found]

def plan(r):
    # (the siblings' stats without what says where they ran; the plan's own with it)
    stats = [[k, sorted((a, b) for a, b in v.items() if a not in PATH_STATS)
              if isinstance(v, dict) else v] for k, v in sorted(r.stats.items())]
    return [plan_restate.same(r, pwant), r.links, copies(r.copies),
            [list(e) for e in r.extents], [list(e) for e in r.repeats], r.fetch.hex(), r.nblk,
            r.skipped, stats]

CALLS = {
    "block_sources": lambda c: (lambda r: [r.src, r.file, r.block, r.skipped,
                                           sorted(r.stats.items())])(
        ca.block_sources(index, sources, context=c)),
    "block_extents": lambda c: (lambda r: ext(r) + [r.skipped])(
        ca.block_extents(index, sources, context=c)),
    "block_repeats": lambda c: ext(ca.block_repeats(rep, context=c)),
    "file_sources": lambda c: (lambda r: [r[0], sorted(r[1].items())])(
        ca.file_sources(fnew, fsrc, context=c)),
    "index_digests": lambda c: (lambda r: [r.hash_type, r.block_size, r.digests.tobytes().hex(),
                                           r.runs.tolist(), r.nfiles])(
        ca.index_digests(index, c)),
    "file_copies": lambda c: (lambda r: [copies(r[0]), sorted(r[1].items())])(
        ca.file_copies(cnew, csrc, c, skip=cskip)),
    "fetch_plan": lambda c: plan(ca.fetch_plan(pnew, psrc, c)),
}
out = {}
for spec in sys.argv[2:]:
    call, where, env = spec.split(":")
    for k in SWITCHES:
        os.environ.pop(k, None)
    if env:
        k, v = env.split("=")
        os.environ[k] = v
    sys.stderr.write("path %s\n" % spec)
    sys.stderr.flush()
    out[spec] = CALLS[call](ctx if where == "ctx" else None)
print(json.dumps(out))
"""

N = "N"
BS_HOST = ("cir block_sources: N blocks against N pool blocks of N source(s), host; parse N ms, "
           "pool N ms, join N ms, map N ms")
BS_DEV = ("cir block_sources: N blocks against N pool blocks of N source(s), device; parse N ms, "
          "pool N ms, upload N ms, build kernel N ms, probe kernel N ms, download N ms, map N ms")
BS_DEV_PARSE = BS_DEV + ("; device parse of N text(s): frame N ms, text upload N ms, count kernels "
                         "N ms, host parse N ms, decode kernels N ms, runs download N ms")
XMAP = ("cir extents map (block_%s): N blocks; tables upload N ms (N + N runs), map kernel N ms, "
        "scan kernel N ms, emit kernels N ms, downloads N ms; N extents, N bytes downloaded")
REP_DEV = ("cir block_repeats: N blocks, N take part, device (text parsed on the %s); parse N ms, "
           "tables upload N ms (N runs twice), build kernel N ms, probe kernel N ms, map kernel "
           "N ms, scan kernel N ms, join to counts N ms, emit and downloads N ms; N extents")
REP_HOST = "cir block_repeats: N blocks, N take part, host; join N ms, map and merge N ms; N extents"
FS_DEV = ("cir file_sources: N files (N blocks) against N pool files (N blocks) of N source(s), "
          "device; frame and buffers N ms, text upload N ms (N bytes), count kernels N ms, emit "
          "kernels N ms, fold kernels N ms, build kernel N ms, probe kernel N ms, verify kernel "
          "N ms, join and download N ms, compact N ms; N candidates")
FS_HOST = ("cir file_sources: N files against N pool files of N source(s), host (why N); N ms; "
           "N candidates")
FC_DEV = ("cir file_copies: N files (N blocks) against N pool files (N blocks) of N source(s), "
          "device; frame and buffers N ms, text upload N ms (N bytes), count kernels N ms, emit "
          "kernels N ms, fold kernels N ms, build kernel N ms, probe kernel N ms, verify kernel "
          "N ms, join and download N ms, compact and decode N ms; N candidates, N skipped, N at "
          "their own path")
FC_HOST = ("cir file_copies: N files against N pool files of N source(s), host (why N); N ms; "
           "N candidates, N skipped, N at their own path")
FP_DEV = ("cir fetch_plan: N files (N blocks) against N pool files (N blocks) of N source(s), "
          "device; frame and buffers N ms, text upload N ms (N bytes), count kernels N ms, emit "
          "kernels N ms, path join N ms, links glue N ms, content join N ms, want glue N ms, joins "
          "and download N ms, block join N ms, extent map N ms, repeat join N ms, repeat map N ms, "
          "tables to counts N ms, extent tail N ms, repeat tail N ms, compact and decode N ms; "
          "N links, N copies, N extents, N repeats, N blocks to fetch")
FP_HOST = ("cir fetch_plan: N files (N blocks) against N pool files of N source(s), host (why N); "
           "N ms; N links, N copies, N extents, N repeats, N blocks to fetch")
# (the host composition makes the four sibling calls with ctx = NULL, in the plan's order)
FP_HOST_LINES = [FS_HOST, FC_HOST, BS_HOST, REP_HOST, FP_HOST]

# call:ctx or null:switch -> the trace lines of that path, in order
PATHS = {
    "block_sources:ctx:": [BS_DEV_PARSE],
    "block_sources:ctx:CIR_SOURCES_PARSE=host": [BS_DEV],
    "block_sources:ctx:CIR_SOURCES_MAP=host": [BS_DEV_PARSE],
    "block_sources:ctx:CIR_SOURCES_MAP=device": [XMAP % "sources", BS_DEV_PARSE],
    "block_sources:ctx:CIR_LINKS_MATCH=host": [BS_DEV_PARSE],
    "block_sources:null:": [BS_HOST],
    "block_extents:ctx:": [XMAP % "extents", BS_DEV_PARSE],
    "block_extents:ctx:CIR_SOURCES_PARSE=host": [BS_DEV],
    "block_extents:ctx:CIR_SOURCES_MAP=host": [BS_DEV_PARSE],
    "block_extents:ctx:CIR_SOURCES_MAP=device": [XMAP % "extents", BS_DEV_PARSE],
    "block_extents:ctx:CIR_LINKS_MATCH=host": [XMAP % "extents", BS_DEV_PARSE],
    "block_extents:null:": [BS_HOST],
    "block_repeats:ctx:": [REP_DEV % "device"],
    "block_repeats:ctx:CIR_SOURCES_PARSE=host": [REP_DEV % "host"],
    "block_repeats:ctx:CIR_SOURCES_MAP=host": [REP_DEV % "device"],
    "block_repeats:ctx:CIR_SOURCES_MAP=device": [REP_DEV % "device"],
    "block_repeats:ctx:CIR_LINKS_MATCH=host": [REP_DEV % "device"],
    "block_repeats:null:": [REP_HOST],
    "file_sources:ctx:": [FS_DEV],
    "file_sources:ctx:CIR_SOURCES_PARSE=host": [FS_DEV],
    "file_sources:ctx:CIR_SOURCES_MAP=host": [FS_DEV],
    "file_sources:ctx:CIR_SOURCES_MAP=device": [FS_DEV],
    "file_sources:ctx:CIR_LINKS_MATCH=host": [FS_HOST],
    "file_sources:null:": [FS_HOST],
    "index_digests:ctx:": [],
    "index_digests:ctx:CIR_SOURCES_PARSE=host": [],
    "index_digests:ctx:CIR_SOURCES_MAP=host": [],
    "index_digests:ctx:CIR_SOURCES_MAP=device": [],
    "index_digests:ctx:CIR_LINKS_MATCH=host": [],
    "index_digests:null:": [],
    "file_copies:ctx:": [FC_DEV],
    "file_copies:ctx:CIR_SOURCES_PARSE=host": [FC_DEV],
    "file_copies:ctx:CIR_SOURCES_MAP=host": [FC_DEV],
    "file_copies:ctx:CIR_SOURCES_MAP=device": [FC_DEV],
    "file_copies:ctx:CIR_LINKS_MATCH=host": [FC_HOST],
    "file_copies:null:": [FC_HOST],
    "fetch_plan:ctx:": [FP_DEV],
    "fetch_plan:ctx:CIR_PLAN=host": FP_HOST_LINES,
    "fetch_plan:null:": FP_HOST_LINES,
}
TRACED = ("cir block_sources:", "cir extents map", "cir block_repeats:", "cir file_sources:",
          "cir file_copies:", "cir fetch_plan:")
# (the paths with a context that an environment switch sends to the host)
HOST_BY_ENV = ("file_sources:ctx:CIR_LINKS_MATCH=host", "file_copies:ctx:CIR_LINKS_MATCH=host",
               "fetch_plan:ctx:CIR_PLAN=host")
# (what differs between the paths of one call by design: where it ran and why)
PATH_STATS = ("on_device", "table_slots", "why_host")


@pytest.fixture(scope="module")
def child():
    """({path: result}, {path: [trace line, ...]}) of the one child."""
    from conftest import ROOT
    env = dict(os.environ, CIR_TRACE="1")
    for k in ("CIR_SOURCES_PARSE", "CIR_SOURCES_MAP", "CIR_LINKS_MATCH", "CIR_PLAN"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + list(PATHS), env=env,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines, at = {}, None
    for ln in p.stderr.decode().splitlines():
        if ln.startswith("path "):
            at = ln[5:]
            lines[at] = []
        elif at is not None and ln.startswith(TRACED):
            lines[at].append(ln)
    return json.loads(p.stdout), lines


def shape(line):
    return re.sub(r"-?\d+(?:\.\d+)?", N, line)


def test_every_path_prints_its_trace_line(child):
    _, lines = child
    assert set(lines) == set(PATHS)
    for path, want in PATHS.items():
        assert [shape(ln) for ln in lines[path]] == want, path


def _without_path_stats(v):
    if isinstance(v, list):
        if len(v) == 2 and isinstance(v[0], str):
            return None if v[0] in PATH_STATS else v
        return [w for w in (_without_path_stats(x) for x in v) if w is not None]
    return v


def test_every_path_gives_the_same_answer(child):
    results, _ = child
    for call in ("block_sources", "block_extents", "block_repeats", "file_sources",
                 "index_digests", "file_copies", "fetch_plan"):
        got = {p: _without_path_stats(r) for p, r in results.items() if p.startswith(call + ":")}
        assert len(got) == (3 if call == "fetch_plan" else 6)
        first = got[call + ":null:"]
        assert first and all(r == first for r in got.values()), call
    # (and the stats that say where it ran)
    st = {p: dict(map(tuple, r[-2] if p.startswith("block_extents") else r[-1]))
          for p, r in results.items() if not p.startswith("index_digests")}
    for p, s in st.items():
        on = s["on_device"]
        if p.endswith(":null:") or p in HOST_BY_ENV:
            assert on == 0, p
        else:
            assert on == 1, p
    assert st["file_sources:ctx:CIR_LINKS_MATCH=host"]["why_host"] == 4
    assert st["file_sources:ctx:"]["why_host"] == st["file_sources:null:"]["why_host"] == 0
    for call in ("file_copies", "fetch_plan"):
        for p, s in st.items():
            if p.startswith(call + ":"):
                assert s["why_host"] == (4 if p in HOST_BY_ENV else 0), p
    # (every array of cir_file_copies with its path bytes was compared above; the plan also
    # against the restatement, in the child)
    assert results["file_copies:null:"][0] and all(
        r[0] is True for p, r in results.items() if p.startswith("fetch_plan:"))


def _lap_names(regex):
    """The alternatives of a LAP expression's first group."""
    pat = regex.pattern
    return pat[1:pat.index(")")].split("|")


def _twice(case, lines):
    """A traced bench child's stderr: the case mark, a warm-up line and one more."""
    return "bench case %s\n" % case + "".join(ln + "\n" for ln in lines + lines)


def test_the_bench_tools_parsers_find_their_laps(child):
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import block_repeats_bench
        import block_sources_bench
        import fetch_plan_bench
        import file_copies_bench
        import file_sources_bench
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    _, lines = child
    # cir block_sources: the laps main() adds up, on the device line's two forms and the host's
    for path in ("block_sources:ctx:", "block_sources:ctx:CIR_SOURCES_PARSE=host"):
        text = _twice("c", lines[path][-1:] + lines["block_sources:null:"])
        laps = block_sources_bench.parse_trace(text)["c"]
        for name in ("parse", "pool", "upload", "build kernel", "probe kernel", "download", "map"):
            assert len(laps["device"][name]) == 1, (path, name)
        for name in ("parse", "pool", "join", "map"):
            assert len(laps["host"][name]) == 1, (path, name)
    laps = block_sources_bench.parse_trace(_twice("c", lines["block_sources:ctx:"]))["c"]["device"]
    for name in ("frame", "text upload", "count kernels", "host parse", "decode kernels",
                 "runs download"):
        assert len(laps[name]) == 1, name
    # cir extents map, of either call
    for path in ("block_sources:ctx:CIR_SOURCES_MAP=device", "block_extents:ctx:"):
        got = block_sources_bench.parse_extents_trace(_twice("c v", lines[path][:1]))["c"]["v"]
        assert sorted(got) == sorted(_lap_names(block_sources_bench.XLAP)), path
        assert all(len(v) == 1 for v in got.values())
    # cir block_repeats:, cir file_sources:, cir file_copies: and cir fetch_plan: on the device
    for mod, path in ((block_repeats_bench, "block_repeats:ctx:"),
                      (block_repeats_bench, "block_repeats:ctx:CIR_SOURCES_PARSE=host"),
                      (file_sources_bench, "file_sources:ctx:"),
                      (file_copies_bench, "file_copies:ctx:"),
                      (fetch_plan_bench, "fetch_plan:ctx:")):
        got = mod.parse_trace(_twice("c", lines[path]))["c"]
        assert sorted(got) == sorted(_lap_names(mod.LAP)), path
        assert all(len(v) == 1 for v in got.values()), path


# ---- a multi-tile text set: ctx against NULL ------------------------------------------

def _text_set():
    """(new index, [three sources]): the sources' lengths differ modulo 16, the
    first is longer than two 4096-byte tiles, the second has a doubled space
    (the device declines it, the host parser takes it), the third a bad hex
    digit (no parser takes it; the decode pass finds it, after the pool was
    laid out).  The new index draws blocks from all three."""
    rng = random.Random(20261020)
    d = [rng.randbytes(32) for _ in range(200)]
    big = _emit([(b"/", [_file(b"big", 131 * BS, d[0:131])]),
                 (b"/d", [_file(b"tail", BS + 9, d[131:133])])])
    mid = _emit([(b"/", [_file(b"m0", 3 * BS, d[140:143]), _file(b"m1", 2 * BS + 1, d[143:146])])])
    bad = _emit([(b"/x", [_file(b"b", 4 * BS, d[150:154])])])
    assert len(big) > 2 * 4096 + 65
    at = mid.index(b" f ")
    mid = mid[:at] + b" " + mid[at:]
    at = bad.index(b" f ") + 20
    assert bad[at:at + 1] in b"0123456789abcdef"
    bad = bad[:at] + b"g" + bad[at + 1:]
    new = _emit([(b"/", [_file(b"n0", 70 * BS, d[60:128] + d[141:143]),
                         _file(b"n1", 3 * BS + 9, d[128:131] + [d[132]]),
                         _file(b"n2", 5 * BS, d[143:145] + d[150:152] + [d[199]])])])
    assert len({len(t) % 16 for t in (big, mid, bad)}) == 3
    return new, [big, mid, bad]


def _clean_set():
    """The same with three well-formed sources, so that cir_file_sources stays
    on the device: files of `new` under their own paths in the sources, and
    one that only the third source holds, under another name."""
    rng = random.Random(20261021)
    d = [rng.randbytes(32) for _ in range(200)]
    f0, f1, f2 = (_file(b"big", 131 * BS, d[0:131]), _file(b"m", 2 * BS + 1, d[140:143]),
                  _file(b"s", BS, [d[150]]))
    new = _emit([(b"/", [f0, f1, f2, _file(b"moved", 2 * BS, d[160:162])])])
    srcs = [_emit([(b"/", [f0, _file(b"s", BS, [d[151]])])]), _emit([(b"/", [f1, f2])]),
            _emit([(b"/", [_file(b"another", 2 * BS, d[160:162]), f2])])]
    assert len({len(t) % 16 for t in srcs}) == 3 and len(srcs[0]) > 2 * 4096 + 65
    return new, srcs


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=gpu._n.CIR_STAGING_LAZY)


def _extents(r):
    return [tuple(getattr(e, f) for f in ("first", "count", "need_file", "need_block", "src",
                                          "src_file", "src_block", "bytes")) for e in r.extents]


def _same_but(a, b, *names):
    return {k: v for k, v in a.items() if k not in names} == \
        {k: v for k, v in b.items() if k not in names}


@pytest.mark.parametrize("make", [_text_set, _clean_set])
def test_multi_tile_text_set_ctx_against_null(gpu, ctx, make):
    new, srcs = make()
    dev, host = gpu.block_sources(new, srcs, context=ctx), gpu.block_sources(new, srcs)
    assert (dev.src, dev.file, dev.block, dev.skipped) == \
        (host.src, host.file, host.block, host.skipped)
    assert _same_but(dev.stats, host.stats, "on_device", "table_slots")
    assert dev.stats["on_device"] == 1 and dev.found > 0
    assert dev.skipped == (1 if make is _text_set else 0)
    assert {s for s in dev.src if s is not None} >= {0, 1}
    dev, host = gpu.block_extents(new, srcs, context=ctx), gpu.block_extents(new, srcs)
    assert (dev.nblk, _extents(dev), bytes(dev.fetch), dev.skipped) == \
        (host.nblk, _extents(host), bytes(host.fetch), host.skipped)
    assert _same_but(dev.stats, host.stats, "on_device", "table_slots")
    assert dev.stats["on_device"] == 1 and len(dev.extents) >= 3
    dev, host = gpu.file_sources(new, srcs, context=ctx), gpu.file_sources(new, srcs)
    assert dev[0] == host[0] == files_cases.expected(new, srcs)[0]
    assert _same_but(dev[1], host[1], "on_device", "table_slots", "why_host")
    if make is _clean_set:
        assert dev[1]["on_device"] == 1 and dev[1]["why_host"] == 0 and len(dev[0]) == 3
    else:
        assert dev[1]["on_device"] == 0 and dev[1]["why_host"] == gpu._n.CIR_FILE_WHY_DECLINED
    # cir_file_copies and cir_fetch_plan: the file-level stage's offsets over the same texts
    declined = gpu._n.CIR_FILE_WHY_DECLINED
    dev, host = gpu.file_copies(new, srcs, ctx), gpu.file_copies(new, srcs)
    assert dev[0] == host[0]
    assert _same_but(dev[1], host[1], "on_device", "table_slots", "why_host")
    plan, hplan = gpu.fetch_plan(new, srcs, ctx), gpu.fetch_plan(new, srcs)
    for field in ("links", "copies", "extents", "repeats", "fetch", "nblk", "skipped"):
        assert getattr(plan, field) == getattr(hplan, field), field
    flat = lambda st: {(k, a): b for k, v in st.items()
                       for a, b in (v.items() if isinstance(v, dict) else [("", v)])
                       if "on_device" not in (k, a) and "table_slots" not in (k, a) and
                       "why_host" not in (k, a)}
    assert flat(plan.stats) == flat(hplan.stats)
    assert hplan.stats["on_device"] == 0 and hplan.stats["why_host"] == 0
    if make is _clean_set:
        assert dev[1]["on_device"] == 1 and dev[1]["why_host"] == 0
        assert dev[0] == copies_restate.expected_copies(new, srcs, None)[0]
        assert (3, 2, 0, b"/another") in dev[0]
        assert plan_restate.same(plan, plan_restate.expected(new, srcs), 1)
        assert plan.stats["why_host"] == 0
        assert len(plan.links) == 3 and plan.copies == [(3, 2, 0, b"/another")]
    else:
        assert dev[1]["on_device"] == 0 and dev[1]["why_host"] == declined
        assert plan.stats["on_device"] == 0 and plan.stats["why_host"] == declined
