"""cir_plan_links_dev, cir_plan_want_dev and cir_fetch_plan with a context on
the GPU.

The kernels (ciruela_amd/csrc/plan.hip: k_plan_links, k_plan_want) are the glue
between the four joins of a download plan: one lane per need file or per global
block, a ballot per wave, one aligned 64-bit store per wave.  So the shapes are
the word and workgroup boundaries (63, 64, 65, 255, 256, 257), one shape of
many workgroups, and run tables that put file boundaries on and beside them.
Expected values are written here from the rule's words, block by block; for the
whole call they are plan_restate's, the composition of the four restatements,
never the library's own.

Every case whose new index has a block must be answered by the device
(stats on_device == 1, why_host == 0): a silent fall-back would hide a kernel
bug behind the host's correct answer.  Device calls made directly keep
0xA5-filled guard regions behind their outputs, which must come back untouched.
"""
import bisect
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import plan_cases
import plan_restate
from sources_restate import want_words

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
POISON = 0xA5
GUARD = 256
NOSRC = (1 << 32) - 1
BS = 64


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=gpu._n.CIR_STAGING_LAZY)


class Poisoned:
    """nbytes of device memory filled with 0xA5 and GUARD more behind them."""

    def __init__(self, torch, nbytes):
        self.n = nbytes
        self.t = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def guard_intact(self):
        return bool((self.t[self.n:] == POISON).all().item())

    def host(self, dtype):
        return self.t[:self.n].cpu().numpy().view(dtype)


def up(torch, arr):
    """A numpy array in device memory (at least 16 bytes, so never a null pointer)."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.zeros(max(raw.size, 16), dtype=torch.uint8, device="cuda")
    t[:raw.size] = torch.from_numpy(raw.copy())
    return t


def bits_to_words(bits, nwords, tail_ones=False):
    words = [0] * nwords
    for g, b in enumerate(bits):
        if b:
            words[g >> 6] |= 1 << (g & 63)
    if tail_ones:
        for g in range(len(bits), 64 * nwords):
            words[g >> 6] |= 1 << (g & 63)
    return np.array(words, dtype=np.uint64)


# ---- cir_plan_want_dev ---------------------------------------------------------------------

def run_table(blocks_per_file, n, bs=BS):
    """Files of the given block counts, in order, cut off at n blocks: (runs
    [(first, size, file, 0)], n_files).  A file of 0 blocks takes an ordinal
    and no run."""
    runs, at = [], 0
    for f, nb in enumerate(blocks_per_file):
        nb = min(nb, n - at)
        if nb > 0:
            runs.append((at, nb * bs - (f % 3) * (bs // 4), f, 0))   # (short last blocks too)
            at += nb
    return runs, len(blocks_per_file)


def layout(kind, n):
    if kind == "ones":
        return [1] * n
    if kind == "seventy":
        return [70] * (n // 70 + 1)
    per = []                       # "mixed": 70-block files, empty files between, single blocks
    while sum(per) < n:
        per += [70, 0, 1, 0, 0, 63, 2]
    return per


def expect_want(runs, n, bs, n_files, ca, cb, have):
    """The rule's words, block by block: (want bits, [wanted, linked, have])."""
    firsts = [r[0] for r in runs]
    bits, res = [], [0, 0, 0]
    for g in range(n):
        i = bisect.bisect_right(firsts, g) - 1
        cls = None
        if i >= 0:
            first, size, f, _ = runs[i]
            if g - first < size // bs + (1 if size % bs else 0):
                linked = f < n_files and ((ca is not None and ca[f] != NOSRC) or
                                          (cb is not None and cb[f] != NOSRC))
                cls = 1 if linked else 2 if have is not None and have[g] else 0
        bits.append(1 if cls == 0 else 0)
        if cls is not None:
            res[cls] += 1
    return bits, res


def call_want(gpu, torch, ctx, runs, n, bs, n_files, ca, cb, have_words):
    nwords = (n + 63) // 64
    d_runs = up(torch, np.array(runs, dtype=np.uint64).reshape(-1, 4))
    d_a = None if ca is None else up(torch, np.array(ca, dtype=np.uint32))
    d_b = None if cb is None else up(torch, np.array(cb, dtype=np.uint32))
    d_have = None if have_words is None else up(torch, have_words)
    want, res = Poisoned(torch, 8 * nwords), Poisoned(torch, 24)
    ctx.plan_want_dev(d_runs.data_ptr() if runs else 0, len(runs), n, bs, n_files, want.ptr,
                      res.ptr, d_a.data_ptr() if d_a is not None else 0,
                      d_b.data_ptr() if d_b is not None else 0,
                      d_have.data_ptr() if d_have is not None else 0,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert want.guard_intact() and res.guard_intact()
    return want.host(np.uint64), [int(x) for x in res.host(np.uint64)]


def linked_patterns(runs, n_files):
    """none / all / alternate / the files at the word and workgroup boundaries."""
    at_edges = set()
    firsts = [r[0] for r in runs]
    for g in (0, 63, 64, 65, 255, 256, 257):
        i = bisect.bisect_right(firsts, g) - 1
        if i >= 0:
            at_edges.add(runs[i][2])
    return {"none": set(), "all": set(range(n_files)), "alternate": set(range(0, n_files, 2)),
            "edges": at_edges}


@pytest.mark.parametrize("kind", ["ones", "seventy", "mixed"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_want_shapes(gpu, ctx, n, kind):
    import torch
    rng = random.Random(1000 * n + len(kind))
    runs, n_files = run_table(layout(kind, n), n)
    nwords = (n + 63) // 64
    haves = {"absent": None, "all_ones_and_past_n": [1] * n,
             "random": [int(rng.random() < 0.4) for _ in range(n)]}
    cases = 0
    for pname, linked in linked_patterns(runs, n_files).items():
        full = [7 if f in linked else NOSRC for f in range(n_files)]
        half_a = [7 if f in linked and f % 4 < 2 else NOSRC for f in range(n_files)]
        half_b = [9 if f in linked and f % 4 >= 1 else NOSRC for f in range(n_files)]
        for ca, cb in ((full, None), (None, full), (half_a, half_b)):
            for hname, have in haves.items():
                if n > 1000 and (pname, hname) not in (("alternate", "random"), ("edges", "absent"),
                                                       ("none", "all_ones_and_past_n")):
                    continue           # (the large shape: a few combinations, it adds workgroups)
                hw = None if have is None else bits_to_words(have, max(nwords, 1),
                                                             tail_ones=hname.startswith("all"))
                bits, res = expect_want(runs, n, BS, n_files, ca, cb, have)
                got, gres = call_want(gpu, torch, ctx, runs, n, BS, n_files, ca, cb, hw)
                assert bytes(got) == bytes(want_words(bits)), (pname, hname)
                assert gres == res, (pname, hname, gres, res)
                cases += 1
    assert cases >= 9


def test_want_lying_tables(gpu, ctx):
    """Sorted tables that lie get the answer the rule's words define."""
    import torch
    n, n_files = 300, 4
    cand = [5, NOSRC, 5, 5]
    # an ordinal >= n_files is not linked (and cand[] is not read there); a
    # `first` >= n_blocks covers nothing; a size of 2^64 - 1 covers every block
    # up to the next run's first
    runs = [(0, 10 * BS, 0, 0), (10, 5 * BS, 1 << 40, 0), (20, U64, 2, 0), (100, U64, 1, 0),
            (250, 3 * BS, U64, 0), (300, 64 * BS, 0, 0), (1 << 33, BS, 0, 0)]
    bits, res = expect_want(runs, n, BS, n_files, cand, None, None)
    assert bits[:10] == [0] * 10 and bits[10:15] == [1] * 5 and bits[15:20] == [0] * 5
    assert bits[20:100] == [0] * 80 and bits[100:250] == [1] * 150
    assert bits[250:253] == [1] * 3 and bits[253:] == [0] * 47
    assert res == [158, 90, 0]
    for ca, cb in ((cand, None), (None, cand), (cand, cand)):
        got, gres = call_want(gpu, torch, ctx, runs, n, BS, n_files, ca, cb, None)
        assert bytes(got) == bytes(want_words(bits)) and gres == res
    # bs = 1 and the largest size: size / bs + (size % bs != 0) does not wrap
    runs = [(0, U64, 0, 0)]
    got, gres = call_want(gpu, torch, ctx, runs, 130, 1, 1, None, None, None)
    assert bytes(got) == bytes(want_words([1] * 130)) and gres == [130, 0, 0]
    # no run at all, and no file
    got, gres = call_want(gpu, torch, ctx, [], 65, BS, 0, None, None, None)
    assert bytes(got) == bytes(16) and gres == [0, 0, 0]


# ---- cir_plan_links_dev --------------------------------------------------------------------

@pytest.mark.parametrize("n_files", [0, 1, 63, 64, 65, 257])
def test_links_shapes(gpu, ctx, n_files):
    import torch
    rng = random.Random(77 + n_files)
    nwords = (n_files + 63) // 64
    for deny_kind in ("absent", "random", "all_and_past_n"):
        src = [rng.randrange(5) if rng.random() < 0.5 else NOSRC for _ in range(n_files)]
        if n_files:
            src[0] = 3                      # (a denied file with a candidate at the first bit)
            src[-1] = 3 if n_files % 2 else NOSRC
        file = [rng.randrange(1000) if s != NOSRC else U64 for s in src]
        deny = {"absent": None, "random": [int(rng.random() < 0.5) for _ in range(n_files)],
                "all_and_past_n": [1] * n_files}[deny_kind]
        if deny_kind == "random" and n_files:
            deny[0] = 1
        d_src, d_file = Poisoned(torch, 4 * n_files), Poisoned(torch, 8 * n_files)
        if n_files:
            d_src.t[:4 * n_files] = torch.from_numpy(
                np.array(src, dtype=np.uint32).view(np.uint8).copy())
            d_file.t[:8 * n_files] = torch.from_numpy(
                np.array(file, dtype=np.uint64).view(np.uint8).copy())
        d_deny = None if deny is None else up(
            torch, bits_to_words(deny, max(nwords, 1), tail_ones=deny_kind.startswith("all")))
        skip, res = Poisoned(torch, 8 * nwords), Poisoned(torch, 16)
        ctx.plan_links_dev(d_src.ptr, d_file.ptr, n_files, skip.ptr, res.ptr,
                           d_deny.data_ptr() if d_deny is not None else 0,
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for p in (d_src, d_file, skip, res):
            assert p.guard_intact()
        denied = [bool(deny and deny[i]) for i in range(n_files)]
        want_src = [NOSRC if denied[i] else src[i] for i in range(n_files)]
        want_file = [U64 if denied[i] and src[i] != NOSRC else file[i] for i in range(n_files)]
        want_skip = [int(denied[i] or src[i] != NOSRC) for i in range(n_files)]
        assert [int(x) for x in d_src.host(np.uint32)] == want_src
        assert [int(x) for x in d_file.host(np.uint64)] == want_file
        assert bytes(skip.host(np.uint64)) == bytes(want_words(want_skip))
        kept = sum(1 for s in want_src if s != NOSRC)
        gone = sum(1 for i in range(n_files) if denied[i] and src[i] != NOSRC)
        assert [int(x) for x in res.host(np.uint64)] == [kept, gone]
        if deny_kind == "random" and n_files >= 63:      # (denied with and without a candidate)
            assert gone and any(denied[i] and src[i] == NOSRC for i in range(n_files))


# ---- the whole call ------------------------------------------------------------------------

PATH_STATS = ("table_slots", "on_device", "why_host")


def strip(stats):
    return {k: ({a: b for a, b in v.items() if a not in PATH_STATS} if isinstance(v, dict) else v)
            for k, v in stats.items() if k not in PATH_STATS}


def planned(gpu, ctx, index, sources, deny, have):
    """cir_fetch_plan with a context equals the restatement and the host
    composition; returns the device call's result."""
    want = plan_restate.expected(index, sources, deny, have)
    hb = None if have is None else bytes(want_words(have))
    got = gpu.fetch_plan(index, sources, ctx, deny=deny, have=hb)
    assert plan_restate.same(got, want), (got, got.stats)
    host = gpu.fetch_plan(index, sources, None, deny=deny, have=hb)
    assert plan_restate.same(host, want, 0)
    for field in ("links", "copies", "extents", "repeats", "fetch", "nblk", "skipped"):
        assert getattr(got, field) == getattr(host, field), field
    assert strip(got.stats) == strip(host.stats)
    return got, want


def on_device(gpu, got):
    st = got.stats
    ok = st["on_device"] == 1 and st["why_host"] == 0
    if ok:
        for part in ("sources", "copies", "extents", "repeats"):
            assert st[part]["on_device"] == 1, part
        assert st["extents"]["table_slots"] == \
            gpu._n.lib.cir_match_table_slots(st["extents"]["pool_blocks"])
        assert st["repeats"]["table_slots"] == gpu._n.lib.cir_match_table_slots(got.nblk)
    return ok


@pytest.mark.parametrize("case", plan_cases.families(), ids=lambda c: c[0])
def test_families(gpu, ctx, case):
    name, index, sources, deny, have = case
    got, want = planned(gpu, ctx, index, sources, deny, have)
    if want["nblk"]:
        assert on_device(gpu, got), got.stats
    else:
        assert got.stats["on_device"] == 0
        assert got.stats["why_host"] == gpu._n.CIR_PLAN_WHY_EMPTY


def test_hand_made_counts(gpu, ctx):
    new, olds = plan_cases.hand_made()
    got, _ = planned(gpu, ctx, new, olds, None, None)
    hm = plan_cases.HAND_MADE
    assert on_device(gpu, got)
    assert (got.nblk, len(got.links), len(got.copies), len(got.extents), len(got.repeats)) == \
        (hm["nblk"], hm["links"], hm["copies"], hm["extents"], hm["repeats"])
    assert got.repeats[0].count == hm["repeat_blocks"] and got.repeats[0].src == hm["repeat_src"]
    assert got.left_to_fetch() == hm["fetch"]
    got, _ = planned(gpu, ctx, new, olds, [0], None)
    assert (len(got.links), len(got.extents)) == (plan_cases.HAND_MADE_DENY0["links"],
                                                  plan_cases.HAND_MADE_DENY0["extents"])
    fam = {name: rest for name, *rest in plan_cases.families()}
    got, _ = planned(gpu, ctx, *fam["have_and_its_twin"])
    assert [e.src for e in got.repeats] == [0]


@pytest.mark.parametrize("chunk", range(4))
def test_random_sweep(gpu, ctx, chunk):
    for seed in range(50 * chunk, 50 * chunk + 50):
        index, sources, deny, have = plan_cases.random_case(seed)
        got, want = planned(gpu, ctx, index, sources, deny, have)
        if want["nblk"]:
            assert on_device(gpu, got), (seed, got.stats)
        else:
            assert got.stats["why_host"] == gpu._n.CIR_PLAN_WHY_EMPTY


def test_at_least_158_seeds_on_device(gpu, ctx):
    """42 of the 200 seeds have no block or no usable source; the others, at
    the least, are planned on the device."""
    answered = 0
    for seed in range(200):
        index, sources, deny, have = plan_cases.random_case(seed)
        hb = None if have is None else bytes(want_words(have))
        st = gpu.fetch_plan(index, sources, ctx, deny=deny, have=hb).stats
        answered += st["on_device"] == 1 and st["why_host"] == 0
    assert answered >= 158, answered


def big_text_family(gpu):
    """A source text that crosses cir_debug_index_tile_bytes() many times and
    more than cir_debug_extent_tile_blocks() need blocks."""
    rng = random.Random(4242)
    tile_bytes = int(gpu._n.lib.cir_debug_index_tile_bytes())
    tile_blocks = int(gpu._n.lib.cir_debug_extent_tile_blocks())
    f, emit, at = plan_cases.f, plan_cases.emit, plan_cases.at
    files = [f(rng, b"f%03d" % i, 70 if i % 5 else 33) for i in range(tile_blocks // 70 + 8)]
    changed = []
    for i, e in enumerate(files):
        if i % 7 == 3:                                   # one block changed
            d = list(e[4])
            d[len(d) // 2] = rng.randbytes(32)
            e = ("f", e[1], e[2], e[3], d)
        changed.append(e)
    old = emit([(b"/v1", files[:20]), (b"/keep", files[20:])])
    new = emit([(b"/v2", changed[:20]), (b"/keep", changed[20:]),
                (b"/twice", [at(changed[3], b"again"), f(rng, b"fresh", 9)])])
    assert len(old) > 3 * tile_bytes
    return new, [old], tile_blocks


def test_past_the_tiles(gpu, ctx):
    new, olds, tile_blocks = big_text_family(gpu)
    have = [int(g % 11 == 0) for g in range(tile_blocks + 100)]
    for deny, hv in ((None, None), ([0, 21, 22], have)):
        got, want = planned(gpu, ctx, new, olds, deny, hv)
        assert want["nblk"] > tile_blocks and on_device(gpu, got)
        assert all(plan_restate.reach(want)), plan_restate.reach(want)


def test_declined_text_falls_back(gpu, ctx):
    """Two spaces between tokens: the host parser takes the line, the device
    declines it; the host composition answers, with the reason."""
    new, olds = plan_cases.hand_made()
    double = olds[0].replace(b"  tool x ", b"  tool  x ")
    assert double != olds[0]
    want = plan_restate.expected(new, olds)      # (the line means what it meant)
    got = gpu.fetch_plan(new, [double], ctx)
    assert plan_restate.same(got, want, 0)
    host = gpu.fetch_plan(new, [double], None)
    assert plan_restate.same(host, want, 0) and strip(got.stats) == strip(host.stats)
    assert got.stats["on_device"] == 0
    assert got.stats["why_host"] == gpu._n.CIR_FILE_WHY_DECLINED


def test_errors_leave_nothing(gpu, ctx):
    with pytest.raises(gpu.CiruelaError) as e:
        gpu.fetch_plan(b"not an index\n", [], ctx)
    assert e.value.status == gpu._n.CIR_EPARSE


CHILD = r"""
import os
import sys
sys.path[:0] = [%r, %r, %r]
import ciruela_amd as ca
import plan_cases, plan_restate
ctx = ca.Context(device_mask=1, staging_bytes=ca._n.CIR_STAGING_LAZY)
new, olds = plan_cases.hand_made()
mode = sys.argv[1]
if mode == "trace":
    sys.stderr.flush()
    print("BEGIN", file=sys.stderr, flush=True)
    r = ca.fetch_plan(new, olds + [b"garbage"], ctx)
    print("END", file=sys.stderr, flush=True)
    assert r.stats["on_device"] == 1
    print(len(new) + sum(len(o) for o in olds))
else:
    for want_host in (True, False, True):      # (read per call)
        if want_host:
            os.environ["CIR_PLAN"] = "host"
        else:
            del os.environ["CIR_PLAN"]
        r = ca.fetch_plan(new, olds, ctx)
        assert plan_restate.same(r, plan_restate.expected(new, olds))
        print(r.stats["on_device"], r.stats["why_host"])
"""


def child(mode, env):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    p = subprocess.run([sys.executable, "-c", code, mode], capture_output=True, timeout=300,
                       env=dict(os.environ, **env))
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_trace_in_a_child(gpu):
    """One `cir fetch_plan:` line, the texts' own bytes uploaded once, and no
    line of a sibling whole call: the plan goes through none of them."""
    p = child("trace", {"CIR_TRACE": "1"})
    err = p.stderr.decode(errors="replace")
    body = err[err.index("BEGIN"):err.index("END")]
    lines = [ln for ln in body.split("\n") if ln.startswith("cir fetch_plan:")]
    assert len(lines) == 1, body
    m = re.search(r"text upload [0-9.]+ ms \((\d+) bytes\)", lines[0])
    assert m and int(m.group(1)) == int(p.stdout.split()[0]), lines[0]
    for sibling in ("cir file_sources:", "cir file_copies:", "cir block_extents:",
                    "cir block_sources:", "cir block_repeats:"):
        assert sibling not in body, sibling
    for lap in ("count kernels", "emit kernels", "path join", "content join", "block join",
                "repeat join", "extent tail", "repeat tail", "compact and decode"):
        assert lap in lines[0], lap


def test_fallback_by_environment_in_a_child(gpu):
    p = child("env", {"CIR_PLAN": "host"})
    assert p.stdout.split() == b"0 4 1 0 0 4".split(), p.stdout


def test_cli_plan(gpu, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    new, olds = plan_cases.hand_made()
    paths = []
    for k, data in enumerate([new] + olds):
        p = tmp_path / ("i%d.ds1" % k)
        p.write_bytes(data)
        paths.append(str(p))
    outs = []
    for extra in ([], ["--host"]):
        p = subprocess.run([cli, "plan"] + paths + extra, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        assert (b"planned on the host" if extra else b"planned on the device") in p.stderr
        outs.append(p.stdout)
    assert outs[0] == outs[1]
    assert b"link 2 files" in outs[0] and b"fetch 9 blocks" in outs[0]
