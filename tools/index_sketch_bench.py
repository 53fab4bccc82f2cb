#!/usr/bin/env python3
"""What a content sketch costs and what ranking by it buys, timed (one GPU).

(i)  cir_index_sketch with a context on the 1.6 M-block new index of
     tools/fetch_plan_bench.py's case (a), k = 1024 and 4096, against
     cir_index_digests with a context on the same text in the same rounds: the
     sketch call does that call's upload and parse, adds the sketch kernels and
     downloads 8 k bytes of keys where the other downloads 32 bytes per block.
     The order of the three rotates and what each sample followed is kept,
     because the call behind cir_index_digests' 51 MB of returned arrays
     measures slower whichever it is; the two sketch sides are then timed
     among themselves, and ctx = NULL (the host rule) in rounds of its own.
     The sketch kernels' own lap comes from a child process under CIR_TRACE=1.
(ii) case (b)'s 16 sources made unequal for this tool: source j holds the old
     version of a share of the image's files, 5 % to 95 %, and random content in
     the rest (the caller's order is shuffled).  Every index is sketched, the
     sources are ranked by cir_sketch_rank, and cir_fetch_plan runs over all 16
     texts, over the top 4 and over the top 2: per arm the times, the blocks
     left to fetch (the popcount of the fetch bitmap) and the files linked.
     Beside shared / examined the exact containment of every source is
     recorded: the fraction of the new image's distinct digests it holds, from
     the full digest lists (cir_index_digests).  No threshold is set on either.

The mix of changed files in the synthetic image is fetch_plan_bench.py's
assumption, not an observation.  One process, one warm-up of every side, --runs
rounds that alternate the sides, a host clock around whole calls that end in a
synchronise.  Everything goes to profiles/index_sketch/bench.json (--out) as
lists of seconds; the traced child's lines to trace.log beside it.
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import fetch_plan_bench as fpb  # noqa: E402


def unequal_sources(seed, nsrc=16):
    """(new index, [source index], [share of files held]) over case (b)'s image."""
    nfiles, per, _ = fpb.CASES["b"]
    index, (old_text,) = fpb.make_case("a", seed)      # the new version and the old one
    old_lines = re.findall(rb"  f\d{7} f [^\n]*\n", old_text)
    assert len(old_lines) == nfiles
    rng = np.random.default_rng(seed + 1)
    shares = [float(s) for s in rng.permutation(np.linspace(0.05, 0.95, nsrc))]
    sources = []
    for share in shares:
        held = rng.random(nfiles) < share
        lost = np.flatnonzero(~held)
        alt = fpb.tokens(rng, len(lost), per)
        ls = list(old_lines)
        for k, f in enumerate(lost):
            ls[f] = fpb.line(int(f), per, alt[k])
        sources.append(fpb.assemble(ls))
        del alt, ls
    return index, sources, shares


def timed_sketch(n, handle, buf, length, k):
    blob, blob_len = ctypes.c_void_p(), ctypes.c_size_t()
    st = (ctypes.c_uint64 * 6)()
    t0 = time.perf_counter()
    n.check(n.lib.cir_index_sketch(handle, buf, length, k, ctypes.byref(blob),
                                   ctypes.byref(blob_len), st))
    dt = time.perf_counter() - t0
    data = ctypes.string_at(blob.value, blob_len.value)
    n.lib.cir_free(blob)
    return dt, data, list(st)


def timed_digests(n, handle, buf, length, keep=False):
    ht, bs, nblk = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
    dg, rn = ctypes.c_void_p(), ctypes.c_void_p()
    nruns, nfiles = ctypes.c_size_t(), ctypes.c_size_t()
    st = (ctypes.c_uint64 * 4)()
    ref = ctypes.byref
    t0 = time.perf_counter()
    n.check(n.lib.cir_index_digests(handle, buf, length, ref(ht), ref(bs), ref(dg), ref(nblk),
                                    ref(rn), ref(nruns), ref(nfiles), st))
    dt = time.perf_counter() - t0
    d = None
    if keep:
        d = np.frombuffer(ctypes.string_at(dg.value, 32 * nblk.value), dtype=np.uint8).copy()
    n.lib.cir_free(dg)
    n.lib.cir_free(rn)
    return dt, d, list(st)


def distinct(d):
    """The distinct digests of a flat u8 array, as a sorted structured array."""
    return np.unique(d.view(np.dtype([("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("d", "<u8")])))


def cost_part(n, ctx, index, runs, traced):
    buf = ctypes.create_string_buffer(index, len(index))
    out = {"text_bytes": len(index), "seconds": {"sketch_k1024": [], "sketch_k4096": [],
                                                  "index_digests": []},
           "host_seconds": {"sketch_k1024": [], "sketch_k4096": []}}
    blobs = {}
    for k in (1024, 4096):                              # warm-ups, and the answers
        _, blobs[k], st = timed_sketch(n, ctx.handle, buf, len(index), k)
        assert st[0] == 1, st
        out["stats_k%d" % k] = st
    _, _, st = timed_digests(n, ctx.handle, buf, len(index))
    assert st[0] == 1, st
    out["blocks"] = out["stats_k1024"][2]
    if traced:
        for _ in range(runs):
            for k in (1024, 4096):
                timed_sketch(n, ctx.handle, buf, len(index), k)
        return out
    # The order rotates from round to round, and what each sample followed is
    # kept: cir_index_digests hands 51 MB of malloc'd arrays to its caller, and
    # the call that runs right behind their release has measured slower,
    # whichever call it is (tools/fetch_plan_bench.py met the same).
    sides = ["sketch_k1024", "sketch_k4096", "index_digests"]
    out["followed"] = {s: [] for s in sides}
    last = "index_digests"
    for r in range(runs):
        for s in sides[r % 3:] + sides[:r % 3]:
            if s == "index_digests":
                dt = timed_digests(n, ctx.handle, buf, len(index))[0]
            else:
                dt = timed_sketch(n, ctx.handle, buf, len(index), int(s[8:]))[0]
            out["seconds"][s].append(dt)
            out["followed"][s].append(last)
            last = s
    # the two sketch sides alone, behind one call that is not timed
    out["seconds_among_themselves"] = {"sketch_k1024": [], "sketch_k4096": []}
    timed_sketch(n, ctx.handle, buf, len(index), 1024)
    for _ in range(runs):
        for k in (1024, 4096):
            out["seconds_among_themselves"]["sketch_k%d" % k].append(
                timed_sketch(n, ctx.handle, buf, len(index), k)[0])
    for _ in range(min(runs, 3)):
        for k in (1024, 4096):
            dt, blob, st = timed_sketch(n, None, buf, len(index), k)
            assert blob == blobs[k] and st[0] == 0
            out["host_seconds"]["sketch_k%d" % k].append(dt)
    return out


def rank_part(ca, n, ctx, seed, runs, k):
    index, sources, shares = unequal_sources(seed)
    out = {"sources": len(sources), "k": k, "share_of_files_held": shares,
           "text_bytes": len(index) + sum(len(s) for s in sources)}
    t0 = time.perf_counter()
    need = ca.index_sketch(index, ctx, k)
    sk = [ca.index_sketch(s, ctx, k) for s in sources]
    out["sketch_all_seconds"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ranked = ca.sketch_rank(need, sk)
    out["rank_seconds"] = time.perf_counter() - t0
    out["ranked"] = [{"ordinal": o, "shared": sh, "examined": ex} for o, sh, ex in ranked]
    # the exact containment, from the full digest lists
    buf = ctypes.create_string_buffer(index, len(index))
    new_set = distinct(timed_digests(n, ctx.handle, buf, len(index), keep=True)[1])
    exact = []
    for s in sources:
        b = ctypes.create_string_buffer(s, len(s))
        have = distinct(timed_digests(n, ctx.handle, b, len(s), keep=True)[1])
        exact.append(len(np.intersect1d(new_set, have, assume_unique=True)) / len(new_set))
        del b, have
    out["exact_containment"] = exact
    out["estimate"] = {str(o): sh / ex if ex else 0.0 for o, sh, ex in ranked}
    order = [o for o, _, _ in ranked]
    out["order_by_exact"] = sorted(range(len(sources)), key=lambda j: (-exact[j], j))
    arms = {"all_16": list(range(len(sources))), "top_4": order[:4], "top_2": order[:2]}
    calls = {name: fpb.Calls(n, index, [sources[j] for j in pick]) for name, pick in arms.items()}
    out["arms"] = {}
    for name, c in calls.items():                       # warm-ups, and the answers
        _, plan = c.plan(ctx.handle, keep=True)
        assert plan["stats"][42] == 1, plan["stats"][38:]
        out["arms"][name] = {
            "sources": arms[name], "text_bytes": len(index) + sum(len(sources[j])
                                                                  for j in arms[name]),
            "fetch_blocks": int(np.unpackbits(np.frombuffer(plan["fetch"], dtype=np.uint8)).sum()),
            "links": len(plan["links"][0]) // 8, "copies": len(plan["copies"][0]) // 8,
            "extents": len(plan["extents"]) // 64, "nblk": plan["nblk"], "seconds": []}
    for _ in range(runs):
        for name, c in calls.items():
            out["arms"][name]["seconds"].append(c.plan(ctx.handle)[0])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_sketch", "bench.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parts", default="cost,rank")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import ciruela_amd as ca
    n = ca._n
    ctx = ca.Context(device_mask=1, staging_bytes=n.CIR_STAGING_LAZY)
    parts = [p for p in a.parts.split(",") if p]
    result = {"runs": a.runs, "seed": a.seed, "block_size": fpb.BS, "shares": fpb.SHARES}
    if "cost" in parts or a.traced_child:
        index, _ = fpb.make_case("a", a.seed)
        result["cost"] = cost_part(n, ctx, index, a.runs, a.traced_child)
        del index
        if a.traced_child:
            return 0
        print("cost: " + "   ".join("%s %s" % (k, ["%.4f" % s for s in v])
                                     for k, v in result["cost"]["seconds"].items()), flush=True)
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child",
                                "--runs", str(min(a.runs, 3)), "--seed", str(a.seed)],
                               env=dict(os.environ, CIR_TRACE="1"), stdout=subprocess.DEVNULL,
                               stderr=subprocess.PIPE, text=True)
        if child.returncode != 0:
            sys.stderr.write(child.stderr[-4000:])
            return 1
        lines = [ln for ln in child.stderr.splitlines(True) if ln.startswith("cir index_sketch:")]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "trace.log"), "w") as f:
            f.writelines(lines)
        laps = {}
        for ln in lines[2:]:                            # (the two warm-ups dropped)
            k = re.search(r"k (\d+),", ln).group(1)
            for name, ms in re.findall(r"(frame|upload and parse|sketch kernels|sketch and "
                                       r"download) (\d+\.\d+) ms", ln):
                laps.setdefault("k%s" % k, {}).setdefault(name, []).append(float(ms))
        result["cost"]["laps_ms"] = laps
    if "rank" in parts:
        result["rank"] = rank_part(ca, n, ctx, a.seed, a.runs, 1024)
        print("rank: " + "   ".join("%s %s" % (k, ["%.4f" % s for s in v["seconds"]])
                                     for k, v in result["rank"]["arms"].items()), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
