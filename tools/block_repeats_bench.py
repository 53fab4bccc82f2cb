#!/usr/bin/env python3
"""Blocks repeated inside one image, timed (one GPU).

fill_blocks queues one Block per (path, offset) (src/daemon/tracking/
progress.rs:129-170), so a digest that occurs twice inside the new image is
fetched twice; cir_block_repeats joins the index's digests with themselves
instead.  This times the call over synthetic indexes (random digests, files of
64 blocks, no files on disk):

  a  1.6 M blocks, every tenth file a copy of an earlier one
  b  1.6 M blocks, half of them one digest
  c  2,000 blocks, every tenth file a copy of an earlier one

The duplicate fractions are assumptions, not observations of real images.
Each case runs, in one process with the arguments built beforehand, one
warm-up and three timed runs of

  repeats_device   cir_block_repeats with a context
  parent_extents   cir_block_extents(ctx, index, [index]): the parent commit's
                   own code on the same input -- it parses two texts of that
                   size, joins n against n and runs the same four extent
                   kernels -- which is what the device path is measured against
  repeats_host     cir_block_repeats with ctx = NULL (for information only)

and checks that the device and the host give the same output.  The laps of
repeats_device come from a child process that repeats its runs under
CIR_TRACE=1, whose stderr is kept as profiles/block_repeats/trace.log.
Everything goes to profiles/block_repeats/bench.json (--out) as ranges.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from block_sources_bench import PER_FILE, BS, ExtentsCall, make_index  # noqa: E402

CASES = {"a": 1600000, "b": 1600000, "c": 2000}


def make_case(name, seed):
    n = CASES[name]
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if name == "b":      # half of the blocks carry one digest
        d[rng.random(n) < 0.5] = d[0]
    else:                # every tenth file is a copy of an earlier one
        nfiles = n // PER_FILE
        for f in range(9, nfiles, 10):
            src = int(rng.integers(0, f))
            d[f * PER_FILE:(f + 1) * PER_FILE] = d[src * PER_FILE:(src + 1) * PER_FILE]
    return make_index(d, b"n")


class RepeatsCall:
    """cir_block_repeats through ctypes, arguments built once; every block
    wanted, none present."""

    def __init__(self, n, index):
        self.n = n
        self.index = ctypes.create_string_buffer(index, len(index))
        self.len = len(index)
        self.stats = (ctypes.c_uint64 * n.CIR_REPEATS_STATS_FIELDS)()

    def run(self, handle, keep=False):
        n = self.n
        eo, fo = ctypes.c_void_p(), ctypes.c_void_p()
        next_, nblk = ctypes.c_size_t(), ctypes.c_uint64()
        t0 = time.perf_counter()
        n.check(n.lib.cir_block_repeats(handle, ctypes.cast(self.index, ctypes.c_void_p), self.len,
                                        None, None, ctypes.byref(eo), ctypes.byref(next_),
                                        ctypes.byref(fo), ctypes.byref(nblk), self.stats))
        dt = time.perf_counter() - t0
        got = None
        if keep:
            got = (ctypes.string_at(eo.value, 64 * next_.value) if next_.value else b"",
                   ctypes.string_at(fo.value, 8 * ((nblk.value + 63) // 64)))
        for p in (eo, fo):
            n.lib.cir_free(p)
        return dt, got


LAP = re.compile(r"(parse|tables upload|build kernel|probe kernel|map kernel|scan kernel|"
                 r"join to counts|emit and downloads) (\d+\.\d+) ms")


def parse_trace(text):
    """{case: {lap: [ms, ...]}} of the traced child's lines (warm-ups dropped)."""
    out, case, seen = {}, None, 0
    for line in text.splitlines():
        if line.startswith("bench case "):
            case, seen = line.split()[2], 0
            continue
        if not line.startswith("cir block_repeats:") or case is None:
            continue
        seen += 1
        if seen == 1:
            continue
        for name, ms in LAP.findall(line):
            out.setdefault(case, {}).setdefault(name, []).append(float(ms))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_repeats", "bench.json"))
    ap.add_argument("--trace-log", default=None, help="default: trace.log beside --out")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", default="c,a,b")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = [c for c in a.cases.split(",") if c]

    import ciruela_amd as ca
    n = ca._n
    ctx = ca.Context(device_mask=1, staging_bytes=n.CIR_STAGING_LAZY)
    result = {"block_size": BS, "blocks_per_file": PER_FILE, "runs": a.runs, "seed": a.seed,
              "stats_fields": list(ca.RepeatsResult.STATS_FIELDS), "cases": {}}
    for name in names:
        index = make_case(name, a.seed)
        rc = RepeatsCall(n, index)
        out = {"blocks": CASES[name], "index_bytes": len(index), "total_seconds": {}}
        if a.traced_child:
            sys.stderr.write("bench case %s\n" % name)
            sys.stderr.flush()
            for _ in range(a.runs + 1):
                rc.run(ctx.handle)
            continue
        variants = [("repeats_device", rc, ctx.handle),
                    ("parent_extents", ExtentsCall(n, index, [index]), ctx.handle),
                    ("repeats_host", rc, None)]
        kept = {}
        for variant, call, handle in variants:
            _, kept[variant] = call.run(handle, keep=True)     # warm-up, and the output
            out.setdefault("stats", {})[variant] = list(call.stats)
            out["total_seconds"][variant] = [call.run(handle)[0] for _ in range(a.runs)]
            print("%s %-15s %s s" % (name, variant,
                                     ["%.4f" % s for s in out["total_seconds"][variant]]),
                  flush=True)
        assert kept["repeats_device"] == kept["repeats_host"], "device and host differ (%s)" % name
        st = out["stats"]["repeats_device"]
        out.update(repeats=st[1], extents=st[8], left_to_fetch=st[9])
        dev = sorted(out["total_seconds"]["repeats_device"])
        out["device_median_within_the_parent_calls_slowest"] = \
            dev[len(dev) // 2] <= max(out["total_seconds"]["parent_extents"])
        result["cases"][name] = out
        del rc, variants, kept, index
    ctx.close()
    if a.traced_child:
        return 0
    env = dict(os.environ, CIR_TRACE="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child", "--runs",
                            str(a.runs), "--cases", ",".join(names), "--seed", str(a.seed)],
                           env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if child.returncode != 0:
        sys.stderr.write(child.stderr[-4000:])
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = a.trace_log or os.path.join(os.path.dirname(os.path.abspath(a.out)), "trace.log")
    with open(log, "w") as f:      # (the library's lines and the case marks, nothing else)
        f.writelines(l for l in child.stderr.splitlines(True)
                     if l.startswith(("bench case ", "cir")))
    for name, laps in parse_trace(child.stderr).items():
        result["cases"][name]["device_laps_ms"] = laps
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: dict({v: [round(min(t), 4), round(max(t), 4)]
                               for v, t in c["total_seconds"].items()},
                              repeats=c["repeats"], extents=c["extents"],
                              within=c["device_median_within_the_parent_calls_slowest"])
                      for k, c in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
