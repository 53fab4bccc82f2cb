#!/usr/bin/env python3
"""Hardlink candidates matched by content, timed (one GPU).

cir_file_copies finds the files of a new image that an older image holds
unchanged at another path: the new index's texts are parsed and the files
joined by {size, exe, fold of the digests} on the GPU, or, without a context,
by the host rule (the host parser and one hash map of contents).  This times
both over synthetic indexes (random digests, no files on disk) in which every
directory was renamed between the versions (/v1/dNNNNN became /v2/dNNNNN), so
that the same-path rule finds nothing and every candidate is a moved file:

  a  1.6 M blocks in 20,000 files of 80 against 1 source
  b  the same against 16 sources
  c  200,000 one-block files against 4 sources
  d  50 files of 16 blocks against 1 source

Every source is an older version of the new index with a different tenth of
the files changed, so hits and misses both occur.  Each case runs, in one
process with the arguments built beforehand, one warm-up of each call and then
--runs rounds that alternate

  host     cir_file_copies(NULL, ...): the host rule
  device   cir_file_copies(ctx, ...)
  sources  cir_file_sources(ctx, ...) on the same input: unchanged code, as a
           scale (the same parse, a join keyed by path, a smaller download;
           here it finds no candidate)

with a host clock around each whole (synchronising) call, and checks that host
and device give the same five arrays and that the device answered (stats[6] ==
1).  The laps of the device call come from a child process that repeats its
runs under CIR_TRACE=1, whose stderr is kept as profiles/file_copies/trace.log.
Everything goes to profiles/file_copies/bench.json (--out) as lists of seconds.
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

from file_sources_bench import BS, PER_DIR, file_lines  # noqa: E402

# name: (files, blocks per file, sources)
CASES = {"a": (20000, 80, 1), "b": (20000, 80, 16), "c": (200000, 1, 4), "d": (50, 16, 1)}


def assemble(lines, version):
    out = [b"DIRSIGNATURE.v1 blake2b/256 block_size=%d\n/\n/%s\n" % (BS, version)]
    for at in range(0, len(lines), PER_DIR):
        out.append(b"/%s/d%05d\n" % (version, at // PER_DIR))
        out += lines[at:at + PER_DIR]
    out.append(b"00" * 32 + b"\n")
    return b"".join(out)


def make_case(name, seed):
    """(index, [source index, ...], expected candidates): source j is the new
    index below another directory, with the files f, f % 10 == j % 10, given
    other content."""
    nfiles, per, nsrc = CASES[name]
    rng = np.random.default_rng(seed)
    lines = file_lines(rng, nfiles, per)
    sources = []
    for j in range(nsrc):
        changed = list(range(j % 10, nfiles, 10))
        alt = file_lines(rng, len(changed), per)
        ls = list(lines)
        for k, f in enumerate(changed):
            ls[f] = b"  f%07d" % f + alt[k][alt[k].index(b" f "):]
        sources.append(assemble(ls, b"v1"))
    hits = nfiles if nsrc >= 2 else nfiles - len(range(0, nfiles, 10))
    return assemble(lines, b"v2"), sources, hits


class Call:
    """cir_file_copies / cir_file_sources through ctypes, arguments built once."""

    def __init__(self, n, index, sources):
        self.n = n
        self.index = ctypes.create_string_buffer(index, len(index))
        self.len = len(index)
        self.bufs = [ctypes.create_string_buffer(s, len(s)) for s in sources]
        k = len(sources)
        self.sp = (ctypes.c_void_p * k)(*[ctypes.cast(b, ctypes.c_void_p) for b in self.bufs])
        self.sl = (ctypes.c_size_t * k)(*[len(s) for s in sources])
        self.k = k
        self.stats = (ctypes.c_uint64 * n.CIR_FILE_COPIES_STATS_FIELDS)()
        self.fstats = (ctypes.c_uint64 * n.CIR_FILE_SOURCES_STATS_FIELDS)()

    def copies(self, handle, keep=False):
        n = self.n
        outs = [ctypes.c_void_p() for _ in range(5)]
        cnt, sk = ctypes.c_size_t(), ctypes.c_size_t()
        ip = ctypes.cast(self.index, ctypes.c_void_p)
        t0 = time.perf_counter()
        n.check(n.lib.cir_file_copies(handle, ip, self.len, self.sp, self.sl, self.k, None,
                                      *[ctypes.byref(o) for o in outs], ctypes.byref(cnt),
                                      ctypes.byref(sk), self.stats))
        dt = time.perf_counter() - t0
        got = None
        if keep and cnt.value:
            k = cnt.value
            offs = ctypes.string_at(outs[3].value, 8 * (k + 1))
            total = int(np.frombuffer(offs, dtype=np.uint64)[-1])
            got = (ctypes.string_at(outs[0].value, 8 * k), ctypes.string_at(outs[1].value, 4 * k),
                   ctypes.string_at(outs[2].value, 8 * k), offs,
                   ctypes.string_at(outs[4].value, total))
        for p in outs:
            n.lib.cir_free(p)
        return dt, got, cnt.value

    def sources(self, handle):
        n = self.n
        f, s, cnt, sk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        ip = ctypes.cast(self.index, ctypes.c_void_p)
        t0 = time.perf_counter()
        n.check(n.lib.cir_file_sources(handle, ip, self.len, self.sp, self.sl, self.k,
                                       ctypes.byref(f), ctypes.byref(s), ctypes.byref(cnt),
                                       ctypes.byref(sk), self.fstats))
        dt = time.perf_counter() - t0
        for p in (f, s):
            n.lib.cir_free(p)
        return dt, cnt.value


LAP = re.compile(r"(frame and buffers|text upload|count kernels|emit kernels|fold kernels|"
                 r"build kernel|probe kernel|verify kernel|join and download|compact and decode) "
                 r"(\d+\.\d+) ms")


def parse_trace(text):
    """{case: {lap: [ms, ...]}} of the traced child's lines (warm-ups dropped)."""
    out, case, seen = {}, None, 0
    for line in text.splitlines():
        if line.startswith("bench case "):
            case, seen = line.split()[2], 0
            continue
        if not line.startswith("cir file_copies:") or case is None:
            continue
        seen += 1
        if seen == 1:
            continue
        for name, ms in LAP.findall(line):
            out.setdefault(case, {}).setdefault(name, []).append(float(ms))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "file_copies", "bench.json"))
    ap.add_argument("--trace-log", default=None, help="default: trace.log beside --out")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", default="d,c,a,b")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = [c for c in a.cases.split(",") if c]

    import ciruela_amd as ca
    n = ca._n
    ctx = ca.Context(device_mask=1, staging_bytes=n.CIR_STAGING_LAZY)
    result = {"block_size": BS, "runs": a.runs, "seed": a.seed,
              "stats_fields": list(ca.FILE_COPIES_STATS), "cases": {}}
    for name in names:
        index, sources, hits = make_case(name, a.seed)
        call = Call(n, index, sources)
        nfiles, per, nsrc = CASES[name]
        out = {"files": nfiles, "blocks": nfiles * per, "sources": nsrc,
               "text_bytes": len(index) + sum(len(s) for s in sources),
               "total_seconds": {"host": [], "device": [], "sources": []}}
        if a.traced_child:
            sys.stderr.write("bench case %s\n" % name)
            sys.stderr.flush()
            for _ in range(a.runs + 1):
                call.copies(ctx.handle)
            continue
        _, host, cnt = call.copies(None, keep=True)           # warm-ups, and the outputs
        _, dev, _ = call.copies(ctx.handle, keep=True)
        assert host == dev and cnt == hits, "device and host differ (%s)" % name
        assert call.stats[6] == 1 and call.stats[7] == 0 and call.stats[9] == 0, list(call.stats)
        out["stats"] = list(call.stats)
        _, same_path = call.sources(ctx.handle)
        assert same_path == 0 and call.fstats[6] == 1, list(call.fstats)
        for _ in range(a.runs):
            out["total_seconds"]["host"].append(call.copies(None)[0])
            out["total_seconds"]["device"].append(call.copies(ctx.handle)[0])
            out["total_seconds"]["sources"].append(call.sources(ctx.handle)[0])
        print("%-3s " % name + "   ".join(
            "%s %s s" % (k, ["%.4f" % s for s in v]) for k, v in out["total_seconds"].items()),
            flush=True)
        out["candidates"] = cnt
        result["cases"][name] = out
        del call, index, sources
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
    print(json.dumps({k: {v: [round(min(t), 4), round(max(t), 4)]
                          for v, t in c["total_seconds"].items()}
                      for k, c in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
