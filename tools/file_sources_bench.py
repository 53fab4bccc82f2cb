#!/usr/bin/env python3
"""Hardlink candidates matched on the device, timed (one GPU).

scan_links (src/daemon/metadata/hardlink_sources.rs:107-153) walks the new
index and every older one on a host thread; cir_link_candidates restates it
with the host parser and a hash map per source, and cir_file_sources parses
the texts and joins the files on the GPU.  This times both over synthetic
indexes (random digests, no files on disk):

  a  1.6 M blocks in 20,000 files of 80 against 1 source
  b  the same against 16 sources
  c  200,000 one-block files against 4 sources
  s50 .. s5000  the size sweep: n files of 16 blocks against 1 source

Every source is an older version of the new index with a different tenth of
the files changed, so hits and misses both occur.  Each case runs, in one
process with the arguments built beforehand, one warm-up of each call and then
--runs rounds that alternate

  host    cir_link_candidates: the parent commit's parse, maps and loop (it
          gained three counters for cir_file_sources' stats)
  device  cir_file_sources with a context

with a host clock around each whole (synchronising) call, and checks that both
give the same pairs and that the device answered (stats[6] == 1).  The laps of
the device call -- text upload, count and emit kernels, and the join's kernels
from the stream's events -- come from a child process that repeats its runs
under CIR_TRACE=1, whose stderr is kept as profiles/file_sources/trace.log.
`ciruela-index candidates` is timed end to end both ways on case a (process
start, reading the index files and opening the device included), and
`ciruela-index links` likewise against an empty source directory, so that its
check finds no file to read: what differs between its two runs is the
candidates step alone.  Everything goes to profiles/file_sources/bench.json
(--out) as lists of seconds.
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BS = 32768
_HEX = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
# name: (files, blocks per file, sources)
CASES = {"a": (20000, 80, 1), "b": (20000, 80, 16), "c": (200000, 1, 4),
         "s50": (50, 16, 1), "s200": (200, 16, 1), "s1000": (1000, 16, 1), "s5000": (5000, 16, 1)}
PER_DIR = 100


def file_lines(rng, nfiles, per, first=0):
    """The lines of nfiles files of `per` random blocks, as a list of bytes."""
    d = rng.integers(0, 256, size=(nfiles * per, 32), dtype=np.uint8)
    text = np.empty((nfiles * per, 65), dtype=np.uint8)
    text[:, 0] = 0x20
    text[:, 1::2] = _HEX[d >> 4]
    text[:, 2::2] = _HEX[d & 15]
    flat = text.reshape(nfiles, per * 65)
    return [b"  f%07d f %d%s\n" % (first + f, per * BS, flat[f].tobytes()) for f in range(nfiles)]


def assemble(lines):
    out = [b"DIRSIGNATURE.v1 blake2b/256 block_size=%d\n" % BS]
    for at in range(0, len(lines), PER_DIR):
        out.append(b"/\n" if at == 0 else b"/d%05d\n" % (at // PER_DIR))
        out += lines[at:at + PER_DIR]
    out.append(b"00" * 32 + b"\n")
    return b"".join(out)


def make_case(name, seed):
    """(index, [source index, ...], expected candidates): source j is the new
    index with the files f, f % 10 == j % 10, given other content."""
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
        sources.append(assemble(ls))
    hits = nfiles if nsrc >= 2 else nfiles - len(range(0, nfiles, 10))
    return assemble(lines), sources, hits


class Call:
    """cir_link_candidates / cir_file_sources through ctypes, arguments built once."""

    def __init__(self, n, index, sources):
        self.n = n
        self.index = ctypes.create_string_buffer(index, len(index))
        self.len = len(index)
        self.bufs = [ctypes.create_string_buffer(s, len(s)) for s in sources]
        k = len(sources)
        self.sp = (ctypes.c_void_p * k)(*[ctypes.cast(b, ctypes.c_void_p) for b in self.bufs])
        self.sl = (ctypes.c_size_t * k)(*[len(s) for s in sources])
        self.k = k
        self.stats = (ctypes.c_uint64 * n.CIR_FILE_SOURCES_STATS_FIELDS)()

    def run(self, handle, host_call, keep=False):
        n = self.n
        f, s, cnt, sk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        ip = ctypes.cast(self.index, ctypes.c_void_p)
        t0 = time.perf_counter()
        if host_call:
            n.check(n.lib.cir_link_candidates(ip, self.len, self.sp, self.sl, self.k, ctypes.byref(f),
                                              ctypes.byref(s), ctypes.byref(cnt), ctypes.byref(sk)))
        else:
            n.check(n.lib.cir_file_sources(handle, ip, self.len, self.sp, self.sl, self.k,
                                           ctypes.byref(f), ctypes.byref(s), ctypes.byref(cnt),
                                           ctypes.byref(sk), self.stats))
        dt = time.perf_counter() - t0
        got = None
        if keep:
            got = (ctypes.string_at(f.value, 8 * cnt.value) if cnt.value else b"",
                   ctypes.string_at(s.value, 4 * cnt.value) if cnt.value else b"")
        for p in (f, s):
            n.lib.cir_free(p)
        return dt, got, cnt.value


LAP = re.compile(r"(frame and buffers|text upload|count kernels|emit kernels|fold kernels|"
                 r"build kernel|probe kernel|verify kernel|join and download|compact) (\d+\.\d+) ms")


def parse_trace(text):
    """{case: {lap: [ms, ...]}} of the traced child's lines (warm-ups dropped)."""
    out, case, seen = {}, None, 0
    for line in text.splitlines():
        if line.startswith("bench case "):
            case, seen = line.split()[2], 0
            continue
        if not line.startswith("cir file_sources:") or case is None:
            continue
        seen += 1
        if seen == 1:
            continue
        for name, ms in LAP.findall(line):
            out.setdefault(case, {}).setdefault(name, []).append(float(ms))
    return out


def time_cli(index, sources, runs):
    """Seconds of whole `ciruela-index candidates` and `links` processes, with
    and without --host."""
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k, data in enumerate([index] + sources):
            paths.append(os.path.join(tmp, "i%d.ds1" % k))
            with open(paths[-1], "wb") as f:
                f.write(data)
        empty = os.path.join(tmp, "empty")
        os.mkdir(empty)
        cmds = {"candidates": [cli, "candidates"] + paths,
                "links": [cli, "links", paths[0]] + ["%s=%s" % (empty, p) for p in paths[1:]]}
        for name, cmd in cmds.items():
            seen = {}
            for r in range(runs + 1):
                for variant, extra in (("host", ["--host"]), ("device", [])):
                    t0 = time.perf_counter()
                    p = subprocess.run(cmd + extra, capture_output=True)
                    dt = time.perf_counter() - t0
                    assert p.returncode == 0, p.stderr[-2000:]
                    assert seen.setdefault("stdout", p.stdout) == p.stdout
                    if r:      # (the first round warms the page cache)
                        out.setdefault(name, {}).setdefault(variant, []).append(dt)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "file_sources", "bench.json"))
    ap.add_argument("--trace-log", default=None, help="default: trace.log beside --out")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", default="s50,s200,s1000,s5000,c,a,b")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = [c for c in a.cases.split(",") if c]

    import ciruela_amd as ca
    n = ca._n
    ctx = ca.Context(device_mask=1, staging_bytes=n.CIR_STAGING_LAZY)
    result = {"block_size": BS, "runs": a.runs, "seed": a.seed,
              "stats_fields": list(ca.FILE_SOURCES_STATS), "cases": {}}
    for name in names:
        index, sources, hits = make_case(name, a.seed)
        call = Call(n, index, sources)
        nfiles, per, nsrc = CASES[name]
        out = {"files": nfiles, "blocks": nfiles * per, "sources": nsrc,
               "text_bytes": len(index) + sum(len(s) for s in sources),
               "total_seconds": {"host": [], "device": []}}
        if a.traced_child:
            sys.stderr.write("bench case %s\n" % name)
            sys.stderr.flush()
            for _ in range(a.runs + 1):
                call.run(ctx.handle, False)
            continue
        _, host, cnt = call.run(None, True, keep=True)           # warm-ups, and the outputs
        _, dev, _ = call.run(ctx.handle, False, keep=True)
        assert host == dev and cnt == hits, "device and host differ (%s)" % name
        assert call.stats[6] == 1 and call.stats[7] == 0, list(call.stats)
        out["stats"] = list(call.stats)
        for _ in range(a.runs):
            out["total_seconds"]["host"].append(call.run(None, True)[0])
            out["total_seconds"]["device"].append(call.run(ctx.handle, False)[0])
        print("%-6s host %s s   device %s s" % (
            name, ["%.4f" % s for s in out["total_seconds"]["host"]],
            ["%.4f" % s for s in out["total_seconds"]["device"]]), flush=True)
        out["candidates"] = cnt
        if name == "a" and not a.no_cli:
            out["cli_seconds"] = time_cli(index, sources, a.runs)
            print("a cli", json.dumps(out["cli_seconds"]), flush=True)
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
