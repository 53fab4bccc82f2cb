#!/usr/bin/env python3
"""Where a new image's blocks sit in older images' indexes, timed (one GPU).

fill_blocks queues every block of every file that was not hardlinked whole
(src/daemon/tracking/progress.rs:129-170); cir_block_sources joins the new
index's digests with the older indexes' instead.  This times the call over
synthetic indexes (random digests, files of 64 blocks, no files on disk):

  a  one source of 1.6 M blocks against a new index of 1.6 M, 90 % shared
  b  16 sources of 1 M blocks (a 16 M pool) against 1 M needed, 50 % shared
  c  one source of 2,000 blocks against 2,000, 90 % shared
  sN one source of N blocks against N, 90 % shared (a size sweep, e.g. s8000)

each through ctypes with the arguments built beforehand, with a context (the
join on the device) and with ctx = NULL (the join on the host), one warm-up
and three timed runs, and checks that both give the same arrays.  The totals
come from this process; the laps -- parse, pool, upload, build kernel, probe
kernel, download, map on the device; parse, pool, join, map on the host --
from a child process that repeats the runs under CIR_TRACE=1, whose stderr is
kept as profiles/block_sources/trace.log.  The comparison that matters is
join phase against join phase: upload + build + probe + download against the
host's map build + lookups, on the same parsed input.  Everything goes to
profiles/block_sources/bench.json (--out) as ranges.

--extents: the same cases (and v: a new version of a 1.6 M-block image, whole
files shared but one block in a thousand changed) for cir_block_extents and
for cir_block_sources' map on either side, in one process, one warm-up and
three timed runs each:

  sources_default      cir_block_sources with a context, CIR_SOURCES_MAP unset
  sources_device_map   the same with CIR_SOURCES_MAP=device
  sources_host_map     the same with CIR_SOURCES_MAP=host
  sources_parent       the same call of another build of the library
                       (--parent-lib: the parent commit's), when given
  extents_device       cir_block_extents with a context
  extents_join_then_host  cir_block_extents with a context and
                       CIR_SOURCES_MAP=host: the device join, then
                       map_matches and extents_of on a host thread
  extents_host         cir_block_extents with ctx = NULL

with the extent counts and the bytes that come back beside 20 bytes per block.
All variants must give identical output.  The laps of the device map (tables
upload, map kernel, scan kernel, emit kernels, downloads) come from the traced
child; its stderr is kept as profiles/block_extents/trace.log, the ranges as
profiles/block_extents/bench.json.
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BS = 32768
PER_FILE = 64
CASES = {"a": (1, 1600000, 1600000, 0.9), "b": (16, 1000000, 1000000, 0.5),
         "c": (1, 2000, 2000, 0.9), "v": (1, 1600000, 1600000, 0.999)}
_HEX = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)


def make_index(digests, tag):
    """A DIRSIGNATURE.v1 index over the digests (n x 32 uint8), PER_FILE
    blocks per file; the footer is not a hash of anything (nothing reads it)."""
    n = len(digests)
    text = np.empty((n, 65), dtype=np.uint8)
    text[:, 0] = 0x20
    text[:, 1::2] = _HEX[digests >> 4]
    text[:, 2::2] = _HEX[digests & 15]
    out = [b"DIRSIGNATURE.v1 blake2b/256 block_size=%d\n/\n" % BS]
    for f, at in enumerate(range(0, n, PER_FILE)):
        k = min(PER_FILE, n - at)
        out.append(b"  %s%07d f %d" % (tag, f, k * BS))
        out.append(text[at:at + k].tobytes())
        out.append(b"\n")
    out.append(b"00" * 32 + b"\n")
    return b"".join(out)


def make_case(name, seed):
    nsrc, per_src, n_need, shared = CASES[name]
    rng = np.random.default_rng(seed)
    pools = [rng.integers(0, 256, size=(per_src, 32), dtype=np.uint8) for _ in range(nsrc)]
    if name == "v":  # a new version: the old image with one block in a thousand changed
        need = pools[0].copy()
        changed = rng.random(n_need) >= shared
        need[changed] = rng.integers(0, 256, size=(int(changed.sum()), 32), dtype=np.uint8)
        return make_index(need, b"n"), [make_index(pools[0], b"s0_")], int((~changed).sum())
    need = rng.integers(0, 256, size=(n_need, 32), dtype=np.uint8)
    hit = rng.random(n_need) < shared
    which = rng.integers(0, nsrc, size=n_need)
    where = rng.integers(0, per_src, size=n_need)
    for s in range(nsrc):
        m = hit & (which == s)
        need[m] = pools[s][where[m]]
    return make_index(need, b"n"), [make_index(p, b"s%d_" % s) for s, p in enumerate(pools)], \
        int(hit.sum())


class Call:
    """cir_block_sources through ctypes, arguments built once."""

    def __init__(self, n, index, sources):
        self.n = n
        self.index = ctypes.create_string_buffer(index, len(index))
        self.len = len(index)
        self.bufs = [ctypes.create_string_buffer(s, len(s)) for s in sources]
        self.sp = (ctypes.c_void_p * len(sources))(*[ctypes.cast(b, ctypes.c_void_p)
                                                     for b in self.bufs])
        self.sl = (ctypes.c_size_t * len(sources))(*[len(s) for s in sources])
        self.stats = (ctypes.c_uint64 * n.CIR_SOURCES_STATS_FIELDS)()

    def run(self, handle, keep=False):
        n = self.n
        so, fo, bo = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nblk, skipped = ctypes.c_uint64(), ctypes.c_size_t()
        t0 = time.perf_counter()
        n.check(n.lib.cir_block_sources(handle, ctypes.cast(self.index, ctypes.c_void_p), self.len,
                                        self.sp, self.sl, len(self.bufs), None, ctypes.byref(so),
                                        ctypes.byref(fo), ctypes.byref(bo), ctypes.byref(nblk),
                                        ctypes.byref(skipped), self.stats))
        dt = time.perf_counter() - t0
        got = None
        if keep:
            k = nblk.value
            got = (ctypes.string_at(so.value, 4 * k), ctypes.string_at(fo.value, 8 * k),
                   ctypes.string_at(bo.value, 8 * k))
        for p in (so, fo, bo):
            n.lib.cir_free(p)
        return dt, got


class ExtentsCall(Call):
    """cir_block_extents through ctypes, arguments built once."""

    def __init__(self, n, index, sources, lib=None):
        Call.__init__(self, n, index, sources)
        self.lib = lib or n.lib
        self.stats = (ctypes.c_uint64 * 10)()

    def run(self, handle, keep=False):
        n = self.n
        eo, fo = ctypes.c_void_p(), ctypes.c_void_p()
        next_, nblk, skipped = ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_size_t()
        t0 = time.perf_counter()
        n.check(self.lib.cir_block_extents(handle, ctypes.cast(self.index, ctypes.c_void_p),
                                           self.len, self.sp, self.sl, len(self.bufs), None,
                                           ctypes.byref(eo), ctypes.byref(next_), ctypes.byref(fo),
                                           ctypes.byref(nblk), ctypes.byref(skipped), self.stats))
        dt = time.perf_counter() - t0
        got = None
        if keep:
            got = (ctypes.string_at(eo.value, 64 * next_.value) if next_.value else b"",
                   ctypes.string_at(fo.value, 8 * ((nblk.value + 63) // 64)))
        for p in (eo, fo):
            n.lib.cir_free(p)
        return dt, got


class ParentLib:
    """Another build of the library (the parent commit's), loaded beside this
    one: cir_block_sources with a context of its own."""

    def __init__(self, n, path):
        self.lib = ctypes.CDLL(path)
        for name in ("cir_init_n", "cir_destroy", "cir_block_sources", "cir_free"):
            f = getattr(self.lib, name)
            f.restype, f.argtypes = n._SIGS[name]
        self.handle = ctypes.c_void_p()
        n.check(self.lib.cir_init_n(ctypes.byref(self.handle), 1, n.CIR_STAGING_LAZY, 0, 0))

    def close(self):
        self.lib.cir_destroy(self.handle)


class ParentCall(Call):
    def __init__(self, n, index, sources, parent):
        Call.__init__(self, n, index, sources)
        self.parent = parent

    def run(self, handle, keep=False):
        n, lib = self.n, self.parent.lib
        so, fo, bo = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        nblk, skipped = ctypes.c_uint64(), ctypes.c_size_t()
        t0 = time.perf_counter()
        rc = lib.cir_block_sources(self.parent.handle, ctypes.cast(self.index, ctypes.c_void_p),
                                   self.len, self.sp, self.sl, len(self.bufs), None,
                                   ctypes.byref(so), ctypes.byref(fo), ctypes.byref(bo),
                                   ctypes.byref(nblk), ctypes.byref(skipped), self.stats)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        got = None
        if keep:
            k = nblk.value
            got = (ctypes.string_at(so.value, 4 * k), ctypes.string_at(fo.value, 8 * k),
                   ctypes.string_at(bo.value, 8 * k))
        for p in (so, fo, bo):
            lib.cir_free(p)
        return dt, got


XLAP = re.compile(r"(tables upload|map kernel|scan kernel|emit kernels|downloads) (\d+\.\d+) ms")


def parse_extents_trace(text):
    """{case: {variant: {lap: [ms, ...]}}} of the traced child's device-map
    lines (each variant's first line is its warm-up)."""
    out, case, variant, seen = {}, None, None, 0
    for line in text.splitlines():
        if line.startswith("bench case "):
            case, variant, seen = line.split()[2], line.split()[3], 0
            continue
        if not line.startswith("cir extents map") or case is None:
            continue
        seen += 1
        if seen == 1:
            continue
        laps = out.setdefault(case, {}).setdefault(variant, {})
        for name, ms in XLAP.findall(line):
            laps.setdefault(name, []).append(float(ms))
    return out


def set_map(mode):
    if mode is None:
        os.environ.pop("CIR_SOURCES_MAP", None)
    else:
        os.environ["CIR_SOURCES_MAP"] = mode


def main_extents(a, names):
    import ciruela_amd as ca
    n = ca._n
    ctx = ca.Context(device_mask=1, staging_bytes=n.CIR_STAGING_LAZY)
    parent = ParentLib(n, a.parent_lib) if a.parent_lib and not a.traced_child else None
    result = {"block_size": BS, "blocks_per_file": PER_FILE, "runs": a.runs, "seed": a.seed,
              "parent_lib": bool(parent), "cases": {}}
    for name in names:
        index, sources, hits = make_case(name, a.seed)
        sc, ec = Call(n, index, sources), ExtentsCall(n, index, sources)
        variants = [("sources_default", sc, ctx.handle, None),
                    ("sources_device_map", sc, ctx.handle, "device"),
                    ("sources_host_map", sc, ctx.handle, "host")]
        if parent:
            variants.append(("sources_parent", ParentCall(n, index, sources, parent), None, None))
        variants += [("extents_device", ec, ctx.handle, None),
                     ("extents_join_then_host", ec, ctx.handle, "host")]
        if not a.traced_child:
            variants.append(("extents_host", ec, None, None))
        out = {"sources": len(sources), "pool_blocks": CASES[name][0] * CASES[name][1],
               "need_blocks": CASES[name][2], "need_blocks_drawn_from_the_pool": hits,
               "total_seconds": {}}
        kept = {}
        for variant, call, handle, mode in variants:
            if a.traced_child:
                sys.stderr.write("bench case %s %s\n" % (name, variant))
                sys.stderr.flush()
            set_map(mode)
            _, kept[variant] = call.run(handle, keep=True)    # warm-up, and the output
            if call is ec:
                out.setdefault("extents_stats", {})[variant] = list(call.stats)
            out["total_seconds"][variant] = [call.run(handle)[0] for _ in range(a.runs)]
            set_map(None)
            if not a.traced_child:
                print("%s %-22s %s s" % (name, variant,
                                         ["%.4f" % s for s in out["total_seconds"][variant]]),
                      flush=True)
        same = [v for v in kept if v.startswith("sources")]
        assert all(kept[v] == kept[same[0]] for v in same), "the per-block arrays differ (%s)" % name
        same = [v for v in kept if v.startswith("extents")]
        assert all(kept[v] == kept[same[0]] for v in same), "the extents differ (%s)" % name
        st = out["extents_stats"]["extents_device"]
        nblk = CASES[name][2]
        out["extents"] = st[8]
        out["blocks_found"] = st[1]
        out["blocks_left_to_fetch"] = st[9]
        out["bytes_back_extents"] = 64 * st[8] + 8 * ((nblk + 63) // 64)
        out["bytes_back_per_block_arrays"] = 20 * nblk
        result["cases"][name] = out
        del sc, ec, variants, kept, index, sources
    if parent:
        parent.close()
    ctx.close()
    if a.traced_child:
        return 0
    env = dict(os.environ, CIR_TRACE="1")
    env.pop("CIR_SOURCES_MAP", None)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--extents",
                            "--traced-child", "--runs", str(a.runs), "--cases", ",".join(names),
                            "--seed", str(a.seed)],
                           env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if child.returncode != 0:
        sys.stderr.write(child.stderr[-4000:])
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = a.trace_log or os.path.join(os.path.dirname(os.path.abspath(a.out)), "trace.log")
    with open(log, "w") as f:
        f.write(child.stderr)
    for name, laps in parse_extents_trace(child.stderr).items():
        result["cases"][name]["device_map_laps_ms"] = laps
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: dict({v: [round(min(t), 4), round(max(t), 4)]
                               for v, t in c["total_seconds"].items()},
                              extents=c["extents"], bytes_back=c["bytes_back_extents"],
                              per_block_bytes=c["bytes_back_per_block_arrays"])
                      for k, c in result["cases"].items()}))
    return 0


LAP = re.compile(r"([a-z ]+?) (\d+\.\d+) ms")


def parse_trace(text):
    """{case: {path: {lap: [ms, ...]}}} of a child's stderr (warm-ups dropped)."""
    out, case, seen = {}, None, {}
    for line in text.splitlines():
        if line.startswith("bench case "):
            case = line.split()[2]
            seen = {}
            continue
        if not line.startswith("cir block_sources:") or case is None:
            continue
        path = "device" if ", device;" in line else "host"
        seen[path] = seen.get(path, 0) + 1
        if seen[path] == 1:
            continue  # the warm-up
        laps = out.setdefault(case, {}).setdefault(path, {})
        for name, ms in LAP.findall(line.split(";", 1)[1]):
            laps.setdefault(name.strip(" ,"), []).append(float(ms))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None,
                    help="default: profiles/block_sources/bench.json, or "
                         "profiles/block_extents/bench.json with --extents")
    ap.add_argument("--extents", action="store_true",
                    help="time cir_block_extents and cir_block_sources' map on either side")
    ap.add_argument("--parent-lib", default=None,
                    help="--extents: another build of libciruela_amd.so to time beside this one")
    ap.add_argument("--trace-log", default=None, help="default: trace.log beside --out")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", default="c,a,b")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = [c for c in a.cases.split(",") if c]
    for c in names:  # sN: one source of N blocks against N, 90 % shared (a size sweep)
        if re.fullmatch(r"s\d+", c):
            CASES[c] = (1, int(c[1:]), int(c[1:]), 0.9)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "block_extents" if a.extents else "block_sources",
                             "bench.json")
    if a.extents:
        return main_extents(a, names)

    import ciruela_amd as ca
    n = ca._n
    ctx = ca.Context(device_mask=1, staging_bytes=n.CIR_STAGING_LAZY)
    result = {"block_size": BS, "blocks_per_file": PER_FILE, "runs": a.runs, "seed": a.seed,
              "stats_fields": list(ca.SourcesResult.STATS_FIELDS), "cases": {}}
    for name in names:
        index, sources, hits = make_case(name, a.seed)
        call = Call(n, index, sources)
        if a.traced_child:
            sys.stderr.write("bench case %s\n" % name)
            sys.stderr.flush()
        out = {"sources": len(sources), "pool_blocks": CASES[name][0] * CASES[name][1],
               "need_blocks": CASES[name][2], "need_blocks_drawn_from_the_pool": hits,
               "index_bytes": len(index), "source_index_bytes": sum(len(s) for s in sources),
               "total_seconds": {}}
        kept = {}
        for path, handle in (("device", ctx.handle), ("host", None)):
            _, kept[path] = call.run(handle, keep=True)   # warm-up, and the arrays
            out.setdefault("stats", {})[path] = list(call.stats)
            out["total_seconds"][path] = [call.run(handle)[0] for _ in range(a.runs)]
            if not a.traced_child:
                print("%s %-6s %s s" % (name, path,
                                        ["%.4f" % s for s in out["total_seconds"][path]]),
                      flush=True)
        assert kept["device"] == kept["host"], "device and host arrays differ (case %s)" % name
        assert out["stats"]["device"][1] == out["stats"]["host"][1] >= hits
        result["cases"][name] = out
        del call, index, sources, kept
    ctx.close()
    if a.traced_child:
        return 0
    # the laps: the same runs in a child under CIR_TRACE=1
    env = dict(os.environ, CIR_TRACE="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child", "--runs",
                            str(a.runs), "--cases", ",".join(names), "--seed", str(a.seed)],
                           env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if child.returncode != 0:
        sys.stderr.write(child.stderr[-4000:])
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = a.trace_log or os.path.join(os.path.dirname(os.path.abspath(a.out)), "trace.log")
    with open(log, "w") as f:
        f.write(child.stderr)
    for name, laps in parse_trace(child.stderr).items():
        c = result["cases"][name]
        c["laps_ms"] = laps
        d, h = laps.get("device", {}), laps.get("host", {})
        if d and h:
            dev_join = [sum(v) for v in zip(d["upload"], d["build kernel"], d["probe kernel"],
                                            d["download"])]
            c["join_phase_ms"] = {"device_upload_build_probe_download": dev_join,
                                  "host_map_build_and_lookups": h["join"]}
            c["host_join_over_device_join"] = [min(h["join"]) / max(dev_join),
                                               max(h["join"]) / min(dev_join)]
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"total_s": {p: [round(min(v), 4), round(max(v), 4)]
                                      for p, v in c["total_seconds"].items()},
                          "join_ms": {p: [round(min(v), 3), round(max(v), 3)]
                                      for p, v in c.get("join_phase_ms", {}).items()}}
                      for k, c in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
