#!/usr/bin/env python3
"""The whole download plan in one call against the four calls it composes,
timed (one GPU).

cir_fetch_plan uploads and parses the index texts once and runs the four joins
back to back on the GPU; the sequence it replaces is cir_file_sources,
cir_file_copies, cir_block_extents and cir_block_repeats with a context, one
after the other, each of which frames, uploads and parses the texts again.
This times both over synthetic new versions of an image (random digests, no
files on disk), built like tools/file_copies_bench.py's, in which every stage
has work.  By file ordinal f, the new version holds

  f % 10 in 0..4   unchanged at the same path                (same-path link)
  f % 10 in 5, 6   unchanged below a renamed directory       (content link)
  f % 10 == 7      one block changed                         (extents + 1 block)
  f % 10 == 8      a new file                                (fetched)
  f % 10 == 9      a copy of the new file before it          (repeat extent)

These shares are assumptions about images, not observations.  Source 0 is the
old version; every further source is an older one with another tenth of the
files changed.  Cases:

  a  1.6 M blocks in 20,000 files of 80 against 1 source
  b  the same against 16 sources
  d  50 files of 16 blocks against 1 source

Each case runs, in one process, one warm-up of every side and then --runs
rounds that alternate

  plan      cir_fetch_plan(ctx, ...), arguments prebuilt
  sequence  the four calls with a context as bare C calls, their arguments --
            the skip, want and present bitmaps included -- prebuilt; each of
            the four calls alone is a lap of it

and then --runs rounds of

  glued     the four calls through the Python package with the glue a caller
            needs today (file_copies(skip=...), block_extents(skip_files=...),
            block_repeats(want, present))

with a host clock around whole calls that end in a synchronise, and checks
that the plan and the sequence give the same answer and that the device
answered.  --siblings-only times the four calls alone, for a run against
another build of the library (--root).  The laps of the plan come from a child
process that repeats its runs under CIR_TRACE=1, whose stderr is kept as
profiles/fetch_plan/trace.log.  Everything goes to
profiles/fetch_plan/bench.json (--out) as lists of seconds.
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

BS = 4096
PER_DIR = 100
_HEX = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
SHARES = {"same_path": 0.5, "renamed_directory": 0.2, "one_block_changed": 0.1, "new": 0.1,
          "copy_of_new": 0.1}

# name: (files, blocks per file, sources)
CASES = {"a": (20000, 80, 1), "b": (20000, 80, 16), "d": (50, 16, 1)}


def tokens(rng, nfiles, per):
    """(nfiles, per * 65) u8: the hash tokens of nfiles files of `per` random blocks."""
    d = rng.integers(0, 256, size=(nfiles * per, 32), dtype=np.uint8)
    text = np.empty((nfiles * per, 65), dtype=np.uint8)
    text[:, 0] = 0x20
    text[:, 1::2] = _HEX[d >> 4]
    text[:, 2::2] = _HEX[d & 15]
    return text.reshape(nfiles, per * 65)


def line(f, per, toks):
    return b"  f%07d f %d%s\n" % (f, per * BS, toks.tobytes())


def assemble(lines, moved=()):
    """lines[f] under /dNNNNN, but the files in `moved` under /m/dNNNNN."""
    moved = set(moved)
    out = [b"DIRSIGNATURE.v1 blake2b/256 block_size=%d\n/\n" % BS]
    ndirs = (len(lines) + PER_DIR - 1) // PER_DIR
    for d in range(ndirs):
        out.append(b"/d%05d\n" % d)
        out += [lines[f] for f in range(d * PER_DIR, min(len(lines), (d + 1) * PER_DIR))
                if f not in moved]
    if moved:
        out.append(b"/m\n")
        for d in range(ndirs):
            here = [lines[f] for f in range(d * PER_DIR, min(len(lines), (d + 1) * PER_DIR))
                    if f in moved]
            if here:
                out.append(b"/m/d%05d\n" % d)
                out += here
    out.append(b"00" * 32 + b"\n")
    return b"".join(out)


def make_case(name, seed):
    """(new index, [source index, ...])."""
    nfiles, per, nsrc = CASES[name]
    rng = np.random.default_rng(seed)
    old = tokens(rng, nfiles, per)
    new = old.copy()
    fresh = tokens(rng, nfiles, per)
    for f in range(nfiles):
        k = f % 10
        if k == 7:
            b = (f // 10) % per
            new[f, 65 * b:65 * b + 65] = fresh[f, 65 * b:65 * b + 65]
        elif k == 8:
            new[f] = fresh[f]
        elif k == 9:
            new[f] = new[f - 1]
    index = assemble([line(f, per, new[f]) for f in range(nfiles)],
                     moved=[f for f in range(nfiles) if f % 10 in (5, 6)])
    sources = []
    for j in range(nsrc):
        ls = [line(f, per, old[f]) for f in range(nfiles)]
        if j:                                   # an older version: another tenth changed
            alt = tokens(rng, (nfiles + 9) // 10, per)
            for k, f in enumerate(range(j % 10, nfiles, 10)):
                ls[f] = line(f, per, alt[k])
        sources.append(assemble(ls))
    return index, sources


def words(buf, nwords):
    return np.frombuffer(ctypes.string_at(buf, 8 * nwords), dtype=np.uint64).copy()


class Calls:
    """The five entry points through ctypes, arguments built once."""

    def __init__(self, n, index, sources):
        self.n = n
        self.index = ctypes.create_string_buffer(index, len(index))
        self.ip = ctypes.cast(self.index, ctypes.c_void_p)
        self.len = len(index)
        self.bufs = [ctypes.create_string_buffer(s, len(s)) for s in sources]
        k = len(sources)
        self.sp = (ctypes.c_void_p * k)(*[ctypes.cast(b, ctypes.c_void_p) for b in self.bufs])
        self.sl = (ctypes.c_size_t * k)(*[len(s) for s in sources])
        self.k = k
        self.skip = self.want = self.fetch1 = self.present = None

    def _free(self, outs):
        for p in outs:
            self.n.lib.cir_free(p)

    def plan(self, handle, keep=False):
        n, ref = self.n, ctypes.byref
        outs = [ctypes.c_void_p() for _ in range(10)]
        nl, nc, ne, nr, sk = (ctypes.c_size_t() for _ in range(5))
        nblk = ctypes.c_uint64()
        stats = (ctypes.c_uint64 * 44)()
        t0 = time.perf_counter()
        n.check(n.lib.cir_fetch_plan(handle, self.ip, self.len, self.sp, self.sl, self.k, None,
                                     None, ref(outs[0]), ref(outs[1]), ref(nl), ref(outs[2]),
                                     ref(outs[3]), ref(outs[4]), ref(outs[5]), ref(outs[6]),
                                     ref(nc), ref(outs[7]), ref(ne), ref(outs[8]), ref(nr),
                                     ref(outs[9]), ref(nblk), ref(sk), stats))
        dt = time.perf_counter() - t0
        got = None
        if keep:
            at = ctypes.string_at
            got = dict(
                links=(at(outs[0].value, 8 * nl.value), at(outs[1].value, 4 * nl.value)),
                copies=(at(outs[2].value, 8 * nc.value), at(outs[3].value, 4 * nc.value),
                        at(outs[4].value, 8 * nc.value)),
                extents=at(outs[7].value, 64 * ne.value), repeats=at(outs[8].value, 64 * nr.value),
                fetch=at(outs[9].value, 8 * ((nblk.value + 63) // 64)), nblk=nblk.value,
                stats=list(stats))
        self._free(outs)
        return dt, got

    def sequence(self, handle, keep=False):
        """The four calls, bare; the bitmaps between them are those of the
        first kept run (prebuilt, as a caller with perfect glue would have
        them).  Returns (total, [four laps], answer)."""
        n, ref = self.n, ctypes.byref
        laps, got = [], {}
        # 1. cir_file_sources
        f, s, cnt, sk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        st8 = (ctypes.c_uint64 * 8)()
        t0 = time.perf_counter()
        n.check(n.lib.cir_file_sources(handle, self.ip, self.len, self.sp, self.sl, self.k, ref(f),
                                       ref(s), ref(cnt), ref(sk), st8))
        laps.append(time.perf_counter() - t0)
        if keep:
            got["links"] = (ctypes.string_at(f.value, 8 * cnt.value),
                            ctypes.string_at(s.value, 4 * cnt.value))
            files = np.frombuffer(got["links"][0], dtype=np.uint64)
            nfiles = int(st8[0])
            skip = np.zeros((nfiles + 63) // 64 + 1, dtype=np.uint64)
            np.bitwise_or.at(skip, (files >> np.uint64(6)).astype(np.int64),
                             np.uint64(1) << (files & np.uint64(63)))
            self.skip = (ctypes.c_uint64 * len(skip)).from_buffer_copy(skip.tobytes())
            self.linked = set(int(x) for x in files)
            got["on_device"] = [int(st8[6])]
        self._free((f, s))
        # 2. cir_file_copies
        outs = [ctypes.c_void_p() for _ in range(5)]
        st10 = (ctypes.c_uint64 * 10)()
        t0 = time.perf_counter()
        n.check(n.lib.cir_file_copies(handle, self.ip, self.len, self.sp, self.sl, self.k,
                                      self.skip, *[ref(o) for o in outs], ref(cnt), ref(sk), st10))
        laps.append(time.perf_counter() - t0)
        if keep:
            k = cnt.value
            got["copies"] = tuple(ctypes.string_at(outs[i].value, w * k)
                                  for i, w in ((0, 8), (1, 4), (2, 8)))
            self.linked |= set(int(x) for x in np.frombuffer(got["copies"][0], dtype=np.uint64))
            got["on_device"].append(int(st10[6]))
        self._free(outs)
        # 3. cir_block_extents
        if keep:                                  # the want bitmap: the unlinked files' blocks
            self.want = self.want_of(self.linked)
        e, fo, ne, nblk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
        t0 = time.perf_counter()
        n.check(n.lib.cir_block_extents(handle, self.ip, self.len, self.sp, self.sl, self.k,
                                        self.want, ref(e), ref(ne), ref(fo), ref(nblk), ref(sk),
                                        st10))
        laps.append(time.perf_counter() - t0)
        if keep:
            nw = (nblk.value + 63) // 64
            got["extents"] = ctypes.string_at(e.value, 64 * ne.value)
            f1 = words(fo.value, nw)
            pres = ~f1
            if nblk.value & 63:
                pres[-1] &= np.uint64((1 << (nblk.value & 63)) - 1)
            self.fetch1 = (ctypes.c_uint64 * max(nw, 1)).from_buffer_copy(f1.tobytes())
            self.present = (ctypes.c_uint64 * max(nw, 1)).from_buffer_copy(pres.tobytes())
            got["on_device"].append(int(st10[7]))
        self._free((e, fo))
        # 4. cir_block_repeats
        t0 = time.perf_counter()
        n.check(n.lib.cir_block_repeats(handle, self.ip, self.len, self.fetch1, self.present,
                                        ref(e), ref(ne), ref(fo), ref(nblk), st10))
        laps.append(time.perf_counter() - t0)
        if keep:
            got["repeats"] = ctypes.string_at(e.value, 64 * ne.value)
            got["fetch"] = ctypes.string_at(fo.value, 8 * ((nblk.value + 63) // 64))
            got["nblk"] = nblk.value
            got["on_device"].append(int(st10[7]))
        self._free((e, fo))
        return sum(laps), laps, got

    def want_of(self, linked):
        """Every block of a file that is not linked (the files are laid out by
        this tool: ordinals follow the text)."""
        sizes = [int(m) for m in re.findall(rb"\n  \S+ f (\d+)", self.index.raw)]
        bits = np.concatenate([np.full((sz + BS - 1) // BS, 0 if f in linked else 1, dtype=np.uint8)
                               for f, sz in enumerate(sizes)] or [np.zeros(0, dtype=np.uint8)])
        packed = np.packbits(np.pad(bits, (0, (-len(bits)) % 64)), bitorder="little")
        return (ctypes.c_uint64 * max(len(packed) // 8, 1)).from_buffer_copy(
            packed.tobytes().ljust(8, b"\0"))


def glued(ca, ctx, index, sources):
    """The four calls through the package, with the glue a caller needs today."""
    t0 = time.perf_counter()
    l1, _ = ca.file_sources(index, sources, ctx)
    linked = [f for f, _ in l1]
    l2, _ = ca.file_copies(index, sources, ctx, skip=linked)
    linked += [c[0] for c in l2]
    r1 = ca.block_extents(index, sources, skip_files=set(linked), context=ctx)
    inv = (~np.frombuffer(r1.fetch, dtype=np.uint8)).tobytes()
    r2 = ca.block_repeats(index, want=r1.fetch, present=inv, context=ctx)
    dt = time.perf_counter() - t0
    return dt, (len(l1), len(l2), len(r1.extents), len(r2.extents), r2.stats["left_to_fetch"])


LAP = re.compile(r"(frame and buffers|text upload|count kernels|emit kernels|path join|links glue|"
                 r"content join|want glue|joins and download|block join|extent map|repeat join|"
                 r"repeat map|tables to counts|extent tail|repeat tail|compact and decode) "
                 r"(\d+\.\d+) ms")


def parse_trace(text):
    """{case: {lap: [ms, ...]}} of the traced child's lines (warm-ups dropped)."""
    out, case, seen = {}, None, 0
    for ln in text.splitlines():
        if ln.startswith("bench case "):
            case, seen = ln.split()[2], 0
            continue
        if not ln.startswith("cir fetch_plan:") or case is None:
            continue
        seen += 1
        if seen == 1:
            continue
        for name, ms in LAP.findall(ln):
            out.setdefault(case, {}).setdefault(name, []).append(float(ms))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_plan", "bench.json"))
    ap.add_argument("--trace-log", default=None, help="default: trace.log beside --out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cases", default="d,a,b")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--root", default=ROOT, help="the tree whose ciruela_amd is loaded")
    ap.add_argument("--siblings-only", action="store_true",
                    help="time the four calls alone (for another build of the library)")
    ap.add_argument("--no-glued", action="store_true", help="leave the Python-glue side out")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = [c for c in a.cases.split(",") if c]
    sys.path.insert(0, os.path.abspath(a.root))

    import ciruela_amd as ca
    n = ca._n
    ctx = ca.Context(device_mask=1, staging_bytes=n.CIR_STAGING_LAZY)
    result = {"block_size": BS, "runs": a.runs, "seed": a.seed, "shares": SHARES,
              "library": os.path.relpath(os.path.abspath(a.root), ROOT), "cases": {}}
    sides = ("sequence",) if a.siblings_only else ("plan", "sequence") + (
        () if a.no_glued else ("glued",))
    for name in names:
        index, sources = make_case(name, a.seed)
        calls = Calls(n, index, sources)
        nfiles, per, nsrc = CASES[name]
        out = {"files": nfiles, "blocks": nfiles * per, "sources": nsrc,
               "text_bytes": len(index) + sum(len(s) for s in sources),
               "total_seconds": {s: [] for s in sides},
               "sibling_seconds": {k: [] for k in ("file_sources", "file_copies", "block_extents",
                                                   "block_repeats")}}
        if a.traced_child:
            sys.stderr.write("bench case %s\n" % name)
            sys.stderr.flush()
            for _ in range(a.runs + 1):
                calls.plan(ctx.handle)
            continue
        _, _, seq = calls.sequence(ctx.handle, keep=True)           # warm-ups, and the answers
        assert seq["on_device"] == [1, 1, 1, 1], seq["on_device"]
        out["answer"] = {"links": len(seq["links"][0]) // 8, "copies": len(seq["copies"][0]) // 8,
                         "extents": len(seq["extents"]) // 64, "repeats": len(seq["repeats"]) // 64,
                         "fetch_blocks": int(np.unpackbits(
                             np.frombuffer(seq["fetch"], dtype=np.uint8)).sum())}
        if not a.siblings_only:
            _, plan = calls.plan(ctx.handle, keep=True)
            assert plan["stats"][42] == 1 and plan["stats"][43] == 0, plan["stats"][38:]
            for k in ("links", "copies", "extents", "repeats", "fetch", "nblk"):
                assert plan[k] == seq[k], "plan and sequence differ in %s (%s)" % (k, name)
            out["plan_stats"] = plan["stats"]
        for _ in range(a.runs):
            if "plan" in sides:
                out["total_seconds"]["plan"].append(calls.plan(ctx.handle)[0])
            total, laps, _ = calls.sequence(ctx.handle)
            out["total_seconds"]["sequence"].append(total)
            for k, dt in zip(out["sibling_seconds"], laps):
                out["sibling_seconds"][k].append(dt)
        # (in rounds of its own, warm-up included: the package's wrappers copy
        # every text, up to 2 GB allocated and freed per call, and whichever
        # call came next paid for that -- the plan measured 18-32 ms behind it
        # against 9.3-9.7 ms alone or between two sequences)
        if "glued" in sides:
            _, counts = glued(ca, ctx, index, sources)
            a_ = out["answer"]
            assert counts == (a_["links"], a_["copies"], a_["extents"], a_["repeats"],
                              a_["fetch_blocks"]), counts
            for _ in range(a.runs):
                out["total_seconds"]["glued"].append(glued(ca, ctx, index, sources)[0])
        print("%-3s " % name + "   ".join(
            "%s %s s" % (k, ["%.4f" % s for s in v]) for k, v in out["total_seconds"].items()),
            flush=True)
        result["cases"][name] = out
        del calls, index, sources
    ctx.close()
    if a.traced_child:
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not a.siblings_only:
        env = dict(os.environ, CIR_TRACE="1")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child",
                                "--runs", str(min(a.runs, 3)), "--cases", ",".join(names),
                                "--seed", str(a.seed)],
                               env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if child.returncode != 0:
            sys.stderr.write(child.stderr[-4000:])
            return 1
        log = a.trace_log or os.path.join(os.path.dirname(os.path.abspath(a.out)), "trace.log")
        with open(log, "w") as f:      # (the library's lines and the case marks, nothing else)
            f.writelines(ln for ln in child.stderr.splitlines(True)
                         if ln.startswith(("bench case ", "cir")))
        for name, laps in parse_trace(child.stderr).items():
            result["cases"][name]["plan_laps_ms"] = laps
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {v: [round(min(t), 4), round(max(t), 4)]
                          for v, t in list(c["total_seconds"].items()) +
                          list(c["sibling_seconds"].items())}
                      for k, c in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
