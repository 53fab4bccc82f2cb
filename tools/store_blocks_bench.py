#!/usr/bin/env python3
"""An image written out of device memory, indexed, timed (one GPU).

cir_store_blocks is cir_load_blocks mirrored: files that live in HBM are
gathered into the staging slots on the device, hashed there, downloaded one
slot per batch and written out, and the tree's index comes back.  This times
it over the two trees of DESIGN.md 4.5a, all data in HBM --

  small: 20,000 files of 32 KiB          (per-file cost decides)
  large: 2,048 files of 1 MiB            (bandwidth decides)

-- with one warm-up and three timed runs of each of, in one process, every run
into a fresh root under a temporary directory:

  store_blocks   Context.store_blocks (what store_image calls) of the list
  today          the flow it replaces: index_memory of the list, then per file
                 .cpu() and a file write (directories made beforehand)
  load_blocks    Context.load_blocks of the stored tree into tensors allocated
                 beforehand: the opposite direction's figure

and, for the narrow-load path, 2,000 files of 30,000 bytes at block size 1000
stored from odd source addresses (misaligned) and from 16-byte aligned ones
(aligned).  Every run, GiB/s of the files' bytes and the stats go to
profiles/store_blocks/bench.json (--out), with "today_over_store_median" and,
for the third shape, "misaligned_over_aligned_median" beside the spread of the
runs.  Nothing is gated.  The library's CIR_TRACE laps come from a child
process (--laps: one warm-up and one traced store per tree) and are recorded
under "laps".
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

GIB = float(1 << 30)
SHAPES = (("small", "small_files", 32 << 10, 32768), ("large", "large_files", 1 << 20, 32768),
          ("bs1000", "odd_files", 30000, 1000))


def median(v):
    return sorted(v)[len(v) // 2]


def paths_of(nfiles, per_dir=1000):
    return [b"/d%03d/f%05d" % (i // per_dir, i) for i in range(nfiles)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_blocks", "bench.json"))
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the trees are written (default: /dev/shm, else the system's)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small-files", type=int, default=20000)
    ap.add_argument("--large-files", type=int, default=2048)
    ap.add_argument("--odd-files", type=int, default=2000)
    ap.add_argument("--laps", action="store_true",
                    help="one warm-up and one store per tree, nothing recorded (run under CIR_TRACE=1)")
    a = ap.parse_args()

    import torch
    import ciruela_amd as ca
    ctx = ca.Context(device_mask=1)
    ht = ca.HashType.blake2b_256()
    result = {"runs": a.runs, "cases": {},
              "tmp": "tmpfs" if (a.tmp or "").startswith("/dev/shm") else "default"}
    base = tempfile.mkdtemp(prefix="store_blocks_bench_", dir=a.tmp)
    fresh = [0]

    def new_root():
        fresh[0] += 1
        root = os.path.join(base, "img%d" % fresh[0])
        os.mkdir(root)
        return root

    try:
        for name, arg, size, bs in SHAPES:
            nfiles = getattr(a, arg)
            nbytes = nfiles * size
            paths = paths_of(nfiles)
            # one allocation, the files 16 bytes apart from a 16-byte boundary
            pitch = (size + 16 + 15) & ~15
            arena = torch.randint(0, 256, (nfiles * pitch + 16,), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()

            def listed(skew):
                return [(p, (arena.data_ptr() + i * pitch + skew, size)) for i, p in enumerate(paths)]

            out = {"files": nfiles, "file_bytes": size, "bytes": nbytes, "block_size": bs,
                   "methods": {}, "stats": {}}
            last = {}

            def run(mname, fn, keep=False):
                """One warm-up and a.runs timed runs, each into a fresh root that is
                removed outside the timing (the last one stays with keep)."""
                secs = []
                for k in range((1 if a.laps else a.runs) + 1):
                    root = new_root()
                    t0 = time.perf_counter()
                    fn(root)
                    dt = time.perf_counter() - t0
                    if k:
                        secs.append(dt)
                    if keep and k == a.runs:
                        last["root"] = root
                    else:
                        shutil.rmtree(root)
                out["methods"][mname] = {"seconds": secs, "GiBps": [nbytes / GIB / s for s in secs]}
                print("%s %-12s %s s" % (name, mname, ["%.3f" % s for s in secs]), flush=True)

            def storer(key, files):
                def fn(root):
                    stats = {}
                    last["index"] = ctx.store_blocks(root, files, bs, ht, stats=stats)
                    assert stats["bytes"] == nbytes and stats["files"] == nfiles, stats
                    out["stats"][key] = list(stats.values())
                return fn

            def today(root):
                files = listed(0)
                index = ca.index_memory(files, bs, ht, context=ctx)
                assert len(index) > 65
                for d in sorted({os.path.dirname(p) for p in paths}):
                    os.mkdir(os.path.join(os.fsencode(root), d.lstrip(b"/")))
                rootb = os.fsencode(root)
                for i, p in enumerate(paths):
                    t = arena[i * pitch:i * pitch + size].cpu()
                    with open(os.path.join(rootb, p.lstrip(b"/")), "wb") as f:
                        f.write(t.numpy().data)

            if name == "bs1000":
                for key, skew in (("aligned", 0), ("misaligned", 1)):
                    run(key, storer(key, listed(skew)), keep=not a.laps)
                    if not a.laps:
                        first = os.path.join(os.fsencode(last["root"]), paths[0].lstrip(b"/"))
                        with open(first, "rb") as f:
                            assert f.read() == arena[skew:skew + size].cpu().numpy().tobytes()
                        shutil.rmtree(last["root"])
                if not a.laps:
                    m = out["methods"]
                    out["misaligned_over_aligned_median"] = \
                        median(m["misaligned"]["seconds"]) / median(m["aligned"]["seconds"])
                    out["spread"] = {k: max(m[k]["seconds"]) - min(m[k]["seconds"])
                                     for k in ("aligned", "misaligned")}
                    out["median_difference"] = \
                        median(m["misaligned"]["seconds"]) - median(m["aligned"]["seconds"])
            elif a.laps:
                run("store_blocks", storer("store_blocks", listed(0)))
            else:
                run("store_blocks", storer("store_blocks", listed(0)), keep=True)
                root, index = last["root"], last["index"]
                assert ca.check_index(root, index, context=ctx).ok
                dests = torch.empty(nfiles * pitch, dtype=torch.uint8, device="cuda:0")
                # the index's file order is the paths' here: d000/f00000, d000/f00001, ..
                ptrs = [dests.data_ptr() + i * pitch for i in range(nfiles)]

                def load(_root):
                    res = ctx.load_blocks(root, index, ptrs)
                    assert res.complete and res.stats["scattered_bytes"] == nbytes
                run("load_blocks", load)
                view = lambda t: t[:nfiles * pitch].view(nfiles, pitch)[:, :size]  # noqa: E731
                assert torch.equal(view(dests), view(arena))
                del dests
                shutil.rmtree(root)
                run("today", today)
                m = out["methods"]
                out["today_over_store_median"] = \
                    median(m["today"]["seconds"]) / median(m["store_blocks"]["seconds"])
                out["load_over_store_median"] = \
                    median(m["load_blocks"]["seconds"]) / median(m["store_blocks"]["seconds"])
            out["stats_fields"] = list(ca.Context.STORE_STATS_FIELDS)
            result["cases"][name] = out
            del arena
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(base, ignore_errors=True)
        ctx.close()
    if a.laps:
        return 0
    # the library's own laps, from a process of its own with the trace on
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--laps",
                            "--small-files", str(a.small_files), "--large-files",
                            str(a.large_files), "--odd-files", str(a.odd_files)] +
                           (["--tmp", a.tmp] if a.tmp else []),
                           env=dict(os.environ, CIR_TRACE="1"), capture_output=True, timeout=900)
    assert child.returncode == 0, child.stderr[-3000:]
    lines = [ln for ln in child.stderr.decode(errors="replace").split("\n")
             if ln.startswith("cir store_blocks:")]
    # per tree a warm-up and one run; the third shape twice
    names = ["small", "large", "bs1000 aligned", "bs1000 misaligned"]
    result["laps"] = {n: lines[2 * i + 1] for i, n in enumerate(names) if 2 * i + 1 < len(lines)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: round(median(v["seconds"]), 4) for m, v in t["methods"].items()}
                      for k, t in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
