#!/usr/bin/env python3
"""An image read into device memory, verified, timed (one GPU).

cir_load_blocks is cir_check_blocks that keeps the bytes it read in device
buffers of the caller's.  This times it over the two trees of DESIGN.md 4.5a,
built under a temporary directory --

  small: 20,000 files of 32 KiB          (per-file latency decides)
  large: 2,048 files of 1 MiB            (bandwidth decides)

-- indexed by the CPU restatement (oracle/cpu_indexer.py), one warm-up and
three timed runs of each of, in one process:

  check_blocks        Context.check_blocks on the complete tree: the yardstick
  load_blocks         Context.load_blocks into one torch.uint8 tensor per file
                      (allocated beforehand), every file verified in HBM
  check_blocks_again  the yardstick once more, behind load_blocks
  today               what a user does without it: check_blocks, then every
                      file read and .cuda()'d into a tensor, then a synchronise

and once, for the narrow-store path, a tree of 2,000 files of 30,000 bytes at
block size 1000 loaded into buffers at odd addresses (misaligned) and at
16-byte aligned ones (aligned).  Every run, GiB/s of the bytes the index lists
and the stats arrays go to profiles/load_blocks/bench.json (--out).  What is
compared: load_blocks' median against the min-max band of check_blocks' six
runs ("load_inside_check_band", and "load_over_check_median"), and against
today's median ("today_over_load_median").  Nothing is gated.  Run under
CIR_TRACE=1 for the library's laps on stderr.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cpu_indexer  # noqa: E402
from check_blocks_bench import build_tree, index_files, median, timed  # noqa: E402

GIB = float(1 << 30)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load_blocks", "bench.json"))
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the trees are built (default: /dev/shm, else the system's)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small-files", type=int, default=20000)
    ap.add_argument("--large-files", type=int, default=2048)
    ap.add_argument("--odd-files", type=int, default=2000)
    a = ap.parse_args()

    import torch
    import ciruela_amd as ca
    lib = cpu_indexer.load()
    ctx = ca.Context(device_mask=1)
    result = {"runs": a.runs, "cases": {},
              "tmp": "tmpfs" if (a.tmp or "").startswith("/dev/shm") else "default"}
    base = tempfile.mkdtemp(prefix="load_blocks_bench_", dir=a.tmp)
    try:
        for name, nfiles, size, bs in (("small", a.small_files, 32 << 10, 32768),
                                       ("large", a.large_files, 1 << 20, 32768),
                                       ("bs1000", a.odd_files, 30000, 1000)):
            root = os.path.join(base, name, "img")
            os.makedirs(root)
            build_tree(root, nfiles, size)
            index = cpu_indexer.index(root, bs, 4, lib)
            files = index_files(index)
            assert len(files) == nfiles
            nblk = nfiles * ((size + bs - 1) // bs)
            nbytes = nfiles * size
            rootb = os.fsencode(root)
            out = {"files": nfiles, "file_bytes": size, "bytes": nbytes, "blocks": nblk,
                   "block_size": bs, "methods": {}, "stats": {}}

            def record(mname, fn):
                secs = timed(fn, a.runs)
                out["methods"][mname] = {"seconds": secs,
                                         "GiBps": [nbytes / GIB / s for s in secs]}
                print("%s %-18s %s s" % (name, mname, ["%.3f" % s for s in secs]), flush=True)

            def check_blocks():
                res = ctx.check_blocks(root, index)
                assert res.complete and res.nblk == nblk
                out["stats"]["check_blocks"] = list(res.stats.values())

            def loader(key, buffers):
                def run():
                    res = ctx.load_blocks(root, index, buffers)
                    assert res.complete and res.stats["scattered_bytes"] == nbytes, res
                    out["stats"][key] = list(res.stats.values())
                return run

            def today():
                assert ctx.check_blocks(root, index).complete
                keep = []
                for rel, _ in files:
                    with open(os.path.join(rootb, rel), "rb") as f:
                        keep.append(torch.frombuffer(bytearray(f.read()), dtype=torch.uint8).cuda())
                torch.cuda.synchronize()

            if name == "bs1000":
                # one allocation, the files 16 bytes apart from a 16-byte boundary: at odd
                # addresses every store is narrow, at aligned ones 8 bytes wide or better
                pitch = (size + 16 + 15) & ~15
                arena = torch.empty(nfiles * pitch + 16, dtype=torch.uint8, device="cuda:0")
                for key, skew in (("aligned", 0), ("misaligned", 1)):
                    ptrs = [arena.data_ptr() + i * pitch + skew for i in range(nfiles)]
                    record(key, loader(key, ptrs))
                    got = arena[skew:skew + size].cpu().numpy().tobytes()
                    with open(os.path.join(rootb, files[0][0]), "rb") as f:
                        assert got == f.read()
                record("check_blocks", check_blocks)
                del arena
            else:
                tensors = [torch.empty(size, dtype=torch.uint8, device="cuda:0")
                           for _ in range(nfiles)]
                torch.cuda.synchronize()
                # (plain pointers: the wrapper then neither parses the index for the
                # entries' sizes nor looks at 20,000 tensors inside the timed call)
                ptrs = [t.data_ptr() for t in tensors]
                record("check_blocks", check_blocks)
                record("load_blocks", loader("load_blocks", ptrs))
                record("check_blocks_again", check_blocks)
                record("today", today)
                with open(os.path.join(rootb, files[-1][0]), "rb") as f:
                    assert tensors[-1].cpu().numpy().tobytes() == f.read()
                del tensors
                m = out["methods"]
                band = m["check_blocks"]["seconds"] + m["check_blocks_again"]["seconds"]
                load = median(m["load_blocks"]["seconds"])
                out["check_band"] = [min(band), max(band)]
                out["load_median"] = load
                out["load_inside_check_band"] = min(band) <= load <= max(band)
                out["load_over_check_median"] = load / median(band)
                out["today_over_load_median"] = median(m["today"]["seconds"]) / load
            out["stats_fields"] = list(ca.Context.LOAD_STATS_FIELDS)
            result["cases"][name] = out
            shutil.rmtree(os.path.join(base, name))
    finally:
        shutil.rmtree(base, ignore_errors=True)
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: round(median(v["seconds"]), 4) for m, v in t["methods"].items()}
                      for k, t in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
