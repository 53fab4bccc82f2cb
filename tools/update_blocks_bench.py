#!/usr/bin/env python3
"""The next version of an image loaded in the buffers that hold it, timed (one GPU).

cir_update_blocks is cir_reload_blocks with the destinations in the resident
buffers themselves.  This times it over tools/reload_blocks_bench.py's two
trees and three versions N + 1, built under a temporary
directory --

  small: 20,000 files of 32 KiB          large: 2,048 files of 1 MiB
  one_in_1000   one byte flipped in every 1,000th block
  one_in_10     every tenth file replaced by new random bytes
  every_block   one byte flipped in every block

-- one warm-up and three timed runs of each of, in one process:

  update_blocks   Context.update_blocks into version N's own tensors
  reload_blocks   Context.reload_blocks into a second set of tensors
  load_blocks     Context.load_blocks into version N's tensors: the baseline

update_blocks and load_blocks overwrite version N, so the tensors are one
allocation that is restored from a copy of version N before every run, outside
the timed span.  Peak device memory is torch.cuda.max_memory_allocated over a
method's runs less that copy, which only the benchmark needs, plus for
update_blocks the staging scratch the library allocated (stats
"scratch_bytes"); the second set of tensors exists only while reload_blocks
runs.  The library's other per-call scratch is the same for both and is not
counted.

Every run, the stats, the peaks and "update_over_reload_median" go to
profiles/update_blocks/bench.json (--out); nothing is gated.  The library's
laps come from a child process of this script under CIR_TRACE=1 (one run of
each version), whose `cir update_blocks:` and `cir reload_blocks:` lines are
kept per version.
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

import cpu_indexer  # noqa: E402
from check_blocks_bench import build_tree, index_files, median  # noqa: E402
from reload_blocks_bench import VARIANTS, mutate  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_blocks", "bench.json"))
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the trees are built (default: /dev/shm, else the system's)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small-files", type=int, default=20000)
    ap.add_argument("--large-files", type=int, default=2048)
    ap.add_argument("--traced", action="store_true",
                    help="(the child) one run of each version, the laps on stderr, no file")
    a = ap.parse_args()

    import torch
    import ciruela_amd as ca
    lib = cpu_indexer.load()
    ctx = ca.Context(device_mask=1)
    runs = 1 if a.traced else a.runs
    result = {"runs": runs, "cases": {},
              "tmp": "tmpfs" if (a.tmp or "").startswith("/dev/shm") else "default"}
    base = tempfile.mkdtemp(prefix="update_blocks_bench_", dir=a.tmp)
    try:
        for name, nfiles, size, bs in (("small", a.small_files, 32 << 10, 32768),
                                       ("large", a.large_files, 1 << 20, 32768)):
            root = os.path.join(base, name, "img")
            os.makedirs(root)
            build_tree(root, nfiles, size)
            rootb = os.fsencode(root)
            index_n = cpu_indexer.index(root, bs, 4, lib)
            files = index_files(index_n)
            assert len(files) == nfiles
            nblk = nfiles * ((size + bs - 1) // bs)
            held = torch.empty(nfiles * size, dtype=torch.uint8, device="cuda:0")
            base_ptr = held.data_ptr()
            # (plain pointers: the wrapper then looks at no tensor inside the timed call)
            ptrs = [base_ptr + i * size for i in range(nfiles)]
            resident = [(p, size) for p in ptrs]
            assert ctx.load_blocks(root, index_n, ptrs).complete
            version_n = held.clone()
            torch.cuda.synchronize()
            out = {"files": nfiles, "file_bytes": size, "bytes": nfiles * size, "blocks": nblk,
                   "block_size": bs, "variants": {}}
            for variant in VARIANTS:
                changed = mutate(variant, rootb, files, size, bs)
                index = cpu_indexer.index(root, bs, 4, lib)
                v = {"changed_blocks": changed, "methods": {}, "stats": {}}
                fresh = None

                def update_blocks():
                    return ctx.update_blocks(root, index, ptrs, resident)

                def reload_blocks():
                    return ctx.reload_blocks(root, index, fresh_ptrs, resident)

                def load_blocks():
                    return ctx.load_blocks(root, index, ptrs)

                for mname, fn in (("update_blocks", update_blocks),
                                  ("reload_blocks", reload_blocks), ("load_blocks", load_blocks)):
                    if mname == "reload_blocks":
                        fresh = torch.empty(nfiles * size, dtype=torch.uint8, device="cuda:0")
                        fresh_ptrs = [fresh.data_ptr() + i * size for i in range(nfiles)]
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    secs = []
                    for r in range(runs + 1):              # (the first is the warm-up)
                        held.copy_(version_n)
                        torch.cuda.synchronize()
                        if a.traced and mname != "load_blocks":
                            sys.stderr.write("variant %s %s\n" % (name, variant))
                            sys.stderr.flush()
                        t0 = time.perf_counter()
                        res = fn()
                        secs.append(time.perf_counter() - t0)
                        assert res.complete and res.nblk == nblk, res.stats
                    secs = secs[1:]
                    v["stats"][mname] = res.stats
                    peak = torch.cuda.max_memory_allocated() - version_n.numel()
                    peak += res.stats.get("scratch_bytes", 0)
                    v["methods"][mname] = {"seconds": secs, "peak_device_bytes": peak}
                    print("%s %-12s %-14s %s s, peak %.1f MiB" % (
                        name, variant, mname, ["%.4f" % s for s in secs], peak / 2 ** 20),
                        flush=True)
                    where = fresh if mname == "reload_blocks" else held
                    for k in (0, nfiles // 2, nfiles - 1):
                        with open(os.path.join(rootb, files[k][0]), "rb") as f:
                            got = where[k * size:(k + 1) * size].cpu().numpy().tobytes()
                            assert got == f.read(), (mname, k)
                    where = None                           # (no tensor outlives its method)
                    if mname == "reload_blocks":
                        fresh = fresh_ptrs = None
                m = v["methods"]
                v["update_over_reload_median"] = (median(m["update_blocks"]["seconds"]) /
                                                  median(m["reload_blocks"]["seconds"]))
                v["update_over_load_median"] = (median(m["update_blocks"]["seconds"]) /
                                                median(m["load_blocks"]["seconds"]))
                out["variants"][variant] = v
            result["cases"][name] = out
            del held, version_n
            shutil.rmtree(os.path.join(base, name))
    finally:
        shutil.rmtree(base, ignore_errors=True)
        ctx.close()
    if a.traced:
        return 0
    # the laps: a process of its own, so that the timed runs above print nothing
    env = dict(os.environ, CIR_TRACE="1")
    argv = [sys.executable, os.path.abspath(__file__), "--traced", "--small-files",
            str(a.small_files), "--large-files", str(a.large_files)]
    if a.tmp:
        argv += ["--tmp", a.tmp]
    child = subprocess.run(argv, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           check=True, text=True)
    trace, key = {}, None
    for line in child.stderr.splitlines():
        if line.startswith("variant "):  # (the run after the warm-up stays, per method)
            key = line[len("variant "):]
        elif key and line.startswith(("cir update_blocks", "cir reload_blocks")):
            trace.setdefault(key, {})[line.split(":")[0]] = line
    result["trace"] = trace
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {vn: round(v["update_over_reload_median"], 3)
                          for vn, v in t["variants"].items()}
                      for k, t in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
