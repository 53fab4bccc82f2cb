#!/usr/bin/env python3
"""Commit-time check of a whole image, three ways (one GPU).

commit_image (src/daemon/disk/commit.rs:51-117) re-hashes every file of an
image against its index.  This times that check over two trees built under a
temporary directory --

  small: 20,000 files of 32 KiB          (per-file latency decides)
  large: 2 GiB in files of 1 MiB         (bandwidth decides)

-- each indexed by the CPU restatement (oracle/cpu_indexer.py), one warm-up
and three timed runs of:

  batched   Context.check_index            (cir_check_index: one call)
  per_file  a Context.check_file loop over the index's files (cir_check_file,
            one fd per call: the binding INTEGRATION.md had before)
  cpu4      cpu_indexer.index at 4 threads, then a byte compare of the indexes

and writes every run, GiB/s, files/s and the batched check's stats array to
profiles/check_index/bench.json (--out).  The yardstick for the small tree is
the per-file loop in the same process: the batched check must beat it by more
than the spread of the runs.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cpu_indexer  # noqa: E402
import dirsig_oracle  # noqa: E402

BS = 32768
GIB = float(1 << 30)


def build_tree(root, nfiles, size, per_dir=1000):
    """nfiles files of `size` bytes, distinct windows of one random pool."""
    pool = os.urandom((64 << 20) + size)
    step = max(1, (64 << 20) // nfiles) & ~15 or 16
    for i in range(nfiles):
        d = os.path.join(root, "d%03d" % (i // per_dir))
        if i % per_dir == 0:
            os.makedirs(d)
        with open(os.path.join(d, "f%05d" % i), "wb") as f:
            off = (i * step) % (64 << 20)
            f.write(pool[off:off + size])


def index_files(index):
    """[(relative path, [digests])] of the non-empty files, index order."""
    _, _, dirs, _ = dirsig_oracle.parse(index)
    out = []
    for vpath, entries in dirs:
        for e in entries:
            if e[0] == "f" and e[3]:
                out.append((os.path.join(vpath.lstrip(b"/"), e[1]), b"".join(e[4])))
    return out


def timed(fn, runs):
    fn()  # warm-up
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_index", "bench.json"))
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the trees are built (default: /dev/shm, else the system's)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small-files", type=int, default=20000)
    ap.add_argument("--large-mib", type=int, default=2048)
    a = ap.parse_args()

    import ciruela_amd as ca
    lib = cpu_indexer.load()
    ctx = ca.Context(device_mask=1)
    result = {"block_size": BS, "runs": a.runs, "trees": {},
              "scan_rate_config5_GiBps": 51.97,  # BENCH_r06.json, the scan of a 50 GiB tree
              "tmp": "tmpfs" if (a.tmp or "").startswith("/dev/shm") else "default"}
    base = tempfile.mkdtemp(prefix="check_index_bench_", dir=a.tmp)
    try:
        for name, nfiles, size in (("small", a.small_files, 32 << 10),
                                   ("large", a.large_mib, 1 << 20)):
            root = os.path.join(base, name)
            os.makedirs(root)
            build_tree(root, nfiles, size)
            index = cpu_indexer.index(root, BS, 4, lib)
            files = index_files(index)
            nbytes = nfiles * size
            assert len(files) == nfiles
            stats = {}

            def batched():
                res = ctx.check_index(root, index)
                assert res.ok, res
                stats.update(res.stats)

            def per_file():
                rootb = os.fsencode(root)
                for rel, digests in files:
                    fd = os.open(os.path.join(rootb, rel), os.O_RDONLY)
                    try:
                        if not ctx.check_file(fd, BS, digests):
                            raise AssertionError("checksum: %r" % rel)
                    finally:
                        os.close(fd)

            def cpu4():
                assert cpu_indexer.index(root, BS, 4, lib) == index

            tree = {"files": nfiles, "file_bytes": size, "bytes": nbytes, "methods": {}}
            for mname, fn in (("batched", batched), ("per_file", per_file), ("cpu4", cpu4)):
                secs = timed(fn, a.runs)
                tree["methods"][mname] = {
                    "seconds": secs,
                    "GiBps": [nbytes / GIB / s for s in secs],
                    "files_per_s": [nfiles / s for s in secs],
                }
                print("%s %-8s %s s" % (name, mname, ["%.3f" % s for s in secs]), flush=True)
            tree["stats"] = [stats[k] for k in ca.Context.CHECK_STATS_FIELDS]
            tree["stats_fields"] = list(ca.Context.CHECK_STATS_FIELDS)
            b, p = tree["methods"]["batched"]["seconds"], tree["methods"]["per_file"]["seconds"]
            tree["batched_beats_per_file_beyond_spread"] = max(b) < min(p)
            tree["speedup_median"] = sorted(p)[len(p) // 2] / sorted(b)[len(b) // 2]
            result["trees"][name] = tree
            shutil.rmtree(root)
    finally:
        shutil.rmtree(base, ignore_errors=True)
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: round(sorted(v["GiBps"])[len(v["GiBps"]) // 2], 3)
                          for m, v in t["methods"].items()}
                      for k, t in result["trees"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
