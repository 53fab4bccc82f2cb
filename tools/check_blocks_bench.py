#!/usr/bin/env python3
"""Which blocks of an image a directory already holds, timed (one GPU).

After a restart the reference removes a partial image and fetches all of it
again ("Resuming download", src/daemon/tracking/mod.rs:561-585; start_image,
src/daemon/disk/public.rs:91-93; fill_blocks,
src/daemon/tracking/progress.rs:129-170).  cir_check_blocks answers with one
bit per block of the index instead.  This times it over the two trees of
DESIGN.md 4.5a, built under a temporary directory --

  small: 20,000 files of 32 KiB          (per-file latency decides)
  large: 2,048 files of 1 MiB            (bandwidth decides)

-- indexed by the CPU restatement (oracle/cpu_indexer.py), one warm-up and
three timed runs of each of:

  complete     Context.check_blocks on the complete tree                (a)
  complete_c   cir_check_blocks through ctypes with the arguments built
               beforehand (without the Python wrapper's BlocksResult)
  check_index  Context.check_index on the same tree: the same bytes through
               the same pipeline with one verdict -- the yardstick for (a)
  cpu4         hashlib on 4 threads over the same files
  absent       check_blocks with 5 % of the files (seeded) absent       (c)
  truncated    check_blocks with a seeded random half of the files
               truncated to a random length                             (b)

and writes every run, GiB/s of the bytes the index lists, and the stats
arrays to profiles/check_blocks/bench.json (--out).  The expectation for (a):
the C call's median does not exceed the slowest of check_index's three runs
(it moves the same bytes and adds 8 * ceil(n / 64) bytes back per batch);
"complete_c_within_check_index_spread" records whether it held.  (b) and (c)
are recorded, not gated; their block counts are checked against what the
mutations leave.  Run under CIR_TRACE=1 for the library's phase timings on
stderr.
"""
import argparse
import ctypes
import json
import os
import random
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

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
    """[(relative path, [digests])] of the file entries, index order."""
    _, _, dirs, _ = dirsig_oracle.parse(index)
    out = []
    for vpath, entries in dirs:
        for e in entries:
            if e[0] == "f":
                out.append((os.path.join(vpath.lstrip(b"/"), e[1]), e[4]))
    return out


def timed(fn, runs):
    fn()  # warm-up
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_blocks", "bench.json"))
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the trees are built (default: /dev/shm, else the system's)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small-files", type=int, default=20000)
    ap.add_argument("--large-files", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()

    import ciruela_amd as ca
    n = ca._n
    lib = cpu_indexer.load()
    ctx = ca.Context(device_mask=1)
    h = dirsig_oracle.HASHES["blake2b/256"]
    result = {"block_size": BS, "runs": a.runs, "seed": a.seed, "cases": {},
              "tmp": "tmpfs" if (a.tmp or "").startswith("/dev/shm") else "default"}
    base = tempfile.mkdtemp(prefix="check_blocks_bench_", dir=a.tmp)
    try:
        for name, nfiles, size in (("small", a.small_files, 32 << 10),
                                   ("large", a.large_files, 1 << 20)):
            root = os.path.join(base, name, "img")
            aside = os.path.join(base, name, "aside")
            os.makedirs(root)
            os.makedirs(aside)
            build_tree(root, nfiles, size)
            index = cpu_indexer.index(root, BS, 4, lib)
            files = index_files(index)
            assert len(files) == nfiles
            per_file = (size + BS - 1) // BS
            nblk = nfiles * per_file
            nbytes = nfiles * size
            rootb = os.fsencode(root)
            stats = {}

            def blocks(key, have, states):
                def run():
                    res = ctx.check_blocks(root, index)
                    assert res.nblk == nblk and res.stats["have"] == have, (key, res)
                    got = {s: res.states.count(s) for s in set(res.states)}
                    assert got == {k: v for k, v in states.items() if v}, (key, got)
                    stats[key] = [res.stats[k] for k in ca.Context.BLOCKS_STATS_FIELDS]
                return run

            c_index = ctypes.create_string_buffer(index, len(index))
            c_stats = (ctypes.c_uint64 * n.CIR_BLOCKS_STATS_FIELDS)()

            def complete_c():
                have, state = ctypes.c_void_p(), ctypes.c_void_p()
                nb, nf = ctypes.c_uint64(), ctypes.c_size_t()
                n.check(n.lib.cir_check_blocks(ctx.handle, -100, rootb,
                                               ctypes.cast(c_index, ctypes.c_void_p), len(index),
                                               0, ctypes.byref(have), ctypes.byref(nb),
                                               ctypes.byref(state), None, ctypes.byref(nf),
                                               c_stats))
                n.lib.cir_free(have)
                n.lib.cir_free(state)
                assert c_stats[0] == nblk and c_stats[2] == nfiles

            def check_index():
                assert ctx.check_index(root, index).ok

            def cpu_one(i):
                rel, digests = files[i]
                with open(os.path.join(rootb, rel), "rb") as f:
                    data = f.read()
                if [h(data[k:k + BS]) for k in range(0, len(data), BS)] != digests:
                    raise AssertionError("checksum: %r" % rel)

            def cpu4():
                with ThreadPoolExecutor(4) as pool:
                    list(pool.map(cpu_one, range(nfiles), chunksize=64))

            out = {"files": nfiles, "file_bytes": size, "bytes": nbytes, "blocks": nblk,
                   "methods": {}}

            def record(mname, fn):
                secs = timed(fn, a.runs)
                out["methods"][mname] = {"seconds": secs,
                                         "GiBps": [nbytes / GIB / s for s in secs],
                                         "files_per_s": [nfiles / s for s in secs]}
                print("%s %-11s %s s" % (name, mname, ["%.3f" % s for s in secs]), flush=True)

            # (a) and its yardsticks, the two GPU checks alternating
            record("check_index", check_index)
            record("complete", blocks("complete", nblk, {"complete": nfiles}))
            record("complete_c", complete_c)
            record("check_index_again", check_index)
            record("cpu4", cpu4)
            # (c) 5 % of the files absent: moved aside, and back afterwards
            rng = random.Random(a.seed)
            gone = rng.sample(range(nfiles), nfiles // 20)
            for i in gone:
                os.rename(os.path.join(rootb, files[i][0]),
                          os.path.join(os.fsencode(aside), b"%d" % i))
            record("absent", blocks("absent", nblk - len(gone) * per_file,
                                    {"complete": nfiles - len(gone), "absent": len(gone)}))
            for i in gone:
                os.rename(os.path.join(os.fsencode(aside), b"%d" % i),
                          os.path.join(rootb, files[i][0]))
            # (b) a random half of the files truncated to a random length (last:
            # it destroys the tree)
            cut = rng.sample(range(nfiles), nfiles // 2)
            have = nblk
            for i in cut:
                length = rng.randrange(size)
                os.truncate(os.path.join(rootb, files[i][0]), length)
                have -= per_file - length // BS
            record("truncated", blocks("truncated", have,
                                       {"complete": nfiles - len(cut), "partial": len(cut)}))
            out["stats"] = stats
            out["stats_fields"] = list(ca.Context.BLOCKS_STATS_FIELDS)
            m = out["methods"]
            yard = m["check_index"]["seconds"] + m["check_index_again"]["seconds"]
            out["check_index_slowest_of_first_three"] = max(m["check_index"]["seconds"])
            out["check_index_slowest_of_six"] = max(yard)
            out["complete_c_median"] = median(m["complete_c"]["seconds"])
            out["complete_c_within_check_index_spread"] = \
                out["complete_c_median"] <= max(m["check_index"]["seconds"])
            out["complete_over_check_index_median"] = \
                median(m["complete"]["seconds"]) / median(m["check_index"]["seconds"])
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
