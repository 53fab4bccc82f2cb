#!/usr/bin/env python3
"""Verify of the hardlink candidates before a download, four ways (one GPU).

check_and_hardlink (src/daemon/disk/public.rs:285-346) re-hashes every file
of a new image that an older image holds unchanged.  This times that verify
over two sets of candidates built under a temporary directory --

  small: 20,000 files of 32 KiB          (per-file latency decides)
  large: 2,048 files of 1 MiB            (bandwidth decides)

-- each spread over 4 source roots (candidate i lives under root i % 4; the
roots' files are hardlinks of one tree that holds them all, so the bytes
exist once), indexed by the CPU restatement (oracle/cpu_indexer.py), one
warm-up and three timed runs of:

  batched      Context.check_links          (cir_check_links: one call)
  per_file     a Context.check_file loop over the same candidates
               (cir_check_file, one fd per call, plus the mode test: the only
               way before cir_check_links)
  cpu4         hashlib on 4 threads over the same candidates
  check_index  Context.check_index over the one tree that holds every file:
               the same bytes through the same pipeline with one root and one
               verdict, the pipeline's own ceiling

and writes every run, GiB/s, files/s and the batched check's stats array to
profiles/check_links/bench.json (--out).  The yardstick is the per-file loop
in the same process: the batched check must beat it by more than the spread
of the runs.  --methods limits the run, and names two more methods that say
where the batched check's time goes beside check_index (run them under
CIR_TRACE=1 for the library's own phase timings on stderr):

  batched_c_call    cir_check_links through ctypes with the argument arrays
                    built beforehand (without the Python wrapper's marshalling
                    and its LinksResult)
  batched_one_root  Context.check_links with every candidate under the one
                    tree (without the other roots' directory opens)
"""
import argparse
import ctypes
import json
import os
import shutil
import stat
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
NROOTS = 4
GIB = float(1 << 30)


def build_tree(root, nfiles, size, per_dir=1000):
    """nfiles files of `size` bytes, distinct windows of one random pool."""
    pool = os.urandom((64 << 20) + size)
    step = max(1, (64 << 20) // nfiles) & ~15 or 16
    for i in range(nfiles):
        d = os.path.join(root, "d%03d" % (i // per_dir))
        if i % per_dir == 0:
            os.makedirs(d)
        path = os.path.join(d, "f%05d" % i)
        with open(path, "wb") as f:
            off = (i * step) % (64 << 20)
            f.write(pool[off:off + size])
        os.chmod(path, 0o644)


def index_files(index):
    """[(relative path, [digests])] of the file entries, index order (the
    position is the file ordinal: the trees hold no empty file)."""
    _, _, dirs, _ = dirsig_oracle.parse(index)
    out = []
    for vpath, entries in dirs:
        for e in entries:
            if e[0] == "f":
                assert e[3]
                out.append((os.path.join(vpath.lstrip(b"/"), e[1]), e[4]))
    return out


def spread(root, files, base):
    """NROOTS source roots under base: file i hardlinked into root i % NROOTS."""
    roots = [os.path.join(base, "src%d" % j) for j in range(NROOTS)]
    rootb = os.fsencode(root)
    made = set()
    for i, (rel, _) in enumerate(files):
        dst = os.path.join(os.fsencode(roots[i % NROOTS]), rel)
        d = os.path.dirname(dst)
        if d not in made:
            os.makedirs(d, exist_ok=True)
            made.add(d)
        os.link(os.path.join(rootb, rel), dst)
    return roots


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_links", "bench.json"))
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the trees are built (default: /dev/shm, else the system's)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small-files", type=int, default=20000)
    ap.add_argument("--large-files", type=int, default=2048)
    ap.add_argument("--methods", default="batched,per_file,cpu4,check_index")
    a = ap.parse_args()
    methods = a.methods.split(",")

    import ciruela_amd as ca
    lib = cpu_indexer.load()
    ctx = ca.Context(device_mask=1)
    h = dirsig_oracle.HASHES["blake2b/256"]
    result = {"block_size": BS, "runs": a.runs, "source_roots": NROOTS, "cases": {},
              "tmp": "tmpfs" if (a.tmp or "").startswith("/dev/shm") else "default"}
    base = tempfile.mkdtemp(prefix="check_links_bench_", dir=a.tmp)
    try:
        for name, nfiles, size in (("small", a.small_files, 32 << 10),
                                   ("large", a.large_files, 1 << 20)):
            case = os.path.join(base, name)
            root = os.path.join(case, "all")
            os.makedirs(root)
            build_tree(root, nfiles, size)
            index = cpu_indexer.index(root, BS, 4, lib)
            files = index_files(index)
            assert len(files) == nfiles
            roots = spread(root, files, case)
            links = [(i, i % NROOTS) for i in range(nfiles)]
            nbytes = nfiles * size
            stats = {}

            def batched():
                res = ctx.check_links(index, roots, links)
                assert res.stats["ok"] == nfiles, res
                stats.update(res.stats)

            def batched_one_root():
                res = ctx.check_links(index, [root], [(i, 0) for i in range(nfiles)])
                assert res.stats["ok"] == nfiles, res

            n = ca._n
            c_index = ctypes.create_string_buffer(index, len(index))
            c_fds = (ctypes.c_int * NROOTS)(*[-100] * NROOTS)  # AT_FDCWD
            c_dirs = (ctypes.c_char_p * NROOTS)(*[os.fsencode(r) for r in roots])
            c_lf = (ctypes.c_uint64 * nfiles)(*range(nfiles))
            c_ls = (ctypes.c_uint32 * nfiles)(*[i % NROOTS for i in range(nfiles)])
            c_kinds = (ctypes.c_uint8 * nfiles)()
            c_stats = (ctypes.c_uint64 * n.CIR_LINKS_STATS_FIELDS)()

            def batched_c_call():
                n.check(n.lib.cir_check_links(ctx.handle, ctypes.cast(c_index, ctypes.c_void_p),
                                              len(index), c_fds, c_dirs, NROOTS, c_lf, c_ls,
                                              nfiles, 0, c_kinds, None, c_stats))
                assert c_stats[0] == nfiles

            def one(i):
                rel, digests = files[i]
                fd = os.open(os.path.join(os.fsencode(roots[i % NROOTS]), rel),
                             os.O_RDONLY | os.O_NOFOLLOW)
                return fd, digests, rel

            def per_file():
                for i in range(nfiles):
                    fd, digests, rel = one(i)
                    try:
                        if not ctx.check_file(fd, BS, b"".join(digests)) or \
                                stat.S_IMODE(os.fstat(fd).st_mode) != 0o644:
                            raise AssertionError("checksum: %r" % rel)
                    finally:
                        os.close(fd)

            def cpu_one(i):
                fd, digests, rel = one(i)
                with os.fdopen(fd, "rb") as f:
                    data = f.read()
                    mode = stat.S_IMODE(os.fstat(f.fileno()).st_mode)
                if [h(data[k:k + BS]) for k in range(0, len(data), BS)] != digests or mode != 0o644:
                    raise AssertionError("checksum: %r" % rel)

            def cpu4():
                with ThreadPoolExecutor(4) as pool:
                    list(pool.map(cpu_one, range(nfiles), chunksize=64))

            def check_index():
                assert ctx.check_index(root, index).ok

            fns = {"batched": batched, "per_file": per_file, "cpu4": cpu4,
                   "check_index": check_index, "batched_c_call": batched_c_call,
                   "batched_one_root": batched_one_root}
            out = {"files": nfiles, "file_bytes": size, "bytes": nbytes, "methods": {}}
            for mname in methods:
                secs = timed(fns[mname], a.runs)
                out["methods"][mname] = {
                    "seconds": secs,
                    "GiBps": [nbytes / GIB / s for s in secs],
                    "files_per_s": [nfiles / s for s in secs],
                }
                print("%s %-11s %s s" % (name, mname, ["%.3f" % s for s in secs]), flush=True)
            if stats:
                out["stats"] = [stats[k] for k in ca.Context.LINKS_STATS_FIELDS]
                out["stats_fields"] = list(ca.Context.LINKS_STATS_FIELDS)
            m = out["methods"]
            if "batched" in m and "per_file" in m:
                b, p = m["batched"]["seconds"], m["per_file"]["seconds"]
                out["batched_beats_per_file_beyond_spread"] = max(b) < min(p)
                out["speedup_median"] = sorted(p)[len(p) // 2] / sorted(b)[len(b) // 2]
            if "batched" in m and "check_index" in m:
                b, c = m["batched"]["seconds"], m["check_index"]["seconds"]
                # slower than the one-root check by more than the runs' spread?
                out["batched_below_check_index_beyond_spread"] = min(b) > max(c)
                out["batched_over_check_index_median"] = \
                    sorted(b)[len(b) // 2] / sorted(c)[len(c) // 2]
            result["cases"][name] = out
            shutil.rmtree(case)
    finally:
        shutil.rmtree(base, ignore_errors=True)
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: round(sorted(v["GiBps"])[len(v["GiBps"]) // 2], 3)
                          for m, v in t["methods"].items()}
                      for k, t in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
