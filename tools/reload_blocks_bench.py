#!/usr/bin/env python3
"""The next version of an image loaded over the one held in HBM, timed (one GPU).

cir_reload_blocks is cir_load_blocks for a process that holds the previous
version in device memory.  This times it over the two trees of DESIGN.md 4.5o,
built under a temporary directory --

  small: 20,000 files of 32 KiB          (per-file latency decides)
  large: 2,048 files of 1 MiB            (bandwidth decides)

-- version N loaded with load_blocks and kept in its tensors, and then the tree
changed on disk into three versions N + 1, one on top of the other:

  one_in_1000   one byte flipped in every 1,000th block
  one_in_10     every tenth file replaced by new random bytes
  every_block   one byte flipped in every block

Each version is indexed by the CPU restatement (oracle/cpu_indexer.py) and
loaded into a second set of tensors, one warm-up and three timed runs of each
of, in one process:

  reload_blocks   Context.reload_blocks with version N's tensors as resident
  load_blocks     Context.load_blocks of the same tree: the baseline

Every run, the stats arrays and "reload_over_load_median" go to
profiles/reload_blocks/bench.json (--out); nothing is gated.  The library's
laps come from a child process of this script under CIR_TRACE=1 (one run of
each version), whose `cir reload_blocks:` lines are kept per version.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cpu_indexer  # noqa: E402
from check_blocks_bench import build_tree, index_files, median, timed  # noqa: E402

VARIANTS = ("one_in_1000", "one_in_10", "every_block")


def _flip(path, offsets):
    with open(path, "r+b") as f:
        for at in offsets:
            f.seek(at)
            c = f.read(1)
            f.seek(at)
            f.write(bytes([c[0] ^ 0x5A]))


def mutate(variant, rootb, files, size, bs):
    """Changes the tree in place; returns how many blocks it changed."""
    per = (size + bs - 1) // bs
    if variant == "one_in_10":
        for rel, _ in files[::10]:
            with open(os.path.join(rootb, rel), "wb") as f:
                f.write(os.urandom(size))
        return len(files[::10]) * per
    every = 1000 if variant == "one_in_1000" else 1
    n = 0
    for i, (rel, _) in enumerate(files):
        blocks = [j for j in range(per) if (i * per + j) % every == 0]
        if blocks:
            _flip(os.path.join(rootb, rel), [j * bs + 5 for j in blocks])
            n += len(blocks)
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reload_blocks", "bench.json"))
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
    base = tempfile.mkdtemp(prefix="reload_blocks_bench_", dir=a.tmp)
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
            held = [torch.empty(size, dtype=torch.uint8, device="cuda:0") for _ in range(nfiles)]
            fresh = [torch.empty(size, dtype=torch.uint8, device="cuda:0") for _ in range(nfiles)]
            torch.cuda.synchronize()
            assert ctx.load_blocks(root, index_n, [t.data_ptr() for t in held]).complete
            # (plain pointers: the wrapper then looks at no tensor inside the timed call)
            resident = [(t.data_ptr(), size) for t in held]
            ptrs = [t.data_ptr() for t in fresh]
            out = {"files": nfiles, "file_bytes": size, "bytes": nfiles * size, "blocks": nblk,
                   "block_size": bs, "variants": {}}
            for variant in VARIANTS:
                changed = mutate(variant, rootb, files, size, bs)
                index = cpu_indexer.index(root, bs, 4, lib)
                v = {"changed_blocks": changed, "methods": {}, "stats": {}}

                def reload_blocks():
                    if a.traced:
                        sys.stderr.write("variant %s %s\n" % (name, variant))
                        sys.stderr.flush()
                    res = ctx.reload_blocks(root, index, ptrs, resident)
                    assert res.complete and res.nblk == nblk, res.stats
                    v["stats"]["reload_blocks"] = res.stats

                def load_blocks():
                    res = ctx.load_blocks(root, index, ptrs)
                    assert res.complete and res.nblk == nblk, res.stats
                    v["stats"]["load_blocks"] = res.stats

                for mname, fn in (("reload_blocks", reload_blocks), ("load_blocks", load_blocks)):
                    fresh[nfiles // 2].zero_()
                    secs = timed(fn, runs)
                    v["methods"][mname] = {"seconds": secs}
                    print("%s %-12s %-14s %s s" % (name, variant, mname,
                                                   ["%.4f" % s for s in secs]), flush=True)
                    for k in (0, nfiles // 2, nfiles - 1):
                        with open(os.path.join(rootb, files[k][0]), "rb") as f:
                            assert fresh[k].cpu().numpy().tobytes() == f.read(), (mname, k)
                v["reload_over_load_median"] = (median(v["methods"]["reload_blocks"]["seconds"]) /
                                                median(v["methods"]["load_blocks"]["seconds"]))
                out["variants"][variant] = v
            result["cases"][name] = out
            del held, fresh
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
        if line.startswith("variant "):  # (twice per version: the run after the warm-up stays)
            key = line[len("variant "):]
            trace[key] = []
        elif key and line.startswith(("cir reload_blocks", "cir load_blocks")):
            trace[key].append(line)
    result["trace"] = trace
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {vn: round(v["reload_over_load_median"], 3)
                          for vn, v in t["variants"].items()}
                      for k, t in result["cases"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
