#!/usr/bin/env python3
"""What the index of device-resident files costs, timed (one GPU).

cir_index_memory_dev over files that lie in HBM, against what it is made of and
against the only way to such an index before it:

  shape "large": 32 GiB as 1,024 files of 32 MiB  (1 Mi blocks of 32 KiB)
  shape "small": 200,000 files of 32 KiB          (200,000 blocks)

per shape, in the same rounds, alternating:
  * index_memory        the call, device emitter (the default);
  * index_memory_host   the same call under CIR_EMIT=host: the digests come
                        down and the host emits the text;
  * hash_chunks         cir_hash_chunks_dev alone over the same bytes (the files
                        are slices of one allocation, so one call covers them):
                        the floor, hash and nothing else;
and once, on the first 2 GiB of the large shape: the bytes copied to the host,
written to a tmpfs directory and scanned with cir_scan_v1 (the write and the
scan timed apart), with the index compared byte for byte.

One process, one warm-up of every side, --runs rounds, a host clock around
whole calls that end in a synchronise.  The argument arrays are built once,
outside the clock.  Everything goes to profiles/index_memory/bench.json (--out)
as lists of seconds; a child process under CIR_TRACE=1 repeats one call per
shape and side, and its "cir index_memory:" lines go to trace.log beside it.
--scale divides both shapes (a quick run on a small card or a busy one).
"""
import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

BS = 32768
SHAPES = {"large": (1024, 32 << 20), "small": (200000, 32 << 10)}


class Case:
    """nfiles files of fsize bytes in one device allocation, and the argument
    arrays of cir_index_memory_dev over them."""

    def __init__(self, ca, torch, name, nfiles, fsize, seed):
        self.name, self.nfiles, self.fsize = name, nfiles, fsize
        self.nbytes = nfiles * fsize
        self.data = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        ca._n.check(ca._n.lib.cir_fill_splitmix64_dev(self.data.data_ptr(), self.nbytes, seed,
                                                      0, 0, 0))
        torch.cuda.synchronize()
        paths = [b"/d%03d/f%06d" % (i % 256, i) for i in range(nfiles)]
        blob = b"".join(paths)
        offs = [0]
        for p in paths:
            offs.append(offs[-1] + len(p))
        self.paths = paths
        self.c_paths = ctypes.create_string_buffer(blob, len(blob))
        self.c_off = (ctypes.c_uint64 * (nfiles + 1))(*offs)
        self.c_sizes = (ctypes.c_uint64 * nfiles)(*([fsize] * nfiles))
        base = self.data.data_ptr()
        self.c_ptrs = (ctypes.c_void_p * nfiles)(*[base + i * fsize for i in range(nfiles)])
        self.nblk = self.nbytes // BS
        self.out = torch.empty(32 * self.nblk, dtype=torch.uint8, device="cuda")


def timed_index_memory(ca, ctx, case, nfiles=None):
    n = ca._n
    nfiles = case.nfiles if nfiles is None else nfiles
    out, out_len = ctypes.c_void_p(), ctypes.c_size_t()
    iid = ctypes.create_string_buffer(32)
    st = (ctypes.c_uint64 * n.CIR_MEMINDEX_STATS_FIELDS)()
    t0 = time.perf_counter()
    n.check(n.lib.cir_index_memory_dev(ctx.handle, n.CIR_HASH_BLAKE2B_256, BS, case.c_paths,
                                       case.c_off, case.c_sizes, None, nfiles, case.c_ptrs, 0,
                                       ctypes.byref(out), ctypes.byref(out_len), iid, st))
    dt = time.perf_counter() - t0
    index = ctypes.string_at(out.value, out_len.value)
    n.lib.cir_free(out)
    return dt, index, list(st)


def timed_chunks(ca, torch, ctx, case):
    t0 = time.perf_counter()
    ctx.hash_chunks_dev(case.data.data_ptr(), case.nbytes, BS, case.out.data_ptr(), 0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def scan_arm(ca, torch, ctx, case, nbytes, tmp_root):
    """The first nbytes of the case through a file system: device -> host ->
    tmpfs files -> cir_scan_v1; the index must equal index_memory's."""
    nfiles = nbytes // case.fsize
    root = tempfile.mkdtemp(prefix="index_memory_bench_", dir=tmp_root)
    try:
        t0 = time.perf_counter()
        host = case.data[:nfiles * case.fsize].cpu().numpy()
        t1 = time.perf_counter()
        for i in range(nfiles):
            full = os.path.join(os.fsencode(root), case.paths[i][1:])
            os.makedirs(os.path.dirname(full), exist_ok=True)
            with open(full, "wb") as f:
                f.write(host[i * case.fsize:(i + 1) * case.fsize].data)
        t2 = time.perf_counter()
        cfg = ca.ScannerConfig()
        cfg.block_size(BS)
        cfg.add_dir(root, "/")
        ca.v1.scan(cfg, context=ctx)                    # warm-up: the staging slots
        t3 = time.perf_counter()
        scanned = ca.v1.scan(cfg, context=ctx)
        t4 = time.perf_counter()
        dt, index, _ = timed_index_memory(ca, ctx, case, nfiles)
        return {"bytes": nfiles * case.fsize, "files": nfiles, "download_s": t1 - t0,
                "write_s": t2 - t1, "scan_s": t4 - t3, "index_memory_s": dt,
                "identical": scanned == index, "tmp_root": tmp_root}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def traced_child(scale):
    import torch
    import ciruela_amd as ca
    ctx = ca.Context(device_mask=1)
    for name, (nfiles, fsize) in SHAPES.items():
        case = Case(ca, torch, name, max(nfiles // scale, 1), fsize, 1)
        for env in (None, "host"):
            if env:
                os.environ["CIR_EMIT"] = env
            else:
                os.environ.pop("CIR_EMIT", None)
            timed_index_memory(ca, ctx, case)           # warm-up
            sys.stderr.write("# %s, %s emitter\n" % (name, env or "device"))
            sys.stderr.flush()
            timed_index_memory(ca, ctx, case)
        del case
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--scan-bytes", type=int, default=2 << 30)
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_memory", "bench.json"))
    ap.add_argument("--traced-child", action="store_true")
    a = ap.parse_args()
    if a.traced_child:
        return traced_child(a.scale)
    import torch
    import ciruela_amd as ca
    ctx = ca.Context(device_mask=1)
    res = {"block_size": BS, "runs": a.runs, "scale": a.scale,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, (nfiles, fsize) in SHAPES.items():
        case = Case(ca, torch, name, max(nfiles // a.scale, 1), fsize, 1)
        sec = {"index_memory": [], "index_memory_host": [], "hash_chunks": []}
        os.environ.pop("CIR_EMIT", None)
        _, ref, st = timed_index_memory(ca, ctx, case)  # warm-ups, and the answers
        os.environ["CIR_EMIT"] = "host"
        _, href, hst = timed_index_memory(ca, ctx, case)
        timed_chunks(ca, torch, ctx, case)
        for r in range(a.runs):
            order = ["index_memory", "index_memory_host", "hash_chunks"]
            order = order[r % 3:] + order[:r % 3]
            for side in order:
                if side == "hash_chunks":
                    sec[side].append(timed_chunks(ca, torch, ctx, case))
                    continue
                if side == "index_memory_host":
                    os.environ["CIR_EMIT"] = "host"
                else:
                    os.environ.pop("CIR_EMIT", None)
                dt, index, _ = timed_index_memory(ca, ctx, case)
                assert index == ref
                sec[side].append(dt)
        os.environ.pop("CIR_EMIT", None)
        shape = {"files": case.nfiles, "file_bytes": fsize, "bytes": case.nbytes,
                 "blocks": case.nblk, "index_bytes": len(ref), "identical": ref == href,
                 "stats": dict(zip(ca.MEMINDEX_STATS_FIELDS, st)),
                 "stats_host": dict(zip(ca.MEMINDEX_STATS_FIELDS, hst)), "seconds": sec}
        if name == "large" and a.scan_bytes and os.path.isdir(a.tmp):
            shape["through_a_file_system"] = scan_arm(ca, torch, ctx, case,
                                                      min(a.scan_bytes, case.nbytes), a.tmp)
        res["shapes"][name] = shape
        for side, v in sec.items():
            print("%s %-18s min %.2f ms  median %.2f ms  max %.2f ms" % (
                name, side, 1e3 * min(v), 1e3 * sorted(v)[len(v) // 2], 1e3 * max(v)), flush=True)
        del case
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    env = dict(os.environ, CIR_TRACE="1")
    env.pop("CIR_EMIT", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced-child", "--scale",
                        str(a.scale)], capture_output=True, env=env, text=True)
    lines = [ln for ln in p.stderr.splitlines()
             if ln.startswith("cir index_memory:") or ln.startswith("# ")]
    with open(os.path.join(os.path.dirname(a.out), "trace.log"), "w") as f:
        f.write("\n".join(lines) + "\n")
    res["traced_child_status"] = p.returncode
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "shapes"}))


if __name__ == "__main__":
    main()
