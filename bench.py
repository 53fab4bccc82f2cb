#!/usr/bin/env python3
"""Device-resident BLAKE2b-256 block hashing on MI355X (BASELINE.json metric).

One step = one pass of the hot path (cir_hash_chunks_dev: Hashes::hash_file
over a device-resident arena, one launch) over one GPU's batch:
  N = 1 : config 2 — 1,048,576 x 32 KiB blocks (32 GiB) of splitmix64 bytes
          (seed 0x5EED0002), blocks 0-15 all-zero, 16-31 bytes(range(256))*128.
  N > 1 : config 4 — rank g holds global blocks [g*2^20, (g+1)*2^20), block i
          = splitmix64 stream seeded 0x5EED0004 ^ i; no collective on the data
          path (range split), weak scaling.
Inputs are generated in HBM before timing.  W warmup steps, then K timed
steps bracketed by barrier + synchronize; value = all ranks' bytes / max
rank time.  The dominant kernel is also timed per launch with HIP events on
the launch stream for the roofline object; `traffic` comes from the
committed rocprofv3 PMC summary (profiles/) when one matches this config.

cpu_baseline: the oracle (C restatement of RFC 7693 BLAKE2b-256 +
dir-signature's block split, "port") on the host cores of this box, over a
bounded sample of the same config-2 blocks, at 4 threads (the reference's
default --disk-threads), at the per-GPU CPU share (16) and at one thread per
CPU of the affinity mask; the host record names the cgroup CPU quota.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--loader api|glds|direct]
        (the headline figure alone: set-up, W warmup steps, K timed steps, one
        JSON line with value and ms_per_step; the roofline's fields that the
        timed steps' own events give)
    python bench.py ... --full
        (what else the line carries: the parity checks -- golden digests and
        step-to-step identity, sampled oracle digests at N>1 --, the CPU
        baseline, the roofline's VALU ceiling timed live, at N=1 config5,
        config3, config2host and config1 as `secondary` records, at N>1
        devices_seen; without it `parity` says that nothing was checked)
    python bench.py ... --dump-outputs DIR
        (the digests the last timed step left in the caller's buffer, as
        DIR/digests.npy: float32, one row of 32 byte values per block, all
        blocks or a fixed seeded sample with its indices in
        DIR/digests_blocks.npy; the inputs are the same in every run)
    python bench.py --workload config3|config5|config1|config2host|config2sha
        (one secondary config on its own)
    python bench.py --gpus N   (N > 1: launches N ranks itself through
        torch.distributed.run unless WORLD_SIZE is already set)
    python bench.py --gpus 1 --force-dist   (the N>1 code path -- process
        group, config 4, job-wide parity -- on one rank, launched the same way)

With --full the N>1 line also carries devices_seen: every rank's PCI bus id, UUID and
device clocks (cir_debug_device_identity), gathered over the process group;
under RCCL two ranks on one device fail the line.  Config 1's CLI is timed
before this process touches the GPU; config 5 adds a cold scan of the tree
it has just written (value_cold) before the read passes and timed scans.

config.entry_point names the C-ABI call the timed steps made:
cir_hash_chunks_dev (the production path, --loader api, the default) or
cir_debug_hash_uniform_dev (a single-kernel A/B variant, --loader glds|direct).
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GIB = float(1 << 30)
METRIC = "GiB/s block-hashed (device-resident, blocks in HBM) at 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
SEED_C2 = 0x5EED0002
SEED_C4 = 0x5EED0004
PARITY_NOT_CHECKED = "not checked (--full checks it)"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--blocks", type=int, default=1 << 20, help="blocks per GPU")
    p.add_argument("--block-size", type=int, default=32768)
    p.add_argument("--loader", choices=["glds", "direct", "api"], default="api",
                   help="api = cir_hash_chunks_dev (the production path); glds / direct = "
                        "cir_debug_hash_uniform_dev with the LDS-DMA / per-lane loader")
    p.add_argument("--workload", choices=["auto", "config3", "config5", "config1", "config2host",
                                          "config2sha"],
                   default="auto", help="auto = config2 at N=1, config4 at N>1")
    p.add_argument("--tree-gib", type=float, default=50.0, help="config5 tree size")
    p.add_argument("--host-gib", type=int, default=32, help="config2host buffer size")
    p.add_argument("--staging-mib", type=int, default=0,
                   help="staging buffer size of the host paths (0 = library default, 256)")
    p.add_argument("--tree-dir", default="/dev/shm/ciruela_bench_tree")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-secondary", action="store_true",
                   help="N=1 default line without the secondary config3 / config2host / "
                        "config5 records")
    p.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                   help="process group of the N>1 path (nccl = RCCL; gloo for rehearsals "
                        "with several ranks per GPU)")
    p.add_argument("--dry-run", action="store_true",
                   help="launcher and process-group plumbing only (gloo, no GPU, no hashing): "
                        "prints the line skeleton with the ranks the job saw (CPU tests)")
    p.add_argument("--force-dist", action="store_true",
                   help="run the N>1 code path (process group, config 4) even at world size 1")
    p.add_argument("--hash", choices=["blake2b", "sha512"], default="blake2b",
                   help="config 5: the index's hash type (ciruela sync uses blake2b/256; "
                        "sha512/256 is dir-signature's other type)")
    p.add_argument("--footer", choices=["host", "gpu", "ab"], default="host",
                   help="config 5: where the index footer is hashed (cir_set_footer_mode); "
                        "ab alternates host and gpu scans and reports both")
    p.add_argument("--scan-output", choices=["write", "buffer"], default="write",
                   help="config 5: the index appended to a bytearray as the scan writes it "
                        "(cir_scan_v1_write, the reference's v1::scan into a Vec) or returned "
                        "whole (cir_scan_v1) and copied out")
    p.add_argument("--dry-run-shared-device", action="store_true",
                   help="--dry-run only: every rank reports the same device identity (the "
                        "devices_seen check must fail the line under --dist-backend nccl)")
    p.add_argument("--dry-run-bad-rank", type=int, default=-1,
                   help="--dry-run only: this rank corrupts one digest of its shard (the "
                        "job-wide parity reduction must report FAIL)")
    p.add_argument("--cpu-seconds", type=float, default=2.5,
                   help="wall seconds of the 4-thread CPU-baseline measurement (all cores: "
                        "the same CPU work)")
    p.add_argument("--full", action="store_true",
                   help="everything beyond the headline figure: the parity checks, the CPU "
                        "baseline, the secondary configs (1, 3, 5, 2-from-host), the live VALU "
                        "ceiling of the roofline and, at N>1, the ranks' device identities")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the digests the last timed step returned "
                        "as DIR/digests.npy (float32, one row of 32 byte values per block; a "
                        "fixed seeded sample of the blocks when there are too many, their "
                        "indices in DIR/digests_blocks.npy)")
    return p.parse_args()


def fill_config2(ca, data, bs, stream):
    import torch
    ca._n.check(ca._n.lib.cir_fill_splitmix64_dev(data.data_ptr(), data.numel(), SEED_C2, 0, 0,
                                                  stream))
    nspecial = min(32, data.numel() // bs)
    data[:min(16, nspecial) * bs].zero_()
    if nspecial > 16:
        pat = torch.arange(256, dtype=torch.int32, device=data.device).to(torch.uint8)
        data[16 * bs:nspecial * bs].copy_(pat.repeat((nspecial - 16) * bs // 256))


DUMP_MAX_BYTES = 48 << 20  # of digests.npy; with the block indices, under 64 MB
DUMP_SEED = 0x5EEDD0


def dump_blocks(nblk):
    """The blocks --dump-outputs keeps: all of them while their digests fit
    DUMP_MAX_BYTES as float32, else the first and last 64 (the special
    blocks, the launch's edges) and a seeded draw of the rest -- the same
    blocks in every run of the same shape."""
    import numpy as np
    keep = DUMP_MAX_BYTES // (32 * 4)
    if nblk <= keep:
        return np.arange(nblk, dtype=np.int64)
    edge = 64
    rng = np.random.default_rng(DUMP_SEED)
    mid = rng.choice(nblk - 2 * edge, size=keep - 2 * edge, replace=False) + edge
    return np.concatenate([np.arange(edge), np.sort(mid),
                           np.arange(nblk - edge, nblk)]).astype(np.int64)


def dump_outputs(dirname, name, out):
    """What the caller of the timed path holds after its last step: `out`,
    the device buffer of 32-byte digests, as DIR/<name>.npy (float32, one
    row of 32 byte values per kept block) and the kept blocks' indices as
    DIR/<name>_blocks.npy (float64)."""
    import numpy as np
    import torch
    idx = dump_blocks(out.numel() // 32)
    rows = out.view(-1, 32)[torch.from_numpy(idx).to(out.device)].cpu().numpy()
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, name + ".npy"), rows.astype(np.float32))
    np.save(os.path.join(dirname, name + "_blocks.npy"), idx.astype(np.float64))


def load_traffic(cfg_key, field="hbm_bytes_per_launch"):
    """HBM bytes per launch (or per batch) from a committed PMC summary."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            d = json.load(f)
        e = d.get(cfg_key)
        return None if e is None else e.get(field)
    except (OSError, ValueError):
        return None


def load_oracle():
    """The C oracle (test infrastructure): the CPU baseline and the checker
    of the secondary legs, never the measured path."""
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "liboracle_blake2b.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.oracle_hash_chunks.argtypes = [vp, u64, u64, vp, ctypes.c_int]
    lib.oracle_hash_blocks.argtypes = [vp, vp, vp, ctypes.c_size_t, vp, ctypes.c_int]
    lib.oracle_splitmix64_fill.argtypes = [vp, u64, u64, u64, u64, u64]
    return lib


# CPU share of one GPU on the measurement boxes: gpurun gives a one-GPU box
# 16 host CPUs (OMP_NUM_THREADS / MAX_JOBS are set to 16 there) while
# os.cpu_count() and the affinity mask show the whole host.  The CPU baseline
# therefore has three legs over the same sample: 4 threads (the reference's
# default --disk-threads, src/client/global_options.rs:13), the per-GPU share
# (min(affinity, 16) threads) and every CPU in the affinity mask.
CPU_SHARE_PER_GPU = 16


def host_info():
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    quota = None
    try:  # cgroup v2 CPU quota ("max" or "quota period")
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()[:2]
        if q != "max":
            quota = round(int(q) / int(period), 2)
    except (OSError, ValueError):
        pass
    return {"nproc": os.cpu_count(), "affinity_cpus": len(os.sched_getaffinity(0)),
            "cgroup_cpu_quota": quota, "cpu_model": model,
            "cpu_share_per_gpu": CPU_SHARE_PER_GPU}


def per_gpu_share():
    return max(1, min(CPU_SHARE_PER_GPU, len(os.sched_getaffinity(0))))


def all_affinity():
    return max(1, len(os.sched_getaffinity(0)))


def cpu_rates(run, target_s):
    """run(threads) -> bytes hashed by one pass over the sample; repeated
    until `target_s` wall seconds at 4 threads (the same CPU work, so
    target_s * 4 / threads, at more threads; at least one pass).
    {threads: (GiB/s, bytes)} for 4, the per-GPU share and all affinity CPUs."""
    res = {}
    for threads in sorted({4, per_gpu_share(), all_affinity()}):
        wall = target_s * 4.0 / threads if threads > 4 else target_s
        done, t0 = 0, time.perf_counter()
        while True:
            done += run(threads)
            dt = time.perf_counter() - t0
            if dt >= wall:
                break
        res[threads] = (done / dt / GIB, done)
    return res


def cpu_record(res, sample, unit="GiB/s"):
    t4, pg, aa = res[4], res[per_gpu_share()], res[all_affinity()]
    return {"value": round(t4[0], 4), "unit": unit, "cores": 4, "kind": "port",
            "sample": sample,
            "per_gpu_share": {"value": round(pg[0], 4), "cores": per_gpu_share(),
                              "sample_bytes": pg[1],
                              "note": "the host CPUs one GPU's job gets on the measurement box"},
            "all_affinity": {"value": round(aa[0], 4), "cores": all_affinity(),
                             "sample_bytes": aa[1],
                             "note": "one thread per CPU of the process affinity mask"},
            "host": host_info()}


def cpu_baseline(bs, target_s):
    """Oracle BLAKE2b-256 over config-2 blocks on the host (bounded sample)."""
    import numpy as np
    lib = load_oracle()
    # one sample buffer (config-2 bytes of blocks 32.., 4 GiB), hashed over and
    # over until the measurement has run its share of the CPU work
    nmax = 1 << 17
    buf = np.empty(nmax * bs // 8, dtype=np.uint64)
    lib.oracle_splitmix64_fill(buf.ctypes.data, 32 * bs // 8, buf.size, SEED_C2, 0, 0)
    out = np.empty(nmax * 32, dtype=np.uint8)

    def run(threads):
        lib.oracle_hash_chunks(buf.ctypes.data, nmax * bs, bs, out.ctypes.data, threads)
        return nmax * bs
    return cpu_record(cpu_rates(run, target_s),
                      "%d x %d B config-2 blocks (4 GiB of blocks 32.., splitmix64 seed "
                      "0x5EED0002) re-hashed, oracle/blake2b_oracle.c; 4 threads = reference "
                      "default --disk-threads" % (nmax, bs))


def shard(rank, world, nblk_per_gpu):
    """Config 4 range split: rank g owns global blocks [g*n, (g+1)*n)."""
    return rank * nblk_per_gpu, nblk_per_gpu


def timed_steps(step, steps, sync, barrier=None):
    """The timed region of every rank: barrier + sync, exactly `steps` calls
    of step(i), sync + barrier; returns this rank's wall seconds."""
    if barrier is not None:
        barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    sync()
    if barrier is not None:
        barrier()
    return time.perf_counter() - t0


def max_over_ranks(seconds, device=None):
    """The slowest rank's time: all_reduce(MAX) over the process group (the
    identity without one).  device: where the reduced tensor lives (the
    rank's GPU for RCCL, None = host memory for gloo)."""
    import torch
    import torch.distributed as dist
    t = torch.tensor([seconds], dtype=torch.float64, device=device)
    # run whenever a process group exists, world size 1 included, so that a
    # one-rank --force-dist run exercises the same RCCL call as N ranks
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def job_rate(bytes_per_rank_step, world, steps, elapsed_max):
    """Whole-job GiB/s: all ranks' bytes over the slowest rank's time."""
    return bytes_per_rank_step * world * steps / elapsed_max / GIB


def entry_point(loader):
    """(C-ABI entry point the timed steps call, kernel loader it runs) for a
    --loader choice: the production call for "api", the A/B kernel for the
    others.  `traffic_key` picks the committed PMC summary of that launch."""
    if loader == "api":
        return {"entry_point": "cir_hash_chunks_dev", "loader": "lds-dma"}
    return {"entry_point": "cir_debug_hash_uniform_dev",
            "loader": "lds-dma" if loader == "glds" else "direct"}


def traffic_key(bs, nblk, loader):
    return "bs%d/n%d/%s" % (bs, nblk, entry_point(loader)["entry_point"]
                           if loader == "api" else "uniform-" + loader)


def job_summary(rank_stats, device=None):
    """Every rank's [mismatches, checked blocks, failed checks, kernel ms
    avg, kernel ms min] gathered on every rank (one all_gather over the
    process group; the identity at world size 1 or without one).  Returns
    the list of per-rank rows, rank order."""
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(x) for x in rank_stats], dtype=torch.float64, device=device)
    if dist.is_available() and dist.is_initialized():  # world size 1 included
        parts = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, t)
    else:
        parts = [t]
    return [[float(v) for v in p.cpu().tolist()] for p in parts]


def job_parity(rows, reasons=None):
    """The line's parity over every rank's row of job_summary: "ok" only
    when no rank found a mismatch or failed a check."""
    bad = int(sum(r[0] for r in rows))
    checked = int(sum(r[1] for r in rows))
    failed = [i for i, r in enumerate(rows) if r[0] or r[2]]
    if not failed:
        return "ok", checked
    msg = "FAIL: rank(s) %s: %d of %d checked digests differ" % (
        ",".join(map(str, failed)), bad, checked)
    if reasons:
        msg += " (%s)" % reasons
    return msg, checked


def device_identity(ca, device_index):
    """This rank's GPU as its driver and its own counters see it
    (cir_debug_device_identity): PCI bus id, UUID, and one wave's reads of
    the device's wall clock (s_memrealtime) and of its s_memtime counter
    ~100 us apart -- the wall clock's value is the device's own (GPUs of one
    node do not share it), and the counter rate is that GPU's clock."""
    bus = ctypes.create_string_buffer(64)
    uuid = ctypes.create_string_buffer(16)
    clk = (ctypes.c_uint64 * 5)()
    ca._n.check(ca._n.lib.cir_debug_device_identity(device_index, bus, 64, uuid, clk))
    rt0, rt1, c0, c1, khz = list(clk)
    wall_s = (rt1 - rt0) / (khz * 1e3) if khz and rt1 > rt0 else None
    return {"hip_device": device_index, "pci_bus_id": bus.value.decode(),
            "uuid": uuid.raw.hex(), "wall_clock_ticks": rt0, "wall_clock_khz": khz,
            "memtime_mhz": round((c1 - c0) / wall_s / 1e6, 1) if wall_s else None}


def gather_objects(obj):
    """Every rank's `obj`, rank order, on every rank (all_gather_object over
    the process group; [obj] without one)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        out = [None] * dist.get_world_size()
        dist.all_gather_object(out, obj)
        return out
    return [obj]


def devices_check(idents, one_device_per_rank):
    """(distinct, problem) over every rank's device identity: two ranks on
    one device (same PCI bus id or UUID) make the job's N GPUs fewer than N.
    With RCCL (one_device_per_rank) that fails the line; gloo rehearsals with
    shared GPUs only say so."""
    seen, shared = {}, []
    for r, d in enumerate(idents):
        for key in ("pci_bus_id", "uuid"):
            v = d.get(key)
            if v:
                if (key, v) in seen and seen[(key, v)] != r:
                    shared.append((seen[(key, v)], r, v))
                seen.setdefault((key, v), r)
    if not shared:
        return True, None
    pairs = sorted({(a, b) for a, b, _ in shared})
    msg = "ranks %s share a device (%s)" % (
        ", ".join("%d/%d" % p for p in pairs), shared[0][2])
    return False, ("FAIL: " + msg) if one_device_per_rank else msg


def config4_check(oracle_lib, digests, nbytes, bs, first_block, sample=64):
    """Config-4 shard parity outside the timed region: the first and last
    `sample` blocks of this rank's shard (the range boundaries) and `sample`
    blocks spread over it, regenerated on the host from their global block
    index and hashed by the oracle.  Returns the number of mismatches."""
    import numpy as np
    nblk = nbytes // bs
    picks = sorted(set(list(range(min(sample, nblk))) +
                       list(range(max(0, nblk - sample), nblk)) +
                       [int(x) for x in np.linspace(0, nblk - 1, sample)]))
    buf = np.empty(bs // 8, dtype=np.uint64)
    want = np.empty(32, dtype=np.uint8)
    bad = 0
    for b in picks:
        oracle_lib.oracle_splitmix64_fill(buf.ctypes.data, 0, buf.size, SEED_C4, bs // 8,
                                          first_block + b)
        oracle_lib.oracle_hash_chunks(buf.ctypes.data, bs, bs, want.ctypes.data, 1)
        bad += int(digests[32 * b:32 * b + 32].tobytes() != want.tobytes())
    return bad, len(picks)


def config3_layout(total=10 << 30, seed=0x5EED0003):
    """equal bytes per class (4 KiB / 32 KiB / 1 MiB),
    10 % of each class ragged U[1, size-1], shuffled; blocks packed at 128-B
    aligned offsets in descriptor order.  Returns (offsets, lengths, bytes)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = []
    for size in (4096, 32768, 1 << 20):
        count = (total // 3) // size
        ln = np.full(count, size, dtype=np.int64)
        rag = rng.random(count) < 0.1
        ln[rag] = rng.integers(1, size, size=int(rag.sum()))
        lens.append(ln)
    lens = np.concatenate(lens)
    lens = lens[rng.permutation(lens.size)]
    padded = (lens + 127) // 128 * 128
    offs = np.zeros(lens.size, dtype=np.int64)
    offs[1:] = np.cumsum(padded)[:-1]
    return offs, lens.astype(np.int32), int(offs[-1] + padded[-1])


def valu_ceiling(ca, nblk, bs, stream, reps=4):
    """Median time of nblk x ceil(bs/128) register-only compressions (the
    kernel's VALU work with no loads): the measured VALU ceiling."""
    import torch
    if nblk % 256 or bs % 128:
        return None
    buf = torch.empty(32 * nblk, dtype=torch.uint8, device=torch.cuda.current_device())
    ts = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ca._n.check(ca._n.lib.cir_debug_compress_only_dev(nblk, bs // 128, buf.data_ptr(), stream))
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return round(sorted(ts)[len(ts) // 2], 4)


def run_config3(args, ca, ctx, dev, stream):
    import numpy as np
    import torch
    offs, lens, nbytes = config3_layout()
    data = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ca._n.check(ca._n.lib.cir_fill_splitmix64_dev(data.data_ptr(), nbytes, 0x5EED0003, 0, 0,
                                                  stream))
    d_off = torch.from_numpy(offs).to(dev)
    d_len = torch.from_numpy(lens).to(dev)
    n = lens.size
    out = torch.empty(32 * n, dtype=torch.uint8, device=dev)

    def step():
        ca._n.check(ca._n.lib.cir_hash_blocks_dev(ctx.handle, data.data_ptr(), d_off.data_ptr(),
                                                  d_len.data_ptr(), n, out.data_ptr(), stream))
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    # HIP events around each batch's ordering, quad part and lane part on the
    # streams they run on, recorded by the library over the timed steps
    lib = ca._n.lib
    ca._n.check(lib.cir_debug_desc_timing(ctx.handle, 1))
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    parts = (ctypes.c_double * 5)()
    ca._n.check(lib.cir_debug_desc_times(ctx.handle, parts))
    ca._n.check(lib.cir_debug_desc_timing(ctx.handle, 0))
    nb = max(1.0, parts[0])
    order_ms, quad_ms, lane_ms, total_ms = (parts[k] / nb for k in (1, 2, 3, 4))
    hashed = int(lens.astype("int64").sum())
    algo = hashed + 32 * n
    # the same batch through the bounds-checked entry point (descriptors from
    # untrusted data: one more pass over them, include/ciruela_blockhash.h
    # cir_hash_blocks_dev_bounded), timed the same way: what the check costs
    out_b = torch.empty_like(out)
    nrange = torch.full((1,), -1, dtype=torch.int32, device=dev)

    def step_bounded():
        ca._n.check(lib.cir_hash_blocks_dev_bounded(
            ctx.handle, 1, data.data_ptr(), nbytes, d_off.data_ptr(), d_len.data_ptr(), n,
            out_b.data_ptr(), nrange.data_ptr(), stream))
    for _ in range(args.warmup):
        step_bounded()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step_bounded()
    torch.cuda.synchronize()
    dt_b = (time.perf_counter() - t0) / args.steps
    bounded = {"ms_per_step": round(dt_b * 1e3, 3), "value": round(hashed / dt_b / GIB, 3),
               "overhead_pct": round((dt_b / dt - 1) * 100, 2),
               "out_of_range": int(nrange.item()), "same_digests": bool(torch.equal(out, out_b))}
    del out_b
    got = out.cpu().numpy().reshape(-1, 32)
    del data, out
    torch.cuda.empty_cache()

    # oracle check + CPU baseline on the same sample: the first descriptors
    # whose blocks fill the first 2 GiB of the arena (shuffled order, so all
    # three classes and the ragged lengths are in it), regenerated on the host
    lib = load_oracle()  # noqa: F811 (the oracle from here on)
    k = int(np.searchsorted(offs, 2 << 30))
    prefix = int(offs[k - 1] + (lens[k - 1] + 127) // 128 * 128)
    host = np.empty(prefix // 8, dtype=np.uint64)
    lib.oracle_splitmix64_fill(host.ctypes.data, 0, host.size, 0x5EED0003, 0, 0)
    s_off = np.ascontiguousarray(offs[:k].astype(np.uint64))
    s_len = np.ascontiguousarray(lens[:k].astype(np.uint32))
    want = np.empty((k, 32), dtype=np.uint8)
    sample_bytes = int(s_len.astype(np.int64).sum())

    def run(threads):
        lib.oracle_hash_blocks(host.ctypes.data, s_off.ctypes.data, s_len.ctypes.data, k,
                               want.ctypes.data, threads)
        return sample_bytes
    rates = cpu_rates(run, args.cpu_seconds)
    matches = bool(np.array_equal(got[:k], want))
    return {"metric": "GiB/s block-hashed, config 3 (mixed 4K/32K/1M, 10% ragged, shuffled)",
            "value": round(hashed / dt / GIB, 3), "unit": "GiB/s", "ms_per_step": round(dt * 1e3, 3),
            "steps": args.steps, "warmup": args.warmup, "blocks": n, "bytes": hashed,
            "config": {"workload": "config3: 10 GiB of 4 KiB / 32 KiB / 1 MiB blocks (equal bytes "
                                   "per class), 10 % ragged, shuffled, device-resident"},
            "matches_oracle": matches, "oracle_checked_blocks": k,
            "bounded": bounded,
            "roofline": {
                "bound": "hbm", "achieved": round(algo / (total_ms / 1e3) / 1e9, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(algo / (total_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                "traffic": load_traffic("config3", "hbm_bytes_per_batch"),
                "traffic_scope": "per batch: every kernel of cir_hash_blocks_dev (PMC, "
                                 "profiles/pmc_traffic.json config3)",
                "kernel": "k_quad_long (dominant; 1 MiB chains in quad mode)",
                "kernel_ms_avg": round(quad_ms, 4), "batch_kernel_ms_avg": round(total_ms, 4),
                "parts_ms_avg": {"ordering": round(order_ms, 4), "quad_part": round(quad_ms, 4),
                                 "lane_part": round(lane_ms, 4)},
                "timed_batches": int(parts[0]),
                "note": "achieved = (sum of lengths + 32 B per digest) / (ordering start -> "
                        "last part end), HIP events on the streams the kernels run on; the "
                        "quad part is latency-bound (8192 dependent compressions per 1 MiB "
                        "chain), not HBM-bound: see DESIGN.md 4.2"},
            "cpu_baseline": cpu_record(rates, "the first %d descriptors of the config-3 order "
                                       "(%.2f GiB, all classes, ragged included), "
                                       "oracle_hash_blocks; 4 threads = reference default "
                                       "--disk-threads" % (k, sample_bytes / GIB)),
            "note": "includes the on-device longest-chain-first sort (order.hip); the test "
                    "suite checks every config-3 digest (test_gpu_fullsize.py)"}


def run_config2host(args, ca, ctx, dev, stream):
    """Config 2's blocks handed over in (pageable) host memory: cir_hash_memory
    = Hashes::hash_file over an in-memory file, digests back in host memory.
    The PCIe-inclusive rate of the headline shape; never `value`
    of the headline line."""
    import numpy as np  # noqa: F811
    import torch
    bs = args.block_size
    nbytes = args.host_gib << 30
    data = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fill_config2(ca, data, bs, stream)
    dev_out = torch.empty(nbytes // bs * 32, dtype=torch.uint8, device=dev)
    ca._n.check(ca._n.lib.cir_hash_chunks_dev(ctx.handle, data.data_ptr(), nbytes, bs,
                                              dev_out.data_ptr(), stream))
    torch.cuda.synchronize()
    want = dev_out.cpu().numpy().tobytes()
    host = np.empty(nbytes, dtype=np.uint8)
    torch.from_numpy(host).copy_(data)  # pageable host copy of the same bytes
    del data, dev_out
    torch.cuda.empty_cache()
    times = []
    for _ in range(max(1, args.steps)):
        t0 = time.perf_counter()
        got = ctx.hash_memory(host, bs)
        times.append(time.perf_counter() - t0)
    best = min(times)
    # oracle check + CPU baseline on the same host buffer: its first 4 GiB
    # (all special blocks included), Hashes::hash_file over memory on the CPU
    lib = load_oracle()
    sample = min(nbytes, 4 << 30)
    want_cpu = np.empty(sample // bs * 32, dtype=np.uint8)

    def run(threads):
        lib.oracle_hash_chunks(host.ctypes.data, sample, bs, want_cpu.ctypes.data, threads)
        return sample
    rates = cpu_rates(run, args.cpu_seconds)
    return {"metric": "GiB/s block-hashed from host memory, config 2 shape (PCIe-inclusive)",
            "value": round(nbytes / best / GIB, 3), "unit": "GiB/s",
            "seconds_best": round(best, 3), "seconds_all": [round(t, 3) for t in times],
            "config": {"workload": "config2host: %d x %d B blocks in a pageable host buffer "
                                   "(%.0f GiB), cir_hash_memory" % (nbytes // bs, bs, nbytes / GIB)},
            "bytes": nbytes, "block_size": bs, "entry_point": "cir_hash_memory",
            "matches_device_resident": got == want,
            "matches_oracle": got[:len(want_cpu)] == want_cpu.tobytes(),
            "oracle_checked_blocks": sample // bs,
            "cpu_baseline": cpu_record(rates, "the buffer's first %.0f GiB (%d blocks), "
                                       "oracle_hash_chunks (Hashes::hash_file over memory); 4 "
                                       "threads = reference default --disk-threads"
                                       % (sample / GIB, sample // bs)),
            "note": "pageable host buffer -> pinned staging (host copy threads: min(12, 3/4 of "
                    "the CPU share)) -> H2D -> "
                    "k_chunks -> D2H digests, double-buffered"}


def run_config2sha(args, ca, ctx, dev, stream):
    """Config 2's blocks (1 M x 32 KiB, device-resident) hashed with
    dir-signature's second hash type, SHA-512/256 (row f4), through the
    descriptor entry point cir_hash_blocks_dev_ht."""
    import torch
    bs, nblk = args.block_size, args.blocks
    data = torch.empty(nblk * bs, dtype=torch.uint8, device=dev)
    fill_config2(ca, data, bs, stream)
    d_off = torch.arange(nblk, dtype=torch.int64, device=dev) * bs
    d_len = torch.full((nblk,), bs, dtype=torch.int32, device=dev)
    out = torch.empty(nblk * 32, dtype=torch.uint8, device=dev)

    def step():
        ctx.hash_blocks_dev(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), nblk,
                            out.data_ptr(), stream, ca.HashType.sha512_256())
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    import hashlib
    import numpy as np
    ok = all(out[32 * i:32 * i + 32].cpu().numpy().tobytes() ==
             hashlib.new("sha512_256", data[i * bs:(i + 1) * bs].cpu().numpy().tobytes()).digest()
             for i in (0, 20, nblk - 1))
    # oracle check + CPU baseline: the first 1 GiB of the arena (special
    # blocks included) through the threaded SHA-512/256 oracle
    lib = load_oracle()
    lib.oracle_sha_chunks.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_int]
    sample = min(nblk, 32768) * bs
    host = data[:sample].cpu().numpy()
    got = out[:sample // bs * 32].cpu().numpy()
    want = np.empty(sample // bs * 32, dtype=np.uint8)

    def run(threads):
        lib.oracle_sha_chunks(host.ctypes.data, sample, bs, want.ctypes.data, threads)
        return sample
    rates = cpu_rates(run, args.cpu_seconds)
    return {"metric": "GiB/s SHA-512/256 block-hashed, config 2 shape (device-resident)",
            "value": round(nblk * bs / dt / GIB, 3), "unit": "GiB/s",
            "ms_per_step": round(dt * 1e3, 3), "steps": args.steps, "blocks": nblk,
            "config": {"workload": "config2sha: %d x %d B splitmix64 blocks as SHA-512/256 "
                                   "descriptors, device-resident" % (nblk, bs)},
            "block_size": bs, "spot_check_vs_hashlib": ok,
            "matches_oracle": bool(np.array_equal(got, want)),
            "oracle_checked_blocks": sample // bs,
            "cpu_baseline": cpu_record(rates, "the first %d blocks (%.0f GiB), oracle_sha_chunks "
                                       "(SHA-512/256); 4 threads = reference default "
                                       "--disk-threads" % (sample // bs, sample / GIB))}


def make_tree(root, gib, file_mib=32, ndirs=40, seed=0x5EED0005):
    """Config 5 tree: files of file_mib MiB in ndirs directories.  A complete
    tree of this size is reused; anything else at root (a tree of another
    size, a partial one) is removed first, so the scan sees exactly nfiles."""
    import shutil
    import numpy as np
    nfiles = int(gib * 1024 // file_mib)
    done = os.path.join(root, ".complete-%d-%d" % (nfiles, file_mib))
    if os.path.exists(done):
        return nfiles
    shutil.rmtree(root, ignore_errors=True)
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 63, size=file_mib * (1 << 20) // 8, dtype=np.uint64)
    for i in range(nfiles):
        d = os.path.join(root, "d%02d" % (i % ndirs))
        os.makedirs(d, exist_ok=True)
        base[0] = i  # every file (and so every first block) differs
        base[1 + i % (base.size - 1)] ^= np.uint64(i * 0x9E3779B97F4A7C15 & ((1 << 64) - 1))
        with open(os.path.join(d, "f%05d.bin" % i), "wb") as f:
            f.write(base.tobytes())
    open(done, "w").close()
    return nfiles


def tree_read_pass(root, threads=16, piece=4 << 20):
    """One plain CPU read of every file under root (threads x pread into
    reused buffers, no GPU): (bytes, seconds)."""
    from concurrent.futures import ThreadPoolExecutor
    paths = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(root) for f in fs)
    bufs = [bytearray(piece) for _ in range(threads)]

    def work(k):
        mv, n = memoryview(bufs[k]), 0
        for p in paths[k::threads]:
            fd = os.open(p, os.O_RDONLY)
            try:
                off = 0
                while True:
                    r = os.preadv(fd, [mv], off)
                    if r <= 0:
                        break
                    off += r
                    n += r
            finally:
                os.close(fd)
        return n
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        total = sum(ex.map(work, range(threads)))
    return total, time.perf_counter() - t0


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))] if xs else None


def _merge(ivs):
    out = []
    for a, b in sorted(ivs):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def scan_batch_summary(batches, phases):
    """Config 5's per-batch phases (cir_debug_scan_batches rows of one scan)
    reduced to what bounds the scan: H2D time per batch -- split by whether
    the readers were filling a slot meanwhile -- read time, the host's wait
    for a free slot, hash + digest return, and how busy the copy engine and
    the readers were over the hash loop."""
    if not batches:
        return None
    r3 = lambda x: None if x is None else round(x, 3)  # noqa: E731

    def stats(xs):
        return {"median": r3(_pct(xs, 0.5)), "p90": r3(_pct(xs, 0.9)), "sum": r3(sum(xs))}
    h2d = [b["h2d_end_ms"] - b["h2d_start_ms"] for b in batches]
    read = [b["read_end_ms"] - b["read_start_ms"] for b in batches]
    reads = _merge([(b["read_start_ms"], b["read_end_ms"]) for b in batches])
    frac = []
    for b, h in zip(batches, h2d):
        ov = sum(max(0.0, min(b["h2d_end_ms"], e) - max(b["h2d_start_ms"], a)) for a, e in reads)
        frac.append(ov / h if h > 0 else 0.0)
    alone = [h for h, f in zip(h2d, frac) if f < 0.1]
    busy = [h for h, f in zip(h2d, frac) if f > 0.9]
    loop = phases.get("hash_loop_ms") or 0.0
    mib = [b["bytes"] / (1 << 20) for b in batches]
    return {
        "batches": len(batches), "batch_mib_median": r3(_pct(mib, 0.5)),
        "h2d_ms": stats(h2d),
        "h2d_gbs_median": r3(_pct([b["bytes"] / h / 1e6 for b, h in zip(batches, h2d) if h > 0],
                                  0.5)),
        "h2d_ms_while_reading": {"median": r3(_pct(busy, 0.5)), "batches": len(busy)},
        "h2d_ms_without_reads": {"median": r3(_pct(alone, 0.5)), "batches": len(alone)},
        "h2d_read_overlap_frac_median": r3(_pct(frac, 0.5)),
        "read_ms": stats(read),
        "read_gbs_median": r3(_pct([b["bytes"] / r / 1e6 for b, r in zip(batches, read) if r > 0],
                                   0.5)),
        "wait_ms": stats([b["wait_ms"] for b in batches]),
        "hash_d2h_ms_median": r3(_pct([b["done_ms"] - b["hash_start_ms"] for b in batches], 0.5)),
        "copy_busy_frac": r3(sum(h2d) / loop) if loop else None,
        "read_busy_frac": r3(sum(e - a for a, e in reads) / loop) if loop else None,
        "first_read_ms": r3(min(b["read_start_ms"] for b in batches)),
        "last_done_ms": r3(max(b["done_ms"] for b in batches)),
    }


def run_config5(args, ca, ctx, ctx_init_s=None):
    """value = best of the scans; value_first = the first timed scan of
    this process, which is what one `ciruela sync` sees (it scans once per
    run, src/client/sync/mod.rs:192-201) of a tree the page cache already
    holds; value_cold = one scan of the tree right after this process wrote
    it (when it did), before any other read.  A tmpfs tree that was just
    written reads ~6x slower the first time, for any reader
    (tools/first_read_probe.py: a plain 16-thread CPU read pass 16 GiB/s
    first, 100-150 after), so the cold scan measures that first touch; two
    timed CPU read passes (tree_first_read) follow it, before the timed
    scans."""
    fresh = getattr(args, "tree_fresh", None)
    if fresh is None:
        fresh = not tree_complete(args.tree_dir, args.tree_gib)
    t0 = time.perf_counter()
    nfiles = make_tree(args.tree_dir, args.tree_gib)
    gen_s = time.perf_counter() - t0
    nbytes = nfiles * 32 * (1 << 20)
    # reader threads: the library's own choice (auto_threads: min(12, 3/4 of
    # the process's CPU share)) unless CIR_SCAN_THREADS asks
    threads = int(os.environ.get("CIR_SCAN_THREADS", "0"))
    sha = getattr(args, "hash", "blake2b") == "sha512"
    cfg = ca.ScannerConfig.new().threads(threads).add_dir(args.tree_dir, "/")
    if sha:
        cfg.hash(ca.HashType.sha512_256())
    # the cold scan: the library's scan of the tree this process has just
    # written, before anything else has read it -- what `ciruela sync` right
    # after the tree was written sees (the first read of fresh tmpfs pages
    # bounds it, not PCIe: tree_first_read below)
    cold = None
    if fresh:
        ctx.scan_timing(True)
        t0 = time.perf_counter()
        got = bytearray()
        ca.v1.scan(cfg, out=got, context=ctx)
        dt = time.perf_counter() - t0
        summ = scan_batch_summary(ctx.scan_batches(), ctx.scan_phases())
        ctx.scan_timing(False)
        cold = {"seconds": round(dt, 4), "value": round(nbytes / dt / GIB, 3),
                "index": bytes(got),
                "read_gbs_median": (summ or {}).get("read_gbs_median"),
                "copy_busy_frac": (summ or {}).get("copy_busy_frac"),
                "h2d_ms_median": (summ or {}).get("h2d_ms", {}).get("median")}
        del got
    rd_bytes, rd_s = tree_read_pass(args.tree_dir)
    rd2_bytes, rd2_s = tree_read_pass(args.tree_dir)
    # footer placement: the library default (host), the GPU chain, or both
    # alternating in one process (--footer ab); every scan is timed per batch
    modes = {"host": ["host"], "gpu": ["gpu"], "ab": ["host", "gpu"]}[args.footer]
    # the index written into a growing bytearray as the scan emits it
    # (cir_scan_v1_write, as v1::scan fills the caller's Vec), or returned
    # whole (cir_scan_v1) and copied into a bytes object after the scan
    write_out = getattr(args, "scan_output", "write") == "write"
    scans = []
    index = None
    for i in range(max(1, args.steps) * len(modes)):
        mode = modes[i % len(modes)]
        ctx.set_footer_mode(ctx.FOOTER_HOST if mode == "host" else ctx.FOOTER_GPU)
        ctx.scan_timing(True)
        if write_out:  # the reference's call: v1::scan(&cfg, &mut index_buf)
            t0 = time.perf_counter()
            got = bytearray()
            ca.v1.scan(cfg, out=got, context=ctx)
            dt = time.perf_counter() - t0
        else:  # the whole index in one library buffer, copied into bytes
            t0 = time.perf_counter()
            got = ca.v1.scan(cfg, context=ctx)
            dt = time.perf_counter() - t0
        ph = ctx.scan_phases()
        summ = scan_batch_summary(ctx.scan_batches(), ph)
        ctx.scan_timing(False)
        scans.append({"footer": mode, "seconds": round(dt, 4),
                      "phases_ms": {k: round(ph[k], 3) for k in
                                    ("walk_ms", "hash_loop_ms", "last_emit_ms", "footer_tail_ms",
                                     "output_ms", "footer_busy_ms")},
                      "footer_feeds": int(ph["footer_feeds"]), "batches": summ})
        if index is not None and got != index:
            raise SystemExit("config5: two scans of the same tree differ")
        if index is None:
            index = bytes(got)
        del got
    ctx.set_footer_mode(ctx.FOOTER_HOST)
    # row f1 at full size: RawIndex::into_mut + to_raw_data of this index
    # (cir_index_rewrite: parse, rebuild the tree, re-emit, re-hash the
    # footer) must give the same bytes (the reference's roundtrip property,
    # src/cluster/download.rs:368-382)
    t0 = time.perf_counter()
    rewritten = ctx.index_rewrite(index)
    rw_s = time.perf_counter() - t0
    rewrite = {"seconds": round(rw_s, 4), "index_mb_per_s": round(len(index) / rw_s / 1e6, 1),
               "identical": rewritten == index}
    del rewritten
    times = [sc["seconds"] for sc in scans if sc["footer"] == modes[0]]
    best = min(times)
    best_scan = min((sc for sc in scans if sc["footer"] == modes[0]), key=lambda sc: sc["seconds"])
    by_mode = {m: {"seconds_best": min(sc["seconds"] for sc in scans if sc["footer"] == m),
                   "value_best": round(nbytes / min(sc["seconds"] for sc in scans
                                                   if sc["footer"] == m) / GIB, 3)}
               for m in modes}
    # checker: the whole tree indexed again by the CPU restatement (every
    # block digest, the emitter, the footer) on all cores of the GPU's share;
    # its time is the all-cores leg of the CPU baseline on the full workload
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpu_indexer
    lib = cpu_indexer.load()
    t0 = time.perf_counter()
    want = cpu_indexer.index(args.tree_dir, 32768, per_gpu_share(), lib,
                             hash_name="sha512/256" if sha else "blake2b/256")
    full_s = time.perf_counter() - t0
    # 4 threads (the reference default) on a bounded sample: directories
    # d00..d03 (a tenth of the files), indexed as their own trees
    sample = [os.path.join(args.tree_dir, "d%02d" % i) for i in range(4)]
    sample = [d for d in sample if os.path.isdir(d)]
    sample_bytes = sum(os.path.getsize(os.path.join(d, f)) for d in sample for f in os.listdir(d))

    def run(th):
        for d in sample:
            cpu_indexer.index(d, 32768, th, lib, hash_name="sha512/256" if sha else "blake2b/256")
        return sample_bytes
    if getattr(args, "no_cpu_baseline", False):
        cpu = {"skipped": "--no-cpu-baseline"}
    else:
        rates = cpu_rates(run, args.cpu_seconds)
        cpu = cpu_record(rates, "the tree's directories d00..d03 (%d files, %.2f GiB) indexed by "
                         "oracle/cpu_indexer.py (file-level pool, block_size reads, C BLAKE2b); "
                         "4 threads = reference default --disk-threads" % (
                             sum(len(os.listdir(d)) for d in sample), sample_bytes / GIB))
    cpu["full_tree"] = {"seconds": round(full_s, 3), "cores": per_gpu_share(),
                        "value": round(nbytes / full_s / GIB, 4)}
    if cold is not None:
        cold_index = cold.pop("index")
        cold["matches_oracle"] = cold_index == want
        cold["note"] = ("one scan of the tree right after this process wrote it, before any "
                        "read pass: bounded by the first read of fresh tmpfs pages "
                        "(tree_first_read), not by PCIe")
    else:
        cold = {"skipped": "the tree was left by an earlier run (not freshly written)"}
    return {"metric": "GiB/s end-to-end index of a tmpfs tree (config 5)",
            "value": round(nbytes / best / GIB, 3), "unit": "GiB/s",
            "seconds_best": round(best, 3), "seconds_all": [round(t, 3) for t in times],
            "seconds_first": round(times[0], 3),
            "value_first": round(nbytes / times[0] / GIB, 3),
            "value_cold": cold.get("value"), "cold_scan": cold,
            "context_init_s": round(ctx_init_s, 3) if ctx_init_s is not None else None,
            "config": {"workload": "config5: %d files x 32 MiB in 40 dirs (%.0f GiB) on tmpfs, "
                                   "%s (reads -> pinned -> H2D -> hash -> D2H; footer "
                                   "on %s)" % (nfiles, nbytes / GIB,
                                               "cir_scan_v1_write into a bytearray as the scan "
                                               "emits it" if write_out else
                                               "cir_scan_v1, the index copied out after the scan",
                                               "a host thread" if modes[0] == "host"
                                               else "the GPU chain")},
            "scan_output": "write" if write_out else "buffer",
            "footer": modes[0], "by_footer_mode": by_mode,
            "hash_type": "sha512/256" if sha else "blake2b/256",
            # the best scan's phases: the footer's busy time (host thread, or
            # the summed k_chain_step time for the GPU chain) and its tail
            # after the last batch, and the per-batch H2D / read / wait split
            "footer_chain_ms": best_scan["phases_ms"]["footer_busy_ms"],
            "footer_tail_ms": best_scan["phases_ms"]["footer_tail_ms"],
            "phases_best": best_scan,
            # every scan, compact (the best one in full above)
            "scans": [{"footer": sc["footer"], "seconds": sc["seconds"],
                       "hash_loop_ms": sc["phases_ms"]["hash_loop_ms"],
                       "footer_busy_ms": sc["phases_ms"]["footer_busy_ms"],
                       "footer_tail_ms": sc["phases_ms"]["footer_tail_ms"],
                       "h2d_ms_median": (sc["batches"] or {}).get("h2d_ms", {}).get("median"),
                       "h2d_ms_p90": (sc["batches"] or {}).get("h2d_ms", {}).get("p90"),
                       "copy_busy_frac": (sc["batches"] or {}).get("copy_busy_frac")}
                      for sc in scans],
            "files": nfiles, "bytes": nbytes, "index_bytes": len(index),
            "image_id": ca.get_hash(index).hex(),
            "matches_oracle": (index == want and cold.get("matches_oracle", True)
                               and rewrite["identical"]),
            "index_rewrite": rewrite,
            "tree_gen_s": round(gen_s, 1),
            "reader_threads": threads or "auto (min(12, 3/4 of the CPU share))",
            "tree": args.tree_dir,
            "tree_first_read": {"seconds": round(rd_s, 3), "value": round(rd_bytes / rd_s / GIB, 2),
                                "second_pass_value": round(rd2_bytes / rd2_s / GIB, 2),
                                "note": "plain 16-thread CPU read of the tree before the timed "
                                        "scans (no GPU): the first read after the cold scan "
                                        "(or of freshly written pages when there was none), "
                                        "then a second pass"},
            "cpu_baseline": cpu}


def make_config1_tree(root):
    """Config 1 (BASELINE.json configs[0]): 100 files, 10 MiB in total, in 10
    subdirectories, sizes and bytes from numpy default_rng(1).  Returns the
    byte total."""
    import numpy as np
    rng = np.random.default_rng(1)
    sizes = rng.integers(1, 2 * (10 << 20) // 100, size=100)
    sizes = (sizes * ((10 << 20) / sizes.sum())).astype(np.int64)
    sizes[-1] += (10 << 20) - sizes.sum()
    for i, sz in enumerate(sizes):
        d = os.path.join(root, "sub%d" % (i % 10))
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "file%03d" % i), "wb") as f:
            f.write(rng.integers(0, 256, size=int(sz), dtype=np.uint8).tobytes())
    return int(sizes.sum())


CONFIG1_ROOT = "/tmp/ciruela_cfg1_tree"


def time_cli_config1(runs=10):
    """`ciruela-index sync --append` of the config-1 tree as separate
    processes, timed from the parent's side (fork + exec + HIP start-up +
    scan + exit).  bench.py calls it before it touches a GPU itself (no
    torch.cuda call, no context yet), so each CLI process has the GPU to
    itself: the first run and the median of all `runs`."""
    import subprocess
    make_config1_tree(CONFIG1_ROOT)
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    times, out = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        out = subprocess.check_output([cli, "sync", "--append", CONFIG1_ROOT + ":/bench"])
        times.append(time.perf_counter() - t0)
    return {"seconds_first": round(times[0], 4),
            "seconds_median": round(sorted(times)[len(times) // 2], 4),
            "seconds_all": [round(t, 4) for t in times], "runs": runs,
            "image_id": out.decode().split()[0]}


def run_config1(args, ca, ctx):
    """100 files / 10 MiB, 10 subdirectories, through the `ciruela-index sync`
    CLI (the indexing half of `ciruela sync --append`, one process: HIP
    start-up included) and through v1::scan in this process (warm), checked
    against the scan oracle; CPU baseline = the CPU indexer restatement on
    the same tree.  The CLI figures are those main() took before this
    process touched the GPU (args.cli_pre), plus one run now, beside this
    process's own context, for comparison."""
    import subprocess
    root = CONFIG1_ROOT
    total = make_config1_tree(root)
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    pre = getattr(args, "cli_pre", None)
    t0 = time.perf_counter()
    out = subprocess.check_output([cli, "sync", "--append", root + ":/bench"])
    cli_s = time.perf_counter() - t0
    if isinstance(pre, dict) and "image_id" in pre and pre["image_id"] != out.decode().split()[0]:
        raise SystemExit("config1: the CLI's image id changed between runs")
    cfg = ca.ScannerConfig.new().add_dir(root, "/")  # threads(4), the reference default
    warm = []
    for _ in range(max(3, args.steps)):
        t0 = time.perf_counter()
        index = ca.v1.scan(cfg, context=ctx)
        warm.append(time.perf_counter() - t0)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpu_indexer
    import dirsig_oracle
    t0 = time.perf_counter()
    want = dirsig_oracle.scan(root)
    oracle_s = time.perf_counter() - t0
    lib = cpu_indexer.load()
    rates = cpu_rates(lambda th: (cpu_indexer.index(root, 32768, th, lib), total)[1],
                      args.cpu_seconds)
    image_id = out.decode().split()[0]
    best = min(warm)
    return {"metric": "config 1: 100-file / 10 MiB tree via `ciruela-index sync --append`",
            "value": round(total / best / GIB, 4), "unit": "GiB/s",
            "seconds_best": round(best, 5), "seconds_all": [round(t, 5) for t in warm],
            "config": {"workload": "config1: 100 files, %d bytes, 10 subdirectories" % total},
            "cli_seconds": (pre or {}).get("seconds_median", round(cli_s, 3)),
            "cli_seconds_first": (pre or {}).get("seconds_first"),
            "cli": pre if pre else {"skipped": "not measured before the bench's context"},
            "cli_seconds_beside_bench_context": round(cli_s, 3),
            "oracle_python_seconds": round(oracle_s, 3),
            "image_id": image_id,
            "matches_oracle": want.endswith(image_id.encode() + b"\n") and index == want,
            "cpu_baseline": cpu_record(rates, "the whole config-1 tree indexed by "
                                       "oracle/cpu_indexer.py (file-level pool, C BLAKE2b), "
                                       "repeated; 4 threads = reference default --disk-threads"),
            "note": "value = in-process v1::scan (warm context, threads 4); cli_seconds = the "
                    "median of `cli.runs` `ciruela-index sync` processes (HIP start-up and exit "
                    "included) timed before this process touched the GPU, cli_seconds_first the "
                    "first of them; cli_seconds_beside_bench_context = one more while this "
                    "process holds its context and torch's allocator on the same GPU"}


def mem_available_gib():
    """MemAvailable of /proc/meminfo in GiB (None if unreadable): a tmpfs
    tree lives in RAM, whatever statvfs says about the filesystem's size."""
    try:
        with open("/proc/meminfo") as f:
            for ln in f:
                if ln.startswith("MemAvailable:"):
                    return int(ln.split()[1]) / (1 << 20)
    except (OSError, ValueError, IndexError):
        pass
    return None


def tree_complete(root, gib, file_mib=32):
    return os.path.exists(os.path.join(root, ".complete-%d-%d" % (int(gib * 1024 // file_mib),
                                                                  file_mib)))


def run_config5_leg(args, ca, ctx, dev, stream):
    """Config 5 as a secondary record when the tree fits the tmpfs and the
    RAM behind it (skipped, with the reason, when it does not; a complete
    tree left by an earlier run is reused); the tree is removed afterwards."""
    import shutil
    parent = os.path.dirname(args.tree_dir.rstrip("/")) or "/"
    try:
        st = os.statvfs(parent)
        free = st.f_bavail * st.f_frsize / GIB
    except OSError as e:
        return {"skipped": "no tree filesystem: %s" % e, "matches_oracle": None}
    need = args.tree_gib * 1.05 + 4
    if not tree_complete(args.tree_dir, args.tree_gib):
        avail = mem_available_gib()
        if free < need:
            return {"skipped": "%s has %.1f GiB free, the %.0f GiB tree needs %.0f"
                               % (parent, free, args.tree_gib, need), "matches_oracle": None}
        if avail is not None and avail < need + 8:
            return {"skipped": "MemAvailable %.1f GiB, the %.0f GiB tmpfs tree needs %.0f + 8"
                               % (avail, args.tree_gib, need), "matches_oracle": None}
    args.tree_fresh = not tree_complete(args.tree_dir, args.tree_gib)
    try:
        try:
            make_tree(args.tree_dir, args.tree_gib)
        except OSError as e:  # the box's tmpfs, not the indexer: a skip, not a parity failure
            return {"skipped": "could not write the tree: %s" % e, "matches_oracle": None}
        return run_config5(args, ca, ctx)
    finally:
        shutil.rmtree(args.tree_dir, ignore_errors=True)


def run_secondary(args, ca, ctx, dev, stream):
    """The secondary BASELINE configs carried in the default N=1 line, so the
    driver's own run observes them: config 3 (mixed 4K/32K/1M descriptors,
    device-resident), config 2 from host memory (the PCIe-inclusive rate),
    config 5 (the end-to-end scan of a 50 GiB tmpfs tree, when /dev/shm holds
    it) and config 1 (the 100-file / 10 MiB tree, in process and through one
    `ciruela-index sync` process).  Each is a record of its own (value, roofline or seconds,
    cpu_baseline, matches_oracle); a failure is recorded, not raised."""
    import copy
    import traceback
    out = {}
    # config 5 first: after the other legs it ran 6 % slower than on its own
    # (profiles/r03_s2/bench_cfg5/)
    legs = (("config5", run_config5_leg, dict(steps=min(args.steps, 3))),
            ("config3", run_config3, dict(steps=min(args.steps, 10), warmup=min(args.warmup, 2))),
            ("config2host", run_config2host, dict(steps=min(args.steps, 3))),
            ("config1", lambda a, ca_, ctx_, dev_, st_: run_config1(a, ca_, ctx_),
             dict(steps=min(args.steps, 10))))
    for name, fn, over in legs:
        a = copy.copy(args)
        for k, v in over.items():
            setattr(a, k, v)
        t0 = time.perf_counter()
        try:
            out[name] = fn(a, ca, ctx, dev, stream)
        except Exception as e:  # noqa: BLE001 - reported in the line
            traceback.print_exc()
            out[name] = {"error": "%s: %s" % (type(e).__name__, e), "matches_oracle": False}
        out[name]["wall_s"] = round(time.perf_counter() - t0, 1)
        import torch
        torch.cuda.empty_cache()
    return out


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(nproc, argv):
    """`bench.py --gpus N` (N > 1) without a launcher around it: start N rank
    processes through torch.distributed.run (one per GPU, rendezvous on
    127.0.0.1) as children of this process, which has touched no GPU, and
    exit with their status.  Rank 0 writes the one JSON line to the stdout
    this process shares with it."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    log("bench: launching %d ranks: %s" % (nproc, " ".join(cmd)))
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    sys.stdout.flush()
    return subprocess.call(cmd, env=env)


def dry_run(args, rank, world):
    """The N>1 line's plumbing without a GPU: process group (gloo), shard
    plan, timed region, max-over-ranks and the job-wide parity reduction,
    one JSON line from rank 0.  Each rank's shard digests come from the
    oracle here (there is no device; this checks the bookkeeping around the
    hash, not the hash), then go through the same config4_check and
    job_summary as the GPU path; --dry-run-bad-rank R corrupts one of rank
    R's digests first."""
    import numpy as np
    import torch
    import torch.distributed as dist
    distributed = world > 1 or args.force_dist
    if distributed:
        dist.init_process_group("gloo")
    first, count = shard(rank, world, args.blocks)
    elapsed = timed_steps(lambda i: time.sleep(0.01), args.steps, lambda: None,
                          dist.barrier if distributed else None)
    elapsed_max = max_over_ranks(elapsed)
    bs = args.block_size
    oracle_lib = load_oracle()
    buf = np.empty(count * bs // 8, dtype=np.uint64)
    oracle_lib.oracle_splitmix64_fill(buf.ctypes.data, 0, buf.size, SEED_C4, bs // 8, first)
    digests = np.empty(count * 32, dtype=np.uint8)
    oracle_lib.oracle_hash_chunks(buf.ctypes.data, count * bs, bs, digests.ctypes.data, 1)
    if rank == args.dry_run_bad_rank:
        digests[32 * (count - 1)] ^= 1  # the shard's last block: a range boundary
    nbad, checked = config4_check(oracle_lib, digests, count * bs, bs, first, sample=8)
    rows = job_summary([nbad, checked, 0, 10.0 + rank, 10.0 + rank])
    parity, checked_all = job_parity(rows)
    bounds = torch.tensor([first, count], dtype=torch.int64)
    parts = [torch.zeros_like(bounds) for _ in range(world)]
    if distributed:
        dist.all_gather(parts, bounds)
    else:
        parts = [bounds]
    # no GPU here: each rank stands in its host and pid for a device (one
    # shared stand-in with --dry-run-shared-device); the rule is the one the
    # real run applies for --dist-backend
    import socket
    ident = {"pci_bus_id": "dry-run-shared" if args.dry_run_shared_device else
             "dry-run:%s:%d" % (socket.gethostname(), os.getpid()), "uuid": None}
    devices = gather_objects(ident)
    distinct, problem = devices_check(devices, args.dist_backend == "nccl")
    if problem and problem.startswith("FAIL"):
        parity = problem if parity == "ok" else parity + "; " + problem
    if rank == 0:
        print(json.dumps({
            "dry_run": True, "metric": METRIC, "n_gpus": world,
            "ranks_seen": dist.get_world_size() if distributed else 1,
            "steps": args.steps, "ms_per_step": round(elapsed_max / max(1, args.steps) * 1e3, 4),
            "config": {"workload": "config4" if distributed else "config2",
                       "blocks_per_gpu": args.blocks, "block_size": args.block_size},
            "parity": parity, "parity_checked_blocks": checked_all,
            "per_rank": [{"rank": i, "mismatches": int(r[0]), "checked": int(r[1]),
                          "kernel_ms_avg": r[3]} for i, r in enumerate(rows)],
            "devices_seen": [dict(d, rank=i) for i, d in enumerate(devices)],
            "devices_distinct": distinct, "devices_note": problem,
            "shards": [p.tolist() for p in parts]}), flush=True)
    if distributed:
        dist.destroy_process_group()
    return 0 if parity == "ok" else 1


def main():
    args = parse()
    # --gpus N > 1 (or --force-dist) with no launcher: spawn the ranks before
    # anything touches a GPU (no torch.cuda call has run in this process yet;
    # never exec)
    if (args.gpus > 1 or args.force_dist) and "WORLD_SIZE" not in os.environ:
        return launch_ranks(max(1, args.gpus), sys.argv[1:])
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        log("warning: --gpus %d but WORLD_SIZE %d; using WORLD_SIZE" % (args.gpus, world))
    if args.dump_outputs and (args.dry_run or args.workload != "auto"):
        raise SystemExit("bench: --dump-outputs writes the headline workload's digests "
                         "(not with --dry-run or --workload)")
    if args.dry_run:
        return dry_run(args, rank, world)
    # config 1's one-shot CLI, timed while no process of this job holds the
    # GPU (this process has made no GPU call yet and opens no context until
    # after it)
    if world == 1 and not args.force_dist and (
            args.workload == "config1" or (args.workload == "auto" and args.full
                                           and not args.no_secondary)):
        try:
            args.cli_pre = time_cli_config1()
        except Exception as e:  # noqa: BLE001 - reported in the config-1 record
            args.cli_pre = {"error": "%s: %s" % (type(e).__name__, e)}
    import torch
    import torch.distributed as dist

    import ciruela_amd as ca

    # one rank per GPU; more ranks than GPUs only as a rehearsal of the N>1
    # path on a small box with gloo (RCCL refuses two ranks on one GPU)
    ndev = max(1, torch.cuda.device_count())
    if world > ndev and args.dist_backend == "nccl":
        raise SystemExit("bench: %d ranks but %d visible GPU(s): one rank per GPU over RCCL; "
                         "use --dist-backend gloo for a rehearsal with shared GPUs"
                         % (world, ndev))
    ranks_per_gpu = (world + ndev - 1) // ndev if world > ndev else 1
    if ranks_per_gpu > 1:
        log("warning: %d ranks on %d GPU(s): ranks share GPUs (rehearsal, not a scaling run)"
            % (world, ndev))
    torch.cuda.set_device(local % ndev)
    dev = torch.device("cuda", local % ndev)
    distributed = world > 1 or args.force_dist
    # the process group's collectives (barrier, max-over-ranks, the job
    # summary) run on this rank's GPU for RCCL, in host memory for gloo
    coll_dev = dev if distributed and args.dist_backend == "nccl" else None
    if distributed:
        # RCCL prints its version banner on stdout when the communicator
        # comes up; keep stdout for the one JSON line (fd-level, so the C
        # library's writes go to stderr too).
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            if args.dist_backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group("gloo")
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)

    bs = args.block_size
    nblk = args.blocks
    nbytes = nblk * bs
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    # the N>1 line hashes device-resident shards only: no staging slots
    staging = ca._n.CIR_STAGING_LAZY if distributed else args.staging_mib << 20
    ctx = ca.Context(device_mask=1 << (local % ndev), staging_bytes=staging)
    ctx_init_s = time.perf_counter() - t0

    if args.workload != "auto":
        if world != 1:
            raise SystemExit("secondary workloads run on one GPU")
        rec = {"config3": lambda: run_config3(args, ca, ctx, dev, stream),
               "config5": lambda: run_config5(args, ca, ctx, ctx_init_s),
               "config1": lambda: run_config1(args, ca, ctx),
               "config2host": lambda: run_config2host(args, ca, ctx, dev, stream),
               "config2sha": lambda: run_config2sha(args, ca, ctx, dev, stream)}[args.workload]()
        print(json.dumps(rec), flush=True)
        return 0

    data = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(nblk * 32, dtype=torch.uint8, device=dev)
    if not distributed:
        workload = "config2"
        fill_config2(ca, data, bs, stream)
    else:
        workload = "config4"
        first, _ = shard(rank, world, nblk)
        ca._n.check(ca._n.lib.cir_fill_splitmix64_dev(data.data_ptr(), nbytes, SEED_C4, bs,
                                                      first, stream))
    torch.cuda.synchronize()

    lib = ca._n.lib
    if args.loader == "api":
        def step():
            ca._n.check(lib.cir_hash_chunks_dev(ctx.handle, data.data_ptr(), nbytes, bs,
                                                out.data_ptr(), stream))
    else:
        loader = 0 if args.loader == "glds" else 1

        def step():
            ca._n.check(lib.cir_debug_hash_uniform_dev(loader, data.data_ptr(), bs, nblk,
                                                       out.data_ptr(), stream))

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ref_out = out.clone() if args.full else None

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]

    def timed_step(i):
        ev[i][0].record()
        step()
        ev[i][1].record()
    elapsed = timed_steps(timed_step, args.steps, torch.cuda.synchronize,
                          dist.barrier if distributed else None)
    kern_ms = [a.elapsed_time(b) for a, b in ev]
    elapsed_max = max_over_ranks(elapsed, coll_dev)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, "digests" if world == 1 else "digests_rank%d" % rank, out)

    # parity (--full), per rank (no oracle on the config-2 path: golden digests
    # + step-to-step identity; config 4: sampled shard blocks vs the oracle),
    # then reduced over the job so the line describes every rank
    failed, reasons, nbad, checked = 0, [], 0, 0
    if args.full and not torch.equal(out, ref_out):
        failed, reasons = 1, ["digests differ between steps"]
    if args.full and workload == "config2" and nblk >= 32:
        with open(os.path.join(ROOT, "tests", "golden", "blake2b256_vectors.json")) as f:
            gold = json.load(f)["config2"]
        if bs == gold["block_size"]:
            d = out[:32 * 32].cpu().numpy().reshape(32, 32)
            want = [gold["zero_block"]] * 16 + [gold["range_block"]] * 16
            nbad = sum(d[i].tobytes().hex() != want[i] for i in range(32))
            checked = 32
            if nbad:
                reasons.append("golden config-2 blocks differ")
    if args.full and workload == "config4":
        oracle_lib = load_oracle()
        nbad, checked = config4_check(oracle_lib, out.cpu().numpy(), nbytes, bs, first)
        if nbad:
            reasons.append("sampled config-4 digests differ from the oracle")
    if nbad or failed:
        log("PARITY rank %d: %d of %d differ; %s" % (rank, nbad, checked, "; ".join(reasons)))
    rows = job_summary([nbad, checked, failed, sum(kern_ms) / len(kern_ms), min(kern_ms)],
                       coll_dev)
    parity, checked_all = job_parity(rows, "; ".join(reasons) if rank == 0 else None)
    if not args.full:
        parity = PARITY_NOT_CHECKED
    # which GPU each rank ran on, as its driver and its own clocks see it
    devices = distinct = devices_problem = None
    if distributed and args.full:
        try:  # every rank must reach the gather, whatever its probe did
            ident = device_identity(ca, local % ndev)
        except Exception as e:  # noqa: BLE001 - reported in the line
            ident = {"hip_device": local % ndev, "error": "%s: %s" % (type(e).__name__, e)}
        devices = gather_objects(ident)
        distinct, devices_problem = devices_check(devices, args.dist_backend == "nccl")
        if devices_problem and devices_problem.startswith("FAIL"):
            parity = devices_problem if parity == "ok" else parity + "; " + devices_problem
    valu_ms = valu_ceiling(ca, nblk, bs, stream) if args.full else None

    if rank == 0:
        # the roofline of the job's slowest rank: its average launch time
        slow = max(range(len(rows)), key=lambda i: rows[i][3])
        avg_kern_s = rows[slow][3] / 1e3
        algo_bytes = nbytes + 32 * nblk
        achieved = algo_bytes / avg_kern_s / 1e9
        ep = entry_point(args.loader)
        # traffic depends on the launch shape, not on the bytes' values
        cfg_key = traffic_key(bs, nblk, args.loader)
        traffic = load_traffic(cfg_key)
        cycles = load_traffic(cfg_key, "cycles")
        rec = {
            "metric": METRIC,
            "value": round(job_rate(nbytes, world, args.steps, elapsed_max), 3),
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed_max / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "config": {
                "workload": "%s: %d x %d B blocks per GPU (%.0f GiB), splitmix64, device-resident"
                            % (workload, nblk, bs, nbytes / GIB),
                "blocks_per_gpu": nblk, "block_size": bs,
                "entry_point": ep["entry_point"], "loader": ep["loader"],
                "parallelism": "range-split x%d, no collective" % world,
            },
            "roofline": {
                "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic,
                "kernel_ms_avg": round(avg_kern_s * 1e3, 4),
                "kernel_ms_min": round(min(r[4] for r in rows), 4),
                "kernel_rank": slow,
                "kernel_ms_avg_per_rank": [round(r[3], 4) for r in rows],
                # SURVEY.md 8d quotes the median of >= 10 HIP-event timed runs
                # (rank 0's launches)
                "kernel_ms_median_rank0": round(sorted(kern_ms)[len(kern_ms) // 2], 4),
                "valu_ceiling_ms": valu_ms,
                "valu_frac": round(valu_ms / (avg_kern_s * 1e3), 4) if valu_ms else None,
                # from the committed PMC pass (profiles/pmc_traffic.json): the
                # register-only compression's cycles / this kernel's, and the
                # clocks both ran at -- the gap valu_frac shows is the clock
                "cycle_frac": cycles.get("cycle_frac") if cycles else None,
                "clock_ghz": ({"kernel": cycles["clock_ghz_k_chunks"],
                               "register_only": cycles["clock_ghz_k_compress_only"]}
                              if cycles else None),
                "note": "achieved and kernel_ms_avg are the slowest rank's (kernel_rank); "
                        "binding roof is integer VALU (~2.0k VALU ops per 128-B "
                        "compression): valu_ceiling_ms = the same number of "
                        "compressions in registers with no memory traffic, timed "
                        "live; valu_frac = valu_ceiling_ms / kernel_ms_avg; cycle_frac "
                        "and clock_ghz from the committed PMC pass (the kernel issues "
                        "within 1 % of the register-only cycles; the HBM stream lowers "
                        "the clock); see DESIGN.md 4.1",
            },
            "parity": parity,
            "parity_checked_blocks": checked_all,
        }
        if distributed:
            # the process group's own count: every rank of the job took part
            rec["ranks_seen"] = dist.get_world_size()
            rec["dist_backend"] = args.dist_backend
        if devices is not None:
            rec["devices_seen"] = [dict(d, rank=i) for i, d in enumerate(devices)]
            rec["devices_distinct"] = distinct
            rec["devices_note"] = devices_problem
        if ranks_per_gpu > 1:
            rec["config"]["ranks_per_gpu"] = ranks_per_gpu
        if args.full and not distributed and not args.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(bs, args.cpu_seconds)
        if args.full and not distributed and not args.no_secondary:
            del data, out, ref_out
            torch.cuda.empty_cache()
            rec["secondary"] = run_secondary(args, ca, ctx, dev, stream)
            # a skipped leg carries matches_oracle None; a failed one False
            if any(r.get("matches_oracle", False) is False for r in rec["secondary"].values()):
                parity = "FAIL: a secondary config differs from the oracle"
                rec["parity"] = parity
        print(json.dumps(rec), flush=True)
    if distributed:
        dist.destroy_process_group()
    return 0 if parity in ("ok", PARITY_NOT_CHECKED) else 1


if __name__ == "__main__":
    sys.exit(main())
