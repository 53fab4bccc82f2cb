"""cir_sketch_digests_dev and cir_index_sketch with a context on the GPU.

The kernels (ciruela_amd/csrc/sketch.hip): n digests in, the k smallest distinct
64-bit keys out, ascending, or "declined" when the answer does not fit the
scratch.  Every device call here pre-fills the keys, the scratch and the result
words with 0xA5 and keeps a guard region behind k keys, work_bytes of scratch
and the four result words; the guards must come back untouched.

Expected values are the restatement's (tests/sketch_restate.py; its key in
numpy for the large lists, checked against the plain one) and the ctx = NULL
host path's, never the device path's own.  Digests are random bytes or made for
a chosen key by inverting the mix (tests/sketch_cases.py), so nothing is hashed.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import copies_cases
import sketch_cases
import sketch_restate
from conftest import ROOT

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
POISON = 0xA5
GUARD = 256
OK, DECLINED = 0, 1
CANDS = 8192
KS = [1, 64, 1024, 4096]
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 200000]


def keys_np(d):
    """sketch_restate.key over an (n, 32) u8 array, in numpy (u64 wraps)."""
    w = np.ascontiguousarray(d).view("<u8").reshape(-1, 4)
    x = np.full(len(w), sketch_restate.SEED, dtype=np.uint64)
    for i in range(4):
        x = (x ^ w[:, i]) * np.uint64(sketch_restate.MUL)
        x ^= x >> np.uint64(32)
    return x


def want_keys(d, k):
    keys = np.unique(keys_np(d))
    return [int(v) for v in keys[:k]], len(keys)


def as_array(digests):
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32).copy()


_RANDOM = {}


def random_array(n):
    """n random digests (seeded by n), made once and shared."""
    if n not in _RANDOM:
        a = np.random.default_rng(1000 + n).integers(0, 256, size=(n, 32), dtype=np.uint8)
        for row in a[:3]:
            assert int(keys_np(row[None, :])[0]) == sketch_restate.key(row.tobytes())
        _RANDOM[n] = a
    return _RANDOM[n]


class Poisoned:
    """nbytes of device memory filled with 0xA5 and GUARD more behind them."""

    def __init__(self, torch, nbytes):
        self.n = nbytes
        self.t = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def guard_intact(self):
        return bool((self.t[self.n:] == POISON).all().item())

    def host(self, nbytes=None):
        return self.t[:self.n if nbytes is None else nbytes].cpu().numpy()


def run_dev(gpu, d, k, ctx=None):
    """One cir_sketch_digests_dev call on the default stream over the (n, 32)
    array d, with poisoned, guarded outputs; synchronises.  Returns (res[4],
    keys up to the count, or None unless the status is OK)."""
    import torch
    lib = gpu._n.lib
    n = len(d)
    dig = torch.from_numpy(d.reshape(-1)).cuda() if n else None
    wb = lib.cir_sketch_work_bytes(n, k)
    keys, work, res = Poisoned(torch, 8 * k), Poisoned(torch, wb), Poisoned(torch, 32)
    torch.cuda.synchronize()
    args = (dig.data_ptr() if n else None, n, k, keys.ptr, work.ptr, wb, res.ptr)
    if ctx is not None:
        ctx.sketch_digests_dev(*args, stream=0)
    else:
        gpu._n.check(lib.cir_sketch_digests_dev(None, *args, 0))
    torch.cuda.synchronize()
    for o in (keys, work, res):
        assert o.guard_intact()
    r = [int(v) for v in res.host().view(np.uint64)]
    assert r[0] in (OK, DECLINED) and r[2] == n, r
    if r[0] != OK:
        return r, None
    got = keys.host().view(np.uint64)
    assert r[1] <= k and (got[r[1]:] == 0xA5A5A5A5A5A5A5A5).all()
    return r, [int(v) for v in got[:r[1]]]


def check_exact(gpu, d, k, **kw):
    """The device answers, and with the restatement's keys."""
    want, distinct = want_keys(d, k)
    r, got = run_dev(gpu, d, k, **kw)
    assert r[0] == OK, r
    assert r[1] == len(want) == min(k, distinct) and got == want
    assert r[3] <= CANDS and r[3] >= r[1] - 1      # (the key 2^64 - 1 is no candidate)
    return r


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=gpu._n.CIR_STAGING_LAZY)


# ---- the device-resident call --------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_random_digests(gpu, n, k):
    """n < k, n == k, n == k + 1, wave and workgroup edges, and 200,000: for
    random digests the device always answers."""
    r = check_exact(gpu, random_array(n), k)
    assert r[1] == min(n, k)


def test_with_a_context_argument(gpu, ctx):
    check_exact(gpu, random_array(1025), 64, ctx=ctx)


def test_one_digest_repeated(gpu):
    d = np.repeat(random_array(1)[:1], 4097, axis=0)
    for k in (1, 1024):
        r = check_exact(gpu, d, k)
        assert r[1] == 1


def test_many_blocks_share_one_digest(gpu):
    """3,000 blocks of which 2,000 share one digest: distinct < k <= n."""
    d = random_array(1025)[:1001].copy()
    d = np.concatenate([d, np.repeat(d[5:6], 1999, axis=0)])
    np.random.default_rng(2).shuffle(d)
    assert len(d) == 3000
    r = check_exact(gpu, d, 1024)
    assert r[1] == 1001


def test_every_block_twice(gpu):
    d = np.random.default_rng(3).integers(0, 256, size=(5000, 32), dtype=np.uint8)
    d = np.concatenate([d, d])
    np.random.default_rng(4).shuffle(d)
    r = check_exact(gpu, d, 4096)
    assert r[1] == 4096


@pytest.mark.parametrize("n,k", [(100, 1024), (100, 100), (100, 99), (5000, 1024), (5000, 1)])
def test_keys_zero_and_all_ones(gpu, n, k):
    """Crafted digests with the keys 0 and 2^64 - 1 among random ones: both are
    members when the rule says so -- both when n < k, the last slot when k is
    the distinct count, 0 alone when k is small."""
    rng = random.Random(n + k)
    crafted = as_array([sketch_cases.digest_with_key(x, rng) for x in (M64, 0, M64, 0)])
    d = np.concatenate([np.random.default_rng(n).integers(0, 256, size=(n - 2, 32),
                                                          dtype=np.uint8), crafted])
    np.random.default_rng(5).shuffle(d)
    want, distinct = want_keys(d, k)
    assert distinct == n and want[0] == 0
    r, got = run_dev(gpu, d, k)
    assert r[0] == OK and got == want
    assert got[0] == 0 and ((got[-1] == M64) == (k >= n))


def test_only_the_two_crafted_keys(gpu):
    rng = random.Random(6)
    d = as_array([sketch_cases.digest_with_key(M64, rng), sketch_cases.digest_with_key(0, rng)])
    assert run_dev(gpu, d, 1024) == ([OK, 2, 2, 1], [0, M64])
    assert run_dev(gpu, d[:1], 1) == ([OK, 1, 1, 0], [M64])
    assert run_dev(gpu, d, 1) == ([OK, 1, 2, 1], [0])


def test_crafted_prefix_fits(gpu):
    """5,000 distinct keys that share their top 32 bits, below 1,000 random
    ones: more candidates than k, fewer than the buffer holds -- exact."""
    d = np.concatenate([as_array(sketch_cases.prefix_digests(5000, 7)), random_array(1025)[:1000]])
    np.random.default_rng(8).shuffle(d)
    r = check_exact(gpu, d, 1024)
    assert 5000 <= r[3] <= CANDS


def test_crafted_prefix_overflows(gpu):
    """40,000 distinct keys that share their top 32 bits, all below every other
    key: OK and exact, or DECLINED, never anything else."""
    d = np.concatenate([as_array(sketch_cases.prefix_digests(40000, 9)),
                        random_array(1025)[:1000]])
    np.random.default_rng(10).shuffle(d)
    want, _ = want_keys(d, 1024)
    assert want[-1] < 1 << 32
    r, got = run_dev(gpu, d, 1024)
    assert (r[0] == OK and got == want and r[1] == 1024) or (r[0] == DECLINED and got is None), r


def test_stream_order(gpu):
    """The call on a side stream behind a long kernel: the digests are written
    on that stream behind the delay, the outputs are read back on that stream,
    and only that stream is synchronised.  A kernel on another stream, or a
    hidden synchronise, shows as garbage or as a delay that has ended when the
    call returns."""
    import torch
    lib = gpu._n.lib
    n, k = 20000, 1024
    d = np.random.default_rng(11).integers(0, 256, size=(n, 32), dtype=np.uint8)
    want, _ = want_keys(d, k)
    late = torch.from_numpy(d.reshape(-1)).pin_memory()
    dig = torch.full((32 * n,), POISON, dtype=torch.uint8, device="cuda")
    wb = lib.cir_sketch_work_bytes(n, k)
    outs = [Poisoned(torch, 8 * k), Poisoned(torch, wb), Poisoned(torch, 32)]
    pins = [torch.zeros(o.n + GUARD, dtype=torch.uint8).pin_memory() for o in (outs[0], outs[2])]
    # the delay: one BLAKE2b chain on one lane (cir_hash_blocks_dev, NULL context: one launch)
    dlen = 4 << 20
    dbuf = torch.zeros(dlen, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(1, dtype=torch.int64, device="cuda")
    dl = torch.full((1,), dlen, dtype=torch.int32, device="cuda")
    dout = torch.zeros(32, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def call():
        gpu._n.check(lib.cir_sketch_digests_dev(None, dig.data_ptr(), n, k, outs[0].ptr,
                                                outs[1].ptr, wb, outs[2].ptr, s.cuda_stream))

    def delay():
        gpu._n.check(lib.cir_hash_blocks_dev(None, dbuf.data_ptr(), doff.data_ptr(),
                                             dl.data_ptr(), 1, dout.data_ptr(), s.cuda_stream))
    with torch.cuda.stream(s):      # warm: the kernels are loaded before the timed sequence
        dig.copy_(late, non_blocking=True)
        call()
    delay()
    torch.cuda.synchronize()
    dig.fill_(POISON)
    for o in outs:
        o.t.fill_(POISON)
    torch.cuda.synchronize()
    delay()
    marker = torch.cuda.Event()
    marker.record(s)
    with torch.cuda.stream(s):
        dig.copy_(late, non_blocking=True)
        call()
        pending = not marker.query()
        pins[0].copy_(outs[0].t, non_blocking=True)
        pins[1].copy_(outs[2].t, non_blocking=True)
    s.synchronize()
    try:
        assert pending, "delay too short: nothing was tested"
        r = [int(v) for v in pins[1][:32].numpy().view(np.uint64)]
        assert r[:3] == [OK, k, n]
        assert [int(v) for v in pins[0][:8 * k].numpy().view(np.uint64)] == want
        for o, p in zip((outs[0], outs[2]), pins):
            assert (p[o.n:].numpy() == POISON).all()
        assert outs[1].guard_intact()
    finally:
        torch.cuda.synchronize()


# ---- the host-memory call with a context -------------------------------------------------

def golden_index():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "dirsig_v1_example.json")) as f:
        return json.load(f)["index"].encode()


def both_paths(gpu, ctx, index, k):
    """(blob with the context, its stats, blob with ctx = NULL)."""
    st = {}
    dev = gpu.index_sketch(index, ctx, k, stats=st)
    return dev, st, gpu.index_sketch(index, None, k)


@pytest.mark.parametrize("k", [64, 1024])
def test_index_sketch_on_the_cpu_files_indexes(gpu, ctx, k):
    for name, index in [("golden", golden_index())] + sketch_cases.cpu_indexes(64):
        dev, st, host = both_paths(gpu, ctx, index, k)
        assert dev == host == sketch_restate.sketch(index, k), name
        _, _, blocks = sketch_restate.index_blocks(index)
        assert st["on_device"] == 1 and st["why_host"] == 0, (name, st)
        assert st["blocks"] == len(blocks) and st["keys"] == (len(dev) - 40) // 8
        assert st["uploaded"] == len(index) and st["downloaded"] <= 8 * k + 8 * (5 + 4)


def test_index_sketch_on_random_indexes(gpu, ctx):
    answered = 0
    for seed in range(20):
        index, _, _ = copies_cases.random_case(seed)
        dev, st, host = both_paths(gpu, ctx, index, 64)
        assert dev == host == sketch_restate.sketch(index, 64), seed
        assert st["on_device"] == 1 and st["downloaded"] <= 8 * 64 + 72, (seed, st)
        answered += st["blocks"] > 0
    assert answered >= 10


def test_index_sketch_crafted_prefix(gpu, ctx):
    """The crafted index through the public call: the same blob as ctx = NULL
    whichever path answered, and the stats name the path."""
    digests = sketch_cases.prefix_digests(40000, 9) + sketch_cases.random_digests(1000, 12)
    random.Random(13).shuffle(digests)
    index = sketch_cases.index_of(digests)
    dev, st, host = both_paths(gpu, ctx, index, 1024)
    want, _ = want_keys(as_array(digests), 1024)
    assert dev == host == sketch_restate.blob(1, 1024, 64, 41000, want)
    assert (st["on_device"], st["why_host"]) in ((1, 0), (0, gpu._n.CIR_SKETCH_WHY_DECLINED)), st
    assert st["uploaded"] == len(index) and st["blocks"] == 41000 and st["keys"] == 1024
    # and the crafted keys 0 and 2^64 - 1 through the public call
    rng = random.Random(14)
    d = [sketch_cases.digest_with_key(x, rng) for x in (M64, 0)] + \
        sketch_cases.random_digests(30, 15)
    index = sketch_cases.index_of(d)
    dev, st, host = both_paths(gpu, ctx, index, 64)
    assert dev == host == sketch_restate.sketch(index, 64) and st["on_device"] == 1
    assert sketch_restate.parse(dev)[4][0] == 0 and sketch_restate.parse(dev)[4][-1] == M64


def test_index_sketch_falls_back_for_a_declined_text(gpu, ctx):
    """Two spaces between tokens: the device parse declines, the host rule
    answers, and the blob is the canonical text's."""
    index = sketch_cases.index_of(sketch_cases.random_digests(200, 16))
    at = index.index(b" f ")
    lenient = index[:at] + b" " + index[at:]
    dev, st, host = both_paths(gpu, ctx, lenient, 64)
    assert dev == host == sketch_restate.sketch(index, 64)
    assert (st["on_device"], st["why_host"]) == (0, gpu._n.CIR_SKETCH_WHY_TEXT)
    assert st["uploaded"] == len(lenient) and st["blocks"] == 200
    # errors are the host parser's, with a context as without
    for broken, code in ((index.replace(b" f ", b" q ", 1), gpu._n.CIR_EPARSE),
                         (index[:-1], gpu._n.CIR_EPARSE)):
        for c in (ctx, None):
            with pytest.raises(gpu.CiruelaError) as e:
                gpu.index_sketch(broken, c, 64)
            assert e.value.status == code


def test_index_sketch_multi_tile_text(gpu, ctx):
    """A text of several tiles of the parse (cir_debug_index_tile_bytes), so
    that its tiling sits in front of the sketch."""
    tile = int(gpu._n.lib.cir_debug_index_tile_bytes())
    digests = sketch_cases.random_digests(3000, 17)
    digests += digests[:500]
    index = sketch_cases.index_of(digests, per_file=177)
    assert len(index) > 40 * tile
    for k in (1024, 4096):
        dev, st, host = both_paths(gpu, ctx, index, k)
        assert dev == host == sketch_restate.sketch(index, k)
        assert st["on_device"] == 1 and st["blocks"] == 3500 and st["keys"] == min(k, 3000)


_TRACED_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import ciruela_amd as ca
import sketch_cases
index = sketch_cases.index_of(sketch_cases.random_digests(2000, 18))
ctx = ca.Context(device_mask=1, staging_bytes=ca._n.CIR_STAGING_LAZY)
st = {}
blob = ca.index_sketch(index, ctx, 256, stats=st)
sys.stdout.write("%d %d %d %s\n" % (st["on_device"], st["why_host"], len(blob), blob.hex()))
"""


def test_trace_line_and_the_host_switch(gpu):
    """A child process under CIR_TRACE=1: one `cir index_sketch:` line with the
    device's laps and none of a sibling call's; under CIR_SKETCH=host the host
    line, and the same blob."""
    outs = {}
    for mode in ("", "host"):
        env = dict(os.environ, CIR_TRACE="1", CIR_SKETCH=mode)
        p = subprocess.run([sys.executable, "-c", _TRACED_CHILD, ROOT], env=env,
                           capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("cir ")]
        mine = [ln for ln in lines if ln.startswith("cir index_sketch:")]
        assert len(mine) == 1, lines
        assert not [ln for ln in lines if ln.split(":")[0] in (
            "cir block_sources", "cir block_repeats", "cir file_sources", "cir file_copies",
            "cir fetch_plan", "cir check_blocks")], lines
        outs[mode] = (p.stdout.split(), mine[0])
    assert outs[""][0][:3] == [b"1", b"0", b"%d" % (40 + 8 * 256)]
    assert outs["host"][0][:3] == [b"0", b"%d" % gpu._n.CIR_SKETCH_WHY_ENV, b"%d" % (40 + 8 * 256)]
    assert outs[""][0][3] == outs["host"][0][3]
    assert ", device;" in outs[""][1] and "sketch kernels" in outs[""][1]
    assert "host (why 1)" in outs["host"][1]


def test_cli_on_the_device_equals_host(gpu, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    base = sketch_cases.random_digests(600, 19)
    texts = [sketch_cases.index_of(base)] + \
        [sketch_cases.index_of(base[:n] + sketch_cases.random_digests(600 - n, 50 + n))
         for n in (60, 540, 300)]
    paths = []
    for i, t in enumerate(texts):
        (tmp_path / ("i%d.ds1" % i)).write_bytes(t)
        paths.append(str(tmp_path / ("i%d.ds1" % i)))
    got = {}
    for flags in ([], ["--host"]):
        p = subprocess.run([cli, "sketch", paths[0], "-k", "256"] + flags, capture_output=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert (b"sketched on the host" in p.stderr) == bool(flags)
        assert (b"sketched on the device" in p.stderr) == (not flags)
        q = subprocess.run([cli, "rank"] + paths + ["-k", "256"] + flags, capture_output=True,
                           timeout=120)
        assert q.returncode == 0, q.stderr[-2000:]
        got[bool(flags)] = (p.stdout, q.stdout)
    assert got[False] == got[True]
    assert got[True][0] == sketch_restate.sketch(texts[0], 256)
    assert [ln.split()[0] for ln in got[True][1].splitlines()] == [b"1", b"2", b"0"]
