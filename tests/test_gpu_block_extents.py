"""cir_match_extents_dev and cir_block_extents on the GPU, and
cir_block_sources' device map.

The kernels (ciruela_amd/csrc/extents.hip): match[] and two run tables in,
the per-block arrays, the fetch bitmap, the counts and the extent records out.
Inputs are torch tensors; every output (and the scratch) is allocated with
guard words in front of and behind it, filled with a poison value and checked
unchanged afterwards.  The expected value is the Python restatement of the
rule (tests/extents_restate.py); nothing expected comes from the library.
T = cir_debug_extent_tile_blocks(): the shapes put extent heads and tails on
both sides of wave (64) and tile boundaries.

cir_block_extents with a context: every family of tests/extents_cases.py gives
output identical to ctx = NULL and to the restatement; cir_block_sources with
a context gives identical arrays whichever side maps (CIR_SOURCES_MAP); and one
end-to-end run with the sibling calls.

Reference: fill_blocks (src/daemon/tracking/progress.rs:129-170); the
reference has no counterpart of the extents.
"""
import os
import random

import numpy as np
import pytest

import dirsig_oracle
import extents_cases
import extents_restate
import sources_restate

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
POISON = 0x5A5A5A5A
POISON64 = 0x5A5A5A5A5A5A5A5A
GUARD = 16
BS = 4096
CASES = extents_cases.cases()


@pytest.fixture(scope="module")
def T(gpu):
    return int(gpu._n.lib.cir_debug_extent_tile_blocks())


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=1 << 20)


class Guarded:
    """n words (4 or 8 bytes) of device memory between two guards of poison;
    the body is poison too until the library writes it."""

    def __init__(self, torch, n, width=8):
        self.n, self.width = n, width
        self.dtype = np.uint64 if width == 8 else np.uint32
        self.poison = POISON64 if width == 8 else POISON
        tt = torch.int64 if width == 8 else torch.int32
        self.t = torch.full((n + 2 * GUARD,), self.poison, dtype=tt, device="cuda")
        self.ptr = self.t.data_ptr() + width * GUARD

    def body(self):
        return self.t[GUARD:GUARD + self.n].cpu().numpy().view(self.dtype)

    def guards_intact(self):
        h = self.t.cpu().numpy().view(self.dtype)
        return bool((h[:GUARD] == self.poison).all() and (h[GUARD + self.n:] == self.poison).all())

    def untouched(self):
        return bool((self.t.cpu().numpy().view(self.dtype) == self.poison).all())


def _dev(torch, values, dtype):
    """A device tensor of the values (None when empty) and its address."""
    a = np.asarray(values, dtype=dtype).reshape(-1)
    if a.size == 0:
        return None, None
    t = torch.from_numpy(a.view(np.int64 if dtype == np.uint64 else np.int32).copy()).cuda()
    return t, t.data_ptr()


def bits_of(words, n):
    return [int(words[g >> 6]) >> (g & 63) & 1 for g in range(n)]


def run_extents(gpu, match, need_runs, pool_runs, n_pool, bs=BS, want_words=None, cap=None,
                per_block=True, fetch=True, stream=0, ctx=None, join=None):
    """One cir_match_extents_dev call with guards; synchronises the device
    before and after.  join (optional): called right before the call, with
    nothing in between, to queue the join that writes d_match on `stream`;
    returns (keepalive, d_match).  Returns dict(src, file, block, fetch
    (words), extents (list of tuples, or None when none may be written), res
    (6 ints), bufs)."""
    import torch
    lib = gpu._n.lib
    n = len(match)
    nwords = (n + 63) // 64
    if cap is None:
        cap = n
    keep = []
    d_match = None
    if join is None:
        t, d_match = _dev(torch, match, np.uint32)
        keep.append(t)
    t, d_need = _dev(torch, need_runs, np.uint64)
    keep.append(t)
    t, d_pool = _dev(torch, pool_runs, np.uint64)
    keep.append(t)
    d_want = None
    if want_words is not None:
        t, d_want = _dev(torch, np.frombuffer(want_words, dtype=np.uint64), np.uint64)
        keep.append(t)
    wb = lib.cir_extents_work_bytes(n)
    bufs = dict(src=Guarded(torch, n, 4), file=Guarded(torch, n), block=Guarded(torch, n),
                fetch=Guarded(torch, nwords), extents=Guarded(torch, 8 * cap),
                res=Guarded(torch, 6), work=Guarded(torch, wb // 8))
    torch.cuda.synchronize()
    if join is not None:
        t, d_match = join()
        keep.append(t)
    pb = [bufs[k].ptr if per_block else None for k in ("src", "file", "block")]
    args = (d_match, n, d_need, len(need_runs), d_pool, len(pool_runs), n_pool, bs, d_want,
            pb[0], pb[1], pb[2], bufs["fetch"].ptr if fetch else None,
            bufs["extents"].ptr if cap else None, cap, bufs["work"].ptr, wb, bufs["res"].ptr,
            stream)
    if ctx is not None:
        ctx.match_extents_dev(args[0] or 0, n, args[2] or 0, args[3], args[4] or 0, args[5],
                              n_pool, bs, args[15], wb, args[17], d_want=d_want or 0,
                              d_src=pb[0] or 0, d_file=pb[1] or 0, d_block=pb[2] or 0,
                              d_fetch=args[12] or 0, d_extents=args[13] or 0, cap_extents=cap,
                              stream=stream)
    else:
        gpu._n.check(lib.cir_match_extents_dev(None, *args))
    torch.cuda.synchronize()
    del keep
    for name, b in bufs.items():
        assert b.guards_intact(), name
    res = [int(v) for v in bufs["res"].body()]
    out = dict(res=res, bufs=bufs)
    if per_block:
        out.update(src=bufs["src"].body(), file=bufs["file"].body(), block=bufs["block"].body())
    else:
        assert all(bufs[k].untouched() for k in ("src", "file", "block"))
    if fetch:
        out["fetch"] = bufs["fetch"].body()
    else:
        assert bufs["fetch"].untouched()
    if res[0] == 0 and res[5] <= cap:
        e = bufs["extents"].body()
        out["extents"] = [tuple(int(v) for v in e[8 * k:8 * k + 8]) for k in range(res[5])]
        assert (e[8 * res[5]:] == POISON64).all()     # nothing behind the last record
    else:
        out["extents"] = None
        assert bufs["extents"].untouched()
    return out


def check(gpu, match, need_runs, pool_runs, n_pool, bs=BS, want=None, tail_ones=False, **kw):
    """The call against the restatement; returns (result, expectation)."""
    exp = extents_restate.expected_dev(match, need_runs, pool_runs, n_pool, bs, want)
    words = None if want is None else sources_restate.want_words(want, tail_ones=tail_ones)
    got = run_extents(gpu, match, need_runs, pool_runs, n_pool, bs, want_words=words, **kw)
    cap = kw.get("cap")
    over = cap is not None and exp["res"][4] > cap
    assert got["res"] == [1 if over else 0] + exp["res"]
    if "src" in got:
        assert np.array_equal(got["src"], np.array(exp["src"], dtype=np.uint32))
        assert np.array_equal(got["file"], np.array(exp["file"], dtype=np.uint64))
        assert np.array_equal(got["block"], np.array(exp["block"], dtype=np.uint64))
    if "fetch" in got:
        assert got["fetch"].tobytes() == sources_restate.want_words(exp["fetch"])
    if over:
        assert got["extents"] is None
    else:
        assert got["extents"] == exp["extents"]
        assert sum(e[1] for e in exp["extents"]) == exp["res"][1]
        assert sum(e[7] for e in exp["extents"]) == exp["res"][2]
    return got, exp


def one_file(n, src=0, file=0, first=0, tail=0):
    """The run of one file of n blocks (the last one `tail` bytes short)."""
    return (first, n * BS - tail, file, src)


# ---- cir_match_extents_dev -----------------------------------------------------------

def test_edges(gpu, T):
    for n in (0, 1, 63, 64, 65, T - 1, T, T + 1):
        need = [one_file(n, file=3)] if n else []
        pool = [one_file(n + 2, src=1, file=7)]
        match = list(range(2, n + 2))
        got, exp = check(gpu, match, need, pool, n + 2)
        assert exp["extents"] == ([(0, n, 3, 0, 1, 7, 2, n * BS)] if n else [])
        # an empty pool: nothing is found, everything is left to fetch
        got, exp = check(gpu, [NONE] * n, need, [], 0)
        assert exp["res"] == [n, 0, 0, 0, 0] and exp["fetch"] == [1] * n
    # want: all zeros, and ones past n_need in the last word
    n = 70
    need, pool, match = [one_file(n)], [one_file(n)], list(range(n))
    got, exp = check(gpu, match, need, pool, n, want=[0] * n)
    assert exp["res"] == [0, 0, 0, 0, 0] and exp["fetch"] == [0] * n
    got, exp = check(gpu, match, need, pool, n, want=[0] * n, tail_ones=True)
    assert exp["res"] == [0, 0, 0, 0, 0] and not got["fetch"].any()
    got, exp = check(gpu, match, need, pool, n, want=[1, 0] * 35, tail_ones=True)
    assert exp["res"][4] == 35


def test_optional_outputs_null_each_alone(gpu, T):
    n = T + 9
    need, pool = [one_file(40), one_file(n - 40, file=1, first=40)], [one_file(n)]
    match = [g if g % 7 else NONE for g in range(n)]
    check(gpu, match, need, pool, n, fetch=False)
    check(gpu, match, need, pool, n, per_block=False)
    got, _ = check(gpu, match, need, pool, n, cap=0)        # d_extents NULL: counts only
    assert got["res"][0] == 1
    check(gpu, match, need, pool, n, per_block=False, fetch=False)


def test_one_extent_over_several_tiles(gpu, T):
    """The head and the tail are two tiles apart; nobody walks the extent."""
    n = 3 * T + 5
    got, exp = check(gpu, list(range(7, n + 7)), [one_file(n, tail=100)],
                     [one_file(n + 7, tail=100)], n + 7)
    assert exp["extents"] == [(0, n, 0, 0, 0, 0, 7, n * BS - 100)]


def test_extents_at_wave_and_tile_edges(gpu, T):
    n = 2 * T + 130
    ranges = [(0, 63), (128, 191), (T, 2 * T - 1), (2 * T + 1, 2 * T + 62), (2 * T + 64, n - 1)]
    match = [NONE] * n
    for a, b in ranges:
        for g in range(a, b + 1):
            match[g] = g
    got, exp = check(gpu, match, [one_file(n)], [one_file(n)], n)
    assert [(e[0], e[0] + e[1] - 1) for e in exp["extents"]] == ranges
    # single-block extents on both sides of a wave and a tile boundary
    match = [NONE] * n
    for g, j in ((63, 200), (64, 7), (T - 1, 90), (T, 33), (2 * T - 1, 1), (2 * T, 0)):
        match[g] = j
    got, exp = check(gpu, match, [one_file(n)], [one_file(n)], n)
    assert [(e[0], e[1]) for e in exp["extents"]] == [(g, 1) for g in
                                                      (63, 64, T - 1, T, 2 * T - 1, 2 * T)]


def test_every_block_its_own_extent(gpu, T):
    n = T + 70
    got, exp = check(gpu, list(range(n - 1, -1, -1)), [one_file(n)], [one_file(n)], n)
    assert exp["res"][4] == n and got["res"][5] == n


def test_must_not_merge_across_boundaries(gpu, T):
    n = 2 * T + 10
    match = list(range(n))
    for cut in (64, T, T + 64):
        # two need files whose blocks sit back to back in one source file
        need = [one_file(cut), one_file(n - cut, file=1, first=cut)]
        got, exp = check(gpu, match, need, [one_file(n)], n)
        assert [(e[0], e[1], e[2], e[6]) for e in exp["extents"]] == \
            [(0, cut, 0, 0), (cut, n - cut, 1, cut)]
        # two source files back to back in the pool matched by one need file ...
        pool = [one_file(cut, file=4), one_file(n - cut, file=5, first=cut)]
        got, exp = check(gpu, match, [one_file(n)], pool, n)
        assert [(e[0], e[1], e[5], e[6]) for e in exp["extents"]] == \
            [(0, cut, 4, 0), (cut, n - cut, 5, 0)]
        # ... and the same file ordinal in the next source
        pool = [one_file(cut, src=0, file=4), one_file(n - cut, src=1, file=4, first=cut)]
        got, exp = check(gpu, match, [one_file(n)], pool, n)
        assert [(e[0], e[4], e[5]) for e in exp["extents"]] == [(0, 0, 4), (cut, 1, 4)]
    # two need blocks that match the same pool block, across a wave boundary
    match = list(range(n))
    match[64] = 63
    got, exp = check(gpu, match, [one_file(n)], [one_file(n)], n)
    assert [(e[0], e[1]) for e in exp["extents"]] == [(0, 64), (64, 1), (65, n - 65)]


def random_tables(rng, n_need, n_pool, nsrc):
    def files(total, nsrc):
        runs, at, f, s = [], 0, 0, 0
        while at < total:
            f += rng.choice((0, 0, 1))                       # (empty files take an ordinal)
            if s + 1 < nsrc and rng.random() < 0.02:
                s, f = s + 1, 0
            nb = min(total - at, rng.choice((1, 1, 2, 5, 30, 200, 3000)))
            tail = rng.choice((0, 0, 1, 100, BS - 1))
            runs.append((at, nb * BS - tail, f, s))
            at += nb
            f += 1
        return runs
    return files(n_need, 1), files(n_pool, nsrc)


@pytest.mark.parametrize("seed,shared", [(1, 0.0), (2, 0.3), (3, 0.9), (4, 1.0)])
def test_random(gpu, seed, shared):
    rng = random.Random(seed)
    n, n_pool = 50000 + rng.randrange(200), 40000 + rng.randrange(20000)
    need, pool = random_tables(rng, n, n_pool, 3)
    match, g = [], 0
    while g < n:
        ln = min(n - g, rng.choice((1, 2, 3, 50, 700, 5000)))
        if rng.random() < shared:
            j = rng.randrange(n_pool)
            match += [min(j + k, n_pool - 1) for k in range(ln)]
        else:
            match += [rng.choice((NONE, n_pool, n_pool + 5))] * ln
        g += ln
    want = None if seed == 1 else [1 if rng.random() < 0.8 else 0 for _ in range(n)]
    got, exp = check(gpu, match, need, pool, n_pool, want=want, tail_ones=seed == 3)
    if shared:
        assert exp["res"][1] and exp["res"][3] and 1 < exp["res"][4] < exp["res"][1]


def test_capacity(gpu, T):
    rng = random.Random(5)
    n = T + 300
    need, pool = random_tables(rng, n, n, 2)
    match = [g if rng.random() < 0.9 else NONE for g in range(n)]
    exp = extents_restate.expected_dev(match, need, pool, n, BS)
    count = exp["res"][4]
    assert count > 10
    for cap in (count - 1, 0):
        got, _ = check(gpu, match, need, pool, n, cap=cap)
        assert got["res"][0] == 1 and got["res"][5] == count and got["extents"] is None
    got, _ = check(gpu, match, need, pool, n, cap=count)     # exactly enough
    assert got["res"][0] == 0 and len(got["extents"]) == count


def test_hostile_tables_stay_in_bounds(gpu, T):
    """Unsorted runs, `first` beyond n_need, sizes of 2^64 - 1, match entries
    >= n_pool: the answer is unspecified, but the call returns, no guard is
    touched, and the device answers a following ordinary call correctly."""
    rng = random.Random(6)
    n = T + 200
    M = (1 << 64) - 1
    tables = [
        ([(500, 10 * BS, 0, 0), (0, M, 1, 0), (300, BS, 2, 0)], [(900, M, 0, 1), (3, 5, M, M)]),
        ([(n + 5, BS, 0, 0), (M, M, M, M)], [(M, M, M, M), (0, M, 0, 0)]),
        ([(0, M, 0, 0)] * 5, [(0, M, 0, 0)] * 3),
    ]
    for need, pool in tables:
        for bs in (1, BS, M):
            match = [rng.choice((rng.randrange(1 << 32), rng.randrange(2 * n), NONE))
                     for _ in range(n)]
            got = run_extents(gpu, match, need, pool, n, bs=bs, cap=7)   # (guards checked inside)
            assert got["res"][0] in (0, 1) and got["res"][2] <= n
    test_one_extent_over_several_tiles(gpu, T)


def _digest_join(gpu, torch, need_d, pool_d, stream):
    """The buffers of a join, and the function that queues it on `stream`
    and returns (keepalive, d_match ptr)."""
    lib = gpu._n.lib
    dn = torch.from_numpy(np.frombuffer(b"".join(need_d), dtype=np.uint8).copy()).cuda()
    dp = torch.from_numpy(np.frombuffer(b"".join(pool_d), dtype=np.uint8).copy()).cuda()
    slots = lib.cir_match_table_slots(len(pool_d))
    table = torch.full((slots,), 0x33, dtype=torch.int32, device="cuda")
    match = torch.full((len(need_d) + 1,), POISON, dtype=torch.int32, device="cuda")

    def queue():
        gpu._n.check(lib.cir_match_digests_dev(None, dn.data_ptr(), len(need_d), dp.data_ptr(),
                                               len(pool_d), table.data_ptr(), slots, 77,
                                               match.data_ptr(),
                                               match.data_ptr() + 4 * len(need_d), stream))
        return (dn, dp, table, match), match.data_ptr()
    return queue


@pytest.mark.parametrize("with_ctx", [False, True])
def test_stream_order_behind_the_join(gpu, ctx, T, with_ctx):
    """The join and cir_match_extents_dev queued back to back on one
    non-blocking stream, no synchronisation between them."""
    import torch
    rng = random.Random(7)
    n_pool, n = T + 500, T + 100
    pool_d = [rng.randbytes(32) for _ in range(n_pool)]
    need_d = [pool_d[(g + 40) % n_pool] if g % 11 else rng.randbytes(32) for g in range(n)]
    first = {}
    for j, d in enumerate(pool_d):
        first.setdefault(d, j)
    match = [first.get(d, NONE) for d in need_d]
    need, pool = random_tables(rng, n, n_pool, 2)
    s = torch.cuda.Stream()
    exp = extents_restate.expected_dev(match, need, pool, n_pool, BS)
    got = run_extents(gpu, match, need, pool, n_pool, stream=s.cuda_stream,
                      join=_digest_join(gpu, torch, need_d, pool_d, s.cuda_stream),
                      ctx=ctx if with_ctx else None)
    assert got["res"] == [0] + exp["res"] and got["extents"] == exp["extents"]
    assert got["fetch"].tobytes() == sources_restate.want_words(exp["fetch"])
    assert np.array_equal(got["src"], np.array(exp["src"], dtype=np.uint32))


# ---- cir_block_extents / cir_block_sources with a context --------------------------------

def _big_case(T):
    """Two versions of an image of a few tiles of blocks: changed blocks, an
    append, a move, a new file."""
    rng = random.Random(8)
    bs = 64
    d = [rng.randbytes(32) for _ in range(3 * T)]
    fresh = [rng.randbytes(32) for _ in range(200)]

    def f(name, digests, tail=0):
        return ("f", name, False, len(digests) * bs - tail, list(digests))
    old = [(b"/", [f(b"a", d[:T + 30]), f(b"b", d[T + 30:2 * T], tail=5)]),
           (b"/x", [f(b"c", d[2 * T:3 * T])])]
    a2 = list(d[:T + 30])
    for k in (5, 64, T - 1, T):
        a2[k] = fresh[k % 200]
    new = [(b"/", [f(b"a", a2), f(b"b", d[T + 30:2 * T] + fresh[:7])]),
           (b"/y", [f(b"moved", d[2 * T:3 * T]), f(b"new", fresh[100:140], tail=9)])]
    emit = lambda dirs: dirsig_oracle.emit("blake2b/256", bs, dirs, keep_empty=True)
    return ("big", emit(new), [emit(old)], None, False)


def test_block_extents_parity_with_the_host_and_the_restatement(gpu, ctx, T):
    import torch
    for name, index, sources, bits, tail in CASES + [_big_case(T)]:
        want = None if bits is None else sources_restate.want_words(bits, tail_ones=tail)
        exp = extents_restate.expected(index, sources, bits)
        dev = gpu.block_extents(index, sources, want=want, context=ctx)
        host = gpu.block_extents(index, sources, want=want)
        assert extents_restate.same(dev, exp), name
        assert extents_restate.same(host, exp), name
        assert dev.extents == host.extents and dev.fetch == host.fetch, name
        assert dev.stats["on_device"] == 1 and host.stats["on_device"] == 0, name
    # (the big case: file a in four extents around its changed blocks, b and c one each)
    assert len(exp[0]) == 6 and exp[2]["found"] > 2 * T
    assert torch.cuda.current_device() == 0


def test_block_sources_maps_alike_on_either_side(gpu, ctx, T, monkeypatch):
    """cir_block_sources with a context: identical arrays and stats whether
    the host loop (CIR_SOURCES_MAP=host) or k_map_matches (=device) maps, and
    with the variable unset."""
    for name, index, sources, bits, tail in CASES + [_big_case(T)]:
        want = None if bits is None else sources_restate.want_words(bits, tail_ones=tail)
        exp = sources_restate.expected(index, sources, bits)
        got = {}
        for mode in ("host", "device", None):
            if mode is None:
                monkeypatch.delenv("CIR_SOURCES_MAP", raising=False)
            else:
                monkeypatch.setenv("CIR_SOURCES_MAP", mode)
            r = gpu.block_sources(index, sources, want=want, context=ctx)
            assert sources_restate.same(r, exp), (name, mode)
            got[mode] = (r.src, r.file, r.block, r.stats, r.skipped)
        assert got["host"] == got["device"] == got[None], name
        # and block_extents with the host loop behind the device join
        monkeypatch.setenv("CIR_SOURCES_MAP", "host")
        e = gpu.block_extents(index, sources, want=want, context=ctx)
        assert extents_restate.same(e, extents_restate.expected(index, sources, bits)), name
    monkeypatch.delenv("CIR_SOURCES_MAP", raising=False)


def test_block_sources_at_the_device_map_threshold(gpu, ctx, monkeypatch):
    """With CIR_SOURCES_MAP unset cir_block_sources maps on the device from
    16,384 needed blocks on (include/ciruela_blockhash.h) and on the host
    below: one block under, at and over the threshold give the restatement's
    and the host's arrays."""
    monkeypatch.delenv("CIR_SOURCES_MAP", raising=False)
    rng = random.Random(10)
    bs, thr = 64, 16384
    d = [rng.randbytes(32) for _ in range(thr + 1)]

    def f(name, digests, tail=0):
        return ("f", name, False, len(digests) * bs - tail, list(digests))
    def emit(files):
        return dirsig_oracle.emit("blake2b/256", bs, [(b"/", files)], keep_empty=True)
    old = emit([f(b"x", d[:9000]), f(b"y", d[9000:], tail=3)])
    for n in (thr - 1, thr, thr + 1):
        mine = list(d[:n])
        for k in (0, 63, 64, 8999, 9000, n - 1):
            mine[k] = rng.randbytes(32)
        new = emit([f(b"p", mine[:5000]), f(b"q", mine[5000:])])
        exp = sources_restate.expected(new, [old])
        dev = gpu.block_sources(new, [old], context=ctx)
        host = gpu.block_sources(new, [old])
        assert dev.nblk == n and sources_restate.same(dev, exp), n
        assert (dev.src, dev.file, dev.block) == (host.src, host.file, host.block), n
        assert exp[3]["found"] == n - 6


def _write(root, rel, data):
    path = os.path.join(str(root), rel)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def test_end_to_end_with_the_sibling_calls(gpu, ctx, tmp_path):
    """v1 -> v2 with a changed middle block, an append, a move, a new file and
    an unchanged file: exactly .copies() of block_extents(index2, [index1])
    are copied from the v1 tree into an empty directory, the fetch bitmap's
    blocks are written from v2, and then check_blocks is complete and
    check_index passes."""
    bs = 4096
    rng = random.Random(9)
    v1, v2, out = tmp_path / "v1", tmp_path / "v2", tmp_path / "out"
    files = {"changed.bin": rng.randbytes(5 * bs + 100), "log/app.log": rng.randbytes(3 * bs),
             "moved.dat": rng.randbytes(2 * bs + 7), "same.txt": rng.randbytes(bs + 1)}
    for rel, data in files.items():
        _write(v1, rel, data)
    new = dict(files)
    c = bytearray(files["changed.bin"])
    c[2 * bs + 5] ^= 0xFF                                        # a middle block changed
    new["changed.bin"] = bytes(c)
    new["log/app.log"] = files["log/app.log"] + rng.randbytes(bs + 300)   # appended to
    new["elsewhere/moved.dat"] = new.pop("moved.dat")           # moved to a new path
    new["fresh.bin"] = rng.randbytes(2 * bs + 1)                # a new file
    for rel, data in new.items():
        _write(v2, rel, data)

    def scan(root):
        return gpu.v1.scan(gpu.ScannerConfig.new().block_size(bs).add_dir(str(root)), context=ctx)
    index1, index2 = scan(v1), scan(v2)
    res = gpu.block_extents(index2, [index1], context=ctx)
    exp = extents_restate.expected(index2, [index1])
    assert extents_restate.same(res, exp)
    # changed: 2 + 3 blocks in two extents; log: 3; moved: 3; same: 2; fresh: none
    assert res.nblk == 19 and res.found == 13 and len(res.extents) == 5
    assert res.stats["left_to_fetch"] == 6
    copies = list(res.copies())
    assert copies == extents_restate.expected_copies(index2, [index1], exp[0])
    assert sum(c[2] for c in copies) == res.bytes_local
    os.makedirs(str(out))
    for dst, doff, ln, s, src, soff in copies:                   # one copy_file_range each
        assert s == 0
        with open(os.path.join(str(v1), os.fsdecode(src).lstrip("/")), "rb") as f:
            f.seek(soff)
            data = f.read(ln)
        assert len(data) == ln
        path = os.path.join(str(out), os.fsdecode(dst).lstrip("/"))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "r+b" if os.path.exists(path) else "wb") as f:
            f.seek(doff)
            f.write(data)
    blocks = ctx.check_blocks(str(out), index2)
    fetch = bits_of(np.frombuffer(res.fetch, dtype=np.uint64), res.nblk)
    assert blocks.have == sources_restate.want_words([1 - b for b in fetch])
    # the fetch bitmap's blocks, here read from v2
    g = 0
    for path, _, size, digests in extents_restate.file_entries(index2):
        rel = os.fsdecode(path).lstrip("/")
        for b in range(len(digests)):
            if fetch[g + b]:
                p = os.path.join(str(out), rel)
                os.makedirs(os.path.dirname(p), exist_ok=True)
                with open(p, "r+b" if os.path.exists(p) else "wb") as f:
                    f.seek(b * bs)
                    f.write(new[rel][b * bs:(b + 1) * bs])
        g += len(digests)
    assert ctx.check_blocks(str(out), index2).complete
    assert ctx.check_index(str(out), index2).ok


def test_cli_extents_on_the_device(gpu, tmp_path):
    """`ciruela-index sources --extents` (a context) prints what `--host`
    prints."""
    import subprocess

    from conftest import ROOT
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    _, index, sources, _, _ = next(c for c in CASES if c[0] == "one_changed_block")
    names = []
    for i, raw in enumerate([index] + list(sources)):
        names.append(str(tmp_path / ("i%d.ds1" % i)))
        with open(names[-1], "wb") as f:
            f.write(raw)
    dev = subprocess.run([cli, "sources", "--extents"] + names, capture_output=True, timeout=120)
    host = subprocess.run([cli, "sources", "--extents", "--host"] + names, capture_output=True,
                          timeout=120)
    assert dev.returncode == 0 and host.returncode == 0, (dev.stderr, host.stderr)
    assert dev.stdout == host.stdout
    assert dev.stdout.startswith(b"extents: 6 blocks, 5 found in 2 extent(s), ")
