"""cir_match_repeats_dev and cir_block_repeats on the GPU.

The kernels (ciruela_amd/csrc/repeats.hip): n digests and two optional bitmaps
in, per block the leader of its digest out (an ordinal of a pool of 2n, or
UINT32_MAX) and the count.  Inputs are torch tensors; d_match (with its count
word behind it) and the table are allocated with guard words in front of and
behind them and checked afterwards, and the table is pre-filled with values
that look like keys, since the call initialises it.  The expected value is the
Python restatement of the rule (tests/repeats_restate.py); nothing expected
comes from the library.

cir_block_repeats with a context: every family of tests/repeats_cases.py gives
output identical to ctx = NULL and to the restatement, whoever parses the
text; and two end-to-end runs on disk with the sibling calls.

Reference: fill_blocks (src/daemon/tracking/progress.rs:129-170); the
reference has no counterpart.
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import dirsig_oracle
import extents_restate
import repeats_cases
import repeats_restate
import sources_restate
from test_gpu_block_extents import Guarded, _dev, bits_of

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CASES = repeats_cases.cases()
BS = 64


@pytest.fixture(scope="module")
def T(gpu):
    return int(gpu._n.lib.cir_debug_extent_tile_blocks())


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=1 << 20)


def _words(bits, tail=False):
    return None if bits is None else sources_restate.want_words(bits, tail_ones=tail)


def _digests_dev(torch, digests):
    """The digests (a list of 32-byte strings) on the device: (tensor, ptr)."""
    if not digests:
        return None, None
    t = torch.from_numpy(np.frombuffer(b"".join(digests), dtype=np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


def run_join(gpu, digests, want=None, present=None, tail=False, seed=77, ctx=None, stream=0,
             count=True):
    """One cir_match_repeats_dev call with guards; synchronises before and
    after.  Returns (match as a numpy u32 array, count or None)."""
    import torch
    lib = gpu._n.lib
    n = len(digests)
    keep, dd = _digests_dev(torch, digests)
    tw, d_want = _dev(torch, np.frombuffer(_words(want, tail) or b"", dtype=np.uint64), np.uint64)
    tp, d_present = _dev(torch, np.frombuffer(_words(present, tail) or b"", dtype=np.uint64),
                         np.uint64)
    slots = lib.cir_match_table_slots(n)
    table = Guarded(torch, slots, 4)
    # junk that looks like keys of both classes: the call must not trust it
    junk = (torch.arange(slots, dtype=torch.int64, device="cuda") % 7).to(torch.int32)
    junk[1::2] += -(1 << 31)
    table.t[16:16 + slots] = junk
    match = Guarded(torch, n + 1, 4)
    torch.cuda.synchronize()
    d_nmatch = match.ptr + 4 * n if count else None
    if ctx is not None:
        ctx.match_repeats_dev(dd or 0, n, table.ptr, slots, seed, match.ptr, d_want=d_want or 0,
                              d_present=d_present or 0, d_nmatch=d_nmatch or 0, stream=stream)
    else:
        gpu._n.check(lib.cir_match_repeats_dev(None, dd, n, d_want, d_present, table.ptr, slots,
                                               seed, match.ptr, d_nmatch, stream))
    torch.cuda.synchronize()
    del keep, tw, tp
    assert table.guards_intact() and match.guards_intact()
    body = match.body()
    if not count:
        assert int(body[n]) == 0x5A5A5A5A
    return body[:n].copy(), int(body[n]) if count else None


def check_join(gpu, digests, want=None, present=None, **kw):
    exp = repeats_restate.expected_match(digests, want, present)
    got, count = run_join(gpu, digests, want, present, **kw)
    assert np.array_equal(got, np.array(exp, dtype=np.uint32))
    if count is not None:
        assert count == sum(1 for m in exp if m != NONE)
    return exp


# ---- cir_match_repeats_dev -----------------------------------------------------------

def test_edges(gpu):
    rng = random.Random(1)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097):
        distinct = [rng.randbytes(32) for _ in range(n)]
        equal = [distinct[0] if n else b""] * n
        exp = check_join(gpu, distinct)
        assert exp == [NONE] * n
        exp = check_join(gpu, equal)
        assert exp == ([NONE] + [n + 0] * (n - 1) if n else [])
        ones, zeros = [1] * n, [0] * n
        # want given and present NULL, want NULL and present given (ignored: all are wanted)
        assert check_join(gpu, equal, want=ones) == exp
        assert check_join(gpu, equal, present=ones) == exp
        assert check_join(gpu, equal, present=ones, count=False) == exp
        # want all zeros: nothing is wanted, whatever is present, and with tail ones
        assert check_join(gpu, equal, want=zeros, present=ones) == [NONE] * n
        assert check_join(gpu, equal, want=zeros, present=ones, tail=True) == [NONE] * n
        assert check_join(gpu, equal, want=zeros, present=zeros, tail=True) == [NONE] * n
        if n > 1:
            # only the last is wanted: it copies from present block 0, below n
            want = zeros[:-1] + [1]
            exp2 = check_join(gpu, equal, want=want, present=ones, tail=True)
            assert exp2 == [NONE] * (n - 1) + [0]


def test_pairs_across_boundaries(gpu):
    rng = random.Random(2)
    n = 300
    for a, b in ((63, 64), (255, 256), (0, n - 1)):
        d = [rng.randbytes(32) for _ in range(n)]
        d[b] = d[a]
        exp = check_join(gpu, d)
        assert exp[b] == n + a and sum(1 for m in exp if m != NONE) == 1
        # a present, b wanted: b copies from a as from a present block
        want = [1] * n
        want[a] = 0
        present = [1 - w for w in want]
        exp = check_join(gpu, d, want=want, present=present)
        assert exp[b] == a and exp[a] == NONE
        # the other way round: the later block is present and beats the earlier wanted one
        want = [1] * n
        want[b] = 0
        present = [1 - w for w in want]
        exp = check_join(gpu, d, want=want, present=present)
        assert exp[a] == b and exp[b] == NONE


def test_contention_on_one_digest(gpu):
    rng = random.Random(3)
    one = rng.randbytes(32)
    d = []
    for _ in range(20000):
        d += [one, rng.randbytes(32)]
    n = len(d)
    exp = check_join(gpu, d)
    assert exp[0] == NONE and exp[2] == n and sum(1 for m in exp if m != NONE) == 19999
    # one present holder in the middle: every wanted copy points at it, below n
    mid = 20000
    assert d[mid] == one
    want = [1] * n
    want[mid] = 0
    present = [0] * n
    present[mid] = 1
    exp = check_join(gpu, d, want=want, present=present)
    assert exp[0] == mid and exp[n - 2] == mid and exp[mid] == NONE
    assert sum(1 for m in exp if m == mid) == 19999


@pytest.fixture(scope="module")
def random_join():
    rng = random.Random(4)
    universe = [rng.randbytes(32) for _ in range(5000)]
    n = 50000 + rng.randrange(100)
    d = [rng.choice(universe) for _ in range(n)]
    want = [1 if rng.random() < 0.8 else 0 for _ in range(n)]
    present = [1 if rng.random() < 0.5 else 0 for _ in range(n)]
    return d, want, present, repeats_restate.expected_match(d, want, present)


@pytest.mark.parametrize("seed", [0, 77, (1 << 64) - 1])
def test_random(gpu, ctx, random_join, seed):
    d, want, present, exp = random_join
    got, count = run_join(gpu, d, want, present, tail=seed == 77, seed=seed,
                          ctx=ctx if seed == 0 else None)
    assert np.array_equal(got, np.array(exp, dtype=np.uint32))
    assert count == sum(1 for m in exp if m != NONE)
    n = len(d)
    assert any(m < n for m in exp) and any(n <= m < 2 * n for m in exp)


def _frame(gpu, index):
    ht, bs = ctypes.c_int(), ctypes.c_uint64()
    b0, b1 = ctypes.c_uint64(), ctypes.c_uint64()
    gpu._n.check(gpu._n.lib.cir_index_frame(index, len(index), ctypes.byref(ht), ctypes.byref(bs),
                                            ctypes.byref(b0), ctypes.byref(b1)))
    return bs.value, b0.value, b1.value


@pytest.mark.parametrize("with_ctx", [False, True])
def test_stream_order_parse_join_extents(gpu, ctx, T, with_ctx):
    """cir_index_digests_dev, cir_match_repeats_dev and cir_match_extents_dev
    queued back to back on one non-blocking stream, no synchronisation between
    them: the join reads the digests the parse writes, the extent kernels read
    the join's d_match and the parse's run table as the need table."""
    import torch
    lib = gpu._n.lib
    rng = random.Random(5)
    index = repeats_cases.random_index(rng, 200, 300, copy_rate=0.4)
    digests = repeats_restate.index_digests(index)
    n = len(digests)
    assert n > T
    want = [1 if rng.random() < 0.8 else 0 for _ in range(n)]
    present = [1 if rng.random() < 0.5 else 0 for _ in range(n)]
    runs, _ = extents_restate.runs_of_index(index)
    pool = repeats_restate.doubled(runs, n)
    match = repeats_restate.expected_match(digests, want, present)
    exp = extents_restate.expected_dev(match, runs, pool, 2 * n, BS, want)
    bs, b0, b1 = _frame(gpu, index)
    assert bs == BS
    text = torch.from_numpy(np.frombuffer(index + b"\0" * (-len(index) % 8), dtype=np.uint8)
                            .copy()).cuda()
    cap_b, cap_r = len(index) // 65, len(index) // 73
    iwb, xwb = lib.cir_index_work_bytes(len(index)), lib.cir_extents_work_bytes(n)
    slots = lib.cir_match_table_slots(n)
    dg = Guarded(torch, 4 * cap_b)            # 32 bytes per digest
    rn = Guarded(torch, 4 * cap_r)
    iwork, ires = Guarded(torch, iwb // 8), Guarded(torch, 5)
    table, dmatch = Guarded(torch, slots, 4), Guarded(torch, n + 1, 4)
    xwork, xres = Guarded(torch, xwb // 8), Guarded(torch, 6)
    fetch, ext = Guarded(torch, (n + 63) // 64), Guarded(torch, 8 * n)
    assert dg.ptr % 16 == 0
    tp, d_pool = _dev(torch, pool, np.uint64)
    tw, d_want = _dev(torch, np.frombuffer(_words(want), dtype=np.uint64), np.uint64)
    tq, d_present = _dev(torch, np.frombuffer(_words(present), dtype=np.uint64), np.uint64)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = s.cuda_stream
    if with_ctx:
        ctx.index_digests_dev(text.data_ptr(), len(index), b0, b1, bs, dg.ptr, cap_b, rn.ptr,
                              cap_r, iwork.ptr, iwb, ires.ptr, stream=st)
        ctx.match_repeats_dev(dg.ptr, n, table.ptr, slots, 9, dmatch.ptr, d_want=d_want,
                              d_present=d_present, d_nmatch=dmatch.ptr + 4 * n, stream=st)
        ctx.match_extents_dev(dmatch.ptr, n, rn.ptr, len(runs), d_pool, len(pool), 2 * n, bs,
                              xwork.ptr, xwb, xres.ptr, d_want=d_want, d_fetch=fetch.ptr,
                              d_extents=ext.ptr, cap_extents=n, stream=st)
    else:
        gpu._n.check(lib.cir_index_digests_dev(None, text.data_ptr(), len(index), b0, b1, bs,
                                               dg.ptr, cap_b, rn.ptr, cap_r, iwork.ptr, iwb,
                                               ires.ptr, st))
        gpu._n.check(lib.cir_match_repeats_dev(None, dg.ptr, n, d_want, d_present, table.ptr,
                                               slots, 9, dmatch.ptr, dmatch.ptr + 4 * n, st))
        gpu._n.check(lib.cir_match_extents_dev(None, dmatch.ptr, n, rn.ptr, len(runs), d_pool,
                                               len(pool), 2 * n, bs, d_want, None, None, None,
                                               fetch.ptr, ext.ptr, n, xwork.ptr, xwb, xres.ptr,
                                               st))
    torch.cuda.synchronize()
    for g in (dg, rn, iwork, ires, table, dmatch, xwork, xres, fetch, ext):
        assert g.guards_intact()
    assert [int(v) for v in ires.body()][:4] == [0, len(extents_restate.file_entries(index)),
                                                 len(runs), n]
    m = dmatch.body()
    assert np.array_equal(m[:n], np.array(match, dtype=np.uint32))
    assert int(m[n]) == sum(1 for v in match if v != NONE)
    res = [int(v) for v in xres.body()]
    assert res == [0] + exp["res"]
    e = ext.body()
    assert [tuple(int(v) for v in e[8 * k:8 * k + 8]) for k in range(res[5])] == exp["extents"]
    assert fetch.body().tobytes() == sources_restate.want_words(exp["fetch"])
    assert res[5] > 10 and any(x[4] == 0 for x in exp["extents"]) and \
        any(x[4] == 1 for x in exp["extents"])


# ---- cir_block_repeats with a context ---------------------------------------------------

def _file(name, digests, tail=0):
    return ("f", name, False, len(digests) * BS - tail, list(digests))


def _emit(dirs):
    return dirsig_oracle.emit("blake2b/256", BS, dirs, keep_empty=True)


def _big_case(T):
    """A few tiles of blocks with duplicated stretches laid across tile and
    wave boundaries: file a is fresh, b repeats stretches of a that start and
    end next to multiples of 64 and of T, c is b again with a short tail."""
    rng = random.Random(6)
    a = [rng.randbytes(32) for _ in range(T + 40)]
    b = [rng.randbytes(32) for _ in range(2 * T)]
    # b's block k has global number T + 40 + k
    for lo, hi, src in ((24, 88, 0), (T - 40 - 1, T - 40 + 1, 100), (2 * T - 40 - 70, 2 * T - 40 + 3, 300),
                        (1000, 1003, 1001)):
        for k in range(lo, hi):
            b[k] = a[src + k - lo]
    c = b[:T // 2] + [rng.randbytes(32)]
    new = [(b"/", [_file(b"a", a), _file(b"b", b)]), (b"/z", [_file(b"c", c, tail=9)])]
    n = len(a) + len(b) + len(c)
    want = [1 if rng.random() < 0.9 else 0 for _ in range(n)]
    present = [1 if rng.random() < 0.5 else 0 for _ in range(n)]
    index = _emit(new)
    return [("big_all", index, None, None, False), ("big_bitmaps", index, want, present, True)]


def _declined_case():
    """A directory line longer than 4096 bytes: the device declines the text,
    the host parser takes it."""
    rng = random.Random(7)
    d = [rng.randbytes(32) for _ in range(5)]
    long_dir = b"/" + b"d" * 5000
    return ("declined", _emit([(b"/", [_file(b"a", d[0:3])]),
                               (long_dir, [_file(b"b", d[0:3]), _file(b"c", d[3:5])])]),
            None, None, False)


def _parity(gpu, ctx, cases):
    for name, index, want, present, tail in cases:
        exp = repeats_restate.expected(index, want, present)
        w, p = _words(want, tail), _words(present, tail)
        dev = gpu.block_repeats(index, want=w, present=p, context=ctx)
        host = gpu.block_repeats(index, want=w, present=p)
        assert repeats_restate.same(dev, exp), name
        assert repeats_restate.same(host, exp), name
        assert dev.extents == host.extents and dev.fetch == host.fetch, name
        assert dev.stats["on_device"] == 1 and host.stats["on_device"] == 0, name
        slots = gpu._n.lib.cir_match_table_slots(dev.nblk) if dev.nblk else 0
        assert dev.stats["table_slots"] == slots and host.stats["table_slots"] == 0, name
        assert {k: v for k, v in dev.stats.items() if k not in ("table_slots", "on_device")} == \
            {k: v for k, v in host.stats.items() if k not in ("table_slots", "on_device")}, name


def test_block_repeats_parity_with_the_host_and_the_restatement(gpu, ctx, T, monkeypatch):
    import torch
    monkeypatch.delenv("CIR_SOURCES_PARSE", raising=False)
    big = _big_case(T)
    exp = repeats_restate.expected(big[0][1])
    # (b's four stretches, the first two cut where a's run of leaders ends; c: b's first half)
    assert exp[2]["repeats"] > T // 2 and len(exp[0]) >= 5
    declined = _declined_case()
    assert gpu.index_digests(declined[1], ctx).stats["fell_back"] == 1
    assert gpu.index_digests(big[0][1], ctx).stats["on_device"] == 1
    _parity(gpu, ctx, CASES + big + [declined])
    monkeypatch.setenv("CIR_SOURCES_PARSE", "host")
    _parity(gpu, ctx, CASES + big + [declined])
    assert torch.cuda.current_device() == 0


def _write(root, rel, data):
    path = os.path.join(str(root), rel)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def _write_at(root, path, off, data):
    p = os.path.join(str(root), os.fsdecode(path).lstrip("/"))
    os.makedirs(os.path.dirname(p), exist_ok=True)
    with open(p, "r+b" if os.path.exists(p) else "wb") as f:
        f.seek(off)
        f.write(data)


def _read_at(root, path, off, ln):
    with open(os.path.join(str(root), os.fsdecode(path).lstrip("/")), "rb") as f:
        f.seek(off)
        data = f.read(ln)
    assert len(data) == ln
    return data


def _fetch_blocks(out, tree, index, fetch_bytes, bs):
    """Write the fetch bitmap's blocks into `out`, here read from the files'
    contents `tree` ({relative path: bytes})."""
    g = 0
    for path, _, size, digests in extents_restate.file_entries(index):
        rel = os.fsdecode(path).lstrip("/")
        for b in range(len(digests)):
            if fetch_bytes[(g + b) >> 3] >> ((g + b) & 7) & 1:
                _write_at(out, path, b * bs, tree[rel][b * bs:(b + 1) * bs])
        g += len(digests)


def _apply(out, copies, cls):
    for dst, doff, ln, c, src, soff in copies:
        if c == cls:
            _write_at(out, dst, doff, _read_at(out, src, soff, ln))


def test_end_to_end_on_disk(gpu, ctx, tmp_path):
    """A tree with a duplicated file, a file kept under an old and a new name
    and a zero-filled file: only the fetch bitmap's blocks of
    block_repeats(index) are written into an empty directory, .copies() are
    applied, and then check_blocks is complete and check_index passes."""
    bs = 4096
    rng = random.Random(8)
    tree_dir, out = tmp_path / "tree", tmp_path / "out"
    lib = rng.randbytes(3 * bs + 100)
    tree = {"bin/tool": rng.randbytes(2 * bs + 7), "lib/libx.so": lib, "vendor/libx.so": lib,
            "data/old_name": rng.randbytes(bs + 1), "zero.img": bytes(5 * bs),
            "unique.bin": rng.randbytes(bs)}
    tree["data/new_name"] = tree["data/old_name"]
    for rel, data in tree.items():
        _write(tree_dir, rel, data)
    index = gpu.v1.scan(gpu.ScannerConfig.new().block_size(bs).add_dir(str(tree_dir)), context=ctx)
    res = gpu.block_repeats(index, context=ctx)
    exp = repeats_restate.expected(index)
    assert repeats_restate.same(res, exp)
    # libx: 4 blocks, the renamed file: 2, the zero file: 4 of its 5
    assert res.nblk == 3 + 4 + 4 + 2 + 2 + 5 + 1 and res.repeats == 10
    assert res.stats["left_to_fetch"] == res.nblk - 10 and res.stats["on_device"] == 1
    copies = list(res.copies())
    assert copies == repeats_restate.expected_copies(index, exp[0])
    assert all(c[3] == 1 for c in copies) and sum(c[2] for c in copies) == res.bytes_repeated
    os.makedirs(str(out))
    _fetch_blocks(out, tree, index, res.fetch, bs)
    assert not ctx.check_blocks(str(out), index).complete
    _apply(out, copies, 1)
    assert ctx.check_blocks(str(out), index).complete
    assert ctx.check_index(str(out), index).ok


def test_the_composed_flow(gpu, ctx, tmp_path):
    """v1 -> v2, where v2 changes a block, keeps a file and adds a new file
    twice: block_extents, the local copies, block_repeats over what is left,
    the fetch, the copies of fetched blocks; then check_blocks is complete."""
    bs = 4096
    rng = random.Random(9)
    v1, out = tmp_path / "v1", tmp_path / "out"
    old = {"app/main": rng.randbytes(4 * bs + 5), "same.txt": rng.randbytes(bs + 1)}
    for rel, data in old.items():
        _write(v1, rel, data)
    new = dict(old)
    m = bytearray(old["app/main"])
    m[bs + 3] ^= 0xFF
    new["app/main"] = bytes(m)
    fresh = rng.randbytes(2 * bs + 9)
    new["plugins/a/fresh.so"] = fresh
    new["plugins/b/fresh.so"] = fresh
    new["backup/main"] = new["app/main"]            # the changed block twice, the others local
    v2 = tmp_path / "v2"
    for rel, data in new.items():
        _write(v2, rel, data)

    def scan(root):
        return gpu.v1.scan(gpu.ScannerConfig.new().block_size(bs).add_dir(str(root)), context=ctx)
    index1, index2 = scan(v1), scan(v2)
    first = gpu.block_extents(index2, [index1], context=ctx)
    os.makedirs(str(out))
    for dst, doff, ln, s, src, soff in first.copies():
        _write_at(out, dst, doff, _read_at(v1, src, soff, ln))
    complement = bytes(~b & 0xFF for b in first.fetch)
    second = gpu.block_repeats(index2, want=first.fetch, present=complement, context=ctx)
    n = first.nblk
    fbits = bits_of(np.frombuffer(first.fetch, dtype=np.uint64), n)
    assert repeats_restate.same(second, repeats_restate.expected(index2, fbits,
                                                                 [1 - b for b in fbits]))
    # left after the local copies: the changed block twice and fresh.so twice (3 blocks each)
    assert first.stats["left_to_fetch"] == 8 and second.repeats == 4
    assert second.stats["left_to_fetch"] == 4
    assert all(s & ~f == 0 for s, f in zip(second.fetch, first.fetch))
    copies = list(second.copies())
    _apply(out, copies, 0)
    _fetch_blocks(out, new, index2, second.fetch, bs)
    _apply(out, copies, 1)
    assert ctx.check_blocks(str(out), index2).complete
    assert ctx.check_index(str(out), index2).ok


def test_cli_repeats_on_the_device(gpu, tmp_path):
    """`ciruela-index repeats` (a context) prints what `--host` prints."""
    from conftest import ROOT
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    _, index, _, _, _ = next(c for c in CASES if c[0] == "across_two_directories")
    path = str(tmp_path / "i.ds1")
    with open(path, "wb") as f:
        f.write(index)
    dev = subprocess.run([cli, "repeats", path], capture_output=True, timeout=120)
    host = subprocess.run([cli, "repeats", "--host", path], capture_output=True, timeout=120)
    assert dev.returncode == 0 and host.returncode == 0, (dev.stderr, host.stderr)
    assert dev.stdout == host.stdout
    assert dev.stdout.startswith(b"repeats: 10 blocks, 3 repeat in 1 extent(s), 192 bytes, 7 left")
