"""cir_index_emit_dev and cir_index_memory_dev on the GPU.

The emit kernel (ciruela_amd/csrc/emit.hip): digests, a piece table and a
literal arena in device memory to the body text, one lane per 16 bytes.  Every
device call here pre-fills the body and the result word with 0xA5 and keeps a
guard region in front of and behind the body; the guards must come back
untouched and every byte of [0, round_up(body_len, 16)) written.

Expected values are the host form's (cir_index_emit_tables, cir_index_emit:
the same rule on the CPU, itself pinned to the oracle in
tests/test_index_emit_cpu.py) and the restatement's (tests/emit_restate.py),
never the device path's own.  cir_index_memory_dev is compared with the
restatement over the same bytes brought back to the host and with v1.scan of
those bytes written to a temporary directory."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emit_restate as er
from conftest import ROOT

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 256
WG_BYTES = 256 * 16  # one workgroup of k_emit_text


@pytest.fixture(scope="module")
def ctx(gpu):
    c = gpu.Context(device_mask=1)
    yield c
    c.close()


def _rng(seed):
    return np.random.default_rng(seed)


def _lit_bytes(seed, n):
    return _rng(seed).integers(0x21, 0x7f, size=n, dtype=np.uint8).tobytes()


def _digests(seed, n):
    return _rng(seed).integers(0, 256, size=32 * n, dtype=np.uint8).tobytes()


def run_dev(gpu, ctx, pieces, lits, digests, body_len, stream=0):
    """One cir_index_emit_dev call with a poisoned, guarded body; synchronises.
    pieces: [(out_off, lit_off, lit_len, first_block, nblk)].  Returns (the
    round_up(body_len, 16) body bytes, res[0])."""
    import torch
    cap = (body_len + 15) // 16 * 16
    arr = np.array(pieces, dtype=np.uint64).reshape(-1, 5)
    d_pieces = torch.from_numpy(arr.view(np.int64).reshape(-1).copy()).cuda() if len(arr) else None
    d_lits = torch.from_numpy(np.frombuffer(lits, dtype=np.uint8).copy()).cuda() if lits else None
    d_dig = torch.from_numpy(np.frombuffer(digests, dtype=np.uint8).copy()).cuda() \
        if digests else None
    buf = torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    res = torch.full((8 + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
    torch.cuda.synchronize()
    ctx.index_emit_dev(d_dig.data_ptr() if d_dig is not None else None, len(digests) // 32,
                       d_pieces.data_ptr() if d_pieces is not None else None, len(arr),
                       d_lits.data_ptr() if d_lits is not None else None, len(lits),
                       buf.data_ptr() + GUARD, body_len, res.data_ptr(), stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == POISON).all() and (host[GUARD + cap:] == POISON).all(), "guard words"
    assert (res[8:] == POISON).all().item()
    return host[GUARD:GUARD + cap].tobytes(), int(res[:8].cpu().numpy().view(np.uint64)[0])


def check_tables(gpu, ctx, pieces, lits, digests, body_len, restate=True):
    """Device == host form (== restatement) over one set of tables."""
    got = run_dev(gpu, ctx, pieces, lits, digests, body_len)
    want = gpu.index_emit_tables(np.array(pieces, dtype=np.uint64).tobytes(), lits, digests,
                                 body_len)
    assert got[1] == want[1]
    assert got[0] == want[0]
    if restate:
        assert er.body_of_tables(pieces, lits, digests, body_len) == want
    return got


def tile(shapes, lit_seed=1):
    """Consecutive pieces of the given (lit_len, nblk) shapes: (pieces, lits,
    ndigests, body_len), every piece with a literal and blocks of its own."""
    pieces, lits, off, blk = [], b"", 0, 0
    for k, (ll, nb) in enumerate(shapes):
        pieces.append((off, len(lits), ll, blk, nb))
        lits += _lit_bytes(lit_seed * 7919 + k, ll)
        off += ll + 65 * nb + 1
        blk += nb
    return pieces, lits, blk, off


# ---- the kernel against the host form -------------------------------------------------------

def test_every_alignment_of_a_token(gpu, ctx):
    """Literal lengths 1 .. 16 crossed with 0 .. 3 blocks, in two orders: a
    token is 65 bytes, an odd number, so its start meets every offset inside a
    lane's 16 bytes."""
    shapes = [(ll, nb) for ll in range(1, 17) for nb in range(4)]
    for order in (shapes, shapes[::-1], sorted(shapes, key=lambda s: (s[1], s[0]))):
        pieces, lits, nblk, body_len = tile(order)
        starts = {(p[0] + p[2]) % 16 for p in pieces if p[4]}
        assert starts == set(range(16))
        body, bad = check_tables(gpu, ctx, pieces, lits, _digests(2, nblk), body_len)
        assert bad == 0 and body[:body_len].count(b"\n") == len(pieces)


@pytest.mark.parametrize("shapes", [
    [(17, 1), (4096, 2), (33, 0), (4096, 0), (1, 1)],       # literals longer than a lane
    [(1, 0)] * 257 + [(5, 1)] + [(1, 0)] * 40,              # eight pieces inside one lane
    [(7, 0), (7, 0), (7, 0)],                               # "  a f 0\n": a lane spans three
], ids=["long_literals", "zero_block_runs", "three_in_a_lane"])
def test_piece_shapes(gpu, ctx, shapes):
    pieces, lits, nblk, body_len = tile(shapes, 3)
    _, bad = check_tables(gpu, ctx, pieces, lits, _digests(4, nblk), body_len)
    assert bad == 0


@pytest.mark.parametrize("body_len", [15, 16, 17, 31, 32, 33,
                                      WG_BYTES - 17, WG_BYTES - 16, WG_BYTES - 15, WG_BYTES - 1,
                                      WG_BYTES, WG_BYTES + 1, WG_BYTES + 15, WG_BYTES + 16,
                                      WG_BYTES + 17, 3 * WG_BYTES])
def test_body_lengths_around_lane_and_workgroup_edges(gpu, ctx, body_len):
    """Body lengths at a multiple of 16 and one either side, and one lane
    either side of a workgroup edge: the last lane pads with zero bytes and no
    lane of the last workgroup writes past the rounded length."""
    shapes, left = [], body_len
    k = 0
    while left > 0:
        nb = (k % 3) if left >= 66 * 3 + 40 else 0
        ll = min(1 + (k * 5) % 23, left - 65 * nb - 1) if left - 65 * nb - 1 >= 1 else 0
        if left - 65 * nb - 1 <= 24:
            ll = left - 65 * nb - 1
        shapes.append((ll, nb))
        left -= ll + 65 * nb + 1
        k += 1
    pieces, lits, nblk, total = tile(shapes, 5)
    assert total == body_len
    body, bad = check_tables(gpu, ctx, pieces, lits, _digests(6, nblk), body_len)
    assert bad == 0 and len(body) == (body_len + 15) // 16 * 16
    assert body[body_len:] == bytes(len(body) - body_len) and body[body_len - 1:body_len] == b"\n"


def test_empty_body_writes_nothing_but_the_result(gpu, ctx):
    body, bad = run_dev(gpu, ctx, [], b"", b"", 0)
    assert body == b"" and bad == 0


def test_a_real_list_against_index_emit(gpu, ctx):
    """Layout -> device body == the body inside cir_index_emit's index."""
    bs = 4096
    files = [(b"/a.c/z", 3 * bs + 5), (b"/a.b", bs, True), (b"/a", 0), (b"/with space/\xff", 1),
             (b"/a.c/b/c", bs - 1), (b"/d/e/f", bs + 1, True)]
    pieces, lits, _, nblk, body_len = gpu.index_emit_layout(files, bs)
    digests = _digests(7, nblk)
    index = gpu.index_emit(files, digests, bs)
    body, bad = run_dev(gpu, ctx, pieces.tolist(), lits, digests, body_len)
    assert bad == 0 and body[:body_len] == index[index.index(b"\n") + 1:-65]


def test_200000_blocks_in_3000_files(gpu, ctx):
    rng = _rng(8)
    sizes = rng.multinomial(200000 - 3000, np.ones(3000) / 3000) + 1   # blocks per file, >= 1
    bs = 512
    files = [(b"/d%02d/e%d/f%04d" % (i % 37, i % 5, i), int(n) * bs - int(rng.integers(0, bs)),
              i % 7 == 0) for i, n in enumerate(sizes)]
    pieces, lits, _, nblk, body_len = gpu.index_emit_layout(files, bs)
    assert nblk == 200000 and len(pieces) == 3000
    digests = _digests(9, nblk)
    index = gpu.index_emit(files, digests, bs)
    body, bad = run_dev(gpu, ctx, pieces.tolist(), lits, digests, body_len)
    assert bad == 0 and body[:body_len] == index[index.index(b"\n") + 1:-65]


# ---- pieces whose ranges lie outside the arrays --------------------------------------------------

def test_ranges_outside_the_arrays(gpu, ctx):
    """Such pieces yield zero bytes and the exact count; nothing is read
    through them (the arrays are exactly as long as the tables say) and the
    guard words stay."""
    shapes = [(1 + k % 16, k % 4) for k in range(300)]
    pieces, lits, nblk, body_len = tile(shapes, 10)
    digests = _digests(11, nblk)
    damaged, nbad = [], 0
    for k, (out_off, lit_off, lit_len, first, nb) in enumerate(pieces):
        how = k % 9
        if how == 1:
            lit_off = len(lits) - lit_len + 1
        elif how == 2:
            lit_len = (1 << 64) - 1 - k
        elif how == 3:
            first = nblk - nb + 1
        elif how == 4:
            nb = (1 << 63) + k
        elif how == 5:
            lit_off, first = (1 << 64) - 1, (1 << 64) - 1
        nbad += how in (1, 2, 3, 4, 5)
        damaged.append((out_off, lit_off, lit_len, first, nb))
    body, bad = check_tables(gpu, ctx, damaged, lits, digests, body_len)
    assert bad == nbad == 167
    clean, _ = gpu.index_emit_tables(np.array(pieces, dtype=np.uint64).tobytes(), lits, digests,
                                     body_len)
    for k, p in enumerate(pieces):
        end = pieces[k + 1][0] if k + 1 < len(pieces) else body_len
        want = bytes(end - p[0]) if k % 9 in (1, 2, 3, 4, 5) else clean[p[0]:end]
        assert body[p[0]:end] == want, k


def test_invalid_arguments_are_einval(gpu, ctx):
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    for args in ((None, 1, p, 0, p, 0, p, 16, p),          # digests promised, none given
                 (p, 0, p, 0, p, 0, p + 1, 16, p),         # a misaligned body
                 (p, 0, p + 4, 1, p, 0, p, 16, p),         # misaligned pieces
                 (p, 0, p, 0, p, 0, p, 16, None),          # no result word
                 (p, 0, p, 1 << 32, p, 0, p, 16, p),       # more pieces than the bisection takes
                 (p, 0, p, 0, p, 0, p, (1 << 40) + 1, p)):
        with pytest.raises(gpu.CiruelaError) as e:
            ctx.index_emit_dev(*args)
        assert e.value.status == gpu._n.CIR_EINVAL


# ---- the stream contract ------------------------------------------------------------------

class Delay:
    """A device-side delay from the library's own public path, as
    tests/test_gpu_stream_order.py makes it: cir_hash_blocks_dev without a
    context over one long chain, which one lane hashes."""

    def __init__(self, gpu, nbytes=24 << 20):
        import torch
        self.gpu = gpu
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.off = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.len = torch.full((1,), nbytes, dtype=torch.int32, device="cuda")
        self.out = torch.zeros(32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def queue(self, st):
        self.gpu._n.check(self.gpu._n.lib.cir_hash_blocks_dev(
            None, self.buf.data_ptr(), self.off.data_ptr(), self.len.data_ptr(), 1,
            self.out.data_ptr(), st.cuda_stream))


def test_emit_dev_is_ordered_on_its_stream(gpu, ctx):
    """Behind a delay on the caller's stream the digests are still poison when
    the call is made; they are written by a copy queued on that stream in front
    of it.  The call returns while the delay runs (it synchronises nothing)
    and the body is made of the real digests."""
    import torch
    shapes = [(1 + k % 16, 1 + k % 3) for k in range(2000)]
    pieces, lits, nblk, body_len = tile(shapes, 12)
    digests = _digests(13, nblk)
    want, _ = gpu.index_emit_tables(np.array(pieces, dtype=np.uint64).tobytes(), lits, digests,
                                    body_len)
    arr = np.array(pieces, dtype=np.uint64)
    d_pieces = torch.from_numpy(arr.view(np.int64).reshape(-1).copy()).cuda()
    d_lits = torch.from_numpy(np.frombuffer(lits, dtype=np.uint8).copy()).cuda()
    real = torch.from_numpy(np.frombuffer(digests, dtype=np.uint8).copy()).cuda()
    d_dig = torch.full((32 * nblk,), POISON, dtype=torch.uint8, device="cuda")
    body = torch.full((len(want) + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    res = torch.full((8,), POISON, dtype=torch.uint8, device="cuda")
    delay = Delay(gpu)
    st = torch.cuda.Stream()
    done = torch.cuda.Event()
    torch.cuda.synchronize()
    delay.queue(st)
    with torch.cuda.stream(st):
        d_dig.copy_(real, non_blocking=True)
    ctx.index_emit_dev(d_dig.data_ptr(), nblk, d_pieces.data_ptr(), len(pieces), d_lits.data_ptr(),
                       len(lits), body.data_ptr(), body_len, res.data_ptr(), st.cuda_stream)
    done.record(st)
    pending = not done.query()
    st.synchronize()
    assert pending, "delay too short: nothing was tested"
    host = body.cpu().numpy()
    assert host[:len(want)].tobytes() == want and (host[len(want):] == POISON).all()
    assert int(res.cpu().numpy().view(np.uint64)[0]) == 0


# ---- cir_index_memory_dev -----------------------------------------------------------------

def _memory_files(torch, bs, seed):
    """[(path, device tensor view, exe)] and the same bytes on the host: the
    sizes around a block, one of 1 MiB + 1, 300 one-block files, and two files
    viewed at byte offsets 1 and 8 of their allocations."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def dev(n, shift=0):
        t = torch.randint(0, 256, (n + shift,), dtype=torch.uint8, device="cuda", generator=g)
        return t[shift:]

    files = []
    for k, n in enumerate((0, 1, bs - 1, bs, bs + 1, 3 * bs + 5, (1 << 20) + 1)):
        files.append((b"/sizes/s%d" % k, dev(n), k % 2 == 1))
    rng = _rng(seed)
    for k in range(300):
        files.append((b"/many/d%d/f%03d" % (k % 7, k), dev(int(rng.integers(1, bs + 1))), False))
    files.append((b"/views/off1", dev(2 * bs + 3, 1), False))
    files.append((b"/views/off8", dev(bs + 9, 8), True))
    files.append((b"/a.c/x", dev(5), False))
    files.append((b"/a.b", dev(6), False))
    files.append((b"/a", dev(7), False))
    assert files[-5][1].data_ptr() % 16 == 1 and files[-4][1].data_ptr() % 16 == 8
    order = _rng(seed + 1).permutation(len(files))      # the caller's order is not the emission's
    files = [files[i] for i in order]
    torch.cuda.synchronize()
    host = [(p, exe, t.cpu().numpy().tobytes()) for p, t, exe in files]
    return files, host


@pytest.mark.parametrize("bs", [4096, 32768])
@pytest.mark.parametrize("hash_name", ["blake2b/256", "sha512/256"])
def test_index_memory(gpu, ctx, bs, hash_name, tmp_path, monkeypatch):
    import torch
    ht = gpu.HashType.sha512_256() if hash_name == "sha512/256" else gpu.HashType.blake2b_256()
    files, host = _memory_files(torch, bs, 20 + bs % 97)
    iid, stats = [], {}
    got = gpu.index_memory(files, bs, ht, context=ctx, image_id=iid, stats=stats)
    want = er.index_of_data(host, bs, hash_name)
    assert got == want
    assert bytes(iid[0]).hex().encode() + b"\n" == want[-65:]
    assert stats["device_emit"] == 1 and stats["files"] == len(files)
    assert stats["blocks"] == sum(-(-len(d) // bs) for _, _, d in host)
    # the only way to an index before: write the bytes out and scan them
    for p, exe, d in host:
        full = os.path.join(os.fsencode(str(tmp_path)), p[1:])
        os.makedirs(os.path.dirname(full), exist_ok=True)
        with open(full, "wb") as f:
            f.write(d)
        os.chmod(full, 0o755 if exe else 0o644)
    cfg = gpu.ScannerConfig()
    cfg.hash(ht)
    cfg.block_size(bs)
    cfg.add_dir(str(tmp_path), "/")
    scanned = gpu.v1.scan(cfg, context=ctx)
    assert got == scanned and bytes(gpu.get_hash(scanned)) == bytes(iid[0])
    # the host emitter behind the same device hash: identical bytes
    monkeypatch.setenv("CIR_EMIT", "host")
    hstats = {}
    assert gpu.index_memory(files, bs, ht, context=ctx, stats=hstats) == got
    assert hstats["device_emit"] == 0 and hstats["downloaded"] == 32 * stats["blocks"]
    monkeypatch.delenv("CIR_EMIT")
    # cir_index_rewrite of it is the identity: the emission order is the reference's
    assert ctx.index_rewrite(got) == got


def test_index_memory_without_files_and_with_empty_files(gpu, ctx):
    assert gpu.index_memory([], 4096, context=ctx) == er.index_of_data([], 4096)
    files = [(b"/e/b", (0, 0)), (b"/a", (0, 0), True)]
    assert gpu.index_memory(files, 4096, context=ctx) == \
        er.index_of_data([(b"/e/b", False, b""), (b"/a", True, b"")], 4096)


def test_index_memory_errors(gpu, ctx):
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for files in ([(b"rel", t)], [(b"/a/../b", t)], [(b"/a", t), (b"/a", t)],
                  [(b"/a", t), (b"/a/b", t)], [(b"/a", (0, 5))]):
        with pytest.raises(gpu.CiruelaError) as e:
            gpu.index_memory(files, 4096, context=ctx)
        assert e.value.status == gpu._n.CIR_EINVAL and e.value.detail
    with pytest.raises(ValueError):
        gpu.index_memory([(b"/a", torch.zeros(8, 8, dtype=torch.uint8, device="cuda")[:, :4])],
                         context=ctx)


def test_index_memory_behind_a_producer_on_its_stream(gpu, ctx):
    """The data is still being written when the call is made: a delay, then
    the kernel that fills the files, then the call, all on one stream, with
    no synchronise in between.  The buffers hold zeros until the fill runs."""
    import torch
    bs, n = 4096, 5 * 4096 + 24
    lib = gpu._n.lib
    st = torch.cuda.Stream()
    a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    b = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    ref_a, ref_b = torch.zeros_like(a), torch.zeros_like(b)
    gpu._n.check(lib.cir_fill_splitmix64_dev(ref_a.data_ptr(), n, 77, 0, 0, 0))
    gpu._n.check(lib.cir_fill_splitmix64_dev(ref_b.data_ptr(), 2 * n, 78, 0, 0, 0))
    torch.cuda.synchronize()
    host = [(b"/ckpt/a", False, ref_a.cpu().numpy().tobytes()),
            (b"/ckpt/b", False, ref_b.cpu().numpy().tobytes())]
    assert any(host[0][2]) and host[0][2] != host[1][2][:n]
    delay = Delay(gpu)
    started = torch.cuda.Event()
    delay.queue(st)
    started.record(st)
    gpu._n.check(lib.cir_fill_splitmix64_dev(a.data_ptr(), n, 77, 0, 0, st.cuda_stream))
    gpu._n.check(lib.cir_fill_splitmix64_dev(b.data_ptr(), 2 * n, 78, 0, 0, st.cuda_stream))
    assert not started.query(), "delay too short: nothing was tested"
    got = gpu.index_memory([(b"/ckpt/a", a), (b"/ckpt/b", b)], bs, context=ctx,
                           stream=st.cuda_stream)
    assert got == er.index_of_data(host, bs)


def test_exactly_one_trace_line(gpu):
    code = (
        "import torch, ciruela_amd as ca\n"
        "t = torch.arange(10000, dtype=torch.uint8, device='cuda')\n"
        "ctx = ca.Context(device_mask=1)\n"
        "idx = ca.index_memory([(b'/a', t), (b'/b/c', t[1:5000])], 4096, context=ctx)\n"
        "print(len(idx))\n")
    env = dict(os.environ, CIR_TRACE="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stderr.split(b"\n") if ln.startswith(b"cir index_memory:")]
    assert len(lines) == 1, p.stderr[-3000:]
    for lap in (b"hash", b"emit", b"download", b"footer"):
        assert lap in lines[0]
    assert b"2 files, 5 blocks, device emitter" in lines[0]
