"""Every tail length and start alignment through the per-chain loaders.

The digests are bit-exact or wrong, and what can make them wrong unnoticed is
the code that decides which bytes are message, which are padding and where
the last line ends: load_line_safe / hash_chain (k_general), the two-line
pipeline of hash_chain_prefetch (k_lane_rest), load_line_tail16 /
hash_chain_al16 (k_chunks, k_chunks_free), load32_safe / quad_run and
quad_fast (the quad kernels, k_single), load_block_padded / sha::chain
(k_sha_desc).  loader_cases.py enumerates 128 tails x 16 alignments x four
line counts over an arena without a zero byte; the reference is hashlib, and
every digest is compared.  Output buffers are prefilled with a pattern and 64
bytes longer than the digests: those stay untouched.
"""
import hashlib

import numpy as np
import pytest

import loader_cases as lc

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
EXTRA = 64


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=8 << 20)


@pytest.fixture(scope="module")
def dev_arena(gpu):
    """The named grids' arenas in device memory, uploaded once (read only)."""
    import torch
    held = {}

    def get(name):
        if name not in held:
            held[name] = torch.from_numpy(np.array(lc.named(name).arena)).to("cuda:0")
        return held[name]
    return get


def hash_type(gpu, hash_name):
    return gpu.HashType.blake2b_256() if hash_name == "blake2b" else gpu.HashType.sha512_256()


def fresh_out(nbytes):
    import torch
    out = torch.full((nbytes + EXTRA,), PATTERN, dtype=torch.uint8, device="cuda:0")
    assert out.data_ptr() % 16 == 0
    return out


def split_out(out):
    """(digest bytes, extra bytes) of a synchronised output buffer."""
    host = out.cpu().numpy()
    return host[:-EXTRA], host[-EXTRA:]


def run_desc(gpu, ctx, entry, hash_name, arena, offs, lens):
    """n x 32 digest bytes of the descriptors through one entry, and the
    extra bytes behind them."""
    import torch
    n = len(offs)
    d_off = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64))
    d_len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32))
    d_off, d_len = d_off.to("cuda:0"), d_len.to("cuda:0")
    out = fresh_out(32 * n)
    ht = hash_type(gpu, hash_name)
    if entry == "no context":
        gpu._n.check(gpu._n.lib.cir_hash_blocks_dev_ht(
            None, ht.code, arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
            out.data_ptr(), None))
    else:
        ctx.hash_blocks_dev(arena.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                            out.data_ptr(), 0, hash_type=ht)
    torch.cuda.synchronize()
    got, extra = split_out(out)
    return got.reshape(n, 32), extra


@pytest.mark.parametrize("order", lc.ORDERS)
@pytest.mark.parametrize("entry", ["no context", "context"])
@pytest.mark.parametrize("hash_name", lc.HASHES)
def test_loader_lane_grid(gpu, ctx, oracle, dev_arena, hash_name, entry, order):
    """Lengths 0..511 at every alignment (8192 descriptors), lane kernels:
    without a context k_general / hash_chain or k_sha_desc in descriptor order;
    with one k_lane_rest / hash_chain_prefetch (zero to three non-final lines)
    or k_sha_desc through the length order.  SHA-512/256: the pad block at
    positions 0..3, with (t >= 112) and without a length-only block after it."""
    g = lc.named("lane")
    idx = g.order(order)
    got, extra = run_desc(gpu, ctx, entry, hash_name, dev_arena("lane"), g.offs[idx], g.lens[idx])
    want = lc.named_reference("lane", hash_name, oracle)[idx]
    msg = lc.report(got, want, g.k[idx], g.t[idx], g.a[idx], hash_name, entry, order)
    assert msg is None, msg
    assert (extra == PATTERN).all(), "bytes behind the last digest were written"


@pytest.mark.parametrize("which", ["aligned", "all"])
def test_loader_quad_grid(gpu, ctx, dev_arena, which):
    """Lengths 1024..1535 (8 to 12 lines) with a context: quad mode in a batch
    this small.  The 512 descriptors with a == 0 alone make whole waves
    16-B aligned (quad_fast over 8 or 10 lines, skipped in the wave that holds
    k = 8, t = 0; quad_run / load32_safe for the rest of each chain); all 8192
    are ordered by length, which mixes the alignments in every wave: quad_fast
    is off and every line goes through load32_safe."""
    g = lc.named("quad")
    idx = g.where(g.a == 0) if which == "aligned" else g.order("shuffled")
    assert len(idx) == (512 if which == "aligned" else 8192)
    got, extra = run_desc(gpu, ctx, "context", "blake2b", dev_arena("quad"), g.offs[idx],
                          g.lens[idx])
    want = lc.named_reference("quad", "blake2b")[idx]
    msg = lc.report(got, want, g.k[idx], g.t[idx], g.a[idx], "blake2b", "context", which)
    assert msg is None, msg
    assert (extra == PATTERN).all(), "bytes behind the last digest were written"


def chunk_calls(ctx, data, skew, bs, nfull, rs):
    """One cir_hash_chunks_dev per r in rs over nfull * bs + r bytes at
    data + skew, all queued and synchronised once: (len(rs), nfull + 1, 32)
    digest bytes and the extra bytes behind them."""
    import torch
    per = (nfull + 1) * 32
    out = fresh_out(len(rs) * per)
    for j, r in enumerate(rs):
        ctx.hash_chunks_dev(data.data_ptr() + skew, nfull * bs + r, bs, out.data_ptr() + j * per, 0)
    torch.cuda.synchronize()
    got, extra = split_out(out)
    return got.reshape(len(rs), nfull + 1, 32), extra


def chunk_want(host, bs, nfull, rs):
    """The same by hashlib: the whole blocks' digests are those of every call."""
    mem = memoryview(host)
    whole = np.frombuffer(b"".join(lc.digest("blake2b", mem[b * bs:(b + 1) * bs])
                                   for b in range(nfull)), dtype=np.uint8).reshape(nfull, 32)
    want = np.empty((len(rs), nfull + 1, 32), dtype=np.uint8)
    want[:, :nfull] = whole
    for j, r in enumerate(rs):
        want[j, nfull] = np.frombuffer(lc.digest("blake2b", mem[nfull * bs:nfull * bs + r]),
                                       dtype=np.uint8)
    return want


@pytest.mark.parametrize("phase", ["0", "1"])
def test_loader_chunks_tail_lane_mode(gpu, ctx, dev_arena, phase, monkeypatch):
    """hash_chain_al16 / load_line_tail16: the short last block of a file of
    512-byte blocks (below 8 lines: lane mode at any block count), every
    remainder 1..511 (one to four lines), in k_chunks_free ("0") and k_chunks
    ("1"); the 65 whole blocks before it are checked in every call too."""
    monkeypatch.setenv("CIR_CHUNKS_PHASE", phase)
    bs, nfull = 512, 65
    data = dev_arena("lane")[:(nfull + 1) * bs]
    assert data.data_ptr() % 16 == 0
    rs = list(range(1, bs))
    got, extra = chunk_calls(ctx, data, 0, bs, nfull, rs)
    want = chunk_want(np.array(lc.named("lane").arena[:(nfull + 1) * bs]), bs, nfull, rs)
    tails = lc.report(got[:, nfull], want[:, nfull], [r // 128 for r in rs],
                      [r % 128 for r in rs], [0] * len(rs), "blake2b",
                      "chunks, lane tail, phase " + phase, "r = 128 k + t")
    assert tails is None, tails
    whole = lc.differing(got[:, :nfull], want[:, :nfull])
    assert whole.size == 0, "%d whole-block digests differ, first: call r = %d, block %d" % (
        whole.size, rs[whole[0] // nfull], whole[0] % nfull)
    assert (extra == PATTERN).all(), "bytes behind the last digest were written"


def test_loader_chunks_tail_quad_mode(gpu, ctx, dev_arena):
    """A one- or two-line chain inside quad_run (no descriptor batch reaches
    that shape: descriptors that short run on lanes): the short last block of
    a file of 16 blocks of 1024 bytes, every remainder 1..255, the base
    pointer 16-B aligned and skewed by 4 and by 9 bytes."""
    bs, nfull = 1024, 16
    span = (nfull + 1) * bs + 16
    data = dev_arena("quad")[:span]
    assert data.data_ptr() % 16 == 0
    host = np.array(lc.named("quad").arena[:span])
    rs = list(range(1, 256))
    skews = (0, 4, 9)
    got, want = [], []
    for skew in skews:
        g, extra = chunk_calls(ctx, data, skew, bs, nfull, rs)
        assert (extra == PATTERN).all(), "bytes behind the last digest were written"
        got.append(g)
        want.append(chunk_want(host[skew:], bs, nfull, rs))
    got, want = np.stack(got), np.stack(want)  # (skew, r, block, 32)
    tails = lc.report(got[:, :, nfull], want[:, :, nfull], [r // 128 for r in rs] * len(skews),
                      [r % 128 for r in rs] * len(skews), np.repeat(skews, len(rs)), "blake2b",
                      "chunks, quad tail", "r = 128 k + t, a = skew")
    assert tails is None, tails
    whole = lc.differing(got[:, :, :nfull], want[:, :, :nfull])
    assert whole.size == 0, "%d whole-block digests differ, first: skew %d, r = %d, block %d" % (
        whole.size, skews[whole[0] // (nfull * len(rs))], rs[whole[0] // nfull % len(rs)],
        whole[0] % nfull)


def single_report(got, want, hash_name, entry):
    n = np.arange(len(got))
    return lc.report(np.frombuffer(b"".join(got), dtype=np.uint8),
                     np.frombuffer(b"".join(want), dtype=np.uint8), n // 128, n % 128,
                     np.zeros(len(got), dtype=np.int64), hash_name, entry, "n = 128 k + t")


def test_loader_single_shot_sha512_256(gpu, oracle):
    """cir_sha512_256 on every length 0..384: prefixes of one buffer without
    a zero byte, longest first (see test_loader_single_shot_hash_bytes)."""
    buf = lc.named("lane").arena[:384].tobytes()
    got = [gpu.sha512_256(buf[:n]) for n in range(384, -1, -1)][::-1]
    want = [lc.digest("sha512", buf[:n], oracle) for n in range(385)]
    msg = single_report(got, want, "sha512", "cir_sha512_256")
    assert msg is None, msg


def test_loader_single_shot_hash_bytes(gpu):
    """BlockHash.hash_bytes (k_single / quad_single) on every length 0..1300:
    across quad_fast's threshold (8 non-final lines: 1025 bytes).  Longest
    first: the library's input buffer is reused from call to call, so what
    lies behind each input's last byte there is the previous, longer input's
    non-zero continuation, and a byte too many changes the message."""
    buf = lc.named("quad").arena[:1300].tobytes()
    got = [bytes(gpu.BlockHash.hash_bytes(buf[:n])) for n in range(1300, -1, -1)][::-1]
    want = [hashlib.blake2b(buf[:n], digest_size=32).digest() for n in range(1301)]
    msg = single_report(got, want, "blake2b", "hash_bytes")
    assert msg is None, msg
