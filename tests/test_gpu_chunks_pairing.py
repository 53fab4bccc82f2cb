"""k_chunks with phase-aligned workgroups: every digest equals
hashlib.blake2b(digest_size=32).

k_chunks runs 512-thread workgroups whose eight waves meet at a barrier in
front of every fast group of the compression, so a wave that has no blocks
still runs the line loop (on a duplicate of the file's last whole block,
storing nothing).  Blocks of less than 1 KiB always take k_chunks, so the
small cases use 128-B and 512-B blocks at the counts around the wave (64),
the former workgroup (256), the workgroup (512) and its multiples: workgroups
that mix full, partial and empty waves, each count whole, with a 1-byte tail
and with a tail of bs - 1 bytes (the fused ragged workgroup).  One larger
case, 49,153 blocks of 1 KiB, is the smallest count at which blocks of 1 KiB
and more reach k_chunks.

The library routes only batches of whole two-wave layers to the phase-aligned
kernel (kernels.hip chunks_phase_aligned) and the rest to the free-running
k_chunks_free, so every case runs twice: as routed, and with
CIR_CHUNKS_PHASE=1, which sends it through the barriers.
"""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL_BS = (128, 512)
SMALL_NBLK = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
BIG_BS, BIG_NBLK = 1024, 49153
GUARD = 4096  # bytes behind the digests that no wave may write


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=8 << 20)


def digest(b):
    return hashlib.blake2b(b, digest_size=32).digest()


class Source:
    """Device bytes (seeded), their host copy, and the whole-block digests of
    the prefix for one block size, computed once."""

    def __init__(self, gpu, nbytes, seed):
        import torch
        n = (nbytes + 64 + 7) // 8 * 8
        self.dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        gpu._n.check(gpu._n.lib.cir_fill_splitmix64_dev(self.dev.data_ptr(), n, seed, 0, 0, 0))
        torch.cuda.synchronize()
        self.host = self.dev.cpu().numpy().tobytes()
        self.whole = {}

    def reference(self, bs, nfull):
        have = self.whole.setdefault(bs, [])
        for i in range(len(have), nfull):
            have.append(digest(self.host[i * bs:(i + 1) * bs]))
        return b"".join(have[:nfull])


@pytest.fixture(scope="module")
def small(gpu):
    return Source(gpu, max(SMALL_BS) * (max(SMALL_NBLK) + 1), 0x9A121)


@pytest.fixture(scope="module")
def big(gpu):
    return Source(gpu, BIG_BS * (BIG_NBLK + 1), 0x9A122)


@pytest.fixture(params=["routed", "phase"])
def mode(request):
    """The library reads CIR_CHUNKS_PHASE at every call."""
    old = os.environ.pop("CIR_CHUNKS_PHASE", None)
    if request.param == "phase":
        os.environ["CIR_CHUNKS_PHASE"] = "1"
    yield request.param
    os.environ.pop("CIR_CHUNKS_PHASE", None)
    if old is not None:
        os.environ["CIR_CHUNKS_PHASE"] = old


def check(ctx, src, bs, nfull, tail):
    import torch
    nbytes = nfull * bs + tail
    nblk = nfull + (1 if tail else 0)
    out = torch.full((nblk * 32 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ctx.hash_chunks_dev(src.dev.data_ptr(), nbytes, bs, out.data_ptr(), 0)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = src.reference(bs, nfull)
    if tail:
        want += digest(src.host[nfull * bs:nbytes])
    want = np.frombuffer(want, dtype=np.uint8)
    bad = (got[:nblk * 32].reshape(-1, 32) != want.reshape(-1, 32)).any(1)
    assert not bad.any(), (bs, nfull, tail, int(np.nonzero(bad)[0][0]), int(bad.sum()))
    assert (got[nblk * 32:] == 0xA5).all(), (bs, nfull, tail, "wrote past the digests")


def tail_of(kind, bs):
    return {"whole": 0, "tail1": 1, "tailmax": bs - 1}[kind]


@pytest.mark.parametrize("kind", ["whole", "tail1", "tailmax"])
@pytest.mark.parametrize("nblk", SMALL_NBLK)
@pytest.mark.parametrize("bs", SMALL_BS)
def test_small_blocks_at_the_wave_and_workgroup_edges(ctx, small, mode, bs, nblk, kind):
    check(ctx, small, bs, nblk, tail_of(kind, bs))


@pytest.mark.parametrize("kind", ["whole", "tail1", "tailmax"])
def test_smallest_lane_mode_batch_of_1k_blocks(ctx, big, mode, kind):
    check(ctx, big, BIG_BS, BIG_NBLK, tail_of(kind, BIG_BS))
