"""cir_reload_blocks and cir_copy_runs_dev on the GPU.

cir_reload_blocks is cir_load_blocks for a process that holds the previous
version of the image in device memory: the blocks the resident buffers hold
are copied on the device, the rest is read and verified as before.  The
reference has no counterpart (it holds no image in device memory).

No expected value comes from the code under test: copies are plain slice copies
(tests/reload_restate.py), indexes are dirsig_oracle.scan's, the digests of the
resident bytes are the C oracle's, verdicts are tests/blocks_restate.py's
combined with reload_restate's memory rule, and file contents are read from
disk here.  All device buffers of a test -- the resident ones and the
destinations -- lie inside one poisoned allocation with guard bytes between
them, and every byte of that allocation is compared afterwards.
"""
import os
import random
import shutil
import time

import numpy as np
import pytest

from conftest import oracle_digest, oracle_sha

import dirsig_oracle
import links_restate
import reload_restate
import test_gpu_check_blocks as cb
from blocks_restate import COMPLETE, PARTIAL

pytestmark = pytest.mark.gpu

POISON = reload_restate.POISON
GUARD = 64
SKIPPED = "skipped"
BASE_OFFSETS = (0, 1, 3, 8)


@pytest.fixture(scope="module")
def ctx64k(gpu):
    return gpu.Context(device_mask=1, staging_bytes=64 << 10)


@pytest.fixture(scope="module")
def ctx1m(gpu):
    return gpu.Context(device_mask=1, staging_bytes=1 << 20)


# ---- 1. the primitive against the plain slice copy ------------------------------------------

@pytest.mark.parametrize("name", reload_restate.NAMES)
def test_copy_runs_dev(gpu, name):
    """cir_copy_runs_dev inside one buffer: every byte of it is the slice
    copy's (so the sources are unchanged and a store outside a run fails), the
    bad records are counted and none of them is written; d_res is written even
    for the empty table."""
    import torch
    case = reload_restate.copy_case(name)
    d_buf = torch.from_numpy(case.initial.copy()).to("cuda:0")
    table = case.table(d_buf.data_ptr())
    d_runs = torch.from_numpy(table.view(np.int64)).to("cuda:0")
    d_res = torch.full((1,), 12345, dtype=torch.int64, device="cuda:0")
    rc = gpu._n.lib.cir_copy_runs_dev(None, d_runs.data_ptr() if case.nruns else None, case.nruns,
                                      case.given_nunits, d_res.data_ptr(), None)
    assert rc == 0, gpu._n.lib.cir_last_error()
    torch.cuda.synchronize()
    assert int(d_res.item()) == case.nbad
    got = d_buf.cpu().numpy()
    diff = np.nonzero(got != case.expected())[0]
    assert diff.size == 0, (name, diff[:8].tolist())
    if name == "thousand":
        assert case.nunits > 16 * 256


# ---- 2. trees -------------------------------------------------------------------------------

def _extra_sizes(bs):
    return {"x1": 1, "x15": 15, "x16": 16, "x17": 17, "xbsm1": bs - 1, "xbsp1": bs + 1,
            "x3bs5": 3 * bs + 5, "x200k": 200 << 10}


DELETED = b"/zeros"      # wholly resident, and gone from the directory the call sees


@pytest.fixture(scope="module")
def versions(tmp_path_factory):
    """{bs: (version N, version N + 1, version N + 1 as the call sees it)}:
    N is test_gpu_check_blocks' tree and files of 1, 15, 16, 17, bs - 1, bs + 1,
    3 bs + 5 bytes and 200 KiB; N + 1 has one byte flipped in a middle block,
    one file appended to, one truncated, one renamed, one new, one deleted and
    one that is a copy of another's middle blocks.  The third tree is N + 1
    without one of the files that memory holds whole."""
    out = {}
    for bs in (512, 4096, 1000):
        base = tmp_path_factory.mktemp("reload%d" % bs)
        old = base / "n"
        old.mkdir()
        cb.make_tree(old, bs)
        rng = random.Random(7 * bs)
        for name, size in _extra_sizes(bs).items():
            (old / name).write_bytes(rng.randbytes(size))
        new = base / "n1"
        shutil.copytree(str(old), str(new))
        mid = (new / "b130").read_bytes()[5 * bs:25 * bs]
        with open(new / "b130", "r+b") as f:
            f.seek(64 * bs + 5)
            c = f.read(1)
            f.seek(64 * bs + 5)
            f.write(bytes([c[0] ^ 0x40]))
        with open(new / "b63", "ab") as f:
            f.write(rng.randbytes(100))
        os.truncate(new / "b65", 40 * bs + 3)
        os.rename(new / "sub" / "mid", new / "sub" / "moved")
        (new / "fresh").write_bytes(rng.randbytes(3 * bs + 5))
        os.unlink(new / "b64")
        (new / "copy_mid").write_bytes(mid)
        seen = base / "seen"
        shutil.copytree(str(new), str(seen))
        os.unlink(cb.real(seen, DELETED))
        out[bs] = (old, new, seen)
    return out


_cache = {}


def _digest_fn(oracle, hname):
    fn = oracle_sha if hname == "sha512/256" else oracle_digest
    return lambda data: fn(oracle, data)


def _index(root, bs, hname):
    key = ("index", str(root), bs, hname)
    if key not in _cache:
        _cache[key] = dirsig_oracle.scan(str(root), bs, hname)
    return _cache[key]


def _file_bytes(root, path):
    with open(cb.real(root, path), "rb") as f:
        return f.read()


class Arena:
    """One poisoned allocation; the resident buffers, then the destinations,
    each at a base offset of BASE_OFFSETS[i % 4] past a 16-byte boundary, GUARD
    bytes at least between neighbours.  sizes 0 or ordinals in skip get no
    buffer."""

    def __init__(self, torch, resident_sizes, dest_sizes, skip=()):
        pos = 0

        def lay(sizes, skip):
            nonlocal pos
            offs = []
            for i, size in enumerate(sizes):
                if size == 0 or i in skip:
                    offs.append(None)
                    continue
                pos = ((pos + GUARD + 15) & ~15) + BASE_OFFSETS[i % 4]
                offs.append(pos)
                pos += size
            return offs

        self.res_sizes, self.dest_sizes = list(resident_sizes), list(dest_sizes)
        self.res_offs = lay(self.res_sizes, ())
        self.dest_offs = lay(self.dest_sizes, skip)
        self.total = pos + GUARD
        self.dev = torch.full((self.total,), POISON, dtype=torch.uint8, device="cuda:0")
        self.base = self.dev.data_ptr()
        assert self.base % 16 == 0
        self.res_ptrs = [None if o is None else self.base + o for o in self.res_offs]
        self.dest_ptrs = [None if o is None else self.base + o for o in self.dest_offs]

    def resident(self, order_seed=1):
        """The resident list as the call takes it: (ptr, bytes), shuffled."""
        spans = [(p, n) for p, n in zip(self.res_ptrs, self.res_sizes) if p is not None]
        random.Random(order_seed).shuffle(spans)
        return spans

    def host(self):
        return self.dev.cpu().numpy()


def _load_old(ctx, arena, old, index_n):
    res = ctx.load_blocks(str(old), index_n, arena.res_ptrs, 4)
    assert res.complete
    return arena.host()


def _have_set(oracle, hname, bs, arena, snapshot):
    return reload_restate.resident_set(
        _digest_fn(oracle, hname), bs,
        [snapshot[o:o + n].tobytes() for o, n in zip(arena.res_offs, arena.res_sizes)
         if o is not None])


def _check_result(res, e, files_n1):
    assert reload_restate.same(res, e), (res.states, e.states, res.resident, e.resident)
    st = res.stats
    assert (st["have"], st["missing"]) == (sum(e.bits), len(e.bits) - sum(e.bits))
    assert st["copied_blocks"] == e.copied == sum(e.mem)
    assert st["copied_bytes"] == e.copied_bytes
    assert st["bytes"] == st["scattered_bytes"] == e.disk_bytes
    assert st["resident_files"] == sum(e.resident)
    assert st["skipped"] == e.states.count(SKIPPED)
    # (a match dropped for its length needs two blocks of different lengths with one
    # digest: a hash collision.  No test on real digests can force one; the branch is
    # run on the host by tools/copyblk_fuzz.cpp against a block-by-block loop)
    assert st["dropped_length"] == 0
    assert st[COMPLETE] == e.states.count(COMPLETE)


def _expected_allocation(before, arena, files_n1, e, root):
    """The allocation afterwards: what it held, and in every destination the
    file's bytes (of a tree whose blocks all have their bits)."""
    want = before.copy()
    for (path, _, size, _), off in zip(files_n1, arena.dest_offs):
        if off is not None:
            want[off:off + size] = np.frombuffer(_file_bytes(root, path), dtype=np.uint8)
    return want


@pytest.mark.parametrize("bs,hname", [(512, "blake2b/256"), (4096, "blake2b/256"),
                                      (1000, "blake2b/256"), (512, "sha512/256"),
                                      (1000, "sha512/256")])
def test_next_version(gpu, oracle, ctx64k, ctx1m, versions, bs, hname):
    import torch
    old, new, seen = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    files_n = links_restate.file_entries(index_n)
    files_n1 = links_restate.file_entries(index_n1)
    ordinal = {f[0]: i for i, f in enumerate(files_n1)}
    e = None
    for ctx in (ctx64k, ctx1m):
        for threads in (1, 4, 0):
            arena = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
            before = _load_old(ctx, arena, old, index_n)
            if e is None:      # (the resident bytes are the files of version N: once)
                have = _have_set(oracle, hname, bs, arena, before)
                e = reload_restate.expected(index_n1, seen, have)
            res = ctx.reload_blocks(str(seen), index_n1, arena.dest_ptrs,
                                    arena.resident(threads), threads)
            got = arena.host()
            _check_result(res, e, files_n1)
            assert res.complete and all(e.bits)
            want = _expected_allocation(before, arena, files_n1, e, new)
            diff = np.nonzero(got != want)[0]
            assert diff.size == 0, diff[:8].tolist()
            assert res.stats["resident_blocks"] == sum(len(f[3]) for f in files_n)
            # the index of what now stands in the destinations is version N + 1's
            listed = [(path, (arena.dest_ptrs[i] or arena.base, size), exe)
                      for i, (path, exe, size, _) in enumerate(files_n1)]
            iid = []
            back = gpu.index_memory(listed, block_size=bs, context=ctx, image_id=iid,
                                    hash_type=getattr(gpu.HashType, cb.HASHES[hname])())
            assert back == index_n1
            assert bytes(iid[0]) == gpu.get_hash(index_n1)
    # what the versions were built to show
    for path in (DELETED, b"/sub/moved", b"/copy_mid", b"/x200k", b"/b1", b"/x1", b"/x17"):
        assert e.resident[ordinal[path]], path        # unchanged, renamed, copied: never opened
    for path in (b"/fresh", b"/b130", b"/b63", b"/b65"):
        assert not e.resident[ordinal[path]], path
    g = cb.first_block(index_n1, b"/b130")
    assert [j for j in range(130) if not e.mem[g + j]] == [64]     # the flipped block alone
    g = cb.first_block(index_n1, b"/b63")
    assert e.mem[g:g + 64] == [1] * 63 + [0]                       # the appended tail alone
    g = cb.first_block(index_n1, b"/b65")
    assert e.mem[g:g + 41] == [1] * 40 + [0]                       # the new short tail alone
    g = cb.first_block(index_n1, b"/fresh")
    assert e.mem[g:g + 4] == [0] * 4
    # bytes read from disk: exactly the blocks that are not resident
    want_bytes = 0
    for (path, _, size, digests), off in zip(files_n1, arena.dest_offs):
        g = cb.first_block(index_n1, path)
        want_bytes += sum(min(bs, size - j * bs) for j in range(len(digests)) if not e.mem[g + j])
    assert e.disk_bytes == want_bytes


# ---- 3. memory is not believed --------------------------------------------------------------

@pytest.mark.parametrize("bs", [512, 1000])
def test_corrupted_resident_block_comes_from_disk(gpu, oracle, ctx64k, versions, bs):
    import torch
    hname = "blake2b/256"
    old, new, seen = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    files_n = links_restate.file_entries(index_n)
    files_n1 = links_restate.file_entries(index_n1)
    arena = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
    _load_old(ctx64k, arena, old, index_n)
    victim = [i for i, f in enumerate(files_n) if f[0] == b"/x200k"][0]
    at = arena.res_offs[victim] + 2 * bs + 7          # block 2: unchanged between the versions
    arena.dev[at] ^= 0x10
    torch.cuda.synchronize()
    before = arena.host()
    e = reload_restate.expected(index_n1, seen, _have_set(oracle, hname, bs, arena, before))
    res = ctx64k.reload_blocks(str(seen), index_n1, arena.dest_ptrs, arena.resident(), 4)
    got = arena.host()
    _check_result(res, e, files_n1)
    i = [i for i, f in enumerate(files_n1) if f[0] == b"/x200k"][0]
    g = cb.first_block(index_n1, b"/x200k")
    nblk = len(files_n1[i][3])
    assert [j for j in range(nblk) if not e.mem[g + j]] == [2]
    assert res.states[i] == COMPLETE and not res.resident[i] and res.complete
    diff = np.nonzero(got != _expected_allocation(before, arena, files_n1, e, new))[0]
    assert diff.size == 0, diff[:8].tolist()


# ---- 4. equivalence with load_blocks --------------------------------------------------------

@pytest.mark.parametrize("mode", ["env", "empty_list"])
def test_without_memory_it_is_load_blocks(gpu, ctx64k, versions, mode):
    import torch
    bs, hname = 512, "blake2b/256"
    old, new, _ = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    files_n = links_restate.file_entries(index_n)
    files_n1 = links_restate.file_entries(index_n1)
    arena = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
    before = _load_old(ctx64k, arena, old, index_n)
    if mode == "env":
        os.environ["CIR_RELOAD"] = "disk"
    try:
        res = ctx64k.reload_blocks(str(new), index_n1, arena.dest_ptrs,
                                   arena.resident() if mode == "env" else [None, (0, 0)], 4)
    finally:
        os.environ.pop("CIR_RELOAD", None)
    got = arena.host()
    other = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
    want = ctx64k.load_blocks(str(new), index_n1, other.dest_ptrs, 4)
    assert (res.have, res.states, res.long, res.errnos) == \
        (want.have, want.states, want.long, want.errnos)
    assert not any(res.resident)
    assert [res.stats[k] for k in gpu.Context.LOAD_STATS_FIELDS[:8]] == \
        [want.stats[k] for k in gpu.Context.LOAD_STATS_FIELDS[:8]]
    assert [res.stats[k] for k in gpu.Context.RELOAD_STATS_FIELDS[12:]] == [0] * 5
    lo = min(o for o in arena.dest_offs if o is not None)
    assert (got[lo:] == other.host()[lo:]).all()         # the destinations and their guards
    assert (got[:lo] == before[:lo]).all()               # the resident buffers


# ---- 5. also --------------------------------------------------------------------------------

def test_bad_block_on_disk_and_a_skipped_file(gpu, oracle, ctx1m, versions, tmp_path):
    """One bad block on disk whose content is not resident: bit 0 and partial,
    its neighbours unaffected.  One file without a destination: skipped."""
    import torch
    bs, hname = 1000, "blake2b/256"
    old, new, seen = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    files_n = links_restate.file_entries(index_n)
    files_n1 = links_restate.file_entries(index_n1)
    ordinal = {f[0]: i for i, f in enumerate(files_n1)}
    root = cb.copy_tree(seen, tmp_path)
    with open(cb.real(root, b"/fresh"), "r+b") as f:
        f.seek(bs + 3)
        f.write(b"\xff\x00\xff")
    skip = {ordinal[b"/x200k"]}
    arena = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1], skip)
    before = _load_old(ctx1m, arena, old, index_n)
    e = reload_restate.expected(index_n1, root, _have_set(oracle, hname, bs, arena, before), skip)
    res = ctx1m.reload_blocks(str(root), index_n1, arena.dest_ptrs, arena.resident(), 4)
    got = arena.host()
    _check_result(res, e, files_n1)
    i = ordinal[b"/fresh"]
    g = cb.first_block(index_n1, b"/fresh")
    assert res.states[i] == PARTIAL and [res.has(g + j) for j in range(4)] == [1, 0, 1, 1]
    assert res.states[ordinal[b"/x200k"]] == SKIPPED
    assert [s for k, s in enumerate(res.states) if k not in (i, ordinal[b"/x200k"])] == \
        [COMPLETE] * (len(files_n1) - 2)
    # everything but the bad block's bytes (unspecified) is the files' or what it was
    want = _expected_allocation(before, arena, files_n1, e, new)
    off = arena.dest_offs[i]
    want[off + bs:off + 2 * bs] = got[off + bs:off + 2 * bs]
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, diff[:8].tolist()


def _small_case(torch, gpu, oracle, ctx, tmp_path, resident_bytes, name):
    """One file t of 2 bs + 100 bytes against resident buffers given as bytes."""
    bs, hname = 512, "blake2b/256"
    root = tmp_path / name
    root.mkdir()
    data = random.Random(99).randbytes(2 * bs + 100)
    (root / "t").write_bytes(data)
    index = dirsig_oracle.scan(str(root), bs, hname)
    bufs = [b(data) for b in resident_bytes]
    arena = Arena(torch, [len(b) for b in bufs], [len(data)])
    for off, b in zip(arena.res_offs, bufs):
        arena.dev[off:off + len(b)] = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()) \
            .to("cuda:0")
    torch.cuda.synchronize()
    before = arena.host()
    e = reload_restate.expected(index, root, _have_set(oracle, hname, bs, arena, before))
    res = ctx.reload_blocks(str(root), index, arena.dest_ptrs, arena.resident(), 1)
    got = arena.host()
    _check_result(res, e, links_restate.file_entries(index))
    want = before.copy()
    off = arena.dest_offs[0]
    want[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    assert (got == want).all()
    return res, e


def test_tails_and_lengths(gpu, oracle, ctx64k, tmp_path):
    """A tail block matches only a resident tail of equal length; a resident
    buffer that ends mid-block gives no block of the new length."""
    import torch
    bs = 512
    middle = lambda d: d[bs:2 * bs]                    # block 1, whole
    tail = lambda d: d[2 * bs:]                        # the 100-byte tail as a buffer of its own
    longer = lambda d: d[2 * bs:] + bytes(50)          # the tail's bytes in a 150-byte block
    cut = lambda d: d[:bs + 200]                       # block 0, then a buffer end mid-block
    res, e = _small_case(torch, gpu, oracle, ctx64k, tmp_path, [middle, tail, longer, cut], "a")
    assert e.mem == [1, 1, 1] and res.resident == [True] and res.stats["bytes"] == 0
    res, e = _small_case(torch, gpu, oracle, ctx64k, tmp_path, [middle, longer, cut], "b")
    assert e.mem == [1, 1, 0] and res.resident == [False] and res.stats["bytes"] == 100
    res, e = _small_case(torch, gpu, oracle, ctx64k, tmp_path, [cut, longer], "c")
    assert e.mem == [1, 0, 0] and res.stats["bytes"] == bs + 100
    assert res.complete and res.stats["resident_blocks"] == 2 + 1


def test_overlap_and_too_many_resident_blocks(gpu, ctx64k, versions):
    """A destination that overlaps a resident buffer, and a resident list of
    2^31 blocks: CIR_EINVAL with nothing touched."""
    import torch
    bs, hname = 512, "blake2b/256"
    old, new, seen = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    files_n = links_restate.file_entries(index_n)
    files_n1 = links_restate.file_entries(index_n1)
    arena = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
    before = _load_old(ctx64k, arena, old, index_n)
    big = max(range(len(files_n)), key=lambda i: files_n[i][2])
    for shift in (0, 5, files_n[big][2] - 1):
        ptrs = list(arena.dest_ptrs)
        k = [i for i, f in enumerate(files_n1) if f[0] == b"/x1"][0]
        ptrs[k] = arena.res_ptrs[big] + shift          # one byte inside a resident buffer
        with pytest.raises(gpu.CiruelaError) as err:
            ctx64k.reload_blocks(str(seen), index_n1, ptrs, arena.resident(), 4)
        assert err.value.status == gpu._n.CIR_EINVAL and "overlaps" in str(err.value)
    tiny = dirsig_oracle.emit("blake2b/256", 1, [
        (b"/", [("f", b"a", False, 1, dirsig_oracle.block_hashes(b"x", 1, "blake2b/256"))])])
    one = [arena.base + arena.total - 1]
    with pytest.raises(gpu.CiruelaError) as err:
        ctx64k.reload_blocks(str(seen), tiny, one, [(arena.base, 1 << 31)], 1)
    assert err.value.status == gpu._n.CIR_EINVAL and "resident blocks" in str(err.value)
    assert (arena.host() == before).all()


def test_buffers_are_written_behind_the_callers_stream(gpu, ctx1m, versions):
    """test_gpu_load_blocks' stream test with a reload: one long lane chain on
    s1 (calibrated here), behind it the poison fill of the destinations on s1,
    then reload_blocks(..., stream=s1).  A copy or a scatter that did not wait
    for s1 would be overwritten by the fill.  The precondition is proven: the
    event behind the delay is still pending immediately before the call."""
    import torch
    lib = gpu._n.lib
    bs, hname = 512, "blake2b/256"
    old, new, seen = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    files_n = links_restate.file_entries(index_n)
    files_n1 = links_restate.file_entries(index_n1)
    s1 = torch.cuda.Stream()
    cap = 64 << 20
    buf = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    d_off = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_len = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_out = torch.zeros(32, dtype=torch.uint8, device="cuda:0")

    def delay(nbytes):
        d_len.fill_(nbytes)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s1)
        assert lib.cir_hash_blocks_dev(None, buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                       1, d_out.data_ptr(), s1.cuda_stream) == 0
        e1.record(s1)
        return e0, e1

    try:
        ms = []
        for nbytes in (256 << 10, 256 << 10, 1 << 20):     # the first loads the kernel
            e0, e1 = delay(nbytes)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        per_byte = max(ms[2] - ms[1], 1e-6) / ((1 << 20) - (256 << 10))
        arena = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
        _load_old(ctx1m, arena, old, index_n)
        lo = min(o for o in arena.dest_offs if o is not None)
        dests = arena.dev[lo:]
        t0 = time.perf_counter()
        with torch.cuda.stream(s1):
            dests.fill_(POISON)
        torch.cuda.synchronize()
        need_ms = max(50 * (time.perf_counter() - t0) * 1e3, 20.0)
        nbytes = min(cap, -(-int(need_ms / per_byte) // 4096) * 4096)
        dests.fill_(0)                                     # (not the poison: the fill must run)
        torch.cuda.synchronize()
        _, marker = delay(nbytes)
        with torch.cuda.stream(s1):
            dests.fill_(POISON)
        pending = not marker.query()
        res = ctx1m.reload_blocks(str(seen), index_n1, arena.dest_ptrs, arena.resident(), 4,
                                  stream=s1.cuda_stream)
        got = arena.host()                                 # (the call has returned: no wait needed)
        assert pending, "delay too short: nothing was tested"
        assert res.complete and res.stats["copied_blocks"] > 0 and res.stats["bytes"] > 0
        for (path, _, size, _), off in zip(files_n1, arena.dest_offs):
            if off is not None:
                assert got[off:off + size].tobytes() == _file_bytes(new, path), path
    finally:
        torch.cuda.synchronize()


def test_split_context_and_the_context_afterwards(gpu, oracle, versions):
    """A CIR_DEBUG_SPLIT=3 context (three device states on the one GPU) reloads
    through the state that owns the stream's device, and still answers
    check_index afterwards."""
    import torch
    bs, hname = 512, "blake2b/256"
    old, new, seen = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    files_n = links_restate.file_entries(index_n)
    files_n1 = links_restate.file_entries(index_n1)
    os.environ["CIR_DEBUG_SPLIT"] = "3"
    try:
        ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    finally:
        del os.environ["CIR_DEBUG_SPLIT"]
    try:
        assert len(ctx.devices()) == 3
        arena = Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
        before = _load_old(ctx, arena, old, index_n)
        e = reload_restate.expected(index_n1, seen, _have_set(oracle, hname, bs, arena, before))
        res = ctx.reload_blocks(str(seen), index_n1, arena.dest_ptrs, arena.resident(), 4)
        _check_result(res, e, files_n1)
        got = arena.host()
        assert (got == _expected_allocation(before, arena, files_n1, e, new)).all()
        assert ctx.check_index(str(new), index_n1).ok
    finally:
        ctx.close()


def test_reload_image(gpu, ctx1m, versions):
    """reload_image with the dict load_image returned: new tensors that hold
    version N + 1, the old ones left alone."""
    bs, hname = 4096, "blake2b/256"
    old, new, seen = versions[bs]
    index_n, index_n1 = _index(old, bs, hname), _index(new, bs, hname)
    held, res = gpu.load_image(str(old), index_n, context=ctx1m)
    assert res.complete
    tensors, res = gpu.reload_image(str(seen), index_n1, held, context=ctx1m)
    files_n1 = links_restate.file_entries(index_n1)
    assert res.complete and set(tensors) == {f[0] for f in files_n1 if f[2]}
    assert res.stats["copied_blocks"] > 0 and res.resident[[f[0] for f in files_n1].index(DELETED)]
    for path, t in tensors.items():
        assert t.cpu().numpy().tobytes() == _file_bytes(new, path), path
    for path, t in held.items():
        assert t.cpu().numpy().tobytes() == _file_bytes(old, path), path
