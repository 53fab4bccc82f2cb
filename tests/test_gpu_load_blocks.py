"""cir_load_blocks and cir_scatter_runs_dev on the GPU.

cir_load_blocks is cir_check_blocks that keeps what it read: the verdicts are
cir_check_blocks', and the bytes of every block it read stand in the caller's
device buffers.  The reference has no counterpart (its consumers read committed
files from disk: commit_image, src/daemon/disk/commit.rs:51-117, is the last
look at the bytes).

No expected value comes from the code under test: the scatter's expected
buffers are plain slice copies (tests/scatter_cases.py), indexes are
dirsig_oracle.scan's, bitmaps, states and errnos tests/blocks_restate.py's,
file contents are read from disk here and block digests are the C oracle's.
Every destination lies inside one poisoned allocation with guard bytes around
it, and every byte of that allocation is looked at afterwards.
"""
import os
import stat
import time

import numpy as np
import pytest

from conftest import oracle_digest, oracle_sha

import blocks_restate
import dirsig_oracle
import links_restate
import scatter_cases
import test_gpu_check_blocks as cb
from blocks_restate import ABSENT, BLOCKED, COMPLETE, PARTIAL

pytestmark = pytest.mark.gpu

POISON = scatter_cases.POISON
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

@pytest.mark.parametrize("name", scatter_cases.NAMES)
def test_scatter_runs_dev(gpu, name):
    """cir_scatter_runs_dev into one poisoned buffer: every byte of it is the
    slice copy's (so a store outside a run fails), the bad records are counted
    and none of them is written; d_res is written even for the empty table."""
    import torch
    case = scatter_cases.build(name)
    d_src = torch.from_numpy(case.src.copy() if case.src_bytes else np.zeros(16, np.uint8)) \
        .to("cuda:0")
    d_buf = torch.full((case.buf_bytes,), POISON, dtype=torch.uint8, device="cuda:0")
    table = case.table(d_buf.data_ptr())
    d_runs = torch.from_numpy((table if len(table) else np.zeros(4, np.uint64)).view(np.int64)) \
        .to("cuda:0")
    d_res = torch.full((1,), 12345, dtype=torch.int64, device="cuda:0")
    rc = gpu._n.lib.cir_scatter_runs_dev(None, d_src.data_ptr() if case.src_bytes else None,
                                         case.src_bytes, d_runs.data_ptr() if case.nruns else None,
                                         case.nruns, case.nunits, d_res.data_ptr(), None)
    assert rc == 0, gpu._n.lib.cir_last_error()
    torch.cuda.synchronize()
    assert int(d_res.item()) == case.nbad
    got = d_buf.cpu().numpy()
    diff = np.nonzero(got != scatter_cases.expected(case))[0]
    assert diff.size == 0, (name, diff[:8].tolist())


# ---- 2. trees -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """{bs: complete tree}: test_gpu_check_blocks' shapes, and block size 1000
    so that run destinations are not 16-byte aligned."""
    out = {}
    for bs in (512, 4096, 1000):
        root = tmp_path_factory.mktemp("load%d" % bs) / "img"
        root.mkdir()
        cb.make_tree(root, bs)
        out[bs] = root
    return out


_indexes = {}


def index_of(trees, bs, hname="blake2b/256"):
    if (bs, hname) not in _indexes:
        _indexes[bs, hname] = dirsig_oracle.scan(str(trees[bs]), bs, hname)
    return _indexes[bs, hname]


class Buffers:
    """One poisoned allocation; file entry i's buffer inside it at a base
    offset of BASE_OFFSETS[i % 4] past a 16-byte boundary, GUARD bytes at
    least between neighbours.  skip: the ordinals that get no buffer."""

    def __init__(self, torch, index, skip=()):
        self.files = links_restate.file_entries(index)
        self.offs, pos = [], 0
        for i, (_, _, size, _) in enumerate(self.files):
            if size == 0 or i in skip:
                self.offs.append(None)
                continue
            pos = ((pos + GUARD + 15) & ~15) + BASE_OFFSETS[i % 4]
            self.offs.append(pos)
            pos += size
        self.total = pos + GUARD
        self.dev = torch.full((self.total,), POISON, dtype=torch.uint8, device="cuda:0")
        base = self.dev.data_ptr()
        assert base % 16 == 0
        self.ptrs = [None if o is None else base + o for o in self.offs]

    def host(self):
        return self.dev.cpu().numpy()


def _read_blocks(root, path, size, bs):
    """How many leading blocks of the entry cir_check_blocks reads: those
    wholly inside the file's length, when the path is a regular file reached
    through real directories."""
    p = cb.real(root, path)
    cur = os.fsencode(str(root))
    for comp in path.lstrip(b"/").split(b"/")[:-1]:
        cur = os.path.join(cur, comp)
        if not stat.S_ISDIR(os.lstat(cur).st_mode):
            return 0
    try:
        st = os.lstat(p)
    except OSError:
        return 0
    if not stat.S_ISREG(st.st_mode):
        return 0
    nblk = (size + bs - 1) // bs
    return nblk if st.st_size >= size else st.st_size // bs


def check_load(oracle, ctx, index, root, threads, skip=()):
    """One load_blocks call and every assertion of the contract; returns the
    result and the host copy of the allocation."""
    import torch
    hname, bs, _, _ = dirsig_oracle.parse(index)
    digest = oracle_sha if hname == "sha512/256" else oracle_digest
    bufs = Buffers(torch, index, skip)
    res = ctx.load_blocks(str(root), index, bufs.ptrs, threads)
    got = bufs.host()
    bits, states, longs, errnos = blocks_restate.expected(index, root)
    # the restatement with the skipped files taken out of it
    g = 0
    for i, (_, _, size, digests) in enumerate(bufs.files):
        if i in skip and size:
            bits[g:g + len(digests)] = [0] * len(digests)
            states[i], longs[i], errnos[i] = SKIPPED, False, 0
        g += len(digests)
    assert blocks_restate.same(res, (bits, states, longs, errnos)), (res.states, states)
    st = res.stats
    assert (st["have"], st["missing"]) == (sum(bits), len(bits) - sum(bits))
    assert [st[s] for s in (COMPLETE, ABSENT, PARTIAL, BLOCKED)] == \
        [states.count(s) for s in (COMPLETE, ABSENT, PARTIAL, BLOCKED)]
    assert st["skipped"] == states.count(SKIPPED)
    # the bytes
    untouched = np.ones(bufs.total, dtype=bool)      # what must still hold the poison
    g = read_bytes = 0
    for i, (path, _, size, digests) in enumerate(bufs.files):
        off = bufs.offs[i]
        if off is not None:
            nread = _read_blocks(root, path, size, bs)
            end = min(nread * bs, size)
            untouched[off:off + end] = False
            read_bytes += end
            if states[i] == COMPLETE:
                with open(cb.real(root, path), "rb") as f:
                    assert got[off:off + size].tobytes() == f.read(), path
            for j, want in enumerate(digests):
                if bits[g + j]:
                    assert j < nread
                    blk = got[off + j * bs:off + min((j + 1) * bs, size)].tobytes()
                    assert digest(oracle, blk) == want, (path, j)
        g += len(digests)
    wrong = np.nonzero(untouched & (got != POISON))[0]
    assert wrong.size == 0, wrong[:8].tolist()
    assert st["bytes"] == st["scattered_bytes"] == read_bytes
    return res, got, bufs


@pytest.mark.parametrize("bs,hname", [(512, "blake2b/256"), (4096, "blake2b/256"),
                                      (512, "sha512/256"), (1000, "blake2b/256"),
                                      (1000, "sha512/256")])
def test_complete_tree(gpu, oracle, ctx64k, ctx1m, trees, bs, hname):
    root = trees[bs]
    index = index_of(trees, bs, hname)
    for ctx in (ctx64k, ctx1m):
        for threads in (1, 4, 0):
            res, _, bufs = check_load(oracle, ctx, index, root, threads)
            assert res.complete and res.stats["bytes"] == sum(f[2] for f in bufs.files)
            want = ctx.check_blocks(str(root), index, threads)
            assert (res.have, res.states, res.errnos) == (want.have, want.states, want.errnos)
            assert [res.stats[k] for k in gpu.Context.BLOCKS_STATS_FIELDS[:8]] == \
                [want.stats[k] for k in gpu.Context.BLOCKS_STATS_FIELDS[:8]]
            if ctx is ctx64k:  # 64 KiB slots: many batches, files that span batches
                assert res.stats["batches"] >= 4


# ---- 3. mutations ---------------------------------------------------------------------------

MUTATIONS = [cb.m_flip_middle_block, cb.m_truncate_mid_block, cb.m_grow_by_one_byte,
             cb.m_missing_file, cb.m_symlink_to_identical_bytes, cb.m_directory_in_its_place]


@pytest.mark.parametrize("bs", [512, 1000])
@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda m: m.__name__[2:])
def test_one_mutation(oracle, ctx64k, ctx1m, trees, tmp_path, mutate, bs):
    """One mutation, the assertions of the complete tree: the victim's verdict
    is the restatement's, no other file's buffer or verdict changes (every
    other file is COMPLETE and its buffer is the file)."""
    index = index_of(trees, bs)
    root = cb.copy_tree(trees[bs], tmp_path)
    out = tmp_path / "outside"
    out.mkdir()
    victims = mutate(root, bs, out)
    for ctx, threads in ((ctx64k, 1), (ctx1m, 4)):
        res, got, bufs = check_load(oracle, ctx, index, root, threads)
        for i, (path, _, _, digests) in enumerate(bufs.files):
            st, lg, lost = victims.get(path, (COMPLETE, False, []))
            assert (res.states[i], res.long[i]) == (st, lg), path
            first = cb.first_block(index, path)
            assert [j for j in range(len(digests)) if not res.has(first + j)] == lost, path


# ---- 4. skipped files -----------------------------------------------------------------------

@pytest.mark.parametrize("bs", [512, 1000])
def test_skipped_files(oracle, ctx64k, trees, tmp_path, bs):
    """Every second non-empty file gets NULL: SKIPPED, bits 0, not opened (the
    tree the call sees does not even hold them), and the others load as
    before."""
    index = index_of(trees, bs)
    files = links_restate.file_entries(index)
    nonempty = [i for i, f in enumerate(files) if f[2]]
    skip = set(nonempty[1::2])
    assert len(skip) >= 4
    res, _, _ = check_load(oracle, ctx64k, index, trees[bs], 4, skip)
    assert res.stats["skipped"] == len(skip)
    assert res.stats["bytes"] == sum(f[2] for i, f in enumerate(files) if i not in skip)
    g = 0
    for i, (_, _, _, digests) in enumerate(files):
        if i in skip:
            assert res.states[i] == SKIPPED and res.errnos[i] == 0
            assert not any(res.has(g + j) for j in range(len(digests)))
        elif files[i][2]:
            assert res.states[i] == COMPLETE
        g += len(digests)
    # not opened: the same call on a copy without the skipped files, with the
    # same peak of descriptors
    root = cb.copy_tree(trees[bs], tmp_path)
    for i in skip:
        os.unlink(cb.real(root, files[i][0]))
    bare, _, _ = check_load(oracle, ctx64k, index, root, 1, skip)
    one, _, _ = check_load(oracle, ctx64k, index, trees[bs], 1, skip)
    assert (bare.have, bare.states) == (one.have, one.states) == (res.have, res.states)
    assert bare.stats["peak_fds"] == one.stats["peak_fds"]


# ---- 5. stream order ------------------------------------------------------------------------

def test_buffers_are_written_behind_the_callers_stream(gpu, oracle, ctx1m, trees):
    """In the manner of tests/test_gpu_stream_order.py: one long lane chain
    through cir_hash_blocks_dev with a NULL context on s1 (calibrated here),
    behind it the poison fill of the destinations on s1, then load_blocks(...,
    stream=s1).  A scatter that did not wait for s1 would be overwritten by the
    fill.  The precondition is proven: the event behind the delay is still
    pending immediately before the call."""
    import torch
    lib = gpu._n.lib
    bs = 512
    index = index_of(trees, bs)
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
        # the host work in front of the call: the buffers, the fill's enqueue
        bufs = Buffers(torch, index)
        t0 = time.perf_counter()
        with torch.cuda.stream(s1):
            bufs.dev.fill_(POISON)
        torch.cuda.synchronize()
        need_ms = max(50 * (time.perf_counter() - t0) * 1e3, 20.0)
        nbytes = min(cap, -(-int(need_ms / per_byte) // 4096) * 4096)
        bufs.dev.fill_(0)                                  # (not the poison: the fill must run)
        torch.cuda.synchronize()
        _, marker = delay(nbytes)
        with torch.cuda.stream(s1):
            bufs.dev.fill_(POISON)
        pending = not marker.query()
        res = ctx1m.load_blocks(str(trees[bs]), index, bufs.ptrs, 4, stream=s1.cuda_stream)
        got = bufs.host()                                  # (the call has returned: no wait needed)
        assert pending, "delay too short: nothing was tested"
        assert res.complete
        for (path, _, size, _), off in zip(bufs.files, bufs.offs):
            if off is not None:
                with open(cb.real(trees[bs], path), "rb") as f:
                    assert got[off:off + size].tobytes() == f.read(), path
    finally:
        torch.cuda.synchronize()


# ---- 6. other contexts and round trips ------------------------------------------------------

def test_split_context_and_the_context_afterwards(gpu, oracle, trees):
    """A CIR_DEBUG_SPLIT=3 context (three device states on the one GPU) loads
    through the state that owns the stream's device, and still answers
    check_index afterwards."""
    bs = 512
    index = index_of(trees, bs)
    os.environ["CIR_DEBUG_SPLIT"] = "3"
    try:
        ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    finally:
        del os.environ["CIR_DEBUG_SPLIT"]
    try:
        assert len(ctx.devices()) == 3
        res, _, _ = check_load(oracle, ctx, index, trees[bs], 4)
        assert res.complete
        assert ctx.check_index(str(trees[bs]), index).ok
        assert ctx.check_blocks(str(trees[bs]), index).complete
    finally:
        ctx.close()


def test_wrong_ndata_and_foreign_stream_device(gpu, ctx64k, trees):
    index = index_of(trees, 512)
    n = len(links_restate.file_entries(index))
    for ptrs in ([None] * (n - 1), [None] * (n + 1), []):
        with pytest.raises(gpu.CiruelaError) as e:
            ctx64k.load_blocks(str(trees[512]), index, ptrs)
        assert e.value.status == gpu._n.CIR_EINVAL
    # everything skipped: no file is opened, every non-empty entry is SKIPPED
    res = ctx64k.load_blocks(str(trees[512]), index, [None] * n)
    assert set(res.states) <= {SKIPPED, COMPLETE} and res.stats["bytes"] == 0
    assert res.stats["batches"] == 0 and res.have == bytes(len(res.have))


@pytest.mark.parametrize("bs", [4096, 1000])
def test_load_image_round_trip(gpu, ctx1m, trees, bs):
    """index_memory(load_image(...)) of a complete tree is the tree's index,
    byte for byte, and so is the ImageId."""
    index = index_of(trees, bs)
    tensors, res = gpu.load_image(str(trees[bs]), index, context=ctx1m)
    files = links_restate.file_entries(index)
    assert res.complete and set(tensors) == {f[0] for f in files if f[2]}
    import torch
    listed = [(path, tensors[path] if size else torch.zeros(0, dtype=torch.uint8, device="cuda:0"),
               exe) for path, exe, size, _ in files]
    iid = []
    back = gpu.index_memory(listed, block_size=bs, context=ctx1m, image_id=iid)
    assert back == index
    assert bytes(iid[0]) == gpu.get_hash(index)
    # `only`: the others are skipped and get no tensor
    some = [f[0] for f in files if f[2]][::3]
    tensors, res = gpu.load_image(str(trees[bs]), index, context=ctx1m, only=some)
    assert set(tensors) == set(some)
    assert res.states.count(SKIPPED) == len([f for f in files if f[2]]) - len(some)
    for path in some:
        with open(cb.real(trees[bs], path), "rb") as f:
            assert tensors[path].cpu().numpy().tobytes() == f.read()
