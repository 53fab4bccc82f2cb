"""cir_store_blocks and cir_gather_runs_dev on the GPU.

cir_store_blocks is cir_load_blocks mirrored: files held in device memory are
written out as an image directory and the directory's index comes back.  The
reference has no counterpart (an image directory is filled block by block from
the network: write_block, src/daemon/disk/public.rs).

No expected value comes from the code under test: the gather's expected
buffers are plain slice copies (tests/gather_cases.py), expected indexes are
dirsig_oracle.emit over dirsig_oracle.block_hashes of the source bytes, and
expected trees are the source bytes.  Every source lies inside one poisoned
allocation with guard bytes around it.
"""
import errno
import os
import random
import stat

import numpy as np
import pytest

import dirsig_oracle
import emit_restate
import gather_cases
import links_restate
from test_gpu_index_emit import Delay

pytestmark = pytest.mark.gpu

POISON = gather_cases.POISON
GUARD = 64
BASE_OFFSETS = (0, 1, 3, 8)
HASHES = ("blake2b/256", "sha512/256")


@pytest.fixture(scope="module")
def ctx64k(gpu):
    return gpu.Context(device_mask=1, staging_bytes=64 << 10)


@pytest.fixture(scope="module")
def ctx1m(gpu):
    return gpu.Context(device_mask=1, staging_bytes=1 << 20)


def hash_type(gpu, hname):
    return gpu.HashType.sha512_256() if hname == "sha512/256" else gpu.HashType.blake2b_256()


# ---- 1. the primitive against the plain slice copy ------------------------------------------

@pytest.mark.parametrize("name", gather_cases.NAMES)
def test_gather_runs_dev(gpu, name):
    """cir_gather_runs_dev into one poisoned buffer from sources of every
    alignment inside one poisoned allocation: every byte of the buffer is the
    slice copy's (so a store outside a record's rounded range fails), the bad
    records are counted and leave no trace, the source allocation is unchanged;
    d_res is written even for the empty table."""
    import torch
    case = gather_cases.build(name)
    d_src = torch.from_numpy(case.src.copy()).to("cuda:0")
    assert d_src.data_ptr() % 16 == 0
    d_buf = torch.full((case.buf_bytes,), POISON, dtype=torch.uint8, device="cuda:0")
    table = case.table(d_src.data_ptr())
    d_runs = torch.from_numpy((table if len(table) else np.zeros(4, np.uint64)).view(np.int64)) \
        .to("cuda:0")
    d_res = torch.full((1,), 12345, dtype=torch.int64, device="cuda:0")
    rc = gpu._n.lib.cir_gather_runs_dev(None, d_buf.data_ptr() if case.nunits else None,
                                        case.dst_bytes, d_runs.data_ptr() if case.nruns else None,
                                        case.nruns, case.nunits, d_res.data_ptr(), None)
    assert rc == 0, gpu._n.lib.cir_last_error()
    torch.cuda.synchronize()
    assert int(d_res.item()) == case.nbad
    got = d_buf.cpu().numpy()
    diff = np.nonzero(got != gather_cases.expected(case))[0]
    assert diff.size == 0, (name, diff[:8].tolist())
    assert (d_src.cpu().numpy() == case.src).all()


# ---- 2. trees -------------------------------------------------------------------------------

def tree_files(bs):
    """[(path, data, exe)] in an order that is not the index's: nested
    directories, a name that needs \\xNN escaping, exe on some, every size at
    which a run, a block or a batch ends differently."""
    rng = random.Random(bs + 7)
    shapes = [(b"/three", 3 * bs + 5, False), (b"/empty", 0, False), (b"/sub/f15", 15, False),
              (b"/sub/deep/f17", 17, True), (b"/one", 1, False), (b"/big", (200 << 10) + 7, False),
              (b"/sub/f16", 16, True), (b"/sp ace\xff/n\\m", bs + 1, False),
              (b"/sub/deep/bsm1", bs - 1, False), (b"/bs", bs, True),
              (b"/sub/deep/empty2", 0, True), (b"/sub/bsp1", bs + 1, False),
              (b"/other/x/y/z", 2 * bs, False)]
    return [(p, rng.randbytes(n), exe) for p, n, exe in shapes]


_expected = {}


def expected_index(bs, hname):
    if (bs, hname) not in _expected:
        _expected[bs, hname] = emit_restate.index_of(
            [(p, exe, len(data), dirsig_oracle.block_hashes(data, bs, hname))
             for p, data, exe in tree_files(bs)], bs, hname)
    return _expected[bs, hname]


class Sources:
    """One poisoned allocation; file i's bytes inside it at a base offset of
    BASE_OFFSETS[i % 4] past a 16-byte boundary, GUARD bytes at least between
    neighbours.  listed: what store_blocks and index_memory take."""

    def __init__(self, torch, files, fill=True):
        self.files = files
        self.offs, pos = [], 0
        for i, (_, data, _) in enumerate(files):
            pos = ((pos + GUARD + 15) & ~15) + BASE_OFFSETS[i % 4]
            self.offs.append(pos)
            pos += len(data)
        self.total = pos + GUARD
        self.host = np.full(self.total, POISON, dtype=np.uint8)
        for off, (_, data, _) in zip(self.offs, files):
            self.host[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host if fill else np.zeros_like(self.host)).to("cuda:0")
        base = self.dev.data_ptr()
        assert base % 16 == 0
        self.listed = [(p, (base + off if data else 0, len(data)), exe)
                       for off, (p, data, exe) in zip(self.offs, files)]


def real(root, path):
    return os.path.join(os.fsencode(str(root)), path.lstrip(b"/"))


def check_tree(root, files):
    """The tree below root is exactly the files: contents, modes, and no other
    name anywhere."""
    want_dirs, want_files = {b""}, set()
    for path, data, exe in files:
        parts = path.lstrip(b"/").split(b"/")
        for k in range(1, len(parts)):
            want_dirs.add(b"/".join(parts[:k]))
        want_files.add(b"/".join(parts))
        st = os.lstat(real(root, path))
        assert stat.S_ISREG(st.st_mode), path
        assert stat.S_IMODE(st.st_mode) == (0o755 if exe else 0o644), (path, oct(st.st_mode))
        with open(real(root, path), "rb") as f:
            assert f.read() == data, path
    got_dirs, got_files = set(), set()
    top = os.fsencode(str(root))
    for cur, dirs, names in os.walk(top):
        rel = os.path.relpath(cur, top)
        rel = b"" if rel == b"." else rel
        got_dirs.add(rel)
        for d in dirs:
            assert not os.path.islink(os.path.join(cur, d))
        got_files |= {os.path.join(rel, n) if rel else n for n in names}
    assert got_dirs == want_dirs and got_files == want_files


def check_store(gpu, ctx, bs, hname, threads, root, src):
    """One store_blocks call and every assertion of the contract."""
    import torch
    files = src.files
    iid, stats = [], {}
    index = ctx.store_blocks(str(root), src.listed, bs, hash_type(gpu, hname), threads=threads,
                             image_id=iid, stats=stats)
    check_tree(root, files)
    assert index == expected_index(bs, hname)
    mem_id = []
    assert index == gpu.index_memory(src.listed, bs, hash_type(gpu, hname), context=ctx,
                                     image_id=mem_id)
    cfg = gpu.ScannerConfig.new().threads(2).hash(hash_type(gpu, hname)).block_size(bs)
    cfg.add_dir(str(root), "/")
    assert index == gpu.v1.scan(cfg, context=ctx)
    assert bytes(iid[0]) == bytes(mem_id[0]) == bytes.fromhex(index[-65:-1].decode())
    assert ctx.check_index(str(root), index).ok
    nblk = sum((len(d) + bs - 1) // bs for _, d, _ in files)
    assert (stats["blocks"], stats["files"], stats["bytes"]) == \
        (nblk, len(files), sum(len(d) for _, d, _ in files))
    assert stats["body_bytes"] == len(index) - index.index(b"\n") - 1 - 65
    # the sources are read, never written
    assert (src.dev.cpu().numpy() == src.host).all()
    return index, stats


@pytest.mark.parametrize("hname", HASHES)
@pytest.mark.parametrize("bs", [512, 4096, 1000])
def test_trees(gpu, ctx64k, ctx1m, tmp_path, bs, hname):
    import torch
    src = Sources(torch, tree_files(bs))
    ndirs = 6                     # sub, sub/deep, "sp ace\xff", other, other/x, other/x/y
    for ci, ctx in enumerate((ctx64k, ctx1m)):
        for threads in (1, 4, 0):
            root = tmp_path / ("img%d_%d" % (ci, threads))
            root.mkdir()
            _, stats = check_store(gpu, ctx, bs, hname, threads, root, src)
            assert stats["dirs_made"] == ndirs
            if ctx is ctx64k:     # 64 KiB slots: the 200 KiB file spans batches
                assert stats["batches"] >= 4


def test_existing_directories_are_accepted_and_a_dir_fd_root(gpu, ctx64k, tmp_path):
    import torch
    bs = 512
    src = Sources(torch, tree_files(bs))
    root = tmp_path / "img"
    (root / "sub" / "deep").mkdir(parents=True)
    fd = os.open(str(root), os.O_RDONLY | os.O_DIRECTORY)
    try:
        stats = {}
        index = ctx64k.store_blocks(None, src.listed, bs, gpu.HashType.blake2b_256(), dir_fd=fd,
                                    stats=stats)
    finally:
        os.close(fd)
    assert index == expected_index(bs, "blake2b/256") and stats["dirs_made"] == 4
    check_tree(root, src.files)


# ---- 3. the closed loop ---------------------------------------------------------------------

@pytest.mark.parametrize("bs", [4096, 1000])
def test_store_load_round_trip(gpu, ctx1m, tmp_path, bs):
    """load_image(root, store_image(root, files)) returns tensors equal to the
    sources, every file "complete"."""
    import torch
    files = tree_files(bs)
    src = Sources(torch, files)
    tensors = [(p, src.dev[off:off + len(data)], exe)
               for off, (p, data, exe) in zip(src.offs, files)]
    root = tmp_path / "img"
    root.mkdir()
    index = gpu.store_image(str(root), tensors, block_size=bs, context=ctx1m, threads=2)
    assert index == expected_index(bs, "blake2b/256")
    back, res = gpu.load_image(str(root), index, context=ctx1m)
    assert res.complete and set(res.states) == {"complete"}
    assert set(back) == {p for p, data, _ in files if data}
    for p, data, _ in files:
        if data:
            assert back[p].cpu().numpy().tobytes() == data, p
    entries = links_restate.file_entries(index)
    listed = [(path, back[path] if size else torch.zeros(0, dtype=torch.uint8, device="cuda:0"),
               exe) for path, exe, size, _ in entries]
    assert gpu.index_memory(listed, block_size=bs, context=ctx1m) == index


# ---- 4. stream order ------------------------------------------------------------------------

def test_sources_are_read_behind_the_callers_stream(gpu, ctx1m, tmp_path):
    """The data is still being produced when the call is made: a delay, then
    the copy that fills the sources, then the call, all on one stream with no
    synchronise in between.  The sources hold zeros until the copy runs, so a
    gather that did not wait would store zeros."""
    import torch
    bs = 4096
    files = tree_files(bs)
    src = Sources(torch, files, fill=False)
    staged = torch.from_numpy(src.host).to("cuda:0")
    root = tmp_path / "img"
    root.mkdir()
    st = torch.cuda.Stream()
    delay = Delay(gpu)
    torch.cuda.synchronize()
    started = torch.cuda.Event()
    delay.queue(st)
    started.record(st)
    with torch.cuda.stream(st):
        src.dev.copy_(staged, non_blocking=True)
    assert not started.query(), "delay too short: nothing was tested"
    index = ctx1m.store_blocks(str(root), src.listed, bs, gpu.HashType.blake2b_256(), threads=2,
                               stream=st.cuda_stream)
    assert index == expected_index(bs, "blake2b/256")
    check_tree(root, files)


# ---- 5. refusals ----------------------------------------------------------------------------

def test_an_existing_file_is_refused(gpu, ctx64k, tmp_path):
    import torch
    bs = 512
    src = Sources(torch, tree_files(bs))
    root = tmp_path / "img"
    (root / "sub").mkdir(parents=True)
    (root / "sub" / "f16").write_bytes(b"mine")
    with pytest.raises(gpu.CiruelaError) as e:
        ctx64k.store_blocks(str(root), src.listed, bs, gpu.HashType.blake2b_256())
    assert e.value.status == gpu._n.CIR_EIO
    assert os.strerror(errno.EEXIST) in e.value.detail and "errno %d" % errno.EEXIST in e.value.detail
    assert "/sub/f16" in e.value.detail
    assert (root / "sub" / "f16").read_bytes() == b"mine"


def test_a_symlinked_directory_is_refused(gpu, ctx64k, tmp_path):
    import torch
    other = tmp_path / "elsewhere"
    other.mkdir()
    root = tmp_path / "img"
    root.mkdir()
    os.symlink(str(other), str(root / "sub"))
    src = Sources(torch, [(b"/sub/a", b"x" * 700, False), (b"/b", b"y" * 30, False)])
    with pytest.raises(gpu.CiruelaError) as e:
        ctx64k.store_blocks(str(root), src.listed, 512, gpu.HashType.blake2b_256())
    assert e.value.status == gpu._n.CIR_EIO and "/sub/a" in e.value.detail
    assert os.listdir(str(other)) == []
    assert os.path.islink(str(root / "sub"))
    # a symlink in a file's place: O_EXCL refuses it, and nothing goes through it
    root2 = tmp_path / "img2"
    root2.mkdir()
    os.symlink(str(other / "target"), str(root2 / "b"))
    with pytest.raises(gpu.CiruelaError) as e:
        ctx64k.store_blocks(str(root2), src.listed[1:], 512, gpu.HashType.blake2b_256())
    assert e.value.status == gpu._n.CIR_EIO
    assert os.listdir(str(other)) == []


def test_a_missing_root_and_a_foreign_list(gpu, ctx64k, tmp_path):
    import torch
    src = Sources(torch, [(b"/a", b"x" * 700, False)])
    with pytest.raises(gpu.CiruelaError) as e:
        ctx64k.store_blocks(str(tmp_path / "nowhere"), src.listed, 512, gpu.HashType.blake2b_256())
    assert e.value.status == gpu._n.CIR_EIO
    assert not (tmp_path / "nowhere").exists()
    # the list's CIR_EINVAL cases with a real context: nothing is created
    root = tmp_path / "img"
    root.mkdir()
    a = src.listed[0][1]
    for bad in ([(b"/a", a), (b"/a/b", a)], [(b"/a", a), (b"/a", a)], [(b"/x/../a", a)],
                [(b"/a", (0, 700))]):
        with pytest.raises(gpu.CiruelaError) as e:
            ctx64k.store_blocks(str(root), bad, 512, gpu.HashType.blake2b_256())
        assert e.value.status == gpu._n.CIR_EINVAL
        assert os.listdir(str(root)) == []


# ---- 6. no file at all, only empty files, a split context -----------------------------------

def test_no_file_at_all_and_only_empty_files(gpu, ctx64k, tmp_path):
    root = tmp_path / "img"
    root.mkdir()
    stats = {}
    index = ctx64k.store_blocks(str(root), [], 4096, gpu.HashType.blake2b_256(), stats=stats)
    assert index == emit_restate.index_of([], 4096)
    body = index[index.index(b"\n") + 1:-65]
    assert body == b"/\n" and os.listdir(str(root)) == []
    assert stats == dict.fromkeys(gpu.Context.STORE_STATS_FIELDS, 0) | {"body_bytes": 2}
    files = [(b"/d/e1", b"", True), (b"/e0", b"", False)]
    index = ctx64k.store_blocks(str(root), [(p, (0, 0), exe) for p, _, exe in files], 4096,
                                gpu.HashType.blake2b_256(), stats=stats)
    assert index == emit_restate.index_of([(p, exe, 0, []) for p, _, exe in files], 4096)
    check_tree(root, files)
    assert (stats["files"], stats["dirs_made"], stats["batches"], stats["bytes"]) == (2, 1, 0, 0)


def test_split_context_and_the_context_afterwards(gpu, tmp_path):
    """A CIR_DEBUG_SPLIT=3 context (three device states on the one GPU) stores
    through the state that owns the stream's device: the result is the same,
    and the context still answers check_blocks afterwards."""
    import torch
    bs = 512
    src = Sources(torch, tree_files(bs))
    os.environ["CIR_DEBUG_SPLIT"] = "3"
    try:
        ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    finally:
        del os.environ["CIR_DEBUG_SPLIT"]
    try:
        assert len(ctx.devices()) == 3
        root = tmp_path / "img"
        root.mkdir()
        index, _ = check_store(gpu, ctx, bs, "blake2b/256", 4, root, src)
        assert ctx.check_blocks(str(root), index).complete
    finally:
        ctx.close()
