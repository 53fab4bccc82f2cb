"""cir_update_blocks on the GPU: the next version of an image loaded in the
buffers that hold the previous one.

Version N is loaded with load_blocks; N + 1 is then loaded with update_blocks,
its destinations the very tensors that hold N wherever path and size are
unchanged, fresh memory elsewhere.  The reference has no counterpart (it holds
no image in device memory).

No expected value comes from the code under test: the classes are
tests/update_restate.py's over the C oracle's digests of the resident bytes,
by address; verdicts are tests/blocks_restate.py's combined with them; indexes
are dirsig_oracle.scan's; file contents are read from disk here.  Every buffer
of a test lies inside one poisoned allocation with guard bytes (test_gpu_
reload_blocks' Arena), and every byte of that allocation is compared
afterwards.
"""
import os
import random
import time

import numpy as np
import pytest

import dirsig_oracle
import links_restate
import test_gpu_check_blocks as cb
import test_gpu_reload_blocks as rb
import update_restate
from blocks_restate import ABSENT, COMPLETE, PARTIAL
from update_restate import DEMOTED, DIRECT, KEPT, STAGED

pytestmark = pytest.mark.gpu

POISON = rb.POISON
SKIPPED = "skipped"
versions = rb.versions
ctx64k = rb.ctx64k
ctx1m = rb.ctx1m


def _in_place(torch, files_n, files_n1, skip=()):
    """rb.Arena with version N's buffers, and version N + 1's destinations: the
    buffer of the same path where the size is unchanged, fresh memory behind
    the resident buffers otherwise."""
    old = {f[0]: (i, f[2]) for i, f in enumerate(files_n)}
    same = [f[2] and f[0] in old and old[f[0]][1] == f[2] for f in files_n1]
    arena = rb.Arena(torch, [f[2] for f in files_n],
                     [0 if s else f[2] for s, f in zip(same, files_n1)], skip)
    for i, f in enumerate(files_n1):
        if same[i] and i not in skip:
            arena.dest_offs[i] = arena.res_offs[old[f[0]][0]]
            arena.dest_ptrs[i] = arena.res_ptrs[old[f[0]][0]]
    return arena


def _spans(arena):
    return [(o, n) for o, n in zip(arena.res_offs, arena.res_sizes) if o is not None]


def _want(before, arena, index, e, new):
    """The allocation afterwards: what it held, and for every block whose bit
    is set and whose file has a destination the block's bytes of `new`."""
    _, bs, _, _ = dirsig_oracle.parse(index)
    want = before.copy()
    g = 0
    for (path, _, size, digests), off in zip(links_restate.file_entries(index), arena.dest_offs):
        if off is not None and size:
            data = np.frombuffer(rb._file_bytes(new, path), dtype=np.uint8)
            for j in range(len(digests)):
                if e.bits[g + j]:
                    want[off + j * bs:off + min((j + 1) * bs, size)] = data[j * bs:(j + 1) * bs]
        g += len(digests)
    return want


def _update(oracle, ctx, arena, old, index_n, root, index_n1, hname, threads=4, scratch_bytes=None,
            spoil=None):
    """Loads N, restates, updates to N + 1; checks the result against the
    restatement.  Returns (before, got, res, e)."""
    import torch
    before = rb._load_old(ctx, arena, old, index_n)
    if spoil is not None:
        arena.dev[spoil] ^= 0x10
        torch.cuda.synchronize()
        before = arena.host()
    e = update_restate.expected(index_n1, root, before, _spans(arena), arena.dest_offs,
                                rb._digest_fn(oracle, hname), scratch_bytes)
    res = ctx.update_blocks(str(root), index_n1, arena.dest_ptrs, arena.resident(threads),
                            scratch_bytes=scratch_bytes, threads=threads)
    got = arena.host()
    assert update_restate.same(res, e), (res.states, e.states, res.resident, e.resident)
    update_restate.check_stats(res, e)
    return before, got, res, e


def _same_bytes(got, want):
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, diff[:8].tolist()


def _trees(oracle, versions, bs, hname):
    old, new, seen = versions[bs]
    index_n, index_n1 = rb._index(old, bs, hname), rb._index(new, bs, hname)
    return (old, new, seen, index_n, index_n1, links_restate.file_entries(index_n),
            links_restate.file_entries(index_n1))


# ---- 1. the unchanged tree ------------------------------------------------------------------

@pytest.mark.parametrize("bs,hname", [(512, "blake2b/256"), (4096, "blake2b/256"),
                                      (1000, "sha512/256")])
def test_unchanged_tree_is_kept(gpu, oracle, ctx64k, versions, tmp_path, bs, hname):
    """N over N, the files gone from disk: every block is kept, nothing is
    copied, read or written, every non-empty file is complete and resident."""
    import torch
    old, _, _, index_n, _, files_n, _ = _trees(oracle, versions, bs, hname)
    arena = _in_place(torch, files_n, files_n)
    empty = tmp_path / "gone"
    empty.mkdir()
    before, got, res, e = _update(oracle, ctx64k, arena, old, index_n, empty, index_n, hname)
    nblk = sum(len(f[3]) for f in files_n)
    assert [c for c in e.cls] == [KEPT] * nblk
    st = res.stats
    assert (st["kept_blocks"], st["kept_bytes"]) == (nblk, sum(f[2] for f in files_n))
    assert st["copied_blocks"] == st["copied_bytes"] == st["bytes"] == st["staged_blocks"] == 0
    assert st["scratch_bytes"] == st["demoted_blocks"] == 0 and st["resident_blocks"] == nblk
    for f, state, resident in zip(files_n, res.states, res.resident):
        assert (state, resident) == ((COMPLETE, True) if f[2] else (ABSENT, False)), f[0]
    _same_bytes(got, before)


# ---- 2. the changed tree --------------------------------------------------------------------

@pytest.mark.parametrize("bs,hname", [(512, "blake2b/256"), (4096, "blake2b/256"),
                                      (1000, "blake2b/256"), (512, "sha512/256"),
                                      (1000, "sha512/256")])
def test_next_version_in_place(gpu, oracle, ctx64k, ctx1m, versions, bs, hname):
    import torch
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(oracle, versions, bs, hname)
    ordinal = {f[0]: i for i, f in enumerate(files_n1)}
    for ctx, threads in ((ctx64k, 1), (ctx1m, 4), (ctx64k, 0)):
        arena = _in_place(torch, files_n, files_n1)
        before, got, res, e = _update(oracle, ctx, arena, old, index_n, seen, index_n1, hname,
                                      threads)
        assert res.complete and all(e.bits)
        _same_bytes(got, _want(before, arena, index_n1, e, new))
        # the index of what now stands in the destinations is version N + 1's
        listed = [(path, (arena.dest_ptrs[i] or arena.base, size), exe)
                  for i, (path, exe, size, _) in enumerate(files_n1)]
        iid = []
        back = gpu.index_memory(listed, block_size=bs, context=ctx, image_id=iid,
                                hash_type=getattr(gpu.HashType, cb.HASHES[hname])())
        assert back == index_n1
        assert bytes(iid[0]) == gpu.get_hash(index_n1)
    assert ctx64k.check_index(str(new), index_n1).ok       # the context afterwards
    # what the versions were built to show
    cls = lambda path: e.cls[cb.first_block(index_n1, path):][:len(files_n1[ordinal[path]][3])]
    for path in (rb.DELETED, b"/x200k", b"/b1", b"/x1", b"/x17"):
        assert set(cls(path)) == {KEPT} and e.resident[ordinal[path]], path
    assert [j for j, c in enumerate(cls(b"/b130")) if c != KEPT] == [64]     # the flipped block
    assert cls(b"/b130")[64] is None and not e.resident[ordinal[b"/b130"]]
    # a grown, a truncated, a renamed file and a copy get fresh memory: direct copies
    assert cls(b"/b63") == [DIRECT] * 63 + [None]
    assert cls(b"/b65") == [DIRECT] * 40 + [None]
    assert set(cls(b"/sub/moved")) == {DIRECT} and set(cls(b"/copy_mid")) == {DIRECT}
    assert cls(b"/fresh") == [None] * 4
    assert STAGED not in e.cls and DEMOTED not in e.cls
    # bytes read from disk: exactly the blocks that memory did not give
    want_bytes, g = 0, 0
    for path, _, size, digests in files_n1:
        want_bytes += sum(min(bs, size - j * bs) for j in range(len(digests)) if not e.mem[g + j])
        g += len(digests)
    assert e.disk_bytes == want_bytes


# ---- 3. the orders a direct copy gets wrong ---------------------------------------------------

def _pair(tmp_path, bs, hname, old_files, new_files):
    old, new = tmp_path / "n", tmp_path / "n1"
    for root, files in ((old, old_files), (new, new_files)):
        root.mkdir()
        for name, data in files.items():
            (root / name).write_bytes(data)
    return (old, new, dirsig_oracle.scan(str(old), bs, hname),
            dirsig_oracle.scan(str(new), bs, hname))


def _blocks(data, bs):
    return [data[i:i + bs] for i in range(0, len(data), bs)]


def _ordering_case(name, bs):
    """(old files, new files, the expected classes in index order): files of
    nine whole blocks and a tail of 77 bytes."""
    rng = random.Random("%s %d" % (name, bs))
    a, b = rng.randbytes(9 * bs + 77), rng.randbytes(9 * bs + 77)
    blk = _blocks(a, bs)
    if name == "reversed":           # cycles of two; the middle block and the tail stay
        new = b"".join(blk[8::-1]) + blk[9]
        return {"a": a}, {"a": new}, [STAGED] * 4 + [KEPT] + [STAGED] * 4 + [KEPT]
    if name == "swapped":
        s = list(blk)
        s[2], s[6] = s[6], s[2]
        want = [KEPT] * 10
        want[2] = want[6] = STAGED
        return {"a": a}, {"a": b"".join(s)}, want
    if name == "shifted":            # a chain: block j is the old block j - 1
        new = rng.randbytes(bs) + a[:8 * bs + 77]
        return {"a": a}, {"a": new}, [None] + [STAGED] * 8 + [None]
    if name == "exchanged":
        return {"a": a, "b": b}, {"a": b, "b": a}, [STAGED] * 20
    raise KeyError(name)


@pytest.mark.parametrize("bs", [512, 1000])
@pytest.mark.parametrize("name", ["reversed", "swapped", "shifted", "exchanged"])
def test_orders_a_direct_copy_gets_wrong(gpu, oracle, ctx64k, tmp_path, name, bs):
    """Same-size files updated in their own tensors: every moved block's
    destination is another block's source."""
    import torch
    hname = "blake2b/256"
    old_files, new_files, classes = _ordering_case(name, bs)
    old, new, index_n, index_n1 = _pair(tmp_path, bs, hname, old_files, new_files)
    files_n, files_n1 = links_restate.file_entries(index_n), links_restate.file_entries(index_n1)
    arena = _in_place(torch, files_n, files_n1)
    assert arena.dest_offs == arena.res_offs
    before, got, res, e = _update(oracle, ctx64k, arena, old, index_n, new, index_n1, hname)
    assert e.cls == classes
    assert res.complete
    nstaged = classes.count(STAGED)
    assert res.stats["staged_blocks"] == res.stats["copied_blocks"] == nstaged
    want = before.copy()
    for (path, _, size, _), off in zip(files_n1, arena.dest_offs):
        want[off:off + size] = np.frombuffer(new_files[path.lstrip(b"/").decode()], dtype=np.uint8)
    _same_bytes(got, want)


# ---- 4. an overlap by odd bytes ---------------------------------------------------------------

def test_destination_three_bytes_into_the_resident_buffer(gpu, oracle, ctx64k, tmp_path):
    """The same file moved up by three bytes: no block stands on the resident
    grid, so none is kept, and every block lands on resident bytes: all staged."""
    import torch
    bs, hname = 1000, "blake2b/256"
    data = random.Random(5).randbytes(5 * bs + 200)
    old, new, index_n, index_n1 = _pair(tmp_path, bs, hname, {"a": data}, {"a": data})
    arena = rb.Arena(torch, [len(data)], [0])
    arena.dest_offs = [arena.res_offs[0] + 3]
    arena.dest_ptrs = [arena.res_ptrs[0] + 3]
    assert arena.dest_offs[0] + len(data) + 16 <= arena.total
    gone = tmp_path / "gone"
    gone.mkdir()
    before, got, res, e = _update(oracle, ctx64k, arena, old, index_n, gone, index_n1, hname)
    assert e.cls == [STAGED] * 6 and res.resident == [True]
    assert res.stats["scratch_bytes"] == 5 * 16 * 63 + 16 * 13 and res.stats["bytes"] == 0
    want = before.copy()
    off = arena.dest_offs[0]
    want[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    _same_bytes(got, want)


# ---- 5. equal blocks ------------------------------------------------------------------------

def test_zero_filled_file_is_kept_not_moved(gpu, oracle, ctx64k, tmp_path):
    """Every block of a file of zeros matches the join's smallest ordinal,
    block 0; the kept test comes first and nothing is copied."""
    import torch
    bs, hname = 512, "blake2b/256"
    files = {"z": bytes(70 * bs), "zt": bytes(3 * bs + 5)}
    old, new, index_n, index_n1 = _pair(tmp_path, bs, hname, files, files)
    files_n = links_restate.file_entries(index_n)
    arena = _in_place(torch, files_n, files_n)
    gone = tmp_path / "gone"
    gone.mkdir()
    before, got, res, e = _update(oracle, ctx64k, arena, old, index_n, gone, index_n1, hname)
    assert e.cls == [KEPT] * 74 and res.stats["kept_blocks"] == 74
    assert res.stats["copied_blocks"] == res.stats["copied_bytes"] == res.stats["bytes"] == 0
    assert res.resident == [True, True]
    _same_bytes(got, before)


# ---- 6. the cap -----------------------------------------------------------------------------

@pytest.mark.parametrize("scratch_bytes,nstaged", [(0, 0), (3 * 512 + 100, 3), (8 * 512 - 16, 7),
                                                   (8 * 512, 8), (None, 8)])
def test_scratch_cap(gpu, oracle, ctx64k, tmp_path, scratch_bytes, nstaged):
    """The reversed file under a cap: the first k STAGED candidates in block
    order are staged, the rest demoted and read from disk; with the file gone
    from disk the bitmap shows which."""
    import torch
    bs, hname = 512, "blake2b/256"
    old_files, new_files, classes = _ordering_case("reversed", bs)
    old, new, index_n, index_n1 = _pair(tmp_path, bs, hname, old_files, new_files)
    files_n, files_n1 = links_restate.file_entries(index_n), links_restate.file_entries(index_n1)
    cut = [i for i, c in enumerate(classes) if c == STAGED][nstaged:]
    classes = [DEMOTED if i in cut else c for i, c in enumerate(classes)]
    gone = tmp_path / "gone"
    gone.mkdir()
    for root in (new, gone):
        arena = _in_place(torch, files_n, files_n1)
        before, got, res, e = _update(oracle, ctx64k, arena, old, index_n, root, index_n1, hname,
                                      scratch_bytes=scratch_bytes)
        assert e.cls == classes
        st = res.stats
        assert (st["staged_blocks"], st["scratch_bytes"], st["demoted_blocks"]) == \
            (nstaged, nstaged * bs, 8 - nstaged)
        if root is new:              # the demoted blocks came from disk: the same final bytes
            assert res.complete and st["bytes"] == (8 - nstaged) * bs
            want = before.copy()
            off = arena.dest_offs[0]
            want[off:off + len(new_files["a"])] = np.frombuffer(new_files["a"], dtype=np.uint8)
        else:                        # ... or from nowhere: their bits are 0, their bytes untouched
            assert res.states == [ABSENT if nstaged < 8 else COMPLETE] and st["bytes"] == 0
            assert [res.has(g) for g in range(10)] == [0 if c == DEMOTED else 1 for c in classes]
            want = _want(before, arena, index_n1, e, new)
        _same_bytes(got, want)


# ---- 7. memory is not believed --------------------------------------------------------------

@pytest.mark.parametrize("bs", [512, 1000])
def test_corrupted_resident_block_comes_from_disk(gpu, oracle, ctx64k, versions, bs):
    import torch
    hname = "blake2b/256"
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(oracle, versions, bs, hname)
    arena = _in_place(torch, files_n, files_n1)
    victim = [i for i, f in enumerate(files_n) if f[0] == b"/x200k"][0]
    at = arena.res_offs[victim] + 2 * bs + 7          # block 2: unchanged between the versions
    before, got, res, e = _update(oracle, ctx64k, arena, old, index_n, seen, index_n1, hname,
                                  spoil=at)
    i = [i for i, f in enumerate(files_n1) if f[0] == b"/x200k"][0]
    g = cb.first_block(index_n1, b"/x200k")
    nblk = len(files_n1[i][3])
    assert [j for j in range(nblk) if e.cls[g + j] != KEPT] == [2] and e.cls[g + 2] is None
    assert res.states[i] == COMPLETE and not res.resident[i] and res.complete
    _same_bytes(got, _want(before, arena, index_n1, e, new))


# ---- 8. equivalences ------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["env", "empty_list"])
def test_without_memory_it_is_load_blocks(gpu, oracle, ctx64k, versions, mode):
    import torch
    bs, hname = 512, "blake2b/256"
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(oracle, versions, bs, hname)
    arena = rb.Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
    before = rb._load_old(ctx64k, arena, old, index_n)
    if mode == "env":
        os.environ["CIR_UPDATE"] = "disk"
    try:
        res = ctx64k.update_blocks(str(new), index_n1, arena.dest_ptrs,
                                   arena.resident() if mode == "env" else [None, (0, 0)],
                                   threads=4)
    finally:
        os.environ.pop("CIR_UPDATE", None)
    got = arena.host()
    other = rb.Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
    want = ctx64k.load_blocks(str(new), index_n1, other.dest_ptrs, 4)
    assert (res.have, res.states, res.long, res.errnos) == \
        (want.have, want.states, want.long, want.errnos)
    assert not any(res.resident)
    assert [res.stats[k] for k in gpu.Context.LOAD_STATS_FIELDS[:8]] == \
        [want.stats[k] for k in gpu.Context.LOAD_STATS_FIELDS[:8]]
    assert [res.stats[k] for k in gpu.Context.UPDATE_STATS_FIELDS[12:]] == [0] * 10
    lo = min(o for o in arena.dest_offs if o is not None)
    assert (got[lo:] == other.host()[lo:]).all()         # the destinations and their guards
    assert (got[:lo] == before[:lo]).all()               # the resident buffers


def test_with_disjoint_destinations_it_is_reload_blocks(gpu, oracle, ctx64k, versions):
    import torch
    bs, hname = 1000, "blake2b/256"
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(oracle, versions, bs, hname)
    arenas, results = [], []
    for call in ("reload", "update"):
        arena = rb.Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
        rb._load_old(ctx64k, arena, old, index_n)
        fn = ctx64k.reload_blocks if call == "reload" else ctx64k.update_blocks
        results.append(fn(str(seen), index_n1, arena.dest_ptrs, arena.resident(), threads=4))
        arenas.append(arena.host())
    r, u = results
    assert (u.have, u.states, u.long, u.errnos, u.resident) == \
        (r.have, r.states, r.long, r.errnos, r.resident)
    fields = gpu.Context.RELOAD_STATS_FIELDS
    assert [u.stats[k] for k in fields[:8] + fields[9:]] == [r.stats[k] for k in fields[:8] + fields[9:]]
    assert u.stats["kept_blocks"] == u.stats["staged_blocks"] == u.stats["demoted_blocks"] == 0
    assert u.stats["copied_blocks"] > 0 and u.stats["bytes"] > 0
    _same_bytes(arenas[1], arenas[0])


# ---- 9. the rest of reload's contract ---------------------------------------------------------

def test_bad_block_on_disk_and_a_skipped_file(gpu, oracle, ctx1m, versions, tmp_path):
    """One bad block on disk whose content is not resident: bit 0 and partial,
    its neighbours unaffected.  One file without a destination: skipped, and
    its resident buffer still serves as a source and is left as it was."""
    import torch
    bs, hname = 1000, "blake2b/256"
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(oracle, versions, bs, hname)
    ordinal = {f[0]: i for i, f in enumerate(files_n1)}
    root = cb.copy_tree(seen, tmp_path)
    with open(cb.real(root, b"/fresh"), "r+b") as f:
        f.seek(bs + 3)
        f.write(b"\xff\x00\xff")
    skip = {ordinal[b"/x200k"]}
    arena = _in_place(torch, files_n, files_n1, skip)
    assert arena.dest_offs[ordinal[b"/x200k"]] is None
    before, got, res, e = _update(oracle, ctx1m, arena, old, index_n, root, index_n1, hname)
    i = ordinal[b"/fresh"]
    g = cb.first_block(index_n1, b"/fresh")
    assert res.states[i] == PARTIAL and [res.has(g + j) for j in range(4)] == [1, 0, 1, 1]
    assert res.states[ordinal[b"/x200k"]] == SKIPPED
    assert [s for k, s in enumerate(res.states) if k not in (i, ordinal[b"/x200k"])] == \
        [COMPLETE] * (len(files_n1) - 2)
    # everything but the bad block's bytes (unspecified) is the files' or what it was
    want = _want(before, arena, index_n1, e, new)
    off = arena.dest_offs[i]
    want[off + bs:off + 2 * bs] = got[off + bs:off + 2 * bs]
    _same_bytes(got, want)


def test_overlapping_lists_are_refused(gpu, ctx64k, versions):
    """Two destinations that overlap one another, two resident buffers that
    overlap one another: CIR_EINVAL with nothing touched."""
    import torch
    bs, hname = 512, "blake2b/256"
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(None, versions, bs, hname)
    arena = _in_place(torch, files_n, files_n1)
    before = rb._load_old(ctx64k, arena, old, index_n)
    ordinal = {f[0]: i for i, f in enumerate(files_n1)}
    big, small = ordinal[b"/x200k"], ordinal[b"/x17"]
    for shift in (0, 5, files_n1[big][2] - 1):
        ptrs = list(arena.dest_ptrs)
        ptrs[small] = arena.dest_ptrs[big] + shift
        with pytest.raises(gpu.CiruelaError) as err:
            ctx64k.update_blocks(str(seen), index_n1, ptrs, arena.resident(), threads=4)
        assert err.value.status == gpu._n.CIR_EINVAL and "destinations overlap" in str(err.value)
    spans = arena.resident()
    p, n = spans[0]
    for extra in ((p, n), (p + n - 1, 8), (p - 4, 5)):
        with pytest.raises(gpu.CiruelaError) as err:
            ctx64k.update_blocks(str(seen), index_n1, arena.dest_ptrs, spans + [extra], threads=4)
        assert err.value.status == gpu._n.CIR_EINVAL
        assert "resident buffers overlap" in str(err.value)
    assert (arena.host() == before).all()


def test_buffers_are_written_behind_the_callers_stream(gpu, ctx1m, versions):
    """test_gpu_reload_blocks' stream test with an update into fresh
    destinations: one long lane chain on s1 (calibrated here), behind it the
    poison fill of the destinations on s1, then update_blocks(..., stream=s1).
    A copy or a scatter that did not wait for s1 would be overwritten by the
    fill.  The precondition is proven: the event behind the delay is still
    pending immediately before the call."""
    import torch
    lib = gpu._n.lib
    bs, hname = 512, "blake2b/256"
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(None, versions, bs, hname)
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
        arena = rb.Arena(torch, [f[2] for f in files_n], [f[2] for f in files_n1])
        rb._load_old(ctx1m, arena, old, index_n)
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
        res = ctx1m.update_blocks(str(seen), index_n1, arena.dest_ptrs, arena.resident(),
                                  threads=4, stream=s1.cuda_stream)
        got = arena.host()                                 # (the call has returned: no wait needed)
        assert pending, "delay too short: nothing was tested"
        assert res.complete and res.stats["copied_blocks"] > 0 and res.stats["bytes"] > 0
        for (path, _, size, _), off in zip(files_n1, arena.dest_offs):
            if off is not None:
                assert got[off:off + size].tobytes() == rb._file_bytes(new, path), path
    finally:
        torch.cuda.synchronize()


def test_update_image(gpu, ctx1m, versions):
    """update_image with the dict load_image returned: the same tensor where
    path and size agree, a new one elsewhere; the dict itself is left alone."""
    bs, hname = 4096, "blake2b/256"
    old, new, seen, index_n, index_n1, files_n, files_n1 = _trees(None, versions, bs, hname)
    held, res = gpu.load_image(str(old), index_n, context=ctx1m)
    assert res.complete
    keys, ids = list(held), {p: id(t) for p, t in held.items()}
    sizes_n = {f[0]: f[2] for f in files_n}
    tensors, res = gpu.update_image(str(seen), index_n1, held, context=ctx1m)
    assert res.complete and set(tensors) == {f[0] for f in files_n1 if f[2]}
    assert list(held) == keys and {p: id(t) for p, t in held.items()} == ids
    reused = 0
    for path, _, size, _ in files_n1:
        if size:
            assert (tensors[path] is held.get(path)) == (sizes_n.get(path) == size), path
            reused += tensors[path] is held.get(path)
    assert reused >= 8 and b"/b64" not in tensors and b"/sub/mid" not in tensors
    assert res.stats["kept_blocks"] > 0 and res.stats["copied_blocks"] > 0
    assert res.resident[[f[0] for f in files_n1].index(rb.DELETED)]
    for path, t in tensors.items():
        assert t.cpu().numpy().tobytes() == rb._file_bytes(new, path), path
    for path in (b"/b64", b"/sub/mid", b"/b63"):           # vanished or replaced: left as they were
        assert held[path].cpu().numpy().tobytes() == rb._file_bytes(old, path), path
