"""cir_check_links and cir_verify_segments_dev on the GPU.

check_and_hardlink (src/daemon/disk/public.rs:285-346) re-hashes every
hardlink candidate on its own (try_hardlink, :308-346: Error::ReadFile for a
file it cannot open or read, Error::Checksum for one whose blocks or mode bits
differ) and keeps the paths that passed; a bad candidate never affects another
(:303).  cir_check_links gives those verdicts for all candidates in one call.

No expected value comes from the code under test: digests are hashlib's
(oracle/dirsig_oracle.py HASHES), indexes are dirsig_oracle.scan's, expected
candidates and per-candidate verdicts are tests/links_restate.py's, which
walks dirsig_oracle.parse(index) with os.stat(dir_fd=...,
follow_symlinks=False) component by component.
"""
import errno
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import dirsig_oracle
import links_restate
from links_restate import CHECKSUM, OK, READ, expected_verdicts, same_verdicts

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
HASHES = {"blake2b/256": "blake2b_256", "sha512/256": "sha512_256"}


@pytest.fixture(scope="module")
def ctx64k(gpu):
    return gpu.Context(device_mask=1, staging_bytes=64 << 10)


@pytest.fixture(scope="module")
def ctx1m(gpu):
    return gpu.Context(device_mask=1, staging_bytes=1 << 20)


# ---- 1. the kernel's edges through verify_segments_dev ------------------------------

GUARD = 64


def _seg_call(ctx, torch, hasht, d_arena, arena_bytes, d_off, d_len, n, expected, seg_end):
    """One cir_verify_segments_dev call with 0xAA in the flags (and in a guard
    region behind them) and garbage in the count: (flags, guard, count, digests)."""
    nseg = len(seg_end)
    d_exp = torch.tensor(np.frombuffer(bytes(expected) or b"\0" * 32, dtype=np.uint8).copy(),
                         device="cuda:0")
    d_dig = torch.full((32 * max(n, 1),), 0xCD, dtype=torch.uint8, device="cuda:0")
    d_seg = torch.tensor(np.array(list(seg_end) or [0], dtype=np.uint32).view(np.int32),
                         device="cuda:0")
    d_bad = torch.full((nseg + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.full((1,), 999, dtype=torch.int32, device="cuda:0")
    ctx.verify_segments_dev(d_arena.data_ptr() if d_arena is not None else 0, arena_bytes,
                            d_off.data_ptr() if n else 0, d_len.data_ptr() if n else 0, n,
                            d_exp.data_ptr(), d_dig.data_ptr(), d_seg.data_ptr(), nseg,
                            d_bad.data_ptr(), d_cnt.data_ptr(), 0, hasht)
    torch.cuda.synchronize()
    flags = d_bad.cpu().numpy()
    return (flags[:nseg].tolist(), flags[nseg:].tolist(), int(d_cnt.item()) & 0xFFFFFFFF,
            d_dig.cpu().numpy())


def _want_flags(seg_end, bad):
    out, start = [], 0
    for end in seg_end:
        out.append(1 if any(start <= b < end for b in bad) else 0)
        start = end
    return out


def _cuts(nblk, rng):
    """Segment tables over nblk blocks: one segment, one per block, and random
    cuts with a leading, a trailing and several consecutive empty segments and
    an empty segment between two neighbours at nblk // 2."""
    if nblk == 0:
        return [[], [0], [0, 0, 0]]
    m = nblk // 2
    pts = sorted(rng.choices(range(0, nblk + 1), k=min(nblk, 12)) + [m, m])
    return [[nblk], list(range(1, nblk + 1)), [0] + pts + [nblk, nblk, nblk, nblk],
            [0, 0] + sorted(rng.choices(range(0, nblk + 1), k=5)) + [nblk]]


@pytest.mark.parametrize("hname", sorted(HASHES))
@pytest.mark.parametrize("nblk", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_seg_bad_kernel_edges(gpu, ctx1m, nblk, hname):
    import torch
    h = dirsig_oracle.HASHES[hname]
    hasht = getattr(gpu.HashType, HASHES[hname])()
    rng = random.Random(nblk * 5 + len(hname))
    lens = [rng.randrange(0, 201) for _ in range(nblk)]
    offs, pos = [], 0
    for ln in lens:
        offs.append(pos)
        pos += ln
    host = np.frombuffer(rng.randbytes(pos + 64), dtype=np.uint8).copy()
    raw = host.tobytes()
    good = [h(raw[o:o + ln]) for o, ln in zip(offs, lens)]
    d_arena = torch.from_numpy(host).to("cuda:0")
    d_off = torch.tensor(np.array(offs or [0], dtype=np.uint64).view(np.int64), device="cuda:0")
    d_len = torch.tensor(np.array(lens or [0], dtype=np.uint32).view(np.int32), device="cuda:0")

    def flipped(i):
        d = bytearray(good[i])
        d[i % 32] ^= 0x10
        return bytes(d)

    def run(seg_end, bad, arena_bytes=U64):
        exp = [flipped(i) if i in bad else good[i] for i in range(nblk)]
        flags, guard, count, dig = _seg_call(ctx1m, torch, hasht, d_arena, arena_bytes, d_off,
                                             d_len, nblk, b"".join(exp), seg_end)
        want = _want_flags(seg_end, bad)
        assert flags == want, (seg_end, sorted(bad))          # byte for byte, 0xAA overwritten
        assert guard == [0xAA] * GUARD                        # nothing behind the flags
        assert count == sum(want)
        if nblk:  # the digests themselves are the oracle's, whatever is expected
            assert dig.tobytes() == b"".join(good)

    m = nblk // 2
    bad_sets = [set(), set(range(nblk))]
    bad_sets += [{b} for b in sorted({0, nblk - 1, 63, 64, 255, 256, m - 1, m}) if 0 <= b < nblk]
    if nblk >= 3:
        bad_sets.append(set(rng.sample(range(nblk), min(nblk, rng.randrange(2, 40)))))
    for seg_end in _cuts(nblk, rng):
        for bad in bad_sets:
            run(seg_end, bad)
        # through the bounds pass, with every descriptor in range
        run(seg_end, set(), pos)
        run(seg_end, bad_sets[-1], pos)


def test_seg_bad_out_of_range_descriptor(gpu, ctx1m):
    """A descriptor one byte past arena_bytes (inside a larger allocation: only
    the bounds pass shows the bound) marks its own segment and no other."""
    import torch
    h = dirsig_oracle.HASHES["blake2b/256"]
    rng = random.Random(12)
    arena_bytes = 20000
    host = np.frombuffer(rng.randbytes(arena_bytes + 4096), dtype=np.uint8).copy()
    raw = host.tobytes()
    n = 200
    lens = [rng.randrange(0, 90) for _ in range(n)]
    offs = [rng.randrange(0, arena_bytes - 100) for _ in range(n)]
    offs[130], lens[130] = arena_bytes - 10, 11     # one byte past the end
    offs[131], lens[131] = arena_bytes - 10, 10     # the last in-range block
    good = [h(raw[o:o + ln]) for o, ln in zip(offs, lens)]
    d_arena = torch.from_numpy(host).to("cuda:0")
    d_off = torch.tensor(np.array(offs, dtype=np.uint64).view(np.int64), device="cuda:0")
    d_len = torch.tensor(np.array(lens, dtype=np.uint32).view(np.int32), device="cuda:0")
    hasht = gpu.HashType.blake2b_256()
    seg_end = [100, 130, 130, 131, 200]             # block 130 is a segment of its own
    flags, guard, count, dig = _seg_call(ctx1m, torch, hasht, d_arena, arena_bytes, d_off, d_len,
                                         n, b"".join(good), seg_end)
    assert flags == [0, 0, 0, 1, 0] and count == 1 and guard == [0xAA] * GUARD
    dig = dig.reshape(-1, 32)
    assert not dig[130].any() and dig[131].tobytes() == good[131]
    # with the whole allocation as the arena the same batch is clean
    flags, _, count, _ = _seg_call(ctx1m, torch, hasht, d_arena, arena_bytes + 4096, d_off, d_len,
                                   n, b"".join(good), seg_end)
    assert flags == [0] * 5 and count == 0


# ---- 2. trees ------------------------------------------------------------------------------

NSRC = 3


def make_new_tree(root, bs):
    rng = random.Random(bs)
    (root / "sub" / "deep").mkdir(parents=True)
    sizes = {"empty": 0, "one": 1, "bsm1": bs - 1, "bs": bs, "bsp1": bs + 1, "three": 3 * bs,
             "big": 40 * bs + 7, "run.sh": 2 * bs + 5, "with space": 17, "back\\slash": bs // 2,
             "sub/zero": 0, "sub/mid": 2 * bs, "sub/deep/nested": bs + 9}
    for name, size in sizes.items():
        (root / name).write_bytes(rng.randbytes(size))
        os.chmod(root / name, 0o644)
    os.chmod(root / "run.sh", 0o755)


def copy_sources(new, base, n=NSRC):
    roots = []
    for j in range(n):
        r = base / ("src%d" % j)
        shutil.copytree(str(new), str(r), symlinks=True)
        roots.append(r)
    return roots


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """{bs: (new tree, its oracle index)}; the sources are copies of it."""
    out = {}
    for bs in (512, 4096):
        root = tmp_path_factory.mktemp("new%d" % bs) / "img"
        root.mkdir()
        make_new_tree(root, bs)
        out[bs] = (root, dirsig_oracle.scan(str(root), bs))
    return out


def ordinals(index):
    return {path: f for f, (path, _, _, _) in enumerate(links_restate.file_entries(index))}


def all_pairs(index, nsrc=NSRC):
    return [(f, s) for f in range(len(links_restate.file_entries(index))) for s in range(nsrc)]


def real(root, path):
    return os.path.join(os.fsencode(str(root)), path.lstrip(b"/"))


def _flip(root, path, at):
    with open(real(root, path), "r+b") as f:
        f.seek(at)
        c = f.read(1)
        f.seek(at)
        f.write(bytes([c[0] ^ 1]))


def check_against_restatement(contexts, index, roots, links, threads=(1, 4, 0)):
    want = expected_verdicts(index, roots, links)
    want_ok = links_restate.expected_ok_paths(index, roots, links)
    res = None
    for ctx in contexts:
        for t in threads:
            res = ctx.check_links(index, [str(r) for r in roots], links, t)
            assert same_verdicts(res, want), (res.kinds, res.errnos, want)
            assert res.ok_paths == want_ok
            kinds = [k for k, _ in want]
            assert (res.stats["ok"], res.stats["checksum"], res.stats["read"]) == \
                (kinds.count(OK), kinds.count(CHECKSUM), kinds.count(READ))
    return want, res


@pytest.mark.parametrize("hname", sorted(HASHES))
@pytest.mark.parametrize("bs", [512, 4096])
def test_clean_sources_all_ok(gpu, ctx64k, ctx1m, trees, tmp_path, bs, hname):
    new, index = trees[bs]
    if hname != "blake2b/256":
        index = dirsig_oracle.scan(str(new), bs, hname)
    roots = copy_sources(new, tmp_path)
    files = links_restate.file_entries(index)
    # scan_links over three identical older indexes: every file, from the first
    cands, skipped = links_restate.expected_candidates(index, [index] * NSRC)
    assert cands == [(f, 0) for f in range(len(files))] and skipped == 0
    assert gpu.link_candidates(index, [index] * NSRC) == cands
    for links in (cands, [(f, f % NSRC) for f in range(len(files))], all_pairs(index)):
        want, res = check_against_restatement((ctx64k, ctx1m), index, roots, links)
        assert [k for k, _ in want] == [OK] * len(links)
        assert res.ok_paths == {p for p, _, _, _ in files}
        st = res.stats
        assert st["blocks"] == sum(len(files[f][3]) for f, _ in links)
        assert st["bytes"] == sum(files[f][2] for f, _ in links)
        assert st["empty_candidates"] == sum(1 for f, _ in links if files[f][2] == 0)
        assert st["batches"] >= 1 and 1 <= st["peak_fds"]
    # /big at 4096 is 160 KiB: through 64 KiB slots it spans several batches
    if bs == 4096:
        f = ordinals(index)[b"/big"]
        assert ctx64k.check_links(index, [str(roots[0])], [(f, 0)]).stats["batches"] >= 3
    # a root as a directory fd, and relative to one
    fd = os.open(str(roots[1]), os.O_RDONLY | os.O_DIRECTORY)
    pfd = os.open(str(tmp_path), os.O_RDONLY | os.O_DIRECTORY)
    try:
        res = gpu.check_links(index, [str(roots[0]), fd, (pfd, "src2")],
                              [(f, f % NSRC) for f in range(len(files))], context=ctx64k)
        assert res.kinds == [OK] * len(files) and res.errnos == [0] * len(files)
    finally:
        os.close(fd)
        os.close(pfd)
    # no candidates at all
    res = ctx64k.check_links(index, [str(r) for r in roots], [])
    assert res.kinds == [] and res.ok_paths == set() and res.stats["batches"] == 0


# ---- 3. one mutation at a time in one source ---------------------------------------------

def m_flip_first_block(root, bs, out):
    _flip(root, b"/three", 0)
    return {b"/three": CHECKSUM}


def m_flip_last_block(root, bs, out):
    _flip(root, b"/three", 3 * bs - 1)
    return {b"/three": CHECKSUM}


def m_flip_middle_of_multi_batch(root, bs, out):
    _flip(root, b"/big", 20 * bs + 3)
    return {b"/big": CHECKSUM}


def m_truncate_one(root, bs, out):
    os.truncate(real(root, b"/bsp1"), bs)
    return {b"/bsp1": CHECKSUM}


def m_grow_one(root, bs, out):
    with open(real(root, b"/bs"), "ab") as f:
        f.write(b"\0")
    return {b"/bs": CHECKSUM}


def m_mode_0600(root, bs, out):
    os.chmod(real(root, b"/one"), 0o600)
    return {b"/one": CHECKSUM}


def m_exe_made_0644(root, bs, out):
    os.chmod(real(root, b"/run.sh"), 0o644)
    return {b"/run.sh": CHECKSUM}


def m_empty_made_nonempty(root, bs, out):
    with open(real(root, b"/empty"), "wb") as f:
        f.write(b"x")
    return {b"/empty": CHECKSUM}


def m_missing(root, bs, out):
    os.unlink(real(root, b"/bsm1"))
    return {b"/bsm1": (READ, errno.ENOENT)}


def m_empty_missing(root, bs, out):
    os.unlink(real(root, b"/sub/zero"))
    return {b"/sub/zero": (READ, errno.ENOENT)}


def m_symlink_to_identical_bytes(root, bs, out):
    shutil.move(os.fsdecode(real(root, b"/with space")), str(out / "moved"))
    os.symlink(str(out / "moved"), real(root, b"/with space"))
    return {b"/with space": READ}


def m_replaced_by_directory(root, bs, out):
    os.unlink(real(root, b"/back\\slash"))
    os.mkdir(real(root, b"/back\\slash"))
    return {b"/back\\slash": READ}


def m_parent_replaced_by_symlink(root, bs, out):
    shutil.move(os.fsdecode(real(root, b"/sub")), str(out / "moved_sub"))
    os.symlink(str(out / "moved_sub"), real(root, b"/sub"))
    return {b"/sub/zero": READ, b"/sub/mid": READ, b"/sub/deep/nested": READ}


MUTATIONS = [m_flip_first_block, m_flip_last_block, m_flip_middle_of_multi_batch, m_truncate_one,
             m_grow_one, m_mode_0600, m_exe_made_0644, m_empty_made_nonempty, m_missing,
             m_empty_missing, m_symlink_to_identical_bytes, m_replaced_by_directory,
             m_parent_replaced_by_symlink]


def _expect(index, links, victims, src):
    """The table's row as a verdict vector: the victims under source `src`,
    every other candidate OK."""
    files = links_restate.file_entries(index)
    out = []
    for f, s in links:
        v = victims.get(files[f][0]) if s == src else None
        out.append(OK if v is None else v[0] if isinstance(v, tuple) else v)
    return out


@pytest.mark.parametrize("bs", [512, 4096])
@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda m: m.__name__[2:])
def test_one_mutation_in_one_source(ctx64k, ctx1m, trees, tmp_path, mutate, bs):
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path)
    out = tmp_path / "outside"
    out.mkdir()
    victims = mutate(roots[1], bs, out)
    links = all_pairs(index)
    want, res = check_against_restatement((ctx64k, ctx1m), index, roots, links, threads=(1, 4))
    # the restatement gives the table's row: only that candidate changed
    assert [k for k, _ in want] == _expect(index, links, victims, 1)
    for (f, s), (k, e), got in zip(links, want, res.errnos):
        v = victims.get(links_restate.file_entries(index)[f][0]) if s == 1 else None
        if isinstance(v, tuple):
            assert e == v[1] and got == v[1]


@pytest.mark.parametrize("bs", [512, 4096])
def test_missing_source_root(ctx64k, ctx1m, trees, tmp_path, bs):
    """A root that does not open makes READ of its candidates and of no
    others; the call itself succeeds."""
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path)
    os.rename(str(roots[1]), str(tmp_path / "gone"))
    links = all_pairs(index)
    want, res = check_against_restatement((ctx64k, ctx1m), index, roots, links, threads=(1, 4))
    assert [k for k, _ in want] == [READ if s == 1 else OK for _, s in links]
    assert [e for e in res.errnos] == [errno.ENOENT if s == 1 else 0 for _, s in links]
    # a root that is a file
    (tmp_path / "src1").write_bytes(b"not a directory")
    res = ctx64k.check_links(index, [str(r) for r in roots], links)
    assert res.kinds == [READ if s == 1 else OK for _, s in links]


# ---- 4. other shapes ----------------------------------------------------------------------

def test_several_mutations_across_sources(ctx64k, ctx1m, trees, tmp_path):
    bs = 4096
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path)
    out = tmp_path / "outside"
    out.mkdir()
    m_flip_middle_of_multi_batch(roots[0], bs, out)
    m_missing(roots[0], bs, out)
    m_exe_made_0644(roots[1], bs, out)
    m_parent_replaced_by_symlink(roots[1], bs, out)
    m_truncate_one(roots[2], bs, out)
    m_empty_made_nonempty(roots[2], bs, out)
    _flip(roots[2], b"/big", 40 * bs + 6)            # the last byte of the short tail
    links = all_pairs(index)
    want, _ = check_against_restatement((ctx64k, ctx1m), index, roots, links)
    kinds = [k for k, _ in want]
    assert kinds.count(CHECKSUM) == 5 and kinds.count(READ) == 4
    # the same candidates in another order: the same verdict for each
    rng = random.Random(4)
    shuffled = list(links)
    rng.shuffle(shuffled)
    want2, _ = check_against_restatement((ctx64k,), index, roots, shuffled, threads=(3,))
    assert dict(zip(shuffled, want2)) == dict(zip(links, want))


def test_same_file_from_two_sources_one_bad(ctx64k, trees, tmp_path):
    bs = 512
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path)
    f = ordinals(index)[b"/big"]
    _flip(roots[1], b"/big", 7 * bs)
    links = [(f, 0), (f, 1), (f, 1), (f, 2), (f, 0)]
    want, res = check_against_restatement((ctx64k,), index, roots, links)
    assert res.kinds == [OK, CHECKSUM, CHECKSUM, OK, OK]
    assert res.ok_paths == {b"/big"}                 # it passed somewhere
    assert res.stats["blocks"] == 5 * 41


def test_unsorted_link_file(ctx64k, ctx1m, trees, tmp_path):
    bs = 512
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path)
    _flip(roots[2], b"/three", bs + 1)
    os.unlink(real(roots[0], b"/one"))
    links = all_pairs(index)
    links.sort(key=lambda fs: (-fs[0], fs[1]))       # file ordinals descending
    want, res = check_against_restatement((ctx64k, ctx1m), index, roots, links)
    assert res.kinds.count(CHECKSUM) == 1 and res.kinds.count(READ) == 1


def test_striped_devices(gpu, trees, tmp_path):
    """Three device states on the one GPU (CIR_DEBUG_SPLIT=3), stripes of 4
    blocks dealt round-robin: a candidate's blocks lie on several devices and
    its verdict is OR-ed on the host; the verdicts are those of one device."""
    bs = 512
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path)
    out = tmp_path / "outside"
    out.mkdir()
    os.environ["CIR_DEBUG_SPLIT"] = "3"
    try:
        ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    finally:
        del os.environ["CIR_DEBUG_SPLIT"]
    assert len(ctx.devices()) == 3

    def check(links, threads):
        os.environ["CIR_DEBUG_STRIPE_BLOCKS"] = "4"
        try:
            return ctx.check_links(index, [str(r) for r in roots], links, threads)
        finally:
            del os.environ["CIR_DEBUG_STRIPE_BLOCKS"]

    links = all_pairs(index)
    files = links_restate.file_entries(index)
    res = check(links, 4)
    assert res.kinds == [OK] * len(links)
    assert res.stats["blocks"] == sum(len(files[f][3]) for f, _ in links)
    assert res.stats["bytes"] == sum(files[f][2] for f, _ in links)
    _flip(roots[0], b"/big", 33 * bs)                # one block of 41, on one device's stripe
    _flip(roots[1], b"/three", 2 * bs)
    m_missing(roots[2], bs, out)
    m_mode_0600(roots[2], bs, out)
    m_parent_replaced_by_symlink(roots[0], bs, out)
    want = expected_verdicts(index, roots, links)
    assert sorted({k for k, _ in want}) == sorted([OK, CHECKSUM, READ])
    for rep in range(4):
        assert same_verdicts(check(links, 1 + rep), want), rep
    ctx.close()


def test_fd_bound_with_thousands_of_candidates(ctx1m, tmp_path):
    """2,000 one-block candidates of 512 B fill batches of hundreds of files;
    the check holds the roots and O(reader threads) descriptors, not one per
    candidate.  From the code (check.cpp): the roots a candidate names (2),
    the packer's directory and the file it is looking at (2), and per reader
    its directory and its file (2 x threads)."""
    rng = random.Random(9)
    d = tmp_path / "new" / "many"
    d.mkdir(parents=True)
    blob = rng.randbytes(512 + 2000)
    for i in range(2000):
        with open(d / ("f%04d" % i), "wb") as f:
            f.write(blob[i:i + 512])
    index = dirsig_oracle.scan(str(tmp_path / "new"), 512)
    roots = copy_sources(tmp_path / "new", tmp_path, 2)
    links = [(f, f % 2) for f in range(2000)]
    threads = 4
    res = ctx1m.check_links(index, [str(r) for r in roots], links, threads)
    assert res.kinds == [OK] * 2000
    assert res.stats["blocks"] == 2000 and res.stats["bytes"] == 2000 * 512
    assert res.stats["batches"] <= 12                # hundreds of candidates per batch
    assert 1 <= res.stats["peak_fds"] <= 2 + 2 + 2 * threads
    # a flipped byte deep inside such a batch is found, at its candidate alone
    _flip(roots[1], b"/many/f1357", 100)
    res = ctx1m.check_links(index, [str(r) for r in roots], links, threads)
    assert res.kinds == [CHECKSUM if f == 1357 else OK for f, _ in links]


def test_context_is_healthy_after_bad_verdicts(gpu, trees, tmp_path):
    bs = 4096
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path)
    ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    _flip(roots[0], b"/big", 5)
    os.unlink(real(roots[1], b"/three"))
    links = all_pairs(index)
    want = expected_verdicts(index, roots, links)
    assert {k for k, _ in want} == {OK, CHECKSUM, READ}
    assert same_verdicts(ctx.check_links(index, [str(r) for r in roots], links), want)
    assert ctx.check_index(str(new), index).ok
    assert ctx.check_index(str(roots[2]), index).ok
    res = ctx.check_index(str(roots[0]), index)
    assert (res.kind, res.path) == (CHECKSUM, b"/big")
    assert same_verdicts(ctx.check_links(index, [str(r) for r in roots], links), want)
    ctx.close()


def test_parse_errors(gpu, ctx64k, trees):
    new, index = trees[512]
    n = gpu._n

    def status(ix, links=((0, 0),)):
        with pytest.raises(gpu.CiruelaError) as e:
            ctx64k.check_links(ix, [str(new)], list(links))
        return e.value.status

    assert status(index[:len(index) // 2]) == n.CIR_EPARSE
    assert status(b"") == n.CIR_EPARSE
    assert status(index, [(len(links_restate.file_entries(index)), 0)]) == n.CIR_EINVAL
    assert status(index, [(0, 1)]) == n.CIR_EINVAL
    assert ctx64k.check_links(index, [str(new)], [(0, 0)]).kinds == [OK]


# ---- 5. randomised ----------------------------------------------------------------------------

RANDOM_MUTATIONS = ["none", "flip", "truncate_one", "grow_one", "delete", "mode_0600", "mode_0755",
                    "file_to_symlink", "file_to_dir", "dir_to_symlink", "empty_gets_a_byte",
                    "empty_deleted", "root_missing"]


def _random_case(seed, base):
    rng = random.Random(seed)
    bs = rng.choice([512, 4096])
    new = base / "new"
    dirs = [new] + [new / ("d%d" % i) for i in range(rng.randrange(0, 4))]
    dirs += [dirs[-1] / "sub"] if len(dirs) > 1 and rng.random() < 0.5 else []
    for d in dirs:
        d.mkdir(parents=True, exist_ok=True)
    for i in range(rng.randrange(1, 31)):
        nb = rng.randrange(0, 4)
        size = 0 if nb == 0 else rng.choice([nb * bs, (nb - 1) * bs + rng.randrange(1, bs)])
        p = rng.choice(dirs) / ("f%02d" % i)
        p.write_bytes(rng.randbytes(size))
        os.chmod(p, 0o755 if rng.random() < 0.2 else 0o644)
    hname = rng.choice(sorted(HASHES))
    index = dirsig_oracle.scan(str(new), bs, hname)
    nsrc = rng.randrange(1, 4)
    roots = copy_sources(new, base, nsrc)
    files = links_restate.file_entries(index)
    out = base / "outside"
    out.mkdir()
    done = []
    for k in range(rng.randrange(0, 4)):
        kind = RANDOM_MUTATIONS[(seed + 5 * k) % len(RANDOM_MUTATIONS)]
        root = rng.choice(roots)
        path, _, size, _ = rng.choice(files)
        p = real(root, path)
        if not os.path.isdir(str(root)) or os.path.islink(p) or not os.path.isfile(p):
            continue  # already mutated away
        if kind == "flip" and size:
            _flip(root, path, rng.randrange(size))
        elif kind == "truncate_one" and size:
            os.truncate(p, size - 1)
        elif kind == "grow_one" and size:
            with open(p, "ab") as f:
                f.write(b"\0")
        elif kind == "delete" and size:
            os.unlink(p)
        elif kind == "mode_0600":
            os.chmod(p, 0o600)
        elif kind == "mode_0755":
            os.chmod(p, 0o755)
        elif kind == "file_to_symlink":
            shutil.move(os.fsdecode(p), str(out / ("moved%d" % k)))
            os.symlink(str(out / ("moved%d" % k)), p)
        elif kind == "file_to_dir":
            os.unlink(p)
            os.mkdir(p)
        elif kind == "dir_to_symlink" and path.count(b"/") > 1:
            d = os.path.dirname(p)
            if not os.path.islink(d):
                shutil.move(os.fsdecode(d), str(out / ("moved_dir%d" % k)))
                os.symlink(str(out / ("moved_dir%d" % k)), d)
        elif kind == "empty_gets_a_byte" and size == 0:
            with open(p, "wb") as f:
                f.write(b"x")
        elif kind == "empty_deleted" and size == 0:
            os.unlink(p)
        elif kind == "root_missing" and nsrc > 1:
            os.rename(str(root), str(base / ("gone%d" % k)))
        done.append(kind)
    links = [(f, s) for f in range(len(files)) for s in range(nsrc)]
    rng.shuffle(links)
    return index, roots, links[:rng.randrange(0, len(links) + 1)], done


@pytest.mark.parametrize("seed", range(20))
def test_random_trees_and_mutations(ctx64k, ctx1m, tmp_path, seed):
    index, roots, links, done = _random_case(seed, tmp_path)
    ctx = ctx64k if seed % 2 else ctx1m
    want = expected_verdicts(index, roots, links)
    res = ctx.check_links(index, [str(r) for r in roots], links, 1 + seed % 4)
    assert same_verdicts(res, want), (done, res.kinds, res.errnos, want)
    assert res.ok_paths == links_restate.expected_ok_paths(index, roots, links)


# ---- 6. the CLI ------------------------------------------------------------------------------------

def _escaped_paths(index):
    """The file entries' paths as the index spells them, in index order."""
    _, _, dirs, _ = dirsig_oracle.parse(index)
    return [(b"" if vesc == b"/" else vesc) + b"/" + e[1]
            for vesc, entries in dirs for e in entries if e[0] == "f"]


def test_cli_links(trees, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    bs = 4096
    new, index = trees[bs]
    roots = copy_sources(new, tmp_path, 2)
    # the first older image differs in one file, so that file comes from the second
    with open(real(roots[0], b"/three"), "r+b") as f:
        f.write(b"another version")
    src_index = [dirsig_oracle.scan(str(r), bs) for r in roots]
    # after the indexes were written: a file rots in the first, one goes missing
    _flip(roots[0], b"/big", 9 * bs)
    os.unlink(real(roots[0], b"/back\\slash"))
    paths = []
    for name, data in [("new.ds1", index), ("s0.ds1", src_index[0]), ("s1.ds1", src_index[1])]:
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    cands, skipped = links_restate.expected_candidates(index, src_index)
    assert skipped == 0 and (ordinals(index)[b"/three"], 1) in cands
    want = expected_verdicts(index, roots, cands)
    assert [k for k, _ in want].count(CHECKSUM) == 1 and [k for k, _ in want].count(READ) == 1
    esc = _escaped_paths(index)
    lines = {os.fsencode(str(roots[s])) + b"\t" + esc[f]
             for (f, s), (k, _) in zip(cands, want) if k == OK}
    assert any(b"with\\x20space" in ln for ln in lines)
    p = subprocess.run([cli, "links", paths[0], "%s=%s" % (roots[0], paths[1]),
                        "%s=%s" % (roots[1], paths[2]), "--disk-threads", "2"],
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.split(b"\n")
    assert got[-1] == b"" and len(got) - 1 == len(lines) and set(got[:-1]) == lines
    assert b"%d candidates: %d ok, 1 checksum, 1 read" % (len(cands), len(lines)) in p.stderr
    # an index that does not parse: exit 2, nothing on stdout
    (tmp_path / "new.ds1").write_bytes(index[:100])
    p = subprocess.run([cli, "links", paths[0], "%s=%s" % (roots[0], paths[1])],
                       capture_output=True, timeout=120)
    assert p.returncode == 2 and p.stdout == b""
