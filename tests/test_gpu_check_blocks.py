"""cir_check_blocks and cir_verify_bitmap_dev on the GPU.

The reference resumes an unfinished image by starting over: "Resuming
download" (src/daemon/tracking/mod.rs:561-585) goes through start_image, which
removes the partial directory (src/daemon/disk/public.rs:91-93), and
fill_blocks queues every block again (src/daemon/tracking/progress.rs:129-170).
cir_check_blocks answers, for the directory as it stands, which blocks of the
index are present and correct: one bit per block, one state per file.

No expected value comes from the code under test: digests are hashlib's
(oracle/dirsig_oracle.py HASHES), indexes are dirsig_oracle.scan's, and the
expected bitmaps, states and missing lists are tests/blocks_restate.py's, which
walks dirsig_oracle.parse(index) with os.stat(dir_fd=...,
follow_symlinks=False) component by component and reads the files itself.
"""
import errno
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import blocks_restate
import dirsig_oracle
import links_restate
from blocks_restate import ABSENT, BLOCKED, COMPLETE, PARTIAL

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
HASHES = {"blake2b/256": "blake2b_256", "sha512/256": "sha512_256"}
SENTINEL = 0xA5A5A5A5A5A5A5A5
GUARD = 8  # sentinel words behind the bitmap


@pytest.fixture(scope="module")
def ctx64k(gpu):
    return gpu.Context(device_mask=1, staging_bytes=64 << 10)


@pytest.fixture(scope="module")
def ctx1m(gpu):
    return gpu.Context(device_mask=1, staging_bytes=1 << 20)


# ---- 1. the kernel's edges through verify_bitmap_dev --------------------------------

def _bitmap_call(ctx, torch, hasht, d_arena, arena_bytes, d_off, d_len, n, expected,
                 count_before=999):
    """One cir_verify_bitmap_dev call with the sentinel in every word of the
    bitmap and behind it, and `count_before` in the count: (words, guard,
    count, digests)."""
    nw = (n + 63) // 64
    d_exp = torch.tensor(np.frombuffer(bytes(expected) or b"\0" * 32, dtype=np.uint8).copy(),
                         device="cuda:0")
    d_dig = torch.full((32 * max(n, 1),), 0xCD, dtype=torch.uint8, device="cuda:0")
    d_have = torch.tensor(np.full(nw + GUARD, SENTINEL, dtype=np.uint64).view(np.int64),
                          device="cuda:0")
    d_cnt = torch.full((1,), count_before, dtype=torch.int32, device="cuda:0")
    ctx.verify_bitmap_dev(d_arena.data_ptr() if d_arena is not None else 0, arena_bytes,
                          d_off.data_ptr() if n else 0, d_len.data_ptr() if n else 0, n,
                          d_exp.data_ptr(), d_dig.data_ptr(), d_have.data_ptr(), d_cnt.data_ptr(),
                          0, hasht)
    torch.cuda.synchronize()
    words = d_have.cpu().numpy().view(np.uint64)
    return (words[:nw].tolist(), words[nw:].tolist(), int(d_cnt.item()) & 0xFFFFFFFF,
            d_dig.cpu().numpy())


def _want_words(n, bad):
    """The bitmap of n blocks of which `bad` do not match, tail bits 0."""
    words = [0] * ((n + 63) // 64)
    for b in range(n):
        if b not in bad:
            words[b >> 6] |= 1 << (b & 63)
    return words


@pytest.mark.parametrize("hname", sorted(HASHES))
@pytest.mark.parametrize("nblk", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_block_bits_kernel_edges(gpu, ctx1m, nblk, hname):
    """The wave (64), word (64) and workgroup (256) boundaries of k_block_bits:
    the bitmap is the oracle's, the last word's tail bits are 0, the word
    behind the last is untouched, and the count is right whatever it held."""
    import torch
    h = dirsig_oracle.HASHES[hname]
    hasht = getattr(gpu.HashType, HASHES[hname])()
    rng = random.Random(nblk * 7 + len(hname))
    lens = [rng.randrange(100, 701) for _ in range(nblk)]
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

    def run(bad, arena_bytes=U64, count_before=999):
        exp = [flipped(i) if i in bad else good[i] for i in range(nblk)]
        words, guard, count, dig = _bitmap_call(ctx1m, torch, hasht, d_arena, arena_bytes, d_off,
                                                d_len, nblk, b"".join(exp), count_before)
        assert words == _want_words(nblk, bad), sorted(bad)   # every word written, tail bits 0
        assert guard == [SENTINEL] * GUARD                    # nothing behind the last word
        assert count == len(bad)
        if nblk:  # the digests themselves are the oracle's, whatever is expected
            assert dig.tobytes() == b"".join(good)

    # none, every block, lane 0 and lane 63 of each wave edge, the first and the last block
    bad_sets = [set(), set(range(nblk))]
    bad_sets += [{b} for b in sorted({0, 63, 64, 127, 128, 192, 255, 256, nblk - 64, nblk - 1})
                 if 0 <= b < nblk]
    bad_sets.append({b for b in range(nblk) if b % 64 == 0})     # lane 0 of every wave
    bad_sets.append({b for b in range(nblk) if b % 64 == 63})    # lane 63 of every wave
    if nblk >= 3:
        bad_sets.append(set(rng.sample(range(nblk), min(nblk, rng.randrange(2, 40)))))
    for bad in bad_sets:
        run(bad)
    # the count when it held something else beforehand, and zero
    run(bad_sets[-1], count_before=0)
    run(bad_sets[-1], count_before=-1)
    # through the bounds pass, with every descriptor in range
    run(set(), pos)
    run(bad_sets[-1], pos)


def test_block_bits_out_of_range_descriptors(gpu, ctx1m):
    """Descriptors that leave the arena -- one byte past its end (inside a
    larger allocation: only the bounds pass shows the bound) and one whose
    off + len wraps around 2^64 -- are never read and their bits are 0; every
    other bit is the oracle's.  Every buffer passed is valid."""
    import torch
    h = dirsig_oracle.HASHES["blake2b/256"]
    rng = random.Random(21)
    arena_bytes = 20000
    host = np.frombuffer(rng.randbytes(arena_bytes + 4096), dtype=np.uint8).copy()
    raw = host.tobytes()
    n = 200
    lens = [rng.randrange(100, 701) for _ in range(n)]
    offs = [rng.randrange(0, arena_bytes - 800) for _ in range(n)]
    offs[130], lens[130] = arena_bytes - 10, 11     # one byte past the end
    offs[131], lens[131] = arena_bytes - 10, 10     # the last in-range block
    offs[64], lens[64] = U64 - 15, 100              # off + len wraps around 2^64
    out = {130, 64}
    good = [b"\0" * 32 if i in out else h(raw[o:o + ln])
            for i, (o, ln) in enumerate(zip(offs, lens))]
    d_arena = torch.from_numpy(host).to("cuda:0")
    d_off = torch.tensor(np.array(offs, dtype=np.uint64).view(np.int64), device="cuda:0")
    d_len = torch.tensor(np.array(lens, dtype=np.uint32).view(np.int32), device="cuda:0")
    hasht = gpu.HashType.blake2b_256()
    # expected digests: the true ones where in range, so only the range flags clear bits
    exp = [h(raw[arena_bytes - 10:arena_bytes + 1]) if i == 130 else good[i] for i in range(n)]
    words, guard, count, dig = _bitmap_call(ctx1m, torch, hasht, d_arena, arena_bytes, d_off,
                                            d_len, n, b"".join(exp))
    assert words == _want_words(n, out) and count == 2 and guard == [SENTINEL] * GUARD
    dig = dig.reshape(-1, 32)
    assert not dig[130].any() and not dig[64].any() and dig[131].tobytes() == good[131]
    # an expected digest of zeros does not make an out-of-range block "have"
    words, _, count, _ = _bitmap_call(ctx1m, torch, hasht, d_arena, arena_bytes, d_off, d_len, n,
                                      b"".join(good))
    assert words == _want_words(n, out) and count == 2


# ---- 2. trees ------------------------------------------------------------------------------

def sizes_for(bs):
    """Files of 0, 1, 63, 64, 65 and 130 blocks, with ragged and whole last
    blocks; 323 + a few blocks in all."""
    return {"b1": bs // 2 + 1, "b130": 129 * bs + bs - 1, "b63": 63 * bs, "b64": 63 * bs + 7,
            "b65": 65 * bs, "empty": 0, "with space": 17, "back\\slash": bs,
            "sub/zero": 0, "sub/mid": 2 * bs, "sub/deep/nested": bs + 9,
            "zeros": 4 * bs}


def make_tree(root, bs):
    rng = random.Random(bs + 1)
    (root / "sub" / "deep").mkdir(parents=True)
    for name, size in sizes_for(bs).items():
        data = rng.randbytes(size)
        if name == "zeros":  # blocks 1 and 2 are all zeros, 0 and 3 are not
            data = data[:bs] + b"\0" * (2 * bs) + data[3 * bs:]
        (root / name).write_bytes(data)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """{bs: (complete tree, its oracle index)}; the tests mutate copies."""
    out = {}
    for bs in (512, 4096):
        root = tmp_path_factory.mktemp("img%d" % bs) / "img"
        root.mkdir()
        make_tree(root, bs)
        out[bs] = (root, dirsig_oracle.scan(str(root), bs))
    return out


def copy_tree(src, base, name=".tmp.img"):
    dst = base / name
    shutil.copytree(str(src), str(dst), symlinks=True)
    return dst


def real(root, path):
    return os.path.join(os.fsencode(str(root)), path.lstrip(b"/"))


def ordinals(index):
    return {path: f for f, (path, _, _, _) in enumerate(links_restate.file_entries(index))}


def first_block(index, path):
    g = 0
    for p, _, _, digests in links_restate.file_entries(index):
        if p == path:
            return g
        g += len(digests)
    raise KeyError(path)


def _flip(root, path, at):
    with open(real(root, path), "r+b") as f:
        f.seek(at)
        c = f.read(1)
        f.seek(at)
        f.write(bytes([c[0] ^ 1]))


def check_against_restatement(contexts, index, root, threads=(1, 4, 0)):
    """The result equals the restatement's on every context and thread count,
    its stats add up, and the invariant with check_index holds."""
    want = blocks_restate.expected(index, root)
    bits, states, longs, _ = want
    files = links_restate.file_entries(index)
    res = None
    for ctx in contexts:
        for t in threads:
            res = ctx.check_blocks(str(root), index, t)
            assert blocks_restate.same(res, want), (res, res.states, res.errnos, want[1:])
            assert res.missing() == blocks_restate.expected_missing(index, bits)
            st = res.stats
            assert (st["have"], st["missing"]) == (sum(bits), len(bits) - sum(bits))
            assert [st[s] for s in (COMPLETE, ABSENT, PARTIAL, BLOCKED)] == \
                [states.count(s) for s in (COMPLETE, ABSENT, PARTIAL, BLOCKED)]
            assert res.complete == all(s == COMPLETE for s in states)
            assert st["unread_blocks"] <= st["missing"] and st["peak_fds"] >= 1
        # the invariant: check_index passes exactly when every non-empty file is
        # complete and every size-0 file complete or absent
        assert ctx.check_index(str(root), index).ok == blocks_restate.check_index_ok(index, states)
    assert len(files) == len(states)
    return want, res


@pytest.mark.parametrize("bs,hname", [(512, "blake2b/256"), (4096, "blake2b/256"),
                                      (512, "sha512/256")])
def test_complete_tree(gpu, ctx64k, ctx1m, trees, bs, hname):
    root, index = trees[bs]
    if hname != "blake2b/256":
        index = dirsig_oracle.scan(str(root), bs, hname)
    want, res = check_against_restatement((ctx64k, ctx1m), index, root)
    bits, states, longs, errnos = want
    files = links_restate.file_entries(index)
    assert all(bits) and states == [COMPLETE] * len(files) and not any(longs)
    assert res.complete and res and res.missing() == []
    assert res.nblk == sum(len(f[3]) for f in files)
    assert res.stats["bytes"] == sum(f[2] for f in files) and res.stats["unread_blocks"] == 0
    assert ctx64k.check_index(str(root), index).ok
    # 64 KiB slots: many batches, with runs that start off word boundaries
    many = ctx64k.check_blocks(str(root), index).stats["batches"]
    assert many >= (4 if bs == 512 else 20)
    # the root as a directory fd, and relative to one; the module-level call
    fd = os.open(str(root), os.O_RDONLY | os.O_DIRECTORY)
    pfd = os.open(str(root.parent), os.O_RDONLY | os.O_DIRECTORY)
    try:
        assert blocks_restate.same(ctx64k.check_blocks(None, index, dir_fd=fd), want)
        assert blocks_restate.same(gpu.check_blocks("img", index, dir_fd=pfd, context=ctx1m), want)
    finally:
        os.close(fd)
        os.close(pfd)
    with pytest.raises(gpu.CiruelaError) as e:
        ctx64k.check_blocks(str(root / "nowhere"), index)
    assert e.value.status == gpu._n.CIR_EIO


# ---- 3. one mutation at a time ----------------------------------------------------------
# Each returns {path: (state, long, the blocks of the file that are lost)}.

def m_flip_first_block(root, bs, out):
    _flip(root, b"/b130", 0)
    return {b"/b130": (PARTIAL, False, [0])}


def m_flip_middle_block(root, bs, out):
    _flip(root, b"/b130", 70 * bs + 3)
    return {b"/b130": (PARTIAL, False, [70])}


def m_flip_last_block(root, bs, out):
    _flip(root, b"/b130", 130 * bs - 2)
    return {b"/b130": (PARTIAL, False, [129])}


def m_flip_last_block_of_b64(root, bs, out):
    _flip(root, b"/b64", 63 * bs + 6)
    return {b"/b64": (PARTIAL, False, [63])}


def m_truncate_to_block_boundary(root, bs, out):
    os.truncate(real(root, b"/b65"), 40 * bs)
    return {b"/b65": (PARTIAL, False, list(range(40, 65)))}


def m_truncate_mid_block(root, bs, out):
    os.truncate(real(root, b"/b65"), 40 * bs + bs // 3)
    return {b"/b65": (PARTIAL, False, list(range(40, 65)))}


def m_truncate_ragged_last_block_by_one(root, bs, out):
    os.truncate(real(root, b"/b64"), 63 * bs + 6)
    return {b"/b64": (PARTIAL, False, [63])}


def m_truncate_to_zero(root, bs, out):
    os.truncate(real(root, b"/b63"), 0)
    return {b"/b63": (PARTIAL, False, list(range(63)))}


def m_grow_by_one_byte(root, bs, out):
    with open(real(root, b"/b63"), "ab") as f:
        f.write(b"\0")
    return {b"/b63": (PARTIAL, True, [])}


def m_grow_ragged_by_a_block(root, bs, out):
    with open(real(root, b"/b1"), "ab") as f:
        f.write(b"x" * bs)
    return {b"/b1": (PARTIAL, True, [])}


def m_missing_file(root, bs, out):
    os.unlink(real(root, b"/b64"))
    return {b"/b64": (ABSENT, False, list(range(64)))}


def m_missing_directory(root, bs, out):
    shutil.rmtree(os.fsdecode(real(root, b"/sub")))
    return {b"/sub/zero": (ABSENT, False, []), b"/sub/mid": (ABSENT, False, [0, 1]),
            b"/sub/deep/nested": (ABSENT, False, [0, 1])}


def m_directory_in_its_place(root, bs, out):
    os.unlink(real(root, b"/back\\slash"))
    os.mkdir(real(root, b"/back\\slash"))
    return {b"/back\\slash": (BLOCKED, False, [0])}


def m_symlink_to_identical_bytes(root, bs, out):
    shutil.move(os.fsdecode(real(root, b"/with space")), str(out / "moved"))
    os.symlink(str(out / "moved"), real(root, b"/with space"))
    return {b"/with space": (BLOCKED, False, [0])}


def m_fifo_in_its_place(root, bs, out):
    os.unlink(real(root, b"/sub/mid"))
    os.mkfifo(real(root, b"/sub/mid"))
    return {b"/sub/mid": (BLOCKED, False, [0, 1])}


def m_parent_replaced_by_symlink(root, bs, out):
    shutil.move(os.fsdecode(real(root, b"/sub")), str(out / "moved_sub"))
    os.symlink(str(out / "moved_sub"), real(root, b"/sub"))
    return {b"/sub/zero": (BLOCKED, False, []), b"/sub/mid": (BLOCKED, False, [0, 1]),
            b"/sub/deep/nested": (BLOCKED, False, [0, 1])}


def m_empty_gets_a_byte(root, bs, out):
    (root / "empty").write_bytes(b"x")
    return {b"/empty": (PARTIAL, True, [])}


def m_empty_missing(root, bs, out):
    os.unlink(real(root, b"/empty"))
    return {b"/empty": (ABSENT, False, [])}


def m_empty_is_a_directory(root, bs, out):
    os.unlink(real(root, b"/sub/zero"))
    os.mkdir(real(root, b"/sub/zero"))
    return {b"/sub/zero": (BLOCKED, False, [])}


def m_unreadable(root, bs, out):
    os.chmod(real(root, b"/b63"), 0)
    return {b"/b63": (BLOCKED, False, list(range(63)))}


def _punch(root, path, bs, blocks):
    """Rewrite the file with holes over `blocks` (never written: they read
    as zeros)."""
    p = real(root, path)
    data = open(p, "rb").read()
    os.unlink(p)
    with open(p, "wb") as f:
        for j in range(0, len(data), bs):
            if j // bs in blocks:
                continue
            f.seek(j)
            f.write(data[j:j + bs])
        f.truncate(len(data))


def m_hole_over_zero_blocks(root, bs, out):
    _punch(root, b"/zeros", bs, {1, 2})       # all-zero blocks: the hole reads the same
    return {}


def m_hole_over_nonzero_block(root, bs, out):
    _punch(root, b"/zeros", bs, {2, 3})       # block 3 held random bytes
    return {b"/zeros": (PARTIAL, False, [3])}


MUTATIONS = [m_flip_first_block, m_flip_middle_block, m_flip_last_block, m_flip_last_block_of_b64,
             m_truncate_to_block_boundary, m_truncate_mid_block,
             m_truncate_ragged_last_block_by_one, m_truncate_to_zero, m_grow_by_one_byte,
             m_grow_ragged_by_a_block, m_missing_file, m_missing_directory,
             m_directory_in_its_place, m_symlink_to_identical_bytes, m_fifo_in_its_place,
             m_parent_replaced_by_symlink, m_empty_gets_a_byte, m_empty_missing,
             m_empty_is_a_directory, m_hole_over_zero_blocks, m_hole_over_nonzero_block]
if os.geteuid() != 0:  # (root reads every file)
    MUTATIONS.append(m_unreadable)


@pytest.mark.parametrize("bs", [512, 4096])
@pytest.mark.parametrize("mutate", MUTATIONS, ids=lambda m: m.__name__[2:])
def test_one_mutation(ctx64k, ctx1m, trees, tmp_path, mutate, bs):
    src, index = trees[bs]
    root = copy_tree(src, tmp_path)
    out = tmp_path / "outside"
    out.mkdir()
    victims = mutate(root, bs, out)
    want, res = check_against_restatement((ctx64k, ctx1m), index, root, threads=(1, 4))
    bits, states, longs, errnos = want
    # the restatement gives the table's row: only the victims changed, by these blocks
    files = links_restate.file_entries(index)
    lost = set()
    for (path, _, _, _), st, lg in zip(files, states, longs):
        v = victims.get(path, (COMPLETE, False, []))
        assert (st, lg) == v[:2], path
        lost |= {first_block(index, path) + j for j in v[2]}
    assert {g for g, b in enumerate(bits) if not b} == lost
    if mutate is m_missing_file:
        assert res.errnos == [0] * len(files)
    if mutate is m_unreadable:
        assert res.errnos[ordinals(index)[b"/b63"]] == errno.EACCES
    if mutate is m_directory_in_its_place:
        assert res.errnos[ordinals(index)[b"/back\\slash"]] == errno.EISDIR


@pytest.mark.parametrize("bs", [512, 4096])
def test_fresh_empty_tmp_directory(ctx64k, ctx1m, trees, tmp_path, bs):
    """What the reference starts from: everything is absent and no bit is set."""
    _, index = trees[bs]
    root = tmp_path / ".tmp.img"
    root.mkdir()
    want, res = check_against_restatement((ctx64k, ctx1m), index, root, threads=(1, 0))
    bits, states, _, _ = want
    assert not any(bits) and states == [ABSENT] * len(states)
    assert res.have == bytes(len(res.have)) and res.stats["have"] == 0
    assert res.stats["batches"] == 0 and res.stats["bytes"] == 0
    assert res.stats["unread_blocks"] == res.nblk == len(bits)
    assert len(res.missing()) == res.nblk


# ---- 4. other shapes ------------------------------------------------------------------------

RANDOM_MUTATIONS = ["flip", "truncate", "truncate_block", "grow", "delete", "file_to_symlink",
                    "file_to_dir", "dir_to_symlink", "dir_deleted", "empty_gets_a_byte",
                    "empty_deleted", "fifo"]


def _random_case(seed, base):
    rng = random.Random(seed)
    bs = rng.choice([512, 1000, 4096])
    hname = rng.choice(sorted(HASHES))
    src = base / "img"
    dirs = [src, src / "a", src / "a" / "b", src / "z z"]
    for d in dirs:
        d.mkdir()
    for i in range(rng.randrange(1, 25)):
        size = rng.choice([0, 1, bs - 1, bs, bs + 1, 3 * bs, 64 * bs, 65 * bs + 5,
                           rng.randrange(0, 12 * bs)])
        (rng.choice(dirs) / ("f%02d" % i)).write_bytes(rng.randbytes(size))
    index = dirsig_oracle.scan(str(src), bs, hname)
    files = links_restate.file_entries(index)
    root = copy_tree(src, base)
    out = base / "outside"
    out.mkdir()
    done = []
    for k in range(rng.randrange(0, 8)):
        kind = RANDOM_MUTATIONS[(seed + 5 * k) % len(RANDOM_MUTATIONS)]
        path, _, size, _ = rng.choice(files)
        p = real(root, path)
        if os.path.islink(p) or not os.path.isfile(p):
            continue  # already mutated away
        cur = os.path.getsize(p)  # (an earlier mutation may have cut or grown it)
        if kind == "flip" and cur:
            _flip(root, path, rng.randrange(cur))
        elif kind == "truncate" and cur:
            os.truncate(p, rng.randrange(cur))
        elif kind == "truncate_block" and size > bs:
            os.truncate(p, bs * rng.randrange(1, (size + bs - 1) // bs))
        elif kind == "grow" and size:
            with open(p, "ab") as f:
                f.write(b"\0" * rng.choice([1, bs, bs + 1]))
        elif kind == "delete":
            os.unlink(p)
        elif kind == "file_to_symlink":
            shutil.move(os.fsdecode(p), str(out / ("moved%d" % k)))
            os.symlink(str(out / ("moved%d" % k)), p)
        elif kind == "file_to_dir":
            os.unlink(p)
            os.mkdir(p)
        elif kind == "fifo":
            os.unlink(p)
            os.mkfifo(p)
        elif kind == "dir_to_symlink" and path.count(b"/") > 1:
            d = os.path.dirname(p)
            if not os.path.islink(d):
                shutil.move(os.fsdecode(d), str(out / ("moved_dir%d" % k)))
                os.symlink(str(out / ("moved_dir%d" % k)), d)
        elif kind == "dir_deleted" and path.count(b"/") > 1:
            if not os.path.islink(os.path.dirname(p)):
                shutil.rmtree(os.fsdecode(os.path.dirname(p)))
        elif kind == "empty_gets_a_byte" and size == 0:
            with open(p, "wb") as f:
                f.write(b"x")
        elif kind == "empty_deleted" and size == 0:
            os.unlink(p)
        done.append(kind)
    return index, root, done


@pytest.mark.parametrize("seed", range(8))
def test_random_trees_and_mutations(ctx64k, ctx1m, tmp_path, seed):
    index, root, done = _random_case(seed, tmp_path)
    ctx = ctx64k if seed % 2 else ctx1m
    want = blocks_restate.expected(index, root)
    res = ctx.check_blocks(str(root), index, 1 + seed % 4)
    assert blocks_restate.same(res, want), (done, res.states, res.errnos, want[1:])
    assert res.missing() == blocks_restate.expected_missing(index, want[0])
    assert ctx.check_index(str(root), index).ok == blocks_restate.check_index_ok(index, want[1])


def test_striped_devices(gpu, ctx64k, trees, tmp_path):
    """Three device states on the one GPU (CIR_DEBUG_SPLIT=3), stripes of 5
    blocks dealt round-robin: a file's blocks lie on several devices, a stripe
    ends on no word boundary, and the merged bitmap is that of one device."""
    bs = 512
    src, index = trees[bs]
    root = copy_tree(src, tmp_path)
    out = tmp_path / "outside"
    out.mkdir()
    os.environ["CIR_DEBUG_SPLIT"] = "3"
    try:
        ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    finally:
        del os.environ["CIR_DEBUG_SPLIT"]
    assert len(ctx.devices()) == 3

    def check(threads):
        os.environ["CIR_DEBUG_STRIPE_BLOCKS"] = "5"
        try:
            return ctx.check_blocks(str(root), index, threads)
        finally:
            del os.environ["CIR_DEBUG_STRIPE_BLOCKS"]

    want = blocks_restate.expected(index, root)
    assert all(want[0])
    assert blocks_restate.same(check(4), want)
    _flip(root, b"/b130", 33 * bs)
    m_truncate_mid_block(root, bs, out)
    m_grow_by_one_byte(root, bs, out)
    m_missing_file(root, bs, out)
    m_fifo_in_its_place(root, bs, out)
    m_empty_gets_a_byte(root, bs, out)
    want = blocks_restate.expected(index, root)
    assert set(want[1]) == {COMPLETE, ABSENT, PARTIAL, BLOCKED}
    one = ctx64k.check_blocks(str(root), index)
    assert blocks_restate.same(one, want)
    for rep in range(4):
        res = check(1 + rep)
        assert blocks_restate.same(res, want), rep
        assert res.have == one.have and res.states == one.states
    ctx.close()


def test_fd_bound_with_thousands_of_files(ctx1m, tmp_path):
    """2,000 one-block files of 512 B fill batches of hundreds of files; the
    check holds the root and O(reader threads) descriptors, not one per file.
    From the code (check.cpp): the root (1), the packer's directory and the
    file it is looking at (2), and per reader its directory and its file
    (2 x threads)."""
    rng = random.Random(9)
    d = tmp_path / "img" / "many"
    d.mkdir(parents=True)
    blob = rng.randbytes(512 + 2000)
    for i in range(2000):
        with open(d / ("f%04d" % i), "wb") as f:
            f.write(blob[i:i + 512])
    root = tmp_path / "img"
    index = dirsig_oracle.scan(str(root), 512)
    threads = 4
    res = ctx1m.check_blocks(str(root), index, threads)
    assert res.complete and res.nblk == 2000 and res.stats["have"] == 2000
    assert res.stats["bytes"] == 2000 * 512
    assert res.stats["batches"] <= 12                # hundreds of files per batch
    assert 1 <= res.stats["peak_fds"] <= 1 + 2 + 2 * threads
    # a flipped byte, a short file and a missing one deep inside such a batch:
    # found at their own blocks alone
    _flip(root, b"/many/f1357", 100)
    os.truncate(str(d / "f0700"), 511)
    os.unlink(str(d / "f0064"))
    res = ctx1m.check_blocks(str(root), index, threads)
    assert [g for g in range(2000) if not res.has(g)] == [64, 700, 1357]
    assert [res.states[g] for g in (64, 700, 1357)] == [ABSENT, PARTIAL, PARTIAL]
    assert res.states.count(COMPLETE) == 1997
    assert 1 <= res.stats["peak_fds"] <= 1 + 2 + 2 * threads


def test_context_is_healthy_after_bad_verdicts(gpu, trees, tmp_path):
    bs = 4096
    src, index = trees[bs]
    root = copy_tree(src, tmp_path)
    ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    for path, _, size, _ in links_restate.file_entries(index):
        if size:
            _flip(root, path, size - 1)              # every file's last block is bad
    os.unlink(real(root, b"/b65"))
    want = blocks_restate.expected(index, root)
    assert COMPLETE not in [s for s, f in zip(want[1], links_restate.file_entries(index)) if f[2]]
    assert blocks_restate.same(ctx.check_blocks(str(root), index), want)
    # the context goes on: the complete tree, the other checks, and the bad tree again
    assert ctx.check_blocks(str(src), index).complete
    assert ctx.check_index(str(src), index).ok
    assert not ctx.check_index(str(root), index).ok
    assert blocks_restate.same(ctx.check_blocks(str(root), index), want)
    ctx.close()


def test_parse_errors(gpu, ctx64k, trees):
    root, index = trees[512]
    for bad in (b"", index[:40], index[:len(index) // 2]):
        with pytest.raises(gpu.CiruelaError) as e:
            ctx64k.check_blocks(str(root), bad)
        assert e.value.status == gpu._n.CIR_EPARSE
    assert ctx64k.check_blocks(str(root), index).complete


# ---- 5. the CLI ------------------------------------------------------------------------------------

def _escaped_paths(index):
    """The file entries' paths as the index spells them, in index order."""
    _, _, dirs, _ = dirsig_oracle.parse(index)
    return [(b"" if vesc == b"/" else vesc) + b"/" + e[1]
            for vesc, entries in dirs for e in entries if e[0] == "f"]


def test_cli_blocks(trees, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    bs = 4096
    src, index = trees[bs]
    (tmp_path / "img.ds1").write_bytes(index)
    ds1 = str(tmp_path / "img.ds1")
    files = links_restate.file_entries(index)
    nblk = sum(len(f[3]) for f in files)
    # the complete tree: the "ok" status of `check`, with and without --list
    for extra in ([], ["--list"]):
        p = subprocess.run([cli, "blocks", str(src), ds1] + extra, capture_output=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout == (b"blocks: %d of %d; files: %d complete, 0 absent, 0 partial, "
                            b"0 blocked\n" % (nblk, nblk, len(files)))
    root = copy_tree(src, tmp_path)
    _flip(root, b"/b130", 70 * bs)
    os.truncate(real(root, b"/with space"), 3)
    os.unlink(real(root, b"/sub/mid"))
    os.unlink(real(root, b"/back\\slash"))
    os.mkdir(real(root, b"/back\\slash"))
    bits, states, _, _ = blocks_restate.expected(index, root)
    summary = (b"blocks: %d of %d; files: %d complete, %d absent, %d partial, %d blocked\n"
               % (sum(bits), nblk, states.count(COMPLETE), states.count(ABSENT),
                  states.count(PARTIAL), states.count(BLOCKED)))
    assert states.count(ABSENT) == 1 and states.count(BLOCKED) == 1 and states.count(PARTIAL) == 2
    p = subprocess.run([cli, "blocks", str(root), ds1, "--disk-threads", "2"],
                       capture_output=True, timeout=120)
    assert p.returncode == 1, p.stderr[-2000:]               # the "bad" status of `check`
    assert p.stdout == summary
    esc = dict(zip([f[0] for f in files], _escaped_paths(index)))
    lines = [esc[path] + b" %d" % off
             for path, off in blocks_restate.expected_missing(index, bits)]
    assert len(lines) == 1 + 1 + 2 + 1 and b"/with\\x20space 0" in lines
    p = subprocess.run([cli, "blocks", str(root), ds1, "--list"], capture_output=True,
                       timeout=120)
    assert p.returncode == 1
    assert p.stdout == summary + b"".join(ln + b"\n" for ln in lines)
    # a root that does not open and an index that does not parse: exit 2, no verdict
    p = subprocess.run([cli, "blocks", str(tmp_path / "nowhere"), ds1], capture_output=True,
                       timeout=120)
    assert p.returncode == 2 and p.stdout == b""
    (tmp_path / "img.ds1").write_bytes(index[:100])
    p = subprocess.run([cli, "blocks", str(root), ds1], capture_output=True, timeout=120)
    assert p.returncode == 2 and p.stdout == b""
