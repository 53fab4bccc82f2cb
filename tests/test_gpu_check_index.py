"""cir_check_index and cir_verify_first_dev on the GPU.

commit_image (src/daemon/disk/commit.rs:51-117) walks the index in order and
fails at the first entry that does not match: Error::Checksum for a file
whose blocks differ (:108-111) or an "empty" file that is not (:79-81),
Error::ReadFile for one it cannot open or read (:98-106).  cir_check_index
gives that verdict for a whole image in one call.

No expected verdict comes from the code under test: digests are hashlib's
(oracle/dirsig_oracle.py HASHES), indexes are dirsig_oracle.scan's, and the
expected (kind, path) is `expected_verdict` below, which walks
dirsig_oracle.parse(index) in order with os.stat(dir_fd=...,
follow_symlinks=False) and applies the entry rules itself.
"""
import ctypes
import errno
import os
import random
import re
import shutil
import stat
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import dirsig_oracle

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
OK, CHECKSUM, READ = "ok", "checksum", "read"
_DIR = os.O_RDONLY | os.O_DIRECTORY | os.O_CLOEXEC


# ---- the expected verdict (independent of the library) ---------------------

def unescape(b):
    return re.sub(rb"\\x([0-9a-f]{2})", lambda m: bytes([int(m.group(1), 16)]), b)


def _open_dir_nofollow(rootfd, comps):
    """(fd, 0) of rootfd/comps..., each component lstat'ed and opened without
    following symlinks, or (None, errno): ENOENT for a missing component,
    ENOTDIR for one that is not a directory."""
    fd = os.dup(rootfd)
    for c in comps:
        try:
            st = os.stat(c, dir_fd=fd, follow_symlinks=False)
        except OSError as e:
            os.close(fd)
            return None, e.errno
        if not stat.S_ISDIR(st.st_mode):
            os.close(fd)
            return None, errno.ENOTDIR
        nfd = os.open(c, _DIR | os.O_NOFOLLOW, dir_fd=fd)
        os.close(fd)
        fd = nfd
    return fd, 0


def expected_verdict(root, index):
    """(kind, path) of the first failing entry in index order."""
    hash_name, bs, dirs, _ = dirsig_oracle.parse(index)
    h = dirsig_oracle.HASHES[hash_name]
    rootfd = os.open(root, _DIR)
    try:
        for vesc, entries in dirs:
            vpath = unescape(vesc)
            dfd, derr = _open_dir_nofollow(rootfd, [c for c in vpath.split(b"/") if c])
            try:
                for e in entries:
                    if e[0] != "f":
                        continue  # symlinks are the caller's to create
                    name = unescape(e[1])
                    path = (b"/" if vpath == b"/" else vpath + b"/") + name
                    size, digests = e[3], e[4]
                    st = None
                    if dfd is None:
                        err = derr
                    else:
                        try:
                            st = os.stat(name, dir_fd=dfd, follow_symlinks=False)
                            err = 0
                        except OSError as ex:
                            err = ex.errno
                    if size == 0:
                        if err == errno.ENOENT:
                            continue
                        if err:
                            return READ, path
                        if not (stat.S_ISREG(st.st_mode) and st.st_size == 0):
                            return CHECKSUM, path
                        continue
                    if err or not stat.S_ISREG(st.st_mode):
                        return READ, path
                    if st.st_size != size:
                        return CHECKSUM, path
                    fd = os.open(name, os.O_RDONLY | os.O_NOFOLLOW, dir_fd=dfd)
                    with os.fdopen(fd, "rb") as f:
                        data = f.read()
                    if [h(data[i:i + bs]) for i in range(0, len(data), bs)] != digests:
                        return CHECKSUM, path
            finally:
                if dfd is not None:
                    os.close(dfd)
    finally:
        os.close(rootfd)
    return OK, None


def listed_files(index):
    """[(path bytes, size, nblocks)] of the file entries, in index order."""
    _, _, dirs, _ = dirsig_oracle.parse(index)
    out = []
    for vesc, entries in dirs:
        vpath = unescape(vesc)
        for e in entries:
            if e[0] == "f":
                out.append(((b"/" if vpath == b"/" else vpath + b"/") + unescape(e[1]), e[3],
                            len(e[4])))
    return out


def real(root, path):
    return os.path.join(os.fsencode(str(root)), path.lstrip(b"/"))


def verdict(res):
    return res.kind, res.path


# ---- trees and contexts -----------------------------------------------------

def make_tree(root):
    """The shape of test_gpu_parity.make_tree: empty files, an exe, symlinks,
    names with a space and a backslash, an exact-multiple file, a short tail."""
    rng = random.Random(5)
    (root / "a" / "b" / "c").mkdir(parents=True)
    (root / "empty_dir").mkdir()
    (root / "z").mkdir()
    (root / "hello.txt").write_bytes(b"hello\n")
    (root / "test.txt").write_bytes(b"")
    (root / "a" / "big.bin").write_bytes(rng.randbytes(5 * 32768 + 1234))
    (root / "a" / "exact.bin").write_bytes(rng.randbytes(2 * 32768))
    (root / "a" / "none").write_bytes(b"")
    (root / "a" / "b" / "run.sh").write_bytes(b"#!/bin/sh\necho hi\n")
    os.chmod(root / "a" / "b" / "run.sh", 0o755)
    (root / "a" / "b" / "c" / "deep").write_bytes(rng.randbytes(rng.randrange(1, 5000)))
    for i in range(60):
        (root / "z" / ("f%03d" % i)).write_bytes(rng.randbytes(rng.randrange(0, 70000)))
    (root / "z" / "f030").write_bytes(rng.randbytes(50000))
    (root / "z" / "with space").write_bytes(b"x")
    (root / "z" / "back\\slash").write_bytes(b"y")
    (root / "z" / "zz_empty").write_bytes(b"")
    os.symlink("../hello.txt", root / "a" / "link")
    os.symlink("target with space", root / "dangling")


HASHES = {"blake2b/256": "blake2b_256", "sha512/256": "sha512_256"}


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    """The clean tree and its oracle indexes, {(bs, hash name): bytes}."""
    root = tmp_path_factory.mktemp("clean") / "img"
    root.mkdir()
    make_tree(root)
    idx = {(bs, hn): dirsig_oracle.scan(str(root), bs, hn)
           for bs in (4096, 32768) for hn in HASHES}
    return root, idx


@pytest.fixture(scope="module")
def ctx64k(gpu):
    return gpu.Context(device_mask=1, staging_bytes=64 << 10)


@pytest.fixture(scope="module")
def ctx1m(gpu):
    return gpu.Context(device_mask=1, staging_bytes=1 << 20)


def copy_tree(clean, tmp_path):
    root = tmp_path / "img"
    shutil.copytree(str(clean[0]), str(root), symlinks=True)
    return root


# ---- 1. the kernel's edges through verify_first_dev ---------------------------

def _first_call(gpu, ctx, torch, hasht, d_arena, arena_bytes, d_off, d_len, n, expected):
    """One cir_verify_first_dev call with garbage in the result cells."""
    d_exp = torch.tensor(np.frombuffer(bytes(expected) or b"\0" * 32, dtype=np.uint8).copy(),
                         device="cuda:0")
    d_dig = torch.full((32 * max(n, 1),), 0xCD, dtype=torch.uint8, device="cuda:0")
    d_first = torch.full((1,), 0x1234567, dtype=torch.int64, device="cuda:0")
    d_nbad = torch.full((1,), 999, dtype=torch.int32, device="cuda:0")
    ctx.verify_first_dev(d_arena.data_ptr() if d_arena is not None else 0, arena_bytes,
                         d_off.data_ptr() if n else 0, d_len.data_ptr() if n else 0, n,
                         d_exp.data_ptr(), d_dig.data_ptr(), d_first.data_ptr(),
                         d_nbad.data_ptr(), 0, hasht)
    torch.cuda.synchronize()
    return int(d_first.item()) & U64, int(d_nbad.item()) & 0xFFFFFFFF, d_dig.cpu().numpy()


@pytest.mark.parametrize("hname", sorted(HASHES))
@pytest.mark.parametrize("nblk", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_first_bad_kernel_edges(gpu, ctx1m, nblk, hname):
    import torch
    h = dirsig_oracle.HASHES[hname]
    hasht = getattr(gpu.HashType, HASHES[hname])()
    rng = random.Random(nblk * 3 + len(hname))
    lens = [rng.randrange(0, 301) for _ in range(nblk)]
    offs, pos = [], 0
    for ln in lens:
        offs.append(pos)
        pos += ln
    host = np.frombuffer(rng.randbytes(pos + 64), dtype=np.uint8).copy()
    raw = host.tobytes()
    good = [h(raw[o:o + ln]) for o, ln in zip(offs, lens)]
    d_arena = torch.from_numpy(host).to("cuda:0")
    d_off = torch.tensor(np.array(offs, dtype=np.uint64).view(np.int64), device="cuda:0")
    d_len = torch.tensor(np.array(lens, dtype=np.uint32).view(np.int32), device="cuda:0")

    def run(expected, arena_bytes=U64):
        first, nbad, dig = _first_call(gpu, ctx1m, torch, hasht, d_arena, arena_bytes, d_off,
                                       d_len, nblk, b"".join(expected))
        if nblk:  # the digests themselves are the oracle's, whatever is expected
            assert dig.tobytes() == b"".join(good)
        return first, nbad

    # nothing bad: trusted descriptors, and through the bounds pass
    assert run(good) == (U64, 0)
    assert run(good, pos) == (U64, 0)
    if nblk == 0:
        return

    def flipped(i, byte=7):
        d = bytearray(good[i])
        d[byte] ^= 0x10
        return bytes(d)

    # one bad block at each edge position
    for b in sorted({p for p in (0, 63, 64, 255, 256, nblk - 1) if p < nblk}):
        exp = list(good)
        exp[b] = flipped(b)
        assert run(exp) == (b, 1), b
    # a digest differing only in its first byte, only in its last
    b = nblk // 2
    for byte in (0, 31):
        exp = list(good)
        exp[b] = flipped(b, byte)
        assert run(exp) == (b, 1), byte
    # several bad blocks: the smallest index, the exact count
    if nblk >= 3:
        bad = sorted(rng.sample(range(nblk), min(nblk, rng.randrange(2, 40))))
        exp = list(good)
        for b in bad:
            exp[b] = flipped(b, b % 32)
        assert run(exp) == (bad[0], len(bad))
        assert run(exp, pos) == (bad[0], len(bad))


def test_first_bad_out_of_range_descriptor(gpu, ctx1m):
    """A descriptor one byte past arena_bytes (inside a larger allocation, as
    in tests/test_gpu_bounded.py: only the flag shows the bound) counts as
    bad whatever is expected of it, and is never read: its digest is zeros."""
    import torch
    h = dirsig_oracle.HASHES["blake2b/256"]
    rng = random.Random(11)
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
    first, nbad, dig = _first_call(gpu, ctx1m, torch, hasht, d_arena, arena_bytes, d_off, d_len, n,
                                   b"".join(good))
    assert (first, nbad) == (130, 1)
    dig = dig.reshape(-1, 32)
    assert not dig[130].any()
    assert dig[131].tobytes() == good[131]
    # the zero digest it is given does not make it good either
    exp = list(good)
    exp[130] = bytes(32)
    exp[150] = bytes(32)
    first, nbad, _ = _first_call(gpu, ctx1m, torch, hasht, d_arena, arena_bytes, d_off, d_len, n,
                                 b"".join(exp))
    assert (first, nbad) == (130, 2)
    # with the whole allocation as the arena the same batch is clean
    first, nbad, _ = _first_call(gpu, ctx1m, torch, hasht, d_arena, arena_bytes + 4096, d_off,
                                 d_len, n, b"".join(good))
    assert (first, nbad) == (U64, 0)


# ---- 2. a clean tree -----------------------------------------------------------

@pytest.mark.parametrize("hname", sorted(HASHES))
@pytest.mark.parametrize("bs", [4096, 32768])
def test_clean_tree_is_ok(gpu, ctx64k, ctx1m, clean, bs, hname):
    root, idx = clean
    index = idx[(bs, hname)]
    assert expected_verdict(str(root), index) == (OK, None)
    files = listed_files(index)
    for ctx in (ctx64k, ctx1m):
        for threads in (1, 4, 0):
            res = ctx.check_index(str(root), index, threads)
            assert res.ok and res.kind == OK and res.path is None and res.errno == 0
            st = res.stats
            assert st["files"] == sum(1 for _, size, _ in files if size)
            assert st["blocks"] == sum(nb for _, _, nb in files)
            assert st["bytes"] == sum(size for _, size, _ in files)
            assert st["empty_entries"] == sum(1 for _, size, _ in files if size == 0)
            assert st["first_bad_block"] == U64
            assert st["batches"] >= 1
    # about 2.6 MB through 64 KiB slots: many batches
    assert ctx64k.check_index(str(root), index).stats["batches"] > 30
    # the root as a directory fd, and relative to one
    fd = os.open(str(root.parent), _DIR)
    try:
        assert gpu.check_index("img", index, dir_fd=fd, context=ctx64k).ok
    finally:
        os.close(fd)
    fd = os.open(str(root), _DIR)
    try:
        assert ctx64k.check_index(None, index, dir_fd=fd).ok
    finally:
        os.close(fd)


# ---- 3. one mutation each ---------------------------------------------------------

def _flip(root, path, at):
    p = real(root, path)
    with open(p, "r+b") as f:
        f.seek(at)
        c = f.read(1)
        f.seek(at)
        f.write(bytes([c[0] ^ 1]))


def _nonempty(index):
    return [(p, size, nb) for p, size, nb in listed_files(index) if size]


def m_flip_first(root, index, out):
    _flip(root, _nonempty(index)[0][0], 0)


def m_flip_last(root, index, out):
    p, size, _ = _nonempty(index)[-1]
    _flip(root, p, size - 1)


def m_flip_middle_block(root, index, out):
    _flip(root, b"/a/big.bin", 3 * 32768 + 17)


def m_flip_last_byte_of_short_tail(root, index, out):
    _flip(root, b"/a/big.bin", 5 * 32768 + 1233)


def m_truncate_one(root, index, out):
    os.truncate(real(root, b"/a/big.bin"), 5 * 32768 + 1233)


def m_truncate_to_boundary(root, index, out):
    os.truncate(real(root, b"/a/big.bin"), 5 * 32768)


def m_grow_one(root, index, out):
    with open(real(root, b"/a/exact.bin"), "ab") as f:
        f.write(b"\0")


def m_grow_block(root, index, out):
    with open(real(root, b"/a/exact.bin"), "ab") as f:
        f.write(bytes(32768))


def m_delete(root, index, out):
    os.unlink(real(root, b"/z/f030"))


def m_file_to_symlink(root, index, out):
    out.mkdir(exist_ok=True)
    shutil.move(os.fsdecode(real(root, b"/a/exact.bin")), str(out / "exact.bin"))
    os.symlink(str(out / "exact.bin"), real(root, b"/a/exact.bin"))


def m_dir_to_symlink(root, index, out):
    out.mkdir(exist_ok=True)
    shutil.move(os.fsdecode(real(root, b"/a/b")), str(out / "b"))
    os.symlink(str(out / "b"), real(root, b"/a/b"))


def m_empty_gets_a_byte(root, index, out):
    with open(real(root, b"/test.txt"), "wb") as f:
        f.write(b"!")


def m_empty_deleted(root, index, out):
    os.unlink(real(root, b"/test.txt"))


def m_empty_dir_of_empty_deleted(root, index, out):
    os.unlink(real(root, b"/z/zz_empty"))
    os.unlink(real(root, b"/a/none"))


def m_extra_file(root, index, out):
    with open(real(root, b"/z/unlisted"), "wb") as f:
        f.write(b"not in the index")
    os.mkdir(real(root, b"/unlisted_dir"))


def m_index_hex_digit(root, index, out):
    lines = index.split(b"\n")
    k = next(i for i, ln in enumerate(lines) if ln.startswith(b"  f030 f "))
    head, last = lines[k].rsplit(b" ", 1)
    lines[k] = head + b" " + last[:10] + (b"0" if last[10:11] != b"0" else b"1") + last[11:]
    return b"\n".join(lines)


def m_flip_name_with_space(root, index, out):
    _flip(root, b"/z/with space", 0)


def m_flip_name_with_backslash(root, index, out):
    _flip(root, b"/z/back\\slash", 0)


def m_none(root, index, out):
    pass


# name -> (mutation, the verdict it must give, beyond equalling the helper's)
MUTATIONS = {
    "flip_first": (m_flip_first, (CHECKSUM, b"/hello.txt")),
    "flip_last": (m_flip_last, (CHECKSUM, b"/z/with space")),
    "flip_middle_block": (m_flip_middle_block, (CHECKSUM, b"/a/big.bin")),
    "flip_last_byte_of_short_tail": (m_flip_last_byte_of_short_tail, (CHECKSUM, b"/a/big.bin")),
    "truncate_one": (m_truncate_one, (CHECKSUM, b"/a/big.bin")),
    "truncate_to_boundary": (m_truncate_to_boundary, (CHECKSUM, b"/a/big.bin")),
    "grow_one": (m_grow_one, (CHECKSUM, b"/a/exact.bin")),
    "grow_block": (m_grow_block, (CHECKSUM, b"/a/exact.bin")),
    "delete": (m_delete, (READ, b"/z/f030")),
    "file_to_symlink": (m_file_to_symlink, (READ, b"/a/exact.bin")),
    "dir_to_symlink": (m_dir_to_symlink, (READ, b"/a/b/run.sh")),
    "empty_gets_a_byte": (m_empty_gets_a_byte, (CHECKSUM, b"/test.txt")),
    "empty_deleted": (m_empty_deleted, (OK, None)),
    "empties_deleted": (m_empty_dir_of_empty_deleted, (OK, None)),
    "extra_file": (m_extra_file, (OK, None)),
    "index_hex_digit": (m_index_hex_digit, (CHECKSUM, b"/z/f030")),
    "name_with_space": (m_flip_name_with_space, (CHECKSUM, b"/z/with space")),
    "name_with_backslash": (m_flip_name_with_backslash, (CHECKSUM, b"/z/back\\slash")),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_one_mutation(gpu, ctx64k, ctx1m, clean, tmp_path, name):
    mutate, must = MUTATIONS[name]
    root = copy_tree(clean, tmp_path)
    for bs, hname, ctx in ((4096, "blake2b/256", ctx64k), (32768, "sha512/256", ctx1m)):
        index = clean[1][(bs, hname)]
        if bs == 4096:  # the tree is mutated once; both indexes see it
            index = mutate(root, index, tmp_path / "outside") or index
        elif mutate is m_index_hex_digit:
            index = mutate(root, index, None)
        want = expected_verdict(str(root), index)
        assert want == must, "the helper disagrees with the case's own expectation"
        res = ctx.check_index(str(root), index, threads=4)
        assert verdict(res) == want, (bs, hname)
        if want[0] == READ:
            assert res.errno in (errno.ENOENT, errno.ELOOP, errno.ENOTDIR), res.errno
            assert res.stats["first_bad_block"] == U64
        elif want[0] == CHECKSUM:
            assert res.errno == 0


def test_checksum_reports_the_first_bad_block(ctx64k, clean, tmp_path):
    """stats[7]: the global index (blocks counted in index order) of the first
    bad block; a length mismatch has none."""
    root = copy_tree(clean, tmp_path)
    index = clean[1][(4096, "blake2b/256")]
    _flip(root, b"/a/big.bin", 20 * 4096 + 5)
    _flip(root, b"/a/big.bin", 30 * 4096)
    before = 0
    for p, _, nb in listed_files(index):
        if p == b"/a/big.bin":
            break
        before += nb
    res = ctx64k.check_index(str(root), index, threads=2)
    assert verdict(res) == (CHECKSUM, b"/a/big.bin")
    assert res.stats["first_bad_block"] == before + 20
    os.truncate(real(root, b"/hello.txt"), 3)
    res = ctx64k.check_index(str(root), index, threads=2)
    assert verdict(res) == (CHECKSUM, b"/hello.txt")
    assert res.stats["first_bad_block"] == U64


# ---- 4. order ----------------------------------------------------------------------

@pytest.mark.parametrize("early,late", [(b"/z/f003", b"/z/f005"),        # neighbours: one batch
                                        (b"/hello.txt", b"/z/f055")])   # far apart: other batches
@pytest.mark.parametrize("missing_first", [True, False])
def test_first_failure_in_index_order_wins(ctx64k, clean, tmp_path, early, late, missing_first):
    root = copy_tree(clean, tmp_path)
    index = clean[1][(4096, "blake2b/256")]
    sizes = {p: size for p, size, _ in listed_files(index)}
    assert sizes[early] and sizes[late]
    if missing_first:
        os.unlink(real(root, early))
        _flip(root, late, sizes[late] // 2)
        must = (READ, early)
    else:
        _flip(root, early, sizes[early] // 2)
        os.unlink(real(root, late))
        must = (CHECKSUM, early)
    assert expected_verdict(str(root), index) == must
    for threads in (1, 4):
        assert verdict(ctx64k.check_index(str(root), index, threads)) == must


# ---- 5. several devices -------------------------------------------------------------

def test_striped_devices(gpu, clean, tmp_path):
    """Three device states on the one GPU (CIR_DEBUG_SPLIT=3), stripes of 4
    blocks dealt round-robin: the verdict is the global minimum, whatever
    the timing of the device threads."""
    root = copy_tree(clean, tmp_path)
    index = clean[1][(4096, "blake2b/256")]
    os.environ["CIR_DEBUG_SPLIT"] = "3"
    try:
        ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    finally:
        del os.environ["CIR_DEBUG_SPLIT"]
    assert len(ctx.devices()) == 3

    def check(threads=4):
        os.environ["CIR_DEBUG_STRIPE_BLOCKS"] = "4"
        try:
            return ctx.check_index(str(root), index, threads)
        finally:
            del os.environ["CIR_DEBUG_STRIPE_BLOCKS"]

    res = check()
    assert res.ok
    files = listed_files(index)
    assert res.stats["files"] == sum(1 for _, size, _ in files if size)
    assert res.stats["blocks"] == sum(nb for _, _, nb in files)
    assert res.stats["bytes"] == sum(size for _, size, _ in files)
    assert res.stats["empty_entries"] == sum(1 for _, size, _ in files if size == 0)
    # two flipped files whose bad blocks lie in stripes of different devices
    first = {}
    g = 0
    for p, _, nb in files:
        first[p] = g
        g += nb
    a, b = b"/a/big.bin", b"/z/f030"
    ga, gb = first[a] + 9, first[b] + 2
    assert (ga // 4) % 3 != (gb // 4) % 3 and ga < gb
    _flip(root, a, 9 * 4096 + 1)
    _flip(root, b, 2 * 4096 + 1)
    assert expected_verdict(str(root), index) == (CHECKSUM, a)
    for rep in range(5):
        res = check(threads=1 + rep)
        assert verdict(res) == (CHECKSUM, a), rep
        assert res.stats["first_bad_block"] == ga
    # a missing file before both wins over them
    os.unlink(real(root, b"/hello.txt"))
    assert verdict(check()) == (READ, b"/hello.txt")
    ctx.close()


# ---- 6. the context after a bad verdict ----------------------------------------------

def test_context_is_healthy_after_bad_verdicts(gpu, clean, tmp_path):
    root = copy_tree(clean, tmp_path)
    index = clean[1][(4096, "blake2b/256")]
    ctx = gpu.Context(device_mask=1, staging_bytes=64 << 10)
    cfg = gpu.ScannerConfig.new().block_size(4096).threads(4).add_dir(str(clean[0]), "/")
    _flip(root, b"/a/big.bin", 5)
    assert verdict(ctx.check_index(str(root), index)) == (CHECKSUM, b"/a/big.bin")
    assert ctx.check_index(str(clean[0]), index).ok
    assert gpu.v1.scan(cfg, context=ctx) == index
    os.unlink(real(root, b"/a/b/c/deep"))
    _flip(root, b"/a/big.bin", 5)  # back to clean
    res = ctx.check_index(str(root), index)
    assert verdict(res) == (READ, b"/a/b/c/deep") and res.errno == errno.ENOENT
    assert ctx.check_index(str(clean[0]), index).ok
    assert gpu.v1.scan(cfg, context=ctx) == index
    ctx.close()


# ---- 7. indexes that do not parse -----------------------------------------------------

def test_parse_errors(gpu, ctx64k, clean):
    root, idx = clean
    index = idx[(4096, "blake2b/256")]
    n = gpu._n

    def status(ix):
        with pytest.raises(gpu.CiruelaError) as e:
            ctx64k.check_index(str(root), ix)
        return e.value.status

    assert status(index[:len(index) // 2]) == n.CIR_EPARSE          # cut inside a line
    assert status(index.replace(b"  hello.txt f", b"  .. f", 1)) == n.CIR_EPARSE
    assert status(index.replace(b"\n/a\n", b"\n/a/../a\n", 1)) == n.CIR_EPARSE
    short = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  f f 10 " + b"ab" * 16 +
             b"\n" + b"ab" * 32 + b"\n")
    assert status(short) in (n.CIR_EHASHSIZE, n.CIR_EPARSE)
    assert status(b"") == n.CIR_EPARSE
    # the root itself missing: the one CIR_EIO
    with pytest.raises(gpu.CiruelaError) as e:
        ctx64k.check_index(str(root / "no such dir"), index)
    assert e.value.status == n.CIR_EIO
    # and the context still works
    assert ctx64k.check_index(str(root), index).ok


# ---- 8. file descriptors ------------------------------------------------------------------

def test_fd_bound_with_thousands_of_small_files(ctx1m, tmp_path):
    """5,000 one-block files in one directory fill batches of thousands of
    files; the check holds O(reader threads) descriptors, not one per file."""
    rng = random.Random(8)
    d = tmp_path / "img" / "many"
    d.mkdir(parents=True)
    blob = rng.randbytes(5000 + 200)
    for i in range(5000):
        with open(d / ("f%04d" % i), "wb") as f:
            f.write(blob[i:i + 1 + i % 200])
    index = dirsig_oracle.scan(str(tmp_path / "img"), 4096)
    res = ctx1m.check_index(str(tmp_path / "img"), index, threads=4)
    assert res.ok
    assert res.stats["files"] == 5000 and res.stats["blocks"] == 5000
    assert res.stats["batches"] <= 8          # thousands of files per batch
    assert 1 <= res.stats["peak_fds"] <= 4 + 8
    # a flipped byte deep inside such a batch is found, at its file
    _flip(tmp_path / "img", b"/many/f3456", 0)
    assert verdict(ctx1m.check_index(str(tmp_path / "img"), index, threads=4)) == \
        (CHECKSUM, b"/many/f3456")


# ---- 9. randomised ----------------------------------------------------------------------------

RANDOM_MUTATIONS = ["none", "flip", "truncate_one", "truncate_to_boundary", "grow_one",
                    "grow_block", "delete", "file_to_symlink", "dir_to_symlink",
                    "empty_gets_a_byte", "empty_deleted", "extra_file", "index_hex_digit"]


def _random_case(seed, base):
    rng = random.Random(seed)
    bs = 4096
    root = base / "img"
    dirs = [root] + [root / ("d%d" % i) for i in range(rng.randrange(0, 4))]
    dirs += [dirs[-1] / "sub"] if len(dirs) > 1 and rng.random() < 0.5 else []
    for d in dirs:
        d.mkdir(parents=True, exist_ok=True)
    for i in range(rng.randrange(1, 41)):
        nb = rng.randrange(0, 4)
        size = 0 if nb == 0 else rng.choice([nb * bs, (nb - 1) * bs + rng.randrange(1, bs)])
        (rng.choice(dirs) / ("f%02d" % i)).write_bytes(rng.randbytes(size))
    hname = rng.choice(sorted(HASHES))
    index = dirsig_oracle.scan(str(root), bs, hname)
    files = listed_files(index)
    nonempty = [f for f in files if f[1]]
    empty = [f for f in files if not f[1]]
    # (every kind comes up: the seeds walk the list, the tree and the victim are random)
    kind = RANDOM_MUTATIONS[seed % len(RANDOM_MUTATIONS)]
    out = base / "outside"
    out.mkdir()
    if kind == "flip" and nonempty:
        p, size, _ = rng.choice(nonempty)
        _flip(root, p, rng.randrange(size))
    elif kind == "truncate_one" and nonempty:
        p, size, _ = rng.choice(nonempty)
        os.truncate(real(root, p), size - 1)
    elif kind == "truncate_to_boundary" and nonempty:
        p, size, _ = rng.choice(nonempty)
        os.truncate(real(root, p), (size - 1) // bs * bs)
    elif kind in ("grow_one", "grow_block") and nonempty:
        p, _, _ = rng.choice(nonempty)
        with open(real(root, p), "ab") as f:
            f.write(bytes(1 if kind == "grow_one" else bs))
    elif kind == "delete" and nonempty:
        os.unlink(real(root, rng.choice(nonempty)[0]))
    elif kind == "file_to_symlink" and nonempty:
        p = rng.choice(nonempty)[0]
        shutil.move(os.fsdecode(real(root, p)), str(out / "moved"))
        os.symlink(str(out / "moved"), real(root, p))
    elif kind == "dir_to_symlink" and len(dirs) > 1:
        d = rng.choice(dirs[1:])
        shutil.move(str(d), str(out / "moved_dir"))
        os.symlink(str(out / "moved_dir"), str(d))
    elif kind == "empty_gets_a_byte" and empty:
        with open(real(root, rng.choice(empty)[0]), "wb") as f:
            f.write(b"x")
    elif kind == "empty_deleted" and empty:
        os.unlink(real(root, rng.choice(empty)[0]))
    elif kind == "extra_file":
        (rng.choice(dirs) / "unlisted").write_bytes(b"extra")
    elif kind == "index_hex_digit" and nonempty:
        lines = index.split(b"\n")
        ks = [i for i, ln in enumerate(lines) if re.match(rb"  \S+ [fx] [1-9]", ln)]
        k = rng.choice(ks)
        head, last = lines[k].rsplit(b" ", 1)
        at = rng.randrange(64)
        last = last[:at] + (b"0" if last[at:at + 1] != b"0" else b"1") + last[at + 1:]
        lines[k] = head + b" " + last
        index = b"\n".join(lines)
    return root, index, kind


@pytest.mark.parametrize("seed", range(20))
def test_random_trees_and_mutations(ctx64k, tmp_path, seed):
    root, index, kind = _random_case(seed, tmp_path)
    want = expected_verdict(str(root), index)
    res = ctx64k.check_index(str(root), index, threads=1 + seed % 4)
    assert verdict(res) == want, kind


# ---- 10. the CLI ------------------------------------------------------------------------------------

def test_cli_check(clean, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    root = copy_tree(clean, tmp_path)
    index = clean[1][(32768, "blake2b/256")]
    ipath = tmp_path / "image.ds1"
    ipath.write_bytes(index)
    p = subprocess.run([cli, "check", str(root), str(ipath)], capture_output=True, timeout=120)
    assert (p.returncode, p.stdout) == (0, b""), p.stderr[-2000:]
    _flip(root, b"/z/with space", 0)
    want = expected_verdict(str(root), index)
    assert want == (CHECKSUM, b"/z/with space")
    p = subprocess.run([cli, "check", str(root), str(ipath), "--disk-threads", "2"],
                       capture_output=True, timeout=120)
    assert p.returncode == 1, p.stderr[-2000:]
    assert p.stdout == b"checksum: /z/with space\n"
    os.unlink(real(root, b"/hello.txt"))
    p = subprocess.run([cli, "check", str(root), str(ipath)], capture_output=True, timeout=120)
    assert p.returncode == 1, p.stderr[-2000:]
    assert p.stdout == b"read: /hello.txt: " + os.strerror(errno.ENOENT).encode() + b"\n"
    ipath.write_bytes(index[:100])
    p = subprocess.run([cli, "check", str(root), str(ipath)], capture_output=True, timeout=120)
    assert p.returncode == 2 and p.stdout == b""
