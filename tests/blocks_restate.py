"""Python restatement of cir_check_blocks' rules, for its tests (no test
module: helpers only).

For every file entry of dirsig_oracle.parse(index), in index order: the path
is walked below the root one component at a time with os.stat(dir_fd=...,
follow_symlinks=False) / os.open(O_DIRECTORY | O_NOFOLLOW); the file is
opened with O_NOFOLLOW and read; block j has its bit exactly when its bytes
[j bs, min((j + 1) bs, size)) lie inside the file's length and their hashlib
digest (dirsig_oracle.HASHES) is the index's.  Nothing here calls the library.
"""
import errno
import os
import stat

import dirsig_oracle
from links_restate import file_entries

COMPLETE, ABSENT, PARTIAL, BLOCKED = "complete", "absent", "partial", "blocked"
_DIR = os.O_RDONLY | os.O_DIRECTORY | os.O_CLOEXEC


def _open_dir_nofollow(rootfd, comps):
    fd = os.dup(rootfd)
    try:
        for c in comps:
            st = os.stat(c, dir_fd=fd, follow_symlinks=False)
            if not stat.S_ISDIR(st.st_mode):
                raise OSError(errno.ENOTDIR, "not a directory")
            nfd = os.open(c, _DIR | os.O_NOFOLLOW, dir_fd=fd)
            os.close(fd)
            fd = nfd
    except OSError:
        os.close(fd)
        raise
    return fd


def _fail(e, none, pin=True):
    """The row of a file that cannot be reached: ENOENT is absent, anything
    else blocked (errno None where the restatement does not pin it)."""
    if e == errno.ENOENT:
        return ABSENT, False, 0, none
    return BLOCKED, False, e if pin else None, none


def _one(rootfd, h, bs, entry):
    """(state, long, errno or None, [bit per block])."""
    path, _, size, digests = entry
    none = [0] * len(digests)
    comps = [c for c in path.split(b"/") if c]
    try:
        dfd = _open_dir_nofollow(rootfd, comps[:-1])
    except OSError as e:
        # (a symlink in a component's place: ELOOP or ENOTDIR, by the open's flags)
        return _fail(e.errno, none, pin=False)
    try:
        try:
            st = os.stat(comps[-1], dir_fd=dfd, follow_symlinks=False)
        except OSError as e:
            return _fail(e.errno, none)
        if not stat.S_ISREG(st.st_mode):
            return BLOCKED, False, None, none
        if size == 0:  # judged without opening it
            return (COMPLETE, False, 0, []) if st.st_size == 0 else (PARTIAL, True, 0, [])
        try:
            fd = os.open(comps[-1], os.O_RDONLY | os.O_NOFOLLOW, dir_fd=dfd)
        except OSError as e:
            return _fail(e.errno, none)
        with os.fdopen(fd, "rb") as f:
            data = f.read()
        bits = []
        for j, want in enumerate(digests):
            end = min((j + 1) * bs, size)
            bits.append(1 if end <= len(data) and h(data[j * bs:end]) == want else 0)
        if all(bits) and len(data) == size:
            return COMPLETE, False, 0, bits
        return PARTIAL, len(data) > size, 0, bits
    finally:
        os.close(dfd)


def expected(index, root):
    """(bits, states, longs, errnos) of the image at `root`: bits one 0/1 per
    block in global order, the others one per file entry; an errno is None
    where the restatement does not pin it (a blocked file that is not
    regular)."""
    hash_name, bs, _, _ = dirsig_oracle.parse(index)
    h = dirsig_oracle.HASHES[hash_name]
    rootfd = os.open(os.fsencode(str(root)), _DIR)
    try:
        rows = [_one(rootfd, h, bs, e) for e in file_entries(index)]
    finally:
        os.close(rootfd)
    bits = [b for r in rows for b in r[3]]
    return bits, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def bitmap_bytes(bits):
    """The bits as the library lays them out: bit g & 63 of little-endian
    u64 word g >> 6 (so bit g & 7 of byte g >> 3), whole words."""
    out = bytearray(8 * ((len(bits) + 63) // 64))
    for g, b in enumerate(bits):
        if b:
            out[g >> 3] |= 1 << (g & 7)
    return bytes(out)


def expected_missing(index, bits):
    """[(path, byte offset)] of the 0 bits, in index order (fill_blocks'
    queue, src/daemon/tracking/progress.rs:136-151)."""
    _, bs, _, _ = dirsig_oracle.parse(index)
    out, g = [], 0
    for path, _, _, digests in file_entries(index):
        for j in range(len(digests)):
            if not bits[g + j]:
                out.append((path, j * bs))
        g += len(digests)
    return out


def check_index_ok(index, states):
    """The invariant's right-hand side: does cir_check_index pass?"""
    for (_, _, size, _), st in zip(file_entries(index), states):
        if st != COMPLETE and not (size == 0 and st == ABSENT):
            return False
    return True


def same(result, want):
    """Does a BlocksResult carry exactly the restatement's answer?"""
    bits, states, longs, errnos = want
    if result.nblk != len(bits) or result.have != bitmap_bytes(bits):
        return False
    if result.states != states or result.long != longs or len(result.errnos) != len(errnos):
        return False
    for got, st, e in zip(result.errnos, states, errnos):
        if st != BLOCKED:
            good = got == 0
        elif e is None:
            good = got != 0
        else:
            good = got == e
        if not good:
            return False
    return True
