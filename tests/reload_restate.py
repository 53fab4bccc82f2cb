"""Python restatement of cir_reload_blocks' rules and the copy tables
cir_copy_runs and cir_copy_runs_dev are tested on (no test module: helpers
only).  Nothing here calls the library.

The memory rule: block g of the new index is taken from memory exactly when
its file has a destination and some block of some resident buffer -- each
buffer cut into blocks of the index's block size from its own offset 0 -- has
the same digest and the same length.  The digests of the resident bytes come
from the caller's `digest` function (the tests pass the C oracle's).  What is
not taken from memory is judged by tests/blocks_restate.py's walk of the image
directory; a non-empty file all of whose blocks memory gives is never looked
at and is complete and resident whatever the directory holds.

The copy tables: sources and destinations carved out of one buffer (16-byte
aligned base) with guard bytes between them; expected() is that buffer as it
must be afterwards by plain slice copies, and which records are bad is restated
by a sequential walk.
"""
import os
import random
import stat

import numpy as np

import blocks_restate
import dirsig_oracle
from blocks_restate import ABSENT, BLOCKED, COMPLETE, PARTIAL
from links_restate import file_entries

SKIPPED = "skipped"
POISON = 0xA5
GUARD = 48
U64 = (1 << 64) - 1


# ---- the memory rule --------------------------------------------------------------------------

def resident_set(digest, bs, buffers):
    """{(digest, length)} over every block of every resident buffer (bytes)."""
    out = set()
    for data in buffers:
        for at in range(0, len(data), bs):
            blk = bytes(data[at:at + bs])
            out.add((digest(blk), len(blk)))
    return out


def _real(root, path):
    return os.path.join(os.fsencode(str(root)), path.lstrip(b"/"))


def _readable_blocks(root, path, size, bs):
    """The leading blocks of the entry that lie wholly inside the file's length
    (0 when the path is not a regular file reached through real directories)."""
    cur = os.fsencode(str(root))
    for comp in path.lstrip(b"/").split(b"/")[:-1]:
        cur = os.path.join(cur, comp)
        try:
            if not stat.S_ISDIR(os.lstat(cur).st_mode):
                return 0
        except OSError:
            return 0
    try:
        st = os.lstat(_real(root, path))
    except OSError:
        return 0
    if not stat.S_ISREG(st.st_mode):
        return 0
    nblk = (size + bs - 1) // bs
    return nblk if st.st_size >= size else st.st_size // bs


class Expected:
    """bits (0/1 per global block), mem (the same, memory's share), states,
    longs, resident, errnos (one per file entry; an errno is None where
    blocks_restate does not pin it), copied (blocks), copied_bytes, disk_bytes
    (what the pipeline reads: the blocks memory did not give that lie inside
    their file's length, of the files it looks at)."""


def expected(index, root, have, skip=()):
    """have: resident_set(...) of the resident buffers; skip: the ordinals
    without a destination."""
    _, bs, _, _ = dirsig_oracle.parse(index)
    d_bits, d_states, d_longs, d_errnos = blocks_restate.expected(index, root)
    e = Expected()
    e.bits, e.mem, e.states, e.longs, e.resident, e.errnos = [], [], [], [], [], []
    e.copied = e.copied_bytes = e.disk_bytes = 0
    g = 0
    for i, (path, _, size, digests) in enumerate(file_entries(index)):
        n = len(digests)
        lens = [min(bs, size - j * bs) for j in range(n)]
        if size and i in skip:
            e.bits += [0] * n
            e.mem += [0] * n
            e.states.append(SKIPPED)
            e.longs.append(False)
            e.resident.append(False)
            e.errnos.append(0)
            g += n
            continue
        mem = [1 if (digests[j], lens[j]) in have else 0 for j in range(n)]
        e.mem += mem
        e.copied += sum(mem)
        e.copied_bytes += sum(l for l, m in zip(lens, mem) if m)
        if n and all(mem):                      # never looked at
            e.bits += mem
            e.states.append(COMPLETE)
            e.longs.append(False)
            e.resident.append(True)
            e.errnos.append(0)
            g += n
            continue
        disk = d_bits[g:g + n]
        st, lg, err = d_states[i], d_longs[i], d_errnos[i]
        e.resident.append(False)
        if st in (ABSENT, BLOCKED):
            e.bits += mem                       # what memory gave stays
            e.states.append(st)
            e.longs.append(False)
            e.errnos.append(err)
        else:
            bits = [m | d for m, d in zip(mem, disk)]
            e.bits += bits
            whole = size == 0 or os.lstat(_real(root, path)).st_size == size
            e.states.append(st if size == 0 else COMPLETE if all(bits) and whole else PARTIAL)
            e.longs.append(lg)
            e.errnos.append(0)
            nread = _readable_blocks(root, path, size, bs)
            e.disk_bytes += sum(lens[j] for j in range(min(n, nread)) if not mem[j])
        g += n
    return e


def same(result, e):
    """Does a BlocksResult carry exactly the restatement's answer?"""
    if not blocks_restate.same(result, (e.bits, e.states, e.longs, e.errnos)):
        return False
    return result.resident == e.resident


# ---- the copy tables --------------------------------------------------------------------------

LENS = [1, 15, 16, 17, 31, 32, 33, 100, 1000, 4101]
NAMES = ["empty", "one", "two", "hundred28", "thousand", "malformed"]


def units(nbytes):
    return (nbytes + 15) // 16


class CopyCase:
    def __init__(self, name, shapes, seed):
        """shapes: [(bytes, source alignment, destination alignment)]."""
        rng = random.Random(seed)
        self.name = name
        self.recs = []                                 # [unit_first, src off, dst off, bytes]
        pos, first = GUARD, 0
        for nbytes, sa, _ in shapes:                   # the sources, then the destinations
            pos = ((pos + GUARD + 15) & ~15) + sa
            self.recs.append([first, pos, 0, nbytes])
            first += units(nbytes)
            pos += nbytes
        for r, (nbytes, _, da) in zip(self.recs, shapes):
            pos = ((pos + GUARD + 15) & ~15) + da
            r[2] = pos
            pos += nbytes
        self.buf_bytes = pos + GUARD
        self.nunits = first
        self.given_nunits = first
        self.nruns = len(self.recs)
        self.initial = np.full(self.buf_bytes, POISON, dtype=np.uint8)
        for _, s, _, n in self.recs:
            self.initial[s:s + n] = np.frombuffer(rng.randbytes(n), dtype=np.uint8)
        self.sound = [list(r) for r in self.recs]

    def table(self, base):
        assert base % 16 == 0
        t = np.zeros(4 * max(self.nruns, 1), dtype=np.uint64)
        for i, (first, s, d, n) in enumerate(self.recs):
            t[4 * i:4 * i + 4] = [first & U64, base + s, base + d, n & U64]
        return t

    @property
    def bad(self):
        out = []
        for r, (first, _, _, nbytes) in enumerate(self.recs):
            want = self.recs[r - 1][0] + units(self.recs[r - 1][3]) if r else 0
            b = nbytes == 0 or first != want
            if r + 1 == self.nruns:
                b = b or first + units(nbytes) != self.given_nunits
            out.append(b)
        return out

    @property
    def nbad(self):
        return sum(self.bad)

    def expected(self):
        want = self.initial.copy()
        for (_, s, d, n), bad in zip(self.sound, self.bad):
            if not bad:
                want[d:d + n] = self.initial[s:s + n]
        return want


def copy_case(name):
    if name == "empty":
        return CopyCase(name, [], 0)
    if name == "one":
        return CopyCase(name, [(33, 5, 11)], 1)
    if name == "two":
        return CopyCase(name, [(4101, 3, 0), (17, 0, 8)], 2)
    if name == "hundred28":
        return CopyCase(name, [(LENS[i % 10], (5 * i) % 16, (3 * i + 1) % 16) for i in range(128)], 3)
    if name == "thousand":
        # every one of the 16 x 16 alignment pairs, every length at several of
        # them; some 40,000 units: more than 150 workgroups of 256
        shapes = [(LENS[(i // 7) % 10], (i % 256) // 16, i % 16) for i in range(1000)]
        assert len({(s, d) for _, s, d in shapes}) == 256
        return CopyCase(name, shapes, 4)
    if name == "malformed":
        c = CopyCase(name, [(LENS[i % 10], (7 * i) % 16, (11 * i + 2) % 16) for i in range(60)], 5)
        c.recs[10][3] = 0                     # zero bytes (11 no longer follows)
        c.recs[30][0] += 1                    # a wrong unit_first (31 follows not)
        c.given_nunits = c.nunits + 1         # the last record does not end at nunits
        assert [i for i, b in enumerate(c.bad) if b] == [10, 11, 30, 31, 59]
        return c
    raise KeyError(name)
