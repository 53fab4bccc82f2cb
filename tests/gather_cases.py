"""The gather tables cir_gather_runs and cir_gather_runs_dev are tested on (no
test module: helpers only), and their expected result by plain slice copies.
Nothing here calls the library.

A case is one source allocation -- the poison everywhere but in the records'
sources, which lie at every alignment with at least GUARD bytes between them --
records {dst_pos, place in the source allocation, bytes} and, for the
malformed case, the damage done to some of them.  expected() is the destination
buffer as it must be afterwards: the poison everywhere but in the sound
records' ranges, which hold the source bytes and zeros up to the next multiple
of 16.  Which records are bad is restated here by a sequential walk
(ciruela_amd/csrc/gather.hpp's rule in ten lines).
"""
import random

import numpy as np

POISON = 0xA5
GUARD = 32
U64 = (1 << 64) - 1
LENS = [1, 15, 16, 17, 31, 32, 33, 4101]
NAMES = ["mixed", "one", "two", "hundred", "thousand", "empty", "malformed"]


def units(nbytes):
    return (nbytes + 15) // 16


class Case:
    def __init__(self, name, src, recs, dst_bytes):
        """recs: [[unit_first, dst_pos, src offset in the allocation, bytes]] as sound."""
        self.name = name
        self.src = src                            # the whole source allocation
        self.recs = [list(r) for r in recs]       # as handed to the library
        self.nunits = sum(units(r[3]) for r in recs)
        self.nruns = len(recs)
        self.dst_bytes = dst_bytes                # what the library is told
        self.buf_bytes = dst_bytes + GUARD        # what is allocated and compared

    def table(self, base):
        """The records as u64 words, sources at base + offset."""
        t = np.zeros(4 * self.nruns, dtype=np.uint64)
        for i, (first, pos, off, nbytes) in enumerate(self.recs):
            t[4 * i:4 * i + 4] = [first & U64, pos & U64, (base + off) & U64, nbytes & U64]
        return t

    @property
    def bad(self):
        out = []
        for r, (first, pos, _, nbytes) in enumerate(self.recs):
            b = pos % 16 != 0 or nbytes == 0 or pos + 16 * units(nbytes) > self.dst_bytes
            want = self.recs[r - 1][0] + units(self.recs[r - 1][3]) if r else 0
            b = b or first != want
            if r + 1 == self.nruns:
                b = b or first + units(nbytes) != self.nunits
            out.append(b)
        return out

    @property
    def nbad(self):
        return sum(self.bad)


def _lay_out(name, shapes, seed):
    """shapes: [(bytes, source alignment)] -> a sound case.  The allocation's
    base is taken as 16-byte aligned."""
    rng = random.Random(seed)
    recs, spos, dpos, first = [], 0, 0, 0
    for nbytes, align in shapes:
        spos = ((spos + GUARD + 15) & ~15) + align
        dpos = (dpos + 15) & ~15
        recs.append([first, dpos, spos, nbytes])
        first += units(nbytes)
        spos += nbytes
        dpos += nbytes
    src = np.full(spos + GUARD, POISON, dtype=np.uint8)
    for _, _, off, nbytes in recs:
        src[off:off + nbytes] = np.frombuffer(rng.randbytes(nbytes), dtype=np.uint8)
    # the destination ends with the last record's rounded range, or 16 bytes behind it
    return Case(name, src, recs, ((dpos + 15) & ~15) + (16 if seed % 2 else 0))


def build(name):
    if name == "mixed":
        # every length at every alignment: 4,304 units (17 workgroups of 256); the
        # 4101-byte runs (257 units) cross wave and workgroup boundaries
        return _lay_out(name, [(n, a) for a in range(16) for n in LENS], 1)
    if name == "one":
        return _lay_out(name, [(33, 5)], 2)
    if name == "two":
        return _lay_out(name, [(4101, 3), (17, 8)], 3)
    if name == "hundred":
        return _lay_out(name, [(LENS[i % 8], (5 * i) % 16) for i in range(128)], 6)
    if name == "thousand":
        rng = random.Random(4)
        return _lay_out(name, [(rng.choice(LENS[:7]), rng.randrange(16)) for _ in range(1000)], 4)
    if name == "empty":
        return Case(name, np.full(GUARD, POISON, dtype=np.uint8), [], 0)
    if name == "malformed":
        c = _lay_out(name, [(n, (3 * a + 1) % 16) for a in range(8) for n in LENS], 5)
        r = c.recs
        r[3][1] += 8                                  # a misaligned dst_pos
        r[10][3] = 0                                  # zero bytes (11 no longer follows)
        r[20][1] = c.dst_bytes + 16                   # the range starts past the destination
        r[30][3] = c.dst_bytes - r[30][1] + 1         # ... ends past it (31 follows not)
        r[40][0] += 1                                 # a wrong unit_first (41 follows not)
        r[50][1], r[50][3] = U64 - 15, 32             # dst_pos + bytes wraps around 2^64
        r[60][3] = U64                                # 16 * units(bytes) wraps (61 follows not)
        assert [i for i, b in enumerate(c.bad) if b] == \
            [3, 10, 11, 20, 30, 31, 40, 41, 50, 51, 60, 61]
        return c
    raise KeyError(name)


def expected(case):
    want = np.full(case.buf_bytes, POISON, dtype=np.uint8)
    for (_, pos, off, nbytes), bad in zip(case.recs, case.bad):
        if not bad:
            want[pos:pos + 16 * units(nbytes)] = 0
            want[pos:pos + nbytes] = case.src[off:off + nbytes]
    return want
