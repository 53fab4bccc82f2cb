"""The scatter tables cir_scatter_runs and cir_scatter_runs_dev are tested on
(no test module: helpers only), and their expected result by plain slice
copies.  Nothing here calls the library.

A case is a source of random bytes, records {src_pos, place in the
destination buffer, bytes} and, for the malformed case, the damage done to
some of them.  The destinations are carved out of one buffer (16-byte aligned
base) with at least GUARD bytes between them; expected() is that buffer as it
must be afterwards: the poison everywhere but in the sound records'
destinations.  Which records are bad is restated here by a sequential walk
(ciruela_amd/csrc/scatter.hpp's rule in ten lines).
"""
import random

import numpy as np

POISON = 0xA5
GUARD = 32
U64 = (1 << 64) - 1
LENS = [1, 15, 16, 17, 31, 32, 33, 4101]
NAMES = ["mixed", "one", "two", "thousand", "empty", "malformed"]


def units(nbytes):
    return (nbytes + 15) // 16


class Case:
    def __init__(self, name, src, recs):
        """recs: [[unit_first, src_pos, dst offset in the buffer, bytes]] as sound."""
        self.name = name
        self.src = src
        self.src_bytes = len(src)
        self.sound = [list(r) for r in recs]
        self.recs = [list(r) for r in recs]       # as handed to the library
        self.nunits = sum(units(r[3]) for r in recs)
        self.nruns = len(recs)
        end = max([r[2] + r[3] for r in recs], default=0)
        self.buf_bytes = end + GUARD

    def table(self, base):
        """The records as u64 words, destinations at base + offset."""
        assert base % 16 == 0
        t = np.zeros(4 * self.nruns, dtype=np.uint64)
        for i, (first, pos, off, nbytes) in enumerate(self.recs):
            t[4 * i:4 * i + 4] = [first & U64, pos & U64, (base + off) & U64, nbytes & U64]
        return t

    @property
    def bad(self):
        out = []
        for r, (first, pos, _, nbytes) in enumerate(self.recs):
            b = pos % 16 != 0 or nbytes == 0 or nbytes > self.src_bytes or \
                pos > self.src_bytes - nbytes
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
    """shapes: [(bytes, destination alignment)] -> a sound case."""
    rng = random.Random(seed)
    recs, spos, dpos, first = [], 0, GUARD, 0
    for nbytes, align in shapes:
        spos = (spos + 15) & ~15
        dpos = ((dpos + GUARD + 15) & ~15) + align
        recs.append([first, spos, dpos, nbytes])
        first += units(nbytes)
        spos += nbytes
        dpos += nbytes
    src = np.frombuffer(rng.randbytes(max(spos, 1)), dtype=np.uint8)[:spos].copy()
    return Case(name, src, recs)


def build(name):
    if name == "mixed":
        # every length at every alignment: 4,304 units (17 workgroups of 256); the
        # 4101-byte runs (257 units) cross wave and workgroup boundaries
        return _lay_out(name, [(n, a) for a in range(16) for n in LENS], 1)
    if name == "one":
        return _lay_out(name, [(33, 5)], 2)
    if name == "two":
        return _lay_out(name, [(4101, 3), (17, 8)], 3)
    if name == "thousand":
        rng = random.Random(4)
        return _lay_out(name, [(rng.choice(LENS[:7]), rng.randrange(16)) for _ in range(1000)], 4)
    if name == "empty":
        return Case(name, np.zeros(0, dtype=np.uint8), [])
    if name == "malformed":
        c = _lay_out(name, [(n, (3 * a + 1) % 16) for a in range(8) for n in LENS], 5)
        r = c.recs
        r[3][1] += 8                                  # a misaligned src_pos
        r[10][3] = 0                                  # zero bytes (11 no longer follows)
        r[20][1] = ((c.src_bytes + 15) & ~15) + 16    # the source starts past the slot
        r[30][3] = c.src_bytes - r[30][1] + 1         # ... ends one byte past it (31 follows not)
        r[40][0] += 1                                 # a wrong unit_first (41 follows not)
        r[50][1], r[50][3] = U64 - 15, 32             # src_pos + bytes wraps around 2^64
        assert [i for i, b in enumerate(c.bad) if b] == [3, 10, 11, 20, 30, 31, 40, 41, 50, 51]
        return c
    raise KeyError(name)


def expected(case):
    want = np.full(case.buf_bytes, POISON, dtype=np.uint8)
    for (_, pos, off, nbytes), bad in zip(case.recs, case.bad):
        if not bad:
            want[off:off + nbytes] = case.src[pos:pos + nbytes]
    return want
