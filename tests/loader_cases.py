"""The descriptor grids the chain loaders are swept over (no test module:
helpers only), and their digests by hashlib.  Nothing here calls the library.

A grid holds one block per (k, t, a): length L = 128 k + t for t in 0..127 (k
whole lines and every tail), start alignment a in 0..15.  Block number i (in
(k, t, a) order) starts at i * stride + a; stride is a multiple of 128 and at
least max L + 32, so no two blocks touch and every block, the last included,
is followed by at least GUARD bytes that belong to no block.  The arena's
bytes are seeded and drawn from 1..255: a loader that takes one byte past a
block's end, drops one before it, or puts SHA-512's 0x80 in the wrong place
hashes another message -- with zero bytes around a block it would often hash
the same one.

The same grid is handed to the library in two orders: `shuffled` (a seeded
permutation: every wave mixes alignment classes, tails and line counts) and
`grouped` (sorted by (a, k, t): whole waves share one alignment class and one
line count, so the loaders' alignment branches are wave-uniform).
"""
import functools
import hashlib

import numpy as np

GUARD = 16
ORDERS = ["shuffled", "grouped"]
HASHES = ["blake2b", "sha512"]

# name: (ks, stride)
#   lane: lengths 0..511 -- at most 4 lines, below the 8 of quad mode; zero to
#         three non-final lines (both exits of the prefetch loop and the
#         skipped loop), SHA-512's pad block at positions 0..3
#   quad: lengths 1024..1535 -- 8..12 lines: quad mode in a batch below 49153
#         (the hand-scheduled loop's count is 6, loop skipped, at k = 8, t = 0
#         and 8, its minimum, for the rest of k = 8; k = 9 leaves a full line
#         and the tail to the general loop; 10 lines at k = 10 and 11)
GRIDS = {"lane": ((0, 1, 2, 3), 640), "quad": ((8, 9, 10, 11), 1664)}
SEEDS = {"lane": 0x10AD0001, "quad": 0x10AD0002}


class Grid:
    def __init__(self, ks, stride, seed):
        ks = tuple(ks)
        assert stride % 128 == 0 and stride >= 128 * max(ks) + 127 + 32
        self.ks, self.stride, self.seed = ks, stride, seed
        k, t, a = np.meshgrid(np.array(ks), np.arange(128), np.arange(16), indexing="ij")
        self.k, self.t, self.a = (x.reshape(-1).astype(np.int64) for x in (k, t, a))
        self.n = self.k.size
        self.lens = (128 * self.k + self.t).astype(np.uint32)
        self.offs = (np.arange(self.n, dtype=np.int64) * stride + self.a).astype(np.uint64)
        rng = np.random.default_rng(seed)
        self.arena = rng.integers(1, 256, size=self.n * stride, dtype=np.uint8)

    def order(self, name):
        """Block numbers in the order the descriptors are handed over."""
        if name == "shuffled":
            return np.random.default_rng(self.seed ^ 0x5F).permutation(self.n)
        if name == "grouped":
            return np.lexsort((self.t, self.k, self.a))
        raise KeyError(name)

    def where(self, mask):
        """Block numbers (in (k, t, a) order) where mask holds."""
        return np.nonzero(mask)[0]


def grid(ks, stride, seed=1):
    return Grid(ks, stride, seed)


@functools.lru_cache(maxsize=None)
def named(name):
    """The lane or the quad grid, built once per process (read only)."""
    ks, stride = GRIDS[name]
    g = Grid(ks, stride, SEEDS[name])
    g.arena.setflags(write=False)
    return g


def have_hashlib(hash_name):
    return hash_name == "blake2b" or "sha512_256" in hashlib.algorithms_available


def digest(hash_name, data, oracle=None):
    """32 digest bytes of `data` (bytes-like) by hashlib; SHA-512/256 by the C
    oracle where this Python's hashlib lacks it (said on stdout)."""
    if hash_name == "blake2b":
        return hashlib.blake2b(data, digest_size=32).digest()
    if hash_name != "sha512":
        raise KeyError(hash_name)
    if have_hashlib("sha512"):
        return hashlib.new("sha512_256", data).digest()
    if oracle is None:
        raise RuntimeError("hashlib has no sha512_256 and no oracle was given")
    import ctypes
    out = ctypes.create_string_buffer(32)
    buf = bytes(data)
    oracle.oracle_sha512_256(out, ctypes.create_string_buffer(buf, max(len(buf), 1)), len(buf))
    return out.raw


def reference(hash_name, arena, offs, lens, oracle=None):
    """n x 32 digest bytes of arena[offs[i] : offs[i] + lens[i]]."""
    if not have_hashlib(hash_name):
        print("loader_cases: hashlib has no sha512_256 here; the reference is the C oracle's")
    mem = memoryview(np.ascontiguousarray(arena))
    out = np.empty((len(offs), 32), dtype=np.uint8)
    for i, (o, ln) in enumerate(zip(offs.tolist(), lens.tolist())):
        out[i] = np.frombuffer(digest(hash_name, mem[o:o + ln], oracle), dtype=np.uint8)
    return out


_REFERENCES = {}


def named_reference(name, hash_name, oracle=None):
    """reference() of a named grid in (k, t, a) order, computed once (read
    only)."""
    if (name, hash_name) not in _REFERENCES:
        g = named(name)
        want = reference(hash_name, g.arena, g.offs, g.lens, oracle)
        want.setflags(write=False)
        _REFERENCES[name, hash_name] = want
    return _REFERENCES[name, hash_name]


def differing(got, want):
    """Rows at which two arrays of n x 32 digest bytes differ."""
    got = np.asarray(got, dtype=np.uint8).reshape(-1, 32)
    want = np.asarray(want, dtype=np.uint8).reshape(-1, 32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.nonzero((got != want).any(axis=1))[0]


def report(got, want, k, t, a, hash_name, entry, order, first=8):
    """None when every digest matches; else the failure message: how many
    differ, the first few as (hash, entry, order, k, t, a), and the distinct t
    and a among them (a loader bug is a pattern in those).  k, t, a: one value
    per row of got / want."""
    bad = differing(got, want)
    if bad.size == 0:
        return None
    k, t, a = (np.asarray(x).reshape(-1) for x in (k, t, a))
    rows = [(hash_name, entry, order, int(k[i]), int(t[i]), int(a[i])) for i in bad[:first]]
    return ("%d of %d digests differ; first (hash, entry, order, k, t, a): %s; "
            "distinct t: %s; distinct a: %s"
            % (bad.size, len(k), rows, sorted(set(t[bad].tolist())),
               sorted(set(a[bad].tolist()))))
