"""The rule of cir_index_sketch and cir_sketch_rank restated in plain Python
(test helper, no test module): the key of a digest, the sketch of an index,
the blob, the overlap of two sketches and the ranking.  Nothing here calls the
library; the text it restates is include/ciruela_blockhash.h's.
"""
import struct
from fractions import Fraction

import dirsig_oracle

M64 = (1 << 64) - 1
SEED = 0x243F6A8885A308D3
MUL = 0x9E3779B97F4A7C15
MAGIC = b"CIRSKv1\0"
MAX_K = 4096
HASH_CODES = {"blake2b/256": 1, "sha512/256": 2}


def key(digest):
    assert len(digest) == 32
    x = SEED
    for w in struct.unpack("<4Q", digest):
        x = ((x ^ w) * MUL) & M64
        x ^= x >> 32
    return x


def keys_of(digests, k):
    """The sketch of a list of 32-byte digests: the k smallest distinct keys."""
    return sorted({key(d) for d in digests})[:k]


def index_blocks(index):
    """(hash code, block size, [digest of every block of every file entry])."""
    hash_name, bs, dirs, _ = dirsig_oracle.parse(index)
    blocks = []
    for _, entries in dirs:
        for e in entries:
            if e[0] == "f":
                blocks += e[4]
    return HASH_CODES[hash_name], bs, blocks


def blob(hash_code, k, bs, n_blocks, keys):
    return MAGIC + struct.pack("<IIQQQ", hash_code, k, bs, n_blocks, len(keys)) + \
        b"".join(struct.pack("<Q", x) for x in keys)


def sketch(index, k=1024):
    hash_code, bs, blocks = index_blocks(index)
    return blob(hash_code, k, bs, len(blocks), keys_of(blocks, k))


def parse(b):
    """A valid blob as (hash code, k, block size, n_blocks, keys), else None."""
    if b is None or len(b) < 40 or b[:8] != MAGIC:
        return None
    hash_code, k, bs, n_blocks, count = struct.unpack("<IIQQQ", b[8:40])
    if not 1 <= k <= MAX_K or count > k or count > n_blocks or len(b) != 40 + 8 * count:
        return None
    keys = list(struct.unpack("<%dQ" % count, b[40:]))
    if any(a >= c for a, c in zip(keys, keys[1:])):
        return None
    return hash_code, k, bs, n_blocks, keys


def overlap(need, src):
    """(shared, examined) of two parsed blobs."""
    def reach(p):
        return p[4][-1] if len(p[4]) == p[1] else M64
    tau = min(reach(need), reach(src))
    mine = [x for x in need[4] if x <= tau]
    held = set(src[4])
    return sum(1 for x in mine if x in held), len(mine)


def rank(need, sources):
    """(CIR_EPARSE?, [(ordinal, shared, examined)] best first, skipped)."""
    n = parse(need)
    if n is None:
        return "EPARSE", [], 0
    rows, skipped = [], 0
    for i, s in enumerate(sources):
        p = parse(s)
        if p is None or p[0] != n[0] or p[2] != n[2]:
            skipped += 1
            continue
        sh, ex = overlap(n, p)
        rows.append((i, sh, ex))
    rows.sort(key=lambda r: (-(Fraction(r[1], r[2]) if r[2] else Fraction(0)), r[0]))
    return None, rows, skipped
