"""Helpers of the cir_index_sketch tests (no test module), shared by the CPU
and the GPU file: digests with chosen sketch keys, made by inverting the mix
(every step of it is invertible, so the last word of a digest can be solved
for any key), and indexes over given digest lists through index_cases' builder.
Nothing here calls the library.
"""
import random
import struct

import index_cases
from sketch_restate import M64, MUL, SEED, key

MUL_INV = pow(MUL, -1, 1 << 64)


def digest_with_key(want, rng):
    """A 32-byte digest whose sketch key is `want`: three random words, the
    fourth solved."""
    words = [rng.getrandbits(64) for _ in range(3)]
    x = SEED
    for w in words:
        x = ((x ^ w) * MUL) & M64
        x ^= x >> 32
    y = want ^ (want >> 32)                 # undo x ^= x >> 32
    last = ((y * MUL_INV) & M64) ^ x        # undo the multiply and the xor
    d = struct.pack("<4Q", *words, last)
    assert key(d) == want
    return d


def random_digests(n, seed):
    rng = random.Random(seed)
    return [rng.randbytes(32) for _ in range(n)]


def prefix_digests(n, seed, top=0):
    """n digests whose keys are distinct, share their top 32 bits (`top`) and
    are spread over the low 32."""
    rng = random.Random(seed)
    lows = rng.sample(range(1 << 32), n)
    return [digest_with_key((top << 32) | lo, rng) for lo in lows]


def index_of(digests, bs=64, per_file=300, hash_name="blake2b/256", seed=0):
    """A canonical index whose block list is `digests`, in order: files of up
    to per_file blocks (the last block of each short), an empty file and a
    symlink between them."""
    rng = random.Random(seed)
    entries, at, fi = [("f", b"empty", False, 0, []), ("s", b"link", b"t")], 0, 0
    while at < len(digests):
        n = min(per_file, len(digests) - at)
        size = (n - 1) * bs + rng.randint(1, bs)
        entries.append(("f", b"f%d" % fi, fi % 5 == 0, size, list(digests[at:at + n])))
        at += n
        fi += 1
    half = len(entries) // 2
    return index_cases.emit([(b"/", entries[:half]), (b"/d", entries[half:])], bs, hash_name)


def cpu_indexes(k):
    """[(name, index)] around a sketch size k: no block, 1, k - 1, k, k + 1
    distinct blocks, one digest 500 times, half the blocks sharing a digest."""
    out = [("no_blocks", index_of([])), ("one_block", index_of(random_digests(1, 1)))]
    for n in (k - 1, k, k + 1):
        out.append(("distinct_%d" % n, index_of(random_digests(n, 10 + n), seed=n)))
    out.append(("one_digest_500_times", index_of(random_digests(1, 2) * 500)))
    d = random_digests(300, 3)
    half = d[:150] + [d[7]] * 150
    random.Random(4).shuffle(half)
    out.append(("half_share_one_digest", index_of(half, hash_name="sha512/256", bs=4096)))
    return out
