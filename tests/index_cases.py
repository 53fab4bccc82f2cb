"""Helpers of the cir_index_digests tests (no test module), shared by the CPU
and the GPU file.  Indexes are dirsig_oracle.emit's over random digests, so no
file needs hashing; expected values are dirsig_oracle.parse's.  Nothing here
calls the library.
"""
import random

import numpy as np

import dirsig_oracle

HASH_CODES = {"blake2b/256": 1, "sha512/256": 2}


def nblocks(size, bs):
    return (size + bs - 1) // bs


def file_entry(rng, name, size, bs, exe=False):
    return ("f", name, exe, size, [rng.randbytes(32) for _ in range(nblocks(size, bs))])


def emit(dirs, bs=64, hash_name="blake2b/256"):
    return dirsig_oracle.emit(hash_name, bs, dirs, keep_empty=True)


def expected(index):
    """(hash code, block size, digests (nblk, 32) u8, runs (nruns, 4) u64,
    file entries) of a canonical index, from dirsig_oracle.parse and a search
    of the text for each entry's line (hash_off = the offset of the first
    token's leading space)."""
    hash_name, bs, dirs, _ = dirsig_oracle.parse(index)
    digests, runs = [], []
    nfiles = blk = 0
    pos = index.index(b"\n") + 1
    for vpath, entries in dirs:
        assert index[pos:pos + len(vpath) + 1] == vpath + b"\n"
        pos += len(vpath) + 1
        for e in entries:
            end = index.index(b"\n", pos)
            if e[0] == "f":
                if e[4]:
                    head = b"  " + e[1] + (b" x " if e[2] else b" f ") + str(e[3]).encode()
                    assert index[pos:pos + len(head)] == head
                    runs.append((blk, e[3], nfiles, pos + len(head)))
                    digests += e[4]
                    blk += len(e[4])
                nfiles += 1
            pos = end + 1
    d = np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32)
    r = np.array(runs, dtype=np.uint64).reshape(-1, 4)
    return HASH_CODES[hash_name], bs, d, r, nfiles


def same(res, exp):
    """Does an IndexDigests equal an expected() tuple?"""
    return (res.hash_type == exp[0] and res.block_size == exp[1] and
            res.digests.shape == exp[2].shape and bool((res.digests == exp[2]).all()) and
            res.runs.shape == exp[3].shape and bool((res.runs == exp[3]).all()) and
            res.nfiles == exp[4])


def random_index(seed, max_bytes=65536):
    """A seeded random small canonical index: directories with escaped names,
    empty files, exe entries, symlinks, short last blocks; both hash types and
    several block sizes."""
    rng = random.Random(seed)
    bs = rng.choice((1, 7, 64, 4096, 32768))
    hash_name = rng.choice(("blake2b/256", "sha512/256"))
    dirs, budget = [], max_bytes - 200
    for di in range(rng.randint(0, 4)):
        entries = []
        for fi in range(rng.randint(0, 12)):
            name = rng.choice((b"f", b"a b", b"\xffq", b"...", b".x", b"back\\slash", b"UP")) + \
                b"%d" % fi
            kind = rng.randrange(8)
            if kind == 0:
                entries.append(("s", name, rng.choice((b"../t g", b"/abs", b"x"))))
                continue
            nb = rng.choice((0, 0, 1, 1, 2, 3, 9, 40, 300))
            if 65 * nb + 100 > budget:
                nb = 0
            budget -= 65 * nb + 100
            size = 0 if nb == 0 else (nb - 1) * bs + rng.randint(1, bs)
            entries.append(file_entry(rng, name, size, bs, exe=kind == 1))
        dirs.append((b"/" if di == 0 else b"/d%d/s p" % di, entries))
    return emit(dirs, bs, hash_name)


def mutate(index, seed):
    """One mutation of an index (bytes): a flipped byte, a deleted or doubled
    space, a swapped case, a truncated line, an injected escape or raw byte, a
    changed size."""
    rng = random.Random(seed)
    s = bytearray(index)
    at = rng.randrange(len(s))
    kind = rng.randrange(8)
    if kind == 0:
        s[at] ^= rng.randint(1, 255)
    elif kind in (1, 2):
        p = s.find(b" ", at)
        if p >= 0:
            if kind == 1:
                del s[p]
            else:
                s.insert(p, 0x20)
    elif kind == 3:
        p = at
        while p < len(s) and not chr(s[p]).isalpha():
            p += 1
        if p < len(s):
            s[p] ^= 0x20
    elif kind == 4:
        e = s.find(b"\n", at)
        if e >= 0:
            del s[at:e]
    elif kind == 5:
        s[at:at] = rng.choice((b"\\x2e", b"\\x2f", b"\\x00", b"\\x41", b"\\x4"))
    elif kind == 6:
        s[at:at] = rng.choice((b"\t", b"\r", b"\x00", b"\x80", b"\n"))
    else:
        p = s.find(b" f ", at)
        if p >= 0 and chr(s[p + 3]).isdigit():
            s[p + 3:p + 4] = rng.choice((b"9", b"0", b"18446744073709551615", b""))
    return bytes(s)
