"""Input families of the cir_block_sources tests (no test module: helpers
only), shared by the CPU and the GPU file.  Indexes are dirsig_oracle.emit's
over random digests; nothing here calls the library.

cases() -> [(name, index, [source index, ...], want bits or None, tail_ones)].
"""
import random

import dirsig_oracle

BS = 64


def _file(name, size, digests, exe=False):
    assert len(digests) == (size + BS - 1) // BS
    return ("f", name, exe, size, list(digests))


def _emit(dirs, hash_name="blake2b/256", bs=BS):
    return dirsig_oracle.emit(hash_name, bs, dirs, keep_empty=True)


def _named():
    rng = random.Random(20240611)
    d = [rng.randbytes(32) for _ in range(40)]
    out = []
    # a digest present in several sources: the first source wins; and several
    # times inside one source: the first place in index order wins
    new = _emit([(b"/", [_file(b"a", 3 * BS, d[0:3]), _file(b"b", 2 * BS, [d[3], d[0]])])])
    s0 = _emit([(b"/", [_file(b"x", 2 * BS, [d[9], d[1]]), _file(b"y", BS, [d[1]])]),
                (b"/sub", [_file(b"z", 3 * BS, [d[1], d[3], d[3]])])])
    s1 = _emit([(b"/", [_file(b"a", 3 * BS, d[0:3]), _file(b"q", BS, [d[3]])])])
    out.append(("first_source_first_place", new, [s0, s1], None, False))
    out.append(("ranking_reversed", new, [s1, s0], None, False))
    # a short last block matching a short last block of the same length, and a
    # whole block that does not match a short one with the same digest
    new = _emit([(b"/", [_file(b"log", 2 * BS + 10, d[10:13])])])
    s0 = _emit([(b"/old", [_file(b"log.1", BS + 10, [d[10], d[12]])])])
    out.append(("short_matches_short", new, [s0], None, False))
    # a lying source lists a needed digest at a block of another length: not
    # found, counted, and the later honest copy is not taken
    liar = _emit([(b"/", [_file(b"l", BS + 5, [d[11], d[10]])])])       # d[10] as a 5-byte block
    honest = _emit([(b"/", [_file(b"h", 2 * BS, [d[10], d[11]])])])
    out.append(("lying_source_first", new, [liar, honest], None, False))
    out.append(("honest_source_first", new, [honest, liar], None, False))
    # skipped sources in front of and between used ones: ordinals refer to the
    # order given
    other_hash = _emit([(b"/", [_file(b"a", BS, [d[10]])])], hash_name="sha512/256")
    other_bs = _emit([(b"/", [_file(b"a", 32, [d[10]])])], bs=32)
    # (the same header with one hash too few: does not parse)
    broken = honest.replace(b" " + d[11].hex().encode(), b"", 1)
    out.append(("skipped_sources", new,
                [b"garbage\n", s0, other_hash, broken, other_bs, honest, b""], None, False))
    # no sources at all; sources that are all skipped
    out.append(("no_sources", new, [], None, False))
    out.append(("only_skipped", new, [other_hash, b"\x00\x01"], None, False))
    # a new index with no non-empty file
    empty = _emit([(b"/", [_file(b"e", 0, []), ("s", b"l", b"e")]), (b"/d", [])])
    out.append(("no_blocks", empty, [s0, honest], None, False))
    # a source with no blocks
    out.append(("empty_source", new, [empty, honest], None, False))
    # sha512/256 indexes
    new5 = _emit([(b"/", [_file(b"a b", 2 * BS + 1, d[20:23])])], hash_name="sha512/256")
    s5 = _emit([(b"/p", [_file(b"\xffq", BS + 1, [d[21], d[22]], exe=True)])],
               hash_name="sha512/256")
    out.append(("sha512_256", new5, [new, s5], None, False))
    return out


def _random(seed):
    """One random family: a universe of whole-block digests and, per short
    length, of short-block digests, so equal digests mostly mean equal
    lengths; one file in eight draws its last digest from the wrong universe
    (a lying or colliding entry)."""
    rng = random.Random(seed)
    whole = [rng.randbytes(32) for _ in range(rng.choice((6, 40, 300)))]
    short = {n: [rng.randbytes(32) for _ in range(3)] for n in (1, 7, BS - 1)}

    def index(nfiles, prefix):
        dirs = []
        for di in range(rng.randint(1, 3)):
            files = []
            for fi in range(rng.randint(0, nfiles)):
                nfull = rng.choice((0, 0, 1, 2, 3, 7, 70))
                tail = rng.choice((0, 0, 1, 7, BS - 1))
                digests = [rng.choice(whole) for _ in range(nfull)]
                if tail:
                    pick = whole if rng.randrange(8) == 0 else short[tail]
                    digests.append(rng.choice(pick))
                files.append(_file(b"%s%02d" % (prefix, fi), nfull * BS + tail, digests,
                                   exe=rng.random() < 0.2))
            dirs.append((b"/" if di == 0 else b"/d%d" % di, files))
        return _emit(dirs)

    new = index(6, b"n")
    sources = []
    for _ in range(rng.randint(0, 5)):
        sources.append(index(5, b"s") if rng.random() < 0.8 else rng.randbytes(20))
    nblk = sum(len(e[4]) for _, es in dirsig_oracle.parse(new)[2] for e in es if e[0] == "f")
    mode = rng.randrange(3)
    if mode == 0:
        return new, sources, None, False
    bits = [1 if rng.random() < 0.6 else 0 for _ in range(nblk)]
    return new, sources, bits, mode == 2


def cases():
    out = _named()
    # `want` with scattered bits, and with a last word whose bits past nblk are set
    name, new, sources, _, _ = out[0]
    out.append(("want_scattered", new, sources, [1, 0, 1, 0, 1], False))
    out.append(("want_tail_ones", new, sources, [0, 1, 1, 0, 1], True))
    out.append(("want_none_wanted", new, sources, [0] * 5, True))
    for seed in range(40):
        new, sources, bits, tail = _random(1000 + seed)
        out.append(("random_%d" % seed, new, sources, bits, tail))
    return out
