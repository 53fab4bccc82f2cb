"""Input families of the cir_block_repeats tests (no test module: helpers
only), shared by the CPU and the GPU file.  Indexes are dirsig_oracle.emit's
over random digests; nothing here calls the library.

cases() -> [(name, index, want bits or None, present bits or None, tail_ones)];
tail_ones sets the bits past the last block in both bitmaps' last word.
"""
import random

import dirsig_oracle
from sources_cases import BS, _emit, _file


def _named():
    rng = random.Random(20250920)
    d = [rng.randbytes(32) for _ in range(40)]
    short = rng.randbytes(32)
    out = []
    # a duplicated file: one extent, from the first copy, which is fetched
    new = _emit([(b"/", [_file(b"a", 4 * BS, d[0:4]), _file(b"b", 4 * BS, d[0:4])])])
    out.append(("duplicated_file", new, None, None, False))
    new = _emit([(b"/", [_file(b"a", 3 * BS + 9, d[0:3] + [short]),
                         _file(b"b", 3 * BS + 9, d[0:3] + [short])])])
    out.append(("duplicated_file_short_tail", new, None, None, False))
    # a zero-filled file: every block repeats the first
    new = _emit([(b"/", [_file(b"pre", BS, [d[5]]), _file(b"zero", 5 * BS, [d[9]] * 5)])])
    out.append(("zero_filled_file", new, None, None, False))
    # the same file in two directories, other files around it
    new = _emit([(b"/", [_file(b"top", 2 * BS, d[10:12])]),
                 (b"/vendor/x", [_file(b"lib.so", 3 * BS, d[0:3]), _file(b"own", BS, [d[12]])]),
                 (b"/y", [_file(b"first", BS, [d[13]]), _file(b"lib.so", 3 * BS, d[0:3], exe=True)])])
    out.append(("across_two_directories", new, None, None, False))
    # wanted, present, wanted with the same digests: the later present copy
    # beats the earlier wanted one, for both
    three = _emit([(b"/", [_file(b"a", 2 * BS, d[0:2]), _file(b"b", 2 * BS, d[0:2]),
                           _file(b"c", 2 * BS, d[0:2])])])
    out.append(("present_beats_earlier_wanted", three, [1, 1, 0, 0, 1, 1], [0, 0, 1, 1, 0, 0],
                False))
    # two present holders: the smaller wins
    out.append(("two_present_holders", three, [0, 0, 0, 0, 1, 1], [1, 1, 1, 1, 0, 0], False))
    # a block that is neither wanted nor present is never a source
    out.append(("neither_is_never_a_source", three, [0, 0, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0], False))
    out.append(("neither_without_present", three, [0, 0, 1, 1, 1, 0], None, False))
    # a bit in both bitmaps means wanted: c copies from a as from a fetched block
    out.append(("bit_in_both_is_wanted", three, [1, 1, 0, 0, 1, 1], [1, 1, 0, 0, 0, 0], False))
    # a short last block with a full block's digest: dropped, stays in fetch,
    # and the block in front of it still repeats
    new = _emit([(b"/", [_file(b"a", 2 * BS, d[0:2]), _file(b"b", BS + 5, [d[1], d[0]])])])
    out.append(("short_equals_full_dropped", new, None, None, False))
    # nothing wanted; and the same with tail ones
    out.append(("want_all_zeros", three, [0] * 6, [1] * 6, False))
    out.append(("tail_ones_in_both", three, [0, 0, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0], True))
    out.append(("tail_ones_nothing_set", three, [0] * 6, [0] * 6, True))
    # sha512/256
    new = _emit([(b"/", [_file(b"a b", 2 * BS + 1, d[20:23]),
                         _file(b"\xffq", 2 * BS + 1, d[20:23], exe=True)])],
                hash_name="sha512/256")
    out.append(("sha512_256", new, None, None, False))
    # no blocks at all; no repeats at all
    empty = _emit([(b"/", [_file(b"e", 0, []), ("s", b"l", b"e")]), (b"/d", [])])
    out.append(("no_blocks", empty, None, None, False))
    new = _emit([(b"/", [_file(b"a", 3 * BS, d[0:3]), _file(b"b", 2 * BS + 1, d[3:6])])])
    out.append(("no_repeats", new, None, None, False))
    # a stretch whose leaders change class in the middle: a's first block is
    # present, its second wanted, and b repeats both
    new = _emit([(b"/", [_file(b"a", 2 * BS, d[0:2]), _file(b"b", 2 * BS, d[0:2])])])
    out.append(("class_change_breaks", new, [0, 1, 1, 1], [1, 0, 0, 0], False))
    return out


def nblocks(index):
    return sum(len(e[4]) for _, es in dirsig_oracle.parse(index)[2] for e in es if e[0] == "f")


def random_index(rng, nfiles, universe, copy_rate=0.3):
    """Files of a few blocks drawn from a small universe; some files are
    copies of earlier ones, some have short tails (one in eight of those with a
    digest of the wrong universe: a lying or colliding entry)."""
    whole = [rng.randbytes(32) for _ in range(universe)]
    short = {t: [rng.randbytes(32) for _ in range(2)] for t in (1, 7, BS - 1)}
    dirs, made = [], []
    for di in range(rng.randint(1, 3)):
        files = []
        for fi in range(nfiles):
            if made and rng.random() < copy_rate:
                size, digests = rng.choice(made)
            else:
                nfull = rng.choice((0, 1, 2, 3, 7, 70))
                tail = rng.choice((0, 0, 1, 7, BS - 1))
                digests = [rng.choice(whole) for _ in range(nfull)]
                if tail:
                    digests.append(rng.choice(whole if rng.randrange(8) == 0 else short[tail]))
                size = nfull * BS + tail
                made.append((size, digests))
            files.append(_file(b"f%02d" % fi, size, digests, exe=rng.random() < 0.2))
        dirs.append((b"/" if di == 0 else b"/d%d" % di, files))
    return _emit(dirs)


def _random(seed):
    rng = random.Random(seed)
    new = random_index(rng, rng.randint(1, 6), rng.choice((4, 30, 200)))
    n = nblocks(new)
    mode = rng.randrange(4)
    want = None if mode == 0 else [1 if rng.random() < 0.6 else 0 for _ in range(n)]
    present = None if mode in (0, 1) else [1 if rng.random() < 0.5 else 0 for _ in range(n)]
    return new, want, present, mode == 3


def cases():
    out = _named()
    for seed in range(24):
        new, want, present, tail = _random(3000 + seed)
        out.append(("random_%d" % seed, new, want, present, tail))
    return out
