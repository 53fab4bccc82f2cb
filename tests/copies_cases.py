"""Input families of the cir_file_copies tests (no test module: helpers only),
shared by the CPU and the GPU file.  Indexes are index_cases.emit's over random
digests (files_cases.f), so every text is in the device's canonical subset
unless the family says otherwise (skipped sources are garbage on purpose);
expected values are copies_restate's.  Nothing here calls the library.

families() -> [(name, index, [source index, ...], skip or None)]
"""
import random

import files_cases
import index_cases

BS = files_cases.BS
f = files_cases.f
emit = index_cases.emit


def at(entry, name, exe=None):
    """The same content under another name (and, if given, another exe flag)."""
    return ("f", name, entry[2] if exe is None else exe, entry[3], entry[4])


def families():
    rng = random.Random(20261020)
    out = []
    # a directory with a version in its name
    run, a, b, conf = f(rng, b"run", 3, exe=True), f(rng, b"a.so", 5), f(rng, b"b.so", 1, short=9), \
        f(rng, b"conf", 2)
    old = emit([(b"/", [conf]), (b"/app-1.2.3", []), (b"/app-1.2.3/bin", [run]),
                (b"/app-1.2.3/lib", [a, b])])
    new = emit([(b"/", [conf]), (b"/app-1.2.4", []), (b"/app-1.2.4/bin", [run]),
                (b"/app-1.2.4/lib", [a, b, f(rng, b"c.so", 2)])])
    out.append(("renamed_dir", new, [old], None))
    out.append(("renamed_dir_unlinked", new, [old], [0]))      # (what the same-path rule linked)
    # one content under three paths of one source: the first in index order
    x = f(rng, b"x", 4)
    three = emit([(b"/", [f(rng, b"other", 4)]), (b"/a", [at(x, b"p")]), (b"/b", [at(x, b"q")]),
                  (b"/c", [at(x, b"x")])])
    out.append(("three_paths_one_source", emit([(b"/c", [x])]), [three], None))
    # the same content in sources 0 and 2
    s0 = emit([(b"/old", [at(x, b"moved")])])
    s1 = emit([(b"/c", [f(rng, b"x", 4)])])
    s2 = emit([(b"/c", [x])])
    out.append(("sources_0_and_2", emit([(b"/c", [x])]), [s0, s1, s2], None))
    out.append(("sources_2_only", emit([(b"/c", [x])]), [s1, s1, s2], None))
    # equal digests, the exe flag flipped; equal digests, another size in the last block
    out.append(("exe_flip", emit([(b"/", [x])]), [emit([(b"/", [at(x, b"x", exe=True)])])], None))
    shorter = ("f", b"x", False, x[3] - 5, x[4])
    out.append(("last_block_size", emit([(b"/", [x])]), [emit([(b"/", [shorter])])], None))
    # empty files on both sides
    e0, e1 = f(rng, b"e0", 0), f(rng, b"e1", 0, exe=True)
    out.append(("empty_files", emit([(b"/", [e0, e1, x])]),
                [emit([(b"/z", [at(e0, b"k"), at(e1, b"l"), e0, e1])])], None))
    # skip bits at 0, 63, 64 and 65 of 70 files that all have a candidate
    many = [f(rng, b"n%02d" % i, 1 + i % 3) for i in range(70)]
    old_many = emit([(b"/v1", many)])
    new_many = emit([(b"/v2", many)])
    out.append(("skip_bits", new_many, [old_many], [0, 63, 64, 65]))
    out.append(("skip_none_of_70", new_many, [old_many], None))
    out.append(("skip_all_of_70", new_many, [old_many], list(range(70))))
    # skipped sources: a bad frame, another block size; the ordinals of the others stay
    other_bs = index_cases.emit([(b"/", [f(rng, b"x", 2, bs=128)])], bs=128)
    out.append(("skipped_sources", emit([(b"/c", [x])]),
                [random.Random(3).randbytes(300), other_bs, s1, b"", s0, s2], None))
    out.append(("no_sources", new, [], None))
    out.append(("no_files", emit([(b"/", [("s", b"l", b"t")])]), [old], None))
    out.append(("only_empty_sources", new, [emit([(b"/", [])])], None))
    # a source path with \xNN escapes and a space
    out.append(("escaped_source_path", emit([(b"/plain", [at(x, b"name")])]),
                [emit([(b"/sp ace", []), (b"/sp ace/\xff\x01dir", [at(x, b"back\\slash and space")])])],
                None))
    out.append(("escaped_root_name", emit([(b"/plain", [at(x, b"name")])]),
                [emit([(b"/", [at(x, b"\x7f top")])])], None))
    # candidates at the entry's own path beside moved ones (stats[9])
    out.append(("own_path_and_moved", emit([(b"/", [conf, at(x, b"was-x")]), (b"/d", [a])]),
                [emit([(b"/", [conf, x]), (b"/d", [a, at(conf, b"copy")])])], None))
    # 70-block files: a file's blocks cross a wave in the fold; a swapped pair of digests differs
    big = f(rng, b"big", 70)
    swapped = ("f", b"big", False, big[3], [big[4][1], big[4][0]] + big[4][2:])
    out.append(("big_files", emit([(b"/n", [big, at(swapped, b"sw")])]),
                [emit([(b"/o", [at(swapped, b"first"), at(big, b"second")])])], None))
    return out


def random_case(seed, max_files=12, nsrc_max=5):
    """A seeded random family over a small universe of contents and a larger
    one of paths, so that moved files, contents held several times, empty
    files, exe flips and short last blocks abound.  Returns (index, sources,
    skip)."""
    rng = random.Random(seed)
    bs = rng.choice((1, 7, BS))
    dirs = [b"/", b"/d", b"/d/e", b"/sp ace", b"/v-%d" % rng.randrange(3)]
    names = [b"a", b"b", b"A", b"c d", b"\xffq", b"long-name-%d" % rng.randrange(3)]
    contents = []
    for _ in range(6):
        n = rng.choice((0, 1, 1, 2, 5, 70))
        size = 0 if n == 0 else (n - 1) * bs + (bs if rng.random() < 0.7 else rng.randint(1, bs))
        contents.append((size, [rng.randbytes(32) for _ in range(n)]))

    def one_index(nfiles):
        per = {}
        for _ in range(rng.randint(0, nfiles)):
            size, digests_ = rng.choice(contents)
            digests_ = list(digests_)
            if digests_ and rng.random() < 0.1:
                digests_[rng.randrange(len(digests_))] = rng.randbytes(32)
            per.setdefault(rng.choice(dirs), []).append(
                ("f", rng.choice(names), rng.random() < 0.15, size, digests_)
                if rng.random() < 0.9 else ("s", rng.choice(names), b"t"))
        return index_cases.emit([(d_, per.get(d_, [])) for d_ in dirs if d_ == b"/" or d_ in per],
                                bs=bs)

    new = one_index(max_files)
    sources = []
    for _ in range(rng.randint(0, nsrc_max)):
        r = rng.random()
        sources.append(new if r < 0.1 else one_index(max_files) if r < 0.9 else rng.randbytes(30))
    skip = None if rng.random() < 0.5 else [i for i in range(max_files) if rng.random() < 0.2]
    return new, sources, skip


__all__ = ["families", "random_case", "at", "BS"]
