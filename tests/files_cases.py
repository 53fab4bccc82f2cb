"""Input families of the cir_file_sources tests (no test module: helpers only),
shared by the CPU and the GPU file.  Indexes are dirsig_oracle.emit's over
random digests (index_cases / sources_cases builders), so no file is hashed;
expected values are links_restate.expected_candidates' and a search of the
text.  Nothing here calls the library.

families() -> [(name, index, [source index, ...])], every text canonical
unless the name says otherwise (skipped sources are garbage on purpose).
"""
import random

import numpy as np

import dirsig_oracle
import index_cases
import links_restate
import sources_cases
from test_check_links_cpu import A, B, C, NEW_DIRS, digests, emit, entry

BS = 64
EXE = 1 << 63


def f(rng, name, nblk, exe=False, bs=BS, short=0):
    """A file entry of nblk blocks over random digests (short: bytes missing
    from the last block)."""
    return index_cases.file_entry(rng, name, nblk * bs - (short if nblk else 0), bs, exe=exe)


def expected_records(index, off_bias=0, block_bias=0):
    """(n, 4) u64 {name_off, dir_off, size, first | exe << 63} of a canonical
    index, by a walk over its lines."""
    recs, pos, dir_off, blk = [], index.index(b"\n") + 1, None, 0
    lines = index.split(b"\n")
    for ln in lines[1:-2]:
        if ln.startswith(b"/"):
            dir_off = pos
        else:
            parts = ln[2:].split(b" ")
            if parts[1] in (b"f", b"x"):
                recs.append((pos + 2 + off_bias, dir_off + off_bias, int(parts[2]),
                             (blk + block_bias) | (EXE if parts[1] == b"x" else 0)))
                blk += len(parts) - 3
        pos += len(ln) + 1
    return np.array(recs, dtype=np.uint64).reshape(-1, 4)


def respell(index, old, new):
    """The same index with one spelling of a name or a directory replaced (the
    footer is not checked by any parser here)."""
    assert old in index
    return index.replace(old, new)


def families():
    rng = random.Random(20260301)
    out = []
    new = emit(NEW_DIRS)
    old1 = emit([(b"/", [entry(b"one", A)]), (b"/d", [entry(b"two", C)])])
    old2 = emit(NEW_DIRS)
    out += [("order_12", new, [old1, old2]), ("order_21", new, [old2, old1]),
            ("one_source", new, [old1]), ("itself", new, [new])]
    # exe flag, size and digest mismatches; the good source behind the bad one
    exe_flip = emit([(b"/", [entry(b"one", A, exe=True), entry(b"run", B, exe=False)])])
    size = emit([(b"/", [entry(b"one", A + b"a")]), (b"/d", [entry(b"two", C[:-1])])])
    d = digests(C)
    d[1] = d[1][:5] + bytes([d[1][5] ^ 1]) + d[1][6:]
    one_byte = emit([(b"/", [entry(b"one", A)]), (b"/d", [("f", b"two", False, len(C), d)])])
    out += [("exe_flip", new, [exe_flip]), ("size_differs", new, [size]),
            ("one_digest_byte", new, [one_byte]), ("bad_then_good", new, [one_byte, old2])]
    # a symlink or a directory at the path; a file at a symlink's path
    old = emit([(b"/", [("s", b"one", b"elsewhere"), entry(b"run", B, exe=True)]),
                (b"/d", []), (b"/d/two", [entry(b"inner", C)])])
    out += [("symlink_or_dir_at_path", new, [old]),
            ("file_at_symlink", new, [emit([(b"/", [entry(b"lnk", A)])])])]
    # skipped sources: garbage, a cut text, an empty one, another block size or hash type
    cut = old2[:len(old2) // 2]
    other_bs = emit([(b"/", [entry(b"one", A, bs=128), entry(b"zero", b"", bs=128)])], bs=128)
    other_hash = emit([(b"/", [entry(b"one", A, hname="sha512/256")])], hname="sha512/256")
    out += [("skipped_framing", new, [random.Random(3).randbytes(300), old2, b""]),
            ("skipped_headers", new, [other_bs, other_hash, old2]),
            ("only_skipped", new, [other_bs, b"garbage\n"])]
    sha_dirs = [(b"/", [entry(b"one", A, hname="sha512/256")])]
    out.append(("sha512_256", emit(sha_dirs, hname="sha512/256"),
                [old2, emit(sha_dirs, hname="sha512/256")]))
    out += [("no_sources", new, []), ("no_files", emit([(b"/", [("s", b"l", b"t")])]), [new])]
    esc = [(b"/", [entry(b"back\\slash", A), entry(b"with space", B)]),
           (b"/sp ace", [entry(b"\xff\x01", C)])]
    out.append(("escaped_names", emit(esc), [emit(esc[:1]), emit(esc)]))
    # duplicate paths inside a source: the first entry wins, even when the
    # second would match
    good, bad = f(rng, b"dup", 3), f(rng, b"dup", 3)
    need = emit([(b"/", [good])])
    out += [("dup_first_wins_miss", need, [emit([(b"/", [bad, good])])]),
            ("dup_first_wins_hit", need, [emit([(b"/", [good, bad])])]),
            ("dup_then_next_source", need, [emit([(b"/", [bad, good])]), emit([(b"/", [good])])])]
    # escaped and unescaped spellings of one name and of one directory
    e1, e2 = f(rng, b"Alpha", 2), f(rng, b"beta", 1)
    plain = emit([(b"/", [e1]), (b"/dir", [e2])])
    spelled = respell(respell(plain, b"  Alpha ", b"  \\x41lph\\x61 "), b"/dir\n", b"/d\\x69r\n")
    out += [("spelling_need_escaped", spelled, [plain]), ("spelling_pool_escaped", plain, [spelled]),
            ("spelling_both", spelled, [spelled])]
    # size-0 files: first, between and last; against a non-empty file of the same name
    z = [f(rng, b"z0", 0), f(rng, b"m", 2), f(rng, b"z1", 0, exe=True), f(rng, b"n", 1, short=5),
         f(rng, b"z2", 0)]
    zi = emit([(b"/", z)])
    out += [("size0_same", zi, [zi]),
            ("size0_vs_nonempty", zi, [emit([(b"/", [f(rng, b"z0", 1), z[1], f(rng, b"z1", 0)])])]),
            ("only_size0", emit([(b"/", [z[0], z[4]])]), [zi])]
    # same path with other digests in source 0 and equal digests in source 1
    p = f(rng, b"same", 4)
    q = ("f", b"same", False, p[3], [rng.randbytes(32) for _ in p[4]])
    out.append(("other_digests_then_equal", emit([(b"/x", [p])]),
                [emit([(b"/x", [q])]), emit([(b"/x", [p])])]))
    # two digests of one file swapped in the source
    sw = ("f", b"same", False, p[3], [p[4][1], p[4][0]] + p[4][2:])
    out.append(("swapped_digests", emit([(b"/x", [p])]), [emit([(b"/x", [sw])])]))
    # the same name in two directories, and a directory named like a file's path
    out.append(("same_name_two_dirs", emit([(b"/a", [p]), (b"/b", [p])]),
                [emit([(b"/b", [p])]), emit([(b"/", [p]), (b"/a", [q])])]))
    return out


def random_case(seed, max_files=12, nsrc_max=5):
    """A seeded random family over a small universe of paths and digest lists,
    so that equal paths with equal and with other content, duplicates, empty
    files and exe flips abound.  Returns (index, sources)."""
    rng = random.Random(seed)
    bs = rng.choice((1, 7, BS))
    dirs = [b"/", b"/d", b"/d/e", b"/sp ace"]
    names = [b"a", b"b", b"A", b"c d", b"\xffq", b"long-name-%d" % rng.randrange(3)]
    contents = [[rng.randbytes(32) for _ in range(rng.choice((0, 1, 1, 2, 5, 70)))]
                for _ in range(6)]

    def one_index(nfiles):
        per = {}
        for _ in range(rng.randint(0, nfiles)):
            digests_ = list(rng.choice(contents))
            n = len(digests_)
            size = 0 if n == 0 else (n - 1) * bs + (bs if rng.random() < 0.7 else rng.randint(1, bs))
            if n and rng.random() < 0.1:
                digests_[rng.randrange(n)] = rng.randbytes(32)
            per.setdefault(rng.choice(dirs), []).append(
                ("f", rng.choice(names), rng.random() < 0.2, size, digests_)
                if rng.random() < 0.9 else ("s", rng.choice(names), b"t"))
        return dirsig_oracle.emit("blake2b/256", bs, [(d_, per.get(d_, [])) for d_ in dirs
                                                      if d_ == b"/" or d_ in per], keep_empty=True)

    new = one_index(max_files)
    sources = []
    for _ in range(rng.randint(0, nsrc_max)):
        r = rng.random()
        sources.append(new if r < 0.15 else one_index(max_files) if r < 0.9 else rng.randbytes(30))
    return new, sources


def expected(index, sources):
    return links_restate.expected_candidates(index, sources)


__all__ = ["families", "random_case", "expected", "expected_records", "f", "BS", "sources_cases"]
