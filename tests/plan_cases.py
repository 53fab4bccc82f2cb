"""Input families of the cir_fetch_plan tests (no test module: helpers only),
shared by the CPU and the GPU file.  Indexes are index_cases.emit's over random
digests (files_cases.f), so every text is in the device's canonical subset
unless the family says otherwise; expected values are plan_restate's.  Nothing
here calls the library.

families() -> [(name, index, [source index, ...], deny or None, have or None)]
deny: a list of file ordinals; have: a 0/1 list over global blocks.
"""
import random

import copies_cases
import files_cases
import index_cases

BS = files_cases.BS
f = files_cases.f
emit = index_cases.emit
at = copies_cases.at

# What the hand-made family must give (tests assert these before anything else).
HAND_MADE = dict(nblk=93, links=2, copies=1, extents=4, repeats=1, repeat_blocks=5, repeat_src=1,
                 fetch=9)
HAND_MADE_DENY0 = dict(links=1, extents=5)


def hand_made():
    """An old image and its new version, BS 64, 93 blocks in the new one: one
    unchanged file (3 blocks), one empty file, one file under a renamed
    directory (5), a 70-block file with block 35 changed, a log with two blocks
    appended (3 blocks, the last one short, become 5), a new 5-block file held
    twice.  The 70-block file's last block repeats its first (the same page at
    both ends), so its unchanged blocks come as three extents: [0, 35), [36, 69)
    and block 69, which the old image holds first at block 0.  With the log's
    two whole blocks that is 4 extents; the changed block, the log's rewritten
    third block with the two appended ones and the new file's first copy are 9
    blocks to fetch; the new file's second copy is one repeat of 5 blocks from
    a fetched source."""
    rng = random.Random(20261021)
    same, empty = f(rng, b"same", 3), f(rng, b"empty", 0)
    moved = f(rng, b"tool", 5, exe=True)
    big = f(rng, b"big", 70)
    big = ("f", b"big", False, big[3], big[4][:69] + [big[4][0]])
    big2 = ("f", b"big", False, big[3], big[4][:35] + [rng.randbytes(32)] + big[4][36:])
    log = f(rng, b"log", 3, short=20)
    log2 = ("f", b"log", False, log[3] + 2 * BS,
            log[4][:2] + [rng.randbytes(32) for _ in range(3)])
    fresh = f(rng, b"fresh", 5)
    old = emit([(b"/", [same, empty]), (b"/app-1", [moved]), (b"/data", [big, log])])
    new = emit([(b"/", [same, empty]), (b"/app-2", [moved]), (b"/data", [big2, log2]),
                (b"/new", [fresh, at(fresh, b"fresh-again")])])
    return new, [old]


def families():
    rng = random.Random(20261022)
    out = []
    new, olds = hand_made()
    out.append(("hand_made", new, olds, None, None))
    out.append(("hand_made_deny0", new, olds, [0], None))
    # a have block whose digest no source holds, and a wanted block equal to it:
    # the only way to a repeat extent with src = 0
    a, b = f(rng, b"a", 4), f(rng, b"b", 3)
    twin = ("f", b"twin", False, 2 * BS, [a[4][1], rng.randbytes(32)])
    new = emit([(b"/", [a, b, twin])])
    old = emit([(b"/", [at(b, b"b-was", exe=True)])])       # (same digests, no link: exe differs)
    have = [0] * 9
    have[1] = 1
    out.append(("have_and_its_twin", new, [old], None, have))
    # a denied file that has a content candidate elsewhere: no link of either kind
    x, y = f(rng, b"x", 4), f(rng, b"y", 2)
    out.append(("denied_with_content_candidate", emit([(b"/", [x, y])]),
                [emit([(b"/", [x]), (b"/other", [at(x, b"x-copy"), y])])], [0], None))
    # every file linked, and nothing linked
    p, q = f(rng, b"p", 3), f(rng, b"q", 70)
    whole = emit([(b"/", [p]), (b"/d", [q])])
    out.append(("all_linked", whole, [whole], None, None))
    out.append(("all_linked_moved", emit([(b"/", [at(p, b"p2")]), (b"/e", [q])]), [whole], None,
                None))
    out.append(("nothing_linked", emit([(b"/", [f(rng, b"p", 3)]), (b"/d", [f(rng, b"q", 6)])]),
                [whole], None, None))
    out.append(("all_denied", whole, [whole], [0, 1], None))
    # deny bits at 0, 63, 64 and 65 of 70 files that all have a same-path candidate
    many = [f(rng, b"n%02d" % i, 1 + i % 3) for i in range(70)]
    many_index = emit([(b"/v", many)])
    out.append(("deny_bits", many_index, [many_index], [0, 63, 64, 65], None))
    out.append(("deny_bits_moved", emit([(b"/w", many)]), [many_index], [0, 63, 64, 65], None))
    # all have, with bits past the last block; have over linked files changes nothing
    out.append(("have_everything", emit([(b"/", [f(rng, b"p", 3)]), (b"/d", [q])]), [whole], None,
                [1] * 200))
    # garbage and foreign-block-size sources among good ones
    other_bs = index_cases.emit([(b"/", [f(rng, b"x", 2, bs=128)])], bs=128)
    new, olds = hand_made()
    out.append(("skipped_sources", new,
                [random.Random(3).randbytes(300), other_bs, olds[0], b"", whole], [1], None))
    out.append(("no_sources", new, [], None, None))
    out.append(("no_blocks", emit([(b"/", [f(rng, b"e", 0), ("s", b"l", b"t")])]), olds, None,
                None))
    out.append(("no_files", emit([(b"/", [("s", b"l", b"t")])]), olds, None, None))
    return out


def random_case(seed):
    """copies_cases.random_case with its skip taken as deny, and a random have
    bitmap in two cases of three, bits past the last block included.  Returns
    (index, sources, deny, have)."""
    index, sources, skip = copies_cases.random_case(seed)
    rng = random.Random(1000003 * seed + 7)
    have = None
    if rng.random() < 2 / 3:
        p = rng.choice((0.1, 0.5, 0.9))
        have = [int(rng.random() < p) for _ in range(rng.choice((64, 200, 600)))]
    return index, sources, skip, have


__all__ = ["families", "random_case", "hand_made", "HAND_MADE", "HAND_MADE_DENY0", "BS"]
