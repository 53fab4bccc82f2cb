"""Input families of the cir_block_extents tests (no test module: helpers
only), shared by the CPU and the GPU file: the families of sources_cases and
the ones that are about extents.  Nothing here calls the library.

cases() -> [(name, index, [source index, ...], want bits or None, tail_ones)].
"""
import random

import sources_cases
from sources_cases import BS, _emit, _file


def _extent_families():
    rng = random.Random(20250307)
    d = [rng.randbytes(32) for _ in range(64)]
    short = rng.randbytes(32)
    out = []
    old = _emit([(b"/", [_file(b"a", 6 * BS, d[0:6]), _file(b"b", 4 * BS + 9, d[6:10] + [short])])])
    # a whole file shared: one extent per file, the short tail inside the second
    out.append(("whole_file_shared", old, [old], None, False))
    # one changed block in the middle: two extents and one fetch bit
    new = _emit([(b"/", [_file(b"a", 6 * BS, d[0:3] + [d[40]] + d[4:6])])])
    out.append(("one_changed_block", new, [old], None, False))
    # an appended file: the old blocks are one extent, the new ones are fetched
    new = _emit([(b"/", [_file(b"a", 8 * BS + 3, d[0:6] + [d[41], d[42], d[43]])])])
    out.append(("appended_file", new, [old], None, False))
    # a moved file: another path and another position among the files
    new = _emit([(b"/", [_file(b"0", BS, [d[44]])]),
                 (b"/moved", [_file(b"b2", 4 * BS + 9, d[6:10] + [short])])])
    out.append(("moved_file", new, [old], None, False))
    # two need files whose blocks sit back to back in one source file: they
    # must not merge (a need-file boundary breaks an extent)
    new = _emit([(b"/", [_file(b"p", 3 * BS, d[0:3]), _file(b"q", 3 * BS, d[3:6])])])
    out.append(("two_need_files_one_source_file", new, [old], None, False))
    # two source files back to back in the pool matched by one need file: they
    # must not merge although the pool ordinals are consecutive -- nor where
    # the second file sits in the next source
    two = _emit([(b"/", [_file(b"h", 2 * BS, d[20:22]), _file(b"t", 2 * BS, d[22:24])])])
    new = _emit([(b"/", [_file(b"ht", 4 * BS, d[20:24])])])
    out.append(("two_source_files_one_need_file", new, [two], None, False))
    s0 = _emit([(b"/", [_file(b"h", 2 * BS, d[20:22])])])
    s1 = _emit([(b"/", [_file(b"t", 2 * BS, d[22:24])])])
    out.append(("two_sources_one_need_file", new, [s0, s1], None, False))
    # a repeated block inside a need file: both match the same pool block
    new = _emit([(b"/", [_file(b"r", 5 * BS, [d[0], d[1], d[1], d[2], d[3]])])])
    out.append(("repeated_block", new, [old], None, False))
    # a short last block against a full source block: dropped, and it ends the
    # extent in front of it
    new = _emit([(b"/", [_file(b"s", 2 * BS + 5, [d[0], d[1], d[2]])])])
    out.append(("short_last_block_dropped", new, [old], None, False))
    # `want` clearing a block in the middle of an extent
    out.append(("want_clears_the_middle", old, [old], [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1], True))
    # a skipped source between two used ones
    other_bs = _emit([(b"/", [_file(b"a", 32, [d[0]])])], bs=32)
    new = _emit([(b"/", [_file(b"ht", 4 * BS, d[20:24])])])
    out.append(("skipped_source_between", new, [s0, other_bs, s1], None, False))
    # source blocks in reverse order: every block its own extent
    rev = _emit([(b"/", [_file(b"v", 6 * BS, d[5::-1])])])
    out.append(("reverse_order", old, [rev], None, False))
    # no blocks at all
    empty = _emit([(b"/", [_file(b"e", 0, [])]), (b"/d", [])])
    out.append(("extents_no_blocks", empty, [old], None, False))
    return out


def cases():
    return sources_cases.cases() + _extent_families()
