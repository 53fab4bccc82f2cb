"""Python restatement of cir_block_extents' / cir_match_extents_dev's rule, for
their tests (no test module: helpers only).  Plain lists; nothing here calls
the library.

* Tables: a need run table and a pool run table, lists of (first, size, file,
  x), `first` ascending; x is the source ordinal in the pool's and ignored in
  the need's.  match[g]: a pool ordinal, or anything >= n_pool for "none".
* Per block g: its need run is the last one with first <= g; none, or g -
  first >= ceil(size / bs): the block lies in no file, is not wanted and not
  found.  Otherwise it is wanted iff want[g] (or want is None).  A wanted block
  with match[g] = j < n_pool whose pool run covers j is found iff the two
  blocks' lengths min(bs, size - b bs) are equal; unequal lengths count as
  dropped.
* cont(g): g - 1 and g both found, in the same need run, the same src and
  src_file, src_block(g) == src_block(g - 1) + 1.  An extent is a maximal
  stretch joined by cont: (first, count, need_file, need_block, src, src_file,
  src_block, bytes), bytes = min(size, (need_block + count) bs) - need_block bs.
* Fetch bit g: wanted and not found.
"""
import bisect

import sources_restate
from links_restate import file_entries

NO_SRC = 0xFFFFFFFF
NONE64 = (1 << 64) - 1


def _run_of(firsts, j):
    """Index of the last run with first <= j, or None."""
    i = bisect.bisect_right(firsts, j) - 1
    return i if i >= 0 else None


def _nblocks(size, bs):
    return (size + bs - 1) // bs


def _blen(size, bs, b):
    return min(bs, size - b * bs)


def map_blocks(match, need_runs, pool_runs, n_pool, bs, want=None):
    """Per block g: None when it lies in no file, else a dict {run, wanted,
    found, dropped, need_file, need_block, size, src, file, block, len}."""
    nf = [r[0] for r in need_runs]
    pf = [r[0] for r in pool_runs]
    out = []
    for g, j in enumerate(match):
        r = _run_of(nf, g)
        if r is None or g - need_runs[r][0] >= _nblocks(need_runs[r][1], bs):
            out.append(None)
            continue
        first, size, nfile, _ = need_runs[r]
        b = g - first
        m = dict(run=r, wanted=want is None or bool(want[g]), found=False, dropped=False,
                 need_file=nfile, need_block=b, size=size, src=None, file=None, block=None,
                 len=_blen(size, bs, b))
        out.append(m)
        if not m["wanted"] or j >= n_pool:
            continue
        p = _run_of(pf, j)
        if p is None:
            continue
        pfirst, psize, pfile, psrc = pool_runs[p]
        pb = j - pfirst
        if pb >= _nblocks(psize, bs):
            continue
        if _blen(psize, bs, pb) != m["len"]:
            m["dropped"] = True
            continue
        m.update(found=True, src=psrc & 0xFFFFFFFF, file=pfile, block=pb)
    return out


def _cont(a, b):
    return (a is not None and b is not None and a["found"] and b["found"] and
            a["run"] == b["run"] and a["src"] == b["src"] and a["file"] == b["file"] and
            b["block"] == a["block"] + 1)


def expected_dev(match, need_runs, pool_runs, n_pool, bs, want=None):
    """What cir_match_extents_dev must give: dict(src, file, block: per-block
    lists with the library's "none" marks; fetch: 0/1 per block; extents: list
    of 8-tuples; res: [wanted, found, bytes, dropped, extents])."""
    maps = map_blocks(match, need_runs, pool_runs, n_pool, bs, want)
    n = len(match)
    src = [m["src"] if m and m["found"] else NO_SRC for m in maps]
    file = [m["file"] if m and m["found"] else NONE64 for m in maps]
    block = [m["block"] if m and m["found"] else NONE64 for m in maps]
    fetch = [1 if m and m["wanted"] and not m["found"] else 0 for m in maps]
    extents = []
    g = 0
    while g < n:
        m = maps[g]
        if not (m and m["found"]):
            g += 1
            continue
        h = g
        while h + 1 < n and _cont(maps[h], maps[h + 1]):
            h += 1
        count = h - g + 1
        nbytes = min(m["size"], (m["need_block"] + count) * bs) - m["need_block"] * bs
        extents.append((g, count, m["need_file"], m["need_block"], m["src"], m["file"],
                        m["block"], nbytes))
        g = h + 1
    res = [sum(1 for m in maps if m and m["wanted"]), sum(1 for m in maps if m and m["found"]),
           sum(m["len"] for m in maps if m and m["found"]),
           sum(1 for m in maps if m and m["dropped"]), len(extents)]
    return dict(src=src, file=file, block=block, fetch=fetch, extents=extents, res=res)


def runs_of_index(index, first0=0, src=0):
    """The run table of one index (first0: the ordinal of its block 0) and its
    block count."""
    runs, at = [], first0
    for f, (_, _, size, digests) in enumerate(file_entries(index)):
        if digests:
            runs.append((at, size, f, src))
            at += len(digests)
    return runs, at - first0


def expected(index, sources, want=None):
    """What cir_block_extents must give, over sources_restate.expected:
    (extents, fetch bits, stats, skipped).  The extents are built from the
    per-block answer, block by block, not from run tables."""
    src, file, block, stats, skipped = sources_restate.expected(index, sources, want)
    _, bs = sources_restate._header(index)
    extents, fetch = [], [0] * len(src)
    g = 0
    for nfile, (_, _, size, digests) in enumerate(file_entries(index)):
        b = 0
        while b < len(digests):
            if src[g + b] is None:
                fetch[g + b] = 1 if want is None or want[g + b] else 0
                b += 1
                continue
            e = b
            while (e + 1 < len(digests) and src[g + e + 1] == src[g + b] and
                   file[g + e + 1] == file[g + b] and block[g + e + 1] == block[g + e] + 1):
                e += 1
            count = e - b + 1
            extents.append((g + b, count, nfile, b, src[g + b], file[g + b], block[g + b],
                            min(size, (b + count) * bs) - b * bs))
            b = e + 1
        g += len(digests)
    stats = dict(stats, extents=len(extents), left_to_fetch=sum(fetch))
    return extents, fetch, stats, skipped


def same(result, want):
    """Does an ExtentsResult carry exactly the restatement's answer?"""
    extents, fetch, stats, skipped = want
    return (result.nblk == len(fetch) and [tuple(e) for e in result.extents] == extents and
            result.fetch == sources_restate.want_words(fetch) and result.skipped == skipped and
            all(result.stats[k] == v for k, v in stats.items()))


def expected_copies(index, sources, extents):
    """[(dst_path, dst_offset, length, src, src_path, src_offset)] per extent."""
    _, bs = sources_restate._header(index)
    paths = [e[0] for e in file_entries(index)]
    spaths = {}
    out = []
    for _, _, nfile, nblock, s, sfile, sblock, nbytes in extents:
        if s not in spaths:
            spaths[s] = [e[0] for e in file_entries(sources[s])]
        out.append((paths[nfile], nblock * bs, nbytes, s, spaths[s][sfile], sblock * bs))
    return out
