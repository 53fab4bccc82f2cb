"""Python restatement of cir_block_repeats' / cir_match_repeats_dev's rule, for
their tests (no test module: helpers only).  Plain lists and a dict; nothing
here calls the library.

* Blocks g < n: the index's file-entry blocks in index order.  Block g is
  wanted when want is None or want[g]; present when it is not wanted and
  present[g]; otherwise it takes no part.
* Key: g when present, 2^31 + g when wanted.  The leader of a digest is the
  participating block with the smallest key among those with that digest.
* match[g] = NONE when g is not wanted or leads its digest, else L when the
  leader is present and n + L when it is wanted.
* The rest is extents_restate.expected_dev over the need run table twice (the
  second copy's `first` raised by n, x = 1; n_pool = 2n).
"""
import extents_restate
import sources_restate
from links_restate import file_entries

NONE = 0xFFFFFFFF
WANTED = 1 << 31


def key_of(g, want, present):
    if want is None or want[g]:
        return WANTED + g
    if present is not None and present[g]:
        return g
    return None


def expected_match(digests, want=None, present=None):
    """match[] of cir_match_repeats_dev for a list of 32-byte digests."""
    n = len(digests)
    leader = {}
    for g, d in enumerate(digests):
        k = key_of(g, want, present)
        if k is not None and k < leader.get(d, 1 << 40):
            leader[d] = k
    match = []
    for g, d in enumerate(digests):
        k = key_of(g, want, present)
        if k is None or k < WANTED or leader[d] == k:
            match.append(NONE)
        else:
            lead = leader[d]
            match.append(n + lead - WANTED if lead >= WANTED else lead)
    return match


def doubled(runs, n):
    """The pool run table of the rule: the need run table twice."""
    return [(f, s, fi, 0) for f, s, fi, _ in runs] + [(f + n, s, fi, 1) for f, s, fi, _ in runs]


def index_digests(index):
    return [d for _, _, _, ds in file_entries(index) for d in ds]


def expected(index, want=None, present=None):
    """What cir_block_repeats must give: (extents, fetch bits, stats)."""
    _, bs = sources_restate._header(index)
    digests = index_digests(index)
    n = len(digests)
    runs, count = extents_restate.runs_of_index(index)
    assert count == n
    match = expected_match(digests, want, present)
    dev = extents_restate.expected_dev(match, runs, doubled(runs, n), 2 * n, bs, want)
    keys = [key_of(g, want, present) for g in range(n)]
    wanted, found, nbytes, dropped, next = dev["res"]
    stats = dict(wanted=wanted, repeats=found, bytes_repeated=nbytes,
                 took_part=sum(1 for k in keys if k is not None),
                 present=sum(1 for k in keys if k is not None and k < WANTED),
                 dropped_length=dropped, extents=next, left_to_fetch=wanted - found)
    assert sum(dev["fetch"]) == wanted - found
    return dev["extents"], dev["fetch"], stats


def same(result, want):
    """Does a RepeatsResult carry exactly the restatement's answer?"""
    extents, fetch, stats = want
    return (result.nblk == len(fetch) and [tuple(e) for e in result.extents] == extents and
            result.fetch == sources_restate.want_words(fetch) and
            all(result.stats[k] == v for k, v in stats.items()))


def expected_copies(index, extents):
    """[(dst_path, dst_offset, length, class, src_path, src_offset)] per extent."""
    _, bs = sources_restate._header(index)
    paths = [e[0] for e in file_entries(index)]
    return [(paths[nf], nb * bs, nbytes, s, paths[sf], sb * bs)
            for _, _, nf, nb, s, sf, sb, nbytes in extents]
