"""The rule of cir_file_copies / cir_match_copies_dev in plain Python (no test
module: helpers only), written from the rule's statement and not from the C++.

Pool files are ordered by source in the order given, then in index order.  A
need file takes part only if its size is greater than 0 and it is not skipped;
its candidate is the pool file with the smallest pool ordinal that has equal
exe flag, equal size and an equal digest list, at any path.  Empty files take
part on neither side.  Sources are skipped as in links_restate (a text that
does not parse, another hash type or block size).  Nothing here calls the
library.
"""
import links_restate


def usable_sources(index, sources):
    """([(source ordinal, file entries)], sources skipped)."""
    head = links_restate._header(index)
    usable, skipped = [], 0
    for j, s in enumerate(sources):
        try:
            if links_restate._header(s) != head:
                raise ValueError("another hash type or block size")
            entries = links_restate.file_entries(s)
        except Exception:
            skipped += 1
            continue
        usable.append((j, entries))
    return usable, skipped


def expected_copies(index, sources, skip=None):
    """([(file ordinal, source ordinal, file ordinal inside the source, source
    path)], sources skipped)."""
    skip = set(skip or ())
    usable, skipped = usable_sources(index, sources)
    first = {}
    for j, entries in usable:               # pool order: by source, then index order
        for k, (path, exe, size, digests) in enumerate(entries):
            if size > 0:
                first.setdefault((exe, size, tuple(digests)), (j, k, path))
    out = []
    for f, (path, exe, size, digests) in enumerate(links_restate.file_entries(index)):
        if size == 0 or f in skip:
            continue
        hit = first.get((exe, size, tuple(digests)))
        if hit is not None:
            out.append((f,) + hit)
    return out, skipped


def expected_stats(index, sources, skip=None):
    """stats[0..4], [8] and [9] of cir_file_copies."""
    want, _ = expected_copies(index, sources, skip)
    files = links_restate.file_entries(index)
    usable, _ = usable_sources(index, sources)
    left_out = len({i for i in (skip or ()) if i < len(files)})
    return {0: len(files), 1: len(want), 2: sum(files[f][2] for f, _, _, _ in want),
            3: sum(len(e) for _, e in usable), 4: len(usable), 8: left_out,
            9: sum(files[f][0] == path for f, _, _, path in want)}


def equal_pool_files(index, sources):
    """Per need file: how many pool files have its content (0 for an empty one)."""
    usable, _ = usable_sources(index, sources)
    count = {}
    for _, entries in usable:
        for _, exe, size, digests in entries:
            if size > 0:
                key = (exe, size, tuple(digests))
                count[key] = count.get(key, 0) + 1
    return [count.get((exe, size, tuple(d)), 0) if size else 0
            for _, exe, size, d in links_restate.file_entries(index)]


def expected_from_records(need, need_dig, pool, pool_dig, src_first, bs, skip=()):
    """The same rule over record arrays ((n, 4) u64 {name_off, dir_off, size,
    first | exe << 63}) and flat digests ((nblk, 32) u8): per need file
    (source, file inside the source, name_off, dir_off) or None."""
    def key(rec, dig):
        size, first = int(rec[2]), int(rec[3])
        n = (size + bs - 1) // bs
        b0 = first & ~(1 << 63)
        return (first >> 63, size, dig[b0:b0 + n].tobytes())
    skip = set(skip)
    table = {}
    for j, rec in enumerate(pool):
        if int(rec[2]) > 0:
            table.setdefault(key(rec, pool_dig), j)
    out = []
    for i, rec in enumerate(need):
        j = None if int(rec[2]) == 0 or i in skip else table.get(key(rec, need_dig))
        if j is None:
            out.append(None)
            continue
        s = max(k for k in range(len(src_first) - 1) if src_first[k] <= j)
        out.append((s, j - src_first[s], int(pool[j][0]), int(pool[j][1])))
    return out
