"""The rule of cir_fetch_plan in plain Python (no test module: helpers only):
the composition of links_restate, copies_restate, extents_restate and
repeats_restate, block by block and file by file.  Nothing here calls the
library.

  1. L1 = the same-path candidates, minus the files in deny.
  2. L2 = the content candidates with skip = deny | files(L1).
  3. linked = files(L1) | files(L2); want1 = every block of a file entry that
     is not linked, minus the 1-bits of have.
  4. (E1, fetch1) = the extents with want = want1.
  5. (E2, fetch2) = the repeats with want = fetch1, present = not fetch1.

deny: an iterable of file ordinals (None: none); have: a 0/1 list over global
blocks, of any length (None: none; bits past the last block are ignored).
"""
import copies_restate
import extents_restate
import links_restate
import repeats_restate
import sources_restate


def expected(index, sources, deny=None, have=None):
    """dict(links, copies, extents, repeats, fetch (0/1 per block), nblk,
    skipped, stats) where stats holds the counts that do not depend on the
    path: the four calls' under "sources", "copies", "extents", "repeats", and
    the plan's own."""
    files = links_restate.file_entries(index)
    deny = {i for i in (deny or ()) if i < len(files)}
    l1_all, skipped = links_restate.expected_candidates(index, sources)
    l1 = [(f, s) for f, s in l1_all if f not in deny]
    skip = deny | {f for f, _ in l1}
    l2, _ = copies_restate.expected_copies(index, sources, skip)
    linked = {f for f, _ in l1} | {c[0] for c in l2}
    want1, linked_blocks, have_blocks = [], 0, 0
    for f, (_, _, _, digests) in enumerate(files):
        for _ in digests:
            g = len(want1)
            if f in linked:
                want1.append(0)
                linked_blocks += 1
            elif have is not None and g < len(have) and have[g]:
                want1.append(0)
                have_blocks += 1
            else:
                want1.append(1)
    e1, fetch1, st1, _ = extents_restate.expected(index, sources, want1)
    e2, fetch2, st2 = repeats_restate.expected(index, fetch1, [1 - b for b in fetch1])
    usable, _ = copies_restate.usable_sources(index, sources)
    stats = {
        "sources": {"files": len(files), "candidates": len(l1_all),
                    "bytes": sum(files[f][2] for f, _ in l1_all),
                    "pool_files": sum(len(e) for _, e in usable), "sources_used": len(usable)},
        "copies": dict(zip(("files", "candidates", "bytes", "pool_files", "sources_used",
                            "skipped_files", "same_path"),
                           (v for _, v in sorted(
                               copies_restate.expected_stats(index, sources, skip).items())))),
        "extents": st1,
        "repeats": st2,
        "withdrawn": len(l1_all) - len(l1),
        "linked": len(linked),
        "linked_blocks": linked_blocks,
        "have_blocks": have_blocks,
    }
    return dict(links=l1, copies=l2, extents=e1, repeats=e2, fetch=fetch2, nblk=len(want1),
                skipped=skipped, stats=stats)


def composed(ca, index, sources, deny=None, have=None, context=None):
    """The same composition through the package's four existing calls (`ca`:
    the ciruela_amd module), as a caller glues them today."""
    files = links_restate.file_entries(index)
    deny = {i for i in (deny or ()) if i < len(files)}
    l1_all, _ = ca.file_sources(index, sources, context)
    l1 = [(f, s) for f, s in l1_all if f not in deny]
    skip = deny | {f for f, _ in l1}
    l2, _ = ca.file_copies(index, sources, context, sorted(skip))
    linked = {f for f, _ in l1} | {c[0] for c in l2}
    want1 = []
    for f, (_, _, _, digests) in enumerate(files):
        for _ in digests:
            g = len(want1)
            want1.append(0 if f in linked or (have is not None and g < len(have) and have[g])
                         else 1)
    r1 = ca.block_extents(index, sources, want=bytes(sources_restate.want_words(want1)),
                          context=context)
    n = len(want1)
    fetch1 = [(r1.fetch[g >> 3] >> (g & 7)) & 1 for g in range(n)]
    r2 = ca.block_repeats(index, want=r1.fetch,
                          present=bytes(sources_restate.want_words([1 - b for b in fetch1])),
                          context=context)
    return dict(links=l1, copies=l2, extents=[tuple(e) for e in r1.extents],
                repeats=[tuple(e) for e in r2.extents], fetch=bytes(r2.fetch), nblk=n)


def same(result, want, on_device=None):
    """Does a PlanResult carry exactly the restatement's answer?  on_device:
    also require stats["on_device"] to be this."""
    st = result.stats
    ok = (result.links == want["links"] and result.copies == want["copies"] and
          [tuple(e) for e in result.extents] == want["extents"] and
          [tuple(e) for e in result.repeats] == want["repeats"] and
          result.nblk == want["nblk"] and
          result.fetch == bytes(sources_restate.want_words(want["fetch"])) and
          result.skipped == want["skipped"])
    for name, val in want["stats"].items():
        if isinstance(val, dict):
            ok = ok and all(st[name][k] == v for k, v in val.items())
        else:
            ok = ok and st[name] == val
    if on_device is not None:
        ok = ok and st["on_device"] == on_device
    return bool(ok)


def reach(want):
    """Which stages a case reaches: (L1, L2, E1, E2, fetch) as booleans."""
    return (bool(want["links"]), bool(want["copies"]), bool(want["extents"]),
            bool(want["repeats"]), any(want["fetch"]))
