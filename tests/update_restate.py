"""Python restatement of cir_update_blocks' rule (no test module: helpers
only).  Nothing here calls the library.

The classes, by address.  The resident buffers and the destinations are spans
of one allocation, given as offsets into a snapshot of it taken before the
call.  Each resident buffer is cut into blocks of the index's block size from
its own offset 0 and every such block is digested by the caller's `digest`
function (the tests pass the C oracle's).  Block g of the new index, of `len`
bytes at dst, is

  kept     when a resident block of len bytes and g's digest begins exactly at
           dst;
  direct   otherwise, when some resident block has g's digest and length and
           [dst, dst + len) meets no resident buffer;
  staged   otherwise, when some resident block has them -- as long as the units
           (16 bytes, rounded up per block) of all such blocks up to and
           including this one, in block order, fit the cap;
  demoted  when they do not fit;
  None     when no resident block has them, or the file has no destination.

kept, direct and staged blocks are memory's share; what is not is judged by
tests/blocks_restate.py's walk of the image directory, combined as in
tests/reload_restate.py: a non-empty file all of whose blocks memory gives is
never looked at and is complete and resident whatever the directory holds.
"""
import os

import blocks_restate
import dirsig_oracle
import reload_restate
from blocks_restate import ABSENT, BLOCKED, COMPLETE, PARTIAL
from links_restate import file_entries
from reload_restate import SKIPPED, units

KEPT, DIRECT, STAGED, DEMOTED = "kept", "direct", "staged", "demoted"


def classes(index, snapshot, res_spans, dest_offs, digest, cap_units=None):
    """One class per global block.  res_spans: [(offset, size)] of the resident
    buffers; dest_offs: one offset per file entry, None: no destination;
    cap_units None: no cap."""
    _, bs, _, _ = dirsig_oracle.parse(index)
    at_addr, anywhere = {}, set()
    for off, size in res_spans:
        for at in range(0, size, bs):
            blk = bytes(snapshot[off + at:off + min(at + bs, size)])
            key = (digest(blk), len(blk))
            at_addr[off + at] = key
            anywhere.add(key)
    out, prefix = [], 0
    for (_, _, size, digests), doff in zip(file_entries(index), dest_offs):
        for j, dg in enumerate(digests):
            n = min(bs, size - j * bs)
            if doff is None:
                out.append(None)
                continue
            dst = doff + j * bs
            if at_addr.get(dst) == (dg, n):
                out.append(KEPT)
            elif (dg, n) not in anywhere:
                out.append(None)
            elif not any(dst < o + s and o < dst + n for o, s in res_spans):
                out.append(DIRECT)
            else:
                prefix += units(n)
                out.append(STAGED if cap_units is None or prefix <= cap_units else DEMOTED)
    return out


def expected(index, root, snapshot, res_spans, dest_offs, digest, scratch_bytes=None):
    """reload_restate.Expected with cls (one class per global block) and the
    counts kept, kept_bytes, staged, scratch_bytes, demoted besides copied
    (direct and staged), copied_bytes and disk_bytes."""
    _, bs, _, _ = dirsig_oracle.parse(index)
    cap = None if scratch_bytes is None else scratch_bytes // 16
    cls = classes(index, snapshot, res_spans, dest_offs, digest, cap)
    d_bits, d_states, d_longs, d_errnos = blocks_restate.expected(index, root)
    e = reload_restate.Expected()
    e.cls = cls
    e.bits, e.mem, e.states, e.longs, e.resident, e.errnos = [], [], [], [], [], []
    e.copied = e.copied_bytes = e.disk_bytes = 0
    e.kept = e.kept_bytes = e.staged = e.scratch_bytes = e.demoted = 0
    g = 0
    for i, (path, _, size, digests) in enumerate(file_entries(index)):
        n = len(digests)
        lens = [min(bs, size - j * bs) for j in range(n)]
        if size and dest_offs[i] is None:
            e.bits += [0] * n
            e.mem += [0] * n
            e.states.append(SKIPPED)
            e.longs.append(False)
            e.resident.append(False)
            e.errnos.append(0)
            g += n
            continue
        mine = cls[g:g + n]
        mem = [1 if c in (KEPT, DIRECT, STAGED) else 0 for c in mine]
        e.mem += mem
        for c, l in zip(mine, lens):
            if c == KEPT:
                e.kept += 1
                e.kept_bytes += l
            elif c in (DIRECT, STAGED):
                e.copied += 1
                e.copied_bytes += l
                if c == STAGED:
                    e.staged += 1
                    e.scratch_bytes += 16 * units(l)
            elif c == DEMOTED:
                e.demoted += 1
        if n and all(mem):                      # never looked at
            e.bits += mem
            e.states.append(COMPLETE)
            e.longs.append(False)
            e.resident.append(True)
            e.errnos.append(0)
            g += n
            continue
        disk = d_bits[g:g + n]
        st, lg, err = d_states[i], d_longs[i], d_errnos[i]
        e.resident.append(False)
        if st in (ABSENT, BLOCKED):
            e.bits += mem                       # what memory gave stays
            e.states.append(st)
            e.longs.append(False)
            e.errnos.append(err)
        else:
            bits = [m | d for m, d in zip(mem, disk)]
            e.bits += bits
            whole = size == 0 or os.lstat(reload_restate._real(root, path)).st_size == size
            e.states.append(st if size == 0 else COMPLETE if all(bits) and whole else PARTIAL)
            e.longs.append(lg)
            e.errnos.append(0)
            nread = reload_restate._readable_blocks(root, path, size, bs)
            e.disk_bytes += sum(lens[j] for j in range(min(n, nread)) if not mem[j])
        g += n
    return e


def same(result, e):
    return reload_restate.same(result, e)


def check_stats(result, e):
    """The result's counts against the restatement's."""
    st = result.stats
    assert (st["have"], st["missing"]) == (sum(e.bits), len(e.bits) - sum(e.bits))
    assert (st["copied_blocks"], st["copied_bytes"]) == (e.copied, e.copied_bytes)
    assert (st["kept_blocks"], st["kept_bytes"]) == (e.kept, e.kept_bytes)
    assert (st["staged_blocks"], st["scratch_bytes"], st["demoted_blocks"]) == \
        (e.staged, e.scratch_bytes, e.demoted)
    assert st["bytes"] == st["scattered_bytes"] == e.disk_bytes
    assert st["resident_files"] == sum(e.resident)
    assert st["skipped"] == e.states.count(SKIPPED)
    # (a match dropped for its length needs a hash collision; tools/update_fuzz.cpp runs
    # that branch on the host)
    assert st["dropped_length"] == 0
    assert st[COMPLETE] == e.states.count(COMPLETE)
