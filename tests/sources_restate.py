"""Python restatement of cir_block_sources' rule, for its tests (no test
module: helpers only).  A dict over dirsig_oracle.parse; nothing here calls
the library.

* Need list: the new index's file entries in index order, blocks ascending
  (the global block numbering of cir_check_blocks).
* Pool: the sources in the order given; one that does not parse or whose
  hash type or block size is not the new index's takes no part and is
  counted.  Within a source the file entries in index order, blocks ascending.
* Block g matches the first place in that order whose digest equals its own
  (the flavour of scan_links' break, src/daemon/metadata/hardlink_sources.rs:
  143); if the two blocks' lengths, min(bs, size - block bs), differ, the
  block is not found, is counted, and no later copy is taken.
"""
import dirsig_oracle
from links_restate import file_entries

NONE = None


def _header(index):
    hash_name, bs, _, _ = dirsig_oracle.parse(index)
    return hash_name, bs


def _block_len(size, bs, b):
    return min(bs, size - b * bs)


def need_blocks(index):
    """[(path, size, block number, digest)] per global block."""
    out = []
    for path, _, size, digests in file_entries(index):
        for b, d in enumerate(digests):
            out.append((path, size, b, d))
    return out


def expected(index, sources, want=None):
    """(src, file, block, stats, skipped): three lists with one entry per
    global block (None where nothing was found or the block is not wanted),
    stats = {wanted, found, bytes_local, pool_blocks, sources_used,
    dropped_length}.  want: a list of 0/1 per block, or None for all."""
    head = _header(index)
    bs = head[1]
    first = {}          # digest -> (source ordinal, file ordinal, block, size): first place wins
    pool_blocks = used = skipped = 0
    for s, raw in enumerate(sources):
        try:
            if _header(raw) != head:
                raise ValueError("another hash type or block size")
            files = file_entries(raw)
            for _, _, size, digests in files:
                if len(digests) != (size + bs - 1) // bs or any(len(d) != 32 for d in digests):
                    raise ValueError("wrong number of hashes")
        except Exception:
            skipped += 1
            continue
        used += 1
        for f, (_, _, size, digests) in enumerate(files):
            for b, d in enumerate(digests):
                first.setdefault(d, (s, f, b, size))
                pool_blocks += 1
    need = need_blocks(index)
    src, file, block = [NONE] * len(need), [NONE] * len(need), [NONE] * len(need)
    wanted = found = nbytes = dropped = 0
    for g, (_, size, b, d) in enumerate(need):
        if want is not None and not want[g]:
            continue
        wanted += 1
        hit = first.get(d)
        if hit is None:
            continue
        s, f, pb, psize = hit
        if _block_len(psize, bs, pb) != _block_len(size, bs, b):
            dropped += 1
            continue
        src[g], file[g], block[g] = s, f, pb
        found += 1
        nbytes += _block_len(size, bs, b)
    stats = dict(wanted=wanted, found=found, bytes_local=nbytes, pool_blocks=pool_blocks,
                 sources_used=used, dropped_length=dropped)
    return src, file, block, stats, skipped


def expected_copies(index, sources, src, file, block):
    """[(dst_path, dst_offset, length, src, src_path, src_offset)] of the found
    blocks in index order, paths as raw bytes."""
    _, bs = _header(index)
    out = []
    spaths = {}
    for g, (path, size, b, _) in enumerate(need_blocks(index)):
        if src[g] is None:
            continue
        s = src[g]
        if s not in spaths:
            spaths[s] = [e[0] for e in file_entries(sources[s])]
        out.append((path, b * bs, _block_len(size, bs, b), s, spaths[s][file[g]], block[g] * bs))
    return out


def want_words(bits, tail_ones=False):
    """A 0/1 list as the library's bitmap (little-endian u64 words, bit g & 63
    of word g >> 6); tail_ones sets the last word's bits past len(bits)."""
    nwords = (len(bits) + 63) // 64
    out = bytearray(8 * nwords)
    for g, b in enumerate(bits):
        if b:
            out[g >> 3] |= 1 << (g & 7)
    if tail_ones:
        for g in range(len(bits), 64 * nwords):
            out[g >> 3] |= 1 << (g & 7)
    return bytes(out)


def same(result, want):
    """Does a SourcesResult carry exactly the restatement's answer?"""
    src, file, block, stats, skipped = want
    return (result.nblk == len(src) and result.src == src and result.file == file and
            result.block == block and result.skipped == skipped and
            all(result.stats[k] == v for k, v in stats.items()))
