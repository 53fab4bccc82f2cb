"""Restatement of the emit rule (ciruela_amd/csrc/emit.hpp) for the tests: the
index of a flat file list through the oracle's emitter, and the body bytes of
a piece table one byte at a time.  Test infrastructure only."""
import hashlib

import dirsig_oracle as o

HASHLIB = {"blake2b/256": lambda b: hashlib.blake2b(b, digest_size=32).digest(),
           "sha512/256": lambda b: hashlib.new("sha512_256", b).digest()}


def dir_list(files):
    """files: [(path bytes, exe, size, [digests])] in any order -> the
    oracle's [(vpath, [entries])] in emission order: per directory its files
    by name, then its subdirectories by name; "/" always, every other
    directory because a file lies below it."""
    tree = {}
    for path, exe, size, digests in files:
        parts = path.split(b"/")[1:]
        node = tree
        for c in parts[:-1]:
            node = node.setdefault(c, {})
            assert isinstance(node, dict), path
        assert parts[-1] not in node, path
        node[parts[-1]] = ("f", parts[-1], exe, size, digests)
    out = []

    def rec(vpath, node):
        names = sorted(node)
        out.append((vpath, [node[n] for n in names if not isinstance(node[n], dict)]))
        for n in names:
            if isinstance(node[n], dict):
                rec(b"/" + n if vpath == b"/" else vpath + b"/" + n, node[n])

    rec(b"/", tree)
    return out


def index_of(files, block_size, hash_name="blake2b/256"):
    """The index of [(path, exe, size, [digests])] by the oracle's emitter."""
    return o.emit(hash_name, block_size, dir_list(files), keep_empty=True)


def index_of_data(files, block_size, hash_name="blake2b/256"):
    """The index of [(path, exe, data bytes)] with hashlib digests."""
    h = HASHLIB[hash_name]
    return index_of([(p, exe, len(data),
                      [h(data[i:i + block_size]) for i in range(0, len(data), block_size)])
                     for p, exe, data in files], block_size, hash_name)


def flat_digests(files, block_size, hash_name="blake2b/256"):
    """The flat digest list of [(path, exe, data)] in the files' own order."""
    h = HASHLIB[hash_name]
    return b"".join(h(data[i:i + block_size]) for _, _, data in files
                    for i in range(0, len(data), block_size))


def body_of_tables(pieces, lits, digests, body_len):
    """emit::byte_at for every byte of [0, round_up(body_len, 16)): pieces =
    [(out_off, lit_off, lit_len, first_block, nblk)] with ascending out_off.
    Returns (bytes, the count of pieces with a range outside the arrays that
    start below body_len)."""
    ndig = len(digests) // 32
    cap = (body_len + 15) // 16 * 16
    out = bytearray(cap)
    bad = 0
    for k, (out_off, lit_off, lit_len, first, nblk) in enumerate(pieces):
        end = pieces[k + 1][0] if k + 1 < len(pieces) else body_len
        end = min(end, body_len)
        if lit_off + lit_len > len(lits) or first + nblk > ndig:
            bad += out_off < body_len
            continue
        text = lits[lit_off:lit_off + lit_len]
        for b in range(first, first + nblk):
            text += b" " + digests[32 * b:32 * b + 32].hex().encode()
        text += b"\n"
        text = text[:max(end - out_off, 0)]
        out[out_off:out_off + len(text)] = text
    return bytes(out), bad
