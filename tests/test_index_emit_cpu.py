"""cir_index_emit, cir_index_emit_layout and cir_index_emit_tables on the CPU:
the emit rule (ciruela_amd/csrc/emit.hpp) against its restatement
(tests/emit_restate.py over the oracle's emitter), the restatement pinned to
the oracle's directory scan, the error cases, and the rule's header under
ASan and UBSan (tools/emit_fuzz.cpp).  No GPU.

(cir_index_rewrite of an emitted index needs a context, so that round trip is
in tests/test_gpu_index_emit.py.)"""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import dirsig_oracle as o
import emit_restate as er
from conftest import ROOT

import ciruela_amd as ca
from ciruela_amd import _native as _n

BS = 4096
SHA = ca.HashType.sha512_256()


def _data(seed, n):
    return random.Random(seed).randbytes(n)


def _emit(files, bs=BS, hash_name="blake2b/256", **kw):
    """ca.index_emit over [(path, exe, data)] with hashlib digests."""
    ht = SHA if hash_name == "sha512/256" else None
    return ca.index_emit([(p, len(d), exe) for p, exe, d in files],
                         er.flat_digests(files, bs, hash_name), bs, ht, **kw)


# the cases of the issue, each [(path, exe, data)] in a deliberately unsorted order
CASES = {
    "no_files": [],
    "sizes": [(b"/s%d" % k, False, _data(k, n))
              for k, n in enumerate((BS + 1, 0, BS, 1, BS - 1, 3 * BS + 5))],
    "exe": [(b"/bin/tool", True, _data(1, 10)), (b"/bin/data", False, _data(2, 10)),
            (b"/run", True, b"")],
    "escapes": [(b"/with space/a\\b", False, _data(3, 5)), (b"/\xff\x01/\x7f", True, _data(4, BS)),
                (b"/tab\there", False, b""), (b"/d/\xc3\xa9", False, _data(5, 2 * BS))],
    # files first, then subdirectories, both bytewise: a, a.b, then a.c/
    "files_then_dirs": [(b"/a.c/z", False, _data(6, 3)), (b"/a.b", False, _data(7, 3)),
                        (b"/a", False, _data(8, 3)), (b"/a.c/a", False, b"x"),
                        (b"/a.c/b/c", False, b"y"), (b"/Z/q", False, b"z"), (b"/b", False, b"")],
    "deep_and_siblings": [(b"/d/e/f/g", False, b"1"), (b"/d/e/h", False, b"2"),
                          (b"/d1/x", False, b"3"), (b"/d/x", False, b"4"), (b"/c/e/f/g", False, b"5"),
                          (b"/d/e/f/a", True, _data(9, BS + 7))],
    # a head ("  name f size") of exactly idxscan::kMaxHead = 4096 bytes
    "max_head": [(b"/" + b"n" * (4096 - 2 - 3 - 1), False, b"7"),
                 (b"/" + b"m" * (4096 - 2 - 3 - 4), True, _data(10, BS))],
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("hash_name", ["blake2b/256", "sha512/256"])
def test_index_emit_equals_the_restatement(name, hash_name):
    files = CASES[name]
    iid = []
    got = _emit(files, hash_name=hash_name, image_id=iid)
    want = er.index_of_data(files, BS, hash_name)
    assert got == want
    assert bytes(iid[0]).hex().encode() + b"\n" == want[-65:]
    assert bytes(ca.get_hash(got)) == bytes(iid[0])


def test_max_head_case_is_at_the_limit():
    want = er.index_of_data(CASES["max_head"], BS)
    heads = [ln.split(b" ")[:5] for ln in want.split(b"\n") if ln.startswith(b"  ")]
    assert sorted(len(b" ".join(h)) for h in heads) == [4096, 4096]


def test_reference_fixture(dirsig_example):
    """The reference's own index: its tree and digests through cir_index_emit
    give its bytes back (sha512/256, block size 32768)."""
    idx = dirsig_example["index"].encode()
    hash_name, bs, dirs, _ = o.parse(idx)
    files, digests = [], b""
    for vpath, entries in dirs:
        for kind, name, exe, size, dg in entries:
            assert kind == "f"
            files.append(((b"" if vpath == b"/" else vpath) + b"/" + name, size, exe))
            digests += b"".join(dg)
    assert hash_name == "sha512/256" and len(files) == 4
    assert ca.index_emit(files, digests, bs, SHA) == idx
    # the caller's order does not matter, the digests follow the files
    rev, rdig, pos = [], b"", 0
    spans = []
    for f in files:
        n = -(-f[1] // bs)
        spans.append(digests[pos:pos + 32 * n])
        pos += 32 * n
    for f, s in reversed(list(zip(files, spans))):
        rev.append(f)
        rdig += s
    assert ca.index_emit(rev, rdig, bs, SHA) == idx


@pytest.mark.parametrize("name", ["no_files", "sizes", "exe", "escapes", "files_then_dirs",
                                  "deep_and_siblings"])
def test_the_restatement_is_the_scan_oracle(name, tmp_path):
    """The rule pinned to the directory scan: the same files written into a
    temporary directory, scanned by the oracle, give the restatement's bytes."""
    files = CASES[name]
    for p, exe, d in files:
        full = os.path.join(os.fsencode(str(tmp_path)), p[1:])
        os.makedirs(os.path.dirname(full), exist_ok=True)
        with open(full, "wb") as f:
            f.write(d)
        os.chmod(full, 0o755 if exe else 0o644)
    assert o.scan(str(tmp_path), BS) == er.index_of_data(files, BS)


@pytest.mark.parametrize("name", sorted(set(CASES) - {"no_files"}))
def test_index_digests_round_trip(name):
    """index_digests of the emitted text returns the digests in emission
    order: file by file through the layout's first_block."""
    files = CASES[name]
    got = ca.index_digests(_emit(files))
    pieces, _, first, nblk, _ = ca.index_emit_layout([(p, len(d), exe) for p, exe, d in files], BS)
    flat = np.frombuffer(er.flat_digests(files, BS), dtype=np.uint8).reshape(-1, 32)
    assert nblk == len(flat) == got.nblk and got.nfiles == len(files)
    want = [flat[int(p[3]) + k] for p in pieces for k in range(int(p[4]))]
    assert np.array_equal(got.digests, np.array(want, dtype=np.uint8).reshape(-1, 32))
    # every file's blocks are where first_block says, in the caller's order
    assert sorted(int(x) for x in first) == sorted(int(p[3]) for p in pieces)


def test_layout_and_tables_against_the_restatement():
    """The pieces tile the body, and cir_index_emit_tables over them is the
    body, padded with zero bytes to 16; the byte-wise restatement agrees."""
    files = CASES["files_then_dirs"] + CASES["sizes"]
    pieces, lits, _, nblk, body_len = ca.index_emit_layout(
        [(p, len(d), exe) for p, exe, d in files], BS)
    digests = er.flat_digests(files, BS)
    want = er.index_of_data(files, BS)
    body_want = want[want.index(b"\n") + 1:-65]
    assert body_len == len(body_want) and nblk == len(digests) // 32
    off = 0
    for out_off, lit_off, lit_len, first, nb in pieces.tolist():
        assert out_off == off and lit_off + lit_len <= len(lits)
        off += lit_len + 65 * nb + 1
    assert off == body_len
    body, bad = ca.index_emit_tables(pieces.tobytes(), lits, digests, body_len)
    cap = (body_len + 15) // 16 * 16
    assert bad == 0 and body == body_want + bytes(cap - body_len)
    assert er.body_of_tables(pieces.tolist(), lits, digests, body_len) == (body, 0)


def test_tables_with_ranges_outside_the_arrays():
    """A piece whose literal or block range lies outside the arrays yields
    zero bytes and is counted; the others are written as ever."""
    lits = b"0123456789abcdef" * 4
    digests = _data(11, 32 * 4)
    pieces, off = [], 0
    for lit_off, lit_len, first, nb in ((0, 5, 0, 1), (60, 5, 1, 1), (3, 9, 3, 2), (7, 2, 2, 2),
                                        (1 << 63, 1 << 63, 0, 0), (0, 1, 1 << 62, 1 << 62),
                                        (10, 3, 0, 0)):
        pieces.append((off, lit_off, lit_len, first, nb))
        off += (lit_len if lit_len < 1000 else 7) + 65 * (nb if nb < 1000 else 1) + 1
    got = ca.index_emit_tables(np.array(pieces, dtype=np.uint64).tobytes(), lits, digests, off)
    assert got == er.body_of_tables(pieces, lits, digests, off)
    assert got[1] == 4 and b"\x00" * 60 in got[0] and got[0][:5] == b"01234"


BAD_LISTS = {
    "relative": [(b"a/b", 1)],
    "empty_path": [(b"", 1)],
    "root_only": [(b"/", 1)],
    "dot": [(b"/a/./b", 1)],
    "dotdot": [(b"/a/../b", 1)],
    "dotdot_last": [(b"/a/..", 1)],
    "empty_component": [(b"/a//b", 1)],
    "trailing_slash": [(b"/a/b/", 1)],
    "nul": [(b"/a/b\x00c", 1)],
    "duplicate": [(b"/a/b", 1), (b"/c", 1), (b"/a/b", 1)],
    "file_then_dir": [(b"/a/b", 1), (b"/a/b/c", 1)],
    "dir_then_file": [(b"/a/b/c/d", 1), (b"/a/x", 1), (b"/a/b", 0)],
    "conflict_among_siblings": [(b"/p/a", 0), (b"/p/b", 0), (b"/p/c", 0), (b"/p/b/z", 0),
                                (b"/p/a.x/y", 0)],
}


@pytest.mark.parametrize("name", sorted(BAD_LISTS))
def test_invalid_lists_are_einval(name):
    files = BAD_LISTS[name]
    digests = bytes(32 * sum(1 for _, s in files if s))
    for call in (lambda: ca.index_emit(files, digests, BS),
                 lambda: ca.index_emit_layout(files, BS)):
        with pytest.raises(ca.CiruelaError) as e:
            call()
        assert e.value.status == _n.CIR_EINVAL and e.value.detail


@pytest.mark.parametrize("ndig", [0, 1, 3])
def test_wrong_digest_count_is_einval(ndig):
    files = [(b"/a", BS + 1), (b"/b", 0)]
    with pytest.raises(ca.CiruelaError) as e:
        ca.index_emit(files, bytes(32 * ndig), BS)
    assert e.value.status == _n.CIR_EINVAL and "digest count" in e.value.detail
    assert ca.index_emit(files, bytes(64), BS)


def test_no_files_takes_null_arrays():
    import ctypes
    out, ln = ctypes.c_void_p(), ctypes.c_size_t()
    _n.check(_n.lib.cir_index_emit(_n.CIR_HASH_BLAKE2B_256, BS, None, None, None, None, 0, None, 0,
                                   ctypes.byref(out), ctypes.byref(ln), None))
    assert _n.take_buffer(out.value, ln.value) == er.index_of_data([], BS)


def test_bad_block_size_and_hash_type_are_einval():
    for bs in (0, 1 << 32):
        with pytest.raises(ca.CiruelaError) as e:
            ca.index_emit([(b"/a", 0)], b"", bs)
        assert e.value.status == _n.CIR_EINVAL
    with pytest.raises(ca.CiruelaError) as e:
        ca.index_emit([(b"/a", 0)], b"", BS, ca.HashType(7, "nope"))
    assert e.value.status == _n.CIR_EINVAL


def test_index_memory_needs_contiguous_data():
    class Strided:
        def data_ptr(self):
            return 4096

        def is_contiguous(self):
            return False

        def element_size(self):
            return 1

        def numel(self):
            return 8

    with pytest.raises(ValueError):
        ca.index_memory([(b"/a", Strided())], context=object())
    with pytest.raises(TypeError):
        ca.index_memory([(b"/a", b"host bytes")], context=object())


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_emit_fuzz_under_asan_ubsan(tmp_path):
    """tools/emit_fuzz.cpp: seeded random file lists; the layout, byte_at and
    fill16 against a plain string builder over a tree built another way, every
    table in a heap buffer of exactly its size, invalid lists and tables with
    ranges outside the arrays included.  A compile failure fails the test."""
    exe = str(tmp_path / "emit_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "emit_fuzz.cpp"),
                        os.path.join(csrc, "dirsig.cpp"), "-o", exe], capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "1500", "7"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"emit_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 1500
    m = re.search(rb"(\d+) files, (\d+) directory lines, (\d+) blocks, (\d+) body bytes; (\d+) "
                  rb"invalid lists rejected; (\d+) bad pieces counted", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr
