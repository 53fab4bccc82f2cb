"""cir_index_frame / cir_index_digests / cir_index_digests_dev /
cir_index_work_bytes without a GPU: the declarations, the ctypes table and
INTEGRATION.md's extern block, the Python names, the frame and the host form
(ctx = NULL) against dirsig_oracle.parse over the reference's fixture and
hand-made and seeded random indexes, the error codes of the host parser, the
argument checks of the device call that need no device, and the rule which
lines the device takes (ciruela_amd/csrc/idxscan.hpp) under AddressSanitizer
and UBSan against the host parser (tools/index_accept_fuzz.cpp, a stand-alone
program).

Reference: the index text is parsed on a host thread by every consumer
(ThreadedBlockReader::register_dir, src/blocks.rs:150-183).  No expected value
comes from the library: tests/index_cases.py builds the indexes with
dirsig_oracle.emit over random digests and reads the expected arrays off
dirsig_oracle.parse.
"""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import index_cases
from ciruela_amd import _native

NEW = ("cir_index_frame", "cir_index_work_bytes", "cir_index_digests_dev", "cir_index_digests")
U64 = (1 << 64) - 1


def _header():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_entry_points_and_constants():
    text = _header()
    assert re.search(r"\buint64_t cir_index_work_bytes\s*\(", text)
    for name in ("cir_index_frame", "cir_index_digests_dev", "cir_index_digests"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
    for define in ("CIR_INDEX_RES_FIELDS 5", "CIR_INDEX_STATS_FIELDS 4", "CIR_INDEX_OK 0",
                   "CIR_INDEX_CAPACITY 1", "CIR_INDEX_DECLINED 2"):
        assert re.search(r"#define %s\b" % define, text), define
    full = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    assert "CIR_SOURCES_PARSE=host" in full


def test_ctypes_table_and_integration_block_bind_them():
    for name in NEW:
        assert name in _native._SIGS
    assert len(_native._SIGS["cir_index_frame"][1]) == 6
    assert len(_native._SIGS["cir_index_digests_dev"][1]) == 14
    assert len(_native._SIGS["cir_index_digests"][1]) == 11
    assert _native.lib.cir_index_work_bytes.restype is ctypes.c_uint64
    assert (_native.CIR_INDEX_RES_FIELDS, _native.CIR_INDEX_STATS_FIELDS) == (5, 4)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))


def test_python_interface():
    import ciruela_amd as ca
    assert callable(ca.index_digests) and callable(ca.Context.index_digests_dev)
    assert "index_digests" in ca.__all__ and "IndexDigests" in ca.__all__
    assert len(ca.IndexDigests.STATS_FIELDS) == _native.CIR_INDEX_STATS_FIELDS
    assert "src/blocks.rs:150-183" in ca.__doc__


def test_work_bytes_and_tile():
    """24 bytes per tile of the text and a spare: pure, monotonic, and the
    tile the GPU tests place their boundaries at is exported."""
    f = _native.lib.cir_index_work_bytes
    tile = _native.lib.cir_debug_index_tile_bytes()
    assert tile == 4096
    assert [f(n) for n in (0, 1, tile - 1, tile, 10 * tile + 5)] == [48, 48, 48, 72, 288]
    assert f(1 << 36) == 24 * ((1 << 24) + 2)


def frame(index):
    ht, bs = ctypes.c_int(-1), ctypes.c_uint64(U64)
    b0, b1 = ctypes.c_uint64(U64), ctypes.c_uint64(U64)
    buf = ctypes.create_string_buffer(index, max(len(index), 1))
    rc = _native.lib.cir_index_frame(buf, len(index), ctypes.byref(ht), ctypes.byref(bs),
                                     ctypes.byref(b0), ctypes.byref(b1))
    return rc, ht.value, bs.value, b0.value, b1.value


def check_against_the_oracle(index):
    import ciruela_amd as ca
    exp = index_cases.expected(index)
    rc, ht, bs, b0, b1 = frame(index)
    assert (rc, ht, bs) == (_native.CIR_OK, exp[0], exp[1])
    assert b0 == index.index(b"\n") + 1
    assert b1 == index.rindex(b"\n", 0, len(index) - 1) + 1
    res = ca.index_digests(index)
    assert index_cases.same(res, exp)
    assert res.stats == dict(on_device=0, fell_back=0, declined_at=None, uploaded_bytes=0)
    for first, size, file, off in res.runs:
        assert index[int(off):int(off) + 1] == b" "
    return res


def test_the_reference_fixture(dirsig_example):
    res = check_against_the_oracle(dirsig_example["index"].encode())
    assert (res.hash_type, res.block_size, res.nfiles, res.nblk) == (2, 32768, 4, 3)
    assert [list(map(int, r[:3])) for r in res.runs] == [[0, 6, 0], [1, 7, 2], [2, 10, 3]]
    assert bytes(res.digests[1]).hex() == \
        "6d7f5f9804ee4dbc1ff7e12c7665387e0119e8ea629996c52d38b75c12ad0acf"


def hand_made():
    rng = random.Random(77)
    f = index_cases.file_entry
    out = {}
    for hash_name in ("blake2b/256", "sha512/256"):
        out["empty_body_" + hash_name[:3]] = index_cases.emit([], 64, hash_name)
        out["mixed_" + hash_name[:3]] = index_cases.emit(
            [(b"/", [f(rng, b"e", 0, 64), ("s", b"l", b"e"), f(rng, b"x", 130, 64, exe=True)]),
             (b"/empty dir", []),
             (b"/d/\xff\x01", [f(rng, b"a b\\c", 64, 64), ("s", b"\tl", b"../a b"),
                               f(rng, b"...", 63, 64), f(rng, b"z", 65, 64)])], 64, hash_name)
    out["one_empty_file"] = index_cases.emit([(b"/", [f(rng, b"e", 0, 4096)])], 4096)
    out["block_size_1"] = index_cases.emit([(b"/", [f(rng, b"b", 5, 1), f(rng, b"c", 1, 1)])], 1)
    out["sizes"] = index_cases.emit(
        [(b"/", [f(rng, b"s%d" % i, s, 32768) for i, s in
                 enumerate((32767, 32768, 32769, 65536))])], 32768)
    return out


HAND = hand_made()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_indexes(name):
    res = check_against_the_oracle(HAND[name])
    if name == "block_size_1":
        assert res.nblk == 6 and [int(r[1]) for r in res.runs] == [5, 1]
    if name == "sizes":
        assert [int(r[0]) for r in res.runs] == [0, 1, 2, 4] and res.nblk == 6


def test_random_indexes():
    for seed in range(60):
        check_against_the_oracle(index_cases.random_index(3000 + seed, max_bytes=16384))


def test_lenient_text_the_host_parser_takes():
    """Upper-case hex, runs of spaces and a default block size: outside the
    device's canonical form, inside the host parser's.  hash_off is the first
    token's leading space however many spaces precede it."""
    import ciruela_amd as ca
    d = [bytes(range(i, i + 32)) for i in (0, 100)]
    index = (b"DIRSIGNATURE.v1  blake2b/256\n/\n  a   f  32769   " + d[0].hex().upper().encode() +
             b"  " + d[1].hex().encode() + b" \n" + b"AB" * 32 + b"\n")
    res = ca.index_digests(index)
    assert (res.hash_type, res.block_size, res.nfiles) == (1, 32768, 1)
    assert [bytes(x) for x in res.digests] == d
    assert res.runs.tolist() == [[0, 32769, 0, index.index(b"32769") + 5]]
    assert frame(index)[:3] == (_native.CIR_OK, 1, 32768)


GOOD = HAND["mixed_bla"]


@pytest.mark.parametrize("bad,code", [
    (b"", "EPARSE"), (b"garbage", "EPARSE"), (b"garbage\n", "EPARSE"),
    (GOOD[:-1], "EPARSE"),                                           # no final newline
    (GOOD.replace(b"DIRSIGNATURE.v1", b"DIRSIGNATURE.v2"), "EPARSE"),
    (GOOD.replace(b"blake2b/256", b"md5/128"), "EPARSE"),
    (GOOD.replace(b"block_size=64", b"block_size=0"), "EPARSE"),
    (GOOD.replace(b"block_size=64", b"block_size=6x"), "EPARSE"),
    (GOOD[:GOOD.rindex(b"\n", 0, len(GOOD) - 1) + 1] + b"zz\n", "EPARSE"),  # the footer is not hex
    (GOOD[:GOOD.rindex(b"\n", 0, len(GOOD) - 1) + 1] + b"\n", "EPARSE"),    # an empty footer
])
def test_frame_and_host_form_fail_alike(bad, code):
    """What the frame rejects the parser rejects, with the same code."""
    import ciruela_amd as ca
    assert frame(bad)[0] == getattr(_native, "CIR_" + code)
    assert b"error parsing index" in _native.lib.cir_last_error()
    with pytest.raises(ca.CiruelaError) as e:
        ca.index_digests(bad)
    assert e.value.status == getattr(_native, "CIR_" + code)


def test_body_errors_match_the_parser():
    """CIR_EPARSE for a body the parser rejects, CIR_EHASHSIZE for a 62-digit
    token; the frame does not look at the body."""
    import ciruela_amd as ca
    head = b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n"
    foot = b"ab" * 32 + b"\n"
    cases = [
        (head + b"  f f 10 " + b"ab" * 31 + b"\n" + foot, _native.CIR_EHASHSIZE),
        (head + b"  f f 10 " + b"zz" * 32 + b"\n" + foot, _native.CIR_EPARSE),
        (head + b"  f f 5000 " + b"ab" * 32 + b"\n" + foot, _native.CIR_EPARSE),
        (head + b"  .. f 0\n" + foot, _native.CIR_EPARSE),
        (head + b"  f q 0\n" + foot, _native.CIR_EPARSE),
        (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n  f f 0\n" + foot, _native.CIR_EPARSE),
        (head + b"  f f 18446744073709551616\n" + foot, _native.CIR_EPARSE),
    ]
    for index, code in cases:
        assert frame(index)[0] == _native.CIR_OK
        with pytest.raises(ca.CiruelaError) as e:
            ca.index_digests(index)
        assert e.value.status == code, index


def test_null_arguments():
    lib = _native.lib
    index = GOOD
    out = dict(ht=ctypes.pointer(ctypes.c_int()), bs=ctypes.pointer(ctypes.c_uint64()),
               dg=ctypes.pointer(ctypes.c_void_p()), nblk=ctypes.pointer(ctypes.c_uint64()),
               rn=ctypes.pointer(ctypes.c_void_p()), nruns=ctypes.pointer(ctypes.c_size_t()),
               nfiles=ctypes.pointer(ctypes.c_size_t()), stats=(ctypes.c_uint64 * 4)())
    for null in out:
        a = dict(out, **{null: None})
        assert lib.cir_index_digests(None, index, len(index), *[a[k] for k in out]) == \
            _native.CIR_EINVAL, null
    assert lib.cir_index_digests(None, None, 0, *out.values()) == _native.CIR_EINVAL
    u = ctypes.c_uint64()
    assert lib.cir_index_frame(None, 0, out["ht"], out["bs"], ctypes.byref(u),
                               ctypes.byref(u)) == _native.CIR_EINVAL
    assert lib.cir_index_frame(index, len(index), None, out["bs"], ctypes.byref(u),
                               ctypes.byref(u)) == _native.CIR_EINVAL


def test_index_digests_dev_argument_checks():
    """Every CIR_EINVAL case, all decided before any device call (the
    addresses are never dereferenced)."""
    lib = _native.lib
    ok = dict(ctx=None, text=1 << 20, len=10000, b0=40, b1=9000, bs=64, dg=1 << 21, capb=153,
              runs=1 << 22, capr=136, work=1 << 23, wb=lib.cir_index_work_bytes(10000),
              res=1 << 24, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_index_digests_dev(*[a[k] for k in ok])
    for kw in (dict(text=None), dict(dg=None), dict(runs=None), dict(work=None), dict(res=None)):
        assert call(**kw) == _native.CIR_EINVAL, kw
        assert b"null" in lib.cir_last_error()
    for kw in (dict(dg=(1 << 21) + 8), dict(text=(1 << 20) + 4), dict(runs=(1 << 22) + 1),
               dict(work=(1 << 23) + 2), dict(res=(1 << 24) + 4)):
        assert call(**kw) == _native.CIR_EINVAL, kw
        assert b"aligned" in lib.cir_last_error()
    for kw in (dict(b0=9001), dict(b1=10001), dict(bs=0), dict(wb=ok["wb"] - 1),
               dict(capb=1 << 32), dict(len=(1 << 36) + 1, b1=9000,
                                        wb=lib.cir_index_work_bytes((1 << 36) + 1))):
        assert call(**kw) == _native.CIR_EINVAL, kw


def test_acceptance_rule_under_asan_and_ubsan(tmp_path):
    """tools/index_accept_fuzz.cpp: a few thousand seeded random indexes and a
    mutation of each through the shared header's host loop and through
    dirsig::parse; whatever the device rule takes the parser takes, with the
    same counts, runs and digests.  A compile failure fails the test."""
    exe = str(tmp_path / "index_accept_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "index_accept_fuzz.cpp"),
                        os.path.join(csrc, "dirsig.cpp"), "-o", exe], capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"index_accept_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
