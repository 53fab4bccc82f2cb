"""The loader sweep's case builder (loader_cases.py) on the CPU: the grids'
own properties, and hashlib's digests -- the sweep's reference -- equal to the
C oracle's for every descriptor of both grids and both hash types, which ties
that reference to the one the rest of the suite uses."""
import hashlib

import numpy as np
import pytest

import loader_cases as lc


@pytest.fixture(scope="module", params=sorted(lc.GRIDS))
def g(request):
    return lc.named(request.param)


def test_grid_sizes():
    lane, quad = lc.named("lane"), lc.named("quad")
    assert lane.n == quad.n == 8192
    assert (int(lane.lens.min()), int(lane.lens.max())) == (0, 511)
    assert (int(quad.lens.min()), int(quad.lens.max())) == (1024, 1535)
    assert lane.arena.size == 8192 * 640 and quad.arena.size == 8192 * 1664


def test_every_case_once(g):
    cases = list(zip(g.k.tolist(), g.t.tolist(), g.a.tolist()))
    assert sorted(cases) == [(k, t, a) for k in sorted(g.ks) for t in range(128)
                             for a in range(16)]
    assert (g.lens.astype(np.int64) == 128 * g.k + g.t).all()


def test_starts_have_their_alignment(g):
    assert (g.offs.astype(np.int64) % 16 == g.a).all()
    assert g.stride % 128 == 0 and g.stride >= int(g.lens.max()) + 32
    assert (g.offs.astype(np.int64) == np.arange(g.n) * g.stride + g.a).all()


def test_blocks_and_guards_disjoint_and_inside(g):
    """Block + GUARD bytes after it: inside the arena, and ending at or before
    the next block's start (the blocks are in ascending address order)."""
    start = g.offs.astype(np.int64)
    end = start + g.lens.astype(np.int64) + lc.GUARD
    assert lc.GUARD >= 16
    assert (start[1:] > start[:-1]).all()
    assert (end[:-1] <= start[1:]).all()
    assert start[0] >= 0 and end[-1] <= g.arena.size


def test_arena_has_no_zero_byte(g):
    assert g.arena.dtype == np.uint8 and int(g.arena.min()) >= 1
    assert len(np.unique(g.arena)) == 255  # drawn from all of 1..255
    again = lc.grid(g.ks, g.stride, g.seed)
    assert np.array_equal(again.arena, g.arena)  # seeded


def test_orders_are_permutations_of_one_set(g):
    sh, gr = g.order("shuffled"), g.order("grouped")
    assert np.array_equal(np.sort(sh), np.arange(g.n))
    assert np.array_equal(np.sort(gr), np.arange(g.n))
    assert np.array_equal(sh, g.order("shuffled"))  # seeded
    assert not np.array_equal(sh, gr)
    key = list(zip(g.a[gr].tolist(), g.k[gr].tolist(), g.t[gr].tolist()))
    assert key == sorted(key)
    # grouped: every wave of 64 descriptors has one alignment and one line count
    assert (g.a[gr].reshape(-1, 64) == g.a[gr].reshape(-1, 64)[:, :1]).all()
    assert (g.k[gr].reshape(-1, 64) == g.k[gr].reshape(-1, 64)[:, :1]).all()
    # shuffled: the waves mix alignments, including 16-B aligned with others
    mixed = [len(set(w)) for w in g.a[sh].reshape(-1, 64).tolist()]
    assert min(mixed) >= 8


def test_report_names_the_pattern():
    g = lc.named("lane")
    want = np.zeros((g.n, 32), dtype=np.uint8)
    assert lc.report(want.copy(), want, g.k, g.t, g.a, "blake2b", "context", "grouped") is None
    got = want.copy()
    bad = g.where((g.t % 4 == 3) & (g.a == 4))
    got[bad, 31] ^= 1
    msg = lc.report(got, want, g.k, g.t, g.a, "blake2b", "context", "grouped")
    assert msg.startswith("%d of 8192 digests differ" % bad.size)
    assert "('blake2b', 'context', 'grouped', 0, 3, 4)" in msg
    assert "distinct t: %s" % list(range(3, 128, 4)) in msg and "distinct a: [4]" in msg


@pytest.mark.parametrize("hash_name", lc.HASHES)
def test_hashlib_equals_the_oracle(g, oracle, hash_name):
    """All 8192 digests of the grid: hashlib's against oracle_hash_blocks
    (BLAKE2b-256) or oracle_sha512_256, per descriptor."""
    if not lc.have_hashlib(hash_name):
        print("hashlib has no sha512_256 here: the oracle is compared with itself")
    want = lc.reference(hash_name, g.arena, g.offs, g.lens, oracle)
    got = np.zeros((g.n, 32), dtype=np.uint8)
    base = g.arena.ctypes.data
    if hash_name == "blake2b":
        assert oracle.oracle_hash_blocks(base, g.offs.ctypes.data, g.lens.ctypes.data, g.n,
                                         got.ctypes.data, 4) == 0
    else:
        for i, (o, ln) in enumerate(zip(g.offs.tolist(), g.lens.tolist())):
            assert oracle.oracle_sha512_256(got.ctypes.data + 32 * i, base + o, ln) == 0
    msg = lc.report(got, want, g.k, g.t, g.a, hash_name, "oracle", "grid")
    assert msg is None, msg
    print("%s: hashlib == oracle on %d digests" % (hash_name, g.n))


def test_reference_is_hashlib_on_the_slices():
    g = lc.named("lane")
    want = lc.named_reference("lane", "blake2b")
    for i in (0, 17, 4095, 8191):
        o, ln = int(g.offs[i]), int(g.lens[i])
        assert bytes(want[i]) == hashlib.blake2b(g.arena[o:o + ln].tobytes(),
                                                 digest_size=32).digest()
    assert bytes(lc.digest("sha512", b"abc")).hex() == \
        "53048e2681941ef99b2e29b76b4c7dabe4c2d0c634fc6d46e0e2f13107e7af23"
