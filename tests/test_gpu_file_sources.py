"""cir_index_files_dev, cir_match_files_dev and cir_file_sources with a context
on the GPU.

The kernels (ciruela_amd/csrc/files.hip): an index text to one record {name_off,
dir_off, size, first | exe << 63} per file entry, and the join of two record
lists -- per need file the first source whose first entry at the same decoded
path has equal exe flag, size and digests.  Expected values are
links_restate.expected_candidates' (scan_links, src/daemon/metadata/
hardlink_sources.rs:107-153, over dirsig_oracle.parse), cir_link_candidates'
and, for the records, a walk over the text's lines (tests/files_cases.py);
never the device path's own.  Indexes are dirsig_oracle.emit's over random
digests, so no file is hashed.  T is the text tile (cir_debug_index_tile_bytes).

Every canonical case must be answered by the device (stats on_device == 1,
why_host == 0): a silent fallback would hide a kernel bug behind the host's
correct answer.  Device calls made directly keep 0xA5-filled guard regions
behind their outputs, which must come back untouched.
"""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import dirsig_oracle
import files_cases
import index_cases
import links_restate
from files_cases import BS, f

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
POISON = 0xA5
GUARD = 256
OK, CAPACITY, DECLINED = 0, 1, 2
EXE = 1 << 63
NOSRC = (1 << 32) - 1
FOOT = b"ab" * 32 + b"\n"
WG = 256     # lanes per workgroup of the fold kernel (one per block)


@pytest.fixture(scope="module")
def T(gpu):
    return int(gpu._n.lib.cir_debug_index_tile_bytes())


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=gpu._n.CIR_STAGING_LAZY)


def frame(gpu, index):
    ht, bs = ctypes.c_int(), ctypes.c_uint64()
    b0, b1 = ctypes.c_uint64(), ctypes.c_uint64()
    gpu._n.check(gpu._n.lib.cir_index_frame(index, len(index), ctypes.byref(ht),
                                            ctypes.byref(bs), ctypes.byref(b0),
                                            ctypes.byref(b1)))
    return ht.value, bs.value, b0.value, b1.value


class Poisoned:
    """nbytes of device memory filled with 0xA5 and GUARD more behind them."""

    def __init__(self, torch, nbytes):
        self.n = nbytes
        self.t = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def guard_intact(self):
        return bool((self.t[self.n:] == POISON).all().item())

    def host(self, nbytes=None):
        return self.t[:self.n if nbytes is None else nbytes].cpu().numpy()


def run_files(gpu, index, cap=None, off_bias=0, block_bias=0, ctx=None):
    """One cir_index_files_dev call with poisoned, guarded outputs; returns
    (res[4], records (n, 4) or None)."""
    import torch
    lib = gpu._n.lib
    _, bs, b0, b1 = frame(gpu, index)
    n = len(index)
    cap = n // 8 if cap is None else cap
    text = torch.from_numpy(np.frombuffer(index, dtype=np.uint8).copy()).cuda()
    wb = lib.cir_index_files_work_bytes(n)
    recs, work, res = Poisoned(torch, 32 * cap), Poisoned(torch, wb), Poisoned(torch, 32)
    torch.cuda.synchronize()
    if ctx is not None:
        ctx.index_files_dev(text.data_ptr(), n, b0, b1, bs, recs.ptr, cap, work.ptr, wb, res.ptr,
                            off_bias=off_bias, block_bias=block_bias)
    else:
        gpu._n.check(lib.cir_index_files_dev(None, text.data_ptr(), n, b0, b1, bs, off_bias,
                                             block_bias, recs.ptr, cap, work.ptr, wb, res.ptr, 0))
    torch.cuda.synchronize()
    for o in (recs, work, res):
        assert o.guard_intact()
    r = [int(v) for v in res.host().view(np.uint64)]
    if r[0] != OK:
        if r[0] == CAPACITY:
            assert (recs.host() == POISON).all()
        return r, None
    assert r[1] <= cap
    q = recs.host().view(np.uint64).reshape(-1, 4)
    assert (q[r[1]:] == 0xA5A5A5A5A5A5A5A5).all()
    return r, q[:r[1]].copy()


def check_records(gpu, index, **kw):
    exp = files_cases.expected_records(index, kw.get("off_bias", 0), kw.get("block_bias", 0))
    r, q = run_files(gpu, index, **kw)
    nblk = len(index_cases.expected(index)[2])
    assert r == [OK, len(exp), nblk, U64], r
    assert q.shape == exp.shape and (q == exp).all(), np.nonzero((q != exp).any(1))[0][:5]
    return r


def header(extra=0, bs=BS):
    return b"DIRSIGNATURE.v1 blake2b/256 block_size=%d" % bs + b" " * extra + b"\n"


def filler(n):
    """A size-0 file line of exactly n >= 8 bytes."""
    return b"  " + b"p" * (n - 7) + b" f 0\n"


def fline(rng, name, nblk, exe=False):
    e = f(rng, name, nblk, exe=exe)
    return b"  " + name + (b" x " if exe else b" f ") + b"%d" % e[3] + \
        b"".join(b" " + d.hex().encode() for d in e[4]) + b"\n"


def pad_to(text, offset):
    """`text` plus size-0 file lines up to exactly `offset` bytes."""
    out = [text]
    left = offset - len(text)
    assert left >= 8
    while left:
        n = left if left < 80 or left - 60 < 8 else 60
        out.append(filler(n))
        left -= n
    return b"".join(out)


# ---- cir_index_files_dev -----------------------------------------------------------------

def test_directory_line_last_of_a_tile(gpu, T):
    rng = random.Random(1)
    d = b"/d/last\n"
    text = pad_to(header() + b"/\n" + fline(rng, b"a", 2), T - len(d)) + d
    assert len(text) == T
    text += fline(rng, b"b", 1, exe=True) + filler(20) + fline(rng, b"c", 3) + FOOT
    check_records(gpu, text)


def test_directory_line_first_of_the_next_tile(gpu, T):
    rng = random.Random(2)
    text = pad_to(header() + b"/\n" + fline(rng, b"a", 1), T)
    text += b"/first/of/tile\n" + fline(rng, b"b", 2) + fline(rng, b"c", 0) + FOOT
    check_records(gpu, text)
    # and one byte either side of the boundary
    for shift in (-1, 1):
        text = pad_to(header() + b"/\n" + fline(rng, b"a", 1), T + shift)
        text += b"/near\n" + fline(rng, b"b", 2) + FOOT
        check_records(gpu, text)


def test_directory_three_tiles_back_behind_a_long_line(gpu, T):
    rng = random.Random(3)
    text = header() + b"/\n" + fline(rng, b"x", 1) + b"/far/back\n" + fline(rng, b"big", 300)
    assert 300 * 65 > 3 * T
    text += fline(rng, b"after", 2) + filler(9) + b"/next\n" + fline(rng, b"n", 1) + FOOT
    check_records(gpu, text)


def test_many_directories_in_one_span(gpu, T):
    rng = random.Random(4)
    text = header() + b"/\n/a\n/b\n/c\n/d\n" + fline(rng, b"f", 1) + b"/e\n/f\n/g\n" + filler(8) + \
        b"/h\n" * 40 + fline(rng, b"g", 2, exe=True) + FOOT
    check_records(gpu, text)


def test_size0_files_first_last_and_between(gpu, T):
    rng = random.Random(5)
    text = header() + b"/\n" + filler(8) + fline(rng, b"a", 2) + filler(9) + filler(10) + \
        fline(rng, b"b", 65) + b"/d\n" + filler(11) + fline(rng, b"c", 1) + filler(12) + FOOT
    r = check_records(gpu, text)
    assert r[1] == 8
    # nothing but empty files, and no file at all
    check_records(gpu, header() + b"/\n" + filler(8) * 700 + FOOT)
    check_records(gpu, header() + b"/\n  l s t\n" + FOOT)
    check_records(gpu, header() + FOOT)


@pytest.mark.parametrize("extra", range(16))
def test_body_off_modulo_16(gpu, T, extra):
    rng = random.Random(60 + extra)
    text = header(extra) + b"/\n" + fline(rng, b"a", 3) + b"/q\n" + fline(rng, b"b", 70) + \
        filler(8) + FOOT
    check_records(gpu, text)


def test_biases_capacity_and_context_method(gpu, T, ctx):
    rng = random.Random(7)
    text = header() + b"/\n" + b"".join(fline(rng, b"f%d" % i, i % 4) for i in range(50)) + FOOT
    check_records(gpu, text, off_bias=(1 << 40) + 16, block_bias=(1 << 33) + 5)
    check_records(gpu, text, off_bias=48, block_bias=7, ctx=ctx)
    nblk = len(index_cases.expected(text)[2])
    r, q = run_files(gpu, text, cap=50)
    assert r[0] == OK and len(q) == 50
    r, q = run_files(gpu, text, cap=49)
    assert r == [CAPACITY, 50, nblk, U64] and q is None
    r, q = run_files(gpu, text, cap=0)
    assert r[0] == CAPACITY and r[1] == 50


def test_declined_line(gpu, T):
    rng = random.Random(8)
    good = fline(rng, b"a", 2)
    bad = b"  two  spaces f 0\n"
    text = pad_to(header() + b"/\n" + good, T + 100) + bad + filler(8) + FOOT
    r, q = run_files(gpu, text)
    assert r[0] == DECLINED and r[3] == text.index(bad) and q is None
    # the first of two declined lines is reported
    text2 = header() + b"/\n" + b"  raw\xc3byte f 0\n" + pad_to(good, 2 * T) + bad + FOOT
    r, q = run_files(gpu, text2)
    assert r[0] == DECLINED and r[3] == text2.index(b"  raw")


def test_bad_token_is_declined_as_by_the_digest_call(gpu, T):
    """The statuses never disagree with cir_index_digests_dev's: a bad hex
    digit inside a token -- in a long line's last token, tiles behind its head
    -- declines that line in both calls."""
    import torch
    lib = gpu._n.lib
    rng = random.Random(9)
    lines = [fline(rng, b"a", 2), fline(rng, b"big", 200), filler(8), fline(rng, b"c", 3)]
    good = header() + b"/\n" + b"".join(lines) + FOOT
    check_records(gpu, good)
    for which, at in ((1, -2), (1, 40), (3, -66), (0, 9 + 64)):    # (-66: a separator)
        ln = bytearray(lines[which])
        at = at % len(ln)
        ln[at:at + 1] = b"g"
        bad = lines[:which] + [bytes(ln)] + lines[which + 1:]
        text = header() + b"/\n" + b"".join(bad) + FOOT
        start = text.index(bytes(ln))
        r, q = run_files(gpu, text)
        assert r[0] == DECLINED and r[3] == start and q is None, r
        # the digest call's verdict on the same bytes
        _, bs, b0, b1 = frame(gpu, text)
        n = len(text)
        dtext = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        wb = lib.cir_index_work_bytes(n)
        dg, rn = Poisoned(torch, 32 * (n // 65)), Poisoned(torch, 32 * (n // 73))
        work, res = Poisoned(torch, wb), Poisoned(torch, 40)
        gpu._n.check(lib.cir_index_digests_dev(None, dtext.data_ptr(), n, b0, b1, bs, dg.ptr, n // 65,
                                               rn.ptr, n // 73, work.ptr, wb, res.ptr, 0))
        torch.cuda.synchronize()
        ri = [int(v) for v in res.host().view(np.uint64)]
        assert (ri[0], ri[4]) == (r[0], r[3])


# ---- the whole call ----------------------------------------------------------------------

def on_device(gpu, ctx, index, sources):
    """cir_file_sources with a context equals the restatement and the host
    call, and was answered by the device."""
    want, skipped = files_cases.expected(index, sources)
    got, st = gpu.file_sources(index, sources, ctx)
    assert got == want, (got[:5], want[:5])
    assert st["skipped"] == skipped
    assert st["on_device"] == 1 and st["why_host"] == 0, st
    assert gpu.link_candidates(index, sources) == want
    files = links_restate.file_entries(index)
    assert st["files"] == len(files) and st["candidates"] == len(want)
    assert st["bytes"] == sum(files[i][2] for i, _ in want)
    assert st["sources_used"] == len(sources) - skipped
    return got, st


def swapped(entry, i=0, j=1):
    d = list(entry[4])
    d[i], d[j] = d[j], d[i]
    return entry[:4] + (d,)


def emit(entries, d=b"/"):
    return index_cases.emit([(d, entries)], BS)


def fold_case(gpu, ctx, entries):
    """Every file is its own candidate; with two digests of one file swapped in
    the source that file, and no other, loses it."""
    new = emit(entries)
    got, _ = on_device(gpu, ctx, new, [new])
    assert got == [(i, 0) for i in range(len(entries))]
    for k, e in enumerate(entries):
        if len(e[4]) < 2:
            continue
        j = len(e[4]) - 1
        src = emit(entries[:k] + [swapped(e, 0, j)] + entries[k + 1:])
        got, _ = on_device(gpu, ctx, new, [src])
        assert got == [(i, 0) for i in range(len(entries)) if i != k]
        if len(e[4]) > 70:      # two digests in different waves
            src = emit(entries[:k] + [swapped(e, 1, 66)] + entries[k + 1:])
            got, _ = on_device(gpu, ctx, new, [src])
            assert got == [(i, 0) for i in range(len(entries)) if i != k]


def test_fold_file_sizes(gpu, ctx):
    rng = random.Random(10)
    fold_case(gpu, ctx, [f(rng, b"n%d" % n, n) for n in (1, 63, 64, 65, 130)])


def test_fold_one_block_files_in_one_wave(gpu, ctx):
    rng = random.Random(11)
    fold_case(gpu, ctx, [f(rng, b"one%d" % i, 1) for i in range(62)] + [f(rng, b"two", 2)])
    fold_case(gpu, ctx, [f(rng, b"one%d" % i, 1, short=3) for i in range(64)])


def test_fold_file_longer_than_three_workgroups(gpu, ctx):
    rng = random.Random(12)
    fold_case(gpu, ctx, [f(rng, b"head", 5), f(rng, b"long", 3 * WG + 1), f(rng, b"tail", 2)])


def test_fold_boundaries_on_wave_and_workgroup_edges(gpu, ctx):
    rng = random.Random(13)
    sizes = [64, 0, 64, 128, WG, 2 * WG - 1, 1, 63, 1]
    fold_case(gpu, ctx, [f(rng, b"e%d" % i, n) for i, n in enumerate(sizes)])


@pytest.mark.parametrize("case", files_cases.families(), ids=lambda c: c[0])
def test_families(gpu, ctx, case):
    _, index, sources = case
    on_device(gpu, ctx, index, sources)


@pytest.mark.parametrize("nsrc", [1, 2, 37])
def test_source_counts(gpu, ctx, nsrc):
    rng = random.Random(20 + nsrc)
    entries = [f(rng, b"f%02d" % i, rng.choice((0, 1, 2, 9))) for i in range(40)]
    new = emit(entries)
    # source j holds every file i with i % nsrc <= j, others with other content: the first
    # source that serves file i is i % nsrc
    sources = []
    for j in range(nsrc):
        sources.append(emit([e if i % nsrc <= j else f(rng, e[1], 3) for i, e in enumerate(entries)]))
    got, st = on_device(gpu, ctx, new, sources)
    assert len(got) == 40 and st["sources_used"] == nsrc
    assert got == [(i, i % nsrc) for i in range(40)]


def test_small_pools_and_need(gpu, ctx):
    rng = random.Random(30)
    entries = [f(rng, b"a", 2), f(rng, b"b", 1)]
    new = emit(entries)
    got, st = on_device(gpu, ctx, new, [emit(entries[1:])])         # a pool of one file
    assert got == [(1, 0)] and st["pool_files"] == 1
    got, st = on_device(gpu, ctx, new, [emit([]), emit([("s", b"a", b"t")])])   # an empty pool
    assert got == [] and st["pool_files"] == 0 and st["sources_used"] == 2
    got, st = on_device(gpu, ctx, emit([("s", b"l", b"t")]), [new])  # a need index without files
    assert got == [] and st["files"] == 0


def test_long_names_and_directories(gpu, ctx):
    """Names that differ only in their last byte, at the longest head the
    device rule takes (4096 bytes: "  " + name + " f " + size), and a
    directory line of 4096 bytes.  A 4096-byte name makes a head of 4103 bytes,
    which the rule declines: that case falls back, with the host's answer."""
    rng = random.Random(31)
    n = 4096 - len(b"   f 128")
    a, b = f(rng, b"n" * (n - 1) + b"a", 2), f(rng, b"n" * (n - 1) + b"b", 2)
    new = emit([a, b])
    assert max(len(l) for l in new.split(b"\n") if l.startswith(b"  ")) == 4096 + 2 * 65
    got, _ = on_device(gpu, ctx, new, [emit([b]), emit([a])])
    assert got == [(0, 1), (1, 0)]
    d1, d2 = b"/" + b"d" * 4094 + b"1", b"/" + b"d" * 4094 + b"2"
    e = f(rng, b"x", 1)
    new = index_cases.emit([(d1, [e]), (d2, [e])], BS)
    got, _ = on_device(gpu, ctx, new, [index_cases.emit([(d2, [e])], BS)])
    assert got == [(1, 0)]
    a, b = f(rng, b"m" * 4095 + b"a", 2), f(rng, b"m" * 4095 + b"b", 2)
    new = emit([a, b])
    got, st = gpu.file_sources(new, [emit([b]), emit([a])], ctx)
    assert got == [(0, 1), (1, 0)] == gpu.link_candidates(new, [emit([b]), emit([a])])
    assert st["on_device"] == 0 and st["why_host"] == gpu._n.CIR_FILE_WHY_DECLINED


def test_table_at_exactly_half_load(gpu, ctx):
    rng = random.Random(32)
    entries = [f(rng, b"t%02d" % i, 1) for i in range(32)]
    new = emit(entries)
    got, st = on_device(gpu, ctx, new, [emit(entries[:16]), emit(entries[16:])])
    assert st["pool_files"] == 32 and st["table_slots"] == 64
    assert got == [(i, i // 16) for i in range(32)]


@pytest.mark.parametrize("chunk", range(6))
def test_random_sweep(gpu, ctx, chunk):
    for seed in range(50 * chunk, 50 * chunk + 50):
        index, sources = files_cases.random_case(seed)
        on_device(gpu, ctx, index, sources)


def test_largest_case(gpu, ctx):
    """About 20,000 files with 200,000 blocks against 4 sources: each source an
    older version with a different tenth of the files changed."""
    rng = random.Random(40)
    pool = [rng.randbytes(32) for _ in range(4096)]

    def content(n):
        return [pool[rng.randrange(4096)] for _ in range(n)]
    entries = []
    for i in range(20000):
        n = rng.choice((0, 1, 2, 5, 10, 20, 32))
        entries.append(("f", b"file%05d" % i, i % 7 == 0, n * BS, content(n)))
    dirs = lambda es: [(b"/" if k == 0 else b"/dir%03d" % k, es[k * 100:(k + 1) * 100])
                       for k in range(200)]
    new = index_cases.emit(dirs(entries), BS)
    sources = []
    for j in range(4):
        es = [("f", e[1], e[2], e[3], content(len(e[4]))) if (i + j) % 10 < 3 else e
              for i, e in enumerate(entries)]
        sources.append(index_cases.emit(dirs(es), BS))
    # by construction: source j changed file i when (i + j) % 10 < 3 (an empty file stays equal)
    want = [(i, next(j for j in range(4) if (i + j) % 10 >= 3 or not e[4]))
            for i, e in enumerate(entries)]
    got, st = gpu.file_sources(new, sources, ctx)
    assert got == want == gpu.link_candidates(new, sources)
    assert st["on_device"] == 1 and st["why_host"] == 0, st
    assert st["files"] == 20000 and st["pool_files"] == 80000 and st["candidates"] == 20000
    assert st["bytes"] == sum(e[3] for e in entries)
    assert 190000 < sum(len(e[4]) for e in entries) < 210000


# ---- fallbacks ---------------------------------------------------------------------------

def host_answer(gpu, ctx, index, sources, why):
    got, st = gpu.file_sources(index, sources, ctx)
    host, hst = gpu.file_sources(index, sources, None)
    assert got == host == gpu.link_candidates(index, sources)
    assert st["on_device"] == 0 and st["why_host"] == why, st
    assert st["table_slots"] == 0
    for k in ("files", "candidates", "bytes", "pool_files", "sources_used", "skipped"):
        assert st[k] == hst[k], k
    return got


def test_fallback_non_canonical_texts(gpu, ctx):
    rng = random.Random(50)
    entries = [f(rng, b"a", 2), f(rng, b"b", 1), f(rng, b"raw", 1)]
    new = emit(entries)
    declined = gpu._n.CIR_FILE_WHY_DECLINED
    double = new.replace(b"  b f ", b"  b  f ")
    assert host_answer(gpu, ctx, double, [new], declined) == [(0, 0), (1, 0), (2, 0)]
    assert host_answer(gpu, ctx, new, [double], declined) == [(0, 0), (1, 0), (2, 0)]
    raw = new.replace(b"  raw f", b"  r\xc3w f")
    assert host_answer(gpu, ctx, raw, [new, raw], declined) == [(0, 0), (1, 0), (2, 1)]
    # upper-case escapes decode on both paths; the device takes them
    up = new.replace(b"  raw f", b"  r\\x4Aw f")
    got, st = gpu.file_sources(up, [new.replace(b"  raw f", b"  rJw f")], ctx)
    assert got == [(0, 0), (1, 0), (2, 0)] and st["on_device"] == 1


def test_fallback_source_that_does_not_parse(gpu, ctx):
    rng = random.Random(51)
    entries = [f(rng, b"a", 2), f(rng, b"b", 1)]
    new = emit(entries)
    # the frame is fine, one hash is missing: the host skips it, the device declines it
    broken = new.replace(b" " + entries[0][4][1].hex().encode(), b"", 1)
    got = host_answer(gpu, ctx, new, [broken, new], gpu._n.CIR_FILE_WHY_DECLINED)
    assert got == [(0, 1), (1, 1)]
    # a bad hex digit shows only in the decode pass
    badhex = new.replace(entries[1][4][0].hex().encode(), b"g" + entries[1][4][0].hex().encode()[1:])
    got = host_answer(gpu, ctx, new, [badhex, new], gpu._n.CIR_FILE_WHY_DECLINED)
    assert got == [(0, 1), (1, 1)]
    # a new index that does not parse is the host's error
    with pytest.raises(gpu.CiruelaError) as ei:
        gpu.file_sources(broken, [new], ctx)
    assert ei.value.status == gpu._n.CIR_EPARSE
    with pytest.raises(gpu.CiruelaError) as eh:
        gpu.file_sources(broken, [new], None)
    assert str(ei.value) == str(eh.value)


CHILD = r"""
import os
import sys
sys.path[:0] = [%r, %r, %r]
import ciruela_amd as ca
import files_cases
ctx = ca.Context(device_mask=1, staging_bytes=ca._n.CIR_STAGING_LAZY)
_, index, sources = files_cases.families()[0]
for mode in ("host", "device", "host"):      # (read per call)
    assert os.environ["CIR_LINKS_MATCH"] == "host"
    if mode == "device":
        del os.environ["CIR_LINKS_MATCH"]
    got, st = ca.file_sources(index, sources, ctx)
    os.environ["CIR_LINKS_MATCH"] = "host"
    assert got == files_cases.expected(index, sources)[0], got
    print(st["on_device"], st["why_host"], st["table_slots"])
"""


def test_fallback_by_environment_in_a_child(gpu):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300,
                       env=dict(os.environ, CIR_LINKS_MATCH="host"))
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.split() == b"0 4 0 1 0 64 0 4 0".split(), p.stdout


# ---- cir_match_files_dev directly --------------------------------------------------------

class DevJoin:
    """The need index and its sources (canonical, one header) in one device
    arena, parsed by cir_index_digests_dev and cir_index_files_dev with the
    biases set, ready for cir_match_files_dev.  Counts come from the text walk
    of tests/files_cases.py."""

    def __init__(self, gpu, index, sources, stream=0):
        import torch
        self.torch, self.gpu, lib = torch, gpu, gpu._n.lib
        texts = [index] + list(sources)
        offs, total = [], 0
        for t in texts:
            offs.append(total)
            total += (len(t) + 15) & ~15
        self.total = total
        arena = np.full(total + 16, 0x0A, dtype=np.uint8)
        for t, o in zip(texts, offs):
            arena[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
        self.h_arena = torch.from_numpy(arena).pin_memory()
        self.arena = torch.full((total + 16,), POISON, dtype=torch.uint8, device="cuda")
        exp = [index_cases.expected(t) for t in texts]
        self.nfiles = [e[4] for e in exp]
        self.nblk = [len(e[2]) for e in exp]
        self.bs = exp[0][1]
        nf, nb = self.nfiles[0], self.nblk[0]
        pf, pb = sum(self.nfiles[1:]), sum(self.nblk[1:])
        self.nf, self.nb, self.pf, self.pb = nf, nb, pf, pb
        P = lambda n: Poisoned(torch, n)
        self.ndig, self.pdig = P(32 * nb), P(32 * pb)
        self.nrec, self.prec = P(32 * nf), P(32 * pf)
        self.wb = lib.cir_match_files_work_bytes(nf, pf)
        self.work, self.csrc, self.cfile, self.res = P(self.wb), P(4 * nf), P(8 * nf), P(32)
        first = np.cumsum([0] + self.nfiles[1:]).astype(np.uint64)
        self.first = torch.from_numpy(first).cuda()
        self.scratch = []
        self.texts, self.offs = texts, offs
        self.frames = [frame(gpu, t) for t in texts]

    def upload(self, stream=None):
        self.arena.copy_(self.h_arena, non_blocking=True)

    def parse(self, stream=0):
        torch, lib, gpu = self.torch, self.gpu._n.lib, self.gpu
        fa = ba = 0
        for k, (t, o) in enumerate(zip(self.texts, self.offs)):
            n = len(t)
            _, bs, b0, b1 = self.frames[k]
            iw, fw = lib.cir_index_work_bytes(n), lib.cir_index_files_work_bytes(n)
            runs, iwork, ires = Poisoned(torch, 32 * (n // 73)), Poisoned(torch, iw), Poisoned(torch, 40)
            fwork, fres = Poisoned(torch, fw), Poisoned(torch, 32)
            self.scratch += [runs, iwork, ires, fwork, fres]
            dig = self.ndig.ptr if k == 0 else self.pdig.ptr + 32 * ba
            rec = self.nrec.ptr if k == 0 else self.prec.ptr + 32 * fa
            gpu._n.check(lib.cir_index_digests_dev(None, self.arena.data_ptr() + o, n, b0, b1, bs,
                                                   dig, self.nblk[k], runs.ptr, n // 73, iwork.ptr,
                                                   iw, ires.ptr, stream))
            gpu._n.check(lib.cir_index_files_dev(None, self.arena.data_ptr() + o, n, b0, b1, bs, o,
                                                 0 if k == 0 else ba, rec, self.nfiles[k], fwork.ptr,
                                                 fw, fres.ptr, stream))
            if k:
                fa += self.nfiles[k]
                ba += self.nblk[k]

    def match(self, seed, verify=0, stream=0, ctx=None):
        a = self.arena.data_ptr()
        need = (a, self.total, self.nrec.ptr, self.nf, self.ndig.ptr, self.nb)
        pool = (a, self.total, self.prec.ptr, self.pf, self.pdig.ptr, self.pb)
        nsrc = len(self.texts) - 1
        if ctx is not None:
            ctx.match_files_dev(need, pool, self.first.data_ptr(), nsrc, self.bs, seed, self.work.ptr,
                                self.wb, self.csrc.ptr, self.cfile.ptr, self.res.ptr,
                                d_pool_verify=verify, stream=stream)
        else:
            self.gpu._n.check(self.gpu._n.lib.cir_match_files_dev(
                None, *need, *pool, self.first.data_ptr(), nsrc, self.bs, verify, seed,
                self.work.ptr, self.wb, self.csrc.ptr, self.cfile.ptr, self.res.ptr, stream))

    def outputs(self):
        return [self.ndig, self.pdig, self.nrec, self.prec, self.work, self.csrc, self.cfile,
                self.res] + self.scratch

    def answer(self):
        for o in self.outputs():
            assert o.guard_intact()
        res = [int(v) for v in self.res.host().view(np.uint64)]
        src = self.csrc.host().view(np.uint32)
        fil = self.cfile.host().view(np.uint64)
        return res, [int(v) for v in src], [int(v) for v in fil]


def expected_direct(index, sources):
    """(cand_src, cand_file) per need file from the restatement's rule."""
    need = links_restate.file_entries(index)
    tabs = []
    for s in sources:
        t = {}
        for k, (path, exe, size, dg) in enumerate(links_restate.file_entries(s)):
            t.setdefault(path, (k, exe, size, dg))
        tabs.append(t)
    cs, cf = [], []
    for path, exe, size, dg in need:
        hit = (NOSRC, U64)
        for j, t in enumerate(tabs):
            if path in t and t[path][1:] == (exe, size, dg):
                hit = (j, t[path][0])
                break
        cs.append(hit[0])
        cf.append(hit[1])
    return cs, cf


def test_match_files_dev_direct_and_collision(gpu, ctx):
    import torch
    rng = random.Random(70)
    entries = [f(rng, b"a", 3), f(rng, b"b", 0), f(rng, b"c", 66, exe=True), f(rng, b"d", 1)]
    new = emit(entries)
    s0 = emit([f(rng, b"zz", 2), entries[2], f(rng, b"a", 3), entries[0]])   # /a: first entry wins
    s1 = emit([entries[1], entries[0], entries[3]])
    j = DevJoin(gpu, new, [s0, s1])
    j.upload()
    j.parse()
    for seed, c in ((1, None), (0xDEADBEEF12345678, ctx)):
        j.match(seed, ctx=c)
        torch.cuda.synchronize()
        res, src, fil = j.answer()
        want = expected_direct(new, [s0, s1])
        assert (src, fil) == want == ([1, 1, 0, 1], [1, 0, 1, 2])
        assert res == [gpu._n.CIR_FILES_OK, 4, sum(e[3] for e in entries), 4]
    # the verify reads another pool digest array than the folds were computed from: one
    # byte of a candidate's block differs -> COLLISION, and nothing else
    other = j.pdig.t[:j.pdig.n].clone()
    blk_c = 2          # s0: zz has blocks 0-1, c has 2..67
    other[32 * (blk_c + 40) + 7] ^= 1
    j.match(5, verify=other.data_ptr())
    torch.cuda.synchronize()
    res, _, _ = j.answer()
    assert res[0] == gpu._n.CIR_FILES_COLLISION and res[3] == 4
    # a differing digest that no candidate holds is no collision
    other = j.pdig.t[:j.pdig.n].clone()
    other[32 * 0 + 3] ^= 1          # block 0 of s0's zz
    j.match(6, verify=other.data_ptr())
    torch.cuda.synchronize()
    res, src, fil = j.answer()
    assert res[0] == gpu._n.CIR_FILES_OK and (src, fil) == want


def test_match_files_dev_garbage_records_do_not_fault(gpu):
    """Records that do not describe the arrays -- offsets past the arena,
    `first` past the block counts, unsorted tables -- give some answer; the
    guards behind every output stay intact."""
    import torch
    rng = random.Random(71)
    entries = [f(rng, b"f%d" % i, rng.choice((0, 1, 3, 70))) for i in range(40)]
    new = emit(entries)
    j = DevJoin(gpu, new, [new, new])
    j.upload()
    j.parse()
    torch.cuda.synchronize()
    g = torch.Generator(device="cpu").manual_seed(5)
    for side in (j.nrec, j.prec):
        junk = torch.randint(0, 1 << 62, (side.n // 8,), dtype=torch.int64, generator=g)
        junk[::3] = -1
        junk[1::5] = torch.randint(0, 5000, (len(junk[1::5]),), dtype=torch.int64, generator=g)
        side.t[:side.n].copy_(junk.view(torch.uint8))
    j.match(9)
    torch.cuda.synchronize()
    res, src, fil = j.answer()
    assert res[3] == 40 and res[0] in (0, 1)


def test_stream_order(gpu):
    """The three *_dev calls on a side stream behind a long kernel: the arena
    is written on that stream behind the delay, the outputs are read back on
    that stream, and only that stream is synchronised."""
    import torch
    lib = gpu._n.lib
    rng = random.Random(72)
    entries = [f(rng, b"f%03d" % i, rng.choice((0, 1, 2, 40))) for i in range(300)]
    new = emit(entries)
    src = emit([e if i % 3 else f(rng, e[1], 2) for i, e in enumerate(entries)])
    want = expected_direct(new, [src])
    j = DevJoin(gpu, new, [src])
    dlen = 24 << 20
    dbuf = torch.zeros(dlen, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(1, dtype=torch.int64, device="cuda")
    dl = torch.full((1,), dlen, dtype=torch.int32, device="cuda")
    dout = torch.zeros(32, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def calls():
        j.upload()
        j.parse(stream=s.cuda_stream)
        j.match(77, stream=s.cuda_stream)
    with torch.cuda.stream(s):      # warm: the kernels are loaded before the timed sequence
        calls()
    gpu._n.check(lib.cir_hash_blocks_dev(None, dbuf.data_ptr(), doff.data_ptr(), dl.data_ptr(), 1,
                                         dout.data_ptr(), s.cuda_stream))
    torch.cuda.synchronize()
    j.scratch = []
    j.arena.fill_(POISON)
    for o in j.outputs():
        o.t.fill_(POISON)
    torch.cuda.synchronize()
    outs = [j.csrc, j.cfile, j.res]
    pins = [torch.zeros(o.n + GUARD, dtype=torch.uint8).pin_memory() for o in outs]
    gpu._n.check(lib.cir_hash_blocks_dev(None, dbuf.data_ptr(), doff.data_ptr(), dl.data_ptr(), 1,
                                         dout.data_ptr(), s.cuda_stream))
    marker = torch.cuda.Event()
    marker.record(s)
    with torch.cuda.stream(s):
        calls()
        pending = not marker.query()
        for o, p in zip(outs, pins):
            p.copy_(o.t, non_blocking=True)
    s.synchronize()
    try:
        assert pending, "delay too short: nothing was tested"
        res = [int(v) for v in pins[2][:32].numpy().view(np.uint64)]
        assert res[0] == 0 and res[1] == sum(1 for v in want[0] if v != NOSRC) and res[3] == 300
        assert [int(v) for v in pins[0][:4 * 300].numpy().view(np.uint32)] == want[0]
        assert [int(v) for v in pins[1][:8 * 300].numpy().view(np.uint64)] == want[1]
        for o, p in zip(outs, pins):
            assert (p[o.n:].numpy() == POISON).all()
    finally:
        torch.cuda.synchronize()


# ---- the CLI -----------------------------------------------------------------------------

def test_cli_candidates_and_links(gpu, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    rng = random.Random(80)
    bs = 4096
    datas = {b"one": rng.randbytes(10000), b"two": rng.randbytes(4096), b"zero": b"",
             b"sp ace": rng.randbytes(5)}
    roots = []
    for k in range(3):      # new, old0 (one file differs), old1 (the same as new)
        root = tmp_path / ("r%d" % k)
        (root / "sub").mkdir(parents=True)
        for name, data in datas.items():
            if k == 1 and name == b"one":
                data = data[:-1] + b"\x00"
            where = root / "sub" if name == b"two" else root
            (where / os.fsdecode(name)).write_bytes(data)
            os.chmod(where / os.fsdecode(name), 0o644)
        roots.append(root)
    idx = [dirsig_oracle.scan(str(r), bs) for r in roots]
    paths = []
    for k, data in enumerate(idx):
        p = tmp_path / ("i%d.ds1" % k)
        p.write_bytes(data)
        paths.append(str(p))
    want, _ = links_restate.expected_candidates(idx[0], idx[1:])
    files = links_restate.file_entries(idx[0])
    assert len(want) == 4 and {s for _, s in want} == {0, 1}
    outs = []
    for extra in ([], ["--host"]):
        p = subprocess.run([cli, "candidates"] + paths + extra, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        assert (b"matched on the host" if extra else b"matched on the device") in p.stderr
        outs.append(p.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].split(b"\n")[:-1]
    assert [tuple(int(x) for x in l.split(b" ")[:2]) for l in lines] == want
    for l, (fi, _) in zip(lines, want):
        assert links_restate.unescape(l.split(b" ", 2)[2]) == files[fi][0]
    outs = []
    for extra in ([], ["--host"]):
        args = [cli, "links", paths[0]] + ["%s=%s" % (roots[k], paths[k]) for k in (1, 2)] + extra
        p = subprocess.run(args, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append((p.stdout, p.stderr.split(b"\n")[-2]))
    assert outs[0] == outs[1]
    assert len(outs[0][0].split(b"\n")) == 5 and b"4 candidates: 4 ok" in outs[0][1]
