"""cir_index_digests_dev and cir_index_digests with a context on the GPU, and
cir_block_sources through them.

The kernels (ciruela_amd/csrc/idxscan.hip): index text in, a flat digest list
and a run record {first, size, file, hash_off} per non-empty file out, or
"declined" for a text outside the canonical form (ciruela_amd/csrc/
idxscan.hpp), which then takes the host parser.  Every device call here
pre-fills the digests, the runs, the scratch and the result words with 0xA5 and
keeps a guard region behind cap_blocks digests, cap_runs records, work_bytes of
scratch and the five result words; the guards must come back untouched.

Expected values are dirsig_oracle.parse's (tests/index_cases.py) and the ctx =
NULL host path's, never the device path's own.  Indexes are dirsig_oracle.emit's
over random digests, so no file is hashed.  T below is the tile of the count and
emit passes (cir_debug_index_tile_bytes): the shapes put line starts, heads and
tokens across its boundaries and across the 16-byte spans of the lanes.

Reference: every consumer parses the text on a host thread
(ThreadedBlockReader::register_dir, src/blocks.rs:150-183; scan_links,
src/daemon/metadata/hardlink_sources.rs:107-153).
"""
import ctypes
import random

import numpy as np
import pytest

import dirsig_oracle
import index_cases
import sources_cases
import sources_restate

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
POISON = 0xA5
GUARD = 256          # bytes behind every output
OK, CAPACITY, DECLINED = 0, 1, 2
FOOT = b"ab" * 32 + b"\n"
BS = 64


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


def run_dev(gpu, index, cap_blocks=None, cap_runs=None, body=None, bs=None, ctx=None):
    """One cir_index_digests_dev call on the default stream with poisoned,
    guarded outputs; synchronises.  Returns (res[5], digests (n, 32), runs (n,
    4)): the arrays up to the counts when the status is OK, else None."""
    import torch
    lib = gpu._n.lib
    if body is None:
        _, bs, b0, b1 = frame(gpu, index)
    else:
        b0, b1 = body
    n = len(index)
    cap_blocks = n // 65 if cap_blocks is None else cap_blocks
    cap_runs = n // 73 if cap_runs is None else cap_runs
    text = torch.from_numpy(np.frombuffer(index, dtype=np.uint8).copy()).cuda()
    wb = lib.cir_index_work_bytes(n)
    dg, rn = Poisoned(torch, 32 * cap_blocks), Poisoned(torch, 32 * cap_runs)
    work, res = Poisoned(torch, wb), Poisoned(torch, 40)
    torch.cuda.synchronize()
    args = (text.data_ptr(), n, b0, b1, bs, dg.ptr, cap_blocks, rn.ptr, cap_runs, work.ptr, wb,
            res.ptr, 0)
    if ctx is not None:
        ctx.index_digests_dev(*args[:-1], stream=0)
    else:
        gpu._n.check(lib.cir_index_digests_dev(None, *args))
    torch.cuda.synchronize()
    for o in (dg, rn, work, res):
        assert o.guard_intact()
    r = [int(v) for v in res.host().view(np.uint64)]
    if r[0] != OK:
        if r[0] == CAPACITY:     # neither array is written
            assert (dg.host() == POISON).all() and (rn.host() == POISON).all()
        return r, None, None
    assert r[3] <= cap_blocks and r[2] <= cap_runs
    d = dg.host().reshape(-1, 32)
    q = rn.host().view(np.uint64).reshape(-1, 4)
    assert (d[r[3]:] == POISON).all() and (q[r[2]:] == 0xA5A5A5A5A5A5A5A5).all()
    return r, d[:r[3]].copy(), q[:r[2]].copy()


def check_ok(gpu, index, exp=None, **kw):
    """The device takes `index` and gives the oracle's arrays."""
    exp = index_cases.expected(index) if exp is None else exp
    r, d, q = run_dev(gpu, index, **kw)
    assert r[0] == OK and r[4] == U64, r
    assert r[1:4] == [exp[4], len(exp[3]), len(exp[2])], r
    assert d.shape == exp[2].shape and (d == exp[2]).all()
    assert q.shape == exp[3].shape and (q == exp[3]).all()
    return r


@pytest.fixture(scope="module")
def T(gpu):
    return int(gpu._n.lib.cir_debug_index_tile_bytes())


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=gpu._n.CIR_STAGING_LAZY)


def header(extra=0, bs=BS):
    """A header line of a chosen length (trailing spaces are the parser's to skip)."""
    return b"DIRSIGNATURE.v1 blake2b/256 block_size=%d" % bs + b" " * extra + b"\n"


def pad_to(text, offset):
    """`text` plus directory lines up to exactly `offset` bytes."""
    out = [text]
    left = offset - len(text)
    assert left == 0 or left >= 2
    while left:
        n = left if left <= 2000 else (1000 if left < 2002 else 2000)
        if left - n == 1:
            n -= 1
        out.append(b"/" + b"p" * (n - 2) + b"\n")
        left -= n
    return b"".join(out)


def file_line(rng, name, size, bs=BS):
    toks = b"".join(b" " + rng.randbytes(32).hex().encode()
                    for _ in range(index_cases.nblocks(size, bs)))
    return b"  " + name + b" f %d" % size + toks + b"\n"


def with_line_at(rng, line, offset, extra=0):
    """An index whose entry line `line` starts at byte `offset`."""
    head = pad_to(header(extra) + b"/\n", offset)
    return head + line + b"  z f 0\n/after\n" + file_line(rng, b"t", BS + 1) + FOOT


# ---- small texts -----------------------------------------------------------------------

def test_small_texts(gpu, ctx):
    rng = random.Random(1)
    r = check_ok(gpu, header() + FOOT)                       # header and footer only
    assert r[1:4] == [0, 0, 0]
    check_ok(gpu, header() + b"/\n  e f 0\n" + FOOT, ctx=ctx)  # one directory, one empty file
    r = check_ok(gpu, header() + b"/\n" + file_line(rng, b"one", 10) + FOOT)
    assert r[1:4] == [1, 1, 1]
    # a body handed over without a frame: empty at offset 0, and the whole text
    r, _, _ = run_dev(gpu, b"/\n", body=(0, 0), bs=BS)
    assert r == [OK, 0, 0, 0, U64]
    r, _, _ = run_dev(gpu, b"/\n  e f 0\n", body=(0, 10), bs=BS)
    assert r == [OK, 1, 0, 0, U64]


# ---- tile boundaries -------------------------------------------------------------------

@pytest.mark.parametrize("where", ["nl_last_of_tile", "nl_first_of_next", "head_straddles",
                                   "token_straddles", "dir_straddles"])
def test_lines_across_a_tile_boundary(gpu, T, where):
    rng = random.Random(2)
    line = file_line(rng, b"name\\x20x", 3 * BS)
    at = {"nl_last_of_tile": 2 * T, "nl_first_of_next": 2 * T + 1, "head_straddles": 2 * T - 7,
          "token_straddles": 2 * T - 100, "dir_straddles": 2 * T - 3}[where]
    if where == "dir_straddles":
        line = b"/dir/that/straddles\n" + line
    index = with_line_at(rng, line, at)
    assert index[at - 1:at] == b"\n"
    check_ok(gpu, index)


@pytest.mark.parametrize("mod", [0, 1, 15])
def test_body_offset_modulo_the_span(gpu, mod):
    rng = random.Random(3)
    extra = (mod - len(header())) % 16
    index = header(extra) + b"/\n" + file_line(rng, b"f", 2 * BS) + b"  l s t\n" + FOOT
    assert frame(gpu, index)[2] % 16 == mod
    check_ok(gpu, index)
    # and a first line that is no directory line is declined at body_off itself
    bad = header(extra) + file_line(rng, b"f", 2 * BS) + FOOT
    r, _, _ = run_dev(gpu, bad)
    assert r[0] == DECLINED and r[4] == len(header(extra))


def test_a_line_longer_than_several_tiles(gpu, T):
    """300 blocks, 19.5 KB: whole tiles hold no line start."""
    rng = random.Random(4)
    line = file_line(rng, b"big", 300 * BS - 5)
    assert len(line) > 4 * T
    index = with_line_at(rng, line, T - 33)
    r = check_ok(gpu, index)
    assert r[3] == 302


@pytest.mark.parametrize("line", [b"/\n", b"  a s b\n"])
def test_many_line_starts_in_one_span(gpu, T, line):
    """3 T bytes of the shortest lines: eight, or two, line starts per lane."""
    rng = random.Random(5)
    n = 3 * T // len(line)
    index = header() + b"/\n" + line * n + file_line(rng, b"f", 1) + b"/\n" * 9 + FOOT
    r = check_ok(gpu, index)
    assert r[1:4] == [1, 1, 1]


@pytest.mark.parametrize("nruns", [63, 64, 65, 255, 256, 257])
def test_run_counts_at_wave_and_workgroup_edges(gpu, nruns):
    rng = random.Random(nruns)
    entries = []
    for i in range(nruns):
        entries.append(index_cases.file_entry(rng, b"f%03d" % i, rng.choice((1, BS, BS + 1)), BS))
        if i % 3 == 0:
            entries.append(index_cases.file_entry(rng, b"e%03d" % i, 0, BS))
    index = index_cases.emit([(b"/", entries)], BS)
    r = check_ok(gpu, index)
    assert r[2] == nruns


def test_sizes_around_the_block_size(gpu):
    rng = random.Random(6)
    bs = 32768
    entries = [index_cases.file_entry(rng, b"s%d" % i, s, bs)
               for i, s in enumerate((bs - 1, bs, bs + 1, 2 * bs, 0, 1))]
    r = check_ok(gpu, index_cases.emit([(b"/", entries)], bs, "sha512/256"))
    assert r[1:4] == [6, 5, 7]
    entries = [index_cases.file_entry(rng, b"b", 5, 1), index_cases.file_entry(rng, b"c", 1, 1)]
    check_ok(gpu, index_cases.emit([(b"/", entries)], 1))


def test_upper_case_hex(gpu, ctx):
    rng = random.Random(7)
    first = file_line(rng, b"f", 3 * BS)
    cut = first.index(b" f 192") + 6
    rest = file_line(rng, b"g", 1) + FOOT
    lower = header() + b"/\n" + first + rest
    upper = header() + b"/\n" + first[:cut] + first[cut:].upper() + rest
    assert upper != lower and len(upper) == len(lower)
    check_ok(gpu, upper, exp=index_cases.expected(lower))
    res = gpu.index_digests(upper, ctx)
    assert res.stats["on_device"] == 1 and index_cases.same(res, index_cases.expected(lower))


# ---- declines --------------------------------------------------------------------------

def host_outcome(gpu, index, ctx=None):
    try:
        return gpu.index_digests(index, ctx)
    except gpu.CiruelaError as e:
        return e.status


def same_outcome(a, b):
    if isinstance(a, int) or isinstance(b, int):
        return a == b
    return (a.hash_type == b.hash_type and a.block_size == b.block_size and
            a.nfiles == b.nfiles and np.array_equal(a.digests, b.digests) and
            np.array_equal(a.runs, b.runs))


def check_declined(gpu, ctx, index, line_start):
    """The device declines `index` at line_start, and cir_index_digests with a
    context returns exactly what ctx = NULL returns, saying that it fell back."""
    r, _, _ = run_dev(gpu, index)
    assert r[0] == DECLINED and r[4] == line_start, (r, line_start)
    host = host_outcome(gpu, index)
    dev = host_outcome(gpu, index, ctx)
    assert same_outcome(dev, host)
    if not isinstance(dev, int):
        assert dev.stats["on_device"] == 0 and dev.stats["fell_back"] == 1
        assert dev.stats["declined_at"] == line_start
        assert dev.stats["uploaded_bytes"] == len(index)
    return host


DECLINES = {
    "double_space": (b"  a  f 0\n", "ok"),
    "trailing_space": (b"  a f 0 \n", "ok"),
    "raw_tab": (b"  a\tb f 0\n", "ok"),
    "escaped_dot": (b"  a\\x2eb f 0\n", "ok"),
    "escaped_dot_name": (b"  \\x2e\\x2e f 0\n", "error"),
    "crlf": (b"  a f 0\r\n", "error"),
    "unknown_type": (b"  a q 0\n", "error"),
    "space_in_dir": (b"/a b\n", "ok"),
    "empty_line": (b"\n", "error"),
}


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_declined_lines(gpu, ctx, T, name):
    rng = random.Random(8)
    line, outcome = DECLINES[name]
    at = T + 5
    index = pad_to(header() + b"/\n" + file_line(rng, b"f", 70), at) + line + \
        file_line(rng, b"g", 1) + FOOT
    host = check_declined(gpu, ctx, index, at)
    assert isinstance(host, int) == (outcome == "error")
    if outcome == "error":
        assert host == gpu._n.CIR_EPARSE


def test_bad_tokens(gpu, ctx, T):
    rng = random.Random(9)
    line = file_line(rng, b"big", 300 * BS)
    at = T - 33
    good = with_line_at(rng, line, at)
    mid = at + len(b"  big f 19200") + 65 * 150 + 30      # inside the middle token
    bad = good[:mid] + b"g" + good[mid + 1:]
    assert check_declined(gpu, ctx, bad, at) == gpu._n.CIR_EPARSE
    # a 62-digit token: the line is two bytes short of its promise -- CIR_EHASHSIZE on the host
    short = good[:mid] + good[mid + 2:]
    assert check_declined(gpu, ctx, short, at) == gpu._n.CIR_EHASHSIZE
    # a separator that is no space, in the last token
    sep = at + len(b"  big f 19200") + 65 * 299
    assert good[sep:sep + 1] == b" "
    assert check_declined(gpu, ctx, good[:sep] + b"_" + good[sep + 1:], at) == gpu._n.CIR_EPARSE
    # two bad lines: the earlier one's start is reported, whichever pass finds them
    after = good.index(b"  t f 65")
    tok2 = after + len(b"  t f 65") + 65 + 7
    two = bad[:tok2] + b"!" + bad[tok2 + 1:]
    check_declined(gpu, ctx, two, at)
    head_bad = good.replace(b"  z f 0\n", b"  z  f 0\n")
    both = head_bad[:tok2 + 1] + b"!" + head_bad[tok2 + 2:]
    check_declined(gpu, ctx, both, good.index(b"  z f 0\n"))


# ---- capacity --------------------------------------------------------------------------

def test_capacity(gpu):
    rng = random.Random(10)
    entries = [index_cases.file_entry(rng, b"f%d" % i, s, BS)
               for i, s in enumerate((1, 0, 3 * BS, 2 * BS + 1, 70 * BS))]
    index = index_cases.emit([(b"/", entries)], BS)
    exp = index_cases.expected(index)
    nblk, nruns = len(exp[2]), len(exp[3])
    check_ok(gpu, index, exp=exp, cap_blocks=nblk, cap_runs=nruns)     # exactly enough
    for kw in (dict(cap_blocks=nblk - 1, cap_runs=nruns), dict(cap_blocks=nblk, cap_runs=nruns - 1),
               dict(cap_blocks=0, cap_runs=0)):
        r, _, _ = run_dev(gpu, index, **kw)
        assert r == [CAPACITY, 5, nruns, nblk, U64], (kw, r)


# ---- random sweep ----------------------------------------------------------------------

def test_random_sweep(gpu, ctx):
    """200 seeded random small indexes and one mutation of each: the context
    path equals the host path on every one (arrays or error code), and the
    unmutated ones equal the oracle on the device."""
    taken = fell = 0
    for seed in range(200):
        index = index_cases.random_index(5000 + seed)
        exp = index_cases.expected(index)
        res = gpu.index_digests(index, ctx)
        assert index_cases.same(res, exp), seed
        assert res.stats["on_device"] == 1 and res.stats["fell_back"] == 0, seed
        if seed % 10 == 0:
            check_ok(gpu, index, exp=exp)          # (the guarded call: a tenth of them)
        mut = index_cases.mutate(index, seed)
        host, dev = host_outcome(gpu, mut), host_outcome(gpu, mut, ctx)
        assert same_outcome(dev, host), seed
        if not isinstance(dev, int):
            taken += dev.stats["on_device"]
            fell += dev.stats["fell_back"]
    assert taken and fell


# ---- the largest case ------------------------------------------------------------------

def test_largest_case(gpu, ctx):
    """About 32 MB of text, 500,000 blocks in 1,000 files, every digest compared."""
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, size=(500000, 32), dtype=np.uint8)
    hexed = raw.tobytes().hex().encode()
    lines, runs, pos = [header(0, 4096) + b"/\n"], [], 0
    pos = len(lines[0])
    for f in range(1000):
        head = b"  file%04d f %d" % (f, 500 * 4096 - f)
        toks = b"".join(b" " + hexed[64 * b:64 * b + 64] for b in range(500 * f, 500 * f + 500))
        runs.append((500 * f, 500 * 4096 - f, f, pos + len(head)))
        lines.append(head + toks + b"\n")
        pos += len(head) + len(toks) + 1
    index = b"".join(lines) + FOOT
    assert 32000000 < len(index) < 34000000
    exp = (1, 4096, raw, np.array(runs, dtype=np.uint64), 1000)
    check_ok(gpu, index, exp=exp)
    res = gpu.index_digests(index, ctx)
    assert res.stats["on_device"] == 1 and index_cases.same(res, exp)


# ---- stream order ----------------------------------------------------------------------

def test_stream_order(gpu):
    """The call on a side stream behind a long kernel: the text is written on
    that stream behind the delay, the outputs are read back on that stream,
    and only that stream is synchronised.  A kernel on another stream, or a
    hidden synchronise, shows as garbage or as a delay that has ended when the
    call returns."""
    import torch
    lib = gpu._n.lib
    rng = random.Random(12)
    entries = [index_cases.file_entry(rng, b"f%d" % i, rng.randint(0, 40 * BS), BS)
               for i in range(300)]
    index = index_cases.emit([(b"/", entries)], BS)
    exp = index_cases.expected(index)
    _, bs, b0, b1 = frame(gpu, index)
    n = len(index)
    cap_b, cap_r, wb = n // 65, n // 73, lib.cir_index_work_bytes(n)
    late = torch.from_numpy(np.frombuffer(index, dtype=np.uint8).copy()).pin_memory()
    text = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    outs = [Poisoned(torch, 32 * cap_b), Poisoned(torch, 32 * cap_r), Poisoned(torch, wb),
            Poisoned(torch, 40)]
    pins = [torch.zeros(o.n + GUARD, dtype=torch.uint8).pin_memory() for o in outs]
    # the delay: one BLAKE2b chain on one lane (cir_hash_blocks_dev, NULL context: one launch)
    dlen = 24 << 20
    dbuf = torch.zeros(dlen, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(1, dtype=torch.int64, device="cuda")
    dl = torch.full((1,), dlen, dtype=torch.int32, device="cuda")
    dout = torch.zeros(32, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def call():
        gpu._n.check(lib.cir_index_digests_dev(None, text.data_ptr(), n, b0, b1, bs, outs[0].ptr,
                                               cap_b, outs[1].ptr, cap_r, outs[2].ptr, wb,
                                               outs[3].ptr, s.cuda_stream))
    with torch.cuda.stream(s):      # warm: the kernels are loaded before the timed sequence
        text.copy_(late, non_blocking=True)
        call()
    gpu._n.check(lib.cir_hash_blocks_dev(None, dbuf.data_ptr(), doff.data_ptr(), dl.data_ptr(), 1,
                                         dout.data_ptr(), s.cuda_stream))
    torch.cuda.synchronize()
    text.fill_(POISON)
    for o in outs:
        o.t.fill_(POISON)
    torch.cuda.synchronize()
    dl.fill_(dlen)
    torch.cuda.synchronize()
    gpu._n.check(lib.cir_hash_blocks_dev(None, dbuf.data_ptr(), doff.data_ptr(), dl.data_ptr(), 1,
                                         dout.data_ptr(), s.cuda_stream))
    marker = torch.cuda.Event()
    marker.record(s)
    with torch.cuda.stream(s):
        text.copy_(late, non_blocking=True)
        call()
        pending = not marker.query()
        for o, p in zip(outs, pins):
            p.copy_(o.t, non_blocking=True)
    s.synchronize()
    try:
        assert pending, "delay too short: nothing was tested"
        r = [int(v) for v in pins[3][:40].numpy().view(np.uint64)]
        assert r == [OK, exp[4], len(exp[3]), len(exp[2]), U64]
        d = pins[0][:32 * r[3]].numpy().reshape(-1, 32)
        q = pins[1][:32 * r[2]].numpy().view(np.uint64).reshape(-1, 4)
        assert (d == exp[2]).all() and (q == exp[3]).all()
        for o, p in zip(outs, pins):
            assert (p[o.n:].numpy() == POISON).all()
    finally:
        torch.cuda.synchronize()


# ---- through cir_block_sources ---------------------------------------------------------

SOURCE_CASES = sources_cases.cases()


def same_sources(a, b):
    return ((a.src, a.file, a.block, a.nblk, a.skipped) == (b.src, b.file, b.block, b.nblk, b.skipped)
            and {k: v for k, v in a.stats.items() if k not in ("on_device", "table_slots")} ==
            {k: v for k, v in b.stats.items() if k not in ("on_device", "table_slots")})


def sources_outcome(gpu, index, sources, want=None, context=None):
    try:
        return gpu.block_sources(index, sources, want=want, context=context)
    except gpu.CiruelaError as e:
        return (e.status, e.detail)


def check_sources(gpu, ctx, index, sources, want=None):
    """With a context (the texts parsed on the device) the result, or the
    error code and text, is that of ctx = NULL."""
    dev = sources_outcome(gpu, index, sources, want, ctx)
    host = sources_outcome(gpu, index, sources, want)
    if isinstance(host, tuple):
        assert dev == host
    else:
        assert not isinstance(dev, tuple) and same_sources(dev, host)
        assert dev.stats["on_device"] == 1 and host.stats["on_device"] == 0
    return host


def test_block_sources_families(gpu, ctx):
    for name, index, sources, bits, tail in SOURCE_CASES:
        want = None if bits is None else sources_restate.want_words(bits, tail_ones=tail)
        host = check_sources(gpu, ctx, index, sources, want)
        assert sources_restate.same(host, sources_restate.expected(index, sources, bits)), name


def test_block_sources_with_declined_texts(gpu, ctx):
    """A source the device declines and the host parser takes (a doubled
    space), one neither takes (a bad hex digit: found by the decode pass, after
    the pool was laid out), an upper-case source, and a declined new index --
    lenient, and unparseable: the error's code and text are the host's."""
    by = {c[0]: c for c in SOURCE_CASES}
    _, index, sources, _, _ = by["first_source_first_place"]
    s0, s1 = sources

    def lenient(text):
        at = text.index(b" f ")
        return text[:at] + b" " + text[at:]

    def bad_token(text):
        at = text.index(b" f ") + 20
        assert text[at:at + 1] in b"0123456789abcdef"
        return text[:at] + b"g" + text[at + 1:]

    def upper(text):
        body, foot = text[:-65], text[-65:]
        at = body.index(b" f ") + 3
        return body[:at] + body[at:].replace(b"a", b"A").replace(b"e", b"E") + foot
    assert upper(s1) != s1
    host = check_sources(gpu, ctx, index, [lenient(s0), s1])
    assert host.skipped == 0 and host.src == sources_restate.expected(index, sources)[0]
    host = check_sources(gpu, ctx, index, [bad_token(s0), s1, lenient(s0)])
    assert host.skipped == 1 and set(host.src) <= {1, 2}
    host = check_sources(gpu, ctx, index, [upper(s1), bad_token(s1), s0])
    assert host.skipped == 1 and set(host.src) == {0}
    host = check_sources(gpu, ctx, lenient(index), [s0, bad_token(s0), s1])
    assert host.src == [2 if v == 1 else v for v in sources_restate.expected(index, sources)[0]]
    for broken in (bad_token(index), index.replace(b" f ", b" q ", 1), index[:-1],
                   index.replace(b"DIRSIGNATURE.v1", b"DIRSIGNATURE.v9")):
        host = check_sources(gpu, ctx, broken, [s0, s1])
        assert isinstance(host, tuple) and host[0] == gpu._n.CIR_EPARSE
    cut = index.index(b" f ") + 10
    short = index[:cut] + index[cut + 2:]
    host = check_sources(gpu, ctx, short, [s0, s1])
    assert isinstance(host, tuple) and host[0] == gpu._n.CIR_EHASHSIZE


def test_block_sources_when_the_count_pass_alone_would_end_the_call(gpu, ctx):
    """A new index without blocks ends the call before any join, so before
    the decode pass has looked at a source's tokens: a source with a bad token
    must still be skipped and left out of the stats, as on the host."""
    by = {c[0]: c for c in SOURCE_CASES}
    _, empty, _, _, _ = by["no_blocks"]
    _, _, (s0, s1), _, _ = by["first_source_first_place"]
    at = s0.index(b" f ") + 20
    bad = s0[:at] + b"g" + s0[at + 1:]
    sep = s1.index(b" f ") + 7 + 64
    assert s1[sep:sep + 1] == b" "
    bad_sep = s1[:sep] + b"_" + s1[sep + 1:]
    for sources, skipped in (([bad, s1], 1), ([s0, bad_sep, bad], 2), ([s0, s1], 0), ([bad], 1)):
        host = check_sources(gpu, ctx, empty, sources)
        assert (host.nblk, host.skipped) == (0, skipped)
        assert host.stats["sources_used"] == len(sources) - skipped
    want = sources_restate.expected(empty, [s1])[3]["pool_blocks"]
    assert check_sources(gpu, ctx, empty, [bad, s1]).stats["pool_blocks"] == want


_TRACED_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/oracle"]
import ciruela_amd as ca
import sources_cases
_, index, sources, _, _ = next(c for c in sources_cases.cases() if c[0] == "skipped_sources")
ctx = ca.Context(device_mask=1, staging_bytes=ca._n.CIR_STAGING_LAZY)
r = ca.block_sources(index, sources, context=ctx)
print(r.found, r.skipped)
"""


def test_block_sources_parses_on_the_device_unless_told_otherwise(gpu):
    """The CIR_TRACE=1 line of a child process names the device parse and its
    laps; under CIR_SOURCES_PARSE=host it is the old line, with the same
    result."""
    import os
    import subprocess
    import sys

    from conftest import ROOT
    outs = {}
    for mode in ("", "host"):
        env = dict(os.environ, CIR_TRACE="1", CIR_SOURCES_PARSE=mode)
        p = subprocess.run([sys.executable, "-c", _TRACED_CHILD, ROOT], env=env,
                           capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("cir block_sources:")]
        assert len(line) == 1
        outs[mode] = (p.stdout, line[0])
    assert outs[""][0] == outs["host"][0] == b"3 5\n"
    assert "device parse of 4 text(s)" in outs[""][1] and "decode kernels" in outs[""][1]
    assert "device parse" not in outs["host"][1] and ", device;" in outs["host"][1]
