"""cir_match_copies_dev and cir_file_copies with a context on the GPU.

The kernels (ciruela_amd/csrc/files.hip: k_files_fold, k_copies_build,
k_copies_probe, k_files_verify) join two file lists by content: per need file
that is neither empty nor skipped, the pool file of the smallest ordinal with
equal exe flag, size and digests, at any path.  Expected values are
copies_restate's (the rule in plain Python) and, for the whole call, the host
rule's as well; never the device path's own.  The direct calls run on records
and digests built with numpy, no text; the whole call on the families and the
random cases of tests/copies_cases.py.

Every canonical case must be answered by the device (stats on_device == 1,
why_host == 0): a silent fall-back would hide a kernel bug behind the host's
correct answer.  Device calls made directly keep 0xA5-filled guard regions
behind their outputs, which must come back untouched.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import copies_cases
import copies_restate
import dirsig_oracle
import links_restate

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
POISON = 0xA5
GUARD = 256
EXE = 1 << 63
NOSRC = (1 << 32) - 1
BS = 64


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=gpu._n.CIR_STAGING_LAZY)


class Poisoned:
    """nbytes of device memory filled with 0xA5 and GUARD more behind them."""

    def __init__(self, torch, nbytes):
        self.n = nbytes
        self.t = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def guard_intact(self):
        return bool((self.t[self.n:] == POISON).all().item())

    def host(self):
        return self.t[:self.n].cpu().numpy()


# ---- synthetic sides -----------------------------------------------------------------------

class Universe:
    """Contents by number: content c of n blocks is a fixed list of n random
    digests; (c, n) with another n is another content."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.known = {}

    def digests(self, c, n):
        if (c, n) not in self.known:
            self.known[(c, n)] = self.rng.integers(0, 256, (n, 32), dtype=np.uint8)
        return self.known[(c, n)]


def side(uni, files, off0):
    """files: [(content number, blocks, exe, bytes missing from the last
    block)].  Returns (records (n, 4) u64, digests (nblk, 32) u8); the two
    offsets of record j are off0 + 2 j and off0 + 2 j + 1."""
    recs, digs, blk = [], [], 0
    for j, (c, n, exe, short) in enumerate(files):
        size = n * BS - (short if n else 0)
        recs.append((off0 + 2 * j, off0 + 2 * j + 1, size, blk | (EXE if exe else 0)))
        if n:
            digs.append(uni.digests(c, n))
        blk += n
    recs = np.array(recs, dtype=np.uint64).reshape(-1, 4)
    digs = np.concatenate(digs) if digs else np.zeros((0, 32), dtype=np.uint8)
    return recs, digs


class Join:
    """One cir_match_copies_dev problem on the device, outputs poisoned and
    guarded."""

    def __init__(self, gpu, need, pools, skip=None):
        import torch
        self.gpu, self.torch = gpu, torch
        self.nrec_h, self.ndig_h = need
        # a source's `first` counts into the pool's flat digest list
        blk, fixed = 0, []
        for recs, digs in pools:
            r = recs.copy()
            r[:, 3] += np.uint64(blk)
            fixed.append(r)
            blk += len(digs)
        self.prec_h = np.concatenate(fixed) if fixed else np.zeros((0, 4), np.uint64)
        self.pdig_h = np.concatenate([p[1] for p in pools]) if pools else np.zeros((0, 32), np.uint8)
        self.first_h = np.cumsum([0] + [len(p[0]) for p in pools]).astype(np.uint64)
        self.nsrc = len(pools)
        self.skip = sorted(skip or ())
        self.nf, self.nb = len(self.nrec_h), len(self.ndig_h)
        self.pf, self.pb = len(self.prec_h), len(self.pdig_h)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        pad = lambda a: np.concatenate([a.reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])
        self.nrec, self.prec = up(pad(self.nrec_h)), up(pad(self.prec_h))
        self.ndig, self.pdig = up(pad(self.ndig_h)), up(pad(self.pdig_h))
        self.first = up(self.first_h)
        self.dskip = None
        if skip is not None:
            words = np.zeros((self.nf + 63) // 64 + 1, dtype=np.uint64)
            for i in self.skip:
                words[i >> 6] |= np.uint64(1 << (i & 63))
            self.dskip = up(words)
        self.wb = gpu._n.lib.cir_match_copies_work_bytes(self.nf, self.pf)
        assert self.wb == 16 * (self.nf + self.pf) + 4 * gpu._n.lib.cir_match_table_slots(self.pf)
        P = lambda n: Poisoned(torch, n)
        self.work, self.csrc, self.cfile = P(self.wb), P(4 * self.nf), P(8 * self.nf)
        self.cplace, self.res = P(16 * self.nf), P(32)

    def outputs(self):
        return [self.work, self.csrc, self.cfile, self.cplace, self.res]

    def match(self, seed, verify=0, stream=0, ctx=None):
        need = (self.nrec.data_ptr(), self.nf, self.ndig.data_ptr(), self.nb)
        pool = (self.prec.data_ptr(), self.pf, self.pdig.data_ptr(), self.pb)
        skip = self.dskip.data_ptr() if self.dskip is not None else 0
        if ctx is not None:
            ctx.match_copies_dev(need, pool, self.first.data_ptr(), self.nsrc, BS, seed,
                                 self.work.ptr, self.wb, self.csrc.ptr, self.cfile.ptr,
                                 self.cplace.ptr, self.res.ptr, d_skip=skip, d_pool_verify=verify,
                                 stream=stream)
        else:
            self.gpu._n.check(self.gpu._n.lib.cir_match_copies_dev(
                None, *need, *pool, self.first.data_ptr(), self.nsrc, BS, skip, verify, seed,
                self.work.ptr, self.wb, self.csrc.ptr, self.cfile.ptr, self.cplace.ptr,
                self.res.ptr, stream))

    def want(self):
        return copies_restate.expected_from_records(
            self.nrec_h, self.ndig_h, self.prec_h, self.pdig_h, [int(v) for v in self.first_h], BS,
            self.skip)

    def decode(self, csrc, cfile, cplace, res):
        """The outputs as the restatement spells them, and res."""
        got = []
        for i in range(self.nf):
            if csrc[i] == NOSRC:
                assert cfile[i] == U64 and cplace[2 * i] == U64 and cplace[2 * i + 1] == U64
                got.append(None)
            else:
                got.append((int(csrc[i]), int(cfile[i]), int(cplace[2 * i]), int(cplace[2 * i + 1])))
        return got, [int(v) for v in res]

    def answer(self):
        for o in self.outputs():
            assert o.guard_intact()
        return self.decode(self.csrc.host().view(np.uint32), self.cfile.host().view(np.uint64),
                           self.cplace.host().view(np.uint64), self.res.host().view(np.uint64))

    def check(self, seeds=(1,), ctx=None):
        want = self.want()
        hits = [i for i, w in enumerate(want) if w is not None]
        for seed in seeds:
            for o in self.outputs():
                o.t.fill_(POISON)
            self.match(seed, ctx=ctx)
            self.torch.cuda.synchronize()
            got, res = self.answer()
            assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
            assert res == [0, len(hits), sum(int(self.nrec_h[i][2]) for i in hits), self.nf], res
        return want


def need_files(rng, n, ncontents):
    return [(rng.randrange(ncontents), rng.choice((0, 1, 1, 2, 70)), rng.random() < 0.2,
             rng.choice((0, 0, 5))) for _ in range(n)]


# ---- cir_match_copies_dev ------------------------------------------------------------------

@pytest.mark.parametrize("nneed", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("per_source,nsrc", [(0, 1), (1, 1), (200, 1), (0, 3), (1, 3), (200, 3)])
def test_shapes(gpu, ctx, nneed, per_source, nsrc):
    """Need files on both sides of a wave and of two, pools of 0, 1 and 200
    files per source, files of 0, 1, 2 and 70 blocks (a file's blocks cross a
    wave in the fold), over 12 contents, so that most need files have several
    equal pool files in several sources."""
    rng = random.Random(1000 * nneed + 10 * per_source + nsrc)
    uni = Universe(nneed)
    need = side(uni, need_files(rng, nneed, 12), 1 << 20)
    pools = [side(uni, need_files(rng, per_source, 12), (k + 1) << 24) for k in range(nsrc)]
    j = Join(gpu, need, pools)
    want = j.check(seeds=(1, 0xDEADBEEF12345678, U64), ctx=ctx if nneed == 64 else None)
    if per_source == 200 and nneed >= 63:
        assert sum(w is not None for w in want) > nneed // 3
        assert sum(w is not None and w[0] == 0 for w in want) > 0


def test_every_pool_file_of_one_content(gpu):
    """300 pool files of one content: every lane of the build meets one slot,
    and it ends holding ordinal 0 -- unless file 0 is the one with another exe
    flag."""
    uni = Universe(2)
    need = side(uni, [(0, 3, False, 0), (0, 3, True, 0), (1, 3, False, 0)], 64)
    j = Join(gpu, need, [side(uni, [(0, 3, False, 0)] * 300, 4096)])
    want = j.check(seeds=(3, 4, 5))
    assert want == [(0, 0, 4096, 4097), None, None]
    j = Join(gpu, need, [side(uni, [(0, 3, True, 0)] + [(0, 3, False, 0)] * 299, 4096)])
    assert j.check(seeds=(3, 4, 5)) == [(0, 1, 4098, 4099), (0, 0, 4096, 4097), None]


def test_many_duplicates_beside_distinct_files(gpu):
    """2,000 pool files of 40 contents and 2,000 distinct ones, in two sources;
    every need content's candidate is its first holder."""
    rng = random.Random(3)
    uni = Universe(3)
    files = [(rng.randrange(40), 2, False, 0) for _ in range(2000)] + \
        [(1000 + i, 1 + i % 3, i % 5 == 0, 0) for i in range(2000)]
    rng.shuffle(files)
    pools = [side(uni, files[:1500], 1 << 20), side(uni, files[1500:], 1 << 24)]
    need = side(uni, [(c, 2, False, 0) for c in range(45)] +
                [(1000 + i, 1 + i % 3, i % 5 == 0, 0) for i in range(0, 2000, 7)] +
                [(1000 + i, 1 + i % 3, i % 5 != 0, 0) for i in range(0, 2000, 97)], 64)
    j = Join(gpu, need, pools)
    want = j.check(seeds=(7, 8, 9))
    assert sum(w is not None for w in want[:45]) == 40
    assert {w[0] for w in want if w is not None} == {0, 1}


def test_skip_bits(gpu, ctx):
    rng = random.Random(4)
    uni = Universe(4)
    files = [(i, 1 + i % 2, False, 0) for i in range(130)]
    need, pool = side(uni, files, 64), side(uni, files[::-1], 4096)
    full = Join(gpu, need, [pool], skip=()).check()       # (an all-zero bitmap)
    assert all(w is not None for w in full)
    assert Join(gpu, need, [pool]).check() == full        # (no bitmap)
    j = Join(gpu, need, [pool], skip=(0, 63, 64))
    want = j.check(seeds=(1, 2), ctx=ctx)
    assert [i for i, w in enumerate(want) if w is None] == [0, 63, 64]
    assert want[1] == (0, 128, 4096 + 2 * 128, 4096 + 2 * 128 + 1)
    every = Join(gpu, need, [pool], skip=range(130)).check()
    assert every == [None] * 130


def test_empty_sides(gpu):
    uni = Universe(5)
    some = side(uni, [(0, 2, False, 0), (1, 0, False, 0)], 64)
    none = side(uni, [], 0)
    assert Join(gpu, some, []).check() == [None, None]                  # no source
    assert Join(gpu, some, [none]).check() == [None, None]              # a source without files
    assert Join(gpu, none, [some]).check() == []                        # no need file
    assert Join(gpu, none, []).check() == []
    only_empty = side(uni, [(1, 0, False, 0), (2, 0, True, 0)], 64)
    assert Join(gpu, only_empty, [only_empty, some]).check() == [None, None]   # no block at all
    assert Join(gpu, some, [only_empty, some]).check() == [(1, 0, 64, 65), None]


def test_collision_status(gpu):
    """The verify reads another pool digest array than the folds were computed
    from.  One byte of the last block of a candidate differs: COLLISION.  One
    byte of a file that is nobody's candidate differs: OK and the same answer."""
    import torch
    uni = Universe(6)
    need = side(uni, [(0, 70, False, 3), (1, 1, False, 0)], 64)
    pool = side(uni, [(2, 2, False, 0), (0, 70, False, 3), (1, 1, False, 0), (0, 70, False, 3)], 4096)
    j = Join(gpu, need, [pool])
    want = j.check()
    assert want == [(0, 1, 4098, 4099), (0, 2, 4100, 4101)]
    other = j.pdig.clone()
    other[32 * (2 + 69) + 31] ^= 1                # the last block of pool file 1
    j.match(5, verify=other.data_ptr())
    torch.cuda.synchronize()
    _, res = j.answer()
    assert res[0] == gpu._n.CIR_FILES_COLLISION and res[3] == 2
    for blk in (0, 2 + 70 + 1 + 5):               # pool file 0; the second holder of content 0
        other = j.pdig.clone()
        other[32 * blk + 3] ^= 1
        j.match(6, verify=other.data_ptr())
        torch.cuda.synchronize()
        got, res = j.answer()
        assert res[0] == gpu._n.CIR_FILES_OK and got == want


def test_garbage_records_do_not_fault(gpu):
    """Records that do not describe the arrays give some answer; the guards
    behind every output stay intact."""
    import torch
    rng = random.Random(7)
    uni = Universe(7)
    need = side(uni, need_files(rng, 100, 8), 64)
    pools = [side(uni, need_files(rng, 150, 8), 4096) for _ in range(2)]
    j = Join(gpu, need, pools)
    g = torch.Generator(device="cpu").manual_seed(5)
    for t, n in ((j.nrec, 32 * j.nf), (j.prec, 32 * j.pf)):
        junk = torch.randint(0, 1 << 62, (n // 8,), dtype=torch.int64, generator=g)
        junk[::3] = -1
        junk[1::5] = torch.randint(0, 5000, (len(junk[1::5]),), dtype=torch.int64, generator=g)
        t[:n].copy_(junk.view(torch.uint8))
    j.first.copy_(torch.from_numpy(np.array([7, 1 << 40, 3], dtype=np.uint64).view(np.uint8)).cuda())
    j.match(9)
    torch.cuda.synchronize()
    for o in j.outputs():
        assert o.guard_intact()
    res = [int(v) for v in j.res.host().view(np.uint64)]
    assert res[3] == 100 and res[0] in (0, 1)


def test_stream_order(gpu):
    """cir_match_copies_dev on a side stream behind a long kernel: the digests
    are copied into place on that stream behind the delay, immediately before
    the call; the outputs are read back by copies on that stream; only that
    stream is synchronised before the comparison."""
    import torch
    lib = gpu._n.lib
    rng = random.Random(8)
    uni = Universe(8)
    need = side(uni, need_files(rng, 300, 30), 64)
    pools = [side(uni, need_files(rng, 400, 30), (k + 1) << 20) for k in range(2)]
    j = Join(gpu, need, pools, skip=(5, 64))
    want = j.want()
    pin = lambda a: torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(16, np.uint8)])).pin_memory()
    h_ndig, h_pdig = pin(j.ndig_h), pin(j.pdig_h)
    dlen = 24 << 20
    dbuf = torch.zeros(dlen, dtype=torch.uint8, device="cuda")
    doff = torch.zeros(1, dtype=torch.int64, device="cuda")
    dl = torch.full((1,), dlen, dtype=torch.int32, device="cuda")
    dout = torch.zeros(32, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def calls():
        j.ndig.copy_(h_ndig, non_blocking=True)
        j.pdig.copy_(h_pdig, non_blocking=True)
        j.match(77, stream=s.cuda_stream)
    with torch.cuda.stream(s):      # warm: the kernels are loaded before the timed sequence
        calls()
    gpu._n.check(lib.cir_hash_blocks_dev(None, dbuf.data_ptr(), doff.data_ptr(), dl.data_ptr(), 1,
                                         dout.data_ptr(), s.cuda_stream))
    torch.cuda.synchronize()
    j.ndig.fill_(POISON)
    j.pdig.fill_(POISON)
    for o in j.outputs():
        o.t.fill_(POISON)
    torch.cuda.synchronize()
    outs = [j.csrc, j.cfile, j.cplace, j.res]
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
        h = [p[:o.n].numpy() for o, p in zip(outs, pins)]
        got, res = j.decode(h[0].view(np.uint32), h[1].view(np.uint64), h[2].view(np.uint64),
                            h[3].view(np.uint64))
        assert got == want
        assert res[0] == 0 and res[1] == sum(w is not None for w in want) > 100 and res[3] == 300
        for o, p in zip(outs, pins):
            assert (p[o.n:].numpy() == POISON).all()
    finally:
        torch.cuda.synchronize()


# ---- the whole call ------------------------------------------------------------------------

def on_device(gpu, ctx, index, sources, skip):
    """cir_file_copies with a context equals the restatement and the host
    rule, and was answered by the device."""
    want, skipped = copies_restate.expected_copies(index, sources, skip)
    got, st = gpu.file_copies(index, sources, ctx, skip=skip)
    assert got == want, (got[:5], want[:5])
    assert st["on_device"] == 1 and st["why_host"] == 0, st
    host, hst = gpu.file_copies(index, sources, None, skip=skip)
    assert host == want
    assert st["skipped"] == skipped == hst["skipped"]
    vals = list(st.values())
    for k, v in copies_restate.expected_stats(index, sources, skip).items():
        assert vals[k] == v, (k, st)
    assert st["table_slots"] == gpu._n.lib.cir_match_table_slots(st["pool_files"])
    for k in st:
        if k not in ("table_slots", "on_device", "why_host"):
            assert st[k] == hst[k], k
    assert hst["table_slots"] == hst["on_device"] == hst["why_host"] == 0
    return got, st


@pytest.mark.parametrize("case", copies_cases.families(), ids=lambda c: c[0])
def test_families(gpu, ctx, case):
    _, index, sources, skip = case
    on_device(gpu, ctx, index, sources, skip)


def test_named_answers(gpu, ctx):
    fam = {name: rest for name, *rest in copies_cases.families()}
    got, st = on_device(gpu, ctx, *fam["renamed_dir"])
    assert [(g[0], g[3]) for g in got] == [(0, b"/conf"), (1, b"/app-1.2.3/bin/run"),
                                           (2, b"/app-1.2.3/lib/a.so"), (3, b"/app-1.2.3/lib/b.so")]
    assert st["same_path"] == 1 and st["candidates"] == 4
    got, _ = on_device(gpu, ctx, *fam["three_paths_one_source"])
    assert got == [(0, 0, 1, b"/a/p")]
    got, _ = on_device(gpu, ctx, *fam["sources_0_and_2"])
    assert got == [(0, 0, 0, b"/old/moved")]
    got, _ = on_device(gpu, ctx, *fam["skipped_sources"])
    assert got == [(0, 4, 0, b"/old/moved")]
    got, _ = on_device(gpu, ctx, *fam["escaped_source_path"])
    assert got == [(0, 0, 0, b"/sp ace/\xff\x01dir/back\\slash and space")]
    got, st = on_device(gpu, ctx, *fam["skip_bits"])
    assert [g[0] for g in got] == [i for i in range(70) if i not in (0, 63, 64, 65)]
    assert st["skipped_files"] == 4


@pytest.mark.parametrize("chunk", range(3))
def test_random_sweep(gpu, ctx, chunk):
    moved = 0
    for seed in range(20 * chunk, 20 * chunk + 20):
        index, sources, skip = copies_cases.random_case(seed)
        got, st = on_device(gpu, ctx, index, sources, skip)
        moved += st["candidates"] - st["same_path"]
    assert moved > 5


def test_declined_text_falls_back(gpu, ctx):
    """Two spaces between tokens: the host parser takes the line, the device
    declines it; the host rule answers, with the reason."""
    _, index, sources, skip = copies_cases.families()[0]
    double = sources[0].replace(b"  run x ", b"  run  x ")
    assert double != sources[0]
    want, _ = copies_restate.expected_copies(index, sources, skip)
    assert len(want) == 4
    got, st = gpu.file_copies(index, [double], ctx, skip=skip)
    assert got == want
    assert st["on_device"] == 0 and st["why_host"] == gpu._n.CIR_FILE_WHY_DECLINED
    assert st["table_slots"] == 0
    host, hst = gpu.file_copies(index, [double], None, skip=skip)
    assert host == want and {k: v for k, v in st.items() if k != "why_host"} == \
        {k: v for k, v in hst.items() if k != "why_host"}


CHILD = r"""
import os
import sys
sys.path[:0] = [%r, %r, %r]
import ciruela_amd as ca
import copies_cases, copies_restate
ctx = ca.Context(device_mask=1, staging_bytes=ca._n.CIR_STAGING_LAZY)
_, index, sources, skip = copies_cases.families()[0]
for mode in ("host", "device", "host"):      # (read per call)
    assert os.environ["CIR_LINKS_MATCH"] == "host"
    if mode == "device":
        del os.environ["CIR_LINKS_MATCH"]
    got, st = ca.file_copies(index, sources, ctx, skip=skip)
    os.environ["CIR_LINKS_MATCH"] = "host"
    assert got == copies_restate.expected_copies(index, sources, skip)[0], got
    print(st["on_device"], st["why_host"], st["table_slots"])
"""


def test_fallback_by_environment_in_a_child(gpu):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300,
                       env=dict(os.environ, CIR_LINKS_MATCH="host"))
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.split() == b"0 4 0 1 0 64 0 4 0".split(), p.stdout


# ---- the CLI -------------------------------------------------------------------------------

def test_cli_copies(gpu, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    rng = random.Random(80)
    bs = 4096
    datas = {"one": rng.randbytes(10000), "two": rng.randbytes(4096), "zero": b"",
             "sp ace": rng.randbytes(5), "stay": rng.randbytes(7000)}
    roots = []
    for k, sub in enumerate(("app-2", "app-1")):      # new, old: the directory was renamed
        root = tmp_path / ("r%d" % k)
        (root / sub).mkdir(parents=True)
        for name, data in datas.items():
            where = root if name == "stay" else root / sub
            (where / name).write_bytes(data)
            os.chmod(where / name, 0o644)
        roots.append(root)
    idx = [dirsig_oracle.scan(str(r), bs) for r in roots]
    paths = []
    for k, data in enumerate(idx):
        p = tmp_path / ("i%d.ds1" % k)
        p.write_bytes(data)
        paths.append(str(p))
    files = links_restate.file_entries(idx[0])
    linked = [f for f, _ in links_restate.expected_candidates(idx[0], idx[1:])[0]]
    assert linked == [0]           # /stay; every other file moved with its directory
    for flags, skip in (([], None), (["--unlinked"], linked)):
        want, _ = copies_restate.expected_copies(idx[0], idx[1:], skip)
        outs = []
        for extra in ([], ["--host"]):
            p = subprocess.run([cli, "copies"] + paths + flags + extra, capture_output=True,
                               timeout=300)
            assert p.returncode == 0, p.stderr[-2000:]
            assert (b"matched on the host" if extra else b"matched on the device") in p.stderr
            outs.append(p.stdout)
        assert outs[0] == outs[1]
        lines = [l.split(b" ") for l in outs[0].split(b"\n")[:-1]]
        assert [tuple(int(x) for x in l[:3]) for l in lines] == [w[:3] for w in want]
        assert [links_restate.unescape(l[3]) for l in lines] == [files[w[0]][0] for w in want]
        assert [links_restate.unescape(l[4]) for l in lines] == [w[3] for w in want]
    assert len(want) == 3 and b"/app-1/sp ace" in [w[3] for w in want]
