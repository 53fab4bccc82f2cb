"""The stream-ordering contract of the device-resident entry points.

include/ciruela_blockhash.h promises for every *_dev call that it
  1. is asynchronous on `stream` and never synchronises the device,
  2. is ordered on `stream` as one launch would be, although with a context
     parts of it run on the device's own quad-part stream (the short last block
     and the relay of launch_chunks_split; the exclusive quad part, both
     descriptor relays and the k_lane_tiles helper of launch_mixed), forked
     from `stream` by an event and joined back into it by another, and
  3. (cir_verify_segments_dev) writes nothing outside d_seg_bad[0 .. nseg)
     whatever d_seg_end holds.

The other GPU tests pass stream 0, produce their inputs beforehand and bracket
every call with a device-wide synchronise, and the part streams are
hipStreamNonBlocking, so none of them would see a dropped fork or join wait or
a hidden device synchronise.  Here nothing between the start of a sequence and
"results on host" waits for the device: only the stream under test is
synchronised.

The delay is the library's own public path: cir_hash_blocks_dev with a NULL
context and one descriptor is one chain on one lane, one launch on the given
stream, no side streams.  It occupies one wave and leaves the rest of the GPU
free, so a side-stream part with a missing dependency really runs early.  Its
length is calibrated per run (test_calibration_is_printed shows the figures), and
every test that relies on it proves its own precondition: an event recorded
right behind the delay must still be pending after the last enqueue has
returned, else the test fails with "delay too short: nothing was tested".

Every expected value is the C oracle's (oracle_hash_blocks,
oracle_hash_chunks, oracle_sha) over the bytes the call must see.  Only arena
bytes and a verify call's expected digests are ever written late; descriptors
and segment tables are final before a sequence starts, so whatever a broken
build reads early still lies inside live allocations.

A join the tests may not see: the on-stream readback shows a missing join only
where the side-stream part outlasts the caller-stream part.  That is D2 (64
quad chains of 8192 lines beside a lane part of tiny chains; also tested
without the delay and with the arena overwritten behind the readback).  For
C1-C3, D3 and D4 the two parts take similar time, and a missing join may go
unseen.

After the host has its results every test ends with a device-wide synchronise,
so that no work of a failing case is still running when the next one starts.
"""
import bisect
import random
import time
import zlib

import numpy as np
import pytest

from conftest import oracle_digest, oracle_sha

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
BLAKE, SHA = 1, 2
POISON = 0xA5
DELAY_CAP = 64 << 20
DELAY_FACTOR = 50
STREAMS = ["s0", "s1", "s2", "s3"]     # s0: torch's default stream (handle 0)


def lane_wave_slots():
    import torch
    return 64 * 4 * torch.cuda.get_device_properties(0).multi_processor_count


# ---- the cases (static: the module collects without a GPU) -------------------------------

DESC_SHAPES = ["D1", "D2", "D3", "D4"]
CHUNK_SHAPES = {"C1": 1024, "C2": 2048, "C3": 4096}
VERIFY_SHAPES = ["D1", "D2"]


def _case_ids():
    ids = []
    for sh in CHUNK_SHAPES:
        ids += ["chunks-%s-ctx" % sh, "chunks-%s-noctx" % sh]
    for sh in DESC_SHAPES + ["D5"]:
        ids += ["blocks-%s-ctx" % sh, "blocks-%s-noctx" % sh]
    for sh in VERIFY_SHAPES:
        ids.append("bounded-%s" % sh)
        ids.append("vblocks-%s" % sh)
        for v in ("vbounded", "vfirst", "vsegments", "vbitmap"):
            ids += ["%s-%s-max" % (v, sh), "%s-%s-real" % (v, sh)]
    return ids


CASE_IDS = _case_ids()   # (D1, D5 and every -noctx case fork nothing: controls)


# ---- shapes ----------------------------------------------------------------------------------

def _desc_lens(name, slots):
    rng = random.Random(zlib.crc32(name.encode()))
    if name == "D1":      # small batch: both parts serial on the caller's stream
        lens = [0, 1, 127, 128, 129, 40000] + [rng.randrange(0, 40001) for _ in range(294)]
        rng.shuffle(lens)
        skew = lambda i: 1 + i % 7  # noqa: E731 - misaligned starts
    elif name == "D2":    # exclusive quad part, gate, paced lane part, helper
        lens = [1 << 20] * 64 + [rng.randrange(0, 201) for _ in range(60000)]
        rng.shuffle(lens)
        skew = lambda i: 0  # noqa: E731 - packed: the short chains start anywhere
    elif name == "D3":    # lane-regime descriptor relay
        lens = [4096] * (slots + 700)
        skew = lambda i: 0  # noqa: E731
    elif name == "D4":    # quad-regime descriptor relay
        lens = [4096] * (2 * (slots // 4) + 77)
        skew = lambda i: 0  # noqa: E731
    elif name == "D5":    # sha512: ordered k_sha_desc through perm
        edge = [0, 1, 111, 112, 127, 128, 129, 4096]
        lens = [rng.choice(edge) if rng.random() < 0.5 else rng.randrange(0, 70000)
                for _ in range(3000)]
        skew = lambda i: i % 3  # noqa: E731
    else:
        raise KeyError(name)
    offs, pos = [], 0
    for i, ln in enumerate(lens):
        pos += skew(i)
        offs.append(pos)
        pos += ln
    return np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32), pos


def _oor_descriptors(offs, lens, arena_bytes, rng):
    """A few descriptors replaced by out-of-range ones (tests/test_gpu_bounded.py's
    kinds); returns the new arrays and the flagged indices."""
    kinds = [(arena_bytes - 10, 11), (arena_bytes + 1, 0), (1 << 40, 32768), (U64 - 15, 100),
             (U64, 1), (arena_bytes - 100, 0xFFFFFFFF)]
    small = [i for i in range(len(lens)) if lens[i] <= 40000]
    bad = sorted(rng.sample(small, len(kinds)))
    offs, lens = offs.copy(), lens.copy()
    for (o, ln), b in zip(kinds, bad):
        offs[b], lens[b] = o, ln
    return offs, lens, bad


class Shape:
    pass


class Out:
    """One output of a call: device bytes, their pinned host copy, what they must hold."""

    def __init__(self, torch, name, want):
        self.name = name
        self.want = np.ascontiguousarray(want).view(np.uint8).reshape(-1).copy()
        n = max(self.want.size, 1)
        self.dev = torch.full((n,), POISON, dtype=torch.uint8, device="cuda:0")
        self.pin = torch.full((n,), POISON, dtype=torch.uint8).pin_memory()

    @property
    def ptr(self):
        return self.dev.data_ptr()


class Case:
    def __init__(self, cid, shape, call, outs, verify=False):
        self.cid, self.shape, self.call, self.outs = cid, shape, call, outs
        # (destination, contents before the sequence, contents written on-stream, late)
        self.inputs = [(shape.arena, shape.decoy, shape.final)]
        if verify:
            self.inputs.append((shape.d_exp, shape.d_exp_decoy, shape.d_exp_final))
        self.unwanted = shape.want_decoy                          # the digests over the decoy

    def reset(self):
        for dst, before, _ in self.inputs:
            dst.copy_(before)
        for o in self.outs:
            o.dev.fill_(POISON)
            o.pin.fill_(POISON)


class World:
    """Everything the module shares: context, streams, shapes with their oracle
    digests (computed once, never changed), cases and the calibrated delay."""

    def __init__(self, gpu, oracle):
        import torch
        self.torch, self.gpu, self.oracle = torch, gpu, oracle
        self.lib, self.check = gpu._n.lib, gpu._n.check
        self.ctx = gpu.Context(device_mask=1, staging_bytes=8 << 20)
        self.streams = {"s0": torch.cuda.default_stream()}
        assert self.streams["s0"].cuda_stream == 0
        for k in STREAMS[1:]:
            self.streams[k] = torch.cuda.Stream()
        self.slots = lane_wave_slots()
        self.shapes, self.cases = {}, {}
        for name in DESC_SHAPES + ["D5"]:
            self.shapes[name] = self._desc_shape(name)
        for name, bs in CHUNK_SHAPES.items():
            self.shapes[name] = self._chunk_shape(name, bs)
        for cid in CASE_IDS:
            self.cases[cid] = self._case(cid)
        torch.cuda.synchronize()

    # -- data --
    def fill(self, nbytes, seed):
        torch = self.torch
        n = (nbytes + 64 + 7) // 8 * 8
        t = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        self.check(self.lib.cir_fill_splitmix64_dev(t.data_ptr(), n, seed, 0, 0, None))
        return t

    def _contents(self, sh, nbytes, seed):
        sh.final = self.fill(nbytes, seed)
        sh.decoy = self.fill(nbytes, seed ^ 0x5DEECE66D)
        sh.arena = sh.decoy.clone()
        self.torch.cuda.synchronize()

    def _blake_desc(self, host, offs, lens):
        want = np.zeros(32 * len(offs), dtype=np.uint8)
        self.oracle.oracle_hash_blocks(host.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                       len(offs), want.ctypes.data, 8)
        return want.reshape(-1, 32)

    def _sha_desc(self, host, offs, lens):
        raw = host.tobytes()
        return np.frombuffer(b"".join(oracle_sha(self.oracle, raw[int(o):int(o) + int(ln)])
                                      for o, ln in zip(offs, lens)),
                             dtype=np.uint8).reshape(-1, 32).copy()

    def dev_desc(self, offs, lens):
        torch = self.torch
        return (torch.tensor(offs.view(np.int64), device="cuda:0"),
                torch.tensor(lens.view(np.int32), device="cuda:0"))

    def _desc_shape(self, name):
        torch = self.torch
        sh = Shape()
        sh.name, sh.kind = name, "desc"
        sh.offs, sh.lens, sh.arena_bytes = _desc_lens(name, self.slots)
        sh.n = len(sh.offs)
        sh.ht = SHA if name == "D5" else BLAKE
        self._contents(sh, sh.arena_bytes, zlib.crc32(name.encode()))
        sh.d_off, sh.d_len = self.dev_desc(sh.offs, sh.lens)
        hashd = self._sha_desc if sh.ht == SHA else self._blake_desc
        sh.want = hashd(sh.final.cpu().numpy(), sh.offs, sh.lens)
        sh.want_decoy = hashd(sh.decoy.cpu().numpy(), sh.offs, sh.lens)
        # the two contents give different digests for every non-empty chain: a
        # call that saw the decoy cannot pass
        nonempty = sh.lens > 0
        assert nonempty.sum() >= sh.n // 2
        assert (sh.want[nonempty] != sh.want_decoy[nonempty]).any(1).all()
        if name in VERIFY_SHAPES:
            rng = random.Random(sh.n)
            sh.offs_oor, sh.lens_oor, sh.oor = _oor_descriptors(sh.offs, sh.lens, sh.arena_bytes,
                                                               rng)
            sh.d_off_oor, sh.d_len_oor = self.dev_desc(sh.offs_oor, sh.lens_oor)
            sh.want_oor = sh.want.copy()
            sh.want_oor[sh.oor] = 0
            # expected digests: the final contents' with a handful corrupted;
            # before the sequence the buffer holds the decoy's
            sh.corrupt = sorted({0, sh.n - 1, sh.n // 2} | set(rng.sample(range(sh.n), 4)))
            exp = sh.want.copy()
            for b in sh.corrupt:
                exp[b, b % 32] ^= 0x10
            sh.d_exp_final = torch.from_numpy(exp.reshape(-1).copy()).to("cuda:0")
            sh.d_exp_decoy = torch.from_numpy(sh.want_decoy.reshape(-1).copy()).to("cuda:0")
            sh.d_exp = sh.d_exp_decoy.clone()
            sh.ok = np.ones(sh.n, dtype=np.uint8)
            sh.ok[sh.corrupt] = 0
            assert 0 < len(sh.corrupt) < sh.n
            # a segment table with empty segments in front, inside and behind
            cuts = sorted(rng.choices(range(sh.n + 1), k=38))
            sh.seg_end = np.array([0] + cuts + [sh.n, sh.n], dtype=np.uint32)
            sh.d_seg_end = torch.tensor(sh.seg_end.view(np.int32), device="cuda:0")
            sh.seg_bad = np.zeros(len(sh.seg_end), dtype=np.uint8)
            for b in sh.corrupt:
                sh.seg_bad[bisect.bisect_right(sh.seg_end.tolist(), b)] = 1
            bits = np.zeros((sh.n + 63) // 64 * 64, dtype=np.uint8)
            bits[:sh.n] = sh.ok
            sh.have = np.packbits(bits, bitorder="little").view(np.uint64)
        return sh

    def _chunk_shape(self, name, bs):
        slots, q = self.slots, self.slots // 4
        nfull, tail, relay = {"C1": (50000, 3, 0), "C2": (slots + 2000, 5, 2000),
                              "C3": (2 * q + 77, 3, 77)}[name]
        # the route, as test_chunks_dev_relay asserts it
        assert self.lib.cir_debug_relay_blocks(nfull, bs) == relay
        sh = Shape()
        sh.name, sh.kind, sh.bs = name, "chunks", bs
        sh.nbytes = nfull * bs + tail
        sh.n = nfull + 1
        self._contents(sh, sh.nbytes, zlib.crc32(name.encode()))

        def chunks(t):
            host = t.cpu().numpy()
            out = np.zeros(sh.n * 32, dtype=np.uint8)
            self.oracle.oracle_hash_chunks(host.ctypes.data, sh.nbytes, bs, out.ctypes.data, 8)
            return out.reshape(-1, 32)
        sh.want, sh.want_decoy = chunks(sh.final), chunks(sh.decoy)
        assert (sh.want != sh.want_decoy).any(1).all()
        return sh

    # -- cases --
    def _case(self, cid):
        torch, lib = self.torch, self.lib
        kind, shname, *opt = cid.split("-")
        sh = self.shapes[shname]
        ctxh = None if opt == ["noctx"] else self.ctx.handle
        arena = sh.arena.data_ptr()
        dig = Out(torch, "digests", sh.want)
        if kind == "chunks":
            return Case(cid, sh, lambda h: lib.cir_hash_chunks_dev(
                ctxh, arena, sh.nbytes, sh.bs, dig.ptr, h), [dig])
        off, ln, n = sh.d_off.data_ptr(), sh.d_len.data_ptr(), sh.n
        if kind == "blocks":
            return Case(cid, sh, lambda h: lib.cir_hash_blocks_dev_ht(
                ctxh, sh.ht, arena, off, ln, n, dig.ptr, h), [dig])
        if kind == "bounded":
            dig = Out(torch, "digests", sh.want_oor)
            nrange = Out(torch, "nrange", np.array([len(sh.oor)], dtype=np.uint32))
            return Case(cid, sh, lambda h: lib.cir_hash_blocks_dev_bounded(
                ctxh, BLAKE, arena, sh.arena_bytes, sh.d_off_oor.data_ptr(),
                sh.d_len_oor.data_ptr(), n, dig.ptr, nrange.ptr, h), [dig, nrange])
        ab = sh.arena_bytes if opt == ["real"] else U64
        exp = sh.d_exp.data_ptr()
        nbad = Out(torch, "nbad", np.array([len(sh.corrupt)], dtype=np.uint32))
        if kind in ("vblocks", "vbounded"):
            ok = Out(torch, "ok", sh.ok)
            if kind == "vblocks":
                call = lambda h: lib.cir_verify_blocks_dev(  # noqa: E731
                    ctxh, BLAKE, arena, off, ln, n, exp, dig.ptr, ok.ptr, nbad.ptr, h)
            else:
                call = lambda h: lib.cir_verify_blocks_dev_bounded(  # noqa: E731
                    ctxh, BLAKE, arena, ab, off, ln, n, exp, dig.ptr, ok.ptr, nbad.ptr, h)
            outs = [dig, ok, nbad]
        elif kind == "vfirst":
            first = Out(torch, "first", np.array([sh.corrupt[0]], dtype=np.uint64))
            call = lambda h: lib.cir_verify_first_dev(  # noqa: E731
                ctxh, BLAKE, arena, ab, off, ln, n, exp, dig.ptr, first.ptr, nbad.ptr, h)
            outs = [dig, first, nbad]
        elif kind == "vsegments":
            flags = Out(torch, "seg_bad", sh.seg_bad)
            nseg_bad = Out(torch, "nbad_seg", np.array([int(sh.seg_bad.sum())], dtype=np.uint32))
            call = lambda h: lib.cir_verify_segments_dev(  # noqa: E731
                ctxh, BLAKE, arena, ab, off, ln, n, exp, dig.ptr, sh.d_seg_end.data_ptr(),
                len(sh.seg_end), flags.ptr, nseg_bad.ptr, h)
            outs = [dig, flags, nseg_bad]
        elif kind == "vbitmap":
            have = Out(torch, "have", sh.have)
            call = lambda h: lib.cir_verify_bitmap_dev(  # noqa: E731
                ctxh, BLAKE, arena, ab, off, ln, n, exp, dig.ptr, have.ptr, nbad.ptr, h)
            outs = [dig, have, nbad]
        else:
            raise KeyError(cid)
        return Case(cid, sh, call, outs, verify=True)

    # -- the delay --
    def init_delay(self):
        torch = self.torch
        self.delay_buf = self.fill(DELAY_CAP, 99)
        self.delay_off = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        self.delay_len = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        self.delay_out = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
        self.delay_bytes = 0

    def set_delay(self, nbytes):
        self.delay_len.fill_(nbytes)
        self.delay_bytes = nbytes
        self.torch.cuda.synchronize()

    def delay(self, st):
        """One chain on one lane, one launch on st; returns the marker event behind it."""
        self.check(self.lib.cir_hash_blocks_dev(
            None, self.delay_buf.data_ptr(), self.delay_off.data_ptr(),
            self.delay_len.data_ptr(), 1, self.delay_out.data_ptr(), st.cuda_stream))
        marker = self.torch.cuda.Event()
        marker.record(st)
        return marker

    def time_delay(self, nbytes):
        """Event-timed duration (ms) of a delay chain of nbytes."""
        torch = self.torch
        st = self.streams["s1"]
        self.set_delay(nbytes)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        self.delay(st)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def enqueue(self, case, st, marker=None, tail_decoy=False):
        """{on-stream late writes, the call, on-stream readback [, the decoy over
        the arena again]} on st; returns whether marker was still pending right
        after the call returned."""
        torch = self.torch
        pending = None
        with torch.cuda.stream(st):
            for dst, _, late in case.inputs:
                dst.copy_(late, non_blocking=True)
            self.check(case.call(st.cuda_stream))
            if marker is not None:
                pending = not marker.query()
            for o in case.outs:
                o.pin.copy_(o.dev, non_blocking=True)
            if tail_decoy:
                case.shape.arena.copy_(case.shape.decoy, non_blocking=True)
        return pending

    def enqueue_seconds(self, case):
        """Median host time of enqueue() on a warm context and an idle stream."""
        torch = self.torch
        st = self.streams["s1"]
        times = []
        for rep in range(6):       # the first one warms the case (and grows the scratch)
            case.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.enqueue(case, st)
            times.append(time.perf_counter() - t0)
            st.synchronize()
        torch.cuda.synchronize()   # nothing of this shape runs into the next one
        return sorted(times[1:])[2]

    def calibrate(self):
        self.init_delay()
        self.time_delay(256 << 10)                      # loads the kernel
        t_a, t_b = self.time_delay(256 << 10), self.time_delay(1 << 20)
        ms_per_byte = max(t_b - t_a, 1e-6) / ((1 << 20) - (256 << 10))
        enq = {cid: self.enqueue_seconds(c) for cid, c in self.cases.items()}
        worst = max(enq, key=enq.get)
        need_ms = DELAY_FACTOR * enq[worst] * 1e3
        nbytes = min(DELAY_CAP, max(256 << 10, -(-int(need_ms / ms_per_byte) // 4096) * 4096))
        ms = self.time_delay(nbytes)
        for _ in range(3):                              # the estimate fell short: lengthen
            if ms >= need_ms or nbytes >= DELAY_CAP:
                break
            nbytes = min(DELAY_CAP, -(-int(nbytes * 1.25 * need_ms / ms) // 4096) * 4096)
            ms = self.time_delay(nbytes)
        self.delay_ms = ms
        self.calibration = (
            "delay calibration: %.3f us per 128-byte line; largest enqueue %.1f us (%s); "
            "chain %d bytes (%d lines), %.2f ms = %.0f x the largest enqueue" %
            (ms_per_byte * 128 * 1e3, enq[worst] * 1e6, worst, nbytes, nbytes // 128, ms,
             ms / (enq[worst] * 1e3)))


@pytest.fixture(scope="module")
def world(gpu, oracle):
    import torch
    w = World(gpu, oracle)
    w.calibrate()
    yield w
    torch.cuda.synchronize()
    w.ctx.close()


def _check_outputs(case):
    for o in case.outs:
        got = o.pin.numpy()
        if o.name == "digests":
            g, w = got.reshape(-1, 32), o.want.reshape(-1, 32)
            bad = np.nonzero((g != w).any(1))[0]
            saw_decoy = [int(b) for b in bad[:8] if (g[b] == case.unwanted[b]).all()]
            assert bad.size == 0, "%s: %d digests differ, first %s; the decoy's digest at %s" % (
                case.cid, bad.size, bad[:8].tolist(), saw_decoy)
            assert (g != case.unwanted).any(), "the decoy's digests"
        else:
            assert np.array_equal(got, o.want), (case.cid, o.name, got[:16].tolist(),
                                                 o.want[:16].tolist())


def _sequence(w, case, st, delay_on=None, tail_decoy=False):
    """Before the sequence: the arena holds the decoy, the expected digests the
    decoy's, the outputs poison; descriptors are final.  Then on st: [the delay
    and a marker,] the late writes, the call, the readback [, the arena
    overwritten again]; st alone is synchronised.  Returns (marker pending
    right after the call, marker pending after the last enqueue)."""
    torch = w.torch
    case.reset()
    torch.cuda.synchronize()
    after_call = after_all = None
    try:
        marker = w.delay(delay_on) if delay_on is not None else None
        after_call = w.enqueue(case, st, marker, tail_decoy)
        if marker is not None:
            after_all = not marker.query()
        st.synchronize()
        _check_outputs(case)
    finally:
        torch.cuda.synchronize()
    return after_call, after_all


def test_calibration_is_printed(world, capsys):
    """The delay's calibration, shown whatever the capture mode (it is a figure
    to read, not a bound: every delayed test checks its own precondition)."""
    with capsys.disabled():
        print("\n" + world.calibration)
    assert world.delay_bytes % 128 == 0 and 0 < world.delay_bytes <= DELAY_CAP


# ---- 2. fork: work queued earlier on the caller's stream is seen by every part --------

@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_fork_sees_earlier_work_on_the_stream(world, cid, stream):
    """Behind a long delay on the caller's stream the arena (and a verify call's
    expected digests) get their real contents, then the call runs and its
    outputs are read back, all on that stream.  Every output is the oracle's
    over the real contents: a part on the quad-part stream that did not wait
    for the fork event would have hashed the decoy long before the copy ran.
    Three created streams beside the default one: with 4 hardware queues a
    user stream may share its queue with the quad-part stream, which hides a
    missing wait on that stream alone.  The on-stream readback is the join
    check (see the module docstring for where it cannot see a missing join)."""
    st = world.streams[stream]
    case = world.cases[cid]
    _, pending = _sequence(world, case, st, delay_on=st)
    assert pending, "delay too short: nothing was tested"


# ---- 3. join: work queued later on the caller's stream sees every part's result ------

@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("cid", ["blocks-D2-ctx", "bounded-D2", "vbitmap-D2-max"])
def test_join_before_later_work_on_the_stream(world, cid, stream):
    """D2 without the delay: the 64 quad chains of 8192 lines run for
    milliseconds on the quad-part stream beside a lane part of tiny chains on
    the caller's.  The readback and a copy of the decoy over the arena follow
    on the caller's stream: without the join the readback takes digests that
    are not written yet and the quad chains hash decoy bytes.  Only here is
    the join check discriminating: for C1-C3, D3 and D4 both parts take
    similar time and a missing join may go unseen."""
    _sequence(world, world.cases[cid], world.streams[stream], tail_decoy=True)


# ---- 4. asynchrony --------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["same_stream", "other_stream"])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_call_returns_while_the_delay_runs(world, cid, where):
    """The context is warm (the calibration ran every case, so no scratch
    grows any more).  With the delay queued on the call's stream, or on another
    one, the call returns while the delay still runs: it waited neither for
    its stream nor for the device (a device-wide synchronise inside the call
    would wait for the other stream's delay too)."""
    st = world.streams["s1"]
    delay_on = st if where == "same_stream" else world.streams["s2"]
    after_call, _ = _sequence(world, world.cases[cid], st, delay_on=delay_on)
    assert after_call, "the call returned only after the delay (%.1f ms) had ended" % \
        world.delay_ms


@pytest.mark.parametrize("where", ["same_stream", "other_stream"])
def test_fill_returns_while_the_delay_runs(world, where):
    torch = world.torch
    st = world.streams["s1"]
    delay_on = st if where == "same_stream" else world.streams["s2"]
    nwords, seed = 100003, 77
    buf = torch.full((8 * nwords,), POISON, dtype=torch.uint8, device="cuda:0")
    pin = torch.zeros(8 * nwords, dtype=torch.uint8).pin_memory()
    want = np.zeros(nwords, dtype=np.uint64)
    world.oracle.oracle_splitmix64_fill(want.ctypes.data, 0, nwords, seed, 0, 0)
    torch.cuda.synchronize()
    try:
        marker = world.delay(delay_on)
        world.check(world.lib.cir_fill_splitmix64_dev(buf.data_ptr(), 8 * nwords, seed, 0, 0,
                                                      st.cuda_stream))
        pending = not marker.query()
        with torch.cuda.stream(st):
            pin.copy_(buf, non_blocking=True)
        st.synchronize()
        assert np.array_equal(pin.numpy().view(np.uint64), want)
    finally:
        torch.cuda.synchronize()
    assert pending, "the call returned only after the delay had ended"


# ---- 5. one context, two streams, no host wait between the calls -------------------------

def test_two_streams_share_the_scratch_without_host_waits(world):
    """D2 on stream A (long-running; the ordering scratch in use), at once
    another batch through cir_hash_blocks_dev_bounded on stream B (ordering and
    bounds scratch), D2 in another shuffle on A, B again: four calls and their
    readbacks with no host wait between them.  The scratch of one call must
    stay untouched until that call is done (order_free, bound_free)."""
    torch, lib, w = world.torch, world.lib, world
    sa, sb = w.streams["s1"], w.streams["s2"]
    d2 = w.shapes["D2"]
    rng = random.Random(5)
    perm = list(range(d2.n))
    rng.shuffle(perm)
    perm = np.array(perm)
    d_off2, d_len2 = w.dev_desc(d2.offs[perm].copy(), d2.lens[perm].copy())
    # B: 5000 chains of 0..4096 bytes at other offsets, a few out of range
    nb = 5000
    b_lens = np.array([rng.randrange(0, 4097) for _ in range(nb)], dtype=np.uint32)
    b_bytes = 6 << 20
    b_offs = np.array([rng.randrange(0, b_bytes - 4096) for _ in range(nb)], dtype=np.uint64)
    b_offs, b_lens, b_oor = _oor_descriptors(b_offs, b_lens, b_bytes, rng)
    b_arena = w.fill(b_bytes, 1234)
    b_host = b_arena.cpu().numpy()
    in_range = np.ones(nb, dtype=bool)
    in_range[b_oor] = False
    b_want = w._blake_desc(b_host, np.where(in_range, b_offs, 0).astype(np.uint64),
                           np.where(in_range, b_lens, 0).astype(np.uint32))
    b_want[b_oor] = 0
    d_boff, d_blen = w.dev_desc(b_offs, b_lens)
    outs = {"a1": Out(torch, "digests", d2.want), "a2": Out(torch, "digests", d2.want[perm]),
            "b1": Out(torch, "digests", b_want), "b2": Out(torch, "digests", b_want)}
    nr = {k: Out(torch, "nrange", np.array([len(b_oor)], dtype=np.uint32)) for k in ("b1", "b2")}
    d2.arena.copy_(d2.final)
    torch.cuda.synchronize()

    def call_a(off, ln, out):
        w.check(lib.cir_hash_blocks_dev_ht(w.ctx.handle, BLAKE, d2.arena.data_ptr(),
                                           off.data_ptr(), ln.data_ptr(), d2.n, out.ptr,
                                           sa.cuda_stream))
        with torch.cuda.stream(sa):
            out.pin.copy_(out.dev, non_blocking=True)

    def call_b(k):
        w.check(lib.cir_hash_blocks_dev_bounded(w.ctx.handle, BLAKE, b_arena.data_ptr(), b_bytes,
                                                d_boff.data_ptr(), d_blen.data_ptr(), nb,
                                                outs[k].ptr, nr[k].ptr, sb.cuda_stream))
        with torch.cuda.stream(sb):
            outs[k].pin.copy_(outs[k].dev, non_blocking=True)
            nr[k].pin.copy_(nr[k].dev, non_blocking=True)

    try:
        call_a(d2.d_off, d2.d_len, outs["a1"])
        call_b("b1")
        call_a(d_off2, d_len2, outs["a2"])
        call_b("b2")
        sa.synchronize()
        sb.synchronize()
        for k, o in list(outs.items()) + list(nr.items()):
            got, want = o.pin.numpy(), o.want
            if o.name == "digests":
                bad = np.nonzero((got.reshape(-1, 32) != want.reshape(-1, 32)).any(1))[0]
                assert bad.size == 0, (k, bad.size, bad[:8].tolist())
            else:
                assert np.array_equal(got, want), (k, got.tolist())
    finally:
        torch.cuda.synchronize()


# ---- 6. hostile segment tables for cir_verify_segments_dev --------------------------------

GUARD = 64
NSEG = 9


def _seg_call(w, d_arena, arena_bytes, d_off, d_len, n, expected, seg_end):
    """One cir_verify_segments_dev call with 0xAA in the flags and in a 64-byte
    guard on both sides of them and garbage in the count: (status, flags, front
    guard, back guard, count, digests)."""
    torch = w.torch
    nseg = len(seg_end)
    d_exp = torch.tensor(np.frombuffer(bytes(expected), dtype=np.uint8).copy(), device="cuda:0")
    d_dig = torch.full((32 * n,), 0xCD, dtype=torch.uint8, device="cuda:0")
    d_seg = torch.tensor(np.array(seg_end, dtype=np.uint32).view(np.int32), device="cuda:0")
    d_bad = torch.full((GUARD + nseg + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.full((1,), 999, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.current_stream()
    rc = w.lib.cir_verify_segments_dev(w.ctx.handle, BLAKE, d_arena.data_ptr(), arena_bytes,
                                       d_off.data_ptr(), d_len.data_ptr(), n, d_exp.data_ptr(),
                                       d_dig.data_ptr(), d_seg.data_ptr(), nseg,
                                       d_bad.data_ptr() + GUARD, d_cnt.data_ptr(), st.cuda_stream)
    st.synchronize()
    flags = d_bad.cpu().numpy()
    return (rc, flags[GUARD:GUARD + nseg].tolist(), flags[:GUARD].tolist(),
            flags[GUARD + nseg:].tolist(), int(d_cnt.item()) & 0xFFFFFFFF, d_dig.cpu().numpy())


def _hostile_tables(nblk, rng):
    return {
        "zeros": [0] * NSEG,
        "ones": [0xFFFFFFFF] * NSEG,
        "decreasing": [nblk - 1 - i * (nblk // NSEG) for i in range(NSEG)],
        "last_below_nblk": sorted(rng.sample(range(nblk // 2), NSEG - 1)) + [nblk - 3],
        "last_above_nblk": sorted(rng.sample(range(nblk), NSEG - 1)) + [nblk + 1000],
        "random_u32": [rng.randrange(0, 1 << 32) for _ in range(NSEG)],
        "single_zero": [0],
    }


@pytest.mark.parametrize("bound", ["max", "real"])
@pytest.mark.parametrize("nblk", [65, 257, 1025])
def test_seg_bad_hostile_tables(world, nblk, bound):
    """Every expected digest is wrong, so every lane of k_seg_bad looks its
    segment up and stores.  Whatever the table holds the call succeeds, the
    guards on both sides of the flags are intact, every flag is 0 or 1, the
    count is the number of 1 flags and the digests are the oracle's; for the
    tables that are still non-decreasing the flags follow the bisection rule
    (the first s with seg_end[s] > b, clamped to nseg - 1)."""
    torch, w = world.torch, world
    rng = random.Random(nblk)
    lens = [rng.randrange(0, 201) for _ in range(nblk)]
    offs, pos = [], 0
    for ln in lens:
        offs.append(pos)
        pos += ln
    host = np.frombuffer(rng.randbytes(pos + 64), dtype=np.uint8).copy()
    raw = host.tobytes()
    good = [oracle_digest(w.oracle, raw[o:o + ln]) for o, ln in zip(offs, lens)]
    wrong = b"".join(bytes([d[0] ^ 1]) + d[1:] for d in good)
    d_arena = torch.from_numpy(host).to("cuda:0")
    d_off, d_len = w.dev_desc(np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32))
    arena_bytes = pos if bound == "real" else U64
    try:
        for name, table in _hostile_tables(nblk, rng).items():
            assert all(0 <= e < 1 << 32 for e in table), name
            rc, flags, front, back, count, dig = _seg_call(w, d_arena, arena_bytes, d_off, d_len,
                                                           nblk, wrong, table)
            assert rc == 0, (name, rc)
            assert front == [0xAA] * GUARD and back == [0xAA] * GUARD, name
            assert set(flags) <= {0, 1}, (name, flags)
            assert count == sum(flags), (name, count, flags)
            assert dig.tobytes() == b"".join(good), name
            if table == sorted(table):
                want = [0] * len(table)
                for b in range(nblk):
                    want[min(bisect.bisect_right(table, b), len(table) - 1)] = 1
                assert flags == want, (name, flags, want)
    finally:
        torch.cuda.synchronize()
