"""cir_index_sketch / cir_sketch_rank / cir_sketch_key / cir_sketch_digests_dev
without a GPU: the declarations in the header, the ctypes table, INTEGRATION.md's
extern block and the Python interface; the key and the host sketch (ctx = NULL)
against the restatement (tests/sketch_restate.py), byte for byte; the ranking
on a hand-counted case and on the skipped kinds; the argument checks of the
device-resident call (all CIR_EINVAL cases are decided before any device call);
the CLI; a sanitized fuzz of the shared rule header (tools/sketch_fuzz.cpp, a
stand-alone program); and the new kernels' resources in the built code object.
No expected value comes from the library.
"""
import ctypes
import json
import os
import random
import re
import struct
import subprocess

import pytest

from conftest import GOLDEN, ROOT

import codeobj
import sketch_cases
import sketch_restate
from ciruela_amd import _native

NEW = ("cir_sketch_key", "cir_sketch_rank", "cir_sketch_work_bytes", "cir_sketch_digests_dev",
       "cir_index_sketch")
KERNELS = ("k_sketch_insert", "k_sketch_scan", "k_sketch_compact", "k_sketch_sort")
M64 = (1 << 64) - 1


def golden_index():
    with open(os.path.join(GOLDEN, "dirsig_v1_example.json")) as f:
        return json.load(f)["index"].encode()


# ---- declarations and bindings ---------------------------------------------------------

def test_header_declares_the_calls():
    full = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|uint64_t) %s\s*\(" % name, text), name
    for define in ("CIR_SKETCH_MAX_K 4096", "CIR_SKETCH_DEFAULT_K 1024", "CIR_SKETCH_RES_FIELDS 4",
                   "CIR_SKETCH_OK 0", "CIR_SKETCH_DECLINED 1", "CIR_SKETCH_STATS_FIELDS 6"):
        assert re.search(r"#define %s\b" % define, text), define
    assert "CIR_SKETCH=host" in full[:full.index("#ifndef CIRUELA_BLOCKHASH_H")]


def test_ctypes_table_binds_the_calls():
    for name in NEW:
        assert name in _native._SIGS
    assert len(_native._SIGS["cir_sketch_rank"][1]) == 10
    assert len(_native._SIGS["cir_sketch_digests_dev"][1]) == 9
    assert len(_native._SIGS["cir_index_sketch"][1]) == 7
    assert (_native.CIR_SKETCH_MAX_K, _native.CIR_SKETCH_DEFAULT_K) == (4096, 1024)
    assert len({0, _native.CIR_SKETCH_WHY_ENV, _native.CIR_SKETCH_WHY_TEXT,
                _native.CIR_SKETCH_WHY_DECLINED, _native.CIR_SKETCH_WHY_SIZE}) == 5


def test_integration_extern_block_names_the_calls():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    assert set(NEW) <= set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    rest = text[text.index("\n}\n"):]
    assert "cir_index_sketch(" in rest and "cir_sketch_rank(" in rest      # the step of section 3


def test_python_interface_exists():
    import ciruela_amd as ca
    for name in ("index_sketch", "sketch_rank", "sketch_key"):
        assert callable(getattr(ca, name)) and name in ca.__all__ and name in ca.__doc__, name
    assert callable(ca.Context.sketch_digests_dev) and "Context.sketch_digests_dev" in ca.__doc__


# ---- the key -------------------------------------------------------------------------------

def test_key_equals_the_restatement():
    lib = _native.lib
    rng = random.Random(5)
    for _ in range(1000):
        d = rng.randbytes(32)
        assert lib.cir_sketch_key(d) == sketch_restate.key(d)
    for want in (0, M64, 1, M64 - 1, 1 << 63):
        d = sketch_cases.digest_with_key(want, rng)
        assert lib.cir_sketch_key(d) == want
    assert sketch_restate.key(bytes(32)) == lib.cir_sketch_key(bytes(32)) != 0


# ---- the host sketch -----------------------------------------------------------------------

def raw_sketch(index, k, ctx=None):
    """cir_index_sketch through ctypes with poisoned outputs: (status, blob
    bytes or None, blob_len, stats)."""
    lib = _native.lib
    blob, blob_len = ctypes.c_void_p(1), ctypes.c_size_t(77)
    stats = (ctypes.c_uint64 * 6)(*([99] * 6))
    rc = lib.cir_index_sketch(ctx, index, len(index), k, ctypes.byref(blob),
                              ctypes.byref(blob_len), stats)
    data = None
    if blob.value:
        data = ctypes.string_at(blob.value, blob_len.value)
        lib.cir_free(blob)
    return rc, data, blob_len.value, list(stats)


HOST_INDEXES = [("golden", golden_index())] + sketch_cases.cpu_indexes(64)


@pytest.mark.parametrize("case", HOST_INDEXES, ids=lambda c: c[0])
@pytest.mark.parametrize("k", [1, 64, 1024, 4096])
def test_host_sketch_equals_the_restatement(case, k):
    _, index = case
    want = sketch_restate.sketch(index, k)
    rc, got, n, stats = raw_sketch(index, k)
    assert rc == 0 and got == want and n == len(want)
    _, _, blocks = sketch_restate.index_blocks(index)
    assert stats == [0, 0, len(blocks), (len(want) - 40) // 8, 0, 0]
    assert sketch_restate.parse(got) is not None


def test_host_sketch_around_the_default_k():
    import ciruela_amd as ca
    for n in (1023, 1024, 1025):
        index = sketch_cases.index_of(sketch_cases.random_digests(n, n))
        assert ca.index_sketch(index) == sketch_restate.sketch(index, 1024)
        assert len(ca.index_sketch(index)) == 40 + 8 * min(n, 1024)


def test_named_host_answers():
    fam = dict(HOST_INDEXES)
    assert len(raw_sketch(fam["no_blocks"], 64)[1]) == 40
    assert len(raw_sketch(fam["one_digest_500_times"], 64)[1]) == 48
    p = sketch_restate.parse(raw_sketch(fam["half_share_one_digest"], 4096)[1])
    assert p[:4] == (2, 4096, 4096, 300) and len(p[4]) == 150
    p = sketch_restate.parse(raw_sketch(fam["golden"], 1024)[1])
    assert p[:4] == (2, 1024, 32768, 3) and len(p[4]) == 3
    # crafted keys 0 and 2^64 - 1 are ordinary members
    rng = random.Random(9)
    d = [sketch_cases.digest_with_key(x, rng) for x in (M64, 0, 5)] + \
        sketch_cases.random_digests(20, 1)
    p = sketch_restate.parse(raw_sketch(sketch_cases.index_of(d), 64)[1])
    assert p[4][0] == 0 and p[4][1] == 5 and p[4][-1] == M64 and len(p[4]) == 23
    p = sketch_restate.parse(raw_sketch(sketch_cases.index_of(d), 2)[1])
    assert p[4] == [0, 5]


def test_errors_leave_null_and_zero_stats():
    index = sketch_cases.index_of(sketch_cases.random_digests(5, 1))
    digest = re.search(rb" ([0-9a-f]{64})[ \n]", index).group(1)
    short_hash = index.replace(digest, digest[:32], 1)
    for bad, code in ((b"not an index\n", _native.CIR_EPARSE), (index[:150], _native.CIR_EPARSE),
                      (short_hash, _native.CIR_EHASHSIZE)):
        rc, blob, n, stats = raw_sketch(bad, 64)
        assert rc == code, (bad[:20], rc)
        assert blob is None and n == 0 and stats == [0] * 6
    for k in (0, 4097, 1 << 31):
        rc, blob, n, stats = raw_sketch(index, k)
        assert rc == _native.CIR_EINVAL and blob is None and n == 0 and stats == [0] * 6
    assert _native.lib.cir_index_sketch(None, None, 0, 64, None, None, None) == _native.CIR_EINVAL


# ---- the ranking ---------------------------------------------------------------------------

def raw_rank(need, sources, nsrc=None):
    """cir_sketch_rank through ctypes: (status, [(ordinal, shared, examined)], skipped)."""
    lib = _native.lib
    bufs = [None if s is None else ctypes.create_string_buffer(s, max(len(s), 1))
            for s in sources]
    n = max(len(sources), 1)
    sp = (ctypes.c_void_p * n)(*[None if b is None else ctypes.cast(b, ctypes.c_void_p)
                                 for b in bufs])
    sl = (ctypes.c_size_t * n)(*[0 if s is None else len(s) for s in sources])
    order, shared, examined = ((ctypes.c_uint64 * n)(*([77] * n)) for _ in range(3))
    nranked, nskipped = ctypes.c_size_t(55), ctypes.c_size_t(55)
    rc = lib.cir_sketch_rank(need, len(need), sp, sl, len(sources) if nsrc is None else nsrc,
                             order, shared, examined, ctypes.byref(nranked),
                             ctypes.byref(nskipped))
    return rc, [(order[i], shared[i], examined[i]) for i in range(nranked.value)], nskipped.value


def blob_of_keys(keys, k, n_blocks=None, hash_code=1, bs=64):
    keys = sorted(keys)
    return sketch_restate.blob(hash_code, k, bs, len(keys) if n_blocks is None else n_blocks, keys)


def test_rank_hand_counted():
    """Need: keys 10..80 step 10, k = 8 (full: t = 80).  Source 0 holds {10, 20, 30, 40} with k
    = 4 (full: t = 40): tau = 40, examined 4, shared 4 -> 4/4.  Source 1 holds {10, 30, 50, 70,
    90} with k = 8 (not full): tau = 80, examined 8, shared 4 -> 4/8.  Source 2 holds {20, 40,
    60, 80, 85, 95} with k = 16 (not full): tau = 80, examined 8, shared 4 -> 4/8, a tie with
    source 1 that keeps the caller's order.  Source 3 holds {5, 15} with k = 2 (full: t = 15):
    tau = 15, examined 1 (the key 10), shared 0."""
    need = blob_of_keys(range(10, 90, 10), 8)
    sources = [blob_of_keys([10, 20, 30, 40], 4), blob_of_keys([10, 30, 50, 70, 90], 8),
               blob_of_keys([20, 40, 60, 80, 85, 95], 16), blob_of_keys([5, 15], 2)]
    want = [(0, 4, 4), (1, 4, 8), (2, 4, 8), (3, 0, 1)]
    assert sketch_restate.rank(need, sources) == (None, want, 0)
    assert raw_rank(need, sources) == (0, want, 0)
    # the tie the other way round: still the caller's order
    swapped = [sources[2], sources[1], sources[0]]
    assert raw_rank(need, swapped) == (0, [(2, 4, 4), (0, 4, 8), (1, 4, 8)], 0)


def test_rank_equals_the_restatement():
    import ciruela_amd as ca
    base = sketch_cases.random_digests(3000, 21)
    need_index = sketch_cases.index_of(base)
    for need_k, src_k in ((1024, 1024), (256, 4096), (4096, 64), (64, 64)):
        need = ca.index_sketch(need_index, None, need_k)
        sources = []
        for i, share in enumerate((0, 300, 1500, 2900, 3000)):
            own = sketch_cases.random_digests(3000 - share, 100 + i)
            sources.append(ca.index_sketch(sketch_cases.index_of(base[:share] + own), None, src_k))
        # a source that is not full: tau = 2^64 - 1 on its side, the exact containment
        small = base[:40] + sketch_cases.random_digests(10, 7)
        sources.append(ca.index_sketch(sketch_cases.index_of(small), None, 4096))
        err, want, skipped = sketch_restate.rank(need, sources)
        assert err is None and raw_rank(need, sources) == (0, want, skipped)
        assert len(want) == 6
        skip = []
        assert ca.sketch_rank(need, sources, skip) == want and skip == [0]
    # neither sketch full: shared / examined is the containment itself
    need = ca.index_sketch(sketch_cases.index_of(base[:100]), None, 4096)
    src = ca.index_sketch(sketch_cases.index_of(small), None, 4096)
    assert raw_rank(need, [src]) == (0, [(0, 40, 100)], 0)


def test_rank_skips_and_errors():
    import ciruela_amd as ca
    d = sketch_cases.random_digests(200, 3)
    need = ca.index_sketch(sketch_cases.index_of(d), None, 64)
    good = ca.index_sketch(sketch_cases.index_of(d[:100]), None, 64)
    other_hash = ca.index_sketch(sketch_cases.index_of(d, hash_name="sha512/256"), None, 64)
    other_bs = ca.index_sketch(sketch_cases.index_of(d, bs=128), None, 64)
    bad = [good[:39], good[:-1], good + b"\0", b"CIRSKv2\0" + good[8:],
           good[:12] + struct.pack("<I", 0) + good[16:],            # k = 0
           good[:12] + struct.pack("<I", 4097) + good[16:],         # k > 4096
           good[:12] + struct.pack("<I", 63) + good[16:],           # count > k
           good[:24] + struct.pack("<Q", 63) + good[32:],           # count > n_blocks
           sketch_restate.blob(1, 64, 64, 10, [1, 2, 2, 3]),        # equal neighbours
           sketch_restate.blob(1, 64, 64, 10, [1, 3, 2]),           # descending keys
           sketch_cases.index_of(d)]                                # an index is no sketch
    sources = [good, None, other_hash, other_bs] + bad + [good]
    err, want, skipped = sketch_restate.rank(need, sources)
    assert err is None and skipped == 3 + len(bad) and [r[0] for r in want] == [0, len(sources) - 1]
    assert raw_rank(need, sources) == (0, want, skipped)
    assert raw_rank(need, []) == (0, [], 0)
    for broken in bad:
        rc, rows, sk = raw_rank(broken, [good])
        assert rc == _native.CIR_EPARSE and rows == [] and sk == 0
        assert sketch_restate.rank(broken, [good])[0] == "EPARSE"
    lib = _native.lib
    assert lib.cir_sketch_rank(None, 0, None, None, 0, None, None, None, None, None) == \
        _native.CIR_EINVAL
    n = ctypes.c_size_t()
    assert lib.cir_sketch_rank(need, len(need), None, None, 1, None, None, None, ctypes.byref(n),
                               None) == _native.CIR_EINVAL


# ---- the argument checks of the device-resident call -----------------------------------------

def test_sketch_digests_dev_argument_checks():
    lib = _native.lib
    work = lib.cir_sketch_work_bytes(1000, 64)
    assert work == lib.cir_sketch_work_bytes(1000, 4096) > 8 * 2 * 1000     # pure, k-free
    assert lib.cir_sketch_work_bytes(0, 1) > 0
    ok = dict(dig=1 << 20, n=1000, k=64, keys=1 << 21, work=1 << 22, wb=work, res=1 << 23,
              stream=None)
    order = tuple(ok)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_sketch_digests_dev(None, *[a[k] for k in order])
    for null in ("dig", "keys", "work", "res"):
        assert call(**{null: None}) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    assert call(dig=ok["dig"] + 8) == _native.CIR_EINVAL
    assert b"16-byte aligned" in lib.cir_last_error()
    for odd in ("keys", "work", "res"):
        assert call(**{odd: ok[odd] + 4}) == _native.CIR_EINVAL, odd
        assert b"8-byte aligned" in lib.cir_last_error()
    for k in (0, 4097):
        assert call(k=k) == _native.CIR_EINVAL
        assert b"k must be" in lib.cir_last_error()
    assert call(n=1 << 32, wb=1 << 62) == _native.CIR_EINVAL
    assert b"2^32-1" in lib.cir_last_error()
    assert call(wb=work - 1) == _native.CIR_EINVAL
    assert b"work_bytes" in lib.cir_last_error()
    assert call(n=2000) == _native.CIR_EINVAL           # (the scratch of 1000 digests)


# ---- the CLI ---------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "bin", "ciruela-index")


def test_cli_usage_lists_sketch_and_rank():
    p = subprocess.run([CLI], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index sketch INDEX [-k N] [-o FILE] [--host]" in p.stderr
    assert b"ciruela-index rank NEED SRC [SRC ...]" in p.stderr
    for args in (["sketch"], ["rank", "/tmp/x"], ["sketch", "a", "b"], ["sketch", "a", "-k", "0"],
                 ["sketch", "a", "-k", "5000"]):
        p = subprocess.run([CLI] + args, capture_output=True)
        assert p.returncode == 2, args


def test_cli_sketch_and_rank_on_the_host(tmp_path):
    base = sketch_cases.random_digests(500, 31)
    texts = [sketch_cases.index_of(base)] + \
        [sketch_cases.index_of(base[:n] + sketch_cases.random_digests(500 - n, 40 + n))
         for n in (50, 450, 250)]
    paths = []
    for i, t in enumerate(texts):
        (tmp_path / ("i%d.ds1" % i)).write_bytes(t)
        paths.append(str(tmp_path / ("i%d.ds1" % i)))
    out = str(tmp_path / "need.sk")
    p = subprocess.run([CLI, "sketch", paths[0], "-k", "128", "-o", out, "--host"],
                       capture_output=True)
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    assert b"sketched on the host" in p.stderr
    assert open(out, "rb").read() == sketch_restate.sketch(texts[0], 128)
    p = subprocess.run([CLI, "sketch", paths[1], "--host"], capture_output=True)
    assert p.returncode == 0 and p.stdout == sketch_restate.sketch(texts[1], 1024)
    (tmp_path / "s1.sk").write_bytes(p.stdout)
    # a sketch file and index files mixed; garbage is left out
    (tmp_path / "junk").write_bytes(b"neither\n")
    args = [out, str(tmp_path / "s1.sk"), paths[2], str(tmp_path / "junk"), paths[3]]
    p = subprocess.run([CLI, "rank"] + args + ["-k", "128", "--host"], capture_output=True)
    assert p.returncode == 0, p.stderr
    blobs = [sketch_restate.sketch(texts[0], 128), sketch_restate.sketch(texts[1], 1024),
             sketch_restate.sketch(texts[2], 128), None, sketch_restate.sketch(texts[3], 128)]
    _, want, skipped = sketch_restate.rank(blobs[0], blobs[1:])
    assert [w[0] for w in want] == [1, 3, 0] and skipped == 1
    assert p.stdout.decode().splitlines() == \
        ["%d %d %d %s" % (o, sh, ex, args[1 + o]) for o, sh, ex in want]
    assert b"3 source(s) ranked, 1 left out" in p.stderr
    p = subprocess.run([CLI, "rank", str(tmp_path / "junk"), out, "--host"], capture_output=True)
    assert p.returncode == 2


# ---- the rule header under the sanitizers ---------------------------------------------------

def test_sketch_fuzz_under_asan_ubsan(tmp_path):
    """tools/sketch_fuzz.cpp: a few thousand seeded random cases; the key, the
    host bottom-k, encode, validate, overlap and rank against one-at-a-time
    restatements, malformed blobs included, every blob in a heap buffer of
    exactly its size.  A compile failure fails the test."""
    exe = str(tmp_path / "sketch_fuzz")
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "ciruela_amd", "csrc")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tools", "sketch_fuzz.cpp"),
                        os.path.join(csrc, "dirsig.cpp"), "-o", exe], capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "2000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"sketch_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 2000
    m = re.search(rb"(\d+) blocks; (\d+) full and (\d+) partial sketches; (\d+) ranked, (\d+) left "
                  rb"out, (\d+) ties; (\d+) malformed blobs rejected", p.stderr)
    assert m and all(int(g) > 100 for g in m.groups()), p.stderr


# ---- the kernels' resources ---------------------------------------------------------------

@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_kernel_resources(tmp_path):
    """The four kernels of sketch.hip off the code object: one symbol each, no
    spill and no scratch; LDS only where the design has it (the scan's wave
    sums and its workgroup vote, some hundred bytes; the sort's 64 KiB)."""
    res = codeobj.resources(str(tmp_path))
    lds = {"k_sketch_insert": (0, 0), "k_sketch_scan": (64, 1024), "k_sketch_compact": (0, 0),
           "k_sketch_sort": (65536, 65536)}
    for name in KERNELS:
        hits = codeobj.find(res, name)
        assert len(hits) == 1, (name, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["private_segment_fixed_size"] == 0, name
        assert lds[name][0] <= k["group_segment_fixed_size"] <= lds[name][1], name
