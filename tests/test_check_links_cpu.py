"""cir_link_candidates / cir_check_links / cir_verify_segments_dev without a
GPU: the declarations in the header, the ctypes table and INTEGRATION.md's
extern block, the argument checks that need no device, k_seg_bad's resources
in the built code object, the CLI's usage text -- and cir_link_candidates
(host only) against a Python restatement of scan_links.

Reference: scan_links (src/daemon/metadata/hardlink_sources.rs:107-153) and
check_and_hardlink / try_hardlink (src/daemon/disk/public.rs:285-346).  No
expected value comes from the library: indexes are built with
dirsig_oracle.emit / scan, digests are hashlib's, and the expected candidates
are links_restate.expected_candidates over dirsig_oracle.parse.
"""
import ctypes
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

import codeobj
import dirsig_oracle
import links_restate
from ciruela_amd import _native

NEW = ("cir_verify_segments_dev", "cir_link_candidates", "cir_check_links")


# ---- declarations and bindings ------------------------------------------------

def _header():
    text = open(os.path.join(ROOT, "include", "ciruela_blockhash.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_all_three():
    text = _header()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
    assert re.search(r"#define CIR_LINKS_STATS_FIELDS 8\b", text)


def test_ctypes_table_binds_all_three():
    for name in NEW:
        assert name in _native._SIGS
        assert getattr(_native.lib, name).restype is ctypes.c_int
    assert len(_native._SIGS["cir_verify_segments_dev"][1]) == 14
    assert len(_native._SIGS["cir_link_candidates"][1]) == 9
    assert len(_native._SIGS["cir_check_links"][1]) == 13
    assert _native.CIR_LINKS_STATS_FIELDS == 8


def test_integration_extern_block_names_all_three():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text[text.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = set(re.findall(r"pub fn (cir_[a-z0-9_]+)\(", block))
    assert set(NEW) <= bound


def test_python_interface_exists():
    import ciruela_amd as ca
    assert callable(ca.link_candidates) and callable(ca.check_links)
    assert callable(ca.Context.check_links) and callable(ca.Context.verify_segments_dev)
    for name in ("link_candidates", "check_links", "LinksResult"):
        assert name in ca.__all__
    assert "src/daemon/disk/public.rs:285-346" in ca.__doc__
    assert "src/daemon/metadata/hardlink_sources.rs:107-153" in ca.__doc__
    index = dirsig_oracle.emit("blake2b/256", 4096, [
        (b"/", [("f", b"a b", False, 0, []), ("s", b"l", b"a b"), ("f", b"z", True, 0, [])]),
        (b"/d", [("f", b"q\\r", False, 0, [])])])
    r = ca.LinksResult(index, [(0, 0), (2, 1), (1, 0)], [0, 1, 2], [0, 0, 2],
                       dict(zip(ca.Context.LINKS_STATS_FIELDS, [1, 1, 1, 0, 0, 0, 3, 3])))
    assert r.kinds == ["ok", "checksum", "read"] and r.errnos == [0, 0, 2]
    assert r.ok_paths == {b"/a b"}
    assert r.stats["peak_fds"] == 3
    r = ca.LinksResult(index, [(2, 0)], [0], [0], {})
    assert r.ok_paths == {b"/d/q\\r"}


INDEX = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  a f 0\n  b f 0\n" + b"ab" * 32 + b"\n")


def _links_args(**kw):
    a = dict(ctx=ctypes.c_void_p(16),  # never dereferenced before the argument checks
             index=INDEX, len=len(INDEX),
             fds=(ctypes.c_int * 2)(-100, -100),
             dirs=(ctypes.c_char_p * 2)(b"/nonexistent/a", b"/nonexistent/b"), nsrc=2,
             lf=(ctypes.c_uint64 * 2)(0, 1), ls=(ctypes.c_uint32 * 2)(0, 1), n=2, threads=0,
             kinds=(ctypes.c_uint8 * 2)(), errnos=(ctypes.c_int32 * 2)(),
             stats=(ctypes.c_uint64 * 8)())
    a.update(kw)
    return [a[k] for k in ("ctx", "index", "len", "fds", "dirs", "nsrc", "lf", "ls", "n",
                           "threads", "kinds", "errnos", "stats")]


def test_check_links_argument_checks():
    """CIR_EINVAL before any I/O and before the context is touched: the roots
    named here do not exist and the non-null context is not a context."""
    lib = _native.lib
    assert lib.cir_check_links(*_links_args(ctx=None)) == _native.CIR_EINVAL
    for null in ("index", "fds", "dirs", "lf", "ls", "kinds", "stats"):
        assert lib.cir_check_links(*_links_args(**{null: None})) == _native.CIR_EINVAL, null
        assert b"null" in lib.cir_last_error()
    # a file ordinal past the last file entry (the index has two)
    assert lib.cir_check_links(*_links_args(lf=(ctypes.c_uint64 * 2)(0, 2))) == _native.CIR_EINVAL
    assert b"link_file" in lib.cir_last_error()
    assert lib.cir_check_links(*_links_args(lf=(ctypes.c_uint64 * 2)((1 << 64) - 1, 0))) == \
        _native.CIR_EINVAL
    # a source ordinal past the roots
    assert lib.cir_check_links(*_links_args(ls=(ctypes.c_uint32 * 2)(0, 2))) == _native.CIR_EINVAL
    assert b"link_src" in lib.cir_last_error()
    assert lib.cir_check_links(*_links_args(nsrc=0)) == _native.CIR_EINVAL
    # an index that does not parse, with everything else in order
    assert lib.cir_check_links(*_links_args(index=INDEX[:30], len=30)) == _native.CIR_EPARSE


def test_verify_segments_dev_argument_checks():
    """The CIR_EINVAL cases, all decided before any device call."""
    lib = _native.lib
    u64 = (1 << 64) - 1
    ok = dict(ctx=None, ht=1, arena=4096, arena_bytes=u64, off=4096, ln=4096, n=4, exp=4096,
              dig=8192, seg_end=256, nseg=2, seg_bad=1024, nbad=512, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cir_verify_segments_dev(a["ctx"], a["ht"], a["arena"], a["arena_bytes"],
                                           a["off"], a["ln"], a["n"], a["exp"], a["dig"],
                                           a["seg_end"], a["nseg"], a["seg_bad"], a["nbad"],
                                           a["stream"])
    assert call(seg_end=None) == _native.CIR_EINVAL
    assert b"null" in lib.cir_last_error()
    assert call(seg_bad=None) == _native.CIR_EINVAL
    assert call(nseg=0) == _native.CIR_EINVAL
    assert call(exp=4096 + 8) == _native.CIR_EINVAL
    assert b"16-byte aligned" in lib.cir_last_error()
    assert call(dig=8192 + 4) == _native.CIR_EINVAL
    assert call(exp=None) == _native.CIR_EINVAL
    assert call(dig=None) == _native.CIR_EINVAL
    assert call(seg_end=258) == _native.CIR_EINVAL
    assert call(nbad=514) == _native.CIR_EINVAL
    assert call(ht=9, arena_bytes=1 << 20) == _native.CIR_EINVAL
    assert call(n=1 << 31, arena_bytes=1 << 20) == _native.CIR_EINVAL


@pytest.mark.skipif(not codeobj.available(), reason="needs the built library and llvm-readelf")
def test_seg_bad_kernel_resources(tmp_path):
    """k_seg_bad is k_first_bad's compare (two 16-B loads per operand, a
    ballot) and, in a mismatching lane only, a bisection and one byte store:
    no spill, no scratch, no LDS, no atomic."""
    res = codeobj.resources(str(tmp_path))
    hits = codeobj.find(res, "k_seg_bad")
    assert len(hits) == 1, list(hits)
    (k,) = hits.values()
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] == 0
    assert len(codeobj.find(res, "k_first_bad")) == 1
    body = next(iter(codeobj.find(codeobj.disassembly(str(tmp_path)), "k_seg_bad").values()))
    ops = [ins.split()[0] for ins in body]
    assert sum(o.startswith("global_load_dwordx4") for o in ops) == 4
    assert sum(o.startswith("global_store_byte") for o in ops) == 1
    assert not any(o.startswith(("scratch_", "ds_", "global_atomic")) for o in ops)


def test_cli_usage_lists_links():
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    p = subprocess.run([cli], capture_output=True)
    assert p.returncode == 2
    assert b"ciruela-index links INDEX SRCDIR=SRCINDEX [SRCDIR=SRCINDEX ...]" in p.stderr
    # no source, and a source without its index: usage, exit 2
    for args in (["links", "/tmp/x.ds1"], ["links", "/tmp/x.ds1", "/tmp"]):
        p = subprocess.run([cli] + args, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr


# ---- cir_link_candidates ------------------------------------------------------------

BS = 64


def digests(data, hname="blake2b/256", bs=BS):
    return dirsig_oracle.block_hashes(data, bs, hname)


def entry(name, data, exe=False, hname="blake2b/256", bs=BS):
    return ("f", name, exe, len(data), digests(data, hname, bs))


def emit(dirs, hname="blake2b/256", bs=BS):
    return dirsig_oracle.emit(hname, bs, dirs, keep_empty=True)


def candidates(index, sources):
    import ciruela_amd as ca
    return ca.link_candidates(index, sources)


def skipped(index, sources):
    lib = _native.lib
    bufs = [ctypes.create_string_buffer(s, max(len(s), 1)) for s in sources]
    sp = (ctypes.c_void_p * max(len(sources), 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sl = (ctypes.c_size_t * max(len(sources), 1))(*[len(s) for s in sources])
    f, s, n, sk = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(77)
    assert lib.cir_link_candidates(index, len(index), sp, sl, len(sources), ctypes.byref(f),
                                   ctypes.byref(s), ctypes.byref(n), ctypes.byref(sk)) == 0
    if n.value == 0:
        assert f.value is None and s.value is None
    lib.cir_free(f)
    lib.cir_free(s)
    return sk.value


def agree(index, sources):
    want, want_skipped = links_restate.expected_candidates(index, sources)
    got = candidates(index, sources)
    assert got == want
    assert skipped(index, sources) == want_skipped
    assert [f for f, _ in got] == sorted({f for f, _ in got})  # strictly increasing
    return got


A, B, C = b"a" * 100, b"b" * 64, b"c" * 200

NEW_DIRS = [(b"/", [entry(b"one", A), ("s", b"lnk", b"one"), entry(b"run", B, exe=True),
                    entry(b"zero", b"")]),
            (b"/d", [entry(b"two", C)])]


def test_candidates_first_source_in_the_given_order_wins():
    new = emit(NEW_DIRS)
    old1 = emit([(b"/", [entry(b"one", A)]), (b"/d", [entry(b"two", C)])])
    old2 = emit(NEW_DIRS)
    assert agree(new, [old1, old2]) == [(0, 0), (1, 1), (2, 1), (3, 0)]
    assert agree(new, [old2, old1]) == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert agree(new, [old1]) == [(0, 0), (3, 0)]
    # the same image again: every file from the one source
    assert agree(new, [new]) == [(0, 0), (1, 0), (2, 0), (3, 0)]


def test_candidates_need_equal_exe_size_and_digests():
    new = emit(NEW_DIRS)
    exe_flip = emit([(b"/", [entry(b"one", A, exe=True), entry(b"run", B, exe=False)])])
    assert agree(new, [exe_flip]) == []
    size = emit([(b"/", [entry(b"one", A + b"a")]), (b"/d", [entry(b"two", C[:-1])])])
    assert agree(new, [size]) == []
    # same size, one flipped byte in one digest (of the second block of /d/two)
    d = digests(C)
    d[1] = d[1][:5] + bytes([d[1][5] ^ 1]) + d[1][6:]
    one_byte = emit([(b"/", [entry(b"one", A)]), (b"/d", [("f", b"two", False, len(C), d)])])
    assert agree(new, [one_byte]) == [(0, 0)]
    # the good source behind the bad one still serves the file
    assert agree(new, [one_byte, emit(NEW_DIRS)]) == [(0, 0), (1, 1), (2, 1), (3, 1)]


def test_candidates_symlink_or_directory_at_the_path_does_not_match():
    new = emit(NEW_DIRS)
    old = emit([(b"/", [("s", b"one", b"elsewhere"), entry(b"run", B, exe=True)]),
                (b"/d", []), (b"/d/two", [entry(b"inner", C)])])
    assert agree(new, [old]) == [(1, 0)]
    # a file where the new index has its symlink is no candidate (only files are walked)
    old = emit([(b"/", [entry(b"lnk", A)])])
    assert agree(new, [old]) == []


def test_candidates_skip_sources_that_cannot_take_part():
    new = emit(NEW_DIRS)
    good = emit(NEW_DIRS)
    rng = random.Random(3)
    garbage = rng.randbytes(300)
    cut = good[:len(good) // 2]              # ends inside a line
    assert skipped(new, [garbage, good, cut, b""]) == 3
    assert agree(new, [garbage, good, cut, b""]) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    other_bs = emit([(b"/", [entry(b"one", A, bs=128), entry(b"zero", b"", bs=128)])], bs=128)
    other_hash = emit([(b"/", [entry(b"one", A, hname="sha512/256"),
                               entry(b"zero", b"", hname="sha512/256")])], hname="sha512/256")
    assert skipped(new, [other_bs, other_hash]) == 2
    assert agree(new, [other_bs, other_hash, good]) == [(0, 2), (1, 2), (2, 2), (3, 2)]
    # sha512/256 on both sides matches
    sha_dirs = [(b"/", [entry(b"one", A, hname="sha512/256")])]
    assert agree(emit(sha_dirs, hname="sha512/256"), [good, emit(sha_dirs, hname="sha512/256")]) \
        == [(0, 1)]


def test_candidates_without_sources():
    new = emit(NEW_DIRS)
    assert agree(new, []) == []
    assert skipped(new, []) == 0
    # an index without file entries
    assert agree(emit([(b"/", [("s", b"l", b"t")])]), [new]) == []


def test_candidates_escaped_names():
    dirs = [(b"/", [entry(b"back\\slash", A), entry(b"with space", B)]),
            (b"/sp ace", [entry(b"\xff\x01", C)])]
    new = emit(dirs)
    assert b"back\\x5cslash" in new and b"with\\x20space" in new and b"/sp\\x20ace" in new
    assert agree(new, [emit(dirs[:1]), emit(dirs)]) == [(0, 0), (1, 0), (2, 1)]


def test_candidates_errors():
    lib = _native.lib
    new = emit(NEW_DIRS)
    f, s, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    out = (ctypes.byref(f), ctypes.byref(s), ctypes.byref(n), None)
    assert lib.cir_link_candidates(None, 0, None, None, 0, *out) == _native.CIR_EINVAL
    assert lib.cir_link_candidates(new, len(new), None, None, 1, *out) == _native.CIR_EINVAL
    assert lib.cir_link_candidates(new, len(new), None, None, 0, None, ctypes.byref(s),
                                   ctypes.byref(n), None) == _native.CIR_EINVAL
    assert lib.cir_link_candidates(new, len(new) // 2, None, None, 0, *out) == _native.CIR_EPARSE
    short = (b"DIRSIGNATURE.v1 blake2b/256 block_size=4096\n/\n  f f 10 " + b"ab" * 16 + b"\n" +
             b"ab" * 32 + b"\n")
    assert lib.cir_link_candidates(short, len(short), None, None, 0, *out) in \
        (_native.CIR_EHASHSIZE, _native.CIR_EPARSE)
    # nskipped_out may be NULL, and no sources is fine
    assert lib.cir_link_candidates(new, len(new), None, None, 0, *out) == 0 and n.value == 0


def _random_index(rng, pool, hname, bs):
    """A small synthetic index over a shared pool of (dir, name) places, so
    that independent draws collide in path, and sometimes in content."""
    dirs = {}
    for d, name in rng.sample(pool, rng.randrange(0, len(pool) + 1)):
        kind = rng.random()
        if kind < 0.1:
            e = ("s", name, b"target")
        else:
            data = bytes([rng.randrange(2)]) * rng.choice([0, 1, bs - 1, bs, bs + 1, 3 * bs])
            e = entry(name, data, exe=rng.random() < 0.3, hname=hname, bs=bs)
        dirs.setdefault(d, []).append(e)
    dirs.setdefault(b"/", [])
    return emit([(d, sorted(es, key=lambda e: e[1])) for d, es in sorted(dirs.items())],
                hname=hname, bs=bs)


@pytest.mark.parametrize("seed", range(50))
def test_candidates_random(seed):
    rng = random.Random(seed)
    pool = [(d, n) for d in (b"/", b"/a", b"/a/b", b"/z z") for n in (b"f1", b"f 2", b"f\\3")]
    hname, bs = rng.choice(["blake2b/256", "sha512/256"]), rng.choice([32, 64])
    new = _random_index(rng, pool, hname, bs)
    sources = []
    for _ in range(rng.randrange(0, 6)):
        r = rng.random()
        if r < 0.1:
            sources.append(rng.randbytes(rng.randrange(0, 200)))
        elif r < 0.2:
            sources.append(_random_index(rng, pool, hname, 96))
        elif r < 0.3:
            sources.append(new)
        else:
            sources.append(_random_index(rng, pool, hname, bs))
    agree(new, sources)
