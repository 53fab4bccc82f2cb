"""cir_check_links_at on the GPU: cir_check_links' verify of a hardlink
candidate at the path where the source holds it (what cir_file_copies
returns), not at the entry's own.

No expected value comes from the code under test: indexes are
dirsig_oracle.scan's, the candidates are copies_restate's (the rule in plain
Python), the verdicts are links_restate._one's -- try_hardlink
(src/daemon/disk/public.rs:308-346) restated with os.stat(dir_fd=...,
follow_symlinks=False) component by component and hashlib digests -- applied to
the entry with the candidate's path in place of its own.  Trees live on
tmp_path, block size 4096, files of 1 to 5 blocks.
"""
import ctypes
import errno
import os
import random
import subprocess

import pytest

from conftest import ROOT

import copies_restate
import dirsig_oracle
import links_restate
from links_restate import CHECKSUM, OK, READ

pytestmark = pytest.mark.gpu

BS = 4096
KINDS = {0: OK, 1: CHECKSUM, 2: READ}
FILES = {"bin/run": (4096 * 2 + 17, 0o755), "lib/a.so": (4096 * 3, 0o644), "lib/b.so": (4096 + 1, 0o644),
         "lib/deep/c": (4096 * 5, 0o644), "one": (4096, 0o644), "tail": (5, 0o644),
         "sp ace": (4096 * 4 - 1, 0o644)}


@pytest.fixture(scope="module")
def ctx(gpu):
    return gpu.Context(device_mask=1, staging_bytes=64 << 10)


def make_tree(root, sub, seed=1):
    """FILES below root/sub, and root/keep beside it; the bytes depend on the
    name and the seed alone, so two trees with two `sub`s hold equal files."""
    for rel, (size, mode) in list(FILES.items()) + [("../keep", (4096 * 2, 0o644))]:
        p = os.path.normpath(os.path.join(root, sub, rel))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(random.Random("%s/%d" % (rel, seed)).randbytes(size))
        os.chmod(p, mode)
    return str(root)


@pytest.fixture()
def trees(tmp_path):
    """(new index, old index, old root): the directory app-1 became app-2."""
    new = make_tree(tmp_path / "new", "app-2")
    old = make_tree(tmp_path / "old", "app-1")
    return dirsig_oracle.scan(new, BS), dirsig_oracle.scan(old, BS), old


def candidates(new_idx, old_idx, skip=None):
    want, _ = copies_restate.expected_copies(new_idx, [old_idx], skip)
    return [(f, s) for f, s, _, _ in want], [p for _, _, _, p in want]


def expected_at(index, roots, links, paths):
    """The restatement's verdicts with each candidate looked for at its path
    (b"": the entry's own)."""
    hash_name, bs = links_restate._header(index)
    files = links_restate.file_entries(index)
    out = []
    for (f, s), p in zip(links, paths):
        path, exe, size, digests = files[f]
        out.append(links_restate._one(os.fsencode(str(roots[s])), hash_name, bs,
                                      (p or path, exe, size, digests)))
    return out


def test_renamed_directory_all_ok(gpu, ctx, trees):
    new_idx, old_idx, old = trees
    links, paths = candidates(new_idx, old_idx)
    assert len(links) == 8 and sum(p.startswith(b"/app-1/") for p in paths) == 7
    # the host rule names the same candidates (it is tested against the restatement elsewhere)
    found, _ = gpu.file_copies(new_idx, [old_idx])
    assert [(f, s) for f, s, _, _ in found] == links and [p for _, _, _, p in found] == paths
    res = ctx.check_links_at(new_idx, [old], links, paths)
    want = expected_at(new_idx, [old], links, paths)
    assert [k for k, _ in want] == [OK] * 8
    assert links_restate.same_verdicts(res, want), (res.kinds, res.errnos)
    assert res.stats["ok"] == 8 and res.stats["blocks"] == sum(
        (size + BS - 1) // BS for size, _ in FILES.values()) + 2
    # at the entries' own paths the moved files are not there
    own = ctx.check_links(new_idx, [old], links)
    assert own.kinds.count(READ) == 7 and own.kinds.count(OK) == 1
    # a directory fd as the root, and the module-level call
    fd = os.open(old, os.O_RDONLY | os.O_DIRECTORY)
    try:
        assert gpu.check_links_at(new_idx, [fd], links, paths, context=ctx).kinds == [OK] * 8
    finally:
        os.close(fd)


def test_bad_candidates_stay_on_their_own(gpu, ctx, trees):
    new_idx, old_idx, old = trees
    links, paths = candidates(new_idx, old_idx)
    by_path = {p: i for i, p in enumerate(paths)}
    a = os.path.join(old, "app-1", "lib", "a.so")
    data = bytearray(open(a, "rb").read())
    data[4096 + 5] ^= 1
    open(a, "wb").write(data)                                    # a flipped byte: CHECKSUM
    os.remove(os.path.join(old, "app-1", "lib", "b.so"))         # removed: READ, ENOENT
    os.chmod(os.path.join(old, "app-1", "one"), 0o600)           # another mode: CHECKSUM
    os.rename(os.path.join(old, "app-1", "bin"), os.path.join(old, "realbin"))
    os.symlink("../realbin", os.path.join(old, "app-1", "bin"))  # a symlinked component: READ
    res = ctx.check_links_at(new_idx, [old], links, paths)
    want = expected_at(new_idx, [old], links, paths)
    assert links_restate.same_verdicts(res, want), (res.kinds, res.errnos, want)
    got = {p: (res.kinds[i], res.errnos[i]) for p, i in by_path.items()}
    assert got[b"/app-1/lib/a.so"] == (CHECKSUM, 0)
    assert got[b"/app-1/lib/b.so"] == (READ, errno.ENOENT)
    assert got[b"/app-1/one"] == (CHECKSUM, 0)
    assert got[b"/app-1/bin/run"][0] == READ and got[b"/app-1/bin/run"][1] != 0
    for p in (b"/keep", b"/app-1/lib/deep/c", b"/app-1/tail", b"/app-1/sp ace"):
        assert got[p] == (OK, 0), p
    assert (res.stats["ok"], res.stats["checksum"], res.stats["read"]) == (4, 2, 2)
    # the same candidates in another order, twice each: the same verdict per candidate
    order = list(range(len(links))) * 2
    random.Random(5).shuffle(order)
    again = ctx.check_links_at(new_idx, [old], [links[i] for i in order], [paths[i] for i in order])
    assert again.kinds == [res.kinds[i] for i in order]
    assert again.errnos == [res.errnos[i] for i in order]


def test_empty_paths_and_null_are_check_links(gpu, ctx, tmp_path):
    """Same-path candidates, some of them bad: empty paths and paths = None give
    exactly cir_check_links' verdicts, errnos and stats."""
    new = make_tree(tmp_path / "new", "app")
    old0 = make_tree(tmp_path / "old0", "app")
    old1 = make_tree(tmp_path / "old1", "app")
    os.remove(os.path.join(old0, "app", "one"))
    os.chmod(os.path.join(old1, "app", "lib", "a.so"), 0o600)
    with open(os.path.join(old0, "app", "lib", "deep", "c"), "r+b") as f:
        f.seek(4096 * 4 + 9)
        f.write(b"\xff")
    new_idx = dirsig_oracle.scan(new, BS)
    n = len(links_restate.file_entries(new_idx))
    links = [(f, s) for s in (1, 0) for f in range(n)]
    base = ctx.check_links(new_idx, [old0, old1], links)
    assert links_restate.same_verdicts(base, links_restate.expected_verdicts(new_idx, [old0, old1], links))
    assert base.kinds.count(OK) == 2 * n - 3
    for paths in (None, [b""] * len(links)):
        res = ctx.check_links_at(new_idx, [old0, old1], links, paths)
        assert (res.kinds, res.errnos) == (base.kinds, base.errnos)
        assert {k: v for k, v in res.stats.items() if k != "peak_fds"} == \
            {k: v for k, v in base.stats.items() if k != "peak_fds"}
    # an own path spelled out is the same place as the empty one
    files = links_restate.file_entries(new_idx)
    spelled = ctx.check_links_at(new_idx, [old0, old1], links, [files[f][0] for f, _ in links])
    assert (spelled.kinds, spelled.errnos) == (base.kinds, base.errnos)
    # ... with any number of slashes, and without the leading one
    odd = ctx.check_links_at(new_idx, [old0, old1], links,
                             [files[f][0].replace(b"/", b"//")[1:] + b"/" for f, _ in links])
    assert odd.kinds == base.kinds


def raw_at(gpu, ctx, index, root, links, paths):
    """cir_check_links_at through ctypes: (status, kinds, errnos, stats)."""
    lib = gpu._n.lib
    n = len(links)
    fds = (ctypes.c_int * 1)(-100)
    dirs = (ctypes.c_char_p * 1)(os.fsencode(root))
    lf = (ctypes.c_uint64 * n)(*[f for f, _ in links])
    ls = (ctypes.c_uint32 * n)(*[s for _, s in links])
    acc = [0]
    for p in paths:
        acc.append(acc[-1] + len(p))
    offs = (ctypes.c_uint64 * (n + 1))(*acc)
    blob = ctypes.create_string_buffer(b"".join(paths), max(acc[-1], 1))
    kinds = (ctypes.c_uint8 * n)(*([9] * n))
    errnos = (ctypes.c_int32 * n)()
    stats = (ctypes.c_uint64 * 8)(*([99] * 8))
    rc = lib.cir_check_links_at(ctx.handle, index, len(index), fds, dirs, 1, lf, ls, offs,
                                ctypes.cast(blob, ctypes.c_void_p), n, 0, kinds, errnos, stats)
    return rc, list(kinds), list(errnos), list(stats)


@pytest.mark.parametrize("bad", [b"/app-1/../app-1/one", b"..", b"/app-1/./one", b".", b"/", b"///",
                                 b"/app-1/lib/..", b"../../etc/passwd"])
def test_invalid_paths_fail_the_call_before_any_io(gpu, ctx, trees, bad):
    new_idx, old_idx, old = trees
    links, paths = candidates(new_idx, old_idx)
    k = paths.index(b"/app-1/one")
    rc, kinds, _, stats = raw_at(gpu, ctx, new_idx, old, links, paths[:k] + [bad] + paths[k + 1:])
    assert rc == gpu._n.CIR_EINVAL
    assert stats[6] == 0 and stats == [0] * 8       # no file was opened
    assert kinds == [9] * len(links)                # and no verdict written
    with pytest.raises(gpu.CiruelaError) as e:
        ctx.check_links_at(new_idx, [old], links, paths[:k] + [bad] + paths[k + 1:])
    assert e.value.status == gpu._n.CIR_EINVAL


def test_names_that_only_look_like_dots_are_paths(gpu, ctx, trees):
    new_idx, old_idx, old = trees
    links, paths = candidates(new_idx, old_idx)
    k = paths.index(b"/app-1/one")
    for name in (b"...", b".hidden", b"..a"):
        res = ctx.check_links_at(new_idx, [old], links, paths[:k] + [b"/app-1/" + name] + paths[k + 1:])
        assert res.kinds[k] == READ and res.errnos[k] == errno.ENOENT
        assert res.kinds[:k] + res.kinds[k + 1:] == [OK] * 7


def test_nul_in_a_component_is_that_candidates_read_error(gpu, ctx, trees):
    new_idx, old_idx, old = trees
    links, paths = candidates(new_idx, old_idx)
    k = paths.index(b"/app-1/lib/a.so")
    for bad in (b"/app-1/lib/a.so\x00", b"/app-1/l\x00ib/a.so", b"\x00"):
        rc, kinds, errnos, stats = raw_at(gpu, ctx, new_idx, old, links,
                                          paths[:k] + [bad] + paths[k + 1:])
        assert rc == 0
        assert kinds[k] == 2 and errnos[k] == errno.EINVAL
        assert kinds[:k] + kinds[k + 1:] == [0] * 7 and errnos[:k] + errnos[k + 1:] == [0] * 7
        assert stats[:3] == [7, 0, 1]


def test_expected_content_is_the_entrys(gpu, ctx, trees):
    """The file at the given path must have the size, the digests and the mode
    of entry link_file[i]: another entry's file there is CHECKSUM."""
    new_idx, old_idx, old = trees
    files = links_restate.file_entries(new_idx)
    f_a = next(i for i, e in enumerate(files) if e[0] == b"/app-2/lib/a.so")
    f_run = next(i for i, e in enumerate(files) if e[0] == b"/app-2/bin/run")
    links = [(f_a, 0), (f_a, 0), (f_run, 0), (f_run, 0)]
    paths = [b"/app-1/lib/a.so", b"/app-1/lib/deep/c", b"/app-1/bin/run", b"/app-1/lib/a.so"]
    res = ctx.check_links_at(new_idx, [old], links, paths)
    assert links_restate.same_verdicts(res, expected_at(new_idx, [old], links, paths))
    assert res.kinds == [OK, CHECKSUM, OK, CHECKSUM]
    # equal size, other bytes: the digests decide
    other = os.path.join(old, "app-1", "lib", "same-size")
    with open(other, "wb") as f:
        f.write(random.Random(9).randbytes(4096 * 3))
    os.chmod(other, 0o644)
    res = ctx.check_links_at(new_idx, [old], [(f_a, 0)], [b"/app-1/lib/same-size"])
    assert res.kinds == [CHECKSUM]


def test_cli_links_any_path(gpu, trees, tmp_path):
    cli = os.path.join(ROOT, "bin", "ciruela-index")
    new_idx, old_idx, old = trees
    (tmp_path / "new.ds1").write_bytes(new_idx)
    (tmp_path / "old.ds1").write_bytes(old_idx)
    args = [cli, "links", str(tmp_path / "new.ds1"), "%s=%s" % (old, tmp_path / "old.ds1")]
    plain = subprocess.run(args, capture_output=True, timeout=300)
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert plain.stdout == os.fsencode(old) + b"\t/keep\n"
    assert b"links: 1 candidates: 1 ok, 0 checksum, 0 read" in plain.stderr
    outs = []
    for extra in ([], ["--host"]):
        p = subprocess.run(args + ["--any-path"] + extra, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append(p.stdout)
        assert b"links: 8 candidates (1 at their own path, 7 by content): 8 ok, 0 checksum, 0 read" \
            in p.stderr
    assert outs[0] == outs[1]
    lines = outs[0].split(b"\n")[:-1]
    assert lines[0] == os.fsencode(old) + b"\t/keep"
    files = links_restate.file_entries(new_idx)
    _, paths = candidates(new_idx, old_idx, skip=[i for i, e in enumerate(files) if e[0] == b"/keep"])
    got = [tuple(links_restate.unescape(x) for x in l.split(b"\t")[1:]) for l in lines[1:]]
    assert [g[1] for g in got] == paths and len(got) == 7
    assert all(a.replace(b"/app-2/", b"/app-1/") == b for a, b in got)
