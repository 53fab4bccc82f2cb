"""Python restatements of the daemon's hardlink step, for the tests of
cir_link_candidates and cir_check_links (no test module: helpers only).

* expected_candidates: scan_links (src/daemon/metadata/hardlink_sources.rs:
  107-153) over dirsig_oracle.parse.
* expected_verdicts: try_hardlink (src/daemon/disk/public.rs:308-346) per
  candidate, with os.stat(dir_fd=..., follow_symlinks=False) component by
  component and hashlib digests (dirsig_oracle.HASHES).
Nothing here calls the library.
"""
import errno
import os
import re
import stat

import dirsig_oracle

OK, CHECKSUM, READ = "ok", "checksum", "read"
_DIR = os.O_RDONLY | os.O_DIRECTORY | os.O_CLOEXEC


def unescape(b):
    return re.sub(rb"\\x([0-9a-f]{2})", lambda m: bytes([int(m.group(1), 16)]), b)


def file_entries(index):
    """[(path, exe, size, [digests])] of the index's file entries, in index
    order: position = file ordinal."""
    _, _, dirs, _ = dirsig_oracle.parse(index)
    out = []
    for vesc, entries in dirs:
        vpath = unescape(vesc)
        for e in entries:
            if e[0] == "f":
                out.append(((b"/" if vpath == b"/" else vpath + b"/") + unescape(e[1]), e[2], e[3],
                            e[4]))
    return out


def _header(index):
    hash_name, bs, _, _ = dirsig_oracle.parse(index)
    return hash_name, bs


def expected_candidates(index, sources):
    """([(file ordinal, source ordinal)], sources skipped)."""
    head = _header(index)
    usable = []
    skipped = 0
    for j, s in enumerate(sources):
        try:
            if _header(s) != head:
                raise ValueError("another hash type or block size")
            table = {}
            for path, exe, size, digests in file_entries(s):
                table.setdefault(path, (exe, size, digests))
        except Exception:
            skipped += 1  # the reference warns and goes on (:95-101)
            continue
        usable.append((j, table))
    out = []
    for f, (path, exe, size, digests) in enumerate(file_entries(index)):
        for j, table in usable:
            if table.get(path) == (exe, size, digests):
                out.append((f, j))
                break
    return out, skipped


def _open_dir_nofollow(rootfd, comps):
    """fd of rootfd/comps..., each component lstat'ed and opened without
    following symlinks; OSError (ENOENT, ENOTDIR) otherwise."""
    fd = os.dup(rootfd)
    try:
        for c in comps:
            st = os.stat(c, dir_fd=fd, follow_symlinks=False)
            if not stat.S_ISDIR(st.st_mode):
                raise OSError(errno.ENOTDIR, "not a directory")
            nfd = os.open(c, _DIR | os.O_NOFOLLOW, dir_fd=fd)
            os.close(fd)
            fd = nfd
    except OSError:
        os.close(fd)
        raise
    return fd


def _one(root, hash_name, bs, entry):
    path, exe, size, digests = entry
    h = dirsig_oracle.HASHES[hash_name]
    comps = [c for c in path.split(b"/") if c]
    try:
        rootfd = os.open(root, _DIR)
    except OSError as e:
        return READ, e.errno
    try:
        try:
            dfd = _open_dir_nofollow(rootfd, comps[:-1])
        except OSError as e:
            return READ, e.errno
        try:
            try:
                st = os.stat(comps[-1], dir_fd=dfd, follow_symlinks=False)
            except OSError as e:
                return READ, e.errno
            if not stat.S_ISREG(st.st_mode):
                return READ, None
            if st.st_size != size:
                return CHECKSUM, 0
            fd = os.open(comps[-1], os.O_RDONLY | os.O_NOFOLLOW, dir_fd=dfd)
            with os.fdopen(fd, "rb") as f:
                data = f.read()
            if [h(data[i:i + bs]) for i in range(0, len(data), bs)] != digests:
                return CHECKSUM, 0
            if st.st_mode & 0o777 != (0o755 if exe else 0o644):
                return CHECKSUM, 0
            return OK, 0
        finally:
            os.close(dfd)
    finally:
        os.close(rootfd)


def expected_verdicts(index, roots, links):
    """[(kind, errno)] per candidate; errno None where the restatement does not
    pin it (a file that is not regular), else the errno of a READ or 0."""
    hash_name, bs = _header(index)
    files = file_entries(index)
    return [_one(os.fsencode(str(roots[s])), hash_name, bs, files[f]) for f, s in links]


def expected_ok_paths(index, roots, links):
    files = file_entries(index)
    return {files[f][0] for (f, _), (kind, _) in zip(links, expected_verdicts(index, roots, links))
            if kind == OK}


def same_verdicts(result, want):
    """Does a LinksResult carry exactly the restatement's verdicts (and its
    errnos wherever the restatement pins them)?"""
    if result.kinds != [k for k, _ in want] or len(result.errnos) != len(want):
        return False
    for got, (k, e) in zip(result.errnos, want):
        if k != READ:
            good = got == 0
        elif e == errno.ENOENT:
            good = got == errno.ENOENT
        else:  # (a symlink in a component's place: ELOOP or ENOTDIR, by the open's flags)
            good = got != 0
        if not good:
            return False
    return True
