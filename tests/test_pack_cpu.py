"""The slot layout shared by the scan and the three check pipelines
(ciruela_amd/csrc/pack.hpp: slot sizes, the packing step, the cut into read
pieces, the cursor over block ranges) under AddressSanitizer and UBSan against
a restatement that goes one block at a time (tools/pack_fuzz.cpp, a
stand-alone program).  No GPU and no library: the header is host-only.
"""
import os
import re
import subprocess

from conftest import ROOT


def test_packing_step_and_cursor_under_asan_and_ubsan(tmp_path):
    """tools/pack_fuzz.cpp: a few thousand seeded cases -- files of 0 to 40
    blocks with ragged last blocks, block sizes 1 to 4096, staging below, at
    and above a block, a block count forced small, one to five ranges that
    start and end inside files, ramp on and off -- driven to the end through
    the header's cursor and packing step, every batch compared with the
    tool's own per-block restatement of the rule, in descriptor arrays of
    exactly cap_blk entries.  A compile failure fails the test."""
    exe = str(tmp_path / "pack_fuzz")
    cxx = os.environ.get("CXX", "g++")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ciruela_amd", "csrc"),
                        os.path.join(ROOT, "tools", "pack_fuzz.cpp"), "-o", exe],
                       capture_output=True)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe, "4000", "11"], capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert re.fullmatch(rb"pack_fuzz: \d+ cases ok\n", p.stdout), p.stdout
    assert int(p.stdout.split()[1]) >= 4000
