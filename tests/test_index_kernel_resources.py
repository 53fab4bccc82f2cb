"""Resources of the four kernels of cir_index_digests_dev
(ciruela_amd/csrc/idxscan.hip), from the built code object (CPU): all four are
there, none spills a register, and only the three that scan across a workgroup
use LDS -- a few words of it."""
import pytest

import codeobj

pytestmark = pytest.mark.skipif(not codeobj.available(),
                                reason="needs the built library and ROCm's llvm-readelf")

KERNELS = ("k_idx_count", "k_idx_scan", "k_idx_emit", "k_idx_decode")


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    return codeobj.resources(str(tmp_path_factory.mktemp("co")))


@pytest.mark.parametrize("short", KERNELS)
def test_present_and_unspilled(res, short):
    hits = codeobj.find(res, short)
    assert len(hits) == 1, (short, list(hits))
    (k,) = hits.values()
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, k


def test_lds_use(res):
    """The scans keep one pair of u64 per wave (and a spare); the decode is a
    plain loop over global memory."""
    for short in KERNELS[:3]:
        (k,) = codeobj.find(res, short).values()
        assert 0 < k["group_segment_fixed_size"] <= 128, (short, k)
    (k,) = codeobj.find(res, "k_idx_decode").values()
    assert k["group_segment_fixed_size"] == 0, k


def test_text_is_read_and_digests_are_stored_wide(tmp_path):
    """A lane of the count and emit passes reads its 16 bytes of text with one
    global_load_dwordx4 per walk of its span (the source's two 8-byte loads,
    merged; the emit pass walks twice: to count, then to write); a lane of the
    decode reads its 16 hex digits with one global_load_dwordx4 at whatever
    alignment they have and stores its 8 bytes with one global_store_dwordx2.
    A compiler or source change that splits them into narrower accesses fails
    here instead of showing up as a slower parse."""
    table = codeobj.disassembly(str(tmp_path))

    def ops(short):
        (body,) = codeobj.find(table, short).values()
        return [ins.split()[0] for ins in body]
    for short, walks in (("k_idx_count", 1), ("k_idx_emit", 2)):
        assert ops(short).count("global_load_dwordx4") == walks, short
        assert ops(short).count("global_load_dwordx2") == 0, short
    dec = ops("k_idx_decode")
    assert dec.count("global_load_dwordx4") == 1 and dec.count("global_store_dwordx2") == 1
    assert not any(o.startswith(("scratch_", "ds_")) for o in dec)
