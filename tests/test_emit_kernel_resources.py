"""The two kernels of ciruela_amd/csrc/emit.hip off the built code object
(CPU only, through tests/codeobj.py): present once each, no spill, no private
segment, no LDS; k_emit_text stores its 16 bytes with exactly one dwordx4
store and has no narrower global store, so no lane can write a part of
another lane's bytes."""
import pytest

import codeobj

pytestmark = pytest.mark.skipif(not codeobj.available(),
                                reason="needs the built library and llvm-objdump")

KERNELS = ("k_emit_text", "k_mem_desc")


def test_kernel_resources(tmp_path):
    res = codeobj.resources(str(tmp_path))
    for name in KERNELS:
        hits = codeobj.find(res, name)
        assert len(hits) == 1, (name, list(hits))
        (k,) = hits.values()
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
        assert k["private_segment_fixed_size"] == 0, name
        assert k["group_segment_fixed_size"] == 0, name


def test_emit_text_stores_once(tmp_path):
    dis = codeobj.disassembly(str(tmp_path))
    hits = codeobj.find(dis, "k_emit_text")
    assert len(hits) == 1, list(hits)
    (body,) = hits.values()
    ops = [ins.split()[0] for ins in body]
    stores = [op for op in ops if "store" in op]
    assert stores == ["global_store_dwordx4"], stores
    assert not [op for op in ops if op.startswith(("scratch_", "ds_", "buffer_"))]
    # the bad-piece count: one atomic per wave, and nothing else writes
    assert [op for op in ops if "atomic" in op] == ["global_atomic_add_x2"]


def test_mem_desc_stores_one_descriptor(tmp_path):
    dis = codeobj.disassembly(str(tmp_path))
    (body,) = codeobj.find(dis, "k_mem_desc").values()
    stores = sorted(ins.split()[0] for ins in body if "store" in ins.split()[0])
    assert stores == ["global_store_dword", "global_store_dwordx2"], stores
