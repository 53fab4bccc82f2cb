"""Barrier discipline of k_chunks, from the built code object (CPU).

k_chunks keeps the waves of a workgroup in phase with one s_barrier at the
entry of every fast group of the compression (uniform.hpp PhaseBarrier,
DESIGN.md 4.1).  A wave that meets fewer barriers than its neighbours hangs
the workgroup, so the shape that makes the count equal by construction is
pinned here: every barrier sits in one of the two line loops (full wave and
partial wave, which can share a workgroup), every way through one iteration
of either loop crosses the same number of them, and both loops run on scalar
conditions only (the trip count is the kernel argument `lines`).

The compiler lays the loops out rotated (entered in the middle, left from the
middle), so the loops are walked as control-flow graphs, not as address
ranges with one branch at the bottom."""
import pytest

import codeobj

pytestmark = pytest.mark.skipif(not codeobj.available(),
                                reason="needs the built library and ROCm's llvm-readelf")

# 12 rounds x 2 half rounds x 4 fast groups
BARRIERS_PER_COMPRESSION = 96
SCALAR_BRANCHES = ("s_cbranch_scc0", "s_cbranch_scc1", "s_branch")


class Kernel:
    def __init__(self, body):
        self.ops = [ins.split()[0] for _, ins in body]
        at = {a: i for i, (a, _) in enumerate(body)}
        self.target = {}
        for i, (a, ins) in enumerate(body):
            op = ins.split()
            if op[0].startswith(("s_cbranch", "s_branch")):
                off = int(op[-1])
                off = off - 65536 if off > 32767 else off
                self.target[i] = at[a + 4 + 4 * off]

    def succ(self, i):
        op = self.ops[i]
        if op == "s_endpgm":
            return []
        if op == "s_branch":
            return [self.target[i]]
        if i in self.target:
            return [i + 1, self.target[i]]
        return [i + 1]

    def loops(self):
        """[(head, last)]: the merged address ranges of the backward branches
        that hold a line's eight ds_read_b128."""
        spans = sorted((t, i) for i, t in self.target.items() if t <= i)
        merged = []
        for lo, hi in spans:
            if merged and lo <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], hi)
            else:
                merged.append([lo, hi])
        return [(lo, hi) for lo, hi in merged
                if self.ops[lo:hi + 1].count("ds_read_b128") == 8]

    def walks(self, start, lo, hi):
        """Every way from `start` to the loop head `lo` ("head") or out of
        [lo, hi] ("exit"), with the s_barrier count of each."""
        found = []
        stack = [(start, 0, frozenset())]
        while stack:
            i, n, seen = stack.pop()
            while True:
                assert i not in seen, ("an inner cycle at", i)
                seen = seen | {i}
                if self.ops[i] == "s_barrier":
                    n += 1
                nxt = self.succ(i)
                ends = [("head" if j == lo else "exit", n) for j in nxt
                        if j == lo or not lo <= j <= hi]
                found.extend(ends)
                nxt = [j for j in nxt if j != lo and lo <= j <= hi]
                if not nxt:
                    break
                for j in nxt[1:]:
                    stack.append((j, n, seen))
                i = nxt[0]
        return found

    def entries(self, lo, hi):
        ins = {t for i, t in self.target.items() if lo <= t <= hi and not lo <= i <= hi}
        if lo > 0 and self.ops[lo - 1] not in ("s_branch", "s_endpgm"):
            ins.add(lo)
        return sorted(ins)


@pytest.fixture(scope="module")
def chunks(tmp_path_factory):
    table = codeobj.disassembly(str(tmp_path_factory.mktemp("co")), with_addr=True)
    (body,) = codeobj.find(table, "k_chunks").values()
    return Kernel(body)


def test_two_line_loops_hold_the_same_barriers(chunks):
    """96 in the full-wave loop and 96 in the partial-wave loop, and every way
    once round either loop crosses all 96."""
    loops = chunks.loops()
    assert len(loops) == 2, loops
    for lo, hi in loops:
        assert chunks.ops[lo:hi + 1].count("s_barrier") == BARRIERS_PER_COMPRESSION, (lo, hi)
        round_trip = chunks.walks(lo, lo, hi)
        laps = [n for kind, n in round_trip if kind == "head"]
        assert laps and set(laps) == {BARRIERS_PER_COMPRESSION}, (lo, hi, laps)
        # a wave enters the rotated loop part-way through an iteration and
        # leaves part-way: way in + way out is a whole number of iterations
        outs = [n for kind, n in round_trip if kind == "exit"]
        assert outs, (lo, hi)
        entries = chunks.entries(lo, hi)
        assert entries, (lo, hi)
        for e in entries:
            for kind, n in ([("head", 0)] if e == lo else chunks.walks(e, lo, hi)):
                if kind == "exit":
                    assert n % BARRIERS_PER_COMPRESSION == 0, (lo, hi, e, n)
                else:
                    for m in outs:
                        assert (n + m) % BARRIERS_PER_COMPRESSION == 0, (lo, hi, e, n, m)


def test_line_loops_branch_on_scalar_conditions(chunks):
    """Every branch inside a line loop, the one back to its head included,
    tests SCC (or is unconditional): the trip count and the refill's skip are
    wave-uniform scalars, never a per-lane mask (vccz / execz would be)."""
    for lo, hi in chunks.loops():
        inside = [(i, chunks.ops[i]) for i in range(lo, hi + 1) if i in chunks.target]
        assert any(t == lo for i, t in chunks.target.items() if lo <= i <= hi)
        bad = [(i, op) for i, op in inside if op not in SCALAR_BRANCHES]
        assert not bad, bad


def test_no_barrier_outside_the_line_loops(chunks):
    inside = set()
    for lo, hi in chunks.loops():
        inside.update(range(lo, hi + 1))
    outside = [i for i, op in enumerate(chunks.ops) if op == "s_barrier" and i not in inside]
    assert not outside, outside[:4]
