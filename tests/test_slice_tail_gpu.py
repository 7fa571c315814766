"""The tail of pglamd_aggregate_sliced and the block schedule of its flat launch: the list counters are zeroed by the hub-table gather,
the flat launch stores finished rows non-temporally, the combine takes two long rows per wave -- rows whose nine rows the flat launch
finished alone ("ready") and rows that wait for a fix-up task ("late") alike -- and an XCD's slice blocks may be packed into the front
of its block sequence (option "slice_front").  None of it may change a bit: every result here is compared exactly -- with the bits the
commit before these changes produced, with a call on a fresh workspace, with the integer sum, with the slice_front = 100 result."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_common import *                        # noqa: F401,F403
import hub_slice_defs as H
import slice_tail_defs as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hub_slices_parent_bits.json")


@pytest.fixture(scope="module")
def indexes(pgl):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = S.device_index(pgl, name)
        return cache[name]
    return get


@pytest.fixture()
def front(pgl):
    """Sets the library's slice_front option; the built-in default is back when the test ends."""
    yield lambda v: pgl.ops.set_option("slice_front", -1 if v is None else v)
    pgl.ops.set_option("slice_front", -1)


_INTS = {}


def _ints(indexes, name, d):
    """(integer-valued features on the device, their exact sum over the graph's own rows): computed once, never written to."""
    if (name, d) not in _INTS:
        _, n, src, dst = indexes(name)
        x = H.small_int_features(n, d, 2000 + d)
        _INTS[name, d] = (dev(x), H.exact_sum(x, src, dst, n))
    return _INTS[name, d]


def _pieces(plan):
    """Chunks every row of the plan's stream is cut into (0 for an empty row, 1 for a row that is not split)."""
    ip = np.asarray(plan.indptr.cpu().numpy(), np.int64)
    lo, hi = ip[:-1], ip[1:]
    return np.where(hi - lo > plan.chunk, (hi - 1) // plan.chunk - lo // plan.chunk + 1, np.minimum(hi - lo, 1))


def _late_rows(plan):
    """[n_long] bool: the long rows with a split piece among their nine rows (the row's remainder and its eight virtual rows)."""
    p = _pieces(plan)
    R, n = plan.n_long, plan.out_rows
    long_rows = plan.long_rows.cpu().numpy()
    late = p[long_rows] > 1
    for s in range(H.SLICES):
        late |= p[n + s * R: n + (s + 1) * R] > 1
    return late


def test_the_golden_file_covers_every_case():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(S.case_id(c) for c in S.BIT_CASES)


@pytest.mark.parametrize("case", S.BIT_CASES, ids=S.case_id)
def test_bits_of_the_parent(pgl, indexes, front, case):
    with open(GOLDEN) as f:
        want = json.load(f)[S.case_id(case)]
    index, n = indexes(case[0])[:2]
    for v in (None,) + S.FRONTS:
        front(v)
        assert S.bits(S.run_case(pgl.ops, index, n, case)[0]) == want, "slice_front = %s" % v


@pytest.mark.parametrize("case", [("rmat14", 8, 128, 32, 0), ("all_hub", 64, 128, 32, 0), ("tiny", 256, 128, 32, 0)], ids=S.case_id)
def test_counters_are_reset_by_the_call_itself(pgl, indexes, case):
    ops = pgl.ops
    index, n = indexes(case[0])[:2]
    ops.release_workspaces()
    fresh = S.bits(S.run_case(ops, index, n, case)[0])
    assert len(ops._WS_HOT) >= 1
    for buf in ops._WS_HOT.values():
        buf.fill_(0xFF)                                # both list counters now read -1 (and every float is a NaN)
    assert S.bits(S.run_case(ops, index, n, case)[0]) == fresh


def test_counters_are_reset_between_two_replays_of_a_graph(pgl, indexes):
    ops = pgl.ops
    index, n = indexes("rmat14")[:2]
    x = torch.from_numpy(S.normal_features(n, 128, 77)).cuda()
    csr = index.view()
    with S.sliced_path(ops, 8, 32):
        want = ops.aggregate(x, csr, "sum", n).clone()     # eager: the plan exists before the capture
        assert [p for p in csr._slices.values() if p is not None]
        # the workspace of a captured call is the capture's own: hand the library a buffer this test can reach
        held = []
        real = ops._ws
        try:
            ops._ws = lambda nbytes, device: held.append(real(nbytes, device)) or held[-1]
            out = torch.empty(n, 128, device="cuda")
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ops.aggregate(x, csr, "sum", n, out=out)
        finally:
            ops._ws = real
    assert len(held) == 1
    for _ in range(2):
        held[0].fill_(0xFF)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


# graph, chunk, which kinds of long rows the plan must hold
_READY_LATE = [("all_hub", 256, "ready"), ("all_hub", 64, "late"), ("rmat14", 8, "both")]


@pytest.mark.parametrize("name,chunk,kinds", _READY_LATE)
def test_ready_and_late_rows(pgl, indexes, name, chunk, kinds):
    ops = pgl.ops
    index, n, src, dst = indexes(name)
    x, want = _ints(indexes, name, 128)
    csr = index.view()
    with S.sliced_path(ops, chunk, 32):
        plan = ops.slice_plan(csr, ops.hub_table(csr, x), n, n)
    late = _late_rows(plan)                             # from the plan alone, before anything is launched
    if kinds == "ready":
        assert plan.n_long >= 64 and not late.any()
    elif kinds == "late":
        assert plan.n_long >= 64 and late.all()
    else:
        assert late.any() and (~late).any()
        assert int(_pieces(plan)[n:].max()) > H.FIX_SHORT + 1          # a virtual row that takes the long fix-up role
    out = torch.full((n, 128), float("nan"), device="cuda")
    ops.release_workspaces()
    with S.sliced_path(ops, chunk, 32):
        ops.aggregate(x, csr, "sum", n, out=out)
        assert [p for p in csr._slices.values() if p is not None] == [plan]     # the call ran over the plan examined above
        assert np.array_equal(host(out), want)          # integers: one dropped or doubled row changes bits
        for buf in ops._WS_HOT.values():
            buf.fill_(0xFF)
        out.fill_(float("nan"))
        ops.aggregate(x, csr, "sum", n, out=out)
    got = host(out)
    assert np.isfinite(got).all() and np.array_equal(got, want)


_TABLES = [("all_hub", 64), ("all_hub", 256), ("one_slice3", 64), ("one_slice6", 64), ("one_slice6", 256), ("tiny", 256), ("tiny", 8)]


@pytest.mark.parametrize("name,chunk", _TABLES)
def test_every_schedule_walks_every_block_once(pgl, indexes, front, name, chunk):
    ops = pgl.ops
    index, n, src, dst = indexes(name)
    x, want = _ints(indexes, name, 128)
    case = (name, chunk, 128, 32, 0)
    front(100)
    base, plan = S.run_case(ops, index, n, case, x=x)
    count = plan.blocks[9:]
    if name == "all_hub":
        assert count[0] == 0 and all(c > 0 for c in count[1:])                         # an empty rest stream
    elif name.startswith("one_slice"):
        assert [c > 0 for c in count[1:]] == [s == int(name[-1]) for s in range(8)]    # one slice with blocks, seven without
    elif chunk == 256:
        assert sum(count) == 3                                                         # three blocks for eight XCDs
    assert np.array_equal(host(base), want)
    for v in S.FRONTS:
        front(v)
        got = S.run_case(ops, index, n, case, x=x)[0]
        assert np.array_equal(host(got), want), "slice_front = %d" % v
        assert torch.equal(got, base), "slice_front = %d" % v


def test_slice_front_refuses_nothing_and_clamps(pgl, indexes, front):
    """Any value is taken: below 1 the slice blocks simply come first, above 100 is 100, negative restores the default."""
    ops = pgl.ops
    index, n = indexes("one_slice3")[:2]
    x, want = _ints(indexes, "one_slice3", 128)
    for v in (0, 1, 1000):
        front(v)
        assert np.array_equal(host(S.run_case(ops, index, n, ("one_slice3", 64, 128, 32, 0), x=x)[0]), want)
