"""What tests/test_slice_tail_gpu.py and scripts/record_slice_bits.py share: the cases whose output BITS are pinned to the commit that
introduced the sliced aggregation's tail changes (tests/golden/hub_slices_parent_bits.json), and how one case is run.  The tail of
pglamd_aggregate_sliced -- counter reset, fix-up, combine -- and the block schedule of its flat launch may change when and where work
runs, never a bit of the result: every row keeps its terms, their order and its roundings."""
import contextlib
import hashlib

import numpy as np

import hub_slice_defs as H

# (graph, chunk, d, row_min, rows beyond the index's)
BIT_CASES = [("rmat14", 8, 128, 32, 0), ("rmat14", 8, 252, 32, 0), ("rmat14", 64, 128, 32, 0), ("rmat14", 256, 128, 128, 0),
             ("rmat14", 128, 128, 128, 0), ("rmat14", 64, 128, 32, 100)] + \
            [(name, chunk, 128, 32, 0) for name in ("all_hub", "tiny", "one_slice3", "one_slice6") for chunk in (8, 64)]

# "slice_front" values (per cent of an XCD's block sequence that holds its slice blocks): the sweep set
FRONTS = (100, 85, 70, 60, 50)


def case_id(case):
    return "%s-chunk%d-d%d-L%d-extra%d" % case


def make_graph(name):
    """(n, src, dst) of a graph of hub_slice_defs by name."""
    return H.rmat14() if name == "rmat14" else H.BUILDERS[name]()


def device_index(pgl, name):
    """-> (destination-sorted index on the device, n, src, dst)"""
    n, src, dst = make_graph(name)
    g = pgl.Graph(edges=np.stack([src, dst], 1), num_nodes=n).tensor()
    return g.adj_dst_index.csr, n, src, dst


def normal_features(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


@contextlib.contextmanager
def sliced_path(ops, chunk, row_min):
    """Lowers the thresholds so that a small graph takes pglamd_aggregate_sliced, with `chunk` edges per chunk."""
    names = ("_HUB_TABLE", "_HUB_SLICES", "_SLICE_MIN_EDGES", "_HUB_MIN_EDGES", "_SLICE_ROW_MIN", "_flat_chunk")
    old = [getattr(ops, k) for k in names]
    try:
        for k, v in zip(names, (True, True, 0, 0, row_min, lambda num_edges: chunk)):
            setattr(ops, k, v)
        yield
    finally:
        for k, v in zip(names, old):
            setattr(ops, k, v)


def run_case(ops, index, n, case, x=None):
    """One sliced sum over a fresh view of `index` -> (the output on the device, the plan the call used)."""
    import torch
    name, chunk, d, row_min, extra = case
    if x is None:
        x = torch.from_numpy(normal_features(n, d, 3000 + d)).cuda()
    csr = index.view()
    with sliced_path(ops, chunk, row_min):
        out = ops.aggregate(x, csr, "sum", n + extra)
    (plan,) = [p for p in (csr._slices or {}).values() if p is not None]
    assert plan.chunk == chunk and plan.row_min == row_min and plan.out_rows == n + extra
    return out, plan


def bits(t):
    """sha256 of a tensor's bytes"""
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()
