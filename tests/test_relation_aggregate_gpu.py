"""Relational aggregation on the MI355X (aggregate_rel.hip: pglamd_aggregate_relations; ops.aggregate_relations,
HeterGraph.send_recv_relations, RGCNConv(fused=True)) held to its definition (tests/relation_aggregate_defs.py): every output element
inside the fp32 re-association bound of its own terms against fp64 and inside twice that against the per-relation send_recv
composition; the scalar and vector paths and every group width; degenerate shapes; the long-row branch (bounds, bit-identical
repeats, hinted and computed max_segment); special values; gradients element by element; the sampler's seeded index.
Graphs have at most 2 000 nodes and 30 k edges over all relations."""
import numpy as np
import pytest
import torch

import grad_defs as G
import relation_aggregate_defs as D
from gpu_common import RTOL, assert_within_fp32_reassociation, check_grad_elements, close_rows, close_terms, dev, host, pgl      # noqa: F401

pytestmark = pytest.mark.gpu

N = 700
TYPES = ["a", "b", "c"]


def _lists(seed=0, n=N, empty_relation=True):
    """Three relations over n nodes: random with duplicate edges and self-loops; one without any edge (or a sparse one); one that
    reaches only rows < n / 4.  Rows >= 0.9 n have no in-edge in any relation."""
    rng = np.random.default_rng(seed)
    top = max(int(n * 0.9), 1)
    s, d = rng.integers(0, n, 6000), rng.integers(0, top, 6000)
    s[:100] = d[:100]
    a = (np.concatenate([s, s[:500]]), np.concatenate([d, d[:500]]))
    b = (np.zeros(0, np.int64), np.zeros(0, np.int64)) if empty_relation else (rng.integers(0, n, 900), rng.integers(0, top, 900))
    c = (rng.integers(0, n, 1500), rng.integers(0, max(n // 4, 1), 1500))
    return [tuple(np.asarray(t, np.int64) for t in a), b, tuple(np.asarray(t, np.int64) for t in c)]


def _hg(pgl, lists, n, types=None):
    types = types or TYPES[:len(lists)]
    return pgl.HeterGraph(edges={et: np.stack([s, d], 1).reshape(-1, 2) for et, (s, d) in zip(types, lists)}, num_nodes=n).tensor()


def _check(got, x, indptr, col, op, out_size=None, per_relation=False, col_scale=None, what=""):
    want, abs_terms, n_terms = D.relation_aggregate(x, indptr, col, op, out_size, per_relation, col_scale)
    got = host(got)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    assert_within_fp32_reassociation(got, want, abs_terms, n_terms, slack=4.0)
    untouched = abs_terms == 0
    assert not np.signbit(got[untouched]).any() and not got[untouched].any(), what + ": an element without a contributing edge must be +0.0"
    return want, abs_terms, n_terms


@pytest.fixture(scope="module")
def base(pgl):
    lists = _lists()
    hg = _hg(pgl, lists, N)
    stacked = hg._stacked_pred()[0]
    indptr, col = D.stack_edges(lists, N)
    assert np.array_equal(host(stacked.indptr), indptr) and np.array_equal(host(stacked.col), col)
    return hg, stacked, lists, indptr, col


# ---- parity: sum / mean x shared / per-relation x x summed / per-relation output, every width ---------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 33, 64, 128, 130])
@pytest.mark.parametrize("op", ["sum", "mean"])
def test_every_layout_against_fp64_and_the_per_relation_composition(pgl, base, d, op):
    hg, stacked, lists, indptr, col = base
    rng = np.random.default_rng(d)
    for stacked_x in (False, True):
        x = rng.standard_normal((3, N, d) if stacked_x else (N, d)).astype(np.float32)
        xd = dev(x)
        parts = [host(hg[et].send_recv(xd[r] if stacked_x else xd, op)) for r, et in enumerate(TYPES)]
        for per_relation in (False, True):
            what = "d=%d %s stacked_x=%s per_relation=%s" % (d, op, stacked_x, per_relation)
            got = pgl.ops.aggregate_relations(xd, stacked, op, per_relation=per_relation)
            want, abs_terms, n_terms = _check(got, x, indptr, col, op, None, per_relation, what=what)
            composed = np.stack(parts, 1) if per_relation else parts[0] + parts[1] + parts[2]
            close_terms(host(got), composed, abs_terms, n_terms, what=what + " vs send_recv per relation")
            again = hg.send_recv_relations(xd, op, per_relation=per_relation)
            assert torch.equal(again, got), what


# ---- shapes that break kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 5])
def test_degenerate_shapes(pgl, base, d):
    hg, stacked, lists, indptr, col = base
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, d)).astype(np.float32)
    # R = 1; R = 3 with an empty relation is the base fixture
    one = _hg(pgl, lists[:1], N)
    ip1, c1 = D.stack_edges(lists[:1], N)
    for per_relation in (False, True):
        _check(pgl.ops.aggregate_relations(dev(x), one._stacked_pred()[0], "mean", per_relation=per_relation), x, ip1, c1, "mean", None, per_relation, what="R=1")
    # many relations (the entry point does not cap R): 70 copies of two small relations
    many = [(s[:40 + r], dd[:40 + r]) for r in range(35) for s, dd in (lists[0], lists[2])]
    types = ["t%d" % i for i in range(70)]
    hg70 = _hg(pgl, many, N, types)
    ip70, c70 = D.stack_edges(many, N)
    _check(pgl.ops.aggregate_relations(dev(x), hg70._stacked_pred()[0], "mean"), x, ip70, c70, "mean", what="R=70")
    _check(pgl.ops.aggregate_relations(dev(x), hg70._stacked_pred()[0], "sum", per_relation=True), x, ip70, c70, "sum", None, True, what="R=70 per relation")
    # out_size < rows; out_size = 0 means every row, as for send_recv
    for m in (1, 255, 257):
        _check(pgl.ops.aggregate_relations(dev(x), stacked, "mean", out_size=m), x, indptr, col, "mean", m, what="out_size=%d" % m)
        _check(pgl.ops.aggregate_relations(dev(x), stacked, "sum", out_size=m, per_relation=True), x, indptr, col, "sum", m, True)
    assert tuple(pgl.ops.aggregate_relations(dev(x), stacked, "mean", out_size=0).shape) == (N, d)
    # N = 1 (self-loops only) and E = 0 overall
    loops = [(np.zeros(3, np.int64), np.zeros(3, np.int64)), (np.zeros(0, np.int64), np.zeros(0, np.int64))]
    hg1 = _hg(pgl, loops, 1)
    ip, c = D.stack_edges(loops, 1)
    _check(pgl.ops.aggregate_relations(dev(x[:1]), hg1._stacked_pred()[0], "mean"), x[:1], ip, c, "mean", what="N=1")
    none = [(np.zeros(0, np.int64), np.zeros(0, np.int64))] * 2
    hg0 = _hg(pgl, none, 9)
    out = pgl.ops.aggregate_relations(dev(x[:9]), hg0._stacked_pred()[0], "sum", per_relation=True)
    assert tuple(out.shape) == (9, 2, d) and not host(out).any() and not np.signbit(host(out)).any()
    # n_src != rows (a block's shape): more feature rows than index rows, and fewer (columns beyond x contribute nothing)
    xl = rng.standard_normal((N + 50, d)).astype(np.float32)
    _check(pgl.ops.aggregate_relations(dev(xl), stacked, "sum"), xl, indptr, col, "sum", what="n_src > rows")
    few = N - 100
    kept = [(s[s < few], dd[s < few]) for s, dd in lists]                 # the definition over the edges whose source row exists
    ipk, ck = D.stack_edges(kept, N)
    assert len(ck) < len(col)
    _check(pgl.ops.aggregate_relations(dev(x[:few]), stacked, "sum"), x[:few], ipk, ck, "sum", what="n_src < rows")


def test_unaligned_view_takes_the_scalar_path(pgl, base):
    hg, stacked, lists, indptr, col = base
    rng = np.random.default_rng(12)
    buf = rng.standard_normal((N, 9)).astype(np.float32)
    xd = dev(buf)[:, 1:]                                                  # d = 8, rows start 4 bytes off a 16-byte boundary, row stride 9
    assert xd.data_ptr() % 16 != 0 and xd.stride(0) == 9
    _check(pgl.ops.aggregate_relations(xd, stacked, "mean"), buf[:, 1:], indptr, col, "mean", what="unaligned view")
    _check(pgl.ops.aggregate_relations(xd.t().contiguous().t(), stacked, "mean"), buf[:, 1:], indptr, col, "mean", what="column-major view")


def test_col_scale(pgl, base):
    hg, stacked, lists, indptr, col = base
    rng = np.random.default_rng(13)
    x, c = rng.standard_normal((N, 12)).astype(np.float32), rng.standard_normal((3, N)).astype(np.float32)
    _check(pgl.ops.aggregate_relations(dev(x), stacked, "sum", col_scale=dev(c)), x, indptr, col, "sum", None, False, c, what="col_scale")
    _check(pgl.ops.aggregate_relations(dev(x), stacked, "sum", per_relation=True, col_scale=dev(c)), x, indptr, col, "sum", None, True, c)


# ---- the long-row branch ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hub(pgl):
    """Row 321 has 5 000 in-edges in relation a and 300 in relation c (and a few in b); 2 000 nodes, 20 000 edges."""
    n = 2000
    rng = np.random.default_rng(21)
    lists = []
    for e, h in ((12000, 5000), (3000, 7), (5000, 300)):
        s, d = rng.integers(0, n, e), rng.integers(0, n, e)
        d[rng.choice(e, h, replace=False)] = 321
        s[rng.choice(e, 2 * h, replace=False)] = 7                         # and a hub SOURCE: the backward's long row
        lists.append((s.astype(np.int64), d.astype(np.int64)))
    indptr, col = D.stack_edges(lists, n)
    assert indptr[0, 322] - indptr[0, 321] >= 5000 and 300 <= indptr[2, 322] - indptr[2, 321] < 320
    return lists, n, indptr, col


@pytest.mark.parametrize("d", [1, 6, 64, 128, 260])
@pytest.mark.parametrize("op", ["sum", "mean"])
def test_long_rows_stay_in_bound_and_repeat_bit_for_bit(pgl, hub, d, op):
    lists, n, indptr, col = hub
    rng = np.random.default_rng(d + 1)
    x = rng.standard_normal((n, d)).astype(np.float32)
    xd = dev(x)
    computed = _hg(pgl, lists, n)._stacked_pred()[0]
    hinted = _hg(pgl, lists, n)._stacked_pred()[0]
    hinted.max_segment = int(np.diff(indptr, axis=1).max())
    assert "max_segment" not in computed.__dict__
    for per_relation in (False, True):
        for long_row in (64, 4096, None):
            runs = [pgl.ops.aggregate_relations(xd, st, op, per_relation=per_relation, long_row=long_row)
                    for st in (computed, computed, hinted)]
            _check(runs[0], x, indptr, col, op, None, per_relation, what="long_row=%s d=%d" % (long_row, d))
            assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), "long_row=%s: not bit-identical" % long_row
    assert computed.max_segment == hinted.max_segment
    assert pgl.ops.stacked_long_rows(computed, 64) is not None and pgl.ops.stacked_long_rows(computed, 10 ** 6) is None
    assert host(pgl.ops.stacked_long_rows(computed, 4096)).tolist() == [321]
    # out_size below the long row: its list entry is ignored
    _check(pgl.ops.aggregate_relations(xd, computed, op, out_size=300, long_row=64), x, indptr, col, op, 300, what="out_size below the hub")


def test_threshold_does_not_change_a_graph_without_long_rows(pgl, base):
    hg, stacked, lists, indptr, col = base
    x = dev(np.random.default_rng(14).standard_normal((N, 64)).astype(np.float32))
    longest = pgl.ops.stacked_max_segment(stacked)
    ref = pgl.ops.aggregate_relations(x, stacked, "mean")
    for long_row in (longest, longest + 1, 4096, 10 ** 9):
        assert torch.equal(pgl.ops.aggregate_relations(x, stacked, "mean", long_row=long_row), ref), long_row


# ---- special values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("d", [3, 64])
def test_non_finite_rows_reach_exactly_their_destinations(pgl, base, hub, bad, d):
    for lists, n in ((base[2], N), (hub[0], hub[1])):
        stacked = _hg(pgl, lists, n)._stacked_pred()[0]
        x = np.random.default_rng(15).standard_normal((n, d)).astype(np.float32)
        u = 5
        x[u] = bad
        for op in ("sum", "mean"):
            got = host(pgl.ops.aggregate_relations(dev(x), stacked, op, per_relation=True, long_row=64))
            summed = host(pgl.ops.aggregate_relations(dev(x), stacked, op, long_row=64))
            reach = np.zeros((n, len(lists)), bool)
            for r, (s, dd) in enumerate(lists):
                reach[dd[s == u], r] = True
            assert reach.any()
            hit = ~np.isfinite(got).all(2)
            assert np.array_equal(hit, reach), "%s: a non-finite source row must reach exactly its destinations, per relation" % op
            assert np.array_equal(~np.isfinite(summed).all(1), reach.any(1))
            if np.isinf(bad):
                only = reach.sum(1) == 1
                assert (summed[only] == bad).all()


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
def _tensors(lists):
    return [(dev(s), dev(d)) for s, d in lists]


@pytest.mark.parametrize("op", ["sum", "mean"])
@pytest.mark.parametrize("stacked_x", [False, True])
@pytest.mark.parametrize("per_relation", [False, True])
@pytest.mark.parametrize("d,out_size", [(8, None), (5, 300), (64, None)])
def test_send_recv_relations_gradient_element_by_element(pgl, base, op, stacked_x, per_relation, d, out_size):
    hg, stacked, lists, indptr, col = base
    rng = np.random.default_rng(31 + d)
    M = out_size or N
    x = rng.standard_normal((3, N, d) if stacked_x else (N, d)).astype(np.float32)
    g = rng.standard_normal((M, 3, d) if per_relation else (M, d)).astype(np.float32)
    xd = dev(x).requires_grad_(True)
    out = hg.send_recv_relations(xd, op, out_size, per_relation)
    _check(out, x, indptr, col, op, out_size, per_relation)
    out.backward(dev(g))
    want, abs_terms, n_terms = D.relation_aggregate_grad(g, indptr, col, x.shape, op, per_relation)
    check_grad_elements(xd.grad, torch.as_tensor(want), torch.as_tensor(abs_terms), torch.as_tensor(np.ascontiguousarray(n_terms)),
                        what="d x (%s, stacked_x=%s, per_relation=%s)" % (op, stacked_x, per_relation))
    # the definition's own autograd agrees with the numpy gradient (the two restatements hold each other)
    r = G.grad_and_terms(lambda t, frozen=None: D.t_send_recv_relations(t, _tensors(lists), op, out_size, per_relation), [dev(x)], dev(g))
    np.testing.assert_allclose(host(r.want64[0]), want, rtol=1e-12, atol=1e-12)


def test_gradient_through_the_long_branch(pgl, hub):
    lists, n, indptr, col = hub
    hg = _hg(pgl, lists, n)
    rng = np.random.default_rng(33)
    x, g = rng.standard_normal((n, 16)).astype(np.float32), rng.standard_normal((n, 16)).astype(np.float32)
    xd = dev(x).requires_grad_(True)
    hg.send_recv_relations(xd, "mean").backward(dev(g))
    want, abs_terms, n_terms = D.relation_aggregate_grad(g, indptr, col, x.shape, "mean")
    check_grad_elements(xd.grad, torch.as_tensor(want), torch.as_tensor(abs_terms), torch.as_tensor(np.ascontiguousarray(n_terms)))


@pytest.mark.parametrize("num_bases", [0, 2])
@pytest.mark.parametrize("order", ["aggregate", "project", None])
@pytest.mark.parametrize("out_size", [None, 200])
def test_rgcn_fused_against_fp64_and_the_loop(pgl, base, num_bases, order, out_size):
    """Bounds: every output / gradient element is a nested sum of monomials (edges x input columns x relations [x bases]); a nested
    fp32 summation of non-negative-weighted monomials stays within (total length of the nested sums) x eps x sum|monomials| (Higham
    4.4 applied level by level), so n_terms = the sum of the lengths of the nested sums + one per scale, K = 1."""
    hg, stacked, lists, indptr, col = base
    d_in, d_out = 12, 8
    torch.manual_seed(3)
    loop = pgl.nn.RGCNConv(d_in, d_out, TYPES, num_bases=num_bases).cuda()
    fused = pgl.nn.RGCNConv(d_in, d_out, TYPES, num_bases=num_bases, fused=True).cuda()
    fused.load_state_dict(loop.state_dict())
    rng = np.random.default_rng(41)
    M = out_size or N
    x, g = rng.standard_normal((N, d_in)).astype(np.float32), rng.standard_normal((M, d_out)).astype(np.float32)
    outs = []
    for layer in (loop, fused):
        xd = dev(x).requires_grad_(True)
        out = layer(hg, xd, out_size=out_size) if layer is loop else layer(hg, xd, out_size=out_size, order=order)
        out.backward(dev(g))
        outs.append((out, xd.grad, [p.grad for p in layer.parameters()]))
    (o0, gx0, gp0), (o1, gx1, gp1) = outs
    close_rows(host(o1), host(o0), RTOL, what="fused vs loop: output")
    close_rows(host(gx1), host(gx0), RTOL, what="fused vs loop: d feat")
    for a, b, (name, _) in zip(gp1, gp0, fused.named_parameters()):
        close_rows(host(a).reshape(a.shape[0], -1), host(b).reshape(b.shape[0], -1), RTOL, what="fused vs loop: d " + name)
    # fp64, element by element
    has_comp = num_bases == 2
    params = dict(fused.named_parameters())
    inputs = [dev(x), params["weight"].detach()] + ([params["w_comp"].detach()] if has_comp else [])
    fn = (lambda f, w, c, frozen=None: D.t_rgcn(f, w, c, _tensors(lists), out_size)) if has_comp else \
         (lambda f, w, frozen=None: D.t_rgcn(f, w, None, _tensors(lists), out_size))
    ind, outd = D.degrees(lists, N, M)
    R, B = 3, max(num_bases, 1)
    n_out = ind + R * d_in + B + 2
    n_feat = outd + d_out * R + B + 2
    n_w = float(M + ind.max() + R + 2)
    r = G.grad_and_terms(fn, inputs, dev(g), n_out=n_out, n_terms=[n_feat, n_w] + ([float(d_in * d_out) + n_w] if has_comp else []))
    check_grad_elements(o1, r.out64, r.out_abs, r.out_n, what="fused output vs fp64")
    check_grad_elements(gx1, r.want64[0], r.abs_terms64[0], r.n_terms[0], what="fused d feat vs fp64")
    check_grad_elements(params["weight"].grad, r.want64[1], r.abs_terms64[1], r.n_terms[1], what="fused d weight vs fp64")
    if has_comp:
        check_grad_elements(params["w_comp"].grad, r.want64[2], r.abs_terms64[2], r.n_terms[2], what="fused d w_comp vs fp64")


def test_rgcn_byte_model_and_edge_type_order(pgl, base):
    hg, stacked, lists, indptr, col = base
    layer = pgl.nn.RGCNConv(16, 64, TYPES, fused=True)
    assert layer.fused_order(10000, 100, 100000) == "aggregate" and pgl.nn.RGCNConv(64, 4, TYPES, fused=True).fused_order(10 ** 6, 1000, 1000) == "project"
    torch.manual_seed(4)
    shuffled = ["c", "a", "b"]
    loop = pgl.nn.RGCNConv(6, 5, shuffled).cuda()
    fused = pgl.nn.RGCNConv(6, 5, shuffled, fused=True).cuda()
    fused.load_state_dict(loop.state_dict())
    x = dev(np.random.default_rng(42).standard_normal((N, 6)).astype(np.float32))
    for order in ("aggregate", "project"):
        close_rows(host(fused(hg, x, order=order)), host(loop(hg, x)), RTOL, what="edge types in another order")
    with pytest.raises(ValueError):
        pgl.nn.RGCNConv(6, 5, ["a", "b"], fused=True).cuda()(hg, x)
    with pytest.raises(ValueError):
        fused(hg, x, order="both")


# ---- the sampler's blocks -------------------------------------------------------------------------------------------------------------
def test_sampler_blocks_carry_their_stacked_index(pgl, base):
    hg, stacked, lists, indptr, col = base
    fan = [10, 0, -1]
    seeds = dev(np.concatenate([np.arange(0, 300, 3), np.arange(0, 60, 3), [699, 699]]).astype(np.int64))
    plain = pgl.sampling.RelationNeighborSampler(hg, [fan, fan], seed=5)
    blocks, out_nodes = plain.sample_neighbors(seeds)
    blocks2, out_nodes2 = pgl.sampling.RelationNeighborSampler(hg, [fan, fan], seed=5).sample_neighbors(seeds)
    assert torch.equal(out_nodes, out_nodes2)
    # what the sampler returns is what the op and the relabel give (the sampler's first layer draws with seed + 1)
    s = pgl.ops.sample_neighbors_relations(stacked, seeds, fan, seed=6)
    src, first_nodes = pgl.ops._relabel(seeds.contiguous(), s.neighbors)
    inner, n_inner = blocks[-1]
    assert n_inner == len(seeds) and int(inner.num_nodes) == len(first_nodes)
    for r, et in enumerate(TYPES):
        a, b = s.edge_split[r], s.edge_split[r + 1]
        assert torch.equal(inner[et].edges, torch.stack([src[a:b], s.dst[a:b]], 1)), et
    torch.manual_seed(5)
    loop = pgl.nn.RGCNConv(10, 7, TYPES).cuda()
    fused = pgl.nn.RGCNConv(10, 7, TYPES, fused=True).cuda()
    fused.load_state_dict(loop.state_dict())
    for (block, n_dst), (block2, n_dst2) in zip(blocks, blocks2):
        assert n_dst == n_dst2
        seeded = block._stacked_p[1]
        assert "max_segment" not in seeded.__dict__                        # (a fan-out of -1: not known for free)
        edges_before = {et: block[et].edges.clone() for et in TYPES}
        rebuilt = pgl.ops.stack_indices([block[et].adj_dst_index.csr for et in TYPES])
        for name, a, b in zip(seeded._fields[:3], seeded[:3], rebuilt[:3]):
            assert a.dtype == b.dtype and torch.equal(a, b), name
        assert seeded.num_nodes == rebuilt.num_nodes and tuple(seeded.edge_base) == tuple(rebuilt.edge_base)
        for et in TYPES:
            assert torch.equal(block[et].edges, block2[et].edges) and torch.equal(block[et].edges, edges_before[et])
            assert torch.equal(block[et].adj_dst_index.csr.indptr, block2[et].adj_dst_index.csr.indptr)
        n_blk = int(block.num_nodes)
        h = dev(np.random.default_rng(n_blk).standard_normal((n_blk, 10)).astype(np.float32))
        ha = h.clone().requires_grad_(True)
        want = loop(block2, ha)[:n_dst]
        g = torch.ones_like(want)
        want.backward(g)
        for order in ("aggregate", "project"):
            hb = h.clone().requires_grad_(True)
            got = fused(block, hb, out_size=n_dst, order=order)
            assert tuple(got.shape) == (n_dst, 7)
            close_rows(host(got), host(want), RTOL, what="block, order=%s" % order)
            got.backward(g)
            close_rows(host(hb.grad), host(ha.grad), RTOL, what="block: d h, order=%s" % order)
        # the successor side from ONE build over the keys r * n_blk + src is the stack of the relations' own src indices
        succ = block._stacked_src()
        twin = pgl.ops.stack_indices([block[et].adj_src_index.csr for et in TYPES])
        assert torch.equal(succ.indptr, twin.indptr) and tuple(succ.edge_base) == tuple(twin.edge_base) and torch.equal(succ.col, twin.col)
    known = pgl.sampling.RelationNeighborSampler(hg, [[10, 0, 4]], seed=5).sample_neighbors(seeds)[0][0][0]
    assert known._stacked_p[1].max_segment == 10


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_value_errors_come_before_any_launch(pgl, base, monkeypatch):
    hg, stacked, lists, indptr, col = base
    x = dev(np.zeros((N, 8), np.float32))
    launches = []
    monkeypatch.setattr(pgl.ops, "_launch", lambda *a, **k: launches.append(a))
    for call in (lambda: pgl.ops.aggregate_relations(x.half(), stacked),
                 lambda: pgl.ops.aggregate_relations(x[None].expand(4, N, 8), stacked),
                 lambda: pgl.ops.aggregate_relations(x, stacked, "sum", col_scale=dev(np.ones((3, N + 1), np.float32))),
                 lambda: pgl.ops.aggregate_relations(x, stacked, col_scale=dev(np.ones((N,), np.float32))),
                 lambda: pgl.ops.aggregate_relations(x, stacked, reduce_op="max"),
                 lambda: pgl.ops.aggregate_relations(x, stacked, out_size=N + 1),
                 lambda: pgl.ops.aggregate_relations(x, stacked, out=torch.empty((N, 9), device="cuda")),
                 lambda: hg.send_recv_relations(x, "max"),
                 lambda: hg.send_recv_relations(x[:-1])):
        with pytest.raises(ValueError):
            call()
    assert not launches
