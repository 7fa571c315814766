"""The induced subgraph on the MI355X (subgraph.hip) held bit for bit to its definition, restated in numpy in
tests/subgraph_defs.py and evaluated on the device's own index: every node-set shape (empty, one self-loop node, zero-degree
rows, shuffled fractions, the whole graph, a hub with none / half / all of its sources), rows around the wave and block sizes,
more selected rows than one launch has lanes, more candidate positions than one launch has tile slots, determinism, refusals,
and what pgl_amd.sampling builds on it (subgraph / induced_subgraph on a tensor graph, ClusterBatches, random_walk_subgraph)."""
import numpy as np
import pytest
import torch

import sampling_defs as S
import subgraph_defs as D
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu

HUB = 4242
EXACT = (63, 64, 65, 255, 256, 257)


def _assert_index_is_the_restated_one(csr, host_csr):
    assert np.array_equal(host(csr.indptr), host_csr[0]) and np.array_equal(host(csr.col32), host_csr[1]) and \
        np.array_equal(host(csr.eid32), host_csr[2])                                      # the index the restatement reads IS the device's


@pytest.fixture(scope="module")
def rmat14(pgl):
    """RMAT-14 with 200 000 edges, built the way test_sampling_gpu.py's rmat_small is, plus a 6 000-edge hub, rows of exactly
    63 / 64 / 65 and 255 / 256 / 257 in-edges, a node whose only in-edges are two self-loops, integer-valued node and edge
    features.  -> dict."""
    from pgl_amd.utils.rmat import rmat_edges
    n = 1 << 14
    e = rmat_edges(14, 200000, seed=11).numpy()
    rng = np.random.default_rng(1)
    e[rng.choice(len(e), 6000, replace=False), 1] = HUB
    empty = np.flatnonzero(np.bincount(e[:, 1], minlength=n) == 0)
    exact_nodes = empty[:len(EXACT)]
    loop_node = int(empty[len(EXACT)])
    e = np.concatenate([e] + [np.stack([rng.integers(0, n, d), np.full(d, v)], 1) for v, d in zip(exact_nodes, EXACT)] +
                       [np.full((2, 2), loop_node)])
    e = e[rng.permutation(len(e))].astype(np.int64)
    deg = np.bincount(e[:, 1], minlength=n)
    assert deg.max() >= 6000 and (deg == 0).sum() > 100 and all(deg[v] == d for v, d in zip(exact_nodes, EXACT))
    assert len(np.unique(e[:, 0] * n + e[:, 1])) < len(e) and (e[:, 0] == e[:, 1]).sum() > 2      # multi-edges, self-loops
    nf = {"h": rng.integers(-8, 9, (n, 5)).astype(np.float32), "y": rng.integers(0, 7, n)}
    ef = {"w": rng.integers(-8, 9, (len(e), 3)).astype(np.float32), "t": np.arange(len(e), dtype=np.int64)}
    g_np = pgl.Graph(edges=e, num_nodes=n, node_feat=dict(nf), edge_feat=dict(ef))
    g = pgl.Graph(edges=e, num_nodes=n, node_feat=dict(nf), edge_feat=dict(ef)).tensor()
    host_csr = S.csr_by_dst(e, n)
    _assert_index_is_the_restated_one(g.adj_dst_index.csr, host_csr)
    return dict(e=e, n=n, g=g, g_np=g_np, csr=g.adj_dst_index.csr, host_csr=host_csr, deg=deg, exact=exact_nodes, loop=loop_node)


SETS = ["empty", "self-loop", "zero-degree", "1%", "30%", "100%", "arange", "exact-rows", "hub-none", "hub-half", "hub-all"]


def _node_set(kind, G):
    n, e, deg = G["n"], G["e"], G["deg"]
    rng = np.random.default_rng(SETS.index(kind))
    if kind == "empty":
        return np.zeros(0, np.int64)
    if kind == "self-loop":
        return np.asarray([G["loop"]], np.int64)
    if kind == "zero-degree":
        return rng.permutation(np.flatnonzero(deg == 0))
    if kind.endswith("%"):
        return rng.permutation(n)[:n * int(kind[:-1]) // 100]
    if kind == "arange":
        return np.arange(n, dtype=np.int64)
    if kind == "exact-rows":                                                               # the 63 .. 257 rows next to all of their sources
        rows = G["exact"]
        return rng.permutation(np.union1d(rows, e[np.isin(e[:, 1], rows), 0]))
    srcs = np.setdiff1d(e[e[:, 1] == HUB, 0], [HUB])
    others = np.setdiff1d(np.arange(n), np.concatenate([srcs, [HUB]]))[:300]
    take = {"hub-none": srcs[:0], "hub-half": rng.permutation(srcs)[:len(srcs) // 2], "hub-all": srcs}[kind]
    return rng.permutation(np.concatenate([[HUB], others, take]))


def _assert_equals_restatement(pgl, csr, host_csr, nodes, n, what):
    want = D.induced_restated(*host_csr, nodes, n)
    got = pgl.ops.induced_subgraph(csr, dev(np.asarray(nodes, np.int64)))
    again = pgl.ops.induced_subgraph(csr, dev(np.asarray(nodes, np.int64)))
    for name, g, a, w in zip(("src_local", "dst_local", "eids"), got, again, want):
        assert g.dtype == torch.int64 and g.is_cuda and tuple(g.shape) == w.shape, (what, name, tuple(g.shape), w.shape)
        assert torch.equal(g, a), (what, name, "two calls differ")
        g = host(g)
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s: %s differ first at entry %d of %d: got %s, want %s" % (what, name, i, len(w), g[i:i + 4], w[i:i + 4]))
    return want


@pytest.mark.parametrize("kind", SETS)
def test_induced_subgraph_equals_the_restatement(pgl, rmat14, kind):
    G = rmat14
    nodes = _node_set(kind, G)
    src, dst, eids = _assert_equals_restatement(pgl, G["csr"], G["host_csr"], nodes, G["n"], kind)
    if kind in ("empty", "zero-degree"):
        assert len(eids) == 0                                                              # kept == 0: no fill launch
    if kind == "self-loop":
        assert src.tolist() == [0, 0] and dst.tolist() == [0, 0] and len(set(eids.tolist())) == 2
    if kind == "arange":                                                                   # the whole index, as it lies
        assert np.array_equal(eids, G["host_csr"][2]) and np.array_equal(src, G["host_csr"][1])
        assert np.array_equal(dst, host(G["csr"].row32))
    if kind == "100%":
        assert len(eids) == len(G["e"])
    if kind == "exact-rows":
        kept = np.bincount(dst, minlength=len(nodes))
        assert sorted(kept[np.isin(nodes, G["exact"])].tolist()) == sorted(EXACT)          # every one of those rows whole
    if kind.startswith("hub"):
        hub_row = int(np.flatnonzero(nodes == HUB)[0])
        into_hub = int((dst == hub_row).sum())
        e = G["e"]
        srcs_in = np.isin(e[:, 0], nodes) & (e[:, 1] == HUB)
        assert into_hub == int(srcs_in.sum())
        if kind == "hub-all":
            assert into_hub == int(G["deg"][HUB]) >= 6000
        if kind == "hub-none":
            assert into_hub == int(((e[:, 0] == HUB) & (e[:, 1] == HUB)).sum())


def test_more_selected_rows_than_one_launch_has_lanes(pgl):
    """Every node of a sparse 1.2 M-node graph, shuffled: the mark kernel and the scans stride."""
    lanes = pgl.ops.induced_subgraph_launch_threads()
    n = lanes + 151424
    rng = np.random.default_rng(3)
    e = rng.integers(0, n, (5000, 2)).astype(np.int64)
    e[:40, 1] = e[0, 1]
    g = pgl.Graph(edges=e, num_nodes=n).tensor()
    host_csr = S.csr_by_dst(e, n)
    _assert_index_is_the_restated_one(g.adj_dst_index.csr, host_csr)
    nodes = rng.permutation(n)
    assert len(nodes) > lanes
    want = _assert_equals_restatement(pgl, g.adj_dst_index.csr, host_csr, nodes, n, "1.2M rows")
    assert len(want[2]) == 5000
    half = nodes[:n // 2]
    want = _assert_equals_restatement(pgl, g.adj_dst_index.csr, host_csr, half, n, "0.6M rows")
    assert 0 < len(want[2]) < 5000


def test_more_candidate_positions_than_one_launch_has_tile_slots(pgl):
    """A tile is four passes of one 256-lane block, so one launch covers 4 x launch_threads candidate positions at once; with
    4.5 M edges selected the count and fill kernels stride over the tiles."""
    slots = 4 * pgl.ops.induced_subgraph_launch_threads()
    n, m = 200000, slots + 300000
    rng = np.random.default_rng(4)
    e = rng.integers(0, n, (m, 2)).astype(np.int64)
    g = pgl.Graph(edges=e, num_nodes=n).tensor()
    csr = g.adj_dst_index.csr
    src, dst, eids = pgl.ops.induced_subgraph(csr, torch.arange(n, device="cuda"))
    assert int(eids.shape[0]) == m > slots
    assert torch.equal(eids, csr.eid32.long()) and torch.equal(src, csr.col32.long()) and torch.equal(dst, csr.row32.long())
    host_csr = (host(csr.indptr), host(csr.col32).astype(np.int64), host(csr.eid32).astype(np.int64))     # (csr_build is held bit-exact in test_a1_a3_index.py)
    nodes = rng.permutation(n)[:n * 97 // 100]
    want = _assert_equals_restatement(pgl, csr, host_csr, nodes, n, "4.5M candidates")
    assert int(np.diff(host_csr[0])[nodes].sum()) > slots and len(want[2]) > 0


def test_repeated_and_out_of_range_ids_are_value_errors_and_leave_nothing_behind(pgl, rmat14):
    G = rmat14
    csr, n = G["csr"], G["n"]
    good = np.random.default_rng(12).permutation(n)[:3000]
    head = good[~np.isin(good, [3, 5, 7, 9])][:1000]                                       # (distinct from the ids of the bad tails)
    for bad in ([7, 9, 7], [-1], [n], [3, 1 << 40], [5, n, 5], [int(head[0])]):
        nodes = np.concatenate([head, np.asarray(bad, np.int64)])
        with pytest.raises(ValueError):
            pgl.ops.induced_subgraph(csr, dev(nodes))
        with pytest.raises(ValueError):
            pgl.sampling.induced_subgraph(G["g"], dev(nodes))
        _assert_equals_restatement(pgl, csr, G["host_csr"], good, n, "after %s" % bad)     # the next call on the same index is right
    with pytest.raises(ValueError):                                                        # more ids than nodes: repeated, refused before any launch
        pgl.ops.induced_subgraph(csr, torch.zeros(n + 1, dtype=torch.int64, device="cuda"))


def _same_graph(sub_t, sub_np, feats=True):
    assert sub_t.is_tensor() and not sub_np.is_tensor()
    assert sub_t.num_nodes == sub_np.num_nodes and sub_t.edges.is_cuda and sub_t.edges.dtype == torch.int64
    assert np.array_equal(host(sub_t.edges), sub_np.edges)
    for a, b in ((sub_t.node_feat, sub_np.node_feat), (sub_t.edge_feat, sub_np.edge_feat)):
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].is_cuda and host(a[k]).dtype == b[k].dtype and np.array_equal(host(a[k]), b[k]), k


@pytest.mark.parametrize("kind", ["empty", "self-loop", "1%", "30%", "hub-half"])
def test_subgraph_and_induced_subgraph_on_a_tensor_graph_equal_the_numpy_path(pgl, rmat14, kind):
    G = rmat14
    g, g_np, n = G["g"], G["g_np"], G["n"]
    nodes = _node_set(kind, G)
    want = D.induced_restated(*G["host_csr"], nodes, n)
    sub = pgl.sampling.induced_subgraph(g, dev(nodes))
    _same_graph(sub, pgl.sampling.induced_subgraph(g_np, nodes))
    assert np.array_equal(host(sub.edges), np.stack([want[0], want[1]], 1)) and np.array_equal(host(sub.node_feat["index"]), nodes)
    assert np.array_equal(host(sub.edge_feat["t"]), want[2])
    _same_graph(pgl.sampling.subgraph(g, dev(nodes), eid=dev(want[2])), pgl.sampling.subgraph(g_np, nodes, eid=want[2]))
    _same_graph(pgl.sampling.subgraph(g, nodes, eid=want[2], with_node_feat=False, with_edge_feat=False),
                pgl.sampling.subgraph(g_np, nodes, eid=want[2], with_node_feat=False, with_edge_feat=False))
    pairs = G["e"][want[2]]
    _same_graph(pgl.sampling.subgraph(g, nodes, edges=pairs, with_edge_feat=False),
                pgl.sampling.subgraph(g_np, nodes, edges=pairs, with_edge_feat=False))
    bare = pgl.sampling.induced_subgraph(g, dev(nodes), with_node_feat=False, with_edge_feat=False)
    assert list(bare.node_feat) == ["index"] and not bare.edge_feat and torch.equal(bare.edges, sub.edges)


def test_subgraph_on_a_tensor_graph_refuses_ids_out_of_range(pgl, rmat14):
    g, n = rmat14["g"], rmat14["n"]
    with pytest.raises(ValueError):
        pgl.sampling.subgraph(g, [1, 2])
    for kw in (dict(nodes=[1, n], eid=[0]), dict(nodes=[1, 2], eid=[g.num_edges]), dict(nodes=[1, 2], eid=[-1]),
               dict(nodes=[1, 2], edges=[[1, n]])):
        with pytest.raises(ValueError):
            pgl.sampling.subgraph(g, **kw)


@pytest.mark.parametrize("kind", ["30%", "hub-all", "zero-degree"])
def test_message_passing_over_the_prebuilt_index(pgl, rmat14, kind):
    """send_recv over the subgraph's dst index (built without a sort) is exact on integer-valued fp32 features, and the
    backward -- which builds the src index -- is the out-degree inside the subgraph."""
    G = rmat14
    nodes = _node_set(kind, G)
    src, dst, _ = D.induced_restated(*G["host_csr"], nodes, G["n"])
    sub = pgl.sampling.induced_subgraph(G["g"], dev(nodes))
    x = np.random.default_rng(7).integers(-4, 5, (len(nodes), 8)).astype(np.float32)
    want = np.zeros_like(x)
    np.add.at(want, dst, x[src])
    assert np.abs(want).max() < 2 ** 20                                                    # every partial sum is an exact fp32 integer
    xt = dev(x).requires_grad_(True)
    out = sub.send_recv(xt, "sum")
    assert np.array_equal(host(out), want)
    out.sum().backward()
    assert np.array_equal(host(xt.grad), np.repeat(np.bincount(src, minlength=len(nodes)).astype(np.float32)[:, None], 8, 1))
    assert np.array_equal(host(sub.indegree()), np.bincount(dst, minlength=len(nodes)))
    assert np.array_equal(host(sub.outdegree()), np.bincount(src, minlength=len(nodes)))


def test_cluster_batches_partition_the_nodes_and_equal_the_restatement(pgl, rmat14):
    G = rmat14
    g, n = G["g"], G["n"]
    np.random.seed(5)
    part = pgl.partition.random_partition(g, 16)
    a, b = (pgl.sampling.ClusterBatches(g, part, clusters_per_batch=3, seed=21) for _ in range(2))
    assert len(a) == 6
    first = list(a)
    ids = [host(i) for _, i in first]
    assert all(i.is_cuda and i.dtype == torch.int64 for _, i in first) and len(first) == 6
    assert np.array_equal(np.sort(np.concatenate(ids)), np.arange(n))                      # every node in exactly one batch
    for (sub, _), i, (sub_b, i_b) in zip(first, ids, b):
        assert torch.equal(sub.edges, sub_b.edges) and np.array_equal(i, host(i_b))        # one seed, one order
        want = D.induced_restated(*G["host_csr"], i, n)
        assert sub.is_tensor() and sub.num_nodes == len(i) and np.array_equal(host(sub.edges), np.stack([want[0], want[1]], 1))
        assert np.array_equal(host(sub.node_feat["index"]), i) and np.array_equal(host(sub.node_feat["h"]), host(g.node_feat["h"])[i])
        cuts = np.flatnonzero(np.diff(part[i]) != 0)
        assert len(cuts) <= 2 and all((np.diff(c) > 0).all() for c in np.split(i, cuts + 1))          # cluster ranges, ascending inside
    second = [host(i) for _, i in a]                                                       # the next epoch draws its own order
    assert np.array_equal(np.sort(np.concatenate(second)), np.arange(n))
    assert any(not np.array_equal(x, y) for x, y in zip(ids, second))
    # the clustering Graph.reorder computes: order[new_id] = old_id, clusters are consecutive new ids
    fixed = [host(i) for _, i in pgl.sampling.ClusterBatches(g, torch.as_tensor(part).cuda(), shuffle=False)]
    assert len(fixed) == 16 and np.array_equal(np.concatenate(fixed), np.argsort(part, kind="stable"))


def test_random_walk_subgraph_is_the_subgraph_of_the_walked_nodes(pgl, rmat14):
    G = rmat14
    g, n = G["g"], G["n"]
    roots = dev(np.random.default_rng(9).integers(0, n, 500))
    sub = pgl.sampling.random_walk_subgraph(g, roots, 4, seed=7)
    paths, _ = pgl.sampling.walks(g, roots, 4, seed=7)
    nodes = np.unique(host(paths)[host(paths) >= 0])
    assert len(nodes) > len(np.unique(host(roots)))
    assert np.array_equal(host(sub.node_feat["index"]), nodes) and sub.num_nodes == len(nodes)
    want = D.induced_restated(*G["host_csr"], nodes, n)
    assert np.array_equal(host(sub.edges), np.stack([want[0], want[1]], 1))
    again = pgl.sampling.random_walk_subgraph(g, roots, 4, seed=7)
    assert torch.equal(again.edges, sub.edges) and torch.equal(again.node_feat["index"], sub.node_feat["index"])
    other = pgl.sampling.random_walk_subgraph(g, roots, 4, seed=8)
    assert not torch.equal(other.node_feat["index"], sub.node_feat["index"])
