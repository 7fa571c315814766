"""CPU tests of host logic: C-ABI surface, numpy-mode Graph, partitioner, relabel, product/oracle
separation.  No GPU compute calls."""
import ast
import os
import re

import numpy as np
import pytest

import golden_vectors as G
import ref_ops as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    import pgl_amd
    L = pgl_amd._ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "pgl_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(pglamd_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 20
    for s in declared:
        assert hasattr(L, s), s
    assert sorted(pgl_amd._ffi.exported_symbols()) == declared
    assert L.pglamd_abi_version() == 4         # ABI 4 (round 6): per-call flags on pglamd_aggregate_ext, the wire-mirror entry points removed


def test_ctypes_signatures_match_the_header_prototypes():
    """Every prototype of include/pgl_amd.h is bound in pgl_amd/_ffi.py with the same number of parameters (a silent
    mismatch would shift every later argument of a call)."""
    import pgl_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgl_amd.h")).read(), flags=re.S)
    protos = re.findall(r"\b(pglamd_\w+)\s*\(([^;{]*?)\)\s*;", hdr)
    assert len(protos) >= 30
    for name, args in protos:
        n = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert name in pgl_amd._ffi._SIGNATURES, name
        assert len(pgl_amd._ffi._SIGNATURES[name][1]) == n, (name, n, len(pgl_amd._ffi._SIGNATURES[name][1]))
    assert set(pgl_amd._ffi._SIGNATURES) == {n for n, _ in protos}


def test_product_never_touches_the_oracle():
    """pgl_amd/ must not import, load or reference anything under oracle/."""
    bad = []
    for dp, _, fs in os.walk(os.path.join(ROOT, "pgl_amd")):
        for f in fs:
            if not f.endswith((".py", ".hip", ".cpp", ".hpp")):
                continue
            txt = open(os.path.join(dp, f)).read()
            if f.endswith(".py"):
                for node in ast.walk(ast.parse(txt)):
                    names = []
                    if isinstance(node, ast.Import):
                        names = [a.name for a in node.names]
                    elif isinstance(node, ast.ImportFrom):
                        names = [node.module or ""]
                    # `paddle` may only be named inside pgl_amd/compat (the product's own name layer over torch, whose files are
                    # held to the same no-oracle rule here); the engine proper must not depend on any paddle namespace
                    banned = ("ref_ops", "ref_native", "ref_python", "build_ref", "oracle") + \
                        (() if os.sep + "compat" in dp else ("paddle",))
                    bad += [(f, n) for n in names if n.split(".")[0] in banned]
            if re.search(r"oracle/(ref_|_ref|_build|paddle_stub)|libref_ops", txt):
                bad.append((f, "path reference"))
    assert not bad, bad


def test_gpu_ops_refuse_cpu_tensors():
    import torch
    import pgl_amd
    x = torch.zeros(4, 4)
    with pytest.raises(RuntimeError):
        pgl_amd.ops.gather_rows(x, torch.zeros(2, dtype=torch.int64))
    g = pgl_amd.Graph(edges=[(0, 1)], num_nodes=2)
    with pytest.raises(ValueError):
        g.send_recv(x)
    with pytest.raises(ValueError):
        g.send(lambda s, d, e: {}, src_feat={"h": x})
    with pytest.raises(ValueError):
        g.recv(lambda m: m, {})
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            g.tensor()


def test_numpy_graph_index_golden_and_reference(ref_native):
    import pgl_amd
    g = pgl_amd.Graph(edges=G.G1_EDGES, num_nodes=G.G1_N)
    ix = g.adj_dst_index
    for got, key in ((ix.degree, "degree"), (ix._sorted_v, "sorted_v"), (ix._sorted_u, "sorted_u"),
                     (ix._sorted_eid, "sorted_eid"), (ix._indptr, "indptr")):
        assert np.array_equal(got, G.G8[key]), key
    g5 = pgl_amd.Graph(edges=G.G5_EDGES, num_nodes=G.G5_N)
    assert np.array_equal(g5.indegree(), G.G5_INDEG) and np.array_equal(g5.outdegree(), G.G5_OUTDEG)
    assert np.array_equal(g5.indegree(nodes=[1, 2]), G.G5_INDEG[[1, 2]])
    g6 = pgl_amd.Graph(edges=G.G6_EDGES, num_nodes=G.G6_N)
    assert [set(a.tolist()) for a in g6.predecessor()] == G.G6_PRED
    assert [set(a.tolist()) for a in g6.successor()] == G.G6_SUCC
    pred, eid = g6.predecessor(nodes=[2], return_eids=True)
    assert set(pred[0].tolist()) == {0, 1} and set(eid[0].tolist()) == {1, 2}
    rng = np.random.default_rng(1)
    for n, e in ((1, 0), (9, 0), (50, 400), (20000, 300000)):
        edges = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)], 1).astype(np.int64) if e else np.zeros((0, 2), np.int64)
        got = pgl_amd.ops.host_build_index(edges[:, 1], edges[:, 0], n)         # strided columns
        ref = ref_native.build_index(edges[:, 1].copy(), edges[:, 0].copy(), n)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
    with pytest.raises(OverflowError):
        pgl_amd.ops.host_build_index(np.array([5]), np.array([0]), 3)


def test_graph_dump_load_roundtrip(tmp_path):
    import pgl_amd
    rng = np.random.default_rng(2)
    edges = np.stack([rng.integers(0, 30, 200), rng.integers(0, 30, 200)], 1)
    g = pgl_amd.Graph(edges=edges, num_nodes=30, node_feat={"h": rng.standard_normal((30, 3))},
                      edge_feat={"w": rng.standard_normal((200, 1))})
    g.indegree(); g.outdegree()
    g.dump(str(tmp_path / "g"))
    for name in ("degree", "sorted_u", "sorted_v", "sorted_eid", "indptr"):       # reference layout
        assert (tmp_path / "g" / "adj_dst" / (name + ".npy")).exists()
    h = pgl_amd.Graph.load(str(tmp_path / "g"))
    assert h.num_nodes == 30 and np.array_equal(h.edges, g.edges)
    assert np.array_equal(h.indegree(), g.indegree())
    assert np.array_equal(h.node_feat["h"], g.node_feat["h"]) and np.array_equal(h.edge_feat["w"], g.edge_feat["w"])
    assert "num_nodes" in repr(h)
    with pytest.raises(ValueError):
        g.sorted_edges("both")


def test_map_ids_matches_reference(ref_native):
    import pgl_amd
    reindex = {10: 0, 42: 1, 7: 2, 99: 3}
    nodes = np.array([42, 7, 7, 10, 99, 5], dtype=np.int64)       # 5 is absent -> 0, like operator[]
    assert np.array_equal(pgl_amd.ops.host_map_ids(nodes, reindex), ref_native.map_nodes(nodes, dict(reindex)))
    edges = np.array([[10, 42], [7, 99], [42, 42]], dtype=np.int64)
    ref = ref_native.map_edges(np.arange(3, dtype=np.int64), edges, dict(reindex))
    got = pgl_amd.ops.host_map_ids(edges.reshape(-1), reindex).reshape(-1, 2)
    assert np.array_equal(got, ref)


def _sym_simple(n, e, seed, communities=0):
    rng = np.random.default_rng(seed)
    if communities:
        size = n // communities
        a = rng.integers(0, n, e)
        same = rng.random(e) < 0.9
        b = np.where(same, (a // size) * size + rng.integers(0, size, e), rng.integers(0, n, e))
    else:
        a, b = rng.integers(0, n, e), rng.integers(0, n, e)
    keep = a != b
    a, b = a[keep], b[keep]
    und = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)
    return np.concatenate([und, und[:, ::-1]], 0).astype(np.int64)


@pytest.mark.parametrize("nparts", [2, 8])
def test_partitioner_balance_and_cut_vs_metis(ref_native, nparts, monkeypatch):
    """Engine's own partitioner (the product default) vs the reference's METIS (oracle/_ref) on a graph with planted
    communities: valid ids, balanced within 3 %, edge cut within 1.05x of METIS and far below random."""
    import pgl_amd
    n = 4000
    edges = _sym_simple(n, 40000, 4, communities=16)
    g = pgl_amd.Graph(edges=edges, num_nodes=n)
    ix = g.adj_dst_index
    with pytest.warns(UserWarning):
        part = pgl_amd.partition.metis_partition(g, nparts)
    assert part.dtype == np.int64 and part.shape == (n,) and part.min() >= 0 and part.max() == nparts - 1
    sizes = np.bincount(part, minlength=nparts)
    assert sizes.max() <= 1.03 * n / nparts + 1e-9
    cut = int((part[edges[:, 0]] != part[edges[:, 1]]).sum())
    metis = ref_native.metis_partition(n, ix._indptr, ix._sorted_v, nparts, None, None, False)
    cut_metis = int((metis[edges[:, 0]] != metis[edges[:, 1]]).sum())
    rnd = np.random.default_rng(0).integers(0, nparts, n)
    cut_rnd = int((rnd[edges[:, 0]] != rnd[edges[:, 1]]).sum())
    assert cut <= 1.05 * cut_metis, (cut, cut_metis)
    assert cut < 0.5 * cut_rnd
    # deterministic for a fixed seed
    with pytest.warns(UserWarning):
        assert np.array_equal(part, pgl_amd.partition.metis_partition(g, nparts))


@pytest.mark.parametrize("nparts", [2, 3, 8])
def test_weighted_partition_vs_the_reference_metis(ref_native, nparts):
    """pgl.partition.metis_partition with node and edge weights (pgl/partition.py:63-79: min-max scaled to positive ints): the
    engine's partitioner against the reference's compiled graph_kernel.metis_partition (oracle/_ref, the comparison partner --
    nothing of it is reachable from the product) on the same CSR and the same scaled weights: weighted cut <= 1.10x METIS's,
    weighted balance <= 1.05."""
    import pgl_amd
    n = 3000
    edges = _sym_simple(n, 30000, 21 + nparts, communities=12)
    g = pgl_amd.Graph(edges=edges, num_nodes=n)
    ix = g.adj_dst_index
    rng = np.random.default_rng(nparts)
    nw = rng.random(n)
    lo_, hi_ = np.minimum(edges[:, 0], edges[:, 1]), np.maximum(edges[:, 0], edges[:, 1])
    ew = (lo_ * 7919 + hi_ * 104729) % 1000 / 1000.0                  # symmetric: METIS checks w(u,v) == w(v,u)
    with pytest.warns(UserWarning):
        part = pgl_amd.partition.metis_partition(g, nparts, node_weights=nw, edge_weights=ew)
    scale = pgl_amd.partition._metis_weight_scale
    snw, sew = scale(nw), scale(ew)
    want = ref_native.metis_partition(n, ix._indptr, ix._sorted_v, nparts, snw, scale(ew[ix._sorted_eid]), False)
    wcut = lambda p_: float(sew[p_[edges[:, 0]] != p_[edges[:, 1]]].sum())
    assert wcut(part) <= 1.10 * wcut(want), (wcut(part), wcut(want))
    w = np.bincount(part, weights=snw, minlength=nparts)
    assert w.max() / w.mean() <= 1.05, w


def test_partition_weights_and_trivial_cases():
    import pgl_amd
    n = 600
    edges = _sym_simple(n, 5000, 6)
    g = pgl_amd.Graph(edges=edges, num_nodes=n)
    assert (pgl_amd.partition.metis_partition(g, 1) == 0).all()
    rng = np.random.default_rng(0)
    with pytest.warns(UserWarning):                                  # "can run" with float weights, as tests/test_partition.py:49-67
        p = pgl_amd.partition.metis_partition(g, 4, node_weights=rng.random(n), edge_weights=rng.random(len(edges)))
    assert set(np.unique(p)) == {0, 1, 2, 3}
    w = pgl_amd.partition._metis_weight_scale(np.array([0.0, 0.5, 1.0]))
    assert w.dtype == np.int64 and w.min() == 1 and w.max() == 1000
    r = pgl_amd.partition.random_partition(g, 4)
    assert np.bincount(r).max() - np.bincount(r).min() <= 1
    assert (pgl_amd.partition.random_partition(g, 1) == 0).all()


def test_rmat_generator_is_deterministic():
    from pgl_amd.utils.rmat import rmat_edges
    a = rmat_edges(10, 5000, seed=42); b = rmat_edges(10, 5000, seed=42)
    assert a.shape == (5000, 2) and bool((a == b).all()) and int(a.max()) < 1024 and int(a.min()) >= 0
    deg = np.bincount(a[:, 1].numpy(), minlength=1024)
    assert deg.max() > 20 * max(1, int(np.median(deg)))              # power-law skew


def test_host_sampling_and_graphsage_sample():
    """numpy-mode sampling path of examples/graphsage (pgl/sampling/sage.py:59-127, custom.py:23-83)."""
    import pgl_amd
    rng = np.random.default_rng(3)
    n = 300
    edges = np.unique(np.stack([rng.integers(0, n, 4000), rng.integers(0, n, 4000)], 1), axis=0).astype(np.int64)
    g = pgl_amd.Graph(edges=edges, num_nodes=n, node_feat={"h": rng.standard_normal((n, 4)).astype(np.float32)})
    np.random.seed(0)
    preds, eids = g.sample_predecessor([5, 6, 7], 3, return_eids=True)
    for v, p, e in zip([5, 6, 7], preds, eids):
        assert len(p) == min(3, int(g.indegree()[v])) and len(set(e.tolist())) == len(e)
        assert (edges[e, 1] == v).all() and np.array_equal(edges[e, 0], p)
    succ = g.sample_successor([1], 1000)
    assert sorted(succ[0].tolist()) == sorted(edges[edges[:, 0] == 1, 1].tolist())
    batch = [0, 1, 2, 3]
    layers = pgl_amd.sampling.graphsage_sample(g, batch, [4, 4])
    assert len(layers) == 2
    for sg, sample_index, node_index in layers:
        assert sg.num_nodes == len(sample_index) and np.array_equal(sample_index[node_index], np.array(batch))
        se = sample_index[sg.edges]                                  # every sampled edge is a real edge
        real = {tuple(x) for x in edges.tolist()}
        assert all(tuple(x) in real for x in se.tolist())
        assert np.array_equal(sg.node_feat["h"], g.node_feat["h"][sample_index])
    assert layers[0][0].num_edges >= layers[1][0].num_edges          # outer layer sees more edges
    sub = pgl_amd.sampling.subgraph(g, nodes=[3, 9, 27], edges=[(3, 9), (27, 3)])
    assert sub.edges.tolist() == [[0, 1], [2, 0]]


def test_bench_and_entry_scripts_import_cleanly():
    """bench.py parses its arguments (argparse exits 0 on --help before touching a GPU) and __graft_entry__ exposes
    build() / smoke(): a broken import in either would only show up on the GPU box otherwise."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--steps" in r.stdout and "--warmup" in r.stdout, r.stderr[-2000:]
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    assert callable(ge.build) and callable(ge.smoke)


def test_bench_options_and_output_dump(tmp_path):
    """bench.py offers --full and --dump-outputs and refuses --steps 0; its dump of an output larger than the budget is a fixed
    seeded row sample (the same rows every run, with their ids) plus every row's float64 sum, inside the budget."""
    import subprocess
    import sys
    import torch
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr[-2000:]
    sys.path.insert(0, ROOT)
    import bench
    out = torch.randn(5000, 16, generator=torch.Generator().manual_seed(3))
    ids = torch.arange(5000) * 3
    budget = 256 << 10
    for sub in ("a", "b"):
        n = bench.dump_outputs(str(tmp_path / sub), out, ids, budget=budget)
        assert n <= budget
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["send_recv_sum_row_ids.npy", "send_recv_sum_row_sums.npy", "send_recv_sum_rows.npy"]
    for f in names:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    rows = np.load(str(tmp_path / "a" / "send_recv_sum_rows.npy"))
    pick = np.load(str(tmp_path / "a" / "send_recv_sum_row_ids.npy")).astype(np.int64) // 3
    assert 0 < len(pick) < 5000 and np.array_equal(rows, out.numpy()[pick])
    sums = np.load(str(tmp_path / "a" / "send_recv_sum_row_sums.npy"))
    assert np.allclose(sums, out.double().sum(1).numpy())
    assert bench.dump_outputs(str(tmp_path / "c"), out[:10], ids[:10], budget=budget) == 10 * (16 * 4 + 8)
    assert np.array_equal(np.load(str(tmp_path / "c" / "send_recv_sum.npy")), out[:10].numpy())


def test_no_metis_code_reachable_from_the_product():
    """the round-3/4 opt-in METIS bridge is gone -- libpglamd exports no METIS entry point, the header declares
    none, no helper library is built or opened, and PGLAMD_PARTITIONER has no effect (the reference's METIS is a comparison
    partner of the tests through oracle/_ref only)."""
    import subprocess
    import pgl_amd
    lib = os.path.join(ROOT, "pgl_amd", "csrc", "libpglamd.so")
    syms = subprocess.run(["nm", "-D", lib], capture_output=True, text=True).stdout.lower()
    assert "metis" not in syms
    assert "metis_partition" not in open(os.path.join(ROOT, "include", "pgl_amd.h")).read().replace("pgl.partition.metis_partition", "").replace("graph_kernel.metis_partition", "")
    assert not os.path.exists(os.path.join(ROOT, "pgl_amd", "_build_metis.py"))
    assert not hasattr(pgl_amd.ops, "host_partition_metis") and not hasattr(pgl_amd.ops, "metis_available")
    g = pgl_amd.Graph(edges=np.array([[0, 1], [1, 0], [2, 3], [3, 2], [1, 2], [2, 1]]), num_nodes=4)
    os.environ["PGLAMD_PARTITIONER"] = "metis"
    try:
        with pytest.warns(UserWarning):
            part = pgl_amd.partition.metis_partition(g, 2)
    finally:
        del os.environ["PGLAMD_PARTITIONER"]
    assert sorted(np.bincount(part, minlength=2).tolist()) == [2, 2]


def test_engine_partitioner_degenerate_inputs():
    """The partitioner is on the default path of every multi-GPU run: empty graphs, more parts than nodes, isolated nodes, self
    loops, stars, duplicate edges, zero and dominant vertex weights must give valid part ids (and the obvious answers where there
    is one), and bad node ids must be refused."""
    import pgl_amd
    P = pgl_amd.ops.host_partition_edges

    def run(e, n, k, **kw):
        e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
        part, cut = P(e, n, k, **kw)
        assert part.shape == (n,) and part.dtype == np.int64
        if n:
            assert part.min() >= 0 and part.max() < max(min(k, n), 1)
        assert cut == (int((part[e[:, 0]] != part[e[:, 1]]).sum()) if len(e) else 0) or len(np.unique(e, axis=0)) != len(e)
        return part
    assert run([], 0, 4).size == 0
    assert run([], 1, 4).tolist() == [0]
    assert sorted(np.bincount(run([], 10, 3), minlength=3).tolist()) == [3, 3, 4]          # isolated nodes level the parts
    assert sorted(run([[0, 1], [1, 2]], 3, 8).tolist()) == [0, 1, 2]                         # k > n: one node per part
    assert (run([[0, 1], [1, 2]], 3, 1) == 0).all()
    assert np.bincount(run([[i, i] for i in range(20)], 20, 4), minlength=4).tolist() == [5, 5, 5, 5]   # self loops are no edges
    star = run([[0, i] for i in range(1, 2000)], 2000, 8)
    assert np.bincount(star, minlength=8).max() <= 1.03 * 250 + 1
    two = [[a, b] for a in range(50) for b in range(50) if a != b] + [[50 + a, 50 + b] for a in range(50) for b in range(50) if a != b] + [[0, 50]]
    p = run(two, 100, 2)
    assert len(set(p[:50].tolist())) == 1 and len(set(p[50:].tolist())) == 1 and p[0] != p[50]   # two cliques, one bridge
    run([[0, 1]] * 1000 + [[1, 2]] * 10, 3, 2)
    rng = np.random.default_rng(0)
    e = rng.integers(0, 500, (5000, 2))
    run(e, 500, 4, node_weights=np.zeros(500, np.int64))
    run(e, 500, 4, node_weights=np.r_[10 ** 9, np.ones(499, np.int64)])
    p = run(rng.integers(0, 5000, (60000, 2)), 5000, 7, node_weights=rng.integers(1, 50, 5000), node_weights2=np.ones(5000, np.int64), ub=1.03, ub2=1.1)
    assert np.bincount(p, minlength=7).max() <= 1.1 * 5000 / 7 + 1
    with pytest.raises((OverflowError, ValueError)):
        P(np.array([[0, 5]]), 3, 2)


# ------------------------------------------------------------------------------------------------
# classifier-head pieces (pgl_amd.nn.Linear / nn.functional.cross_entropy, behind compat paddle.nn.Linear / cross_entropy)
# ------------------------------------------------------------------------------------------------
def test_engine_cross_entropy_and_linear_equal_torch():
    """Same values and gradients as torch.nn.functional.cross_entropy / torch.nn.Linear: what changes is how the gradients of
    inputs with millions of rows are reduced (split reductions instead of one 64-workgroup pass)."""
    import torch
    import torch.nn.functional as F
    import pgl_amd as pgl
    from pgl_amd import autograd as ag
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3000, 41, generator=g, requires_grad=True)
    y = torch.randint(0, 41, (3000,), generator=g)
    y[::7] = -100
    for red in ("mean", "sum", "none"):
        a = pgl.nn.functional.cross_entropy(x, y, reduction=red)
        b = F.cross_entropy(x, y, reduction=red, ignore_index=-100)
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6), red
        ga, = torch.autograd.grad(a.sum(), x)
        gb, = torch.autograd.grad(b.sum(), x)
        assert torch.allclose(ga, gb, rtol=1e-5, atol=1e-7), red
    big = torch.randn(70001, 24, generator=g)
    assert torch.allclose(ag.column_sum(big), big.sum(0), rtol=1e-4, atol=1e-3)
    torch.manual_seed(1)
    lin = pgl.nn.Linear(24, 5)
    ref = torch.nn.Linear(24, 5)
    ref.load_state_dict(lin.state_dict())
    xin = big.clone().requires_grad_(True)
    xref = big.clone().requires_grad_(True)
    cot = torch.randn(70001, 5, generator=g)
    (lin(xin) * cot).sum().backward()
    (ref(xref) * cot).sum().backward()
    assert torch.allclose(xin.grad, xref.grad, rtol=1e-5, atol=1e-6)
    assert torch.allclose(lin.weight.grad, ref.weight.grad, rtol=1e-4, atol=1e-2)
    assert torch.allclose(lin.bias.grad, ref.bias.grad, rtol=1e-4, atol=1e-2)


def test_graph_reorder_is_a_consistent_relabelling():
    """Graph.reorder (engine extension, round 4): order is a permutation, graph2's edge k is edge k with both endpoints renamed,
    node features follow their nodes, edge features stay; a graph with planted clusters ends up with its clusters contiguous."""
    import pgl_amd
    rng = np.random.default_rng(5)
    n, e, c = 8192, 120000, 8
    src = rng.integers(0, n, e)
    dst = np.where(rng.random(e) < 0.9, (src // (n // c)) * (n // c) + rng.integers(0, n // c, e), rng.integers(0, n, e))
    perm = rng.permutation(n)
    edges = np.stack([perm[src], perm[dst]], 1).astype(np.int64)
    feat = rng.standard_normal((n, 3)).astype(np.float32)
    w = rng.standard_normal((e, 1)).astype(np.float32)
    g = pgl_amd.Graph(edges=edges, num_nodes=n, node_feat={"h": feat}, edge_feat={"w": w})
    g2, order = g.reorder(num_clusters=c)
    assert sorted(order.tolist()) == list(range(n))
    new_of_old = np.empty(n, np.int64); new_of_old[order] = np.arange(n)
    assert np.array_equal(g2.edges, new_of_old[edges])
    assert np.array_equal(g2.node_feat["h"], feat[order]) and np.array_equal(g2.edge_feat["w"], w)
    blk = n // c
    before = ((edges[:, 0] // blk) == (edges[:, 1] // blk)).mean()
    after = ((g2.edges[:, 0] // blk) == (g2.edges[:, 1] // blk)).mean()
    assert before < 0.2 and after > 0.8, (before, after)
    assert np.array_equal(g2.indegree(), g.indegree()[order])


# ------------------------------------------------------------------------------------------------
# round 5: EdgeTensor (pgl_amd/edge_tensor.py) -- the wrapper's own logic, on CPU with a stand-in view (the kernels that
# produce / consume the sorted rows are covered by the GPU tests)
# ------------------------------------------------------------------------------------------------
class _FakeView(object):
    def __init__(self, perm):
        import torch
        self.graph = object()
        self.eid = torch.as_tensor(perm)                    # original edge id of sorted position p
        self.inv = torch.empty_like(self.eid)
        self.inv[self.eid] = torch.arange(len(perm))
        self.calls = 0

    def from_order(self, rows):
        self.calls += 1
        return rows[self.inv]

    def to_order(self, rows):
        return rows[self.eid]


def test_edge_tensor_keeps_the_tag_through_elementwise_work_and_reads_back_in_original_order():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from pgl_amd.edge_tensor import EdgeTensor
    rng = np.random.default_rng(0)
    E, H, D = 50, 4, 3
    orig = torch.as_tensor(rng.standard_normal((E, H, D)).astype(np.float32))
    view = _FakeView(rng.permutation(E))
    et = EdgeTensor(orig[view.eid], view)                   # rows in "sorted" order
    attn = torch.as_tensor(rng.standard_normal((1, H, D)).astype(np.float32))
    # the GATv2-style chain (pgl/nn/conv.py:421-424): leaky_relu -> * attn -> sum over the last dim -> reshape -> dropout(p=0)
    a = nn.LeakyReLU(0.2)(et)
    a = torch.sum(a * attn, dim=-1)
    a = (2.0 * a + 1.0).reshape(-1, H, 1)
    a = nn.Dropout(p=0.0)(a)
    a = torch.tanh(a) * torch.exp(-a.abs())
    assert isinstance(a, EdgeTensor) and view.calls == 0 and tuple(a.shape) == (E, H, 1)
    ref = (2.0 * torch.sum(F.leaky_relu(orig, 0.2) * attn, dim=-1) + 1.0).reshape(-1, H, 1)
    ref = torch.tanh(ref) * torch.exp(-ref.abs())
    assert torch.allclose(a.materialize(), ref) and view.calls == 1
    assert torch.allclose(a.materialize(), ref) and view.calls == 1        # cached
    # tensor-on-the-left arithmetic and EdgeTensor (x) EdgeTensor of the same view keep the tag
    b = attn.reshape(1, H, D) * et + et
    assert isinstance(b, EdgeTensor) and torch.allclose(b.materialize(), attn * orig + orig)
    # anything that looks at rows by position gets ORIGINAL order: indexing, sum over the edge dimension, cat, cpu / numpy, comparison
    assert torch.equal(et[3], orig[3]) and torch.equal(et[5:9], orig[5:9])
    assert torch.allclose(et.sum(0), orig.sum(0)) and torch.allclose(torch.sum(et), orig.sum()) and torch.allclose(et.sum(), orig.sum())
    assert torch.equal(torch.cat([et, et], 0), torch.cat([orig, orig], 0))
    assert np.array_equal(et.detach().cpu().numpy(), orig.numpy()) and np.array_equal(np.asarray(et), orig.numpy())
    assert bool((et == orig).all()) and torch.equal(et.reshape(E * H, D), orig.reshape(E * H, D))
    assert not isinstance(et.reshape(E * H, D), EdgeTensor) and isinstance(et.reshape(E, -1), EdgeTensor) and isinstance(et.reshape(-1, H * D), EdgeTensor)
    # a per-EDGE operand (size E in dim 0) cannot be combined without knowing the order: the result is an ordinary original-order tensor
    w = torch.as_tensor(rng.standard_normal((E, 1, 1)).astype(np.float32))
    c = et * w
    assert not isinstance(c, EdgeTensor) and torch.allclose(c, orig * w)
    # two views never mix silently
    other = EdgeTensor(orig[view.eid], _FakeView(rng.permutation(E)))
    assert not isinstance(et + other, EdgeTensor)
    # gradients flow through the permutation
    leaf = orig.clone().requires_grad_(True)
    e2 = EdgeTensor(leaf[view.eid], view)
    (torch.tanh(e2) * 3.0).materialize().square().sum().backward()
    l2 = orig.clone().requires_grad_(True)
    (torch.tanh(l2) * 3.0).square().sum().backward()
    assert torch.allclose(leaf.grad, l2.grad)
    # the engine's kernels refuse the wrapper instead of reading sorted rows as if they were in original order
    import pgl_amd
    with pytest.raises(TypeError, match="EdgeTensor"):
        pgl_amd.ops.gather_rows(et, torch.zeros(1, dtype=torch.int64))


def test_edge_tensor_writes_reach_the_sorted_rows():
    """in-place Tensor methods, item assignment and out= go through the original-order copy; the destination-sorted rows
    the engine's ops consume must follow, and an [E, ...] tensor handed to an element-wise call as an EXTRA operand
    (torch.clamp(t, min=<original-order tensor>)) must not be combined with the sorted rows."""
    import torch
    from pgl_amd.edge_tensor import EdgeTensor
    rng = np.random.default_rng(1)
    E, H = 40, 4
    orig = torch.as_tensor(rng.standard_normal((E, H)).astype(np.float32))
    view = _FakeView(rng.permutation(E))
    mk = lambda: EdgeTensor(orig[view.eid].clone(), view)
    et = mk(); r = et.mul_(2.0)
    assert r is et and torch.equal(et.sorted_rows(), (orig * 2.0)[view.eid]) and torch.equal(et.materialize(), orig * 2.0)
    et = mk(); et.clamp_(min=0.0)
    assert torch.equal(et.sorted_rows(), orig.clamp(min=0.0)[view.eid])
    mask = torch.as_tensor(rng.random((E, H)) < 0.3)                    # an original-order mask
    et = mk(); et.masked_fill_(mask, -1.0)
    assert torch.equal(et.sorted_rows(), orig.masked_fill(mask, -1.0)[view.eid])
    et = mk(); et[3] = 7.0; et[5:8] = torch.zeros(3, H)
    want = orig.clone(); want[3] = 7.0; want[5:8] = 0.0
    assert torch.equal(et.sorted_rows(), want[view.eid]) and torch.equal(et.materialize(), want)
    et = mk(); torch.add(orig, 1.0, out=et)
    assert torch.equal(et.sorted_rows(), (orig + 1.0)[view.eid])
    et = mk(); et.copy_(mk() * 3.0)
    assert torch.equal(et.sorted_rows(), (orig * 3.0)[view.eid])
    # extra [E, ...] operands are in ORIGINAL order: never applied to the sorted rows
    lo = torch.as_tensor(rng.standard_normal((E, H)).astype(np.float32))
    for got in (torch.clamp(mk(), min=lo), mk().clamp(min=lo), torch.add(mk(), 1.0, alpha=2.0)):
        pass
    assert torch.equal(materialize_(torch.clamp(mk(), min=lo)), torch.clamp(orig, min=lo))
    assert torch.equal(materialize_(mk().clamp(min=lo)), orig.clamp(min=lo))
    assert isinstance(torch.clamp(mk(), min=0.0), EdgeTensor) and isinstance(torch.add(mk(), 1.0, alpha=2.0), EdgeTensor)
    assert isinstance(mk().clamp(min=torch.zeros(1, H)), EdgeTensor)     # broadcasts over the edges: order-free


def materialize_(t):
    from pgl_amd.edge_tensor import materialize
    return materialize(t)


def test_edge_tensor_row_wise_ops_keep_the_tag():
    """cat along a trailing dim, matmul / linear with the weight on the right, softmax / normalize over a trailing dim: every output
    row depends on its own input row only, so they are applied to the sorted rows (the UDF message functions of TransformerConv,
    PinSage, ... use them)."""
    import torch
    import torch.nn.functional as F
    from pgl_amd.edge_tensor import EdgeTensor
    rng = np.random.default_rng(1)
    E, D = 40, 6
    orig = torch.as_tensor(rng.standard_normal((E, D)).astype(np.float32))
    view = _FakeView(rng.permutation(E))
    a, b = EdgeTensor(orig[view.eid], view), EdgeTensor((orig * 2)[view.eid], view)
    W, bias = torch.as_tensor(rng.standard_normal((D, 4)).astype(np.float32)), torch.as_tensor(rng.standard_normal(4).astype(np.float32))
    c = torch.cat([a, b], dim=-1)
    assert isinstance(c, EdgeTensor) and torch.equal(c.materialize(), torch.cat([orig, orig * 2], -1)) and view.calls == 1
    m = torch.matmul(a, W); l = F.linear(a, W.t(), bias); s = F.softmax(a, dim=-1); nm = F.normalize(a, dim=1)
    for got, want in ((m, orig @ W), (l, orig @ W + bias), (s, F.softmax(orig, -1)), (nm, F.normalize(orig, dim=1)), (a @ W, orig @ W)):
        assert isinstance(got, EdgeTensor) and torch.allclose(got.materialize(), want, atol=1e-6)
    # along the EDGE dimension these are not row-wise: original order first
    assert not isinstance(torch.cat([a, b], 0), EdgeTensor) and torch.equal(torch.cat([a, b], 0), torch.cat([orig, orig * 2], 0))
    assert not isinstance(F.softmax(a, dim=0), EdgeTensor) and torch.allclose(F.softmax(a, dim=0), F.softmax(orig, 0))
    assert not isinstance(torch.matmul(W.t()[:, :D] @ torch.eye(D), a.materialize().t()), EdgeTensor)


def test_graph_tensor_accepts_the_reference_uva_argument():
    """pgl/graph.py:227: tensor(self, inplace=True, uva=False) -- uva is the reference's second positional argument."""
    import inspect
    import torch
    import pgl_amd
    for cls in (pgl_amd.Graph, pgl_amd.BiGraph):
        params = list(inspect.signature(cls.tensor).parameters)
        assert params[:3] == ["self", "inplace", "uva"], (cls.__name__, params)
    g = pgl_amd.Graph(edges=np.array([[0, 1], [1, 2]], np.int64), num_nodes=3)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="uva"):
            g.tensor(True, True)


# ------------------------------------------------------------------------------------------------
# ops.CSR, the one index type: every field set at construction, views share tensors, edge-row indices skip the hub plan
# ------------------------------------------------------------------------------------------------
def _cpu_csr():
    import torch
    from pgl_amd import ops
    indptr = torch.tensor([0, 2, 3, 6])
    return ops.CSR(indptr, torch.tensor([0, 0, 1, 2, 2, 2], dtype=torch.int32), torch.tensor([1, 2, 0, 0, 1, 2], dtype=torch.int32),
                   torch.arange(6, dtype=torch.int32), 3, 6, degree=indptr[1:] - indptr[:-1])


def test_csr_sets_every_field_at_construction():
    from pgl_amd import ops
    c = _cpu_csr()
    for k in ops.CSR.__slots__:
        getattr(c, k)                                   # an unset slot raises AttributeError
    assert (c.num_nodes, c.num_edges, c.max_row, c.y_rows, c.edge_rows) == (3, 6, 0, 0, False)
    assert c.sorted_u is None and c.sorted_v is None and c.sorted_eid is None
    assert c._hub is None and c._es is None and c._pos_by_dst is None


def test_csr_view_shares_the_unreplaced_tensors_and_starts_with_empty_caches():
    import torch
    c = _cpu_csr()
    c.max_row = 3
    c._hub, c._es, c._pos_by_dst = {(1024, 3): None}, ("key", None, None), (c, None)
    col = torch.tensor([5, 4, 3, 2, 1, 0], dtype=torch.int32)
    v = c.view(col32=col, edge_rows=True)
    assert v is not c and v.col32 is col and v.edge_rows and not c.edge_rows
    for k in ("indptr", "row32", "eid32", "degree"):
        assert getattr(v, k) is getattr(c, k), k
    assert (v.num_nodes, v.num_edges, v.max_row, v.y_rows) == (3, 6, 3, 0)
    assert v._hub is None and v._es is None and v._pos_by_dst is None
    assert c._hub and c._es is not None and c._pos_by_dst is not None          # the parent keeps its own


def test_csr_without_columns_is_an_edge_row_index():
    from pgl_amd import ops
    c = _cpu_csr()
    assert c.view(col32=None).edge_rows
    assert ops.CSR(c.indptr, c.row32, None, None, 3, 6).edge_rows
    s = ops.SegView(c.indptr, c.row32, c.row32, None).as_csr(6)
    assert s.edge_rows and s.col32 is None and s.indptr is c.indptr and (s.num_nodes, s.num_edges) == (3, 6)


def test_hub_gate_turns_edge_row_indices_away_before_any_device_work(monkeypatch):
    import inspect
    import torch
    from pgl_amd import ops

    class Untouchable(object):
        def __getattr__(self, name):
            raise AssertionError("col32.%s read" % name)

    def no_cuda(*a, **k):
        raise AssertionError("torch.cuda called")
    for name, f in inspect.getmembers(torch.cuda, inspect.isfunction):
        monkeypatch.setattr(torch.cuda, name, no_cuda)
    planned = []
    monkeypatch.setattr(ops, "hub_plan", lambda csr, n_src, row_bytes: planned.append(csr))
    monkeypatch.setattr(ops, "_HUB_TABLE", True)
    monkeypatch.setattr(ops, "_HUB_MIN_EDGES", 0)
    x = torch.zeros(8192, 128)                          # plain fp32 rows of 512 bytes: eligible by shape
    c = _cpu_csr()
    for e in (c.view(col32=Untouchable(), edge_rows=True), c.view(col32=None), ops.SegView(c.indptr, c.row32, c.row32).as_csr(6)):
        assert ops.hub_table(e, x) is None
    assert planned == []
    ops.hub_table(c, x)                                 # the same shapes over node columns do reach the plan
    assert planned == [c]


# ------------------------------------------------------------------------------------------------
# ops._aggregate_route: which entry point and which scale form an aggregate() call takes -- decided from shapes alone
# ------------------------------------------------------------------------------------------------
_ROUTE_OPTIONS = ("plain", "x2", "zero_indptr", "max_row", "deal_chunks", "strided_x", "strided_out")


def _route_case(option, scaled, with_y, dtype, reduce_op, d, csr=None):
    """-> (args of ops._aggregate_route, row bytes) for one cell of the option cross over the 3-node index of _cpu_csr()."""
    import torch
    c = _cpu_csr() if csr is None else csr
    n, m = 3, 5
    x = torch.zeros(n, d + 16, dtype=dtype)[:, 8:8 + d] if option == "strided_x" else torch.zeros(n, d, dtype=dtype)
    out = torch.zeros(m, d + 8, dtype=dtype)[:, 4:4 + d] if option == "strided_out" else None
    args = dict(x=x, csr=c.view(max_row=3) if option == "max_row" else c, y=torch.zeros(6, 1, dtype=dtype) if with_y else None,
                src_scale=torch.ones(n) if scaled else None, x2=torch.zeros(2, d, dtype=dtype) if option == "x2" else None,
                zero_indptr=c.indptr.clone() if option == "zero_indptr" else None, out=out, reduce_op=reduce_op,
                deal_chunks=option == "deal_chunks")
    return args, d * x.element_size()


def _route_cross():
    import itertools
    import torch
    return itertools.product(_ROUTE_OPTIONS, (False, True), (False, True), (torch.float32, torch.float64), ("sum", "max"), (8, 33, 192))


@pytest.fixture
def route_without_device(monkeypatch):
    """ops._aggregate_route with torch.cuda and the library out of reach: the route is decided on the host from CPU tensors."""
    import inspect
    import torch
    from pgl_amd import _ffi, ops

    def no_cuda(*a, **k):
        raise AssertionError("torch.cuda called")

    def no_lib():
        raise AssertionError("library opened")
    for name, f in inspect.getmembers(torch.cuda, inspect.isfunction):
        monkeypatch.setattr(torch.cuda, name, no_cuda)
    monkeypatch.setattr(_ffi, "lib", no_lib)
    monkeypatch.setattr(ops, "_EDGE_SCALE", True)
    monkeypatch.setattr(ops, "_PRESCALE_ROW_BYTES", 704)
    return ops._aggregate_route


def test_aggregate_route_invariants_hold_over_the_option_cross(route_without_device):
    import torch
    from pgl_amd import ops
    route, seen = route_without_device, set()
    for option, scaled, with_y, dtype, reduce_op, d in _route_cross():
        args, row_bytes = _route_case(option, scaled, with_y, dtype, reduce_op, d)
        what = (option, scaled, with_y, dtype, reduce_op, d)
        if option == "x2" and scaled:
            with pytest.raises(ValueError, match="x2 must have x's dtype and row shape, and excludes src_scale"):
                route(**args)
            continue
        # the scale form does not depend on zero_indptr: ask without it, then demand the refusal of the fused form with it
        form = route(**dict(args, zero_indptr=None)).scale
        if option == "zero_indptr" and form == "fused":
            with pytest.raises(ValueError, match="aggregate: zero_indptr excludes a fused src_scale"):
                route(**args)
            seen.add("refused")
            continue
        r = route(**args)
        seen.add((r.entry, r.scale))
        assert isinstance(r, ops.AggregateRoute) and r.scale == form, what
        assert (r.scale is None) == (not scaled), what
        plain_operands = not scaled and not with_y and option != "x2"
        assert r.ldx == (args["x"].stride(0) if option == "strided_x" and plain_operands else 0), what
        assert r.ldo == (args["out"].stride(0) if option == "strided_out" and plain_operands else 0), what
        ext_option = option in ("x2", "zero_indptr", "max_row", "deal_chunks") or r.ldx > 0 or r.ldo > 0
        assert (r.entry == "aggregate_ext") == (ext_option and r.scale != "fused"), what
        assert r.entry in ("aggregate", "aggregate_ext"), what
        if r.scale == "fused":
            assert r.ldx == 0 and r.ldo == 0, what
        if r.scale == "edge":
            assert dtype == torch.float32 and reduce_op in ("sum", "mean") and row_bytes > 128 and not with_y and option != "x2", what
        if r.scale == "prescale":
            assert row_bytes <= 704 and not with_y, what
        if with_y and scaled:
            assert r.scale == "fused", what
    # every form and both entry points were reached, with and without a scale
    assert seen >= {"refused", ("aggregate", None), ("aggregate_ext", None), ("aggregate", "edge"), ("aggregate_ext", "edge"),
                    ("aggregate", "prescale"), ("aggregate_ext", "prescale"), ("aggregate", "fused")}
    assert ("aggregate_ext", "fused") not in seen


def test_aggregate_route_scale_forms_by_width_dtype_and_reduce(route_without_device, monkeypatch):
    import torch
    from pgl_amd import ops
    route = route_without_device
    form = lambda dtype, reduce_op, d, **kw: route(**_route_case("plain", True, False, dtype, reduce_op, d, **kw)[0]).scale
    assert form(torch.float32, "sum", 33) == "edge"                 # 132-byte fp32 rows, sum
    assert form(torch.float32, "sum", 192) == "edge"
    assert form(torch.float32, "sum", 8) == "prescale"              # 32 bytes: not wider than 128
    assert form(torch.float64, "sum", 8) == "prescale"
    assert form(torch.float32, "max", 33) == "prescale"             # max: never the edge form; 132 <= 704 bytes
    assert form(torch.float32, "max", 192) == "fused"               # 768-byte rows
    assert form(torch.float64, "sum", 192) == "fused"               # 1536-byte non-fp32 rows
    assert form(torch.int32, "sum", 8) == "fused"                   # integer rows are never multiplied in place
    edge_rows = _cpu_csr().view(edge_rows=True)
    assert form(torch.float32, "sum", 33, csr=edge_rows) == "prescale"      # an index over edge rows has no per-source layout
    assert form(torch.float32, "sum", 192, csr=edge_rows) == "fused"
    monkeypatch.setattr(ops, "_EDGE_SCALE", False)                  # switched off: the edge cases fall to the other two by width
    for option, scaled, with_y, dtype, reduce_op, d in _route_cross():
        if not scaled or option in ("x2", "zero_indptr"):
            continue
        args, row_bytes = _route_case(option, scaled, with_y, dtype, reduce_op, d)
        monkeypatch.setattr(ops, "_EDGE_SCALE", True)
        on = route(**args)
        monkeypatch.setattr(ops, "_EDGE_SCALE", False)
        off = route(**args)
        want = ("prescale" if row_bytes <= 704 else "fused") if on.scale == "edge" else on.scale
        assert off.scale == want and (off.ldx, off.ldo) == (on.ldx, on.ldo), (option, with_y, dtype, reduce_op, d)
    assert form(torch.float32, "sum", 33) == "prescale" and form(torch.float32, "sum", 192) == "fused"


def test_aggregate_route_turns_away_what_no_entry_point_computes(route_without_device):
    import torch
    route = route_without_device
    args, _ = _route_case("x2", False, False, torch.float32, "sum", 8)
    assert route(**args).entry == "aggregate_ext"
    for bad in (torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 9)):
        with pytest.raises(ValueError, match="x2 must have x's dtype and row shape"):
            route(**dict(args, x2=bad))
    # zero_indptr with a scale the route can take out of the kernel is served; with a fused one it was silently dropped before
    for d, reduce_op, with_y, refused in ((8, "sum", False, False), (33, "sum", False, False), (192, "sum", False, False),
                                          (192, "max", False, True), (8, "sum", True, True)):
        args, _ = _route_case("zero_indptr", True, with_y, torch.float32, reduce_op, d)
        if refused:
            with pytest.raises(ValueError, match="zero_indptr excludes a fused src_scale"):
                route(**args)
        else:
            assert route(**args).entry == "aggregate_ext"
