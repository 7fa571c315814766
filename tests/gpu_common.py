"""Shared fixtures and helpers of the GPU parity tests (tests/test_a*.py, test_f*.py), collected from the round-named files in round 6.

Error bars: no tolerance here is tied to max|want|.  Integer / index work is bit-exact.  An fp32 aggregation is held
PER ELEMENT to the re-association bound of its own terms: any order of summing n fp32 terms t_i lies within n * eps32 * sum|t_i| of the
exact sum (Higham, Accuracy and Stability, 4.4) -- `assert_within_fp32_reassociation` against an fp64 evaluation, `close_terms` against
the oracle's fp32 result (two fp32 evaluations of the same sum differ by at most twice that).  So an output element 100x smaller than the
largest one is held to an error 100x smaller, as north_star's "1e-5 relative" says."""
import numpy as np
import pytest
import torch

import ref_ops as R
from grad_defs import _dense_gat_fp64          # noqa: F401  (the edge-by-edge fp64 GAT formulation lives with the other definitions)


RTOL = 1e-5


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    arch = pgl_amd._ffi.lib().pglamd_device_arch().decode()
    assert arch.startswith("gfx950"), "libpglamd sees %r, expected gfx950" % arch
    return pgl_amd


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


EPS = {np.dtype(np.float32): float(np.finfo(np.float32).eps), np.dtype(np.float64): float(np.finfo(np.float64).eps),
       np.dtype(np.float16): float(np.finfo(np.float32).eps)}      # 16-bit STORAGE accumulates in fp32 (the output rounding is added separately)


def reassociation_bound(abs_terms, n_terms, slack=4.0, eps=None):
    """n * eps * sum|t_i|, per output element (Higham 4.4, first order); `slack` covers the rounding of the terms themselves
    (a product, a division by the degree, a scale)."""
    eps = EPS[np.dtype(np.float32)] if eps is None else eps
    return slack * np.maximum(np.asarray(n_terms, np.float64), 1.0) * eps * np.asarray(abs_terms, np.float64) + float(np.finfo(np.float32).tiny)


def _assert_elementwise(err, bound, want, what):
    bad = ~(err <= bound)                                      # (a NaN is out of bound, not inside it)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0)), err.shape)
        raise AssertionError("%s: element %s: |err| %.3e > bound %.3e (want %.6e); %d of %d elements out of bound"
                             % (what or "parity", i, err[i], bound[i], np.asarray(want, np.float64)[i], int(bad.sum()), bad.size))


def close_terms(got, want, abs_terms, n_terms, slack=4.0, eps=None, what=""):
    """`got` against ANOTHER finite-precision evaluation `want` of the same sums (the oracle's serial fp32 loop, a torch op, the
    engine's own other path): each lies within the re-association bound of the exact result, so they differ by at most twice it --
    per element, scaled by that element's own terms (no max|want| anywhere)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = 2.0 * np.broadcast_to(reassociation_bound(abs_terms, n_terms, slack, eps), got.shape)
    _assert_elementwise(np.abs(got - want), bound, want, what)


def close_rel(got, want, rtol, what=""):
    """Purely relative, per element (element-wise maps: one or two roundings each -- send_uv, degree_norm, a cast)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    _assert_elementwise(np.abs(got - want), rtol * np.abs(want) + float(np.finfo(np.float32).tiny), want, what)


def close_rows(got, want, rtol=RTOL, atol_row=None, what="", cancel=None):
    """For COMPOSITE results (a layer's output, a gradient through an attention chain) whose per-element term magnitudes are not at
    hand: |got - want| <= rtol * |want| + atol_row * (largest |want| of the SAME ROW).  The absolute part is tied to the row the element
    lives in -- one node's (or edge's) own feature vector -- never to the largest value of the whole tensor: a row 100x smaller than the
    largest row is held to an error 100x smaller.  (Aggregations, segment ops, send_uv / softmax are held per ELEMENT: check_aggregate,
    close_terms, close_rel.)
    cancel: for results that are sums of CANCELLING terms -- the gradient of a softmax score sums to zero over a destination's edges, a
    key bias has an analytically zero gradient, a bias gradient is a column sum over a million rows -- the error scales with the
    magnitude of the terms, not of the (possibly zero) result: the caller passes that magnitude (a float or an array broadcastable to
    the result) and atol_row * cancel is added to the bound.  Every call site says what it passes."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    atol_row = rtol if atol_row is None else atol_row
    w2 = np.abs(want).reshape(want.shape[0], -1) if want.ndim >= 2 else np.abs(want).reshape(-1, 1)
    row = w2.max(1).reshape((want.shape[0],) + (1,) * (want.ndim - 1)) if want.ndim >= 1 and want.size else 0.0
    extra = 0.0 if cancel is None else atol_row * np.broadcast_to(np.asarray(cancel, np.float64), want.shape)
    _assert_elementwise(np.abs(got - want), rtol * np.abs(want) + atol_row * row + extra + float(np.finfo(np.float32).tiny), want, what)


def fp64_terms(x, src, dst, op="sum", out_size=None, y=None, mop="add"):
    """The fp64 evaluation of send_u_recv / send_ue_recv (the oracle's numpy restatement run in float64: oracle/ref_ops.py
    np_send_u_recv / np_send_ue_recv) together with what bounds a finite-precision evaluation of it, per output
    element: abs_terms = the sum (mean: the mean) of |message| over the element's in-edges, n_terms = how many there are
    (+ 1 per extra rounding: the message op, the division of a mean).  -> (want64, abs_terms64, n_terms)"""
    x64 = np.asarray(x, np.float64)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    m = int(out_size) if (out_size is not None and int(out_size) > 0) else x64.shape[0]
    red = op if op in ("sum", "mean") else "sum"
    if y is None:
        want = R.np_send_u_recv(x64, src, dst, op, out_size)
        absx = R.np_send_u_recv(np.abs(x64), src, dst, red, out_size)
    else:
        y64 = np.asarray(y, np.float64)
        want = R.np_send_ue_recv(x64, y64, src, dst, mop, op, out_size)
        absx = R.np_send_ue_recv(np.abs(x64), np.abs(y64), src, dst, mop if mop in ("mul", "div") else "add", red, out_size)
    deg = np.bincount(dst, minlength=m)[:m].astype(np.float64).reshape((m,) + (1,) * (want.ndim - 1))
    n_terms = deg + (1.0 if op == "mean" else 0.0) + (1.0 if y is not None else 0.0)
    return want, absx, np.broadcast_to(n_terms, want.shape)


_OUT_ROUND = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}


def check_aggregate(got, x, src, dst, op="sum", out_size=None, y=None, mop="add", want=None, slack=4.0, storage=None, what=""):
    """One aggregation result against (1) the fp64 evaluation, per element inside the re-association bound of ITS OWN terms, and
    (2) the oracle's result `want` (the C port of the Paddle CPU kernel: serial COO loop in the storage type), per element inside
    twice that bound.  max / min involve no rounding: exact.  Integer features: exact.  storage "fp16" / "bf16": the features are
    stored in 16 bits, summed in fp32 and the result rounded to 16 bits once (+ half an ulp of the output); float64 features are
    held to the fp64 epsilon."""
    got_a = np.asarray(got)
    if np.issubdtype(np.asarray(x).dtype, np.integer) and op != "mean":
        exact = R.np_send_u_recv(np.asarray(x), src, dst, op, out_size) if y is None else R.np_send_ue_recv(np.asarray(x), np.asarray(y), src, dst, mop, op, out_size)
        assert np.array_equal(got_a, exact), what or "integer aggregation must be exact"
        return
    want64, absx, n_terms = fp64_terms(x, src, dst, op, out_size, y, mop)
    eps = EPS[np.dtype(np.float64)] if np.asarray(x).dtype == np.float64 else EPS[np.dtype(np.float32)]
    if op in ("max", "min") and y is None:
        assert np.array_equal(got_a.astype(np.float64), want64), what or ("%s of stored values involves no rounding: exact" % op)
        if want is not None:
            assert np.array_equal(got_a, np.asarray(want))
        return
    if op in ("max", "min"):                                   # (the message op rounds once)
        bound = 2.0 * eps * np.abs(want64) + float(np.finfo(np.float32).tiny)
    else:
        bound = reassociation_bound(absx, n_terms, slack, eps)
    if storage in _OUT_ROUND:
        bound = bound + _OUT_ROUND[storage] * np.abs(want64) * 1.01
    _assert_elementwise(np.abs(got_a.astype(np.float64) - want64), bound, want64, (what + " vs fp64").strip())
    if want is not None:
        _assert_elementwise(np.abs(got_a.astype(np.float64) - np.asarray(want, np.float64)), 2.0 * bound, want, (what + " vs the oracle").strip())


def rand_graph(n, e, seed, hub=None):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, e).astype(np.int64)
    dst = rng.integers(0, n, e).astype(np.int64)
    if hub is not None:          # one destination receives `hub` of the edges: row spans many chunks
        dst[rng.choice(e, hub, replace=False)] = n // 2
    return np.stack([src, dst], 1), rng


UE_SHAPES = [((d,), (d,)) for d in (1, 2, 8, 15, 16, 17, 32, 33, 64, 65, 128, 130, 300)] + \
            [((d,), (1,)) for d in (8, 16, 17, 32, 64, 128, 129)] + \
            [((h, dd), (h, 1)) for h, dd in ((1, 16), (2, 8), (3, 5), (4, 32), (8, 16), (8, 32), (8, 3), (16, 8), (12, 4), (5, 64))]


# ------------------------------------------------------------------------------------------------
# BASELINE config sizes (RMAT scale 20, |E| = 20 M, d = 128): full compare + size-independent properties
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat20(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    edges = rmat_edges(20, 20_000_000, seed=42, device="cuda")
    g = pgl.Graph(edges=edges, num_nodes=1 << 20)
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    x = torch.randn(1 << 20, 128, generator=gen, device="cuda")
    return g, x


# ------------------------------------------------------------------------------------------------
# rows of 64..128 bytes: the grouped kernel (several edges per wave instruction, one chunk per lane group)
# ------------------------------------------------------------------------------------------------
GROUP_SHAPES = [(np.float32, 17), (np.float32, 18), (np.float32, 20), (np.float32, 24), (np.float32, 31), (np.float32, 32),
                (np.float64, 9), (np.float64, 10), (np.float64, 16), (np.int32, 24), (np.int32, 29), (np.int64, 12), (np.int64, 15),
                (np.float64, 20), (np.float64, 32), (np.int64, 17), (np.int64, 32)]          # 8-byte types: up to 256-byte rows


BOUNDARY_WIDTHS = {np.float32: [7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 80, 81, 127, 129, 255, 257],
                   np.float64: [3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 65],
                   np.int32: [8, 9, 16, 17, 32, 33, 64, 65], np.int64: [4, 5, 8, 9, 16, 17, 32, 33]}


def assert_within_fp32_reassociation(got, want64, abs_terms64, n_terms, slack=4.0):
    """Per-element bound against the fp64 result ("within fp32 reassociation bound of the fp64 result"):
    any order of summing n fp32 terms t_i is within  n_terms * eps32 * sum|t_i|  of the exact sum (first-order bound,
    Higham 4.4); `slack` covers the rounding of the terms themselves.  Unlike an atol tied to max|want| this bound
    scales with each output element's own term magnitudes, so small outputs are held to a small absolute error."""
    bound = np.broadcast_to(reassociation_bound(abs_terms64, n_terms, slack), np.shape(want64))
    _assert_elementwise(np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64)), bound, want64, "vs fp64")


def check_grad_elements(got, want64, abs_terms64, n_terms, K=1.0, what=""):
    """One gradient (or forward) tensor against its fp64 value, per element inside K x the fp32 re-association bound of THAT element's
    own terms (torch tensors; the terms come from grad_defs.grad_and_terms or one of its *_terms functions).  No element is left out,
    nothing is tied to the tensor's largest value."""
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    f = lambda t: t.detach().double().cpu().numpy()
    assert np.isfinite(f(got)).all(), (what + ": not finite").strip()
    bound = K * np.broadcast_to(reassociation_bound(f(abs_terms64), f(n_terms), 4.0), tuple(want64.shape))
    _assert_elementwise(np.abs(f(got) - f(want64)), bound, f(want64), what)


# ------------------------------------------------------------------------------------------------
# VERDICT r1 "weak" 2/3: the FUSED GAT kernels at BASELINE configs[2] size (RMAT scale 20, |E| = 20 M, H = 8, D = 16)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    n, H, D = 1 << 20, 8, 16
    edges = rmat_edges(20, 20_000_000, seed=42, device="cuda")
    g = pgl.Graph(edges=edges, num_nodes=n)
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    f = torch.randn(n, H * D, generator=gen, device="cuda").reshape(n, H, D)
    gen.manual_seed(11)
    a_s = torch.randn(n, H, generator=gen, device="cuda")
    a_d = torch.randn(n, H, generator=gen, device="cuda")
    return g, f, a_s, a_d


# ------------------------------------------------------------------------------------------------
# tighter parity bars: per-element fp64 bounds at BASELINE configs[1] size
# ------------------------------------------------------------------------------------------------
def _c2_graph():
    from pgl_amd.utils.rmat import rmat_edges
    N, E = 1 << 20, 20_000_000
    edges = rmat_edges(20, E, seed=42, device=torch.device("cuda"))
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    x = torch.randn(N, 128, generator=gen, device="cuda", dtype=torch.float32)
    return N, E, edges, x


def _fp64_terms(edges, x64, N):
    """sum_e x[src] and sum_e |x[src]| per destination in fp64 (index_add_ on the GPU: the independent formulation)."""
    s = torch.zeros((N, x64.shape[1]), dtype=torch.float64, device=x64.device).index_add_(0, edges[:, 1], x64[edges[:, 0]])
    a = torch.zeros((N, x64.shape[1]), dtype=torch.float64, device=x64.device).index_add_(0, edges[:, 1], x64[edges[:, 0]].abs())
    return s, a


def _assert_bound(got, want64, abs64, n_terms, eps, slack=4.0):
    bound = slack * n_terms.clamp(min=1).double().unsqueeze(1) * eps * abs64 + torch.finfo(torch.float32).tiny
    err = (got.double() - want64).abs()
    bad = err > bound
    assert not bool(bad.any()), "worst element: err %.3e vs bound %.3e" % (float((err - bound).max()), float(bound.flatten()[(err - bound).argmax()]))


# ------------------------------------------------------------------------------------------------
# C2' = the size north_star's roofline target is quoted at.  Reference: pgl/graph.py:859-861 (send_recv -> send_u_recv),
# pgl/graph_kernel.pyx:59-88 (build_index)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2prime(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    N, E, d = 1 << 22, 100_000_000, 128
    edges = rmat_edges(22, E, seed=42, device="cuda")
    g = pgl.Graph(edges=edges, num_nodes=N)
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    x = torch.randn(N, d, generator=gen, device="cuda")
    return g, x


def _fp64_sum_and_absterms(edges, x, slab=4_000_000):
    n, d = x.shape
    want = torch.zeros(n, d, dtype=torch.float64, device=x.device)
    absterms = torch.zeros(n, d, dtype=torch.float64, device=x.device)
    for lo in range(0, edges.shape[0], slab):                            # fp64 gathers in slabs (4 GB each)
        s, t = edges[lo:lo + slab, 0], edges[lo:lo + slab, 1]
        xs = x[s].double()
        want.index_add_(0, t, xs); absterms.index_add_(0, t, xs.abs())
    return want, absterms


# ------------------------------------------------------------------------------------------------
# GCN's source-side norm as one value per edge POSITION of the sorted stream (ops.edge_scale; flat kernel SS = 2, fused
# layer kernel ES).  Reference: pgl/nn/conv.py:242-250 (h * norm -> send_recv(sum) -> * norm)
# ------------------------------------------------------------------------------------------------
def _hub_graph(pgl, n, e, seed, hub):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, e); dst = rng.integers(0, n, e)
    dst[rng.choice(e, hub, replace=False)] = n // 3                # a row spanning many chunks (split-row fix-up)
    src[rng.choice(e, hub // 2, replace=False)] = 5                # and a hub source (the transposed walk's long row)
    edges = np.stack([src, dst], 1).astype(np.int64)
    return pgl.Graph(edges=edges, num_nodes=n).tensor(), edges, rng


# ------------------------------------------------------------------------------------------------
# (b), (c) BASELINE config 4 at its stated size: N = 2 449 029, E = 123 718 280 directed, d = 100, mean.
# Reference: pgl/graph.py:834-861 (send_recv), pgl/nn/conv.py:81-115 (GraphSageConv), pgl/partition.py:37-91.
# Real OGB files are not available offline: the topology is an RMAT stand-in folded onto N nodes.
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config4(pgl):
    from pgl_amd.utils.rmat import rmat_edges
    N, E, d = 2_449_029, 123_718_280, 100
    edges = rmat_edges(22, E, seed=42, device="cuda") % N
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    x = torch.randn(N, d, generator=gen, device="cuda")
    e = host(edges)
    src, dst = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    want = R.c_send_u_recv(host(x), src, dst, "mean")                 # the serial C port of the Paddle CPU kernel, raw COO order
    # the exact result and the per-element magnitude of its terms, in fp64 on the GPU
    w64 = torch.zeros(N, d, dtype=torch.float64, device="cuda"); a64 = torch.zeros_like(w64)
    for lo in range(0, E, 4_000_000):
        s, t = edges[lo:lo + 4_000_000, 0], edges[lo:lo + 4_000_000, 1]
        xs = x[s].double()
        w64.index_add_(0, t, xs); a64.index_add_(0, t, xs.abs())
    indeg = torch.bincount(edges[:, 1], minlength=N).double()[:, None]
    w64 /= indeg.clamp(min=1); a64 /= indeg.clamp(min=1)
    return dict(N=N, E=E, d=d, edges=edges, x=x, want=want, w64=host(w64), a64=host(a64), indeg=host(indeg), e_host=e)


def _check_full_output(got, c, what):
    want, w = c["want"], c["w64"]
    scale = float(np.abs(want).max())
    # (1) north_star's bar against the EXACT result
    np.testing.assert_allclose(got, w, rtol=1e-5, atol=1e-5 * scale, err_msg=what + " vs fp64")
    # (2) against the reference's serial fp32 loop: 1e-5, plus what that loop itself is away from the exact result on rows with
    #     10^5+ in-edges (tests/test_a6_baseline_sizes.py::test_c2prime_gcn_spmm_vs_oracle explains the term)
    own = np.abs(want.astype(np.float64) - w)
    tol = 1e-5 * np.abs(want) + 1e-5 * scale + own
    err = np.abs(got.astype(np.float64) - want)
    assert not (err > tol).any(), "%s: %d elements beyond 1e-5 + the oracle's own error (worst %.3e)" % (what, int((err > tol).sum()), float((err - tol).max()))
    print("%s: all %d x %d outputs compared; oracle elements farther than 1e-5 from fp64: %d, engine elements: %d"
          % (what, got.shape[0], got.shape[1], int((own > 1e-5 * np.abs(w) + 1e-5 * scale).sum()),
             int((np.abs(got - w) > 1e-5 * np.abs(w) + 1e-5 * scale).sum())))
    # (3) per element: inside the fp32 re-association bound of the fp64 result
    assert_within_fp32_reassociation(got, w, c["a64"], np.broadcast_to(c["indeg"] + 1, got.shape), slack=2.0)


# ------------------------------------------------------------------------------------------------
# EdgeTensor: [E, ...] results of send_uv / sddmm stay in the engine's destination-sorted order across an op
# chain; what is READ is in original edge order (pgl/nn/functional/graph_op.py:117-123)
# ------------------------------------------------------------------------------------------------
def _attn_graph(pgl, n=3000, e=50000, seed=21):
    rng = np.random.default_rng(seed)
    edges = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)], 1).astype(np.int64)
    edges[rng.choice(e, 6000, replace=False), 1] = 17
    return pgl.Graph(edges=edges, num_nodes=n).tensor(), edges, rng


# ------------------------------------------------------------------------------------------------
# BASELINE config 5 at ONE RANK'S REAL SHARE: ogbn-papers100M-sized synthetic (N = 111 059 956,
# |E| = 1 615 685 872, 8 parts, fp16 features), the plan built from the edge list handed over slab by slab -- no global COO
# anywhere -- then one aggregation of the rank's ~200 M in-edges against fp64 on sampled rows.  pgl/partition.py:94-123 (the
# range / random fallback where a partitioner's input does not fit), pgl/graph.py:1509-1553 (what it replaces).
# ------------------------------------------------------------------------------------------------
def _node_features(ids, d, dtype):
    """Deterministic pseudo-random features of GLOBAL node ids ([len(ids), d]): any rank can produce any node's row."""
    col = torch.arange(d, device=ids.device, dtype=torch.float64)
    out = torch.empty((int(ids.shape[0]), d), dtype=dtype, device=ids.device)
    for lo in range(0, int(ids.shape[0]), 1 << 21):                    # (in slabs: the fp64 phase of 60 M rows would be 61 GB)
        ph = (ids[lo:lo + (1 << 21)].double().unsqueeze(1) * 0.6180339887498949 + col.unsqueeze(0) * 0.7548776662466927) % 1.0
        out[lo:lo + (1 << 21)] = (torch.sin(ph * 6.283185307179586 * 3.0) * 0.5).to(dtype)
    return out


# ------------------------------------------------------------------------------------------------
# (k) CSR build, one-sweep passes (pgl/graph_kernel.pyx:59-88 is the semantics): one histogram of
#     all digits + one kernel per pass with decoupled look-back.  The default for builds of up to 1 M edges (where it is faster:
#     profiles/r05/csr_onesweep.txt), forced on / off with pglamd_set_option("csr_onesweep", group / 0); the output must be
#     BIT-identical to the multi-kernel passes (both are stable sorts) and to the oracle.
# ------------------------------------------------------------------------------------------------
def _csr_fields(c):
    return [("degree", c.degree), ("indptr", c.indptr), ("row32", c.row32), ("col32", c.col32), ("eid32", c.eid32),
            ("sorted_u", c.sorted_u), ("sorted_v", c.sorted_v), ("sorted_eid", c.sorted_eid)]


def _csr_keys(kind, E, N, gen):
    if kind == "uniform":
        return torch.randint(0, N, (E,), generator=gen, device="cuda")
    if kind == "one-row":
        return torch.full((E,), N - 1, dtype=torch.int64, device="cuda")
    if kind == "sorted":
        return torch.sort(torch.randint(0, N, (E,), generator=gen, device="cuda")).values
    # skewed: a few hubs take most of the edges (digit bins of very different sizes, long look-back chains on the hot digits)
    k = (torch.rand(E, generator=gen, device="cuda") ** 6 * N).long().clamp_(max=N - 1)
    return k


__all__ = [n for n in dir() if not n.startswith("__")]
