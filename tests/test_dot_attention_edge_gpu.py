"""The fused dot-product attention with edge features (pgl_amd/csrc/dot_attention.hip with EDGE) and
TransformerConv(fused=True, fused_edge_feat=True) on the MI355X, held to the DEFINITION of tests/dot_attention_edge_defs.py: forward
and the four gradients (q, k, v and the per-edge feature) per element against fp64 inside the re-association bound of that element's own
terms (gpu_common.check_grad_elements; every element, none left out), K from the fp32 definition on the host
(dot_attention_edge_defs.K_FAMILY; tests/test_dot_attention_edge_defs.py re-measures it).

Graphs: the 3 000-node hub and classes graphs of tests/test_gradients_gpu.py (64-edge chunks; rows with 0 / 1 / 16 / 17 / 47 further
pieces on BOTH streams, multi-edges, self-loops, nodes without in-edges or out-edges, an edge list in random order) and the degenerate
E0, E1, N1.  ef is random per edge, so a wrong edge-id mapping on either stream fails the bound."""
import numpy as np
import pytest
import torch

import dot_attention_edge_defs as E
import grad_defs as D
from gpu_common import pgl, check_grad_elements, close_rows, host, RTOL  # noqa: F401  (pgl: the fixture)
from layout_defs import misaligned, assert_same_bits
from test_dot_attention_gpu import LAYER_CONFIGS, _rows_ratio, _sliced, _transposed
from test_gradients_gpu import _graphs, _t

pytestmark = pytest.mark.gpu

K = E.K_FAMILY
NAMES = ("d q", "d k", "d v", "d ef")


@pytest.fixture(scope="module")
def graphs(pgl):
    return _graphs(pgl)


def _inputs(G, H, Dh, seed=0):
    q, k, v, ef, cot, scale = E.case_inputs(G.n, G.e, H, Dh, seed)
    return _t(q), _t(k), _t(v), _t(ef), _t(cot), scale


_REFS = {}


def _reference(G, name, H, Dh, p=0.0, drop_seed=0, seed=0):
    """The fp64 definition and its terms on _inputs(G, H, Dh, seed), computed once per case and left unchanged."""
    key = (name, H, Dh, p, drop_seed, seed)
    if key not in _REFS:
        q, k, v, ef, cot, scale = _inputs(G, H, Dh, seed)
        keep = None if p == 0 else _t(D.attention_keep(drop_seed, np.arange(G.e), H, p))
        _REFS[key] = E.definition_and_terms(q, k, v, ef, cot, G.src, G.dst, scale, keep)
    return _REFS[key]


def _run(engine, q, k, v, ef, cot, ef_grad=True):
    xs = [t.detach().requires_grad_(True) for t in (q, k, v)] + [ef.detach().requires_grad_(ef_grad)]
    out = engine(*xs)
    out.backward(cot)
    return out.detach(), [x.grad for x in xs]


def _check(got, r, family, what, order=None):
    """order: the permutation the engine's ef rows were given in (its d ef comes back in that order)."""
    out, grads = got
    check_grad_elements(out, r.out64, r.out_abs, r.out_n, K=K[family], what=what + " forward")
    for i, name in enumerate(NAMES):
        want, terms, n = r.want64[i], r.abs_terms64[i], r.n_terms[i]
        if i == 3 and order is not None:
            want, terms, n = want[order], terms[order], n[order]
        check_grad_elements(grads[i], want, terms, n, K=K[family], what="%s %s" % (what, name))


def _same(a, b, what, n=4):
    assert_same_bits(a[0], b[0], what + ": forward")
    for x, y, name in list(zip(a[1], b[1], NAMES))[:n]:
        assert_same_bits(x, y, "%s: %s" % (what, name))


def _graph_op(G, scale, p=0.0, seed=0):
    return lambda a, b, c, e: G.g.dot_attention(a, b, c, scale, p, seed, edge_feat=e)


# ------------------------------------------------------------------------------------------------
# 1. forward and all four gradients against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "classes"])
@pytest.mark.parametrize("H,Dh", E.SHAPES)
def test_dot_attention_edge_against_fp64(pgl, graphs, graph, H, Dh):
    from pgl_amd import attention_ops, autograd as ag
    G = graphs[graph]
    assert attention_ops.dot_attention_edge_supported(H, Dh)
    q, k, v, ef, cot, scale = _inputs(G, H, Dh)
    r = _reference(G, graph, H, Dh)
    what = "dot_attention_edge %s %dx%d" % (graph, H, Dh)
    _check(_run(_graph_op(G, scale), q, k, v, ef, cot), r, "dot_attention_edge", what + " Graph.dot_attention(edge_feat=)")
    vd, vs = G.g._csr_order_views()                            # ef in the views' order: row p belongs to position p of the dst-sorted stream
    assert vd.eid32 is None
    order = G.g._csr_dst().eid32.long()
    _check(_run(lambda a, b, c, e: ag.dot_attention_edge(a, b, c, e, vd, lambda: vs, scale), q, k, v, ef[order].contiguous(), cot), r,
           "dot_attention_edge", what + " csr-order views", order=order)
    with torch.no_grad():                                    # without a gradient: the forward that writes no statistics
        plain = G.g.dot_attention(q, k, v, scale, edge_feat=ef)
    check_grad_elements(plain, r.out64, r.out_abs, r.out_n, K=K["dot_attention_edge"], what=what + " forward without statistics")


# ------------------------------------------------------------------------------------------------
# 2. an index over edges that are already grouped (eid = position)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["hub", "classes"])
@pytest.mark.parametrize("H,Dh", E.SHAPES)
def test_over_an_index_from_sorted_edges(pgl, graphs, graph, H, Dh):
    from pgl_amd import autograd as ag
    G = graphs[graph]
    order = torch.sort(G.dst, stable=True)[1]
    src, dst = G.src[order].contiguous(), G.dst[order].contiguous()
    cd = pgl.ops.csr_from_sorted(dst, src, G.n)
    cs = pgl.ops.csr_build(src, dst, G.n)
    assert torch.equal(cd.eid32.long(), torch.arange(G.e, device=dst.device))
    q, k, v, ef, cot, scale = _inputs(G, H, Dh)              # (ef row p: the p-th edge of the SORTED list)
    r = E.definition_and_terms(q, k, v, ef, cot, src, dst, scale)
    got = _run(lambda a, b, c, e: ag.dot_attention_edge(a, b, c, e, cd, lambda: cs, scale), q, k, v, ef, cot)
    _check(got, r, "dot_attention_edge", "dot_attention_edge %s %dx%d csr_from_sorted" % (graph, H, Dh))


# ------------------------------------------------------------------------------------------------
# 3. degenerate graphs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E0", "E1", "N1"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_degenerate_graphs(graphs, name, p):
    G = graphs[name]
    H, Dh = 8, 16
    q, k, v, ef, cot, scale = _inputs(G, H, Dh, seed=3)
    r = _reference(G, name, H, Dh, p, 7, seed=3)
    got = _run(_graph_op(G, scale, p, 7), q, k, v, ef, cot)
    assert tuple(got[0].shape) == (G.n, H, Dh) and all(tuple(g.shape) == (G.n, H, Dh) for g in got[1][:3])
    assert tuple(got[1][3].shape) == (G.e, H, Dh)
    _check(got, r, "dot_attention_edge_drop" if p else "dot_attention_edge", "dot_attention_edge %s p=%g" % (name, p))
    if name == "E0":
        assert all(bool((t == 0).all()) for t in [got[0]] + got[1])


# ------------------------------------------------------------------------------------------------
# 4. dropout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,H,Dh,p", E.DROP_CASES)
def test_dot_attention_edge_with_dropout(graphs, graph, H, Dh, p):
    G = graphs[graph]
    seed = E.DROP_SEEDS[p]
    q, k, v, ef, cot, scale = _inputs(G, H, Dh)
    r = _reference(G, graph, H, Dh, p, seed)
    eng = lambda s: _run(_graph_op(G, scale, p, s), q, k, v, ef, cot)
    got = eng(seed)
    _check(got, r, "dot_attention_edge_drop", "dot_attention_edge %s %dx%d p=%g" % (graph, H, Dh, p))
    _same(eng(seed), got, "the same seed twice")
    assert not torch.equal(eng(seed + 1)[0], got[0]), "another seed gives the same output"


# 5.
def test_no_dropout_is_the_plain_launch_whatever_the_seed(graphs):
    G = graphs["classes"]
    q, k, v, ef, cot, scale = _inputs(G, 8, 16)
    plain = _run(_graph_op(G, scale), q, k, v, ef, cot)
    for seed in (1, 2 ** 32 - 5):
        _same(_run(_graph_op(G, scale, 0.0, seed), q, k, v, ef, cot), plain, "p = 0, seed %d" % seed)


def test_dropout_needs_edge_ids(graphs):
    """The csr-order view of the dst-keyed index carries no edge ids: dropout over it is refused (PGLAMD_E_ARG), not run with positions."""
    from pgl_amd import attention_ops
    G = graphs["hub"]
    q, k, v, ef, _, scale = _inputs(G, 8, 16)
    vd, _ = G.g._csr_order_views()
    with pytest.raises(ValueError, match=r"dot_attention_edge: dropout needs .* eid.*code -6"):
        attention_ops.dot_attention_edge(q, k, v, ef, vd, scale, 0.3, 1)


# ------------------------------------------------------------------------------------------------
# 6. bit reproducibility
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(4, 8), (8, 16), (8, 32)])
def test_two_runs_give_identical_bits(graphs, H, Dh):
    G = graphs["classes"]
    q, k, v, ef, cot, scale = _inputs(G, H, Dh)
    for p in (0.0, 0.3):
        eng = lambda: _run(_graph_op(G, scale, p, 11), q, k, v, ef, cot)
        _same(eng(), eng(), "two runs, p = %g" % p)


# ------------------------------------------------------------------------------------------------
# 7. an edge feature that asks for no gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(4, 8), (8, 32)])
def test_without_a_gradient_for_the_edge_feature(graphs, H, Dh):
    from pgl_amd import attention_ops
    G = graphs["classes"]
    q, k, v, ef, cot, scale = _inputs(G, H, Dh)
    full = _run(_graph_op(G, scale, 0.3, 5), q, k, v, ef, cot)
    part = _run(_graph_op(G, scale, 0.3, 5), q, k, v, ef, cot, ef_grad=False)
    assert part[1][3] is None and full[1][3] is not None
    _same(part, full, "ef.requires_grad = False", n=3)
    out, mx, sm = attention_ops.dot_attention_edge(q, k, v, ef, G.g._csr_dst(), scale, 0.3, 5, return_stats=True)
    res = attention_ops.dot_attention_edge_backward(cot, q, k, v, ef, out, mx, sm, G.g._csr_dst(), G.g._csr_src(), scale, 0.3, 5, want_ef=False)
    assert len(res) == 4 and res[3] is None
    _same((out, list(res)), full, "the op with want_ef=False", n=3)


# ------------------------------------------------------------------------------------------------
# 8. operand layout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Dh", [(4, 8), (8, 16), (8, 32)])
@pytest.mark.parametrize("layout", ["transposed", "sliced", "offset-by-one-element"])
def test_operand_layout(graphs, layout, H, Dh):
    """Strided views and contiguous views one element into their storage are copied by the front end (operand layout
    contract): the results equal those on fresh copies bit for bit -- ef alone, and every operand at once."""
    G = graphs["classes"]
    q, k, v, ef, cot, scale = _inputs(G, H, Dh)
    make = {"transposed": _transposed, "sliced": _sliced, "offset-by-one-element": misaligned}[layout]
    want = _run(_graph_op(G, scale, 0.3, 5), *(t.clone() for t in (q, k, v, ef, cot)))
    _same(_run(_graph_op(G, scale, 0.3, 5), q, k, v, make(ef), cot), want, "%s ef alone %dx%d" % (layout, H, Dh))
    _same(_run(_graph_op(G, scale, 0.3, 5), make(q), make(k), make(v), make(ef), make(cot)), want, "%s operands %dx%d" % (layout, H, Dh))


# ------------------------------------------------------------------------------------------------
# 9. NaN containment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,H,Dh", [("hub", 8, 16), ("classes", 4, 8), ("classes", 8, 32)])
def test_a_nan_in_one_edge_row_stays_with_its_destination(graphs, graph, H, Dh):
    G = graphs[graph]
    q, k, v, ef, cot, scale = _inputs(G, H, Dh)
    target = 70 if graph == "hub" else 4                        # a destination whose row is split over many chunks
    into = G.dst == target
    assert int(into.sum()) > 1000
    e = int(torch.nonzero(into)[5])
    clean = _run(_graph_op(G, scale), q, k, v, ef, cot)
    ef2 = ef.clone()
    ef2[e, :, 0] = float("nan")                               # every head of that edge
    bad = _run(_graph_op(G, scale), q, k, v, ef2, cot)
    torch.cuda.synchronize()
    assert bool(torch.isnan(bad[0][target]).all()), "the NaN did not reach its destination's row"
    other = torch.ones(G.n, dtype=torch.bool, device=q.device)
    other[target] = False
    sends_none = torch.ones(G.n, dtype=torch.bool, device=q.device)
    sends_none[G.src[into]] = False
    assert int(sends_none.sum()) > 100 and int((~into).sum()) > 1000
    same = lambda a, b, what: assert_same_bits(a, b, "NaN in ef[%d] (-> %d), %s" % (e, target, what))
    same(bad[0][other], clean[0][other], "output rows other than the destination")
    same(bad[1][0][other], clean[1][0][other], "d q rows other than the destination")
    same(bad[1][1][sends_none], clean[1][1][sends_none], "d k rows of nodes that send nothing into it")
    same(bad[1][2][sends_none], clean[1][2][sends_none], "d v rows of nodes that send nothing into it")
    same(bad[1][3][~into], clean[1][3][~into], "d ef rows of edges not into it")


# ------------------------------------------------------------------------------------------------
# 10. unsupported shapes, 11. a wrong edge operand
# ------------------------------------------------------------------------------------------------
def _edge_layers(pgl, in_size=24, Dh=8, H=4, attn_drop=0.0, **kw):
    """(the default layer = today's path, fused=True alone, fused=True with fused_edge_feat=True) from one state_dict."""
    torch.manual_seed(7)
    mk = lambda **f: pgl.nn.TransformerConv(in_size, Dh, num_heads=H, feat_drop=0.0, attn_drop=attn_drop, **dict(kw, **f)).cuda()
    plain, alone, both = mk(), mk(fused=True), mk(fused=True, fused_edge_feat=True)
    alone.load_state_dict(plain.state_dict())
    both.load_state_dict(plain.state_dict())
    return plain, alone, both


@pytest.mark.parametrize("H,Dh", [(3, 12), (16, 32)])
def test_unsupported_shapes(pgl, graphs, H, Dh):
    from pgl_amd import attention_ops
    G = graphs["hub"]
    assert not attention_ops.dot_attention_edge_supported(H, Dh)
    q, k, v, ef, _, scale = _inputs(G, H, Dh)
    with pytest.raises(ValueError, match=r"dot_attention_edge.*code -1"):
        attention_ops.dot_attention_edge(q, k, v, ef, G.g._csr_dst(), scale)
    plain, _, both = _edge_layers(pgl, Dh=Dh, H=H)
    rng = np.random.default_rng(4)
    x, e = _t(rng.standard_normal((G.n, 24))), _t(rng.standard_normal((G.e, H * Dh)))
    assert not both._takes_fused(G.g, x, e)
    with torch.no_grad():
        assert_same_bits(both(G.g, x, e), plain(G.g, x, e), "TransformerConv %dx%d: both flags on a shape the kernels do not take" % (H, Dh))


def test_a_wrong_edge_operand_is_turned_away(pgl, graphs):
    from pgl_amd import attention_ops
    G = graphs["hub"]
    q, k, v, ef, cot, scale = _inputs(G, 8, 16)
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    for rows in (G.e - 1, G.e + 1, 0):
        wrong = torch.zeros((rows, 8, 16), device=q.device)
        with pytest.raises(ValueError, match=r"ef holds %d rows" % rows):
            attention_ops.dot_attention_edge(q, k, v, wrong, cd, scale)
        with pytest.raises(ValueError, match=r"ef holds %d rows" % rows):
            G.g.dot_attention(q, k, v, scale, edge_feat=wrong)
    out, mx, sm = attention_ops.dot_attention_edge(q, k, v, ef, cd, scale, return_stats=True)
    with pytest.raises(ValueError, match=r"ef holds %d rows" % (G.e - 1)):
        attention_ops.dot_attention_edge_backward(cot, q, k, v, ef[:-1], out, mx, sm, cd, cs, scale)
    with pytest.raises(ValueError, match=r"y_rows"):            # an index over a subset of a graph's edges
        attention_ops.dot_attention_edge(q, k, v, ef, cd.view(y_rows=G.e + 5), scale)
    with pytest.raises(ValueError, match=r"y_rows"):
        attention_ops.dot_attention_edge_backward(cot, q, k, v, ef, out, mx, sm, cd, cs.view(y_rows=G.e + 5), scale)
    with pytest.raises(TypeError):
        attention_ops.dot_attention_edge(q, k, v, ef.double(), cd, scale)
    with pytest.raises(TypeError):
        attention_ops.dot_attention_edge(q, k, v, ef.reshape(G.e, 128), cd, scale)


# ------------------------------------------------------------------------------------------------
# 12. the layer
# ------------------------------------------------------------------------------------------------
def _layer_data(G, kw):
    """x and the cotangent w: the values test_transformer_conv_fused_against_the_three_op_layer compares its two layers on (one
    generator, seed 43, x first); the edge feature: standard normal from the generator of
    test_transformer_conv_with_edge_features_takes_todays_path (seed 47), one of its own so that x and w stay those values.
    The bias gradients are sums over every node that cancel, and two fp32 layers can be compared at RTOL of such a sum only where the
    reference is itself that close to fp64; on these values it is (today's path against the fp64 layer: at most 0.886 of the bound)."""
    rng = np.random.default_rng(43)
    x = rng.standard_normal((G.n, 24)).astype(np.float32)
    w = rng.standard_normal((G.n, 8 if kw.get("concat") is False else 32)).astype(np.float32)
    return x, np.random.default_rng(47).standard_normal((G.e, 32)).astype(np.float32), w


@pytest.mark.parametrize("config", list(LAYER_CONFIGS))
def test_transformer_conv_fused_edge_feat_against_todays_layer(pgl, graphs, config):
    """Output, d x, d edge_feat and every parameter gradient of fused=True, fused_edge_feat=True against the default layer (the
    user-function path) from one state_dict: close_rows at RTOL, nothing added.  k.bias as in
    test_transformer_conv_fused_against_the_three_op_layer: its gradient is analytically zero (a constant added to every key shifts all
    scores of a row alike), so it is held to RTOL of its own terms, sum_u |d k[u, c]|, read from the default layer.

    Measured on an MI355X, worst |difference| / bound per config: output <= 0.047, d x <= 0.097, d edge_feat <= 0.357, weight
    gradients <= 0.230; the bias gradients, column sums over all 3 000 nodes, come closest: d v.bias 0.873 (gate) and 0.936 (bare),
    d q.bias 0.805 (bare).  Both layers are deterministic: six separate processes printed the same digits.  On these inputs today's
    path itself lies within 0.886 of the bound from the same layer evaluated in fp64 (d skip_feat.bias, head-mean), so the
    comparison has a reference to compare against; on a draw where a bias column cancels to a hundredth of its neighbours neither
    fp32 layer is that close to fp64, and the comparison says nothing there (_layer_data)."""
    G = graphs["hub"]
    kw = LAYER_CONFIGS[config]
    plain, alone, both = _edge_layers(pgl, **kw)
    x, ef, w = _layer_data(G, kw)
    keys = []

    def keep_key_gradient(mod, args, out):                      # (returns None: the output stays as it is)
        out.retain_grad()
        keys.append(out)

    hook = plain.k.register_forward_hook(keep_key_gradient)
    res = []
    for layer in (plain, both):
        xd, ed = _t(x).requires_grad_(True), _t(ef).requires_grad_(True)
        assert layer._takes_fused(G.g, xd, ed) == (layer is both)
        out = layer(G.g, xd, ed)
        out.backward(_t(w))
        res.append((out, xd.grad, ed.grad, [p.grad for p in layer.parameters()]))
    hook.remove()
    assert not alone._takes_fused(G.g, _t(x), _t(ef)) and alone._takes_fused(G.g, _t(x), None)      # only with both flags
    assert not pgl.nn.TransformerConv(24, 8, num_heads=4, fused_edge_feat=True).cuda()._takes_fused(G.g, _t(x), _t(ef))
    (o0, gx0, ge0, gp0), (o1, gx1, ge1, gp1) = res
    assert len(keys) == 1 and keys[0].grad is not None
    own_terms = {"k.bias": host(keys[0].grad.double().abs().sum(0)).reshape(-1, 1)}
    flat = lambda t: host(t).reshape(t.shape[0], -1)
    checks = [("output", host(o1), host(o0), None), ("d x", host(gx1), host(gx0), None), ("d edge_feat", host(ge1), host(ge0), None)] + \
             [("d " + name, flat(a), flat(b), own_terms.get(name)) for a, b, (name, _) in zip(gp1, gp0, both.named_parameters())]
    print("fused edge features vs today's path (%s), worst |difference| / bound: %s"
          % (config, ", ".join("%s %.3f" % (n, _rows_ratio(a, b, c)) for n, a, b, c in checks)))
    missed = []
    for name, a, b, cancel in checks:                           # every quantity is held to the bound; all that miss it are reported
        try:
            close_rows(a, b, RTOL, what="fused edge features vs today's path (%s): %s" % (config, name), cancel=cancel)
        except AssertionError as err:
            missed.append(str(err))
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("config", list(LAYER_CONFIGS))
def test_bias_gradients_of_the_fused_layer_against_the_fp64_layer(pgl, graphs, config):
    """Beside the comparison above, not in its place: the gradient of every nn.Linear bias of the fused layer against the same layer
    evaluated in fp64 (today's path on fp64 operands), held to RTOL of its OWN terms as k.bias is above.  d bias[c] = sum_u d y[u, c] over all nodes (y the linear's output), a plain sum of n = 3 000 fp32 terms whose
    re-association bound is n eps sum_u |d y[u, c]|; RTOL = 1e-5 is 84 eps, so RTOL (|want| + sum_u |d y[u, c]|) is 36 times tighter
    than that bound.  The terms are read from the fp64 layer, never from the engine.  Measured: 0.001 .. 0.003 of this bound."""
    import copy
    G = graphs["hub"]
    kw = LAYER_CONFIGS[config]
    _, _, both = _edge_layers(pgl, **kw)
    ref = copy.deepcopy(both).double()
    ref.fused = ref.fused_edge_feat = False
    x, ef, w = _layer_data(G, kw)
    outs, hooks = {}, []

    def keep(name):
        def hook(mod, args, out):                               # (returns None: the output stays as it is)
            out.retain_grad()
            outs[name] = out
        return hook

    linears = [name for name, m in ref.named_modules() if isinstance(m, torch.nn.Linear)]
    assert {"q", "k", "v"} <= set(linears)
    for name in linears:
        hooks.append(ref.get_submodule(name).register_forward_hook(keep(name)))
    assert both._takes_fused(G.g, _t(x), _t(ef)) and not ref._takes_fused(G.g, _t(x).double(), _t(ef).double())
    both(G.g, _t(x), _t(ef)).backward(_t(w))
    ref(G.g, _t(x).double(), _t(ef).double()).backward(_t(w).double())
    for h in hooks:
        h.remove()
    checks = []
    for name in linears:
        got, want = both.get_submodule(name).bias.grad, ref.get_submodule(name).bias.grad
        own = outs[name].grad.abs().reshape(-1, want.shape[0]).sum(0)
        checks.append(("d %s.bias" % name, host(got).reshape(-1, 1), host(want).reshape(-1, 1), host(own).reshape(-1, 1)))
    print("fused edge features vs the fp64 layer (%s), worst |difference| / bound: %s"
          % (config, ", ".join("%s %.3f" % (n, _rows_ratio(a, b, c)) for n, a, b, c in checks)))
    for name, a, b, cancel in checks:
        close_rows(a, b, RTOL, what="fused edge features vs the fp64 layer (%s): %s" % (config, name), cancel=cancel)


def test_fused_alone_keeps_todays_path_with_edge_features(pgl, graphs):
    G = graphs["hub"]
    plain, alone, both = _edge_layers(pgl)
    rng = np.random.default_rng(47)
    x, ef = _t(rng.standard_normal((G.n, 24))), _t(rng.standard_normal((G.e, 32)))
    with torch.no_grad():
        want = plain(G.g, x, ef)
        assert_same_bits(alone(G.g, x, ef), want, "TransformerConv(fused=True) with edge features")
    # not fp32, not on the GPU, not one row per edge, not num_heads * hidden_size columns: today's path
    for other in (ef.double(), ef.cpu(), ef[:-1], ef[:, :-1]):
        assert not both._takes_fused(G.g, x, other)
    assert both._takes_fused(G.g, x, ef) and both._takes_fused(G.g, x, ef.reshape(G.e, 4, 8))


def test_the_layer_in_training_mode_is_the_definition_with_the_seed_it_drew(pgl, graphs):
    """attn_drop = 0.5, .train(): the layer's output against linear -> definition(keep of layer.last_attn_seed) -> skip -> layer norm ->
    relu in fp64, close_rows at 5e-5 (what test_transformer_conv_fused_in_training_mode_is_the_definition_with_the_seed_it_drew holds
    the layer without edge features to)."""
    G = graphs["hub"]
    _, _, both = _edge_layers(pgl, attn_drop=0.5)
    rng = np.random.default_rng(53)
    x, ef = _t(rng.standard_normal((G.n, 24))), _t(rng.standard_normal((G.e, 32)))
    both.train()
    torch.manual_seed(1004)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(1004)
    out = both(G.g, x, ef)
    assert both.last_attn_seed == seed

    def definition(keep):
        xd = x.double()
        lin = lambda m: xd @ m.weight.detach().double().t() + m.bias.detach().double()
        q, k, v = (lin(m).reshape(G.n, 4, 8) for m in (both.q, both.k, both.v))
        o = E.dot_attention_edge(q, k, v, ef.double().reshape(G.e, 4, 8), G.src, G.dst, 8 ** -0.5, keep=keep).reshape(G.n, 32) + lin(both.skip_feat)
        o = torch.nn.functional.layer_norm(o, (32,), both.layer_norm.weight.detach().double(), both.layer_norm.bias.detach().double(),
                                           both.layer_norm.eps)
        return host(torch.relu(o))

    want = definition(_t(D.attention_keep(seed, np.arange(G.e), 4, 0.5)))
    close_rows(host(out), want, rtol=5e-5, what="TransformerConv(fused=True, fused_edge_feat=True).train(): output")
    other = definition(_t(D.attention_keep(seed + 1, np.arange(G.e), 4, 0.5)))
    assert np.abs(other - want).max() > 1e-2 * np.abs(want).max()            # another seed is another mask: the comparison is not vacuous
    both.eval()
    state = torch.get_rng_state()
    with torch.no_grad():
        got = both(G.g, x, ef)
    assert torch.equal(torch.get_rng_state(), state), "an eval forward drew from torch's generator"
    assert both.last_attn_seed is None
    close_rows(host(got), definition(None), rtol=5e-5, what="TransformerConv(fused=True, fused_edge_feat=True).eval(): output")


# ------------------------------------------------------------------------------------------------
# 13. graph replay
# ------------------------------------------------------------------------------------------------
def test_forward_and_backward_replayed_from_a_captured_graph(graphs):
    """Forward plus backward at 8 x 16 on the classes graph captured in torch.cuda.graph on ONE side stream (no parallel branches) after a
    warm-up call there, then replayed on other operand values: the bits of the eager run on those values."""
    G = graphs["classes"]
    q, k, v, ef, cot, scale = _inputs(G, 8, 16)
    eager = _run(_graph_op(G, scale, 0.3, 5), q, k, v, ef, cot)
    first = _inputs(G, 8, 16, seed=1)                            # what the capture sees
    xs = [t.clone().requires_grad_(True) for t in first[:4]]
    g = first[4].clone()

    def step():
        out = _graph_op(G, scale, 0.3, 5)(*xs)
        return (out,) + torch.autograd.grad(out, xs, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # warm-up: indices, workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = step()
    with torch.no_grad():
        for x, new in zip(xs + [g], (q, k, v, ef, cot)):
            x.copy_(new)
        for t in res:
            t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _same((res[0], list(res[1:])), eager, "replayed from a captured graph")
