"""tests/readout_defs.py held to account on the host: the recorded K table against what the fp32 definition measures on the GPU tests'
own inputs, the definition against grad_defs.segment_softmax followed by a segment sum, its autograd against the issue's closed-form
gradients, the host half of the plan (pgl_amd.readout_ops.host_pieces), the front end's refusals, the layers' routing test on inputs
they do not take, and the C ABI surface.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import grad_defs as D
import readout_defs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recorded_ratios_cover_what_the_fp32_definition_measures():
    got = R.measure_definitions(verbose=True)
    assert set(got) == set(R.FP32_DEFINITION_RATIO)
    for family, ratio in got.items():
        assert ratio <= R.FP32_DEFINITION_RATIO[family], (family, ratio, R.FP32_DEFINITION_RATIO[family])
        assert R.K_FAMILY[family] == max(1.0, 4.0 * R.FP32_DEFINITION_RATIO[family])


def _small(mode, d=5, seed=0):
    lengths = [0, 3, 1, 0, 7, 2, 0]
    seg_ptr = R.seg_ptr_of(lengths)
    rng = np.random.default_rng(seed)
    x = torch.as_tensor(rng.standard_normal((int(seg_ptr[-1]), d)))
    opnd = torch.as_tensor(rng.standard_normal(int(seg_ptr[-1])) if mode == "gate" else rng.standard_normal((len(lengths), d)))
    return seg_ptr, x, opnd, torch.as_tensor(rng.standard_normal((len(lengths), d)))


@pytest.mark.parametrize("mode", ["gate", "query"])
def test_the_definition_is_segment_softmax_then_segment_sum(mode):
    seg_ptr, x, opnd, _ = _small(mode)
    S = len(seg_ptr) - 1
    ids = R.segment_ids(seg_ptr)
    s = opnd if mode == "gate" else torch.stack([x[i] @ opnd[int(ids[i])] for i in range(x.shape[0])])
    a = D.segment_softmax(s.reshape(-1, 1), ids, S)
    want = D.segment_pool(a * x, ids, "sum", S)
    got = R.attention_readout(x, seg_ptr, **({"score": opnd} if mode == "gate" else {"query": opnd}))
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-13, atol=1e-15)
    for g in (0, 3, 6):                                       # the empty segments, first and last among them
        assert bool((got[g] == 0).all())


@pytest.mark.parametrize("mode", ["gate", "query"])
def test_autograd_of_the_definition_is_the_closed_form(mode):
    """c_g = <d out[g], out[g]>, t_i = <d out[g], x[i]>, ds_i = a_i (t_i - c_g);  d x = a d out (+ ds q), d score = ds, d q = sum ds x."""
    seg_ptr, x, opnd, cot = _small(mode, seed=1)
    ids = R.segment_ids(seg_ptr)
    kw = (lambda b: dict(score=b)) if mode == "gate" else (lambda b: dict(query=b))
    out, (dx, do) = D.evaluate(lambda a, b: R.attention_readout(a, seg_ptr, **kw(b)), [x, opnd], cot)
    _, a, _ = R.attention_readout(x, seg_ptr, return_parts=True, **kw(opnd))
    ds = a * ((cot[ids] * x).sum(-1) - (cot * out).sum(-1)[ids])
    if mode == "gate":
        assert torch.allclose(dx, a[:, None] * cot[ids], rtol=1e-12, atol=1e-14) and torch.allclose(do, ds, rtol=1e-12, atol=1e-14)
    else:
        assert torch.allclose(dx, a[:, None] * cot[ids] + ds[:, None] * opnd[ids], rtol=1e-12, atol=1e-14)
        want = torch.zeros_like(opnd).index_add(0, ids, ds[:, None] * x)
        assert torch.allclose(do, want, rtol=1e-12, atol=1e-14) and bool((do[0] == 0).all()) and bool((do[6] == 0).all())


def test_terms_are_finite_where_a_score_is_minus_infinity():
    seg_ptr, x, score, cot = _small("gate", seed=2)
    score = score.clone()
    score[0] = -float("inf")                                  # the first row of segment 1 (3 rows)
    t = R.readout_terms(x, seg_ptr, cot, score=score)
    assert all(bool(torch.isfinite(v[0]).all()) for v in t.values())
    assert bool((t["x"][0][0] == 0).all()) and float(t["operand"][0][0]) == 0.0


# ------------------------------------------------------------------------------------------------
# the plan's host half
# ------------------------------------------------------------------------------------------------
def _check_pieces(lengths):
    from pgl_amd import readout_ops
    P = readout_ops.READOUT_PIECE
    seg_ptr = R.seg_ptr_of(lengths)
    pieces, longs = readout_ops.host_pieces(seg_ptr)
    assert pieces.dtype == np.int64 and pieces.ndim == 2 and pieces.shape[1] == 4 and pieces.flags["C_CONTIGUOUS"]
    assert longs.dtype == np.int64 and longs.ndim == 2 and longs.shape[1] == 3
    assert (np.diff(pieces[:, 0]) >= 0).all() and sorted(set(pieces[:, 0].tolist())) == list(range(len(lengths)))     # every segment, in order
    next_part, long_rows = 0, []
    for g, n in enumerate(lengths):
        mine = pieces[pieces[:, 0] == g]
        assert len(mine) == max(1, -(-n // P)), (g, n)
        assert (mine[:, 2] >= 0).all() and (mine[:, 2] <= P).all() and int(mine[:, 2].sum()) == n
        assert (mine[:-1, 2] == P).all()                      # only the last piece may be short
        pos = int(seg_ptr[g])
        for row0, rows in mine[:, 1:3].tolist():              # the segment's rows exactly once and in order
            assert row0 == pos
            pos += rows
        assert pos == int(seg_ptr[g + 1])
        if len(mine) == 1:
            assert int(mine[0, 3]) == -1
        else:
            assert mine[:, 3].tolist() == list(range(next_part, next_part + len(mine)))
            long_rows.append([g, next_part, len(mine)])
            next_part += len(mine)
    assert longs.tolist() == long_rows
    return pieces, longs


def test_host_pieces_tile_every_segment():
    from pgl_amd import readout_ops
    P = readout_ops.READOUT_PIECE
    lengths = [0, 1, P - 1, P, P + 1, 3 * P + 5]
    pieces, longs = _check_pieces(lengths)
    assert longs[:, 0].tolist() == [4, 5] and longs[:, 2].tolist() == [2, 4]
    _check_pieces(lengths[::-1])
    _check_pieces([0])                                        # S = 1, N = 0
    _check_pieces([0, 0, 5, 0])
    _check_pieces(R.LENGTHS)
    for bad in ([0], [0, 3, 2], [-1, 2]):
        with pytest.raises(ValueError):
            readout_ops.host_pieces(np.asarray(bad))


def test_piece_constants_agree():
    from pgl_amd import readout_ops
    hdr = open(os.path.join(ROOT, "include", "pgl_amd.h")).read()
    assert int(re.search(r"#define\s+PGLAMD_READOUT_PIECE\s+(\d+)", hdr).group(1)) == readout_ops.READOUT_PIECE == R.PIECE
    assert int(re.search(r"#define\s+PGLAMD_READOUT_GATE\s+(\d+)", hdr).group(1)) == readout_ops.GATE
    assert int(re.search(r"#define\s+PGLAMD_READOUT_QUERY\s+(\d+)", hdr).group(1)) == readout_ops.QUERY


def test_entry_points_are_declared_and_bound():
    import pgl_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgl_amd.h")).read(), flags=re.S)
    for name in ("pglamd_attention_readout_workspace_bytes", "pglamd_attention_readout", "pglamd_attention_readout_backward"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pgl_amd._ffi.exported_symbols()
        assert hasattr(pgl_amd._ffi.lib(), name)
    ws = pgl_amd._ffi.lib().pglamd_attention_readout_workspace_bytes
    assert ws(0, 64) > 0 and ws(10, 64) >= 10 * (64 + 2) * 4 and ws(1, 513) == 0 and ws(1, 0) == 0


# ------------------------------------------------------------------------------------------------
# the front end and the layers, on what they do not take
# ------------------------------------------------------------------------------------------------
def test_front_end_refusals():
    from pgl_amd import readout_ops
    assert readout_ops.readout_supported(1) and readout_ops.readout_supported(512)
    assert not readout_ops.readout_supported(0) and not readout_ops.readout_supported(513)
    x, s, q = torch.zeros(3, 4), torch.zeros(3), torch.zeros(1, 4)
    with pytest.raises(ValueError, match="exactly one of score / query"):
        readout_ops.attention_readout(x, None, score=s, query=q)
    with pytest.raises(ValueError, match="exactly one of score / query"):
        readout_ops.attention_readout(x, None)
    with pytest.raises(ValueError, match="float32"):
        readout_ops.attention_readout(x.double(), None, score=s.double())
    with pytest.raises(ValueError, match="float32"):
        readout_ops.attention_readout(x, None, query=q.double())
    with pytest.raises(ValueError, match="d = 513"):
        readout_ops.attention_readout(torch.zeros(3, 513), None, score=s)
    with pytest.raises(ValueError, match="on the GPU"):
        readout_ops.attention_readout(x, None, score=s)
    with pytest.raises(ValueError, match="on the GPU"):
        readout_ops.attention_readout(x, None, query=q)
    with pytest.raises(ValueError, match="on the GPU"):
        readout_ops.readout_plan(np.asarray([0, 3]), "cpu")


def test_layers_do_not_take_what_the_kernel_does_not():
    """fused=True on a CPU graph, a numpy-mode graph, fp64 features and a 3-D tensor: _takes_fused is False and the forward is the unfused
    layer's (which has no host path and says so)."""
    import pgl_amd as pgl
    graphs = [pgl.Graph(edges=np.asarray([[0, 1], [1, 2]]), num_nodes=3), pgl.Graph(edges=np.asarray([[0, 1]]), num_nodes=2)]
    bg = pgl.Graph.disjoint(graphs)
    x = torch.as_tensor(np.random.default_rng(0).standard_normal((5, 6)).astype(np.float32))
    torch.manual_seed(0)
    ga = pgl.nn.GlobalAttention(torch.nn.Linear(6, 1), torch.nn.Linear(6, 4))
    ga_f = pgl.nn.GlobalAttention(ga.gate, ga.nn, fused=True)
    s2s = pgl.nn.Set2Set(6, 2)
    s2s_f = pgl.nn.Set2Set(6, 2, fused=True)
    s2s_f.load_state_dict(s2s.state_dict())
    assert ga_f.fused and s2s_f.fused and not ga.fused and not s2s.fused
    for g in (bg, pgl.Graph.disjoint(graphs).tensor(device="cpu")):
        for layer in (ga_f, s2s_f):
            assert not layer._takes_fused(g, x) and not layer._takes_fused(g, x.double()) and not layer._takes_fused(g, x.reshape(5, 2, 3))
    g = pgl.Graph.disjoint(graphs).tensor(device="cpu")
    for layer in (ga_f, s2s_f):                               # the unfused code ran: its segment kernels have no host path
        with torch.no_grad(), pytest.raises(RuntimeError, match="only on an MI355X"):
            layer(g, x)
    assert not pgl.nn.Set2Set(6, 0, fused=True)._takes_fused(g, x)
    assert not ga._takes_fused(g, x) and not s2s._takes_fused(g, x)
