"""tests/gat16_defs.py -- what tests/test_gat16_gpu.py holds the 16-bit GAT kernels to -- held to a plain torch composition on the CPU."""
import numpy as np
import pytest
import torch

import grad_defs as D
import gat16_defs as G16

DTYPES = [torch.float16, torch.bfloat16]


def _data(dt, H=2, Dh=8, seed=9):
    src, dst = G16.small_graph()
    n = 40
    rng = np.random.default_rng(seed)
    f = torch.as_tensor(rng.standard_normal((n, H, Dh)) * 10.0 ** rng.uniform(-4, 0, (n, 1, 1))).to(dt)
    a_s = torch.as_tensor(rng.integers(-512, 512, (n, H)) * 2.0 ** -8).float()
    a_d = torch.as_tensor(rng.integers(-512, 512, (n, H)) * 2.0 ** -8).float()
    return f, a_s, a_d, src, dst


@pytest.mark.parametrize("dt", DTYPES)
def test_host_restatement_is_the_composition_rounded_once(dt):
    """Edge after edge in fp64 and one rounding = gather -> softmax -> index_add in fp64, rounded: the same 16-bit value, or its
    neighbour where the two fp64 sums (different orders) straddle a rounding boundary -- half a 16-bit ulp apart at the most."""
    f, a_s, a_d, src, dst = _data(dt)
    assert src.shape[0] == 200 and int(torch.bincount(dst).max()) >= 60
    got = G16.gat16_host(f, a_s, a_d, src, dst, dt)
    want64 = D.gat(f.double(), a_s.double(), a_d.double(), src, dst, 0.2)
    want = G16.round16(want64, dt)
    assert torch.equal(got.to(dt).double(), got), "the restatement returns values outside the storage type"
    same = (got == want).double().mean()
    assert float(same) > 0.99, float(same)
    assert bool(((got - want64).abs() <= G16.U16[dt] * want64.abs() * (1 + 1e-9) + G16.SUB16[dt] + 1e-300).all())
    rows_without_edges = torch.bincount(dst, minlength=40) == 0
    assert bool(rows_without_edges.any()) and bool((got[rows_without_edges] == 0).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_host_mutant_is_the_accumulator_rounded_after_every_edge(dt):
    """The mutant against a Python loop over the dst-sorted edges that keeps the running row in the storage type: the same bits.  And
    it IS a mutant: on the 60-edge row it leaves the bound of the forward that the restatement keeps."""
    f, a_s, a_d, src, dst = _data(dt)
    got = G16.gat16_host(f, a_s, a_d, src, dst, dt, round_each_edge=True)
    f64 = f.double()
    _, alpha = D._dense_gat_fp64(torch.stack([src, dst], 1), f64, a_s.double(), a_d.double(), 0.2)
    acc = torch.zeros_like(f64).to(dt)
    for e in torch.argsort(dst, stable=True).tolist():
        u, v = int(src[e]), int(dst[e])
        acc[v] = (acc[v].double() + alpha[e][:, None] * f64[u]).to(dt)
    assert torch.equal(got.to(dt).view(torch.int16), acc.view(torch.int16))
    want, bound = G16.bound16(f, a_s, a_d, src, dst, dt)
    ok = G16.gat16_host(f, a_s, a_d, src, dst, dt)
    assert bool(((ok - want).abs() <= bound).all()), "the restatement itself leaves the bound"
    assert bool(((got - want).abs() > bound)[7].any()), "the bound takes a row rounded after every one of its 60 edges"


def test_rounding_constants_are_the_formats_own():
    for dt in DTYPES:
        assert G16.U16[dt] == torch.finfo(dt).eps / 2                       # unit round-off of rounding to nearest
    assert G16.SUB16[torch.float16] == torch.finfo(torch.float16).tiny * torch.finfo(torch.float16).eps / 2 == 2.0 ** -25
    assert torch.finfo(torch.bfloat16).tiny == torch.finfo(torch.float32).tiny   # bf16 keeps fp32's exponent range: no such term
    import test_gradients_gpu as T
    assert T.U16 == G16.U16


@pytest.mark.parametrize("dt", DTYPES)
def test_up_cast_then_round_is_the_identity(dt):
    """x.float().to(dt) gives back x's bits for every finite value of the type (subnormals included): what lets a 16-bit kernel be
    compared with the fp32 kernel on the up-cast operands."""
    x = G16.all_bit_patterns(dt)
    assert x.numel() == 65536 and len(set(x.view(torch.int16).tolist())) == 65536
    finite = torch.isfinite(x.float())
    assert int((~finite).sum()) == {torch.float16: 2 * 1024, torch.bfloat16: 2 * 128}[dt]
    back = x.float().to(dt)
    assert torch.equal(back.view(torch.int16)[finite], x.view(torch.int16)[finite])
    assert torch.equal(x.double().to(dt).view(torch.int16)[finite], x.view(torch.int16)[finite])
    assert bool(torch.isnan(back[torch.isnan(x.float())]).all())
