"""What tests/test_gat16_gpu.py holds the 16-bit GAT kernels (pgl_amd/csrc/gat_fused_16.hip) to, restated on the host.

`gat16_host` walks every destination's edges ONE AFTER THE OTHER in fp64 (the attention weights come from the fp64 softmax of
grad_defs) and rounds the row to the storage type once, at the end: what the kernels promise -- 16-bit storage, wide sums, one
rounding.  Its mutant rounds the running row to the storage type after every edge: what a kernel that accumulated in its storage
type would compute.  `bound16` is the element bound of the forward: the fp32 bound the gat family already has, plus one rounding to
nearest of the result.  Pure torch, no GPU needed; tests/test_gat16_defs.py holds this file to a plain torch composition."""
import numpy as np
import torch

import grad_defs as D

U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # unit round-off of ONE rounding to nearest (test_gradients_gpu.U16)
SUB16 = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}           # half the spacing of fp16's subnormals; bf16 has fp32's exponent range


def round16(t, dt):
    """t (fp64 / fp32) rounded to dt, to nearest even, back in t's type."""
    return t.to(dt).to(t.dtype)


def gat16_host(f, a_s, a_d, src, dst, dt, slope=0.2, keep=None, round_each_edge=False):
    """f [N, H, D] in dt; a_s, a_d [N, H]; src, dst int64 [E] in ORIGINAL edge order -> out [N, H, D] fp64 holding dt's values.
    The edges of a destination are taken in the stable dst-sorted order (the engine's).  round_each_edge: THE MUTANT."""
    assert f.dtype == dt
    f64, a_s, a_d = f.detach().double().cpu(), a_s.detach().double().cpu(), a_d.detach().double().cpu()
    src, dst = src.cpu(), dst.cpu()
    n = f64.shape[0]
    _, alpha = D._dense_gat_fp64(torch.stack([src, dst], 1), f64, a_s, a_d, slope)
    w = alpha if keep is None else alpha * torch.as_tensor(keep).double().cpu()
    order = torch.argsort(dst, stable=True)
    src_s, dst_s, w_s = src[order], dst[order], w[order]
    deg = torch.bincount(dst, minlength=n)
    start = torch.cumsum(deg, 0) - deg
    acc = torch.zeros_like(f64)
    for k in range(int(deg.max()) if deg.numel() and src.numel() else 0):
        live = torch.nonzero(deg > k).reshape(-1)                   # the rows that have a k-th edge
        e = start[live] + k
        acc[live] = acc[live] + w_s[e][:, :, None] * f64[src_s[e]]
        if round_each_edge:
            acc[live] = round16(acc[live], dt)
    return round16(acc, dt)


def bound16(f, a_s, a_d, src, dst, dt, slope=0.2):
    """-> (want64, bound) of the forward, element by element: grad_defs.gat in fp64 on the up-cast inputs; the fp32 bound of the gat
    family (grad_defs.bound over gat_terms' "out" with K_FAMILY["gat"]) + u16 |want| (+ 2**-25 for fp16)."""
    f64, s64, d64 = f.detach().double(), a_s.detach().double(), a_d.detach().double()
    want = D.gat(f64, s64, d64, src, dst, slope)
    terms, n_terms = D.gat_terms(f64, s64, d64, src, dst, torch.zeros_like(f64), slope)["out"]
    return want, D.bound(terms, n_terms, K=D.K_FAMILY["gat"]) + U16[dt] * want.abs() + SUB16[dt]


def all_bit_patterns(dt):
    """Every one of the 65 536 values of a 16-bit float type, as a tensor of that type."""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)


def small_graph(n=40, e=200, seed=3):
    """A 200-edge graph with a row of 60 edges, multi-edges, self-loops and rows without in-edges -> (src, dst) int64."""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(5, n, e)
    src[:4], dst[:4] = 11, 12
    src[4:8] = dst[4:8] = np.arange(20, 24)
    dst[8 + rng.choice(e - 8, 60, replace=False)] = 7
    return torch.as_tensor(src), torch.as_tensor(dst)
