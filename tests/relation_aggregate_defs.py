"""The DEFINITION of relational aggregation (pgl_amd.ops.aggregate_relations, HeterGraph.send_recv_relations, RGCNConv(fused=True)),
restated without any engine code: numpy fp64 for the forward and its gradient, and the same thing in plain torch (index_add, edge by
edge) for tests/grad_defs.grad_and_terms.

    S[r, v, :] = s_r(v) * sum over e in seg(r, v) of c[r, col[e]] * x_r[col[e], :]        seg(r, v) = indptr[r, v] .. indptr[r, v + 1]
    s_r(v) = 1 ("sum") or 1 / len(seg(r, v)) ("mean"); an empty segment contributes nothing
    out[v] = sum over r of S[r, v]   ([M, d])     or, per relation, S itself as [M, R, d];   M = out_size or rows

Every function returns (want64, abs_terms64, n_terms) per output element, as gpu_common.fp64_terms does: abs_terms = the same
expression over absolute values, n_terms = the in-edges over all contributing relations + one rounding per non-empty relation (the
mean's scale and the add across relations)."""
import numpy as np
import torch


def stack_edges(edge_lists, num_nodes):
    """[(src, dst)] per relation -> (indptr int64 [R, num_nodes + 1] of absolute positions, col int32 [E]): the relation-stacked
    dst-sorted index (stable: ties in edge order), built with numpy alone."""
    indptr, col, base = [], [], 0
    for src, dst in edge_lists:
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        order = np.argsort(dst, kind="stable")
        p = np.zeros(num_nodes + 1, np.int64)
        np.cumsum(np.bincount(dst, minlength=num_nodes), out=p[1:])
        indptr.append(p + base); col.append(src[order].astype(np.int32)); base += len(src)
    return np.stack(indptr), (np.concatenate(col) if col else np.zeros(0, np.int32))


def _rows_out(out_size, rows):
    return int(out_size) if (out_size is not None and int(out_size) > 0) else int(rows)


def relation_aggregate(x, indptr, col, op="mean", out_size=None, per_relation=False, col_scale=None):
    """The definition, segment by segment, in fp64.  x [n_src, d] or [R, n_src, d]; col_scale None or [R, n_src]."""
    x = np.asarray(x, np.float64)
    indptr, col = np.asarray(indptr, np.int64), np.asarray(col, np.int64)
    R, rows = indptr.shape[0], indptr.shape[1] - 1
    M, d = _rows_out(out_size, rows), x.shape[-1]
    S = np.zeros((M, R, d)); A = np.zeros((M, R, d)); n = np.zeros((M, R))
    for r in range(R):
        xr = x[r] if x.ndim == 3 else x
        c = None if col_scale is None else np.asarray(col_scale, np.float64)[r]
        for v in range(M):
            b, e = int(indptr[r, v]), int(indptr[r, v + 1])
            if e == b:
                continue
            cc = col[b:e]
            t = xr[cc] if c is None else xr[cc] * c[cc][:, None]
            s = 1.0 / (e - b) if op == "mean" else 1.0
            S[v, r] = s * t.sum(0); A[v, r] = s * np.abs(t).sum(0); n[v, r] = (e - b) + 1
    if per_relation:
        return S, A, np.broadcast_to(n[:, :, None], S.shape)
    return S.sum(1), A.sum(1), np.broadcast_to(n.sum(1)[:, None], (M, d))


def relation_aggregate_grad(g, indptr, col, x_shape, op="mean", per_relation=False):
    """d/dx of sum(out * g) in fp64: g [M, d] (summed output) or [M, R, d]; x_shape (n_src, d) or (R, n_src, d).
    d x_r[u] = sum over the edges (u -> v) of relation r, v < M, of s_r(v) * g_r[v]; shared x: summed over r as well."""
    g = np.asarray(g, np.float64)
    indptr, col = np.asarray(indptr, np.int64), np.asarray(col, np.int64)
    R, M, n_src, d = indptr.shape[0], g.shape[0], x_shape[-2], x_shape[-1]
    G = np.zeros((R, n_src, d)); A = np.zeros((R, n_src, d)); n = np.zeros((R, n_src))
    for r in range(R):
        gr = g[:, r] if per_relation else g
        b, e = int(indptr[r, 0]), int(indptr[r, M])
        seg = np.diff(indptr[r, :M + 1])
        dst = np.repeat(np.arange(M), seg)
        s = (1.0 / np.maximum(seg, 1))[dst][:, None] if op == "mean" else 1.0
        np.add.at(G[r], col[b:e], s * gr[dst]); np.add.at(A[r], col[b:e], s * np.abs(gr[dst])); np.add.at(n[r], col[b:e], 1.0)
    n = n + (n > 0)                                          # (the scale of a mean / the add across relations)
    if len(x_shape) == 3:
        return G, A, np.broadcast_to(n[:, :, None], G.shape)
    return G.sum(0), A.sum(0), np.broadcast_to(n.sum(0)[:, None], (n_src, d))


# ------------------------------------------------------------------------------------------------
# plain torch, edge by edge (for grad_defs.grad_and_terms: fp64 gradients and their |terms|)
# ------------------------------------------------------------------------------------------------
def t_send_recv_relations(x, edge_lists, op="mean", out_size=None, per_relation=False, frozen=None):
    """edge_lists: [(src, dst)] int64 tensors per relation; x [n, d] or [R, n, d]."""
    rows = x.shape[-2]
    M = _rows_out(out_size, rows)
    outs = []
    for r, (src, dst) in enumerate(edge_lists):
        xr = x[r] if x.dim() == 3 else x
        keep = dst < M
        src, dst = src[keep], dst[keep]
        o = torch.zeros((M, x.shape[-1]), dtype=x.dtype, device=x.device).index_add(0, dst, xr[src])
        if op == "mean":
            o = o / torch.bincount(dst, minlength=M)[:M].clamp(min=1).to(x.dtype)[:, None]
        outs.append(o)
    return torch.stack(outs, 1) if per_relation else torch.stack(outs, 0).sum(0)


def t_rgcn(feat, weight, w_comp, edge_lists, out_size=None, frozen=None):
    """RGCNConv (pgl/nn/conv.py:1006-1024): sum over relations of mean_r(feat @ W_r); W = w_comp x weight when w_comp is given."""
    W = weight if w_comp is None else torch.einsum("rb,bio->rio", w_comp, weight)
    h = torch.einsum("ni,rio->rno", feat, W)
    return t_send_recv_relations(h, edge_lists, "mean", out_size)


def degrees(edge_lists, n, M):
    """(in-degree over all relations of the rows < M [M], out-degree over all relations towards rows < M [n])."""
    ind, outd = np.zeros(M), np.zeros(n)
    for src, dst in edge_lists:
        src, dst = np.asarray(src), np.asarray(dst)
        k = dst < M
        ind += np.bincount(dst[k], minlength=M)[:M]; outd += np.bincount(src[k], minlength=n)[:n]
    return ind, outd
