"""The sparse embedding step in plain fp64 numpy: the sum of the entries' rows by id, then the four update formulas of
pgl_amd.embedding_ops.sparse_step, with the error bar an fp32 evaluation may show.  test_sparse_step_defs.py pins these formulas against
torch.optim; test_sparse_step_gpu.py holds the kernel to them."""
import numpy as np

KINDS = ("sgd", "adagrad", "rowwise_adagrad", "lazy_adam")
STATE_KEYS = {"sgd": (), "adagrad": ("s",), "rowwise_adagrad": ("s",), "lazy_adam": ("m", "v")}
EPS32 = float(np.finfo(np.float32).eps)
# fp32 roundings between the summed row and the stored element, counted along the longest chain (a host float such as lr, scale, beta,
# 1 - beta, a bias correction counts one for its own rounding; a square doubles what its operand carries, a square root halves it):
#   G = acc * scale: 2.                                  sgd:  lr * G 2 + 2, the subtraction 1                                       ->  5
#   adagrad: s' = fma(G, G, s) 4 + 1 = 5; sqrt 2.5 + 1, + eps 1 = 4.5; lr * G 4; the division 1, the subtraction 1               -> 10.5
#   rowwise: G^2 4, a chain of <= 8 fmas and 6 butterfly additions 14, / d 1, + s 1 = 20 (the state); sqrt 11, + 1e-10 1;
#            lr * G 4; division 1, subtraction 1 = 18                                                                             -> 20
#   lazy Adam: m = fma(b1, m, ob1 * G) 1 + 2 + 1 + 1 + 1 = 6; v = fma(b2, v, ob2 * G * G) 1 + 4 + 2 + 1 + 1 = 9; m / c1 8; v / c2 11,
#            sqrt 6.5, + eps 7.5; lr * mhat 10; division 10 + 7.5 + 1 = 18.5, subtraction 1                                      -> 19.5
ROUNDINGS = {"sgd": 5, "adagrad": 11, "rowwise_adagrad": 20, "lazy_adam": 20}


def sum_by_id(ids, rows, N, col=None, w=None, scale=1.0):
    """-> (uids [U] ascending, G [U, d], A [U, d], n [U]): per id in [0, N) that occurs, scale * sum w[m] rows[col[m]] in fp64, the sum of
    the terms' magnitudes and their number.  col=None: the entry's position; w=None: 1; a col outside rows adds a zero row."""
    ids, rows = np.asarray(ids, np.int64), np.asarray(rows, np.float64)
    M, R = ids.shape[0], rows.shape[0]
    col = np.arange(M) if col is None else np.asarray(col, np.int64)
    w = np.ones(M) if w is None else np.asarray(w, np.float64)
    ok = (col >= 0) & (col < R)
    terms = np.where(ok[:, None], w[:, None] * rows[np.clip(col, 0, max(R - 1, 0))], 0.0) * scale
    live = (ids >= 0) & (ids < N)
    uids = np.unique(ids[live])
    pos = np.searchsorted(uids, ids[live])
    G, A = np.zeros((uids.shape[0], rows.shape[1])), np.zeros((uids.shape[0], rows.shape[1]))
    np.add.at(G, pos, terms[live])
    np.add.at(A, pos, np.abs(terms[live]))
    return uids, G, A, np.bincount(pos, minlength=uids.shape[0])


def update(kind, w, st, G, lr, eps=1e-10, betas=(0.9, 0.999), t=1):
    """The rows w [U, d] and their state rows st (dict) after one step with the summed gradients G [U, d] -> (w', st')."""
    if kind == "sgd":
        return w - lr * G, {}
    if kind == "adagrad":
        s = st["s"] + G * G
        return w - lr * G / (np.sqrt(s) + eps), {"s": s}
    if kind == "rowwise_adagrad":              # shared_embedding.py:335-344: moment += mean(g^2); std = sqrt(moment) + 1e-10
        s = st["s"] + (G * G).mean(1)
        return w - lr * G / (np.sqrt(s) + 1e-10)[:, None], {"s": s}
    b1, b2 = betas
    m = b1 * st["m"] + (1 - b1) * G
    v = b2 * st["v"] + (1 - b2) * G * G
    return w - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps), {"m": m, "v": v}


def step(kind, table, state, ids, rows, col=None, w=None, scale=1.0, **hyper):
    """One step on copies -> (table', state', uids, bound_w [U, d], bound_state {k: [U(, d)]}).  The bounds: the fp32 sum lies within
    eG = 4 n eps sum|terms| of G (gpu_common.reassociation_bound); the update is evaluated at G, G - eG, G + eG (its first-order
    range) and with every magnitude down / up, and the formula's own fp32 roundings add ROUNDINGS[kind] eps of the magnitudes combined."""
    table, state = np.array(table, np.float64), {k: np.array(v, np.float64) for k, v in state.items()}
    uids, G, A, n = sum_by_id(ids, rows, table.shape[0], col, w, scale)
    eG = 4.0 * np.maximum(n, 1)[:, None] * EPS32 * A + float(np.finfo(np.float32).tiny)
    w0, st0 = table[uids], {k: v[uids] for k, v in state.items()}
    w1, st1 = update(kind, w0, st0, G, **hyper)
    K = ROUNDINGS[kind] * EPS32
    bw = K * (np.abs(w0) + np.abs(w1 - w0))
    bs = {k: K * np.abs(v) for k, v in st1.items()}
    sg = np.where(G < 0, -1.0, 1.0)
    for Gx in (G - eG, G + eG, G - sg * eG, G + sg * eG):       # shifted, and every magnitude down / up (the extremes of a mean of squares)
        wx, stx = update(kind, w0, st0, Gx, **hyper)
        bw = np.maximum(bw, np.abs(wx - w1) + K * (np.abs(w0) + np.abs(wx - w0)))
        bs = {k: np.maximum(bs[k], np.abs(stx[k] - st1[k]) + K * np.abs(stx[k])) for k in bs}
    table[uids] = w1
    for k in state:
        state[k][uids] = st1[k]
    return table, state, uids, bw, bs
