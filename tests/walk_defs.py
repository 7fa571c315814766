"""Shared by tests/test_walks_host.py and tests/test_walks_gpu.py: a small graph with the cases a walk has to get right, the
walk laws restated from their definition (pgl/sampling/walk.py, pgl/graph_kernel.pyx:140-224) in numpy, and a chi-square
check of empirical path counts against them."""
import numpy as np

# triangles (0 1 2, 0 2 5), multi-edges (0->2 twice, 2->5 twice), a self-loop (3->3), a dead end (4: no successors)
EDGES = np.array([[0, 1], [0, 2], [0, 2], [0, 5], [1, 2], [1, 0], [1, 4], [2, 0], [2, 3], [2, 5], [2, 5], [3, 3], [3, 1],
                  [3, 5], [5, 0], [5, 2], [5, 6], [6, 5]], dtype=np.int64)
N = 7


def successors(edges=EDGES, n=N):
    """succ lists WITH multiplicity (one entry per edge), the candidates of pgl's graph.successor."""
    succ = [[] for _ in range(n)]
    for s, d in edges.tolist():
        succ[s].append(d)
    return succ


def step_law(succ, walk, p, q, mode):
    """{next: probability} of the step from walk[-1], by definition.  mode: "uniform", "node2vec", "plus"."""
    cur = walk[-1]
    cand = succ[cur]
    if not cand:
        return {}
    if mode == "uniform" or len(walk) == 1:
        w = [1.0] * len(cand)
    else:
        prev = walk[-2]
        seen = set(succ[prev]) if mode == "node2vec" else set(x for v in walk[:-1] for x in succ[v])
        w = [1.0 / p if x == prev else (1.0 if x in seen else 1.0 / q) for x in cand]
    tot = sum(w)
    law = {}
    for x, wx in zip(cand, w):
        law[x] = law.get(x, 0.0) + wx / tot
    return law


def path_law(succ, start, steps, p, q, mode):
    """{path tuple padded with -1 to steps + 1 nodes: probability} of every walk of `steps` steps from `start`."""
    out = {}

    def rec(walk, pr):
        law = step_law(succ, walk, p, q, mode) if len(walk) <= steps else {}
        if not law:
            out[tuple(walk) + (-1,) * (steps + 1 - len(walk))] = pr
            return
        for x, px in law.items():
            rec(walk + [x], pr * px)

    rec([start], 1.0)
    return out


def chi2_paths(paths, law, min_expected=5.0):
    """Pearson chi-square of the rows of `paths` (int [W, steps + 1]) against `law`; cells expected below min_expected are
    pooled.  -> (statistic, degrees of freedom); every observed path must have positive probability."""
    from collections import Counter
    W = len(paths)
    seen = Counter(map(tuple, np.asarray(paths).tolist()))
    bad = [k for k in seen if k not in law]
    assert not bad, "paths the law gives probability 0: %s" % bad[:5]
    obs, exp, pool_o, pool_e = [], [], 0.0, 0.0
    for k, pr in law.items():
        e = W * pr
        if e < min_expected:
            pool_o += seen.get(k, 0); pool_e += e
        else:
            obs.append(seen.get(k, 0)); exp.append(e)
    if pool_e > 0:
        obs.append(pool_o); exp.append(pool_e)
    obs, exp = np.asarray(obs, np.float64), np.asarray(exp, np.float64)
    return float(((obs - exp) ** 2 / exp).sum()), len(obs) - 1


def assert_law(paths, law, what):
    from scipy.stats import chi2
    stat, dof = chi2_paths(paths, law)
    assert dof >= 3, (what, dof)
    pv = float(chi2.sf(stat, dof))
    assert pv > 1e-4, (what, stat, dof, pv)


# The laws the distribution tests draw from: (mode, p, q, steps).  plus at 3 steps: the step from position 2 weighs its
# candidates against succ(walk[0]) | succ(walk[1]), which differs from node2vec's succ(walk[1]) on this graph.
LAW_CASES = [("uniform", 1.0, 1.0, 3), ("node2vec", 0.25, 0.25, 3), ("node2vec", 4.0, 0.25, 3), ("plus", 4.0, 0.25, 3)]


def skip_gram_restated(paths, lengths, win_size, seed):
    """ops.skip_gram_pairs restated in numpy from the documented window hash (walk_core.hpp skip_gram_window)."""
    M = (1 << 64) - 1

    def mix64(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    salt = 0x5EED5EED5EED5EED
    src, dst = [], []
    for w, (row, l) in enumerate(zip(np.asarray(paths).tolist(), np.asarray(lengths).tolist())):
        key = mix64((seed ^ salt) ^ mix64(w))
        for i in range(l):
            h = mix64(key ^ mix64(i)) >> 32
            r = 1 + ((h * win_size) >> 32)
            for j in range(max(0, i - r), min(l - 1, i + r) + 1):
                if row[j] != row[i]:
                    src.append(row[i]); dst.append(row[j])
    return np.asarray(src, np.int64), np.asarray(dst, np.int64)
