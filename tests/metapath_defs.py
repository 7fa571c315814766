"""Shared by tests/test_metapath_host.py and tests/test_metapath_gpu.py (definitions only, no tests, no project imports): a small
heterogeneous graph with the cases a metapath walk has to get right, the walk law restated from its definition
(examples/metapath2vec/datasets/sampling.py:350-398: step i follows a uniformly drawn successor under edge type
metapath[i % len(metapath)]) in plain Python, and the check that every step of a walk is an edge of its step's relation.

Nodes: authors 0 .. 3, papers 4 .. 8, venues 9 .. 10, and 11, which no edge touches.  Relations, by number:
  0 "a2p"  author -> paper, with a multi-edge (0 -> 4 twice); author 3 writes nothing
  1 "p2a"  paper -> author, with a multi-edge (8 -> 2 twice); paper 7 has no author, so a walk that reaches 7 under a2p and has
           to leave it under p2a ends there although 7 has successors under p2p: a dead end of the RELATION, not of the node
  2 "p2p"  paper -> paper (citations, with cycles: walks of any length exist)
  3 "p2v"  no edges at all
Author 3 is reached under p2a and has no successors under any relation (a dead end of the node); the venues and node 11 are
isolated."""
import collections

import numpy as np

N = 12
NODE_TYPES = ["a"] * 4 + ["p"] * 5 + ["v"] * 2 + ["a"]
EDGE_TYPES = ["a2p", "p2a", "p2p", "p2v"]
EDGES = {
    "a2p": np.array([[0, 4], [0, 4], [0, 5], [1, 5], [1, 6], [2, 6], [2, 7], [2, 8]], np.int64),
    "p2a": np.array([[4, 0], [4, 1], [5, 0], [5, 1], [5, 2], [6, 1], [6, 2], [6, 3], [8, 2], [8, 2]], np.int64),
    "p2p": np.array([[4, 5], [5, 6], [6, 4], [6, 7], [7, 8], [7, 4], [8, 7]], np.int64),
    "p2v": np.zeros((0, 2), np.int64),
}
# weights of the weighted cases, in edge order: a zero on 0 -> 5 (never followed), the two copies of 0 -> 4 weighted differently, a
# zero on one copy of 8 -> 2, several orders of magnitude
WEIGHTS = {
    "a2p": np.array([1.0, 3.0, 0.0, 2.0, 0.5, 1.0, 4.0, 0.25], np.float32),
    "p2a": np.array([1.0, 2.0, 0.5, 8.0, 1.0, 1.0, 1.0, 0.125, 0.0, 5.0], np.float32),
    "p2p": np.array([1.0, 1.0, 2.0, 6.0, 1.0, 3.0, 1.0], np.float32),
    "p2v": np.zeros(0, np.float32),
}
# the metapaths of the tests as relation numbers, by length
METAPATHS = {1: [2], 2: [0, 1], 3: [0, 2, 1], 4: [0, 2, 2, 1], 5: [0, 1, 0, 2, 1]}
LAW_STEPS, LAW_STARTS, LAW_WALKS = 4, (0, 2), 200000


def edge_lists():
    """The relations' [E_r, 2] edge lists in relation-number order."""
    return [EDGES[et] for et in EDGE_TYPES]


def successors(weights=None):
    """succs_by_relation[r][v]: the successors of v under relation r WITH multiplicity (one entry per edge); with `weights` (one
    vector of integer weights per relation, in edge order) entries are (dst, weight) and zero-weight edges are left out."""
    out = []
    for r, e in enumerate(edge_lists()):
        succ = [[] for _ in range(N)]
        for i, (s, d) in enumerate(e.tolist()):
            if weights is None:
                succ[s].append(d)
            elif int(weights[r][i]) > 0:
                succ[s].append((d, int(weights[r][i])))
        out.append(succ)
    return out


def edge_sets():
    return [set(map(tuple, e.tolist())) for e in edge_lists()]


def path_law(succs_by_relation, start, steps, metapath, phase=0):
    """{path tuple padded with -1 to steps + 1 nodes: probability} of every metapath walk of `steps` steps from `start`: the step
    from position t draws from succs_by_relation[metapath[(phase + t) % len(metapath)]][current node], uniformly over its entries
    (so a multi-edge counts with its multiplicity), or proportionally to the weights when the entries are (dst, weight)."""
    out = {}

    def rec(walk, pr):
        t = len(walk) - 1
        cand = succs_by_relation[metapath[(phase + t) % len(metapath)]][walk[-1]] if t < steps else []
        if not cand:
            out[tuple(walk) + (-1,) * (steps + 1 - len(walk))] = out.get(tuple(walk) + (-1,) * (steps + 1 - len(walk)), 0.0) + pr
            return
        pairs = [c if isinstance(c, tuple) else (c, 1) for c in cand]
        tot = float(sum(x for _, x in pairs))
        law = {}
        for d, x in pairs:
            law[d] = law.get(d, 0.0) + x / tot
        for d, px in law.items():
            rec(walk + [d], pr * px)

    rec([start], 1.0)
    return out


def follows(paths, lengths, edge_sets, metapath, phase=0):
    """True when every walk is a metapath walk as far as it goes: lengths in [1, width]; every consecutive pair (walk[t], walk[t+1])
    is an edge of relation metapath[(phase + t) % len(metapath)]; a walk shorter than the row ends at a node WITHOUT successors
    under the relation of its next step (it stopped because it had to); everything after it is -1."""
    paths, lengths = np.asarray(paths), np.asarray(lengths)
    width, L = paths.shape[1], len(metapath)
    sources = [set(s for s, _ in es) for es in edge_sets]
    for row, n in zip(paths.tolist(), lengths.tolist()):
        if not 1 <= n <= width or any(x != -1 for x in row[n:]):
            return False
        for t in range(n - 1):
            if (row[t], row[t + 1]) not in edge_sets[metapath[(phase + t) % L]]:
                return False
        if n < width and row[n - 1] in sources[metapath[(phase + n - 1) % L]]:
            return False
    return True


def walktimes_properties(walks, starts, names, walk_length, walk_times):
    """What metapath_randomwalk_with_walktimes promises, whichever sampler takes the first step: start by start, the second nodes
    are a sub-multiset of the start's metapath[0] successors of size min(walk_times, degree); every later step follows its
    relation; a walk is shorter than walk_length only at a dead end."""
    succ, number = successors(), {et: r for r, et in enumerate(EDGE_TYPES)}
    rel = [number[et] for et in names]
    want_count = [min(walk_times, len(succ[rel[0]][s])) for s in starts]
    assert len(walks) == sum(want_count)
    at = 0
    for s, c in zip(starts, want_count):
        mine = walks[at:at + c]
        at += c
        assert all(w[0] == s and 2 <= len(w) <= max(walk_length, 2) for w in mine)
        assert not collections.Counter(w[1] for w in mine) - collections.Counter(succ[rel[0]][s])
    rows = np.full((len(walks), max(walk_length, 2) - 1), -1, np.int64)
    for i, w in enumerate(walks):
        rows[i, :len(w) - 1] = w[1:]
    assert follows(rows, [len(w) - 1 for w in walks], edge_sets(), rel, 1 % len(rel))
