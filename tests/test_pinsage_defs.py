"""The PinSAGE neighbourhood definition (tests/pinsage_defs.py) on hand-worked walks, and the host twin on the graphs whose walks
have no choice to make (no GPU)."""
import numpy as np
import pytest

import pinsage_defs as P


@pytest.fixture(scope="module")
def pgl():
    import pgl_amd
    return pgl_amd


def _paths(rows, width):
    paths = np.full((len(rows), width), -1, np.int64)
    for i, r in enumerate(rows):
        paths[i, :len(r)] = r
    return paths, np.array([len(r) for r in rows], np.int64)


def test_two_cycle_one_neighbour_counted_at_the_odd_positions():
    # 0 <-> 1, R = 3 walks of L = 5 steps from 0: every walk is 0 1 0 1 0 1; positions 1, 3, 5 hold node 1, the rest the seed
    paths, lengths = _paths([[0, 1, 0, 1, 0, 1]] * 3, 6)
    nbr, cnt, num = P.visit_topk(paths, lengths, [0], 3, 2)
    assert nbr.tolist() == [[1, -1]] and cnt.tolist() == [[9, 0]] and num.tolist() == [1]
    assert nbr.dtype == np.int64 and cnt.dtype == np.int32 and num.dtype == np.int32


def test_star_ties_are_broken_by_id():
    # centre 0 -> leaves 1 .. 4 (dead ends).  Six walks: leaf 3 twice, leaf 2 twice, leaf 4 once, leaf 1 once
    paths, lengths = _paths([[0, 3], [0, 2], [0, 4], [0, 3], [0, 1], [0, 2]], 4)
    nbr, cnt, num, distinct, tie = P.visit_topk(paths, lengths, [0], 6, 3, full=True)
    assert nbr.tolist() == [[2, 3, 1]] and cnt.tolist() == [[2, 2, 1]] and num.tolist() == [3]
    assert distinct.tolist() == [4] and tie.tolist() == [True]          # 1 and 4 both have one visit: the smaller id is kept
    nbr, cnt, num = P.visit_topk(paths, lengths, [0], 6, 6)
    assert nbr.tolist() == [[2, 3, 1, 4, -1, -1]] and cnt.tolist() == [[2, 2, 1, 1, 0, 0]] and num.tolist() == [4]


def test_seed_without_successors_has_no_neighbours():
    paths, lengths = _paths([[4], [4]], 3)
    nbr, cnt, num = P.visit_topk(paths, lengths, [4], 2, 2)
    assert nbr.tolist() == [[-1, -1]] and cnt.tolist() == [[0, 0]] and num.tolist() == [0]


def test_self_loop_visits_of_the_seed_are_dropped():
    # 0 -> {0, 1}, 1 -> 0: the walk 0 0 1 0 0 visits the seed three times and node 1 once
    paths, lengths = _paths([[0, 0, 1, 0, 0], [0, 1, 0, 1, 0]], 5)
    nbr, cnt, num = P.visit_topk(paths, lengths, [0], 2, 1)
    assert nbr.tolist() == [[1]] and cnt.tolist() == [[3]] and num.tolist() == [1]


def test_two_seeds_take_their_own_rows():
    paths, lengths = _paths([[0, 1, 2], [0, 2], [5, 6, 6], [5]], 3)
    nbr, cnt, num = P.visit_topk(paths, lengths, [0, 5], 2, 2)
    assert nbr.tolist() == [[2, 1], [6, -1]] and cnt.tolist() == [[2, 1], [2, 0]] and num.tolist() == [2, 1]


# ---- the host twin where a walk has no choice -----------------------------------------------------------------------------------
def test_host_twin_on_the_two_cycle(pgl):
    indptr, col = P.csr_of([[0, 1], [1, 0]], 2)
    nbr, cnt, num = pgl.ops.host_walk_visit_topk(indptr, col, [0, 1], 3, 5, 2, seed=1)
    assert nbr.tolist() == [[1, -1], [0, -1]] and cnt.tolist() == [[9, 0], [9, 0]] and num.tolist() == [1, 1]


def test_host_twin_on_a_dead_end_and_a_pure_self_loop(pgl):
    indptr, col = P.csr_of([[0, 0], [2, 1]], 3)             # 0 only reaches itself, 1 has no successors, 2 -> 1
    nbr, cnt, num = pgl.ops.host_walk_visit_topk(indptr, col, [0, 1, 2], 4, 3, 2, seed=5)
    assert nbr.tolist() == [[-1, -1], [-1, -1], [1, -1]] and cnt.tolist() == [[0, 0], [0, 0], [4, 0]] and num.tolist() == [0, 0, 1]


def test_host_twin_on_the_star_counts_every_walk_once(pgl):
    indptr, col = P.csr_of([[0, 1], [0, 2], [0, 3], [0, 4]], 5)
    nbr, cnt, num = pgl.ops.host_walk_visit_topk(indptr, col, [0], 64, 3, 4, seed=2)
    assert num.tolist() == [4] and sorted(nbr[0].tolist()) == [1, 2, 3, 4] and int(cnt.sum()) == 64
    c = cnt[0].tolist()
    assert c == sorted(c, reverse=True)
    assert all(a < b for a, b, ca, cb in zip(nbr[0, :-1], nbr[0, 1:], c[:-1], c[1:]) if ca == cb)      # equal counts: ids ascending
