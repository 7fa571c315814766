"""Ops queued behind unfinished work on a non-default stream, no graph anywhere (tests/replay_cases.py: run_side_stream_case): a
delay, the inputs overwritten in place, the op -- all on a side stream s that is still busy when the op returns -- must give what
the op gives eagerly on the new inputs.  A launch, copy or memset that escaped to another stream would read the old inputs.  The
eager result is held once to the op's definition.  Covered: the segment, edge, row-move, epilogue and index set-up ops; the chunked
aggregation family is not driven from here (replay_cases.NO_SIDE_STREAM_CASE).  Six ops that read back to the host go through the
same delay against their definitions: their read must wait on s."""
import numpy as np
import pytest
import torch

import ref_ops as R
import replay_cases as RC
from gpu_common import dev, host, pgl      # noqa: F401  (pgl: the module fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(pgl):
    return RC.Env(pgl)


@pytest.mark.parametrize("name", RC.case_names())
def test_side_stream_equals_eager(env, name):
    RC.run_side_stream_case(env, {c.name: c for c in RC.side_stream_cases()}[name])


# ---- six ops that read back to the host, behind a delay on a side stream: the read must wait on that stream ---------------------------
def _behind_delay(static, B, fn):
    """B copied into the static inputs and fn called on a side stream, both queued behind a delay.  (The op's own host read drains
    the stream, so it is idle when fn returns: what shows a read that did not wait is the result, which then comes from A.)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda._sleep(RC.SIDE_STREAM_SLEEP_CYCLES)
        for k, v in B.items():
            static[k].copy_(v)
        out = fn()
    s.synchronize()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def index(env):
    g = env.g
    succ = g._csr_succ_sorted()
    return {"dst": (host(env.csr.indptr), host(env.csr.col32), host(env.csr.eid32)), "succ": succ,
            "succ_host": (host(succ.indptr), host(succ.col32))}


def _ids(env, seed, count, hi=None):
    return env.randint(env.gen(seed), 0, hi or env.n, count)


def test_csr_build_on_a_side_stream(env):
    gen = env.gen(3)
    A = {"e": torch.stack([env.randint(gen, 0, env.n, env.E), env.randint(gen, 0, env.n, env.E)], 1)}
    B = {"e": dev(env.edges)}
    static = {k: v.clone() for k, v in A.items()}
    c = _behind_delay(static, B, lambda: env.ops.csr_build(static["e"][:, 1], static["e"][:, 0], env.n))
    degree, sorted_v, sorted_u, sorted_eid, indptr = R.c_build_index(env.dst, env.src, env.n)
    for got, want in ((c.indptr, indptr), (c.degree, degree), (c.sorted_v, sorted_v), (c.sorted_u, sorted_u), (c.sorted_eid, sorted_eid),
                      (c.col32, sorted_v), (c.row32, sorted_u), (c.eid32, sorted_eid)):
        assert np.array_equal(host(got).astype(np.int64), np.asarray(want, np.int64))


def test_sample_neighbors_on_a_side_stream(env, index):
    import sampling_defs as S
    A, B = {"nodes": _ids(env, 1, 2000)}, {"nodes": _ids(env, 2, 2000)}
    B["nodes"][::50] = env.n // 3                                  # the hub row
    static = {k: v.clone() for k, v in A.items()}
    nbr, cnt, eids = _behind_delay(static, B, lambda: env.ops.sample_neighbors(env.csr, static["nodes"], 10, seed=3, return_eids=True))
    want = S.sample_restated(*index["dst"], host(B["nodes"]), 10, 3)
    assert np.array_equal(host(cnt), want[1]) and np.array_equal(host(nbr), want[0]) and np.array_equal(host(eids), want[2])


def test_reindex_graph_on_a_side_stream(env):
    import sampling_defs as S
    def make(seed):
        gen = env.gen(seed)
        return {"nodes": torch.randperm(env.n, generator=gen, device="cuda")[:500], "nbr": env.randint(gen, 0, env.n, 4000),
                "count": torch.full((500,), 8, dtype=torch.int64, device="cuda")}
    A, B = make(1), make(2)
    static = {k: v.clone() for k, v in A.items()}
    src, dst, out_nodes = _behind_delay(static, B, lambda: env.ops.reindex_graph(static["nodes"], static["nbr"], static["count"]))
    want = S.reindex_restated(host(B["nodes"]), host(B["nbr"]), host(B["count"]))
    assert np.array_equal(host(src), want[0]) and np.array_equal(host(dst), want[1]) and np.array_equal(host(out_nodes), want[2])


def test_random_walk_on_a_side_stream(env, index):
    A, B = {"starts": _ids(env, 1, 3000)}, {"starts": _ids(env, 2, 3000)}
    static = {k: v.clone() for k, v in A.items()}
    paths, lengths = _behind_delay(static, B, lambda: env.ops.random_walk(index["succ"], static["starts"], 8, seed=5))
    want = env.ops.host_random_walk(*index["succ_host"], host(B["starts"]), 8, seed=5)      # the host twin: the same steps, the same RNG
    assert np.array_equal(host(paths), want[0]) and np.array_equal(host(lengths), want[1])


def test_sample_negatives_on_a_side_stream(env, index):
    import negative_defs as D
    A, B = {"src": _ids(env, 1, 300)}, {"src": _ids(env, 2, 300)}
    B["src"][::30] = 5                                             # the hub source
    static = {k: v.clone() for k, v in A.items()}
    neg = _behind_delay(static, B, lambda: env.ops.sample_negatives(index["succ"], static["src"], 3, seed=2))
    assert np.array_equal(host(neg), D.negatives_restated(*index["succ_host"], host(B["src"]), 3, seed=2)[0])


def test_induced_subgraph_on_a_side_stream(env, index):
    import subgraph_defs as D
    def make(seed):
        return {"nodes": torch.randperm(env.n, generator=env.gen(seed), device="cuda")[:1200]}
    A, B = make(1), make(2)
    static = {k: v.clone() for k, v in A.items()}
    got = _behind_delay(static, B, lambda: env.ops.induced_subgraph(env.csr, static["nodes"]))
    want = D.induced_restated(*index["dst"], host(B["nodes"]), env.n)
    for g, w in zip(got, want):
        assert np.array_equal(host(g), w)
