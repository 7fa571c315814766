"""Rows a16, e on ONE GPU and in ONE process -- the row-partitioned flow's compute (plan -> pack -> [emulated exchange] -> interior / boundary launches), the library's transport with one rank, bench.py's N > 1 code path as a dry run.  The multi-process runs are tests/test_gpu_distributed.py, the world-4 / 8 transport tests/test_e_transport_stub_rccl.py.

Regrouped by SURVEY section 8 row in round 6 (rounds 1-5 kept these tests in files named after the round that added them:
test_gpu_parity.py, test_gpu_round2..5.py); the shared fixtures and the per-element error bounds are in tests/gpu_common.py."""
import ctypes                                   # noqa: F401
import os                                       # noqa: F401
import subprocess                               # noqa: F401
import sys                                      # noqa: F401

import numpy as np                              # noqa: F401
import pytest
import torch                                    # noqa: F401

import golden_vectors as G                      # noqa: F401
import ref_ops as R                             # noqa: F401
from gpu_common import *                        # noqa: F401,F403

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# partitioned multi-GPU data flow with the HIP kernels (exchange simulated in-process: the GPU box
# has one device; the RCCL all-to-all itself is covered by the gloo tests + the driver's 8-GPU run)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("op", ["sum", "mean", "max", "min"])
def test_distgraph_compute_path_matches_single_gpu(pgl, world, op):
    from pgl_amd.distributed import DistGraph, HaloPlan
    n, e, d = 6000, 90000, 128
    edges, rng = rand_graph(n, e, 300 + world, hub=8000)
    x = dev(rng.standard_normal((n, d)).astype(np.float32))
    et = dev(edges)
    want = pgl.Graph(edges=et, num_nodes=n).send_recv(x, op)
    part = pgl.partition.random_partition(pgl.Graph(edges=edges, num_nodes=n), world)
    dgs = [DistGraph(HaloPlan(et, n, part, r, world)) for r in range(world)]
    packs = [dg.pack(dg.take_owned(x)) for dg in dgs]
    full = torch.zeros_like(want)
    for r, dg in enumerate(dgs):
        recv = []
        for q, dq in enumerate(dgs):
            so = np.concatenate([[0], np.cumsum(dq.plan.send_splits)])
            recv.append(packs[q][so[r]:so[r + 1]])
        recv = torch.cat(recv, 0)
        assert recv.shape[0] == dg.plan.n_halo
        full[dg.plan.own_global] = dg.aggregate_with_halo(dg.take_owned(x), recv, op)
    close_rows(host(full), host(want))


def test_distgraph_world1_is_plain_graph(pgl):
    from pgl_amd.distributed import DistGraph
    n, e = 3000, 40000
    edges, rng = rand_graph(n, e, 77)
    x = dev(rng.standard_normal((n, 64)).astype(np.float32))
    dg = DistGraph.from_global(dev(edges), n, 0, 1)
    out = dg.send_recv(dg.take_owned(x), "sum")
    want = pgl.Graph(edges=dev(edges), num_nodes=n).send_recv(x, "sum")
    assert torch.equal(out, want[dg.plan.own_global])


def test_eight_way_partition_in_process_rmat(pgl):
    """Config-4/5 data flow (8 parts, halo exchange emulated in-process) on RMAT scale 18, 4 M edges."""
    from pgl_amd.distributed import DistGraph, HaloPlan
    from pgl_amd.utils.rmat import rmat_edges
    N, E, d, world = 1 << 18, 4_000_000, 100, 8
    edges = rmat_edges(18, E, seed=3, device="cuda")
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    x = torch.randn(N, d, generator=gen, device="cuda")
    want = pgl.Graph(edges=edges, num_nodes=N).send_recv(x, "mean")
    part = torch.randint(0, world, (N,), generator=gen, device="cuda")
    dgs = [DistGraph(HaloPlan(edges, N, part, r, world)) for r in range(world)]
    packs = [dg.pack(dg.take_owned(x)) for dg in dgs]
    full = torch.empty_like(want)
    for r, dg in enumerate(dgs):
        recv = torch.cat([packs[q][sum(dq.plan.send_splits[:r]):sum(dq.plan.send_splits[:r + 1])] for q, dq in enumerate(dgs)], 0)
        full[dg.plan.own_global] = dg.aggregate_with_halo(dg.take_owned(x), recv, "mean")
    close_rows(host(full), host(want))
    assert sum(dg.plan.local_edges for dg in dgs) == E


def test_bench_multi_rank_code_path_dry_run():
    """bench.py --gpus 2 launched exactly as the driver launches it (torch.distributed.run, one process per rank), with
    PGLAMD_BENCH_DRYRUN=1 so that both ranks share cuda:0 and talk over gloo: partition, halo plan, pack, exchange,
    local + halo aggregation, max-over-ranks timing and the JSON line all execute (the RCCL transport itself cannot be
    exercised on a single-GPU box)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PGLAMD_BENCH_DRYRUN="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29731", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--scale", "16", "--edges", "1000000", "--target-scale", "15", "--target-edges", "400000", "--full"], env=env, capture_output=True, text=True, cwd=root, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["value"] > 0 and rec["scaling"] == "strong"
    assert rec["halo"]["local_edges"] > 0 and "roofline" in rec
    # the headline layout is north_star's: row partition + halo exchange, partitioned by the ENGINE'S OWN partitioner (no code built
    # from the reference on the default path)
    assert rec["config"]["parallelism"].startswith("row partition (kway)") and rec["halo"]["mode"] == "rows"
    # the |E| = 100 M leg of an N > 1 run (here at a size a shared GPU finishes in seconds)
    assert rec["target_size"]["value"] > 0 and len(rec["target_size"]["recv_bytes_per_rank"]) == 2
    assert rec["halo"]["exchange_only_ms"] > 0 and len(rec["halo"]["recv_bytes_per_rank"]) == 2
    flows = ("split", "fold", "accumulate", "pipeline", "rows2")
    assert rec["halo"]["flow"] in flows and rec["target_size"]["flow"] in flows
    # round 4: the candidates (fold / cost-model flow over torch.distributed, the cost-model flow over the library's transport) were
    # all tried and timed, the timed region ran on the fastest, every phase reported its wall time on stderr
    c = rec["halo"]["candidates"]
    assert [(k["flow"], k["transport"]) for k in c] == [("fold", "torch"), ("pipeline", "torch"), ("cost-model", "torch"), ("cost-model", "abi")]
    assert all(k["status"] == "ok" and k["trial_ms_per_step"] > 0 and k["trial_steps"] == 3 for k in c) and c[0]["ran_flow"] == "fold"
    assert c[1]["ran_flow"] == "pipeline"
    # round 6: what the cost model predicted rides next to every measured candidate and the target-size leg; one run refits the model's
    # wire constants (halo.calibration); the bf16 wire is timed as a labelled SECONDARY
    assert all(k["model_predicted_ms"] > 0 for k in c) and rec["target_size"]["model_predicted_ms"] > 0
    cal = rec["halo"]["calibration"]
    assert cal["model_constants_used"]["link_GBs"] == 150.0 and "fit" in cal
    assert rec["halo"]["wire_bf16_secondary"]["ms_per_step"] > 0 and "NOT the headline" in rec["halo"]["wire_bf16_secondary"]["note"]
    # round 5: per-rank phase times ride along (pack / before the wait / after the wait, each alone on its rank)
    ph = rec["halo"]["phases_ms_per_rank"]
    assert len(ph["pack"]) == 2 and len(ph["after_the_wait"]) == 2 and all(v >= 0 for v in ph["before_the_wait"])
    assert rec["halo"]["chosen"]["transport"] in ("torch", "abi") and "aborted" not in rec
    assert "phase 'partition + halo plan' done" in r.stderr and "phase 'target size leg" in r.stderr


def test_bench_phase_limit_ends_a_hung_run_with_the_best_completed_measurement():
    """A phase that does not finish (here: every phase after the first candidate) must end the run instead of hanging it, with a
    JSON line that reports the last COMPLETED measurement -- which is a FULL one (every candidate is measured over W warm-up + K
    steps), so the run still counts: rc 0, the line says which candidate it measured and which phase hung."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PGLAMD_BENCH_DRYRUN="1", PGLAMD_BENCH_HANG_AFTER="trial fold/torch")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29741", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--scale", "15", "--edges", "400000", "--phase-limit", "20"], env=env, capture_output=True, text=True, cwd=root, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["aborted"]["phase"].startswith("trial pipeline/torch") and rec["value"] > 0 and rec["n_gpus"] == 2
    assert not rec["metric"].startswith("ABORTED")
    assert "candidate fold/torch" in rec["timed"] and rec["steps"] == 3 and rec["halo"]["candidates"][0]["status"] == "ok"


def test_abi_rccl_transport_single_rank_plumbing(pgl):
    """pglamd_comm_init / pglamd_halo_exchange_{start,wait} on the one GPU of the box: a world-1 communicator, the own
    block is the copy the side stream performs -- this exercises RCCL loading, communicator creation, the side stream
    and both event hand-overs (N > 1 needs an 8-GPU node: the driver's scaling run)."""
    from pgl_amd.distributed import AbiTransport
    tr = AbiTransport(None)
    assert tr.world == 1 and tr.comm
    x = torch.randn(1000, 64, device="cuda")
    y = torch.empty_like(x)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                       # a non-default compute stream: ordering must come from the events
        z = x * 2.0                                     # "pack kernel" queued before the exchange
        w = tr.exchange(z, [1000], y, [1000])
        w.wait()
        out = y + 1.0                                   # consumer queued after the wait
    side.synchronize()
    assert torch.equal(out, x * 2.0 + 1.0)
    w2 = tr.exchange(z[:0], [0], y[:0], [0]); w2.wait()
    tr.close()


def test_distgraph_degenerate_partitions_on_the_engine(pgl):
    """A rank that owns nothing / a rank without halo rows / max-min with an empty boundary: the plan's empty index sets must go
    through csr_build and the kernels (no process group: the exchange is a no-op)."""
    from pgl_amd.distributed import DistGraph, HaloPlan
    rng = np.random.default_rng(8)
    n, e, d = 500, 4000, 32
    edges = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)], 1).astype(np.int64)
    x = dev(rng.standard_normal((n, d)).astype(np.float32))
    g = pgl.Graph(edges=edges, num_nodes=n).tensor()
    part = np.ones(n, np.int64)                                    # everything on rank 1 of 3
    for r in range(3):
        dg = DistGraph(HaloPlan(dev(edges), n, part, r, 3))
        xo = dg.take_owned(x)
        for op in ("sum", "mean", "max", "min"):
            out = dg.send_recv(xo, op)
            assert out.shape[0] == dg.plan.n_own
            if r == 1:
                want = g.send_recv(x, op)[dg.plan.own_global]
                close_rows(host(out), host(want), rtol=1e-5, atol_row=1e-5)
        xr = xo.clone().requires_grad_(True)
        dg.send_recv(xr, "sum").sum().backward()
        assert xr.grad.shape == xo.shape
        assert dg.halo_extend(xo).shape[0] == dg.plan.n_own
        # the generic ops (local graph over the extended node space) on an empty / halo-free share
        ye = dg.take_edges(dev(rng.standard_normal((e, 1)).astype(np.float32)))
        assert ye.shape[0] == dg.plan.local_edges
        assert dg.send_ue_recv(xo.clone().requires_grad_(True), ye, "mul", "sum").shape[0] == dg.plan.n_own
        assert dg.send_uv(xo, xo, "add").shape[0] == dg.plan.local_edges
        f = xo.reshape(-1, 4, 8)
        a = xo[:, :4].contiguous()
        assert dg.gat_aggregate(f, a, a, 0.2).shape == f.shape


def test_single_write_partitioned_flow_on_one_gpu(pgl):
    """DistGraph's interior / boundary launches (no process group: the exchanged rows are handed over by the test) reproduce
    the single-graph result for every reduce op, with and without the folded single launch, and with the 16-bit wire."""
    from pgl_amd.distributed import DistGraph, HaloPlan
    rng = np.random.default_rng(9)
    n, e, d, P = 3000, 60000, 64, 4
    edges = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)], 1).astype(np.int64)
    edges[rng.choice(e, 5000, replace=False), 1] = 5
    x = rng.standard_normal((n, d)).astype(np.float32)
    part = torch.from_numpy(rng.integers(0, P, n))
    et = dev(edges)
    dgs = [DistGraph(HaloPlan(et, n, part, r, P), device=torch.device("cuda")) for r in range(P)]
    xs = [dg.take_owned(dev(x)) for dg in dgs]
    packs = [dg.pack(xo) for dg, xo in zip(dgs, xs)]
    for op in ("sum", "mean", "max", "min"):
        want = R.c_send_u_recv(x, edges[:, 0], edges[:, 1], op)
        full = np.full_like(want, np.nan)
        for r, dg in enumerate(dgs):
            # what the all-to-all-v would deliver: peer q's block for me, in peer order
            offs = [np.concatenate([[0], np.cumsum(dgq.plan.pull_splits)]) for dgq in dgs]
            recv = torch.cat([packs[q][offs[q][r]:offs[q][r + 1]] for q in range(P)], 0)
            full[host(dg.plan.own_global)] = host(dg.aggregate_with_halo(xs[r], recv, op))
        if op in ("max", "min"):
            assert np.array_equal(full, want), op
        else:
            close_rows(full, want, rtol=1e-5, atol_row=1e-5, what=op)


def test_config4_eight_way_engine_partition_vs_oracle(pgl, config4):
    """The config-4 data flow as north_star states it: the graph row-partitioned 8 ways by the ENGINE'S partitioner (what stands
    where the reference calls METIS, pgl/partition.py:37-91), each rank packing the rows its peers pull, the all-to-all-v
    emulated in-process (one GPU), interior rows first and boundary rows from [owned | received] afterwards -- and the result
    compared with the ORACLE (not with the single-GPU engine)."""
    from pgl_amd.distributed import DistGraph, HaloPlan
    c = config4
    N, world, edges, x = c["N"], 8, c["edges"], c["x"]
    part = DistGraph.partition(edges, N, world, "kway")
    sizes = torch.bincount(part, minlength=world)
    assert int(sizes.min()) > 0
    pe = part.to(edges.device)[edges[:, 1]]
    work = torch.bincount(pe, minlength=world).double() + sizes.to(edges.device).double()      # in-degree + 1 per owned row
    assert float(work.max() / work.mean()) <= 1.05, work
    dgs = [DistGraph(HaloPlan(edges, N, part, r, world)) for r in range(world)]
    packs = [dg.pack(dg.take_owned(x)) for dg in dgs]
    full = torch.empty_like(x)
    cut = 0
    for r, dg in enumerate(dgs):
        recv = torch.cat([packs[q][sum(dq.plan.pull_splits[:r]):sum(dq.plan.pull_splits[:r + 1])] for q, dq in enumerate(dgs)], 0)
        assert recv.shape[0] == dg.plan.n_halo
        full[dg.plan.own_global] = dg.aggregate_with_halo(dg.take_owned(x), recv, "mean")
        cut += int(dg.plan.hal_rows.shape[0])
    assert sum(dg.plan.local_edges for dg in dgs) == c["E"]
    print("config 4, engine partitioner, P = 8: edge cut %.3f, rows per rank %s" % (cut / c["E"], sizes.tolist()))
    _check_full_output(host(full), c, "config 4 send_recv(mean), 8-way partitioned flow")


def test_config5_one_rank_share_streamed_plan_fp16(pgl):
    import time
    from pgl_amd.distributed import DistGraph, HaloPlan
    from pgl_amd.utils.rmat import rmat_slabs
    N, E, P, d, rank = 111_059_956, 1_615_685_872, 8, 128, 3
    slab = 48_000_000                                                   # 1/34 of the global list
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base_mem = torch.cuda.memory_allocated()
    t0 = time.time()
    plan = HaloPlan.from_edge_slabs(rmat_slabs(27, E, slab, seed=42, device="cuda", fold=N), N, rank, P)
    torch.cuda.synchronize()
    t_plan = time.time() - t0
    peak_plan = torch.cuda.max_memory_allocated() - base_mem
    assert plan.n_own == (N * (rank + 1)) // P - (N * rank) // P
    assert 0.5 * E / P < plan.local_edges < 2.0 * E / P and plan.local_edges <= E // 4        # a rank holds its share, never a quarter of the list
    assert slab * 16 <= E * 16 // 32
    assert int(plan.in_degree.sum()) == plan.local_edges
    assert sum(plan.halo_splits) == plan.n_halo and plan.halo_splits[rank] == 0 and sum(plan.pull_splits) == plan.n_send
    t0 = time.time()
    dg = DistGraph(plan)
    x_own = _node_features(plan.own_global, d, torch.float16)
    halo = _node_features(plan.halo_global, d, torch.float16)          # what the all-to-all-v would deliver (pull layout)
    out = dg.aggregate_with_halo(x_own, halo, "mean")
    torch.cuda.synchronize()
    t_first = time.time() - t0                                          # includes the two index builds (interior / boundary)
    t0 = time.time()
    for _ in range(3):
        out = dg.aggregate_with_halo(x_own, halo, "mean")
    torch.cuda.synchronize()
    t_step = (time.time() - t0) / 3
    peak_all = torch.cuda.max_memory_allocated() - base_mem
    assert out.dtype == torch.float16 and tuple(out.shape) == (plan.n_own, d)
    # sampled rows against fp64 on the same fp16-quantised inputs: reassociation bound + one fp16 rounding of the result
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rows = torch.randint(0, plan.n_own, (96,), generator=gen, device="cuda").unique()
    hub = torch.argmax(plan.in_degree).reshape(1)
    rows = torch.cat([rows, hub]).unique()
    src_of = torch.cat([plan.own_global[plan.loc_cols], plan.halo_global[plan.hal_cols]])      # global source of every local edge
    row_of = torch.cat([plan.loc_rows, plan.hal_rows])
    worst = 0.0
    for r in rows.tolist():
        srcs = src_of[row_of == r]
        deg = int(srcs.shape[0])
        assert deg == int(plan.in_degree[r])
        if deg == 0:
            assert float(out[r].abs().max()) == 0.0
            continue
        f = _node_features(srcs, d, torch.float16).double()
        want = f.sum(0) / deg
        # fp32 reassociation of the sum + THREE fp16 roundings: the sum is stored in fp16, 1 / degree is an fp16 value, so is their product
        # (a 16-bit mean applies its scale after the kernel: pgl_amd/distributed.py, aggregate_with_halo)
        bound = (2.0 * deg * 2.0 ** -24 * f.abs().sum(0) / deg) + 3.0 * 2.0 ** -11 * want.abs() + 1e-7
        err = (out[r].double() - want).abs()
        assert bool((err <= bound).all()), (r, deg, float(err.max()), float(bound.max()))
        worst = max(worst, float((err / bound).max()))
    msg = ("config 5, rank %d of %d: %d owned rows, %d in-edges (%.3f of |E|), %d halo rows, %d rows sent | plan from %d slabs of %d edges: "
           "%.1f s, peak device memory %.2f GB | first aggregation incl. index builds %.2f s, then %.1f ms / aggregation (fp16 rows, "
           "fp32 accumulation) | peak device memory overall %.2f GB | sampled rows incl. the hub (in-degree %d): worst error / bound = %.2f"
           % (rank, P, plan.n_own, plan.local_edges, plan.local_edges / E, plan.n_halo, plan.n_send, -(-E // slab), slab, t_plan, peak_plan / 1e9,
              t_first, t_step * 1e3, peak_all / 1e9, int(plan.in_degree.max()), worst))
    print(msg)
    import os
    os.makedirs("gpurun_out/r05", exist_ok=True)
    open("gpurun_out/r05/config5_one_rank_share.txt", "w").write(msg + "\n")
