#!/usr/bin/env python3
"""bench.py -- aggregated edges/sec of the GCN send+recv_sum hot path (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is ONE pass of Graph.send_recv(x, "sum") (= pglamd_aggregate through the C ABI) over the whole synthetic graph with the
feature matrix already resident in HBM.  Workload (config.workload): BASELINE.json configs[1] -- RMAT (0.57,0.19,0.19,0.05)
|V| = 2^20, |E| = 20 M, d = 128 fp32, graph seed 42, feature seed 7.

A plain run sets up, warms up, times the K steps and prints one JSON line: metric / value / unit / higher_is_better / dtype /
ms_per_step (host clock over the K steps), config, and roofline.headline_workload (the dominant kernel's HIP-event time inside
the timed steps, the section 8(d) byte model, the committed PMC traffic when its stamp matches).  Everything else below -- the
event-timed distribution, the GCN-norm leg, the known-bytes roofline legs, the target-size leg, the CPU baselines and, at N > 1,
the exchange-only / per-rank-phase / bf16-wire diagnostics and the target-size leg -- runs only with --full.

--dump-outputs DIR: after the timed steps, what the last step returned (the [|V|, d] output of send_recv) is written as float
.npy files -- the whole output when it fits 48 MB, else a fixed seeded sample of rows (send_recv_sum_rows.npy, their ids in
send_recv_sum_row_ids.npy) plus every row's sum in float64 (send_recv_sum_row_sums.npy).  The inputs are seeded, so two builds
run with the same arguments can be compared output for output.  At N > 1 every rank writes its owned rows, prefixed rank<r>_.

--full, N = 1: the JSON line also holds
  roofline      PHYSICAL: achieved / frac come from the same kernel (agg_flat_kernel, d = 128 fp32 sum) on a graph whose gathered
                bytes are KNOWN (uniform in-degree-19 graph over 8.6 GB of features: <= 3.5 % of the gathers can hit any cache),
                timed with HIP events in this run; `traffic` = PMC bytes of that leg from profiles/r06/traffic.json, replayed only
                when the file's stamp (kernel symbol + sha256 of the kernel sources) matches this tree, else null.  The headline
                workload's own figures -- section 8(d) model bytes / kernel time, which is NOT a bandwidth on RMAT (hub rows live
                in L2 / Infinity Cache) -- ride along under roofline.headline_workload, labelled; no ratio above 1 is printed.
  timing        median / p95 over 100 event-timed runs of the step (SURVEY 8d protocol)
  gcn_norm      send_recv(sum) with both degree norms, fused (one kernel) and unfused (three ops) -- SURVEY 8d "report both"
  target_size   |E| = 100 M (north_star's size, SURVEY 8d C2'), same seeds, same op
  cpu_baseline  the oracle's C port of the Paddle CPU kernel (serial raw-COO loop, 1 core; the checker, never the product), the
                reference's own compiled build_index, an OpenMP CSR variant, scipy CSR @ dense and torch.index_add_ as sanity baselines

N > 1 (strong scaling, the SAME global graph and features): north_star's layout -- row partition by the engine's own partitioner
(pglamd_partition_edges: in-degree + 1 and rows balanced; standing where north_star says "METIS-partitioned"), one
RCCL halo all-to-all-v per step, interior rows aggregated while the rows travel, boundary rows afterwards from [owned | received]:
every output row written once (DistGraph).  value = global |E| / max-rank time; halo bytes ride along, and with --full the
exchange-only time per rank and target_size = the |E| = 100 M graph through the same flow.  The run is self-diagnosing
(PhaseWatchdog): per-phase wall times on stderr, candidates tried from the most conservative flow / transport up (halo.candidates: fold over torch.distributed, the cost
model's flow over torch.distributed, the same over the library's own RCCL communicator -- --transport), the timed region on the
fastest; a phase that exceeds its limit ends the run with the best COMPLETED measurement instead of hanging, and a failure of
the target-size leg cannot lose the headline.
"""
import os
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: required by RCCL on this driver (set before HIP initialises)
import argparse  # noqa: E402
import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s)


def algorithmic_bytes(E, N, d, s):
    """B = E*(d*s + 4) + N*(d*s + 8)."""
    return E * (d * s + 4) + N * (d * s + 8)


DUMP_BYTES = 48 << 20          # --dump-outputs: the whole output up to this size, else a seeded row sample of about this size


def dump_outputs(dirname, out, row_ids, prefix="", budget=DUMP_BYTES):
    """--dump-outputs: `out` ([rows, d] fp32 on the GPU, what the last timed step returned) as .npy files under `dirname`.
    row_ids[i] = the global node id of out[i].  Whole when it fits `budget`; otherwise a fixed seeded sample of rows (ids as
    float64, exact below 2^53) plus, while they take at most a quarter of the budget, every row's float64 sum, so no row goes
    unchecked.  -> total bytes written."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    path = lambda name: os.path.join(dirname, prefix + name + ".npy")
    n = int(out.shape[0])
    row_bytes = out.numel() // max(n, 1) * 4
    ids = row_ids.to(torch.float64).cpu().numpy()
    if n * (row_bytes + 8) <= budget:
        np.save(path("send_recv_sum"), out.float().cpu().numpy())
        np.save(path("send_recv_sum_row_ids"), ids)
        return n * (row_bytes + 8)
    sum_bytes = n * 8 if n * 8 <= budget // 4 else 0
    if sum_bytes:
        np.save(path("send_recv_sum_row_sums"), out.sum(dim=tuple(range(1, out.dim())), dtype=torch.float64).cpu().numpy())
    k = max(1, (budget - sum_bytes) // (row_bytes + 8))
    pick = np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
    np.save(path("send_recv_sum_rows"), out[torch.from_numpy(pick).to(out.device)].float().cpu().numpy())
    np.save(path("send_recv_sum_row_ids"), ids[pick])
    return k * (row_bytes + 8) + sum_bytes


TRAFFIC_FILES = ("profiles/r06/traffic.json",)
KERNEL_SOURCES = ("pgl_amd/csrc/aggregate_flat.hpp", "pgl_amd/csrc/aggregate.hpp", "pgl_amd/csrc/aggregate.hip", "pgl_amd/csrc/common.hpp")


def kernel_source_hash():
    """sha256 over the sources of the dominant kernel: the stamp a recorded PMC profile must carry to be replayed."""
    import hashlib
    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()


def recorded_traffic(key, kernel):
    """(bytes, source) -- HBM-side bytes per launch of the dominant kernel as RECORDED in the committed PMC profile of this
    exact workload (separate rocprofv3 --pmc passes, FETCH/WRITE calibrated as MI355X_MICROARCH.md prescribes;
    scripts/gpu_session.sh profile).  PMC counters cannot be collected from inside a timed run, so this is a replayed figure:
    it is returned only when the profile's stamp -- kernel symbol + sha256 of the kernel's sources -- matches what THIS run
    launched from THIS tree; otherwise (None, reason), and the line says traffic: null."""
    for rel in TRAFFIC_FILES:
        try:
            t = json.load(open(os.path.join(ROOT, rel)))
        except Exception:
            continue
        st = t.get("stamp", {})
        if st.get("source_sha256") != kernel_source_hash():
            return None, "%s was recorded from other kernel sources (stamp %s...): stale, not replayed" % (rel, str(st.get("source_sha256"))[:12])
        w = t.get("workloads", {}).get(key)
        if w is None:
            return None, "%s holds no PMC pass of workload %s" % (rel, key)
        if kernel and w.get("kernel") and w["kernel"] != kernel:
            return None, "%s recorded kernel %s, this run launched %s" % (rel, w["kernel"], kernel)
        return w["traffic_bytes"], ("%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, calibrated; stamp matches this "
                                    "tree's kernel sources; replayed, not measured in this run)" % rel)
    return None, "no committed PMC profile"


def step_distribution(step, n=100, warm=10):
    """SURVEY 8(d) timing protocol: n runs, each between its own pair of events on the launch stream -> median and p95 (ms)."""
    for _ in range(warm):
        step()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record(); step(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return {"runs": n, "median_ms": ts[n // 2], "p95_ms": ts[min(n - 1, int(round(0.95 * n)) - 1)], "min_ms": ts[0], "max_ms": ts[-1]}


def timed_leg(pgl, step, steps, warmup):
    """-> (ms per step by host clock, dominant-kernel ms per launch from the library's HIP events, launches/step, kernel name)."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    pgl.ops.profile_begin()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kms, n = pgl.ops.profile_end()
    return dt / steps * 1e3, kms / max(n, 1), n / steps, pgl.ops.profile_last_kernel()


def no_reuse_legs(pgl, dev, d, steps=5, warmup=2):
    """Roofline legs whose gathered bytes are KNOWN, so achieved/peak is a physical fraction (<= 1):
      permutation   every source row is gathered exactly once, in random order (degree 1): no reuse is possible;
      uniform_deg19 uniform-random sources, in-degree 19 like the benchmark graph, over 2^24 rows = 8.6 GB of features:
                    at most (256 MiB Infinity Cache + 32 MiB L2) / 8.6 GB = 3.4 % of the gathers can hit a cache, and the
                    known bytes are discounted by that bound.
    Both run the SAME kernel as the headline workload (agg_flat_kernel, d = 128 fp32)."""
    out = {}
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    # --- permutation graph ---
    n = 1 << 23
    perm = torch.randperm(n, generator=gen, device=dev)
    g = pgl.Graph(edges=torch.stack([perm, torch.arange(n, device=dev)], 1), num_nodes=n); g.adj_dst_index
    x = torch.randn(n, d, generator=gen, device=dev)
    ms, kms, _, kname = timed_leg(pgl, lambda: g.send_recv(x, "sum"), steps, warmup)
    known = n * (d * 4 + 8) + n * d * 4                           # x row + (row, col) ids read, out row written
    out["permutation"] = {"rows": n, "edges": n, "known_bytes": known, "kernel_ms": kms, "kernel": kname,
                          "achieved": known / (kms * 1e-3) / 1e9, "frac": known / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    del g, x, perm
    # --- uniform random, in-degree 19 ---
    n, deg = 1 << 24, 19
    e = n * deg
    src = torch.randint(0, n, (e,), generator=gen, device=dev)
    dst = torch.arange(n, device=dev).repeat_interleave(deg)
    g = pgl.Graph(edges=torch.stack([src, dst], 1), num_nodes=n); g.adj_dst_index
    del src, dst
    x = torch.randn(n, d, generator=gen, device=dev)
    ms, kms, _, kname = timed_leg(pgl, lambda: g.send_recv(x, "sum"), steps, warmup)
    cache_bound = (256 + 32) * 2.0 ** 20 / (n * d * 4)
    known = e * (d * 4) * (1.0 - cache_bound) + e * 8 + n * d * 4
    out["uniform_deg19"] = {"rows": n, "edges": e, "known_bytes": known, "cache_hit_bound": cache_bound, "kernel_ms": kms,
                            "kernel": kname, "edges_per_s": e / (kms * 1e-3),
                            "achieved": known / (kms * 1e-3) / 1e9, "frac": known / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    del g, x
    torch.cuda.empty_cache()
    # --- uniform random sources over a table INSIDE the Infinity Cache (2^18 rows x 512 B = 128 MB: 32 x one XCD's L2, half of the 256 MiB
    #     Infinity Cache), in-degree 19 over 2^21 output rows.  At most 4 MB / 128 MB = 3 % of the gathers can hit an L2, and after the first
    #     launch none has to come from DRAM: known bytes / time is what the FABRIC + INFINITY CACHE deliver to this kernel's access pattern
    #     (random 512-byte rows) -- the ceiling the RMAT launch's L2-miss traffic is read against (profiles/r06/tablesize.txt: the rate is
    #     flat, 6.8 - 7.0 TB/s of gathered rows, for tables of 64 ... 512 MB and falls only beyond: the memory side, not DRAM, sets it).
    n_out, R, deg = 1 << 21, 1 << 18, 19
    e = n_out * deg
    src = torch.randint(0, R, (e,), generator=gen, device=dev)
    dst = torch.arange(n_out, device=dev).repeat_interleave(deg)
    g = pgl.Graph(edges=torch.stack([src, dst], 1), num_nodes=n_out); g.adj_dst_index
    del src, dst
    x = torch.randn(n_out, d, generator=gen, device=dev)
    ms, kms, _, kname = timed_leg(pgl, lambda: g.send_recv(x, "sum"), steps, warmup)
    l2_bound = 4.0 * 2 ** 20 / (R * d * 4)
    # gathered rows + ids read + rows written.  (NOT discounted by the 3 % of the gathers that could hit an L2: the counters say they do not --
    #  164.8 M memory-side 128-byte read requests per launch = 21.1 GB for 20.4 GB of gathered rows + 0.3 GB of ids, profiles/r06/tablesize_pmc.txt)
    past_l2 = e * (d * 4) + e * 8 + n_out * d * 4
    out["infinity_cache_table"] = {"table_rows": R, "table_bytes": R * d * 4, "rows": n_out, "edges": e, "l2_hit_bound": l2_bound,
                                   "bytes_past_l2": past_l2, "kernel_ms": kms, "kernel": kname, "edges_per_s": e / (kms * 1e-3),
                                   "achieved": past_l2 / (kms * 1e-3) / 1e9}
    del g, x
    torch.cuda.empty_cache()
    return out


def gcn_norm_leg(pgl, g, x, E, steps=10, warmup=3):
    """"send_recv(sum) incl. both norm scalings fused or not -- report both": GCNConv's h * norm -> send_recv(sum) ->
    * norm (pgl/nn/conv.py:242-250) as ONE aggregation with both degree norms inside (Graph.send_recv_scaled) and as the
    reference's three ops."""
    norm = pgl.nn.functional.degree_norm(g)                          # [N, 1] fp32, clip(indegree, 1) ** -0.5
    fused = lambda: g.send_recv_scaled(x, norm, norm)
    unfused = lambda: g.send_recv(x * norm, "sum") * norm
    tf = step_distribution(fused, n=30, warm=warmup)
    tu = step_distribution(unfused, n=30, warm=warmup)
    return {"what": "x * norm -> send_recv(sum) -> * norm at the headline workload (GCNConv's aggregation, pgl/nn/conv.py:242-250)",
            "fused_ms": tf["median_ms"], "fused_p95_ms": tf["p95_ms"], "fused_edges_per_s": E / (tf["median_ms"] * 1e-3),
            "unfused_ms": tu["median_ms"], "unfused_p95_ms": tu["p95_ms"], "unfused_edges_per_s": E / (tu["median_ms"] * 1e-3)}


def target_size_leg(pgl, dev, d, scale=22, E=100_000_000, steps=10, warmup=3):
    """north_star's target size (SURVEY 8d C2'): RMAT scale 22, |E| = 100 M, same seeds, same op."""
    from pgl_amd.utils.rmat import rmat_edges
    N = 1 << scale
    edges = rmat_edges(scale, E, seed=42, device=dev)
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    x = torch.randn(N, d, generator=gen, device=dev, dtype=torch.float32)
    g = pgl.Graph(edges=edges, num_nodes=N); g.adj_dst_index
    ms, kms, lps, kname = timed_leg(pgl, lambda: g.send_recv(x, "sum"), steps, warmup)
    B = algorithmic_bytes(E, N, d, 4)
    tb, tsrc = recorded_traffic("scale%d_e%d_d%d_f32" % (scale, E, d), kname)
    dist_ = step_distribution(lambda: g.send_recv(x, "sum"), n=30, warm=2)
    rec = {"workload": "RMAT scale %d |V|=%d |E|=%d d=%d fp32 (north_star target size, SURVEY 8d C2')" % (scale, N, E, d),
           "value": E / (ms * 1e-3), "unit": "edges/s", "ms_per_step": ms, "steps": steps, "median_ms": dist_["median_ms"],
           "p95_ms": dist_["p95_ms"], "kernel_ms": kms, "kernel": kname,
           "model_bytes_per_launch": B, "model_bytes_over_kernel_time_GBs": B / (kms * 1e-3) / 1e9,
           "model_note": "section 8(d) byte model (no cache reuse assumed) / kernel time: NOT a bandwidth -- RMAT hub rows are "
                         "served from L2 / Infinity Cache, so it may exceed the 8 TB/s peak; the physical fraction is roofline.frac",
           "traffic": tb, "traffic_source": tsrc,
           "traffic_frac_of_peak": (tb / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS) if tb else None}
    del g, x, edges
    torch.cuda.empty_cache()
    return rec


def target_size_leg_dist(pgl, dev, d, rank, world, args, timed, note, steps=10):
    """The |E| = 100 M graph of target_size_leg, row-partitioned over the N ranks of this run (same flow as the headline)."""
    import torch.distributed as dist
    from pgl_amd.distributed import DistGraph
    from pgl_amd.utils.rmat import rmat_edges
    scale, E = args.target_scale, args.target_edges
    N = 1 << scale
    note("target size: generating RMAT scale %d, %d edges" % (scale, E))
    edges = rmat_edges(scale, E, seed=42, device=dev)
    t0 = time.perf_counter()
    dg = DistGraph.from_global(edges, N, rank, world, method=args.partition, device=dev, push=args.push, row_order=args.row_order)
    t_plan = time.perf_counter() - t0
    note("target size: partition + plan %.1f s" % t_plan)
    del edges
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    x_own = dg.take_owned(torch.randn(N, d, generator=gen, device=dev, dtype=torch.float32))
    fn = lambda: dg.send_recv(x_own, "sum")
    fn(); fn(); fn()
    t = timed(fn, steps) / steps * 1e3
    t_x = timed(lambda: dg.exchange_only(x_own), 5) / 5 * 1e3
    st = dg.stats()                                              # (after the timed steps: "flow" is the one that ran)
    pred = torch.tensor([dg.model_estimates(d).get(st["flow"], float("nan"))], dtype=torch.float64, device=dev)
    dist.all_reduce(pred, op=dist.ReduceOp.MAX)
    try:
        pk = torch.tensor([dg.phase_times(x_own, iters=5)["pack_ms"]], dtype=torch.float64, device=dev)
    except Exception:                                            # noqa: BLE001 -- a diagnostic
        pk = torch.zeros(1, dtype=torch.float64, device=dev)
    dist.all_reduce(pk, op=dist.ReduceOp.MAX)
    allp = torch.zeros((world, 3), dtype=torch.float64, device=dev)
    allp[rank, 0], allp[rank, 1], allp[rank, 2] = float(st["recv_rows"]) * d * 4, float(st["local_edges"]), float(st["local_rows"])
    dist.all_reduce(allp)
    rec = {"workload": "RMAT scale %d |V|=%d |E|=%d d=%d fp32 (north_star target size, SURVEY 8d C2'), row partition (%s) x%d"
                       % (scale, N, E, d, st["partition"], world),
           "value": E / (t * 1e-3), "unit": "edges/s", "ms_per_step": t, "steps": steps, "exchange_only_ms": t_x,
           "model_predicted_ms": float(pred.item()), "pack_ms": float(pk.item()),
           "partition_and_plan_s": t_plan, "pushed_pairs": st["pushed_pairs"], "flow": st["flow"], "recv_bytes_per_rank": allp[:, 0].tolist(),
           "edges_per_rank": allp[:, 1].tolist(), "rows_per_rank": allp[:, 2].tolist()}
    del dg, x_own
    torch.cuda.empty_cache()
    return rec


class PhaseWatchdog(object):
    """N > 1 runs are self-diagnosing: every phase (partition + plan, each candidate's trial, the timed region, the target-size
    leg) runs under a deadline.  A phase that is still running at its deadline -- a collective that never completes, a rank
    that died inside one -- ends the run instead of hanging it: rank 0 prints the JSON line of the best measurement COMPLETED so
    far (labelled with the phase that hung), every rank leaves with os._exit.  Each rank runs its own watchdog on the same
    schedule, so the ranks stuck behind the one that hung leave as well.  Phase wall times go to stderr on rank 0."""

    def __init__(self, rank, emit, grace=3.0):
        import threading
        self.rank, self.emit, self.grace = rank, emit, grace
        self.best = None                    # callable -> the record to print if a later phase hangs (rank 0 only)
        self.hang_next = False
        self.timed_done = False             # set once the timed region has completed on this rank
        self.deadline, self.name, self.t0 = None, None, time.perf_counter()
        self.t_phase = 0.0
        self.lock = threading.Lock()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def note(self, msg):
        if self.rank == 0:
            print("[bench %7.1fs] %s" % (time.perf_counter() - self.t0, msg), file=sys.stderr, flush=True)

    def begin(self, name, seconds):
        with self.lock:
            self.name, self.deadline, self.t_phase = name, time.perf_counter() + seconds, time.perf_counter()
        self.note("phase %r (limit %.0f s)" % (name, seconds))
        if self.hang_next:                                           # test seam (PGLAMD_BENCH_HANG_AFTER=<phase>): the phase after it never finishes
            while True:
                time.sleep(1.0)

    def end(self):
        with self.lock:
            name, dt = self.name, time.perf_counter() - self.t_phase
            self.name, self.deadline = None, None
        if name == os.environ.get("PGLAMD_BENCH_HANG_AFTER"):
            self.hang_next = True
        self.note("phase %r done in %.2f s" % (name, dt))
        return dt

    def _run(self):
        while True:
            time.sleep(0.25)
            with self.lock:
                late = self.deadline is not None and time.perf_counter() > self.deadline
                name = self.name
            if not late:
                continue
            print("[bench] rank %d: phase %r exceeded its limit -- ending the run" % (self.rank, name), file=sys.stderr, flush=True)
            # Exit code: 0 only when the TIMED REGION had completed (the record then is the contract's measurement and
            # only an extra leg hung); a run that ends before it exits 3, and the record it leaves behind for diagnosis says so in
            # its `metric` string, so a driver reading value / n_gpus / rc cannot take a 3-step candidate trial for the headline.
            rc = 3
            if self.best is not None:
                try:
                    rec = self.best()                                # (the same record on every rank: only rank 0 prints it)
                    rec["aborted"] = {"phase": name, "what": "this phase did not finish within its limit; the line reports the best "
                                                             "measurement completed before it"}
                    full = not str(rec.get("timed", "")).startswith("trial")
                    if not full:
                        rec["metric"] = "ABORTED before the timed region (candidate trial only, not a measurement): " + rec["metric"]
                    if self.rank == 0:
                        self.emit(rec)
                    else:
                        time.sleep(self.grace)                       # rank 0 prints first
                    rc = 0 if full else 3
                except Exception as ex:                              # noqa: BLE001
                    print("[bench] could not emit the fallback record: %r" % ex, file=sys.stderr, flush=True)
            os._exit(rc)


def cpu_baseline(edges_cpu, x_cpu, budget_s=12.0):
    """Oracle C port of the Paddle CPU kernel (kind "port": serial loop over the edges in raw COO
    order, 1 core) timed on this box: whole passes over the SAME graph and features until about
    `budget_s` seconds of CPU work have been spent (>= 1 pass).  The OpenMP row-parallel CSR variant on
    all host cores rides along as `omp_*` (not the reference's algorithm, just the all-cores number)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_ops as R
    e = edges_cpu.numpy()
    x = x_cpu.numpy()
    R.lib()
    passes, spent = 0, 0.0
    while passes < 1 or spent < budget_s:
        t0 = time.perf_counter()
        R.c_send_u_recv(x, e[:, 0], e[:, 1], "sum")
        spent += time.perf_counter() - t0
        passes += 1
    rec = {"value": len(e) * passes / spent, "unit": "edges/s", "cores": 1, "kind": "port",
           "sample": "%d full pass(es) over the same RMAT graph (%d edges, [N,%d] fp32 features), %.1f s, "
                     "oracle/ref_ops.c ref_send_u_recv_f32 (serial raw-COO loop)" % (passes, len(e), x.shape[1], spent)}
    try:
        # the reference's OWN native CPU path (north_star: "graph_kernel.pyx CPU path timed on the same box"):
        # graph_kernel.build_index compiled from /root/reference by oracle/build_ref.py (oracle/_ref, prebuilt .so travels)
        import numpy as np
        import ref_native
        gk = ref_native.load(build_if_missing=False)
        if gk is not None:
            u, v = np.ascontiguousarray(e[:, 1]), np.ascontiguousarray(e[:, 0])
            t0 = time.perf_counter()
            gk.build_index(u, v, int(x.shape[0]))
            t = time.perf_counter() - t0
            rec["reference_native"] = {"what": "pgl/graph_kernel.pyx build_index (the reference's compiled CSR build, 1 core), "
                                               "one pass over the same %d edges" % len(e),
                                       "kind": "reference", "seconds": t, "value": len(e) / t, "unit": "edges/s", "cores": 1}
    except Exception as ex:                                          # noqa: BLE001 -- the port above remains the baseline
        rec["reference_native"] = {"error": repr(ex)}
    try:
        _, sv, _, _, ip = R.c_build_index(e[:, 1], e[:, 0], x.shape[0])
        R.c_csr_spmm_sum_omp(x, ip, sv)
        t0 = time.perf_counter()
        R.c_csr_spmm_sum_omp(x, ip, sv)
        rec["omp_value"] = len(e) / (time.perf_counter() - t0)
        rec["omp_cores"] = os.cpu_count()
        # two independent formulations as sanity baselines (one pass each)
        import numpy as np
        import scipy.sparse as sp
        A = sp.csr_matrix((np.ones(len(e), np.float32), sv, ip), shape=(x.shape[0], x.shape[0]))
        t0 = time.perf_counter()
        ref = A @ x
        rec["scipy_csr_value"] = len(e) / (time.perf_counter() - t0)
        xt, src, dst = torch.from_numpy(x), torch.from_numpy(e[:, 0]), torch.from_numpy(e[:, 1])
        t0 = time.perf_counter()
        got = torch.zeros_like(xt).index_add_(0, dst, xt[src])
        rec["torch_index_add_value"] = len(e) / (time.perf_counter() - t0)
        rec["torch_threads"] = torch.get_num_threads()
        rec["sanity_max_abs_diff"] = float(np.abs(got.numpy() - ref).max())
    except Exception as ex:                                          # noqa: BLE001
        rec["sanity_error"] = repr(ex)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--partition", default="kway", choices=["kway", "random", "auto"],
                    help="row partition for N > 1: 'kway' (default) = the engine's own multilevel partitioner (pglamd_partition_edges, "
                         "balanced on in-degree + 1 and on rows), 'random' = balanced random, 'auto' = kway vs random, "
                         "keep the plan whose slowest rank receives fewer rows")
    ap.add_argument("--parallel", default="rows", choices=["rows"],
                    help="N > 1 layout: row partition by the engine's own partitioner (where north_star says METIS) + one RCCL halo "
                         "all-to-all-v per step overlapped with the local edges (DistGraph) -- north_star's layout, the only one in the product "
                         "(rounds 3-5 also carried a feature-column and a grid layout: removed in round 6)")
    ap.add_argument("--push", default="never", choices=["never", "auto"],
                    help="'never' (default) = halo source rows are pulled, every edge is aggregated by its destination's owner (what the "
                         "partitioner balanced); 'auto' = per rank pair the cheaper of pulling source rows and pushing pre-aggregated "
                         "destination rows (fewer bytes, but it moves edge work between ranks)")
    ap.add_argument("--row-order", default="peers", choices=["peers", "id"],
                    help="N > 1: how a rank orders its rows.  'peers' (default): rows pulled by the same set of peers lie together, so every "
                         "peer's rows are a few contiguous ranges of the feature matrix and the row-pipelined exchange (flow 'rows2') sends "
                         "them from where they are -- no pack launch, no send buffer; 'id': by node id (round 4's layout; the exchange packs)")
    ap.add_argument("--transport", default="auto", choices=["auto", "torch", "abi"],
                    help="N > 1 halo transport: 'torch' = torch.distributed all_to_all_single (RCCL), 'abi' = the library's own RCCL "
                         "communicator on its side stream (pglamd_halo_exchange_*, SURVEY 8b), 'auto' = time both, report both, run the "
                         "timed region on the faster")
    ap.add_argument("--phase-limit", type=float, default=float(os.environ.get("PGLAMD_BENCH_PHASE_LIMIT", "150")),
                    help="N > 1: seconds a phase (one candidate's trial, the timed region) may take before the run ends with the best "
                         "completed measurement; set-up phases (partition + plan, the target-size leg) get 4x")
    ap.add_argument("--target-scale", type=int, default=22, help="target_size leg: RMAT scale (north_star: 22)")
    ap.add_argument("--target-edges", type=int, default=100_000_000, help="target_size leg: edges (north_star: 100 M)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the event-timed distribution, the GCN-norm leg, the known-bytes roofline legs, the "
                         "target-size leg and the CPU baselines (N = 1); the exchange-only, per-rank-phase and bf16-wire diagnostics "
                         "and the target-size leg (N > 1).  Off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step returned as DIR/<name>.npy (float32 / float64, "
                         "<= 48 MB: a fixed seeded row sample of a larger output plus every row's sum)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="--full, N = 1: skip the no-reuse roofline legs and the |E| = 100 M target-size leg (profiling runs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "--gpus %d but WORLD_SIZE=%d" % (args.gpus, world)
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    # PGLAMD_BENCH_DRYRUN=1: every rank on cuda:0 with the gloo backend -- exercises the N > 1 code path end to end on a
    # single-GPU box (tests only; the numbers it prints mean nothing)
    dryrun = os.environ.get("PGLAMD_BENCH_DRYRUN") == "1"
    dev = torch.device("cuda", 0 if dryrun else local)
    torch.cuda.set_device(dev)

    import pgl_amd as pgl
    from pgl_amd.utils.rmat import rmat_edges

    N, E, d = 1 << args.scale, args.edges, args.dim
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        if dryrun:
            dist.init_process_group("gloo", timeout=datetime.timedelta(minutes=10))
        else:
            dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(minutes=10))

    edges = rmat_edges(args.scale, E, seed=42, device=dev)           # identical on every rank
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    x = torch.randn(N, d, generator=gen, device=dev, dtype=torch.float32)

    if world == 1:
        g = pgl.Graph(edges=edges, num_nodes=N)
        g.adj_dst_index                                            # CSR build = setup, not timed
        step = lambda: g.send_recv(x, "sum")
        sync = lambda: torch.cuda.synchronize()
        barrier = lambda: None
        halo = None
    else:
        import torch.distributed as dist
        import pgl_amd.distributed as pd
        from pgl_amd.distributed import DistGraph
        sync = lambda: torch.cuda.synchronize()
        barrier = lambda: dist.barrier()

        def timed(fn, n):
            sync(); barrier(); sync()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            sync()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        def agreed(ok):
            """True only if the step succeeded on EVERY rank (a rank that failed must not leave the others waiting in a collective)."""
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            return bool(int(flag.item()))

        def base_record(ms_step, how):
            """The contract fields of an N > 1 line for a measured ms/step."""
            return {"metric": "aggregated edges/sec (GCN send+recv_sum, d=%d)" % d, "value": E / (ms_step * 1e-3), "unit": "edges/s",
                    "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step, "higher_is_better": True,
                    "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "timed": how}

        wd = PhaseWatchdog(rank, lambda rec: print(json.dumps(rec), flush=True))
        note = wd.note
        lim = args.phase_limit
        n_trial = max(args.warmup, 3)
        trial, cands, built = {}, [], {}
        mode = "rows"
        extra = None

        if True:
            # ---- north_star's layout: row partition + one halo all-to-all-v per step ------------------------------------------------
            wd.begin("partition + halo plan", 4 * lim)
            dg = DistGraph.from_global(edges, N, rank, world, method=args.partition, device=dev, push=args.push, row_order=args.row_order)
            x_own = dg.take_owned(x)
            st0 = dg.stats()
            wd.end()
            step = lambda: dg.send_recv(x_own, "sum")
            # Candidates, most conservative first: one exchange and ONE aggregation launch after the wait ("fold") over
            # torch.distributed's all_to_all_single; then the flow the cost model picks (interior rows or local edges during the
            # exchange, possibly two column blocks in flight); then the same over the library's own RCCL communicator and side
            # stream (pglamd_halo_exchange_*).  Every trial runs under the phase limit; a candidate that raises is dropped on all
            # ranks; one that hangs ends the run with the best candidate measured before it.
            # ("pipeline" = round 4's flow: two column blocks, packed; "" = the cost model's choice, which with a peer-ordered plan is
            #  the zero-copy row-pipelined flow where pipelining pays: over torch.distributed point-to-point, then over the library's
            #  own communicator -- pglamd_halo_exchange_start_ranges)
            want = [("fold", "torch"), ("pipeline", "torch"), ("", "torch")] if args.transport in ("auto", "torch") else []
            if args.transport in ("auto", "abi"):
                want.append(("", "abi"))
            best = None
            for flow, transport in want:
                label = "%s/%s" % (flow or "cost-model", transport)
                wd.begin("trial %s" % label, lim)
                err, ms = None, None
                try:
                    pd.set_flow(flow, transport, graphs=[dg])
                    step(); step()
                except Exception as ex:                              # noqa: BLE001
                    err = ex
                if not agreed(err is None):
                    cands.append({"flow": flow or "cost-model", "transport": transport, "status": "failed", "error": repr(err)[:300]})
                    print("[bench] candidate %s failed (rank %d: %r)" % (label, rank, err), file=sys.stderr, flush=True)
                    wd.end()
                    continue
                # a candidate's trial IS a full measurement (W warm-up + K steps, barrier + synchronize on both sides, max over ranks:
                # tens of milliseconds): if a later phase hangs, the line left behind is a complete measurement of the best
                # candidate that finished, not a 3-step sample
                for _ in range(args.warmup):
                    step()
                ms = timed(step, args.steps) / args.steps * 1e3
                ran = dg.stats()["flow"]
                # what the cost model predicted for the flow that ran (slowest rank), next to what was measured: one multi-GPU run
                # shows how far the model's constants are from the machine (halo.calibration refits the two wire constants)
                pred = torch.tensor([dg.model_estimates(d).get(ran, float("nan"))], dtype=torch.float64, device=dev)
                dist.all_reduce(pred, op=dist.ReduceOp.MAX)
                cands.append({"flow": flow or "cost-model", "ran_flow": ran, "transport": transport, "status": "ok", "trial_ms_per_step": ms,
                              "model_predicted_ms": float(pred.item()), "trial_steps": args.steps, "packs": dg._idx.get(("ran_pack", "x"), "pack")})
                wd.end()
                note("candidate %-22s -> %.3f ms/step (flow that ran: %s)" % (label, ms, ran))
                if best is None or ms < best[0]:
                    best = (ms, flow, transport, ran)
                    wd.best = (lambda ms=ms, label=label, ran=ran: dict(
                        base_record(ms, "%d steps after %d warm-up steps of candidate %s, barrier + synchronize on both sides, max over ranks (a later "
                                        "phase did not finish)" % (args.steps, args.warmup, label)),
                        config={"workload": "RMAT scale %d |V|=%d |E|=%d d=%d fp32" % (args.scale, N, E, d), "parallelism":
                                "row partition (%s) x%d + halo all-to-all-v, flow %s" % (st0["partition"], world, ran)},
                        roofline={"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None},
                        halo=dict(st0, mode="rows", candidates=cands)))
            if best is None:
                raise RuntimeError("bench.py: no halo-exchange candidate ran on every rank: %r" % cands)
            pd.set_flow(best[1], best[2], graphs=[dg])
            step(); step()
            trial["rows"] = best[0]
            halo = dict(st0, mode="rows", candidates=cands, chosen={"flow": best[1] or "cost-model", "transport": best[2]},
                        flow=dg.stats()["flow"])                     # the flow that RAN: DESIGN section 5
            d_loc, n_loc, e_loc = d, st0["local_rows"], st0["local_edges"]
            extra = (dg, x_own)
        if args.full:
            # exchange alone (pack kernel + all-to-all-v + wait, no aggregation) and its bytes, per rank
            wd.begin("exchange only", lim)
            t_x = timed(lambda: dg.exchange_only(x_own), n_trial) / n_trial * 1e3
            allp = torch.zeros((world, 2), dtype=torch.float64, device=dev)
            allp[rank, 0], allp[rank, 1] = float(halo["recv_rows"]) * d * 4, float(halo["send_rows"]) * d * 4
            dist.all_reduce(allp)                                    # (a sum of one-hot rows = an all-gather every backend has)
            halo.update(exchange_only_ms=t_x, recv_bytes_per_rank=allp[:, 0].tolist(), send_bytes_per_rank=allp[:, 1].tolist(),
                        flow=dg.stats()["flow"])                     # the flow that RAN: DESIGN section 5
            wd.end()
            # per-rank compute phases (pack / work before the wait / work after it), each alone, no collective: the line can then be
            # read against the single-GPU per-rank measurements of scripts/prof.py rows (profiles/r04, r05 rows_c2p.txt) column by
            # column, and the cost model's constants (_LINK, _LAT, _RMW) calibrated from exchange_only_ms and these
            wd.begin("per-rank phases", lim)
            try:
                ph = dg.phase_times(x_own, iters=max(n_trial, 5))
                allq = torch.zeros((world, 3), dtype=torch.float64, device=dev)
                allq[rank, 0], allq[rank, 1], allq[rank, 2] = ph["pack_ms"], ph["before_ms"], ph["after_ms"]
                dist.all_reduce(allq)
                halo["phases_ms_per_rank"] = {"flow": ph["flow"], "pack": allq[:, 0].tolist(), "before_the_wait": allq[:, 1].tolist(),
                                              "after_the_wait": allq[:, 2].tolist(),
                                              "what": "each phase alone on its rank (HIP events, no collective); exchange_only_ms = pack + all-to-all-v + wait"}
            except Exception as ex:                                  # noqa: BLE001 -- a diagnostic: never lose the headline over it
                print("[bench] per-rank phases failed on rank %d: %r" % (rank, ex), file=sys.stderr, flush=True)
                dist.all_reduce(torch.zeros((world, 3), dtype=torch.float64, device=dev))
            wd.end()
            # secondary, NEVER the headline (north_star: fp32 parity to 1e-5): the same step with the halo rows travelling as bf16 -- half
            # the xGMI bytes, ~1e-3 relative error on the remote contributions.  Reported because the builder's own model says >= 6x at
            # 8 GPUs needs > 75 % link efficiency at fp32.
            wd.begin("secondary: bf16 wire", lim)
            try:
                dg.wire_dtype = torch.bfloat16
                step(); step()
                ms16 = timed(step, n_trial) / n_trial * 1e3
                halo["wire_bf16_secondary"] = {"ms_per_step": ms16, "value": E / (ms16 * 1e-3), "flow": dg.stats()["flow"],
                                               "note": "halo rows as bf16 (half the bytes; remote contributions rounded to 8 bits of mantissa): NOT the headline"}
            except Exception as ex:                                  # noqa: BLE001
                print("[bench] bf16-wire secondary failed on rank %d: %r" % (rank, ex), file=sys.stderr, flush=True)
            finally:
                dg.wire_dtype = None
                pd.set_flow(best[1], best[2], graphs=[dg])
                step(); step()
            wd.end()
        del x

    if world > 1:
        wd.begin("timed region: %d warm-up + %d steps" % (args.warmup, args.steps), 2 * lim)
    for _ in range(args.warmup):
        step()
    sync(); barrier(); sync()
    if not os.environ.get("PGLAMD_BENCH_NOPROF"):
        pgl.ops.profile_begin()
    t0 = time.perf_counter()
    for _ in range(args.steps - 1):
        step()
    out = step()                                                     # the last step's result is kept for --dump-outputs
    sync(); barrier(); sync()
    dt = time.perf_counter() - t0
    kern_ms, launches = pgl.ops.profile_end()

    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs:
        if world == 1:
            dump_outputs(args.dump_outputs, out, torch.arange(N))
        else:
            dump_outputs(args.dump_outputs, out, dg.plan.own_global, prefix="rank%d_" % rank, budget=DUMP_BYTES // world)
    del out

    # N > 1: north_star's target size (|E| = 100 M, SURVEY 8d C2') through the same partitioned flow -- every rank regenerates the
    # graph from the seed, rank 0 partitions it with the engine's partitioner (seconds), all ranks time the same steps.  The
    # headline above is complete at this point: if this leg raises or hangs, the line is printed without it.
    target_rec = None
    if world > 1:
        wd.end()
        wd.timed_done = True
        ms_done, flow_done = dt / args.steps * 1e3, (halo.get("flow") if isinstance(halo, dict) else None)
        wd.best = lambda: dict(base_record(ms_done, "%d steps after %d warm-up steps, barrier + synchronize on both sides, max over ranks"
                                           % (args.steps, args.warmup)),
                               config={"workload": "RMAT scale %d |V|=%d |E|=%d d=%d fp32" % (args.scale, N, E, d),
                                       "parallelism": "layout %s x%d, flow %s" % (mode, world, flow_done)},
                               roofline={"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None},
                               halo=halo)
    if world > 1 and mode == "rows" and args.full and not args.no_extra_legs:
        wd.begin("target size leg (|E| = %d)" % args.target_edges, 6 * lim)
        # the flow that won at the headline size need not be the one for 5x the edges: back to the cost model's own choice (on the
        # transport that won) -- unless that candidate failed above, in which case the forced one stays
        if any(k["flow"] == "cost-model" and k["status"] == "ok" and k["transport"] == halo["chosen"]["transport"] for k in cands):
            pd.set_flow("", None)
        err = None
        try:
            target_rec = target_size_leg_dist(pgl, dev, d, rank, world, args, timed, note)
        except Exception as ex:                                      # noqa: BLE001
            err = ex
            target_rec = {"error": repr(ex)[:400]}
            print("[bench] target-size leg failed on rank %d: %r" % (rank, ex), file=sys.stderr, flush=True)
        wd.end()
    if world > 1:
        wd.begin("report", lim)

    if rank == 0:
        ms_step = dt / args.steps * 1e3
        value = E * args.steps / dt
        B = algorithmic_bytes(E, N, d, 4) if world == 1 else algorithmic_bytes(e_loc, n_loc, d_loc, 4)
        kms = kern_ms / max(args.steps, 1)          # flat-kernel time per step (1 launch at N=1; interior + boundary launches at N>1)
        kname = pgl.ops.profile_last_kernel()
        rec = {
            "metric": "aggregated edges/sec (GCN send+recv_sum, d=%d)" % d, "value": value, "unit": "edges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,   # the N = 1..8 series runs the SAME global graph
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "RMAT(0.57,0.19,0.19,0.05) scale %d |V|=%d |E|=%d d=%d fp32, Graph.send_recv(sum) "
                                   "via pglamd_aggregate (BASELINE configs[1])" % (args.scale, N, E, d),
                       "graph_seed": 42, "feature_seed": 7,
                       "parallelism": "single GPU" if world == 1 else
                       ("row partition (%s) x%d + RCCL halo all-to-all-v (pull/push per pair: %d pairs push), interior rows "
                        "overlap the exchange, boundary rows read [owned | received]"
                        % (halo["partition"], world, halo.get("pushed_pairs", 0)))},
        }
        # roofline.  The section 8(d) byte model assumes NO cache reuse; on RMAT the hub rows are served from L2 / Infinity Cache, so
        # model bytes / kernel time is not a bandwidth and can exceed the peak.  roofline.achieved / frac are therefore
        # taken from the SAME kernel on a graph whose gathered bytes are known (uniform in-degree-19 graph over 8.6 GB of features:
        # <= 3.5 % of the gathers can hit any cache) -- a physical fraction.  The headline workload's own figures ride along under
        # roofline.headline_workload, labelled for what they are.
        tb, tsrc = recorded_traffic("scale%d_e%d_d%d_f32" % (args.scale, E, d), kname) if world == 1 else (None, None)
        head = {"kernel": kname, "kernel_ms": kms, "launches_per_step": launches / args.steps,
                "model_bytes_per_launch": B, "model_bytes_over_kernel_time_GBs": B / (kms * 1e-3) / 1e9 if kms > 0 else None,
                "model_note": "section 8(d) byte model (no reuse assumed) / kernel time; NOT a bandwidth on a graph with cache-resident hubs",
                "compulsory_bytes_per_launch": E * 4 + N * (2 * d * 4 + 8) if world == 1 else None,
                "traffic": tb, "traffic_source": tsrc,
                "traffic_frac_of_peak": (tb / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS) if (tb and kms > 0) else None,
                # how much of `traffic` (bytes that left the L2s) came from DRAM and how much from the 256 MiB
                # Infinity Cache?  No counter this rocprofv3 offers can say: all 688 are on the compute side of the fabric (SQ / TCP /
                # TCC ...; no UMC / MALL / DF block), and TCC_EA0_RDREQ_DRAM counts requests by DESTINATION class (DRAM vs GMI vs IO):
                # measured equal to TCC_EA0_RDREQ to the last digit on this kernel (profiles/r06/pmc_hub.txt).  So dram_bytes is
                # bounded, not measured: compulsory_bytes_per_launch <= dram_bytes <= traffic.
                "dram_bytes": None, "dram_bytes_bounds": [E * 4 + N * (2 * d * 4 + 8) if world == 1 else None, tb],
                "dram_bytes_note": "no memory-side counter exists on this platform (profiles/r06/pmc_hub.txt, counters_avail.txt): "
                                   "compulsory <= DRAM bytes <= L2-miss traffic; as fractions of 8 TB/s over the kernel time: %s"
                                   % (["%.3f" % ((E * 4 + N * (2 * d * 4 + 8)) / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS),
                                       "%.3f" % (tb / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS)] if (tb and kms > 0 and world == 1) else None)}
        rec["roofline"] = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None,
                           "kernel": kname, "headline_workload": head}
        if world == 1 and kms > 0:
            # SURVEY 8(d) to the letter on the headline workload: model bytes (no reuse assumed) / kernel time / peak.  NOT a physical
            # bandwidth fraction on RMAT (hub rows are cache-resident: it exceeds 1); printed, labelled, so nobody has to divide.
            rec["roofline"]["frac_model_8d"] = B / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS
            rec["roofline"]["frac_model_8d_note"] = ("section 8(d) byte model on the HEADLINE workload / kernel time / 8 TB/s -- non-physical when "
                                                     "> 1 (the model assumes no cache reuse; RMAT hubs are served by L2 / Infinity Cache). "
                                                     "`frac` is the physical one: the same kernel on a graph with known gathered bytes")
        if halo is not None:
            rec["halo"] = halo
        if world > 1:
            rec["timed"] = "%d steps after %d warm-up steps, barrier + synchronize on both sides, max over ranks" % (args.steps, args.warmup)
        if world > 1 and target_rec is not None:
            rec["target_size"] = target_rec
        if world > 1 and isinstance(halo, dict) and halo.get("exchange_only_ms"):
            # refit the cost model's wire constants from THIS run: the all-to-all-v alone = exchange_only - the pack phase, against the
            # largest pair block (what one xGMI link carries), at the headline size and at the target size
            from pgl_amd.distributed import DistGraph as _DG
            pts = []
            pk = max(halo.get("phases_ms_per_rank", {}).get("pack", [0.0]) or [0.0])
            pts.append((max(halo["recv_bytes_per_rank"]) / max(world - 1, 1), (halo["exchange_only_ms"] - pk) * 1e-3))
            if isinstance(target_rec, dict) and target_rec.get("exchange_only_ms"):
                pts.append((max(target_rec["recv_bytes_per_rank"]) / max(world - 1, 1), (target_rec["exchange_only_ms"] - target_rec.get("pack_ms", 0.0)) * 1e-3))
            halo["calibration"] = {"fit": _DG.calibrate_link(pts), "model_constants_used": {"link_GBs": _DG._LINK / 1e9, "lat_us": _DG._LAT * 1e6,
                                   "rate_Gedges_s": _DG._RATE / 1e9, "launch_us": _DG._LAUNCH * 1e6, "rmw_TBs": _DG._RMW / 1e12},
                                   "how": "t = (bytes of a rank's received rows / (N - 1) peers) / link + lat, from exchange_only_ms minus the pack phase at the two sizes"}
        if world == 1 and args.full:
            rec["timing"] = step_distribution(step)                  # median / p95 over 100 event-timed runs
            rec["gcn_norm"] = gcn_norm_leg(pgl, g, x, E)             # send_recv with both degree norms, fused and unfused
        edges_cpu = x_cpu = None
        if world == 1 and args.full and not args.no_extra_legs:
            edges_cpu, x_cpu = edges.cpu(), x.cpu()
            del g, x, edges
            torch.cuda.empty_cache()
            legs = no_reuse_legs(pgl, dev, d)
            u = legs["uniform_deg19"]
            ut, usrc = recorded_traffic("uniform_deg19_n16777216_d128_f32", u["kernel"])
            rec["roofline"].update({
                "achieved": u["achieved"], "frac": u["frac"], "kernel": u["kernel"], "kernel_ms": u["kernel_ms"],
                "bytes_per_launch": u["known_bytes"], "traffic": ut, "traffic_source": usrc,
                "what": "agg_flat_kernel (the headline kernel, d=128 fp32 sum) on the uniform in-degree-19 graph over 2^24 rows: known "
                        "gathered bytes (discounted by the largest possible cache-hit share) / HIP-event kernel time, measured in this run",
                "no_reuse": legs, "frac_permutation": legs["permutation"]["frac"],
                # the known-bytes leg runs in one of two modes from box to box (profiles/r04/noreuse_slab_allocations_slow_box.txt:
                # same binary, same counters, 29.7 vs 34.3 ms; it is the node slot, not the allocation): say which one this run saw
                # the HEADLINE launch against the ceiling that binds it: its L2-miss traffic per second over what the fabric + Infinity
                # Cache deliver to the same kernel gathering from a 128 MB table (no DRAM, no L2 hits) in this run
                "fabric_ceiling_GBs": legs["infinity_cache_table"]["achieved"],
                "slot": "fast" if u["kernel_ms"] < 32.0 else "slow",
                "slot_note": "known-bytes leg %.2f ms: < 32 ms = the fast node slot (frac ~0.71), otherwise the slow one (~0.61)" % u["kernel_ms"]})
            hw = rec["roofline"]["headline_workload"]
            ceil_gbs = legs["infinity_cache_table"]["achieved"]
            hw["fabric_ceiling_GBs"] = ceil_gbs
            hw["traffic_frac_of_fabric_ceiling"] = (hw["traffic"] / (hw["kernel_ms"] * 1e-3) / 1e9 / ceil_gbs) if (hw.get("traffic") and hw["kernel_ms"] > 0) else None
            hw["fabric_ceiling_note"] = ("bytes that leave the L2s per second, measured in this run with the same kernel on uniform sources over a "
                                         "128 MB table (inside the Infinity Cache, 32 x an L2): the RMAT launch is bound by this memory-side rate, "
                                         "not by DRAM (tables of 64 .. 512 MB run at the same rate: profiles/r06/tablesize.txt)")
            rec["target_size"] = target_size_leg(pgl, dev, d, args.target_scale, args.target_edges)
        elif world == 1:
            rec["roofline"]["what"] = ("%s: the known-bytes leg was skipped, so no physical fraction is reported in this run"
                                       % ("--no-extra-legs" if args.full else "without --full"))
        if world == 1 and args.full and not args.no_cpu_baseline:
            if edges_cpu is None:
                edges_cpu, x_cpu = edges.cpu(), x.cpu()
            rec["cpu_baseline"] = cpu_baseline(edges_cpu, x_cpu)
        print(json.dumps(rec), flush=True)

    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        wd.end()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
