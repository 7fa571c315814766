"""The public callables of pgl_amd.ops sorted by what they do to a stream that is being captured into a HIP graph.  Three explicit
name sets, held to the module by tests/test_replay_cases.py (no GPU): they partition the public callables, and every host read and
every floating-point atomic that is quoted here is still in the source where it is said to be.  A new op cannot land without
someone deciding which set it belongs to.

Plain Python, importable without a GPU (torch and pgl_amd are touched inside functions only).  Public: no leading underscore, not
host_*, not a class or constant.

The second half holds the side-stream cases and their harness (tests/test_side_stream_gpu.py runs them): an op queued behind
unfinished work on a non-default stream must give its eager result.  No graph is captured anywhere in this module.

What this table does NOT say: that a replayed result of a CAPTURABLE op equals its eager result.  The set is the list of ops a
replay test owes a case to (DESIGN.md 6d says which replays are tested)."""

# No host read on the default path: launches (and torch ops) on the current stream, caller-owned or freshly allocated buffers.
CAPTURABLE = frozenset([
    "csr_from_sorted", "exclusive_scan_i64", "narrow_i64", "edge_scale", "aggregate", "aggregate_dense", "winner_grad",
    "edge_operand_grad", "scatter_add_coo", "send_uv", "segment_reduce", "seg_ptr_from_ids", "segment_softmax", "gat_aggregate",
    "gat_backward", "sddmm", "add_score", "add_score_backward", "dot_attention", "dot_attention_backward", "gather_rows",
    "gather_rows_cast", "scatter_rows", "degree_norm", "sample_from_table", "stack_relations", "stack_weight_tables", "stack_indices",
    "stacked_segments", "stacked_mean_scale", "aggregate_relations", "row_epilogue", "row_epilogue_backward"])

# Reads back to the host by design: name -> (where the read is, text of the reading line, why).  `where` is a function of pgl_amd.ops
# (the test looks the text up in that function's source) or a source file under pgl_amd/.
NOT_CAPTURABLE = {
    "csr_build": ("csr_build", "int(flag.item())", "check_range=True reads the library's range flag"),
    "unique_segment": ("unique_segment", "int(cnt.item())", "the number of distinct keys sizes the result"),
    "hub_plan": ("hub_plan", "float(deg[ids].sum())", "first build per index reads the coverage; under capture it declines to build"),
    "hub_table": ("hub_plan", "float(deg[ids].sum())", "hub_plan with the call's shapes: first build reads the coverage"),
    "slice_plan": ("_build_slice_plan", ".tolist()", "first build per index reads the segment boundaries; under capture it declines to build"),
    "slice_table": ("_build_slice_plan", ".tolist()", "slice_plan with the call's shapes: first build reads the segment boundaries"),
    "send_u_recv": ("send_u_recv", "csr = csr_build(", "raw indices: builds an index with check_range=True (the atomic route of small inputs does not)"),
    "sample_neighbors": ("sample_neighbors", "total = int((offsets[-1] + count[-1]).item())", "the sample total sizes the result"),
    "edge_weight_table": ("_device_table", "int(flag.item())", "reads the weight flag (NaN / negative / infinite)"),
    "weight_table": ("_device_table", "int(flag.item())", "reads the weight flag (NaN / negative / infinite)"),
    "reindex_graph": ("_relabel", "int(num.item())", "the number of distinct ids sizes out_nodes"),
    "reindex_heter_graph": ("_relabel", "int(num.item())", "the number of distinct ids sizes out_nodes"),
    "induced_subgraph": ("induced_subgraph", "status.tolist()", "kept edges and the id-check flags, between count and fill"),
    "random_walk": ("random_walk", "int(flag.item())", "check_range=True reads the start-range flag"),
    "skip_gram_pairs": ("skip_gram_pairs", "total = int((offsets[-1] + count[-1]).item())", "the pair total sizes the result"),
    "sample_negatives": ("sample_negatives", "int(flags.item())", "check=True reads the range / empty flags"),
    "metapath_walk": ("metapath_walk", "int(flag.item())", "check_range=True reads the start-range flag"),
    "sample_neighbors_relations": ("_sample_relations", "split = tuple(bounds.tolist())", "edge_split, R + 1 numbers, sizes the result"),
    "stacked_max_segment": ("stacked_max_segment", "int(seg.max().item())", "first call per index reads the longest segment"),
    "stacked_long_rows": ("stacked_long_rows", ".nonzero()", "first build per (index, long_row): the compaction's length is read"),
    "walk_visit_topk": ("walk_visit_topk", "int(flag.item())", "check_range=True reads the seed-range flag"),
    "profile_end": ("csrc/aggregate.hip", "hipEventSynchronize(pr.second)", "waits for every bracketing event and reads its time"),
}

# Predicates, planners and switches: no launch, no allocation on the device.
NO_DEVICE_WORK = frozenset([
    "set_option", "release_workspaces", "tensor_version", "slice_blocks", "aggregate_dense_supported", "winner_grad_supported",
    "edge_operand_grad_supported", "profile_begin", "profile_last_kernel", "sddmm_supported", "dot_attention_supported",
    "induced_subgraph_launch_threads", "walk_params", "default_max_trials", "relation_seed", "row_epilogue_width_ok",
    "row_epilogue_supported"])

# CAPTURABLE ops that are NOT bit-reproducible from run to run, because their kernel adds floats with atomics: name -> (file under
# pgl_amd/, text of the line of the atomic).  A replay test may compare these with a bound only; every other one bit for bit.
FLOAT_ATOMICS = {
    "scatter_add_coo": ("csrc/edge_ops.hip", "unsafeAtomicAdd(out + (int64_t)t * d + j, x[(int64_t)s * d + j])"),
}


def public_callables(ops):
    import inspect
    return sorted(n for n, v in vars(ops).items()
                  if not n.startswith("_") and not n.startswith("host_") and inspect.isfunction(v) and v.__module__ == ops.__name__)


def partition_errors(public, capturable, not_capturable, no_device_work):
    """What keeps the three sets from being a partition of `public`: a list of sentences, empty when they are one."""
    sets = {"CAPTURABLE": set(capturable), "NOT_CAPTURABLE": set(not_capturable), "NO_DEVICE_WORK": set(no_device_work)}
    errors = []
    listed = set().union(*sets.values())
    for n in sorted(set(public) - listed):
        errors.append("%s is in none of CAPTURABLE, NOT_CAPTURABLE, NO_DEVICE_WORK: decide where it belongs" % n)
    for n in sorted(listed - set(public)):
        errors.append("%s is listed but is no public callable of pgl_amd.ops" % n)
    names = sorted(sets)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for n in sorted(sets[a] & sets[b]):
                errors.append("%s is listed twice: %s and %s" % (n, a, b))
    return errors


# CAPTURABLE ops that read the host on an index they have not seen: name -> the helper that reads and what the caller owes.
NEEDS_WARM_INDEX = {
    "aggregate_relations": ("stacked_long_rows", "one eager call per (StackedIndex, long_row) first: stacked_max_segment / stacked_long_rows read "
                                                 "the longest segment and the list length, and have no capture guard"),
}

# CAPTURABLE ops without a side-stream case below: the chunked aggregation family.  (A captured grouped fp32 aggregation, d = 20,
# on the hub graph ended in an illegal memory access, cause open -- DESIGN.md 6d; nothing of that family is driven from here.)
NO_SIDE_STREAM_CASE = frozenset([
    "aggregate", "aggregate_dense", "edge_scale", "winner_grad", "edge_operand_grad", "gat_aggregate", "gat_backward", "dot_attention",
    "dot_attention_backward", "aggregate_relations"])

# torch.cuda._sleep argument of the side-stream check: 41.7 ms on an MI355X (20 M: 8.3 ms, 10 M: 4.2 ms), against well under a
# millisecond of host time per op.
SIDE_STREAM_SLEEP_CYCLES = 100_000_000

# The host-reading ops that go through the side-stream check against their definitions (tests/test_side_stream_gpu.py).
SIDE_STREAM_HOST_READERS = ("csr_build", "sample_neighbors", "reindex_graph", "random_walk", "sample_negatives", "induced_subgraph")


# ---- side-stream cases: an op queued behind unfinished work on a non-default stream, no graph anywhere ---------------------------------
class Case(object):
    """name; ops: the public callables of pgl_amd.ops the case calls (the harness records the calls and holds the list to them);
    make(env, seed) -> dict of plain tensors (views are taken inside fn); fn(env, inp) -> tuple of tensors; check(env, inp, outs): the
    op's definition, applied once to the eager result, so that the chain ends at a reference and not at the code under test;
    bounded: the kernel adds floats with atomics, so both results are held to `check` instead of to each other."""

    def __init__(self, name, ops, make, fn, check=None, bounded=False):
        self.name, self.ops, self.make, self.fn, self.check, self.bounded = name, tuple(ops), make, fn, check, bounded

    def __repr__(self):
        return self.name


class Env(object):
    """The hub graph of gpu_common._hub_graph(3000, 50000, hub=6000) with both indices built, shared by the cases."""

    def __init__(self, pgl):
        import numpy as np
        import torch
        import gpu_common as C
        self.pgl, self.ops, self.torch, self.np, self.C = pgl, pgl.ops, torch, np, C
        self.n, self.E = 3000, 50000
        self.g, self.edges, _ = C._hub_graph(pgl, self.n, self.E, 5, hub=6000)
        self.src, self.dst = self.edges[:, 0].copy(), self.edges[:, 1].copy()
        self.csr, self.csr_t = self.g.adj_dst_index.csr, self.g.adj_src_index.csr
        self.src32, self.dst32 = self.g._edge_cols32()
        torch.cuda.synchronize()

    def gen(self, seed):
        return self.torch.Generator(device="cuda").manual_seed(int(seed))

    def randn(self, gen, *shape):
        return self.torch.randn(*shape, generator=gen, device="cuda", dtype=self.torch.float32)

    def randint(self, gen, lo, hi, *shape, dtype=None):
        return self.torch.randint(lo, hi, shape, generator=gen, device="cuda", dtype=dtype or self.torch.int64)

    def positive(self, gen, *shape):
        return self.torch.rand(*shape, generator=gen, device="cuda") + 0.5


def host(t):
    return t.detach().cpu().numpy()


def _equal(definition):
    def check(env, inp, outs):
        want = definition(env, inp)
        assert len(want) == len(outs)
        for i, (a, b) in enumerate(zip(outs, want)):
            assert a.dtype == b.dtype and env.torch.equal(a, b), "output %d differs from its definition" % i
    return check


def side_stream_cases():
    import torch
    cases = []
    add = cases.append
    i32 = torch.int32

    # segment ops: the ids are inputs too
    def seg_make(env, seed, rows=20000, segs=500, d=16):
        g = env.gen(seed)
        return {"x": env.randn(g, rows, d), "ids": env.randint(g, 0, segs, rows).sort().values}

    def seg_check(op):
        def check(env, inp, outs):
            ids = host(inp["ids"])
            env.C.check_aggregate(host(outs[0]), host(inp["x"]), env.np.arange(len(ids)), ids, op, 500, what="segment_%s vs fp64" % op)
        return check
    for op in ("sum", "mean", "max", "min"):
        add(Case("segment_reduce_" + op, ["segment_reduce"], seg_make,
                 lambda env, inp, op=op: (env.ops.segment_reduce(inp["x"], inp["ids"], op, 500),), check=seg_check(op)))

    # (forward only: the backward's segment sum goes through ops.aggregate, which is not driven from here)
    def softmax_check(ids_of):
        """p = exp(x - max) / sum: every term is positive, so a sum of n of them carries at most n eps of relative error (Higham 4.4);
        4 more roundings for the subtraction, exp and the division -> close_terms with the result as its own term and n + 4 terms."""
        def check(env, inp, outs):
            import grad_defs as G
            ids = ids_of(env, inp)
            m = int(ids.max()) + 1
            want = G.segment_softmax(inp["x"].double(), ids, m)
            n_terms = env.torch.bincount(ids, minlength=m)[ids].double().reshape(-1, 1) + 4.0
            env.C.close_terms(host(outs[0]), host(want), host(want), host(n_terms), what="segment_softmax vs fp64")
        return check
    add(Case("segment_softmax_sorted_ids", ["segment_softmax", "seg_ptr_from_ids", "narrow_i64"], lambda env, seed: seg_make(env, seed, d=4),
             lambda env, inp: (env.pgl.math.segment_softmax(inp["x"], inp["ids"], 500),), check=softmax_check(lambda env, inp: inp["ids"])))

    def softmax_unsorted(env, inp):
        from pgl_amd.nn import functional as GF
        return (GF.edge_softmax(env.g, inp["x"]),)
    add(Case("segment_softmax_unsorted_ids", ["segment_softmax"], lambda env, seed: {"x": env.randn(env.gen(seed), env.E, 4)}, softmax_unsorted,
             check=softmax_check(lambda env, inp: env.torch.as_tensor(env.dst).cuda())))

    # row moves, degree norm, send_uv
    def rows_make(env, seed):
        g = env.gen(seed)
        return {"x": env.randn(g, env.n, 24), "idx": env.randint(g, 0, env.n, 7001),
                "perm": env.torch.randperm(env.n, generator=g, device="cuda")[:2000], "out": env.randn(g, env.n, 24), "src": env.randn(g, 2000, 24)}
    add(Case("gather_rows", ["gather_rows"], rows_make, lambda env, inp: (env.ops.gather_rows(inp["x"], inp["idx"]),),
             check=_equal(lambda env, inp: (inp["x"][inp["idx"]],))))
    add(Case("gather_rows_cast_f16_column_block", ["gather_rows_cast"], rows_make,
             lambda env, inp: (env.ops.gather_rows_cast(inp["x"][:, 4:20], inp["idx"].to(env.torch.int32), env.torch.float16),),
             check=_equal(lambda env, inp: (inp["x"][:, 4:20][inp["idx"]].to(env.torch.float16),))))

    def scatter_def(env, inp):
        o = inp["out"].clone(); o[inp["perm"]] = inp["src"]
        return (o,)
    add(Case("scatter_rows", ["scatter_rows"], rows_make, lambda env, inp: (env.ops.scatter_rows(inp["out"], inp["perm"], inp["src"]),),
             check=_equal(scatter_def)))

    def coo_check(env, inp, outs):
        env.C.check_aggregate(host(outs[0]), host(inp["x"]), env.src, env.dst, "sum", what="scatter_add_coo vs fp64")
    add(Case("scatter_add_coo", ["scatter_add_coo"], lambda env, seed: {"x": env.randn(env.gen(seed), env.n, 16)},
             lambda env, inp: (env.ops.scatter_add_coo(inp["x"], env.src32, env.dst32, env.n),), check=coo_check, bounded=True))

    def degree_check(env, inp, outs):
        deg = host(inp["deg"]).astype(env.np.float64)
        env.C.close_rel(host(outs[0]), env.np.maximum(deg, 1.0).reshape(-1, 1) ** -0.5, env.C.RTOL, what="degree_norm")
    add(Case("degree_norm", ["degree_norm"], lambda env, seed: {"deg": env.randint(env.gen(seed), 0, 9000, env.n)},
             lambda env, inp: (env.ops.degree_norm(inp["deg"]),), check=degree_check))
    for mop in ("add", "sub", "mul", "div"):
        def make(env, seed):
            g = env.gen(seed)
            return {"x": env.randn(g, env.n, 8, 4), "y": env.positive(g, env.n, 8, 1)}

        def uv_check(env, inp, outs, mop=mop):
            import ref_ops as R
            want = R.np_send_uv(host(inp["x"]).astype(env.np.float64), host(inp["y"]).astype(env.np.float64), env.src, env.dst, mop)
            env.C.close_rel(host(outs[0]), want, env.C.RTOL, what="send_uv " + mop)
        add(Case("send_uv_" + mop, ["send_uv"], make,
                 lambda env, inp, mop=mop: (env.ops.send_uv(inp["x"], inp["y"], env.src32, env.dst32, mop),), check=uv_check))

    # the score ops at (H, D) = (4, 16)
    def hd(names, extra=None):
        def make(env, seed):
            g = env.gen(seed)
            inp = {k: env.randn(g, env.n, 4, 16) for k in names}
            if extra:
                inp.update(extra(env, g))
            return inp
        return make

    def sddmm_check(env, inp, outs):
        t = env.torch
        src, dst = t.as_tensor(env.src).cuda(), t.as_tensor(env.dst).cuda()
        prod = inp["x"].double()[src] * inp["y"].double()[dst]
        env.C.close_terms(host(outs[0]), host(prod.sum(-1)), host(prod.abs().sum(-1)), 17.0, what="sddmm vs fp64")
    add(Case("sddmm_4x16", ["sddmm"], hd(("x", "y")), lambda env, inp: (env.ops.sddmm(inp["x"], inp["y"], env.csr),), check=sddmm_check))

    def score_check(env, inp, outs):
        t = env.torch
        src, dst = t.as_tensor(env.src).cuda(), t.as_tensor(env.dst).cuda()
        terms = inp["w"].double() * t.nn.functional.leaky_relu(inp["x"].double()[src] + inp["y"].double()[dst], 0.2)
        env.C.close_terms(host(outs[0]), host(terms.sum(-1)), host(terms.abs().sum(-1)), 18.0, what="add_score vs fp64")
    add(Case("add_score_4x16", ["add_score"], hd(("x", "y"), extra=lambda env, g: {"w": env.randn(g, 4, 16)}),
             lambda env, inp: (env.ops.add_score(inp["x"], inp["y"], inp["w"], env.csr),), check=score_check))
    add(Case("add_score_backward_4x16_want_w", ["add_score_backward"],
             hd(("x", "y"), extra=lambda env, g: {"w": env.randn(g, 4, 16), "gs": env.randn(g, env.E, 4)}),
             lambda env, inp: env.ops.add_score_backward(inp["x"], inp["y"], inp["w"], inp["gs"], env.csr, env.n, want_w=True)))

    # the layer epilogue, both ways
    def epi_make(env, seed):
        g = env.gen(seed)
        return {"z": env.randn(g, env.n, 48), "b": env.randn(g, 48), "dy": env.randn(g, env.n, 48)}

    def epi_fn(env, inp):
        y, inv = env.ops.row_epilogue(inp["z"], inp["b"], "relu", True)
        dz, db = env.ops.row_epilogue_backward(inp["dy"], y, inv, "relu", True, want_bias=True)
        return (y, inv, dz, db)

    def epi_check(env, inp, outs):
        import grad_defs as G
        want = G.row_epilogue(inp["z"].double(), inp["b"].double(), "relu", True)
        env.C.close_rows(host(outs[0]), host(want), what="row_epilogue vs fp64")
    add(Case("row_epilogue_fwd_bwd_bias_relu_normalize", ["row_epilogue", "row_epilogue_backward"], epi_make, epi_fn, check=epi_check))

    # integer set-up ops that read nothing back
    add(Case("exclusive_scan_i64", ["exclusive_scan_i64"], lambda env, seed: {"c": env.randint(env.gen(seed), 0, 50, 70001)},
             lambda env, inp: (env.ops.exclusive_scan_i64(inp["c"]),),
             check=_equal(lambda env, inp: (env.torch.cumsum(inp["c"], 0) - inp["c"],))))
    add(Case("narrow_i64_strided", ["narrow_i64"], lambda env, seed: {"e": env.randint(env.gen(seed), 0, 1 << 30, 70001, 2)},
             lambda env, inp: (env.ops.narrow_i64(inp["e"][:, 1]),),
             check=_equal(lambda env, inp: (inp["e"][:, 1].to(env.torch.int32),))))

    def sorted_keys(env, seed):
        g = env.gen(seed)
        return {"u": env.randint(g, 0, 900, 40000).sort().values, "v": env.randint(g, 0, 900, 40000)}

    def from_sorted_fn(env, inp):
        c = env.ops.csr_from_sorted(inp["u"], inp["v"], 900)
        return (c.indptr, c.row32, c.col32, c.eid32, c.degree)

    def from_sorted_def(env, inp):
        t = env.torch
        deg = t.bincount(inp["u"], minlength=900)
        indptr = t.cat([deg.new_zeros(1), t.cumsum(deg, 0)])
        return (indptr, inp["u"].to(t.int32), inp["v"].to(t.int32), t.arange(40000, dtype=t.int32, device="cuda"), deg)
    add(Case("csr_from_sorted", ["csr_from_sorted", "seg_ptr_from_ids", "narrow_i64"], sorted_keys, from_sorted_fn, check=_equal(from_sorted_def)))
    add(Case("seg_ptr_from_ids_int32", ["seg_ptr_from_ids"], sorted_keys,
             lambda env, inp: (env.ops.seg_ptr_from_ids(inp["u"].to(env.torch.int32), 900),),
             check=_equal(lambda env, inp: (from_sorted_def(env, inp)[0],))))

    def table_check(env, inp, outs):
        import weighted_defs as W
        want = W.sample_from_table_restated(host(inp["cum"]), 4096, 9)
        assert env.np.array_equal(host(outs[0]), env.np.asarray(want, env.np.int64)), "sample_from_table vs its restatement"
    add(Case("sample_from_table", ["sample_from_table"],
             lambda env, seed: {"cum": env.torch.cumsum(env.randint(env.gen(seed), 1, 1000, 5000), 0)},
             lambda env, inp: (env.ops.sample_from_table(inp["cum"], 4096, seed=9),), check=table_check))

    # stacking the relations' indices: torch ops only, the index tensors are the inputs
    def stack_make(env, seed):
        g = env.gen(seed)
        inp = {}
        for r in range(3):
            u = env.randint(g, 0, 400, 3000 + 100 * r).sort().values
            deg = env.torch.bincount(u, minlength=400)
            inp["p%d" % r] = env.torch.cat([deg.new_zeros(1), env.torch.cumsum(deg, 0)])
            inp["c%d" % r] = env.randint(g, 0, 400, 3000 + 100 * r, dtype=i32)
            inp["e%d" % r] = env.randint(g, 0, 3000, 3000 + 100 * r, dtype=i32)
            inp["w%d" % r] = env.randint(g, 1, 99, 3000 + 100 * r)
            inp["n%d" % r] = deg.clone()
        return inp

    def stack_fn(env, inp):
        o = env.ops
        csrs = [o.CSR(inp["p%d" % r], None, inp["c%d" % r], inp["e%d" % r], 400, 3000 + 100 * r) for r in range(3)]
        si, sr = o.stack_indices(csrs), o.stack_relations(csrs)
        wt = o.stack_weight_tables([o.WeightTable(inp["w%d" % r], inp["n%d" % r]) for r in range(3)])
        return (si.indptr, si.col, si.eid, sr.indptr, sr.col, wt.cum, wt.npos, o.stacked_segments(si), o.stacked_mean_scale(si, 300))

    def stack_def(env, inp):
        t = env.torch
        base = [0, 3000, 6100]
        indptr = t.stack([inp["p%d" % r] + base[r] for r in range(3)])
        col, eid = t.cat([inp["c%d" % r] for r in range(3)]), t.cat([inp["e%d" % r] for r in range(3)])
        seg = indptr[:, 1:] - indptr[:, :-1]
        scale = t.where(seg[:, :300] > 0, 1.0 / seg[:, :300].clamp(min=1).float(), t.zeros((), device="cuda"))
        return (indptr, col, eid, indptr, col, t.cat([inp["w%d" % r] for r in range(3)]), t.cat([inp["n%d" % r] for r in range(3)]), seg, scale)
    add(Case("stack_relations_indices_tables", ["stack_indices", "stack_relations", "stack_weight_tables", "stacked_segments", "stacked_mean_scale"],
             stack_make, stack_fn, check=_equal(stack_def)))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


def case_names():
    return [c.name for c in side_stream_cases()]


class _Recorder(object):
    """pgl_amd.ops' public callables wrapped for the length of one fn call: which of them were called."""

    def __init__(self, ops):
        self.ops, self.called, self.keep = ops, set(), {}

    def __enter__(self):
        import functools
        for name in public_callables(self.ops):
            f = self.keep[name] = getattr(self.ops, name)

            def wrapped(*a, _f=f, _n=name, **kw):
                self.called.add(_n)
                return _f(*a, **kw)
            setattr(self.ops, name, functools.wraps(f)(wrapped))
        return self

    def __exit__(self, *exc):
        for name, f in self.keep.items():
            setattr(self.ops, name, f)


def run_side_stream_case(env, case, cycles=SIDE_STREAM_SLEEP_CYCLES):
    """Two input sets A and B of one shape.  Eager on B (default stream) is the reference, held once to the op's definition.  Then, on
    a non-default stream s: a delay, B copied into tensors that hold A, in place, and fn -- all queued on s -- and s still busy when fn
    returns.  A launch, copy or memset that went to another stream reads A and the comparison fails."""
    torch = env.torch
    A, B = case.make(env, 1), case.make(env, 2)
    clone = lambda inp: {k: v.clone() for k, v in inp.items()}
    with _Recorder(env.ops) as rec:
        want = tuple(t.clone() for t in case.fn(env, clone(B)))
    assert set(case.ops) <= rec.called, "%s lists %s but never called %s" % (case.name, case.ops, sorted(set(case.ops) - rec.called))
    torch.cuda.synchronize()
    if case.check is not None:
        case.check(env, B, want)
    static = clone(A)
    case.fn(env, clone(A))                                           # (whatever the op builds lazily exists before the side stream is used)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(cycles))
        for k, v in B.items():
            static[k].copy_(v)
        got = case.fn(env, static)
        busy = not s.query()
    s.synchronize()
    torch.cuda.synchronize()
    assert busy, "the side stream had drained before the op returned: the delay is too short to show anything"
    assert len(got) == len(want)
    if case.bounded:
        case.check(env, B, got)
        return
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), "output %d differs from the eager result on B" % i
