"""Every kernel held to its definition on misaligned and strided operands (DESIGN.md "Operand layout contract").

The cases are the tables of tests/layout_defs.py (tests/test_layout_defs.py proves on the CPU that they reach every branch).  Every case
runs the op on the offset or strided operands and on an aligned twin with the same values, checks that no byte outside a view was
written, and compares by one rule -- no new tolerance:
  * bit-identical to the aligned twin wherever the layout cannot re-associate a float addition: row moves, casts, send_uv, max and
    min, every integer dtype, the index arrays, and everything the front end copies to an aligned allocation first;
  * float sums and means: BOTH twins inside gpu_common.check_aggregate's per-element bound of the fp64 result (the grouped kernel's
    chunk length depends on the lane, so their bits may differ);
  * softmax, GAT, the additive score, the epilogue, the dense layer: inside the bound the existing test of that op uses.
Expected everywhere: the aligned twin's values, never an exception."""
import functools

import numpy as np
import pytest
import torch

import grad_defs as D
import layout_defs as L
import ref_ops as R
from gpu_common import pgl, dev, host, EPS, RTOL, close_rel, reassociation_bound, _assert_elementwise, _csr_fields  # noqa: F401  (pgl: the fixture)
from layout_defs import offset_view, column_block, guards_intact, assert_same_bits, alignment, stride_alignment

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
EPS32, EPS64 = EPS[np.dtype(np.float32)], EPS[np.dtype(np.float64)]
T = L.DTYPES


def _ids(cases):
    return [c.id for c in cases]


def _values(dtype, shape, seed, lo=-50, hi=50):
    """Deterministic values of any storage type on the device: standard normal floats, integers in [lo, hi)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.complex128:
        t = torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))
    elif dtype.is_floating_point:
        t = torch.randn(shape, generator=g, dtype=torch.float32 if dtype != torch.float64 else torch.float64).to(dtype)
    else:
        t = torch.randint(lo, hi, shape, generator=g).to(dtype)
    return t.to(DEVICE)


def _place(t, k):
    """t at k elements past an aligned address (k = 0 / None: a guarded ALIGNED view) -> (view, guard)."""
    return offset_view(t, int(k or 0))


# ================================================================================================
# A. aggregation forward
# ================================================================================================
@functools.lru_cache(maxsize=None)
def _agg_graph():
    g = L.AGG_GRAPH
    rng = np.random.default_rng(11)
    rows = rng.integers(0, L.AGG_ROWS_WITH_EDGES, g["e"]); rows[:g["long_edges"]] = g["long_row"]     # a row longer than any chunk; 20 rows without edges
    cols = rng.integers(0, g["n_src"], g["e"])
    import pgl_amd
    c = pgl_amd.ops.csr_build(dev(rows.astype(np.int64)), dev(cols.astype(np.int64)), g["n_rows"], want_i64=False)
    empty = torch.zeros(0, dtype=torch.int64, device=DEVICE)
    c0 = pgl_amd.ops.csr_build(empty, empty, g["n_rows"], want_i64=False)
    return rows.astype(np.int64), cols.astype(np.int64), c, c0


@functools.lru_cache(maxsize=None)
def _agg_data(dtype, d, generic=False):
    g = L.AGG_GRAPH
    x = _values(T[dtype], (g["n_src"], 1 if generic else d), 100 + d)
    y = (torch.rand((g["e"], d), generator=torch.Generator().manual_seed(200 + d)) + 0.5).to(T[dtype]).to(DEVICE) if T[dtype].is_floating_point else None
    return x, y


@functools.lru_cache(maxsize=None)
def _agg_definition(dtype, d, op, mop, generic=False):
    """-> ("exact", want tensor) for max / min / integers, ("bound", want64, bound) for float sums and means: computed once per shape."""
    rows, cols, _, _ = _agg_graph()
    x, y = _agg_data(dtype, d, generic)
    y = y if mop else None
    n = L.AGG_GRAPH["n_rows"]
    if not T[dtype].is_floating_point or (op in ("max", "min") and mop is None):
        xs = host(x.double()) if T[dtype] == torch.bfloat16 or T[dtype] == torch.float16 else host(x)
        want = R.np_send_u_recv(xs, cols, rows, op, n)
        return "exact", torch.as_tensor(want).to(T[dtype])
    want64, bound = L.aggregate_reference(x, cols, rows, op, y, mop or "add", n)
    return ("bound", want64, bound)


def _check_agg(got, definition, what):
    if definition[0] == "exact":
        assert_same_bits(got.cpu(), definition[1], what)
    else:
        L.assert_within(got, definition[1], definition[2], what)


def _kernel(pgl):
    """(family, element bytes, VEC or None) of the last profiled launch."""
    name = pgl.ops.profile_last_kernel()
    inner = name[name.index("<") + 1:name.rindex(">")].split(", ")
    if name.startswith("agg_flat_kernel"):
        return "flat", L.KERNEL_TYPE[inner[0]], int(inner[1])
    if name.startswith("agg_group_kernel"):
        return "grouped", int(inner[0].split("-")[0]), int(inner[1])
    assert name.startswith("agg_narrow_kernel"), name
    return "lane-per-edge", int(inner[0].split("-")[0]), None


def _run_agg(pgl, case, moved):
    """One launch of `case`; moved=False: the aligned twin (guarded views at aligned addresses, a dense copy of a column block).
    -> (result tensor, guards, kernel, the operand views in the launch's alignment term)."""
    ops = pgl.ops
    rows, cols, csr, csr0 = _agg_graph()
    g = L.AGG_GRAPH
    generic = case.layout == "generic"
    x, y = _agg_data(case.dtype, case.d, generic)
    y = y if case.mop else None
    off = case.offsets if moved else {}
    guards, term = [], []
    if case.layout == "block-x" and moved:
        xv, gd = column_block(x, *off["x"])
    else:
        xv, gd = _place(x, off.get("x"))
    guards.append(gd); term.append(xv)
    yv = None
    if y is not None:
        yv, gd = _place(y, off.get("y")); guards.append(gd)
        if not generic:
            term.append(yv)
    index = csr0 if case.layout == "empty" else csr
    changes = {}
    for name in ("row32", "col32", "eid32"):
        if off.get(name):
            v, gd = _place(getattr(csr, name), off[name]); guards.append(gd); changes[name] = v
            assert alignment(v) == 4
    if changes:
        index = index.view(**changes)
    # the destination: always handed in, so that what lies around it can be checked.  Rows without edges keep 7 under accumulate.
    init = torch.zeros((g["n_rows"], case.d), dtype=T[case.dtype], device=DEVICE)
    if case.accumulate:
        init[L.AGG_ROWS_WITH_EDGES:] = 7
    else:
        init.fill_(3)                                          # (every row is rewritten)
    if case.layout == "block-out" and moved:
        ov, gd = column_block(init, *off["out"])
    else:
        ov, gd = _place(init, off.get("out"))
    guards.append(gd); term.append(ov)
    ops.profile_begin()
    try:
        out = ops.aggregate(xv, index, case.op, g["n_rows"], y=yv, message_op=case.mop or "add", out=ov, accumulate=case.accumulate)
        torch.cuda.synchronize()
    finally:
        ops.profile_end()
    assert out.data_ptr() == ov.data_ptr()
    return ov, guards, (_kernel(pgl) if case.layout not in ("empty", "generic") else None), term


def _lane_contract(kernel, term, what):
    """THE CONTRACT: the lane of the launch, VEC * sizeof(T) bytes, divides the address of every operand of its alignment term and
    every row stride."""
    fam, esz, vec = kernel
    if vec is None:
        return
    lane = vec * esz
    for t in term:
        assert alignment(t) % lane == 0, "%s: a %d-byte lane on an operand aligned to %d bytes (%s)" % (what, lane, alignment(t), kernel)
        assert stride_alignment(t) % lane == 0, "%s: a %d-byte lane over a row stride of %d bytes (%s)" % (what, lane, t.stride(0) * t.element_size(), kernel)


@pytest.mark.parametrize("case", L.AGG_CASES, ids=_ids(L.AGG_CASES))
def test_aggregate(pgl, case):
    generic = case.layout == "generic"
    if case.layout == "empty":
        got, guards, _, _ = _run_agg(pgl, case, True)
        assert guards_intact(*guards), case.id
        assert_same_bits(got.cpu(), torch.zeros_like(got).cpu(), case.id)
        return
    definition = _agg_definition(case.dtype, case.d, case.op, case.mop, generic)
    twin, tguards, tkernel, tterm = _run_agg(pgl, case, False)
    assert guards_intact(*tguards), case.id + " (aligned twin)"
    got, guards, kernel, term = _run_agg(pgl, case, True)
    assert guards_intact(*guards), case.id + ": a byte outside the operands was written"
    edge_rows = slice(0, L.AGG_ROWS_WITH_EDGES)
    for name, res in (("aligned twin", twin), ("moved operands", got)):
        r = res.contiguous()
        if case.accumulate:
            assert bool((r[L.AGG_ROWS_WITH_EDGES:] == 7).all()), "%s %s: accumulate rewrote a row without edges" % (case.id, name)
            r = r.clone(); r[L.AGG_ROWS_WITH_EDGES:] = 0
        _check_agg(r, definition, "%s %s" % (case.id, name))
    if definition[0] == "exact":
        assert_same_bits(got.contiguous().cpu(), twin.contiguous().cpu(), case.id + " vs the aligned twin")
    if kernel is not None:
        print("%s: %s, the aligned twin %s" % (case.id, kernel, tkernel))
        _lane_contract(tkernel, tterm, case.id + " (aligned twin)")
        _lane_contract(kernel, term, case.id)
        assert kernel[1] == L.ESIZE[case.dtype]


@pytest.mark.parametrize("esz", [2, 4, 8])
def test_aggregate_reaches_all_three_families_and_moved_twins_take_a_narrower_lane(pgl, esz):
    """Per element size: the shapes of the table reach the lane-per-edge, the grouped and the flat kernel; and in the two families
    whose launch reports its lane, an aligned case with VEC > 1 has a moved twin that reports a strictly smaller VEC -- the narrower
    branch really ran.  (The flat kernel prefers 64 busy lanes to wide ones: only rows of 128 elements and more take VEC > 1 there.)"""
    seen, narrower = set(), set()
    mine = [c for c in L.AGG_CASES if L.ESIZE[c.dtype] == esz and c.layout == "offset" and not c.mop and c.op in ("sum", "mean") and not c.accumulate]
    for b in [c for c in mine if not c.offsets]:
        kb = _run_agg(pgl, b, False)[2]
        seen.add(kb[0])
        for c in mine:
            if (c.dtype, c.d, c.op) == (b.dtype, b.d, b.op) and c.offsets and set(c.offsets) <= {"x", "out"}:
                k = _run_agg(pgl, c, True)[2]
                print("%s: %s; %s: %s" % (b.id, kb, c.id, k))
                if kb[2] and kb[2] > 1 and k[0] == kb[0] and k[2] < kb[2]:
                    narrower.add(kb[0])
    assert seen == set(L.AGG_FAMILIES), (esz, seen)
    assert narrower >= {"grouped", "flat"}, (esz, narrower)


# ================================================================================================
# B. edge-wise kernels and row moves
# ================================================================================================
@functools.lru_cache(maxsize=None)
def _edge_graph(e=None):
    n = L.EDGE_GRAPH["n"]
    e = e or L.EDGE_GRAPH["e"]
    rng = np.random.default_rng(21)
    src, dst = rng.integers(0, n, e).astype(np.int32), rng.integers(0, n, e).astype(np.int32)
    return src, dst, dev(src), dev(dst)


def _send_uv_operands(case):
    n = L.EDGE_GRAPH["n"]
    dt = T[case.dtype]
    x = _values(dt, (n, case.dx), 31 + case.dx)
    if dt.is_floating_point:
        y = (torch.rand((n, case.dy), generator=torch.Generator().manual_seed(32 + case.dy), dtype=torch.float64) + 0.5).to(dt).to(DEVICE)
    else:
        y = _values(dt, (n, case.dy), 33 + case.dy, 1, 9) * (1 - 2 * (_values(dt, (n, case.dy), 34, 0, 2)))       # non-zero divisors of either sign
        if case.mop != "div":                                                                                  # sums and products that wrap
            big = 2 ** 30 if case.dtype == "int32" else 2 ** 62
            x = _values(dt, (n, case.dx), 35 + case.dx, -big, big)
            if case.mop != "mul":
                y = _values(dt, (n, case.dy), 36 + case.dy, -big, big)
    return x, y


def _send_uv(pgl, case, moved):
    ops = pgl.ops
    src, dst, src_d, dst_d = _edge_graph(case.e)
    x, y = _send_uv_operands(case)
    off = case.offsets if moved else {}
    (xv, gx), (yv, gy) = _place(x, off.get("x")), _place(y, off.get("y"))
    dout = max(case.dx, case.dy)
    if case.via == "ops":
        out, go = ops.send_uv(xv, yv, src_d, dst_d, case.mop), None
    else:                                                     # the C ABI directly: the only way to hand the kernel a destination of the caller's
        ov, go = _place(torch.zeros((case.e, dout), dtype=T[case.dtype], device=DEVICE), off.get("out"))
        with torch.cuda.device(x.device):
            rc = ops._ffi.lib().pglamd_send_uv(ops._ptr(xv), ops._ptr(yv), ops._code(x.dtype), case.dx, case.dy, dout, ops._ptr(src_d),
                                               ops._ptr(dst_d), case.e, ops.MSG[case.mop], ops._ptr(ov), ops._stream(x))
        assert rc == 0, ops._ffi.lib().pglamd_last_error()
        out = ov
    torch.cuda.synchronize()
    assert guards_intact(gx, gy, go), case.id
    return out.contiguous().cpu(), x, y, src, dst


@pytest.mark.parametrize("case", L.SEND_UV_CASES, ids=_ids(L.SEND_UV_CASES))
def test_send_uv(pgl, case):
    twin, x, y, src, dst = _send_uv(pgl, case, False)
    got = _send_uv(pgl, case, True)[0]
    assert_same_bits(got, twin, case.id + " vs the aligned twin")
    if T[case.dtype].is_floating_point:                       # one IEEE operation per element: the bound of the existing send_uv tests (fp64: two ulps)
        want = L.float_send_uv(host(x.double()), host(y.double()), src, dst, case.mop)
        close_rel(host(got), want.reshape(got.shape), RTOL if case.dtype == "fp32" else 2 * EPS64, case.id + " vs the fp64 definition")
    else:
        want = torch.as_tensor(L.int_send_uv(host(x), host(y), src, dst, case.mop))
        assert_same_bits(got, want.reshape(got.shape), case.id + " vs the definition")


@functools.lru_cache(maxsize=None)
def _softmax_segments():
    """sorted ids as test_gradients_gpu._segment_ids draws them -- one long segment, absent ids (every 7th and a run) -- over the edge
    graph's 4 099 rows and 1 200 segments; and a graph whose destinations are those ids in a shuffled edge order."""
    import pgl_amd
    rng = np.random.default_rng(15)
    n_rows, n_seg, long = L.EDGE_GRAPH["e"], L.EDGE_GRAPH["n"], 1500
    present = np.array([s for s in range(n_seg) if s % 7 != 3 and not 100 <= s < 120])
    ids = np.sort(np.concatenate([rng.choice(present, n_rows - long), np.full(long, 50)]))
    ids[-1] = n_seg - 1
    ids = ids.astype(np.int64)
    dst = ids[rng.permutation(n_rows)]
    src = rng.integers(0, n_seg, n_rows).astype(np.int64)
    g = pgl_amd.Graph(edges=np.stack([src, dst], 1), num_nodes=n_seg).tensor()
    return torch.as_tensor(ids, device=DEVICE), torch.as_tensor(dst, device=DEVICE), g


@functools.lru_cache(maxsize=None)
def _softmax_definition(dtype, d, kind):
    ids_sorted, dst, _ = _softmax_segments()
    ids = ids_sorted if kind == "segment" else dst
    n_rows = L.EDGE_GRAPH["e"]
    rng = np.random.default_rng(16 + d)
    x = rng.standard_normal((n_rows, d)) * 3
    x[n_rows // 3] += 80.0                                                # one row of large logits
    x = torch.as_tensor(x, device=DEVICE).to(T[dtype])
    want = D.segment_softmax(x.double(), ids, L.EDGE_GRAPH["n"])
    out_t, _, n_t = D.segment_softmax_terms(x, ids, L.EDGE_GRAPH["n"], torch.ones_like(x))
    bound = D.K_FAMILY["softmax"] * reassociation_bound(host(out_t), host(n_t), 4.0, EPS64 if dtype == "fp64" else EPS32)
    return x, host(want), bound


@pytest.mark.parametrize("case", L.SOFTMAX_CASES, ids=_ids(L.SOFTMAX_CASES))
def test_softmax(pgl, case):
    ids_sorted, dst, g = _softmax_segments()
    x, want, bound = _softmax_definition(case.dtype, case.d, case.kind)
    xv, guard = _place(x, case.offsets.get("data"))
    if case.kind == "segment":
        got = pgl.math.segment_softmax(xv, ids_sorted)
    else:
        got = pgl.nn.functional.edge_softmax(g, xv, "dst")
    got = got if isinstance(got, torch.Tensor) else got.materialize()
    torch.cuda.synchronize()
    assert guards_intact(guard), case.id
    assert tuple(got.shape) == tuple(x.shape) and got.dtype == x.dtype
    _assert_elementwise(np.abs(host(got.double()) - want), bound, want, case.id)


def _move_operands(case):
    dt = T[case.dtype]
    n_x, n_idx = 700, 1031
    idt = torch.int32 if case.index == "int32" else torch.int64
    g = torch.Generator().manual_seed(41)
    if case.op == "gather":
        x = _values(dt, (n_x, case.d), 42, 0, 250)
        index = torch.randint(0, n_x, (n_idx,), generator=g).to(idt).to(DEVICE)
        return x, index, None
    x = _values(dt, (n_x, case.d), 43, 0, 250)
    index = torch.randperm(n_idx, generator=g)[:n_x].to(idt).to(DEVICE)         # unique destinations
    return x, index, _values(dt, (n_idx, case.d), 44, 0, 250)


@pytest.mark.parametrize("case", L.MOVE_CASES, ids=_ids(L.MOVE_CASES))
def test_gather_and_scatter_rows(pgl, case):
    x, index, base = _move_operands(case)
    esz = x.element_size()
    off = case.offsets
    assert all(v % esz == 0 for k, v in off.items() if k != "index")
    xv, gx = _place(x, off.get("x", 0) // esz)
    iv, gi = _place(index, off.get("index"))
    if case.op == "gather":
        got = pgl.ops.gather_rows(xv, iv)
        want = x[index.long()]
        go = None
    else:
        ov, go = _place(base, off.get("out", 0) // esz)
        got = pgl.ops.scatter_rows(ov, iv, xv)
        want = base.clone(); want[index.long()] = x
    torch.cuda.synchronize()
    assert guards_intact(gx, gi, go), case.id
    assert_same_bits(got.contiguous().cpu(), want.cpu(), case.id)


@pytest.mark.parametrize("case", L.CAST_CASES, ids=_ids(L.CAST_CASES))
def test_gather_rows_cast(pgl, case):
    n_x, n_idx = 600, 1031
    x = _values(T[case.src], (n_x, case.d), 51)
    index = torch.randint(0, n_x, (n_idx,), generator=torch.Generator().manual_seed(52)).to(torch.int32).to(DEVICE) if case.index else None
    n_out = n_idx if case.index else n_x
    if case.layout == "block":
        xv, gx = column_block(x, *case.offsets["x"])
    else:
        xv, gx = _place(x, case.offsets.get("x"))
    ov, go = _place(torch.zeros((n_out, case.d), dtype=T[case.dst], device=DEVICE), case.offsets.get("out"))
    got = pgl.ops.gather_rows_cast(xv, index, T[case.dst], out=ov)
    fresh = pgl.ops.gather_rows_cast(xv, index, T[case.dst])
    torch.cuda.synchronize()
    assert guards_intact(gx, go), case.id
    want = (x if index is None else x[index.long()]).to(T[case.dst])             # torch's cast of the same rows
    assert_same_bits(got.cpu(), want.cpu(), case.id)
    assert_same_bits(fresh.cpu(), want.cpu(), case.id + " (a result the front end allocates)")


@pytest.mark.parametrize("case", L.SEG_REDUCE_CASES, ids=_ids(L.SEG_REDUCE_CASES))
def test_segment_reduce(pgl, case):
    ids_sorted, _, _ = _softmax_segments()
    n_rows, n_seg = L.EDGE_GRAPH["e"], L.EDGE_GRAPH["n"]
    exact = case.pool in ("max", "min")
    data = _values(torch.float32, (n_rows, case.d), 61 + case.d)
    ids = ids_sorted.to(torch.int32 if case.ids == "int32" else torch.int64)
    twin = pgl.ops.segment_reduce(data, ids, case.pool, n_seg)
    dv, gd = _place(data, case.offsets.get("data"))
    iv, gi = _place(ids, case.offsets.get("ids"))
    got = pgl.ops.segment_reduce(dv, iv, case.pool, n_seg)
    torch.cuda.synchronize()
    assert guards_intact(gd, gi), case.id
    rows = np.arange(n_rows)
    if exact:
        assert_same_bits(got.cpu(), twin.cpu(), case.id + " vs the aligned twin")
        assert_same_bits(got.cpu(), torch.as_tensor(R.np_send_u_recv(host(data), rows, host(ids_sorted), case.pool, n_seg)), case.id)
    else:
        want64, bound = L.aggregate_reference(data, rows, host(ids_sorted), case.pool, out_size=n_seg)
        L.assert_within(twin, want64, bound, case.id + " aligned twin")
        L.assert_within(got, want64, bound, case.id)


# ================================================================================================
# C. index construction
# ================================================================================================
def _csr_inputs(form, u, v):
    """u (the key column), v as ops.csr_build is handed them in `form` -> (u view, v view, guards)."""
    E = int(u.shape[0])
    if form == "separate":
        return u.clone(), v.clone(), []
    if form in ("pair", "pair-swapped", "pair-8-bytes-in"):
        k = 1 if form == "pair-8-bytes-in" else 0
        first, second = (v, u) if form == "pair-swapped" else (u, v)
        pairs, gd = _place(torch.stack([first, second], 1).contiguous(), k)
        assert alignment(pairs) == (8 if k else 256)
        uu, vv = (pairs[:, 1], pairs[:, 0]) if form == "pair-swapped" else (pairs[:, 0], pairs[:, 1])
        return uu, vv, [gd]
    if form == "of-three":
        m, gd = _place(torch.stack([u, v, torch.full_like(u, -1)], 1).contiguous(), 0)
        return m[:, 0], m[:, 1], [gd]
    (uu, g1), (vv, g2) = _place(u, 1), _place(v, 1)
    return uu, vv, [g1, g2]


@pytest.mark.parametrize("onesweep", [0, 2])
@pytest.mark.parametrize("E,N", L.CSR_SIZES)
def test_csr_build_input_forms(pgl, E, N, onesweep):
    gen = torch.Generator(device=DEVICE); gen.manual_seed(E + N)
    u = torch.randint(0, N, (E,), generator=gen, device=DEVICE)
    v = torch.randint(0, N, (E,), generator=gen, device=DEVICE)
    try:
        pgl.ops.set_option("csr_onesweep", onesweep)
        want = None
        for form, branch in L.CSR_FORMS.items():
            uu, vv, guards = _csr_inputs(form, u, v)
            if E > 1:
                assert L.csr_input_form(uu.stride(0), vv.stride(0), (vv.data_ptr() - uu.data_ptr()) // 8, alignment(uu), alignment(vv)) == branch, form
            got = pgl.ops.csr_build(uu, vv, N)
            torch.cuda.synchronize()
            assert guards_intact(*guards), form
            if want is None:
                want = got
                ref = R.np_build_index(host(u), host(v), N)
                assert np.array_equal(host(got.indptr), ref[4]) and np.array_equal(host(got.sorted_eid), ref[3])
            for (name, a), (_, b) in zip(_csr_fields(want), _csr_fields(got)):
                assert torch.equal(a, b), (form, name, E, N, onesweep)
    finally:
        pgl.ops.set_option("csr_onesweep", -1)


@pytest.mark.parametrize("case", L.BOUNDS_CASES, ids=_ids(L.BOUNDS_CASES))
def test_row_bounds_from_sorted_keys(pgl, case):
    keys, n_rows = L.gapped_keys(case.e, seed=case.e)
    want = L.seg_ptr_definition(keys, n_rows)
    kd = torch.as_tensor(keys, device=DEVICE).to(torch.int32 if case.ids == "int32" else torch.int64)
    kv, guard = _place(kd, case.k)
    if case.entry == "seg_ptr_from_ids":
        got = pgl.ops.seg_ptr_from_ids(kv, n_rows)
    else:
        c = pgl.ops.csr_from_sorted(kv, torch.zeros(case.e, dtype=torch.int64, device=DEVICE), n_rows)
        got = c.indptr
        assert torch.equal(c.row32.cpu(), torch.as_tensor(keys, dtype=torch.int32))
        assert torch.equal(c.degree.cpu(), want[1:] - want[:-1])
    torch.cuda.synchronize()
    assert guards_intact(guard), case.id
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), case.id


# ================================================================================================
# D. fused attention, epilogue, fused dense layer -- through the front end, forward and backward
# ================================================================================================
from test_gradients_gpu import assert_grads, _graphs, _t, rows as _rows, lattice, Q, _gat_terms      # noqa: E402  (the checks and data of the gradient tests)


@pytest.fixture(scope="module")
def classes(pgl):
    return _graphs(pgl)["classes"]


class _Copies(object):
    """Counts how often ops._aligned hands back a fresh allocation for a CONTIGUOUS operand (the monkeypatch-and-count idiom of
    test_aggregate_operands_at_a_misaligned_storage_offset)."""

    def __init__(self, pgl_, monkeypatch):
        self.n = 0
        real = pgl_.ops._aligned

        def counted(t, nbytes=16):
            r = real(t, nbytes)
            if t is not None and t.is_contiguous() and r.data_ptr() != t.data_ptr():
                self.n += 1
            return r
        monkeypatch.setattr(pgl_.ops, "_aligned", counted)

    def take(self):
        n, self.n = self.n, 0
        return n


def _run_twice(eng, inputs, cot):
    """forward and every gradient of eng on `inputs` (views keep their storage offset) -> [out, grads...] detached."""
    xs = [t.detach().requires_grad_(True) for t in inputs]
    out = eng(*xs)
    out = out if isinstance(out, torch.Tensor) else out.materialize()
    out.backward(cot)
    return [out.detach()] + [x.grad for x in xs]


def _att_case_data(G, op, H, D_):
    if op == "gat":
        rng = np.random.default_rng(29 + H)
        a_s, a_d = lattice(rng, True, G.n, H), lattice(rng, False, G.n, H)
        assert np.abs(a_s[G.src_np] + a_d[G.dst_np]).min() >= Q > 1e-4
        f, a_s, a_d, cot = _t(_rows(rng, G.n, H, D_)), _t(a_s), _t(a_d), _t(_rows(rng, G.n, H, D_))
        terms = _gat_terms(D.gat_terms(f, a_s, a_d, G.src, G.dst, cot), ("f", "a_s", "a_d"))
        return ([f, a_s, a_d], cot, lambda a, b, c: G.g.gat_aggregate(a, b, c, 0.2),
                dict(def_fn=lambda a, b, c, frozen=None: D.gat(a, b, c, G.src, G.dst, 0.2), terms=terms, family="gat"))
    if op == "sddmm":
        rng = np.random.default_rng(19 + H)
        x, y = _t(_rows(rng, G.n, H, D_)), _t(_rows(rng, G.n, H, D_))
        cot = _t(_rows(rng, G.e, H))
        return ([x, y], cot, lambda a, b: G.g.sddmm(a, b),
                dict(def_fn=lambda a, b, frozen=None: D.sddmm(a, b, G.src, G.dst), n_out=D_ + 1.0, n_terms=[G.outdeg + 2, G.indeg + 2]))
    from pgl_amd import autograd as ag
    rng = np.random.default_rng(23 + H)
    x, y = lattice(rng, True, G.n, H, D_), lattice(rng, False, G.n, H, D_)
    assert np.abs(x[G.src_np] + y[G.dst_np]).min() >= Q > 1e-4
    x, y, w = _t(x), _t(y), _t(_rows(rng, H, D_))
    cot = _t(_rows(rng, G.e, H))
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    return ([x, y, w], cot, lambda a, b, c: ag.add_score(a, b, c, cd, lambda: cs, 0.2),
            dict(def_fn=lambda a, b, c, frozen=None: D.add_score(a, b, c, G.src, G.dst, 0.2, frozen=frozen), n_out=D_ + 2.0,
                 n_terms=[G.outdeg + 2, G.indeg + 2, float(G.e) + 2], frozen_fn=lambda a, b, c: D.add_score_frozen(a, b, c, G.src, G.dst, 0.2),
                 family="add_score"))


@pytest.mark.parametrize("case", L.ATT_CASES, ids=_ids(L.ATT_CASES))
def test_attention_family(pgl, classes, monkeypatch, case):
    """Graph.gat_aggregate (default backward route), Graph.sddmm and autograd.add_score with ONE operand, or the cotangent, 4 or 8
    bytes into its storage: the aligned twin's bits, forward and every gradient, inside the bounds of test_gat_attention /
    test_sddmm / test_additive_score -- never an exception.  The copy falls on the moved operand alone: the aligned twin makes none."""
    G = classes
    inputs, cot, eng, kw = _att_case_data(G, case.op, case.H, case.D)
    names = L.ATT_OPERANDS[case.op]
    copies = _Copies(pgl, monkeypatch)
    twin = _run_twice(eng, inputs, cot)
    assert copies.take() == 0, "aligned operands were copied"
    guards = []
    moved, mcot = list(inputs), cot
    i = names.index(case.operand)
    if case.operand == "cotangent":
        mcot, gd = _place(cot, case.offset_bytes // 4)
    else:
        moved[i], gd = _place(inputs[i], case.offset_bytes // 4)
    guards.append(gd)
    got = _run_twice(eng, moved, mcot)
    n = copies.take()
    assert (n > 0) == (case.branch.split(":")[1].startswith(" a fresh copy")), (case.id, n, case.branch)
    torch.cuda.synchronize()
    assert guards_intact(*guards), case.id
    for k, (a, b) in enumerate(zip(got, twin)):
        assert_same_bits(a.cpu(), b.cpu(), "%s: %s vs the aligned twin" % (case.id, "forward" if k == 0 else "d " + names[k - 1]))
    assert_grads(eng, kw.pop("def_fn"), moved, mcot, what=case.id, **kw)


@pytest.mark.parametrize("case", L.EPI_CASES, ids=_ids(L.EPI_CASES))
def test_row_epilogue(pgl, monkeypatch, case):
    from pgl_amd import autograd as ag
    rng = np.random.default_rng(41 + case.d)
    n, d, act, nz = 300, case.d, case.act, case.normalize
    z, b = lattice(rng, True, n, d), lattice(rng, False, d)
    assert np.abs(z + b).min() >= Q > 1e-4
    z, b, cot = _t(z), _t(b), _t(_rows(rng, n, d))
    eng = lambda a, c: ag.row_epilogue(a, c, act, nz)
    copies = _Copies(pgl, monkeypatch)
    twin = _run_twice(eng, [z, b], cot)
    assert copies.take() == 0, "aligned operands were copied"
    k = case.offset_bytes // 4
    if case.operand == "y":                                   # the forward's own result: only a direct call can move it
        y, inv = pgl.ops.row_epilogue(z, b, act, nz)
        want = pgl.ops.row_epilogue_backward(cot, y, inv, act, nz, want_bias=True)
        yv, gd = _place(y, k)
        got = pgl.ops.row_epilogue_backward(cot, yv, inv, act, nz, want_bias=True)
        torch.cuda.synchronize()
        assert guards_intact(gd), case.id
        assert (copies.take() > 0) == case.branch.split(":")[1].startswith(" a fresh copy")
        for a, c, name in zip(got, want, ("dz", "dbias")):
            assert_same_bits(a.cpu(), c.cpu(), "%s %s vs the aligned twin" % (case.id, name))
        for a, c, name in zip(got, twin[1:], ("dz", "dbias")):
            assert_same_bits(a.cpu(), c.cpu(), "%s %s vs the autograd node" % (case.id, name))
        return
    moved, mcot = [z, b], cot
    if case.operand == "dy":
        mcot, gd = _place(cot, k)
    else:
        i = ("z", "bias").index(case.operand)
        moved[i], gd = _place(moved[i], k)
    got = _run_twice(eng, moved, mcot)
    torch.cuda.synchronize()
    assert guards_intact(gd), case.id
    assert (copies.take() > 0) == case.branch.split(":")[1].startswith(" a fresh copy"), (case.id, case.branch)
    for a, c, name in zip(got, twin, ("forward", "dz", "dbias")):
        assert_same_bits(a.cpu(), c.cpu(), "%s %s vs the aligned twin" % (case.id, name))
    res = D.row_epilogue_terms(z, b, act, nz, cot)
    assert_grads(eng, lambda a, c, frozen=None: D.row_epilogue(a, c, act, nz), moved, mcot,
                 terms={"out": res["out"], 0: res["z"], 1: res["bias"]}, family="row_epilogue", what=case.id)


@pytest.mark.parametrize("case", L.DENSE_CASES, ids=_ids(L.DENSE_CASES))
def test_aggregate_dense(pgl, classes, monkeypatch, case):
    G = classes
    d_in, d_out = case.d_in, case.d_out
    rng = np.random.default_rng(43 + d_in + d_out)
    x, w, b = _t(_rows(rng, G.n, d_in)), _t(rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)), _t(rng.standard_normal(d_out))
    cot = _t(_rows(rng, G.n, d_out))
    eng = lambda a, ww, bb: G.g.send_recv_dense(a, ww, bb, None, None, None, "sum")
    copies = _Copies(pgl, monkeypatch)
    twin = _run_twice(eng, [x, w, b], cot)
    assert copies.take() == 0, "aligned operands were copied"
    moved = [x, w, b]
    i = L.DENSE_OPERANDS.index(case.operand)
    moved[i], gd = _place(moved[i], case.offset_bytes // 4)
    got = _run_twice(eng, moved, cot)
    n = copies.take()
    torch.cuda.synchronize()
    assert guards_intact(gd), case.id
    # (the forward hands the library weight.t(), a copy of the layer's own; the backward multiplies by the weight as it is stored
    #  -- through the same entry point where its shape fits: d_out of 64 or 128)
    assert (n > 0) == (case.operand == "x" or (case.operand == "w" and d_out in (64, 128))), (case.id, n)
    for a, c, name in zip(got, twin, ("forward", "d x", "d w", "d bias")):
        assert_same_bits(a.cpu(), c.cpu(), "%s %s vs the aligned twin" % (case.id, name))
    n_out = G.indeg + d_in + 3
    n_terms = [G.outdeg + d_out + 3, float(G.n) + float(G.indeg.max()) + 3, float(G.n) + 1]
    assert_grads(eng, lambda a, ww, bb, frozen=None: D.aggregate_dense(a, ww, bb, G.src, G.dst, None, None, None, "sum", frozen=frozen),
                 moved, cot, n_out, n_terms, family="dense", what="dense " + case.id)
    if case.operand == "w":                                   # ops.aggregate_dense itself with a CONTIGUOUS [d_in, d_out] weight 4 bytes in
        wt = w.t().contiguous()
        copies.take()
        want = pgl.ops.aggregate_dense(x, G.g._csr_dst(), wt, b)[0]
        assert copies.take() == 0
        wv, gw = _place(wt, 1)
        out = pgl.ops.aggregate_dense(x, G.g._csr_dst(), wv, b)[0]
        torch.cuda.synchronize()
        assert copies.take() == 1 and guards_intact(gw)
        assert_same_bits(out.cpu(), want.cpu(), case.id + " ops.aggregate_dense vs the aligned twin")


# ------------------------------------------------------------------------------------------------
# the C entry points that document an alignment: an operand below it is refused with the documented code, nothing is written
# ------------------------------------------------------------------------------------------------
def _sentinel(*shape):
    return torch.full(shape, -123.25, dtype=torch.float32, device=DEVICE)


@pytest.mark.parametrize("entry", list(L.REFUSALS))
def test_c_entry_points_refuse_an_operand_below_their_alignment(pgl, classes, entry):
    ops = pgl.ops
    lib, P = ops._ffi.lib(), ops._ptr
    G = classes
    H, D_ = 8, 16
    cd, cs = G.g._csr_dst(), G.g._csr_src()
    n, E = G.n, G.e
    f = _values(torch.float32, (n, H, D_), 71)
    f4 = offset_view(f, 1).view                                # 4 bytes past a 16-byte boundary: below the 8-byte lane of 8 x 16
    a = _values(torch.float32, (n, H), 72)
    w = _values(torch.float32, (H, D_), 73)
    st = ops._stream(f)
    outs = []
    with torch.cuda.device(f.device):
        if entry == "gat_aggregate":
            ws = ops._scratch(ops._ws, "gat_aggregate", f, E, H, D_)
            outs = [_sentinel(n, H, D_)]
            rc = lib.pglamd_gat_aggregate(P(f4), P(a), P(a), H, D_, 0.2, 0.0, 0, P(cd.row32), P(cd.col32), P(cd.eid32), P(cd.indptr), E, n, n,
                                          P(outs[0]), None, None, None, None, P(ws), ws.numel(), st)
        elif entry == "gat_backward":
            ws = ops._scratch(ops._ws, "gat_backward", f, E, n, H, D_)
            outs = [_sentinel(n, H, D_), _sentinel(n, H), _sentinel(n, H)]
            rc = lib.pglamd_gat_backward(P(f), P(f4), P(a), P(a), P(a), P(a), P(f), H, D_, 0.2, 0.0, 0, P(cd.row32), P(cd.col32), P(cd.eid32),
                                         P(cd.indptr), P(cs.row32), P(cs.col32), P(cs.eid32), P(cs.indptr), E, n, P(outs[0]), P(outs[1]),
                                         P(outs[2]), None, None, None, P(ws), ws.numel(), st)
        elif entry == "sddmm":
            outs = [_sentinel(E, H)]
            rc = lib.pglamd_sddmm(P(f4), P(f), H, D_, P(cd.row32), P(cd.col32), P(cd.eid32), E, P(outs[0]), st)
        elif entry == "add_score":
            outs = [_sentinel(E, H)]
            rc = lib.pglamd_add_score(P(f), P(f), P(offset_view(w, 1).view), H, D_, 0.2, P(cd.row32), P(cd.col32), P(cd.eid32), E, P(outs[0]), st)
        elif entry == "add_score_backward":
            ws = ops._scratch(ops._ws, "gat_aggregate", f, E, H, D_)
            outs = [_sentinel(n, H, D_)]
            g = _values(torch.float32, (E, H), 74)
            rc = lib.pglamd_add_score_backward(P(f), P(f), P(offset_view(w, 2).view), P(g), H, D_, 0.2, P(cd.row32), P(cd.col32), P(cd.eid32),
                                               P(cd.indptr), E, n, P(outs[0]), None, P(ws), ws.numel(), st)      # w 8 bytes in: enough for the lane, below the 16 it asks
        elif entry == "aggregate_dense":
            x4 = offset_view(_values(torch.float32, (n, 64), 75), 1).view
            wt = _values(torch.float32, (64, 32), 76)
            ws = ops._scratch(ops._ws, "aggregate_dense", f, E, 64, 32)
            outs = [_sentinel(n, 32)]
            rc = lib.pglamd_aggregate_dense(P(x4), 64, P(cd.row32), P(cd.col32), P(cd.indptr), E, n, n, 0, None, None, P(wt), None, 0, 32, None,
                                            P(outs[0]), P(ws), ws.numel(), st)
        elif entry == "row_epilogue":
            z4 = offset_view(_values(torch.float32, (300, 64), 77), 1).view
            outs = [_sentinel(300, 64), _sentinel(300)]
            rc = lib.pglamd_row_epilogue(P(z4), None, 300, 64, 1, 1, 1e-12, P(outs[0]), P(outs[1]), st)
        else:
            dy2 = offset_view(_values(torch.float32, (300, 130), 78), 1).view          # d = 130: 8-byte lanes
            y = _values(torch.float32, (300, 130), 79)
            parts = int(lib.pglamd_row_epilogue_partials(300))
            outs = [_sentinel(300, 130), _sentinel(parts, 130)]
            rc = lib.pglamd_row_epilogue_backward(P(dy2), P(y), P(_values(torch.float32, (300,), 80)), 300, 130, 1, 1, P(outs[0]), P(outs[1]), st)
    torch.cuda.synchronize()
    operand, code = L.REFUSALS[entry]
    assert rc == L.CODES[code], (entry, operand, rc, lib.pglamd_last_error())
    for o in outs:
        assert bool((o == -123.25).all()), entry + ": a refused call wrote its result"
