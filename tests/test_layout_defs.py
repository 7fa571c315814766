"""tests/layout_defs.py held to what it claims, on the CPU: the builders produce each alignment class, the tables reach every branch
their headers list with every operand of a family's alignment term moved ALONE at least once, the restated selection rules agree with
the branch a row names, and the comparison helpers refuse the three ways a layout bug shows."""
import numpy as np
import pytest
import torch

import layout_defs as L
from special_defs import refuses

DTYPES = [torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.int32, torch.float64, torch.int64, torch.complex128]


def _values(dtype, *shape):
    g = torch.Generator().manual_seed(3)
    if dtype == torch.complex128:
        return torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g).to(dtype)
    return torch.randint(1, 100, shape, generator=g).to(dtype)


# ------------------------------------------------------------------------------------------------
# the builders
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_offset_view_produces_each_alignment_class(dtype):
    t = _values(dtype, 7, 5)
    esz = t.element_size()
    for k in (0, 1, 2, 3, 4, 6, 8, 16, 64):
        v, guard = L.offset_view(t, k)
        assert v.is_contiguous() and v.dtype == dtype and tuple(v.shape) == (7, 5)
        L.assert_same_bits(v, t, "values")
        want = 256 if (k * esz) % 256 == 0 else (k * esz) & -(k * esz)
        assert L.alignment(v) == want and v.data_ptr() % want == 0 and (want == 256 or v.data_ptr() % (2 * want) != 0)
        assert guard.buf.data_ptr() % 256 == 0
        lo = v.data_ptr() - guard.buf.data_ptr()
        assert lo >= 64 and guard.buf.numel() - (lo + t.numel() * esz) >= 64              # at least 64 guard bytes on either side
        assert guard.intact() and L.guards_intact(guard, None)


def test_misaligned_is_the_view_the_gradient_tests_used():
    for dtype in (torch.float32, torch.float64, torch.float16):
        t = _values(dtype, 6, 4)
        v = L.misaligned(t)
        assert v.is_contiguous() and torch.equal(v, t) and v.data_ptr() % 16 == t.element_size() % 16 != 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.int64], ids=["fp16", "fp32", "int64"])
def test_column_blocks_produce_the_address_and_the_stride_class(dtype):
    t = _values(dtype, 9, 8)
    esz = t.element_size()
    for a, width in ((3, 23), (5, 25), (4, 20), (0, 24), (1, 18)):
        v, guard = L.column_block(t, a, width)
        assert not v.is_contiguous() and v.stride(0) == width and v.stride(1) == 1
        L.assert_same_bits(v.contiguous(), t, "values")
        assert L.alignment(v) == L.pow2_class(a * esz)
        assert L.stride_alignment(v) == L.pow2_class(width * esz) and (width * esz) % L.stride_alignment(v) == 0
        assert guard.intact()
    v, _ = L.column_block(t, 3, 23)
    assert L.stride_alignment(v) == esz                          # an odd parent width: no lane wider than an element keeps its alignment from row to row


def test_guards_detect_a_write_on_either_side_and_between_the_columns():
    t = _values(torch.float32, 6, 4)
    for where in ("before", "after"):
        v, guard = L.offset_view(t, 3)
        flat = guard.buf
        lo = v.data_ptr() - flat.data_ptr()
        flat[lo - 1 if where == "before" else lo + t.numel() * 4] = 0
        assert not guard.intact() and not L.guards_intact(None, guard)
    v, guard = L.column_block(t, 3, 11)
    parent = guard.buf[L.GUARD:L.GUARD + 6 * 11 * 4].view(torch.float32).view(6, 11)
    parent[2, 7] = 1.0                                           # the first column after the block
    assert not guard.intact()
    v, guard = L.column_block(t, 3, 11)
    v.mul_(2.0)                                                   # writing the block itself is what the block is for
    assert guard.intact()


# ------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(L.TABLES))
def test_every_table_reaches_every_branch_and_moves_every_operand_alone(family):
    cases, branches, operands = L.TABLES[family]
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)), "case ids must be unique"
    reached = {c.branch for c in cases}
    assert set(branches) <= reached, ("no case left for", sorted(set(branches) - reached))
    assert reached <= set(branches), ("a branch the header does not list", sorted(reached - set(branches)))
    for c in cases:
        assert ":" in c.branch.split(" ")[0] or c.branch.startswith("ops.py"), c.branch        # file:line of the branch
    for operand in operands:
        assert L.offset_alone(cases, operand), "%s: no case moves %s alone" % (family, operand)


def test_a_table_that_loses_a_branch_is_noticed():
    cases, branches, operands = L.TABLES["softmax"]
    cut = [c for c in cases if c.branch != L.SOFTMAX_THREE_PASS % 1]
    assert not set(branches) <= {c.branch for c in cut}
    assert not L.offset_alone([c for c in L.SEND_UV_CASES if set(c.offsets) != {"y"}], "y")


def test_aggregate_table_covers_the_issue_s_shapes():
    seen = {(c.dtype, c.d) for c in L.AGG_CASES if c.layout == "offset"}
    for dtype, fams in L.AGG_WIDTHS.items():
        for widths in fams:
            for d in widths:
                assert (dtype, d) in seen
    for dtype, fams in L.AGG_WIDTHS.items():
        esz = L.ESIZE[dtype]
        for fam, widths in zip(L.AGG_FAMILIES, fams):
            mine = [c for c in L.AGG_CASES if c.dtype == dtype and c.family == fam]
            assert {"sum", "mean", "max", "min"} <= {c.op for c in mine} or dtype.startswith("int") and {"sum", "max", "min"} <= {c.op for c in mine}
            for k in L.AGG_OFFSETS[esz]:
                assert any(c.offsets == {"x": k} for c in mine) and any(c.offsets == {"out": k} and c.accumulate == a for c in mine for a in (0, 1))
                assert any(c.offsets == {"out": k} and c.accumulate == 1 for c in mine)
            assert any(c.layout == "block-x" for c in mine) and any(c.layout == "block-out" for c in mine)
            assert any("row32" in c.offsets for c in mine)
            if not dtype.startswith("int"):
                assert any(c.offsets == {"y": L.AGG_OFFSETS[esz][0]} for c in mine) and any("eid32" in c.offsets for c in mine)
            for c in mine:
                if c.layout.startswith("block"):
                    (a, w), = c.offsets.values()
                    assert a % 2 == 1 and w % 2 == 1                # an odd first column of an odd-width parent
            # an aligned case with VEC > 1 whose twin can only take a strictly smaller lane
            if fam != "lane-per-edge":
                wide = [c for c in mine if c.layout == "offset" and not c.offsets and not c.mop and c.branch != L.AGG_VMAX % 1]
                assert any(any(t.d == c.d and t.layout == "offset" and t.offsets and not t.mop and int(t.branch.rsplit("=", 1)[1]) < int(c.branch.rsplit("=", 1)[1])
                               for t in mine) for c in wide), (dtype, fam)
        words = {c.branch for c in L.AGG_CASES if c.dtype == dtype and c.layout == "empty"}
        assert len(words) >= 2 and L.AGG_ZERO % 16 in words


def test_restated_rules_agree_with_the_rows():
    for c in L.SEND_UV_CASES:
        if c.branch != L.SEND_UV_SECOND_TRIP:
            al = 0
            for v in c.offsets.values():
                al |= v * L.ESIZE[c.dtype]
            assert c.branch == L.send_uv_branch(L.ESIZE[c.dtype], c.dx, c.dy, max(c.dx, c.dy), al or 256), c.id
        else:
            assert c.e * max(c.dx, c.dy) > L.SEND_UV_GRID and c.dx == 1                       # just above one trip of the grid
    assert sum(c.e > 70001 for c in L.SEND_UV_CASES) == 1
    # softmax: {18, 20, 33, 100} take the three-pass form with VEC 2, 4, 1, 4 in fp32
    assert [L.softmax_branch(4, d, 256) for d in (18, 20, 33, 100)] == [L.SOFTMAX_THREE_PASS % v for v in (2, 4, 1, 4)]
    assert all(L.softmax_branch(4, d, 256).startswith(L.SOFTMAX_ONE_PASS[:30]) for d in (1, 2, 6, 8, 16))
    # row moves: every offset of a row knocks the word down exactly one class from the previous one
    for rb in L.MOVE_ROW_BYTES:
        for dtype in L.MOVE_ELEMS:
            words = sorted({int(c.branch.split(" ")[3]) for c in L.MOVE_CASES if c.dtype == dtype and c.d * L.MOVE_ELEMS[dtype] == rb
                            and "index" not in c.offsets}, reverse=True)
            assert all(a == 2 * b for a, b in zip(words, words[1:])), (rb, dtype, words)
    assert {(c.src, c.dst) for c in L.CAST_CASES} == set(L.CAST_PAIRS) and len(L.CAST_PAIRS) == 7
    assert {c.d % 4 == 0 for c in L.CAST_CASES} == {True, False} and {c.index for c in L.CAST_CASES} == {True, False}
    assert L.csr_input_form(2, 2, 1, 16, 8) == L.CSR_PAIR1 and L.csr_input_form(2, 2, -1, 8, 16) == L.CSR_PAIR2
    assert L.csr_input_form(2, 2, 1, 8, 16) == L.CSR_STRIDED and L.csr_input_form(1, 1, 4095, 256, 256) == L.CSR_STRIDED
    assert L.csr_input_form(3, 3, 1, 256, 8) == L.CSR_STRIDED
    assert set(L.CSR_FORMS.values()) == set(L.CSR_BRANCHES)
    assert [L.gat_lane_bytes(H, D, True) for H, D in L.ATT_HD] == [4, 8, 16]              # one, two and four columns per lane
    assert [L.epilogue_lane_bytes(d) for d in L.EPILOGUE_D] == [4, 16, 8, 16, 16]
    # the defects the issue names, each as a named case that needs the front end's copy
    named = {c.id: c for c in L.ATT_CASES}
    for cid in ("gat-8x16-feature-4", "sddmm-8x16-x-4", "add_score-8x16-x-4"):
        assert named[cid].branch == L.ATT_COPY % 8, cid
    assert named["add_score-8x16-w-4"].branch == named["add_score-4x8-w-8"].branch == L.ATT_COPY % 16
    assert {c.id for c in L.DENSE_CASES} >= {"64-32-x-4", "128-128-x-4"}
    assert set(L.REFUSALS) == {"gat_aggregate", "gat_backward", "sddmm", "add_score", "add_score_backward", "aggregate_dense", "row_epilogue",
                               "row_epilogue_backward"}


def test_gapped_keys_have_every_gap_and_a_tail():
    for e in L.BOUNDS_E:
        keys, n_rows = L.gapped_keys(e, seed=e)
        assert keys.shape == (e,) and (np.diff(keys) >= 0).all() and n_rows - int(keys[-1]) > 16
        if e >= 255:
            assert {0, 1, 2, 16, 17, 18} <= set(np.diff(keys).tolist())
        ptr = L.seg_ptr_definition(keys, n_rows).numpy()
        assert ptr[0] == 0 and ptr[-1] == e and np.array_equal(np.diff(ptr), np.bincount(keys, minlength=n_rows))


# ------------------------------------------------------------------------------------------------
# the definitions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_integer_send_uv_wraps_and_truncates(dtype):
    info = np.iinfo(dtype)
    x = np.array([[info.max, -7, 7, info.min]], dtype)
    y = np.array([[1, 2, -2, -1]], dtype)
    z = np.zeros(1, np.int64)
    assert L.int_send_uv(x, y, z, z, "add").tolist() == [[info.min, -5, 5, info.max]]
    assert L.int_send_uv(x, y, z, z, "sub").tolist() == [[info.max - 1, -9, 9, info.min + 1]]
    assert L.int_send_uv(x, np.array([[2, 2, 2, 2]], dtype), z, z, "mul").tolist() == [[-2, -14, 14, 0]]
    assert L.int_send_uv(np.array([[-7, 7, -7, 7]], dtype), np.array([[2, -2, -2, 2]], dtype), z, z, "div").tolist() == [[-3, -3, 3, 3]]   # C: toward zero
    assert L.int_send_uv(np.array([[5], [6]], dtype), np.array([[1, 2, 3]], dtype), np.array([1]), z, "mul").tolist() == [[6, 12, 18]]


def test_aggregate_reference_is_check_aggregate_s_bound():
    import gpu_common as C
    rng = np.random.default_rng(0)
    n, e, d = 40, 600, 6
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    for dtype, op in ((torch.float32, "sum"), (torch.float32, "mean"), (torch.float64, "sum"), (torch.float16, "mean")):
        x = torch.as_tensor(rng.standard_normal((n, d))).to(dtype)
        want64, bound = L.aggregate_reference(x, src, dst, op)
        storage = {torch.float16: "fp16"}.get(dtype)
        xn = x.numpy()                                            # (fp16 features as numpy float16: check_aggregate then takes the fp32 epsilon)
        inside = torch.as_tensor(want64 + 0.9 * bound)
        outside = torch.as_tensor(want64 + 1.2 * bound)
        L.assert_within(inside, want64, bound)
        C.check_aggregate(inside.numpy(), xn, src, dst, op, storage=storage)
        assert refuses(L.assert_within, outside, want64, bound)
        assert refuses(C.check_aggregate, outside.numpy(), xn, src, dst, op, storage=storage)


# ------------------------------------------------------------------------------------------------
# the three ways a layout bug shows, as doctored results of the reference
# ------------------------------------------------------------------------------------------------
def _reference_case():
    rng = np.random.default_rng(1)
    n, e, d = 50, 900, 12
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    x = torch.as_tensor(rng.standard_normal((n, d)), dtype=torch.float32)
    want64, bound = L.aggregate_reference(x, src, dst, "sum")
    return x, torch.as_tensor(want64, dtype=torch.float32), want64, bound


def test_a_stale_last_element_per_row_is_refused():
    """A vector lane cut short: the last element of every row keeps what the buffer held before."""
    x, ref, want64, bound = _reference_case()
    L.assert_same_bits(ref.clone(), ref)
    L.assert_within(ref, want64, bound)
    stale = ref.clone()
    stale[:, -1] = torch.full((1,), L.SENTINEL * 0x01010101, dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert refuses(L.assert_same_bits, stale, ref) and refuses(L.assert_within, stale, want64, bound)
    one = ref.clone()
    one[17, -1] = 0.0                                             # and in a single row
    assert refuses(L.assert_same_bits, one, ref) and refuses(L.assert_within, one, want64, bound)


def test_a_result_shifted_by_the_offset_is_refused():
    """The offset ignored: the kernel wrote (or read) from the buffer's aligned base, so the view holds the result k elements late."""
    x, ref, want64, bound = _reference_case()
    for k in (1, 2, 3):
        shifted = torch.roll(ref.reshape(-1), k).reshape(ref.shape)
        assert refuses(L.assert_same_bits, shifted, ref) and refuses(L.assert_within, shifted, want64, bound)
    moved = L.aggregate_reference(torch.roll(x.reshape(-1), 1).reshape(x.shape), *(np.random.default_rng(1).integers(0, 50, 900) for _ in range(2)), "sum")[0]
    assert refuses(L.assert_within, torch.as_tensor(moved), want64, bound)              # the INPUT read one element early


def test_an_element_written_outside_the_view_is_refused():
    """An over-wide store: the values inside are right, one element next to them is not the sentinel any more."""
    x, ref, want64, bound = _reference_case()
    v, guard = L.offset_view(torch.zeros_like(ref), 1)
    v.copy_(ref)
    L.assert_same_bits(v, ref)
    assert L.guards_intact(guard)
    end = v.data_ptr() - guard.buf.data_ptr() + ref.numel() * 4
    guard.buf[end:end + 4] = 0                                   # one float past the end
    L.assert_same_bits(v, ref)                                    # the values alone do not show it
    assert not L.guards_intact(guard)
    v, guard = L.column_block(torch.zeros_like(ref), 3, 29)
    v.copy_(ref)
    m = guard.buf[L.GUARD:L.GUARD + 50 * 29 * 4].view(torch.float32).view(50, 29)
    m[49, 15] = 0.0                                               # the column after the block, last row
    L.assert_same_bits(v.contiguous(), ref)
    assert not L.guards_intact(guard)
