"""Operand layout (DESIGN.md "Operand layout contract"): where an operand lies in memory is an INPUT of almost every launch.

Almost every entry point of the library picks its lane width, word width or load form from the ADDRESSES and ROW STRIDES of its
operands, not only from d and the dtype.  A fresh torch allocation is 256-byte aligned, so a suite that only ever allocates never
runs the narrower branches, nor the refusals.  This module builds the operands that do (pure torch / numpy, no GPU needed), names in
one table per kernel family the cases the GPU tests run and the branch each one is there to reach, restates the selection rules the
tables rely on, and holds the definitions and comparison helpers the cases share.  tests/test_layout_defs.py proves on the CPU that
the builders produce the alignment classes they claim, that every table reaches every branch its header lists, and that the
helpers refuse the three ways a layout bug shows (a stale last element per row, a result shifted by the offset, an element written
outside the view).  tests/test_operand_layout_gpu.py runs the tables on the MI355X.

Branch names are "file:line what" with the line of the branch in pgl_amd/csrc at the time of writing."""
import collections

import numpy as np
import torch

from special_defs import assert_bits_equal

SENTINEL = 0xA5                  # every guard byte; as fp32 0xA5A5A5A5 = -2.87e-16, as fp16 -0.0220: a number, never a NaN
GUARD = 256                      # bytes of guard in front of a view (>= 64, and a multiple of every alignment class) and behind it


# ------------------------------------------------------------------------------------------------
# operands at a chosen address class
# ------------------------------------------------------------------------------------------------
def alignment(t):
    """The largest power of two, capped at 256, that divides t's address."""
    a = int(t.data_ptr())
    return 256 if a % 256 == 0 else a & -a


def stride_alignment(t):
    """The largest power of two, capped at 256, that divides t's row stride in BYTES (a lane of that many bytes or fewer that starts
    aligned in row 0 starts aligned in every row)."""
    s = int(t.stride(0)) * t.element_size() if t.dim() >= 1 else 0
    return 256 if s % 256 == 0 else s & -s


def pow2_class(nbytes):
    nbytes = int(nbytes)
    return 256 if nbytes % 256 == 0 else nbytes & -nbytes


class Guard(object):
    """What surrounds a view: `buf` the whole allocation as bytes, `payload` a bool tensor, True where a byte belongs to the view."""

    def __init__(self, buf, payload):
        self.buf, self.payload = buf, payload

    def intact(self):
        return bool((self.buf[~self.payload] == SENTINEL).all())


OffsetView = collections.namedtuple("OffsetView", ["view", "guard"])


def _arena(nbytes, device):
    """-> (bytes tensor whose first byte is 256-byte aligned, filled with the sentinel)."""
    raw = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
    lead = (-int(raw.data_ptr())) % 256
    buf = raw[lead:lead + int(nbytes)]
    assert int(buf.data_ptr()) % 256 == 0, "buffer base not 256-byte aligned"
    buf.fill_(SENTINEL)
    return buf


def offset_view(t, k, device=None):
    """The values of `t` as a CONTIGUOUS view that starts k elements past a 256-byte aligned address of a fresh buffer, with at
    least 256 sentinel bytes before and after it -> OffsetView(view, guard).  The view's address has exactly the alignment class of
    k * element_size (k = 0: 256), asserted."""
    device = t.device if device is None else torch.device(device)
    esz, n = t.element_size(), t.numel() * t.element_size()
    lo = GUARD + int(k) * esz
    buf = _arena(lo + n + GUARD + 16, device)
    view = buf[lo:lo + n].view(t.dtype).view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and alignment(view) == pow2_class(int(k) * esz), (alignment(view), k, esz)
    payload = torch.zeros(buf.shape[0], dtype=torch.bool, device=device)
    payload[lo:lo + n] = True
    return OffsetView(view, Guard(buf, payload))


def misaligned(t):
    """The same values as a contiguous view whose storage offset is 4-byte but not 16-byte aligned (one element in: for 2- and 8-byte
    types the element size)."""
    v = offset_view(t, 1).view
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() % 16 != 0
    return v


def column_block(t, a, width, device=None):
    """The values of the 2-D `t` [n, d] as the column block m[:, a:a + d] of a fresh row-major [n, width] matrix whose row 0 starts
    256-byte aligned: address class that of a * element_size, row stride width * element_size.  The columns outside the block (and
    256 bytes before and after the matrix) are the guard -> OffsetView(view, guard)."""
    device = t.device if device is None else torch.device(device)
    n, d = int(t.shape[0]), int(t.shape[1])
    a, width, esz = int(a), int(width), t.element_size()
    assert t.dim() == 2 and 0 <= a and a + d <= width and width > d
    nbytes = n * width * esz
    buf = _arena(GUARD + nbytes + GUARD, device)
    m = buf[GUARD:GUARD + nbytes].view(t.dtype).view(n, width)
    view = m[:, a:a + d]
    view.copy_(t)
    assert not view.is_contiguous() and view.stride(1) == 1 and view.stride(0) == width
    assert alignment(view) == pow2_class(a * esz) and stride_alignment(view) == pow2_class(width * esz)
    payload = torch.zeros((n, width * esz), dtype=torch.bool, device=device)
    payload[:, a * esz:(a + d) * esz] = True
    full = torch.zeros(buf.shape[0], dtype=torch.bool, device=device)
    full[GUARD:GUARD + nbytes] = payload.reshape(-1)
    return OffsetView(view, Guard(buf, full))


def guards_intact(*guards):
    """True when no byte outside the views was written (None entries: operands without a guard)."""
    return all(g is None or g.intact() for g in guards)


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
_TORCH_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """The raw bits of a tensor as an unsigned numpy array of the element's size (complex128: two 8-byte words per element)."""
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.complex128:
        t = torch.view_as_real(t).contiguous()
    return t.view(_TORCH_INT[t.element_size()]).numpy().view(_UINT[t.element_size()])


def _isnan(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.complex128:
        t = torch.view_as_real(t).contiguous()
    return torch.isnan(t).numpy() if t.is_floating_point() else np.zeros(tuple(t.shape), bool)


def assert_same_bits(got, want, what=""):
    """Bit equality of two tensors of one dtype and shape; NaN compared as a class (special_defs.assert_bits_equal)."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    assert_bits_equal(bits(got), bits(want), _isnan(want), _isnan(got), what)


_OUT_ROUND = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def aggregate_reference(x, src, dst, op, y=None, mop="add", out_size=None):
    """What gpu_common.check_aggregate holds a float sum / mean to, computed once and shared between the twins of a case:
    -> (want64, bound) per element -- fp64_terms and reassociation_bound with check_aggregate's constants (slack 4, the fp64 epsilon
    for fp64 features, half an output ulp more for 16-bit storage).  x, y: torch tensors in their storage type (on any device)."""
    import gpu_common as C
    xs = x.detach().cpu()
    storage = _OUT_ROUND.get(xs.dtype)
    xn = xs.double().numpy() if storage else xs.numpy()
    yn = None if y is None else (y.detach().cpu().double().numpy() if storage else y.detach().cpu().numpy())
    want64, absx, n_terms = C.fp64_terms(xn, src, dst, op, out_size, yn, mop)
    eps = C.EPS[np.dtype(np.float64)] if xs.dtype == torch.float64 else C.EPS[np.dtype(np.float32)]
    bound = C.reassociation_bound(absx, n_terms, 4.0, eps)
    if storage:
        bound = bound + C._OUT_ROUND[storage] * np.abs(want64) * 1.01
    return want64, bound


def assert_within(got, want64, bound, what=""):
    import gpu_common as C
    g = got.detach().cpu().double().numpy()
    C._assert_elementwise(np.abs(g - want64), np.broadcast_to(bound, g.shape), want64, what)


# ------------------------------------------------------------------------------------------------
# definitions the oracle and grad_defs do not have
# ------------------------------------------------------------------------------------------------
def int_send_uv(x, y, src, dst, mop):
    """send_uv on integer features as the kernel's C arithmetic defines it: wrap-around add / sub / mul in the storage width, division
    truncating toward zero (divisors non-zero).  numpy arrays in, [E, dout] out; trailing-dim broadcast as numpy does it."""
    a, b = np.asarray(x)[np.asarray(src)], np.asarray(y)[np.asarray(dst)]
    assert a.dtype == b.dtype and np.issubdtype(a.dtype, np.integer)
    if a.shape[1] != b.shape[1]:
        dout = max(a.shape[1], b.shape[1])
        a = np.repeat(a, dout // a.shape[1], 1) if a.shape[1] == 1 else a
        b = np.repeat(b, dout // b.shape[1], 1) if b.shape[1] == 1 else b
    with np.errstate(over="ignore"):
        if mop == "add":
            return a + b
        if mop == "sub":
            return a - b
        if mop == "mul":
            return a * b
    assert (b != 0).all()
    q = np.abs(a.astype(object)) // np.abs(b.astype(object))
    return (np.sign(a).astype(object) * np.sign(b).astype(object) * q).astype(a.dtype)


def float_send_uv(x, y, src, dst, mop):
    """send_uv on float features in the STORAGE type (one IEEE operation per element: what the kernel computes, bit for bit)."""
    a, b = np.asarray(x)[np.asarray(src)], np.asarray(y)[np.asarray(dst)]
    with np.errstate(all="ignore"):
        return {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}[mop](a, b).astype(a.dtype)


def seg_ptr_definition(keys, n_rows):
    """indptr of sorted keys: torch.searchsorted in int64 -- indptr[r] = the number of keys < r, r = 0 .. n_rows."""
    k = torch.as_tensor(np.asarray(keys), dtype=torch.int64)
    return torch.searchsorted(k, torch.arange(int(n_rows) + 1, dtype=torch.int64), right=False)


def gapped_keys(E, seed=0):
    """-> (sorted int64 keys [E], n_rows): consecutive distinct keys 1, 15, 16 and 17 absent ids apart (the row-fill loop of
    row_bounds_kernel switches at 16), repeated keys in between, and 40 rows after the last key."""
    rng = np.random.default_rng(seed)
    gaps = np.array([1, 2, 16, 17, 18])                     # a step of g leaves g - 1 ids absent: 0, 1, 15, 16, 17
    steps = np.where(rng.random(E) < 0.5, 0, gaps[np.arange(E) % len(gaps)])
    steps[0] = 17
    keys = np.cumsum(steps).astype(np.int64)
    return keys, int(keys[-1]) + 41


# ------------------------------------------------------------------------------------------------
# the selection rules, restated (what a row of a table is expected to reach)
# ------------------------------------------------------------------------------------------------
DTYPES = {"fp32": torch.float32, "fp64": torch.float64, "int32": torch.int32, "int64": torch.int64, "fp16": torch.float16,
          "bf16": torch.bfloat16, "uint8": torch.uint8, "c128": torch.complex128}
ESIZE = {"fp32": 4, "fp64": 8, "int32": 4, "int64": 8, "fp16": 2, "bf16": 2, "uint8": 1, "c128": 16}
KERNEL_TYPE = {"float": 4, "double": 8, "int": 4, "long": 8, "__half": 2, "__hip_bfloat16": 2}     # aggregate_flat.hpp type_name


def aggregate_vmax(esz, d, al, ldx_bytes=None, ldo_bytes=None):
    """aggregate_flat.hpp:982-986: the widest lane (elements) the row length, the row strides and the OR of the addresses allow."""
    v = 16 // esz
    row = d * esz
    ldx_bytes = row if ldx_bytes is None else ldx_bytes
    ldo_bytes = row if ldo_bytes is None else ldo_bytes
    while v > 1 and (d % v or ldx_bytes % (v * esz) or ldo_bytes % (v * esz) or al % (v * esz)):
        v //= 2
    return v


def zero_rows_word(row_bytes, al):
    """aggregate.hip:113-120 zero_empty_rows: bytes per store."""
    for w in (16, 8, 4):
        if row_bytes % w == 0 and al % w == 0:
            return w
    return 2


def send_uv_branch(esz, dx, dy, dout, al):
    vec = 16 // esz
    if dx == dout and dy == dout and dout % vec == 0 and al % 16 == 0:
        per = dout // vec
        return SEND_UV_VEC_POW2 if per & (per - 1) == 0 else SEND_UV_VEC_ANY
    return SEND_UV_GENERIC


def softmax_branch(esz, d, al):
    narrow = d <= (16 if esz == 4 else 8)
    vmax = 16 // esz
    vec = vmax if d % vmax == 0 and al % 16 == 0 else 2 if d % 2 == 0 and al % (2 * esz) == 0 else 1
    return (SOFTMAX_ONE_PASS if narrow else SOFTMAX_THREE_PASS) % vec


def move_rows_word(row_bytes, al):
    """edge_ops.hip:226-230: bytes per word of a row move."""
    for w in (16, 8, 4, 2):
        if row_bytes % w == 0 and al % w == 0:
            return w
    return 1


def gather_cast_vec(d, ld, al):
    return 4 if d % 4 == 0 and ld % 4 == 0 and al % 16 == 0 else 1


def csr_input_form(u_stride, v_stride, v_minus_u, u_al, v_al):
    """csr_build.hip:796-797 (u: the key column, strides and the distance v - u in elements)."""
    if u_stride == 2 and v_stride == 2 and v_minus_u == 1 and u_al % 16 == 0:
        return CSR_PAIR1
    if u_stride == 2 and v_stride == 2 and v_minus_u == -1 and v_al % 16 == 0:
        return CSR_PAIR2
    return CSR_STRIDED


def gat_lane_bytes(H, D, pow2):
    """gat_fused.hip:802-812 gat_vec on 16-byte aligned operands: bytes per lane (0: no width fits)."""
    for v in (1, 2, 4):
        lph = D // v
        if D % v == 0 and H * D <= 64 * v and not (pow2 and lph & (lph - 1)):
            return 4 * v
    return 0


def epilogue_lane_bytes(d):
    return 16 if d % 4 == 0 else 8 if d % 2 == 0 else 4


# ------------------------------------------------------------------------------------------------
# A. aggregation forward (ops.aggregate)
#    branches: AGG_BRANCHES below.  Alignment term (aggregate_flat.hpp:983-986, 1042-1044): x | out | y (a [E, d] operand) | ws, ldx, ldo.
#    The workspace is the front end's own 256-byte aligned scratch: not an operand a caller can move.
# ------------------------------------------------------------------------------------------------
AGG_GRAPH = dict(n_src=900, n_rows=500, e=40000, long_row=23, long_edges=7000)      # the graph of test_column_block_aggregation_reads_and_writes_in_place
AGG_WIDTHS = {"fp32": ((4, 8, 12, 16), (24, 32), (64, 128, 132, 256, 300)), "fp64": ((2, 8), (16, 32), (64, 128)),
              "int32": ((8,), (24,), (64,)), "int64": ((4,), (12,), (64,)),
              "fp16": ((8,), (24,), (64, 128, 136)), "bf16": ((8,), (24,), (64, 128, 136))}
# (the issue's widths, and fp64 d = 128: the flat kernel prefers 64 busy lanes to wide ones, so an 8-byte type takes VEC = 2 there only
#  from 128 elements on.  The classes hold for sum / mean without an edge operand and aligned operands -- max / min go to the grouped
#  kernel from 32 bytes up, 16-bit rows of 128 bytes too; the GPU test reads the family of every launch from its name.)
AGG_FAMILIES = ("lane-per-edge", "grouped", "flat")
AGG_OFFSETS = {4: (1, 2, 3), 8: (1,), 2: (1, 2, 4)}           # elements
AGG_VMAX = "aggregate_flat.hpp:986 vmax=%d"
AGG_NARROW_VEC = "aggregate_flat.hpp:1042 narrow_vec=%d"
AGG_ZERO = "aggregate.hip:113 zero_empty_rows word=%d"
AGG_GENERIC = "aggregate_flat.hpp:1063 generic fallback"
AGG_OPERANDS = ("x", "out", "y", "row32", "col32", "eid32")

AggCase = collections.namedtuple("AggCase", ["id", "dtype", "d", "op", "family", "layout", "offsets", "accumulate", "mop", "branch"])
# layout: "offset" (contiguous views `offsets` = {operand: elements}), "block-x" / "block-out" (column blocks: offsets = {operand: (first
# column, parent width)}), "empty" (an index without edges writing an offset out), "generic" (x [N, 1] against y [E, d]: gx > 1)


def _agg_branch(dtype, d, fam, offsets, has_y):
    esz = ESIZE[dtype]
    al = 0
    for k in ("x", "out") + (("y",) if has_y else ()):
        al |= offsets.get(k, 0) * esz
    al = al or 256
    if fam == "lane-per-edge":
        lv = min(16, d * esz)
        ok = lv & (lv - 1) == 0 and al % lv == 0
        return AGG_NARROW_VEC % (1 if ok else 0)
    return AGG_VMAX % aggregate_vmax(esz, d, al)


def _agg_cases():
    out = []

    def add(dtype, d, op, fam, layout, offsets, acc=0, mop=None, branch=None):
        tag = "+".join("%s%s" % (k, v if not isinstance(v, tuple) else "%d/%d" % v) for k, v in sorted(offsets.items())) or "aligned"
        cid = "%s-d%d-%s-%s-%s%s%s" % (dtype, d, op, layout, tag, "-acc" if acc else "", "-" + mop if mop else "")
        out.append(AggCase(cid, dtype, d, op, fam, layout, dict(offsets), acc, mop, branch or _agg_branch(dtype, d, fam, offsets, mop is not None)))

    for dtype, fams in AGG_WIDTHS.items():
        esz = ESIZE[dtype]
        offs = AGG_OFFSETS[esz]
        is_float = dtype in ("fp32", "fp64", "fp16", "bf16")
        for fam, widths in zip(AGG_FAMILIES, fams):
            for wi, d in enumerate(widths):
                op = ("sum", "mean", "max")[wi % 3]
                add(dtype, d, op, fam, "offset", {})                                        # the aligned case of this shape
                if wi == 0:
                    for k in offs:
                        add(dtype, d, "sum", fam, "offset", {"x": k})
                        add(dtype, d, "mean" if is_float else "sum", fam, "offset", {"out": k})
                        add(dtype, d, "sum", fam, "offset", {"out": k}, acc=1)
                    add(dtype, d, "max", fam, "offset", {"x": offs[0]})
                    add(dtype, d, "min", fam, "offset", {"out": offs[-1]})
                    add(dtype, d, "max", fam, "offset", {"x": offs[0], "out": offs[0]})
                    if is_float:
                        add(dtype, d, "sum", fam, "offset", {}, mop="mul")
                        add(dtype, d, "sum", fam, "offset", {"y": offs[0]}, mop="mul")
                        add(dtype, d, "sum", fam, "offset", {"x": offs[0], "out": offs[0], "y": offs[0]}, mop="mul")
                    else:
                        add(dtype, d, "sum", fam, "offset", {"x": offs[0], "out": offs[0]})
                    # column blocks at an odd first column of an odd-width parent: neither the address nor the stride is a multiple of a lane
                    add(dtype, d, "sum", fam, "block-x", {"x": (3, 2 * d + 7)}, branch=AGG_VMAX % 1 if fam != "lane-per-edge" else AGG_NARROW_VEC % 0)
                    add(dtype, d, "max", fam, "block-out", {"out": (5, 2 * d + 9)}, branch=AGG_VMAX % 1 if fam != "lane-per-edge" else AGG_NARROW_VEC % 0)
                    add(dtype, d, "sum", fam, "block-out", {"out": (5, 2 * d + 9)}, acc=1, branch=AGG_VMAX % 1 if fam != "lane-per-edge" else AGG_NARROW_VEC % 0)
                    add(dtype, d, "sum", fam, "offset", {"row32": 1, "col32": 1})
                    if is_float:
                        add(dtype, d, "sum", fam, "offset", {"eid32": 1}, mop="mul")
                else:
                    add(dtype, d, op, fam, "offset", {"x": offs[0]})
                    add(dtype, d, op, fam, "offset", {"out": offs[-1]})
                    add(dtype, d, op, fam, "offset", {"x": offs[-1], "out": offs[-1]})
        # an index without edges writing an offset out: every word width of zero_empty_rows this element size can reach
        d0 = {4: 4, 8: 2, 2: 8}[esz]
        for k in (0,) + offs:
            add(dtype, d0, "sum", "zero-fill", "empty", {"out": k} if k else {}, branch=AGG_ZERO % zero_rows_word(d0 * esz, (k * esz) or 256))
    add("fp32", 8, "sum", "generic", "generic", {}, mop="mul", branch=AGG_GENERIC)
    add("fp32", 8, "sum", "generic", "generic", {"x": 1, "y": 1, "out": 1}, mop="mul", branch=AGG_GENERIC)
    return out


AGG_CASES = _agg_cases()
AGG_BRANCHES = sorted({AGG_VMAX % v for v in (1, 2, 4, 8)} | {AGG_NARROW_VEC % v for v in (0, 1)} | {AGG_ZERO % w for w in (2, 4, 8, 16)} | {AGG_GENERIC})


# ------------------------------------------------------------------------------------------------
# B. edge-wise kernels and row moves (edge_ops.hip)
# ------------------------------------------------------------------------------------------------
EDGE_GRAPH = dict(n=1200, e=4099)                               # 4099: not a multiple of the unroll (4) nor of a block
SEND_UV_VEC_POW2 = "edge_ops.hip:119 vector kernel, power-of-two groups"
SEND_UV_VEC_ANY = "edge_ops.hip:119 vector kernel, log2per = -1"
SEND_UV_GENERIC = "edge_ops.hip:121 generic kernel"
SEND_UV_SECOND_TRIP = "edge_ops.hip:101 generic kernel, second trip of the grid-stride loop"
SEND_UV_BRANCHES = (SEND_UV_VEC_POW2, SEND_UV_VEC_ANY, SEND_UV_GENERIC, SEND_UV_SECOND_TRIP)
SEND_UV_OPERANDS = ("x", "y", "out")
SEND_UV_GRID = 8192 * 256                                       # grid_for's cap times the block: one trip of the generic kernel

SendUVCase = collections.namedtuple("SendUVCase", ["id", "dtype", "dx", "dy", "mop", "e", "offsets", "via", "branch"])


def _send_uv_cases():
    out = []
    mops = ("add", "sub", "mul", "div")
    i = 0
    for dtype in ("fp32", "fp64", "int32", "int64"):
        esz = ESIZE[dtype]
        for d in (4, 8, 16, 12, 5):
            for offsets, via in (({}, "ops"), ({"x": 1}, "ops"), ({"y": 1}, "ops"), ({"out": 1}, "abi"), ({}, "abi")):
                if d in (8, 16) and offsets and "x" not in offsets:
                    continue
                al = 0
                for v in offsets.values():
                    al |= v * esz
                mop = mops[i % 4]; i += 1
                tag = "+".join("%s%d" % kv for kv in sorted(offsets.items())) or "aligned"
                out.append(SendUVCase("%s-d%d-%s-%s-%s" % (dtype, d, mop, tag, via), dtype, d, d, mop, EDGE_GRAPH["e"], dict(offsets), via,
                                      send_uv_branch(esz, d, d, d, al or 256)))
        for dx, dy in ((1, 8), (8, 1)):
            for offsets in ({}, {"x": 1}, {"y": 1}):
                mop = mops[i % 4]; i += 1
                tag = "+".join("%s%d" % kv for kv in sorted(offsets.items())) or "aligned"
                out.append(SendUVCase("%s-%dx%d-%s-%s" % (dtype, dx, dy, mop, tag), dtype, dx, dy, mop, EDGE_GRAPH["e"], dict(offsets), "ops", SEND_UV_GENERIC))
    out.append(SendUVCase("fp32-d1-add-second-trip", "fp32", 1, 1, "add", SEND_UV_GRID + 257, {"x": 1}, "ops", SEND_UV_SECOND_TRIP))
    return out


SEND_UV_CASES = _send_uv_cases()

SOFTMAX_ONE_PASS = "edge_ops.hip:187 one-pass normalisation (narrow statistics), VEC=%d"
SOFTMAX_THREE_PASS = "edge_ops.hip:187 three-pass form, VEC=%d"
SOFTMAX_D = (1, 2, 6, 8, 16, 18, 20, 33, 100)
SOFTMAX_OPERANDS = ("data",)
SoftmaxCase = collections.namedtuple("SoftmaxCase", ["id", "dtype", "d", "kind", "offsets", "branch"])
SOFTMAX_CASES = [SoftmaxCase("%s-%s-d%d-k%d" % (kind, dtype, d, k), dtype, d, kind, {"data": k} if k else {},
                             softmax_branch(ESIZE[dtype], d, (k * ESIZE[dtype]) or 256))
                 for dtype in ("fp32", "fp64") for d in SOFTMAX_D for k in (0, 1, 2)
                 for kind in (("segment", "edge") if d in (1, 8, 20) else ("segment",) if d % 2 else ("edge",))]
SOFTMAX_BRANCHES = sorted({SOFTMAX_ONE_PASS % v for v in (1, 2, 4)} | {SOFTMAX_THREE_PASS % v for v in (1, 2, 4)})

MOVE_WORD = "edge_ops.hip:226 word of %d bytes, %s index"
MOVE_OPERANDS = ("x", "out", "index")
MOVE_ELEMS = {"uint8": 1, "fp16": 2, "fp32": 4, "fp64": 8, "c128": 16}
MOVE_ROW_BYTES = (3, 6, 12, 24, 48)
MoveCase = collections.namedtuple("MoveCase", ["id", "op", "dtype", "d", "index", "offsets", "branch"])     # offsets: x / out in BYTES, index in elements


def _move_cases():
    out = []
    i = 0
    for rb in MOVE_ROW_BYTES:
        for dtype, esz in MOVE_ELEMS.items():
            if rb % esz:
                continue
            # offsets that knock the word down one class at a time: from the widest word the row allows to the element size
            offs = [0] + [w for w in (8, 4, 2, 1) if w % esz == 0 and rb % (2 * w) == 0]
            for off in offs:
                # gather_rows allocates its result itself: x is the operand a caller can move; scatter_rows takes both
                for op, operand in (("gather", "x"), ("scatter", "out"), ("scatter", "x")):
                    idx = ("int32", "int64")[(i // 3 + i) % 2]; i += 1
                    word = move_rows_word(rb, off or 256)
                    out.append(MoveCase("%s-%s-row%d-%s%d-%s" % (op, dtype, rb, operand, off, idx), op, dtype, rb // esz, idx,
                                        {operand: off} if off else {}, MOVE_WORD % (word, idx)))
    for idx in ("int32", "int64"):
        for op in ("gather", "scatter"):
            out.append(MoveCase("%s-fp32-row48-index1-%s" % (op, idx), op, "fp32", 12, idx, {"index": 1}, MOVE_WORD % (16, idx)))
    return out


MOVE_CASES = _move_cases()
MOVE_BRANCHES = sorted({MOVE_WORD % (w, i) for w in (1, 2, 4, 8, 16) for i in ("int32", "int64")})

CAST_VEC = "edge_ops.hip:414 gather_cast VEC=%d"
CAST_PAIRS = (("fp32", "fp16"), ("fp32", "bf16"), ("fp16", "fp32"), ("bf16", "fp32"), ("fp32", "fp32"), ("fp16", "fp16"), ("bf16", "bf16"))
CAST_OPERANDS = ("x", "out")
CastCase = collections.namedtuple("CastCase", ["id", "src", "dst", "d", "layout", "offsets", "index", "branch"])


def _cast_cases():
    out = []
    for s, t in CAST_PAIRS:
        for d in (8, 6):
            for layout, offsets, index in (("offset", {}, True), ("offset", {}, False), ("offset", {"x": 1}, True), ("offset", {"out": 1}, True),
                                           ("block", {"x": (3, 2 * d + 5)}, True), ("block", {"x": (4, 2 * d + 4)}, False)):
                if layout == "block":
                    a, w = offsets["x"]
                    vec = gather_cast_vec(d, w, pow2_class(a * ESIZE[s]))
                else:
                    al = 0
                    for k, v in offsets.items():
                        al |= v * ESIZE[s if k == "x" else t]
                    vec = gather_cast_vec(d, d, al or 256)
                tag = "+".join("%s%s" % (k, v if not isinstance(v, tuple) else "%d/%d" % v) for k, v in sorted(offsets.items())) or "aligned"
                out.append(CastCase("%s-to-%s-d%d-%s-%s-%s" % (s, t, d, layout, tag, "index" if index else "rows"), s, t, d, layout, dict(offsets), index, CAST_VEC % vec))
    return out


CAST_CASES = _cast_cases()
CAST_BRANCHES = [CAST_VEC % 1, CAST_VEC % 4]

SegReduceCase = collections.namedtuple("SegReduceCase", ["id", "d", "pool", "ids", "offsets", "branch"])
SEG_REDUCE_OPERANDS = ("data", "ids")
BOUNDS_ALIGNED = "csr_build.hip:59 aligned key load"
BOUNDS_UNALIGNED = "csr_build.hip:63 key by key"
SEG_REDUCE_CASES = [SegReduceCase("%s-d%d-%s-%s" % (pool, d, ids, "+".join("%s%d" % kv for kv in sorted(o.items())) or "aligned"), d, pool, ids, dict(o),
                                  BOUNDS_UNALIGNED if "ids" in o and ids == "int32" else BOUNDS_ALIGNED)
                    for d, pool in ((8, "sum"), (33, "max"), (128, "mean"))
                    for ids in ("int32", "int64") for o in ({}, {"ids": 1}, {"data": 1}, {"ids": 1, "data": 1})]
# (pglamd_segment_reduce narrows int64 ids into its own scratch before row_bounds_kernel sees them: only int32 ids reach it unaligned)


# ------------------------------------------------------------------------------------------------
# C. index construction (csr_build.hip)
# ------------------------------------------------------------------------------------------------
CSR_PAIR1 = "csr_build.hip:796 pair = 1"
CSR_PAIR2 = "csr_build.hip:797 pair = 2"
CSR_STRIDED = "csr_build.hip:795 strided columns"
CSR_BRANCHES = (CSR_PAIR1, CSR_PAIR2, CSR_STRIDED)
CSR_SIZES = ((1, 1), (4095, 300), (4097, 300), (70001, 70000))
# form -> (what ops.csr_build is handed, the branch): u is the KEY column
CSR_FORMS = collections.OrderedDict([
    ("separate", CSR_STRIDED),            # two separate contiguous columns: the form every other one must equal bit for bit
    ("pair", CSR_PAIR1),                  # u, v = the two columns of an aligned [E, 2]
    ("pair-swapped", CSR_PAIR2),          # u, v = column 1, column 0 of the same [E, 2]
    ("pair-8-bytes-in", CSR_STRIDED),     # the same [E, 2] 8 bytes into its storage: int64 pairs at an address that is 8 mod 16
    ("of-three", CSR_STRIDED),            # columns 0 and 1 of an [E, 3]
    ("separate-8-bytes-in", CSR_STRIDED),  # separate columns, each 8 bytes into its storage
])
BOUNDS_E = (1, 3, 4, 5, 255, 256, 257, 1021)
BOUNDS_BRANCHES = (BOUNDS_ALIGNED, BOUNDS_UNALIGNED)
BoundsCase = collections.namedtuple("BoundsCase", ["id", "entry", "ids", "e", "k", "branch"])
# (row_bounds_kernel loads 4 keys at once from a key array aligned to 4 keys; ops.csr_from_sorted narrows int64 keys into a fresh
#  int32 array first and takes int32 keys as they are)
BOUNDS_CASES = [BoundsCase("%s-%s-E%d-k%d" % (entry, ids, e, k), entry, ids, e, k,
                           BOUNDS_ALIGNED if k % 4 == 0 or (entry == "csr_from_sorted" and ids == "int64") else BOUNDS_UNALIGNED)
                for entry in ("seg_ptr_from_ids", "csr_from_sorted") for ids in ("int32", "int64") for e in BOUNDS_E for k in (0, 1, 2)]


# ------------------------------------------------------------------------------------------------
# D. fused attention, epilogue, fused dense layer -- through the front end
#    "copy": ops._aligned hands the entry point a fresh allocation; "as it is": the operand satisfies the entry point's alignment.
# ------------------------------------------------------------------------------------------------
ATT_HD = ((4, 8), (8, 16), (8, 32))
ATT_COPY = "ops.py _aligned: a fresh copy (below the %d-byte lane)"
ATT_AS_IS = "ops.py _aligned: as it is (%d-byte lane)"
ATT_OPERANDS = {"gat": ("feature", "attn_src", "attn_dst", "cotangent"), "sddmm": ("x", "y", "cotangent"), "add_score": ("x", "y", "w", "cotangent")}
AttCase = collections.namedtuple("AttCase", ["id", "op", "H", "D", "operand", "offset_bytes", "branch"])


def _att_branch(op, H, D, operand, off):
    # the widest lane any entry point of the op's forward and backward reads the operand in (per-(node, head) and per-edge scalars: 4 bytes)
    if operand in ("attn_src", "attn_dst"):
        need = 4
    elif op == "add_score" and operand == "w":
        need = 16                                               # (pglamd_add_score_backward asks 16 bytes of w at every width)
    elif operand == "cotangent":
        need = 16 if op == "gat" else 4 if op == "sddmm" else 4
    else:
        need = gat_lane_bytes(H, D, op != "gat")
    return (ATT_AS_IS if off % need == 0 else ATT_COPY) % need


ATT_CASES = [AttCase("%s-%dx%d-%s-%d" % (op, H, D, operand, off), op, H, D, operand, off, _att_branch(op, H, D, operand, off))
             for op in ("gat", "sddmm", "add_score") for H, D in ATT_HD for operand in ATT_OPERANDS[op] for off in (4, 8)]
ATT_BRANCHES = sorted({ATT_COPY % 8, ATT_COPY % 16, ATT_AS_IS % 4, ATT_AS_IS % 8})
AGG_ROWS_WITH_EDGES = 480        # rows 480 .. 499 of the aggregation graph receive no edge (zero-fill; kept as they are under accumulate)

EPILOGUE_D = (7, 64, 130, 256, 516)
EPILOGUE_MODES = ((None, False), ("relu", False), (None, True), ("relu", True))
EPILOGUE_OPERANDS = ("z", "dy", "y", "bias")
EPI_COPY = "ops.py _aligned: a fresh copy (below the %d-byte lane)"
EPI_AS_IS = "ops.py _aligned: as it is (%d-byte lane)"
EpiCase = collections.namedtuple("EpiCase", ["id", "d", "act", "normalize", "operand", "offset_bytes", "branch"])


def _epi_cases():
    out = []
    for d in EPILOGUE_D:
        lane = epilogue_lane_bytes(d)
        for mi, (act, nz) in enumerate(EPILOGUE_MODES):
            for operand in EPILOGUE_OPERANDS:
                if operand == "y" and not (act or nz):
                    continue                                    # (the backward reads y only behind an activation or a normalisation)
                for off in ((4, 8) if mi == 3 else (4,)):
                    need = 4 if operand == "bias" else lane
                    out.append(EpiCase("d%d-%s-%s-%s-%d" % (d, act, "norm" if nz else "plain", operand, off), d, act, nz, operand, off,
                                       (EPI_AS_IS if off % need == 0 else EPI_COPY) % need))
    return out


EPI_CASES = _epi_cases()
EPI_BRANCHES = sorted({EPI_COPY % 8, EPI_COPY % 16, EPI_AS_IS % 4, EPI_AS_IS % 8})

DENSE_SHAPES = ((64, 32), (128, 128))
DENSE_OPERANDS = ("x", "w", "bias")
DENSE_COPY_X = "aggregate.hip:348 x below 8 bytes: ops._aligned copies"
DENSE_FORM2_KEPT = "aggregate.hip:360 w below 16 bytes: ops._aligned copies, the LDS form is kept"
DENSE_BIAS = "aggregate.hpp:143 bias one float at a time: as it is"
DenseCase = collections.namedtuple("DenseCase", ["id", "d_in", "d_out", "operand", "offset_bytes", "branch"])
DENSE_CASES = [DenseCase("%d-%d-%s-%d" % (di, do, operand, 4), di, do, operand, 4, {"x": DENSE_COPY_X, "w": DENSE_FORM2_KEPT, "bias": DENSE_BIAS}[operand])
               for di, do in DENSE_SHAPES for operand in DENSE_OPERANDS]
DENSE_BRANCHES = (DENSE_COPY_X, DENSE_FORM2_KEPT, DENSE_BIAS)

# the C entry points that document an alignment they need -> (operand below it, the code the header documents)
REFUSALS = collections.OrderedDict([
    ("gat_aggregate", ("feature", "PGLAMD_E_SHAPE")), ("gat_backward", ("feature", "PGLAMD_E_SHAPE")), ("sddmm", ("x_by_col", "PGLAMD_E_SHAPE")),
    ("add_score", ("w", "PGLAMD_E_SHAPE")), ("add_score_backward", ("w", "PGLAMD_E_SHAPE")), ("aggregate_dense", ("x", "PGLAMD_E_ARG")),
    ("row_epilogue", ("z", "PGLAMD_E_ARG")), ("row_epilogue_backward", ("dy", "PGLAMD_E_ARG"))])
CODES = {"PGLAMD_E_SHAPE": -1, "PGLAMD_E_ARG": -6}


# ------------------------------------------------------------------------------------------------
# what every table must satisfy (tests/test_layout_defs.py)
# ------------------------------------------------------------------------------------------------
def offset_alone(cases, operand, key="offsets"):
    """The cases of a table that move `operand` and nothing else."""
    hit = []
    for c in cases:
        o = getattr(c, key, None)
        if isinstance(o, dict):
            if set(o) == {operand}:
                hit.append(c)
        elif getattr(c, "operand", None) == operand:
            hit.append(c)
    return hit


TABLES = collections.OrderedDict([
    ("aggregate", (AGG_CASES, AGG_BRANCHES, ("x", "out", "y"))),
    ("send_uv", (SEND_UV_CASES, SEND_UV_BRANCHES, SEND_UV_OPERANDS)),
    ("softmax", (SOFTMAX_CASES, SOFTMAX_BRANCHES, SOFTMAX_OPERANDS)),
    ("move_rows", (MOVE_CASES, MOVE_BRANCHES, MOVE_OPERANDS)),
    ("cast", (CAST_CASES, CAST_BRANCHES, CAST_OPERANDS)),
    ("segment_reduce", (SEG_REDUCE_CASES, BOUNDS_BRANCHES, SEG_REDUCE_OPERANDS)),
    ("row_bounds", (BOUNDS_CASES, BOUNDS_BRANCHES, ())),
    ("attention", (ATT_CASES, ATT_BRANCHES, tuple(sorted({o for v in ATT_OPERANDS.values() for o in v})))),
    ("epilogue", (EPI_CASES, EPI_BRANCHES, EPILOGUE_OPERANDS)),
    ("dense", (DENSE_CASES, DENSE_BRANCHES, DENSE_OPERANDS)),
])
