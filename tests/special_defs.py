"""Special values (DESIGN.md "Special values"): NaN, +-inf, subnormals and integer wrap-around, as DEFINITIONS.

The definition of every op is its existing fp64 restatement evaluated with IEEE semantics -- oracle/ref_ops.py np_send_u_recv /
np_send_ue_recv / np_segment*, the torch definitions of tests/grad_defs.py -- which does not depend on edge order.  This module adds
what the special-value tests (tests/test_special_defs.py on the CPU, tests/test_special_values_gpu.py on the MI355X) share:

  * classify_and_check: rule 1 of the contract.  Per output element the CLASS (NaN / +inf / -inf / finite) must equal the definition's,
    a finite element must lie inside its bound.  There is NO absolute floor (gpu_common.reassociation_bound adds finfo(float32).tiny,
    so a result flushed to zero passes it) and no element is left out.  +-0 compare equal.
  * rebound: the re-association bound of gpu_common without that floor.
  * special_graph / plant: ONE graph for the aggregation cases -- empty rows, a row of one edge, rows of 255 / 256 / 257 and
    4096 / 4353 edges (the chunk and fix-up class boundaries), a 40 000-edge hub -- whose rows have SLOTS: positions of the
    destination-sorted row (first, middle, last, and positions in later chunks of split rows) whose source is a carrier node read by
    that one edge only, so a planted value reaches exactly one message.
  * subnormal_features: multiples of 2**-149 whose row totals stay below 2**-125, so every partial sum in ANY order is exact in fp32.
  * the fp32 -> 16-bit cast set and torch's CPU cast as the definition of a 16-bit store.
"""
import numpy as np
import torch

import ref_ops as R
from grad_defs import K_FAMILY

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
NAN, INF = float("nan"), float("inf")
FINITE, ISNAN, PINF, NINF = 0, 1, 2, 3
CLASS_NAME = {FINITE: "finite", ISNAN: "NaN", PINF: "+inf", NINF: "-inf"}
OVERFLOW_GUARD = 2.0 ** 126          # every finite-class element's sum of |terms| stays below this: no order of summation overflows fp32


def classes(a):
    a = np.asarray(a, np.float64)
    c = np.zeros(a.shape, np.int8)
    c[np.isnan(a)] = ISNAN
    c[np.isposinf(a)] = PINF
    c[np.isneginf(a)] = NINF
    return c


def rebound(abs_terms, n_terms, eps=EPS32, slack=4.0):
    """slack * n * eps * sum|t_i| per element (Higham 4.4) -- gpu_common.reassociation_bound WITHOUT its absolute floor."""
    with np.errstate(invalid="ignore", over="ignore"):
        return slack * np.maximum(np.asarray(n_terms, np.float64), 1.0) * eps * np.asarray(abs_terms, np.float64)


def classify_and_check(got, want64, bound=0.0, what=""):
    """Rule 1.  got: the result under test (any float or integer type); want64: the definition (fp64, or the integer type for
    integer results, which are compared exactly); bound: per-element bound of the finite elements (broadcastable; a NaN / inf bound
    on an element of non-finite class is ignored, on a finite-class element it fails).  Raises AssertionError naming the worst element
    and its class."""
    got_a, want_a = np.asarray(got), np.asarray(want64)
    assert got_a.shape == want_a.shape, (what, got_a.shape, want_a.shape)
    if np.issubdtype(got_a.dtype, np.integer) or np.issubdtype(want_a.dtype, np.integer):
        assert got_a.dtype == want_a.dtype, (what, got_a.dtype, want_a.dtype)
        bad = got_a != want_a
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: integer element %s: got %d, want %d; %d of %d elements differ"
                                 % (what or "special values", i, got_a[i], want_a[i], int(bad.sum()), bad.size))
        return
    g, w = got_a.astype(np.float64), want_a.astype(np.float64)
    cg, cw = classes(g), classes(w)
    b = np.broadcast_to(np.asarray(bound, np.float64), w.shape)
    fin = (cg == FINITE) & (cw == FINITE)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(g - w), 0.0)
        bad_val = fin & ~(err <= b)                     # (a NaN bound on a finite element is out of bound)
    bad_cls = cg != cw
    if not (bad_cls.any() or bad_val.any()):
        return
    if bad_cls.any():
        i = tuple(int(v) for v in np.argwhere(bad_cls)[0])
        head = "element %s: class %s, the definition's is %s (got %r, want %r)" % (i, CLASS_NAME[int(cg[i])], CLASS_NAME[int(cw[i])], g[i], w[i])
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bad_val, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.inf), 0.0)
        i = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), w.shape))
        head = "element %s: class finite, |err| %.6e > bound %.6e (got %.9e, want %.9e)" % (i, err[i], b[i], g[i], w[i])
    raise AssertionError("%s: %s; %d elements of the wrong class, %d finite elements out of bound, of %d"
                         % (what or "special values", head, int(bad_cls.sum()), int(bad_val.sum()), w.size))


def refuses(fn, *a, **kw):
    """True when fn(*a, **kw) raises AssertionError (a mutant must be refused)."""
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------
# the aggregation graph
# ------------------------------------------------------------------------------------------------
ROW_LENS = {0: 1, 1: 2, 2: 3, 3: 5, 4: 17, 5: 64, 6: 255, 7: 256, 8: 257, 9: 4096, 10: 4353, 11: 40000}
ALL_CARRIER_ROWS = (0, 1, 2, 8)        # every edge of these rows has a carrier source: all-NaN / all -inf rows (8: a split row)
PREFIX_ROWS = {9: 300, 11: 300}       # the first 300 edges of these long rows have carrier sources too: a hub whose whole first chunks are masked
N_GENERIC = 500                        # generic source nodes 0..499; rows 20..399 receive short random rows, 12..19 and 400..499 none
EMPTY_ROWS = tuple(range(12, 20)) + tuple(range(400, 500))


def _slot_positions(L):
    pos = {0, L // 2, L - 1}
    for p in (256, 300, 4095, 4096, 4200, 20000, 39990):      # positions in chunks other than the first (chunks of 256 edges and larger)
        if p < L:
            pos.add(p)
    return sorted(pos)


class SpecialGraph(object):
    """n nodes; src / dst int64 [E] in a shuffled (original) edge order; slots[row] = positions (of the destination-sorted row) whose
    source is a carrier; carrier[(row, pos)] = that node.  The engine's index is a STABLE sort by destination, so position p of row r
    is the p-th edge of the original list with that destination: edge_of[(row, pos)]."""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        dst = [np.full(L, r, np.int64) for r, L in ROW_LENS.items()] + [rng.integers(20, 400, 3000).astype(np.int64)]
        dst = np.concatenate(dst)
        dst = dst[rng.permutation(len(dst))]
        src = rng.integers(0, N_GENERIC, len(dst)).astype(np.int64)
        order = np.argsort(dst, kind="stable")
        starts = np.zeros(N_GENERIC + 1, np.int64)
        np.cumsum(np.bincount(dst, minlength=N_GENERIC), out=starts[1:])
        self.slots, self.carrier, self.edge_of = {}, {}, {}
        nxt = N_GENERIC
        for r, L in ROW_LENS.items():
            self.slots[r] = list(range(L)) if r in ALL_CARRIER_ROWS else sorted(set(_slot_positions(L)) | set(range(PREFIX_ROWS.get(r, 0))))
            for p in self.slots[r]:
                e = int(order[starts[r] + p])
                src[e] = nxt
                self.carrier[(r, p)], self.edge_of[(r, p)] = nxt, e
                nxt += 1
        self.n, self.src, self.dst, self.E = nxt, src, dst, len(dst)
        self.indeg = np.bincount(dst, minlength=self.n)
        assert (np.bincount(src, minlength=self.n)[N_GENERIC:] == 1).all()          # a carrier feeds exactly one edge
        assert all(self.indeg[r] == 0 for r in EMPTY_ROWS) and (self.indeg[N_GENERIC:] == 0).all()

    @property
    def edges(self):
        return np.stack([self.src, self.dst], 1)

    def features(self, d, dtype=np.float32, seed=1):
        """Finite, normal features in the storage type `dtype` (numpy type, or torch.float16 / torch.bfloat16 -> a torch tensor)."""
        rng = np.random.default_rng(seed + d)
        if isinstance(dtype, torch.dtype):
            return torch.from_numpy(rng.standard_normal((self.n, d)).astype(np.float32)).to(dtype)
        if np.issubdtype(dtype, np.integer):
            return rng.integers(-1000, 1000, (self.n, d)).astype(dtype)
        return rng.standard_normal((self.n, d)).astype(dtype)


def as_f64(x):
    """The stored values of a numpy array or (16-bit) torch tensor, in fp64."""
    return x.double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def plant(G, x, plants):
    """plants: list of (row, position-in-row, column or None for the whole feature row, value).  -> a copy of x with the value written
    into the carrier of that slot.  (The expectation is the definition evaluated on the result: `expect`.)"""
    x = x.clone() if isinstance(x, torch.Tensor) else np.array(x, copy=True)
    for r, p, col, v in plants:
        node = G.carrier[(r, p)]
        if col is None:
            x[node] = v
        else:
            x[node, col] = v
    return x


def expect(G, x, op, out_size=None, y=None, mop="add"):
    """-> (want64, bound): the fp64 definition on the stored values and the per-element bound of the finite elements: 0 for max / min
    of stored values, else the re-association bound of the element's own finite terms in the ACCUMULATION type (fp32 for fp32 and
    16-bit storage) plus, for 16-bit storage, the one rounding of the result."""
    x64 = as_f64(x)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if y is None:
            want = R.np_send_u_recv(x64, G.src, G.dst, op, out_size)
            absx = R.np_send_u_recv(np.abs(x64), G.src, G.dst, op if op == "mean" else "sum", out_size)
        else:
            y64 = as_f64(y)
            want = R.np_send_ue_recv(x64, y64, G.src, G.dst, mop, op, out_size)
            msg = np.abs(R._mop(x64[G.src], y64, mop))
            absx = R._np_reduce_rows(msg, G.dst, want.shape[0], op if op == "mean" else "sum")
    m = want.shape[0]
    deg = np.bincount(G.dst, minlength=m)[:m].astype(np.float64).reshape((m,) + (1,) * (want.ndim - 1))
    is64 = (not isinstance(x, torch.Tensor)) and np.asarray(x).dtype == np.float64
    eps = EPS64 if is64 else EPS32
    if op in ("max", "min"):
        bound = np.zeros_like(want) if y is None else 2.0 * eps * np.abs(want)
    else:
        bound = rebound(absx, deg + (op == "mean") + (y is not None), eps)
    if isinstance(x, torch.Tensor) and x.dtype in (torch.float16, torch.bfloat16) and not (op in ("max", "min") and y is None):
        # one round-to-nearest of the fp32 accumulator to 16 bits: half an ulp, relative -- and for fp16, whose subnormals begin at
        # 2**-14, half a subnormal spacing (2**-25) where the result is that small (the format's own precision, not a floor of ours)
        with np.errstate(invalid="ignore"):
            bound = bound + (2.0 ** -11 if x.dtype == torch.float16 else 2.0 ** -8) * 1.01 * np.abs(want) + \
                (2.0 ** -25 if x.dtype == torch.float16 else 0.0)
    if op in ("sum", "mean"):
        assert_no_overflow(want, absx)
    return want, bound


def assert_no_overflow(want64, abs_terms):
    """The condition of the contract: every finite-class element's sum of |terms| stays below 2**126."""
    fin = classes(want64) == FINITE
    a = np.broadcast_to(np.asarray(abs_terms, np.float64), np.shape(want64))
    assert np.isfinite(a[fin]).all() and (a[fin] < OVERFLOW_GUARD).all(), "a finite-class element's terms could overflow fp32 in some order"


# the planted cases of the aggregation tests: name -> list of (row, position, value); positions "first" / "mid" / "last" / "late" (the
# last slot that is not the last position: inside a later chunk of a split row) are resolved per row by `resolve`
def resolve(G, row, where):
    s = G.slots[row]
    L = ROW_LENS[row]
    if where == "first": return 0
    if where == "last": return L - 1
    if where == "late": return [p for p in s if p != L - 1][-1]
    if where == "mid": return L // 2
    raise KeyError(where)


PLANT_ROWS = (0, 3, 5, 6, 7, 8, 9, 10, 11)


def planted_cases(G):
    """-> {name: [(row, pos, col, value)]}; col None = the whole feature row of the carrier."""
    cases = {}
    for name, v in (("nan", NAN), ("pinf", INF), ("ninf", -INF)):
        pl = []
        for i, r in enumerate(PLANT_ROWS):
            where = ("first", "mid", "last", "late")[i % 4] if ROW_LENS[r] > 1 else "first"
            pl.append((r, resolve(G, r, where), None, v))
        for where in ("first", "mid", "last", "late"):           # the split rows and the hub: every position class
            for r in (8, 10, 11):
                pl.append((r, resolve(G, r, where), 0, v))         # (column 0 only: the other columns of these messages stay finite)
        cases[name] = pl
    cases["inf_and_minus_inf"] = [(r, resolve(G, r, "first"), None, INF) for r in (3, 8, 10, 11)] + \
                                 [(r, resolve(G, r, "late" if ROW_LENS[r] > 5 else "last"), None, -INF) for r in (3, 8, 10, 11)]
    cases["all_nan_rows"] = [(r, p, None, NAN) for r in ALL_CARRIER_ROWS for p in G.slots[r]]
    cases["all_ninf_rows"] = [(r, p, None, -INF) for r in ALL_CARRIER_ROWS for p in G.slots[r]]
    return cases


# ------------------------------------------------------------------------------------------------
# subnormals: sums that are exact in fp32 in any order
# ------------------------------------------------------------------------------------------------
SUB_UNIT = 2.0 ** -149


def subnormal_features(G, d, seed=5, signed=True):
    """fp32 [n, d]: integer multiples k * 2**-149 with |k| small enough that the sum of |x[src]| over ANY destination row stays below
    2**-125 = 2**24 units -- so every partial sum, in any order, is an integer below 2**24 units: exact (subnormal or the lowest
    normal binade, whose spacing is the same 2**-149).  sum / max / min are then bit-exact and a mean is one correctly rounded
    division away (at most one fp32 rounding, of a value that may itself be subnormal: half a unit)."""
    rng = np.random.default_rng(seed + d)
    kmax = max(1, int((2 ** 24 - 1) // int(G.indeg.max())))               # 40 000-edge hub: |k| <= 419
    k = rng.integers(-kmax if signed else 0, kmax + 1, (G.n, d))
    x = (k.astype(np.float64) * SUB_UNIT).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), k * SUB_UNIT)              # representable
    tot = R.np_send_u_recv(np.abs(x.astype(np.float64)), G.src, G.dst, "sum")
    assert tot.max() < 2.0 ** -125 and (np.abs(x) < 2.0 ** -126).all() and (x != 0).any()
    return x


# ------------------------------------------------------------------------------------------------
# 16-bit stores: one IEEE round-to-nearest-even of the fp32 value; torch's CPU cast is the definition
# ------------------------------------------------------------------------------------------------
def f32_from_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def cast_set(kind):
    """fp32 bit patterns for the fp32 -> fp16 / bf16 cast: every exponent (x 3 mantissas), both neighbours of each rounding tie and
    the ties themselves (odd and even kept bits), the overflow threshold, both subnormal thresholds, +-0, +-inf, NaNs of several
    payloads -- and their negatives.  kind: "fp16" | "bf16"."""
    keep = 10 if kind == "fp16" else 7                  # mantissa bits kept
    drop = 23 - keep
    half = 1 << (drop - 1)
    pats = []
    for e in range(256):
        for m in (0, 0x2AAAAA, 0x7FFFFF):
            pats.append((e << 23) | m)
        for kept in (0, 1, (1 << keep) - 2, (1 << keep) - 1):          # even / odd kept mantissas incl. the carry into the exponent
            base = (e << 23) | (kept << drop)
            pats += [base | (half - 1), base | half, base | (half + 1)]
    if kind == "fp16":
        # overflow threshold 65520 = 0x477FF000 (ties to inf), largest finite 65504; normal threshold 2**-14; subnormal threshold 2**-24,
        # half of it 2**-25 (ties to even: 0), and every fp16 subnormal tie k + 1/2 units for a few k
        thr = [0x477FF000, 0x477FE000, 0x477FEFFF, 0x477FF001, 0x38800000, 0x387FFFFF, 0x38800001, 0x33800000, 0x33000000, 0x33000001,
               0x32FFFFFF, 0x337FFFFF, 0x33800001]
        for k in (1, 2, 3, 511, 512, 1022, 1023):
            v = np.float32((k + 0.5) * 2.0 ** -24)
            b = int(np.asarray(v).view(np.uint32))
            thr += [b - 1, b, b + 1]
        pats += thr
    else:
        pats += [0x7F7F8000, 0x7F7F7FFF, 0x7F7F8001, 0x7F7FFFFF, 0x00800000, 0x007FFFFF, 0x00008000, 0x00007FFF, 0x00008001, 0x00000001,
                 0x00018000, 0x00017FFF, 0x00018001]
    pats += [0x00000000, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF, 0x7F80FFFF, 0x7FA00000, 0x7F808000, 0x7F807FFF]
    p = np.unique(np.asarray(pats, np.uint64) & 0x7FFFFFFF).astype(np.uint32)
    return np.concatenate([p, p | np.uint32(0x80000000)])


def torch_cast_bits(x32, tdt):
    """torch's CPU cast of fp32 values to a 16-bit type -> (uint16 bit patterns, NaN mask)."""
    t = torch.from_numpy(np.ascontiguousarray(x32)).to(tdt)
    return t.view(torch.int16).numpy().view(np.uint16).copy(), torch.isnan(t).numpy()


def trunc16(v32, tdt):
    """fp32 values rounded TOWARD ZERO to the 16-bit type tdt (as fp32 again): always finite for finite input."""
    v32 = np.asarray(v32, np.float32)
    if tdt == torch.bfloat16:
        return (v32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    with np.errstate(over="ignore"):
        h = v32.astype(np.float16)
    h = np.where(np.abs(h.astype(np.float64)) > np.abs(v32.astype(np.float64)), np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def split16(x32, tdt, n_terms, scale=1.0):
    """x32 * scale written as a sum of n_terms values of the 16-bit type (successive truncations: disjoint bit fields of one mantissa,
    so EVERY subset sum is exact in fp32, in any order).  -> (terms fp32 [len, n_terms], ok mask: the split is exact and x is a
    non-zero finite number)."""
    x32 = np.asarray(x32, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (x32.astype(np.float64) * scale).astype(np.float32)
        ok = np.isfinite(x32) & (x32 != 0) & np.isfinite(y) & (y.astype(np.float64) == x32.astype(np.float64) * scale)
        r = np.where(ok, y, np.float32(1.0)).astype(np.float64)
        terms = []
        for _ in range(n_terms):
            t = trunc16(r.astype(np.float32), tdt)
            terms.append(t)
            r = r - t.astype(np.float64)
    return np.stack(terms, 1), ok & (r == 0)


def assert_bits_equal(got_bits, want_bits, want_nan, got_nan, what="", zero_sign_free=False):
    """Bit equality, NaN compared as a class (any payload, either sign).  The sign bit counts -- a cast must keep the sign of a zero and
    of a value that underflows to zero -- unless zero_sign_free: where ARITHMETIC produces the zero (0 + -0 in an accumulator that
    starts at +0) the contract leaves its sign open."""
    got_bits, want_bits = np.asarray(got_bits), np.asarray(want_bits)
    mag = (1 << (8 * got_bits.dtype.itemsize - 1)) - 1
    both_zero = ((got_bits & mag) == 0) & ((want_bits & mag) == 0) & bool(zero_sign_free)
    bad = np.where(want_nan | got_nan, want_nan != got_nan, (got_bits != want_bits) & ~both_zero)
    if bad.any():
        i = int(np.argwhere(bad.reshape(-1))[0][0])
        raise AssertionError("%s: element %d: bits 0x%x, the definition's are 0x%x (%s); %d of %d differ"
                             % (what, i, int(got_bits.reshape(-1)[i]), int(want_bits.reshape(-1)[i]),
                                "NaN" if want_nan.reshape(-1)[i] else "a number", int(bad.sum()), bad.size))


# ------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------
def softmax_def(x, ids, n_seg):
    """torch.softmax per segment and column in fp64 on the stored values (grad_defs.segment_softmax is the same formula):
    exp(x - max) / sum, IEEE: a -inf logit weighs 0; a segment of only -inf, or one with +inf or NaN, is NaN throughout."""
    x64 = torch.as_tensor(as_f64(x))
    flat = x64.reshape(x64.shape[0], -1)
    ids_t = torch.as_tensor(np.asarray(ids), dtype=torch.int64)
    out = torch.empty_like(flat)
    for s in range(int(n_seg)):
        sel = ids_t == s
        if bool(sel.any()):
            out[sel] = torch.softmax(flat[sel], 0)
    return out.reshape(x64.shape).numpy()


def softmax_bound(x, ids, n_seg, want64, eps=EPS32, K=K_FAMILY["softmax"]):
    """Per element: K x the re-association bound of p * (1 + |x - max|) over the segment's length + 3 terms -- the terms and the count
    of grad_defs.segment_softmax_terms, K the softmax family's factor (grad_defs.K_FAMILY).  An element of weight exactly 0 (a -inf
    logit, or exp(-6e38)) has bound 0."""
    x64 = as_f64(x).reshape(len(ids), -1)
    w = np.asarray(want64, np.float64).reshape(len(ids), -1)
    ids = np.asarray(ids, np.int64)
    mx = np.full((int(n_seg), x64.shape[1]), -np.inf)
    np.fmax.at(mx, ids, x64)
    n = np.bincount(ids, minlength=int(n_seg))[ids].astype(np.float64)[:, None] + 3.0
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.where(w == 0, 0.0, w * (1.0 + np.abs(x64 - mx[ids])))
    return (K * rebound(terms, n, eps)).reshape(np.shape(want64))


def softmax_segments(d, seed=3):
    """-> (x fp32 [n, d], ids int64 sorted, n_seg, names): one segment per case, with an ordinary neighbour on either side of each."""
    rng = np.random.default_rng(seed)
    segs, names = [], []

    def add(name, a):
        segs.append(rng.standard_normal((40, d)).astype(np.float32)); names.append("neighbour")
        segs.append(np.asarray(a, np.float32)); names.append(name)

    base = lambda L: (rng.standard_normal((L, d)) * 3).astype(np.float32)
    for name, pos in (("ninf_first", 0), ("ninf_mid", 35), ("ninf_last", 69)):
        a = base(70); a[pos] = -INF; add(name, a)
    a = base(30000); a[:300] = -INF; add("ninf_first_300_of_30000", a)
    a = base(30000); a[15000:15400] = -INF; a[-1] = -INF; add("ninf_mid_chunks_of_30000", a)
    add("all_ninf", np.full((50, d), -INF))
    add("all_ninf_700", np.full((700, d), -INF))
    a = base(70); a[10] = INF; add("one_pinf", a)
    a = base(70); a[20] = NAN; add("one_nan", a)
    a = base(600); a[599] = NAN; add("nan_last_of_600", a)
    a = np.full((64, d), -3e38); a[::2] = 3e38; add("pm_3e38", a)
    add("all_3e38", np.full((256, d), 3e38))
    a = base(1); a[0] = -INF; add("single_ninf", a)
    segs.append(rng.standard_normal((40, d)).astype(np.float32)); names.append("neighbour")
    ids = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(segs)])
    return np.concatenate(segs), ids, len(segs), names
