"""The graphs the host and GPU tests of the sliced aggregation share (ops.slice_plan + pglamd_aggregate_sliced), the inputs whose sums
are exact in fp32, and what a slice plan says about the branches a launch over it enters.  numpy only; tests/test_hub_slice_defs.py
proves every property claimed here on the CPU, so the GPU tests' preconditions hold before a GPU is touched.

Every graph has N = 8192 nodes: hub_plan needs K = n // 8 >= 1024 hub rows, so this is the smallest graph a slice plan exists for.
Sources 0 .. 1023 are the hubs and carry the highest out-degrees in non-increasing order of id, so hub rank == source id and
slice s holds the hubs with id % 8 == s.  Builders return (n, src, dst) as int64 arrays in a random edge order."""
import numpy as np

N = 8192
HUBS = 1024
SLICES = 8
FIX_SHORT = 16                # csrc/split_rows.hpp kFixShort: a split row with more further pieces than this takes the long role
MIN_ROWS = 64                 # ops._SLICE_MIN_ROWS


def _shuffled(src, dst, seed):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    perm = np.random.default_rng(seed).permutation(len(src))
    return N, src[perm], dst[perm]


def all_hub(rows=64):
    """Every hub sends one edge to each of rows 4096 .. 4096 + rows - 1: E = 1024 * rows, `rows` rows of 1024 hub edges, no other
    edge -- the rest stream is empty and every slice holds 128 * rows edges; 8192 - rows real rows receive nothing."""
    src = np.tile(np.arange(HUBS), rows)
    dst = np.repeat(4096 + np.arange(rows), HUBS)
    return _shuffled(src, dst, 21)


def one_slice(s=3):
    """Every hub has 24 out-edges.  The 128 hubs with id % 8 == s feed rows 2000 .. 2063 (48 hub edges each, nothing else); the
    other hubs feed rows 4000 .. 6999 (7 or 8 edges each).  E = 24576; at row_min = 32 only slice s has edges, so 7 * 64 virtual
    rows are empty."""
    mine = np.repeat(np.array([i for i in range(HUBS) if i % SLICES == s]), 24)
    rest = np.repeat(np.array([i for i in range(HUBS) if i % SLICES != s]), 24)
    src = np.concatenate([mine, rest])
    dst = np.concatenate([2000 + np.arange(len(mine)) % 64, 4000 + np.arange(len(rest)) % 3000])
    return _shuffled(src, dst, 22 + s)


def tiny():
    """64 rows (4096 .. 4159) of 33 hub edges each and nothing else, E = 2112: hubs 0 .. 63 have three out-edges, hubs 64 .. 1023
    two, so every slice holds exactly 264 edges.  At chunk 256 the stream has 3 blocks of 1024 edges: fewer blocks than XCDs,
    slices that own no block, and every segment boundary inside a block."""
    src = np.concatenate([np.repeat(np.arange(HUBS), 2), np.arange(64)])
    dst = 4096 + np.arange(len(src)) % 64
    return _shuffled(src, dst, 23)


def hand_graph():
    """8192 nodes; sources 0..1023 all have 24 out-edges (more than any other source), so hub rank == source id.
    rows 2100..2199: ~210 hub edges + 10 cold edges each            row 2010: hub edges only (its rest row is empty)
    row 2011: 50 cold edges (eight empty virtual rows)                row 2012: exactly L edges, row 2013: L + 1
    hubs with id % 8 == 7 send to short rows only (slice 7 has no edge); duplicate edges, self loops and rows without edges."""
    src, dst, rng = _hand_edges()
    perm = rng.permutation(len(src))
    return N, src[perm], dst[perm]


def _hand_edges():
    n = N
    rng = np.random.default_rng(5)
    slots = np.repeat(np.array([i for i in range(1024) if i % 8 != 7]), 24)      # hub id of every hub -> long-row edge
    dst = np.empty(len(slots), np.int64)
    dst[:16] = 2012; dst[16:33] = 2013; dst[33:83] = 2010                        # (16 / 17 parallel edges from hub 0: duplicates)
    dst[83:] = 2100 + np.arange(len(slots) - 83) % 100
    src, dsts = [slots], [dst]
    h7 = np.repeat(np.array([i for i in range(1024) if i % 8 == 7]), 24)
    src.append(h7); dsts.append(4000 + np.arange(len(h7)) % 3000)
    cold = lambda k: rng.integers(1024, n, k)
    for r, k in [(2011, 50), (2012, 16), (2013, 16)] + [(r, 10) for r in range(2100, 2200)]:
        src.append(cold(k)); dsts.append(np.full(k, r))
    loops = np.array([2150, 3000, 3001, 3002, 3002])                             # self loops: one on a long row, one doubled
    src.append(loops); dsts.append(loops)
    return np.concatenate(src).astype(np.int64), np.concatenate(dsts).astype(np.int64), rng


MIXED_COLD_ROW = 2300          # mixed_long: 3000 cold + 200 hub edges
MIXED_ONE_RESIDUE_ROW = 2301   # mixed_long: 256 hub edges, all of residue MIXED_RESIDUE
MIXED_RESIDUE = 2


def mixed_long():
    """hand_graph's edges, plus two more out-edges per hub (26 each, so rank == id still holds):
    row 2300: 3000 cold edges and 200 hub edges of residues other than 2 -- its remainder row is itself split over many chunks;
    row 2301: both extra edges of the 128 hubs with id % 8 == 2 and nothing else -- one virtual row of 256 edges (more than
              17 chunks of 8: the long fix-up role), seven empty ones and an empty remainder;
    the other 1592 extra hub edges go to rows 7000 .. 7999 (one or two each: short rows)."""
    src, dst, _ = _hand_edges()
    rng = np.random.default_rng(7)
    two = np.repeat(np.array([i for i in range(HUBS) if i % SLICES == MIXED_RESIDUE]), 2)
    others = rng.permutation(np.repeat(np.array([i for i in range(HUBS) if i % SLICES != MIXED_RESIDUE]), 2))
    o_dst = np.concatenate([np.full(200, MIXED_COLD_ROW), 7000 + np.arange(len(others) - 200) % 1000])
    cold = rng.integers(HUBS, N, 3000)
    src = np.concatenate([src, two, others, cold])
    dst = np.concatenate([dst, np.full(len(two), MIXED_ONE_RESIDUE_ROW), o_dst, np.full(3000, MIXED_COLD_ROW)])
    return _shuffled(src, dst, 8)


BUILDERS = {"all_hub": all_hub, "one_slice3": one_slice, "one_slice6": lambda: one_slice(6), "tiny": tiny, "mixed_long": mixed_long,
            "hand_graph": hand_graph}


def rmat14():
    """RMAT scale 14 with 400 k edges from the CPU generator (the same edges on every machine): 16384 nodes, 1751 rows longer than
    32 edges and 470 longer than 128 (the benchmark's configuration at 1/50 of the edges), the longest of 8650.  Hub rank is NOT
    the source id here."""
    import torch
    from pgl_amd.utils.rmat import rmat_edges
    e = rmat_edges(14, 400_000, seed=3, device=torch.device("cpu")).numpy()
    return 1 << 14, np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])


def small_int_features(n, d, seed):
    """fp32 [n, d] with integer values in [-8, 8]: a sum of k of them is an integer of magnitude <= 8 k, so for k < 2^21 every
    partial sum in any association is exact in fp32 (and in fp64) and every correct kernel returns the same bits."""
    return np.random.default_rng(seed).integers(-8, 9, (n, d)).astype(np.float32)


def exact_sum(x, src, dst, out_rows):
    """The fp64 sum of x[src] over dst, cast to fp32 (exact for small_int_features while max degree * 8 < 2^24)."""
    assert int(np.bincount(dst).max()) * 8 < (1 << 24)
    out = np.zeros((out_rows, x.shape[1]), np.float64)
    np.add.at(out, dst, x.astype(np.float64)[src])
    return out.astype(np.float32)


def cpu_csr(ops, n, src, dst):
    """The destination-sorted index of (src, dst) as an ops.CSR over CPU tensors (what csr_build makes on the device)."""
    import torch
    order = np.argsort(dst, kind="stable")
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=indptr[1:])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    return ops.CSR(t(indptr, torch.int64), t(dst[order], torch.int32), t(src[order], torch.int32), t(order, torch.int32), n, len(src))


def plan_facts(plan):
    """What a launch over `plan` enters, from the plan alone (numpy on its indptr):
    virtual_chunks / rest_chunks: the most chunks one virtual / one real row is cut into (a row of <= chunk edges is never cut; a
        longer one is cut on the chunk grid, so it has pieces in chunks first_edge // chunk .. last_edge // chunk);
    virtual_long / virtual_short: how many virtual rows are cut into more than FIX_SHORT + 1 pieces (fixup_tasks LONG) / into
        2 .. FIX_SHORT + 1 pieces (the short role);  rest_long / rest_short: the same for the real rows;
    empty_virtual: virtual rows without an edge (zero-filled behind the partial rows);
    blocks_per_segment: block counts of the rest stream and of the eight slices."""
    ip = np.asarray(plan.indptr.cpu().numpy(), np.int64)
    lo, hi = ip[:-1], ip[1:]
    length = hi - lo
    pieces = np.where(length > plan.chunk, (hi - 1) // plan.chunk - lo // plan.chunk + 1, np.minimum(length, 1))
    virt, rest = pieces[plan.out_rows:], pieces[:plan.out_rows]
    assert len(virt) == SLICES * plan.n_long
    f = lambda p: (int((p > FIX_SHORT + 1).sum()), int(((p >= 2) & (p <= FIX_SHORT + 1)).sum()))
    return dict(virtual_chunks=int(virt.max()), rest_chunks=int(rest.max()), virtual_long=f(virt)[0], virtual_short=f(virt)[1],
                rest_long=f(rest)[0], rest_short=f(rest)[1], empty_virtual=int((length[plan.out_rows:] == 0).sum()),
                blocks_per_segment=list(plan.blocks[SLICES + 1:]))


def slice_block(tab, b):
    """csrc/common.hpp slice_block restated: grid block b -> logical block of the stream, or -1 for a surplus block.  A guard for
    the TABLES slice_plan emits (does the grid the launch sizes from them reach every block once?), not a test of the device
    function, which only runs on the GPU."""
    x, j = b % SLICES, b // SLICES
    n_rest = tab[SLICES + 1]
    r_lo = n_rest * x // SLICES
    nr = n_rest * (x + 1) // SLICES - r_lo
    ns, s_lo = tab[SLICES + 2 + x], tab[1 + x]
    total = nr + ns
    if j >= total:
        return -1
    a = j * ns // total
    return s_lo + a if (j + 1) * ns // total > a else r_lo + (j - a)


def slice_blocks_per_xcd(tab):
    n_rest = tab[SLICES + 1]
    return max(n_rest * (x + 1) // SLICES - n_rest * x // SLICES + tab[SLICES + 2 + x] for x in range(SLICES))
