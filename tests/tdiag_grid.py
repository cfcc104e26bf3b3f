"""The compiled variants of the per-feature-coefficient layer's kernels (csrc/basis_tdiag.hip) and the cases that reach
every one of them, every loop of theirs beyond its first trip, and every boundary of their dispatch.

k_tdiag_rows and k_tdiag_dp are compiled for VEC in {4, 1} x TPR in {64, 128, 256}, k_tdiag_dcoef and k_tdiag_dh_join
for VEC in {4, 1}.  With nvec = d / VEC column vectors:
  * a short row is walked by TPR lanes, `cidx += TPR`: lane_trips(d) = ceil(nvec / TPR) trips (a second one only at
    nvec > 256);
  * a long row (more than LONG_ROW slots) by a whole workgroup, 8 slot-lanes x 128 column lanes, `c0 += 128`:
    column_passes(d) = ceil(nvec / 128) passes over one LDS reduction buffer -- in k_tdiag_dp with two LDS round trips
    per live basis function inside every pass;
  * the source-major kernel runs B basis functions in basis_passes(B) launches of BT = 8, the last one with nbt of them;
  * a workgroup of the coefficient gradient walks the B d entries of its slab row in dcoef_trips(B, d) trips of 256 VEC;
  * the dH epilogue is a grid-stride loop over V d / VEC vectors on at most 8192 x 256 threads: join_trips(V, d);
  * long rows are shared among long_blocks(E) workgroups, relations cut into chunks of chunk_of(E, max_edges) messages
    (onehot_grid's mirrors: basis_tdiag.hip repeats basis_onehot.hip's long_blocks, the chunks are graph_prep.hip's);
  * dW_dir = H^T dP_dir is split over V in dw_split(V, d, B) slabs: auto_split_k's figure, capped at the 16 the context
    allocates.
The functions below mirror those formulas on the host, so that a test can state which cell a case reaches; TDIAG_GRID is
one case per cell and per boundary, each with hub rows that take the long-row path at chosen slot counts;
STRUCTURE_CASES vary the graph instead of the width; LARGE_CASES are the two shapes at which the dH epilogue takes a
second trip.  tests/test_tdiag_grid.py keeps the tables honest without a GPU; tests/test_gpu_tdiag_grid.py runs them.
"""
import numpy as np

import times_diag_reference as tdr
from kernel_grid import BASIS_BT, LONG_ROW, grid_triples, row_slots  # noqa: F401  (re-exported to the tests)
from onehot_grid import (CHUNK_EDGE_COUNTS, HUBS, chunk_of, lane_slots, long_blocks, stale_graphs,  # noqa: F401
                         structure_triples)

VECS = (4, 1)
TPRS = (64, 128, 256)
COLUMN_LANES = 128          # basis_tdiag.hip: red[8][128 * VEC], `c0 += 128`
DCOEF_THREADS = 256         # k_tdiag_dcoef: `e += 256 * VEC`
JOIN_THREADS = 8192 * 256   # tdiag_dh_join: at most 8192 workgroups of 256 threads
DW_SLABS = 16               # rgcn_api.hip / rgcn_schedule.hip: split-K slabs of gemm_tdiag_dw


# ----------------------------------------------------------------------------- host mirrors
def vec_tpr(d):
    """basis_tdiag.hip (tdiag_rows_forward, tdiag_dp): float4 columns when d % 4 == 0 (the engine's buffers are 16-byte
    aligned), then 64 / 128 / 256 lanes per short row for up to 64 / 128 / more column vectors."""
    vec = 4 if d % 4 == 0 else 1
    nvec = d // vec
    return vec, (64 if nvec <= 64 else (128 if nvec <= 128 else 256))


def nvec_of(d):
    return d // vec_tpr(d)[0]


def column_passes(d):
    """k_tdiag_rows / k_tdiag_dp: passes of the long-row column loop `for (int c0 = 0; c0 < nvec; c0 += 128)`"""
    return -(-nvec_of(d) // COLUMN_LANES)


def lane_trips(d):
    """k_tdiag_rows / k_tdiag_dp: trips of the short-row lane loop `for (int cidx = lane; cidx < nvec; cidx += TPR)`"""
    return -(-nvec_of(d) // vec_tpr(d)[1])


def basis_passes(B):
    """tdiag_dp: (launches of k_tdiag_dp, `for (int b0 = 0; b0 < c->B; b0 += BT)`; nbt of the last one)"""
    n = -(-B // BASIS_BT)
    return n, B - BASIS_BT * (n - 1)


def dcoef_trips(B, d):
    """k_tdiag_dcoef: trips of `for (int e = threadIdx.x * VEC; e < Bd; e += 256 * VEC)` of thread 0"""
    return -(-(B * d) // (DCOEF_THREADS * vec_tpr(d)[0]))


def join_trips(V, d):
    """tdiag_dh_join / k_tdiag_dh_join: trips of the grid-stride loop of thread 0 (grid capped at 8192 workgroups)"""
    nvec = V * d // vec_tpr(d)[0]
    threads = min(-(-nvec // 256), 8192) * 256
    return -(-nvec // threads)


def auto_split_k(M, N, K, narrow=False):
    """rgcn_api.hip (auto_split_k)"""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 192:
        return 1
    s = ((256 if narrow else 512) + tiles - 1) // tiles
    return max(1, min(s, (K + 127) // 128, 64))


def dw_split(V, d, B):
    """rgcn_schedule.hip (bwd_layer_partial, RGCN_KIND_BASIS_TDIAG): (what auto_split_k asks for, what gemm_tdiag_dw gets)"""
    asked = auto_split_k(d, 2 * B * d, V, True)
    return asked, min(asked, DW_SLABS)


def cell_of(case):
    """(VEC, TPR, column passes, lane trips, basis passes, nbt of the last basis pass, dcoef trips)"""
    vec, tpr = vec_tpr(case["d"])
    bp, nbt = basis_passes(case["B"])
    return vec, tpr, column_passes(case["d"]), lane_trips(case["d"]), bp, nbt, dcoef_trips(case["B"], case["d"])


# ----------------------------------------------------------------------------- the width table
# Every case: V 300, R 237, E 3000 random triples among the vertices >= 4, then vertex h given exactly HUBS[h] = 32, 33,
# 51, 400 slots (kernel_grid.grid_triples; onehot_grid.py says what each count does to the 8 slot-lanes).  R = 237 keeps
# nearly every (relation, vertex) run at length 1, so under local norms the 400-slot hub's sum is not damped: the cases
# run with L = 2 under intended norms and as the top layer (L = 1) under local ones, as the one-hot grid's do.
V_GRID, R_GRID, E_GRID = 300, 237, 3000


def _case(d, B):
    return dict(name="tdiag_d%d_B%d" % (d, B), V=V_GRID, R=R_GRID, d=d, B=B, E=E_GRID, hubs=HUBS, seed=5000 + d + B)


TDIAG_GRID_LIST = [
    _case(20, 8),           # (4, 64): exactly one full tile of basis functions
    _case(516, 9),          # (4, 256): nvec 129, the second column pass has one live lane; second B-tile (nbt 1) on it
    _case(1028, 2),         # (4, 256): nvec 257, two lane trips, three column passes
    _case(9, 8),            # (1, 64)
    _case(129, 17),         # (1, 256): nvec 129, two column passes under three B-tiles (nbt 1)
    _case(301, 9),          # (1, 256): two lane trips, three column passes, second B-tile (nbt 1) on them
    # the dispatch boundaries nvec 64 | 65, 128 | 129 of each VEC (VEC 4: d = 4 nvec; VEC 1: 64 and 128 are multiples of
    # 4, so the last width below each boundary is 63 and 127).  d = 516 and d = 129 above are the nvec 129 of each VEC.
    _case(256, 1), _case(260, 2), _case(512, 3),
    _case(63, 1), _case(65, 2), _case(127, 3),
]
TDIAG_GRID = {c["name"]: c for c in TDIAG_GRID_LIST}
BOUNDARY_NVECS = (64, 65, 128, 129)
BOUNDARY_WIDTHS = {4: (256, 260, 512, 516), 1: (63, 65, 127, 129)}
WIDEST = {4: "tdiag_d1028_B2", 1: "tdiag_d301_B9"}      # generated dropout: drop_factor's index at the largest offsets
THREE_PASSES = "tdiag_d301_B9"                          # determinism: a three-column-pass case

# H_1 of tdiag_d129_B17 as the top layer under local norms: the 400-slot hub adds 400 x 17 undamped products per column
# (|H_1| reaches 161, where 1e-4 is 6e-7 relative), and a plain float32 evaluation of the restatement (numpy float32, one summation order)
# is already 1.587e-04 from float64 on that case's inputs -- every other case, layer and buffer of every table holds
# FWD_ATOL = 1e-4 in float32 (5.2e-05 at most).  Four times the measured figure, for H_1 of that one case in that one
# run; tests/test_tdiag_grid.py asserts that float32 stays within the figure.
LOCAL_D129_B17_H1_F32 = 1.587e-04
LOCAL_D129_B17_H1_ATOL = 4 * LOCAL_D129_B17_H1_F32


def forward_atol(name, norm, L, buf, l, default=1e-4):
    """the absolute bound of buffer `buf` ('H' | 'P') of layer l of a run of case `name`"""
    return LOCAL_D129_B17_H1_ATOL if (name, norm, L, buf, l) == ("tdiag_d129_B17", "local", 1, "H", 1) else default

# ----------------------------------------------------------------------------- graphs that vary the structure, d = 20
STRUCTURE_CASES = {
    # more long rows than long-row workgroups: the `lb += n_long_blocks` loop
    "many_long_rows": dict(name="many_long_rows", V=300, R=7, d=20, B=9, E=8000, seed=4001),
    # 2 E > 65536: 512 long-row workgroups and relation chunks of 96
    "capacity_switch": dict(name="capacity_switch", V=300, R=7, d=20, B=3, E=33000, seed=4002),
    # relations whose messages fill exactly one chunk, one chunk plus one, none, one message, two chunks, two plus one
    "chunk_edges": dict(name="chunk_edges", V=300, R=8, d=20, B=9, E=3000, seed=4003),
}

# ----------------------------------------------------------------------------- the dH epilogue's second trip
# V d / VEC just past 8192 x 256 = 2,097,152 threads, with the least memory: one layer, one basis function, few edges.
# At d = 257 the weight-gradient GEMM (M = 257, N = 2 x 257: 15 tiles) is also asked to split V into 18 slabs, more
# than the 16 the context allocates: the cap of rgcn_schedule.hip applies.
LARGE_CASES = {
    "large_vec1": dict(name="large_vec1", V=8200, R=7, d=257, B=1, E=2000, seed=6001, L=1, dw_split=(18, 16)),
    "large_vec4": dict(name="large_vec4", V=32300, R=7, d=260, B=1, E=2000, seed=6002, L=1, dw_split=(18, 16)),
}
ALL_CASES = dict(TDIAG_GRID, **STRUCTURE_CASES, **LARGE_CASES)


def case_triples(case):
    return grid_triples(case) if "hubs" in case else structure_triples(case)


def case_inputs(case, L):
    """times_diag_reference.make_case's weights, masks and upstream gradient for L layers on the case's own graph"""
    c = tdr.make_case(case["V"], case["R"], case["d"], L, case["B"], case_triples(case), seed=case["seed"])
    c["name"] = case["name"]
    return c


STALE_TABLE = "tdiag_d20_B8"      # the case whose coefficients change between two forward passes


def second_coefficients(params, L, seed=4200):
    """the same weights with other C_f / C_b in every layer: the sigmoid table of the first ones is stale"""
    rng = np.random.RandomState(seed)
    p = dict(params)
    for l in range(1, L + 1):
        for n in ("C_f%d" % l, "C_b%d" % l):
            p[n] = rng.normal(0, 1, size=params[n].shape).astype(np.float32)
    return p


def stale_case(B=17, d=20, L=2):
    """(case on the first graph of onehot_grid.stale_graphs, second graph, quiet vertices)"""
    first, second, quiet = stale_graphs()
    c = tdr.make_case(300, 7, d, L, B, first, seed=4100)
    c["name"] = "stale_dP"
    return c, second, quiet
