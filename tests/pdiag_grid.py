"""The compiled variants of the per-relation-diagonal layer's kernels (csrc/basis_pdiag.hip) and the cases that reach
every one of them, every loop of theirs beyond its first trip, and every boundary of their dispatch.

k_pdiag_rows and k_pdiag_dh_join are compiled for VEC in {4, 1} x TPR in {64, 128, 256}; k_pdiag_epilogue,
k_pdiag_row_bwd and k_pdiag_ddiag for VEC in {4, 1}; k_pdiag_dcoef and k_pdiag_ddiag_reduce once.  With nvec = d / VEC
column vectors:
  * a short row is walked by TPR lanes, `cidx += TPR`: lane_trips(d) = ceil(nvec / TPR) trips (a second one only at
    nvec > 256); its 2 B mixing scalars by the same lanes, `j += TPR`: mix_trips(B, d) (a second one at 2 B > TPR);
  * a long row (more than LONG_ROW slots) by a whole workgroup, 8 slot-lanes x 128 column lanes: the 2 B <= 128 mixing
    scalars in one LDS reduction, then `c0 += 128`: column_passes(d) = ceil(nvec / 128) passes;
  * the epilogue and the row-local backward kernel give a row one wave, `cidx += 64`: wave_trips(d) = ceil(nvec / 64);
  * a workgroup of the diagonal tables' gradient walks the d entries of its slab row in ddiag_trips(d) trips of 256 VEC;
    the coefficient gradient gives basis function b of a chunk lane b of one wave (B <= 64);
  * long rows are shared among long_blocks(E) workgroups, relations cut into chunks of chunk_of(E, max_edges) messages
    (onehot_grid's mirrors: basis_pdiag.hip repeats basis.hip's long_blocks, the chunks are graph_prep.hip's).
The dense products are the basis kind's and are covered by its own tables.  The functions below mirror those formulas on
the host, so that a test can state which cell a case reaches; PDIAG_GRID is one case per cell and per boundary, each with
hub rows that take the long-row path at chosen slot counts; STRUCTURE_CASES vary the graph instead of the width.
tests/test_pdiag_grid.py keeps the tables honest without a GPU; tests/test_gpu_pdiag_grid.py runs them.
"""
import add_diagonal_reference as adr
from kernel_grid import LONG_ROW, grid_triples, row_slots  # noqa: F401  (re-exported to the tests)
from onehot_grid import CHUNK_EDGE_COUNTS, HUBS, chunk_of, lane_slots, long_blocks, structure_triples  # noqa: F401

VECS = (4, 1)
TPRS = (64, 128, 256)
COLUMN_LANES = 128          # basis_pdiag.hip: red[8][128 * VEC], `c0 += 128`
MIX_LANES = 128             # kMixLanes: 2 B <= 128
WAVE = 64                   # k_pdiag_epilogue / k_pdiag_row_bwd: `cidx += 64`
DDIAG_THREADS = 256         # k_pdiag_ddiag: `e += 256 * VEC`


# ----------------------------------------------------------------------------- host mirrors
def vec_tpr(d):
    """basis_pdiag.hip (row_lanes; pdiag_rows_forward, pdiag_dh_join): float4 columns when d % 4 == 0 (the engine's buffers
    are 16-byte aligned), then 64 / 128 / 256 lanes per short row for up to 64 / 128 / more column vectors."""
    vec = 4 if d % 4 == 0 else 1
    nvec = d // vec
    return vec, (64 if nvec <= 64 else (128 if nvec <= 128 else 256))


def nvec_of(d):
    return d // vec_tpr(d)[0]


def column_passes(d):
    """k_pdiag_rows / k_pdiag_dh_join: passes of the long-row column loop `for (int c0 = 0; c0 < nvec; c0 += 128)`"""
    return -(-nvec_of(d) // COLUMN_LANES)


def lane_trips(d):
    """k_pdiag_rows / k_pdiag_dh_join: trips of the short-row lane loop `for (int cidx = lane; cidx < nvec; cidx += TPR)`"""
    return -(-nvec_of(d) // vec_tpr(d)[1])


def mix_trips(B, d):
    """k_pdiag_rows: trips of lane 0 in the short-row loop `for (int j = lane; j < nmix; j += TPR)`"""
    return -(-2 * B // vec_tpr(d)[1])


def wave_trips(d):
    """k_pdiag_epilogue / k_pdiag_row_bwd: trips of `for (int cidx = lane; cidx < nvec; cidx += 64)`"""
    return -(-nvec_of(d) // WAVE)


def ddiag_trips(d):
    """k_pdiag_ddiag: trips of `for (int e = threadIdx.x * VEC; e < a.d; e += 256 * VEC)` of thread 0"""
    return -(-d // (DDIAG_THREADS * vec_tpr(d)[0]))


def cell_of(case):
    """(VEC, TPR, column passes, lane trips, mixing trips, wave trips, ddiag trips)"""
    vec, tpr = vec_tpr(case["d"])
    d, B = case["d"], case["B"]
    return vec, tpr, column_passes(d), lane_trips(d), mix_trips(B, d), wave_trips(d), ddiag_trips(d)


# ----------------------------------------------------------------------------- the width table
# Every case: V 300, R 237, E 3000 random triples among the vertices >= 4, then vertex h given exactly HUBS[h] = 32, 33,
# 51, 400 slots (kernel_grid.grid_triples; onehot_grid.py says what each count does to the 8 slot-lanes).  The cases run
# with L = 2 under intended norms and as the top layer (L = 1) under local ones, as the times-diag grid's do.
V_GRID, R_GRID, E_GRID = 300, 237, 3000


def _case(d, B):
    return dict(name="pdiag_d%d_B%d" % (d, B), V=V_GRID, R=R_GRID, d=d, B=B, E=E_GRID, hubs=HUBS, seed=7000 + d + B)


PDIAG_GRID_LIST = [
    _case(20, 8),           # (4, 64): B at the basis kernels' eight-function tile
    _case(516, 9),          # (4, 256): nvec 129, the second column pass has one live lane; three wave trips
    _case(1028, 2),         # (4, 256): nvec 257, two lane trips, three column passes, two ddiag trips
    _case(9, 8),            # (1, 64)
    _case(129, 17),         # (1, 256): nvec 129, two column passes
    _case(301, 9),          # (1, 256): two lane trips, three column passes, two ddiag trips
    # the dispatch boundaries nvec 64 | 65, 128 | 129 of each VEC (VEC 4: d = 4 nvec; VEC 1: 64 and 128 are multiples of
    # 4, so the last width below each boundary is 63 and 127).  d = 516 and d = 129 above are the nvec 129 of each VEC.
    _case(256, 1), _case(260, 2), _case(512, 3),
    _case(63, 1), _case(65, 2), _case(127, 3),
    # the mixing scalars: 2 B = 64 | 66 on 64 lanes (a second trip of `j += TPR`), 2 B = 128 (every mixing lane of a long row)
    _case(12, 32), _case(10, 33), _case(8, 64),
]
PDIAG_GRID = {c["name"]: c for c in PDIAG_GRID_LIST}
BOUNDARY_NVECS = (64, 65, 128, 129)
BOUNDARY_WIDTHS = {4: (256, 260, 512, 516), 1: (63, 65, 127, 129)}
WIDEST = {4: "pdiag_d1028_B2", 1: "pdiag_d301_B9"}      # generated dropout: drop_factor's index at the largest offsets
THREE_PASSES = "pdiag_d301_B9"                          # determinism: a three-column-pass case

# ----------------------------------------------------------------------------- graphs that vary the structure, d = 20
STRUCTURE_CASES = {
    # more long rows than long-row workgroups: the `lb += n_long_blocks` loop
    "many_long_rows": dict(name="many_long_rows", V=300, R=7, d=20, B=9, E=8000, seed=4001),
    # 2 E > 65536: 512 long-row workgroups and relation chunks of 96
    "capacity_switch": dict(name="capacity_switch", V=300, R=7, d=20, B=3, E=33000, seed=4002),
    # relations whose messages fill exactly one chunk, one chunk plus one, none, one message, two chunks, two plus one
    "chunk_edges": dict(name="chunk_edges", V=300, R=8, d=20, B=9, E=3000, seed=4003),
}
ALL_CASES = dict(PDIAG_GRID, **STRUCTURE_CASES)


def case_triples(case):
    return grid_triples(case) if "hubs" in case else structure_triples(case)


def case_inputs(case, L):
    """add_diagonal_reference.make_case's weights, masks and upstream gradient for L layers on the case's own graph"""
    c = adr.make_case(case["V"], case["R"], case["d"], L, case["B"], case_triples(case), seed=case["seed"])
    c["name"] = case["name"]
    return c
