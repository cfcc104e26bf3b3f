"""The compiled variants of the featureless first layer's kernels (csrc/basis_onehot.hip) and the cases that reach every
one of them, every loop of theirs beyond its first trip, and every boundary of their dispatch.

k_onehot_fwd and k_onehot_tables are compiled for VEC in {4, 1} x TPR in {64, 128, 256}, k_onehot_dcoef for VEC in {4, 1}.
With nvec = d / VEC column vectors:
  * a short row is walked by TPR lanes, `cidx += TPR`: lane_trips(d) = ceil(nvec / TPR) trips (a second one only at
    nvec > 256);
  * a long row (more than LONG_ROW slots) by a whole workgroup, 8 slot-lanes x 128 column lanes, `c0 += 128`:
    column_passes(d) = ceil(nvec / 128) passes over one LDS reduction buffer;
  * the table gradient runs B basis functions in basis_passes(B) launches of BT = 8, the last one with nbt = B - 8 (passes
    - 1) of them live;
  * long rows are shared among long_blocks(E) workgroups (64, or 512 once 2 E > 65536), `lb += n_long_blocks`;
  * the coefficient gradient takes one workgroup per chunk_of(E, max_edges) messages of one directed relation.
The functions below mirror those formulas on the host, so that a test can state which cell a case reaches; ONEHOT_GRID is
one case per cell and per boundary, each with hub rows that take the long-row path at chosen slot counts;
STRUCTURE_CASES vary the graph instead of the width.  tests/test_onehot_grid.py keeps the table honest without a GPU;
tests/test_gpu_onehot_grid.py runs it.
"""
import numpy as np

import featureless_reference as fr
from kernel_grid import BASIS_BT, LONG_ROW, grid_triples, row_slots  # noqa: F401  (re-exported to the tests)

VECS = (4, 1)
TPRS = (64, 128, 256)
COLUMN_LANES = 128          # basis_onehot.hip: red[8][128 * VEC], `c0 += 128`
SLOT_LANES = 8              # ... and the 8 slot-lanes of a long-row workgroup (stride of lookup_range / tables_range)


# ----------------------------------------------------------------------------- host mirrors
def onehot_vec_tpr(d):
    """basis_onehot.hip (onehot_forward, onehot_backward_tables): float4 columns when d % 4 == 0 (the engine's buffers
    are 16-byte aligned), then 64 / 128 / 256 lanes per short row for up to 64 / 128 / more column vectors."""
    vec = 4 if d % 4 == 0 else 1
    nvec = d // vec
    return vec, (64 if nvec <= 64 else (128 if nvec <= 128 else 256))


def nvec_of(d):
    return d // onehot_vec_tpr(d)[0]


def column_passes(d):
    """passes of the long-row column loop `for (int c0 = 0; c0 < nvec; c0 += 128)`"""
    return -(-nvec_of(d) // COLUMN_LANES)


def lane_trips(d):
    """trips of the short-row lane loop `for (int cidx = lane; cidx < nvec; cidx += TPR)`"""
    return -(-nvec_of(d) // onehot_vec_tpr(d)[1])


def basis_passes(B):
    """launches of k_onehot_tables (`for (int b0 = 0; b0 < c->B; b0 += BT)`), also k_onehot_dcoef's inner passes"""
    return -(-B // BASIS_BT)


def long_blocks(E):
    """basis_onehot.hip (long_blocks): workgroups that share the long rows of a graph of E edges"""
    return 512 if 2 * E > 65536 else 64


def chunk_of(E, max_edges):
    """graph_prep.hip (graph_build) under rgcn_api.hip's capacity bound: messages per relation chunk of a graph of E edges
    on a context created for max_edges"""
    cap = 48 * ((2 * max_edges + 65535) // 65536) if 2 * max_edges > 65536 else 48
    return min(cap, 48 * max(1, (2 * E + 65535) // 65536))


def cell_of(case):
    """(VEC, TPR, column passes, lane trips, basis passes, nbt of the last basis pass)"""
    vec, tpr = onehot_vec_tpr(case["d"])
    bp = basis_passes(case["B"])
    return vec, tpr, column_passes(case["d"]), lane_trips(case["d"]), bp, case["B"] - BASIS_BT * (bp - 1)


def lane_slots(n):
    """slots each of the 8 slot-lanes of a long-row workgroup walks in a row of n slots (lane sl: beg + sl, + 8, ...)"""
    return [len(range(sl, n, SLOT_LANES)) for sl in range(SLOT_LANES)]


# ----------------------------------------------------------------------------- the table
# Every case: V 300, R 237, E 3000 random triples among the vertices >= 4, then vertex h given exactly HUBS[h] slots
# (kernel_grid.grid_triples: object and subject alternately, so both message directions reach it):
#   32   the longest short row;
#   33   the first long row: slot-lane 0 walks 5 slots, the others 4 -- an odd count in one lane of the two-in-flight
#        walk and even ones in the rest, remainders 1 and 0 of the four-in-flight walk;
#   51   lanes walk 7 and 6 slots: remainders 3 and 2;
#   400  50 slots per lane.
V_GRID, R_GRID, E_GRID = 300, 237, 3000
HUBS = (32, 33, 51, 400)


def _case(d, B):
    return dict(name="onehot_d%d_B%d" % (d, B), V=V_GRID, R=R_GRID, d=d, B=B, E=E_GRID, hubs=HUBS, seed=3000 + d + B)


SHIPPED = (500, 5)          # settings/gcn_basis.exp: the shipped gcn_basis width and basis count

ONEHOT_GRID_LIST = [
    _case(20, 64),          # (4, 64): eight full basis passes
    _case(500, 5),          # (4, 128): the shipped shape
    _case(516, 9),          # (4, 256): nvec 129, the second column pass has one live lane; last basis pass nbt 1
    _case(1028, 2),         # (4, 256): nvec 257, two lane trips, three column passes
    _case(9, 8),            # (1, 64): exactly one full basis pass
    _case(101, 16),         # (1, 128): two full basis passes
    _case(301, 17),         # (1, 256): two lane trips, three column passes, three basis passes (nbt 1)
    # the dispatch boundaries nvec 64 | 65, 128 | 129 of each VEC (VEC 4: d = 4 nvec; VEC 1: 64 and 128 are multiples of
    # 4, so the last width below each boundary is 63 and 127).  d = 516 above is VEC 4's nvec 129.
    _case(256, 1), _case(260, 2), _case(512, 3),
    _case(63, 1), _case(65, 2), _case(127, 3), _case(129, 1),
]
ONEHOT_GRID = {c["name"]: c for c in ONEHOT_GRID_LIST}
BOUNDARY_NVECS = (64, 65, 128, 129)
BOUNDARY_WIDTHS = {4: (256, 260, 512, 516), 1: (63, 65, 127, 129)}
WIDEST = {4: "onehot_d1028_B2", 1: "onehot_d301_B17"}      # generated dropout: drop_factor's index at the largest offsets


# ----------------------------------------------------------------------------- graphs that vary the structure, d = 20
CHUNK_EDGE_COUNTS = (48, 49, 0, 1, 96, 97)      # edges of relations 0..5 of chunk_edges: one chunk, one + 1, none, 1, 2, 2 + 1

STRUCTURE_CASES = {
    # more long rows than long-row workgroups: the `lb += n_long_blocks` loop
    "many_long_rows": dict(name="many_long_rows", V=300, R=7, d=20, B=9, E=8000, seed=4001),
    # 2 E > 65536: 512 long-row workgroups and relation chunks of 96
    "capacity_switch": dict(name="capacity_switch", V=300, R=7, d=20, B=3, E=33000, seed=4002),
    # relations whose messages fill exactly one chunk, one chunk plus one, none, one message, two chunks, two plus one
    "chunk_edges": dict(name="chunk_edges", V=300, R=8, d=20, B=9, E=3000, seed=4003),
}
ALL_CASES = dict(ONEHOT_GRID, **STRUCTURE_CASES)


def structure_triples(case):
    V, R, E = case["V"], case["R"], case["E"]
    rng = np.random.RandomState(case["seed"] + 7)
    rel = rng.randint(0, R, size=E)
    if case["name"] == "chunk_edges":
        fixed = np.repeat(np.arange(len(CHUNK_EDGE_COUNTS)), CHUNK_EDGE_COUNTS)
        rel = np.concatenate([fixed, rng.randint(len(CHUNK_EDGE_COUNTS), R, size=E - len(fixed))])[rng.permutation(E)]
    return np.stack([rng.randint(0, V, size=E), rel, rng.randint(0, V, size=E)], axis=1).astype(np.int32)


def case_triples(case):
    return grid_triples(case) if "hubs" in case else structure_triples(case)


def case_inputs(case, L):
    """The case as tests/test_gpu_featureless.py's helpers take it: shape, featureless_reference.make_case's weights, masks
    and upstream gradient for L layers, and the case's own graph."""
    c = dict(V=case["V"], R=case["R"], d=case["d"], B=case["B"], L=L, E=case["E"], name=case["name"])
    c["params"], _, c["masks"], c["dcodes"] = fr.make_case(c["V"], c["R"], c["d"], L, c["B"], 0, seed=case["seed"])
    c["triples"] = case_triples(case)
    return c


# ----------------------------------------------------------------------------- stale table rows
def stale_graphs(V=300, R=7, E=3000, quiet=50, seed=4100):
    """(first, second, quiet vertices): in `first` every vertex below `quiet` sends in both directions -- vertices 0..3 are
    the HUBS rows, long and short --; in `second` none of them appears in an edge, and the others' rows are long and short
    alike."""
    first = grid_triples(dict(V=V, R=R, E=E, hubs=HUBS, seed=seed))
    rng = np.random.RandomState(seed)
    k = np.arange(4, quiet)
    both = np.concatenate([np.stack([k, rng.randint(0, R, len(k)), rng.randint(quiet, V, len(k))], 1),
                           np.stack([rng.randint(quiet, V, len(k)), rng.randint(0, R, len(k)), k], 1)])
    first = np.concatenate([first, both]).astype(np.int32)
    second = np.stack([rng.randint(quiet, V, E), rng.randint(0, R, E), rng.randint(quiet, V, E)], 1).astype(np.int32)
    return first, second, np.arange(quiet)
