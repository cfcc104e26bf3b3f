"""The launch shapes of the highway kernels (csrc/highway.hip) and the cases that reach every one of them, every loop of
theirs beyond its first trip, and every boundary of their dispatch.

k_highway_fwd is a grid-stride loop over V d / VEC vectors on at most 8192 x 256 threads: fwd_trips(V, d).  The row-lane
kernels k_highway_bwd and k_highway_join (VEC in {4, 1}) lay a workgroup of 256 threads out as CL column lanes x RL row
lanes, CL = column_lanes(d) the power of two that covers nvec = d / VEC, at most 256, RL = row_lanes(d) = 256 / CL:
  * `c0 += CL` walks the columns in column_chunks(d) = ceil(nvec / CL) chunks (a second one only at nvec > 256); on every
    chunk after the first hw_column_partial reuses the LDS buffer `red` behind its leading __syncthreads();
  * row_grid(V, d) = ceil(V / RL) workgroups, at most 1024, each leaving one row of column partials (b_highway, b_emb),
    which k_colsum_final adds;
  * `r += gridDim.x * RL` walks the rows in row_trips(V, d) trips (a second one only at CL = 256 and V > 1024).
The functions below mirror those formulas on the host; HIGHWAY_GRID is one case per cell and per boundary.  The highway
kernels do not see the layer kind beneath them, so the table uses the basis kind with one or two basis functions, and
one block case, since a highway context also changes the block layer's backward epilogue.
tests/test_highway_grid.py keeps the table honest without a GPU; tests/test_gpu_highway_grid.py runs it.
"""
import highway_reference as hr
from kernel_grid import grid_triples

VECS = (4, 1)
HW_THREADS = 256            # highway.hip: kHwThreads
HW_MAX_BLOCKS = 1024        # highway.hip: kHwMaxBlocks
FWD_MAX_BLOCKS = 8192       # highway.hip (highway_forward): `if (grid > 8192) grid = 8192;`


# ----------------------------------------------------------------------------- host mirrors
def vec_of(d):
    """highway.hip (highway_forward, highway_backward, highway_join): float4 accesses when d % 4 == 0 (the engine's
    buffers are 16-byte aligned), scalar ones otherwise"""
    return 4 if d % 4 == 0 else 1


def nvec_of(d):
    return d // vec_of(d)


def column_lanes(d):
    """highway.hip (hw_column_lanes): the power of two that covers nvec, at most the workgroup"""
    cl = 1
    while cl < nvec_of(d) and cl < HW_THREADS:
        cl *= 2
    return cl


def row_lanes(d):
    """k_highway_bwd / k_highway_join: `RL = kHwThreads / CL`"""
    return HW_THREADS // column_lanes(d)


def column_chunks(d):
    """k_highway_bwd / k_highway_join: chunks of `for (int c0 = 0; c0 < nvec; c0 += CL)`"""
    return -(-nvec_of(d) // column_lanes(d))


def row_grid(V, d):
    """highway.hip (hw_row_grid): every row lane of the grid gets a row, capped at kHwMaxBlocks workgroups"""
    return max(1, min(-(-V // row_lanes(d)), HW_MAX_BLOCKS))


def row_trips(V, d):
    """k_highway_bwd / k_highway_join: trips of `r += gridDim.x * RL` of row lane 0 of workgroup 0"""
    return -(-V // (row_grid(V, d) * row_lanes(d)))


def fwd_trips(V, d):
    """highway_forward / k_highway_fwd: trips of the grid-stride loop of thread 0 (grid capped at 8192 workgroups)"""
    nvec = V * d // vec_of(d)
    threads = min(-(-nvec // HW_THREADS), FWD_MAX_BLOCKS) * HW_THREADS
    return -(-nvec // threads)


def cell_of(case):
    """(VEC, CL, column chunks, row trips, forward trips)"""
    V, d = case["V"], case["d"]
    return vec_of(d), column_lanes(d), column_chunks(d), row_trips(V, d), fwd_trips(V, d)


# ----------------------------------------------------------------------------- the table
# Every case: R 237, E 3000 random triples among the vertices >= 3, then rows of exactly 33, 100 and 400 slots
# (kernel_grid.grid_triples, kernel_grid.py's basis hubs); the width cases at V = 300.  R = 237 keeps the block case's
# weights at the shipped model's size (kernel_grid.py).
R_GRID, E_GRID = 237, 3000
HUBS = (33, 100, 400)


def _case(d, V=300, L=2, kind="basis", nb=1, name=None):
    return dict(name=name or "hw_d%d" % d, kind=kind, V=V, R=R_GRID, d=d, L=L, nb=nb, E=E_GRID, hubs=HUBS,
                seed=7000 + d + V + L)


HIGHWAY_GRID_LIST = [
    # VEC 4
    _case(4),                # CL 1, RL 256: one column lane, and V = 300 is no multiple of RL
    _case(20, nb=2),         # CL 8 over nvec 5: ragged
    _case(512),              # CL 128 = nvec: an exact power of two, the lower side of nvec 128 | 129
    _case(516, L=3),         # CL 256 over nvec 129: the upper side; three layers, the D / dS / dZ ping-pong at width
    _case(1024),             # CL 256 = nvec: exact, RL 1, the lower side of nvec 256 | 257
    _case(1028),             # nvec 257: two column chunks, one live lane in the second
    # VEC 1 (256 and 128 are multiples of 4: the last scalar widths below the boundaries are 255 and 127)
    _case(2, nb=2),          # CL 2 = nvec: the one exact power of two a scalar width can have besides 1; RL 128
    _case(127),              # CL 128 over nvec 127: ragged, the lower side of 128 | 129
    _case(129),              # CL 256: the upper side
    _case(255),              # CL 256 over nvec 255: the lower side of 256 | 257
    _case(257),              # two column chunks, one live lane in the second
    # the block layer's backward epilogue on a highway context, at a CL = 256 width: d = 129 blocks of 4
    _case(516, kind="block", nb=129, name="hw_block_d516"),
    # V > 1024 at CL = 256: a second trip of the row loop, and k_colsum_final adds 1024 partial rows
    _case(1028, V=1100, name="hw_rows_vec4"),
    _case(257, V=1100, name="hw_rows_vec1"),
    # V d / VEC just past 8192 x 256 threads: a second trip of k_highway_fwd's loop, with the least memory (one layer)
    _case(260, V=32300, L=1, name="hw_fwd_vec4"),
    _case(257, V=8200, L=1, name="hw_fwd_vec1"),
]
HIGHWAY_GRID = {c["name"]: c for c in HIGHWAY_GRID_LIST}
BOUNDARY_WIDTHS = {4: (512, 516, 1024, 1028), 1: (127, 129, 255, 257)}     # nvec 128 | 129 and 256 | 257
WIDEST = {4: "hw_d1028", 1: "hw_d257"}       # generated dropout on the second column chunk
GEMM_MODE_0 = "hw_d516"
ROW_TRIPS = {4: "hw_rows_vec4", 1: "hw_rows_vec1"}
FWD_TRIPS = {4: "hw_fwd_vec4", 1: "hw_fwd_vec1"}


def case_inputs(case):
    """highway_reference.make_case's weights, masks and upstream gradient on the case's own graph"""
    c = hr.make_case(case["V"], case["R"], case["d"], case["L"], case["kind"], case["nb"], grid_triples(case),
                     seed=case["seed"])
    c["name"] = case["name"]
    return c
