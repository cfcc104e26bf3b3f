"""The giant-row cut of the block encoder and the cases that reach every boundary of it.

Above 65,536 messages the block kind on one GPU sums a row with more than kGiantRow = 2048 slots piece by piece
(graph_prep.hip: k_ptrs registers the pieces through two atomic counters; block_rows.hip / k_combine: one workgroup per
2048-slot piece into rgcn_ctx::giant_slab; elementwise.hip: k_combine_giant_finish adds a row's pieces on a fixed grid of
64 workgroups; k_colsum_giant_rows gives every giant row a column-sum part row of its own for the bias gradient).  Every
full-graph evaluation pass runs there.  The functions below mirror the host-side formulas of that path, so that a test
can state which boundary a case reaches; GIANT_CASES is one case per cell and boundary.  tests/test_giant_grid.py keeps
the table honest without a GPU; tests/test_gpu_giant_grid.py runs it against float64.
"""
import numpy as np

import kernel_grid as kg

GIANT_ROW = kg.GIANT_ROW              # rgcn_internal.h:98 (kGiantRow)
GIANT_MESSAGES = 65536                # graph_prep.hip:601: the cut is on above this many messages (2E)
FINISH_GRID = 64                      # elementwise.hip:464 (combine_giant_finish): workgroups of k_combine_giant_finish
PIECE_LANES = 128                     # elementwise.hip:197: column vectors per trip of k_combine's piece loop
FINISH_LANES = 256                    # elementwise.hip:256: column vectors per trip of the finish kernel's column loop
BASE_CHUNK = 48                       # rgcn_internal.h:465 (rgcn_ctx::chunk): messages per relation chunk at minibatch scale


def giant_on(E, kind="block", world=1):
    """graph_prep.hip:601 (graph_build): g.giant_on = kind == BLOCK && world == 1 && 2E > 65536."""
    return kind == "block" and world == 1 and 2 * E > GIANT_MESSAGES


def pieces(slots):
    """graph_prep.hip:223-225 (k_ptrs): a row with more than kGiantRow slots is cut into ceil(slots / kGiantRow) pieces."""
    return -(-slots // GIANT_ROW) if slots > GIANT_ROW else 0


def last_piece(slots):
    """block_rows.hip:426-427: slots of a giant row's last piece."""
    return slots - (pieces(slots) - 1) * GIANT_ROW if slots > GIANT_ROW else 0


def giant_cap(max_edges):
    """graph_prep.hip:511 (graph_alloc): entries of the giant-row list."""
    return 2 * max_edges // GIANT_ROW + 1


def piece_cap(max_edges):
    """graph_prep.hip:512 (graph_alloc): entries of the piece list and rows of giant_slab."""
    return 2 * (2 * max_edges // GIANT_ROW) + 2


def relation_chunk(E, cap):
    """graph_prep.hip:598 (graph_build): messages per relation chunk of THIS graph; cap = the context's own
    (context_chunk)."""
    return min(cap, BASE_CHUNK * max(1, (2 * E + 65535) // 65536))


def context_chunk(max_edges):
    """rgcn_api.hip:688 (create_impl): the capacity-scaled upper bound of relation_chunk."""
    return BASE_CHUNK * ((2 * max_edges + 65535) // 65536) if 2 * max_edges > 65536 else BASE_CHUNK


def rows_long_wg(E):
    """block_rows.hip:671-672 (block_rows): workgroups per band that walk the long-row and piece lists."""
    return max(32, min(1024, 2 * E // 256)) if E > 0 else 0


def combine_long_blocks(E):
    """elementwise.hip:439-442 (combine): long-row workgroups of k_combine (the two-kernel form)."""
    return 4 * max(64, min(1024, 2 * E // 1024))


def rows_per_wg(nb):
    """block_rows.hip:664-669 (block_rows): rows of one short-row workgroup."""
    quantum = 4 * (64 // kg.rows_group_width(nb))
    return max(quantum, min(256, 64 // quantum * quantum))


def colsum_part_floats(V, d):
    """rgcn_api.hip:661 (create_shared_tail): floats of one half of the column-sum scratch."""
    return ((V + 3) // 4 + 1024 + 2 + ((V + 3) // 4 + 1024) // 32 + 2) * d


def colsum_in_kernel(V, d, E, max_edges, nb):
    """block_rows.hip:679-681 (block_rows): the bottom layer's row-gradient kernel leaves the bias gradient's column
    partials itself when one part row per workgroup of a band plus giant_cap rows for the giant rows fit the scratch;
    otherwise a separate pass sums the columns of dL/dH0."""
    grid8 = rows_long_wg(E) + -(-V // rows_per_wg(nb))
    parts = giant_cap(max_edges) if giant_on(E) else 0
    return (grid8 + parts) * d <= colsum_part_floats(V, d)


def finish_trips(n_giant):
    """elementwise.hip:254 (k_combine_giant_finish): trips of `for (i = blockIdx.x; i < n; i += gridDim.x)`."""
    return -(-n_giant // FINISH_GRID)


def vec_width(d):
    """elementwise.hip:431 / :462: float4 columns when d % 4 == 0 (the engine's buffers are 16-byte aligned)."""
    return 4 if d % 4 == 0 else 1


def piece_loop_chunks(d):
    """elementwise.hip:197 (k_combine): trips of `for (c0 = 0; c0 < nvec; c0 += 128)` over a piece."""
    return -(-(d // vec_width(d)) // PIECE_LANES)


def finish_loop_chunks(d):
    """elementwise.hip:256 (k_combine_giant_finish): trips of `for (cidx = threadIdx.x; cidx < nvec; cidx += 256)`."""
    return -(-(d // vec_width(d)) // FINISH_LANES)


# ----------------------------------------------------------------------------- the table
# R = 237, L = 2 as in kernel_grid.py (the activations stay at the shipped model's size).  Graphs by kernel_grid.grid_triples:
# the random part avoids the hub vertices, hub h gets exactly hubs[h] slots, object and subject alternately.
R_GIANT, L_GIANT = 237, 2
# two ordinary long rows; the longest UNCUT row; pieces 2048 + 1; two full pieces; 2048 + 2048 + 1; a last piece of 1904
HUBS = (33, 400, 2048, 2049, 4096, 4097, 6000)
V_STD, E_STD = 3000, 33000            # 2E = 66,000: the seven rows above are the only long ones, four of them giant


def _case(name, nb, sd, V=V_STD, E=E_STD, hubs=HUBS, seed=None, **more):
    c = dict(name=name, kind="block", V=V, R=R_GIANT, d=nb * sd, L=L_GIANT, nb=nb, E=E, hubs=tuple(hubs),
             seed=3000 + 10 * nb + sd if seed is None else seed, max_edges=E, drop_free_edge=False, float64=True)
    c.update(more)
    return c


def _std(nb, sd, **more):
    return _case("giant_sd%d_nb%d" % (sd, nb), nb, sd, **more)


GIANT_GRID = [
    # block size and vector width, all GW 8: d 9 and d 15 take VEC 1 (k_combine_giant_finish<1>); nb 3 leaves the column
    # bands 0, 1, 3, 4, 6 without a block  (nb 9: the formula's seed 3091 draws an eighth long row, of 36 slots)
    _std(9, 1, seed=3092), _std(10, 2), _std(5, 3), _std(6, 4), _std(4, 5), _std(3, 8),
    # group width and column chunks: GW 16; GW 32 with nvec 129 (second chunk of the piece loop); GW 64, VEC 1 with
    # nvec 257 (third chunk of the piece loop, second trip of the finish loop)
    _std(100, 2), _std(129, 4), _std(257, 1),
    # VEC 4 on the finish loop's second trip needs d > 1024: bitwise form comparison only (its float64 reference is ~25 s)
    _std(257, 4, float64=False),
    # counting: every one of the 300 rows long, so the long-row list wraps round k_combine's 256 long-row workgroups
    _case("giant_all_long", 4, 5, V=300, hubs=(2049, 4097), seed=3101),
    # 66 giant rows: a second trip of the finish kernel, k_colsum_giant_rows' rank over 66 part rows
    _case("giant_many", 2, 4, V=600, E=140000, hubs=tuple(2049 + h for h in range(66)), seed=3102),
    # the switch: 2E = 65,538 (cut on) and the same triples without the last edge that touches no hub, 2E = 65,536 (cut
    # off: the rows of 2049 .. 6000 slots go down the ordinary long-row path)
    _case("giant_switch_on", 4, 5, E=32769, seed=3103),
    _case("giant_switch_off", 4, 5, E=32769, seed=3103, drop_free_edge=True),
    # a context sized for 1,200,000 edges: giant_cap = 1172 part rows no longer fit the column-sum scratch of V = 64
    _case("giant_colsum_fallback", 2, 4, V=64, hubs=(2049, 4097), seed=3104, max_edges=1200000),
]

GIANT_CASES = {c["name"]: c for c in GIANT_GRID}
FLOAT64_CASES = sorted(n for n, c in GIANT_CASES.items() if c["float64"])


def case_edges(case):
    """Edges of the graph the engine is given (giant_switch_off: one fewer than grid_triples draws)."""
    return case["E"] - (1 if case["drop_free_edge"] else 0)


def free_edge(case, triples=None):
    """Index of the last edge of grid_triples(case) that touches no hub."""
    t = kg.grid_triples(case) if triples is None else triples
    nh = len(case["hubs"])
    return int(np.flatnonzero((t[:, 0] >= nh) & (t[:, 2] >= nh))[-1])


def giant_triples(case):
    """The case's graph: kernel_grid.grid_triples, for drop_free_edge without free_edge(case)."""
    t = kg.grid_triples(case)
    if case["drop_free_edge"]:
        t = np.delete(t, free_edge(case, t), axis=0)
    return np.ascontiguousarray(t)


def giant_inputs(case, train=True):
    """(params, triples, masks, dcodes) of a case: helpers.make_case's weights, masks and upstream gradient."""
    params, _, masks, dcodes = kg.grid_inputs(case, train=train)
    return params, giant_triples(case), masks, dcodes


def giant_rows(case, slots=None):
    """Slot counts of the rows the engine cuts (empty when the cut is off)."""
    if not giant_on(case_edges(case), case["kind"]):
        return []
    s = kg.row_slots(giant_triples(case), case["V"]) if slots is None else slots
    return [int(n) for n in s if n > GIANT_ROW]
