"""The compiled variants of the encoder's row kernels and the cases that reach every one of them.

The block kind's row kernel k_block_rows<SD, BWD, GW, CS> (block_rows.hip) is compiled for six block sizes SD = d / nb
and four group widths GW, and tiles its long rows in TS-slot tiles (LongTile<SD, GW>::TS); its weight-gradient kernel
k_block_msg_bwd (block_msgs.hip) keeps G message slots per workgroup.  The basis kind's k_basis_agg /
k_basis_bwd_gather (basis.hip) pick a vector width VEC and a lane count TPR, and run B > 8 in passes of BT = 8.
The functions below mirror those dispatch formulas on the host, so that a test can state which cell a case reaches;
GRID_CASES is one case per cell (and per boundary of the formulas), each with hub rows that take the long-row paths.
tests/test_kernel_grid.py keeps the table honest without a GPU; tests/test_gpu_parity.py runs it.
"""
import numpy as np

from helpers import make_case

BLOCK_SIZES = (1, 2, 3, 4, 5, 8)      # block_msgs.hip:184-192 (dispatch_sd) and block_rows.hip:701-703
GROUP_WIDTHS = (8, 16, 32, 64)
TILE_SIZES = (64, 32, 16, 8)
LONG_ROW = 32                         # rgcn_internal.h:93 (kLongRow): a row with more slots takes the long-row path
GIANT_ROW = 2048                      # rgcn_internal.h:98 (kGiantRow): full-graph scale only; tests/giant_grid.py reaches it
MAX_BLOCKS = 512                      # config_check.h (check_config)
MAX_BASES = 64                        # config_check.h (check_config)
BASIS_BT = 8                          # row_walk.h:15 (BT): basis functions per pass
D500_BLOCK_COUNTS = (100, 125, 250, 500)   # every nb that divides the shipped d = 500 into a compiled block size


def rows_group_width(nb):
    """block_rows.hip:77-80: the smallest of 8 / 16 / 32 / 64 lanes that holds a band's ceil(nb / 8) blocks."""
    band = (nb + 7) // 8
    return 8 if band <= 8 else (16 if band <= 16 else (32 if band <= 32 else 64))


def long_tile(sd, gw):
    """block_rows.hip:258 (LongTile<SD, GW>::TS): slots of one long-row tile."""
    return 64 if gw * sd <= 80 else (32 if gw * sd <= 160 else (16 if gw * sd <= 320 else 8))


def block_slots(nb, sd):
    """block_msgs.hip (block_geometry): (workgroup size, G message slots per workgroup) of k_block_msg_fwd/_bwd."""
    best_block = best_g = 0
    best_util = 0.0
    for blk in range(64, 513, 64):
        g = blk // nb
        if g < 1:
            continue
        g = min(g, 8)
        while g > 1 and (g - 1) * sd * sd * nb * 4 > 60 * 1024:
            g -= 1
        util = g * nb / blk
        if util > best_util + 1e-9:
            best_util, best_block, best_g = util, blk, g
    return best_block, best_g


def basis_vec_tpr(d):
    """basis.hip:342-344 (and the other launchers, :370-373): float4 columns when d % 4 == 0 (the engine's buffers are
    16-byte aligned), then row_walk.h:48 (row_lanes): 64 / 128 / 256 lanes per row for up to 64 / 128 / more column vectors."""
    vec = 4 if d % 4 == 0 else 1
    nvec = d // vec
    return vec, (64 if nvec <= 64 else (128 if nvec <= 128 else 256))


def block_cell(nb, d):
    """(SD, GW, TS, G) of a block-kind configuration."""
    sd = d // nb
    gw = rows_group_width(nb)
    return sd, gw, long_tile(sd, gw), block_slots(nb, sd)[1]


def empty_bands(nb):
    """Column bands x of k_block_rows / k_wtile_build that hold no block: [x nb / 8, (x + 1) nb / 8) is empty
    (block_rows.hip:109)."""
    return [x for x in range(8) if (x * nb) >> 3 == ((x + 1) * nb) >> 3]


def row_slots(triples, V):
    """Slots of every destination row of k_block_rows / k_basis_agg: a triple (s, r, o) is a message of row o and one of
    row s (graph_prep.hip: row_ptr counts both directions), so a self edge counts twice."""
    t = np.asarray(triples).reshape(-1, 3)
    return np.bincount(np.concatenate([t[:, 2], t[:, 0]]), minlength=V)


# ----------------------------------------------------------------------------- the table
# Every case: V 300, R 237, L 2, E 3000 random triples among the vertices >= len(hubs), then hub h (vertex h) given
# exactly hubs[h] slots by moving one endpoint of that many edges (object and subject alternately, so both message
# directions reach it): a row of exactly 33 slots (the first long row), one of 3 TS + 7 (several tiles and a partial
# one; for TS = 8 a short row of 31) and one of 400 (more than 3 TS for every TS).
# R = 237 (FB15k-237's relation count) keeps the activations at the shipped model's size: the block kind draws every
# layer weight, W_self included, with std 3 / sqrt(R + sd) (gcn_basis_concat.py:22), so at R = 9 and d = 2080 the top
# layer reaches |H2| ~ 300 and even the fp32 oracle sits 1.4e-4 from float64, past the 1e-4 absolute forward tolerance.
V_GRID, R_GRID, L_GRID, E_GRID = 300, 237, 2, 3000


def _block(nb, sd):
    ts = long_tile(sd, rows_group_width(nb))
    return dict(name="block_sd%d_nb%d" % (sd, nb), kind="block", V=V_GRID, R=R_GRID, d=nb * sd, L=L_GRID, nb=nb,
                E=E_GRID, hubs=(33, 3 * ts + 7, 400), seed=1000 + 10 * nb + sd)


def _basis(d, B):
    return dict(name="basis_d%d_B%d" % (d, B), kind="basis", V=V_GRID, R=R_GRID, d=d, L=L_GRID, nb=B, E=E_GRID,
                hubs=(33, 100, 400), seed=2000 + d + B)


BLOCK_GRID = [
    # sd 1: the boundaries 64 / 65 / 129 / 512 of rows_group_width; nb 500 = the shipped d = 500 at one-wide blocks
    _block(64, 1), _block(65, 1), _block(129, 1), _block(500, 1), _block(512, 1),
    # sd 2: nb 128 (last GW 16), nb 250 (d = 500), nb 257 (first GW 64, TS 32)
    _block(20, 2), _block(128, 2), _block(250, 2), _block(257, 2),
    # sd 3: nb 256 (last GW 32, TS 32), nb 260 (TS 16)
    _block(9, 3), _block(100, 3), _block(256, 3), _block(260, 3),
    # sd 4: nb 125 (d = 500), nb 136 (TS 32, G 3), nb 300 (TS 16)
    _block(13, 4), _block(125, 4), _block(136, 4), _block(300, 4),
    # sd 5: nb 6 (bands 0 and 4 hold no block), nb 100 (the shipped configuration), nb 136 (TS 32), nb 264 (TS 16)
    _block(6, 5), _block(100, 5), _block(136, 5), _block(264, 5),
    # sd 8: nb 3 (bands 0, 1, 3, 4, 6 hold no block), nb 72 (TS 32, G 4), nb 136 (TS 16, G 2), nb 260 (TS 8)
    _block(3, 8), _block(72, 8), _block(136, 8), _block(260, 8),
]

BASIS_GRID = [
    # (VEC, TPR) = (4, 64), (4, 128), (4, 256), (1, 64), (1, 128), (1, 256); B in one, two, three and eight passes
    _basis(20, 64), _basis(500, 8), _basis(600, 16), _basis(9, 17), _basis(101, 64), _basis(301, 17),
]

GRID_CASES = {c["name"]: c for c in BLOCK_GRID + BASIS_GRID}


def cell_of(case):
    """The compiled variant a case reaches: ("block", SD, GW, TS, G) or ("basis", VEC, TPR, passes of BT)."""
    if case["kind"] == "block":
        return ("block",) + block_cell(case["nb"], case["d"])
    vec, tpr = basis_vec_tpr(case["d"])
    return ("basis", vec, tpr, -(-case["nb"] // BASIS_BT))


def grid_triples(case):
    """The case's graph: E random triples, the hub rows injected with exact slot counts."""
    V, R, E, hubs = case["V"], case["R"], case["E"], case["hubs"]
    nh = len(hubs)
    rng = np.random.RandomState(case["seed"] + 7)
    triples = np.stack([nh + rng.randint(0, V - nh, size=E), rng.randint(0, R, size=E),
                        nh + rng.randint(0, V - nh, size=E)], axis=1).astype(np.int32)
    edges = rng.permutation(E)
    used = 0
    for h, n in enumerate(hubs):
        for k, e in enumerate(edges[used:used + n]):
            triples[e, 2 if k % 2 == 0 else 0] = h
        used += n
    assert used <= E
    return triples


def grid_inputs(case, train=True):
    """(params, triples, masks, dcodes) of a grid case: helpers.make_case's weights, masks and upstream gradient."""
    params, _, masks, dcodes = make_case(case["V"], case["R"], case["d"], case["L"], case["kind"], case["nb"], 0,
                                         seed=case["seed"], train=train)
    return params, grid_triples(case), masks, dcodes
