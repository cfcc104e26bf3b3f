"""The kernel-variant table (tests/kernel_grid.py) covers every compiled variant of the encoder's row kernels, and every
case's graph holds the rows it is meant to send down the long-row paths.  No GPU: a later edit of the table that drops
a cell fails here, naming the cell."""
import os

import numpy as np
import pytest

import kernel_grid as kg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")


def _cells(kind):
    return {kg.cell_of(c) for c in kg.GRID_CASES.values() if c["kind"] == kind}


def test_every_block_size_and_group_width_is_in_the_table():
    have = {(sd, gw) for _, sd, gw, _, _ in _cells("block")}
    missing = [(sd, gw) for sd in kg.BLOCK_SIZES for gw in kg.GROUP_WIDTHS if (sd, gw) not in have]
    assert not missing, "block (SD, GW) cells without a case: %s" % missing


def test_every_long_row_tile_size_is_in_the_table():
    have = {ts for _, _, _, ts, _ in _cells("block")}
    missing = [ts for ts in kg.TILE_SIZES if ts not in have]
    assert not missing, "LongTile::TS values without a case: %s" % missing


def test_slot_reduction_of_the_weight_gradient_runs_at_sd_8():
    """k_block_msg_bwd sums its G slots through LDS when G > 1; at sd = 8 that sum is the largest."""
    have = {g for _, sd, _, _, g in _cells("block") if sd == 8}
    assert any(g > 1 for g in have), "no sd = 8 case with G > 1 message slots (have G %s)" % sorted(have)


def test_block_count_boundaries_are_in_the_table():
    nbs = {c["nb"] for c in kg.BLOCK_GRID}
    missing = [nb for nb in (64, 65, 128, 129, 256, 257, 512) if nb not in nbs]
    assert not missing, "group-width boundaries nb without a case: %s" % missing
    assert any(nb % 8 for nb in nbs), "no nb % 8 != 0 case"
    assert any(kg.empty_bands(nb) for nb in nbs if nb < 8), "no nb < 8 case with empty column bands"


def test_every_block_count_of_the_shipped_width_is_in_the_table():
    have = {c["nb"] for c in kg.BLOCK_GRID if c["d"] == 500}
    missing = [nb for nb in kg.D500_BLOCK_COUNTS if nb not in have]
    assert not missing, "d = 500 block counts without a case: %s" % missing
    # and those are all of them: every divisor of 500 whose quotient is a compiled block size
    assert sorted(nb for nb in range(1, kg.MAX_BLOCKS + 1) if 500 % nb == 0 and 500 // nb in kg.BLOCK_SIZES) == \
        list(kg.D500_BLOCK_COUNTS)


def test_every_basis_variant_and_pass_count_is_in_the_table():
    have = {(vec, tpr) for _, vec, tpr, _ in _cells("basis")}
    missing = [(vec, tpr) for vec in (4, 1) for tpr in (64, 128, 256) if (vec, tpr) not in have]
    assert not missing, "basis (VEC, TPR) cells without a case: %s" % missing
    Bs = {c["nb"] for c in kg.BASIS_GRID}
    missing = [B for B in (8, 16, 17, kg.MAX_BASES) if B not in Bs]
    assert not missing, "basis counts B without a case: %s" % missing


@pytest.mark.parametrize("name", sorted(kg.GRID_CASES))
def test_case_graph_has_its_long_rows(name):
    """Counted from the incidence of both directions: a row of exactly 33 slots, a row longer than 3 TS (several
    long-row tiles), the hub rows reached from both directions, no giant row, and vertex ids within range."""
    c = kg.GRID_CASES[name]
    t = kg.grid_triples(c)
    assert t.shape == (c["E"], 3) and t.dtype == np.int32
    assert t[:, [0, 2]].min() >= 0 and t[:, [0, 2]].max() < c["V"] and 0 <= t[:, 1].min() and t[:, 1].max() < c["R"]
    slots = kg.row_slots(t, c["V"])
    assert slots.sum() == 2 * c["E"]
    for h, n in enumerate(c["hubs"]):
        assert slots[h] == n, "%s: hub %d has %d slots, not %d" % (name, h, slots[h], n)
        if n > 1:
            assert (t[:, 2] == h).any() and (t[:, 0] == h).any(), "%s: hub %d reached from one direction" % (name, h)
    assert (slots == kg.LONG_ROW + 1).any(), "%s: no row of exactly %d slots" % (name, kg.LONG_ROW + 1)
    assert (slots > kg.LONG_ROW).sum() >= 2, "%s: fewer than two long rows" % name
    if c["kind"] == "block":
        ts = kg.cell_of(c)[3]
        assert (slots > max(3 * ts, kg.LONG_ROW)).any(), "%s: no long row spanning more than 3 tiles of %d" % (name, ts)
    assert slots.max() <= kg.GIANT_ROW


def test_case_shapes_are_valid_configurations():
    for name, c in kg.GRID_CASES.items():
        if c["kind"] == "block":
            assert c["d"] % c["nb"] == 0 and c["d"] // c["nb"] in kg.BLOCK_SIZES and c["nb"] <= kg.MAX_BLOCKS, name
        else:
            assert 1 <= c["nb"] <= kg.MAX_BASES, name


@pytest.mark.parametrize("source,text", [
    ("block_rows.hip", "return band <= 8 ? 8 : (band <= 16 ? 16 : (band <= 32 ? 32 : 64));"),
    ("block_rows.hip", "TS = GW * SD <= 80 ? 64 : (GW * SD <= 160 ? 32 : (GW * SD <= 320 ? 16 : 8));"),
    ("block_rows.hip", "const int b0 = (x * nb) >> 3, b1 = ((x + 1) * nb) >> 3;"),
    ("block_msgs.hip", "while (g > 1 && (size_t)(g - 1) * c->sd * c->sd * c->nb * sizeof(float) > 60 * 1024) --g;"),
    ("row_walk.h", "inline int row_lanes(int nvec) { return nvec <= 64 ? 64 : (nvec <= 128 ? 128 : 256); }"),
    ("basis.hip", "const int tpr = row_lanes(nvec);"),
    ("row_walk.h", "constexpr int BT = 8;"),
    ("rgcn_internal.h", "constexpr int kLongRow = 32;"),
])
def test_host_mirrors_follow_the_kernel_sources(source, text):
    """The mirrors in kernel_grid.py are copies of these dispatch lines: when one changes, the table has to be re-derived."""
    with open(os.path.join(CSRC, source)) as f:
        assert text in f.read(), "%s no longer holds `%s`: update tests/kernel_grid.py's mirror" % (source, text)


def test_mirrors_on_known_configurations():
    assert [kg.rows_group_width(nb) for nb in (1, 64, 65, 128, 129, 256, 257, 512)] == [8, 8, 16, 16, 32, 32, 64, 64]
    assert kg.block_cell(100, 500) == (5, 16, 64, 5)
    assert kg.block_cell(72, 576)[1:] == (16, 32, 4)
    assert kg.block_cell(260, 2080)[1:3] == (64, 8)
    assert [kg.basis_vec_tpr(d) for d in (20, 500, 600, 9, 101, 301)] == \
        [(4, 64), (4, 128), (4, 256), (1, 64), (1, 128), (1, 256)]
