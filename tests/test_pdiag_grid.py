"""The add-diagonal variant tables (tests/pdiag_grid.py) cover every compiled variant of csrc/basis_pdiag.hip's kernels,
every loop of theirs beyond its first trip and every boundary of their dispatch; every case's graph holds the rows and
relations it is meant to hold; the mirrors follow the kernel sources; and a plain float32 numpy evaluation of the float64
restatement passes, on every case's inputs, the very checks tests/test_gpu_pdiag_grid.py applies -- the condition its
bounds rest on.  No GPU: a later edit of a table that drops a cell fails here, naming the cell."""
import os
import re

import numpy as np
import pytest

import add_diagonal_reference as adr
import pdiag_grid as pg
from helpers import assert_close
from test_add_diagonal_host import float32_deviation

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")
GRID = pg.PDIAG_GRID_LIST


def _cells():
    return [pg.cell_of(c) for c in GRID]


# ----------------------------------------------------------------------------- cell coverage
def test_the_cells_of_the_table_are_the_product_the_kernels_are_compiled_for():
    have = {cell[:2] for cell in _cells()}
    assert have == {(vec, tpr) for vec in pg.VECS for tpr in pg.TPRS}, "pdiag (VEC, TPR) cells reached: %s" % sorted(have)


def test_every_column_pass_count_and_lane_trip_count_is_in_the_table_for_both_vector_widths():
    passes = {(c[0], c[2]) for c in _cells()}
    missing = [(vec, cp) for vec in pg.VECS for cp in (1, 2, 3) if (vec, cp) not in passes]
    assert not missing, "(VEC, long-row column passes) without a case: %s" % missing
    trips = {(c[0], c[3]) for c in _cells()}
    missing = [(vec, lt) for vec in pg.VECS for lt in (1, 2) if (vec, lt) not in trips]
    assert not missing, "(VEC, short-row lane trips) without a case: %s" % missing


def test_a_partial_last_column_pass_with_one_live_lane_is_in_the_table_for_both_vector_widths():
    have = {pg.vec_tpr(c["d"])[0] for c in GRID if pg.nvec_of(c["d"]) % pg.COLUMN_LANES == 1}
    assert have == set(pg.VECS), "VEC with a case of nvec = 128 k + 1: %s" % sorted(have)


def test_the_wave_per_row_kernels_take_one_trip_and_several_for_both_vector_widths():
    trips = {(c[0], min(c[5], 3)) for c in _cells()}
    missing = [(vec, t) for vec in pg.VECS for t in (1, 2, 3) if (vec, t) not in trips]
    assert not missing, "(VEC, wave trips: 1 | 2 | 3 or more) without a case: %s" % missing
    assert [pg.wave_trips(d) for d in (256, 260, 63, 65)] == [1, 2, 1, 2]      # the boundary nvec 64 | 65 of each VEC


def test_the_mixing_scalars_fill_their_lanes_and_take_a_second_trip():
    Bs = {c["B"] for c in GRID}
    missing = [B for B in (1, 8, 9, 17, 32, 33, 64) if B not in Bs]
    assert not missing, "basis counts B without a case: %s" % missing
    by_B = {c["B"]: pg.cell_of(c) for c in GRID if c["B"] in (32, 33, 64)}
    assert [by_B[B][1] for B in (32, 33, 64)] == [64, 64, 64]                 # 64 lanes per short row in all three
    assert [by_B[B][4] for B in (32, 33, 64)] == [1, 2, 2]                    # 2 B = 64 | 66 | 128 on them
    assert 2 * max(Bs) == pg.MIX_LANES
    assert {pg.vec_tpr(c["d"])[0] for c in GRID if c["B"] in (33, 64)} == set(pg.VECS)


def test_the_diagonal_gradient_takes_one_trip_and_two_for_both_vector_widths():
    trips = {(c[0], c[6]) for c in _cells()}
    missing = [(vec, t) for vec in pg.VECS for t in (1, 2) if (vec, t) not in trips]
    assert not missing, "(VEC, ddiag trips) without a case: %s" % missing
    assert pg.ddiag_trips(1024) == 1 and pg.ddiag_trips(1028) == 2      # d > 1024 with VEC 4
    assert pg.ddiag_trips(255) == 1 and pg.ddiag_trips(257) == 2        # d > 256 with VEC 1


def test_every_dispatch_boundary_is_in_the_table():
    widths = {c["d"] for c in GRID}
    missing = [(vec, d) for vec in pg.VECS for d in pg.BOUNDARY_WIDTHS[vec] if d not in widths]
    assert not missing, "dispatch boundaries (VEC, d) without a case: %s" % missing
    assert [pg.nvec_of(d) for d in pg.BOUNDARY_WIDTHS[4]] == list(pg.BOUNDARY_NVECS)
    assert [pg.vec_tpr(d) for d in pg.BOUNDARY_WIDTHS[4]] == [(4, 64), (4, 128), (4, 128), (4, 256)]
    assert [pg.vec_tpr(d) for d in pg.BOUNDARY_WIDTHS[1]] == [(1, 64), (1, 128), (1, 128), (1, 256)]
    assert pg.vec_tpr(64)[0] == 4 and pg.vec_tpr(128)[0] == 4      # why VEC 1's lower sides are 63 and 127


def test_the_widest_case_of_each_vector_width_is_named():
    for vec in pg.VECS:
        widest = max((c for c in GRID if pg.vec_tpr(c["d"])[0] == vec), key=lambda c: c["d"])
        assert pg.WIDEST[vec] == widest["name"]
        assert pg.lane_trips(widest["d"]) == 2
    assert pg.column_passes(pg.PDIAG_GRID[pg.THREE_PASSES]["d"]) == 3


def test_mirrors_on_known_configurations():
    assert [pg.cell_of(c) for c in GRID[:6]] == [
        (4, 64, 1, 1, 1, 1, 1), (4, 256, 2, 1, 1, 3, 1), (4, 256, 3, 2, 1, 5, 2),
        (1, 64, 1, 1, 1, 1, 1), (1, 256, 2, 1, 1, 3, 1), (1, 256, 3, 2, 1, 5, 2)]
    # what tests/test_gpu_add_diagonal.py reaches: (4, 64) at d = 8, (1, 64) at d = 10, (4, 128) at d = 500: one column
    # pass, two wave trips
    assert [pg.vec_tpr(d) for d in (8, 10, 500)] == [(4, 64), (1, 64), (4, 128)]
    assert pg.column_passes(500) == 1 and pg.wave_trips(500) == 2
    assert [pg.long_blocks(E) for E in (3000, 32768, 32769, 33000)] == [64, 64, 512, 512]
    assert [pg.chunk_of(E, E) for E in (3000, 32768, 32769, 33000)] == [48, 48, 96, 96]


# ----------------------------------------------------------------------------- hub and structure counts
def test_hub_rows_give_the_slot_lanes_unequal_shares():
    assert pg.HUBS == (32, 33, 51, 400) and pg.LONG_ROW == 32
    assert pg.lane_slots(33) == [5, 4, 4, 4, 4, 4, 4, 4]
    assert pg.lane_slots(51) == [7, 7, 7, 6, 6, 6, 6, 6]


@pytest.mark.parametrize("name", sorted(pg.PDIAG_GRID))
def test_grid_case_graph_has_its_hub_rows(name):
    c = pg.PDIAG_GRID[name]
    assert (c["V"], c["R"], c["E"], c["hubs"]) == (300, 237, 3000, pg.HUBS)
    t = pg.case_triples(c)
    assert t.shape == (c["E"], 3) and t.dtype == np.int32
    assert t[:, [0, 2]].min() >= 0 and t[:, [0, 2]].max() < c["V"] and 0 <= t[:, 1].min() and t[:, 1].max() < c["R"]
    slots = pg.row_slots(t, c["V"])
    assert slots.sum() == 2 * c["E"]
    for h, n in enumerate(c["hubs"]):
        assert slots[h] == n, "%s: hub %d has %d slots, not %d" % (name, h, slots[h], n)
        assert (t[:, 2] == h).any() and (t[:, 0] == h).any(), "%s: hub %d reached from one direction" % (name, h)
    assert (slots > pg.LONG_ROW).sum() >= 3 and (slots == 0).sum() == 0
    assert pg.long_blocks(c["E"]) == 64 and pg.chunk_of(c["E"], c["E"]) == 48
    assert 2 * c["V"] * c["B"] * c["d"] < 2 ** 31 and c["B"] <= 64


@pytest.mark.parametrize("name,blocks,chunk", [("many_long_rows", 64, 48), ("capacity_switch", 512, 96)])
def test_dense_graphs_have_more_long_rows_than_their_first_64_workgroups(name, blocks, chunk):
    c = pg.STRUCTURE_CASES[name]
    t = pg.case_triples(c)
    slots = pg.row_slots(t, c["V"])
    assert pg.long_blocks(c["E"]) == blocks and pg.chunk_of(c["E"], c["E"]) == chunk
    assert c["d"] == 20 and c["B"] <= 9
    long_rows = int((slots > pg.LONG_ROW).sum())
    if name == "many_long_rows":
        assert long_rows > 4 * 64 and long_rows % 64 != 0      # every workgroup a fifth row, the last round a partial one
    else:
        assert 2 * c["E"] > 65536 and 64 < long_rows < 512
    assert np.bincount(t[:, 1], minlength=c["R"]).min() > 10 * chunk


def test_chunk_edges_has_its_relations_at_the_chunk_boundaries():
    c = pg.STRUCTURE_CASES["chunk_edges"]
    t = pg.case_triples(c)
    chunk = pg.chunk_of(c["E"], c["E"])
    per_rel = np.bincount(t[:, 1], minlength=c["R"])
    assert chunk == 48 and c["B"] == 9 and c["R"] == 8
    assert tuple(per_rel[:6]) == (chunk, chunk + 1, 0, 1, 2 * chunk, 2 * chunk + 1) == pg.CHUNK_EDGE_COUNTS


def test_case_names_are_unique():
    assert len(pg.PDIAG_GRID) == len(GRID)
    assert len(pg.ALL_CASES) == len(GRID) + len(pg.STRUCTURE_CASES)


# ----------------------------------------------------------------------------- the mirrors follow the sources
@pytest.mark.parametrize("source,pattern,count", [
    ("row_walk.h", r"inline int row_lanes\(int nvec\) \{ return nvec <= 64 \? 64 : \(nvec <= 128 \? 128 : 256\); \}", 1),
    ("basis_pdiag.hip", r"const int tpr = row_lanes\(nvec\);", 2),
    ("row_walk.h", r"constexpr int kRowThreads = 1024;", 1),
    ("basis_pdiag.hip", r"constexpr int kMixLanes = 128;", 1),
    ("row_walk.h", r"inline int long_blocks\(const rgcn_ctx\* c\) \{ return 2 \* c->g\.E > 65536 \? 512 : 64; \}", 1),
    # (k_pdiag_rows keeps its own walk; k_pdiag_dh_join's is the single-accumulator form of row_walk.h, which holds the
    # banked form as well)
    ("basis_pdiag.hip", r"__shared__ float red\[8\]\[128 \* VEC\];", 1),
    ("row_walk.h", r"__shared__ float red\[8\]\[128 \* VEC\];", 2),
    ("basis_pdiag.hip", r"for \(int c0 = 0; c0 < nvec; c0 \+= 128\) \{", 1),
    ("row_walk.h", r"for \(int c0 = 0; c0 < nvec; c0 \+= 128\) \{", 2),
    ("basis_pdiag.hip", r"for \(int cidx = lane; cidx < nvec; cidx \+= TPR\) \{", 1),
    ("row_walk.h", r"for \(int cidx = lane; cidx < nvec; cidx \+= TPR\) \{", 2),
    ("basis_pdiag.hip", r"for \(int j = lane; j < nmix; j \+= TPR\) \{", 1),
    ("basis_pdiag.hip", r"for \(int cidx = lane; cidx < nvec; cidx \+= 64\) \{", 3),
    ("basis_pdiag.hip", r"for \(int e = threadIdx\.x \* VEC; e < a\.d; e \+= 256 \* VEC\) \{", 1),
    ("basis_pdiag.hip", r"const int b = threadIdx\.x;      // \(B <= 64\)", 1),
    ("rgcn_internal.h", r"constexpr int kLongRow = 32;", 1),
    # (B <= 64 itself: tests/test_config_check.py, test_the_add_diagonal_kind_takes_64_bases_and_refuses_65)
])
def test_host_mirrors_follow_the_kernel_sources(source, pattern, count):
    """The mirrors in pdiag_grid.py are copies of these lines: when one changes, the tables have to be re-derived."""
    with open(os.path.join(CSRC, source)) as f:
        found = len(re.findall(pattern, f.read()))
    assert found == count, "%s holds `%s` %d times, not %d: update tests/pdiag_grid.py's mirror" % (source, pattern, found, count)


def row_dispatch_cells():
    """the (VEC, TPR) instantiations the one dispatch definition of the row kernels, RGCN_LAUNCH_ROWS, names"""
    with open(os.path.join(CSRC, "row_walk.h")) as f:
        text = f.read()
    assert text.count("#define RGCN_LAUNCH_ROWS(") == 1
    return [(int(v), int(t)) for v, t in re.findall(r"kernel<(\d+), (\d+)>", text.split("#define RGCN_LAUNCH_ROWS(")[1])]


def test_the_compiled_variants_are_the_product_of_vecs_and_tprs():
    assert sorted(row_dispatch_cells()) == sorted((vec, tpr) for vec in pg.VECS for tpr in pg.TPRS)      # each cell once
    with open(os.path.join(CSRC, "basis_pdiag.hip")) as f:
        text = f.read()
    for kernel in ("k_pdiag_rows", "k_pdiag_dh_join"):      # every row launcher goes through it, and launches no other way
        assert len(re.findall(r"RGCN_LAUNCH_ROWS\(%s, vec4, tpr, grid, block, c->stream, a, nlb\);" % kernel, text)) == 1, kernel
        assert not re.findall(kernel + r"<\d", text), kernel
    for kernel in ("k_pdiag_epilogue", "k_pdiag_row_bwd", "k_pdiag_ddiag"):
        assert set(re.findall(kernel + r"<(\d)>", text)) == {"4", "1"}, kernel


# ----------------------------------------------------------------------------- the float32 condition
def float32_passes(c, norm, tag):
    """what tests/test_gpu_pdiag_grid.py asks of the engine, asked of a plain float32 evaluation"""
    dev, g32, g64 = float32_deviation(c, "train", norm)
    for l, quantities in enumerate(dev, start=1):
        for what, (err, bound) in zip("HaG", quantities):
            print("%s %s L%d layer %d %s: float32 vs float64 max abs %.3e, bound %.3e" % (tag, norm, c["L"], l, what, err, bound))
            assert err <= bound, (tag, norm, l, what, err, bound)
    for n in adr.weight_names(c["L"])[:-1]:
        assert g32[n].dtype == np.float32
        assert_close(g32[n], g64[n], name="%s %s %s" % (tag, norm, n))


@pytest.mark.parametrize("name", [c["name"] for c in GRID] + list(pg.STRUCTURE_CASES))
def test_float32_passes_the_gpu_checks_under_intended_norms(name):
    float32_passes(pg.case_inputs(pg.ALL_CASES[name], 2), "intended", name)


@pytest.mark.parametrize("name", [c["name"] for c in GRID])
def test_float32_passes_the_gpu_checks_as_the_top_layer_under_local_norms(name):
    float32_passes(pg.case_inputs(pg.ALL_CASES[name], 1), "local", name)
