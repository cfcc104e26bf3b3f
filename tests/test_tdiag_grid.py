"""The times-diag variant tables (tests/tdiag_grid.py) cover every compiled variant of csrc/basis_tdiag.hip's kernels, every
loop of theirs beyond its first trip and every boundary of their dispatch; every case's graph holds the rows and
relations it is meant to hold; the mirrors follow the kernel sources; and a plain float32 numpy evaluation of the float64
restatement passes, on every case's inputs, the very checks tests/test_gpu_tdiag_grid.py applies -- the condition its
bounds rest on.  No GPU: a later edit of a table that drops a cell fails here, naming the cell."""
import os
import re

import numpy as np
import pytest

import tdiag_grid as tg
import times_diag_reference as tdr
from helpers import assert_close
from test_times_diag_host import FWD_ATOL, float32_deviation

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")
GRID = tg.TDIAG_GRID_LIST


def _cells():
    return [tg.cell_of(c) for c in GRID]


# ----------------------------------------------------------------------------- cell coverage
def test_the_cells_of_the_table_are_the_product_the_kernels_are_compiled_for():
    have = {cell[:2] for cell in _cells()}
    assert have == {(vec, tpr) for vec in tg.VECS for tpr in tg.TPRS}, "tdiag (VEC, TPR) cells reached: %s" % sorted(have)


def test_every_column_pass_count_and_lane_trip_count_is_in_the_table_for_both_vector_widths():
    passes = {(c[0], c[2]) for c in _cells()}
    missing = [(vec, cp) for vec in tg.VECS for cp in (1, 2, 3) if (vec, cp) not in passes]
    assert not missing, "(VEC, long-row column passes) without a case: %s" % missing
    trips = {(c[0], c[3]) for c in _cells()}
    missing = [(vec, lt) for vec in tg.VECS for lt in (1, 2) if (vec, lt) not in trips]
    assert not missing, "(VEC, short-row lane trips) without a case: %s" % missing


def test_a_partial_last_column_pass_with_one_live_lane_is_in_the_table_for_both_vector_widths():
    have = {tg.vec_tpr(c["d"])[0] for c in GRID if tg.nvec_of(c["d"]) % tg.COLUMN_LANES == 1}
    assert have == set(tg.VECS), "VEC with a case of nvec = 128 k + 1: %s" % sorted(have)


def test_every_basis_count_is_in_the_table_and_a_second_tile_runs_on_a_multi_pass_long_row():
    Bs = {c["B"] for c in GRID}
    missing = [B for B in (1, 8, 9, 17) if B not in Bs]
    assert not missing, "basis counts B without a case: %s" % missing
    assert [tg.basis_passes(B) for B in (1, 8, 9, 17)] == [(1, 1), (1, 8), (2, 1), (3, 1)]
    for vec in tg.VECS:
        wide = [c["name"] for c in GRID if tg.vec_tpr(c["d"])[0] == vec and c["B"] in (9, 17) and tg.column_passes(c["d"]) >= 2]
        assert wide, "VEC %d: no case with a second B-tile at two or more column passes" % vec
    assert max(c["B"] * c["d"] for c in GRID) <= 5200


def test_the_coefficient_gradient_takes_one_trip_and_several_for_both_vector_widths():
    trips = {(c[0], min(c[6], 2)) for c in _cells()}
    missing = [(vec, t) for vec in tg.VECS for t in (1, 2) if (vec, t) not in trips]
    assert not missing, "(VEC, dcoef trips: 1 | 2 or more) without a case: %s" % missing
    assert tg.dcoef_trips(1, 1024) == 1 and tg.dcoef_trips(1, 1028) == 2      # B d > 1024 with VEC 4
    assert tg.dcoef_trips(1, 255) == 1 and tg.dcoef_trips(1, 257) == 2        # B d > 256 with VEC 1


def test_every_dispatch_boundary_is_in_the_table():
    widths = {c["d"] for c in GRID}
    missing = [(vec, d) for vec in tg.VECS for d in tg.BOUNDARY_WIDTHS[vec] if d not in widths]
    assert not missing, "dispatch boundaries (VEC, d) without a case: %s" % missing
    assert [tg.nvec_of(d) for d in tg.BOUNDARY_WIDTHS[4]] == list(tg.BOUNDARY_NVECS)
    assert [tg.vec_tpr(d) for d in tg.BOUNDARY_WIDTHS[4]] == [(4, 64), (4, 128), (4, 128), (4, 256)]
    assert [tg.vec_tpr(d) for d in tg.BOUNDARY_WIDTHS[1]] == [(1, 64), (1, 128), (1, 128), (1, 256)]
    assert tg.vec_tpr(64)[0] == 4 and tg.vec_tpr(128)[0] == 4      # why VEC 1's lower sides are 63 and 127


def test_the_widest_case_of_each_vector_width_is_named():
    for vec in tg.VECS:
        widest = max((c for c in GRID if tg.vec_tpr(c["d"])[0] == vec), key=lambda c: c["d"])
        assert tg.WIDEST[vec] == widest["name"]
        assert tg.lane_trips(widest["d"]) == 2
    assert tg.column_passes(tg.TDIAG_GRID[tg.THREE_PASSES]["d"]) == 3


def test_mirrors_on_known_configurations():
    assert [tg.cell_of(c) for c in GRID[:6]] == [
        (4, 64, 1, 1, 1, 8, 1), (4, 256, 2, 1, 2, 1, 5), (4, 256, 3, 2, 1, 2, 3),
        (1, 64, 1, 1, 1, 8, 1), (1, 256, 2, 1, 3, 1, 9), (1, 256, 3, 2, 2, 1, 11)]
    # what tests/test_gpu_times_diag.py reaches: (4, 64) at d = 8, (1, 64) at d = 10, (4, 128) at d = 500, one column pass
    assert [tg.vec_tpr(d) for d in (8, 10, 500)] == [(4, 64), (1, 64), (4, 128)] and tg.column_passes(500) == 1
    assert [tg.long_blocks(E) for E in (3000, 32768, 32769, 33000)] == [64, 64, 512, 512]
    assert [tg.chunk_of(E, E) for E in (3000, 32768, 32769, 33000)] == [48, 48, 96, 96]
    assert [tg.join_trips(V, d) for V, d in ((300, 1028), (8160, 257), (8161, 257), (32263, 260), (32264, 260))] == [1, 1, 2, 1, 2]
    assert tg.auto_split_k(500, 500, 14541) == 32 and tg.auto_split_k(500, 500, 14541, True) == 16
    assert tg.auto_split_k(1028, 2 * 2 * 1028, 300, True) == 1 and tg.auto_split_k(257, 514, 300, True) == 3


# ----------------------------------------------------------------------------- the large cases
def test_the_large_cases_take_a_second_trip_of_the_dh_epilogue_with_the_least_memory():
    vecs = set()
    for c in tg.LARGE_CASES.values():
        vec = tg.vec_tpr(c["d"])[0]
        vecs.add(vec)
        assert tg.join_trips(c["V"], c["d"]) == 2 and tg.join_trips(c["V"] - 100, c["d"]) == 1, c["name"]
        assert c["B"] == 1 and c["L"] == 1 and c["E"] <= 3000
        assert 2 * c["V"] * c["B"] * c["d"] < 2 ** 31
    assert vecs == set(tg.VECS)
    assert all(tg.join_trips(c["V"], c["d"]) == 1 for c in list(GRID) + list(tg.STRUCTURE_CASES.values()))


def test_the_weight_gradient_split_is_capped_in_a_large_case_and_not_in_the_width_table():
    for c in tg.LARGE_CASES.values():
        assert tg.dw_split(c["V"], c["d"], c["B"]) == c["dw_split"], c["name"]
    assert any(c["dw_split"][0] > tg.DW_SLABS == c["dw_split"][1] for c in tg.LARGE_CASES.values())
    assert all(tg.dw_split(c["V"], c["d"], c["B"])[0] <= 3 for c in GRID)


# ----------------------------------------------------------------------------- hub and structure counts
def test_hub_rows_give_the_slot_lanes_unequal_shares():
    assert tg.HUBS == (32, 33, 51, 400) and tg.LONG_ROW == 32
    assert tg.lane_slots(33) == [5, 4, 4, 4, 4, 4, 4, 4]
    assert tg.lane_slots(51) == [7, 7, 7, 6, 6, 6, 6, 6]
    assert len(set(tg.lane_slots(33))) == 2 and len(set(tg.lane_slots(51))) == 2 and tg.lane_slots(400) == [50] * 8


@pytest.mark.parametrize("name", sorted(tg.TDIAG_GRID))
def test_grid_case_graph_has_its_hub_rows(name):
    c = tg.TDIAG_GRID[name]
    assert (c["V"], c["R"], c["E"], c["hubs"]) == (300, 237, 3000, tg.HUBS)
    t = tg.case_triples(c)
    assert t.shape == (c["E"], 3) and t.dtype == np.int32
    assert t[:, [0, 2]].min() >= 0 and t[:, [0, 2]].max() < c["V"] and 0 <= t[:, 1].min() and t[:, 1].max() < c["R"]
    slots = tg.row_slots(t, c["V"])
    assert slots.sum() == 2 * c["E"]
    for h, n in enumerate(c["hubs"]):
        assert slots[h] == n, "%s: hub %d has %d slots, not %d" % (name, h, slots[h], n)
        assert (t[:, 2] == h).any() and (t[:, 0] == h).any(), "%s: hub %d reached from one direction" % (name, h)
    assert (slots > tg.LONG_ROW).sum() >= 3 and (slots == 0).sum() == 0
    assert tg.long_blocks(c["E"]) == 64 and tg.chunk_of(c["E"], c["E"]) == 48


@pytest.mark.parametrize("name,blocks,chunk", [("many_long_rows", 64, 48), ("capacity_switch", 512, 96)])
def test_dense_graphs_have_more_long_rows_than_their_first_64_workgroups(name, blocks, chunk):
    c = tg.STRUCTURE_CASES[name]
    t = tg.case_triples(c)
    slots = tg.row_slots(t, c["V"])
    assert tg.long_blocks(c["E"]) == blocks and tg.chunk_of(c["E"], c["E"]) == chunk
    assert c["d"] == 20 and c["B"] <= 9
    long_rows = int((slots > tg.LONG_ROW).sum())
    if name == "many_long_rows":
        assert long_rows > 4 * 64 and long_rows % 64 != 0      # every workgroup a fifth row, the last round a partial one
    else:
        assert 2 * c["E"] > 65536 and 64 < long_rows < 512
    assert np.bincount(t[:, 1], minlength=c["R"]).min() > 10 * chunk


def test_chunk_edges_has_its_relations_at_the_chunk_boundaries():
    c = tg.STRUCTURE_CASES["chunk_edges"]
    t = tg.case_triples(c)
    chunk = tg.chunk_of(c["E"], c["E"])
    per_rel = np.bincount(t[:, 1], minlength=c["R"])
    assert chunk == 48 and c["B"] == 9 and c["R"] == 8
    assert tuple(per_rel[:6]) == (chunk, chunk + 1, 0, 1, 2 * chunk, 2 * chunk + 1) == tg.CHUNK_EDGE_COUNTS


def test_stale_case_silences_vertices_that_sent_on_long_rows_and_short_ones():
    c, second, quiet = tg.stale_case()
    assert c["nb"] == 17 and tg.basis_passes(c["nb"]) == (3, 1) and len(quiet) == 50
    slots = tg.row_slots(c["triples"], 300)
    assert tuple(slots[:4]) == tg.HUBS and (slots[quiet] > 0).all()
    assert not np.isin(second[:, [0, 2]], quiet).any() and len(second) <= len(c["triples"])


def test_case_names_are_unique():
    assert len(tg.TDIAG_GRID) == len(GRID)
    assert len(tg.ALL_CASES) == len(GRID) + len(tg.STRUCTURE_CASES) + len(tg.LARGE_CASES)


# ----------------------------------------------------------------------------- the mirrors follow the sources
@pytest.mark.parametrize("source,pattern,count", [
    ("row_walk.h", r"inline int row_lanes\(int nvec\) \{ return nvec <= 64 \? 64 : \(nvec <= 128 \? 128 : 256\); \}", 1),
    ("basis_tdiag.hip", r"const int tpr = row_lanes\(nvec\);", 2),
    ("row_walk.h", r"constexpr int BT = 8;", 1),
    ("row_walk.h", r"constexpr int kRowThreads = 1024;", 1),
    ("row_walk.h", r"inline int long_blocks\(const rgcn_ctx\* c\) \{ return 2 \* c->g\.E > 65536 \? 512 : 64; \}", 1),
    # (the two forms of the row walk: single accumulator, k_tdiag_rows; banked, k_tdiag_dp)
    ("row_walk.h", r"__shared__ float red\[8\]\[128 \* VEC\];", 2),
    ("row_walk.h", r"for \(int c0 = 0; c0 < nvec; c0 \+= 128\) \{", 2),
    ("row_walk.h", r"for \(int cidx = lane; cidx < nvec; cidx \+= TPR\) \{", 2),
    ("basis_tdiag.hip", r"for \(int e = threadIdx\.x \* VEC; e < Bd; e \+= 256 \* VEC\) \{", 1),
    ("basis_tdiag.hip", r"int64_t blocks = \(nvec \+ 255\) / 256;\s+if \(blocks > 8192\) blocks = 8192;", 1),
    ("basis_tdiag.hip", r"for \(int b0 = 0; b0 < c->B; b0 \+= BT\) \{", 1),
    ("rgcn_internal.h", r"constexpr int kLongRow = 32;", 1),
    ("rgcn_schedule.hip", r"int split = auto_split_k\(d, 2 \* Bd, V, true\);\s+if \(split > 16\) split = 16;", 1),
    ("rgcn_api.hip", r"const size_t s2 = 16 \* 2 \* \(size_t\)c->B \* d \* d;", 1),
    ("rgcn_api.hip", r"const int tiles = \(\(M \+ 127\) / 128\) \* \(\(N \+ 127\) / 128\);\s+if \(tiles >= 192\) return 1;\s+"
                     r"const int target = narrow \? 256 : 512;\s+int s = \(target \+ tiles - 1\) / tiles;\s+"
                     r"const int max_by_k = \(K \+ 127\) / 128;[^\n]*\s+if \(s > max_by_k\) s = max_by_k;\s+if \(s > 64\) s = 64;", 1),
])
def test_host_mirrors_follow_the_kernel_sources(source, pattern, count):
    """The mirrors in tdiag_grid.py are copies of these lines: when one changes, the tables have to be re-derived."""
    with open(os.path.join(CSRC, source)) as f:
        found = len(re.findall(pattern, f.read()))
    assert found == count, "%s holds `%s` %d times, not %d: update tests/tdiag_grid.py's mirror" % (source, pattern, found, count)


def row_dispatch_cells():
    """the (VEC, TPR) instantiations the one dispatch definition of the row kernels, RGCN_LAUNCH_ROWS, names"""
    with open(os.path.join(CSRC, "row_walk.h")) as f:
        text = f.read()
    assert text.count("#define RGCN_LAUNCH_ROWS(") == 1
    return [(int(v), int(t)) for v, t in re.findall(r"kernel<(\d+), (\d+)>", text.split("#define RGCN_LAUNCH_ROWS(")[1])]


def test_the_compiled_variants_are_the_product_of_vecs_and_tprs():
    assert sorted(row_dispatch_cells()) == sorted((vec, tpr) for vec in tg.VECS for tpr in tg.TPRS)      # each cell once
    with open(os.path.join(CSRC, "basis_tdiag.hip")) as f:
        text = f.read()
    for kernel in ("k_tdiag_rows", "k_tdiag_dp"):      # every row launcher goes through it, and launches no other way
        assert len(re.findall(r"RGCN_LAUNCH_ROWS\(%s, vec4, tpr, grid, block, c->stream, a, nlb\);" % kernel, text)) == 1, kernel
        assert not re.findall(kernel + r"<\d", text), kernel
    assert set(re.findall(r"k_tdiag_dcoef<(\d)>", text)) == set(re.findall(r"k_tdiag_dh_join<(\d)>", text)) == {"4", "1"}


# ----------------------------------------------------------------------------- the float32 condition
def float32_passes(c, norm, tag):
    """what tests/test_gpu_tdiag_grid.py's assert_pass asks of the engine, asked of a plain float32 evaluation"""
    dev, g32, g64 = float32_deviation(c, "train", norm)
    for l, (eh, ep) in enumerate(dev, start=1):
        print("%s %s L%d layer %d: float32 vs float64 max abs H %.3e, P %.3e" % (tag, norm, c["L"], l, eh, ep))
        wide = tg.forward_atol(tag, norm, c["L"], "H", l, FWD_ATOL) != FWD_ATOL      # (float32 within the recorded figure)
        assert eh <= (tg.LOCAL_D129_B17_H1_F32 * 1.001 if wide else FWD_ATOL), (tag, norm, l, eh)
        assert tg.forward_atol(tag, norm, c["L"], "P", l, FWD_ATOL) == FWD_ATOL and ep <= FWD_ATOL, (tag, norm, l, ep)
    for n in tdr.weight_names(c["L"])[:-1]:
        assert g32[n].dtype == np.float32
        assert_close(g32[n], g64[n], name="%s %s %s" % (tag, norm, n))


@pytest.mark.parametrize("name", [c["name"] for c in GRID] + list(tg.STRUCTURE_CASES))
def test_float32_passes_the_gpu_checks_under_intended_norms(name):
    float32_passes(tg.case_inputs(tg.ALL_CASES[name], 2), "intended", name)


@pytest.mark.parametrize("name", [c["name"] for c in GRID])
def test_float32_passes_the_gpu_checks_as_the_top_layer_under_local_norms(name):
    float32_passes(tg.case_inputs(tg.ALL_CASES[name], 1), "local", name)


def test_one_buffer_of_one_case_has_a_wider_bound():
    runs = [(c["name"], norm, L) for c in tg.ALL_CASES.values() for norm, L in (("intended", 1), ("intended", 2), ("local", 1))]
    wide = [(r, buf, l) for r in runs for buf in "HP" for l in (1, 2) if tg.forward_atol(*r, buf, l) != FWD_ATOL]
    assert wide == [(("tdiag_d129_B17", "local", 1), "H", 1)]
    assert tg.LOCAL_D129_B17_H1_ATOL == 4 * tg.LOCAL_D129_B17_H1_F32 and FWD_ATOL < tg.LOCAL_D129_B17_H1_F32 < 2e-4


@pytest.mark.parametrize("name", list(tg.LARGE_CASES))
def test_float32_passes_the_gpu_checks_on_the_large_cases(name):
    case = tg.LARGE_CASES[name]
    float32_passes(tg.case_inputs(case, case["L"]), "intended", name)


def test_float32_passes_the_gpu_checks_on_both_graphs_of_the_stale_case():
    c, second, _ = tg.stale_case()
    float32_passes(c, "intended", "stale dP, first graph")
    float32_passes(dict(c, triples=second), "intended", "stale dP, second graph")


def test_float32_passes_the_gpu_checks_with_the_second_coefficients_of_the_stale_table_case():
    c = tg.case_inputs(tg.TDIAG_GRID[tg.STALE_TABLE], 2)
    float32_passes(dict(c, params=tg.second_coefficients(c["params"], c["L"])), "intended", "stale sigmoid table")
