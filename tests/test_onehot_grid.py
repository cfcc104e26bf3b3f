"""The one-hot variant table (tests/onehot_grid.py) covers every compiled variant of the featureless first layer's kernels,
every loop of theirs beyond its first trip and every boundary of their dispatch, and every case's graph holds the rows
and relations it is meant to hold.  No GPU: a later edit of the table that drops a cell fails here, naming the cell."""
import os
import re

import numpy as np
import pytest

import onehot_grid as og

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")
GRID = og.ONEHOT_GRID_LIST


def _cells():
    return [og.cell_of(c) for c in GRID]


# ----------------------------------------------------------------------------- cell coverage
def test_every_vec_and_tpr_is_in_the_table():
    have = {(vec, tpr) for vec, tpr, _, _, _, _ in _cells()}
    missing = [(vec, tpr) for vec in og.VECS for tpr in og.TPRS if (vec, tpr) not in have]
    assert not missing, "one-hot (VEC, TPR) cells without a case: %s" % missing


def test_every_column_pass_count_and_lane_trip_count_is_in_the_table_for_both_vector_widths():
    passes = {(vec, cp) for vec, _, cp, _, _, _ in _cells()}
    missing = [(vec, cp) for vec in og.VECS for cp in (1, 2, 3) if (vec, cp) not in passes]
    assert not missing, "(VEC, long-row column passes) without a case: %s" % missing
    trips = {(vec, lt) for vec, _, _, lt, _, _ in _cells()}
    missing = [(vec, lt) for vec in og.VECS for lt in (1, 2) if (vec, lt) not in trips]
    assert not missing, "(VEC, short-row lane trips) without a case: %s" % missing


def test_a_partial_last_column_pass_with_one_live_lane_is_in_the_table_for_both_vector_widths():
    have = {og.onehot_vec_tpr(c["d"])[0] for c in GRID if og.nvec_of(c["d"]) % og.COLUMN_LANES == 1}
    missing = [vec for vec in og.VECS if vec not in have]
    assert not missing, "VEC without a case of nvec = 128 k + 1: %s" % missing


def test_every_basis_count_is_in_the_table():
    Bs = {c["B"] for c in GRID}
    missing = [B for B in (8, 9, 16, 17, 64) if B not in Bs]
    assert not missing, "basis counts B without a case: %s" % missing
    assert {(og.basis_passes(B), B - 8 * (og.basis_passes(B) - 1)) for B in (8, 9, 16, 17, 64)} == \
        {(1, 8), (2, 1), (2, 8), (3, 1), (8, 8)}


def test_the_shipped_shape_is_in_the_table():
    assert og.SHIPPED in {(c["d"], c["B"]) for c in GRID}, "no case of the shipped gcn_basis shape d = %d, B = %d" % og.SHIPPED
    assert og.cell_of(og.ONEHOT_GRID["onehot_d500_B5"]) == (4, 128, 1, 1, 1, 5)


def test_every_dispatch_boundary_is_in_the_table():
    widths = {c["d"] for c in GRID}
    missing = [(vec, d) for vec in og.VECS for d in og.BOUNDARY_WIDTHS[vec] if d not in widths]
    assert not missing, "dispatch boundaries (VEC, d) without a case: %s" % missing
    # and those widths are the boundaries: nvec 64 | 65 and 128 | 129, or for VEC 1 the last scalar width below them
    assert [og.nvec_of(d) for d in og.BOUNDARY_WIDTHS[4]] == list(og.BOUNDARY_NVECS)
    assert [og.onehot_vec_tpr(d) for d in og.BOUNDARY_WIDTHS[4]] == [(4, 64), (4, 128), (4, 128), (4, 256)]
    assert [og.onehot_vec_tpr(d) for d in og.BOUNDARY_WIDTHS[1]] == [(1, 64), (1, 128), (1, 128), (1, 256)]
    assert og.onehot_vec_tpr(64)[0] == 4 and og.onehot_vec_tpr(128)[0] == 4


def test_the_widest_case_of_each_vector_width_is_named():
    for vec in og.VECS:
        widest = max((c for c in GRID if og.onehot_vec_tpr(c["d"])[0] == vec), key=lambda c: c["d"])
        assert og.WIDEST[vec] == widest["name"]
        assert og.lane_trips(widest["d"]) == 2


def test_mirrors_on_known_configurations():
    assert [og.cell_of(c) for c in GRID[:7]] == [
        (4, 64, 1, 1, 8, 8), (4, 128, 1, 1, 1, 5), (4, 256, 2, 1, 2, 1), (4, 256, 3, 2, 1, 2),
        (1, 64, 1, 1, 1, 8), (1, 128, 1, 1, 2, 8), (1, 256, 3, 2, 3, 1)]
    assert [og.long_blocks(E) for E in (3000, 32768, 32769, 33000)] == [64, 64, 512, 512]
    assert [og.chunk_of(E, E) for E in (3000, 32768, 32769, 33000, 70000)] == [48, 48, 96, 96, 144]
    assert og.chunk_of(3000, 33000) == 48          # a small graph on a context sized for a large one


# ----------------------------------------------------------------------------- hub and structure counts
def test_hub_rows_give_the_slot_walks_their_odd_counts_and_remainders():
    assert og.HUBS == (32, 33, 51, 400) and og.LONG_ROW == 32
    assert og.lane_slots(33) == [5, 4, 4, 4, 4, 4, 4, 4]                   # odd | even of two in flight; 1 | 0 of four
    assert og.lane_slots(51) == [7, 7, 7, 6, 6, 6, 6, 6]                   # remainders 3 | 2 of four in flight
    assert og.lane_slots(400) == [50] * 8
    assert {n % 4 for h in og.HUBS[1:] for n in og.lane_slots(h)} == {0, 1, 2, 3}
    assert {n % 2 for h in og.HUBS[1:] for n in og.lane_slots(h)} == {0, 1}


@pytest.mark.parametrize("name", sorted(og.ONEHOT_GRID))
def test_grid_case_graph_has_its_hub_rows(name):
    c = og.ONEHOT_GRID[name]
    assert (c["V"], c["R"], c["E"], c["hubs"]) == (300, 237, 3000, og.HUBS)
    assert 1 <= c["B"] <= 64
    t = og.case_triples(c)
    assert t.shape == (c["E"], 3) and t.dtype == np.int32
    assert t[:, [0, 2]].min() >= 0 and t[:, [0, 2]].max() < c["V"] and 0 <= t[:, 1].min() and t[:, 1].max() < c["R"]
    slots = og.row_slots(t, c["V"])
    assert slots.sum() == 2 * c["E"]
    for h, n in enumerate(c["hubs"]):
        assert slots[h] == n, "%s: hub %d has %d slots, not %d" % (name, h, slots[h], n)
        assert (t[:, 2] == h).any() and (t[:, 0] == h).any(), "%s: hub %d reached from one direction" % (name, h)
    assert (slots > og.LONG_ROW).sum() >= 3 and (slots == 0).sum() == 0
    assert og.long_blocks(c["E"]) == 64 and og.chunk_of(c["E"], c["E"]) == 48


@pytest.mark.parametrize("name,blocks,chunk", [("many_long_rows", 64, 48), ("capacity_switch", 512, 96)])
def test_dense_graphs_have_more_long_rows_than_their_first_64_workgroups(name, blocks, chunk):
    c = og.STRUCTURE_CASES[name]
    t = og.case_triples(c)
    slots = og.row_slots(t, c["V"])
    assert og.long_blocks(c["E"]) == blocks and og.chunk_of(c["E"], c["E"]) == chunk
    assert c["d"] == 20 and c["B"] <= 9
    long_rows = int((slots > og.LONG_ROW).sum())
    print("%s: %d long rows, longest %d slots" % (name, long_rows, slots.max()))
    if name == "many_long_rows":
        assert long_rows > 4 * 64, "%s: %d long rows do not give every workgroup a fifth row" % (name, long_rows)
        assert long_rows % 64 != 0              # the last round of the `lb += n_long_blocks` loop is a partial one
        assert slots.max() < 100
    else:
        assert 64 < long_rows < 512             # every row long, and most of the 512 workgroups draw none
        assert slots.max() > 240
    per_rel = np.bincount(t[:, 1], minlength=c["R"])
    assert per_rel.min() > 10 * chunk           # every relation spans many chunks


def test_chunk_edges_has_its_relations_at_the_chunk_boundaries():
    c = og.STRUCTURE_CASES["chunk_edges"]
    t = og.case_triples(c)
    chunk = og.chunk_of(c["E"], c["E"])
    per_rel = np.bincount(t[:, 1], minlength=c["R"])
    assert chunk == 48 and c["B"] == 9 and c["R"] == 8
    assert tuple(per_rel[:6]) == (chunk, chunk + 1, 0, 1, 2 * chunk, 2 * chunk + 1) == og.CHUNK_EDGE_COUNTS
    assert per_rel[6] > 1000 and per_rel[7] > 1000 and per_rel.sum() == c["E"]
    # the fixed relations are spread over the edge list, not a prefix of it
    assert np.flatnonzero(t[:, 1] < 6).max() > c["E"] // 2


def test_stale_graphs_silence_the_vertices_that_sent_in_both_directions():
    first, second, quiet = og.stale_graphs()
    assert len(quiet) == 50
    slots = og.row_slots(first, 300)
    assert tuple(slots[:4]) == og.HUBS
    for v in quiet:
        assert (first[:, 0] == v).any() and (first[:, 2] == v).any(), v
    assert not np.isin(second[:, [0, 2]], quiet).any()
    slots2 = og.row_slots(second, 300)
    assert (slots2[quiet] == 0).all()
    assert (slots2 > og.LONG_ROW).sum() >= 10 and ((slots2 > 0) & (slots2 <= og.LONG_ROW)).sum() >= 100
    assert max(len(first), len(second)) == len(first)


def test_case_names_are_unique():
    assert len(og.ONEHOT_GRID) == len(GRID) and len(og.ALL_CASES) == len(GRID) + len(og.STRUCTURE_CASES)


# ----------------------------------------------------------------------------- the mirrors follow the sources
@pytest.mark.parametrize("source,text", [
    ("row_walk.h", "inline int row_lanes(int nvec) { return nvec <= 64 ? 64 : (nvec <= 128 ? 128 : 256); }"),
    ("basis_onehot.hip", "const int tpr = row_lanes(nvec);"),
    ("row_walk.h", "constexpr int BT = 8;"),
    ("row_walk.h", "inline int long_blocks(const rgcn_ctx* c) { return 2 * c->g.E > 65536 ? 512 : 64; }"),
    # (k_onehot_fwd's walk is row_walk.h's; k_onehot_tables keeps a body of its own)
    ("basis_onehot.hip", "__shared__ float red[8][128 * VEC];"),
    ("row_walk.h", "__shared__ float red[8][128 * VEC];"),
    ("basis_onehot.hip", "for (int c0 = 0; c0 < nvec; c0 += 128) {"),
    ("row_walk.h", "for (int c0 = 0; c0 < nvec; c0 += 128) {"),
    ("graph_prep.hip", "g.chunk = std::min(c->chunk, 48 * (int)std::max<int64_t>(1, ((int64_t)M + 65535) / 65536));"),
    ("rgcn_api.hip", "if (2 * f.max_edges > 65536) c->chunk = 48 * (int)((2 * f.max_edges + 65535) / 65536);"),
    ("rgcn_internal.h", "constexpr int kLongRow = 32;"),
])
def test_host_mirrors_follow_the_kernel_sources(source, text):
    """The mirrors in onehot_grid.py are copies of these dispatch lines: when one changes, the table has to be re-derived."""
    with open(os.path.join(CSRC, source)) as f:
        assert text in f.read(), "%s no longer holds `%s`: update tests/onehot_grid.py's mirror" % (source, text)


def test_the_compiled_variants_are_the_product_of_vecs_and_tprs():
    """the one dispatch definition of the row kernels names every (VEC, TPR) cell once, and both row launchers of
    basis_onehot.hip go through it"""
    with open(os.path.join(CSRC, "row_walk.h")) as f:
        macro = f.read().split("#define RGCN_LAUNCH_ROWS(")
    assert len(macro) == 2
    have = [(int(v), int(t)) for v, t in re.findall(r"kernel<(\d+), (\d+)>", macro[1])]
    assert sorted(have) == sorted((vec, tpr) for vec in og.VECS for tpr in og.TPRS)
    with open(os.path.join(CSRC, "basis_onehot.hip")) as f:
        text = f.read()
    for kernel in ("k_onehot_fwd", "k_onehot_tables"):
        assert len(re.findall(r"RGCN_LAUNCH_ROWS\(%s, vec4, tpr, grid, block, c->stream, a, nlb\);" % kernel, text)) == 1, kernel
        assert not re.findall(kernel + r"<\d", text), kernel
