"""The giant-row table (tests/giant_grid.py) reaches every boundary of the giant-row cut, and every case's graph holds the
rows it is meant to cut.  No GPU: a later edit of the table, or of a formula it mirrors, fails here and names what went."""
import os

import numpy as np
import pytest

import giant_grid as gg
import kernel_grid as kg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")
CASES = gg.GIANT_CASES


def _slots(name, _cache={}):
    if name not in _cache:
        c = CASES[name]
        _cache[name] = kg.row_slots(gg.giant_triples(c), c["V"])
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_graph_has_its_rows(name):
    """Every hub row has exactly its stated slots and is reached from both directions, nothing else has 2048 slots or
    more, the ids are in range, and the piece and giant-row lists of the context hold the graph's."""
    c = CASES[name]
    t = gg.giant_triples(c)
    E = gg.case_edges(c)
    assert t.shape == (E, 3) and t.dtype == np.int32 and E <= c["max_edges"]
    assert t[:, [0, 2]].min() >= 0 and t[:, [0, 2]].max() < c["V"] and 0 <= t[:, 1].min() and t[:, 1].max() < c["R"]
    slots = _slots(name)
    assert slots.sum() == 2 * E
    nh = len(c["hubs"])
    for h, n in enumerate(c["hubs"]):
        assert slots[h] == n, "%s: hub %d has %d slots, not %d" % (name, h, slots[h], n)
        assert (t[:, 2] == h).any() and (t[:, 0] == h).any(), "%s: hub %d reached from one direction" % (name, h)
    assert slots[nh:].max() < gg.GIANT_ROW, "%s: a row that is no hub has %d slots" % (name, slots[nh:].max())
    want = [n for n in c["hubs"] if n > gg.GIANT_ROW] if gg.giant_on(E) else []
    assert sorted(gg.giant_rows(c, slots)) == sorted(want)
    assert sum(gg.pieces(n) for n in want) <= gg.piece_cap(c["max_edges"]), name
    assert len(want) < gg.giant_cap(c["max_edges"]), name
    assert c["d"] % c["nb"] == 0 and c["d"] // c["nb"] in kg.BLOCK_SIZES and c["nb"] <= kg.MAX_BLOCKS, name


def test_standard_shape_has_exactly_the_seven_long_rows():
    for name, c in CASES.items():
        if c["hubs"] == gg.HUBS:
            slots = _slots(name)
            assert sorted(np.flatnonzero(slots > kg.LONG_ROW).tolist()) == list(range(len(gg.HUBS))), name
            assert [gg.pieces(n) for n in gg.HUBS] == [0, 0, 0, 2, 2, 3, 3]
            assert [gg.last_piece(n) for n in gg.HUBS] == [0, 0, 0, 1, 2048, 1, 1904]


def test_the_cut_is_on_everywhere_but_below_the_switch():
    off = [n for n, c in CASES.items() if not gg.giant_on(gg.case_edges(c), c["kind"])]
    assert off == ["giant_switch_off"]
    on, below = CASES["giant_switch_on"], CASES["giant_switch_off"]
    assert 2 * gg.case_edges(on) == gg.GIANT_MESSAGES + 2 and 2 * gg.case_edges(below) == gg.GIANT_MESSAGES
    # the same graph but for one edge that touches no hub, the same weights, masks and upstream gradient
    t, k = kg.grid_triples(on), gg.free_edge(on)
    assert t[k, 0] >= len(gg.HUBS) and t[k, 2] >= len(gg.HUBS)
    assert not ((t[k + 1:, 0] >= len(gg.HUBS)) & (t[k + 1:, 2] >= len(gg.HUBS))).any()
    np.testing.assert_array_equal(np.delete(gg.giant_triples(on), k, axis=0), gg.giant_triples(below))
    assert {x: on[x] for x in on if x not in ("name", "drop_free_edge")} == \
        {x: below[x] for x in below if x not in ("name", "drop_free_edge")}
    # below the switch the cut rows are ordinary long rows, and the relation chunk is half as long
    assert (_slots("giant_switch_off") > gg.GIANT_ROW).sum() == 4 and gg.giant_rows(below) == []
    cap = gg.context_chunk(on["max_edges"])
    assert (gg.relation_chunk(gg.case_edges(on), cap), gg.relation_chunk(gg.case_edges(below), cap)) == (96, 48)


def test_every_block_size_group_width_and_vector_width_is_in_the_table():
    cells = {kg.block_cell(c["nb"], c["d"])[:2] for c in CASES.values() if c["float64"]}
    assert {sd for sd, _ in cells} == set(kg.BLOCK_SIZES)
    assert {gw for _, gw in cells} == set(kg.GROUP_WIDTHS)
    assert {gg.vec_width(c["d"]) for c in CASES.values() if c["float64"]} == {1, 4}
    assert kg.empty_bands(CASES["giant_sd8_nb3"]["nb"]) == [0, 1, 3, 4, 6]


def test_every_piece_boundary_and_loop_trip_is_in_the_table():
    float64 = [c for c in CASES.values() if c["float64"]]
    last = {gg.last_piece(n) for c in float64 for n in gg.giant_rows(c)}
    assert 1 in last and gg.GIANT_ROW in last and any(1 < n < gg.GIANT_ROW for n in last), sorted(last)
    assert any(gg.GIANT_ROW in c["hubs"] for c in float64), "no row of exactly %d slots (the longest uncut row)" % gg.GIANT_ROW
    assert {gg.finish_trips(len(gg.giant_rows(c))) for c in float64 if not c["drop_free_edge"]} == {1, 2}
    assert {gg.piece_loop_chunks(c["d"]) for c in float64} == {1, 2, 3}
    assert {gg.finish_loop_chunks(c["d"]) for c in float64} == {1, 2}
    # both vector widths on the finish loop's second trip (the float4 one in the bitwise form comparison only)
    assert {gg.vec_width(c["d"]) for c in CASES.values() if gg.finish_loop_chunks(c["d"]) == 2} == {1, 4}


def test_both_outcomes_of_the_column_sum_condition_are_in_the_table():
    outcome = {n: gg.colsum_in_kernel(c["V"], c["d"], gg.case_edges(c), c["max_edges"], c["nb"]) for n, c in CASES.items()}
    assert [n for n, inside in outcome.items() if not inside] == ["giant_colsum_fallback"]
    c = CASES["giant_colsum_fallback"]
    assert gg.giant_cap(c["max_edges"]) == 1172 and gg.colsum_part_floats(c["V"], c["d"]) == 1076 * c["d"]
    assert gg.colsum_in_kernel(c["V"], c["d"], c["E"], c["E"], c["nb"]), "the same graph in a context of its own size"


def test_counting_cases():
    c = CASES["giant_all_long"]
    slots = _slots("giant_all_long")
    assert slots.min() > kg.LONG_ROW, "a row of %d slots is not long" % slots.min()
    # more long rows than the two-kernel form has long-row workgroups: its list walk wraps
    assert (slots > kg.LONG_ROW).sum() - len(gg.giant_rows(c)) > gg.combine_long_blocks(c["E"]) == 256
    c = CASES["giant_many"]
    assert len(gg.giant_rows(c)) == 66 > gg.FINISH_GRID and gg.giant_cap(c["max_edges"]) == 137
    assert sum(c["hubs"]) == 137379 <= c["E"]
    assert gg.rows_long_wg(c["E"]) == 1024 and gg.rows_long_wg(CASES["giant_sd5_nb4"]["E"]) == 257


@pytest.mark.parametrize("source,text", [
    ("rgcn_internal.h", "constexpr int kGiantRow = 2048;"),
    ("rgcn_internal.h", "  int chunk = 48;                        // messages per relation chunk (capacity-scaled"),
    ("graph_prep.hip", "g.giant_on = c->kind == RGCN_KIND_BLOCK && c->world == 1 && M > 65536;"),
    ("graph_prep.hip", "const int np = (end - beg + kGiantRow - 1) / kGiantRow;"),
    ("graph_prep.hip", "g.giant_cap = (int32_t)(M / kGiantRow + 1);"),
    ("graph_prep.hip", "g.piece_cap = (int32_t)(2 * (M / kGiantRow) + 2);"),
    ("graph_prep.hip", "g.chunk = std::min(c->chunk, 48 * (int)std::max<int64_t>(1, ((int64_t)M + 65535) / 65536));"),
    ("rgcn_api.hip", "if (2 * f.max_edges > 65536) c->chunk = 48 * (int)((2 * f.max_edges + 65535) / 65536);"),
    ("rgcn_api.hip", "c->colsum_part_floats = ((V + 3) / 4 + 1024 + 2 + ((V + 3) / 4 + 1024) / 32 + 2) * d;"),
    ("block_rows.hip", "const int64_t want = (2 * c->g.E) / 256;"),
    ("block_rows.hip", "a.n_long_wg = c->g.E > 0 ? (int)std::max<int64_t>(32, std::min<int64_t>(1024, want)) : 0;"),
    ("block_rows.hip", "const int quantum = 4 * (64 / rows_group_width(c));"),
    ("block_rows.hip", "const int rpw = std::max(quantum, std::min(256, 64 / quantum * quantum));"),
    ("block_rows.hip", "const int n_row_wg = (c->V + a.rows_per_wg - 1) / a.rows_per_wg;"),
    ("block_rows.hip", "const int grid = 8 * (a.n_long_wg + n_row_wg);"),
    ("block_rows.hip", "const int giant_parts = giant ? c->g.giant_cap : 0;"),
    ("block_rows.hip", "(size_t)(grid / 8 + giant_parts) * c->d <= c->colsum_part_floats) {"),
    ("block_rows.hip", "const int end = min(a.row_ptr[v + 1], beg + kGiantRow);"),
    ("elementwise.hip", "constexpr int kLongBlocksMin = 64;"),
    ("elementwise.hip", "int64_t want = 2 * c->g.E / 1024;"),
    ("elementwise.hip", "n_long_blocks = (int)(want < kLongBlocksMin ? kLongBlocksMin : (want > 1024 ? 1024 : want));"),
    ("elementwise.hip", "n_long_blocks *= 4;"),
    ("elementwise.hip", "for (int c0 = 0; c0 < nvec; c0 += 128) {"),
    ("elementwise.hip", "for (int cidx = threadIdx.x; cidx < nvec; cidx += 256) {"),
    ("elementwise.hip", "for (int i = blockIdx.x; i < n; i += gridDim.x) {"),
    ("elementwise.hip", "if (vec4) hipLaunchKernelGGL((k_combine_giant_finish<4>), dim3(64), dim3(256), 0, c->stream, a);"),
    ("elementwise.hip", "else hipLaunchKernelGGL((k_combine_giant_finish<1>), dim3(64), dim3(256), 0, c->stream, a);"),
])
def test_host_mirrors_follow_the_kernel_sources(source, text):
    """The mirrors in giant_grid.py are copies of these lines: when one changes, the table has to be re-derived."""
    with open(os.path.join(CSRC, source)) as f:
        assert text in f.read(), "%s no longer holds `%s`: update tests/giant_grid.py's mirror" % (source, text)


def test_mirrors_on_known_configurations():
    assert [gg.pieces(n) for n in (2047, 2048, 2049, 4096, 4097, 6000)] == [0, 0, 2, 2, 3, 3]
    assert [gg.last_piece(n) for n in (2049, 4096, 4097, 6000)] == [1, 2048, 1, 1904]
    assert (gg.giant_on(32768), gg.giant_on(32769), gg.giant_on(10 ** 6, "basis"), gg.giant_on(10 ** 6, world=2)) == \
        (False, True, False, False)
    assert (gg.giant_cap(33000), gg.piece_cap(33000), gg.giant_cap(272115), gg.piece_cap(272115)) == (33, 66, 266, 532)
    assert [gg.rows_long_wg(E) for E in (0, 1, 4096, 33000, 272115)] == [0, 32, 32, 257, 1024]
    assert [gg.combine_long_blocks(E) for E in (3000, 33000, 272115, 10 ** 6)] == [256, 256, 2124, 4096]
    assert [gg.rows_per_wg(nb) for nb in (4, 100, 129, 257)] == [64, 64, 64, 64]
    assert [gg.finish_trips(n) for n in (0, 1, 64, 65, 66)] == [0, 1, 1, 2, 2]
    assert [(gg.vec_width(d), gg.piece_loop_chunks(d), gg.finish_loop_chunks(d)) for d in (9, 20, 516, 257, 1028)] == \
        [(1, 1, 1), (4, 1, 1), (4, 2, 1), (1, 3, 2), (4, 3, 2)]
    assert (gg.context_chunk(15000), gg.context_chunk(33000), gg.context_chunk(272115)) == (48, 96, 432)
    assert gg.relation_chunk(15000, 432) == 48 and gg.relation_chunk(272115, 432) == 432
