"""The full-graph table (tests/fullgraph_grid.py): every case is in the regime it claims, fg_local's relabelled row is the
two runs it says, the source lines the regime rests on are still in the sources, and a plain float32 numpy evaluation of
the float64 restatement passes, on every case's inputs, the very checks tests/test_gpu_fullgraph_grid.py applies -- the
condition its bounds rest on (tests/test_highway_grid.py's convention).  No GPU."""
import functools
import os

import numpy as np
import pytest

import fullgraph_grid as fg
import giant_grid as gg
import highway_grid as hg
import kernel_grid as kg
import local_norm_reference as lnr
from tdiag_grid import auto_split_k

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relationprediction_amd", "csrc")
CASES = fg.FULLGRAPH_CASES


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = fg.case_inputs(CASES[name])
    for a in [c["triples"], c["dcodes"]] + list(c["masks"]) + list(c["params"].values()):
        a.setflags(write=False)
    return c


def test_the_table_is_the_issue_s():
    assert [c["name"] for c in fg.FULLGRAPH_GRID] == ["fg_highway", "fg_highway_L3", "fg_highway_wide", "fg_highway_vec1",
                                                      "fg_highway_basis", "fg_local", "fg_out", "fg_all"]
    base = dict(kind="block", V=3000, R=237, E=33000, hubs=(33, 400, 2048, 2049, 4096, 4097, 6000), nb=4, d=20, L=2,
                skip="none", norm="intended", code_dim=0, relabel=False)
    differs = {"fg_highway": dict(skip="highway"), "fg_highway_L3": dict(skip="highway", L=3),
               "fg_highway_wide": dict(skip="highway", nb=129, d=516), "fg_highway_vec1": dict(skip="highway", nb=3, d=9),
               "fg_highway_basis": dict(skip="highway", kind="basis", nb=2), "fg_local": dict(norm="local", relabel=True),
               "fg_out": dict(code_dim=8), "fg_all": dict(skip="highway", norm="local", relabel=True, code_dim=8)}
    for name, c in CASES.items():
        want = dict(base, **differs[name])
        assert {k: c[k] for k in want} == want, name
        assert c["max_edges"] == c["E"] and not c["drop_free_edge"]
    assert set(fg.EVAL_CASES) | set(fg.FORM_CASES) | set(fg.LOST_PIECE_CASES) <= set(CASES)
    assert all(CASES[n]["skip"] == "highway" for n in fg.LOST_PIECE_CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_in_the_regime_it_claims(name):
    c = CASES[name]
    t = fg.case_triples(c)
    E = len(t)
    assert t.shape == (33000, 3) and t.dtype == np.int32 and 2 * E == 66000 > gg.GIANT_MESSAGES
    assert t[:, [0, 2]].min() >= 0 and t[:, [0, 2]].max() < c["V"] and 0 <= t[:, 1].min() and t[:, 1].max() < c["R"]
    slots = kg.row_slots(t, c["V"])
    assert tuple(slots[:len(gg.HUBS)]) == gg.HUBS
    assert sorted(np.flatnonzero(slots > kg.LONG_ROW).tolist()) == list(range(len(gg.HUBS))), "a long row that is no hub"
    # the cut: on for the block kind (four giant rows, ten pieces, last pieces of 1, 2048, 1 and 1904 slots), never for basis
    assert gg.giant_on(E, c["kind"]) == (c["kind"] == "block")
    assert sorted(gg.giant_rows(c, slots)) == fg.GIANT_ROWS[name]
    if c["kind"] == "block":
        assert [gg.pieces(n) for n in fg.GIANT_ROWS[name]] == [2, 2, 3, 3]
        assert [gg.last_piece(n) for n in fg.GIANT_ROWS[name]] == [1, 2048, 1, 1904]
        assert sum(gg.pieces(n) for n in fg.GIANT_ROWS[name]) <= gg.piece_cap(c["max_edges"])
        assert len(fg.GIANT_ROWS[name]) < gg.giant_cap(c["max_edges"])
        assert gg.finish_trips(len(fg.GIANT_ROWS[name])) == 1
        assert c["d"] // c["nb"] in kg.BLOCK_SIZES
        assert gg.rows_long_wg(E) == 257
        # db_emb's partials: the row kernel would leave them itself on a plain context (k_colsum_giant_rows for the giant
        # rows); a highway context turns that off and highway_join supplies them
        assert gg.colsum_in_kernel(c["V"], c["d"], E, c["max_edges"], c["nb"])
    # the full-graph relation chunk, block and basis alike; the small graph of item 6 is on the other side of everything
    assert gg.relation_chunk(E, gg.context_chunk(c["max_edges"])) == 96
    small = fg.small_triples(c)
    assert len(small) == 3000 and not gg.giant_on(len(small), c["kind"])
    assert gg.relation_chunk(len(small), gg.context_chunk(c["max_edges"])) == 48
    assert kg.row_slots(small, c["V"]).max() == 400


def test_the_cells_the_table_names():
    wide, vec1 = CASES["fg_highway_wide"], CASES["fg_highway_vec1"]
    # highway CL = 256 with GW 32, the piece loop's second column chunk, one trip of the finish loop
    assert hg.cell_of(wide)[:3] == (4, 256, 1) and kg.rows_group_width(wide["nb"]) == 32
    assert (gg.piece_loop_chunks(wide["d"]), gg.finish_loop_chunks(wide["d"])) == (2, 1)
    # gemm_highway_dw and gemm_self_dw, split over K = V = 3000 rows, one after the other through the same slabs
    assert auto_split_k(wide["d"], wide["d"], wide["V"], False) == 21
    # the scalar forms of both
    assert gg.vec_width(vec1["d"]) == hg.vec_of(vec1["d"]) == 1 and kg.empty_bands(vec1["nb"]) == [0, 1, 3, 4, 6]
    assert all(gg.vec_width(c["d"]) == 4 for c in CASES.values() if c is not vec1)
    assert CASES["fg_highway_L3"]["L"] == 3 and all(c["L"] == 2 for n, c in CASES.items() if n != "fg_highway_L3")


@pytest.mark.parametrize("name", ["fg_local", "fg_all"])
def test_the_relabelled_row_is_two_runs(name):
    """Row 5 (4097 slots): 2049 arriving edges of one relation, then 2048 leaving ones.  The first run crosses the piece
    boundary at slot 2048, the second fills the rest of piece 2 and the one slot of piece 3.  Under `local` their norms
    are float32(1) / 2049 and / 2048.  Row 6 (6000 slots) stays spread over the relations."""
    c = CASES[name]
    t = fg.case_triples(c)
    E, R = len(t), c["R"]
    inc, rel2 = fg.row_slot_order(t, R, fg.HUB_LOCAL)
    q = fg.relabel_relation(c)
    assert fg.runs_of(rel2) == [2049, 2048] and rel2[0] == q and rel2[-1] == R + q
    assert (inc[:2049] < E).all() and (inc[2049:] >= E).all() and (np.diff(inc) > 0).all()
    assert fg.runs_of(rel2)[0] > gg.GIANT_ROW          # the arriving run ends in the second piece
    n_f, n_b = lnr.message_norms_f32(t, c["V"], "local")
    assert n_f.dtype == n_b.dtype == np.float32
    assert (n_f[inc[:2049]] == np.float32(1) / np.float32(2049)).all()
    assert (n_b[inc[2049:] - E] == np.float32(1) / np.float32(2048)).all()
    # the other graph of the pair: the same edges, their own relations
    plain = gg.giant_triples(c)
    assert np.array_equal(plain[:, [0, 2]], t[:, [0, 2]]) and (plain[:, 1] != t[:, 1]).sum() > 4000
    runs = fg.runs_of(fg.row_slot_order(t, R, fg.HUB_LOST)[1])
    assert sum(runs) == 6000 and len(runs) > 400 and max(runs) < 40
    # a piece boundary of that row falls inside a run or between two: either way norms change along the pieces
    assert len(set(np.concatenate([n_f, n_b]).tolist())) > 20


@pytest.mark.parametrize("source,text", [
    ("graph_prep.hip", "g.giant_on = c->kind == RGCN_KIND_BLOCK && c->world == 1 && M > 65536;"),
    # the third branch of bwd_block_rows
    ("rgcn_schedule.hip", "const bool minibatch = c->world == 1 && c->g.E <= 65536;"),
    ("rgcn_schedule.hip", "if (minibatch && c->use_aux) {"),
    ("rgcn_schedule.hip", "} else if (minibatch) {"),
    ("rgcn_schedule.hip", "c->dw_pending = side.active;"),
    ("rgcn_schedule.hip", "if (c->dw_pending) {       // the previous layer's weight-gradient kernel reads the D buffer this layer may overwrite"),
    # the highway branch of fwd_layer_partial and of bwd_layer_partial
    ("rgcn_schedule.hip", "float* dst = c->world > 1 ? c->exch : c->highway ? c->hw_N[l] : c->H[l];"),
    ("rgcn_schedule.hip", "a.out2 = nullptr; a.gate = nullptr; a.drop2 = make_drop(c, l - 1, false);"),
    ("rgcn_schedule.hip", "RGCN_TRY(bwd_highway_open(c, s));"),
    ("rgcn_schedule.hip", "RGCN_TRY(highway_join(c, a.out, c->self_buf, c->hw_carry, l == 1 ? s.Hin : nullptr, &nparts));"),
    ("rgcn_schedule.hip", "if (l == 1) c->colsum_parts = nparts;      // db_emb: bwd_end adds them"),
    ("rgcn_schedule.hip", "StreamScope side(c, 1);\n    RGCN_TRY(gemm_f32(c, \"gemm_highway_dw\", false, false, d, d, V, s.Hin, d, c->hw_dz[l & 1], d, s.lb->gwhw, d,"),
    # the output layer's backward pass ahead of the stack's
    ("rgcn_schedule.hip", "if (l == c->L && c->out_layer) RGCN_TRY(output_forward(c));"),
])
def test_the_regime_s_source_lines_are_still_there(source, text):
    with open(os.path.join(CSRC, source)) as f:
        assert text in f.read(), "%s no longer holds `%s`: re-derive tests/fullgraph_grid.py" % (source, text)


def test_the_highway_branch_comes_before_the_pending_join_and_the_layer_form():
    """bwd_layer_partial: the highway epilogue arguments and bwd_highway_open, then the dw_pending join, then the layer's
    form (bwd_block_rows), then highway_join -- the order tests/test_gpu_fullgraph_grid.py's item 6 is about"""
    with open(os.path.join(CSRC, "rgcn_schedule.hip")) as f:
        text = f.read()
    body = text[text.index("rgcn_status bwd_layer_partial(rgcn_ctx* c, int l) {"):]
    body = body[:body.index("\n}\n")]
    marks = ["if (c->highway) {", "RGCN_TRY(bwd_highway_open(c, s));", "if (c->dw_pending) {", "RGCN_TRY(stream_join(c, 0));",
             "case FORM_BLOCK_ROWS: RGCN_TRY(bwd_block_rows(c, s, &defer_joins)); break;", "RGCN_TRY(highway_join(",
             "if (!defer_joins) RGCN_TRY(stream_join(c, 1));"]
    at = [body.index(m) for m in marks]
    assert at == sorted(at), list(zip(marks, at))


# ----------------------------------------------------------------------------- the float32 condition
@pytest.mark.parametrize("name", [c["name"] for c in fg.FULLGRAPH_GRID])
def test_float32_passes_the_gpu_checks(name):
    """What item 1 of tests/test_gpu_fullgraph_grid.py asks of the engine, asked of a plain float32 evaluation in one
    summation order on the same inputs: every activation within FWD_ATOL of float64, every gradient within assert_close's
    defaults of the float64 reverse mode at the float32 activations.  It passes on every tensor of every case (6000-term
    float32 sums included), so no bar other than the features' own is needed."""
    c = inputs(name)
    ref = fg.reference_forward(c)
    a32 = fg.reference_forward(c, dtype=np.float32)
    for _, a in fg.compared_activations(c, a32):
        assert a.dtype == np.float32
    g32 = fg.reference_backward(c, a32, dtype=np.float32)
    g64 = fg.reference_backward(c, a32)
    assert all(g.dtype == np.float32 for g in g32.values())
    fwd, bwd = fg.check_against_float64(c, a32, g32, ref, g64, tag="float32 ")
    print("%s float32 restatement against float64: %s | %s" % (name, "; ".join(fwd), "; ".join(bwd)))


@pytest.mark.parametrize("name", fg.LOST_PIECE_CASES)
def test_the_check_sees_a_lost_piece(name):
    """Item 8 without a GPU: the float32 restatement held to a mirror whose N_1 lacks the last piece of the 6000-slot row
    fails the check (and passes it against the true mirror: test_float32_passes_the_gpu_checks)."""
    c = inputs(name)
    ref = fg.reference_forward(c)
    lost, moved = fg.lost_piece_mirror(c, ref)
    print("%s: row %d of N_1 moves by %.3e without its last piece" % (name, fg.HUB_LOST, moved))
    assert moved > 10 * fg.FWD_ATOL
    with pytest.raises(AssertionError, match="N1 against float64"):
        fg.check_forward(c, fg.reference_forward(c, dtype=np.float32), lost)
