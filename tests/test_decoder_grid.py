"""The decoder's kernel-variant table (tests/decoder_grid.py) covers every compiled variant of decoder_compute, and every
case's batch holds the rows and relations it claims.  No GPU: a later edit of the table that drops a cell fails here,
naming the cell."""
import os

import numpy as np
import pytest

import decoder_grid as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relationprediction_amd", "csrc")


def _cells(stage):
    return {dg.cell_of(c)[stage] for c in dg.DECODER_GRID}


def test_every_energy_kernel_variant_is_in_the_table():
    have = _cells(0)
    missing = [cell for cell in dg.ENERGY_CELLS if cell not in have]
    assert not missing, "energy / relation-partial variants without a case: %s" % missing


def test_every_entity_gradient_variant_is_in_the_table():
    have = _cells(1)
    missing = [cell for cell in dg.ENTITY_CELLS if cell not in have]
    assert not missing, "entity-gradient variants without a case: %s" % missing


def test_every_variant_meets_long_rows():
    """k_dec_long_finish<VEC> follows the vector width: both widths need a case whose batch has pieces."""
    have = {dg.vec_width(c["d"]) for c in dg.DECODER_GRID if c["n"] > 1}
    assert have == {1, 4}, "k_dec_long_finish widths without a long row: %s" % sorted({1, 4} - have)


def test_dispatch_boundaries_are_in_the_table():
    # plain cases: the shipped relation count, an untiled batch, unscaled weights
    ds = {c["d"] for c in dg.DECODER_GRID if c["R"] == dg.R_DEC and c["rate"] is None and not c["saturate"]}
    missing = [d for d in (20, 256, 260, 500, 512, 516, 1024, 1028, 9, 63, 66, 126, 130, 255, 258, 1030) if d not in ds]
    assert not missing, "widths d at the dispatch boundaries without a case: %s" % missing
    # the line form: one partial band; eight bands in one pass; two, three and five passes
    assert any(dg.bands(d) == 1 and d % dg.LINE for d in ds if dg.vec_width(d) == 4)
    passes = {dg.band_passes(d) for d in ds if dg.vec_width(d) == 4}
    missing = [p for p in (1, 2, 3, 5) if p not in passes]
    assert not missing, "band-pass counts of k_dec_entity_lines without a case: %s" % missing
    assert any(dg.bands(d) == 8 for d in ds if dg.vec_width(d) == 4)
    # k_dec_rel_partial: three column passes at VEC 4, nine at VEC 1
    assert {dg.rel_partial_passes(d) for d in ds if dg.energy_cell(d)[0] == "energy"} >= {3, 9}


def test_relation_table_boundaries_are_in_the_table():
    have = {(c["d"], c["R"]) for c in dg.DECODER_GRID}
    missing = [k for k in ((20, 512), (20, 513), (260, 512), (260, 513), (1028, 513)) if k not in have]
    assert not missing, "(d, R) cases at the 64 KB LDS bound without a case: %s" % missing
    assert dg.relation_lds(512) and not dg.relation_lds(513)


def test_saturation_and_tiled_batches_are_in_the_table():
    assert any(c["saturate"] and c["saturate"] > 90 for c in dg.DECODER_GRID), "no saturated-energy case"
    tiled = {(c["rate"], c["n"] > 1) for c in dg.DECODER_GRID if c["rate"] is not None}
    missing = [k for k in ((10, True), (1, True), (0, True)) if k not in tiled]
    assert not missing, "tiled batches (rate, n > 1) without a case: %s" % missing
    assert any(c["n"] == 1 and dg.copies(c) == 1 for c in dg.DECODER_GRID), "no single-triple (untiled) sampler batch"


def test_train_step_subset():
    cells = {dg.cell_of(dg.DECODER_CASES[n]) for n in dg.TRAIN_STEP_CASES}
    energy = {e for e, _ in cells}
    entity = {f for _, f in cells}
    assert {("energy_rel", 1, 2), ("energy_rel", 1, 4), ("energy", 1, None), ("energy", 4, None)} <= energy
    assert {("lines", True), ("lines", False), ("rows", 1, 128), ("rows", 1, 256)} <= entity
    assert all(dg.DECODER_CASES[n]["rate"] is None for n in dg.TRAIN_STEP_CASES)


@pytest.mark.parametrize("name", sorted(dg.DECODER_CASES))
def test_case_batch_has_its_counts(name):
    """Counted over both sides of the batch (the first copies of a tiled one): every entity row and relation count of
    the table, the hub reached as subject and as object, s == o triples, ids in range."""
    c = dg.DECODER_CASES[name]
    X, Y = dg.case_batch(c)
    assert X.shape == (c["n"], 3) and X.dtype == np.int32
    assert X[:, [0, 2]].min() >= 0 and X[:, [0, 2]].max() < c["V"] and X[:, 1].min() >= 0 and X[:, 1].max() < c["R"]
    assert (Y is None) == (c["rate"] is not None)
    if c["n"] == 1:
        return
    inc = dg.incidences(X, c["V"])
    assert inc.sum() == 2 * c["n"]
    for e, want in enumerate(dg.ENTITY_COUNTS):
        assert inc[e] == want, "%s: entity %d has %d incidences, not %d" % (name, e, inc[e], want)
    assert inc[len(dg.ENTITY_COUNTS):].max() <= dg.LONG_ROW, "%s: an ordinary entity took a long row" % name
    assert [dg.pieces(n) for n in dg.ENTITY_COUNTS] == [0, 0, 0, 1, 1, 2, 3]
    hub = len(dg.ENTITY_COUNTS) - 1
    assert ((X[:, 0] == hub) & (X[:, 2] != hub)).any() and ((X[:, 2] == hub) & (X[:, 0] != hub)).any(), name
    assert (X[:, 0] == X[:, 2]).sum() >= dg.SELF_EDGES + 1 and ((X[:, 0] == hub) & (X[:, 2] == hub)).any(), name
    rc = np.bincount(X[:, 1], minlength=c["R"])
    want = dg.rel_counts(c)
    assert list(rc[:len(want)]) == list(want), "%s: relation counts %s, not %s" % (name, list(rc[:len(want)]), want)
    # decoded (x copies): an empty relation, a partial chunk, a chunk boundary hit exactly and one passed by at most one
    # copy, and a relation of at least five chunks (k_dec_rel_reduce's 4-way turn and its tail)
    k = dg.copies(c)
    decoded = [n * k for n in want]
    assert 0 in decoded and any(0 < n < dg.CHUNK for n in decoded)
    assert any(n and n % dg.CHUNK == 0 for n in decoded)
    assert any(n > dg.CHUNK and 0 < n % dg.CHUNK <= k for n in decoded)
    assert max(dg.chunks(n) for n in decoded) >= 5
    if Y is not None:
        assert 0 < Y.sum() < len(Y)


def test_host_tiled_layout():
    X, _ = dg.case_batch(dg.DECODER_CASES["dec_d20_rate10"])
    T, Y = dg.host_tiled(X, 10, dg.V_DEC, 1)
    n = len(X)
    assert T.shape == (11 * n, 3) and np.array_equal(T[:n], X) and (Y[:n] == 1).all() and not Y[n:].any()
    assert np.array_equal(T[:, 1], np.tile(X[:, 1], 11))
    assert not ((T[n:, 0] != np.tile(X, (10, 1))[:, 0]) & (T[n:, 2] != np.tile(X, (10, 1))[:, 2])).any()


def test_case_shapes_are_valid_configurations():
    for name, c in dg.DECODER_CASES.items():
        assert c["d"] % c["nb"] == 0 and c["d"] // c["nb"] in dg.BLOCK_SIZES and c["nb"] <= dg.MAX_BLOCKS, name
        assert c["V"] % 8 != 0 and c["L"] == 1 and c["kind"] == "block", name
        assert c["R"] <= c["V"], name           # relation ids index W_relation, which has V rows


# ----------------------------------------------------------------------------- row weights and the tiled order
def test_weighted_cases_cover_every_weighted_energy_cell():
    assert len(dg.WEIGHTED_ENERGY_CELLS) == 16 and len(set(dg.WEIGHTED_ENERGY_CELLS)) == 16
    have = {dg.weighted_energy_cell(dg.DECODER_CASES[n]) for n in dg.WEIGHTED_CASES}
    missing = [cell for cell in dg.WEIGHTED_ENERGY_CELLS if cell not in have]
    assert not missing, "WEIGHTED energy variants (cell, order) without a case: %s" % missing
    for n in dg.WEIGHTED_CASES:
        c = dg.DECODER_CASES[n]
        assert dg.weighted_cell_of(c) == dg.cell_of(c) + (True,) and dg.weighted_cell_of(c, False)[2] is False
    # the untiled one per cell, the saturated energies, the global relation band, every batch the sampler tiled
    plain = {dg.energy_cell(dg.DECODER_CASES[n]["d"]) for n in dg.WEIGHTED_CASES if not dg.is_tiled(dg.DECODER_CASES[n])}
    assert plain == set(dg.ENERGY_CELLS)
    assert "dec_d20_sat" in dg.WEIGHTED_CASES and "dec_d260_R513" in dg.WEIGHTED_CASES
    assert {c["name"] for c in dg.DECODER_GRID if dg.is_tiled(c)} <= set(dg.WEIGHTED_CASES)
    assert len(set(dg.WEIGHTED_CASES)) == len(dg.WEIGHTED_CASES) == 19


def test_tiled_cases_cover_every_variant():
    tiled = [c for c in dg.DECODER_GRID if dg.is_tiled(c)]
    have = {dg.energy_cell(c["d"]) for c in tiled}
    missing = [cell for cell in dg.ENERGY_CELLS if cell not in have]
    assert not missing, "energy variants without a tiled case: %s" % missing
    passes = {dg.band_passes(c["d"]) for c in tiled if dg.vec_width(c["d"]) == 4}
    assert {1, 2} <= passes and max(passes) >= 3, "band passes of the line form under the tiled order: %s" % sorted(passes)
    # both unfused kernels: k_dec_energy<1> / <4>, each followed by k_dec_rel_partial walking the tiled permr
    assert {("energy", 1, None), ("energy", 4, None)} <= have
    assert all(dg.copies(c) == c["rate"] + 1 for c in tiled)
    assert all(dg.is_tiled(dg.DECODER_CASES[n]) and dg.DECODER_CASES[n]["n"] == 1500 for n in dg.RELATION_ROW_CASES)
    assert {dg.energy_cell(dg.DECODER_CASES[n]["d"]) for n in dg.RELATION_ROW_CASES} == \
        {("energy_rel", 1, 2), ("energy_rel", 4, 2), ("energy", 4, None)}


def test_lone_rows_mirror_the_two_per_turn_walk():
    """the walk itself, triple by triple: wave w of a chunk starts at w and takes j and j + 4, then j += 8"""
    for count in (1, 2, 3, 4, 5, 8, 9, 12, 127, 128, 129, 131, 257):
        rows = np.arange(1000, 1000 + count)
        want = []
        for beg in range(0, count, dg.CHUNK):
            end, alone = min(beg + dg.CHUNK, count), []
            for wave in range(4):
                j = beg + wave
                while j < end:
                    if not j + 4 < end:
                        alone.append(int(rows[j]))
                    j += 8
            want.append(alone)
        assert dg.lone_rows(rows) == want, count
    assert dg.lone_rows(np.arange(5)) == [[1, 2, 3]] and dg.lone_rows(np.arange(8)) == [[]]


def _relation_rows_batch(c):
    """what rgcn_negative_sample_relation_device writes for a RELATION_ROW_CASES case, by its byte-exact mirror"""
    import relation_negatives_reference as rnr
    batch, _ = dg.case_batch(c)
    s = rnr.sample(np.zeros(0, dtype=np.uint64), batch, dg.RELATION_ROW_RATE, dg.RELATION_ROW_M, c["V"], c["R"], c["seed"],
                   False)
    return s["X"].astype(np.int32)


def _check_case_weights(c, N, X):
    name, n = c["name"], c["n"]
    w = dg.case_weights(c, N, X)
    assert w.shape == (N,) and w.dtype == np.float32 and np.isfinite(w).all() and w.min() == 0 and 2.9 < w.max() < 3
    assert np.array_equal(w, dg.case_weights(c, N, X))                       # a function of the case
    for value in (0.0, 1.0):
        assert 0.10 <= (w == value).mean() <= 0.19, (name, value, (w == value).mean())
    assert (w > dg.HIGH).mean() >= 0.10 and ((w > 0) & (w < 1)).mean() >= 0.2
    batch, _ = dg.case_batch(c)
    if X is None:
        rel, ents = np.tile(batch[:, 1], N // n), batch
        order = dg.relation_order(rel, n if dg.is_tiled(c) else None)
    else:
        rel, ents = X[:, 1], X
        order = dg.relation_order(rel)
    assert sorted(order) == list(range(N)) and (np.diff(rel[order]) >= 0).all()
    small = 0
    for r, rows in dg.relation_segments(rel, order):
        assert (rel[rows] == r).all()
        if len(rows) % 2 == 1:
            assert w[rows[-1]] > dg.HIGH, (name, r)
        if r < 7 and len(rows) >= 2:
            small += 1
            assert (w[rows] == 0).any() and (w[rows] > dg.HIGH).any(), (name, r)
            for alone in dg.lone_rows(rows):
                assert not alone or (w[alone] > dg.HIGH).any(), (name, r)
    assert small >= 5, name
    hubs = 0
    for e in range(7):
        rows = dg.entity_rows(ents, e)
        if len(rows) >= 2:
            hubs += 1
            assert (w[rows] == 0).any() and (w[rows] > dg.HIGH).any(), (name, e)
    assert hubs >= 5, name                      # entities 2 .. 6 (and, among corrupted rows, whichever of 0 and 1 was drawn)
    # the copies of a triple (rows g, g + n, ...) never share a weight: pairwise up to 7 copies; past that a triple's
    # zeros (and ones) are 7 copies apart and the rest is pairwise different
    k = N // n
    if k > 1:
        groups = w.reshape(k, n)
        for a in range(k):
            for b in range(a + 1, k):
                same = groups[a] == groups[b]
                if k <= 7:
                    assert not same.any(), (name, a, b)
                else:
                    assert not (same & ~np.isin(groups[a], (0.0, 1.0))).any() and (b - a == 7 or not same.any()), (name, a, b)


@pytest.mark.parametrize("name", sorted(n for n, c in dg.DECODER_CASES.items() if c["n"] > 1))
def test_case_weights_hold_their_constructed_properties(name):
    c = dg.DECODER_CASES[name]
    _check_case_weights(c, c["n"] * dg.copies(c), None)


@pytest.mark.parametrize("name", dg.RELATION_ROW_CASES)
def test_case_weights_on_relation_rows(name):
    """the batch of test_relation_rows_on_grid_batches: the copies of a triple no longer share a relation, the order is
    the general one, and the weights are built on the rows themselves"""
    c = dg.DECODER_CASES[name]
    X = _relation_rows_batch(c)
    N = c["n"] * (dg.RELATION_ROW_RATE + 1 + dg.RELATION_ROW_M)
    assert X.shape == (N, 3) and N == 6000
    first = c["n"] * (dg.RELATION_ROW_RATE + 1)
    assert (X[first:, 1] != np.tile(X[:c["n"], 1], dg.RELATION_ROW_M)).all()
    _check_case_weights(c, N, X)
    rc = np.bincount(X[:, 1], minlength=c["R"])
    assert max(dg.chunks(m) for m in rc) > 1 and (rc % 2 == 1).any() and dg.incidences(X, c["V"])[6] > dg.LONG_ROW


def test_float32_restatement_of_the_weighted_decoder():
    """adversarial_reference.weighted_decoder(dtype = float32), the yardstick of the weighted grid test's l2 bar: with unit
    weights it is oracle.distmult_loss_and_grads byte for byte, with
    the case's weights it is the float64 mirror to float32 rounding, and far from the unit-weight answer."""
    import adversarial_reference as adv
    import helpers
    import oracle
    c = dg.DECODER_CASES["dec_d66_rate1"]
    rng = np.random.RandomState(3)
    codes = (rng.randn(c["V"], c["d"]) * 0.5).astype(np.float32)
    w_rel = (rng.randn(c["V"], c["d"]) * 0.5).astype(np.float32)
    batch, _ = dg.case_batch(c)
    X, Y = dg.host_tiled(batch, c["rate"], c["V"], c["seed"])
    ones = np.ones(len(X), np.float32)
    f = adv.weighted_decoder(codes, w_rel, X, Y, ones, 0.01, dtype=np.float32)
    oloss, odcodes, odw = oracle.distmult_loss_and_grads(codes, w_rel, X, Y, 0.01)
    assert f["dcodes"].dtype == np.float32 and f["dW"].dtype == np.float32 and f["dx"].dtype == np.float32
    assert f["loss"] == oloss and np.array_equal(f["dcodes"], odcodes) and np.array_equal(f["dW"], odw)
    w = dg.case_weights(c, len(X))
    f = adv.weighted_decoder(codes, w_rel, X, Y, w, 0.01, dtype=np.float32)
    g = adv.weighted_decoder(codes, w_rel, X, Y, w, 0.01)
    assert abs(f["loss"] - g["loss"]) <= 1e-6 * abs(g["loss"])
    assert abs(g["loss"] - (g["loss"] - (w * g["per"]).mean() + g["per"].mean())) > 1e-2 * abs(g["loss"])
    for name in ("dcodes", "dW"):
        worst, l2 = helpers.error_against(g[name], f[name])
        # sequential float32 sums of up to 1,025 terms (the hub) and 640 (relation 6): some sqrt(m) u = 2e-6 of scale
        assert 0 < worst <= 1e-5 and l2 <= 5e-6, (name, worst, l2)
        assert helpers.error_against(g[name], {"dcodes": odcodes, "dW": odw}[name])[1] > 0.1     # the weights matter
    assert not g["dx"][w == 0].any() and not f["dx"][w == 0].any()


def test_uniform_draws_alone_would_not_hold_them():
    """why the weights are built: uniform draws with a seventh of zeros scattered leave a small relation without one"""
    missed = 0
    for c in dg.DECODER_GRID:
        if c["n"] == 1:
            continue
        N = c["n"] * dg.copies(c)
        rng = np.random.RandomState(c["seed"] + 100003)
        w = rng.rand(N) * 3.0
        w[rng.rand(N) < 1.0 / 7] = 0.0
        batch, _ = dg.case_batch(c)
        rel = np.tile(batch[:, 1], N // c["n"])
        missed += any(r < 7 and len(rows) >= 2 and not (w[rows] == 0).any()
                      for r, rows in dg.relation_segments(rel, dg.relation_order(rel)))
    assert missed > 0


@pytest.mark.parametrize("source,text", [
    ("decoder.hip", "if (row_weights == nullptr) {"),
    ("decoder.hip", "if (vec4) RGCN_LAUNCH_ER_T(4, true); else RGCN_LAUNCH_ER_T(1, true);"),
    ("decoder.hip", "if (vec4) RGCN_LAUNCH_E(4, true); else RGCN_LAUNCH_E(1, true);"),
    ("decoder.hip", "if (T == 1) RGCN_LAUNCH_ER(VEC, 1, WT); else if (T == 2) RGCN_LAUNCH_ER(VEC, 2, WT); else RGCN_LAUNCH_ER(VEC, 4, WT); \\"),
    ("decoder.hip", "hipLaunchKernelGGL((k_dec_energy_rel<VEC, TT, WT>), dim3(q.max_chunks), dim3(256), lds, c->stream, codes, Wr, q.X, Y, \\"),
    ("decoder.hip", "hipLaunchKernelGGL((k_dec_energy<VEC, WT>), dim3(q.energy_blocks), dim3(256), 0, c->stream, codes, Wr, q.X, Y, \\"),
    ("decoder.hip", "if constexpr (WEIGHTED) { w0 = Wt[m0]; w1 = two ? Wt[m1] : 0.f; }"),
    ("decoder.hip", "int j = beg + wave;"),
    ("decoder.hip", "int n0 = j < end ? permr[j] : -1, n1 = j + 4 < end ? permr[j + 4] : -1;"),
    ("decoder.hip", "j += 8;"),
    ("decoder.hip", "if (X == q.tiled_X && N64 == q.tiled_N && (N_total <= 0 || N_total == N64) && q.tiled_period > 1 &&"),
    ("decoder.hip", "int t = p + j * period;"),
    ("decoder.hip", "c->dec.tiled_X = nullptr;"),
    ("decoder.hip", "const bool fused = nvec_e <= 256;"),
    ("decoder.hip", "const int T = nvec_e <= 64 ? 1 : (nvec_e <= 128 ? 2 : 4);"),
    ("row_walk.h", "inline int row_lanes(int nvec) { return nvec <= 64 ? 64 : (nvec <= 128 ? 128 : 256); }"),
    ("decoder.hip", "const int tpr = row_lanes(nvec);"),
    ("decoder.hip", "const bool rlds = lds <= 64 * 1024;"),
    ("decoder.hip", "const size_t lds = (size_t)R * kLine * sizeof(float);"),
    ("decoder.hip", "const bool vec4 = (d % 4 == 0) && aligned16(codes)"),
    ("decoder.hip", "const bool lines = vec4 && knob(\"RGCN_DEC_LINES\", 1) != 0"),
    ("decoder.hip", "for (int band = x, pass = 0; band < b.nbands; band += 8, ++pass) {"),
    ("decoder.hip", "q.nbands = (int32_t)((d + kLine - 1) / kLine);"),
    ("decoder.hip", "const int np = (end - beg + kDecPiece - 1) / kDecPiece;"),
    ("decoder.hip", "for (int c0 = 0; c0 < nvec; c0 += 128) {"),
    ("decoder.hip", "q.tiled_period > 1 &&"),
    ("decoder.hip", "constexpr int kDecLongRow = 256;"),
    ("decoder.hip", "constexpr int kDecPiece = 512;"),
    ("decoder.hip", "constexpr int kDecChunk = 128;"),
    ("decoder.hip", "constexpr int kLine = 32;"),
    ("../../include/rgcn.h", "#define RGCN_MAX_DECODER_TRIPLES ((int64_t)1 << 29)"),
    ("rgcn_api.hip", "if (max_triples <= 0 || max_triples > RGCN_MAX_DECODER_TRIPLES)"),
    ("rgcn_api.hip", "if (n * (int64_t)(rate + 1) > RGCN_MAX_DECODER_TRIPLES)"),
])
def test_host_mirrors_follow_the_kernel_sources(source, text):
    """The mirrors in decoder_grid.py are copies of these dispatch lines: when one changes, the table has to be
    re-derived."""
    with open(os.path.join(CSRC, source)) as f:
        assert text in f.read(), "%s no longer holds `%s`: update tests/decoder_grid.py's mirror" % (source, text)


def test_batch_bound_keeps_the_decoder_indices_in_int32():
    """The largest int expressions of the decoder path at N = the bound: 3 N + 2 (X[3 * n + 2]) and the launch size
    2 N + 255 (k_dec_keys, k_dec_slots; lower_bound_u32 over 2 N keys)."""
    N = dg.MAX_DECODER_TRIPLES
    assert 3 * (N - 1) + 2 < 2 ** 31 and 2 * N + 255 < 2 ** 31
    assert 3 * (2 ** 30 - 1) + 2 >= 2 ** 31                  # the old bound did overflow


def test_mirrors_on_known_configurations():
    assert [dg.energy_cell(d) for d in (20, 256, 260, 512, 516, 1024, 1028)] == \
        [("energy_rel", 4, 1)] * 2 + [("energy_rel", 4, 2)] * 2 + [("energy_rel", 4, 4)] * 2 + [("energy", 4, None)]
    assert [dg.energy_cell(d) for d in (9, 63, 66, 126, 130, 255, 258)] == \
        [("energy_rel", 1, 1)] * 2 + [("energy_rel", 1, 2)] * 2 + [("energy_rel", 1, 4)] * 2 + [("energy", 1, None)]
    assert [dg.entity_tpr(d) for d in (9, 63, 66, 126, 130, 255, 258)] == [64, 64, 128, 128, 256, 256, 256]
    assert [dg.bands(d) for d in (20, 256, 260, 516, 1028)] == [1, 8, 9, 17, 33]
    assert [dg.band_passes(d) for d in (20, 256, 260, 516, 1028)] == [1, 1, 2, 3, 5]
    assert dg.rel_partial_passes(1028) == 3 and dg.rel_partial_passes(1030) == 9
    assert dg.entity_cell(500, 237) == ("lines", True) and dg.entity_cell(20, 513) == ("lines", False)
