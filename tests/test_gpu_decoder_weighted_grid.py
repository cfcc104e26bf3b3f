"""Row weights, the tiled order and relation rows at every compiled variant of decoder_compute (tests/decoder_grid.py:
WEIGHTED_CASES, WEIGHTED_ENERGY_CELLS, RELATION_ROW_CASES, case_weights) against the float64 mirror of
tests/adversarial_reference.py at the engine's own codes.

The bars are test_decoder_grid_matches_float64's, unchanged: the loss within 2e-6 relative, every entry of dL/dcodes and
dL/dW_relation within 5e-6 of the tensor's scale (helpers.error_against, no excused fraction), the l2 error at most 4x plus
1e-7 that of the fp32 restatement of the same weighted formula (adversarial_reference.weighted_decoder, dtype = float32).

dx has no read-back in the ABI.  That a zero-weight row's dx is exactly 0 is asserted through what it would move: the run is
repeated with the label of every zero-weight row replaced by 1 - y, which moves such a row's sigmoid(x) - y by one whole
unit, and loss, dL/dcodes and dL/dW_relation have to come back equal entry for entry."""
import numpy as np
import pytest

import adversarial_reference as adv
import decoder_grid as dg
import helpers
import oracle
from helpers import make_case
from test_gpu_train_step import _decoder_grads, _grid_decoder, _grid_energies

pytestmark = pytest.mark.gpu

# The regulariser is not weighted.  At the 0.01 of the unweighted grid test it is 99.6 % of the saturated case's loss (its
# W_relation is scaled up until an energy reaches 150), so that no weights in [0, 3) could move that loss by the 1000 loss
# tolerances demanded below; at 0.001 every case can be asked for them, and the loss bar weighs the cross-entropy sum ten
# times as heavily.  The regulariser's own gradient terms are the unweighted kernels' lines, held at 0.01 there.
REG = 0.001
LOSS_TOL, MAX_TOL = 2e-6, 5e-6
TILED_NAMES = tuple(n for n in dg.WEIGHTED_CASES if dg.is_tiled(dg.DECODER_CASES[n]))
FLOAT4_NAMES = tuple(n for n in dg.WEIGHTED_CASES if dg.vec_width(dg.DECODER_CASES[n]["d"]) == 4)
STEP_NAMES = ("dec_d66_rate1", "dec_d260_rate1", "dec_d1028_rate1")


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def _weights(c, N, X):
    """case_weights: built on the relations the samplers keep (and on the first copies' entities); on the rows themselves
    when relation rows follow"""
    return dg.case_weights(c, N, X if N != c["n"] * dg.copies(c) else None)


_RUNS = {}


def _runs(native, name):
    """the device's answers for a case, computed once and shared by the tests below (left unchanged by them)"""
    if name not in _RUNS:
        _RUNS[name] = _grid_decoder(native, dg.DECODER_CASES[name], runs=("plain", "null", "ones", "weighted", "flipped"),
                                    weights=_weights, reg=REG)
    return _RUNS[name]


def _against_float64(tag, c, codes, w_rel, X, Y, w, got, weighted=True):
    """the three bars; returns the float64 mirror.  Prints the measured errors next to the fp32 restatement's."""
    loss, dcodes, dwrel = got
    ref = adv.weighted_decoder(codes, w_rel, X, Y, w, REG)
    f32 = adv.weighted_decoder(codes, w_rel, X, Y, w, REG, dtype=np.float32)
    report = ["loss %.1e (fp32 %.1e)" % (abs(loss - ref["loss"]) / abs(ref["loss"]),
                                         abs(f32["loss"] - ref["loss"]) / abs(ref["loss"]))]
    bad = []
    if not abs(loss - ref["loss"]) <= LOSS_TOL * abs(ref["loss"]):
        bad.append("loss %.9g, float64 %.9g" % (loss, ref["loss"]))
    for g, key, what in ((dcodes, "dcodes", "dcodes"), (dwrel, "dW", "dW_relation")):
        worst, l2 = helpers.error_against(ref[key], g)
        oworst, ol2 = helpers.error_against(ref[key], f32[key])
        report.append("%s %.1e/%.1e (fp32 %.1e/%.1e)" % (what, worst, l2, oworst, ol2))
        if not worst <= MAX_TOL:
            bad.append("%s against float64: max %.2e of scale" % (what, worst))
        if not l2 <= 4 * ol2 + 1e-7:
            bad.append("%s: l2 %.2e, the fp32 restatement's %.2e" % (what, l2, ol2))
    print(tag, dg.weighted_cell_of(c, weighted), dg.weighted_energy_cell(c)[1], "; ".join(report))
    assert not bad, (tag, bad)
    return ref


def _exact_zero_structure(c, X, dcodes, dwrel):
    """test_decoder_grid_matches_float64's: entities without an incidence, relations without a triple, rows >= R"""
    R, V = c["R"], c["V"]
    inc = dg.incidences(X, V)
    assert (inc == 0).any() or c["rate"] is not None
    assert not dcodes[inc == 0].any() and dcodes[inc > 0].any(axis=1).all()
    rc = np.bincount(X[:, 1], minlength=R)
    assert (rc == 0).any()
    assert not dwrel[:R][rc == 0].any() and dwrel[:R][rc > 0].any(axis=1).all()
    assert not dwrel[R:].any()


def _same_bytes(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1], err_msg="%s: dcodes" % what)
    np.testing.assert_array_equal(a[2], b[2], err_msg="%s: dW_relation" % what)


@pytest.mark.parametrize("name", dg.WEIGHTED_CASES)
def test_weighted_decoder_grid_matches_float64(native, name):
    """All 16 WEIGHTED energy instantiations (eight cells, each under the plain and the tiled order), the saturated
    energies and the global relation band with dg.case_weights: exact zeros, exact ones, a large weight on the row a wave
    takes alone, zeros and large weights in every small relation and on every hub row, different weights on the copies of
    a triple."""
    c = dg.DECODER_CASES[name]
    codes, w_rel, X, Y, w, got = _runs(native, name)
    assert np.array_equal(w, dg.case_weights(c, len(X)))
    if c["saturate"]:
        assert np.abs(_grid_energies(codes, w_rel, X)).max() > 90
    if dg.is_tiled(c):                     # what case_weights assumed of the sampler's rows
        assert np.array_equal(X[:, 1], np.tile(X[:c["n"], 1], len(X) // c["n"]))
    ref = _against_float64(name, c, codes, w_rel, X, Y, w, got["weighted"])
    # the comparison is not one of unit weights: the weights move the loss by over 1000 x its tolerance
    unit = ref["loss"] - float((w.astype(np.float64) * ref["per"]).mean()) + float(ref["per"].mean())
    assert abs(ref["loss"] - unit) >= 1000 * LOSS_TOL * abs(ref["loss"]), (ref["loss"], unit)
    _exact_zero_structure(c, X, got["weighted"][1], got["weighted"][2])
    # dx of a zero-weight row is exactly 0 (the module's docstring)
    assert (w == 0).sum() >= len(w) // 10 and not ref["dx"][w == 0].any()
    _same_bytes(got["flipped"], got["weighted"], "labels of the zero-weight rows flipped")


@pytest.mark.parametrize("name", dg.WEIGHTED_CASES)
def test_unit_and_null_weights_reproduce_the_unweighted_bytes_on_the_grid(native, name):
    """WEIGHTED with all ones (wt * t is t) and the NULL pointer against rgcn_decoder_loss_backward_device on the same
    context and batch: the same bytes, at every cell and order"""
    codes, w_rel, X, Y, w, got = _runs(native, name)
    assert np.abs(got["plain"][1]).max() > 0 and np.abs(got["plain"][2]).max() > 0
    _same_bytes(got["null"], got["plain"], "NULL weights")
    _same_bytes(got["ones"], got["plain"], "unit weights")
    assert got["weighted"][0] != got["plain"][0]


@pytest.mark.parametrize("name", FLOAT4_NAMES)
def test_entity_gradient_forms_are_bitwise_equal_under_weights(native, name):
    """test_entity_gradient_forms_are_bitwise_equal_on_the_grid with dx = w (sigmoid(x) - y) / N: k_dec_entity_lines against
    k_dec_entity_grad (RGCN_DEC_LINES = 0, the devtools build).  A tiled case's rows are laid out on the host as the
    sampler lays them out."""
    c = dg.DECODER_CASES[name]
    X, Y = dg.case_batch(c)
    if c["rate"] is not None:
        X, Y = dg.host_tiled(X, c["rate"], c["V"], c["seed"])
    w = dg.case_weights(c, len(X))
    a = _decoder_grads(native, c["V"], c["R"], c["d"], c["nb"], X, Y, lines=False, seed=c["seed"], weights=w)
    b = _decoder_grads(native, c["V"], c["R"], c["d"], c["nb"], X, Y, lines=True, seed=c["seed"], weights=w)
    _same_bytes(a, b, "line form against row form")
    assert np.abs(a[1]).max() > 0 and np.abs(a[2]).max() > 0 and a[0] != 0


@pytest.mark.parametrize("name", TILED_NAMES)
def test_adversarial_weights_then_decoder_on_tiled_grid_batches(native, name):
    """The device sampler, rgcn_adversarial_weights_device(P = n: 375 workgroups at n = 1500) and the weighted decoder in
    the tiled order.  The weights within the mirror's derived tolerance, every group's sum K within K x the group's
    largest tolerance; the decoder at the bars above, fed the device's own weights.  (K = rate: the rate 10 case spreads
    its weights, 0.67 .. 1.31; a group of one negative or none weighs 1, which the mirror's tolerance then demands of the device.)"""
    c = dg.DECODER_CASES[name]
    codes, w_rel, X, Y, w, got = _grid_decoder(native, c, runs=("weighted",), temperature=adv.ALPHA, reg=REG)
    P, K = c["n"], c["rate"]
    ref = adv.weights(codes, w_rel, X, P, adv.ALPHA)
    err = np.abs(w.astype(np.float64) - ref["w"])
    print("%s: weights %.4g .. %.4g, worst error %.3g at a tolerance of %.3g"
          % (name, w.min(), w.max(), err.max(), ref["tol"][int(np.argmax(err))]))
    assert ref["K"] == K and np.isfinite(w).all() and (w >= 0).all() and (w[:P] == 1.0).all()
    assert (err <= ref["tol"]).all(), float((err - ref["tol"]).max())
    if K > 0:
        sums = w[P:].astype(np.float64).reshape(K, P).sum(axis=0)
        assert (np.abs(sums - K) <= K * ref["tol"][P:].reshape(K, P).max(axis=0)).all()
    if K > 1:
        assert w[P:].max() > 1.25 and w[P:].min() < 0.75            # (these codes' energies are small: a modest spread)
    else:
        assert (w == 1.0).all()
    _against_float64(name + " adversarial", c, codes, w_rel, X, Y, w, got["weighted"])
    _exact_zero_structure(c, X, got["weighted"][1], got["weighted"][2])


@pytest.mark.parametrize("name", dg.RELATION_ROW_CASES)
def test_relation_rows_on_grid_batches(native, name):
    """rgcn_negative_sample_relation_device (rate 1, m = 2: N = 6000) on the case's 1500-row batch: the copies of a triple
    no longer share a relation, decoder_prepare takes its general path.  Unweighted and with case_weights built on the rows
    the sampler wrote."""
    c = dg.DECODER_CASES[name]
    assert c["rate"] == dg.RELATION_ROW_RATE
    codes, w_rel, X, Y, w, got = _grid_decoder(native, c, runs=("plain", "weighted", "flipped"), weights=_weights,
                                               relation_rate=dg.RELATION_ROW_M, reg=REG)
    n, N = c["n"], len(X)
    assert N == 6000 and np.array_equal(w, dg.case_weights(c, N, X))
    first = n * (c["rate"] + 1)
    assert (X[first:, 1] != np.tile(X[:n, 1], dg.RELATION_ROW_M)).all() and not Y[n:].any() and Y[:n].all()
    # what the batch still exercises: a relation of several chunks, an odd count, the hub above kDecLongRow
    rc = np.bincount(X[:, 1], minlength=c["R"])
    assert max(dg.chunks(m) for m in rc) > 1 and (rc % 2 == 1).any()
    assert dg.incidences(X, c["V"])[len(dg.ENTITY_COUNTS) - 1] > dg.LONG_ROW
    ones = np.ones(N, np.float32)
    _against_float64(name + " relation rows", c, codes, w_rel, X, Y, ones, got["plain"], weighted=False)
    ref = _against_float64(name + " relation rows, weighted", c, codes, w_rel, X, Y, w, got["weighted"])
    unit = ref["loss"] - float((w.astype(np.float64) * ref["per"]).mean()) + float(ref["per"].mean())
    assert abs(ref["loss"] - unit) >= 1000 * LOSS_TOL * abs(ref["loss"])
    for run in ("plain", "weighted"):
        inc = dg.incidences(X, c["V"])
        assert not got[run][1][inc == 0].any() and not got[run][2][:c["R"]][rc == 0].any() and not got[run][2][c["R"]:].any()
    _same_bytes(got["flipped"], got["weighted"], "labels of the zero-weight rows flipped")


@pytest.mark.parametrize("name", STEP_NAMES)
def test_train_step_under_the_mode_on_the_grid(native, name):
    """One rgcn_train_step_device (L = 2, keep_prob 0.8) under rgcn_set_adversarial_negatives(ALPHA, n) on the host-tiled
    batch of a grid case: the entity-gradient kernel writes the weighted dL/dcodes x dropout for the top layer's self-loop
    GEMMs (ds_ready, store_dcodes).  Every encoder gradient and dW_relation against the float64 reverse mode at the
    engine's own activations, fed the float64 weighted decoder with the device's weights
    (RGCN_BUF_ADVERSARIAL_WEIGHTS): test_train_step_grid_matches_float64's bars, max 5e-6 of scale, l2 2e-6."""
    c = dg.DECODER_CASES[name]
    V, R, d, nb, L, n = c["V"], c["R"], c["d"], c["nb"], 2, c["n"]
    params, triples, _, _ = make_case(V, R, d, L, "block", nb, 4 * V, seed=c["seed"])
    batch, _ = dg.case_batch(c)
    X, Y = dg.host_tiled(batch, c["rate"], V, c["seed"])
    N = len(X)
    names = [k for k in oracle.weight_names("block", L) if not (k.startswith("b") and k != "b_emb")]
    with native.Engine(V, R, d, L, "block", nb, keep_prob=0.8, max_edges=len(triples)) as eng:
        eng.set_params(params)
        eng.decoder_reserve(N)
        eng.set_adversarial_negatives(adv.ALPHA, n)
        td, xd, yd = eng.to_device(triples), eng.to_device(X), eng.to_device(Y)
        eng.train_step_device(td, len(triples), xd, yd, N, seed=60, reg_param=REG)
        loss, grads, w = eng.loss(), eng.get_grads(), eng.read_buffer(native.BUF_ADVERSARIAL_WEIGHTS)
        acts = [eng.activation(l) for l in range(L + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, L + 1)]
        for b in (td, xd, yd):
            b.free()
    assert w.shape == (N,)
    wref = adv.weights(acts[-1], params["W_relation"], X, n, adv.ALPHA)
    assert (np.abs(w.astype(np.float64) - wref["w"]) <= wref["tol"]).all() and (w[:n] == 1.0).all()
    ref = adv.weighted_decoder(acts[-1], params["W_relation"], X, Y, w, REG)
    assert abs(loss - ref["loss"]) <= LOSS_TOL * abs(ref["loss"]), (loss, ref["loss"])
    g64 = helpers.float64_grads_at(dict(V=V, R=R, d=d, L=L, kind="block", nb=nb, params=params, triples=triples,
                                        masks=masks, dcodes=ref["dcodes"]), acts)
    g64["W_relation"] = ref["dW"]
    report, bad = [], []
    for k in names:
        assert np.abs(g64[k]).max() > 0, k
        worst, l2 = helpers.error_against(g64[k], grads[k])
        report.append("%s %.1e/%.1e" % (k, worst, l2))
        if not (worst <= 5e-6 and l2 <= 2e-6):
            bad.append("%s grad %s against float64: max %.2e l2 %.2e" % (name, k, worst, l2))
    print(name, "under the mode;", "; ".join(report))
    assert not bad, bad
