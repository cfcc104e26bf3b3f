"""tests/step_matrix.py's table and composed mirror, held to their own claims on the CPU: the coverage the table promises,
that every enabled option matters on every row's own batch (so that tests/test_gpu_step_matrix.py cannot pass by comparing
zeros), and that compose() is the gradient of the loss it returns.

The gradient check: central differences with step FD_STEP = 1e-4 of the float64 loss (query rows exact, the adversarial
weights held constant, as the step treats them) at ten entries of the codes and of W_relation, an entry of a row R + r
among them where the batch has inverse positives.  At that step the error is the difference's own truncation: the plain
decoder mirror (relation_softmax_reference.decoder) disagrees with its own central difference by 3.15e-07 of the gradient's
largest entry at worst over the three cases (1.1e-07, 2.4e-07, 3.15e-07; at 1e-5 it is 4e-09, at 1e-6 round-off takes over
at 2e-08).  PLAIN_FD = 3.2e-07 is asserted for the plain mirror and ten times that, 3.2e-06, for the composed one, whose
measured figures are 1.4e-07 (block-all-terms), 1.5e-07 (out6-masked) and 2.4e-07 (block-typed+reciprocal)."""
import functools

import numpy as np
import pytest

import relation_softmax_reference as rsr
import step_matrix as sm

FD_STEP, PLAIN_FD = 1e-4, 3.2e-7
SEED = 91           # the negative seed of the minibatch rows


@functools.lru_cache(maxsize=None)
def mirror(name):
    """the case, its batch and the whole float64 step at the seeded masks: computed once, left unchanged"""
    c = sm.case_inputs(name)
    X, Y, n_pos = sm.mirror_batch(c, SEED)
    graph = c["batch"] if c["step"] == "minibatch" else c["triples"]
    out, g64 = sm.mirror_step(c, X, Y, n_pos, c["masks"], graph)
    return c, X, Y, n_pos, graph, out, g64


RUN = [c["name"] for c in sm.STEP_MATRIX if not c["off"]]


# ------------------------------------------------------------------ coverage
def test_every_form_has_all_three_terms_together():
    rows = [c for c in sm.STEP_MATRIX if c["step"] == "xy" and c["adv"] and c["relsm"] and c["entsm"] and not c["relsm_exclusive"]]
    assert [c["form"] for c in rows] == [f["name"] for f in sm.FORM_LIST] and len(sm.FORM_LIST) == 10
    assert sm.ALL_TERMS == [c["name"] for c in rows]
    assert {(f["kind"], f["input_mode"], f["skip"], f["norm"], bool(f["code_dim"])) for f in sm.FORM_LIST} >= {
        ("block", "embedding", "none", "intended", False), ("basis", "embedding", "none", "intended", False),
        ("basis_tdiag", "embedding", "none", "intended", False), ("basis_pdiag", "embedding", "none", "intended", False),
        ("basis", "onehot", "none", "intended", False), ("block", "embedding", "highway", "intended", False),
        ("block", "embedding", "none", "intended", True), ("basis", "embedding", "none", "intended", True),
        ("block", "embedding", "none", "local", False), ("block", "embedding", "highway", "local", True)}
    for f in sm.FORM_LIST:
        assert 2 * f["R"] <= f["V"] and f["L"] == 2


def test_every_sampling_mode_meets_every_term_it_is_legal_with():
    for form in sm.MINIBATCH_FORMS:
        rows = {c["mode"]: c for c in sm.STEP_MATRIX if c["form"] == form and c["step"] == "minibatch"}
        assert set(rows) == set(sm.MODES) == {"plain", "exclusive", "relation", "typed", "typed+relation", "reciprocal",
                                               "typed+reciprocal"}
        for mode, c in rows.items():
            assert c["adv"] and c["relsm"]
            assert bool(c["entsm"]) == (not sm.MODES[mode][2])        # reciprocal never appears with the entity term
        assert rows["plain"]["entsm_count"] == sm.LEADING < sm.N_BATCH
        assert rows["exclusive"]["relsm_exclusive"] and rows["exclusive"]["entsm_exclusive"]
    assert not any(c["entsm"] for c in sm.STEP_MATRIX if c["mode"] and "reciprocal" in c["mode"])
    assert set(sm.MINIBATCH_FORMS) == {"block", "out8", "highway"} and sm.M_REL == 2


def test_masks_and_odd_shapes_are_in_the_table():
    masked = {c["form"] for c in sm.STEP_MATRIX if c["relsm_exclusive"] and c["entsm_exclusive"] and c["step"] == "xy"}
    assert masked >= {"block", "out8", "out6"}
    assert sum(f["V"] % 4 != 0 for f in sm.FORM_LIST) >= 3 and any(f["dc"] % 4 != 0 for f in sm.FORM_LIST)
    assert sm.FORMS["out8"]["V"] % 4 == 3 and sm.FORMS["out6"]["dc"] == 6
    assert {c["form"] for c in sm.STEP_MATRIX if c["off"]} == {"out8", "highway"}
    import pdiag_grid
    import tdiag_grid
    assert sm.FORMS["tdiag"]["d"] == min(c["d"] for c in tdiag_grid.TDIAG_GRID_LIST)
    assert "tdiag_d%d_B%d" % (sm.FORMS["tdiag"]["d"], sm.FORMS["tdiag"]["nb"]) in tdiag_grid.TDIAG_GRID
    assert "pdiag_d%d_B%d" % (sm.FORMS["pdiag"]["d"], sm.FORMS["pdiag"]["nb"]) in pdiag_grid.PDIAG_GRID


def test_the_graph_has_a_hub_past_the_long_row_cut():
    for f in sm.FORM_LIST:
        c = sm.form_inputs(f)
        t, V = c["triples"], c["V"]
        slots = np.bincount(np.concatenate([t[:, 0], t[:, 2]]), minlength=V)
        assert len(t) == sm.E and slots[V - 1] > 32 and np.sort(slots)[-2] <= 32
        assert len(np.unique(t, axis=0)) < len(t)                         # a duplicated edge
        assert t[:, 1].max() == sm.R - 2                                  # relation R - 1 sends no message
        assert set(map(tuple, c["X"][:sm.P_STEP].tolist())) <= set(map(tuple, t.tolist()))


# ------------------------------------------------------------------ each option counts, per case
@pytest.mark.parametrize("name", RUN)
def test_each_option_counts(name):
    c, X, Y, n_pos, graph, out, g64 = mirror(name)
    sm.check_options_count(c, out, n_pos)
    if c["relsm_exclusive"] or c["entsm_exclusive"]:
        plain = sm.compose(dict(c, relsm_exclusive=False, entsm_exclusive=False), sm.forward64(c, c["masks"], graph)["codes"],
                           X, Y, n_pos)
        assert abs(plain["rel"]["loss"] - out["rel"]["loss"]) > 1e-3 and abs(plain["ent"]["loss"] - out["ent"]["loss"]) > 1e-3
        for key in ("rel", "ent"):           # the gold stays a candidate
            assert out[key]["mask"].shape == plain[key]["mask"].shape and plain[key]["mask"].all()
    if c["entsm_count"]:
        assert len(out["ent"]["mask"]) == 2 * sm.LEADING
    elif c["entsm"]:
        assert len(out["ent"]["mask"]) == 2 * n_pos
    assert out["rel"]["G"].shape == (n_pos, sm.R)
    # no compared gradient is all zeros but the layers' unused biases
    for n in sm.weight_names(c):
        assert (not np.abs(g64[n]).max() > 0) == sm.unused_bias(c, n), (name, n)
    if c["mode"] and sm.MODES[c["mode"]][2]:
        assert np.abs(g64["W_relation"][sm.R:2 * sm.R]).max() > 0         # the inverse relations' rows
        assert len(X) == n_pos * (sm.RATE + 2 + sm.MODES[c["mode"]][1])
    print("%s: loss %.6f = decoder %.6f (unit weights %.6f) + relation term %.6f + entity term %.6f" % (
        name, out["loss"], out["decoder"], out["plain"], out["rel"]["loss"], out["ent"]["loss"] if out["ent"] else 0.0))


# ------------------------------------------------------------------ compose is a gradient
def _entries(c, X, n_pos):
    rng = np.random.RandomState(3)
    dc = c["dc"]
    codes = [(int(X[i, 0]), int(rng.randint(dc))) for i in (0, 1, 2)] + [(int(X[i, 2]), int(rng.randint(dc))) for i in (3, 4, n_pos + 1)]
    rel = [(int(X[i, 1]), int(rng.randint(dc))) for i in (0, 5)] + [(int(X[-1, 1]), 1), (int(X[-2, 1]), 0)]
    return codes, rel


def _disagreement(f, codes, W, g_codes, g_W, entries):
    """max over the entries of |central difference - gradient| / max |gradient|"""
    worst = 0.0
    for which, ents, g in (("codes", entries[0], g_codes), ("W", entries[1], g_W)):
        for i, j in ents:
            a, b = codes.copy(), W.copy()
            t = a if which == "codes" else b
            t[i, j] += FD_STEP
            up = f(a, b)
            t[i, j] -= 2 * FD_STEP
            fd = (up - f(a, b)) / (2 * FD_STEP)
            assert g[i, j] != 0, (which, i, j)
            worst = max(worst, abs(fd - g[i, j]) / np.abs(g).max())
    return worst


@pytest.mark.parametrize("name", sm.GRADIENT_CASES)
def test_compose_is_the_gradient_of_its_loss(name):
    c, X, Y, n_pos, graph, _, _ = mirror(name)
    assert c["adv"] and c["relsm"]
    codes = np.array(sm.forward64(c, c["masks"], graph)["codes"], dtype=np.float64)
    W = c["params"]["W_relation"].astype(np.float64)
    w = sm.compose(c, codes, X, Y, n_pos, w_relation=W, exact_query=True)["w"]
    ana = sm.compose(c, codes, X, Y, n_pos, w_relation=W, exact_query=True, row_weights=w)
    entries = _entries(c, X, n_pos)
    if name == "block-typed+reciprocal":
        assert sm.R <= entries[1][2][0] < 2 * sm.R                         # an entry of a row R + r
    _, pc, pw = rsr.decoder(codes, W, X, Y, sm.REG)
    plain = _disagreement(lambda a, b: rsr.decoder(a, b, X, Y, sm.REG)[0], codes, W, pc, pw, entries)
    composed = _disagreement(lambda a, b: sm.compose(c, a, X, Y, n_pos, w_relation=b, exact_query=True, row_weights=w)["loss"],
                             codes, W, ana["dcodes"], ana["dW"], entries)
    print("%s: central differences at step %g: plain decoder %.3e, composed %.3e" % (name, FD_STEP, plain, composed))
    assert plain <= PLAIN_FD and composed <= 10 * PLAIN_FD
    # the float32 query rows of the mirrors the GPU is held to move the gradient by far less than its bar of 1e-3
    f32 = sm.compose(c, codes, X, Y, n_pos, w_relation=W)
    assert np.abs(f32["dcodes"] - ana["dcodes"]).max() <= 1e-5 * np.abs(ana["dcodes"]).max()
