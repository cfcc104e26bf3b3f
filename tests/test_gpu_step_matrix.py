"""The decoder's loss terms and row weights on every encoder form, on the GPU (tests/step_matrix.py's table), against the
float64 mirror composed there from the options' and the forms' own reference modules.

The bars are the fused-step tests' own: the loss and every gradient through helpers.assert_close(rel = 1e-3) against the
mirror, the adversarial weights within adversarial_reference's derived tolerance.  Where a form's activations can be read
back behind a fused step (every form but highway) the mirror is evaluated at the engine's own codes and activations -- its
own relu gates --, the encoder's own parameters keep the forms' own tighter bar there (assert_close's default rel = 2e-4,
fullgraph_grid.check_gradients'), and the codes are held to the float64 forward under the engine's masks within FWD_ATOL
of their scale.  A highway context is held to the float64 forward under the engine's masks throughout, the route
test_gpu_highway.py::test_one_train_step_with_clip_and_adam takes.

Every test prints one line per case: the loss's relative error, the worst adversarial weight error as a fraction of its
tolerance, and `max / l2` relative error of every parameter's gradient.

Read from a run on an MI355X, the worst figure over the 34 cases held to the mirror: codes 3.1e-07 of their scale (bar
1e-4), loss 2.4e-08 relative (bar 1e-3), adversarial weights 0.13 of their tolerance, gradients 7.2e-07 max / 4.8e-07 l2
relative (W_highway2 of highway-all-terms; bar 5e-3 / 1e-3) -- the highway cases, held to the float64 forward, sit at
2e-07 to 7e-07, every other form at 3e-08 to 4e-07.  No case exposed a mismatch.  The first case of the module takes 0.4 s (the library
loads), every other one under 0.05 s.
"""
import functools
import time

import numpy as np
import pytest

import entity_softmax_reference as esr
import helpers
import step_matrix as sm

pytestmark = pytest.mark.gpu

SEED, ESEED, NSEED = 60, 41, 91          # dropout, edge dropout, negatives


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case with its form's graph, weights and batches: built once per module and never written to."""
    c = sm.case_inputs(name)
    for a in [c["triples"], c["known"], c["batch"], c["X"], c["Y"]] + list(c["masks"]) + list(c["params"].values()):
        a.setflags(write=False)
    return c


def make_engine(native, c, max_edges):
    eng = native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], keep_prob=sm.KEEP, norm_mode=c["norm"],
                        max_edges=max_edges, input_mode=c["input_mode"], skip=c["skip"], code_dim=c["code_dim"] or None)
    try:
        assert eng.param_names == sm.weight_names(c), eng.param_names
        eng.set_params(c["params"])
    except Exception:
        eng.close()
        raise
    return eng


def switch_on(eng, c, n_pos, count=None):
    """the reserves and the setters of the case's options; count: num_positives of the three setters (0: the minibatch
    step's batch rows)"""
    count = n_pos if count is None else count
    if c["relsm_exclusive"] or c["entsm_exclusive"] or c["mode"] == "exclusive":
        eng.known_positives_reserve(c["known"])
    eng.relation_softmax_reserve(n_pos)
    eng.set_adversarial_negatives(c["adv"], count)
    eng.set_relation_softmax(c["relsm"], count, exclusive=c["relsm_exclusive"])
    if c["entsm"]:
        eng.entity_softmax_reserve(n_pos)
        eng.set_entity_softmax(c["entsm"], c["entsm_count"] or count, exclusive=c["entsm_exclusive"])
    if c["mode"]:
        kind, m, recip = sm.MODES[c["mode"]]
        if kind == "exclusive":
            eng.set_exclusive_negatives(True)
        if kind == "typed":
            eng.type_sets_reserve(c["known"])
            eng.set_typed_negatives(True)
        if m:
            eng.set_relation_negatives(m)
        if recip:
            eng.set_reciprocal_relations(True)


def read_step(native, eng, c, N):
    """what a fused step left: loss, gradients, weights, masks, codes and the activations that can be read back"""
    got = {"loss": eng.loss(), "grads": eng.get_grads(), "w": eng.read_buffer(native.BUF_ADVERSARIAL_WEIGHTS)[:N],
           "masks": [eng.dropout_mask(l) for l in range(1, c["L"] + 1)], "codes": eng.codes()}
    assert got["codes"].shape == (c["V"], c["dc"])
    if sm.readable(c):
        first = 1 if c["input_mode"] == "onehot" else 0
        got["acts"] = {"H": [None] * first + [eng.activation(l) for l in range(first, c["L"] + 1)], "codes": got["codes"]}
    return got


def same_bytes(a, b, tag):
    assert a["loss"] == b["loss"], (tag, a["loss"], b["loss"])
    assert a["w"].tobytes() == b["w"].tobytes(), tag + ": adversarial weights"
    for k in a["grads"]:
        np.testing.assert_array_equal(a["grads"][k], b["grads"][k], err_msg="%s grad %s" % (tag, k))


def hold_to_the_mirror(c, got, X, Y, n_pos, graph, started):
    """the comparison of one step; returns the composed mirror at the engine's own codes"""
    name = c["name"]
    tail = n_pos if c["mode"] and sm.MODES[c["mode"]][2] else 0
    ref = sm.forward64(c, got["masks"], graph)
    # FWD_ATOL is the forms' own bound at codes of order 1; these codes reach 5 to 50, so it is taken of their scale
    code_err = float(np.abs(got["codes"] - ref["codes"]).max()) / max(1.0, float(np.abs(ref["codes"]).max()))
    assert code_err <= sm.FWD_ATOL, "%s codes against float64: %.3e of their scale" % (name, code_err)
    for m in got["masks"]:
        assert set(np.unique(m)) == {0, 1} and 0.7 < m.mean() < 0.9
    if sm.readable(c):
        out, g64 = sm.mirror_step(c, X, Y, n_pos, got["masks"], graph, acts=got["acts"])
        at_engine = out
    else:
        out, g64 = sm.mirror_step(c, X, Y, n_pos, got["masks"], graph, acts=ref)
        at_engine = sm.compose(c, got["codes"], X, Y, n_pos)
    sm.check_options_count(c, at_engine, n_pos)
    # the adversarial weights: adversarial_reference's derived tolerance, at the engine's own codes
    w_err = np.abs(got["w"].astype(np.float64) - at_engine["w"])
    w_frac = float((w_err / np.maximum(at_engine["tol"], 1e-300))[at_engine["tol"] > 0].max())
    report = ["loss %.1e" % (abs(got["loss"] - at_engine["loss"]) / abs(at_engine["loss"])), "w %.2f of tol" % w_frac]
    print_line = lambda: print("%s [%.2f s]: codes %.1e; %s" % (name, time.time() - started, code_err, "; ".join(report)))
    try:
        assert (w_err <= at_engine["tol"]).all(), "%s adversarial weights: %.3e of the tolerance" % (name, w_frac)
        assert (got["w"][:n_pos] == 1).all() and (got["w"][len(X) - tail:] == 1).all()      # positives, inverse positives
        helpers.assert_close(np.array([got["loss"]]), np.array([at_engine["loss"]]), rel=1e-3, name=name + " loss")
        helpers.assert_close(got["grads"]["W_relation"], at_engine["dW"], rel=1e-3, name=name + " W_relation at the engine's codes")
        # at the engine's own activations the encoder's parameters keep the forms' own bar, assert_close's default
        report += sm.check_gradients(c, got["grads"], g64, rel=2e-4 if sm.readable(c) else 1e-3)
    finally:
        print_line()
    return at_engine


# ------------------------------------------------------------------ a. all three terms on every form
def xy_step(native, c, read_g=False):
    X, Y, P = c["X"], c["Y"], sm.P_STEP
    N, E = len(X), len(c["triples"])
    with make_engine(native, c, E) as eng:
        eng.decoder_reserve(N)
        switch_on(eng, c, P)
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(X), eng.to_device(Y)
        runs = []
        for _ in range(2):
            eng.train_step_device(td, E, xd, yd, N, seed=SEED, reg_param=sm.REG)
            runs.append(read_step(native, eng, c, N))
        if read_g:
            runs[0]["G_ent"] = eng.read_buffer(native.BUF_ENTITY_SOFTMAX_G)
            runs[0]["G_rel"] = eng.read_buffer(native.BUF_RELATION_SOFTMAX_G)
            runs[0]["plans"] = (eng._entsm_plan, eng._relsm_plan)
        for b in (td, xd, yd):
            b.free()
    # twice the same bytes: a race between the streams the terms fork and join on would show here
    same_bytes(runs[0], runs[1], c["name"] + " run twice")
    return runs[0]


@pytest.mark.parametrize("name", sm.ALL_TERMS)
def test_all_terms_on_every_form(native, name):
    """rgcn_train_step_device with X / Y given under rgcn_set_adversarial_negatives, rgcn_set_relation_softmax and
    rgcn_set_entity_softmax together, no optimizer: twice the same bytes; loss, every parameter's gradient (W_out, b_out,
    W_highway*, b_highway* where present) and the adversarial weights against the composed mirror."""
    started = time.time()
    c = inputs(name)
    got = xy_step(native, c)
    hold_to_the_mirror(c, got, c["X"], c["Y"], sm.P_STEP, c["triples"], started)


# ------------------------------------------------------------------ b. both masks inside the step
@pytest.mark.parametrize("name", sm.MASKED)
def test_masked_terms_in_the_step(native, name):
    """the same step with exclusive = True on both terms behind rgcn_known_positives_reserve(graph + more known triples):
    the mirror under the masks, and both G buffers exactly zero outside the candidate sets and in the pad columns"""
    started = time.time()
    c = inputs(name)
    V, P = c["V"], sm.P_STEP
    got = xy_step(native, c, read_g=True)
    out = hold_to_the_mirror(c, got, c["X"], c["Y"], P, c["triples"], started)
    ent_plan, rel_plan = got["plans"]
    G, mask = got["G_ent"], out["ent"]["mask"]
    assert 2 * P <= ent_plan["chunk"] and G.shape[1] == ent_plan["padded_v"] == (V + 3) // 4 * 4
    assert mask.shape == (2 * P, V) and 3 * int((~mask).any(axis=1).sum()) >= 2 * P
    assert not G[:2 * P, V:].any()                                       # the pad columns
    assert not G[:2 * P, :V][~mask].any()                                # exactly zero outside the candidate sets
    gold = esr.rows_of(c["X"][:P])[2]
    assert (G[np.arange(2 * P), gold] < 0).all()                         # the gold is inside: softmax - 1 < 0
    helpers.assert_close(G[:2 * P, :V], out["ent"]["G"], rel=1e-3, name=name + " entity G")
    G, mask = got["G_rel"], out["rel"]["mask"]
    assert P <= rel_plan["chunk"] and G.shape[1] == rel_plan["padded_r"] >= sm.R
    assert mask.shape == (P, sm.R) and 3 * int((~mask).any(axis=1).sum()) >= P
    assert not G[:P, sm.R:].any() and not G[:P, :sm.R][~mask].any()
    assert (G[np.arange(P), c["X"][:P, 1]] < 0).all()
    helpers.assert_close(G[:P, :sm.R], out["rel"]["G"], rel=1e-3, name=name + " relation G")


# ------------------------------------------------------------------ c. the sampling modes stacked with the terms
@pytest.mark.parametrize("name", sm.MINIBATCH)
def test_minibatch_modes(native, name):
    """rgcn_train_step_minibatch_device under each sampling mode with every term the mode is legal with: X[:n] is the
    batch, the rows are the mode's stand-alone samplers' (reciprocal_reference over the samplers' own mirrors, bit for
    bit), and the step is the composed mirror's on those rows and on the graph the edge dropout drew."""
    started = time.time()
    c = inputs(name)
    n, batch = sm.N_BATCH, c["batch"]
    kind, m, recip = sm.MODES[c["mode"]]
    N = n * (sm.RATE + 1 + m) + (n if recip else 0)
    want_X, want_Y, n_pos = sm.mirror_batch(c, NSEED)
    assert n_pos == n and len(want_X) == N
    with make_engine(native, c, n) as eng:
        eng.decoder_reserve(N)
        switch_on(eng, c, n, count=0)
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        eng.train_step_minibatch_device(bd, n, sm.KEEP_EDGES, ESEED, sm.RATE, NSEED, xd, yd, seed=SEED, reg_param=sm.REG)
        got = read_step(native, eng, c, N)
        graph = eng.graph_edges()
        X, Y = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        for b in (bd, xd, yd):
            b.free()
    np.testing.assert_array_equal(X[:n], batch)
    assert len(graph) == sm.KEEP_EDGES and set(map(tuple, graph.tolist())) <= set(map(tuple, batch.tolist()))
    assert X.tobytes() == want_X.tobytes() and Y.tobytes() == want_Y.tobytes(), name + ": the rows are not the samplers'"
    if recip:
        assert np.array_equal(X[N - n:, 1], batch[:, 1] + sm.R) and (X[n:N - n, 1] >= sm.R).any()
    out = hold_to_the_mirror(c, got, X, Y, n, graph, started)
    if recip:
        # the inverse relations' rows take a gradient -- all but R + (R - 1): the graph has no edge of relation R - 1
        inverse = np.abs(got["grads"]["W_relation"][sm.R:2 * sm.R]).max(axis=1) > 0
        assert (got["w"][N - n:] == 1).all() and inverse[:sm.R - 1].all()
        assert np.array_equal(inverse, np.abs(out["dW"][sm.R:2 * sm.R]).max(axis=1) > 0)
        assert not got["grads"]["W_relation"][2 * sm.R:].any()
    if c["entsm_count"]:
        assert len(out["ent"]["ell"]) == 2 * sm.LEADING


# ------------------------------------------------------------------ d. everything on, then everything off
@pytest.mark.parametrize("name", sm.OFF)
def test_switching_everything_off_restores_every_byte(native, name):
    """every option set and reset -- the three terms with both masks, exclusive and typed negatives, relation rows, and
    (with the entity term off again, which refuses it) reciprocal relations: loss, gradients and updated weights of both
    fused steps equal those of a context that never called a setter."""
    c = inputs(name)
    n, batch, X, Y = sm.N_BATCH, c["batch"], c["X"], c["Y"]
    E, N = len(c["triples"]), sm.N_BATCH * (sm.RATE + 1)
    seen = []
    for touch in (False, True):
        with make_engine(native, c, E) as eng:
            eng.decoder_reserve(max(N, len(X)))
            eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
            td, xd, yd = eng.to_device(c["triples"]), eng.to_device(X), eng.to_device(Y)
            bd, xs, ys = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
            if touch:
                on = dict(c, mode="typed+relation", relsm_exclusive=True, entsm_exclusive=True)
                switch_on(eng, on, n, count=sm.P_STEP)
                eng.set_exclusive_negatives(True)
                eng.set_adversarial_negatives(0.0)
                eng.set_relation_softmax(0.0)
                eng.set_entity_softmax(0.0)
                eng.set_reciprocal_relations(True)
                eng.set_reciprocal_relations(False)
                eng.set_exclusive_negatives(False)
                eng.set_typed_negatives(False)
                eng.set_relation_negatives(0)
            got = []
            eng.train_step_device(td, E, xd, yd, len(X), seed=SEED, reg_param=sm.REG)
            got.append((eng.loss(), eng.get_grads(), eng.get_params()))
            eng.train_step_minibatch_device(bd, n, sm.KEEP_EDGES, ESEED, sm.RATE, NSEED, xs, ys, seed=SEED + 1, reg_param=sm.REG)
            got.append((eng.loss(), eng.get_grads(), eng.get_params(), xs.download(np.int32, (N, 3))))
            seen.append(got)
            for b in (td, xd, yd, bd, xs, ys):
                b.free()
    for step, (a, b) in enumerate(zip(*seen)):
        assert a[0] == b[0] and np.isfinite(a[0]), (name, step, a[0], b[0])
        for k in a[1]:
            np.testing.assert_array_equal(a[1][k], b[1][k], err_msg="step %d grad %s" % (step, k))
            np.testing.assert_array_equal(a[2][k], b[2][k], err_msg="step %d weight %s" % (step, k))
            assert sm.unused_bias(c, k) or not np.array_equal(a[2][k], c["params"][k]), k      # the optimizer moved it
    np.testing.assert_array_equal(seen[0][1][3], seen[1][1][3])
