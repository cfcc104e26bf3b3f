"""The featureless first layer of the basis encoder (RGCN_INPUT_ONEHOT, csrc/basis_onehot.hip) on the GPU, through the
C ABI, against the float64 restatement of tests/featureless_reference.py.  Bounds are the project's own: activations
FWD_ATOL absolute, gradients helpers.assert_close(rel=2e-4) against the float64 reverse mode of the forward pass the
engine computed (its own activations decide the relu gates); the train step's are test_gpu_train_step.py's for the
basis kind."""
import numpy as np
import pytest

import oracle
import featureless_reference as fr
from helpers import assert_close
from test_featureless_host import toy_settings_text
from test_gpu_eval import csr_for
from test_gpu_topk import assert_rows_equal_reference, known_lists
from test_gpu_train_step import decoder_batch
from test_plugin_surface import load_settings

pytestmark = pytest.mark.gpu

FWD_ATOL = 1e-4
MAIN = dict(V=50, R=5, d=20, B=3, L=2, E=200)
NORMS = ["intended", "tf_as_executed", "none"]


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def engine(native, c, norm="intended"):
    return native.Engine(c["V"], c["R"], c["d"], c["L"], "basis", c["B"], keep_prob=0.8, norm_mode=norm,
                         max_edges=max(len(c["triples"]), 1), input_mode="onehot")


def make(shape, seed, triples=None):
    c = dict(shape)
    c["params"], t, c["masks"], c["dcodes"] = fr.make_case(c["V"], c["R"], c["d"], c["L"], c["B"], c["E"], seed=seed)
    c["triples"] = t if triples is None else triples
    return c


@pytest.fixture(scope="module")
def main_case():
    return make(MAIN, seed=21)


def check_pass(native, c, norm, train):
    """one forward + backward through the C ABI; returns (activations, gradients) of the engine"""
    V, L = c["V"], c["L"]
    with engine(native, c, norm) as eng:
        assert eng.param_names == fr.weight_names(L)
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.forward(train=train, masks=c["masks"] if train else None)
        acts = [None] + [eng.activation(l) for l in range(1, L + 1)]
        with pytest.raises(native.RgcnError) as e:
            eng.activation(0)
        assert e.value.status == 1                      # RGCN_ERR_INVALID: there is no H_0
        eng.backward(c["dcodes"])
        grads = eng.get_grads()
    mode = "train" if train else "test"
    ref = fr.forward(c["params"], c["triples"], V, L, mode=mode, masks=c["masks"], norm_mode=norm)
    for l in range(1, L + 1):
        err = float(np.abs(acts[l] - ref[l]).max())
        print("%s %s H%d: max abs err %.3e" % (norm, mode, l, err))
        assert err <= FWD_ATOL, (l, err)
    g64 = fr.backward(c["params"], c["triples"], V, L, acts, c["dcodes"], mode=mode, masks=c["masks"], norm_mode=norm)
    for n in fr.weight_names(L)[:-1]:
        assert_close(grads[n], g64[n], rel=2e-4, name="%s %s %s" % (norm, mode, n))
    return acts, grads


@pytest.mark.parametrize("train", [True, False], ids=["train", "test"])
@pytest.mark.parametrize("norm", NORMS)
def test_main_case(native, main_case, norm, train):
    check_pass(native, main_case, norm, train)


def test_edge_case_scalar_columns_many_bases_one_layer(native):
    """d % 4 != 0 (scalar columns), B = 9 above the per-launch basis tile of 8, L = 1 (no relu), relation 1 has no edge"""
    c = make(dict(V=40, R=3, d=6, B=9, L=1, E=120), seed=5)
    c["triples"][:, 1] = np.where(c["triples"][:, 1] == 1, 2, c["triples"][:, 1])
    acts, grads = check_pass(native, c, "intended", True)
    assert (acts[1] < 0).any()                                       # the top layer is not rectified
    assert not grads["C_f1"][1].any() and not grads["C_b1"][1].any()
    check_pass(native, c, "intended", False)


def hub_triples(V, R, rng):
    """vertex 0 in 2,500 of 3,000 edges (1,250 as subject, 1,250 as object: 2,500 slots, above kGiantRow = 2048, as a
    receiver and as a sender), vertices 1..5 in 40 edges each (above kLongRow = 32), vertices 250.. in none"""
    mid = lambda n: rng.randint(6, 250, size=n)
    rel = lambda n: rng.randint(0, R, size=n)
    rows = [np.stack([np.zeros(1250, int), rel(1250), mid(1250)], 1), np.stack([mid(1250), rel(1250), np.zeros(1250, int)], 1)]
    for v in range(1, 6):
        rows.append(np.stack([np.full(20, v), rel(20), mid(20)], 1))
        rows.append(np.stack([mid(20), rel(20), np.full(20, v)], 1))
    rows.append(np.stack([mid(300), rel(300), mid(300)], 1))
    t = np.concatenate(rows).astype(np.int32)
    assert len(t) == 3000
    return t[rng.permutation(len(t))]


def test_hub_graph_long_rows_and_silent_vertices(native):
    shape = dict(V=300, R=4, d=8, B=2, L=2, E=3000)
    c = make(shape, seed=9, triples=hub_triples(300, 4, np.random.RandomState(9)))
    deg = np.bincount(np.concatenate([c["triples"][:, 0], c["triples"][:, 2]]), minlength=300)
    assert deg[0] == 2500 and (deg[1:6] == 40).all() and (deg[250:] == 0).all()
    acts, grads = check_pass(native, c, "intended", True)
    silent = np.flatnonzero(deg == 0)
    assert len(silent) >= 50
    assert not grads["W_f1"][silent].any() and not grads["W_b1"][silent].any()
    alone = np.maximum(c["params"]["W_self1"] * (c["masks"][0].astype(np.float32) * (np.float32(1) / np.float32(0.8))), 0)
    np.testing.assert_array_equal(acts[1][silent], alone[silent])


def test_empty_graph(native):
    c = make(dict(V=40, R=3, d=12, B=2, L=2, E=0), seed=2)
    acts, grads = check_pass(native, c, "intended", True)
    for n in ("W_f1", "W_b1", "C_f1", "C_b1", "W_f2", "W_b2", "C_f2", "C_b2"):
        assert not grads[n].any(), n
    c1 = make(dict(V=40, R=3, d=12, B=2, L=1, E=0), seed=2)
    acts1, _ = check_pass(native, c1, "intended", False)
    np.testing.assert_array_equal(acts1[1], c1["params"]["W_self1"])            # codes = W_self: no dropout, no relu


def test_generated_dropout_is_what_the_forward_used(native, main_case):
    c = main_case
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.forward(train=True, seed=1234)
        codes = eng.codes()
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
    assert all(0.6 < m.mean() < 0.95 for m in masks)
    ref = fr.forward(c["params"], c["triples"], c["V"], c["L"], mode="train", masks=masks)
    assert float(np.abs(codes - ref[-1]).max()) <= FWD_ATOL


def test_two_identical_steps_give_the_same_bytes(native, main_case):
    """rgcn_step_device twice on a one-hot context: bitwise equal gradients, equal to the restatement's"""
    c = main_case
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        td, dd = eng.to_device(c["triples"]), eng.to_device(c["dcodes"])
        runs = []
        for _ in range(2):
            eng.step_device(td, len(c["triples"]), dd, train=True, seed=77)
            runs.append(eng.get_grads())
        acts = [None] + [eng.activation(l) for l in range(1, c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
        td.free(); dd.free()
    for n in runs[0]:
        assert np.array_equal(runs[0][n].view(np.uint32), runs[1][n].view(np.uint32)), n
    g64 = fr.backward(c["params"], c["triples"], c["V"], c["L"], acts, c["dcodes"], mode="train", masks=masks)
    for n in fr.weight_names(c["L"])[:-1]:
        assert_close(runs[0][n], g64[n], rel=2e-4, name=n)


def adam_float64(params, grads, names, lr, b1, b2, eps, max_norm):
    """first step of clip_by_global_norm + Adam in float64"""
    gn = np.sqrt(sum(float(np.sum(grads[n].astype(np.float64) ** 2)) for n in names))
    scale = max_norm / max(gn, max_norm)
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    out = {}
    for n in names:
        g = grads[n].astype(np.float64) * scale
        m, v = (1 - b1) * g, (1 - b2) * g * g
        out[n] = params[n].astype(np.float64) - lr_t * m / (np.sqrt(v) + eps)
    return out


def test_one_train_step_with_clip_and_adam(native, main_case):
    c = main_case
    V, L, E = c["V"], c["L"], len(c["triples"])
    X, Y = decoder_batch(np.random.RandomState(2), c["triples"], V)
    names = [n for n in fr.weight_names(L) if not n.startswith("b")]
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(X))
        eng.optimizer_config(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0)
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(X), eng.to_device(Y)
        eng.train_step_device(td, E, xd, yd, len(X), seed=500, reg_param=0.01)
        loss = eng.loss()
        masks = [eng.dropout_mask(l) for l in range(1, L + 1)]
        acts = [None] + [eng.activation(l) for l in range(1, L + 1)]
        grads = eng.get_grads()
        new = eng.get_params()
        for b in (td, xd, yd):
            b.free()
    ref = fr.forward(c["params"], c["triples"], V, L, mode="train", masks=masks)
    assert float(np.abs(acts[L] - ref[L]).max()) <= FWD_ATOL
    oloss, odc, odw = oracle.distmult_loss_and_grads(ref[L].astype(np.float32), c["params"]["W_relation"], X, Y, 0.01)
    assert abs(loss - oloss) <= 5e-5 * max(1.0, abs(oloss)), (loss, oloss)
    og = fr.backward(c["params"], c["triples"], V, L, acts, odc, mode="train", masks=masks)
    og["W_relation"] = odw
    for n in names:
        assert_close(grads[n], og[n], rel=1e-3, name="grad " + n)
    expect = adam_float64(c["params"], grads, names, 0.01, 0.9, 0.999, 1e-8, 1.0)
    for n in names:
        assert_close(new[n], expect[n], rel=2e-5, spike=2e-4, name="weight " + n)
    for n in fr.weight_names(L):
        if n not in names:
            np.testing.assert_array_equal(new[n], c["params"][n])              # the unused biases never move


def test_ranking_and_topk_on_onehot_codes(native, main_case):
    c = main_case
    V = c["V"]
    rng = np.random.RandomState(4)
    queries = c["triples"][rng.choice(len(c["triples"]), 60, replace=False)].copy()
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.forward(train=False)
        codes = eng.codes()
        eng.rank_reserve(64)
        for object_side in (True, False):
            known = known_lists(c["triples"], object_side)
            ptr, idx = csr_for(queries, known, object_side)
            raw, filt = eng.ranks(queries, object_side, ptr, idx)
            oraw, ofilt = oracle.distmult_ranks(codes, c["params"]["W_relation"], queries, object_side, known)
            # (as test_gpu_eval.py: two fp32 products with different summation orders may flip a near-tie by one)
            assert np.mean(raw != oraw) <= 0.02 and np.abs(raw - oraw).max() <= 1
            assert np.mean(filt != ofilt) <= 0.02 and np.abs(filt - ofilt).max() <= 1
            for k in (1, 10, V):
                ids, energy = eng.topk(queries, object_side, k)
                energies = eng.read_buffer(native.BUF_RANK_ENERGIES)[:len(queries)]
                assert_rows_equal_reference(energies, ids, energy, k, None, ("onehot", object_side, k))
                q = codes[queries[:, 0]] * c["params"]["W_relation"][queries[:, 1]] if object_side else \
                    codes[queries[:, 2]] * c["params"]["W_relation"][queries[:, 1]]
                want = q.astype(np.float64) @ codes.astype(np.float64).T
                assert float(np.abs(energies - want).max()) <= 1e-4 * max(1.0, float(np.abs(want).max()))


def test_refusals_are_loud_and_leave_the_library_usable(native, main_case):
    c = main_case
    args = (c["V"], c["R"], c["d"], c["L"])
    with pytest.raises(native.RgcnError) as e:
        native.Engine(*args, "block", 4, max_edges=10, input_mode="onehot")
    assert e.value.status == 5                                        # RGCN_ERR_UNSUPPORTED
    with pytest.raises(native.RgcnError) as e:
        native.Engine(*args, "basis", c["B"], max_edges=10, world=2, rank=0, input_mode="onehot")
    assert e.value.status == 5
    with pytest.raises(native.RgcnError) as e:
        native.Engine(*args, "basis", c["B"], max_edges=10, input_mode=2)
    assert e.value.status == 1                                        # RGCN_ERR_INVALID
    with pytest.raises(native.RgcnError) as e:
        native.Engine(1 << 22, 3, 128, 1, "basis", 4, max_edges=10, input_mode="onehot")     # V B d = 2^31
    assert e.value.status == 5
    with engine(native, c) as eng:
        with pytest.raises(native.RgcnError) as e:
            eng.capture_begin()
        assert e.value.status == 5 and "rgcn_capture_begin" in str(e.value)
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.forward(train=False)
        ref = fr.forward(c["params"], c["triples"], c["V"], c["L"], mode="test")
        assert float(np.abs(eng.codes() - ref[-1]).max()) <= FWD_ATOL


def test_plugin_chain_from_the_settings_file(tmp_path):
    from relationprediction_amd.common import model_builder
    V, R, d, B, L = 16, 9, 20, 3, 2
    import helpers
    triples = helpers.load_graph("toy_train")
    s, enc, dec = load_settings(tmp_path, toy_settings_text(dim=d, bases=B, layers=L), V=V, R=R, E=len(triples))
    model = model_builder.build_decoder(model_builder.build_encoder(enc, triples), dec)
    np.random.seed(3)
    model.preprocess(triples)
    model.register_for_test(triples)
    model.initialize_train()
    weights = model.get_weights()
    names = fr.weight_names(L)
    params = {n: w.value() for w, n in zip(weights, names)}
    rng = np.random.RandomState(0)
    graph = triples[rng.choice(len(triples), 21, replace=False)]
    neg = triples.copy(); neg[:, 2] = rng.randint(0, V, len(triples))
    X = np.concatenate([triples, neg]).astype(np.int32)
    Y = np.concatenate([np.ones(len(triples)), np.zeros(len(triples))]).astype(np.float32)
    # the eager surface: loss and gradients of the chain against the restatement
    for var, val in zip(model.get_train_input_variables(), (graph, X, Y)):
        var.feed(val)
    loss = model.get_loss('train') + model.get_regularization()
    grads = model.backward()
    rt = model.get_runtime()
    assert rt.affine is None and rt.engine.param_names == names
    masks = [rt.engine.dropout_mask(l) for l in range(1, L + 1)]
    acts = [None] + [rt.engine.activation(l) for l in range(1, L + 1)]
    ref = fr.forward(params, graph, V, L, mode="train", masks=masks)
    oloss, dcodes, dWrel = oracle.distmult_loss_and_grads(ref[L].astype(np.float32), params["W_relation"], X, Y, 0.01)
    assert abs(loss - oloss) <= 1e-5 * max(1.0, abs(oloss))
    og = fr.backward(params, graph, V, L, acts, dcodes, mode="train", masks=masks)
    og["W_relation"] = dWrel
    assert len(grads) == len(weights)
    for w, n, g in zip(weights, names, grads):
        assert g.shape == w.shape
        assert_close(g, og[n], rel=5e-4, name=n)
    # the device surface: a train step moves the weights, device_ranks agrees with the eager scoring methods
    model.configure_device_optimizer(0.01, 0.9, 0.999, 1e-8, 1.0)
    model.device_train_step(graph, X, Y, 11)
    assert np.isfinite(model.device_loss())
    assert not np.array_equal(weights[0].value(), params["W_f1"])
    queries = triples[:12].astype(np.int32)
    for object_side in (True, False):
        known = known_lists(triples, object_side)
        ptr, idx = csr_for(queries, known, object_side)
        raw, filt = model.device_ranks(triples, queries, object_side, ptr, idx)
        scores = model.score_all_objects(queries) if object_side else model.score_all_subjects(queries)
        gold = queries[:, 2] if object_side else queries[:, 0]
        eager = (scores >= scores[np.arange(len(queries)), gold][:, None]).sum(axis=1)      # evaluation.py:148-153
        assert np.abs(raw - eager).max() <= 1 and np.mean(raw != eager) <= 0.1
        assert (filt >= 1).all() and (filt <= raw).all()
