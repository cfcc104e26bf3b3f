"""The featureless basis encoder (UseInputTransform=No) without a GPU: the float64 restatement of
tests/featureless_reference.py against the unchanged oracle fed one-hot rows, its analytic gradients against central
differences, and the plugin chain model_builder assembles for the flag."""
import os
import re

import numpy as np
import pytest

import oracle
import featureless_reference as fr
from helpers import oracle_float64
from relationprediction_amd.common import model_builder
from test_plugin_surface import load_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, R, d, B, L, E = 30, 4, 8, 3, 2, 60
NORMS = [oracle.NORM_INTENDED, oracle.NORM_TF_AS_EXECUTED, oracle.NORM_NONE]


def featureless_settings_text():
    """the settings file INTEGRATION.md ships for the mode (the tree carries no settings/ directory)"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"settings/gcn_basis_featureless\.exp`:\n\n```ini\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md lost the featureless settings block"
    return m.group(1)


def toy_settings_text(dim=d, bases=B, layers=L):
    t = featureless_settings_text()
    t = t.replace("InternalEncoderDimension=500", "InternalEncoderDimension=%d" % dim)
    t = t.replace("CodeDimension=500", "CodeDimension=%d" % dim)
    t = t.replace("NumberOfBasisFunctions=5", "NumberOfBasisFunctions=%d" % bases)
    t = t.replace("NumberOfLayers=2", "NumberOfLayers=%d" % layers)
    return t.replace("\tGraphBatchSize=30000\n", "")


@pytest.fixture(scope="module")
def case():
    params, triples, masks, dcodes = fr.make_case(V, R, d, L, B, E, seed=11)
    return {"params": params, "triples": triples, "masks": masks, "dcodes": dcodes}


@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("norm", NORMS)
def test_restatement_equals_the_oracle_fed_onehot_rows(case, mode, norm):
    """H = I makes the oracle's dense path the lookup: I . W.reshape(V, B.d) = W, I . W_self = W_self."""
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in case["params"].items()}
    acts = fr.forward(case["params"], case["triples"], V, L, mode=mode, masks=case["masks"], norm_mode=norm)
    s, r, o = oracle.split_graph(case["triples"])
    with oracle_float64():
        H = np.eye(V)
        for l in range(1, L + 1):
            F, K = oracle.basis_messages(H, s, r, o, p64["W_f%d" % l], p64["W_b%d" % l], p64["C_f%d" % l], p64["C_b%d" % l])
            S = oracle.self_loop(H, p64["W_self%d" % l])
            if mode == "train":
                S = oracle.dropout(S, 0.8, case["masks"][l - 1])
            H = oracle.combine_messages(F, K, S, s, o, V, use_nonlinearity=l < L, norm_mode=norm)
            assert H.dtype == np.float64
            assert float(np.abs(H - acts[l]).max()) <= 1e-12, (l, mode, norm)


@pytest.mark.parametrize("norm", NORMS)
def test_analytic_gradients_equal_central_differences(case, norm):
    """loss = <G, codes> for a fixed random G; h = 1e-6, relative 1e-6 of the tensor's largest gradient entry.  Tensors of
    up to 100 entries entry by entry, 64 seeded entries of the larger ones (every tensor is covered)."""
    rng = np.random.RandomState(5)
    G = rng.randn(V, d)
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in case["params"].items()}

    def loss(p):
        return float((G * fr.forward(p, case["triples"], V, L, mode="train", masks=case["masks"], norm_mode=norm)[-1]).sum())

    acts = fr.forward(p64, case["triples"], V, L, mode="train", masks=case["masks"], norm_mode=norm)
    grads = fr.backward(p64, case["triples"], V, L, acts, G, mode="train", masks=case["masks"], norm_mode=norm)
    h = 1e-6
    for name in fr.weight_names(L)[:-1]:
        g = grads[name]
        assert g.shape == p64[name].shape
        if name.startswith("b"):
            assert not g.any()
            continue
        flat = p64[name].reshape(-1)
        picks = np.arange(flat.size) if flat.size <= 100 else rng.choice(flat.size, 64, replace=False)
        scale = max(float(np.abs(g).max()), 1e-12)
        for i in picks:
            keep = flat[i]
            flat[i] = keep + h
            up = loss(p64)
            flat[i] = keep - h
            down = loss(p64)
            flat[i] = keep
            assert abs((up - down) / (2 * h) - g.reshape(-1)[i]) <= 1e-6 * scale, (name, int(i))


def _chain(model):
    c = model
    while c is not None:
        yield c
        c = c.next_component


def _build(tmp_path, text=None):
    s, enc, dec = load_settings(tmp_path, text or toy_settings_text(), V=V, R=R, E=E)
    model = model_builder.build_decoder(model_builder.build_encoder(enc, np.zeros((E, 3), dtype=int)), dec)
    return model, enc, dec


def test_settings_file_parses(tmp_path):
    s, enc, dec = load_settings(tmp_path, featureless_settings_text())
    assert enc['UseInputTransform'] == 'No' and enc['Name'] == 'gcn_basis' and enc['Concatenation'] == 'No'
    assert enc['NumberOfBasisFunctions'] == '5' and enc['InternalEncoderDimension'] == '500'
    assert s['General']['ExperimentName'] == 'models/GcnBasisFeatureless'


def test_model_builder_builds_the_featureless_chain(tmp_path):
    model, enc, dec = _build(tmp_path)
    assert [type(c).__name__ for c in _chain(model)] == ["BilinearDiag", "RelationEmbedding", "BasisGcn", "BasisGcn",
                                                         "Representation"]
    layers = [c for c in _chain(model) if type(c).__name__ == "BasisGcn"]
    assert [l.onehot_input for l in layers] == [False, True]            # top layer first
    assert [l.use_nonlinearity for l in layers] == [False, True]
    assert model.needs_graph()
    np.random.seed(7)
    model.initialize_train()
    weights = model.get_weights()
    names = fr.weight_names(L)
    expect = fr.init_params(V, R, d, L, B, np.random.RandomState(7))
    assert [w.name for w in weights] == ["W_forward", "W_backward", "C_forward", "C_backward", "W_self", "b"] * L + ["W_relation"]
    assert [tuple(w.shape) for w in weights[:6]] == [(V, B, d), (V, B, d), (R, B), (R, B), (V, d), (d,)]
    assert [tuple(w.shape) for w in weights[6:12]] == [(d, B, d), (d, B, d), (R, B), (R, B), (d, d), (d,)]
    for w, n in zip(weights, names):
        # same numpy stream in the reference's creation order: layer 1's V-sized tensors with std glorot_variance([V, d])
        np.testing.assert_array_equal(w.value(), expect[n], err_msg=n)
    std = 3.0 / np.sqrt(V + d)
    for w in (weights[0], weights[1], weights[4]):
        assert abs(float(w.value().std()) / std - 1.0) < 0.15, w.name


def test_other_input_variants_stay_refused(tmp_path):
    text = toy_settings_text()
    with pytest.raises(NotImplementedError):
        _build(tmp_path, text.replace("Concatenation=No", "Concatenation=Yes").replace("NumberOfBasisFunctions=3", "NumberOfBasisFunctions=4"))
    for key in ("RandomInput", "PartiallyRandomInput"):
        with pytest.raises(NotImplementedError):
            _build(tmp_path, text.replace(key + "=No", key + "=Yes"))


def test_save_load_round_trip_restores_by_position(tmp_path):
    model, _, _ = _build(tmp_path)
    np.random.seed(3)
    model.initialize_train()
    before = [w.value().copy() for w in model.get_weights()]
    model.save(str(tmp_path / "ckpt"))
    other, _, _ = _build(tmp_path)
    np.random.seed(4)
    other.initialize_train()
    assert not np.array_equal(other.get_weights()[0].value(), before[0])
    other.load(str(tmp_path / "ckpt-0.npz"))
    for w, v in zip(other.get_weights(), before):
        np.testing.assert_array_equal(w.value(), v)


# ---- the reference's own model code with the flag flipped (tests/golden/make_reference_featureless_fixture.py)
@pytest.fixture(scope="module")
def ref_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "reference_featureless.npz")) as z:
        fix = {k: z[k] for k in z.files}
    fV, fR, fd, fB, fL, fE, fN, seed = (int(x) for x in fix["config"])
    names = fr.weight_names(fL)
    c = {"V": fV, "R": fR, "d": fd, "B": fB, "L": fL, "seed": seed, "names": names, "fix": fix,
         "params": {n: fix["weight%02d" % i] for i, n in enumerate(names)},
         "masks": [fix["mask%d" % (l + 1)] for l in range(fL)]}
    return c


def test_reference_fixture_weights_are_bitwise_the_restatements_draws(ref_fixture):
    c = ref_fixture
    mine = fr.init_params(c["V"], c["R"], c["d"], c["L"], c["B"], np.random.RandomState(c["seed"]))
    assert len([k for k in c["fix"] if k.startswith("weight")]) == len(c["names"])
    for n in c["names"]:
        assert mine[n].dtype == c["params"][n].dtype == np.float32, n
        np.testing.assert_array_equal(mine[n], c["params"][n], err_msg=n)


def test_restatement_equals_the_reference_dataflow(ref_fixture):
    """tolerances of test_reference_model.py for the same quantities: codes 2e-6 x max(1, scale), loss 2e-6 relative,
    every gradient 2e-5 of its largest entry; the unconnected variables are exactly the per-layer biases"""
    c, fix = ref_fixture, ref_fixture["fix"]
    V, L = c["V"], c["L"]
    test = fr.forward(c["params"], fix["triples"], V, L, mode="test")
    assert float(np.abs(test[-1] - fix["codes_test"]).max()) <= 2e-6 * max(1.0, float(np.abs(fix["codes_test"]).max()))
    train = fr.forward(c["params"], fix["triples"], V, L, mode="train", masks=c["masks"])
    assert float(np.abs(train[-1] - fix["codes_train"]).max()) <= 2e-6 * max(1.0, float(np.abs(fix["codes_train"]).max()))
    with oracle_float64():
        loss, dcodes, d_rel = oracle.distmult_loss_and_grads(train[-1], c["params"]["W_relation"].astype(np.float64),
                                                             fix["X"], fix["Y"], 0.01)
    assert float(loss) == pytest.approx(float(fix["loss_train"]), rel=2e-6)
    grads = fr.backward(c["params"], fix["triples"], V, L, train, dcodes, mode="train", masks=c["masks"])
    grads["W_relation"] = d_rel
    connected = {n: bool(fix["grad%02d_connected" % i]) for i, n in enumerate(c["names"])}
    assert sorted(n for n, ok in connected.items() if not ok) == sorted("b%d" % l for l in range(1, L + 1))
    for i, n in enumerate(c["names"]):
        want = fix["grad%02d" % i]
        if connected[n]:
            scale = max(float(np.abs(want).max()), 1e-6)
            assert float(np.abs(grads[n] - want).max()) <= 2e-5 * scale + 1e-7, n
        else:
            assert not np.asarray(grads[n]).any(), n
