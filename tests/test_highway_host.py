"""SkipConnections=Highway without a GPU: the float64 restatement of tests/highway_reference.py against the vectors
the reference's own model code produced (tests/golden/reference_highway.npz) and against torch-CPU autograd in float64,
and the plugin chain model_builder assembles for the flag."""
import os
import re

import numpy as np
import pytest

import oracle
import highway_reference as hr
from helpers import oracle_float64
from relationprediction_amd.common import model_builder
from test_plugin_surface import load_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["basis", "block"]


def highway_settings_text(kind="basis", dim=500, bases=5, layers=2):
    """the featureless settings file INTEGRATION.md ships, with its [Encoder] section replaced by the highway one"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    full = re.search(r"settings/gcn_basis_featureless\.exp`:\n\n```ini\n(.*?)```", text, re.S)
    enc = re.search(r"settings/gcn_basis_highway\.exp`.*?```ini\n(\[Encoder\]\n.*?)```", text, re.S)
    assert full and enc, "INTEGRATION.md lost a settings block"
    t = enc.group(1) + "\n" + full.group(1)[full.group(1).index("[Decoder]"):]
    assert "SkipConnections=Highway" in t and "UseInputTransform=Yes" in t
    t = t.replace("InternalEncoderDimension=500", "InternalEncoderDimension=%d" % dim)
    t = t.replace("CodeDimension=500", "CodeDimension=%d" % dim)
    t = t.replace("NumberOfBasisFunctions=5", "NumberOfBasisFunctions=%d" % bases)
    t = t.replace("NumberOfLayers=2", "NumberOfLayers=%d" % layers)
    if kind == "block":
        t = t.replace("Concatenation=No", "Concatenation=Yes")
    return t.replace("\tGraphBatchSize=30000\n", "")


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "reference_highway.npz")) as z:
        fix = {k: z[k] for k in z.files}
    V, R, d, E, N, seed = (int(x) for x in fix["config"])
    out = {"V": V, "R": R, "d": d, "E": E, "seed": seed, "triples": fix["triples"], "X": fix["X"], "Y": fix["Y"]}
    for name in CASES:
        nb, L = (int(x) for x in fix[name + "_config"])
        names = hr.weight_names(name, L)
        assert len([k for k in fix if re.fullmatch(name + r"_weight\d\d", k)]) == len(names)
        out[name] = {"kind": name, "nb": nb, "L": L, "names": names,
                     "chain": str(fix[name + "_chain"]).split(","),
                     "params": {n: fix["%s_weight%02d" % (name, i)] for i, n in enumerate(names)},
                     "masks": [fix["%s_mask%d" % (name, l + 1)] for l in range(L)],
                     "grads": {n: fix["%s_grad%02d" % (name, i)] for i, n in enumerate(names)},
                     "connected": {n: bool(fix["%s_grad%02d_connected" % (name, i)]) for i, n in enumerate(names)},
                     "loss": float(fix[name + "_loss_train"]), "codes_train": fix[name + "_codes_train"],
                     "codes_test": fix[name + "_codes_test"]}
    return out


def test_fixture_is_the_two_runs_of_the_reference(fixture):
    assert (fixture["V"], fixture["R"], fixture["d"], fixture["E"]) == (30, 4, 8, 60)
    assert (fixture["basis"]["nb"], fixture["basis"]["L"]) == (3, 2) and (fixture["block"]["nb"], fixture["block"]["L"]) == (4, 3)
    assert fixture["basis"]["loss"] == pytest.approx(27.625767, abs=1e-5)
    assert fixture["block"]["loss"] == pytest.approx(5.515750, abs=1e-5)
    for name, layer in (("basis", "BasisGcn"), ("block", "ConcatGcn")):
        L = fixture[name]["L"]
        assert fixture[name]["chain"] == ["BilinearDiag", "RelationEmbedding"] + ["HighwayLayer", layer] * L + \
            ["AffineTransform", "Representation"]
        for l in range(1, L + 1):       # non-zero gradients for every highway weight
            assert np.abs(fixture[name]["grads"]["W_highway%d" % l]).max() > 0
            assert np.abs(fixture[name]["grads"]["b_highway%d" % l]).max() > 0
            np.testing.assert_array_equal(fixture[name]["params"]["b_highway%d" % l], np.ones(fixture["d"], np.float32))


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_dataflow(fixture, name):
    """the bounds test_featureless_host.py applies to its fixture: codes 2e-6 x max(1, scale), loss 2e-6 relative, every
    gradient 2e-5 of its largest entry; the unconnected variables are exactly the per-layer biases"""
    c, V = fixture[name], fixture["V"]
    L, kind = c["L"], c["kind"]
    test = hr.forward(kind, c["params"], fixture["triples"], V, L, mode="test")[0]
    assert float(np.abs(test[-1] - c["codes_test"]).max()) <= 2e-6 * max(1.0, float(np.abs(c["codes_test"]).max()))
    H, N, T = hr.forward(kind, c["params"], fixture["triples"], V, L, mode="train", masks=c["masks"])
    assert float(np.abs(H[-1] - c["codes_train"]).max()) <= 2e-6 * max(1.0, float(np.abs(c["codes_train"]).max()))
    with oracle_float64():
        loss, dcodes, d_rel = oracle.distmult_loss_and_grads(H[-1], c["params"]["W_relation"].astype(np.float64),
                                                             fixture["X"], fixture["Y"], 0.01)
    assert float(loss) == pytest.approx(c["loss"], rel=2e-6)
    grads = hr.backward(kind, c["params"], fixture["triples"], V, L, H, N, T, dcodes, mode="train", masks=c["masks"])
    grads["W_relation"] = d_rel
    assert sorted(n for n, ok in c["connected"].items() if not ok) == sorted("b%d" % l for l in range(1, L + 1))
    for n in c["names"]:
        want = c["grads"][n]
        if c["connected"][n]:
            scale = max(float(np.abs(want).max()), 1e-6)
            assert float(np.abs(grads[n] - want).max()) <= 2e-5 * scale + 1e-7, n
        else:
            assert not np.asarray(grads[n]).any(), n


def _torch_forward(kind, p, triples, V, L, masks, keep):
    """the forward formulas once more, on float64 torch tensors (dense per-edge form, index_add for the scatter)"""
    import torch
    t = torch.as_tensor(np.asarray(triples, dtype=np.int64))
    s, r, o = t[:, 0], t[:, 1], t[:, 2]
    n_f = torch.as_tensor(np.asarray(oracle.incidence_values(np.asarray(o), V, oracle.NORM_INTENDED), dtype=np.float64))
    n_b = torch.as_tensor(np.asarray(oracle.incidence_values(np.asarray(s), V, oracle.NORM_INTENDED), dtype=np.float64))
    H = torch.relu(p["W_emb"] + p["b_emb"])
    E = len(s)
    for l in range(1, L + 1):
        pre = (H @ p["W_self%d" % l]) * torch.as_tensor(masks[l - 1].astype(np.float64) / keep)
        for tag, rows_in, rows_out, nrm in (("f", s, o, n_f), ("b", o, s, n_b)):
            W = p["W_%s%d" % (tag, l)]
            if kind == "block":
                R, nb, sd, _ = W.shape
                m = torch.einsum("ebij,ebj->ebi", W[r], H[rows_in].reshape(E, nb, sd)).reshape(E, nb * sd)
            else:
                d_in, B, d_out = W.shape
                m = torch.einsum("ebk,eb->ek", (H[rows_in] @ W.reshape(d_in, B * d_out)).reshape(E, B, d_out),
                                 p["C_%s%d" % (tag, l)][r])
            pre = pre.index_add(0, rows_out, m * nrm[:, None])
        n = torch.relu(pre) if l < L else pre
        gate = torch.sigmoid(H @ p["W_highway%d" % l] + p["b_highway%d" % l])
        H = gate * n + (1 - gate) * H
    return H


@pytest.mark.parametrize("kind,nb,L", [("basis", 3, 2), ("block", 4, 3)])
def test_restatement_equals_torch_autograd_in_float64(kind, nb, L):
    import torch
    import local_norm_reference as lnr
    V, R, d = 40, 5, 8
    c = hr.make_case(V, R, d, L, kind, nb, lnr.extended_graph(V, R, 150), seed=3)
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in c["params"].items()}
    out = _torch_forward(kind, p, c["triples"], V, L, c["masks"], c["keep"])
    (out * torch.as_tensor(c["dcodes"].astype(np.float64))).sum().backward()
    H, N, T = hr.forward(kind, c["params"], c["triples"], V, L, mode="train", masks=c["masks"])
    assert float(np.abs(H[-1] - out.detach().numpy()).max()) <= 1e-12
    grads = hr.backward(kind, c["params"], c["triples"], V, L, H, N, T, c["dcodes"], mode="train", masks=c["masks"])
    for n in hr.weight_names(kind, L)[:-1]:
        if re.fullmatch(r"b\d+", n):
            assert p[n].grad is None and not grads[n].any()
            continue
        want = p[n].grad.numpy()
        assert float(np.abs(grads[n] - want).max()) <= 1e-11 * max(1.0, float(np.abs(want).max())), n


def _chain(model):
    c = model
    while c is not None:
        yield c
        c = c.next_component


def _build(tmp_path, text, V, R, E):
    s, enc, dec = load_settings(tmp_path, text, V=V, R=R, E=E)
    return model_builder.build_decoder(model_builder.build_encoder(enc, np.zeros((E, 3), dtype=int)), dec)


@pytest.mark.parametrize("name", CASES)
def test_model_builder_builds_the_highway_chain(tmp_path, fixture, name):
    c = fixture[name]
    V, R, d, E = fixture["V"], fixture["R"], fixture["d"], fixture["E"]
    model = _build(tmp_path, highway_settings_text(name, d, c["nb"], c["L"]), V, R, E)
    assert [type(x).__name__ for x in _chain(model)] == c["chain"]
    layers = [x for x in _chain(model) if type(x).__name__ in ("BasisGcn", "ConcatGcn")]
    assert [l.use_nonlinearity for l in layers] == [False] + [True] * (c["L"] - 1)       # top layer first
    assert not any(l.onehot_input for l in layers) and model.needs_graph()
    np.random.seed(fixture["seed"])
    model.initialize_train()
    weights = model.get_weights()
    per = ["W_forward", "W_backward"] + (["C_forward", "C_backward"] if name == "basis" else []) + ["W_self", "b"]
    assert [w.name for w in weights] == ["W_emb", "b_emb"] + (per + ["W_highway", "b_highway"]) * c["L"] + ["W_relation"]
    for w, n in zip(weights, c["names"]):
        # the same numpy stream consumed in the reference's creation order: bit-equal initial values
        assert w.value().dtype == np.float32 and tuple(w.shape) == c["params"][n].shape, n
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)
    mine = hr.init_params(V, R, d, c["L"], name, c["nb"], np.random.RandomState(fixture["seed"]))
    for n in c["names"]:
        np.testing.assert_array_equal(mine[n], c["params"][n], err_msg=n)


def test_highway_without_input_transform_and_residual_stay_refused(tmp_path):
    text = highway_settings_text("basis", 8, 3, 2)
    with pytest.raises(NotImplementedError, match="one-hot follow-up"):
        _build(tmp_path, text.replace("UseInputTransform=Yes", "UseInputTransform=No"), 30, 4, 60)
    for value in ("Residual", "Dense"):
        with pytest.raises(NotImplementedError, match="SkipConnections other than None"):
            _build(tmp_path, text.replace("SkipConnections=Highway", "SkipConnections=" + value), 30, 4, 60)


def test_save_load_round_trip_keeps_the_highway_weights(tmp_path):
    text = highway_settings_text("block", 8, 4, 3)
    model = _build(tmp_path, text, 30, 4, 60)
    np.random.seed(3)
    model.initialize_train()
    before = [(w.name, w.value().copy()) for w in model.get_weights()]
    assert sum(n == "W_highway" for n, _ in before) == 3 and sum(n == "b_highway" for n, _ in before) == 3
    model.save(str(tmp_path / "ckpt"))
    other = _build(tmp_path, text, 30, 4, 60)
    np.random.seed(4)
    other.initialize_train()
    hw = [i for i, (n, _) in enumerate(before) if n == "W_highway"]
    assert not np.array_equal(other.get_weights()[hw[0]].value(), before[hw[0]][1])
    other.load(str(tmp_path / "ckpt-0.npz"))
    for w, (n, v) in zip(other.get_weights(), before):
        assert w.name == n
        np.testing.assert_array_equal(w.value(), v)
