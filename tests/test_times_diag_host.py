"""DiagonalCoefficients=Yes without a GPU: the float64 restatement of tests/times_diag_reference.py against the vectors
the reference's own model code produced (tests/golden/reference_times_diag.npz) and against torch-CPU autograd in
float64, the plugin chain model_builder assembles for the flag, and the condition the GPU test's bounds rest on: a plain
float32 evaluation of the same formulas passes, on every GPU case's inputs, the very checks the GPU test applies."""
import os
import re

import numpy as np
import pytest

import oracle
import local_norm_reference as lnr
import times_diag_reference as tdr
from helpers import assert_close, oracle_float64
from relationprediction_amd.common import model_builder
from test_highway_host import highway_settings_text
from test_plugin_surface import load_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["concat_no", "concat_yes"]
LAYER = "BasisGcnTimesDiag"

# ---- what tests/test_gpu_times_diag.py runs (shared, so that the float32 condition below covers exactly its inputs)
FWD_ATOL = 1e-4
V, R, E = 40, 5, 150
# (B, d, L): smallest shape; baseline; scalar path (d % 4 != 0); a middle layer; B equal to one tile of the source-major
# kernel (8 basis functions per launch) and B past one tile
SMALL = [(1, 8, 2), (3, 8, 2), (3, 10, 2), (3, 8, 3), (8, 8, 2), (9, 8, 2)]
LOCAL_NORM_CASE = (3, 8, 2)
TILE = dict(V=257, R=5, d=500, B=2, L=2, E=600)


def small_case(B, d, L):
    return tdr.make_case(V, R, d, L, B, lnr.extended_graph(V, R, E), seed=7 + d + L + B)


def tile_case():
    t = TILE
    return tdr.make_case(t["V"], t["R"], t["d"], t["L"], t["B"], lnr.extended_graph(t["V"], t["R"], t["E"]), seed=31)


def times_diag_settings_text(dim=500, bases=5, layers=2, concat="No"):
    """the highway settings text of INTEGRATION.md with the two flags set the other way: DiagonalCoefficients=Yes,
    SkipConnections=None (every other section, GraphSplitSize=0.5 included, as shipped)"""
    t = highway_settings_text("basis", dim, bases, layers)
    assert "DiagonalCoefficients=No" in t and "SkipConnections=Highway" in t and "Concatenation=No" in t
    t = t.replace("DiagonalCoefficients=No", "DiagonalCoefficients=Yes").replace("SkipConnections=Highway", "SkipConnections=None")
    return t.replace("Concatenation=No", "Concatenation=" + concat)


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "reference_times_diag.npz")) as z:
        fix = {k: z[k] for k in z.files}
    Vf, Rf, d, Ef, N, seed = (int(x) for x in fix["config"])
    out = {"V": Vf, "R": Rf, "d": d, "E": Ef, "seed": seed, "triples": fix["triples"], "X": fix["X"], "Y": fix["Y"]}
    for name in CASES:
        B, L = (int(x) for x in fix[name + "_config"])
        names = tdr.weight_names(L)
        assert len([k for k in fix if re.fullmatch(name + r"_weight\d\d", k)]) == len(names)
        out[name] = {"kind": "basis_tdiag", "nb": B, "L": L, "names": names, "V": Vf, "R": Rf, "d": d, "keep": 0.8,
                     "triples": fix["triples"], "X": fix["X"], "Y": fix["Y"], "seed": seed,
                     "concat": "Yes" if name == "concat_yes" else "No",
                     "chain": str(fix[name + "_chain"]).split(","),
                     "params": {n: fix["%s_weight%02d" % (name, i)] for i, n in enumerate(names)},
                     "masks": [fix["%s_mask%d" % (name, l + 1)] for l in range(L)],
                     "grads": {n: fix["%s_grad%02d" % (name, i)] for i, n in enumerate(names)},
                     "connected": {n: bool(fix["%s_grad%02d_connected" % (name, i)]) for i, n in enumerate(names)},
                     "loss": float(fix[name + "_loss_train"]), "codes_train": fix[name + "_codes_train"],
                     "codes_test": fix[name + "_codes_test"]}
    return out


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_fixture_is_the_two_runs_of_the_reference(fixture):
    assert (fixture["V"], fixture["R"], fixture["d"], fixture["E"]) == (30, 4, 8, 60)
    assert (fixture["concat_no"]["nb"], fixture["concat_no"]["L"]) == (3, 2)
    assert (fixture["concat_yes"]["nb"], fixture["concat_yes"]["L"]) == (4, 2)
    assert fixture["concat_no"]["loss"] == pytest.approx(6.222989, abs=1e-5)
    assert fixture["concat_yes"]["loss"] == pytest.approx(7.346231, abs=1e-5)
    for name in CASES:
        c = fixture[name]
        assert c["chain"] == ["BilinearDiag", "RelationEmbedding"] + [LAYER] * c["L"] + ["AffineTransform", "Representation"]
        assert all(c["connected"].values())       # every weight receives a gradient, the layers' biases included
        for l in range(1, c["L"] + 1):
            assert c["params"]["C_f%d" % l].shape == (fixture["R"], c["nb"], fixture["d"])
            assert np.abs(c["grads"]["b%d" % l]).max() > 0 and np.abs(c["grads"]["C_b%d" % l]).max() > 0


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_dataflow(fixture, name):
    """the bounds test_highway_host.py applies to its fixture: codes 2e-6 x max(1, scale), loss 2e-6 relative, every
    gradient 2e-5 of its largest entry"""
    c, Vf = fixture[name], fixture["V"]
    L = c["L"]
    test = tdr.forward(c["params"], fixture["triples"], Vf, L, mode="test")[0]
    assert float(np.abs(test[-1] - c["codes_test"]).max()) <= 2e-6 * max(1.0, float(np.abs(c["codes_test"]).max()))
    H, P = tdr.forward(c["params"], fixture["triples"], Vf, L, mode="train", masks=c["masks"])
    assert float(np.abs(H[-1] - c["codes_train"]).max()) <= 2e-6 * max(1.0, float(np.abs(c["codes_train"]).max()))
    with oracle_float64():
        loss, dcodes, d_rel = oracle.distmult_loss_and_grads(H[-1], c["params"]["W_relation"].astype(np.float64),
                                                             fixture["X"], fixture["Y"], 0.01)
    assert float(loss) == pytest.approx(c["loss"], rel=2e-6)
    grads = tdr.backward(c["params"], fixture["triples"], Vf, L, H, dcodes, mode="train", masks=c["masks"])
    grads["W_relation"] = d_rel
    for n in c["names"]:
        want = c["grads"][n]
        scale = max(float(np.abs(want).max()), 1e-6)
        assert float(np.abs(grads[n] - want).max()) <= 2e-5 * scale + 1e-7, n


def _torch_forward(p, triples, Vc, L, masks, keep, n_f, n_b):
    """the forward formulas once more, on float64 torch tensors (dense per-edge form, index_add for the scatter)"""
    import torch
    t = torch.as_tensor(np.asarray(triples, dtype=np.int64))
    s, r, o = t[:, 0], t[:, 1], t[:, 2]
    n_f, n_b = torch.as_tensor(n_f), torch.as_tensor(n_b)
    H = torch.relu(p["W_emb"] + p["b_emb"])
    E_ = len(s)
    for l in range(1, L + 1):
        pre = (H @ p["W_self%d" % l]) * torch.as_tensor(masks[l - 1].astype(np.float64) / keep)
        for tag, rows_in, rows_out, nrm in (("f", s, o, n_f), ("b", o, s, n_b)):
            W = p["W_%s%d" % (tag, l)]
            d_in, B, d_out = W.shape
            terms = (H[rows_in] @ W.reshape(d_in, B * d_out)).reshape(E_, B, d_out)
            m = (terms * torch.sigmoid(p["C_%s%d" % (tag, l)][r])).sum(1)
            pre = pre.index_add(0, rows_out, m * nrm[:, None])
        pre = pre + p["b%d" % l]
        H = torch.relu(pre) if l < L else pre
    return H


@pytest.mark.parametrize("norm", ["intended", "local"])
def test_restatement_equals_torch_autograd_in_float64(norm):
    import torch
    c = small_case(3, 8, 3)
    n_f, n_b = lnr.norms(c["triples"], V, norm)
    p = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in c["params"].items()}
    out = _torch_forward(p, c["triples"], V, c["L"], c["masks"], c["keep"], n_f, n_b)
    (out * torch.as_tensor(c["dcodes"].astype(np.float64))).sum().backward()
    H, P = tdr.forward(c["params"], c["triples"], V, c["L"], mode="train", masks=c["masks"], norm=norm)
    assert float(np.abs(H[-1] - out.detach().numpy()).max()) <= 1e-12
    grads = tdr.backward(c["params"], c["triples"], V, c["L"], H, c["dcodes"], mode="train", masks=c["masks"], norm=norm)
    for n in tdr.weight_names(c["L"])[:-1]:
        want = p[n].grad.numpy()
        assert np.abs(want).max() > 0, n
        assert float(np.abs(grads[n] - want).max()) <= 1e-11 * max(1.0, float(np.abs(want).max())), n


def _chain(model):
    c = model
    while c is not None:
        yield c
        c = c.next_component


def _build(tmp_path, text, Vc, Rc, Ec):
    s, enc, dec = load_settings(tmp_path, text, V=Vc, R=Rc, E=Ec)
    return model_builder.build_decoder(model_builder.build_encoder(enc, np.zeros((Ec, 3), dtype=int)), dec)


@pytest.mark.parametrize("name", CASES)
def test_model_builder_builds_the_times_diag_chain(tmp_path, fixture, name):
    """DiagonalCoefficients=Yes selects BasisGcnTimesDiag -- with Concatenation=Yes too (model_builder.py:287-292) -- under
    the shipped GraphSplitSize=0.5, which the reference's own parse_settings cannot read"""
    c = fixture[name]
    Vf, Rf, d, Ef = fixture["V"], fixture["R"], fixture["d"], fixture["E"]
    text = times_diag_settings_text(d, c["nb"], c["L"], concat=c["concat"])
    assert "GraphSplitSize=0.5" in text and "Concatenation=%s" % c["concat"] in text
    model = _build(tmp_path, text, Vf, Rf, Ef)
    assert [type(x).__name__ for x in _chain(model)] == c["chain"]
    layers = [x for x in _chain(model) if type(x).__name__ == LAYER]
    assert [l.use_nonlinearity for l in layers] == [False] + [True] * (c["L"] - 1)       # top layer first
    assert not any(l.onehot_input for l in layers) and model.needs_graph()
    assert all(type(l).KIND == "basis_tdiag" and l.n_coefficients == c["nb"] for l in layers)
    np.random.seed(fixture["seed"])
    model.initialize_train()
    weights = model.get_weights()
    per = ["W_forward", "W_backward", "C_forward", "C_backward", "W_self", "b"]
    assert [w.name for w in weights] == ["W_emb", "b_emb"] + per * c["L"] + ["W_relation"]
    for w, n in zip(weights, c["names"]):
        # the same numpy stream consumed in the reference's creation order: bit-equal initial values
        assert w.value().dtype == np.float32 and tuple(w.shape) == c["params"][n].shape, n
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)
    mine = tdr.init_params(Vf, Rf, d, c["L"], c["nb"], np.random.RandomState(fixture["seed"]))
    for n in c["names"]:
        np.testing.assert_array_equal(mine[n], c["params"][n], err_msg=n)


def test_refused_combinations(tmp_path):
    text = times_diag_settings_text(8, 3, 2)
    with pytest.raises(NotImplementedError, match="DiagonalCoefficients=Yes with UseInputTransform=No"):
        _build(tmp_path, text.replace("UseInputTransform=Yes", "UseInputTransform=No"), 30, 4, 60)
    with pytest.raises(NotImplementedError, match="DiagonalCoefficients=Yes with SkipConnections=Highway"):
        _build(tmp_path, text.replace("SkipConnections=None", "SkipConnections=Highway"), 30, 4, 60)
    with pytest.raises(NotImplementedError, match="AddDiagonal=Yes"):       # ahead of DiagonalCoefficients: stays refused
        _build(tmp_path, text.replace("AddDiagonal=No", "AddDiagonal=Yes"), 30, 4, 60)


def test_save_load_round_trip(tmp_path):
    text = times_diag_settings_text(8, 3, 2)
    model = _build(tmp_path, text, 30, 4, 60)
    np.random.seed(3)
    model.initialize_train()
    before = [(w.name, w.value().copy()) for w in model.get_weights()]
    assert sum(n == "C_forward" for n, _ in before) == 2 and before[4][1].shape == (4, 3, 8)
    model.save(str(tmp_path / "ckpt"))
    other = _build(tmp_path, text, 30, 4, 60)
    np.random.seed(4)
    other.initialize_train()
    assert not np.array_equal(other.get_weights()[4].value(), before[4][1])
    other.load(str(tmp_path / "ckpt-0.npz"))
    for w, (n, v) in zip(other.get_weights(), before):
        assert w.name == n
        np.testing.assert_array_equal(w.value(), v)


# ---- the condition on the GPU test's bounds: float32 itself passes them on the GPU test's inputs
def float32_deviation(c, mode, norm="intended"):
    """per layer (max |H32 - H64|, max |P32 - P64|), and the float32 gradients with their float64 counterparts evaluated
    at the float32 activations (as the GPU test evaluates float64 at the engine's own)"""
    kw = dict(mode=mode, keep=c["keep"], masks=c["masks"] if mode == "train" else None, norm=norm)
    H64, P64 = tdr.forward(c["params"], c["triples"], c["V"], c["L"], **kw)
    H32, P32 = tdr.forward_float32(c["params"], c["triples"], c["V"], c["L"], **kw)
    dev = [(float(np.abs(H32[l] - H64[l]).max()), float(np.abs(P32[l] - P64[l]).max())) for l in range(1, c["L"] + 1)]
    g32 = tdr.backward(c["params"], c["triples"], c["V"], c["L"], H32, c["dcodes"], dtype=np.float32, **kw)
    g64 = tdr.backward(c["params"], c["triples"], c["V"], c["L"], H32, c["dcodes"], **kw)
    return dev, g32, g64


@pytest.mark.parametrize("B,d,L", SMALL, ids=["B%d-d%d-L%d" % s for s in SMALL])
def test_float32_passes_the_gpu_checks_on_the_small_cases(B, d, L):
    c = small_case(B, d, L)
    for mode, norm in [("train", "intended"), ("test", "intended")] + ([("train", "local")] if (B, d, L) == LOCAL_NORM_CASE else []):
        dev, g32, g64 = float32_deviation(c, mode, norm)
        for l, (eh, ep) in enumerate(dev, start=1):
            assert eh <= FWD_ATOL and ep <= FWD_ATOL, (mode, norm, l, eh, ep)
        for n in tdr.weight_names(L)[:-1]:
            assert g32[n].dtype == np.float32
            assert_close(g32[n], g64[n], name="%s %s %s" % (mode, norm, n))


def test_float32_passes_the_gpu_checks_at_the_real_tile_shapes():
    """V 257, d 500, B 2: float32 holds FWD_ATOL on every activation and product of this case (the largest deviation
    printed here is the figure test_gpu_times_diag.py quotes), and assert_close's defaults on every gradient"""
    c = tile_case()
    dev, g32, g64 = float32_deviation(c, "train")
    for l, (eh, ep) in enumerate(dev, start=1):
        print("d500 layer %d: float32 vs float64 max abs H %.3e, P %.3e" % (l, eh, ep))
        assert eh <= FWD_ATOL and ep <= FWD_ATOL, (l, eh, ep)
    for n in tdr.weight_names(c["L"])[:-1]:
        assert_close(g32[n], g64[n], name=n)
