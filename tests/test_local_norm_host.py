"""IncidenceNormalization=local (RGCN_NORM_LOCAL) without a GPU: the float64 restatement of tests/local_norm_reference.py
against the paper's dense form and against central differences, the input condition of the shared test graph, and the
surface (header values, _native names, the settings key and its refusal)."""
import os
import re

import numpy as np
import pytest

import oracle
import local_norm_reference as ln
from relationprediction_amd.common import model_builder
from test_plugin_surface import BLOCK_EXP, load_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, R, d, L = 12, 4, 8, 2
KINDS = [("block", 4), ("basis", 3), ("onehot", 3)]


def make_params(kind, nb, seed):
    rng = np.random.RandomState(seed)
    if kind == "onehot":
        import featureless_reference as fr
        p = fr.init_params(V, R, d, L, nb, rng)
    else:
        p = oracle.init_params(V, R, d, L, kind, nb, rng=rng)
        p["b_emb"] = (rng.randn(d) * 0.05).astype(np.float32)
    masks = [(rng.rand(V, d) < 0.8).astype(np.uint8) for _ in range(L)]
    return p, masks


def test_input_condition_of_the_shared_graph():
    t = ln.base_graph()
    assert t[:, [0, 2]].max() < V and t[:, 1].max() < R
    lf, lb = ln.message_norms_f32(t, V, "local")
    gf, gb = ln.message_norms_f32(t, V, "intended")
    # vertex 0 receives three edges of relation 0 and one of relation 1; vertex 1 sends the mirror case
    into0, from1 = t[:, 2] == 0, t[:, 0] == 1
    assert sorted(lf[into0].tolist()) == sorted([np.float32(1) / np.float32(3)] * 3 + [1.0]) and (gf[into0] == 0.25).all()
    assert sorted(lb[from1].tolist()) == sorted([np.float32(1) / np.float32(3)] * 3 + [1.0]) and (gb[from1] == 0.25).all()
    assert (lf != gf).any() and (lb != gb).any()
    assert len(np.unique(t, axis=0)) < len(t)                           # a duplicated triple
    assert (t[:, 0] == t[:, 2]).any()                                   # a self-edge
    assert len(np.setdiff1d(np.arange(R), t[:, 1])) >= 1                # a relation with no edge
    dup = (t == np.array([6, 2, 7])).all(axis=1)
    assert dup.sum() == 2 and (lf[dup] == 0.5).all() and (lb[dup] == 0.5).all()      # duplicates count once each
    loop = t[:, 0] == t[:, 2]
    assert (lf[loop] == 1.0).all() and (lb[loop] == 1.0).all()
    for e in (ln.extended_graph(), ln.extended_graph(V=70000, R=5, E=200, hub=False)):
        assert len(np.setdiff1d(np.arange(5), e[:, 1])) >= 1 and len(np.unique(e, axis=0)) < len(e)
    e = ln.extended_graph()
    hub = 39
    for col in (0, 2):
        assert sorted(np.unique(e[e[:, col] == hub][:, 1]).tolist())[:2] == [0, 1]
    assert (e[:, 0] == hub).sum() + (e[:, 2] == hub).sum() > 32         # kLongRow


@pytest.mark.parametrize("kind,nb", KINDS)
def test_forward_equals_the_papers_dense_form(kind, nb):
    """H_l = act( dropout(self) + sum_r A_r H W_r ), A_r the row-normalised multigraph adjacency of relation r per
    direction (R-GCN eq. 2 with c_{i,r} = |N_i^r|), built densely here; to 1e-12."""
    t = ln.base_graph()
    p32, masks = make_params(kind, nb, seed=3)
    p = {k: np.asarray(v, dtype=np.float64) for k, v in p32.items()}
    n_f, n_b = ln.norms(t, V)
    acts = ln.forward(kind, p, t, V, L, n_f, n_b, mode="train", masks=masks)
    A = np.zeros((2, R, V, V))
    for s, r, o in t:
        A[0, r, o, s] += 1.0                 # forward: the object receives from the subject
        A[1, r, s, o] += 1.0
    rows = A.sum(axis=3, keepdims=True)
    A = np.divide(A, rows, out=np.zeros_like(A), where=rows > 0)
    H = None if kind == "onehot" else np.maximum(p["W_emb"] + p["b_emb"], 0.0)
    for l in range(1, L + 1):
        table = kind == "onehot" and l == 1
        X = np.eye(V) if table else H
        Ws = p["W_self%d" % l]
        pre = (X @ Ws) * (masks[l - 1] / 0.8)
        for di, tag in enumerate("fb"):
            W = p["W_%s%d" % (tag, l)]
            for r in range(R):
                if kind == "block":
                    Wr = np.zeros((d, d))
                    sd = d // nb
                    for b in range(nb):      # out[b, i] = sum_j W[r, b, i, j] x[b, j]
                        Wr[b * sd:(b + 1) * sd, b * sd:(b + 1) * sd] = W[r, b].T
                else:
                    Wr = np.einsum("b,ibk->ik", p["C_%s%d" % (tag, l)][r], W)
                pre += A[di, r] @ X @ Wr
        H = np.maximum(pre, 0.0) if l < L else pre
        assert float(np.abs(H - acts[l]).max()) <= 1e-12, (kind, l)


@pytest.mark.parametrize("kind,nb", KINDS)
def test_analytic_gradients_equal_central_differences(kind, nb):
    """loss = <G, codes>; h = 1e-6, relative 1e-6 of the tensor's largest gradient entry; up to 100 entries entry by
    entry, 48 seeded entries of the larger tensors"""
    t = ln.base_graph()
    p32, masks = make_params(kind, nb, seed=4)
    p = {k: np.asarray(v, dtype=np.float64) for k, v in p32.items()}
    n_f, n_b = ln.norms(t, V)
    rng = np.random.RandomState(5)
    G = rng.randn(V, d)

    def loss(q):
        return float((G * ln.forward(kind, q, t, V, L, n_f, n_b, mode="train", masks=masks)[-1]).sum())

    acts = ln.forward(kind, p, t, V, L, n_f, n_b, mode="train", masks=masks)
    grads = ln.backward(kind, p, t, V, L, n_f, n_b, acts, G, mode="train", masks=masks)
    h = 1e-6
    assert set(grads) == set(p) - {"W_relation"}
    for name, g in grads.items():
        assert g.shape == p[name].shape, name
        if re.fullmatch(r"b\d+", name):
            assert not g.any()
            continue
        flat = p[name].reshape(-1)
        picks = np.arange(flat.size) if flat.size <= 100 else rng.choice(flat.size, 48, replace=False)
        scale = max(float(np.abs(g).max()), 1e-12)
        for i in picks:
            keep = flat[i]
            flat[i] = keep + h
            up = loss(p)
            flat[i] = keep - h
            down = loss(p)
            flat[i] = keep
            assert abs((up - down) / (2 * h) - g.reshape(-1)[i]) <= 1e-6 * scale, (name, int(i))


def test_restatement_with_global_norms_is_the_oracle():
    """the same layers fed the oracle's own 'intended' norms reproduce the oracle in float64: what differs under 'local' is
    the norms alone"""
    from helpers import oracle_float64
    t = ln.base_graph()
    for kind, nb in KINDS[:2]:
        p32, masks = make_params(kind, nb, seed=6)
        n_f, n_b = ln.norms(t, V, "intended")
        acts = ln.forward(kind, p32, t, V, L, n_f, n_b, mode="train", masks=masks)
        with oracle_float64():
            p64 = {k: np.asarray(v, dtype=np.float64) for k, v in p32.items()}
            ref = oracle.encoder_forward(p64, t, V, L, kind, mode="train", dropout_masks=masks)
        for a, b in zip(acts, ref):
            assert float(np.abs(a - b).max()) <= 1e-12


def test_native_names_and_header_values():
    from relationprediction_amd import _native
    assert _native.NORMS["local"] == 3 == _native.NORM_LOCAL
    assert _native.NORMS == {"intended": 0, "tf_as_executed": 1, "none": 2, "local": 3}
    assert _native.BUF_MSG_NORM == 11
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgcn.h")).read(), flags=re.S)
    values = {k: int(v) for k, v in re.findall(r"\b(RGCN_[A-Z_0-9]+)\s*=\s*(\d+)", text)}
    assert values["RGCN_NORM_LOCAL"] == 3 and values["RGCN_BUF_MSG_NORM"] == 11
    assert (values["RGCN_NORM_INTENDED"], values["RGCN_NORM_TF_AS_EXECUTED"], values["RGCN_NORM_NONE"]) == (0, 1, 2)
    assert re.search(r"#define\s+RGCN_ABI_VERSION\s+1\b", text)
    for k, v in values.items():                     # the Python mirror of every value of the two enums
        if k.startswith("RGCN_NORM_") or k.startswith("RGCN_BUF_"):
            assert getattr(_native, k[len("RGCN_"):]) == v, k


class _Recorder(Exception):
    pass


def _runtime_norm(tmp_path, monkeypatch, value):
    """build the Toy chain with the key set and ask for its runtime; the engine constructor is replaced by a recorder"""
    from relationprediction_amd import _native
    seen = {}

    def fake_engine(*args, **kwargs):
        seen.update(kwargs)
        raise _Recorder()

    monkeypatch.setattr(_native, "Engine", fake_engine)
    text = BLOCK_EXP if value is None else BLOCK_EXP.replace("\tConcatenation=Yes\n",
                                                             "\tConcatenation=Yes\n\tIncidenceNormalization=%s\n" % value)
    s, enc, dec = load_settings(tmp_path, text)
    model = model_builder.build_decoder(model_builder.build_encoder(enc, np.zeros((43, 3), dtype=int)), dec)
    np.random.seed(1)
    model.initialize_train()
    with pytest.raises(_Recorder):
        model.get_runtime()
    return seen["norm_mode"]


@pytest.mark.parametrize("value", [None, "intended", "tf_as_executed", "none", "local"])
def test_runtime_forwards_the_settings_key(tmp_path, monkeypatch, value):
    from relationprediction_amd import _native
    got = _runtime_norm(tmp_path, monkeypatch, value)
    assert got == (value or "intended") and _native.norm_mode_value(got) == _native.NORMS[got]


def test_unknown_value_is_a_value_error_naming_the_four(tmp_path, monkeypatch):
    from relationprediction_amd import _native
    with pytest.raises(ValueError) as e:
        _runtime_norm(tmp_path, monkeypatch, "per_relation")
    assert not isinstance(e.value, KeyError)
    for name in ("intended", "tf_as_executed", "none", "local"):
        assert name in str(e.value)
    assert "per_relation" in str(e.value)
    with pytest.raises(ValueError):
        _native.norm_mode_value("Local")
    assert _native.norm_mode_value(3) == 3
