"""IncidenceNormalization=local (RGCN_NORM_LOCAL) on the GPU.  The graph preparation is held BITWISE to a host recount
through RGCN_BUF_MSG_NORM (all four modes, every path into the prep); the encoder is held to the float64 restatement of
tests/local_norm_reference.py with the bounds the existing parity tests apply to the same kernels: activations 1e-4
absolute (test_gpu_parity.py FWD_ATOL), gradients helpers.assert_close with its defaults against the float64 reverse mode
of the forward pass the engine computed."""
import numpy as np
import pytest

import oracle
import featureless_reference as fr
import local_norm_reference as ln
from helpers import assert_close
from test_plugin_surface import BLOCK_EXP

pytestmark = pytest.mark.gpu

FWD_ATOL = 1e-4
NORMS = ["intended", "tf_as_executed", "none", "local"]


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_prep(native, eng, triples, V, R, norm, owned=None, tag=""):
    """RGCN_BUF_MSG_NORM, entry j <-> message RGCN_BUF_PERM_RELATION[j], against the host recount, bitwise.  owned: the
    relations of this rank (None: all)"""
    E = len(triples)
    perm = eng.read_buffer(native.BUF_PERM_RELATION)
    got = eng.read_buffer(native.BUF_MSG_NORM)
    assert perm.shape == got.shape == (2 * E,)
    n = 2 * E if owned is None else 2 * int(np.isin(triples[:, 1], owned).sum())
    perm = perm[:n]
    assert len(np.unique(perm)) == n and (n == 0 or (perm.min() >= 0 and perm.max() < 2 * E))
    if owned is not None:
        assert np.isin(triples[perm % E, 1], owned).all()
    want = ln.message_list_norms(triples, V, R, norm, perm)
    assert np.array_equal(bits(got[:n]), bits(want)), (tag, norm)
    return perm, got[:n]


# ---------------------------------------------------------------------------------------------- 1. the prep, bit-exact
def prep_graphs():
    return {"main": (40, 5, ln.extended_graph(40, 5, 150, seed=1)),
            "one": (40, 5, np.array([[3, 2, 3]], dtype=np.int32)),
            "empty": (40, 5, np.zeros((0, 3), dtype=np.int32)),
            # (V + 1) 2R = 700,010: the (vertex, relation) sort key takes a third byte
            "wide": (70000, 5, np.concatenate([ln.extended_graph(70000, 5, 180, seed=2, hub=False),
                                               np.array([[69999, 1, 69998]] * 3 + [[65536, 0, 69999]] * 2 + [[256, 2, 65535]] * 15,
                                                        dtype=np.int32)]))}


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name", ["main", "one", "empty", "wide"])
def test_prep_is_the_host_recount_bitwise(native, name, norm):
    V, R, t = prep_graphs()[name]
    d = 4 if name == "wide" else 8
    assert name != "wide" or len(t) == 200
    with native.Engine(V, R, d, 1, "block", 2, norm_mode=norm, max_edges=max(len(t), 1)) as eng:
        assert_prep(native, eng_set(eng, t), t, V, R, norm, tag=name)
        if name == "main":
            hub = V - 1
            rp = eng.read_buffer(native.BUF_ROWPTR)
            assert rp[hub + 1] - rp[hub] > 32                            # kLongRow
            # the same context, a smaller graph, the first one again: nothing of the previous graph survives
            assert_prep(native, eng_set(eng, t[:37]), t[:37], V, R, norm, tag="smaller")
            assert_prep(native, eng_set(eng, t), t, V, R, norm, tag="again")


def eng_set(eng, t):
    eng.set_graph(t)
    return eng


def test_local_differs_from_intended_where_it_should(native):
    V, R, t = prep_graphs()["main"]
    out = {}
    for norm in ("intended", "local"):
        with native.Engine(V, R, 8, 1, "basis", 2, norm_mode=norm, max_edges=len(t)) as eng:
            perm, got = assert_prep(native, eng_set(eng, t), t, V, R, norm)
            full = np.empty(2 * len(t), dtype=np.float32)
            full[perm] = got
            out[norm] = full
    E = len(t)
    assert (out["local"][:E] != out["intended"][:E]).any() and (out["local"][E:] != out["intended"][E:]).any()
    assert (out["local"] >= out["intended"]).all()                        # a (relation, row) group is part of its row


def test_wide_key_without_the_relation_in_the_vertex_key(native):
    """(V + 1) 2R >= 2^31: the incidence CSR is keyed by vertex alone, the count runs over the message list sorted by
    destination (one more job of the radix sort)"""
    V, R = 1100000, 1000
    assert (V + 1) * 2 * R >= 2 ** 31
    rng = np.random.RandomState(3)
    t = ln.extended_graph(40, 5, 150, seed=4)
    far = np.stack([rng.randint(V - 300, V, 60), rng.randint(990, 1000, 60), rng.randint(V - 300, V, 60)], 1).astype(np.int32)
    t = np.concatenate([t, far, far[:10], np.array([[V - 1, 999, V - 1]] * 3, dtype=np.int32)])
    t = t[rng.permutation(len(t))]
    with native.Engine(V, R, 4, 1, "basis", 2, norm_mode="local", max_edges=len(t)) as eng:
        assert_prep(native, eng_set(eng, t), t, V, R, "local", tag="bare vertex key")
        assert_prep(native, eng_set(eng, t[:50]), t[:50], V, R, "local", tag="bare vertex key, smaller")


# ---------------------------------------------------------------------------------------------- 2. edge dropout
@pytest.mark.parametrize("norm", ["local", "intended"])
def test_counts_see_the_kept_edges_only(native, norm):
    V, R = 40, 5
    rng = np.random.RandomState(7)
    batch = np.concatenate([ln.extended_graph(V, R, 150, seed=5), ln.extended_graph(V, R, 50, seed=6, hub=False)])
    assert len(batch) == 200
    with native.Engine(V, R, 8, 1, "block", 2, norm_mode=norm, max_edges=200) as eng:
        bd = eng.to_device(batch)
        eng.set_graph_dropout_device(bd, 200, 100, seed=11)
        kept = eng.graph_edges()
        assert kept.shape == (100, 3)
        assert_prep(native, eng, kept, V, R, norm, tag="dropout")
        # a caller's mask instead of the draw
        mask = np.zeros(200, dtype=np.uint8)
        mask[rng.choice(200, 100, replace=False)] = 1
        md = eng.to_device(mask)
        eng.set_graph_dropout_device(bd, 200, 100, seed=0, keep_mask=md)
        kept = eng.graph_edges()
        assert np.array_equal(kept, batch[mask.astype(bool)])
        assert_prep(native, eng, kept, V, R, norm, tag="dropout mask")
        # (what a count over the whole batch would have given these edges is a different array)
        assert (ln.message_norms_f32(batch, V, norm)[0][mask.astype(bool)] != ln.message_norms_f32(kept, V, norm)[0]).any()
        bd.free(); md.free()


# ---------------------------------------------------------------------------------------------- 3. encoder parity
def encoder_case(kind, V, R, d, L, nb, seed):
    rng = np.random.RandomState(seed)
    if kind == "onehot":
        params = fr.init_params(V, R, d, L, nb, rng)
    else:
        params = oracle.init_params(V, R, d, L, kind, nb, rng=rng)
        params["b_emb"] = (rng.randn(d) * 0.05).astype(np.float32)
    masks = [(rng.rand(V, d) < 0.8).astype(np.uint8) for _ in range(L)]
    dcodes = (rng.randn(V, d) * 1e-1).astype(np.float32)
    return dict(kind=kind, V=V, R=R, d=d, L=L, nb=nb, params=params, masks=masks, dcodes=dcodes,
                triples=ln.extended_graph(V, R, 150, seed=seed))


@pytest.fixture(scope="module")
def cases():
    out = {"block": encoder_case("block", 40, 5, 20, 2, 4, 31), "basis": encoder_case("basis", 40, 5, 20, 2, 3, 32),
           "onehot": encoder_case("onehot", 40, 5, 12, 2, 2, 33)}
    for c in out.values():
        c["n_f"], c["n_b"] = ln.norms(c["triples"], c["V"], "local")
        c["ref"] = ln.forward(c["kind"], c["params"], c["triples"], c["V"], c["L"], c["n_f"], c["n_b"], mode="train",
                              masks=c["masks"])
    return out


def make_engine(native, c, norm="local"):
    k = c["kind"]
    return native.Engine(c["V"], c["R"], c["d"], c["L"], "basis" if k == "onehot" else k, c["nb"], keep_prob=0.8,
                         norm_mode=norm, max_edges=len(c["triples"]), input_mode="onehot" if k == "onehot" else "embedding")


@pytest.mark.parametrize("name,fusion", [("block", 0), ("block", 1), ("basis", None), ("onehot", None)])
def test_encoder_equals_the_float64_restatement(native, cases, name, fusion):
    c = cases[name]
    V, L, first = c["V"], c["L"], 1 if name == "onehot" else 0
    with make_engine(native, c) as eng:
        if fusion is not None:
            eng.set_fusion(fusion)
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.forward(train=True, masks=c["masks"])
        acts = [None] * first + [eng.activation(l) for l in range(first, L + 1)]
        eng.backward(c["dcodes"])
        grads = eng.get_grads()
    for l in range(first, L + 1):
        err = float(np.abs(acts[l] - c["ref"][l]).max())
        print("%s fusion %s H%d: max abs err %.3e" % (name, fusion, l, err))
        assert err <= FWD_ATOL, (name, l, err)
    g64 = ln.backward(c["kind"], c["params"], c["triples"], V, L, c["n_f"], c["n_b"], acts, c["dcodes"], mode="train",
                      masks=c["masks"])
    assert set(g64) == set(grads) - {"W_relation"}
    for n, g in g64.items():
        assert_close(grads[n], g, name="%s fusion %s grad %s" % (name, fusion, n))
    # and the mode is not a no-op: the intended norms give other codes
    n_f, n_b = ln.norms(c["triples"], V, "intended")
    other = ln.forward(c["kind"], c["params"], c["triples"], V, L, n_f, n_b, mode="train", masks=c["masks"])
    assert float(np.abs(other[L] - acts[L]).max()) > 100 * FWD_ATOL


# ---------------------------------------------------------------------------------------------- 4. prefetch and capture
@pytest.mark.parametrize("name", ["block", "basis"])
def test_prefetched_and_captured_steps_equal_the_plain_step_bitwise(native, cases, name):
    c = cases[name]
    V, R, t = c["V"], c["R"], c["triples"]
    t2 = np.ascontiguousarray(t[::-1][:120])
    eng, ref = make_engine(native, c), make_engine(native, c)
    held = []
    try:
        for e in (eng, ref):
            e.set_params(c["params"])
            held.append((e.to_device(t), e.to_device(t2), e.to_device(c["dcodes"])))
        (A, B, D), (rA, rB, rD) = held

        def plain(tri_dev, tri, seed):
            ref.set_graph_device(tri_dev, len(tri))
            ref.step_device(tri_dev, len(tri), rD, train=True, seed=seed)
            assert_prep(native, ref, tri, V, R, "local", tag="plain")
            return ref.get_grads(), ref.read_buffer(native.BUF_MSG_NORM)

        def same(got, want, tag):
            for k in want[0]:
                if want[0][k] is not None:
                    assert np.array_equal(bits(got[0][k]), bits(want[0][k])), (tag, k)
            assert np.array_equal(bits(got[1]), bits(want[1])), tag

        # the second GraphBufs set, prepared on the prefetch stream, adopted by the step
        eng.step_device(A, len(t), D, train=True, seed=1)
        eng.prefetch_graph_device(B, len(t2))
        eng.step_device(B, len(t2), D, train=True, seed=2)
        assert_prep(native, eng, t2, V, R, "local", tag="prefetched")
        same((eng.get_grads(), eng.read_buffer(native.BUF_MSG_NORM)), plain(rB, t2, 2), "prefetch")
        eng.prefetch_graph_device(A, len(t))
        eng.step_device(A, len(t), D, train=True, seed=3)
        same((eng.get_grads(), eng.read_buffer(native.BUF_MSG_NORM)), plain(rA, t, 3), "prefetch back")
        # one captured step (its graph preparation inside the capture), replayed
        eng.sync()
        eng.capture_begin()
        eng.step_device(B, len(t2), D, train=True, seed=100)
        gid = eng.capture_end()
        eng.graph_launch(gid)                      # replay 1 draws dropout from (captured seed + 1)
        assert_prep(native, eng, t2, V, R, "local", tag="captured")
        same((eng.get_grads(), eng.read_buffer(native.BUF_MSG_NORM)), plain(rB, t2, 101), "capture")
        eng.graph_destroy(gid)
    finally:
        for bufs in held:
            for b in bufs:
                b.free()
        eng.close()
        ref.close()


def test_fused_minibatch_step_counts_the_kept_edges(native, cases):
    c = cases["block"]
    V, R = c["V"], c["R"]
    batch = np.concatenate([c["triples"], ln.extended_graph(V, R, 50, seed=8, hub=False)])
    n, keep, rate = len(batch), 100, 2
    N = n * (rate + 1)
    with native.Engine(V, R, c["d"], c["L"], "block", c["nb"], norm_mode="local", max_edges=n) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(N)
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        bd, xd, yd = eng.to_device(batch), native.DeviceBuffer(eng, 12 * N), native.DeviceBuffer(eng, 4 * N)
        eng.prefetch_graph_dropout_device(bd, n, keep, 21)
        eng.train_step_minibatch_device(bd, n, keep, 21, rate, 22, xd, yd, seed=23, reg_param=0.01)
        kept = eng.graph_edges()
        assert_prep(native, eng, kept, V, R, "local", tag="prefetched minibatch")
        eng.train_step_minibatch_device(bd, n, keep, 31, rate, 32, xd, yd, seed=33, reg_param=0.01)
        kept2 = eng.graph_edges()
        assert not np.array_equal(kept, kept2)
        assert_prep(native, eng, kept2, V, R, "local", tag="minibatch")
        assert np.isfinite(eng.loss())
        for b in (bd, xd, yd):
            b.free()


# ---------------------------------------------------------------------------------------------- 5. sharding
@pytest.mark.parametrize("norm", ["local", "intended"])
def test_each_rank_holds_the_single_context_values_of_its_messages(native, norm):
    V, R, t = prep_graphs()["main"]
    owner = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    with native.Engine(V, R, 8, 1, "block", 2, norm_mode=norm, max_edges=len(t)) as single:
        perm, got = assert_prep(native, eng_set(single, t), t, V, R, norm)
        whole = np.empty(2 * len(t), dtype=np.float32)
        whole[perm] = got
    seen = []
    for rank in (0, 1):
        with native.Engine(V, R, 8, 1, "block", 2, norm_mode=norm, max_edges=len(t), rank=rank, world=2) as eng:
            eng.set_relation_owner(owner)
            mine = np.flatnonzero(owner == rank)
            perm, got = assert_prep(native, eng_set(eng, t), t, V, R, norm, owned=mine, tag="rank %d" % rank)
            assert np.array_equal(bits(got), bits(whole[perm]))
            seen.append(perm)
    assert sorted(np.concatenate(seen).tolist()) == list(range(2 * len(t)))


# ---------------------------------------------------------------------------------------------- 6. the plugin chain
def _toy_model(tmp_path, norm, triples, V, R):
    from relationprediction_amd import train
    from relationprediction_amd.common import settings_reader
    text = BLOCK_EXP if norm is None else BLOCK_EXP.replace("\tConcatenation=Yes\n",
                                                            "\tConcatenation=Yes\n\tIncidenceNormalization=%s\n" % norm)
    p = tmp_path / ("toy_%s.exp" % norm)
    p.write_text(text)
    _, model = train.build_model(settings_reader.read(str(p)), triples, V, R)      # what train and predict both call
    np.random.seed(3)
    train.initialize_model(model, triples)
    return model


def test_plugin_chain_runs_in_the_mode_of_the_settings_file(native, tmp_path):
    import helpers
    V, R, L = 16, 9, 2
    triples = helpers.load_graph("toy_train")
    models = {norm: _toy_model(tmp_path, norm, triples, V, R) for norm in ("local", None)}
    model = models["local"]
    assert model.get_runtime().engine.cfg.norm_mode == native.NORM_LOCAL
    assert models[None].get_runtime().engine.cfg.norm_mode == native.NORM_INTENDED
    weights = model.get_weights()
    params = {n: w.value() for w, n in zip(weights, oracle.weight_names("block", L))}
    X = triples[:8].astype(np.int32)
    for var, val in zip(model.get_test_input_variables(), (triples, X)):
        var.feed(val)
    codes = np.asarray(model.next_component.get_all_codes(mode='test')[0])
    n_f, n_b = ln.norms(triples, V, "local")
    ref = ln.forward("block", params, triples, V, L, n_f, n_b, mode="test")
    assert float(np.abs(codes - ref[L]).max()) <= FWD_ATOL
    g_f, g_b = ln.norms(triples, V, "intended")
    assert float(np.abs(ln.forward("block", params, triples, V, L, g_f, g_b, mode="test")[L] - codes).max()) > 100 * FWD_ATOL
    # a checkpoint of this model, loaded into a chain built from the same settings (what predict does), encodes alike
    model.save(str(tmp_path / "ckpt"))
    again = _toy_model(tmp_path, "local", triples, V, R)
    again.load(str(tmp_path / "ckpt-0.npz"))
    for var, val in zip(again.get_test_input_variables(), (triples, X)):
        var.feed(val)
    assert np.array_equal(np.asarray(again.next_component.get_all_codes(mode='test')[0]), codes)
    # three device train steps on the same seeds in both modes
    rng = np.random.RandomState(0)
    graph = triples[rng.choice(len(triples), 21, replace=False)]
    neg = triples.copy(); neg[:, 2] = rng.randint(0, V, len(triples))
    X = np.concatenate([triples, neg]).astype(np.int32)
    Y = np.concatenate([np.ones(len(triples)), np.zeros(len(triples))]).astype(np.float32)
    losses = {}
    for norm, m in models.items():
        m.configure_device_optimizer(0.01, 0.9, 0.999, 1e-8, 1.0)
        losses[norm] = []
        for step in range(3):
            m.device_train_step(graph, X, Y, 11 + step)
            losses[norm].append(float(m.device_loss()))
    print("losses local %s intended %s" % (losses["local"], losses[None]))
    assert np.isfinite(losses["local"]).all() and np.isfinite(losses[None]).all()
    assert losses["local"] != losses[None]
