"""The basis layer with a per-relation diagonal (RGCN_KIND_BASIS_PDIAG, csrc/basis_pdiag.hip) on the GPU, through the C
ABI, against the float64 restatement of tests/add_diagonal_reference.py and the vectors of the reference's own model code
(tests/golden/reference_add_diagonal.npz).  Bounds: activations, the mixing table a (RGCN_BUF_PDIAG_MIX) and the diagonal
aggregate (RGCN_BUF_PDIAG_AGG) FWD_ATOL x max(1, largest |float64 value| of that tensor) against the float64 forward --
the C and D tables are unit-variance and unsquashed, so this layer's activations are not O(1) (17 to 27 on the fixture) --,
gradients helpers.assert_close defaults against the float64 reverse mode evaluated at the engine's own activations (its
own relu gates); the train step's are test_gpu_train_step.py's.  tests/test_add_diagonal_host.py shows on the CPU that a
plain float32 evaluation passes these very checks on these very inputs.  float32 against float64 there, at most: small
cases 1.5e-05 in H (bound 5.0e-03, B 9), 5.7e-07 in a, 3.5e-06 in the aggregate; d = 500: 2.5e-06 in H (bound 6.3e-04),
2.2e-07 in a, 1.1e-06 in the aggregate -- so the bound applies to every case and no case's inputs had to be made smaller."""
import numpy as np
import pytest

import oracle
import local_norm_reference as lnr
import add_diagonal_reference as adr
from helpers import assert_close, oracle_float64
from test_gpu_eval import csr_for
from test_gpu_featureless import adam_float64
from test_gpu_topk import known_lists
from test_plugin_surface import load_settings
from test_add_diagonal_host import (LOCAL_NORM_CASE, SMALL, E, R, V, add_diagonal_settings_text, fwd_bound, load_fixture,
                                    small_case, tile_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def engine(native, c, **kw):
    return native.Engine(c["V"], c["R"], c["d"], c["L"], "basis_pdiag", c["nb"], keep_prob=c["keep"],
                         max_edges=max(len(c["triples"]), 1), **kw)


def forward_by_phases(native, eng, c, train, masks=None, seed=0):
    """the phase API, reading a_l and the diagonal aggregate behind every rgcn_forward_layer_finish; returns (H, A, G)"""
    L = c["L"]
    eng.forward_begin(train=train, seed=seed, masks=masks)
    A, G = [None], [None]
    for l in range(1, L + 1):
        eng.forward_layer_partial(l)
        eng.forward_layer_finish(l)
        A.append(eng.read_buffer(native.BUF_PDIAG_MIX))
        G.append(eng.read_buffer(native.BUF_PDIAG_AGG))
    return [eng.activation(l) for l in range(L + 1)], A, G


def check_pass(native, eng, c, variant, tag, norm="intended"):
    """one forward + backward; variant 'explicit' (the case's masks), 'generated' (the engine's, read back) or 'eval'"""
    Vc, L, B, d = c["V"], c["L"], c["nb"], c["d"]
    train = variant != "eval"
    H, A, G = forward_by_phases(native, eng, c, train, masks=c["masks"] if variant == "explicit" else None, seed=991)
    masks = c["masks"] if variant == "explicit" else [eng.dropout_mask(l) for l in range(1, L + 1)] if train else None
    if variant == "generated":
        assert all(0.6 < m.mean() < 0.95 for m in masks)
    mode = "train" if train else "test"
    rH, rA, rG = adr.forward(c["params"], c["triples"], Vc, L, mode=mode, keep=c["keep"], masks=masks, norm=norm)
    for l in range(1, L + 1):
        assert A[l].shape == (2, Vc, B) and G[l].shape == (Vc, d)
        for name, got, ref in (("H", H[l], rH[l]), ("a", A[l], rA[l]), ("agg", G[l], rG[l])):
            err = float(np.abs(got - ref).max())
            print("%s %s %s%d: max abs err %.3e (scale %.3e)" % (tag, variant, name, l, err, float(np.abs(ref).max())))
            assert err <= fwd_bound(ref), (tag, variant, name, l, err)
    np.testing.assert_array_equal(eng.codes(), H[L])
    eng.backward(c["dcodes"])
    grads = eng.get_grads()
    g64 = adr.backward(c["params"], c["triples"], Vc, L, H, c["dcodes"], mode=mode, keep=c["keep"], masks=masks, norm=norm)
    for n in adr.weight_names(L)[:-1]:
        assert_close(grads[n], g64[n], name="%s %s %s" % (tag, variant, n))
    return grads


@pytest.mark.parametrize("B,d,L", SMALL, ids=["B%d-d%d-L%d" % s for s in SMALL])
def test_parity_small_shapes(native, B, d, L):
    """the graph has a hub row past kLongRow, duplicates, self-edges and a relation without edges; d = 10 takes the scalar
    path of every kernel; L = 3 has a middle layer; B = 8 and B = 9 sit at and past the basis kernels' eight-function tile.
    One engine per case, switched through both arithmetic modes."""
    c = small_case(B, d, L)
    with engine(native, c) as eng:
        assert eng.param_names == adr.weight_names(L)
        assert eng.param_shapes[eng.param_names.index("C_b1")] == (R, B)
        assert eng.param_shapes[eng.param_names.index("D_b1")] == (R, d)
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        for gemm in (6, 0):
            eng.set_gemm_mode(gemm)
            for variant in ("explicit", "generated", "eval"):
                grads = check_pass(native, eng, c, variant, "B%d d%d L%d gemm%d" % (B, d, L, gemm))
        for l in range(1, L + 1):
            assert np.abs(grads["b%d" % l]).max() > 0 and np.abs(grads["C_f%d" % l]).max() > 0
            assert np.abs(grads["D_f%d" % l]).max() > 0 and np.abs(grads["D_b%d" % l]).max() > 0
            for n in ("C_f", "C_b", "D_f", "D_b"):
                assert not grads["%s%d" % (n, l)][R - 1].any(), (n, l)      # the relation without edges


def test_parity_local_norm(native):
    B, d, L = LOCAL_NORM_CASE
    c = small_case(B, d, L)
    with engine(native, c, norm_mode="local") as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        for variant in ("explicit", "eval"):
            check_pass(native, eng, c, variant, "local norm", norm="local")


def test_empty_graph(native):
    c = adr.make_case(V, R, 8, 2, 3, np.zeros((0, 3), np.int32), seed=2)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        grads = check_pass(native, eng, c, "explicit", "empty")
    for n in grads:
        if n[:3] in ("W_f", "W_b", "C_f", "C_b", "D_f", "D_b"):
            assert not grads[n].any(), n
    for l in (1, 2):
        assert np.abs(grads["b%d" % l]).max() > 0 and np.abs(grads["W_self%d" % l]).max() > 0


def test_parity_at_the_real_tile_shapes(native):
    """V = 257, d = 500, B = 2: the GEMMs' real tiles (K = B d = 1000) and the 16-byte path with ragged tails (125 column
    vectors on 128 column lanes, two trips of the wave-per-row kernels).  float32 itself holds the forward bound on these
    inputs (test_add_diagonal_host.py)."""
    c = tile_case()
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        check_pass(native, eng, c, "explicit", "d500")


def test_two_backward_passes_are_bitwise_equal(native):
    c = small_case(3, 8, 3)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        runs = []
        for _ in range(2):
            eng.forward(train=True, masks=c["masks"])
            eng.backward(c["dcodes"])
            runs.append(eng.get_grads())
    for n in runs[0]:
        assert np.array_equal(runs[0][n].view(np.uint32), runs[1][n].view(np.uint32)), n


def test_step_device_twice_agrees_with_forward_and_backward(native):
    """rgcn_step_device ends joined on such a context (no deferred joins): two steps in a row give the same bytes, and the
    bytes of rgcn_forward + rgcn_backward with the same seed"""
    c = small_case(3, 8, 2)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        td, dd = eng.to_device(c["triples"]), eng.to_device(c["dcodes"])
        runs = []
        for _ in range(2):
            eng.step_device(td, len(c["triples"]), dd, train=True, seed=77)
            runs.append(eng.get_grads())
        codes = eng.codes()
        eng.set_graph(c["triples"])
        eng.forward(train=True, seed=77)
        np.testing.assert_array_equal(eng.codes(), codes)
        eng.backward(c["dcodes"])
        runs.append(eng.get_grads())
        td.free(); dd.free()
    for n in runs[0]:
        for other in runs[1:]:
            assert np.array_equal(runs[0][n].view(np.uint32), other[n].view(np.uint32)), n


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


@pytest.mark.parametrize("name", ["b3_l2", "b4_l3"])
def test_loss_and_gradients_of_the_reference_code(native, fixture, name):
    """forward with the reference run's masks, the device decoder, the backward pass: the loss and every gradient the
    reference's own code gave.  Loss: test_gpu_train_step.py's 2e-5 x max(1, |loss|); gradients: its rel = 1e-3."""
    c = fixture[name]
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.decoder_reserve(len(c["X"]))
        xd, yd = eng.to_device(c["X"]), eng.to_device(c["Y"])
        eng.forward(train=True, masks=c["masks"])
        codes = eng.codes()
        eng.decoder_loss_backward_device(xd, yd, len(c["X"]), 0.01)
        loss = eng.loss()
        eng.backward_from_decoder()
        grads = eng.get_grads()
        xd.free(); yd.free()
    assert float(np.abs(codes - c["codes_train"]).max()) <= fwd_bound(c["codes_train"])
    assert abs(loss - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"])), (loss, c["loss"])
    for n in c["names"]:
        assert_close(grads[n], c["grads"][n], rel=1e-3, name=n)


def test_one_train_step_with_clip_and_adam(native, fixture):
    c = fixture["b3_l2"]
    Vc, L, Ec, X, Y = c["V"], c["L"], len(c["triples"]), c["X"], c["Y"]
    names = c["names"]                 # every weight moves: this layer's biases are live parameters
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(X))
        eng.optimizer_config(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0)
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(X), eng.to_device(Y)
        eng.train_step_device(td, Ec, xd, yd, len(X), seed=500, reg_param=0.01)
        loss = eng.loss()
        masks = [eng.dropout_mask(l) for l in range(1, L + 1)]
        grads = eng.get_grads()
        new = eng.get_params()
        for b in (td, xd, yd):
            b.free()
    rH = adr.forward(c["params"], c["triples"], Vc, L, mode="train", masks=masks)[0]
    with oracle_float64():
        oloss, odc, odw = oracle.distmult_loss_and_grads(rH[L], c["params"]["W_relation"].astype(np.float64), X, Y, 0.01)
    assert abs(loss - oloss) <= 2e-5 * max(1.0, abs(oloss)), (loss, oloss)
    og = adr.backward(c["params"], c["triples"], Vc, L, rH, odc, mode="train", masks=masks)
    og["W_relation"] = odw
    for n in names:
        assert_close(grads[n], og[n], rel=1e-3, name="grad " + n)
    # the device update, replayed in numpy from the DEVICE gradients (test_gpu_train_step.py's bound for the same check)
    expect = adam_float64(c["params"], grads, names, 0.01, 0.9, 0.999, 1e-8, 1.0)
    for n in names:
        assert_close(new[n], expect[n], rel=2e-5, spike=2e-4, name="weight " + n)
        assert not np.array_equal(new[n], c["params"][n]), n
    for l in range(1, L + 1):
        assert np.abs(new["b%d" % l]).max() > 0        # (zeros before the step)


def test_plugin_chain_from_the_settings_file(tmp_path, fixture):
    from relationprediction_amd.common import model_builder
    c = fixture["b3_l2"]               # (b4_l3's codes reach 27: nearly every energy saturates the fp32 sigmoid the ranks compare)
    triples = c["triples"]

    def build(seed):
        s, enc, dec = load_settings(tmp_path, add_diagonal_settings_text(c["d"], c["nb"], c["L"]), V=c["V"],
                                    R=c["R"], E=len(triples))
        encoder = model_builder.build_encoder(enc, triples)
        model = model_builder.build_decoder(encoder, dec)
        np.random.seed(seed)
        model.preprocess(triples)
        model.register_for_test(triples)
        model.initialize_train()
        return encoder, model

    encoder, model = build(c["seed"])
    for var, val in zip(model.get_train_input_variables(), (triples, c["X"], c["Y"])):
        var.feed(val)
    test_codes = encoder.get_all_codes(mode='test')[0]
    rt = model.get_runtime()
    assert rt.kind == "basis_pdiag" and rt.engine.param_names == c["names"]
    for w, n in zip(model.get_weights(), c["names"]):
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)       # moved into the engine, bit for bit
    assert float(np.abs(test_codes - c["codes_test"]).max()) <= fwd_bound(c["codes_test"])
    # train-mode codes through the plugin surface: the engine draws its own masks, read back for the float64 forward
    train_codes = model.get_all_codes(mode='train')[0]
    masks = [rt.engine.dropout_mask(l) for l in range(1, c["L"] + 1)]
    rH = adr.forward(c["params"], triples, c["V"], c["L"], mode="train", masks=masks)[0]
    assert float(np.abs(train_codes - rH[-1]).max()) <= fwd_bound(rH[-1])
    # the eager surface: the gradient list follows get_weights()
    loss = model.get_loss('train') + model.get_regularization()
    grads = model.backward()
    assert np.isfinite(loss) and [g.shape for g in grads] == [w.shape for w in model.get_weights()]
    # save / load round trip through the engine-bound variables
    model.save(str(tmp_path / "ckpt"))
    encoder2, model2 = build(c["seed"] + 1)
    model2.get_runtime()
    assert not np.array_equal(model2.get_weights()[4].value(), c["params"]["C_f1"])
    model2.load(str(tmp_path / "ckpt-0.npz"))
    for w, n in zip(model2.get_weights(), c["names"]):
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)
    # filtered ranks against a numpy ranking of the float64 codes' energies, wherever no energy ties with the gold one
    # within rounding: the engine compares fp32 sigmoids, so a gold energy above 5 (sigmoid' below 6.6e-3, where the margin
    # kept here shrinks towards one fp32 step of the score) is left out too; a negative energy saturates only where the
    # fp32 sigmoid leaves the normal range (exp(-87)): this layer's unsquashed tables reach it, so a gold energy below -80
    # is left out as well
    codes64 = adr.forward(c["params"], triples, c["V"], c["L"], mode="test")[0][-1]
    w_rel = c["params"]["W_relation"].astype(np.float64)
    queries = triples[:24].astype(np.int32)
    compared = 0
    for object_side in (True, False):
        known = known_lists(triples, object_side)
        ptr, idx = csr_for(queries, known, object_side)
        raw, filt = model2.device_ranks(triples, queries, object_side, ptr, idx)
        for i, (s, r, o) in enumerate(queries):
            fixed, gold = (s, o) if object_side else (o, s)
            energy = codes64 @ (codes64[fixed] * w_rel[r])
            gap = np.abs(energy - energy[gold])
            gap[gold] = np.inf
            if gap.min() <= 1e-3 * max(1.0, float(np.abs(energy).max())) or energy[gold] > 5.0 or energy[gold] < -80.0:
                continue
            above = energy >= energy[gold]
            lst = idx[ptr[i]:ptr[i + 1]]
            assert raw[i] == int(above.sum()), (object_side, i)
            assert filt[i] == int(above.sum()) - int(above[lst].sum()) + 1, (object_side, i)
            compared += 1
    assert compared >= 10, compared


def test_refusals(native):
    args = (V, R, 8, 2)

    def refused(*a, **kw):
        with pytest.raises(native.RgcnError) as e:
            native.Engine(*a, **kw)
        assert e.value.status == 5, e.value                           # RGCN_ERR_UNSUPPORTED
        return str(e.value)

    assert "sharded" in refused(*args, "basis_pdiag", 3, max_edges=10, world=2, rank=0)
    assert "RGCN_INPUT_ONEHOT" in refused(*args, "basis_pdiag", 3, max_edges=10, input_mode="onehot")
    assert "RGCN_SKIP_HIGHWAY" in refused(*args, "basis_pdiag", 3, max_edges=10, skip="highway")
    assert "NumberOfBasisFunctions > 64" in refused(*args, "basis_pdiag", 65, max_edges=10)
    assert "2^31" in refused(1 << 20, R, 16, 2, "basis_pdiag", 64, max_edges=10)      # 2 V B d = 2^31 exactly
    with native.Engine(*args, "basis_pdiag", 3, max_edges=10) as eng:
        with pytest.raises(native.RgcnError) as e:
            eng.capture_begin()
        assert e.value.status == 5 and "rgcn_capture_begin" in str(e.value)
        with pytest.raises(native.RgcnError) as e:
            eng.read_buffer(native.BUF_PDIAG_MIX)                     # no layer has run yet
        assert e.value.status == 4
        with pytest.raises(native.RgcnError) as e:
            eng.read_buffer(native.BUF_PDIAG_AGG)
        assert e.value.status == 4
    with native.Engine(*args, "basis", 3, max_edges=10) as eng:       # not such a context: no such buffer
        with pytest.raises(native.RgcnError) as e:
            eng.read_buffer(native.BUF_PDIAG_MIX)
        assert e.value.status == 4                                    # RGCN_ERR_STATE
        with pytest.raises(native.RgcnError) as e:
            eng.read_buffer(native.BUF_PDIAG_AGG)
        assert e.value.status == 4


def test_pool_accounting_create_step_destroy():
    """tests/test_gpu_memory_ownership.py's create / destroy accounting, for one basis_pdiag context (devtools build)"""
    import test_gpu_memory_ownership as mo
    from relationprediction_amd import _native
    _native.load_library(devtools=True)
    rng = np.random.RandomState(5)
    graph = np.stack([rng.randint(0, mo.V, mo.E), rng.randint(0, mo.R, mo.E), rng.randint(0, mo.V, mo.E)], 1).astype(np.int32)
    dcodes = (np.random.RandomState(6).randn(mo.V, mo.D) * 0.1).astype(np.float32)
    seen = []
    for _ in range(3):
        eng = _native.Engine(mo.V, mo.R, mo.D, mo.L, "basis_pdiag", mo.NB, max_edges=mo.E, devtools=True)
        try:
            seen.append(eng.device_memory())
            eng.set_graph(graph)
            eng.forward(train=True, seed=1)
            eng.backward(dcodes)
            assert np.isfinite(eng.codes()).all()
            # the step adds the staging copy of the host dcodes (dcodes_own) and nothing else
            assert eng.device_memory() == (seen[-1][0] + 1, seen[-1][1] + 4 * mo.V * mo.D)
        finally:
            eng.close()
    assert seen[0][0] > 0 and seen[0] == seen[1] == seen[2], seen
