"""Highway skip connections (RGCN_SKIP_HIGHWAY, csrc/highway.hip) on the GPU, through the C ABI, against the float64
restatement of tests/highway_reference.py and the vectors of the reference's own model code
(tests/golden/reference_highway.npz).  Bounds are the project's own: activations (H_l, N_l, T_l) FWD_ATOL absolute
against the float64 forward, gradients helpers.assert_close defaults against the float64 reverse mode evaluated at the
engine's own H_l, N_l and T_l (its own relu gates); the train step's are test_gpu_train_step.py's."""
import ctypes

import numpy as np
import pytest

import oracle
import highway_reference as hr
import local_norm_reference as lnr
from helpers import assert_close
from test_gpu_eval import csr_for
from test_gpu_featureless import adam_float64
from test_gpu_topk import known_lists
from test_highway_host import highway_settings_text
from test_plugin_surface import load_settings

pytestmark = pytest.mark.gpu

FWD_ATOL = 1e-4
# Layer 2 of the block case at d = 500 (test_parity_at_the_real_tile_shapes): N_2 and H_2 reach 1.4e+2 and 1.2e+2 there,
# where 1e-4 absolute is 1e-6 relative -- below what one fp32 evaluation can hold.  Measured on the CPU, on that case's
# inputs: highway_reference.forward_float32 (numpy float32, one summation order) against highway_reference.forward
# (float64) differs by at most 6.124e-05 in N_2 and 5.559e-05 in H_2 (layer 1: 4.1e-06; T_1, T_2: 1.2e-07, 9.1e-07; the
# basis case: 1.8e-06 at most).  Four times the larger figure, for the different summation order, for N_2 and H_2 of that
# case; FWD_ATOL for everything else, the basis case included.
BLOCK_D500_LAYER2_ATOL = 4 * 6.124e-05
V, R, E = 40, 5, 150


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def engine(native, c, **kw):
    return native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], keep_prob=c["keep"],
                         max_edges=max(len(c["triples"]), 1), skip=kw.pop("skip", "highway"), **kw)


def forward_by_phases(native, eng, c, train, masks=None, seed=0):
    """the phase API, reading N_l and T_l of every layer behind its rgcn_forward_layer_finish; returns (H, N, T)"""
    L = c["L"]
    eng.forward_begin(train=train, seed=seed, masks=masks)
    N, T = [None], [None]
    for l in range(1, L + 1):
        eng.forward_layer_partial(l)
        eng.forward_layer_finish(l)
        N.append(eng.read_buffer(native.BUF_HIGHWAY_INNER))
        T.append(eng.read_buffer(native.BUF_HIGHWAY_GATE))
    return [eng.activation(l) for l in range(L + 1)], N, T


def check_pass(native, eng, c, variant, tag, atol=lambda name, l: FWD_ATOL):
    """one forward + backward; variant 'explicit' (the case's masks), 'generated' (the engine's, read back) or 'eval'"""
    kind, Vc, L = c["kind"], c["V"], c["L"]
    train = variant != "eval"
    H, N, T = forward_by_phases(native, eng, c, train, masks=c["masks"] if variant == "explicit" else None, seed=991)
    masks = c["masks"] if variant == "explicit" else [eng.dropout_mask(l) for l in range(1, L + 1)] if train else None
    if variant == "generated":
        assert all(0.6 < m.mean() < 0.95 for m in masks)
    mode = "train" if train else "test"
    rH, rN, rT = hr.forward(kind, c["params"], c["triples"], Vc, L, mode=mode, keep=c["keep"], masks=masks)
    for l in range(1, L + 1):
        for name, got, ref in (("H", H[l], rH[l]), ("N", N[l], rN[l]), ("T", T[l], rT[l])):
            err = float(np.abs(got - ref).max())
            print("%s %s %s%d: max abs err %.3e (scale %.3e)" % (tag, variant, name, l, err, float(np.abs(ref).max())))
            assert err <= atol(name, l), (tag, variant, name, l, err)
        assert ((T[l] >= 0) & (T[l] <= 1)).all()      # (a saturated gate is exactly 0 or 1 in fp32, never beyond)
    np.testing.assert_array_equal(eng.codes(), H[L])
    eng.backward(c["dcodes"])
    grads = eng.get_grads()
    g64 = hr.backward(kind, c["params"], c["triples"], Vc, L, H, N, T, c["dcodes"], mode=mode, keep=c["keep"], masks=masks)
    for n in hr.weight_names(kind, L)[:-1]:
        assert_close(grads[n], g64[n], name="%s %s %s" % (tag, variant, n))
    return grads


SMALL = [("block", 2, 8, 2), ("block", 2, 8, 3), ("block", 2, 10, 2), ("basis", 3, 8, 2), ("basis", 3, 8, 3)]


@pytest.mark.parametrize("kind,nb,d,L", SMALL, ids=["%s-nb%d-d%d-L%d" % s for s in SMALL])
def test_parity_small_shapes(native, kind, nb, d, L):
    """the graph has a hub row past kLongRow; d = 10 takes the scalar path of every highway kernel; L = 3 has a middle
    layer with a highway layer above and below it (the D / dS / dZ ping-pong).  One engine per case, switched through
    both block forms and both arithmetic modes."""
    c = hr.make_case(V, R, d, L, kind, nb, lnr.extended_graph(V, R, E), seed=7 + d + L)
    with engine(native, c) as eng:
        assert eng.param_names == hr.weight_names(kind, L)
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        for fusion in ((1, 0) if kind == "block" else (1,)):
            eng.set_fusion(fusion)
            for gemm in (6, 0):
                eng.set_gemm_mode(gemm)
                for variant in ("explicit", "generated", "eval"):
                    check_pass(native, eng, c, variant, "%s d%d L%d fusion%d gemm%d" % (kind, d, L, fusion, gemm))


@pytest.mark.parametrize("kind,nb", [("block", 2), ("basis", 3)])
def test_empty_graph(native, kind, nb):
    c = hr.make_case(V, R, 8, 2, kind, nb, np.zeros((0, 3), np.int32), seed=2)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        grads = check_pass(native, eng, c, "explicit", kind + " empty")
    for n in grads:
        if n[:3] in ("W_f", "W_b", "C_f", "C_b"):
            assert not grads[n].any(), n
    assert np.abs(grads["W_highway1"]).max() > 0 and np.abs(grads["b_highway2"]).max() > 0


@pytest.mark.parametrize("kind,nb", [("block", 100), ("basis", 2)])
def test_parity_at_the_real_tile_shapes(native, kind, nb):
    """V = 257, d = 500: the GEMMs' real tiles and the 16-byte path with ragged tails (125 column vectors on 128 column
    lanes, 257 rows on 2 row lanes).  FWD_ATOL everywhere but N_2 and H_2 of the block case (BLOCK_D500_LAYER2_ATOL)."""
    Vb, Rb, d, L = 257, 5, 500, 2
    c = hr.make_case(Vb, Rb, d, L, kind, nb, lnr.extended_graph(Vb, Rb, 600), seed=31)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        check_pass(native, eng, c, "explicit", "%s d500" % kind,
                   atol=lambda name, l: BLOCK_D500_LAYER2_ATOL if (kind == "block" and l == 2 and name in "NH") else FWD_ATOL)


def test_two_backward_passes_are_bitwise_equal(native):
    c = hr.make_case(V, R, 8, 3, "block", 2, lnr.extended_graph(V, R, E), seed=5)
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
    """rgcn_step_device ends joined on a highway context (no deferred joins): two steps in a row give the same bytes, and
    the bytes of rgcn_forward + rgcn_backward with the same seed"""
    c = hr.make_case(V, R, 8, 2, "block", 2, lnr.extended_graph(V, R, E), seed=6)
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
def ref_case():
    """the basis case of tests/golden/reference_highway.npz"""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_highway.npz")) as z:
        fix = {k: z[k] for k in z.files}
    Vf, Rf, d, Ef, N, seed = (int(x) for x in fix["config"])
    nb, L = (int(x) for x in fix["basis_config"])
    names = hr.weight_names("basis", L)
    return {"V": Vf, "R": Rf, "d": d, "L": L, "kind": "basis", "nb": nb, "keep": 0.8, "triples": fix["triples"],
            "X": fix["X"], "Y": fix["Y"], "names": names, "seed": seed,
            "params": {n: fix["basis_weight%02d" % i] for i, n in enumerate(names)},
            "masks": [fix["basis_mask%d" % (l + 1)] for l in range(L)],
            "grads": {n: fix["basis_grad%02d" % i] for i, n in enumerate(names)},
            "loss": float(fix["basis_loss_train"]), "codes_train": fix["basis_codes_train"],
            "codes_test": fix["basis_codes_test"]}


def test_loss_and_gradients_of_the_reference_code(native, ref_case):
    """forward with the reference run's masks, the device decoder, the backward pass: the loss and every gradient the
    reference's own code gave.  Loss: test_gpu_train_step.py's 2e-5 x max(1, |loss|); gradients: its rel = 1e-3."""
    c = ref_case
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
    assert float(np.abs(codes - c["codes_train"]).max()) <= FWD_ATOL
    assert abs(loss - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"])), (loss, c["loss"])
    for n in c["names"]:
        assert_close(grads[n], c["grads"][n], rel=1e-3, name=n)
    for l in range(1, c["L"] + 1):
        assert np.abs(grads["W_highway%d" % l]).max() > 0 and np.abs(grads["b_highway%d" % l]).max() > 0


def test_one_train_step_with_clip_and_adam(native, ref_case):
    c = ref_case
    Vc, L, Ec, X, Y = c["V"], c["L"], len(c["triples"]), c["X"], c["Y"]
    names = [n for n in c["names"] if not (n[0] == "b" and n[1].isdigit())]      # (the layers' unused biases never move)
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
    rH, rN, rT = hr.forward("basis", c["params"], c["triples"], Vc, L, mode="train", masks=masks)
    with __import__("helpers").oracle_float64():
        oloss, odc, odw = oracle.distmult_loss_and_grads(rH[L], c["params"]["W_relation"].astype(np.float64), X, Y, 0.01)
    assert abs(loss - oloss) <= 2e-5 * max(1.0, abs(oloss)), (loss, oloss)
    og = hr.backward("basis", c["params"], c["triples"], Vc, L, rH, rN, rT, odc, mode="train", masks=masks)
    og["W_relation"] = odw
    for n in names:
        assert_close(grads[n], og[n], rel=1e-3, name="grad " + n)
    # the device update, replayed in numpy from the DEVICE gradients (test_gpu_train_step.py's bound for the same check)
    expect = adam_float64(c["params"], grads, names, 0.01, 0.9, 0.999, 1e-8, 1.0)
    for n in names:
        assert_close(new[n], expect[n], rel=2e-5, spike=2e-4, name="weight " + n)
        assert not np.array_equal(new[n], c["params"][n]), n
    for n in c["names"]:
        if n not in names:
            np.testing.assert_array_equal(new[n], c["params"][n])


def test_plugin_chain_from_the_settings_file(tmp_path, ref_case):
    from relationprediction_amd.common import model_builder
    c = ref_case
    triples = c["triples"]
    s, enc, dec = load_settings(tmp_path, highway_settings_text("basis", c["d"], c["nb"], c["L"]), V=c["V"], R=c["R"],
                                E=len(triples))
    encoder = model_builder.build_encoder(enc, triples)
    model = model_builder.build_decoder(encoder, dec)
    np.random.seed(c["seed"])
    model.preprocess(triples)
    model.register_for_test(triples)
    model.initialize_train()
    for var, val in zip(model.get_train_input_variables(), (triples, c["X"], c["Y"])):
        var.feed(val)
    test_codes = encoder.get_all_codes(mode='test')[0]
    rt = model.get_runtime()
    assert rt.highway and rt.engine.param_names == c["names"]
    for w, n in zip(model.get_weights(), c["names"]):
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)       # moved into the engine, bit for bit
    assert float(np.abs(test_codes - c["codes_test"]).max()) <= FWD_ATOL
    rt.engine.forward(train=True, masks=c["masks"])
    assert float(np.abs(rt.engine.codes() - c["codes_train"]).max()) <= FWD_ATOL
    # the eager surface: the gradient list follows get_weights()
    loss = model.get_loss('train') + model.get_regularization()
    grads = model.backward()
    assert np.isfinite(loss) and [g.shape for g in grads] == [w.shape for w in model.get_weights()]
    queries = triples[:12].astype(np.int32)
    for object_side in (True, False):
        known = known_lists(triples, object_side)
        ptr, idx = csr_for(queries, known, object_side)
        raw, filt = model.device_ranks(triples, queries, object_side, ptr, idx)
        assert (raw >= 1).all() and (raw <= c["V"]).all() and (filt >= 1).all() and (filt <= raw).all()


def test_refusals(native):
    args = (V, R, 8, 2)
    with pytest.raises(native.RgcnError) as e:
        native.Engine(*args, "block", 2, max_edges=10, world=2, rank=0, skip="highway")
    assert e.value.status == 5                                        # RGCN_ERR_UNSUPPORTED
    with pytest.raises(native.RgcnError) as e:
        native.Engine(*args, "basis", 3, max_edges=10, input_mode="onehot", skip="highway")
    assert e.value.status == 5
    with pytest.raises(native.RgcnError) as e:
        native.Engine(*args, "block", 2, max_edges=10, skip=7)
    assert e.value.status == 1                                        # RGCN_ERR_INVALID
    lib = native.load_library()
    cfg = native.Engine(*args, "block", 2, max_edges=10).cfg
    ctx = ctypes.c_void_p()
    for size in (0, 4, 16):
        ext = native.RgcnConfigExt(size, native.SKIP_HIGHWAY)
        assert lib.rgcn_create_ex(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(ctx)) == 1 and not ctx.value
    with native.Engine(*args, "block", 2, max_edges=10, skip="highway") as eng:
        with pytest.raises(native.RgcnError) as e:
            eng.capture_begin()
        assert e.value.status == 5 and "rgcn_capture_begin" in str(e.value)
    with native.Engine(*args, "block", 2, max_edges=10) as eng:        # not a highway context: no such buffers
        with pytest.raises(native.RgcnError) as e:
            eng.read_buffer(native.BUF_HIGHWAY_GATE)
        assert e.value.status == 4                                    # RGCN_ERR_STATE


def test_skip_none_through_create_ex_is_rgcn_create(native):
    import helpers
    params, triples, masks, dcodes = helpers.make_case(V, R, 8, 2, "block", 2, E, seed=4)
    runs = []
    for kw in ({}, {"create_ex": "null"}, {"create_ex": True}):
        with native.Engine(V, R, 8, 2, "block", 2, max_edges=E, skip="none", **kw) as eng:
            assert not any("highway" in n for n in eng.param_names)
            eng.set_params(params)
            eng.set_graph(triples)
            eng.forward(train=True, masks=masks)
            codes = eng.codes()
            eng.backward(dcodes)
            runs.append((codes, eng.get_grads()))
    for codes, grads in runs[1:]:
        assert np.array_equal(codes.view(np.uint32), runs[0][0].view(np.uint32))
        for n in grads:
            assert np.array_equal(grads[n].view(np.uint32), runs[0][1][n].view(np.uint32)), n
