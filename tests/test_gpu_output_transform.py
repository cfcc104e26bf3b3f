"""The encoder's output transform (rgcn_config_ext::code_dim, csrc/output_transform.hip) on the GPU, through the C ABI,
against the float64 restatement of tests/output_transform_reference.py.  Bounds are the project's own: activations and
codes FWD_ATOL absolute against the float64 forward, gradients helpers.assert_close defaults against the float64 reverse
mode evaluated at the engine's own activations (its own relu gates); the train step's are test_gpu_train_step.py's."""
import ctypes

import numpy as np
import pytest

import oracle
import local_norm_reference as lnr
import output_transform_reference as otr
from helpers import assert_close, oracle_float64
from relation_query_reference import known_relation_lists, relation_ranks_from_energies
from test_gpu_eval import csr_for
from test_gpu_topk import assert_rows_equal_reference, csr, exclusion_lists, known_lists
from test_gpu_train_step import decoder_batch, numpy_clip_adam

pytestmark = pytest.mark.gpu

FWD_ATOL = 1e-4            # test_gpu_highway.py's and test_gpu_parity.py's bound
V, R, E = 40, 5, 150
INVALID, STATE, UNSUPPORTED = 1, 4, 5


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def engine(native, c, **kw):
    return native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], keep_prob=c["keep"],
                         max_edges=max(len(c["triples"]), 1), code_dim=c["c"], **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ================================================================== 1. parity, basis and block
def check_pass(native, eng, c, variant, tag, codes_atol=FWD_ATOL, backward=True):
    """one forward + backward; variant 'explicit' (the case's masks), 'generated' (the engine's, read back) or 'eval'"""
    kind, Vc, L = c["kind"], c["V"], c["L"]
    train = variant != "eval"
    eng.forward(train=train, seed=991, masks=c["masks"] if variant == "explicit" else None)
    masks = c["masks"] if variant == "explicit" else [eng.dropout_mask(l) for l in range(1, L + 1)] if train else None
    if variant == "generated":
        assert all(0.6 < m.mean() < 0.95 for m in masks)
    mode = "train" if train else "test"
    H = [eng.activation(l) for l in range(L + 1)]
    codes = eng.codes()
    assert codes.shape == (Vc, c["c"]) and H[L].shape == (Vc, c["d"])
    rH, rcodes = otr.forward(kind, c["params"], c["triples"], Vc, L, mode=mode, keep=c["keep"], masks=masks)
    for l in range(L + 1):
        err = float(np.abs(H[l] - rH[l]).max())
        print("%s %s H%d: max abs err %.3e (scale %.3e)" % (tag, variant, l, err, float(np.abs(rH[l]).max())))
        assert err <= FWD_ATOL, (tag, variant, l, err)
    err = float(np.abs(codes - rcodes).max())
    print("%s %s codes: max abs err %.3e (scale %.3e)" % (tag, variant, err, float(np.abs(rcodes).max())))
    assert err <= codes_atol, (tag, variant, "codes", err)
    if not backward:
        return None
    eng.backward(c["dcodes"])
    grads = eng.get_grads()
    g64 = otr.backward(kind, c["params"], c["triples"], Vc, L, H, c["dcodes"], mode=mode, keep=c["keep"], masks=masks)
    for n in otr.weight_names(kind, L)[:-1]:
        assert_close(grads[n], g64[n], name="%s %s %s" % (tag, variant, n))
    assert np.abs(grads["W_out"]).max() > 0 and np.abs(grads["b_out"]).max() > 0
    return grads


SMALL = [("basis", 3, 8, 8, 2), ("basis", 3, 8, 4, 2), ("basis", 3, 8, 12, 2), ("basis", 3, 10, 6, 2), ("basis", 3, 12, 7, 1),
         ("block", 2, 8, 4, 2), ("block", 2, 10, 6, 3)]


@pytest.mark.parametrize("kind,nb,d,c,L", SMALL, ids=["%s-nb%d-d%d-c%d-L%d" % s for s in SMALL])
def test_parity_small_shapes(native, kind, nb, d, c, L):
    """the graph has a hub row past kLongRow; d 10 -> c 6 takes the scalar path on both widths, c = 7 is odd, c = d keeps
    the layer.  One engine per case, switched through both block forms and both arithmetic modes."""
    case = otr.make_case(V, R, d, c, L, kind, nb, lnr.extended_graph(V, R, E), seed=11 + d + c + L)
    with engine(native, case) as eng:
        assert eng.param_names == otr.weight_names(kind, L)
        assert eng.param_shapes[-3:] == [(d, c), (c,), (V, c)]
        eng.set_params(case["params"])
        eng.set_graph(case["triples"])
        for fusion in ((1, 0) if kind == "block" else (1,)):
            eng.set_fusion(fusion)
            for gemm in (6, 0):
                eng.set_gemm_mode(gemm)
                for variant in ("explicit", "generated", "eval"):
                    check_pass(native, eng, case, variant, "%s d%d c%d L%d fusion%d gemm%d" % (kind, d, c, L, fusion, gemm))


# ================================================================== 2. the stack cannot tell
STACKS = [("basis", dict(kind="basis", nb=3), 8, 4), ("block", dict(kind="block", nb=2), 10, 6),
          ("times-diag", dict(kind="basis_tdiag", nb=3), 8, 4), ("plus-diag", dict(kind="basis_pdiag", nb=3), 8, 4),
          ("one-hot", dict(kind="basis", nb=3, input_mode="onehot"), 8, 4),
          ("highway", dict(kind="basis", nb=3, skip="highway"), 8, 4)]


@pytest.mark.parametrize("name,cfg,d,c", STACKS, ids=[s[0] for s in STACKS])
def test_the_stack_cannot_tell(native, name, cfg, d, c):
    """two engines with the same stack parameters, masks and graph, one with the layer: (a) H_L is bitwise equal; (b) the
    layer's outputs against the float64 layer at the engine's own H_L; (c) the second engine, fed the first one's
    RGCN_BUF_OUT_DH as its dcodes, returns every stack gradient bit for bit"""
    L = 2
    cfg = dict(cfg)
    kind, nb = cfg.pop("kind"), cfg.pop("nb")
    triples = lnr.extended_graph(V, R, E)
    rng = np.random.RandomState(5 + d)
    masks = [(rng.rand(V, d) < 0.8).astype(np.uint8) for _ in range(L)]
    dcodes = (rng.randn(V, c) * 1e-1).astype(np.float32)
    with native.Engine(V, R, d, L, kind, nb, max_edges=E, code_dim=c, **cfg) as a, \
            native.Engine(V, R, d, L, kind, nb, max_edges=E, **cfg) as b:
        assert [n for n in a.param_names if n not in ("W_out", "b_out")] == b.param_names
        params = {n: (rng.randn(*s) * 0.3).astype(np.float32) for n, s in zip(a.param_names, a.param_shapes)}
        a.set_params(params)
        stack = [n for n in b.param_names if n != "W_relation"]
        for n in stack:
            b.set_param(n, params[n])
        for e in (a, b):
            e.set_graph(triples)
            e.forward(train=True, masks=masks)
        H_L = a.activation(L)
        assert np.array_equal(bits(H_L), bits(b.activation(L)))                      # (a)
        assert np.array_equal(bits(b.codes()), bits(H_L))
        a.backward(dcodes)
        out_dh = a.read_buffer(native.BUF_OUT_DH)
        ga = a.get_grads()
        D_L, gW, gb = otr.layer_backward(H_L, params["W_out"], dcodes)                # (b)
        assert float(np.abs(a.codes() - otr.layer_forward(H_L, params["W_out"], params["b_out"])).max()) <= 1e-4
        assert float(np.abs(out_dh - D_L).max()) <= 1e-4
        assert_close(ga["W_out"], gW, name=name + " W_out")
        assert_close(ga["b_out"], gb, name=name + " b_out")
        b.backward(out_dh)                                                            # (c)
        gb_ = b.get_grads()
    for n in stack:
        assert np.array_equal(bits(ga[n]), bits(gb_[n])), (name, n)
    assert any(np.abs(ga[n]).max() > 0 for n in stack)


# ================================================================== 3. real tiles
# Measured on the CPU on each case's own inputs: output_transform_reference.forward_float32 (numpy float32, one summation
# order) against its float64 forward differs in the codes by at most
#   case 1 (V 257, d 500 -> c 200, basis B 2, L 2):  7.046e-06 (train mode; codes reach 1.2e+01)
#   case 2 (V 10113, d 64 -> c 300, one layer):      9.281e-07 (test mode; train mode 6.092e-07; codes reach 2.3e+00)
# Four times either figure, for the other summation order, is below FWD_ATOL: FWD_ATOL is the bound of both.
TILE_CODES_ATOL = max(FWD_ATOL, 4 * 7.046e-06, 4 * 9.281e-07)


def test_real_tiles_ragged_n_and_k(native):
    """V 257, d 500 -> c 200: N = 200 is ragged in the 128-wide tile, K = 500 is no multiple of 16 (nor is 200, the depth
    of dcodes . W_out^T), 257 rows leave the vector path of the bias pass a tail workgroup"""
    case = otr.make_case(257, 5, 500, 200, 2, "basis", 2, lnr.extended_graph(257, 5, 600), seed=31)
    with engine(native, case) as eng:
        eng.set_params(case["params"])
        eng.set_graph(case["triples"])
        check_pass(native, eng, case, "explicit", "d500 c200", codes_atol=TILE_CODES_ATOL)


def test_real_tiles_eight_wavefront_kernel_forward(native):
    """V 10113, d 64 -> c 300, one layer, forward only: 80 x 2 = 160 tiles, the smallest launch gemm_plan sends to the
    eight-wavefront kernel; N = 300 is ragged in its 256-wide tile"""
    case = otr.make_case(10113, 5, 64, 300, 1, "basis", 2, lnr.extended_graph(10113, 5, 600), seed=32)
    with engine(native, case) as eng:
        eng.set_params(case["params"])
        eng.set_graph(case["triples"])
        check_pass(native, eng, case, "explicit", "d64 c300", codes_atol=TILE_CODES_ATOL, backward=False)
        check_pass(native, eng, case, "eval", "d64 c300", codes_atol=TILE_CODES_ATOL, backward=False)


# ================================================================== 4. consumers at c != d
WIDTHS = [(10, 6), (8, 12)]


@pytest.mark.parametrize("d,c", WIDTHS)
def test_train_step_device_with_clip_and_adam(native, d, c):
    """two rgcn_train_step_device steps; the loss, every gradient and the updated parameters against float64 at the bounds
    of test_gpu_train_step.py::test_train_step_device_with_clip_and_adam (5e-5 x max(1, |loss|); rel 1e-3; rel 2e-5 with
    spike 2e-4 -- literals inside that test, hence repeated here; its helpers are imported)"""
    L, kind, nb = 2, "basis", 3
    case = otr.make_case(V, R, d, c, L, kind, nb, lnr.extended_graph(V, R, E), seed=40 + d)
    triples = case["triples"]
    X, Y = decoder_batch(np.random.RandomState(2), triples, V)
    names = [n for n in otr.weight_names(kind, L) if not (n[0] == "b" and n[1].isdigit())]      # (the layers' unused biases)
    with engine(native, case) as eng:
        eng.set_params(case["params"])
        eng.decoder_reserve(len(X))
        eng.optimizer_config(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0)
        td, xd, yd = eng.to_device(triples), eng.to_device(X), eng.to_device(Y)
        state = {}
        cur = {k: v.copy() for k, v in case["params"].items()}
        for step in range(2):
            eng.train_step_device(td, len(triples), xd, yd, len(X), seed=500 + step, reg_param=0.01)
            loss = eng.loss()
            masks = [eng.dropout_mask(l) for l in range(1, L + 1)]
            grads = eng.get_grads()
            assert eng.dcodes().shape == (V, c)
            new = eng.get_params()
            rH, rcodes = otr.forward(kind, cur, triples, V, L, mode="train", masks=masks)
            with oracle_float64():
                oloss, odc, odw = oracle.distmult_loss_and_grads(rcodes, cur["W_relation"].astype(np.float64), X, Y, 0.01)
            assert abs(loss - oloss) <= 5e-5 * max(1.0, abs(oloss)), (step, loss, oloss)
            og = otr.backward(kind, cur, triples, V, L, rH, odc, mode="train", masks=masks)
            og["W_relation"] = odw
            for n in names:
                assert_close(grads[n], og[n], rel=1e-3, name="step %d grad %s" % (step, n))
            expect, _ = numpy_clip_adam(cur, grads, names, 0.01, 0.9, 0.999, 1e-8, 1.0, state)
            for n in names:
                assert_close(new[n], expect[n], rel=2e-5, spike=2e-4, name="step %d weight %s" % (step, n))
                assert not np.array_equal(new[n], cur[n]), n
            for n in eng.param_names:
                if n not in names:
                    np.testing.assert_array_equal(new[n], cur[n])
            cur = new
        for b in (td, xd, yd):
            b.free()


@pytest.fixture(scope="module", params=WIDTHS, ids=["d%d-c%d" % w for w in WIDTHS])
def scored(native, request):
    """an engine after a test-mode forward, its codes and W_relation [V, c]"""
    d, c = request.param
    case = otr.make_case(V, R, d, c, 2, "basis", 3, lnr.extended_graph(V, R, E), seed=50 + d)
    eng = engine(native, case)
    eng.set_params(case["params"])
    eng.set_graph(case["triples"])
    eng.forward(train=False)
    eng.rank_reserve(64)
    queries = case["triples"][np.random.RandomState(4).choice(len(case["triples"]), 60, replace=False)].copy()
    yield eng, case, eng.codes(), queries
    eng.close()


def test_entity_ranks_and_topk_at_the_code_width(native, scored):
    eng, case, codes, queries = scored
    w_rel = case["params"]["W_relation"]
    assert codes.shape[1] == case["c"] == w_rel.shape[1]
    for object_side in (True, False):
        known = known_lists(case["triples"], object_side)
        ptr, idx = csr_for(queries, known, object_side)
        raw, filt = eng.ranks(queries, object_side, ptr, idx)
        oraw, ofilt = oracle.distmult_ranks(codes, w_rel, queries, object_side, known)
        # (as test_gpu_eval.py: two fp32 products with different summation orders may flip a near-tie by one)
        assert np.mean(raw != oraw) <= 0.02 and np.abs(raw - oraw).max() <= 1
        assert np.mean(filt != ofilt) <= 0.02 and np.abs(filt - ofilt).max() <= 1
        lists = exclusion_lists(queries, case["triples"], object_side, V, np.random.RandomState(9))
        eptr, eidx = csr(lists)
        ids, energy = eng.topk(queries, object_side, 3, eptr, eidx)
        energies = eng.read_buffer(native.BUF_RANK_ENERGIES)[:len(queries)]
        assert_rows_equal_reference(energies, ids, energy, 3, lists, ("entity", object_side))      # (test_gpu_topk.py: bit exact)
        q = codes[queries[:, 0 if object_side else 2]] * w_rel[queries[:, 1]]
        want = q.astype(np.float64) @ codes.astype(np.float64).T
        assert float(np.abs(energies - want).max()) <= 1e-4 * max(1.0, float(np.abs(want).max()))


def test_relation_ranks_and_topk_at_the_code_width(native, scored):
    """test_gpu_relation_queries.py's treatment: ranks and selection bit exact on the device's own energies, the energies
    within the float64 dot-product bound"""
    from relation_query_reference import float64_relation_energies
    eng, case, codes, queries = scored
    w_rel = case["params"]["W_relation"]
    known = known_relation_lists(case["triples"])
    lists = [list(known[(int(s), int(o))]) for s, r, o in queries]
    ptr, flat = csr(lists)
    raw, filt = eng.ranks_relation(queries, ptr, flat)
    energies = eng.read_buffer(native.BUF_RELATION_ENERGIES)[:len(queries)]
    want_raw, want_filt = relation_ranks_from_energies(energies, queries[:, 1], lists)
    assert np.array_equal(raw, want_raw) and np.array_equal(filt, want_filt)
    E64, bound = float64_relation_energies(codes, w_rel, queries, R)
    assert (np.abs(energies.astype(np.float64) - E64) <= bound).all()
    excl = [lst if i % 3 else [] for i, lst in enumerate(lists)]
    eptr, eflat = csr(excl)
    ids, energy = eng.topk_relation(queries, 3, eptr, eflat)
    energies = eng.read_buffer(native.BUF_RELATION_ENERGIES)[:len(queries)]
    assert_rows_equal_reference(energies, ids, energy, 3, excl, "relation")


# ================================================================== 5. ABI edges
def plain_case(d=8, L=2, kind="block", nb=2):
    import helpers
    params, triples, masks, dcodes = helpers.make_case(V, R, d, L, kind, nb, E, seed=4)
    return params, triples, masks, dcodes


@pytest.mark.parametrize("kw", [dict(code_dim=0), dict(ext_struct_size=8), dict(ext_struct_size=8, code_dim=4)],
                         ids=["code_dim-0", "struct_size-8", "struct_size-8-ignores-code_dim"])
def test_no_layer_is_todays_context(native, kw):
    """code_dim 0, and the extension struct of the earlier layout (struct_size 8, whose code_dim is not read): today's
    parameter list, [V,d] codes, and the bytes of rgcn_create"""
    params, triples, masks, dcodes = plain_case()
    runs = []
    for k in ({}, kw):
        with native.Engine(V, R, 8, 2, "block", 2, max_edges=E, **k) as eng:
            assert eng.param_names == oracle.weight_names("block", 2) and eng.dc == eng.d == 8
            assert eng.param_shapes[-1] == (V, 8)
            eng.set_params(params)
            eng.set_graph(triples)
            eng.forward(train=True, masks=masks)
            codes = eng.codes()
            assert codes.shape == (V, 8) and np.array_equal(bits(codes), bits(eng.activation(2)))
            eng.backward(dcodes)
            runs.append((codes, eng.get_grads()))
            with pytest.raises(native.RgcnError) as e:
                eng.read_buffer(native.BUF_OUT_DH)
            assert e.value.status == STATE
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0]))
    for n in runs[0][1]:
        assert np.array_equal(bits(runs[0][1][n]), bits(runs[1][1][n])), n


def test_wrong_counts_states_and_refusals(native):
    lib = native.load_library()
    case = otr.make_case(V, R, 8, 4, 2, "block", 2, lnr.extended_graph(V, R, E), seed=3)
    with engine(native, case) as eng:
        eng.set_params(case["params"])
        eng.set_graph(case["triples"])
        eng.forward(train=True, masks=case["masks"])
        with pytest.raises(native.RgcnError) as e:                     # no backward pass yet
            eng.read_buffer(native.BUF_OUT_DH)
        assert e.value.status == STATE
        for count in (V * 8, V * 4 - 1, 0):                            # [V,d] is the wrong size now
            buf = np.zeros(V * 8, dtype=np.float32)
            assert lib.rgcn_get_codes(eng.ctx, buf.ctypes.data_as(ctypes.c_void_p), count) == INVALID
            assert lib.rgcn_backward(eng.ctx, buf.ctypes.data_as(ctypes.c_void_p), count) == INVALID
        assert eng.activation(2).shape == (V, 8)                       # rgcn_get_activation(L) stays H_L [V,d]
        eng.backward(case["dcodes"])
        assert eng.read_buffer(native.BUF_OUT_DH).shape == (V, 8)
        with pytest.raises(native.RgcnError) as e:
            eng.capture_begin()
        assert e.value.status == UNSUPPORTED and "rgcn_capture_begin" in str(e.value)
    args = (V, R, 8, 2)
    for kw, status, word in ((dict(kind="block", num_bases=2, code_dim=-1), INVALID, "code_dim"),
                             (dict(kind="block", num_bases=2, code_dim=4, world=2, rank=0), UNSUPPORTED, "sharded"),
                             (dict(kind="embedding", num_bases=1, code_dim=4), UNSUPPORTED, "EMBEDDING")):
        a = (V, R, 8, 0) if kw["kind"] == "embedding" else args
        with pytest.raises(native.RgcnError) as e:
            native.Engine(*a, max_edges=10, **kw)
        assert e.value.status == status and word in str(e.value), str(e.value)
    cfg = native.Engine(*args, "block", 2, max_edges=10).cfg
    ctx = ctypes.c_void_p()
    for size in (0, 4, 16):
        ext = native.RgcnConfigExt(size, native.SKIP_NONE, 4)
        assert lib.rgcn_create_ex(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(ctx)) == INVALID and not ctx.value


def test_two_backward_passes_are_bitwise_equal(native):
    case = otr.make_case(V, R, 8, 4, 3, "block", 2, lnr.extended_graph(V, R, E), seed=5)
    with engine(native, case) as eng:
        eng.set_params(case["params"])
        eng.set_graph(case["triples"])
        runs = []
        for _ in range(2):
            eng.forward(train=True, masks=case["masks"])
            eng.backward(case["dcodes"])
            runs.append(dict(eng.get_grads(), out_dh=eng.read_buffer(native.BUF_OUT_DH)))
    for n in runs[0]:
        assert np.array_equal(bits(runs[0][n]), bits(runs[1][n])), n


@pytest.mark.parametrize("kind,nb", [("block", 2), ("basis", 3)])
def test_empty_graph(native, kind, nb):
    case = otr.make_case(V, R, 8, 4, 2, kind, nb, np.zeros((0, 3), np.int32), seed=2)
    with engine(native, case) as eng:
        eng.set_params(case["params"])
        eng.set_graph(case["triples"])
        grads = check_pass(native, eng, case, "explicit", kind + " empty")
    for n in grads:
        if n[:3] in ("W_f", "W_b", "C_f", "C_b"):
            assert not grads[n].any(), n
    assert np.abs(grads["W_out"]).max() > 0 and np.abs(grads["b_out"]).max() > 0
