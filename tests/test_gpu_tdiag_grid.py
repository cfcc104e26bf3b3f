"""Every compiled variant of the per-feature-coefficient layer's kernels (k_tdiag_rows, k_tdiag_dp, k_tdiag_dcoef,
k_tdiag_dh_join; csrc/basis_tdiag.hip) on the GPU, through the C ABI, at the cases of tests/tdiag_grid.py: every
(VEC, TPR) cell and dispatch boundary, the second lane trip, the long-row column loop beyond its first pass with a second
tile of basis functions on it, the coefficient gradient's and the dH epilogue's loops beyond their first trip, more long
rows than long-row workgroups, the 64 -> 512 workgroup / 48 -> 96 chunk switch, relations at the chunk boundaries, the
capped split of the weight-gradient GEMM, and the two caches that can go stale: the sigmoid table and dP's rows.

The reference is the float64 restatement of tests/times_diag_reference.py.  Bounds are the project's own: H_l and P_l
FWD_ATOL = 1e-4 absolute, gradients helpers.assert_close defaults against the float64 reverse mode at the engine's own
activations; the train steps' are tests/test_gpu_times_diag.py's.  tests/test_tdiag_grid.py shows on the CPU that a plain
float32 evaluation passes these very checks on these very inputs (forward within 5.2e-05 everywhere) -- but for H_1 of
tdiag_d129_B17 under local norms, whose bound tdiag_grid.LOCAL_D129_B17_H1_ATOL is four times float32's own 1.587e-04."""
import functools

import numpy as np
import pytest

import oracle
import tdiag_grid as tg
import times_diag_reference as tdr
from helpers import assert_close, oracle_float64
from test_gpu_featureless import adam_float64
from test_gpu_times_diag import engine, forward_by_phases
from test_gpu_train_step import decoder_batch
from test_times_diag_host import FWD_ATOL

pytestmark = pytest.mark.gpu

GRID_NAMES = [c["name"] for c in tg.TDIAG_GRID_LIST]
STRUCTURE_NAMES = list(tg.STRUCTURE_CASES)


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def _freeze(c):
    for a in [c["triples"], c["dcodes"]] + c["masks"] + list(c["params"].values()):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def inputs(name, L):
    """the case's weights, masks, upstream gradient and graph: made once, read by every test that runs the case"""
    return _freeze(tg.case_inputs(tg.ALL_CASES[name], L))


@functools.lru_cache(maxsize=None)
def reference(name, L, norm):
    """the float64 forward of the case with its own masks: (H, P), computed once"""
    c = inputs(name, L)
    H, P = tdr.forward(c["params"], c["triples"], c["V"], L, mode="train", keep=c["keep"], masks=c["masks"], norm=norm)
    for a in H + P[1:]:
        a.setflags(write=False)
    return H, P


def run_pass(native, eng, c, masks=None, seed=0):
    """forward by phases (P_l read behind every layer) + backward; (H, P, gradients) of the engine"""
    H, P = forward_by_phases(native, eng, c, True, masks=masks, seed=seed)
    eng.backward(c["dcodes"])
    return H, P, eng.get_grads()


def assert_forward(c, norm, H, P, ref, tag=""):
    rH, rP = ref
    for l in range(1, c["L"] + 1):
        assert P[l].shape == (2, c["V"], c["nb"] * c["d"])
        for buf, got, want in (("H", H[l], rH[l]), ("P", P[l], rP[l])):
            err = float(np.abs(got - want).max())
            print("%s%s %s L%d %s%d: max abs err %.3e (scale %.3e)" % (tag, c["name"], norm, c["L"], buf, l, err,
                                                                      float(np.abs(want).max())))
            assert err <= tg.forward_atol(c["name"], norm, c["L"], buf, l, FWD_ATOL), (c["name"], norm, buf, l, err)


def assert_gradients(c, norm, H, grads, masks=None, tag=""):
    g64 = tdr.backward(c["params"], c["triples"], c["V"], c["L"], H, c["dcodes"], mode="train", keep=c["keep"],
                       masks=c["masks"] if masks is None else masks, norm=norm)
    names = tdr.weight_names(c["L"])[:-1]
    assert set(g64) == set(names)
    for n in names:      # both weight tensors, both coefficient sets, W_self and the bias per layer, W_emb and b_emb
        assert_close(grads[n], g64[n], name="%s%s %s %s" % (tag, c["name"], norm, n))


# ----------------------------------------------------------------------------- every case, intended norms, two layers
@pytest.mark.parametrize("name", GRID_NAMES + STRUCTURE_NAMES)
def test_case_equals_the_float64_restatement(native, name):
    c = inputs(name, 2)
    with engine(native, c) as eng:
        assert eng.param_names == tdr.weight_names(2)
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, P, grads = run_pass(native, eng, c, masks=c["masks"])
    assert_forward(c, "intended", H, P, reference(name, 2, "intended"))
    assert_gradients(c, "intended", H, grads)
    if name == "chunk_edges":                   # relation 2 has no edge: no chunk, and the reduction writes zeros
        for l in (1, 2):
            assert not grads["C_f%d" % l][2].any() and not grads["C_b%d" % l][2].any()
            assert grads["C_f%d" % l][3].any() and grads["C_b%d" % l][3].any()       # ... and relation 3's one message arrives


# ----------------------------------------------------------------------------- every width case, local norms, one layer
@pytest.mark.parametrize("name", GRID_NAMES)
def test_case_as_the_top_layer_under_local_norms(native, name):
    """L = 1: the layer is the top layer, its epilogue runs without relu on short and long rows alike.  With R = 237
    nearly every (relation, vertex) run has length 1, so the 400-slot hub's sum is not damped (tdiag_grid.py)."""
    c = inputs(name, 1)
    with engine(native, c, norm_mode="local") as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, P, grads = run_pass(native, eng, c, masks=c["masks"])
    assert (H[1][:4] < 0).any(axis=1).all()                            # the hub rows, short and long, are not rectified
    assert_forward(c, "local", H, P, reference(name, 1, "local"))
    assert_gradients(c, "local", H, grads)


# ----------------------------------------------------------------------------- generated dropout at the widest cases
@pytest.mark.parametrize("vec", tg.VECS)
def test_generated_dropout_is_what_the_forward_used_on_the_second_lane_trip(native, vec):
    """drop_factor's index off + k at the largest offsets (V d = 308,400 at d = 1028) and on the second lane trip"""
    c = inputs(tg.WIDEST[vec], 2)
    assert tg.vec_tpr(c["d"])[0] == vec and tg.lane_trips(c["d"]) == 2
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, P = forward_by_phases(native, eng, c, True, seed=4321 + vec)
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
    for m in masks:
        assert m.shape == (c["V"], c["d"]) and set(np.unique(m)) == {0, 1}
        assert 0.78 < m.mean() < 0.82
        tail = m[:, 256 * vec:]                                        # the columns of the second lane trip
        assert tail.shape[1] >= 4 and 0.7 < tail.mean() < 0.9
    ref = tdr.forward(c["params"], c["triples"], c["V"], c["L"], mode="train", keep=c["keep"], masks=masks)
    assert_forward(c, "intended", H, P, ref, tag="generated dropout ")


# ----------------------------------------------------------------------------- a stale sigmoid table
def test_other_coefficients_rebuild_the_sigmoid_table(native):
    """the table G = sigmoid(C) is rebuilt when the weights' version moves: set_params, forward, set_params with other C
    only, forward -- the second pass is the float64 forward of the second weights"""
    c = inputs(tg.STALE_TABLE, 2)
    second = dict(c, params=tg.second_coefficients(c["params"], c["L"]))
    changed = [n for n in c["params"] if not np.array_equal(c["params"][n], second["params"][n])]
    assert sorted(changed) == ["C_b1", "C_b2", "C_f1", "C_f2"]
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, P, grads = run_pass(native, eng, c, masks=c["masks"])
        assert_forward(c, "intended", H, P, reference(tg.STALE_TABLE, 2, "intended"), tag="first weights ")
        eng.set_params(second["params"])
        H, P, grads = run_pass(native, eng, second, masks=c["masks"])
    ref = tdr.forward(second["params"], c["triples"], c["V"], c["L"], mode="train", keep=c["keep"], masks=c["masks"])
    assert float(np.abs(ref[0][2] - reference(tg.STALE_TABLE, 2, "intended")[0][2]).max()) > 100 * FWD_ATOL
    assert_forward(second, "intended", H, P, ref, tag="second weights ")
    assert_gradients(second, "intended", H, grads, tag="second weights ")


def test_the_second_train_step_sees_the_coefficients_the_first_one_wrote(native):
    """two rgcn_train_step_device calls with clip and Adam: the second step's loss and gradients are the float64 ones of
    the weights read back after the first (tests/test_gpu_times_diag.py's train-step bounds)"""
    c = inputs(tg.STALE_TABLE, 2)
    V, L, E = c["V"], c["L"], len(c["triples"])
    X, Y = decoder_batch(np.random.RandomState(2), c["triples"][:500], V)
    names = tdr.weight_names(L)
    steps = []
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(X))
        eng.optimizer_config(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0)
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(X), eng.to_device(Y)
        before = c["params"]
        for step in range(2):
            eng.train_step_device(td, E, xd, yd, len(X), seed=500 + step, reg_param=0.01)
            steps.append(dict(before=before, loss=eng.loss(), masks=[eng.dropout_mask(l) for l in range(1, L + 1)],
                              grads=eng.get_grads(), after=eng.get_params()))
            before = steps[-1]["after"]
        for b in (td, xd, yd):
            b.free()
    for k, s in enumerate(steps):
        p = s["before"]
        rH, _ = tdr.forward(p, c["triples"], V, L, mode="train", masks=s["masks"])
        with oracle_float64():
            oloss, odc, odw = oracle.distmult_loss_and_grads(rH[L], p["W_relation"].astype(np.float64), X, Y, 0.01)
        print("step %d: loss %.6f, float64 %.6f" % (k + 1, s["loss"], oloss))
        assert abs(s["loss"] - oloss) <= 2e-5 * max(1.0, abs(oloss)), (k, s["loss"], oloss)
        g64 = tdr.backward(p, c["triples"], V, L, rH, odc, mode="train", masks=s["masks"])
        g64["W_relation"] = odw
        for n in names:
            assert_close(s["grads"][n], g64[n], rel=1e-3, name="step %d grad %s" % (k + 1, n))
            assert not np.array_equal(s["after"][n], p[n]), (k, n)
    # the first update, replayed in numpy from the device gradients; the coefficients moved by about the learning rate
    expect = adam_float64(c["params"], steps[0]["grads"], names, 0.01, 0.9, 0.999, 1e-8, 1.0)
    for n in names:
        assert_close(steps[0]["after"][n], expect[n], rel=2e-5, spike=2e-4, name="weight " + n)
    assert float(np.abs(steps[0]["after"]["C_f1"] - c["params"]["C_f1"]).max()) > 5e-3


# ----------------------------------------------------------------------------- stale dP rows
def test_rows_of_vertices_that_stopped_sending_are_zero_in_every_launch_of_dp(native):
    """B = 17: three launches of k_tdiag_dp.  Vertices that sent in both directions (long rows and short ones) appear in
    no edge of the next graph: dW_dir = H^T dP_dir reads their rows of dP all the same, and every gradient is the
    float64 one of the second graph."""
    c, second, quiet = tg.stale_case()
    _freeze(c)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H1, P1, g1 = run_pass(native, eng, c, masks=c["masks"])
        eng.set_graph(second)
        H, P, g2 = run_pass(native, eng, c, masks=c["masks"])
    assert_gradients(c, "intended", H1, g1, tag="first graph ")
    c2 = dict(c, triples=second)
    ref = tdr.forward(c["params"], second, c["V"], c["L"], mode="train", keep=c["keep"], masks=c["masks"])
    assert_forward(c2, "intended", H, P, ref, tag="second graph ")
    assert_gradients(c2, "intended", H, g2, tag="second graph ")
    for n in ("W_f1", "W_b1", "W_f2", "W_b2"):
        assert not np.array_equal(g1[n], g2[n]), n


# ----------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["many_long_rows", tg.THREE_PASSES])
def test_two_identical_steps_give_the_same_bytes(native, name):
    c = inputs(name, 2)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        td, dd = eng.to_device(c["triples"]), eng.to_device(c["dcodes"])
        runs = []
        for _ in range(2):
            eng.step_device(td, len(c["triples"]), dd, train=True, seed=77)
            runs.append((eng.get_grads(), [eng.activation(l) for l in range(1, c["L"] + 1)]))
        td.free(); dd.free()
    for n in tdr.weight_names(c["L"])[:-1]:
        assert np.array_equal(runs[0][0][n].view(np.uint32), runs[1][0][n].view(np.uint32)), n
        assert runs[0][0][n].any(), n
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------- the dH epilogue's second trip
@pytest.mark.parametrize("name", list(tg.LARGE_CASES))
def test_large_case_equals_the_float64_restatement(native, name):
    """V d / VEC past 8192 x 256: the grid-stride loop of k_tdiag_dh_join takes a second trip; at d = 257 the weight
    gradient's split over V is capped at the context's 16 slabs as well (tests/test_tdiag_grid.py checks both figures)"""
    case = tg.LARGE_CASES[name]
    c = inputs(name, case["L"])
    assert tg.join_trips(c["V"], c["d"]) == 2
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, P, grads = run_pass(native, eng, c, masks=c["masks"])
    assert_forward(c, "intended", H, P, reference(name, case["L"], "intended"))
    assert_gradients(c, "intended", H, grads)
    tail = grads["W_emb"][c["V"] - 90:]         # the rows of the second trip: V d / VEC - 2,097,152 vectors
    assert tail.any() and np.abs(grads["W_emb"]).max() > 0
