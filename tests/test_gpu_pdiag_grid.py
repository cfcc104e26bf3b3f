"""Every compiled variant of the per-relation-diagonal layer's kernels (k_pdiag_rows, k_pdiag_epilogue, k_pdiag_row_bwd,
k_pdiag_dcoef, k_pdiag_ddiag, k_pdiag_dh_join; csrc/basis_pdiag.hip) on the GPU, through the C ABI, at the cases of
tests/pdiag_grid.py: every (VEC, TPR) cell and dispatch boundary, the second lane trip, the long-row column loop beyond
its first pass, the mixing scalars at 2 B = 64, 66 and 128, the wave-per-row kernels' and the diagonal gradient's loops
beyond their first trip, more long rows than long-row workgroups, the 64 -> 512 workgroup / 48 -> 96 chunk switch and
relations at the chunk boundaries.

The reference is the float64 restatement of tests/add_diagonal_reference.py.  Bounds are tests/test_gpu_add_diagonal.py's:
H_l, a_l and the diagonal aggregate FWD_ATOL x max(1, largest |float64 value| of that tensor), gradients
helpers.assert_close defaults against the float64 reverse mode at the engine's own activations.  tests/test_pdiag_grid.py
shows on the CPU that a plain float32 evaluation passes these very checks on these very inputs."""
import functools

import numpy as np
import pytest

import add_diagonal_reference as adr
import pdiag_grid as pg
from helpers import assert_close
from test_add_diagonal_host import fwd_bound
from test_gpu_add_diagonal import engine, forward_by_phases

pytestmark = pytest.mark.gpu

GRID_NAMES = [c["name"] for c in pg.PDIAG_GRID_LIST]
STRUCTURE_NAMES = list(pg.STRUCTURE_CASES)


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
    return _freeze(pg.case_inputs(pg.ALL_CASES[name], L))


@functools.lru_cache(maxsize=None)
def reference(name, L, norm):
    """the float64 forward of the case with its own masks: (H, a, aggregate), computed once"""
    c = inputs(name, L)
    ref = adr.forward(c["params"], c["triples"], c["V"], L, mode="train", keep=c["keep"], masks=c["masks"], norm=norm)
    for q in ref:
        for a in q:
            if a is not None:
                a.setflags(write=False)
    return ref


def run_pass(native, eng, c, masks=None, seed=0):
    """forward by phases (a_l and the aggregate read behind every layer) + backward"""
    H, A, G = forward_by_phases(native, eng, c, True, masks=masks, seed=seed)
    eng.backward(c["dcodes"])
    return H, A, G, eng.get_grads()


def assert_forward(c, norm, H, A, G, ref, tag=""):
    rH, rA, rG = ref
    for l in range(1, c["L"] + 1):
        assert A[l].shape == (2, c["V"], c["nb"]) and G[l].shape == (c["V"], c["d"])
        for buf, got, want in (("H", H[l], rH[l]), ("a", A[l], rA[l]), ("agg", G[l], rG[l])):
            err = float(np.abs(got - want).max())
            print("%s%s %s L%d %s%d: max abs err %.3e (scale %.3e)" % (tag, c["name"], norm, c["L"], buf, l, err,
                                                                      float(np.abs(want).max())))
            assert err <= fwd_bound(want), (c["name"], norm, buf, l, err)


def assert_gradients(c, norm, H, grads, masks=None, tag=""):
    g64 = adr.backward(c["params"], c["triples"], c["V"], c["L"], H, c["dcodes"], mode="train", keep=c["keep"],
                       masks=c["masks"] if masks is None else masks, norm=norm)
    names = adr.weight_names(c["L"])[:-1]
    assert set(g64) == set(names)
    for n in names:
        assert_close(grads[n], g64[n], name="%s%s %s %s" % (tag, c["name"], norm, n))


# ----------------------------------------------------------------------------- every case, intended norms, two layers
@pytest.mark.parametrize("name", GRID_NAMES + STRUCTURE_NAMES)
def test_case_equals_the_float64_restatement(native, name):
    c = inputs(name, 2)
    with engine(native, c) as eng:
        assert eng.param_names == adr.weight_names(2)
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, A, G, grads = run_pass(native, eng, c, masks=c["masks"])
    assert_forward(c, "intended", H, A, G, reference(name, 2, "intended"))
    assert_gradients(c, "intended", H, grads)
    if name == "chunk_edges":                   # relation 2 has no edge: no chunk, and the reductions write zeros
        for l in (1, 2):
            for n in ("C_f", "C_b", "D_f", "D_b"):
                assert not grads["%s%d" % (n, l)][2].any(), (n, l)
                assert grads["%s%d" % (n, l)][3].any(), (n, l)       # ... and relation 3's one message arrives


# ----------------------------------------------------------------------------- every width case, local norms, one layer
@pytest.mark.parametrize("name", GRID_NAMES)
def test_case_as_the_top_layer_under_local_norms(native, name):
    """L = 1: the layer is the top layer, its epilogue runs without relu on short and long rows alike"""
    c = inputs(name, 1)
    with engine(native, c, norm_mode="local") as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, A, G, grads = run_pass(native, eng, c, masks=c["masks"])
    assert (H[1][:4] < 0).any(axis=1).all()                            # the hub rows, short and long, are not rectified
    assert_forward(c, "local", H, A, G, reference(name, 1, "local"))
    assert_gradients(c, "local", H, grads)


# ----------------------------------------------------------------------------- generated dropout at the widest cases
@pytest.mark.parametrize("vec", pg.VECS)
def test_generated_dropout_is_what_the_forward_used_on_the_second_lane_trip(native, vec):
    """drop_factor's index off + k at the largest offsets (V d = 308,400 at d = 1028) in the epilogue and, behind the
    backward pass, in the dropout copy k_pdiag_dh_join writes on its second lane trip"""
    c = inputs(pg.WIDEST[vec], 2)
    assert pg.vec_tpr(c["d"])[0] == vec and pg.lane_trips(c["d"]) == 2
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        H, A, G, grads = run_pass(native, eng, c, seed=4321 + vec)
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
    for m in masks:
        assert m.shape == (c["V"], c["d"]) and set(np.unique(m)) == {0, 1}
        assert 0.78 < m.mean() < 0.82
    ref = adr.forward(c["params"], c["triples"], c["V"], c["L"], mode="train", keep=c["keep"], masks=masks)
    assert_forward(c, "intended", H, A, G, ref, tag="generated dropout ")
    assert_gradients(c, "intended", H, grads, masks=masks, tag="generated dropout ")


# ----------------------------------------------------------------------------- determinism on the long-row paths
def test_two_passes_over_three_column_passes_are_bitwise_equal(native):
    c = inputs(pg.THREE_PASSES, 2)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        runs = [run_pass(native, eng, c, masks=c["masks"]) for _ in range(2)]
    for l in (1, 2):
        for q in range(3):
            assert np.array_equal(runs[0][q][l].view(np.uint32), runs[1][q][l].view(np.uint32)), (l, q)
    for n in runs[0][3]:
        assert np.array_equal(runs[0][3][n].view(np.uint32), runs[1][3][n].view(np.uint32)), n
