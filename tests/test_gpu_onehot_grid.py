"""Every compiled variant of the featureless first layer's kernels (k_onehot_fwd, k_onehot_tables, k_onehot_dcoef;
csrc/basis_onehot.hip) on the GPU, through the C ABI, at the cases of tests/onehot_grid.py: every (VEC, TPR) cell and
dispatch boundary, the second lane trip, the long-row column loop beyond its first pass, basis passes over long rows,
more long rows than long-row workgroups, the 64 -> 512 workgroup / 48 -> 96 chunk switch, relations at the chunk
boundaries.

The reference is the float64 restatement of tests/local_norm_reference.py with the norms passed in (one restatement for
every norm mode).  Bounds are the project's own: activations FWD_ATOL = 1e-4 absolute, gradients
helpers.assert_close(rel=2e-4) against the float64 reverse mode of the forward pass the engine computed (its own
activations decide the relu gates).  A plain float32 numpy evaluation of the same restatement on these graphs stays
inside both: forward within 5.2e-6 (intended, L = 2) and 2.0e-5 (local, L = 1), worst at d = 20, B = 64 each time."""
import functools

import numpy as np
import pytest

import featureless_reference as fr
import local_norm_reference as ln
import onehot_grid as og
from helpers import assert_close
from test_gpu_featureless import FWD_ATOL, engine

pytestmark = pytest.mark.gpu

GRID_NAMES = [c["name"] for c in og.ONEHOT_GRID_LIST]
STRUCTURE_NAMES = list(og.STRUCTURE_CASES)


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@functools.lru_cache(maxsize=None)
def inputs(name, L):
    """the case's weights, masks, upstream gradient and graph: made once, read by every test that runs the case"""
    c = og.case_inputs(og.ALL_CASES[name], L)
    for a in [c["triples"], c["dcodes"]] + c["masks"] + list(c["params"].values()):
        a.setflags(write=False)
    return c


def encoder_names(L):
    return fr.weight_names(L)[:-1]


def run_pass(eng, c, triples=None):
    """one forward + backward with the given masks; (activations, gradients) of the engine"""
    eng.set_graph(c["triples"] if triples is None else triples)
    eng.forward(train=True, masks=c["masks"])
    acts = [None] + [eng.activation(l) for l in range(1, c["L"] + 1)]
    eng.backward(c["dcodes"])
    return acts, eng.get_grads()


def assert_pass(c, norm, acts, grads, triples=None, masks=None, tag=""):
    """activations against the float64 forward, gradients against the float64 reverse mode at the engine's activations"""
    V, L = c["V"], c["L"]
    t = c["triples"] if triples is None else triples
    masks = c["masks"] if masks is None else masks
    n_f, n_b = ln.norms(t, V, norm)
    ref = ln.forward("onehot", c["params"], t, V, L, n_f, n_b, mode="train", masks=masks)
    for l in range(1, L + 1):
        err = float(np.abs(acts[l] - ref[l]).max())
        print("%s%s %s L%d H%d: max abs err %.3e (max |H| %.3g)" % (tag, c["name"], norm, L, l, err, np.abs(ref[l]).max()))
        assert err <= FWD_ATOL, (c["name"], norm, l, err)
    if grads is None:
        return
    g64 = ln.backward("onehot", c["params"], t, V, L, n_f, n_b, acts, c["dcodes"], mode="train", masks=masks)
    assert set(g64) == set(encoder_names(L))
    for n in encoder_names(L):                  # both tables, both coefficient sets, W_self and the unused bias, per layer
        assert_close(grads[n], g64[n], rel=2e-4, name="%s%s %s %s" % (tag, c["name"], norm, n))


# ----------------------------------------------------------------------------- every case, intended norms, two layers
@pytest.mark.parametrize("name", GRID_NAMES + STRUCTURE_NAMES)
def test_case_equals_the_float64_restatement(native, name):
    c = inputs(name, 2)
    with engine(native, c, "intended") as eng:
        assert eng.param_names == fr.weight_names(2)
        eng.set_params(c["params"])
        acts, grads = run_pass(eng, c)
    assert_pass(c, "intended", acts, grads)
    if name == "chunk_edges":                   # relation 2 has no edge: no chunk, and the reduction writes zeros
        assert not grads["C_f1"][2].any() and not grads["C_b1"][2].any()
        assert grads["C_f1"][3].any() and grads["C_b1"][3].any()       # ... and the single message of relation 3 arrives


# ----------------------------------------------------------------------------- every grid case, local norms, one layer
@pytest.mark.parametrize("name", GRID_NAMES)
def test_case_as_the_top_layer_under_local_norms(native, name):
    """L = 1: the one-hot layer is the top layer, its epilogue runs without relu on short and long rows alike.  With
    R = 237 nearly every (relation, vertex) run has length 1, so the 400-slot hub's sum is not damped: a second layer on
    top would carry |H2| in the hundreds, where a plain fp32 evaluation of the reference already misses 1e-4."""
    c = inputs(name, 1)
    with engine(native, c, "local") as eng:
        eng.set_params(c["params"])
        acts, grads = run_pass(eng, c)
    assert (acts[1][:4] < 0).any(axis=1).all()                         # the hub rows, short and long, are not rectified
    assert_pass(c, "local", acts, grads)


# ----------------------------------------------------------------------------- generated dropout at the widest cases
@pytest.mark.parametrize("vec", og.VECS)
def test_generated_dropout_is_what_the_forward_used_on_the_second_lane_trip(native, vec):
    """drop_factor's index off + k at the largest offsets (V d = 308,400 at d = 1028) and on the second lane trip"""
    c = inputs(og.WIDEST[vec], 2)
    assert og.onehot_vec_tpr(c["d"])[0] == vec and og.lane_trips(c["d"]) == 2
    with engine(native, c, "intended") as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.forward(train=True, seed=4321 + vec)
        acts = [None] + [eng.activation(l) for l in range(1, c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
    for m in masks:
        assert m.shape == (c["V"], c["d"]) and set(np.unique(m)) == {0, 1}
        assert 0.78 < m.mean() < 0.82
        tail = m[:, 4 * 256 if vec == 4 else 256:]                     # the columns of the second lane trip
        assert tail.shape[1] >= 4 and 0.7 < tail.mean() < 0.9
    assert_pass(c, "intended", acts, None, masks=masks, tag="generated dropout ")


# ----------------------------------------------------------------------------- stale table rows
def test_rows_of_vertices_that_stopped_sending_are_zeroed_in_every_basis_pass(native):
    """B = 17: three launches of k_onehot_tables.  Vertices that sent in both directions (long rows and short ones) appear
    in no edge of the next graph: every one of their 17 basis rows of both tables' gradients is exactly zero afterwards."""
    first, second, quiet = og.stale_graphs()
    c = dict(V=300, R=7, d=20, B=17, L=2, E=len(first), name="stale_rows")
    c["params"], _, c["masks"], c["dcodes"] = fr.make_case(c["V"], c["R"], c["d"], c["L"], c["B"], 0, seed=4100)
    c["triples"] = first
    with engine(native, c, "intended") as eng:
        eng.set_params(c["params"])
        _, g1 = run_pass(eng, c)
        acts, g2 = run_pass(eng, c, triples=second)
    for n in ("W_f1", "W_b1"):
        assert g1[n].shape == (c["V"], c["B"], c["d"])
        assert np.abs(g1[n][quiet]).max(axis=2).min() > 0, n          # every basis row of every quiet vertex was written
        assert not g2[n][quiet].any(), "%s: rows of the first graph survive in %d entries" % (
            n, np.count_nonzero(g2[n][quiet]))
    assert_pass(c, "intended", acts, g2, triples=second, tag="second graph ")


# ----------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["many_long_rows", "onehot_d516_B9"])
def test_two_identical_steps_give_the_same_bytes(native, name):
    c = inputs(name, 2)
    with engine(native, c, "intended") as eng:
        eng.set_params(c["params"])
        td, dd = eng.to_device(c["triples"]), eng.to_device(c["dcodes"])
        runs = []
        for _ in range(2):
            eng.step_device(td, len(c["triples"]), dd, train=True, seed=77)
            runs.append((eng.get_grads(), [eng.activation(l) for l in range(1, c["L"] + 1)]))
        td.free(); dd.free()
    for n in encoder_names(c["L"]):
        assert np.array_equal(runs[0][0][n].view(np.uint32), runs[1][0][n].view(np.uint32)), n
        assert n.startswith("b") or runs[0][0][n].any(), n
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
