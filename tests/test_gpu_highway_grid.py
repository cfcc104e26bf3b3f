"""Every launch shape of the highway kernels (k_highway_fwd, k_highway_bwd, k_highway_join; csrc/highway.hip) on the GPU,
through the C ABI, at the cases of tests/highway_grid.py: one column lane and 256 of them, exact and ragged widths, both
sides of nvec 128 | 129 and 256 | 257, the column-chunk loop and the row loop beyond their first trip (1024 partial rows
under k_colsum_final), the forward's grid-stride loop beyond its first trip, three layers at width, and the block layer's
backward epilogue on a highway context.

The reference is the float64 restatement of tests/highway_reference.py.  Bounds are tests/test_gpu_highway.py's: H_l, N_l
and T_l FWD_ATOL = 1e-4 absolute, gradients helpers.assert_close defaults against the float64 reverse mode at the
engine's own H_l, N_l and T_l.  No bound is widened: tests/test_highway_grid.py shows on the CPU that a plain float32
evaluation passes these very checks on these very inputs (forward within 3.8e-06 everywhere)."""
import functools

import numpy as np
import pytest

import highway_grid as hg
import highway_reference as hr
from helpers import assert_close
from test_gpu_highway import FWD_ATOL, engine, forward_by_phases

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in hg.HIGHWAY_GRID_LIST]


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the case's weights, masks, upstream gradient and graph: made once, read by every test that runs the case"""
    c = hg.case_inputs(hg.HIGHWAY_GRID[name])
    for a in [c["triples"], c["dcodes"]] + c["masks"] + list(c["params"].values()):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 forward of the case with its own masks: (H, N, T), computed once"""
    c = inputs(name)
    ref = hr.forward(c["kind"], c["params"], c["triples"], c["V"], c["L"], mode="train", keep=c["keep"], masks=c["masks"])
    for part in ref:
        for a in part:
            if a is not None:
                a.setflags(write=False)
    return ref


def run_pass(native, eng, c, masks=None, seed=0):
    """forward by phases (N_l and T_l read behind every layer) + backward; ((H, N, T), gradients) of the engine"""
    acts = forward_by_phases(native, eng, c, True, masks=masks, seed=seed)
    eng.backward(c["dcodes"])
    return acts, eng.get_grads()


def assert_pass(c, acts, grads, ref, masks=None, tag=""):
    H, N, T = acts
    L = c["L"]
    for l in range(1, L + 1):
        for buf, got, want in (("H", H[l], ref[0][l]), ("N", N[l], ref[1][l]), ("T", T[l], ref[2][l])):
            err = float(np.abs(got - want).max())
            print("%s%s %s%d: max abs err %.3e (scale %.3e)" % (tag, c["name"], buf, l, err, float(np.abs(want).max())))
            assert err <= FWD_ATOL, (c["name"], buf, l, err)
        assert ((T[l] >= 0) & (T[l] <= 1)).all()
    if grads is None:
        return
    g64 = hr.backward(c["kind"], c["params"], c["triples"], c["V"], L, H, N, T, c["dcodes"], mode="train", keep=c["keep"],
                      masks=c["masks"] if masks is None else masks)
    names = hr.weight_names(c["kind"], L)[:-1]
    assert set(g64) == set(names)
    for n in names:      # b_highway<l> and b_emb come out of the column-partial path
        assert_close(grads[n], g64[n], name="%s%s %s" % (tag, c["name"], n))
    for l in range(1, L + 1):
        assert np.abs(grads["b_highway%d" % l]).min() > 0 and np.abs(grads["b_emb"]).max() > 0


# ----------------------------------------------------------------------------- every case, explicit masks
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_float64_restatement(native, name):
    c = inputs(name)
    with engine(native, c) as eng:
        assert eng.param_names == hr.weight_names(c["kind"], c["L"])
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        acts, grads = run_pass(native, eng, c, masks=c["masks"])
    assert_pass(c, acts, grads, reference(name))


def test_a_wide_case_under_gemm_mode_0(native):
    c = inputs(hg.GEMM_MODE_0)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        eng.set_gemm_mode(0)
        acts, grads = run_pass(native, eng, c, masks=c["masks"])
    assert_pass(c, acts, grads, reference(hg.GEMM_MODE_0), tag="gemm mode 0 ")


# ----------------------------------------------------------------------------- generated dropout at the widest cases
@pytest.mark.parametrize("vec", hg.VECS)
def test_generated_dropout_reaches_the_second_column_chunk_and_the_gradients(native, vec):
    """drop_factor's index off + k in the columns of the second column chunk; dS = D * dropout is formed in k_highway_bwd
    on a highway context, so W_self and the relational gradients see the generated masks too"""
    c = inputs(hg.WIDEST[vec])
    assert hg.vec_of(c["d"]) == vec and hg.column_chunks(c["d"]) == 2
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.set_graph(c["triples"])
        acts, grads = run_pass(native, eng, c, seed=4321 + vec)
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
    for m in masks:
        assert m.shape == (c["V"], c["d"]) and set(np.unique(m)) == {0, 1}
        assert 0.78 < m.mean() < 0.82
        tail = m[:, 256 * vec:]                                        # the columns of the second column chunk
        assert tail.shape[1] in (1, 4) and 0.7 < tail.mean() < 0.9
        assert not np.array_equal(m, c["masks"][0])
    ref = hr.forward(c["kind"], c["params"], c["triples"], c["V"], c["L"], mode="train", keep=c["keep"], masks=masks)
    assert_pass(c, acts, grads, ref, masks=masks, tag="generated dropout ")


# ----------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("vec", hg.VECS)
def test_two_identical_steps_give_the_same_bytes_with_two_row_trips(native, vec):
    c = inputs(hg.ROW_TRIPS[vec])
    assert hg.row_trips(c["V"], c["d"]) == 2
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        td, dd = eng.to_device(c["triples"]), eng.to_device(c["dcodes"])
        runs = []
        for _ in range(2):
            eng.step_device(td, len(c["triples"]), dd, train=True, seed=77)
            runs.append((eng.get_grads(), [eng.activation(l) for l in range(1, c["L"] + 1)]))
        td.free(); dd.free()
    for n in hr.weight_names(c["kind"], c["L"])[:-1]:
        assert np.array_equal(runs[0][0][n].view(np.uint32), runs[1][0][n].view(np.uint32)), n
        assert (n[0] == "b" and n[1].isdigit()) or runs[0][0][n].any(), n      # (the layers' own biases are unused)
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
