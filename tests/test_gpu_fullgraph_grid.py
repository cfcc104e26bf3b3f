"""Highway, IncidenceNormalization=local and the output transform on the GPU at full-graph scale (tests/fullgraph_grid.py's
table: V 3000, E 33,000, rows of 2049 .. 6000 slots cut into pieces, the third branch of bwd_block_rows), against the
float64 restatement built from the features' own reference modules.

The bars are the features' own, unchanged: every activation (H_l, N_l, T_l, codes) within FWD_ATOL = 1e-4 absolute of the
float64 forward, every gradient within helpers.assert_close's defaults of the float64 reverse mode evaluated at the
engine's own activations.  No other bar was needed: tests/test_fullgraph_grid.py shows on the CPU that a plain float32
evaluation in one summation order passes these very checks on these very inputs, 6000-term sums included.

Distances from float64, the worst tensor of each case: `max abs (max / l2 relative to the tensor's scale)` over the
activations, `max / l2 relative` over the gradients.  The float32 restatement's are measured on the CPU
(tests/test_fullgraph_grid.py prints them), the engine's on an MI355X (item 1: train mode, the case's masks).

  case              float32 restatement           its gradients      engine                        its gradients
  fg_highway        1.8e-07 (1.2e-06 / 2.4e-07)   1.7e-06 / 1.1e-06  9.3e-08 (3.4e-07 / 1.8e-07)   1.0e-06 / 8.0e-07
  fg_highway_L3     2.6e-07 (9.9e-07 / 2.8e-07)   1.2e-06 / 1.0e-06  9.4e-08 (3.5e-07 / 1.9e-07)   1.2e-06 / 1.2e-06
  fg_highway_wide   8.7e-06 (2.6e-06 / 3.7e-07)   2.7e-06 / 1.1e-06  2.7e-06 (9.6e-07 / 4.9e-07)   7.2e-07 / 5.3e-07
  fg_highway_vec1   1.5e-07 (1.6e-06 / 2.0e-07)   1.6e-06 / 1.2e-06  9.6e-08 (2.7e-07 / 1.4e-07)   7.4e-07 / 5.5e-07
  fg_highway_basis  2.4e-06 (1.2e-06 / 4.8e-07)   2.1e-06 / 1.5e-06  3.8e-07 (2.4e-07 / 1.4e-07)   1.0e-06 / 6.3e-07
  fg_local          2.4e-06 (1.2e-06 / 8.1e-07)   2.1e-06 / 1.8e-06  4.3e-07 (2.2e-07 / 1.7e-07)   6.1e-07 / 3.6e-07
  fg_out            5.0e-07 (2.2e-06 / 3.3e-07)   2.3e-06 / 1.3e-06  8.7e-08 (2.7e-07 / 1.8e-07)   1.3e-06 / 7.9e-07
  fg_all            3.9e-06 (1.6e-06 / 9.2e-07)   2.6e-06 / 1.4e-06  4.3e-07 (2.3e-07 / 1.7e-07)   5.5e-07 / 5.8e-07

Test mode (item 2), the engine: fg_highway 9.2e-08 (3.8e-07 / 1.7e-07), fg_local 3.6e-07 (1.8e-07 / 1.7e-07), fg_all
5.6e-07 (2.3e-07 / 1.7e-07).  Generated dropout (item 5), fg_highway: 9.2e-08 (3.6e-07 / 1.8e-07), gradients 7.1e-07 /
8.1e-07.  Row 6 of N_1 without its last piece sits more than 1e-3 from the true mirror (item 8): ten bars away.
"""
import functools

import numpy as np
import pytest

import fullgraph_grid as fg
import giant_grid as gg
from test_gpu_highway import forward_by_phases
from test_gpu_local_norm import assert_prep

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in fg.FULLGRAPH_GRID]


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def _freeze(arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case with its graph, weights, masks and upstream gradient: built once per module and never written to."""
    c = fg.case_inputs(fg.FULLGRAPH_CASES[name])
    _freeze([c["triples"], c["dcodes"]] + list(c["masks"]) + list(c["params"].values()))
    return c


@functools.lru_cache(maxsize=None)
def reference(name, mode="train"):
    """The float64 forward of the case (train mode: with its own masks), computed once."""
    ref = fg.reference_forward(inputs(name), mode=mode)
    for v in ref.values():
        _freeze(v if isinstance(v, list) else [v])
    return ref


def make_engine(native, c, fusion=None):
    eng = native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], keep_prob=fg.KEEP, norm_mode=c["norm"],
                        max_edges=c["max_edges"], skip=c["skip"], code_dim=c["code_dim"] or None)
    try:
        assert eng.param_names == fg.weight_names(c)
        if fusion is not None:
            eng.set_fusion(fusion)
        eng.set_params(c["params"])
    except Exception:
        eng.close()
        raise
    return eng


def run_step(native, eng, c, triples=None, train=True, generated=False, seed=0, backward=True):
    """One forward pass (a highway context: by phases, N_l and T_l read behind every layer, as
    test_gpu_highway.forward_by_phases does) and, in train mode, the backward pass: (activations, gradients)."""
    eng.set_graph(c["triples"] if triples is None else triples)
    masks = c["masks"] if train and not generated else None
    acts = {}
    if c["skip"] == "highway":
        acts["H"], acts["N"], acts["T"] = forward_by_phases(native, eng, c, train, masks=masks, seed=seed)
    else:
        eng.forward(train=train, seed=seed, masks=masks)
        acts["H"] = [eng.activation(l) for l in range(c["L"] + 1)]
    codes = eng.codes()
    if c["code_dim"]:
        assert codes.shape == (c["V"], c["code_dim"])
        acts["codes"] = codes
    else:
        np.testing.assert_array_equal(codes, acts["H"][c["L"]])
    grads = None
    if backward:
        eng.backward(c["dcodes"])
        grads = eng.get_grads()
    return acts, grads


def fresh_step(native, c, fusion=None, **kw):
    with make_engine(native, c, fusion) as eng:
        return run_step(native, eng, c, **kw)


_RUNS = {}


def run_of(native, name):
    """The engine's train step on a case (injected masks), in a fresh context, once per module."""
    if name not in _RUNS:
        _RUNS[name] = fresh_step(native, inputs(name))
    return _RUNS[name]


def assert_same_step(c, got, want, tag, b_emb_scale=None):
    """bitwise; b_emb_scale: b_emb within 2e-6 of that scale instead (two fixed orders of the same column sums)"""
    for (name, x), (_, y) in zip(fg.compared_activations(c, got[0]), fg.compared_activations(c, want[0])):
        np.testing.assert_array_equal(x, y, err_msg="%s %s" % (tag, name))
    assert (got[1] is None) == (want[1] is None)
    for k in (want[1] or {}):
        if k == "b_emb" and b_emb_scale is not None:
            assert np.abs(got[1][k].astype(np.float64) - want[1][k]).max() <= 2e-6 * b_emb_scale, (tag, k)
            continue
        np.testing.assert_array_equal(got[1][k], want[1][k], err_msg="%s %s" % (tag, k))


def report(name, what, fwd, bwd=()):
    print("%s %s: %s | %s" % (name, what, "; ".join(fwd), "; ".join(bwd)))


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("name", NAMES)
def test_train_step_against_float64(native, name):
    """Train-mode forward with the case's masks, then backward: every activation and every gradient of every case."""
    c = inputs(name)
    E = len(c["triples"])
    assert gg.giant_on(E, c["kind"]) == (c["kind"] == "block") and 2 * E > gg.GIANT_MESSAGES
    assert sorted(gg.giant_rows(c)) == fg.GIANT_ROWS[name]
    acts, grads = run_of(native, name)
    g64 = fg.reference_backward(c, acts)
    report(name, "engine against float64", *fg.check_against_float64(c, acts, grads, reference(name), g64))


# ------------------------------------------------------------------ 2. the evaluation pass
@pytest.mark.parametrize("name", fg.EVAL_CASES)
def test_evaluation_pass_against_float64(native, name):
    """train = False, forward only: what a full-graph evaluation runs, and what the ranks are computed from."""
    c = inputs(name)
    acts, _ = fresh_step(native, c, train=False, backward=False)
    report(name, "test mode against float64", fg.check_forward(c, acts, reference(name, "test"), tag="test mode "))


# ------------------------------------------------------------------ 3. the message norms, exactly
def test_message_norms_along_the_pieces_are_the_host_recount_bitwise(native):
    c = inputs("fg_local")
    t, E, R = c["triples"], len(c["triples"]), c["R"]
    with make_engine(native, c) as eng:
        eng.set_graph(t)
        perm, got = assert_prep(native, eng, t, c["V"], R, "local", tag="fg_local")
        row_ptr = eng.read_buffer(native.BUF_ROWPTR)
        perm_vertex = eng.read_buffer(native.BUF_PERM_VERTEX)
    norm_of = np.empty(2 * E, dtype=np.float32)
    norm_of[perm] = got
    # the slot order the table's row bookkeeping assumes is the engine's
    for v in (3, fg.HUB_LOCAL, fg.HUB_LOST):
        inc, _ = fg.row_slot_order(t, R, v)
        np.testing.assert_array_equal(perm_vertex[row_ptr[v]:row_ptr[v + 1]], inc, err_msg="row %d" % v)
    inc, rel2 = fg.row_slot_order(t, R, fg.HUB_LOCAL)
    assert fg.runs_of(rel2) == [2049, 2048]
    along = norm_of[inc]
    assert (along[:2049] == np.float32(1) / np.float32(2049)).all()       # slot 2048, in the second piece, among them
    assert (along[2049:] == np.float32(1) / np.float32(2048)).all()


# ------------------------------------------------------------------ 4. both forms
@pytest.mark.parametrize("name", fg.FORM_CASES)
def test_single_pass_equals_the_two_kernel_form(native, name):
    """set_fusion(1) (k_block_rows' pieces) against set_fusion(0) (combine()'s own giant branch under these epilogues):
    activations and gradients bitwise, b_emb within 2e-6 of scale where the two forms sum it in different orders
    (test_gpu_parity.py::_single_pass_equals_two_kernel_form's rule)."""
    c = inputs(name)
    fused, two = fresh_step(native, c, fusion=1), fresh_step(native, c, fusion=0)
    scale = float(np.abs(two[1]["W_emb"]).astype(np.float64).sum(axis=0).max()) + 1e-30
    assert_same_step(c, fused, two, name, b_emb_scale=scale)
    assert_same_step(c, fused, run_of(native, name), name + " (the default form is the single pass)")
    assert np.abs(fused[1]["W_f1"]).max() > 0


# ------------------------------------------------------------------ 5. generated dropout
def test_generated_dropout_on_giant_rows(native):
    """masks = None and a seed: drop_factor's index on giant rows through the finish kernel.  The masks are read back and
    handed to the mirror; item 1's bars."""
    name = "fg_highway"
    c = inputs(name)
    with make_engine(native, c) as eng:
        acts, grads = run_step(native, eng, c, generated=True, seed=4321)
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
    for m, given in zip(masks, c["masks"]):
        assert m.shape == (c["V"], c["d"]) and set(np.unique(m)) == {0, 1} and 0.78 < m.mean() < 0.82
        assert not np.array_equal(m, given)
        assert 0.6 < m[3:7].mean() < 0.95            # the giant rows
    ref = fg.reference_forward(c, masks=masks)
    g64 = fg.reference_backward(c, acts, masks=masks)
    report(name, "generated dropout against float64", *fg.check_against_float64(c, acts, grads, ref, g64, tag="generated "))


# ------------------------------------------------------------------ 6. one context, both regimes
def test_one_highway_context_alternates_between_the_regimes(native):
    """The product's rhythm on ONE context of max_edges = 33,000: a step on a 3000-edge graph (minibatch branch, cut off),
    the full graph in test mode, the full graph in train mode with backward, the 3000-edge step again -- each bitwise
    the result of a fresh engine given only that graph (nothing of hw_N / hw_T / giant_slab / colsum_parts / dw_pending
    survives a change of regime)."""
    name = "fg_highway"
    c = inputs(name)
    small = fg.small_triples(c)
    assert not gg.giant_on(len(small)) and gg.giant_on(len(c["triples"])) and c["max_edges"] == 33000
    want_small = fresh_step(native, c, triples=small)
    want_eval = fresh_step(native, c, train=False, backward=False)
    with make_engine(native, c) as eng:
        assert_same_step(c, run_step(native, eng, c, triples=small), want_small, "minibatch step")
        assert_same_step(c, run_step(native, eng, c, train=False, backward=False), want_eval, "full graph, test mode")
        assert_same_step(c, run_step(native, eng, c), run_of(native, name), "full graph, train step")
        assert_same_step(c, run_step(native, eng, c, triples=small), want_small, "minibatch step again")


def test_one_local_norm_context_alternates_between_the_regimes(native):
    """The same, forward only, under IncidenceNormalization=local: no norm of the other graph survives."""
    name = "fg_local"
    c = inputs(name)
    small = fg.small_triples(c)
    want_small = fresh_step(native, c, triples=small, backward=False)
    want_eval = fresh_step(native, c, train=False, backward=False)
    want_train = (run_of(native, name)[0], None)
    with make_engine(native, c) as eng:
        assert_same_step(c, run_step(native, eng, c, triples=small, backward=False), want_small, "minibatch graph")
        assert_same_step(c, run_step(native, eng, c, train=False, backward=False), want_eval, "full graph, test mode")
        assert_same_step(c, run_step(native, eng, c, backward=False), want_train, "full graph, train mode")
        assert_same_step(c, run_step(native, eng, c, triples=small, backward=False), want_small, "minibatch graph again")


# ------------------------------------------------------------------ 7. repeatability
def test_two_fresh_engines_give_identical_bytes(native):
    name = "fg_all"
    c = inputs(name)
    assert_same_step(c, fresh_step(native, c), run_of(native, name), name)


# ------------------------------------------------------------------ 8. the check can fail
@pytest.mark.parametrize("name", fg.LOST_PIECE_CASES)
def test_the_check_would_see_a_lost_piece(native, name):
    """Item 1's comparison, handed a mirror whose N_1 lacks the last piece (1904 slots) of the 6000-slot row, reports a
    failure -- and it passes against the true mirror (test_train_step_against_float64).  No altered kernel runs."""
    c = inputs(name)
    acts, _ = run_of(native, name)
    lost, moved = fg.lost_piece_mirror(c, reference(name))
    assert moved > 10 * fg.FWD_ATOL
    with pytest.raises(AssertionError, match="N1 against float64"):
        fg.check_forward(c, acts, lost)
    fg.check_forward(c, acts, reference(name))
