"""The relation-softmax loss term on the GPU (csrc/relation_softmax.hip; include/rgcn.h rgcn_relation_softmax_device,
rgcn_set_relation_softmax) against the float64 mirror of tests/relation_softmax_reference.py.

Bounds: the energies within float64_relation_energies' forward error bound (tests/relation_query_reference.py); the loss
within 2e-5 x max(1, |loss|); dW_relation and dcodes within helpers.assert_close(rel=2e-4) -- what
tests/test_gpu_train_step.py and tests/test_gpu_embedding.py hold the decoder to; full-step gradients within
assert_close(rel=1e-3), that file's bound for them.  The stand-alone term is isolated by differencing against a weight-0
call on the same context and batch."""
import os

import numpy as np
import pytest

import helpers
import oracle
import relation_softmax_reference as rsr
from helpers import assert_close
from relation_query_reference import float64_relation_energies

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = 1, 4, 5        # RGCN_ERR_*
REG = 0.01


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def status_of(native, call, *args, **kw):
    with pytest.raises(native.RgcnError) as e:
        call(*args, **kw)
    return e.value.status


def decoder_batch(pos, V, seed):
    """the positives, label 1, and one object corruption of each, label 0"""
    rng = np.random.RandomState(seed)
    neg = pos.copy()
    neg[:, 2] = rng.randint(0, V, len(pos))
    X = np.concatenate([pos, neg]).astype(np.int32)
    Y = np.concatenate([np.ones(len(pos)), np.zeros(len(pos))]).astype(np.float32)
    return X, Y


def stand_alone(native, codes, w_rel, pos, R, weight, known=None, reserve=None, repeat=1):
    """The term on an embedding context (the codes are W_emb): decoder pass + weight-0 call, then decoder pass + the term.
    Returns the differences (loss, dcodes, dW) and the term's buffers; repeat > 1: the second pair `repeat` times, every
    result kept (bitwise repeatability)."""
    V, dc = codes.shape
    P = len(pos)
    X, Y = decoder_batch(pos, V, 5)
    out = {}
    with native.Engine(V, R, dc, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
        eng.decoder_reserve(len(X))
        eng.relation_softmax_reserve(reserve or P)
        if known is not None:
            eng.known_positives_reserve(known)
        xd, yd, pd = eng.to_device(X), eng.to_device(Y), eng.to_device(pos)
        eng.forward(train=True, seed=1)
        eng.decoder_loss_backward_device(xd, yd, len(X), REG)
        eng.relation_softmax_device(pd, P, 0.0, exclusive=known is not None)
        base = (eng.loss(), eng.dcodes(), eng.get_grad("W_relation"))
        runs = []
        for _ in range(repeat):
            eng.decoder_loss_backward_device(xd, yd, len(X), REG)
            eng.relation_softmax_device(pd, P, weight, exclusive=known is not None)
            runs.append((eng.loss(), eng.dcodes(), eng.get_grad("W_relation")))
        out["plan"] = native.relation_softmax_plan(reserve or P, R, dc)
        out["E"] = eng.read_buffer(native.BUF_RELATION_SOFTMAX_ENERGIES)
        out["G"] = eng.read_buffer(native.BUF_RELATION_SOFTMAX_G)
        out["dQ"] = eng.read_buffer(native.BUF_RELATION_SOFTMAX_DQ)
        for b in (xd, yd, pd):
            b.free()
    out["base"], out["runs"] = base, runs
    got = runs[0]
    out["loss"] = got[0] - base[0]
    out["dcodes"] = got[1].astype(np.float64) - base[1].astype(np.float64)
    out["dW"] = got[2].astype(np.float64) - base[2].astype(np.float64)
    return out


def check_against_mirror(out, codes, w_rel, pos, R, weight, known=None, name=""):
    ref = rsr.term(codes, w_rel, pos, R, weight, known=known)
    P = len(pos)
    assert abs(ref["loss"]) > 0 and np.abs(ref["dW"]).max() > 0 and np.abs(ref["dcodes"]).max() > 0, name
    total = out["base"][0] + ref["loss"]
    print("%s: term %.9g, mirror %.9g; loss with the term %.9g" % (name, out["loss"], ref["loss"], out["runs"][0][0]))
    assert abs(out["runs"][0][0] - total) <= 2e-5 * max(1.0, abs(total)), (name, out["runs"][0][0], total)
    if P <= out["plan"]["chunk"]:          # one chunk: the buffers hold every row
        E64, bound = float64_relation_energies(codes, w_rel, pos, R)
        E = out["E"][:P, :R].astype(np.float64)
        assert (np.abs(E - E64) <= bound).all(), (name, float(np.max(np.abs(E - E64) - bound)))
        assert not out["E"][:P, R:].any() and not out["G"][:P, R:].any(), name      # the pad columns stay zero
        assert_close(out["G"][:P, :R], ref["G"], rel=2e-4, name=name + " G")
        assert_close(out["dQ"][:P], ref["dq"], rel=2e-4, name=name + " dQ")
    dW = np.zeros_like(out["dW"])
    dW[:R] = ref["dW"]
    assert not out["dW"][R:].any(), name
    assert_close(out["dW"], dW, rel=2e-4, name=name + " dW_relation")
    assert_close(out["dcodes"], ref["dcodes"], rel=2e-4, name=name + " dcodes")
    return ref


# P round the GEMM's 128-row tile; R: the smallest legal count, a sub-wavefront count, a non-multiple of 4 above one
# wavefront, one past a 256-relation trip of the row kernel's loop; dc: the scalar path, the float4 path, one past the
# GEMM's 128-column tile
SHAPES = [(1, 18, 8), (127, 18, 8), (128, 18, 8), (129, 18, 8), (300, 18, 8),
          (129, 2, 8), (129, 67, 8), (129, 257, 8), (129, 18, 6), (129, 67, 132), (300, 257, 6)]


@pytest.mark.parametrize("P,R,dc", SHAPES, ids=["P%d-R%d-dc%d" % s for s in SHAPES])
def test_term_matches_float64(native, P, R, dc):
    V = max(R + 7, 90)
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed=P + R + dc, self_pairs=1)
    assert pos[0, 0] == pos[0, 2]                     # a self pair: both contributions land on one row
    out = stand_alone(native, codes, w_rel, pos, R, 0.8)
    check_against_mirror(out, codes, w_rel, pos, R, 0.8, name="P%d R%d dc%d" % (P, R, dc))


def masked_case():
    V, R, dc, P = 120, 18, 8, 260
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed=11)
    rng = np.random.RandomState(12)
    known = [pos]
    for n in range(0, P, 2):                            # every other pair knows one to three other relations
        for rr in rng.choice(R, size=1 + n % 3, replace=False):
            known.append(np.array([[pos[n, 0], rr, pos[n, 2]]], dtype=np.int32))
    return codes, w_rel, pos, np.concatenate(known).astype(np.int32), R


def test_masked_term_matches_float64(native):
    codes, w_rel, pos, known, R = masked_case()
    mask = rsr.candidate_mask(pos, R, len(codes), known)
    assert (~mask).any(axis=1).sum() >= 100             # at least 100 rows have a known other relation
    plain = rsr.term(codes, w_rel, pos, R, 0.8)
    out = stand_alone(native, codes, w_rel, pos, R, 0.8, known=known)
    ref = check_against_mirror(out, codes, w_rel, pos, R, 0.8, known=known, name="masked")
    assert abs(ref["loss"] - plain["loss"]) > 1e-3      # the mask matters on this fixture
    assert not out["G"][:len(pos), :R][~mask].any()     # no gradient outside the candidate sets


def test_saturated_mask_contributes_exactly_nothing(native):
    V, R, dc, P = 50, 2, 8, 70
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed=3)
    known = np.concatenate([np.stack([pos[:, 0], np.full(P, r), pos[:, 2]], 1) for r in range(R)]).astype(np.int32)
    assert abs(rsr.term(codes, w_rel, pos, R, 0.8)["loss"]) > 0          # (the plain term of this fixture is not zero)
    ref = rsr.term(codes, w_rel, pos, R, 0.8, known=known)
    assert ref["loss"] == 0 and not ref["G"].any()
    out = stand_alone(native, codes, w_rel, pos, R, 0.8, known=known)
    assert out["runs"][0][0] == out["base"][0]
    np.testing.assert_array_equal(out["runs"][0][1], out["base"][1])
    np.testing.assert_array_equal(out["runs"][0][2], out["base"][2])
    assert not out["G"][:P].any() and not out["dQ"][:P].any()


def test_hub_rows_on_both_sides_of_the_long_row_cut(native):
    V, R, dc, P = 90, 18, 8, 300
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed=21, hub=(4, 300, 50))
    cut = native.relation_softmax_plan(P, R, dc)["long_row"]
    counts = np.bincount(np.concatenate([pos[:, 0], pos[:, 2]]), minlength=V)
    assert (pos[:, 0] == 4).all() and (pos[:, 2] == 4).sum() >= 50 and counts[4] == counts.max() > cut and 0 < np.sort(counts)[-2] <= cut
    out = stand_alone(native, codes, w_rel, pos, R, 0.8)
    check_against_mirror(out, codes, w_rel, pos, R, 0.8, name="hub")


def test_chunked_call_matches_one_chunk_and_repeats_bitwise(native):
    V, R, dc, P = 90, 18, 8, 150
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed=31, self_pairs=2)
    assert native.relation_softmax_plan(64, R, dc)["chunk"] == 64
    chunked = stand_alone(native, codes, w_rel, pos, R, 0.8, reserve=64, repeat=2)
    whole = stand_alone(native, codes, w_rel, pos, R, 0.8)
    check_against_mirror(chunked, codes, w_rel, pos, R, 0.8, name="chunked")
    assert abs(chunked["runs"][0][0] - whole["runs"][0][0]) <= 2e-5 * max(1.0, abs(whole["runs"][0][0]))
    assert_close(chunked["dW"], whole["dW"], rel=2e-4, name="chunked against whole dW")
    assert_close(chunked["dcodes"], whole["dcodes"], rel=2e-4, name="chunked against whole dcodes")
    a, b = chunked["runs"]
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])


# ------------------------------------------------------------------ fused steps
def step_case(kind, nb):
    V, R, d, L, E, P = 80, 8, 20, 2, 300, 130
    params, triples, _, _ = helpers.make_case(V, R, d, L, kind, nb, E, seed=77)
    rng = np.random.RandomState(4)
    pos = triples[rng.choice(E, P, replace=False)].astype(np.int32)
    X, Y = decoder_batch(pos, V, 6)
    return dict(V=V, R=R, d=d, L=L, E=E, P=P, kind=kind, nb=nb, params=params, triples=triples, pos=pos, X=X, Y=Y)


def mirror_step(c, acts, masks, X, Y, pos, triples, weight):
    """decoder mirror + term mirror, pushed through the float64 encoder restatement at the engine's own activations"""
    codes = acts[-1]
    dloss, dcodes, dW = rsr.decoder(codes, c["params"]["W_relation"], X, Y, REG)
    t = rsr.term(codes, c["params"]["W_relation"], pos, c["R"], weight)
    assert abs(t["loss"]) > 0 and np.abs(t["dcodes"]).max() > 0
    dW[:c["R"]] += t["dW"]
    g64 = helpers.float64_grads_at(dict(V=c["V"], R=c["R"], d=c["d"], L=c["L"], kind=c["kind"], nb=c["nb"],
                                        params=c["params"], triples=triples, masks=masks, dcodes=dcodes + t["dcodes"]), acts)
    g64["W_relation"] = dW
    return dloss + t["loss"], g64


@pytest.mark.parametrize("kind,nb", [("block", 4), ("basis", 2)])
def test_train_step_device_with_the_term(native, kind, nb):
    c = step_case(kind, nb)
    # every parameter with a gradient: the per-layer biases of these two kinds are created and never read (their gradient
    # is all zeros), the exclusion tests/test_gpu_train_step.py makes with the same expression; they are checked to be zero
    names = [n for n in oracle.weight_names(kind, c["L"]) if not (n.startswith("b") and n != "b_emb")]
    with native.Engine(c["V"], c["R"], c["d"], c["L"], kind, nb, keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(c["X"]))
        eng.relation_softmax_reserve(c["P"])
        eng.set_relation_softmax(0.7, c["P"])
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"])
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        loss, grads = eng.loss(), eng.get_grads()
        acts = [eng.activation(l) for l in range(c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
        for b in (td, xd, yd):
            b.free()
    want, g64 = mirror_step(c, acts, masks, c["X"], c["Y"], c["pos"], c["triples"], 0.7)
    print("%s: loss %.9g, mirror %.9g" % (kind, loss, want))
    assert_close(np.array([loss]), np.array([want]), rel=1e-3, name="loss")
    for n in names:
        assert np.abs(g64[n]).max() > 0, n
        assert_close(grads[n], g64[n], rel=1e-3, name="grad " + n)
    for n in grads:
        assert n in names or not grads[n].any(), n


@pytest.mark.parametrize("kind,nb", [("block", 4), ("basis", 2)])
def test_train_step_minibatch_device_with_the_term(native, kind, nb):
    c = step_case(kind, nb)
    n, rate, keep = 200, 2, 120
    batch = np.unique(c["triples"], axis=0)[:n].astype(np.int32)
    assert len(batch) == n
    N = n * (rate + 1)
    # (the unread per-layer biases: as in test_train_step_device_with_the_term)
    names = [k for k in oracle.weight_names(kind, c["L"]) if not (k.startswith("b") and k != "b_emb")]
    with native.Engine(c["V"], c["R"], c["d"], c["L"], kind, nb, keep_prob=0.8, max_edges=n) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(N)
        eng.relation_softmax_reserve(n)
        eng.set_relation_softmax(0.7)                      # num_positives 0: the minibatch step only
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        eng.train_step_minibatch_device(bd, n, keep, 41, rate, 91, xd, yd, seed=8, reg_param=REG)
        loss, grads = eng.loss(), eng.get_grads()
        acts = [eng.activation(l) for l in range(c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
        graph = eng.graph_edges()
        X, Y = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        # an X/Y step under "the minibatch step only" is refused, and the context goes on
        assert status_of(native, eng.train_step_device, bd, n, xd, yd, N, seed=9, reg_param=REG) == STATE
        eng.set_relation_softmax(0.0)
        eng.train_step_device(bd, n, xd, yd, N, seed=9, reg_param=REG)
        assert np.isfinite(eng.loss())
        for b in (bd, xd, yd):
            b.free()
    np.testing.assert_array_equal(X[:n], batch)
    want, g64 = mirror_step(c, acts, masks, X, Y, batch, graph, 0.7)
    print("%s minibatch: loss %.9g, mirror %.9g" % (kind, loss, want))
    assert_close(np.array([loss]), np.array([want]), rel=1e-3, name="loss")
    for k in names:
        assert np.abs(g64[k]).max() > 0, k
        assert_close(grads[k], g64[k], rel=1e-3, name="grad " + k)
    for k in grads:
        assert k in names or not grads[k].any(), k


def test_weight_zero_restores_every_byte(native):
    """set and reset: loss, gradients and updated weights of both fused steps equal those of a context that never called
    the setter (the decoder writes the top layer's dropout copy again: the ds_ready route)"""
    c = step_case("block", 4)
    n, rate, keep = 200, 2, 120
    batch = np.unique(c["triples"], axis=0)[:n].astype(np.int32)
    N = n * (rate + 1)
    seen = []
    for touch in (False, True):
        with native.Engine(c["V"], c["R"], c["d"], c["L"], "block", 4, keep_prob=0.8, max_edges=c["E"]) as eng:
            eng.set_params(c["params"])
            eng.decoder_reserve(max(N, len(c["X"])))
            eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
            td, xd, yd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"])
            bd, xs, ys = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
            if touch:
                eng.relation_softmax_reserve(c["P"])
                eng.set_relation_softmax(0.7, c["P"])
                eng.set_relation_softmax(0.0, c["P"])
            got = []
            eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
            got.append((eng.loss(), eng.get_grads(), eng.get_params()))
            eng.train_step_minibatch_device(bd, n, keep, 41, rate, 91, xs, ys, seed=8, reg_param=REG)
            got.append((eng.loss(), eng.get_grads(), eng.get_params()))
            seen.append(got)
            for b in (td, xd, yd, bd, xs, ys):
                b.free()
    for a, b in zip(*seen):
        assert a[0] == b[0]
        for k in a[1]:
            np.testing.assert_array_equal(a[1][k], b[1][k], err_msg="grad " + k)
            np.testing.assert_array_equal(a[2][k], b[2][k], err_msg="weight " + k)


def test_embedding_step_runs_the_term(native):
    V, R, dc, P = 90, 18, 8, 140
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed=41)
    X, Y = decoder_batch(pos, V, 7)
    with native.Engine(V, R, dc, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
        eng.decoder_reserve(len(X))
        eng.relation_softmax_reserve(P)
        eng.set_relation_softmax(0.5, P)
        xd, yd = eng.to_device(X), eng.to_device(Y)
        eng.train_step_device(None, 0, xd, yd, len(X), seed=2, reg_param=REG)
        loss, grads = eng.loss(), eng.get_grads()
        for b in (xd, yd):
            b.free()
    dloss, dcodes, dW = rsr.decoder(codes, w_rel, X, Y, REG)
    t = rsr.term(codes, w_rel, pos, R, 0.5)
    dW[:R] += t["dW"]
    assert abs(loss - (dloss + t["loss"])) <= 2e-5 * max(1.0, abs(dloss + t["loss"]))
    assert abs(t["loss"]) > 1e-3
    assert_close(grads["W_emb"], dcodes + t["dcodes"], rel=1e-3, name="W_emb")
    assert_close(grads["W_relation"], dW, rel=1e-3, name="W_relation")


# ------------------------------------------------------------------ argument checks
def test_refusals_leave_the_context_usable(native):
    V, R, dc, P = 60, 9, 8, 40
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed=51)
    X, Y = decoder_batch(pos, V, 8)
    with native.Engine(V, R, dc, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
        eng.decoder_reserve(len(X))
        xd, yd, pd = eng.to_device(X), eng.to_device(Y), eng.to_device(pos)
        assert status_of(native, eng.read_buffer, native.BUF_RELATION_SOFTMAX_G) == STATE
        assert status_of(native, eng.relation_softmax_reserve, 0) == INVALID
        eng.relation_softmax_reserve(P)
        eng.forward(train=True, seed=1)
        assert status_of(native, eng.relation_softmax_device, pd, P, 0.5) == STATE        # no decoder pass yet
        eng.decoder_loss_backward_device(xd, yd, len(X), REG)
        for bad in (-1.0, float("nan"), float("inf")):
            assert status_of(native, eng.relation_softmax_device, pd, P, bad) == INVALID
            assert status_of(native, eng.set_relation_softmax, bad, P) == INVALID
        assert status_of(native, eng.relation_softmax_device, pd, 0, 0.5) == INVALID
        assert status_of(native, eng.set_relation_softmax, 0.5, -1) == INVALID
        assert status_of(native, eng.relation_softmax_device, pd, P, 0.5, exclusive=True) == STATE    # no index
        assert status_of(native, eng.set_relation_softmax, 0.5, P, exclusive=True) == STATE
        # an id out of range fails through the error flag at the next synchronising call; nothing faults
        for col, value in ((0, V), (1, R), (2, -1)):
            wrong = pos.copy()
            wrong[7, col] = value
            wd = eng.to_device(wrong)
            eng.decoder_loss_backward_device(xd, yd, len(X), REG)
            eng.relation_softmax_device(wd, P, 0.5)
            assert status_of(native, eng.loss) == INVALID
            wd.free()
        # a leading row with label 0 in an X/Y step
        eng.set_relation_softmax(0.5, P + 1)
        eng.train_step_device(None, 0, xd, yd, len(X), seed=2, reg_param=REG)
        assert status_of(native, eng.loss) == INVALID
        eng.set_relation_softmax(0.5, len(X) + 1)
        assert status_of(native, eng.train_step_device, None, 0, xd, yd, len(X), seed=2, reg_param=REG) == INVALID
        eng.set_relation_softmax(0.5, 0)
        assert status_of(native, eng.train_step_device, None, 0, xd, yd, len(X), seed=2, reg_param=REG) == STATE
        # the context goes on: the term of the good batch is the mirror's
        eng.set_relation_softmax(0.0)
        eng.decoder_loss_backward_device(xd, yd, len(X), REG)
        base = eng.loss()
        eng.decoder_loss_backward_device(xd, yd, len(X), REG)
        eng.relation_softmax_device(pd, P, 0.5)
        t = rsr.term(codes, w_rel, pos, R, 0.5)["loss"]
        assert abs(eng.loss() - base - t) <= 2e-5 * max(1.0, abs(base + t))
        for b in (xd, yd, pd):
            b.free()
    # a relation-sharded context: the setter succeeds, both fused steps and the stand-alone call are refused while the
    # term is on (ahead of the check for a communicator, which this context does not have), and with the weight back at 0
    # the step's refusal is the communicator's again
    with native.Engine(V, R, 8, 1, "block", 2, max_edges=P, rank=0, world=2) as sharded:
        sharded.decoder_reserve(len(X))
        sharded.relation_softmax_reserve(P)
        xd, yd, pd = sharded.to_device(X), sharded.to_device(Y), sharded.to_device(pos)
        sharded.set_relation_softmax(0.5, P)
        assert status_of(native, sharded.train_step_device, pd, P, xd, yd, len(X), seed=2, reg_param=REG) == UNSUPPORTED
        assert status_of(native, sharded.train_step_minibatch_device, pd, P, P // 2, 3, 1, 4, xd, yd, seed=2,
                         reg_param=REG) == UNSUPPORTED
        assert status_of(native, sharded.relation_softmax_device, pd, P, 0.5) == UNSUPPORTED
        sharded.set_relation_softmax(0.0, P)
        assert status_of(native, sharded.train_step_device, pd, P, xd, yd, len(X), seed=2, reg_param=REG) == STATE
        for b in (xd, yd, pd):
            b.free()
    with native.Engine(V, 1, dc, 0, "embedding", 1) as eng:                 # one relation: nothing to tell apart
        assert status_of(native, eng.relation_softmax_reserve, P) == INVALID
        assert status_of(native, eng.set_relation_softmax, 0.5, P) == INVALID
        eng.set_relation_softmax(0.0, P)


def test_capture_and_step_state_rules(native):
    c = step_case("block", 4)
    with native.Engine(c["V"], c["R"], c["d"], c["L"], "block", 4, keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(c["X"]))
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"])
        eng.set_relation_softmax(0.7, c["P"])
        # the step needs the reserve
        assert status_of(native, eng.train_step_device, td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG) == STATE
        eng.relation_softmax_reserve(c["P"])
        eng.set_relation_softmax(0.0)
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        eng.capture_begin()
        assert status_of(native, eng.set_relation_softmax, 0.7, c["P"]) == STATE
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        gid = eng.capture_end()
        eng.graph_launch(gid)
        eng.sync()
        eng.graph_destroy(gid)
        eng.set_relation_softmax(0.7, c["P"])
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        assert np.isfinite(eng.loss())
        for b in (td, xd, yd):
            b.free()


# ------------------------------------------------------------------ the driver
DRIVER_PATHS = {"device": [], "host_sampler": ["--host-sampler"], "host_dropout": ["--host-edge-dropout"],
                "host_negatives": ["--host-negatives", "--batch-workers", "0"]}


def assert_weights_did_not_move(eng):
    """Adam's step is at most a few times the learning rate, 1e-30 here: an entry of 1e-20 or more has an ulp above
    1e-27 and keeps its bits; an entry the initialiser left at zero ends below 1e-28, which no mirror at 2e-5 sees"""
    for name in eng.param_names:
        w = np.abs(eng.get_param(name).astype(np.float64))
        assert ((w <= 1e-28) | (w >= 1e-20)).all(), name


DRIVER_CASES = ([(p, 1, False) for p in sorted(DRIVER_PATHS)] + [(p, 2, False) for p in sorted(DRIVER_PATHS)] +
                [("device", 1, True), ("host_dropout", 1, True), ("host_negatives", 1, True)])


@pytest.mark.parametrize("path,iterations,exclusive", DRIVER_CASES,
                         ids=["%s-%d%s" % (p, i, "-masked" if e else "") for p, i, e in DRIVER_CASES])
def test_train_driver_with_the_term(tmp_path, capsys, path, iterations, exclusive):
    """[Decoder] RelationSoftmaxWeight=0.5 with Metric=RelationMRR through `train` on the toy dataset of
    tests/test_gpu_driver.py, on each of the four paths.  One iteration: the FIRST loss the driver reports ("Initial
    loss") is the device's and equals decoder mirror + term mirror on the batch that step trained on, read back from the
    device where the device drew it.  Two iterations: the same for the last step.  The learning rate is 1e-30, so the
    weights read back afterwards are the ones the step saw (assert_weights_did_not_move).  masked:
    ExclusiveNegativeSampling=Yes, the training set is the term's mask."""
    from relationprediction_amd import train
    from test_gpu_driver import SETTINGS, write_dataset
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    os.makedirs(str(tmp_path / "models"))
    settings = tmp_path / "toy.exp"
    text = ((SETTINGS % dict(nb=4, concat="Yes", exp=str(tmp_path / "models" / "Toy")))
            .replace("RegularizationParameter=0.01", "RegularizationParameter=0.01\n\tRelationSoftmaxWeight=0.5")
            .replace("learning_rate=0.01", "learning_rate=1e-30")
            .replace("Metric=MRR", "Metric=RelationMRR"))
    if exclusive:
        text = text.replace("GraphBatchSize=300", "GraphBatchSize=300\n\tExclusiveNegativeSampling=Yes")
    settings.write_text(text)
    np.random.seed(0)
    model, done = train.main(["--settings", str(settings), "--dataset", data, "--max-iterations", str(iterations)]
                             + DRIVER_PATHS[path])
    out = capsys.readouterr().out
    assert done == iterations and model.relation_softmax_weight == 0.5
    assert (model.relation_softmax_known is not None) == exclusive
    rt = model.get_runtime()
    eng = rt.engine
    n, N = 300, 300 * 6
    assert rt._relsm_state == (0.5, n, exclusive) and rt._relsm_reserved >= n
    assert_weights_did_not_move(eng)
    loss = eng.loss()
    first = [l for l in out.splitlines() if l.startswith("Initial loss: ")]
    assert len(first) == 1
    if iterations == 1:
        assert float(first[0].split(": ")[1]) == loss          # the first reported loss is this step's
    X, Y = rt._dev["X"].download(np.int32, (N, 3)), rt._dev["Y"].download(np.float32, (N,))
    assert Y[:n].all() and not Y[n:].any()
    K = {tuple(t) for t in train_triples.tolist()}
    assert all(tuple(t) in K for t in X[:n].tolist())
    codes = eng.activation(2)
    w_rel = eng.get_param("W_relation")
    dloss, _, _ = rsr.decoder(codes, w_rel, X, Y, REG)
    t = rsr.term(codes, w_rel, X[:n], 6, 0.5, known=train_triples if exclusive else None)
    print("%s: loss %.9g, decoder mirror %.9g + term mirror %.9g" % (path, loss, dloss, t["loss"]))
    assert abs(t["loss"]) > 0.1
    if exclusive:                                              # (pairs of the batch with a second training relation exist)
        plain = rsr.term(codes, w_rel, X[:n], 6, 0.5)["loss"]
        print("masked %.9g, plain %.9g, rows with a masked relation %d" % (t["loss"], plain, int((~t["mask"]).any(axis=1).sum())))
    assert abs(loss - (dloss + t["loss"])) <= 2e-5 * max(1.0, abs(dloss + t["loss"]))
