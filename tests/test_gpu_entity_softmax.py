"""The entity-softmax loss term on the GPU (csrc/entity_softmax.hip; include/rgcn.h rgcn_entity_softmax_device,
rgcn_set_entity_softmax) against the float64 mirror of tests/entity_softmax_reference.py.

Bounds, those of tests/test_gpu_relation_softmax.py: the loss within 2e-5 x max(1, |loss|); G, dQ, dW_relation and dcodes
within helpers.assert_close(rel=2e-4); full-step gradients within assert_close(rel=1e-3), that file's bound for them.
The stand-alone term is isolated by differencing against a weight-0 call on the same context and batch."""
import os

import numpy as np
import pytest

import adversarial_reference as adv
import entity_softmax_reference as esr
import helpers
import oracle
import relation_softmax_reference as rsr
from helpers import assert_close

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
        eng.entity_softmax_reserve(reserve or P)
        if known is not None:
            eng.known_positives_reserve(known)
        xd, yd, pd = eng.to_device(X), eng.to_device(Y), eng.to_device(pos)
        eng.forward(train=True, seed=1)
        eng.decoder_loss_backward_device(xd, yd, len(X), REG)
        eng.entity_softmax_device(pd, P, 0.0, exclusive=known is not None)
        base = (eng.loss(), eng.dcodes(), eng.get_grad("W_relation"))
        runs = []
        for _ in range(repeat):
            eng.decoder_loss_backward_device(xd, yd, len(X), REG)
            eng.entity_softmax_device(pd, P, weight, exclusive=known is not None)
            runs.append((eng.loss(), eng.dcodes(), eng.get_grad("W_relation")))
        out["plan"] = native.entity_softmax_plan(reserve or P, V, dc)
        out["G"] = eng.read_buffer(native.BUF_ENTITY_SOFTMAX_G)
        out["dQ"] = eng.read_buffer(native.BUF_ENTITY_SOFTMAX_DQ)
        for b in (xd, yd, pd):
            b.free()
    out["base"], out["runs"] = base, runs
    got = runs[0]
    out["loss"] = got[0] - base[0]
    out["dcodes"] = got[1].astype(np.float64) - base[1].astype(np.float64)
    out["dW"] = got[2].astype(np.float64) - base[2].astype(np.float64)
    return out


def check_against_mirror(out, codes, w_rel, pos, weight, known=None, name=""):
    ref = esr.term(codes, w_rel, pos, weight, known=known)
    M, V = 2 * len(pos), len(codes)
    # nothing compares zeros
    assert abs(ref["loss"]) > 0 and np.abs(ref["G"]).max() > 0 and np.abs(ref["dq"]).max() > 0, name
    assert np.abs(ref["dW"]).max() > 0 and np.abs(ref["dcodes"]).max() > 0, name
    total = out["base"][0] + ref["loss"]
    print("%s: term %.9g, mirror %.9g; loss with the term %.9g" % (name, out["loss"], ref["loss"], out["runs"][0][0]))
    assert abs(out["runs"][0][0] - total) <= 2e-5 * max(1.0, abs(total)), (name, out["runs"][0][0], total)
    if M <= out["plan"]["chunk"]:          # one chunk: the buffers hold every row
        assert out["G"].shape[1] == out["plan"]["padded_v"] == (V + 3) // 4 * 4
        assert not out["G"][:M, V:].any(), name                         # the pad columns stay zero
        assert_close(out["G"][:M, :V], ref["G"], rel=2e-4, name=name + " G")
        assert_close(out["dQ"][:M], ref["dq"], rel=2e-4, name=name + " dQ")
    assert_close(out["dW"], ref["dW"], rel=2e-4, name=name + " dW_relation")
    assert_close(out["dcodes"], ref["dcodes"], rel=2e-4, name=name + " dcodes")
    return ref


# (P, V, R, dc).  P: 2P rows on both sides of the GEMM's 128-row tile (128, then 130), one positive, and 300 rows (two
# slices of the TN product); V: the smallest legal count, round one wavefront's stride of 64 float4 = 256 columns and past a
# second trip, multiples and non-multiples of 4; dc: the scalar path, the float4 path, one past a 128-column tile
SHAPES = [(1, 64, 2, 8), (1, 2, 2, 6), (64, 64, 18, 8), (65, 65, 18, 8), (65, 2, 2, 8), (65, 63, 18, 6), (64, 63, 2, 132),
          (64, 257, 18, 8), (150, 257, 18, 6), (150, 300, 18, 8), (65, 300, 2, 132), (150, 65, 18, 132)]


@pytest.mark.parametrize("P,V,R,dc", SHAPES, ids=["P%d-V%d-R%d-dc%d" % s for s in SHAPES])
def test_term_matches_float64(native, P, V, R, dc):
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed=P + V + R + dc)
    a, r, g, _ = esr.rows_of(pos)
    assert (g == 0).any() and (g == V - 1).any()                       # golds on the first and the last column
    assert P == 1 or pos[0, 0] == pos[0, 2]                            # both rows and both roles on one entity
    out = stand_alone(native, codes, w_rel, pos, R, 0.8)
    check_against_mirror(out, codes, w_rel, pos, 0.8, name="P%d V%d R%d dc%d" % (P, V, R, dc))


def masked_case():
    V, R, dc, P = 120, 18, 8, 130
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed=11)
    rng = np.random.RandomState(12)
    known = [pos]
    for n in range(0, P, 2):                            # every other positive: one to three more known objects of (s, r) ...
        for e in rng.choice(V, size=1 + n % 3, replace=False):
            known.append(np.array([[pos[n, 0], pos[n, 1], e]], dtype=np.int32))
    for n in range(1, P, 2):                            # ... and for the others, more known subjects of (r, o)
        for e in rng.choice(V, size=1 + n % 3, replace=False):
            known.append(np.array([[e, pos[n, 1], pos[n, 2]]], dtype=np.int32))
    return codes, w_rel, pos, np.concatenate(known).astype(np.int32), R


def test_masked_term_matches_float64(native):
    codes, w_rel, pos, known, R = masked_case()
    V = len(codes)
    mask = esr.candidate_mask(pos, V, known)
    a, r, g, _ = esr.rows_of(pos)
    assert mask.shape == (260, V) and (~mask).any(axis=1).sum() >= 100  # at least 100 of the 260 rows mask something
    assert mask[np.arange(260), g].all()                                # the gold stays a candidate although it is in K
    plain = esr.term(codes, w_rel, pos, 0.8)
    out = stand_alone(native, codes, w_rel, pos, R, 0.8, known=known)
    ref = check_against_mirror(out, codes, w_rel, pos, 0.8, known=known, name="masked")
    assert abs(ref["loss"] - plain["loss"]) > 1e-3                      # the mask matters on this fixture
    G = out["G"][:260, :V]
    assert not G[~mask].any()                                           # exactly zero outside the candidate sets
    assert (G[np.arange(260), g] < 0).all()                             # ... and the gold is inside: softmax - 1 < 0


def test_saturated_mask_contributes_exactly_nothing(native):
    V, R, dc, P = 5, 2, 8, 40
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed=3)
    every = np.arange(V)
    known = np.concatenate([np.stack([np.full(V, s), np.full(V, r), every], 1) for s, r, o in pos.tolist()] +
                           [np.stack([every, np.full(V, r), np.full(V, o)], 1) for s, r, o in pos.tolist()]).astype(np.int32)
    assert abs(esr.term(codes, w_rel, pos, 0.8)["loss"]) > 0            # (the plain term of this fixture is not zero)
    ref = esr.term(codes, w_rel, pos, 0.8, known=known)
    assert ref["loss"] == 0 and not ref["G"].any()
    out = stand_alone(native, codes, w_rel, pos, R, 0.8, known=known)
    assert out["runs"][0][0] == out["base"][0]
    np.testing.assert_array_equal(out["runs"][0][1], out["base"][1])
    np.testing.assert_array_equal(out["runs"][0][2], out["base"][2])
    assert not out["G"][:2 * P].any() and not out["dQ"][:2 * P].any()


def test_hub_entity_and_hub_relation_on_both_sides_of_the_long_row_cut(native):
    V, R, dc, P = 90, 18, 8, 150
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed=21, hub_entity=(4, 100), hub_relation=(3, 140))
    cut = native.entity_softmax_plan(P, V, dc)["long_row"]
    a, r, _, _ = esr.rows_of(pos)
    by_entity, by_relation = np.sort(np.bincount(a, minlength=V)), np.sort(np.bincount(r, minlength=R))
    assert np.bincount(a, minlength=V)[4] == by_entity[-1] > cut and 0 < by_entity[-2] <= cut
    assert np.bincount(r, minlength=R)[3] == by_relation[-1] >= 2 * P - 20 and 0 < by_relation[-2] <= cut
    out = stand_alone(native, codes, w_rel, pos, R, 0.8)
    check_against_mirror(out, codes, w_rel, pos, 0.8, name="hubs")


def test_chunked_call_matches_one_chunk_and_repeats_bitwise(native):
    V, R, dc, P = 90, 18, 8, 100
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed=31)
    # 200 rows in chunks of 70: [0, 70) and [70, 140) and the partial [140, 200); row 70 is an object row, row 139 a subject
    # row, and the object row of positive 50 (row 50, chunk 0) is a chunk away from its subject row (row 150, chunk 2)
    assert native.entity_softmax_plan(35, V, dc)["chunk"] == 70
    chunked = stand_alone(native, codes, w_rel, pos, R, 0.8, reserve=35, repeat=3)
    whole = stand_alone(native, codes, w_rel, pos, R, 0.8)
    assert whole["plan"]["chunk"] == 200
    check_against_mirror(chunked, codes, w_rel, pos, 0.8, name="chunked")
    assert abs(chunked["runs"][0][0] - whole["runs"][0][0]) <= 2e-5 * max(1.0, abs(whole["runs"][0][0]))
    assert_close(chunked["dW"], whole["dW"], rel=2e-4, name="chunked against whole dW")
    assert_close(chunked["dcodes"], whole["dcodes"], rel=2e-4, name="chunked against whole dcodes")
    a = chunked["runs"][0]
    for b in chunked["runs"][1:]:
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
    t = esr.term(codes, c["params"]["W_relation"], pos, weight)
    assert abs(t["loss"]) > 0 and np.abs(t["dcodes"]).max() > 0 and np.abs(t["dW"]).max() > 0
    g64 = helpers.float64_grads_at(dict(V=c["V"], R=c["R"], d=c["d"], L=c["L"], kind=c["kind"], nb=c["nb"],
                                        params=c["params"], triples=triples, masks=masks, dcodes=dcodes + t["dcodes"]), acts)
    g64["W_relation"] = dW + t["dW"]
    return dloss + t["loss"], g64


def check_step(c, loss, grads, want, g64, name):
    # every parameter with a gradient: the per-layer biases of these two kinds are created and never read (their gradient
    # is all zeros), the exclusion tests/test_gpu_train_step.py makes with the same expression; they are checked to be zero
    names = [n for n in oracle.weight_names(c["kind"], c["L"]) if not (n.startswith("b") and n != "b_emb")]
    print("%s: loss %.9g, mirror %.9g" % (name, loss, want))
    assert_close(np.array([loss]), np.array([want]), rel=1e-3, name="loss")
    for n in names:
        assert np.abs(g64[n]).max() > 0, n
        assert_close(grads[n], g64[n], rel=1e-3, name="grad " + n)
    for n in grads:
        assert n in names or not grads[n].any(), n


@pytest.mark.parametrize("kind,nb", [("block", 4), ("basis", 2)])
def test_train_step_device_with_the_term(native, kind, nb):
    c = step_case(kind, nb)
    with native.Engine(c["V"], c["R"], c["d"], c["L"], kind, nb, keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(c["X"]))
        eng.entity_softmax_reserve(c["P"])
        eng.set_entity_softmax(0.7, c["P"])
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"])
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        loss, grads = eng.loss(), eng.get_grads()
        acts = [eng.activation(l) for l in range(c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
        for b in (td, xd, yd):
            b.free()
    want, g64 = mirror_step(c, acts, masks, c["X"], c["Y"], c["pos"], c["triples"], 0.7)
    check_step(c, loss, grads, want, g64, kind)


@pytest.mark.parametrize("kind,nb,limit", [("block", 4, 0), ("basis", 2, 0), ("block", 4, 77)],
                         ids=["block", "basis", "block-leading-77"])
def test_train_step_minibatch_device_with_the_term(native, kind, nb, limit):
    c = step_case(kind, nb)
    n, rate, keep = 200, 2, 120
    batch = np.unique(c["triples"], axis=0)[:n].astype(np.int32)
    assert len(batch) == n
    N = n * (rate + 1)
    with native.Engine(c["V"], c["R"], c["d"], c["L"], kind, nb, keep_prob=0.8, max_edges=n) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(N)
        eng.entity_softmax_reserve(n)
        eng.set_entity_softmax(0.7, limit)                 # num_positives 0: the minibatch step only, all its batch rows
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        eng.train_step_minibatch_device(bd, n, keep, 41, rate, 91, xd, yd, seed=8, reg_param=REG)
        loss, grads = eng.loss(), eng.get_grads()
        acts = [eng.activation(l) for l in range(c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
        graph = eng.graph_edges()
        X, Y = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        if limit == 0:
            # an X/Y step under "the minibatch step only" is refused, and the context goes on
            assert status_of(native, eng.train_step_device, bd, n, xd, yd, N, seed=9, reg_param=REG) == STATE
        eng.set_entity_softmax(0.0)
        eng.train_step_device(bd, n, xd, yd, N, seed=9, reg_param=REG)
        assert np.isfinite(eng.loss())
        for b in (bd, xd, yd):
            b.free()
    np.testing.assert_array_equal(X[:n], batch)
    want, g64 = mirror_step(c, acts, masks, X, Y, batch[:limit] if limit else batch, graph, 0.7)
    check_step(c, loss, grads, want, g64, "%s minibatch" % kind)


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
                eng.entity_softmax_reserve(c["P"])
                eng.set_entity_softmax(0.7, c["P"])
                eng.set_entity_softmax(0.0, c["P"])
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
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed=41)
    X, Y = decoder_batch(pos, V, 7)
    with native.Engine(V, R, dc, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
        eng.decoder_reserve(len(X))
        eng.entity_softmax_reserve(P)
        eng.set_entity_softmax(0.5, P)
        xd, yd = eng.to_device(X), eng.to_device(Y)
        eng.train_step_device(None, 0, xd, yd, len(X), seed=2, reg_param=REG)
        loss, grads = eng.loss(), eng.get_grads()
        for b in (xd, yd):
            b.free()
    dloss, dcodes, dW = rsr.decoder(codes, w_rel, X, Y, REG)
    t = esr.term(codes, w_rel, pos, 0.5)
    assert abs(loss - (dloss + t["loss"])) <= 2e-5 * max(1.0, abs(dloss + t["loss"]))
    assert abs(t["loss"]) > 1e-3
    assert_close(grads["W_emb"], dcodes + t["dcodes"], rel=1e-3, name="W_emb")
    assert_close(grads["W_relation"], dW + t["dW"], rel=1e-3, name="W_relation")


def test_the_terms_add_with_the_relation_softmax_and_adversarial_weights(native):
    """RelationSoftmaxWeight, AdversarialTemperature and the entity term in one step: the sum of the three mirrors"""
    V, R, dc, P, K = 90, 18, 8, 70, 2
    codes, w_rel = adv.tables(V, R, dc, 61)
    X, Y = adv.batch("entity", V, R, P, K, 62)
    pos = X[:P]
    with native.Engine(V, R, dc, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
        eng.decoder_reserve(len(X))
        eng.entity_softmax_reserve(P)
        eng.relation_softmax_reserve(P)
        eng.set_entity_softmax(0.5, P)
        eng.set_relation_softmax(0.6, P)
        eng.set_adversarial_negatives(adv.ALPHA, P)
        xd, yd = eng.to_device(X), eng.to_device(Y)
        eng.train_step_device(None, 0, xd, yd, len(X), seed=2, reg_param=REG)
        loss, grads = eng.loss(), eng.get_grads()
        for b in (xd, yd):
            b.free()
    ref = adv.adversarial_decoder(codes, w_rel, X, Y, P, adv.ALPHA, REG)
    plain = rsr.decoder(codes, w_rel, X, Y, REG)[0]
    rel = rsr.term(codes, w_rel, pos, R, 0.6)
    ent = esr.term(codes, w_rel, pos, 0.5)
    assert abs(ref["loss"] - plain) > 1e-3 and abs(rel["loss"]) > 1e-3 and abs(ent["loss"]) > 1e-3      # each term counts
    want = ref["loss"] + rel["loss"] + ent["loss"]
    print("loss %.9g, mirrors %.9g + %.9g + %.9g" % (loss, ref["loss"], rel["loss"], ent["loss"]))
    assert abs(loss - want) <= 2e-5 * max(1.0, abs(want))
    dW = ref["dW"] + ent["dW"]
    dW[:R] += rel["dW"]
    assert_close(grads["W_emb"], ref["dcodes"] + rel["dcodes"] + ent["dcodes"], rel=1e-3, name="W_emb")
    assert_close(grads["W_relation"], dW, rel=1e-3, name="W_relation")


# ------------------------------------------------------------------ argument checks
def test_refusals_leave_the_context_usable(native):
    V, R, dc, P = 60, 9, 8, 40
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed=51)
    X, Y = decoder_batch(pos, V, 8)
    with native.Engine(V, R, dc, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
        eng.decoder_reserve(len(X))
        xd, yd, pd = eng.to_device(X), eng.to_device(Y), eng.to_device(pos)

        def good_call():
            """a successful call on the same context: the term of the good batch is the mirror's"""
            eng.decoder_loss_backward_device(xd, yd, len(X), REG)
            base = eng.loss()
            eng.decoder_loss_backward_device(xd, yd, len(X), REG)
            eng.entity_softmax_device(pd, P, 0.5)
            t = esr.term(codes, w_rel, pos, 0.5)["loss"]
            assert abs(t) > 1e-3 and abs(eng.loss() - base - t) <= 2e-5 * max(1.0, abs(base + t))

        assert status_of(native, eng.read_buffer, native.BUF_ENTITY_SOFTMAX_G) == STATE
        assert status_of(native, eng.entity_softmax_reserve, 0) == INVALID
        eng.forward(train=True, seed=1)
        eng.decoder_loss_backward_device(xd, yd, len(X), REG)
        assert status_of(native, eng.entity_softmax_device, pd, P, 0.5) == STATE          # before the reserve
        eng.entity_softmax_reserve(P)
        good_call()
        for bad in (-1.0, float("nan"), float("inf")):
            assert status_of(native, eng.entity_softmax_device, pd, P, bad) == INVALID
            assert status_of(native, eng.set_entity_softmax, bad, P) == INVALID
            good_call()
        assert status_of(native, eng.entity_softmax_device, pd, 0, 0.5) == INVALID        # P <= 0
        good_call()
        assert eng.lib.rgcn_entity_softmax_device(eng.ctx, None, P, native.C.c_float(0.5), 0) == INVALID     # NULL positives
        good_call()
        assert status_of(native, eng.set_entity_softmax, 0.5, -1) == INVALID
        assert status_of(native, eng.entity_softmax_device, pd, P, 0.5, exclusive=True) == STATE    # no index
        good_call()
        assert status_of(native, eng.set_entity_softmax, 0.5, P, exclusive=True) == STATE
        good_call()
        # an id out of range fails through the error flag at the next synchronising call; nothing faults
        for col, value in ((0, V), (1, R), (2, -1)):
            wrong = pos.copy()
            wrong[7, col] = value
            wd = eng.to_device(wrong)
            eng.decoder_loss_backward_device(xd, yd, len(X), REG)
            eng.entity_softmax_device(wd, P, 0.5)
            assert status_of(native, eng.loss) == INVALID
            G = eng.read_buffer(native.BUF_ENTITY_SOFTMAX_G)
            assert not G[7].any() and not G[P + 7].any() and G[6].any()                   # zero rows for the bad positive
            wd.free()
            good_call()
        # a leading row with label 0 in an X/Y step
        eng.set_entity_softmax(0.5, P + 1)
        eng.train_step_device(None, 0, xd, yd, len(X), seed=2, reg_param=REG)
        assert status_of(native, eng.loss) == INVALID
        eng.set_entity_softmax(0.5, len(X) + 1)
        assert status_of(native, eng.train_step_device, None, 0, xd, yd, len(X), seed=2, reg_param=REG) == INVALID
        eng.set_entity_softmax(0.5, 0)
        assert status_of(native, eng.train_step_device, None, 0, xd, yd, len(X), seed=2, reg_param=REG) == STATE
        eng.set_entity_softmax(0.0)
        eng.forward(train=True, seed=1)
        good_call()
        for b in (xd, yd, pd):
            b.free()
    # without a decoder pass
    with native.Engine(V, R, dc, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
        eng.decoder_reserve(len(X))
        eng.entity_softmax_reserve(P)
        xd, yd, pd = eng.to_device(X), eng.to_device(Y), eng.to_device(pos)
        eng.forward(train=True, seed=1)
        assert status_of(native, eng.entity_softmax_device, pd, P, 0.5) == STATE
        eng.decoder_loss_backward_device(xd, yd, len(X), REG)
        eng.entity_softmax_device(pd, P, 0.5)
        assert np.isfinite(eng.loss())
        for b in (xd, yd, pd):
            b.free()
    # a relation-sharded context: the setter succeeds, both fused steps and the stand-alone call are refused while the
    # term is on (ahead of the check for a communicator, which this context does not have), and with the weight back at 0
    # the step's refusal is the communicator's again
    with native.Engine(V, R, 8, 1, "block", 2, max_edges=P, rank=0, world=2) as sharded:
        sharded.decoder_reserve(len(X))
        sharded.entity_softmax_reserve(P)
        xd, yd, pd = sharded.to_device(X), sharded.to_device(Y), sharded.to_device(pos)
        sharded.set_entity_softmax(0.5, P)
        assert status_of(native, sharded.train_step_device, pd, P, xd, yd, len(X), seed=2, reg_param=REG) == UNSUPPORTED
        assert status_of(native, sharded.train_step_minibatch_device, pd, P, P // 2, 3, 1, 4, xd, yd, seed=2,
                         reg_param=REG) == UNSUPPORTED
        assert status_of(native, sharded.entity_softmax_device, pd, P, 0.5) == UNSUPPORTED
        sharded.set_entity_softmax(0.0, P)
        assert status_of(native, sharded.train_step_device, pd, P, xd, yd, len(X), seed=2, reg_param=REG) == STATE
        for b in (xd, yd, pd):
            b.free()
    with native.Engine(1, 1, dc, 0, "embedding", 1) as eng:                 # one entity: nothing to tell apart
        assert status_of(native, eng.entity_softmax_reserve, P) == INVALID
        assert status_of(native, eng.set_entity_softmax, 0.5, P) == INVALID
        eng.set_entity_softmax(0.0, P)


def test_capture_and_step_state_rules(native):
    c = step_case("block", 4)
    with native.Engine(c["V"], c["R"], c["d"], c["L"], "block", 4, keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(c["X"]))
        td, xd, yd, pd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"]), eng.to_device(c["pos"])
        eng.set_entity_softmax(0.7, c["P"])
        # the step needs the reserve
        assert status_of(native, eng.train_step_device, td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG) == STATE
        eng.entity_softmax_reserve(c["P"])
        eng.set_entity_softmax(0.0)
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        eng.capture_begin()
        assert status_of(native, eng.set_entity_softmax, 0.7, c["P"]) == STATE
        assert status_of(native, eng.entity_softmax_device, pd, c["P"], 0.7) == STATE
        assert status_of(native, eng.entity_softmax_reserve, 2 * c["P"]) == STATE
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        gid = eng.capture_end()
        eng.graph_launch(gid)
        eng.sync()
        eng.graph_destroy(gid)
        eng.set_entity_softmax(0.7, c["P"])
        eng.train_step_device(td, c["E"], xd, yd, len(c["X"]), seed=60, reg_param=REG)
        assert np.isfinite(eng.loss())
        for b in (td, xd, yd, pd):
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


DRIVER_CASES = [(p, i, v) for p in sorted(DRIVER_PATHS) for i in (1, 2) for v in ("plain", "masked", "leading-100")]


@pytest.mark.parametrize("path,iterations,variant", DRIVER_CASES, ids=["%s-%d-%s" % c for c in DRIVER_CASES])
def test_train_driver_with_the_term(tmp_path, capsys, path, iterations, variant):
    """[Decoder] EntitySoftmaxWeight=0.5 through `train` on the toy dataset of tests/test_gpu_driver.py, on each of the four
    paths.  One iteration: the FIRST loss the driver reports ("Initial loss") is the device's and equals decoder mirror +
    term mirror on the batch that step trained on, read back from the device where the device drew it.  Two iterations:
    the same for the last step.  The learning rate is 1e-30, so the weights read back afterwards are the ones the step saw
    (assert_weights_did_not_move).  masked: ExclusiveNegativeSampling=Yes, the training set is the term's mask.
    leading-100: EntitySoftmaxPositives=100, a third of the batch."""
    from relationprediction_amd import train
    from test_gpu_driver import SETTINGS, write_dataset
    exclusive, limit = variant == "masked", 100 if variant == "leading-100" else 0
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    os.makedirs(str(tmp_path / "models"))
    settings = tmp_path / "toy.exp"
    keys = "RegularizationParameter=0.01\n\tEntitySoftmaxWeight=0.5" + ("\n\tEntitySoftmaxPositives=%d" % limit if limit else "")
    text = ((SETTINGS % dict(nb=4, concat="Yes", exp=str(tmp_path / "models" / "Toy")))
            .replace("RegularizationParameter=0.01", keys)
            .replace("learning_rate=0.01", "learning_rate=1e-30"))
    if exclusive:
        text = text.replace("GraphBatchSize=300", "GraphBatchSize=300\n\tExclusiveNegativeSampling=Yes")
    settings.write_text(text)
    np.random.seed(0)
    model, done = train.main(["--settings", str(settings), "--dataset", data, "--max-iterations", str(iterations)]
                             + DRIVER_PATHS[path])
    out = capsys.readouterr().out
    assert done == iterations and model.entity_softmax_weight == 0.5 and model.entity_softmax_positives == limit
    assert (model.relation_softmax_known is not None) == exclusive
    rt = model.get_runtime()
    eng = rt.engine
    n, N = 300, 300 * 6
    taken = limit or n
    assert rt._entsm_state == (0.5, taken, exclusive) and rt._entsm_reserved >= taken
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
    t = esr.term(codes, w_rel, X[:taken], 0.5, known=train_triples if exclusive else None)
    print("%s: loss %.9g, decoder mirror %.9g + term mirror %.9g" % (path, loss, dloss, t["loss"]))
    assert abs(t["loss"]) > 0.1
    if exclusive:              # (whether a query of the batch has a second training answer is the toy dataset's affair:
        #                        test_masked_term_matches_float64 is where the mask is made to matter)
        plain = esr.term(codes, w_rel, X[:taken], 0.5)["loss"]
        print("masked %.9g, plain %.9g, rows that mask something %d" % (t["loss"], plain, int((~t["mask"]).any(axis=1).sum())))
    assert abs(loss - (dloss + t["loss"])) <= 2e-5 * max(1.0, abs(dloss + t["loss"]))
