"""Self-adversarial negative weights on the GPU (csrc/adversarial.hip, the weighted kernels of csrc/decoder.hip;
include/rgcn.h rgcn_adversarial_weights_device, rgcn_decoder_loss_backward_weighted_device,
rgcn_set_adversarial_negatives) against the float64 mirror of tests/adversarial_reference.py.

Bounds.  A weight: the derived tolerance of the mirror, (exp(2 alpha B) - 1) w + 4 ulp(w) + 1e-37 with B the forward error
bound of a float32 energy (the maximum over the group).  The weighted decoder: the loss within 2e-5 x max(1, |loss|),
dW_relation and dcodes within helpers.assert_close(rel=2e-4) -- what tests/test_gpu_train_step.py and
tests/test_gpu_embedding.py hold the decoder to; full steps within assert_close(rel=1e-3), that file's bound for them.
The inputs of every weight case are checked on the host (tests/test_adversarial_host.py): the mirror's weights lie on
both sides of 1 wherever a case claims to test weighting."""
import os

import numpy as np
import pytest

import adversarial_reference as adv
import helpers
import oracle
import relation_softmax_reference as rsr
from helpers import assert_close

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = 1, 4, 5        # RGCN_ERR_*
REG = 0.01
ALPHA = 1.5


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def status_of(native, call, *args, **kw):
    with pytest.raises(native.RgcnError) as e:
        call(*args, **kw)
    return e.value.status


def embedding_engine(native, codes, w_rel, R=adv.R_CASE):
    V, dc = codes.shape
    eng = native.Engine(V, R, dc, 0, "embedding", 1)
    eng.set_params({"W_emb": codes, "b_emb": np.zeros(dc, np.float32), "W_relation": w_rel})
    return eng


def device_weights(native, c, repeat=1):
    """the weights of case c from an embedding context (the codes are W_emb), `repeat` times"""
    N = len(c["X"])
    runs = []
    with embedding_engine(native, c["codes"], c["w_rel"]) as eng:
        eng.forward(train=True, seed=1)
        wd = eng.alloc(4 * N)
        if "batch" in c:                                  # the device sampler's own rows, relation rows included
            bd, xd, yd = eng.to_device(c["batch"]), eng.alloc(12 * N), eng.alloc(4 * N)
            eng.negative_sample_device(bd, len(c["batch"]), c["rate"], c["seed"], xd, yd, relation_rate=c["m"])
            np.testing.assert_array_equal(xd.download(np.int32, (N, 3)), c["X"])
            bufs = (bd, xd, yd)
        else:
            xd = eng.to_device(c["X"])
            bufs = (xd,)
        for _ in range(repeat):
            wd.upload(np.full(N, -7.0, np.float32))       # (nothing of an earlier call survives)
            eng.adversarial_weights(xd, N, c["P"], c["alpha"], wd)
            runs.append(wd.download(np.float32, (N,)))
        for b in bufs + (wd,):
            b.free()
    return runs


def check_weights(c, got, name=""):
    ref = adv.weights(c["codes"], c["w_rel"], c["X"], c["P"], c["alpha"])
    err = np.abs(got.astype(np.float64) - ref["w"])
    print("%s: weights %.4g .. %.4g, worst error %.3g at a tolerance of %.3g"
          % (name, got.min(), got.max(), err.max(), ref["tol"][int(np.argmax(err))]))
    assert np.isfinite(got).all() and (got >= 0).all(), name
    assert (got[:c["P"]] == 1.0).all(), name
    assert (err <= ref["tol"]).all(), (name, float((err - ref["tol"]).max()))
    return ref


@pytest.mark.parametrize("name", adv.WEIGHT_CASE_NAMES)
def test_weights_match_float64(native, name):
    c = adv.weight_case(name)
    a, b = device_weights(native, c, repeat=2)
    np.testing.assert_array_equal(a, b)                   # two calls, the same bytes
    check_weights(c, a, name)
    if not c["spreads"]:                                  # K = 1, and negatives identical to their positive
        assert (a == 1.0).all()
    else:
        assert a[c["P"]:].max() >= 1.5 - 0.1 and a[c["P"]:].min() <= 0.5 + 0.1


def test_weights_of_the_device_samplers_rows(native):
    """entity corruptions and relation rows as rgcn_negative_sample_relation_device writes them (m = 2)"""
    c = adv.relation_rows_case()
    first = c["P"] * (c["rate"] + 1)
    assert (c["X"][first:, 1] != np.tile(c["batch"][:, 1], c["m"])).all()      # the relation rows replace r
    (got,) = device_weights(native, c)
    check_weights(c, got, "relation rows")


def test_a_dominating_negative_takes_its_group(native):
    c = adv.dominating_case()
    (got,) = device_weights(native, c)
    check_weights(c, got, "dominating")
    P, K = c["P"], c["K"]
    group = got[P:].reshape(K, P)[:, 1]
    assert abs(got[c["big"]] - K) <= 1e-2 and not np.delete(group, 3).any()


def test_temperature_zero_and_no_negatives_give_ones(native):
    c = adv.weight_case("dc8")
    c0 = dict(c, alpha=0.0)
    (got,) = device_weights(native, c0)
    assert (got == 1.0).all()
    only = dict(c, X=c["X"][:c["P"]], Y=c["Y"][:c["P"]], K=0)
    (got,) = device_weights(native, only)
    assert got.shape == (c["P"],) and (got == 1.0).all()


def test_an_id_out_of_range_reads_nothing_and_weighs_nothing(native):
    c = adv.weight_case("dc8")
    P, K = c["P"], c["K"]
    X = c["X"].copy()
    X[P + 2] = (adv.V_CASE, 0, 1)                         # negative 0 of positive 2
    X[P + P + 2] = (3, -1, 1)                             # negative 1 of positive 2
    X[P + 3 * P + 4] = (3, 0, 2 ** 30)                    # negative 3 of positive 4
    bad = dict(c, X=X)
    (got,) = device_weights(native, bad)
    for i in (P + 2, 2 * P + 2, 4 * P + 4):
        assert got[i] == 0.0
    # the rest of such a group is the softmax over the rows that take part, scaled by K; the other groups are untouched
    ref = adv.weights(c["codes"], c["w_rel"], c["X"], P, c["alpha"])
    for b in (0, 1, 3):
        idx = P + b + P * np.arange(K)
        assert (np.abs(got[idx] - ref["w"][idx]) <= ref["tol"][idx]).all()
    for b, out in ((2, [0, 1]), (4, [3])):
        idx = P + b + P * np.delete(np.arange(K), out)
        x = ref["x"][idx]
        t = np.exp(1.5 * (x - x.max()))
        assert np.allclose(got[idx], K * t / t.sum(), rtol=1e-3, atol=1e-6)
        assert abs(got[P + b + P * np.arange(K)].sum() - K) < 1e-3


# ------------------------------------------------------------------ the weighted decoder
def decoder_runs(native, c, weights):
    """(loss, dcodes, dW_relation) of the weighted decoder for each entry of `weights` (None: the NULL pointer; "plain":
    rgcn_decoder_loss_backward_device itself)"""
    N = len(c["X"])
    out = []
    with embedding_engine(native, c["codes"], c["w_rel"]) as eng:
        eng.decoder_reserve(N)
        eng.forward(train=True, seed=1)
        xd, yd = eng.to_device(c["X"]), eng.to_device(c["Y"])
        for w in weights:
            if isinstance(w, str):
                eng.decoder_loss_backward_device(xd, yd, N, REG)
            else:
                wd = eng.to_device(w) if w is not None else None
                eng.decoder_loss_backward_weighted_device(xd, yd, wd, N, REG)
            out.append((eng.loss(), eng.dcodes(), eng.get_grad("W_relation")))
            if not isinstance(w, str) and w is not None:
                wd.free()
        for b in (xd, yd):
            b.free()
    return out


@pytest.mark.parametrize("dc", [6, 8, 516, 1028])
def test_weighted_decoder_matches_float64(native, dc):
    """caller's weights in [0, 3] with exact zeros: the fused energy kernel (dc 6, 8, 516) and the unfused one (1028)"""
    c = adv.decoder_case(dc)
    assert (c["w"] == 0).sum() >= 20 and c["w"].max() > 2.5 and 0 < c["Y"].sum() < len(c["Y"])
    (loss, dcodes, dW), = decoder_runs(native, c, [c["w"]])
    ref = adv.weighted_decoder(c["codes"], c["w_rel"], c["X"], c["Y"], c["w"], REG)
    plain = adv.weighted_decoder(c["codes"], c["w_rel"], c["X"], c["Y"], np.ones(len(c["w"])), REG)
    assert abs(ref["loss"] - plain["loss"]) > 1e-2        # the weights matter on this batch
    print("dc %d: loss %.9g, mirror %.9g (unweighted %.9g)" % (dc, loss, ref["loss"], plain["loss"]))
    assert abs(loss - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"]))
    assert_close(dW, ref["dW"], rel=2e-4, name="dW_relation")
    assert_close(dcodes, ref["dcodes"], rel=2e-4, name="dcodes")


@pytest.mark.parametrize("dc", [6, 8, 516, 1028])
def test_null_and_unit_weights_reproduce_the_unweighted_bytes(native, dc):
    c = adv.decoder_case(dc)
    plain, null, ones = decoder_runs(native, c, ["plain", None, np.ones(len(c["X"]), np.float32)])
    for got in (null, ones):
        assert got[0] == plain[0]
        np.testing.assert_array_equal(got[1], plain[1])
        np.testing.assert_array_equal(got[2], plain[2])


def test_a_bad_weight_is_refused_at_the_next_synchronising_call(native):
    c = adv.decoder_case(8)
    N = len(c["X"])
    with embedding_engine(native, c["codes"], c["w_rel"]) as eng:
        eng.decoder_reserve(N)
        eng.forward(train=True, seed=1)
        xd, yd = eng.to_device(c["X"]), eng.to_device(c["Y"])
        for value in (-0.5, float("nan"), float("inf")):
            w = c["w"].copy()
            w[17] = value
            wd = eng.to_device(w)
            eng.decoder_loss_backward_weighted_device(xd, yd, wd, N, REG)
            assert status_of(native, eng.loss) == INVALID
            wd.free()
        wd = eng.to_device(c["w"])
        eng.decoder_loss_backward_weighted_device(xd, yd, wd, N, REG)      # the context goes on
        ref = adv.weighted_decoder(c["codes"], c["w_rel"], c["X"], c["Y"], c["w"], REG)
        assert abs(eng.loss() - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"]))
        for b in (xd, yd, wd):
            b.free()


# ------------------------------------------------------------------ fused steps
def step_case(kind, nb, K=2):
    V, R, d, L, E, P = 80, 8, 20, 2, 300, 130
    params, triples, _, _ = helpers.make_case(V, R, d, L, kind, nb, E, seed=77)
    params["W_relation"] = (params["W_relation"] * 0.1).astype(np.float32)      # energies of unit order on these codes
    X, Y = adv.batch("entity", V, R, P, K, 6)
    return dict(V=V, R=R, d=d, L=L, E=E, P=P, K=K, kind=kind, nb=nb, params=params, triples=triples, X=X, Y=Y)


def mirror_step(c, acts, masks, X, Y, P, triples, alpha, relsm=0.0):
    """weights and weighted decoder of the mirror on the engine's own codes, pushed through the float64 encoder"""
    codes = acts[-1]
    ref = adv.adversarial_decoder(codes, c["params"]["W_relation"], X, Y, P, alpha, REG)
    loss, dcodes, dW = ref["loss"], ref["dcodes"], ref["dW"]
    if relsm > 0:
        t = rsr.term(codes, c["params"]["W_relation"], X[:P], c["R"], relsm)
        loss, dcodes = loss + t["loss"], dcodes + t["dcodes"]
        dW[:c["R"]] += t["dW"]
    g64 = helpers.float64_grads_at(dict(V=c["V"], R=c["R"], d=c["d"], L=c["L"], kind=c["kind"], nb=c["nb"],
                                        params=c["params"], triples=triples, masks=masks, dcodes=dcodes), acts)
    g64["W_relation"] = dW
    return loss, g64, ref


def check_step(c, loss, grads, weights, want, g64, ref, name):
    # (the unread per-layer biases: the exclusion tests/test_gpu_train_step.py makes with the same expression)
    names = [n for n in oracle.weight_names(c["kind"], c["L"]) if not (n.startswith("b") and n != "b_emb")]
    neg = ref["w"][len(ref["w"]) // (c["K"] + 1):]
    print("%s: loss %.9g, mirror %.9g; mirror weights %.3g .. %.3g" % (name, loss, want, neg.min(), neg.max()))
    assert neg.max() >= 1.5 and neg.min() <= 0.5, name               # the step weighs: ones would not pass
    assert (np.abs(weights.astype(np.float64) - ref["w"]) <= ref["tol"]).all(), name
    assert_close(np.array([loss]), np.array([want]), rel=1e-3, name=name + " loss")
    for n in names:
        assert np.abs(g64[n]).max() > 0, n
        assert_close(grads[n], g64[n], rel=1e-3, name=name + " grad " + n)
    for n in grads:
        assert n in names or not grads[n].any(), n


@pytest.mark.parametrize("kind,nb", [("block", 4), ("basis", 2)])
def test_train_step_device_under_the_mode(native, kind, nb):
    c = step_case(kind, nb)
    N = len(c["X"])
    with native.Engine(c["V"], c["R"], c["d"], c["L"], kind, nb, keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(N)
        eng.set_adversarial_negatives(ALPHA, c["P"])
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"])
        runs = []
        for _ in range(2):
            eng.train_step_device(td, c["E"], xd, yd, N, seed=60, reg_param=REG)
            runs.append((eng.loss(), eng.get_grads(), eng.read_buffer(native.BUF_ADVERSARIAL_WEIGHTS)))
        acts = [eng.activation(l) for l in range(c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
        for b in (td, xd, yd):
            b.free()
    (loss, grads, w), again = runs
    assert again[0] == loss                                          # two calls, the same bytes
    np.testing.assert_array_equal(again[2], w)
    for n in grads:
        np.testing.assert_array_equal(again[1][n], grads[n], err_msg=n)
    want, g64, ref = mirror_step(c, acts, masks, c["X"], c["Y"], c["P"], c["triples"], ALPHA)
    plain = adv.weighted_decoder(acts[-1], c["params"]["W_relation"], c["X"], c["Y"], np.ones(N), REG)["loss"]
    assert abs(want - plain) > 3e-3 * abs(want)                      # outside the bound of the unweighted loss
    check_step(c, loss, grads, w, want, g64, ref, kind)


@pytest.mark.parametrize("kind,nb,relation_rate,relsm", [("block", 4, 0, 0.0), ("basis", 2, 0, 0.0), ("block", 4, 2, 0.0),
                                                         ("block", 4, 2, 0.7)],
                         ids=["block", "basis", "block-relation-rows", "block-relation-rows-softmax"])
def test_train_step_minibatch_device_under_the_mode(native, kind, nb, relation_rate, relsm):
    rate = 2
    c = step_case(kind, nb, K=rate + relation_rate)
    n, keep = 200, 120
    batch = np.unique(c["triples"], axis=0)[:n].astype(np.int32)
    assert len(batch) == n
    N = n * (rate + 1 + relation_rate)
    with native.Engine(c["V"], c["R"], c["d"], c["L"], kind, nb, keep_prob=0.8, max_edges=n) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(N)
        eng.set_adversarial_negatives(ALPHA)                          # num_positives 0: the minibatch step only
        if relation_rate:
            eng.set_relation_negatives(relation_rate)
        if relsm > 0:
            eng.relation_softmax_reserve(n)
            eng.set_relation_softmax(relsm)
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        eng.train_step_minibatch_device(bd, n, keep, 41, rate, 91, xd, yd, seed=8, reg_param=REG)
        loss, grads, w = eng.loss(), eng.get_grads(), eng.read_buffer(native.BUF_ADVERSARIAL_WEIGHTS)
        acts = [eng.activation(l) for l in range(c["L"] + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, c["L"] + 1)]
        graph = eng.graph_edges()
        X, Y = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        # an X/Y step under "the minibatch step only" is refused, and the context goes on
        assert status_of(native, eng.train_step_device, bd, n, xd, yd, N, seed=9, reg_param=REG) == STATE
        eng.set_adversarial_negatives(0.0)
        if relsm > 0:
            eng.set_relation_softmax(0.0)                            # (its own "minibatch step only" would refuse too)
        eng.train_step_device(bd, n, xd, yd, N, seed=9, reg_param=REG)
        assert np.isfinite(eng.loss())
        for b in (bd, xd, yd):
            b.free()
    np.testing.assert_array_equal(X[:n], batch)
    assert w.shape == (N,)
    want, g64, ref = mirror_step(c, acts, masks, X, Y, n, graph, ALPHA, relsm=relsm)
    check_step(c, loss, grads, w, want, g64, ref, "%s minibatch" % kind)


def test_embedding_step_under_the_mode(native):
    c = adv.weight_case("P129")
    N = len(c["X"])
    with embedding_engine(native, c["codes"], c["w_rel"]) as eng:
        eng.decoder_reserve(N)
        eng.set_adversarial_negatives(ALPHA, c["P"])
        xd, yd = eng.to_device(c["X"]), eng.to_device(c["Y"])
        eng.train_step_device(None, 0, xd, yd, N, seed=2, reg_param=REG)
        loss, grads, w = eng.loss(), eng.get_grads(), eng.read_buffer(native.BUF_ADVERSARIAL_WEIGHTS)
        for b in (xd, yd):
            b.free()
    ref = adv.adversarial_decoder(c["codes"], c["w_rel"], c["X"], c["Y"], c["P"], ALPHA, REG)
    assert (np.abs(w.astype(np.float64) - ref["w"]) <= ref["tol"]).all()
    assert abs(loss - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"]))
    assert_close(grads["W_emb"], ref["dcodes"], rel=1e-3, name="W_emb")
    assert_close(grads["W_relation"], ref["dW"], rel=1e-3, name="W_relation")


def test_temperature_zero_restores_every_byte(native):
    """a context that ran steps under the mode and switched it off against one that never called the setter: loss,
    gradients and updated weights of both fused steps"""
    c = step_case("block", 4)
    n, rate, keep = 200, 2, 120
    batch = np.unique(c["triples"], axis=0)[:n].astype(np.int32)
    N = n * (rate + 1)
    NX = len(c["X"])
    seen = []
    for touch in (False, True):
        with native.Engine(c["V"], c["R"], c["d"], c["L"], "block", 4, keep_prob=0.8, max_edges=c["E"]) as eng:
            eng.set_params(c["params"])
            eng.decoder_reserve(max(N, NX))
            td, xd, yd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"])
            bd, xs, ys = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
            if touch:                                     # (no optimizer yet: the weights stay what they are)
                eng.set_adversarial_negatives(ALPHA, c["P"])
                eng.train_step_device(td, c["E"], xd, yd, NX, seed=60, reg_param=REG)
                under = eng.loss()
                eng.train_step_minibatch_device(bd, n, keep, 41, rate, 91, xs, ys, seed=8, reg_param=REG)
                eng.set_adversarial_negatives(0.0, c["P"])
            eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
            got = []
            eng.train_step_device(td, c["E"], xd, yd, NX, seed=60, reg_param=REG)
            got.append((eng.loss(), eng.get_grads(), eng.get_params()))
            eng.train_step_minibatch_device(bd, n, keep, 41, rate, 91, xs, ys, seed=8, reg_param=REG)
            got.append((eng.loss(), eng.get_grads(), eng.get_params()))
            seen.append(got)
            for b in (td, xd, yd, bd, xs, ys):
                b.free()
    assert under != seen[0][0][0]                         # the mode did change the first step's loss
    for a, b in zip(*seen):
        assert a[0] == b[0]
        for k in a[1]:
            np.testing.assert_array_equal(a[1][k], b[1][k], err_msg="grad " + k)
            np.testing.assert_array_equal(a[2][k], b[2][k], err_msg="weight " + k)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(native):
    c = adv.weight_case("dc8")
    N, P = len(c["X"]), c["P"]
    with embedding_engine(native, c["codes"], c["w_rel"]) as eng:
        eng.decoder_reserve(N)
        xd, yd, wd = eng.to_device(c["X"]), eng.to_device(c["Y"]), eng.alloc(4 * N)
        assert status_of(native, eng.adversarial_weights, xd, N, P, ALPHA, wd) == STATE          # before a forward pass
        assert status_of(native, eng.read_buffer, native.BUF_ADVERSARIAL_WEIGHTS) == STATE
        eng.forward(train=True, seed=1)
        assert status_of(native, eng.adversarial_weights, xd, N, P + 1, ALPHA, wd) == INVALID    # N % P != 0
        assert status_of(native, eng.adversarial_weights, xd, N, 0, ALPHA, wd) == INVALID
        assert status_of(native, eng.adversarial_weights, xd, N, -P, ALPHA, wd) == INVALID
        assert status_of(native, eng.adversarial_weights, xd, 0, P, ALPHA, wd) == INVALID
        assert status_of(native, eng.adversarial_weights, None, N, P, ALPHA, wd) == INVALID      # a NULL pointer
        assert status_of(native, eng.adversarial_weights, xd, N, P, ALPHA, None) == INVALID
        for bad in (-1.0, float("nan"), float("inf")):
            assert status_of(native, eng.adversarial_weights, xd, N, P, bad, wd) == INVALID
            assert status_of(native, eng.set_adversarial_negatives, bad, P) == INVALID
        assert status_of(native, eng.set_adversarial_negatives, ALPHA, -1) == INVALID
        # the fused step: positives that do not divide N, "the minibatch step only"
        eng.set_adversarial_negatives(ALPHA, P + 1)
        assert status_of(native, eng.train_step_device, None, 0, xd, yd, N, seed=2, reg_param=REG) == INVALID
        eng.set_adversarial_negatives(ALPHA, 0)
        assert status_of(native, eng.train_step_device, None, 0, xd, yd, N, seed=2, reg_param=REG) == STATE
        # a label of 1 among the negatives, a label of 0 among the positives: the error flag at the next synchronising call
        eng.set_adversarial_negatives(ALPHA, P)
        for row in (P + 3, 1):
            y = c["Y"].copy()
            y[row] = 1.0 - y[row]
            bad = eng.to_device(y)
            eng.train_step_device(None, 0, xd, bad, N, seed=2, reg_param=REG)
            assert status_of(native, eng.loss) == INVALID
            bad.free()
        # the context goes on: the step on the good batch is the mirror's
        eng.train_step_device(None, 0, xd, yd, N, seed=2, reg_param=REG)
        ref = adv.adversarial_decoder(c["codes"], c["w_rel"], c["X"], c["Y"], P, ALPHA, REG)
        assert abs(eng.loss() - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"]))
        eng.adversarial_weights(xd, N, P, ALPHA, wd)
        assert (np.abs(wd.download(np.float32, (N,)) - ref["w"]) <= ref["tol"]).all()
        for b in (xd, yd, wd):
            b.free()
    # a relation-sharded context: the setter succeeds, both fused steps are refused while the mode is on (ahead of the check
    # for a communicator, which this context does not have); with the temperature back at 0 the refusal is the communicator's
    with native.Engine(adv.V_CASE, adv.R_CASE, 8, 1, "block", 2, max_edges=P, rank=0, world=2) as sharded:
        sharded.decoder_reserve(N)
        xd, yd, pd = sharded.to_device(c["X"]), sharded.to_device(c["Y"]), sharded.to_device(c["X"][:P])
        sharded.set_adversarial_negatives(ALPHA, P)
        assert status_of(native, sharded.train_step_device, pd, P, xd, yd, N, seed=2, reg_param=REG) == UNSUPPORTED
        assert status_of(native, sharded.train_step_minibatch_device, pd, P, P // 2, 3, c["K"], 4, xd, yd, seed=2,
                         reg_param=REG) == UNSUPPORTED
        sharded.set_adversarial_negatives(0.0, P)
        assert status_of(native, sharded.train_step_device, pd, P, xd, yd, N, seed=2, reg_param=REG) == STATE
        for b in (xd, yd, pd):
            b.free()


def test_capture_rules(native):
    c = step_case("block", 4)
    N = len(c["X"])
    with native.Engine(c["V"], c["R"], c["d"], c["L"], "block", 4, keep_prob=0.8, max_edges=c["E"]) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(N)
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(c["X"]), eng.to_device(c["Y"])
        eng.train_step_device(td, c["E"], xd, yd, N, seed=60, reg_param=REG)
        eng.capture_begin()
        assert status_of(native, eng.set_adversarial_negatives, ALPHA, c["P"]) == STATE
        eng.train_step_device(td, c["E"], xd, yd, N, seed=60, reg_param=REG)
        gid = eng.capture_end()
        eng.graph_launch(gid)
        eng.sync()
        eng.graph_destroy(gid)
        # the mode switched on ahead of a capture: the step inside it is refused, the capture itself goes on
        eng.set_adversarial_negatives(ALPHA, c["P"])
        eng.capture_begin()
        assert status_of(native, eng.train_step_device, td, c["E"], xd, yd, N, seed=60, reg_param=REG) == STATE
        eng.set_adversarial_negatives(0.0)
        eng.train_step_device(td, c["E"], xd, yd, N, seed=60, reg_param=REG)
        gid = eng.capture_end()
        eng.graph_destroy(gid)
        eng.set_adversarial_negatives(ALPHA, c["P"])
        eng.train_step_device(td, c["E"], xd, yd, N, seed=60, reg_param=REG)
        assert np.isfinite(eng.loss())
        for b in (td, xd, yd):
            b.free()


# ------------------------------------------------------------------ the driver
DRIVER_PATHS = {"device": [], "host_sampler": ["--host-sampler"], "host_dropout": ["--host-edge-dropout"],
                "host_negatives": ["--host-negatives", "--batch-workers", "0"]}


def run_driver(tmp_path, text, extra, iterations):
    from relationprediction_amd import train
    from test_gpu_driver import write_dataset
    data = str(tmp_path / "data")
    write_dataset(data)
    os.makedirs(str(tmp_path / "models"), exist_ok=True)
    settings = tmp_path / "toy.exp"
    settings.write_text(text)
    np.random.seed(0)
    return train.main(["--settings", str(settings), "--dataset", data, "--max-iterations", str(iterations)] + extra)


def toy_settings(tmp_path, temperature=None, exclusive=False, relation_rate=0):
    from test_gpu_driver import SETTINGS
    text = SETTINGS % dict(nb=4, concat="Yes", exp=str(tmp_path / "models" / "Toy"))
    extra = ""
    if temperature is not None:
        extra += "\n\tAdversarialTemperature=%s" % temperature
    if exclusive:
        extra += "\n\tExclusiveNegativeSampling=Yes"
    if relation_rate:
        extra += "\n\tRelationNegativeSampleRate=%d" % relation_rate
    return text.replace("NegativeSampleRate=5", "NegativeSampleRate=5" + extra)


DRIVER_CASES = [(p, False) for p in sorted(DRIVER_PATHS)] + [("device", True), ("host_negatives", True)]


@pytest.mark.parametrize("path,exclusive", DRIVER_CASES, ids=["%s%s" % (p, "-exclusive" if e else "") for p, e in DRIVER_CASES])
def test_train_driver_under_the_mode(tmp_path, capsys, path, exclusive):
    """[General] AdversarialTemperature=1 (with RelationNegativeSampleRate=1) through `train` on the toy dataset of
    tests/test_gpu_driver.py, on each of the four paths: the engine was told, the last step's weights are the mirror's on
    the batch and the codes of that step, read back from the device, they move away from ones, and the losses are finite.
    The learning rate is 1e-30, so W_relation read back afterwards is the one the step saw."""
    text = toy_settings(tmp_path, "1", exclusive, relation_rate=1).replace("learning_rate=0.01", "learning_rate=1e-30")
    model, done = run_driver(tmp_path, text, DRIVER_PATHS[path], 3)
    out = capsys.readouterr().out
    assert done == 3 and model.adversarial_temperature == 1.0
    rt = model.get_runtime()
    eng = rt.engine
    n, K = 300, 6
    N = n * (K + 1)
    assert rt._adv_state == (1.0, n)
    loss = eng.loss()
    initial = float([l for l in out.splitlines() if l.startswith("Initial loss: ")][0].split(": ")[1])
    assert np.isfinite(loss) and np.isfinite(initial)
    w = rt.adversarial_weights()
    assert w.shape == (N,) and (w[:n] == 1.0).all() and np.isfinite(w).all()
    assert abs(float(w.astype(np.float64).sum()) - N) <= 1e-4 * N
    print("%s: loss %.9g, weights %.4g .. %.4g" % (path, loss, w[n:].min(), w[n:].max()))
    assert w[n:].max() > 1.01 and w[n:].min() < 0.99                      # the step weighed its negatives
    X, Y = rt._dev["X"].download(np.int32, (N, 3)), rt._dev["Y"].download(np.float32, (N,))
    assert Y[:n].all() and not Y[n:].any()
    ref = adv.weights(eng.activation(2), eng.get_param("W_relation"), X, n, 1.0)
    assert (np.abs(w.astype(np.float64) - ref["w"]) <= ref["tol"]).all()


def test_train_driver_embedding_under_the_mode(tmp_path, capsys):
    from test_embedding_host import DISTMULT_EXP
    text = (DISTMULT_EXP % 20).replace("models/Distmult", str(tmp_path / "models" / "Distmult")) \
        .replace("NegativeSampleRate=10", "NegativeSampleRate=10\n\tAdversarialTemperature=1")
    model, done = run_driver(tmp_path, text, [], 3)
    assert done == 3 and model.adversarial_temperature == 1.0
    rt = model.get_runtime()
    n = 700
    assert rt._adv_state == (1.0, n)
    w = rt.adversarial_weights()
    assert w.shape == (11 * n,) and (w[:n] == 1.0).all() and np.isfinite(w).all() and np.isfinite(rt.engine.loss())
    assert abs(float(w.astype(np.float64).sum()) - 11 * n) <= 1e-4 * 11 * n
    assert w[n:].max() > 1.0 and w[n:].min() < 1.0


@pytest.mark.parametrize("path", ["device", "host_negatives"])
def test_temperature_zero_in_the_file_trains_to_the_same_bytes(tmp_path, capsys, path):
    """AdversarialTemperature=0 against a file without the key: the same weights after three iterations"""
    seen = []
    for temperature in (None, "0"):
        sub = tmp_path / ("t%s" % temperature)
        sub.mkdir()
        model, done = run_driver(sub, toy_settings(sub, temperature), DRIVER_PATHS[path], 3)
        assert done == 3 and model.adversarial_temperature == 0.0
        eng = model.get_runtime().engine
        seen.append((eng.loss(), {name: eng.get_param(name) for name in eng.param_names}))
    assert seen[0][0] == seen[1][0]
    for name in seen[0][1]:
        np.testing.assert_array_equal(seen[0][1][name], seen[1][1][name], err_msg=name)
