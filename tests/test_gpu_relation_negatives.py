"""The relation corruptions on the device (rgcn_negative_sample_relation_device, rgcn_set_relation_negatives) against the
numpy mirror of tests/relation_negatives_reference.py, bit for bit.  The statistics and the properties are asserted on the
mirror without a GPU (tests/test_relation_negatives_host.py); here the device has to produce the mirror's bytes, the fused
step has to train on them through the decoder's general path, and the driver has to carry the setting and the metric."""
import os

import numpy as np
import pytest

import exclusive_negatives_reference as ent
import helpers
import oracle
import relation_negatives_reference as ref

pytestmark = pytest.mark.gpu

STATUS_INVALID, STATUS_STATE, STATUS_UNSUPPORTED = 1, 4, 5
GUARD = 64


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def _sample(eng, batch, rate, m, seed, exclusive, bufs=None):
    """(X, Y) of one stand-alone call, with GUARD rows behind the output that have to come back untouched"""
    n = len(batch)
    total = n * (rate + 1 + m)
    own = bufs is None
    if own:
        bufs = (eng.to_device(batch), eng.to_device(np.full((total + GUARD, 3), -77, dtype=np.int32)),
                eng.to_device(np.full(total + GUARD, -77, dtype=np.float32)))
    try:
        eng.negative_sample_device(bufs[0], n, rate, seed, bufs[1], bufs[2], exclusive=exclusive, relation_rate=m)
        X, Y = bufs[1].download(np.int32, (total + GUARD, 3)), bufs[2].download(np.float32, (total + GUARD,))
    finally:
        if own:
            for b in bufs:
                b.free()
    assert (X[total:] == -77).all() and (Y[total:] == -77).all()         # nothing written behind the last row
    return X[:total], Y[:total]


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_device_equals_the_mirror(native, name):
    """X, Y and both counters, exclusive and plain; RGCN_BUF_NEGATIVE_UNRESOLVED is what the entity rows alone produce"""
    c = ref.case(name)
    eng = native.Engine(c["V"], c["R"], 8, 1, "block", 2, max_edges=16)
    try:
        eng.known_positives_reserve(c["known"])
        assert eng.negative_unresolved() == 0 and eng.negative_relation_unresolved() == 0
        X, Y = _sample(eng, c["batch"], c["rate"], c["relation_rate"], c["seed"], True)
        assert np.array_equal(X, c["mirror"]["X"]) and np.array_equal(Y, c["mirror"]["Y"])
        assert eng.negative_relation_unresolved() == c["mirror"]["relation"]["unresolved"]
        assert eng.negative_unresolved() == c["mirror"]["entity_unresolved"]
        Xp, Yp = _sample(eng, c["batch"], c["rate"], c["relation_rate"], c["seed"], False)
        assert np.array_equal(Xp, c["plain"]["X"]) and np.array_equal(Yp, c["plain"]["Y"])
        # the plain form counts nothing
        assert eng.negative_relation_unresolved() == c["mirror"]["relation"]["unresolved"]
        assert eng.negative_unresolved() == c["mirror"]["entity_unresolved"]
        if name == "small":
            assert c["mirror"]["relation"]["first_known"].sum() >= 100
        if name == "saturated":
            assert c["mirror"]["relation"]["unresolved"] == 128
            _sample(eng, c["batch"], c["rate"], c["relation_rate"], c["seed"], True)     # a total since the reserve
            assert eng.negative_relation_unresolved() == 256
            eng.known_positives_reserve(c["known"])                                      # ... and a reserve starts it over
            assert eng.negative_relation_unresolved() == 0 and eng.negative_unresolved() == 0
    finally:
        eng.close()


@pytest.fixture(scope="module")
def small():
    V, R, batch, known = ref.small_fixture()
    return dict(V=V, R=R, batch=batch, known=known, keys=ent.build_index(known, V, R))


# (n, rate, m): 255, 256 and 257 relation rows around the 256-thread workgroup; the boundary n (rate + 1) inside a
# wavefront (255 and 257); one batch row; relation rows only
@pytest.mark.parametrize("n,rate,m", [(85, 2, 3), (128, 1, 2), (257, 0, 1), (1, 3, 2), (1, 0, 1), (300, 0, 1)])
@pytest.mark.parametrize("exclusive", [False, True], ids=["plain", "exclusive"])
def test_launch_boundaries(native, small, n, rate, m, exclusive):
    V, R, batch = small["V"], small["R"], small["batch"][:n]
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=16)
    try:
        eng.known_positives_reserve(small["known"])
        X, Y = _sample(eng, batch, rate, m, 31, exclusive)
        X0, Y0 = _sample(eng, batch, rate, 0, 31, exclusive)                 # m = 0 through the new entry point
    finally:
        eng.close()
    want = ref.sample(small["keys"], batch, rate, m, V, R, 31, exclusive)
    assert np.array_equal(X, want["X"]) and np.array_equal(Y, want["Y"])
    first = n * (rate + 1)
    assert len(X) == first + n * m and (Y[:n] == 1).all() and (Y[n:] == 0).all()
    if rate == 0:
        assert np.array_equal(X[:first], batch)
    assert np.array_equal(X0, X[:first]) and np.array_equal(Y0, Y[:first])


def test_rate_zero_is_the_existing_call(native, small):
    """m = 0 through rgcn_negative_sample_relation_device itself: the bytes of rgcn_negative_sample_device and of its
    exclusive form"""
    V, R, batch, rate, seed = small["V"], small["R"], small["batch"][:300], 3, 55
    n, total = len(batch), len(batch) * 4
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=16)
    bufs = []
    try:
        eng.known_positives_reserve(small["known"])
        bd = eng.to_device(batch)
        bufs.append(bd)
        for exclusive in (0, 1):
            xa, ya, xb, yb = (eng.alloc(12 * total), eng.alloc(4 * total), eng.alloc(12 * total), eng.alloc(4 * total))
            bufs += [xa, ya, xb, yb]
            eng.negative_sample_device(bd, n, rate, seed, xa, ya, exclusive=bool(exclusive))
            import ctypes as C
            eng._check(eng.lib.rgcn_negative_sample_relation_device(eng.ctx, bd.ptr, n, rate, 0, exclusive, C.c_uint64(seed),
                                                                    xb.ptr, yb.ptr))
            assert xa.download(np.int32, (total, 3)).tobytes() == xb.download(np.int32, (total, 3)).tobytes()
            assert ya.download(np.float32, (total,)).tobytes() == yb.download(np.float32, (total,)).tobytes()
    finally:
        for b in bufs:
            b.free()
        eng.close()


@pytest.mark.parametrize("exclusive", [False, True], ids=["plain", "exclusive"])
def test_fused_step_appends_the_relation_rows(native, small, exclusive):
    """rgcn_train_step_minibatch_device under rgcn_set_relation_negatives(2): the scratch is the stand-alone call's output;
    the loss is, with ==, that of rgcn_train_step_device fed those X / Y and the drawn graph on an identically initialised
    context; loss and every gradient against float64 at the bar tests/test_gpu_train_step.py holds the decoder's general
    path and the train step to (test_decoder_grid_matches_float64: loss 2e-6; test_train_step_grid_matches_float64: every
    gradient max 5e-6 of scale, l2 2e-6) -- the float64 decoder of helpers.chunked_distmult_float64 on that X, the float64
    reverse mode at the engine's own activations behind it.  Rate 0 again: the first step's loss and scratch bytes.
    Block context, V 150, R 9, d 20, L 2."""
    V, R, d, L, nb, rate, m, keep = small["V"], small["R"], 20, 2, 4, 3, 2, 500
    batch = small["batch"]
    n = len(batch)
    N0, N = n * (rate + 1), n * (rate + 1 + m)
    params = oracle.init_params(V, R, d, L, "block", nb, rng=np.random.RandomState(2))
    eseed, nseed, seed = 41, 91, 8
    eng = native.Engine(V, R, d, L, "block", nb, keep_prob=0.8, max_edges=n)
    other = native.Engine(V, R, d, L, "block", nb, keep_prob=0.8, max_edges=n)
    bufs = []
    try:
        for e in (eng, other):
            e.set_params(params)
            e.decoder_reserve(N)
            e.known_positives_reserve(small["known"])
            e.set_exclusive_negatives(exclusive)
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * (N + GUARD)), eng.alloc(4 * (N + GUARD))
        bufs += [bd, xd, yd]
        eng.copy_to_device(xd, np.full((N + GUARD, 3), -77, dtype=np.int32))
        # mode off (the default): today's bytes
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        off_loss = eng.loss()
        Xoff = xd.download(np.int32, (N + GUARD, 3))
        want_off = (ent.exclusive(small["keys"], batch, rate, V, R, nseed)["X"] if exclusive
                    else ent.plain(batch, rate, V, nseed)[0])
        assert np.array_equal(Xoff[:N0], want_off) and (Xoff[N0:] == -77).all()
        # mode on
        eng.set_relation_negatives(m)
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        loss = eng.loss()
        Xon, Yon = xd.download(np.int32, (N + GUARD, 3)), yd.download(np.float32, (N,))
        assert (Xon[N:] == -77).all()
        Xon = Xon[:N]
        kept = eng.graph_edges()
        acts = [eng.activation(l) for l in range(L + 1)]
        masks = [eng.dropout_mask(l) for l in range(1, L + 1)]
        grads = eng.get_grads()
        want = ref.sample(small["keys"], batch, rate, m, V, R, nseed, exclusive)
        assert np.array_equal(Xon, want["X"]) and np.array_equal(Yon, want["Y"])
        assert np.array_equal(Xon[:N0], Xoff[:N0]) and loss != off_loss
        # the same step from its pieces on the other context: the rows the dropout kernel drew, the stand-alone call,
        # rgcn_train_step_device (no optimizer is configured: the weights have not moved)
        obd, ox, oy, gd = other.to_device(batch), other.alloc(12 * N), other.alloc(4 * N), other.alloc(12 * n)
        bufs += [obd, ox, oy, gd]
        other.set_graph_dropout_device(obd, n, keep, seed=eseed)
        assert np.array_equal(other.graph_edges(), kept)
        other.copy_to_device(gd, other.graph_edges())
        other.negative_sample_device(obd, n, rate, nseed, ox, oy, exclusive=exclusive, relation_rate=m)
        assert np.array_equal(ox.download(np.int32, (N, 3)), Xon) and np.array_equal(oy.download(np.float32, (N,)), Yon)
        other.train_step_device(gd, keep, ox, oy, N, seed=seed, reg_param=0.01)
        assert loss == other.loss()
        # rate 0 again: the first step's loss and scratch bytes, the tiled path included
        eng.set_relation_negatives(0)
        eng.copy_to_device(xd, np.full((N + GUARD, 3), -77, dtype=np.int32))
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        assert eng.loss() == off_loss and xd.download(np.int32, (N + GUARD, 3)).tobytes() == Xoff.tobytes()
    finally:
        for b in bufs:
            b.free()
        eng.close()
        other.close()
    # float64: the decoder on that X at the step's own codes, the encoder's reverse mode behind it
    loss64, dc64, dw64 = helpers.chunked_distmult_float64(acts[-1], params["W_relation"], Xon, Yon, 0.01)
    g64 = helpers.float64_grads_at(dict(V=V, R=R, d=d, L=L, kind="block", nb=nb, params=params, triples=kept,
                                        masks=masks, dcodes=dc64), acts)
    g64["W_relation"] = dw64
    names = [k for k in oracle.weight_names("block", L) if not (k.startswith("b") and k != "b_emb")]
    report, bad = ["loss %.1e" % (abs(loss - loss64) / abs(loss64))], []
    if not abs(loss - loss64) <= 2e-6 * abs(loss64):
        bad.append("loss %.9g, float64 %.9g" % (loss, loss64))
    for k in names:
        assert np.abs(g64[k]).max() > 0, k
        worst, l2 = helpers.error_against(g64[k], grads[k])
        report.append("%s %.1e/%.1e" % (k, worst, l2))
        if not (worst <= 5e-6 and l2 <= 2e-6):
            bad.append("grad %s against float64: max %.2e l2 %.2e" % (k, worst, l2))
    print("; ".join(report))
    assert not bad, bad
    # every relation took part: the relation rows reach rows of W_relation the entity rows of a triple never do
    assert np.abs(grads["W_relation"][:R]).max(axis=1).all()


def _refused(native, call, status):
    with pytest.raises(native.RgcnError) as err:
        call()
    assert err.value.status == status, (err.value.status, str(err.value))


def test_refusals(native, small):
    V, R, batch = small["V"], small["R"], small["batch"][:100]
    n, rate, m = len(batch), 1, 2
    N0, N = n * (rate + 1), n * (rate + 1 + m)
    # one relation
    one = native.Engine(V, 1, 8, 1, "block", 2, max_edges=n)
    try:
        b1 = batch.copy()
        b1[:, 1] = 0
        bd, xd, yd = one.to_device(b1), one.alloc(12 * N), one.alloc(4 * N)
        _refused(native, lambda: one.negative_sample_device(bd, n, rate, 3, xd, yd, relation_rate=m), STATUS_INVALID)
        _refused(native, lambda: one.set_relation_negatives(m), STATUS_INVALID)
        one.negative_sample_device(bd, n, rate, 3, xd, yd)                   # rate 0 asks nothing of the relation count
        one.set_relation_negatives(0)
        for b in (bd, xd, yd):
            b.free()
    finally:
        one.close()
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=n)
    bufs = []
    try:
        eng.set_params(oracle.init_params(V, R, 8, 1, "block", 2, rng=np.random.RandomState(2)))
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        xs, ys = eng.alloc(12 * N0), eng.alloc(4 * N0)                       # sized for n (rate + 1) only
        bufs += [bd, xd, yd, xs, ys]
        # bad rates, exclusive without an index, the counter without one
        for bad in (-1, 1025):
            _refused(native, lambda: eng.negative_sample_device(bd, n, rate, 3, xd, yd, relation_rate=bad), STATUS_INVALID)
            _refused(native, lambda: eng.set_relation_negatives(bad), STATUS_INVALID)
        _refused(native, lambda: eng.negative_sample_device(bd, n, rate, 3, xd, yd, exclusive=True, relation_rate=m),
                 STATUS_STATE)
        _refused(native, eng.negative_relation_unresolved, STATUS_STATE)
        _refused(native, lambda: eng.negative_sample_device(bd, 1 << 20, 1023, 3, xd, yd, relation_rate=1024), STATUS_INVALID)
        eng.negative_sample_device(bd, n, rate, 3, xd, yd, relation_rate=m)  # the plain form needs no index
        assert np.array_equal(xd.download(np.int32, (N, 3)), ref.sample(None, batch, rate, m, V, R, 3, False)["X"])
        # the fused step: a decoder reserve, then a scratch, sized for n (rate + 1) only
        eng.set_relation_negatives(m)
        eng.decoder_reserve(N0)
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xd, yd), STATUS_STATE)
        eng.decoder_reserve(N)
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xs, yd), STATUS_STATE)
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xd, ys), STATUS_STATE)
        eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xd, yd)
        assert np.isfinite(eng.loss())
        assert np.array_equal(xd.download(np.int32, (N, 3)), ref.sample(None, batch, rate, m, V, R, 2, False)["X"])
        # during a capture: the stand-alone call, the switch and the step with the mode on
        eng.sync()
        eng.capture_begin()
        _refused(native, lambda: eng.negative_sample_device(bd, n, rate, 3, xd, yd, relation_rate=m), STATUS_STATE)
        _refused(native, lambda: eng.set_relation_negatives(0), STATUS_STATE)
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xd, yd), STATUS_STATE)
        eng.negative_sample_device(bd, n, rate, 3, xd, yd)                   # (something to capture)
        eng.graph_destroy(eng.capture_end())
    finally:
        for b in bufs:
            b.free()
        eng.close()
    # a relation-sharded context
    with native.Engine(V, R, 8, 1, "block", 2, max_edges=n, rank=0, world=2) as sharded:
        _refused(native, lambda: sharded.set_relation_negatives(m), STATUS_UNSUPPORTED)
        sharded.set_relation_negatives(0)


def test_embedding_kind(native, small):
    """the stand-alone call and the counter on an RGCN_KIND_EMBEDDING context"""
    V, R, batch = small["V"], small["R"], small["batch"][:300]
    eng = native.Engine(V, R, 8, 0, "embedding", 1, max_edges=0)
    try:
        eng.known_positives_reserve(small["known"])
        X, Y = _sample(eng, batch, 4, 2, 77, True)
        assert eng.negative_relation_unresolved() == 0
    finally:
        eng.close()
    want = ref.sample(small["keys"], batch, 4, 2, V, R, 77, True)
    assert np.array_equal(X, want["X"]) and np.array_equal(Y, want["Y"]) and want["relation"]["first_known"].any()


DRIVER_PATHS = {"device": [], "host_sampler": ["--host-sampler"], "host_dropout": ["--host-edge-dropout"],
                "host_negatives": ["--host-negatives", "--batch-workers", "0"]}


@pytest.mark.parametrize("path", sorted(DRIVER_PATHS))
def test_train_driver_with_relation_negatives_and_the_relation_metric(tmp_path, capsys, path):
    """[General] RelationNegativeSampleRate=2 and [Evaluation] Metric=RelationMRR through the driver on the toy dataset of
    tests/test_gpu_driver.py: the fused step (device and host sampler), the stand-alone call (host edge dropout) and the
    numpy port (--host-negatives); the validation score and the test table are the relation ranks'; the checkpoint loads
    in predict --side relation"""
    from relationprediction_amd import predict, train
    from test_gpu_driver import SETTINGS, write_dataset
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    os.makedirs(str(tmp_path / "models"))
    exp = str(tmp_path / "models" / "Toy")
    settings = tmp_path / "toy.exp"
    settings.write_text((SETTINGS % dict(nb=4, concat="Yes", exp=exp))
                        .replace("GraphBatchSize=300", "GraphBatchSize=300\n\tRelationNegativeSampleRate=2")
                        .replace("Metric=MRR", "Metric=RelationMRR"))
    np.random.seed(0)
    model, iterations = train.main(["--settings", str(settings), "--dataset", data, "--max-iterations", "25"]
                                   + DRIVER_PATHS[path])
    out = capsys.readouterr().out
    checks = [l for l in out.splitlines() if l.startswith("Tested validation score")]
    assert iterations == 25 and len(checks) == 1 and 0.0 < float(checks[0].split("Result: ")[1]) <= 1.0
    assert "MRR" in out and "H@10" in out and "Exclusive relation negative sampling:" not in out
    rt = model.get_runtime()
    n, N = 300, 300 * 8
    assert rt._dec_reserved >= N
    if path != "host_negatives":
        X = rt._dev["X"].download(np.int32, (N, 3))
        K = {tuple(t) for t in train_triples.tolist()}
        assert all(tuple(t) in K for t in X[:n].tolist())
        rel, tiled = X[6 * n:], np.tile(X[:n], (2, 1))
        assert np.array_equal(rel[:, [0, 2]], tiled[:, [0, 2]]) and (rel[:, 1] != tiled[:, 1]).all()
        assert ((rel[:, 1] >= 0) & (rel[:, 1] < 6)).all()
        assert getattr(rt, "_relation_rate", 0) == (0 if path == "host_dropout" else 2)
    # the checkpoint answers relation queries
    pairs = [(int(s), int(o)) for s, r, o in train_triples[:5]]
    (tmp_path / "q.txt").write_text("".join("e%d\te%d\n" % p for p in pairs))
    answers = tmp_path / "answers.txt"
    predict.main(["--settings", str(settings), "--dataset", data, "--model", exp + "-0.npz", "--queries",
                  str(tmp_path / "q.txt"), "--k", "3", "--side", "relation", "--keep-known", "--out", str(answers)])
    lines = [l.split("\t") for l in answers.read_text().splitlines()]
    assert len(lines) == 15 and {l[1] for l in lines} <= {"r%d" % i for i in range(6)}
