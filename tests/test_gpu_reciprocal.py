"""Reciprocal relations on the device (rgcn_reciprocal_rows_device, rgcn_set_reciprocal_relations) against the numpy mirror
of tests/reciprocal_reference.py, bit for bit, and against float64.  The properties of the pass are asserted on the mirror
without a GPU (tests/test_reciprocal_host.py); here the device has to produce the mirror's bytes behind each of the three
samplers, the queries have to read W_relation[R + r] on the subject side, the decoder and both fused steps have to take the
2R relation rows, and the refusals have to hold."""
import functools

import numpy as np
import pytest

import helpers
import oracle
import reciprocal_reference as ref
import relation_negatives_reference as rel

pytestmark = pytest.mark.gpu

STATUS_INVALID, STATUS_STATE, STATUS_UNSUPPORTED = 1, 4, 5
GUARD = 64


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def small():
    V, R, batch, known = rel.small_fixture()
    return dict(V=V, R=R, batch=batch, known=known)


@functools.lru_cache(maxsize=None)
def mirror(kind, n, rate, m, seed):
    """the mirror's answer on the first n batch rows of the small fixture; computed once, to be left unchanged"""
    V, R, batch, known = rel.small_fixture()
    out = ref.sample(kind, batch[:n], known, rate, m, V, R, seed)
    for a in out.values():
        a.setflags(write=False)
    return out


def _draw(eng, kind, bd, n, rate, m, seed, xd, yd, reciprocal):
    """the stand-alone calls of one batch: the sampler of `kind` (the typed entity rows replace the ones the relation call
    drew in front of its relation rows, as the runtime does it), then the reciprocal pass"""
    if kind != "typed" or m:
        eng.negative_sample_device(bd, n, rate, seed, xd, yd, exclusive=kind == "exclusive", relation_rate=m,
                                   reciprocal=reciprocal and kind != "typed")
    if kind == "typed":
        eng.negative_sample_typed_device(bd, n, rate, seed, xd, yd, exclusive=False)
        if reciprocal:
            eng.reciprocal_rows_device(bd, n, rate, m, seed, xd, yd)


# (n, rate, m): 255, 256 and 257 threads of the pass around the 256-thread workgroup; tail rows only; one batch row;
# relation rows between the negatives and the tail
@pytest.mark.parametrize("n,rate,m", [(85, 2, 0), (64, 3, 0), (257, 0, 0), (1, 3, 2), (128, 1, 2)])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_device_equals_the_mirror(native, small, kind, n, rate, m):
    """X and Y behind each sampler, with GUARD rows of -77 behind the output that come back untouched; and the pass rewrites
    nothing but the relation column of negatives and the tail: X before and after differ nowhere else"""
    V, R, batch, seed = small["V"], small["R"], small["batch"][:n], 31
    N0, N = n * (rate + 1 + m), n * (rate + 2 + m)
    assert n * rate + n in {255, 256, 257, 4}
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=16)
    bufs = []
    try:
        eng.known_positives_reserve(small["known"])
        eng.type_sets_reserve(small["known"])
        bd = eng.to_device(batch)
        xd = eng.to_device(np.full((N + GUARD, 3), -77, dtype=np.int32))
        yd = eng.to_device(np.full(N + GUARD, -77, dtype=np.float32))
        bufs += [bd, xd, yd]
        _draw(eng, kind, bd, n, rate, m, seed, xd, yd, False)
        X0, Y0 = xd.download(np.int32, (N + GUARD, 3)), yd.download(np.float32, (N + GUARD,))
        if kind == "typed":
            eng.reciprocal_rows_device(bd, n, rate, m, seed, xd, yd)
        else:
            # the chained form of the engine: the sampler again (the same bytes), the pass behind it
            _draw(eng, kind, bd, n, rate, m, seed, xd, yd, True)
        X, Y = xd.download(np.int32, (N + GUARD, 3)), yd.download(np.float32, (N + GUARD,))
    finally:
        for b in bufs:
            b.free()
        eng.close()
    want = mirror(kind, n, rate, m, seed)
    assert np.array_equal(X0[:N0], want["X0"]) and np.array_equal(Y0[:N0], want["Y0"])
    assert (X0[N0:] == -77).all() and (Y0[N0:] == -77).all()
    assert np.array_equal(X[:N], want["X"]) and np.array_equal(Y[:N], want["Y"])
    assert (X[N:] == -77).all() and (Y[N:] == -77).all()                 # nothing written behind the last row
    # untouched words: everything in front of the tail but the relation column of the entity negatives
    changed = X[:N0] != X0[:N0]
    assert not changed[:, [0, 2]].any() and not changed[:n].any() and not changed[n * (rate + 1):].any()
    assert np.array_equal(Y[:N0], Y0[:N0])
    assert np.array_equal(changed[n:n * (rate + 1), 1], want["coin"] == 0)


def _query_engines(native, V, R, d, seed):
    """three block contexts after a test-mode forward over one graph: the mode on, the mode off with rows r of W_relation
    overwritten by rows R + r, and the mode off untouched"""
    L, nb = 1, 4 if d == 20 else 2            # (block sizes 5 and 4)
    rng = np.random.RandomState(seed)
    params = oracle.init_params(V, R, d, L, "block", nb, rng=rng)
    graph = np.stack([rng.randint(0, V, 600), rng.randint(0, R, 600), rng.randint(0, V, 600)], 1).astype(np.int32)
    swapped = dict(params)
    swapped["W_relation"] = params["W_relation"].copy()
    swapped["W_relation"][:R] = params["W_relation"][R:2 * R]
    engines = []
    for p, on in ((params, True), (swapped, False), (params, False)):
        eng = native.Engine(V, R, d, L, "block", nb, max_edges=len(graph))
        engines.append(eng)
        eng.set_params(p)
        eng.set_graph(graph)
        eng.forward(train=False)
        eng.type_sets_reserve(graph)
        eng.set_reciprocal_relations(on)
    return engines, graph, rng


@pytest.mark.parametrize("d", [20, 8])
def test_subject_queries_read_the_inverse_relation(native, d):
    """rgcn_rank_device, rgcn_topk_device (k = 3), rgcn_rank_typed_device and rgcn_score_queries_device with predict_object =
    0: the context with the mode on answers what a context without it answers whose rows r of W_relation hold rows R + r --
    the same energies buffer, ranks and answers, bit for bit; with predict_object = 1 it answers what the untouched
    context answers.  V 150, R 9; 40 queries in chunks of 16."""
    V, R = 150, 9
    engines, graph, rng = _query_engines(native, V, R, d, 5 + d)
    on, swapped, plain = engines
    try:
        queries = np.concatenate([graph[rng.randint(0, len(graph), 20)],
                                  np.stack([rng.randint(0, V, 20), rng.randint(0, R, 20), rng.randint(0, V, 20)], 1)
                                  ]).astype(np.int32)
        ptr = np.arange(len(queries) + 1, dtype=np.int64)
        for eng in engines:
            eng.rank_reserve(16)
        for predict_object, other in ((False, swapped), (True, plain)):
            gold = np.ascontiguousarray(queries[:, 2 if predict_object else 0])
            got, want = [], []
            for eng, out in ((on, got), (other, want)):
                out.append(eng.ranks(queries, predict_object, ptr, gold))
                out.append(eng.topk(queries, predict_object, 3))
                out.append(eng.ranks_typed(queries, predict_object, ptr, gold))
                eng.score_queries(queries[:16], predict_object)
                out.append((eng.read_buffer(native.BUF_RANK_ENERGIES),))
            for a, b in zip(got, want):
                for x, y in zip(a, b):
                    assert x.tobytes() == y.tobytes()
        # the two sides differ: the mode-on context against the untouched one on the subject side
        on.score_queries(queries[:16], False)
        plain.score_queries(queries[:16], False)
        assert not np.array_equal(on.read_buffer(native.BUF_RANK_ENERGIES), plain.read_buffer(native.BUF_RANK_ENERGIES))
        # a relation >= R is refused on either side, mode on: the id is validated against R first
        bad = queries[:4].copy()
        bad[2, 1] = R
        for predict_object in (False, True):
            with pytest.raises(native.RgcnError):
                on.topk(bad, predict_object, 3)
        assert on.topk(queries[:4], False, 3)[0].tobytes() == swapped.topk(queries[:4], False, 3)[0].tobytes()
    finally:
        for eng in engines:
            eng.close()


def _embedding(native, V, R, d, seed):
    rng = np.random.RandomState(seed)
    eng = native.Engine(V, R, d, 0, "embedding", 1, keep_prob=1.0, max_edges=0)
    params = {"W_emb": (0.5 * rng.randn(V, d)).astype(np.float32), "b_emb": np.zeros(d, dtype=np.float32),
              "W_relation": (0.5 * rng.randn(V, d)).astype(np.float32)}
    eng.set_params(params)
    return eng, params


def _against_float64(loss, grads, loss64, grads64):
    """the bars tests/test_gpu_relation_negatives.py takes from tests/test_gpu_train_step.py: loss 2e-6 relative, every
    gradient max 5e-6 of scale and l2 2e-6"""
    report, bad = ["loss %.1e" % (abs(loss - loss64) / abs(loss64))], []
    if not abs(loss - loss64) <= 2e-6 * abs(loss64):
        bad.append("loss %.9g, float64 %.9g" % (loss, loss64))
    for k in sorted(grads64):
        assert np.abs(grads64[k]).max() > 0, k
        worst, l2 = helpers.error_against(grads64[k], grads[k])
        report.append("%s %.1e/%.1e" % (k, worst, l2))
        if not (worst <= 5e-6 and l2 <= 2e-6):
            bad.append("grad %s against float64: max %.2e l2 %.2e" % (k, worst, l2))
    print("; ".join(report))
    assert not bad, bad


@pytest.mark.parametrize("d,reserve_first", [(20, True), (8, False), (10, True)])
def test_decoder_takes_a_reciprocal_batch(native, small, d, reserve_first):
    """rgcn_decoder_loss_backward_device on the mirror's batch (n 300, rate 3, m 2) against
    helpers.chunked_distmult_float64 on the same X, Y, at a float4 width with and without the line form of the entity
    gradient (d 20, d 8) and at a scalar width (d 10); the reserve before and after the setter.  dW_relation has rows
    [0, 2R) all non-zero (the batch holds every relation) and rows >= 2R exactly zero; with the mode off the same batch
    is refused."""
    V, R, n, rate, m = small["V"], small["R"], 300, 3, 2
    want = mirror("plain", n, rate, m, 77)
    X, Y = want["X"], want["Y"]
    N = len(X)
    assert set(np.unique(X[:, 1]).tolist()) == set(range(2 * R))
    eng, params = _embedding(native, V, R, d, 3)
    bufs = []
    try:
        if reserve_first:
            eng.decoder_reserve(N)
        eng.set_reciprocal_relations(True)
        if not reserve_first:
            eng.decoder_reserve(N)
        xd, yd = eng.to_device(X), eng.to_device(Y)
        bufs += [xd, yd]
        eng.forward(train=True, seed=1)
        eng.decoder_loss_backward_device(xd, yd, N, 0.01)
        loss, dcodes, dW = eng.loss(), eng.dcodes(), eng.get_grad("W_relation")
        # the mode off: r >= R stays the error it is
        eng.set_reciprocal_relations(False)
        assert not eng.get_grad("W_relation")[R:].any()
        eng.forward(train=True, seed=1)
        with pytest.raises(native.RgcnError):
            eng.decoder_loss_backward_device(xd, yd, N, 0.01)
            eng.loss()
    finally:
        for b in bufs:
            b.free()
        eng.close()
    loss64, dc64, dw64 = helpers.chunked_distmult_float64(params["W_emb"], params["W_relation"], X, Y, 0.01)
    _against_float64(loss, {"dcodes": dcodes, "W_relation": dW}, loss64, {"dcodes": dc64, "W_relation": dw64})
    assert np.abs(dW[:2 * R]).max(axis=1).all() and not dW[2 * R:].any()


@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("exclusive", [False, True], ids=["plain", "exclusive"])
def test_fused_step_trains_on_the_reciprocal_batch(native, small, exclusive, m):
    """rgcn_train_step_minibatch_device under rgcn_set_reciprocal_relations: the scratch is the mirror's batch; the loss is,
    with ==, that of rgcn_train_step_device fed the stand-alone calls' X / Y and the drawn graph on an identically
    initialised context; loss and every gradient against float64 (the decoder of helpers.chunked_distmult_float64 on that
    X at the step's own codes, the float64 reverse mode at the engine's own activations behind it).  The mode off again:
    the first step's loss and scratch bytes, the tiled path included.  Block context, V 150, R 9, d 20, L 2, rate 3."""
    V, R, d, L, nb, rate, keep = small["V"], small["R"], 20, 2, 4, 3, 500
    batch = small["batch"]
    n = len(batch)
    kind = "exclusive" if exclusive else "plain"
    N0, N = n * (rate + 1), n * (rate + 2 + m)
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
        fill = np.full((N + GUARD, 3), -77, dtype=np.int32)
        eng.copy_to_device(xd, fill)
        # mode off (the default): today's bytes
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        off_loss = eng.loss()
        Xoff = xd.download(np.int32, (N + GUARD, 3))
        assert np.array_equal(Xoff[:N0], mirror(kind, n, rate, 0, nseed)["X0"]) and (Xoff[N0:] == -77).all()
        # mode on
        eng.set_reciprocal_relations(True)
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
        want = mirror(kind, n, rate, m, nseed)
        assert np.array_equal(Xon, want["X"]) and np.array_equal(Yon, want["Y"]) and loss != off_loss
        # the same step from its pieces on the other context: the rows the dropout kernel drew, the stand-alone calls,
        # rgcn_train_step_device (no optimizer is configured: the weights have not moved)
        other.set_reciprocal_relations(True)
        obd, ox, oy, gd = other.to_device(batch), other.alloc(12 * N), other.alloc(4 * N), other.alloc(12 * n)
        bufs += [obd, ox, oy, gd]
        other.set_graph_dropout_device(obd, n, keep, seed=eseed)
        assert np.array_equal(other.graph_edges(), kept)
        other.copy_to_device(gd, other.graph_edges())
        other.negative_sample_device(obd, n, rate, nseed, ox, oy, exclusive=exclusive, relation_rate=m, reciprocal=True)
        assert np.array_equal(ox.download(np.int32, (N, 3)), Xon) and np.array_equal(oy.download(np.float32, (N,)), Yon)
        other.train_step_device(gd, keep, ox, oy, N, seed=seed, reg_param=0.01)
        assert loss == other.loss()
        # the mode off again: the first step's loss and scratch bytes, the tiled path included
        eng.set_reciprocal_relations(False)
        eng.set_relation_negatives(0)
        eng.copy_to_device(xd, fill)
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        assert eng.loss() == off_loss and xd.download(np.int32, (N + GUARD, 3)).tobytes() == Xoff.tobytes()
        assert not eng.get_grad("W_relation")[R:].any()
    finally:
        for b in bufs:
            b.free()
        eng.close()
        other.close()
    loss64, dc64, dw64 = helpers.chunked_distmult_float64(acts[-1], params["W_relation"], Xon, Yon, 0.01)
    g64 = helpers.float64_grads_at(dict(V=V, R=R, d=d, L=L, kind="block", nb=nb, params=params, triples=kept,
                                        masks=masks, dcodes=dc64), acts)
    g64["W_relation"] = dw64
    names = [k for k in oracle.weight_names("block", L) if not (k.startswith("b") and k != "b_emb")]
    _against_float64(loss, grads, loss64, {k: g64[k] for k in names})
    assert np.abs(grads["W_relation"][:2 * R]).max(axis=1).all() and not grads["W_relation"][2 * R:].any()


@pytest.mark.parametrize("m", [0, 2])
def test_adversarial_weights_under_the_mode(native, small, m):
    """AdversarialTemperature with the mode on, in the fused minibatch step: two calls return the same bytes, the tail
    weights are exactly 1, every group of the first N - n rows sums to K + m (within the 1e-3 tests/test_gpu_adversarial.py
    allows that sum), and the head is what rgcn_adversarial_weights_device returns for the first N - n rows"""
    V, R, d, L, nb, rate, n, keep, T = small["V"], small["R"], 20, 2, 4, 3, 257, 150, 1.5
    batch = small["batch"][:n]
    N = n * (rate + 2 + m)
    head = N - n
    eng = native.Engine(V, R, d, L, "block", nb, keep_prob=0.8, max_edges=n)
    bufs = []
    try:
        eng.set_params(oracle.init_params(V, R, d, L, "block", nb, rng=np.random.RandomState(2)))
        eng.decoder_reserve(N)
        eng.set_reciprocal_relations(True)
        eng.set_relation_negatives(m)
        eng.set_adversarial_negatives(T)
        bd, xd, yd, wd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N), eng.alloc(4 * head)
        bufs += [bd, xd, yd, wd]
        got = []
        for _ in range(2):
            eng.train_step_minibatch_device(bd, n, keep, 41, rate, 91, xd, yd, seed=8, reg_param=0.01)
            assert np.isfinite(eng.loss())
            got.append(eng.read_buffer(native.BUF_ADVERSARIAL_WEIGHTS))
        eng.adversarial_weights(xd, head, n, T, wd)                         # the codes of the step's forward pass
        alone = wd.download(np.float32, (head,))
        X = xd.download(np.int32, (N, 3))
    finally:
        for b in bufs:
            b.free()
        eng.close()
    w = got[0]
    assert len(w) == N and w.tobytes() == got[1].tobytes()
    assert np.array_equal(w[head:], np.ones(n, dtype=np.float32)) and np.array_equal(w[:n], np.ones(n, dtype=np.float32))
    groups = w[n:head].reshape(rate + m, n)
    assert (np.abs(groups.sum(axis=0) - (rate + m)) < 1e-3).all() and groups.std() > 1e-3
    assert w[:head].tobytes() == alone.tobytes()
    assert np.array_equal(X, mirror("plain", n, rate, m, 91)["X"]) and X[n:head, 1].max() >= R   # both directions in a group


def test_embedding_kind(native, small):
    """an RGCN_KIND_EMBEDDING context: the sampler pass, the step on its batch against float64, and subject ranks that
    read W_relation[R + r]"""
    V, R, n, rate, m, d = small["V"], small["R"], 300, 4, 1, 12
    batch = small["batch"][:n]
    N = n * (rate + 2 + m)
    eng, params = _embedding(native, V, R, d, 9)
    swapped = dict(params)
    swapped["W_relation"] = params["W_relation"].copy()
    swapped["W_relation"][:R] = params["W_relation"][R:2 * R]
    other = native.Engine(V, R, d, 0, "embedding", 1, keep_prob=1.0, max_edges=0)
    bufs = []
    try:
        other.set_params(swapped)
        eng.known_positives_reserve(small["known"])
        eng.set_reciprocal_relations(True)
        eng.decoder_reserve(N)
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        bufs += [bd, xd, yd]
        eng.negative_sample_device(bd, n, rate, 77, xd, yd, exclusive=True, relation_rate=m, reciprocal=True)
        X, Y = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        eng.train_step_device(None, 0, xd, yd, N, seed=5, reg_param=0.01)
        loss, grads = eng.loss(), eng.get_grads()
        queries = batch[:40]
        ptr = np.arange(41, dtype=np.int64)
        for e in (eng, other):
            e.forward(train=False)
            e.rank_reserve(40)
        for predict_object, same in ((False, True), (True, False)):
            gold = np.ascontiguousarray(queries[:, 2 if predict_object else 0])
            a, b = eng.ranks(queries, predict_object, ptr, gold), other.ranks(queries, predict_object, ptr, gold)
            assert (a[0].tobytes() == b[0].tobytes()) == same
    finally:
        for b in bufs:
            b.free()
        eng.close()
        other.close()
    want = mirror("exclusive", n, rate, m, 77)
    assert np.array_equal(X, want["X"]) and np.array_equal(Y, want["Y"])
    loss64, dc64, dw64 = helpers.chunked_distmult_float64(params["W_emb"], params["W_relation"], X, Y, 0.01)
    _against_float64(loss, grads, loss64, {"W_emb": dc64, "W_relation": dw64})
    assert np.abs(grads["W_relation"][:2 * R]).max(axis=1).all() and not grads["W_relation"][2 * R:].any()


def _refused(native, call, status):
    with pytest.raises(native.RgcnError) as err:
        call()
    assert err.value.status == status, (err.value.status, str(err.value))


def test_refusals(native, small):
    V, R, batch = small["V"], small["R"], small["batch"][:100]
    n, rate = len(batch), 1
    N0, N = n * (rate + 1), n * (rate + 2)
    # 2R > V: W_relation has no rows for the inverse relations
    with native.Engine(16, 9, 8, 1, "block", 2, max_edges=n) as few:
        b16 = batch % np.array([16, 9, 16], dtype=np.int32)
        bd, xd, yd = few.to_device(b16), few.alloc(12 * N), few.alloc(4 * N)
        _refused(native, lambda: few.set_reciprocal_relations(True), STATUS_UNSUPPORTED)
        few.negative_sample_device(bd, n, rate, 3, xd, yd)
        _refused(native, lambda: few.reciprocal_rows_device(bd, n, rate, 0, 3, xd, yd), STATUS_UNSUPPORTED)
        few.set_reciprocal_relations(False)
        for b in (bd, xd, yd):
            b.free()
    with native.Engine(18, 9, 8, 1, "block", 2, max_edges=n) as just:       # 2R == V is enough
        just.set_reciprocal_relations(True)
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=n)
    bufs = []
    try:
        eng.set_params(oracle.init_params(V, R, 8, 1, "block", 2, rng=np.random.RandomState(2)))
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        xs, ys = eng.alloc(12 * N0), eng.alloc(4 * N0)                       # sized for n (rate + 1) only
        bufs += [bd, xd, yd, xs, ys]
        for bad in (-1, 1025):
            _refused(native, lambda: eng.reciprocal_rows_device(bd, n, bad, 0, 3, xd, yd), STATUS_INVALID)
            _refused(native, lambda: eng.reciprocal_rows_device(bd, n, rate, bad, 3, xd, yd), STATUS_INVALID)
        eng.negative_sample_device(bd, n, rate, 3, xs, ys)
        _refused(native, lambda: eng.reciprocal_rows_device(bd, n, rate, 0, 3, xs, yd), STATUS_STATE)
        _refused(native, lambda: eng.reciprocal_rows_device(bd, n, rate, 0, 3, xd, ys), STATUS_STATE)
        # the entity softmax, set in either order
        eng.set_entity_softmax(0.5, n)
        _refused(native, lambda: eng.set_reciprocal_relations(True), STATUS_UNSUPPORTED)
        eng.set_entity_softmax(0.0)
        eng.set_reciprocal_relations(True)
        _refused(native, lambda: eng.set_entity_softmax(0.5, n), STATUS_UNSUPPORTED)
        eng.set_entity_softmax(0.0)                                          # (switching it off is always allowed)
        # the fused step: a decoder reserve, then a scratch, sized for n (rate + 1) only
        eng.decoder_reserve(N0)
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xd, yd), STATUS_STATE)
        eng.decoder_reserve(N)
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xs, yd), STATUS_STATE)
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xd, ys), STATUS_STATE)
        eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 2, xd, yd)
        assert np.isfinite(eng.loss())
        assert np.array_equal(xd.download(np.int32, (N, 3)), mirror("plain", n, rate, 0, 2)["X"])
        # capture: refused to begin with the mode on; with it off, the switch and the pass are refused inside one
        eng.sync()
        _refused(native, eng.capture_begin, STATUS_UNSUPPORTED)
        eng.set_reciprocal_relations(False)
        eng.capture_begin()
        _refused(native, lambda: eng.set_reciprocal_relations(True), STATUS_UNSUPPORTED)
        _refused(native, lambda: eng.reciprocal_rows_device(bd, n, rate, 0, 3, xd, yd), STATUS_STATE)
        eng.negative_sample_device(bd, n, rate, 3, xd, yd)                   # (something to capture)
        eng.graph_destroy(eng.capture_end())
    finally:
        for b in bufs:
            b.free()
        eng.close()
    # a relation-sharded context
    with native.Engine(V, R, 8, 1, "block", 2, max_edges=n, rank=0, world=2) as sharded:
        _refused(native, lambda: sharded.set_reciprocal_relations(True), STATUS_UNSUPPORTED)
        sharded.set_reciprocal_relations(False)
