"""The exclusive negative sampler on the device (rgcn_known_positives_reserve, rgcn_negative_sample_exclusive_device,
rgcn_set_exclusive_negatives) against the numpy mirror of tests/exclusive_negatives_reference.py, bit for bit.  The
statistics (redraws uniform, saturated pairs, brute force over sets) are asserted on the mirror without a GPU
(tests/test_exclusive_negatives_host.py); here the device has to produce the mirror's bytes."""
import numpy as np
import pytest

import exclusive_negatives_reference as ref
import oracle

pytestmark = pytest.mark.gpu

STATUS_INVALID, STATUS_STATE = 1, 4


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def _sample(native, eng, batch, rate, seed, exclusive=True, bufs=None):
    """(X, Y) of one stand-alone sampling call; bufs: (batch, X, Y) device buffers to reuse"""
    n, total = len(batch), len(batch) * (rate + 1)
    own = bufs is None
    if own:
        bufs = (eng.to_device(batch), native.DeviceBuffer(eng, max(12 * total, 16)), native.DeviceBuffer(eng, max(4 * total, 16)))
    try:
        eng.negative_sample_device(bufs[0], n, rate, seed, bufs[1], bufs[2], exclusive=exclusive)
        return bufs[1].download(np.int32, (total, 3)), bufs[2].download(np.float32, (total,))
    finally:
        if own:
            for b in bufs:
                b.free()


@pytest.mark.parametrize("name", ["brute_force", "saturated", "uniform"])
def test_device_equals_the_mirror(native, name):
    """cases 2, 3 and 4 of the host tests: X, Y and the counter of unresolved rows"""
    c = ref.case(name)
    eng = native.Engine(c["V"], c["R"], 8, 1, "block", 2, max_edges=16)
    try:
        eng.known_positives_reserve(c["known"])
        assert eng.negative_unresolved() == 0
        X, Y = _sample(native, eng, c["batch"], c["rate"], c["seed"])
        assert np.array_equal(X, c["mirror"]["X"]) and np.array_equal(Y, c["mirror"]["Y"])
        assert eng.negative_unresolved() == c["mirror"]["unresolved"]
        if name == "saturated":
            assert c["mirror"]["unresolved"] > 0 and c["mirror"]["scanned"].any()
            _sample(native, eng, c["batch"], c["rate"], c["seed"])          # the counter is a total since the reserve
            assert eng.negative_unresolved() == 2 * c["mirror"]["unresolved"]
            eng.known_positives_reserve(c["known"])                         # ... and a reserve starts it over
            assert eng.negative_unresolved() == 0
    finally:
        eng.close()


@pytest.fixture(scope="module")
def small():
    """V 150, R 9 (the parity tests' small shape): K = a batch of 800 distinct triples + 20,000 random ones, about a tenth
    of the candidate space, so that a few hundred corruptions are redrawn"""
    V, R, n = 150, 9, 800
    rng = np.random.RandomState(17)
    flat = rng.permutation(V * R * V)[:n]
    batch = np.stack([flat // (R * V), (flat // V) % R, flat % V], 1).astype(np.int32)
    extra = np.stack([rng.randint(0, V, 20000), rng.randint(0, R, 20000), rng.randint(0, V, 20000)], 1).astype(np.int32)
    known = np.concatenate([batch, extra])
    return dict(V=V, R=R, batch=batch, known=known, keys=ref.build_index(known, V, R))


@pytest.mark.parametrize("n,rate", [(85, 2), (128, 1), (257, 0), (171, 2)])
def test_launch_boundaries(native, small, n, rate):
    """255, 256, 257 and 513 rows around the 256-thread workgroup; rate 0: no negatives, X is the batch"""
    V, R, batch = small["V"], small["R"], small["batch"][:n]
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=16)
    try:
        eng.known_positives_reserve(small["known"])
        guard = np.int32(-77)
        total = n * (rate + 1)
        bd, xd, yd = eng.to_device(batch), eng.to_device(np.full((total + 64, 3), guard)), eng.to_device(
            np.full(total + 64, -77, dtype=np.float32))
        eng.negative_sample_device(bd, n, rate, 31, xd, yd, exclusive=True)
        X, Y = xd.download(np.int32, (total + 64, 3)), yd.download(np.float32, (total + 64,))
        for b in (bd, xd, yd):
            b.free()
    finally:
        eng.close()
    m = ref.exclusive(small["keys"], batch, rate, V, R, 31)
    assert np.array_equal(X[:total], m["X"]) and np.array_equal(Y[:total], m["Y"])
    assert (X[total:] == guard).all() and (Y[total:] == -77).all()       # nothing written behind the last row
    if rate == 0:
        assert np.array_equal(X[:total], batch) and (Y[:total] == 1).all()
    else:
        assert m["first_known"].any()


def test_determinism_and_the_plain_sampler(native, small):
    """the same seed twice: the same bytes, another seed: others; and the plain sampler on the same context and seed
    differs from the exclusive output exactly in the rows the mirror says are known"""
    V, R, batch, rate, seed = small["V"], small["R"], small["batch"], 3, 1234
    n = len(batch)
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=16)
    try:
        eng.known_positives_reserve(small["known"])
        Xa, Ya = _sample(native, eng, batch, rate, seed)
        Xb, Yb = _sample(native, eng, batch, rate, seed)
        Xc, _ = _sample(native, eng, batch, rate, seed + 1)
        Xp, Yp = _sample(native, eng, batch, rate, seed, exclusive=False)
    finally:
        eng.close()
    assert Xa.tobytes() == Xb.tobytes() and Ya.tobytes() == Yb.tobytes()
    assert not np.array_equal(Xa, Xc)
    m = ref.exclusive(small["keys"], batch, rate, V, R, seed)
    assert np.array_equal(Xa, m["X"])
    assert np.array_equal(Xp, ref.plain(batch, rate, V, seed)[0]) and np.array_equal(Yp, Ya)
    differs = (Xa[n:] != Xp[n:]).any(axis=1)
    assert np.array_equal(differs, m["first_known"]) and differs.sum() >= 100


def test_fused_step_draws_exclusively_when_the_mode_is_on(native, small):
    """rgcn_train_step_minibatch_device under rgcn_set_exclusive_negatives: the scratch is the stand-alone exclusive call's
    output, the loss that of rgcn_train_step_device fed those X / Y (and the graph the dropout kernel drew) on an
    identically initialised context; with the mode off the scratch is the plain sampler's.  Block context, V 150, R 9,
    d 20, L 2."""
    V, R, d, L, nb, rate, keep = small["V"], small["R"], 20, 2, 4, 3, 500
    batch = small["batch"]
    n = len(batch)
    N = n * (rate + 1)
    params = oracle.init_params(V, R, d, L, "block", nb, rng=np.random.RandomState(2))
    eseed, nseed, seed = 41, 91, 8
    eng = native.Engine(V, R, d, L, "block", nb, max_edges=n)
    other = native.Engine(V, R, d, L, "block", nb, max_edges=n)
    bufs = []
    try:
        for e in (eng, other):
            e.set_params(params)
            e.decoder_reserve(N)
        bd, xd, yd = eng.to_device(batch), native.DeviceBuffer(eng, 12 * N), native.DeviceBuffer(eng, 4 * N)
        bufs += [bd, xd, yd]
        # mode off (the default): the plain sampler's bytes
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        plain_loss = eng.loss()
        Xoff = xd.download(np.int32, (N, 3))
        assert np.array_equal(Xoff, ref.plain(batch, rate, V, nseed)[0])
        # mode on
        eng.known_positives_reserve(small["known"])
        eng.set_exclusive_negatives(True)
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        loss = eng.loss()
        Xon, Yon = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        kept = eng.graph_edges()
        x2, y2 = native.DeviceBuffer(eng, 12 * N), native.DeviceBuffer(eng, 4 * N)
        bufs += [x2, y2]
        Xs, Ys = _sample(native, eng, batch, rate, nseed, bufs=(bd, x2, y2))
        assert np.array_equal(Xon, Xs) and np.array_equal(Yon, Ys)
        assert np.array_equal(Xon, ref.exclusive(small["keys"], batch, rate, V, R, nseed)["X"])
        assert not np.array_equal(Xon, Xoff)
        # the same step from its pieces on the other context, as test_minibatch_step_equals_the_step_on_its_own_draws
        # compares the plain one: the rows the dropout kernel drew, the stand-alone sampling call, rgcn_train_step_device
        # (no optimizer is configured: the weights have not moved)
        other.known_positives_reserve(small["known"])
        obd, ox, oy = other.to_device(batch), native.DeviceBuffer(other, 12 * N), native.DeviceBuffer(other, 4 * N)
        gd = native.DeviceBuffer(other, 12 * n)
        bufs += [obd, ox, oy, gd]
        other.set_graph_dropout_device(obd, n, keep, seed=eseed)
        assert np.array_equal(other.graph_edges(), kept)
        other.copy_to_device(gd, other.graph_edges())
        other.negative_sample_device(obd, n, rate, nseed, ox, oy, exclusive=True)
        assert np.array_equal(ox.download(np.int32, (N, 3)), Xon) and np.array_equal(oy.download(np.float32, (N,)), Yon)
        other.train_step_device(gd, keep, ox, oy, N, seed=seed, reg_param=0.01)
        assert loss == other.loss()
        assert loss != plain_loss
        # and off again; a released index switches the mode off by itself
        eng.set_exclusive_negatives(False)
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        assert eng.loss() == plain_loss and np.array_equal(xd.download(np.int32, (N, 3)), Xoff)
        eng.set_exclusive_negatives(True)
        eng.known_positives_reserve(np.zeros((0, 3), dtype=np.int32))
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        assert eng.loss() == plain_loss and np.array_equal(xd.download(np.int32, (N, 3)), Xoff)
    finally:
        for b in bufs:
            b.free()
        eng.close()
        other.close()


def test_embedding_kind(native, small):
    """the stand-alone call, the counter and the reserve on an RGCN_KIND_EMBEDDING context"""
    V, R, batch = small["V"], small["R"], small["batch"][:300]
    eng = native.Engine(V, R, 8, 0, "embedding", 1, max_edges=0)
    try:
        eng.known_positives_reserve(small["known"])
        X, Y = _sample(native, eng, batch, 4, 77)
        assert eng.negative_unresolved() == 0
    finally:
        eng.close()
    m = ref.exclusive(small["keys"], batch, 4, V, R, 77)
    assert np.array_equal(X, m["X"]) and np.array_equal(Y, m["Y"]) and m["first_known"].any()


def test_captured_sampling_call_follows_the_replay_offset(native, small):
    """One captured exclusive sampling call, beside a captured plain one.  The direct call is the mirror at `seed`; the
    context's replay counter is bumped at the head of every replay, so the k-th replay (k = 1, 2, 3) is the mirror at
    seed + k -- for the exclusive kernel exactly as for the plain one."""
    V, R, batch, rate, seed = small["V"], small["R"], small["batch"][:300], 2, 500
    n, total = len(batch), len(batch) * 3
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=16)
    try:
        eng.known_positives_reserve(small["known"])
        bd = eng.to_device(batch)
        xd, yd = native.DeviceBuffer(eng, 12 * total), native.DeviceBuffer(eng, 4 * total)
        xp, yp = native.DeviceBuffer(eng, 12 * total), native.DeviceBuffer(eng, 4 * total)
        X0, _ = _sample(native, eng, batch, rate, seed, bufs=(bd, xd, yd))
        assert np.array_equal(X0, ref.exclusive(small["keys"], batch, rate, V, R, seed)["X"])
        eng.sync()
        eng.capture_begin()
        with pytest.raises(native.RgcnError) as err:
            eng.known_positives_reserve(small["known"])                  # reads host memory
        assert err.value.status == STATUS_STATE
        with pytest.raises(native.RgcnError) as err:
            eng.set_exclusive_negatives(True)
        assert err.value.status == STATUS_STATE
        eng.negative_sample_device(bd, n, rate, seed, xd, yd, exclusive=True)
        eng.negative_sample_device(bd, n, rate, seed, xp, yp)
        gid = eng.capture_end()
        for k in (1, 2, 3):
            eng.graph_launch(gid)
            X, Xp = xd.download(np.int32, (total, 3)), xp.download(np.int32, (total, 3))
            assert np.array_equal(X, ref.exclusive(small["keys"], batch, rate, V, R, seed + k)["X"]), k
            assert np.array_equal(Xp, ref.plain(batch, rate, V, seed + k)[0]), k
        eng.graph_destroy(gid)
        for b in (bd, xd, yd, xp, yp):
            b.free()
    finally:
        eng.close()


@pytest.mark.parametrize("extra", [[], ["--host-sampler"], ["--host-edge-dropout"]], ids=["device", "host_sampler", "host_dropout"])
def test_train_driver_with_the_setting_on(tmp_path, capsys, extra):
    """[General] ExclusiveNegativeSampling=Yes through the driver, on the fused minibatch step (device and host sampler)
    and on the stand-alone sampling call (host edge dropout): the runtime reserved the training triples, and the decoder
    batch of the last step holds no training triple among its negatives"""
    import os
    from relationprediction_amd import train
    from test_gpu_driver import SETTINGS, write_dataset
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    os.makedirs(str(tmp_path / "models"))
    settings = tmp_path / "toy.exp"
    settings.write_text((SETTINGS % dict(nb=4, concat="Yes", exp=str(tmp_path / "models" / "Toy")))
                        .replace("GraphBatchSize=300", "GraphBatchSize=300\n\tExclusiveNegativeSampling=Yes"))
    np.random.seed(0)
    model, iterations = train.main(["--settings", str(settings), "--dataset", data, "--max-iterations", "25"] + extra)
    out = capsys.readouterr().out
    assert iterations == 25 and "Tested validation score" in out
    assert "Exclusive negative sampling:" not in out                     # nothing unresolved: nothing printed
    rt = model.get_runtime()
    assert rt._known is not None and np.array_equal(rt._known, train_triples) and rt._exclusive_on
    assert rt.negative_unresolved() == 0 and model.device_negative_unresolved() == 0
    N = 300 * 6
    X = rt._dev["X"].download(np.int32, (N, 3))
    K = {tuple(t) for t in train_triples.tolist()}
    assert all(tuple(t) in K for t in X[:300].tolist())                  # the positives are training triples
    assert not any(tuple(t) in K for t in X[300:].tolist())
    assert (X[300:] != np.tile(X[:300], (5, 1))).any(axis=1).all()       # ... and no negative is its own positive


def test_states(native, small):
    V, R, batch = small["V"], small["R"], small["batch"][:100]
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=16)
    try:
        bd, xd, yd = eng.to_device(batch), native.DeviceBuffer(eng, 12 * 200), native.DeviceBuffer(eng, 4 * 200)
        # before a reserve
        for call in (lambda: eng.negative_sample_device(bd, 100, 1, 3, xd, yd, exclusive=True),
                     lambda: eng.set_exclusive_negatives(True), eng.negative_unresolved):
            with pytest.raises(native.RgcnError) as err:
                call()
            assert err.value.status == STATUS_STATE
        eng.set_exclusive_negatives(False)                               # switching off needs nothing
        eng.known_positives_reserve(small["known"])
        eng.set_exclusive_negatives(True)
        want = ref.exclusive(small["keys"], batch, 1, V, R, 3)["X"]
        # a reserve with a bad id: refused, and the earlier index still answers
        for bad in ((V, 0, 1), (1, R, 1), (1, 0, -1)):
            with pytest.raises(native.RgcnError) as err:
                eng.known_positives_reserve(np.array([(1, 0, 1), bad], dtype=np.int32))
            assert err.value.status == STATUS_INVALID
        eng.negative_sample_device(bd, 100, 1, 3, xd, yd, exclusive=True)
        assert np.array_equal(xd.download(np.int32, (200, 3)), want)
        # num_triples = 0 releases the index, and the mode is off
        eng.known_positives_reserve(np.zeros((0, 3), dtype=np.int32))
        with pytest.raises(native.RgcnError) as err:
            eng.negative_sample_device(bd, 100, 1, 3, xd, yd, exclusive=True)
        assert err.value.status == STATUS_STATE
        with pytest.raises(native.RgcnError) as err:
            eng.set_exclusive_negatives(True)
        assert err.value.status == STATUS_STATE
        eng.negative_sample_device(bd, 100, 1, 3, xd, yd)
        assert np.array_equal(xd.download(np.int32, (200, 3)), ref.plain(batch, 1, V, 3)[0])
        for b in (bd, xd, yd):
            b.free()
    finally:
        eng.close()
