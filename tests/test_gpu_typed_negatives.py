"""Type-constrained negatives, ranks and top-k on the device (rgcn_type_sets_reserve, rgcn_negative_sample_typed_device,
rgcn_set_typed_negatives, rgcn_rank_typed_device, rgcn_topk_typed_device) against the mirror of
tests/typed_negatives_reference.py, bit for bit.  The statistics and the decision's corner cases are asserted on the
mirror and on the C++ text without a GPU (tests/test_typed_negatives_host.py); here the device has to produce the
mirror's bytes.  V = 67 (the last mask word is partial), 31 (one partial word) and 257 (past the 256-lane stride), R = 5.

The queries run on a code table of small integers (test_gpu_topk.table_engine), so every energy is an integer the host
computes exactly, whatever kernel the GEMM chose and however the call was chunked."""
import ctypes as C

import numpy as np
import pytest

import exclusive_negatives_reference as xref
import oracle
import typed_negatives_reference as ref
from test_gpu_topk import csr, table_engine

pytestmark = pytest.mark.gpu

STATUS_INVALID, STATUS_STATE, STATUS_UNSUPPORTED = 1, 4, 5
R = 5
GUARD = -77


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def _refused(native, call, status):
    with pytest.raises(native.RgcnError) as err:
        call()
    assert err.value.status == status, (err.value.status, status)


def _valid(batch, V):
    """the rows of a case's batch that a train step accepts (the cases carry two rows with an id out of range)"""
    return np.ascontiguousarray(batch[(batch >= 0).all(axis=1) & (batch[:, [0, 2]] < V).all(axis=1) & (batch[:, 1] < R)])


def _sample(native, eng, batch, rate, seed, exclusive, typed=True):
    """(X, Y) of one stand-alone sampling call, with 64 guard rows behind the last one"""
    n, total = len(batch), len(batch) * (rate + 1)
    bufs = (eng.to_device(batch), eng.to_device(np.full((total + 64, 3), GUARD, dtype=np.int32)),
            eng.to_device(np.full(total + 64, GUARD, dtype=np.float32)))
    try:
        if typed:
            eng.negative_sample_typed_device(bufs[0], n, rate, seed, bufs[1], bufs[2], exclusive=exclusive)
        else:
            eng.negative_sample_device(bufs[0], n, rate, seed, bufs[1], bufs[2], exclusive=exclusive)
        X, Y = bufs[1].download(np.int32, (total + 64, 3)), bufs[2].download(np.float32, (total + 64,))
    finally:
        for b in bufs:
            b.free()
    assert (X[total:] == GUARD).all() and (Y[total:] == GUARD).all()          # nothing written behind the last row
    return X[:total], Y[:total]


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_device_equals_the_mirror(native, name):
    """plain and exclusive typed output, byte for byte, at 255, 256 and 257 rows and at V = 31, 67, 257; both counters;
    the OPEN counter is a total since the reserve and a new T restarts it"""
    c = ref.case(name)
    V, n, rate, seed, sets = c["V"], len(c["batch"]), c["rate"], c["seed"], c["sets"]
    K = {tuple(t) for t in c["known"].tolist()}
    tiled = np.tile(c["batch"], (rate, 1))
    with native.Engine(V, R, 8, 1, "block", 2, max_edges=16) as eng:
        eng.type_sets_reserve(c["T"])
        eng.known_positives_reserve(c["known"])
        assert eng.negative_typed_open() == 0
        opened = 0
        for exclusive in (False, True):
            m = c["exclusive" if exclusive else "plain"]
            before = eng.negative_unresolved()
            X, Y = _sample(native, eng, c["batch"], rate, seed, exclusive)
            assert X.tobytes() == m["X"].tobytes() and Y.tobytes() == m["Y"].tobytes()
            opened += m["open_count"]
            assert eng.negative_typed_open() == opened
            assert eng.negative_unresolved() - before == m["unresolved_count"]
            # on the device's own output: a typed row's new entity is in its list and is not the row's own
            neg = X[n:]
            for j in np.flatnonzero(~m["open"]):
                coin = int(m["coin"][j])
                e, own = (neg[j, 2], tiled[j, 2]) if coin else (neg[j, 0], tiled[j, 0])
                assert e != own and int(e) in ref.candidate_set(sets, coin, int(tiled[j, 1]))
            if exclusive:
                # no row is a known positive unless the counter of unresolved rows counted it
                in_K = np.array([tuple(t) in K for t in neg.tolist()])
                assert not in_K[m["unresolved"] == 0].any()
        if rate:
            assert c["plain"]["open_count"] > 0 and (~c["plain"]["open"]).any()
        eng.type_sets_reserve(c["T"])                                     # a new T starts the count over
        assert eng.negative_typed_open() == 0


@pytest.mark.parametrize("V", [31, 67])
def test_all_open_sets_reproduce_the_other_samplers(native, V):
    """T with one triple per relation: every list is a singleton, so every list is open -- the output is
    rgcn_negative_sample_device's (exclusive: rgcn_negative_sample_exclusive_device's) byte for byte, every negative row is
    counted open"""
    rng = np.random.RandomState(V)
    T = np.array([(r + 1, r, r + 2) for r in range(R - 1)], dtype=np.int32)          # (relation R - 1 is absent)
    n, rate = 100, 3
    batch = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), rng.randint(0, V, n)], 1).astype(np.int32)
    known = np.stack([rng.randint(0, V, 4000), rng.randint(0, R, 4000), rng.randint(0, V, 4000)], 1).astype(np.int32)
    with native.Engine(V, R, 8, 1, "block", 2, max_edges=16) as eng:
        eng.type_sets_reserve(T)
        eng.known_positives_reserve(known)
        for exclusive in (False, True):
            before = eng.negative_typed_open()
            X, Y = _sample(native, eng, batch, rate, 77, exclusive)
            Xo, Yo = _sample(native, eng, batch, rate, 77, exclusive, typed=False)
            assert X.tobytes() == Xo.tobytes() and Y.tobytes() == Yo.tobytes()
            assert eng.negative_typed_open() - before == n * rate
        assert not np.array_equal(X, _sample(native, eng, batch, rate, 77, False)[0])      # (the exclusive redraws are there)


def test_embedding_kind(native):
    """the stand-alone call, the counter and the reserve on an RGCN_KIND_EMBEDDING context"""
    c = ref.case("v67_255")
    with native.Engine(c["V"], R, 8, 0, "embedding", 1, max_edges=0) as eng:
        eng.type_sets_reserve(c["T"])
        eng.known_positives_reserve(c["known"])
        X, Y = _sample(native, eng, c["batch"], c["rate"], c["seed"], True)
        assert np.array_equal(X, c["exclusive"]["X"]) and np.array_equal(Y, c["exclusive"]["Y"])
        assert eng.negative_typed_open() == c["exclusive"]["open_count"]


# ------------------------------------------------------------------ the fused step
@pytest.mark.parametrize("temperature", [0.0, 1.0], ids=["plain_loss", "adversarial"])
def test_fused_step_draws_from_the_lists_when_the_mode_is_on(native, temperature):
    """rgcn_train_step_minibatch_device under rgcn_set_typed_negatives: the scratch is the stand-alone typed call's output
    (exclusive iff rgcn_set_exclusive_negatives), the loss that of rgcn_train_step_device fed those X / Y and the graph the
    dropout kernel drew, on an identically initialised context, bitwise -- once with AdversarialTemperature on as well.
    With the mode off the scratch and the loss are the plain sampler's again.  Block context, V 67, R 5, d 20, L 2."""
    c = ref.case("v67_255")
    V, d, L, nb, rate, keep = c["V"], 20, 2, 4, 3, 50
    batch = _valid(c["batch"], V)                       # (the two rows with a bad id leave: the step rejects them)
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
            e.type_sets_reserve(c["T"])
            e.known_positives_reserve(c["known"])
        if temperature:
            eng.set_adversarial_negatives(temperature)
            other.set_adversarial_negatives(temperature, n)
        bd, xd, yd = eng.to_device(batch), native.DeviceBuffer(eng, 12 * N), native.DeviceBuffer(eng, 4 * N)
        obd, ox, oy = other.to_device(batch), native.DeviceBuffer(other, 12 * N), native.DeviceBuffer(other, 4 * N)
        gd = native.DeviceBuffer(other, 12 * n)
        bufs += [bd, xd, yd, obd, ox, oy, gd]
        # mode off (the default): the plain sampler's bytes
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        plain_loss = eng.loss()
        Xoff = xd.download(np.int32, (N, 3))
        assert np.array_equal(Xoff, xref.plain(batch, rate, V, nseed)[0])
        assert eng.negative_typed_open() == 0
        for exclusive in (False, True):
            eng.set_exclusive_negatives(exclusive)
            eng.set_typed_negatives(True)
            opened = eng.negative_typed_open()
            eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
            loss = eng.loss()
            Xon, Yon = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
            kept = eng.graph_edges()
            m = ref.typed(c["sets"], c["known"], batch, rate, nseed, exclusive)
            assert Xon.tobytes() == m["X"].tobytes() and Yon.tobytes() == m["Y"].tobytes()
            assert eng.negative_typed_open() - opened == m["open_count"]
            assert not np.array_equal(Xon, Xoff)
            # the same step from its pieces on the other context: the rows the dropout kernel drew, the stand-alone typed
            # call, rgcn_train_step_device (no optimizer is configured: the weights have not moved)
            other.set_graph_dropout_device(obd, n, keep, seed=eseed)
            assert np.array_equal(other.graph_edges(), kept)
            other.copy_to_device(gd, other.graph_edges())
            other.negative_sample_typed_device(obd, n, rate, nseed, ox, oy, exclusive=exclusive)
            assert np.array_equal(ox.download(np.int32, (N, 3)), Xon) and np.array_equal(oy.download(np.float32, (N,)), Yon)
            other.train_step_device(gd, keep, ox, oy, N, seed=seed, reg_param=0.01)
            assert loss == other.loss()
            assert loss != plain_loss
        # off again: the parent's bytes; and released sets switch the mode off by themselves
        eng.set_exclusive_negatives(False)
        eng.set_typed_negatives(False)
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        assert eng.loss() == plain_loss and np.array_equal(xd.download(np.int32, (N, 3)), Xoff)
        eng.set_typed_negatives(True)
        eng.type_sets_reserve(np.zeros((0, 3), dtype=np.int32))
        eng.train_step_minibatch_device(bd, n, keep, eseed, rate, nseed, xd, yd, seed=seed, reg_param=0.01)
        assert eng.loss() == plain_loss and np.array_equal(xd.download(np.int32, (N, 3)), Xoff)
    finally:
        for b in bufs:
            b.free()
        eng.close()
        other.close()


def test_relation_rows_stay_behind_the_typed_entity_rows(native):
    """rgcn_set_relation_negatives with the typed mode on: rows [0, n (rate + 1)) are the typed call's, the relation rows
    behind them are the ones rgcn_negative_sample_relation_device writes"""
    c = ref.case("v67_255")
    V, rate, m_rel = c["V"], 2, 2
    batch = _valid(c["batch"], V)
    n = len(batch)
    first, N = n * (rate + 1), n * (rate + 1 + m_rel)
    with native.Engine(V, R, 20, 2, "block", 4, max_edges=n) as eng:
        eng.set_params(oracle.init_params(V, R, 20, 2, "block", 4, rng=np.random.RandomState(2)))
        eng.decoder_reserve(N)
        eng.type_sets_reserve(c["T"])
        bd, xd, yd = eng.to_device(batch), native.DeviceBuffer(eng, 12 * N), native.DeviceBuffer(eng, 4 * N)
        x2, y2 = native.DeviceBuffer(eng, 12 * N), native.DeviceBuffer(eng, 4 * N)
        eng.set_typed_negatives(True)
        eng.set_relation_negatives(m_rel)
        eng.train_step_minibatch_device(bd, n, n // 2, 5, rate, 19, xd, yd, seed=3, reg_param=0.01)
        assert np.isfinite(eng.loss())
        X, Y = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        assert np.array_equal(X[:first], ref.typed(c["sets"], c["known"], batch, rate, 19, False)["X"])
        eng.negative_sample_device(bd, n, rate, 19, x2, y2, relation_rate=m_rel)
        assert np.array_equal(X[first:], x2.download(np.int32, (N, 3))[first:])
        assert (Y[:n] == 1).all() and (Y[n:] == 0).all()
        assert (X[first:, 1] != np.tile(batch[:, 1], m_rel)).all()
        for b in (bd, xd, yd, x2, y2):
            b.free()


# ------------------------------------------------------------------ ranks and top-k
def _query_case(native, V, scale, seed, all_open=False):
    """(engine on an integer code table after a forward, T, its sets, the exact energies function)"""
    rng = np.random.RandomState(seed)
    half = 4
    codes = rng.randint(-1, 2, size=(V, half)).astype(np.float32)
    rel = (rng.randint(-2, 3, size=(R, half)) * scale).astype(np.float32)
    T = np.array([(r + 1, r, r + 2) for r in range(R)], dtype=np.int32) if all_open else ref.typed_graph(V, R, seed)
    eng, _ = table_engine(native, codes, rel)
    eng.type_sets_reserve(T)

    def energies(queries, predict_object):
        given = queries[:, 0] if predict_object else queries[:, 2]
        return ((codes[given] * rel[queries[:, 1]]) @ codes.T).astype(np.float32)
    return eng, T, ref.build_sets(T, V, R), energies


def _queries(T, V, n, seed):
    """training triples (gold inside its list), random rows (gold mostly outside), repeated rows"""
    rng = np.random.RandomState(seed)
    q = np.concatenate([T[rng.randint(0, len(T), n // 2)],
                        np.stack([rng.randint(0, V, n - n // 2), rng.randint(0, R, n - n // 2),
                                  rng.randint(0, V, n - n // 2)], 1).astype(np.int32)])
    q[:3] = q[1]
    return np.ascontiguousarray(q[rng.permutation(n)])


def _lists(queries, V, rng, every_third_empty):
    """per row: random entities, inside and outside the row's list, duplicates included for the exclusions"""
    out = []
    for i in range(len(queries)):
        if every_third_empty and i % 3 == 0:
            out.append([])
            continue
        out.append(rng.permutation(V)[:rng.randint(0, max(2, V // 2))].tolist())
    return out


@pytest.mark.parametrize("V,scale", [(67, 1), (67, 20), (31, 1), (257, 1), (257, 20)])
def test_typed_ranks_equal_the_mirror(native, V, scale):
    """raw and filtered ranks on every row, both sides, one chunk and chunked (reserve 7 for 40 queries): gold entities
    outside their list, filter entries outside the list, and with scale 20 (every positive energy is at least 20: its fp32 sigmoid is 1) saturated scores that tie"""
    eng, T, sets, energies = _query_case(native, V, scale, seed=V + scale)
    try:
        queries = _queries(T, V, 40, 3)
        rng = np.random.RandomState(4)
        for predict_object in (True, False):
            lists = _lists(queries, V, rng, False)
            for i, q in enumerate(queries.tolist()):                  # the gold entity is in its own filter list
                gold = q[2] if predict_object else q[0]
                if gold not in lists[i]:
                    lists[i].append(gold)
            ptr, flat = csr(lists)
            E = energies(queries, predict_object)
            want_raw, want_filt = ref.typed_ranks_from_energies(sets, E, queries, predict_object, lists)
            eng.rank_reserve(len(queries))
            raw, filt = eng.ranks_typed(queries, predict_object, ptr, flat)
            assert np.array_equal(eng.read_buffer(native.BUF_RANK_ENERGIES)[:len(queries)], E)
            assert raw.dtype == np.int32 and np.array_equal(raw, want_raw), np.flatnonzero(raw != want_raw)[:8]
            assert np.array_equal(filt, want_filt), np.flatnonzero(filt != want_filt)[:8]
            assert (filt >= 1).all() and (filt <= raw).all()
            # the open ranks of the same rows are never better
            open_raw, open_filt = eng.ranks(queries, predict_object, ptr, flat)
            assert (raw <= open_raw).all() and (filt <= open_filt).all() and (raw < open_raw).any()
            # the cases the rows are there for
            side = 1 if predict_object else 0
            gold = queries[:, 2] if predict_object else queries[:, 0]
            inside = np.array([int(g) in ref.candidate_set(sets, side, int(r)) for g, r in zip(gold, queries[:, 1])])
            assert inside.any() and (~inside).any()
            assert any(set(l) - ref.candidate_set(sets, side, int(q[1])) for l, q in zip(lists, queries))
            if scale == 20:
                by_energy = np.array([sum(1 for e in ref.candidate_set(sets, side, int(q[1])) | {int(g)} if E[i, e] >= E[i, g])
                                      for i, (q, g) in enumerate(zip(queries, gold))])
                assert (by_energy != want_raw).any()                  # saturated scores tie where energies do not
    finally:
        eng.close()
    # chunked: a reserve of 7 walks the 40 queries in six chunks (a fresh engine, since a reserve never shrinks); the
    # subject side, whose lists and mirror ranks the loop above left behind
    eng, T, sets, energies = _query_case(native, V, scale, seed=V + scale)
    try:
        eng.rank_reserve(7)
        raw, filt = eng.ranks_typed(queries, False, ptr, flat)
        assert np.array_equal(raw, want_raw) and np.array_equal(filt, want_filt)
    finally:
        eng.close()


@pytest.mark.parametrize("V", [31, 67, 257])
def test_typed_topk_equals_the_mirror(native, V):
    """idx equal and energy bitwise equal on every row, both sides: k above the length of most lists (rows end in
    (-1, -inf)), k = 1, exclusion lists that overlap the complement of the list and the list itself, and no list"""
    eng, T, sets, energies = _query_case(native, V, 1, seed=V + 7)
    try:
        queries = _queries(T, V, 30, 5)
        eng.rank_reserve(len(queries))
        rng = np.random.RandomState(6)
        for predict_object in (True, False):
            lists = _lists(queries, V, rng, True)
            blank = queries.copy()
            blank[:, 2 if predict_object else 0] = -1                 # the predicted column is not read
            E = energies(queries, predict_object)
            short = 0
            for k in (1, 5, min(V, 40)):
                for excluded in (None, lists):
                    ptr, flat = csr(excluded) if excluded is not None else (None, None)
                    idx, energy = eng.topk_typed(blank, predict_object, k, ptr, flat)
                    want_idx, want_energy = ref.typed_topk_from_energies(sets, E, queries, predict_object, k, excluded)
                    assert idx.dtype == np.int32 and energy.dtype == np.float32
                    assert np.array_equal(idx, want_idx), (k, excluded is not None, np.flatnonzero((idx != want_idx).any(1))[:5])
                    assert np.array_equal(energy.view(np.uint32), want_energy.view(np.uint32))
                    short += int((idx[:, -1] == -1).sum())
                    side = 1 if predict_object else 0
                    for i, row in enumerate(idx.tolist()):
                        allowed = ref.candidate_set(sets, side, int(queries[i, 1]))
                        assert all(e in allowed for e in row if e >= 0)
            assert short > 0                                          # rows with fewer than k members left
            if V > 31:
                full = eng.topk(blank, predict_object, 5)[0]
                assert not np.array_equal(full, eng.topk_typed(blank, predict_object, 5)[0])
    finally:
        eng.close()


@pytest.mark.parametrize("V", [31, 67])
def test_all_open_sets_reproduce_the_open_ranks_and_topk(native, V):
    """every list a singleton: rgcn_rank_typed_device and rgcn_topk_typed_device return rgcn_rank_device's and
    rgcn_topk_device's bytes"""
    eng, T, sets, energies = _query_case(native, V, 10, seed=V, all_open=True)
    try:
        queries = _queries(T, V, 30, 8)
        rng = np.random.RandomState(9)
        lists = _lists(queries, V, rng, True)
        ptr, flat = csr(lists)
        eng.rank_reserve(len(queries))
        for predict_object in (True, False):
            a, b = eng.ranks_typed(queries, predict_object, ptr, flat), eng.ranks(queries, predict_object, ptr, flat)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            for k in (1, V):
                for p, f in ((None, None), (ptr, flat)):
                    a, b = eng.topk_typed(queries, predict_object, k, p, f), eng.topk(queries, predict_object, k, p, f)
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    finally:
        eng.close()


# ------------------------------------------------------------------ statuses
def test_states(native):
    c = ref.case("v67_255")
    V = c["V"]
    batch = _valid(c["batch"], V)[:50]
    n, rate = len(batch), 1
    want = ref.typed(c["sets"], c["known"], batch, rate, 3, False)["X"]
    eng = native.Engine(V, R, 8, 1, "block", 2, max_edges=len(c["T"]))
    bufs = []
    try:
        eng.set_params(oracle.init_params(V, R, 8, 1, "block", 2, rng=np.random.RandomState(2)))
        eng.decoder_reserve(2 * n)
        bd, xd, yd = eng.to_device(batch), native.DeviceBuffer(eng, 12 * 2 * n), native.DeviceBuffer(eng, 4 * 2 * n)
        bufs += [bd, xd, yd]
        eng.set_graph(c["T"])
        eng.forward(train=False)
        eng.rank_reserve(8)
        queries = c["T"][:8]
        ptr, flat = csr([[int(q[2])] for q in queries])
        # before a reserve
        for call in (lambda: eng.negative_sample_typed_device(bd, n, rate, 3, xd, yd),
                     lambda: eng.set_typed_negatives(True), eng.negative_typed_open,
                     lambda: eng.ranks_typed(queries, True, ptr, flat), lambda: eng.topk_typed(queries, True, 3)):
            _refused(native, call, STATUS_STATE)
        eng.set_typed_negatives(False)                                   # switching off needs nothing
        eng.type_sets_reserve(c["T"])
        # exclusive without an index of known positives
        _refused(native, lambda: eng.negative_sample_typed_device(bd, n, rate, 3, xd, yd, exclusive=True), STATUS_STATE)
        # a reserve with a bad id: refused naming the row, and the earlier sets still answer
        for bad in ((V, 0, 1), (1, R, 1), (1, 0, -1)):
            with pytest.raises(native.RgcnError) as err:
                eng.type_sets_reserve(np.array([(1, 0, 1), bad], dtype=np.int32))
            assert err.value.status == STATUS_INVALID and "triple 1" in str(err.value)
        eng.negative_sample_typed_device(bd, n, rate, 3, xd, yd)
        assert np.array_equal(xd.download(np.int32, (2 * n, 3)), want)
        # bad ids in the queries, and one NULL pointer of the exclusion list
        bad_q = queries.copy()
        bad_q[2, 1] = R
        _refused(native, lambda: eng.ranks_typed(bad_q, True, ptr, flat), STATUS_INVALID)
        _refused(native, lambda: eng.topk_typed(bad_q, True, 3), STATUS_INVALID)
        bad_q = queries.copy()
        bad_q[1, 0] = V
        _refused(native, lambda: eng.ranks_typed(bad_q, True, ptr, flat), STATUS_INVALID)
        _refused(native, lambda: eng.ranks_typed(queries, True, ptr, np.array([V] * len(flat), dtype=np.int32)), STATUS_INVALID)
        qd, od = eng.to_device(queries), native.DeviceBuffer(eng, 8 * 8 * 3)
        pd = eng.to_device(ptr)
        bufs += [qd, od, pd]
        out_e = C.c_void_p(od.ptr.value + 4 * 8 * 3)
        assert eng.lib.rgcn_topk_typed_device(eng.ctx, qd.ptr, 8, 1, 3, pd.ptr, None, od.ptr, out_e) == STATUS_INVALID
        assert eng.lib.rgcn_topk_typed_device(eng.ctx, qd.ptr, 8, 1, 3, None, pd.ptr, od.ptr, out_e) == STATUS_INVALID
        assert eng.lib.rgcn_rank_typed_device(eng.ctx, qd.ptr, 8, 1, None, None, od.ptr, out_e) == STATUS_INVALID
        assert eng.lib.rgcn_topk_typed_device(eng.ctx, qd.ptr, 8, 1, 0, None, None, od.ptr, out_e) == STATUS_INVALID
        # during a capture: the reserve, the stand-alone call, the switch, the queries and the step with the mode on
        eng.set_typed_negatives(True)
        eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 3, xd, yd)
        assert np.isfinite(eng.loss()) and np.array_equal(xd.download(np.int32, (2 * n, 3)), want)
        eng.sync()
        eng.capture_begin()
        _refused(native, lambda: eng.type_sets_reserve(c["T"]), STATUS_STATE)
        _refused(native, lambda: eng.negative_sample_typed_device(bd, n, rate, 3, xd, yd), STATUS_STATE)
        _refused(native, lambda: eng.set_typed_negatives(False), STATUS_STATE)
        assert eng.lib.rgcn_rank_typed_device(eng.ctx, qd.ptr, 8, 1, pd.ptr, pd.ptr, od.ptr, out_e) == STATUS_STATE
        assert eng.lib.rgcn_topk_typed_device(eng.ctx, qd.ptr, 8, 1, 3, None, None, od.ptr, out_e) == STATUS_STATE
        _refused(native, lambda: eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 3, xd, yd), STATUS_STATE)
        eng.negative_sample_device(bd, n, rate, 3, xd, yd)                   # (something to capture)
        eng.graph_destroy(eng.capture_end())
        # num_triples = 0 releases the sets, and the mode is off
        eng.type_sets_reserve(np.zeros((0, 3), dtype=np.int32))
        _refused(native, lambda: eng.negative_sample_typed_device(bd, n, rate, 3, xd, yd), STATUS_STATE)
        _refused(native, lambda: eng.set_typed_negatives(True), STATUS_STATE)
        _refused(native, eng.negative_typed_open, STATUS_STATE)
        eng.train_step_minibatch_device(bd, n, n // 2, 1, rate, 3, xd, yd)
        assert np.array_equal(xd.download(np.int32, (2 * n, 3)), xref.plain(batch, rate, V, 3)[0])
    finally:
        for b in bufs:
            b.free()
        eng.close()
    # a relation-sharded context: the sets and the stand-alone call are there, the fused mode is not
    with native.Engine(V, R, 8, 1, "block", 2, max_edges=n, rank=0, world=2) as sharded:
        sharded.type_sets_reserve(c["T"])
        _refused(native, lambda: sharded.set_typed_negatives(True), STATUS_UNSUPPORTED)
        sharded.set_typed_negatives(False)
