"""Relation queries on the device (include/rgcn.h rgcn_rank_relation_device, rgcn_topk_relation_device,
rgcn_score_relation_queries_device) -- `-m gpu`, through the C ABI and the plugin chain.  The project's layering: the
energies the device scored (RGCN_BUF_RELATION_ENERGIES) lie within the forward error bound of float64
(tests/relation_query_reference.py), and ranks and top-k are EXACT functions of those energies (the same reference's
ranks, tests/topk_reference.py's selection)."""
import ctypes as C

import numpy as np
import pytest

from helpers import make_case
from relation_query_reference import (energy_order_ranks, float64_relation_energies, known_relation_lists,
                                      relation_ranks_from_energies, sigmoid_f32)
from test_gpu_topk import (assert_rows_equal_reference, assert_within_float64_bound, csr, random_case_engine,
                           table_engine)

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 4
# (V, R, d, blocks, edges, scale of W_relation): R = 257 puts a column past the row kernels' 256-thread stride and past
# a 128-wide GEMM tile, R = 1 is the degenerate table, scale 40 saturates the sigmoids
SHAPES = [(300, 257, 40, 8, 1500, 1.0), (90, 5, 20, 4, 400, 1.0), (1031, 1, 20, 4, 3000, 1.0)]
# the same shape on a seeded code table (table_engine: codes [c, 0] with c ~ N(0, 1), d = 40) whose relation rows are
# scaled by 40: energies of standard deviation ~180, so the fp32 sigmoids saturate at both ends
SATURATED = (300, 257, 40, 0, 1500, 40.0)
WIDE = (1200, 1100, 8, 2, 2500, 1.0)          # k = 1024 < R


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def case_engine(native, V, R, d, nb, E, scale, seed):
    """(engine after a test-mode forward, {"W_relation": ...}, triples) of a shape above"""
    if (V, R, d, nb, E, scale) != SATURATED:
        return random_case_engine(native, V, R, d, nb, E, scale, seed)
    rng = np.random.RandomState(40)
    c = rng.randn(V, d // 2).astype(np.float32)
    rel = (rng.randn(R, d // 2) * scale).astype(np.float32)
    triples = np.stack([rng.randint(0, V, E), rng.randint(0, R, E), rng.randint(0, V, E)], 1).astype(np.int32)
    eng, w_rel = table_engine(native, c, rel)
    return eng, {"W_relation": w_rel}, triples


def pick_queries(triples, n, seed):
    rng = np.random.RandomState(seed)
    queries = triples[rng.choice(len(triples), n, replace=False)].copy()
    queries[:5] = queries[3]                                          # repeated queries
    return queries


def filter_lists(queries, triples, R, rng):
    """per row: the relations known between the pair (the gold one among them) plus random extras, each once"""
    known = known_relation_lists(triples)
    out = []
    for s, r, o in queries:
        lst = list(known[(int(s), int(o))])
        for extra in rng.randint(0, R, size=rng.randint(0, max(2, R // 4))):
            if int(extra) not in lst:
                lst.append(int(extra))
        out.append(lst)
    return out


def exclusion_lists(queries, triples, R, rng):
    """per row: the known relations of the pair and random extras, duplicates included; every third row excludes nothing"""
    known = known_relation_lists(triples)
    out = []
    for i, (s, r, o) in enumerate(queries):
        if i % 3 == 0:
            out.append([])
            continue
        extra = rng.randint(0, R, size=rng.randint(0, max(2, R // 4)))
        out.append(list(known.get((int(s), int(o)), [])) + list(extra) + list(extra[:3]))
    return out


def blank_relation(queries, value=-1):
    q = queries.copy()
    q[:, 1] = value
    return q


def relation_energies(native, eng, n, R):
    energies = eng.read_buffer(native.BUF_RELATION_ENERGIES)[:n]
    assert energies.shape == (n, R) and energies.dtype == np.float32
    return energies


def ks_for(R):
    return sorted({1, 10, 64, min(257, R), min(R, 1024)} & set(range(1, R + 1)))


# ------------------------------------------------------------------ energies
@pytest.mark.parametrize("V,R,d,nb,E,scale", SHAPES)
def test_relation_energies_lie_within_the_float64_bound(native, V, R, d, nb, E, scale):
    """every entry of RGCN_BUF_RELATION_ENERGIES after score_relation_queries, 100 queries; the r column is not read"""
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, scale, seed=E + 11)
    try:
        queries = pick_queries(triples, 100, 5)
        eng.rank_reserve(len(queries))
        assert eng.relation_energies_device() is None                 # nobody has asked yet
        eng.score_relation_queries(blank_relation(queries))
        assert eng.relation_energies_device() is not None
        got = relation_energies(native, eng, len(queries), R)
        E64, bound = float64_relation_energies(eng.codes(), params["W_relation"], queries, R)
        assert (np.abs(got.astype(np.float64) - E64) <= bound).all(), float(np.max(np.abs(got - E64) - bound))
        assert np.abs(E64).max() > 0
    finally:
        eng.close()


# ------------------------------------------------------------------ ranks
@pytest.mark.parametrize("V,R,d,nb,E,scale", SHAPES + [SATURATED])
def test_relation_ranks_are_bit_exact_on_the_devices_own_energies(native, V, R, d, nb, E, scale):
    """raw and filtered equal the reference computed from the read-back energies on every row.  With W_relation scaled
    by 40 (SATURATED) the saturated sigmoids tie and change the rank: at least 30 % of the rows must differ from the
    rank by energy order, or the case has stopped testing the tie rule.  R = 1: every rank is 1."""
    eng, params, triples = case_engine(native, V, R, d, nb, E, scale, seed=E + 12)
    try:
        queries = pick_queries(triples, 100, 6)
        lists = filter_lists(queries, triples, R, np.random.RandomState(3))
        ptr, flat = csr(lists)
        eng.rank_reserve(len(queries))
        raw, filt = eng.ranks_relation(queries, ptr, flat)
        energies = relation_energies(native, eng, len(queries), R)
        want_raw, want_filt = relation_ranks_from_energies(energies, queries[:, 1], lists)
        assert raw.dtype == np.int32 and filt.dtype == np.int32
        assert np.array_equal(raw, want_raw), np.flatnonzero(raw != want_raw)[:8]
        assert np.array_equal(filt, want_filt), np.flatnonzero(filt != want_filt)[:8]
        assert (filt >= 1).all() and (filt <= raw).all()
        if scale == 40.0:
            changed = float(np.mean(energy_order_ranks(energies, queries[:, 1]) != want_raw))
            print("rows whose rank the saturated ties change: %.2f" % changed)
            assert changed >= 0.3, changed
        if R == 1:
            assert (raw == 1).all() and (filt == 1).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ top-k
@pytest.mark.parametrize("V,R,d,nb,E,scale", SHAPES + [SATURATED, WIDE])
def test_relation_topk_is_bit_exact_on_the_devices_own_energies(native, V, R, d, nb, E, scale):
    """idx equal and energy bitwise equal to topk_from_energies on every row: k in {1, 10, 64, min(257, R), min(R, 1024)}
    (those that R admits), with and without exclusion lists, the unread r column set to -1; a second call returns the
    same bytes"""
    eng, params, triples = case_engine(native, V, R, d, nb, E, scale, seed=E + 13)
    try:
        queries = pick_queries(triples, 100, 7)
        lists = exclusion_lists(queries, triples, R, np.random.RandomState(11))
        q = blank_relation(queries)
        eng.rank_reserve(len(queries))
        for k in ks_for(R):
            for excluded in (None, lists):
                ptr, flat = csr(excluded) if excluded is not None else (None, None)
                idx, energy = eng.topk_relation(q, k, ptr, flat)
                energies = relation_energies(native, eng, len(queries), R)
                assert_rows_equal_reference(energies, idx, energy, k, excluded, ("relation", R, k, excluded is not None))
                again = eng.topk_relation(q, k, ptr, flat)
                assert np.array_equal(again[0], idx) and np.array_equal(again[1].view(np.uint32), energy.view(np.uint32))
    finally:
        eng.close()


@pytest.mark.parametrize("V,R", [(1031, 300), (300, 257)])
def test_relation_ties_at_the_threshold_go_to_the_lowest_ids(native, V, R):
    """Codes and relation rows uniform in {-1, 0, 1}, d = 20: every energy is a small integer and dozens of relations tie
    with the k-th best.  At least 30 % of the rows must have a tie straddling position k."""
    rng = np.random.RandomState(V)
    half, n = 20, 120
    c = rng.randint(-1, 2, size=(V, half)).astype(np.float32)
    rel = rng.randint(-1, 2, size=(R, half)).astype(np.float32)
    eng, _ = table_engine(native, c, rel)
    try:
        queries = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), rng.randint(0, V, n)], 1).astype(np.int32)
        lists = exclusion_lists(queries, queries, R, rng)
        eng.rank_reserve(n)
        for k in (10, 64):
            for excluded in (None, lists):
                ptr, flat = csr(excluded) if excluded is not None else (None, None)
                idx, energy = eng.topk_relation(blank_relation(queries), k, ptr, flat)
                energies = relation_energies(native, eng, n, R)
                assert np.array_equal(energies, np.round(energies))              # integers, exactly
                assert_rows_equal_reference(energies, idx, energy, k, excluded, ("ties", V, R, k))
                if excluded is None:
                    ordered = -np.sort(-energies, axis=1)
                    straddle = float(np.mean(ordered[:, k - 1] == ordered[:, k]))
                    print("rows with a tie straddling position %d: %.2f" % (k, straddle))
                    assert straddle >= 0.3, (V, R, k, straddle)
    finally:
        eng.close()


def test_relation_topk_against_float64_within_the_dot_product_bound(native):
    """Every returned relation's float64 energy reaches the float64 threshold less the two bounds, and every relation
    above the threshold by more than the two bounds is returned -- on every row"""
    V, R, d, nb, E, scale = SHAPES[0]
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, scale, seed=E + 14)
    try:
        queries = pick_queries(triples, 100, 8)
        lists = exclusion_lists(queries, triples, R, np.random.RandomState(8))
        ptr, flat = csr(lists)
        E64, bound = float64_relation_energies(eng.codes(), params["W_relation"], queries, R)
        eng.rank_reserve(len(queries))
        for k in (1, 10, 64):
            idx, _ = eng.topk_relation(blank_relation(queries), k, ptr, flat)
            assert_within_float64_bound(E64, bound, idx, k, lists, ("relation", k))
    finally:
        eng.close()


@pytest.mark.parametrize("V,R,d,nb,E,scale", [SHAPES[0], SHAPES[1], SATURATED])
def test_gold_relation_position_is_consistent_with_the_filtered_rank(native, V, R, d, nb, E, scale):
    """ranks_relation with filter list F (gold among it) and topk_relation with k = R excluding F minus the gold see the
    same energies: the gold relation is answered, its position p is at most its filtered rank (the rank counts ties of
    the fp32 score against the gold, the position orders them) and equal to it when no other candidate has the gold's
    score"""
    eng, params, triples = case_engine(native, V, R, d, nb, E, scale, seed=E + 15)
    try:
        queries = pick_queries(triples, 100, 4)
        F = filter_lists(queries, triples, R, np.random.RandomState(4))
        gold = queries[:, 1]
        eng.rank_reserve(len(queries))
        ptr, flat = csr(F)
        _, filt = eng.ranks_relation(queries, ptr, flat)
        ptr, flat = csr([[r for r in f if r != g] for f, g in zip(F, gold)])
        idx, _ = eng.topk_relation(queries, R, ptr, flat)
        scores = sigmoid_f32(relation_energies(native, eng, len(queries), R))
        equal = 0
        for i, g in enumerate(gold):
            where = np.flatnonzero(idx[i] == g)
            assert len(where) == 1, (i, g)
            p = int(where[0]) + 1
            assert p <= filt[i], (i, p, filt[i])
            others = np.ones(R, dtype=bool)
            others[np.asarray(F[i], dtype=np.int64)] = False            # candidates other than the gold relation
            if not (scores[i, others] == scores[i, g]).any():
                assert p == filt[i], (i, p, filt[i])
                equal += 1
        assert equal > 0
    finally:
        eng.close()


# ------------------------------------------------------------------ chunking and the two buffers
def test_long_inputs_are_chunked_and_the_two_energy_buffers_stay_apart(native):
    """Reserve 64, ask 150: chunks of 64, 64 and 22, the relation buffer keeps the last; the results equal those of one
    chunk under a reserve of 150.  RGCN_BUF_RANK_ENERGIES keeps, byte for byte, what an entity-side score_queries left
    there across relation calls, and an entity-side call leaves the relation buffer alone."""
    V, R, d, nb, E, scale = SHAPES[0]
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, scale, seed=77)
    try:
        queries = pick_queries(triples, 150, 6)
        rng = np.random.RandomState(6)
        excl, filt_lists = exclusion_lists(queries, triples, R, rng), filter_lists(queries, triples, R, rng)
        ptr, flat = csr(excl)
        fptr, fflat = csr(filt_lists)
        eng.rank_reserve(64)
        eng.score_queries(queries[:50], True)
        entity_side = eng.read_buffer(native.BUF_RANK_ENERGIES).copy()
        assert np.abs(entity_side[:50]).max() > 0

        idx, energy = eng.topk_relation(queries, 10, ptr, flat)
        last = relation_energies(native, eng, 22, R).copy()
        assert_rows_equal_reference(last, idx[128:], energy[128:], 10, excl[128:], "last chunk")
        raw, filt = eng.ranks_relation(queries, fptr, fflat)
        assert np.array_equal(relation_energies(native, eng, 22, R).view(np.uint32), last.view(np.uint32))
        want_raw, want_filt = relation_ranks_from_energies(last, queries[128:, 1], filt_lists[128:])
        assert np.array_equal(raw[128:], want_raw) and np.array_equal(filt[128:], want_filt)
        eng.score_relation_queries(queries[128:])                     # one chunk of the same 22 queries
        assert np.array_equal(relation_energies(native, eng, 22, R).view(np.uint32), last.view(np.uint32))
        assert np.array_equal(eng.read_buffer(native.BUF_RANK_ENERGIES).view(np.uint32), entity_side.view(np.uint32))

        whole = eng.read_buffer(native.BUF_RELATION_ENERGIES).copy()
        eng.topk(queries[:40], False, 5)                              # an entity-side call
        assert np.array_equal(eng.read_buffer(native.BUF_RELATION_ENERGIES).view(np.uint32), whole.view(np.uint32))

        eng.rank_reserve(150)                                         # grows: the ranking buffers are released
        assert eng.relation_energies_device() is None
        with pytest.raises(native.RgcnError) as err:
            eng.read_buffer(native.BUF_RELATION_ENERGIES)
        assert err.value.status == STATE
        idx1, energy1 = eng.topk_relation(queries, 10, ptr, flat)
        raw1, filt1 = eng.ranks_relation(queries, fptr, fflat)
        assert np.array_equal(idx1, idx) and np.array_equal(energy1.view(np.uint32), energy.view(np.uint32))
        assert np.array_equal(raw1, raw) and np.array_equal(filt1, filt)
    finally:
        eng.close()


def test_rows_with_fewer_than_k_relations_are_padded(native):
    V, R, d, nb, E, scale = SHAPES[0]
    k = 10
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, scale, seed=9)
    try:
        rng = np.random.RandomState(1)
        queries = triples[:6].copy()
        left = [0, 1, k - 1, 0, 1, k - 1]
        lists = [list(rng.permutation(R)[:R - j]) + [3, 3] * (j == 0) for j in left]
        ptr, flat = csr(lists)
        eng.rank_reserve(8)
        idx, energy = eng.topk_relation(queries, k, ptr, flat)
        assert_rows_equal_reference(relation_energies(native, eng, 6, R), idx, energy, k, lists, "exhausted")
        for i, j in enumerate(left):
            assert (idx[i, :j] >= 0).all() and (idx[i, j:] == -1).all() and np.isneginf(energy[i, j:]).all()
    finally:
        eng.close()


# ------------------------------------------------------------------ refusals
def status_of(native, call, *args):
    try:
        call(*args)
    except native.RgcnError as err:
        return err.status
    return 0


def test_relation_query_argument_checks(native):
    """Refusals are return codes, found on the host or by the device validation that substitutes id 0 until its verdict
    is read; the engine answers a valid call afterwards.  The r column of top-k and score may hold anything."""
    V, R, d = 60, 7, 8
    params, triples, _, _ = make_case(V, R, d, 1, "block", 2, 60, seed=1)
    eng = native.Engine(V, R, d, 1, "block", 2, max_edges=60)
    try:
        eng.set_params(params)
        q = triples[:4].copy()
        ptr, flat = np.arange(5, dtype=np.int64), np.array([0, 1, 2, 3], np.int32)
        calls = {"rank": lambda x=q, p=ptr, f=flat: eng.ranks_relation(x, p, f),
                 "topk": lambda x=q, p=ptr, f=flat, k=5: eng.topk_relation(x, k, p, f),
                 "score": lambda x=q: eng.score_relation_queries(x)}
        eng.rank_reserve(4)
        for name, call in calls.items():                              # no forward yet
            assert status_of(native, call) == STATE, name
        eng.set_graph(triples)
        eng.forward(train=False)
        fresh = native.Engine(V, R, d, 1, "block", 2, max_edges=60)   # a forward, no reserve
        try:
            fresh.set_params(params)
            fresh.set_graph(triples)
            fresh.forward(train=False)
            assert status_of(native, fresh.ranks_relation, q, ptr, flat) == STATE
            assert status_of(native, fresh.topk_relation, q, 5, ptr, flat) == STATE
            assert status_of(native, fresh.score_relation_queries, q) == STATE
        finally:
            fresh.close()

        want_idx, want_energy = eng.topk_relation(q, 5, ptr, flat)
        for column in (0, 2):                                         # s or o out of range: every call
            for value in (V, -1):
                bad = q.copy()
                bad[1, column] = value
                for name, call in calls.items():
                    assert status_of(native, call, bad) == INVALID, (name, column, value)
        for value in (R, -1):                                         # the gold relation: rank only
            bad = q.copy()
            bad[2, 1] = value
            assert status_of(native, calls["rank"], bad) == INVALID, value
        for value in (V, -1, 2 ** 31 - 1):                            # the unread column: not an error
            idx, energy = eng.topk_relation(blank_relation(q, value), 5, ptr, flat)
            assert np.array_equal(idx, want_idx) and np.array_equal(energy.view(np.uint32), want_energy.view(np.uint32))
            assert status_of(native, calls["score"], blank_relation(q, value)) == 0
        for k in (0, R + 1):
            assert status_of(native, eng.topk_relation, q, k, ptr, flat) == INVALID, k
        decreasing = np.array([0, 3, 2, 4, 4], np.int64)
        assert status_of(native, calls["rank"], q, decreasing) == INVALID
        assert status_of(native, calls["topk"], q, decreasing) == INVALID
        for entry in (R, -1):                                         # a list entry out of [0, R)
            assert status_of(native, calls["rank"], q, ptr, np.array([0, 1, entry, 2], np.int32)) == INVALID
            assert status_of(native, calls["topk"], q, ptr, np.array([0, 1, entry, 2], np.int32)) == INVALID
        big = np.concatenate([q, q])[:5]                              # score: one chunk only
        assert status_of(native, calls["score"], big) == INVALID

        # straight to the C entries: one of ptr / idx NULL, and n = 0
        buf = native.DeviceBuffer(eng, 4096)
        try:
            host = np.zeros(1024, np.int32)
            host[:10].view(np.int64)[:] = ptr
            host[16:28] = q.reshape(-1)
            host[32:36] = flat
            buf.upload(host.view(np.uint8))
            at = lambda words: C.c_void_p(buf.ptr.value + 4 * words)
            lib, ctx = eng.lib, eng.ctx
            assert lib.rgcn_topk_relation_device(ctx, at(16), 4, 5, at(0), None, at(64), at(128)) == INVALID
            assert lib.rgcn_topk_relation_device(ctx, at(16), 4, 5, None, at(32), at(64), at(128)) == INVALID
            assert lib.rgcn_rank_relation_device(ctx, at(16), 4, None, at(32), at(64), at(128)) == INVALID
            assert lib.rgcn_topk_relation_device(ctx, at(16), 4, 5, at(0), at(32), at(64), at(128)) == 0
            assert lib.rgcn_rank_relation_device(ctx, at(16), 4, at(0), at(32), at(64), at(128)) == 0
            assert lib.rgcn_rank_relation_device(ctx, None, 0, None, None, None, None) == 0
            assert lib.rgcn_topk_relation_device(ctx, None, 0, 5, None, None, None, None) == 0
            assert lib.rgcn_score_relation_queries_device(ctx, None, 0) == 0
            assert lib.rgcn_score_relation_queries_device(ctx, None, -1) == INVALID
        finally:
            buf.free()
        idx, energy = eng.topk_relation(q, 5, ptr, flat)              # the engine still answers
        assert np.array_equal(idx, want_idx) and np.array_equal(energy.view(np.uint32), want_energy.view(np.uint32))
    finally:
        eng.close()


def test_more_relations_than_entities_is_unsupported(native):
    """W_relation is stored [EntityCount, d]: its first RelationCount rows are the candidates, so RelationCount above
    EntityCount is refused (status 5) before anything runs"""
    V, R, d = 8, 12, 8
    params, triples, _, _ = make_case(V, R, d, 1, "block", 2, 20, seed=2)
    eng = native.Engine(V, R, d, 1, "block", 2, max_edges=20)
    try:
        eng.set_params(params)
        eng.set_graph(triples)
        eng.forward(train=False)
        eng.rank_reserve(4)
        q = np.array([[0, 0, 1], [2, 1, 3]], np.int32)
        ptr, flat = np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32)
        assert status_of(native, eng.ranks_relation, q, ptr, flat) == 5
        assert status_of(native, eng.topk_relation, q, 3, ptr, flat) == 5
        assert status_of(native, eng.score_relation_queries, q) == 5
        assert eng.relation_energies_device() is None
    finally:
        eng.close()


# ------------------------------------------------------------------ the other context kinds and the plugin chain
def test_embedding_contexts_answer_relation_queries(native):
    """RGCN_KIND_EMBEDDING at (90, 5, 20): the codes are W_emb; energies within the bound, ranks and top-k exact on them,
    the relation buffer readable"""
    V, R, d, n = 90, 5, 20, 40
    rng = np.random.RandomState(12)
    params = {"W_emb": (rng.randn(V, d) * 0.6).astype(np.float32), "b_emb": np.zeros(d, np.float32),
              "W_relation": rng.randn(V, d).astype(np.float32)}
    queries = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), rng.randint(0, V, n)], 1).astype(np.int32)
    eng = native.Engine(V, R, d, 0, "embedding", 1)
    try:
        eng.set_params(params)
        eng.forward(train=False)
        eng.rank_reserve(n)
        lists = filter_lists(queries, queries, R, rng)
        ptr, flat = csr(lists)
        raw, filt = eng.ranks_relation(queries, ptr, flat)
        energies = relation_energies(native, eng, n, R)
        E64, bound = float64_relation_energies(params["W_emb"], params["W_relation"], queries, R)
        assert (np.abs(energies.astype(np.float64) - E64) <= bound).all()
        want_raw, want_filt = relation_ranks_from_energies(energies, queries[:, 1], lists)
        assert np.array_equal(raw, want_raw) and np.array_equal(filt, want_filt)
        for k in (1, R):
            idx, energy = eng.topk_relation(blank_relation(queries), k, ptr, flat)
            assert_rows_equal_reference(relation_energies(native, eng, n, R), idx, energy, k, lists, ("embedding", k))
    finally:
        eng.close()


def test_plugin_chain_device_relation_topk_agrees_with_the_eager_relation_scores(tmp_path):
    """A small gcn_block model built through model_builder (16 entities, 9 relations): BilinearDiag.device_relation_topk
    within the float64 bound on the model's own codes; the eager predict_all_relation_scores within the same bound
    carried through the sigmoid (slope <= 1/4) plus the rounding of the fp32 score (numpy evaluates exp, 1 + e and the
    quotient in fp32, half an ulp each of a value <= 1: 3 x 2^-24), and its ordering selects within that bound too;
    device_relation_ranks equal the reference on the eager path's float64 energies wherever the gold score is further
    from every other score than the bound."""
    import helpers
    from relationprediction_amd.common import model_builder
    from test_plugin_surface import BLOCK_EXP, load_settings
    V, R, k = 16, 9, 5
    triples = helpers.load_graph("toy_train")
    s, enc, dec = load_settings(tmp_path, BLOCK_EXP, V=V, R=R, E=len(triples))
    model = model_builder.build_decoder(model_builder.build_encoder(enc, triples), dec)
    np.random.seed(3)
    model.preprocess(triples)
    model.register_for_test(triples)
    model.initialize_train()
    queries = triples[:12].astype(np.int32)
    lists = exclusion_lists(queries, triples, R, np.random.RandomState(2))
    ptr, flat = csr(lists)
    idx, energy = model.device_relation_topk(triples, queries, k, ptr, flat)
    codes = model.get_all_codes(mode='test')
    E64, bound = float64_relation_energies(np.asarray(codes[0], dtype=np.float32), np.asarray(codes[1], dtype=np.float32),
                                           queries, R)
    assert_within_float64_bound(E64, bound, idx, k, lists, "device")
    scores = model.score_all_relations(queries)
    assert scores.shape == (len(queries), R) and scores.dtype == np.float32
    S64 = 1.0 / (1.0 + np.exp(-E64))
    score_bound = 0.25 * bound + 3 * 2.0 ** -24
    assert (np.abs(scores.astype(np.float64) - S64) <= score_bound).all()
    eager_idx = np.full((len(queries), k), -1, dtype=np.int32)
    for i in range(len(queries)):
        ids = np.setdiff1d(np.arange(R), np.asarray(lists[i], dtype=np.int64))
        order = ids[np.lexsort((ids, -scores[i, ids].astype(np.float64)))][:k]
        eager_idx[i, :len(order)] = order
    assert_within_float64_bound(S64, score_bound, eager_idx, k, lists, "eager")
    F = filter_lists(queries, triples, R, np.random.RandomState(5))
    fptr, fflat = csr(F)
    raw, filt = model.device_relation_ranks(triples, queries, fptr, fflat)
    want_raw, want_filt = relation_ranks_from_energies(E64.astype(np.float32), queries[:, 1], F)
    for i, g in enumerate(queries[:, 1]):
        gap = np.abs(S64[i] - S64[i, g])
        gap[g] = np.inf
        if (gap > 2 * score_bound[i].max() + 2.0 ** -23).all():
            assert raw[i] == want_raw[i] and filt[i] == want_filt[i], i


def test_predict_command_side_relation_end_to_end_with_a_real_checkpoint(tmp_path):
    """relationprediction_amd.predict --side relation on the reference's Toy data: a model built by the command's own
    build_model, saved with Model.save, asked through predict.main (which builds a second chain, with other initial
    weights, and loads the checkpoint) -- the lines are the first model's device_relation_topk answers, ids and fp32
    scores alike."""
    import helpers
    from relationprediction_amd import predict
    from relationprediction_amd.common import evaluation, settings_reader
    from test_plugin_surface import BLOCK_EXP
    V, R, k = 16, 9, 4
    triples = helpers.load_graph("toy_train")
    ents, rels = ["e%d" % i for i in range(V)], ["r%d" % i for i in range(R)]
    (tmp_path / "entities.dict").write_text("".join("%d\t%s\n" % (i, n) for i, n in enumerate(ents)))
    (tmp_path / "relations.dict").write_text("".join("%d\t%s\n" % (i, n) for i, n in enumerate(rels)))
    lines = ["%s\t%s\t%s\n" % (ents[s], rels[r], ents[o]) for s, r, o in triples]
    (tmp_path / "train.txt").write_text("".join(lines[:-6]))
    (tmp_path / "valid.txt").write_text("".join(lines[-6:-3]))
    (tmp_path / "test.txt").write_text("".join(lines[-3:]))
    (tmp_path / "s.exp").write_text(BLOCK_EXP)
    pairs = [(int(s), int(o)) for s, r, o in triples[:7]] + [(int(triples[0, 2]), int(triples[0, 0]))]
    (tmp_path / "q.txt").write_text("".join("%s\t%s\n" % (ents[a], ents[b]) for a, b in pairs))
    splits = {"train": triples[:-6].astype(np.int32), "valid": triples[-6:-3], "test": triples[-3:]}
    np.random.seed(7)
    model = predict.build_model(settings_reader.read(str(tmp_path / "s.exp")), splits, V, R)
    model.save(str(tmp_path / "models" / "Toy"))
    queries = np.full((len(pairs), 3), -1, dtype=np.int32)
    queries[:, 0] = [p[0] for p in pairs]
    queries[:, 2] = [p[1] for p in pairs]
    scorer = evaluation.Scorer({'Metric': 'MRR'})
    scorer.register_data(triples)
    for keep_known in (False, True):
        np.random.seed(8)                                              # the command's chain starts from other weights
        out = tmp_path / ("answers_%d.txt" % keep_known)
        predict.main(["--settings", str(tmp_path / "s.exp"), "--dataset", str(tmp_path), "--model",
                      str(tmp_path / "models" / "Toy-0.npz"), "--queries", str(tmp_path / "q.txt"), "--k", str(k),
                      "--side", "relation", "--out", str(out)] + (["--keep-known"] if keep_known else []))
        ptr, idx = (None, None) if keep_known else evaluation.known_completions_csr(pairs, scorer.known_relation_triples)
        want_idx, want_energy = model.device_relation_topk(splits["train"], queries, k, ptr, idx)
        want_score = predict.sigmoid_f32(want_energy)
        got = [l.split("\t") for l in out.read_text().splitlines()]
        want = [[ents[a], rels[r], ents[b], str(p + 1), "%.9g" % sc] for (a, b), ids, row in zip(pairs, want_idx, want_score)
                for p, (r, sc) in enumerate(zip(ids, row)) if r >= 0]
        assert got == want and len(got) > len(pairs)
