"""Top-k link prediction on the device (include/rgcn.h rgcn_topk_device) -- `-m gpu`, through the C ABI and the
plugin chain.  The selection is held BIT-EXACT to tests/topk_reference.py on the energies the device itself scored
(RGCN_BUF_RANK_ENERGIES); the energies are held to float64 within the forward error bound of a length-d fp32 dot
product."""
import numpy as np
import pytest

from helpers import make_case
from topk_reference import topk_from_energies

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def known_lists(triples, object_side):
    known = {}
    for s, r, o in triples:
        key, val = ((s, r), o) if object_side else ((o, r), s)
        lst = known.setdefault(key, [])
        if val not in lst:
            lst.append(val)
    return known


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return ptr, idx.astype(np.int32)


def exclusion_lists(queries, triples, object_side, V, rng):
    """per row: the known completions of the pair, on two rows of three with random extras (duplicates included);
    every third row excludes nothing"""
    known = known_lists(triples, object_side)
    out = []
    for i, (s, r, o) in enumerate(queries):
        if i % 3 == 0:
            out.append([])
            continue
        extra = rng.randint(0, V, size=rng.randint(0, max(2, V // 4)))
        out.append(list(known.get((s, r) if object_side else (o, r), [])) + list(extra) + list(extra[:3]))
    return out


def blank_unread(queries, object_side, value=-1):
    q = queries.copy()
    q[:, 2 if object_side else 0] = value
    return q


def table_engine(native, c, rel):
    """A one-layer chain on an empty graph whose codes are EXACTLY [c, 0] and whose relation rows are [rel, 0]
    (relu(c) - relu(-c) through an identity self-loop; tests/test_gpu_eval.py uses the same arrangement)."""
    V, half = c.shape
    R, d = rel.shape[0], 2 * half
    eye = np.eye(half, dtype=np.float32)
    w_self = np.zeros((d, d), dtype=np.float32)
    w_self[:half, :half] = eye
    w_self[half:, :half] = -eye
    w_rel = np.zeros((V, d), dtype=np.float32)
    w_rel[:R, :half] = rel
    eng = native.Engine(V, R, d, 1, "block", d // 4, max_edges=1)
    eng.set_params({"W_emb": np.concatenate([np.maximum(c, 0), np.maximum(-c, 0)], axis=1).astype(np.float32),
                    "b_emb": np.zeros(d, np.float32), "W_f1": np.zeros((R, d // 4, 4, 4), np.float32),
                    "W_b1": np.zeros((R, d // 4, 4, 4), np.float32), "W_self1": w_self, "b1": np.zeros(d, np.float32),
                    "W_relation": w_rel})
    eng.set_graph(np.zeros((0, 3), dtype=np.int32))
    eng.forward(train=False)
    codes = eng.codes()
    assert np.array_equal(codes[:, :half], c) and not codes[:, half:].any()
    return eng, w_rel


def random_case_engine(native, V, R, d, nb, E, scale, seed):
    params, triples, _, _ = make_case(V, R, d, 2, "block", nb, E, seed=seed)
    rng = np.random.RandomState(5)
    params["W_relation"] = (rng.randn(V, d) * scale).astype(np.float32)
    eng = native.Engine(V, R, d, 2, "block", nb, max_edges=E)
    eng.set_params(params)
    eng.set_graph(triples)
    eng.forward(train=False)
    return eng, params, triples


def assert_rows_equal_reference(energies, idx, energy, k, excluded, tag):
    assert idx.shape == energy.shape == (len(energies), k) and idx.dtype == np.int32 and energy.dtype == np.float32
    for i in range(len(energies)):
        want_idx, want_energy = topk_from_energies(energies[i], k, excluded[i] if excluded is not None else ())
        assert np.array_equal(idx[i], want_idx), (tag, i, idx[i][:8], want_idx[:8])
        assert np.array_equal(energy[i].view(np.uint32), want_energy.view(np.uint32)), (tag, i)


def ks_for(V):
    return sorted({1, 10, 64, min(257, V), min(V, 1024)})


def run_bit_exact(native, eng, queries, triples, V, tag):
    rng = np.random.RandomState(11)
    eng.rank_reserve(len(queries))                                  # one chunk: the buffer holds every query's row
    for object_side in (True, False):
        lists = exclusion_lists(queries, triples, object_side, V, rng)
        q = blank_unread(queries, object_side)                        # the column being predicted is not read
        for k in ks_for(V):
            for excluded in (None, lists):
                ptr, flat = csr(excluded) if excluded is not None else (None, None)
                idx, energy = eng.topk(q, object_side, k, ptr, flat)
                energies = eng.read_buffer(native.BUF_RANK_ENERGIES)[:len(queries)]
                assert energies.shape == (len(queries), V)
                assert_rows_equal_reference(energies, idx, energy, k, excluded, (tag, object_side, k, excluded is not None))
                again = eng.topk(q, object_side, k, ptr, flat)       # the same energies: the same bytes
                assert np.array_equal(again[0], idx) and np.array_equal(again[1].view(np.uint32), energy.view(np.uint32))


@pytest.mark.parametrize("V,R,d,nb,E,scale", [(300, 11, 40, 8, 1500, 1.0), (90, 5, 20, 4, 400, 40.0),
                                              (1031, 7, 20, 4, 3000, 6.0)])
def test_topk_is_bit_exact_on_the_devices_own_energies(native, V, R, d, nb, E, scale):
    """idx equal and energy bitwise equal to topk_from_energies on every row: k in {1, 10, 64, 257, min(V, 1024)}, both
    sides, with and without exclusion lists, repeated queries, the unread column set to -1; a second call returns the
    same bytes."""
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, scale, seed=E + 1)
    try:
        rng = np.random.RandomState(5)
        queries = triples[rng.choice(len(triples), 120, replace=False)].copy()
        queries[:7] = queries[3]
        run_bit_exact(native, eng, queries, triples, V, V)
    finally:
        eng.close()


def test_topk_is_bit_exact_at_fb15k237_scale(native):
    """V = 14541 (odd: rows start at every alignment), d = 500, a seeded code table on an empty graph"""
    V, R, half = 14541, 7, 250
    rng = np.random.RandomState(2)
    eng, _ = table_engine(native, rng.randn(V, half).astype(np.float32), rng.randn(R, half).astype(np.float32))
    try:
        triples = np.stack([rng.randint(0, V, 400), rng.randint(0, R, 400), rng.randint(0, V, 400)], 1).astype(np.int32)
        queries = triples[:48].copy()
        queries[:5] = queries[2]
        run_bit_exact(native, eng, queries, triples, V, "fb237")
    finally:
        eng.close()


@pytest.mark.parametrize("V", [300, 1031])
def test_ties_at_the_threshold_go_to_the_lowest_ids(native, V):
    """Codes and relation rows uniform in {-1, 0, 1}, d = 20: every energy is a small integer, hundreds of entities
    tie with the k-th best and which of them are answered is exactly what the (energy descending, id ascending) rule
    decides.  At least 30 % of the rows must have a tie straddling position k, or the case has stopped testing it."""
    rng = np.random.RandomState(V)
    R, half, n = 5, 20, 120
    c = rng.randint(-1, 2, size=(V, half)).astype(np.float32)
    rel = rng.randint(-1, 2, size=(R, half)).astype(np.float32)
    eng, _ = table_engine(native, c, rel)
    try:
        queries = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), rng.randint(0, V, n)], 1).astype(np.int32)
        eng.rank_reserve(n)
        for object_side in (True, False):
            lists = exclusion_lists(queries, queries, object_side, V, rng)
            q = blank_unread(queries, object_side)
            for k in ks_for(V):
                for excluded in (None, lists):
                    ptr, flat = csr(excluded) if excluded is not None else (None, None)
                    idx, energy = eng.topk(q, object_side, k, ptr, flat)
                    energies = eng.read_buffer(native.BUF_RANK_ENERGIES)[:n]
                    assert np.array_equal(energies, np.round(energies))          # integers, exactly
                    assert_rows_equal_reference(energies, idx, energy, k, excluded, ("ties", V, object_side, k))
                    if excluded is None and k < V and k <= 257:
                        ordered = -np.sort(-energies, axis=1)
                        straddle = float(np.mean(ordered[:, k - 1] == ordered[:, k]))
                        assert straddle >= 0.3, (V, k, straddle)
    finally:
        eng.close()


def float64_energies(codes, w_rel, queries, object_side):
    """(E64 [n,V], bound [n,V]): the energies in float64 from the engine's codes, and the forward error bound of the
    fp32 path for each: (d + 2) 2^-24 sum_k |q_k| |codes[e,k]| -- a length-d fp32 dot product (gemm_f32 is exact fp32
    MFMA) plus the rounding of q = codes[ent] * W_relation[rel]"""
    c64 = codes.astype(np.float64)
    ent = queries[:, 0] if object_side else queries[:, 2]
    q = c64[ent] * w_rel.astype(np.float64)[queries[:, 1]]
    d = codes.shape[1]
    return q @ c64.T, (d + 2) * 2.0 ** -24 * (np.abs(q) @ np.abs(c64).T)


def assert_within_float64_bound(E64, bound, idx, k, excluded, tag):
    n, V = E64.shape
    for i in range(n):
        avail = np.ones(V, dtype=bool)
        if excluded is not None and len(excluded[i]):
            avail[np.asarray(excluded[i], dtype=np.int64)] = False
        ids = np.flatnonzero(avail)
        kk = min(k, len(ids))
        got = idx[i, :kk].astype(np.int64)
        assert (idx[i, kk:] == -1).all(), (tag, i)
        if kk == 0:
            continue
        assert (got >= 0).all() and len(set(got.tolist())) == kk and avail[got].all(), (tag, i, got[:8])
        t_id = ids[np.argsort(-E64[i, ids], kind="stable")[kk - 1]]
        t, b_t = E64[i, t_id], bound[i, t_id]
        assert (E64[i, got] >= t - bound[i, got] - b_t).all(), (tag, i)
        must = ids[E64[i, ids] > t + bound[i, ids] + b_t]
        assert set(must.tolist()) <= set(got.tolist()), (tag, i)


@pytest.mark.parametrize("V,R,d,nb,E,scale", [(300, 11, 40, 8, 1500, 1.0), (1031, 7, 20, 4, 3000, 6.0)])
def test_topk_against_float64_within_the_dot_product_bound(native, V, R, d, nb, E, scale):
    """Every returned entity's float64 energy reaches the float64 threshold less the two bounds, and every entity above
    the threshold by more than the two bounds is returned -- on every row."""
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, scale, seed=E + 2)
    try:
        rng = np.random.RandomState(8)
        queries = triples[rng.choice(len(triples), 100, replace=False)].copy()
        codes = eng.codes()
        eng.rank_reserve(len(queries))
        for object_side in (True, False):
            E64, bound = float64_energies(codes, params["W_relation"], queries, object_side)
            lists = exclusion_lists(queries, triples, object_side, V, rng)
            ptr, flat = csr(lists)
            for k in (1, 10, 64):
                idx, _ = eng.topk(blank_unread(queries, object_side), object_side, k, ptr, flat)
                assert_within_float64_bound(E64, bound, idx, k, lists, (V, object_side, k))
    finally:
        eng.close()


def sigmoid_f32(x):
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)


@pytest.mark.parametrize("V,R,d,nb,E,scale", [(300, 11, 40, 8, 1500, 1.0), (90, 5, 20, 4, 400, 40.0),
                                              (1031, 7, 20, 4, 3000, 6.0)])
def test_gold_position_is_consistent_with_the_filtered_rank(native, V, R, d, nb, E, scale):
    """Engine.ranks with filter list F (gold among it) and Engine.topk excluding F minus the gold entity see the same
    energies: the gold entity's position p is at most its filtered rank (the rank counts ties of the fp32 score against
    the gold entity, the position orders them), equal when no other candidate has the gold's score, and the gold
    entity is missing only when its filtered rank exceeds k."""
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, scale, seed=E + 3)
    try:
        rng = np.random.RandomState(4)
        queries = triples[rng.choice(len(triples), 120, replace=False)].copy()
        eng.rank_reserve(len(queries))
        absent = 0
        # k = min(V, 1024) answers (nearly) everything; k = 10 is where most gold entities fall outside the answer
        for object_side, k in ((True, min(V, 1024)), (False, min(V, 1024)), (True, 10), (False, 10)):
            known = known_lists(triples, object_side)
            gold = queries[:, 2] if object_side else queries[:, 0]
            F = [known[(s, r) if object_side else (o, r)] for s, r, o in queries]
            ptr, flat = csr(F)
            _, filt = eng.ranks(queries, object_side, ptr, flat)
            ptr, flat = csr([[e for e in f if e != g] for f, g in zip(F, gold)])
            idx, _ = eng.topk(queries, object_side, k, ptr, flat)
            scores = sigmoid_f32(eng.read_buffer(native.BUF_RANK_ENERGIES)[:len(queries)])
            for i, g in enumerate(gold):
                where = np.flatnonzero(idx[i] == g)
                if len(where) == 0:
                    assert filt[i] > k, (i, filt[i])
                    absent += 1
                    continue
                p = int(where[0]) + 1
                assert p <= filt[i], (i, p, filt[i])
                others = np.ones(V, dtype=bool)
                others[np.asarray(F[i], dtype=np.int64)] = False        # candidates other than the gold entity
                if not (scores[i, others] == scores[i, g]).any():
                    assert p == filt[i], (i, p, filt[i])
        assert absent > 0                                           # the clause above has really been exercised
    finally:
        eng.close()


def test_long_inputs_are_chunked_and_the_energy_buffer_keeps_the_last_chunk(native):
    V, R, d, nb, E = 300, 11, 40, 8, 1500
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, 1.0, seed=77)
    try:
        rng = np.random.RandomState(6)
        queries = triples[rng.choice(len(triples), 150, replace=False)].copy()
        lists = exclusion_lists(queries, triples, True, V, rng)
        ptr, flat = csr(lists)
        eng.rank_reserve(64)                                           # 150 queries: chunks of 64, 64 and 22
        idx, energy = eng.topk(queries, True, 10, ptr, flat)
        last = eng.read_buffer(native.BUF_RANK_ENERGIES)[:22].copy()
        known = known_lists(triples, True)
        rptr, rflat = csr([known[(s, r)] for s, r, o in queries[128:]])
        eng.ranks(queries[128:], True, rptr, rflat)                   # one chunk of the same 22 queries
        assert np.array_equal(eng.read_buffer(native.BUF_RANK_ENERGIES)[:22].view(np.uint32), last.view(np.uint32))
        assert_rows_equal_reference(last, idx[128:], energy[128:], 10, lists[128:], "last chunk")
        eng.rank_reserve(150)
        idx1, energy1 = eng.topk(queries, True, 10, ptr, flat)
        assert np.array_equal(idx1, idx) and np.array_equal(energy1.view(np.uint32), energy.view(np.uint32))
    finally:
        eng.close()


def test_rows_with_fewer_than_k_candidates_are_padded(native):
    V, R, d, nb, E, k = 90, 5, 20, 4, 400, 10
    eng, params, triples = random_case_engine(native, V, R, d, nb, E, 1.0, seed=9)
    try:
        rng = np.random.RandomState(1)
        queries = triples[:6].copy()
        left = [0, 1, k - 1, 0, 1, k - 1]
        lists = [list(rng.permutation(V)[:V - j]) + [3, 3] * (j == 0) for j in left]
        ptr, flat = csr(lists)
        eng.rank_reserve(8)
        idx, energy = eng.topk(queries, True, k, ptr, flat)
        energies = eng.read_buffer(native.BUF_RANK_ENERGIES)[:6]
        assert_rows_equal_reference(energies, idx, energy, k, lists, "exhausted")
        for i, j in enumerate(left):
            assert (idx[i, :j] >= 0).all() and (idx[i, j:] == -1).all() and np.isneginf(energy[i, j:]).all()
    finally:
        eng.close()


def test_topk_argument_checks(native):
    """Refusals are return codes (RgcnError), found on the host or by the device validation that substitutes id 0 until
    its verdict is read; the engine answers a valid call afterwards.  The UNREAD column may hold anything."""
    V, R, d = 1031, 3, 8
    params, triples, _, _ = make_case(V, R, d, 1, "block", 2, 60, seed=1)
    eng = native.Engine(V, R, d, 1, "block", 2, max_edges=60)
    try:
        eng.set_params(params)
        q = triples[:4].copy()
        ptr, flat = np.arange(5, dtype=np.int64), np.array([0, 1, 2, 3], np.int32)
        eng.rank_reserve(8)
        with pytest.raises(native.RgcnError) as err:                  # no forward yet
            eng.topk(q, True, 5, ptr, flat)
        assert err.value.status == 4
        eng.set_graph(triples)
        eng.forward(train=False)
        for k in (0, V + 1, 1025, -3):
            with pytest.raises(native.RgcnError) as err:
                eng.topk(q, True, k, ptr, flat)
            assert err.value.status == 1, k
        bad = q.copy(); bad[1, 0] = V                                  # a read id (subject, object side)
        with pytest.raises(native.RgcnError):
            eng.topk(bad, True, 5, ptr, flat)
        bad = q.copy(); bad[2, 1] = R
        with pytest.raises(native.RgcnError):
            eng.topk(bad, False, 5, ptr, flat)
        with pytest.raises(native.RgcnError):                          # exclusion entry out of range
            eng.topk(q, True, 5, ptr, np.array([0, 1, V + 3, 2], np.int32))
        with pytest.raises(native.RgcnError):
            eng.topk(q, True, 5, ptr, np.array([0, -1, 3, 2], np.int32))
        with pytest.raises(native.RgcnError):                          # decreasing ptr
            eng.topk(q, True, 5, np.array([0, 3, 2, 4, 4], np.int64), flat)
        for value in (V, -1, 2 ** 31 - 1):                             # the unread column: not an error
            for object_side in (True, False):
                idx, energy = eng.topk(blank_unread(q, object_side, value), object_side, 5, ptr, flat)
                want, _ = eng.topk(q, object_side, 5, ptr, flat)
                assert np.array_equal(idx, want) and (idx >= 0).all()
        small = native.Engine(50, R, d, 1, "block", 2, max_edges=60)  # k above V where V < RGCN_MAX_TOPK
        try:
            p50, t50, _, _ = make_case(50, R, d, 1, "block", 2, 60, seed=1)
            small.set_params(p50)
            small.set_graph(t50)
            small.forward(train=False)
            small.rank_reserve(4)
            with pytest.raises(native.RgcnError) as err:
                small.topk(t50[:4], True, 51)
            assert err.value.status == 1
            idx, _ = small.topk(t50[:4], True, 50)
            assert sorted(idx[0].tolist()) == list(range(50))
        finally:
            small.close()
    finally:
        eng.close()


def test_sharded_contexts_answer_their_own_query_slices(native):
    """The two-context arrangement of tests/test_gpu_eval.py: the test is the collective of the test-mode forward, then
    each rank answers ITS half of the queries.  The exchanged sum adds in another order than the single context's
    reduction, so the codes differ by roundings: position j of a row is DETERMINED when the float64 energies (of the
    unsharded codes) around it are further apart than twice the largest (dot-product bound + float64 difference
    between the two contexts' energies) of the row; there the answers must be equal, and most positions are such."""
    from relationprediction_amd.sharding import lpt_partition
    V, R, d, nb, E, L, world, k = 150, 8, 20, 4, 700, 2, 2, 10
    params, triples, _, _ = make_case(V, R, d, L, "block", nb, E, seed=31)
    queries = triples[np.random.RandomState(5).choice(E, 120, replace=False)]
    owner = lpt_partition(np.bincount(triples[:, 1], minlength=R), world)
    ref = native.Engine(V, R, d, L, "block", nb, max_edges=E)
    engs = [native.Engine(V, R, d, L, "block", nb, max_edges=E, rank=r, world=world) for r in range(world)]
    try:
        ref.set_params(params)
        ref.set_graph(triples)
        ref.forward(train=False)
        ref.rank_reserve(64)
        want, _ = ref.topk(queries, True, k)
        for e in engs:
            e.set_params(params)
            e.set_relation_owner(owner)
            e.set_graph(triples)
            e.forward_begin(train=False)
            e.rank_reserve(64)
        for l in range(1, L + 1):
            for e in engs:
                e.forward_layer_partial(l)
            total = sum(e.read_buffer(native.BUF_EXCHANGE) for e in engs)
            for e in engs:
                e.write_buffer(native.BUF_EXCHANGE, total)
                e.forward_layer_finish(l)
        Er, br = float64_energies(ref.codes(), params["W_relation"], queries, True)
        determined = total_positions = 0
        for r, e in enumerate(engs):
            mine = queries[r::world]
            got, _ = e.topk(mine, True, k)
            Es, bs = float64_energies(e.codes(), params["W_relation"], mine, True)
            assert_within_float64_bound(Es, bs, got, k, None, ("rank", r))
            for i in range(len(mine)):
                row = Er[r::world][i]
                margin = 2.0 * float(np.max(np.maximum(br[r::world][i], bs[i]) + np.abs(row - Es[i])))
                ordered = -np.sort(-row)
                gaps = ordered[:-1] - ordered[1:]                       # gaps[j]: between positions j and j + 1
                for j in range(k):
                    total_positions += 1
                    if (j == 0 or gaps[j - 1] > margin) and gaps[j] > margin:
                        determined += 1
                        assert got[i, j] == want[r::world][i, j], (r, i, j)
        assert determined > 0.5 * total_positions, (determined, total_positions)
    finally:
        for e in [ref] + engs:
            e.close()


def test_plugin_chain_device_topk_agrees_with_the_eager_predict_top(tmp_path):
    """A small gcn_block model built through model_builder: BilinearDiag.device_topk (the device path) within the
    float64 bound on the model's own codes; the eager predict_top, which orders fp32 SCORES, within the same bound
    carried through the sigmoid (slope <= 1/4) plus the rounding of the two fp32 scores it compares (numpy evaluates
    exp, 1 + e and the quotient in fp32, half an ulp each of a value <= 1: 3 x 2^-24 per score)."""
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
    for object_side in (True, False):
        lists = exclusion_lists(queries, triples, object_side, V, np.random.RandomState(2))
        ptr, flat = csr(lists)
        idx, energy = model.device_topk(triples, queries, object_side, k, ptr, flat)
        codes = model.get_all_codes(mode='test')
        w_rel = np.asarray(codes[1], dtype=np.float32)
        E64, bound = float64_energies(np.asarray(codes[0], dtype=np.float32), w_rel, queries, object_side)
        assert_within_float64_bound(E64, bound, idx, k, lists, ("device", object_side))
        for var, val in zip(model.get_test_input_variables(), (triples, queries)):
            var.feed(val)
        eager_idx, eager_scores = model.predict_top(object_side, k, ptr, flat)
        S64 = 1.0 / (1.0 + np.exp(-E64))
        assert_within_float64_bound(S64, 0.25 * bound + 3 * 2.0 ** -24, eager_idx, k, lists, ("eager", object_side))
        assert eager_scores.shape == (len(queries), k) and (np.diff(eager_scores, axis=1) <= 0).all()


def test_exclusion_mask_at_the_entity_limit(native):
    """RGCN_MAX_TOPK_ENTITIES = 2^19 entities: the row's exclusion mask is 64 KB of LDS beside the sort buffers; one
    more entity is RGCN_ERR_UNSUPPORTED (status 5), refused before anything runs."""
    V, R, d, n, k = 1 << 19, 3, 8, 4, 1024
    rng = np.random.RandomState(0)
    params = {"W_emb": rng.randn(V, d).astype(np.float32), "b_emb": np.zeros(d, np.float32),
              "W_f1": np.zeros((R, 2, 4, 4), np.float32), "W_b1": np.zeros((R, 2, 4, 4), np.float32),
              "W_self1": rng.randn(d, d).astype(np.float32), "b1": np.zeros(d, np.float32),
              "W_relation": rng.randn(V, d).astype(np.float32)}
    eng = native.Engine(V, R, d, 1, "block", 2, max_edges=1)
    try:
        eng.set_params(params)
        eng.set_graph(np.zeros((0, 3), dtype=np.int32))
        eng.forward(train=False)
        eng.rank_reserve(n)
        queries = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), np.full(n, -1)], 1).astype(np.int32)
        lists = [list(rng.randint(0, V, 5000)) + [V - 1, 0] for _ in range(n)]
        ptr, flat = csr(lists)
        idx, energy = eng.topk(queries, True, k, ptr, flat)
        assert_rows_equal_reference(eng.read_buffer(native.BUF_RANK_ENERGIES)[:n], idx, energy, k, lists, "limit")
    finally:
        eng.close()
    big = native.Engine(V + 1, R, d, 1, "block", 2, max_edges=1)
    try:
        with pytest.raises(native.RgcnError) as err:
            big.topk(queries, True, k)
        assert err.value.status == 5 and str(V) in str(err.value)
    finally:
        big.close()


def test_predict_command_end_to_end_with_a_real_checkpoint(tmp_path):
    """relationprediction_amd.predict on the reference's Toy data: a model built by the command's own build_model,
    saved with Model.save, asked through predict.main (which builds a second chain, with other initial weights, and
    loads the checkpoint) -- the lines are the first model's device_topk answers, ids and fp32 scores alike."""
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
    pairs = [(int(s), int(r)) for s, r, o in triples[:7]] + [(int(triples[0, 2]), int(triples[0, 1]))]
    (tmp_path / "q.txt").write_text("".join("%s\t%s\n" % (ents[e], rels[r]) for e, r in pairs))
    splits = {"train": triples[:-6].astype(np.int32), "valid": triples[-6:-3], "test": triples[-3:]}
    np.random.seed(7)
    model = predict.build_model(settings_reader.read(str(tmp_path / "s.exp")), splits, V, R)
    model.save(str(tmp_path / "models" / "Toy"))
    for side in ("object", "subject"):
        np.random.seed(8)                                              # the command's chain starts from other weights
        out = tmp_path / ("answers_%s.txt" % side)
        predict.main(["--settings", str(tmp_path / "s.exp"), "--dataset", str(tmp_path), "--model",
                      str(tmp_path / "models" / "Toy-0.npz"), "--queries", str(tmp_path / "q.txt"), "--k", str(k),
                      "--side", side, "--out", str(out)])
        known = {}
        evaluation.Scorer.extend_triple_dict(known, triples, object_list=side == "object")
        ptr, idx = evaluation.known_completions_csr(pairs, known)
        queries = np.full((len(pairs), 3), -1, dtype=np.int32)
        queries[:, 0 if side == "object" else 2] = [p[0] for p in pairs]
        queries[:, 1] = [p[1] for p in pairs]
        want_idx, want_energy = model.device_topk(splits["train"], queries, side == "object", k, ptr, idx)
        want_score = predict.sigmoid_f32(want_energy)
        got = [l.split("\t") for l in out.read_text().splitlines()]
        want = [[ents[e], rels[r], ents[a], str(p + 1), "%.9g" % sc] for (e, r), ids, row in zip(pairs, want_idx, want_score)
                for p, (a, sc) in enumerate(zip(ids, row)) if a >= 0]
        assert got == want and len(got) > len(pairs)
