"""Plain-Python / numpy mirror of the type-constrained sampler and queries (csrc/type_sets.h, csrc/negative_typed.h,
k_negative_sample_typed of csrc/decoder.hip, k_rank_rows_typed and the typed k_topk_rows of csrc/ranking.hip): the list
build, the per-row decision with its open rows and both counters, the typed ranks and the typed top-k.  Row by row in
Python integers (the counter draws are 64-bit arithmetic masked by hand); the ranks follow
tests/relation_query_reference.py's tie rule (fp32 sigmoid evaluated in double, saturated scores tie).

The tests that compare against it (the sanitizer driver, Python sets, the device) share the cases of this module, so
that each is computed once per session (`case(name)`)."""
import bisect
import functools

import numpy as np

from relation_query_reference import sigmoid_f32

M64 = 2 ** 64 - 1
GOLDEN = 0x9E3779B97F4A7C15
MUL1, MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TAG_COIN, TAG_FIRST, TAG_REDRAW = 0x6e65, (0x6e66, 0x6e67), (0x6e68, 0x6e69)
MAX_DRAWS = 32                         # RGCN_NEG_MAX_DRAWS of include/rgcn.h
MIN_CANDIDATES = 2                     # RGCN_TYPED_MIN_CANDIDATES of include/rgcn.h


def bits(seed, tag, idx):
    """drop_bits(seed, tag, idx) of counter_rng.h: 24 bits"""
    z = (seed + GOLDEN * (idx + (tag << 44) + 1)) & M64
    z = ((z ^ (z >> 30)) * MUL1) & M64
    z = ((z ^ (z >> 27)) * MUL2) & M64
    return (z ^ (z >> 31)) >> 40


def draw48(seed, tags, idx):
    return (bits(seed, tags[0], idx) << 24) | bits(seed, tags[1], idx + 1)


# ---- the sets ----------------------------------------------------------------------------------------------------------

def sets_limits(V, R, num_triples):
    """type_sets_limits: 0 (RGCN_OK) or 5 (RGCN_ERR_UNSUPPORTED), in Python integers"""
    return 5 if 2 * R * ((V + 31) // 32) >= 2 ** 31 or num_triples >= 2 ** 31 else 0


def build_sets(triples, V, R):
    """type_sets_build: {"ptr": int64 [2R+1], "idx": int32, "mask": uint32 [2R, W], "lists": [sorted members]};
    ValueError for an id out of range"""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t[:, [0, 2]].max() >= V or t[:, 1].max() >= R):
        raise ValueError("type sets: a triple with an id out of range")
    members = [set() for _ in range(2 * R)]
    for s, r, o in t.tolist():
        members[r].add(s)
        members[R + r].add(o)
    lists = [sorted(m) for m in members]
    ptr = np.zeros(2 * R + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.array([e for l in lists for e in l], dtype=np.int32)
    W = (V + 31) // 32
    mask = np.zeros((2 * R, W), dtype=np.uint32)
    for l, lst in enumerate(lists):
        for e in (range(V) if len(lst) < MIN_CANDIDATES else lst):
            mask[l, e >> 5] |= np.uint32(1 << (e & 31))
    return {"ptr": ptr, "idx": idx, "mask": mask, "lists": lists, "V": V, "R": R}


def candidate_set(sets, side, r):
    """the entities list (side, r) stands for: its members, or all V where it is open"""
    lst = sets["lists"][side * sets["R"] + r]
    return set(range(sets["V"])) if len(lst) < MIN_CANDIDATES else set(lst)


# ---- the decision ------------------------------------------------------------------------------------------------------

def _known(K, coin, s, r, o, e):
    return ((s, r, e) if coin else (e, r, o)) in K


def exclusive_row(K, V, R, seed, j, s, r, o):
    """negative_exclusive_choice: (entity, coin, lookups, unresolved); K a Python set of (s, r, o)"""
    coin = bits(seed, TAG_COIN, 2 * j) & 1
    first = (draw48(seed, TAG_FIRST, 2 * j) * V) >> 48
    if not (0 <= s < V and 0 <= o < V and 0 <= r < R):
        return first, coin, 0, 0
    e, lookups = first, 1
    if not _known(K, coin, s, r, o, e):
        return e, coin, lookups, 0
    for t in range(1, MAX_DRAWS):
        e = (draw48(seed, TAG_REDRAW, 2 * (j * MAX_DRAWS + t)) * V) >> 48
        lookups += 1
        if not _known(K, coin, s, r, o, e):
            return e, coin, lookups, 0
    for _ in range(1, V):
        e = 0 if e + 1 == V else e + 1
        lookups += 1
        if not _known(K, coin, s, r, o, e):
            return e, coin, lookups, 0
    return first, coin, lookups, 1


def typed_row(sets, K, exclusive, seed, j, s, r, o):
    """negative_typed_choice: (entity, coin, open, lookups, unresolved)"""
    V, R = sets["V"], sets["R"]

    def open_row(lookups):
        if exclusive:
            e, coin, more, unresolved = exclusive_row(K, V, R, seed, j, s, r, o)
            return e, coin, 1, lookups + more, unresolved
        return (draw48(seed, TAG_FIRST, 2 * j) * V) >> 48, bits(seed, TAG_COIN, 2 * j) & 1, 1, lookups, 0

    if not (0 <= s < V and 0 <= o < V and 0 <= r < R):
        return open_row(0)
    coin = bits(seed, TAG_COIN, 2 * j) & 1
    L = sets["lists"][coin * R + r]
    m = len(L)
    if m < MIN_CANDIDATES:
        return open_row(0)
    own = o if coin else s
    at = bisect.bisect_left(L, own)
    p = at if at < m and L[at] == own else -1
    n = m - (1 if p >= 0 else 0)
    if n < 1:
        return open_row(0)

    def position(u):
        c = (u * n) >> 48
        return c + 1 if p >= 0 and c >= p else c

    c = position(draw48(seed, TAG_FIRST, 2 * j))
    if not exclusive:
        return L[c], coin, 0, 0, 0
    lookups = 1
    if not _known(K, coin, s, r, o, L[c]):
        return L[c], coin, 0, lookups, 0
    for t in range(1, MAX_DRAWS):
        c = position(draw48(seed, TAG_REDRAW, 2 * (j * MAX_DRAWS + t)))
        lookups += 1
        if not _known(K, coin, s, r, o, L[c]):
            return L[c], coin, 0, lookups, 0
    for _ in range(1, m):
        c = 0 if c + 1 == m else c + 1
        if c == p:
            continue
        lookups += 1
        if not _known(K, coin, s, r, o, L[c]):
            return L[c], coin, 0, lookups, 0
    return open_row(lookups)


def typed(sets, known, batch, rate, seed, exclusive):
    """k_negative_sample_typed.  Returns a dict: X int32 [n (rate + 1), 3], Y float32, coin / open / lookups / unresolved
    per negative row [n rate], open_count and unresolved_count (the two counters' increments)."""
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, 3)
    K = {tuple(t) for t in np.asarray(known).reshape(-1, 3).tolist()} if exclusive else set()
    n = len(batch)
    X = np.tile(batch, (rate + 1, 1))
    Y = np.zeros(n * (rate + 1), dtype=np.float32)
    Y[:n] = 1
    rows = batch.tolist()
    out = np.zeros((n * rate, 4), dtype=np.int64)
    for j in range(n * rate):
        s, r, o = rows[j % n]
        e, coin, is_open, lookups, unresolved = typed_row(sets, K, exclusive, int(seed) & M64, j, s, r, o)
        X[n + j, 2 if coin else 0] = e
        out[j] = (coin, is_open, lookups, unresolved)
    return {"X": X, "Y": Y, "coin": out[:, 0].astype(bool), "open": out[:, 1].astype(bool), "lookups": out[:, 2],
            "unresolved": out[:, 3], "open_count": int(out[:, 1].sum()), "unresolved_count": int(out[:, 3].sum())}


# ---- ranks and top-k ---------------------------------------------------------------------------------------------------

def typed_ranks_from_energies(sets, energies, queries, predict_object, filter_lists):
    """(raw int32 [n], filtered int32 [n]) from float32 energies [n,V]: the candidates of row i are C = list
    (predict_object, r_i) + {gold_i}; raw = #{e in C : score[e] >= score[gold]}, filtered = raw - #{e in the row's filter
    list and in C : score[e] >= score[gold]} + 1, on fp32 sigmoid scores.  A list counts once per entry."""
    scores = sigmoid_f32(np.asarray(energies, dtype=np.float32))
    queries = np.asarray(queries)
    side = 1 if predict_object else 0
    raw = np.zeros(len(scores), dtype=np.int32)
    filtered = np.zeros(len(scores), dtype=np.int32)
    for i, q in enumerate(queries.tolist()):
        gold = q[2] if side else q[0]
        C = candidate_set(sets, side, q[1]) | {gold}
        inC = np.zeros(scores.shape[1], dtype=bool)
        inC[sorted(C)] = True
        reaches = inC & (scores[i] >= scores[i, gold])
        raw[i] = int(reaches.sum())
        listed = np.asarray(filter_lists[i], dtype=np.int64)
        filtered[i] = raw[i] - int(reaches[listed].sum()) + 1
    return raw, filtered


def typed_topk_from_energies(sets, energies, queries, predict_object, k, exclude_lists=None):
    """(idx int32 [n,k], energy float32 [n,k]): the min(k, |list \\ excluded|) best members of list (predict_object, r_i)
    by (energy descending, id ascending) on the float order of the bits (-0.0 below +0.0), padded with (-1, -inf)"""
    energies = np.asarray(energies, dtype=np.float32)
    side = 1 if predict_object else 0
    idx = np.full((len(energies), k), -1, dtype=np.int32)
    val = np.full((len(energies), k), -np.inf, dtype=np.float32)
    for i, q in enumerate(np.asarray(queries).tolist()):
        allowed = candidate_set(sets, side, q[1]) - set(int(e) for e in (exclude_lists[i] if exclude_lists else ()))
        ids = np.array(sorted(allowed), dtype=np.int64)
        if len(ids) == 0:
            continue
        b = energies[i, ids].view(np.uint32).astype(np.int64)
        key = np.where(b & 0x80000000, (~b) & 0xffffffff, b | 0x80000000)      # float_key of ranking.hip
        order = np.lexsort((ids, -key))[:k]
        idx[i, :len(order)] = ids[order]
        val[i, :len(order)] = energies[i, ids[order]]
    return idx, val


# ---- the shared cases --------------------------------------------------------------------------------------------------

def typed_graph(V, R, seed):
    """T with lists of many shapes: relation 0 unseen (both lists open), relation 1 a single (s, o) pair (singletons:
    open), relation 2 two subjects and three objects, relation 3 thirty-three subjects and most objects, relation 4
    (R - 1) random, ids V - 1 present, duplicates"""
    rng = np.random.RandomState(seed)
    t = [(5, 1, 6), (5, 1, 6)]
    t += [(1, 2, 3), (2, 2, 4), (1, 2, 8 % V), (2, 2, 3)]
    subj33 = rng.permutation(V)[:min(33, V - 1)]
    t += [(int(s), 3, int(o)) for s in subj33 for o in rng.randint(0, V, 3)]
    t += [(V - 1, R - 1, V - 1), (0, R - 1, V - 1), (V - 1, R - 1, 0)]
    t += [(int(s), R - 1, int(o)) for s, o in zip(rng.randint(0, V, 40), rng.randint(0, V, 40))]
    return np.array(t, dtype=np.int32)


def _device_case(V, n, rate, seed):
    R = 5
    T = typed_graph(V, R, seed)
    rng = np.random.RandomState(seed + 1)
    # the batch: training triples (own inside its list), random rows (own mostly outside), two rows with bad ids
    pick = T[rng.randint(0, len(T), n - n // 3 - 2)]
    rand = np.stack([rng.randint(0, V, n // 3), rng.randint(0, R, n // 3), rng.randint(0, V, n // 3)], 1).astype(np.int32)
    bad = np.array([(V, 2, 3), (1, -1, 3)], dtype=np.int32)
    batch = np.concatenate([pick, rand, bad])[rng.permutation(n)]
    return dict(V=V, R=R, rate=rate, seed=1000 + seed, T=T, batch=np.ascontiguousarray(batch), known=T)


CASES = {
    # n (rate + 1) = 255, 256, 257 at V = 67 (the last mask word is partial); V = 31 and V = 257
    "v67_255": lambda: _device_case(67, 85, 2, 1),
    "v67_256": lambda: _device_case(67, 64, 3, 2),
    "v67_257": lambda: _device_case(67, 257, 0, 3),
    "v31": lambda: _device_case(31, 50, 4, 4),
    "v257": lambda: _device_case(257, 120, 3, 5),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case with its sets and the mirror's two answers; computed once, shared, to be left unchanged"""
    c = CASES[name]()
    c["sets"] = build_sets(c["T"], c["V"], c["R"])
    c["plain"] = typed(c["sets"], c["known"], c["batch"], c["rate"], c["seed"], False)
    c["exclusive"] = typed(c["sets"], c["known"], c["batch"], c["rate"], c["seed"], True)
    for a in [c["batch"], c["T"], c["sets"]["ptr"], c["sets"]["idx"], c["sets"]["mask"]] + \
            [v for m in (c["plain"], c["exclusive"]) for v in m.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return c
