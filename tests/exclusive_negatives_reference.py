"""numpy mirror of the device negative samplers (csrc/counter_rng.h, csrc/negative_exclusive.h,
csrc/known_positives_index.h, k_negative_sample / k_negative_sample_exclusive of csrc/decoder.hip), in uint64 with wrapping
arithmetic: the counter draws, the plain sampler, the index of known positives and the exclusive decision with its scan
and its counter of unresolved rows.  Vectorised over the rows: attempt 0 for all of them, then every further attempt for
the rows that are still known, then the (rare) scan row by row.

The three tests that compare against it (the sanitizer driver, brute force over Python sets, the device) share the
cases of this module, so that each is computed once per session (`case(name)`)."""
import functools

import numpy as np

U64 = np.uint64
GOLDEN = 0x9E3779B97F4A7C15
MUL1, MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TAG_COIN, TAG_FIRST, TAG_REDRAW = 0x6e65, (0x6e66, 0x6e67), (0x6e68, 0x6e69)
MAX_DRAWS = 32                         # RGCN_NEG_MAX_DRAWS of include/rgcn.h


def drop_bits(seed, tag, idx):
    """drop_bits(seed, tag, idx) of counter_rng.h for an array of indices: 24 bits each"""
    with np.errstate(over="ignore"):
        idx = np.atleast_1d(np.asarray(idx)).astype(U64)
        seed = np.full(1, int(seed) & (2 ** 64 - 1), dtype=U64)
        z = seed + U64(GOLDEN) * (idx + U64(tag << 44) + U64(1))
        z = (z ^ (z >> U64(30))) * U64(MUL1)
        z = (z ^ (z >> U64(27))) * U64(MUL2)
        z = z ^ (z >> U64(31))
    return (z >> U64(40)).astype(np.int64)


def candidates(seed, tags, idx, V):
    """negative_candidate: 48 bits from two draws at idx and idx + 1, scaled to [0, V)"""
    idx = np.atleast_1d(np.asarray(idx)).astype(U64)
    u = (drop_bits(seed, tags[0], idx).astype(U64) << U64(24)) | drop_bits(seed, tags[1], idx + U64(1)).astype(U64)
    return ((u * U64(V)) >> U64(48)).astype(np.int64)      # u < 2^48 and V < 2^16 here and at FB15k-237: no wrap


def pack(s, r, o, V):
    with np.errstate(over="ignore"):
        return (np.asarray(r).astype(U64) * U64(V) + np.asarray(s).astype(U64)) * U64(V) + np.asarray(o).astype(U64)


def build_index(triples, V, R):
    """known_index_build: the sorted unique packed keys; ValueError for an id out of range"""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t[:, [0, 2]].max() >= V or t[:, 1].max() >= R):
        raise ValueError("known positive with an id out of range")
    return np.unique(pack(t[:, 0], t[:, 1], t[:, 2], V))


def index_limits(V, R, num_triples):
    """known_index_limits: 0 (RGCN_OK) or 5 (RGCN_ERR_UNSUPPORTED), in Python integers"""
    return 5 if R * V * V >= 2 ** 63 or num_triples >= 2 ** 31 else 0


def has(keys, key):
    key = np.atleast_1d(key)
    if len(keys) == 0:
        return np.zeros(len(key), dtype=bool)
    pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
    return keys[pos] == key


def plain(batch, rate, V, seed):
    """k_negative_sample: (X int32 [n (rate + 1), 3], Y float32, coin of every negative row)"""
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, 3)
    n = len(batch)
    X = np.tile(batch, (rate + 1, 1))
    Y = np.zeros(n * (rate + 1), dtype=np.float32)
    Y[:n] = 1
    j = np.arange(n * rate, dtype=np.int64)
    coin = (drop_bits(seed, TAG_COIN, 2 * j) & 1).astype(bool)
    ent = candidates(seed, TAG_FIRST, 2 * j, V).astype(np.int32)
    neg = X[n:]
    neg[coin, 2] = ent[coin]
    neg[~coin, 0] = ent[~coin]
    return X, Y, coin


def exclusive(keys, batch, rate, V, R, seed):
    """k_negative_sample_exclusive.  Returns a dict: X, Y, coin [n rate] (True: object side), first_known [n rate]
    (attempt 0 hit K), lookups [n rate] (NegativeChoice::lookups), scanned [n rate] (the row went through the scan),
    unresolved (the counter's increment)."""
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, 3)
    n = len(batch)
    X, Y, coin = plain(batch, rate, V, seed)
    m = n * rate
    neg = X[n:]
    tiled = np.tile(batch.astype(np.int64), (rate, 1))
    s, r, o = tiled[:, 0], tiled[:, 1], tiled[:, 2]
    valid = (s >= 0) & (s < V) & (o >= 0) & (o < V) & (r >= 0) & (r < R)
    sv, rv, ov = np.where(valid, s, 0), np.where(valid, r, 0), np.where(valid, o, 0)
    base = np.where(coin, pack(sv, rv, 0, V), pack(0, rv, ov, V))
    stride = np.where(coin, U64(1), U64(V))
    ent = np.where(coin, neg[:, 2], neg[:, 0]).astype(np.int64)
    first = ent.copy()
    lookups = valid.astype(np.int64)
    known = valid & has(keys, base + ent.astype(U64) * stride)
    first_known = known.copy()
    for t in range(1, MAX_DRAWS):
        rows = np.nonzero(known)[0]
        if len(rows) == 0:
            break
        e = candidates(seed, TAG_REDRAW, 2 * (rows * MAX_DRAWS + t), V)
        ent[rows] = e
        lookups[rows] += 1
        known[rows] = has(keys, base[rows] + e.astype(U64) * stride[rows])
    scanned = known.copy()
    unresolved = 0
    for row in np.nonzero(known)[0]:
        e, found = int(ent[row]), False
        for _ in range(1, V):
            e = 0 if e + 1 == V else e + 1
            lookups[row] += 1
            if not has(keys, base[row] + U64(e) * stride[row])[0]:
                found = True
                break
        if found:
            ent[row] = e
        else:
            ent[row] = first[row]
            unresolved += 1
    ent32 = ent.astype(np.int32)
    neg[coin, 2] = ent32[coin]
    neg[~coin, 0] = ent32[~coin]
    return {"X": X, "Y": Y, "coin": coin, "first_known": first_known, "lookups": lookups, "scanned": scanned,
            "unresolved": unresolved}


# ---- the shared cases ------------------------------------------------------------------------------------------------

def _brute_force_case():
    # the shape of test_device_negative_sampler_layout_and_distribution; K = the batch + 20,000 random triples: about
    # 1.4 % of the 500 candidates of a (pair, side) are known, so several hundred of the 40,000 negatives are redrawn
    V, R, n, rate, seed = 500, 7, 4000, 10, 123
    rng = np.random.RandomState(0)
    batch = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), rng.randint(0, V, n)], 1).astype(np.int32)
    extra = np.stack([rng.randint(0, V, 20000), rng.randint(0, R, 20000), rng.randint(0, V, 20000)], 1).astype(np.int32)
    return dict(V=V, R=R, rate=rate, seed=seed, batch=batch, known=np.concatenate([batch, extra]))


def _saturated_case():
    # (0, 0, .) knows objects 0..10, (1, 0, .) knows all 12
    V, R, rate, seed = 12, 2, 4, 5
    known = np.array([(0, 0, o) for o in range(11)] + [(1, 0, o) for o in range(12)], dtype=np.int32)
    batch = np.array([(0, 0, 0)] * 1000 + [(1, 0, 0)] * 1000, dtype=np.int32)
    return dict(V=V, R=R, rate=rate, seed=seed, batch=batch, known=known)


UNIFORM_SEED = 7       # chosen on the CPU: both chi-square statistics of test_redraws_are_uniform hold for it


def _uniform_case():
    # the pair (3, 1, .) has 32 known objects (the even ids), (., 1, 10) has 16 known subjects (3 and the ids 49..63)
    V, R, rate = 64, 2, 10
    known = np.array([(3, 1, o) for o in range(0, 64, 2)] + [(s, 1, 10) for s in range(49, 64)], dtype=np.int32)
    batch = np.array([(3, 1, 10)] * 2000, dtype=np.int32)
    return dict(V=V, R=R, rate=rate, seed=UNIFORM_SEED, batch=batch, known=known)


CASES = {"brute_force": _brute_force_case, "saturated": _saturated_case, "uniform": _uniform_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case with its index and the mirror's answer; computed once, shared, to be left unchanged"""
    c = CASES[name]()
    c["keys"] = build_index(c["known"], c["V"], c["R"])
    c["mirror"] = exclusive(c["keys"], c["batch"], c["rate"], c["V"], c["R"], c["seed"])
    c["plain"] = plain(c["batch"], c["rate"], c["V"], c["seed"])
    for a in [c["batch"], c["known"], c["keys"], c["plain"][0], c["plain"][1]] + \
            [v for v in c["mirror"].values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return c
