"""numpy mirror of the relation corruptions (csrc/negative_relation.h, k_negative_sample_relation of csrc/decoder.hip),
integer-exact in uint64: attempt 0 for all rows, then every further attempt for the rows that are still known, then the
(rare) scan row by row.  The entity rows in front are the existing mirror's (tests/exclusive_negatives_reference.py), whose
counter draws, packed keys and index this module reuses.

The tests that compare against it (the sanitizer driver, the properties, the device) share the named cases of this module,
each computed once per session (`case(name)`)."""
import functools

import numpy as np

from exclusive_negatives_reference import drop_bits, pack, build_index, has, plain, exclusive

U64 = np.uint64
TAG_FIRST, TAG_REDRAW = (0x6e6a, 0x6e6b), (0x6e6c, 0x6e6d)
MAX_DRAWS = 32                         # RGCN_NEG_MAX_DRAWS of include/rgcn.h


def draws(seed, tags, idx, R):
    """relation_draw: 48 bits from two draws at idx and idx + 1, scaled to [0, R - 1)"""
    idx = np.atleast_1d(np.asarray(idx)).astype(U64)
    u = (drop_bits(seed, tags[0], idx).astype(U64) << U64(24)) | drop_bits(seed, tags[1], idx + U64(1)).astype(U64)
    return ((u * U64(R - 1)) >> U64(48)).astype(np.int64)          # u < 2^48, R < 2^16: no wrap


def relation_rows(keys, batch, relation_rate, V, R, seed, exclusive_mode):
    """the n m relation rows alone.  Returns a dict: X int32 [n m, 3], first [n m] (attempt 0's candidate, or its raw draw
    for a row with an id out of range), valid [n m], first_known [n m] (attempt 0 hit K; all False in the plain form),
    lookups [n m] (RelationChoice::lookups), scanned [n m], unresolved_rows [n m], unresolved (the counter's increment)."""
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, 3)
    n = len(batch)
    m = n * relation_rate
    tiled = np.tile(batch.astype(np.int64), (relation_rate, 1))
    s, r, o = tiled[:, 0], tiled[:, 1], tiled[:, 2]
    valid = (s >= 0) & (s < V) & (o >= 0) & (o < V) & (r >= 0) & (r < R)
    j = np.arange(m, dtype=np.int64)
    d = draws(seed, TAG_FIRST, 2 * j, R)
    first = np.where(valid, d + (d >= r), d)
    rel = first.copy()
    lookups = np.zeros(m, dtype=np.int64)
    known = np.zeros(m, dtype=bool)
    sv, ov = np.where(valid, s, 0), np.where(valid, o, 0)
    if exclusive_mode:
        lookups = valid.astype(np.int64)
        known = valid & has(keys, pack(sv, np.where(valid, rel, 0), ov, V))
    first_known = known.copy()
    for t in range(1, MAX_DRAWS):
        rows = np.nonzero(known)[0]
        if len(rows) == 0:
            break
        d = draws(seed, TAG_REDRAW, 2 * (rows * MAX_DRAWS + t), R)
        e = d + (d >= r[rows])
        rel[rows] = e
        lookups[rows] += 1
        known[rows] = has(keys, pack(sv[rows], e, ov[rows], V))
    scanned = known.copy()
    unresolved_rows = np.zeros(m, dtype=bool)
    for row in np.nonzero(known)[0]:
        e, found = int(rel[row]), False
        for _ in range(1, R):
            e = 0 if e + 1 == R else e + 1
            if e == r[row]:
                continue
            lookups[row] += 1
            if not has(keys, pack(sv[row], e, ov[row], V))[0]:
                found = True
                break
        if found:
            rel[row] = e
        else:
            rel[row] = first[row]
            unresolved_rows[row] = True
    X = tiled.astype(np.int32)
    X[:, 1] = rel.astype(np.int32)
    return {"X": X, "first": first, "valid": valid, "first_known": first_known, "lookups": lookups, "scanned": scanned,
            "unresolved_rows": unresolved_rows, "unresolved": int(unresolved_rows.sum())}


def sample(keys, batch, rate, relation_rate, V, R, seed, exclusive_mode):
    """rgcn_negative_sample_relation_device: the entity rows of the existing mirror, the relation rows behind them.
    Returns a dict: X [n (1 + rate + m), 3], Y, entity_unresolved (what RGCN_BUF_NEGATIVE_UNRESOLVED grows by),
    relation (the dict of relation_rows)."""
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, 3)
    if exclusive_mode:
        e = exclusive(keys, batch, rate, V, R, seed)
        Xe, Ye, entity_unresolved = e["X"], e["Y"], e["unresolved"]
    else:
        Xe, Ye, _ = plain(batch, rate, V, seed)
        entity_unresolved = 0
    rel = relation_rows(keys, batch, relation_rate, V, R, seed, exclusive_mode)
    return {"X": np.concatenate([Xe, rel["X"]]), "Y": np.concatenate([Ye, np.zeros(len(rel["X"]), dtype=np.float32)]),
            "entity_unresolved": entity_unresolved, "relation": rel}


# ---- the shared cases ------------------------------------------------------------------------------------------------

def small_fixture():
    """the `small` fixture of tests/test_gpu_exclusive_negatives.py, by its recipe and seed: V 150, R 9, 800 distinct batch
    triples, K = the batch + 20,000 random triples"""
    V, R, n = 150, 9, 800
    rng = np.random.RandomState(17)
    flat = rng.permutation(V * R * V)[:n]
    batch = np.stack([flat // (R * V), (flat // V) % R, flat % V], 1).astype(np.int32)
    extra = np.stack([rng.randint(0, V, 20000), rng.randint(0, R, 20000), rng.randint(0, V, 20000)], 1).astype(np.int32)
    return V, R, batch, np.concatenate([batch, extra])


def _small_case():
    V, R, batch, known = small_fixture()
    return dict(V=V, R=R, rate=2, relation_rate=2, seed=1234, batch=batch, known=known)


def _two_relations_case():
    V, R = 7, 2
    rng = np.random.RandomState(4)
    batch = np.stack([rng.randint(0, V, 60), rng.randint(0, R, 60), rng.randint(0, V, 60)], 1).astype(np.int32)
    return dict(V=V, R=R, rate=1, relation_rate=3, seed=9, batch=batch, known=np.array([(6, 1, 6)], dtype=np.int32))


def _scan_case(free=(37,)):
    # (0, ., 1) knows 62 of the 63 relations other than the batch's own: all but `free`.  A row reaches the scan when all
    # 32 candidates are known, with probability (62/63)^32 = 0.60
    V, R = 5, 64
    known = np.array([(0, r, 1) for r in range(1, R) if r not in free], dtype=np.int32)
    batch = np.array([(0, 0, 1)] * 64, dtype=np.int32)
    return dict(V=V, R=R, rate=1, relation_rate=2, seed=21, batch=batch, known=known)


def _saturated_case():
    return _scan_case(free=())


def _invalid_rows_case():
    V, R, batch, known = small_fixture()
    batch = batch[:40].copy()
    batch[3, 0] = V                    # one s, one r and one o out of range
    batch[11, 1] = R
    batch[17, 2] = -1
    return dict(V=V, R=R, rate=2, relation_rate=2, seed=77, batch=batch, known=known)


CASES = {"small": _small_case, "two_relations": _two_relations_case, "scan": _scan_case, "saturated": _saturated_case,
         "invalid_rows": _invalid_rows_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """the named case with its index and the mirror's answers (`mirror`: exclusive, `plain`: plain form); computed once,
    shared, to be left unchanged"""
    c = CASES[name]()
    c["keys"] = build_index(c["known"], c["V"], c["R"])
    args = (c["keys"], c["batch"], c["rate"], c["relation_rate"], c["V"], c["R"], c["seed"])
    c["mirror"] = sample(*args, exclusive_mode=True)
    c["plain"] = sample(*args, exclusive_mode=False)
    for a in (c["batch"], c["known"], c["keys"]):
        a.setflags(write=False)
    for out in (c["mirror"], c["plain"]):
        for v in list(out.values()) + list(out["relation"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c
