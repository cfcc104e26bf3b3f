"""numpy mirror of reciprocal relations (csrc/negative_reciprocal.h, k_reciprocal_rows of csrc/decoder.hip), integer-exact:
the pass behind the samplers' rows.  The rows in front are the existing mirrors' (tests/exclusive_negatives_reference.py,
tests/relation_negatives_reference.py, tests/typed_negatives_reference.py), whose counter draws this module reuses.

    rows [0, n)                 the positives: kept
    rows [n, n (K + 1))         the entity corruptions: relation r -> r + R where the coin drop_bits(seed, 0x6e65, 2 j) & 1
                                of negative row j = row - n is 0 (the subject was replaced); r outside [0, R) is kept
    rows [n (K + 1), n (K + 1 + m))   the relation rows: kept
    rows behind them, n         new: (s, r + R, o) of the batch, label 1
"""
import numpy as np

from exclusive_negatives_reference import drop_bits

KEEP, SHIFT, TAIL = 0, 1, 2
TAG_COIN = 0x6e65


def coins(seed, count):
    """the samplers' coin of negative rows 0 .. count - 1: 1 = the object was replaced"""
    j = np.arange(count, dtype=np.uint64)
    return (drop_bits(seed, TAG_COIN, np.uint64(2) * j) & 1).astype(np.int64) if count else np.zeros(0, dtype=np.int64)


def choice(i, n, K, m, R, seed):
    """reciprocal_choice for one row: (action, source)"""
    entity_end, tail = n * (K + 1), n * (K + 1 + m)
    if i < n or i >= tail + n:
        return KEEP, -1
    if i < entity_end:
        coin = int(drop_bits(seed, TAG_COIN, np.array([2 * (i - n)], dtype=np.uint64))[0]) & 1
        return (KEEP if coin else SHIFT), -1
    if i < tail:
        return KEEP, -1
    return TAIL, i - tail


def shift_relation(r, R):
    """reciprocal_relation on an array: r + R inside [0, R), r itself outside"""
    r = np.asarray(r, dtype=np.int64)
    return np.where((r >= 0) & (r < R), r + R, r)


KINDS = ("plain", "exclusive", "typed")


def sampler_rows(kind, batch, known, rate, relation_rate, V, R, seed):
    """(X, Y) of one of the three entity samplers with relation_rate relation rows behind its rows, from the existing
    mirrors: what the device calls write in front of the reciprocal pass.  kind: "plain", "exclusive" (against `known`)
    or "typed" (the sets of `known`, not exclusive)."""
    import relation_negatives_reference as rel
    import typed_negatives_reference as typ
    from exclusive_negatives_reference import build_index
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, 3)
    if kind == "typed":
        e = typ.typed(typ.build_sets(known, V, R), known, batch, rate, seed, False)
        rows = rel.relation_rows(np.zeros(0, dtype=np.uint64), batch, relation_rate, V, R, seed, False)
        return (np.concatenate([e["X"], rows["X"]]).astype(np.int32),
                np.concatenate([e["Y"], np.zeros(len(rows["X"]), dtype=np.float32)]))
    exclusive = kind == "exclusive"
    keys = build_index(known, V, R) if exclusive else np.zeros(0, dtype=np.uint64)
    out = rel.sample(keys, batch, rate, relation_rate, V, R, seed, exclusive_mode=exclusive)
    return out["X"].astype(np.int32), out["Y"].astype(np.float32)


def sample(kind, batch, known, rate, relation_rate, V, R, seed):
    """the sampler call and the reciprocal pass behind it: a dict with X0, Y0 (the sampler's), X, Y (the batch under the
    mode) and coin [n rate] (1: the object was replaced)"""
    X0, Y0 = sampler_rows(kind, batch, known, rate, relation_rate, V, R, seed)
    X, Y = transform(batch, X0, Y0, rate, relation_rate, R, seed)
    return {"X0": X0, "Y0": Y0, "X": X, "Y": Y, "coin": coins(seed, len(batch) * rate)}


def transform(batch, X, Y, rate, relation_rate, R, seed):
    """the pass over a sampler's output X [n (rate + 1 + m), 3], Y: (X' int32 [n (rate + 2 + m), 3], Y' float32).  The
    inputs are left unchanged."""
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, 3)
    n = len(batch)
    X = np.asarray(X, dtype=np.int32).reshape(-1, 3)
    assert len(X) == n * (rate + 1 + relation_rate) and len(Y) == len(X)
    out = np.concatenate([X, batch]).astype(np.int32)
    subject = coins(seed, n * rate) == 0
    neg = out[n:n * (rate + 1), 1]
    out[n:n * (rate + 1), 1] = np.where(subject, shift_relation(neg, R), neg).astype(np.int32)
    out[len(X):, 1] = shift_relation(batch[:, 1], R).astype(np.int32)
    return out, np.concatenate([np.asarray(Y, dtype=np.float32), np.ones(n, dtype=np.float32)])
