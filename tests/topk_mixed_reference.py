"""Numpy side of the ensemble top-k tests (include/rgcn.h rgcn_topk_mixed_device): the selection restated on a row of
mixed scores, and a case whose expected answer does not depend on how anyone rounds an exponential.  No GPU, no library.

The grid.  Own and partner energies are drawn from GRID, multiples of 0.5 in [-3, 3], and the weight is 0.5.  At that
weight 0.5 * s_a + 0.5 * s_b is commutative in IEEE arithmetic, so two entities with the same unordered (own, partner)
pair tie bit for bit, on the device and in numpy; two entities with different pairs must be far apart.  All thirteen
multiples cannot be used: sigmoid(x) + sigmoid(-x) = 1 for every x, so {x, -x}, {y, -y} and {0, 0} are different pairs
with the same mixed score.  A grid may therefore hold 0 and one sign of each magnitude, seven values at the most; the
signs below are the choice with the widest smallest gap between two different pairs, 6.9e-3 (grid_margin(), asserted
against MARGIN by grid_case and by tests/test_topk_mixed_host.py)."""
import numpy as np

import embedding_reference as er
from topk_reference import float_key

GRID = (-3.0, -2.5, 0.0, 0.5, 1.0, 1.5, 2.0)       # 1.0 is in it: the query entity's own value
MARGIN = 1e-5           # about a hundred times the fp32 rounding of a mixed score (2^-23 = 1.2e-7)
GRID_WEIGHT = 0.5
GRID_SHAPES = {"V1100": (1100, 24)}                  # name -> (V, queries): past one 1,024-entity trip of the select loops
GRID_KS = (1, 10)                                    # the k at which ties must straddle the cut (k = V cannot)


def mixed_topk(row, k, excluded=()):
    """(ids int32 [k], scores float32 [k]): the k best non-excluded entries of a float32 row of mixed scores ordered by
    (value descending, id ascending), padded with (-1, -inf).  Values are compared as the device compares them, through
    float_key; mixed scores lie in [0, 1] and are never -0.0, so that is their numeric order."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    keep = np.ones(len(row), dtype=bool)
    ex = np.asarray(list(excluded), dtype=np.int64)
    if len(ex):
        keep[ex] = False
    ids = np.flatnonzero(keep)
    keys = float_key(row.view(np.uint32)).astype(np.int64)
    order = ids[np.lexsort((ids, -keys[ids]))][:k]
    idx = np.full(k, -1, dtype=np.int32)
    score = np.full(k, -np.inf, dtype=np.float32)
    idx[:len(order)] = order
    score[:len(order)] = row[order]
    return idx, score


def grid_margin(grid=GRID, weight=GRID_WEIGHT):
    """the smallest float64 distance between the mixed scores of two DIFFERENT unordered (own, partner) pairs of `grid`"""
    values = sorted(float(er.mixed_scores(a, b, weight)) for i, a in enumerate(grid) for b in grid[i:])
    return float(np.min(np.diff(values)))


def grid_case(V, n):
    """An embedding model, queries and partner energies whose mixed top-k is known exactly.

    W_emb[e] = (g_e, 0, ..., 0) with g_e from GRID, every relation row (1, 0, ..., 0), every query entity one with g = 1:
    the own energy of entity e is g_e exactly, on either side and through the split-bf16 GEMM (every factor is a bf16
    number, every product and sum exact).  The partner's energies are drawn from GRID per query and entity.  Returns the
    parameters, the queries, `own` and `partner` (float32 [n, V]), `m` = the float64 mixed scores at GRID_WEIGHT (equal
    pairs give equal float64 values there as well) and per-query exclusion lists: none on every third row, else a few
    random ids with duplicates."""
    assert grid_margin() > MARGIN
    d, R = 16, 3
    rng = np.random.RandomState(7000 + V)
    g = rng.choice(GRID, size=V).astype(np.float32)
    ones = np.arange(0, V, max(1, V // 8))[:8]
    g[ones] = 1.0
    emb = np.zeros((V, d), np.float32)
    emb[:, 0] = g
    rel = np.zeros((V, d), np.float32)                # W_relation has V rows, of which the first R are relations
    rel[:, 0] = 1.0
    params = {"W_emb": emb, "b_emb": np.zeros(d, np.float32), "W_relation": rel}
    fixed = rng.choice(ones, size=n)
    queries = np.stack([fixed, rng.randint(0, R, n), fixed], 1).astype(np.int32)
    own = np.tile(g, (n, 1))
    partner = rng.choice(GRID, size=(n, V)).astype(np.float32)
    lists = []
    for i in range(n):
        if i % 3 == 0:
            lists.append([])
            continue
        extra = [int(e) for e in rng.randint(0, V, rng.randint(1, V // 4))]
        lists.append(extra + extra[:3])
    return {"V": V, "R": R, "d": d, "n": n, "params": params, "queries": queries, "own": own, "partner": partner,
            "m": er.mixed_scores(own, partner, GRID_WEIGHT), "lists": lists}


def expected_ids(m_row, k, excluded=()):
    """ids int32 [k] of the k best non-excluded entries of a float64 row in which equal pairs hold equal values: (value
    descending, id ascending), padded with -1"""
    keep = np.ones(len(m_row), dtype=bool)
    ex = np.asarray(list(excluded), dtype=np.int64)
    if len(ex):
        keep[ex] = False
    ids = np.flatnonzero(keep)
    order = ids[np.lexsort((ids, -m_row[ids]))][:k]
    out = np.full(k, -1, dtype=np.int32)
    out[:len(order)] = order
    return out


def tie_straddles(m_row, k, excluded=()):
    """does a group of exactly equal values hold both position k and position k + 1 of the row's order?"""
    keep = np.ones(len(m_row), dtype=bool)
    ex = np.asarray(list(excluded), dtype=np.int64)
    if len(ex):
        keep[ex] = False
    v = np.sort(m_row[keep])[::-1]
    return len(v) > k and v[k - 1] == v[k]


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.asarray([e for x in lists for e in x], dtype=np.int32)
    return ptr, idx


def exclusion_variants(V, lists):
    """the exclusion lists the GPU cases run with: none at all, the case's own (some empty, some with duplicates), and
    lists that leave row i only i % 7 entities -- fewer than k for every k >= 7, none at all on every seventh row"""
    heavy = [[e for e in range(V) if (e * 7 + i) % V >= i % 7] for i in range(len(lists))]
    return {"none": None, "lists": lists, "few_left": heavy}
