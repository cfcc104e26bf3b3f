"""Float64 mirror of the entity-softmax loss term (include/rgcn.h, rgcn_entity_softmax_device): loss, G, dq and the
contributions to dL/dcodes and dL/dW_relation, plain and masked.  numpy only; shared by the host and the GPU tests.

Every positive (s_n, r_n, o_n), n < P, gives the object row m = n (query a = s_n, gold g = o_n) and the subject row
m = P + n (a = o_n, g = s_n):

    q_m = c[a_m] * W[r_m]                     (float32 product, as the device forms it; float64 from there on)
    E[m, e] = q_m . c[e]
    ell_m = log sum_{e in C_m} exp(E[m, e]) - E[m, g_m]
    term = weight / (2P) * sum_m ell_m
    G[m, e] = weight / (2P) * (softmax over C_m at e - [e = g_m]), 0 outside C_m
    dcodes[e] += sum_m G[m, e] q_m;  dq_m = sum_e G[m, e] c[e];  dcodes[a_m] += dq_m * W[r_m];  dW[r_m] += dq_m * c[a_m]
"""
import numpy as np


def rows_of(positives):
    """(a, r, g, side) of the 2P rows: object rows first, then subject rows"""
    pos = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    P = len(pos)
    a = np.concatenate([pos[:, 0], pos[:, 2]])
    g = np.concatenate([pos[:, 2], pos[:, 0]])
    r = np.concatenate([pos[:, 1], pos[:, 1]])
    side = np.concatenate([np.zeros(P, dtype=np.int64), np.ones(P, dtype=np.int64)])
    return a, r, g, side


def candidate_mask(positives, V, known=None):
    """[2P, V] bool: C_m.  known None: every entity; else {g_m} and the entities e for which the row's completed triple
    -- (s, r, e) for an object row, (e, r, o) for a subject row -- is not known"""
    a, r, g, side = rows_of(positives)
    mask = np.ones((len(a), V), dtype=bool)
    if known is not None:
        k = np.asarray(known, dtype=np.int64).reshape(-1, 3)
        objects, subjects = {}, {}
        for s, rr, o in k.tolist():
            objects.setdefault((s, rr), set()).add(o)
            subjects.setdefault((rr, o), set()).add(s)
        for m in range(len(a)):
            out = objects.get((a[m], r[m]), ()) if side[m] == 0 else subjects.get((r[m], a[m]), ())
            for e in out:
                if e != g[m]:
                    mask[m, e] = False
    return mask


def query_rows(codes, w_relation, positives):
    """float64 copies of the float32 products codes[a] * W_relation[r] (one rounding per element, as on the device)"""
    a, r, _, _ = rows_of(positives)
    return (np.asarray(codes, dtype=np.float32)[a] * np.asarray(w_relation, dtype=np.float32)[r]).astype(np.float64)


def term(codes, w_relation, positives, weight, known=None, exact_query=False):
    """dict: loss, E [2P,V], G [2P,V], dq [2P,dc], dcodes [V,dc], dW [rows of w_relation, dc], mask [2P,V], ell [2P].
    exact_query: q in float64 from the start (what the finite-difference check differentiates)"""
    a, r, g, _ = rows_of(positives)
    c = np.asarray(codes, dtype=np.float64)
    W = np.asarray(w_relation, dtype=np.float64)
    V = c.shape[0]
    M = len(a)
    q = c[a] * W[r] if exact_query else query_rows(codes, w_relation, positives)
    E = q @ c.T
    mask = candidate_mask(positives, V, known)
    Em = np.where(mask, E, -np.inf)
    m = Em.max(axis=1, keepdims=True)
    ex = np.exp(Em - m)
    ssum = ex.sum(axis=1, keepdims=True)
    rows = np.arange(M)
    ell = np.log(ssum[:, 0]) + m[:, 0] - E[rows, g]
    onehot = np.zeros((M, V))
    onehot[rows, g] = 1.0
    G = weight / M * (ex / ssum - onehot)
    dq = G @ c
    dcodes = G.T @ q
    np.add.at(dcodes, a, dq * W[r])
    dW = np.zeros_like(W)
    np.add.at(dW, r, dq * c[a])
    return {"loss": weight / M * float(ell.sum()), "E": E, "G": G, "dq": dq, "dcodes": dcodes, "dW": dW, "mask": mask,
            "ell": ell}


def make_case(V, R, dc, P, seed, scale=0.6, hub_entity=None, hub_relation=None):
    """codes [V,dc], W_relation [max(V,R),dc] (rows >= R unused), positives [P,3].  Every case holds a positive with
    s = o (where P >= 1), one whose object is entity 0 and one whose subject is entity V - 1 (where P >= 3), so that
    the golds of its rows include 0 and V - 1.  hub_entity = (entity, count): the entity is the subject of the LAST
    `count` positives; hub_relation = (relation, count): the relation of the last `count` positives."""
    rng = np.random.RandomState(seed)
    codes = (rng.randn(V, dc) * scale).astype(np.float32)
    w_rel = (rng.randn(max(V, R), dc) * scale).astype(np.float32)
    pos = np.stack([rng.randint(0, V, P), rng.randint(0, R, P), rng.randint(0, V, P)], 1).astype(np.int32)
    if hub_entity is not None:
        pos[P - hub_entity[1]:, 0] = hub_entity[0]
    if hub_relation is not None:
        pos[P - hub_relation[1]:, 1] = hub_relation[0]
    pos[0, 2] = pos[0, 0]                  # both rows and both roles on one entity
    if P == 1:
        pos[0, 0], pos[0, 2] = 0, V - 1    # (one positive cannot be all three: it takes the two boundary golds)
    if P == 2:
        pos[1, 2], pos[1, 0] = 0, V - 1
    if P >= 3:
        pos[1, 2] = 0                      # an object row whose gold is entity 0
        pos[2, 0] = V - 1                  # a subject row whose gold is entity V - 1
    return codes, w_rel, pos
