"""Float64 mirror of the relation-softmax loss term (include/rgcn.h, rgcn_relation_softmax_device): loss, G and the
contributions to dL/dW_relation and dL/dcodes, plain and masked.  numpy only; shared by the host and the GPU tests.

    q_n = c[s_n] * c[o_n]                     (float32 product, as the device forms it; float64 from there on)
    E[n, r'] = q_n . W[r']
    ell_n = log sum_{r' in C_n} exp(E[n, r']) - E[n, r_n]
    term = weight / P * sum_n ell_n
    G[n, r'] = weight / P * (softmax over C_n at r' - [r' = r_n]), 0 outside C_n
"""
import numpy as np


def known_set(known, V):
    """the packed keys (r V + s) V + o of the known positives, as a Python set"""
    k = np.asarray(known, dtype=np.int64).reshape(-1, 3)
    return set(((k[:, 1] * V + k[:, 0]) * V + k[:, 2]).tolist())


def candidate_mask(positives, R, V, known=None):
    """[P, R] bool: C_n.  known None: every relation; else {r_n} and the relations not known for the pair"""
    pos = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    mask = np.ones((len(pos), R), dtype=bool)
    if known is not None:
        keys = known_set(known, V)
        for n, (s, r, o) in enumerate(pos):
            for rr in range(R):
                if rr != r and ((rr * V + s) * V + o) in keys:
                    mask[n, rr] = False
    return mask


def query_rows(codes, positives):
    """float64 copies of the float32 products codes[s] * codes[o] (one rounding per element, as on the device)"""
    pos = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    c = np.asarray(codes, dtype=np.float32)
    return (c[pos[:, 0]] * c[pos[:, 2]]).astype(np.float64)


def term(codes, w_relation, positives, R, weight, known=None, exact_query=False):
    """dict: loss, E [P,R], G [P,R], dW [R,dc], dcodes [V,dc], mask [P,R], ell [P].  exact_query: q in float64 from the
    start (what the finite-difference check differentiates)"""
    pos = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    c64 = np.asarray(codes, dtype=np.float64)
    W = np.asarray(w_relation, dtype=np.float64)[:R]
    V = c64.shape[0]
    P = len(pos)
    q = c64[pos[:, 0]] * c64[pos[:, 2]] if exact_query else query_rows(codes, pos)
    E = q @ W.T
    mask = candidate_mask(pos, R, V, known)
    Em = np.where(mask, E, -np.inf)
    m = Em.max(axis=1, keepdims=True)
    ex = np.exp(Em - m)
    ssum = ex.sum(axis=1, keepdims=True)
    gold = E[np.arange(P), pos[:, 1]]
    ell = np.log(ssum[:, 0]) + m[:, 0] - gold
    onehot = np.zeros((P, R))
    onehot[np.arange(P), pos[:, 1]] = 1.0
    G = weight / P * (ex / ssum - onehot)
    dW = G.T @ q
    dq = G @ W
    dcodes = np.zeros_like(c64)
    np.add.at(dcodes, pos[:, 0], dq * c64[pos[:, 2]])
    np.add.at(dcodes, pos[:, 2], dq * c64[pos[:, 0]])
    return {"loss": weight / P * float(ell.sum()), "E": E, "G": G, "dW": dW, "dcodes": dcodes, "mask": mask, "ell": ell,
            "dq": dq}


def decoder(codes, w_relation, X, Y, reg):
    """float64 mirror of the DistMult decoder's loss (cross-entropy mean + regulariser) and gradients: what the term is
    added to.  Returns (loss, dcodes [V,dc], dW [rows of w_relation, dc])."""
    x = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    y = np.asarray(Y, dtype=np.float64)
    c = np.asarray(codes, dtype=np.float64)
    W = np.asarray(w_relation, dtype=np.float64)
    e1, r, e2 = c[x[:, 0]], W[x[:, 1]], c[x[:, 2]]
    n, d = e1.shape
    en = np.sum(e1 * r * e2, axis=1)
    per = (1 - y) * en + np.log1p(np.exp(-np.abs(en))) + np.maximum(-en, 0)
    loss = per.mean() + reg * (np.mean(e1 ** 2) + np.mean(r ** 2) + np.mean(e2 ** 2))
    dx = ((1.0 / (1.0 + np.exp(-en)) - y) / n)[:, None]
    k = reg * 2.0 / (n * d)
    dcodes = np.zeros_like(c)
    np.add.at(dcodes, x[:, 0], dx * (r * e2) + k * e1)
    np.add.at(dcodes, x[:, 2], dx * (e1 * r) + k * e2)
    dW = np.zeros_like(W)
    np.add.at(dW, x[:, 1], dx * (e1 * e2) + k * r)
    return float(loss), dcodes, dW


def make_case(V, R, dc, P, seed, scale=0.6, hub=None, self_pairs=0):
    """codes [V,dc], W_relation [V,dc] (rows >= R unused), positives [P,3].  hub = (entity, as_subject, as_object): the
    entity is the subject of the first as_subject positives and the object of the last as_object; self_pairs: that many
    leading positives get s = o"""
    rng = np.random.RandomState(seed)
    codes = (rng.randn(V, dc) * scale).astype(np.float32)
    w_rel = (rng.randn(max(V, R), dc) * scale).astype(np.float32)
    pos = np.stack([rng.randint(0, V, P), rng.randint(0, R, P), rng.randint(0, V, P)], 1).astype(np.int32)
    if hub is not None:
        e, ns, no = hub
        pos[:ns, 0] = e
        pos[P - no:, 2] = e
    for i in range(self_pairs):
        pos[i, 2] = pos[i, 0]
    return codes, w_rel, pos
