"""float64 numpy restatement of the encoder under IncidenceNormalization=local (RGCN_NORM_LOCAL; reference:
code/extras/graph_representations.py:94-107,134-147, the 'local' branch of forward/backward_incidence_matrix: softmax
of ones over the entries that share (relation, row), summed over the relation axis).  TEST INFRASTRUCTURE: the oracle
cannot express this mode (its incidence_values knows vertex rows only), so the norms come from a host recount here and
the layers are written out with the norms passed in, for the block kind, the basis kind and the featureless basis
encoder alike.

    n_f[e] = 1 / |{e' : r' = r, o' = o}|      forward message  s -> o, directed relation r
    n_b[e] = 1 / |{e' : r' = r, s' = s}|      backward message o -> s, directed relation R + r

Counts run over the triples given (duplicates count once each, a self-edge counts in both directions)."""
import numpy as np

import oracle

F64 = np.float64


# ----------------------------------------------------------------------------- the norms of all four modes
def counts(triples):
    """(per-edge count of edges sharing (r, o), per-edge count of edges sharing (r, s)), int64"""
    t = np.asarray(triples).reshape(-1, 3).astype(np.int64)
    out = []
    for col in (2, 0):
        if len(t) == 0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        _, inv, cnt = np.unique(t[:, [1, col]], axis=0, return_inverse=True, return_counts=True)
        out.append(cnt[np.asarray(inv).reshape(-1)])
    return out[0], out[1]


def message_norms_f32(triples, V, norm):
    """(n_f, n_b) per edge exactly as the device computes them: float32(1) / float32(integer count)"""
    t = np.asarray(triples).reshape(-1, 3)
    if norm == "local":
        c_f, c_b = counts(t)
        return np.float32(1) / c_f.astype(np.float32), np.float32(1) / c_b.astype(np.float32)
    mode = {"intended": oracle.NORM_INTENDED, "tf_as_executed": oracle.NORM_TF_AS_EXECUTED, "none": oracle.NORM_NONE}[norm]
    return oracle.incidence_values(t[:, 2], V, mode), oracle.incidence_values(t[:, 0], V, mode)


def norms(triples, V, norm="local"):
    """(n_f, n_b) per edge in float64: the exact rational's rounding, not that of its float32 value"""
    if norm == "local":
        c_f, c_b = counts(triples)
        return 1.0 / c_f.astype(F64), 1.0 / c_b.astype(F64)
    from helpers import oracle_float64
    with oracle_float64():
        n_f, n_b = message_norms_f32(triples, V, norm)
    return n_f.astype(F64), n_b.astype(F64)


def message_list_norms(triples, V, R, norm, perm_relation):
    """what RGCN_BUF_MSG_NORM must hold for the message ids of RGCN_BUF_PERM_RELATION (m < E: forward message of edge m,
    m >= E: backward message of edge m - E), float32"""
    n_f, n_b = message_norms_f32(triples, V, norm)
    return np.concatenate([n_f, n_b]).astype(np.float32)[np.asarray(perm_relation)]


# ----------------------------------------------------------------------------- layers with the norms passed in
def _messages(kind, l, p, H, rows_in, r, tag):
    """[E, d] messages of one direction (tag 'f': W_forward from the subject, 'b': W_backward from the object)"""
    W = p["W_%s%d" % (tag, l)]
    E = len(r)
    if kind == "block":
        R, nb, sd, _ = W.shape
        return np.einsum("ebij,ebj->ebi", W[r], H[rows_in].reshape(E, nb, sd)).reshape(E, nb * sd)
    C = p["C_%s%d" % (tag, l)]
    if kind == "onehot" and l == 1:
        return np.einsum("eb,ebk->ek", C[r], W[rows_in])
    d_in, B, d_out = W.shape
    return np.einsum("ebk,eb->ek", (H[rows_in] @ W.reshape(d_in, B * d_out)).reshape(E, B, d_out), C[r])


def _drop(mode, keep, masks, l, shape, dtype=F64):
    return np.asarray(masks[l - 1], dtype=dtype) / dtype(keep) if mode == "train" else np.ones(shape, dtype=dtype)


def forward(kind, params, triples, V, L, n_f, n_b, mode="train", keep=0.8, masks=None, dtype=F64):
    """[H0, ..., HL] in float64; kind 'block' | 'basis' | 'onehot' (the featureless basis encoder: H0 is None).
    dtype=np.float32: the same formulas with every array and every operation in float32, one summation order (what
    tests/test_fullgraph_grid.py sizes the full-graph bounds with)"""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    n_f, n_b = np.asarray(n_f, dtype=dtype), np.asarray(n_b, dtype=dtype)
    s, r, o = oracle.split_graph(triples)
    H = None if kind == "onehot" else np.maximum(p["W_emb"] + p["b_emb"], dtype(0))
    acts = [H]
    for l in range(1, L + 1):
        Ws = p["W_self%d" % l]
        S = Ws if (kind == "onehot" and l == 1) else H @ Ws
        pre = S * _drop(mode, keep, masks, l, S.shape, dtype)
        if len(s):
            np.add.at(pre, o, _messages(kind, l, p, H, s, r, "f") * n_f[:, None])
            np.add.at(pre, s, _messages(kind, l, p, H, o, r, "b") * n_b[:, None])
        H = np.maximum(pre, dtype(0)) if l < L else pre
        assert H.dtype == dtype
        acts.append(H)
    return acts


def backward(kind, params, triples, V, L, n_f, n_b, acts, dcodes, mode="train", keep=0.8, masks=None, dtype=F64):
    """gradient of <dcodes, HL> with respect to every encoder parameter, evaluated at the given activations; dtype as in
    forward()"""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    n_f, n_b = np.asarray(n_f, dtype=dtype), np.asarray(n_b, dtype=dtype)
    s, r, o = oracle.split_graph(triples)
    E = len(s)
    acts = [None if a is None else np.asarray(a, dtype=dtype) for a in acts]
    grads = {}
    dH = np.asarray(dcodes, dtype=dtype)
    for l in range(L, 0, -1):
        Hin, table = acts[l - 1], kind == "onehot" and l == 1
        D = dH * (acts[l] > 0) if l < L else dH
        dS = D * _drop(mode, keep, masks, l, D.shape, dtype)
        grads["W_self%d" % l] = dS if table else Hin.T @ dS
        grads["b%d" % l] = np.zeros(D.shape[1], dtype=dtype)
        dHin = None if table else dS @ p["W_self%d" % l].T
        for tag, rows_in, rows_out, nrm in (("f", s, o, n_f), ("b", o, s, n_b)):
            W = p["W_%s%d" % (tag, l)]
            gW = np.zeros_like(W)
            g = D[rows_out] * nrm[:, None] if E else np.zeros((0, D.shape[1]), dtype=dtype)
            if kind == "block":
                R, nb, sd, _ = W.shape
                g3, x3 = g.reshape(E, nb, sd), Hin[rows_in].reshape(E, nb, sd)
                np.add.at(gW, r, np.einsum("ebi,ebj->ebij", g3, x3))
                np.add.at(dHin, rows_in, np.einsum("ebij,ebi->ebj", W[r], g3).reshape(E, nb * sd))
            else:
                C = p["C_%s%d" % (tag, l)]
                gC = np.zeros_like(C)
                gterms = C[r][:, :, None] * g[:, None, :]                       # [E, B, d]
                if table:
                    np.add.at(gW, rows_in, gterms)
                    np.add.at(gC, r, np.einsum("ebk,ek->eb", W[rows_in], g))
                else:
                    d_in, B, d_out = W.shape
                    x = Hin[rows_in]
                    terms = (x @ W.reshape(d_in, B * d_out)).reshape(E, B, d_out)
                    np.add.at(gC, r, np.einsum("ebk,ek->eb", terms, g))
                    gW += (x.T @ gterms.reshape(E, B * d_out)).reshape(W.shape)
                    np.add.at(dHin, rows_in, gterms.reshape(E, B * d_out) @ W.reshape(d_in, B * d_out).T)
                grads["C_%s%d" % (tag, l)] = gC
            grads["W_%s%d" % (tag, l)] = gW
        dH = dHin
    if kind != "onehot":
        g0 = dH * (acts[0] > 0)
        grads["W_emb"], grads["b_emb"] = g0, g0.sum(axis=0)
    return grads


# ----------------------------------------------------------------------------- the graphs the tests share
def base_graph():
    """V = 12, R = 4 (relation 3 has no edge).  Vertex 0 receives three edges of relation 0 and one of relation 1:
    local 1/3 and 1 against 1/4 intended; vertex 1 sends three of relation 0 and one of relation 2: the mirror case.
    A duplicated triple, a self-edge, and a few plain edges."""
    t = [(2, 0, 0), (3, 0, 0), (4, 0, 0), (5, 1, 0),            # into vertex 0
         (1, 0, 6), (1, 0, 7), (1, 0, 8), (1, 2, 9),            # out of vertex 1
         (6, 2, 7), (6, 2, 7),                                  # a duplicate
         (9, 1, 9),                                             # a self-edge
         (10, 2, 11), (11, 1, 10), (3, 2, 4), (8, 0, 5)]
    return np.asarray(t, dtype=np.int32)


def extended_graph(V=40, R=5, E=150, seed=0, hub=True):
    """base_graph (relation R - 1 stays without an edge) + a hub (vertex V - 1: more than 32 slots, reached by relations
    0 and 1 as object and as subject) + random edges, shuffled"""
    rng = np.random.RandomState(seed)
    parts = [base_graph()]
    if hub:
        n = 12
        for rel in (0, 1):
            parts.append(np.stack([rng.randint(12, V - 1, n), np.full(n, rel), np.full(n, V - 1)], 1))
            parts.append(np.stack([np.full(n, V - 1), np.full(n, rel), rng.randint(12, V - 1, n)], 1))
    have = sum(len(x) for x in parts)
    n = E - have
    parts.append(np.stack([rng.randint(0, V, n), rng.randint(0, R - 1, n), rng.randint(0, V, n)], 1))
    t = np.concatenate(parts).astype(np.int32)
    return t[rng.permutation(len(t))]
