"""float64 numpy restatement of the featureless basis encoder (Name=gcn_basis, UseInputTransform=No, Concatenation=No):
the first BasisGcn has onehot_input=True (code/common/model_builder.py:140-165,277-283), so dot_or_lookup takes its
lookup branch (shared_functions.py:5-9) and layer 1's weights are per-entity tables (gcn_basis.py:16-24,60-71,
message_gcn.py:28-79).  TEST INFRASTRUCTURE: layer 1 is written out as the gathers and scatters it is, layers 2..L and
the normalisation values are the oracle's own functions, run in float64.

    pre1[v] = dropout(W_self)[v] + sum_{m -> v} n_m sum_b C_dir(m)[rel_m,b] W_dir(m)[src_m,b,:]
    H1      = relu(pre1) if L > 1 else pre1

Forward messages (W_forward, C_forward) go from subject to object and are normalised by the object's row of the
forward incidence matrix; backward messages (W_backward, C_backward) from object to subject, by the subject's row of
the backward one."""
import numpy as np

import oracle
from helpers import oracle_float64

F64 = np.float64


def weight_names(L):
    """get_weights() order: no W_emb / b_emb; per layer gcn_basis.py:33-37; W_relation last."""
    names = []
    for l in range(1, L + 1):
        names += ["W_f%d" % l, "W_b%d" % l, "C_f%d" % l, "C_b%d" % l, "W_self%d" % l, "b%d" % l]
    return names + ["W_relation"]


def init_params(V, R, d, L, B, rng):
    """The reference's creation order (outermost component first, model.py:156-164): RelationEmbedding, top layer ...
    layer 1; layer 1's three V-sized tensors with std glorot_variance([V, d]) (gcn_basis.py:16-24)."""
    p = {"W_relation": rng.randn(V, d).astype(np.float32)}
    for l in range(L, 0, -1):
        d_in = V if l == 1 else d
        std = oracle.glorot_variance([d_in, d])
        p["W_f%d" % l] = rng.normal(0, std, size=(d_in, B, d)).astype(np.float32)
        p["W_b%d" % l] = rng.normal(0, std, size=(d_in, B, d)).astype(np.float32)
        p["W_self%d" % l] = rng.normal(0, std, size=(d_in, d)).astype(np.float32)
        p["C_f%d" % l] = rng.normal(0, 1, size=(R, B)).astype(np.float32)
        p["C_b%d" % l] = rng.normal(0, 1, size=(R, B)).astype(np.float32)
        p["b%d" % l] = np.zeros(d, dtype=np.float32)
    return p


def _norms(triples, V, norm_mode):
    s, r, o = oracle.split_graph(triples)
    with oracle_float64():
        n_f = oracle.incidence_values(o, V, norm_mode).astype(F64)
        n_b = oracle.incidence_values(s, V, norm_mode).astype(F64)
    return s, r, o, n_f, n_b


def _dropscale(mode, keep, mask, shape):
    if mode != "train":
        return np.ones(shape, dtype=F64)
    return np.asarray(mask, dtype=F64) / F64(keep)


def forward(params, triples, V, L, mode="train", keep=0.8, masks=None, norm_mode=oracle.NORM_INTENDED):
    """[None, H1, ..., HL] in float64 (there is no H0)."""
    p = {k: np.asarray(v, dtype=F64) for k, v in params.items()}
    s, r, o, n_f, n_b = _norms(triples, V, norm_mode)
    d = p["W_self1"].shape[1]
    pre = p["W_self1"] * _dropscale(mode, keep, None if masks is None else masks[0], (V, d))
    if len(s):
        msg_f = np.einsum("eb,ebk->ek", p["C_f1"][r], p["W_f1"][s]) * n_f[:, None]      # lands on the object
        msg_b = np.einsum("eb,ebk->ek", p["C_b1"][r], p["W_b1"][o]) * n_b[:, None]      # lands on the subject
        np.add.at(pre, o, msg_f)
        np.add.at(pre, s, msg_b)
    H = np.maximum(pre, 0.0) if L > 1 else pre
    acts = [None, H]
    with oracle_float64():
        for l in range(2, L + 1):
            F, K = oracle.basis_messages(H, s, r, o, p["W_f%d" % l], p["W_b%d" % l], p["C_f%d" % l], p["C_b%d" % l])
            S = oracle.self_loop(H, p["W_self%d" % l])
            if mode == "train":
                S = oracle.dropout(S, keep, np.asarray(masks[l - 1]))
            H = oracle.combine_messages(F, K, S, s, o, V, use_nonlinearity=l < L, norm_mode=norm_mode)
            acts.append(np.asarray(H, dtype=F64))
    return acts


def backward(params, triples, V, L, acts, dcodes, mode="train", keep=0.8, masks=None, norm_mode=oracle.NORM_INTENDED):
    """Gradients of every encoder parameter from dcodes = dL/dH_L, float64; name -> array."""
    p = {k: np.asarray(v, dtype=F64) for k, v in params.items()}
    s, r, o, n_f, n_b = _norms(triples, V, norm_mode)
    grads = {}
    if L > 1:
        # layers 2..L are an (L-1)-layer oracle encoder over the input H1: its "W_emb" gradient is dL/dH1 * (H1 > 0),
        # which is D = dL/dpre1
        sub = {"W_emb": acts[1], "b_emb": np.zeros(acts[1].shape[1])}
        for l in range(2, L + 1):
            for base in ("W_f", "W_b", "C_f", "C_b", "W_self", "b"):
                sub["%s%d" % (base, l - 1)] = p["%s%d" % (base, l)]
        with oracle_float64():
            g = oracle.encoder_backward(sub, triples, V, L - 1, oracle.KIND_BASIS,
                                        [np.asarray(a, dtype=F64) for a in acts[1:]], np.asarray(dcodes, dtype=F64),
                                        mode=mode, keep_prob=keep, dropout_masks=None if masks is None else masks[1:],
                                        norm_mode=norm_mode)
        for l in range(2, L + 1):
            for base in ("W_f", "W_b", "C_f", "C_b", "W_self", "b"):
                grads["%s%d" % (base, l)] = np.asarray(g["%s%d" % (base, l - 1)], dtype=F64)
        D = np.asarray(g["W_emb"], dtype=F64)
    else:
        D = np.asarray(dcodes, dtype=F64)
    grads["W_self1"] = D * _dropscale(mode, keep, None if masks is None else masks[0], D.shape)
    gWf, gWb = np.zeros_like(p["W_f1"]), np.zeros_like(p["W_b1"])
    gCf, gCb = np.zeros_like(p["C_f1"]), np.zeros_like(p["C_b1"])
    if len(s):
        dF = D[o] * n_f[:, None]          # gradient of every forward message
        dK = D[s] * n_b[:, None]
        np.add.at(gWf, s, p["C_f1"][r][:, :, None] * dF[:, None, :])
        np.add.at(gWb, o, p["C_b1"][r][:, :, None] * dK[:, None, :])
        np.add.at(gCf, r, np.einsum("ebk,ek->eb", p["W_f1"][s], dF))
        np.add.at(gCb, r, np.einsum("ebk,ek->eb", p["W_b1"][o], dK))
    grads.update({"W_f1": gWf, "W_b1": gWb, "C_f1": gCf, "C_b1": gCb, "b1": np.zeros(D.shape[1])})
    return grads


def make_case(V, R, d, L, B, E, seed=0, keep=0.8):
    """params, triples, masks, dcodes of a seeded featureless workload"""
    rng = np.random.RandomState(seed)
    params = init_params(V, R, d, L, B, rng)
    triples = np.stack([rng.randint(0, V, size=E), rng.randint(0, R, size=E), rng.randint(0, V, size=E)],
                       axis=1).astype(np.int32).reshape(E, 3)
    masks = [(rng.rand(V, d) < keep).astype(np.uint8) for _ in range(L)]
    dcodes = (rng.randn(V, d) * 1e-1).astype(np.float32)
    return params, triples, masks, dcodes
