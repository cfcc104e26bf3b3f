"""Float64 mirror of the self-adversarial negative weights and of the weighted DistMult decoder (include/rgcn.h,
rgcn_adversarial_weights_device, rgcn_decoder_loss_backward_weighted_device, rgcn_set_adversarial_negatives), and the
inputs of the GPU cases.  numpy, and scipy's sparse product for the decoder's scatter-adds (the oracle's own for the fp32 restatement);
shared by the host and the GPU tests.

A batch of N rows: the first P are the positives, row i >= P is a negative of positive i mod P, K = N / P - 1.

    p_i  = exp(alpha x_i - M_b) / sum_{j in G_b} exp(alpha x_j - M_b),   M_b = max over the group
    w_i  = K p_i for a negative, 1 for a positive
    loss = (1/N) sum_n w_n xent(x_n, y_n) + reg (mean e1^2 + mean r^2 + mean e2^2)
    dx_n = w_n (sigmoid(x_n) - y_n) / N                  (the weights are constants)

The weight tolerance is derived: a float32 energy of d terms a_k b_k e_k, each a product of two roundings, summed by
fused multiply-adds in any order, differs from the exact one by at most B = gamma_{d+2} sum_k |a_k b_k e_k|, gamma_n =
n u / (1 - n u), u = 2^-24.  Every exponent of a group's softmax then moves by at most alpha B (B the group's maximum), a
ratio of two of them by a factor within exp(+-2 alpha B); the float64 softmax itself and the final rounding cost less
than 4 ulp of the weight, and 1e-37 covers the weights that underflow."""
import numpy as np

import relation_negatives_reference as rnr

U = 2.0 ** -24


def float64_energies(codes, w_relation, X):
    """(x [N] float64, B [N]): the exact energies of the float32 inputs and the forward error bound of a float32 evaluation"""
    x = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    c = np.asarray(codes, dtype=np.float64)
    W = np.asarray(w_relation, dtype=np.float64)
    t = c[x[:, 0]] * W[x[:, 1]] * c[x[:, 2]]
    n = c.shape[1] + 2
    return t.sum(axis=1), n * U / (1.0 - n * U) * np.abs(t).sum(axis=1)


def group_weights(x, P, alpha):
    """the weights [N] of energies x [N] (float64), alpha as the device holds it (a float32)"""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    assert N % P == 0
    K = N // P - 1
    w = np.ones(N)
    if K == 0 or alpha == 0:
        return w
    a = np.float64(np.float32(alpha)) * x[P:].reshape(K, P)
    t = np.exp(a - a.max(axis=0, keepdims=True))
    w[P:] = (K * t / t.sum(axis=0, keepdims=True)).reshape(-1)
    return w


def weights(codes, w_relation, X, P, alpha):
    """dict: w [N] the mirror's weights, x [N] the energies, tol [N] what a device weight may differ by"""
    x, B = float64_energies(codes, w_relation, X)
    N = len(x)
    K = N // P - 1
    w = group_weights(x, P, alpha)
    tol = np.zeros(N)
    if K > 0 and alpha != 0:
        Bg = np.tile(B[P:].reshape(K, P).max(axis=0), K)
        w32 = w[P:].astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(w32), np.float32(1e-37))).astype(np.float64)
        tol[P:] = np.expm1(2.0 * float(np.float32(alpha)) * Bg) * w[P:] + 4.0 * ulp + 1e-37
    return {"w": w, "x": x, "tol": tol, "K": K}


def _weighted_decoder_float32(codes, w_relation, X, Y, w, reg):
    """the same weighted formula as oracle.distmult_loss_and_grads states the unweighted one: float32 products and sums,
    float64 only where that function uses it (the mean of the per-row terms and the regulariser)"""
    F = np.float32
    x = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    c, W = np.asarray(codes, dtype=F), np.asarray(w_relation, dtype=F)
    z, wt = np.asarray(Y, dtype=F), np.asarray(w, dtype=F)
    e1, r, e2 = c[x[:, 0]], W[x[:, 1]], c[x[:, 2]]
    n, d = e1.shape
    en = np.sum(e1 * r * e2, axis=1).astype(F)
    per = (1 - z) * en + (np.log1p(np.exp(-np.abs(en))) + np.maximum(-en, 0))
    loss = (wt * per).mean(dtype=np.float64) + reg * (np.mean(e1.astype(np.float64) ** 2) + np.mean(r.astype(np.float64) ** 2)
                                                      + np.mean(e2.astype(np.float64) ** 2))
    ex = np.exp(-np.abs(en))
    sig = np.where(en >= 0, 1.0 / (1.0 + ex), ex / (1.0 + ex))
    dx = (wt * ((sig - z) / n)).astype(F)
    dcol = n * d

    def segment_sum(index, rows, M):           # the oracle's _segment_sum_rows: a float32 sparse product
        import scipy.sparse as sp
        S = sp.csr_matrix((np.ones(n, dtype=F), (index, np.arange(n))), shape=(rows, n), dtype=F)
        return np.asarray(S @ M.astype(F), dtype=F)

    dcodes = segment_sum(x[:, 0], c.shape[0], dx[:, None] * (r * e2) + reg * 2.0 * e1 / dcol) \
        + segment_sum(x[:, 2], c.shape[0], dx[:, None] * (e1 * r) + reg * 2.0 * e2 / dcol)
    dW = segment_sum(x[:, 1], W.shape[0], dx[:, None] * (e1 * e2) + reg * 2.0 * r / dcol)
    return {"loss": float(loss), "dx": dx, "dcodes": dcodes.astype(F), "dW": dW, "x": en}


def weighted_decoder(codes, w_relation, X, Y, w, reg, codes_override=None, dtype=np.float64):
    """float64 mirror of the weighted decoder: dict loss, dx [N], dcodes [V,dc], dW [rows of w_relation, dc], x [N] the
    energies, per [N] the unweighted per-row loss terms (loss - mean(w per) + mean(per) is the unit-weight loss).
    dtype = numpy.float32: the fp32 restatement of the same formula, the yardstick of an l2 comparison."""
    if np.dtype(dtype) == np.float32:
        return _weighted_decoder_float32(codes, w_relation, X, Y, w, reg)
    assert np.dtype(dtype) == np.float64, dtype
    x = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    y = np.asarray(Y, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    c = np.asarray(codes, dtype=np.float64)
    W = np.asarray(w_relation, dtype=np.float64)
    e1, r, e2 = c[x[:, 0]], W[x[:, 1]], c[x[:, 2]]
    n, d = e1.shape
    en = np.sum(e1 * r * e2, axis=1)
    per = (1 - y) * en + np.log1p(np.exp(-np.abs(en))) + np.maximum(-en, 0)
    loss = (w * per).mean() + reg * (np.mean(e1 ** 2) + np.mean(r ** 2) + np.mean(e2 ** 2))
    dx = w * (1.0 / (1.0 + np.exp(-en)) - y) / n
    k = reg * 2.0 / (n * d)
    def scatter_add(index, rows, M):            # out[index[i]] += M[i], as a float64 sparse product (helpers.chunked_distmult_float64's)
        import scipy.sparse as sp
        return np.asarray(sp.csr_matrix((np.ones(n), (index, np.arange(n))), shape=(rows, n)) @ M)

    dcodes = scatter_add(x[:, 0], c.shape[0], dx[:, None] * (r * e2) + k * e1) \
        + scatter_add(x[:, 2], c.shape[0], dx[:, None] * (e1 * r) + k * e2)
    dW = scatter_add(x[:, 1], W.shape[0], dx[:, None] * (e1 * e2) + k * r)
    return {"loss": float(loss), "dx": dx, "dcodes": dcodes, "dW": dW, "x": en, "per": per}


def adversarial_decoder(codes, w_relation, X, Y, P, alpha, reg):
    """the objective of a fused step under the mode: the mirror's weights, then the weighted decoder"""
    w = weights(codes, w_relation, X, P, alpha)
    out = weighted_decoder(codes, w_relation, X, Y, w["w"], reg)
    out["w"], out["tol"] = w["w"], w["tol"]
    return out


# ------------------------------------------------------------------ the GPU cases' inputs
V_CASE, R_CASE = 90, 18
ALPHA = 1.5


def tables(V, R, dc, seed):
    """codes [V,dc] and W_relation [max(V,R),dc] scaled so that an energy (dc products of three entries) is of unit order"""
    rng = np.random.RandomState(seed)
    scale = 1.3 * dc ** (-1.0 / 6.0)
    codes = (rng.randn(V, dc) * scale).astype(np.float32)
    w_rel = (rng.randn(max(V, R), dc) * scale).astype(np.float32)
    return codes, w_rel


def batch(layout, V, R, P, K, seed):
    """X [P (K + 1), 3], Y: the positives, then K negatives of each in the samplers' order"""
    rng = np.random.RandomState(seed + 1000)
    pos = np.stack([rng.randint(0, V, P), rng.randint(0, R, P), rng.randint(0, V, P)], 1).astype(np.int32)
    rows = [pos]
    for t in range(K):
        neg = pos.copy()
        if layout == "entity":                       # object or subject replaced, as the entity samplers do
            side = rng.randint(0, 2, P) * 2
            neg[np.arange(P), side] = rng.randint(0, V, P)
        elif layout == "arbitrary":                  # a caller's own rows: no id shared with the positive
            for col, n in ((0, V), (1, R), (2, V)):
                neg[:, col] = (pos[:, col] + 1 + rng.randint(0, n - 1, P)) % n
        elif layout == "identical":
            pass
        else:
            raise ValueError(layout)
        rows.append(neg)
    X = np.concatenate(rows).astype(np.int32)
    Y = np.concatenate([np.ones(P), np.zeros(P * K)]).astype(np.float32)
    return X, Y


def sampled_batch(V, R, n, rate, m, seed):
    """what rgcn_negative_sample_relation_device(batch, n, rate, m, exclusive = 0, seed) writes (the byte-exact mirror of
    tests/relation_negatives_reference.py): (batch [n,3], X, Y)"""
    rng = np.random.RandomState(seed + 2000)
    b = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), rng.randint(0, V, n)], 1).astype(np.int32)
    s = rnr.sample(np.zeros(0, dtype=np.uint64), b, rate, m, V, R, seed, False)
    return b, s["X"].astype(np.int32), s["Y"].astype(np.float32)


LDS_CAP = 512        # energies of one group the weight kernel keeps in LDS (csrc/adversarial.hip, kAdvCap)

# (name, layout, P, K, dc): P round the four wavefronts of a workgroup and past one workgroup; K = 1 (all ones), 2, 10,
# 65 (past one wavefront of energies), one past the LDS cap; dc = the scalar path, float4 with T = 1, 1, 2, 4, the looped path
WEIGHT_CASES = (
    [("dc%d" % dc, "entity", 5, 10, dc) for dc in (6, 8, 132, 260, 516, 1028)] +
    [("P%d" % P, "entity", P, 10, 8) for P in (1, 3, 4, 129)] +
    [("K%d" % K, "entity", 5, K, 8) for K in (1, 2, 65)] +
    [("K%d-P3" % (LDS_CAP + 1), "entity", 3, LDS_CAP + 1, 8), ("K65-dc1028", "entity", 3, 65, 1028),
     ("K2-dc6", "entity", 4, 2, 6)] +
    [("arbitrary-dc%d" % dc, "arbitrary", 5, 10, dc) for dc in (6, 8, 132, 516, 1028)] +
    [("identical-dc%d" % dc, "identical", 5, 10, dc) for dc in (8, 1028)])
WEIGHT_CASE_NAMES = [c[0] for c in WEIGHT_CASES]


def weight_case(name):
    """dict of one case: codes, w_rel, X, Y, P, K, alpha, spreads (whether the case claims to test weighting)"""
    _, layout, P, K, dc = WEIGHT_CASES[WEIGHT_CASE_NAMES.index(name)]
    seed = WEIGHT_CASE_NAMES.index(name)
    codes, w_rel = tables(V_CASE, R_CASE, dc, seed)
    X, Y = batch(layout, V_CASE, R_CASE, P, K, seed)
    return dict(name=name, codes=codes, w_rel=w_rel, X=X, Y=Y, P=P, K=K, dc=dc, alpha=ALPHA,
                spreads=K >= 2 and layout != "identical")


def relation_rows_case(dc=8):
    """entity and relation corruptions as the device sampler writes them: n = 7, rate = 3, m = 2, K = 5"""
    codes, w_rel = tables(V_CASE, R_CASE, dc, 77)
    n, rate, m, seed = 7, 3, 2, 4321
    b, X, Y = sampled_batch(V_CASE, R_CASE, n, rate, m, seed)
    return dict(name="relation-rows", codes=codes, w_rel=w_rel, X=X, Y=Y, P=n, K=rate + m, dc=dc, alpha=ALPHA, batch=b,
                rate=rate, m=m, seed=seed, spreads=True)


def dominating_case():
    """one group (of positive 1) holds a negative whose energy is 300 / alpha above every other: its object is an entity
    built to align with codes[s] * W[r] of that positive"""
    dc, P, K = 8, 3, 10
    codes, w_rel = tables(V_CASE, R_CASE, dc, 99)
    X, Y = batch("entity", V_CASE - 1, R_CASE, P, K, 99)      # (entity V - 1 is the built one: no other row uses it)
    s, r = X[1, 0], X[1, 1]
    ab = codes[s].astype(np.float64) * w_rel[r].astype(np.float64)
    codes[V_CASE - 1] = (np.sign(ab) * (300.0 / ALPHA + 20.0) / np.abs(ab).sum()).astype(np.float32)
    big = 1 + 4 * P                                           # row of negative t = 3 of positive 1
    X[big] = (s, r, V_CASE - 1)
    return dict(name="dominating", codes=codes, w_rel=w_rel, X=X, Y=Y, P=P, K=K, dc=dc, alpha=ALPHA, big=big, spreads=True)


def all_weight_cases():
    return [weight_case(n) for n in WEIGHT_CASE_NAMES] + [relation_rows_case(), dominating_case()]


def decoder_case(dc, seed=5):
    """a weighted-decoder case: an arbitrary batch of 150 rows with labels of both kinds and caller's weights in [0, 3]
    with exact zeros among them"""
    rng = np.random.RandomState(seed + dc)
    codes, w_rel = tables(V_CASE, R_CASE, dc, seed + dc)
    N = 150
    X = np.stack([rng.randint(0, V_CASE, N), rng.randint(0, R_CASE, N), rng.randint(0, V_CASE, N)], 1).astype(np.int32)
    Y = (rng.rand(N) < 0.3).astype(np.float32)
    w = (rng.rand(N) * 3.0).astype(np.float32)
    w[rng.choice(N, 20, replace=False)] = 0.0
    return dict(codes=codes, w_rel=w_rel, X=X, Y=Y, w=w, dc=dc)
