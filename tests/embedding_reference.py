"""Float64 restatement of the DistMult baseline (Encoder.Name=embedding; the reference's model_builder.py:27-41,
affine_transform.py with onehot_input=True, use_bias=False, use_nonlinearity=False, relation_embedding.py,
bilinear_diag.py) and of the ensemble rank of the reference's tools/ensemble.py (WeightEnsemble.combine_prediction), with
the inputs the CPU and GPU tests of both share.  No GPU, no library."""
import os

import numpy as np

import oracle
from helpers import GOLDEN_DIR, oracle_float64

NAMES = ["W_emb", "b_emb", "W_relation"]          # Model.get_weights() order


def load_fixture():
    """tests/golden/reference_embedding.npz (make_reference_embedding_fixture.py) as a case dictionary"""
    z = np.load(os.path.join(GOLDEN_DIR, "reference_embedding.npz"))
    V, R, d, N, seed = (int(x) for x in z["config"])
    c = {"V": V, "R": R, "d": d, "N": N, "seed": seed, "chain": str(z["chain"]).split(","), "triples": z["triples"],
         "X": z["X"], "Y": z["Y"], "loss": float(z["loss_train"]), "codes_train": z["codes_train"],
         "codes_test": z["codes_test"], "subject_scores": z["subject_scores"], "object_scores": z["object_scores"]}
    c["params"] = {n: z["weight%02d" % i] for i, n in enumerate(NAMES)}
    c["grads"] = {n: z["grad%02d" % i] for i, n in enumerate(NAMES)}
    c["connected"] = {n: bool(z["grad%02d_connected" % i]) for i, n in enumerate(NAMES)}
    return c


def codes(params, mode="train"):
    """the codes ARE the table: no bias, no relu, no dropout, in either mode"""
    assert mode in ("train", "test")
    return params["W_emb"].astype(np.float64)


def loss_and_grads(params, X, Y, reg=0.01):
    """(loss + regulariser, {name: gradient}) in float64; the decoder half is oracle.distmult_loss_and_grads, the encoder
    half the identity: dL/dW_emb = dL/dcodes, and b_emb -- never read -- gets zeros"""
    with oracle_float64():
        loss, dcodes, dwrel = oracle.distmult_loss_and_grads(codes(params), params["W_relation"].astype(np.float64),
                                                             X, Y, reg)
    return loss, {"W_emb": dcodes, "b_emb": np.zeros(params["b_emb"].shape, np.float64), "W_relation": dwrel}


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def energies(params, queries, object_side):
    """float64 [N, V]: every entity against the fixed entity and relation of each query (bilinear_diag.py:51-61)"""
    c, w = codes(params), params["W_relation"].astype(np.float64)
    q = np.asarray(queries)
    fixed = c[q[:, 0]] if object_side else c[q[:, 2]]
    return (fixed * w[q[:, 1]]) @ c.T


def all_scores(params, X, object_side):
    return sigmoid64(energies(params, X, object_side))


def adam_steps_float64(params, grads_per_step, names, lr, b1, b2, eps, max_norm):
    """clip_by_global_norm + Adam in float64 over several steps, each step's gradients given (the device's): the weights
    after every step.  Step 1 is test_gpu_featureless.adam_float64."""
    w = {n: params[n].astype(np.float64) for n in names}
    m = {n: np.zeros_like(w[n]) for n in names}
    v = {n: np.zeros_like(w[n]) for n in names}
    out = []
    for t, grads in enumerate(grads_per_step, start=1):
        gn = np.sqrt(sum(float(np.sum(grads[n].astype(np.float64) ** 2)) for n in names))
        scale = max_norm / max(gn, max_norm)
        lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        for n in names:
            g = grads[n].astype(np.float64) * scale
            m[n] = b1 * m[n] + (1 - b1) * g
            v[n] = b2 * v[n] + (1 - b2) * g * g
            w[n] = w[n] - lr_t * m[n] / (np.sqrt(v[n]) + eps)
        out.append({n: w[n].copy() for n in names})
    return out


# ---------------------------------------------------------------- ensemble ranks
def mixed_scores(ea, eb, w):
    """float64 w * sigmoid(ea) + (1 - w) * sigmoid(eb)"""
    return w * sigmoid64(ea) + (1.0 - w) * sigmoid64(eb)


def mixed_ranks(ea, eb, w, gold, lists):
    """rgcn_rank_mixed_device's definition in float64.  ea, eb [N, V] energies of the two models, gold [N], lists: per
    query the filter list (entity ids; duplicates count as often as they appear, as on the device).
    raw = #{e : m[e] >= m[gold]}, filtered = raw - #{e in list : m[e] >= m[gold]} + 1."""
    m = mixed_scores(ea, eb, w)
    raw, filt = [], []
    for i, g in enumerate(gold):
        above = m[i] >= m[i, g]
        lst = np.asarray(lists[i], dtype=np.int64)
        raw.append(int(above.sum()))
        filt.append(raw[-1] - int(above[lst].sum()) + 1)
    return np.asarray(raw, np.int32), np.asarray(filt, np.int32)


def ensemble_rule(target, others, w_pair):
    """WeightEnsemble.combine_prediction restated directly (tools/ensemble.py): (target, others) per model are the score of
    the gold entity and the scores of the candidates that REMAIN after filtering; rank = 1 + #{others >= target}"""
    w = w_pair
    t = w * target[0] + (1 - w) * target[1]
    o = w * np.asarray(others[0], np.float64) + (1 - w) * np.asarray(others[1], np.float64)
    return int(np.sum(o >= t)) + 1


TIE_MARGIN = 1e-5          # a query is comparable when no candidate's float64 mixed score lies this close to the gold's
MAX_LEFT_OUT = 0.05        # share of a case's queries the margin may leave out


def comparable(ea, eb, w, gold):
    """bool [N]: the float32 evaluation on the device and the float64 one above must agree on these queries"""
    m = mixed_scores(ea, eb, w)
    ok = np.ones(len(gold), dtype=bool)
    for i, g in enumerate(gold):
        gap = np.abs(m[i] - m[i, g])
        gap[g] = np.inf
        ok[i] = gap.min() > TIE_MARGIN
    return ok


MIXED_WEIGHTS = (0.4, 0.5)
MIXED_SHAPES = {"V300": (300, 7, 16, 96), "V30": (30, 4, 16, 30)}       # name -> (V, R, d, queries per side)


def mixed_case(name):
    """Two embedding parameter sets over the same entities and the queries both sides of the mixed-rank tests rank: codes
    ~ N(0, 0.6^2), W_relation ~ N(0, 1).  V = 300 is no multiple of the 256-thread workgroup, V = 30 has fewer entities
    than threads.  Filter lists per query and side: the gold among three to six random others; every fifth list holds
    duplicates, every seventh is empty.  The partner's energies are rounded to float32 HERE: they are an input."""
    V, R, d, n = MIXED_SHAPES[name]
    rng = np.random.RandomState(1000 + V)

    def params():
        return {"W_emb": (rng.randn(V, d) * 0.6).astype(np.float32), "b_emb": np.zeros(d, np.float32),
                "W_relation": rng.randn(V, d).astype(np.float32)}

    a, b = params(), params()
    queries = np.stack([rng.randint(0, V, n), rng.randint(0, R, n), rng.randint(0, V, n)], 1).astype(np.int32)
    case = {"V": V, "R": R, "d": d, "n": n, "a": a, "b": b, "queries": queries, "sides": {}}
    for object_side in (True, False):
        gold = queries[:, 2] if object_side else queries[:, 0]
        lists = []
        for i in range(n):
            if i % 7 == 6:
                lists.append([])
                continue
            lst = [int(gold[i])] + [int(e) for e in rng.randint(0, V, rng.randint(3, 7))]
            if i % 5 == 4:
                lst = lst + lst[:2]
            lists.append(lst)
        ptr = np.zeros(n + 1, np.int64)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        idx = np.asarray([e for x in lists for e in x], dtype=np.int32)
        case["sides"][object_side] = {"gold": gold, "lists": lists, "ptr": ptr, "idx": idx,
                                      "ea": energies(a, queries, object_side),
                                      "eb": energies(b, queries, object_side).astype(np.float32)}
    return case
