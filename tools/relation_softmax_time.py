"""The relation-softmax term's launches, and the train step with the term off, on, and with relation corruptions
instead, in one run:

    python tools/relation_softmax_time.py [reps] [steps]

K, the known positives of the masked form, is the training set: the real one when data/FB-Toutanova lies beside the
package, otherwise 272,115 synthetic triples with oracle.synthetic_graph's skewed relation and entity frequencies (the
output says which).

1. Every launch of the term (rgcn_profile_*: HIP events around each launch, side streams off), plain and masked, after a
   decoder pass, `reps` (default 10) calls after two warm-ups, microseconds per launch:
     - at the FB15k-237 minibatch on a gcn_block context (V = 14,541, R = 237, d = 500, 100 blocks, L = 2): 30,000
       positives;
     - at the `Name=embedding` size on an embedding context of the same V, R and d: all 272,115 training triples, which the
       term walks in chunks.
2. The fb237 block train step (rgcn_train_step_minibatch_device: 30,000 batch edges, 15,000 kept, rate 10, clip + Adam,
   plain sampler): the term off, on (weight 0.5), on and masked, and -- the comparison the term exists for -- the term
   off with RelationNegativeSampleRate 1 and 2; the round repeated, milliseconds per step from HIP events around `steps`
   (default 30) consecutive steps after three warm-ups, the smaller of the two rounds reported."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402
from relation_negatives_time import training_set  # noqa: E402

V, R, D, NB, L, BATCH, KEEP, RATE, WEIGHT = 14541, 237, 500, 100, 2, 30000, 15000, 10, 0.5


def launches(eng, positives, reps):
    """per-launch microseconds of one rgcn_relation_softmax_device call, plain and masked"""
    P = len(positives)
    y = np.ones(P, dtype=np.float32)
    pd, yd = eng.to_device(positives), eng.to_device(y)
    eng.decoder_reserve(P)
    eng.relation_softmax_reserve(P)
    out = {"positives": P, "plan": _native.relation_softmax_plan(P, R, D)}
    try:
        eng.forward(train=True, seed=1)
        eng.decoder_loss_backward_device(pd, yd, P, 0.01)
        for masked in (False, True):
            for _ in range(2):
                eng.relation_softmax_device(pd, P, WEIGHT, exclusive=masked)
            eng.sync()
            eng.profile_enable(True)
            eng.profile_reset()
            for _ in range(reps):
                eng.relation_softmax_device(pd, P, WEIGHT, exclusive=masked)
            rows = [p for p in eng.profile() if p["name"].startswith(("relsm_", "splitk_reduce"))]
            eng.profile_enable(False)
            out["masked" if masked else "plain"] = {
                "us_per_call": {p["name"]: 1e3 * p["total_ms"] / reps for p in rows},
                "launches_per_call": {p["name"]: p["calls"] / float(reps) for p in rows},
                "sum_us_per_call": 1e3 * sum(p["total_ms"] for p in rows) / reps}
        eng.decoder_loss_backward_device(pd, yd, P, 0.01)
        base = eng.loss()
        eng.relation_softmax_device(pd, P, WEIGHT)
        out["term"] = eng.loss() - base
    finally:
        for b in (pd, yd):
            b.free()
    return out


def train_steps(eng, train, steps):
    rng = np.random.RandomState(3)
    batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
    N = BATCH * (RATE + 1 + 2)
    eng.decoder_reserve(N)
    eng.relation_softmax_reserve(BATCH)
    eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
    # (name, weight, masked, relation corruptions per positive)
    configs = [("off", 0.0, False, 0), ("term", WEIGHT, False, 0), ("term_masked", WEIGHT, True, 0),
               ("relation_negatives_1", 0.0, False, 1), ("relation_negatives_2", 0.0, False, 2)]
    out = {"batch_edges": BATCH, "kept": KEEP, "steps": steps, "rounds": []}
    try:
        count = 0
        for name, weight, masked, m in configs + configs:
            eng.set_relation_softmax(weight, 0, exclusive=masked)
            eng.set_relation_negatives(m)
            for _ in range(3):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, RATE, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            eng.sync()
            eng.timer_start()
            for _ in range(steps):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, RATE, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            out["rounds"].append({"config": name, "ms": eng.timer_stop() / steps})
        out["loss_at_end"] = eng.loss()
    finally:
        eng.set_relation_softmax(0.0)
        eng.set_relation_negatives(0)
        for b in (bd, xd, yd):
            b.free()
    out["ms_per_step"] = {name: min(r["ms"] for r in out["rounds"] if r["config"] == name) for name, _, _, _ in configs}
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rng = np.random.RandomState(0)
    train, source = training_set(rng)
    out = {"V": V, "R": R, "d": D, "blocks": NB, "layers": L, "known_positives": source, "triples": len(train),
           "weight": WEIGHT, "reps": reps}
    eng = _native.Engine(V, R, D, L, "block", NB, max_edges=BATCH)
    try:
        eng.set_params(oracle.init_params(V, R, D, L, "block", NB, rng=rng))
        eng.known_positives_reserve(train)
        batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
        eng.set_graph(batch[:KEEP])
        eng.set_overlap(False)
        out["minibatch"] = launches(eng, batch, reps)
        eng.set_overlap(True)
        out["train_step"] = train_steps(eng, train, steps)
    finally:
        eng.close()
    emb = _native.Engine(V, R, D, 0, "embedding", 1)
    try:
        w = (rng.randn(V, D) * 0.1).astype(np.float32)
        emb.set_params({"W_emb": w, "b_emb": np.zeros(D, np.float32), "W_relation": (rng.randn(V, D) * 0.1).astype(np.float32)})
        emb.known_positives_reserve(train)
        emb.set_overlap(False)
        out["embedding"] = launches(emb, train, max(2, reps // 3))
    finally:
        emb.close()
    print(json.dumps(out, indent=1))
    for where in ("minibatch", "embedding"):
        for form in ("plain", "masked"):
            s = out[where][form]
            print("%s, %d positives, %s: %.1f us per call: %s"
                  % (where, out[where]["positives"], form, s["sum_us_per_call"],
                     ", ".join("%s %.1f" % kv for kv in sorted(s["us_per_call"].items()))))
    t = out["train_step"]["ms_per_step"]
    print("train step, ms: " + ", ".join("%s %.4f" % (k, t[k]) for k in
                                         ("off", "term", "term_masked", "relation_negatives_1", "relation_negatives_2")))


if __name__ == "__main__":
    main()
