"""The entity-softmax term's launches, and the train step with the term off, on, masked and cut down by
EntitySoftmaxPositives, in one run:

    python tools/entity_softmax_time.py [reps] [steps]

K, the known positives of the masked form, is the training set: the real one when data/FB-Toutanova lies beside the
package, otherwise 272,115 synthetic triples with oracle.synthetic_graph's skewed relation and entity frequencies (the
output says which).  The positives are drawn from it either way.

1. Every launch of the term (rgcn_profile_*: HIP events around each launch, side streams off), plain and masked, after a
   decoder pass, `reps` (default 3) calls after one warm-up, microseconds per launch summed over the call's chunks:
     - at the FB15k-237 minibatch on a gcn_block context (V = 14,541, R = 237, d = 500, 100 blocks, L = 2): 30,000
       positives, 60,000 rows, 14 chunks of 4,608;
     - at the `Name=embedding` size on an embedding context of the same V, R and d: all 272,115 training triples
       (one call: the term is three products of 544,230 x 14,541 x 500).
2. The fb237 block train step (rgcn_train_step_minibatch_device: 30,000 batch edges, 15,000 kept, rate 10, clip + Adam,
   plain sampler): the term off, on (weight 0.5), on and masked, and on over the leading 1,024 and 4,096 positives
   (EntitySoftmaxPositives); the round repeated, milliseconds per step from HIP events around consecutive steps after
   warm-ups (`steps`, default 30, for the cheap configurations; a tenth of that, at least 2, where the whole batch is
   taken), the smaller of the two rounds reported."""
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


def launches(eng, positives, reps, warm=1):
    """per-launch microseconds of one rgcn_entity_softmax_device call, plain and masked"""
    P = len(positives)
    y = np.ones(P, dtype=np.float32)
    pd, yd = eng.to_device(positives), eng.to_device(y)
    eng.decoder_reserve(P)
    eng.entity_softmax_reserve(P)
    out = {"positives": P, "plan": _native.entity_softmax_plan(P, V, D)}
    try:
        eng.forward(train=True, seed=1)
        eng.decoder_loss_backward_device(pd, yd, P, 0.01)
        for masked in (False, True):
            for _ in range(warm):
                eng.entity_softmax_device(pd, P, WEIGHT, exclusive=masked)
            eng.sync()
            eng.profile_enable(True)
            eng.profile_reset()
            for _ in range(reps):
                eng.entity_softmax_device(pd, P, WEIGHT, exclusive=masked)
            rows = [p for p in eng.profile() if p["name"].startswith(("entsm_", "splitk_reduce"))]
            eng.profile_enable(False)
            out["masked" if masked else "plain"] = {
                "us_per_call": {p["name"]: 1e3 * p["total_ms"] / reps for p in rows},
                "launches_per_call": {p["name"]: p["calls"] / float(reps) for p in rows},
                "sum_us_per_call": 1e3 * sum(p["total_ms"] for p in rows) / reps}
        eng.decoder_loss_backward_device(pd, yd, P, 0.01)
        base = eng.loss()
        eng.entity_softmax_device(pd, P, WEIGHT)
        out["term"] = eng.loss() - base
    finally:
        for b in (pd, yd):
            b.free()
    return out


def train_steps(eng, train, steps):
    rng = np.random.RandomState(3)
    batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
    N = BATCH * (RATE + 1)
    eng.decoder_reserve(N)
    eng.entity_softmax_reserve(BATCH)
    eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
    few = max(2, steps // 10)
    # (name, weight, masked, EntitySoftmaxPositives, timed steps)
    configs = [("off", 0.0, False, 0, steps), ("term", WEIGHT, False, 0, few), ("term_masked", WEIGHT, True, 0, few),
               ("term_1024", WEIGHT, False, 1024, steps), ("term_4096", WEIGHT, False, 4096, steps)]
    out = {"batch_edges": BATCH, "kept": KEEP, "steps": steps, "steps_whole_batch": few, "rounds": []}
    try:
        count = 0
        for name, weight, masked, limit, timed in configs + configs:
            eng.set_entity_softmax(weight, limit, exclusive=masked)
            for _ in range(3 if timed == steps else 1):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, RATE, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            eng.sync()
            eng.timer_start()
            for _ in range(timed):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, RATE, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            out["rounds"].append({"config": name, "ms": eng.timer_stop() / timed})
        out["loss_at_end"] = eng.loss()
    finally:
        eng.set_entity_softmax(0.0)
        for b in (bd, xd, yd):
            b.free()
    out["ms_per_step"] = {c[0]: min(r["ms"] for r in out["rounds"] if r["config"] == c[0]) for c in configs}
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
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
        out["embedding"] = launches(emb, train, 1, warm=0)
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
    print("train step, ms: " + ", ".join("%s %.4f" % (k, t[k]) for k in ("off", "term", "term_masked", "term_1024", "term_4096")))


if __name__ == "__main__":
    main()
