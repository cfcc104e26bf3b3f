"""The reciprocal pass next to the entity sampler, and the train step with the mode off and on, in one run on one context:

    python tools/reciprocal_time.py [reps] [steps]

One FB15k-237 gcn_block context (V = 14,541, R = 237, d = 500, 100 blocks, L = 2).  The training set is the real one when
data/FB-Toutanova lies beside the package, otherwise 272,115 synthetic triples with oracle.synthetic_graph's skewed
relation and entity frequencies (the output says which).  Everything is at the FB15k-237 minibatch: n = 30,000 batch
triples, rate 10.

1. `reciprocal_rows` beside `negative_sample` of the same calls (rgcn_profile_*: HIP events around each launch, side
   streams off): `reps` (default 20) calls after two warm-ups, microseconds per launch.  The device's last output is checked
   against the numpy mirror (tests/reciprocal_reference.py).
2. The fb237 block train step (rgcn_train_step_minibatch_device: 30,000 batch edges, 15,000 kept, rate 10, clip + Adam,
   plain sampler) with the mode off, the mode on, RelationNegativeSampleRate = 1 with the mode off (the step the mode is
   expected to cost as much as: the same general path, the same n extra rows) and the mode-off step at rate 11 (the same N,
   all rows entity corruptions, the batch tiled: what the extra rows alone cost), the round repeated: milliseconds per
   step from HIP events around `steps` (default 30) consecutive steps after three warm-ups."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reciprocal_reference as ref  # noqa: E402
import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, NB, L, TRAIN, BATCH, KEEP, RATE = 14541, 237, 500, 100, 2, 272115, 30000, 15000, 10


def training_set(rng):
    path = os.path.join(ROOT, "data", "FB-Toutanova")
    if os.path.exists(os.path.join(path, "train.txt")):
        from relationprediction_amd import train as train_module
        splits, entities, relations = train_module.load_dataset(path)
        if len(entities) == V and len(relations) == R:
            return np.ascontiguousarray(splits["train"], dtype=np.int32), "data/FB-Toutanova/train.txt"
    return np.ascontiguousarray(oracle.synthetic_graph(V, R, TRAIN, rng), dtype=np.int32), "synthetic"


def pass_rows(eng, train, batch, reps, seed):
    n = len(batch)
    total = n * (RATE + 2)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * total), eng.alloc(4 * total)
    out = {"n": n, "rate": RATE, "rows": total, "threads": n * (RATE + 1)}
    try:
        for _ in range(2):
            eng.negative_sample_device(bd, n, RATE, seed, xd, yd, reciprocal=True)
        eng.sync()
        eng.profile_enable(True)
        eng.profile_reset()
        for i in range(reps):
            eng.negative_sample_device(bd, n, RATE, seed + i, xd, yd, reciprocal=True)
        rows = {p["name"]: p for p in eng.profile()}
        eng.profile_enable(False)
        for name in ("negative_sample", "reciprocal_rows"):
            out["%s_us" % name] = 1e3 * rows[name]["total_ms"] / rows[name]["calls"]
        want = ref.sample("plain", batch, train, RATE, 0, V, R, seed + reps - 1)
        out["device_equals_mirror"] = bool(np.array_equal(xd.download(np.int32, (total, 3)), want["X"]) and
                                           np.array_equal(yd.download(np.float32, (total,)), want["Y"]))
        out["share_subject_replaced"] = float((want["coin"] == 0).mean())
    finally:
        for b in (bd, xd, yd):
            b.free()
    return out


def train_steps(eng, train, steps):
    rng = np.random.RandomState(3)
    batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
    N = BATCH * (RATE + 2)
    eng.decoder_reserve(N)
    eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
    out = {"batch_edges": BATCH, "kept": KEEP, "steps": steps, "ms_per_step": []}
    # (name, rate, relation rate, reciprocal)
    configs = [("off", RATE, 0, False), ("reciprocal", RATE, 0, True), ("relation_rate_1", RATE, 1, False),
               ("off_rate_11", RATE + 1, 0, False)]
    try:
        count = 0
        for name, rate, m, reciprocal in configs + configs:
            eng.set_relation_negatives(m)
            eng.set_reciprocal_relations(reciprocal)
            for _ in range(3):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, rate, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            eng.sync()
            eng.timer_start()
            for _ in range(steps):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, rate, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            out["ms_per_step"].append({"step": name, "decoder_triples": BATCH * (rate + 1 + m + (1 if reciprocal else 0)),
                                       "ms": eng.timer_stop() / steps})
        out["loss_at_end"] = eng.loss()
    finally:
        eng.set_relation_negatives(0)
        eng.set_reciprocal_relations(False)
        for b in (bd, xd, yd):
            b.free()

    def best(name):
        return min(r["ms"] for r in out["ms_per_step"] if r["step"] == name)
    off, on, rel, tiled = best("off"), best("reciprocal"), best("relation_rate_1"), best("off_rate_11")
    out["summary"] = {"off_ms": off, "on_ms": on, "ratio": on / off, "growth_of_N": 1.0 / (RATE + 1),
                      "relation_rate_1_ms": rel, "on_over_relation_rate_1": on / rel, "tiled_at_the_same_N_ms": tiled,
                      "share_of_the_increase_from_the_rows_alone": (tiled - off) / (on - off) if on > off else None,
                      "untiled_layout_ms": on - tiled}
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rng = np.random.RandomState(0)
    train, source = training_set(rng)
    out = {"V": V, "R": R, "d": D, "blocks": NB, "layers": L, "training_set": source, "triples": len(train), "reps": reps}
    eng = _native.Engine(V, R, D, L, "block", NB, max_edges=BATCH)
    try:
        eng.set_params(oracle.init_params(V, R, D, L, "block", NB, rng=rng))
        eng.set_overlap(False)
        batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
        out["pass"] = pass_rows(eng, train, batch, reps, 1000)
        eng.set_overlap(True)
        out["train_step"] = train_steps(eng, train, steps)
    finally:
        eng.close()
    print(json.dumps(out, indent=1))
    p, s = out["pass"], out["train_step"]["summary"]
    print("reciprocal_rows %6.1f us per launch (%d threads), beside it negative_sample %6.1f us; %.1f %% of the negatives "
          "had their subject replaced; device == mirror: %s"
          % (p["reciprocal_rows_us"], p["threads"], p["negative_sample_us"], 100 * p["share_subject_replaced"],
             p["device_equals_mirror"]))
    print("train step, ms: " + ", ".join("%s %.4f" % (r["step"], r["ms"]) for r in out["train_step"]["ms_per_step"]))
    print("mode on %.4f ms against %.4f ms off, ratio %.3f (N grows by %.3f); RelationNegativeSampleRate=1: %.4f ms (on / "
          "that: %.3f); rate %d with the mode off, the same N tiled: %.4f ms; the untiled layout costs %.4f ms"
          % (s["on_ms"], s["off_ms"], s["ratio"], s["growth_of_N"], s["relation_rate_1_ms"], s["on_over_relation_rate_1"],
             RATE + 1, s["tiled_at_the_same_N_ms"], s["untiled_layout_ms"]))


if __name__ == "__main__":
    main()
