"""The self-adversarial weight kernel next to the decoder's energy kernel, and the train step with the mode off and on,
in one run:

    python tools/adversarial_time.py [reps] [steps]

Sizes of FB15k-237 (V = 14,541, R = 237, d = 500); the training set is synthetic (272,115 triples with
oracle.synthetic_graph's skewed relation and entity frequencies): no dataset travels with the tree.

1. One gcn_block context (100 blocks, L = 2), the FB15k-237 minibatch: 30,000 positives, rate 10, N = 330,000 rows.
   `reps` (default 10) fused minibatch steps at AdversarialTemperature 1 under rgcn_profile_* (HIP events around each
   launch, side streams off) after two warm-ups: microseconds per launch of `adv_weights` and of `dec_energy_rel` in the
   same steps.  The same with RelationNegativeSampleRate 2 (N = 390,000; the batch is not the tiled one).
2. One Name=embedding context, the whole training set as the batch: 272,115 positives, rate 10, N = 2,993,265 rows; the
   same two kernels from `reps` train steps.
3. The fb237 block train step (rgcn_train_step_minibatch_device: 30,000 batch edges, 15,000 kept, rate 10, clip + Adam) with
   the mode off and on, alternating, three rounds: milliseconds per step from HIP events around `steps` (default 30)
   consecutive steps after three warm-ups."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, NB, L, TRAIN, BATCH, KEEP, RATE = 14541, 237, 500, 100, 2, 272115, 30000, 15000, 10
ALPHA = 1.0


def kernel_rows(eng, step, reps):
    """microseconds per launch of the weight kernel and of the energy kernel over `reps` calls of step(i)"""
    for i in range(2):
        step(i)
    eng.sync()
    eng.profile_enable(True)
    eng.profile_reset()
    for i in range(reps):
        step(2 + i)
    rows = {p["name"]: p for p in eng.profile()}
    eng.profile_enable(False)
    out = {}
    for name in ("adv_weights", "dec_energy_rel"):
        out[name + "_us"] = 1e3 * rows[name]["total_ms"] / rows[name]["calls"]
        out[name + "_calls"] = rows[name]["calls"]
    out["ratio"] = out["adv_weights_us"] / out["dec_energy_rel_us"]
    return out


def block_context(train, rng, reps, steps):
    out = {}
    batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
    N = BATCH * (RATE + 1 + 2)
    with _native.Engine(V, R, D, L, "block", NB, max_edges=BATCH) as eng:
        eng.set_params(oracle.init_params(V, R, D, L, "block", NB, rng=rng))
        eng.decoder_reserve(N)
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)

        def step(i):
            eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + i, RATE, 200 + i, xd, yd, seed=i, reg_param=0.01)
        try:
            eng.set_overlap(False)
            eng.set_adversarial_negatives(ALPHA)
            out["minibatch"] = dict(kernel_rows(eng, step, reps), rows=BATCH * (RATE + 1), positives=BATCH)
            w = eng.read_buffer(_native.BUF_ADVERSARIAL_WEIGHTS)
            out["minibatch"]["weights_min_max_sum"] = [float(w.min()), float(w.max()), float(w.astype(np.float64).sum())]
            eng.set_relation_negatives(2)
            out["minibatch_relation_rows_2"] = dict(kernel_rows(eng, step, reps), rows=N, positives=BATCH)
            eng.set_relation_negatives(0)
            eng.set_overlap(True)
            ms, count = [], 1000
            for temperature in (0.0, ALPHA) * 3:
                eng.set_adversarial_negatives(temperature)
                for _ in range(3):
                    count += 1
                    step(count)
                eng.sync()
                eng.timer_start()
                for _ in range(steps):
                    count += 1
                    step(count)
                ms.append({"temperature": temperature, "ms": eng.timer_stop() / steps})
            out["train_step"] = {"steps": steps, "ms_per_step": ms, "loss_at_end": eng.loss(),
                                 "off_ms": [r["ms"] for r in ms if r["temperature"] == 0],
                                 "on_ms": [r["ms"] for r in ms if r["temperature"] > 0]}
        finally:
            eng.set_adversarial_negatives(0.0)
            for b in (bd, xd, yd):
                b.free()
    return out


def embedding_context(train, rng, reps):
    n = len(train)
    N = n * (RATE + 1)
    with _native.Engine(V, R, D, 0, "embedding", 1) as eng:
        eng.set_params({"W_emb": (rng.randn(V, D) * 0.1).astype(np.float32), "b_emb": np.zeros(D, np.float32),
                        "W_relation": (rng.randn(V, D) * 0.1).astype(np.float32)})
        eng.decoder_reserve(N)
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        bd, xd, yd = eng.to_device(train), eng.alloc(12 * N), eng.alloc(4 * N)

        def step(i):
            eng.negative_sample_device(bd, n, RATE, 300 + i, xd, yd)
            eng.train_step_device(None, 0, xd, yd, N, seed=i, reg_param=0.01)
        try:
            eng.set_overlap(False)
            eng.set_adversarial_negatives(ALPHA, n)
            out = dict(kernel_rows(eng, step, reps), rows=N, positives=n)
            out["loss_at_end"] = eng.loss()
        finally:
            for b in (bd, xd, yd):
                b.free()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rng = np.random.RandomState(0)
    train = np.ascontiguousarray(oracle.synthetic_graph(V, R, TRAIN, rng), dtype=np.int32)
    out = {"V": V, "R": R, "d": D, "blocks": NB, "layers": L, "triples": len(train), "reps": reps, "temperature": ALPHA}
    out.update(block_context(train, rng, reps, steps))
    out["embedding"] = embedding_context(train, rng, reps)
    print(json.dumps(out, indent=1))
    for name in ("minibatch", "minibatch_relation_rows_2", "embedding"):
        s = out[name]
        print("%s (%d rows, %d positives): adv_weights %.1f us, dec_energy_rel %.1f us in the same steps, ratio %.2f"
              % (name, s["rows"], s["positives"], s["adv_weights_us"], s["dec_energy_rel_us"], s["ratio"]))
    t = out["train_step"]
    print("train step, ms: off " + ", ".join("%.4f" % v for v in t["off_ms"]) + "; on " +
          ", ".join("%.4f" % v for v in t["on_ms"]))


if __name__ == "__main__":
    main()
