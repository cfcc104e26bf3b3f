"""The exclusive negative sampler next to the plain one, and the train step with the mode off and on, in one run on one
context:

    python tools/exclusive_negatives_time.py [reps] [steps]

One FB15k-237 gcn_block context (V = 14,541, R = 237, d = 500, 100 blocks, L = 2).  K, the known positives, is the training
set: the real one when data/FB-Toutanova lies beside the package, otherwise 272,115 synthetic triples with
oracle.synthetic_graph's skewed relation and entity frequencies (the output says which).

1. `negative_sample` and `negative_sample_exclusive` (rgcn_profile_*: HIP events around each launch, side streams off), rate
   10, alternating `reps` (default 20) launches of each after two warm-ups, at the minibatch size (n = 30,000 training
   triples) and at the DistMult size (n = 272,115, the whole training set): microseconds per launch.
2. For both sizes, from the numpy mirror (tests/exclusive_negatives_reference.py), whose rows the device's are checked
   against: the share of negative rows whose attempt 0 was known, the largest number of lookups a row made, the rows that
   reached the scan, the unresolved rows.
3. The fb237 block train step (rgcn_train_step_minibatch_device: 30,000 batch edges, 15,000 kept, rate 10, clip + Adam)
   with the mode off and on, alternating, twice each: milliseconds per step from HIP events around `steps` (default 30)
   consecutive steps after three warm-ups."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import exclusive_negatives_reference as ref  # noqa: E402
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


def sampler_rows(eng, keys, batch, reps, seed):
    n = len(batch)
    total = n * (RATE + 1)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * total), eng.alloc(4 * total)
    out = {"n": n, "rate": RATE, "rows": total}
    try:
        for exclusive in (False, True, False, True):
            eng.negative_sample_device(bd, n, RATE, seed, xd, yd, exclusive=exclusive)
        eng.sync()
        before = eng.negative_unresolved()
        eng.profile_enable(True)
        eng.profile_reset()
        for i in range(reps):
            for exclusive in (False, True):
                eng.negative_sample_device(bd, n, RATE, seed + i, xd, yd, exclusive=exclusive)
        rows = {p["name"]: p for p in eng.profile()}
        eng.profile_enable(False)
        for name in ("negative_sample", "negative_sample_exclusive"):
            out[name + "_us"] = 1e3 * rows[name]["total_ms"] / rows[name]["calls"]
        out["extra_us"] = out["negative_sample_exclusive_us"] - out["negative_sample_us"]
        # what the draws looked like, from the mirror -- and the device's last output against it
        m = ref.exclusive(keys, batch, RATE, V, R, seed + reps - 1)
        out["device_equals_mirror"] = bool(np.array_equal(xd.download(np.int32, (total, 3)), m["X"]))
        out["share_first_draw_known"] = float(m["first_known"].mean())
        out["largest_lookups_of_a_row"] = int(m["lookups"].max())
        out["rows_scanned"] = int(m["scanned"].sum())
        out["rows_unresolved"] = int(m["unresolved"])
        out["device_unresolved_per_launch"] = (eng.negative_unresolved() - before) / float(reps)
    finally:
        for b in (bd, xd, yd):
            b.free()
    return out


def train_steps(eng, train, steps):
    rng = np.random.RandomState(3)
    batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
    N = BATCH * (RATE + 1)
    eng.decoder_reserve(N)
    eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
    out = {"batch_edges": BATCH, "kept": KEEP, "decoder_triples": N, "steps": steps, "ms_per_step": []}
    try:
        count = 0
        for mode in (False, True, False, True):
            eng.set_exclusive_negatives(mode)
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
            out["ms_per_step"].append({"exclusive": mode, "ms": eng.timer_stop() / steps})
        out["loss_at_end"] = eng.loss()
    finally:
        eng.set_exclusive_negatives(False)
        for b in (bd, xd, yd):
            b.free()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rng = np.random.RandomState(0)
    train, source = training_set(rng)
    keys = ref.build_index(train, V, R)
    out = {"V": V, "R": R, "d": D, "blocks": NB, "layers": L, "known_positives": source, "triples": len(train),
           "keys": len(keys), "index_MB": keys.nbytes / 1e6, "probes_per_lookup": int(np.ceil(np.log2(len(keys)))), "reps": reps}
    eng = _native.Engine(V, R, D, L, "block", NB, max_edges=BATCH)
    try:
        eng.set_params(oracle.init_params(V, R, D, L, "block", NB, rng=rng))
        eng.known_positives_reserve(train)
        eng.set_overlap(False)
        out["minibatch"] = sampler_rows(eng, keys, np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]]), reps, 1000)
        out["distmult"] = sampler_rows(eng, keys, train, reps, 2000)
        eng.set_overlap(True)
        out["train_step"] = train_steps(eng, train, steps)
    finally:
        eng.close()
    print(json.dumps(out, indent=1))
    for name in ("minibatch", "distmult"):
        s = out[name]
        print("%-9s n %7d: negative_sample %6.1f us, negative_sample_exclusive %6.1f us (+%.1f); first draw known in "
              "%.3f %% of the rows, at most %d lookups, %d rows scanned, %d unresolved; device == mirror: %s"
              % (name, s["n"], s["negative_sample_us"], s["negative_sample_exclusive_us"], s["extra_us"],
                 100 * s["share_first_draw_known"], s["largest_lookups_of_a_row"], s["rows_scanned"], s["rows_unresolved"],
                 s["device_equals_mirror"]))
    print("train step, ms: " + ", ".join("%s %.4f" % ("on" if r["exclusive"] else "off", r["ms"])
                                         for r in out["train_step"]["ms_per_step"]))


if __name__ == "__main__":
    main()
