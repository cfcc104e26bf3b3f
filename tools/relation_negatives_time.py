"""The relation corruptions next to the entity sampler, and the train step with the mode off and on, in one run on one
context:

    python tools/relation_negatives_time.py [reps] [steps]

One FB15k-237 gcn_block context (V = 14,541, R = 237, d = 500, 100 blocks, L = 2).  K, the known positives, is the training
set: the real one when data/FB-Toutanova lies beside the package, otherwise 272,115 synthetic triples with
oracle.synthetic_graph's skewed relation and entity frequencies (the output says which).  Everything is at the FB15k-237
minibatch: n = 30,000 batch triples, rate 10, and m = 1 and m = 2 relation rows per positive.

1. `negative_sample_relation`, plain and exclusive, beside `negative_sample` / `negative_sample_exclusive` of the same
   calls (rgcn_profile_*: HIP events around each launch, side streams off): `reps` (default 20) calls of the plain form,
   then as many of the exclusive form, after two warm-ups of each, microseconds per launch.  The device's last output is checked against the numpy mirror
   (tests/relation_negatives_reference.py), which also says how many relation rows had a known first draw.
2. The fb237 block train step (rgcn_train_step_minibatch_device: 30,000 batch edges, 15,000 kept, rate 10, clip + Adam,
   plain sampler) with the mode off, m = 1 and m = 2, the round repeated: milliseconds per step from HIP events around
   `steps` (default 30) consecutive steps after three warm-ups.  With the mode on the decoder batch is not the tiled one
   and decoder_prepare takes its general path; N grows by m / 11.  The control is the mode-off step at rate 10 + m: the
   same N, all rows entity corruptions, the batch tiled -- what the extra rows alone cost.  The ratio to the mode-off
   step, the share of the increase the rows alone explain and the remainder (the untiled layout) are printed."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import exclusive_negatives_reference as ent  # noqa: E402
import relation_negatives_reference as ref  # noqa: E402
import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, NB, L, TRAIN, BATCH, KEEP, RATE = 14541, 237, 500, 100, 2, 272115, 30000, 15000, 10
RELATION_RATES = (1, 2)


def training_set(rng):
    path = os.path.join(ROOT, "data", "FB-Toutanova")
    if os.path.exists(os.path.join(path, "train.txt")):
        from relationprediction_amd import train as train_module
        splits, entities, relations = train_module.load_dataset(path)
        if len(entities) == V and len(relations) == R:
            return np.ascontiguousarray(splits["train"], dtype=np.int32), "data/FB-Toutanova/train.txt"
    return np.ascontiguousarray(oracle.synthetic_graph(V, R, TRAIN, rng), dtype=np.int32), "synthetic"


def sampler_rows(eng, keys, batch, m, reps, seed):
    n = len(batch)
    total = n * (RATE + 1 + m)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * total), eng.alloc(4 * total)
    out = {"n": n, "rate": RATE, "relation_rate": m, "rows": total, "relation_rows": n * m}
    try:
        for exclusive in (False, True, False, True):
            eng.negative_sample_device(bd, n, RATE, seed, xd, yd, exclusive=exclusive, relation_rate=m)
        eng.sync()
        before = eng.negative_relation_unresolved()
        for exclusive in (False, True):
            eng.profile_enable(True)
            eng.profile_reset()
            for i in range(reps):
                eng.negative_sample_device(bd, n, RATE, seed + i, xd, yd, exclusive=exclusive, relation_rate=m)
            rows = {p["name"]: p for p in eng.profile()}
            eng.profile_enable(False)
            form = "exclusive" if exclusive else "plain"
            entity = "negative_sample_exclusive" if exclusive else "negative_sample"
            out["negative_sample_relation_%s_us" % form] = (1e3 * rows["negative_sample_relation"]["total_ms"] /
                                                            rows["negative_sample_relation"]["calls"])
            out["%s_us" % entity] = 1e3 * rows[entity]["total_ms"] / rows[entity]["calls"]
            want = ref.sample(keys, batch, RATE, m, V, R, seed + reps - 1, exclusive)
            out["device_equals_mirror_%s" % form] = bool(np.array_equal(xd.download(np.int32, (total, 3)), want["X"]))
            if exclusive:
                rel = want["relation"]
                out["share_first_draw_known"] = float(rel["first_known"].mean())
                out["largest_lookups_of_a_row"] = int(rel["lookups"].max())
                out["rows_scanned"] = int(rel["scanned"].sum())
                out["rows_unresolved"] = int(rel["unresolved"])
        out["device_unresolved_per_launch"] = (eng.negative_relation_unresolved() - before) / float(reps)
    finally:
        for b in (bd, xd, yd):
            b.free()
    return out


def train_steps(eng, train, steps):
    rng = np.random.RandomState(3)
    batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
    N = BATCH * (RATE + 1 + max(RELATION_RATES))
    eng.decoder_reserve(N)
    eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
    out = {"batch_edges": BATCH, "kept": KEEP, "steps": steps, "ms_per_step": []}
    # (rate, m): the mode off, the mode on, and the control -- as many rows as the mode-on step, all of them entity
    # corruptions, so that the batch stays tiled: what the extra rows alone cost
    configs = [(RATE, 0)] + [(RATE, m) for m in RELATION_RATES] + [(RATE + m, 0) for m in RELATION_RATES]
    try:
        count = 0
        for rate, m in configs + configs:
            eng.set_relation_negatives(m)
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
            out["ms_per_step"].append({"rate": rate, "relation_rate": m, "decoder_triples": BATCH * (rate + 1 + m),
                                       "ms": eng.timer_stop() / steps})
        out["loss_at_end"] = eng.loss()
    finally:
        eng.set_relation_negatives(0)
        for b in (bd, xd, yd):
            b.free()

    def best(rate, m):
        return min(r["ms"] for r in out["ms_per_step"] if r["rate"] == rate and r["relation_rate"] == m)
    off = best(RATE, 0)
    out["summary"] = []
    for m in RELATION_RATES:
        on, tiled = best(RATE, m), best(RATE + m, 0)
        out["summary"].append({"relation_rate": m, "off_ms": off, "on_ms": on, "ratio": on / off,
                               "growth_of_N": m / float(RATE + 1), "tiled_at_the_same_N_ms": tiled,
                               "share_of_the_increase_from_the_rows_alone": (tiled - off) / (on - off) if on > off else None,
                               "untiled_layout_ms": on - tiled})
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rng = np.random.RandomState(0)
    train, source = training_set(rng)
    keys = ent.build_index(train, V, R)
    out = {"V": V, "R": R, "d": D, "blocks": NB, "layers": L, "known_positives": source, "triples": len(train),
           "keys": len(keys), "reps": reps}
    eng = _native.Engine(V, R, D, L, "block", NB, max_edges=BATCH)
    try:
        eng.set_params(oracle.init_params(V, R, D, L, "block", NB, rng=rng))
        eng.known_positives_reserve(train)
        eng.set_overlap(False)
        batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
        out["sampler"] = [sampler_rows(eng, keys, batch, m, reps, 1000 * m) for m in RELATION_RATES]
        eng.set_overlap(True)
        out["train_step"] = train_steps(eng, train, steps)
    finally:
        eng.close()
    print(json.dumps(out, indent=1))
    for s in out["sampler"]:
        print("m %d (%d relation rows): negative_sample_relation plain %6.1f us, exclusive %6.1f us; beside them negative_sample "
              "%6.1f us, negative_sample_exclusive %6.1f us; first draw known in %.3f %% of the relation rows, at most %d "
              "lookups, %d rows scanned, %d unresolved; device == mirror: %s / %s"
              % (s["relation_rate"], s["relation_rows"], s["negative_sample_relation_plain_us"],
                 s["negative_sample_relation_exclusive_us"], s["negative_sample_us"], s["negative_sample_exclusive_us"],
                 100 * s["share_first_draw_known"], s["largest_lookups_of_a_row"], s["rows_scanned"], s["rows_unresolved"],
                 s["device_equals_mirror_plain"], s["device_equals_mirror_exclusive"]))
    print("train step, ms: " + ", ".join("rate %d m %d %.4f" % (r["rate"], r["relation_rate"], r["ms"])
                                         for r in out["train_step"]["ms_per_step"]))
    for s in out["train_step"]["summary"]:
        print("m %d: %.4f ms against %.4f ms off, ratio %.3f (N grows by %.3f); rate %d with the mode off, the same N tiled: "
              "%.4f ms; the untiled layout costs %.4f ms"
              % (s["relation_rate"], s["on_ms"], s["off_ms"], s["ratio"], s["growth_of_N"], RATE + s["relation_rate"],
                 s["tiled_at_the_same_N_ms"], s["untiled_layout_ms"]))


if __name__ == "__main__":
    main()
