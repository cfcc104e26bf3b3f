"""Time of one train step at FB15k-237 minibatch size, basis kind, B = 5, in both input modes on the same batch:

    python tools/featureless_time.py [steps] [warmup]

V = 14,541, R = 237, d = 500, L = 2; the message graph is 15,000 edges of a seeded synthetic graph with FB15k-237's
skew (GraphBatchSize 30,000 x GraphSplitSize 0.5), the decoder batch its 30,000-edge batch with 10 corruptions each,
drawn on the device.  `rgcn_train_step_device` (graph preparation, encoder, DistMult loss, backward, clip + Adam) is
timed with HIP events around `steps` consecutive calls after `warmup` calls, once with the embedding input
(input_mode="embedding": W_emb under two dense layers) and once featureless (input_mode="onehot": layer 1 reads the
[V,B,d] tables of csrc/basis_onehot.hip).  A second pass of 3 steps with the per-kernel profile on lists where the
featureless step's time goes.  Prints one JSON object and a summary line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402


def seeded_params(eng, rng):
    out = {}
    for name, shape in zip(eng.param_names, eng.param_shapes):
        if name.startswith("b"):
            out[name] = np.zeros(shape, np.float32)
        elif name.startswith("C_") or name == "W_relation":
            out[name] = rng.standard_normal(shape).astype(np.float32)
        else:
            out[name] = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    return out


def run(mode, batch, graph, steps, warmup, rate=10):
    V, R, d, L, B = 14541, 237, 500, 2, 5
    n = len(batch) * (rate + 1)
    eng = _native.Engine(V, R, d, L, "basis", B, keep_prob=0.8, max_edges=len(graph), input_mode=mode)
    try:
        eng.set_params(seeded_params(eng, np.random.default_rng(1)))
        eng.decoder_reserve(n)
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        gd, bd = eng.to_device(graph), eng.to_device(batch)
        xd, yd = eng.alloc(12 * n), eng.alloc(4 * n)
        eng.negative_sample_device(bd, len(batch), rate, 7, xd, yd)

        def step(i):
            eng.train_step_device(gd, len(graph), xd, yd, n, seed=100 + i, reg_param=0.01)

        for i in range(warmup):
            step(i)
        eng.sync()
        eng.timer_start()
        for i in range(steps):
            step(warmup + i)
        ms = eng.timer_stop() / steps
        loss = eng.loss()
        eng.profile_enable(True)
        eng.profile_reset()
        for i in range(3):
            step(i)
        rows = sorted(eng.profile(), key=lambda p: -p["total_ms"])
        eng.profile_enable(False)
        kernels = [{"name": p["name"], "us_per_step": round(1e3 * p["total_ms"] / 3, 1),
                    "design_MB_per_step": round(p["alg_bytes"] / 3e6, 1),
                    "compulsory_MB_per_step": round(p["compulsory_bytes"] / 3e6, 1)} for p in rows[:8]]
        for b in (gd, bd, xd, yd):
            b.free()
    finally:
        eng.close()
    return {"ms_per_step": round(ms, 4), "loss": loss, "kernels": kernels}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rng = np.random.RandomState(0)
    batch = oracle.synthetic_graph(14541, 237, 30000, rng).astype(np.int32)
    graph = np.ascontiguousarray(batch[rng.choice(len(batch), 15000, replace=False)])
    out = {"steps": steps, "warmup": warmup, "graph_edges": len(graph), "decoder_triples": len(batch) * 11}
    for mode in ("embedding", "onehot"):
        out[mode] = run(mode, batch, graph, steps, warmup)
    out["ratio_onehot_over_embedding"] = round(out["onehot"]["ms_per_step"] / out["embedding"]["ms_per_step"], 3)
    print(json.dumps(out, indent=1))
    print("train step, B = 5: embedding input %.3f ms, one-hot input %.3f ms, ratio %.2f"
          % (out["embedding"]["ms_per_step"], out["onehot"]["ms_per_step"], out["ratio_onehot_over_embedding"]))


if __name__ == "__main__":
    main()
