"""Encoder-step time with and without highway skip connections (SkipConnections=Highway, RGCN_SKIP_HIGHWAY), from HIP
events and the engine's own profile records:

    python tools/highway_time.py [reps]

FB15k-237 minibatch shape: V = 14,541, R = 237, d = 500, E = 15,000 (a seeded synthetic graph with its skew), L = 2,
train mode.  Block kind (100 blocks) and basis kind (B = 2), each with skip none and with highway, in ONE process:
  * `rgcn_step_device` (graph preparation + forward + backward), HIP events around `reps` consecutive calls after 5
    warm-up calls, in milliseconds per step.  The yardstick is the skip-none step of the same run: a context without
    highway launches exactly what it launched before the feature existed;
  * the profile rows of what highway adds -- `highway_fwd`, `highway_bwd`, `highway_join`, `gemm_highway_fwd`,
    `gemm_highway_dh`, `gemm_highway_dw` -- in microseconds per step, beside the layer's own three self-loop GEMMs.
No ratio is fixed in advance.  The expectation to compare against: three more d x d GEMMs per layer beside the three the
layer has, plus about ten [V,d] passes (forward 5, backward 8 + 5 per layer at 4 V d bytes each).  Prints one JSON object
and a summary line per configuration."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, L, E = 14541, 237, 500, 2, 15000
CONFIGS = [("block", 100), ("basis", 2)]
ROWS = ("highway_fwd", "highway_bwd", "highway_join", "gemm_highway_fwd", "gemm_highway_dh", "gemm_highway_dw",
        "gemm_self_fwd", "gemm_self_dh", "gemm_self_dw", "bias_grad_colsum")


def step_time(kind, nb, skip, graph, reps, warmup=5):
    """(milliseconds per rgcn_step_device, {profile row: microseconds per step})"""
    rng = np.random.default_rng(1)
    eng = _native.Engine(V, R, D, L, kind, nb, keep_prob=0.8, max_edges=len(graph), skip=skip)
    try:
        params = {}
        for name, shape in zip(eng.param_names, eng.param_shapes):
            params[name] = np.zeros(shape, np.float32) if name.startswith("b") else \
                (rng.standard_normal(shape) * 0.05).astype(np.float32)
        eng.set_params(params)
        gd = eng.to_device(graph)
        dd = eng.to_device((rng.standard_normal((V, D)) * 0.01).astype(np.float32))
        for i in range(warmup):
            eng.step_device(gd, len(graph), dd, train=True, seed=i)
        eng.sync()
        eng.timer_start()
        for i in range(reps):
            eng.step_device(gd, len(graph), dd, train=True, seed=warmup + i)
        ms = eng.timer_stop() / reps
        eng.sync()
        eng.profile_enable(True)
        eng.profile_reset()
        for i in range(reps):
            eng.step_device(gd, len(graph), dd, train=True, seed=warmup + reps + i)
        eng.sync()
        rows = {p["name"]: round(1e3 * p["total_ms"] / reps, 2) for p in eng.profile() if p["name"] in ROWS}
        eng.profile_enable(False)
        gd.free(); dd.free()
    finally:
        eng.close()
    return round(ms, 4), rows


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rng = np.random.RandomState(0)
    full = oracle.synthetic_graph(V, R, 272115, rng).astype(np.int32)
    graph = np.ascontiguousarray(full[rng.choice(len(full), E, replace=False)])
    out = {"reps": reps, "shape": {"V": V, "R": R, "d": D, "L": L, "E": E}}
    for kind, nb in CONFIGS:
        for skip in ("none", "highway"):
            ms, rows = step_time(kind, nb, skip, graph, reps)
            out["%s_%s" % (kind, skip)] = {"step_ms": ms, "rows_us_per_step": rows}
    print(json.dumps(out, indent=1))
    for kind, nb in CONFIGS:
        a, b = out[kind + "_none"], out[kind + "_highway"]
        added = sum(v for k, v in b["rows_us_per_step"].items() if "highway" in k)
        print("%s (%d): step %.3f ms without, %.3f ms with highway (x %.2f); highway kernels + GEMMs %.1f us per step "
              "(exclusive times)" % (kind, nb, a["step_ms"], b["step_ms"], b["step_ms"] / a["step_ms"], added))


if __name__ == "__main__":
    main()
