"""Encoder-step time of the basis layer with a per-relation diagonal (AddDiagonal=Yes, RGCN_KIND_BASIS_PDIAG) next to the
basis layer it extends, from HIP events and the engine's own profile records:

    python tools/add_diagonal_time.py [reps]

FB15k-237 minibatch shape: V = 14,541, R = 237, d = 500, E = 15,000 (a seeded synthetic graph with its skew), L = 2,
train mode.  Kind `basis` and kind `basis_pdiag`, each at B = 2 and at B = 5, in ONE process:
  * `rgcn_step_device` (graph preparation + forward + backward), HIP events around `reps` consecutive calls after 5
    warm-up calls, in milliseconds per step.  The yardstick is the basis step of the same run;
  * the per-kernel profile table of a second set of `reps` steps (side streams on, as the step runs them: rows overlap,
    their sum exceeds the step), in microseconds per step with the design bytes and flops each launch site declares.
No ratio is fixed in advance.  The expectation to compare against, from the shapes alone: per layer basis_pdiag does the
basis kind's three products over the (row, direction) units, gathers d floats per message forward (H[src] under one row
of D) and 2 d backward (dD and the diagonal part of dH), and keeps [2][V][B] mixing scalars; what it does NOT do is the
basis kind's B-fold accumulation per message -- its unit rows are the row's own features scaled.  Prints one JSON object
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
CONFIGS = [("basis", 2), ("basis_pdiag", 2), ("basis", 5), ("basis_pdiag", 5)]


def step_time(kind, nb, graph, reps, warmup=5):
    """(milliseconds per rgcn_step_device, [profile rows, microseconds per step])"""
    rng = np.random.default_rng(1)
    eng = _native.Engine(V, R, D, L, kind, nb, keep_prob=0.8, max_edges=len(graph))
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
        rows = [{"name": p["name"], "calls_per_step": round(p["calls"] / reps, 2),
                 "us_per_step": round(1e3 * p["total_ms"] / reps, 2),
                 "design_MB_per_step": round(p["alg_bytes"] / reps / 1e6, 2),
                 "GFLOP_per_step": round(p["alg_flops"] / reps / 1e9, 3)} for p in eng.profile()]
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
        ms, rows = step_time(kind, nb, graph, reps)
        out["%s_B%d" % (kind, nb)] = {"step_ms": ms, "profile": rows}
    print(json.dumps(out, indent=1))
    for nb in sorted({nb for _, nb in CONFIGS}):
        a, b = out["basis_B%d" % nb], out["basis_pdiag_B%d" % nb]
        print("B = %d: step %.3f ms basis, %.3f ms basis_pdiag (x %.2f)" % (nb, a["step_ms"], b["step_ms"],
                                                                          b["step_ms"] / a["step_ms"]))
        for r in b["profile"]:
            if "pdiag" in r["name"]:
                print("    %-22s %9.2f us  %9.2f MB  %8.3f GFLOP" % (r["name"], r["us_per_step"], r["design_MB_per_step"],
                                                                  r["GFLOP_per_step"]))


if __name__ == "__main__":
    main()
