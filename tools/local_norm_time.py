"""Graph-preparation time and encoder-step time by normalisation mode (IncidenceNormalization), from the engine's own
profile records:

    python tools/local_norm_time.py [reps] [modes]        # modes: comma-separated, default intended,local

V = 14,541, R = 237 (FB15k-237), seeded synthetic graphs with its skew.  Per mode:
  * the graph preparation (`rgcn_set_graph_device`: every `prep_*` record of csrc/graph_prep.hip and csrc/csr_sort.hip) at
    the minibatch (E = 15,000) and at the 272,115-edge training graph, in microseconds per call, per record and in sum;
  * the headline encoder step (`rgcn_step_device`, block kind, d = 500, 100 blocks, L = 2, train mode) at the minibatch,
    HIP events around `reps` consecutive calls after 5 warm-up calls, in milliseconds per step.
`local` counts inside k_build_msgs (two binary searches per message over the sorted incidence keys): it adds no launch,
so its cost shows as the difference of the `prep_build_msgs` records.  Prints one JSON object and a summary line per
mode.  A tree without a mode (an older library) is asked for the modes it has."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, L, NB = 14541, 237, 500, 2, 100


def prep_time(mode, graph, reps):
    """microseconds per rgcn_set_graph_device, by profile record"""
    eng = _native.Engine(V, R, 8, 1, "block", 2, norm_mode=mode, max_edges=len(graph))
    try:
        gd = eng.to_device(graph)
        for _ in range(3):
            eng.set_graph_device(gd, len(graph))
        eng.sync()
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(reps):
            eng.set_graph_device(gd, len(graph))
        eng.sync()
        rows = {p["name"]: 1e3 * p["total_ms"] / reps for p in eng.profile() if p["name"].startswith("prep_")}
        eng.profile_enable(False)
        gd.free()
    finally:
        eng.close()
    out = {k: round(v, 2) for k, v in sorted(rows.items())}
    out["sum"] = round(sum(rows.values()), 2)
    return out


def step_time(mode, graph, reps, warmup=5):
    """milliseconds per rgcn_step_device (graph preparation + forward + backward)"""
    rng = np.random.default_rng(1)
    eng = _native.Engine(V, R, D, L, "block", NB, keep_prob=0.8, norm_mode=mode, max_edges=len(graph))
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
        gd.free(); dd.free()
    finally:
        eng.close()
    return round(ms, 4)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    modes = sys.argv[2].split(",") if len(sys.argv) > 2 else ["intended", "local"]
    rng = np.random.RandomState(0)
    full = oracle.synthetic_graph(V, R, 272115, rng).astype(np.int32)
    mini = np.ascontiguousarray(full[rng.choice(len(full), 15000, replace=False)])
    out = {"reps": reps}
    for mode in modes:
        out[mode] = {"prep_us_E15000": prep_time(mode, mini, reps), "prep_us_E272115": prep_time(mode, full, reps),
                     "step_ms_E15000": step_time(mode, mini, reps)}
    print(json.dumps(out, indent=1))
    for mode in modes:
        m = out[mode]
        print("%s: prep %.1f us (E = 15,000), %.1f us (E = 272,115); encoder step %.3f ms"
              % (mode, m["prep_us_E15000"]["sum"], m["prep_us_E272115"]["sum"], m["step_ms_E15000"]))


if __name__ == "__main__":
    main()
