"""Kernel times of the three optimizer algorithms in one run:

    python tools/optimizer_time.py [reps]

One context with the parameters of the FB15k-237 gcn_block configuration (V = 14,541, R = 237, d = 500, 100 blocks, L = 2:
about 10 million trainable elements).  One small train step leaves real gradients; then, per algorithm, three warm-up
optimizer steps (the first creates the state) and `reps` (default 20) profiled ones (rgcn_profile_*: HIP events around each
launch, side streams off).  Printed: microseconds per launch of `opt_adam`, `opt_adagrad` and `opt_sgd`, the bytes each
declares (28, 20 and 12 per element), the rate that makes, and each time as a fraction of `opt_adam`'s next to the fraction
the bytes predict (20/28 = 0.71, 12/28 = 0.43) -- with `opt_grad_norm` and `opt_clip_scale`, which all three share."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, NB, L, E = 14541, 237, 500, 100, 2, 2000
SCOPES = {"Adam": "opt_adam", "AdaGrad": "opt_adagrad", "GradientDescent": "opt_sgd"}
RATES = {"Adam": 0.01, "AdaGrad": 0.1, "GradientDescent": 0.5}
BYTES_PER_ELEMENT = {"Adam": 28, "AdaGrad": 20, "GradientDescent": 12}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rng = np.random.RandomState(0)
    params = oracle.init_params(V, R, D, L, "block", NB, rng=rng)
    triples = np.ascontiguousarray(oracle.synthetic_graph(V, R, E, rng), dtype=np.int32)
    X = np.concatenate([triples, np.stack([rng.randint(0, V, E), triples[:, 1], triples[:, 2]], 1)]).astype(np.int32)
    Y = np.concatenate([np.ones(E), np.zeros(E)]).astype(np.float32)
    out = {"V": V, "R": R, "d": D, "blocks": NB, "layers": L, "reps": reps, "algorithms": {}}
    eng = _native.Engine(V, R, D, L, "block", NB, max_edges=E)
    try:
        eng.set_params(params)
        eng.decoder_reserve(len(X))
        td, xd, yd = eng.to_device(triples), eng.to_device(X), eng.to_device(Y)
        eng.train_step_device(td, E, xd, yd, len(X), seed=1, reg_param=0.01)      # (no optimizer yet: gradients only)
        eng.sync()
        eng.set_overlap(False)
        for algorithm, scope in SCOPES.items():
            eng.optimizer_config(lr=RATES[algorithm], max_grad_norm=1.0, algorithm=algorithm)
            for _ in range(3):
                eng.optimizer_step()
            eng.sync()
            eng.profile_enable(True)
            eng.profile_reset()
            for _ in range(reps):
                eng.optimizer_step()
            rows = {p["name"]: p for p in eng.profile()}
            eng.profile_enable(False)
            row = rows[scope]
            us = 1e3 * row["total_ms"] / row["calls"]
            out["algorithms"][algorithm] = {
                "scope": scope, "calls": row["calls"], "us_per_launch": us,
                "elements": row["alg_bytes"] / row["calls"] / BYTES_PER_ELEMENT[algorithm],
                "design_MB": row["alg_bytes"] / row["calls"] / 1e6,
                "GB_per_s": row["alg_bytes"] / row["calls"] / (us * 1e3),
                "opt_grad_norm_us": 1e3 * rows["opt_grad_norm"]["total_ms"] / rows["opt_grad_norm"]["calls"],
                "opt_clip_scale_us": 1e3 * rows["opt_clip_scale"]["total_ms"] / rows["opt_clip_scale"]["calls"]}
        for b in (td, xd, yd):
            b.free()
    finally:
        eng.close()
    print(json.dumps(out, indent=1))
    adam = out["algorithms"]["Adam"]["us_per_launch"]
    for algorithm, a in out["algorithms"].items():
        print("%-12s %8.1f us  %7.1f MB  %7.0f GB/s  %.2f of opt_adam (by bytes: %.2f)"
              % (a["scope"], a["us_per_launch"], a["design_MB"], a["GB_per_s"], a["us_per_launch"] / adam,
                 BYTES_PER_ELEMENT[algorithm] / 28.0))


if __name__ == "__main__":
    main()
