"""Encoder-step time with and without the output transform (UseOutputTransform=Yes, rgcn_config_ext::code_dim), and what
the code width does to the evaluation, from HIP events and the engine's own profile records:

    python tools/output_transform_time.py [reps] [queries]

FB15k-237 minibatch shape: V = 14,541, R = 237, d = 500, E = 15,000 (a seeded synthetic graph with its skew), L = 2,
basis kind, B = 2, train mode.  Three contexts in ONE process -- no output layer, c = 500, c = 200:
  * `rgcn_step_device` (graph preparation + forward + backward), HIP events around `reps` consecutive calls after 5
    warm-up calls (the stop event is synchronised inside the window), in milliseconds per step.  The yardstick is the step
    without the layer in the same run: such a context launches exactly what it launched before the feature existed;
  * the profile rows of what the layer adds -- `gemm_out_fwd`, `out_bias`, `gemm_out_dh`, `gemm_out_dw` and the column
    sums (`bias_grad_colsum`: b_emb's on every context, b_out's on top of them with the layer) -- in microseconds per
    step, beside the layer stack's own self-loop GEMMs;
  * `rank_query`, the `rank_scores` GEMM and `topk_rows` (k = 10) for `queries` (default 2,048) object-side queries on a
    test-mode forward of the same graph, microseconds per call: the GEMM is [queries, V] x c.
No ratio is fixed in advance.  The expectation to compare against: the step grows by three V x d x c products and two
[V,c] passes; `rank_scores` shrinks about in proportion to c.  All three launches of the layer's backward pass are on the
main stream: if `gemm_out_dw` is a visible share of the step, moving it to a side stream is the follow-up.  Prints one
JSON object and a summary line per configuration."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, L, E, B = 14541, 237, 500, 2, 15000, 2
CODE_DIMS = (None, 500, 200)
STEP_ROWS = ("gemm_out_fwd", "out_bias", "gemm_out_dh", "gemm_out_dw", "bias_grad_colsum", "gemm_self_fwd", "gemm_self_dh",
             "gemm_self_dw", "gemm_basis_fwd", "gemm_basis_dw", "gemm_basis_dz")
QUERY_ROWS = ("rank_query", "rank_scores", "topk_rows")


def measure(code_dim, graph, reps, queries, warmup=5):
    """(ms per rgcn_step_device, {step row: us per step}, {query row: us per call})"""
    rng = np.random.default_rng(1)
    eng = _native.Engine(V, R, D, L, "basis", B, keep_prob=0.8, max_edges=len(graph), code_dim=code_dim)
    try:
        params = {}
        for name, shape in zip(eng.param_names, eng.param_shapes):
            params[name] = np.zeros(shape, np.float32) if name.startswith("b") else \
                (rng.standard_normal(shape) * 0.05).astype(np.float32)
        eng.set_params(params)
        gd = eng.to_device(graph)
        dd = eng.to_device((rng.standard_normal((V, eng.dc)) * 0.01).astype(np.float32))
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
        step_rows = {p["name"]: round(1e3 * p["total_ms"] / reps, 2) for p in eng.profile() if p["name"] in STEP_ROWS}
        eng.profile_enable(False)
        # the evaluation at this code width: object-side top-10 of `queries` triples of the graph
        eng.set_graph(graph)
        eng.forward(train=False)
        eng.rank_reserve(queries)
        q = np.ascontiguousarray(graph[np.random.RandomState(2).choice(len(graph), queries, replace=queries > len(graph))])
        for _ in range(2):
            eng.topk(q, True, 10)
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(reps):
            eng.topk(q, True, 10)
        query_rows = {p["name"]: round(1e3 * p["total_ms"] / max(p["calls"], 1), 2) for p in eng.profile()
                      if p["name"] in QUERY_ROWS}
        eng.profile_enable(False)
        gd.free(); dd.free()
    finally:
        eng.close()
    return round(ms, 4), step_rows, query_rows


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    queries = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    rng = np.random.RandomState(0)
    full = oracle.synthetic_graph(V, R, 272115, rng).astype(np.int32)
    graph = np.ascontiguousarray(full[rng.choice(len(full), E, replace=False)])
    out = {"reps": reps, "queries": queries, "shape": {"V": V, "R": R, "d": D, "L": L, "E": E, "kind": "basis", "B": B}}
    for c in CODE_DIMS:
        ms, step_rows, query_rows = measure(c, graph, reps, queries)
        out["none" if c is None else "c%d" % c] = {"step_ms": ms, "step_rows_us": step_rows, "query_rows_us": query_rows}
    print(json.dumps(out, indent=1))
    base = out["none"]
    for c in CODE_DIMS:
        r = out["none" if c is None else "c%d" % c]
        added = sum(v for k, v in r["step_rows_us"].items() if "out" in k) + \
            r["step_rows_us"].get("bias_grad_colsum", 0.0) - base["step_rows_us"].get("bias_grad_colsum", 0.0)
        print("code_dim %s: step %.3f ms (x %.2f of the step without the layer); the layer's kernels %.1f us per step "
              "(exclusive times), gemm_out_dw %.1f us = %.1f %% of the step; rank_scores %.1f us, topk_rows %.1f us per %d "
              "queries" % (c, r["step_ms"], r["step_ms"] / base["step_ms"], added, r["step_rows_us"].get("gemm_out_dw", 0.0),
                           0.1 * r["step_rows_us"].get("gemm_out_dw", 0.0) / r["step_ms"],
                           r["query_rows_us"].get("rank_scores", 0.0), r["query_rows_us"].get("topk_rows", 0.0), queries))


if __name__ == "__main__":
    main()
