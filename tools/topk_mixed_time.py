"""Kernel times of the ensemble top-k (rgcn_topk_mixed_device) at FB15k-237 size:

    python tools/topk_mixed_time.py [queries] [reps]

Two `Name=embedding` engines over V = 14,541 entities, d = 500, with different parameter sets; `queries` (2,048)
object-side queries, the real FB15k-237 valid + test triples of tests/golden/graphs.npz with their known objects as
exclusion / filter lists.  The partner engine scores the queries once (rgcn_score_queries_device) and its buffer is read
in place.  For k = 10 and k = 1024, `reps` calls each after two warm-ups, profile on, side streams off (durations are
exclusive), all in one run and on one context:

    rgcn_topk_device         rank_scores (the GEMM), topk_rows
    rgcn_rank_mixed_device   rank_scores, rank_rows_mixed
    rgcn_topk_mixed_device   rank_scores, topk_mix_rows (k_mix_rows), topk_rows_mixed (k_topk_rows on the mixed scores)

By construction topk_mix_rows should cost about what rank_rows_mixed costs (the same two double-precision exponentials per
entity, plus one write) and topk_rows_mixed what topk_rows costs (the same kernel on other floats); the last lines print
the two ratios."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from relationprediction_amd import _native  # noqa: E402

V, R, D = 14541, 237, 500
KS = (10, 1024)
SCOPES = ("rank_scores", "topk_rows", "rank_rows_mixed", "topk_mix_rows", "topk_rows_mixed")


def embedding_params(rng):
    return {"W_emb": (rng.randn(V, D) * 3 / np.sqrt(V + D)).astype(np.float32), "b_emb": np.zeros(D, np.float32),
            "W_relation": rng.randn(V, D).astype(np.float32)}


def measure(n, reps):
    with np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz")) as z:
        pool = z["fb237_valid_test"].astype(np.int32)
    rng = np.random.RandomState(1)
    known = {}
    for s, r, o in pool:
        lst = known.setdefault((int(s), int(r)), [])
        if int(o) not in lst:
            lst.append(int(o))
    queries = np.ascontiguousarray(pool[rng.choice(len(pool), n, replace=False)])
    lists = [known[(int(s), int(r))] for s, r, o in queries]
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.concatenate([np.asarray(x, np.int32) for x in lists])
    out = {"queries": n, "V": V, "d": D, "reps": reps, "weight": 0.5}
    with _native.Engine(V, R, D, 0, "embedding", 1) as other, _native.Engine(V, R, D, 0, "embedding", 1) as eng:
        other.set_params(embedding_params(rng))
        other.forward(train=False)
        other.rank_reserve(n)
        other.score_queries(queries, True)                       # synchronises: the buffer is complete from here on
        partner = other.rank_energies_device()
        eng.set_params(embedding_params(rng))
        eng.forward(train=False)
        eng.rank_reserve(n)
        eng.set_overlap(False)
        for k in KS:
            calls = {"topk": lambda: eng.topk(queries, True, k, ptr, idx),
                     "rank_mixed": lambda: eng.ranks_mixed(queries, True, partner, 0.5, ptr, idx),
                     "topk_mixed": lambda: eng.topk_mixed(queries, True, k, partner, 0.5, ptr, idx)}
            out["k=%d" % k] = {}
            for name, call in calls.items():
                for _ in range(2):
                    call()
                eng.profile_enable(True)
                eng.profile_reset()
                for _ in range(reps):
                    call()
                rows = {p["name"]: p for p in eng.profile()}
                eng.profile_enable(False)
                out["k=%d" % k][name] = {s: {"us_per_call": 1e3 * v["total_ms"] / v["calls"],
                                             "design_bytes": v["alg_bytes"] / v["calls"],
                                             "compulsory_bytes": v["compulsory_bytes"] / v["calls"],
                                             "GB_per_s": v["compulsory_bytes"] / v["calls"] / (1e6 * v["total_ms"] / v["calls"])}
                                         for s, v in rows.items() if s in SCOPES}
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    out = measure(n, reps)
    print(json.dumps(out, indent=1))
    for k in KS:
        t = out["k=%d" % k]
        us = lambda call, scope: t[call][scope]["us_per_call"]
        print("k = %d, %d queries: rank_scores %.1f us | topk_rows %.1f us, topk_rows_mixed %.1f us (ratio %.2f) | "
              "rank_rows_mixed %.1f us, topk_mix_rows %.1f us (ratio %.2f)"
              % (k, n, us("topk_mixed", "rank_scores"), us("topk", "topk_rows"), us("topk_mixed", "topk_rows_mixed"),
                 us("topk_mixed", "topk_rows_mixed") / us("topk", "topk_rows"), us("rank_mixed", "rank_rows_mixed"),
                 us("topk_mixed", "topk_mix_rows"), us("topk_mixed", "topk_mix_rows") / us("rank_mixed", "rank_rows_mixed")))


if __name__ == "__main__":
    main()
