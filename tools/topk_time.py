"""Kernel time of the top-k selection next to the rank counting, same run, same queries, same energies:

    python tools/topk_time.py [queries] [reps]

2,048 object-side queries (default) at FB15k-237 size -- V = 14,541, d = 500, codes of a one-layer block encoder on an
empty graph with seeded weights -- drawn from the real FB15k-237 valid + test triples of tests/golden/graphs.npz, whose
known objects per (subject, relation) are the filter lists of the rank call and (less the gold object) the exclusion
lists of the top-k calls.  Per-kernel durations from rgcn_profile_get (HIP events around every launch), `reps` calls
each after two warm-up calls: rank_scores (the GEMM before both), rank_rows, topk_rows at k = 10 and k = 1024, with the
bytes per second each achieves on its compulsory bytes."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from relationprediction_amd import _native  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    V, R, d, nb = 14541, 237, 500, 100
    with np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz")) as z:
        pool = z["fb237_valid_test"].astype(np.int32)
    rng = np.random.RandomState(0)
    known = {}
    for s, r, o in pool:
        lst = known.setdefault((int(s), int(r)), [])
        if int(o) not in lst:
            lst.append(int(o))
    queries = np.ascontiguousarray(pool[rng.choice(len(pool), n, replace=False)])
    lists = [known[(int(s), int(r))] for s, r, o in queries]
    fptr = np.zeros(n + 1, np.int64)
    fptr[1:] = np.cumsum([len(x) for x in lists])
    fidx = np.concatenate([np.asarray(x, np.int32) for x in lists])
    ex = [[e for e in x if e != int(o)] for x, (s, r, o) in zip(lists, queries)]
    eptr = np.zeros(n + 1, np.int64)
    eptr[1:] = np.cumsum([len(x) for x in ex])
    eidx = np.concatenate([np.asarray(x, np.int32) for x in ex] + [np.zeros(0, np.int32)])

    eng = _native.Engine(V, R, d, 1, "block", nb, max_edges=1)
    sd = d // nb
    eng.set_params({"W_emb": (rng.randn(V, d) * 0.3).astype(np.float32), "b_emb": np.zeros(d, np.float32),
                    "W_f1": np.zeros((R, nb, sd, sd), np.float32), "W_b1": np.zeros((R, nb, sd, sd), np.float32),
                    "W_self1": (rng.randn(d, d) / np.sqrt(d)).astype(np.float32), "b1": np.zeros(d, np.float32),
                    "W_relation": rng.randn(V, d).astype(np.float32)})
    eng.set_graph(np.zeros((0, 3), np.int32))
    eng.forward(train=False)
    eng.rank_reserve(n)
    eng.set_overlap(False)
    calls = {"rank": lambda: eng.ranks(queries, True, fptr, fidx),
             "topk_k10": lambda: eng.topk(queries, True, 10, eptr, eidx),
             "topk_k1024": lambda: eng.topk(queries, True, 1024, eptr, eidx)}
    out = {"queries": n, "V": V, "d": d, "reps": reps, "mean_list_length": float(fptr[-1]) / n}
    for name, call in calls.items():
        for _ in range(2):
            call()
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(reps):
            call()
        rows = {p["name"]: p for p in eng.profile()}
        eng.profile_enable(False)
        out[name] = {k: {"us_per_call": 1e3 * v["total_ms"] / v["calls"], "compulsory_bytes": v["compulsory_bytes"] / v["calls"],
                         "GB_per_s": v["compulsory_bytes"] / v["calls"] / (1e6 * v["total_ms"] / v["calls"])}
                     for k, v in rows.items() if k in ("rank_query", "rank_scores", "rank_rows", "topk_rows")}
    eng.close()
    print(json.dumps(out, indent=1))
    rr = out["rank"]["rank_rows"]["us_per_call"]
    for name in ("topk_k10", "topk_k1024"):
        t = out[name]["topk_rows"]["us_per_call"]
        print("%s: topk_rows %.1f us, rank_rows %.1f us, ratio %.2f, rank_scores %.1f us"
              % (name, t, rr, t / rr, out[name]["rank_scores"]["us_per_call"]))


if __name__ == "__main__":
    main()
