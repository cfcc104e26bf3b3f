"""Kernel time of the relation queries next to the entity-side calls, same run, same queries, same codes:

    python tools/relation_queries_time.py [queries] [reps]

2,048 queries (default) at FB15k-237 size -- V = 14,541, R = 237, d = 500, codes of a one-layer block encoder on an empty
graph with seeded weights -- drawn from the real FB15k-237 valid + test triples of tests/golden/graphs.npz.  The relation
calls take the relations known between each (subject, object) pair as filter lists and (less the gold relation) as
exclusion lists; the entity-side calls of the same triples take the known objects per (subject, relation) likewise.
Per-kernel durations from rgcn_profile_get (HIP events around every launch), `reps` calls each after two warm-up calls:
rank_query_relation (the pair-query kernel), rank_scores_relation (the GEMM against W_relation), rank_rows_relation and
topk_rows_relation at k = 10, and beside them rank_query, rank_scores, rank_rows and topk_rows of the entity side."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from relationprediction_amd import _native  # noqa: E402

SCOPES = ("rank_query", "rank_scores", "rank_rows", "topk_rows",
          "rank_query_relation", "rank_scores_relation", "rank_rows_relation", "topk_rows_relation")


def known_lists(pool, key_columns, value_column):
    known = {}
    for row in pool:
        lst = known.setdefault(tuple(int(row[c]) for c in key_columns), [])
        if int(row[value_column]) not in lst:
            lst.append(int(row[value_column]))
    return known


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return ptr, np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)])


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    V, R, d, nb, k = 14541, 237, 500, 100, 10
    with np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz")) as z:
        pool = z["fb237_valid_test"].astype(np.int32)
    rng = np.random.RandomState(0)
    queries = np.ascontiguousarray(pool[rng.choice(len(pool), n, replace=False)])
    objects, relations = known_lists(pool, (0, 1), 2), known_lists(pool, (0, 2), 1)
    obj_lists = [objects[(int(s), int(r))] for s, r, o in queries]
    rel_lists = [relations[(int(s), int(o))] for s, r, o in queries]
    fptr, fidx = csr(obj_lists)
    eptr, eidx = csr([[e for e in x if e != int(o)] for x, (s, r, o) in zip(obj_lists, queries)])
    rfptr, rfidx = csr(rel_lists)
    reptr, reidx = csr([[e for e in x if e != int(r)] for x, (s, r, o) in zip(rel_lists, queries)])

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
             "topk": lambda: eng.topk(queries, True, k, eptr, eidx),
             "rank_relation": lambda: eng.ranks_relation(queries, rfptr, rfidx),
             "topk_relation": lambda: eng.topk_relation(queries, k, reptr, reidx)}
    out = {"queries": n, "V": V, "R": R, "d": d, "k": k, "reps": reps,
           "mean_object_list_length": float(fptr[-1]) / n, "mean_relation_list_length": float(rfptr[-1]) / n}
    for name, call in calls.items():
        for _ in range(2):
            call()
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(reps):
            call()
        rows = {p["name"]: p for p in eng.profile()}
        eng.profile_enable(False)
        out[name] = {key: {"us_per_call": 1e3 * v["total_ms"] / v["calls"],
                           "compulsory_bytes": v["compulsory_bytes"] / v["calls"],
                           "GB_per_s": v["compulsory_bytes"] / v["calls"] / (1e6 * v["total_ms"] / v["calls"])}
                     for key, v in rows.items() if key in SCOPES}
    eng.close()
    print(json.dumps(out, indent=1))

    def us(call, scope):
        return out[call][scope]["us_per_call"]
    print("%d queries: pair query %.1f us (entity query %.1f us) | relation GEMM %.1f us (entity GEMM %.1f us) | "
          "rank_rows_relation %.1f us (rank_rows %.1f us) | topk_rows_relation k = %d %.1f us (topk_rows %.1f us)"
          % (n, us("rank_relation", "rank_query_relation"), us("rank", "rank_query"),
             us("rank_relation", "rank_scores_relation"), us("rank", "rank_scores"),
             us("rank_relation", "rank_rows_relation"), us("rank", "rank_rows"),
             k, us("topk_relation", "topk_rows_relation"), us("topk", "topk_rows")))


if __name__ == "__main__":
    main()
