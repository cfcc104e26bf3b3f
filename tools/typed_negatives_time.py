"""The type-constrained sampler next to the plain and the exclusive one, the typed rank and top-k kernels next to their
open twins, and the train step with the mode off and on, in one run on one context:

    python tools/typed_negatives_time.py [reps] [steps]

One FB15k-237 gcn_block context (V = 14,541, R = 237, d = 500, 100 blocks, L = 2).  The training set T is SYNTHETIC and
typed by construction: every relation gets a domain and a range, each a random subset of the entities whose size is
log-uniform between 2 and V (2 (V / 2)^u, u uniform in [0, 1): as many relations with a dozen fillers as with thousands);
a triple draws its relation with probability proportional to 1 / (1 + rank of the relation), its subject uniformly from
the relation's domain and its object uniformly from its range, until 272,115 distinct triples exist.  T is both the type
sets' and the known positives' triples.

1. The four sampler kernels (`negative_sample`, `negative_sample_exclusive`, `negative_sample_typed` plain and exclusive;
   rgcn_profile_*: HIP events around each launch, side streams off) at the FB15k-237 minibatch (n = 30,000, rate 10:
   330,000 rows) and at the DistMult size (n = 272,115, rate 10: 2,993,265 rows): `reps` (default 20) calls each after
   two warm-ups, microseconds per launch, and the share of open rows the device counted.  About 2,000 evenly spaced
   negative rows of the device's last typed outputs are checked against the mirror (tests/typed_negatives_reference.py).
2. `rank_rows` / `topk_rows` (k = 10) against `rank_rows_typed` / `topk_rows_typed` on 2,048 queries after a test-mode
   forward over T, the object side, filter and exclusion lists = the known objects of each pair, `reps` calls each.
3. The fb237 block train step (rgcn_train_step_minibatch_device: 30,000 batch edges, 15,000 kept, rate 10, clip + Adam)
   with the mode off, on, and on with the exclusive sampler, the round repeated: milliseconds per step from HIP events
   around `steps` (default 30) consecutive steps after three warm-ups."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import typed_negatives_reference as ref  # noqa: E402
import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, NB, L, TRAIN, BATCH, KEEP, RATE = 14541, 237, 500, 100, 2, 272115, 30000, 15000, 10
QUERIES, TOPK = 2048, 10


def typed_training_set(rng):
    sizes = lambda: np.maximum(2, (2 * (V / 2.0) ** rng.random_sample(R)).astype(np.int64))  # noqa: E731
    dom_len, ran_len = sizes(), sizes()
    domains = np.stack([rng.permutation(V) for _ in range(R)])      # row r: its first dom_len[r] entries are domain(r)
    ranges = np.stack([rng.permutation(V) for _ in range(R)])
    p = 1.0 / (1.0 + rng.permutation(R))
    p /= p.sum()
    seen = np.empty(0, dtype=np.int64)
    while seen.size < TRAIN:
        m = 2 * (TRAIN - seen.size) + 1024
        r = rng.choice(R, size=m, p=p)
        s = domains[r, (rng.random_sample(m) * dom_len[r]).astype(np.int64)].astype(np.int64)
        o = ranges[r, (rng.random_sample(m) * ran_len[r]).astype(np.int64)].astype(np.int64)
        seen = np.unique(np.concatenate([seen, (s * R + r) * V + o]))
    seen = seen[rng.permutation(seen.size)[:TRAIN]]
    return np.ascontiguousarray(np.stack([seen // (R * V), (seen // V) % R, seen % V], 1).astype(np.int32))


def sampler_rows(eng, sets, known_set, batch, reps, seed):
    n = len(batch)
    total = n * (RATE + 1)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * total), eng.alloc(4 * total)
    out = {"n": n, "rate": RATE, "rows": total}
    forms = [("negative_sample", False, False), ("negative_sample_exclusive", False, True),
             ("negative_sample_typed", True, False), ("negative_sample_typed", True, True)]

    def call(typed, exclusive, s):
        if typed:
            eng.negative_sample_typed_device(bd, n, RATE, s, xd, yd, exclusive=exclusive)
        else:
            eng.negative_sample_device(bd, n, RATE, s, xd, yd, exclusive=exclusive)
    try:
        for _ in range(2):
            for _, typed, exclusive in forms:
                call(typed, exclusive, seed)
        eng.sync()
        for scope, typed, exclusive in forms:
            opened = eng.negative_typed_open()
            eng.profile_enable(True)
            eng.profile_reset()
            for i in range(reps):
                call(typed, exclusive, seed + i)
            rows = {p["name"]: p for p in eng.profile()}
            eng.profile_enable(False)
            key = scope + ("_exclusive" if typed and exclusive else "")
            out[key + "_us"] = 1e3 * rows[scope]["total_ms"] / rows[scope]["calls"]
            if typed:
                out[key + "_open_share"] = (eng.negative_typed_open() - opened) / float(reps * n * RATE)
                # the mirror walks its rows in Python: every (n rate / 2000)-th negative row of the last call
                got = xd.download(np.int32, (total, 3))
                K = known_set if exclusive else set()
                rows_ok = True
                for j in range(0, n * RATE, max(1, n * RATE // 2000)):
                    s, r, o = batch[j % n].tolist()
                    e, coin, _, _, _ = ref.typed_row(sets, K, exclusive, seed + reps - 1, j, s, r, o)
                    rows_ok = rows_ok and int(got[n + j, 2 if coin else 0]) == e
                out[key + "_equals_mirror_on_sampled_rows"] = bool(rows_ok)
    finally:
        for b in (bd, xd, yd):
            b.free()
    return out


def query_rows(eng, train, reps):
    rng = np.random.RandomState(5)
    queries = np.ascontiguousarray(train[rng.permutation(len(train))[:QUERIES]])
    known = {}
    for s, r, o in train.tolist():
        known.setdefault((s, r), []).append(o)
    out = {"queries": QUERIES, "k": TOPK}
    eng.set_graph(train)
    eng.forward(train=False)
    eng.rank_reserve(QUERIES)
    ptr = np.zeros(QUERIES + 1, dtype=np.int64)
    lists = [known[(int(s), int(r))] for s, r, _ in queries]
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists])
    calls = {"rank_rows": lambda: eng.ranks(queries, True, ptr, flat),
             "rank_rows_typed": lambda: eng.ranks_typed(queries, True, ptr, flat),
             "topk_rows": lambda: eng.topk(queries, True, TOPK, ptr, flat),
             "topk_rows_typed": lambda: eng.topk_typed(queries, True, TOPK, ptr, flat)}
    results = {}
    for _ in range(2):
        for name, call in calls.items():
            results[name] = call()
    for name, call in calls.items():
        eng.profile_enable(True)
        eng.profile_reset()
        for _ in range(reps):
            call()
        rows = {p["name"]: p for p in eng.profile()}
        eng.profile_enable(False)
        out[name + "_us"] = 1e3 * rows[name]["total_ms"] / rows[name]["calls"]
    out["typed_ranks_never_above_open"] = bool((results["rank_rows_typed"][0] <= results["rank_rows"][0]).all())
    out["mean_raw_rank_open"] = float(results["rank_rows"][0].mean())
    out["mean_raw_rank_typed"] = float(results["rank_rows_typed"][0].mean())
    return out


def train_steps(eng, train, steps):
    rng = np.random.RandomState(3)
    batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
    N = BATCH * (RATE + 1)
    eng.decoder_reserve(N)
    eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
    bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
    out = {"batch_edges": BATCH, "kept": KEEP, "steps": steps, "ms_per_step": []}
    configs = [("off", False, False), ("typed", True, False), ("typed + exclusive", True, True)]
    try:
        count = 0
        for name, typed, exclusive in configs + configs:
            eng.set_typed_negatives(typed)
            eng.set_exclusive_negatives(exclusive)
            for _ in range(3):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, RATE, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            eng.sync()
            eng.timer_start()
            for _ in range(steps):
                count += 1
                eng.train_step_minibatch_device(bd, BATCH, KEEP, 100 + count, RATE, 200 + count, xd, yd, seed=count,
                                                reg_param=0.01)
            out["ms_per_step"].append({"mode": name, "ms": eng.timer_stop() / steps})
        out["loss_at_end"] = eng.loss()
    finally:
        eng.set_typed_negatives(False)
        eng.set_exclusive_negatives(False)
        for b in (bd, xd, yd):
            b.free()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rng = np.random.RandomState(0)
    train = typed_training_set(rng)
    sets = ref.build_sets(train, V, R)
    lens = np.diff(sets["ptr"])
    out = {"V": V, "R": R, "d": D, "blocks": NB, "layers": L, "triples": len(train), "reps": reps,
           "list_lengths": {"min": int(lens.min()), "median": float(np.median(lens)), "max": int(lens.max()),
                            "open_lists": int((lens < ref.MIN_CANDIDATES).sum()), "members": int(lens.sum())},
           "set_bytes": int(8 * len(sets["ptr"]) + 4 * len(sets["idx"]) + 4 * sets["mask"].size)}
    eng = _native.Engine(V, R, D, L, "block", NB, max_edges=TRAIN)
    try:
        eng.set_params(oracle.init_params(V, R, D, L, "block", NB, rng=rng))
        eng.type_sets_reserve(train)
        eng.known_positives_reserve(train)
        eng.set_overlap(False)
        batch = np.ascontiguousarray(train[rng.permutation(len(train))[:BATCH]])
        known_set = {tuple(t) for t in train.tolist()}
        out["sampler"] = [sampler_rows(eng, sets, known_set, batch, reps, 1000),
                          sampler_rows(eng, sets, known_set, train, reps, 2000)]
        out["queries"] = query_rows(eng, train, reps)
        eng.set_overlap(True)
        out["train_step"] = train_steps(eng, train, steps)
    finally:
        eng.close()
    print(json.dumps(out, indent=1))
    for s in out["sampler"]:
        print("%9d rows: negative_sample %6.1f us, _exclusive %6.1f us, _typed %6.1f us (open %.4f), _typed exclusive %6.1f us "
              "(open %.4f)" % (s["rows"], s["negative_sample_us"], s["negative_sample_exclusive_us"],
                               s["negative_sample_typed_us"], s["negative_sample_typed_open_share"],
                               s["negative_sample_typed_exclusive_us"], s["negative_sample_typed_exclusive_open_share"]))
    q = out["queries"]
    print("%d queries: rank_rows %6.1f us, rank_rows_typed %6.1f us; topk_rows %6.1f us, topk_rows_typed %6.1f us (k = %d)"
          % (q["queries"], q["rank_rows_us"], q["rank_rows_typed_us"], q["topk_rows_us"], q["topk_rows_typed_us"], q["k"]))
    print("train step, ms: " + ", ".join("%s %.4f" % (r["mode"], r["ms"]) for r in out["train_step"]["ms_per_step"]))


if __name__ == "__main__":
    main()
