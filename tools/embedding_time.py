"""Kernel times of the DistMult baseline (Encoder.Name=embedding) and of the ensemble rank:

    python tools/embedding_time.py [steps] [queries] [reps]

1. The `Name=embedding` train step at FB15k-237 size.  settings/distmult.exp of the reference has no BatchSize, so an
   iteration's positives are the whole training set: 272,115 triples (synthetic here, drawn with oracle.synthetic_graph's
   skewed relation and entity frequencies over V = 14,541, R = 237), NegativeSampleRate = 10, d = 500 -- a decoder batch of
   N = 11 x 272,115 = 2,993,265 triples, corruptions drawn on the device, clip + Adam behind it.  Milliseconds per step
   from HIP events around `steps` consecutive steps after two warm-up steps, then the per-kernel rows of a second set of
   steps with the profile on (side streams off: durations are exclusive).
2. rgcn_rank_mixed_device next to rgcn_rank_device on the same `queries` (2,048) object-side queries, the real FB15k-237
   valid + test triples of tests/golden/graphs.npz with their known objects as filter lists, the partner's energies a
   second parameter set's, resident on the device.  Per-kernel microseconds per call over `reps` calls after two warm-ups.

A limit rgcn_decoder_reserve or the step hits at that N is printed as it is reported (status and message), not worked round."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from relationprediction_amd import _native  # noqa: E402

V, R, D, TRAIN, RATE = 14541, 237, 500, 272115, 10


def embedding_params(rng):
    return {"W_emb": (rng.randn(V, D) * 3 / np.sqrt(V + D)).astype(np.float32), "b_emb": np.zeros(D, np.float32),
            "W_relation": rng.randn(V, D).astype(np.float32)}


def rows_of(profile, calls):
    return [{"kernel": p["name"], "calls_per_step": p["calls"] / calls, "us_per_step": 1e3 * p["total_ms"] / calls,
             "design_MB_per_step": p["alg_bytes"] / calls / 1e6, "GFLOP_per_step": p["alg_flops"] / calls / 1e9}
            for p in profile]


def train_step(steps):
    rng = np.random.RandomState(0)
    train = np.ascontiguousarray(oracle.synthetic_graph(V, R, TRAIN, rng), dtype=np.int32)
    N = TRAIN * (RATE + 1)
    out = {"V": V, "R": R, "d": D, "positives": TRAIN, "negative_rate": RATE, "N": N, "steps": steps}
    eng = _native.Engine(V, R, D, 0, "embedding", 1)
    try:
        eng.set_params(embedding_params(rng))
        try:
            eng.decoder_reserve(N)
        except _native.RgcnError as e:
            out["decoder_reserve"] = {"status": e.status, "message": str(e)}
            return out
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        bd, xd, yd = eng.to_device(train), eng.alloc(12 * N), eng.alloc(4 * N)

        def step(i):
            eng.negative_sample_device(bd, TRAIN, RATE, 1000 + i, xd, yd)
            eng.train_step_device(None, 0, xd, yd, N, seed=i, reg_param=0.01)

        try:
            for i in range(2):
                step(i)
            out["loss_after_warmup"] = eng.loss()
            eng.timer_start()
            for i in range(steps):
                step(2 + i)
            out["ms_per_step"] = eng.timer_stop() / steps
            eng.set_overlap(False)
            eng.profile_enable(True)
            eng.profile_reset()
            for i in range(steps):
                step(2 + steps + i)
            out["kernels"] = rows_of(eng.profile(), steps)
            eng.profile_enable(False)
            out["loss_at_end"] = eng.loss()
        except _native.RgcnError as e:
            out["step"] = {"status": e.status, "message": str(e)}
        for b in (bd, xd, yd):
            b.free()
    finally:
        eng.close()
    return out


def mixed_rank(n, reps):
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
    fptr = np.zeros(n + 1, np.int64)
    fptr[1:] = np.cumsum([len(x) for x in lists])
    fidx = np.concatenate([np.asarray(x, np.int32) for x in lists])
    out = {"queries": n, "V": V, "d": D, "reps": reps}
    with _native.Engine(V, R, D, 0, "embedding", 1) as other:
        other.set_params(embedding_params(rng))
        other.forward(train=False)
        other.rank_reserve(n)
        other.ranks(queries, True, fptr, fidx)
        partner_host = other.read_buffer(_native.BUF_RANK_ENERGIES)[:n]
    with _native.Engine(V, R, D, 0, "embedding", 1) as eng:
        eng.set_params(embedding_params(rng))
        eng.forward(train=False)
        eng.rank_reserve(n)
        eng.set_overlap(False)
        partner = eng.to_device(partner_host)
        calls = {"rank": lambda: eng.ranks(queries, True, fptr, fidx),
                 "rank_mixed": lambda: eng.ranks_mixed(queries, True, partner, 0.5, fptr, fidx)}
        for name, call in calls.items():
            for _ in range(2):
                call()
            eng.profile_enable(True)
            eng.profile_reset()
            for _ in range(reps):
                call()
            rows = {p["name"]: p for p in eng.profile()}
            eng.profile_enable(False)
            out[name] = {k: {"us_per_call": 1e3 * v["total_ms"] / v["calls"],
                             "compulsory_bytes": v["compulsory_bytes"] / v["calls"],
                             "GB_per_s": v["compulsory_bytes"] / v["calls"] / (1e6 * v["total_ms"] / v["calls"])}
                         for k, v in rows.items() if k.startswith("rank_")}
        partner.free()
    return out


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    out = {"train_step": train_step(steps), "mixed_rank": mixed_rank(n, reps)}
    print(json.dumps(out, indent=1))
    ts = out["train_step"]
    if "ms_per_step" in ts:
        print("Name=embedding train step, N = %d: %.3f ms per step" % (ts["N"], ts["ms_per_step"]))
    mr = out["mixed_rank"]
    a, b = mr["rank"]["rank_rows"]["us_per_call"], mr["rank_mixed"]["rank_rows_mixed"]["us_per_call"]
    print("rank_rows %.1f us, rank_rows_mixed %.1f us (ratio %.1f), rank_scores %.1f us, %d queries"
          % (a, b, b / a, mr["rank"]["rank_scores"]["us_per_call"], n))


if __name__ == "__main__":
    main()
