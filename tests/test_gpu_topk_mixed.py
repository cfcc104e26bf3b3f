"""rgcn_topk_mixed_device and rgcn_score_queries_device (csrc/ranking.hip: k_mix_rows, then k_topk_rows on the mixed
scores) on the GPU -- `-m gpu`, embedding engines throughout.  The mixed scores the device wrote (RGCN_BUF_RANK_MIXED_SCORES)
are held to float64 within 2^-23; the selection is held BIT-EXACT to tests/topk_mixed_reference.py on those scores; the
grid case of that file pins the ids with no exponential evaluated on the host at all; and the count of returned scores at
or above a gold entity's equals rgcn_rank_mixed_device's raw rank exactly.  Then the buffers the call leaves, the status
codes, the scratch's ownership and the command end to end."""
import os

import numpy as np
import pytest

import embedding_reference as er
import topk_mixed_reference as tm
from test_embedding_host import DISTMULT_EXP
from test_gpu_driver import SETTINGS, write_dataset
from test_gpu_embedding import INVALID, STATE, status_of

pytestmark = pytest.mark.gpu

SCORE_BOUND = 2.0 ** -23
"""each fp32 sigmoid lies within 2^-25 of the exact one (a value in [0, 1] rounded once), the weighted sum inherits at most
that, the final rounding adds 2^-25: below 2^-24 in all, and the bound gives that twice over to absorb a last-place
difference between the device's and numpy's exp"""


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module", params=sorted(er.MIXED_SHAPES))
def case(request):
    return er.mixed_case(request.param)


def engine(native, case, params, reserve=None, **kw):
    eng = native.Engine(case["V"], case["R"], case["d"], 0, "embedding", 1, **kw)
    eng.set_params(params)
    eng.forward(train=False)
    eng.rank_reserve(reserve or case["n"])
    return eng


def blank_unread(queries, object_side):
    q = queries.copy()
    q[:, 2 if object_side else 0] = -1
    return q


def ks_for(V):
    return (1, 10, V)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_selection(M, idx, score, k, lists, tag):
    assert idx.shape == score.shape == (len(M), k) and idx.dtype == np.int32 and score.dtype == np.float32
    for i in range(len(M)):
        want_idx, want_score = tm.mixed_topk(M[i], k, lists[i] if lists is not None else ())
        assert np.array_equal(idx[i], want_idx), (tag, i, idx[i][:8], want_idx[:8])
        assert np.array_equal(bits(score[i]), bits(want_score)), (tag, i)


@pytest.mark.parametrize("weight", er.MIXED_WEIGHTS)
def test_mixed_scores_against_float64_and_the_selection_exactly(native, case, weight):
    """cases 1 and 2: every M[i, e] within 2^-23 of the float64 mix of the device's own fp32 energies and the uploaded
    partner; (idx, score) == mixed_topk(M) bit for bit for every row, k in {1, 10, V} and exclusion list (none, with
    duplicates and empty rows, fewer than k left); a second call returns the same bytes"""
    n, V = case["n"], case["V"]
    worst = 0.0
    with engine(native, case, case["a"]) as eng:
        for side, s in case["sides"].items():
            q = blank_unread(case["queries"], side)
            for kind, lists in tm.exclusion_variants(V, s["lists"]).items():
                ptr, flat = tm.csr(lists) if lists is not None else (None, None)
                for k in ks_for(V):
                    idx, score = eng.topk_mixed(q, side, k, s["eb"], weight, ptr, flat)
                    M = eng.read_buffer(native.BUF_RANK_MIXED_SCORES)[:n]
                    own = eng.read_buffer(native.BUF_RANK_ENERGIES)[:n]
                    err = float(np.abs(M.astype(np.float64) - er.mixed_scores(own, s["eb"], weight)).max())
                    worst = max(worst, err)
                    assert err <= SCORE_BOUND, (side, kind, k, err)
                    assert_selection(M, idx, score, k, lists, (side, kind, k))
                    left = [V - len(set(x)) for x in lists] if lists is not None else [V] * n
                    assert [(r >= 0).sum() for r in idx] == [min(k, x) for x in left]
            again = eng.topk_mixed(q, side, k, s["eb"], weight, ptr, flat)
            assert np.array_equal(again[0], idx) and np.array_equal(bits(again[1]), bits(score))
    print("V %d weight %.1f: largest |M - float64| = %.3g (bound %.3g)" % (V, weight, worst, SCORE_BOUND))


def test_grid_case_ids_are_exact(native):
    """case 3: own and partner energies on a grid of half-integers, weight 0.5 -- equal (own, partner) pairs tie bit for
    bit, different pairs lie 6.9e-3 apart, so the ids follow from a lexsort of float64 values however an exponential is
    rounded.  V = 1100: past one 1,024-entity trip of the select loops and no multiple of it."""
    (V, n), = tm.GRID_SHAPES.values()
    c = tm.grid_case(V, n)
    with engine(native, c, c["params"]) as eng:
        for side in (True, False):
            q = blank_unread(c["queries"], side)
            for kind, lists in tm.exclusion_variants(V, c["lists"]).items():
                ptr, flat = tm.csr(lists) if lists is not None else (None, None)
                for k in (1, 10, 1024):                               # (k = V is above RGCN_MAX_TOPK here)
                    idx, score = eng.topk_mixed(q, side, k, c["partner"], tm.GRID_WEIGHT, ptr, flat)
                    for i in range(n):
                        want = tm.expected_ids(c["m"][i], k, lists[i] if lists is not None else ())
                        assert np.array_equal(idx[i], want), (side, kind, k, i)
            assert np.array_equal(eng.read_buffer(native.BUF_RANK_ENERGIES)[:n], c["own"])       # exact by construction
            M = eng.read_buffer(native.BUF_RANK_MIXED_SCORES)[:n]
            assert float(np.abs(M - c["m"]).max()) <= SCORE_BOUND


@pytest.mark.parametrize("weight", (0.0, 0.5, 1.0))
def test_agreement_with_the_ensemble_ranks(native, case, weight):
    """case 4: k = V, no exclusions; #{returned scores >= the score in the gold entity's slot} is rgcn_rank_mixed_device's
    raw rank for the same query, partner and weight -- both sides call the same mixed_score, so exactly"""
    n, V = case["n"], case["V"]
    with engine(native, case, case["a"]) as eng:
        for side, s in case["sides"].items():
            raw, _ = eng.ranks_mixed(case["queries"], side, s["eb"], weight, s["ptr"], s["idx"])
            idx, score = eng.topk_mixed(blank_unread(case["queries"], side), side, V, s["eb"], weight)
            for i, g in enumerate(s["gold"]):
                slot, = np.flatnonzero(idx[i] == g)
                assert int((score[i] >= score[i, slot]).sum()) == raw[i], (side, i)


def distinct_at_the_cut(M, k, lists):
    """rows whose k + 1 best non-excluded scores are pairwise distinct"""
    ok = np.zeros(len(M), dtype=bool)
    for i in range(len(M)):
        _, best = tm.mixed_topk(M[i], min(k + 1, M.shape[1]), lists[i] if lists is not None else ())
        best = best[np.isfinite(best)]
        ok[i] = len(np.unique(best)) == len(best)
    return ok


def test_weights_one_and_zero_are_one_model_alone(native, case):
    """case 5: at weight 1 M is the fp32 sigmoid of the own energies, at weight 0 of the partner's, as k_mix_rows computes
    it: the two are compared on the device's own results (engine a at weight 1 against engine b at weight 0 with a's
    energies as the partner, and the other way round) bit for bit, and against numpy's within one last place of a value in
    [0.5, 1], 2^-24.  The selection is mixed_topk of that M, and wherever a row's k + 1 best scores are pairwise distinct
    the ids are rgcn_topk_device's of the model that counts."""
    n, V = case["n"], case["V"]
    with engine(native, case, case["a"]) as a, engine(native, case, case["b"]) as b:
        for side, s in case["sides"].items():
            q = blank_unread(case["queries"], side)
            ptr, flat = tm.csr(s["lists"])
            for k in ks_for(V):
                plain = {}
                for name, eng in (("a", a), ("b", b)):
                    ids, _ = eng.topk(q, side, k, ptr, flat)
                    plain[name] = (ids, eng.read_buffer(native.BUF_RANK_ENERGIES)[:n].copy())
                # (engine, its weight, the partner's energies, whose scores M must hold)
                runs = {"a1": (a, 1.0, plain["b"][1], "a"), "a0": (a, 0.0, plain["b"][1], "b"),
                        "b1": (b, 1.0, plain["a"][1], "b"), "b0": (b, 0.0, plain["a"][1], "a")}
                M = {}
                for tag, (eng, w, partner, whose) in runs.items():
                    idx, score = eng.topk_mixed(q, side, k, partner, w, ptr, flat)
                    M[tag] = eng.read_buffer(native.BUF_RANK_MIXED_SCORES)[:n].copy()
                    assert_selection(M[tag], idx, score, k, s["lists"], (tag, side, k))
                    host = er.sigmoid64(plain[whose][1]).astype(np.float32)
                    assert float(np.abs(M[tag] - host).max()) <= 2.0 ** -24, (tag, side, k)
                    ok = distinct_at_the_cut(M[tag], k, s["lists"])
                    assert ok.sum() >= n // 2, (tag, side, k, int(ok.sum()))
                    assert np.array_equal(idx[ok], plain[whose][0][ok]), (tag, side, k)
                assert np.array_equal(bits(M["a1"]), bits(M["b0"])) and np.array_equal(bits(M["b1"]), bits(M["a0"]))


def test_buffers_after_the_call_and_the_partner_by_pointer(native, case):
    """case 6: RGCN_BUF_RANK_ENERGIES afterwards is bitwise what rgcn_topk_device leaves; the partner array is unchanged;
    N = 1 and N = the reserve; the partner as a pointer to another live engine's score buffer (rgcn_score_queries_device
    there) gives the bytes an uploaded copy gives"""
    n, V = case["n"], case["V"]
    with engine(native, case, case["a"]) as eng, engine(native, case, case["b"]) as other:
        for side, s in case["sides"].items():
            q = blank_unread(case["queries"], side)
            ptr, flat = tm.csr(s["lists"])
            eng.topk(q, side, 10, ptr, flat)
            left = eng.read_buffer(native.BUF_RANK_ENERGIES).copy()
            partner = native.DeviceBuffer(eng, s["eb"].nbytes).upload(s["eb"])
            try:
                by_buffer = eng.topk_mixed(q, side, 10, partner, 0.4, ptr, flat)            # N = the reserve
                assert np.array_equal(bits(eng.read_buffer(native.BUF_RANK_ENERGIES)), bits(left))
                assert np.array_equal(bits(partner.download(np.float32, s["eb"].shape)), bits(s["eb"]))
            finally:
                partner.free()
            by_array = eng.topk_mixed(q, side, 10, s["eb"], 0.4, ptr, flat)
            assert np.array_equal(by_buffer[0], by_array[0]) and np.array_equal(bits(by_buffer[1]), bits(by_array[1]))
            for i in (0, n - 1):                                       # N = 1: one workgroup, one row of the partner
                sub_ptr, sub_idx = ptr[i:i + 2] - ptr[i], flat[ptr[i]:ptr[i + 1]]
                eng.topk(q[i:i + 1], side, 10, sub_ptr, sub_idx)
                left_one = eng.read_buffer(native.BUF_RANK_ENERGIES)[:1].copy()
                one = eng.topk_mixed(q[i:i + 1], side, 10, s["eb"][i:i + 1], 0.4, sub_ptr, sub_idx)
                assert np.array_equal(bits(eng.read_buffer(native.BUF_RANK_ENERGIES)[:1]), bits(left_one))
                M = eng.read_buffer(native.BUF_RANK_MIXED_SCORES)[:1]
                assert float(np.abs(M - er.mixed_scores(left_one, s["eb"][i:i + 1], 0.4)).max()) <= SCORE_BOUND
                assert_selection(M, one[0], one[1], 10, [s["lists"][i]], (side, "N=1", i))
            # the other engine scores the same queries and hands its buffer over in place
            other.score_queries(q, side)
            copy = other.read_buffer(native.BUF_RANK_ENERGIES)[:n].copy()
            by_pointer = eng.topk_mixed(q, side, 10, other.rank_energies_device(), 0.4, ptr, flat)
            by_copy = eng.topk_mixed(q, side, 10, copy, 0.4, ptr, flat)
            assert np.array_equal(by_pointer[0], by_copy[0]) and np.array_equal(bits(by_pointer[1]), bits(by_copy[1]))
            assert np.array_equal(bits(other.read_buffer(native.BUF_RANK_ENERGIES)[:n]), bits(copy))


def test_score_queries_leaves_the_energies_of_topk_and_rank(native, case):
    """case 7: bitwise the energies of rgcn_topk_device and of rgcn_rank_device on the same rows, with the predicted column
    set to -1"""
    n = case["n"]
    with engine(native, case, case["a"]) as eng:
        for side, s in case["sides"].items():
            eng.ranks(case["queries"], side, s["ptr"], s["idx"])
            by_rank = eng.read_buffer(native.BUF_RANK_ENERGIES).copy()
            eng.topk(blank_unread(case["queries"], side), side, 1)
            by_topk = eng.read_buffer(native.BUF_RANK_ENERGIES).copy()
            eng.topk(blank_unread(case["queries"][::-1], side), side, 1)             # something else in the buffer
            eng.score_queries(blank_unread(case["queries"], side), side)
            got = eng.read_buffer(native.BUF_RANK_ENERGIES)
            assert np.array_equal(bits(got), bits(by_topk)) and np.array_equal(bits(got), bits(by_rank))
            assert float(np.abs(got[:n] - s["ea"]).max()) <= 1e-5 * max(1.0, float(np.abs(s["ea"]).max()))
            eng.topk(blank_unread(case["queries"][3:4], side), side, 1)              # N = 1
            one = eng.read_buffer(native.BUF_RANK_ENERGIES)[:1].copy()
            eng.topk(blank_unread(case["queries"][5:6], side), side, 1)
            eng.score_queries(blank_unread(case["queries"][3:4], side), side)
            assert np.array_equal(bits(eng.read_buffer(native.BUF_RANK_ENERGIES)[:1]), bits(one))


def test_status_codes(native, case):
    """case 8"""
    q, n, V = blank_unread(case["queries"], True), case["n"], case["V"]
    s = case["sides"][True]
    ptr, flat = tm.csr(s["lists"])
    eng = native.Engine(V, case["R"], case["d"], 0, "embedding", 1)
    try:
        eng.set_params(case["a"])
        args = (q, True, 10, s["eb"], 0.5, ptr, flat)
        assert status_of(native, eng.topk_mixed, *args)[0] == STATE                  # before a forward pass
        assert status_of(native, eng.score_queries, q, True)[0] == STATE
        eng.forward(train=False)
        assert status_of(native, eng.topk_mixed, *args)[0] == STATE                  # before rgcn_rank_reserve
        assert status_of(native, eng.score_queries, q, True)[0] == STATE
        eng.rank_reserve(n)
        eng.score_queries(q, True)
        eng.topk(q, True, 10, ptr, flat)
        assert status_of(native, eng.read_buffer, native.BUF_RANK_MIXED_SCORES)[0] == STATE    # before the first mixed call
        good = eng.topk_mixed(*args)
        assert eng.read_buffer(native.BUF_RANK_MIXED_SCORES).shape == (n, V)
        for w in (-0.1, 1.5, float("nan")):
            st, msg = status_of(native, eng.topk_mixed, q, True, 10, s["eb"], w, ptr, flat)
            assert st == INVALID and "weight" in msg, (w, msg)
        more = np.concatenate([q, q[:1]])                                            # one chunk only
        st, msg = status_of(native, eng.topk_mixed, more, True, 10, np.concatenate([s["eb"], s["eb"][:1]]), 0.5,
                            np.concatenate([ptr, ptr[-1:]]), flat)
        assert st == INVALID and "chunk" in msg
        st, msg = status_of(native, eng.score_queries, more, True)
        assert st == INVALID and "chunk" in msg
        for k in (0, min(V, 1024) + 1):
            assert status_of(native, eng.topk_mixed, q, True, k, s["eb"], 0.5, ptr, flat)[0] == INVALID
        for col, bad in ((0, V), (0, -1), (1, case["R"])):                           # the two ids that are read
            x = q.copy()
            x[3, col] = bad
            assert status_of(native, eng.topk_mixed, x, True, 10, s["eb"], 0.5, ptr, flat)[0] == INVALID
            assert status_of(native, eng.score_queries, x, True)[0] == INVALID
        flat_bad = flat.copy()
        flat_bad[5] = V
        assert status_of(native, eng.topk_mixed, q, True, 10, s["eb"], 0.5, ptr, flat_bad)[0] == INVALID
        ptr_bad = ptr.copy()
        ptr_bad[2] = ptr_bad[1] - 1                                                  # a decreasing range
        assert status_of(native, eng.topk_mixed, q, True, 10, s["eb"], 0.5, ptr_bad, flat)[0] == INVALID
        with pytest.raises(ValueError):
            eng.topk_mixed(q, True, 10, s["eb"], 0.5, ptr, None)
        again = eng.topk_mixed(*args)                                                # the context is as good as before
        assert np.array_equal(again[0], good[0]) and np.array_equal(bits(again[1]), bits(good[1]))
    finally:
        eng.close()


def test_growing_the_reserve_releases_the_scratch_and_the_next_call_allocates_it_again(native, case):
    """case 9: a context that never asks the ensemble holds what it held; after reserve, mixed call, a larger reserve and
    another mixed call it holds what a fresh context holds after the same two calls, and answers the same"""
    native.load_library(devtools=True)
    n, V = case["n"], case["V"]
    s = case["sides"][True]
    q = blank_unread(case["queries"], True)
    ptr, flat = tm.csr(s["lists"])
    scratch = lambda rows: 4 * rows * V

    def calls(eng):
        return eng.topk_mixed(q[:n // 2], True, 10, s["eb"][:n // 2], 0.5, ptr[:n // 2 + 1], flat[:ptr[n // 2]])

    with engine(native, case, case["a"], reserve=n // 2, devtools=True) as eng:
        eng.topk(q[:n // 2], True, 10)
        blocks0, bytes0 = eng.device_memory()                       # reserve and plain top-k: no scratch
        first = calls(eng)
        assert eng.device_memory() == (blocks0 + 1, bytes0 + scratch(n // 2))
        calls(eng)
        assert eng.device_memory() == (blocks0 + 1, bytes0 + scratch(n // 2))        # allocated once
        eng.rank_reserve(n)                                         # grows: everything is released, the scratch too
        blocks1, bytes1 = eng.device_memory()
        assert blocks1 == blocks0 and status_of(native, eng.read_buffer, native.BUF_RANK_MIXED_SCORES)[0] == STATE
        second = calls(eng)
        assert np.array_equal(second[0], first[0]) and np.array_equal(bits(second[1]), bits(first[1]))
        grown = eng.device_memory()
        assert grown == (blocks1 + 1, bytes1 + scratch(n))
        eng.rank_reserve(n // 2)                                    # does not shrink: nothing moves
        assert eng.device_memory() == grown
    with engine(native, case, case["a"], reserve=n, devtools=True) as fresh:
        assert fresh.device_memory() == (blocks1, bytes1)
        third = calls(fresh)
        assert fresh.device_memory() == grown
        assert np.array_equal(third[0], first[0]) and np.array_equal(bits(third[1]), bits(first[1]))


def test_predict_command_with_the_ensemble_end_to_end(tmp_path):
    """case 10: two iterations each of a gcn_basis and a DistMult model on the toy world, then predict with --settings2 /
    --model2: positions from 1, scores non-increasing per query, known completions absent, the line count; --weight 1
    gives plain predict's scores within 2^-23 and its answers wherever plain predict's consecutive scores differ by more"""
    from relationprediction_amd import predict, train
    from relationprediction_amd.common import evaluation
    data = str(tmp_path / "data")
    write_dataset(data)
    os.makedirs(str(tmp_path / "models"))
    files = {}
    for name, text in (("basis", SETTINGS % dict(nb=2, concat="No", exp=str(tmp_path / "models" / "Basis"))),
                       ("distmult", (DISTMULT_EXP % 20).replace("models/Distmult", str(tmp_path / "models" / "Distmult")))):
        files[name] = tmp_path / (name + ".exp")
        files[name].write_text(text)
        np.random.seed(0)
        model, iterations = train.main(["--settings", str(files[name]), "--dataset", data, "--max-iterations", "2",
                                        "--batch-workers", "0"])
        assert iterations == 2
        model.save(str(tmp_path / "models" / name))
    k, V = 7, 200
    rng = np.random.RandomState(3)
    pairs = [(int(e), int(r)) for e, r in zip(rng.randint(0, V, 25), rng.randint(0, 6, 25))]
    (tmp_path / "q.txt").write_text("".join("e%d\tr%d\n" % p for p in pairs))
    known = {}
    for part in ("train", "valid", "test"):
        rows = [l.split("\t") for l in open(os.path.join(data, part + ".txt")).read().splitlines()]
        evaluation.Scorer.extend_triple_dict(known, [(int(s[1:]), int(r[1:]), int(o[1:])) for s, r, o in rows])

    def run(*extra, answers=k):
        np.random.seed(1)
        out = tmp_path / "answers.txt"
        predict.main(["--settings", str(files["basis"]), "--model", str(tmp_path / "models" / "basis-0.npz"), "--dataset",
                      data, "--queries", str(tmp_path / "q.txt"), "--k", str(answers), "--out", str(out)] + list(extra))
        return [l.split("\t") for l in out.read_text().splitlines()]

    second = ["--settings2", str(files["distmult"]), "--model2", str(tmp_path / "models" / "distmult-0.npz")]
    lines = run(*(second + ["--weight", "0.5"]))
    assert len(lines) == k * len(pairs) and all(len(l) == 5 for l in lines)           # 200 entities: every row is full
    for i, (e, r) in enumerate(pairs):
        rows = lines[k * i:k * (i + 1)]
        assert all(l[0] == "e%d" % e and l[1] == "r%d" % r for l in rows)
        assert [l[3] for l in rows] == [str(p) for p in range(1, k + 1)]
        scores = [float(l[4]) for l in rows]
        assert scores == sorted(scores, reverse=True) and 0.0 <= scores[-1] and scores[0] <= 1.0
        assert not {int(l[2][1:]) for l in rows} & set(known.get((e, r), ()))
    assert any(known.get(p) for p in pairs)
    assert run(*second) == lines                                                      # 0.5 is the default
    # plain predict with one answer more: whether the k-th score stands clear of the next one is then visible too
    plain, one = run(answers=k + 1), run(*(second + ["--weight", "1"]))
    assert len(plain) == (k + 1) * len(pairs) and len(one) == len(lines)
    for i in range(len(pairs)):
        a, b = plain[(k + 1) * i:(k + 1) * (i + 1)], one[k * i:k * (i + 1)]
        sa, sb = np.array([float(l[4]) for l in a]), np.array([float(l[4]) for l in b])
        assert float(np.abs(sa[:k] - sb).max()) <= SCORE_BOUND
        clear = np.abs(np.diff(sa)) > SCORE_BOUND                    # [j]: positions j + 1 and j + 2 stand apart
        settled = np.concatenate([[True], clear[:-1]]) & clear
        assert [l[2] for l, ok in zip(a, settled) if ok] == [l[2] for l, ok in zip(b, settled) if ok]
