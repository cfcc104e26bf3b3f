"""Host side of the ensemble top-k tests: the numpy selection of tests/topk_mixed_reference.py against a brute-force
sort, and the grid case's guarantees -- different (own, partner) pairs far apart, equal pairs exactly equal, ties across
position k -- for every shape tests/test_gpu_topk_mixed.py runs.  No GPU."""
import numpy as np

import embedding_reference as er
import topk_mixed_reference as tm


def brute_force(row, k, excluded):
    gone = set(int(e) for e in excluded)
    ids = [e for e in range(len(row)) if e not in gone]
    for i in range(1, len(ids)):           # insertion sort: value descending, id ascending
        j = i
        while j > 0 and (row[ids[j]] > row[ids[j - 1]] or (row[ids[j]] == row[ids[j - 1]] and ids[j] < ids[j - 1])):
            ids[j], ids[j - 1] = ids[j - 1], ids[j]
            j -= 1
    return ids[:k]


def test_mixed_topk_against_a_brute_force_sort():
    rng = np.random.RandomState(0)
    for trial in range(30):
        V = int(rng.randint(1, 60))
        row = (rng.randint(0, 5, size=V) / 4.0).astype(np.float32)            # values in [0, 1], forced ties
        if trial % 2:
            row = er.mixed_scores(rng.choice(tm.GRID, V), rng.choice(tm.GRID, V), 0.5).astype(np.float32)
        excluded = list(rng.randint(0, V, size=rng.randint(0, V + 1)))
        k = int(rng.randint(1, V + 3))
        idx, score = tm.mixed_topk(row, k, excluded)
        want = brute_force(row, k, excluded)
        assert idx.dtype == np.int32 and score.dtype == np.float32 and idx.shape == score.shape == (k,)
        assert idx[:len(want)].tolist() == want
        assert (idx[len(want):] == -1).all() and np.isneginf(score[len(want):]).all()
        assert np.array_equal(score[:len(want)].view(np.uint32), row[want].view(np.uint32))


def test_grid_margin_and_why_the_grid_has_seven_values():
    assert tm.grid_margin() > tm.MARGIN
    assert 1.0 in tm.GRID and all(x * 2 == int(x * 2) and -3 <= x <= 3 for x in tm.GRID)
    # both signs of one magnitude beside 0 (or beside another such pair) make two different pairs coincide
    assert tm.grid_margin(tm.GRID + (-0.5,)) < tm.MARGIN
    assert tm.grid_margin(tuple(np.arange(-3.0, 3.01, 0.5))) < tm.MARGIN


def test_grid_cases_are_exact_and_tie_across_position_k():
    for name, (V, n) in tm.GRID_SHAPES.items():
        c = tm.grid_case(V, n)
        assert c["own"].dtype == c["partner"].dtype == np.float32 and c["partner"].shape == (n, V)
        # the own energies: exact in float64 too, on both sides (the fixed entity is the same in either column)
        for side in (True, False):
            assert np.array_equal(er.energies(c["params"], c["queries"], side), c["own"].astype(np.float64))
        assert set(np.unique(c["own"])) <= set(tm.GRID) and set(np.unique(c["partner"])) <= set(tm.GRID)
        # equal unordered pairs hold equal float64 values, different pairs lie more than MARGIN apart
        lo, hi = np.minimum(c["own"], c["partner"]), np.maximum(c["own"], c["partner"])
        pair = (lo * 2 + 6).astype(np.int64) * 13 + (hi * 2 + 6).astype(np.int64)
        for i in range(n):
            order = np.argsort(c["m"][i], kind="stable")
            m, p = c["m"][i][order], pair[i][order]
            same = p[1:] == p[:-1]
            assert (np.diff(m)[same] == 0).all() and (np.diff(m)[~same] > tm.MARGIN).all(), (name, i)
        for kind, lists in tm.exclusion_variants(V, c["lists"]).items():
            if kind == "few_left":
                continue
            for k in tm.GRID_KS:
                rows = [i for i in range(n) if tm.tie_straddles(c["m"][i], k, lists[i] if lists else ())]
                assert rows, (name, kind, k)
        # the float32 rounding of the float64 values orders the same way: what the device must reproduce
        for i in range(0, n, 5):
            ids, _ = tm.mixed_topk(c["m"][i].astype(np.float32), 10, c["lists"][i])
            assert np.array_equal(ids, tm.expected_ids(c["m"][i], 10, c["lists"][i]))


def test_exclusion_variants_leave_what_they_say():
    for V in (30, 300, 1100):
        heavy = tm.exclusion_variants(V, [[]] * 15)["few_left"]
        assert [V - len(set(x)) for x in heavy] == [i % 7 for i in range(15)]
