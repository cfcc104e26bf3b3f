"""rgcn_rank_mixed_device (csrc/ranking.hip, k_rank_rows_mixed) on the GPU: ranks under weight x own score + (1 - weight)
x partner score, against rgcn_rank_device where the weight makes them equal (bit for bit) and against the float64
mixed_ranks of tests/embedding_reference.py on every comparable query elsewhere (tests/test_embedding_host.py asserts, on
the CPU and for these very inputs, that the comparability margin leaves out at most 5 % of a case's queries).  Then two
contexts alive at once -- one's score buffer read in place by the other -- and the ensemble command end to end."""
import os

import numpy as np
import pytest

import embedding_reference as er
from test_embedding_host import DISTMULT_EXP
from test_gpu_driver import SETTINGS, write_dataset
from test_gpu_embedding import INVALID, STATE, status_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module", params=sorted(er.MIXED_SHAPES))
def case(request):
    return er.mixed_case(request.param)


def engine(native, case, params, reserve=None):
    eng = native.Engine(case["V"], case["R"], case["d"], 0, "embedding", 1)
    eng.set_params(params)
    eng.forward(train=False)
    eng.rank_reserve(reserve or case["n"])
    return eng


def test_weights_one_and_zero_are_one_model_s_own_ranks(native, case):
    q, n = case["queries"], case["n"]
    with engine(native, case, case["b"]) as eng_b:
        own_b = {}
        for side, s in case["sides"].items():
            ranks = eng_b.ranks(q, side, s["ptr"], s["idx"])
            own_b[side] = (ranks, eng_b.read_buffer(native.BUF_RANK_ENERGIES)[:n].copy())      # read back: the partner
    with engine(native, case, case["a"]) as eng:
        for side, s in case["sides"].items():
            own = eng.ranks(q, side, s["ptr"], s["idx"])
            left = eng.read_buffer(native.BUF_RANK_ENERGIES).copy()
            (ranks_b, energies_b) = own_b[side]
            # the device's energies are the float64 ones within float32 rounding of a d-term dot product
            assert float(np.abs(left[:n] - s["ea"]).max()) <= 1e-5 * max(1.0, float(np.abs(s["ea"]).max()))
            one = eng.ranks_mixed(q, side, energies_b, 1.0, s["ptr"], s["idx"])
            np.testing.assert_array_equal(one[0], own[0])
            np.testing.assert_array_equal(one[1], own[1])
            # RGCN_BUF_RANK_ENERGIES afterwards: the context's own energies, what rgcn_rank_device leaves, bit for bit
            np.testing.assert_array_equal(eng.read_buffer(native.BUF_RANK_ENERGIES), left)
            zero = eng.ranks_mixed(q, side, energies_b, 0.0, s["ptr"], s["idx"])
            np.testing.assert_array_equal(zero[0], ranks_b[0])
            np.testing.assert_array_equal(zero[1], ranks_b[1])
            # N = 1: one workgroup, and the row stride of the partner is still V
            for i in (0, n - 1):
                sub_ptr = s["ptr"][i:i + 2] - s["ptr"][i]
                sub_idx = s["idx"][s["ptr"][i]:s["ptr"][i + 1]]
                single = eng.ranks_mixed(q[i:i + 1], side, energies_b[i:i + 1], 1.0, sub_ptr, sub_idx)
                assert (single[0][0], single[1][0]) == (own[0][i], own[1][i])


@pytest.mark.parametrize("weight", er.MIXED_WEIGHTS)
def test_mixed_weights_against_float64(native, case, weight):
    q, n = case["queries"], case["n"]
    left_out = total = 0
    with engine(native, case, case["a"]) as eng:
        for side, s in case["sides"].items():
            raw, filt = eng.ranks_mixed(q, side, s["eb"], weight, s["ptr"], s["idx"])      # N = the reserved count
            raw64, filt64 = er.mixed_ranks(s["ea"], s["eb"], weight, s["gold"], s["lists"])
            ok = er.comparable(s["ea"], s["eb"], weight, s["gold"])
            left_out += int((~ok).sum())
            total += n
            np.testing.assert_array_equal(raw[ok], raw64[ok])
            np.testing.assert_array_equal(filt[ok], filt64[ok])
            empty = np.flatnonzero(np.diff(s["ptr"]) == 0)
            assert len(empty) and (filt[empty] == raw[empty] + 1).all()           # an empty list filters nothing
            assert (raw >= 1).all() and (raw <= case["V"]).all()
    print("V %d weight %.1f: %d of %d queries left out" % (case["V"], weight, left_out, total))
    assert left_out <= er.MAX_LEFT_OUT * total


def test_filter_lists_with_the_gold_alone_and_twice(native, case):
    """list = [gold]: filtered == raw; list = [gold, gold]: the duplicate counts twice, filtered == raw - 1 (the device's
    rule, mixed_ranks' too); lists of every entity: filtered == 1"""
    q, n, V = case["queries"], case["n"], case["V"]
    with engine(native, case, case["a"]) as eng:
        for side, s in case["sides"].items():
            gold = s["gold"].astype(np.int32)
            raw, filt = eng.ranks_mixed(q, side, s["eb"], 0.5, np.arange(n + 1, dtype=np.int64), gold)
            np.testing.assert_array_equal(filt, raw)
            raw2, filt2 = eng.ranks_mixed(q, side, s["eb"], 0.5, 2 * np.arange(n + 1, dtype=np.int64), np.repeat(gold, 2))
            np.testing.assert_array_equal(raw2, raw)
            np.testing.assert_array_equal(filt2, raw - 1)
            everyone = np.tile(np.arange(V, dtype=np.int32), n)
            raw3, filt3 = eng.ranks_mixed(q, side, s["eb"], 0.5, V * np.arange(n + 1, dtype=np.int64), everyone)
            np.testing.assert_array_equal(raw3, raw)
            assert (filt3 == 1).all()


def test_saturated_scores_tie(native, case):
    """own energies driven past the fp32 sigmoid's saturation and partner energies of +100 / -100 on every entity of a row:
    every mixed score is the gold's, raw rank = V"""
    q, n, V, d = case["queries"][:8], 8, case["V"], case["d"]
    big = {"W_emb": np.full((V, d), 3.0, np.float32), "b_emb": np.zeros(d, np.float32),
           "W_relation": np.full((V, d), 3.0, np.float32)}                         # energy = 27 d >= 432: sigmoid == 1.0f
    ptr, idx = np.arange(n + 1, dtype=np.int64), None
    with engine(native, case, big) as eng:
        for side in (True, False):
            gold = (q[:, 2] if side else q[:, 0]).astype(np.int32)
            partner = np.full((n, V), 100.0, np.float32)
            partner[1::2] = -100.0                                                  # sigmoid(-100) = 3.7e-44: a denormal, the same on every entity
            for w in (0.0, 0.3, 1.0):
                raw, filt = eng.ranks_mixed(q, side, partner, w, ptr, gold)
                assert (raw == V).all() and (filt == V).all(), (side, w, raw)
            own = eng.ranks(q, side, ptr, gold)
            assert (own[0] == V).all()


def test_status_codes(native, case):
    q, n, V = case["queries"], case["n"], case["V"]
    s = case["sides"][True]
    eng = native.Engine(V, case["R"], case["d"], 0, "embedding", 1)
    try:
        eng.set_params(case["a"])
        args = (q, True, s["eb"], 0.5, s["ptr"], s["idx"])
        assert eng.rank_energies_device() is None
        assert status_of(native, eng.ranks_mixed, *args)[0] == STATE                 # before a forward pass
        eng.forward(train=False)
        assert status_of(native, eng.ranks_mixed, *args)[0] == STATE                 # before rgcn_rank_reserve
        eng.rank_reserve(n)
        assert eng.rank_energies_device() is not None
        good = eng.ranks_mixed(*args)
        for w in (-0.1, 1.5, float("nan")):
            st, msg = status_of(native, eng.ranks_mixed, q, True, s["eb"], w, s["ptr"], s["idx"])
            assert st == INVALID and "weight" in msg, (w, msg)
        # one chunk only: N above the reserve
        more = np.concatenate([q, q[:1]])
        ptr_more = np.concatenate([s["ptr"], s["ptr"][-1:]])
        partner_more = np.concatenate([s["eb"], s["eb"][:1]])
        st, msg = status_of(native, eng.ranks_mixed, more, True, partner_more, 0.5, ptr_more, s["idx"])
        assert st == INVALID and "chunk" in msg
        # ids out of range are caught by the check kernel (nothing is dereferenced with them)
        for col, bad in ((0, V), (2, -1), (1, case["R"])):
            x = q.copy()
            x[3, col] = bad
            assert status_of(native, eng.ranks_mixed, x, True, s["eb"], 0.5, s["ptr"], s["idx"])[0] == INVALID
        idx_bad = s["idx"].copy()
        idx_bad[5] = V
        assert status_of(native, eng.ranks_mixed, q, True, s["eb"], 0.5, s["ptr"], idx_bad)[0] == INVALID
        ptr_bad = s["ptr"].copy()
        ptr_bad[2] = ptr_bad[1] - 1                                               # a decreasing range
        assert status_of(native, eng.ranks_mixed, q, True, s["eb"], 0.5, ptr_bad, s["idx"])[0] == INVALID
        again = eng.ranks_mixed(*args)                                             # and the context is as good as before
        np.testing.assert_array_equal(again[0], good[0])
        np.testing.assert_array_equal(again[1], good[1])
    finally:
        eng.close()


def test_two_contexts_alive_at_once(native):
    """a basis engine and an embedding engine in one process on one GPU: each gives the ranks it gives alone, and the
    pointer hand-over (one's score buffer read in place by the other, after rgcn_sync) equals the uploaded copy exactly"""
    from helpers import make_case
    V, R, d, E, n = 120, 5, 16, 400, 40
    params, triples, _, _ = make_case(V, R, d, 2, "basis", 2, E, seed=3)
    rng = np.random.RandomState(4)
    emb = {"W_emb": (rng.randn(V, d) * 0.6).astype(np.float32), "b_emb": np.zeros(d, np.float32),
           "W_relation": rng.randn(V, d).astype(np.float32)}
    q = triples[:n].astype(np.int32)
    ptr, idx = np.arange(n + 1, dtype=np.int64), q[:, 2].astype(np.int32).copy()

    def basis_engine():
        eng = native.Engine(V, R, d, 2, "basis", 2, max_edges=E)
        eng.set_params(params)
        eng.set_graph(triples)
        eng.forward(train=False)
        eng.rank_reserve(n)
        return eng

    def embedding_engine():
        eng = native.Engine(V, R, d, 0, "embedding", 1)
        eng.set_params(emb)
        eng.forward(train=False)
        eng.rank_reserve(n)
        return eng

    with basis_engine() as alone:
        basis_alone = alone.ranks(q, True, ptr, idx)
        basis_energy = alone.read_buffer(native.BUF_RANK_ENERGIES)[:n].copy()
    with embedding_engine() as alone:
        emb_alone = alone.ranks(q, True, ptr, idx)
        emb_energy = alone.read_buffer(native.BUF_RANK_ENERGIES)[:n].copy()
    with basis_engine() as first, embedding_engine() as second:
        # interleaved calls: neither disturbs the other
        r2 = second.ranks(q, True, ptr, idx)
        r1 = first.ranks(q, True, ptr, idx)
        for got, want in ((r1, basis_alone), (r2, emb_alone)):
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(first.read_buffer(native.BUF_RANK_ENERGIES)[:n], basis_energy)
        np.testing.assert_array_equal(second.read_buffer(native.BUF_RANK_ENERGIES)[:n], emb_energy)
        for w in (0.0, 0.5, 1.0):
            second.sync()
            by_pointer = first.ranks_mixed(q, True, second.rank_energies_device(), w, ptr, idx)
            by_copy = first.ranks_mixed(q, True, emb_energy, w, ptr, idx)
            np.testing.assert_array_equal(by_pointer[0], by_copy[0])
            np.testing.assert_array_equal(by_pointer[1], by_copy[1])
            # ... and the other way round
            first.sync()
            back = second.ranks_mixed(q, True, first.rank_energies_device(), 1.0 - w, ptr, idx)
            np.testing.assert_array_equal(back[0], by_copy[0])
            np.testing.assert_array_equal(back[1], by_copy[1])
        np.testing.assert_array_equal(by_pointer[0], basis_alone[0])               # (w = 1 came last)
        # a train step on one context leaves the other's codes and ranks alone
        second.decoder_reserve(n)
        second.optimizer_config(lr=0.01, max_grad_norm=1.0)
        xd, yd = second.to_device(q), second.to_device(np.ones(n, np.float32))
        second.train_step_device(None, 0, xd, yd, n, seed=1, reg_param=0.01)
        assert np.isfinite(second.loss())
        again = first.ranks(q, True, ptr, idx)
        np.testing.assert_array_equal(again[0], basis_alone[0])
        for b in (xd, yd):
            b.free()


def test_ensemble_command_end_to_end(tmp_path, capsys):
    from relationprediction_amd import ensemble, train
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
    capsys.readouterr()

    def run(weight):
        np.random.seed(1)
        out = ensemble.main(["--settings", str(files["basis"]), "--model", str(tmp_path / "models" / "basis-0.npz"),
                             "--settings2", str(files["distmult"]), "--model2", str(tmp_path / "models" / "distmult-0.npz"),
                             "--dataset", data, "--weight", str(weight)])
        lines = capsys.readouterr().out.splitlines()
        heads = [i for i, l in enumerate(lines) if l.startswith(("Model 1", "Model 2", "Ensemble"))]
        assert len(heads) == 3
        blocks = [lines[i + 1:i + 6] for i in heads]
        for b in blocks:                                     # Scorer's summary: a header and four rows
            assert b[0] == "\tRaw\tFiltered" and [r.split("\t")[0] for r in b[1:]] == ["MRR", "H@1", "H@3", "H@10"]
        return out, blocks

    out, blocks = run(0.5)
    assert set(out) == {"first", "second", "ensemble"}
    for s in out.values():
        assert 0.0 < s.results['Filtered']['MRR'] <= 1.0 and s.results['Raw']['MRR'] <= s.results['Filtered']['MRR']
    out1, blocks1 = run(1)
    assert blocks1[2] == blocks1[0] and out1["ensemble"].results == out1["first"].results
    out0, blocks0 = run(0)
    assert blocks0[2] == blocks0[1] and out0["ensemble"].results == out0["second"].results
    assert blocks0[0] == blocks1[0] == blocks[0] and blocks0[1] == blocks1[1] == blocks[1]
    with pytest.raises(ValueError):
        ensemble.main(["--settings", str(files["basis"]), "--model", "x", "--settings2", str(files["distmult"]),
                       "--model2", "y", "--dataset", data, "--weight", "1.5"])
