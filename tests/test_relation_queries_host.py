"""Host side of the relation queries: the float64 / fp32-sigmoid reference on hand-made energies, the Scorer's
known_relation_triples and compute_relation_mrr_scores with a fake model, and `predict --side relation` driven with a
fake model.  No GPU."""
import numpy as np
import pytest

from relationprediction_amd import predict
from relationprediction_amd.common import evaluation
from relation_query_reference import (energy_order_ranks, float64_relation_energies, known_relation_lists,
                                      relation_ranks_from_energies)
from topk_reference import topk_from_energies


# ------------------------------------------------------------------ the reference on hand-made energies
def test_reference_ranks_on_hand_made_energies():
    energies = np.array([[3.0, 1.0, 3.0, -2.0, 0.5],        # the gold (2) ties with relation 0
                         [20.0, 30.0, 18.0, 1.0, 40.0],     # 18, 20, 30 and 40 saturate to 1.0f and tie
                         [-200.0, -150.0, 0.0, -300.0, 1.0],  # the gold's score is 0: everything ties with it
                         [0.0, -0.0, 1.0, 2.0, 3.0]], dtype=np.float32)
    gold = [2, 2, 3, 1]
    lists = [[2], [2, 4], [3, 0, 1], [1, 0, 4]]
    raw, filtered = relation_ranks_from_energies(energies, gold, lists)
    assert raw.dtype == np.int32 and filtered.dtype == np.int32
    assert raw.tolist() == [2, 4, 5, 5]                     # row 3: sigmoid(-0.0) == sigmoid(0.0)
    assert filtered.tolist() == [2, 3, 3, 3]                # the gold inside its list leaves the + 1
    assert energy_order_ranks(energies, gold).tolist() == [2, 4, 5, 5]
    assert energy_order_ranks(energies[1:2], [2]).tolist() == [4]
    # the saturated ties change the rank where the gold is the LOWEST of the saturated energies' betters
    assert relation_ranks_from_energies(energies[1:2], [0], [[0]])[0].tolist() == [4]
    assert energy_order_ranks(energies[1:2], [0]).tolist() == [3]


def test_reference_selection_with_ties_and_short_rows():
    row = np.array([1.0, 2.0, 2.0, -0.0, 0.0, 2.0], dtype=np.float32)
    idx, energy = topk_from_energies(row, 2)
    assert idx.tolist() == [1, 2] and energy.tolist() == [2.0, 2.0]                  # ties go to the lowest ids
    idx, energy = topk_from_energies(row, 4, [1, 1, 0])
    assert idx.tolist() == [2, 5, 4, 3]                                              # +0.0 before -0.0
    idx, energy = topk_from_energies(row, 4, [0, 1, 2, 5, 5])                        # fewer than k are left
    assert idx.tolist() == [4, 3, -1, -1] and np.isneginf(energy[2:]).all()
    assert np.signbit(energy[1]) and not np.signbit(energy[0])


def test_reference_energies_and_their_bound():
    rng = np.random.RandomState(0)
    V, R, d = 7, 3, 5
    codes, w_rel = rng.randn(V, d).astype(np.float32), rng.randn(V, d).astype(np.float32)
    queries = np.array([[0, -1, 1], [2, 9, 2], [6, 0, 3]])                           # the r column is not read
    E64, bound = float64_relation_energies(codes, w_rel, queries, R)
    assert E64.shape == bound.shape == (3, R) and E64.dtype == np.float64
    for i, (s, _, o) in enumerate(queries):
        for r in range(R):
            terms = [float(codes[s, k]) * float(codes[o, k]) * float(w_rel[r, k]) for k in range(d)]
            assert abs(E64[i, r] - sum(terms)) < 1e-12
            assert abs(bound[i, r] - (d + 2) * 2.0 ** -24 * sum(abs(t) for t in terms)) < 1e-18
    # the fp32 path itself stays inside the bound
    p32 = codes[queries[:, 0]] * codes[queries[:, 2]]
    assert (np.abs((p32 @ w_rel[:R].T).astype(np.float64) - E64) <= bound).all()


# ------------------------------------------------------------------ Scorer
TRIPLES = np.array([[0, 0, 1], [0, 1, 1], [0, 0, 1], [3, 1, 0], [2, 0, 1], [1, 2, 0]])


def test_register_data_fills_known_relation_triples_and_leaves_the_other_dictionaries():
    scorer = evaluation.Scorer({'Metric': 'MRR'})
    scorer.register_data(TRIPLES)
    assert scorer.known_relation_triples == {(0, 1): [0, 1], (3, 0): [1], (2, 1): [0], (1, 0): [2]}
    assert scorer.known_relation_triples == known_relation_lists(TRIPLES)
    assert scorer.known_object_triples == {(0, 0): [1], (0, 1): [1], (3, 1): [0], (2, 0): [1], (1, 2): [0]}
    assert scorer.known_subject_triples == {(1, 0): [0, 2], (1, 1): [0], (0, 1): [3], (0, 2): [1]}
    assert scorer.relation_freqs == {0: 3, 1: 2, 2: 1}
    scorer.register_data(np.array([[0, 2, 1], [0, 0, 1]]))                           # a second split extends the lists
    assert scorer.known_relation_triples[(0, 1)] == [0, 1, 2]
    ptr, idx = evaluation.known_completions_csr([(0, 1), (1, 1), (3, 0)], scorer.known_relation_triples)
    assert ptr.tolist() == [0, 3, 3, 4] and idx.tolist() == [0, 1, 2, 1] and idx.dtype == np.int32


class FakeRankModel(object):
    """device_relation_ranks stand-in: scripted ranks, one per triple, handed out in order"""

    def __init__(self, raw, filtered):
        self.raw, self.filtered = np.asarray(raw), np.asarray(filtered)
        self.test_graph = "graph"
        self.calls, self.at = [], 0

    def device_relation_ranks(self, graph, triples, ptr, idx):
        self.calls.append((graph, np.array(triples), np.array(ptr), np.array(idx)))
        sl = slice(self.at, self.at + len(triples))
        self.at += len(triples)
        return self.raw[sl].astype(np.int32), self.filtered[sl].astype(np.int32)

    def device_ranks(self, *args):
        raise AssertionError("the relation evaluation asks no entity-side ranks")


def test_compute_relation_mrr_scores_with_scripted_ranks():
    scorer = evaluation.Scorer({'Metric': 'MRR'})
    scorer.register_data(TRIPLES)
    scorer.register_degrees(TRIPLES)
    scorer.finalize_frequency_computation(TRIPLES)
    test = np.array([[0, 0, 1], [3, 1, 0], [2, 0, 1], [1, 2, 0], [0, 1, 1]])
    model = FakeRankModel(raw=[1, 2, 4, 3, 10], filtered=[1, 1, 2, 3, 5])
    scorer.register_model(model)
    scorer.chunk_size = 2                                                            # chunks of 2, 2 and 1
    score = scorer.compute_relation_mrr_scores(test)
    assert isinstance(score, evaluation.MrrScore) and score.pointer == len(test)     # one line per triple
    assert [len(c[1]) for c in model.calls] == [2, 2, 1] and all(c[0] == "graph" for c in model.calls)
    assert np.array_equal(np.concatenate([c[1] for c in model.calls]), test)
    # the filter lists: the relations known for each pair, the gold one among them
    assert model.calls[0][2].tolist() == [0, 2, 3] and model.calls[0][3].tolist() == [0, 1, 1]
    assert model.calls[2][2].tolist() == [0, 2] and model.calls[2][3].tolist() == [0, 1]
    results = score.get_summary().results
    assert results['Raw']['MRR'] == pytest.approx(np.mean([1, 1 / 2, 1 / 4, 1 / 3, 1 / 10]))
    assert results['Filtered']['MRR'] == pytest.approx(np.mean([1, 1, 1 / 2, 1 / 3, 1 / 5]))
    assert results['Raw']['H@1'] == pytest.approx(1 / 5) and results['Raw']['H@3'] == pytest.approx(3 / 5)
    assert results['Raw']['H@10'] == pytest.approx(1.0)
    assert results['Filtered']['H@1'] == pytest.approx(2 / 5) and results['Filtered']['H@3'] == pytest.approx(4 / 5)
    # per-line columns: degrees and vertex frequency of the SUBJECT, frequency of the gold relation
    subjects = test[:, 0]
    assert score.in_degree[:5].tolist() == [scorer.in_degree[int(v)] for v in subjects]
    assert score.out_degree[:5].tolist() == [scorer.out_degree[int(v)] for v in subjects]
    assert score.in_degree[:5].tolist() == [2, 0, 0, 4, 2] and score.out_degree[:5].tolist() == [3, 1, 1, 1, 3]
    assert score.vertex_freq[:5].tolist() == [scorer.avg_freq[int(v)] for v in subjects]
    assert score.relation_freq[:5].tolist() == [3, 2, 3, 1, 2]
    assert score.raw_ranks[:5].tolist() == [1, 2, 4, 3, 10] and score.filtered_ranks[:5].tolist() == [1, 1, 2, 3, 5]


def test_compute_scores_does_not_change():
    class EntityOnly(FakeRankModel):
        def device_relation_ranks(self, *args):
            raise AssertionError("compute_scores asks no relation ranks")

        def device_ranks(self, graph, triples, predict_object, ptr, idx):
            self.calls.append(predict_object)
            return np.ones(len(triples), np.int32), np.ones(len(triples), np.int32)
    scorer = evaluation.Scorer({'Metric': 'MRR'})
    scorer.register_data(TRIPLES)
    scorer.register_degrees(TRIPLES)
    scorer.finalize_frequency_computation(TRIPLES)
    model = EntityOnly([], [])
    scorer.register_model(model)
    score = scorer.compute_scores(TRIPLES[:3])
    assert model.calls == [False, True] and score.pointer == 6


# ------------------------------------------------------------------ the command
class FakeRelationModel(object):
    """device_relation_topk stand-in: the reference selection on a fixed energy table indexed by (subject, object)"""

    def __init__(self, V, R):
        self.table = np.random.RandomState(3).randn(V, V, R).astype(np.float32)
        self.test_graph = "graph"
        self.loaded, self.calls = None, []

    def load(self, path):
        self.loaded = path

    def device_topk(self, *args):
        raise AssertionError("--side relation asks no entity-side top-k")

    def device_relation_topk(self, graph, queries, k, ptr, idx):
        self.calls.append((graph, np.array(queries), k, ptr, idx))
        out_i, out_e = np.empty((len(queries), k), np.int32), np.empty((len(queries), k), np.float32)
        for i, (s, r, o) in enumerate(queries):
            excluded = idx[ptr[i]:ptr[i + 1]] if ptr is not None else ()
            out_i[i], out_e[i] = topk_from_energies(self.table[s, o], k, excluded)
        return out_i, out_e


@pytest.fixture
def dataset(tmp_path):
    names = ["a", "b", "c", "d", "e"]
    (tmp_path / "entities.dict").write_text("".join("%d\t%s\n" % (i, n) for i, n in enumerate(names)))
    (tmp_path / "relations.dict").write_text("0\tr\n1\tq\n2\tp\n")
    (tmp_path / "train.txt").write_text("a\tr\tb\na\tq\tb\nb\tq\tc\na\tr\tb\n")
    (tmp_path / "valid.txt").write_text("a\tp\tb\n")
    (tmp_path / "test.txt").write_text("c\tq\ta\n")
    (tmp_path / "s.exp").write_text("[Encoder]\n\tName=gcn_basis\n\n[Decoder]\n\tName=bilinear-diag\n\n[Shared]\n\n"
                                    "[Optimizer]\n\n[General]\n\n[Evaluation]\n\tMetric=MRR\n")
    (tmp_path / "q.txt").write_text("c\ta\n\nb\tc\nd\te\n")
    return tmp_path


def run(dataset, monkeypatch, capsys, *extra):
    model = FakeRelationModel(5, 3)
    built = []

    def fake_build(settings, splits, n_entities, n_relations):
        built.append((n_entities, n_relations, len(splits['train'])))
        return model
    monkeypatch.setattr(predict, "build_model", fake_build)
    argv = ["--settings", str(dataset / "s.exp"), "--dataset", str(dataset), "--model", "ckpt.npz",
            "--queries", str(dataset / "q.txt"), "--side", "relation"] + list(extra)
    result = predict.main(argv)
    return model, built, capsys.readouterr().out, result


def test_predict_side_relation_maps_names_excludes_known_and_formats_lines(dataset, monkeypatch, capsys):
    model, built, out, (top, scores) = run(dataset, monkeypatch, capsys, "--k", "2")
    assert built == [(5, 3, 4)] and model.loaded == "ckpt.npz"
    graph, queries, k, ptr, idx = model.calls[0]
    assert graph == "graph" and k == 2
    assert queries.tolist() == [[2, -1, 0], [1, -1, 2], [3, -1, 4]]    # the blank line is skipped, the relation unread
    assert ptr.tolist() == [0, 1, 2, 2] and idx.tolist() == [1, 1]     # (c, a): q from test; (b, c): q from train
    lines = [l.split("\t") for l in out.splitlines()]
    assert len(lines) == 6 and all(len(l) == 5 for l in lines)
    assert [(l[0], l[2]) for l in lines] == [("c", "a")] * 2 + [("b", "c")] * 2 + [("d", "e")] * 2
    assert [l[3] for l in lines] == ["1", "2"] * 3
    names = ["r", "q", "p"]
    for (s, o), rows in (((2, 0), lines[:2]), ((3, 4), lines[4:])):
        want_ids, want_e = topk_from_energies(model.table[s, o], 2, [1] if s == 2 else [])
        assert [l[1] for l in rows] == [names[i] for i in want_ids]
        for l, e in zip(rows, want_e):                                 # fp32 sigmoid, rounded once from double
            assert np.float32(l[4]) == np.float32(1.0 / (1.0 + np.exp(-np.float64(e))))
    assert top.shape == scores.shape == (3, 2) and scores.dtype == np.float32


def test_predict_side_relation_short_rows_keep_known_and_out_file(dataset, monkeypatch, capsys):
    (dataset / "q.txt").write_text("a\tb\n")                            # r, q (train) and p (valid) are all known
    model, _, out, (top, _) = run(dataset, monkeypatch, capsys, "--k", "3")
    assert model.calls[0][3].tolist() == [0, 3] and sorted(model.calls[0][4].tolist()) == [0, 1, 2]
    assert out == "" and (top == -1).all()                             # nothing is left to answer
    model, _, out, _ = run(dataset, monkeypatch, capsys, "--k", "3", "--keep-known", "--out", str(dataset / "answers.txt"))
    assert model.calls[0][3] is None and model.calls[0][4] is None and out == ""
    lines = (dataset / "answers.txt").read_text().splitlines()
    assert len(lines) == 3 and [l.split("\t")[3] for l in lines] == ["1", "2", "3"]
    assert sorted(l.split("\t")[1] for l in lines) == ["p", "q", "r"]


def test_predict_side_relation_refuses_bad_queries_k_and_the_ensemble(dataset, monkeypatch, capsys):
    (dataset / "q.txt").write_text("a\tb\nzz\tb\n")
    with pytest.raises(ValueError, match="line 2.*zz"):
        run(dataset, monkeypatch, capsys, "--k", "2")
    (dataset / "q.txt").write_text("a\tb\n\na\tnope\n")
    with pytest.raises(ValueError, match="line 3.*nope"):
        run(dataset, monkeypatch, capsys, "--k", "2")
    (dataset / "q.txt").write_text("a\tr\n")                            # a relation name is no entity
    with pytest.raises(ValueError, match="line 1.*'r'"):
        run(dataset, monkeypatch, capsys, "--k", "2")
    for text in ("a\tr\tb\n", "a\n"):
        (dataset / "q.txt").write_text(text)
        with pytest.raises(ValueError, match="line 1.*subject<TAB>object"):
            run(dataset, monkeypatch, capsys, "--k", "2")
    (dataset / "q.txt").write_text("a\tb\n")

    def no_device(*a):
        raise AssertionError("the model was built for a call that cannot be answered")
    monkeypatch.setattr(predict, "build_model", no_device)
    base = ["--settings", str(dataset / "s.exp"), "--dataset", str(dataset), "--model", "ckpt.npz",
            "--queries", str(dataset / "q.txt"), "--side", "relation"]
    for k in ("4", "0"):                                               # three relations (five entities)
        with pytest.raises(ValueError, match="--k.*relations"):
            predict.main(base + ["--k", k])
    with pytest.raises(ValueError, match="--side relation"):
        predict.main(base + ["--k", "2", "--settings2", str(dataset / "s.exp"), "--model2", "other.npz"])
