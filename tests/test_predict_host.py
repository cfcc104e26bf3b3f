"""Host side of top-k prediction: the numpy reference of the selection, the exclusion-CSR helper and the command line
(relationprediction_amd.predict) driven with a fake model.  No GPU."""
import numpy as np
import pytest

from relationprediction_amd import predict
from relationprediction_amd.common import evaluation
from topk_reference import float_key, topk_from_energies


# ------------------------------------------------------------------ the reference of the selection
def brute_force(row, k, excluded):
    def before(a, b):                      # does entry a come before entry b?  (energy descending, id ascending)
        xa, xb = float(row[a]), float(row[b])
        if xa != xb:
            return xa > xb
        sa, sb = np.signbit(row[a]), np.signbit(row[b])
        if sa != sb:                       # +0.0 before -0.0
            return sb
        return a < b
    ids = [e for e in range(len(row)) if e not in set(excluded)]
    for i in range(1, len(ids)):           # insertion sort by the comparison above
        j = i
        while j > 0 and before(ids[j], ids[j - 1]):
            ids[j], ids[j - 1] = ids[j - 1], ids[j]
            j -= 1
    return ids[:k]


def test_reference_selection_against_a_brute_force_sort():
    rng = np.random.RandomState(0)
    for trial in range(30):
        V = int(rng.randint(1, 60))
        row = rng.randint(-3, 4, size=V).astype(np.float32)            # forced ties
        row[rng.rand(V) < 0.2] = -0.0
        row[rng.rand(V) < 0.1] = 0.0
        if trial % 3 == 0:
            row[rng.randint(0, V)] = np.inf
            row[rng.randint(0, V)] = -np.inf
        excluded = list(rng.randint(0, V, size=rng.randint(0, V + 1)))
        k = int(rng.randint(1, V + 3))
        idx, energy = topk_from_energies(row, k, excluded)
        want = brute_force(row, k, excluded)
        assert idx.dtype == np.int32 and energy.dtype == np.float32 and idx.shape == energy.shape == (k,)
        assert idx[:len(want)].tolist() == want
        assert (idx[len(want):] == -1).all() and np.isneginf(energy[len(want):]).all()
        assert np.array_equal(energy[:len(want)].view(np.uint32), row[want].view(np.uint32))
    keys = float_key(np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32).view(np.uint32))
    assert (np.diff(keys.astype(np.int64)) > 0).all()                  # numeric order, -0.0 below +0.0


# ------------------------------------------------------------------ exclusion lists
def test_known_completions_csr_against_hand_built_dictionaries():
    triples = np.array([[0, 0, 1], [0, 0, 2], [0, 0, 1], [3, 1, 0], [2, 0, 1]])
    scorer = evaluation.Scorer({'Metric': 'MRR'})
    scorer.register_data(triples)
    assert scorer.known_object_triples == {(0, 0): [1, 2], (3, 1): [0], (2, 0): [1]}
    assert scorer.known_subject_triples == {(1, 0): [0, 2], (2, 0): [0], (0, 1): [3]}
    ptr, idx = evaluation.known_completions_csr([(0, 0), (4, 0), (3, 1), (0, 0)], scorer.known_object_triples)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32
    assert ptr.tolist() == [0, 2, 2, 3, 5] and idx.tolist() == [1, 2, 0, 1, 2]       # (4, 0): nothing known
    ptr, idx = evaluation.known_completions_csr(np.array([[1, 0], [0, 1], [1, 1]]), scorer.known_subject_triples)
    assert ptr.tolist() == [0, 2, 3, 3] and idx.tolist() == [0, 2, 3]
    ptr, idx = evaluation.known_completions_csr([], scorer.known_object_triples)
    assert ptr.tolist() == [0] and idx.shape == (0,) and idx.dtype == np.int32


# ------------------------------------------------------------------ the command
class FakePredictModel(object):
    """device_topk stand-in: the reference selection on a fixed energy table indexed by the fixed entity"""

    def __init__(self, V):
        self.V = V
        self.table = np.random.RandomState(3).randn(V, V).astype(np.float32)
        self.test_graph = "graph"
        self.loaded, self.calls = None, []

    def load(self, path):
        self.loaded = path

    def device_topk(self, graph, queries, predict_object, k, ptr, idx):
        self.calls.append((graph, np.array(queries), predict_object, k, ptr, idx))
        out_i, out_e = np.empty((len(queries), k), np.int32), np.empty((len(queries), k), np.float32)
        for i, (s, r, o) in enumerate(queries):
            row = self.table[s if predict_object else o] + np.float32(r)
            excluded = idx[ptr[i]:ptr[i + 1]] if ptr is not None else ()
            out_i[i], out_e[i] = topk_from_energies(row, k, excluded)
        return out_i, out_e


@pytest.fixture
def dataset(tmp_path):
    names = ["a", "b", "c", "d", "e"]
    (tmp_path / "entities.dict").write_text("".join("%d\t%s\n" % (i, n) for i, n in enumerate(names)))
    (tmp_path / "relations.dict").write_text("0\tr\n1\tq\n")
    (tmp_path / "train.txt").write_text("a\tr\tb\na\tr\tc\nb\tq\tc\n")
    (tmp_path / "valid.txt").write_text("a\tr\td\n")
    (tmp_path / "test.txt").write_text("e\tq\ta\n")
    (tmp_path / "s.exp").write_text("[Encoder]\n\tName=gcn_basis\n\n[Decoder]\n\tName=bilinear-diag\n\n[Shared]\n\n"
                                    "[Optimizer]\n\n[General]\n\n[Evaluation]\n\tMetric=MRR\n")
    (tmp_path / "q.txt").write_text("a\tr\n\nc\tq\n")
    return tmp_path


def run(dataset, monkeypatch, capsys, *extra):
    model = FakePredictModel(5)
    built = []

    def fake_build(settings, splits, n_entities, n_relations):
        built.append((n_entities, n_relations, len(splits['train'])))
        return model
    monkeypatch.setattr(predict, "build_model", fake_build)
    argv = ["--settings", str(dataset / "s.exp"), "--dataset", str(dataset), "--model", "ckpt.npz",
            "--queries", str(dataset / "q.txt")] + list(extra)
    predict.main(argv)
    return model, built, capsys.readouterr().out


def test_predict_command_maps_names_excludes_known_and_formats_lines(dataset, monkeypatch, capsys):
    model, built, out = run(dataset, monkeypatch, capsys, "--k", "3")
    assert built == [(5, 2, 3)] and model.loaded == "ckpt.npz"
    graph, queries, predict_object, k, ptr, idx = model.calls[0]
    assert graph == "graph" and predict_object is True and k == 3
    assert queries.tolist() == [[0, 0, -1], [2, 1, -1]]                # the blank line is skipped, the object unread
    assert ptr.tolist() == [0, 3, 3] and idx.tolist() == [1, 2, 3]     # (a, r): b, c from train and d from valid
    lines = [l.split("\t") for l in out.splitlines()]
    assert len(lines) == 2 + 3 and all(len(l) == 5 for l in lines)     # (a, r, ?) has only a and e left
    assert [l[:2] for l in lines] == [["a", "r"]] * 2 + [["c", "q"]] * 3
    assert [l[3] for l in lines] == ["1", "2", "1", "2", "3"]
    names = ["a", "b", "c", "d", "e"]
    want_ids, want_e = topk_from_energies(model.table[0], 3, [1, 2, 3])
    assert [l[2] for l in lines[:2]] == [names[i] for i in want_ids[:2]]
    for l, e in zip(lines[:2], want_e[:2]):                            # fp32 sigmoid, rounded once from double
        assert np.float32(l[4]) == np.float32(1.0 / (1.0 + np.exp(-np.float64(e))))
    assert [float(l[4]) for l in lines[2:]] == sorted((float(l[4]) for l in lines[2:]), reverse=True)


def test_predict_command_sides_keep_known_and_out_file(dataset, monkeypatch, capsys):
    model, _, out = run(dataset, monkeypatch, capsys, "--k", "2", "--side", "subject")
    graph, queries, predict_object, k, ptr, idx = model.calls[0]
    assert predict_object is False and queries.tolist() == [[-1, 0, 0], [-1, 1, 2]]
    assert ptr.tolist() == [0, 0, 1] and idx.tolist() == [1]           # (?, q, c): b is known; (?, r, a): nothing
    assert len(out.splitlines()) == 4
    model, _, out = run(dataset, monkeypatch, capsys, "--k", "5", "--keep-known", "--out", str(dataset / "answers.txt"))
    assert model.calls[0][4] is None and model.calls[0][5] is None and out == ""
    lines = (dataset / "answers.txt").read_text().splitlines()
    assert len(lines) == 10 and lines[0].split("\t")[3] == "1"


def test_predict_command_refuses_unknown_names_and_a_k_above_the_entity_count(dataset, monkeypatch, capsys):
    (dataset / "q.txt").write_text("a\tr\nzz\tr\n")
    with pytest.raises(ValueError, match="line 2.*zz"):
        run(dataset, monkeypatch, capsys, "--k", "2")
    (dataset / "q.txt").write_text("a\tr\n\na\tnope\n")
    with pytest.raises(ValueError, match="line 3.*nope"):
        run(dataset, monkeypatch, capsys, "--k", "2")
    (dataset / "q.txt").write_text("a\tr\tb\n")
    with pytest.raises(ValueError, match="line 1"):
        run(dataset, monkeypatch, capsys, "--k", "2")
    (dataset / "q.txt").write_text("a\tr\n")

    def no_device(*a):
        raise AssertionError("the model was built for a k that cannot be answered")
    monkeypatch.setattr(predict, "build_model", no_device)
    for k in ("6", "0"):
        with pytest.raises(ValueError, match="--k"):
            predict.main(["--settings", str(dataset / "s.exp"), "--dataset", str(dataset), "--model", "ckpt.npz",
                          "--queries", str(dataset / "q.txt"), "--k", k])
