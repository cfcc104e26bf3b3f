"""The ensemble arguments of the prediction command (relationprediction_amd.predict --settings2 --model2 --weight) driven
with fake models: argument pairing and range, the one-GPU check, chunking at Scorer.chunk_size, the order of the two
models' calls, name mapping, exclusion and line format -- and that without the new arguments the command calls
device_topk exactly as before.  No GPU."""
import numpy as np
import pytest

import embedding_reference as er
from relationprediction_amd import predict
from relationprediction_amd.common import evaluation
from test_predict_host import FakePredictModel, dataset          # noqa: F401  (dataset is a fixture)
from topk_mixed_reference import mixed_topk

NAMES = ["a", "b", "c", "d", "e"]
LOG = []


class FakeEngine(object):
    def __init__(self, owner, device):
        self.owner = owner
        self.cfg = type("Cfg", (), {"device": device})()

    def rank_energies_device(self):
        LOG.append(("address", self.owner.name))
        return self.owner


class FakeRuntime(object):
    def __init__(self, engine):
        self.engine = engine


class FakeEnsembleModel(FakePredictModel):
    """device_score_queries keeps the energies of the chunk it was handed; device_topk_mixed reads them from the partner
    it is given (the other fake, standing in for the device address of its buffer) and selects with the reference"""

    def __init__(self, name, V, seed, device=0):
        super().__init__(V)
        self.name = name
        self.table = np.random.RandomState(seed).randn(V, V).astype(np.float32)
        self.runtime = FakeRuntime(FakeEngine(self, device))
        self.scored = None

    def load(self, path):
        LOG.append(("load", self.name, path))
        self.loaded = path

    def get_runtime(self):
        return self.runtime

    def energies(self, queries, predict_object):
        return np.stack([self.table[s if predict_object else o] + np.float32(r) for s, r, o in queries])

    def device_score_queries(self, graph, queries, predict_object):
        LOG.append(("score", self.name, graph, np.array(queries), predict_object))
        self.scored = self.energies(queries, predict_object)

    def device_topk_mixed(self, graph, queries, predict_object, k, partner, weight, ptr, idx):
        LOG.append(("topk_mixed", self.name, graph, np.array(queries), predict_object, k, partner.name, weight,
                    None if ptr is None else np.array(ptr), None if idx is None else np.array(idx)))
        assert partner.scored.shape == (len(queries), self.V)            # the partner scored THIS chunk
        m = er.mixed_scores(self.energies(queries, predict_object), partner.scored, weight).astype(np.float32)
        out_i, out_s = np.empty((len(queries), k), np.int32), np.empty((len(queries), k), np.float32)
        for i in range(len(queries)):
            out_i[i], out_s[i] = mixed_topk(m[i], k, idx[ptr[i]:ptr[i + 1]] if ptr is not None else ())
        return out_i, out_s

    def device_topk(self, *args):
        LOG.append(("topk", self.name))
        return super().device_topk(*args)


def run(dataset, monkeypatch, capsys, *extra, devices=(0, 0)):
    del LOG[:]
    models = [FakeEnsembleModel("first", 5, 3, devices[0]), FakeEnsembleModel("second", 5, 4, devices[1])]
    built = []

    def fake_build(settings, splits, n_entities, n_relations):
        built.append(settings)
        return models[len(built) - 1]
    monkeypatch.setattr(predict, "build_model", fake_build)
    (dataset / "s2.exp").write_text((dataset / "s.exp").read_text().replace("gcn_basis", "embedding"))
    argv = ["--settings", str(dataset / "s.exp"), "--dataset", str(dataset), "--model", "ckpt.npz",
            "--queries", str(dataset / "q.txt")] + list(extra)
    result = predict.main(argv)
    return models, built, capsys.readouterr().out, result


def ensemble_args(dataset, *more):
    return ("--settings2", str(dataset / "s2.exp"), "--model2", "ckpt2.npz") + more


def test_argument_pairing_and_weight_range(dataset, monkeypatch, capsys):
    def no_model(*a):
        raise AssertionError("a model was built for arguments that cannot be answered")
    (dataset / "s2.exp").write_text((dataset / "s.exp").read_text())
    base = ["--settings", str(dataset / "s.exp"), "--dataset", str(dataset), "--model", "ckpt.npz", "--queries",
            str(dataset / "q.txt"), "--k", "2"]
    monkeypatch.setattr(predict, "build_model", no_model)
    with pytest.raises(ValueError, match="come together"):
        predict.main(base + ["--settings2", str(dataset / "s2.exp")])
    with pytest.raises(ValueError, match="come together"):
        predict.main(base + ["--model2", "ckpt2.npz"])
    with pytest.raises(ValueError, match="--weight"):
        predict.main(base + ["--weight", "0.5"])                          # a weight with nothing to weigh
    for w in ("-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match="--weight"):
            predict.main(base + list(ensemble_args(dataset, "--weight", w)))


def test_the_two_models_must_sit_on_one_gpu(dataset, monkeypatch, capsys):
    with pytest.raises(ValueError, match=r"one GPU \(Device 0 and 1\)"):
        run(dataset, monkeypatch, capsys, "--k", "2", *ensemble_args(dataset), devices=(0, 1))
    assert not [e for e in LOG if e[0] in ("score", "topk_mixed", "topk")]


def test_ensemble_maps_names_excludes_known_and_formats_lines(dataset, monkeypatch, capsys):
    models, built, out, _ = run(dataset, monkeypatch, capsys, "--k", "3", *ensemble_args(dataset))
    first, second = models
    assert [s['Encoder']['Name'] for s in built] == ["gcn_basis", "embedding"]          # each from its own settings file
    assert [e[:3] for e in LOG if e[0] == "load"] == [("load", "first", "ckpt.npz"), ("load", "second", "ckpt2.npz")]
    calls = [e for e in LOG if e[0] in ("score", "address", "topk_mixed", "topk")]
    assert [e[:2] for e in calls] == [("score", "second"), ("address", "second"), ("topk_mixed", "first")]
    _, _, graph, queries, predict_object = calls[0]
    assert graph == "graph" and predict_object is True and queries.tolist() == [[0, 0, -1], [2, 1, -1]]
    _, _, graph, queries, predict_object, k, partner, weight, ptr, idx = calls[2]
    assert graph == "graph" and predict_object is True and k == 3 and partner == "second" and weight == 0.5   # the default
    assert queries.tolist() == [[0, 0, -1], [2, 1, -1]]
    assert ptr.tolist() == [0, 3, 3] and idx.tolist() == [1, 2, 3]     # (a, r): b, c from train and d from valid
    lines = [l.split("\t") for l in out.splitlines()]
    assert len(lines) == 2 + 3 and all(len(l) == 5 for l in lines)     # (a, r, ?) has only a and e left
    assert [l[:2] for l in lines] == [["a", "r"]] * 2 + [["c", "q"]] * 3
    assert [l[3] for l in lines] == ["1", "2", "1", "2", "3"]
    m = er.mixed_scores(first.table[[0, 2]] + np.float32([[0], [1]]), second.table[[0, 2]] + np.float32([[0], [1]]),
                        0.5).astype(np.float32)
    want = [mixed_topk(m[0], 3, [1, 2, 3]), mixed_topk(m[1], 3)]
    assert [l[2] for l in lines] == [NAMES[i] for i in want[0][0][:2]] + [NAMES[i] for i in want[1][0]]
    assert [l[4] for l in lines] == ["%.9g" % s for s in want[0][1][:2]] + ["%.9g" % s for s in want[1][1]]


def test_ensemble_sides_weight_keep_known_and_out_file(dataset, monkeypatch, capsys):
    models, _, out, _ = run(dataset, monkeypatch, capsys, "--k", "2", "--side", "subject", "--weight", "0.25",
                            *ensemble_args(dataset))
    score, mixed = [e for e in LOG if e[0] == "score"][0], [e for e in LOG if e[0] == "topk_mixed"][0]
    assert score[4] is False and score[3].tolist() == [[-1, 0, 0], [-1, 1, 2]]
    assert mixed[4] is False and mixed[7] == 0.25 and mixed[8].tolist() == [0, 0, 1] and mixed[9].tolist() == [1]
    assert len(out.splitlines()) == 4
    models, _, out, _ = run(dataset, monkeypatch, capsys, "--k", "5", "--keep-known", "--out", str(dataset / "answers.txt"),
                            *ensemble_args(dataset, "--weight", "1"))
    mixed = [e for e in LOG if e[0] == "topk_mixed"][0]
    assert mixed[7] == 1.0 and mixed[8] is None and mixed[9] is None and out == ""
    lines = (dataset / "answers.txt").read_text().splitlines()
    assert len(lines) == 10 and lines[0].split("\t")[3] == "1"


def test_queries_are_taken_in_chunks_and_model_two_scores_each_chunk_first(dataset, monkeypatch, capsys):
    monkeypatch.setattr(evaluation.Scorer, "chunk_size", 3)
    pairs = [("a", "r"), ("c", "q"), ("b", "q"), ("a", "r"), ("e", "q"), ("d", "r"), ("b", "r")]
    (dataset / "q.txt").write_text("".join("%s\t%s\n" % p for p in pairs))
    models, _, out, (top, scores) = run(dataset, monkeypatch, capsys, "--k", "2", *ensemble_args(dataset))
    calls = [e for e in LOG if e[0] in ("score", "address", "topk_mixed")]
    assert [e[:2] for e in calls] == [("score", "second"), ("address", "second"), ("topk_mixed", "first")] * 3
    assert [len(e[3]) for e in calls if e[0] == "score"] == [3, 3, 1]
    for s, t in zip([e for e in calls if e[0] == "score"], [e for e in calls if e[0] == "topk_mixed"]):
        assert np.array_equal(s[3], t[3])                                  # the same queries, in the same order
    # each chunk's exclusion CSR starts at 0 and holds that chunk's lists only
    ids = {n: i for i, n in enumerate(NAMES)}
    known = {}
    for part in ("train", "valid", "test"):
        rows = [l.split("\t") for l in (dataset / (part + ".txt")).read_text().splitlines()]
        evaluation.Scorer.extend_triple_dict(known, [(ids[s], {"r": 0, "q": 1}[r], ids[o]) for s, r, o in rows], object_list=True)
    keys = [(ids[e], {"r": 0, "q": 1}[r]) for e, r in pairs]
    for n, t in enumerate(e for e in calls if e[0] == "topk_mixed"):
        ptr, idx = evaluation.known_completions_csr(keys[3 * n:3 * n + 3], known)
        assert t[8].tolist() == ptr.tolist() and t[9].tolist() == idx.tolist()
    # ... and the answers are the ones one call over all queries gives
    first, second = models
    q = np.array([[k[0], k[1], -1] for k in keys])
    m = er.mixed_scores(first.energies(q, True), second.energies(q, True), 0.5).astype(np.float32)
    ptr, idx = evaluation.known_completions_csr(keys, known)
    for i in range(len(keys)):
        want = mixed_topk(m[i], 2, idx[ptr[i]:ptr[i + 1]])
        assert np.array_equal(top[i], want[0]) and np.array_equal(scores[i].view(np.uint32), want[1].view(np.uint32))
    assert len(out.splitlines()) == int((top >= 0).sum())


def test_without_the_new_arguments_the_command_calls_device_topk_as_before(dataset, monkeypatch, capsys):
    models, built, out, _ = run(dataset, monkeypatch, capsys, "--k", "3")
    assert len(built) == 1 and [e[:2] for e in LOG if e[0] != "load"] == [("topk", "first")]
    graph, queries, predict_object, k, ptr, idx = models[0].calls[0]
    assert graph == "graph" and predict_object is True and k == 3 and queries.tolist() == [[0, 0, -1], [2, 1, -1]]
    assert ptr.tolist() == [0, 3, 3] and idx.tolist() == [1, 2, 3]
    plain = FakePredictModel(5)
    plain.table = models[0].table
    monkeypatch.setattr(predict, "build_model", lambda *a: plain)
    predict.main(["--settings", str(dataset / "s.exp"), "--dataset", str(dataset), "--model", "ckpt.npz", "--queries",
                  str(dataset / "q.txt"), "--k", "3"])
    assert capsys.readouterr().out == out and len(out.splitlines()) == 5
