"""[General] TypeConstrainedNegatives=Yes and [Evaluation] TypeConstrained=Yes through the training driver, and
`predict --type-constrained`, on the toy dataset of tests/test_gpu_driver.py written to tmp_path: relation r maps entity e
to (a_r e + b_r) mod 200, about 117 training triples per relation, so a relation's subjects and objects are each about half
of the entities."""
import io
import os

import numpy as np
import pytest

from test_gpu_driver import SETTINGS, write_dataset

pytestmark = pytest.mark.gpu


def _lists(train_triples):
    """{relation: set of subjects}, {relation: set of objects} of the training triples"""
    subjects, objects = {}, {}
    for s, r, o in train_triples.tolist():
        subjects.setdefault(r, set()).add(s)
        objects.setdefault(r, set()).add(o)
    return subjects, objects


def _settings(tmp_path, general="", evaluation=""):
    os.makedirs(str(tmp_path / "models"), exist_ok=True)
    path = tmp_path / "toy.exp"
    text = SETTINGS % dict(nb=4, concat="Yes", exp=str(tmp_path / "models" / "Toy"))
    text = text.replace("GraphBatchSize=300", "GraphBatchSize=300" + general).replace("Metric=MRR", "Metric=MRR" + evaluation)
    path.write_text(text)
    return str(path)


@pytest.mark.parametrize("extra", [[], ["--host-edge-dropout"]], ids=["fused_step", "stand_alone_call"])
def test_train_with_both_keys(tmp_path, capsys, extra):
    """the OPEN count is printed with every validation report, the reports are typed MRRs, the runtime reserved the
    training triples once, and every negative of the last step's decoder batch comes from its relation's list and is not
    the row's own entity"""
    from relationprediction_amd import train
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    settings = _settings(tmp_path, "\n\tTypeConstrainedNegatives=Yes", "\n\tTypeConstrained=Yes")
    np.random.seed(0)
    model, iterations = train.main(["--settings", settings, "--dataset", data, "--max-iterations", "40"] + extra)
    out = capsys.readouterr().out
    assert iterations == 40
    reports = [l for l in out.splitlines() if l.startswith("Type-constrained negative sampling:")]
    checks = [l for l in out.splitlines() if l.startswith("Tested validation score")]
    assert len(reports) == len(checks) == 2 and "MRR" in out and "H@10" in out
    counts = [int(l.split(": ")[1].split()[0]) for l in reports]
    rt = model.get_runtime()
    assert counts[0] <= counts[1] <= rt.negative_typed_open() == model.device_negative_typed_open()
    assert rt._types is not None and np.array_equal(rt._types, train_triples)
    assert getattr(rt, "_typed_on", False) == (not extra)               # the fused step's mode; the other path calls
    N = 300 * 6
    X = rt._dev["X"].download(np.int32, (N, 3))
    subjects, objects = _lists(train_triples)
    src = np.tile(X[:300], (5, 1))
    neg = X[300:]
    changed_s, changed_o = neg[:, 0] != src[:, 0], neg[:, 2] != src[:, 2]
    assert (changed_s ^ changed_o).all() and (neg[:, 1] == src[:, 1]).all()     # one entity, never the row's own
    assert all(int(s) in subjects[int(r)] for s, r in neg[changed_s][:, :2])
    assert all(int(o) in objects[int(r)] for r, o in neg[changed_o][:, 1:])
    # every list of the toy world has dozens of members: no row was open
    assert rt.negative_typed_open() == 0


def test_typed_mrr_and_predict_on_one_checkpoint(tmp_path, capsys):
    """on the checkpoint a short run leaves: typed ranks never exceed the open ranks, rank by rank, so the typed MRR is
    not below the open one; `predict --type-constrained` prints only members of the lists, the plain call does not"""
    from relationprediction_amd import predict, train
    from relationprediction_amd.common import evaluation
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    settings = _settings(tmp_path)
    np.random.seed(0)
    model, _ = train.main(["--settings", settings, "--dataset", data, "--max-iterations", "21"])
    capsys.readouterr()
    splits, entities, relations = train.load_dataset(data)
    summaries, ranks = {}, {}
    for value in ("No", "Yes"):
        scorer = evaluation.Scorer({"Metric": "MRR", "TypeConstrained": value})
        for part in ("train", "valid", "test"):
            scorer.register_data(splits[part])
        scorer.register_degrees(splits["train"])
        scorer.register_model(model)
        scorer.finalize_frequency_computation(np.concatenate([splits[p] for p in ("train", "valid", "test")]))
        if value == "Yes":
            scorer.register_type_sets(splits["train"])
        score = scorer.compute_scores(splits["test"])
        ranks[value] = (score.raw_ranks[:score.pointer].copy(), score.filtered_ranks[:score.pointer].copy())
        summaries[value] = score.get_summary().results
    for which in (0, 1):
        assert (ranks["Yes"][which] <= ranks["No"][which]).all() and (ranks["Yes"][which] >= 1).all()
    assert (ranks["Yes"][0] < ranks["No"][0]).any()
    for name in ("Raw", "Filtered"):
        assert summaries["Yes"][name]["MRR"] >= summaries["No"][name]["MRR"]

    queries = tmp_path / "queries.txt"
    picked = train_triples[:6]                                  # (distinct (s, r) pairs: r is a function of them)
    queries.write_text("".join("e%d\tr%d\n" % (s, r) for s, r, _ in picked))
    checkpoint = str(tmp_path / "models" / "Toy-0.npz")
    subjects, objects = _lists(train_triples)
    answers = {}
    for flag in ([], ["--type-constrained"]):
        sink = io.StringIO()
        predict.main(["--settings", settings, "--dataset", data, "--model", checkpoint, "--queries", str(queries),
                      "--k", "150", "--keep-known"] + flag, out=sink)
        answers[bool(flag)] = [l.split("\t") for l in sink.getvalue().splitlines()]
    typed, plain = answers[True], answers[False]
    assert len(plain) == 6 * 150 and 0 < len(typed) < len(plain)                # most lists hold fewer than 150 entities
    assert all(int(a[2][1:]) in objects[int(a[1][1:])] for a in typed)
    assert not all(int(a[2][1:]) in objects[int(a[1][1:])] for a in plain)
    # the typed answers of a query are the plain answers that are members, in the plain order
    for s, r, _ in picked.tolist():
        mine = [a[2] for a in typed if a[0] == "e%d" % s and a[1] == "r%d" % r]
        theirs = [a[2] for a in plain if a[0] == "e%d" % s and a[1] == "r%d" % r and int(a[2][1:]) in objects[r]]
        assert mine[:len(theirs)] == theirs[:len(mine)] and len(mine) >= len(theirs)
