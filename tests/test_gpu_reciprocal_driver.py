"""[Decoder] ReciprocalRelations=Yes through the training driver and `predict --side subject`, on the toy dataset of
tests/test_gpu_driver.py written to tmp_path (V 200, R 6): device negatives (the fused minibatch step) and host negatives
(the numpy port) run to a checkpoint, and the checkpoint's subject answers are those of W_relation[R + r], reproduced in
float64 from the saved weights."""
import io
import os

import numpy as np
import pytest

from test_gpu_driver import SETTINGS, write_dataset

pytestmark = pytest.mark.gpu

PATHS = {"device": [], "host_negatives": ["--host-negatives", "--batch-workers", "0"]}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_train_and_predict_subjects_with_reciprocal_relations(tmp_path, capsys, path):
    from relationprediction_amd import predict, train
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    os.makedirs(str(tmp_path / "models"))
    exp = str(tmp_path / "models" / "Toy")
    settings = tmp_path / "toy.exp"
    settings.write_text((SETTINGS % dict(nb=4, concat="Yes", exp=exp))
                        .replace("RegularizationParameter=0.01", "RegularizationParameter=0.01\n\tReciprocalRelations=Yes"))
    np.random.seed(0)
    model, iterations = train.main(["--settings", str(settings), "--dataset", data, "--max-iterations", "25"] + PATHS[path])
    out = capsys.readouterr().out
    checks = [l for l in out.splitlines() if l.startswith("Tested validation score")]
    assert iterations == 25 and len(checks) == 1 and 0.0 < float(checks[0].split("Result: ")[1]) <= 1.0
    V, R, n, rate = 200, 6, 300, 5
    N = n * (rate + 2)
    rt = model.get_runtime()
    assert model.reciprocal and rt._reciprocal_want and rt.engine._reciprocal and rt._dec_reserved >= N
    X = rt._dev["X"].download(np.int32, (N, 3))
    known = {tuple(t) for t in train_triples.tolist()}
    assert all(tuple(t) in known for t in X[:n].tolist())
    assert np.array_equal(X[N - n:], X[:n] + np.array([0, R, 0], dtype=np.int32))
    neg, tiled = X[n:N - n], np.tile(X[:n], (rate, 1))
    moved_s, moved_r = neg[:, 0] != tiled[:, 0], neg[:, 1] != tiled[:, 1]
    assert np.array_equal(neg[moved_r][:, 1], tiled[moved_r][:, 1] + R) and 0 < moved_r.sum() < len(neg)
    assert (moved_r | ~moved_s).all()                       # every row with another subject asks the inverse relation
    assert np.array_equal(neg[moved_r][:, 2], tiled[moved_r][:, 2])

    # the checkpoint answers (?, r, o) with W_relation[R + r]
    checkpoint = exp + "-0.npz"
    picked = train_triples[:4]
    queries = tmp_path / "queries.txt"
    queries.write_text("".join("e%d\tr%d\n" % (o, r) for _, r, o in picked))
    sink = io.StringIO()
    top, scores = predict.main(["--settings", str(settings), "--dataset", data, "--model", checkpoint, "--queries",
                                str(queries), "--k", "5", "--side", "subject", "--keep-known"], out=sink)
    assert len(sink.getvalue().splitlines()) == 20
    with np.load(checkpoint) as z:
        W = z[[k for k in z.files if k.endswith("W_relation")][0]].astype(np.float64)
    assert W.shape == (V, 20)
    model.load(checkpoint)
    codes = model._scoring_runtime(model.test_graph).forward('test').codes().astype(np.float64)
    differs = False
    for (_, r, o), ids, row in zip(picked.tolist(), top, scores):
        energy = codes @ (W[R + r] * codes[o])
        score = 1.0 / (1.0 + np.exp(-energy))
        # float32 products of 20 terms on the device: 1e-5 on a sigmoid (slope <= 1/4) is two orders above their rounding
        assert np.abs(score[ids] - row).max() <= 1e-5
        rest = np.delete(energy, ids)
        assert energy[ids].min() >= rest.max() - 1e-4 * max(1.0, np.abs(energy).max())
        forward = 1.0 / (1.0 + np.exp(-(codes @ (W[r] * codes[o]))))
        differs = differs or np.abs(forward[ids] - row).max() > 1e-3
    assert differs                                          # the forward vector would have answered otherwise
