"""UseOutputTransform=Yes through the plugin chain and the command-line tools, on the GPU: the chain model_builder
assembles from a settings file reproduces the vectors of the reference's own model code
(tests/golden/reference_output_transform.npz), and a model with d 10 / c 6 is trained by the driver, checkpointed, reloaded,
evaluated and asked on each side.  Bounds: test_gpu_highway.py's for its reference fixture (codes FWD_ATOL, loss 2e-5 x
max(1, |loss|), gradients helpers.assert_close at rel 1e-3)."""
import os

import numpy as np
import pytest

from helpers import assert_close
from test_gpu_driver import SETTINGS, write_dataset
from test_gpu_eval import csr_for
from test_gpu_topk import known_lists
from test_output_transform_host import CASES, fixture, output_transform_settings_text      # noqa: F401 (fixture)
from test_plugin_surface import load_settings

pytestmark = pytest.mark.gpu

FWD_ATOL = 1e-4


@pytest.mark.parametrize("name", CASES)
def test_plugin_chain_reproduces_the_reference_run(tmp_path, fixture, name):      # noqa: F811
    from relationprediction_amd.common import model_builder
    c, V, d = fixture[name], fixture["V"], fixture["d"]
    triples = fixture["triples"]
    s, enc, dec = load_settings(tmp_path, output_transform_settings_text(d, c["c"], c["nb"], c["L"]), V=V, R=fixture["R"],
                                E=len(triples))
    encoder = model_builder.build_encoder(enc, triples)
    model = model_builder.build_decoder(encoder, dec)
    np.random.seed(fixture["seed"])
    model.preprocess(triples)
    model.register_for_test(triples)
    model.initialize_train()
    graph_var, x_var, y_var = model.get_train_input_variables()
    for var, val in zip((graph_var, x_var, y_var), (triples, fixture["X"], fixture["Y"])):
        var.feed(val)
    test_codes = encoder.get_all_codes(mode='test')[0]
    rt = model.get_runtime()
    assert rt.engine.param_names == c["names"] and (rt.d, rt.dc, rt.engine.dc) == (d, c["c"], c["c"])
    for w, n in zip(model.get_weights(), c["names"]):
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)       # moved into the engine, bit for bit
    assert test_codes.shape == (V, c["c"])
    assert float(np.abs(test_codes - c["codes_test"]).max()) <= FWD_ATOL
    # the train-mode pass under the reference run's masks; the eager surface then reads these activations
    rt.engine.forward(train=True, masks=c["masks"])
    rt._state = (graph_var.version, 'train', rt.weights_version)
    codes = encoder.get_all_codes(mode='train')
    assert codes[0].shape == (V, c["c"]) and codes[1].shape == (V, c["c"])
    assert float(np.abs(codes[0] - c["codes_train"]).max()) <= FWD_ATOL
    loss = model.get_loss('train') + model.get_regularization()
    assert abs(loss - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"])), (loss, c["loss"])
    grads = model.backward()
    assert [g.shape for g in grads] == [w.shape for w in model.get_weights()]
    for g, n in zip(grads, c["names"]):
        if c["connected"][n]:
            assert_close(g, c["grads"][n], rel=1e-3, name=n)
        else:
            assert not g.any(), n
    # the fused paths at the code width
    queries = triples[:12].astype(np.int32)
    for object_side in (True, False):
        known = known_lists(triples, object_side)
        ptr, idx = csr_for(queries, known, object_side)
        raw, filt = model.device_ranks(triples, queries, object_side, ptr, idx)
        assert (raw >= 1).all() and (raw <= V).all() and (filt >= 1).all() and (filt <= raw).all()


def test_train_checkpoint_reload_evaluate_and_predict(tmp_path, capsys):
    """a settings file with d 10 / c 6: three iterations through the driver (validation MRR printed, checkpoint written),
    the checkpoint reloaded by the predict command into a chain with other initial weights, one query per side"""
    from relationprediction_amd import predict, train
    from relationprediction_amd.common import settings_reader
    data = str(tmp_path / "data")
    train_triples = write_dataset(data)
    os.makedirs(str(tmp_path / "models"))
    exp = str(tmp_path / "models" / "Toy")
    text = (SETTINGS % dict(nb=2, concat="No", exp=exp)).replace("UseOutputTransform=No", "UseOutputTransform=Yes") \
        .replace("InternalEncoderDimension=20", "InternalEncoderDimension=10").replace("CodeDimension=20", "CodeDimension=6") \
        .replace("CheckEvery=20", "CheckEvery=3").replace("ReportTrainLossEvery=10", "ReportTrainLossEvery=1")
    settings = tmp_path / "toy.exp"
    settings.write_text(text)
    np.random.seed(0)
    model, iterations = train.main(["--settings", str(settings), "--dataset", data, "--max-iterations", "3"])
    out = capsys.readouterr().out
    assert iterations == 3
    checks = [l for l in out.splitlines() if l.startswith("Tested validation score")]
    assert len(checks) == 1 and 0.0 < float(checks[0].split("Result: ")[1]) <= 1.0
    assert "MRR" in out and "H@10" in out
    names = [w.name for w in model.get_weights()]
    assert names[-3:] == ["W_out", "b_out", "W_relation"]
    trained = {i: w.value() for i, w in enumerate(model.get_weights())}
    assert trained[len(names) - 3].shape == (10, 6) and trained[len(names) - 1].shape == (200, 6)
    assert np.abs(trained[len(names) - 2]).max() > 0                     # b_out started at zero: Adam moved it
    assert os.path.exists(exp + "-0.npz")
    with np.load(exp + "-0.npz") as z:
        keys = sorted(z.files)
        assert keys[-1].endswith("W_relation") and z[keys[-1]].shape == (200, 6) and keys[-3].endswith("W_out")
        stored = [z[k] for k in keys]
    # the checkpoint into a freshly built chain: the codes it encodes are the trained model's
    splits, entities, relations = train.load_dataset(data, "MRR")
    np.random.seed(5)
    other = predict.build_model(settings_reader.read(str(settings)), splits, len(entities), len(relations))
    other.load(exp + "-0.npz")
    for w, v in zip(other.get_weights(), stored):
        np.testing.assert_array_equal(w.value(), v)
    # one query per side through the command
    s0, r0, o0 = (int(x) for x in train_triples[0])
    for side, line in (("object", "e%d\tr%d\n" % (s0, r0)), ("subject", "e%d\tr%d\n" % (o0, r0)),
                       ("relation", "e%d\te%d\n" % (s0, o0))):
        (tmp_path / "q.txt").write_text(line)
        answers = tmp_path / ("answers_%s.txt" % side)
        np.random.seed(8)
        predict.main(["--settings", str(settings), "--dataset", data, "--model", exp + "-0.npz", "--queries",
                      str(tmp_path / "q.txt"), "--k", "3", "--side", side, "--keep-known", "--out", str(answers)])
        rows = [l.split("\t") for l in answers.read_text().splitlines()]
        assert len(rows) == 3 and [r[3] for r in rows] == ["1", "2", "3"]
        scores = [float(r[4]) for r in rows]
        assert all(0.0 <= x <= 1.0 for x in scores) and scores == sorted(scores, reverse=True)
