"""The DistMult baseline's engine kind (RGCN_KIND_EMBEDDING: no graph, no layers, the codes are W_emb) on the GPU, through
the C ABI and through the plugin chain model_builder assembles from the reference's settings/distmult.exp, against the
vectors of the reference's own model code (tests/golden/reference_embedding.npz) and the float64 restatement of
tests/embedding_reference.py.  Bounds: loss 2e-5 x max(1, |loss|) and gradients assert_close(rel=1e-3), which are
tests/test_gpu_train_step.py's; weights after clip + Adam rel = 2e-5, spike = 2e-4 against the float64 replay from the
DEVICE gradients, that file's too.  The codes are compared bit for bit: nothing is computed."""
import numpy as np
import pytest

import embedding_reference as er
from helpers import assert_close
from test_embedding_host import DISTMULT_EXP
from test_gpu_eval import csr_for, known_lists
from test_gpu_featureless import adam_float64
from test_plugin_surface import load_settings

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = 1, 4, 5        # RGCN_ERR_*


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def fixture():
    return er.load_fixture()


def engine(native, c, **kw):
    return native.Engine(c["V"], c["R"], c["d"], 0, "embedding", 1, **kw)


def status_of(native, call, *args, **kw):
    with pytest.raises(native.RgcnError) as e:
        call(*args, **kw)
    return e.value.status, str(e.value)


def test_parameters_and_codes(native, fixture):
    c = fixture
    with engine(native, c) as eng:
        assert eng.param_names == er.NAMES
        assert eng.param_shapes == [(c["V"], c["d"]), (c["d"],), (c["V"], c["d"])]
        assert status_of(native, eng.codes)[0] == STATE                          # no forward pass yet
        eng.set_params(c["params"])
        for train in (True, False):                                               # no graph was ever set
            eng.forward(train=train, seed=77)
            np.testing.assert_array_equal(eng.codes(), c["params"]["W_emb"])
            np.testing.assert_array_equal(eng.activation(0), c["codes_train" if train else "codes_test"])
        assert status_of(native, eng.activation, 1)[0] == INVALID
        assert status_of(native, eng.dropout_mask, 1)[0] == INVALID
        # the codes are the parameter's own storage: a new table is what the next read returns
        other = (c["params"]["W_emb"] * 2).astype(np.float32)
        eng.set_param("W_emb", other)
        np.testing.assert_array_equal(eng.codes(), other)


def test_loss_and_gradients_of_the_reference_code(native, fixture):
    c = fixture
    X, Y = c["X"], c["Y"]
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(X))
        xd, yd = eng.to_device(X), eng.to_device(Y)
        # piecewise: forward, decoder pass, backward fed with the decoder's own dL/dcodes (written in place)
        eng.forward(train=True, seed=1)
        eng.decoder_loss_backward_device(xd, yd, len(X), 0.01)
        eng.backward_from_decoder()
        piecewise = (eng.loss(), eng.get_grads())
        np.testing.assert_array_equal(eng.dcodes(), piecewise[1]["W_emb"])
        # a caller's own gradient, from the host and from a device buffer
        dcodes = np.random.RandomState(3).randn(c["V"], c["d"]).astype(np.float32)
        eng.backward(dcodes)
        np.testing.assert_array_equal(eng.get_grad("W_emb"), dcodes)
        dd = eng.to_device(dcodes * 3)
        eng.backward_device(dd)
        np.testing.assert_array_equal(eng.get_grad("W_emb"), dcodes * 3)
        assert not eng.get_grad("b_emb").any()
        # the whole step (no optimizer configured: the weights stay).  It finds those numbers in the gradient it writes in
        # place and must leave none of them: rows of entities the batch does not mention are written too, as zeros
        eng.train_step_device(None, 0, xd, yd, len(X), seed=2, reg_param=0.01)
        whole = (eng.loss(), eng.get_grads())
        np.testing.assert_array_equal(eng.get_param("W_emb"), c["params"]["W_emb"])
        absent = np.setdiff1d(np.arange(c["V"]), X[:, [0, 2]].ravel())
        assert len(absent) and not whole[1]["W_emb"][absent].any()
        for b in (xd, yd, dd):
            b.free()
    loss64, grads64 = er.loss_and_grads(c["params"], X, Y, 0.01)
    for tag, (loss, grads) in (("piecewise", piecewise), ("step", whole)):
        print("%s: loss %.9g, reference code %.9g, float64 %.9g" % (tag, loss, c["loss"], loss64))
        assert abs(loss - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"])), (tag, loss, c["loss"])
        for n in er.NAMES:
            assert_close(grads[n], c["grads"][n], rel=1e-3, name="%s %s" % (tag, n))
            assert_close(grads[n], grads64[n], rel=1e-3, name="%s %s (float64)" % (tag, n))
        assert not grads["b_emb"].any()
    for n in er.NAMES:
        np.testing.assert_array_equal(piecewise[1][n], whole[1][n], err_msg=n)


def test_two_train_steps_with_clip_and_adam(native, fixture):
    c = fixture
    X, Y = c["X"], c["Y"]
    names = ["W_emb", "W_relation"]                      # b_emb is not a trained tensor
    hyper = (0.01, 0.9, 0.999, 1e-8, 1.0)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(len(X))
        eng.optimizer_config(lr=hyper[0], beta1=hyper[1], beta2=hyper[2], eps=hyper[3], max_grad_norm=hyper[4])
        xd, yd = eng.to_device(X), eng.to_device(Y)
        seen = []
        for step in range(2):
            eng.train_step_device(None, 0, xd, yd, len(X), seed=500 + step, reg_param=0.01)
            seen.append((eng.loss(), eng.get_grads(), eng.get_params()))
            # the codes are the updated table, without a new forward pass
            np.testing.assert_array_equal(eng.codes(), seen[-1][2]["W_emb"])
        for b in (xd, yd):
            b.free()
    before = c["params"]
    for step, (loss, grads, after) in enumerate(seen):
        # each step's loss and gradients belong to the weights the step started from: the second saw the first's update
        loss64, grads64 = er.loss_and_grads(before, X, Y, 0.01)
        assert abs(loss - loss64) <= 2e-5 * max(1.0, abs(loss64)), (step, loss, loss64)
        for n in er.NAMES:
            assert_close(grads[n], grads64[n], rel=1e-3, name="step %d grad %s" % (step, n))
        assert not grads["b_emb"].any() and not after["b_emb"].any()
        for n in names:
            assert not np.array_equal(after[n], before[n]), (step, n)
        before = after
    assert seen[1][0] < seen[0][0]                       # the loss of the same batch fell
    first = adam_float64(c["params"], seen[0][1], names, *hyper)
    both = er.adam_steps_float64(c["params"], [seen[0][1], seen[1][1]], names, *hyper)
    for n in names:
        np.testing.assert_array_equal(first[n], both[0][n])
        assert_close(seen[0][2][n], both[0][n], rel=2e-5, spike=2e-4, name="step 1 weight " + n)
        assert_close(seen[1][2][n], both[1][n], rel=2e-5, spike=2e-4, name="step 2 weight " + n)
    # rows of W_relation past RelationCount are never gathered: no gradient, no update
    np.testing.assert_array_equal(seen[1][2]["W_relation"][c["R"]:], c["params"]["W_relation"][c["R"]:])


def test_device_negatives_then_a_train_step(native, fixture):
    c = fixture
    batch, rate = c["triples"], 3
    n, N = len(batch), len(batch) * (rate + 1)
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        eng.decoder_reserve(N)
        bd, xd, yd = eng.to_device(batch), eng.alloc(12 * N), eng.alloc(4 * N)
        eng.negative_sample_device(bd, n, rate, 99, xd, yd)
        eng.train_step_device(None, 0, xd, yd, N, seed=5, reg_param=0.01)
        loss, grads = eng.loss(), eng.get_grads()
        X, Y = xd.download(np.int32, (N, 3)), yd.download(np.float32, (N,))
        for b in (bd, xd, yd):
            b.free()
    np.testing.assert_array_equal(X[:n], batch)
    assert Y[:n].all() and not Y[n:].any()
    for k in range(1, rate + 1):                          # a corruption replaces exactly one entity
        rows = X[k * n:(k + 1) * n]
        np.testing.assert_array_equal(rows[:, 1], batch[:, 1])
        assert ((rows[:, 0] == batch[:, 0]) | (rows[:, 2] == batch[:, 2])).all()
    assert X.min() >= 0 and X[:, [0, 2]].max() < c["V"]
    loss64, grads64 = er.loss_and_grads(c["params"], X, Y, 0.01)
    assert abs(loss - loss64) <= 2e-5 * max(1.0, abs(loss64)), (loss, loss64)
    for n_ in er.NAMES:
        assert_close(grads[n_], grads64[n_], rel=1e-3, name=n_)


def build_chain(tmp_path, c, seed):
    from relationprediction_amd.common import model_builder
    s, enc, dec = load_settings(tmp_path, DISTMULT_EXP % c["d"], V=c["V"], R=c["R"], E=len(c["triples"]))
    encoder = model_builder.build_encoder(enc, c["triples"])
    model = model_builder.build_decoder(encoder, dec)
    np.random.seed(seed)
    model.preprocess(c["triples"])
    model.register_for_test(c["triples"])
    model.initialize_train()
    return encoder, model


def test_plugin_chain_from_the_settings_file(tmp_path, fixture):
    c = fixture
    triples = c["triples"]
    encoder, model = build_chain(tmp_path, c, c["seed"])
    rt = model.get_runtime()
    assert rt.kind == "embedding" and rt.engine.param_names == er.NAMES and rt.engine.L == 0
    for w, n in zip(model.get_weights(), er.NAMES):
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)       # moved into the engine, bit for bit
    for var, val in zip(model.get_train_input_variables(), (c["X"], c["Y"])):
        var.feed(val)
    for mode in ("train", "test"):
        s_codes, r_codes, o_codes = model.get_all_codes(mode=mode)
        np.testing.assert_array_equal(s_codes, c["codes_" + mode])
        np.testing.assert_array_equal(o_codes, c["codes_" + mode])
        np.testing.assert_array_equal(r_codes, c["params"]["W_relation"])
    # the eager surface against the reference code's numbers
    loss = model.get_loss('train') + model.get_regularization()
    assert abs(loss - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"]))
    grads = model.backward()
    assert [g.shape for g in grads] == [w.shape for w in model.get_weights()]
    for g, n in zip(grads, er.NAMES):
        assert_close(g, c["grads"][n], rel=1e-3, name="eager " + n)
    assert float(np.abs(model.score_all_subjects(c["X"]) - c["subject_scores"]).max()) <= 2e-6
    assert float(np.abs(model.score_all_objects(c["X"]) - c["object_scores"]).max()) <= 2e-6
    # save / load round trip through the engine-bound variables
    model.save(str(tmp_path / "ckpt"))
    encoder2, model2 = build_chain(tmp_path, c, c["seed"] + 1)
    model2.get_runtime()
    assert not np.array_equal(model2.get_weights()[0].value(), c["params"]["W_emb"])
    model2.load(str(tmp_path / "ckpt-0.npz"))
    for w, n in zip(model2.get_weights(), er.NAMES):
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)
    # ranks against a numpy ranking of the float64 energies, tests/test_gpu_add_diagonal.py's tie rule: a query is compared
    # where no energy lies within 1e-3 x max(1, largest |energy|) of the gold's and the gold's is within [-80, 5]
    queries = triples[:24].astype(np.int32)
    compared = 0
    for object_side in (True, False):
        known = known_lists(triples, object_side)
        ptr, idx = csr_for(queries, known, object_side)
        raw, filt = model2.device_ranks(triples, queries, object_side, ptr, idx)
        energy_all = er.energies(c["params"], queries, object_side)
        for i, (s, r, o) in enumerate(queries):
            gold = o if object_side else s
            energy = energy_all[i]
            gap = np.abs(energy - energy[gold])
            gap[gold] = np.inf
            if gap.min() <= 1e-3 * max(1.0, float(np.abs(energy).max())) or energy[gold] > 5.0 or energy[gold] < -80.0:
                continue
            above = energy >= energy[gold]
            lst = idx[ptr[i]:ptr[i + 1]]
            assert raw[i] == int(above.sum()), (object_side, i)
            assert filt[i] == int(above.sum()) - int(above[lst].sum()) + 1, (object_side, i)
            compared += 1
        # top-k on the same energies: ids in (energy descending, id ascending) order wherever the k + 1 best are apart
        k = 5
        top, top_energy = model2.device_topk(triples, queries, object_side, k)
        for i in range(len(queries)):
            order = np.lexsort((np.arange(c["V"]), -energy_all[i]))
            best = energy_all[i][order[:k + 1]]
            if np.min(-np.diff(best)) <= 1e-3 * max(1.0, float(np.abs(energy_all[i]).max())):
                continue
            np.testing.assert_array_equal(top[i], order[:k])
            assert float(np.abs(top_energy[i] - best[:k]).max()) <= 1e-5 * max(1.0, float(np.abs(best).max()))
            compared += 1
    assert compared >= 40, compared


def test_train_steps_through_the_chain(tmp_path, fixture):
    """HipOptimizer's three calls on a graph-less model: host (X, Y), device negatives with the positives resident"""
    c = fixture
    encoder, model = build_chain(tmp_path, c, c["seed"])
    model.configure_device_optimizer(0.01, max_grad_norm=1.0)
    rt = model.get_runtime()
    w0 = model.get_weights()[0].value()
    model.device_train_step(None, c["X"], c["Y"], 11)
    first = model.device_loss()
    assert abs(first - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"]))
    w1 = model.get_weights()[0].value()
    assert not np.array_equal(w0, w1)
    train = c["triples"]
    losses = []
    for step in range(3):
        model.device_train_step_negatives(None, train, 10, 12 + step)
        losses.append(model.device_loss())
        assert rt._resident is train                       # uploaded once, found resident afterwards
    assert np.isfinite(losses).all()                       # (other corruptions every step: no two losses compare)
    assert not np.array_equal(model.get_weights()[0].value(), w1)
    assert rt._dev["batch"].nbytes >= train.nbytes and rt._dec_reserved == 11 * len(train)
    model.device_stage(None, train)                        # nothing to stage for a graph-less model: a no-op
    with pytest.raises(ValueError):
        rt.train_step(train, c["X"], c["Y"], 0.01, 1)      # a graph has no place here
    np.testing.assert_array_equal(model.get_all_codes('test')[0], model.get_weights()[0].value())


@pytest.mark.parametrize("extra", [[], ["--host-negatives", "--batch-workers", "0"]], ids=["device-negatives", "host-negatives"])
def test_train_driver_on_the_reference_settings_file(tmp_path, capsys, extra):
    """relationprediction_amd.train on the text of settings/distmult.exp (a small CodeDimension, checks every 4 iterations):
    the loss of the whole-training-set batch falls, validation MRR is computed, checkpoints hold the three weights"""
    import os
    from relationprediction_amd import train
    from test_gpu_driver import write_dataset
    data = str(tmp_path / "data")
    write_dataset(data)
    exp = str(tmp_path / "models" / "Distmult")
    text = (DISTMULT_EXP % 20).replace("models/Distmult", exp).replace("CheckEvery=2000", "CheckEvery=4") \
        .replace("ReportTrainLossEvery=100", "ReportTrainLossEvery=4")
    (tmp_path / "distmult.exp").write_text(text)
    np.random.seed(0)
    model, iterations = train.main(["--settings", str(tmp_path / "distmult.exp"), "--dataset", data,
                                    "--max-iterations", "9"] + extra)
    out = capsys.readouterr().out
    assert iterations == 9
    initial = float([l for l in out.splitlines() if l.startswith("Initial loss")][0].split(": ")[1])
    losses = [float(l.split(": ")[-1]) for l in out.splitlines() if l.startswith("Average train loss")]
    assert len(losses) == 2 and losses[-1] < initial, (initial, losses)
    checks = [l for l in out.splitlines() if l.startswith("Tested validation score")]
    assert len(checks) == 2 and all(0.0 < float(c.split("Result: ")[1]) <= 1.0 for c in checks)
    with np.load(exp + "-1.npz") as z:
        assert [k.split("_", 1)[1] for k in sorted(z.files)] == er.NAMES
        assert z[sorted(z.files)[0]].shape == (200, 20) and not z[sorted(z.files)[1]].any()      # b_emb: still zeros
    assert not model.needs_graph()


def test_predict_command_from_an_embedding_checkpoint(tmp_path):
    """relationprediction_amd.predict, unchanged, on a Name=embedding checkpoint (tests/test_gpu_topk.py's end-to-end case)"""
    import helpers
    from relationprediction_amd import predict
    from relationprediction_amd.common import evaluation, settings_reader
    V, R, k = 16, 9, 4
    triples = helpers.load_graph("toy_train")
    ents, rels = ["e%d" % i for i in range(V)], ["r%d" % i for i in range(R)]
    (tmp_path / "entities.dict").write_text("".join("%d\t%s\n" % (i, n) for i, n in enumerate(ents)))
    (tmp_path / "relations.dict").write_text("".join("%d\t%s\n" % (i, n) for i, n in enumerate(rels)))
    lines = ["%s\t%s\t%s\n" % (ents[s], rels[r], ents[o]) for s, r, o in triples]
    (tmp_path / "train.txt").write_text("".join(lines[:-6]))
    (tmp_path / "valid.txt").write_text("".join(lines[-6:-3]))
    (tmp_path / "test.txt").write_text("".join(lines[-3:]))
    (tmp_path / "s.exp").write_text(DISTMULT_EXP % 12)
    pairs = [(int(s), int(r)) for s, r, o in triples[:7]]
    (tmp_path / "q.txt").write_text("".join("%s\t%s\n" % (ents[e], rels[r]) for e, r in pairs))
    splits = {"train": triples[:-6].astype(np.int32), "valid": triples[-6:-3], "test": triples[-3:]}
    np.random.seed(7)
    model = predict.build_model(settings_reader.read(str(tmp_path / "s.exp")), splits, V, R)
    model.save(str(tmp_path / "models" / "Distmult"))
    np.random.seed(8)                                                  # the command's chain starts from other weights
    out = tmp_path / "answers.txt"
    predict.main(["--settings", str(tmp_path / "s.exp"), "--dataset", str(tmp_path), "--model",
                  str(tmp_path / "models" / "Distmult-0.npz"), "--queries", str(tmp_path / "q.txt"), "--k", str(k),
                  "--out", str(out)])
    known = {}
    evaluation.Scorer.extend_triple_dict(known, triples, object_list=True)
    ptr, idx = evaluation.known_completions_csr(pairs, known)
    queries = np.full((len(pairs), 3), -1, dtype=np.int32)
    queries[:, 0] = [p[0] for p in pairs]
    queries[:, 1] = [p[1] for p in pairs]
    want_idx, want_energy = model.device_topk(splits["train"], queries, True, k, ptr, idx)
    want_score = predict.sigmoid_f32(want_energy)
    got = [l.split("\t") for l in out.read_text().splitlines()]
    want = [[ents[e], rels[r], ents[a], str(p + 1), "%.9g" % sc] for (e, r), ids, row in zip(pairs, want_idx, want_score)
            for p, (a, sc) in enumerate(zip(ids, row)) if a >= 0]
    assert got == want and len(got) > len(pairs)


def test_refusals(native, fixture):
    c = fixture
    V, R, d = c["V"], c["R"], c["d"]
    make = native.Engine
    assert status_of(native, make, V, R, d, 1, "embedding", 1)[0] == INVALID          # layers
    assert status_of(native, make, V, R, d, 0, "embedding", 2)[0] == INVALID          # bases
    assert status_of(native, make, V, R, d, 0, "basis", 1, max_edges=4)[0] == INVALID  # num_layers <= 0 stays invalid elsewhere
    assert status_of(native, make, V, R, d, 0, "block", 1, max_edges=4)[0] == INVALID
    assert status_of(native, make, V, R, d, 0, "embedding", 1, keep_prob=0.0)[0] == INVALID
    assert status_of(native, make, V, R, d, 0, "embedding", 1, norm_mode=9)[0] == INVALID
    for kw in (dict(world=2, rank=0), dict(input_mode="onehot"), dict(skip="highway")):
        st, msg = status_of(native, make, V, R, d, 0, "embedding", 1, **kw)
        assert st == UNSUPPORTED and "RGCN_KIND_EMBEDDING" in msg, (kw, msg)
    X, Y = c["X"], c["Y"]
    with engine(native, c) as eng:
        eng.set_params(c["params"])
        td, xd, yd = eng.to_device(c["triples"]), eng.to_device(X), eng.to_device(Y)
        scratch_x, scratch_y = eng.alloc(12 * 4 * len(X)), eng.alloc(4 * 4 * len(X))
        dcodes = eng.to_device(np.zeros((V, d), np.float32))
        refused = [
            ("rgcn_set_graph", lambda: eng.set_graph(c["triples"])),
            ("rgcn_set_graph_device", lambda: eng.set_graph_device(td, len(c["triples"]))),
            ("rgcn_set_graph_dropout_device", lambda: eng.set_graph_dropout_device(td, 10, 5, seed=1)),
            ("rgcn_prefetch_graph_device", lambda: eng.prefetch_graph_device(td, 10)),
            ("rgcn_prefetch_graph_dropout_device", lambda: eng.prefetch_graph_dropout_device(td, 10, 5, 1)),
            ("rgcn_step_device", lambda: eng.step_device(td, 10, dcodes)),
            ("rgcn_train_step_minibatch_device",
             lambda: eng.train_step_minibatch_device(td, 10, 5, 1, 3, 2, scratch_x, scratch_y)),
            ("rgcn_neighborhood_reserve", lambda: eng.neighborhood_reserve(c["triples"])),
            ("rgcn_forward_begin", lambda: eng.forward_begin(train=False)),
            ("rgcn_forward_layer_partial", lambda: eng.forward_layer_partial(1)),
            ("rgcn_forward_layer_finish", lambda: eng.forward_layer_finish(1)),
            ("rgcn_backward_begin", lambda: eng.backward_begin(dcodes)),
            ("rgcn_backward_layer_partial", lambda: eng.backward_layer_partial(1)),
            ("rgcn_backward_layer_finish", lambda: eng.backward_layer_finish(1)),
            ("rgcn_backward_end", lambda: eng.backward_end()),
            ("rgcn_set_relation_owner", lambda: eng.set_relation_owner(np.zeros(R, np.int32))),
            ("rgcn_capture_begin", lambda: eng.capture_begin()),
        ]
        for name, call in refused:
            st, msg = status_of(native, call)
            assert st == UNSUPPORTED and name + ":" in msg and "RGCN_KIND_EMBEDDING" in msg, (name, st, msg)
        # a train step with a graph: invalid, whichever half of the graph argument is there
        eng.decoder_reserve(len(X))
        assert status_of(native, eng.train_step_device, td, 0, xd, yd, len(X))[0] == INVALID
        assert status_of(native, eng.train_step_device, None, 3, xd, yd, len(X))[0] == INVALID
        assert status_of(native, eng.backward, np.zeros((V, d), np.float32))[0] == STATE      # before any forward pass
        assert status_of(native, eng.read_buffer, native.BUF_SELF)[0] == STATE
        assert status_of(native, eng.read_buffer, native.BUF_INDEG)[0] == STATE
        # what stays: the step itself still runs after all the refusals
        eng.train_step_device(None, 0, xd, yd, len(X), seed=1, reg_param=0.01)
        assert abs(eng.loss() - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"]))
        for b in (td, xd, yd, scratch_x, scratch_y, dcodes):
            b.free()


def test_pool_accounting_create_step_destroy():
    """tests/test_gpu_memory_ownership.py's create / destroy accounting, for one embedding context (devtools build): the
    context owns the three parameters, their gradients, the slab, the zero page and the error flag -- nine blocks -- and a
    host-fed backward pass adds none (the staging copy of dcodes IS W_emb's gradient)"""
    from relationprediction_amd import _native
    _native.load_library(devtools=True)
    V, d = 300, 20
    dcodes = (np.random.RandomState(6).randn(V, d) * 0.1).astype(np.float32)
    rng = np.random.RandomState(5)
    X = np.stack([rng.randint(0, V, 50), rng.randint(0, 5, 50), rng.randint(0, V, 50)], 1).astype(np.int32)
    Y = (np.arange(50) < 10).astype(np.float32)
    seen = []
    for _ in range(3):
        eng = _native.Engine(V, 5, d, 0, "embedding", 1, devtools=True)
        try:
            seen.append(eng.device_memory())
            assert seen[-1] == (9, 4 * (4 * V * d + 2 * d + 1024 + 1024 + 1))
            eng.forward(train=True, seed=1)
            eng.backward(dcodes)
            assert eng.device_memory() == seen[-1]
            eng.decoder_reserve(len(X))
            eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
            xd, yd = eng.to_device(X), eng.to_device(Y)
            reserved = eng.device_memory()
            eng.train_step_device(None, 0, xd, yd, len(X), seed=1, reg_param=0.01)
            assert np.isfinite(eng.loss())
            after = eng.device_memory()
            # the first optimizer step adds the moments of W_emb and of the R used rows of W_relation, its state and partials
            assert after[0] > reserved[0] and after[1] >= reserved[1] + 4 * 2 * (V * d + 5 * d)
            eng.train_step_device(None, 0, xd, yd, len(X), seed=2, reg_param=0.01)
            assert eng.device_memory() == after                    # and a second step nothing
            for b in (xd, yd):
                b.free()
        finally:
            eng.close()
    assert seen[0] == seen[1] == seen[2], seen
