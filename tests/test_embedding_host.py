"""The DistMult baseline (Encoder.Name=embedding) and the ensemble rank on the CPU: the float64 restatement of
tests/embedding_reference.py against the vectors of the reference's own model code (tests/golden/reference_embedding.npz),
the plugin chain model_builder assembles from the reference's settings/distmult.exp, and the comparability rule the GPU
tests of rgcn_rank_mixed_device use, with its cap asserted for the very inputs they run.  No GPU, no engine."""
import numpy as np
import pytest

import embedding_reference as er
from helpers import assert_close
from test_plugin_surface import load_settings

# the reference's settings/distmult.exp; CodeDimension is the placeholder the tests fill in
DISTMULT_EXP = """[Encoder]
\tName=embedding

[Decoder]
\tName=bilinear-diag
\tRegularizationParameter=0.01

[Shared]
\tCodeDimension=%d

[Optimizer]
\tMaxGradientNorm=1
\tReportTrainLossEvery=100

\t[EarlyStopping]
\t\tCheckEvery=2000
\t\tBurninPhaseDuration=6000

\t[Algorithm]
\t\tName=Adam
\t\tlearning_rate=0.01

[General]
\tNegativeSampleRate=10
\tGraphSplitSize=0.5
\tExperimentName=models/Distmult
\tGraphBatchSize=30000

[Evaluation]
\tMetric=MRR
"""


@pytest.fixture(scope="module")
def fixture():
    return er.load_fixture()


def chain_of(model):
    out, c = [], model
    while c is not None:
        out.append(c)
        c = c.next_component
    return out


def test_fixture_is_the_chain_the_issue_names(fixture):
    c = fixture
    assert c["chain"] == ["BilinearDiag", "RelationEmbedding", "AffineTransform"]
    assert [c["params"][n].shape for n in er.NAMES] == [(30, 8), (8,), (30, 8)]
    assert c["connected"] == {"W_emb": True, "b_emb": False, "W_relation": True}      # use_bias=False never reads b
    assert not c["params"]["b_emb"].any()


def test_float64_restatement_against_the_reference_code(fixture):
    c = fixture
    for mode in ("train", "test"):
        np.testing.assert_array_equal(er.codes(c["params"], mode).astype(np.float32), c["codes_" + mode])
    np.testing.assert_array_equal(c["codes_train"], c["params"]["W_emb"])          # the codes ARE the table
    loss, grads = er.loss_and_grads(c["params"], c["X"], c["Y"], 0.01)
    assert abs(loss - c["loss"]) <= 2e-6 * max(1.0, abs(c["loss"])), (loss, c["loss"])
    for n in er.NAMES:
        assert_close(c["grads"][n], grads[n], name=n)                             # the reference's are float32
    assert not grads["b_emb"].any() and not c["grads"]["b_emb"].any()
    assert not grads["W_relation"][c["R"]:].any()                                  # rows >= RelationCount: never gathered
    for side, key in ((False, "subject_scores"), (True, "object_scores")):
        got = er.all_scores(c["params"], c["X"], side)
        assert got.shape == c[key].shape == (c["N"], c["V"])
        assert float(np.abs(got - c[key]).max()) <= 2e-6, key


def test_model_builder_on_the_reference_settings_file(tmp_path, fixture):
    from relationprediction_amd.common import model_builder
    from relationprediction_amd.decoders.bilinear_diag import BilinearDiag
    from relationprediction_amd.encoders.affine_transform import AffineTransform
    from relationprediction_amd.encoders.relation_embedding import RelationEmbedding
    c = fixture
    s, enc, dec = load_settings(tmp_path, DISTMULT_EXP % c["d"], V=c["V"], R=c["R"], E=len(c["triples"]))
    encoder = model_builder.build_encoder(enc, c["triples"])
    model = model_builder.build_decoder(encoder, dec)
    comps = chain_of(model)
    assert [type(x) for x in comps] == [BilinearDiag, RelationEmbedding, AffineTransform]
    affine = comps[-1]
    assert affine.onehot_input and not affine.use_bias and not affine.use_nonlinearity and affine.next_component is None
    assert not model.needs_graph() and not encoder.needs_graph()
    np.random.seed(c["seed"])
    model.preprocess(c["triples"])
    model.register_for_test(c["triples"])
    model.initialize_train()
    weights = model.get_weights()
    assert [w.name for w in weights] == er.NAMES
    for w, n in zip(weights, er.NAMES):                     # the reference's draws under the fixture's seed, bit for bit
        np.testing.assert_array_equal(w.value(), c["params"][n], err_msg=n)
    assert [v.name for v in model.get_train_input_variables()] == ["X", "Y"]
    assert [v.name for v in model.get_test_input_variables()] == ["X"]


def test_names_that_stay_refused(tmp_path):
    from relationprediction_amd.common import model_builder
    from relationprediction_amd.encoders.affine_transform import AffineTransform
    for name in ("variational_embedding", "gcn_diag", "bipartite_gcn", "Embedding"):
        s, enc, dec = load_settings(tmp_path, DISTMULT_EXP.replace("Name=embedding", "Name=" + name) % 8)
        with pytest.raises(NotImplementedError):
            model_builder.build_encoder(enc, np.zeros((3, 3), dtype=int))
    s, enc, dec = load_settings(tmp_path, (DISTMULT_EXP % 8).replace("Name=bilinear-diag", "Name=complex"))
    with pytest.raises(NotImplementedError):
        model_builder.build_decoder(None, dec)
    # Name=embedding in a file that also describes a graph-convolution stack: contradictory, refused naming the keys
    from test_plugin_surface import BLOCK_EXP
    s, enc, dec = load_settings(tmp_path, BLOCK_EXP.replace("Name=gcn_basis", "Name=embedding"))
    with pytest.raises(NotImplementedError, match="NumberOfLayers"):
        model_builder.build_encoder(enc, np.zeros((3, 3), dtype=int))
    for key, value in (("NumberOfLayers", "2"), ("Concatenation", "Yes"), ("SkipConnections", "None")):
        text = (DISTMULT_EXP % 8).replace("\tName=embedding\n", "\tName=embedding\n\t%s=%s\n" % (key, value))
        s, enc, dec = load_settings(tmp_path, text)
        with pytest.raises(NotImplementedError, match=key):
            model_builder.build_encoder(enc, np.zeros((3, 3), dtype=int))
    # every AffineTransform variant but the two that are built
    s, enc, dec = load_settings(tmp_path, DISTMULT_EXP % 8)
    for onehot, bias, relu in ((True, True, False), (True, False, True), (False, False, False), (False, True, True)):
        with pytest.raises(NotImplementedError):
            AffineTransform([16, 8], enc, onehot_input=onehot, use_bias=bias, use_nonlinearity=relu)
    other = AffineTransform([16, 8], enc, onehot_input=True, use_bias=False, use_nonlinearity=False)
    with pytest.raises(NotImplementedError):                # the lookup has nothing beneath it
        AffineTransform([16, 8], enc, next_component=other, onehot_input=True, use_bias=False, use_nonlinearity=False)


def test_graphless_transform_hands_out_the_training_set(tmp_path):
    """make_transform for a graph-less encoder: (X, Y) of the whole training set under host negatives, the training array
    itself (to stay resident on the device) otherwise; the GraphBatchSize of distmult.exp is never looked at"""
    from relationprediction_amd import train
    from relationprediction_amd.common import model_builder
    from relationprediction_amd.optimization.optimize import DeviceNegatives
    rng = np.random.RandomState(0)
    triples = np.stack([rng.randint(0, 16, 40), rng.randint(0, 3, 40), rng.randint(0, 16, 40)], 1).astype(np.int32)
    s, enc, dec = load_settings(tmp_path, DISTMULT_EXP % 8, V=16, R=3, E=len(triples))
    encoder = model_builder.build_encoder(enc, triples)
    t = train.make_transform(triples, s['General'], encoder, device_negatives=False)      # 30000 > 40 edges: not an error
    X, Y = t(triples)
    assert X.shape == (40 * 11, 3) and Y.shape == (40 * 11,) and Y[:40].all() and not Y[40:].any()
    np.testing.assert_array_equal(X[:40], triples)
    b = train.make_transform(triples, s['General'], encoder, device_negatives=True, device_dropout=True)(triples)
    assert isinstance(b, DeviceNegatives) and b.graph_edges is None and b.batch is triples and b.rate == 10


# ---------------------------------------------------------------- ensemble ranks
def test_mixed_ranks_against_the_reference_rule():
    """tiny arrays: mixed_ranks' filtered rank is WeightEnsemble.combine_prediction's -- 1 + the remaining candidates
    whose mixed score is at least the gold's -- where the list is distinct and holds the gold"""
    rng = np.random.RandomState(7)
    V, n = 9, 12
    ea, eb = rng.randn(n, V) * 2, rng.randn(n, V) * 2
    ea[3] = ea[3, 0]                                      # a row of ties in one model
    eb[3] = eb[3, 0]                                      # ... and in both: every candidate ties with the gold
    gold = rng.randint(0, V, n)
    lists = [sorted(set([int(g)] + [int(e) for e in rng.randint(0, V, 3)])) for g in gold]
    for w in (0.0, 0.4, 0.5, 1.0):
        raw, filt = er.mixed_ranks(ea, eb, w, gold, lists)
        sa, sb = er.sigmoid64(ea), er.sigmoid64(eb)
        for i in range(n):
            rest = [e for e in range(V) if e not in lists[i]]
            assert filt[i] == er.ensemble_rule((sa[i, gold[i]], sb[i, gold[i]]), (sa[i, rest], sb[i, rest]), w)
            everyone = [e for e in range(V) if e != gold[i]]
            assert raw[i] == er.ensemble_rule((sa[i, gold[i]], sb[i, gold[i]]), (sa[i, everyone], sb[i, everyone]), w)
        assert raw[3] == V
    # weight 1 / 0: one model's own ranks
    one = er.mixed_ranks(ea, eb, 1.0, gold, lists)
    assert np.array_equal(one[0], er.mixed_ranks(ea, ea, 0.3, gold, lists)[0])
    assert np.array_equal(er.mixed_ranks(ea, eb, 0.0, gold, lists)[1], er.mixed_ranks(eb, eb, 0.7, gold, lists)[1])
    # an empty list filters nothing and still adds the reference's + 1; a duplicate counts twice (the device's rule)
    r, f = er.mixed_ranks(ea[:1], eb[:1], 0.5, gold[:1], [[]])
    assert f[0] == r[0] + 1
    r2, f2 = er.mixed_ranks(ea[:1], eb[:1], 0.5, gold[:1], [[int(gold[0]), int(gold[0])]])
    assert f2[0] == r2[0] - 1


def test_comparability_rule():
    ea = np.array([[0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 0.0, 5.0]])
    eb = np.zeros((3, 3))
    gold = np.array([1, 1, 0])
    ok = er.comparable(ea, eb, 0.5, gold)
    assert list(ok) == [True, True, False]                # row 2: candidate 1 ties with the gold exactly
    ea[1, 2] = 1.0 + 2e-5                                  # mixed scores 0.5 * sigmoid'(1) * 2e-5 = 2e-6 apart: too close
    assert list(er.comparable(ea, eb, 0.5, gold)) == [True, False, False]


@pytest.mark.parametrize("name", sorted(er.MIXED_SHAPES))
def test_the_cap_holds_for_the_inputs_the_gpu_tests_use(name):
    """the margin may leave out at most 5 % of a case's queries (both sides together): a condition on the inputs, asserted
    here for exactly what tests/test_gpu_rank_mixed.py runs; a float32 evaluation agrees on every query that is kept"""
    case = er.mixed_case(name)
    for w in er.MIXED_WEIGHTS:
        left_out = total = 0
        for object_side, side in case["sides"].items():
            ok = er.comparable(side["ea"], side["eb"], w, side["gold"])
            left_out += int((~ok).sum())
            total += len(ok)
            raw64, filt64 = er.mixed_ranks(side["ea"], side["eb"], w, side["gold"], side["lists"])
            # the device's arithmetic on the host: float32 energies, float32 sigmoids, the mix in double rounded once
            sa = er.sigmoid64(side["ea"].astype(np.float32)).astype(np.float32)
            sb = er.sigmoid64(side["eb"]).astype(np.float32)
            m = (w * sa.astype(np.float64) + (1.0 - w) * sb.astype(np.float64)).astype(np.float32)
            for i in np.flatnonzero(ok):
                above = m[i] >= m[i, side["gold"][i]]
                lst = np.asarray(side["lists"][i], dtype=np.int64)
                assert int(above.sum()) == raw64[i] and int(above.sum()) - int(above[lst].sum()) + 1 == filt64[i]
        print("%s w=%.1f: %d of %d queries left out" % (name, w, left_out, total))
        assert left_out <= er.MAX_LEFT_OUT * total, (name, w, left_out, total)
