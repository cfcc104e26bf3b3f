"""Golden vectors of the DistMult baseline (Encoder.Name=embedding) computed by the reference's own model code (run where
a checkout of the reference exists; its `code/` directory is the argument or $RELATIONPREDICTION_REFERENCE_CODE):

    python -B tests/golden/make_reference_embedding_fixture.py <reference>/code  ->  tests/golden/reference_embedding.npz

make_reference_add_diagonal_fixture.py's recipe -- the TensorFlow stand-ins (tf_numpy_shim.py, tf_torch_shim.py) imported
unedited -- on the reference's model_builder with Name=embedding and the bilinear-diag decoder (the sections of
settings/distmult.exp, CodeDimension lowered).  The chain it assembles is
BilinearDiag -> RelationEmbedding -> AffineTransform (common/model_builder.py:27-41: onehot_input=True, use_bias=False,
use_nonlinearity=False, nothing beneath it).  V 30, R 4, d 8, N 30.  Stored: the initial weights in get_weights() order
(W [V,d], b [d], W_relation [V,d]), the train- and test-mode codes, train.py's loss (get_loss + get_regularization), the
scores of predict_all_subject_scores / predict_all_object_scores for the N triples and -- from a second run of the same
model code on torch tensors -- the gradient of that loss w.r.t. every weight with a flag saying whether autograd reached
it at all (b is not: use_bias=False never reads it).  tests/test_embedding_host.py holds the float64 restatement
(tests/embedding_reference.py) and the plugin chain's initial weights to these vectors.
"""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ["RELATIONPREDICTION_REFERENCE_CODE"])
V, R, d, N, SEED = 30, 4, 8, 30, 13


def settings():
    # EdgeCount: Model.__init__ of the reference reads it from every component's settings (train.py:78 puts it)
    enc = {'Name': 'embedding', 'CodeDimension': str(d), 'EntityCount': V, 'RelationCount': R, 'EdgeCount': N,
           'NegativeSampleRate': '10', 'GraphSplitSize': '0.5', 'GraphBatchSize': '30000'}
    dec = {'Name': 'bilinear-diag', 'RegularizationParameter': '0.01', 'CodeDimension': str(d),
           'EntityCount': V, 'RelationCount': R, 'EdgeCount': N, 'NegativeSampleRate': '10'}
    return enc, dec


def main():
    sys.path.insert(0, HERE)
    import tf_numpy_shim as tf
    import tf_torch_shim as tft
    sys.modules['tensorflow'] = tf
    for stub in ("theano", "theano.tensor"):
        sys.modules.setdefault(stub, types.ModuleType(stub))
    sys.modules["theano"].tensor = sys.modules["theano.tensor"]
    sys.path.insert(0, REF)
    from common import model_builder                       # the reference's
    from decoders.bilinear_diag import BilinearDiag

    rng = np.random.RandomState(100 + SEED)
    triples = np.stack([rng.randint(0, V, N), rng.randint(0, R, N), rng.randint(0, V, N)], 1).astype(np.int32)
    X = np.stack([rng.randint(0, V, N), rng.randint(0, R, N), rng.randint(0, V, N)], 1).astype(np.int32)
    X[:N // 3] = triples[:N // 3]
    Y = (np.arange(N) < N // 3).astype(np.float32)
    enc, dec = settings()

    def build():
        BilinearDiag.encoder_cache = {'train': None, 'test': None}       # class-level cache
        np.random.seed(SEED)
        encoder = model_builder.build_encoder(enc, triples)
        model = model_builder.build_decoder(encoder, dec)
        model.preprocess(triples)
        model.register_for_test(triples)
        model.initialize_train()
        return encoder, model

    tf.reset({'X': X, 'Y': Y}, dropout_seed=SEED, sparse_softmax_mode="intended")
    encoder, model = build()
    assert not model.needs_graph()
    chain, c = [], model
    while c is not None:
        chain.append(type(c).__name__)
        c = c.next_component
    weights = [np.array(w) for w in model.get_weights()]
    loss = model.get_loss(mode='train') + model.get_regularization()
    codes_train = np.array(encoder.get_all_codes(mode='train')[0])
    BilinearDiag.encoder_cache = {'train': None, 'test': None}
    codes_test = np.array(encoder.get_all_codes(mode='test')[0])
    out = {"config": np.array([V, R, d, N, SEED], dtype=np.int64), "triples": triples, "X": X, "Y": Y,
           "chain": np.array(",".join(chain)), "loss_train": np.float64(loss), "codes_train": codes_train,
           "codes_test": codes_test,
           "subject_scores": np.array(model.predict_all_subject_scores()),
           "object_scores": np.array(model.predict_all_object_scores())}
    for i, w in enumerate(weights):
        out["weight%02d" % i] = w
    # the same model code on torch tensors: tf.gradients(loss, weights) by autograd over the reference's own dataflow
    ref_modules = [m for m in list(sys.modules.values())
                   if getattr(m, '__file__', None) and str(m.__file__).startswith(REF) and hasattr(m, 'tf')]
    for m in ref_modules:
        m.tf = tft
    tft.reset({'X': X, 'Y': Y}, [], sparse_softmax_mode="intended")
    encoder_t, model_t = build()
    weights_t = model_t.get_weights()
    for w_np, w_t in zip(weights, weights_t):
        assert np.array_equal(w_np, w_t.detach().numpy())
    loss_t = model_t.get_loss(mode='train') + model_t.get_regularization()
    assert abs(float(loss_t) - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    loss_t.backward()
    for i, w_t in enumerate(weights_t):
        out["grad%02d" % i] = w_t.grad.numpy() if w_t.grad is not None else np.zeros_like(weights[i])
        out["grad%02d_connected" % i] = np.array(w_t.grad is not None)
    print("chain", chain, "weights", [w.shape for w in weights], "loss %.6f" % loss,
          "unconnected", [i for i, w_t in enumerate(weights_t) if w_t.grad is None])
    np.savez_compressed(os.path.join(HERE, "reference_embedding.npz"), **out)


if __name__ == "__main__":
    main()
