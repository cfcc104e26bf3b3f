"""Golden vectors of the encoder under UseOutputTransform=Yes computed by the reference's own model code (run where
the reference checkout exists):

    python -B tests/golden/make_reference_output_transform_fixture.py <reference>/code
        ->  tests/golden/reference_output_transform.npz      (or RELATIONPREDICTION_REFERENCE_CODE=<reference>/code)

make_reference_highway_fixture.py's recipe -- the TensorFlow stand-ins (tf_numpy_shim.py, tf_torch_shim.py) imported
unedited, the class-level caches reset between builds -- with UseInputTransform=Yes and UseOutputTransform=Yes.  The
reference's model_builder then assembles Representation -> AffineTransform -> BasisGcn x L -> AffineTransform
[InternalEncoderDimension, CodeDimension] (dense, bias, no relu) -> RelationEmbedding [EntityCount, CodeDimension] ->
BilinearDiag (common/model_builder.py:131-135,170-182, encoders/affine_transform.py:63-83).  Two basis cases at V 30,
R 4, E 60, N 30: `narrow` (d 8 -> c 4, B 3, L 2) and `wide` (d 8 -> c 12, B 3, L 1).  Stored per case, keys prefixed with
its name: the initial weights in get_weights() order, the dropout masks, the train- and test-mode codes, train.py's
loss, and -- from a second run of the same model code on torch tensors -- the gradient of that loss w.r.t. every weight.
tests/test_output_transform_host.py holds the float64 restatement (tests/output_transform_reference.py) to these vectors.
"""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ["RELATIONPREDICTION_REFERENCE_CODE"])
V, R, d, E, N, SEED = 30, 4, 8, 60, 30, 13
CASES = {"narrow": (4, 3, 2), "wide": (12, 3, 1)}       # name -> (CodeDimension, NumberOfBasisFunctions, L)


def settings(c, nb, L):
    enc = {'Name': 'gcn_basis', 'DropoutKeepProbability': '0.8', 'InternalEncoderDimension': str(d),
           'NumberOfBasisFunctions': str(nb), 'NumberOfLayers': str(L), 'UseInputTransform': 'Yes',
           'UseOutputTransform': 'Yes', 'AddDiagonal': 'No', 'DiagonalCoefficients': 'No', 'SkipConnections': 'None',
           'StoreEdgeData': 'No', 'RandomInput': 'No', 'PartiallyRandomInput': 'No',
           'Concatenation': 'No',
           'CodeDimension': str(c), 'EntityCount': V, 'RelationCount': R, 'EdgeCount': E, 'NegativeSampleRate': '10',
           'GraphSplitSize': '0.5'}
    dec = {'Name': 'bilinear-diag', 'RegularizationParameter': '0.01', 'CodeDimension': str(c),
           'EntityCount': V, 'RelationCount': R, 'EdgeCount': E, 'NegativeSampleRate': '10'}
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
    from encoders.message_gcns.message_gcn import MessageGcn
    from decoders.bilinear_diag import BilinearDiag

    rng = np.random.RandomState(100 + SEED)
    triples = np.stack([rng.randint(0, V, E), rng.randint(0, R, E), rng.randint(0, V, E)], 1).astype(np.int32)
    X = np.stack([rng.randint(0, V, N), rng.randint(0, R, N), rng.randint(0, V, N)], 1).astype(np.int32)
    X[:N // 3] = triples[:N // 3]
    Y = (np.arange(N) < N // 3).astype(np.float32)
    out = {"config": np.array([V, R, d, E, N, SEED], dtype=np.int64), "triples": triples, "X": X, "Y": Y}
    ref_modules = None
    for name, (cdim, nb, L) in CASES.items():
        enc, dec = settings(cdim, nb, L)

        def build():
            MessageGcn.vertex_embedding_function = {'train': None, 'test': None}      # class-level caches
            BilinearDiag.encoder_cache = {'train': None, 'test': None}
            np.random.seed(SEED)
            encoder = model_builder.build_encoder(enc, triples)
            model = model_builder.build_decoder(encoder, dec)
            model.preprocess(triples)
            model.register_for_test(triples)
            model.initialize_train()
            return encoder, model

        if ref_modules is not None:
            for m in ref_modules:
                m.tf = tf
        tf.reset({'graph_edges': triples, 'X': X, 'Y': Y}, dropout_seed=SEED, sparse_softmax_mode="intended")
        encoder, model = build()
        chain, c = [], model
        while c is not None:
            chain.append(type(c).__name__)
            c = c.next_component
        weights = [np.array(w) for w in model.get_weights()]
        loss = model.get_loss(mode='train') + model.get_regularization()
        codes_train = np.array(encoder.get_all_codes(mode='train')[0])
        masks = [np.array(m) for m in tf.DROPOUT_MASKS]                            # call order: bottom layer first
        assert len(masks) == L
        codes_test = np.array(encoder.get_all_codes(mode='test')[0])
        pre = name + "_"
        assert codes_train.shape == codes_test.shape == (V, cdim)
        out[pre + "config"] = np.array([cdim, nb, L], dtype=np.int64)
        out[pre + "chain"] = np.array(",".join(chain))
        out[pre + "loss_train"] = np.float64(loss)
        out[pre + "codes_train"] = codes_train
        out[pre + "codes_test"] = codes_test
        for i, w in enumerate(weights):
            out[pre + "weight%02d" % i] = w
        for i, m in enumerate(masks):
            out[pre + "mask%d" % (i + 1)] = m
        # the same model code on torch tensors: tf.gradients(loss, weights) by autograd over the reference's own dataflow
        ref_modules = [m for m in list(sys.modules.values())
                       if getattr(m, '__file__', None) and str(m.__file__).startswith(REF) and hasattr(m, 'tf')]
        for m in ref_modules:
            m.tf = tft
        tft.reset({'graph_edges': triples, 'X': X, 'Y': Y}, masks, sparse_softmax_mode="intended")
        encoder_t, model_t = build()
        weights_t = model_t.get_weights()
        for w_np, w_t in zip(weights, weights_t):
            assert np.array_equal(w_np, w_t.detach().numpy())
        loss_t = model_t.get_loss(mode='train') + model_t.get_regularization()
        assert abs(float(loss_t) - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
        loss_t.backward()
        for i, w_t in enumerate(weights_t):
            out[pre + "grad%02d" % i] = w_t.grad.numpy() if w_t.grad is not None else np.zeros_like(weights[i])
            out[pre + "grad%02d_connected" % i] = np.array(w_t.grad is not None)
        print(name, "chain", chain, "weights", [w.shape for w in weights], "loss %.6f" % loss,
              "unconnected", [i for i, w_t in enumerate(weights_t) if w_t.grad is None])
    np.savez_compressed(os.path.join(HERE, "reference_output_transform.npz"), **out)


if __name__ == "__main__":
    main()
