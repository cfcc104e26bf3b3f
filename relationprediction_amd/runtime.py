"""EncoderRuntime: binds a chain of reference-shaped plugin components to ONE HIP engine context.

The reference builds a TF graph by recursing through `get_all_codes` (message_gcn.py:39,58) and runs
it in `session.run`.  Here the same recursion is collapsed: the first `get_all_codes` of a step makes
the engine run the whole encoder stack (input layer + L graph-convolution layers) and every component
then reads "its" activation.  The runtime lives on the graph `Representation` at the bottom of the chain.
"""
import numpy as np

from . import _native


class EncoderRuntime(object):
    def __init__(self, layers, affine, representation, output=None):
        """layers: MessageGcn components bottom -> top.  affine: the input layer under them, or None when the bottom
        layer is featureless (onehot_input=True, UseInputTransform=No: it reads entity ids, there is no H_0).  output:
        the dense AffineTransform over the top layer (UseOutputTransform=Yes), or None: the codes are H_L."""
        self.layers = layers
        self.affine = affine
        self.output = output
        self.representation = representation
        kinds = {type(l).KIND for l in layers}
        if len(kinds) != 1:
            raise NotImplementedError("mixed graph-convolution layer types in one encoder")
        self.kind = kinds.pop()
        top = layers[-1]
        for i, l in enumerate(layers):
            if l.use_nonlinearity != (i < len(layers) - 1):
                raise NotImplementedError("only 'relu on all but the last layer' stacks are supported "
                                          "(model_builder.py:275)")
            if l.onehot_input != (i == 0 and affine is None):
                raise NotImplementedError("onehot_input belongs to the bottom layer of a stack without an input "
                                          "transform, and to no other (model_builder.py:277-283)")
        if affine is None and self.kind != "basis":
            raise NotImplementedError("UseInputTransform=No with Concatenation=Yes: the reference's one-hot branch of "
                                      "ConcatGcn cannot execute (gcn_basis_concat.py:18-19,42-46)")
        # SkipConnections=Highway: every layer carries its wrapper (extras/highway_layer.py), or none does
        self.highways = [getattr(l, 'highway_layer', None) for l in layers]
        if any(h is None for h in self.highways) and any(h is not None for h in self.highways):
            raise NotImplementedError("highway layers around some graph-convolution layers only (the reference's one-hot "
                                      "first layer gets none, model_builder.py:304: not built)")
        self.highway = self.highways[0] is not None
        if self.highway and affine is None:
            raise NotImplementedError("SkipConnections=Highway with UseInputTransform=No (the one-hot follow-up)")
        if self.kind == "basis_tdiag" and (self.highway or affine is None):
            raise NotImplementedError("DiagonalCoefficients=Yes with SkipConnections=Highway or UseInputTransform=No: "
                                      "BasisGcnTimesDiag runs on embedding input without highway layers only")
        if self.kind == "basis_pdiag" and (self.highway or affine is None):
            raise NotImplementedError("AddDiagonal=Yes with SkipConnections=Highway or UseInputTransform=No: "
                                      "BasisGcnWithDiag runs on embedding input without highway layers only")
        s = top.settings
        self.V, self.R = top.entity_count, top.relation_count
        self.d = int(top.shape[1])
        if output is not None and int(output.shape[0]) != self.d:
            raise ValueError("the output transform's shape %s does not start with InternalEncoderDimension %d"
                             % (list(output.shape), self.d))
        self.dc = int(output.shape[1]) if output is not None else self.d      # the code width
        norm = s['IncidenceNormalization'] if 'IncidenceNormalization' in s else 'intended'
        _native.norm_mode_value(norm)        # an unknown name: ValueError naming the accepted ones, before any engine exists
        device = int(s['Device']) if 'Device' in s else 0
        max_edges = max(int(top.edge_count), 1)
        if 'GraphBatchSize' in s:
            max_edges = max(max_edges, int(s['GraphBatchSize']))
        self.engine = _native.Engine(self.V, self.R, self.d, len(layers), self.kind, top.n_coefficients,
                                     keep_prob=top.dropout_keep_probability, norm_mode=norm,
                                     max_edges=max_edges, device=device,
                                     input_mode="embedding" if affine is not None else "onehot",
                                     skip="highway" if self.highway else "none",
                                     code_dim=self.dc if output is not None else None)
        self._state = None        # (graph version, mode) of the activations held by the engine
        self._dev = {}            # persistent device buffers of the fused train step (name -> DeviceBuffer)
        self._dec_reserved = 0
        self._rank_reserved = 0
        self._graph_version = None
        self.weights_version = 0
        self._fwd_weights_version = -1
        # move the weights into the engine (names follow rgcn_param_info)
        if affine is not None:
            affine.W.bind(*self._accessors("W_emb"))
            affine.b.bind(*self._accessors("b_emb"))
        for i, l in enumerate(layers, start=1):
            l.layer_index = i
            for var, base in l.engine_variables() + (self.highways[i - 1].engine_variables() if self.highway else []):
                var.bind(*self._accessors("%s%d" % (base, i)))
        if output is not None:
            output.W.bind(*self._accessors("W_out"))
            output.b.bind(*self._accessors("b_out"))

    def _accessors(self, name):
        eng = self.engine

        def getter():
            return eng.get_param(name)

        def setter(value):
            eng.set_param(name, value)
            self.weights_version += 1

        return getter, setter

    def forward(self, mode):
        ph = self.representation.X
        if ph.value is None:
            raise RuntimeError("graph_edges was not fed")
        if self._graph_version != ph.version:
            self.engine.set_graph(ph.value)
            self._graph_version = ph.version
            self._state = None
        key = (ph.version, mode, self.weights_version)
        if self._state != key:
            train = mode == 'train'
            seed = int(np.random.randint(0, 2 ** 31 - 1)) if train else 0
            self.engine.forward(train=train, seed=seed)
            self._state = key
        return self

    def activation(self, layer):
        return self.engine.activation(layer)

    def codes(self):
        """[V, code width]: H_L, or the output transform's result"""
        return self.engine.codes()

    # ---- fused device paths (include/rgcn.h: rgcn_train_step_device, rgcn_rank_device)
    def _upload(self, name, arr):
        """Device copy of `arr` in a persistent buffer that only ever grows."""
        arr = np.ascontiguousarray(arr)
        buf = self._dev.get(name)
        if buf is None or buf.nbytes < arr.nbytes:
            if buf is not None:
                buf.free()
            buf = _native.DeviceBuffer(self.engine, max(arr.nbytes, 16))
            self._dev[name] = buf
        if arr.nbytes:
            self.engine.copy_to_device(buf, arr)
        return buf

    def _buffer(self, name, nbytes):
        buf = self._dev.get(name)
        if buf is None or buf.nbytes < nbytes:
            if buf is not None:
                buf.free()
            buf = _native.DeviceBuffer(self.engine, max(nbytes, 16))
            self._dev[name] = buf
        return buf

    def _exclusive(self, known):
        """ExclusiveNegativeSampling: `known` (the training triples, the same array every iteration) moves to the device
        once (rgcn_known_positives_reserve) and the fused minibatch step's mode follows it; None: the plain sampler.
        Returns whether the stand-alone sampling call is to be the exclusive one."""
        on = known is not None
        if on and getattr(self, "_known", None) is not known:
            self.engine.known_positives_reserve(known)
            self._known = known
        if on != getattr(self, "_exclusive_on", False):
            self.engine.set_exclusive_negatives(on)
            self._exclusive_on = on
        return on

    def _typed(self, types, fused=False):
        """TypeConstrainedNegatives: `types` (the training triples, the same array every iteration) moves to the device
        once (rgcn_type_sets_reserve); None: corruptions over all entities.  fused: the minibatch step's mode follows
        (rgcn_set_typed_negatives).  Returns whether the stand-alone sampling call is to be the typed one."""
        on = types is not None
        cur = getattr(self, "_types", None)
        # (the same triples under another array object -- the sampler's and the scorer's -- are not reserved again: a
        # reserve restarts the count of open rows)
        if on and cur is not types and not (cur is not None and np.shape(cur) == np.shape(types)
                                            and np.array_equal(cur, types)):
            self.engine.type_sets_reserve(types)
            self._types = types
        if fused and on != getattr(self, "_typed_on", False):
            self.engine.set_typed_negatives(on)
            self._typed_on = on
        return on

    def _draw_negatives(self, bd, nb, rate, seed, xd, yd, known, relation_rate, types):
        """the stand-alone sampling call of train_step_device_negatives.  types: the entity rows come from the type sets
        (rgcn_negative_sample_typed_device); with relation rows as well, the call that writes those runs first and the
        typed entity rows replace the ones it drew (an entity row it could not resolve stays counted)."""
        exclusive, typed = self._exclusive(known), self._typed(types)
        if relation_rate or not typed:
            self.engine.negative_sample_device(bd, nb, rate, seed, xd, yd, exclusive=exclusive, relation_rate=relation_rate)
        if typed:
            self.engine.negative_sample_typed_device(bd, nb, rate, seed, xd, yd, exclusive=exclusive)
        if self._reciprocal():
            self.engine.reciprocal_rows_device(bd, nb, rate, relation_rate, seed, xd, yd)

    def negative_typed_open(self):
        """negative rows the typed sampler drew over all entities, since the type sets were reserved (0 without them)"""
        return self.engine.negative_typed_open() if getattr(self, "_types", None) is not None else 0

    def _relation_negatives(self, relation_rate):
        """RelationNegativeSampleRate: the fused minibatch step appends this many relation rows per batch edge
        (rgcn_set_relation_negatives); the engine is told when the rate changes.  Returns the rate."""
        relation_rate = int(relation_rate)
        if relation_rate != getattr(self, "_relation_rate", 0):
            self.engine.set_relation_negatives(relation_rate)
            self._relation_rate = relation_rate
        return relation_rate

    def set_reciprocal_relations(self, on):
        """[Decoder] ReciprocalRelations: (?, r, o) is asked of W_relation[R + r], and every later train step trains on a
        reciprocal batch -- the samplers' rows through the reciprocal pass, the inverse positives behind them
        (rgcn_set_reciprocal_relations); the engine is told when the setting changes."""
        on = bool(on)
        if on != getattr(self, "_reciprocal_want", False):
            self.engine.set_reciprocal_relations(on)
            self._reciprocal_want = on

    def _reciprocal(self):
        return 1 if getattr(self, "_reciprocal_want", False) else 0

    def _positives(self, y):
        """the positives that lead a caller's batch: the rows with label 1, but for the inverse positives at its end"""
        ones = int(np.count_nonzero(y == 1))
        return ones // 2 if self._reciprocal() else ones

    def set_relation_softmax(self, weight, known=None):
        """[Decoder] RelationSoftmaxWeight: the weight of the softmax-over-relations term every later train step adds
        (rgcn_set_relation_softmax) and, under ExclusiveNegativeSampling, the known positives its mask reads; 0: off."""
        self._relsm_weight, self._relsm_known = float(weight), known

    def _relation_softmax(self, num_positives):
        """before a step: the term's buffers, the index of its mask and the engine's setting follow what
        set_relation_softmax asked for; the engine is told only when something changed"""
        weight = getattr(self, "_relsm_weight", 0.0)
        known = getattr(self, "_relsm_known", None) if weight > 0 else None
        if weight > 0:
            # (an index the exclusive sampler reserved is the same training set: it serves the mask too)
            if known is not None and getattr(self, "_known", None) is None:
                self.engine.known_positives_reserve(known)
                self._known = known
            if num_positives > getattr(self, "_relsm_reserved", 0):
                self.engine.relation_softmax_reserve(num_positives)
                self._relsm_reserved = num_positives
        state = (weight, int(num_positives), known is not None) if weight > 0 else (0.0, 0, False)
        if state != getattr(self, "_relsm_state", (0.0, 0, False)):
            self.engine.set_relation_softmax(*state)
            self._relsm_state = state

    def set_entity_softmax(self, weight, known=None, positives=0):
        """[Decoder] EntitySoftmaxWeight: the weight of the softmax-over-entities term every later train step adds
        (rgcn_set_entity_softmax), under ExclusiveNegativeSampling the known positives its mask reads, and
        EntitySoftmaxPositives: how many leading positives of a step the term takes (0: all); weight 0: off."""
        self._entsm_weight, self._entsm_known, self._entsm_positives = float(weight), known, int(positives)

    def _entity_softmax(self, num_positives):
        """before a step: the term's buffers, the index of its mask and the engine's setting follow what
        set_entity_softmax asked for; the engine is told only when something changed"""
        weight = getattr(self, "_entsm_weight", 0.0)
        known = getattr(self, "_entsm_known", None) if weight > 0 else None
        limit = getattr(self, "_entsm_positives", 0)
        if limit > 0:
            num_positives = min(int(num_positives), limit)
        if weight > 0:
            # (an index the exclusive sampler or the relation term reserved is the same training set: it serves this mask too)
            if known is not None and getattr(self, "_known", None) is None:
                self.engine.known_positives_reserve(known)
                self._known = known
            if num_positives > getattr(self, "_entsm_reserved", 0):
                self.engine.entity_softmax_reserve(num_positives)
                self._entsm_reserved = num_positives
        state = (weight, int(num_positives), known is not None) if weight > 0 else (0.0, 0, False)
        if state != getattr(self, "_entsm_state", (0.0, 0, False)):
            self.engine.set_entity_softmax(*state)
            self._entsm_state = state

    def set_adversarial_temperature(self, temperature):
        """[General] AdversarialTemperature: every later train step weighs each negative by the softmax of its group's
        energies at this temperature (rgcn_set_adversarial_negatives); 0: off."""
        self._adv_temperature = float(temperature)

    def _adversarial(self, num_positives):
        """before a step: the engine's setting follows set_adversarial_temperature; told only when something changed"""
        temperature = getattr(self, "_adv_temperature", 0.0)
        state = (temperature, int(num_positives)) if temperature > 0 else (0.0, 0)
        if state != getattr(self, "_adv_state", (0.0, 0)):
            self.engine.set_adversarial_negatives(*state)
            self._adv_state = state

    def adversarial_weights(self):
        """the row weights of the last train step under AdversarialTemperature > 0 (RGCN_BUF_ADVERSARIAL_WEIGHTS)"""
        from . import _native
        return self.engine.read_buffer(_native.BUF_ADVERSARIAL_WEIGHTS)

    def negative_unresolved(self):
        """negative rows every entity was a known positive for, since the known positives were reserved (0 without them)"""
        return self.engine.negative_unresolved() if getattr(self, "_known", None) is not None else 0

    def negative_relation_unresolved(self):
        """relation rows every other relation was a known positive for, since the reserve (0 without known positives)"""
        return self.engine.negative_relation_unresolved() if getattr(self, "_known", None) is not None else 0

    def stage(self, graph_edges, batch=None):
        """Feed the NEXT train step while the current one runs: its triples go to the inactive one of two device
        buffer pairs without the host waiting (pinned staging), the message graph on the prefetch stream where
        rgcn_prefetch_graph_device then builds its structures beside the running step, the decoder batch (if the
        negatives are drawn on the device) on the main stream behind that step.  The step that is then asked to
        train on these very arrays (identity) finds everything in place."""
        g = np.ascontiguousarray(graph_edges, dtype=np.int32).reshape(-1, 3)
        if len(g) > self.engine.max_edges:
            return                                   # the step itself reports the error
        slot = getattr(self, "_slot", 0) ^ 1
        gd = self._buffer("graph%d" % slot, g.nbytes)
        self.engine.copy_to_device_async(gd, g, on_prefetch_stream=True)
        self.engine.prefetch_graph_device(gd, len(g))
        bd, nb = None, 0
        if batch is not None:
            b = np.ascontiguousarray(batch, dtype=np.int32).reshape(-1, 3)
            bd, nb = self._buffer("batch%d" % slot, b.nbytes), len(b)
            self.engine.copy_to_device_async(bd, b)
        self._staged = (graph_edges, batch, slot, gd, len(g), bd, nb)

    def _sampled_batch(self, mb, slot_name, on_prefetch_stream):
        """the graph batch of a device-sampled minibatch: drawn into a device buffer by the device sampler (or
        already drawn there by presample_minibatch)"""
        train, size, seed = mb.sample
        pre = getattr(self, "_presampled", None)
        if pre is not None and pre[0] is mb:
            self._presampled = None
            return pre[1], int(size)
        if getattr(self, "_nbr_graph", None) is not train:
            self.engine.neighborhood_reserve(train)        # the training graph moves to the device once
            self._nbr_graph = train
        bd = self._buffer(slot_name, 12 * int(size))
        self.engine.sample_neighborhood_device(int(size), int(seed), bd, on_prefetch_stream=on_prefetch_stream)
        return bd, int(size)

    def presample_minibatch(self, mb):
        """Draw the graph batch of the minibatch AFTER the staged one, on the prefetch stream behind the staged one's
        graph preparation.  Three buffers in turn: the step that runs reads one, the staged preparation read the
        second, this draw writes the third -- and it is ordered, on the prefetch stream, behind a preparation that
        waited for the step which last read that third buffer."""
        if getattr(mb, "sample", None) is None or int(mb.sample[1]) > self.engine.max_edges:
            return
        ring = getattr(self, "_sample_ring", 0)
        self._sample_ring = (ring + 1) % 3
        self._presampled = None
        bd, _ = self._sampled_batch(mb, "sampled%d" % ring, True)
        self._presampled = (mb, bd)

    def stage_minibatch(self, mb):
        """The device-dropout flavour of stage(): ONE upload (the graph batch; it is the edge-dropout input and the
        decoder's positives at once) on the prefetch stream, then the draw of the kept edges and the preparation of
        their graph there, beside the running step (rgcn_prefetch_graph_dropout_device).  A device-sampled minibatch
        has no upload at all: the batch itself is drawn there first (rgcn_sample_neighborhood_device)."""
        slot = getattr(self, "_slot", 0) ^ 1
        if getattr(mb, "sample", None) is not None:
            if int(mb.sample[1]) > self.engine.max_edges:
                return
            bd, nb = self._sampled_batch(mb, "mbatch%d" % slot, True)
        else:
            b = np.ascontiguousarray(mb.batch, dtype=np.int32).reshape(-1, 3)
            if len(b) > self.engine.max_edges:
                return
            bd, nb = self._buffer("mbatch%d" % slot, b.nbytes), len(b)
            self.engine.copy_to_device_async(bd, b, on_prefetch_stream=True)
        self.engine.prefetch_graph_dropout_device(bd, nb, mb.keep, mb.edge_seed)
        self._staged = (mb, None, slot, bd, nb, None, 0)

    def train_step_minibatch(self, mb, reg_param, seed):
        """One iteration from a graph batch resident on the device: edge dropout, negative sampling and the train
        step in one asynchronous call (rgcn_train_step_minibatch_device)."""
        sampled = getattr(mb, "sample", None) is not None
        if sampled:
            nb = int(mb.sample[1])
        else:
            b = np.ascontiguousarray(mb.batch, dtype=np.int32).reshape(-1, 3)
            nb = len(b)
        relation_rate = int(getattr(mb, "relation_rate", 0))
        n = nb * (int(mb.rate) + 1 + relation_rate + self._reciprocal())
        if n == 0:
            raise ValueError("empty decoder batch")
        if nb > self.engine.max_edges:
            raise ValueError("graph batch of %d edges exceeds the context's max_edges %d"
                             % (nb, self.engine.max_edges))
        if n > self._dec_reserved:
            self.engine.decoder_reserve(n)
            self._dec_reserved = n
        st = self._take_staged(mb, None)
        if st is not None:
            bd = st[3]
        elif sampled:
            bd, _ = self._sampled_batch(mb, "mbatch", False)
        else:
            bd = self._upload("mbatch", b)
        xd, yd = self._buffer("X", 12 * n), self._buffer("Y", 4 * n)
        self._exclusive(getattr(mb, "known", None))
        self._typed(getattr(mb, "types", None), fused=True)
        self._relation_negatives(relation_rate)
        self._relation_softmax(nb)
        self._entity_softmax(nb)
        self._adversarial(nb)
        self.engine.train_step_minibatch_device(bd, nb, mb.keep, mb.edge_seed, mb.rate, seed ^ 0x5bd1e995, xd, yd,
                                                seed=seed, reg_param=reg_param)
        self._state = None
        self._graph_version = None
        self.weights_version += 1

    def _take_staged(self, graph_edges, batch):
        st = getattr(self, "_staged", None)
        self._staged = None
        if st is not None and st[0] is graph_edges and st[1] is batch:
            self._slot = st[2]
            return st
        return None

    def configure_optimizer(self, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, max_grad_norm=0.0,
                            algorithm="Adam", initial_accumulator=0.1):
        self.engine.optimizer_config(learning_rate, beta1, beta2, epsilon, max_grad_norm, algorithm=algorithm,
                                     initial_accumulator=initial_accumulator)

    def train_step(self, graph_edges, x, y, reg_param, seed):
        """One update_from_batch (optimize.py:81-88) on the device: graph prep, encoder forward, DistMult
        loss + gradients, encoder backward, clip + Adam.  Asynchronous; `loss()` synchronises."""
        g = np.ascontiguousarray(graph_edges, dtype=np.int32).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 3)
        y = np.ascontiguousarray(y, dtype=np.float32).ravel()
        if len(x) != len(y) or len(x) == 0:
            raise ValueError("decoder batch: X [N,3] and Y [N] must have the same non-zero length")
        if len(g) > self.engine.max_edges:
            raise ValueError("graph batch of %d edges exceeds the context's max_edges %d"
                             % (len(g), self.engine.max_edges))
        if len(x) > self._dec_reserved:
            self.engine.decoder_reserve(len(x))
            self._dec_reserved = len(x)
        st = self._take_staged(graph_edges, None)
        gd = st[3] if st is not None else self._upload("graph", g)
        xd, yd = self._upload("X", x), self._upload("Y", y)
        self._relation_softmax(self._positives(y))      # (the sampler's positives lead the batch)
        self._entity_softmax(self._positives(y))
        self._adversarial(self._positives(y))
        self.engine.train_step_device(gd, len(g), xd, yd, len(x), seed=seed, reg_param=reg_param)
        self._state = None            # activations now belong to this train step's graph
        self._graph_version = None
        self.weights_version += 1

    def train_step_device_negatives(self, graph_edges, batch, rate, reg_param, seed, known=None, relation_rate=0,
                                    types=None):
        """As train_step, with the decoder batch (positives + `rate` corruptions each) drawn on the device from
        `batch` (rgcn_negative_sample_device): only the two triple lists cross the PCIe bus.  known: the known positives
        the corruptions avoid (rgcn_negative_sample_exclusive_device), None for the plain sampler.  relation_rate: relation
        corruptions per positive behind them (rgcn_negative_sample_relation_device).  types: the triples whose per-relation
        entity sets the corruptions are drawn from (rgcn_negative_sample_typed_device), None for all entities."""
        g = np.ascontiguousarray(graph_edges, dtype=np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(batch, dtype=np.int32).reshape(-1, 3)
        relation_rate = int(relation_rate)
        n = len(b) * (int(rate) + 1 + relation_rate + self._reciprocal())
        if n == 0:
            raise ValueError("empty decoder batch")
        if len(g) > self.engine.max_edges:
            raise ValueError("graph batch of %d edges exceeds the context's max_edges %d"
                             % (len(g), self.engine.max_edges))
        if n > self._dec_reserved:
            self.engine.decoder_reserve(n)
            self._dec_reserved = n
        st = self._take_staged(graph_edges, batch)
        if st is not None:
            gd, bd = st[3], st[5]
        else:
            gd, bd = self._upload("graph", g), self._upload("batch", b)
        for name, nbytes in (("X", 12 * n), ("Y", 4 * n)):
            buf = self._dev.get(name)
            if buf is None or buf.nbytes < nbytes:
                if buf is not None:
                    buf.free()
                self._dev[name] = _native.DeviceBuffer(self.engine, nbytes)
        xd, yd = self._dev["X"], self._dev["Y"]
        self._draw_negatives(bd, len(b), rate, seed ^ 0x5bd1e995, xd, yd, known, relation_rate, types)
        self._relation_softmax(len(b))
        self._entity_softmax(len(b))
        self._adversarial(len(b))
        self.engine.train_step_device(gd, len(g), xd, yd, n, seed=seed, reg_param=reg_param)
        self._state = None
        self._graph_version = None
        self.weights_version += 1

    def loss(self):
        return self.engine.loss()

    def _scoring_engine(self, chunk):
        """the engine after a test-mode forward over the fed graph, with room for `chunk` queries at a time"""
        self.forward('test')
        if self._rank_reserved < chunk:
            self.engine.rank_reserve(chunk)
            self._rank_reserved = chunk
        return self.engine

    def ranks(self, triples, predict_object, filter_ptr, filter_idx, chunk=2048):
        """Raw / filtered ranks on the codes of a test-mode forward over the fed graph."""
        return self._scoring_engine(chunk).ranks(triples, predict_object, filter_ptr, filter_idx)

    def ranks_typed(self, triples, predict_object, filter_ptr, filter_idx, types, chunk=2048):
        """ranks() among the entities the per-relation sets of `types` (the training triples) hold for the predicted slot,
        and the gold entity (rgcn_rank_typed_device)."""
        engine = self._scoring_engine(chunk)
        self._typed(types)
        return engine.ranks_typed(triples, predict_object, filter_ptr, filter_idx)

    def topk_typed(self, queries, predict_object, k, types, exclude_ptr=None, exclude_idx=None, chunk=2048):
        """topk() among the entities the per-relation sets of `types` hold for the predicted slot
        (rgcn_topk_typed_device)."""
        engine = self._scoring_engine(chunk)
        self._typed(types)
        return engine.topk_typed(queries, predict_object, k, exclude_ptr, exclude_idx)

    def ranks_mixed(self, triples, predict_object, partner, weight, filter_ptr, filter_idx, chunk=2048):
        """ranks() on weight * own score + (1 - weight) * partner score (rgcn_rank_mixed_device); partner: the other
        model's [N, V] energies for the same triples, an array or a device address; N <= chunk."""
        return self._scoring_engine(chunk).ranks_mixed(triples, predict_object, partner, weight, filter_ptr, filter_idx)

    def topk(self, queries, predict_object, k, exclude_ptr=None, exclude_idx=None, chunk=2048):
        """The k best completions of every query, best first, on the codes of a test-mode forward over the fed graph
        (rgcn_topk_device): (entity ids int32 [N,k], energies float32 [N,k])."""
        return self._scoring_engine(chunk).topk(queries, predict_object, k, exclude_ptr, exclude_idx)

    def score_queries(self, queries, predict_object, chunk=2048):
        """The energies of every entity for each query, left in the engine's score buffer (rgcn_score_queries_device):
        what another runtime's topk_mixed reads through engine.rank_energies_device(); N <= chunk."""
        self._scoring_engine(chunk).score_queries(queries, predict_object)

    def topk_mixed(self, queries, predict_object, k, partner, weight, exclude_ptr=None, exclude_idx=None, chunk=2048):
        """topk() on weight * own score + (1 - weight) * partner score (rgcn_topk_mixed_device): (entity ids int32 [N,k],
        mixed scores float32 [N,k]); partner: the other model's [N, V] energies for the same queries, an array or a
        device address; N <= chunk."""
        return self._scoring_engine(chunk).topk_mixed(queries, predict_object, k, partner, weight, exclude_ptr, exclude_idx)

    def ranks_relation(self, triples, filter_ptr, filter_idx, chunk=2048):
        """Raw / filtered ranks of the gold relation among all relations between each triple's subject and object
        (rgcn_rank_relation_device), on the codes of a test-mode forward over the fed graph."""
        return self._scoring_engine(chunk).ranks_relation(triples, filter_ptr, filter_idx)

    def topk_relation(self, queries, k, exclude_ptr=None, exclude_idx=None, chunk=2048):
        """The k best relations between the subject and object of every query, best first (rgcn_topk_relation_device):
        (relation ids int32 [N,k], energies float32 [N,k])."""
        return self._scoring_engine(chunk).topk_relation(queries, k, exclude_ptr, exclude_idx)

    def score_relation_queries(self, queries, chunk=2048):
        """The energies of every relation for each query's pair, left in the engine's relation buffer
        (rgcn_score_relation_queries_device; engine.relation_energies_device() is its address); N <= chunk."""
        self._scoring_engine(chunk).score_relation_queries(queries)

    def backward(self, dcodes):
        if self._state is None or self._state[1] != 'train':
            raise RuntimeError("backward() needs a train-mode forward pass on the current graph")
        self.engine.backward(dcodes)
        return self

    def grad(self, name):
        return self.engine.get_grad(name)


class EmbeddingRuntime(EncoderRuntime):
    """The graph-less runtime of `Name=embedding` (the DistMult baseline): ONE RGCN_KIND_EMBEDDING engine context, owned by
    the lookup AffineTransform at the bottom of the chain.  The codes are W_emb itself; a step is the decoder's loss and
    gradients, clip and Adam (rgcn_train_step_device without a graph).  EncoderRuntime's method names and meanings; the
    `graph_edges` arguments are None."""

    def __init__(self, affine):
        self.layers, self.affine, self.representation = [], affine, None
        self.kind = "embedding"
        self.highway = False
        s = affine.settings
        self.V, self.R = affine.entity_count, affine.relation_count
        self.d = self.dc = int(affine.shape[1])
        self.output = None
        device = int(s['Device']) if 'Device' in s else 0
        self.engine = _native.Engine(self.V, self.R, self.d, 0, "embedding", 1, keep_prob=1.0, max_edges=0, device=device)
        self._state = None
        self._dev = {}
        self._dec_reserved = 0
        self._rank_reserved = 0
        self._graph_version = None
        self.weights_version = 0
        self._resident = None         # the positives array whose device copy is in self._dev["batch"]
        affine.W.bind(*self._accessors("W_emb"))
        affine.b.bind(*self._accessors("b_emb"))

    def forward(self, mode):
        key = (0, mode, self.weights_version)
        if self._state != key:
            self.engine.forward(train=mode == 'train', seed=0)
            self._state = key
        return self

    def stage(self, graph_edges, batch=None):
        pass

    def train_step(self, graph_edges, x, y, reg_param, seed):
        if graph_edges is not None:
            raise ValueError("a graph-less encoder takes no graph_edges")
        x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 3)
        y = np.ascontiguousarray(y, dtype=np.float32).ravel()
        if len(x) != len(y) or len(x) == 0:
            raise ValueError("decoder batch: X [N,3] and Y [N] must have the same non-zero length")
        if len(x) > self._dec_reserved:
            self.engine.decoder_reserve(len(x))
            self._dec_reserved = len(x)
        xd, yd = self._upload("X", x), self._upload("Y", y)
        self._relation_softmax(self._positives(y))
        self._entity_softmax(self._positives(y))
        self._adversarial(self._positives(y))
        self.engine.train_step_device(None, 0, xd, yd, len(x), seed=seed, reg_param=reg_param)
        self._state = None
        self.weights_version += 1

    def train_step_device_negatives(self, graph_edges, batch, rate, reg_param, seed, known=None, relation_rate=0,
                                    types=None):
        """The positives are uploaded once and stay resident while the SAME array object is fed (the training set, every
        iteration); the corruptions are drawn on the device, avoiding `known` if given, `relation_rate` relation
        corruptions per positive behind them, from the type sets of `types` if given.  A caller that rewrites the array in
        place feeds a new one."""
        if graph_edges is not None:
            raise ValueError("a graph-less encoder takes no graph_edges")
        nb = len(batch)
        relation_rate = int(relation_rate)
        n = nb * (int(rate) + 1 + relation_rate + self._reciprocal())
        if n == 0:
            raise ValueError("empty decoder batch")
        if n > self._dec_reserved:
            self.engine.decoder_reserve(n)
            self._dec_reserved = n
        if self._resident is not batch or "batch" not in self._dev:
            self._upload("batch", np.ascontiguousarray(batch, dtype=np.int32).reshape(-1, 3))
            self._resident = batch
        xd, yd = self._buffer("X", 12 * n), self._buffer("Y", 4 * n)
        self._draw_negatives(self._dev["batch"], nb, rate, seed ^ 0x5bd1e995, xd, yd, known, relation_rate, types)
        self._relation_softmax(nb)
        self._entity_softmax(nb)
        self._adversarial(nb)
        self.engine.train_step_device(None, 0, xd, yd, n, seed=seed, reg_param=reg_param)
        self._state = None
        self.weights_version += 1

    def _no_graph(self, *args, **kwargs):
        raise NotImplementedError("a graph-less encoder (Name=embedding) has no graph batches to stage, sample or drop edges from")

    stage_minibatch = presample_minibatch = train_step_minibatch = _no_graph
