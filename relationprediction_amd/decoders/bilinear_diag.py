"""DistMult decoder (reference: code/decoders/bilinear_diag.py).

energy = sum_k e1_k r_k e2_k over the gathered codes (:18-21,30); loss = mean sigmoid cross-entropy
with pos_weight forced to 1 (:32-34); regulariser = RegularizationParameter x (mean(e1^2) + mean(r^2) +
mean(e2^2)) (:63-69); scoring against every entity as `sigmoid(codes . (r*e2)^T)` (:46-61).

BASELINE.json: "the DistMult decoder and negative-sampling loss stay as-is".  The call-by-call surface of
the reference (get_loss, predict_*, backward) is evaluated eagerly in numpy on codes the engine computed;
the training driver and the scorer use the fused device paths below (csrc/decoder.hip,
csrc/optimizer.hip, csrc/ranking.hip).
"""
import numpy as np

from ..model import Model, Placeholder


def _sigmoid(x):
    x = np.asarray(x, dtype=np.float32)
    e = np.exp(-np.abs(x))                       # never overflows
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).astype(np.float32)


def parse_relation_softmax_weight(settings):
    """[Decoder] RelationSoftmaxWeight=lambda (not in the reference; absent: 0): the weight of the softmax-over-relations
    loss term of the positives (include/rgcn.h, rgcn_relation_softmax_device).  A non-negative finite float."""
    if 'RelationSoftmaxWeight' not in settings:
        return 0.0
    value = settings['RelationSoftmaxWeight']
    try:
        if isinstance(value, bool):
            raise ValueError
        weight = float(str(value).strip())
    except ValueError:
        raise ValueError("Decoder.RelationSoftmaxWeight must be a non-negative number, not %r" % (value,))
    if not np.isfinite(weight) or weight < 0:
        raise ValueError("Decoder.RelationSoftmaxWeight must be a non-negative finite number, not %r" % (value,))
    return weight


def parse_entity_softmax_weight(settings):
    """[Decoder] EntitySoftmaxWeight=lambda (not in the reference; absent: 0): the weight of the softmax-over-entities loss
    term of the positives (include/rgcn.h, rgcn_entity_softmax_device).  A non-negative finite float."""
    if 'EntitySoftmaxWeight' not in settings:
        return 0.0
    value = settings['EntitySoftmaxWeight']
    try:
        if isinstance(value, bool):
            raise ValueError
        weight = float(str(value).strip())
    except ValueError:
        raise ValueError("Decoder.EntitySoftmaxWeight must be a non-negative number, not %r" % (value,))
    if not np.isfinite(weight) or weight < 0:
        raise ValueError("Decoder.EntitySoftmaxWeight must be a non-negative finite number, not %r" % (value,))
    return weight


def parse_entity_softmax_positives(settings):
    """[Decoder] EntitySoftmaxPositives=k (absent: 0, meaning all): the term takes the leading min(k, P) positives of a
    step -- batches are drawn at random, so a uniform subsample.  A non-negative integer."""
    if 'EntitySoftmaxPositives' not in settings:
        return 0
    value = settings['EntitySoftmaxPositives']
    try:
        if isinstance(value, (bool, float)):
            raise ValueError
        k = int(str(value).strip())
    except ValueError:
        raise ValueError("Decoder.EntitySoftmaxPositives must be a non-negative integer, not %r" % (value,))
    if k < 0:
        raise ValueError("Decoder.EntitySoftmaxPositives must be a non-negative integer, not %r" % (value,))
    return k


def parse_reciprocal_relations(settings):
    """[Decoder] ReciprocalRelations=Yes|No (not in the reference; absent: No): every relation gets a second vector,
    W_relation[RelationCount + r], which answers (?, r, o) while W_relation[r] answers (s, r, ?) (include/rgcn.h,
    rgcn_set_reciprocal_relations).  Refused with EntitySoftmaxWeight > 0 and where W_relation has too few rows."""
    value = settings['ReciprocalRelations'] if 'ReciprocalRelations' in settings else 'No'
    if value not in ('Yes', 'No'):
        raise ValueError("Decoder.ReciprocalRelations must be Yes or No, not %r" % (value,))
    if value == 'No':
        return False
    if parse_entity_softmax_weight(settings) > 0:
        raise ValueError("Decoder.ReciprocalRelations = Yes with Decoder.EntitySoftmaxWeight > 0: the entity-softmax term is "
                         "not built for the inverse relations' rows; drop one of the two keys")
    if 'RelationCount' in settings and 'EntityCount' in settings \
            and 2 * int(settings['RelationCount']) > int(settings['EntityCount']):
        raise ValueError("Decoder.ReciprocalRelations = Yes needs 2 x RelationCount <= EntityCount (W_relation has one row "
                         "per entity): the dataset has %d relations and %d entities"
                         % (int(settings['RelationCount']), int(settings['EntityCount'])))
    return True


def reciprocal_row_weights(energies, labels, temperature, reciprocal):
    """adversarial_row_weights for a batch that may end in its inverse positives (ReciprocalRelations=Yes: the last n of its
    2 n rows with label 1): the weights of the rows in front of them, and 1 for them."""
    if not reciprocal:
        return adversarial_row_weights(energies, labels, temperature)
    z = np.asarray(labels).reshape(-1)
    n = int(np.count_nonzero(z == 1)) // 2
    head = len(z) - n
    if n == 0 or not (z[head:] == 1).all():
        raise ValueError("a reciprocal batch ends in its inverse positives (label 1), as many as it has positives in front")
    x = np.asarray(energies, dtype=np.float32).reshape(-1)
    return np.concatenate([adversarial_row_weights(x[:head], z[:head], temperature), np.ones(n, dtype=np.float32)])


def parse_adversarial_temperature(settings):
    """[General] AdversarialTemperature=alpha (not in the reference; absent: 0): the temperature of the self-adversarial
    weights of the negatives (include/rgcn.h, rgcn_set_adversarial_negatives).  A non-negative finite float."""
    if 'AdversarialTemperature' not in settings:
        return 0.0
    value = settings['AdversarialTemperature']
    try:
        if isinstance(value, bool):
            raise ValueError
        alpha = float(str(value).strip())
    except ValueError:
        raise ValueError("General.AdversarialTemperature must be a non-negative number, not %r" % (value,))
    if not np.isfinite(alpha) or alpha < 0:
        raise ValueError("General.AdversarialTemperature must be a non-negative finite number, not %r" % (value,))
    return alpha


def adversarial_row_weights(energies, labels, temperature):
    """The numpy port of csrc/adversarial_weights.h over a whole batch: float32 weights [N] from float32 energies.  The
    batch is laid out as the samplers write it -- P = the leading rows with label 1, every later row i a negative of
    positive i mod P, K = N / P - 1 -- and a negative's weight is K times the softmax of temperature x energy over its
    group, evaluated in float64 and rounded once; a positive's weight is 1.  ValueError for any other layout."""
    x = np.asarray(energies, dtype=np.float32).reshape(-1)
    z = np.asarray(labels).reshape(-1)
    N = len(x)
    w = np.ones(N, dtype=np.float32)
    P = int(np.count_nonzero(z == 1))
    if temperature == 0 or N == 0:
        return w
    if P == 0 or N % P != 0 or not (z[:P] == 1).all() or not (z[P:] == 0).all():
        raise ValueError("adversarial weights need the positives (label 1) first and a whole number of negatives "
                         "(label 0) per positive behind them: %d rows, %d with label 1" % (N, P))
    K = N // P - 1
    if K == 0:
        return w
    a = np.float64(np.float32(temperature)) * x[P:].astype(np.float64).reshape(K, P)
    t = np.exp(a - a.max(axis=0, keepdims=True))
    w[P:] = (K * t / t.sum(axis=0, keepdims=True)).astype(np.float32).reshape(-1)
    return w


def relation_softmax_terms(codes, relation_codes, positives, relation_count, weight):
    """The unmasked term evaluated eagerly in float64: (term, dcodes [V,dc], d_rel [rows of relation_codes, dc])."""
    pos = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    c = np.asarray(codes, dtype=np.float64)
    W = np.asarray(relation_codes, dtype=np.float64)
    P = len(pos)
    dcodes, d_rel = np.zeros_like(c), np.zeros_like(W)
    if P == 0 or weight == 0:
        return 0.0, dcodes, d_rel
    q = (np.asarray(codes, dtype=np.float32)[pos[:, 0]] * np.asarray(codes, dtype=np.float32)[pos[:, 2]]).astype(np.float64)
    E = q @ W[:relation_count].T
    m = E.max(axis=1, keepdims=True)
    ex = np.exp(E - m)
    ssum = ex.sum(axis=1, keepdims=True)
    ell = np.log(ssum[:, 0]) + m[:, 0] - E[np.arange(P), pos[:, 1]]
    G = ex / ssum
    G[np.arange(P), pos[:, 1]] -= 1.0
    G *= weight / P
    d_rel[:relation_count] = G.T @ q
    dq = G @ W[:relation_count]
    np.add.at(dcodes, pos[:, 0], dq * c[pos[:, 2]])
    np.add.at(dcodes, pos[:, 2], dq * c[pos[:, 0]])
    return weight / P * float(ell.sum()), dcodes, d_rel


def entity_softmax_terms(codes, relation_codes, positives, weight):
    """The unmasked entity-softmax term evaluated eagerly in float64 (the numpy port of csrc/entity_softmax.hip): every
    positive gives an object row (query s, gold o) and a subject row (query o, gold s), each the cross-entropy of its gold
    entity against all.  Returns (term, dcodes [V,dc], d_rel [rows of relation_codes, dc])."""
    pos = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    c32 = np.asarray(codes, dtype=np.float32)
    c = c32.astype(np.float64)
    W = np.asarray(relation_codes, dtype=np.float64)
    P = len(pos)
    dcodes, d_rel = np.zeros_like(c), np.zeros_like(W)
    if P == 0 or weight == 0:
        return 0.0, dcodes, d_rel
    a = np.concatenate([pos[:, 0], pos[:, 2]])
    g = np.concatenate([pos[:, 2], pos[:, 0]])
    r = np.concatenate([pos[:, 1], pos[:, 1]])
    q = (c32[a] * np.asarray(relation_codes, dtype=np.float32)[r]).astype(np.float64)      # rounded once, as the device's
    E = q @ c.T
    m = E.max(axis=1, keepdims=True)
    ex = np.exp(E - m)
    ssum = ex.sum(axis=1, keepdims=True)
    rows = np.arange(2 * P)
    ell = np.log(ssum[:, 0]) + m[:, 0] - E[rows, g]
    G = ex / ssum
    G[rows, g] -= 1.0
    G *= weight / (2 * P)
    dcodes += G.T @ q
    dq = G @ c
    np.add.at(dcodes, a, dq * W[r])
    np.add.at(d_rel, r, dq * c[a])
    return weight / (2 * P) * float(ell.sum()), dcodes, d_rel


class BilinearDiag(Model):
    X = None
    Y = None
    relation_softmax_known = None      # the known positives the term's mask reads (ExclusiveNegativeSampling=Yes)

    def parse_settings(self):
        self.regularization_parameter = float(self.settings['RegularizationParameter'])
        self.relation_softmax_weight = parse_relation_softmax_weight(self.settings)
        self.adversarial_temperature = parse_adversarial_temperature(self.settings)
        self.entity_softmax_weight = parse_entity_softmax_weight(self.settings)
        self.entity_softmax_positives = parse_entity_softmax_positives(self.settings)
        self.reciprocal = parse_reciprocal_relations(self.settings)

    def _forward_positives(self, x, z):
        """the rows with label 1 that the softmax terms take: under ReciprocalRelations the first half of them -- the
        inverse positives at the end of the batch carry relations >= RelationCount, which are no candidates"""
        pos = np.asarray(x)[np.asarray(z) == 1]
        return pos[:len(pos) // 2] if self.reciprocal else pos

    def _entity_softmax_rows(self, x, z):
        """the positives the eager entity-softmax term takes: the rows with label 1, the leading EntitySoftmaxPositives"""
        pos = np.asarray(x)[np.asarray(z) == 1]
        return pos[:self.entity_softmax_positives] if self.entity_softmax_positives > 0 else pos

    def set_relation_softmax_known(self, known):
        """the triples whose relations leave a pair's candidate set on the device paths (the training set, under
        ExclusiveNegativeSampling=Yes); None: every relation competes"""
        self.relation_softmax_known = None if known is None else np.ascontiguousarray(known, dtype=np.int32)

    def _relation_softmax(self):
        """tell the runtime the term's weight and mask before a device step (nothing to tell while the key is absent)"""
        rt = self._runtime()
        if self.relation_softmax_weight > 0 or getattr(rt, "_relsm_weight", 0.0) > 0:
            rt.set_relation_softmax(self.relation_softmax_weight, self.relation_softmax_known)
        if self.adversarial_temperature > 0 or getattr(rt, "_adv_temperature", 0.0) > 0:
            rt.set_adversarial_temperature(self.adversarial_temperature)
        if self.entity_softmax_weight > 0 or getattr(rt, "_entsm_weight", 0.0) > 0:
            # (the mask reads the same known positives as the relation term's: ExclusiveNegativeSampling=Yes)
            rt.set_entity_softmax(self.entity_softmax_weight, self.relation_softmax_known, self.entity_softmax_positives)
        return rt

    def _runtime(self):
        """the encoder's runtime, told whether relations are reciprocal (nothing to tell while the key is absent)"""
        rt = self.next_component.get_runtime()
        if self.reciprocal or getattr(rt, "_reciprocal_want", False):
            rt.set_reciprocal_relations(self.reciprocal)
        return rt

    def local_initialize_train(self):
        self.Y = Placeholder('Y', np.float32)
        self.X = Placeholder('X', np.int32, ncols=3)

    def local_get_train_input_variables(self):
        return [self.X, self.Y]

    def local_get_test_input_variables(self):
        return [self.X]

    def compute_codes(self, mode='train'):
        subject_codes, relation_codes, object_codes = self.next_component.get_all_codes(mode=mode)
        x = self.X.value
        return subject_codes[x[:, 0]], relation_codes[x[:, 1]], object_codes[x[:, 2]]

    def get_loss(self, mode='train'):
        e1s, rs, e2s = self.compute_codes(mode=mode)
        energies = np.sum(e1s * rs * e2s, axis=1)
        z = self.Y.value
        # tf.nn.weighted_cross_entropy_with_logits(targets=z, logits=x, pos_weight=1)
        per = (1 - z) * energies + np.log1p(np.exp(-np.abs(energies))) + np.maximum(-energies, 0)
        if self.adversarial_temperature > 0:
            per = reciprocal_row_weights(energies, z, self.adversarial_temperature, self.reciprocal) * per
        loss = float(np.mean(per, dtype=np.float64))
        if self.relation_softmax_weight > 0:
            # the unmasked softmax-over-relations term over the rows with label 1 (the device paths' small-size cross-check)
            subject_codes, relation_codes, _ = self.next_component.get_all_codes(mode=mode)
            loss += relation_softmax_terms(subject_codes, relation_codes, self._forward_positives(self.X.value, z),
                                           self.relation_count, self.relation_softmax_weight)[0]
        if self.entity_softmax_weight > 0:
            # the unmasked softmax-over-entities term over the rows with label 1 (the device paths' small-size cross-check)
            subject_codes, relation_codes, _ = self.next_component.get_all_codes(mode=mode)
            loss += entity_softmax_terms(subject_codes, relation_codes, self._entity_softmax_rows(self.X.value, z),
                                         self.entity_softmax_weight)[0]
        return loss

    def local_get_regularization(self):
        e1s, rs, e2s = self.compute_codes(mode='train')
        reg = np.mean(np.square(e1s), dtype=np.float64) + np.mean(np.square(rs), dtype=np.float64) \
            + np.mean(np.square(e2s), dtype=np.float64)
        return self.regularization_parameter * float(reg)

    def predict(self):
        e1s, rs, e2s = self.compute_codes(mode='test')
        return _sigmoid(np.sum(e1s * rs * e2s, axis=1))

    def predict_all_subject_scores(self):
        e1s, rs, e2s = self.compute_codes(mode='test')
        if self.reciprocal:
            # (?, r, o) is asked of the inverse relation's vector, W_relation[RelationCount + r]
            relation_codes = self.next_component.get_all_codes(mode='test')[1]
            rs = relation_codes[self.X.value[:, 1] + self.relation_count]
        all_subject_codes = self.next_component.get_all_subject_codes(mode='test')
        return _sigmoid(np.matmul(all_subject_codes, (rs * e2s).T).T)

    def predict_all_object_scores(self):
        e1s, rs, e2s = self.compute_codes(mode='test')
        all_object_codes = self.next_component.get_all_object_codes(mode='test')
        return _sigmoid(np.matmul(e1s * rs, all_object_codes.T))

    def predict_all_relation_scores(self):
        """score of every relation between the subject and object of the triples fed to X: [N, RelationCount]"""
        e1s, rs, e2s = self.compute_codes(mode='test')
        relation_codes = self.next_component.get_all_codes(mode='test')[1]
        return _sigmoid(np.matmul(e1s * e2s, relation_codes[:self.relation_count].T))

    # ---- fused device paths: what the training driver and the scorer use (the eager numpy methods above
    # keep the reference's call-by-call surface and serve as their small-size cross-check)
    def configure_device_optimizer(self, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, max_grad_norm=0.0,
                                   algorithm="Adam", initial_accumulator=0.1):
        self.next_component.get_runtime().configure_optimizer(learning_rate, beta1, beta2, epsilon, max_grad_norm,
                                                              algorithm=algorithm,
                                                              initial_accumulator=initial_accumulator)

    def device_optimizer_engine(self):
        """the engine whose optimizer state Model.save_optimizer / load_optimizer read and write"""
        return self._runtime().engine

    def device_train_step(self, graph_edges, x, y, seed):
        """loss + regularisation, all gradients, clip and Adam in one asynchronous device step (graph_edges None: a
        graph-less encoder, Name=embedding)."""
        self._relation_softmax().train_step(graph_edges, x, y, self.regularization_parameter, seed)

    def device_train_step_negatives(self, graph_edges, batch, rate, seed, known=None, relation_rate=0, types=None):
        """device_train_step with the negatives drawn on the device from `batch`; known: the known positives they avoid
        (ExclusiveNegativeSampling=Yes), None for the plain sampler; relation_rate: relation corruptions per positive
        (RelationNegativeSampleRate); types: the triples whose per-relation entity sets the corruptions come from
        (TypeConstrainedNegatives=Yes), None for all entities."""
        extra = {} if types is None else {'types': types}
        self._relation_softmax().train_step_device_negatives(graph_edges, batch, rate, self.regularization_parameter, seed,
                                                             known=known, relation_rate=relation_rate, **extra)

    def device_negative_typed_open(self):
        """negative rows the typed device sampler drew over all entities since its type sets were reserved"""
        return self.next_component.get_runtime().negative_typed_open()

    def device_negative_unresolved(self):
        """negative rows the exclusive device sampler could not resolve since its known positives were reserved"""
        return self.next_component.get_runtime().negative_unresolved()

    def device_negative_relation_unresolved(self):
        """relation rows the exclusive device sampler could not resolve since its known positives were reserved"""
        return self.next_component.get_runtime().negative_relation_unresolved()

    def device_stage(self, graph_edges, batch=None):
        """feed the next train step beside the running one (runtime.stage); a graph-less encoder has nothing to stage"""
        if graph_edges is None:
            return
        self.next_component.get_runtime().stage(graph_edges, batch)

    def device_train_step_minibatch(self, minibatch, seed):
        """the whole iteration from the graph batch on: edge dropout, negatives, train step, all on the device"""
        self._relation_softmax().train_step_minibatch(minibatch, self.regularization_parameter, seed)

    def device_stage_minibatch(self, minibatch):
        self.next_component.get_runtime().stage_minibatch(minibatch)

    def device_presample_minibatch(self, minibatch):
        self.next_component.get_runtime().presample_minibatch(minibatch)

    def device_loss(self):
        return self.next_component.get_runtime().loss()

    def _scoring_runtime(self, graph):
        """the runtime with `graph` fed: re-encoded only when the graph or the weights changed"""
        variables = self.get_test_input_variables()
        if self.needs_graph() and (getattr(self, '_ranks_graph', None) is not graph or variables[0].value is None):
            variables[0].feed(graph)
            self._ranks_graph = graph
        return self._runtime()

    def device_ranks(self, graph, triplets, predict_object, filter_ptr, filter_idx):
        """Ranks of the gold subjects / objects of `triplets` against every entity, codes from a test-mode
        pass over `graph` (what score_all_subjects / score_all_objects + MrrScore.append_line compute)."""
        return self._scoring_runtime(graph).ranks(triplets, predict_object, filter_ptr, filter_idx)

    def device_ranks_typed(self, graph, triplets, predict_object, filter_ptr, filter_idx, types):
        """device_ranks among the entities that `types` (the training triples) have seen in the predicted slot of each
        triple's relation, and the gold entity (rgcn_rank_typed_device): type-constrained ranks."""
        return self._scoring_runtime(graph).ranks_typed(triplets, predict_object, filter_ptr, filter_idx, types)

    def device_topk_typed(self, graph, queries, predict_object, k, types, exclude_ptr=None, exclude_idx=None):
        """device_topk among the entities that `types` have seen in the predicted slot of each query's relation
        (rgcn_topk_typed_device)."""
        return self._scoring_runtime(graph).topk_typed(queries, predict_object, k, types, exclude_ptr, exclude_idx)

    def device_ranks_mixed(self, graph, triplets, predict_object, partner, weight, filter_ptr, filter_idx):
        """device_ranks under weight * this model's score + (1 - weight) * another model's (rgcn_rank_mixed_device):
        partner = that model's energies for the same triplets in the same order, a float32 [N, EntityCount] array or the
        device address of its engine's score buffer (Engine.rank_energies_device, same GPU); one chunk of at most
        Scorer.chunk_size triplets."""
        return self._scoring_runtime(graph).ranks_mixed(triplets, predict_object, partner, weight, filter_ptr, filter_idx)

    def device_topk(self, graph, queries, predict_object, k, exclude_ptr=None, exclude_idx=None):
        """The k most plausible objects of (s, r, ?) (predict_object) or subjects of (?, r, o) for every row of
        `queries`, best first, leaving out row i's exclude_idx[exclude_ptr[i]:exclude_ptr[i + 1]]; codes from a
        test-mode pass over `graph`.  Returns (entity ids int32 [N,k], energies float32 [N,k]); the column being
        predicted is not read; rows short of k answers end in (-1, -inf).  Scores are _sigmoid(energies)."""
        return self._scoring_runtime(graph).topk(queries, predict_object, k, exclude_ptr, exclude_idx)

    def device_score_queries(self, graph, queries, predict_object):
        """Energies of every entity for each row of `queries` (the column being predicted is not read), left in the
        engine's score buffer (rgcn_score_queries_device; Engine.rank_energies_device is its address): what the other
        model of an ensemble hands to device_topk_mixed.  One chunk of at most Scorer.chunk_size queries."""
        self._scoring_runtime(graph).score_queries(queries, predict_object)

    def device_topk_mixed(self, graph, queries, predict_object, k, partner, weight, exclude_ptr=None, exclude_idx=None):
        """device_topk under weight * this model's score + (1 - weight) * another model's (rgcn_topk_mixed_device):
        partner = that model's energies for the same queries in the same order, a float32 [N, EntityCount] array or the
        device address of its engine's score buffer (same GPU).  Returns (entity ids int32 [N,k], mixed scores float32
        [N,k]) ordered by (mixed score descending, entity id ascending); one chunk of at most Scorer.chunk_size queries."""
        return self._scoring_runtime(graph).topk_mixed(queries, predict_object, k, partner, weight, exclude_ptr, exclude_idx)

    def device_relation_ranks(self, graph, triplets, filter_ptr, filter_idx):
        """Ranks of the gold relations of `triplets` against every relation between their subject and object, codes
        from a test-mode pass over `graph` (rgcn_rank_relation_device): (raw int32 [N], filtered int32 [N]).  filter_ptr /
        filter_idx: CSR of the relations known for each pair, the gold one among them."""
        return self._scoring_runtime(graph).ranks_relation(triplets, filter_ptr, filter_idx)

    def device_relation_topk(self, graph, queries, k, exclude_ptr=None, exclude_idx=None):
        """The k most plausible relations of (s, ?, o) for every row of `queries`, best first, leaving out row i's
        exclude_idx[exclude_ptr[i]:exclude_ptr[i + 1]]; codes from a test-mode pass over `graph`
        (rgcn_topk_relation_device).  Returns (relation ids int32 [N,k], energies float32 [N,k]); the relation column is
        not read; rows short of k answers end in (-1, -inf).  Scores are _sigmoid(energies)."""
        return self._scoring_runtime(graph).topk_relation(queries, k, exclude_ptr, exclude_idx)

    def predict_top(self, predict_object, k, exclude_ptr=None, exclude_idx=None):
        """device_topk restated eagerly on predict_all_object_scores / predict_all_subject_scores of the triples fed
        to X (all three columns valid ids): (entity ids int32 [N,k], scores float32 [N,k]) ordered by (score
        descending, id ascending).  Scores saturate where energies do not, so this order is coarser than the
        device's; the small-size cross-check of the device path, like the other eager methods."""
        scores = self.predict_all_object_scores() if predict_object else self.predict_all_subject_scores()
        n, V = scores.shape
        idx = np.full((n, int(k)), -1, dtype=np.int32)
        top = np.zeros((n, int(k)), dtype=np.float32)
        for i in range(n):
            keep = np.ones(V, dtype=bool)
            if exclude_ptr is not None:
                keep[np.asarray(exclude_idx[exclude_ptr[i]:exclude_ptr[i + 1]], dtype=np.int64)] = False
            ids = np.flatnonzero(keep)
            order = ids[np.lexsort((ids, -scores[i, ids].astype(np.float64)))][:int(k)]
            idx[i, :len(order)] = order
            top[i, :len(order)] = scores[i, order]
        return idx, top

    def backward(self, upstream=None):
        """d(loss + regularisation)/d(codes, W_relation), then down the chain."""
        subject_codes, relation_codes, object_codes = self.next_component.get_all_codes(mode='train')
        x, z = self.X.value, self.Y.value
        e1s, rs, e2s = subject_codes[x[:, 0]], relation_codes[x[:, 1]], object_codes[x[:, 2]]
        n, d = e1s.shape
        energies = np.sum(e1s * rs * e2s, axis=1)
        dx = ((_sigmoid(energies) - z) / n).astype(np.float32)
        if self.adversarial_temperature > 0:
            # (the weights are constants)
            dx = reciprocal_row_weights(energies, z, self.adversarial_temperature, self.reciprocal) * dx
        dx = dx[:, None]
        k = np.float32(self.regularization_parameter * 2.0 / (n * d))
        g_e1, g_r, g_e2 = dx * (rs * e2s) + k * e1s, dx * (e1s * e2s) + k * rs, dx * (e1s * rs) + k * e2s
        dcodes = np.zeros_like(subject_codes)
        np.add.at(dcodes, x[:, 0], g_e1)
        np.add.at(dcodes, x[:, 2], g_e2)
        d_rel = np.zeros_like(relation_codes)
        np.add.at(d_rel, x[:, 1], g_r)
        if self.relation_softmax_weight > 0:
            _, t_codes, t_rel = relation_softmax_terms(subject_codes, relation_codes, self._forward_positives(x, z),
                                                       self.relation_count, self.relation_softmax_weight)
            dcodes = (dcodes + t_codes).astype(dcodes.dtype)
            d_rel = (d_rel + t_rel).astype(d_rel.dtype)
        if self.entity_softmax_weight > 0:
            _, t_codes, t_rel = entity_softmax_terms(subject_codes, relation_codes, self._entity_softmax_rows(x, z),
                                                     self.entity_softmax_weight)
            dcodes = (dcodes + t_codes).astype(dcodes.dtype)
            d_rel = (d_rel + t_rel).astype(d_rel.dtype)
        return self.next_component.backward((dcodes, d_rel))
