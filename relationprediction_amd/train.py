"""Training driver with the reference's command line (code/train.py):

    python -m relationprediction_amd.train --settings settings/gcn_block.exp --dataset data/FB-Toutanova

Same stages in the same order: read the dataset (:21-47), merge the settings sections (:66-86), build the
encoder / decoder chain (:92-93), the scorer with validation MRR as early-stopping score (:99-128), the
minibatch transform (neighbourhood graph batch -> edge dropout split -> negative sampling, :133-247), and the
Converge loop (:255-284).  What runs where: the chain's components configure ONE HIP engine context; every
iteration is one asynchronous device step (graph prep, R-GCN forward, DistMult loss, backward, clip, Adam);
the host draws the next minibatch meanwhile (neighbourhood sampler in librgcn.so, O(log V) per pick); validation
encodes the training graph once and ranks on the device.  `Name=embedding` (settings/distmult.exp, the DistMult baseline)
has no graph: every iteration's positives are the whole training set, resident on the device, and the step is the
decoder's loss and gradients, clip and Adam.

Continuing a run (not in the reference, whose checkpoints hold the weights alone): `--save-optimizer-state` writes
`<ExperimentName>-<n>.opt.npz` -- the algorithm's name, its step count and its moments or accumulators -- beside every
checkpoint `<ExperimentName>-<n>.npz`; `--resume <ExperimentName>-<n>.npz` loads the weights and, if it is there, that
sibling (otherwise it says that the optimizer starts fresh), and numbers its own checkpoints from n + 1.  Only the model
and the optimizer continue: whatever counts ITERATIONS -- MaxIterations, the early stopper's burn-in and last score,
the loss reports -- starts over at 1, and the random streams are the new process's."""
import argparse
import os
import re

import numpy as np

from . import _native
from .common import settings_reader, io, model_builder, optimizer_parameter_parser, evaluation, auxilliaries
from .optimization.optimize import build_hip


def load_dataset(dataset, metric='MRR'):
    """code/train.py:21-47.  Metric 'Accuracy' reads valid_accuracy.txt / test_accuracy.txt instead of valid.txt /
    test.txt (:32-35); 'RelationMRR' (this project's: the rank of the gold relation for a pair, Scorer.
    compute_relation_mrr_scores) reads valid.txt / test.txt as 'MRR' does.  A metric that does not exist is refused HERE,
    at start-up, not at the first early-stopping check thousands of iterations in."""
    if metric not in ('MRR', 'Accuracy', 'RelationMRR'):
        raise NotImplementedError("Evaluation.Metric = %r: the reference has 'MRR' and 'Accuracy', this project adds "
                                  "'RelationMRR'" % (metric,))
    relations_path = dataset + '/relations.dict'
    entities_path = dataset + '/entities.dict'
    splits = {}
    for name in ('train', 'valid', 'test'):
        path = dataset + '/' + name + ('_accuracy' if metric == 'Accuracy' and name != 'train' else '') + '.txt'
        splits[name] = np.array(io.read_triplets_as_list(path, entities_path, relations_path), dtype=np.int32)
    return splits, io.read_dictionary(entities_path), io.read_dictionary(relations_path)


def exclusive_negative_sampling(general_settings):
    """[General] ExclusiveNegativeSampling=Yes|No (absent from the reference's settings files; default No): redraw every
    corruption that is a training triple, NegativeSampler.transform_exclusive instead of .transform"""
    value = general_settings['ExclusiveNegativeSampling'] if 'ExclusiveNegativeSampling' in general_settings else 'No'
    if value not in ('Yes', 'No'):
        raise ValueError("General.ExclusiveNegativeSampling must be Yes or No, not %r" % (value,))
    return value == 'Yes'


def type_constrained_negatives(general_settings):
    """[General] TypeConstrainedNegatives=Yes|No (absent from the reference's settings files; default No): every entity
    corruption is drawn from the entities the training triples have seen in that slot of the row's relation
    (NegativeSampler.transform_typed; on the device rgcn_negative_sample_typed_device)"""
    value = general_settings['TypeConstrainedNegatives'] if 'TypeConstrainedNegatives' in general_settings else 'No'
    if value not in ('Yes', 'No'):
        raise ValueError("General.TypeConstrainedNegatives must be Yes or No, not %r" % (value,))
    return value == 'Yes'


def relation_negative_sample_rate(general_settings):
    """[General] RelationNegativeSampleRate=m (absent from the reference's settings files; default 0): m further negative
    rows (s, r', o) per positive, with a relation other than r -- what trains W_relation to tell relations apart for a
    fixed pair.  A non-negative integer; m > 0 needs two relations."""
    value = general_settings['RelationNegativeSampleRate'] if 'RelationNegativeSampleRate' in general_settings else 0
    text = str(value).strip()
    if isinstance(value, bool) or isinstance(value, float) or not text.isdigit():
        raise ValueError("General.RelationNegativeSampleRate must be a non-negative integer, not %r" % (value,))
    rate = int(text)
    if rate > 0 and 'RelationCount' in general_settings and int(general_settings['RelationCount']) < 2:
        raise ValueError("General.RelationNegativeSampleRate = %d needs at least two relations, the dataset has %d"
                         % (rate, int(general_settings['RelationCount'])))
    return rate


def reciprocal_relations(decoder_settings):
    """[Decoder] ReciprocalRelations=Yes|No (absent from the reference's settings files; default No): a second vector per
    relation, W_relation[RelationCount + r], answers (?, r, o); every step trains on the samplers' rows through the
    reciprocal pass and on the inverse positives behind them (decoders.bilinear_diag.parse_reciprocal_relations)."""
    from .decoders.bilinear_diag import parse_reciprocal_relations
    return parse_reciprocal_relations(decoder_settings)


def adversarial_temperature(general_settings):
    """[General] AdversarialTemperature=alpha (absent from the reference's settings files; default 0): the temperature of
    the self-adversarial weights of every step's negatives.  A non-negative finite float
    (decoders.bilinear_diag.parse_adversarial_temperature), checked when the model is built."""
    from .decoders.bilinear_diag import parse_adversarial_temperature
    return parse_adversarial_temperature(general_settings)


def relation_softmax_weight(decoder_settings, relation_count):
    """[Decoder] RelationSoftmaxWeight=lambda (absent from the reference's settings files; default 0): the weight of the
    softmax-over-relations loss term of every step's positives.  A non-negative finite float
    (decoders.bilinear_diag.parse_relation_softmax_weight); lambda > 0 needs two relations."""
    from .decoders.bilinear_diag import parse_relation_softmax_weight
    weight = parse_relation_softmax_weight(decoder_settings)
    if weight > 0 and int(relation_count) < 2:
        raise ValueError("Decoder.RelationSoftmaxWeight = %g needs at least two relations, the dataset has %d"
                         % (weight, int(relation_count)))
    return weight


def entity_softmax_settings(decoder_settings, entity_count):
    """[Decoder] EntitySoftmaxWeight=lambda and EntitySoftmaxPositives=k (absent from the reference's settings files;
    defaults 0 and 0 = all): the weight of the softmax-over-entities loss term of every step's positives and how many
    leading positives of a step it takes (decoders.bilinear_diag.parse_entity_softmax_*); lambda > 0 needs two entities.
    Returns (lambda, k)."""
    from .decoders.bilinear_diag import parse_entity_softmax_positives, parse_entity_softmax_weight
    weight = parse_entity_softmax_weight(decoder_settings)
    positives = parse_entity_softmax_positives(decoder_settings)
    if weight > 0 and int(entity_count) < 2:
        raise ValueError("Decoder.EntitySoftmaxWeight = %g needs at least two entities, the dataset has %d"
                         % (weight, int(entity_count)))
    return weight, positives


def make_transform(train_triplets, general_settings, encoder, device_negatives=False, device_dropout=False,
                   device_sampler=False, reciprocal=False):
    """The reference's t_func (train.py:201-247): minibatch -> (graph_split, X, Y).

    ExclusiveNegativeSampling=Yes: the corruptions avoid the training triples -- on the host path through
    ns.transform_exclusive, on the device paths through `known=` of the batch objects (the runtime reserves the training
    triples on the device once).

    RelationNegativeSampleRate=m: m relation corruptions per positive follow the entity corruptions, on the host path
    through the sampler's relation_rate, on the device paths through `relation_rate=` of the batch objects.

    TypeConstrainedNegatives=Yes: the entity corruptions come from the per-relation entity sets of the training triples --
    on the host path through ns.transform_typed, on the device paths through `types=` of the batch objects (the runtime
    reserves the sets on the device once).

    reciprocal (ReciprocalRelations=Yes, a key of [Decoder]): on the host path the sampler's transform_reciprocal runs
    behind whichever transform drew the rows; on the device paths the decoder tells the runtime, whose steps run the
    device's pass, so the batch objects carry nothing.

    Every batch is a function of ONE seed drawn from numpy's global generator when the batch is requested, so
    batches can be built ahead of time by background threads (`t_func.seeded(data, seed)`, used by
    optimization.optimize.HipOptimizer) and still come out in a reproducible order; `t_func(data)` itself
    draws the seed and builds the batch in place, like the reference's function."""
    import threading
    relation_rate = relation_negative_sample_rate(general_settings)
    ns = auxilliaries.NegativeSampler(int(general_settings['NegativeSampleRate']), general_settings['EntityCount'],
                                      relation_rate=relation_rate,
                                      relation_count=int(general_settings['RelationCount'])
                                      if relation_rate or reciprocal else None, reciprocal=reciprocal)
    ns.set_known_positives(train_triplets)
    exclusive = exclusive_negative_sampling(general_settings)
    host_negatives = ns.transform_exclusive if exclusive else ns.transform
    typed = type_constrained_negatives(general_settings)
    if typed:
        ns.set_type_sets(train_triplets)

        def host_negatives(x, rng):
            return ns.transform_typed(x, rng, exclusive=exclusive)
    # (a graph-less encoder never reaches the sampler: settings/distmult.exp carries a GraphBatchSize it does not use)
    use_sampler = 'GraphBatchSize' in general_settings and encoder.needs_graph()
    if use_sampler and int(general_settings['GraphBatchSize']) > len(train_triplets):
        # the reference's sampler runs out of edges and dies on NaN probabilities (train.py:173-178)
        raise ValueError("General.GraphBatchSize = %d exceeds the %d training edges (EdgeCount): remove the key to "
                         "train on the whole graph, or lower it" % (int(general_settings['GraphBatchSize']),
                                                                    len(train_triplets)))
    local = threading.local()            # the native sampler keeps per-sample state: one per thread
    train_arr = np.ascontiguousarray(train_triplets, dtype=np.int32)     # (what the device sampler keeps resident)
    known = train_arr if exclusive else None      # K is the training set alone, as the reference registers it
    extra = {'types': train_arr} if typed else {}   # (the type sets are the training set's too)

    def seeded(x, seed):
        rng = np.random.RandomState(seed)
        arr = np.asarray(x)
        if not encoder.needs_graph():
            # Name=embedding (train.py:227-229): no graph batch, no edge dropout -- every iteration's positives are the
            # whole training set.  Device negatives: the array itself is handed on, so that the step finds it resident
            if device_negatives:
                from .optimization.optimize import DeviceNegatives
                return DeviceNegatives(None, arr, ns.negative_sample_rate, known=known, relation_rate=relation_rate,
                                       **extra)
            return host_negatives(arr, rng)
        if use_sampler and device_sampler and device_dropout:
            # all three draws on the device: the iteration is three seeds, nothing is built on the host or uploaded
            from .optimization.optimize import DeviceMinibatch
            size = int(general_settings['GraphBatchSize'])
            split_size = int(float(general_settings['GraphSplitSize']) * size)
            sample = (train_arr, size, rng.randint(0, 2 ** 31 - 1))
            return DeviceMinibatch(None, split_size, rng.randint(0, 2 ** 31 - 1), ns.negative_sample_rate, sample=sample,
                                   known=known, relation_rate=relation_rate, **extra)
        if use_sampler:
            if not hasattr(local, 'sampler'):
                local.sampler = _native.NeighborhoodSampler(train_triplets, int(general_settings['EntityCount']))
            graph_batch_ids = local.sampler.sample(int(general_settings['GraphBatchSize']), rng.randint(0, 2 ** 31 - 1))
        else:
            graph_batch_ids = np.arange(arr.shape[0])
        graph_batch = train_triplets[graph_batch_ids]
        # edge dropout: the encoder sees a random GraphSplitSize fraction of the batch (exact-k, :235-238)
        split_size = int(float(general_settings['GraphSplitSize']) * graph_batch.shape[0])
        if device_dropout:            # both draws (kept edges, corruptions) are made by the device step
            from .optimization.optimize import DeviceMinibatch
            return DeviceMinibatch(graph_batch, split_size, rng.randint(0, 2 ** 31 - 1), ns.negative_sample_rate,
                                   known=known, relation_rate=relation_rate, **extra)
        graph_split_ids = rng.choice(graph_batch_ids, size=split_size, replace=False)
        graph_split = train_triplets[graph_split_ids]
        if device_negatives:          # corruptions are drawn by the device step (optimize.DeviceNegatives)
            from .optimization.optimize import DeviceNegatives
            return DeviceNegatives(graph_split, graph_batch, ns.negative_sample_rate, known=known,
                                   relation_rate=relation_rate, **extra)
        t = host_negatives(graph_batch, rng)
        return (graph_split, t[0], t[1])

    def t_func(x):
        return seeded(x, np.random.randint(0, 2 ** 31 - 1))

    t_func.seeded = seeded
    t_func.sampler = ns
    return t_func


def report_unresolved_negatives(model):
    """with each validation report: how many negative rows the exclusive device sampler had to leave as drawn because
    every entity was a known positive for them -- printed only when there are any"""
    count = model.device_negative_unresolved()
    if count:
        print("Exclusive negative sampling: %d rows so far had no entity that is not a known positive" % count)
    return count


def report_unresolved_relation_negatives(model):
    """as report_unresolved_negatives, for the relation corruptions: rows every other relation was a known positive for"""
    count = model.device_negative_relation_unresolved()
    if count:
        print("Exclusive relation negative sampling: %d rows so far had no relation that is not a known positive" % count)
    return count


def report_typed_open_negatives(model, sampler=None):
    """with each validation report under TypeConstrainedNegatives: how many negative rows were drawn over all entities so
    far because their list is open, holds no entity but the row's own, or (exclusive) held known positives only -- the
    device sampler's count, with --host-negatives the host sampler's"""
    count = model.device_negative_typed_open() or 0
    if sampler is not None:
        count += sampler.typed_open
    print("Type-constrained negative sampling: %d rows so far were drawn over all entities (open lists)" % count)
    return count


def make_validation_function(scorer, metric, test_triplets, model, typed_sampler=False):
    """code/train.py:114-128: the early-stopping score is the validation split's filtered MRR (Metric=MRR), its filtered
    relation MRR (RelationMRR) or its accuracy; the test split's table is printed with every report."""
    def score_validation_data(validation_data):
        score_summary = scorer.compute_scores(validation_data, verbose=False).get_summary()
        lookup_string = (score_summary.mrr_string() if metric in ('MRR', 'RelationMRR')
                         else score_summary.accuracy_string())               # code/train.py:116-121
        early_stopping = score_summary.results['Filtered'][lookup_string]
        score_summary = scorer.compute_scores(test_triplets, verbose=False).get_summary()
        score_summary.pretty_print()
        report_unresolved_negatives(model)
        report_unresolved_relation_negatives(model)
        if typed_sampler is not False:
            report_typed_open_negatives(model, typed_sampler)
        return early_stopping
    return score_validation_data


def build_model(settings, train_triplets, entity_count, relation_count):
    """code/train.py:76-93: the dataset's counts into General, the section merges, the encoder / decoder chain.
    Returns (encoder, model).  The training driver and relationprediction_amd.predict both build their model here."""
    encoder_settings, decoder_settings = settings['Encoder'], settings['Decoder']
    shared_settings, general_settings = settings['Shared'], settings['General']
    general_settings.put('EntityCount', entity_count)
    general_settings.put('RelationCount', relation_count)
    general_settings.put('EdgeCount', len(train_triplets))
    encoder_settings.merge(shared_settings)
    encoder_settings.merge(general_settings)
    decoder_settings.merge(shared_settings)
    decoder_settings.merge(general_settings)
    settings['Optimizer'].merge(general_settings)
    settings['Evaluation'].merge(general_settings)
    weight = relation_softmax_weight(decoder_settings, relation_count)
    adversarial_temperature(general_settings)
    entity_weight, _ = entity_softmax_settings(decoder_settings, entity_count)
    encoder = model_builder.build_encoder(encoder_settings, train_triplets)
    model = model_builder.build_decoder(encoder, decoder_settings)
    if (weight > 0 or entity_weight > 0) and exclusive_negative_sampling(general_settings) \
            and hasattr(model, 'set_relation_softmax_known'):
        # the terms' masks follow ExclusiveNegativeSampling: relations (entities) that are training facts for a pair (for a
        # row's query) do not compete
        model.set_relation_softmax_known(np.ascontiguousarray(train_triplets, dtype=np.int32))
    return encoder, model


def initialize_model(model, train_triplets):
    """code/train.py:249-251: the training graph is what test-mode calls encode; the weights are drawn"""
    model.preprocess(train_triplets)
    model.register_for_test(train_triplets)
    model.initialize_train()


def optimizer_state_path(checkpoint):
    """<ExperimentName>-<n>.npz -> <ExperimentName>-<n>.opt.npz, the optimizer's state beside a weight checkpoint"""
    return (checkpoint[:-4] if checkpoint.endswith('.npz') else checkpoint) + '.opt.npz'


def save_with_optimizer_state(model):
    """Model.save, and the optimizer's state beside every checkpoint it writes (--save-optimizer-state)"""
    def save(path):
        n = model.save_iter
        model.save(path)
        model.save_optimizer(optimizer_state_path("%s-%d.npz" % (path, n)))
    return save


def resume_weights(model, checkpoint):
    """--resume, first half (after initialize_model): the checkpoint's weights, and the checkpoint numbering continues
    behind the <n> of <ExperimentName>-<n>.npz so that the run overwrites nothing it started from."""
    model.load(checkpoint)
    m = re.search(r'-(\d+)\.npz$', checkpoint)
    if m is None:
        print("resume: %s is not named <ExperimentName>-<n>.npz, checkpoints are numbered from %d"
              % (checkpoint, model.save_iter))
    else:
        model.save_iter = int(m.group(1)) + 1


def resume_optimizer(model, checkpoint):
    """--resume, second half (after the optimizer is configured): the state beside the checkpoint, if there is one"""
    path = optimizer_state_path(checkpoint)
    if not os.path.exists(path):
        print("resume: no %s, the optimizer starts fresh" % path)
        return None
    step = model.load_optimizer(path)
    print("resume: optimizer state of %s, %d steps taken" % (path, step))
    return step


def main(argv=None):
    parser = argparse.ArgumentParser(description="Train a model on a given dataset.")
    parser.add_argument("--settings", help="Filepath for settings file.", required=True)
    parser.add_argument("--dataset", help="Filepath for dataset.", required=True)
    parser.add_argument("--max-iterations", type=int, default=None,
                        help="stop after this many iterations (sets Optimizer.MaxIterations)")
    parser.add_argument("--host-negatives", action="store_true",
                        help="draw the negative samples with the reference's numpy code on the host instead of on the device")
    parser.add_argument("--host-edge-dropout", action="store_true",
                        help="choose the GraphSplitSize subset of each graph batch with numpy on the host (the "
                             "reference's np.random.choice) instead of on the device")
    parser.add_argument("--host-sampler", action="store_true",
                        help="draw the neighbourhood graph batch with the host sampler (librgcn.so's O(log V) port of "
                             "sample_edge_neighborhood, built ahead by --batch-workers threads) instead of on the device")
    parser.add_argument("--batch-workers", type=int, default=8,
                        help="background threads that build minibatches ahead of the device (0: build in line)")
    parser.add_argument("--save-optimizer-state", action="store_true",
                        help="write <ExperimentName>-<n>.opt.npz (the optimizer's moments / accumulators and step count) "
                             "beside every checkpoint <ExperimentName>-<n>.npz")
    parser.add_argument("--resume", metavar="CHECKPOINT.npz", default=None,
                        help="start from this checkpoint's weights and, if CHECKPOINT.opt.npz lies beside it, its "
                             "optimizer state; new checkpoints are numbered behind it.  What counts iterations "
                             "(MaxIterations, the burn-in, the reports) starts over")
    args = parser.parse_args(argv)

    settings = settings_reader.read(args.settings)
    print(settings)

    encoder_settings = settings['Encoder']
    decoder_settings = settings['Decoder']
    shared_settings = settings['Shared']
    general_settings = settings['General']
    optimizer_settings = settings['Optimizer']
    evaluation_settings = settings['Evaluation']

    splits, entities, relations = load_dataset(args.dataset, evaluation_settings['Metric'])
    train_triplets, valid_triplets, test_triplets = splits['train'], splits['valid'], splits['test']

    encoder, model = build_model(settings, train_triplets, len(entities), len(relations))
    if args.max_iterations is not None:
        optimizer_settings.put('MaxIterations', args.max_iterations)

    opp = optimizer_parameter_parser.Parser(optimizer_settings)
    opp.set_save_function(save_with_optimizer_state(model) if args.save_optimizer_state else model.save)

    scorer = evaluation.Scorer(evaluation_settings)
    scorer.register_data(train_triplets)
    scorer.register_data(valid_triplets)
    scorer.register_data(test_triplets)
    scorer.register_degrees(train_triplets)
    scorer.register_model(model)
    scorer.finalize_frequency_computation(np.concatenate((train_triplets, valid_triplets, test_triplets), axis=0))

    if scorer.type_constrained:
        scorer.register_type_sets(train_triplets)

    t_func = None
    if 'NegativeSampleRate' in general_settings:
        t_func = make_transform(train_triplets, general_settings, encoder, device_negatives=not args.host_negatives,
                                device_dropout=not (args.host_negatives or args.host_edge_dropout),
                                device_sampler=not args.host_sampler,
                                reciprocal=reciprocal_relations(decoder_settings))
    typed_sampler = False          # False: no report; None: the device's count; a sampler: the host's beside it
    if t_func is not None and type_constrained_negatives(general_settings):
        typed_sampler = t_func.sampler if args.host_negatives else None
    score_validation_data = make_validation_function(scorer, evaluation_settings['Metric'], test_triplets, model,
                                                     typed_sampler=typed_sampler)

    opp.set_early_stopping_score_function(score_validation_data)
    print(len(train_triplets))

    if t_func is not None:
        opp.set_sample_transform_function(t_func)

    initialize_model(model, train_triplets)
    if args.resume is not None:
        resume_weights(model, args.resume)
    print(model.get_train_input_variables())

    optimizer = build_hip(model, opp.get_parametrization(), batch_workers=args.batch_workers)
    if args.resume is not None:
        resume_optimizer(model, args.resume)
    iterations = optimizer.fit(train_triplets, validation_data=valid_triplets)
    return model, iterations


if __name__ == '__main__':
    main()
