"""Ask a trained model: the k most plausible completions of (entity, relation, ?), (?, relation, entity) or
(subject, ?, object).

    python -m relationprediction_amd.predict --settings settings/gcn_block.exp --dataset data/FB-Toutanova \
        --model models/GcnBlock-3.npz --queries queries.txt --k 10 [--side object|subject|relation] [--keep-known] \
        [--type-constrained] [--out FILE] [--settings2 settings/distmult.exp --model2 models/Distmult-3.npz [--weight 0.5]]

The model is built exactly as train.py builds it (same settings merge, same chain), the checkpoint is one written by
Model.save, the training graph is encoded once in test mode and the selection runs on the device (rgcn_topk_device:
energies of every entity from one GEMM per chunk of queries, the k best per query picked and ordered there; nothing of
size [queries, entities] crosses to the host).  The reference has no such command: its checkpoints can only be ranked
against a test set (code/train.py:99-128).

--queries: one `entity<TAB>relation` per line, names as in entities.dict / relations.dict.  --side object (default)
reads the entity as the subject and answers objects; --side subject reads it as the object and answers subjects.
Completions already known from train / valid / test are left out unless --keep-known.  Output, one line per answer:

    query_entity<TAB>relation<TAB>answer_entity<TAB>position<TAB>score

position counts from 1 (best); score = sigmoid(energy), evaluated in double and rounded once to float32 as everywhere
else (csrc/ranking.hip).  Answers are ordered by (energy descending, entity id ascending).

--type-constrained (entity sides) answers only entities that the training triples have seen in the predicted slot of
the query's relation -- the objects of r for --side object, its subjects for --side subject (rgcn_topk_typed_device; a
relation with fewer than two such entities constrains nothing).  With --side relation or --settings2 it is a ValueError.

--side relation asks which relation holds between two entities (rgcn_topk_relation_device: the energies of every
relation for the pair, selected on the device alike).  --queries lines are then `subject<TAB>object`, --k is bounded by
the number of relations, the relations known for the pair from train / valid / test are left out unless --keep-known,
and the output lines are

    subject<TAB>answer_relation<TAB>object<TAB>position<TAB>score

ordered by (energy descending, relation id ascending).  There is no ensemble form: with --settings2 / --model2 it is a
ValueError.

--settings2 and --model2 (together) ask the R-GCN+ ensemble instead: a second model, built and loaded the same way on the
same GPU, is scored with the first as `weight * score_1 + (1 - weight) * score_2` (ensemble.py's mixture; --weight is
model 1's weight, in [0, 1], default 0.5).  Per chunk of Scorer.chunk_size queries model 2 leaves its energies in its
engine's score buffer (rgcn_score_queries_device) and model 1's engine mixes and selects reading that buffer in place
(rgcn_topk_mixed_device); the dataset is loaded once, under model 1's Evaluation.Metric.  The lines keep their format; the
last column is the mixed score, and the answers are ordered by (mixed score descending, entity id ascending)."""
import argparse
import sys

import numpy as np

from .common import settings_reader, evaluation

MAX_K = 1024          # RGCN_MAX_TOPK (include/rgcn.h)


def read_queries(path, entity_ids, relation_ids):
    """[(entity id, relation id)] of a query file; an unknown name or a malformed line is a ValueError naming the line"""
    pairs = []
    with open(path, "r") as f:
        for number, line in enumerate(f, start=1):
            if not line.strip():
                continue
            fields = line.rstrip("\r\n").split("\t")
            if len(fields) != 2:
                raise ValueError("%s line %d: expected entity<TAB>relation, got %d field(s)" % (path, number, len(fields)))
            entity, relation = fields
            if entity not in entity_ids:
                raise ValueError("%s line %d: unknown entity %r" % (path, number, entity))
            if relation not in relation_ids:
                raise ValueError("%s line %d: unknown relation %r" % (path, number, relation))
            pairs.append((entity_ids[entity], relation_ids[relation]))
    return pairs


def read_pair_queries(path, entity_ids):
    """[(subject id, object id)] of a --side relation query file; errors as read_queries'"""
    pairs = []
    with open(path, "r") as f:
        for number, line in enumerate(f, start=1):
            if not line.strip():
                continue
            fields = line.rstrip("\r\n").split("\t")
            if len(fields) != 2:
                raise ValueError("%s line %d: expected subject<TAB>object, got %d field(s)" % (path, number, len(fields)))
            for entity in fields:
                if entity not in entity_ids:
                    raise ValueError("%s line %d: unknown entity %r" % (path, number, entity))
            pairs.append((entity_ids[fields[0]], entity_ids[fields[1]]))
    return pairs


def build_model(settings, splits, n_entities, n_relations):
    """The training driver's own chain (train.build_model, train.initialize_model), ready for test-mode calls."""
    from . import train
    _, model = train.build_model(settings, splits['train'], n_entities, n_relations)
    train.initialize_model(model, splits['train'])
    return model


def sigmoid_f32(energies):
    with np.errstate(over='ignore'):
        return (1.0 / (1.0 + np.exp(-np.asarray(energies, dtype=np.float64)))).astype(np.float32)


def main(argv=None, out=None):
    parser = argparse.ArgumentParser(description="Top-k link prediction with a trained model.")
    parser.add_argument("--settings", help="Filepath for settings file.", required=True)
    parser.add_argument("--dataset", help="Filepath for dataset.", required=True)
    parser.add_argument("--model", help="checkpoint written by Model.save (.npz)", required=True)
    parser.add_argument("--queries", help="file of entity<TAB>relation lines (names); --side relation: subject<TAB>object",
                        required=True)
    parser.add_argument("--k", type=int, default=10, help="answers per query (at most %d)" % MAX_K)
    parser.add_argument("--side", choices=("object", "subject", "relation"), default="object",
                        help="what is predicted: the object of (entity, relation, ?), the subject of (?, relation, entity) "
                             "or the relation of (subject, ?, object)")
    parser.add_argument("--keep-known", action="store_true",
                        help="do not leave out the completions known from train / valid / test")
    parser.add_argument("--type-constrained", action="store_true",
                        help="answer only entities the training triples have seen in the predicted slot of the relation "
                             "(entity sides, one model)")
    parser.add_argument("--out", default=None, help="write the answers here instead of standard output")
    parser.add_argument("--settings2", default=None, help="settings file of model 2: answer under the ensemble of the two")
    parser.add_argument("--model2", default=None, help="checkpoint of model 2")
    parser.add_argument("--weight", type=float, default=None,
                        help="weight of model 1's score; model 2 gets 1 - weight (default 0.5; needs --settings2 / --model2)")
    args = parser.parse_args(argv)
    if (args.settings2 is None) != (args.model2 is None):
        raise ValueError("--settings2 and --model2 come together")
    ensemble = args.settings2 is not None
    if ensemble and args.side == "relation":
        raise ValueError("--side relation has no ensemble form: drop --settings2 / --model2")
    if args.type_constrained and (ensemble or args.side == "relation"):
        raise ValueError("--type-constrained is for the entity sides of one model: drop --side relation / --settings2")
    if args.weight is not None and not ensemble:
        raise ValueError("--weight needs --settings2 and --model2")
    weight = 0.5 if args.weight is None else args.weight
    if not 0.0 <= weight <= 1.0:                 # (NaN fails both comparisons)
        raise ValueError("--weight %r: must lie in [0, 1]" % (weight,))

    settings = settings_reader.read(args.settings)
    from .train import load_dataset
    splits, entities, relations = load_dataset(args.dataset, settings['Evaluation']['Metric'])
    if args.side == "relation":
        return predict_relations(args, settings, splits, entities, relations, out)
    if not 1 <= args.k <= min(len(entities), MAX_K):
        raise ValueError("--k %d: must be between 1 and min(number of entities = %d, %d)"
                         % (args.k, len(entities), MAX_K))
    entity_ids = {name: i for i, name in entities.items()}
    relation_ids = {name: i for i, name in relations.items()}
    pairs = read_queries(args.queries, entity_ids, relation_ids)
    predict_object = args.side == "object"

    ptr = idx = None
    if not args.keep_known:
        known = {}
        for part in ('train', 'valid', 'test'):
            evaluation.Scorer.extend_triple_dict(known, splits[part], object_list=predict_object)
        ptr, idx = evaluation.known_completions_csr(pairs, known)

    model = build_model(settings, splits, len(entities), len(relations))
    model.load(args.model)
    queries = np.full((len(pairs), 3), -1, dtype=np.int32)         # the predicted column is not read
    if pairs:
        queries[:, 0 if predict_object else 2] = [p[0] for p in pairs]
        queries[:, 1] = [p[1] for p in pairs]
    if ensemble:
        second = build_model(settings_reader.read(args.settings2), splits, len(entities), len(relations))
        second.load(args.model2)
        devices = [m.get_runtime().engine.cfg.device for m in (model, second)]
        if devices[0] != devices[1]:
            raise ValueError("the two models must run on one GPU (Device %d and %d): model 1 reads model 2's scores in place"
                             % tuple(devices))
        top, scores = np.full((len(pairs), args.k), -1, np.int32), np.full((len(pairs), args.k), -np.inf, np.float32)
        chunk_size = evaluation.Scorer.chunk_size
        for lo in range(0, len(pairs), chunk_size):
            hi = min(lo + chunk_size, len(pairs))
            chunk_ptr = chunk_idx = None
            if ptr is not None:
                chunk_ptr, chunk_idx = ptr[lo:hi + 1] - ptr[lo], idx[ptr[lo]:ptr[hi]]
            # model 2 first: the call synchronises, and its energies of THIS chunk stay in its engine's buffer until its
            # next scoring call
            second.device_score_queries(second.test_graph, queries[lo:hi], predict_object)
            partner = second.get_runtime().engine.rank_energies_device()
            top[lo:hi], scores[lo:hi] = model.device_topk_mixed(model.test_graph, queries[lo:hi], predict_object, args.k,
                                                                partner, weight, chunk_ptr, chunk_idx)
    elif args.type_constrained:
        types = np.ascontiguousarray(splits['train'], dtype=np.int32)
        top, energies = model.device_topk_typed(model.test_graph, queries, predict_object, args.k, types, ptr, idx)
        scores = sigmoid_f32(energies)
    else:
        top, energies = model.device_topk(model.test_graph, queries, predict_object, args.k, ptr, idx)
        scores = sigmoid_f32(energies)

    sink = open(args.out, "w") if args.out else (out or sys.stdout)
    try:
        for (entity, relation), ids, row in zip(pairs, top, scores):
            for position, (answer, score) in enumerate(zip(ids, row), start=1):
                if answer < 0:
                    break                                            # fewer than k entities were left to answer
                sink.write("%s\t%s\t%s\t%d\t%.9g\n" % (entities[entity], relations[relation], entities[int(answer)],
                                                       position, score))
    finally:
        if args.out:
            sink.close()
    return top, scores


def predict_relations(args, settings, splits, entities, relations, out):
    """main() for --side relation: (relation ids int32 [N,k], scores float32 [N,k])"""
    if not 1 <= args.k <= min(len(relations), MAX_K):
        raise ValueError("--k %d: must be between 1 and min(number of relations = %d, %d)"
                         % (args.k, len(relations), MAX_K))
    pairs = read_pair_queries(args.queries, {name: i for i, name in entities.items()})
    ptr = idx = None
    if not args.keep_known:
        scorer = evaluation.Scorer(settings['Evaluation'])
        for part in ('train', 'valid', 'test'):
            scorer.register_data(splits[part])
        ptr, idx = evaluation.known_completions_csr(pairs, scorer.known_relation_triples)

    model = build_model(settings, splits, len(entities), len(relations))
    model.load(args.model)
    queries = np.full((len(pairs), 3), -1, dtype=np.int32)         # the relation column is not read
    if pairs:
        queries[:, 0] = [p[0] for p in pairs]
        queries[:, 2] = [p[1] for p in pairs]
    top, energies = model.device_relation_topk(model.test_graph, queries, args.k, ptr, idx)
    scores = sigmoid_f32(energies)

    sink = open(args.out, "w") if args.out else (out or sys.stdout)
    try:
        for (subject, obj), ids, row in zip(pairs, top, scores):
            for position, (answer, score) in enumerate(zip(ids, row), start=1):
                if answer < 0:
                    break                                            # fewer than k relations were left to answer
                sink.write("%s\t%s\t%s\t%d\t%.9g\n" % (entities[subject], relations[int(answer)], entities[obj],
                                                       position, score))
    finally:
        if args.out:
            sink.close()
    return top, scores


if __name__ == '__main__':
    main()
