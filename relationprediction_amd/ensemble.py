"""R-GCN+: link-prediction ranks of the weighted sum of two trained models' scores.

    python -m relationprediction_amd.ensemble --settings A.exp --model A.npz --settings2 B.exp --model2 B.npz \
        --dataset D [--weight 0.5] [--split test]

The paper's best FB15k-237 model is a trained R-GCN and a trained DistMult scored together,
`weight * score_1 + (1 - weight) * score_2`; the reference gets it from code/tools/ensemble.py (WeightEnsemble: rank =
1 + the remaining candidates whose combined score is at least the gold's), which reads score files holding EntityCount
floats per query as text.  Here both models are built exactly as train.py builds them (train.build_model), their
checkpoints are ones written by Model.save, each is encoded once in test mode, and no score leaves the device: per chunk
of queries and per side model 2 is ranked (its energies stay in its engine's score buffer), model 1 is ranked alone, and
model 1's engine then ranks the mixture reading model 2's buffer in place (rgcn_rank_mixed_device).  Both engines live
in this process, on the same GPU.  --weight is model 1's weight.

Prints raw and filtered MRR and hits@1/3/10 for model 1, model 2 and the ensemble, each as Scorer's summary prints it,
under a heading line.  Filter lists are the ones common/evaluation.py builds (train + valid + test completions).
CutoffEnsemble, the reference's other method, is not built."""
import argparse

import numpy as np

from .common import settings_reader, evaluation


def main(argv=None):
    parser = argparse.ArgumentParser(description="Rank a split under the weighted sum of two trained models' scores.")
    parser.add_argument("--settings", help="settings file of model 1", required=True)
    parser.add_argument("--model", help="checkpoint of model 1 (written by Model.save, .npz)", required=True)
    parser.add_argument("--settings2", help="settings file of model 2", required=True)
    parser.add_argument("--model2", help="checkpoint of model 2", required=True)
    parser.add_argument("--dataset", help="Filepath for dataset.", required=True)
    parser.add_argument("--weight", type=float, default=0.5, help="weight of model 1's score; model 2 gets 1 - weight")
    parser.add_argument("--split", choices=("train", "valid", "test"), default="test", help="the triples to rank")
    args = parser.parse_args(argv)
    if not 0.0 <= args.weight <= 1.0:            # (NaN fails both comparisons)
        raise ValueError("--weight %r: must lie in [0, 1]" % (args.weight,))

    from . import predict
    from .train import load_dataset
    both = [settings_reader.read(args.settings), settings_reader.read(args.settings2)]
    for s in both:
        if s['Evaluation']['Metric'] != 'MRR':
            raise NotImplementedError("the ensemble ranks: Evaluation.Metric must be MRR in both settings files")
    splits, entities, relations = load_dataset(args.dataset, 'MRR')
    models = []
    for s, checkpoint in zip(both, (args.model, args.model2)):
        model = predict.build_model(s, splits, len(entities), len(relations))
        model.load(checkpoint)
        models.append(model)
    first, second = models
    devices = [m.get_runtime().engine.cfg.device for m in models]
    if devices[0] != devices[1]:
        raise ValueError("the two models must run on one GPU (Device %d and %d): model 1 reads model 2's scores in place"
                         % tuple(devices))

    scorer = evaluation.Scorer(both[0]['Evaluation'])
    for part in ('train', 'valid', 'test'):
        scorer.register_data(splits[part])
    triples = np.asarray(splits[args.split])
    ranks = {name: ([], []) for name in ("first", "second", "ensemble")}
    chunk_size = evaluation.Scorer.chunk_size
    for lo in range(0, len(triples), chunk_size):
        chunk = triples[lo:lo + chunk_size]
        for subject_side in (True, False):                   # Scorer.evaluate_mrr's row order
            ptr, idx = scorer._filter_csr(chunk, subject_side)
            # model 2 first: the call synchronises, and its energies of THIS chunk and side stay in its engine's buffer
            # until its next ranking call
            results = {"second": second.device_ranks(second.test_graph, chunk, not subject_side, ptr, idx),
                       "first": first.device_ranks(first.test_graph, chunk, not subject_side, ptr, idx)}
            partner = second.get_runtime().engine.rank_energies_device()
            results["ensemble"] = first.device_ranks_mixed(first.test_graph, chunk, not subject_side, partner,
                                                           args.weight, ptr, idx)
            for name, (raw, filtered) in results.items():
                ranks[name][0].extend(raw)
                ranks[name][1].extend(filtered)

    summaries = {}
    for name, title in (("first", "Model 1 (%s)" % args.model), ("second", "Model 2 (%s)" % args.model2),
                        ("ensemble", "Ensemble (%g x model 1 + %g x model 2)" % (args.weight, 1.0 - args.weight))):
        print(title)
        summaries[name] = evaluation.MrrSummary(ranks[name][0], ranks[name][1])
        summaries[name].pretty_print()
    return summaries


if __name__ == '__main__':
    main()
