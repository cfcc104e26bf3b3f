"""Float64 restatement of the relation queries (include/rgcn.h rgcn_rank_relation_device, rgcn_topk_relation_device):
which relation holds between s and o.  The energies of every relation for a pair in float64 with the forward error
bound of the device's fp32 path, and the ranks as a function of a given energy matrix under the fp32-sigmoid rule.
The selection is tests/topk_reference.py's topk_from_energies: it orders any row of floats."""
import numpy as np


def float64_relation_energies(codes, w_rel, queries, R):
    """(E64 [n,R], bound [n,R]): E64 = (c64[s] * c64[o]) @ W64[:R].T and the forward error bound of the fp32 path for
    each entry, (d + 2) 2^-24 (|p| @ |W|.T) -- a length-d fp32 dot product plus the rounding of p = codes[s] * codes[o]
    (the bound tests/test_gpu_topk.py's float64_energies uses on the entity side)"""
    c64 = np.asarray(codes, dtype=np.float64)
    w64 = np.asarray(w_rel, dtype=np.float64)[:R]
    queries = np.asarray(queries)
    p = c64[queries[:, 0]] * c64[queries[:, 2]]
    d = c64.shape[1]
    return p @ w64.T, (d + 2) * 2.0 ** -24 * (np.abs(p) @ np.abs(w64).T)


def sigmoid_f32(x):
    """the score the device compares: evaluated in double, rounded once to float32"""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))).astype(np.float32)


def relation_ranks_from_energies(energies, gold, filter_lists):
    """(raw int32 [n], filtered int32 [n]) from float32 energies [n,R]: raw = #{r' : score[r'] >= score[gold]},
    filtered = raw - #{r' in the row's filter list : score[r'] >= score[gold]} + 1 on fp32 sigmoid scores (saturated
    scores tie).  A list counts once per entry, as the device's walk does: lists hold each relation once."""
    scores = sigmoid_f32(np.asarray(energies, dtype=np.float32))
    raw = np.zeros(len(scores), dtype=np.int32)
    filtered = np.zeros(len(scores), dtype=np.int32)
    for i, g in enumerate(gold):
        reaches = scores[i] >= scores[i, int(g)]
        raw[i] = int(reaches.sum())
        listed = np.asarray(filter_lists[i], dtype=np.int64)
        filtered[i] = raw[i] - int(reaches[listed].sum()) + 1
    return raw, filtered


def energy_order_ranks(energies, gold):
    """raw rank by the ENERGIES (no sigmoid): what the rank would be if saturated scores did not tie"""
    energies = np.asarray(energies, dtype=np.float32)
    return np.array([int((energies[i] >= energies[i, int(g)]).sum()) for i, g in enumerate(gold)], dtype=np.int32)


def known_relation_lists(triples):
    """{(s, o): [r, ...]}, each relation once per pair, in order of first appearance"""
    known = {}
    for s, r, o in np.asarray(triples):
        lst = known.setdefault((int(s), int(o)), [])
        if int(r) not in lst:
            lst.append(int(r))
    return known
