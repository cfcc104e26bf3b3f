"""Numpy reference of the device's top-k selection (include/rgcn.h rgcn_topk_device): the answer as a function of one
row of float32 energies.  Order: (energy descending, entity id ascending), energies compared through the mapping of
floats to unsigned integers in numeric order that csrc/ranking.hip's float_key makes (-0.0 below +0.0)."""
import numpy as np


def float_key(bits):
    """uint32 bit patterns of floats -> uint32 keys in the floats' numeric order"""
    b = np.asarray(bits, dtype=np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def topk_from_energies(row, k, excluded=()):
    """(ids int32 [k], energies float32 [k]) of the k best non-excluded entries of `row`, padded with (-1, -inf)"""
    row = np.ascontiguousarray(row, dtype=np.float32)
    keys = float_key(row.view(np.uint32)).astype(np.int64)
    keep = np.ones(len(row), dtype=bool)
    ex = np.asarray(list(excluded), dtype=np.int64)
    if len(ex):
        keep[ex] = False
    ids = np.flatnonzero(keep)
    order = ids[np.lexsort((ids, -keys[ids]))][:k]
    idx = np.full(k, -1, dtype=np.int32)
    energy = np.full(k, -np.inf, dtype=np.float32)
    idx[:len(order)] = order
    energy[:len(order)] = row[order]
    return idx, energy
