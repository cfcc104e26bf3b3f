"""The device neighbourhood sampler (csrc/neighborhood.hip) against its float64 mirror, draw by draw, on the grid of
tests/nbr_grid.py.  The batch is a function of (graph, seed, k) alone; tests/nbr_reference.py predicts it on the host and
bounds what float32 can move by a derived margin m = (H + 4) 2^-23: every batch is k rows in strictly increasing edge
order, holds every edge that MUST be in it and none that MAY not -- on a determined draw (all but a fraction of a
percent, tests/test_nbr_grid.py) exactly the mirror's set.  tests/test_gpu_sampler.py compares distributions, which
decides whether percolation is the reference's process; this file decides whether the kernels compute the percolation:
hub rows of 1 / 2 / 3 segments merged with atomicMin, the stop test in the 1-, 2- and 4-sweep regimes, all six select
passes, the compaction at its 1,024-edge block edges, whole components (`use_state`), graphs of self loops only.

Run on an MI355X: 20 tests, 12,782 draws of which the mirror determines 12,766, no mismatch, 5.8 s.  Per case, draws /
determined / largest H / largest margin:
  tiny_a 400 / 400 / 3 / 8.3e-7       tiny_b 250 / 250 / 4 / 9.5e-7        loops_only 200 / 200 / 0 / 4.8e-7
  hub256 1,683 / 1,682 / 14 / 2.2e-6  hub257 2,248 / 2,244 / 17 / 2.5e-6   hub512 830 / 830 / 12 / 1.9e-6
  hub513 835 / 834 / 13 / 2.0e-6      two_hubs 2,320 / 2,318 / 16 / 2.4e-6 one_edge 3 / 3 / 1 / 6.0e-7
  chain60 600 / 600 / 55 / 7.0e-6     chain100 1,000 / 998 / 96 / 1.2e-5   lollipop 1,440 / 1,434 / 65 / 8.2e-6
  blocks1023 168 / 168 / 23 / 3.2e-6  blocks1024 166 / 166 / 23 / 3.2e-6   blocks1025 174 / 174 / 21 / 3.0e-6
  blocks2049 183 / 183 / 23 / 3.2e-6  components 258 / 258 / 39 / 5.1e-6   wide_ids 24 / 24 / 25 / 3.5e-6
Tried once, each as
a one-line change of neighborhood.hip, with test_gpu_sampler.py (without its slow test) beside this file:
  the sweep's minimum over 3 of a lane's 4 entries        here: the four hub cases, two_hubs, the stream test; there: passes
  no segment for the last entry of a hub's list           here: hub257, hub513, the stream test; there: passes
  the stop test reads 8 of the 16 flag slots              here: 11 tests; there: the 1,200-vertex chain
  select pass 3 counts every key, whatever its prefix     here: wide_ids (count flag 32); there: the two 272,115-edge tests
  the sixth select pass 3 bits wide                       here: 15 tests; there: 5 of 7
  the shared branch stores plainly, no atomicMin          passes both: the next launch's `best < cur` repairs a lost minimum,
                                                          and a launch that moved nothing has every segment's best >= d(v)
  one sweep per launch from launch 24 on, same budget     passes both: it changes when a draw settles, not what it
                                                          settles to; a budget too small is refused (flag 8)"""
import numpy as np
import pytest

import nbr_grid as grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


class Rows:
    """rows of a case's graph -> edge ids (every row is unique)"""

    def __init__(self, g, R):
        self.V, self.R = g.V, R
        key = self.key(g.triples)
        self.by = np.argsort(key)
        self.sorted = key[self.by]
        assert (np.diff(self.sorted) > 0).all()

    def key(self, t):
        t = t.astype(np.int64)
        return (t[:, 0] * self.R + t[:, 1]) * self.V + t[:, 2]

    def ids(self, rows):
        key = self.key(rows)
        at = np.minimum(np.searchsorted(self.sorted, key), len(self.sorted) - 1)
        return np.where(self.sorted[at] == key, self.by[at], -1)


def verdict(g, rows_of, seed, k, rows):
    """None when the batch is what the mirror allows, else what is wrong with it; and whether the draw is determined"""
    must, may, info = g.draw(seed, k)
    ids = rows_of.ids(rows)
    if (ids < 0).any():
        return "a row that is no row of the graph", info["determined"]
    if not (np.diff(ids) > 0).all():
        return "edge ids not strictly increasing", info["determined"]
    if not np.isin(must, ids).all():
        return "misses edges %s that must be in it" % np.setdiff1d(must, ids)[:8].tolist(), info["determined"]
    if not np.isin(ids, may).all():
        return "holds edges %s that cannot be in it" % np.setdiff1d(ids, may)[:8].tolist(), info["determined"]
    assert not info["determined"] or np.array_equal(ids, may)
    return None, info["determined"]


def open_engine(native, g, R):
    return native.Engine(g.V, R, 4, 1, "block", 1, max_edges=g.n)


@pytest.mark.parametrize("name", sorted(grid.CASES))
def test_every_draw_is_the_mirrors(native, name):
    """every (seed, k) of the case: one draw, read back, mapped to edge ids, held to the mirror; no draw raises the
    sweep-budget flag (8) or the count flag (32)"""
    g, R = grid.graph(name), grid.relations(name)
    rows_of = Rows(g, R)
    draws = determined = 0
    wrong = []
    with open_engine(native, g, R) as eng:
        eng.neighborhood_reserve(g.triples)
        buf = native.DeviceBuffer(eng, 12 * g.n)
        try:
            for seed, ks in grid.draws(name):
                for k in ks:
                    draws += 1
                    try:
                        eng.sample_neighborhood_device(k, seed, buf)
                        rows = buf.download(np.int32, (k, 3))
                        eng.sync()                                 # reads the device's error flag
                    except native.RgcnError as e:                  # no further draw on a context that reported an error
                        pytest.fail("%s, seed %d, k %d, after %d draws: %s" % (name, seed, k, draws - 1, e))
                    what, det = verdict(g, rows_of, seed, k, rows)
                    determined += det
                    if what is not None:
                        wrong.append((seed, k, what))
        finally:
            buf.free()
    print("%s: %d draws, %d determined, %d mismatches" % (name, draws, determined, len(wrong)))
    assert not wrong, "%s: %d draws, %d determined, %d mismatches; the first: %s" % (
        name, draws, determined, len(wrong), wrong[:5])


REPEAT = (("hub513", 300, ((1, 400), (12, 818), (12, 37))), ("chain100", 300, ((4, 50), (2, 99), (9, 100))))


def test_a_second_reserve_on_a_live_context(native):
    """One context reserves hub513 and draws, reserves chain100 -- another launch budget, so the draw graph is recorded
    again -- and draws, then hub513 again: every batch is, bit for bit, the batch of a context that has seen nothing
    else, and satisfies the mirror."""
    R = max(grid.relations(name) for name, _, _ in REPEAT)
    fresh = {}
    for name, V, sk in REPEAT:
        g = grid.graph(name)
        with native.Engine(V, R, 4, 1, "block", 1, max_edges=g.n) as eng:
            eng.neighborhood_reserve(g.triples)
            buf = native.DeviceBuffer(eng, 12 * g.n)
            try:
                for seed, k in sk:
                    eng.sample_neighborhood_device(k, seed, buf)
                    fresh[(name, seed, k)] = buf.download(np.int32, (k, 3))
                    eng.sync()
                    what, _ = verdict(g, Rows(g, grid.relations(name)), seed, k, fresh[(name, seed, k)])
                    assert what is None, (name, seed, k, what)
            finally:
                buf.free()
    with native.Engine(300, R, 4, 1, "block", 1, max_edges=grid.graph("hub513").n) as eng:
        buf = native.DeviceBuffer(eng, 12 * grid.graph("hub513").n)
        try:
            for name, _, sk in (REPEAT[0], REPEAT[1], REPEAT[0], REPEAT[1]):
                eng.neighborhood_reserve(grid.graph(name).triples)
                for seed, k in sk:
                    eng.sample_neighborhood_device(k, seed, buf)
                    rows = buf.download(np.int32, (k, 3))
                    eng.sync()
                    np.testing.assert_array_equal(rows, fresh[(name, seed, k)], err_msg="%s seed %d k %d" % (name, seed, k))
        finally:
            buf.free()


def test_alternating_streams_are_held_to_the_mirror(native):
    """hub513's draws back to back, even ones on the main stream and odd ones on the prefetch stream as the driver
    issues them, no host wait in between: each batch is the mirror's (test_gpu_sampler.py compares such draws with the
    same code run alone)."""
    name = "hub513"
    g, R = grid.graph(name), grid.relations(name)
    rows_of = Rows(g, R)
    todo = [(seed, k) for seed, ks in grid.draws(name) for k in ks[7::41]]
    assert len(todo) >= 16
    with open_engine(native, g, R) as eng:
        eng.neighborhood_reserve(g.triples)
        bufs = [native.DeviceBuffer(eng, 12 * k) for _, k in todo]
        try:
            for i, (seed, k) in enumerate(todo):
                eng.sample_neighborhood_device(k, seed, bufs[i], on_prefetch_stream=bool(i % 2))
            eng.sync()
            wrong = []
            for i, (seed, k) in enumerate(todo):
                what, _ = verdict(g, rows_of, seed, k, bufs[i].download(np.int32, (k, 3)))
                if what is not None:
                    wrong.append((i, seed, k, what))
        finally:
            for b in bufs:
                b.free()
    assert not wrong, "%d of %d draws: %s" % (len(wrong), len(todo), wrong[:5])
