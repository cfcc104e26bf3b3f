"""Who owns the device memory (csrc/dev_pool.h): every allocation of a context belongs to one DevPool -- the context's, a
graph set's, the decoder batch's, the sampler's, the optimizer's, the ranking scratch's -- and rgcn_debug_device_memory
(devtools build) reports the live blocks and bytes summed over them.  Nothing here compares numbers with a reference: the
cases pin that the totals are reproducible from context to context, that growing a reservation leaves what a fresh
reservation of that size holds, that steps allocate nothing once the lazy buffers exist, and that every destroy path runs
(a double free or a stale alias aborts the process; a leak shows as a drifting total).  Contexts are tiny: V = 64, R = 3,
d = 16, L = 2, two blocks / bases, 40 edges."""
import numpy as np
import pytest

from test_gpu_train_step import decoder_batch

pytestmark = pytest.mark.gpu

V, R, D, L, NB, E = 64, 3, 16, 2, 2, 40

CONFIGS = {
    "block": dict(kind="block"),
    "basis": dict(kind="basis"),
    "onehot": dict(kind="basis", input_mode="onehot"),
    "local": dict(kind="block", norm_mode="local"),
    # world = 2 without a communicator: W_self's (and the basis tensors') gradients are views into ONE allocation
    "block_sharded": dict(kind="block", world=2, rank=0),
    "basis_sharded": dict(kind="basis", world=2, rank=0),
}


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library(devtools=True)
    return _native


@pytest.fixture(scope="module")
def graph():
    rng = np.random.RandomState(5)
    return np.stack([rng.randint(0, V, E), rng.randint(0, R, E), rng.randint(0, V, E)], 1).astype(np.int32)


@pytest.fixture(scope="module")
def dcodes():
    return (np.random.RandomState(6).randn(V, D) * 0.1).astype(np.float32)


def engine(native, name="block"):
    cfg = dict(CONFIGS[name])
    return native.Engine(V, R, D, L, cfg.pop("kind"), NB, max_edges=E, devtools=True, **cfg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_create_step_destroy_three_times(native, graph, dcodes, name):
    seen = []
    for _ in range(3):
        eng = engine(native, name)
        try:
            seen.append(eng.device_memory())
            if "sharded" not in name:
                eng.set_graph(graph)
                eng.forward(train=True, seed=1)
                eng.backward(dcodes)
                assert np.isfinite(eng.codes()).all()
                # the step adds the staging copy of the host dcodes (dcodes_own) and nothing else
                assert eng.device_memory() == (seen[-1][0] + 1, seen[-1][1] + 4 * V * D)
        finally:
            eng.close()
    assert seen[0][0] > 0 and seen[0][1] > 0
    assert seen[0] == seen[1] == seen[2], seen


def test_local_norm_with_a_bare_vertex_key_creates_and_destroys(native):
    """(V + 1) 2R >= 2^31 (the shape of test_gpu_local_norm.py's bare-vertex-key case): the only contexts whose graph sets
    hold the destination sort of the message list -- six more buffers per set than the same context under another norm"""
    bigV, bigR = 1100000, 1000
    seen = {}
    for norm in ("local", "intended"):
        eng = native.Engine(bigV, bigR, 4, 1, "basis", 2, norm_mode=norm, max_edges=E, devtools=True)
        try:
            seen[norm] = eng.device_memory()
        finally:
            eng.close()
    assert seen["local"][0] == seen["intended"][0] + 2 * 6


def reserve_case(native, graph, which):
    """(grow in two steps, the final size at once, a smaller request afterwards) for one of the three reservations"""
    if which == "decoder":
        return [lambda e: e.decoder_reserve(64), lambda e: e.decoder_reserve(256)], lambda e: e.decoder_reserve(32)
    if which == "rank":
        return [lambda e: e.rank_reserve(4), lambda e: e.rank_reserve(16)], lambda e: e.rank_reserve(2)
    return [lambda e: e.neighborhood_reserve(graph), lambda e: e.neighborhood_reserve(graph[:30])], None


@pytest.mark.parametrize("which", ["decoder", "rank", "neighborhood"])
def test_growing_a_reservation_leaves_what_a_fresh_one_holds(native, graph, which):
    steps, smaller = reserve_case(native, graph, which)
    grown, fresh = engine(native), engine(native)
    try:
        base = grown.device_memory()
        assert fresh.device_memory() == base
        steps[0](grown)
        first = grown.device_memory()
        assert first[0] > base[0] and first[1] > base[1]
        steps[1](grown)
        steps[1](fresh)
        assert grown.device_memory() == fresh.device_memory(), which
        if which != "neighborhood":
            assert grown.device_memory()[1] > first[1]                  # it did grow
            after = grown.device_memory()
            smaller(grown)
            assert grown.device_memory() == after, which
    finally:
        grown.close()
        fresh.close()


@pytest.mark.parametrize("kind", ["block", "basis"])
def test_train_steps_allocate_nothing_after_the_first(native, graph, kind):
    X, Y = decoder_batch(np.random.RandomState(1), graph, V)
    eng = engine(native, kind)
    held = []
    try:
        eng.decoder_reserve(len(X))
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        held = [eng.to_device(graph), eng.to_device(X), eng.to_device(Y)]
        T, Xd, Yd = held
        before = eng.device_memory()
        seen = []
        for step in range(3):
            eng.train_step_device(T, E, Xd, Yd, len(X), seed=step, reg_param=0.01)
            eng.sync()
            seen.append(eng.device_memory())
        assert seen[0][0] > before[0]                                    # the optimizer's moments and state: lazy
        assert seen[0] == seen[1] == seen[2], seen
        assert np.isfinite(eng.loss())
    finally:
        for b in held:
            b.free()
        eng.close()


def test_steps_with_explicit_masks_allocate_nothing_after_the_first(native, graph, dcodes):
    """minibatch-scale steps under the caller's dropout masks: the [L,V,d] device copy of the masks and the staging copy of
    dcodes appear with the first step and stay"""
    rng = np.random.RandomState(2)
    masks = [(rng.rand(V, D) < 0.8).astype(np.uint8) for _ in range(L)]
    eng = engine(native)
    try:
        eng.set_graph(graph)
        before = eng.device_memory()
        seen = []
        for _ in range(3):
            eng.forward(train=True, masks=masks)
            eng.backward(dcodes)
            seen.append(eng.device_memory())
        assert seen[0] == (before[0] + 2, before[1] + L * V * D + 4 * V * D)
        assert seen[0] == seen[1] == seen[2], seen
    finally:
        eng.close()


def test_minibatch_steps_allocate_nothing_after_the_first(native, graph):
    keep, rate = 30, 2
    N = E * (rate + 1)
    eng = engine(native)
    held = []
    try:
        eng.decoder_reserve(N)
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        held = [eng.to_device(graph), native.DeviceBuffer(eng, 12 * N), native.DeviceBuffer(eng, 4 * N)]
        B, Xd, Yd = held
        seen = []
        for step in range(3):
            eng.train_step_minibatch_device(B, E, keep, 10 + step, rate, 20 + step, Xd, Yd, seed=30 + step, reg_param=0.01)
            eng.sync()
            seen.append(eng.device_memory())
        assert seen[0] == seen[1] == seen[2], seen
    finally:
        for b in held:
            b.free()
        eng.close()


def test_capture_replay_destroy_allocates_the_replay_counter_only(native, graph):
    """one capture / replay / graph_destroy cycle after a train step: the device counter that replays bump (8 bytes,
    allocated by the context's first rgcn_capture_begin and kept) is all it adds; a second cycle adds nothing"""
    X, Y = decoder_batch(np.random.RandomState(1), graph, V)
    eng = engine(native)
    held = []
    try:
        eng.decoder_reserve(len(X))
        eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        held = [eng.to_device(graph), eng.to_device(X), eng.to_device(Y)]
        T, Xd, Yd = held
        eng.train_step_device(T, E, Xd, Yd, len(X), seed=1, reg_param=0.01)
        eng.sync()
        before = eng.device_memory()
        seen = []
        for cycle in range(2):
            eng.capture_begin()
            eng.train_step_device(T, E, Xd, Yd, len(X), seed=50, reg_param=0.01)
            gid = eng.capture_end()
            eng.graph_launch(gid)
            eng.sync()
            assert np.isfinite(eng.loss())
            eng.graph_destroy(gid)
            seen.append(eng.device_memory())
        assert seen[0] == (before[0] + 1, before[1] + 8)
        assert seen[1] == seen[0]
    finally:
        for b in held:
            b.free()
        eng.close()


def test_destroy_in_mid_capture_then_a_new_context_runs(native, graph, dcodes):
    """rgcn_destroy between rgcn_capture_begin and rgcn_capture_end ends the capture, releases every pool and hands the
    streams on; the next context holds what any fresh context holds and runs a forward pass.  (The caller-owned buffers
    belong to a third context, so that they can be freed after the capturing one is gone.)"""
    holder = engine(native)
    try:
        t, dc = holder.to_device(graph), holder.to_device(dcodes)
        fresh = holder.device_memory()
        eng = engine(native)
        try:
            eng.step_device(t, E, dc, train=True, seed=3)               # the lazy allocations happen outside the capture
            eng.sync()
            eng.capture_begin()
            eng.step_device(t, E, dc, train=True, seed=3)
        finally:
            eng.close()                                                  # in mid-capture
        nxt = engine(native)
        try:
            assert nxt.device_memory() == fresh
            nxt.set_graph(graph)
            nxt.forward(train=False)
            assert np.isfinite(nxt.codes()).all()
        finally:
            nxt.close()
        t.free()
        dc.free()
    finally:
        holder.close()
