"""rgcn_step_device ends without making the main stream wait for its side kernels ("Deferred end-of-step
joins"): the weight gradients, their slabs and the bias gradient are still being written on the side streams when the call
returns, and the first call that needs them -- or that rewrites what those kernels read -- takes the join.

Every sequence below is run twice, with the side streams on (joins deferred) and off (rgcn_set_overlap 0: one chain,
nothing to defer), and everything it downloads must be bitwise equal: no kernel's arithmetic depends on the schedule, so a
difference is a missing join.  Each sequence runs once per case."""
import numpy as np
import pytest

from helpers import make_case

pytestmark = pytest.mark.gpu

# (V, R, d, L, nb, E): the small shape of the parity tests, and one whose side kernels run long enough to trail the chain
SHAPES = [(150, 9, 20, 2, 4, 800), (3000, 40, 100, 2, 20, 6000)]


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


class Case:
    def __init__(self, native, shape, overlap):
        V, R, d, L, nb, E = shape
        self.E = E
        params, tri_a, _, dcodes = make_case(V, R, d, L, "block", nb, E, seed=51)
        _, tri_b, _, _ = make_case(V, R, d, L, "block", nb, E, seed=52)
        _, tri_c, _, _ = make_case(V, R, d, L, "block", nb, E, seed=53)
        self.eng = eng = native.Engine(V, R, d, L, "block", nb, keep_prob=0.8, max_edges=E)
        self.held = []
        try:
            eng.set_overlap(overlap)
            eng.set_params(params)
            self.graphs = [eng.to_device(t) for t in (tri_a, tri_b, tri_c)]
            self.dc = eng.to_device(dcodes)
            self.held = self.graphs + [self.dc]
        except Exception:
            self.close()
            raise

    def step(self, g, seed):
        self.eng.step_device(self.graphs[g], self.E, self.dc, train=True, seed=seed)

    def prefetch(self, g):
        self.eng.prefetch_graph_device(self.graphs[g], self.E)

    def outputs(self):
        out = {"codes": self.eng.codes()}
        out.update(("grad_" + n, g) for n, g in self.eng.get_grads().items() if n != "W_relation")
        return out

    def close(self):
        for b in self.held:
            b.free()
        self.held = []
        self.eng.close()


def both(native, shape, sequence):
    """sequence(case) -> {name: array}, with the side streams on and off; -> the two results"""
    res = []
    for overlap in (True, False):
        case = Case(native, shape, overlap)
        try:
            res.append(sequence(case))
        finally:
            case.close()
    return res


def assert_same(on, off):
    assert sorted(on) == sorted(off)
    for k in on:
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)


@pytest.mark.parametrize("shape", SHAPES, ids=["small", "mid"])
def test_step_then_immediate_download(native, shape):
    def seq(c):
        c.step(0, 7)
        return c.outputs()
    assert_same(*both(native, shape, seq))


@pytest.mark.parametrize("shape", SHAPES, ids=["small", "mid"])
def test_step_then_step_on_another_graph(native, shape):
    """the second step builds its graph in line: the build rewrites the message lists the first step's side kernels read"""
    def seq(c):
        c.step(0, 7)
        c.step(1, 8)
        return c.outputs()
    assert_same(*both(native, shape, seq))


@pytest.mark.parametrize("shape", SHAPES, ids=["small", "mid"])
def test_step_prefetch_third_graph_step(native, shape):
    """pipelined: the prefetch of graph 2 rebuilds the set step 0 used while step 1's side kernels are pending"""
    def seq(c):
        c.step(0, 7)
        c.prefetch(1)
        c.step(1, 8)
        c.prefetch(2)
        c.step(2, 9)
        first = c.outputs()
        c.prefetch(0)
        c.step(0, 10)
        out = c.outputs()
        out.update(("first_" + k, v) for k, v in first.items())
        return out
    assert_same(*both(native, shape, seq))


@pytest.mark.parametrize("shape", SHAPES, ids=["small", "mid"])
def test_step_then_optimizer(native, shape):
    def seq(c):
        c.eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        c.step(0, 7)
        c.eng.optimizer_step()
        out = {"param_" + n: p for n, p in c.eng.get_params().items()}
        c.step(1, 8)
        c.eng.optimizer_step()
        out.update(("param2_" + n, p) for n, p in c.eng.get_params().items())
        return out
    assert_same(*both(native, shape, seq))


@pytest.mark.parametrize("shape", SHAPES[:1], ids=["small"])
def test_step_then_train_step(native, shape):
    V, R = shape[0], shape[1]
    rng = np.random.RandomState(5)
    N = 600
    X = np.stack([rng.randint(0, V, N), rng.randint(0, R, N), rng.randint(0, V, N)], 1).astype(np.int32)
    Y = (rng.rand(N) < 0.5).astype(np.float32)

    def seq(c):
        c.eng.decoder_reserve(N)
        c.eng.optimizer_config(lr=0.01, max_grad_norm=1.0)
        xd, yd = c.eng.to_device(X), c.eng.to_device(Y)
        c.held += [xd, yd]
        c.step(0, 7)
        c.eng.train_step_device(c.graphs[1], c.E, xd, yd, N, seed=8, reg_param=0.01)
        out = {"param_" + n: p for n, p in c.eng.get_params().items()}
        out["loss"] = np.float64(c.eng.loss())
        return out
    assert_same(*both(native, shape, seq))


@pytest.mark.parametrize("shape", SHAPES, ids=["small", "mid"])
def test_step_then_capture(native, shape):
    def seq(c):
        c.step(0, 7)
        c.eng.capture_begin()
        c.step(1, 8)
        gid = c.eng.capture_end()
        c.eng.graph_launch(gid)
        out = c.outputs()
        c.step(0, 9)                 # a deferred step, then a replay that rewrites everything its side kernels touch
        c.eng.graph_launch(gid)
        out.update(("again_" + k, v) for k, v in c.outputs().items())
        c.eng.graph_destroy(gid)
        return out
    assert_same(*both(native, shape, seq))


@pytest.mark.parametrize("shape", SHAPES, ids=["small", "mid"])
def test_step_then_close(native, shape):
    """a context destroyed with its gradients pending; the next context on the pooled streams computes the same"""
    def seq(c):
        c.step(0, 7)
        return {}
    both(native, shape, seq)

    def seq2(c):
        c.step(0, 7)
        return c.outputs()
    assert_same(*both(native, shape, seq2))


@pytest.mark.parametrize("shape", SHAPES[:1], ids=["small"])
def test_step_then_forward_backward(native, shape):
    """the phase-free calls after a deferred step: rgcn_forward overwrites the activations, rgcn_backward the gradients"""
    def seq(c):
        c.step(0, 7)
        c.eng.forward(train=True, seed=11)
        c.eng.backward_device(c.dc)
        return c.outputs()
    assert_same(*both(native, shape, seq))
