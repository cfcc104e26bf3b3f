"""The three algorithms of Algorithm.Name on the GPU (csrc/optimizer.hip k_adam, k_adagrad, k_sgd behind k_sqnorm_part and
k_clip_scale) and the optimizer's state through the C ABI (rgcn_get/set_optimizer_slot, _step): every update against the
float64 mirror of tests/optimizer_reference.py fed with the DEVICE's gradients, pre-step weights and pre-step slots, within
the bounds that module counts from the kernels, no element excused; the sharded phase API, rank by rank; state handed from
one context to another; a captured step; the training driver with --save-optimizer-state / --resume.

Shapes of the real-gradient cases, with 256 x 8 = 2048 elements per workgroup and 4 per lane and load:
  block  V 257, R 5, d 9, 3 blocks, L 2: W_emb 2313 = one full workgroup + a tail of 265 (66 quads and one element: the
         one-by-one path inside a vectorised tensor), W_self 81 and b_emb 9 (less than a workgroup, odd), W_f / W_b 135;
  basis  B 2, V 130, R 8, d 20, L 2: W_emb 2600 (a second workgroup), the [d, B, d] tensors in their device layout;
  embedding  V 300, d 12: W_emb 3600, W_relation 3600 of which the first R rows (72 elements) are updated.
Shapes of the injected-gradient cases (an embedding engine hands backward()'s argument to the optimizer as dL/dW_emb, bit
for bit, so a [V, d] tensor of any size gets any gradient): INJECTED below."""
import os

import numpy as np
import pytest

import optimizer_reference as ref
from helpers import make_case

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = 1, 4, 5
RATES = {"AdaGrad": 0.1, "GradientDescent": 0.5, "Adam": 0.01}
CASES = {
    "block": dict(kind="block", V=257, R=5, d=9, nb=3, L=2, E=300),
    "basis": dict(kind="basis", V=130, R=8, d=20, nb=2, L=2, E=300),
    "embedding": dict(kind="embedding", V=300, R=6, d=12, nb=1, L=0, E=0),
}


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


def decoder_batch(rng, triples, V, neg_rate=3):
    pos = triples.copy()
    neg = np.tile(pos, (neg_rate, 1))
    side = rng.rand(len(neg)) < 0.5
    rnd = rng.randint(0, V, len(neg))
    neg[side, 2] = rnd[side]
    neg[~side, 0] = rnd[~side]
    X = np.concatenate([pos, neg]).astype(np.int32)
    Y = np.concatenate([np.ones(len(pos)), np.zeros(len(neg))]).astype(np.float32)
    return X, Y


def case_data(c, seed=77):
    """(params, graph triples or None, X, Y) of a case; the embedding kind has no graph and its own three weights"""
    rng = np.random.RandomState(seed)
    if c["kind"] == "embedding":
        V, R, d = c["V"], c["R"], c["d"]
        params = {"W_emb": rng.randn(V, d).astype(np.float32) * 0.5, "b_emb": np.zeros(d, np.float32),
                  "W_relation": rng.randn(V, d).astype(np.float32)}
        pos = np.stack([rng.randint(0, V, 300), rng.randint(0, R, 300), rng.randint(0, V, 300)], 1).astype(np.int32)
        triples = None
    else:
        params, triples, _, _ = make_case(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], c["E"], seed=seed)
        pos = triples
    X, Y = decoder_batch(rng, pos, c["V"])
    return params, triples, X, Y


def engine_of(native, c, **kw):
    return native.Engine(c["V"], c["R"], c["d"], c["L"], c["kind"], c["nb"], max_edges=c["E"], **kw)


def moved_names(eng):
    """the parameters the optimizer moves: all but the biases nothing reads -- the layers' b1, b2, ... and, of the
    embedding kind (use_bias=False), b_emb"""
    return [n for n in eng.param_names if not (n.startswith("b") and n[1:].isdigit()) and not (eng.L == 0 and n == "b_emb")]


class Run(object):
    """an engine with a case's weights, its batch on the device and an optimizer; step(seed) is one train step"""

    def __init__(self, native, c, algorithm, max_norm=1.0, data=None, set_params=True, **kw):
        self.c = c
        self.params, self.triples, self.X, self.Y = data or case_data(c)
        self.eng = engine_of(native, c, **kw)
        self.bufs = []
        try:
            if set_params:
                self.eng.set_params(self.params)
            self.eng.decoder_reserve(len(self.X))
            self.eng.optimizer_config(lr=RATES[algorithm], max_grad_norm=max_norm, algorithm=algorithm)
            self.td = self.eng.to_device(self.triples) if self.triples is not None else None
            self.xd, self.yd = self.eng.to_device(self.X), self.eng.to_device(self.Y)
            self.bufs = [b for b in (self.td, self.xd, self.yd) if b is not None]
        except Exception:
            self.close()
            raise

    def step(self, seed):
        self.eng.train_step_device(self.td, self.c["E"], self.xd, self.yd, len(self.X), seed=seed, reg_param=0.01)

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ------------------------------------------------------------------ one step held to the mirror
ADAM_DEFAULTS = dict(beta1=ref.f32(0.9), beta2=ref.f32(0.999), eps=ref.f32(1e-8))


def excess(err, bound):
    """max err / bound; an error where nothing is allowed is infinite"""
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def read_slots(eng, names):
    return {n: tuple(eng.get_optimizer_slot(n, s) for s in range(eng.optimizer_slot_count())) for n in names}


def mirror_state(algorithm, slots):
    if algorithm == "Adam":
        return {n: (s[0], s[1]) for n, s in slots.items()}
    return {n: s[0] for n, s in slots.items()} if algorithm == "AdaGrad" else None


def hold_step(label, algorithm, names, cur, grads, pre, new, post, lr, max_norm, step_count=0, hyper=None, scale=None,
              select=None, per_tensor_size=True, accumulator_rtol=None):
    """Mirrors one step from the pre-step values and asserts the bounds of optimizer_reference on EVERY element of the
    change and (post given) of the slots; prints max err / bound per tensor and quantity first.  select: {name: index}, the
    elements of a tensor that are this context's to move; accumulator_rtol: AdaGrad's, where a test holds a tighter one than
    optimizer_reference.accumulator_rtol.  Returns (mirrored change, mirrored state, {name: bound})."""
    clipped = max_norm > 0
    hyper = hyper or (ADAM_DEFAULTS if algorithm == "Adam" else {})
    want, state = ref.step(algorithm, cur, grads, mirror_state(algorithm, pre) if pre is not None else None, names, lr,
                           max_norm, step_count=step_count, scale=scale, **hyper)
    bounds, largest, widest = {}, 0.0, 0.0
    for n in names:
        pick = (select or {}).get(n, Ellipsis)
        old = cur[n].astype(np.float64)
        got = new[n].astype(np.float64) - old
        bounds[n] = ref.update_bound(old, state[n].U if algorithm == "Adam" else want[n], clipped)
        ratios = [("change", excess(np.abs(got - want[n])[pick], bounds[n][pick]))]
        zero = old[pick] == 0                      # there the bound is the update's alone: no rounding of w to hide behind
        ratios.append(("change(w=0)", excess(np.abs(got - want[n])[pick][zero], bounds[n][pick][zero])))
        if post is not None and algorithm == "Adam":
            ratios.append(("m", excess(np.abs(post[n][0] - state[n].m)[pick], ref.adam_m_bound(state[n].A, clipped)[pick])))
            ratios.append(("v", excess(np.abs(post[n][1] - state[n].v)[pick], ref.adam_v_bound(state[n].v, clipped)[pick])))
        if post is not None and algorithm == "AdaGrad":
            ratios.append(("accumulator", excess(np.abs(post[n][0] - state[n])[pick],
                                                 (accumulator_rtol or ref.accumulator_rtol(clipped)) * np.abs(state[n])[pick])))
        big, wide = float(np.abs(want[n][pick]).max()), float(bounds[n][pick].max())
        print("HELD %s %s %s %-10s max|d_ref| %.3e  max bound %.3e  max err/bound %s"
              % (algorithm, "clip" if clipped else "noclip", label, n, big, wide,
                 "  ".join("%s %.3f" % r for r in ratios)))
        if per_tensor_size:
            assert big >= 100 * wide, (label, n, big, wide)
        largest, widest = max(largest, big), max(widest, wide)
        for what, ratio in ratios:
            assert ratio <= 1.0, (label, n, what, ratio)
    assert largest >= 100 * widest, (label, largest, widest)          # the comparison could fail: a change 100 bounds large
    return want, state, bounds


def worst_miss(got_change, wrong_change, bounds, names, select=None):
    """by how many bounds a wrong mirror misses the device's change, at the element where it misses most"""
    return max(excess(np.abs(got_change[n] - np.nan_to_num(wrong_change[n], nan=np.inf))[(select or {}).get(n, Ellipsis)],
                      bounds[n][(select or {}).get(n, Ellipsis)]) for n in names)


# ------------------------------------------------------------------ the update against the float64 mirror
@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["unclipped", "clip-1"])
@pytest.mark.parametrize("algorithm", ["Adam", "AdaGrad", "GradientDescent"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_update_matches_the_float64_mirror(native, case, algorithm, max_norm):
    """Three train steps.  After each: the device's gradients, weights and slots; the step mirrored in float64 from those
    gradients and the PRE-step weights and slots; compared is the CHANGE new - old (an update is about 1e-4 of a weight: at
    a tolerance made for weights no update at all would pass), per element, within
        2^-23 |w| + 8 x 2^-23 |d_ref|      (max_grad_norm 0: the rounding of w - u, and at most eight roundings in u)
        2^-23 |w| + 13 x 2^-23 |d_ref|     (max_grad_norm 1: the clip scale's 5 x 2^-23 on top)
    with Adam's U (the update before its two terms cancel) in place of |d_ref|; AdaGrad's accumulators within 8 x 2^-23
    relative, clipped or not, Adam's m and v within optimizer_reference's bounds.  Every comparison first shows that
    it could fail: the largest mirrored change is at least 100 times the largest error allowed.  AdaGrad: the mirror
    started from accumulators 0.1 lower (an initial accumulator of 0) misses the bound by more than 100 times; Adam: so do
    the three wrong Adams of optimizer_reference.ADAM_VARIANTS.  What has no gradient does not change by a bit."""
    c, lr = CASES[case], ref.f32(RATES[algorithm])
    with Run(native, c, algorithm, max_norm) as run:
        eng = run.eng
        names = moved_names(eng)
        slots = eng.optimizer_slot_count()
        assert slots == {"Adam": 2, "AdaGrad": 1, "GradientDescent": 0}[algorithm]
        cur = eng.get_params()
        pre = read_slots(eng, names)
        if slots:
            initial = np.float32(0.1 if algorithm == "AdaGrad" else 0.0)
            assert all((a == initial).all() for held in pre.values() for a in held)
        for step in range(3):
            run.step(seed=500 + step)
            assert np.isfinite(eng.loss())
            grads = eng.get_grads()
            new = eng.get_params()
            post = read_slots(eng, names)
            assert eng.optimizer_step_count() == step + 1
            want, _, bounds = hold_step("%s step %d" % (case, step + 1), algorithm, names, cur, grads, pre, new, post, lr,
                                        max_norm, step_count=step, accumulator_rtol=ref.ACCUMULATOR_RTOL)
            got = {n: new[n].astype(np.float64) - cur[n] for n in names}
            if algorithm == "AdaGrad":
                zero_start = {n: pre[n][0].astype(np.float64) - 0.1 for n in names}
                with np.errstate(invalid="ignore", divide="ignore"):
                    unfilled, _ = ref.step(algorithm, cur, grads, zero_start, names, lr, max_norm)
                assert worst_miss(got, unfilled, bounds, names) > 100, step
            if algorithm == "Adam":
                for variant in ref.ADAM_VARIANTS:
                    wrong, _ = ref.step(algorithm, cur, grads, mirror_state(algorithm, pre), names, lr, max_norm,
                                        step_count=step, variant=variant, **ADAM_DEFAULTS)
                    assert worst_miss(got, wrong, bounds, names) > 100, (step, variant)
            for n in eng.param_names:
                if n not in names:
                    assert np.array_equal(new[n], cur[n]), n                         # no gradient: not a bit
            R = c["R"]
            assert np.array_equal(new["W_relation"][R:], cur["W_relation"][R:])        # rows past RelationCount
            assert not np.array_equal(new["W_relation"][:R], cur["W_relation"][:R])
            for slot in post["W_relation"]:
                assert (slot[R:] == initial).all()
            cur, pre = new, post


# ------------------------------------------------------------------ injected gradients at the kernels' boundaries
# (V, d) of an embedding engine, R = 3: W_emb has n = V d elements; a workgroup takes 2048, a lane 4 per load
INJECTED = [(3, 5),         # 15: less than one wave
            (89, 23),       # 2047: the last quad short by one
            (64, 32),       # 2048: exactly one workgroup
            (241, 17),      # 4097 = 2 x 2048 + 1: a workgroup of one element
            (82, 25),       # 2050 = 2048 + 2
            (683, 9),       # 6147 = 3 x 2048 + 3
            (8400, 500)]    # 4,200,000: 2051 + 1 block partials, the second trip of k_clip_scale's eight-at-a-time loop
INJECTED_R = 3
_inputs = {}


def injected_inputs(n):
    """optimizer_reference.injected_case(n, seed n), made once and shared read-only"""
    if n not in _inputs:
        w, grads = ref.injected_case(n, seed=n, steps=3 if n < 1000000 else 1)
        for a in [w] + grads:
            a.setflags(write=False)
        _inputs[n] = (w, grads)
    return _inputs[n]


def heads(tensors, names):
    """the elements the optimizer moves: of W_relation the first R rows"""
    return {n: tensors[n][:INJECTED_R] if n == "W_relation" else tensors[n] for n in names}


class Injected(object):
    """An embedding engine [V, d] with an optimizer.  step(w, g): W_emb = w, a forward pass, the decoder's pass over a
    50-triple batch (it leaves W_relation's first R rows a real gradient; decoder=False: none, the gradient is g alone),
    backward(g) -- which makes dL/dW_emb = g -- and optimizer_step() alone; everything read back before and after."""
    names = ["W_emb", "W_relation"]

    def __init__(self, native, V, d, algorithm, max_norm, lr=None, **hyper):
        self.V, self.d, self.algorithm, self.max_norm = V, d, algorithm, max_norm
        self.lr = ref.f32(RATES[algorithm] if lr is None else lr)
        self.hyper = {k: ref.f32(v) for k, v in hyper.items()} or None
        rng = np.random.RandomState(1000 + V)
        self.eng = native.Engine(V, INJECTED_R, d, 0, "embedding", 1)
        self.bufs = []
        try:
            assert moved_names(self.eng) == self.names
            self.eng.set_params({"W_emb": np.zeros((V, d), np.float32), "b_emb": (0.05 * rng.randn(d)).astype(np.float32),
                                 "W_relation": rng.randn(V, d).astype(np.float32)})
            X = np.stack([rng.randint(0, V, 50), rng.randint(0, INJECTED_R, 50), rng.randint(0, V, 50)], 1).astype(np.int32)
            Y = (rng.rand(50) < 0.3).astype(np.float32)
            self.eng.decoder_reserve(50)
            self.eng.optimizer_config(lr=self.lr, max_grad_norm=max_norm, algorithm=algorithm, **(self.hyper or {}))
            self.bufs = [self.eng.to_device(X), self.eng.to_device(Y)]
        except Exception:
            self.close()
            raise

    def step(self, w, g, seed=0, decoder=True):
        eng, shape = self.eng, (self.V, self.d)
        eng.set_param("W_emb", w.reshape(shape))
        eng.forward(train=True, seed=seed)
        if decoder:
            eng.decoder_loss_backward_device(self.bufs[0], self.bufs[1], 50, 0.01)
        eng.backward(g.reshape(shape))
        self.grads, self.cur, self.pre, self.t0 = eng.get_grads(), eng.get_params(), read_slots(eng, self.names), \
            eng.optimizer_step_count()
        assert np.array_equal(self.grads["W_emb"], g.reshape(shape))                 # the gradient is the one handed in
        assert not self.grads["W_relation"][INJECTED_R:].any() and self.grads["W_relation"][:INJECTED_R].any() == decoder
        eng.optimizer_step()
        self.new, self.post, self.t1 = eng.get_params(), read_slots(eng, self.names), eng.optimizer_step_count()
        assert self.t1 == self.t0 + 1
        self.got = {n: self.new[n][:len(self.head(self.cur)[n])].astype(np.float64) - self.head(self.cur)[n] for n in self.names}

    def head(self, tensors):
        return heads(tensors, self.names)

    def head_slots(self, slots):
        return {n: tuple(a[:INJECTED_R] if n == "W_relation" else a for a in slots[n]) for n in self.names}

    def mirror(self, max_norm=None, **kw):
        """ref.step from the values read before the last step; keywords: a wrong mirror's"""
        return ref.step(self.algorithm, self.head(self.cur), self.head(self.grads),
                        mirror_state(self.algorithm, self.head_slots(self.pre)), self.names, self.lr,
                        self.max_norm if max_norm is None else max_norm, step_count=self.t0,
                        **dict(self.hyper or (ADAM_DEFAULTS if self.algorithm == "Adam" else {}), **kw))

    def hold(self, label):
        """the last step against the mirror, every element; then what must not have moved by a bit"""
        R, clipped, algorithm = INJECTED_R, self.max_norm > 0, self.algorithm
        hyper = self.hyper or ADAM_DEFAULTS
        scale = ref.clip_scale(self.head(self.grads), self.names, self.max_norm)
        if algorithm == "Adam":                       # the inputs keep every non-zero intermediate a normal float32
            for n in self.names:
                g = self.head(self.grads)[n].astype(np.float64) * scale
                small = (1.0 - hyper["beta2"]) * g[g != 0] ** 2
                assert not small.size or small.min() >= 2.0 ** -126, (label, n, float(small.min()))
        want, state, bounds = hold_step(label, algorithm, self.names, self.head(self.cur), self.head(self.grads),
                                        self.head_slots(self.pre), self.head(self.new), self.head_slots(self.post), self.lr,
                                        self.max_norm, step_count=self.t0, hyper=self.hyper, per_tensor_size=False)
        for n in self.names:                           # a zero gradient on zero momentum: nothing moves
            g, w0, w1 = (self.head(x)[n] for x in (self.grads, self.cur, self.new))
            still = g == 0
            if algorithm == "Adam":
                m0, v0 = self.head_slots(self.pre)[n]
                m1, v1 = self.head_slots(self.post)[n]
                still = still & (m0 == 0)
                assert not m1[still].any(), (label, n)
                decayed = hyper["beta2"] * v0[still].astype(np.float64)
                assert (np.abs(v1[still] - decayed) <= 2 * ref.U24 * decayed).all(), (label, n)
            elif algorithm == "AdaGrad":
                assert np.array_equal(self.head_slots(self.post)[n][0][still], self.head_slots(self.pre)[n][0][still]), (label, n)
            assert still.any() or n != "W_emb" or g.size < 100
            assert np.array_equal(w1[still], w0[still]), (label, n)
        assert np.array_equal(self.new["W_relation"][R:], self.cur["W_relation"][R:]), label
        for before, after in zip(self.pre["W_relation"], self.post["W_relation"]):
            assert np.array_equal(after[R:], before[R:]), label
        assert np.array_equal(self.new["b_emb"], self.cur["b_emb"]) and self.new["b_emb"].any(), label
        return want, state, bounds, scale

    def tells_wrong_adams(self, bounds, label, variants=ref.ADAM_VARIANTS):
        for variant in variants:
            wrong, _ = self.mirror(variant=variant)
            assert worst_miss(self.got, wrong, bounds, self.names) > 100, (label, variant)

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["unclipped", "clip-1"])
@pytest.mark.parametrize("algorithm", ["Adam", "AdaGrad", "GradientDescent"])
@pytest.mark.parametrize("shape", INJECTED, ids=["%dx%d" % s for s in INJECTED])
def test_injected_gradients_at_the_kernels_boundaries(native, shape, algorithm, max_norm):
    """Three optimizer steps (one at 4.2 M elements) on gradients of optimizer_reference.injected_case: fifteen decades of
    magnitude, exact zeros, a tenth where Adam's eps decides, a tenth whose m cancels, a step-2 gradient a thousand times
    smaller (another clip scale); half of the weights exactly 0 before every step, where the bound is the update's alone.
    After every step every element of the change, of m and v and of AdaGrad's accumulator is inside the bounds counted in
    optimizer_reference, and the largest mirrored change is 100 times the largest bound.  Adam: the three wrong Adams miss
    the bound by more than 100 times somewhere, and so does the unclipped mirror on a clipped step after the first.  A zero
    gradient on zero momentum moves nothing by a bit (v decays to b2 v0 within 2 x 2^-24); nor do W_relation's rows past
    R, their slots, or b_emb."""
    V, d = shape
    w, grads = injected_inputs(V * d)
    with Injected(native, V, d, algorithm, max_norm) as run:
        assert (w == 0).sum() == (V * d) // 2
        clipped_later = 0
        for step, g in enumerate(grads):
            label = "%dx%d step %d" % (V, d, step + 1)
            run.step(w, g, seed=step)
            _, _, bounds, scale = run.hold(label)
            if algorithm == "Adam":
                run.tells_wrong_adams(bounds, label)
                if max_norm > 0 and step >= 1 and scale < 0.99:     # (a norm below the threshold: the two mirrors are one)
                    unclipped, _ = run.mirror(max_norm=0.0)
                    assert worst_miss(run.got, unclipped, bounds, run.names) > 100, label
                    clipped_later += 1
        assert run.eng.optimizer_step_count() == len(grads)
        if algorithm == "Adam" and max_norm > 0 and len(grads) == 3:
            assert clipped_later >= (1 if V * d < 100 else 2)


def preset_state(n, g, seed):
    """m0 of the gradient's magnitude and the opposite sign, v0 log-uniform in [1e-30, 1e6]"""
    rng = np.random.RandomState(seed)
    return (-g).astype(np.float32), (10.0 ** rng.uniform(-30, 6, n)).astype(np.float32)


def put_state(run, m0, v0):
    shape = (run.V, run.d)
    run.eng.set_optimizer_slot("W_emb", 0, m0.reshape(shape))
    run.eng.set_optimizer_slot("W_emb", 1, v0.reshape(shape))
    assert np.array_equal(run.eng.get_optimizer_slot("W_emb", 1), v0.reshape(shape))


TWO_SHAPES = [(89, 23), (241, 17)]
two_shapes = pytest.mark.parametrize("shape", TWO_SHAPES, ids=["%dx%d" % s for s in TWO_SHAPES])


@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["unclipped", "clip-1"])
@two_shapes
def test_adam_from_a_preset_state(native, shape, max_norm):
    """one step from an m0 that opposes the gradient and a v0 spread over thirty-six decades"""
    V, d = shape
    w, grads = injected_inputs(V * d)
    with Injected(native, V, d, "Adam", max_norm) as run:
        put_state(run, *preset_state(V * d, grads[0], seed=V))
        run.step(w, grads[0])
        assert run.pre["W_emb"][0].any() and run.pre["W_emb"][1].all()
        _, _, bounds, _ = run.hold("%dx%d preset" % shape)
        run.tells_wrong_adams(bounds, "preset")


@pytest.mark.parametrize("t0", [9, 999, 99999, 2 ** 24 - 2])
@two_shapes
def test_adam_at_a_set_step_count(native, shape, t0):
    """rgcn_set_optimizer_step puts t0 in front of the step: the mirror's rate is that of t0 + 1, the count afterwards is
    t0 + 1 -- 2^24 - 1 at the last value, the largest the device's float holds exactly -- and is accepted back.  Up to a
    thousand steps a rate one step late or uncorrected misses by more than 100 bounds; from 1e5 steps on the correction is
    1 to the last bit of a double and there is nothing left to tell."""
    V, d = shape
    w, grads = injected_inputs(V * d)
    with Injected(native, V, d, "Adam", 1.0) as run:
        run.eng.set_optimizer_step_count(t0)
        run.step(w, grads[0])
        assert run.t0 == t0 and run.t1 == t0 + 1
        _, _, bounds, _ = run.hold("%dx%d t0 %d" % (V, d, t0))
        if t0 < 1000:
            run.tells_wrong_adams(bounds, t0)
        else:
            assert ref.adam_rate(run.lr, ADAM_DEFAULTS["beta1"], ADAM_DEFAULTS["beta2"], t0 + 1) == run.lr
            run.tells_wrong_adams(bounds, t0, variants=("eps_under_root",))
        run.eng.set_optimizer_step_count(run.eng.optimizer_step_count())
        assert run.eng.optimizer_step_count() == t0 + 1


@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["unclipped", "clip-1"])
@two_shapes
def test_adam_with_other_hyper_parameters(native, shape, max_norm):
    """beta1 0.5, beta2 0.9, eps 1e-3, lr 0.003, from a preset state (the betas weigh it; m0 is half the gradient's
    magnitude: at the full one b1 m0 + (1 - b1) g would be 0 everywhere) at step count 4"""
    V, d = shape
    w, grads = injected_inputs(V * d)
    with Injected(native, V, d, "Adam", max_norm, lr=0.003, beta1=0.5, beta2=0.9, eps=1e-3) as run:
        m0, v0 = preset_state(V * d, grads[0], seed=V + 1)
        put_state(run, np.float32(0.5) * m0, v0)
        run.eng.set_optimizer_step_count(4)
        run.step(w, grads[0])
        _, _, bounds, _ = run.hold("%dx%d hyper" % shape)
        run.tells_wrong_adams(bounds, "hyper")
        defaults, _ = run.mirror(**ADAM_DEFAULTS)
        assert worst_miss(run.got, defaults, bounds, run.names) > 100


@pytest.mark.parametrize("algorithm", ["Adam", "GradientDescent"])
@two_shapes
def test_clip_threshold(native, shape, algorithm):
    """A gradient whose only non-zero element, the tensor's last, equals max_grad_norm = 1 (no decoder pass: W_relation's
    gradient is zero): the norm is exactly the threshold, the scale exactly 1, and weights and slots are bitwise those of
    the same step without a clip.  The element doubled: the scale is 0.5, and the change matches the mirror at that scale.
    The element's weight is 0, so GradientDescent shows the scale itself: d = -lr s g."""
    V, d = shape
    n = V * d
    w = injected_inputs(n)[0].copy()
    w[-1] = 0.0
    seen = {}
    for max_norm, value in ((1.0, 1.0), (0.0, 1.0), (1.0, 2.0)):
        g = np.zeros(n, np.float32)
        g[-1] = value
        with Injected(native, V, d, algorithm, max_norm) as run:
            run.step(w, g, decoder=False)
            scale = ref.clip_scale(run.head(run.grads), run.names, max_norm)
            assert scale == (0.5 if value == 2.0 else 1.0)
            label = "%dx%d threshold norm %g max_norm %g" % (V, d, value, max_norm)
            hold_step(label, algorithm, ["W_emb"], run.cur, run.grads, run.pre, run.new, run.post, run.lr, max_norm,
                      hyper=run.hyper)
            assert np.array_equal(run.new["W_relation"], run.cur["W_relation"])
            moved = np.flatnonzero(run.new["W_emb"].ravel() != run.cur["W_emb"].ravel())
            assert moved.tolist() == [n - 1]
            if algorithm == "GradientDescent":
                d_ref = -run.lr * scale * value
                assert abs(float(run.new["W_emb"].ravel()[-1]) - d_ref) <= 13 * ref.EPS32 * abs(d_ref)
            seen[(max_norm, value)] = (run.new, run.post)
    on, off = seen[(1.0, 1.0)], seen[(0.0, 1.0)]
    for name in on[0]:
        assert np.array_equal(on[0][name], off[0][name]), name
    for name in on[1]:
        for a, b in zip(on[1][name], off[1][name]):
            assert np.array_equal(a, b), name


# ------------------------------------------------------------------ sharded: the phase API with the host as the collective
@pytest.mark.parametrize("algorithm", ["AdaGrad", "GradientDescent"])
def test_sharded_steps_match_the_unsharded_run(native, algorithm):
    """test_sharded_train_steps_match_the_unsharded_run (tests/test_gpu_train_step.py) with the two algorithms, world 2 on
    one GPU, block kind at d = 9: the replicated gradients are slices of one buffer, 9- and 81-element ones among them,
    so most slices start off a 16-byte boundary and go element by element.  Its criterion: the loss of every step to
    1e-5, and after four steps every weight within 2 x lr x steps of the unsharded run's, all but 0.2 % within 2e-4."""
    from relationprediction_amd.sharding import lpt_partition
    V, R, d, nb, L, E, world = 90, 10, 9, 3, 2, 600, 2
    kind, lr, steps = "block", RATES[algorithm], 4
    params, triples, _, _ = make_case(V, R, d, L, kind, nb, E, seed=21)
    X, Y = decoder_batch(np.random.RandomState(2), triples[:200], V)
    owner = lpt_partition(np.bincount(triples[:, 1], minlength=R), world)
    single = native.Engine(V, R, d, L, kind, nb, max_edges=E)
    engs = [native.Engine(V, R, d, L, kind, nb, max_edges=E, rank=r, world=world) for r in range(world)]
    held = []

    def exchange(which):
        total = sum(e.read_buffer(which) for e in engs)
        for e in engs:
            e.write_buffer(which, total)

    def same_trajectory(got, want, what):
        diff = np.abs(got - want)
        assert float(diff.max()) <= 2 * lr * steps + 1e-6, what
        assert float((diff > 2e-4).mean()) <= 0.002, (what, float((diff > 2e-4).mean()))

    try:
        for e in [single] + engs:
            e.set_params(params)
            e.decoder_reserve(len(X))
            e.optimizer_config(lr=lr, max_grad_norm=1.0, algorithm=algorithm)
            held.append((e.to_device(triples), e.to_device(X), e.to_device(Y)))
        for e in engs:
            e.set_relation_owner(owner)
        for step in range(steps):
            T, Xd, Yd = held[0]
            single.train_step_device(T, E, Xd, Yd, len(X), seed=100 + step, reg_param=0.01)
            for e in engs:
                e.set_graph(triples)
                e.forward_begin(train=True, seed=100 + step)
            for l in range(1, L + 1):
                for e in engs:
                    e.forward_layer_partial(l)
                exchange(native.BUF_EXCHANGE)
                for e in engs:
                    e.forward_layer_finish(l)
            for e, (_, Xd, Yd) in zip(engs, held[1:]):
                e.decoder_loss_backward_device(Xd, Yd, len(X), 0.01)
                e.backward_begin()
            for l in range(L, 0, -1):
                for e in engs:
                    e.backward_layer_partial(l)
                exchange(native.BUF_EXCHANGE)
                exchange(native.BUF_DSELF_EXCHANGE)
                for e in engs:
                    e.backward_layer_finish(l)
            for e in engs:
                e.backward_end()
                e.optimizer_norm_partial()
            exchange(native.BUF_NORM_EXCHANGE)
            for e in engs:
                e.optimizer_apply()
            for e in engs:
                assert abs(e.loss() - single.loss()) <= 1e-5 * max(1.0, abs(single.loss())), step
        want = single.get_params()
        for r, e in enumerate(engs):
            got = e.get_params()
            for k, w in want.items():
                if k.startswith(("W_f", "W_b")):
                    mine = owner == r
                    assert mine.any()
                    same_trajectory(got[k][mine], w[mine], (r, k))
                    assert np.array_equal(got[k][~mine], params[k][~mine]), (r, k)       # never touched off-owner
                else:
                    same_trajectory(got[k], w, (r, k))
        moved = max(float(np.abs(want[k] - params[k]).max()) for k in want)
        assert moved > 1e-3, moved                                  # the steps did happen
        # the state of a sharded context is not for reading: a relation's is current on its owner only
        for call in (lambda: engs[0].get_optimizer_slot("W_emb", 0), lambda: engs[0].optimizer_step_count(),
                     lambda: engs[0].set_optimizer_step_count(1),
                     lambda: engs[0].set_optimizer_slot("W_emb", 0, np.zeros((V, d), np.float32))):
            with pytest.raises(native.RgcnError) as err:
                call()
            assert err.value.status == UNSUPPORTED
    finally:
        for t in held:
            for b in t:
                b.free()
        for e in [single] + engs:
            e.close()


@pytest.mark.parametrize("algorithm,steps", [("Adam", 1), ("AdaGrad", 1), ("GradientDescent", 3)])
def test_sharded_steps_rank_by_rank_against_the_mirror(native, algorithm, steps):
    """The world-2 loop of test_sharded_steps_match_the_unsharded_run, max_grad_norm 1, each rank held to the float64 mirror.
    After optimizer_norm_partial a rank's BUF_NORM_EXCHANGE is the squared norm of ITS W_f* / W_b* gradients (k_sum_range
    over k_sqnorm_part's partials) within 17 x 2^-24.  The mirror's global norm counts the replicated tensors once and
    sums the sharded ones over the ranks; each rank's change, on the relations it owns and on every replicated tensor, is
    inside the clipped bounds, and off-owner relations do not change by a bit.  The slots of a sharded context cannot be
    read, so Adam and AdaGrad run the one step whose state is known (zeros, 0.1) and GradientDescent runs three."""
    from relationprediction_amd.sharding import lpt_partition
    V, R, d, nb, L, E, world = 90, 10, 9, 3, 2, 600, 2
    kind, lr = "block", ref.f32(RATES[algorithm])
    params, triples, _, _ = make_case(V, R, d, L, kind, nb, E, seed=21)
    X, Y = decoder_batch(np.random.RandomState(2), triples[:200], V)
    owner = lpt_partition(np.bincount(triples[:, 1], minlength=R), world)
    engs = [native.Engine(V, R, d, L, kind, nb, max_edges=E, rank=r, world=world) for r in range(world)]
    held = []

    def exchange(which):
        total = sum(e.read_buffer(which) for e in engs)
        for e in engs:
            e.write_buffer(which, total)

    try:
        for e in engs:
            e.set_params(params)
            e.decoder_reserve(len(X))
            e.optimizer_config(lr=lr, max_grad_norm=1.0, algorithm=algorithm)
            held.append((e.to_device(X), e.to_device(Y)))
            e.set_relation_owner(owner)
        names = moved_names(engs[0])
        sharded = [n for n in names if n.startswith(("W_f", "W_b"))]
        assert len(sharded) == 2 * L and all(params[n].shape[0] == R for n in sharded)
        for step in range(steps):
            for e in engs:
                e.set_graph(triples)
                e.forward_begin(train=True, seed=100 + step)
            for l in range(1, L + 1):
                for e in engs:
                    e.forward_layer_partial(l)
                exchange(native.BUF_EXCHANGE)
                for e in engs:
                    e.forward_layer_finish(l)
            for e, (Xd, Yd) in zip(engs, held):
                e.decoder_loss_backward_device(Xd, Yd, len(X), 0.01)
                e.backward_begin()
            for l in range(L, 0, -1):
                for e in engs:
                    e.backward_layer_partial(l)
                exchange(native.BUF_EXCHANGE)
                exchange(native.BUF_DSELF_EXCHANGE)
                for e in engs:
                    e.backward_layer_finish(l)
            for e in engs:
                e.backward_end()
            grads = [e.get_grads() for e in engs]
            cur = [e.get_params() for e in engs]
            for e in engs:
                e.optimizer_norm_partial()
            shard_sq = []
            for r, e in enumerate(engs):
                for n in sharded:
                    assert not grads[r][n][owner != r].any(), (r, n)          # a rank holds the gradient of what it owns
                sq = sum(float((grads[r][n].astype(np.float64) ** 2).sum()) for n in sharded)
                got = float(e.read_buffer(native.BUF_NORM_EXCHANGE)[0])
                print("HELD %s clip sharded step %d rank %d shard norm^2 %.6e  err/bound %.3f"
                      % (algorithm, step + 1, r, sq, abs(got - sq) / (ref.SHARD_NORM_RTOL * sq)))
                assert sq > 0 and abs(got - sq) <= ref.SHARD_NORM_RTOL * sq, (r, got, sq)
                shard_sq.append(sq)
            exchange(native.BUF_NORM_EXCHANGE)
            for e in engs:
                e.optimizer_apply()
            for r, e in enumerate(engs):
                new = e.get_params()
                mine = owner == r
                assert mine.any() and not mine.all()
                replicated_sq = sum(float((grads[r][n].astype(np.float64) ** 2).sum()) for n in names if n not in sharded)
                scale = ref.scale_of_norm(float(np.sqrt(replicated_sq + sum(shard_sq))), 1.0)
                pre = None
                if algorithm != "GradientDescent":
                    fill = np.float32(0.1 if algorithm == "AdaGrad" else 0.0)
                    pre = {n: tuple(np.full(params[n].shape, fill, np.float32) for _ in range(2)) for n in names}
                print("rank %d step %d clip scale %.6f" % (r, step + 1, scale))
                assert step > 0 or scale < 0.9                                     # the first step's norm is above the threshold
                hold_step("sharded step %d rank %d" % (step + 1, r), algorithm, names, cur[r], grads[r], pre, new, None, lr,
                          1.0, step_count=step, scale=scale, select={n: mine for n in sharded}, per_tensor_size=False)
                for n in sharded:
                    assert np.array_equal(new[n][~mine], cur[r][n][~mine]), (r, n)
                    assert not np.array_equal(new[n][mine], cur[r][n][mine]), (r, n)
                for n in e.param_names:
                    if n not in names:
                        assert np.array_equal(new[n], cur[r][n]), (r, n)
    finally:
        for t in held:
            for b in t:
                b.free()
        for e in engs:
            e.close()


# ------------------------------------------------------------------ state and resume
@pytest.mark.parametrize("algorithm", ["Adam", "AdaGrad", "GradientDescent"])
def test_state_handed_to_a_fresh_context_continues_bit_for_bit(native, algorithm):
    """A runs five steps.  B runs two, hands its weights and optimizer_state() over and is closed; C, fresh, takes them and
    runs steps three to five: C's weights and slots are A's, bit for bit."""
    c = CASES["basis"]
    data = case_data(c)
    with Run(native, c, algorithm, data=data) as a:
        assert a.eng.optimizer_step_count() == 0
        for s in range(5):
            a.step(seed=40 + s)
            assert a.eng.optimizer_step_count() == s + 1
        want, want_state = a.eng.get_params(), a.eng.optimizer_state()
    with Run(native, c, algorithm, data=data) as b:
        for s in range(2):
            b.step(seed=40 + s)
        weights, state = b.eng.get_params(), b.eng.optimizer_state()
    names = moved_names(a.eng)
    assert state["algorithm"] == algorithm and state["step"] == 2 and want_state["step"] == 5
    assert sorted(state["slots"]) == (sorted(names) if algorithm != "GradientDescent" else [])
    assert all(len(v) == {"Adam": 2, "AdaGrad": 1}[algorithm] for v in state["slots"].values())
    with Run(native, c, algorithm, data=data, set_params=False) as cc:
        cc.eng.set_params(weights)
        cc.eng.set_optimizer_state(state)
        assert cc.eng.optimizer_step_count() == 2
        for s in range(2, 5):
            cc.step(seed=40 + s)
        got, got_state = cc.eng.get_params(), cc.eng.optimizer_state()
    assert got_state["step"] == 5
    for n in want:
        assert np.array_equal(got[n], want[n]), n
    for n in want_state["slots"]:
        for s, (x, y) in enumerate(zip(got_state["slots"][n], want_state["slots"][n])):
            assert np.array_equal(x, y), (n, s)
    if algorithm != "GradientDescent":      # the handed-over state mattered: without it the run ends elsewhere
        with Run(native, c, algorithm, data=data, set_params=False) as fresh:
            fresh.eng.set_params(weights)
            for s in range(2, 5):
                fresh.step(seed=40 + s)
            assert not np.array_equal(fresh.eng.get_param("W_emb"), want["W_emb"])


def test_slots_of_a_fresh_context_and_a_change_of_algorithm(native):
    c = CASES["basis"]
    with Run(native, c, "Adam") as run:
        eng, R = run.eng, c["R"]
        assert eng.optimizer_slot_count() == 2
        for n in moved_names(eng):
            for s in (0, 1):
                slot = eng.get_optimizer_slot(n, s)
                assert slot.shape == eng.get_param(n).shape and not slot.any()
        run.step(seed=1)
        run.step(seed=2)
        assert eng.optimizer_step_count() == 2 and eng.get_optimizer_slot("W_emb", 0).any()
        v = eng.get_optimizer_slot("W_relation", 1)
        assert v[:R].any() and not v[R:].any()
        # the same algorithm again: a new rate, the same state
        eng.optimizer_config(lr=0.02, max_grad_norm=1.0)
        assert eng.optimizer_step_count() == 2 and np.array_equal(eng.get_optimizer_slot("W_relation", 1), v)
        # another one: no state, the count starts over, the slots are the new algorithm's
        eng.optimizer_config(lr=0.1, max_grad_norm=1.0, algorithm="AdaGrad", initial_accumulator=0.25)
        assert eng.optimizer_slot_count() == 1 and eng.optimizer_step_count() == 0
        for n in moved_names(eng):
            assert (eng.get_optimizer_slot(n, 0) == np.float32(0.25)).all()
        run.step(seed=3)
        a = eng.get_optimizer_slot("W_relation", 0)
        assert (a[:R] > np.float32(0.25)).any() and (a[R:] == np.float32(0.25)).all()
        # a written slot comes back; W_relation's rows past RelationCount are ignored and read as the initial value
        a2 = np.random.RandomState(0).rand(*a.shape).astype(np.float32) + 1
        eng.set_optimizer_slot("W_relation", 0, a2)
        back = eng.get_optimizer_slot("W_relation", 0)
        assert np.array_equal(back[:R], a2[:R]) and (back[R:] == np.float32(0.25)).all()
        c1 = np.random.RandomState(1).rand(*eng.get_param("C_f1").shape).astype(np.float32) + 1
        eng.set_optimizer_slot("C_f1", 0, c1)
        assert np.array_equal(eng.get_optimizer_slot("C_f1", 0), c1)
        w = np.random.RandomState(2).rand(*eng.get_param("W_f1").shape).astype(np.float32) + 1     # a private device layout
        eng.set_optimizer_slot("W_f1", 0, w)
        assert np.array_equal(eng.get_optimizer_slot("W_f1", 0), w)
        eng.optimizer_config(lr=0.5, max_grad_norm=1.0, algorithm="GradientDescent")
        assert eng.optimizer_slot_count() == 0 and eng.optimizer_step_count() == 0
        assert eng.optimizer_state() == {"algorithm": "GradientDescent", "step": 0, "slots": {}}
        run.step(seed=4)
        assert eng.optimizer_step_count() == 1


def test_refusals(native):
    c = CASES["basis"]

    def status(call, *a, **kw):
        with pytest.raises(native.RgcnError) as err:
            call(*a, **kw)
        return err.value.status

    eng = engine_of(native, c)
    try:
        zeros = np.zeros(eng.get_param("W_emb").shape, np.float32)
        # before any configuration there is no algorithm whose state one could mean
        assert status(eng.get_optimizer_slot, "W_emb", 0) == STATE
        assert status(eng.optimizer_step_count) == STATE
        # hyper-parameters (csrc/optimizer_check.h; tests/test_optimizers_host.py has the table)
        assert status(eng.optimizer_config, lr=0.0, algorithm="AdaGrad") == INVALID
        assert status(eng.optimizer_config, lr=0.1, algorithm="AdaGrad", initial_accumulator=0.0) == INVALID
        assert status(eng.optimizer_config, lr=0.1, algorithm=3) == INVALID
        assert status(eng.optimizer_config, lr=0.1, algorithm="AdaGrad", struct_size=28) == INVALID
        assert status(eng.optimizer_config, lr=0.1, beta1=1.0) == INVALID
        eng.optimizer_config(lr=0.1, algorithm="AdaGrad", max_grad_norm=1.0)
        # a parameter without a gradient, a slot out of range, a wrong count
        assert status(eng.get_optimizer_slot, "b1", 0) == INVALID
        assert status(eng.set_optimizer_slot, "b1", 0, np.zeros(c["d"], np.float32)) == INVALID
        assert status(eng.get_optimizer_slot, "W_emb", 1) == INVALID
        assert status(eng.get_optimizer_slot, "W_emb", -1) == INVALID
        assert status(eng.set_optimizer_slot, "W_emb", 1, zeros) == INVALID
        assert status(eng.set_optimizer_step_count, -1) == INVALID
        out = np.empty(5, np.float32)
        assert eng.lib.rgcn_get_optimizer_slot(eng.ctx, 0, 0, out.ctypes.data, 5) == INVALID
        assert eng.lib.rgcn_get_optimizer_slot(eng.ctx, len(eng.param_names), 0, out.ctypes.data, 5) == INVALID
        assert "b1" not in eng.optimizer_state()["slots"] and "b2" not in eng.optimizer_state()["slots"]
        # during a capture nothing synchronises, and the algorithm stays
        eng.capture_begin()
        try:
            assert status(eng.get_optimizer_slot, "W_emb", 0) == STATE
            assert status(eng.set_optimizer_slot, "W_emb", 0, zeros) == STATE
            assert status(eng.optimizer_step_count) == STATE
            assert status(eng.set_optimizer_step_count, 3) == STATE
            assert status(eng.optimizer_config, lr=0.1, algorithm="GradientDescent") == STATE
        finally:
            try:
                eng.graph_destroy(eng.capture_end())
            except native.RgcnError:
                pass                               # an empty capture may be refused: the context stays usable
        assert eng.optimizer_step_count() == 0
    finally:
        eng.close()


# ------------------------------------------------------------------ capture
def test_captured_adagrad_step_matches_stepwise_training(native):
    """one ordinary step (it creates the accumulators), then one step captured and replayed twice, against the same three
    steps issued one by one: the same losses, weights, accumulators and step count"""
    c = CASES["basis"]
    data = case_data(c)
    with Run(native, c, "AdaGrad", data=data) as cap, Run(native, c, "AdaGrad", data=data) as plain:
        for run in (cap, plain):
            run.step(seed=5)
        cap.eng.sync()
        cap.eng.capture_begin()
        cap.step(seed=50)
        gid = cap.eng.capture_end()
        for launch in (1, 2):
            cap.eng.graph_launch(gid)
            plain.step(seed=50 + launch)
            assert cap.eng.loss() == plain.eng.loss(), launch
        got, want = cap.eng.get_params(), plain.eng.get_params()
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        a, b = cap.eng.optimizer_state(), plain.eng.optimizer_state()
        assert a["step"] == b["step"] == 3                                   # the device counted the replays
        for n in b["slots"]:
            assert np.array_equal(a["slots"][n][0], b["slots"][n][0]), n
        cap.eng.graph_destroy(gid)


# ------------------------------------------------------------------ the driver
def _drive(tmp_path, text, exp):
    from relationprediction_amd import train
    from test_gpu_driver import write_dataset
    data = str(tmp_path / "data")
    write_dataset(data)
    settings = tmp_path / "run.exp"
    settings.write_text(text)
    np.random.seed(0)
    common = ["--settings", str(settings), "--dataset", data]
    model, iterations = train.main(common + ["--max-iterations", "6", "--save-optimizer-state"])
    assert iterations == 6
    files = sorted(os.listdir(os.path.dirname(exp)))
    base = os.path.basename(exp)
    assert files == sorted([base + "-%d%s" % (n, ext) for n in range(3) for ext in (".npz", ".opt.npz")]), files
    return train, common, model


def _state_file(path):
    with np.load(path) as z:
        return str(z["algorithm"]), int(z["step"]), {k: z[k] for k in z.files if k not in ("algorithm", "step")}


def test_driver_saves_and_resumes_adagrad(tmp_path, capsys):
    """train.main on test_gpu_driver's toy world with Name=AdaGrad, a checkpoint every second iteration: six iterations
    leave three weight files and three state files, the last at step 6; --resume of it numbers on from 3 and its first
    state file stands at 6 + 2 steps; without the flag nothing but the weights is written"""
    from test_gpu_driver import SETTINGS
    exp = str(tmp_path / "models" / "Toy")
    text = (SETTINGS % dict(nb=2, concat="No", exp=exp)).replace("Name=Adam\n\t\tlearning_rate=0.01",
                                                                 "Name=AdaGrad\n\t\tlearning_rate=0.1") \
        .replace("\tReportTrainLossEvery=10", "\tReportTrainLossEvery=10\n\tSaveEveryN=2").replace("CheckEvery=20", "CheckEvery=3")
    assert "Name=AdaGrad" in text and "SaveEveryN=2" in text
    train, common, model = _drive(tmp_path, text, exp)
    algorithm, step, slots = _state_file(exp + "-2.opt.npz")
    assert algorithm == "AdaGrad" and step == 6
    names = model.get_runtime().engine.param_names
    assert sorted(slots) == sorted("%04d_%s_0" % (i, n) for i, n in enumerate(names) if not (n[0] == "b" and n[1:].isdigit()))
    assert all((a >= np.float32(0.1)).all() for a in slots.values()) and any((a > 0.11).any() for a in slots.values())
    assert _state_file(exp + "-0.opt.npz")[1] == 2
    capsys.readouterr()
    model2, iterations = train.main(common + ["--max-iterations", "2", "--save-optimizer-state", "--resume", exp + "-2.npz"])
    out = capsys.readouterr().out
    assert iterations == 2 and "optimizer state of " + exp + "-2.opt.npz, 6 steps taken" in out
    assert os.path.exists(exp + "-3.npz") and not os.path.exists(exp + "-4.npz")
    algorithm, step, slots3 = _state_file(exp + "-3.opt.npz")
    assert algorithm == "AdaGrad" and step == 8
    assert all((slots3[k] >= slots[k]).all() for k in slots) and any((slots3[k] > slots[k]).any() for k in slots)
    # the first run's files are as they were
    assert _state_file(exp + "-2.opt.npz")[1] == 6
    # no flag: weights only; no sibling: said
    os.remove(exp + "-3.opt.npz")
    train.main(common + ["--max-iterations", "2", "--resume", exp + "-3.npz"])
    out = capsys.readouterr().out
    assert "the optimizer starts fresh" in out
    assert os.path.exists(exp + "-4.npz") and not os.path.exists(exp + "-4.opt.npz")


def test_driver_saves_and_resumes_gradient_descent_on_the_embedding_model(tmp_path, capsys):
    """the same for Name=embedding (the DistMult baseline) with GradientDescent: no slots, the step count alone"""
    from test_embedding_host import DISTMULT_EXP
    exp = str(tmp_path / "models" / "Distmult")
    text = (DISTMULT_EXP % 20).replace("models/Distmult", exp).replace("CheckEvery=2000", "CheckEvery=3") \
        .replace("\tReportTrainLossEvery=100", "\tReportTrainLossEvery=100\n\tSaveEveryN=2") \
        .replace("Name=Adam\n\t\tlearning_rate=0.01", "Name=GradientDescent\n\t\tlearning_rate=0.5")
    assert "Name=GradientDescent" in text and "SaveEveryN=2" in text
    train, common, model = _drive(tmp_path, text, exp)
    assert not model.needs_graph()
    assert _state_file(exp + "-2.opt.npz") == ("GradientDescent", 6, {})
    capsys.readouterr()
    train.main(common + ["--max-iterations", "2", "--save-optimizer-state", "--resume", exp + "-2.npz"])
    assert "6 steps taken" in capsys.readouterr().out
    assert _state_file(exp + "-3.opt.npz") == ("GradientDescent", 8, {})
