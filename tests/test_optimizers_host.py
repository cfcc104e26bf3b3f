"""Algorithm.Name = AdaGrad and GradientDescent beside Adam, without a GPU: the optimizer stack and what it hands the model,
the optimizer-state files of Model.save_optimizer / load_optimizer, train.py's --resume helpers, the float64 mirror the GPU
tests measure the kernels by (tests/optimizer_reference.py) against values computed by hand, its error bounds against the
kernels' arithmetic redone in numpy float32, and the hyper-parameter check of
rgcn_optimizer_config_ex (csrc/optimizer_check.h) under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import optimizer_reference as ref
from relationprediction_amd import model as model_module
from relationprediction_amd import train
from relationprediction_amd.common import optimizer_parameter_parser, settings_reader
from relationprediction_amd.optimization import optimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the stack
class ScriptedModel(object):
    def __init__(self):
        self.args, self.kwargs, self.steps = None, None, 0

    def configure_device_optimizer(self, *a, **kw):
        self.args, self.kwargs = a, kw

    def device_train_step(self, graph, x, y, seed):
        self.steps += 1

    def device_loss(self):
        return 1.0

    def save(self, path):
        pass


def optimizer_settings(tmp_path, algorithm):
    p = tmp_path / "s.exp"
    p.write_text("[Optimizer]\n\tMaxGradientNorm=1\n\tMaxIterations=2\n\n\t[Algorithm]\n%s\n\n"
                 "[General]\n\tExperimentName=models/X\n" % "\n".join("\t\t" + line for line in algorithm))
    s = settings_reader.read(str(p))
    s['Optimizer'].merge(s['General'])
    return s['Optimizer']


def built(tmp_path, algorithm):
    opp = optimizer_parameter_parser.Parser(optimizer_settings(tmp_path, algorithm))
    model = ScriptedModel()
    opp.set_save_function(model.save)
    opp.set_sample_transform_function(lambda x: (0, 1, 2))
    opt = optimize.build_hip(model, opp.get_parametrization())
    return model, opt


@pytest.mark.parametrize("name", ["AdaGrad", "GradientDescent"])
def test_the_two_algorithms_build(name):
    stack = optimize.build_stack([(name, {'learning_rate': 0.1})])
    assert type(stack).__name__ == name and stack.learning_rate == 0.1
    assert optimize.COMPONENTS[name] is type(stack)


def test_adagrad_from_the_settings_reaches_the_model(tmp_path):
    model, opt = built(tmp_path, ["Name=AdaGrad", "learning_rate=0.1"])
    assert model.args == (0.1, 0.9, 0.999, 1e-8, 1.0)
    assert model.kwargs == {"algorithm": "AdaGrad", "initial_accumulator": 0.1}
    assert opt.fit([0]) == 2 and model.steps == 2
    model, _ = built(tmp_path, ["Name=AdaGrad", "learning_rate=0.1", "initial_accumulator_value=0.5"])
    assert model.kwargs == {"algorithm": "AdaGrad", "initial_accumulator": 0.5}


def test_gradient_descent_from_the_settings_reaches_the_model(tmp_path):
    model, _ = built(tmp_path, ["Name=GradientDescent", "learning_rate=0.5"])
    assert model.args == (0.5, 0.9, 0.999, 1e-8, 1.0)
    assert model.kwargs == {"algorithm": "GradientDescent"}


def test_adam_still_delivers_five_positional_values_and_no_keyword(tmp_path):
    model, _ = built(tmp_path, ["Name=Adam", "learning_rate=0.01"])
    assert model.args == (0.01, 0.9, 0.999, 1e-8, 1.0) and model.kwargs == {}


def test_refusals_of_the_stack():
    for name in ("AdaGrad", "GradientDescent", "Adam"):
        with pytest.raises(ValueError, match="valid stack"):
            optimize.build_stack([(name, {})])
    with pytest.raises(NotImplementedError):
        optimize.build_stack([('RmsProp', {'learning_rate': 0.1})])
    with pytest.raises(NotImplementedError):
        optimize.build_stack([('Adadelta', {'learning_rate': 0.1})])
    two = optimize.build_stack([('AdaGrad', {'learning_rate': 0.1}), ('GradientDescent', {'learning_rate': 0.1})])
    with pytest.raises(ValueError, match="two Algorithm components.*AdaGrad"):
        optimize.HipOptimizer(two, ScriptedModel())
    with pytest.raises(ValueError, match="no Algorithm"):
        optimize.HipOptimizer(optimize.build_stack([('GradientClipping', {'max_norm': 1.0})]), ScriptedModel())


# ------------------------------------------------------------------ the state files
class FakeEngine(object):
    """optimizer_state / set_optimizer_state of _native.Engine over numpy arrays"""
    param_names = ["W_emb", "b_emb", "W_f1", "b1", "W_relation"]       # b1: no gradient, no state

    def __init__(self, algorithm, seed=None):
        self.algorithm, self.step, self.slots = algorithm, 0, {}
        if seed is not None:
            rng = np.random.RandomState(seed)
            count = {"Adam": 2, "AdaGrad": 1, "GradientDescent": 0}[algorithm]
            self.step = 6000
            for n in self.param_names:
                if n != "b1" and count:
                    self.slots[n] = [rng.rand(3, 4).astype(np.float32) for _ in range(count)]

    def optimizer_algorithm(self):
        return self.algorithm

    def optimizer_state(self):
        return {"algorithm": self.algorithm, "step": self.step, "slots": self.slots}

    def set_optimizer_state(self, state):
        assert state["algorithm"] == self.algorithm
        self.step, self.slots = state["step"], state["slots"]


class EngineModel(model_module.Model):
    def __init__(self, engine):
        self.engine = engine

    def device_optimizer_engine(self):
        return self.engine


@pytest.mark.parametrize("algorithm", ["Adam", "AdaGrad", "GradientDescent"])
def test_optimizer_state_file_round_trip(tmp_path, algorithm):
    src = FakeEngine(algorithm, seed=3)
    path = str(tmp_path / "models" / "X-4.opt.npz")
    EngineModel(src).save_optimizer(path)
    assert os.listdir(str(tmp_path / "models")) == ["X-4.opt.npz"]          # that name, nothing appended to it
    with np.load(path) as z:
        assert str(z["algorithm"]) == algorithm and int(z["step"]) == 6000
        keys = sorted(k for k in z.files if k not in ("algorithm", "step"))
    want = {"Adam": ["0000_W_emb_0", "0000_W_emb_1", "0001_b_emb_0", "0001_b_emb_1", "0002_W_f1_0", "0002_W_f1_1",
                     "0004_W_relation_0", "0004_W_relation_1"],
            "AdaGrad": ["0000_W_emb_0", "0001_b_emb_0", "0002_W_f1_0", "0004_W_relation_0"], "GradientDescent": []}
    assert keys == want[algorithm]
    dst = FakeEngine(algorithm)
    assert EngineModel(dst).load_optimizer(path) == 6000
    assert dst.step == 6000 and sorted(dst.slots) == sorted(src.slots)
    for n in src.slots:
        assert len(dst.slots[n]) == len(src.slots[n])
        for a, b in zip(dst.slots[n], src.slots[n]):
            np.testing.assert_array_equal(a, b)


def test_optimizer_state_of_another_algorithm_is_refused(tmp_path):
    path = str(tmp_path / "X-0.opt.npz")
    EngineModel(FakeEngine("AdaGrad", seed=1)).save_optimizer(path)
    dst = FakeEngine("Adam")
    with pytest.raises(ValueError, match="AdaGrad.*Adam"):
        EngineModel(dst).load_optimizer(path)
    assert dst.step == 0 and dst.slots == {}


# ------------------------------------------------------------------ --resume
class StubModel(object):
    def __init__(self, engine):
        self.save_iter, self.loaded, self.written, self.engine = 0, [], [], engine

    def load(self, path):
        self.loaded.append(path)

    def save(self, path):
        self.written.append("%s-%d.npz" % (path, self.save_iter))
        self.save_iter += 1

    def save_optimizer(self, path):
        self.written.append(path)
        EngineModel(self.engine).save_optimizer(path)

    def load_optimizer(self, path):
        return EngineModel(self.engine).load_optimizer(path)


def test_resume_continues_the_checkpoint_numbering(tmp_path, capsys):
    base = str(tmp_path / "models" / "GcnBlock")
    first = StubModel(FakeEngine("AdaGrad", seed=5))
    save = train.save_with_optimizer_state(first)
    for _ in range(3):
        save(base)
    assert first.written == [base + "-0.npz", base + "-0.opt.npz", base + "-1.npz", base + "-1.opt.npz",
                             base + "-2.npz", base + "-2.opt.npz"]
    assert train.optimizer_state_path(base + "-2.npz") == base + "-2.opt.npz"
    # the next process: weights after initialize_model, state after the optimizer is configured
    second = StubModel(FakeEngine("AdaGrad"))
    train.resume_weights(second, base + "-2.npz")
    assert second.loaded == [base + "-2.npz"] and second.save_iter == 3
    assert train.resume_optimizer(second, base + "-2.npz") == 6000
    assert second.engine.step == 6000 and sorted(second.engine.slots) == sorted(first.engine.slots)
    train.save_with_optimizer_state(second)(base)
    assert second.written == [base + "-3.npz", base + "-3.opt.npz"]          # nothing of the first run is overwritten
    # a checkpoint without a sibling: said, and the optimizer is left as configured
    third = StubModel(FakeEngine("AdaGrad"))
    train.resume_weights(third, base + "-7.npz")
    assert third.save_iter == 8
    capsys.readouterr()
    assert train.resume_optimizer(third, base + "-7.npz") is None
    assert "starts fresh" in capsys.readouterr().out and third.engine.step == 0


def test_the_command_line_has_the_two_flags(capsys):
    with pytest.raises(SystemExit):
        train.main(["--help"])
    out = capsys.readouterr().out
    assert "--save-optimizer-state" in out and "--resume" in out


# ------------------------------------------------------------------ the float64 mirror, by hand
W = {"w": np.array([1.0, -2.0, 0.5])}
G = {"w": np.array([3.0, 0.0, -4.0])}           # norm 5; an element without a gradient


def test_mirror_gradient_descent_by_hand():
    d, acc = ref.step("GradientDescent", W, G, None, ["w"], lr=0.5)
    assert acc is None
    np.testing.assert_allclose(d["w"], [-1.5, 0.0, 2.0], rtol=1e-15, atol=0)
    d, _ = ref.step("GradientDescent", W, G, None, ["w"], lr=0.5, max_norm=1.0)           # scale 1/5
    np.testing.assert_allclose(d["w"], [-0.3, 0.0, 0.4], rtol=1e-15, atol=0)
    d, _ = ref.step("GradientDescent", W, G, None, ["w"], lr=0.5, max_norm=10.0)          # inside the ball: untouched
    np.testing.assert_allclose(d["w"], [-1.5, 0.0, 2.0], rtol=1e-15, atol=0)


def test_mirror_adagrad_by_hand():
    a0 = {"w": np.full(3, 0.1)}
    d, acc = ref.step("AdaGrad", W, G, a0, ["w"], lr=0.1)
    np.testing.assert_allclose(acc["w"], [9.1, 0.1, 16.1], rtol=1e-15)
    np.testing.assert_allclose(d["w"], [-0.3 / np.sqrt(9.1), 0.0, 0.4 / np.sqrt(16.1)], rtol=1e-15, atol=0)
    assert a0["w"].tolist() == [0.1, 0.1, 0.1]                                       # inputs are left alone
    # second step from that state
    d2, acc2 = ref.step("AdaGrad", W, {"w": np.array([1.0, 2.0, 0.0])}, acc, ["w"], lr=0.1)
    np.testing.assert_allclose(acc2["w"], [10.1, 4.1, 16.1], rtol=1e-15)
    np.testing.assert_allclose(d2["w"], [-0.1 / np.sqrt(10.1), -0.2 / np.sqrt(4.1), 0.0], rtol=1e-15, atol=0)
    # clipped: g = (0.6, 0, -0.8)
    d, acc = ref.step("AdaGrad", W, G, a0, ["w"], lr=0.1, max_norm=1.0)
    np.testing.assert_allclose(acc["w"], [0.46, 0.1, 0.74], rtol=1e-14)
    np.testing.assert_allclose(d["w"], [-0.06 / np.sqrt(0.46), 0.0, 0.08 / np.sqrt(0.74)], rtol=1e-14, atol=0)
    # the zero accumulator the fill exists to avoid
    with np.errstate(invalid="ignore", divide="ignore"):
        d, _ = ref.step("AdaGrad", W, G, {"w": np.zeros(3)}, ["w"], lr=0.1)
    assert np.isnan(d["w"][1]) and d["w"][0] == pytest.approx(-0.1)


def test_mirror_norm_runs_over_all_named_tensors():
    grads = {"a": np.array([3.0]), "b": np.array([[4.0]]), "unused": np.array([100.0])}
    assert ref.global_norm(grads, ["a", "b"]) == 5.0
    assert ref.clip_scale(grads, ["a", "b"], 1.0) == pytest.approx(0.2) and ref.clip_scale(grads, ["a", "b"], 0.0) == 1.0
    b = ref.update_bound(np.array([2.0]), np.array([0.5]), clipped=False)
    assert b[0] == pytest.approx(2.0 ** -23 * 2 + 8 * 2.0 ** -23 * 0.5)
    # clipped: the scale's own error, 5 x 2^-23 (sixteen roundings under a square root, one to float, one divide), on top
    assert ref.SCALE_RTOL == 5 * 2.0 ** -23
    b = ref.update_bound(np.array([2.0]), np.array([0.5]), clipped=True)
    assert b[0] == pytest.approx(2.0 ** -22 + 13 * 2.0 ** -23 * 0.5, rel=1e-12)
    assert ref.accumulator_rtol(False) == 8 * 2.0 ** -23 and ref.accumulator_rtol(True) == 28 * 2.0 ** -24
    three, u = np.array([3.0]), 2.0 ** -24
    assert ref.adam_m_bound(three, False)[0] == 12 * u and ref.adam_m_bound(three, True)[0] == 48 * u
    assert ref.adam_v_bound(three, False)[0] == 12 * u and ref.adam_v_bound(three, True)[0] == 84 * u


ZEROS = {"w": (np.zeros(1), np.zeros(1))}


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clip-1"])
def test_mirror_adam_by_hand_with_the_defaults(clipped):
    """one element, two steps, lr 0.01, b1 0.9, b2 0.999, eps 1e-8; gradients 2 and -1, or under max_norm 1 (a norm of 2 and
    of 4: scales 1/2 and 1/4) twice those, which the clip turns into the same two"""
    k = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0 if clipped else 0.0)
    g1, g2 = ({"w": np.array([2.0])}, {"w": np.array([-4.0])}) if clipped else ({"w": np.array([1.0])}, {"w": np.array([-1.0])})
    w = {"w": np.array([0.25])}
    d, s = ref.step("Adam", w, g1, ZEROS, ["w"], step_count=0, **k)                 # g' = 1
    s = s["w"]
    np.testing.assert_allclose([s.m[0], s.A[0], s.v[0]], [0.1, 0.1, 0.001], rtol=1e-15)
    rate1 = 0.01 * np.sqrt(0.001) / 0.1
    np.testing.assert_allclose(d["w"], [-rate1 * 0.1 / (np.sqrt(0.001) + 1e-8)], rtol=1e-15)
    np.testing.assert_allclose(d["w"], [-0.01 / (1 + 1e-8 / np.sqrt(0.001))], rtol=1e-14)     # lr, but for eps
    np.testing.assert_allclose(s.U, -d["w"], rtol=1e-15)
    d2, s2 = ref.step("Adam", w, g2, {"w": (s.m, s.v)}, ["w"], step_count=1, **k)       # g' = -1
    s2 = s2["w"]
    np.testing.assert_allclose([s2.m[0], s2.A[0], s2.v[0]], [-0.01, 0.19, 0.001999], rtol=1e-14)
    rate2 = 0.01 * np.sqrt(1 - 0.998001) / 0.19
    np.testing.assert_allclose(d2["w"], [rate2 * 0.01 / (np.sqrt(0.001999) + 1e-8)], rtol=1e-13)
    np.testing.assert_allclose(s2.U, [rate2 * 0.19 / (np.sqrt(0.001999) + 1e-8)], rtol=1e-13)
    assert ZEROS["w"][0][0] == 0 and s.m[0] == pytest.approx(0.1)                   # inputs are left alone
    # the three wrong Adams are other numbers
    for variant, want in (("rate_uncorrected", -0.01 * 0.1 / (np.sqrt(0.001) + 1e-8)),
                          ("step_late", -rate2 * 0.1 / (np.sqrt(0.001) + 1e-8)),
                          ("eps_under_root", -rate1 * 0.1 / np.sqrt(0.001 + 1e-8))):
        wrong, _ = ref.step("Adam", w, g1, ZEROS, ["w"], step_count=0, variant=variant, **k)
        np.testing.assert_allclose(wrong["w"], [want], rtol=1e-14)


def test_mirror_adam_by_hand_with_other_hyper_parameters():
    """b1 0.5, b2 0.9, eps 1e-3, lr 0.003; gradients 2 and -2: on the second step m cancels to nothing, A and U do not"""
    k = dict(lr=0.003, beta1=0.5, beta2=0.9, eps=1e-3)
    w = {"w": np.array([0.25])}
    d, s = ref.step("Adam", w, {"w": np.array([2.0])}, ZEROS, ["w"], step_count=0, **k)
    s = s["w"]
    np.testing.assert_allclose([s.m[0], s.A[0], s.v[0]], [1.0, 1.0, 0.4], rtol=1e-15)
    rate1 = 0.003 * np.sqrt(0.1) / 0.5
    np.testing.assert_allclose(d["w"], [-rate1 / (np.sqrt(0.4) + 1e-3)], rtol=1e-14)
    d2, s2 = ref.step("Adam", w, {"w": np.array([-1.0])}, {"w": (s.m, s.v)}, ["w"], step_count=1, **k)
    s2 = s2["w"]
    assert s2.m[0] == 0.0 and d2["w"][0] == 0.0
    np.testing.assert_allclose([s2.A[0], s2.v[0]], [1.0, 0.46], rtol=1e-14)
    rate2 = 0.003 * np.sqrt(0.19) / 0.75
    np.testing.assert_allclose(s2.U, [rate2 / (np.sqrt(0.46) + 1e-3)], rtol=1e-14)
    # the hyper-parameters as the ABI receives them: float32, and 1 - b exact
    assert ref.f32(0.999) == 0.9990000128746033 and 1.0 - ref.f32(0.999) == float(np.float32(1) - np.float32(0.999))
    assert ref.adam_rate(0.01, 0.9, 0.999, 2 ** 24 - 1) == 0.01


# ------------------------------------------------------------------ the bounds against the kernels' arithmetic in numpy float32
HYPER = dict(lr=ref.f32(0.01), beta1=ref.f32(0.9), beta2=ref.f32(0.999), eps=ref.f32(1e-8))


def excess(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["unclipped", "clip-1"])
@pytest.mark.parametrize("n", [15, 2047, 4097])
def test_fp32_emulation_stays_inside_the_bounds_and_wrong_mirrors_do_not(n, max_norm):
    """ref.emulated_adam / emulated_clip_scale do in numpy float32 what k_sqnorm_part, k_clip_scale and k_adam do, operation
    by operation, on the inputs the GPU test injects (ref.injected_case), three steps.  Mirrored in float64 from the
    emulation's own pre-step values, every element of the change, of m and of v is inside the bounds, so the bounds are
    not too tight for correct fp32 arithmetic; each of the three wrong Adams, and with the clip on the unclipped mirror from
    step 2 (wherever the step's norm is above the threshold: there is nothing to miss otherwise), is outside the change's
    bound by 100 times or more on some element, so they are not too wide to tell.  The weights start every step as they
    were: half of them stay exactly 0, where the bound is the update's alone."""
    clipped = max_norm > 0
    w, grads = ref.injected_case(n, seed=n, steps=3)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = {"d": 0.0, "m": 0.0, "v": 0.0, "d0": 0.0}
    told_unclipped = 0
    for t0, g in enumerate(grads):
        scale = ref.emulated_clip_scale([g], max_norm)
        assert abs(float(scale) - ref.clip_scale({"w": g}, ["w"], max_norm)) <= ref.SCALE_RTOL * float(scale)
        w1, m1, v1 = ref.emulated_adam(w, g, m, v, step_count=t0, scale=scale, **HYPER)
        a = ({"w": w}, {"w": g}, {"w": (m, v)}, ["w"])
        d, s = ref.step("Adam", *a, max_norm=max_norm, step_count=t0, **HYPER)
        s = s["w"]
        got = w1.astype(np.float64) - w
        bound = ref.update_bound(w, s.U, clipped)
        worst["d"] = max(worst["d"], excess(np.abs(got - d["w"]), bound))
        worst["d0"] = max(worst["d0"], excess(np.abs(got - d["w"])[w == 0], bound[w == 0]))
        worst["m"] = max(worst["m"], excess(np.abs(m1 - s.m), ref.adam_m_bound(s.A, clipped)))
        worst["v"] = max(worst["v"], excess(np.abs(v1 - s.v), ref.adam_v_bound(s.v, clipped)))
        assert (np.abs(got - d["w"]) <= bound).all() and (np.abs(m1 - s.m) <= ref.adam_m_bound(s.A, clipped)).all()
        assert (np.abs(v1 - s.v) <= ref.adam_v_bound(s.v, clipped)).all()
        assert float(np.abs(d["w"]).max()) >= 100 * float(bound.max())
        for variant in ref.ADAM_VARIANTS:
            wrong, _ = ref.step("Adam", *a, max_norm=max_norm, step_count=t0, variant=variant, **HYPER)
            assert excess(np.abs(got - wrong["w"]), bound) >= 100, (t0, variant)
        if clipped and t0 >= 1 and float(scale) < 0.99:     # (15 elements of step 2 can have a norm below 1: no clip to miss)
            wrong, _ = ref.step("Adam", *a, max_norm=0.0, step_count=t0, **HYPER)
            assert excess(np.abs(got - wrong["w"]), bound) >= 100, t0
            told_unclipped += 1
        m, v = m1, v1                            # (the weights start every step as they were: half of them stay 0)
    assert told_unclipped >= (1 if n == 15 else 2) or not clipped
    print("n %d max_norm %g: max err / bound  change %.3f (zero weights %.3f)  m %.3f  v %.3f"
          % (n, max_norm, worst["d"], worst["d0"], worst["m"], worst["v"]))


def test_injected_case_is_what_its_docstring_says():
    n = 4097
    w, grads = ref.injected_case(n, seed=1, steps=3)
    assert (w == 0).sum() == n // 2 and len(grads) == 3 and all(g.dtype == np.float32 for g in grads)
    tenth = n // 10
    for s, g in enumerate(grads):
        top = 1e3 * (1e-3 if s == 1 else 1.0)
        nz = np.abs(g[g != 0]).astype(np.float64)
        assert 0.07 <= (g == 0).mean() <= 0.13 and nz.min() >= 0.99e-12 * top / 1e3 and nz.max() <= 1.01 * top
        first = np.abs(g[:tenth][g[:tenth] != 0]).astype(np.float64) * (1e3 / top)
        assert first.min() >= 0.99e-9 and first.max() <= 1.01e-7
    second = slice(tenth, 2 * tenth)
    both = (grads[0][second] != 0) & (grads[1][second] != 0) & (grads[2][second] != 0)
    assert both.sum() > tenth // 2
    assert (np.sign(grads[0][second][both]) == np.sign(grads[2][second][both])).all()
    assert (np.sign(grads[0][second][both]) == -np.sign(grads[1][second][both])).all()
    # the tail weighs in the norm
    assert all(np.abs(g[-3:]).min() >= 99.0 * (1e-3 if s == 1 else 1.0) for s, g in enumerate(grads))
    stay = (grads[0] == 0) & (grads[1] == 0) & (grads[2] == 0)
    assert stay.sum() >= n // 40                                                    # state that stays zero


# ------------------------------------------------------------------ csrc/optimizer_check.h under ASan + UBSan
OK, BAD = "0|", "1|bad optimizer hyper-parameters"
STRUCT = "1|rgcn_optimizer_params::struct_size is not sizeof(rgcn_optimizer_params)"
ALGORITHM = "1|unknown optimizer algorithm (0: Adam, 1: GradientDescent, 2: AdaGrad)"
ACCUMULATOR = "1|AdaGrad's initial_accumulator must be positive (a zero accumulator under a zero gradient is 0 / 0)"

EXPECTED = {
    "ok_adam": OK, "ok_gradient_descent": OK, "ok_adagrad": OK, "ok_no_clip": OK, "ok_beta1_0": OK,
    "null": "1|rgcn_optimizer_config_ex: NULL parameters",
    "struct_size_short": STRUCT, "struct_size_long": STRUCT, "struct_size_0": STRUCT,
    "algorithm_3": ALGORITHM, "algorithm_negative": ALGORITHM,
    "adam_rate_0": BAD, "adam_rate_negative": BAD, "adam_rate_nan": BAD, "adam_clip_negative": BAD,
    "gradient_descent_rate_0": BAD, "gradient_descent_rate_negative": BAD, "gradient_descent_rate_nan": BAD,
    "gradient_descent_clip_negative": BAD,
    "adagrad_rate_0": BAD, "adagrad_rate_negative": BAD, "adagrad_rate_nan": BAD, "adagrad_clip_negative": BAD,
    "adam_beta1_1": BAD, "adam_beta1_negative": BAD, "adam_beta2_1": BAD, "adam_epsilon_0": BAD,
    "gradient_descent_ignores_beta1": OK, "adagrad_ignores_epsilon": OK,
    "adagrad_accumulator_0": ACCUMULATOR, "adagrad_accumulator_negative": ACCUMULATOR, "adagrad_accumulator_nan": ACCUMULATOR,
    "adam_ignores_accumulator": OK, "gradient_descent_ignores_accumulator": OK,
    "both_algorithm_and_rate": ALGORITHM, "both_rate_and_accumulator": BAD,
}


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("optimizer_check") / "optimizer_check_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "optimizer_check_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "optimizer_check_driver: ok"
    got = dict(line.split(": ", 1) for line in lines[:-1])
    assert len(got) == len(lines) - 1, "a case name printed twice"
    return got


def test_optimizer_check_table_under_asan_and_ubsan(verdicts):
    wrong = {k: (verdicts.get(k), v) for k, v in EXPECTED.items() if verdicts.get(k) != v}
    assert not wrong, "\n".join("%s:\n  got      %s\n  expected %s" % (k, g, e) for k, (g, e) in wrong.items())
    assert set(verdicts) == set(EXPECTED), sorted(set(verdicts) ^ set(EXPECTED))
