"""Algorithm.Name = AdaGrad and GradientDescent beside Adam, without a GPU: the optimizer stack and what it hands the model,
the optimizer-state files of Model.save_optimizer / load_optimizer, train.py's --resume helpers, the float64 mirror the GPU
tests measure the kernels by (tests/optimizer_reference.py) against values computed by hand, and the hyper-parameter check of
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
    assert ref.update_bound(np.array([2.0]), np.array([0.5]), clipped=True)[0] == pytest.approx(2.0 ** -22 + 1e-5)


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
