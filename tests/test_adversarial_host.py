"""Self-adversarial negative weights without a GPU: the float64 mirror's invariants (tests/adversarial_reference.py), the
host-and-device softmax text (csrc/adversarial_weights.h) under AddressSanitizer and UndefinedBehaviorSanitizer, the numpy
port and the eager decoder against the mirror, the settings key, the runtime's bookkeeping, and the guard on the inputs
of every GPU case: a case that claims to test weighting has weights on both sides of 1, so a kernel that returned ones
cannot pass it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adversarial_reference as adv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = 0.01
CASES = adv.all_weight_cases()
CASE_IDS = [c["name"] for c in CASES]


# ------------------------------------------------------------------ invariants of the mirror
@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_group_weights_sum_to_K_and_positives_are_one(c):
    w = adv.weights(c["codes"], c["w_rel"], c["X"], c["P"], c["alpha"])
    P, K = c["P"], c["K"]
    assert (w["w"][:P] == 1.0).all()
    groups = w["w"][P:].reshape(K, P)
    np.testing.assert_allclose(groups.sum(axis=0), K, rtol=1e-12)
    assert abs(w["w"].sum() - len(c["X"])) <= 1e-9 * len(c["X"])
    assert (w["w"] >= 0).all() and np.isfinite(w["w"]).all()


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_gpu_case_inputs_spread_the_weights(c):
    """the input guard: energies of unit order, and some weight >= 1.5 and some <= 0.5 wherever weighting is claimed"""
    w = adv.weights(c["codes"], c["w_rel"], c["X"], c["P"], c["alpha"])
    neg = w["w"][c["P"]:]
    print("%s: energies |x| median %.3g max %.3g; weights min %.3g max %.3g; tolerance max %.3g"
          % (c["name"], np.median(np.abs(w["x"])), np.abs(w["x"]).max(), neg.min(), neg.max(), w["tol"].max()))
    assert 1.0 <= c["alpha"] <= 2.0
    if c["spreads"]:
        assert neg.max() >= 1.5 and neg.min() <= 0.5, c["name"]
        assert 0.1 <= np.median(np.abs(w["x"])) <= 10.0
        # the tolerance tells a weight from 1: far below the spread
        assert w["tol"].max() <= 1e-2 * max(1.0, neg.max())
    else:
        assert (neg == 1.0).all()          # K = 1 and negatives identical to their positive: exactly ones


def test_temperature_zero_and_equal_energies_give_ones():
    c = adv.weight_case("dc8")
    x, _ = adv.float64_energies(c["codes"], c["w_rel"], c["X"])
    assert (adv.group_weights(x, c["P"], 0.0) == 1.0).all()
    assert (adv.group_weights(np.full(len(x), 0.37), c["P"], 1.5) == 1.0).all()
    small = adv.group_weights(x, c["P"], 1e-6)
    assert np.abs(small - 1.0).max() < 1e-4          # alpha -> 0 tends to the unweighted loss


def test_shifting_a_groups_energies_changes_nothing():
    c = adv.weight_case("P3")
    x, _ = adv.float64_energies(c["codes"], c["w_rel"], c["X"])
    P, K = c["P"], c["K"]
    shift = np.tile(np.array([5.0, -3.0, 40.0]), K + 1)
    np.testing.assert_allclose(adv.group_weights(x + shift, P, 1.5), adv.group_weights(x, P, 1.5), rtol=1e-12)


def test_dominating_negative_takes_the_whole_group():
    c = adv.dominating_case()
    w = adv.weights(c["codes"], c["w_rel"], c["X"], c["P"], c["alpha"])
    P, K = c["P"], c["K"]
    group = w["w"][P:].reshape(K, P)[:, 1]
    x = w["x"][P:].reshape(K, P)[:, 1]
    assert np.sort(x)[-1] - np.sort(x)[-2] >= 200.0 / c["alpha"]
    assert abs(w["w"][c["big"]] - K) < 1e-9 and np.isfinite(w["w"]).all()
    assert (np.delete(group, 3).astype(np.float32) == 0).all()          # the others underflow in float32


def test_dx_is_the_derivative_of_the_loss_with_the_weights_held_fixed():
    c = adv.weight_case("dc8")
    codes, w_rel = c["codes"].astype(np.float64), c["w_rel"].astype(np.float64)
    out = adv.adversarial_decoder(codes, w_rel, c["X"], c["Y"], c["P"], c["alpha"], REG)
    assert np.abs(out["dx"]).max() > 0
    rng = np.random.RandomState(1)
    h = 1e-6
    for _ in range(10):
        v, k = rng.randint(0, codes.shape[0]), rng.randint(0, codes.shape[1])
        for table, grad in ((0, out["dcodes"]), (1, out["dW"])):
            if table == 1 and v >= adv.R_CASE:
                continue
            lo, hi = [codes.copy(), w_rel.copy()], [codes.copy(), w_rel.copy()]
            lo[table][v, k] -= h
            hi[table][v, k] += h
            f = [adv.weighted_decoder(t[0], t[1], c["X"], c["Y"], out["w"], REG)["loss"] for t in (lo, hi)]
            fd = (f[1] - f[0]) / (2 * h)
            assert abs(fd - grad[v, k]) <= 1e-7 * max(1.0, np.abs(grad).max()) + 1e-9, (table, v, k, fd, grad[v, k])
    # ... and it is NOT the derivative of the loss with the weights following the codes: the mode treats them as constants
    lo, hi = codes.copy(), codes.copy()
    v, k = c["X"][c["P"], 2], 0
    lo[v, k] -= h
    hi[v, k] += h
    f = [adv.adversarial_decoder(t, w_rel, c["X"], c["Y"], c["P"], c["alpha"], REG)["loss"] for t in (lo, hi)]
    assert abs((f[1] - f[0]) / (2 * h) - out["dcodes"][v, k]) > 1e-6


# ------------------------------------------------------------------ the numpy port and the eager decoder
@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_numpy_port_equals_the_mirror(c):
    """float32 energies in, float32 weights out: within the mirror's own tolerance of it"""
    from relationprediction_amd.decoders.bilinear_diag import adversarial_row_weights
    w = adv.weights(c["codes"], c["w_rel"], c["X"], c["P"], c["alpha"])
    x = c["X"]
    e32 = np.sum(c["codes"][x[:, 0]] * c["w_rel"][x[:, 1]] * c["codes"][x[:, 2]], axis=1, dtype=np.float32)
    got = adversarial_row_weights(e32, c["Y"], c["alpha"])
    assert got.dtype == np.float32 and got.shape == (len(x),)
    assert (np.abs(got.astype(np.float64) - w["w"]) <= w["tol"]).all()
    assert (adversarial_row_weights(e32, c["Y"], 0.0) == 1.0).all()


def test_numpy_port_refuses_another_layout():
    from relationprediction_amd.decoders.bilinear_diag import adversarial_row_weights
    x = np.zeros(6, np.float32)
    for y in ([1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0]):
        with pytest.raises(ValueError, match="positives"):
            adversarial_row_weights(x, np.array(y, np.float32), 1.0)


class _Codes(object):
    """what BilinearDiag asks of the component under it"""

    def __init__(self, codes, w_rel):
        self.codes, self.w_rel, self.upstream = codes, w_rel, None

    def get_all_codes(self, mode='train'):
        return self.codes, self.w_rel, self.codes

    def backward(self, upstream):
        self.upstream = upstream
        return upstream


class _Settings(dict):
    def put(self, key, value):
        self[key] = value


def eager(codes, w_rel, R, temperature=None):
    from relationprediction_amd.decoders.bilinear_diag import BilinearDiag
    s = _Settings(EntityCount=len(codes), RelationCount=R, EdgeCount=1, RegularizationParameter=str(REG))
    if temperature is not None:
        s["AdversarialTemperature"] = temperature
    model = BilinearDiag(_Codes(codes, w_rel), s)
    model.local_initialize_train()
    return model


@pytest.mark.parametrize("name", ["dc8", "dc6", "K65", "arbitrary-dc132"])
def test_eager_loss_and_backward_equal_the_mirror(name):
    c = adv.weight_case(name)
    model = eager(c["codes"], c["w_rel"], adv.R_CASE, str(c["alpha"]))
    plain = eager(c["codes"], c["w_rel"], adv.R_CASE)
    for m in (model, plain):
        m.X.feed(c["X"])
        m.Y.feed(c["Y"])
    ref = adv.adversarial_decoder(c["codes"], c["w_rel"], c["X"], c["Y"], c["P"], c["alpha"], REG)
    loss = model.get_loss('train') + model.local_get_regularization()
    assert abs(loss - ref["loss"]) <= 2e-5 * max(1.0, abs(ref["loss"]))
    assert abs(model.get_loss('train') - plain.get_loss('train')) > 1e-3          # the weights matter on this batch
    dcodes, d_rel = model.backward()
    scale = max(np.abs(ref["dcodes"]).max(), np.abs(ref["dW"]).max())
    assert np.abs(dcodes - ref["dcodes"]).max() <= 2e-4 * scale
    assert np.abs(d_rel - ref["dW"]).max() <= 2e-4 * scale


# ------------------------------------------------------------------ the settings key
@pytest.mark.parametrize("value,expected", [(None, 0.0), ("0", 0.0), ("0.5", 0.5), ("2", 2.0), (" 1e-3 ", 1e-3), (1.5, 1.5)])
def test_setting_is_parsed(value, expected):
    from relationprediction_amd import train as train_module
    from relationprediction_amd.decoders.bilinear_diag import parse_adversarial_temperature
    s = _Settings(RegularizationParameter="0.01")
    if value is not None:
        s["AdversarialTemperature"] = value
    assert parse_adversarial_temperature(s) == expected
    assert train_module.adversarial_temperature(s) == expected
    assert eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, value).adversarial_temperature == expected


@pytest.mark.parametrize("value", ["-1", "-0.5", "half", "", "Yes", "nan", "inf", "-inf", True])
def test_a_bad_setting_value_is_refused(value):
    from relationprediction_amd import train as train_module
    from relationprediction_amd.decoders.bilinear_diag import parse_adversarial_temperature
    with pytest.raises(ValueError, match="AdversarialTemperature"):
        parse_adversarial_temperature(_Settings(AdversarialTemperature=value))
    with pytest.raises(ValueError, match="AdversarialTemperature"):
        train_module.adversarial_temperature(_Settings(AdversarialTemperature=value))
    with pytest.raises(ValueError, match="AdversarialTemperature"):
        eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, value)


def test_the_runtime_tells_the_engine_only_what_changed():
    """every driver path goes through EncoderRuntime._adversarial: the setter when (temperature, positives) changed"""
    from relationprediction_amd.runtime import EncoderRuntime

    class Engine(object):
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name,) + a)

    rt = EncoderRuntime.__new__(EncoderRuntime)
    rt.engine = Engine()
    rt._adversarial(300)
    assert rt.engine.calls == []                                        # the key is absent: the engine hears nothing
    rt.set_adversarial_temperature(1.5)
    rt._adversarial(300)
    rt._adversarial(300)
    assert rt.engine.calls == [("set_adversarial_negatives", 1.5, 300)]
    rt._adversarial(200)
    assert rt.engine.calls[1:] == [("set_adversarial_negatives", 1.5, 200)]
    rt.set_adversarial_temperature(0.0)
    rt._adversarial(200)
    rt._adversarial(100)
    assert rt.engine.calls[2:] == [("set_adversarial_negatives", 0.0, 0)]


def test_abi_constants_are_the_headers():
    import re
    from relationprediction_amd import _native
    header = open(os.path.join(ROOT, "include", "rgcn.h")).read()
    assert int(re.search(r"RGCN_BUF_ADVERSARIAL_WEIGHTS = (\d+)", header).group(1)) == _native.BUF_ADVERSARIAL_WEIGHTS == 25
    kernel = open(os.path.join(ROOT, "relationprediction_amd", "csrc", "adversarial.hip")).read()
    assert int(re.search(r"constexpr int kAdvCap = (\d+);", kernel).group(1)) == adv.LDS_CAP
    for name in ("rgcn_decoder_loss_backward_weighted_device", "rgcn_adversarial_weights_device",
                 "rgcn_set_adversarial_negatives"):
        assert name in header and name in _native.exported_symbols()


# ------------------------------------------------------------------ the shared header under the sanitizers
def driver_groups():
    """(name, alpha, energies): K = 1, K = 2,048, equal energies, one energy 200 / alpha above the rest, the extremes of
    float32 without an infinity, and every group of two GPU cases"""
    rng = np.random.RandomState(3)
    big = np.float32(3.0e38)
    groups = [("one", 1.5, np.array([0.7], np.float32)),
              ("k2048", 1.0, rng.randn(2048).astype(np.float32) * 2),
              ("equal", 1.5, np.full(10, -1.25, np.float32)),
              ("dominating", 1.5, np.concatenate([rng.randn(9), [200.0 / 1.5 + 4.0]]).astype(np.float32)),
              ("extremes", 2.0, np.array([big, -big, 0.0, 1e-38, -1e-38, big], np.float32)),
              ("all_lowest", 1.0, np.full(5, -big, np.float32))]
    for name in ("dc8", "K65"):
        c = adv.weight_case(name)
        x, _ = adv.float64_energies(c["codes"], c["w_rel"], c["X"])
        xs = x[c["P"]:].reshape(c["K"], c["P"]).astype(np.float32)
        groups += [("%s_g%d" % (name.lower(), b), c["alpha"], xs[:, b]) for b in range(c["P"])]
    return groups


def test_header_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "adversarial_weights_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "adversarial_weights_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    groups = driver_groups()
    lines = []
    for name, alpha, x in groups:
        lines.append("case %s %d %.9g" % (name, len(x), alpha))
        lines += ["%.9g" % v for v in x.tolist()]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:] + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.split()
    assert run.stdout.splitlines()[-1] == "adversarial_weights_driver: ok"
    pos = 0
    for name, alpha, x in groups:
        K = len(x)
        assert out[pos:pos + 3] == ["case", name, str(K)], (name, out[pos:pos + 3])
        got = np.array([float(v) for v in out[pos + 4:pos + 3 + 2 * K:2]], dtype=np.float32)
        assert out[pos + 3 + 2 * K:pos + 5 + 2 * K] == ["end", name]
        pos += 5 + 2 * K
        want = adv.group_weights(np.concatenate([[0.0], x.astype(np.float64)]), 1, alpha)[1:]
        assert np.isfinite(got).all() and (got >= 0).all(), name
        # the same float64 arithmetic but for the order of the sum: within 2 ulp after the one rounding
        ulp = np.spacing(np.maximum(np.abs(want.astype(np.float32)), np.float32(1e-37))).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= 2 * ulp + 1e-37).all(), name
        assert abs(float(got.astype(np.float64).sum()) - K) <= 1e-5 * K, name
        if name in ("one", "equal", "all_lowest"):
            assert (got == 1.0).all(), name
        if name == "dominating":
            assert got[-1] == K and (got[:-1] == 0).all()
        if name == "extremes":
            assert got[0] == got[5] == 3.0 and not got[1:5].any()
