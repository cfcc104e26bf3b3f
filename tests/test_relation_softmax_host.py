"""The relation-softmax loss term without a GPU: the float64 mirror (tests/relation_softmax_reference.py) against finite
differences of its own loss and against its own special cases, the eager numpy surface of BilinearDiag against the mirror,
the [Decoder] RelationSoftmaxWeight key, the host plan function's table (csrc/relation_softmax_plan.h) and its sanitizer
driver (tests/sanitize/relation_softmax_plan_driver.cpp, built with g++ under ASan + UBSan and run as a program)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import relation_softmax_reference as rsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (V, R, dc, P, seed, masked)
CASES = {"small": (30, 5, 4, 12, 1, False), "two_relations": (20, 2, 3, 9, 2, False), "wide": (40, 67, 6, 20, 3, False),
         "masked": (30, 6, 4, 16, 4, True), "self_pairs": (25, 7, 5, 10, 5, False)}


def case(name):
    V, R, dc, P, seed, masked = CASES[name]
    codes, w_rel, pos = rsr.make_case(V, R, dc, P, seed, self_pairs=3 if name == "self_pairs" else 0)
    known = None
    if masked:
        rng = np.random.RandomState(seed)
        extra = np.stack([pos[::2, 0], rng.randint(0, R, len(pos[::2])), pos[::2, 2]], 1)
        known = np.concatenate([pos, extra]).astype(np.int32)
    return codes, w_rel, pos, R, known


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_case_compares_zeros(name):
    codes, w_rel, pos, R, known = case(name)
    t = rsr.term(codes, w_rel, pos, R, 0.7, known=known)
    assert abs(t["loss"]) > 1e-3 and np.abs(t["G"]).max() > 0 and np.abs(t["dW"]).max() > 0 and np.abs(t["dcodes"]).max() > 0
    if known is not None:
        assert (~t["mask"]).sum() > 0 and not t["G"][~t["mask"]].any()
    np.testing.assert_allclose(t["G"].sum(axis=1), 0, atol=1e-15)      # softmax minus one-hot


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_agree_with_central_differences(name):
    codes, w_rel, pos, R, known = case(name)
    c64, w64 = codes.astype(np.float64), w_rel.astype(np.float64)
    t = rsr.term(c64, w64, pos, R, 0.7, known=known, exact_query=True)
    h = 1e-6
    rng = np.random.RandomState(0)
    for which, arr, grad in (("codes", c64, t["dcodes"]), ("W_relation", w64, np.vstack([t["dW"], np.zeros((len(w64) - R, w64.shape[1]))]))):
        touched = np.argwhere(grad != 0)
        picks = touched[rng.choice(len(touched), size=min(25, len(touched)), replace=False)]
        for i, j in picks:
            up, down = arr.copy(), arr.copy()
            up[i, j] += h
            down[i, j] -= h
            args = (lambda a: (a, w64)) if which == "codes" else (lambda a: (c64, a))
            fd = (rsr.term(*args(up), pos, R, 0.7, known=known, exact_query=True)["loss"]
                  - rsr.term(*args(down), pos, R, 0.7, known=known, exact_query=True)["loss"]) / (2 * h)
            assert abs(fd - grad[i, j]) <= 1e-7 * max(1.0, abs(grad[i, j])), (which, i, j, fd, grad[i, j])
    assert not np.vstack([t["dW"]])[R:].any()


def test_masked_equals_plain_when_no_other_relation_is_known():
    codes, w_rel, pos, R, _ = case("small")
    _, first = np.unique(pos[:, [0, 2]], axis=0, return_index=True)    # no pair with two relations
    pos = pos[np.sort(first)]
    assert len(pos) >= 8
    plain = rsr.term(codes, w_rel, pos, R, 0.7)
    masked = rsr.term(codes, w_rel, pos, R, 0.7, known=pos)            # K holds the positives themselves only
    assert masked["loss"] == plain["loss"]
    for k in ("G", "dW", "dcodes"):
        np.testing.assert_array_equal(masked[k], plain[k])


def test_a_pair_that_knows_every_relation_contributes_exactly_zero():
    codes, w_rel, pos, R, _ = case("small")
    _, first = np.unique(pos[:, [0, 2]], axis=0, return_index=True)    # the saturated pair occurs once
    pos = pos[np.sort(first)]
    full = np.concatenate([pos] + [np.array([[pos[0, 0], r, pos[0, 2]]]) for r in range(R)]).astype(np.int32)
    t = rsr.term(codes, w_rel, pos, R, 0.7, known=full)
    assert t["ell"][0] == 0 and not t["G"][0].any() and np.abs(t["ell"][1:]).min() > 0


def test_weight_zero_is_the_decoder_loss():
    codes, w_rel, pos, R, _ = case("small")
    t = rsr.term(codes, w_rel, pos, R, 0.0)
    assert t["loss"] == 0 and not t["G"].any() and not t["dW"].any() and not t["dcodes"].any()
    # ... and through the eager surface: the loss and gradients with the key at 0 are those without the key, bit for bit
    X = np.concatenate([pos, pos[:, [2, 1, 0]]]).astype(np.int32)
    Y = np.concatenate([np.ones(len(pos)), np.zeros(len(pos))]).astype(np.float32)
    seen = []
    for weight in (None, "0"):
        model = eager(codes, w_rel, R, weight)
        model.X.feed(X)
        model.Y.feed(Y)
        seen.append((model.get_loss('train'), model.backward()))
    dloss = rsr.decoder(codes, w_rel, X, Y, 0.0)[0]
    assert seen[0][0] == seen[1][0] and abs(seen[1][0] - dloss) <= 1e-6 * max(1.0, abs(dloss))
    for a, b in zip(seen[0][1], seen[1][1]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ the eager numpy surface
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


def eager(codes, w_rel, R, weight=None):
    from relationprediction_amd.decoders.bilinear_diag import BilinearDiag
    s = _Settings(EntityCount=len(codes), RelationCount=R, EdgeCount=1, RegularizationParameter="0.01")
    if weight is not None:
        s["RelationSoftmaxWeight"] = weight
    model = BilinearDiag(_Codes(codes, w_rel), s)
    model.local_initialize_train()
    return model


def test_eager_loss_and_backward_equal_the_mirror():
    codes, w_rel, pos, R, _ = case("wide")
    rng = np.random.RandomState(9)
    neg = pos.copy()
    neg[:, 0] = rng.randint(0, len(codes), len(pos))
    X = np.concatenate([pos[:5], neg, pos[5:]]).astype(np.int32)       # the positives are where the labels say, not in front
    Y = np.concatenate([np.ones(5), np.zeros(len(neg)), np.ones(len(pos) - 5)]).astype(np.float32)
    out = {}
    for weight in (None, "0.6"):
        model = eager(codes, w_rel, R, weight)
        model.X.feed(X)
        model.Y.feed(Y)
        out[weight] = (model.get_loss('train'), model.backward())
    t = rsr.term(codes, w_rel, pos, R, 0.6)
    assert abs(t["loss"]) > 1e-3
    assert abs(out["0.6"][0] - out[None][0] - t["loss"]) <= 1e-12 * max(1.0, abs(t["loss"]))
    dcodes = out["0.6"][1][0].astype(np.float64) - out[None][1][0].astype(np.float64)
    d_rel = out["0.6"][1][1].astype(np.float64) - out[None][1][1].astype(np.float64)
    # (the eager surface returns float32: the difference of two float32 sums against the float64 mirror)
    scale = max(np.abs(out[None][1][0]).max(), np.abs(out[None][1][1]).max(), np.abs(t["dcodes"]).max(), np.abs(t["dW"]).max())
    assert np.abs(dcodes - t["dcodes"]).max() <= 4 * 2.0 ** -24 * scale
    assert np.abs(d_rel[:R] - t["dW"]).max() <= 4 * 2.0 ** -24 * scale and not d_rel[R:].any()


# ------------------------------------------------------------------ the settings key
@pytest.mark.parametrize("value,expected", [(None, 0.0), ("0", 0.0), ("0.5", 0.5), ("2", 2.0), (" 1e-3 ", 1e-3), (0.25, 0.25)])
def test_setting_is_parsed(value, expected):
    from relationprediction_amd.decoders.bilinear_diag import parse_relation_softmax_weight
    s = _Settings(RegularizationParameter="0.01")
    if value is not None:
        s["RelationSoftmaxWeight"] = value
    assert parse_relation_softmax_weight(s) == expected
    assert eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, value).relation_softmax_weight == expected


@pytest.mark.parametrize("value", ["-1", "-0.5", "half", "", "Yes", "nan", "inf", True])
def test_a_bad_setting_value_is_refused(value):
    from relationprediction_amd.decoders.bilinear_diag import parse_relation_softmax_weight
    with pytest.raises(ValueError, match="RelationSoftmaxWeight"):
        parse_relation_softmax_weight(_Settings(RelationSoftmaxWeight=value))
    with pytest.raises(ValueError, match="RelationSoftmaxWeight"):
        eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, value)


def test_one_relation_is_refused_at_start_up():
    from relationprediction_amd import train as train_module
    with pytest.raises(ValueError, match="two relations"):
        train_module.relation_softmax_weight(_Settings(RelationSoftmaxWeight="0.5"), 1)
    assert train_module.relation_softmax_weight(_Settings(RelationSoftmaxWeight="0"), 1) == 0.0      # off asks nothing
    assert train_module.relation_softmax_weight(_Settings(), 1) == 0.0
    assert train_module.relation_softmax_weight(_Settings(RelationSoftmaxWeight="0.5"), 2) == 0.5


def test_the_runtime_tells_the_engine_only_what_changed():
    """all four driver paths go through EncoderRuntime._relation_softmax: reserve when the positives outgrow it, the
    setter when (weight, positives, mask) changed, the index only when none is resident"""
    from relationprediction_amd.runtime import EncoderRuntime

    class Engine(object):
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name,) + tuple(x if np.isscalar(x) else "array" for x in a))

    rt = EncoderRuntime.__new__(EncoderRuntime)
    rt.engine = Engine()
    rt._relation_softmax(300)
    assert rt.engine.calls == []                                        # the key is absent: the engine hears nothing
    rt.set_relation_softmax(0.5)
    rt._relation_softmax(300)
    rt._relation_softmax(300)
    assert rt.engine.calls == [("relation_softmax_reserve", 300), ("set_relation_softmax", 0.5, 300, False)]
    rt.set_relation_softmax(0.5, known=np.zeros((2, 3), np.int32))
    rt._relation_softmax(200)
    assert rt.engine.calls[2:] == [("known_positives_reserve", "array"), ("set_relation_softmax", 0.5, 200, True)]
    rt.set_relation_softmax(0.0)
    rt._relation_softmax(200)
    assert rt.engine.calls[4:] == [("set_relation_softmax", 0.0, 0, False)]


# ------------------------------------------------------------------ the host plan
PLAN = {
    # what a context runs (the term's own slabs, 2^23 floats).  2 x 4 tiles of the [240, 500] product -> 256 / 8 = 32
    # slices, 937 rows deep each; 69 slabs of 120,000 floats would fit
    "fb237_minibatch": "chunk=30000 padded_r=240 split=32",
    # 2^24 floats of energies / 240 columns = 69,905 rows -> 69,888 in whole tiles, cut at 65,536; 32 slices of 2,048 rows
    "fb237_embedding": "chunk=65536 padded_r=240 split=32",
    # 16,777,216 / 1,348 = 12,446 -> 97 tiles of rows; 11 x 2 tiles -> 256 / 22 = 11 slices (31 slabs would fit)
    "fb15k_embedding": "chunk=12416 padded_r=1348 split=11",
    "reserve_64": "chunk=64 padded_r=20 split=1",                   # 64 rows: no slice is 256 deep
    "one_positive": "chunk=1 padded_r=4 split=1",
    "r_multiple_of_4": "chunk=4096 padded_r=256 split=16",          # 4,096 / 256 rows a slice at least
    "huge_r": "chunk=128 padded_r=200000 split=1",                  # never less than one tile of rows
    "bad_arguments": "chunk=0 padded_r=0 split=1",
    "bad_relations": "chunk=0 padded_r=0 split=1",
    # the function's own slab limit (no context reaches it): room for five slabs, room for none
    "slab_limit_5": "chunk=30000 padded_r=240 split=5",
    "slab_limit_0": "chunk=30000 padded_r=240 split=1",
}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_plan_table_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "relation_softmax_plan_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "relation_softmax_plan_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "relation_softmax_plan_driver: ok"
    got = dict(line.split(": ", 1) for line in lines[:-1])
    assert got.pop("cuts") == "long_row=64 piece=64" and got.pop("own_slab_floats") == str(2 ** 23)
    wrong = {k: (got.get(k), v) for k, v in PLAN.items() if got.get(k) != v}
    assert not wrong, wrong
    assert set(got) == set(PLAN)


def test_the_library_answers_with_the_same_plan():
    """rgcn_relation_softmax_plan is the header's function behind the C ABI (context-free: no GPU)"""
    from relationprediction_amd import _native
    assert _native.relation_softmax_plan(30000, 237, 500) == {
        "chunk": 30000, "padded_r": 240, "split_k": 32, "long_row": 64, "piece": 64}
    assert _native.relation_softmax_plan(272115, 237, 500)["split_k"] == 32        # the driver's fb237_embedding row
    assert _native.relation_softmax_plan(483142, 1345, 200) == {
        "chunk": 12416, "padded_r": 1348, "split_k": 11, "long_row": 64, "piece": 64}
    assert _native.relation_softmax_plan(64, 18, 8)["chunk"] == 64
    with pytest.raises(_native.RgcnError):
        _native.relation_softmax_plan(0, 18, 8)
