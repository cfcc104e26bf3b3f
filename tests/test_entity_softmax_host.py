"""The entity-softmax loss term without a GPU: the float64 mirror (tests/entity_softmax_reference.py) against finite
differences of its own loss and against its own special cases, the eager numpy surface of BilinearDiag against the mirror,
the [Decoder] EntitySoftmaxWeight and EntitySoftmaxPositives keys, the runtime's bookkeeping, and the host-side code --
the plan's table (csrc/entity_softmax_plan.h), the range lookup's edge cases (csrc/entity_softmax_range.h) and the second
index's builder -- in their sanitizer driver (tests/sanitize/entity_softmax_driver.cpp, built with g++ under ASan + UBSan
and run as a program)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import entity_softmax_reference as esr
import relation_softmax_reference as rsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (V, R, dc, P, seed, masked)
CASES = {"small": (30, 5, 4, 12, 1, False), "two_entities": (2, 3, 3, 9, 2, False), "wide": (67, 4, 6, 20, 3, False),
         "masked": (30, 6, 4, 16, 4, True)}


def case(name):
    V, R, dc, P, seed, masked = CASES[name]
    codes, w_rel, pos = esr.make_case(V, R, dc, P, seed)
    known = None
    if masked:
        rng = np.random.RandomState(seed)
        more_objects = np.stack([pos[::2, 0], pos[::2, 1], rng.randint(0, V, len(pos[::2]))], 1)
        more_subjects = np.stack([rng.randint(0, V, len(pos[1::2])), pos[1::2, 1], pos[1::2, 2]], 1)
        known = np.concatenate([pos, more_objects, more_subjects]).astype(np.int32)
    return codes, w_rel, pos, known


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_case_compares_zeros(name):
    codes, w_rel, pos, known = case(name)
    t = esr.term(codes, w_rel, pos, 0.7, known=known)
    assert abs(t["loss"]) > 1e-3 and np.abs(t["G"]).max() > 0 and np.abs(t["dW"]).max() > 0 and np.abs(t["dcodes"]).max() > 0
    assert np.abs(t["dq"]).max() > 0
    if known is not None:
        assert (~t["mask"]).sum() > 0 and not t["G"][~t["mask"]].any()
        a, r, g, side = esr.rows_of(pos)
        assert t["mask"][np.arange(len(g)), g].all()                   # the gold stays a candidate although it is known
    np.testing.assert_allclose(t["G"].sum(axis=1), 0, atol=1e-15)      # softmax minus one-hot
    assert pos[0, 0] == pos[0, 2]                                      # both roles on one entity


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_agree_with_central_differences(name):
    """both roles of the codes (candidate and query) and W_relation: the mirror's dcodes and dW against
    (loss(x + h) - loss(x - h)) / 2h of its own loss, in float64 throughout (exact_query)"""
    codes, w_rel, pos, known = case(name)
    c64, w64 = codes.astype(np.float64), w_rel.astype(np.float64)
    t = esr.term(c64, w64, pos, 0.7, known=known, exact_query=True)
    h = 1e-6
    rng = np.random.RandomState(0)
    for which, arr, grad in (("codes", c64, t["dcodes"]), ("W_relation", w64, t["dW"])):
        touched = np.argwhere(grad != 0)
        picks = touched[rng.choice(len(touched), size=min(25, len(touched)), replace=False)]
        for i, j in picks:
            up, down = arr.copy(), arr.copy()
            up[i, j] += h
            down[i, j] -= h
            args = (lambda a: (a, w64)) if which == "codes" else (lambda a: (c64, a))
            fd = (esr.term(*args(up), pos, 0.7, known=known, exact_query=True)["loss"]
                  - esr.term(*args(down), pos, 0.7, known=known, exact_query=True)["loss"]) / (2 * h)
            assert abs(fd - grad[i, j]) <= 1e-7 * max(1.0, abs(grad[i, j])), (which, i, j, fd, grad[i, j])
    used = np.unique(pos[:, 1])
    assert not np.delete(t["dW"], used, axis=0).any()                  # rows of W_relation no positive names


def distinct_queries(pos):
    """positives no two of which share (s, r) or (r, o): K = the positives masks nothing but golds"""
    _, a = np.unique(pos[:, [0, 1]], axis=0, return_index=True)
    pos = pos[np.sort(a)]
    _, b = np.unique(pos[:, [1, 2]], axis=0, return_index=True)
    return pos[np.sort(b)]


def test_masked_equals_plain_when_nothing_else_is_known():
    codes, w_rel, pos, _ = case("small")
    pos = distinct_queries(pos)
    assert len(pos) >= 8
    plain = esr.term(codes, w_rel, pos, 0.7)
    masked = esr.term(codes, w_rel, pos, 0.7, known=pos)               # K holds the positives themselves only
    assert masked["mask"].all() and masked["loss"] == plain["loss"]
    for k in ("G", "dq", "dW", "dcodes"):
        np.testing.assert_array_equal(masked[k], plain[k])


def test_a_saturated_row_contributes_exactly_zero():
    codes, w_rel, pos, _ = case("small")
    pos = distinct_queries(pos)
    V = len(codes)
    s, r, o = pos[3]
    full = np.concatenate([pos, np.stack([np.full(V, s), np.full(V, r), np.arange(V)], 1)]).astype(np.int32)
    t = esr.term(codes, w_rel, pos, 0.7, known=full)                   # every object is known for (s, r, ?)
    assert t["ell"][3] == 0 and not t["G"][3].any() and not t["dq"][3].any()
    assert np.abs(np.delete(t["ell"], 3)).min() > 0                    # ... and its subject row, like the others, is not


def test_weight_zero_is_the_decoder_loss():
    codes, w_rel, pos, _ = case("small")
    t = esr.term(codes, w_rel, pos, 0.0)
    assert t["loss"] == 0 and not t["G"].any() and not t["dW"].any() and not t["dcodes"].any()
    # ... and through the eager surface: the loss and gradients with the key at 0 are those without the key, bit for bit
    X = np.concatenate([pos, pos[:, [2, 1, 0]]]).astype(np.int32)
    Y = np.concatenate([np.ones(len(pos)), np.zeros(len(pos))]).astype(np.float32)
    seen = []
    for weight in (None, "0"):
        model = eager(codes, w_rel, 5, weight)
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


def eager(codes, w_rel, R, weight=None, positives=None):
    from relationprediction_amd.decoders.bilinear_diag import BilinearDiag
    s = _Settings(EntityCount=len(codes), RelationCount=R, EdgeCount=1, RegularizationParameter="0.01")
    if weight is not None:
        s["EntitySoftmaxWeight"] = weight
    if positives is not None:
        s["EntitySoftmaxPositives"] = positives
    model = BilinearDiag(_Codes(codes, w_rel), s)
    model.local_initialize_train()
    return model


@pytest.mark.parametrize("limit", [None, "7"])
def test_eager_loss_and_backward_equal_the_mirror(limit):
    codes, w_rel, pos, _ = case("wide")
    rng = np.random.RandomState(9)
    neg = pos.copy()
    neg[:, 0] = rng.randint(0, len(codes), len(pos))
    X = np.concatenate([pos[:5], neg, pos[5:]]).astype(np.int32)       # the positives are where the labels say, not in front
    Y = np.concatenate([np.ones(5), np.zeros(len(neg)), np.ones(len(pos) - 5)]).astype(np.float32)
    out = {}
    for weight in (None, "0.6"):
        model = eager(codes, w_rel, 4, weight, limit)
        model.X.feed(X)
        model.Y.feed(Y)
        out[weight] = (model.get_loss('train'), model.backward())
    t = esr.term(codes, w_rel, pos if limit is None else pos[:7], 0.6)
    assert abs(t["loss"]) > 1e-3
    assert abs(out["0.6"][0] - out[None][0] - t["loss"]) <= 1e-12 * max(1.0, abs(t["loss"]))
    dcodes = out["0.6"][1][0].astype(np.float64) - out[None][1][0].astype(np.float64)
    d_rel = out["0.6"][1][1].astype(np.float64) - out[None][1][1].astype(np.float64)
    # (the eager surface returns float32: the difference of two float32 sums against the float64 mirror)
    scale = max(np.abs(out[None][1][0]).max(), np.abs(out[None][1][1]).max(), np.abs(t["dcodes"]).max(), np.abs(t["dW"]).max())
    assert np.abs(dcodes - t["dcodes"]).max() <= 4 * 2.0 ** -24 * scale
    assert np.abs(d_rel - t["dW"]).max() <= 4 * 2.0 ** -24 * scale


# ------------------------------------------------------------------ the settings keys
@pytest.mark.parametrize("value,expected", [(None, 0.0), ("0", 0.0), ("0.5", 0.5), ("2", 2.0), (" 1e-3 ", 1e-3), (0.25, 0.25)])
def test_weight_is_parsed(value, expected):
    from relationprediction_amd.decoders.bilinear_diag import parse_entity_softmax_weight
    s = _Settings(RegularizationParameter="0.01")
    if value is not None:
        s["EntitySoftmaxWeight"] = value
    assert parse_entity_softmax_weight(s) == expected
    assert eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, value).entity_softmax_weight == expected


@pytest.mark.parametrize("value", ["-1", "-0.5", "half", "", "Yes", "nan", "inf", True])
def test_a_bad_weight_is_refused(value):
    from relationprediction_amd.decoders.bilinear_diag import parse_entity_softmax_weight
    with pytest.raises(ValueError, match="EntitySoftmaxWeight"):
        parse_entity_softmax_weight(_Settings(EntitySoftmaxWeight=value))
    with pytest.raises(ValueError, match="EntitySoftmaxWeight"):
        eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, value)


@pytest.mark.parametrize("value,expected", [(None, 0), ("0", 0), ("1024", 1024), (" 7 ", 7), (4096, 4096)])
def test_positives_are_parsed(value, expected):
    from relationprediction_amd.decoders.bilinear_diag import parse_entity_softmax_positives
    s = _Settings()
    if value is not None:
        s["EntitySoftmaxPositives"] = value
    assert parse_entity_softmax_positives(s) == expected
    assert eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, "0.5", value).entity_softmax_positives == expected


@pytest.mark.parametrize("value", ["-1", "1.5", "many", "", "Yes", "1e3", True, 2.0])
def test_bad_positives_are_refused(value):
    from relationprediction_amd.decoders.bilinear_diag import parse_entity_softmax_positives
    with pytest.raises(ValueError, match="EntitySoftmaxPositives"):
        parse_entity_softmax_positives(_Settings(EntitySoftmaxPositives=value))
    with pytest.raises(ValueError, match="EntitySoftmaxPositives"):
        eager(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), 3, "0.5", value)


def test_one_entity_is_refused_at_start_up():
    from relationprediction_amd import train as train_module
    with pytest.raises(ValueError, match="two entities"):
        train_module.entity_softmax_settings(_Settings(EntitySoftmaxWeight="0.5"), 1)
    assert train_module.entity_softmax_settings(_Settings(EntitySoftmaxWeight="0"), 1) == (0.0, 0)      # off asks nothing
    assert train_module.entity_softmax_settings(_Settings(), 1) == (0.0, 0)
    assert train_module.entity_softmax_settings(_Settings(EntitySoftmaxWeight="0.5", EntitySoftmaxPositives="9"), 2) == (0.5, 9)


def test_the_runtime_tells_the_engine_only_what_changed():
    """all four driver paths go through EncoderRuntime._entity_softmax: reserve when the positives outgrow it, the setter
    when (weight, positives, mask) changed, the index only when none is resident, the count cut at EntitySoftmaxPositives"""
    from relationprediction_amd.runtime import EncoderRuntime

    class Engine(object):
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name,) + tuple(x if np.isscalar(x) else "array" for x in a))

    rt = EncoderRuntime.__new__(EncoderRuntime)
    rt.engine = Engine()
    rt._entity_softmax(300)
    assert rt.engine.calls == []                                        # the key is absent: the engine hears nothing
    rt.set_entity_softmax(0.5)
    rt._entity_softmax(300)
    rt._entity_softmax(300)
    assert rt.engine.calls == [("entity_softmax_reserve", 300), ("set_entity_softmax", 0.5, 300, False)]
    rt.set_entity_softmax(0.5, known=np.zeros((2, 3), np.int32))
    rt._entity_softmax(200)
    assert rt.engine.calls[2:] == [("known_positives_reserve", "array"), ("set_entity_softmax", 0.5, 200, True)]
    rt.set_entity_softmax(0.5, positives=64)                            # the leading 64 of a step's positives
    rt._entity_softmax(200)
    rt._entity_softmax(300)
    assert rt.engine.calls[4:] == [("set_entity_softmax", 0.5, 64, False)]
    rt._entity_softmax(40)                                              # a step with fewer positives than the key allows
    assert rt.engine.calls[5:] == [("set_entity_softmax", 0.5, 40, False)]
    rt.set_entity_softmax(0.0)
    rt._entity_softmax(200)
    assert rt.engine.calls[6:] == [("set_entity_softmax", 0.0, 0, False)]


# ------------------------------------------------------------------ the host plan, the range lookup, the second index
PLAN = {
    # FB15k-237, V = 14,541 -> 14,544 columns: 2^26 floats / 14,544 = 4,614 rows -> 36 whole tiles = 4,608.  114 x 4 tiles
    # of the [14,544, 500] product already exceed the 256 the split aims at: no split.  V % 4 = 1: the NN product reads the
    # padded copy
    "fb237_minibatch": "chunk=4608 padded_v=14544 split=1 nn_padded=1",
    "fb237_embedding": "chunk=4608 padded_v=14544 split=1 nn_padded=1",
    # the 256 MB boundary: 2 x 2,303 = 4,606 rows fit as they are; 4,608 are exactly what the cap holds; 4,610 are cut
    "boundary_below": "chunk=4606 padded_v=14544 split=1 nn_padded=1",
    "boundary_at": "chunk=4608 padded_v=14544 split=1 nn_padded=1",
    "boundary_above": "chunk=4608 padded_v=14544 split=1 nn_padded=1",
    "reserve_64": "chunk=128 padded_v=92 split=1 nn_padded=1",         # two rows per positive; one slice of 128 rows
    "two_slices": "chunk=300 padded_v=300 split=2 nn_padded=0",        # 300 rows / 128 a slice at least
    "one_positive": "chunk=2 padded_v=4 split=1 nn_padded=1",
    "v_multiple_of_4": "chunk=8192 padded_v=256 split=64 nn_padded=0", # 2 tiles -> 128 slices wanted, 64 at most
    "huge_v": "chunk=128 padded_v=2000000 split=1 nn_padded=0",        # never less than one tile of rows
    "bad_arguments": "chunk=0 padded_v=0 split=1 nn_padded=0",
    "bad_entities": "chunk=0 padded_v=0 split=1 nn_padded=0",
    # the function's own slab limit: room for five slabs of [300, 8], room for none
    "slab_limit_5": "chunk=6000 padded_v=300 split=5 nn_padded=0",
    "slab_limit_0": "chunk=6000 padded_v=300 split=1 nn_padded=0",
}

RANGES = {
    "empty_index": ("lo=0 hi=0 of 0", []),
    "range_at_key_0": ("lo=0 hi=2 of 3", [0, 3]),
    "range_at_last_key": ("lo=1 hi=3 of 3", [1, 4]),
    "whole_index": ("lo=0 hi=3 of 3", [0, 2, 4]),
    "between_neighbours": ("lo=2 hi=4 of 6", [0, 4]),
    "absent_between_neighbours": ("lo=1 hi=1 of 2", []),
    "subjects_of_a_pair": ("lo=1 hi=3 of 6", [2, 3]),
}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_plan_table_and_range_lookup_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "entity_softmax_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-x", "c++",
           os.path.join(ROOT, "tests", "sanitize", "entity_softmax_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr) and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "entity_softmax_driver: ok"
    got = dict(line.split(": ", 1) for line in lines[:-1])
    assert got.pop("cuts") == "long_row=64 piece=64" and got.pop("own_slab_floats") == str(2 ** 24)
    assert got.pop("energy_floats") == str(2 ** 26)                     # 256 MB
    for name, (span, members) in RANGES.items():
        assert got.pop(name) == span, name
        assert [int(got.pop("%s[%d]" % (name, i))) for i in range(len(members))] == members, name
    wrong = {k: (got.get(k), v) for k, v in PLAN.items() if got.get(k) != v}
    assert not wrong, wrong
    assert set(got) == set(PLAN)


def test_the_library_answers_with_the_same_plan():
    """rgcn_entity_softmax_plan is the header's function behind the C ABI (context-free: no GPU)"""
    from relationprediction_amd import _native
    assert _native.entity_softmax_plan(30000, 14541, 500) == {
        "chunk": 4608, "padded_v": 14544, "split_k": 1, "long_row": 64, "piece": 64}
    assert _native.entity_softmax_plan(2303, 14541, 500)["chunk"] == 4606
    assert _native.entity_softmax_plan(150, 300, 8) == {"chunk": 300, "padded_v": 300, "split_k": 2, "long_row": 64, "piece": 64}
    assert _native.entity_softmax_plan(64, 90, 8)["chunk"] == 128
    with pytest.raises(_native.RgcnError):
        _native.entity_softmax_plan(0, 18, 8)
