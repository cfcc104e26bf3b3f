"""Algorithm.Name = AdaGrad and GradientDescent on the GPU (csrc/optimizer.hip k_adagrad, k_sgd) and the optimizer's state
through the C ABI (rgcn_get/set_optimizer_slot, _step): every update against the float64 mirror of
tests/optimizer_reference.py fed with the DEVICE's gradients, pre-step weights and pre-step accumulators; the sharded phase
API; state handed from one context to another; a captured step; the training driver with --save-optimizer-state / --resume.

Shapes of the update cases, with 256 x 8 = 2048 elements per workgroup and 4 per lane and load:
  block  V 257, R 5, d 9, 3 blocks, L 2: W_emb 2313 = one full workgroup + a tail of 265 (66 quads and one element: the
         one-by-one path inside a vectorised tensor), W_self 81 and b_emb 9 (less than a workgroup, odd), W_f / W_b 135;
  basis  B 2, V 130, R 8, d 20, L 2: W_emb 2600 (a second workgroup), the [d, B, d] tensors in their device layout;
  embedding  V 300, d 12: W_emb 3600, W_relation 3600 of which the first R rows (72 elements) are updated."""
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


# ------------------------------------------------------------------ the update against the float64 mirror
@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["unclipped", "clip-1"])
@pytest.mark.parametrize("algorithm", ["AdaGrad", "GradientDescent"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_update_matches_the_float64_mirror(native, case, algorithm, max_norm):
    """Three train steps.  After each: the device's gradients, weights and accumulators; the step mirrored in float64 from
    those gradients and the PRE-step weights and accumulators; compared is the CHANGE new - old (an update is about 1e-4
    of a weight: at a tolerance made for weights no update at all would pass), per element, within
        2^-23 |w| + 8 x 2^-23 |d_ref|      (max_grad_norm 0: the rounding of w - u, and at most eight roundings in u)
        2^-23 |w| + 2e-5 |d_ref|           (max_grad_norm 1: the project's allowance for the fp32 norm, as the Adam replay)
    and the accumulators within 8 x 2^-23 relative.  Every comparison first shows that it could fail: the largest mirrored
    change is at least 100 times the largest error allowed.  AdaGrad: the mirror started from accumulators 0.1 lower (an
    initial accumulator of 0) misses the bound by more than 100 times.  What has no gradient does not change by a bit."""
    c, lr, clipped = CASES[case], RATES[algorithm], max_norm > 0
    with Run(native, c, algorithm, max_norm) as run:
        eng = run.eng
        names = moved_names(eng)
        slots = eng.optimizer_slot_count()
        assert slots == (1 if algorithm == "AdaGrad" else 0)
        cur = eng.get_params()
        acc = {n: eng.get_optimizer_slot(n, 0) for n in names} if slots else None
        if slots:
            assert all((a == np.float32(0.1)).all() for a in acc.values())
        for step in range(3):
            run.step(seed=500 + step)
            assert np.isfinite(eng.loss())
            grads = eng.get_grads()
            new = eng.get_params()
            new_acc = {n: eng.get_optimizer_slot(n, 0) for n in names} if slots else None
            assert eng.optimizer_step_count() == step + 1
            want, want_acc = ref.step(algorithm, cur, grads, acc, names, lr, max_norm)
            if slots:
                zero_start = {n: acc[n].astype(np.float64) - 0.1 for n in names}
                with np.errstate(invalid="ignore", divide="ignore"):
                    unfilled, _ = ref.step(algorithm, cur, grads, zero_start, names, lr, max_norm)
            worst_unfilled = 0.0
            for n in names:
                old = cur[n].astype(np.float64)
                got = new[n].astype(np.float64) - old
                bound = ref.update_bound(old, want[n], clipped)
                largest = float(np.abs(want[n]).max())
                print("%s %s step %d %-10s max|d_ref| %.3e  max bound %.3e  max err/bound %.3f"
                      % (case, algorithm, step, n, largest, float(bound.max()),
                         float((np.abs(got - want[n]) / np.maximum(bound, 1e-300)).max())))
                assert largest >= 100 * float(bound.max()), (step, n, largest, float(bound.max()))
                err = np.abs(got - want[n])
                assert (err <= bound).all(), (step, n, float((err / np.maximum(bound, 1e-300)).max()))
                if slots:
                    a_ref = want_acc[n]
                    assert (np.abs(new_acc[n] - a_ref) <= ref.ACCUMULATOR_RTOL * a_ref).all(), (step, n)
                    miss = np.abs(got - np.nan_to_num(unfilled[n], nan=np.inf)) / np.maximum(bound, 1e-300)
                    worst_unfilled = max(worst_unfilled, float(miss.max()))
            if slots:
                assert worst_unfilled > 100, (step, worst_unfilled)
            for n in eng.param_names:
                if n not in names:
                    assert np.array_equal(new[n], cur[n]), n                         # no gradient: not a bit
            R = c["R"]
            assert np.array_equal(new["W_relation"][R:], cur["W_relation"][R:])        # rows past RelationCount
            assert not np.array_equal(new["W_relation"][:R], cur["W_relation"][:R])
            if slots:
                assert (new_acc["W_relation"][R:] == np.float32(0.1)).all()
            cur, acc = new, new_acc


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
