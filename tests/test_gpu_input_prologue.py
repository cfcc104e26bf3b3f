"""The A-operand prologue of the pre-split-weight NN GEMM kernels (csrc/gemm_bf16x3_w8.hip, csrc/gemm_bf16x3.hip APRO):
layer 1's self-loop product reads W_emb, forms H0 = relu(W_emb + b_emb) on load -- k_input_fwd's fp32 expression -- and
writes it back, so the separate pass over H0 leaves the step (csrc/rgcn_schedule.hip, h0_by_self_loop_gemm).

Kernel level (rgcn_debug_gemm_prologue): the written-back operand is bitwise np.maximum(A + bias, 0), nothing outside
[rows below the limit] x [K] of the target is touched, and the product is bitwise the same kernel's product on the
materialised operand -- padding in K (partial last k-tile, fewer k-tiles than the ring is deep), rows past the extent,
both XCD swizzles, both kernels, six and nine partial products.
Engine level: with the devtools knob RGCN_H0_IN_GEMM on and off, codes, activations and every gradient are bitwise equal
(train and test mode, and through a captured step), and the paths that must keep k_input_fwd still launch it."""
import os

import numpy as np
import pytest

import oracle
from helpers import assert_close, make_case

pytestmark = pytest.mark.gpu

KNOB = "RGCN_H0_IN_GEMM"
CANARY = np.float32(-77.25)


@pytest.fixture(scope="module")
def native():
    from relationprediction_amd import _native
    _native.load_library()
    return _native


class knob:
    """the devtools build reads the knob from the environment at every forward pass"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.prev = os.environ.get(KNOB)
        os.environ[KNOB] = str(self.value)

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.prev


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ kernel level
@pytest.fixture(scope="module")
def gemm_engines(native):
    engs = {}
    for mode in (6, 9):
        e = native.Engine(16, 2, 8, 1, "block", 2, max_edges=4, devtools=True)
        e.set_gemm_mode(mode)
        engs[mode] = e
    yield engs
    for e in engs.values():
        e.close()


@pytest.mark.parametrize("mode", [6, 9])
@pytest.mark.parametrize("wide", [True, False], ids=["w8", "128x128"])
@pytest.mark.parametrize("K", [4, 16, 20, 500])
def test_prologue_gemm_writes_back_and_multiplies_the_transformed_operand(gemm_engines, mode, wide, K):
    """M in {1, 127, 129, 257} x N in {5, 256, 260, 500} x both swizzles for one (kernel, mode, K): K = 20 and 500 leave a
    partial last k-tile, K = 4 is less than one tile (and fewer stages than the eight-wavefront ring is deep), the bias is
    nowhere zero (relu(0 + b) != 0: padding that went through the prologue would show in C), the write-back target has
    lda = K + 4 > K and is filled with a canary."""
    eng = gemm_engines[mode]
    rng = np.random.RandomState(1000 * K + 10 * mode + int(wide))
    lda = K + 4
    bias = (rng.uniform(0.25, 1.5, K) * rng.choice([-1.0, 1.0, 1.0], K)).astype(np.float32)
    for M in (1, 127, 129, 257):
        for N in (5, 256, 260, 500):
            A = np.full((M, lda), 3.5, dtype=np.float32)          # (the padding columns hold finite junk: never read)
            A[:, :K] = rng.randn(M, K).astype(np.float32)
            B = (rng.randn(K, N) * np.exp(rng.uniform(-3, 3, (K, N)))).astype(np.float32)
            # swizzle 1: no device-side extent; swizzle 2: the extent read on the device, the last rows do not exist
            for limit in (-1, max(1, M - 3)):
                rows = M if limit < 0 else limit
                tag = "M %d N %d K %d limit %d wide %s mode %d" % (M, N, K, limit, wide, mode)
                canary = np.full((M, lda), CANARY, dtype=np.float32)
                C, a_out = eng.debug_gemm_prologue(A, bias, B, canary, wide=wide, prologue=True, row_limit=limit)
                want = canary.copy()
                want[:rows, :K] = np.maximum(A[:rows, :K] + bias[None, :], np.float32(0))
                # (a) the transformed operand, (b) nothing else of the lda x M extent
                np.testing.assert_array_equal(bits(a_out), bits(want), err_msg="a_out: " + tag)
                # (c) the same kernel on the materialised operand
                C_ref, untouched = eng.debug_gemm_prologue(a_out, bias, B, canary, wide=wide, prologue=False, row_limit=limit)
                np.testing.assert_array_equal(bits(untouched), bits(canary), err_msg="plain product wrote a_out: " + tag)
                np.testing.assert_array_equal(bits(C[:rows]), bits(C_ref[:rows]), err_msg="C: " + tag)
                assert not C[rows:].any() and not C_ref[rows:].any(), "rows past the extent were stored: " + tag
                assert np.isfinite(C).all(), tag


# ------------------------------------------------------------------ engine level
ENGINE_CASES = [(130, 20, 5), (300, 20, 4), (300, 32, 8), (130, 32, 8)]      # (V, d, nb): sd = d / nb in {4, 5}
R, L, E, KEEP = 7, 2, 400, 0.8


def run_once(native, V, d, nb, train, on, kind="block", fusion=1, profile=False):
    params, triples, masks, dcodes = make_case(V, R, d, L, kind, nb, E, seed=V + d + nb)
    with knob(1 if on else 0):
        eng = native.Engine(V, R, d, L, kind, nb, keep_prob=KEEP, max_edges=E, devtools=True)
        try:
            eng.set_fusion(fusion)
            eng.set_params(params)
            eng.set_graph(triples)
            if profile:
                eng.profile_enable(True)
            eng.forward(train=train, seed=3, masks=masks if train else None)
            acts = [eng.activation(l) for l in range(L + 1)]
            eng.backward(dcodes)
            grads = eng.get_grads()
            prof = None
            if profile:
                eng.profile_enable(False)
                prof = {p["name"]: p for p in eng.profile()}
            return acts, grads, prof
        finally:
            eng.close()


@pytest.mark.parametrize("train", [True, False], ids=["train", "test"])
@pytest.mark.parametrize("V,d,nb", ENGINE_CASES)
def test_engine_is_bitwise_the_separate_pass(native, V, d, nb, train):
    acts_on, grads_on, prof = run_once(native, V, d, nb, train, True, profile=True)
    acts_off, grads_off, prof_off = run_once(native, V, d, nb, train, False, profile=True)
    # the knob does what it says: the pass is gone with it on, there with it off, and the GEMM accounts for the H0 write
    assert prof.get("input_fwd", {"calls": 0})["calls"] == 0
    assert prof_off["input_fwd"]["calls"] == 1
    extra = prof["gemm_self_fwd"]["alg_bytes"] - prof_off["gemm_self_fwd"]["alg_bytes"]
    assert extra == 4.0 * V * d
    assert prof["gemm_self_fwd"]["compulsory_bytes"] - prof_off["gemm_self_fwd"]["compulsory_bytes"] == 4.0 * V * d
    for l, (a, b) in enumerate(zip(acts_on, acts_off)):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg="H%d" % l)
    assert set(grads_on) == set(grads_off)
    for k in grads_off:
        np.testing.assert_array_equal(bits(grads_on[k]), bits(grads_off[k]), err_msg="grad " + k)
    # the knob-off run against the oracle, at test_gpu_parity.py's tolerance
    params, triples, masks, dcodes = make_case(V, R, d, L, "block", nb, E, seed=V + d + nb)
    oacts, ograds = oracle.encoder_step(params, triples, V, L, "block", dcodes, keep_prob=KEEP,
                                        dropout_masks=masks if train else None, mode="train" if train else "test")
    for l, (a, b) in enumerate(zip(acts_off, oacts)):
        assert float(np.abs(a - b).max()) <= 1e-4, "H%d against the oracle" % l
    for k, g in grads_off.items():
        if k != "W_relation":
            assert_close(g, ograds[k], rel=2e-4, name="grad " + k)


def test_captured_step_is_bitwise_the_separate_pass(native):
    V, d, nb = 300, 20, 5
    params, triples, masks, dcodes = make_case(V, R, d, L, "block", nb, E, seed=9)
    out = {}
    for on in (True, False):
        with knob(1 if on else 0):
            eng = native.Engine(V, R, d, L, "block", nb, keep_prob=KEEP, max_edges=E, devtools=True)
            try:
                eng.set_params(params)
                T, D = eng.to_device(triples), eng.to_device(dcodes)
                eng.step_device(T, len(triples), D, train=True, seed=1)      # lazy allocations happen here
                eng.sync()
                eng.capture_begin()
                eng.step_device(T, len(triples), D, train=True, seed=100)
                gid = eng.capture_end()
                eng.graph_launch(gid)
                eng.graph_launch(gid)
                out[on] = ([eng.activation(l) for l in range(L + 1)], eng.get_grads())
                T.free()
                D.free()
            finally:
                eng.close()
    for l, (a, b) in enumerate(zip(out[True][0], out[False][0])):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg="H%d" % l)
    for k in out[False][1]:
        np.testing.assert_array_equal(bits(out[True][1][k]), bits(out[False][1][k]), err_msg="grad " + k)


@pytest.mark.parametrize("kind,nb,fusion", [("basis", 2, 1), ("block", 5, 0)], ids=["basis", "two-kernel-block"])
def test_other_paths_keep_the_separate_pass(native, kind, nb, fusion):
    """The basis kind's aggregation and the two-kernel block form's message kernel read H0 beside the self-loop GEMM:
    k_input_fwd stays, knob or no knob."""
    _, _, prof = run_once(native, 130, 20, nb, True, True, kind=kind, fusion=fusion, profile=True)
    assert prof["input_fwd"]["calls"] == 1
