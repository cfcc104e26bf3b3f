"""Float64 mirror of the device optimizer's three algorithms (csrc/optimizer.hip k_adam, k_sgd, k_adagrad) behind
tf.clip_by_global_norm, as TensorFlow 1.x documents them (tensorflow_backend/algorithms.py:5-16,27-42,44-55,58-68):

    scale = max_norm / max(||g||_2, max_norm)   (1 when max_norm is 0: no GradientClipping component);  g <- scale * g
    GradientDescent:  w -= lr * g
    AdaGrad:          a += g^2;  w -= lr * g / sqrt(a)        a starts at initial_accumulator (0.1), there is no epsilon
    Adam:             t = steps taken before + 1;  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
                      m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  w -= lr_t m / (sqrt(v) + eps)

Everything is float64 whatever comes in.  Adam's hyper-parameters are to be given AS THE FLOAT32 VALUES THE ABI RECEIVES
(f32(0.999), not 0.999): 1 - b is then exact, as it is on the device.  tests/test_optimizers_host.py pins the mirror to
hand-computed values and the bounds below to an fp32 emulation of the kernels; the GPU tests (tests/test_gpu_optimizers.py)
feed the mirror the DEVICE's gradients, pre-step weights and pre-step slots, one step at a time, so that what they compare is
the optimizer alone.

The bounds, counted from the kernels with u = 2^-24 (one correctly rounded fp32 operation; the library is built without
fast-math, so divide and square root are correctly rounded too):

  clip scale   k_sqnorm_part makes 8 fma, 6 shuffle adds and 2 adds: 16 roundings on a sum of non-negative terms; the
               partials are summed in double; the square root halves the relative error (8u); one rounding to float and
               one for the division: SCALE_RTOL = 10u = 5 x 2^-23.
  shard norm   k_sum_range: the same 16 roundings and one to float, no square root: SHARD_NORM_RTOL = 17u.
  change       2^-23 |w_old| for the rounding of w - update, and of the update 8 x 2^-23 (at most eight roundings; Adam:
               lr_t, lr_t m, sqrt, + eps, the divide, 2u A from m and 1.5u from v under the root: below 5 x 2^-23), with
               the clip on (8 + 5) x 2^-23: one more factor with SCALE_RTOL and its rounding.  Adam's update is measured
               by U = lr_t A / (sqrt(v) + eps), A = |b1 m0| + |(1 - b1) g|, not by |d|: m can cancel, its error does not.
  m            4u A, clipped 16u A;        v and AdaGrad's accumulator: 4u v (8 x 2^-23 a), clipped 28u."""
import collections

import numpy as np

EPS32 = 2.0 ** -23
U24 = 2.0 ** -24
SCALE_RTOL = 10 * U24
SHARD_NORM_RTOL = 17 * U24
ADAM_VARIANTS = ("rate_uncorrected", "step_late", "eps_under_root")      # three wrong Adams a test must tell from the right one

AdamStep = collections.namedtuple("AdamStep", "m v A U")


def f32(x):
    """a hyper-parameter as the float32 the ABI receives, as a Python float"""
    return float(np.float32(x))


def global_norm(grads, names):
    return float(np.sqrt(sum(float((np.asarray(grads[n], np.float64) ** 2).sum()) for n in names)))


def scale_of_norm(norm, max_norm):
    return max_norm / max(norm, max_norm) if max_norm > 0 else 1.0


def clip_scale(grads, names, max_norm):
    if not max_norm > 0:
        return 1.0
    return scale_of_norm(global_norm(grads, names), max_norm)


def adam_rate(lr, beta1, beta2, t):
    return lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def step(algorithm, weights, grads, accumulators, names, lr, max_norm=0.0, step_count=0, beta1=f32(0.9), beta2=f32(0.999),
         eps=f32(1e-8), scale=None, variant=None):
    """One update of the tensors `names`.  Returns (change of every weight = new - old, new state or None); the inputs are
    left alone.  accumulators: the state as it stood BEFORE the step -- AdaGrad {name: accumulator}, Adam {name: (m, v)},
    ignored otherwise; step_count: Adam's steps taken BEFORE this one.  The new state: AdaGrad {name: accumulator}, Adam
    {name: AdamStep(m, v, A, U)}.  scale: the clip scale, where the caller knows the global norm better than `grads` does
    (a sharded run).  variant: one of ADAM_VARIANTS, an Adam that is wrong in that way."""
    if scale is None:
        scale = clip_scale(grads, names, max_norm)
    delta, acc = {}, (None if algorithm == "GradientDescent" else {})
    if algorithm == "Adam":
        assert variant is None or variant in ADAM_VARIANTS, variant
        t = step_count + (2 if variant == "step_late" else 1)
        lr_t = lr if variant == "rate_uncorrected" else adam_rate(lr, beta1, beta2, t)
    for n in names:
        g = np.asarray(grads[n], np.float64) * scale
        if algorithm == "GradientDescent":
            delta[n] = -lr * g
        elif algorithm == "AdaGrad":
            acc[n] = np.asarray(accumulators[n], np.float64) + g * g
            delta[n] = -lr * g / np.sqrt(acc[n])
        elif algorithm == "Adam":
            m0, v0 = (np.asarray(x, np.float64) for x in accumulators[n])
            m = beta1 * m0 + (1.0 - beta1) * g
            A = np.abs(beta1 * m0) + np.abs((1.0 - beta1) * g)
            v = beta2 * v0 + (1.0 - beta2) * g * g
            root = np.sqrt(v + eps) if variant == "eps_under_root" else np.sqrt(v) + eps
            delta[n] = -lr_t * m / root
            acc[n] = AdamStep(m, v, A, lr_t * A / root)
        else:
            raise ValueError(algorithm)
    return delta, acc


def update_bound(old_weights, delta_ref, clipped):
    """The bound on |delta_device - delta_ref|, per element: the rounding of w - u (2^-23 |w|) plus the update's own error,
    at most eight fp32 roundings (8 x 2^-23 |d|) and, with the clip on, the scale's (13 x 2^-23 |d|).  Adam: delta_ref is
    AdamStep.U, the update's size before its two terms cancel."""
    return EPS32 * np.abs(np.asarray(old_weights, np.float64)) + (13 if clipped else 8) * EPS32 * np.abs(delta_ref)


ACCUMULATOR_RTOL = 8 * EPS32


def accumulator_rtol(clipped):
    """AdaGrad's accumulator, relative: a + g^2 in one fma; with the clip on g^2 carries twice the scale's error"""
    return 28 * U24 if clipped else ACCUMULATOR_RTOL


def adam_m_bound(A, clipped):
    return (16 if clipped else 4) * U24 * np.asarray(A, np.float64)


def adam_v_bound(v, clipped):
    return (28 if clipped else 4) * U24 * np.asarray(v, np.float64)


# ------------------------------------------------------------------ inputs that reach the kernels' corners
def injected_case(n, seed, steps=3):
    """(weights [n] float32, [gradient [n] float32 per step]) for an optimizer fed gradients of the test's own making.
    Gradients: magnitude log-uniform in [1e-12, 1e3], random sign; the first tenth in [1e-9, 1e-7], where Adam's eps
    decides; the second tenth keeps its magnitude and has the same sign on steps 1 and 3 and the opposite one on step 2, so
    that m cancels; a tenth are exact zeros, half of those on every step (state that stays zero); the last three elements
    are of the top decade, so that the norm shows whether a tensor's tail was counted; step 2 is multiplied by 1e-3, so the
    clip scale differs from step to step.  Weights: half 0.5 x randn, half exactly 0 -- where the bound is the
    update's alone."""
    rng = np.random.RandomState(seed)
    tenth = max(n // 10, 1)
    w = (0.5 * rng.randn(n)).astype(np.float32)
    w[rng.permutation(n)[: n // 2]] = 0.0
    always_zero = rng.rand(n) < 0.05
    magnitude2 = 10.0 ** rng.uniform(-12, 3, tenth)
    sign2 = np.where(rng.rand(tenth) < 0.5, -1.0, 1.0)
    grads = []
    for s in range(steps):
        g = 10.0 ** rng.uniform(-12, 3, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
        g[:tenth] = 10.0 ** rng.uniform(-9, -7, tenth) * np.sign(g[:tenth])
        g[tenth:2 * tenth] = (magnitude2 * sign2 * (-1.0 if s == 1 else 1.0))[: len(g[tenth:2 * tenth])]
        g[always_zero | (rng.rand(n) < 0.05)] = 0.0
        g[-3:] = (10.0 ** rng.uniform(2, 3, 3) * np.where(rng.rand(3) < 0.5, -1.0, 1.0))[-min(n, 3):]
        if s == 1:
            g *= 1e-3
        grads.append(g.astype(np.float32))
    return w, grads


# ------------------------------------------------------------------ the kernels' arithmetic in numpy float32
def _fma32(a, b, c):
    """fmaf: the product of two floats is exact in double; the sum's rounding to double before the one to float can move a
    result that lies within 2^-29 ulp of a tie, which no bound here notices"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def emulated_partials(g):
    """k_sqnorm_part's block partials of one tensor: 2048 elements per workgroup, a lane's two quads 1024 apart, eight fma
    in element order, the 64-lane shuffle tree, (r0 + r1) + (r2 + r3)"""
    g = np.asarray(g, np.float32).ravel()
    blocks = (g.size + 2047) // 2048
    q = np.zeros(blocks * 2048, np.float32)
    q[: g.size] = g
    q = q.reshape(blocks, 2, 256, 4)                       # [block, k, thread, element of the quad]
    acc = np.zeros((blocks, 256), np.float32)
    for k in range(2):
        for e in range(4):
            acc = _fma32(q[:, k, :, e], q[:, k, :, e], acc)
    acc = acc.reshape(blocks, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[:, :, :off] + acc[:, :, off:2 * off]
    return (acc[:, 0, 0] + acc[:, 1, 0]) + (acc[:, 2, 0] + acc[:, 3, 0])


def emulated_clip_scale(tensors, max_norm):
    """k_clip_scale after k_sqnorm_part over `tensors`: float32"""
    if not max_norm > 0:
        return np.float32(1.0)
    total = sum(float(emulated_partials(g).astype(np.float64).sum()) for g in tensors)
    norm = np.float32(np.sqrt(total))
    return np.float32(max_norm) / max(norm, np.float32(max_norm))


def emulated_adam(w, g, m0, v0, lr, beta1, beta2, eps, step_count, scale):
    """k_adam, operation by operation in float32: (new w, m, v)"""
    one = np.float32(1.0)
    b1, b2, eps = np.float32(beta1), np.float32(beta2), np.float32(eps)
    lr_t = np.float32(adam_rate(float(np.float32(lr)), float(b1), float(b2), step_count + 1))
    g = np.asarray(g, np.float32) * np.float32(scale)
    m = _fma32(b1, m0, (one - b1) * g)
    v = _fma32(b2, v0, (one - b2) * g * g)
    return np.asarray(w, np.float32) - lr_t * m / (np.sqrt(v) + eps), m, v
