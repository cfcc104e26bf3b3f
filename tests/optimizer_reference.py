"""Float64 mirror of the device optimizer's two stateless-per-row algorithms (csrc/optimizer.hip k_sgd, k_adagrad) behind
tf.clip_by_global_norm, as TensorFlow 1.x documents them (tensorflow_backend/algorithms.py:5-16,44-55,58-68):

    scale = max_norm / max(||g||_2, max_norm)   (1 when max_norm is 0: no GradientClipping component);  g <- scale * g
    GradientDescent:  w -= lr * g
    AdaGrad:          a += g^2;  w -= lr * g / sqrt(a)        a starts at initial_accumulator (0.1), there is no epsilon

Everything is float64 whatever comes in.  tests/test_optimizers_host.py pins it to hand-computed values; the GPU tests
(tests/test_gpu_optimizers.py) feed it the DEVICE's gradients, pre-step weights and pre-step accumulators, one step at a time,
so that what they compare is the optimizer alone."""
import numpy as np

EPS32 = 2.0 ** -23


def global_norm(grads, names):
    return float(np.sqrt(sum(float((np.asarray(grads[n], np.float64) ** 2).sum()) for n in names)))


def clip_scale(grads, names, max_norm):
    if not max_norm > 0:
        return 1.0
    return max_norm / max(global_norm(grads, names), max_norm)


def step(algorithm, weights, grads, accumulators, names, lr, max_norm=0.0):
    """One update of the tensors `names`.  Returns (change of every weight = new - old, new accumulators or None); the
    inputs are left alone.  accumulators: AdaGrad's, {name: array} as they stood BEFORE the step (ignored otherwise)."""
    scale = clip_scale(grads, names, max_norm)
    delta, acc = {}, ({} if algorithm == "AdaGrad" else None)
    for n in names:
        g = np.asarray(grads[n], np.float64) * scale
        if algorithm == "GradientDescent":
            delta[n] = -lr * g
        elif algorithm == "AdaGrad":
            acc[n] = np.asarray(accumulators[n], np.float64) + g * g
            delta[n] = -lr * g / np.sqrt(acc[n])
        else:
            raise ValueError(algorithm)
    return delta, acc


def update_bound(old_weights, delta_ref, clipped):
    """The issue's bound on |delta_device - delta_ref|, per element: the rounding of w - u (2^-23 |w|) plus the update's own
    error: at most eight fp32 roundings (8 x 2^-23 |d|) or, with the clip on, the project's allowance for the fp32 norm in
    the Adam replay (2e-5 |d|)."""
    return EPS32 * np.abs(np.asarray(old_weights, np.float64)) + (2e-5 if clipped else 8 * EPS32) * np.abs(delta_ref)


ACCUMULATOR_RTOL = 8 * EPS32
