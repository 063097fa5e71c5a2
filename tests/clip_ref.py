"""float64 numpy restatement of clipping by global norm: segment norms, the global norm, the clipping scale and
the Adam + EMA step on the scaled gradient.  g = grad * grad_scale is formed in fp32, as the optimiser forms it; everything
after that is float64."""
import numpy as np

F32 = np.float32


def scaled_grad(grad, grad_scale=1.0):
    """grad * grad_scale rounded to fp32, as float64."""
    return (np.asarray(grad, F32) * F32(grad_scale)).astype(np.float64)


def segment_norms(grad, bounds, grad_scale=1.0):
    """(norms float64 [n_seg], global norm): segment k is [bounds[k], bounds[k + 1]); the global norm is the square root of the
    sum of the segments' sums of squares."""
    g = scaled_grad(grad, grad_scale)
    sums = np.array([np.sum(np.square(g[bounds[k]:bounds[k + 1]])) for k in range(len(bounds) - 1)], np.float64)
    return np.sqrt(sums), float(np.sqrt(np.sum(sums)))


def clip_scale(norm, clip):
    """tf.clip_by_global_norm's factor with the norm rounded to fp32 before the comparison and the division (the device holds
    it in fp32): exactly 1.0 at norm <= clip, hence for clip = inf."""
    n32, c32 = F32(norm), F32(clip)
    if n32 <= c32:
        return 1.0
    return float(np.float64(c32) / np.float64(n32))


def adam_ema_step(p, grad, m, v, ema, *, lr_t, grad_scale=1.0, scale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, decay=0.999):
    """One TF-1.x Adam + EMA step on (grad * grad_scale) * scale (both products in fp32, in that order), float64 after that.
    Returns new (p, m, v, ema)."""
    g = ((np.asarray(grad, F32) * F32(grad_scale)) * F32(scale)).astype(np.float64)
    p, m, v, ema = (np.asarray(a, np.float64) for a in (p, m, v, ema))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - lr_t * m / (np.sqrt(v) + eps)
    ema = ema - (1.0 - decay) * (ema - p)
    return p, m, v, ema
