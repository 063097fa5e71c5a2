"""Gradient accumulation restated in numpy (WaveNet.accumulate): the fp32 left-to-right sum that vqw_grad_accumulate
builds over a window, and the window's bookkeeping on the host -- which call copies, which adds, which closes, and what
global_step and accum_index read after each.

The sum is part of the contract: acc = g0 (a copy), acc = fl(acc + g_k) for the micro-steps in between, and the closing call
leaves fl(acc + g_{N-1}) in the flat gradient.  One fp32 add per element and call, in call order; nothing is reassociated.
"""
import numpy as np

F32 = np.float32


def window_sum(grads):
    """fl(fl(g0 + g1) + g2) ...: the flat gradient after the closing micro-step of a window over `grads` (fp32 arrays)."""
    acc = np.asarray(grads[0], F32).copy()
    for g in grads[1:]:
        acc = (acc + np.asarray(g, F32)).astype(F32)      # (fp32 + fp32 in numpy is one IEEE fp32 add per element)
    return acc


def window_sum_right_to_left(grads):
    """A wrong variant: the same terms summed from the last to the first."""
    return window_sum(list(grads)[::-1])


def window_sum_closing_twice(grads):
    """A wrong variant: the closing gradient added once more (what a closing step would leave that also wrote the accumulator
    and then read it again)."""
    return window_sum(list(grads) + [grads[-1]])


def window_sum_fp64(grads):
    return np.sum([np.asarray(g, np.float64) for g in grads], axis=0)


def kernel(acc, grad):
    """One vqw_grad_accumulate call: the copy (acc None) or one fp32 add per element."""
    grad = np.asarray(grad, F32)
    with np.errstate(all='ignore'):      # (an overflow to Inf, or Inf - Inf = NaN, is a result here, not a warning)
        return grad.copy() if acc is None else (np.asarray(acc, F32) + grad).astype(F32)


def same_by_class(got, want):
    """Per element: both NaN, or both +Inf, or both -Inf, or bit-equal finite values (NaN payloads are no part of the contract)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(got) & np.isnan(want)
    bits = got.view(np.uint32) == want.view(np.uint32)        # (covers +-Inf and the finite values, signed zeros included)
    return bool(np.all(nan | (bits & ~np.isnan(got) & ~np.isnan(want))))


def schedule(n_accumulate, calls, global_step=0, k=0):
    """The bookkeeping of `calls` train_step calls with accumulate = N from (global_step, accum_index) = (global_step, k): one
    dict per call -- form ('copy': out = acc <- grad; 'add': acc <- acc + grad; 'close': grad <- acc + grad, then the optimiser;
    with N = 1 'step': the optimiser alone), closes, the k the call ran with, and global_step / accum_index after it."""
    out = []
    for _ in range(calls):
        if n_accumulate == 1:
            form, closes = 'step', True
        else:
            closes = k == n_accumulate - 1
            form = 'close' if closes else ('copy' if k == 0 else 'add')
        ran_with = k
        if closes:
            global_step, k = global_step + 1, 0
        else:
            k += 1
        out.append({'form': form, 'closes': closes, 'k': ran_with, 'global_step': global_step, 'accum_index': k})
    return out
