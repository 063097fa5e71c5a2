"""numpy restatement of the time-jitter contract (include/vqwave.h) that the kernel tests compare against
bit for bit.

    lo = float32(p / 2), hi = float32(1 - p / 2)      (each formed in float64, rounded once)
    move = -1 if u < lo, +1 if u >= hi, else 0        (float32 compares)
    src = t + move; src < 0: += 2; src >= Tz: -= 2; Tz == 1: 0
    fwd:  out[b, d, t] = z[b, d, src[b, t]]
    bwd:  dz[b, d, s] = sum of g[b, d, t] over t in {s-1, s, s+1} inside [0, Tz) with src[b, t] == s,
          added in ascending t in the dtype of g, starting from +0.0
Rows (b) are independent."""
import numpy as np


def thresholds(p):
    return np.float32(np.float64(p) / 2.0), np.float32(1.0 - np.float64(p) / 2.0)


def src_of(u, p):
    """u float32 [B][Tz] -> src int32 [B][Tz]."""
    u = np.asarray(u, dtype=np.float32)
    lo, hi = thresholds(p)
    Tz = u.shape[1]
    move = np.where(u < lo, -1, np.where(u >= hi, 1, 0))
    src = np.arange(Tz)[None, :] + move
    src = np.where(src < 0, src + 2, src)
    src = np.where(src >= Tz, src - 2, src)
    if Tz == 1:
        src = np.zeros_like(src)
    return src.astype(np.int32)


def fwd(z, src):
    """z [B][D][Tz], src [B][Tz] -> out [B][D][Tz] (a gather along time: no arithmetic)."""
    z = np.asarray(z)
    return np.take_along_axis(z, np.broadcast_to(src[:, None, :].astype(np.int64), z.shape), axis=2)


def bwd(g, src):
    """g [B][D][Tz], src [B][Tz] -> dz [B][D][Tz] in g's dtype, terms added in ascending t from +0.0."""
    g = np.asarray(g)
    B, D, Tz = g.shape
    dz = np.zeros_like(g)
    s = np.arange(Tz)
    for off in (-1, 0, 1):
        t = s + off
        ok = (t >= 0) & (t < Tz)
        tc = np.clip(t, 0, Tz - 1)
        hit = ok[None, :] & (src[:, tc] == s[None, :])                    # [B][Tz]: frame t read frame s
        term = g[:, :, tc]
        dz = np.where(hit[:, None, :], (dz + term).astype(g.dtype), dz)
    return dz
