"""numpy restatement of the codebook-by-moving-averages contract (include/vqwave.h) that the kernel and model
tests compare against bit for bit.  Frames are numbered f = b * Tz + t, Nf = B * Tz.

    g = float32(decay), h = float32(1 - decay) (the subtraction in float64, rounded once), tau = float32(restart)
    pick[k] = min(int(u[k] * Nf), Nf - 1)             (a float32 product, truncated)
    cnt[k] = #{f : idx[f] == k};  sum[k] = z_e of those frames added in ascending f in float32 from +0.0;
    cand[k] = z_e of frame pick[k]
    n' = g n + h float(cnt);  m' = g m + h sum        (every operation rounded to float32 on its own)
    n' < tau (tau > 0): n' = 1, m' = E = cand;  else cnt > 0: E = m' / n';  else E keeps its bits
    info = (codes restarted, codes with cnt > 0)"""
import numpy as np

f32 = np.float32


def constants(decay, restart=0.0):
    return f32(decay), f32(1.0 - np.float64(decay)), f32(restart)


def picks(u, Nf):
    """u float32 [K] in [0, 1) -> pick int32 [K]."""
    p = (np.asarray(u, f32) * f32(Nf)).astype(f32)
    return np.minimum(p.astype(np.int32), Nf - 1).astype(np.int32)


def stats(z_e, idx, K, pick=None):
    """z_e float32 [B][D][Tz], idx int [B][Tz] -> cnt int32 [K], sum float32 [K][D], cand float32 [K][D] (None without pick)."""
    z_e = np.asarray(z_e, f32)
    B, D, Tz = z_e.shape
    flat = np.asarray(idx).reshape(-1)
    cnt = np.zeros(K, np.int32)
    tot = np.zeros((K, D), f32)                       # +0.0
    for f in range(B * Tz):                           # ascending f: the order of the adds
        k = int(flat[f])
        if 0 <= k < K:
            cnt[k] += 1
            tot[k] = (tot[k] + z_e[f // Tz, :, f % Tz]).astype(f32)
    cand = None
    if pick is not None:
        p = np.clip(np.asarray(pick), 0, B * Tz - 1)
        cand = np.ascontiguousarray(z_e[p // Tz, :, p % Tz]).astype(f32)
    return cnt, tot, cand


def update(E, n, m, cnt, tot, cand, decay, restart=0.0):
    """One update; returns new (E, n, m, info) and leaves its arguments alone."""
    g, h, tau = constants(decay, restart)
    E, n, m = np.array(E, f32), np.array(n, f32), np.array(m, f32)
    cnt = np.asarray(cnt, np.int32)
    n1 = ((g * n).astype(f32) + (h * cnt.astype(f32)).astype(f32)).astype(f32)
    m1 = ((g * m).astype(f32) + (h * np.asarray(tot, f32)).astype(f32)).astype(f32)
    dead = (n1 < tau) if tau > 0 else np.zeros(n1.shape, bool)
    used = (cnt > 0) & ~dead
    with np.errstate(divide='ignore', invalid='ignore'):
        q = (m1 / n1[:, None]).astype(f32)
    E[used] = q[used]
    if dead.any():
        c = np.asarray(cand, f32)
        E[dead], m1[dead], n1[dead] = c[dead], c[dead], f32(1)
    return E, n1, m1, np.array([int(dead.sum()), int((cnt > 0).sum())], np.int32)


def step(E, n, m, z_e, idx, u, decay, restart=0.0):
    """Statistics, picks and update of one training step on one rank."""
    K = E.shape[0]
    B, D, Tz = z_e.shape
    pick = picks(u, B * Tz) if restart > 0 else None
    cnt, tot, cand = stats(z_e, idx, K, pick)
    return update(E, n, m, cnt, tot, cand, decay, restart)
