"""References of the kernels between the encoder and the decoder -- the two vq_nearest entries and the speaker tile of
csrc/vq.hip, the three local-condition projections of csrc/cond_proj.hip -- their seeded case tables and their bars, for
tests/test_cond_path_ref_cpu.py and tests/test_cond_path_kernels_gpu.py.

Everything here is numpy on the CPU, written from the sentences of include/vqwave.h and not from the kernels' index arithmetic.
Every reference takes the caller's flat buffers, the outputs as they are before the call included, and returns per output an
Out(vals, mask, bar): a float64 copy of the whole flat buffer with the written positions replaced, the mask of those positions,
and the elementwise bar over the buffer (None: bit for bit).  compare() holds the masked positions to the bar and everything
else -- gaps of a wider batch stride, table rows no frame chose, guard bands -- to bit-equality.

Exact expectations.  The VQ forward pass is fp32 arithmetic in a stated order (subtract, multiply and add each rounded, d
ascending: oracle.ref_model.vq_distances_np), the lowest index among equal minima, e_k a copy and zq = z + (e_k - z) with both
steps rounded; the speaker forward pass is a copy.  A distance that is not below +inf (NaN, overflow) never wins: a row all of
whose distances are such gets idx 0 and mind = +inf, which is what oracle/vqw_oracle.c returns (its argmin starts from
(+inf, 0) and takes strict improvements only).  NaN compares equal to NaN here whatever its payload.

Bars.  Each is n * U * S elementwise, U = 2^-24: S the float64 sum of the absolute values of everything added into the element
(the old contents included where the kernel accumulates), n the number of additions any summation order needs plus one per
extra rounding the header's formula contains:

    cond_proj_fwd     Cc + 1          cond_proj_wgrad   B*Tz + 2          cond_proj_dgrad   Mall
    demb              frames of that code + 2                             dtable            Tz + rows of that speaker + 1
    dz_e              3 * U * (|dzq| + |cscale (z - e_k)|)

The bars are set against the reference, never against a kernel: the CPU test evaluates each with a plain fp32 emulation of
its formula (a sequential sum, each product rounded once) and asserts that it stays at or under EMU_FRACTION of the bar on
every case.  One constant was moved because the EMULATION did not fit, none because a kernel failed: cond_proj_fwd was Cc.
The emulation rounds every product before it is summed, one rounding more than the Cc - 1 additions and the spare one that
n = Cc holds; at Cc = 1 that rounding is the whole error and attains U * |w cond| itself (0.996 of the bar over 50 000
elements), at Cc = 2 the three roundings against 2 U S came to 0.96.  Cc + 1 is the count with that rounding in it: 0.50 and
0.64.  (Measured afterwards: the forward kernel's own worst case is that 0.64 at Cc = 2, digit for digit -- DESIGN 6.)
The tightest of the others is dz_e, whose emulation reaches 0.74 of 3 U (|dzq| + |cscale (z - e_k)|) on 525 000 elements."""
import collections

import numpy as np

from conv_ref import GUARD, SENTINEL, Buf, randn  # noqa: F401  (re-exported to the two test files)
from pointwise_ref import EMU_FRACTION, F32, U, ratio_of, seed_of  # noqa: F401

Out = collections.namedtuple('Out', 'vals mask bar')
CUS = (32, 256, 304)                       # CU counts the path rules are checked at: a partition, MI355X, MI300X


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _out(buf0, pos, vals, bar=None):
    """The caller's flat buffer with `vals` at the flat positions `pos` (bar likewise, zero elsewhere)."""
    v = _f64(buf0).reshape(-1).copy()
    m = np.zeros(v.size, dtype=bool)
    pos = np.asarray(pos).reshape(-1)
    v[pos] = _f64(vals).reshape(-1)
    m[pos] = True
    b = None
    if bar is not None:
        b = np.zeros(v.size)
        b[pos] = _f64(bar).reshape(-1)
    return Out(v, m, b)


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- comparison
def compare(got, buf, out, what=''):
    """got: the WHOLE fp32 buffer read back; buf: the conv_ref.Buf as it was before the launch; out: the reference's Out over
    the view.  Returns the worst err / bar (0.0 for a bit-exact comparison)."""
    ref = buf.full.astype(np.float64)
    ref[buf.lo:buf.lo + buf.n] = out.vals
    written = np.zeros(ref.size, dtype=bool)
    written[buf.lo:buf.lo + buf.n] = out.mask
    g = np.asarray(got).reshape(-1)
    assert g.dtype == np.float32 and g.size == ref.size, '%s: buffer sizes differ' % what
    r32 = ref.astype(F32)
    same = (g.view(np.uint32) == r32.view(np.uint32)) | (np.isnan(g) & np.isnan(r32))
    if out.bar is None:
        same |= written & (g == 0) & (r32 == 0)                  # a written zero has no promised sign
        bad = ~same
    else:
        bad = ~same & ~written
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError('%s: %d elements are not bit-equal to the reference (first: element %d, %s, got %r, want %r)' % (
            what, int(bad.sum()), i - buf.lo, 'written' if written[i] else 'must stay untouched', float(g[i]), float(ref[i])))
    if out.bar is None:
        return 0.0
    bar = np.zeros(ref.size)
    bar[buf.lo:buf.lo + buf.n] = out.bar
    return ratio_of(g[written], ref[written], bar[written], what, np.flatnonzero(written) - buf.lo)


# ---------------------------------------------------------------------------------------------------- vq_nearest_fwd
VQ_FWD_SHAPES = ((1, 1, 4, 1), (1, 3, 4, 63), (2, 5, 60, 64), (3, 5, 64, 65), (2, 9, 68, 130), (2, 7, 128, 512), (8, 104, 64, 512))
VQ_NONFINITE = ((2, 9, 68, 130), (8, 104, 64, 512))
VQ_PLANTS = ('same_lane', 'adjacent') + tuple('xor%d' % s for s in range(6)) + ('with_0', 'with_last', 'winner_last')


def vq_fwd_cases():
    return [dict(name='b%d_t%d_d%d_k%d' % s, B=s[0], Tz=s[1], D=s[2], K=s[3], nonfinite=s in VQ_NONFINITE, order=i, family='vq_fwd')
            for i, s in enumerate(VQ_FWD_SHAPES)]


def vq_fwd_variants(c):
    """(zq_bstride, with e_k, with zq, with mind): production's wide stride, the default, each optional output absent."""
    wide = (c['D'] + 16) * c['Tz']
    return [(wide, True, True, True), (0, True, True, True), (wide, False, True, True), (wide, True, False, True), (0, True, True, False)]


def vq_fwd_legal(c):
    """vqw_vq_nearest_fwd: positive sizes, D a multiple of 4 (emb 16-byte aligned: the test's to provide)."""
    return c['B'] > 0 and c['Tz'] > 0 and c['K'] > 0 and c['D'] > 0 and c['D'] % 4 == 0


def vq_plant_groups(K, order):
    """Disjoint groups of codes made exactly equal, as (kind, codes, winner).  winner_last needs code K-1 to be unique, so
    a case plants either it or with_last (by `order`)."""
    used, out = {0, K - 1}, []

    def take(kind, pairs):
        for a, b in pairs:
            if b < K and a != b and a not in used and b not in used:
                used.update((a, b))
                out.append((kind, (a, b), min(a, b)))
                return
    take('same_lane', ((k, k + 64) for k in range(1, K)))                  # both scanned by lane k % 64
    take('adjacent', ((k, k + 1) for k in range(1, K, 2)))                 # odd k: the two differ in more than bit 0
    for s in range(6):
        take('xor%d' % s, ((k, k ^ (1 << s)) for k in range(1, K)))        # lanes that meet in shuffle stage s
    if K >= 4:
        j = next(k for k in range(1, K - 1) if k not in used)
        used.add(j)
        out.append(('with_0', (0, j), 0))
        if order % 2 == 0:
            j = next((k for k in range(1, K - 1) if k not in used), None)
            if j is not None:
                out.append(('with_last', (j, K - 1), j))
    if K >= 2 and (order % 2 == 1 or K < 4):
        out.append(('winner_last', (K - 1,), K - 1))
    return out[order % max(len(out), 1):] + out[:order % max(len(out), 1)]


def vq_fwd_inputs(c):
    """z [B][D][Tz], emb [K][D], plants [(kind, row, codes, winner)], nan_row, inf_row (row = b * Tz + t; None without).
    Plants fill the rows from the last one down (the partial last block of four rows gets some), the two non-finite rows are
    rows 0 and 1."""
    B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
    sd = seed_of('vq_fwd', c['name'])
    rng = np.random.RandomState(sd)
    z = (rng.standard_normal((B, D, Tz)) * 0.2).astype(F32)
    emb = rng.uniform(-0.13, 0.13, (K, D)).astype(F32)
    rows = B * Tz
    first = 2 if c['nonfinite'] else 0
    plants = []
    for i, (kind, codes, winner) in enumerate(vq_plant_groups(K, c['order'])):
        row = rows - 1 - i
        if row < first:
            break
        for k in codes[1:]:
            emb[k] = emb[codes[0]]
        z[row // Tz, :, row % Tz] = emb[codes[0]]
        plants.append((kind, row, codes, winner))
    nan_row = inf_row = None
    if c['nonfinite']:
        nan_row, inf_row = 0, 1
        z[0, D // 2, 0] = np.nan
        z[1 // Tz, :, 1 % Tz] = F32(1e20) * np.where(np.arange(D) % 2, F32(-1), F32(1)).astype(F32)
    return dict(z=z, emb=emb, plants=plants, nan_row=nan_row, inf_row=inf_row)


def vq_rows(z_e, B, D, Tz):
    """The frames as rows: [B*Tz][D] from the flat [B][D][Tz]."""
    return np.ascontiguousarray(np.asarray(z_e, F32).reshape(B, D, Tz).transpose(0, 2, 1).reshape(B * Tz, D))


def vq_pos(B, D, Tz, bstride):
    """Flat positions b * bstride + d * Tz + t of the frames' rows, [B*Tz][D]."""
    b, t, d = np.arange(B)[:, None, None], np.arange(Tz)[None, :, None], np.arange(D)[None, None, :]
    return (b * bstride + d * Tz + t).reshape(B * Tz, D)


def vq_nearest_ref(z_e, emb, e_k0, zq0, zq_bstride, mind0, B, D, Tz, K):
    """-> dict(idx int64 [B*Tz], e_k, zq, mind): Out or None where the caller passes no buffer.  All bit-exact."""
    from oracle import ref_model as M
    rows, e = vq_rows(z_e, B, D, Tz), np.asarray(emb, F32).reshape(K, D)
    with np.errstate(all='ignore'):
        dist = M.vq_distances_np(rows, e)
        dist = np.where(dist < np.inf, dist, F32(np.inf))                 # never below the (+inf, 0) the search starts from
        idx = np.argmin(dist, axis=1).astype(np.int64)                     # numpy: the first of equal minima
        ek = e[idx]
        zq = (rows + (ek - rows).astype(F32)).astype(F32)
    bs = zq_bstride or D * Tz
    return dict(idx=idx,
                e_k=None if e_k0 is None else _out(e_k0, vq_pos(B, D, Tz, D * Tz), ek),
                zq=None if zq0 is None else _out(zq0, vq_pos(B, D, Tz, bs), zq),
                mind=None if mind0 is None else _out(mind0, np.arange(B * Tz), dist.min(1)))


_oracle = []


def oracle_vq_nearest(rows, emb):
    """oracle/vqw_oracle.c (built as tests/test_oracle.py builds it) on frames as rows -> idx, e_k, zq [rows][D], mind."""
    import ctypes
    import os
    import subprocess
    if not _oracle:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        so = os.path.join(root, 'oracle', '_build', 'liboracle.so')
        if not os.path.exists(so):
            subprocess.check_call(['make', '-s', '-C', os.path.join(root, 'oracle')])
        _oracle.append(ctypes.CDLL(so))
    rows, emb = np.ascontiguousarray(rows, F32), np.ascontiguousarray(emb, F32)
    n, D = rows.shape
    vp = ctypes.c_void_p
    idx, ek, zq, md = np.zeros(n, np.int64), np.zeros_like(rows), np.zeros_like(rows), np.zeros(n, F32)
    _oracle[0].oracle_vq_nearest(rows.ctypes.data_as(vp), emb.ctypes.data_as(vp), idx.ctypes.data_as(vp), ek.ctypes.data_as(vp),
                                 zq.ctypes.data_as(vp), md.ctypes.data_as(vp), n, emb.shape[0], D)
    return idx, ek, zq, md


# ---------------------------------------------------------------------------------------------------- vq_nearest_bwd
VQ_LDS_BYTES = 144 * 1024
VQ_LDS_PASS = 64 * 256 * 16                # elements one pass of the LDS kernel's grid covers
GRID_PASS = 2048 * 256                     # elements one pass of a plain grid-stride kernel covers
VQ_CSCALE, VQ_ESCALE = float(F32(0.3)), float(F32(0.7))


def _vb(B, Tz, D, K, codes='nearest', dzq=True, dz_e=True, demb=True, wide=True):
    tag = ''.join(t for t, on in (('_nodzq', not dzq), ('_nodz', not dz_e), ('_nodemb', not demb), ('_dense', not wide)) if on)
    return dict(name='b%d_t%d_d%d_k%d_%s%s' % (B, Tz, D, K, codes, tag), B=B, Tz=Tz, D=D, K=K, codes=codes, dzq=dzq, dz_e=dz_e,
                demb=demb, wide=wide, family='vq_bwd')


def vq_bwd_cases():
    """codes: 'nearest' = vq_nearest_ref's, 'one' = every frame on one code, 'all' = spread over all K, 'rand'."""
    return [_vb(1, 1, 4, 1), _vb(2, 5, 12, 40), _vb(3, 7, 8, 16, 'all'), _vb(2, 5, 6, 40, 'rand', wide=False),
            _vb(2, 9, 64, 576, 'rand'), _vb(2, 9, 64, 577, 'rand'),                 # K*D*4 = 147 456 exactly, and one code more
            _vb(2, 5, 12, 40, demb=False), _vb(2, 5, 12, 40, dz_e=False), _vb(2, 5, 12, 40, dzq=False),
            _vb(2, 9, 64, 577, 'rand', dz_e=False), _vb(2, 9, 64, 577, 'rand', dzq=False),
            _vb(4, 64, 16, 8, 'one'), _vb(4, 64, 16, 2305, 'one'),
            _vb(40, 104, 64, 32, 'rand'), _vb(79, 104, 64, 577, 'rand')]             # a second pass of each kernel's grid


def vq_bwd_legal(c):
    """vqw_vq_nearest_bwd: z_e, e_k and idx, and at least one of dz_e and demb."""
    return min(c['B'], c['Tz'], c['D'], c['K']) > 0 and (c['dz_e'] or c['demb'])


def vq_bwd_path(c):
    """The LDS kernel holds the whole table: it runs when demb is asked for and K * D * 4 <= 144 KiB, the plain kernel else."""
    p = 'lds' if (c['demb'] and c['K'] * c['D'] * 4 <= VQ_LDS_BYTES) else 'plain'
    n = c['B'] * c['D'] * c['Tz']
    return p, n > (VQ_LDS_PASS if p == 'lds' else GRID_PASS)


def vq_bwd_inputs(c):
    B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
    sd = seed_of('vq_bwd', c['name'])
    rng = np.random.RandomState(sd)
    z = (rng.standard_normal((B, D, Tz)) * 0.2).astype(F32)
    emb = rng.uniform(-0.13, 0.13, (K, D)).astype(F32)
    rows = B * Tz
    if c['codes'] == 'nearest':
        idx = vq_nearest_ref(z, emb, None, None, 0, None, B, D, Tz, K)['idx']
    elif c['codes'] == 'one':
        idx = np.full(rows, K // 2, dtype=np.int64)
    elif c['codes'] == 'all':
        idx = rng.permutation(np.arange(rows) % K).astype(np.int64)
    else:
        idx = rng.randint(0, K, rows).astype(np.int64)
    e_k = np.ascontiguousarray(emb[idx].reshape(B, Tz, D).transpose(0, 2, 1))
    bs = (D + 16) * Tz if c['wide'] else D * Tz
    return dict(z=z, e_k=e_k, idx=idx, dzq=randn(sd + 1, (B - 1) * bs + D * Tz), dzq_bstride=bs, demb0=randn(sd + 2, K, D),
                cscale=VQ_CSCALE, escale=VQ_ESCALE)


def vq_bwd_ref(z_e, e_k, idx, dzq, dzq_bstride, dz_e0, demb0, cscale, escale, B, D, Tz, K):
    """dz_e = dzq + cscale (z - e_k);  demb[idx] += escale (e_k - z), onto the caller's demb.  dzq None: zero.
    -> dict(dz_e, demb): Out or None where the caller passes no buffer."""
    z, e = vq_rows(z_e, B, D, Tz).astype(np.float64), vq_rows(e_k, B, D, Tz).astype(np.float64)
    idx = np.asarray(idx, np.int64).reshape(-1)
    out = dict(dz_e=None, demb=None)
    if dz_e0 is not None:
        g = np.zeros_like(z) if dzq is None else _f64(dzq).reshape(-1)[vq_pos(B, D, Tz, dzq_bstride)]
        c = cscale * (z - e)
        out['dz_e'] = _out(dz_e0, vq_pos(B, D, Tz, D * Tz), g + c, 3.0 * U * (np.abs(g) + np.abs(c)))
    if demb0 is not None:
        a = escale * (e - z)
        v, s = _f64(demb0).reshape(K, D).copy(), np.abs(_f64(demb0)).reshape(K, D)
        np.add.at(v, idx, a)
        np.add.at(s, idx, np.abs(a))
        frames = np.bincount(idx, minlength=K)
        chosen = np.flatnonzero(frames)
        pos = (chosen[:, None] * D + np.arange(D)[None, :])
        out['demb'] = _out(demb0, pos, v[chosen], (frames[chosen, None] + 2) * U * s[chosen])
    return out


def vq_bwd_emulation(z_e, e_k, idx, dzq, dzq_bstride, demb0, cscale, escale, B, D, Tz, K):
    """Plain fp32: every step of both formulas rounded, demb summed frame after frame.  -> dz_e [B*Tz][D], demb [K][D]."""
    z, e = vq_rows(z_e, B, D, Tz), vq_rows(e_k, B, D, Tz)
    g = np.zeros_like(z) if dzq is None else np.asarray(dzq, F32).reshape(-1)[vq_pos(B, D, Tz, dzq_bstride)]
    dz = (g + (F32(cscale) * (z - e).astype(F32)).astype(F32)).astype(F32)
    demb = np.asarray(demb0, F32).reshape(K, D).copy()
    np.add.at(demb, np.asarray(idx).reshape(-1), (F32(escale) * (e - z).astype(F32)).astype(F32))     # unbuffered: in frame order
    return dz, demb


# ---------------------------------------------------------------------------------------------------- speaker tile
def _sp(B, Cs, Tz, ids, row0=0, wide=False, n_spk=5):
    return dict(name='b%d_cs%d_t%d_%s_row%d%s' % (B, Cs, Tz, ids, row0, '_wide' if wide else ''), B=B, Cs=Cs, Tz=Tz, ids=ids,
                row0=row0, wide=wide, n_spk=n_spk, family='speaker')


def speaker_cases():
    """ids: 'distinct', 'repeat' (batch rows share speakers), 'outside' (-1 and n_speakers among them)."""
    return [_sp(1, 1, 1, 'distinct'), _sp(16, 16, 8, 'repeat', row0=64, wide=True), _sp(1, 257, 3, 'distinct', row0=4),
            _sp(25, 16, 5, 'repeat', row0=64, n_spk=7), _sp(8, 50, 1, 'outside', row0=12, wide=True), _sp(3, 16, 8, 'outside'),
            _sp(2, 16, 104, 'repeat', row0=64), _sp(33, 16, 1000, 'repeat', wide=True, n_spk=9)]     # the last: 528 000 elements


def speaker_legal(c):
    """vqw_speaker_tile_*: positive sizes, int64 ids (any value), a table of n_speakers >= 1 rows."""
    return min(c['B'], c['Cs'], c['Tz'], c['n_spk']) > 0 and c['row0'] >= 0


def speaker_inputs(c):
    B, Cs, Tz, S, row0 = c['B'], c['Cs'], c['Tz'], c['n_spk'], c['row0']
    sd = seed_of('speaker', c['name'])
    rng = np.random.RandomState(sd)
    if c['ids'] == 'distinct':
        spk = rng.permutation(S)[:B]
    else:
        spk = rng.randint(1, S - 1, B)                      # rows 0 and S-1 stay unchosen unless an outside id picks row 0
        if B > 1:
            spk[-1] = spk[0]
    spk = spk.astype(np.int64)
    if c['ids'] == 'outside':
        spk[0], spk[-1] = -1, S
    bs = (row0 + Cs + (3 if c['wide'] else 0)) * Tz
    return dict(table=randn(sd + 1, S, Cs), spk=spk, bstride=bs, dcond=randn(sd + 2, B * bs), dtable0=randn(sd + 3, S, Cs))


def _speaker_rows(spk, n_spk):
    spk = np.asarray(spk, np.int64).reshape(-1)
    return np.where((spk >= 0) & (spk < n_spk), spk, 0)      # an id outside the table reads row 0


def _speaker_pos(B, Cs, Tz, bstride, row0):
    b, j, t = np.arange(B)[:, None, None], np.arange(Cs)[None, :, None], np.arange(Tz)[None, None, :]
    return b * bstride + (row0 + j) * Tz + t


def speaker_fwd_ref(table, spk, cond0, cond_bstride, row0, B, Cs, Tz, n_spk):
    """cond[b*cond_bstride + (row0+j)*Tz + t] = table[spk[b]][j] for all t: a copy, bit-exact."""
    rows = np.asarray(table, F32).reshape(n_spk, Cs)[_speaker_rows(spk, n_spk)]
    return _out(cond0, _speaker_pos(B, Cs, Tz, cond_bstride, row0), np.broadcast_to(rows[:, :, None], (B, Cs, Tz)))


def speaker_bwd_ref(dcond, dcond_bstride, row0, spk, dtable0, B, Cs, Tz, n_spk):
    """dtable[spk[b]][j] += sum_t dcond[b][row0+j][t], onto the caller's dtable."""
    g = _f64(dcond).reshape(-1)[_speaker_pos(B, Cs, Tz, dcond_bstride, row0)]
    rows = _speaker_rows(spk, n_spk)
    v, s = _f64(dtable0).reshape(n_spk, Cs).copy(), np.abs(_f64(dtable0)).reshape(n_spk, Cs)
    np.add.at(v, rows, g.sum(-1))
    np.add.at(s, rows, np.abs(g).sum(-1))
    count = np.bincount(rows, minlength=n_spk)
    chosen = np.flatnonzero(count)
    pos = chosen[:, None] * Cs + np.arange(Cs)[None, :]
    return _out(dtable0, pos, v[chosen], (Tz + count[chosen, None] + 1) * U * s[chosen])


def speaker_bwd_emulation(dcond, dcond_bstride, row0, spk, dtable0, B, Cs, Tz, n_spk):
    g = np.asarray(dcond, F32).reshape(-1)[_speaker_pos(B, Cs, Tz, dcond_bstride, row0)]
    s = np.zeros((B, Cs), F32)
    for t in range(Tz):
        s = (s + g[:, :, t]).astype(F32)
    dt = np.asarray(dtable0, F32).reshape(n_spk, Cs).copy()
    np.add.at(dt, _speaker_rows(spk, n_spk), s)
    return dt


# ---------------------------------------------------------------------------------------------------- cond_proj
FWD_CC = (1, 2, 7, 8, 9, 16, 17, 33, 80, 128, 130)
FWD_MALL = (4, 36, 128, 132, 1000)
FWD_TZ = (1, 4, 127, 128, 129, 260)
FWD_B = (1, 3)
WGRAD_TZ = (4, 28, 32, 36, 64, 68, 132)
WGRAD_CC = (1, 31, 32, 33, 64, 65, 128)
WGRAD_MALL = (5, 36, 100, 129, 260)
WGRAD_B = (1, 2, 3, 5)
DGRAD_MALL = (4, 36, 256, 260, 1000)
DGRAD_TZ = (1, 31, 32, 33, 130)
DGRAD_B = (1, 2, 3)


def _pj(entry, B, Cc, Mall, Tz, cus=0):
    """cus None: Mall is taken from the device when the case runs (proj_resolve)."""
    name = 'b%d_cc%d_m%s_t%d' % (B, Cc, 'auto' if cus is None else str(Mall), Tz)
    return dict(entry=entry, name=name, B=B, Cc=Cc, Mall=Mall, Tz=Tz, cus=cus, family='proj')


def _draw(entry, n, axes, corners):
    """A seeded draw, not the full product: every value of every axis at least once (each axis a shuffled cycle), the corners
    by hand."""
    rng = np.random.RandomState(seed_of('proj_draw', entry))
    cols = []
    for values in axes:
        col = []
        while len(col) < n:
            col += list(rng.permutation(values))
        cols.append(col[:n])
    seen, out = set(), []
    for shape in corners + list(zip(*cols)):
        shape = tuple(int(v) for v in shape)
        if shape not in seen:
            seen.add(shape)
            out.append(_pj(entry, *shape))
    return out


def proj_fwd_cases():
    return _draw('fwd', 30, (FWD_B, FWD_CC, FWD_MALL, FWD_TZ),
                 [(1, 1, 4, 1), (3, 130, 1000, 260), (1, 128, 132, 129), (3, 7, 36, 127), (1, 2, 128, 128), (3, 80, 1000, 104)])


def proj_wgrad_cases():
    """The last two force KS = 1 with a batch loop longer than one: their Mall is the smallest at which the column tiles alone
    fill 8 * CUs, 32 * ceil(8 * CUs / ceil(Cc / 32)), computed from the device at run time."""
    return _draw('wgrad', 24, (WGRAD_B, WGRAD_CC, WGRAD_MALL, WGRAD_TZ),
                 [(1, 1, 5, 4), (5, 128, 260, 132), (2, 33, 129, 28), (3, 65, 36, 68)]) + [
        _pj('wgrad', 3, 128, 0, 4, cus=None), _pj('wgrad', 2, 128, 0, 4, cus=None)]


def proj_dgrad_cases():
    return _draw('dgrad', 24, (DGRAD_B, WGRAD_CC, DGRAD_MALL, DGRAD_TZ),
                 [(1, 1, 4, 1), (3, 128, 1000, 130), (2, 33, 260, 33), (1, 65, 36, 31)])


def proj_resolve(c, cus):
    """The case with its Mall: a case of cus = None gets 32 * ceil(8 * cus / ceil(Cc / 32))."""
    if c['cus'] is not None:
        return c
    return dict(c, Mall=32 * _cdiv(8 * cus, _cdiv(c['Cc'], 32)))


def proj_legal(c):
    """The header's preconditions: fwd none beyond positive sizes; wgrad Cc <= 128 and Tz % 4 == 0; dgrad Cc <= 128 and
    Mall % 4 == 0 (16-byte alignment of cond, dce and w: the test's to provide)."""
    ok = min(c['B'], c['Cc'], c['Mall'], c['Tz']) > 0
    if c['entry'] == 'wgrad':
        ok = ok and c['Cc'] <= 128 and c['Tz'] % 4 == 0
    if c['entry'] == 'dgrad':
        ok = ok and c['Cc'] <= 128 and c['Mall'] % 4 == 0
    return ok


def proj_wgrad_ks(c, cus):
    """Batch ranges of a wgrad launch: two when B >= 2 and the ceil(Mall/32) * ceil(Cc/32) tiles are fewer than 8 * CUs."""
    return 2 if (c['B'] >= 2 and _cdiv(c['Mall'], 32) * _cdiv(c['Cc'], 32) < 8 * cus) else 1


def proj_inputs(c):
    """Every operand of all three entries, plus the accumulator's contents before a wgrad call."""
    B, Cc, Mall, Tz = c['B'], c['Cc'], c['Mall'], c['Tz']
    sd = seed_of('proj', c['entry'], c['name'], Mall)
    return dict(cond=randn(sd, B, Cc, Tz), w=randn(sd + 1, Cc, Mall), dce=randn(sd + 2, B, Mall, Tz), dw0=randn(sd + 3, Cc, Mall))


def cond_proj_fwd_ref(cond, w, out0, B, Cc, Mall, Tz):
    """out[b][m][t] = sum_c w[c][m] cond[b][c][t]"""
    x, wt = _f64(cond).reshape(B, Cc, Tz), _f64(w).reshape(Cc, Mall).T
    v, s = np.matmul(wt[None], x), np.matmul(np.abs(wt)[None], np.abs(x))
    return _out(out0, np.arange(B * Mall * Tz), v, (Cc + 1) * U * s)


def cond_proj_wgrad_ref(cond, dce, dw0, B, Cc, Mall, Tz):
    """dw[c][m] += sum_{b,t} cond[b][c][t] dce[b][m][t], onto the caller's dw."""
    x, d = _f64(cond).reshape(B, Cc, Tz), _f64(dce).reshape(B, Mall, Tz)
    v = _f64(dw0).reshape(Cc, Mall) + np.matmul(x, d.transpose(0, 2, 1)).sum(0)
    s = np.abs(_f64(dw0)).reshape(Cc, Mall) + np.matmul(np.abs(x), np.abs(d).transpose(0, 2, 1)).sum(0)
    return _out(dw0, np.arange(Cc * Mall), v, (B * Tz + 2) * U * s)


def cond_proj_dgrad_ref(w, dce, dcond0, B, Cc, Mall, Tz):
    """dcond[b][c][t] = sum_m w[c][m] dce[b][m][t]"""
    wm, d = _f64(w).reshape(Cc, Mall), _f64(dce).reshape(B, Mall, Tz)
    v, s = np.matmul(wm[None], d), np.matmul(np.abs(wm)[None], np.abs(d))
    return _out(dcond0, np.arange(B * Cc * Tz), v, Mall * U * s)


def cond_proj_emulation(entry, ins, c):
    """Plain fp32: a sequential sum over the contraction index (b then t for wgrad, from the old contents), each product
    rounded once."""
    B, Cc, Mall, Tz = c['B'], c['Cc'], c['Mall'], c['Tz']
    x, w, d = ins['cond'].reshape(B, Cc, Tz), ins['w'].reshape(Cc, Mall), ins['dce'].reshape(B, Mall, Tz)
    if entry == 'fwd':
        acc = np.zeros((B, Mall, Tz), F32)
        for k in range(Cc):
            acc = (acc + (w[k][None, :, None] * x[:, k, None, :]).astype(F32)).astype(F32)
    elif entry == 'wgrad':
        acc = ins['dw0'].reshape(Cc, Mall).copy()
        for b in range(B):
            for t in range(Tz):
                acc = (acc + (x[b, :, t, None] * d[b, None, :, t]).astype(F32)).astype(F32)
    else:
        acc = np.zeros((B, Cc, Tz), F32)
        for m in range(Mall):
            acc = (acc + (w[None, :, m, None] * d[:, m, None, :]).astype(F32)).astype(F32)
    return acc


# ---------------------------------------------------------------------------------------------------- one door for all tables
def legality(c):
    """The header's preconditions of the case's entry (a projection case with its Mall resolved)."""
    return dict(vq_fwd=vq_fwd_legal, vq_bwd=vq_bwd_legal, speaker=speaker_legal, proj=proj_legal)[c['family']](c)


def path(c, cus):
    """The kernel path a case takes on a device of `cus` CUs: 'lds' or 'plain' backward kernel, 'ks1' or 'ks2' weight gradient;
    the entries with one kernel name it."""
    if c['family'] == 'vq_bwd':
        return vq_bwd_path(c)[0]
    if c['family'] == 'proj' and c['entry'] == 'wgrad':
        return 'ks%d' % proj_wgrad_ks(proj_resolve(c, cus), cus)
    return c.get('entry', c['family'])
