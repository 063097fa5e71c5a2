"""tests/cond_path_ref.py checked on the CPU: its references against what the project already trusts (torch in float64 --
einsum, index_add_, autograd of the straight-through estimator with its two loss terms -- oracle.ref_model.discretise and
oracle/vqw_oracle.c), the conditions its case tables rest on (legality under the header's preconditions, every kernel path
reached at 32, 256 and 304 CUs, every planted tie present), every bar against a plain fp32 emulation of its formula (at most
cond_path_ref.EMU_FRACTION of the bar), and the detection power of the cases: one deliberately wrong reference per mistake a
kernel could make, each of which must leave the right one by more than 4 bars, or by a bit where the comparison is exact.

WRONG is also the table a GPU run swaps in, one entry at a time, to see which of them the device cases catch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_path_ref as CR  # noqa: E402
from oracle import ref_model as M  # noqa: E402

F32 = np.float32
TOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
    assert err <= TOL, '%s: %.3e' % (what, err)


def _t64(a, grad=False):
    return torch.from_numpy(np.array(a, np.float64)).requires_grad_(grad)


def _ids(cases):
    return [c['name'] for c in cases]


def _sent(n):
    return np.full(n, CR.SENTINEL, F32)


def _proj_cases(cus=32):
    return [CR.proj_resolve(c, cus) for c in CR.proj_fwd_cases() + CR.proj_wgrad_cases() + CR.proj_dgrad_cases()]


def _proj_ref(c, ins):
    B, Cc, Mall, Tz = c['B'], c['Cc'], c['Mall'], c['Tz']
    if c['entry'] == 'fwd':
        return CR.cond_proj_fwd_ref(ins['cond'], ins['w'], _sent(B * Mall * Tz), B, Cc, Mall, Tz)
    if c['entry'] == 'wgrad':
        return CR.cond_proj_wgrad_ref(ins['cond'], ins['dce'], ins['dw0'], B, Cc, Mall, Tz)
    return CR.cond_proj_dgrad_ref(ins['w'], ins['dce'], _sent(B * Cc * Tz), B, Cc, Mall, Tz)


def _vq_fwd_ref(c, ins, variant=None):
    B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
    bs, with_ek, with_zq, with_mind = variant or CR.vq_fwd_variants(c)[0]
    return CR.vq_nearest_ref(ins['z'], ins['emb'], _sent(B * D * Tz) if with_ek else None,
                             _sent((B - 1) * (bs or D * Tz) + D * Tz) if with_zq else None, bs,
                             _sent(B * Tz) if with_mind else None, B, D, Tz, K)


def _vq_bwd_ref(c, ins):
    B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
    return CR.vq_bwd_ref(ins['z'], ins['e_k'], ins['idx'], ins['dzq'] if c['dzq'] else None, ins['dzq_bstride'],
                         _sent(B * D * Tz) if c['dz_e'] else None, ins['demb0'] if c['demb'] else None, ins['cscale'], ins['escale'],
                         B, D, Tz, K)


def _spk_refs(c, ins):
    B, Cs, Tz, S, row0, bs = c['B'], c['Cs'], c['Tz'], c['n_spk'], c['row0'], ins['bstride']
    return (CR.speaker_fwd_ref(ins['table'], ins['spk'], _sent(B * bs), bs, row0, B, Cs, Tz, S),
            CR.speaker_bwd_ref(ins['dcond'], bs, row0, ins['spk'], ins['dtable0'], B, Cs, Tz, S))


# ---------------------------------------------------------------------------------------------------- 1. the references
@pytest.mark.parametrize('c', _proj_cases()[::4], ids=['%s_%s' % (c['entry'], c['name']) for c in _proj_cases()[::4]])
def test_projection_references_are_torch_einsum(c):
    B, Cc, Mall, Tz = c['B'], c['Cc'], c['Mall'], c['Tz']
    ins = CR.proj_inputs(c)
    out = _proj_ref(c, ins)
    x, w, d = _t64(ins['cond']), _t64(ins['w']), _t64(ins['dce'])
    want = {'fwd': lambda: torch.einsum('cm,bct->bmt', w, x), 'dgrad': lambda: torch.einsum('cm,bmt->bct', w, d),
            'wgrad': lambda: _t64(ins['dw0']) + torch.einsum('bct,bmt->cm', x, d)}[c['entry']]()
    assert out.mask.all() and out.bar.shape == out.vals.shape
    _close(out.vals, want.numpy().reshape(-1), c['entry'])


@pytest.mark.parametrize('c', CR.vq_bwd_cases()[:-2], ids=_ids(CR.vq_bwd_cases()[:-2]))
def test_vq_backward_reference_is_autograd_of_the_straight_through_estimator(c):
    B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
    ins = CR.vq_bwd_inputs(c)
    out = _vq_bwd_ref(c, ins)
    z, idx = _t64(ins['z'], True), torch.from_numpy(ins['idx']).reshape(B, Tz)
    # the codebook whose rows idx picks: e_k where a frame chose the code, anything elsewhere
    emb = np.zeros((K, D))
    emb[ins['idx']] = CR.vq_rows(ins['e_k'], B, D, Tz)
    emb = _t64(emb, True)
    e_k = emb[idx].permute(0, 2, 1)                                          # [B][D][Tz]
    zq = z + (e_k - z).detach()
    g = np.zeros((B, D, Tz)) if not c['dzq'] else ins['dzq'].astype(np.float64)[CR.vq_pos(B, D, Tz, ins['dzq_bstride'])].reshape(
        B, Tz, D).transpose(0, 2, 1)
    loss = (zq * _t64(g)).sum() + 0.5 * ins['cscale'] * ((z - e_k.detach()) ** 2).sum() + 0.5 * ins['escale'] * ((z.detach() - e_k) ** 2).sum()
    loss.backward()
    if c['dz_e']:
        assert out['dz_e'].mask.all()
        _close(out['dz_e'].vals.reshape(B, D, Tz), z.grad.numpy(), 'dz_e')
    if c['demb']:
        want = _t64(ins['demb0']) + emb.grad
        _close(out['demb'].vals.reshape(K, D), want.numpy(), 'demb')
        want2 = _t64(ins['demb0']).index_add_(0, torch.from_numpy(ins['idx']), ins['escale'] * (_t64(CR.vq_rows(ins['e_k'], B, D, Tz)) - _t64(CR.vq_rows(ins['z'], B, D, Tz))))
        _close(out['demb'].vals.reshape(K, D), want2.numpy(), 'demb by index_add_')
        assert np.array_equal(out['demb'].mask.reshape(K, D).all(1), np.bincount(ins['idx'], minlength=K) > 0)
        assert np.array_equal(out['demb'].mask.reshape(K, D).any(1), out['demb'].mask.reshape(K, D).all(1))


@pytest.mark.parametrize('c', CR.speaker_cases(), ids=_ids(CR.speaker_cases()))
def test_speaker_references_are_torch_gather_and_index_add(c):
    B, Cs, Tz, S, row0 = c['B'], c['Cs'], c['Tz'], c['n_spk'], c['row0']
    ins = CR.speaker_inputs(c)
    fwd, bwd = _spk_refs(c, ins)
    rows = torch.from_numpy(np.where((ins['spk'] >= 0) & (ins['spk'] < S), ins['spk'], 0))
    width = ins['bstride'] // Tz
    want = torch.full((B, width, Tz), float(CR.SENTINEL), dtype=torch.float64)
    want[:, row0:row0 + Cs] = _t64(ins['table'])[rows][:, :, None]
    assert np.array_equal(fwd.vals.astype(F32), want.numpy().astype(F32).reshape(-1)) and fwd.bar is None
    assert int(fwd.mask.sum()) == B * Cs * Tz
    g = _t64(ins['dcond']).reshape(B, width, Tz)[:, row0:row0 + Cs].sum(-1)
    wantb = _t64(ins['dtable0']).index_add_(0, rows, g)
    _close(bwd.vals.reshape(S, Cs), wantb.numpy(), 'dtable')
    assert np.array_equal(bwd.mask.reshape(S, Cs).all(1), np.bincount(rows.numpy(), minlength=S) > 0)


@pytest.mark.parametrize('c', CR.vq_fwd_cases(), ids=_ids(CR.vq_fwd_cases()))
def test_vq_nearest_reference_is_discretise_and_the_c_oracle_bit_for_bit(c):
    B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
    ins = CR.vq_fwd_inputs(c)
    ref = _vq_fwd_ref(c, ins, (0, True, True, True))
    rows = CR.vq_rows(ins['z'], B, D, Tz)
    to_rows = lambda o: o.vals.astype(F32).reshape(B, D, Tz).transpose(0, 2, 1).reshape(B * Tz, D)  # noqa: E731
    with np.errstate(all='ignore'):
        q, e_k, z_q = M.discretise(torch.from_numpy(rows), torch.from_numpy(ins['emb']))
    assert np.array_equal(ref['idx'], q.numpy())
    assert np.array_equal(to_rows(ref['e_k']), e_k.numpy()) and np.array_equal(to_rows(ref['zq']), z_q.numpy(), equal_nan=True)
    oi, oe, oz, om = CR.oracle_vq_nearest(rows, ins['emb'])
    assert np.array_equal(ref['idx'], oi) and np.array_equal(to_rows(ref['e_k']), oe)
    assert np.array_equal(to_rows(ref['zq']), oz, equal_nan=True)
    assert np.array_equal(ref['mind'].vals.astype(F32).view(np.uint32), om.view(np.uint32))
    if c['nonfinite']:                                     # what the header now states: code 0 at +inf, for NaN and overflow alike
        for r in (ins['nan_row'], ins['inf_row']):
            assert oi[r] == 0 and om[r] == np.inf
        assert np.isnan(oz[ins['nan_row']]).sum() == 1 and np.isfinite(oz[ins['inf_row']]).all()
    # the wide layout moves zq and nothing else
    wide = _vq_fwd_ref(c, ins)
    bs = (D + 16) * Tz
    assert np.array_equal(wide['zq'].vals[CR.vq_pos(B, D, Tz, bs)].astype(F32), to_rows(ref['zq']), equal_nan=True)
    assert int(wide['zq'].mask.sum()) == B * D * Tz and wide['zq'].vals.size == (B - 1) * bs + D * Tz


# ---------------------------------------------------------------------------------------------------- 2. legality and reach
def test_every_case_is_legal():
    assert all(CR.vq_fwd_legal(c) for c in CR.vq_fwd_cases())
    assert all(CR.vq_bwd_legal(c) for c in CR.vq_bwd_cases())
    assert all(CR.speaker_legal(c) for c in CR.speaker_cases())
    for cus in CR.CUS:
        assert all(CR.proj_legal(c) for c in _proj_cases(cus))
    every = CR.vq_fwd_cases() + CR.vq_bwd_cases() + CR.speaker_cases() + [c for cus in CR.CUS for c in _proj_cases(cus)]
    assert all(CR.legality(c) for c in every)
    for cus in CR.CUS:
        assert {CR.path(c, cus) for c in every} == {'vq_fwd', 'lds', 'plain', 'speaker', 'fwd', 'ks1', 'ks2', 'dgrad'}
    for cases in (CR.vq_fwd_cases(), CR.vq_bwd_cases(), CR.speaker_cases(), CR.proj_fwd_cases(), CR.proj_wgrad_cases(), CR.proj_dgrad_cases()):
        assert len(set(_ids(cases))) == len(cases)


def test_the_tables_hold_every_value_the_issue_names():
    for cases, axes in ((CR.proj_fwd_cases(), dict(B=CR.FWD_B, Cc=CR.FWD_CC, Mall=CR.FWD_MALL, Tz=CR.FWD_TZ)),
                        (CR.proj_wgrad_cases()[:-2], dict(B=CR.WGRAD_B, Cc=CR.WGRAD_CC, Mall=CR.WGRAD_MALL, Tz=CR.WGRAD_TZ)),
                        (CR.proj_dgrad_cases(), dict(B=CR.DGRAD_B, Cc=CR.WGRAD_CC, Mall=CR.DGRAD_MALL, Tz=CR.DGRAD_TZ))):
        for axis, values in axes.items():
            assert {c[axis] for c in cases} >= set(values), axis       # (the hand-made corners add the benchmark's Tz = 104)
    assert {c['B'] * c['Cs'] for c in CR.speaker_cases()} >= {1, 256, 257, 400}
    assert {c['row0'] for c in CR.speaker_cases()} >= {0, 64} and {c['Tz'] for c in CR.speaker_cases()} >= {1}
    assert any(c['B'] * c['Cs'] * c['Tz'] > CR.GRID_PASS for c in CR.speaker_cases())
    assert any((c['B'] * c['Tz']) % 4 for c in CR.vq_fwd_cases())


def test_every_kernel_path_is_reached():
    paths = {CR.vq_bwd_path(c) for c in CR.vq_bwd_cases()}
    assert paths == {('lds', False), ('lds', True), ('plain', False), ('plain', True)}
    by = {(c['K'], c['D']): CR.vq_bwd_path(c)[0] for c in CR.vq_bwd_cases() if c['demb'] and c['dz_e'] and c['dzq']}
    assert by[(576, 64)] == 'lds' and 576 * 64 * 4 == CR.VQ_LDS_BYTES and by[(577, 64)] == 'plain'
    assert any(CR.vq_bwd_path(c)[0] == 'plain' and c['K'] * c['D'] * 4 <= CR.VQ_LDS_BYTES for c in CR.vq_bwd_cases())   # demb absent
    assert {c['codes'] for c in CR.vq_bwd_cases()} == {'nearest', 'one', 'all', 'rand'}
    for path in ('lds', 'plain'):
        assert any(CR.vq_bwd_path(c)[0] == path and c['codes'] == 'one' for c in CR.vq_bwd_cases())
    for cus in CR.CUS:
        got = set()
        for c in CR.proj_wgrad_cases():
            r = CR.proj_resolve(c, cus)
            got.add((CR.proj_wgrad_ks(r, cus), r['B'] > 1, r['B'] % 2 == 1))
            if c['cus'] is None:                     # the formula: the smallest Mall whose tiles alone fill 8 * CUs
                assert CR.proj_wgrad_ks(r, cus) == 1 and r['B'] > 1
                assert CR.proj_wgrad_ks(dict(r, Mall=r['Mall'] - 32), cus) == 2
        assert (1, True, True) in got and (1, True, False) in got and (2, True, True) in got and (2, True, False) in got
        assert (1, False, True) in got


def test_every_tie_is_planted_and_is_a_tie():
    seen = set()
    for c in CR.vq_fwd_cases():
        ins = CR.vq_fwd_inputs(c)
        rows = CR.vq_rows(ins['z'], c['B'], c['D'], c['Tz'])
        idx = _vq_fwd_ref(c, ins)['idx']
        dist = M.vq_distances_np(rows[[p[1] for p in ins['plants']]], ins['emb']) if ins['plants'] else []
        for (kind, row, codes, winner), d in zip(ins['plants'], dist):
            seen.add(kind)
            assert idx[row] == winner and d[winner] == 0.0
            assert sorted(np.flatnonzero(d == 0.0)) == sorted(codes), (c['name'], kind)
            a, b = codes[0], codes[-1]
            if kind == 'same_lane':
                assert b == a + 64
            if kind.startswith('xor'):
                assert a ^ b == 1 << int(kind[3:]) and (a % 64) ^ (b % 64) == 1 << int(kind[3:])
            if kind == 'adjacent':
                assert b == a + 1 and a ^ b != 1
            if kind == 'with_0':
                assert a == 0
            if kind in ('with_last', 'winner_last'):
                assert b == c['K'] - 1
    assert seen == set(CR.VQ_PLANTS)


# ---------------------------------------------------------------------------------------------------- 3. emulation headroom
def _headroom(emu, out, what):
    m = out.mask
    r = CR.ratio_of(np.asarray(emu, F32).reshape(-1)[m] if np.size(emu) == m.size else emu, out.vals[m], out.bar[m], what)
    assert r <= CR.EMU_FRACTION, '%s: the fp32 emulation of the formula reaches %.2f of its bar' % (what, r)
    return r


@pytest.mark.parametrize('c', _proj_cases(), ids=['%s_%s' % (c['entry'], c['name']) for c in _proj_cases()])
def test_projection_bars_leave_the_fp32_emulation_headroom(c):
    ins = CR.proj_inputs(c)
    _headroom(CR.cond_proj_emulation(c['entry'], ins, c), _proj_ref(c, ins), c['entry'] + ' ' + c['name'])


@pytest.mark.parametrize('c', CR.vq_bwd_cases(), ids=_ids(CR.vq_bwd_cases()))
def test_vq_backward_bars_leave_the_fp32_emulation_headroom(c):
    B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
    ins = CR.vq_bwd_inputs(c)
    out = _vq_bwd_ref(c, ins)
    dz, demb = CR.vq_bwd_emulation(ins['z'], ins['e_k'], ins['idx'], ins['dzq'] if c['dzq'] else None, ins['dzq_bstride'], ins['demb0'],
                                   ins['cscale'], ins['escale'], B, D, Tz, K)
    if c['dz_e']:
        _headroom(dz.reshape(B, Tz, D).transpose(0, 2, 1), out['dz_e'], 'dz_e ' + c['name'])
    if c['demb']:
        _headroom(demb, out['demb'], 'demb ' + c['name'])


@pytest.mark.parametrize('c', CR.speaker_cases(), ids=_ids(CR.speaker_cases()))
def test_speaker_backward_bar_leaves_the_fp32_emulation_headroom(c):
    ins = CR.speaker_inputs(c)
    bwd = _spk_refs(c, ins)[1]
    emu = CR.speaker_bwd_emulation(ins['dcond'], ins['bstride'], c['row0'], ins['spk'], ins['dtable0'], c['B'], c['Cs'], c['Tz'], c['n_spk'])
    _headroom(emu, bwd, 'dtable ' + c['name'])


# ---------------------------------------------------------------------------------------------------- 4. detection power
def _moved(out, delta):
    """out with delta added to its written values (same mask, same bar)."""
    v = out.vals.copy()
    v[out.mask] += np.asarray(delta, np.float64).reshape(-1)
    return CR.Out(v, out.mask, out.bar)


_right = {n: getattr(CR, n) for n in ('cond_proj_fwd_ref', 'cond_proj_wgrad_ref', 'cond_proj_dgrad_ref', 'vq_nearest_ref', 'vq_bwd_ref',
                                      'speaker_fwd_ref', 'speaker_bwd_ref')}


def fwd_last_c_dropped(cond, w, out0, B, Cc, Mall, Tz):
    x, wm = np.asarray(cond, np.float64).reshape(B, Cc, Tz), np.asarray(w, np.float64).reshape(Cc, Mall)
    return _moved(_right['cond_proj_fwd_ref'](cond, w, out0, B, Cc, Mall, Tz), -wm[Cc - 1][None, :, None] * x[:, Cc - 1, None, :])


def _wgrad_minus(frames):
    def wrong(cond, dce, dw0, B, Cc, Mall, Tz):
        x, d = np.asarray(cond, np.float64).reshape(B, Cc, Tz), np.asarray(dce, np.float64).reshape(B, Mall, Tz)
        keep = frames(B, Tz)
        return _moved(_right['cond_proj_wgrad_ref'](cond, dce, dw0, B, Cc, Mall, Tz), -np.einsum('bct,bmt,bt->cm', x, d, keep))
    return wrong


wgrad_last_frame_dropped = _wgrad_minus(lambda B, Tz: (np.arange(Tz)[None, :] == Tz - 1) * np.ones((B, 1)))
wgrad_second_range_dropped = _wgrad_minus(lambda B, Tz: ((np.arange(B)[:, None] >= B // 2) & (B >= 2)) * np.ones((1, Tz)))


def wgrad_overwrites(cond, dce, dw0, B, Cc, Mall, Tz):
    return _moved(_right['cond_proj_wgrad_ref'](cond, dce, dw0, B, Cc, Mall, Tz), -np.asarray(dw0, np.float64))


def dgrad_last_of_eight_dropped(w, dce, dcond0, B, Cc, Mall, Tz):
    wm, d = np.asarray(w, np.float64).reshape(Cc, Mall), np.asarray(dce, np.float64).reshape(B, Mall, Tz)
    sel = np.arange(Mall) % 8 == 7
    return _moved(_right['cond_proj_dgrad_ref'](w, dce, dcond0, B, Cc, Mall, Tz), -np.matmul(wm[None, :, sel], d[:, sel]))


def dgrad_sums_past_the_row(w, dce, dcond0, B, Cc, Mall, Tz):
    """m runs to Mall rounded up to 8: w reads into its next row, dce into the next batch row (zero behind either buffer)."""
    wf = np.concatenate([np.asarray(w, np.float64).reshape(-1), np.zeros(8)])
    df = np.concatenate([np.asarray(dce, np.float64).reshape(-1), np.zeros(8 * Tz)])
    extra = np.zeros((B, Cc, Tz))
    for m in range(Mall, -(-Mall // 8) * 8):
        wv = wf[np.arange(Cc) * Mall + m]
        dv = df[(np.arange(B)[:, None] * Mall + m) * Tz + np.arange(Tz)[None, :]]
        extra += wv[None, :, None] * dv[:, None, :]
    return _moved(_right['cond_proj_dgrad_ref'](w, dce, dcond0, B, Cc, Mall, Tz), extra)


def _vq_with(dist_fn=M.vq_distances_np, last=False, zq_is_ek=False):
    def wrong(z_e, emb, e_k0, zq0, zq_bstride, mind0, B, D, Tz, K):
        rows, e = CR.vq_rows(z_e, B, D, Tz), np.asarray(emb, F32).reshape(K, D)
        with np.errstate(all='ignore'):
            dist = dist_fn(rows, e)
            dist = np.where(dist < np.inf, dist, F32(np.inf))
            idx = (K - 1 - np.argmin(dist[:, ::-1], axis=1) if last else np.argmin(dist, axis=1)).astype(np.int64)
            idx = np.where(np.isinf(dist.min(1)), 0, idx)
            ek = e[idx]
            zq = ek if zq_is_ek else (rows + (ek - rows).astype(F32)).astype(F32)
        out = _right['vq_nearest_ref'](z_e, emb, e_k0, zq0, zq_bstride, mind0, B, D, Tz, K)
        res = dict(idx=idx)
        for name, vals, pos in (('e_k', ek, CR.vq_pos(B, D, Tz, D * Tz)), ('zq', zq, CR.vq_pos(B, D, Tz, zq_bstride or D * Tz)),
                                ('mind', dist.min(1), np.arange(B * Tz))):
            res[name] = None if out[name] is None else CR._out(out[name].vals, pos, vals)
        return res
    return wrong


def _fma_distances(rows, emb):
    acc = np.zeros((rows.shape[0], emb.shape[0]), F32)
    for d in range(rows.shape[1]):
        diff = (rows[:, None, d] - emb[None, :, d]).astype(F32).astype(np.float64)
        acc = (acc.astype(np.float64) + diff * diff).astype(F32)                     # the product is not rounded
    return acc


vq_highest_index_on_ties = _vq_with(last=True)
vq_fma_contracted_distance = _vq_with(dist_fn=_fma_distances)
vq_zq_is_e_k = _vq_with(zq_is_ek=True)


def demb_sign_flipped(z_e, e_k, idx, dzq, dzq_bstride, dz_e0, demb0, cscale, escale, B, D, Tz, K):
    out = _right['vq_bwd_ref'](z_e, e_k, idx, dzq, dzq_bstride, dz_e0, demb0, cscale, escale, B, D, Tz, K)
    if out['demb'] is not None:
        flipped = _right['vq_bwd_ref'](z_e, e_k, idx, dzq, dzq_bstride, None, demb0, cscale, -escale, B, D, Tz, K)['demb']
        out['demb'] = CR.Out(flipped.vals, flipped.mask, out['demb'].bar)
    return out


def demb_last_block_missing(z_e, e_k, idx, dzq, dzq_bstride, dz_e0, demb0, cscale, escale, B, D, Tz, K):
    """The elements of the last 256-thread block of the flat [B][D][Tz] range never reach demb."""
    out = _right['vq_bwd_ref'](z_e, e_k, idx, dzq, dzq_bstride, dz_e0, demb0, cscale, escale, B, D, Tz, K)
    if out['demb'] is not None:
        n = B * D * Tz
        lost = np.arange(n) >= (n - 1) // 256 * 256
        z, e = np.asarray(z_e, np.float64).reshape(-1), np.asarray(e_k, np.float64).reshape(-1)
        a = np.where(lost, escale * (e - z), 0.0).reshape(B, D, Tz).transpose(0, 2, 1).reshape(B * Tz, D)
        v = out['demb'].vals.reshape(K, D).copy()
        np.subtract.at(v, np.asarray(idx).reshape(-1), a)
        out['demb'] = CR.Out(v.reshape(-1), out['demb'].mask, out['demb'].bar)
    return out


def _clamped(spk, n_spk):
    return np.clip(np.asarray(spk, np.int64), 0, n_spk - 1)       # -1 still reads row 0, n_speakers the last row


def speaker_fwd_id_clamped(table, spk, cond0, cond_bstride, row0, B, Cs, Tz, n_spk):
    return _right['speaker_fwd_ref'](table, _clamped(spk, n_spk), cond0, cond_bstride, row0, B, Cs, Tz, n_spk)


def speaker_bwd_id_clamped(dcond, dcond_bstride, row0, spk, dtable0, B, Cs, Tz, n_spk):
    return _right['speaker_bwd_ref'](dcond, dcond_bstride, row0, _clamped(spk, n_spk), dtable0, B, Cs, Tz, n_spk)


def speaker_fwd_row0_ignored(table, spk, cond0, cond_bstride, row0, B, Cs, Tz, n_spk):
    return _right['speaker_fwd_ref'](table, spk, cond0, cond_bstride, 0, B, Cs, Tz, n_spk)


def speaker_bwd_row0_ignored(dcond, dcond_bstride, row0, spk, dtable0, B, Cs, Tz, n_spk):
    return _right['speaker_bwd_ref'](dcond, dcond_bstride, 0, spk, dtable0, B, Cs, Tz, n_spk)


# name -> (family, the reference it stands in for, the wrong reference)
WRONG = {
    'fwd_last_c_dropped': ('proj', 'cond_proj_fwd_ref', fwd_last_c_dropped),
    'wgrad_last_frame_dropped': ('proj', 'cond_proj_wgrad_ref', wgrad_last_frame_dropped),
    'wgrad_second_range_dropped': ('proj', 'cond_proj_wgrad_ref', wgrad_second_range_dropped),
    'wgrad_overwrites': ('proj', 'cond_proj_wgrad_ref', wgrad_overwrites),
    'dgrad_last_of_eight_dropped': ('proj', 'cond_proj_dgrad_ref', dgrad_last_of_eight_dropped),
    'dgrad_sums_past_the_row': ('proj', 'cond_proj_dgrad_ref', dgrad_sums_past_the_row),
    'vq_highest_index_on_ties': ('vq_fwd', 'vq_nearest_ref', vq_highest_index_on_ties),
    'vq_fma_contracted_distance': ('vq_fwd', 'vq_nearest_ref', vq_fma_contracted_distance),
    'vq_zq_is_e_k': ('vq_fwd', 'vq_nearest_ref', vq_zq_is_e_k),
    'demb_sign_flipped': ('vq_bwd', 'vq_bwd_ref', demb_sign_flipped),
    'demb_last_block_missing': ('vq_bwd', 'vq_bwd_ref', demb_last_block_missing),
    'speaker_fwd_id_clamped': ('speaker', 'speaker_fwd_ref', speaker_fwd_id_clamped),
    'speaker_bwd_id_clamped': ('speaker', 'speaker_bwd_ref', speaker_bwd_id_clamped),
    'speaker_fwd_row0_ignored': ('speaker', 'speaker_fwd_ref', speaker_fwd_row0_ignored),
    'speaker_bwd_row0_ignored': ('speaker', 'speaker_bwd_ref', speaker_bwd_row0_ignored),
}


def _bars_apart(right, wrong):
    """The largest distance of two expectations of one output in bars of the right one; inf for a bit where it is exact or
    for a position only one of them writes."""
    if right is None:
        return 0.0
    if isinstance(right, np.ndarray):
        return np.inf if not np.array_equal(right, wrong) else 0.0
    if not np.array_equal(right.mask, wrong.mask):
        return np.inf
    a, b = right.vals[right.mask], wrong.vals[right.mask]
    if right.bar is None:
        same = (a.astype(F32).view(np.uint32) == b.astype(F32).view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        return 0.0 if same.all() else np.inf
    d = np.abs(a - b)
    return float(np.max(np.where(d == 0, 0.0, d / np.maximum(right.bar[right.mask], 1e-300)), initial=0.0))


def _family_calls(family):
    """Every (case name, reference name, arguments) a family's table makes."""
    if family == 'proj':
        for c in _proj_cases():
            ins = CR.proj_inputs(c)
            B, Cc, Mall, Tz = c['B'], c['Cc'], c['Mall'], c['Tz']
            args = dict(fwd=(ins['cond'], ins['w'], _sent(B * Mall * Tz)), wgrad=(ins['cond'], ins['dce'], ins['dw0']),
                        dgrad=(ins['w'], ins['dce'], _sent(B * Cc * Tz)))[c['entry']]
            yield c['name'], 'cond_proj_%s_ref' % c['entry'], args + (B, Cc, Mall, Tz)
    elif family == 'vq_fwd':
        for c in CR.vq_fwd_cases()[:-1]:
            ins = CR.vq_fwd_inputs(c)
            B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
            yield c['name'], 'vq_nearest_ref', (ins['z'], ins['emb'], _sent(B * D * Tz), _sent(B * D * Tz), 0, _sent(B * Tz), B, D, Tz, K)
    elif family == 'vq_bwd':
        for c in CR.vq_bwd_cases()[:-2]:
            ins = CR.vq_bwd_inputs(c)
            B, Tz, D, K = c['B'], c['Tz'], c['D'], c['K']
            yield c['name'], 'vq_bwd_ref', (ins['z'], ins['e_k'], ins['idx'], ins['dzq'] if c['dzq'] else None, ins['dzq_bstride'],
                                            _sent(B * D * Tz) if c['dz_e'] else None, ins['demb0'] if c['demb'] else None,
                                            ins['cscale'], ins['escale'], B, D, Tz, K)
    else:
        for c in CR.speaker_cases()[:-1]:
            ins = CR.speaker_inputs(c)
            B, Cs, Tz, S, row0, bs = c['B'], c['Cs'], c['Tz'], c['n_spk'], c['row0'], ins['bstride']
            yield c['name'], 'speaker_fwd_ref', (ins['table'], ins['spk'], _sent(B * bs), bs, row0, B, Cs, Tz, S)
            yield c['name'], 'speaker_bwd_ref', (ins['dcond'], bs, row0, ins['spk'], ins['dtable0'], B, Cs, Tz, S)


@pytest.mark.parametrize('family', ('proj', 'vq_fwd', 'vq_bwd', 'speaker'))
def test_a_wrong_reference_is_more_than_four_bars_from_the_right_one(family):
    worst = {name: 0.0 for name, (fam, _, _) in WRONG.items() if fam == family}
    assert worst
    for case, ref_name, args in _family_calls(family):
        right = None
        for name in worst:
            _, stands_for, fn = WRONG[name]
            if stands_for != ref_name or worst[name] == np.inf:
                continue
            right = _right[ref_name](*args) if right is None else right
            wrong = fn(*args)
            pairs = [(right[k], wrong[k]) for k in right] if isinstance(right, dict) else [(right, wrong)]
            worst[name] = max([worst[name]] + [_bars_apart(r, w) for r, w in pairs])
    for name, r in worst.items():
        assert r > 4.0, '%s: the cases tell it from the right reference by %.2f bars at most' % (name, r)
