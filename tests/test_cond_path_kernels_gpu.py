"""The kernels between the encoder and the decoder -- vqw_vq_nearest_fwd / _bwd and the speaker tile of csrc/vq.hip, the three
projections of csrc/cond_proj.hip -- against the exact and float64 references of tests/cond_path_ref.py, through kernels.py, at
the smallest shapes that reach each loop, shuffle stage, kernel path and tile edge.

Every output is a view into a sentinel-filled buffer with guards on both sides; cond_path_ref.compare holds the written
positions to the case's expectation -- bit-equality for the VQ and speaker forward passes, an elementwise bar in units of 2^-24
for everything that sums -- and every other element (guards, the gap of a wider batch stride, table rows no frame chose) to
bit-equality.  A refusal must raise and leave its outputs' bits alone.

Every test records err / bar of its case (record_property 'err_over_bar', with 'family'); DESIGN 6 lists the maxima."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_path_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
IGUARD = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_off(a, off):
    """A device copy of `a` whose first element lies `off` floats past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    full = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
    v = full[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


class DBuf:
    """The device twin of a conv_ref.Buf: `view` is what the kernel gets, host() the whole buffer read back."""

    def __init__(self, n, off=0, init=None):
        self.buf = CR.Buf(n, off, init)
        self.full = _dev(self.buf.full)
        self.view = self.full[self.buf.lo:self.buf.lo + n]

    def host(self):
        return self.full.cpu().numpy()

    def check(self, out, what):
        return CR.compare(self.host(), self.buf, out, what)

    def untouched(self, what):
        return self.check(CR.Out(self.buf.view.astype(np.float64), np.zeros(self.buf.n, dtype=bool), None), what)


class IBuf:
    """int64 indices between guards."""

    def __init__(self, n):
        self.n = n
        self.full = torch.full((CR.GUARD + n + CR.GUARD,), IGUARD, dtype=torch.int64, device=DEV)
        self.view = self.full[CR.GUARD:CR.GUARD + n]

    def check(self, want, what):
        got = self.full.cpu().numpy()
        assert (got[:CR.GUARD] == IGUARD).all() and (got[CR.GUARD + self.n:] == IGUARD).all(), what + ': an idx guard changed'
        bad = np.flatnonzero(got[CR.GUARD:CR.GUARD + self.n] != want)
        assert bad.size == 0, '%s: %d indices differ (first: row %d, got %d, want %d)' % (
            what, bad.size, bad[0], got[CR.GUARD + bad[0]], want[bad[0]])


def _ids(cases):
    return [c['name'] for c in cases]


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ---------------------------------------------------------------------------------------------------- vq_nearest_fwd
@pytest.mark.parametrize('c', CR.vq_fwd_cases(), ids=_ids(CR.vq_fwd_cases()))
def test_vq_nearest_fwd_is_bit_exact(K, record_property, c):
    B, Tz, D, Kc = c['B'], c['Tz'], c['D'], c['K']
    ins = CR.vq_fwd_inputs(c)
    dz, demb = _dev(ins['z']), _dev(ins['emb'])
    for bs, with_ek, with_zq, with_mind in CR.vq_fwd_variants(c):
        what = 'vq_nearest_fwd %s zq_bstride=%d e_k=%d zq=%d mind=%d' % (c['name'], bs, with_ek, with_zq, with_mind)
        idx = IBuf(B * Tz)
        ek = DBuf(B * D * Tz) if with_ek else None
        zq = DBuf((B - 1) * (bs or D * Tz) + D * Tz) if with_zq else None
        mind = DBuf(B * Tz) if with_mind else None
        ref = CR.vq_nearest_ref(ins['z'], ins['emb'], ek and ek.buf.view, zq and zq.buf.view, bs, mind and mind.buf.view, B, D, Tz, Kc)
        K.vq_nearest_fwd(dz, demb, idx=idx.view.view(B, Tz), e_k=ek and ek.view, zq=zq and zq.view, zq_bstride=bs, mind=mind and mind.view)
        idx.check(ref['idx'], what + ' idx')
        for name, buf in (('e_k', ek), ('zq', zq), ('mind', mind)):
            if buf is not None:
                buf.check(ref[name], what + ' ' + name)
        got = idx.view.cpu().numpy()
        for kind, row, codes, winner in ins['plants']:
            assert got[row] == winner, '%s: planted tie %s of codes %r in row %d went to %d' % (what, kind, codes, row, got[row])
        if c['nonfinite'] and with_ek and with_zq and with_mind and bs == 0:
            # a row with a NaN and a row whose every distance overflows: what oracle/vqw_oracle.c returns, code 0 at +inf
            sel = [ins['nan_row'], ins['inf_row']]
            oi, oe, oz, om = CR.oracle_vq_nearest(CR.vq_rows(ins['z'], B, D, Tz)[sel], ins['emb'])
            rows_of = lambda b: CR.vq_rows(b.view.cpu().numpy(), B, D, Tz)[sel]  # noqa: E731
            assert np.array_equal(got[sel], oi) and np.array_equal(got[sel], [0, 0])
            assert np.array_equal(rows_of(ek), oe) and np.array_equal(rows_of(zq), oz, equal_nan=True)
            assert np.array_equal(mind.view.cpu().numpy()[sel], om) and np.isinf(om).all()
    record_property('family', 'vq_nearest_fwd')
    record_property('err_over_bar', 0.0)


# ---------------------------------------------------------------------------------------------------- vq_nearest_bwd
@pytest.mark.parametrize('c', CR.vq_bwd_cases(), ids=_ids(CR.vq_bwd_cases()))
def test_vq_nearest_bwd_matches_float64_reference(K, record_property, c):
    B, Tz, D, Kc = c['B'], c['Tz'], c['D'], c['K']
    ins = CR.vq_bwd_inputs(c)
    path, second_pass = CR.vq_bwd_path(c)
    what = 'vq_nearest_bwd %s (%s kernel%s)' % (c['name'], path, ', two passes' if second_pass else '')
    dz = DBuf(B * D * Tz) if c['dz_e'] else None
    de = DBuf(Kc * D, init=ins['demb0']) if c['demb'] else None
    dzq = ins['dzq'] if c['dzq'] else None
    ref = CR.vq_bwd_ref(ins['z'], ins['e_k'], ins['idx'], dzq, ins['dzq_bstride'], dz and dz.buf.view, de and de.buf.view.copy(),
                        ins['cscale'], ins['escale'], B, D, Tz, Kc)
    K.vq_nearest_bwd(_dev(ins['z']), _dev(ins['e_k']), _dev(ins['idx']).view(B, Tz), dzq=None if dzq is None else _dev(dzq),
                     dzq_bstride=ins['dzq_bstride'], dz_e=dz and dz.view.view(B, D, Tz), demb=de and de.view,
                     cscale=ins['cscale'], escale=ins['escale'], K=Kc)
    r_dz = dz.check(ref['dz_e'], what + ' dz_e') if dz else 0.0
    r_de = de.check(ref['demb'], what + ' demb') if de else 0.0
    record_property('family', 'vq_nearest_bwd')
    record_property('err_over_bar', max(r_dz, r_de))
    record_property('err_over_bar_dz_e', r_dz)
    record_property('err_over_bar_demb', r_de)


# ---------------------------------------------------------------------------------------------------- speaker tile
@pytest.mark.parametrize('c', CR.speaker_cases(), ids=_ids(CR.speaker_cases()))
def test_speaker_tile_matches_references(K, record_property, c):
    B, Cs, Tz, S, row0 = c['B'], c['Cs'], c['Tz'], c['n_spk'], c['row0']
    ins = CR.speaker_inputs(c)
    bs, spk = ins['bstride'], _dev(ins['spk'])
    what = 'speaker_tile %s' % c['name']
    cond = DBuf(B * bs)
    ref = CR.speaker_fwd_ref(ins['table'], ins['spk'], cond.buf.view, bs, row0, B, Cs, Tz, S)
    K.speaker_tile_fwd(_dev(ins['table']), spk, cond.view, cond_bstride=bs, row0=row0, Cs=Cs, Tz=Tz)
    cond.check(ref, what + ' fwd')
    dt = DBuf(S * Cs, init=ins['dtable0'])
    refb = CR.speaker_bwd_ref(ins['dcond'], bs, row0, ins['spk'], dt.buf.view.copy(), B, Cs, Tz, S)
    K.speaker_tile_bwd(_dev(ins['dcond']), spk, dt.view.view(S, Cs), dcond_bstride=bs, row0=row0, Cs=Cs, Tz=Tz)
    r = dt.check(refb, what + ' bwd')
    record_property('family', 'speaker_tile_bwd')
    record_property('err_over_bar', r)


# ---------------------------------------------------------------------------------------------------- cond_proj
def _proj_params():
    cases = CR.proj_fwd_cases() + CR.proj_wgrad_cases() + CR.proj_dgrad_cases()
    return dict(argnames='c', argvalues=cases, ids=['%s_%s' % (c['entry'], c['name']) for c in cases])


@pytest.mark.parametrize(**_proj_params())
def test_cond_proj_matches_float64_reference(K, record_property, c):
    cus = _cus()
    c = CR.proj_resolve(c, cus)
    B, Cc, Mall, Tz, entry = c['B'], c['Cc'], c['Mall'], c['Tz'], c['entry']
    assert CR.proj_legal(c)
    ins = CR.proj_inputs(c)
    dims = dict(B=B, Cc=Cc, Mall=Mall, Tz=Tz)
    what = 'cond_proj_%s %s' % (entry, c['name'])
    if entry == 'fwd':
        bufs = [DBuf(B * Mall * Tz), DBuf(B * Mall * Tz)]
        ref = CR.cond_proj_fwd_ref(ins['cond'], ins['w'], bufs[0].buf.view, B, Cc, Mall, Tz)
        for o in bufs:
            K.cond_proj_fwd(_dev(ins['cond']), _dev(ins['w']), o.view, **dims)
    elif entry == 'wgrad':
        what += ' (KS = %d at %d CUs)' % (CR.proj_wgrad_ks(c, cus), cus)
        bufs = [DBuf(Cc * Mall, init=ins['dw0'])]
        ref = CR.cond_proj_wgrad_ref(ins['cond'], ins['dce'], bufs[0].buf.view.copy(), B, Cc, Mall, Tz)
        K.cond_proj_wgrad(_dev(ins['cond']), _dev(ins['dce']), bufs[0].view, **dims)
    else:
        bufs = [DBuf(B * Cc * Tz), DBuf(B * Cc * Tz)]
        ref = CR.cond_proj_dgrad_ref(ins['w'], ins['dce'], bufs[0].buf.view, B, Cc, Mall, Tz)
        n = K.cond_proj_dgrad_scratch(B, Cc, Mall, Tz)
        for o in bufs:
            scratch = DBuf(n, init=np.full(n, np.nan, F32))        # NaN at exactly the size the query returns, guards behind it
            K.cond_proj_dgrad(_dev(ins['w']), _dev(ins['dce']), o.view, scratch.view, **dims)
            host = scratch.host()
            assert (host[:scratch.buf.lo] == CR.SENTINEL).all() and (host[scratch.buf.lo + n:] == CR.SENTINEL).all(), what + ': scratch guard'
    r = max(o.check(ref, what) for o in bufs)
    if len(bufs) == 2:
        assert torch.equal(bufs[0].view.view(torch.int32), bufs[1].view.view(torch.int32)), what + ': two launches differ'
    record_property('family', 'cond_proj_' + entry)
    record_property('err_over_bar', r)


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(call, outputs, what):
    with pytest.raises((RuntimeError, ValueError)):
        call()
    torch.cuda.synchronize()
    for o in outputs:
        o.untouched(what)


def test_cond_proj_refusals_launch_nothing(K):
    B, Mall, Tz = 2, 36, 8
    for entry, Cc, M2, T2, off in (('wgrad', 129, Mall, Tz, None), ('dgrad', 129, Mall, Tz, None), ('wgrad', 16, Mall, 6, None),
                                   ('dgrad', 16, 38, Tz, None), ('wgrad', 16, Mall, Tz, 'cond'), ('wgrad', 16, Mall, Tz, 'dce'),
                                   ('dgrad', 16, Mall, Tz, 'w'), ('dgrad', 16, Mall, Tz, 'scratch')):
        sd = CR.seed_of('refusal', entry, Cc, M2, T2, off)
        dims = dict(B=B, Cc=Cc, Mall=M2, Tz=T2)
        what = 'cond_proj_%s refusal Cc=%d Mall=%d Tz=%d %s' % (entry, Cc, M2, T2, off)
        cond = _dev_off(CR.randn(sd, B * Cc * T2), 1 if off == 'cond' else 0)
        dce = _dev_off(CR.randn(sd + 1, B * M2 * T2), 1 if off == 'dce' else 0)
        w = _dev_off(CR.randn(sd + 2, Cc * M2), 1 if off == 'w' else 0)
        if entry == 'wgrad':
            dw = DBuf(Cc * M2, init=CR.randn(sd + 3, Cc * M2))
            _refused(lambda: K.cond_proj_wgrad(cond, dce, dw.view, **dims), [dw], what)
        else:
            n = K.cond_proj_dgrad_scratch(B, Cc, M2, T2)
            dcond, scratch = DBuf(B * Cc * T2), DBuf(n)
            sv = scratch.view[:n - 1] if off == 'scratch' else scratch.view           # one float short
            _refused(lambda: K.cond_proj_dgrad(w, dce, dcond.view, sv, **dims), [dcond, scratch], what)


def test_vq_nearest_fwd_refusals_launch_nothing(K):
    B, Tz, Kc = 2, 5, 8
    for D, off in ((6, 0), (8, 1)):
        sd = CR.seed_of('vq refusal', D, off)
        z, emb = _dev(CR.randn(sd, B, D, Tz)), _dev_off(CR.randn(sd + 1, Kc, D), off)
        idx, ek, zq, mind = IBuf(B * Tz), DBuf(B * D * Tz), DBuf(B * D * Tz), DBuf(B * Tz)
        what = 'vq_nearest_fwd refusal D=%d emb offset %d' % (D, off)
        _refused(lambda: K.vq_nearest_fwd(z, emb, idx=idx.view.view(B, Tz), e_k=ek.view, zq=zq.view, mind=mind.view), [ek, zq, mind], what)
        assert (idx.full == IGUARD).all(), what + ': idx changed'


def test_speaker_tile_refuses_int32_ids(K):
    B, Cs, Tz, S = 2, 4, 3, 5
    table, spk = _dev(CR.randn(1, S, Cs)), torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    cond, dt = DBuf(B * Cs * Tz), DBuf(S * Cs)
    _refused(lambda: K.speaker_tile_fwd(table, spk, cond.view, cond_bstride=Cs * Tz, row0=0, Cs=Cs, Tz=Tz), [cond], 'speaker_tile_fwd int32 ids')
    _refused(lambda: K.speaker_tile_bwd(_dev(CR.randn(2, B * Cs * Tz)), spk, dt.view.view(S, Cs), dcond_bstride=Cs * Tz, row0=0, Cs=Cs, Tz=Tz),
             [dt], 'speaker_tile_bwd int32 ids')
