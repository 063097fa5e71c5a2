"""tests/conv_ref.py checked on the CPU: (1) the float64 reference of vqw_conv_gemm / vqw_wgrad_gemm equals the oracle's ops
and torch autograd of them, to 1e-12; (2) the comparison helper rejects every single-row / single-column / single-element
mutation of a correct result and accepts the reference rounded to fp32; (3) the case lists of
tests/test_conv_engine_epilogues_gpu.py meet the ABI's preconditions and contain the edges they are there for."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_ops as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as CR  # noqa: E402


def rnd(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape))        # float64


def bct(x_btc):
    return x_btc.detach().transpose(1, 2).contiguous().numpy()


def same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want.detach() if torch.is_tensor(want) else want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = float(np.abs(got - want).max())
    assert err <= 1e-12 * max(1.0, float(np.abs(want).max())), '%s: max abs err %.3e' % (what, err)


def out_of(res, name, *shape):
    vals, mask = res[name]
    assert mask.all(), '%s: not every element was written' % name
    return vals.reshape(shape)


# ---------------------------------------------------------------------------------------------------- reference vs oracle
@pytest.mark.parametrize('k,dil,stride', [(3, 3, 2), (2, 7, 1), (3, 60, 1)])
def test_store_is_conv1d_v2_with_dilation_and_stride(k, dil, stride):
    B, T, Cin, Cout = 2, 101, 16, 12
    x, w, b = rnd(1, B, T, Cin), rnd(2, k, Cin, Cout), rnd(3, Cout)
    want = R.conv1d_v2(x, w, b, dilations=dil, stride=stride)
    To = want.shape[1]
    res = CR.conv_ref(x0=bct(x), w=w.numpy(), bias=b.numpy(), out0=np.zeros(B * Cout * To), B=B, T_in=T, T_out=To, M=Cout, C0=Cin,
                      taps=[-(k - 1 - j) * dil for j in range(k)], in_stride=stride)
    same(out_of(res, 'out0', B, Cout, To), want.transpose(1, 2), 'conv1d_v2')


def test_gate_is_gated_cnn_with_a_condition():
    B, T, Cin, H, Cc, ratio, dil = 2, 100, 16, 20, 8, 20, 2
    Tz = T // ratio
    x, w, b = rnd(1, B, T, Cin), rnd(2, 3, Cin, 2 * H) * 0.2, rnd(3, 2 * H)
    cond, wc = rnd(4, B, Tz, Cc), rnd(5, 1, Cc, 2 * H)
    want = R.gated_cnn(x, {'gated/kernel': w, 'gated/bias': b, 'gated/local_condition/kernel': wc}, H, dil, cond)
    enc = R.conv1d_v2(cond, wc)                                            # [B,Tz,2H]
    pad = 7                                                                # an offset view with a batch stride above M * cond_T
    cbuf = np.full(3 + B * (2 * H * Tz + pad), 99.0)
    for i in range(B):
        cbuf[3 + i * (2 * H * Tz + pad):][:2 * H * Tz] = bct(enc)[i].reshape(-1)
    n = B * H * T
    res = CR.conv_ref(x0=bct(x), w=w.numpy(), bias=b.numpy(), cond=cbuf[3:], cond_T=Tz, cond_bstride=2 * H * Tz + pad,
                      out0=np.zeros(n), save0=np.zeros(n), save1=np.zeros(n), B=B, T_in=T, T_out=T, M=2 * H, C0=Cin,
                      taps=[-2 * dil, -dil, 0], epilogue=CR.EPI_GATE)
    same(out_of(res, 'out0', B, H, T), want.transpose(1, 2), 'gated_cnn')
    same(out_of(res, 'save0', B, H, T) * out_of(res, 'save1', B, H, T), want.transpose(1, 2), 'saved tanh * sigmoid')


@pytest.mark.parametrize('T_in,k', [(101, 5), (100, 4), (37, 5)])
def test_store_is_keras_same_conv_at_stride_2(T_in, k):
    B, Cin, Cout = 2, 16, 12
    x, w, b = rnd(1, B, T_in, Cin), rnd(2, k, Cin, Cout), rnd(3, Cout)
    want = R.keras_conv1d(x, w, b, stride=2, padding='same', relu=True)
    To, (pl, _) = want.shape[1], R.same_pads(T_in, k, 2)
    assert To == -(-T_in // 2) and CR.same_pads(T_in, k, 2) == R.same_pads(T_in, k, 2)
    sc, sh = rnd(4, Cout), rnd(5, Cout)
    n = B * Cout * To
    res = CR.conv_ref(x0=bct(x), w=w.numpy(), bias=b.numpy(), scale=sc.numpy(), shift=sh.numpy(), out0=np.zeros(n), save0=np.zeros(n),
                      B=B, T_in=T_in, T_out=To, M=Cout, C0=Cin, taps=[j - pl for j in range(k)], in_stride=2, out_relu=True)
    same(out_of(res, 'save0', B, Cout, To), want.transpose(1, 2), 'keras conv + relu')
    same(out_of(res, 'out0', B, Cout, To), (want * sc + sh).transpose(1, 2), 'relu -> affine')


def test_accum_split_is_skip_and_residual():
    B, T, Cg, S, Rr = 2, 77, 16, 12, 20
    gated, w, b = rnd(1, B, T, Cg), rnd(2, 1, Cg, S + Rr), rnd(3, S + Rr)
    skip0, net0 = rnd(4, B, T, S), rnd(5, B, T, Rr)
    want = R.conv1d_v2(gated, w, b)
    skip, net = bct(skip0).reshape(-1), bct(net0).reshape(-1)
    res = CR.conv_ref(x0=bct(gated), w=w.numpy(), bias=b.numpy(), out0=skip, out1=net, aux1=net, B=B, T_in=T, T_out=T, M=S + Rr,
                      M0=S, C0=Cg, taps=[0], epilogue=CR.EPI_ACCUM_SPLIT)
    same(out_of(res, 'out0', B, S, T), (skip0 + want[..., :S]).transpose(1, 2), 'skip += conv')
    same(out_of(res, 'out1', B, Rr, T), (net0 + want[..., S:]).transpose(1, 2), 'net = net + conv, in place')
    same(skip, bct(skip0).reshape(-1), 'the caller\'s buffer is not touched')
    # the residual half alone, from a view of the wide kernel (M0 = 0, ldw = S + R), out0 never written
    res = CR.conv_ref(x0=bct(gated), w=w.numpy().reshape(-1)[S:], ldw=S + Rr, bias=b.numpy()[S:], out0=net, out1=net, aux1=bct(net0),
                      B=B, T_in=T, T_out=T, M=Rr, M0=0, C0=Cg, taps=[0], epilogue=CR.EPI_ACCUM_SPLIT)
    assert res['out0'] is res['out1']
    same(out_of(res, 'out1', B, Rr, T), (net0 + want[..., S:]).transpose(1, 2), 'residual from the kernel view')


def test_gate_bwd_is_autograd_of_the_gate_through_skip_and_residual():
    B, T, H, S, Rr = 2, 53, 12, 16, 32
    pre = rnd(1, B, T, 2 * H).requires_grad_(True)
    th, sg = torch.tanh(pre[..., :H]), torch.sigmoid(pre[..., H:])
    w = rnd(2, 1, H, S + Rr)
    dskip, dnet = rnd(3, B, T, S), rnd(4, B, T, Rr)
    R.conv1d_v2(th * sg, w).backward(torch.cat([dskip, dnet], -1))
    res = CR.conv_ref(x0=bct(dskip), x1=bct(dnet), w=w[0].t().contiguous().numpy(), out0=np.zeros(B * 2 * H * T), aux0=bct(th),
                      aux1=bct(sg), B=B, T_in=T, T_out=T, M=H, C0=S, C1=Rr, taps=[0], epilogue=CR.EPI_GATE_BWD)
    same(out_of(res, 'out0', B, 2 * H, T), pre.grad.transpose(1, 2), 'gate backward')


@pytest.mark.parametrize('in_place', [False, True])
def test_mask_is_autograd_of_relu_then_affine(in_place):
    B, T, Cc, Q = 2, 61, 12, 16
    a = rnd(1, B, T, Cc)
    a[:, ::5] = 0.0                                                        # relu'(0) = 0
    a.requires_grad_(True)
    sc, w, dy = rnd(2, Cc), rnd(3, 1, Cc, Q), rnd(4, B, T, Q)
    h = torch.relu(a)
    R.conv1d_v2(h * sc, w).backward(dy)
    hb = bct(h).reshape(-1)
    res = CR.conv_ref(x0=bct(dy), w=w[0].t().contiguous().numpy(), scale=sc.numpy(), aux0=hb, out0=hb if in_place else np.zeros(hb.size),
                      B=B, T_in=T, T_out=T, M=Cc, C0=Q, taps=[0], epilogue=CR.EPI_MASK)
    same(out_of(res, 'out0', B, Cc, T), a.grad.transpose(1, 2), 'mask')
    assert float(np.abs(out_of(res, 'out0', B, Cc, T)[:, :, ::5]).max()) == 0.0


def test_store_with_transposed_taps_is_the_input_gradient_of_conv1d_v2():
    B, T, Cin, Cout, k, dil = 2, 101, 12, 16, 3, 5
    x, w, dy = rnd(1, B, T, Cin).requires_grad_(True), rnd(2, k, Cin, Cout), rnd(3, B, T, Cout)
    R.conv1d_v2(x, w, None, dilations=dil).backward(dy)
    wT = w.transpose(1, 2).contiguous().numpy()
    for split in (0, 3, -3):
        res = CR.conv_ref(x0=bct(dy), w=wT, out0=np.zeros(B * Cin * T) if split < 0 else np.full(B * Cin * T, 7.0), B=B, T_in=T,
                          T_out=T, M=Cin, C0=Cout, taps=[(k - 1 - j) * dil for j in range(k)], split_k=split)
        same(out_of(res, 'out0', B, Cin, T), x.grad.transpose(1, 2), 'dgrad, split_k %d' % split)


@pytest.mark.parametrize('T_in,k', [(101, 5), (100, 5), (101, 4), (100, 4), (37, 5)])
@pytest.mark.parametrize('split', [0, -2])
def test_two_phase_store_is_the_input_gradient_of_the_stride_2_conv(T_in, k, split):
    """The encoders' decomposition: output times tau = 2u + p take the taps j = p + pad_left (mod 2) of the per-tap transposed
    kernel; each launch writes its own parity and the two together are autograd's dx, for odd and even T_in."""
    B, Cin, Cout = 2, 12, 16
    x, w = rnd(1, B, T_in, Cin).requires_grad_(True), rnd(2, k, Cin, Cout)
    y = R.keras_conv1d(x, w, None, stride=2, padding='same')
    dy = rnd(3, *y.shape)
    y.backward(dy)
    To, (pl, _) = y.shape[1], R.same_pads(T_in, k, 2)
    wT = w.transpose(1, 2).contiguous().numpy().reshape(-1)
    n = B * Cin * T_in
    buf, masks = (np.zeros(n) if split < 0 else np.full(n, float(CR.SENTINEL))), []
    for p in (0, 1):
        j0 = (p + pl) % 2
        res = CR.conv_ref(x0=bct(dy), w=wT[j0 * Cout * Cin:], w_tap_stride=2 * Cout * Cin, out0=buf, B=B, T_in=To,
                          T_out=(T_in - p + 1) // 2, M=Cin, C0=Cout, taps=[(p + pl - j) // 2 for j in range(j0, k, 2)],
                          out_tstride=2, out_toffset=p, T_store=T_in, split_k=split)
        buf, m = res['out0']
        masks.append(m.reshape(B, Cin, T_in))
        assert m.reshape(B, Cin, T_in)[:, :, p::2].all() and not m.reshape(B, Cin, T_in)[:, :, 1 - p::2].any()
    assert not (masks[0] & masks[1]).any() and (masks[0] | masks[1]).all()
    same(buf.reshape(B, Cin, T_in), x.grad.transpose(1, 2), 'two-phase dgrad')


def test_wgrad_is_autograd_of_conv1d_v2_and_of_the_stride_2_conv():
    B, T, Cin, Q0, Q1, k, dil = 2, 101, 12, 10, 6, 3, 4
    x, dy = rnd(1, B, T, Cin), rnd(2, B, T, Q0 + Q1)
    x[:, ::7] = 0.0
    w = torch.zeros(k, Cin, Q0 + Q1, dtype=torch.float64, requires_grad=True)
    R.conv1d_v2(torch.relu(x), w, None, dilations=dil).backward(dy)
    # two sources, relu on p, into a view of a wider non-zero matrix with its own tap stride
    ld, off, dts = Q0 + Q1 + 5, 3, Cin * (Q0 + Q1 + 5) + 9
    old = rnd(3, off + k * dts).numpy()
    vals, mask = CR.wgrad_ref(p=bct(x), q0=bct(dy[..., :Q0]), q1=bct(dy[..., Q0:]), dw=old[off:], B=B, T_q=T, T_p=T, Cp=Cin, Q0=Q0, Q1=Q1,
                              taps=[-(k - 1 - j) * dil for j in range(k)], p_relu=True, lddw=ld, dw_tap_stride=dts)
    ix = np.arange(k)[:, None, None] * dts + np.arange(Cin)[None, :, None] * ld + np.arange(Q0 + Q1)[None, None, :]
    same(vals[ix] - old[off:][ix], w.grad, 'wgrad += , two sources, relu, strided view')
    assert mask[ix].all() and int(mask.sum()) == ix.size and np.array_equal(vals[~mask], old[off:][~mask])
    for T_in, kk in ((101, 5), (100, 4)):
        x2 = rnd(4, B, T_in, Cin)
        w2 = torch.zeros(kk, Cin, Q0, dtype=torch.float64, requires_grad=True)
        y = R.keras_conv1d(x2, w2, None, stride=2, padding='same')
        dy2 = rnd(5, *y.shape)
        y.backward(dy2)
        pl, _ = R.same_pads(T_in, kk, 2)
        vals, mask = CR.wgrad_ref(p=bct(x2), q0=bct(dy2), dw=np.zeros(kk * Cin * Q0), B=B, T_q=y.shape[1], T_p=T_in, Cp=Cin, Q0=Q0,
                                  taps=[j - pl for j in range(kk)], p_stride=2)
        assert mask.all()
        same(vals.reshape(kk, Cin, Q0), w2.grad, 'wgrad, p_stride 2, T_p %d' % T_in)


def test_every_conv_family_matches_a_direct_evaluation_on_a_ragged_case():
    """The generated cases themselves (strided stores, aliases, two launches) against the formula evaluated point by point."""
    for fam in CR.FAMILIES:
        c = [c for c in CR.conv_base_cases() if c['fam'] == fam and c['T_in'] not in (1024,) and c['C0'] <= 96][0]
        ins, bufs, exp = CR.conv_expected(c, 1)
        L = CR.launches_of(c)[0]
        kw, ops = CR.conv_kwargs(c, L), CR.conv_operands(c, L, ins, {n: b.view for n, b in bufs.items()})
        acc = CR.conv_acc(**kw, **ops)
        g = CR.geometry(c)
        x = np.concatenate([ins['x0']] + ([ins['x1']] if c['C1'] else []), axis=1).astype(np.float64)
        if c['in_relu']:
            x = np.maximum(x, 0)
        rng = np.random.RandomState(0)
        for _ in range(50):
            b, m, t = rng.randint(c['B']), rng.randint(c['M']), rng.randint(L['T_out'])
            v = 0.0
            for j, s in enumerate(L['taps']):
                ti = c['in_stride'] * t + s
                if 0 <= ti < c['T_in']:
                    v += float(np.dot(ins['w'].astype(np.float64)[L['woff'] + j * g['wts'] + np.arange(g['C']) * g['ldw'] + m], x[b, :, ti]))
            assert abs(v - acc[b, m, t]) <= 1e-12 * max(1.0, abs(v)), c['name']
        for n, (ref, keep) in exp.items():
            b = bufs[n]
            assert keep[:b.lo].all() and keep[b.lo + b.n:].all() and np.array_equal(ref[keep], b.full.astype(np.float64)[keep]), c['name']


# ---------------------------------------------------------------------------------------------------- the helper has teeth
def _case(name):
    return [c for c in CR.conv_base_cases() if c['name'] == name][0]


def _as_got(exp):
    """A correct result: the reference rounded to fp32."""
    return {n: e[0].astype(np.float32) for n, e in exp.items()}


def _check(got, exp, c):
    return CR.check(got, {n: e[0] for n, e in exp.items()}, {n: e[1] for n, e in exp.items()}, CR.bar_of(c), c['name'])


def _mutated(c, change):
    """(correct expectation, the result of the same case with `change(ins, bufs)` applied to its operands)."""
    _, _, exp = CR.conv_expected(c, 0)
    ins, bufs = CR.build_conv(c, 0)
    ins = {n: a.copy() for n, a in ins.items()}
    change(ins, bufs)
    _, _, bad = CR.conv_expected(c, 0, (ins, bufs))
    return exp, _as_got(bad)


@pytest.mark.parametrize('off', [0, 1])
def test_check_accepts_the_reference_rounded_to_fp32(off):
    for c in CR.conv_base_cases():
        if c['C0'] > 96 or c['T_in'] == 1024:
            continue
        _, _, exp = CR.conv_expected(c, off)
        assert _check(_as_got(exp), exp, c) < (0.05 if c['epilogue'] == CR.EPI_GATE else 0.01), c['name']
    for c in CR.wgrad_cases()[:3]:
        _, _, (ref, keep) = CR.wgrad_expected(c, off)
        assert CR.check({'dw': ref.astype(np.float32)}, {'dw': ref}, {'dw': keep}, CR.BAR_WGRAD) < 0.01


def test_check_rejects_a_bias_dropped_on_the_last_row():
    c = _case('store/all/0')

    def change(ins, bufs):
        ins['bias'][-1] = 0.0
    exp, got = _mutated(c, change)
    with pytest.raises(AssertionError, match='max abs err'):
        _check(got, exp, c)


def test_check_rejects_a_condition_frame_off_by_one_at_one_boundary():
    c = _case('store/cond')                       # out = acc + cond[b][row][t // ratio], nothing else
    _, _, exp = CR.conv_expected(c, 0)
    ins, bufs = CR.build_conv(c, 0)
    g, ratio = CR.geometry(c), c['T_out'] // c['cond_T']
    got = _as_got(exp)
    b, row, frame = c['B'] - 1, c['M'] - 1, 3     # the first column of frame 3 takes frame 2's value
    cond = ins['cond'][c['cond_off'] + b * g['cond_bstride'] + row * c['cond_T']:]
    o = bufs['out0'].lo + (b * c['M'] + row) * g['Ts'] + frame * ratio
    got['out0'][o] += np.float32(cond[frame - 1] - cond[frame])
    assert abs(float(cond[frame - 1] - cond[frame])) > 100 * CR.BAR_CONV
    with pytest.raises(AssertionError, match='max abs err'):
        _check(got, exp, c)


def test_check_rejects_an_unwritten_last_column_of_the_last_partial_tile():
    for name in ('store/all/0', 'gate/H132/all', 'mask/in_place/scale'):
        c = _case(name)
        _, _, exp = CR.conv_expected(c, 0)
        ins, bufs = CR.build_conv(c, 0)
        got = _as_got(exp)
        b, Ts = bufs['out0'], CR.geometry(c)['Ts']
        last = b.lo + np.arange(Ts - 1, b.n, Ts)               # the last column of every row
        o = int(last[np.abs(b.full[last] - exp['out0'][0][last]) > 0.1][-1])   # (in place: aux0 may equal the result, 0)
        assert not exp['out0'][1][o]
        got['out0'][o] = bufs['out0'].full[o]                  # what was there before: the sentinel, or aux0 in place
        with pytest.raises(AssertionError, match='max abs err'):
            _check(got, exp, c)


def test_check_rejects_shift_replaced_by_scale_on_one_row():
    c = _case('store/affine')

    def change(ins, bufs):
        ins['shift'][c['M'] // 2] = ins['scale'][c['M'] // 2]
    exp, got = _mutated(c, change)
    with pytest.raises(AssertionError, match='max abs err'):
        _check(got, exp, c)


def test_check_rejects_the_m0_boundary_row_in_the_wrong_output():
    c = _case('store/split')
    _, _, exp = CR.conv_expected(c, 0)
    ins, bufs = CR.build_conv(c, 0)
    g = CR.geometry(c)
    Ts, m0 = g['Ts'], g['m0']
    assert 0 < m0 < c['M']
    row = exp['out1'][0][bufs['out1'].lo:][:Ts].astype(np.float32)       # row M0 of batch 0: the first row of out1
    # ... stored as row M0 of out0 instead, which is row 0 of the next batch element there; out1 keeps its sentinels
    got = _as_got(exp)
    got['out1'][bufs['out1'].lo:][:Ts] = CR.SENTINEL
    with pytest.raises(AssertionError, match='out1: max abs err'):
        _check(got, exp, c)
    got = _as_got(exp)
    got['out0'][bufs['out0'].lo + m0 * Ts:][:Ts] = row
    with pytest.raises(AssertionError, match='out0: max abs err'):
        _check(got, exp, c)


def test_check_rejects_one_overwritten_sentinel():
    c = _case('strides/dgrad/even_phase_only')
    _, _, exp = CR.conv_expected(c, 1)
    ins, bufs = CR.build_conv(c, 1)
    b = bufs['out0']
    for o in (0, b.lo - 1, b.lo + 1, b.lo + b.n - 2, b.lo + b.n, b.full.size - 1):   # guard bands and the odd stride phase
        got = _as_got(exp)
        assert exp['out0'][1][o]
        got['out0'][o] = np.float32(0.0)
        with pytest.raises(AssertionError, match='must not touch'):
            _check(got, exp, c)
    got = _as_got(exp)
    got['out0'][0] = CR.SENTINEL                                         # the same value: accepted
    _check(got, exp, c)
    c = [c for c in CR.wgrad_cases() if c['name'] == 'wgrad/view/lddw136'][0]
    _, dw, (ref, keep) = CR.wgrad_expected(c, 0)
    got = ref.astype(np.float32)
    o = dw.lo + c['dw_off'] + c['Q0']                                    # the first column right of the view, row 0
    assert keep[o]
    got[o] = np.nextafter(got[o], np.float32(np.inf))                    # one ulp
    with pytest.raises(AssertionError, match='must not touch'):
        CR.check({'dw': got}, {'dw': ref}, {'dw': keep}, CR.BAR_WGRAD)


def test_check_rejects_mask_passing_zero():
    c = _case('mask/out_of_place')

    def change(ins, bufs):                         # a kernel testing aux0 >= 0: the same as zeros turned positive
        v = bufs['aux0'].view
        assert (v == 0).sum() > 10 and (v > 0).any() and (v < 0).any()
        v[v == 0] = 1.0
    exp, got = _mutated(c, change)
    got['aux0'] = exp['aux0'][0].astype(np.float32)
    with pytest.raises(AssertionError, match='out0: max abs err'):
        _check(got, exp, c)


def test_check_rejects_nan_and_a_missing_relu():
    c = _case('store/out_relu')
    _, _, exp = CR.conv_expected(c, 0)
    ins, bufs = CR.build_conv(c, 0)
    got = _as_got(exp)
    got['out0'][bufs['out0'].lo + 5] = np.nan
    with pytest.raises(AssertionError, match='max abs err'):
        _check(got, exp, c)
    c2 = dict(c, out_relu=False)
    _, _, bad = CR.conv_expected(c2, 0)
    with pytest.raises(AssertionError, match='max abs err'):
        _check(_as_got(bad), exp, c)


# ---------------------------------------------------------------------------------------------------- the case lists
def test_every_case_meets_the_preconditions():
    for c, tile in CR.conv_cases():
        assert CR.legality(c, tile) == [], CR.case_id(c, tile)
    for c in CR.conv_base_cases():
        g = CR.geometry(c)
        ins, bufs = CR.build_conv(c, 1)
        assert ins['w'].size >= g['w_len'] and ins['w'].dtype == np.float32
        for L in CR.launches_of(c):
            assert (ins['w'][L['woff']:].ctypes.data - ins['w'].ctypes.data) % 16 == 0
        for n, b in bufs.items():
            assert b.n * 4 <= 1024 * 1024, '%s: %s has %d KB' % (c['name'], n, b.n * 4 // 1024)
            assert b.lo >= CR.GUARD and b.full.size - b.lo - b.n >= CR.GUARD
        assert c['B'] in (1, 2, 3) and c['T_out'] <= 1024
    for c in CR.wgrad_cases():
        assert CR.wgrad_legality(c) == [], c['name']
    assert CR.legality(dict(_case('store/bias'), C0=24), 0) and CR.legality(dict(_case('store/bias'), M=6), 0)
    assert CR.legality(_case('gate/H36/one_frame'), 12) and CR.legality(dict(_case('store/cond'), cond_T=7), 0)
    assert CR.legality(dict(_case('store/bias'), ldw=134), 0) and CR.legality(dict(_case('accum_split/M0=0/weight_view'), woff=98), 0)


@pytest.mark.parametrize('fam', CR.EPILOGUE_FAMILIES)
def test_every_epilogue_family_contains_the_edges(fam):
    cases = [(c, t) for c, t in CR.conv_cases() if c['fam'] == fam]
    tiles = CR.GATE_TILES if fam == 'gate' else CR.TILES
    legal_main = [t for t in CR.MAIN_TILES if fam != 'gate' or t // 10 == 2]
    assert any(CR.geometry(c)['Ts'] % 4 for c, _ in cases)
    assert any(c['T_out'] < 64 for c, _ in cases)
    assert any(c['T_out'] == 1024 for c, _ in cases)
    assert any(CR.tile_geometry(c, t)[0] > 1 and CR.tile_geometry(c, t)[1] < CR.tile_geometry(c, t)[2] for c, t in cases if t)
    for t in legal_main:
        assert any(tile == t for _, tile in cases)
        # more than one M tile with a partial last one, more than one column tile with a partial last one, on THIS tile
        # (GATE_BWD's M of 36 and 100 is one tile of the MT=2 forms)
        ragged_m = [tile == t and CR.tile_geometry(c, t)[0] > 1 and CR.tile_geometry(c, t)[1] < CR.tile_geometry(c, t)[2] for c, tile in cases]
        assert any(ragged_m) or (fam == 'gate_bwd' and t // 10 == 2), t
        assert any(tile == t and c['T_out'] > CR.tile_geometry(c, t)[3] and c['T_out'] % CR.tile_geometry(c, t)[3] for c, tile in cases), t
    assert any(t >= 10000 for t in tiles)
    for c, t in cases:                                   # a tail form must really hand columns to half-width tiles somewhere
        if t >= 10000 and -(-c['T_out'] // CR.tile_geometry(c, t)[3]) > t // 10000:
            break
    else:
        raise AssertionError('no case on which a tail-tile form takes effect')
    for c in {c['name']: c for c, _ in cases}.values():
        assert tuple(t for cc, t in cases if cc is c) == tiles, c['name']
    if fam in ('store', 'gate'):
        ratios = {c['T_out'] // c['cond_T'] for c, _ in cases if c['cond_T']}
        assert any(64 % r for r in ratios) and any(r == 4 for r in ratios) and any(r == 20 for r in ratios)
        assert any(c['cond_T'] == 1 for c, _ in cases)                              # one frame: ratio = T_out
    if fam == 'store':
        names = {c['name'] for c, _ in cases}
        assert {'store/' + o for o in ('bias', 'cond', 'out_relu', 'save0', 'affine', 'aux1', 'split', 'in_relu')} <= names
        assert any(all(t + c['in_stride'] * (c['T_out'] - 1) < 0 for t in c['taps'][:-1]) and len(c['taps']) > 2 for c, _ in cases)
    if fam == 'accum_split':
        m0s = {(c['M0'], c['M']) for c, _ in cases}
        assert any(m0 == 0 for m0, _ in m0s) and any(m0 == m for m0, m in m0s) and any(0 < m0 < m and m0 % 32 for m0, m in m0s)
        assert any(c['twice'] for c, _ in cases) and any(c['woff'] and CR.geometry(c)['ldw'] > c['M'] for c, _ in cases)
        assert any(set(c['alias']) == {'aux1', 'out1'} for c, _ in cases) and any(len(c['alias']) == 3 for c, _ in cases)
    if fam == 'gate':
        assert {c['M'] // 2 for c, _ in cases} == {4, 36, 68, 100, 132}
    if fam == 'gate_bwd':
        assert {c['M'] for c, _ in cases} == {36, 100} and {c['C1'] > 0 for c, _ in cases} == {True, False}
    if fam == 'mask':
        assert {(bool(c['alias']), c['affine']) for c, _ in cases} == {(a, s) for a in (True, False) for s in (True, False)}


def test_stride_split_k_and_wgrad_lists_contain_their_cases():
    st = [c for c in CR.conv_base_cases() if c['fam'] == 'strides']
    assert {c['T_in'] for c in st if c['in_stride'] == 2} >= {250, 255, 256}
    ph = [c for c in st if c['phases']]
    assert {c['T_store'] % 2 for c in ph} == {0, 1} and {c['split_k'] < 0 for c in ph} == {True, False}
    assert all(c['w_tap_stride'] == 2 * c['C0'] * c['M'] and c['out_tstride'] == 2 for c in ph)
    sk = {c['name']: c for c in CR.conv_base_cases() if c['fam'] == 'split_k'}
    a = sk['split_k/auto']                                 # the automatic branch on a chip of >= 16 CUs, on every tile it runs on
    assert len(a['taps']) * a['C0'] // 16 >= 64 and a['split_k'] == 0
    assert -(-a['M'] // 64) * -(-a['T_out'] // 64) * a['B'] * 2 <= 16          # blocks of the narrowest tile
    ksteps = {n: len(c['taps']) * c['C0'] // 16 for n, c in sk.items()}
    assert any(c['split_k'] > ksteps[n] for n, c in sk.items()) and {2, 7} <= {c['split_k'] for c in sk.values()}
    wg = CR.wgrad_cases()
    assert {(64, 32), (100, 28), (64, 256), (128, 132)} <= {(c['Q0'], c['Q1']) for c in wg}
    assert {c['T_q'] for c in wg} >= {37, 100, 333, 1000} and {c['splits'] for c in wg} == {0, 1, 3}
    assert any(c['p_stride'] == 2 and c['T_p'] % 2 for c in wg) and any(c['p_relu'] for c in wg)
    assert any(CR.wgrad_geometry(c)['lddw'] > c['Q0'] + c['Q1'] and c['dw_tap_stride'] and c['nonzero'] for c in wg)
