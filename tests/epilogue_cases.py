"""Seeded cases for the epilogues of the fp16x3 conv kernels (gate conv, residual 1x1 + skip, input gradient, gate backward,
head), driven through kernels.py.  Every case returns the raw bytes of every output it wrote: fp32 tensors, planes viewed as
int16, the max-abs slot and the range flag.  tests/golden/make_epilogue_digests.py hashes them into
tests/golden/epilogue_digests.json; tests/test_epilogue_pipeline_gpu.py compares against that file.

Shapes are the smallest with more than one epilogue group, column tile, row block and batch row: B = 2, T = 512.
A case name is kernel/mode/key=value/...; cases that differ only in `alias` or in which optional outputs they ask for
must agree on the outputs they share (the test checks that from the digests)."""
import functools
import hashlib
import itertools

import torch

B, T = 2, 512
X3_BF16, X3_HALF = 1, 2
MODES = (('m0', 0), ('half', X3_HALF))
DEV = 'cuda:0'


def _rand(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _planes(n_halves):
    # (sized for two fp16 planes; the bf16 engine uses the first half.  Zeroed: a case never returns bytes it did not write)
    return torch.zeros(n_halves, dtype=torch.float16, device=DEV)


def _slots():
    return torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)


def raw(t):
    """The bytes of a device tensor (fp16 / bf16 planes as int16)."""
    if t.dtype == torch.float16:
        t = t.view(torch.int16)
    return t.detach().cpu().contiguous().numpy().tobytes()


def digest(outputs):
    return {k: hashlib.sha256(raw(v)).hexdigest() for k, v in sorted(outputs.items())}


# ---------------------------------------------------------------- residual 1x1 + skip (epi 0, S > 0)
@functools.lru_cache(maxsize=None)
def _res_inputs(K, mode):
    R, S = 256, 512
    g = _rand(101, B, R, T)
    w = _rand(102, R, S + R, scale=0.05)
    gp, wp = _planes(2 * B * R * T), _planes(2 * R * (S + R))
    K.f16x3_split_activations(g, gp, B, R, T, mode=mode)
    K.f16x3_pack_weights(w, wp, R, S + R, S + R, 256.0, mode=mode)
    return dict(R=R, S=S, gp=gp, wp=wp, bias=_rand(103, S + R), skip=_rand(104, B, S, T), net=_rand(105, B, R, T),
                out_scale=torch.tensor([4.0], device=DEV))


def res_case(K, mode, alias, planes):
    i = _res_inputs(K, mode)
    R, S = i['R'], i['S']
    skip, net_in = i['skip'].clone(), i['net'].clone()
    net_out = net_in if alias else torch.zeros_like(net_in)
    kw, out = {}, {}
    if planes:
        amax, flag = _slots()
        pl = _planes(2 * B * R * T)
        kw = dict(net_out_planes=pl, out_scale=i['out_scale'], out_amax=amax, flag=flag)
        out = dict(planes=pl, amax=amax, flag=flag)
    K.f16x3_out_conv(xp=i['gp'], wp=i['wp'], B=B, T=T, R=R, S=S, w_scale_inv=1.0 / 256.0, skip=skip, net_in=net_in, net_out=net_out,
                     bias=i['bias'], mode=mode, **kw)
    out.update(skip=skip, net_out=net_out)
    return out


# ---------------------------------------------------------------- input gradient of the gate conv (epi 0, S = 0, dir < 0)
@functools.lru_cache(maxsize=None)
def _dgrad_inputs(K, mode):
    R, Cin, ks = 256, 512, 3
    x = _rand(201, B, Cin, T)
    w = _rand(202, ks * Cin, R, scale=0.03)
    xp, wp = _planes(2 * B * Cin * T), _planes(2 * ks * Cin * R)
    K.f16x3_split_activations(x, xp, B, Cin, T, mode=mode)
    K.f16x3_pack_weights(w, wp, ks * Cin, R, R, 256.0, mode=mode)
    return dict(R=R, Cin=Cin, ks=ks, xp=xp, wp=wp, net=_rand(203, B, R, T), out_scale=torch.tensor([2.0], device=DEV))


def dgrad_case(K, mode, dilation, net_in):
    i = _dgrad_inputs(K, mode)
    R = i['R']
    src = None if net_in == 'none' else i['net'].clone()
    net_out = src if net_in == 'alias' else torch.zeros(B, R, T, device=DEV)
    amax, flag = _slots()
    pl = _planes(2 * B * R * T)
    K.f16x3_out_conv(xp=i['xp'], wp=i['wp'], B=B, T=T, R=R, S=0, Cin=i['Cin'], ks=i['ks'], dilation=dilation, direction=-1,
                     w_scale_inv=1.0 / 256.0, net_in=src, net_out=net_out, net_out_planes=pl, out_scale=i['out_scale'], out_amax=amax,
                     flag=flag, mode=mode)
    return dict(net_out=net_out, planes=pl, amax=amax, flag=flag)


# ---------------------------------------------------------------- gate backward (epi 1)
@functools.lru_cache(maxsize=None)
def _bwd_inputs(K, mode):
    R, S = 256, 256
    dcat = _rand(301, B, S + R, T, scale=1e-5)
    w = _rand(302, S + R, R, scale=0.05)
    xf, xg = _rand(303, B, R, T, scale=2.0), _rand(304, B, R, T, scale=3.0)
    xg[:, ::7, ::5] = -200.0          # sigmoid == 0
    xg[:, 3::7, 1::5] = -88.0         # a denormal sigmoid
    xg[:, 5::7, 2::5] = -87.0         # the smallest normal numbers
    th, sg = torch.tanh(xf), torch.sigmoid(xg)
    gated = th * sg
    sc = torch.tensor([2.0 ** 28, 64.0, 2.0 ** 26], device=DEV)
    gr, wp = _planes(2 * B * (S + R) * T), _planes(2 * (S + R) * R)
    K.f16x3_split_activations(dcat, gr, B, S + R, T, scale_dev=sc[0:1], mode=mode)
    K.f16x3_pack_weights(w, wp, S + R, R, R, 1.0, scale_dev=sc[1:2], mode=mode)
    gpl = _planes(2 * B * 3 * R * T)      # the gated planes inside a wider planes tensor (three layers side by side)
    K.f16x3_split_activations(gated, gpl, B, R, T, kc0=R // 8, KC=3 * (R // 8), mode=mode)
    return dict(R=R, S=S, gr=gr, wp=wp, th=th, sg=sg, gated=gated, gpl=gpl, sc=sc)


def bwd_case(K, mode, aux, fp32):
    i = _bwd_inputs(K, mode)
    R, S, sc = i['R'], i['S'], i['sc']
    amax, flag = _slots()
    pl = _planes(2 * B * 2 * R * T)
    dpre = torch.zeros(B, 2 * R, T, device=DEV) if fp32 else None
    kw = dict(aux0=i['th']) if aux == 'tanh' else dict(aux0=i['gated'], aux0_is_gated=True) if aux == 'gated' else \
        dict(aux0_is_gated=True, aux0_planes=i['gpl'], aux0_KC=3 * (R // 8), aux0_kc0=R // 8)
    K.f16x3_out_conv(epi=1, xp=i['gr'], Cin=S + R, wp=i['wp'], aux1=i['sg'], net_out=dpre, net_out_planes=pl, B=B, T=T, R=R, S=0,
                     w_scale_inv=1.0, x_scale=sc[0:1], w_scale=sc[1:2], out_scale=sc[2:3], out_amax=amax, flag=flag, mode=mode, **kw)
    out = dict(planes=pl, amax=amax, flag=flag)
    if fp32:
        out['dpre'] = dpre
    return out


# ---------------------------------------------------------------- gate conv
GATE_OUTPUTS = ('out0', 'save0', 'save1', 'out_planes')
# every subset the entry point accepts: out0 may be left out only where save1 and the planes are written
GATE_SUBSETS = tuple(s for n in range(1, 5) for s in itertools.combinations(GATE_OUTPUTS, n)
                     if 'out0' in s or ('save1' in s and 'out_planes' in s))
COND_T = 8


@functools.lru_cache(maxsize=None)
def _gate_inputs(K, mode, R, ks):
    x = _rand(401 + R + ks, B, R, T)
    w = _rand(402 + R + ks, ks, R, 2 * R, scale=0.05)
    xp, wp = _planes(2 * B * R * T), _planes(2 * ks * R * 2 * R)
    K.f16x3_split_activations(x, xp, B, R, T, mode=mode)
    K.f16x3_pack_gate_weights(w, wp, ks, R, 2 * R, 256.0, mode=mode)
    return dict(xp=xp, wp=wp, bias=_rand(403 + R, 2 * R), cond=_rand(404 + R, B, 2 * R, COND_T))


def gate_case(K, mode, R, ks, dilation, bias, cond, subset):
    i = _gate_inputs(K, mode, R, ks)
    out = {n: (_planes(2 * B * R * T) if n == 'out_planes' else torch.zeros(B, R, T, device=DEV)) for n in subset}
    K.f16x3_gate_conv(xp=i['xp'], wp=i['wp'], out0=out.get('out0'), B=B, T=T, R=R, ks=ks, dilation=dilation, w_scale_inv=1.0 / 256.0,
                      bias=i['bias'] if bias else None, cond=i['cond'] if cond else None, cond_T=COND_T if cond else 0,
                      save0=out.get('save0'), save1=out.get('save1'), out_planes=out.get('out_planes'), mode=mode)
    return out


# ---------------------------------------------------------------- head (epi 2)
@functools.lru_cache(maxsize=None)
def _head_inputs(K, mode):
    Cin, R = 256, 512
    x = _rand(501, B, Cin, T)
    w = _rand(502, Cin, R, scale=0.05)
    xp, wp = _planes(2 * B * Cin * T), _planes(2 * Cin * R)
    K.f16x3_split_activations(x, xp, B, Cin, T, mode=mode)
    K.f16x3_pack_weights(w, wp, Cin, R, R, 256.0, mode=mode)
    return dict(Cin=Cin, R=R, xp=xp, wp=wp, bias=_rand(503, R), net=_rand(504, B, R, T), mask=_rand(505, B, R, T),
                cond=_rand(506, B, R, COND_T), out_scale=torch.tensor([2.0], device=DEV))


def head_case(K, mode, alias, cond, relu):
    i = _head_inputs(K, mode)
    R = i['R']
    net_in, mask = i['net'].clone(), i['mask'].clone()
    net_out = net_in if alias == 'net_in' else mask if alias == 'aux0' else torch.zeros(B, R, T, device=DEV)
    amax, flag = _slots()
    pl = _planes(2 * B * R * T)
    K.f16x3_out_conv(epi=2, xp=i['xp'], wp=i['wp'], B=B, T=T, R=R, S=0, Cin=i['Cin'], w_scale_inv=1.0 / 256.0, net_in=net_in, net_out=net_out,
                     aux0=mask, bias=i['bias'], net_out_planes=pl, out_scale=i['out_scale'], out_amax=amax, flag=flag, mode=mode,
                     cond=i['cond'] if cond else None, cond_T=COND_T if cond else 0, cond_bstride=R * COND_T if cond else 0,
                     relu_planes=relu)
    return dict(net_out=net_out, planes=pl, amax=amax, flag=flag)


# ---------------------------------------------------------------- the table
def _sub(s):
    return '+'.join(s)


def cases():
    """[(name, thunk(K) -> {output: tensor})] in a fixed order."""
    c = []
    for mn, m in MODES:
        for alias, planes in itertools.product((0, 1), (0, 1)):
            c.append(('res/%s/alias=%d/planes=%d' % (mn, alias, planes), functools.partial(res_case, mode=m, alias=alias, planes=planes)))
        for dil, ni in itertools.product((3, 300), ('none', 'distinct', 'alias')):
            c.append(('dgrad/%s/d=%d/net_in=%s' % (mn, dil, ni), functools.partial(dgrad_case, mode=m, dilation=dil, net_in=ni)))
        for aux, fp32 in itertools.product(('tanh', 'gated', 'planes'), (1, 0)):
            c.append(('bwd/%s/aux0=%s/fp32=%d' % (mn, aux, fp32), functools.partial(bwd_case, mode=m, aux=aux, fp32=fp32)))
        # every subset of the outputs on two geometries ...
        for (R, ks, dil, hb, hc), sub in itertools.product(((256, 3, 1, 1, 1), (128, 2, 300, 0, 1)), GATE_SUBSETS):
            c.append(('gate/%s/R=%d/ks=%d/d=%d/bias=%d/cond=%d/%s' % (mn, R, ks, dil, hb, hc, _sub(sub)),
                      functools.partial(gate_case, mode=m, R=R, ks=ks, dilation=dil, bias=hb, cond=hc, subset=sub)))
        # ... and every geometry with what the training step asks for (even) or with all four outputs (odd)
        for n, (R, ks, dil, hb, hc) in enumerate(itertools.product((128, 256), (2, 3), (1, 300), (0, 1), (0, 1))):
            sub = GATE_OUTPUTS if n & 1 else ('save1', 'out_planes')
            name = 'gate/%s/R=%d/ks=%d/d=%d/bias=%d/cond=%d/%s' % (mn, R, ks, dil, hb, hc, _sub(sub))
            if name not in dict(c):
                c.append((name, functools.partial(gate_case, mode=m, R=R, ks=ks, dilation=dil, bias=hb, cond=hc, subset=sub)))
        for alias, cond, relu in itertools.product(('none', 'net_in', 'aux0'), (0, 1), (0, 1)):
            c.append(('head/%s/alias=%s/cond=%d/relu=%d' % (mn, alias, cond, relu),
                      functools.partial(head_case, mode=m, alias=alias, cond=cond, relu=relu)))
    # one bf16 case per kernel
    c.append(('res/bf16/alias=1/planes=1', functools.partial(res_case, mode=X3_BF16, alias=1, planes=1)))
    c.append(('dgrad/bf16/d=3/net_in=alias', functools.partial(dgrad_case, mode=X3_BF16, dilation=3, net_in='alias')))
    c.append(('bwd/bf16/aux0=planes/fp32=0', functools.partial(bwd_case, mode=X3_BF16, aux='planes', fp32=0)))
    c.append(('gate/bf16/R=256/ks=3/d=1/bias=1/cond=1/save1+out_planes',
              functools.partial(gate_case, mode=X3_BF16, R=256, ks=3, dilation=1, bias=1, cond=1, subset=('save1', 'out_planes'))))
    c.append(('head/bf16/alias=net_in/cond=1/relu=1', functools.partial(head_case, mode=X3_BF16, alias='net_in', cond=1, relu=1)))
    return [(n, (lambda K, f=f: f(K))) for n, f in c]


def all_digests(K):
    """{case: {output: sha256}} of the whole table."""
    out = {}
    for name, run in cases():
        out[name] = digest(run(K))
    torch.cuda.synchronize()
    return out
