"""Seeded cases for the MAIN LOOP of the fp16x3 conv kernels (f16x3_mainloop: how operands reach LDS and in which order the
stages of the ring are filled), beside tests/epilogue_cases.py, whose table pins the epilogues.  Every case returns the raw bytes
of every output it wrote; tests/golden/make_x3_loop_digests.py hashes them into tests/golden/x3_loop_digests.json and
tests/test_x3_loop_gpu.py compares against that file.

What the epilogue table does not reach:
  * dilations 1, 2, 256 and 512 at T = 512, ks = 3, B = 2, gate conv and its input gradient: taps that shift by less than a tile,
    by half a batch row and by a whole one -- the first and the last column tile of each batch row have rows before / behind their
    own batch row, which must read zero and not the neighbouring batch row's samples (or a stale stage of the ring);
  * a head conv over Cin = 3 * 256 channels: 48 K steps, the ring wraps 12 to 16 times;
  * the stride-2 convs (vqw_f16x3_strided_conv), forward and input gradient, on every block shape the launcher's automatic
    choice can return (2: 128 rows, 3: 256, 4: 192, 5: 64) at T_out = 256 (two column tiles, one batch row each), and the
    split-K launches at T_out = 64 (one partial column tile that holds both batch rows), with Cin = 64 and 128: 20 / 40 K steps
    forward, 12 + 8 / 24 + 16 for the two output parities of the input gradient.  (The entry point takes Cin >= 64; a split
    input gradient needs 8 steps per part, i.e. Cin >= 128.)
Both block heights (mode 0: 256 rows, X3_HALF: 128 rows) and one bf16 case per kernel."""
import functools

import torch

import epilogue_cases as E

B, T, DEV = E.B, E.T, E.DEV
DILATIONS = (1, 2, 256, 512)
SCONV_SHAPES = (2, 3, 4, 5)
KS, PL = 5, 1       # the encoder's stride-2 convs: five taps, SAME padding = one zero in front


# ---------------------------------------------------------------- head conv, long K
@functools.lru_cache(maxsize=None)
def _head_inputs(K, mode):
    Cin, R = 3 * 256, 256
    x = E._rand(601, B, Cin, T)
    w = E._rand(602, Cin, R, scale=0.05)
    xp, wp = E._planes(2 * B * Cin * T), E._planes(2 * Cin * R)
    K.f16x3_split_activations(x, xp, B, Cin, T, mode=mode)
    K.f16x3_pack_weights(w, wp, Cin, R, R, 256.0, mode=mode)
    return dict(Cin=Cin, R=R, xp=xp, wp=wp, bias=E._rand(603, R), net=E._rand(604, B, R, T), mask=E._rand(605, B, R, T),
                out_scale=torch.tensor([2.0], device=DEV))


def head_case(K, mode):
    i = _head_inputs(K, mode)
    R = i['R']
    net_out = torch.zeros(B, R, T, device=DEV)
    amax, flag = E._slots()
    pl = E._planes(2 * B * R * T)
    K.f16x3_out_conv(epi=2, xp=i['xp'], wp=i['wp'], B=B, T=T, R=R, S=0, Cin=i['Cin'], w_scale_inv=1.0 / 256.0, net_in=i['net'],
                     net_out=net_out, aux0=i['mask'], bias=i['bias'], net_out_planes=pl, out_scale=i['out_scale'], out_amax=amax,
                     flag=flag, mode=mode)
    return dict(net_out=net_out, planes=pl, amax=amax, flag=flag)


# ---------------------------------------------------------------- stride-2 convs
@functools.lru_cache(maxsize=None)
def _sconv_inputs(K, Tout, Cin, M):
    Tin = 2 * Tout
    x = E._rand(701 + Tout + Cin, B, Cin, Tin)
    w = E._rand(702 + Cin + M, KS, Cin, M, scale=0.05)
    dy = E._rand(703 + Tout + M, B, M, Tout, scale=1e-4)
    sc = torch.tensor([8.0, 256.0, 2.0 ** 22], device=DEV)                 # x, w, dy
    xp, wp = E._planes(2 * B * Cin * Tin), E._planes(2 * KS * Cin * M)
    dyp, wtp = E._planes(2 * B * M * Tout), E._planes(2 * KS * M * Cin)
    K.f16x3_split_activations(x, xp, B, Cin, Tin, scale_dev=sc[0:1], mode=K.X3_S2D)
    K.f16x3_pack_weights(w, wp, KS * Cin, M, M, 1.0, scale_dev=sc[1:2], mode=0)
    K.f16x3_split_activations(dy, dyp, B, M, Tout, scale_dev=sc[2:3], mode=0)
    K.f16x3_pack_weights(w.permute(0, 2, 1).contiguous(), wtp, KS * M, Cin, Cin, 1.0, scale_dev=sc[1:2], mode=0)
    return dict(xp=xp, wp=wp, dyp=dyp, wtp=wtp, sc=sc, bias=E._rand(704 + M, M, scale=0.5), bsc=E._rand(705 + M, M), bsh=E._rand(706 + M, M, scale=0.3))


@functools.lru_cache(maxsize=None)
def _split_scratch():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return torch.zeros(cus * 65536, device=DEV), torch.zeros(1024, dtype=torch.int32, device=DEV)


def sconv_case(K, Tout, Cin, M, shape, ksplit, dgrad):
    """Forward: Cin -> M channels; input gradient: the planes of dy [B][M][Tout] through the transposed kernel -> dx [B][Cin][2 Tout]."""
    i = _sconv_inputs(K, Tout, Cin, M)
    sc = i['sc']
    kw = {}
    if ksplit > 1:
        slab, cnt = _split_scratch()
        kw = dict(split_slab=slab, split_counters=cnt, ksplit=ksplit)
    if dgrad:
        dx = torch.zeros(B, Cin, 2 * Tout, device=DEV)
        K.f16x3_strided_conv(xp=i['dyp'], wp=i['wtp'], out=dx, B=B, T=Tout, Cin=M, M=Cin, ks=KS, pad_left=PL, dgrad=True, x_scale=sc[2:3],
                             w_scale=sc[1:2], shape=shape, **kw)
        out = dict(dx=dx)
    else:
        y, r = torch.zeros(B, M, Tout, device=DEV), torch.zeros(B, M, Tout, device=DEV)
        K.f16x3_strided_conv(xp=i['xp'], wp=i['wp'], out=y, save_r=r, B=B, T=Tout, Cin=Cin, M=M, ks=KS, pad_left=PL, bias=i['bias'],
                             bn_scale=i['bsc'], bn_shift=i['bsh'], relu=True, x_scale=sc[0:1], w_scale=sc[1:2], shape=shape, **kw)
        out = dict(out=y, save_r=r)
    if ksplit > 1:
        out['counters'] = kw['split_counters'].clone()
    return out


# ---------------------------------------------------------------- the table
def cases():
    """[(name, thunk(K) -> {output: tensor})] in a fixed order."""
    c = []
    for mn, m in E.MODES + (('bf16', E.X3_BF16),):
        for d in (DILATIONS if mn != 'bf16' else (256,)):
            c.append(('gate/%s/d=%d' % (mn, d), functools.partial(E.gate_case, mode=m, R=256, ks=3, dilation=d, bias=1, cond=1,
                                                                   subset=('save1', 'out_planes'))))
            c.append(('dgrad/%s/d=%d' % (mn, d), functools.partial(E.dgrad_case, mode=m, dilation=d, net_in='distinct')))
        c.append(('head/%s/Cin=768' % mn, functools.partial(head_case, mode=m)))
    # unsplit: the input gradient's "M" (rows of the block) is the forward conv's Cin, so the row count 768 (a multiple of 64, 128,
    # 192 and 256) sits on the other side there
    for Cin in (64, 128):
        for shape in SCONV_SHAPES:
            c.append(('sconv/fwd/T=256/Cin=%d/shape=%d' % (Cin, shape), functools.partial(sconv_case, Tout=256, Cin=Cin, M=768, shape=shape, ksplit=1, dgrad=False)))
            c.append(('sconv/dgrad/T=256/Cin=%d/shape=%d' % (Cin, shape), functools.partial(sconv_case, Tout=256, Cin=768, M=Cin, shape=shape, ksplit=1, dgrad=True)))
        # split-K (128-row blocks only): two blocks per tile (and per parity)
        c.append(('sconv/fwd/T=64/Cin=%d/split=2' % Cin, functools.partial(sconv_case, Tout=64, Cin=Cin, M=256, shape=0, ksplit=2, dgrad=False)))
    c.append(('sconv/fwd/T=64/Cin=128/split=4', functools.partial(sconv_case, Tout=64, Cin=128, M=256, shape=0, ksplit=4, dgrad=False)))
    c.append(('sconv/dgrad/T=64/Cin=128/split=2', functools.partial(sconv_case, Tout=64, Cin=256, M=128, shape=0, ksplit=2, dgrad=True)))
    c.append(('sconv/dgrad/T=64/Cin=256/split=2', functools.partial(sconv_case, Tout=64, Cin=256, M=256, shape=0, ksplit=2, dgrad=True)))
    return [(n, (lambda K, f=f: f(K))) for n, f in c]


def all_digests(K):
    """{case: {output: sha256}} of the whole table."""
    out = {}
    for name, run in cases():
        out[name] = E.digest(run(K))
    torch.cuda.synchronize()
    return out
