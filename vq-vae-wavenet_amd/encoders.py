"""The reference's three encoders on the libvqwave engines, behind one interface.

VQVAE picks one class (model._setup_front) and from then on only calls:
    ratio                            audio samples per latent frame
    latent_len(T)                    Tz, or ValueError for a length the encoder cannot take
    segments()                       its tensors of the flat parameter buffer, in order
    init(P, uus, glorot)             their initial values
    named(model, V, out, bn_stats)   the views V of its segments under the reference's variable names
    scratch(dev)                     transposed-kernel scratch of its input-gradient GEMMs (model.T)
    transpose(model)                 fill that scratch at the start of a backward pass
    on_engine(model)                 some of its layers can run on the guarded fp16x3 engine (StepPlan.enc_x3 / enc_wg3)
    workspace(model, ws, train)      its buffers of one (B, T) problem
    forward(model, x, ws, save)      x [B][T] -> ws['z_e'] [B][D][Tz]
    backward(model, x, ws)           ws['dz'] = d loss / d z_e -> its gradients, accumulated into model.G; it also tells
                                     model.grad_sync (where set) when the flat gradient in front of 'pre_w' is final
An encoder keeps constants only: every tensor, switch and stream it uses is the model's, handed in with each call.

`Encoder64` mirrors Encoder/encoder.py:8-26 (class Encoder_64), the default: a k=5 stride-2 conv from the one audio channel,
five k=5 stride-2 convs F -> F, a 1x1 to latent_dim, each followed by relu (not the last) and an inference-mode BatchNorm.

`EncoderMagenta` mirrors Encoder/encoder.py:29-63 (class Encoder_Magenta): shift + mu-law,
causal k=5 conv, then 6 x [1x1 stride-2 conv -> gate / filter k=5 dilated (1,2,4,8,16,16)
causal convs -> tanh(gate) * sigmoid(filter) -> d + 1x1], then a 1x1 to latent_dim.  Every conv is
`conv1d_v2` (wavenet_ops.py:59-90), i.e. the same implicit-GEMM engine as the decoder: the
gate/filter pair is ONE launch with the GATE epilogue (kernels stored side by side), the
residual add is the ACCUM_SPLIT epilogue, the stride-2 1x1 uses in_stride=2 staging.
"""
from collections import OrderedDict

import torch

from . import _alloc as A
from . import kernels as K
from .wavenet import causal_taps, mirrored_taps, side_after, side_mark

BN_EPS = 1e-3  # Keras BatchNormalization default epsilon


def strided_conv_dgrad(dy, wt, dx, B, F, ks, pad_left, T_q, T_in, **split):
    """The input gradient dx [B][F][T_in] of a stride-2 conv of ks taps (F -> F, output gradient dy [B][F][T_q], transposed
    kernel wt) as a transposed conv in two parity launches: output times tau = 2u + p get the taps j with j = p + pad_left
    (mod 2).  split: conv_gemm's split-K arguments (tile, split_k < 0: both launches add their K slices into a zeroed dx)."""
    for p in (0, 1):
        j0 = (p + pad_left) % 2
        K.conv_gemm(x0=dy, w=wt[j0:], w_tap_stride=2 * F * F, out0=dx, B=B, T_in=T_q, T_out=(T_in - p + 1) // 2, M=F, C0=F,
                    taps=[(p + pad_left - j) // 2 for j in range(j0, ks, 2)], out_tstride=2, out_toffset=p, T_store=T_in, **split)


def same_pads(n, k, s):
    """TF 'SAME' padding (left, right) -- SURVEY.md Appendix A-4."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def _suffix(i):      # Keras layer names in creation order: conv1d, conv1d_1, ...
    return '' if i == 0 else '_%d' % i


class Encoder:
    """What the three share: `ratio` audio samples per latent frame, the length check, no layer on the fp16x3 engine."""

    def __init__(self, latent_dim, filters=None):      # (filters: Encoder_64's encoder_filters; the other two have the reference's constants)
        self.D = latent_dim

    def latent_len(self, T):
        if T % self.ratio != 0:
            raise ValueError('length must be a multiple of %d for %s (got %d)' % (self.ratio, self.name, T))
        return T // self.ratio

    def on_engine(self, model):
        return False


class Encoder64(Encoder):
    name, ratio = 'Encoder_64', 64

    def __init__(self, latent_dim, filters):
        self.D, self.F = latent_dim, filters

    # ------------------------------------------------------------------ parameters
    def segments(self):
        F, D = self.F, self.D
        seg = OrderedDict()
        seg['enc_w0'] = (5, F)                 # conv1d/kernel [5,1,F]
        seg['enc_w'] = (5, 5, F, F)            # conv1d_1..5/kernel
        seg['enc_b'] = (6, F)
        seg['enc_w6'] = (F, D)                 # conv1d_6/kernel [1,F,D]
        seg['enc_b6'] = (D,)
        seg['bn_gamma'] = (6 * F + D,)
        seg['bn_beta'] = (6 * F + D,)
        return seg

    def init(self, P, uus, glorot):
        F, D = self.F, self.D
        P['enc_w0'].copy_(glorot((5, F), 5, 1, F))
        P['enc_w'].copy_(glorot((5, 5, F, F), 5, F, F))
        P['enc_w6'].copy_(glorot((F, D), 1, F, D))
        P['bn_gamma'].fill_(1.0)

    def named(self, model, V, out, bn_stats=True):
        F, D = self.F, self.D
        out['encoder/conv1d/kernel'] = V['enc_w0'].reshape(5, 1, F)
        for i in range(1, 6):
            out['encoder/conv1d_%d/kernel' % i] = V['enc_w'][i - 1]
        for i in range(6):
            out['encoder/conv1d%s/bias' % _suffix(i)] = V['enc_b'][i]
        out['encoder/conv1d_6/kernel'] = V['enc_w6'].reshape(1, F, D)
        out['encoder/conv1d_6/bias'] = V['enc_b6']
        for i in range(7):
            n = F if i < 6 else D
            sl = slice(i * F, i * F + n)
            out['encoder/batch_normalization%s/gamma' % _suffix(i)] = V['bn_gamma'][sl]
            out['encoder/batch_normalization%s/beta' % _suffix(i)] = V['bn_beta'][sl]
            if bn_stats:
                out['encoder/batch_normalization%s/moving_mean' % _suffix(i)] = model.bn_mean[sl]
                out['encoder/batch_normalization%s/moving_variance' % _suffix(i)] = model.bn_var[sl]

    def scratch(self, dev):
        F, D = self.F, self.D
        return {'enc_w': A.empty(5, 5, F, F, device=dev), 'enc_w6': A.empty(D, F, device=dev)}

    def transpose(self, model):
        pass        # (made on first use, model._tt: the engine's layers pack their planes straight from the parameters)

    # ------------------------------------------------------------------ workspace
    def on_engine(self, model):         # the long strided layers can run on the guarded fp16x3 engine
        return model.x3_guard and self.F % 256 == 0

    def workspace(self, model, ws, train=True):
        F, D, B, T, Tz, dev = self.F, self.D, ws['B'], ws['T'], ws['Tz'], model.dev
        e = lambda *s: A.empty(*s, device=dev)  # noqa: E731
        h = lambda *s: A.empty(*s, dtype=torch.float16, device=dev)  # noqa: E731
        Tl = ws['Tl'] = [T // (2 ** (i + 1)) for i in range(6)]
        ws['X'] = [e(B, F, t) for t in Tl]         # BN outputs of encoder layers 0..5
        ws['scale'], ws['shift'] = e(6 * F + D), e(6 * F + D)
        if self.on_engine(model):      # fp16x3 engine for layers 1..3 (StepPlan.enc_x3)
            ws['eplanes'] = h(2 * B * F * Tl[0])   # planes of one layer's operand
            ws['ewp'] = h(5, 2 * 5 * F * F)
            ws['enc_amax'] = torch.zeros(12, dtype=torch.int32, device=dev)
            ws['enc_scale'] = torch.ones(12, device=dev)
            if train:
                ws['ewtp'] = h(5, 2 * 5 * F * F)
                if model.wg_planes:     # the planes of each layer's input (space-to-depth) and output gradient are KEPT: the strided weight
                    # gradients read them (p_planes / q_planes) instead of fetching fp32 one float per request (240 MB at B = 8)
                    ws['esp'] = {i: h(2 * B * F * Tl[i - 1]) for i in range(1, 6)}
                    ws['edp'] = {i: h(2 * B * F * Tl[i]) for i in range(1, 6)}
        if train:
            ws['r'] = [e(B, F, t) for t in Tl]     # relu outputs
            ws['y6'] = e(B, D, Tz)
            ws['dX'] = [e(B, F, t) for t in Tl]
            ws['dscale'] = e(6 * F + D)

    @staticmethod
    def _sconv_split(model, ws):
        """Scratch of the strided convs' split-K launches (layers 3-5: 24..78 tiles of 240 K steps on 256 CUs): partial tiles
        of one launch (at most two rounds of 128-row blocks) and the tiles' ticket counters, which every launch leaves at zero."""
        if not model.sw.sconv_split:
            return {}
        slab = lambda: A.empty(torch.cuda.get_device_properties(model.dev).multi_processor_count * 65536, device=model.dev)    # noqa: E731
        return {'split_slab': A.scratch(ws, 'sslab', slab),
                'split_counters': A.scratch(ws, 'scount', lambda: torch.zeros(1024, dtype=torch.int32, device=model.dev))}

    @staticmethod
    def _short_layer_split(M, T_out, B, cus=256):
        """K slices for a conv whose 64x128 tiles (4 resident per CU) cannot fill the chip: aim at ~4 blocks per CU."""
        nb = -(-M // 64) * -(-T_out // 128) * B
        if nb * 2 > 4 * cus:
            return 1
        return max(1, min(8, (4 * cus) // nb))

    @staticmethod
    def _bn_affine(model, ws):
        """Inference-mode BatchNorm as a per-channel affine (encoder.py:20,25; Appendix A-3)."""
        inv = torch.rsqrt(model.bn_var + BN_EPS)
        torch.mul(model.P['bn_gamma'], inv, out=ws['scale'])
        torch.addcmul(model.P['bn_beta'], model.bn_mean, ws['scale'], value=-1.0, out=ws['shift'])
        return inv

    @staticmethod
    def _measure(model, ws, t, slot, target_exp=13):
        """This step's guard scale of tensor t: the exact power of two that puts its max-abs below 2^(target_exp + 1); a non-finite
        value raises the step's range flag (-> fp32 repeat).  Slots of ws['enc_scale'] / ws['enc_amax']: 0 the kernels, i the input
        of layer i, 5 + i d(its conv output).  Returns the scale's 1-element view."""
        amax, scale = ws['enc_amax'][slot:slot + 1], ws['enc_scale'][slot:slot + 1]
        K.f16x3_amax(t, amax, flag=model.x3_flag)
        K.f16x3_update_scales(amax, scale, target_exp=target_exp, flag=model.x3_flag)
        return scale

    # ------------------------------------------------------------------ forward / backward
    def forward(self, model, x, ws, save=True):
        """x [B][T] -> ws['z_e'] [B][D][T/64] (encoder.py:13-26)."""
        P, F, D, B, T = model.P, self.F, self.D, ws['B'], ws['T']
        self._bn_affine(model, ws)
        sc, sh = ws['scale'], ws['shift']
        pl, _ = same_pads(T, 5, 2)
        K.conv_cin1_fwd(x, P['enc_w0'], P['enc_b'][0], ws['X'][0], k=5, stride=2, offset=-pl, relu=True,
                        scale=sc[:F], shift=sh[:F], save_r=ws['r'][0] if save else None)
        Tin = ws['Tl'][0]
        # the long strided layers on the fp16x3 engine (space-to-depth planes): exact power-of-two scales from a
        # max-abs pass over this step's tensors
        ex3 = ws['enc_x3'] = model._plan(ws, ws is model._ws.get((B, T, True))).enc_x3      # (a training workspace: also under encode())
        if ex3:
            es = ws['enc_scale']
            self._measure(model, ws, P['enc_w'], 0, target_exp=14)
            K.f16x3_pack_weights(P['enc_w'], ws['ewp'], 5 * F, F, F, 1.0, count=5, scale_dev=es[0:1], mode=0)
        for i in range(1, 6):
            Tout = ws['Tl'][i]
            pl, _ = same_pads(Tin, 5, 2)
            nsplit = self._short_layer_split(F, Tout, B)
            if i in ex3:
                self._measure(model, ws, ws['X'][i - 1], i)
                epl = ws['esp'][i] if (save and model.wg_planes) else ws['eplanes']
                K.f16x3_split_activations(ws['X'][i - 1], epl, B, F, Tin, scale_dev=es[i:i + 1], mode=K.X3_S2D)
                K.f16x3_strided_conv(xp=epl, wp=ws['ewp'][i - 1], out=ws['X'][i], save_r=ws['r'][i] if save else None,
                                     B=B, T=Tout, Cin=F, M=F, ks=5, pad_left=pl, bias=P['enc_b'][i], bn_scale=sc[i * F:(i + 1) * F],
                                     bn_shift=sh[i * F:(i + 1) * F], relu=True, x_scale=es[i:i + 1], w_scale=es[0:1], **self._sconv_split(model, ws))
            elif nsplit > 1:
                # short layer (T_out down to 104): too few tiles for 256 CUs, but K = 5*768 is long: split-K into the
                # output buffer (plain STORE + atomics), then relu / save / BatchNorm affine as a second, tiny pass
                K.conv_gemm(x0=ws['X'][i - 1], w=P['enc_w'][i - 1], bias=P['enc_b'][i], out0=ws['X'][i], B=B, T_in=Tin,
                            T_out=Tout, M=F, C0=F, in_stride=2, taps=[j - pl for j in range(5)], tile=12, split_k=nsplit)
                K.relu_bn_fwd(ws['X'][i], ws['r'][i] if save else None, sc[i * F:(i + 1) * F], sh[i * F:(i + 1) * F])
            else:
                K.conv_gemm(x0=ws['X'][i - 1], w=P['enc_w'][i - 1], bias=P['enc_b'][i], out0=ws['X'][i],
                            save0=ws['r'][i] if save else None, scale=sc[i * F:(i + 1) * F], shift=sh[i * F:(i + 1) * F],
                            B=B, T_in=Tin, T_out=Tout, M=F, C0=F, in_stride=2, taps=[j - pl for j in range(5)],
                            out_relu=True)
            Tin = Tout
        Tz = ws['Tz']
        K.conv_gemm(x0=ws['X'][5], w=P['enc_w6'], bias=P['enc_b6'], out0=ws['z_e'], save0=ws['y6'] if save else None,
                    scale=sc[6 * F:], shift=sh[6 * F:], B=B, T_in=Tz, T_out=Tz, M=D, C0=F, taps=[0])

    def backward(self, model, x, ws):
        """ws['dz'] = d loss / d z_e -> parameter gradients (encoder.py:13-26 backwards, BN in inference mode)."""
        P, G, F, D = model.P, model.G, self.F, self.D
        B, T, Tz = ws['B'], ws['T'], ws['Tz']
        grad_sync, enc_w0, enc_w_n = model.grad_sync, model.seg_off['enc_w'][0], 5 * F * F      # (one layer's kernel: 11.8 MB)
        sc, dsc = ws['scale'], ws['dscale']
        dsc.zero_()
        dz = ws['dz']
        # BatchNorm / relu backward with its three sums (d scale, d beta, the conv's bias gradient) in one pass per layer
        K.bn_relu_bwd_sums(dz, ws['y6'], None, sc[6 * F:], dz, dscale=dsc[6 * F:], dbeta=G['bn_beta'][6 * F:],
                           dbias=G['enc_b6'])                        # dz := d(conv6 output)
        K.wgrad_gemm(p=ws['X'][5], q0=dz, dw=G['enc_w6'], B=B, T_q=Tz, T_p=Tz, Cp=F, Q0=D, taps=[0])
        K.conv_gemm(x0=dz, w=model._tt('enc_w6'), out0=ws['dX'][5], B=B, T_in=Tz, T_out=Tz, M=F, C0=D, taps=[0])
        main = torch.cuda.current_stream()
        side = model._side_stream() if model.overlap_wgrad else main
        # layers 1..5 on the fp16x3 engine: the input gradient where the forward conv ran there (ws['enc_x3']), the weight
        # gradient (operands split in registers, bias sums riding along) whenever the decoder's ran there this step.  Scales:
        # exact powers of two from max-abs passes over THIS step's tensors (slots: _measure)
        ex3, wg3 = ws['plan'].enc_x3, ws['plan'].enc_wg3
        es = ws.get('enc_scale')
        if ex3:
            K.f16x3_pack_weights_t(P['enc_w'], ws['ewtp'], 5 * F, F, F, F, F * F, 1.0, count=5, scale_dev=es[0:1], mode=0)
        for i in range(5, -1, -1):
            dX, r = ws['dX'][i], ws['r'][i]
            Ti = ws['Tl'][i]
            Tin = ws['Tl'][i - 1] if i > 0 else T
            pl, _ = same_pads(Tin, 5, 2)
            on_c = i in ex3
            on_w = wg3 and 1 <= i <= 5 and Ti % 4 == 0 and B * Ti >= 256 and Tin == 2 * Ti and B * F * Tin * 4 < (1 << 31)
            K.bn_relu_bwd_sums(dX, r, r, sc[i * F:(i + 1) * F], dX, dscale=dsc[i * F:(i + 1) * F],
                               dbeta=G['bn_beta'][i * F:(i + 1) * F],
                               dbias=None if on_w else G['enc_b'][i])   # dX := d(conv_i output); (the engine's wgrad sums the bias itself)
            if on_c or on_w:
                self._measure(model, ws, dX, 5 + i)
                if not on_c:                                         # (the forward pass measured X[i-1] otherwise)
                    self._measure(model, ws, ws['X'][i - 1], i)
            ready = side_mark(main, side)
            # both operands as planes where the forward conv ran on the engine (its space-to-depth input planes were kept):
            # tap j, e = j - pad_left, is parity block e & 1 at row offset e >> 1
            w_planes = on_w and on_c and model.wg_planes
            if w_planes:     # (the split the input gradient needs anyway, into this layer's own buffer, BEFORE the weight gradient)
                K.f16x3_split_activations(dX, ws['edp'][i], B, F, Ti, scale_dev=es[5 + i:6 + i], mode=0)
                ready = side_mark(main, side)
            with side_after(side, ready):                            # weight / bias gradients: nothing downstream waits
                if w_planes:
                    K.f16x3_wgrad(p_planes=ws['esp'][i], p_planes_KC=2 * F // 8, p_tap_chunk=[((j - pl) & 1) * (F // 8) for j in range(5)],
                                  q_planes=ws['edp'][i], dw=G['enc_w'][i - 1], slab=ws['wslab'], B=B, T=Ti, Cp=F, Q0=F,
                                  taps=[(j - pl) >> 1 for j in range(5)], p_scale=es[i:i + 1], q0_scale=es[5 + i:6 + i],
                                  q_total=G['enc_b'][i], mode=0)
                elif on_w:
                    K.f16x3_wgrad(p=ws['X'][i - 1], q0=dX, dw=G['enc_w'][i - 1], slab=ws['wslab'], B=B, T=Ti, Cp=F, Q0=F,
                                  taps=[j - pl for j in range(5)], p_scale=es[i:i + 1], q0_scale=es[5 + i:6 + i], p_stride=2, T_p=Tin,
                                  q_total=G['enc_b'][i], mode=0)
                else:
                    if i == 0:
                        K.conv_cin1_wgrad(x, dX, G['enc_w0'], k=5, stride=2, offset=-pl)
                    else:
                        K.wgrad_gemm(p=ws['X'][i - 1], q0=dX, dw=G['enc_w'][i - 1], B=B, T_q=Ti, T_p=Tin, Cp=F, Q0=F, p_stride=2,
                                     taps=[j - pl for j in range(5)])
                if grad_sync is not None and i >= 2:      # this layer's kernel gradient is final: exchange it under the rest
                    grad_sync.bucket_ready(enc_w0 + (i - 1) * enc_w_n, enc_w0 + i * enc_w_n)      # of the encoder backward
            if i == 0:
                break
            if on_c:
                if not w_planes:
                    K.f16x3_split_activations(dX, ws['eplanes'], B, F, Ti, scale_dev=es[5 + i:6 + i], mode=0)
                K.f16x3_strided_conv(xp=ws['edp'][i] if w_planes else ws['eplanes'], wp=ws['ewtp'][i - 1], out=ws['dX'][i - 1], B=B, T=Ti, Cin=F, M=F, ks=5,
                                     pad_left=pl, dgrad=True, x_scale=es[5 + i:6 + i], w_scale=es[0:1], **self._sconv_split(model, ws))
                continue
            nsplit = self._short_layer_split(F, (Tin + 1) // 2, B)
            if nsplit > 1:
                ws['dX'][i - 1].zero_()        # both parity launches add their K slices into it (split_k < 0)
            strided_conv_dgrad(dX, model._tt('enc_w')[i - 1], ws['dX'][i - 1], B, F, 5, pl, Ti, Tin,
                               tile=12 if nsplit > 1 else 0, split_k=-nsplit if nsplit > 1 else 0)
        if side is not main:
            main.wait_stream(side)
        dsc.addcmul_(model.bn_mean, G['bn_beta'], value=-1.0)         # shift = beta - mean*scale
        torch.mul(dsc, torch.rsqrt(model.bn_var + BN_EPS), out=dsc)
        G['bn_gamma'] += dsc
        if grad_sync is not None:      # what the per-layer buckets above left: the first layers' kernels, biases, BatchNorm, codebook
            grad_sync.bucket_ready(0, enc_w0 + enc_w_n)
            grad_sync.bucket_ready(enc_w0 + 5 * enc_w_n, model.seg_off['pre_w'][0])


class EncoderMagenta(Encoder):
    name, ratio = 'Encoder_Magenta', 64
    FILTERS = 128
    KS = 5
    DIL = [1, 2, 4, 8, 16, 16]     # encoder.py:33

    # ------------------------------------------------------------------ parameters
    def segments(self):
        F, D, L, k = self.FILTERS, self.D, len(self.DIL), self.KS
        seg = OrderedDict()
        seg['mag_pre_w'] = (k, F)            # encoder/preprocess/kernel [5,1,F]
        seg['mag_pre_b'] = (F,)
        seg['mag_d_w'] = (L, F, F)           # .../dilated/kernel [1,F,F] (stride 2)
        seg['mag_d_b'] = (L, F)
        seg['mag_gf_w'] = (L, k, F, 2 * F)   # gate | filter kernels side by side
        seg['mag_gf_b'] = (L, 2 * F)
        seg['mag_r_w'] = (L, F, F)           # .../residual/kernel
        seg['mag_r_b'] = (L, F)
        seg['mag_post_w'] = (F, D)           # encoder/postprocess/kernel
        seg['mag_post_b'] = (D,)
        return seg

    def init(self, P, uus, glorot):
        F, D, L, k = self.FILTERS, self.D, len(self.DIL), self.KS
        P['mag_pre_w'].copy_(uus((k, F), k, 1.0))
        P['mag_d_w'].copy_(uus((L, F, F), F, 1.0))
        P['mag_gf_w'].copy_(uus((L, k, F, 2 * F), k * F, 1.0))
        P['mag_r_w'].copy_(uus((L, F, F), F, 1.0))
        P['mag_post_w'].copy_(uus((F, D), F, 1.0))

    def named(self, model, V, out, bn_stats=True):
        F, D, k = self.FILTERS, self.D, self.KS
        out['encoder/preprocess/kernel'] = V['mag_pre_w'].reshape(k, 1, F)
        out['encoder/preprocess/bias'] = V['mag_pre_b']
        for i in range(len(self.DIL)):
            s = 'encoder/cycle_1/layer_%d' % (i + 1)
            out[s + '/dilated/kernel'] = V['mag_d_w'][i].unsqueeze(0)
            out[s + '/dilated/bias'] = V['mag_d_b'][i]
            out[s + '/gate/kernel'] = V['mag_gf_w'][i][:, :, :F]
            out[s + '/gate/bias'] = V['mag_gf_b'][i][:F]
            out[s + '/filter/kernel'] = V['mag_gf_w'][i][:, :, F:]
            out[s + '/filter/bias'] = V['mag_gf_b'][i][F:]
            out[s + '/residual/kernel'] = V['mag_r_w'][i].unsqueeze(0)
            out[s + '/residual/bias'] = V['mag_r_b'][i]
        out['encoder/postprocess/kernel'] = V['mag_post_w'].unsqueeze(0)
        out['encoder/postprocess/bias'] = V['mag_post_b']

    def scratch(self, dev):
        F, D, L, k = self.FILTERS, self.D, len(self.DIL), self.KS
        return {'mag_d_w': A.empty(L, F, F, device=dev), 'mag_gf_w': A.empty(L, k, 2 * F, F, device=dev),
                'mag_r_w': A.empty(L, F, F, device=dev), 'mag_post_w': A.empty(D, F, device=dev)}

    def transpose(self, model):
        P, Tt = model.P, model.T
        F, D, L, k = self.FILTERS, self.D, len(self.DIL), self.KS
        K.transpose(P['mag_d_w'], Tt['mag_d_w'], L, F, F)
        K.transpose(P['mag_gf_w'], Tt['mag_gf_w'], L * k, F, 2 * F)
        K.transpose(P['mag_r_w'], Tt['mag_r_w'], L, F, F)
        K.transpose(P['mag_post_w'], Tt['mag_post_w'], 1, F, D)

    def workspace(self, model, ws, train=True):
        F, L, B, T, dev = self.FILTERS, len(self.DIL), ws['B'], ws['T'], model.dev
        e = lambda *s: A.empty(*s, device=dev)  # noqa: E731
        Tl = [T // (2 ** (i + 1)) for i in range(L)]
        ws['m_Tl'] = Tl
        # The encoder compands its own input at 256 levels (encoder.py:43) into the decoder's input buffer, which at 256 levels
        # holds the same values (the decoder's backward and this one both read it again).  A decoder at another level keeps
        # that buffer and the labels to itself: the encoder's input gets one of its own.
        ws['m_inputs'] = ws['inputs'] if model.levels == 256 else e(B, T)
        ws['m_en'] = [e(B, F, T)] + [e(B, F, t) for t in Tl]     # en_0 .. en_6
        ws['m_dd'] = [e(B, F, t) for t in Tl]
        ws['m_gated'] = [e(B, F, t) for t in Tl]
        if not train:       # forward only (model.encode): nothing is saved for a backward pass
            ws['m_th'] = ws['m_sg'] = [None] * L
            return
        ws['m_th'] = [e(B, F, t) for t in Tl]
        ws['m_sg'] = [e(B, F, t) for t in Tl]
        ws['m_den'] = [e(B, F, T)] + [e(B, F, t) for t in Tl]    # gradients w.r.t. en_i
        ws['m_dpre'] = [e(B, 2 * F, t) for t in Tl]
        ws['m_ddd'] = [e(B, F, t) for t in Tl]

    # ------------------------------------------------------------------ forward / backward
    def forward(self, model, x, ws, save=True):
        """x [B][T] -> ws['z_e'] [B][D][T/64] (encoder.py:38-63)."""
        P, F, D, k, B, T = model.P, self.FILTERS, self.D, self.KS, ws['B'], ws['T']
        K.wavenet_inputs(x, ws['m_inputs'], ws['labels'] if model.levels == 256 else None)   # shift_right + mu_law_encode
        en = ws['m_en']
        K.conv_cin1_fwd(ws['m_inputs'], P['mag_pre_w'], P['mag_pre_b'], en[0], k=k, stride=1, offset=-(k - 1))
        Tin = T
        for i, d in enumerate(self.DIL):
            To = ws['m_Tl'][i]
            dd = ws['m_dd'][i]
            K.conv_gemm(x0=en[i], w=P['mag_d_w'][i], bias=P['mag_d_b'][i], out0=dd, B=B, T_in=Tin, T_out=To, M=F,
                        C0=F, in_stride=2, taps=[0])                                               # 'dilated'
            K.conv_gemm(x0=dd, w=P['mag_gf_w'][i], bias=P['mag_gf_b'][i], out0=ws['m_gated'][i],
                        save0=ws['m_th'][i] if save else None, save1=ws['m_sg'][i] if save else None, B=B, T_in=To,
                        T_out=To, M=2 * F, C0=F, taps=causal_taps(k, d), epilogue=K.EPI_GATE)
            K.conv_gemm(x0=ws['m_gated'][i], w=P['mag_r_w'][i], bias=P['mag_r_b'][i], out0=en[i + 1], out1=en[i + 1],
                        aux1=dd, B=B, T_in=To, T_out=To, M=F, M0=0, C0=F, taps=[0], epilogue=K.EPI_ACCUM_SPLIT)
            Tin = To
        K.conv_gemm(x0=en[-1], w=P['mag_post_w'], bias=P['mag_post_b'], out0=ws['z_e'], B=B, T_in=Tin, T_out=Tin, M=D,
                    C0=F, taps=[0])

    def backward(self, model, x, ws):
        """ws['dz'] = d loss / d z_e -> parameter gradients (accumulated into model.G)."""
        P, G, Tt = model.P, model.G, model.T
        F, D, k, B, T = self.FILTERS, self.D, self.KS, ws['B'], ws['T']
        L = len(self.DIL)
        en, den = ws['m_en'], ws['m_den']
        dz, Tz = ws['dz'], ws['Tz']
        K.wgrad_gemm(p=en[L], q0=dz, dw=G['mag_post_w'], B=B, T_q=Tz, T_p=Tz, Cp=F, Q0=D, taps=[0])
        K.rowsum(dz, total=G['mag_post_b'])
        K.conv_gemm(x0=dz, w=Tt['mag_post_w'], out0=den[L], B=B, T_in=Tz, T_out=Tz, M=F, C0=D, taps=[0])
        for i in range(L - 1, -1, -1):
            d, To = self.DIL[i], ws['m_Tl'][i]
            Tin = ws['m_Tl'][i - 1] if i > 0 else T
            g_out, dpre, ddd = den[i + 1], ws['m_dpre'][i], ws['m_ddd'][i]
            # en_{i+1} = dd + conv1x1(gated)
            K.wgrad_gemm(p=ws['m_gated'][i], q0=g_out, dw=G['mag_r_w'][i], B=B, T_q=To, T_p=To, Cp=F, Q0=F, taps=[0])
            K.rowsum(g_out, total=G['mag_r_b'][i])
            K.conv_gemm(x0=g_out, w=Tt['mag_r_w'][i], out0=dpre, aux0=ws['m_th'][i], aux1=ws['m_sg'][i], B=B, T_in=To,
                        T_out=To, M=F, C0=F, taps=[0], epilogue=K.EPI_GATE_BWD)
            K.wgrad_gemm(p=ws['m_dd'][i], q0=dpre, dw=G['mag_gf_w'][i], B=B, T_q=To, T_p=To, Cp=F, Q0=2 * F, taps=causal_taps(k, d))
            K.rowsum(dpre, total=G['mag_gf_b'][i])
            K.conv_gemm(x0=dpre, w=Tt['mag_gf_w'][i], out0=ddd, out1=ddd, aux1=g_out, B=B, T_in=To, T_out=To, M=F,
                        M0=0, C0=2 * F, taps=mirrored_taps(k, d), epilogue=K.EPI_ACCUM_SPLIT)
            # dd = conv1x1(en_i, stride 2)
            K.wgrad_gemm(p=en[i], q0=ddd, dw=G['mag_d_w'][i], B=B, T_q=To, T_p=Tin, Cp=F, Q0=F, p_stride=2, taps=[0])
            K.rowsum(ddd, total=G['mag_d_b'][i])
            den[i].zero_()                                       # odd time steps receive no gradient
            K.conv_gemm(x0=ddd, w=Tt['mag_d_w'][i], out0=den[i], B=B, T_in=To, T_out=To, M=F, C0=F, taps=[0],
                        out_tstride=2, out_toffset=0, T_store=Tin)
        K.conv_cin1_wgrad(ws['m_inputs'], den[0], G['mag_pre_w'], k=k, stride=1, offset=-(k - 1))
        K.rowsum(den[0], total=G['mag_pre_b'])
        if model.grad_sync is not None:
            model.grad_sync.bucket_ready(0, model.seg_off['pre_w'][0])


def mel_weight_matrix(num_mel_bins=80, num_spectrogram_bins=201, sample_rate=16000, lower_edge_hertz=20.0,
                      upper_edge_hertz=8000.0):
    """tf.contrib.signal.linear_to_mel_weight_matrix as called by encoder_ops.py:30-36 (HTK mel
    scale, triangular filters, DC bin row zero) -> float32 [num_spectrogram_bins][num_mel_bins]."""
    import numpy as np
    mel = lambda f: 1127.0 * np.log1p(np.asarray(f, dtype=np.float64) / 700.0)  # noqa: E731
    linear = np.linspace(0.0, sample_rate / 2.0, num_spectrogram_bins)[1:]
    spec = mel(linear)[:, None]
    edges = np.linspace(mel(lower_edge_hertz), mel(upper_edge_hertz), num_mel_bins + 2)
    lo, ce, up = edges[:-2][None], edges[1:-1][None], edges[2:][None]
    w = np.maximum(0.0, np.minimum((spec - lo) / (ce - lo), (up - spec) / (up - ce)))
    return torch.from_numpy(np.pad(w, [[1, 0], [0, 0]]).astype(np.float32))


class Encoder2019(Encoder):
    """Encoder/encoder.py:66-98 (class Encoder_2019) + encoder_ops.py:14-70: MFCC-13 front end
    (vqw_mfcc), conv_3_768 -> conv_3_768 + residual -> strided_conv_4_768 -> 2 x (conv + residual)
    -> 4 x (`relu + relu`, i.e. 2*relu(conv): encoder.py:91-93) -> linear_64.  Keras layer names
    conv1d, conv1d_1 .. conv1d_9 in creation order.  The 13 MFCC channels are padded to 16 (zero
    channels / zero kernel rows) for the conv engine.  Needs T % 320 == 0."""
    name, ratio = 'Encoder_2019', 320
    F = 768
    CPAD = 16
    K3 = {1: 0, 3: 1, 4: 2, 5: 3, 6: 4, 7: 5, 8: 6}      # conv index -> slot in the stacked k=3 kernels

    def segments(self):
        F, D = self.F, self.D
        seg = OrderedDict()
        seg['e19_w0'] = (3, self.CPAD, F)        # conv1d/kernel [3,13,768] (+3 zero rows)
        seg['e19_wk3'] = (7, 3, F, F)            # conv1d_{1,3,4,5,6,7,8}/kernel
        seg['e19_w2'] = (4, F, F)                # conv1d_2/kernel (stride 2)
        seg['e19_b'] = (9, F)
        seg['e19_w9'] = (F, D)                   # conv1d_9/kernel [1,768,D]
        seg['e19_b9'] = (D,)
        return seg

    def init(self, P, uus, glorot):
        F, D = self.F, self.D
        P['e19_w0'].zero_()
        P['e19_w0'][:, :13, :].copy_(glorot((3, 13, F), 3, 13, F))
        P['e19_wk3'].copy_(glorot((7, 3, F, F), 3, F, F))
        P['e19_w2'].copy_(glorot((4, F, F), 4, F, F))
        P['e19_w9'].copy_(glorot((F, D), 1, F, D))

    def named(self, model, V, out, bn_stats=True):
        F, D = self.F, self.D
        out['encoder/conv1d/kernel'] = V['e19_w0'][:, :13, :]
        for i, slot in self.K3.items():
            out['encoder/conv1d_%d/kernel' % i] = V['e19_wk3'][slot]
        out['encoder/conv1d_2/kernel'] = V['e19_w2']
        for i in range(9):
            out['encoder/conv1d%s/bias' % _suffix(i)] = V['e19_b'][i]
        out['encoder/conv1d_9/kernel'] = V['e19_w9'].unsqueeze(0)
        out['encoder/conv1d_9/bias'] = V['e19_b9']

    def scratch(self, dev):
        F, D = self.F, self.D
        return {'e19_wk3': A.empty(7, 3, F, F, device=dev), 'e19_w2': A.empty(4, F, F, device=dev),
                'e19_w9': A.empty(D, F, device=dev), 'e19_mel': mel_weight_matrix().to(dev),
                'e19_ones': torch.ones(F, device=dev), 'e19_twos': torch.full((F,), 2.0, device=dev),
                'e19_zeros': torch.zeros(F, device=dev)}

    def transpose(self, model):
        P, Tt = model.P, model.T
        F, D = self.F, self.D
        K.transpose(P['e19_wk3'], Tt['e19_wk3'], 21, F, F)
        K.transpose(P['e19_w2'], Tt['e19_w2'], 4, F, F)
        K.transpose(P['e19_w9'], Tt['e19_w9'], 1, F, D)

    def workspace(self, model, ws, train=True):
        F, B, T, dev = self.F, ws['B'], ws['T'], model.dev
        e = lambda *s: A.empty(*s, device=dev)  # noqa: E731
        Fr = T // 160
        Tz = Fr // 2
        ws['e_Fr'] = Fr
        ws['e_mf'] = e(B, self.CPAD, Fr)
        Ts = [Fr, Fr] + [Tz] * 7
        ws['e_T'] = Ts
        ws['e_a'] = [e(B, F, t) for t in Ts]          # layer outputs a_0 .. a_8
        if not train:       # forward only (model.encode)
            ws['e_r'] = [None] * len(Ts)
            return
        ws['e_r'] = [e(B, F, t) for t in Ts]          # relu outputs before residual / doubling
        ws['e_da'] = [e(B, F, t) for t in Ts]         # gradients w.r.t. a_i
        ws['e_dc'] = [e(B, F, Fr), e(B, F, Tz)]       # masked conv-output gradients (per resolution)

    def forward(self, model, x, ws, save=True):
        P, Tt = model.P, model.T
        F, D, B = self.F, self.D, ws['B']
        Fr, Tz = ws['e_Fr'], ws['Tz']
        a, r = ws['e_a'], ws['e_r']
        K.mfcc(x, Tt['e19_mel'], ws['e_mf'])                                        # encoder_ops.py:14-43
        k3 = [-1, 0, 1]                                                            # 'same', k=3: pads (1,1)
        K.conv_gemm(x0=ws['e_mf'], w=P['e19_w0'], bias=P['e19_b'][0], out0=a[0], B=B, T_in=Fr, T_out=Fr, M=F,
                    C0=self.CPAD, taps=k3, out_relu=True)
        K.conv_gemm(x0=a[0], w=P['e19_wk3'][0], bias=P['e19_b'][1], out0=a[1], save0=r[1] if save else None, aux1=a[0], B=B, T_in=Fr,
                    T_out=Fr, M=F, C0=F, taps=k3, out_relu=True)
        pl, _ = same_pads(Fr, 4, 2)
        K.conv_gemm(x0=a[1], w=P['e19_w2'], bias=P['e19_b'][2], out0=a[2], B=B, T_in=Fr, T_out=Tz, M=F, C0=F,
                    in_stride=2, taps=[j - pl for j in range(4)], out_relu=True)
        for i in (3, 4):
            K.conv_gemm(x0=a[i - 1], w=P['e19_wk3'][self.K3[i]], bias=P['e19_b'][i], out0=a[i], save0=r[i] if save else None,
                        aux1=a[i - 1], B=B, T_in=Tz, T_out=Tz, M=F, C0=F, taps=k3, out_relu=True)
        for i in (5, 6, 7, 8):                                                     # net = relu + relu
            K.conv_gemm(x0=a[i - 1], w=P['e19_wk3'][self.K3[i]], bias=P['e19_b'][i], out0=a[i], save0=r[i] if save else None,
                        scale=Tt['e19_twos'], shift=Tt['e19_zeros'], B=B, T_in=Tz, T_out=Tz, M=F, C0=F, taps=k3,
                        out_relu=True)
        K.conv_gemm(x0=a[8], w=P['e19_w9'], bias=P['e19_b9'], out0=ws['z_e'], B=B, T_in=Tz, T_out=Tz, M=D, C0=F,
                    taps=[0])

    def backward(self, model, x, ws):
        P, G, Tt = model.P, model.G, model.T
        F, D, B = self.F, self.D, ws['B']
        Fr, Tz = ws['e_Fr'], ws['Tz']
        a, r, da, dc = ws['e_a'], ws['e_r'], ws['e_da'], ws['e_dc']
        dz = ws['dz']
        k3, k3b = [-1, 0, 1], [1, 0, -1]
        ones, twos = Tt['e19_ones'], Tt['e19_twos']
        K.wgrad_gemm(p=a[8], q0=dz, dw=G['e19_w9'], B=B, T_q=Tz, T_p=Tz, Cp=F, Q0=D, taps=[0])
        K.rowsum(dz, total=G['e19_b9'])
        K.conv_gemm(x0=dz, w=Tt['e19_w9'], out0=da[8], B=B, T_in=Tz, T_out=Tz, M=F, C0=D, taps=[0])
        for i in (8, 7, 6, 5):                       # a_i = 2*relu(conv_i(a_{i-1}))
            K.bn_relu_bwd(da[i], r[i], twos, da[i])
            K.rowsum(da[i], total=G['e19_b'][i])
            K.wgrad_gemm(p=a[i - 1], q0=da[i], dw=G['e19_wk3'][self.K3[i]], B=B, T_q=Tz, T_p=Tz, Cp=F, Q0=F, taps=k3)
            K.conv_gemm(x0=da[i], w=Tt['e19_wk3'][self.K3[i]], out0=da[i - 1], B=B, T_in=Tz, T_out=Tz, M=F, C0=F,
                        taps=k3b)
        for i in (4, 3):                             # a_i = relu(conv_i(a_{i-1})) + a_{i-1}
            K.bn_relu_bwd(da[i], r[i], ones, dc[1])
            K.rowsum(dc[1], total=G['e19_b'][i])
            K.wgrad_gemm(p=a[i - 1], q0=dc[1], dw=G['e19_wk3'][self.K3[i]], B=B, T_q=Tz, T_p=Tz, Cp=F, Q0=F, taps=k3)
            K.conv_gemm(x0=dc[1], w=Tt['e19_wk3'][self.K3[i]], out0=da[i - 1], out1=da[i - 1], aux1=da[i], B=B,
                        T_in=Tz, T_out=Tz, M=F, M0=0, C0=F, taps=k3b, epilogue=K.EPI_ACCUM_SPLIT)
        # a_2 = relu(strided_conv_4(a_1))
        K.bn_relu_bwd(da[2], a[2], ones, da[2])
        K.rowsum(da[2], total=G['e19_b'][2])
        pl, _ = same_pads(Fr, 4, 2)
        K.wgrad_gemm(p=a[1], q0=da[2], dw=G['e19_w2'], B=B, T_q=Tz, T_p=Fr, Cp=F, Q0=F, p_stride=2,
                     taps=[j - pl for j in range(4)])
        strided_conv_dgrad(da[2], Tt['e19_w2'], da[1], B, F, 4, pl, Tz, Fr)
        # a_1 = relu(conv_1(a_0)) + a_0
        K.bn_relu_bwd(da[1], r[1], ones, dc[0])
        K.rowsum(dc[0], total=G['e19_b'][1])
        K.wgrad_gemm(p=a[0], q0=dc[0], dw=G['e19_wk3'][0], B=B, T_q=Fr, T_p=Fr, Cp=F, Q0=F, taps=k3)
        K.conv_gemm(x0=dc[0], w=Tt['e19_wk3'][0], out0=da[0], out1=da[0], aux1=da[1], B=B, T_in=Fr, T_out=Fr, M=F,
                    M0=0, C0=F, taps=k3b, epilogue=K.EPI_ACCUM_SPLIT)
        # a_0 = relu(conv_0(mfcc))
        K.bn_relu_bwd(da[0], a[0], ones, da[0])
        K.rowsum(da[0], total=G['e19_b'][0])
        K.wgrad_gemm(p=ws['e_mf'], q0=da[0], dw=G['e19_w0'], B=B, T_q=Fr, T_p=Fr, Cp=self.CPAD, Q0=F, taps=k3)
        if model.grad_sync is not None:
            model.grad_sync.bucket_ready(0, model.seg_off['pre_w'][0])


# the reference's class names (Encoder/encoder.py:8,29,66)
Encoder_64 = Encoder64
Encoder_Magenta = EncoderMagenta
Encoder_2019 = Encoder2019
