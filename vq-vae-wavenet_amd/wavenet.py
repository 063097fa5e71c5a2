"""The trainable conditional WaveNet on MI355X: what model.VQVAE (the decoder behind the VQ-VAE's front) and prior.LatentPrior
(a WaveNet over VQ codes) both are.

Mirrors Decoder/decoder.py:12-62 (WavenetDecoder) and Decoder/WaveNet/wavenet.py:24-172 (Wavenet) of the reference, with the
optimiser of model.py:109-130.  The reference builds a TF graph and lets TF autodiff + the TF runtime do the
work; here one training step is an explicit forward + backward sequence of libvqwave kernels
on (batch, channel, time) fp32 tensors.  PyTorch only owns device memory and streams.

Parameters live in ONE flat fp32 buffer (so gradients are one contiguous all-reduce payload
and Adam+EMA is one kernel); `named_parameters()` exposes them under the reference's TF
variable names and shapes.
"""
import contextlib
import json
import math
import os
import time
import sys
from collections import OrderedDict, namedtuple

import torch

from . import _alloc as A
from . import kernels as K
from .utils import mu_law_levels

DEFAULT_ENGINE = 'f16x3'

# The model's VQW_* switches (tools/README.md), read ONCE, when a model is constructed (WaveNet.sw): field name = variable name.
_ON = 'overlap wgrad_pp head_x3 cond_proj enc_x3 sconv_split wgrad_batch wgrad_x3 wgrad_qp enc_wgrad_x3'.split()         # off with '0'
_IS1 = dict(x3_half='1', x3_half_skip='0', x3_half_bwd='1', x3_half_dgrad='0', x3_half_head='1', defer_guard='0', save_tanh='0', save_gated='0')  # on with '1'
Switches = namedtuple('Switches', ['engine', 'gate_f16x3', 'dtype', 'skip_groups', 'wg_gate_batch', 'wg_res_batch'] + _ON + list(_IS1))
StepPlan = namedtuple('StepPlan', 'save f16x3 f16x3_out f16x3_skip x3_used gd calib ngrp WS GS GSh head_x3 keep_xp drop_th drop_g dgrad_x3 gbwd_x3 '
                      'wg_x3 batched qp pp gate_batch res_batch enc_x3 enc_wg3 why')      # which engine carries what in one pass (WaveNet._step_plan)


def read_switches(dtype='f32'):
    """The environment's switches with their defaults (dtype: the config's; VQW_DTYPE overrides it)."""
    env = lambda name, dflt: os.environ.get('VQW_' + name.upper(), dflt)                           # noqa: E731
    batch = lambda name, dflt: max(1, min(K.WGRAD_MAX_BATCH, int(env(name, dflt))))                 # noqa: E731
    return Switches(engine=env('engine', DEFAULT_ENGINE), gate_f16x3=env('gate_f16x3', '0'), dtype=env('dtype', dtype), skip_groups=max(1, int(env('skip_groups', '1'))),
                    wg_gate_batch=batch('wg_gate_batch', '6'), wg_res_batch=batch('wg_res_batch', '29'), **{n: env(n, '1') != '0' for n in _ON},
                    **{n: env(n, d) == '1' for n, d in _IS1.items()})



def load_configs(model_json='model_parameters.json', wavenet_json=None):
    """Same two JSON files as the reference (train.py:54-61, wavenet.py:10-13)."""
    with open(model_json) as f:
        m = json.load(f)
    with open(wavenet_json or m['wavenet_parameters']) as f:
        w = json.load(f)
    assert len(w['dilation_rates']) == w['num_cycles'] * w['num_cycle_layers']  # wavenet.py:13
    return m, w


def prefill_window(t_end, ks, dilations, pre_k, ratio):
    """The window of a prompt of t_end steps that a prefill computes (WaveNet.decoder_states): (W, s0, end).
    W = (ks-1) * sum(dilations) + pre_k is how far back a step can reach into the generator's state after the prompt: layer l's
    oldest queued step t_end - (ks-1) d_l looks back (ks-1) * sum_{j<l} d_j + pre_k - 1 inputs more, and the input of step t
    is the prompt's value at t - 1.  s0 = max(0, t_end - W) rounded down to a multiple of ratio (whole condition frames);
    end = t_end rounded up to a multiple of ratio (the columns past t_end are zeros: the convs are causal, nothing before
    t_end sees them).  The zero history that the window's left edge brings (its first input included) only reaches steps
    before t_end - W + 1, which the state does not keep.  t_end = 0: an empty window (0, 0)."""
    if t_end < 0 or ratio < 1:
        raise ValueError('prefill_window: t_end must be >= 0 and ratio >= 1 (got %d, %d)' % (t_end, ratio))
    W = (ks - 1) * sum(dilations) + pre_k
    s0 = max(0, t_end - W) // ratio * ratio
    end = -(-t_end // ratio) * ratio
    return W, s0, end


def causal_taps(ks, d):
    """The input shifts of a causal conv of ks taps with dilation d, oldest tap first: tap j reads t - (ks - 1 - j) d."""
    return [-(ks - 1 - j) * d for j in range(ks)]


def mirrored_taps(ks, d):
    """causal_taps mirrored: the shifts of that conv's input gradient (tap j reads t + (ks - 1 - j) d of the output gradient)."""
    return [(ks - 1 - j) * d for j in range(ks)]


def side_mark(main, side):
    """Fork work to the side stream, first half: the point on main it may start behind, as a recorded event (None when
    side is main: nothing to wait for)."""
    if side is main:
        return None
    mark = torch.cuda.Event()
    mark.record(main)
    return mark


@contextlib.contextmanager
def side_after(side, mark):
    """... second half: what runs inside is enqueued on the side stream, behind side_mark's mark (on the current stream when
    there is none).  Nothing downstream waits for it until main waits for the side stream."""
    if mark is None:
        yield
        return
    with torch.cuda.stream(side):
        side.wait_event(mark)
        yield


def mix_seed(*words):
    """splitmix64 over integer words: the seed of a device generator that is a pure function of them (reconstruct's uniforms; the VQ-VAE's draws)."""
    seed = 0
    for v in words:
        seed = (seed ^ (int(v) & 0xFFFFFFFFFFFFFFFF)) + 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF
        seed = (seed ^ (seed >> 30)) * 0xBF58476D1CE4E5B9 & 0xFFFFFFFFFFFFFFFF
        seed = (seed ^ (seed >> 27)) * 0x94D049BB133111EB & 0xFFFFFFFFFFFFFFFF
        seed ^= seed >> 31
    return seed >> 1


def layer_scope(i, num_cycle_layers, scope='decoder'):
    return '%s/cycle_%d/layer_%d' % (scope, 1 + i // num_cycle_layers, 1 + i % num_cycle_layers)


class _WgradSchedule:
    """The residual stack's weight gradients, bias sums and share of the condition gradient, beside the backward chain
    (WaveNet._backward_stack): where the chain writes per layer, and when the launches go out.  The chain calls
        buffers(l) -> (dpre, dplanes, dnet_next)    before layer l: where its gate backward and input gradient write
        layer(l, dnet, dpre, ready)                 behind layer l's two launches (dnet: d loss / d net[l + 1], None at the top
                                                    layer; ready: the mark on main behind gate backward, side_mark)
        finish()                                    behind layer 0
    Nothing downstream waits for what a schedule launches: it forks to the side stream (main itself without VQW_OVERLAP), which
    the chain joins after finish()."""

    def __init__(self, model, ws, dskip, main, side):
        self.m, self.ws, self.dskip, self.main, self.side = model, ws, dskip, main, side
        self.plan, self.sc = ws['plan'], model._guards(ws['plan'])[0]


class _PerLayerWgrads(_WgradSchedule):
    """A layer's launches as soon as its dpre is ready: the plane engine's two kernels (VQW_WGRAD_BATCH=0), or the fp32 engine's
    with their row sums.  Two streams: the chain stays on main and these run on the side stream, so one kernel's thin last round
    is filled by the other's blocks.  dnet / dpre are rings (3 / 2 buffers): the chain may run two layers ahead of the side stream
    before it has to wait for it."""

    def __init__(self, model, ws, dskip, main, side):
        super().__init__(model, ws, dskip, main, side)
        self.done = {}       # layer -> the event behind its launches on the side stream
        self.seg = None if self.plan.wg_x3 else A.empty(ws['B'], 2 * model.R, ws['Tz'], device=model.dev)

    def buffers(self, l):
        if (l + 2) in self.done:
            self.main.wait_event(self.done[l + 2])            # dpre[l % 2] and dnet[(l - 1) % 3] are free again
        return self.ws['dpre_ring'][l % 2], self.ws.get('dp'), self.ws['dnet_ring'][(l - 1) % 3]

    def layer(self, l, dnet, dpre, ready):
        m, ws, sc, dskip = self.m, self.ws, self.sc, self.dskip
        G, R, S, B, T, Tz, dce = m.G, m.R, m.S, ws['B'], ws['T'], ws['Tz'], ws['dcondenc']
        top, taps, md = dnet is None, causal_taps(m.ks, m.dil[l]), m.x3_mode_bwd
        with side_after(self.side, ready):
            if self.plan.wg_x3:    # weight gradients on the fp16 pipe too: operands split in registers with the planes' guard scales;
                # the bias sums and the condition gradient (sums of dpre per condition frame) come out of the same kernels
                K.f16x3_wgrad(p=ws['gated'][l], q0=dskip, q1=dnet, dw=G['out_w'][l], slab=ws['wslab'], B=B,
                              T=T, Cp=R, Q0=S, Q1=0 if top else R, lddw=S + R, taps=[0], q0_scale=sc('G'), q1_scale=sc('G'),
                              q_total=None if top else G['out_b'][l], total_cols=(S, S + R), mode=md)
                K.f16x3_wgrad(p=ws['net'][l], q0=dpre, dw=G['gated_w'][l], slab=ws['wslab'], B=B, T=T, Cp=R, Q0=2 * R,
                              taps=taps, p_scale=sc('X', l), q0_scale=sc('DP', l),
                              q_seg=dce.view(-1)[l * 2 * R * Tz:], seg_T=Tz, seg_bstride=m.Mall * Tz, mode=md)
            else:
                K.wgrad_gemm(p=ws['gated'][l], q0=dskip, q1=dnet, dw=G['out_w'][l], B=B, T_q=T, T_p=T,
                             Cp=R, Q0=S, Q1=0 if top else R, lddw=S + R, taps=[0])
                if not top:
                    K.rowsum(dnet, total=G['out_b'][l][S:])
                K.wgrad_gemm(p=ws['net'][l], q0=dpre, dw=G['gated_w'][l], B=B, T_q=T, T_p=T, Cp=R, Q0=2 * R, taps=taps)
                K.rowsum(dpre, seg_out=self.seg, total=G['gated_b'][l], seg=ws['ratio'])
                dce[:, l * 2 * R:(l + 1) * 2 * R].copy_(self.seg)
            if self.side is not self.main:
                self.done[l] = torch.cuda.Event()
                self.done[l].record(self.side)

    def finish(self):
        pass


class _BatchedWgrads(_WgradSchedule):
    """The plane engine's default: dpre and dnet of EVERY layer are kept (4.9 GB at B = 8 instead of rings of 2 / 3 buffers) and
    the weight gradients of several layers go out as ONE launch (vqw_f16x3_wgrad_batch):
      * the skip halves of all layers' 1x1 kernels, dW_s[l] = gated[l] (x) dskip -- dskip is the same tensor for every
        layer -- at once, before the first layer: 60 tiles x 4 K splits instead of 30 x (2 tiles x 80 splits);
      * the gate kernels of up to 6 layers (VQW_WG_GATE_BATCH) (layers whose tap shifts are all multiples of 4 and the others --
        dilations 1 and 2 -- in separate batches: the latter need the kernel's slower unaligned-window variant);
      * the residual halves, dW_r[l] = gated[l] (x) dnet[l+1], of up to 29 layers (VQW_WG_RES_BATCH).
    A launch writes tiles x splits <= CUs partial 256x256 tiles to the slab whatever its batch size: per layer the slab
    traffic (2 x 61 MB per single launch, 7.3 GB per step) falls with the batch size, dskip is read once per XCD instead
    of once per layer, and 68 reductions become ~10.
    ... and (qp) dpre is kept as the operand PLANES gate backward writes for the input gradient anyway: the gate kernels' weight
    gradient reads its q operand from them (transposed LDS reads, vqw_f16x3_wgrad q_planes) and gate backward no longer
    writes fp32 dpre at all (109 of its 312 MB per layer); (pp) p = the layer's input planes and the gated planes likewise."""

    def __init__(self, model, ws, dskip, main, side):
        super().__init__(model, ws, dskip, main, side)
        m, plan, sc = model, self.plan, self.sc
        R, S, L, B, T = m.R, m.S, m.L, ws['B'], ws['T']
        A.scratch(ws, 'dnet_all', lambda: [A.empty(B, R, T, device=m.dev) for _ in range(L)])       # dnet_all[l] = d loss / d net[l]
        if plan.qp:
            A.scratch(ws, 'dp_all', lambda: [A.empty(2 * B * 2 * R * T, dtype=torch.float16, device=m.dev) for _ in range(L)])
        else:
            A.scratch(ws, 'dpre_all', lambda: [A.empty(B, 2 * R, T, device=m.dev) for _ in range(L)])
        self.pend_gate, self.pend_res = {False: [], True: []}, []      # layers waiting for a launch (gate: by tap alignment)
        # the skip halves of all layers (dskip: the first S / 8 chunks of the gradient planes)
        qsk = dict(q_planes=ws['gr'], q_planes_KC=(S + R) // 8, q_planes_scale=plan.GS) if (plan.qp and plan.gbwd_x3) else dict(q0=dskip)
        for i0 in range(0, L, K.WGRAD_MAX_BATCH):
            self._launch([dict(dw=m.G['out_w'][i].view(-1), **self._gated(i)) for i in range(i0, min(L, i0 + K.WGRAD_MAX_BATCH))],
                         Q0=S, lddw=S + R, taps=[0], q0_scale=sc('G'), **qsk)

    def _gated(self, i):         # layer i's gated output as the p operand
        m, ws = self.m, self.ws
        return dict(p_planes=ws['gp'], p_planes_kc0=i * (m.R // 8), p_planes_KC=m.L * (m.R // 8)) if self.plan.pp else dict(p=ws['gated'][i])

    def _launch(self, probs, **common):
        ws = self.ws
        with side_after(self.side, side_mark(self.main, self.side)):
            K.f16x3_wgrad_batch(probs, slab=ws['wslab'], B=ws['B'], T=ws['T'], Cp=self.m.R, mode=self.m.x3_mode_bwd, **common)

    def buffers(self, l):
        ws = self.ws
        return (None, ws['dp_all'][l], ws['dnet_all'][l]) if self.plan.qp else (ws['dpre_all'][l], ws.get('dp'), ws['dnet_all'][l])

    def layer(self, l, dnet, dpre, ready):
        odd = any(shift % 4 for shift in mirrored_taps(self.m.ks, self.m.dil[l]))
        self.pend_gate[odd].append(l)
        if len(self.pend_gate[odd]) >= self.plan.gate_batch:      # 6: 36 tiles x 7 K splits = 252 blocks (tools/wg_batch_sweep.sh)
            self._flush_gate(odd)
        if dnet is not None:         # layer l + 1 wrote dnet[l + 1] before this one (the top layer has no dnet: its residual kernel gets no gradient)
            self.pend_res.append(l)
            if len(self.pend_res) >= self.plan.res_batch:
                self._flush_res()

    def _flush_gate(self, odd):
        m, ws, plan, sc = self.m, self.ws, self.plan, self.sc
        layers, self.pend_gate[odd] = self.pend_gate[odd], []
        if layers:
            R, Tz, dce = m.R, ws['Tz'], ws['dcondenc']
            self._launch([dict(dw=m.G['gated_w'][i], taps=causal_taps(m.ks, m.dil[i]),
                               p_scale=sc('X', i), q0_scale=sc('DP', i), q_seg=dce.view(-1)[i * 2 * R * Tz:],
                               **(dict(p_planes=ws['xp_all'][i]) if plan.pp else dict(p=ws['net'][i])),
                               **(dict(q_planes=ws['dp_all'][i], q_planes_scale=plan.GS) if plan.qp else dict(q0=ws['dpre_all'][i]))) for i in layers],
                         Q0=2 * R, seg_T=Tz, seg_bstride=m.Mall * Tz)

    def _flush_res(self):
        m, ws, S = self.m, self.ws, self.m.S
        layers, self.pend_res = self.pend_res, []
        if layers:
            self._launch([dict(q0=ws['dnet_all'][i + 1], dw=m.G['out_w'][i].view(-1)[S:], q_total=m.G['out_b'][i][S:], **self._gated(i))
                          for i in layers], Q0=m.R, lddw=S + m.R, taps=[0], q0_scale=self.sc('G'), total_cols=(0, m.R))

    def finish(self):
        self._flush_gate(False)
        self._flush_gate(True)
        self._flush_res()


class WaveNet:
    """Decoder/WaveNet/wavenet.py:24-172 with its training step: flat parameters, engine switches and range guards, workspaces,
    forward, backward, Adam + EMA, teacher-forced scoring.  What makes the condition (and, for the prior, the input stage) is the
    subclass's: the hooks below named _front_* / _setup_front / _init_front / _named_front / _encode / _decode_input /
    _backward_input / _backward_front / _length_unit / losses."""

    scope = 'decoder'      # name scope of the WaveNet's variables (named_parameters)
    _recon_gen = None      # the device generator of reconstruct's uniforms
    _jitter_step = None    # the step whose forward pass is running inside train_step (_forward_step); None: a pass outside a step (forward(), evaluate, ...)
    _accumulate = 1        # micro-batches per optimiser step (accumulate; 1 = off: the step is what it always was)
    _accum_k = 0           # micro-steps already in the open window (accum_index)
    _acc = None            # the window's running sum, one more n_flat buffer: made at the first accumulating step

    def __init__(self, model_cfg, wavenet_cfg, num_speakers, device='cuda', seed=0):
        self.m, self.w = model_cfg, wavenet_cfg
        self.dev = torch.device(device)
        self.S_spk = num_speakers
        sw = self.sw = read_switches(model_cfg.get('dtype', 'f32'))      # after this line nothing in the class reads the environment
        self._setup_front(model_cfg, num_speakers)
        w = wavenet_cfg
        self.dil = list(w['dilation_rates'])
        self.L = len(self.dil)
        self.ks = w['kernel_size']
        self.R, self.S, self.Q = w['residual_filters'], w['skip_filters'], w['quantization_channels']
        # the mu-law level of labels, decoder input and generated audio: Q at 512 and 1024, otherwise 256 (which leaves every
        # other Q exactly as it has always run; only 256, 512 and 1024 are mu-law models).  LatentPrior has no mu-law.
        self.levels = mu_law_levels(self.Q)
        if w['dilation_filters'] != self.R or w['preprocess']['filters'] != self.R:
            raise NotImplementedError('dilation_filters / preprocess filters must equal residual_filters '
                                      '(the reference adds them: wavenet.py:73)')
        self.pre_k = w['preprocess']['kernel_size']
        self.Mall = self.L * 2 * self.R + self.S  # all local-condition projections side by side
        self.receptive_field = sum(self.dil) * (self.ks - 1) + 1 + self.pre_k - 1  # wavenet.py:16-17
        self.schedule = [(int(k), float(v)) for k, v in model_cfg['learning_rate_schedule'].items()]
        self.global_step = 0
        self._clip_norm, self._gn = None, None     # clipping by global norm (clip_norm): off
        self.grad_sync = None   # parallel.GradAllReduce when training data-parallel
        self.overlap_wgrad = sw.overlap                                  # decoder backward on two streams
        # Engine of the decoder's contractions.  VQW_ENGINE=f16x3: fp32 operands as two fp16 planes, three
        # MFMA terms on the fp16 matrix pipe, fp32 accumulate, with device-side range guards (per-tensor power-of-two
        # scales from measured max-abs values; a step whose planes would leave fp16's range is repeated on the fp32
        # engine).  VQW_ENGINE=fp32: the fp32-MFMA engine everywhere.  VQW_GATE_F16X3=1..5 (development ladder, fixed
        # scales, no guards): 1 gate convs; 2 + the 1x1 skip/residual convs; 3 skip path as ONE contraction; 4 + the gate
        # convs' input gradient; 5 + gate backward.
        engine, ladder = sw.engine, sw.gate_f16x3
        if engine not in ('fp32', 'f16x3'):
            raise ValueError("VQW_ENGINE must be 'fp32' or 'f16x3' (got %r)" % engine)
        # VQW_DTYPE=bf16 (BASELINE.json configs[4]: bf16 storage + fp32 accumulate): the same kernels with ONE bf16 plane per
        # operand and one bf16 MFMA per product; master weights, optimiser state and the residual stream stay fp32
        self.bf16 = sw.dtype == 'bf16'
        # mode bits of the plane engine: bf16, and the block height of its conv kernels per call site -- 128-row blocks (two
        # per CU) for the forward gate conv + residual 1x1 (decoder forward loop 6.05 vs 7.13 ms, tools/x3_chain.py) and for
        # gate backward, 256-row blocks for the K = 7680 skip contraction and the input gradient (whole step, same box:
        # 34.1 ms against 35.0 with 256-row blocks everywhere): VQW_X3_HALF, _SKIP, _BWD, _DGRAD
        self.x3_mode = K.X3_BF16 if self.bf16 else 0
        half = lambda on: self.x3_mode | (K.X3_HALF_BLOCKS if on else 0)  # noqa: E731
        self.x3_mode_fwd = half(sw.x3_half)                # gate conv + residual 1x1
        self.x3_mode_skip = half(sw.x3_half_skip)          # the all-layers skip contraction
        self.x3_mode_bwd = half(sw.x3_half_bwd)            # gate backward
        self.x3_mode_dgrad = half(sw.x3_half_dgrad)        # input gradient
        self.x3_mode_head = half(sw.x3_half_head)          # postprocess1 / 2 and their input gradients
        self.x3_guard = engine == 'f16x3' and ladder == '0' and not self.bf16
        self.x3_all = self.x3_guard or self.bf16          # the plane engine carries every decoder contraction, or none
        if self.x3_all:
            ladder = '5'
        self.gate_f16x3 = ladder in ('1', '2', '3', '4', '5')
        self.out_f16x3 = ladder in ('2', '3', '4', '5')
        self.skip_f16x3 = ladder in ('3', '4', '5')
        self.dgrad_f16x3 = ladder in ('4', '5')
        self.gbwd_f16x3 = ladder == '5'
        self.wg_planes = sw.wgrad_pp    # weight gradients read p from operand planes too
        self._x3_active = True         # False while a step is being repeated on the fp32 engine
        self._x3_warned = set()        # (B, T) shapes already reported as running on the fp32 engine
        self.x3_fallbacks = 0          # steps repeated on the fp32 engine because a plane left fp16's range
        self.x3_steps = 0              # steps that ran on the fp16x3 engine
        self._side = None
        self._build_layout()
        self._init_params(seed)
        self._ws = {}
        self.loss_buf = torch.zeros(4, device=self.dev)  # [CE sum, sum of min distances, -, -]
        # per-call-site tile choices of the conv engine (10*MT+NT; 0 = library heuristic), from
        # tools/bench_kernels.py on MI355X at B=8, T=6656: block counts are 13*2^k, so the tile
        # that balances best over 256 CUs differs per GEMM shape
        self.tiles = {'out': 12, 'gate_bwd': 12, 'dgrad': 12}
        # guard state of the fp16x3 engine: one power-of-two scale + one max-abs collector per tensor kind
        #   WG all gate kernels | WO all 1x1 skip/residual kernels | G = dskip and every dnet (they share one contraction)
        #   X[l] input planes of layer l (l = 0..L) | DP[l] d pre-activation of layer l
        L = self.L
        #   SK relu(skip) planes | H1 relu(postprocess1) planes | DH d postprocess1 | WH the three kernels around the stack
        n = 3 + 2 * L + 1
        self.SL = {'WG': 0, 'WO': 1, 'G': 2, 'X': 3, 'DP': 3 + L + 1, 'SK': n, 'H1': n + 1, 'DH': n + 2, 'WH': n + 3, 'N': n + 4}
        self.x3_scale = torch.ones(self.SL['N'], device=self.dev)
        self.x3_scale[self.SL['G']] = 2.0 ** 20          # first step: |d loss / d logits| <= 1 / (B T)
        self.x3_scale[self.SL['DP']:self.SL['SK']] = 2.0 ** 20
        self.x3_scale[self.SL['DH']] = 2.0 ** 20
        self.head_x3 = sw.head_x3
        self.x3_amax = torch.zeros(self.SL['N'], dtype=torch.int32, device=self.dev)
        self.x3_flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.x3_void = torch.zeros(1, dtype=torch.int32, device=self.dev)      # deferred mode: a flagged step is waiting to be repeated
        self._guard_sets = {}                   # (sc, am, flag) per kind of pass (_guards)
        self.defer_guard = sw.defer_guard       # read the range flag one step late (train_step)
        self._pending, self._void_host, self._void_slot, self._in_step = [], None, 0, False
        # the condition projections (K = Cc ~ 80, rows of Tz ~ 104 frames) on their own fp32-MFMA kernels (csrc/cond_proj.hip)
        self.cond_proj = self.Cc <= 128 and self.Mall % 4 == 0 and sw.cond_proj
        self.host_enqueue_ms = None

    def _setup_front(self, cfg, num_speakers):
        """What feeds the WaveNet's condition; sets Cc (condition channels), Cc_ref (the reference's count) and whatever the other hooks read (hook)."""
        raise NotImplementedError

    def _build_layout(self):
        R, S, Q, L, ks, Cc = self.R, self.S, self.Q, self.L, self.ks, self.Cc
        seg = OrderedDict()  # internal (grouped) tensors of the flat buffer
        self._front_segments(seg)
        seg['pre_w'] = self._pre_w_shape()
        seg['pre_b'] = (R,)
        seg['skip0_w'] = (R, S)
        seg['skip0_b'] = (S,)
        seg['gated_w'] = (L, ks, R, 2 * R)
        seg['gated_b'] = (L, 2 * R)
        seg['cond_w'] = (Cc, self.Mall)        # [layer0 | layer1 | ... | postprocess1]
        seg['out_w'] = (L, R, S + R)           # skip | residual 1x1 kernels side by side
        seg['out_b'] = (L, S + R)
        seg['post1_w'] = (S, S)
        seg['post1_b'] = (S,)
        seg['post2_w'] = (S, Q)
        seg['post2_b'] = (Q,)
        off = 0
        self.seg_off = {}
        for n, shp in seg.items():
            self.seg_off[n] = (off, shp)
            off += (math.prod(shp) + 3) // 4 * 4  # keep every segment 16-byte aligned
        self.n_flat = off
        self.seg_shapes = seg

    def _front_segments(self, seg):
        """Flat-buffer segments in front of the WaveNet's (hook)."""
        raise NotImplementedError

    def _pre_w_shape(self):
        """The preprocess kernel: [pre_k][R] over the one input channel (prior: [pre_k][k][R] over one-hot codes)."""
        return (self.pre_k, self.R)

    def _views(self, flat):
        return {n: flat[o:o + math.prod(shp)].view(shp) for n, (o, shp) in self.seg_off.items()}

    def _init_params(self, seed):
        dev = self.dev
        self.flat = torch.zeros(self.n_flat, device=dev)
        self.grad = torch.zeros(self.n_flat, device=dev)
        self.adam_m = torch.zeros(self.n_flat, device=dev)
        self.adam_v = torch.zeros(self.n_flat, device=dev)
        self.P = self._views(self.flat)
        self.G = self._views(self.grad)
        g = torch.Generator().manual_seed(seed)

        def uus(shape, fan, factor):   # tf.uniform_unit_scaling_initializer
            lim = math.sqrt(3.0 / fan) * factor
            return (torch.rand(shape, generator=g) * 2 - 1) * lim

        def glorot(shape, k, cin, cout):  # Keras glorot_uniform
            lim = math.sqrt(6.0 / (k * cin + k * cout))
            return (torch.rand(shape, generator=g) * 2 - 1) * lim

        R, S, Q, L, ks, Cc = self.R, self.S, self.Q, self.L, self.ks, self.Cc
        P = self.P
        self._init_front(P, uus, glorot)
        pre_shape = self._pre_w_shape()
        P['pre_w'].copy_(uus(pre_shape, math.prod(pre_shape[:-1]), 1.0))          # wavenet_ops.py:69
        P['skip0_w'].copy_(uus((R, S), R, 1.0))
        P['gated_w'].copy_(uus((L, ks, R, 2 * R), ks * R, 1.0))
        P['cond_w'].copy_(uus((Cc, self.Mall), self.Cc_ref, 1.0))
        P['out_w'].copy_(uus((L, R, S + R), R, 1.0))
        P['post1_w'].copy_(uus((S, S), S, 1.0))
        P['post2_w'].copy_(uus((S, Q), S, 1.0))
        self.ema = self.flat.clone()     # ExponentialMovingAverage shadows start at the variables
        self.E = self._views(self.ema)
        # scratch: per-tap transposed kernels for the input-gradient GEMMs
        self._poison_T = []
        with A.record(self._poison_T):
            self._alloc_scratch()

    def _init_front(self, P, uus, glorot):
        """Initial values of the _front_segments (hook)."""
        raise NotImplementedError

    def _alloc_scratch(self):
        dev = self.dev
        R, S, Q, L, ks, Cc = self.R, self.S, self.Q, self.L, self.ks, self.Cc
        self.T = {
            'gated_w': A.empty(L, ks, 2 * R, R, device=dev),
            'out_w': A.empty(L, S + R, R, device=dev),
            'post1_w': A.empty(S, S, device=dev),
            'post2_w': A.empty(Q, S, device=dev),
            'skip0_w': A.empty(S, R, device=dev),
            'cond_w': A.empty(self.Mall, Cc, device=dev),
        }
        self.T.update(self._front_scratch())

    def _front_scratch(self):
        """Transposed-kernel scratch of the front's input-gradient GEMMs, by name (hook; none)."""
        return {}

    # ------------------------------------------------------------------ reference-name views
    def _named(self, V, bn_stats=True):
        """Reference TF variable name -> tensor (copy) with the reference shape."""
        R, S, L = self.R, self.S, self.L
        out = OrderedDict()
        self._named_front(V, out, bn_stats)
        sc = self.scope
        out[sc + '/preprocess/kernel'] = V['pre_w'].reshape(self.pre_k, -1, R)
        out[sc + '/preprocess/bias'] = V['pre_b']
        out[sc + '/skip/kernel'] = V['skip0_w'].reshape(1, R, S)
        out[sc + '/skip/bias'] = V['skip0_b']
        ncl = self.w['num_cycle_layers']
        for l in range(L):
            s = layer_scope(l, ncl, sc)
            out[s + '/gated/kernel'] = V['gated_w'][l]
            out[s + '/gated/bias'] = V['gated_b'][l]
            out[s + '/gated/local_condition/kernel'] = V['cond_w'][:self.Cc_ref, l * 2 * R:(l + 1) * 2 * R].unsqueeze(0)
            out[s + '/skip/kernel'] = V['out_w'][l][:, :S].unsqueeze(0)
            out[s + '/skip/bias'] = V['out_b'][l][:S]
            out[s + '/residual/kernel'] = V['out_w'][l][:, S:].unsqueeze(0)
            out[s + '/residual/bias'] = V['out_b'][l][S:]
        out[sc + '/postprocess1/kernel'] = V['post1_w'].reshape(1, S, S)
        out[sc + '/postprocess1/bias'] = V['post1_b']
        out[sc + '/postprocess1/local_condition/kernel'] = V['cond_w'][:self.Cc_ref, L * 2 * R:].unsqueeze(0)
        out[sc + '/postprocess2/kernel'] = V['post2_w'].reshape(1, S, self.Q)
        out[sc + '/postprocess2/bias'] = V['post2_b']
        return out

    def _named_front(self, V, out, bn_stats=True):
        """The _front_segments under the reference's names (hook)."""
        raise NotImplementedError

    def named_parameters(self, ema=False):
        """Copies of all variables under the reference's names (ema=True: the EMA shadows
        that generate.py:88-90 restores)."""
        self.finish_steps()
        return OrderedDict((k, v.detach().clone()) for k, v in self._named(self.E if ema else self.P).items())

    def named_gradients(self):
        self.finish_steps()
        return OrderedDict((k, v.detach().clone()) for k, v in self._named(self.G, bn_stats=False).items())

    def load_named(self, params, also_ema=True):
        """Load variables given under the reference's names (any device)."""
        self.finish_steps()
        dst = self._named(self.P)
        for name, view in dst.items():
            if name not in params:
                raise KeyError('missing variable ' + name)
            view.copy_(torch.as_tensor(params[name]).to(self.dev).reshape(view.shape))
        if also_ema:
            self.ema.copy_(self.flat)

    def use_ema_weights(self):
        """generate.py:88-90: restore the EMA shadow variables into the live variables."""
        self.flat.copy_(self.ema)

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B, T, train=True):
        """Buffers of one (B, T) problem, cached.  train=False: only what the front's forward pass (_encode) writes
        (model.encoding of generate.py:92) -- about 3 KB per audio sample instead of the 136 KB per sample of the
        training workspace (saved decoder activations of 30 layers + backward buffers).  train='score': the forward-only
        workspace of evaluate() (_score_workspace)."""
        key = (B, T, train)
        if key in self._ws:
            return self._ws[key]
        if not train and (B, T, True) in self._ws:
            return self._ws[(B, T, True)]
        rec = []
        with A.record(rec):
            ws = self._build_workspace(B, T, train)
        ws['_poison'] = rec          # (VQW_POISON=1: refilled with NaN at the start of every step)
        self._ws[key] = ws
        return ws

    def _build_workspace(self, B, T, train):
        ws = self._front_workspace(B, T, train is True)
        if not train:
            return ws
        if train == 'score':
            return self._score_workspace(ws)
        dev, R, S, Q, L, T = self.dev, self.R, self.S, self.Q, self.L, ws['T']
        e = lambda *s: A.empty(*s, device=dev)  # noqa: E731
        ws['condenc'] = e(B, self.Mall, ws['Tz'])
        ws['net'] = [e(B, R, T) for _ in range(L + 1)]
        ws['skip'] = e(B, S, T)
        ws['gated'] = [e(B, R, T) for _ in range(L)]
        ws['th'] = [e(B, R, T) for _ in range(L)]
        ws['sg'] = [e(B, R, T) for _ in range(L)]
        self._plane_buffers(ws, True)
        ws['h1'] = e(B, S, T)
        ws['logits'] = e(B, Q, T)
        # backward
        ws['dnet'] = e(B, R, T)
        ws['dpre'] = e(B, 2 * R, T)
        ws['dnet_ring'] = [ws['dnet'], e(B, R, T), e(B, R, T)]      # ping-pong sets for the two-stream backward
        ws['dpre_ring'] = [ws['dpre'], e(B, 2 * R, T)]
        ws['dcondenc'] = e(B, self.Mall, ws['Tz'])
        ws['dcond'] = e(B, self.Cc, ws['Tz'])
        ws['bskip'] = e(S)
        self._front_workspace_train(ws)
        return ws

    def _head_on_engine(self):          # the convs around the stack (skip start, postprocess1 / 2) can run on the plane engine
        return self.x3_all and self.S % 256 == 0 and self.Q % 256 == 0

    def _keeps_layer_planes(self):      # the input planes of EVERY layer are kept (1.6 GB at B = 8) for the weight gradients (p_planes)
        return self.x3_all and self.wg_planes

    def _plane_buffers(self, ws, train):
        """The decoder's operand planes (fp16 pairs / bf16) of a training workspace (train: with what only the backward pass reads) or a score workspace."""
        if not self.gate_f16x3:
            return
        R, S, Q, L, ks, B, T = self.R, self.S, self.Q, self.L, self.ks, ws['B'], ws['T']
        h = lambda *s: A.empty(*s, dtype=torch.float16, device=self.dev)  # noqa: E731
        ws['xp'] = h(2 * B * R * T)
        if train and self._keeps_layer_planes():
            ws['xp_all'] = [ws['xp']] + [h(2 * B * R * T) for _ in range(L)]
        ws['wp_all'] = h(L, 2 * ks * R * 2 * R)
        ws['wp'] = [ws['wp_all'][l] for l in range(L)]
        ws['gp'] = h(2 * B * R * T * (L if self.skip_f16x3 else 1))
        if train and self.dgrad_f16x3:
            ws['dp'], ws['wdg'] = h(2 * B * 2 * R * T), h(L, 2 * ks * 2 * R * R)
            if self.gbwd_f16x3:     # gr: the [dskip | dnet] lifted planes
                ws['gr'], ws['wgb'], ws['wgb_top'] = h(2 * B * (S + R) * T), h(L, 2 * (S + R) * R), h(2 * S * R)
        if self.skip_f16x3:
            ws['wskip'], ws['wres'] = h(2 * L * R * S), h(L, 2 * R * R)
            if self._head_on_engine():
                # relu(skip) / d postprocess1 (S channels); relu(postprocess1) (S) / d logits (Q channels: more than S at 1024 levels)
                ws['hp'], ws['hp2'] = h(2 * B * S * T), h(2 * B * max(S, Q) * T)
                for name, n_ in (('wskip0', R * S), ('wpost1', S * S), ('wpost2', S * Q)):
                    for sfx in (('', 't') if train else ('',)):      # (+ 't': the transposed kernel of the input gradient)
                        ws[name + sfx] = h(2 * n_)
                if train:     # |d loss / d logits| <= 1 / (B T): a fixed power-of-two scale, max-abs below 2^13
                    ws['dl_scale'] = torch.full((1,), 2.0 ** math.floor(math.log2(2.0 ** 13 * B * T)), device=self.dev)
        ws['wop_all'] = h(L, 2 * R * (S + R))
        ws['wop'] = [ws['wop_all'][l] for l in range(L)]

    def _score_workspace(self, ws):
        """The decoder's buffers for a pass with save=False on top of the front's forward buffers (evaluate): no per-layer
        fp32 activations (two ping-pong net buffers and one gated buffer, aliased into the lists _decode_layers indexes), ONE
        input-plane buffer for all layers (the keep_xp = False path), the gated planes of all layers (the skip contraction
        over K = L*R reads them), no tanh / sigmoid and no backward buffers."""
        dev, R, S, Q, L, B, T = self.dev, self.R, self.S, self.Q, self.L, ws['B'], ws['T']
        e = lambda *s: A.empty(*s, device=dev)  # noqa: E731
        ws['condenc'] = e(B, self.Mall, ws['Tz'])
        pong = [e(B, R, T), e(B, R, T)]
        ws['net'] = [pong[l & 1] for l in range(L + 1)]
        ws['skip'] = e(B, S, T)
        ws['gated'] = [e(B, R, T)] * L
        self._plane_buffers(ws, False)
        ws['h1'] = e(B, S, T)
        ws['logits'] = e(B, Q, T)
        ws['nll'], ws['entropy'] = e(B, T), e(B, T)
        return ws

    def _front_workspace(self, B, T, train):
        """The (B, T) workspace up to the condition: B, T, Tz, ratio, inputs / labels, the front's buffers, ws['cond'] (hook)."""
        raise NotImplementedError

    def _front_workspace_train(self, ws):
        """Backward buffers of the front (hook)."""
        raise NotImplementedError

    # ------------------------------------------------------------------ forward pieces
    def _encode(self, x, spk, ws, save=True):
        """The front's forward pass -> ws['cond'] [B][Cc][Tz] (hook)."""
        raise NotImplementedError

    def _wslab(self, ws):
        """Slab of the engine's weight-gradient kernels: the partial 256x256 tiles of ONE launch.  The launcher cuts K so that
        tiles x K splits <= the device's CU count (vqw_device_cus), hence one 256x256 fp32 tile per CU."""
        return A.scratch(ws, 'wslab', lambda: A.empty(torch.cuda.get_device_properties(self.dev).multi_processor_count * 65536, device=self.dev))

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        return self._side

    def _forward_step(self, x, spk, step, lengths=None):
        """forward() as a pass of training step `step`: the only passes in which a front does what belongs to a training step alone."""
        self._jitter_step = step
        try:
            return self.forward(x, spk, lengths=lengths) if lengths is not None else self.forward(x, spk)
        finally:
            self._jitter_step = None

    def _step_plan(self, B, T, Tz, save, active):
        """The StepPlan of one pass over a (B, T) problem with Tz condition frames: a pure function of the model's constants, self.sw and its arguments
        (no tensors, no workspace, no launches).  save: a training pass on a training workspace (False: the score workspace); active: self._x3_active."""
        sw, R, S, L = self.sw, self.R, self.S, self.L
        # fp16x3 needs whole 256-step tiles inside a batch row, 128-channel blocks and one condition frame per 32 steps;
        # |w| < 255 and |net| < 65504 (fp16 range of the leading planes) are assumed, not checked
        f16x3 = self.gate_f16x3 and T % 256 == 0 and R % 128 == 0 and (T // Tz) % 32 == 0
        f16x3_skip = f16x3 and self.skip_f16x3 and R % 256 == 0 and S % 256 == 0
        f16x3_out = f16x3 and self.out_f16x3 and R % 256 == 0 and S % 256 == 0    # the 1x1 skip + residual conv too; it hands the next layer its planes
        off = self.x3_all and not (f16x3_skip and active)   # guarded / bf16 engine: all of it or none of it
        why = None if not (off and active) else ('length %d is not a multiple of 256' % T if T % 256 else
                                                 'residual / skip widths %d / %d are not multiples of 256' % (R, S) if (R % 256 or S % 256) else
                                                 '%d samples per condition frame is not a multiple of 32' % (T // Tz))
        if off:
            f16x3 = f16x3_skip = f16x3_out = False
        # the skip contraction over all layers reads L*R/8 chunks of the gated planes through 32-bit offsets: at most 2 GiB
        # per plane and launch, so a large batch cuts it into groups of layers (batch 16 x 6656: 2 groups; one up to B*T = 139 k)
        ngrp = sw.skip_groups                               # (VQW_SKIP_GROUPS forces groups at small shapes: tests)
        while f16x3_skip and (L % ngrp or 2 * (L // ngrp) * R * B * T >= (1 << 31)):
            ngrp += 1
        full = f16x3_skip and self.x3_all                   # x3_used
        gd = self.x3_guard and f16x3_skip
        head_x3 = full and self.head_x3 and self._head_on_engine() and T % 32 == 0
        # layer l's input planes: kept per layer for the weight gradients where the skip contraction runs on the engine (then
        # every layer hands its successor planes), else one buffer (slot L: the planes of net[L], which nothing reads)
        keep_xp = save and self._keeps_layer_planes() and f16x3_skip
        # the guarded engine's gate backward forms tanh = gated / sigmoid itself: tanh is not stored (54 MB less per layer and gate
        # conv, 166 -> 157 us); VQW_SAVE_TANH=1 stores it
        drop_th = full and self.gbwd_f16x3 and not sw.save_tanh
        # Gate backward and the gate convs' input gradient on the plane engine.  Guarded engine: the gradient planes carry
        # device-side power-of-two scales (slots G and DP[l]); development ladder (VQW_GATE_F16X3=4,5): a fixed lift by 2^20
        # (d(loss)/d(logits) is bounded by 1 / (B T); |dpre| < 0.06 assumed there, not checked).
        dgrad_x3 = self.dgrad_f16x3 and T % 256 == 0 and R % 256 == 0 and (full or not self.x3_all)
        gbwd_x3 = dgrad_x3 and self.gbwd_f16x3 and S % 256 == 0
        wg_x3 = full and gbwd_x3 and T % 32 == 0 and sw.wgrad_x3
        batched = wg_x3 and sw.wgrad_batch                  # several layers' weight gradients per launch (backward)
        pp = batched and keep_xp                            # ... their p operands from the kept input planes and the gated planes
        # ... and then nothing reads the fp32 gated output (gate backward and the 1x1 kernels' weight gradients take the gated
        # planes): the gate conv does not write it (54 MB less per layer)
        drop_g = gd and pp and drop_th and not sw.save_gated
        enc_x3, enc = self._front_plan(B, T, save, active)
        return StepPlan(      # (WS, GS: 1.0 where the scales live on the device; enc_wg3: head_x3 or wg_x3 = this step's backward makes the slab)
            save=save, f16x3=f16x3, f16x3_out=f16x3_out, f16x3_skip=f16x3_skip, x3_used=full, gd=gd, calib=self.x3_guard and not active,
            ngrp=ngrp, WS=1.0 if gd else 256.0, GS=1.0 if gd else float(2 ** 20), GSh=1.0 if self.x3_guard else float(2 ** 20),
            head_x3=head_x3, keep_xp=keep_xp, drop_th=drop_th, drop_g=drop_g, dgrad_x3=dgrad_x3, gbwd_x3=gbwd_x3, wg_x3=wg_x3,
            batched=batched, qp=batched and sw.wgrad_qp, pp=pp, gate_batch=sw.wg_gate_batch, res_batch=sw.wg_res_batch, enc_x3=enc_x3,
            enc_wg3=(head_x3 or wg_x3) and enc and sw.enc_wgrad_x3, why=why)

    def _front_plan(self, B, T, save, active):
        """The front's share of a StepPlan: (enc_x3 = its layers on the fp16x3 engine in this pass, whether its weight gradients can
        run there at all) (hook; none)."""
        return (), False

    def _plan(self, ws, save):          # _step_plan of a pass over ws, computed once per (save, _x3_active)
        plans, key = ws.setdefault('_plans', {}), (save, self._x3_active)
        if key not in plans:
            plans[key] = self._step_plan(ws['B'], ws['T'], ws['Tz'], save, self._x3_active)
        return plans[key]

    def _slots(self, buf, on):
        """The accessor of the guard slots of buf = x3_scale or x3_amax: sc('X', l), am('G') give the 1-element view of slot (name, i); None where the guards are off."""
        return (lambda name, i=0: buf[self.SL[name] + i:self.SL[name] + i + 1]) if on else (lambda name, i=0: None)

    def _guards(self, plan):
        """(sc, am, flag) of any stage of a pass, forward or backward: the accessors of the guard's scales and max-abs collectors
        (_slots) and the range flag, each off (None) unless the plan runs the guarded engine.  calib: the fp32 repeat of a step
        measures what the planes would have held, so its collectors are on (nothing of it runs on the plane engine).  Built once
        per kind of pass: the buffers are the model's for its lifetime."""
        key = (plan.gd, plan.gd or plan.calib)
        if key not in self._guard_sets:
            self._guard_sets[key] = (self._slots(self.x3_scale, key[0]), self._slots(self.x3_amax, key[1]), self.x3_flag if key[0] else None)
        return self._guard_sets[key]

    def _decode_prologue(self, x, ws, save=True):
        """Everything of the decoder's forward pass that does not depend on the front: inputs / labels, the preprocess conv
        (wavenet.py:33-44), this step's guard scales and weight planes, the skip start (wavenet.py:53-54).  Leaves the plan of
        the step as ws['plan'] (for _decode_layers and the backward pass) and returns it."""
        P, R, S, Q, L, B, T = self.P, self.R, self.S, self.Q, self.L, ws['B'], ws['T']
        plan = ws['plan'] = self._plan(ws, save)
        if plan.why and (B, T) not in self._x3_warned:
            self._x3_warned.add((B, T))
            print('[vqwave] batch %d x length %d runs on the fp32-MFMA engine (about half the speed of the %s engine): %s'
                  % (B, T, 'bf16' if self.bf16 else 'fp16x3', plan.why), file=sys.stderr, flush=True)
        self._decode_input(x, ws)
        net, gd, WS, ngrp, md = ws['net'], plan.gd, plan.WS, plan.ngrp, self.x3_mode_fwd
        ws['skip_groups'], ws['x3_used'] = ngrp if plan.f16x3_skip else 0, plan.x3_used
        sc, am, flag = self._guards(plan)
        if gd:
            K.f16x3_amax(P['gated_w'], am('WG'), flag=flag)
            K.f16x3_amax(P['out_w'], am('WO'), flag=flag)
            K.f16x3_amax(net[0], am('X', 0), flag=flag)
            # weights and the first layer's input: exact scales (amax < 2^14 after scaling); the collectors restart
            K.f16x3_update_scales(self.x3_amax[:2], self.x3_scale[:2], target_exp=14, flag=flag)
            K.f16x3_update_scales(am('X', 0), sc('X', 0), target_exp=13, flag=flag)
        if plan.head_x3:      # the three kernels around the stack share one scale (bf16 planes need none)
            if gd:
                for name in ('skip0_w', 'post1_w', 'post2_w'):
                    K.f16x3_amax(P[name], am('WH'), flag=flag)
                K.f16x3_update_scales(am('WH'), sc('WH'), target_exp=14, flag=flag)
            K.f16x3_pack_weights(P['skip0_w'], ws['wskip0'], R, S, S, 1.0, scale_dev=sc('WH'), mode=md)
            K.f16x3_pack_weights(P['post1_w'], ws['wpost1'], S, S, S, 1.0, scale_dev=sc('WH'), mode=md)
            K.f16x3_pack_weights(P['post2_w'], ws['wpost2'], S, Q, Q, 1.0, scale_dev=sc('WH'), mode=md)
            # wavenet.py:53-54 on the first layer's input planes (ws['xp']: also xp_all[0])
            K.f16x3_split_activations(net[0], ws['xp'], B, R, T, scale_dev=sc('X', 0), flag=flag, mode=md)
            K.f16x3_out_conv(xp=ws['xp'], Cin=R, wp=ws['wskip0'], bias=P['skip0_b'], net_out=ws['skip'], B=B, T=T, R=S, S=0,
                             w_scale_inv=1.0, x_scale=sc('X', 0), w_scale=sc('WH'), mode=md)
        else:
            K.conv_gemm(x0=net[0], w=P['skip0_w'], bias=P['skip0_b'], out0=ws['skip'], B=B, T_in=T, T_out=T, M=S,
                        C0=R, taps=[0])                                                   # wavenet.py:53-54
        if plan.f16x3:      # this step's weights of all layers as fp16 planes, one launch per kind
            K.f16x3_pack_gate_weights(P['gated_w'], ws['wp_all'], self.ks, R, 2 * R, WS, count=L, scale_dev=sc('WG'), mode=md)
            if plan.f16x3_skip:     # [L*R][S] skip kernels of all layers as one K = L*R operand (per layer group); the residual kernels per layer
                K.f16x3_pack_weights(P['out_w'], ws['wskip'], L // ngrp * R, S, S + R, WS, count=ngrp, scale_dev=sc('WO'), mode=md)
                K.f16x3_pack_weights(P['out_w'].view(-1)[S:], ws['wres'], R, R, S + R, WS, count=L, scale_dev=sc('WO'), mode=md)
            elif plan.f16x3_out:
                K.f16x3_pack_weights(P['out_w'], ws['wop_all'], R, S + R, S + R, WS, count=L, mode=md)
        return plan

    def _decode_input(self, x, ws):
        """The input stage: labels and net[0] = the preprocess conv of the shifted input (hook)."""
        lv = {} if self.levels == 256 else {'levels': self.levels}     # (256: the call as it has always been)
        K.wavenet_inputs(x, ws['inputs'], ws['labels'], **lv)                             # wavenet.py:33-37
        K.conv_cin1_fwd(ws['inputs'], self.P['pre_w'], self.P['pre_b'], ws['net'][0], k=self.pre_k, stride=1,
                        offset=-(self.pre_k - 1))                                         # wavenet.py:42-44

    def _decode_layers(self, ws, plan):
        """The condition projections, the residual stack and the convs behind it (wavenet.py:58-100; wavenet_ops.py:93-138)."""
        P, R, S, Q, L, B, T, Tz = self.P, self.R, self.S, self.Q, self.L, ws['B'], ws['T'], ws['Tz']
        f16x3, f16x3_skip, f16x3_out, ngrp, WS, head_x3, drop_th, drop_g, save = (
            plan.f16x3, plan.f16x3_skip, plan.f16x3_out, plan.ngrp, plan.WS, plan.head_x3, plan.drop_th, plan.drop_g, plan.save)
        Lg, md = L // ngrp, self.x3_mode_fwd
        sc, am, flag = self._guards(plan)
        xpl = (lambda l: ws['xp_all'][l]) if plan.keep_xp else (lambda l: ws['xp'])    # noqa: E731
        net = ws['net']
        if self.cond_proj:                                                                # all add_condition 1x1s
            K.cond_proj_fwd(ws['cond'], P['cond_w'], ws['condenc'], B=B, Cc=self.Cc, Mall=self.Mall, Tz=Tz)
        else:
            K.conv_gemm(x0=ws['cond'], w=P['cond_w'], out0=ws['condenc'], B=B, T_in=Tz, T_out=Tz, M=self.Mall,
                        C0=self.Cc, taps=[0])
        cbs = self.Mall * Tz
        ce_flat = ws['condenc'].view(-1)   # layer l's rows start at l*2R*Tz inside every batch block
        for l, d in enumerate(self.dil):
            if f16x3:
                if (l == 0 and not head_x3) or not f16x3_out:
                    K.f16x3_split_activations(net[l], xpl(l), B, R, T, scale_dev=sc('X', 0), flag=flag, mode=md)
                K.f16x3_gate_conv(xp=xpl(l), wp=ws['wp'][l], out0=None if drop_g else ws['gated'][l],
                                  save0=ws['th'][l] if (save and not drop_th) else None,
                                  save1=ws['sg'][l] if save else None, bias=P['gated_b'][l],
                                  cond=ce_flat[l * 2 * R * Tz:], cond_T=Tz, cond_bstride=cbs, B=B, T=T, R=R, ks=self.ks,
                                  dilation=d, w_scale_inv=1.0 / WS, out_planes=ws['gp'] if f16x3_out else None,
                                  out_planes_kc0=l * (R // 8) if f16x3_skip else 0, out_planes_KC=L * (R // 8) if f16x3_skip else 0,
                                  x_scale=sc('X', l), w_scale=sc('WG'), mode=md)
                if f16x3_skip:   # residual half now; the skip half of all layers after the loop
                    if l < L - 1:    # the top layer's residual output feeds nothing (wavenet.py:58-78: TF prunes the op from the graph)
                        K.f16x3_out_conv(xp=ws['gp'], xp_kc0=l * (R // 8), xp_KC=L * (R // 8), Cin=R, wp=ws['wres'][l],
                                         bias=P['out_b'][l][S:], net_in=net[l], net_out=net[l + 1], net_out_planes=xpl(l + 1),
                                         B=B, T=T, R=R, S=0, w_scale_inv=1.0 / WS, w_scale=sc('WO'), out_scale=sc('X', l + 1),
                                         out_amax=am('X', l + 1), flag=flag, mode=md)
                    continue
                if f16x3_out:
                    K.f16x3_out_conv(xp=ws['gp'], wp=ws['wop'][l], bias=P['out_b'][l], skip=ws['skip'], net_in=net[l],
                                     net_out=net[l + 1], net_out_planes=xpl(l + 1), B=B, T=T, R=R, S=S, w_scale_inv=1.0 / 256.0, mode=md)
                    continue
            else:
                K.conv_gemm(x0=net[l], w=P['gated_w'][l], bias=P['gated_b'][l], out0=ws['gated'][l],
                            save0=ws['th'][l] if save else None, save1=ws['sg'][l] if save else None,
                            cond=ce_flat[l * 2 * R * Tz:], cond_T=Tz, cond_bstride=cbs, B=B, T_in=T, T_out=T,
                            M=2 * R, C0=R, taps=causal_taps(self.ks, d),
                            epilogue=K.EPI_GATE)                                          # wavenet_ops.py:104-114
            # the 1x1 skip + residual conv on the fp32 engine (also behind a plane gate conv: ladder step 1)
            K.conv_gemm(x0=ws['gated'][l], w=P['out_w'][l], bias=P['out_b'][l], out0=ws['skip'], out1=net[l + 1],
                        aux1=net[l], B=B, T_in=T, T_out=T, M=S + R, M0=S, C0=R, taps=[0],
                        epilogue=K.EPI_ACCUM_SPLIT, tile=self.tiles['out'])                                       # :132-136, wavenet.py:72-73
        wsk = ws['wskip'].view(ngrp, -1) if f16x3_skip else None
        if head_x3:      # the same contraction hands relu(skip) over as planes; wavenet.py:80-96 on planes
            for gi in range(ngrp):
                last = gi == ngrp - 1
                K.f16x3_out_conv(epi=2, xp=ws['gp'], Cin=Lg * R, xp_kc0=gi * Lg * (R // 8), xp_KC=L * (R // 8), wp=wsk[gi],
                                 bias=P['out_b'][:, :S].sum(0) if gi == 0 else None, net_in=ws['skip'], net_out=ws['skip'],
                                 net_out_planes=ws['hp'] if last else None, relu_planes=last, B=B, T=T, R=S, S=0,
                                 w_scale_inv=1.0 / WS, w_scale=sc('WO'), out_scale=sc('SK') if last else None,
                                 out_amax=am('SK') if last else None, flag=flag if last else None, mode=self.x3_mode_skip)
            K.f16x3_out_conv(epi=2, xp=ws['hp'], Cin=S, wp=ws['wpost1'], bias=P['post1_b'], cond=ce_flat[L * 2 * R * Tz:], cond_T=Tz,
                             cond_bstride=cbs, net_out=ws['h1'], net_out_planes=ws['hp2'], relu_planes=True, B=B, T=T, R=S, S=0,
                             w_scale_inv=1.0, x_scale=sc('SK'), w_scale=sc('WH'), out_scale=sc('H1'), out_amax=am('H1'), flag=flag,
                             mode=self.x3_mode_head)
            K.f16x3_out_conv(epi=2, xp=ws['hp2'], Cin=S, wp=ws['wpost2'], bias=P['post2_b'], net_out=ws['logits'], B=B, T=T, R=Q,
                             S=0, w_scale_inv=1.0, x_scale=sc('H1'), w_scale=sc('WH'), mode=self.x3_mode_head)
            return
        for gi in range(ngrp if f16x3_skip else 0):   # skip = skip0 + sum_l (W_s,l g_l + b_s,l)   (wavenet.py:72 summed over the layers)
            K.f16x3_out_conv(xp=ws['gp'], Cin=Lg * R, xp_kc0=gi * Lg * (R // 8), xp_KC=L * (R // 8), wp=wsk[gi],
                             bias=P['out_b'][:, :S].sum(0) if gi == 0 else None, skip=ws['skip'], B=B, T=T, R=0, S=S,
                             w_scale_inv=1.0 / WS, w_scale=sc('WO'), mode=self.x3_mode_skip)
        K.conv_gemm(x0=ws['skip'], in_relu=True, w=P['post1_w'], bias=P['post1_b'], out0=ws['h1'],
                    cond=ce_flat[L * 2 * R * Tz:], cond_T=Tz, cond_bstride=cbs, B=B, T_in=T, T_out=T, M=S,
                    C0=S, taps=[0])                                                       # wavenet.py:80-88
        K.conv_gemm(x0=ws['h1'], in_relu=True, w=P['post2_w'], bias=P['post2_b'], out0=ws['logits'], B=B, T_in=T,
                    T_out=T, M=Q, C0=S, taps=[0])                                         # wavenet.py:94-96

    def forward(self, x, spk, compute_grad_seed=True, lengths=None):
        """model.py:145-151 up to the losses.  x [B][T] raw audio in [-1,1], spk int64 [B].
        Leaves logits (or d loss/d logits when compute_grad_seed) in the workspace and the
        loss sums in self.loss_buf (no host sync).  lengths: None, or what train_step takes: the loss and its gradient seed
        cover t < lengths[b] alone (the seed is +0.0 behind it) and the mean is over sum(lengths) positions."""
        B, T = x.shape
        lens = self._train_lengths('forward', lengths, B, T)     # (refused before anything is launched)
        if self._pending and not self._in_step:      # a caller's own forward pass between deferred steps: settle those first
            self.finish_steps()
        ws = self._workspace(B, T)
        if A.POISON:             # debug: every workspace buffer and the transposed-kernel scratch start the step as NaN
            A.repoison(ws['_poison'] + self._poison_T)
        # (the decoder's front-independent prologue on the side stream under the front's short layers measured null, 27.0 vs
        # 27.0 ms: the step is not bound by those ~35 small launches)
        plan = self._decode_prologue(x, ws)
        self._encode(x, spk, ws)
        self._decode_layers(ws, plan)
        self.loss_buf.zero_()
        N = ws['count'] = B * T if lens is None else sum(lens)      # the positions the loss is the mean over (losses())
        if lens is None:
            ws['dl'] = ws.get('dl_scale')
            K.softmax_xent(ws['logits'], ws['labels'], loss_sum=self.loss_buf[0:1],
                           dlogits=ws['logits'] if compute_grad_seed else None, grad_scale=1.0 / N)  # model.py:91-94
        else:
            if 'dl_scale' in ws:     # |d loss / d logits| <= 1 / count now: the fixed scale of its planes follows the count (no host read)
                ws['dl'] = ws.setdefault('dl_masked', torch.empty(1, device=self.dev)).fill_(2.0 ** math.floor(math.log2(2.0 ** 13 * N)))
            K.softmax_xent_ranged(ws['logits'], ws['labels'], loss_sum=self.loss_buf[0:1],
                                  dlogits=ws['logits'] if compute_grad_seed else None, grad_scale=1.0 / N,
                                  t_end=self._lengths_device(lens))
        self._front_loss(ws)
        return ws

    _masked_training = None     # why a subclass cannot train on lengths (a message), or None: it can

    def _row_lengths(self, who, lengths, B, T):
        """lengths (None, a host sequence or a CPU tensor) as a list of B ints: positive multiples of _length_unit(), at most T;
        anything else raises ValueError (named after `who`)."""
        if lengths is None:
            return None
        unit = self._length_unit()
        lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lens) != B:
            raise ValueError('%s: %d lengths for a batch of %d' % (who, len(lens), B))
        bad = [v for v in lens if v <= 0 or v > T or v % unit]
        if bad:
            raise ValueError('%s: lengths must be positive multiples of %d and at most T = %d (got %s)' % (who, unit, T, bad[:5]))
        return lens

    def _train_lengths(self, who, lengths, B, T):
        """_row_lengths for a training pass, with what training on lengths cannot do refused."""
        if lengths is None:
            return None
        if self._masked_training is not None:
            raise NotImplementedError('%s: %s' % (who, self._masked_training))
        if self.grad_sync is not None and getattr(self.grad_sync, 'active', True):
            raise NotImplementedError('%s: lengths with data-parallel gradients (grad_sync) is not supported: the ranks would have to '
                                      'agree on a global count of scored positions' % who)
        return self._row_lengths(who, lengths, B, T)

    def _lengths_device(self, lens):
        """The lengths of one step as a device int32 [B]: staged in pinned host memory and copied without blocking.  The staging
        block comes from torch's caching host allocator, which holds a block back until the copy that reads it has run: the host
        may be any number of steps ahead of the device (the fp32 engine's step has no host read at all) and no step waits."""
        host = torch.tensor(lens, dtype=torch.int32)
        if self.dev.type != 'cuda':
            return host
        return host.pin_memory().to(self.dev, non_blocking=True)

    def _front_loss(self, ws):
        """The front's own loss sums into loss_buf[1:] (hook; none)."""

    def forward_checked(self, x, spk, compute_grad_seed=False, lengths=None):
        """forward() for callers that do not go on to train_step (evaluation, summaries of a held-out batch).  On the guarded
        fp16x3 engine the activation planes are scaled with the PREVIOUS training step's max-abs values (1.0 on a fresh model):
        train_step reads the range flag and repeats a flagged step on the fp32 engine; a bare forward() does not.  This one
        does: the flag is zeroed, read after the pass (one host sync) and a flagged pass is repeated on the fp32 engine."""
        lens = self._train_lengths('forward_checked', lengths, *x.shape)
        self.finish_steps()
        if not self.x3_guard:
            return self.forward(x, spk, compute_grad_seed, lens)
        self.x3_flag.zero_()
        ws = self.forward(x, spk, compute_grad_seed, lens)
        if self._ran_guarded(ws) and int(self.x3_flag.item()) != 0:
            with self._fp32_engine():
                ws = self.forward(x, spk, compute_grad_seed, lens)
        return ws

    # ------------------------------------------------------------------ held-out scoring
    def _length_unit(self):
        """What a row's scored length must be a multiple of (hook; 1)."""
        return 1

    def evaluate(self, x, spk, lengths=None, weights='ema', per_position=False):
        """Score held-out rows: the decoder's teacher-forced pass over the padded batch x [B][T] (forward only, on the score
        workspace), restricted per row to t < lengths[b] -- what oracle.ref_model.forward gives for the same padded input.
        Returns a scoring.Score: per row nll_sum / entropy_sum (nats, float64), count, hits (the label is the lowest index
        among the maxima of its logits, the generators' greedy decision); what the front adds over the frames f < lengths[b] // ratio
        (_score_front; model.VQVAE says what and how padding reaches it); with per_position the nll / entropy
        [B][T] device tensors (0 where not scored).
        lengths: None (whole rows) or B positive multiples of _length_unit(), at most T; anything
        else raises before a launch.  The decoder is causal: its padding never reaches a scored position.
        weights: 'ema' scores with the EMA shadows (what generate.py uses), 'live' with the live parameters.  The pass behaves
        like forward_checked (range flag zeroed, read once, a flagged pass repeated on the fp32 engine).  Afterwards -- also
        when the call raises -- the parameters, EMA shadows, optimiser state, step counter, the front's state, the guard's
        scales, max-abs collectors, range flag and the sticky void flag are bit-identical to what they were: an evaluation
        between two training steps leaves the second step what it would have been.  Synchronises."""
        from . import scoring

        def finish(ws, t_end, f_end):
            sums, counts = K.softmax_score(ws['logits'], ws['labels'], t_end=t_end, nll=ws['nll'] if per_position else None,
                                           entropy=ws['entropy'] if per_position else None)
            out = scoring.Score(nll_sum=sums[:, 0].cpu(), entropy_sum=sums[:, 1].cpu(), count=counts[:, 0].cpu().long(),
                                hits=counts[:, 1].cpu().long())
            if per_position:
                out.nll, out.entropy = ws['nll'].clone(), ws['entropy'].clone()
            self._score_front(ws, f_end, out)
            return out
        return self._teacher_forced('evaluate', x, spk, lengths, weights, finish)

    def _teacher_forced(self, who, x, spk, lengths, weights, finish):
        """What evaluate and reconstruct share: the argument checks (errors named after `who`), the teacher-forced pass on the
        score workspace with the EMA or the live weights, forward_checked's handling of the range flag, and the restoration of
        every piece of training state, also when something raises.  finish(ws, t_end, f_end) turns the pass's logits into the
        caller's result while the chosen weights are still in place (t_end / f_end: device int32 [B], None without lengths)."""
        if weights not in ('ema', 'live'):
            raise ValueError("%s: weights must be 'ema' or 'live' (got %r)" % (who, weights))
        if x.dim() != 2 or spk.numel() != x.shape[0]:
            raise ValueError('%s: x [B][T] and B speaker ids expected (got %s, %d ids)' % (who, tuple(x.shape), spk.numel()))
        B, T = x.shape
        lens = self._row_lengths(who, lengths, B, T)
        self.finish_steps()
        ws = self._workspace(B, T, 'score')
        t_end = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=self.dev)
        f_end = None if lens is None else torch.tensor([v // ws['ratio'] for v in lens], dtype=torch.int32, device=self.dev)
        guard = [(t, t.clone()) for t in (self.x3_scale, self.x3_amax, self.x3_flag, self.x3_void)]
        live = self.flat.clone() if weights == 'ema' else None
        try:
            if live is not None:
                self.flat.copy_(self.ema)
            self.x3_flag.zero_()
            self._score_pass(x, spk, ws)
            if self.x3_guard and self._ran_guarded(ws) and int(self.x3_flag.item()) != 0:
                with self._fp32_engine():
                    self._score_pass(x, spk, ws)
            return finish(ws, t_end, f_end)
        finally:
            if live is not None:
                self.flat.copy_(live)
            for t, saved in guard:
                t.copy_(saved)
            self._tt_done = set()          # (transposed kernels cached from the parameters: made again on next use)

    def _reconstruct(self, who, x, spk, lengths, weights, mode, uniforms, seed, temperature, top_k, top_p, return_probs, audio):
        from .generator import sampling_settings
        if mode not in ('sample', 'greedy'):
            raise ValueError("%s: mode must be 'sample' or 'greedy' (got %r)" % (who, mode))
        if x.dim() == 2:
            sampling_settings(x.shape[0], mode, temperature, top_k, top_p)      # refused before anything runs
            if uniforms is not None and (mode != 'sample' or tuple(uniforms.shape) != tuple(x.shape) or uniforms.dtype != torch.float32):
                raise ValueError("%s: uniforms must be float32 [B][T] and need mode 'sample'" % who)

        def finish(ws, t_end, f_end):
            B, T = ws['B'], ws['T']
            u = uniforms
            if mode == 'sample' and u is None:
                if self._recon_gen is None:
                    self._recon_gen = torch.Generator(device=self.dev)
                self._recon_gen.manual_seed(mix_seed(int(seed)))
                u = torch.rand(B, T, generator=self._recon_gen, device=self.dev)
            Q = ws['logits'].shape[1]
            out_audio = torch.empty(B, T, device=self.dev) if audio else None
            probs = torch.empty(B, T, Q, device=self.dev) if return_probs else None
            idx = K.softmax_sample(ws['logits'], mode=mode, uniforms=u, temperature=temperature, top_k=top_k, top_p=top_p,
                                   t_end=t_end, audio=out_audio, probs=probs,
                                   **({} if self.levels == 256 else {'levels': self.levels}))
            torch.cuda.synchronize(self.dev)
            out = ((out_audio,) if audio else ()) + (idx,) + ((probs,) if return_probs else ())
            return out if len(out) > 1 else out[0]
        return self._teacher_forced(who, x, spk, lengths, weights, finish)

    def _score_pass(self, x, spk, ws):
        if A.POISON:
            A.repoison(ws['_poison'])
        plan = self._decode_prologue(x, ws, save=False)
        self._encode(x, spk, ws, save=False)
        self._decode_layers(ws, plan)

    def _score_front(self, ws, f_end, out):
        """The front's statistics of a scored batch into the scoring.Score `out` (hook; none)."""

    def losses(self, ws):
        """(loss, cross-entropy, 0, 0) as python floats: the WaveNet's loss is the cross-entropy alone (synchronises; hook)."""
        self.finish_steps()
        ce = float(self.loss_buf[0]) / ws.get('count', ws['B'] * ws['T'])     # (count: sum(lengths) of a masked step)
        return ce, ce, 0.0, 0.0

    # ------------------------------------------------------------------ backward
    def _tt(self, name):
        """The transposed fp32 copy of a kernel for the fp32 engine's input-gradient GEMMs, made on first use in this backward pass
        (the fp16x3 engine packs its planes straight from the parameters, vqw_f16x3_pack_weights_t: on the default path only the
        condition projection and the front's last 1x1 layer still need a copy -- six transposes per step fewer)."""
        if name not in self._tt_done:
            rows, cols = self.P[name].shape[-2:]        # (a grouped kernel [...][rows][cols]: every [rows][cols] block on its own)
            K.transpose(self.P[name], self.T[name], self.P[name].numel() // (rows * cols), rows, cols)
            self._tt_done.add(name)
        return self.T[name]

    def _backward_prepare(self):
        """Transposed kernels of the front's backward pass (hook; none)."""

    def backward(self, x, spk, ws):
        """Gradients of the loss (VQ-VAE: CE + vq + commitment, model.py:90-106) w.r.t. every trainable
        variable, accumulated into self.grad (zeroed here): the stages of forward() in reverse, by ws['plan'] -- what the
        forward pass decided; nothing is derived again here."""
        self.grad.zero_()
        self._tt_done = set()
        self._backward_prepare()
        if ws['plan'].wg_x3 or ws['plan'].head_x3:
            self._wslab(ws)
        dskip = self._backward_head(ws)
        dnet = self._backward_stack(ws, dskip)
        self._backward_tail(x, ws, dskip, dnet)
        self._backward_front(x, spk, ws)

    def _backward_head(self, ws):
        """postprocess2 / postprocess1 (wavenet.py:79-96) from d logits: their gradients, postprocess1's part of the condition
        gradient (ws['dcondenc']), and d skip, which it returns (in ws['skip'])."""
        P, G, R, S, Q, L = self.P, self.G, self.R, self.S, self.Q, self.L
        B, T, Tz, ratio = ws['B'], ws['T'], ws['Tz'], ws['ratio']
        dlog, h1, skip = ws['logits'], ws['h1'], ws['skip']
        cbs, dce = self.Mall * Tz, ws['dcondenc']
        plan, md = ws['plan'], self.x3_mode_bwd
        calib, GSh = plan.calib, plan.GSh
        sc, am, flag = self._guards(plan)
        if plan.head_x3:
            # the convs around the stack on the fp16x3 engine (forward: _decode_layers): d logits as planes with a fixed scale
            # (|d logits| <= 1 / (B T)), each input gradient hands the next one its planes, the weight gradients split their fp32
            # operands in registers (p = relu of the forward tensor), bias and condition sums ride along
            dl = ws['dl']               # (forward(): dl_scale, or the masked step's own)
            K.f16x3_pack_weights_t(P['post2_w'], ws['wpost2t'], Q, S, Q, Q, 0, 1.0, scale_dev=sc('WH'), mode=md)
            K.f16x3_pack_weights_t(P['post1_w'], ws['wpost1t'], S, S, S, S, 0, 1.0, scale_dev=sc('WH'), mode=md)
            K.f16x3_pack_weights_t(P['skip0_w'], ws['wskip0t'], S, R, S, S, 0, 1.0, scale_dev=sc('WH'), mode=md)
            dce.zero_()
            # ---- postprocess2 (wavenet.py:93-96)
            K.f16x3_split_activations(dlog, ws['hp2'], B, Q, T, scale_dev=dl, mode=md)
            K.f16x3_wgrad(p=h1, p_relu=True, q0=dlog, dw=G['post2_w'], slab=ws['wslab'], B=B, T=T, Cp=S, Q0=Q, taps=[0],
                          p_scale=sc('H1'), q0_scale=dl, q_total=G['post2_b'], mode=md)
            K.f16x3_out_conv(epi=2, xp=ws['hp2'], Cin=Q, wp=ws['wpost2t'], net_out=h1, aux0=h1, net_out_planes=ws['hp'], B=B, T=T,
                             R=S, S=0, w_scale_inv=1.0, x_scale=dl, w_scale=sc('WH'), out_scale=sc('DH'), out_amax=am('DH'),
                             flag=flag, mode=self.x3_mode_head)   # h1 := d h1 (pre-relu)
            # ---- postprocess1 (wavenet.py:79-88)
            K.f16x3_wgrad(p=skip, p_relu=True, q0=h1, dw=G['post1_w'], slab=ws['wslab'], B=B, T=T, Cp=S, Q0=S, taps=[0],
                          p_scale=sc('SK'), q0_scale=sc('DH'), q_total=G['post1_b'], q_seg=dce.view(-1)[L * 2 * R * Tz:], seg_T=Tz,
                          seg_bstride=cbs, mode=md)
            K.f16x3_out_conv(epi=2, xp=ws['hp'], Cin=S, wp=ws['wpost1t'], net_out=skip, aux0=skip, net_out_planes=ws['gr'],
                             planes_kc0=0, planes_KC=(S + R) // 8, plane_scale=GSh, B=B, T=T, R=S, S=0, w_scale_inv=1.0, x_scale=sc('DH'),
                             w_scale=sc('WH'), out_scale=sc('G'), out_amax=am('G'), flag=flag, mode=self.x3_mode_head)   # skip := d skip, and its planes
        else:
            # ---- postprocess2 (wavenet.py:93-96)
            K.wgrad_gemm(p=h1, p_relu=True, q0=dlog, dw=G['post2_w'], B=B, T_q=T, T_p=T, Cp=S, Q0=Q, taps=[0])
            K.rowsum(dlog, total=G['post2_b'])
            K.conv_gemm(x0=dlog, w=self._tt('post2_w'), out0=h1, aux0=h1, B=B, T_in=T, T_out=T, M=S, C0=Q, taps=[0],
                        epilogue=K.EPI_MASK)                       # h1 := d h1 (pre-relu)
            if calib:
                K.f16x3_amax(h1, am('DH'))
            # ---- postprocess1 (wavenet.py:79-88)
            K.wgrad_gemm(p=skip, p_relu=True, q0=h1, dw=G['post1_w'], B=B, T_q=T, T_p=T, Cp=S, Q0=S, taps=[0])
            seg_p1 = A.empty(B, S, Tz, device=self.dev)
            K.rowsum(h1, seg_out=seg_p1, total=G['post1_b'], seg=ratio)
            dce[:, L * 2 * R:].copy_(seg_p1)
            K.conv_gemm(x0=h1, w=self._tt('post1_w'), out0=skip, aux0=skip, B=B, T_in=T, T_out=T, M=S, C0=S, taps=[0],
                        epilogue=K.EPI_MASK)                       # skip := d skip (same for every layer)
        return skip

    def _backward_stack(self, ws, dskip):
        """The residual stack, top layer first (wavenet.py:63-74): the chain gate backward -> input gradient down the layers on
        the current stream.  The layers' weight gradients, bias sums and their part of the condition gradient go out beside it
        by a schedule (_BatchedWgrads / _PerLayerWgrads), which also says where each layer writes.  Returns dnet =
        d loss / d net[0] without the skip start's share."""
        P, G, R, S, L, ks, B, T = self.P, self.G, self.R, self.S, self.L, self.ks, ws['B'], ws['T']
        plan, md, dce = ws['plan'], self.x3_mode_bwd, ws['dcondenc']
        sc, am, flag = self._guards(plan)
        main = torch.cuda.current_stream()
        side = self._side_stream() if self.overlap_wgrad else main
        if plan.dgrad_x3:
            K.f16x3_pack_weights_t(P['gated_w'], ws['wdg'], ks * 2 * R, R, 2 * R, 2 * R, R * 2 * R, plan.WS, count=L, scale_dev=sc('WG'), mode=md)
        if plan.gbwd_x3:
            K.f16x3_pack_weights_t(P['out_w'], ws['wgb'], S + R, R, S + R, S + R, R * (S + R), plan.WS, count=L, scale_dev=sc('WO'), mode=md)
            K.f16x3_pack_weights_t(P['out_w'][L - 1], ws['wgb_top'], S, R, S, S + R, 0, plan.WS, scale_dev=sc('WO'), mode=md)       # the top layer has no dnet
            if not plan.head_x3:      # (the input gradient of postprocess1 wrote them otherwise)
                K.f16x3_split_activations(dskip, ws['gr'], B, S, T, scale=plan.GS, kc0=0, KC=(S + R) // 8, scale_dev=sc('G'),
                                          amax=am('G'), flag=flag, mode=md)   # one tensor for all layers
        if plan.calib:
            K.f16x3_amax(dskip, am('G'))
        if plan.wg_x3 and not plan.head_x3:      # the weight-gradient kernels add the per-frame sums of dpre into the condition gradient
            dce[:, :L * 2 * R].zero_()
        wgrads = (_BatchedWgrads if plan.batched else _PerLayerWgrads)(self, ws, dskip, main, side)
        dnet = None                  # the top layer has none: net[L] is unused by the graph, its gradient is zero
        for l in range(L - 1, -1, -1):
            dpre, dplanes, dnet_next = wgrads.buffers(l)
            self._gate_backward(ws, l, dskip, dnet, dpre, dplanes)
            ready = side_mark(main, side)            # dpre of layer l is complete
            self._gate_dgrad(ws, l, dpre, dplanes, dnet, dnet_next)
            wgrads.layer(l, dnet, dpre, ready)
            dnet = dnet_next
        wgrads.finish()
        if side is not main:
            main.wait_stream(side)
        if plan.wg_x3:      # gated biases: the condition gradient summed over batch and frames, all layers in one launch
            tot = torch.zeros(self.Mall, device=self.dev)
            K.rowsum(dce, total=tot)
            G['gated_b'].view(-1).add_(tot[:L * 2 * R])
        return dnet

    def _gate_backward(self, ws, l, dskip, dnet, dpre, dplanes):
        """Layer l's link of the chain, first half: dpre = d loss / d (gate pre-activation) from dskip and dnet = d loss / d net[l + 1]
        (None: the top layer), as fp32 (dpre) and / or operand planes (dplanes) -- on the plane engine or the fp32 engine."""
        R, S, L, B, T = self.R, self.S, self.L, ws['B'], ws['T']
        plan, md, top = ws['plan'], self.x3_mode_bwd, dnet is None
        sc, am, flag = self._guards(plan)
        if plan.gbwd_x3:
            GS, WS, th_dropped, g_dropped = plan.GS, plan.WS, plan.drop_th, plan.drop_g
            K.f16x3_out_conv(epi=1, xp=ws['gr'], Cin=S if top else S + R, xp_KC=(S + R) // 8,
                             wp=ws['wgb_top'] if top else ws['wgb'][l], aux0=None if g_dropped else (ws['gated'][l] if th_dropped else ws['th'][l]),
                             aux0_planes=ws['gp'] if g_dropped else None, aux0_KC=L * (R // 8), aux0_kc0=l * (R // 8),
                             aux0_is_gated=th_dropped, aux1=ws['sg'][l], net_out=dpre,
                             net_out_planes=dplanes, plane_scale=GS, B=B, T=T, R=R, S=0, w_scale_inv=1.0 / (WS * GS),
                             x_scale=sc('G'), w_scale=sc('WO'), out_scale=sc('DP', l), out_amax=am('DP', l), flag=flag, mode=md)
        else:
            K.conv_gemm(x0=dskip, x1=dnet, w=self._tt('out_w')[l], out0=dpre, aux0=ws['th'][l],
                        aux1=ws['sg'][l], B=B, T_in=T, T_out=T, M=R, C0=S, C1=0 if top else R, taps=[0],
                        epilogue=K.EPI_GATE_BWD, tile=self.tiles['gate_bwd'])
        if plan.calib:
            K.f16x3_amax(dpre, am('DP', l))

    def _gate_dgrad(self, ws, l, dpre, dplanes, dnet, dnet_next):
        """... second half: dnet_next = d loss / d net[l] = the gate conv's input gradient of dpre, plus dnet (the residual
        connection; None: the top layer) -- on the plane engine (guarded, or the ladder's fixed lift behind either gate backward)
        or the fp32 engine."""
        R, S, ks, d, B, T = self.R, self.S, self.ks, self.dil[l], ws['B'], ws['T']
        plan, md = ws['plan'], self.x3_mode_bwd
        sc, am, flag = self._guards(plan)
        if plan.dgrad_x3:
            gbwd_x3, GS = plan.gbwd_x3, plan.GS
            if not gbwd_x3:      # (gate backward hands dpre over as planes)
                K.f16x3_split_activations(dpre, ws['dp'], B, 2 * R, T, scale=GS, mode=md)
            K.f16x3_out_conv(xp=dplanes, Cin=2 * R, ks=ks, dilation=d, direction=-1, wp=ws['wdg'][l],
                             net_in=dnet, net_out=dnet_next, B=B, T=T, R=R, S=0,
                             w_scale_inv=1.0 / (plan.WS * GS),
                             net_out_planes=ws['gr'] if gbwd_x3 else None, planes_kc0=S // 8 if gbwd_x3 else 0,
                             planes_KC=(S + R) // 8 if gbwd_x3 else 0, plane_scale=GS if gbwd_x3 else 0.0,
                             x_scale=sc('DP', l), w_scale=sc('WG'), out_scale=sc('G'), out_amax=am('G'), flag=flag, mode=self.x3_mode_dgrad)
        elif dnet is None:
            K.conv_gemm(x0=dpre, w=self._tt('gated_w')[l], out0=dnet_next, B=B, T_in=T, T_out=T, M=R, C0=2 * R, taps=mirrored_taps(ks, d),
                        tile=self.tiles['dgrad'])
        else:
            K.conv_gemm(x0=dpre, w=self._tt('gated_w')[l], out1=dnet_next, aux1=dnet, out0=dnet_next, B=B, T_in=T, T_out=T,
                        M=R, M0=0, C0=2 * R, taps=mirrored_taps(ks, d), epilogue=K.EPI_ACCUM_SPLIT, tile=self.tiles['dgrad'])
        if plan.calib:
            K.f16x3_amax(dnet_next, am('G'))

    def _backward_tail(self, x, ws, dskip, dnet):
        """Skip start + preprocess (wavenet.py:42-55): dnet += W_skip0^T dskip, the skip start's gradients and the skip bias sums,
        the input stage (_backward_input), then the condition projections (wavenet_ops.py:93-101): ws['dcond'] for _backward_front."""
        P, G, R, S, B, T, Tz = self.P, self.G, self.R, self.S, ws['B'], ws['T'], ws['Tz']
        dce, net = ws['dcondenc'], ws['net']
        plan, md = ws['plan'], self.x3_mode_bwd
        wg_x3, GS = plan.wg_x3, plan.GS
        sc = self._guards(plan)[0]
        if plan.head_x3 and plan.gbwd_x3:      # dnet += W_skip0^T dskip over dskip's planes (chunks 0..S/8 of the gradient planes)
            K.f16x3_out_conv(xp=ws['gr'], xp_KC=(S + R) // 8, Cin=S, wp=ws['wskip0t'], net_in=dnet, net_out=dnet, B=B, T=T, R=R, S=0,
                             w_scale_inv=1.0 / GS, x_scale=sc('G'), w_scale=sc('WH'), mode=md)
        else:
            K.conv_gemm(x0=dskip, w=self._tt('skip0_w'), out1=dnet, aux1=dnet, out0=dnet, B=B, T_in=T, T_out=T, M=R, M0=0,
                        C0=S, taps=[0], epilogue=K.EPI_ACCUM_SPLIT)
        ws['bskip'].zero_()      # sum of dskip over batch and time: the bias gradient of skip0 and of every layer's skip half
        if wg_x3:      # both operands already have guard scales (layer-0 input planes, gradient planes); the sum rides along
            K.f16x3_wgrad(p=net[0], q0=dskip, dw=G['skip0_w'], slab=ws['wslab'], B=B, T=T, Cp=R, Q0=S, taps=[0],
                          p_scale=sc('X', 0), q0_scale=sc('G'), q_total=ws['bskip'], mode=md)
        else:
            K.wgrad_gemm(p=net[0], q0=dskip, dw=G['skip0_w'], B=B, T_q=T, T_p=T, Cp=R, Q0=S, taps=[0])
            K.rowsum(dskip, total=ws['bskip'])
        G['out_b'][:, :S] += ws['bskip']
        G['skip0_b'] += ws['bskip']
        self._backward_input(x, ws, dnet)
        # ---- local condition (wavenet_ops.py:93-101) -> d cond
        if self.cond_proj and Tz % 4 == 0 and P['cond_w'].data_ptr() % 16 == 0:
            scratch = A.scratch(ws, 'cp_scratch', lambda: A.empty(K.cond_proj_dgrad_scratch(B, self.Cc, self.Mall, Tz), device=self.dev))
            K.cond_proj_wgrad(ws['cond'], dce, G['cond_w'], B=B, Cc=self.Cc, Mall=self.Mall, Tz=Tz)
            K.cond_proj_dgrad(P['cond_w'], dce, ws['dcond'], scratch, B=B, Cc=self.Cc, Mall=self.Mall, Tz=Tz)
        else:
            K.wgrad_gemm(p=ws['cond'], q0=dce, dw=G['cond_w'], B=B, T_q=Tz, T_p=Tz, Cp=self.Cc, Q0=self.Mall, taps=[0])
            K.conv_gemm(x0=dce, w=self._tt('cond_w'), out0=ws['dcond'], B=B, T_in=Tz, T_out=Tz, M=self.Cc, C0=self.Mall, taps=[0])

    def _backward_input(self, x, ws, dnet):
        """Gradients of the preprocess conv from dnet = d loss / d net[0] (hook)."""
        G = self.G
        K.conv_cin1_wgrad(ws['inputs'], dnet, G['pre_w'], k=self.pre_k, stride=1, offset=-(self.pre_k - 1))
        K.rowsum(dnet, total=G['pre_b'])

    def _backward_front(self, x, spk, ws):
        """From ws['dcond'] = d loss / d cond on: the front's backward pass (hook)."""
        raise NotImplementedError

    # ------------------------------------------------------------------ optimiser
    def lr_at(self, step):
        """Piecewise-constant schedule of model.py:111-114."""
        lr = self.schedule[0][1]
        for key, value in self.schedule:
            if not (step < key):
                lr = value
        return lr

    @property
    def clip_norm(self):
        """Clipping by global norm (tf.clip_by_global_norm on grad * grad_scale).  None: off, the step is what it
        was without this attribute.  A float > 0: the threshold.  float('inf'): the norms are measured (grad_norms), nothing
        is clipped.  Settable at any time; not part of state_dict."""
        return self._clip_norm

    @clip_norm.setter
    def clip_norm(self, value):
        if value is not None:
            value = float(value)
            if not K.clip_as_fp32(value) > 0.0:       # (the kernels take the threshold as fp32: 1e-50 would be 0 there)
                raise ValueError('clip_norm must be None, a threshold > 0 in fp32 or inf (got %r)' % value)
        elif self._gn is not None:
            self._gn['steps'] = 0                     # what a step measured before clipping was switched off is not reported later
        self._clip_norm = value

    @property
    def accumulate(self):
        """Micro-batches per optimiser step.  1: off, train_step is what it was without this attribute.  N > 1: a
        window of N consecutive train_step calls sums their gradients in fp32, in call order (fl(fl(g0 + g1) + g2) ...), and the
        N-th call takes ONE Adam + EMA step on the sum scaled by 1 / (N * world): with inference-mode BatchNorm and losses that
        are means over rows, the step of one batch of N * B rows up to fp32 summation order.  global_step advances on that call
        alone; under data parallel the window's one gradient exchange runs there too.  Every micro-step stays a whole guarded
        pass.  Settable at a window boundary (accum_index == 0); refused together with codebook_ema; not part of state_dict."""
        return self._accumulate

    @accumulate.setter
    def accumulate(self, value):
        if isinstance(value, bool) or not isinstance(value, int) or value < 1:
            raise ValueError('accumulate must be an integer >= 1 (got %r)' % (value,))
        if self._accum_k != 0:
            raise ValueError('accumulate cannot change while a window is open (%d of %d micro-steps done)' % (self._accum_k, self._accumulate))
        if value > 1 and getattr(self, '_codebook_ema', 0.0) > 0.0:
            raise ValueError("accumulate > 1 with codebook_ema is not supported: the codebook's own update per micro-batch has no rule yet")
        self._accumulate = value

    @property
    def accum_index(self):
        """Micro-steps already in the open window: 0 at a window boundary (read-only)."""
        return self._accum_k

    def _commit_window(self, ws, world, guard):
        """The tail of _commit with accumulate = N > 1, micro-step k of the window.  k = 0: acc = grad, a guarded copy (the
        accumulator is never assumed clean); 0 < k < N - 1: acc += grad; k = N - 1: grad = acc + grad -- acc is NOT written --
        then the window's gradient exchange and the optimiser on grad.  A voided micro-step (skip set when the kernels run)
        therefore changes neither acc nor a parameter: what the replay of an older window still needs stays, and grad is
        scratch that every pass rewrites."""
        N, k = self._accumulate, self._accum_k
        if self._acc is None:
            self._acc = torch.empty(self.n_flat, device=self.dev)
        if k < N - 1:
            if k == 0:
                K.grad_accumulate(self._acc, self.grad, **guard)
            else:
                K.grad_accumulate(self._acc, self.grad, acc=self._acc, **guard)
            self._accum_k = k + 1
            return
        K.grad_accumulate(self.grad, self.grad, acc=self._acc, **guard)
        gs = self.grad_sync
        if gs is not None:      # the one exchange of the window: the whole flat buffer in the buckets of a normal step (the ranges
            gs.hold = False     # this pass's backward was refused: they tile [0, n_flat) once), not overlapped with a backward pass
            for lo, hi in gs.last_held:
                gs.bucket_ready(lo, hi)
            world = gs.finish()
        self._front_step(ws, **guard)
        self.apply_gradients(1.0 / (N * world), **guard)
        self._accum_k = 0

    def _grad_norm_state(self):
        """Chunk table and output buffer of the norm pass, made at the first clipped step.  Segment k is the k-th trainable
        variable under its reference name: the flat elements its view (_named) covers, a column block of a grouped kernel
        being one run per row.  What no variable covers (alignment padding, the zero-padded condition rows, a variable
        no loss reaches: gradients that are always zero) is one more, unnamed segment, so that the global norm is that of the whole
        buffer the optimiser sees."""
        if self._gn is None:
            import numpy as np
            idx = torch.arange(self.n_flat, dtype=torch.int32)
            owner = np.full(self.n_flat, -1, dtype=np.int32)
            names = []
            for k, (name, view) in enumerate(self._named(self._views(idx), bn_stats=False).items()):
                owner[view.reshape(-1).numpy()] = k
                names.append(name)
            rest = len(names)
            if (owner < 0).any():
                owner[owner < 0] = rest
            cut = np.flatnonzero(np.diff(owner)) + 1
            starts = np.concatenate(([0], cut))
            ends = np.concatenate((cut, [self.n_flat]))
            segs = owner[starts]
            order = np.lexsort((starts, segs))
            runs = [(int(starts[i]), int(ends[i] - starts[i]), int(segs[i])) for i in order]
            plan = K.grad_norm_plan_runs(runs, int(segs.max()) + 1)
            self._gn = {'plan': plan, 'names': names, 'out': torch.zeros(plan.n_seg + 2, device=self.dev), 'steps': 0}
        return self._gn

    def _front_step(self, ws, skip=None):
        """What the front updates by itself from the pass that is kept, enqueued right before apply_gradients (skip: as there) (hook; nothing)."""

    def apply_gradients(self, grad_scale=1.0, skip=None):
        """TF-1.x Adam + EMA(0.999) (model.py:116-128).  skip: device int32, non-zero when the kernel runs = nothing changes.
        With clip_norm set, the two launches of the norm pass run first on the same stream and the optimiser reads their scale
        on the device (no host read; a voided step measures a norm too, and its repeat overwrites it)."""
        t = self.global_step + 1
        lr = self.lr_at(self.global_step)
        lr_t = lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        scale = None
        if self._clip_norm is not None:
            gn = self._grad_norm_state()
            K.grad_norm(self.grad, gn['plan'], grad_scale=grad_scale, clip=self._clip_norm, out=gn['out'])
            gn['steps'] += 1
            scale = gn['out'][1:2]
        K.adam_ema_step(self.flat, self.grad, self.adam_m, self.adam_v, self.ema, lr_t=lr_t, grad_scale=grad_scale, skip=skip,
                        scale=scale)
        self.global_step = t
        return lr

    def grad_norms(self):
        """Gradient norms of the last step, measured on the device before the optimiser ran (clip_norm set):
        {'global': norm of grad * grad_scale, 'scale': what the step multiplied it by (1.0 = not clipped),
         'segments': {reference variable name: norm}} with the trainable names of named_parameters().  Synchronises."""
        if self._clip_norm is None:
            raise ValueError('grad_norms: clip_norm is None (set a threshold, or inf to measure only)')
        self.finish_steps()
        if self._gn is None or self._gn['steps'] == 0:
            raise ValueError('grad_norms: no step has run since clip_norm was set')
        out = self._gn['out'].tolist()
        return {'global': out[0], 'scale': out[1], 'segments': OrderedDict(zip(self._gn['names'], out[2:]))}

    def train_step(self, x, spk, on_forward=None, lengths=None):
        """One sess.run(train_op) (train.py:104-114).  on_forward(ws): called between the forward and the backward pass of the
        step that is kept (tests snapshot the relu inputs there: backward overwrites them in place).  With self.grad_sync set (data parallel)
        the flat gradient is sum-all-reduced over RCCL in buckets that overlap the backward pass, and averaged.
        Guarded fp16x3 engine: a step whose planes left fp16's range is repeated on the fp32 engine, which also measures the
        max-abs values the next step's scales come from.  The step's range flag is read before the optimiser runs (one host sync
        per step) -- or, with self.defer_guard (bench.py, train.py), one step LATE: see _train_step_deferred.
        lengths (None: the step as it always was): B row lengths, a host sequence or a CPU tensor of positive multiples of
        _length_unit(), at most T.  The loss is then the mean cross-entropy over the sum(lengths) positions t < lengths[b], and
        every gradient is that loss's: the stack is causal, so a gradient seed that is zero from lengths[b] on makes whatever
        the row holds behind it immaterial.  Checked before anything is launched; no host synchronisation is added.
        With accumulate = N > 1 a call is one micro-step of a window of N: the passes and the guard are those of a step, the
        optimiser (and global_step) moves on the N-th call alone (accumulate, _commit_window)."""
        lens = self._train_lengths('train_step', lengths, *x.shape) if lengths is not None else None
        if self.defer_guard and self.x3_guard and on_forward is None:
            return self._train_step_deferred(x, spk, lens)
        self.finish_steps()
        return self._train_step_now(x, spk, on_forward, lengths=lens)

    @contextlib.contextmanager
    def _fp32_engine(self):
        """A pass repeated on the fp32 engine: inside, no plan puts anything on the plane engine."""
        self._x3_active = False
        try:
            yield
        finally:
            self._x3_active = True

    @staticmethod
    def _ran_guarded(ws):
        """Whether the pass in this workspace ran anything on the guarded engine (the stack or the front's layers): whether its range flag says anything."""
        return bool(ws.get('x3_used') or ws.get('enc_x3'))

    def _attempt(self, x, spk, step, lengths, *hooks):
        """One attempt at training step `step`: forward, the hooks (called with the workspace between the passes; None: skipped),
        backward, the end of the gradient exchange.  Returns (workspace, data-parallel world size)."""
        self._in_step = True           # (forward() settles deferred steps for every other caller)
        if self.grad_sync is not None:          # no bucket leaves during a window's passes: _commit_window exchanges the sum
            self.grad_sync.hold = self._accumulate > 1
        try:
            ws = self._forward_step(x, spk, step, lengths)
            for hook in hooks:
                if hook is not None:
                    hook(ws)
            self.backward(x, spk, ws)
        finally:
            self._in_step = False
        return ws, self.grad_sync.finish() if self.grad_sync is not None else 1

    def _commit(self, ws, world, scales=True, skip=None):
        """Keep the attempt: the next step's plane scales (scales=False: the pass measured none), what the front updates by itself,
        Adam + EMA.  skip: device int32, non-zero when the kernels run = each of the three changes nothing.  With accumulate > 1
        the part behind the scales is _commit_window's: the optimiser runs on a window's last micro-step alone."""
        guard = {} if skip is None else {'skip': skip}      # (an unguarded step names none: the calls are what they were)
        if scales:     # the planes written inside the kernels: max-abs * scale in [2^12, 2^13), 8x headroom
            n0 = self.SL['G']
            K.f16x3_update_scales(self.x3_amax[n0:], self.x3_scale[n0:], target_exp=13, **guard)
        if self._accumulate > 1:
            return self._commit_window(ws, world, guard)
        self._front_step(ws, **guard)
        self.apply_gradients(1.0 / world, **guard)

    def _train_step_now(self, x, spk, on_forward=None, known_flagged=False, lengths=None):
        """The step with its range flag read on the spot.  known_flagged: the fp16x3 attempt of this step already ran and
        raised the flag (deferred mode): go straight to the repeat.  lengths: train_step's, already checked."""
        guarded, world, ws = self.x3_guard and known_flagged, 1, None
        gs0 = self.global_step           # (every pass of this step is a pass of step gs0: _forward_step)
        if not known_flagged:
            if self.x3_guard:
                self.x3_flag.zero_()
            ws, world = self._attempt(x, spk, gs0, lengths, on_forward)
            if self.bf16 and ws.get('x3_used'):
                self.x3_steps += 1
            guarded = bool(self.x3_guard and self._ran_guarded(ws))
        if guarded and (known_flagged or self._x3_overflowed()):
            self.x3_fallbacks += 1

            def measure(ws):                     # what the layer-input planes would have held (net[L] feeds nothing)
                am = self._guards(ws['plan'])[1]
                for l in range(1, self.L):
                    K.f16x3_amax(ws['net'][l], am('X', l))
                K.f16x3_amax(ws['skip'], am('SK'))
                K.f16x3_amax(ws['h1'], am('H1'))
            with self._fp32_engine():
                self.x3_amax.zero_()
                ws, world = self._attempt(x, spk, gs0, lengths, measure, on_forward)
        elif guarded:
            self.x3_steps += 1
        self._commit(ws, world, scales=guarded)
        return ws

    def _train_step_deferred(self, x, spk, lengths=None):
        """The guarded step without a host sync on its path.  Reading the range flag before the optimiser drains the launch queue
        once per step, and the host then needs ~1.2 ms of the next step to get ahead of the GPU again (bench.py's shape: 26.6 ->
        25.5 ms).  Here the verdict stays on the device: the flag is latched into the sticky x3_void, the optimiser is enqueued
        behind that guard (vqw_adam_ema_step_guarded, vqw_f16x3_update_scales_guarded: a voided step changes no parameter, Adam slot,
        EMA shadow or plane scale), x3_void is
        copied to pinned host memory, and the host looks at the copy of step k only after it has enqueued step k + 1.  If step k
        was flagged, it and step k + 1 (enqueued behind it, voided by the sticky guard) have changed nothing: the guard is
        cleared, the step counter rewound, step k is repeated on the fp32 engine and step k + 1 is run again -- the same steps are repeated as in the immediate mode
        and the state agrees with it as closely as two runs of that mode do (tests/test_model_gpu.py::test_deferred_guard_matches_immediate: tolerances).
        With accumulate > 1 an entry also records its place k in its window, and k is rewound with the step counter: a voided
        micro-step has changed neither the accumulator nor anything else (_commit_window).
        Callers keep x / spk unchanged until the step is resolved (finish_steps(), or the next-but-one train_step) and call
        finish_steps() before reading what a step left behind (losses, gradients, parameters; state_dict() / encode() do)."""
        t_host = time.perf_counter()
        self.x3_flag.zero_()
        ws, world = self._attempt(x, spk, self.global_step, lengths)
        if not self._ran_guarded(ws):       # nothing on the guarded engine in this workspace
            self._commit(ws, world, scales=False)
            return ws
        if self.grad_sync is not None and self.grad_sync.active:
            self.grad_sync.all_reduce_max(self.x3_flag)       # every rank takes the same branch
        torch.maximum(self.x3_void, self.x3_flag, out=self.x3_void)
        gs0, k0 = self.global_step, self._accum_k
        self._commit(ws, world, skip=self.x3_void)
        if self._void_host is None:
            self._void_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        slot = self._void_slot
        self._void_slot = (slot + 1) % 4
        self._void_host[slot:slot + 1].copy_(self.x3_void, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append({'x': x, 'spk': spk, 'gs0': gs0, 'k': k0, 'ev': ev, 'slot': slot, 'lengths': lengths})      # (lengths: the step's own, for its repeat; k: its place in its window)
        self.host_enqueue_ms = (time.perf_counter() - t_host) * 1e3        # what the host needs to enqueue one step (it must stay below the step's GPU time)
        while len(self._pending) > 1:
            self._resolve_oldest()
        return ws

    def _resolve_oldest(self):
        p = self._pending[0]
        p['ev'].synchronize()
        if int(self._void_host[p['slot']]) == 0:
            self._pending.pop(0)
            self.x3_steps += 1
            return
        pend, self._pending = self._pending, []           # p was flagged: it and everything behind it changed nothing
        self.x3_void.zero_()
        self.global_step = p['gs0']
        for n, q in enumerate(pend):
            self._accum_k = q['k']      # (the oldest's rewinds the window; the others' are what its replay leaves)
            self._train_step_now(q['x'], q['spk'], known_flagged=(n == 0), lengths=q['lengths'])

    def finish_steps(self):
        """Resolve the deferred steps (defer_guard): afterwards parameters, gradients and losses are those of the last step."""
        while self._pending:
            self._resolve_oldest()

    def _x3_overflowed(self):
        """Range flag of this step (max over the data-parallel ranks: every rank must take the same branch)."""
        flag = self.x3_flag
        if self.grad_sync is not None and self.grad_sync.active:
            self.x3_own_flag = int(flag.item())      # (this rank's own verdict, kept for diagnostics)
            self.grad_sync.all_reduce_max(flag)
        return int(flag.item()) != 0

    # ------------------------------------------------------------------ generation
    def decoder_states(self, x, cond, t_end, sink, ratio=64):
        """The decoder's teacher-forced states after a prompt, for a generator's prefill: the input stage and the residual
        stack over prefill_window's window [s0, end) of x (x [B][>= t_end]: raw audio in [-1, 1], or codes for the prior, the
        _decode_input hook's input), with the condition cond [B][Cc][Tz] of the whole utterance (Tz * ratio >= end).  Hands
        net[l] (the input of layer l, [B][R][end - s0], column t - s0) to sink(l, net_l, s0) for l = 0 .. L-1 as soon as it is
        made; a buffer is reused two layers later, so sink must consume it (enqueue its reads) before it returns.  Runs on the
        fp32-MFMA engine (the generator is fp32) and never touches the front or the training workspace.  Returns (s0, end)."""
        self.finish_steps()
        B = x.shape[0]
        Cc, Tz = cond.shape[1], cond.shape[2]
        W, s0, end = prefill_window(t_end, self.ks, self.dil, self.pre_k, ratio)
        if x.dim() != 2 or x.shape[1] < t_end or cond.shape[0] != B or Cc != self.Cc or Tz * ratio < end:
            raise ValueError('decoder_states: x [B][>= %d] and cond [B][%d][>= %d] expected (got %s, %s)'
                             % (t_end, self.Cc, -(-end // ratio), tuple(x.shape), tuple(cond.shape)))
        Tw = end - s0
        if Tw == 0:
            return s0, end
        P, R, L, Mall = self.P, self.R, self.L, self.Mall
        dev = self.dev
        xw = torch.zeros(B, Tw, dtype=x.dtype, device=dev)
        xw[:, :t_end - s0] = x[:, s0:t_end]
        Tzw = Tw // ratio
        cw = cond[:, :, s0 // ratio:end // ratio].contiguous()
        ce = torch.empty(B, Mall, Tzw, device=dev)
        if self.cond_proj:
            K.cond_proj_fwd(cw, P['cond_w'], ce, B=B, Cc=Cc, Mall=Mall, Tz=Tzw)
        else:
            K.conv_gemm(x0=cw, w=P['cond_w'], out0=ce, B=B, T_in=Tzw, T_out=Tzw, M=Mall, C0=Cc, taps=[0])
        ce_flat = ce.view(-1)
        net = [torch.empty(B, R, Tw, device=dev) for _ in range(2)]
        gated = torch.empty(B, R, Tw, device=dev)
        ws = {'B': B, 'T': Tw, 'Tz': Tzw, 'inputs': torch.empty(B, Tw, device=dev),
              'labels': torch.empty(B, Tw, dtype=torch.int32, device=dev), 'net': [net[0]]}
        self._decode_input(xw, ws)
        sink(0, net[0], s0)
        S = self.S
        for l in range(L - 1):           # the top layer's output is not part of the state
            cur, nxt = net[l & 1], net[(l + 1) & 1]
            d = self.dil[l]
            K.conv_gemm(x0=cur, w=P['gated_w'][l], bias=P['gated_b'][l], out0=gated, cond=ce_flat[l * 2 * R * Tzw:],
                        cond_T=Tzw, cond_bstride=Mall * Tzw, B=B, T_in=Tw, T_out=Tw, M=2 * R, C0=R,
                        taps=causal_taps(self.ks, d), epilogue=K.EPI_GATE)
            # the residual half of the 1x1 skip | residual conv only (the skip sum is not part of the state): M0 = 0, every
            # row goes to out1 = aux1 + conv (out0 is never written)
            K.conv_gemm(x0=gated, w=P['out_w'][l].view(-1)[S:], ldw=S + R, bias=P['out_b'][l][S:], out1=nxt, aux1=cur,
                        out0=nxt, B=B, T_in=Tw, T_out=Tw, M=R, M0=0, C0=R, taps=[0], epilogue=K.EPI_ACCUM_SPLIT)
            sink(l + 1, nxt, s0)
        return s0, end

    def free_workspaces(self):
        """Drop the cached (B, T) workspaces (a long-running host changing shapes would otherwise keep them all)."""
        self._ws.clear()

    def state_dict(self):
        if self._accum_k != 0:      # (the accumulator is no part of a checkpoint)
            raise ValueError('state_dict: a window of accumulate = %d is open (%d micro-steps done): a checkpoint is taken at a window boundary'
                             % (self._accumulate, self._accum_k))
        self.finish_steps()
        # x3_scale: the guarded engine's power-of-two plane scales (measured by the last step, used by the next): with them a
        # resumed run continues exactly as the uninterrupted one would (without them its first step runs on the start-up scales)
        sd = {'flat': self.flat, 'ema': self.ema, 'adam_m': self.adam_m, 'adam_v': self.adam_v,
              'x3_scale': self.x3_scale, 'global_step': torch.tensor(self.global_step, dtype=torch.int64)}
        return sd

    def load_state_dict(self, sd):
        self.finish_steps()
        for k in ('flat', 'ema', 'adam_m', 'adam_v'):
            getattr(self, k).copy_(sd[k].to(self.dev))
        if 'x3_scale' in sd and tuple(sd['x3_scale'].shape) == tuple(self.x3_scale.shape):      # (absent in round-2 files)
            self.x3_scale.copy_(sd['x3_scale'].to(self.dev))
        self.global_step = int(sd['global_step'])
        self._accum_k = 0           # (a loaded state starts a window)
