"""VQ-VAE-WaveNet on MI355X: host-side mirror of the reference's model assembly.

Mirrors model.py:7-159 (class VQVAE) of the reference: the front of a wavenet.WaveNet -- one of the three encoders of
encoders.py (self.encoder), the VQ codebook and the speaker embedding make the decoder's condition.  The WaveNet itself, its
training step and the flat parameter buffer are wavenet.py's.
"""
import math

import torch

from . import _alloc as A
from . import kernels as K
from .encoders import Encoder64, Encoder2019, EncoderMagenta
from .wavenet import DEFAULT_ENGINE, WaveNet, load_configs, mix_seed, prefill_window  # noqa: F401  (load_configs, prefill_window, DEFAULT_ENGINE: callers' names)


def cond_conv_config(cfg):
    """(C, k) of the decoder's conditioning conv from a model configuration: 'condition_conv' output channels (absent or 0:
    off, C = 0) and 'condition_conv_kernel' taps (default 3).  Refuses by key what the kernels do not take."""
    C, k = cfg.get('condition_conv', 0), cfg.get('condition_conv_kernel', 3)
    if isinstance(C, bool) or not isinstance(C, int) or C < 0 or C % 16 != 0:
        raise ValueError("'condition_conv' must be a positive multiple of 16 channels, or 0 / absent for none (got %r)" % (C,))
    if isinstance(k, bool) or not isinstance(k, int) or k % 2 != 1 or not 1 <= k <= 7:
        raise ValueError("'condition_conv_kernel' must be odd and in 1..7 (got %r)" % (k,))
    return C, k


class VQVAE(WaveNet):
    """model.py:7-159.  encoder '64' + VQ + speaker embedding + WaveNet decoder."""

    _time_jitter = 0.0     # probability that a latent frame the decoder reads is its neighbour's (time_jitter; 0 = off)
    jitter_seed = 0        # seed of the jitter draws (jitter_uniforms); not part of state_dict
    _jitter_gen = None     # the device generator of jitter_uniforms
    # (_jitter_step, WaveNet's: the step whose forward pass is running inside train_step; None: no jitter, no cluster statistics)
    _codebook_ema = 0.0    # decay of the codebook's moving averages (codebook_ema; 0 = off: Adam trains the codebook)
    _codebook_restart = 0.0    # a code whose moving count falls below this is restarted on an encoder output (codebook_restart; 0 = never)
    codebook_seed = 0      # seed of the restart picks (codebook_uniforms); not part of state_dict
    _codebook_gen = None   # the device generator of codebook_uniforms
    vq_ema_n = None        # fp32 [K]: moving count per code, and
    vq_ema_m = None        # fp32 [K][D]: moving sum of the encoder outputs assigned to it (made at the first such step / by load_state_dict)
    _cb_info = None        # int32 [8]: vqw_vq_codebook_ema_step's info

    def _setup_front(self, model_cfg, num_speakers):
        """What feeds the WaveNet's condition: encoder, VQ codebook, speaker embedding (hook: prior.LatentPrior has only the last)."""
        self.enc = model_cfg.get('encoder', '64')
        encoders = {'64': Encoder64, 'Magenta': EncoderMagenta, '2019': Encoder2019}
        if self.enc not in encoders:
            raise NotImplementedError('encoder %s not implemented' % self.enc)
        self.F = model_cfg.get('encoder_filters', 768)
        self.D = model_cfg['latent_dim']
        self.Kc = model_cfg['k']
        self.Cs = model_cfg['speaker_embedding']
        self.beta = float(model_cfg['beta'])
        self.use_vq = bool(model_cfg.get('use_vq', True))     # false: z_q = e_k = z_e, reconstruction loss only (model.py:139-141)
        self.time_jitter = model_cfg.get('time_jitter', 0.0)  # train_step only: latent frames the decoder reads move
        # the codebook as moving averages of the encoder outputs instead of an Adam-trained variable
        self._set_codebook(model_cfg.get('codebook_ema', 0.0), model_cfg.get('codebook_restart', 0.0))
        # speaker_embedding = 0: the one-hot speaker vector itself is the global condition (model.py:19-27 leaves self.h
        # as [B, 1, num_speakers]); its width is padded to a multiple of 16 channels for the conv engine (the extra
        # condition rows are always zero, their kernel rows never receive a gradient)
        self.spk_table = self.Cs > 0
        self.Cs_eff = self.Cs if self.spk_table else (num_speakers + 15) // 16 * 16
        # the 2019 decoder's conditioning conv over the latents (condition_conv channels, condition_conv_kernel taps):
        # between the VQ and the speaker concat.  Dc: the latent rows of the condition
        self.cconv, self.cconv_k = cond_conv_config(model_cfg)
        self.Dc = self.cconv or self.D
        self.Cc_ref = self.Dc + (self.Cs if self.spk_table else num_speakers)      # the reference's condition width
        self.Cc = self.Dc + self.Cs_eff
        self.encoder = encoders[self.enc](self.D, self.F)     # (constants only: every call hands it the model, encoders.py)

    def _front_segments(self, seg):
        """Flat-buffer segments in front of the WaveNet's: speaker table, encoder, VQ codebook (hook)."""
        if self.spk_table:
            seg['speaker_embedding'] = (self.S_spk, self.Cs)
        seg.update(self.encoder.segments())
        seg['embedding'] = (self.Kc, self.D)
        if self.cconv:
            seg['condition_conv_w'] = (self.cconv_k, self.D, self.cconv)      # [k][D][C]: the Keras layout
            seg['condition_conv_b'] = (self.cconv,)

    def _init_front(self, P, uus, glorot):
        """Initial values of the _front_segments (hook)."""
        if self.spk_table:
            P['speaker_embedding'].copy_(uus((self.S_spk, self.Cs), self.S_spk, 2.0))   # model.py:23-26
        else:
            self.onehot = torch.eye(self.S_spk, self.Cs_eff, device=self.dev)         # row s = one_hot(s), zero padded
        self.encoder.init(P, uus, glorot)
        self.bn_mean = torch.zeros(6 * self.F + self.D, device=self.dev)   # moving stats (never updated:
        self.bn_var = torch.ones(6 * self.F + self.D, device=self.dev)     #  SURVEY.md Appendix A-3)
        P['embedding'].copy_(uus((self.Kc, self.D), self.Kc, 1.7))                  # model.py:47-49
        if self.cconv:          # Keras's defaults: glorot-uniform kernel, zero bias (the flat buffer starts as zeros)
            P['condition_conv_w'].copy_(glorot((self.cconv_k, self.D, self.cconv), self.cconv_k, self.D, self.cconv))

    def _front_scratch(self):
        """Transposed-kernel scratch of the encoder's input-gradient GEMMs (hook)."""
        return self.encoder.scratch(self.dev)

    def _named_front(self, V, out, bn_stats=True):
        """The _front_segments under the reference's names (hook)."""
        if self.spk_table:
            out['speaker_embedding'] = V['speaker_embedding']
        self.encoder.named(self, V, out, bn_stats)
        if self.use_vq:          # (the reference only creates the codebook under use_vq, model.py:137-138)
            out['embedding/embedding'] = V['embedding']
        if self.cconv:
            out['decoder/condition_conv/kernel'] = V['condition_conv_w']
            out['decoder/condition_conv/bias'] = V['condition_conv_b']

    def _front_workspace(self, B, T, train):
        """The (B, T) workspace up to the condition: inputs / labels, encoder + VQ buffers, ws['cond'] (hook)."""
        Tz = self.encoder.latent_len(T)
        dev, D = self.dev, self.D
        e = lambda *s: A.empty(*s, device=dev)  # noqa: E731
        ws = {'B': B, 'T': T, 'Tz': Tz, 'ratio': T // Tz}
        ws['inputs'] = e(B, T)
        ws['labels'] = A.empty(B, T, dtype=torch.int32, device=dev)
        self.encoder.workspace(self, ws, train)
        ws['z_e'] = e(B, D, Tz)
        ws['idx'] = A.empty(B, Tz, dtype=torch.int64, device=dev)
        ws['e_k'] = e(B, D, Tz)
        ws['mind'] = e(B, Tz)
        ws['cond'] = e(B, self.Cc, Tz)
        if self.cconv:          # z_q, what the conditioning conv reads (the jitter puts a second such buffer between them)
            ws['zq'] = e(B, D, Tz)
        return ws

    def _front_workspace_train(self, ws):
        """Backward buffers of the VQ (hook; the encoder's are made with its forward buffers)."""
        B, D, Tz = ws['B'], self.D, ws['Tz']
        ws['dz'] = A.empty(B, D, Tz, device=self.dev)
        if self.cconv:          # d z_q (straight into dz where nothing is quantised) and the partial sums of the conv's weight gradients
            if self.use_vq:
                ws['dzq'] = A.empty(B, D, Tz, device=self.dev)
            ws['cconv_scratch'] = A.empty(K.cond_conv_wgrad_scratch(B, D, self.cconv, Tz, self.cconv_k), device=self.dev)

    # ------------------------------------------------------------------ forward pieces
    def _encode(self, x, spk, ws, save=True):
        """The encoder + model.py:57-74 + decoder_ops.py:39-43 -> ws['cond'] [B][Cc][Tz]."""
        self.encoder.forward(self, x, ws, save)
        self._quantise(spk, ws)

    def _quantise(self, spk, ws):
        """model.py:57-74 (VQ) + model.py:22-27 / decoder_ops.py:39-43 (speaker embedding tiled over time)."""
        if self.cconv:
            return self._quantise_conv(spk, ws)
        P, D, Tz = self.P, self.D, ws['Tz']
        # time jitter (a train_step's passes only): z_q goes to a buffer of its own and the jitter kernel fills the
        # condition's first D rows from it; idx, e_k, mind (the VQ / commitment losses) are those of the un-jittered latents
        jit = ws['jittered'] = self._jitter_step is not None and self._time_jitter > 0.0
        zq, zq_bs = (self._jitter_buffers(ws)['zq'], D * Tz) if jit else (ws['cond'], self.Cc * Tz)
        if self.use_vq:
            K.vq_nearest_fwd(ws['z_e'], P['embedding'], idx=ws['idx'], e_k=ws['e_k'], zq=zq, zq_bstride=zq_bs, mind=ws['mind'])
            if self._codebook_ema > 0.0:      # (a train_step's passes only) the cluster statistics the codebook's update reads
                ws['cb_stats'] = self._jitter_step is not None
                if ws['cb_stats']:
                    self._cluster_stats(ws, self._jitter_step)
        else:                       # z_q = e_k = z_e (model.py:139-141): a copy, no quantisation losses
            (zq if jit else zq[:, :D]).copy_(ws['z_e'])
            ws['idx'].zero_()
            ws['mind'].zero_()
        if jit:
            ws['jitter_u'].copy_(self.jitter_uniforms(ws['B'], Tz, self._jitter_step))
            K.time_jitter_fwd(zq, ws['jitter_u'], ws['cond'], ws['jitter_src'], p=self._time_jitter, D=D,
                              out_bstride=self.Cc * Tz)
        K.speaker_tile_fwd(P['speaker_embedding'] if self.spk_table else self.onehot, spk, ws['cond'],
                           cond_bstride=self.Cc * Tz, row0=D, Cs=self.Cs_eff, Tz=Tz)

    def _quantise_conv(self, spk, ws):
        """_quantise with the conditioning conv: VQ -> ws['zq'], jitter (a train_step's passes only) -> ws['zj'],
        conv of whichever is last -> the condition's first Dc rows, speaker rows behind them.  idx, e_k, mind, the losses and
        the codebook statistics are those of the un-jittered, un-convolved latents."""
        P, D, Tz, zq = self.P, self.D, ws['Tz'], ws['zq']
        jit = ws['jittered'] = self._jitter_step is not None and self._time_jitter > 0.0
        if self.use_vq:
            K.vq_nearest_fwd(ws['z_e'], P['embedding'], idx=ws['idx'], e_k=ws['e_k'], zq=zq, zq_bstride=D * Tz, mind=ws['mind'])
            if self._codebook_ema > 0.0:
                ws['cb_stats'] = self._jitter_step is not None
                if ws['cb_stats']:
                    self._cluster_stats(ws, self._jitter_step)
        else:
            zq.copy_(ws['z_e'])
            ws['idx'].zero_()
            ws['mind'].zero_()
        if jit:
            self._jitter_buffers(ws)
            ws['jitter_u'].copy_(self.jitter_uniforms(ws['B'], Tz, self._jitter_step))
            K.time_jitter_fwd(zq, ws['jitter_u'], ws['zj'], ws['jitter_src'], p=self._time_jitter, D=D)
        ws['cconv_in'] = ws['zj'] if jit else zq
        K.cond_conv_fwd(ws['cconv_in'], P['condition_conv_w'], P['condition_conv_b'], ws['cond'], out_bstride=self.Cc * Tz)
        K.speaker_tile_fwd(P['speaker_embedding'] if self.spk_table else self.onehot, spk, ws['cond'],
                           cond_bstride=self.Cc * Tz, row0=self.Dc, Cs=self.Cs_eff, Tz=Tz)

    # ------------------------------------------------------------------ time jitter
    @property
    def time_jitter(self):
        """Probability that a latent frame the decoder reads in train_step is replaced by its left or right neighbour of the
        same utterance (p / 2 each; arXiv 1901.08810).  0: off, the step is what it was without this attribute.
        forward() called directly, evaluate, encode and the generators never jitter.  Not part of state_dict."""
        return self._time_jitter

    @time_jitter.setter
    def time_jitter(self, value):
        K.jitter_thresholds(value)                    # (refuses what is not a probability)
        self._time_jitter = float(value)

    def _jitter_buffers(self, ws):
        """z_q before the jitter, its gradient, the step's uniforms and source frames: made at the first jittered step.  (With
        the conditioning conv z_q has its buffer already, and the jitter's own output and its gradient are made here: zj, dzj.)"""
        if 'jitter_src' not in ws:
            B, D, Tz = ws['B'], self.D, ws['Tz']
            a, b = ('zj', 'dzj') if self.cconv else ('zq', 'dzq')
            with A.record(ws['_poison']):
                ws[a], ws[b] = A.empty(B, D, Tz, device=self.dev), A.empty(B, D, Tz, device=self.dev)
                ws['jitter_u'] = A.empty(B, Tz, device=self.dev)
            ws['jitter_src'] = torch.zeros(B, Tz, dtype=torch.int32, device=self.dev)
        return ws

    def jitter_uniforms(self, B, Tz, step):
        """The uniforms [B][Tz] (fp32 in [0, 1), on the device) that decide step `step`'s jitter: a pure function of
        (jitter_seed, step, data-parallel rank; with accumulate > 1 also accum_index) -- a device generator of its own, seeded again at every call, so the global
        torch RNG is never touched and every pass that belongs to one step (the fp16x3 attempt, its fp32 repeat, a deferred
        step run again) draws the same values.  No host sync.  Each data-parallel rank draws its own stream: a sharded batch
        is not the same draw as the full batch."""
        if self._jitter_gen is None:
            self._jitter_gen = torch.Generator(device=self.dev)
        rank = self.grad_sync.rank if self.grad_sync is not None else 0
        # (accumulate > 1: the micro-step's place in its window is a seed word too -- the micro-batches of one step draw apart)
        words = (step, rank) if self._accumulate == 1 else (step, rank, self._accum_k)
        self._jitter_gen.manual_seed(mix_seed(self.jitter_seed, *words))
        return torch.rand(B, Tz, generator=self._jitter_gen, device=self.dev)

    def jitter_moved(self, ws):
        """Share of the (b, t) whose frame moved (src != t) in the last jittered pass on ws (synchronises); 0.0 without jitter."""
        if not ws.get('jittered'):
            return 0.0
        self.finish_steps()
        src = ws['jitter_src']
        return float((src != torch.arange(ws['Tz'], dtype=torch.int32, device=self.dev)).float().mean())

    # ------------------------------------------------------------------ codebook by moving averages
    @property
    def codebook_ema(self):
        """Decay of the codebook's moving averages (sonnet's VectorQuantizerEMA).  0: off, the codebook is an Adam-trained
        variable and the step is what it was without this attribute.  0 < decay < 1: train_step moves the codebook to the moving
        average of the encoder outputs assigned to each code, it gets no gradient and `loss` has no codebook term."""
        return self._codebook_ema

    @codebook_ema.setter
    def codebook_ema(self, value):
        self._set_codebook(value, self._codebook_restart)

    @property
    def codebook_restart(self):
        """Threshold below which a code's moving count makes it dead: it is restarted on an encoder output of the batch.
        0: never.  Needs codebook_ema."""
        return self._codebook_restart

    @codebook_restart.setter
    def codebook_restart(self, value):
        self._set_codebook(self._codebook_ema, value)

    def _set_codebook(self, decay, restart):
        K.codebook_ema_constants(decay, restart)      # (refuses what is no decay / no threshold)
        if (float(decay) != 0.0 or float(restart) != 0.0) and not self.use_vq:
            raise ValueError('codebook_ema / codebook_restart need a codebook (use_vq is false)')
        if float(decay) > 0.0 and self._accumulate > 1:      # (the other order is refused by WaveNet.accumulate)
            raise ValueError("codebook_ema with accumulate > 1 is not supported: the codebook's own update per micro-batch has no rule yet")
        self._codebook_ema, self._codebook_restart = float(decay), float(restart)

    def _world(self):
        """(world, rank) of the exchange of the cluster statistics: (1, 0) unless a data-parallel grad_sync is active."""
        gs = self.grad_sync
        return (gs.world, gs.rank) if gs is not None and gs.active else (1, 0)

    def _codebook_buffers(self, ws):
        """The statistics of a pass, made at the first such step: cnt int32 [K] and ONE fp32 buffer sum [K][D] | cand [K][D] |
        float(cnt) [K] (what the data-parallel ranks exchange in one all-reduce)."""
        if 'cb_pack' not in ws:
            Kc, D, dev = self.Kc, self.D, self.dev
            if ws['B'] * ws['Tz'] * self._world()[0] > 2 ** 24:
                raise ValueError('codebook_ema: more than 2^24 frames per step (the ranks exchange the counts as fp32, exact up to there)')
            with A.record(ws['_poison']):
                ws['cb_pack'] = A.empty(Kc * (2 * D + 1), device=dev)
                ws['cb_u'] = A.empty(Kc, device=dev)
            ws['cb_sum'], ws['cb_cand'] = ws['cb_pack'][:Kc * D].view(Kc, D), ws['cb_pack'][Kc * D:2 * Kc * D].view(Kc, D)
            ws['cb_cntf'] = ws['cb_pack'][2 * Kc * D:]
            ws['cb_cnt'] = torch.zeros(Kc, dtype=torch.int32, device=dev)
            ws['cb_pick'] = torch.zeros(Kc, dtype=torch.int32, device=dev)
        return ws

    def _cluster_stats(self, ws, step):
        """cnt / sum of the un-jittered z_e, idx of this pass and, with restarts on, cand = the frame pick[k] = min(int(u[k] * Nf), Nf - 1)
        (an fp32 product; the kernel clamps) for u = codebook_uniforms(K, step)."""
        self._codebook_buffers(ws)
        pick = cand = None
        if self._codebook_restart > 0.0:
            pick, cand = ws['cb_pick'], ws['cb_cand']
            torch.mul(self.codebook_uniforms(self.Kc, step), float(ws['B'] * ws['Tz']), out=ws['cb_u'])
            pick.copy_(ws['cb_u'])                    # (fp32 -> int32: truncation)
        K.vq_cluster_stats(ws['z_e'], ws['idx'], cnt=ws['cb_cnt'], sum=ws['cb_sum'], pick=pick, cand=cand, K=self.Kc)

    def codebook_uniforms(self, Kc, step):
        """The uniforms [K] (fp32 in [0, 1), on the device) behind step `step`'s restart picks: a pure function of
        (codebook_seed, step) -- a device generator of its own, seeded again at every call as jitter_uniforms seeds its one, so
        the global torch RNG is never touched and the attempt, its fp32 repeat and a deferred step run again draw the same
        picks.  No host sync.  Every data-parallel rank draws the same values (and picks among its own frames)."""
        if self._codebook_gen is None:
            self._codebook_gen = torch.Generator(device=self.dev)
        self._codebook_gen.manual_seed(mix_seed(self.codebook_seed, step, 0x636F6465626F6F6B))      # (the last word keeps the stream apart from the jitter's)
        return torch.rand(Kc, generator=self._codebook_gen, device=self.dev)

    def _codebook_state(self, reset=False):
        """vq_ema_n = 1, vq_ema_m = the embedding, made at the first moving-average step (reset: made again from the current
        embedding).  The embedding's Adam slots are zeroed with it: from here on its gradient is zero, and Adam leaves a variable
        with zero gradient and zero slots bit for bit (a checkpoint trained the old way arrives with slots that would go on moving it)."""
        if self.vq_ema_n is None or reset:
            o, shp = self.seg_off['embedding']
            self.vq_ema_n = torch.ones(self.Kc, device=self.dev)
            self.vq_ema_m = self.P['embedding'].detach().clone()
            self._cb_info = torch.zeros(8, dtype=torch.int32, device=self.dev)
            self.adam_m[o:o + math.prod(shp)].zero_()
            self.adam_v[o:o + math.prod(shp)].zero_()

    def _front_step(self, ws, skip=None):
        """The codebook's update from the statistics of the pass that is kept, enqueued right before apply_gradients (skip: as
        there).  Data parallel: the ranks first sum sum | cand | float(cnt) in one all-reduce on this stream; cand[k] comes from
        rank k % world alone (the others contribute zeros), so every rank applies the same restart."""
        if not (self._codebook_ema > 0.0 and ws.get('cb_stats')):
            return
        self._codebook_state()
        restart = self._codebook_restart
        if self.grad_sync is not None and self.grad_sync.active:
            ws['cb_cntf'].copy_(ws['cb_cnt'])
            if restart > 0.0:
                if ws.get('cb_world') != self._world():      # codes whose restart candidate another rank supplies
                    ws['cb_world'] = world, rank = self._world()
                    ws['cb_other'] = (torch.arange(self.Kc, device=self.dev) % world != rank).view(self.Kc, 1)
                ws['cb_cand'].masked_fill_(ws['cb_other'], 0.0)
            else:
                ws['cb_cand'].zero_()
            self.grad_sync.all_reduce_sum(ws['cb_pack'])
            ws['cb_cnt'].copy_(ws['cb_cntf'])
        K.vq_codebook_ema_step(self.P['embedding'], self.vq_ema_n, self.vq_ema_m, cnt=ws['cb_cnt'], sum=ws['cb_sum'],
                               cand=ws['cb_cand'] if restart > 0.0 else None, decay=self._codebook_ema, restart=restart,
                               info=self._cb_info, skip=skip)

    def codebook_info(self):
        """{'used': codes that won a frame, 'restarted': codes restarted} in the last applied moving-average step (zeros before
        the first).  Synchronises."""
        self.finish_steps()
        used = restarted = 0
        if self._cb_info is not None:
            restarted, used = self._cb_info[:2].tolist()
        return {'used': used, 'restarted': restarted}

    def _front_plan(self, B, T, save, active):
        # encoder layers (1..5) whose conv and input gradient run on the fp16x3 engine (training workspaces only: train_step reads the
        # step's range flag): channel blocks of 128; the 256-column tiles over the flat (batch, time) rows may be partial (layers 4, 5: 1664,
        # 832 columns at B = 8).  Slots of ws['enc_scale'] / ws['enc_amax']: 0 the kernels, i the input of layer i, 5 + i d(its conv output)
        enc, Tl = self.encoder.on_engine(self), [T // (2 ** (i + 1)) for i in range(6)]
        enc_x3 = tuple(i for i in (1, 2, 3, 4, 5) if B * Tl[i] >= 256 and Tl[i - 1] == 2 * Tl[i]) if (enc and active and save and self.sw.enc_x3) else ()
        return enc_x3, enc

    # training on row lengths is the causal WaveNet's (LatentPrior): here the encoder sees the padding, and the VQ / commitment
    # losses, the codebook statistics and the jitter would each need a mask of their own
    _masked_training = ('the VQ-VAE does not train on lengths: its encoder is not causal, and the VQ and commitment losses, the '
                        'codebook statistics and the jitter are not masked')

    def _front_loss(self, ws):
        """loss_buf[1] = the sum of the VQ distances (hook)."""
        K.rowsum(ws['mind'].view(1, 1, -1), total=self.loss_buf[1:2])

    # ------------------------------------------------------------------ held-out scoring
    def _length_unit(self):
        """What a row's scored length must be a multiple of: the encoder's ratio (hook: the prior has no encoder)."""
        return self.encoder.ratio

    def reconstruct(self, x, spk, lengths=None, weights='ema', mode='sample', uniforms=None, seed=0, temperature=1.0, top_k=0,
                    top_p=1.0, return_probs=False):
        """The decoder's teacher-forced reconstruction of x [B][T]: exactly the pass evaluate runs (score workspace, EMA or
        live weights, the fp32 repeat of a flagged pass, the same `lengths` rules, every piece of training state bit-identical
        afterwards, also when the call raises), then ONE class per position from its logits (kernels.softmax_sample).
        Returns (audio fp32 [B][T], idx int32 [B][T]) and, with return_probs, probs fp32 [B][T][Q] (the distribution drawn
        from).  idx[b][t] is the prediction for sample t given x[b][:t]: it aligns with the labels evaluate scores, and
        mode 'greedy' hits exactly where evaluate counts a hit.  Positions t >= lengths[b] read idx -1, audio 0, probs 0.
        mode 'sample': temperature / top_k / top_p as FastGenerator.generate takes them (scalars or one value per row) and
        uniforms fp32 [B][T] in [0, 1]; None: drawn from a device generator of their own seeded with `seed` (as
        jitter_uniforms does it: the global torch RNG is never touched; the same seed gives the same uniforms, and the same
        audio wherever two passes make the same logits -- they differ by about 1e-6, DESIGN 3.8, so a draw whose uniform
        lies that close to a cdf value can differ between two calls).  Synchronises."""
        return self._reconstruct('reconstruct', x, spk, lengths, weights, mode, uniforms, seed, temperature, top_k, top_p,
                                 return_probs, audio=True)

    def _score_front(self, ws, f_end, out):
        """evaluate's codebook part.  With use_vq the Score also holds the per-row sum of VQ distances over the frames
        f < lengths[b] // ratio, their number, the batch's code counts [k] and the codes [B][Tz] themselves.  lengths are multiples
        of the encoder's ratio (64; 320 for '2019').  The encoder is NOT causal: the last latent frames of a row shorter than T do
        see the zero padding behind it (Encoder_64's strided convs reach about 190 samples ahead), so such a row scores as that
        padded input does, not as the utterance alone would."""
        if self.use_vq:
            self._score_codes(ws, f_end, out)

    def _score_codes(self, ws, f_end, out):
        """Codebook statistics of a scored batch: code counts and per-row VQ distance sums over the valid frames."""
        B, Tz = ws['B'], ws['Tz']
        counts = torch.zeros(self.Kc, dtype=torch.int32, device=self.dev)
        flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        K.code_histogram(ws['idx'], counts, flag, f_end=f_end)
        mind = ws['mind'].double()
        if f_end is not None:
            mind = mind * (torch.arange(Tz, device=self.dev)[None, :] < f_end[:, None])
        out.vq_sum = mind.sum(1).cpu()
        out.frames = torch.full((B,), Tz, dtype=torch.int64) if f_end is None else f_end.cpu().long()
        out.code_counts = counts.cpu().long()
        out.codes = ws['idx'].clone()
        if int(flag.item()) != 0:
            raise RuntimeError('evaluate: a VQ index outside [0, %d)' % self.Kc)

    def losses(self, ws):
        """(loss, reconstruction, vq, commitment) as python floats (synchronises; hook)."""
        self.finish_steps()
        v = self.loss_buf.tolist()
        recon = v[0] / (ws['B'] * ws['T'])
        vq = v[1] / (ws['B'] * ws['Tz'] * self.D) if self.use_vq else 0.0   # model.py:100
        commit = self.beta * vq                             # model.py:103 (same forward value)
        if self._codebook_ema > 0.0:                        # the codebook term is not optimised (sonnet's VectorQuantizerEMA)
            return recon + commit, recon, vq, commit
        return recon + vq + commit, recon, vq, commit

    def summaries(self, ws, bins=30):
        """What the reference hands to TensorBoard every `-interval` steps (model.py:28-69,95-104; train.py:104-109), as plain
        numbers: for every histogram tag its min / max / mean / std and `bins` equal-width counts, plus the loss scalars.
        `_u` / `_v` are the mean / variance over the last (feature) axis, as tf.nn.moments(x, [-1]).  The reference's
        'distances' histogram is over the [B, Tz, K] tensor this build never materialises; 'distances_min' (the distance to
        the chosen code) stands in for it.  Synchronises."""
        self.finish_steps()
        def hist(t):
            t = t.detach().float().reshape(-1)
            lo, hi = float(t.min()), float(t.max())
            counts = torch.histc(t, bins=bins, min=lo, max=hi if hi > lo else lo + 1.0)
            return {'min': lo, 'max': hi, 'mean': float(t.mean()), 'std': float(t.std()) if t.numel() > 1 else 0.0,
                    'counts': [int(c) for c in counts.tolist()]}

        def moments(t):          # features on the last axis
            return t.mean(-1), t.var(-1, unbiased=False)
        out = {}
        z_e = ws['z_e'].permute(0, 2, 1)                    # [B, Tz, D] as the reference holds it
        tags = {'z_e': z_e}
        if self.spk_table:
            tags['speaker_embedding'] = self.P['speaker_embedding']
        if self.use_vq:
            tags['embedding'] = self.P['embedding']
            tags['e_k'] = ws['e_k'].permute(0, 2, 1)
            out['q(z|x)'] = hist(ws['idx'])
            out['distances_min'] = hist(ws['mind'])
        for name, t in tags.items():
            out[name] = hist(t)
            if name != 'e_k':
                u, v = moments(t)
                out[name + '_u'], out[name + '_v'] = hist(u), hist(v)
        loss, recon, vq, commit = self.losses(ws)
        out['reconstruction_loss'] = recon
        if self.use_vq:
            out['vq_loss'], out['commitment_loss'] = vq, commit
        return out

    def _backward_prepare(self):
        """Transposed kernels of the encoder's backward pass (hook)."""
        self.encoder.transpose(self)

    def _backward_front(self, x, spk, ws):
        """From d cond on: speaker embedding, VQ and encoder backward (hook)."""
        G, D, B, Tz = self.G, self.D, ws['B'], ws['Tz']
        if self.grad_sync is not None:      # decoder gradients are final: exchange them under the encoder backward
            self.grad_sync.bucket_ready(self.seg_off['pre_w'][0], self.n_flat)
        # ---- speaker embedding + VQ (model.py:22-27, 57-74, 99-106)
        if self.spk_table:
            K.speaker_tile_bwd(ws['dcond'], spk, G['speaker_embedding'], dcond_bstride=self.Cc * Tz, row0=self.Dc, Cs=self.Cs, Tz=Tz)
        nd = float(B * Tz * D)
        dzq, dzq_bs = ws['dcond'], self.Cc * Tz
        if self.cconv:
            # the conditioning conv: weight and bias gradients, then d z_q from d cond's first Dc rows -- through the jitter's
            # transposed gather where the pass jittered (straight into dz where nothing is quantised)
            K.cond_conv_wgrad(ws['cconv_in'], ws['dcond'], G['condition_conv_w'], G['condition_conv_b'], ws['cconv_scratch'],
                              dout_bstride=self.Cc * Tz)
            dzq, dzq_bs = ws['dzq'] if self.use_vq else ws['dz'], D * Tz
            dzc = ws['dzj'] if ws.get('jittered') else dzq
            K.cond_conv_dgrad(self.P['condition_conv_w'], ws['dcond'], dzc, dout_bstride=self.Cc * Tz)
            if ws.get('jittered'):
                K.time_jitter_bwd(dzc, ws['jitter_src'], dzq, D=D)
        elif ws.get('jittered'):      # d z_q from d cond through the transposed gather (straight into dz where nothing is quantised)
            dzq, dzq_bs = ws['dzq'] if self.use_vq else ws['dz'], D * Tz
            K.time_jitter_bwd(ws['dcond'], ws['jitter_src'], dzq, D=D, dout_bstride=self.Cc * Tz)
        if self.use_vq:
            K.vq_nearest_bwd(ws['z_e'], ws['e_k'], ws['idx'], dzq=dzq, dzq_bstride=dzq_bs, dz_e=ws['dz'],
                             demb=None if self._codebook_ema > 0.0 else G['embedding'],      # (moving averages: no codebook-loss gradient)
                             cscale=2.0 * self.beta / nd, escale=2.0 / nd, K=self.Kc)
        elif not ws.get('jittered') and not self.cconv:
            ws['dz'].copy_(ws['dcond'][:, :D])
        self.encoder.backward(self, x, ws)

    # ------------------------------------------------------------------ generation
    def encode(self, x, spk):
        """model.encoding of generate.py:92: [B][Cc][Tz] (channel-major).  x [B][T], or ONE utterance [1][T] with
        B speaker ids (generate.py:40 repeats the utterance per speaker: the encoder and VQ then run once and only the
        speaker rows of the condition differ)."""
        self.finish_steps()
        Bx, T = x.shape
        B = spk.numel()
        if Bx != B and Bx != 1:
            raise ValueError('encode: %d utterances for %d speaker ids' % (Bx, B))
        ws = self._workspace(Bx, T, train=False)
        self._encode(x, spk[:Bx].contiguous(), ws, save=False)
        if Bx == B:
            return ws['cond'].clone()
        cond = ws['cond'].repeat(B, 1, 1)
        K.speaker_tile_fwd(self.P['speaker_embedding'] if self.spk_table else self.onehot, spk, cond,
                           cond_bstride=self.Cc * ws['Tz'], row0=self.Dc, Cs=self.Cs_eff, Tz=ws['Tz'])
        return cond

    def encode_codes(self, x, spk):
        """The VQ indices [B][Tz] (int32) that encode() computes for x [B][T]: the discrete codes a latent prior
        (prior.LatentPrior) models."""
        if not self.use_vq:
            raise ValueError('encode_codes: the model has no codebook (use_vq is false)')
        self.finish_steps()
        B, T = x.shape
        ws = self._workspace(B, T, train=False)
        self._encode(x, spk.contiguous(), ws, save=False)
        return ws['idx'].to(torch.int32)

    def condition_from_codes(self, codes, spk):
        """The [B][Cc][Tz] condition [embedding[codes]; speaker] that encode() produces for those VQ codes (model.py:57-74 +
        decoder.py:30-31): decodes codes sampled from a latent prior."""
        if not self.use_vq:
            raise ValueError('condition_from_codes: the model has no codebook (use_vq is false)')
        self.finish_steps()
        B, Tz = codes.shape
        if spk.numel() != B:
            raise ValueError('condition_from_codes: %d code rows for %d speaker ids' % (B, spk.numel()))
        cond = torch.empty(B, self.Cc, Tz, device=self.dev)
        z_q = self.P['embedding'][codes.long()].permute(0, 2, 1)                   # e_k = the chosen rows, exactly
        if self.cconv:          # the conv encode() runs on them
            K.cond_conv_fwd(z_q.contiguous(), self.P['condition_conv_w'], self.P['condition_conv_b'], cond, out_bstride=self.Cc * Tz)
        else:
            cond[:, :self.D] = z_q
        K.speaker_tile_fwd(self.P['speaker_embedding'] if self.spk_table else self.onehot, spk, cond,
                           cond_bstride=self.Cc * Tz, row0=self.Dc, Cs=self.Cs_eff, Tz=Tz)
        return cond

    def state_dict(self):
        """WaveNet's, with the BatchNorm statistics (behind the optimiser's slots, where a VQ-VAE's files have always had them) and, with
        codebook_ema, the codebook's moving averages (before the first such step: n = 1, m = the embedding)."""
        sd = super().state_dict()
        rest = {k: sd.pop(k) for k in ('x3_scale', 'global_step')}
        sd.update(bn_mean=self.bn_mean, bn_var=self.bn_var, **rest)
        if self._codebook_ema > 0.0:
            self._codebook_state()
            sd.update(vq_ema_n=self.vq_ema_n, vq_ema_m=self.vq_ema_m)
        if self.cconv:          # (channels, taps): a model of another setting refuses the state by this key
            sd['condition_conv'] = torch.tensor([self.cconv, self.cconv_k], dtype=torch.int64)
        return sd

    def load_state_dict(self, sd):
        theirs = tuple(int(v) for v in sd['condition_conv']) if 'condition_conv' in sd else (0, self.cconv_k)
        if theirs[0] != self.cconv or (self.cconv and theirs[1] != self.cconv_k):
            raise ValueError("load_state_dict: 'condition_conv' is %d (kernel %d) in the state and %d (kernel %d) in the model: the "
                             "decoder's local_condition kernels have %d rows there and %d here"
                             % (theirs + (self.cconv, self.cconv_k, (theirs[0] or self.D) + self.Cs_eff, self.Cc)))
        super().load_state_dict(sd)
        for k in ('bn_mean', 'bn_var'):
            getattr(self, k).copy_(sd[k].to(self.dev))
        if self._codebook_ema > 0.0:
            # a state saved without the moving averages (trained the old way): n = 1, m = the loaded embedding, its Adam slots zeroed
            if 'vq_ema_n' in sd and 'vq_ema_m' in sd:
                self.vq_ema_n = sd['vq_ema_n'].to(self.dev, torch.float32).clone().reshape(self.Kc)
                self.vq_ema_m = sd['vq_ema_m'].to(self.dev, torch.float32).clone().reshape(self.Kc, self.D)
                self._cb_info = torch.zeros(8, dtype=torch.int32, device=self.dev)
            else:
                self._codebook_state(reset=True)
