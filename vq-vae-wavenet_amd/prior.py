"""A WaveNet prior over the VQ-VAE's discrete codes (the reference's open TODO, "Train a prior based on vq", README.md; its
prior.py is a stub that never ran).  With it, speech is generated without an input utterance: sample codes from the prior,
decode them with the VQ-VAE's WaveNet decoder (VQVAE.condition_from_codes + generator.FastGenerator).

The prior is the decoder's WaveNet with three differences:
  * its input is a discrete code c[b][t] in [0, k), one per 64 audio samples.  The input stage is
        net0[b][:][t] = b_pre + sum_{j < pre_k} W_pre[j][c[b][t - pre_k + j]][:]     (terms before t = 0 omitted)
    i.e. conv1d_v2(one_hot(shift_right(c)), W_pre, b_pre) with CAUSAL padding (wavenet_ops.py:59-90): tap pre_k - 1 meets the
    previous code.  The one-hot tensor is never materialised (csrc/prior.hip);
  * it has Q = k classes and its loss is the mean cross-entropy of the logits against c[b][t];
  * its only condition is the speaker: its own speaker table (speaker_embedding 0: one-hot speakers, as in VQVAE), tiled
    over condition frames of 64 code steps, the ratio every condition kernel is built for (T must be a multiple of 64).
Everything else -- the residual stack, the head, the fp16x3 engine and its guards, the deferred range flag, the two-stream
backward, the condition projections, Adam + EMA -- is wavenet.WaveNet, which the prior is as the VQ-VAE is, through the same hooks.
"""
import json

import torch

from . import _alloc as A
from . import kernels as K
from .wavenet import WaveNet

CODES_PER_FRAME = 64     # code steps per condition frame
ENCODER_RATIO = {'64': 64}   # audio samples per code of the encoders a prior can be trained on


def load_prior_config(path, vqvae_cfg=None):
    """prior_parameters.json: the format of wavenet_parameters.json plus the prior's own keys (speaker_embedding,
    learning_rate_schedule).  vqvae_cfg: the VQ-VAE's model_parameters; its codebook size k must equal
    quantization_channels, and its encoder must make one code per 64 samples."""
    with open(path) as f:
        cfg = json.load(f)
    check_prior_config(cfg, vqvae_cfg)
    return cfg


def check_prior_config(cfg, vqvae_cfg=None):
    for key in ('quantization_channels', 'residual_filters', 'skip_filters', 'dilation_filters', 'dilation_rates', 'num_cycles',
                'num_cycle_layers', 'kernel_size', 'preprocess', 'speaker_embedding', 'learning_rate_schedule'):
        if key not in cfg:
            raise ValueError('prior config lacks %r' % key)
    if len(cfg['dilation_rates']) != cfg['num_cycles'] * cfg['num_cycle_layers']:
        raise ValueError('prior config: %d dilation rates for %d cycles x %d layers'
                         % (len(cfg['dilation_rates']), cfg['num_cycles'], cfg['num_cycle_layers']))
    if vqvae_cfg is not None:
        if not vqvae_cfg.get('use_vq', True):
            raise ValueError('the VQ-VAE has no codebook (use_vq is false): there are no codes to model')
        if int(vqvae_cfg['k']) != int(cfg['quantization_channels']):
            raise ValueError('prior quantization_channels %d != the VQ-VAE codebook size k = %d'
                             % (cfg['quantization_channels'], vqvae_cfg['k']))
        enc = vqvae_cfg.get('encoder', '64')
        if ENCODER_RATIO.get(enc) != CODES_PER_FRAME:
            raise ValueError('encoder %r does not make one code per 64 samples: the prior needs Encoder_64' % enc)


class LatentPrior(WaveNet):
    """WaveNet prior over VQ codes.  train_step(codes int32 [B][T], spk int64 [B]); T a multiple of 64."""

    scope = 'prior'

    def __init__(self, cfg, num_speakers, device='cuda', seed=0, n_codes=None):
        check_prior_config(cfg)
        if n_codes is not None and int(n_codes) != int(cfg['quantization_channels']):
            raise ValueError('prior quantization_channels %d != codebook size %d' % (cfg['quantization_channels'], n_codes))
        super().__init__(cfg, cfg, num_speakers, device=device, seed=seed)
        self.levels = 256      # the classes are VQ codes: there is no mu-law here, whatever their number

    # ------------------------------------------------------------------ hooks of WaveNet
    def _setup_front(self, cfg, num_speakers):
        if 'time_jitter' in cfg:
            raise ValueError('the latent prior has no encoder and no latents to jitter: time_jitter is a key of the VQ-VAE\'s config')
        if 'codebook_ema' in cfg or 'codebook_restart' in cfg:
            raise ValueError('the latent prior has no codebook: codebook_ema / codebook_restart are keys of the VQ-VAE\'s config')
        if self.sw.dtype == 'bf16':
            raise NotImplementedError('the latent prior has no bf16 storage mode')
        self.Cs = cfg['speaker_embedding']
        self.spk_table = self.Cs > 0
        self.Cs_eff = self.Cs if self.spk_table else (num_speakers + 15) // 16 * 16
        self.Cc_ref = self.Cs if self.spk_table else num_speakers
        self.Cc = self.Cs_eff

    def _front_segments(self, seg):
        if self.spk_table:
            seg['speaker_embedding'] = (self.S_spk, self.Cs)

    def _pre_w_shape(self):
        return (self.pre_k, self.Q, self.R)

    def _init_front(self, P, uus, glorot):
        if self.spk_table:
            P['speaker_embedding'].copy_(uus((self.S_spk, self.Cs), self.S_spk, 2.0))
        else:
            self.onehot = torch.eye(self.S_spk, self.Cs_eff, device=self.dev)

    def _named_front(self, V, out, bn_stats=True):
        if self.spk_table:
            out[self.scope + '/speaker_embedding'] = V['speaker_embedding']

    def _front_workspace(self, B, T, train):
        if T % CODES_PER_FRAME != 0:
            raise ValueError('prior length must be a multiple of %d code steps (got %d)' % (CODES_PER_FRAME, T))
        Tz = T // CODES_PER_FRAME
        ws = {'B': B, 'T': T, 'Tz': Tz, 'ratio': CODES_PER_FRAME}
        ws['labels'] = A.empty(B, T, dtype=torch.int32, device=self.dev)
        ws['cond'] = A.empty(B, self.Cc, Tz, device=self.dev)
        return ws

    def _front_workspace_train(self, ws):
        ws['dnet_t'] = A.empty(ws['B'], ws['T'], self.R, device=self.dev)     # dnet as [B][T][R] for the code-input weight gradient

    def _encode(self, codes, spk, ws, save=True):
        """The prior's condition: the speaker embedding tiled over the frames."""
        K.speaker_tile_fwd(self.P['speaker_embedding'] if self.spk_table else self.onehot, spk, ws['cond'],
                           cond_bstride=self.Cc * ws['Tz'], row0=0, Cs=self.Cs_eff, Tz=ws['Tz'])

    def _decode_input(self, codes, ws):
        K.prior_input_fwd(codes, self.P['pre_w'], self.P['pre_b'], ws['net'][0], ws['labels'])

    def _backward_input(self, codes, ws, dnet):
        B, T = ws['B'], ws['T']
        order, starts = K.prior_code_buckets(codes, self.Q)
        K.transpose(dnet, ws['dnet_t'], B, self.R, T)
        K.prior_input_wgrad(order, starts, ws['dnet_t'], self.G['pre_w'], B=B, T=T)
        K.rowsum(dnet, total=self.G['pre_b'])

    def _backward_front(self, codes, spk, ws):
        if self.spk_table:
            K.speaker_tile_bwd(ws['dcond'], spk, self.G['speaker_embedding'], dcond_bstride=self.Cc * ws['Tz'], row0=0,
                               Cs=self.Cs, Tz=ws['Tz'])

    # ------------------------------------------------------------------ public
    def _check_codes(self, codes, spk):
        if codes.dtype != torch.int32 or codes.dim() != 2 or not codes.is_contiguous():
            raise ValueError('codes must be a contiguous int32 [B][T] tensor')
        if spk.numel() != codes.shape[0]:
            raise ValueError('%d code rows for %d speaker ids' % (codes.shape[0], spk.numel()))

    def forward(self, codes, spk, compute_grad_seed=True, lengths=None):
        self._check_codes(codes, spk)
        return super().forward(codes, spk, compute_grad_seed, lengths)

    def train_step(self, codes, spk, on_forward=None, lengths=None):
        """One Adam + EMA step on the mean cross-entropy of the next code (codes int32 [B][T], T % 64 == 0).  lengths: None, or
        B code counts in 1..T: row b is an utterance of lengths[b] codes from its first one, and the loss is the mean over the
        sum(lengths) real codes -- whatever the row holds behind them changes nothing (WaveNet.train_step)."""
        self._check_codes(codes, spk)
        return super().train_step(codes, spk, on_forward, lengths)

    def evaluate(self, codes, spk, lengths=None, weights='ema', per_position=False):
        """Score held-out code rows (codes int32 [B][T], T % 64 == 0, row b restricted to t < lengths[b]): per row nll_sum,
        entropy_sum (nats), count and hits of the next code, as VQVAE.evaluate (forward only, EMA or live weights, every piece
        of training state left bit-identical).  No codebook statistics: the prior has no codebook."""
        self._check_codes(codes, spk)
        return super().evaluate(codes, spk, lengths=lengths, weights=weights, per_position=per_position)

    def reconstruct(self, codes, spk, lengths=None, weights='ema', mode='sample', uniforms=None, seed=0, temperature=1.0, top_k=0,
                    top_p=1.0, return_probs=False):
        """The prior's teacher-forced code predictions next to the true codes: idx int32 [B][T] (idx[b][t] is the prediction
        for code t given codes[b][:t]; -1 at t >= lengths[b]) and, with return_probs, probs fp32 [B][T][k], as
        VQVAE.reconstruct (the pass evaluate runs, every piece of training state left bit-identical).  No audio: the classes are codes."""
        self._check_codes(codes, spk)
        return self._reconstruct('reconstruct', codes, spk, lengths, weights, mode, uniforms, seed, temperature, top_k, top_p,
                                 return_probs, audio=False)

    def speaker_condition(self, spk, Tz):
        """[B][Cc][Tz]: the speaker embedding tiled over Tz frames (the generator's condition)."""
        B = spk.numel()
        cond = torch.empty(B, self.Cc, Tz, device=self.dev)
        K.speaker_tile_fwd(self.P['speaker_embedding'] if self.spk_table else self.onehot, spk, cond,
                           cond_bstride=self.Cc * Tz, row0=0, Cs=self.Cs_eff, Tz=Tz)
        return cond
