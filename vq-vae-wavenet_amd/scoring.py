"""Held-out scoring, host side: the result of VQVAE.evaluate / LatentPrior.evaluate and the numbers derived from it.
Pure Python over small host arrays (no GPU needed):

    bits(nll_sum, count)   = nll_sum / (count * ln 2)            bits per scored position
    perplexity(counts)     = exp(-sum p ln p),  p = counts / counts.sum(), zeros ignored, float64
    used(counts)           = number of codes that occur at all

Conversion scoring (mcd, on the GPU): mel-cepstral distortion between a converted utterance x and the target speaker's own
recording y of the same sentence, in dB:

    MCD(x, y) = (10 sqrt(2) / ln 10) * (1 / N) * sum over the DTW path (i, j) of  sqrt(sum_{d=1..12} (cx[d][i] - cy[d][j])^2)

with N the number of cells on the path.  The path is the symmetric-step DTW alignment (no slope weights, no band) that
minimises the summed frame distance; c0 (energy) is left out.  The cepstra cx, cy are the 13 MFCCs of vqw_mfcc / ops.mfcc
(frame 400, step 160 at 16 kHz: 100 frames per second; 80 mel bins, log, DCT-II): NOT the mel-generalised cepstra (MGC, e.g.
SPTK mcep order 24) that published MCD figures usually rest on, so the number compares systems scored HERE with one
another and is not comparable with figures from papers.
"""
import collections
import math

import numpy as np

FRAME_STEP = 160                                           # vqw_mfcc: samples per cepstral frame
MAX_FRAMES = 4096                                          # vqw_cepstral_dtw's bound (41 s)
MCD_K = 10.0 * math.sqrt(2.0) / math.log(10.0)             # 6.1418...: Euclidean cepstral distance -> dB

MCD = collections.namedtuple('MCD', 'mcd cost steps frames_x frames_y')
_mel = {}


def frames_of(n):
    """Cepstral frames of an utterance of n samples: ceil(n / 160) (stft with pad_end)."""
    return -(-int(n) // FRAME_STEP)


def mcd(x, y, nx=None, ny=None):
    """Mel-cepstral distortion of every pair (x[p], y[p]).  x fp32 [P][Tx], y fp32 [P][Ty]: audio on the GPU, each row ZERO
    beyond its nx[p] / ny[p] samples (lists of P; None: whole rows).  Per pair: the MFCCs of both sides (ops.mfcc's kernel,
    written as [P][13][frames], which is the layout vqw_cepstral_dtw reads), frames = ceil(n / 160), then the DTW over
    coefficients 1..12.  Two mfcc launches and one dtw launch per call; the cost and path length come back to the host and
    mcd = MCD_K * cost / steps is formed there in float64.  Returns MCD(mcd float64 [P], cost float32 [P], steps int32 [P],
    frames_x int32 [P], frames_y int32 [P]) as numpy arrays.  A pair's numbers do not depend on the rest of the batch."""
    import torch
    from . import kernels as K
    from .encoders import mel_weight_matrix
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0]:
        raise ValueError('mcd: x must be [P][Tx] and y [P][Ty] with the same P (got %s and %s)' % (tuple(x.shape), tuple(y.shape)))
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError('mcd: audio must be float32 (got %s and %s)' % (x.dtype, y.dtype))
    P = x.shape[0]
    frames = []
    for n, t, what in ((nx, x, 'nx'), (ny, y, 'ny')):
        n = [t.shape[1]] * P if n is None else [int(v) for v in n]
        if len(n) != P or min(n) < 1 or max(n) > t.shape[1]:
            raise ValueError('mcd: %s must hold %d sample counts in 1..%d (got %s)' % (what, P, t.shape[1], n[:8]))
        frames.append(np.array([frames_of(v) for v in n], dtype=np.int32))
    dev = x.device
    if dev not in _mel:
        _mel[dev] = mel_weight_matrix().to(dev).contiguous()
    cep = []
    for t in (x, y):
        c = torch.empty(P, 13, frames_of(t.shape[1]), device=dev)
        K.mfcc(t.contiguous(), _mel[dev], c, n_keep=13)
        cep.append(c)
    na, nb = (torch.from_numpy(f).to(dev) for f in frames)
    cost, steps = K.cepstral_dtw(cep[0], cep[1], na=na, nb=nb, d0=1, D=12)
    cost, steps = cost.cpu().numpy(), steps.cpu().numpy()
    return MCD(MCD_K * cost.astype(np.float64) / steps.astype(np.float64), cost, steps, frames[0], frames[1])


def mcd_report(results, missing=0):
    """The report of score_conversion.py from a list of MCD results (one per batch): pairs, missing, the mean MCD per pair,
    the frame-weighted mean sum(MCD_K * cost) / sum(steps), min, max and the total frames of both sides.  float64 sums in
    list order."""
    m = np.concatenate([r.mcd for r in results])
    cost = np.concatenate([r.cost for r in results]).astype(np.float64)
    steps = np.concatenate([r.steps for r in results]).astype(np.int64)
    frames = int(sum(int(r.frames_x.sum()) + int(r.frames_y.sum()) for r in results))
    return {'pairs': int(m.size), 'missing': int(missing), 'mcd_mean': float(m.mean()),
            'mcd_frame_weighted': float(MCD_K * cost.sum() / steps.sum()), 'mcd_min': float(m.min()), 'mcd_max': float(m.max()),
            'frames': frames, 'path_steps': int(steps.sum())}


def bits(nll_sum, count):
    """Bits per scored position from a sum of negative log-likelihoods in nats."""
    count = float(count)
    if count <= 0:
        raise ValueError('bits: no scored positions')
    return float(nll_sum) / (count * math.log(2.0))


def perplexity(counts):
    """exp of the entropy of the code distribution p = counts / counts.sum() (float64; codes that never occur add nothing)."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    if (c < 0).any() or c.sum() <= 0:
        raise ValueError('perplexity: counts must be non-negative and not all zero')
    p = c[c > 0] / c.sum()
    return float(np.exp(-(p * np.log(p)).sum()))


def used(counts):
    """How many codes occur at least once."""
    return int((np.asarray(counts).reshape(-1) > 0).sum())


class Score:
    """What evaluate() returns.  Per row (host tensors of B elements): nll_sum, entropy_sum (float64, nats), count, hits
    (int64); with a codebook: vq_sum (float64: the sum of the VQ distances over the row's valid frames), frames (int64) and
    code_counts (int64 [k], the whole batch) and codes (device int64 [B][Tz]); with per_position: nll, entropy (device fp32 [B][T], 0 where not scored)."""

    def __init__(self, nll_sum, entropy_sum, count, hits):
        self.nll_sum, self.entropy_sum, self.count, self.hits = nll_sum, entropy_sum, count, hits
        self.vq_sum = self.frames = self.code_counts = self.codes = None
        self.nll = self.entropy = None

    def row_bits(self):
        """Bits per scored position of every row."""
        return [bits(n, c) for n, c in zip(self.nll_sum.tolist(), self.count.tolist())]


class Totals:
    """Sums of Score objects over batches (and, merged on rank 0, over ranks): integer counts and float64 sums only, added
    in the order they arrive."""
    FIELDS = ('nll', 'entropy', 'count', 'hits', 'vq', 'frames', 'rows')

    def __init__(self, k=0):
        self.nll = self.entropy = self.vq = 0.0
        self.count = self.hits = self.frames = self.rows = 0
        self.code_counts = np.zeros(k, dtype=np.int64)

    def add(self, score):
        self.nll += float(score.nll_sum.sum())
        self.entropy += float(score.entropy_sum.sum())
        self.count += int(score.count.sum())
        self.hits += int(score.hits.sum())
        self.rows += int(score.count.numel())
        if score.code_counts is not None:
            self.vq += float(score.vq_sum.sum())
            self.frames += int(score.frames.sum())
            self.code_counts += score.code_counts.numpy()

    def merge(self, other):
        for f in self.FIELDS:
            setattr(self, f, getattr(self, f) + getattr(other, f))
        self.code_counts = self.code_counts + other.code_counts

    def report(self, unit='sample', latent_dim=0):
        """The numbers of the evaluation report: bits per `unit`, mean nll / entropy (nats), top-1 accuracy over the scored
        positions; with a codebook the vq_loss mean (distance per latent element, model.py:100), codes used and perplexity."""
        out = {'bits_per_' + unit: bits(self.nll, self.count), 'nll': self.nll / self.count, 'entropy': self.entropy / self.count,
               'accuracy': self.hits / self.count, unit + 's': self.count}
        if self.frames and latent_dim:
            out.update(vq_loss=self.vq / (self.frames * latent_dim), codes_used=used(self.code_counts),
                       codes=int(self.code_counts.size), code_perplexity=perplexity(self.code_counts))
        return out


def score_batches(model, batches, dev, weights='ema', rows=None, prior=None, prior_totals=None):
    """Score (files, x, speaker ids, lengths) batches (data.padded_batches; lengths None: whole rows) with model.evaluate and
    return their Totals.  rows: a list that receives one {file, speaker, samples, bits, accuracy} per utterance.  prior /
    prior_totals: also score every row's codes (its first lengths[b] // ratio frames) with the latent prior."""
    totals = Totals(model.Kc if model.use_vq else 0)
    for files, x, spk, lengths in batches:
        spk_d = spk.to(dev)
        sc = model.evaluate(x.to(dev), spk_d, lengths=lengths, weights=weights)
        totals.add(sc)
        if rows is not None:
            for j, f in enumerate(files):
                n, c = float(sc.nll_sum[j]), int(sc.count[j])
                rows.append({'file': f, 'speaker': int(spk[j]), 'samples': c, 'bits': bits(n, c), 'accuracy': int(sc.hits[j]) / c})
        if prior is not None:
            frames = sc.frames.tolist()
            Tz = sc.codes.shape[1]
            Tp = -(-Tz // 64) * 64                     # the prior's condition frames hold 64 code steps
            codes = sc.codes.new_zeros((len(files), Tp)).int()
            codes[:, :Tz] = sc.codes
            prior_totals.add(prior.evaluate(codes.contiguous(), spk_d, lengths=frames, weights=weights))
    return totals
