"""Held-out scoring, host side: the result of VQVAE.evaluate / LatentPrior.evaluate and the numbers derived from it.
Pure Python over small host arrays (no GPU needed):

    bits(nll_sum, count)   = nll_sum / (count * ln 2)            bits per scored position
    perplexity(counts)     = exp(-sum p ln p),  p = counts / counts.sum(), zeros ignored, float64
    used(counts)           = number of codes that occur at all
"""
import math

import numpy as np


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
