"""Float64 restatement of the length-masked prior step (LatentPrior.train_step lengths=) and of the ranged loss
kernel (vqw_softmax_xent_ranged), for tests/test_masked_loss_cpu.py and tests/test_masked_loss_gpu.py.

The network is tests/test_prior_gpu.py::ref_logits' -- oracle.ref_ops over one_hot(shift_right(codes)), the residual stack and
head with the speaker as the only condition -- written for ANY number of steps: the condition, the same in every frame of 64
steps, is tiled over ceil(T / 64) frames and handed over per step, which is what the nearest upsampling of add_condition
makes of it.  The loss of rows of lengths len_b is
    sum_b sum_{t < len_b} CE(logits[b][t], codes[b][t]) / sum_b len_b
and every gradient comes from autograd.  It is evaluated two ways: on the padded batch with a mask (padded_loss), and as the
sum over rows of the network run on codes[b, :len_b] ALONE (rowwise_loss), which cannot know what the padding holds."""
import numpy as np
import torch
import torch.nn.functional as Fn

import pointwise_ref as PR
from oracle import ref_model as M
from oracle import ref_ops as R

FRAME = 64


def prior_logits(codes, spk, P, cfg):
    """codes int64 [B][T] (any T >= 1), spk int64 [B] -> logits [B][T][k] in the parameters' dtype."""
    k = cfg['quantization_channels']
    B, T = codes.shape
    x = R.shift_right(Fn.one_hot(codes, k).to(P['prior/preprocess/kernel'].dtype))
    net = R.conv1d_v2(x, P['prior/preprocess/kernel'], P['prior/preprocess/bias'])
    skip = R.conv1d_v2(net, P['prior/skip/kernel'], P['prior/skip/bias'])
    frames = -(-T // FRAME)
    cond = P['prior/speaker_embedding'][spk].unsqueeze(1).repeat(1, frames, 1)            # [B][frames][Cs]
    cond = cond.repeat_interleave(FRAME, dim=1)[:, :T]                                    # one per step: frame t // 64
    for i, d in enumerate(cfg['dilation_rates']):
        s = M.layer_scope(i, cfg['num_cycle_layers']).replace('decoder/', 'prior/')
        p = {n[len(s) + 1:]: v for n, v in P.items() if n.startswith(s + '/')}
        s_out, r_out = R.residual_stack(net, p, cfg['dilation_filters'], d, cond)
        skip, net = skip + s_out, net + r_out
    h = R.conv1d_v2(torch.relu(skip), P['prior/postprocess1/kernel'], P['prior/postprocess1/bias'])
    h = R.add_condition(h, cond, P['prior/postprocess1/local_condition/kernel'])
    return R.conv1d_v2(torch.relu(h), P['prior/postprocess2/kernel'], P['prior/postprocess2/bias'])


def padded_loss(codes, spk, lengths, P, cfg):
    """The masked mean on the padded batch."""
    B, T = codes.shape
    ce = Fn.cross_entropy(prior_logits(codes, spk, P, cfg).permute(0, 2, 1), codes, reduction='none')      # [B][T]
    mask = torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]
    return (ce * mask).sum() / int(sum(lengths))


def rowwise_loss(codes, spk, lengths, P, cfg):
    """The same mean from every row run alone on its own codes[b, :len_b]."""
    total = 0.0
    for b, n in enumerate(lengths):
        row = codes[b:b + 1, :n]
        total = total + Fn.cross_entropy(prior_logits(row, spk[b:b + 1], P, cfg).permute(0, 2, 1), row, reduction='sum')
    return total / int(sum(lengths))


def loss_and_grads(fn, codes, spk, lengths, P, cfg):
    """-> (loss float, {name: gradient}) of fn = padded_loss or rowwise_loss; a variable no loss reaches gets zeros."""
    for p in P.values():
        p.requires_grad_(True)
        p.grad = None
    loss = fn(codes, spk, lengths, P, cfg)
    loss.backward()
    grads = {n: p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p) for n, p in P.items()}
    for p in P.values():
        p.requires_grad_(False)
    return float(loss.detach()), grads


def masked_step(codes, spk, lengths, P, cfg, state):
    """One masked training step of the restatement: loss, gradients, then Adam + EMA on P / state in place."""
    loss, grads = loss_and_grads(padded_loss, codes, spk, lengths, P, cfg)
    M.adam_ema_step(P, grads, state, M.lr_at(cfg['learning_rate_schedule'], state['t']))
    return loss, grads


def random_params(named, seed, dtype=torch.float64):
    """Every variable of `named` (name -> tensor: LatentPrior.named_parameters()) random, as tests/test_prior_gpu.py::random_params."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, v in named.items():
        scale = float(v.abs().max()) if float(v.abs().max()) > 0 else 0.1
        out[n] = ((torch.rand(v.shape, generator=g) * 2 - 1) * scale).float().to(dtype)
    return out


# ---------------------------------------------------------------------------------------------------- the ranged loss kernel
def range_mask(B, T, t_begin=None, t_end=None):
    """bool [B][T]: clamp(t_begin[b], 0, T) <= t < clamp(t_end[b], 0, T); None: 0 / T."""
    tb = np.zeros(B, np.int64) if t_begin is None else np.clip(np.asarray(t_begin, np.int64), 0, T)
    te = np.full(B, T, np.int64) if t_end is None else np.clip(np.asarray(t_end, np.int64), 0, T)
    t = np.arange(T)[None, :]
    return (t >= tb[:, None]) & (t < te[:, None])


def xent_ranged_ref(logits, labels, grad_scale=1.0, t_begin=None, t_end=None):
    """float64 vqw_softmax_xent_ranged over pointwise_ref.softmax_ref: mask [B][T], p and d [B][Q][T] (0 where not scored),
    loss [B][T] (0 where not scored), and the whole-row softmax_ref as `full` (the bars are formulas in it).  Logits outside
    the ranges may be anything: they are replaced by zeros before the reference looks at them."""
    B, Q, T = logits.shape
    mask = range_mask(B, T, t_begin, t_end)
    x = np.where(mask[:, None, :], np.asarray(logits, np.float64), 0.0)
    full = PR.softmax_ref(x, labels)
    m3 = mask[:, None, :]
    return dict(mask=mask, x=x, full=full, p=np.where(m3, full['p'], 0.0),
                d=np.where(m3, (full['p'] - PR.onehot(labels, Q)) * grad_scale, 0.0), loss=np.where(mask, full['loss'], 0.0))


def xent_ranged_bars(ref, labels, grad_scale):
    """pointwise_ref.softmax_bars of the scored subset: p / dlogits elementwise (0 where not scored: an exact +0.0 is asked
    for), loss_sum the sum of the scored positions' bars + the any-order bound over them."""
    bars = PR.softmax_bars(ref['x'], labels, ref['full'], grad_scale)
    mask = ref['mask']
    m3 = mask[:, None, :]
    n = int(mask.sum())
    loss_sum = bars['loss'][mask].sum() + n * PR.U * (abs(PR.SOFTMAX_LOSS0) + np.abs(ref['full']['loss'][mask]).sum())
    return dict(p=np.where(m3, bars['p'], 0.0), dlogits=np.where(m3, bars['dlogits'], 0.0), loss_sum=float(loss_sum))
