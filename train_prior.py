#!/usr/bin/env python3
"""train_prior.py -- fit a WaveNet prior over the VQ codes of a trained VQ-VAE (prior.py), same flag style as train.py.

    python3 train_prior.py -restore saved_model/weights-110640.pt -dataset VCTK -length 1024 -batch 16 \\
        -step 100000 -save saved_prior/prior

Every step encodes fresh audio crops of `length` x 64 samples with the VQ-VAE's EMA weights (encoder + VQ: one code per 64
samples) and runs one prior training step on those codes and their speakers.  Checkpoints are `<save>-<step>.pt` (+ a
`<name>.json` with the prior's config and speaker count).  One GPU: data-parallel prior training is not supported.
`-clip_norm C` clips the gradients to the global norm C, `-grad_norm` only measures it; either adds `[gnorm ...]` to the
console line (as train.py).

`-whole_utterances [-min_frames N]`: rows are whole utterances, not crops from the middle of speech.  A file shorter than
`-length` frames is taken from its first sample, zero-padded, and the step is told its length (LatentPrior.train_step
lengths=): the loss is the mean over the real codes, so the prior sees utterances begin -- what sampling asks of it at step 0 --
and end.  Longer files give random windows of `-length` frames as before; files under N frames (default 16) are left out.  The
console line gains `[scored 0.73]`, the share of the logged step's positions that were scored.

`-eval_list FILE -eval_interval N [-eval_batches M]` (as train.py): every N steps the first M padded batches of the list are
scored with the EMA weights (LatentPrior.evaluate on the codes of the zero-padded audio, lengths = the rows' frames) and the
line gains `[eval bits/code ...]`.

`-accumulate N` (as train.py): every optimiser step sums the gradients of N batches (LatentPrior.accumulate); `-step` stays the
number of optimiser steps, and logging, evaluation and saving happen on a step's last batch, whose loss is the one logged.  With
`-whole_utterances` every batch contributes the mean over its own scored codes: a step is the average of N such means, not the
mean over all codes of the N batches.  The console line gains `[accum N]`.

Every logged step also appends one line to `summaries.jsonl` next to `-save`: `global_step`, `learning_rate`, `loss`, with
`-clip_norm` / `-grad_norm` `grad_norm`, with `-accumulate N > 1` `accumulate`.
"""
import importlib
import json
import os
import sys
import time
from argparse import ArgumentParser

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    parser = ArgumentParser()
    parser.add_argument('-restore', dest='vqvae_path', required=True, metavar='string', help='trained VQ-VAE weights (<save>-<step>.pt)')
    parser.add_argument('-prior_restore', dest='prior_path', metavar='string', help='prior weights to resume from')
    parser.add_argument('-dataset', default='VCTK', type=str, help='VCTK or LibriSpeech or Aishell (or synthetic)', metavar='DATASET')
    parser.add_argument('-length', default=1024, type=int, dest='frames', metavar='int', help='code frames per crop (x 64 audio samples)')
    parser.add_argument('-step', default=100000, type=int, dest='num_steps', metavar='int', help='number of steps to train')
    parser.add_argument('-batch', default=16, type=int, dest='batch_size', metavar='int', help='batch size')
    parser.add_argument('-interval', default=200, type=int, dest='interval', metavar='int', help='log every interval step')
    parser.add_argument('-save', default='saved_prior/prior', dest='save_path', metavar='string', help='path to save weights')
    parser.add_argument('-params', default='prior_parameters.json', dest='prior_params', metavar='str', help='prior parameters file')
    parser.add_argument('-vqvae_params', default='model_parameters.json', dest='vqvae_params', metavar='str',
                        help='the VQ-VAE\'s parameters file')
    parser.add_argument('-clip_norm', default=None, type=float, dest='clip_norm', metavar='float', help='clip gradients to this global norm (> 0)')
    parser.add_argument('-grad_norm', action='store_true', dest='grad_norm', help='log gradient norms without clipping')
    parser.add_argument('-whole_utterances', action='store_true', dest='whole', help='train on whole utterances: short files from their '
                        'first code, zero-padded, with a length-masked loss')
    parser.add_argument('-min_frames', default=None, type=int, dest='min_frames', metavar='int',
                        help='shortest admitted utterance in code frames (default 16; needs -whole_utterances)')
    parser.add_argument('-eval_list', dest='eval_list', metavar='string', help='held-out file list scored during training')
    parser.add_argument('-eval_interval', default=0, type=int, dest='eval_interval', metavar='int', help='score the list every N steps (0 = never)')
    parser.add_argument('-eval_batches', default=4, type=int, dest='eval_batches', metavar='int', help='held-out batches per evaluation')
    parser.add_argument('-eval_dataset', default=None, dest='eval_dataset', metavar='DATASET', help='dataset the list belongs to (default: -dataset)')
    parser.add_argument('-data_root', default='data/', dest='data_root', metavar='string', help='where the held-out wavs and *_speakers.txt are')
    parser.add_argument('-accumulate', default=1, type=int, dest='accumulate', metavar='int',
                        help='batches whose gradients are summed before each optimiser step (1 = off)')
    args = parser.parse_args()
    if args.accumulate < 1:
        parser.error('-accumulate must be an integer >= 1 (got %r)' % args.accumulate)
    if args.clip_norm is not None and not args.clip_norm > 0:
        parser.error('-clip_norm must be > 0 (got %r)' % args.clip_norm)
    if args.min_frames is not None and not args.whole:
        parser.error('-min_frames needs -whole_utterances')
    if args.whole:
        args.min_frames = 16 if args.min_frames is None else args.min_frames
        if not 1 <= args.min_frames <= args.frames:
            parser.error('-min_frames must be in 1..-length = %d (got %d)' % (args.frames, args.min_frames))
    if args.eval_interval < 0 or args.eval_batches < 1:
        parser.error('-eval_interval must be >= 0 and -eval_batches >= 1')
    if args.eval_interval > 0 and args.eval_list is None:
        parser.error('-eval_interval needs -eval_list')
    if args.eval_list is not None:
        if args.eval_interval == 0:
            parser.error('-eval_list needs -eval_interval N (N > 0): the list would never be scored')
        if not os.path.isfile(args.eval_list):
            parser.error('-eval_list: no such file: %s' % args.eval_list)
        args.eval_dataset = args.eval_dataset or ('VCTK' if args.dataset == 'synthetic' else args.dataset)
        if args.eval_dataset not in ('VCTK', 'LibriSpeech', 'Aishell'):
            parser.error('-eval_dataset must be VCTK, LibriSpeech or Aishell')
    elif args.eval_dataset is not None:
        parser.error('-eval_dataset needs -eval_list')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise NotImplementedError('train_prior.py runs on one GPU (multi-GPU prior training is not supported)')

    pkg = importlib.import_module('vq-vae-wavenet_amd')
    vq_cfg, vq_wavenet = pkg.model.load_configs(args.vqvae_params)
    prior_cfg = pkg.prior.load_prior_config(args.prior_params, vq_cfg)     # k and the encoder ratio are checked here
    if args.frames % pkg.prior.CODES_PER_FRAME:
        raise ValueError('-length must be a multiple of %d code frames' % pkg.prior.CODES_PER_FRAME)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)

    D = pkg.data
    T_audio = args.frames * 64
    dargs = dict(batch_size=args.batch_size, max_len=T_audio, device=dev)
    if args.whole:
        dargs.update(whole=True, unit=64, min_len=args.min_frames * 64)
    if args.dataset == 'VCTK':
        dataset = D.VCTK(relative_path='data/', **dargs)
    elif args.dataset == 'LibriSpeech':
        dataset = D.LibriSpeech(relative_path='data/', **dargs)
    elif args.dataset == 'Aishell':
        dataset = D.Aishell(relative_path='data/', **dargs)
    elif args.dataset == 'synthetic':
        dataset = D.Synthetic(seed=1234, **dargs)
    else:
        raise NotImplementedError('dataset %s not implemented' % args.dataset)
    dataset = D.Prefetcher(dataset, depth=3, device=dev)

    vqvae = pkg.model.VQVAE(vq_cfg, vq_wavenet, dataset.num_speakers, device=dev, seed=0)
    vqvae.load_state_dict(torch.load(args.vqvae_path, map_location='cpu', weights_only=True))
    vqvae.use_ema_weights()                    # codes of the EMA weights, as generate.py decodes with
    prior = pkg.prior.LatentPrior(prior_cfg, dataset.num_speakers, device=dev, seed=0, n_codes=vqvae.Kc)
    if args.prior_path is not None:
        prior.load_state_dict(torch.load(args.prior_path, map_location='cpu', weights_only=True))
    prior.defer_guard = os.environ.get('VQW_DEFER_GUARD', '1') != '0'
    prior.clip_norm = args.clip_norm if args.clip_norm is not None else (float('inf') if args.grad_norm else None)
    prior.accumulate = args.accumulate
    gs = prior.global_step
    print('[restore] last global step: %d, learning rate: %.5f' % (gs, prior.lr_at(gs)))
    save_dir, save_name = os.path.split(args.save_path)
    if save_dir and not os.path.isdir(save_dir):
        os.makedirs(save_dir)

    eval_set = None
    if args.eval_list is not None:      # the same rows at every evaluation: read and encoded once (the VQ-VAE does not change)
        held = D.HeldOutList(args.eval_dataset, args.eval_list, relative_path=args.data_root, ratio=64)
        if held.num_speakers != dataset.num_speakers:
            raise ValueError('-eval_list: %d speakers under %s, the model has %d' % (held.num_speakers, args.data_root, dataset.num_speakers))
        utts, _ = held.utterances()
        if not utts:
            raise ValueError('-eval_list: no file of %s holds a code frame' % args.eval_list)
        eval_set = []
        for _, ex, espk, lengths in D.padded_batches(utts, args.batch_size, multiple=64 * pkg.prior.CODES_PER_FRAME):
            if len(eval_set) == args.eval_batches:
                break
            espk = espk.to(dev)
            eval_set.append((vqvae.encode_codes(ex.to(dev), espk), espk, [n // 64 for n in lengths]))

    for step in range(1, 1 + args.num_steps):
        t = time.time()
        for _ in range(args.accumulate):      # one window: global_step advances on its last batch, and only then is anything logged
            if args.whole:
                x, spk, lengths = dataset.next()
                frames = lengths // 64                   # CPU int32 [B]: the rows' code counts
            else:
                (x, spk), frames = dataset.next(), None
            codes = vqvae.encode_codes(x, spk)       # [B][frames] int32
            prior.train_step(codes, spk) if frames is None else prior.train_step(codes, spk, lengths=frames)
        gs = prior.global_step
        eval_now = eval_set is not None and gs % args.eval_interval == 0
        if gs % args.interval == 0 or step == args.num_steps or eval_now:
            ws = prior._workspace(args.batch_size, args.frames)
            loss = prior.losses(ws)[0]             # synchronises: only every `interval` steps
            t = time.time() - t
            summary = {'global_step': gs, 'learning_rate': prior.lr_at(gs - 1), 'loss': loss}
            gnorm = ''
            if prior.clip_norm is not None:
                summary['grad_norm'] = prior.grad_norms()['global']
                gnorm = ' [gnorm %.4f]' % summary['grad_norm']
            if args.accumulate > 1:               # (the loss is that of the window's last batch)
                summary['accumulate'] = args.accumulate
                gnorm += ' [accum %d]' % args.accumulate
            if frames is not None:
                gnorm += ' [scored %.2f]' % (int(frames.sum()) / (args.batch_size * args.frames))
            if eval_now:
                totals = pkg.scoring.Totals()
                for ecodes, espk, eframes in eval_set:
                    totals.add(prior.evaluate(ecodes, espk, lengths=eframes, weights='ema'))
                gnorm += ' [eval bits/code %.5f]' % totals.report('code')['bits_per_code']
            print('\r[step %d] %.2f%% [prior %.5f] [lr %.5f]%s [BATCH %.3fs]     '
                  % (gs, step / args.num_steps * 100, loss, prior.lr_at(gs - 1), gnorm, t), end='', flush=True)
            with open(os.path.join(save_dir or '.', 'summaries.jsonl'), 'a') as f:
                f.write(json.dumps(summary) + '\n')
    torch.cuda.synchronize()
    path = '%s-%d.pt' % (args.save_path, prior.global_step)
    torch.save(prior.state_dict(), path)
    with open(os.path.join(save_dir or '.', save_name + '.json'), 'w') as f:
        json.dump({'prior': prior_cfg, 'num_speakers': dataset.num_speakers}, f)
    print('\nsaved', path)
    dataset.close()


if __name__ == '__main__':
    main()
