#!/usr/bin/env python3
"""evaluate.py -- score a checkpoint on held-out audio (no counterpart in the reference, which only logs the training loss).

    python3 evaluate.py -restore saved_model/weights-110640.pt -dataset VCTK -list data/vctk_heldout.txt \\
        [-length 0] [-batch 8] [-weights ema] [-params model_parameters.json] [-out eval_110640.json] [-per_utterance] \\
        [-data_root data/] [-prior saved_prior/prior-100000.pt -prior_params prior_parameters.json]

`-list` is a file in the format of the `<name>_train.txt` lists (one path per line, relative to the dataset's wav directory
under `-data_root`, where the dataset's `*_speakers.txt` is looked up too).  `-length 0` scores WHOLE utterances: each is
trimmed to a multiple of the encoder's ratio, files are sorted by length, batched, zero-padded to the batch's longest row
rounded up to a multiple of 256 and scored with their lengths (VQVAE.evaluate: forward only, teacher forced).  `-length N`
scores the first N samples of every file that is long enough; shorter files are skipped and counted.

Prints ONE JSON line (and writes it to `-out`): bits per sample, mean NLL and entropy in nats and top-1 accuracy over the
scored samples; the vq_loss mean, the codes used of k and the code perplexity; utterances, samples, files skipped, the
weights used and the checkpoint's step; with `-per_utterance` a list of {file, speaker, samples, bits, accuracy}; with
`-prior` the same utterances' codes scored by the latent prior (bits per code, entropy, accuracy).  Under torchrun the
files are sharded over the ranks and rank 0 merges the integer counts and float64 sums.
"""
import importlib
import json
import math
import os
import re
import sys
from argparse import ArgumentParser

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    parser = ArgumentParser()
    parser.add_argument('-restore', dest='restore_path', help='path to weights (train.py\'s <save>-<step>.pt)')
    parser.add_argument('-dataset', default='VCTK', type=str, help='VCTK or LibriSpeech or Aishell')
    parser.add_argument('-list', dest='list_path', help='held-out file list (format of the <name>_train.txt lists)')
    parser.add_argument('-data_root', default='data/', dest='data_root', help='where the wav directory and *_speakers.txt are')
    parser.add_argument('-length', default=0, type=int, dest='length', help='0: whole utterances; N: the first N samples of every file')
    parser.add_argument('-batch', default=8, type=int, dest='batch_size', help='utterances per batch')
    parser.add_argument('-weights', default='ema', dest='weights', help='ema (what generate.py uses) or live')
    parser.add_argument('-params', default='model_parameters.json', dest='parameter_path', help='path to parameters file')
    parser.add_argument('-out', dest='out_path', help='write the JSON report here too')
    parser.add_argument('-per_utterance', action='store_true', help='add one entry per utterance to the report')
    parser.add_argument('-prior', dest='prior_path', help='latent prior weights: also score the utterances\' codes')
    parser.add_argument('-prior_params', default=None, dest='prior_params', help='the prior\'s parameters file (with -prior)')
    args = parser.parse_args()
    if args.restore_path is None or args.list_path is None:
        parser.error('-restore and -list are required')
    if args.dataset not in ('VCTK', 'LibriSpeech', 'Aishell'):
        parser.error('-dataset must be VCTK, LibriSpeech or Aishell (a held-out list names files)')
    if args.weights not in ('ema', 'live'):
        parser.error('-weights must be ema or live')
    if args.length < 0 or args.length % 64:
        parser.error('-length must be 0 (whole utterances) or a positive multiple of 64')
    if args.batch_size < 1:
        parser.error('-batch must be at least 1')
    if args.prior_params is not None and args.prior_path is None:
        parser.error('-prior_params needs -prior')
    for path, what in ((args.restore_path, '-restore'), (args.list_path, '-list'), (args.parameter_path, '-params'),
                       (args.prior_path, '-prior')):
        if path is not None and not os.path.isfile(path):
            parser.error('%s: no such file: %s' % (what, path))

    import torch
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    S = pkg.scoring
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    parameters, wavenet_parameters = pkg.model.load_configs(args.parameter_path)
    ratio = 320 if parameters.get('encoder', '64') == '2019' else 64
    if args.length % ratio:
        parser.error('-length must be a multiple of the encoder\'s ratio %d' % ratio)
    held = pkg.data.HeldOutList(args.dataset, args.list_path, relative_path=args.data_root, ratio=ratio)
    meta = re.sub(r'-\d+\.(pt|safetensors|npz)$', '', args.restore_path) + '.json'      # written by train.py next to the weights
    if os.path.isfile(meta):
        with open(meta) as f:
            n_ckpt = json.load(f)['num_speakers']
        if n_ckpt != held.num_speakers:
            parser.error('the checkpoint was trained with %d speakers, the dataset under %s has %d'
                         % (n_ckpt, args.data_root, held.num_speakers))
    model = pkg.model.VQVAE(parameters, wavenet_parameters, held.num_speakers, device=dev, seed=0)
    if args.restore_path.endswith(('.safetensors', '.npz')):
        pkg.checkpoint.load(model, args.restore_path)
    else:
        model.load_state_dict(torch.load(args.restore_path, map_location='cpu', weights_only=True))
    prior = prior_totals = None
    if args.prior_path is not None:
        prior_cfg = pkg.prior.load_prior_config(args.prior_params or 'prior_parameters.json', parameters)
        prior = pkg.prior.LatentPrior(prior_cfg, held.num_speakers, device=dev, seed=0, n_codes=model.Kc)
        prior.load_state_dict(torch.load(args.prior_path, map_location='cpu', weights_only=True))
        prior_totals = S.Totals()

    files = held.files[rank::world]
    if args.length:
        utts, skipped = held.crops(args.length, files=files)
        batches = pkg.data.fixed_batches(utts, args.batch_size)
    else:
        utts, skipped = held.utterances(files=files)
        lcm = 256 * ratio // math.gcd(256, ratio)
        batches = pkg.data.padded_batches(utts, args.batch_size, multiple=lcm)
    rows = [] if args.per_utterance else None
    totals = S.score_batches(model, batches, dev, weights=args.weights, rows=rows, prior=prior, prior_totals=prior_totals)
    if world > 1:          # the one small collective: rank 0 adds what the ranks counted, in rank order
        mine = (totals, prior_totals, rows, skipped)
        parts = [None] * world if rank == 0 else None
        dist.gather_object(mine, parts, dst=0)
        if rank == 0:
            for t, pt, r, sk in parts[1:]:
                totals.merge(t)
                skipped += sk
                if pt is not None:
                    prior_totals.merge(pt)
                if rows is not None:
                    rows += r
    if rank == 0:
        if totals.count == 0:
            raise SystemExit('evaluate.py: no file of %s could be scored (%d skipped)' % (args.list_path, skipped))
        report = totals.report('sample', latent_dim=model.D if model.use_vq else 0)
        report.update(utterances=totals.rows, skipped=skipped, weights=args.weights, step=model.global_step, length=args.length)
        if prior is not None:
            report['prior'] = dict(prior_totals.report('code'), step=prior.global_step)
        if rows is not None:
            report['per_utterance'] = rows
        line = json.dumps(report)
        if args.out_path:
            with open(args.out_path, 'w') as f:
                f.write(line + '\n')
        print(line)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
