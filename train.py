#!/usr/bin/env python3
"""train.py -- same command line as the reference's train.py:12-37, running on MI355X.

    python3 train.py -dataset VCTK -length 6656 -batch 8 -step 100000 -save saved_model/weights
    python3 -m torch.distributed.run --nproc-per-node 8 train.py ...      # data parallel (RCCL)

Differences from the reference: `-dataset synthetic` needs no files; checkpoints are torch
files `<save>-<global_step>.pt` (the reference writes TF checkpoints `<save>-<global_step>`);
TF summaries are replaced by the console line.

`-eval_list FILE -eval_interval N [-eval_batches M]`: every N steps rank 0 scores the same M held-out batches with the EMA
weights (VQVAE.evaluate, forward only: the first `-length` samples of the first M x batch files of the list that are long
enough, so the curve is comparable from step to step), adds `[eval bits ...]` to the console line and an `eval` object to
that step's line of summaries.jsonl.  The list is in the format of the `<name>_train.txt` lists, read under `-data_root` as
`-eval_dataset` (default: `-dataset`; VCTK when that is synthetic).

`-audio_interval N [-audio_count 2] [-audio_dir DIR]` (needs `-eval_list`): every N steps rank 0 reconstructs the first
`-audio_count` rows of the first held-out batch with the EMA weights (VQVAE.reconstruct: teacher forced, mode sample, seed 0,
default settings) and writes `DIR/<step>_<k>_teacher.wav` (float32, 16 kHz; DIR defaults to `audio/` next to `-save`), once
per run also `DIR/<k>_original.wav`; the console line of that step gains `[audio <count>]`.  0 (the default) = never.

`-clip_norm C`: gradients are clipped to the global norm C (tf.clip_by_global_norm; norm and scale stay on the device).
`-grad_norm`: the norms are measured and logged, nothing is clipped.  Either adds `[gnorm ...]` to the console line and
`grad_norm`, `grad_clip_scale` and a per-variable `grad_norms` object to summaries.jsonl, on logged steps.

`-time_jitter P`: in training, every latent frame the decoder reads is replaced with probability P by its left or right
neighbour of the same utterance (arXiv 1901.08810; overrides `time_jitter` of the parameters file, 0 = off).  Adds
`[jitter ...]` to the console line and `jitter_moved` (the share of frames that moved in that step) to summaries.jsonl, on
logged steps.

`-codebook_ema G`: the VQ codebook is trained as the moving average (decay G, e.g. 0.99) of the encoder outputs assigned to each
code (sonnet's VectorQuantizerEMA) instead of by Adam on the codebook loss; `-codebook_restart T` (needs `-codebook_ema`): a
code whose moving count falls below T (e.g. 0.05) is restarted on an encoder output of the batch.  They override `codebook_ema`
/ `codebook_restart` of the parameters file (0 = off).  Adds `[codebook used U/K restarted R]` to the console line and
`codebook_used`, `codebook_restarted` to summaries.jsonl, on logged steps.

`-accumulate N`: every optimiser step sums the gradients of N batches of `-batch` rows (VQVAE.accumulate: one Adam + EMA step on
a batch of N x `-batch` rows, up to fp32 summation order; data parallel: one gradient exchange per step).  `-step` stays the
number of optimiser steps; logging, evaluation, audio and saving happen on a step's last batch, and the logged losses are that
batch's.  Adds `[accum N]` to the console line and `accumulate` to summaries.jsonl.  Not together with `-codebook_ema`.
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


def display_time(t, second):
    """Console suffix in the reference's format (utils.py:49-67): batch time, then the ETA as seconds, `Nm S.SSSs` above
    one minute, `Nh Nm S.SSSs` above one hour of minutes (the reference's thresholds are strict: 60 s prints as seconds)."""
    eta = '%.3fs' % second
    if second > 60:
        minute, second = divmod(second, 60)
        eta = '%dm %.3fs' % (minute, second)
        if minute > 60:
            eta = '%dh %dm %.3fs' % (minute // 60, minute % 60, second)
    return ' [BATCH %.3fs / ETA %s]     ' % (t, eta)


def main():
    parser = ArgumentParser()
    parser.add_argument('-dataset', default='VCTK', type=str, help='VCTK or LibriSpeech or Aishell (or synthetic)', metavar='DATASET')
    parser.add_argument('-length', default=6656, type=int, dest='max_len', metavar='int', help='number of samples one audio will contain')
    parser.add_argument('-step', default=1000000, type=int, dest='num_steps', metavar='int', help='number of steps to train')
    parser.add_argument('-batch', default=8, type=int, dest='batch_size', metavar='int', help='batch size (per GPU)')
    parser.add_argument('-interval', default=200, type=int, dest='interval', metavar='int', help='log every interval step')
    parser.add_argument('-restore', dest='restore_path', metavar='string', help='path to restore weights')
    parser.add_argument('-save', default='saved_model/weights', dest='save_path', metavar='string', help='path to save weights')
    parser.add_argument('-params', default='model_parameters.json', dest='parameter_path', metavar='str', help='path to parameters file')
    parser.add_argument('-eval_list', dest='eval_list', metavar='string', help='held-out file list scored during training')
    parser.add_argument('-eval_interval', default=0, type=int, dest='eval_interval', metavar='int', help='score the list every N steps (0 = never)')
    parser.add_argument('-eval_batches', default=4, type=int, dest='eval_batches', metavar='int', help='held-out batches per evaluation')
    parser.add_argument('-eval_dataset', default=None, dest='eval_dataset', metavar='DATASET', help='dataset the list belongs to (default: -dataset)')
    parser.add_argument('-data_root', default='data/', dest='data_root', metavar='string', help='where the held-out wavs and *_speakers.txt are')
    parser.add_argument('-audio_interval', default=0, type=int, dest='audio_interval', metavar='int',
                        help='write teacher-forced reconstructions of held-out rows every N steps (0 = never; needs -eval_list)')
    parser.add_argument('-audio_count', default=2, type=int, dest='audio_count', metavar='int', help='held-out rows reconstructed each time')
    parser.add_argument('-audio_dir', default=None, dest='audio_dir', metavar='string', help='where the wavs go (default: audio/ next to -save)')
    parser.add_argument('-clip_norm', default=None, type=float, dest='clip_norm', metavar='float', help='clip gradients to this global norm (> 0)')
    parser.add_argument('-grad_norm', action='store_true', dest='grad_norm', help='log gradient norms without clipping')
    parser.add_argument('-time_jitter', default=None, type=float, dest='time_jitter', metavar='float',
                        help='probability in [0, 1] that a latent frame the decoder reads is its neighbour (0 = off)')
    parser.add_argument('-codebook_ema', default=None, type=float, dest='codebook_ema', metavar='float',
                        help='decay in (0, 1) of the codebook\'s moving averages (0 = off: Adam trains the codebook)')
    parser.add_argument('-codebook_restart', default=None, type=float, dest='codebook_restart', metavar='float',
                        help='restart a code whose moving count falls below this threshold in (0, 1) (0 = never; needs -codebook_ema)')
    parser.add_argument('-accumulate', default=1, type=int, dest='accumulate', metavar='int',
                        help='batches whose gradients are summed before each optimiser step (1 = off)')
    args = parser.parse_args()
    if args.accumulate < 1:
        parser.error('-accumulate must be an integer >= 1 (got %r)' % args.accumulate)
    if args.accumulate > 1 and args.codebook_ema:
        parser.error('-accumulate > 1 cannot be combined with -codebook_ema (the codebook\'s own update per batch has no rule yet)')
    if args.clip_norm is not None and not args.clip_norm > 0:
        parser.error('-clip_norm must be > 0 (got %r)' % args.clip_norm)
    if args.time_jitter is not None and not 0.0 <= args.time_jitter <= 1.0:
        parser.error('-time_jitter must be a probability in [0, 1] (got %r)' % args.time_jitter)
    if args.codebook_ema is not None and not 0.0 <= args.codebook_ema < 1.0:
        parser.error('-codebook_ema must be 0 (off) or a decay in (0, 1) (got %r)' % args.codebook_ema)
    if args.codebook_restart is not None and not 0.0 <= args.codebook_restart < 1.0:
        parser.error('-codebook_restart must be 0 (never) or a threshold in (0, 1) (got %r)' % args.codebook_restart)
    if args.codebook_restart and args.codebook_ema == 0.0:
        parser.error('-codebook_restart needs -codebook_ema (got -codebook_ema 0)')
    if args.eval_interval < 0 or args.eval_batches < 1:
        parser.error('-eval_interval must be >= 0 and -eval_batches >= 1')
    if args.audio_interval < 0 or args.audio_count < 1:
        parser.error('-audio_interval must be >= 0 and -audio_count >= 1')
    if args.audio_interval > 0 and args.eval_list is None:
        parser.error('-audio_interval needs -eval_list (the held-out rows it reconstructs)')
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

    pkg = importlib.import_module('vq-vae-wavenet_amd')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    D = pkg.data
    dargs = dict(batch_size=args.batch_size, max_len=args.max_len, device=dev)
    if args.dataset == 'VCTK':
        dataset = D.VCTK(relative_path='data/', rank=rank, world=world, **dargs)
    elif args.dataset == 'LibriSpeech':
        dataset = D.LibriSpeech(relative_path='data/', rank=rank, world=world, **dargs)
    elif args.dataset == 'Aishell':
        dataset = D.Aishell(relative_path='data/', rank=rank, world=world, **dargs)
    elif args.dataset == 'synthetic':
        dataset = D.Synthetic(seed=1234 + rank, **dargs)
    else:
        raise NotImplementedError('dataset %s not implemented' % args.dataset)

    dataset = D.Prefetcher(dataset, depth=3, device=dev)       # WAV reading / resampling off the step loop (dataset.py:75-84)
    parameters, wavenet_parameters = pkg.model.load_configs(args.parameter_path)
    if parameters['encoder'] not in ('64', 'Magenta', '2019'):                      # train.py:52-60
        raise NotImplementedError('encoder %s not implemented' % parameters['encoder'])
    if args.time_jitter is not None:
        parameters['time_jitter'] = args.time_jitter
    for key in ('codebook_ema', 'codebook_restart'):
        if getattr(args, key) is not None:
            parameters[key] = getattr(args, key)
    model = pkg.model.VQVAE(parameters, wavenet_parameters, dataset.num_speakers, device=dev, seed=0)
    if args.restore_path is not None:
        if args.restore_path.endswith(('.safetensors', '.npz')):      # TF variable names (checkpoint.py)
            pkg.checkpoint.load(model, args.restore_path)
        else:
            model.load_state_dict(torch.load(args.restore_path, map_location='cpu', weights_only=True))
    if world > 1:
        model.grad_sync = pkg.parallel.GradAllReduce(model.grad)
    model.defer_guard = os.environ.get('VQW_DEFER_GUARD', '1') != '0'     # the engine's range flag is read one step late (no host sync per step)
    model.clip_norm = args.clip_norm if args.clip_norm is not None else (float('inf') if args.grad_norm else None)
    model.accumulate = args.accumulate
    gs, lr = model.global_step, model.lr_at(model.global_step)
    if rank == 0:
        print('[restore] last global step: %d, learning rate: %.5f' % (gs, lr))
    save_dir, save_name = args.save_path.split('/')
    if rank == 0 and not os.path.isdir(save_dir):
        os.mkdir(save_dir)

    eval_set = None
    if args.eval_list is not None and rank == 0:      # the same crops at every evaluation, read once
        ratio = 320 if parameters['encoder'] == '2019' else 64
        if args.max_len % ratio:
            raise ValueError('-length must be a multiple of %d to score a held-out list' % ratio)
        held = D.HeldOutList(args.eval_dataset, args.eval_list, relative_path=args.data_root, ratio=ratio)
        if held.num_speakers != dataset.num_speakers:
            raise ValueError('-eval_list: %d speakers under %s, the model has %d' % (held.num_speakers, args.data_root, dataset.num_speakers))
        crops, _ = held.crops(args.max_len, limit=args.eval_batches * args.batch_size)
        if not crops:
            raise ValueError('-eval_list: no file of %s has %d samples' % (args.eval_list, args.max_len))
        eval_set = list(D.fixed_batches(crops, args.batch_size))
    audio_dir = None
    if eval_set is not None and args.audio_interval > 0:
        audio_dir = args.audio_dir or os.path.join(save_dir, 'audio')
        os.makedirs(audio_dir, exist_ok=True)
        _, ax, aspk, _ = eval_set[0]
        ax, aspk = ax[:args.audio_count].contiguous(), aspk[:args.audio_count].contiguous()
        from scipy.io import wavfile
        for k in range(ax.shape[0]):
            wavfile.write(os.path.join(audio_dir, '%d_original.wav' % k), 16000, ax[k].cpu().numpy())

    for step in range(1, 1 + args.num_steps):
        t = time.time()
        for _ in range(args.accumulate):      # one window: global_step advances on its last batch, and only then is anything logged
            x, spk = dataset.next()
            ws = model.train_step(x, spk)
        gs = model.global_step
        eval_now = eval_set is not None and gs % args.eval_interval == 0
        audio_now = audio_dir is not None and gs % args.audio_interval == 0
        if rank == 0 and (gs % args.interval == 0 or step == args.num_steps or eval_now or audio_now):
            loss, rl, vq, commit = model.losses(ws)          # synchronises: only every `interval` steps
            extra = {}
            if model.time_jitter > 0:             # from the step's source frames; read here, on logged steps only
                extra['jitter_moved'] = model.jitter_moved(ws)
            if model.codebook_ema > 0:            # counts the update kernel left on the device; read here, on logged steps only
                info = model.codebook_info()
                extra.update(codebook_used=info['used'], codebook_restarted=info['restarted'])
            if eval_now:
                extra['eval'] = pkg.scoring.score_batches(model, eval_set, dev, weights='ema').report(
                    'sample', latent_dim=model.D if model.use_vq else 0)
            if audio_now:
                rec, _ = model.reconstruct(ax.to(dev), aspk.to(dev), weights='ema', mode='sample', seed=0)
                for k, row in enumerate(rec.cpu().numpy()):
                    wavfile.write(os.path.join(audio_dir, '%d_%d_teacher.wav' % (gs, k)), 16000, row)
            t = time.time() - t
            progress = '\r[step %d] %.2f' % (gs, step / args.num_steps * 100) + '%'
            msg = ' [recons %.5f] [vq %.5f] [lr %.5f]' % (rl, vq, model.lr_at(gs - 1))
            if model.clip_norm is not None:       # measured on the device by the step itself; read here, on logged steps only
                gn = model.grad_norms()
                extra.update(grad_norm=gn['global'], grad_clip_scale=gn['scale'], grad_norms=gn['segments'])
                msg += ' [gnorm %.4f]' % gn['global']
            if 'jitter_moved' in extra:
                msg += ' [jitter %.3f]' % extra['jitter_moved']
            if 'codebook_used' in extra:
                msg += ' [codebook used %d/%d restarted %d]' % (extra['codebook_used'], model.Kc, extra['codebook_restarted'])
            if eval_now:
                msg += ' [eval bits %.5f]' % extra['eval']['bits_per_sample']
            if audio_now:
                msg += ' [audio %d]' % ax.shape[0]
            if args.accumulate > 1:               # (the losses are those of the window's last batch)
                extra['accumulate'] = args.accumulate
                msg += ' [accum %d]' % args.accumulate
            print(progress + msg + display_time(t, (args.num_steps - step) * t), end='', flush=True)
            # the reference writes its merged summaries to a TensorBoard event file here (train.py:104-109); without
            # TensorFlow the same tags go to <save_dir>/summaries.jsonl, one line per logged step
            with open(os.path.join(save_dir, 'summaries.jsonl'), 'a') as f:
                f.write(json.dumps({'global_step': gs, 'learning_rate': model.lr_at(gs - 1), **model.summaries(ws), **extra}) + '\n')
    if rank == 0:
        torch.cuda.synchronize()
        path = '%s-%d.pt' % (args.save_path, model.global_step)
        torch.save(model.state_dict(), path)
        # the same state under the reference's TF variable names (+ EMA shadows, Adam slots): checkpoint.py
        pkg.checkpoint.save(model, '%s-%d.safetensors' % (args.save_path, model.global_step))
        with open(os.path.join(save_dir, save_name + '.json'), 'w') as f:
            json.dump({'model': parameters, 'wavenet': wavenet_parameters, 'num_speakers': dataset.num_speakers}, f)
        print('\nsaved', path)
    dataset.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
