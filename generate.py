#!/usr/bin/env python3
"""generate.py -- same command line as the reference's generate.py:14-32, running on MI355X.

    python3 generate.py -restore saved_model/weights-110640.pt -audio data/p225_001.wav \\
        -speakers p225 p226 p227 p228 -mode sample

Encodes the utterance once (encoder + VQ), then generates it back sample by sample with the
fast WaveNet generator conditioned on each requested speaker, using the EMA weights, and writes
`<dir>/<step>_<speaker>.wav` (float32, 16 kHz) plus `embedding_<step>.npy` /
`speaker_embedding_<step>.npy` like the reference (generate.py:94-117).  Under torchrun the
speakers are sharded over the GPUs (rows of the batch never interact).

With `-prior <prior.pt> -frames N` no input utterance is needed: N VQ codes per speaker are sampled from a latent prior
(prior.py, trained by train_prior.py), decoded through the VQ-VAE's codebook (condition_from_codes) and its fast WaveNet
generator, and written as `<dir>/<step>_<speaker>_prior.wav` (N x 64 samples) plus `prior_codes_<step>_<speaker>.npy`.

`-prior ... -count M` (M > 1) samples a corpus: M takes per speaker, every (speaker k, take m) pair one row i = k M + m of the wide
generators (generator.WidePriorGenerator for the codes, generator.WideGenerator for the audio), `-rows` (1..1024, default 256)
rows per batch; writes `<dir>/<step>_<speaker>_prior_<m>.wav` and `prior_codes_<step>_<speaker>_<m>.npy`.  With `-seed` row i
draws its code uniforms from child 0 of the seed sequence (seed, i) and its audio uniforms from child 1, so a row's codes and
audio do not depend on `-rows`.  Not with `-prompt_frames` (many continuations of one prompt: `-takes`).

`-temperature / -top_k / -top_p` temper and truncate the audio sampling, `-prior_temperature / -prior_top_k / -prior_top_p`
the code sampling of `-prior` (mode sample only; the same values for every speaker; the defaults are plain sampling).

Prompted generation (the generators are prefilled from a prompt in one teacher-forced pass, FastGenerator.prefill /
PriorGenerator.prefill): `-prompt_samples N` with `-audio` continues the first N samples of the (trimmed) utterance for every
speaker; the wav holds them verbatim, then `length - N` generated samples.  `-prompt_frames N` with `-prior` and `-audio`
prefills the prior with the utterance's first N codes (encode_codes), samples `-frames` more, and decodes all N + frames codes
with the audio generator prefilled with the utterance's first N x 64 samples (which the wav holds verbatim); the codes file
holds all N + frames codes.  With `-seed`, uniforms are drawn for the generated samples / codes only.

`-takes M` (M > 1) with a prompt: M sampled continuations of the one prompt per speaker, on the wide generators prefilled from
the prompt (WideGenerator.prefill_prompt / WidePriorGenerator.prefill_codes); every (speaker k, take m) pair is one row i = k M + m, `-rows`
(1..1024, default 256) rows per batch.  With `-audio A -prompt_samples N` it writes `<dir>/<step>_<speaker>_take_<m>.wav` (the
prompt verbatim, then `length - N` generated samples); with `-prior P -audio A -prompt_frames N`,
`<dir>/<step>_<speaker>_prior_take_<m>.wav` and `prior_codes_<step>_<speaker>_take_<m>.npy` (`-frames` more codes per row).  With
`-seed` row i draws its code uniforms from row_uniforms' stage 0 and its audio uniforms from stage 1, so a take does not depend on
`-rows`.  Mode sample only (greedy takes would all be equal); not with `-audio_list`, `-count` above 1 or `-teacher_forced`.

`-audio_list FILE` (one wav path per line; `-data_root` for relative paths) converts every utterance of the list to every
speaker with the wide generator (generator.WideGenerator): every (utterance, speaker) pair is one row, `-rows` (1..1024, default
256) rows per batch, batches formed by length (generator.plan_rows); each utterance is encoded on its own as `-audio` does it, and
with `-seed` row i draws from a generator seeded with (seed, i), so a row's audio does not depend on `-rows`.  Writes
`<out_dir>/<step>_<basename>_<speaker>.wav`.  Not with `-audio`, `-prior`, a prompt or `-teacher_forced`.

`-teacher_forced` with `-audio` and `-speakers`: no autoregression.  The decoder is given the TRUE past of the utterance and
every sample is decided from its logits in one pass (VQVAE.reconstruct), by `-mode` with `-seed / -temperature / -top_k /
-top_p`: what the decoder predicts when nothing it predicted is fed back.  The utterance is trimmed to a multiple of the
encoder's ratio, zero-padded to a multiple of lcm(256, ratio) as evaluate.py pads, reconstructed with its true length and
trimmed back; `<dir>/<step>_<speaker>_teacher.wav` is written for every speaker.  Not with `-prior` or a prompt.
"""
import importlib
import json
import os
import sys
from argparse import ArgumentParser

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    parser = ArgumentParser()
    parser.add_argument('-restore', dest='restore_path', help='path to weights')
    parser.add_argument('-audio', dest='audio_path', help='path to audio')
    parser.add_argument('-speakers', nargs='+', dest='speakers', help='speaker id')
    parser.add_argument('-mode', default='sample', dest='mode', help='decode mode, sample or greedy')
    parser.add_argument('-params', default='model_parameters.json', dest='parameter_path', metavar='str', help='path to parameters file')
    parser.add_argument('-seed', default=None, type=int, help='seed of the sampling uniforms (reference: unseeded)')
    parser.add_argument('-prior', dest='prior_path', help='latent prior weights (train_prior.py): sample codes instead of encoding -audio')
    parser.add_argument('-frames', default=256, type=int, dest='frames', help='codes to sample per speaker with -prior (x 64 samples)')
    parser.add_argument('-prior_params', default='prior_parameters.json', dest='prior_params', metavar='str',
                        help='the prior\'s parameters file (with -prior)')
    parser.add_argument('-temperature', default=1.0, type=float, help='audio sampling: softmax temperature (> 0; 1 = off)')
    parser.add_argument('-top_k', default=0, type=int, help='audio sampling: keep the k most likely classes (0 = off)')
    parser.add_argument('-top_p', default=1.0, type=float,
                        help='audio sampling: keep the smallest most-likely set of mass >= p (nucleus, (0, 1]; 1 = off)')
    parser.add_argument('-prior_temperature', default=1.0, type=float, help='code sampling with -prior: softmax temperature')
    parser.add_argument('-prior_top_k', default=0, type=int, help='code sampling with -prior: top-k (0 = off)')
    parser.add_argument('-prior_top_p', default=1.0, type=float, help='code sampling with -prior: top-p (1 = off)')
    parser.add_argument('-prompt_samples', default=0, type=int,
                        help='with -audio: continue the first N samples of the utterance instead of generating from nothing')
    parser.add_argument('-prompt_frames', default=0, type=int,
                        help='with -prior and -audio: continue the first N codes (N x 64 samples) of the utterance')
    parser.add_argument('-teacher_forced', action='store_true',
                        help='with -audio: the decoder\'s one-pass reconstruction given the true past (<step>_<speaker>_teacher.wav)')
    parser.add_argument('-audio_list', dest='audio_list', help='text file of wav paths, one per line: convert every utterance '
                        'to every speaker with the wide generator (<step>_<basename>_<speaker>.wav)')
    parser.add_argument('-rows', default=256, type=int, help='with -audio_list: (utterance, speaker) rows per batch, 1..1024; '
                        'with -prior -count M: (speaker, take) rows per batch')
    parser.add_argument('-count', default=1, type=int, help='with -prior: takes per speaker; above 1 both stages run on the wide '
                        'generators (<step>_<speaker>_prior_<m>.wav, prior_codes_<step>_<speaker>_<m>.npy)')
    parser.add_argument('-takes', default=1, type=int, help='with a prompt (-prompt_samples / -prompt_frames): sampled continuations '
                        'per speaker; above 1 they run on the wide generators (<step>_<speaker>_take_<m>.wav)')
    parser.add_argument('-data_root', default='', help='with -audio_list: directory the list\'s relative paths start from')
    parser.add_argument('-out_dir', default=None, help='with -audio_list: where the wavs go (default: beside the weights)')
    args = parser.parse_args()
    if args.takes < 1:
        parser.error('-takes %d must be >= 1' % args.takes)
    if args.takes > 1:
        for flag, on in (('-audio_list', args.audio_list is not None), ('-count above 1', args.count > 1),
                         ('-teacher_forced', args.teacher_forced)):
            if on:
                parser.error('-takes %d continues one prompt several times: not with %s' % (args.takes, flag))
        if not args.prompt_samples and not args.prompt_frames:
            parser.error('-takes %d needs a prompt (-prompt_samples, or -prompt_frames with -prior); without one, -audio_list '
                         'converts many utterances and -prior -count samples many takes' % args.takes)
        if args.mode == 'greedy':
            parser.error('-takes %d with -mode greedy: all takes of a prompt would be equal' % args.takes)
        if not 1 <= args.rows <= 1024:
            parser.error('-rows %d must be in 1..1024' % args.rows)
    if args.audio_list is not None:
        return convert_list(args, parser)
    if args.count < 1:
        parser.error('-count %d must be >= 1' % args.count)
    if args.count > 1:
        if args.prior_path is None:
            parser.error('-count %d needs -prior: takes are sampled from the latent prior' % args.count)
        if args.prompt_frames:
            parser.error('-count %d with -prompt_frames: the wide generators have no prefill' % args.count)
        if not 1 <= args.rows <= 1024:
            parser.error('-rows %d must be in 1..1024' % args.rows)
    if args.teacher_forced and (args.prior_path is not None or args.prompt_samples or args.prompt_frames):
        parser.error('-teacher_forced reconstructs -audio in one pass: not with -prior, -prompt_samples or -prompt_frames')
    if args.teacher_forced and args.audio_path is None:
        parser.error('-teacher_forced needs -audio (the utterance whose true past the decoder is given)')
    if args.prior_path is None and args.audio_path is None:
        parser.error('-audio is required (or -prior to sample codes from a latent prior)')
    if args.prompt_samples < 0 or args.prompt_frames < 0:
        parser.error('-prompt_samples / -prompt_frames must be >= 0')
    if args.prompt_samples and args.prior_path is not None:
        parser.error('-prompt_samples applies to -audio conversion; with -prior use -prompt_frames')
    if args.prompt_frames and (args.prior_path is None or args.audio_path is None):
        parser.error('-prompt_frames needs -prior and -audio (the utterance whose codes and samples are the prompt)')
    if args.mode not in ('sample', 'greedy'):
        raise NotImplementedError('decode mode %s not implemented' % args.mode)

    pkg = importlib.import_module('vq-vae-wavenet_amd')
    try:        # every speaker gets the same settings; checked before anything is loaded or built
        for kind in ('', 'prior_'):
            pkg.generator.sampling_settings(1, args.mode, getattr(args, kind + 'temperature'), getattr(args, kind + 'top_k'),
                                            getattr(args, kind + 'top_p'))
    except ValueError as e:
        parser.error(str(e))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0')) % max(torch.cuda.device_count(), 1)   # no collective: ranks may share a GPU
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)

    gs = int(args.restore_path.split('-')[-1].split('.')[0])
    from scipy.io import wavfile
    if args.prior_path is not None:
        return generate_from_prior(args, pkg, gs, rank, world, dev, parser)
    if args.teacher_forced:
        return teacher_forced(args, pkg, gs, rank, world, dev, parser)
    if args.takes > 1:
        return prompted_takes(args, pkg, gs, rank, world, dev, parser)
    wav = read_wav(args.audio_path)
    length = len(wav)
    n_prompt = args.prompt_samples
    if n_prompt >= length:
        parser.error('-prompt_samples %d is not shorter than the trimmed utterance (%d samples): nothing to generate'
                     % (n_prompt, length))

    num_speakers, ids = speaker_ids(args, pkg)

    parameters, wavenet_parameters = pkg.model.load_configs(args.parameter_path)
    model = load_vqvae(args, pkg, parameters, wavenet_parameters, num_speakers, dev)
    save_path = args.restore_path.split('/weights')[0]
    if rank == 0:
        if model.use_vq:                      # generate.py:96-101
            np.save(save_path + '/embedding_%d.npy' % gs, model.P['embedding'].cpu().numpy())
        if model.spk_table:
            np.save(save_path + '/speaker_embedding_%d.npy' % gs, model.P['speaker_embedding'].cpu().numpy())

    mine = list(range(rank, len(ids), world))  # shard speakers over GPUs: no collective needed
    if mine:
        B = len(mine)
        x = torch.from_numpy(wav).to(dev).unsqueeze(0).contiguous()       # ONE utterance: encoder + VQ run once,
        spk = torch.tensor([ids[i] for i in mine], dtype=torch.int64, device=dev)
        enc = model.encode(x, spk)             # only the speaker rows differ (model.encoding, generate.py:40,92)
        out = np.zeros([B, length], dtype=np.float32)
        uniforms = None
        if args.mode == 'sample':      # one row of uniforms per requested speaker, whatever the sharding
            g = torch.Generator().manual_seed(args.seed) if args.seed is not None else None
            uniforms = torch.rand(len(ids), length - n_prompt, generator=g)[mine].contiguous().to(dev)
        out[:, :n_prompt] = wav[:n_prompt]
        for b0 in range(0, B, 12):             # 12 rows = three 4-row handles in one persistent launch at R=256
            rows = slice(b0, min(b0 + 12, B))
            gen = pkg.generator.FastGenerator(model, batch=rows.stop - rows.start)
            if n_prompt:
                gen.prefill(x[:, :n_prompt].expand(rows.stop - rows.start, n_prompt).contiguous(), enc[rows].contiguous(),
                            ratio=length // enc.shape[2])
            audio, _ = gen.generate(enc[rows].contiguous(), length - n_prompt, mode=args.mode, ratio=length // enc.shape[2],
                                    uniforms=None if uniforms is None else uniforms[rows].contiguous(),
                                    temperature=args.temperature, top_k=args.top_k, top_p=args.top_p)
            out[rows, n_prompt:] = audio.cpu().numpy()
            gen.close()
        for j, i in enumerate(mine):
            s = 'no_speaker' if args.speakers[i] == 'None' else args.speakers[i]
            wavfile.write(save_path + '/%d_%s.wav' % (gs, s), 16000, out[j])
            print('wrote', save_path + '/%d_%s.wav' % (gs, s))


def prompted_takes(args, pkg, gs, rank, world, dev, parser):
    """-audio -prompt_samples N -takes M: every (speaker k, take m) pair is row i = k M + m of the wide generator, cut into
    consecutive batches of at most -rows.  Each batch is prefilled from the utterance's first N samples (WideGenerator.prefill_prompt)
    and generates length - N more; with -seed row i draws from row_uniforms' stage 1 (the audio stage), so with the
    generator's batch independence a take depends neither on -rows nor on the sharding."""
    from scipy.io import wavfile
    wav = read_wav(args.audio_path)
    length, n_prompt, M = len(wav), args.prompt_samples, args.takes
    if n_prompt >= length:
        parser.error('-prompt_samples %d is not shorter than the trimmed utterance (%d samples): nothing to generate'
                     % (n_prompt, length))
    num_speakers, ids = speaker_ids(args, pkg)
    parameters, wavenet_parameters = pkg.model.load_configs(args.parameter_path)
    model = load_vqvae(args, pkg, parameters, wavenet_parameters, num_speakers, dev)
    save_path = args.restore_path.split('/weights')[0]
    all_rows = [(k, m) for k in range(len(ids)) for m in range(M)]            # speaker order, then take
    mine = list(range(rank, len(all_rows), world))                            # rows sharded over ranks: no collective
    if not mine:
        return
    x = torch.from_numpy(wav).to(dev).unsqueeze(0).contiguous()
    enc_all = model.encode(x, torch.tensor(ids, dtype=torch.int64, device=dev))      # one row per speaker
    ratio = length // enc_all.shape[2]
    n = length - n_prompt
    gens = {}
    for b0 in range(0, len(mine), args.rows):
        batch = mine[b0:b0 + args.rows]
        nb = len(batch)
        enc = enc_all[[all_rows[i][0] for i in batch]].contiguous()
        uniforms = torch.stack([row_uniforms(args.seed, i, n, stage=1) for i in batch]).to(dev)
        if nb not in gens:
            gens[nb] = pkg.generator.WideGenerator(model, batch=nb)
        gens[nb].prefill_prompt(x[:, :n_prompt].expand(nb, n_prompt).contiguous(), enc, ratio=ratio)
        audio, _ = gens[nb].generate(enc, n, mode=args.mode, ratio=ratio, uniforms=uniforms, temperature=args.temperature,
                                     top_k=args.top_k, top_p=args.top_p)
        audio = audio.cpu().numpy()
        for j, i in enumerate(batch):
            k, m = all_rows[i]
            s = 'no_speaker' if args.speakers[k] == 'None' else args.speakers[k]
            name = save_path + '/%d_%s_take_%d.wav' % (gs, s, m)
            wavfile.write(name, 16000, np.concatenate([wav[:n_prompt], audio[j]]))
            print('wrote', name)
    for gen in gens.values():
        gen.close()


def read_list(path, data_root):
    """The wav paths of an -audio_list file: one per line, blank lines and lines starting with # skipped, relative paths
    taken from data_root."""
    with open(path) as f:
        names = [ln.strip() for ln in f]
    return [n if os.path.isabs(n) else os.path.join(data_root, n) for n in names if n and not n.startswith('#')]


def row_uniforms(seed, row, n, stage=None):
    """The n uniforms of row `row` (list order, then speaker order): seeded by (seed, row) alone, so a row's draw does not
    depend on -rows, on the batch it lands in or on the sharding; unseeded without -seed.  stage (-prior -count: 0 the codes,
    1 the audio): a row's stages draw from generators of their own, seeded by child `stage` of the row's seed sequence
    (SeedSequence([seed, row], spawn_key=(stage,)) = .spawn(...)[stage]).  Not SeedSequence([seed, row, stage]): numpy pads
    the entropy with zeros, so [seed, row, 0] IS [seed, row] and stage 0 would repeat the unstaged draw."""
    if seed is None:
        return torch.rand(n)
    ss = np.random.SeedSequence([seed, row], spawn_key=() if stage is None else (stage,))
    s = int(ss.generate_state(1, np.uint64)[0] >> np.uint64(1))
    return torch.rand(n, generator=torch.Generator().manual_seed(s))


def convert_list(args, parser):
    """-audio_list: every (utterance, speaker) pair is one row of the wide generator (generator.WideGenerator).  Each
    utterance is read, trimmed and encoded on its own, exactly as -audio does it, so no utterance sees another's padding;
    rows are batched by length (generator.plan_rows), a batch's conditions are padded to its longest row by repeating the
    last frame, and each row's audio is cut to its own length."""
    for flag, on in (('-audio', args.audio_path is not None), ('-prior', args.prior_path is not None),
                     ('-prompt_samples', args.prompt_samples != 0), ('-prompt_frames', args.prompt_frames != 0),
                     ('-teacher_forced', args.teacher_forced)):
        if on:
            parser.error('-audio_list converts whole utterances with the wide generator: not with %s' % flag)
    if not 1 <= args.rows <= 1024:
        parser.error('-rows %d must be in 1..1024' % args.rows)
    if not args.speakers:
        parser.error('-audio_list needs -speakers')
    if not args.restore_path:
        parser.error('-audio_list needs -restore')
    if args.mode not in ('sample', 'greedy'):
        raise NotImplementedError('decode mode %s not implemented' % args.mode)
    if not os.path.isfile(args.audio_list):
        parser.error('-audio_list %s: no such file' % args.audio_list)
    paths = read_list(args.audio_list, args.data_root)
    if not paths:
        parser.error('-audio_list %s names no utterance' % args.audio_list)
    wavs = []
    for p in paths:
        if not os.path.isfile(p):
            parser.error('-audio_list: %s: no such file' % p)
        wav = read_wav(p)
        if len(wav) == 0:
            parser.error('-audio_list: %s is shorter than 512 samples' % p)
        wavs.append(wav)

    pkg = importlib.import_module('vq-vae-wavenet_amd')
    try:        # every row gets the same settings; checked before anything is loaded or built
        pkg.generator.sampling_settings(1, args.mode, args.temperature, args.top_k, args.top_p)
    except ValueError as e:
        parser.error(str(e))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0')) % max(torch.cuda.device_count(), 1)   # no collective: ranks may share a GPU
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    gs = int(args.restore_path.split('-')[-1].split('.')[0])
    from scipy.io import wavfile
    num_speakers, ids = speaker_ids(args, pkg)
    parameters, wavenet_parameters = pkg.model.load_configs(args.parameter_path)
    model = load_vqvae(args, pkg, parameters, wavenet_parameters, num_speakers, dev)
    out_dir = args.out_dir or args.restore_path.split('/weights')[0]
    os.makedirs(out_dir, exist_ok=True)

    ns = len(ids)
    all_rows = [(u, k) for u in range(len(wavs)) for k in range(ns)]          # list order, then speaker order
    mine = list(range(rank, len(all_rows), world))                            # rows sharded over ranks: no collective
    if not mine:
        return
    spk_all = torch.tensor(ids, dtype=torch.int64, device=dev)
    cond, ratio, seen = {}, None, set()
    for u in sorted({all_rows[r][0] for r in mine}):
        x = torch.from_numpy(wavs[u]).to(dev).unsqueeze(0).contiguous()
        enc = model.encode(x, spk_all)                 # this utterance alone with its speakers: what -audio computes
        r_u = len(wavs[u]) // enc.shape[2]
        if ratio is None:
            ratio = r_u
        assert r_u == ratio and enc.shape[2] * ratio == len(wavs[u])
        for r in mine:
            if all_rows[r][0] == u:
                cond[r] = enc[all_rows[r][1]].clone()
        if len(wavs[u]) not in seen:                   # the encode workspace is cached by (B, T): a list has many lengths
            seen.add(len(wavs[u]))
            model.free_workspaces()
    lengths = [len(wavs[all_rows[r][0]]) for r in mine]
    batches, padded = pkg.generator.plan_rows(lengths, args.rows)
    print('%d rows in %d batches of at most %d; %d of %d row-steps are padding'
          % (len(mine), len(batches), args.rows, padded, padded + sum(lengths)))
    gens = {}
    for batch in batches:
        nb, n = len(batch), max(lengths[j] for j in batch)
        Tz = n // ratio
        enc = torch.empty(nb, model.Cc, Tz, device=dev)
        for i, j in enumerate(batch):
            c = cond[mine[j]]
            enc[i, :, :c.shape[1]] = c
            enc[i, :, c.shape[1]:] = c[:, -1:]         # padded by repeating the last frame
        uniforms = None
        if args.mode == 'sample':
            uniforms = torch.zeros(nb, n)
            for i, j in enumerate(batch):
                uniforms[i, :lengths[j]] = row_uniforms(args.seed, mine[j], lengths[j])
            uniforms = uniforms.to(dev)
        if nb not in gens:
            gens[nb] = pkg.generator.WideGenerator(model, batch=nb)
        gen = gens[nb]
        gen.reset()
        audio, _ = gen.generate(enc, n, mode=args.mode, ratio=ratio, uniforms=uniforms, temperature=args.temperature,
                                top_k=args.top_k, top_p=args.top_p)
        audio = audio.cpu().numpy()
        for i, j in enumerate(batch):
            u, k = all_rows[mine[j]]
            s = 'no_speaker' if args.speakers[k] == 'None' else args.speakers[k]
            name = os.path.join(out_dir, '%d_%s_%s.wav' % (gs, os.path.splitext(os.path.basename(paths[u]))[0], s))
            wavfile.write(name, 16000, audio[i, :lengths[j]])
            print('wrote', name)
    for gen in gens.values():
        gen.close()


def read_wav(path, multiple=512):
    """The utterance as float32 at 16 kHz, trimmed to a multiple of 512 samples (generate.py:39, 512 = largest dilation)."""
    from scipy.io import wavfile
    sr, wav = wavfile.read(path)
    if wav.ndim > 1:
        wav = wav[:, 0]
    wav = wav.astype(np.float32) / 32768.0 if wav.dtype == np.int16 else wav.astype(np.float32)
    if sr != 16000:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(sr, 16000)
        wav = resample_poly(wav, 16000 // g, sr // g).astype(np.float32)
    return wav[:len(wav) // multiple * multiple]


def speaker_ids(args, pkg):
    first = args.speakers[0]
    if first[0] == 'p':
        spk_file, num_speakers = 'data/vctk_speakers.txt', 109
    elif first[0].lower() == 's':
        spk_file, num_speakers = 'data/aishell_speakers.txt', 340
    else:
        spk_file, num_speakers = 'data/librispeech_speakers.txt', 251
    speaker_to_int = pkg.data.get_speaker_to_int(spk_file) if os.path.exists(spk_file) else {}
    # 'None' -> all-zero one-hot -> argmax 0 (generate.py:59-60, model.py:22)
    ids = []
    for sp in args.speakers:
        if sp.lower() != 'none' and sp not in speaker_to_int:
            raise ValueError('unknown speaker %r (not in %s)' % (sp, spk_file))
        i = 0 if sp.lower() == 'none' else speaker_to_int[sp]
        if not 0 <= i < num_speakers:
            raise ValueError('speaker %r maps to %d, outside the %d-row speaker table' % (sp, i, num_speakers))
        ids.append(i)
    return num_speakers, ids


def load_vqvae(args, pkg, parameters, wavenet_parameters, num_speakers, dev):
    model = pkg.model.VQVAE(parameters, wavenet_parameters, num_speakers, device=dev, seed=0)
    if args.restore_path.endswith(('.safetensors', '.npz')):      # TF variable names (checkpoint.py); EMA shadows -> live
        pkg.checkpoint.load(model, args.restore_path, ema_to_live=True)
    else:
        model.load_state_dict(torch.load(args.restore_path, map_location='cpu', weights_only=True))
        model.use_ema_weights()                # generate.py:88-90
    return model


def teacher_forced(args, pkg, gs, rank, world, dev, parser):
    """The decoder's teacher-forced reconstruction of the utterance for every speaker: one pass, no generator."""
    from math import gcd
    from scipy.io import wavfile
    num_speakers, ids = speaker_ids(args, pkg)
    parameters, wavenet_parameters = pkg.model.load_configs(args.parameter_path)
    ratio = 320 if parameters.get('encoder', '64') == '2019' else 64
    wav = read_wav(args.audio_path, multiple=ratio)
    length = len(wav)
    if length == 0:
        parser.error('-audio: the utterance is shorter than one latent frame (%d samples)' % ratio)
    model = load_vqvae(args, pkg, parameters, wavenet_parameters, num_speakers, dev)     # the EMA weights are the live ones now
    save_path = args.restore_path.split('/weights')[0]
    lcm = 256 * ratio // gcd(256, ratio)
    padded = -(-length // lcm) * lcm
    mine = list(range(rank, len(ids), world))
    uniforms = None
    if args.mode == 'sample' and mine:     # one row of uniforms per requested speaker, whatever the sharding
        g = torch.Generator().manual_seed(args.seed) if args.seed is not None else None
        uniforms = torch.zeros(len(mine), padded)
        uniforms[:, :length] = torch.rand(len(ids), length, generator=g)[mine]
    for b0 in range(0, len(mine), 8):
        rows = mine[b0:b0 + 8]
        x = torch.zeros(len(rows), padded)
        x[:, :length] = torch.from_numpy(wav)
        spk = torch.tensor([ids[i] for i in rows], dtype=torch.int64, device=dev)
        audio, _ = model.reconstruct(x.to(dev), spk, lengths=[length] * len(rows), weights='live', mode=args.mode,
                                     uniforms=None if uniforms is None else uniforms[b0:b0 + len(rows)].contiguous().to(dev),
                                     temperature=args.temperature, top_k=args.top_k, top_p=args.top_p)
        audio = audio[:, :length].cpu().numpy()
        for j, i in enumerate(rows):
            s = 'no_speaker' if args.speakers[i] == 'None' else args.speakers[i]
            wavfile.write(save_path + '/%d_%s_teacher.wav' % (gs, s), 16000, audio[j])
            print('wrote', save_path + '/%d_%s_teacher.wav' % (gs, s))


def generate_from_prior(args, pkg, gs, rank, world, dev, parser):
    """Sample codes from the latent prior, decode them with the VQ-VAE's WaveNet (no input utterance; with -prompt_frames
    the utterance's first codes and samples are the prompt of both generators)."""
    from scipy.io import wavfile
    n_prompt = args.prompt_frames
    if n_prompt:
        wav = read_wav(args.audio_path)
        if n_prompt * 64 > len(wav):
            parser.error('-prompt_frames %d (%d samples) is longer than the trimmed utterance (%d samples)'
                         % (n_prompt, n_prompt * 64, len(wav)))
    num_speakers, ids = speaker_ids(args, pkg)
    parameters, wavenet_parameters = pkg.model.load_configs(args.parameter_path)
    prior_cfg = pkg.prior.load_prior_config(args.prior_params, parameters)
    model = load_vqvae(args, pkg, parameters, wavenet_parameters, num_speakers, dev)
    prior = pkg.prior.LatentPrior(prior_cfg, num_speakers, device=dev, seed=0, n_codes=model.Kc)
    prior.load_state_dict(torch.load(args.prior_path, map_location='cpu', weights_only=True))
    prior.use_ema_weights()
    save_path = args.restore_path.split('/weights')[0]
    if args.count > 1:
        return prior_corpus(args, pkg, gs, rank, world, dev, ids, model, prior, save_path)
    if args.takes > 1:
        return prior_takes(args, pkg, gs, rank, world, dev, ids, model, prior, save_path, wav)
    mine = list(range(rank, len(ids), world))
    n, length = args.frames, args.frames * 64
    g = torch.Generator().manual_seed(args.seed) if args.seed is not None else None
    u_codes = torch.rand(len(ids), n, generator=g)[mine].contiguous().to(dev) if args.mode == 'sample' else None
    u_audio = torch.rand(len(ids), length, generator=g)[mine].contiguous().to(dev) if args.mode == 'sample' else None
    if n_prompt and mine:
        x = torch.from_numpy(wav).to(dev).unsqueeze(0).contiguous()
        prompt_codes = model.encode_codes(x, torch.tensor([ids[mine[0]]], dtype=torch.int64, device=dev))[:, :n_prompt]
        prompt_audio = x[:, :n_prompt * 64]
    for b0 in range(0, len(mine), 8):
        rows = mine[b0:b0 + 8]
        sl = slice(b0, b0 + len(rows))
        spk = torch.tensor([ids[i] for i in rows], dtype=torch.int64, device=dev)
        pgen = pkg.generator.PriorGenerator(prior, batch=len(rows))
        if n_prompt:
            pgen.prefill(prompt_codes.expand(len(rows), n_prompt).contiguous(), spk)
        codes = pgen.sample(n, spk, mode=args.mode, uniforms=None if u_codes is None else u_codes[sl].contiguous(),
                            temperature=args.prior_temperature, top_k=args.prior_top_k, top_p=args.prior_top_p)
        pgen.close()
        if n_prompt:
            codes = torch.cat([prompt_codes.expand(len(rows), n_prompt), codes], dim=1).contiguous()
        cond = model.condition_from_codes(codes, spk)
        gen = pkg.generator.FastGenerator(model, batch=len(rows))
        if n_prompt:
            gen.prefill(prompt_audio.expand(len(rows), n_prompt * 64).contiguous(), cond, ratio=64)
        audio, _ = gen.generate(cond, length, mode=args.mode, ratio=64,
                                uniforms=None if u_audio is None else u_audio[sl].contiguous(),
                                temperature=args.temperature, top_k=args.top_k, top_p=args.top_p)
        gen.close()
        if n_prompt:
            audio = torch.cat([prompt_audio.expand(len(rows), n_prompt * 64), audio], dim=1)
        audio, codes = audio.cpu().numpy(), codes.cpu().numpy()
        for j, i in enumerate(rows):
            s = 'no_speaker' if args.speakers[i] == 'None' else args.speakers[i]
            wavfile.write(save_path + '/%d_%s_prior.wav' % (gs, s), 16000, audio[j])
            np.save(save_path + '/prior_codes_%d_%s.npy' % (gs, s), codes[j])
            print('wrote', save_path + '/%d_%s_prior.wav' % (gs, s))


def prior_corpus(args, pkg, gs, rank, world, dev, ids, model, prior, save_path):
    """-prior -count M: every (speaker k, take m) pair is row i = k M + m of both wide generators.  All rows have the same
    length, so the rows (sharded over ranks as convert_list shards them) are cut into consecutive batches of at most -rows:
    WidePriorGenerator draws the codes, condition_from_codes makes the condition, WideGenerator decodes it from reset.  With
    -seed row i draws its code uniforms from row_uniforms' stage 0 and its audio uniforms from stage 1; with the generators'
    batch independence a row's codes and audio depend neither on -rows nor on the sharding."""
    from scipy.io import wavfile
    M = args.count
    n, length = args.frames, args.frames * 64
    all_rows = [(k, m) for k in range(len(ids)) for m in range(M)]            # speaker order, then take
    mine = list(range(rank, len(all_rows), world))                            # rows sharded over ranks: no collective
    pgens, gens = {}, {}
    for b0 in range(0, len(mine), args.rows):
        batch = mine[b0:b0 + args.rows]
        nb = len(batch)
        spk = torch.tensor([ids[all_rows[i][0]] for i in batch], dtype=torch.int64, device=dev)
        u_codes = u_audio = None
        if args.mode == 'sample':
            u_codes = torch.stack([row_uniforms(args.seed, i, n, stage=0) for i in batch]).to(dev)
            u_audio = torch.stack([row_uniforms(args.seed, i, length, stage=1) for i in batch]).to(dev)
        if nb not in gens:
            pgens[nb] = pkg.generator.WidePriorGenerator(prior, batch=nb)
            gens[nb] = pkg.generator.WideGenerator(model, batch=nb)
        pgens[nb].reset()
        codes = pgens[nb].sample(n, spk, mode=args.mode, uniforms=u_codes, temperature=args.prior_temperature,
                                 top_k=args.prior_top_k, top_p=args.prior_top_p)
        cond = model.condition_from_codes(codes, spk)
        gens[nb].reset()
        audio, _ = gens[nb].generate(cond, length, mode=args.mode, ratio=64, uniforms=u_audio, temperature=args.temperature,
                                     top_k=args.top_k, top_p=args.top_p)
        audio, codes = audio.cpu().numpy(), codes.cpu().numpy()
        for j, i in enumerate(batch):
            k, m = all_rows[i]
            s = 'no_speaker' if args.speakers[k] == 'None' else args.speakers[k]
            wavfile.write(save_path + '/%d_%s_prior_%d.wav' % (gs, s, m), 16000, audio[j])
            np.save(save_path + '/prior_codes_%d_%s_%d.npy' % (gs, s, m), codes[j])
            print('wrote', save_path + '/%d_%s_prior_%d.wav' % (gs, s, m))
    for gen in list(pgens.values()) + list(gens.values()):
        gen.close()


def prior_takes(args, pkg, gs, rank, world, dev, ids, model, prior, save_path, wav):
    """-prior -audio -prompt_frames N -takes M: every (speaker k, take m) pair is row i = k M + m of both wide generators, in
    batches of at most -rows.  WidePriorGenerator is prefilled with the utterance's first N codes and draws -frames more
    (row_uniforms' stage 0); WideGenerator is prefilled with the first N x 64 samples and decodes the new codes (stage 1)."""
    from scipy.io import wavfile
    M, n_prompt = args.takes, args.prompt_frames
    n, length = args.frames, args.frames * 64
    all_rows = [(k, m) for k in range(len(ids)) for m in range(M)]            # speaker order, then take
    mine = list(range(rank, len(all_rows), world))                            # rows sharded over ranks: no collective
    if not mine:
        return
    x = torch.from_numpy(wav).to(dev).unsqueeze(0).contiguous()
    prompt_codes = model.encode_codes(x, torch.tensor([ids[0]], dtype=torch.int64, device=dev))[:, :n_prompt]
    prompt_audio = x[:, :n_prompt * 64]
    pgens, gens = {}, {}
    for b0 in range(0, len(mine), args.rows):
        batch = mine[b0:b0 + args.rows]
        nb = len(batch)
        spk = torch.tensor([ids[all_rows[i][0]] for i in batch], dtype=torch.int64, device=dev)
        u_codes = torch.stack([row_uniforms(args.seed, i, n, stage=0) for i in batch]).to(dev)
        u_audio = torch.stack([row_uniforms(args.seed, i, length, stage=1) for i in batch]).to(dev)
        if nb not in gens:
            pgens[nb] = pkg.generator.WidePriorGenerator(prior, batch=nb)
            gens[nb] = pkg.generator.WideGenerator(model, batch=nb)
        pgens[nb].prefill_codes(prompt_codes.expand(nb, n_prompt).contiguous(), spk)
        codes = pgens[nb].sample(n, spk, mode=args.mode, uniforms=u_codes, temperature=args.prior_temperature,
                                 top_k=args.prior_top_k, top_p=args.prior_top_p)
        codes = torch.cat([prompt_codes.expand(nb, n_prompt), codes], dim=1).contiguous()
        cond = model.condition_from_codes(codes, spk)
        gens[nb].prefill_prompt(prompt_audio.expand(nb, n_prompt * 64).contiguous(), cond, ratio=64)
        audio, _ = gens[nb].generate(cond, length, mode=args.mode, ratio=64, uniforms=u_audio, temperature=args.temperature,
                                     top_k=args.top_k, top_p=args.top_p)
        audio = torch.cat([prompt_audio.expand(nb, n_prompt * 64), audio], dim=1).cpu().numpy()
        codes = codes.cpu().numpy()
        for j, i in enumerate(batch):
            k, m = all_rows[i]
            s = 'no_speaker' if args.speakers[k] == 'None' else args.speakers[k]
            wavfile.write(save_path + '/%d_%s_prior_take_%d.wav' % (gs, s, m), 16000, audio[j])
            np.save(save_path + '/prior_codes_%d_%s_take_%d.npy' % (gs, s, m), codes[j])
            print('wrote', save_path + '/%d_%s_prior_take_%d.wav' % (gs, s, m))
    for gen in list(pgens.values()) + list(gens.values()):
        gen.close()


if __name__ == '__main__':
    main()
