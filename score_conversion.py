#!/usr/bin/env python3
"""score_conversion.py -- mel-cepstral distortion (MCD) of converted speech against the target speaker's own recordings of
the same sentences (no counterpart in the reference).  Needs no model and no checkpoint: wavs in, one number out.

    python3 score_conversion.py -pairs pairs.txt [-data_root D] [-batch 64] [-per_pair] [-out mcd.json] [-dry_run]
    python3 score_conversion.py -converted_dir DIR -list data/vctk_heldout.txt -speakers p226 p227 -step 110640 [-data_root D]

`-pairs`: one `<converted wav> <target wav>` per line (blank lines and lines starting with # skipped, relative paths taken
from `-data_root`).  The second form builds the pairs from what `generate.py -audio_list` wrote: for every source file of
`-list` (generate.py's list format) and every speaker, the converted file is `DIR/<step>_<basename>_<speaker>.wav` and the
target follows VCTK's parallel numbering: a source `<src>_<nnn>.wav` maps to `<speaker>_<nnn>.wav`, looked up beside the
source file and then in the sibling directory `../<speaker>/` (VCTK's wav48/<speaker>/ layout).  A pair whose target does
not exist is left out and counted as `missing` (VCTK's speakers did not all read every sentence); no pair left is an error.

Every file is read with generate.py's read_wav (first channel, resampled to 16 kHz, trimmed to a multiple of 512 samples).
Pairs are sorted by length, batched (`-batch` pairs, zero-padded) and scored by scoring.mcd: 13 MFCCs at 100 frames per
second on both sides, a DTW alignment over coefficients 1..12 (vqw_cepstral_dtw), MCD = (10 sqrt 2 / ln 10) * cost / steps
in dB.  scoring.py has the definition and why the number is not comparable with MCD figures based on mel-generalised cepstra.

Prints ONE JSON line (and writes it to `-out`): pairs, missing, mcd_mean (the mean over pairs), mcd_frame_weighted
(sum(K * cost) / sum(steps)), mcd_min, mcd_max, frames (both sides, all pairs), path_steps; with `-per_pair` a list of
{converted, target, mcd, cost, steps, frames_x, frames_y} in the order of the pairs.  `-dry_run` prints the pairs and the
missing count and stops before the GPU is touched.  A file of more than 4096 frames (40.96 s) is refused by name before any
audio is read; so are files that do not exist and files shorter than 512 samples.
"""
import importlib
import json
import os
import re
import sys
from argparse import ArgumentParser

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MAX_FRAMES, FRAME_STEP, TRIM = 4096, 160, 512


def rooted(path, data_root):
    return path if os.path.isabs(path) else os.path.join(data_root, path)


def read_pairs(path, data_root, parser):
    """The (converted, target) paths of a -pairs file."""
    pairs = []
    with open(path) as f:
        for no, ln in enumerate(f, 1):
            ln = ln.strip()
            if not ln or ln.startswith('#'):
                continue
            names = ln.split()
            if len(names) != 2:
                parser.error('-pairs %s line %d: expected `<converted wav> <target wav>`, got %r' % (path, no, ln))
            pairs.append((rooted(names[0], data_root), rooted(names[1], data_root)))
    return pairs


def target_of(source, speaker):
    """VCTK's parallel numbering: <src>_<nnn>.wav -> <speaker>_<nnn>.wav beside the source, else in ../<speaker>/.  None if
    neither exists; ValueError if the source's name has no sentence number."""
    m = re.match(r'^(.+)_(\d+)$', os.path.splitext(os.path.basename(source))[0])
    if m is None:
        raise ValueError(source)
    name = '%s_%s.wav' % (speaker, m.group(2))
    here = os.path.dirname(source)
    for cand in (os.path.join(here, name), os.path.join(os.path.dirname(here), speaker, name)):
        if os.path.isfile(cand):
            return cand
    return None


def build_pairs(args, parser):
    """The pairs of the -converted_dir form and how many targets were missing."""
    with open(args.list_path) as f:
        sources = [ln.strip() for ln in f]
    sources = [rooted(n, args.data_root) for n in sources if n and not n.startswith('#')]       # generate.py's read_list
    pairs, missing = [], 0
    for src in sources:
        base = os.path.splitext(os.path.basename(src))[0]
        for spk in args.speakers:
            try:
                target = target_of(src, spk)
            except ValueError:
                parser.error('-list %s: %s is not named <speaker>_<number>.wav, so it has no parallel sentence' % (args.list_path, src))
            if target is None:
                missing += 1
                continue
            pairs.append((os.path.join(args.converted_dir, '%d_%s_%s.wav' % (args.step, base, spk)), target))
    return pairs, missing


def header_frames(path, parser):
    """Cepstral frames the file will have at 16 kHz after read_wav's trim, from its header alone (the samples stay on disk)."""
    from scipy.io import wavfile
    if not os.path.isfile(path):
        parser.error('%s: no such file' % path)
    sr, wav = wavfile.read(path, mmap=True)
    n = -(-wav.shape[0] * 16000 // sr) // TRIM * TRIM
    if n < TRIM:
        parser.error('%s is shorter than %d samples at 16 kHz' % (path, TRIM))
    frames = -(-n // FRAME_STEP)
    if frames > MAX_FRAMES:
        parser.error('%s has %d frames (%.2f s); the alignment takes at most %d frames (%.2f s)'
                     % (path, frames, n / 16000.0, MAX_FRAMES, MAX_FRAMES * FRAME_STEP / 16000.0))
    return frames


def main():
    parser = ArgumentParser()
    parser.add_argument('-pairs', dest='pairs_path', help='text file of `<converted wav> <target wav>` lines')
    parser.add_argument('-converted_dir', help='directory generate.py -audio_list wrote (<step>_<basename>_<speaker>.wav)')
    parser.add_argument('-list', dest='list_path', help='with -converted_dir: the -audio_list file the conversion was made from')
    parser.add_argument('-speakers', nargs='+', help='with -converted_dir: the target speakers, as given to generate.py')
    parser.add_argument('-step', type=int, help='with -converted_dir: the checkpoint step in the converted files\' names')
    parser.add_argument('-data_root', default='', help='directory that relative paths of -pairs / -list start from')
    parser.add_argument('-batch', default=64, type=int, dest='batch_size', help='pairs per batch (one workgroup each)')
    parser.add_argument('-per_pair', action='store_true', help='add one entry per pair to the report')
    parser.add_argument('-out', dest='out_path', help='write the JSON report here too')
    parser.add_argument('-dry_run', action='store_true', help='print the pairs and the missing count; no GPU')
    args = parser.parse_args()
    if (args.pairs_path is None) == (args.converted_dir is None):
        parser.error('give exactly one of -pairs and -converted_dir (got %s)' % ('both' if args.pairs_path is not None else 'neither'))
    if args.batch_size < 1:
        parser.error('-batch must be at least 1')
    if args.pairs_path is not None:
        if args.list_path is not None or args.speakers is not None or args.step is not None:
            parser.error('-list, -speakers and -step belong to -converted_dir, not to -pairs')
        if not os.path.isfile(args.pairs_path):
            parser.error('-pairs %s: no such file' % args.pairs_path)
        pairs, missing = read_pairs(args.pairs_path, args.data_root, parser), 0
    else:
        if args.list_path is None or args.speakers is None or args.step is None:
            parser.error('-converted_dir needs -list, -speakers and -step')
        if not os.path.isdir(args.converted_dir):
            parser.error('-converted_dir %s: no such directory' % args.converted_dir)
        if not os.path.isfile(args.list_path):
            parser.error('-list %s: no such file' % args.list_path)
        pairs, missing = build_pairs(args, parser)
    if not pairs:
        parser.error('no pair to score (%d without a target recording)' % missing)
    frames = [(header_frames(c, parser), header_frames(t, parser)) for c, t in pairs]
    if args.dry_run:
        print(json.dumps({'pairs': [list(p) for p in pairs], 'missing': missing, 'frames': [list(f) for f in frames]}))
        return

    import numpy as np
    import torch
    from generate import read_wav
    pkg = importlib.import_module('vq-vae-wavenet_amd')
    S = pkg.scoring
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
    order = sorted(range(len(pairs)), key=lambda i: frames[i])           # stable: list order among equals
    results, rows = [], [None] * len(pairs)
    for i0 in range(0, len(order), args.batch_size):
        batch = order[i0:i0 + args.batch_size]
        sides = []
        for side in (0, 1):
            wavs = [read_wav(pairs[i][side]) for i in batch]
            x = np.zeros((len(batch), max(len(w) for w in wavs)), dtype=np.float32)
            for j, w in enumerate(wavs):
                x[j, :len(w)] = w
            sides.append((torch.from_numpy(x).cuda(), [len(w) for w in wavs]))
        r = S.mcd(sides[0][0], sides[1][0], sides[0][1], sides[1][1])
        results.append(r)
        for j, i in enumerate(batch):
            rows[i] = {'converted': pairs[i][0], 'target': pairs[i][1], 'mcd': float(r.mcd[j]), 'cost': float(r.cost[j]),
                       'steps': int(r.steps[j]), 'frames_x': int(r.frames_x[j]), 'frames_y': int(r.frames_y[j])}
    report = S.mcd_report(results, missing=missing)
    if args.per_pair:
        report['per_pair'] = rows
    line = json.dumps(report)
    if args.out_path:
        with open(args.out_path, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
