"""Input pipeline: mirror of dataset.py:33-84,114-144 and utils.py:93-100 of the reference.

`-dataset synthetic` (what bench.py measures) needs no files.  The real datasets read 16 kHz
mono WAVs listed in `<relative_path>/<name>_train.txt` with speaker ids from
`<relative_path>/<name>_speakers.txt` ("<id>, <int>" per line), pick a random file and a random
crop of max_len samples per example and scale int16 PCM as (pcm + 0.5) / 32767.5
(dataset.py:41).  librosa is not available; files at other sample rates are resampled with
scipy.signal.resample_poly.
"""
import math
import os
import queue
import threading

import numpy as np
import torch


def get_speaker_to_int(speaker_path):
    """utils.py:93-100."""
    speaker_to_int = {}
    with open(speaker_path) as f:
        for line in f:
            if line.strip():
                speaker, number = line.strip().split(', ')
                speaker_to_int[speaker] = int(number)
    return speaker_to_int


class Synthetic:
    """SURVEY.md 8(d) synthetic int16-PCM segments (4 sinusoids x slow envelope + noise)."""

    def __init__(self, batch_size, max_len, num_speakers=109, seed=1234, device='cuda', whole=False, unit=64, min_len=None):
        self.B, self.T, self.num_speakers, self.dev = batch_size, max_len, num_speakers, device
        self.g = torch.Generator().manual_seed(seed)
        # whole: rows of random lengths as WavDataset(whole=True) hands them out (multiples of unit in [min_len, T], zeros behind),
        # drawn from a generator of their own: the audio is what it is without the option
        self.whole, self.unit, self.min_len = whole, unit, _whole_min_len(whole, unit, min_len, max_len)
        self.g_len = torch.Generator().manual_seed(seed + 104729)

    def next(self):
        return _to_device(self.next_host(), self.dev)

    def next_host(self):
        B, T, g = self.B, self.T, self.g
        n = torch.arange(T, dtype=torch.float64)
        f = 80 + (3400 - 80) * torch.rand(B, 4, generator=g, dtype=torch.float64)
        ph = 2 * math.pi * torch.rand(B, 4, generator=g, dtype=torch.float64)
        env = 0.6 + 0.4 * torch.sin(2 * math.pi * n / T * (1 + 3 * torch.rand(B, 1, generator=g, dtype=torch.float64)))
        s = torch.sin(2 * math.pi * f[:, :, None] * n / 16000.0 + ph[:, :, None]).sum(1)
        wav = torch.clamp(0.25 * s * env + 0.02 * torch.randn(B, T, generator=g, dtype=torch.float64), -1, 1)
        pcm = torch.round(wav * 32767).to(torch.int16)
        x = (pcm.to(torch.float32) + 0.5) / 32767.5
        spk = torch.randint(0, self.num_speakers, (B,), generator=g)
        if not self.whole:
            return x, spk
        lo, hi = -(-self.min_len // self.unit), T // self.unit
        lengths = (torch.randint(lo, hi + 1, (B,), generator=self.g_len) * self.unit).to(torch.int32)
        x = x * (torch.arange(T)[None, :] < lengths[:, None])
        return x, spk, lengths


def _whole_min_len(whole, unit, min_len, max_len):
    """The shortest admitted row of a whole-utterance source, checked: 1 <= unit, unit | T, and min_len in [1, T] (default: unit)."""
    if not whole:
        if min_len is not None:
            raise ValueError('min_len is an option of whole-utterance sources (whole=True)')
        return None
    min_len = unit if min_len is None else int(min_len)
    if unit < 1 or max_len % unit or not 1 <= min_len <= max_len:
        raise ValueError('whole utterances: unit %d must divide max_len %d and min_len %d lie in 1..max_len' % (unit, max_len, min_len))
    return min_len


def _to_device(batch, dev):
    """(x, spk[, lengths]) of next_host() with x and spk on the device; the lengths stay CPU tensors (the model uploads them)."""
    return tuple(t.to(dev, non_blocking=True) for t in batch[:2]) + tuple(batch[2:])


class Prefetcher:
    """The reference feeds its graph from a tf.data pipeline with prefetch (dataset.py:75-84); here a background thread
    reads / crops / resamples the NEXT batches into pinned host buffers while the GPU runs the current step, and `next()`
    only starts the asynchronous host-to-device copy (8 x 6656 fp32 = 213 KB per batch).  `source.next_host()` must return
    (x float32 [B, T], speaker ids int64 [B]) as CPU tensors, or that with more CPU tensors behind (a whole-utterance source:
    lengths int32 [B]).  next() returns as many: x and the speaker ids on the device, the others as CPU tensors of their own
    (the model uploads lengths itself).  `waits` counts the calls that found no batch ready."""

    def __init__(self, source, depth=3, device='cuda'):
        self.source, self.dev = source, torch.device(device)
        self.num_speakers = getattr(source, 'num_speakers', None)
        self.pin = self.dev.type == 'cuda' and torch.cuda.is_available()
        self.slots, self.free, self.ready = [], queue.Queue(), queue.Queue()
        self.waits, self.served, self.error = 0, 0, None
        self.depth = depth
        self._stop = threading.Event()
        self.thread = threading.Thread(target=self._produce, name='vqw-prefetch', daemon=True)
        self.thread.start()

    def _slot(self, x, spk, *rest):
        mk = (lambda t: torch.empty_like(t).pin_memory()) if self.pin else torch.empty_like
        return {'x': mk(x), 'spk': mk(spk), 'rest': [torch.empty_like(t) for t in rest], 'event': torch.cuda.Event() if self.pin else None,
                'used': False}

    def _produce(self):
        try:
            while not self._stop.is_set():
                x, spk, *rest = self.source.next_host()
                if len(self.slots) < self.depth:
                    self.slots.append(self._slot(x, spk, *rest))
                    i = len(self.slots) - 1
                else:
                    while True:
                        try:
                            i = self.free.get(timeout=0.1)
                            break
                        except queue.Empty:
                            if self._stop.is_set():
                                return
                slot = self.slots[i]
                if slot['used'] and slot['event'] is not None:
                    slot['event'].synchronize()          # the copy that last read this pinned buffer has finished
                slot['x'].copy_(x)
                slot['spk'].copy_(spk)
                for dst, src in zip(slot['rest'], rest):
                    dst.copy_(src)
                self.ready.put(i)
        except BaseException as e:      # surfaced by next()
            self.error = e
            self.ready.put(None)

    def next(self):
        if self.ready.empty():
            self.waits += 1
        i = self.ready.get()
        if i is None:
            raise RuntimeError('input pipeline failed') from self.error
        slot = self.slots[i]
        x = slot['x'].to(self.dev, non_blocking=True)
        spk = slot['spk'].to(self.dev, non_blocking=True)
        if not self.pin:                                  # (CPU target: .to() may alias the buffer)
            x, spk = x.clone(), spk.clone()
        else:
            slot['event'].record()
        rest = tuple(t.clone() for t in slot['rest'])    # (host tensors of the caller's own: the slot is refilled behind its back)
        slot['used'] = True
        self.free.put(i)
        self.served += 1
        return (x, spk) + rest

    def close(self):
        self._stop.set()
        self.thread.join(timeout=2.0)


class WavDataset:
    """dataset.py:14-84: random file, random crop, one-hot speaker (here: speaker index)."""
    speaker_of = staticmethod(lambda rel: rel.split('/')[0])

    def __init__(self, batch_size, max_len, relative_path, list_name, speakers_name, data_dir='', sr=16000,
                 seed=0, device='cuda', rank=0, world=1, whole=False, unit=64, min_len=None):
        """whole=True (train_prior.py -whole_utterances): next_host() also returns lengths int32 [B].  A file is trimmed to a
        multiple of `unit` samples and refused below `min_len` (default: unit); one shorter than max_len is taken WHOLE from its
        first sample and zero-padded, its length its own; a longer one gives a uniformly random window of max_len samples, as
        without the option, with length max_len.  Off, nothing changes."""
        self.B, self.T, self.sr, self.dev = batch_size, max_len, sr, device
        self.whole, self.unit, self.min_len = whole, unit, _whole_min_len(whole, unit, min_len, max_len)
        self.root = relative_path
        self.data_dir = data_dir
        with open(os.path.join(relative_path, list_name)) as f:
            self.files = [ln.strip() for ln in f if ln.strip()]
        self.speaker_to_int = get_speaker_to_int(os.path.join(relative_path, speakers_name))
        self.num_speakers = len(self.speaker_to_int)
        bad = {k: v for k, v in self.speaker_to_int.items() if not 0 <= v < self.num_speakers}
        if bad:      # the id indexes the [num_speakers][Cs] embedding table (model.py:19-27)
            raise ValueError('%s: speaker ids outside 0..%d: %s' % (speakers_name, self.num_speakers - 1, sorted(bad.items())[:5]))
        self.rng = np.random.RandomState(seed + 7919 * rank)

    def _read(self, rel):
        """-> float32 samples in [-1,1].  16 kHz int16 files: (pcm + 0.5) / 32767.5 (dataset.py:41);
        other rates are resampled to 16 kHz from pcm / 32768 (what librosa.load returns, :50)."""
        from scipy.io import wavfile
        sr, wav = wavfile.read(os.path.join(self.root, self.data_dir, rel))
        if wav.ndim > 1:
            wav = wav[:, 0]
        if sr == self.sr and wav.dtype == np.int16:
            return ((wav.astype(np.float32) + 0.5) / 32767.5).astype(np.float32)
        f = wav.astype(np.float64) / 32768.0 if wav.dtype == np.int16 else wav.astype(np.float64)
        if sr != self.sr:
            from scipy.signal import resample_poly
            g = math.gcd(sr, self.sr)
            f = resample_poly(f, self.sr // g, sr // g)
        return f.astype(np.float32)

    def next(self):
        return _to_device(self.next_host(), self.dev)

    def _next_whole(self):
        x, ss, ls, tries = np.zeros((self.B, self.T), dtype=np.float32), [], [], 0
        while len(ss) < self.B:
            rel = self.files[self.rng.randint(len(self.files))]
            wav = self._read(rel)
            n = len(wav) // self.unit * self.unit
            if n < self.min_len:                        # too short to learn from -> another file
                tries += 1
                if tries > 1000 * self.B:
                    raise ValueError('no file of at least %d samples among 1000 draws per row' % self.min_len)
                continue
            if n > self.T:
                start, n = self.rng.randint(0, n - self.T + 1), self.T
                x[len(ss)] = wav[start:start + n]
            else:
                x[len(ss), :n] = wav[:n]
            ss.append(self.speaker_to_int[self.speaker_of(rel)])
            ls.append(n)
        return torch.from_numpy(x), torch.tensor(ss, dtype=torch.int64), torch.tensor(ls, dtype=torch.int32)

    def next_host(self):
        if self.whole:
            return self._next_whole()
        xs, ss = [], []
        while len(xs) < self.B:
            rel = self.files[self.rng.randint(len(self.files))]
            wav = self._read(rel)
            if len(wav) <= self.T:                      # dataset.py:44-45: too short -> another file
                continue
            start = self.rng.randint(0, len(wav) - self.T)
            xs.append(wav[start:start + self.T])
            ss.append(self.speaker_to_int[self.speaker_of(rel)])
        return torch.from_numpy(np.stack(xs)), torch.tensor(ss, dtype=torch.int64)


class VCTK(WavDataset):       # dataset.py:125-133
    def __init__(self, batch_size, max_len, relative_path='data/', **kw):
        super().__init__(batch_size, max_len, relative_path, 'vctk_train.txt', 'vctk_speakers.txt',
                         data_dir='VCTK-Corpus/wav48/', **kw)


class LibriSpeech(WavDataset):  # dataset.py:114-122
    speaker_of = staticmethod(lambda rel: rel.split('/')[-1].split('-', 1)[0])

    def __init__(self, batch_size, max_len, relative_path='data/', **kw):
        super().__init__(batch_size, max_len, relative_path, 'librispeech_train_clean_100.txt', 'librispeech_speakers.txt', **kw)


class Aishell(WavDataset):     # dataset.py:136-144
    speaker_of = staticmethod(lambda rel: rel.split('/train/')[1].split('/')[0])

    def __init__(self, batch_size, max_len, relative_path='data/', **kw):
        super().__init__(batch_size, max_len, relative_path, 'aishell_train.txt', 'aishell_speakers.txt', **kw)


# ---------------------------------------------------------------------------- held-out lists (evaluate.py, train.py -eval_list)
DATASETS = {'VCTK': VCTK, 'LibriSpeech': LibriSpeech, 'Aishell': Aishell}


class HeldOutList:
    """A list file in the format of the `<name>_train.txt` lists (one path per line, relative to the dataset's wav directory
    under `relative_path`), read in FILE ORDER with no random crops; speaker ids come from the path and
    `<relative_path>/<name>_speakers.txt`, as in WavDataset.  `ratio`: the encoder's samples per latent frame (64; 320 for
    the '2019' encoder): whole utterances are trimmed to a multiple of it."""

    def __init__(self, dataset, list_path, relative_path='data/', ratio=64, sr=16000):
        if dataset not in DATASETS:
            raise NotImplementedError('dataset %s has no file lists' % dataset)
        cls = DATASETS[dataset]
        self.reader = cls.__new__(cls)            # WavDataset._read / speaker_of, without its training list
        self.reader.root, self.reader.sr = relative_path, sr
        self.reader.data_dir = 'VCTK-Corpus/wav48/' if dataset == 'VCTK' else ''
        with open(list_path) as f:
            self.files = [ln.strip() for ln in f if ln.strip()]
        speakers = {'VCTK': 'vctk_speakers.txt', 'LibriSpeech': 'librispeech_speakers.txt', 'Aishell': 'aishell_speakers.txt'}[dataset]
        self.speaker_to_int = get_speaker_to_int(os.path.join(relative_path, speakers))
        self.num_speakers = len(self.speaker_to_int)
        self.ratio = ratio

    def speaker(self, rel):
        return self.speaker_to_int[self.reader.speaker_of(rel)]

    def read(self, rel):
        return self.reader._read(rel)

    def utterances(self, files=None):
        """[(file, speaker id, samples trimmed to a multiple of ratio)] in file order; files shorter than one frame are
        left out (second result: how many)."""
        out, skipped = [], 0
        for rel in (self.files if files is None else files):
            wav = self.read(rel)
            n = len(wav) // self.ratio * self.ratio
            if n == 0:
                skipped += 1
                continue
            out.append((rel, self.speaker(rel), wav[:n]))
        return out, skipped

    def crops(self, length, limit=None, files=None):
        """[(file, speaker id, the first `length` samples)] of the files that are long enough, in file order, at most
        `limit` of them; the second result counts the files that were too short."""
        out, skipped = [], 0
        for rel in (self.files if files is None else files):
            if limit is not None and len(out) >= limit:
                break
            wav = self.read(rel)
            if len(wav) < length:
                skipped += 1
                continue
            out.append((rel, self.speaker(rel), wav[:length]))
        return out, skipped


def padded_length(n, multiple=256):
    """The batch length for a longest row of n samples: n rounded up to a multiple of `multiple` (the plane engine's tiles)."""
    return -(-n // multiple) * multiple


def padded_batches(utts, batch_size, multiple=256):
    """Sort utterances [(file, speaker, samples)] by length (stable: file order among equals), cut them into batches of
    batch_size and zero-pad each batch to its longest row rounded up to `multiple`.  Yields (files, x float32 [B][T],
    speaker ids int64 [B], lengths [B]) as host tensors / lists."""
    order = sorted(range(len(utts)), key=lambda i: len(utts[i][2]))
    for i0 in range(0, len(order), batch_size):
        rows = [utts[i] for i in order[i0:i0 + batch_size]]
        lengths = [len(r[2]) for r in rows]
        x = np.zeros((len(rows), padded_length(max(lengths), multiple)), dtype=np.float32)
        for j, r in enumerate(rows):
            x[j, :lengths[j]] = r[2]
        yield [r[0] for r in rows], torch.from_numpy(x), torch.tensor([r[1] for r in rows], dtype=torch.int64), lengths


def fixed_batches(utts, batch_size):
    """Batches of equally long crops [(file, speaker, samples)] in list order, as padded_batches yields them (lengths None:
    whole rows are scored)."""
    for i0 in range(0, len(utts), batch_size):
        rows = utts[i0:i0 + batch_size]
        yield ([r[0] for r in rows], torch.from_numpy(np.stack([r[2] for r in rows])),
               torch.tensor([r[1] for r in rows], dtype=torch.int64), None)
