"""CPU tests of held-out scoring: the float64 restatement (score_ref.py) on hand-made cases, the host-side helpers
(scoring.bits / perplexity / used), the refusals of evaluate.py and of train.py's -eval_* flags (before anything is
loaded), the C entry points' argument checks, and the held-out list reader on wavs written to tmp_path."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def test_ref_uniform_and_certain_positions():
    z = np.zeros((1, 4, 3))
    z[0, :, 1] = [1000.0, -1000.0, -1000.0, -1000.0]          # the label has probability 1
    z[0, :, 2] = [0.0, math.log(3.0), 0.0, 0.0]
    r = SR.score_ref(z, np.array([[2, 0, 1]]))
    np.testing.assert_allclose(r['nll'][0, 0], math.log(4.0), rtol=1e-15)
    np.testing.assert_allclose(r['entropy'][0, 0], math.log(4.0), rtol=1e-15)
    assert r['nll'][0, 1] == 0.0 and r['entropy'][0, 1] == 0.0
    p = np.array([1, 3, 1, 1]) / 6.0
    np.testing.assert_allclose(r['nll'][0, 2], -math.log(0.5), rtol=1e-14)
    np.testing.assert_allclose(r['entropy'][0, 2], -(p * np.log(p)).sum(), rtol=1e-14)
    assert r['count'].tolist() == [3]
    # position 0: every logit is a maximum, the lowest index (0) wins: label 2 is no hit; positions 1 and 2 hit
    assert r['hits'].tolist() == [2]
    np.testing.assert_allclose(r['nll_sum'][0], r['nll'].sum(), rtol=1e-15)


def test_ref_tie_lowest_index_wins():
    z = np.array([[[1.0], [5.0], [5.0], [0.0]]])              # Q = 4, maxima at 1 and 2
    assert SR.score_ref(z, np.array([[1]]))['hits'].tolist() == [1]
    assert SR.score_ref(z, np.array([[2]]))['hits'].tolist() == [0]


def test_ref_masks():
    g = np.random.RandomState(0)
    z = g.randn(3, 8, 10) * 3
    lab = g.randint(0, 8, (3, 10))
    full = SR.score_ref(z, lab)
    r = SR.score_ref(z, lab, t_begin=[0, 4, 6], t_end=[10, 9, 6])
    assert r['count'].tolist() == [10, 5, 0]
    assert (r['nll'][1, :4] == 0).all() and (r['nll'][1, 9:] == 0).all() and (r['entropy'][2] == 0).all()
    np.testing.assert_array_equal(r['nll'][1, 4:9], full['nll'][1, 4:9])
    np.testing.assert_allclose(r['nll_sum'][1], full['nll'][1, 4:9].sum(), rtol=1e-15)
    assert r['nll_sum'][2] == 0 and r['hits'][2] == 0
    assert r['hits'][1] == ((z[1].argmax(0) == lab[1])[4:9]).sum()
    # the float32 evaluation of the same formulas stays within float32's reach of the float64 one
    r32 = SR.score_ref(z, lab, dtype=np.float32)
    assert r32['nll'].dtype == np.float32 and np.abs(r32['nll'] - full['nll']).max() < 1e-5


def test_histogram_ref():
    idx = np.array([[0, 1, 1, 7], [3, 3, 9, -1]])
    c, bad = SR.histogram_ref(idx, 8)
    assert c.tolist() == [1, 2, 0, 2, 0, 0, 0, 1] and bad
    c, bad = SR.histogram_ref(idx, 8, f_end=[3, 2])
    assert c.tolist() == [1, 2, 0, 2, 0, 0, 0, 0] and not bad


# ------------------------------------------------------------------ host-side helpers
def test_bits_perplexity_used(pkg):
    S = pkg.scoring
    assert S.bits(math.log(2.0) * 10, 10) == pytest.approx(1.0, rel=1e-15)
    assert S.bits(math.log(256.0) * 7, 7) == pytest.approx(8.0, rel=1e-15)
    with pytest.raises(ValueError):
        S.bits(1.0, 0)
    for k in (1, 2, 32, 512):
        assert S.perplexity(np.full(k, 5)) == pytest.approx(k, rel=1e-12)
    assert S.perplexity([0, 0, 9, 0]) == 1.0
    assert S.perplexity([3, 0, 3, 0, 0]) == pytest.approx(2.0, rel=1e-15)          # zeros are ignored
    assert S.perplexity(np.array([1, 3])) == pytest.approx(math.exp(-(0.25 * math.log(0.25) + 0.75 * math.log(0.75))), rel=1e-15)
    assert S.used([0, 4, 0, 1]) == 2 and S.used(np.zeros(5)) == 0
    with pytest.raises(ValueError):
        S.perplexity([0, 0])
    with pytest.raises(ValueError):
        S.perplexity([1, -1])


def test_totals_merge_and_report(pkg):
    import torch
    S = pkg.scoring
    a = S.Score(torch.tensor([2.0, 4.0], dtype=torch.float64), torch.tensor([1.0, 1.0], dtype=torch.float64),
                torch.tensor([2, 2]), torch.tensor([1, 0]))
    a.vq_sum, a.frames, a.code_counts = torch.tensor([0.5, 1.5], dtype=torch.float64), torch.tensor([1, 1]), torch.tensor([2, 0, 0, 0])
    b = S.Score(torch.tensor([2.0], dtype=torch.float64), torch.tensor([2.0], dtype=torch.float64), torch.tensor([4]), torch.tensor([3]))
    b.vq_sum, b.frames, b.code_counts = torch.tensor([2.0], dtype=torch.float64), torch.tensor([2]), torch.tensor([0, 2, 0, 0])
    t, u = S.Totals(4), S.Totals(4)
    t.add(a)
    u.add(b)
    t.merge(u)
    r = t.report('sample', latent_dim=2)
    assert r['samples'] == 8 and r['nll'] == 1.0 and r['entropy'] == 0.5 and r['accuracy'] == 0.5
    assert r['bits_per_sample'] == pytest.approx(1.0 / math.log(2.0))
    assert r['vq_loss'] == 0.5 and r['codes_used'] == 2 and r['codes'] == 4 and r['code_perplexity'] == pytest.approx(2.0)
    assert t.rows == 3
    assert a.row_bits() == [pytest.approx(1.0 / math.log(2.0)), pytest.approx(2.0 / math.log(2.0))]


# ------------------------------------------------------------------ C entry points: argument checks
def test_entry_points_refuse_bad_arguments(pkg):
    lib = pkg._lib.lib()
    one = 1 << 12       # never dereferenced: the checks come first
    assert lib.vqw_softmax_score(None, None, None, None, None, None, None, None, None, 0, 1, 4, 64, None) != 0
    assert b'null pointer' in lib.vqw_last_error()
    assert lib.vqw_softmax_score(one, one, None, None, None, None, one, one, one, 4, 1, 6, 64, None) != 0
    assert b'multiple of 4' in lib.vqw_last_error()
    assert lib.vqw_softmax_score(one, one, None, None, None, None, one, one, one, 4, 1, 2048, 64, None) != 0
    assert b'at most 1024' in lib.vqw_last_error()
    assert lib.vqw_softmax_score(one, one, None, None, None, None, one, one, one, 4, 1, 8, 65, None) != 0      # two tiles
    assert b'scratch' in lib.vqw_last_error()
    assert lib.vqw_softmax_score(one, one, None, None, None, None, one, one, one, 4, 0, 8, 64, None) != 0
    assert lib.vqw_code_histogram(None, None, None, None, 1, 1, 1, None) != 0
    assert b'null pointer' in lib.vqw_last_error()
    assert lib.vqw_code_histogram(one, None, one, one, 1, 0, 4, None) != 0
    assert b'bad shape' in lib.vqw_last_error()


def test_wrappers_refuse_cpu_tensors(pkg):
    import torch
    with pytest.raises(ValueError, match='GPU'):
        pkg.kernels.softmax_score(torch.zeros(1, 4, 64), torch.zeros(1, 64, dtype=torch.int32))
    with pytest.raises(ValueError, match='GPU'):
        pkg.kernels.code_histogram(torch.zeros(1, 4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------ command lines
def run(script, *argv, cwd=None):
    # a broken import of the package would show up as a traceback, not as a usage error: the refusals come first
    env = dict(os.environ, PYTHONPATH=ROOT, VQW_LIB_NAME='no_such_library.so')
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(argv), cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=300)


def test_evaluate_cli_refuses_bad_combinations(tmp_path):
    ck, lst = tmp_path / 'w-1.pt', tmp_path / 'l.txt'
    ck.write_bytes(b'')
    lst.write_text('p1/a.wav\n')
    ok = ['-restore', str(ck), '-list', str(lst), '-params', os.path.join(ROOT, 'model_parameters.json')]
    for argv, msg in ((['-list', str(lst)], 'required'), (['-restore', str(ck)], 'required'),
                      (ok + ['-weights', 'best'], 'ema or live'), (ok + ['-length', '100'], 'multiple of 64'),
                      (ok + ['-length', '-64'], 'multiple of 64'), (ok + ['-batch', '0'], 'at least 1'),
                      (ok + ['-dataset', 'synthetic'], '-dataset must be'), (ok + ['-prior_params', 'p.json'], 'needs -prior'),
                      (ok[:3] + [str(tmp_path / 'none.txt')] + ok[4:], 'no such file'),
                      (ok + ['-prior', str(tmp_path / 'none.pt')], 'no such file')):
        r = run('evaluate.py', *argv, cwd=str(tmp_path))
        assert r.returncode == 2 and 'error:' in r.stderr and msg in r.stderr and 'Traceback' not in r.stderr, (argv, r.stderr[-500:])


def test_train_cli_refuses_bad_eval_flags(tmp_path):
    lst = tmp_path / 'l.txt'
    lst.write_text('p1/a.wav\n')
    for argv, msg in ((['-eval_interval', '5'], 'needs -eval_list'), (['-eval_list', str(lst)], 'needs -eval_interval'),
                      (['-eval_list', str(lst), '-eval_interval', '-1'], '>= 0'),
                      (['-eval_list', str(lst), '-eval_interval', '2', '-eval_batches', '0'], '>= 1'),
                      (['-eval_list', str(tmp_path / 'none.txt'), '-eval_interval', '2'], 'no such file'),
                      (['-eval_list', str(lst), '-eval_interval', '2', '-eval_dataset', 'synthetic'], '-eval_dataset must be'),
                      (['-eval_dataset', 'VCTK'], 'needs -eval_list')):
        r = run('train.py', '-dataset', 'synthetic', *argv, cwd=str(tmp_path))
        assert r.returncode == 2 and 'error:' in r.stderr and msg in r.stderr and 'Traceback' not in r.stderr, (argv, r.stderr[-500:])


# ------------------------------------------------------------------ the list reader
def write_dataset(root, lengths, speakers=('p225', 'p226', 'p227')):
    """A VCTK-shaped data root: <root>/vctk_speakers.txt and 16 kHz int16 wavs under <root>/VCTK-Corpus/wav48/<speaker>/."""
    from scipy.io import wavfile
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, 'vctk_speakers.txt'), 'w') as f:
        for i, s in enumerate(speakers):
            f.write('%s, %d\n' % (s, i))
    rels, g = [], np.random.RandomState(5)
    for i, n in enumerate(lengths):
        s = speakers[i % len(speakers)]
        os.makedirs(os.path.join(root, 'VCTK-Corpus', 'wav48', s), exist_ok=True)
        rel = '%s/%s_%03d.wav' % (s, s, i)
        t = np.arange(n) / 16000.0
        pcm = (np.sin(2 * np.pi * (150 + 70 * i) * t) * 9000 + g.randn(n) * 300).astype(np.int16)
        wavfile.write(os.path.join(root, 'VCTK-Corpus', 'wav48', rel), 16000, pcm)
        rels.append(rel)
    return rels


def test_list_reader_order_trim_sort_pad(pkg, tmp_path):
    D = pkg.data
    root = str(tmp_path / 'data')
    rels = write_dataset(root, [1000, 300, 50, 700, 640])
    lst = tmp_path / 'held.txt'
    lst.write_text('\n'.join(rels) + '\n\n')
    held = D.HeldOutList('VCTK', str(lst), relative_path=root, ratio=64)
    assert held.files == rels and held.num_speakers == 3
    utts, skipped = held.utterances()
    assert [u[0] for u in utts] == [rels[0], rels[1], rels[3], rels[4]] and skipped == 1          # file order; 50 < 64 is left out
    assert [len(u[2]) for u in utts] == [960, 256, 640, 640] and [u[1] for u in utts] == [0, 1, 0, 1]
    from scipy.io import wavfile
    pcm = wavfile.read(os.path.join(root, 'VCTK-Corpus', 'wav48', rels[0]))[1]
    np.testing.assert_array_equal(utts[0][2], ((pcm[:960].astype(np.float32) + 0.5) / 32767.5).astype(np.float32))
    batches = list(D.padded_batches(utts, 3, multiple=256))
    assert [b[0] for b in batches] == [[rels[1], rels[3], rels[4]], [rels[0]]]                 # by length, file order among equals
    files, x, spk, lengths = batches[0]
    assert tuple(x.shape) == (3, 768) and lengths == [256, 640, 640] and spk.tolist() == [1, 0, 1]
    assert (x[0, 256:] == 0).all() and (x[1, 640:] == 0).all()
    np.testing.assert_array_equal(x[1, :640].numpy(), utts[2][2])
    assert tuple(batches[1][1].shape) == (1, 1024) and batches[1][3] == [960]
    assert D.padded_length(256) == 256 and D.padded_length(257) == 512 and D.padded_length(640, 1280) == 1280
    crops, short = held.crops(640)
    assert [c[0] for c in crops] == [rels[0], rels[3], rels[4]] and short == 2 and all(len(c[2]) == 640 for c in crops)
    crops, _ = held.crops(256, limit=2)
    assert [c[0] for c in crops] == rels[:2]
    fb = list(D.fixed_batches(held.crops(640)[0], 2))
    assert [tuple(b[1].shape) for b in fb] == [(2, 640), (1, 640)] and fb[0][3] is None and fb[0][2].tolist() == [0, 0]
    with pytest.raises(NotImplementedError):
        D.HeldOutList('synthetic', str(lst), relative_path=root)
