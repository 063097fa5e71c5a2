"""CPU tests of the latent prior over VQ codes (prior.py): config loading and its refusals, the parameter inventory under
the scope prior/, and the new command-line flags.  No GPU: the model is built on the CPU device only where nothing
launches a kernel."""
import copy
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_prior(k=32, pre_k=3):
    return {"quantization_channels": k, "num_cycles": 2, "num_cycle_layers": 4, "dilation_rates": [1, 2, 4, 8, 1, 2, 4, 8],
            "kernel_size": 3, "dilation_filters": 32, "skip_filters": 64, "residual_filters": 32,
            "preprocess": {"kernel_size": pre_k, "filters": 32}, "speaker_embedding": 16, "learning_rate_schedule": {"0": 1e-3}}


def vqvae_cfg(k=512, encoder='64'):
    with open(os.path.join(ROOT, 'model_parameters.json')) as f:
        m = json.load(f)
    m['k'], m['encoder'] = k, encoder
    return m


def test_default_config_loads_against_the_default_vqvae(pkg):
    cfg = pkg.prior.load_prior_config(os.path.join(ROOT, 'prior_parameters.json'), vqvae_cfg())
    assert cfg['quantization_channels'] == 512
    assert cfg['residual_filters'] == 256 and cfg['skip_filters'] == 512 and cfg['kernel_size'] == 3
    assert cfg['dilation_rates'] == [2 ** i for i in range(10)] * 2 and cfg['num_cycles'] == 2
    assert cfg['preprocess'] == {'kernel_size': 1, 'filters': 256} and cfg['speaker_embedding'] == 64
    assert 'learning_rate_schedule' in cfg
    for n in (cfg['residual_filters'], cfg['skip_filters'], cfg['quantization_channels']):
        assert n % 256 == 0          # the fp16x3 engine's widths


def test_config_refusals(pkg, tmp_path):
    path = tmp_path / 'p.json'
    path.write_text(json.dumps(tiny_prior(k=32)))
    with pytest.raises(ValueError, match='codebook size'):
        pkg.prior.load_prior_config(str(path), vqvae_cfg(k=64))            # k mismatch
    for enc in ('Magenta', '2019'):
        with pytest.raises(ValueError, match='one code per 64 samples'):
            pkg.prior.load_prior_config(str(path), vqvae_cfg(k=32, encoder=enc))
    novq = vqvae_cfg(k=32)
    novq['use_vq'] = False
    with pytest.raises(ValueError, match='no codebook'):
        pkg.prior.load_prior_config(str(path), novq)
    bad = tiny_prior()
    bad['num_cycles'] = 3
    with pytest.raises(ValueError, match='dilation rates'):
        pkg.prior.check_prior_config(bad)
    bad = tiny_prior()
    del bad['speaker_embedding']
    with pytest.raises(ValueError, match='speaker_embedding'):
        pkg.prior.check_prior_config(bad)
    with pytest.raises(ValueError, match='codebook size'):
        pkg.prior.LatentPrior(tiny_prior(k=32), 10, device='cpu', n_codes=64)
    assert pkg.prior.load_prior_config(str(path), vqvae_cfg(k=32))['quantization_channels'] == 32


def test_length_must_be_whole_condition_frames(pkg):
    prior = pkg.prior.LatentPrior(tiny_prior(), 10, device='cpu')
    with pytest.raises(ValueError, match='multiple of 64'):
        prior._front_workspace(2, 500, True)
    ws = prior._front_workspace(2, 512, False)
    assert ws['Tz'] == 8 and ws['ratio'] == 64 and tuple(ws['cond'].shape) == (2, 16, 8)


@pytest.mark.parametrize('spk_emb', [16, 0])
def test_parameter_inventory(pkg, spk_emb):
    cfg = tiny_prior(k=32, pre_k=3)
    cfg['speaker_embedding'] = spk_emb
    prior = pkg.prior.LatentPrior(cfg, 10, device='cpu')
    named = prior.named_parameters()
    assert all(n.startswith('prior/') for n in named)
    shapes = {n: tuple(v.shape) for n, v in named.items()}
    Cc = 16 if spk_emb else 10
    want = {'prior/preprocess/kernel': (3, 32, 32), 'prior/preprocess/bias': (32,), 'prior/skip/kernel': (1, 32, 64),
            'prior/skip/bias': (64,), 'prior/postprocess1/kernel': (1, 64, 64), 'prior/postprocess1/bias': (64,),
            'prior/postprocess1/local_condition/kernel': (1, Cc, 64), 'prior/postprocess2/kernel': (1, 64, 32),
            'prior/postprocess2/bias': (32,)}
    if spk_emb:
        want['prior/speaker_embedding'] = (10, 16)
    for c in (1, 2):
        for l in (1, 2, 3, 4):
            s = 'prior/cycle_%d/layer_%d/' % (c, l)
            want.update({s + 'gated/kernel': (3, 32, 64), s + 'gated/bias': (64,), s + 'gated/local_condition/kernel': (1, Cc, 64),
                         s + 'skip/kernel': (1, 32, 64), s + 'skip/bias': (64,), s + 'residual/kernel': (1, 32, 32),
                         s + 'residual/bias': (32,)})
    assert shapes == want
    assert not any('encoder' in n or 'embedding/embedding' in n or 'decoder' in n for n in named)
    # load_named round trip under the same names
    other = pkg.prior.LatentPrior(cfg, 10, device='cpu', seed=5)
    other.load_named(named)
    assert all((other.named_parameters()[n] == v).all() for n, v in named.items())
    assert prior.state_dict()['flat'].numel() == prior.n_flat


def test_state_dict_has_no_batchnorm_statistics_and_loads_files_that_do(pkg):
    """A prior is a WaveNet, not a VQ-VAE: no BatchNorm buffers, none of the VQ-VAE's front.  Its state_dict is the WaveNet's;
    load_state_dict takes it, and takes a file written when a prior still carried two zero-length bn_mean / bn_var tensors."""
    import torch
    prior = pkg.prior.LatentPrior(tiny_prior(), 10, device='cpu', seed=1)
    for name in ('bn_mean', 'bn_var', 'time_jitter', 'codebook_ema', 'codebook_restart', 'encode', 'encode_codes', 'summaries', 'encoder'):
        assert not hasattr(prior, name), name
    prior.global_step = 7
    prior.adam_m.fill_(0.25)
    prior.x3_scale.mul_(2.0)
    sd = prior.state_dict()
    assert list(sd) == ['flat', 'ema', 'adam_m', 'adam_v', 'x3_scale', 'global_step']
    old = dict(sd, bn_mean=torch.zeros(0), bn_var=torch.ones(0))          # a file from before
    for state in (sd, old):
        other = pkg.prior.LatentPrior(tiny_prior(), 10, device='cpu', seed=2)
        assert not torch.equal(other.flat, prior.flat)
        other.load_state_dict({k: v.clone() for k, v in state.items()})
        assert other.global_step == 7
        for k in ('flat', 'ema', 'adam_m', 'adam_v', 'x3_scale'):
            assert torch.equal(getattr(other, k), getattr(prior, k)), k
        assert list(other.state_dict()) == list(sd)


def test_vqvae_inventory_unchanged_by_the_hooks(pkg):
    """The decoder's hooks are pure moves: VQVAE's names, order and shapes are what they were."""
    m = vqvae_cfg(k=32)
    m.update(latent_dim=16, speaker_embedding=16, encoder_filters=48)
    w = copy.deepcopy(tiny_prior())
    w['quantization_channels'] = 256
    w['preprocess'] = {'kernel_size': 32, 'filters': 32}
    model = pkg.model.VQVAE(m, w, 10, device='cpu')
    names = list(model.named_parameters())
    assert names[0] == 'speaker_embedding' and names[1] == 'encoder/conv1d/kernel'
    assert 'embedding/embedding' in names and 'decoder/preprocess/kernel' in names
    assert tuple(model.named_parameters()['decoder/preprocess/kernel'].shape) == (32, 1, 32)
    assert names[-1] == 'decoder/postprocess2/bias'


@pytest.mark.parametrize('script,flags', [
    ('train_prior.py', ['-restore', '-dataset', '-length', '-batch', '-step', '-interval', '-save', '-params', '-vqvae_params']),
    ('generate.py', ['-prior', '-frames', '-prior_params', '-audio', '-restore', '-speakers', '-mode']),
])
def test_cli_help_shows_the_new_flags(script, flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, script), '-h'], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    for f in flags:
        assert f in out.stdout, (script, f)


def test_train_prior_refuses_multiple_ranks(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train_prior.py'), '-restore', 'x.pt', '-dataset', 'synthetic'],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path),
                         env=dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE='2'))
    assert out.returncode != 0 and 'one GPU' in out.stderr
