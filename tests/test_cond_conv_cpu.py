"""CPU tests of the conditioning conv's host logic: the configuration keys and their refusals, the condition's
widths, the variables under the reference's names, and a state of one setting refused by a model of the other."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_model_gpu import tiny_cfg  # noqa: E402

NAMES = ('decoder/condition_conv/kernel', 'decoder/condition_conv/bias')


def model(pkg, **keys):
    m, w = tiny_cfg()
    return pkg.model.VQVAE(dict(m, **keys), w, 10, device='cpu', seed=0)


@pytest.mark.parametrize('keys,word', [
    ({'condition_conv': 8}, "'condition_conv'"), ({'condition_conv': 24}, "'condition_conv'"), ({'condition_conv': -16}, "'condition_conv'"),
    ({'condition_conv': 16.0}, "'condition_conv'"), ({'condition_conv': True}, "'condition_conv'"), ({'condition_conv': '16'}, "'condition_conv'"),
    ({'condition_conv': 16, 'condition_conv_kernel': 2}, "'condition_conv_kernel'"), ({'condition_conv': 16, 'condition_conv_kernel': 9}, "'condition_conv_kernel'"),
    ({'condition_conv': 16, 'condition_conv_kernel': 0}, "'condition_conv_kernel'"), ({'condition_conv': 16, 'condition_conv_kernel': -1}, "'condition_conv_kernel'"),
    ({'condition_conv': 16, 'condition_conv_kernel': 3.0}, "'condition_conv_kernel'")])
def test_bad_keys_are_refused_by_name_before_anything_is_allocated(pkg, keys, word):
    VQVAE = pkg.model.VQVAE
    m, w = tiny_cfg()
    probe = VQVAE.__new__(VQVAE)
    with pytest.raises(ValueError, match=word):
        probe._setup_front(dict(m, **keys), 10)          # the first thing the constructor does with the configuration
    assert not hasattr(probe, 'flat') and not hasattr(probe, 'encoder')
    with pytest.raises(ValueError, match=word):
        VQVAE(dict(m, **keys), w, 10, device='cpu')


def test_keys_and_defaults(pkg):
    cfg = pkg.model.cond_conv_config
    assert cfg({}) == (0, 3) and cfg({'condition_conv': 0}) == (0, 3) and cfg({'condition_conv': 128}) == (128, 3)
    assert [cfg({'condition_conv': 16, 'condition_conv_kernel': k}) for k in (1, 3, 5, 7)] == [(16, 1), (16, 3), (16, 5), (16, 7)]


def test_condition_widths(pkg):
    """Dc = C with the conv, D without; Cc = Dc + the speaker rows (one-hot speakers: padded to 16), Cc_ref the reference's."""
    m, _ = tiny_cfg()
    D, Cs = m['latent_dim'], m['speaker_embedding']
    off, on = model(pkg), model(pkg, condition_conv=48)
    assert (off.Dc, off.Cc, off.Cc_ref, off.cconv) == (D, D + Cs, D + Cs, 0)
    assert (on.D, on.Dc, on.Cc, on.Cc_ref, on.cconv, on.cconv_k) == (D, 48, 48 + Cs, 48 + Cs, 48, 3)
    hot_off, hot_on = model(pkg, speaker_embedding=0), model(pkg, speaker_embedding=0, condition_conv=32, condition_conv_kernel=5)
    assert (hot_off.Dc, hot_off.Cc, hot_off.Cc_ref) == (D, D + 16, D + 10)
    assert (hot_on.Dc, hot_on.Cc, hot_on.Cc_ref, hot_on.cconv_k) == (32, 32 + 16, 32 + 10, 5)
    # the projections' own kernels take Cc <= 128 (wavenet.py); a wider condition runs them on the fp32 conv engine
    assert on.cond_proj and not model(pkg, condition_conv=128).cond_proj


def test_names_shapes_and_initial_values(pkg):
    m, _ = tiny_cfg()
    off, on = model(pkg), model(pkg, condition_conv=32, condition_conv_kernel=5)
    assert not any('condition_conv' in n for n in off.named_parameters()) and not any('condition_conv' in n for n in off.seg_off)
    named = on.named_parameters()
    assert tuple(named[NAMES[0]].shape) == (5, m['latent_dim'], 32) and tuple(named[NAMES[1]].shape) == (32,)
    order = list(on.seg_off)
    assert order[order.index('embedding') + 1:][:2] == ['condition_conv_w', 'condition_conv_b']
    lim = (6.0 / (5 * m['latent_dim'] + 5 * 32)) ** 0.5          # Keras glorot_uniform over [k, Cin, Cout]; bias zero
    kernel = named[NAMES[0]]
    assert 0.9 * lim < float(kernel.abs().max()) <= lim and abs(float(kernel.mean())) < 0.1 * lim and not bool(named[NAMES[1]].any())
    assert tuple(named['decoder/postprocess1/local_condition/kernel'].shape)[1] == on.Cc_ref
    for n in NAMES:
        assert n in on.named_parameters(ema=True) and n in on.named_gradients()
    # the front's other variables start exactly as they do without the key (the new draw comes after theirs)
    assert torch.equal(off.P['embedding'], on.P['embedding']) and torch.equal(off.P['speaker_embedding'], on.P['speaker_embedding'])


def test_state_of_one_setting_is_refused_by_the_other(pkg, tmp_path):
    off, on, on5 = model(pkg), model(pkg, condition_conv=32), model(pkg, condition_conv=32, condition_conv_kernel=5)
    assert 'condition_conv' not in off.state_dict() and on.state_dict()['condition_conv'].tolist() == [32, 3]
    for a, b in ((off, on), (on, off), (on, on5), (on, model(pkg, condition_conv=48))):
        before = a.flat.clone()
        with pytest.raises(ValueError, match="'condition_conv'"):
            a.load_state_dict(b.state_dict())
        assert torch.equal(a.flat, before)
    on.load_state_dict(model(pkg, condition_conv=32).state_dict())
    off.load_state_dict(model(pkg).state_dict())
    # the same through a file of reference names
    ck = pkg.checkpoint
    ck.save(on, str(tmp_path / 'on.safetensors'))
    ck.save(off, str(tmp_path / 'off.safetensors'))
    for a, f in ((off, 'on'), (on, 'off')):
        with pytest.raises(ValueError, match="'condition_conv'"):
            ck.load(a, str(tmp_path / (f + '.safetensors')))
    ck.load(on, str(tmp_path / 'on.safetensors'))
    ck.load(off, str(tmp_path / 'off.safetensors'))


def test_front_end_needs_gpu_tensors(pkg):
    K = pkg.kernels
    z, w, b, o = torch.zeros(1, 2, 3), torch.zeros(3, 2, 16), torch.zeros(16), torch.zeros(1, 16, 3)
    with pytest.raises(ValueError, match='GPU'):
        K.cond_conv_fwd(z, w, b, o)
    with pytest.raises(ValueError, match='GPU'):
        K.cond_conv_dgrad(w, o, z)
    with pytest.raises(ValueError, match='GPU'):
        K.cond_conv_wgrad(z, o, w.clone(), b.clone(), torch.zeros(1000))
    assert K.cond_conv_wgrad_scratch(8, 64, 128, 104, 3) == 16 * (3 * 64 * 128 + 128)          # (needs no GPU: a size)
    assert K.cond_conv_wgrad_scratch(1, 4, 16, 1, 3) == 1 * (3 * 4 * 16 + 16)
    with pytest.raises(RuntimeError, match='multiple of 16'):
        K.cond_conv_wgrad_scratch(1, 4, 8, 1, 3)
