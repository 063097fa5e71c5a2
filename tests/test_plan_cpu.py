"""VQVAE._step_plan: which engine carries which contraction of a step, as a pure function of the model's constants, the switches
read at construction (model.sw) and (B, T, Tz, save, active).  The rows are what the forward and the backward pass each derived
for themselves before there was one plan; the invariants are the two consistency errors the backward pass used to raise.
Reference widths (R 256, S 512, Q 256, 30 layers, ks 3, encoder_filters 768), device='cpu': no tensor of the model is touched,
so the weights' initialisation is skipped."""
import itertools

import pytest

from oracle import ref_model as M

SWITCHES = ('VQW_ENGINE', 'VQW_GATE_F16X3', 'VQW_DTYPE', 'VQW_WGRAD_BATCH', 'VQW_WGRAD_QP', 'VQW_WGRAD_PP', 'VQW_HEAD_X3', 'VQW_SAVE_TANH',
            'VQW_SAVE_GATED', 'VQW_SKIP_GROUPS', 'VQW_WGRAD_X3', 'VQW_ENC_X3', 'VQW_ENC_WGRAD_X3', 'VQW_WG_GATE_BATCH', 'VQW_WG_RES_BATCH')
FWD = ('f16x3', 'f16x3_out', 'f16x3_skip')
ENGINE = FWD + ('x3_used', 'gd', 'dgrad_x3', 'gbwd_x3', 'wg_x3', 'head_x3')
EXTRAS = ('keep_xp', 'drop_th', 'drop_g', 'batched', 'qp', 'pp', 'enc_wg3')


@pytest.fixture
def build(pkg, monkeypatch):
    """build(VQW_X='..', ...): a model constructed under exactly these switches (set BEFORE construction: they are read there)."""
    monkeypatch.setattr(pkg.model.VQVAE, '_init_params', lambda self, seed: None)      # (35 M weights that no plan reads)

    def make(**env):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model = pkg.model.VQVAE(dict(M.DEFAULT_MODEL), dict(M.DEFAULT_WAVENET), 109, device='cpu', seed=0)
        assert (model.R, model.S, model.Q, model.L, model.ks, model.F) == (256, 512, 256, 30, 3, 768)
        return model
    return make


def flags(plan, names):
    return {n: getattr(plan, n) for n in names}


def all_of(names, value):
    return dict.fromkeys(names, value)


def test_default_switches(build):
    p = build()._step_plan(1, 1024, 16, True, True)
    assert flags(p, ENGINE + EXTRAS) == all_of(ENGINE + EXTRAS, True)
    assert (p.ngrp, p.gate_batch, p.res_batch, p.WS, p.GS, p.GSh) == (1, 6, 29, 1.0, 1.0, 1.0)
    assert p.enc_x3 == (1,)               # layer 1 has B * T_out = 256 columns, layer 2 has 128
    assert p.save is True and p.calib is False and p.why is None


def test_plan_of_a_real_model_is_the_same(pkg, monkeypatch, build):
    stub = build()._step_plan(1, 1024, 16, True, True)
    monkeypatch.undo()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    model = pkg.model.VQVAE(dict(M.DEFAULT_MODEL), dict(M.DEFAULT_WAVENET), 109, device='cpu', seed=0)
    assert model._step_plan(1, 1024, 16, True, True) == stub


def test_fp32_repeat_of_a_guarded_step(build):
    p = build()._step_plan(1, 1024, 16, True, False)
    assert flags(p, ENGINE + EXTRAS) == all_of(ENGINE + EXTRAS, False)
    assert p.calib is True and p.enc_x3 == () and p.why is None and (p.WS, p.GS) == (256.0, 2.0 ** 20)


def test_length_that_is_no_multiple_of_256(build):
    p = build()._step_plan(1, 960, 15, True, True)
    assert flags(p, ENGINE + EXTRAS) == all_of(ENGINE + EXTRAS, False)
    assert p.calib is False and p.enc_x3 == () and '960' in p.why and 'multiple of 256' in p.why
    assert build()._step_plan(8, 960, 15, True, True).enc_x3 == (1, 2, 3)   # (the encoder's layers do not follow the decoder's shape rules)


def test_fp32_engine(build):
    model = build(VQW_ENGINE='fp32')
    for active in (True, False):
        p = model._step_plan(1, 1024, 16, True, active)
        assert flags(p, ENGINE + EXTRAS) == all_of(ENGINE + EXTRAS, False)
        assert p.calib is False and p.enc_x3 == () and p.why is None


def test_bf16_engine(build):
    p = build(VQW_DTYPE='bf16')._step_plan(1, 1024, 16, True, True)
    assert flags(p, ENGINE) == dict(all_of(ENGINE, True), gd=False)
    assert flags(p, EXTRAS) == dict(all_of(EXTRAS, True), drop_g=False, enc_wg3=False)
    assert (p.WS, p.GS, p.GSh) == (256.0, 2.0 ** 20, 2.0 ** 20) and p.enc_x3 == () and p.calib is False


@pytest.mark.parametrize('level', [1, 2, 3, 4, 5])
def test_development_ladder(build, level):
    model = build(VQW_GATE_F16X3=str(level))
    assert not model.x3_guard and not model.x3_all
    for active in (True, False):         # (the ladder has no fp32 repeat: nothing depends on it)
        p = model._step_plan(1, 1024, 16, True, active)
        assert flags(p, ENGINE) == dict(all_of(ENGINE, False), f16x3=True, f16x3_out=level >= 2, f16x3_skip=level >= 3,
                                        dgrad_x3=level >= 4, gbwd_x3=level >= 5)
        assert flags(p, EXTRAS) == all_of(EXTRAS, False)
        assert (p.WS, p.GS) == (256.0, 2.0 ** 20) and p.enc_x3 == () and p.calib is False and p.why is None


def test_weight_gradients_one_layer_per_launch(build):
    p = build(VQW_WGRAD_BATCH='0')._step_plan(1, 1024, 16, True, True)
    assert flags(p, ENGINE) == all_of(ENGINE, True)
    assert flags(p, EXTRAS) == dict(all_of(EXTRAS, True), batched=False, qp=False, pp=False, drop_g=False)
    assert p.enc_x3 == (1,)


def test_single_switches(build):
    """Rows read off the derivations the two passes had: keep_xp wanted the per-layer planes (VQW_WGRAD_PP), drop_g wanted keep_xp
    and drop_th, the encoder's weight gradients wanted the slab that the head OR the decoder's weight gradients make."""
    shape = (1, 1024, 16, True, True)
    p = build(VQW_WGRAD_PP='0')._step_plan(*shape)
    assert flags(p, ENGINE) == all_of(ENGINE, True)
    assert flags(p, EXTRAS) == dict(all_of(EXTRAS, True), keep_xp=False, pp=False, drop_g=False)
    p = build(VQW_SAVE_TANH='1')._step_plan(*shape)
    assert flags(p, ENGINE + EXTRAS) == dict(all_of(ENGINE + EXTRAS, True), drop_th=False, drop_g=False)
    p = build(VQW_SAVE_GATED='1')._step_plan(*shape)
    assert flags(p, ENGINE + EXTRAS) == dict(all_of(ENGINE + EXTRAS, True), drop_g=False)
    p = build(VQW_HEAD_X3='0')._step_plan(*shape)
    assert flags(p, ENGINE + EXTRAS) == dict(all_of(ENGINE + EXTRAS, True), head_x3=False)
    p = build(VQW_WGRAD_QP='0')._step_plan(*shape)
    assert flags(p, ENGINE + EXTRAS) == dict(all_of(ENGINE + EXTRAS, True), qp=False)
    # nothing makes the slab.  (Here the forward pass used to leave the fp32 gated output out and the backward pass, which needed it
    # for its fp32-operand weight gradients, raised: in the one plan drop_g follows pp, the step runs and stores it.)
    p = build(VQW_HEAD_X3='0', VQW_WGRAD_X3='0')._step_plan(*shape)
    assert not (p.wg_x3 or p.batched or p.qp or p.pp or p.drop_g or p.enc_wg3) and p.drop_th and p.keep_xp and p.gbwd_x3
    assert build(VQW_ENC_X3='0')._step_plan(*shape).enc_x3 == () and build(VQW_ENC_WGRAD_X3='0')._step_plan(*shape).enc_wg3 is False
    p = build(VQW_WG_GATE_BATCH='100', VQW_WG_RES_BATCH='0')._step_plan(*shape)
    assert (p.gate_batch, p.res_batch) == (32, 1)                            # clamped to [1, kernels.WGRAD_MAX_BATCH]


def test_scoring_pass(build):
    p = build()._step_plan(1, 1024, 16, False, True)
    assert p.save is False and p.head_x3 is True and p.x3_used is True and p.drop_th is True
    assert (p.keep_xp, p.drop_g, p.pp) == (False, False, False) and p.enc_x3 == ()


def test_skip_groups_at_large_shapes(build):
    model = build()
    assert model._step_plan(16, 6656, 104, True, True).ngrp == 1
    assert model._step_plan(32, 6656, 104, True, True).ngrp == 2
    assert build(VQW_SKIP_GROUPS='3')._step_plan(16, 1024, 16, True, True).ngrp == 3


def test_switches_are_read_at_construction_only(build, monkeypatch):
    model = build()
    before = model._step_plan(1, 1024, 16, True, True)
    for k, v in (('VQW_ENGINE', 'fp32'), ('VQW_WGRAD_BATCH', '0'), ('VQW_SKIP_GROUPS', '3'), ('VQW_SAVE_TANH', '1'), ('VQW_ENC_X3', '0')):
        monkeypatch.setenv(k, v)
    assert model._step_plan(1, 1024, 16, True, True) == before
    assert model.sw.engine == 'f16x3' and model.sw.wgrad_batch is True and model.sw.skip_groups == 1


def test_plan_is_cached_per_workspace_save_and_engine_state(build):
    model = build()
    ws = {'B': 1, 'T': 1024, 'Tz': 16}
    a = model._plan(ws, True)
    assert model._plan(ws, True) is a and model._plan(ws, False) is not a and model._plan(ws, False).save is False
    model._x3_active = False
    b = model._plan(ws, True)
    assert b.calib and not b.x3_used and model._plan(ws, True) is b
    model._x3_active = True
    assert model._plan(ws, True) is a


ENGINES = [dict(VQW_ENGINE='fp32'), dict(VQW_ENGINE='f16x3'), dict(VQW_DTYPE='bf16')] + [dict(VQW_GATE_F16X3=str(i)) for i in range(1, 6)]


@pytest.mark.parametrize('engine', ENGINES, ids=lambda e: '-'.join(e.values()))
def test_invariants(build, engine):
    """What the backward pass used to check against the forward pass's flags (and raise): a tensor the forward pass did not
    store is one the backward pass does not read."""
    names = ('VQW_WGRAD_BATCH', 'VQW_WGRAD_QP', 'VQW_WGRAD_PP', 'VQW_HEAD_X3', 'VQW_SAVE_TANH', 'VQW_SAVE_GATED')
    for values in itertools.product('01', repeat=len(names)):
        model = build(**engine, **dict(zip(names, values)))
        for T, save, active in itertools.product((960, 1024), (True, False), (True, False)):
            p = model._step_plan(1, T, T // 64, save, active)
            what = (engine, values, T, save, active, p)
            assert not p.drop_th or p.gbwd_x3, what
            assert not p.drop_g or (p.pp and p.gbwd_x3), what
            assert not p.head_x3 or p.x3_used, what
            if model.x3_all:
                assert p.f16x3 == p.f16x3_out == p.f16x3_skip, what
            assert all(isinstance(getattr(p, n), bool) for n in ENGINE + EXTRAS + ('calib', 'save')), what
