"""The host issues the launches it issued before: every kernel call of forward() + backward() with its arguments, buffer roles,
streams, event edges and grad_sync ranges, recorded on the CPU (tests/launch_trace.py) and held to the digests in
tests/golden/launch_trace.json -- for the three encoders and for every branch of Encoder_64's passes (fp16x3 layers, split-K and
unsplit short layers, plane or register weight gradients, one or two streams, a pass that saves nothing), for the decoder's own
branches (at 2 layers, and at 8 where the backward stack's rings and weight-gradient batches come into play), the latent prior,
train_step and the forward-only passes.  Next to it the facts
checkpoints and the data-parallel bucket ranges rest on: flat-buffer segments and offsets, state_dict keys, reference names."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import launch_trace as LT  # noqa: E402

with open(LT.GOLDEN) as f:
    GOLDEN = json.load(f)


def test_golden_file_covers_the_cases():
    assert sorted(GOLDEN['cases']) == sorted(LT.CASES) and sorted(GOLDEN['layouts']) == sorted(LT.LAYOUTS)


@pytest.mark.parametrize('name', list(LT.CASES))
def test_launches_are_the_golden_ones(pkg, name):
    want = GOLDEN['cases'][name]
    with pytest.MonkeyPatch.context() as mp:
        trace = LT.run_case(mp, pkg, name)
    assert [e[0] for e in trace] == want['calls'] if 'calls' in want else len(trace) == want['entries']
    assert LT.digest(trace) == want['sha256'], 'same calls, other arguments / buffers / streams: python tests/launch_trace.py --dump %s' % name


@pytest.mark.parametrize('name', ['enc64', 'magenta', '2019', 'enc64-grad-sync', 'train-step-deferred', 'train-step-deferred-flagged', 'deep',
                                  'deep-wgrad-batch-0'])
def test_a_second_run_gives_the_same_trace(pkg, name):
    digests = []
    for _ in range(2):
        with pytest.MonkeyPatch.context() as mp:
            digests.append(LT.digest(LT.run_case(mp, pkg, name)))
    assert digests[0] == digests[1] == GOLDEN['cases'][name]['sha256']


def test_the_cases_reach_the_branches_they_are_named_for(pkg):
    """(so that a golden file made again from other shapes cannot quietly stop covering a branch)"""
    def traced(name):
        with pytest.MonkeyPatch.context() as mp:
            return LT.run_case(mp, pkg, name)
    names = lambda t: [e[0] for e in t]                                    # noqa: E731
    base = traced('enc64')
    assert names(base).count('f16x3_strided_conv') == 2                    # layer 1: forward and input gradient
    assert sum(1 for e in base if e[0] == 'conv_gemm' and e[2].get('split_k', 0) > 1) == 4     # layers 2..5 forward
    assert any(e[0] == 'f16x3_wgrad' and 'p_planes' in e[3] and 'p_tap_chunk' in e[2] for e in base)
    assert {e[1] for e in base} == {'main', 'side1'}
    assert {e[1] for e in traced('enc64-overlap-0')} == {'main'}
    assert 'f16x3_strided_conv' not in names(traced('enc64-enc-x3-0')) and 'f16x3_strided_conv' not in names(traced('enc64-fp32-repeat'))
    assert not any('p_tap_chunk' in e[2] for e in traced('enc64-wgrad-pp-0'))
    assert not any('split_slab' in e[3] for e in traced('enc64-sconv-split-0')) and any('split_slab' in e[3] for e in base)
    unsplit = traced('enc64-unsplit')
    fwd = [e[2].get('split_k', 0) for e in unsplit if e[0] == 'conv_gemm' and e[2].get('in_stride') == 2]
    bwd = [e[2].get('split_k', 0) for e in unsplit if e[0] == 'conv_gemm' and e[2].get('out_tstride') == 2]
    assert fwd[:2] == [0, 2] and bwd[-2:] == [0, 0] and bwd[-4:-2] == [-2, -2]     # layer 1 in one piece, layer 2 in two, both ways
    ranges = [(e[2]['lo'], e[2]['hi']) for e in traced('enc64-grad-sync') if e[0] == 'grad_sync.bucket_ready']
    assert len(ranges) == 7 and ranges[0][1] > ranges[0][0] and sorted(ranges)[0][0] == 0
    assert not any(e[3].get('save_r') or e[3].get('save0') for e in traced('enc64-encode-nosave'))
    # the decoder's branches, the prior and the step
    prior = names(traced('prior'))
    assert 'prior_input_fwd' in prior and 'prior_input_wgrad' in prior
    assert not {'vq_nearest_fwd', 'relu_bn_fwd', 'wavenet_inputs'} & set(prior)
    assert 'f16x3_wgrad_batch' in names(base) and 'f16x3_wgrad_batch' not in names(traced('dec-wgrad-batch-0'))
    in_stack = lambda t: [e for e in t if e[0] == 'wgrad_gemm' and e[2]['taps'] == [-2, -1, 0]]      # noqa: E731  (layer 1's gate kernel)
    assert in_stack(traced('dec-wgrad-x3-0')) and not in_stack(base)
    assert any(e[0] == 'conv_gemm' and e[2].get('in_relu') for e in traced('dec-head-x3-0'))
    assert not any(e[0] == 'conv_gemm' and e[2].get('in_relu') for e in base)
    ladder = [traced('dec-ladder-%d' % n) for n in (1, 2, 3, 4, 5)]
    assert len({LT.digest(t) for t in ladder}) == 5 and 'f16x3_out_conv' not in names(ladder[0]) and 'f16x3_out_conv' in names(ladder[1])
    assert 'f16x3_amax' in names(base) and 'f16x3_amax' not in names(traced('dec-bf16'))
    jitter = names(traced('train-step-jitter-ema'))
    assert {'time_jitter_fwd', 'time_jitter_bwd', 'vq_cluster_stats', 'vq_codebook_ema_step'} <= set(jitter)
    assert not {'time_jitter_fwd', 'vq_cluster_stats', 'vq_codebook_ema_step'} & set(names(traced('train-step')))
    # the deferred range flag: a voided step is repeated on the fp32 engine (the stack's wgrad_gemm; the encoder's short layers
    # use that kernel on either engine), once: the second step runs again on the plane engine; a clean one is not
    flagged = traced('train-step-deferred-flagged')
    assert len(in_stack(flagged)) == 1 and not in_stack(traced('train-step-deferred'))
    # a refused length: the only plane-engine calls are the encoder's (its kernels alone, and none once its engine layers are off)
    refused = {e[0] for e in traced('dec-refused-length') if e[0].startswith('f16x3_')}
    assert 'f16x3_strided_conv' in refused and not refused & {'f16x3_gate_conv', 'f16x3_out_conv', 'f16x3_pack_gate_weights', 'f16x3_wgrad_batch'}
    assert not any(n.startswith('f16x3_') for n in names(traced('dec-refused-length-enc-x3-0')))
    # the deep stack: what 2 layers never reach.  Per-layer weight gradients on a side stream: the chain waits for the rings ...
    waits = lambda t: sum(1 for e in t if e[0] == 'wait_event' and e[1] == 'main')      # noqa: E731
    deep = {name: traced(name) for name in LT.CASES if name.startswith('deep')}
    for name in ('deep-wgrad-batch-0', 'deep-engine-fp32', 'deep-wgrad-x3-0'):
        assert waits(deep[name]) == 6, name                                # layers 5..0 of 8: two layers ahead, then one wait per layer
    assert not any(waits(traced(name)) for name in LT.CASES if name not in deep)
    assert waits(deep['deep']) == 0 and not waits(deep['deep-wgrad-batch-0-overlap-0'])
    # ... batches that fill and flush inside the loop, on both tap-alignment classes (dilations 1, 2 / 4, 8)
    batches = lambda t: [e for e in t if e[0] == 'f16x3_wgrad_batch']                  # noqa: E731
    assert len(batches(deep['deep'])) == 4 and len(batches(deep['deep-wg-batches-2-3'])) == 8
    gate_taps = {tuple(p['taps']) for e in batches(deep['deep-wg-batches-2-3']) for p in e[3]['problems'] if 'taps' in p}
    assert {taps for taps in gate_taps if any(s % 4 for s in taps)} and {taps for taps in gate_taps if not any(s % 4 for s in taps)}
    assert names(deep['deep-wgrad-batch-0']).count('f16x3_wgrad') == 20
    assert names(deep['deep-engine-fp32']).count('wgrad_gemm') == 25
    # ... one stream: no event, nothing on a side stream
    for name in ('deep-wgrad-batch-0-overlap-0', 'deep-overlap-0'):
        assert {e[1] for e in deep[name]} == {'main'} and 'record' not in names(deep[name]), name
    assert batches(deep['deep-overlap-0']) and not batches(deep['deep-wgrad-batch-0-overlap-0'])
    # ... the gate kernels' q operand: the planes gate backward wrote (qp), or fp32 dpre
    gate_probs = lambda t: [p for e in batches(t) if e[2]['Q0'] == 512 and 'seg_T' in e[2] for p in e[3]['problems']]     # noqa: E731
    assert len(gate_probs(deep['deep'])) == 8 and all('q_planes' in p and 'q0' not in p for p in gate_probs(deep['deep']))
    assert len(gate_probs(deep['deep-wgrad-qp-0'])) == 8 and all('q0' in p and 'q_planes' not in p for p in gate_probs(deep['deep-wgrad-qp-0']))
    assert names(deep['deep-fp32-repeat']).count('f16x3_amax') > names(deep['deep-engine-fp32']).count('f16x3_amax') + 8      # (the calibrating repeat: per layer)
    assert len({LT.digest(t) for t in deep.values()}) == len(deep)


@pytest.mark.parametrize('name', list(LT.LAYOUTS))
def test_layout_state_dict_and_reference_names(pkg, name):
    with pytest.MonkeyPatch.context() as mp:
        got = LT.layout_facts(mp, pkg, name)
    want = GOLDEN['layouts'][name]
    if list(want) == ['sha256']:
        assert LT.digest(got) == want['sha256'], 'python tests/launch_trace.py --dump %s' % name
        return
    for key in want:
        assert got[key] == want[key], key
    assert sorted(got) == sorted(want)
