"""tests/adapter_postln_ref.py against torch's own float64 post-LN encoder and autograd, the reference fixture against the
restatement, the checks of the GPU tests against planted faults, and the CPU-side surface of the feature (the post-LN
adapter constructs with the reference's keys, the bindings carry the layout and the max code).  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_postln_ref as pr  # noqa: E402
import fewshot_ref as fr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'adapter_postln.npz')
# (B, T, (D, d, heads, ffn), layers, p, residual): small enough for the fp32 restatement's index-order sums
SMALL = ((3, 5, (16, 8, 2, 12), 2, 0.0, 0.5), (2, 4, (12, 8, 1, 20), 1, 0.3, 0.8), (3, 3, (8, 8, 2, 4), 3, 0.0, 0.0))


def _setup(case, seed=0):
    B, T, (D, d, heads, ffn), layers, p, r = case
    top, blocks = fr.adapter_params(D, d, heads, ffn, layers, seed)
    img, valid, d_out = fr.adapter_inputs(B, T, D)
    return top, blocks, img, valid, d_out, heads, p, r


@pytest.mark.parametrize('case', [c for c in SMALL if c[4] == 0] + [(3, 5, (64, 32, 4, 48), 2, 0.0, 0.5)], ids=str)
def test_restatement_matches_torch_float64_module(case):
    """Forward on EVERY row (padded views included) and every gradient of autograd, float64 against float64."""
    top, blocks, img, valid, d_out, heads, p, r = _setup(case)
    out, tape = pr.postln_forward(fr.A64, img, valid, top, blocks, heads, r)
    want, P, x = pr.torch_adapter(top, blocks, heads, False, img, valid, r)
    torch.testing.assert_close(out, want.detach(), rtol=1e-11, atol=1e-12)
    want.backward(d_out.double())
    grads, d_img, _ = pr.postln_backward(fr.A64, img, valid, top, blocks, heads, r, tape, d_out)
    for k, g in pr.named_grads(grads).items():
        torch.testing.assert_close(g, P[k].grad, rtol=1e-9, atol=1e-11, msg=k)
    torch.testing.assert_close(d_img, x.grad, rtol=1e-9, atol=1e-11)
    # the fp32 restatement stays near it
    out32, _ = pr.postln_forward(fr.A32, img, valid, top, blocks, heads, r)
    torch.testing.assert_close(out32.double(), out, rtol=pr.SERVE_RTOL, atol=pr.SERVE_ATOL)


def test_pre_ln_is_a_different_function():
    top, blocks, img, valid, d_out, heads, p, r = _setup(SMALL[0])
    post, _ = pr.postln_forward(fr.A64, img, valid, top, blocks, heads, r)
    pre, _ = fr.adapter_forward(fr.A64, img, valid, top, blocks, heads, r)
    assert float((post - pre).abs().max()) > 1e-2


def test_fixture_matches_the_restatement():
    """The reference's own TransformerAdapter(norm_first=False) (tools/make_golden_adapter_postln.py): output on valid views
    and every gradient against the float64 restatement, at the serving tolerance / the training steps' gradient tolerance."""
    z = np.load(GOLDEN)
    geo = pr.FIXTURE_GEOMETRY
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')}
    assert set(sd) == set(pr.state_dict_of(*fr.adapter_params(geo['D'], geo['d'], geo['heads'], geo['ffn'], geo['layers'])))
    top = {f: sd[n] for f, n in pr.TOP_NAMES.items()}
    blocks = [{f: sd[f'transformer_encoder.layers.{l}.{n}'] for f, n in pr.NAMES.items()} for l in range(geo['layers'])]
    img, valid, d_out = (torch.from_numpy(z[k]) for k in ('feats', 'valid', 'd_out'))
    assert img.shape == (geo['B'], geo['T'], geo['D']) and not bool(img[~valid].any())
    r = float(z['residual'])
    out, tape = pr.postln_forward(fr.A64, img, valid, top, blocks, geo['heads'], r)
    got = torch.from_numpy(z['out']).double()
    torch.testing.assert_close(got[valid], out[valid], rtol=pr.SERVE_RTOL, atol=pr.SERVE_ATOL)
    d_masked = d_out * valid[..., None]                   # the fixture's loss reads the valid views only
    grads, d_img, _ = pr.postln_backward(fr.A64, img, valid, top, blocks, geo['heads'], r, tape, d_masked)
    for k, g in pr.named_grads(grads).items():
        w = torch.from_numpy(z['g:' + k]).double()
        assert float((w - g).abs().max()) <= pr.GRAD_TOL * float(g.abs().max()), k
    w = torch.from_numpy(z['g_feats']).double()
    assert float((w - d_img)[valid].abs().max()) <= pr.GRAD_TOL * float(d_img.abs().max())


# ---- planted faults: the check functions of the GPU tests must reject each of them, and pass the fp32 restatement ----
def _f32_model(case, fwd_fault=None, bwd_fault=None):
    top, blocks, img, valid, d_out, heads, p, r = _setup(case)
    out, tape = pr.postln_forward(fr.A32, img, valid, top, blocks, heads, r, p, 77, fault=fwd_fault)
    clean_tape = pr.postln_forward(fr.A32, img, valid, top, blocks, heads, r, p, 77)[1] if fwd_fault else tape
    grads, d_img, scr = pr.postln_backward(fr.A32, img, valid, top, blocks, heads, r, clean_tape, d_out, p, 77, fault=bwd_fault)
    return (img, valid, top, blocks, heads, r, p, 77), out, tape, d_out, grads, d_img, scr


@pytest.mark.parametrize('case', SMALL, ids=str)
def test_checks_pass_the_fp32_restatement(case):
    a, out, tape, d_out, grads, d_img, scr = _f32_model(case)
    worst = pr.check_postln_forward(*a, out, tape, 'f32')
    if case[3] == 1:
        worst.update(pr.check_postln_backward(*a, tape, d_out, grads, d_img, scr, 'f32'))
    print(f'\n[postln checks] {case}: fp32 restatement, worst error / bound = { {k: round(v, 4) for k, v in worst.items()} }')
    assert max(worst.values()) <= 1, worst


@pytest.mark.parametrize('fault', ['pre_ln', 'no_last_norm2', 'res2_from_s1'])
def test_forward_check_rejects(fault):
    for case in SMALL[:2]:
        a, out, tape, *_ = _f32_model(case, fwd_fault=fault)
        with pytest.raises(AssertionError):
            pr.check_postln_forward(*a, out, tape, fault)


def test_backward_check_rejects_in_proj_gradient_against_norm1_output():
    a, out, tape, d_out, grads, d_img, scr = _f32_model(SMALL[1], bwd_fault='qkv_w_against_a')
    with pytest.raises(AssertionError, match='qkv_w'):
        pr.check_postln_backward(*a, tape, d_out, grads, d_img, scr, 'fault')


def test_end_to_end_tolerance_rejects_the_faults():
    """The tolerances of the end-to-end GPU tests (3e-4 of the largest gradient) see each fault too."""
    case = SMALL[0]
    top, blocks, img, valid, d_out, heads, p, r = _setup(case)
    _, tape = pr.postln_forward(fr.A64, img, valid, top, blocks, heads, r)
    want, _, _ = pr.postln_backward(fr.A64, img, valid, top, blocks, heads, r, tape, d_out)
    want = pr.named_grads(want)
    for ff, bf in (('res2_from_s1', None), ('no_last_norm2', None), (None, 'qkv_w_against_a')):
        _, t32 = pr.postln_forward(fr.A32, img, valid, top, blocks, heads, r, fault=ff)
        got, _, _ = pr.postln_backward(fr.A32, img, valid, top, blocks, heads, r, t32, d_out, fault=bf)
        got = {k: v.double() for k, v in pr.named_grads(got).items()}
        with pytest.raises(AssertionError):
            pr.assert_e2e(0.0, None, got, 0.0, None, want, 'fault')
    _, t32 = pr.postln_forward(fr.A32, img, valid, top, blocks, heads, r)
    got, _, _ = pr.postln_backward(fr.A32, img, valid, top, blocks, heads, r, t32, d_out)
    assert pr.assert_e2e(0.0, None, pr.named_grads(got), 0.0, None, want, 'clean') < 0.1


# ---- max aggregation ----
@pytest.mark.parametrize('i', range(len(pr.MAX_SHAPES)))
def test_committed_seeds_keep_the_two_best_views_apart(i):
    """float64 gap of at least MIN_GAP between the two best valid views of every (sample, class), for the identity head and
    behind both adapters; and no configuration the GPU tests run is a saturated problem (float64 loss at least MIN_LOSS)."""
    gaps, losses = [], []
    for layout, agg, probs in pr.E2E_CONFIGS:
        y = pr.max_yardstick(pr.max_case(i, layout), layout, agg, probs)
        losses.append(float(y['loss']))
        if agg == 'max':
            gaps.append(y['gap'])
    print(f'\n[max gap] shape {pr.MAX_SHAPES[i]} seed {pr.MAX_SEEDS[i]}: gaps {min(gaps):.3f} .. {max(gaps):.3f}, '
          f'losses {min(losses):.3f} .. {max(losses):.3f}')
    assert min(gaps) >= pr.MIN_GAP, gaps
    assert min(losses) >= pr.MIN_LOSS, losses


def _max_dl(full, valid, d_logits, fault=None):
    vm = valid[..., None]
    if fault == 'spread':
        return (d_logits[:, None, :] * vm).float()
    l = full.double() if fault == 'padded_wins' else full.double().masked_fill(~vm, float('-inf'))
    win = torch.nn.functional.one_hot(l.argmax(1), full.shape[1]).transpose(1, 2)
    return (d_logits[:, None, :] * win).float()


def test_max_check_rejects_spread_gradient_and_padded_winner():
    c = pr.max_case(0, None)
    y = pr.max_yardstick(c, None, 'max', False)
    B, K = y['logits'].shape
    d_logits = (torch.softmax(y['logits'], -1) - torch.nn.functional.one_hot(c['labels'], K)) / B
    full = y['full'].clone()
    assert not c['valid'].all()
    full[~c['valid']] = 0.0                                      # what the scatter leaves on padded views
    full = full - full[c['valid']].max() - 1.0                   # every valid logit negative: a padded 0 would win
    full[~c['valid']] = 0.0
    assert pr.check_max_head(full, c['valid'], d_logits, _max_dl(full, c['valid'], d_logits), 'clean') <= 1e-3
    with pytest.raises(AssertionError, match='not the maximum'):
        pr.check_max_head(full, c['valid'], d_logits, _max_dl(full, c['valid'], d_logits, 'spread'), 'spread')
    with pytest.raises(AssertionError, match='padded'):
        pr.check_max_head(full, c['valid'], d_logits, _max_dl(full, c['valid'], d_logits, 'padded_wins'), 'padded')


def test_head64_max_is_the_reference_expression():
    c = pr.max_case(0, None)
    loss, logits, full = pr.head64(c['feats'].double(), c['valid'], c['labels'], c['text'].double(), pr.LOGIT_SCALE, 'max', False)
    want = full.masked_fill(~c['valid'][..., None], float('-inf')).max(1).values
    assert torch.equal(logits, want)
    # against the project's own dZ yardstick: the gradient of the aggregated logits goes to the maximal valid view
    gl = torch.ones_like(logits)
    dz = fr.classify_dz(fr.A64, full * c['valid'][..., None], c['valid'], 'max', d_logits=gl)
    assert torch.equal(dz.sum(1), gl) and not bool(dz[~c['valid']].any())


# ---- the surface that needs no GPU ----
def test_post_ln_adapter_constructs_with_the_reference_keys():
    from eventclip_amd.adapter import TransformerAdapter, adapter_param_names
    ad = TransformerAdapter(in_dim=64, d_model=32, num_heads=4, ffn_dim=48, norm_first=False, num_layers=2, residual=0.5)
    assert ad.norm_first is False and ad.transformer_encoder.layers[0].norm_first is False
    assert [n for n, _ in ad.named_parameters()] == adapter_param_names(2)
    assert set(ad.state_dict()) == set(np.load(GOLDEN)['keys'].tolist())
    assert TransformerAdapter(in_dim=64, d_model=32, num_heads=4, ffn_dim=48).norm_first is True


def test_bindings_carry_the_layout_and_the_max_code():
    from eventclip_amd import _lib, ft, train
    from eventclip_amd.adapter import _adapter_struct
    assert _lib.EcAdapterWeights._fields_[-1] == ('post_norm', ctypes.c_int)
    assert _lib.EcAdapterTrainParams._fields_[-1] == ('post_norm', ctypes.c_int)
    assert _lib.EcAdapterWeights().post_norm == 0 and _lib.EcAdapterTrainParams().post_norm == 0     # zero means pre-LN
    none = [None] * 16
    assert _adapter_struct(none, 8, 8, 1, 4, 1, 0.5)[0].post_norm == 0
    assert _adapter_struct(none, 8, 8, 1, 4, 1, 0.5, 1)[0].post_norm == 1
    assert train._AGG['max'] == _lib.EC_AGG_MAX == 2 and ft._AGG is train._AGG
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'include', 'eventclip_hip.h')).read()
    assert f'#define EC_ABI_VERSION {_lib.ABI_VERSION}' in header and _lib.ABI_VERSION >= 606
