"""agg_func = 'max' in the three fused training steps (fs_text_loss_grad, fs_trans_loss_grad behind a pre- and a post-LN
adapter, ft_loss_grad), both loss kinds, against float64 autograd over the reference's expression
(logits - (1 - valid) * 1e6).max(views); agreement with the classify + classify_bwd route; exact zeros on views that are
not the maximum and on padded views; the trainers.  Inputs come from fixed seeds whose float64 gap between the two best
valid views is asserted (tests/adapter_postln_ref.py: MIN_GAP), so the fp32 forward picks the view float64 picks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_postln_ref as pr  # noqa: E402
from test_autograd_gpu import _classifier  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(i, probs) for i in range(len(pr.MAX_SHAPES)) for probs in (False, True)]
IDS = [f'{"x".join(map(str, pr.MAX_SHAPES[i]))}-{"probs" if p else "logits"}' for i, p in CASES]
_YARD = {}


def _problem(i, layout, probs):
    if (i, layout, probs) not in _YARD:
        c = pr.max_case(i, layout)
        y = pr.max_yardstick(c, layout, 'max', probs)
        assert y['gap'] >= pr.MIN_GAP, f'near tie: gap {y["gap"]}'
        _YARD[i, layout, probs] = (c, y)
    return _YARD[i, layout, probs]


def _cuda(c):
    return c['feats'].cuda(), c['valid'].cuda(), c['labels'].cuda(), c['text'].cuda()


def _report(name, msg):
    print(f'\n[train max] {name}: {msg}')


def _compact_idx(valid):
    from eventclip_amd.adapter import compact_row_idx
    return compact_row_idx(valid)


def _classify_route(feats, valid, labels, text, probs):
    """The same loss through classify + classify_bwd (loss.backward()): -> (loss, logits, d text_feats, d feats [B, T, D])."""
    B, T, D = feats.shape
    idx = _compact_idx(valid)
    rows = feats[valid].contiguous().requires_grad_(True)
    t = text.clone().requires_grad_(True)
    text_t = torch.nn.functional.normalize(t, dim=-1).t().contiguous()
    full, logits, pr_ = torch.ops.eventclip_hip.classify(rows, idx, text_t, pr.LOGIT_SCALE, 2, True)
    loss = torch.nn.functional.nll_loss(torch.log(pr_ + 1e-6), labels) if probs else torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    d_feats = torch.zeros(B, T, D, device=feats.device)
    d_feats[valid] = rows.grad
    return loss.detach(), logits.detach(), t.grad, d_feats


@pytest.mark.parametrize('i,probs', CASES, ids=IDS)
def test_text_and_ft_steps_with_max(i, probs, hip):
    from eventclip_amd import ft, train
    c, y = _problem(i, None, probs)
    f, v, lab, text = _cuda(c)
    B, T, D = f.shape
    K = text.shape[0]
    loss, grad, logits = train.fs_text_loss_grad(f, v, lab, text, pr.LOGIT_SCALE, 'max', probs, return_logits=True)
    w = pr.assert_e2e(loss, logits, {'text_feats': grad}, y['loss'], y['logits'], y['grads'], f'fs_text {IDS[CASES.index((i, probs))]}')
    # the head's per-view logit gradient, where ec_fs_text_loss_grad leaves it in its workspace (Fn [R, D] | dL [R, K] | ...)
    ws = train._scratch[f.device.index].get(int(__import__('eventclip_amd._lib', fromlist=['x']).lib()
                                                .ec_fs_text_train_workspace_bytes(B, T, D, K)), f.device)
    off = (B * T * D * 4 + 255) // 256 * 256
    dL = ws[off:off + B * T * K * 4].view(torch.float32).reshape(B, T, K).cpu()
    if not probs:
        d_logits = (torch.softmax(y['logits'], -1) - torch.nn.functional.one_hot(c['labels'], K)) / B
        pr.check_max_head(y['full'], c['valid'], d_logits, dL, 'fs_text dL')
    loss2, gimg, gtext, logits2 = ft.ft_loss_grad(f, v, lab, text, pr.LOGIT_SCALE, 'max', probs)
    pr.assert_e2e(loss2, logits2, {'text_feats': gtext}, y['loss'], y['logits'], y['grads'], 'ft_loss_grad')
    err = float((gimg.double().cpu() - y['d_feats']).abs().max())
    assert err <= pr.GRAD_TOL * float(y['d_feats'].abs().max()), f'ft_loss_grad: d feats off by {err:.3e}'
    assert not bool(gimg[~v].any()), 'a padded view got a feature gradient'
    if not probs:
        l = y['full'].masked_fill(~c['valid'][..., None], float('-inf'))
        wins = torch.zeros(B, T, dtype=torch.bool).scatter_(1, l.argmax(1), True)
        assert not bool(gimg.cpu()[~wins].any()), 'a view that is the maximum of no class got a feature gradient'
    # compact rows + row_idx, the layout FTTrainer hands over
    loss3, gimg3, _, _ = ft.ft_loss_grad(f[v].contiguous(), v, lab, text, pr.LOGIT_SCALE, 'max', probs, row_idx=_compact_idx(v))
    assert torch.equal(loss3, loss2) and torch.equal(gimg3, gimg[v])
    # the autograd route on the same inputs
    loss4, logits4, gtext4, gfeat4 = _classify_route(f, v, lab, text, probs)
    assert abs(float(loss4) - float(loss2)) <= pr.loss_tol(y['loss'])
    torch.testing.assert_close(logits4, logits2, rtol=pr.LOGITS_RTOL, atol=pr.LOGITS_ATOL)
    for name, a, b_, ref in (('text_feats', gtext4, gtext, y['grads']['text_feats']), ('feats', gfeat4, gimg, y['d_feats'])):
        assert float((a - b_).abs().max()) <= 2 * pr.GRAD_TOL * float(ref.abs().max()), f'classify route: d {name}'
    if not probs:
        assert torch.equal(gfeat4 == 0, gimg == 0), 'the two routes send the gradient to different views'
    _report(IDS[CASES.index((i, probs))], f'fs_text worst gradient error / (3e-4 max) = {w:.4f}, gap {y["gap"]:.3f}')


@pytest.mark.parametrize('layout', ['pre', 'post'])
@pytest.mark.parametrize('i,probs', CASES, ids=IDS)
def test_trans_step_with_max(i, probs, layout, hip):
    from eventclip_amd import train
    from test_adapter_postln_gpu import _module
    B, T, D, K, d, heads, ffn, layers = pr.MAX_SHAPES[i]
    c, y = _problem(i, layout, probs)
    f, v, lab, text = _cuda(c)
    ad = _module(c['top'], c['blocks'], D, d, heads, ffn, c['residual'], layout == 'pre')
    loss, grads, logits = train.fs_trans_loss_grad(f, v, lab, text, pr.LOGIT_SCALE, ad, 'max', probs, return_logits=True)
    w = pr.assert_e2e(loss, logits, grads, y['loss'], y['logits'], y['grads'], f'fs_trans {layout}')
    _report(f'{IDS[CASES.index((i, probs))]} {layout}-LN', f'worst gradient error / (3e-4 max) = {w:.4f}, gap {y["gap"]:.3f}')


def test_trainers_step_with_max(hip):
    """TextFeatTrainer, AdapterTrainer and FTTrainer's head accept agg_func = 'max' and move their parameters."""
    from eventclip_amd.train import AdapterTrainer, TextFeatTrainer
    B, T, D, K, d, heads, ffn, layers = pr.MAX_SHAPES[0]
    c, _ = _problem(0, 'post', False)
    f, v, lab, _ = _cuda(c)
    clf = _classifier(dict(adapter_type='text-identity', in_dim=D, residual=True), K, 'max', False)
    f512 = torch.nn.functional.pad(f, (0, clf.text_feats.shape[1] - D))
    before = clf.text_feats.detach().clone()
    loss = TextFeatTrainer(clf, lr=1e-3, total_steps=10).step(f512, v, lab)
    assert np.isfinite(float(loss)) and not torch.equal(before, clf.text_feats.data)
    C = clf.text_feats.shape[1]
    clf = _classifier(dict(adapter_type='text-trans', in_dim=C, d_model=d, num_heads=heads, ffn_dim=ffn, num_layers=layers,
                           residual=0.5, norm_first=False), K, 'max', True)
    before = clf.adapter.in_proj.weight.detach().clone()
    loss = AdapterTrainer(clf, lr=1e-3, total_steps=10).step(f512, v, lab)
    assert np.isfinite(float(loss)) and not torch.equal(before, clf.adapter.in_proj.weight.data)


def test_ft_trainer_step_with_max(hip):
    """One FTTrainer step of a classifier built with agg_func = 'max' (the golden fine-tuning case, its aggregation swapped)."""
    from eventclip_amd import ft
    from test_ft_train_gpu import _classifier_for, _golden_case
    _, c = _golden_case('bias')
    clf = _classifier_for(dict(c, agg='max'))
    assert clf.agg_func == 'max'
    tr = ft.FTTrainer(clf, lr=1e-3, clip_lr=1e-3, total_steps=100, init_scale=1024.0)
    before = {k: v.clone() for k, v in tr.tensors.items()}
    loss = tr.step({'img': c['imgs'].cuda(), 'valid_mask': c['valid'].cuda(), 'label': c['labels'].cuda()})
    tr.resolve()
    assert np.isfinite(float(loss)) and not tr.last['skipped']
    assert any(not torch.equal(before[k], v) for k, v in tr.tensors.items())
