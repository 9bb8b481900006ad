"""The few-shot classifiers under torch autograd on the MI355X: the `classify` VJP and the adapter's train ops
against float64, the dropout replayed in the oracle, the whole `forward -> calc_train_loss -> backward` against the
reference's own autograd vectors and the fused trainers, a torch optimiser, and what stays as it was.

Bounds (tests/test_train_gpu.py: the arithmetic is the same fp32, so the bounds are the same):
    gradients within 5e-4 * max(|want|, 1e-3) of the reference's autograd fixtures,
    gradients within 1e-3 * max(|want|, 1e-4) of float64,
    losses within 3e-4 * max(1, |want|).
Every test prints the errors it measured.
"""
import copy
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AGG = {'sum': 0, 'mean': 1, 'max': 2}


def _check_grad(name, got, want, rel, floor):
    """max |got - want| < rel * max(max |want|, floor); prints the measured figures."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, ref = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f'{name}: max err {err:.3e}, max |want| {ref:.3e}, bound {rel * max(ref, floor):.3e}')
    assert err < rel * max(ref, floor), (name, err, ref)


def _idx(valid):
    import torch
    B, T = valid.shape
    return torch.where(valid, torch.arange(B * T, device=valid.device).view(B, T),
                       torch.full((B, T), -1, device=valid.device)).to(torch.int32)


# ------------------------------------------------------------------------------------------------
# 1. the classify VJP against float64 autograd over oracle.classify
# ------------------------------------------------------------------------------------------------
def _classify_problem(B, T, C, K, agg, normalize):
    """Ragged mask (sample 0 holds a single valid view), compact feature rows in a shuffled order plus one row no view
    names, unit text rows.  normalize=False: features of norm ~10 (un-normalised logits up to a few hundred).
    agg='max': drawn again until no two valid views of a sample are near a tie in any class, so that the fp32 forward
    and the float64 reference agree on the maximal view."""
    import torch
    from oracle import classify as oc
    for seed in range(400):
        g = torch.Generator().manual_seed(1000 * seed + 31 * B + 7 * T + K)
        valid = torch.rand(B, T, generator=g) < 0.6
        valid[:, 0] = True
        if T > 1:
            valid[0, 1:] = False
        nv = int(valid.sum())
        feats = torch.randn(nv + 1, C, generator=g, dtype=torch.float64) * (10. / C ** 0.5 if not normalize else 0.7)
        text = torch.nn.functional.normalize(torch.randn(K, C, generator=g, dtype=torch.float64), dim=-1)
        rows = torch.randperm(nv + 1, generator=g)[:nv]                   # one row stays unused
        row_idx = torch.full((B, T), -1, dtype=torch.int64)
        row_idx[valid] = rows
        if agg != 'max':
            break
        # a fp32 logit is off by a few eps * scale * |f| |t|; 64 of those between the two largest views keeps the argmax
        used = feats[rows] if not normalize else torch.nn.functional.normalize(feats[rows], dim=-1)
        full = torch.full((B, T, K), -1e30, dtype=torch.float64)
        full[valid] = 100. * used @ text.T
        top = full.topk(min(2, T), dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min()) if T > 1 else 1.
        if gap > 64 * 6e-8 * 100. * float(used.norm(dim=-1).max()):
            break
    else:
        raise AssertionError('no tie-free draw')
    return valid, row_idx, feats, text, oc


def _classify_ref(oc, feats, text, valid, row_idx, agg, normalize):
    """float64 outputs of the oracle with autograd into feats [n_rows, C] and text [K, C]."""
    import torch
    used = feats[row_idx[valid]]                                          # (b, t) row-major order
    if not normalize:
        return oc.zs_forward(used, valid, text, 100., agg)
    B, T = valid.shape
    full = torch.zeros(B, T, feats.shape[1], dtype=torch.float64).masked_scatter(valid[..., None], used)
    return oc.fs_tail(full, valid, text, 100., agg)


@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('agg', ['sum', 'mean', 'max'])
@pytest.mark.parametrize('B,T,C,K', [(3, 4, 64, 5), (1, 1, 64, 2), (2, 10, 768, 101), (2, 16, 512, 1000)])
def test_classify_vjp_matches_float64(B, T, C, K, agg, normalize, hip):
    import torch
    from eventclip_amd import torch_ops  # noqa: F401
    valid, row_idx, feats64, text64, oc = _classify_problem(B, T, C, K, agg, normalize)
    feats64.requires_grad_(True)
    text64.requires_grad_(True)
    ref = _classify_ref(oc, feats64, text64, valid, row_idx, agg, normalize)
    f = feats64.detach().float().cuda().requires_grad_(True)
    tt = text64.detach().float().t().contiguous().cuda().requires_grad_(True)
    ri = row_idx.to(torch.int32).cuda()
    out = dict(zip(('full_logits', 'logits', 'probs'),
                   torch.ops.eventclip_hip.classify(f, ri, tt, 100., AGG[agg], normalize)))
    g = torch.Generator().manual_seed(5)
    cot = {k: torch.randn(ref[k].shape, generator=g, dtype=torch.float64) for k in out}
    unused = torch.ones(feats64.shape[0], dtype=torch.bool)
    unused[row_idx[valid]] = False
    for names in (('full_logits',), ('logits',), ('probs',), ('full_logits', 'logits', 'probs')):
        want_f, want_t = torch.autograd.grad([ref[k] for k in names], [feats64, text64], [cot[k] for k in names],
                                             retain_graph=True)
        got_f, got_t = torch.autograd.grad([out[k] for k in names], [f, tt], [cot[k].float().cuda() for k in names],
                                           retain_graph=True)
        tag = f'classify {B}x{T}x{C}x{K} {agg} normalize={normalize} d({"+".join(names)})'
        _check_grad(tag + ' / d_feats', got_f.cpu(), want_f, 1e-3, 1e-4)
        _check_grad(tag + ' / d_text', got_t.t().cpu(), want_t, 1e-3, 1e-4)
        assert float(got_f[unused.cuda()].abs().max()) == 0., 'a feature row no view names got a gradient'
    # invalid views: exact zeros in dZ, seen through the VJP of full_logits alone with the cotangent on invalid views only
    if not bool(valid.all()):
        c = (cot['full_logits'] * (~valid)[..., None]).float().cuda()
        zf, zt = torch.autograd.grad(out['full_logits'], [f, tt], c)
        assert float(zf.abs().max()) == 0. and float(zt.abs().max()) == 0.


# ------------------------------------------------------------------------------------------------
# 2. adapter_train_fwd / adapter_train_bwd against the float64 torch modules
# ------------------------------------------------------------------------------------------------
def _adapter(D, d, heads, ffn, residual, seed, noise=0.05):
    import torch
    from eventclip_amd.adapter import TransformerAdapter
    torch.manual_seed(seed)
    ad = TransformerAdapter(in_dim=D, d_model=d, num_heads=heads, ffn_dim=ffn, num_layers=2, residual=residual)
    with torch.no_grad():
        for p in ad.parameters():
            p.add_(torch.randn_like(p) * noise)
    return ad


def _adapter_ref64(ad, x, valid):
    """in_proj -> transformer_encoder(src_key_padding_mask) -> out_proj -> residual on the float64 eval-mode copy."""
    ref = copy.deepcopy(ad).double().cpu().eval()
    y = ref.in_proj(x)
    y = ref.transformer_encoder(y, src_key_padding_mask=~valid)
    y = ref.out_proj(y)
    return ref, x * ad.residual + y * (1. - ad.residual)


@pytest.mark.parametrize('residual', [0., 0.8])
@pytest.mark.parametrize('D,d,heads,ffn', [(48, 32, 2, 64), (768, 256, 4, 1024)])
@pytest.mark.parametrize('T', [1, 2, 5, 10])
def test_adapter_train_ops_match_float64(T, D, d, heads, ffn, residual, hip):
    import torch
    B = 3                                                               # B * T = 3, 6, 15, 30: no multiple of 4
    ad = _adapter(D, d, heads, ffn, residual, seed=T + D)
    g = torch.Generator().manual_seed(T)
    valid = torch.rand(B, T, generator=g) < 0.6
    valid[:, 0] = True
    x64 = (torch.randn(B, T, D, generator=g, dtype=torch.float64) * valid[..., None]).requires_grad_(True)
    cot = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    ref, want_out = _adapter_ref64(ad, x64, valid)
    want_out.backward(cot)
    ad = ad.cuda().eval()                                               # eval: no dropout, the function the reference copy computes
    x = x64.detach().float().cuda().requires_grad_(True)
    out, tape = torch.ops.eventclip_hip.adapter_train_fwd(x.reshape(B * T, D), _idx(valid.cuda()), list(ad.parameters()),
                                                          d, heads, ffn, 2, float(residual), 0., 0)
    assert tape.dtype == torch.uint8 and not tape.requires_grad and out.requires_grad
    tag = f'adapter T={T} {d}/{heads}/{ffn} D={D} r={residual}'
    err = float((out.detach().cpu().double() - want_out.detach()).abs().max())
    want_max = float(want_out.detach().abs().max())
    print(f'{tag} / out: max err {err:.3e}, max |want| {want_max:.3e}')
    assert err < 3e-4 * max(1., want_max)
    out.backward(cot.float().cuda())
    for (name, p), q in zip(ad.named_parameters(), ref.parameters()):
        _check_grad(f'{tag} / {name}', p.grad.cpu(), q.grad, 1e-3, 1e-4)
    _check_grad(f'{tag} / d_feats', x.grad.cpu(), x64.grad, 1e-3, 1e-4)


# ------------------------------------------------------------------------------------------------
# 3. dropout
# ------------------------------------------------------------------------------------------------
def test_dropout_masks_replayed_in_the_oracle(hip):
    """The problem of test_text_trans_dropout_replayed_in_the_oracle through the autograd ops: p = 0.3, the masks of
    train.dropout_mask replayed in oracle.train.fs_trans_loss_and_grads; the same seed gives the same bits."""
    import torch
    import torch.nn.functional as F
    from eventclip_amd import train
    from oracle import train as ot
    torch.manual_seed(5)
    B, T, D, K, d, ffn, heads, p_drop, seed = 12, 6, 96, 9, 64, 128, 4, 0.3, 987654321
    ad = _adapter(D, d, heads, ffn, 0.6, seed=5)
    valid = torch.rand(B, T) < 0.7
    valid[:, 0] = True
    labels = torch.randint(0, K, (B,))
    text = torch.randn(K, D) * 0.5
    feats = (torch.randn(B, T, D) + 0.15 * text[labels][:, None]) * valid[..., None]
    sizes = {0: B * heads * T * T, 1: B * T * d, 2: B * T * ffn, 3: B * T * d}
    masks = {(l, s): train.dropout_mask(seed, 4 * l + s, n, p_drop).cpu().numpy() for l in range(2) for s, n in sizes.items()}
    want_loss, want, _ = ot.fs_trans_loss_and_grads(
        {k: v.detach().numpy() for k, v in ad.state_dict().items()}, feats.numpy(), valid.numpy(), labels.numpy(),
        text.numpy(), 100.0, heads, 0.6, 'mean', False, dropout_p=p_drop, masks=masks)
    ad = ad.cuda()
    tp = text.cuda().requires_grad_(True)
    rows, idx = feats.cuda().reshape(B * T, D), _idx(valid.cuda())

    def run():
        out, _ = torch.ops.eventclip_hip.adapter_train_fwd(rows, idx, list(ad.parameters()), d, heads, ffn, 2, 0.6,
                                                           p_drop, seed)
        text_t = F.normalize(tp, dim=-1).t().contiguous()
        _, logits, _ = torch.ops.eventclip_hip.classify(out.reshape(B * T, D), idx, text_t, 100., AGG['mean'], True)
        return out, F.cross_entropy(logits, labels.cuda())

    out, loss = run()
    print(f'dropout / loss: got {float(loss):.6f}, want {want_loss:.6f}')
    assert abs(float(loss) - want_loss) < 3e-4 * max(1., abs(want_loss))
    loss.backward()
    for name, p in list(ad.named_parameters()) + [('text_feats', tp)]:
        _check_grad(f'dropout / {name}', p.grad.cpu(), want[name], 1e-3, 1e-4)
    out2, loss2 = run()
    assert torch.equal(out, out2) and torch.equal(loss, loss2)
    out3, _ = torch.ops.eventclip_hip.adapter_train_fwd(rows, idx, list(ad.parameters()), d, heads, ffn, 2, 0.6, p_drop,
                                                        seed + 1)
    assert not torch.equal(out, out3)


def test_dropout_seed_comes_from_the_default_generator(hip):
    import torch
    ad = _adapter(48, 32, 2, 64, 0.5, seed=1).cuda().train()
    valid = torch.ones(3, 5, dtype=torch.bool, device='cuda')
    valid[1, 3:] = False
    x = torch.randn(3, 5, 48, device='cuda') * valid[..., None]
    torch.manual_seed(7)
    a, b = ad(x, valid), ad(x, valid)
    torch.manual_seed(7)
    c, d = ad(x, valid), ad(x, valid)
    assert a.requires_grad and not torch.equal(a, b)
    assert torch.equal(a, c) and torch.equal(b, d)
    ad.eval()                                                           # eval: the fused inference kernel, no graph
    e, f = ad(x, valid), ad(x, valid)
    assert torch.equal(e, f) and not e.requires_grad
    with torch.no_grad():
        assert not ad.train()(x, valid).requires_grad


# ------------------------------------------------------------------------------------------------
# 4. end to end against the reference's own autograd, and against the fused steps
# ------------------------------------------------------------------------------------------------
_CLIP = {}


def _tiny_clip():
    from eventclip_amd import clip as eclip
    if 'm' not in _CLIP:
        cfg = eclip.arch_config('ViT-B/32', layers=1, text_layers=1, vocab_size=49408)
        _CLIP['m'] = (cfg, eclip.CLIP(cfg, eclip.random_state_dict(cfg, seed=9)).cuda().eval())
    return _CLIP['m']


def _classifier(adapter_dict, K, agg, probs_loss, cls=None):
    from eventclip_amd import clip as eclip
    from eventclip_amd.clip_cls import FSCLIPClassifier
    _, m = _tiny_clip()
    return (cls or FSCLIPClassifier)(
        adapter_dict=adapter_dict,
        clip_dict=dict(clip_model=m, prompt='a {}', class_names=[f'c{i}' for i in range(K)], agg_func=agg,
                       class_tokens=eclip.synthetic_tokens(K, seed=4)),
        loss_dict=dict(use_logits_loss=not probs_loss, use_probs_loss=probs_loss)).cuda()


def _inject(clf, feats, valid):
    """Stub the frozen encoder: `_view_feats` hands out the compact valid-view rows of feats [B, T, C]."""
    import torch
    flat = valid.reshape(-1)
    row_idx = torch.where(flat, torch.cumsum(flat.int(), 0) - 1, torch.full_like(flat, -1, dtype=torch.int64))
    row_idx = row_idx.to(torch.int32).reshape(valid.shape)
    compact = feats[valid].float().contiguous()
    clf._view_feats = lambda data_dict: (compact, row_idx, valid)


def _fixture_classifier(z, ci, kind, agg, loss):
    import torch
    from torch import nn
    C, K = int(z['C']), int(z['K'])
    if kind == 'trans':
        ad = dict(adapter_type='text-trans', in_dim=C, d_model=int(z['adcfg_d_model']),
                  num_heads=int(z['adcfg_num_heads']), ffn_dim=int(z['adcfg_ffn_dim']),
                  num_layers=int(z['adcfg_num_layers']), residual=float(z['adcfg_residual']))
    else:
        ad = dict(adapter_type='text-identity', in_dim=C, residual=True)
    clf = _classifier(ad, K, agg, loss == 'probs')
    if kind == 'trans':
        clf.adapter.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')})
    clf.text_feats = nn.Parameter(torch.from_numpy(z[f'c{ci}_text_param']).cuda())
    clf.logit_scale = float(z[f'c{ci}_logit_scale'])
    clf = clf.cuda()
    clf.train()
    clf.adapter.eval()                                                  # no dropout: the function the fixtures differentiate
    return clf


def _end_to_end(z, ci, kind, agg, loss):
    import torch
    from eventclip_amd import train
    tag = f'c{ci}_{agg}_{loss}'
    clf = _fixture_classifier(z, ci, kind, agg, loss)
    f = torch.from_numpy(z[f'c{ci}_feats']).cuda()
    v = torch.from_numpy(z[f'c{ci}_valid']).cuda()
    y = torch.from_numpy(z[f'c{ci}_labels']).cuda()
    _inject(clf, f, v)
    data = {'valid_mask': v, 'label': y}
    out = clf(data)
    ce = clf.calc_train_loss(data, out)['ce_loss']
    ce.backward()
    want_loss = float(z[tag + '_loss'])
    print(f'{kind} {tag} / ce_loss: got {float(ce):.6f}, want {want_loss:.6f}')
    assert abs(float(ce) - want_loss) < 3e-4 * max(1., abs(want_loss))
    np.testing.assert_allclose(out['logits'].detach().cpu().numpy(), z[tag + '_logits'], rtol=2e-4, atol=2e-3)
    got = {'text_feats': clf.text_feats.grad}
    got.update({k: p.grad for k, p in clf.adapter.named_parameters() if p.requires_grad})
    if kind == 'trans':
        want = {k.split('_g:')[1]: z[k] for k in z.files if k.startswith(tag + '_g:')}
        fused_loss, fused = train.fs_trans_loss_grad(f, v, y, clf.text_feats.data, clf.logit_scale, clf.adapter, agg,
                                                     loss == 'probs')
    else:
        want = {'text_feats': z[tag + '_grad']}
        fused_loss, g = train.fs_text_loss_grad(f, v, y, clf.text_feats.data, clf.logit_scale, agg, loss == 'probs')
        fused = {'text_feats': g}
    assert set(got) == set(want) == set(fused)
    for k in want:
        assert got[k] is not None, k
        _check_grad(f'{kind} {tag} / {k} vs the reference', got[k].cpu(), want[k], 5e-4, 1e-3)
        _check_grad(f'{kind} {tag} / {k} vs the fused step', got[k].cpu(), fused[k].cpu(), 5e-4, 1e-3)
    assert abs(float(ce) - float(fused_loss)) < 3e-4 * max(1., abs(float(fused_loss)))


@pytest.mark.parametrize('ci,agg,loss', [(ci, a, l) for ci in range(3) for a, l in (('sum', 'logits'), ('mean', 'probs'))])
def test_text_trans_end_to_end_matches_reference_autograd(ci, agg, loss, hip):
    _end_to_end(np.load(os.path.join(GOLDEN, 'train_text_trans.npz')), ci, 'trans', agg, loss)


@pytest.mark.parametrize('ci,agg,loss', [(ci, a, l) for ci in range(3) for a in ('sum', 'mean') for l in ('logits', 'probs')])
def test_text_identity_end_to_end_matches_reference_autograd(ci, agg, loss, hip):
    _end_to_end(np.load(os.path.join(GOLDEN, 'train_text_identity.npz')), ci, 'identity', agg, loss)


# ------------------------------------------------------------------------------------------------
# 5. a torch optimiser fits
# ------------------------------------------------------------------------------------------------
def _separable_problem():
    """The problem of test_adapter_trainer_reduces_the_loss_and_updates_the_forward."""
    import torch
    cfg, _ = _tiny_clip()
    K, B, T, D = 4, 16, 3, cfg['embed_dim']
    clf = _classifier(dict(adapter_type='text-trans', in_dim=D, d_model=64, num_heads=2, ffn_dim=128, num_layers=2,
                           residual=0.5), K, 'mean', False)
    g = torch.Generator(device='cuda').manual_seed(2)
    labels = torch.arange(B, device='cuda') % K
    centres = torch.randn(K, D, device='cuda', generator=g)
    valid = torch.ones(B, T, dtype=torch.bool, device='cuda')
    valid[1::3, 2] = False
    feats = (centres[labels][:, None] + 0.5 * torch.randn(B, T, D, device='cuda', generator=g)) * valid[..., None]
    _inject(clf, feats, valid)
    return clf, {'valid_mask': valid, 'label': labels}


def test_torch_adam_fits_and_the_inference_kernel_sees_the_update(hip):
    import torch
    from eventclip_amd.train import cosine_warmup_lr
    clf, data = _separable_problem()
    before = clf.eval()(data)['logits'].clone()                         # packs the adapter's inference copies
    assert clf.adapter._packed is not None
    clf.train()
    torch.manual_seed(0)
    opt = torch.optim.Adam([p for p in clf.parameters() if p.requires_grad], lr=3e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: cosine_warmup_lr(s, 60, 3e-3, 3e-5, 3.0) / 3e-3)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = clf.calc_train_loss(data, clf(data))['ce_loss']
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss))
    print(f'torch Adam: loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert losses[-1] < 0.2 * losses[0]
    clf.adapter.eval()
    train_logits = clf(data)['logits']                                  # train path (grad on), no dropout
    assert train_logits.requires_grad
    eval_logits = clf.eval()(data)['logits']                            # the fused inference kernel
    assert not torch.equal(eval_logits, before)
    torch.testing.assert_close(eval_logits, train_logits.detach(), rtol=1e-3, atol=1e-2)
    assert float((eval_logits.argmax(-1) == data['label']).float().mean()) == 1.0


# ------------------------------------------------------------------------------------------------
# 6. unchanged and refused
# ------------------------------------------------------------------------------------------------
def test_eval_and_no_grad_outputs_are_the_inference_ops(hip):
    import torch
    from eventclip_amd import torch_ops
    clf, data = _separable_problem()
    feats, row_idx, valid = clf._view_feats(data)
    B, T = valid.shape
    full = torch.ops.eventclip_hip.adapter_fwd(feats, row_idx, torch_ops.handle_of(clf.adapter))
    want = torch.ops.eventclip_hip.classify(full.reshape(B * T, -1).contiguous(), _idx(valid), clf._text_transposed(),
                                            float(clf.logit_scale), AGG['mean'], True)
    clf.eval()
    outs = [clf(data)]
    clf.train()
    with torch.no_grad():
        outs.append(clf(data))
    for out in outs:
        for k, w in zip(('full_logits', 'logits', 'probs'), want):
            assert torch.equal(out[k], w) and not out[k].requires_grad, k
    ev = clf.calc_eval_loss(data, outs[0])
    assert set(ev) == {'ce_loss', 'probs_acc', 'logits_acc'} and not ev['ce_loss'].requires_grad


def test_frozen_parameters_retain_graph_and_no_double_backward(hip):
    import torch
    clf, data = _separable_problem()
    clf.train()
    clf.adapter.eval()
    frozen = ['in_proj.weight', 'transformer_encoder.layers.1.norm2.bias', 'transformer_encoder.layers.0.linear1.weight']
    named = dict(clf.adapter.named_parameters())
    for k in frozen:
        named[k].requires_grad_(False)
    loss = clf.calc_train_loss(data, clf(data))['ce_loss']
    loss.backward(retain_graph=True)
    first = {k: p.grad.clone() for k, p in clf.named_parameters() if p.grad is not None}
    assert set(first) == {'text_feats'} | {'adapter.' + k for k in named if k not in frozen}
    loss.backward()                                                     # the tape is only read: the same bits again
    for k, p in clf.named_parameters():
        if k in first:
            assert torch.equal(p.grad, 2 * first[k]), k
        else:
            assert p.grad is None, k
    # the backward ops carry no autograd formula
    loss = clf.calc_train_loss(data, clf(data))['ce_loss']
    g, = torch.autograd.grad(loss, clf.text_feats, create_graph=True)
    with pytest.raises(RuntimeError):
        g.square().sum().backward()
    clf.text_feats.requires_grad_(False)                                # a frozen prompt: only the adapter trains
    clf.zero_grad()
    clf.calc_train_loss(data, clf(data))['ce_loss'].backward()
    assert clf.text_feats.grad is None and named['out_proj.weight'].grad is not None


def test_ft_classifier_builds_no_graph_in_train_mode(hip):
    import torch
    from eventclip_amd.clip_cls_ft import FTCLIPClassifier
    clf = _classifier(dict(adapter_type='text-identity', residual=True), 3, 'mean', False, cls=FTCLIPClassifier).train()
    g = torch.Generator(device='cuda').manual_seed(3)
    data = {'img': torch.randn(2, 2, 3, 224, 224, device='cuda', generator=g),
            'valid_mask': torch.tensor([[True, True], [True, False]], device='cuda')}
    assert clf.text_feats.requires_grad and torch.is_grad_enabled()
    out = clf(data)
    assert not out['logits'].requires_grad and not out['probs'].requires_grad and out['logits'].grad_fn is None


def test_opcheck_on_the_new_and_changed_ops(hip):
    import torch
    from eventclip_amd import torch_ops  # noqa: F401
    ops = torch.ops.eventclip_hip
    B, T, C, K, d, heads, ffn = 2, 3, 48, 5, 32, 2, 64
    ad = _adapter(C, d, heads, ffn, 0.8, seed=2).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    valid = torch.tensor([[True, True, False], [True, False, False]], device='cuda')
    idx = _idx(valid)
    rows = (torch.randn(B, T, C, device='cuda', generator=g) * valid[..., None]).reshape(B * T, C)
    text_t = torch.randn(C, K, device='cuda', generator=g)
    params = [p.detach().clone().requires_grad_(True) for p in ad.parameters()]
    geo = (d, heads, ffn, 2, 0.8, 0.1, 11)
    torch.library.opcheck(ops.classify.default, (rows.clone().requires_grad_(True), idx, text_t.clone().requires_grad_(True),
                                                 100., AGG['mean'], True))
    torch.library.opcheck(ops.adapter_train_fwd.default, (rows.clone().requires_grad_(True), idx, params) + geo)
    full, logits, probs = ops.classify(rows, idx, text_t, 100., AGG['max'], True)
    torch.library.opcheck(ops.classify_bwd.default, (rows, idx, text_t, full, torch.randn_like(full), None,
                                                     torch.randn_like(probs), 100., AGG['max'], True, True, True))
    out, tape = ops.adapter_train_fwd(rows, idx, [p.detach() for p in params], *geo)
    torch.library.opcheck(ops.adapter_train_bwd.default, (rows, idx, [p.detach() for p in params], tape,
                                                          torch.randn_like(out)) + geo + ((1 << 28) | 0b1011,))
