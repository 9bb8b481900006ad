"""The post-LN feature adapter on the GPU, and serving at the training depth of 8 layers: the fused serving kernel on every
row against the float64 restatement, the training launches stage by stage through ec_adapter_train_layout, the fused step and
the autograd pair end to end against float64 autograd.  tests/adapter_postln_ref.py holds the yardsticks, tables, tolerances
and check functions (run against planted faults in tests/test_adapter_postln_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_postln_ref as pr  # noqa: E402
import fewshot_ref as fr  # noqa: E402
from test_autograd_gpu import _classifier, _idx, _inject  # noqa: E402
from test_fewshot_edges_gpu import SEED, Adapter, _bits  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'adapter_postln.npz')


def _report(name, worst):
    print(f'\n[adapter postln] {name}: {worst}')


def _module(top, blocks, D, d, heads, ffn, residual, norm_first):
    from eventclip_amd.adapter import TransformerAdapter
    ad = TransformerAdapter(in_dim=D, d_model=d, num_heads=heads, ffn_dim=ffn, norm_first=norm_first, num_layers=len(blocks),
                            residual=float(residual))
    ad.load_state_dict(pr.state_dict_of(top, blocks))
    return ad.cuda()


# ---------------------------------------------------------------------------------------------------------------
# serving kernel
# ---------------------------------------------------------------------------------------------------------------
def _serve(case, norm_first, layers=None):
    B, T, D, d, heads, ffn, L, r = case
    L = layers or L
    top, blocks = fr.adapter_params(D, d, heads, ffn, L, seed=L)
    img, valid, _ = fr.adapter_inputs(B, T, D)
    ad = _module(top, blocks, D, d, heads, ffn, r, norm_first).eval()
    got = ad(img.cuda(), valid.cuda()).cpu()
    ref = (fr.adapter_forward if norm_first else pr.postln_forward)(fr.A64, img, valid, top, blocks, heads, r)[0]
    err = (got.double() - ref).abs()
    worst = float((err / (pr.SERVE_ATOL + pr.SERVE_RTOL * ref.abs())).max())
    _report(f'serve {case} norm_first={norm_first} layers={L}', f'worst error / tolerance = {worst:.4f} (all rows)')
    torch.testing.assert_close(got.double(), ref, rtol=pr.SERVE_RTOL, atol=pr.SERVE_ATOL)     # every row, padded views too


@pytest.mark.parametrize('case', pr.SERVE_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_serving_post_ln_matches_float64(case, hip):
    _serve(case, False)


@pytest.mark.parametrize('case', pr.SERVE_CASES[3:], ids=lambda c: 'x'.join(map(str, c)))
def test_serving_pre_ln_at_eight_layers(case, hip):
    _serve(case, True, layers=8)


def test_serving_matches_the_reference_fixture(hip):
    z = np.load(GOLDEN)
    geo = pr.FIXTURE_GEOMETRY
    from eventclip_amd.adapter import TransformerAdapter
    ad = TransformerAdapter(in_dim=geo['D'], d_model=geo['d'], num_heads=geo['heads'], ffn_dim=geo['ffn'], norm_first=False,
                            num_layers=geo['layers'], residual=float(z['residual']))
    ad.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')})
    valid = torch.from_numpy(z['valid'])
    got = ad.cuda().eval()(torch.from_numpy(z['feats']).cuda(), valid.cuda()).cpu()
    torch.testing.assert_close(got[valid], torch.from_numpy(z['out'])[valid], rtol=pr.SERVE_RTOL, atol=pr.SERVE_ATOL)


# ---------------------------------------------------------------------------------------------------------------
# training, stage by stage
# ---------------------------------------------------------------------------------------------------------------
class PostAdapter(Adapter):
    """tests/test_fewshot_edges_gpu.py's driver of ec_adapter_train_forward / _backward with the layout set."""

    def __init__(self, *a, post_norm=1, **k):
        super().__init__(*a, **k)
        self.w.post_norm = post_norm


def _same_bits(a, g1, d1, d_out, p):
    g2, d2 = a.backward(d_out, p, SEED)
    for k, v in fr.flat_grads(g1, d1).items():
        assert torch.equal(_bits(v), _bits(fr.flat_grads(g2, d2)[k])), f'second backward: {k} differs'


@pytest.mark.parametrize('case', fr.adapter_cases(), ids=lambda c: f'B{c[0]}T{c[1]}-{"x".join(map(str, c[2]))}-p{c[4]}-r{c[5]}')
def test_post_ln_stage_by_stage(case, hip):
    """layers = 1: every tape slot and out after the forward, every scratch slot, parameter gradient and d_img_feats after
    the backward; a second backward gives the same bits and the tape stays bit-unchanged."""
    B, T, geom, layers, p, r = case
    a = PostAdapter(B, T, geom, layers, r)
    img, valid, d_out = fr.adapter_inputs(B, T, geom[0])
    out = a.forward(img, valid, p, SEED)
    tape = a.tape_views()
    worst = pr.check_postln_forward(img, valid, a.top, a.blocks, geom[2], r, p, SEED, out, tape, f'forward {case}')
    before = a.tape.clone()
    grads, d_img = a.backward(d_out, p, SEED)
    wb = pr.check_postln_backward(img, valid, a.top, a.blocks, geom[2], r, p, SEED, tape, d_out, grads, d_img, a.scratch_views(),
                                  f'backward {case}')
    for k, v in wb.items():
        worst[k] = max(worst.get(k, 0.0), v)
    _same_bits(a, grads, d_img, d_out, p)
    assert torch.equal(before.view(torch.int32), a.tape.view(torch.int32)), 'the backward wrote into the tape'
    _report(f'stages {case}', {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize('layers,shape,p,r', fr.E2E_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_post_ln_deep(layers, shape, p, r, hip):
    """layers 2 and 8: the forward slots of every layer stage by stage; every gradient against the float64 replay of the whole
    chain (equal to torch autograd: tests/test_adapter_postln_cpu.py) within the training steps' 3e-4 of the largest element;
    two backwards over one tape give equal bits."""
    B, T, geom = shape
    a = PostAdapter(B, T, geom, layers, r)
    img, valid, d_out = fr.adapter_inputs(B, T, geom[0])
    out = a.forward(img, valid, p, SEED)
    worst = pr.check_postln_forward(img, valid, a.top, a.blocks, geom[2], r, p, SEED, out, a.tape_views(), f'forward L={layers}')
    grads, d_img = a.backward(d_out, p, SEED)
    _, tape64 = pr.postln_forward(fr.A64, img, valid, a.top, a.blocks, geom[2], r, p, SEED)
    g64, di64, _ = pr.postln_backward(fr.A64, img, valid, a.top, a.blocks, geom[2], r, tape64, d_out, p, SEED)
    worst['chain / 3e-4 max'] = pr.assert_e2e(0.0, None, fr.flat_grads(grads, d_img), 0.0, None, fr.flat_grads(g64, di64),
                                              f'L={layers}')
    _same_bits(a, grads, d_img, d_out, p)
    _report(f'deep layers={layers} {shape}', {k: round(v, 4) for k, v in worst.items()})


def test_layout_value_is_checked_and_zero_is_pre_ln(hip):
    """post_norm = 2 is refused; a struct left at its zero initialisation runs the pre-LN launches (the bits of an explicit 0)."""
    geom = fr.GEOMETRIES[0]
    img, valid, _ = fr.adapter_inputs(2, 3, geom[0])
    bad = PostAdapter(2, 3, geom, 1, 0.8, post_norm=2)
    rc, _ = bad.forward(img, valid, 0.0, 1, expect_fail=True)
    from eventclip_amd import _lib
    assert rc != 0 and b'geometry' in _lib.lib().ec_last_error()
    pre, post = Adapter(2, 3, geom, 1, 0.8), PostAdapter(2, 3, geom, 1, 0.8)
    o_pre, o_post = pre.forward(img, valid, 0.0, 1), post.forward(img, valid, 0.0, 1)
    fr.check_adapter_forward(img, valid, pre.top, pre.blocks, geom[2], 0.8, 0.0, 1, o_pre, pre.tape_views(), 'zero = pre-LN')
    assert not torch.equal(o_pre, o_post)


# ---------------------------------------------------------------------------------------------------------------
# training, end to end
# ---------------------------------------------------------------------------------------------------------------
_YARD = {}


def _problem(i, agg, probs):
    """Shape i of E2E_SHAPES behind the post-LN adapter and its float64 autograd yardstick, computed once."""
    if (i, agg, probs) not in _YARD:
        c = pr.max_case(i, 'post')
        _YARD[i, agg, probs] = (c, pr.max_yardstick(c, 'post', agg, probs))
    return _YARD[i, agg, probs]


@pytest.mark.parametrize('agg,probs', [('sum', False), ('mean', True)])
@pytest.mark.parametrize('i', range(len(pr.E2E_SHAPES)))
def test_post_ln_training_end_to_end(i, agg, probs, hip):
    """fs_trans_loss_grad and FSCLIPClassifier(norm_first=False) -> calc_train_loss -> loss.backward() against float64
    autograd; the fused step's adapter gradients equal the autograd ops' bit for bit."""
    from eventclip_amd import train
    B, T, D, K, d, heads, ffn, layers = pr.E2E_SHAPES[i]
    c, y = _problem(i, agg, probs)
    f, v, lab, text = c['feats'].cuda(), c['valid'].cuda(), c['labels'].cuda(), c['text'].cuda()
    ad = _module(c['top'], c['blocks'], D, d, heads, ffn, c['residual'], False)
    loss, grads, logits = train.fs_trans_loss_grad(f, v, lab, text, pr.LOGIT_SCALE, ad, agg, probs, return_logits=True)
    w1 = pr.assert_e2e(loss, logits, grads, y['loss'], y['logits'], y['grads'], f'fused {pr.E2E_SHAPES[i]} {agg}')
    clf = _classifier(dict(adapter_type='text-trans', in_dim=D, d_model=d, num_heads=heads, ffn_dim=ffn, num_layers=layers,
                           residual=c['residual'], norm_first=False), K, agg, probs)
    clf.adapter.load_state_dict(pr.state_dict_of(c['top'], c['blocks']))
    clf.text_feats = torch.nn.Parameter(text.clone())
    clf.logit_scale = pr.LOGIT_SCALE
    clf = clf.cuda()
    clf.train()
    clf.adapter.TRAIN_DROPOUT = 0.0                        # train mode, dropout forced to 0: the function float64 differentiates
    _inject(clf, f, v)
    data = {'valid_mask': v, 'label': lab}
    out = clf(data)
    ce = clf.calc_train_loss(data, out)['ce_loss']
    ce.backward()
    got = {k: p.grad for k, p in clf.adapter.named_parameters()}
    got['text_feats'] = clf.text_feats.grad
    w2 = pr.assert_e2e(ce.detach(), out['logits'].detach(), got, y['loss'], y['logits'], y['grads'], f'autograd {agg}')
    # (the two heads differ -- classify runs a hi + lo product -- so bit equality of the adapter's share is the next test's)
    _report(f'e2e {pr.E2E_SHAPES[i]} {agg} probs={probs}', f'worst gradient error / (3e-4 max): fused {w1:.4f}, autograd {w2:.4f}')


@pytest.mark.parametrize('i', range(len(pr.E2E_SHAPES)))
def test_fused_step_equals_the_autograd_ops_bit_for_bit(i, hip):
    """ec_fs_trans_loss_grad and ec_adapter_train_forward / _backward share one launch sequence: the ops' forward gives the
    fused step's mixed features, and from the fused head's upstream gradient -- here rebuilt with the head's own kernels via
    ft_loss_grad on the ops' output -- the ops' backward gives the fused step's adapter gradients bit for bit."""
    from eventclip_amd import ft, train
    B, T, D, K, d, heads, ffn, layers = pr.E2E_SHAPES[i]
    c, _ = _problem(i, 'sum', False)
    f, v, lab, text = c['feats'].cuda(), c['valid'].cuda(), c['labels'].cuda(), c['text'].cuda()
    ad = _module(c['top'], c['blocks'], D, d, heads, ffn, c['residual'], False)
    loss, grads = train.fs_trans_loss_grad(f, v, lab, text, pr.LOGIT_SCALE, ad, 'sum', False)
    params = [p.detach().clone().requires_grad_(True) for p in ad.parameters()]
    rows = f.reshape(B * T, D)
    out, _ = torch.ops.eventclip_hip.adapter_train_fwd(rows, _idx(v), params, d, heads, ffn, layers, c['residual'], 0.0, 0, 1)
    loss2, gimg, gtext, _ = ft.ft_loss_grad(out.detach(), v, lab, text, pr.LOGIT_SCALE, 'sum', False)
    assert torch.equal(_bits(loss.reshape(1)), _bits(loss2.reshape(1))) and torch.equal(_bits(grads['text_feats']), _bits(gtext))
    out.backward(gimg.reshape(out.shape))
    for (k, _), p in zip(ad.named_parameters(), params):
        assert torch.equal(_bits(grads[k]), _bits(p.grad)), f'{k}: the fused step and the autograd ops differ'


def test_opcheck_and_the_default_layout(hip):
    """torch.library.opcheck on both ops with the layout argument; the pre-LN value passed explicitly gives the bits of the
    call without it."""
    ops = torch.ops.eventclip_hip
    B, T, D, K, d, heads, ffn, layers = pr.E2E_SHAPES[0]
    c, _ = _problem(0, 'sum', False)
    f, v = c['feats'].cuda(), c['valid'].cuda()
    ad = _module(c['top'], c['blocks'], D, d, heads, ffn, 0.5, False)
    rows, idx = f.reshape(B * T, D), _idx(v)
    params = [p.detach().clone().requires_grad_(True) for p in ad.parameters()]
    geo = (d, heads, ffn, layers, 0.5, 0.1, 11)
    torch.library.opcheck(ops.adapter_train_fwd.default, (rows.clone().requires_grad_(True), idx, params) + geo + (1,))
    plain = [p.detach() for p in params]
    out, tape = ops.adapter_train_fwd(rows, idx, plain, *geo, 1)
    mask = (1 << len(plain)) | 0b1011
    torch.library.opcheck(ops.adapter_train_bwd.default, (rows, idx, plain, tape, torch.randn_like(out)) + geo + (mask, 1))
    o_def, t_def = ops.adapter_train_fwd(rows, idx, plain, *geo)
    o_pre, t_pre = ops.adapter_train_fwd(rows, idx, plain, *geo, 0)
    assert torch.equal(_bits(o_def), _bits(o_pre)) and torch.equal(t_def, t_pre) and not torch.equal(o_def, out)
    d_out = torch.randn_like(out)
    g_def = ops.adapter_train_bwd(rows, idx, plain, t_def, d_out, *geo, mask)
    g_pre = ops.adapter_train_bwd(rows, idx, plain, t_pre, d_out, *geo, mask, 0)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(g_def, g_pre))
    # and under autograd, where the dispatcher drops an argument that equals its default before the backward sees the call
    got = []
    for tail in ((), (0,), (1,)):
        ps = [p.detach().clone().requires_grad_(True) for p in params]
        o, _ = ops.adapter_train_fwd(rows, idx, ps, *geo, *tail)
        o.backward(d_out)
        got.append([p.grad for p in ps])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got[0], got[1]))
    assert not all(torch.equal(a, b) for a, b in zip(got[0], got[2]))


def test_trainer_step_on_a_post_ln_eight_layer_adapter_then_serve(hip):
    """One AdapterTrainer step, then the eval forward (the serving kernel at 8 layers) agrees with the train op at p = 0
    within the serving tolerance."""
    from eventclip_amd.train import AdapterTrainer
    B, T, D, K, d, heads, ffn, layers = pr.E2E_SHAPES[1]
    assert layers == 8
    c, _ = _problem(1, 'sum', False)
    f, v, lab = c['feats'].cuda(), c['valid'].cuda(), c['labels'].cuda()
    clf = _classifier(dict(adapter_type='text-trans', in_dim=D, d_model=d, num_heads=heads, ffn_dim=ffn, num_layers=layers,
                           residual=0.5, norm_first=False), K, 'mean', False)
    clf.adapter.load_state_dict(pr.state_dict_of(c['top'], c['blocks']))
    clf.text_feats = torch.nn.Parameter(c['text'].cuda())
    clf = clf.cuda()
    before = {k: p.detach().clone() for k, p in clf.adapter.named_parameters()}
    loss = AdapterTrainer(clf, lr=1e-3, total_steps=10).step(f, v, lab)
    assert np.isfinite(float(loss)) and all(not torch.equal(before[k], p) for k, p in clf.adapter.named_parameters())
    ad = clf.adapter
    served = ad.eval()(f, v)
    ad.train()
    ad.TRAIN_DROPOUT = 0.0
    with torch.enable_grad():
        trained = ad(f, v)
    torch.testing.assert_close(served, trained.detach(), rtol=pr.SERVE_RTOL, atol=pr.SERVE_ATOL)
