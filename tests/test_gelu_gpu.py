"""The exact GELU, x Phi(x) (cfg['activation'] = 'gelu': open_clip's CLIPs without a -quickgelu suffix, Hugging Face
hidden_act "gelu"), on the MI355X, through every layer that applies an activation: the GEMM epilogues and their K-batched
form (ec_gemm_args.activation = 1), ec_split16(gelu = 2), every chain of the two towers, the training tower under
VisualTower / FTTrainer / loss.backward(), and the loaders.

Yardsticks: float64 x Phi(x) from erfc with the per-element bounds of tests/gelu_ref.py for the kernels; for the towers the
project's own oracle with its module-level activation swapped (tests/test_gelu_ref_cpu.py holds that swap to torch.nn.GELU
modules and to Hugging Face's CLIP), under the bounds the existing tests of each chain use for QuickGELU.  Every tower case
must also sit more than ten times its bound away from the OTHER activation's oracle: a swap cannot pass.

Weights of the tower cases: seeded random weights with the c_fc biases moved to the negative side (-2 in the serving cases,
-1.5 in the fine-tuning ones) and a branch gain on c_proj.  At the init scale the pre-activations are N(0, 0.7) around zero,
where the two activations differ in second order only (x Phi(x) - x sigmoid(1.702 x) = -0.027 x^2 + ...: an even function, whose
contributions through a zero-mean c_proj mostly average out) and the features of the two networks are 5e-3 .. 1e-2 apart --
inside ten times the default bound.  On the negative side, where trained MLPs sit, they differ in first order: the oracles of
the serving cases are 5.9e-2 (image) and 9.8e-2 (text) apart.  The weights were chosen on the oracles' distance and on the
error of the EXISTING QuickGELU chains on them (3.7e-4 default, 6.5e-4 the 16-bit text tower: inside their 1e-3 with room;
with a query / key gain of 2 on top the existing default chain itself is at 2.3e-3), never on the new path's."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gelu_ref as ref  # noqa: E402
import gemm_ref as gr  # noqa: E402
import rowops_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT = gr.DTYPES
NAN = float('nan')


@contextlib.contextmanager
def swapped_oracle():
    """oracle.clip_ref with x Phi(x) in place of QuickGELU (_blocks calls the module-level name) for the block's duration."""
    from oracle import clip_ref
    mp = pytest.MonkeyPatch()
    mp.setattr(clip_ref, 'quick_gelu', ref.exact_gelu)
    try:
        yield clip_ref
    finally:
        mp.undo()


def _ops():
    from eventclip_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------
# 1. GEMM epilogues
# ---------------------------------------------------------------------------------------------------------------
MODES = {
    'gelu16': dict(epi='gelu16'),
    'gelu16+lo16': dict(epi='gelu16', seg='both', lo_out='16'),                 # the f16 / bf16 lo output: LO_16, SEG 1
    'gelu16+e4m3': dict(epi='gelu16', seg='a_lo8', lo_out='e4m3'),              # e4m3 lo products and lo output: LO_E4M3, SEG 2
    'gelu16_ln@1': dict(epi='gelu16_ln', stride=1),                             # statistics through LDS
    'gelu16_ln@5': dict(epi='gelu16_ln', stride=5),                             # ... read from memory
    'gelu16_save': dict(epi='gelu16_save'),
    'gelu_bwd16': dict(epi='gelu_bwd16'),
}
GEMM_M, GEMM_N = (1, 255, 257), (16, 272)


def _launch(c, mode, ws=None, lead=64, activation='gelu'):
    """One ops.gemm launch of the case into fresh buffers (the conventions of tests/test_gemm_edges_gpu.py) -> bufs."""
    import test_gemm_edges_gpu as E
    bufs = gr.case_buffers(c, 'cuda')
    epi, kw = c['epi'], {}
    if 'aux' in bufs:
        kw['aux'] = bufs['aux'][1]
    if 'aux8' in bufs:
        kw['aux8'] = (bufs['aux8'][1], c['aux_exp'])
    if epi.endswith('_ln'):
        stride = mode.get('stride', 1)
        kw.update(row_stats=E._stats_array(c['stats'], stride), col_sums=c['colsum'], row_stats_stride=stride)
    for k in ('A_lo', 'W_lo'):
        if k in c:
            kw[k] = gr.window(c[k], lead=lead if k == 'A_lo' else 64 - lead)
    for k in ('A_lo8', 'W8', 'A8', 'W_lo8'):
        if k in c:
            kw[k] = c[k]
    _ops().gemm(gr.window(c['A'], lead=lead), gr.window(c['W'], lead=64 - lead), c['bias'], epi, out=bufs['out'][1], ws=ws,
                activation=activation, **kw)
    return bufs


def _run(c, mode, what, acc_s=None, ws=None):
    specs = ref.case_specs(c, acc_s)
    bufs = _launch(c, mode, ws)
    gr.verify(c, specs, bufs, what)
    return bufs


def _case(mode, dt, M, N, K, family, rot=0):
    return gr.case_to(gr.make_case(mode['epi'], dt, M, N, K, family, rot, mode.get('seg'), mode.get('lo_out')), 'cuda')


# (the e4m3 lo products are f16 only)
@pytest.mark.parametrize('mode,dt', [(m, d) for m in MODES for d in DT if d == 'float16' or MODES[m].get('lo_out') != 'e4m3'])
def test_gemm_epilogues(mode, dt, hip):
    """ec_gemm(activation = 1) at M in {1, 255, 257} x N in {16, 272}, one and three K tiles (64 deep; 128 deep for the e4m3
    segments): gemm_ref's random family (outlier column, cancelling and zero rows; M = 1 at the rotations that bring those
    rows to the front) and the GELU tails as the bias (the saved pre-activation for gelu_bwd16), outputs NaN-prefilled with
    padding columns and a guard row that must come back untouched."""
    e4m3 = MODES[mode].get('lo_out') == 'e4m3'
    mode, dt = MODES[mode], DT[dt]
    Mx, Nx = max(GEMM_M), max(GEMM_N)
    for K in ((128, 384) if e4m3 else (64, 192)):
        for family in ('random', 'tails'):
            full = _case(mode, dt, Mx, Nx, K, family)
            acc, S = gr.product(gr.case_segments(full))
            for M in GEMM_M:
                for N in GEMM_N:
                    _run(gr.slice_case(full, 0, M, N), mode, f'{family} M={M} N={N} K={K}', (acc[:M, :N], S[:M, :N]))
            if family == 'tails' and mode['epi'] != 'gelu_bwd16':
                # far negative: zero or tiny, never NaN or the input; far positive: the input
                bufs = _run(full, mode, f'tails K={K}', (acc, S))
                tails = gr.tails_bias(Nx).cuda()
                out = bufs['out'][1].float()
                assert float(out[:, tails <= -20].abs().max()) <= 2.0 ** -24
                if mode['epi'] != 'gelu16_ln':
                    assert torch.equal(out[:, tails >= 20], tails[tails >= 20].to(dt).float().expand(Mx, -1))
        for rot in gr.rotations(1)[1:]:
            full = _case(mode, dt, 1, Nx, K, 'random', rot)
            for N in GEMM_N:
                _run(gr.slice_case(full, 0, 1, N), mode, f'random rot={rot} M=1 N={N} K={K}')


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('epi', ['gelu16', 'gelu16_save', 'gelu_bwd16'])
def test_gemm_k_batched_form(epi, dt, hip):
    """The K-batched form (kbatch_fixup_kernel) at gemm_ref.WS_SHAPES[1] = (257, 272) with four K tiles; that it ran shows in
    the scratch."""
    import test_gemm_edges_gpu as E
    mode, dt = MODES[epi], DT[dt]
    M, N = gr.WS_SHAPES[1]
    batches = E._ws_batches(M, N, 4, E._cus())
    assert batches > 1
    ws32 = torch.empty(batches * M * N, dtype=F32, device='cuda')
    for family in ('random', 'tails'):
        ws32.fill_(NAN)
        _run(_case(mode, dt, M, N, 256, family), mode, f'K-batched {family}', ws=ws32.view(torch.uint8))
        assert bool(torch.isfinite(ws32).all()), 'not the K-batched form'


def test_gemm_refuses_an_activation_it_would_not_read(hip):
    ops = _ops()
    A = torch.zeros(16, 64, dtype=F16, device='cuda')
    W = torch.zeros(16, 64, dtype=F16, device='cuda')
    for epi in ('store16', 'store32'):
        with pytest.raises(RuntimeError, match=r'args\.activation goes with'):
            ops.gemm(A, W, None, epi, activation='gelu')
    with pytest.raises(RuntimeError, match=r'unknown args\.activation 7'):
        ops.gemm(A, W, None, 'gelu16', activation=7)
    ops.gemm(A, W, None, 'store16', activation='quick_gelu')          # 0: what every older caller passes


# ---------------------------------------------------------------------------------------------------------------
# 2. the row kernel
# ---------------------------------------------------------------------------------------------------------------
SPLIT_VECTORS = (1, 4, 1027)


@pytest.mark.parametrize('dt', list(DT))
def test_split16_exact_gelu(dt, hip):
    """ec_split16(gelu = 2): hi and hi + lo against float64 at n = 1, 4 and 1027 float4 vectors (the kernel's unit: one
    thread's worth, one wave's sixteenth, four workgroups and three threads; ec_split16 takes multiples of 4 elements and
    refuses anything else), nothing written behind the last element; the negative tail (-6, -8, -12 among the inputs) of the
    right sign and size, i.e. Phi computed without cancellation; in bf16, which can hold them, inputs whose square overflows."""
    from eventclip_amd import _lib
    lib, s, dtype = _lib.lib(), _lib.stream_ptr(), DT[dt]
    code = _lib.EC_F16 if dtype == F16 else _lib.EC_BF16
    for nv in SPLIT_VECTORS:
        n = 4 * nv
        x = ref.split_input(n, 'cuda', huge=dtype == BF16 and nv > 4)
        hi = torch.full((n + 64,), NAN, dtype=dtype, device='cuda')
        lo = torch.full((n + 64,), NAN, dtype=dtype, device='cuda')
        _lib.check(lib.ec_split16(_lib.ptr(x), n, 2, _lib.ptr(hi), _lib.ptr(lo), code, s), 'ec_split16')
        assert bool(torch.isnan(hi[n:]).all() and torch.isnan(lo[n:]).all()), f'n={n}: elements behind the last written'
        hi, lo = hi[:n], lo[:n]
        assert bool(torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all())
        want, b_hi, b_pair = ref.split_bounds(x, dtype, dtype)
        pair = hi.double() + lo.double()
        assert rr.excess(hi, want, b_hi) <= 0, f'{dt} n={n}: hi {rr.excess(hi, want, b_hi):.3e} over the bound'
        assert rr.excess(pair, want, b_pair) <= 0, f'{dt} n={n}: hi + lo {rr.excess(pair, want, b_pair):.3e} over the bound'
        if nv > 4:
            ref.tail_check(pair, x, gr.FLOOR16 if dtype == F16 else 0.0, f'{dt} n={n}')
        zero = x == 0
        assert bool((hi[zero] == 0).all() and (lo[zero] == 0).all())
    x = torch.zeros(8, device='cuda')
    h = torch.zeros(8, dtype=dtype, device='cuda')
    for n_bad in (1, 1027):
        assert lib.ec_split16(_lib.ptr(x), n_bad, 2, _lib.ptr(h), _lib.ptr(h), code, s) == _lib.EC_ERR_INVALID
        assert b'multiple of 4' in lib.ec_last_error()
    assert lib.ec_split16(_lib.ptr(x), 8, 3, _lib.ptr(h), _lib.ptr(h), code, s) == _lib.EC_ERR_INVALID
    assert b'gelu=3' in lib.ec_last_error()


# ---------------------------------------------------------------------------------------------------------------
# 3. towers
# ---------------------------------------------------------------------------------------------------------------
N_IMG = 3


def shifted(sd, text_branch=2.0, visual_branch=1.0, shift=-1.5):
    """The docstring's weights: every c_fc bias moved by ``shift``; the text tower's c_proj doubled (random_state_dict's
    branch_gain reaches the vision tower only); visual_branch: the vision tower's c_proj (the fine-tuning cases, whose
    weights come without a branch gain)."""
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith('mlp.c_fc.bias'):
            out[k] = v + shift
        elif k.endswith('mlp.c_proj.weight'):
            out[k] = v * (visual_branch if 'visual' in k or not k.startswith('transformer.') else text_branch)
    return out


@functools.lru_cache(maxsize=None)
def tower_case():
    """-> (cfg, sd, img, tok, oracle features {(tower, activation): fp32}) of ViT-B/32, 3 blocks, one text block."""
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg = eclip.arch_config('ViT-B/32', layers=3, text_layers=1, vocab_size=1024)
    sd = shifted(eclip.random_state_dict(cfg, seed=3, branch_gain=3.0), shift=-2.0)
    img = torch.randn(N_IMG, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    t = eclip.synthetic_tokens(9, seed=3)
    tok = torch.where(t == 49407, torch.tensor(1023), torch.where(t == 49406, torch.tensor(1022), t % 1000)).int()
    want = {('image', 'quick_gelu'): clip_ref.encode_image(sd, cfg, img), ('text', 'quick_gelu'): clip_ref.encode_text(sd, cfg, tok)}
    with swapped_oracle():
        want[('image', 'gelu')] = clip_ref.encode_image(sd, cfg, img)
        want[('text', 'gelu')] = clip_ref.encode_text(sd, cfg, tok)
    return cfg, sd, img, tok, want


TOWER_CASES = {
    'default (folded)': ('image', dict(), 1e-3),
    'ln_folded=False': ('image', dict(ln_folded=False), 1e-3),
    'image_precise': ('image', dict(image_precise=True), 2e-5),
    'split-operand blocks, e4m3 lo': ('image', dict(image_precise_blocks=2, image_precise_attn_blocks=1, image_lo_fp8=True), 1e-3),
    'split-operand blocks, 16-bit lo': ('image', dict(image_precise_blocks=2, image_precise_attn_blocks=1, image_lo_fp8=False), 1e-3),
    'low_latency': ('image', dict(low_latency=True), 1e-3),
    'text, precise': ('text', dict(text_precise=True), 2e-5),
    'text, 16-bit': ('text', dict(text_precise=False), 1e-3),
}


def _features(cfg, sd, tower, kw, activation, img, tok):
    from eventclip_amd import clip as eclip
    m = eclip.CLIP(dict(cfg, activation=activation), sd, dtype='float16', **kw).cuda().eval()
    if tower == 'image' and kw.get('image_lo_fp8') is not None:
        assert m._pack()['vit'].lo_fp8 == int(kw['image_lo_fp8'])
    return (m.encode_image(img.cuda()) if tower == 'image' else m.encode_text(tok.cuda())).cpu()


@pytest.mark.parametrize('case', list(TOWER_CASES))
def test_tower_chains(case, hip):
    """Every chain with activation = 'gelu' against the swapped oracle: inside the bound the existing test of that chain uses
    for QuickGELU; at most 1.5 x the error of the SAME weights run with 'quick_gelu' against the unswapped oracle, + 1e-4 (the
    yardstick is the existing path); more than 10 x the bound away from the other activation's oracle."""
    tower, kw, bound = TOWER_CASES[case]
    cfg, sd, img, tok, want = tower_case()
    got = _features(cfg, sd, tower, kw, 'gelu', img, tok)
    quick = _features(cfg, sd, tower, kw, 'quick_gelu', img, tok)
    assert torch.isfinite(got).all()
    e_gelu, e_quick = ref.rel_err(got, want[(tower, 'gelu')]), ref.rel_err(quick, want[(tower, 'quick_gelu')])
    away = ref.rel_err(got, want[(tower, 'quick_gelu')])
    print(f'\n[{case}] gelu vs swapped oracle {e_gelu:.2e}, quick_gelu vs oracle {e_quick:.2e} (bound {bound:.0e}); '
          f'gelu vs the QuickGELU oracle {away:.2e}')
    assert e_gelu < bound
    assert e_gelu < 1.5 * e_quick + 1e-4
    assert away > 10 * bound


# ---------------------------------------------------------------------------------------------------------------
# 4. fine-tuning
# ---------------------------------------------------------------------------------------------------------------
FT_BRANCH = 4.0      # c_proj of the fine-tuning cases' vision towers (two blocks at the init scale: see the module docstring)


def _train_tower(cfg, sd, dtype='float16'):
    from eventclip_amd import clip as eclip, ft
    model = eclip.CLIP(cfg, sd, dtype=dtype, full_last_block=True, ln_folded=False, q_scaled=False).cuda()
    return model, ft.VisualTower(model)


@pytest.mark.parametrize('name,dtype', [('tiny', 'float16'), ('tiny', 'bfloat16'), ('b32_2blocks', 'float16')])
def test_visual_tower_forward_and_backward(name, dtype, hip):
    """VisualTower.forward / .backward with activation = 'gelu' against float64 autograd through the swapped oracle, under
    the bounds of test_ft_train_gpu.test_tower_gradients_match_the_oracle; the forward is the inference forward, bit for
    bit; the features are not QuickGELU's."""
    import test_ft_train_gpu as T
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg, n = T.CONFIGS[name]
    cfg = dict(cfg, activation='gelu')
    sd = shifted(eclip.random_state_dict(cfg, seed=1), visual_branch=FT_BRANCH)
    model, tower = _train_tower(cfg, sd, dtype)
    assert tower._vit.activation == 1 and tower._vit_t.activation == 1
    torch.manual_seed(5)
    imgs = torch.randn(n, 3, cfg['image_size'], cfg['image_size'])
    d_feats = torch.randn(n, cfg['embed_dim'])
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith('visual.')}
    quick = clip_ref.encode_image(sd, cfg, imgs)
    with swapped_oracle():
        want_feats = clip_ref.encode_image_autograd(leaves, cfg, imgs.double())
        want_feats.backward(d_feats.double())
    patches = T._patchify(tower, imgs)
    feats = tower.forward(patches)
    assert torch.equal(feats, model.encode_patches(patches))
    tol_f = 1e-3 if dtype == 'float16' else 1e-2
    e, away = ref.rel_err(feats.cpu(), want_feats.detach()), ref.rel_err(feats.cpu(), quick)
    print(f'\n[{name} {dtype}] features vs swapped oracle {e:.2e}, vs the QuickGELU oracle {away:.2e}')
    assert e < tol_f and away > (10 if dtype == 'float16' else 5) * tol_f       # (bf16: 5e-2; the oracles are 7e-2 apart)
    names = list(tower.master)
    grads, flat = tower.backward(d_feats.cuda(), names)
    assert torch.isfinite(flat).all()
    tol, cos = (T.GRAD_REL, 0.9995) if dtype == 'float16' else (8e-2, 0.995)
    W, bad = cfg['width'], {}
    for k in names:
        want = leaves['visual.' + k].grad
        got = grads[k].reshape(want.shape).cpu().double()
        if k.endswith('attn.in_proj_bias'):       # zero key-bias gradient in exact arithmetic: q, v relatively, k absolutely
            ok = T.rel_l2(torch.cat([got[:W], got[2 * W:]]), torch.cat([want[:W], want[2 * W:]])) < tol and \
                float(got[W:2 * W].abs().max()) < 1e-2 * float(want.abs().max())
        else:
            ok = T.rel_l2(got, want) < tol and T.cosine(got, want) > cos
        if not ok:
            bad[k] = (T.rel_l2(got, want), T.cosine(got, want))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def ft_case(kind):
    """A case in the form of test_oracle_ft_train.case on the geometry, images, labels and text features of the ft_train
    fixture's 'full' case, with activation = 'gelu', shifted c_fc biases and kind = 'full' | 'bias' (only_bias) | 'lora'
    (qkvo-4, non-zero up factors); its float64 expectations through the swapped oracle."""
    import test_ft_train_gpu as T
    from oracle import ft_train as oft
    z, c = T._golden_case('full')
    visual = shifted(c['visual'], visual_branch=FT_BRANCH)
    flags = dict(only_conv1=False, only_bias=kind == 'bias', only_ln=False, only_cls_fc=False, only_cls_token=False)
    clip_dict = dict(lora='qkvo-4' if kind == 'lora' else -1, **flags)
    if kind == 'lora':
        g = torch.Generator().manual_seed(17)
        visual = oft.inject_lora(visual, 'qkvo-4', g)
        visual = {k: (torch.randn(v.shape, generator=g) * 0.02 if 'lora_up' in k else v) for k, v in visual.items()}
    train = oft.trainable_names(visual, clip_dict)
    names = sorted(['model.visual.' + k for k in train] + (['text_feats'] if c['prompt'] else []))
    sd = {'model.visual.' + k: v for k, v in visual.items()}
    sd['text_feats'] = c['text']
    c = dict(c, cfg=dict(c['cfg'], activation='gelu'), visual=visual, clip_dict=clip_dict, trainable=names, sd=sd)
    args = (c['visual'], c['cfg'], c['imgs'], c['valid'], c['labels'], c['text'], 100.0, c['agg'], c['probs_loss'])
    quick_feats = oft.loss_and_grads(*args, train=train, text_trainable=c['prompt'])[3]
    with swapped_oracle():
        loss, grads, _, feats = oft.loss_and_grads(*args, train=train, text_trainable=c['prompt'])
    grads = {('text_feats' if k == 'text_feats' else 'model.visual.' + k): v for k, v in grads.items()}
    return c, loss, grads, feats, quick_feats


def _check_step(c, want_loss, want_grads, want_feats, quick_feats, loss, feats, grads, what):
    """The bounds of test_ft_train_gpu.test_training_step_matches_the_reference, on loss, features and every gradient."""
    import test_ft_train_gpu as T
    assert abs(float(loss) - want_loss) < 2e-3 * max(1.0, abs(want_loss)), (what, float(loss), want_loss)
    scale = float(want_feats.abs().max())
    e, away = float((feats.cpu().double() - want_feats).abs().max()), float((feats.cpu().double() - quick_feats).abs().max())
    print(f'\n[{what}] loss {float(loss):.5f} (float64 {want_loss:.5f}); features {e / scale:.2e} of the largest, '
          f'{away / scale:.2e} from QuickGELU\'s')
    assert e < 1e-3 * scale and away > 10 * 1e-3 * scale
    assert sorted(grads) == c['trainable']
    for name in c['trainable']:
        want = want_grads[name]
        got = grads[name].reshape(want.shape).cpu().double()
        if name.endswith('attn.in_proj_bias'):
            W = c['cfg']['width']
            sel = torch.cat([torch.arange(W), torch.arange(2 * W, 3 * W)])
            assert T.rel_l2(got[sel], want[sel]) < T.GRAD_REL, (what, name)
            continue
        assert T.rel_l2(got, want) < T.GRAD_REL and T.cosine(got, want) > 0.9995, (what, name, T.rel_l2(got, want))


@pytest.mark.parametrize('kind', ['full', 'bias', 'lora'])
def test_ft_trainer_step(kind, hip):
    """One FTTrainer step (the fused training path) with activation = 'gelu': full fine-tuning, only_bias, LoRA qkvo-4."""
    import test_ft_train_gpu as T
    from eventclip_amd import ft
    c, want_loss, want_grads, want_feats, quick_feats = ft_case(kind)
    clf = T._classifier_for(c)
    assert clf.model.cfg['activation'] == 'gelu'
    tr = ft.FTTrainer(clf, lr=1e-3, clip_lr=1e-5, total_steps=10 ** 9, warmup_steps_pct=0.0, init_scale=1024.0)
    if tr.lora:
        for k in tr.lora.params:
            tr.lora.params[k].copy_(c['visual'][k].cuda())
        tr.lora.merge()
    assert tr.trainable_names() == c['trainable']
    loss = tr.step({'img': c['imgs'].cuda(), 'valid_mask': c['valid'].cuda(), 'label': c['labels'].cuda()})
    tr.resolve()
    assert not tr.last['skipped']
    _check_step(c, want_loss, want_grads, want_feats, quick_feats, loss, tr.last['feats'], tr.last['grads'], f'FTTrainer {kind}')


@pytest.mark.parametrize('kind', ['full', 'lora'])
def test_autograd_classifier_step(kind, hip):
    """FTCLIPClassifier(autograd=True) with activation = 'gelu': the train-mode features are VisualTower's bit for bit (as
    test_ft_autograd_gpu asserts for QuickGELU), one loss.backward() gives the float64 oracle's gradients, and the ops give
    VisualTower.backward's bits."""
    import test_ft_autograd_gpu as A
    from eventclip_amd import ft, torch_ops
    c, want_loss, want_grads, want_feats, quick_feats = ft_case(kind)
    clf = A.autograd_classifier(c)
    data = A.batch(c)
    out, feats = A.train_feats(clf, data)
    assert torch.equal(feats.detach(), A._fresh_tower_feats(clf, data))
    loss = clf.calc_train_loss(data, out)['ce_loss']
    loss.backward()
    _check_step(c, want_loss, want_grads, want_feats, quick_feats, loss.detach(), feats.detach(), A.grads_of(clf), f'autograd {kind}')
    if kind == 'full':
        tower = ft.VisualTower(clf.model)
        assert tower._vit_t.activation == 1
        for p in tower.param.values():
            p.requires_grad_(True)
        names = tower.trainable()
        params = [tower.param[k].detach() for k in names]
        patches, _, _ = ft.valid_patches(tower, data)
        d_feats = torch.randn(patches.shape[0], c['cfg']['embed_dim'], device='cuda', generator=torch.Generator('cuda').manual_seed(2))
        h = torch_ops.handle_of(tower)
        f2, tape = torch.ops.eventclip_hip.vit_train_fwd(patches, params, h)
        got = [g.clone() for g in torch.ops.eventclip_hip.vit_train_bwd(patches, params, tape, d_feats, h, [True] * len(params))]
        assert torch.equal(f2, tower.forward(patches))
        want, _ = tower.backward(d_feats, names)
        for k, g in zip(names, got):
            assert torch.equal(g, want[k]), k


# ---------------------------------------------------------------------------------------------------------------
# 5. the seam
# ---------------------------------------------------------------------------------------------------------------
def test_loaders_build_the_same_model(tmp_path, hip):
    """clip.load(path, activation='gelu') on a state-dict file, and clip.load(directory) on the same weights in Hugging Face
    layout (config.json says hidden_act "gelu"), give the features of CLIP(cfg with the activation, sd) bit for bit -- and not
    those of the default load."""
    import test_gelu_ref_cpu as C
    from eventclip_amd import clip as eclip
    cfg, sd, img, tok, _ = tower_case()
    cfg, img = dict(cfg, activation='gelu'), img.cuda()
    direct = eclip.CLIP(cfg, sd).cuda().eval()
    want_i, want_t = direct.encode_image(img), direct.encode_text(tok.cuda())
    path = str(tmp_path / 'open_clip_pytorch_model.bin')
    torch.save(sd, path)
    hf = str(tmp_path / 'hf')
    C.write_hf_directory(hf, sd, cfg, 'gelu')
    for src, kw in ((path, dict(activation='gelu')), (hf, dict())):
        m, pre = eclip.load(src, **kw)
        assert m.cfg['activation'] == 'gelu' and {k: v for k, v in m.cfg.items()} == cfg
        assert torch.equal(m.encode_image(img), want_i) and torch.equal(m.encode_text(tok.cuda()), want_t), src
    plain = eclip.load(path)[0]
    assert plain.cfg['activation'] == 'quick_gelu' and not torch.equal(plain.encode_image(img), want_i)


def test_zero_shot_classifier_end_to_end(hip):
    """Events -> frames -> preprocess -> ViT -> logits with an exact-GELU model handed to ZSCLIPClassifier as it is, against
    the oracle chain with the swapped activation, inside the default bound (the run of __graft_entry__.smoke)."""
    from eventclip_amd import clip as eclip
    from eventclip_amd.clip_cls import ZSCLIPClassifier
    from eventclip_amd.event2img import Event2ImagePipeline
    from eventclip_amd.synthetic import make_batch
    from oracle import classify as oc
    from oracle import events as oe
    from oracle import preprocess as op
    res = (100, 120)
    qa = dict(max_imgs=2, N=30000, split_method='event_count', convert_method='event_histogram', grayscale=True,
              count_non_zero=True, background_mask=False)
    cfg = eclip.arch_config('ViT-B-32', layers=2, text_layers=2)           # open_clip's name: exact GELU
    assert cfg['activation'] == 'gelu'
    sd = shifted(eclip.random_state_dict(cfg, seed=0))
    clip_model = eclip.CLIP(cfg, sd, dtype='float16').cuda().eval()
    tokens = eclip.synthetic_tokens(5, seed=0)
    model = ZSCLIPClassifier(clip_dict=dict(clip_model=clip_model, prompt='a {}', class_names=list('abcde'), agg_func='mean',
                                            class_tokens=tokens)).cuda().eval()
    evs = make_batch(2, [65000, 12500], res, seed=1)
    pipe = Event2ImagePipeline(res, 60000, qa, n_px=224, patch=32, kpad=clip_model.kpad)
    out = model(pipe(evs))
    frames, valid = [], torch.zeros(2, 2, dtype=torch.bool)
    for b, ev in enumerate(evs):
        f = oe.events2frames(ev, 'event_count', 'event_histogram', shape=res, N=30000, grayscale=True, count_non_zero=True,
                             background_mask=False)
        valid[b, :len(f)] = True
        frames.append(f)
    imgs = torch.from_numpy(op.preprocess(np.concatenate(frames), 224))

    def logits(clip_ref):
        feats = clip_ref.encode_image(sd, cfg, imgs)
        text = torch.nn.functional.normalize(clip_ref.encode_text(sd, cfg, tokens), dim=-1)
        return oc.zs_forward(feats, valid, text, 100.0, 'mean')['logits']
    from oracle import clip_ref
    quick = logits(clip_ref)
    with swapped_oracle():
        want = logits(clip_ref)
    got = out['logits'].cpu()
    err, away = ref.rel_err(got, want), ref.rel_err(got, quick)
    print(f'\nlogits vs the swapped oracle {err:.2e}; vs the QuickGELU oracle {away:.2e}')
    assert torch.equal(out['valid_masks'].cpu(), valid)
    assert err < 1e-3 and away > 10 * 1e-3
