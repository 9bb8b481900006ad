"""The vision tower differentiated with respect to its input image on the MI355X: ``ec_unpatchify``, the embedding
stage's data gradient, ``ec_vit_train_backward_image`` end to end against float64 autograd of the oracle, a frozen
tower against a trainable one, ``FTCLIPClassifier(autograd=True)`` with ``img.requires_grad``,
``CLIP.encode_image(differentiable=True)`` and the autograd behaviour of ``eventclip_hip::vit_image_fwd`` / ``_bwd``.

Bounds.  ``ec_unpatchify`` is a permutation: bit for bit.  The embedding stage is held per element to
(u + (W + 2) 2^-24) sum |d_tok| |w| with u = 2^-11 (f16) / 2^-8 (bf16): one operand rounding (d pre to 16 bit; the
weight goes in as hi + lo) plus fp32 accumulation.  ``d_image`` end to end is held to what tests/test_ft_train_gpu.py
holds every parameter gradient to: relative l2 < GRAD_REL with cosine > 0.9995 (f16), 8e-2 with 0.995 (bf16)."""
import ctypes
import functools

import pytest
import torch

import input_grad_ref as R
import test_ft_autograd_gpu as A
import test_ft_train_gpu as T
import test_gelu_gpu as G

pytestmark = pytest.mark.gpu

UNIT = {'float16': 2.0 ** -11, 'bfloat16': 2.0 ** -8}
BOUNDS = {'float16': (T.GRAD_REL, 0.9995), 'bfloat16': (8e-2, 0.995)}
# a tiny tower (width 64, 1 head, 2 layers, image 32, patch 16, n = 3) beside the suite's two ViT-L/14 blocks
E2E = {'tiny32': (T._tiny_cfg(image_size=32, patch=16), 3), 'l14_2blocks': T.CONFIGS['l14_2blocks']}


# ------------------------------------------------------------------------------------------------
# 1. ec_unpatchify alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p,g,n', [(14, 1, 1), (14, 2, 3), (16, 3, 2), (32, 2, 1), (14, 16, 1)])
def test_unpatchify_is_the_reference_permutation_bit_for_bit(hip, p, g, n):
    """fp32 rows with a class row in front of every image's patches (NaN: never read) and columns past 3 p^2 (NaN too),
    into a NaN-prefilled output with a guard region behind it: every element written, nothing beyond."""
    from eventclip_amd import _lib
    torch.manual_seed(p * 100 + g * 10 + n)
    res, S, k = p * g, g * g + 1, 3 * p * p
    ld = (k + 15) // 16 * 16 + 8
    rows = torch.full((n, S, ld), float('nan'))
    rows[:, 1:, :k] = torch.randn(n, S - 1, k)
    want = R.unpatchify(rows[:, 1:, :k].contiguous(), p, res)
    total, guard = n * 3 * res * res, 4096
    out = torch.full((total + guard,), float('nan'), device='cuda')
    _lib.launch('ec_unpatchify', rows.cuda(), ld, S, 1, n, res, p, out)
    got = out.cpu()
    assert torch.equal(got[:total].view(n, 3, res, res), want)          # finite everywhere: every element was written
    assert bool(torch.isnan(got[total:]).all())
    # rows without a class row (seq = patches, row_off = 0) and a dense row stride
    dense = rows[:, 1:, :k].contiguous()
    out2 = torch.full((total + guard,), float('nan'), device='cuda')
    _lib.launch('ec_unpatchify', dense.cuda(), k, S - 1, 0, n, res, p, out2)
    assert torch.equal(out2.cpu()[:total].view(n, 3, res, res), want) and bool(torch.isnan(out2[total:]).all())
    # geometry that does not fit is refused
    with pytest.raises(RuntimeError, match='ec_unpatchify'):
        _lib.launch('ec_unpatchify', dense.cuda(), k - 1, S - 1, 0, n, res, p, out2)
    with pytest.raises(RuntimeError, match='ec_unpatchify'):
        _lib.launch('ec_unpatchify', dense.cuda(), k, S - 1, 1, n, res, p, out2)


# ------------------------------------------------------------------------------------------------
# 2. the embedding stage's data gradient
# ------------------------------------------------------------------------------------------------
def _backward_image(tower, imgs, d_feats, grads=None):
    """``ec_vit_train_forward`` + ``ec_vit_train_backward_image`` straight over the C ABI -> (d_image, d pre [n, S, W]
    as the pass left it in its scratch, found through ``ec_vit_train_layout``)."""
    from eventclip_amd import _lib
    lib, n, dev = _lib.lib(), imgs.shape[0], torch.device('cuda', torch.cuda.current_device())
    res = tower.cfg['image_size']
    patches = T._patchify(tower, imgs)
    tape = _lib.scratch(tower.workspace_bytes(n), dev).zero_()
    feats = torch.empty(n, tower.D, device=dev)
    _lib.launch('ec_vit_train_forward', tower._vit, patches, n, feats, tape, tape.numel())
    scr = _lib.scratch(lib.ec_vit_train_backward_image_scratch_bytes(ctypes.byref(tower._vit), n), dev).zero_()
    g, keep = tower.grads_over(grads or {})                               # noqa: F841 (the struct's block array)
    d_image = torch.full((n, 3, res, res), float('nan'), device=dev)
    _lib.launch('ec_vit_train_backward_image', tower._vit, tower._vit_t, patches, n, d_feats.cuda(), g, None,
                *tower.conv_operands(), d_image, tape, tape.numel(), scr, scr.numel())
    cnt = _lib.EC_VT_BLOCK0 + _lib.EC_VT_PER_BLOCK * tower.L
    offs = (ctypes.c_int64 * cnt)()
    assert lib.ec_vit_train_layout(ctypes.byref(tower._vit), n, offs, cnt) == cnt
    # the pass's scratch follows the tape in the layout's buffer; here it is a buffer of its own, first slot g16
    o = offs[_lib.EC_VT_DH32] - offs[_lib.EC_VT_G16]
    nbytes = n * tower.S * tower.W * 4
    assert 0 <= o and o + nbytes <= scr.numel()
    d_pre = scr[o:o + nbytes].view(torch.float32).view(n, tower.S, tower.W).clone()
    return d_image, d_pre


@pytest.mark.parametrize('name', ['wide_odd', 'l14_2blocks'])
@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_embedding_stage_against_float64_of_d_pre_times_conv1(hip, name, dtype):
    cfg, n = T.CONFIGS[name]
    model, tower, sd = T._tower(cfg, seed=2, dtype=dtype)
    torch.manual_seed(13)
    imgs = torch.randn(n, 3, cfg['image_size'], cfg['image_size'])
    d_feats = torch.randn(n, cfg['embed_dim'])
    d_image, d_pre = _backward_image(tower, imgs, d_feats)
    assert bool(torch.isfinite(d_image).all()) and float(d_pre.abs().max()) > 0
    d_tok = d_pre[:, 1:].double().cpu()
    w = tower.master['conv1.weight'].double().cpu()
    want, bound = R.embed_data_grad(d_tok, w), R.embed_data_grad_bound(d_tok, w, UNIT[dtype])
    err = (d_image.double().cpu() - want).abs()
    print(f'{name} {dtype}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, '
          f'relative l2 {T.rel_l2(d_image, want):.2e}')
    assert bool((err <= bound).all())


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_embedding_stage_zero_row_cancelling_row_and_the_repack(hip, dtype):
    """``ec_patch_embed_backward`` on hand-made 16-bit token gradients: a patch row of zeros gives a patch of exact
    zeros; a row (a, -a, 0, ...) against a conv1.weight whose first two output channels were made equal cancels to
    within the bound, whose sum of magnitudes does not cancel.  Writing conv1.weight re-packs its transposed operand
    copies through ``VisualTower.refresh``."""
    from eventclip_amd import _lib
    cfg, n = T.CONFIGS['wide_odd']
    model, tower, sd = T._tower(cfg, seed=3, dtype=dtype)
    tower.refresh()
    before = tower.conv_operands()[0].clone()
    w = tower.master['conv1.weight']
    with torch.no_grad():
        w[1].copy_(w[0])
    launches = []
    real = _lib.launch
    _lib.launch = lambda name, *a: (launches.append(name), real(name, *a))[1]
    try:
        assert tower.refresh()
    finally:
        _lib.launch = real
    assert 'ec_pack_weight16_batched' in launches
    assert torch.equal(tower.packed['conv_t'], before)                   # built when the image gradient asks, not by the re-pack
    conv_t, conv_lo_t = tower.conv_operands()
    assert tower.conv_operands()[0] is conv_t and not tower._conv_t_stale
    W, k, kt, S, cd = tower.W, tower.k, tower.kt, tower.S, tower.cd
    assert kt % 16 == 0 and kt >= k
    flat = w.reshape(W, k)
    hi = flat.to(cd)
    assert torch.equal(conv_t[:k], hi.t()) and not torch.equal(conv_t, before)
    assert torch.equal(conv_lo_t[:k], (flat - hi.float()).to(cd).t())
    assert not conv_t[k:].any() and not conv_lo_t[k:].any()
    torch.manual_seed(17)
    d_tok16 = (torch.randn(n, S, W, device='cuda') * 0.05).to(cd)
    d_tok16[0, 3] = 0                                                    # image 0, patch 2: a zero row
    d_tok16[1, 1] = 0                                                    # image 1, patch 0: the cancelling row
    d_tok16[1, 1, 0], d_tok16[1, 1, 1] = 0.75, -0.75
    res, p = cfg['image_size'], cfg['patch']
    d_pix = torch.full((n * S, kt), float('nan'), device='cuda')
    d_image = torch.full((n, 3, res, res), float('nan'), device='cuda')
    _lib.launch('ec_patch_embed_backward', tower._vit, conv_t, conv_lo_t,
                d_tok16.contiguous(), n, d_pix, d_image)
    d_tok = d_tok16[:, 1:].double().cpu()
    w64 = w.double().cpu()
    want, bound = R.embed_data_grad(d_tok, w64), R.embed_data_grad_bound(d_tok, w64, UNIT[dtype])
    got = d_image.double().cpu()
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= bound).all())
    g = res // p
    zero = got[0, :, (2 // g) * p:(2 // g + 1) * p, (2 % g) * p:(2 % g + 1) * p]
    assert float(zero.abs().max()) == 0.0 and float(bound[0, :, :p, 2 * p:3 * p].max()) == 0.0
    cancel, cb = got[1, :, :p, :p], bound[1, :, :p, :p]
    assert float(want[1, :, :p, :p].abs().max()) == 0.0 and float(cb.min()) > 0
    print(f'{dtype}: cancelling row: worst |d_image| {float(cancel.abs().max()):.3e} (bound {float(cb.max()):.3e})')


# ------------------------------------------------------------------------------------------------
# 3. end to end against float64 autograd of the oracle
# ------------------------------------------------------------------------------------------------
def _weights(name, activation):
    """(cfg, n, state dict) of an end-to-end case (seed 1).  The exact-GELU towers take the weights tests/test_gelu_gpu.py
    gives its fine-tuning cases: every c_fc bias shifted and c_proj scaled, so that the two activations are far apart."""
    from eventclip_amd import clip as eclip
    cfg, n = E2E[name]
    sd = eclip.random_state_dict(cfg, seed=1)
    if activation == 'gelu':
        cfg, sd = dict(cfg, activation='gelu'), G.shifted(sd, visual_branch=G.FT_BRANCH)
    return cfg, n, sd


@functools.lru_cache(maxsize=None)
def _oracle(name, activation='quick_gelu'):
    """fp64 autograd of the oracle tower with the image a leaf, once for both operand types; activation 'gelu': through
    the oracle with x Phi(x) in place of QuickGELU (``test_gelu_gpu.swapped_oracle``).  -> (imgs, d_feats, d_image,
    features, d_image of the OTHER activation on the same weights)"""
    from oracle import clip_ref
    cfg, n, sd = _weights(name, activation)
    torch.manual_seed(5)
    imgs = torch.randn(n, 3, cfg['image_size'], cfg['image_size'])
    d_feats = torch.randn(n, cfg['embed_dim'])
    leaves = {k: v.double() for k, v in sd.items() if k.startswith('visual.')}

    def run():
        x = imgs.double().requires_grad_(True)
        feats = clip_ref.encode_image_autograd(leaves, cfg, x)
        feats.backward(d_feats.double())
        return x.grad, feats.detach()
    quick = run()
    if activation != 'gelu':
        return imgs, d_feats, quick[0], quick[1], None
    with G.swapped_oracle():
        exact = run()
    return imgs, d_feats, exact[0], exact[1], quick[0]


def _check_d_image(got, want, dtype, what):
    tol, cos = BOUNDS[dtype]
    e, c = T.rel_l2(got, want), T.cosine(got, want)
    print(f'{what} {dtype}: d_image relative l2 {e:.2e} cosine {c:.6f}')
    assert bool(torch.isfinite(got).all())
    assert e < tol and c > cos, (what, e, c)


@pytest.mark.parametrize('name,activation', [('tiny32', 'quick_gelu'), ('tiny32', 'gelu'), ('l14_2blocks', 'quick_gelu')])
@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_image_gradient_matches_the_float64_oracle(hip, name, activation, dtype):
    """``image.grad`` after ``backward`` of a random cotangent on the features of ``vit_image_fwd``: the tiny tower frozen,
    with both activations (QuickGELU, and the exact GELU against the swapped oracle: the GELU_BWD16 chain down to the
    image), and the two ViT-L/14 blocks with every parameter trainable.
    Measured (relative l2 / cosine): tiny32 QuickGELU f16 8.95e-4 / 1.000000, bf16 7.25e-3 / 0.999975; tiny32 exact GELU
    f16 1.04e-3 / 1.000000, bf16 7.36e-3 / 0.999974; l14_2blocks f16 9.15e-4 / 1.000000, bf16 7.17e-3 / 0.999974
    (DESIGN.md 6)."""
    from eventclip_amd import torch_ops
    imgs, d_feats, want, feats64, other = _oracle(name, activation)
    cfg, n, sd = _weights(name, activation)
    model, tower = G._train_tower(cfg, sd, dtype)
    assert tower._vit.activation == tower._vit_t.activation == int(activation == 'gelu')
    for p in tower.param.values():
        p.requires_grad_(name != 'tiny32')
    params = [tower.param[k] for k in tower.trainable()]
    img = imgs.cuda().requires_grad_(True)
    feats, tape = torch.ops.eventclip_hip.vit_image_fwd(img, params, torch_ops.handle_of(tower))
    assert feats.requires_grad and not tape.requires_grad
    print(f'{name} {dtype}: features vs float64, max-normalised '
          f'{float((feats.detach().cpu().double() - feats64).abs().max() / feats64.abs().max()):.2e}')
    feats.backward(d_feats.cuda())
    assert img.grad is not None and img.grad.shape == img.shape and img.grad.dtype == torch.float32
    assert all((p.grad is not None) == (name != 'tiny32') for p in tower.param.values())
    _check_d_image(img.grad, want, dtype, f'{name} {activation}')
    if other is not None:
        # which activation was differentiated: the two oracles' gradients on these weights lie `apart` from each other
        # (a property of the references alone, 7.4e-2: inside bf16's 8e-2), and the result has to sit at the exact GELU's,
        # within a quarter of that distance
        apart = T.rel_l2(other, want)
        print(f'{name} {activation} {dtype}: d_image of the QuickGELU oracle lies {apart:.2e} from that of the exact GELU, '
              f'the result {T.rel_l2(img.grad, other):.2e} from it')
        assert apart > 5e-2 and T.rel_l2(img.grad, want) < 0.25 * apart


# ------------------------------------------------------------------------------------------------
# 4. a frozen tower against every parameter trainable
# ------------------------------------------------------------------------------------------------
# every weight-, bias- and LayerNorm-gradient ends in a partial-sum reduction, conv1's starts with transposed copies
# (K-batched GEMMs are no sign of one: the dX products' last row tiles run in K-batches too, gemm_rows32)
WEIGHT_GRAD_KERNELS = ('transpose_kernel', 'colsum_kernel + reduce_kernel')


def _profiled(fn):
    from eventclip_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_begin()
    out = fn()
    torch.cuda.synchronize()
    return out, {e['name']: e['launches'] for e in _lib.profile_end() if e['launches']}


@pytest.mark.parametrize('name,spec,dtype', [('wide_odd', None, 'float16'), ('l14_2blocks', None, 'bfloat16'),
                                             ('tiny', 'qkvo-2', 'float16')])
def test_frozen_tower_gives_the_same_image_gradient_and_launches_no_weight_gradient(hip, monkeypatch, name, spec, dtype):
    from eventclip_amd import _lib, ft, torch_ops
    ops = torch.ops.eventclip_hip
    tower, params, names, cfg, n, _ = A.tower_with_params(name, dtype=dtype, spec=spec)
    torch.manual_seed(6)
    imgs = torch.randn(n, 3, cfg['image_size'], cfg['image_size'], device='cuda')
    d_feats = torch.randn(n, cfg['embed_dim'], device='cuda')
    h = torch_ops.handle_of(tower)
    plain = [p.detach() for p in params]
    # the trainable case is vit_train_fwd / vit_train_bwd on patchify(image), bit for bit
    patches = T._patchify(tower, imgs)
    feats0, tape0 = ops.vit_train_fwd(patches, plain, h)
    want = ops.vit_train_bwd(patches, plain, tape0, d_feats, h, [True] * len(plain))
    feats, tape = ops.vit_image_fwd(imgs, plain, h)
    assert torch.equal(feats, feats0)
    launches = A.count_launches(monkeypatch)
    full, prof_full = _profiled(lambda: ops.vit_image_bwd(plain, tape, d_feats, h, True, [True] * len(plain)))
    assert len(full) == 1 + len(plain) and bool(torch.isfinite(full[0]).all())
    for k, a, b in zip(names, full[1:], want):
        assert torch.equal(a, b), k
    assert [nm for nm, _ in launches if nm.startswith('ec_vit_train_backward')] == ['ec_vit_train_backward_image']
    # frozen: the same d_image, nothing else
    del launches[:]
    frozen, prof = _profiled(lambda: ops.vit_image_bwd(plain, tape, d_feats, h, True, [False] * len(plain)))
    assert torch.equal(frozen[0], full[0]) and all(t.numel() == 0 for t in frozen[1:])
    (args,) = [a for nm, a in launches if nm == 'ec_vit_train_backward_image']
    g, lora = args[5], args[6]
    assert isinstance(g, _lib.EcVitGrads) and lora is None
    assert not any(getattr(g, f) for f, _ in ft._TOP)
    assert not any(getattr(g.blocks[i], f) for i in range(tower.L) for f, _ in ft._BLOCK)
    # ... and on the device: no transposed copy, no column sum or partial-sum reduction (every weight, bias and
    # LayerNorm gradient ends in one), and ec_sgemm's class -- the head's d cls_ln, the LoRA products -- launched
    # once: the head
    print(name, 'frozen backward launches:', prof)
    assert not [k for k in WEIGHT_GRAD_KERNELS if k in prof], prof
    assert prof.get('sgemm_kernel') == 1, prof
    assert prof.get('unpatchify_kernel') == 1 and prof['ln_bwd_kernel'] == 2 * tower.L + 2
    assert (spec is not None or 'colsum_kernel + reduce_kernel' in prof_full) and prof_full['sgemm_kernel'] > 1
    assert sum(prof.values()) < sum(prof_full.values())
    # without the image the op is vit_train_bwd on the tape's patch rows
    some = [i % 2 == 0 for i in range(len(plain))]
    got = ops.vit_image_bwd(plain, tape, d_feats, h, False, some)
    ref = ops.vit_train_bwd(patches, plain, tape0, d_feats, h, some)
    assert got[0].numel() == 0 and all(torch.equal(a, b) for a, b in zip(got[1:], ref))


@pytest.mark.parametrize('spec', [None, 'qv-2'])
def test_without_the_image_the_two_backward_ops_are_one_pass(hip, monkeypatch, spec):
    """``vit_image_bwd(need_image=False, need)`` returns the bits of ``vit_train_bwd(patches, need)``: with every master
    needed (spec None); under 'qv-2' with every factor needed and with exactly one factor of a down / up pair needed --
    the kernels write both, so the op has to find the partner a buffer, and the wanted gradient is the one the full call
    gives.  With nothing needed neither op launches."""
    from eventclip_amd import torch_ops
    ops = torch.ops.eventclip_hip
    tower, params, names, cfg, n, _ = A.tower_with_params('tiny', spec=spec)
    torch.manual_seed(8)
    imgs = torch.randn(n, 3, cfg['image_size'], cfg['image_size'], device='cuda')
    d_feats = torch.randn(n, cfg['embed_dim'], device='cuda')
    h = torch_ops.handle_of(tower)
    plain = [p.detach() for p in params]
    patches = T._patchify(tower, imgs)
    _, tape0 = ops.vit_train_fwd(patches, plain, h)
    _, tape = ops.vit_image_fwd(imgs, plain, h)
    needs = [[True] * len(plain)]
    if spec is not None:
        _, _, kd, ku = tower.lora.projections()[-1]             # v of the last block: the pass stops there
        needs += [[k == kd for k in names], [k == ku for k in names]]
        assert all(sum(need) == 1 for need in needs[1:])
    launches = A.count_launches(monkeypatch)
    full = None
    for need in needs:
        got = ops.vit_image_bwd(plain, tape, d_feats, h, False, need)
        ref = ops.vit_train_bwd(patches, plain, tape0, d_feats, h, need)
        full = full or ref
        assert len(got) == 1 + len(ref) == 1 + len(plain) and got[0].numel() == 0
        for k, b, p, a, r, f in zip(names, need, plain, got[1:], ref, full):
            if b:
                assert a.shape == p.shape and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, k
                assert torch.equal(a, r) and torch.equal(a, f), k
            else:
                assert a.numel() == 0 and r.numel() == 0, k
    assert [nm for nm, _ in launches] == ['ec_vit_train_backward_over'] * (2 * len(needs))
    del launches[:]
    none = [False] * len(plain)
    assert all(t.numel() == 0 for t in ops.vit_image_bwd(plain, tape, d_feats, h, False, none))
    assert all(t.numel() == 0 for t in ops.vit_train_bwd(patches, plain, tape0, d_feats, h, none))
    assert not launches


# ------------------------------------------------------------------------------------------------
# 5. the classifier
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['full', 'lora_qkvo'])
def test_classifier_fills_img_grad_and_leaves_the_plain_path_alone(hip, tag):
    from oracle import clip_ref, ft_train as oft
    z, c = T._golden_case(tag)
    valid = c['valid'].clone()
    if bool(valid.all()):
        valid[0, -1] = False                                              # a padded view
    data = {'img': c['imgs'].cuda(), 'valid_mask': valid.cuda(), 'label': c['labels'].cuda()}
    # the parent path: img does not require grad
    clf = A.autograd_classifier(c)
    out0 = clf(data)
    loss0 = clf.calc_train_loss(data, out0)['ce_loss']
    loss0.backward()
    plain = {k: g.clone() for k, g in A.grads_of(clf).items()}
    clf.zero_grad(set_to_none=True)
    # the image path
    img = data['img'].clone().requires_grad_(True)
    out = clf(dict(data, img=img))
    loss = clf.calc_train_loss(data, out)['ce_loss']
    loss.backward()
    assert img.grad is not None and img.grad.shape == img.shape
    assert torch.equal(loss.detach(), loss0.detach())                    # the same kernels on the same patch rows
    assert sorted(out) == sorted(out0)
    for k in out:                                                        # full_logits, logits, probs, valid_masks
        assert torch.equal(out[k].detach(), out0[k].detach()), k
    grads = A.grads_of(clf)
    assert sorted(grads) == sorted(plain) and all(torch.equal(grads[k], plain[k]) for k in plain)
    assert float(img.grad[~valid.cuda()].abs().max()) == 0.0             # padded views: exact zeros
    assert float(img.grad[valid.cuda()].abs().max()) > 0
    # float64 autograd of the oracle: tower, normalised features, logits, aggregation, cross-entropy
    leaves = {k: v.double() for k, v in c['visual'].items()}
    eff = {'visual.' + k: v for k, v in oft.effective_visual(leaves).items()}
    cfg = dict(T._tiny_cfg(**c['cfg']))
    x = c['imgs'].double().requires_grad_(True)
    feats = clip_ref.encode_image_autograd(eff, cfg, x[valid])
    text = (clf.text_feats.detach() if c['prompt'] else c['text']).double().cpu()
    want_loss, _ = oft.head(feats, valid, c['labels'].long(), text, clf.logit_scale, c['agg'], c['probs_loss'], c['prompt'])
    want_loss.backward()
    assert abs(float(loss.detach()) - float(want_loss.detach())) < 2e-3 * max(1.0, abs(float(want_loss.detach())))
    _check_d_image(img.grad.cpu()[valid], x.grad[valid], 'float16', f'classifier {tag}')
    # without grad mode, or in eval mode, nothing is built
    with torch.no_grad():
        assert not clf(dict(data, img=img))['logits'].requires_grad


# ------------------------------------------------------------------------------------------------
# 6. CLIP.encode_image(differentiable=True)
# ------------------------------------------------------------------------------------------------
def test_encode_image_differentiable(hip):
    from eventclip_amd import clip as eclip
    dtype = 'float16'
    imgs, d_feats, want, _, _ = _oracle('tiny32')
    cfg, n, sd = _weights('tiny32', 'quick_gelu')
    model = eclip.CLIP(cfg, sd, dtype=dtype).cuda().eval()               # the serving chain: scaled q, folded LayerNorm
    before = model.encode_image(imgs.cuda())
    assert not before.requires_grad
    img = imgs.cuda().requires_grad_(True)
    feats = model.encode_image(img, differentiable=True)
    assert feats.requires_grad and feats.shape == before.shape
    # the training form is the plain chain: the same features up to the last bits (1e-3 is the f16 serving contract)
    diff = float((feats.detach() - before).abs().max() / before.abs().max())
    print(f'{dtype}: differentiable vs default features, max-normalised {diff:.2e}')
    assert diff < 1e-3
    feats.backward(d_feats.cuda())
    _check_d_image(img.grad, want, dtype, 'encode_image')
    assert all(p.grad is None for p in model.parameters())               # a frozen tower
    # a graph alive while the module drops its cached tower (.cuda() / .to()) keeps the tower it ran through
    img2 = imgs.cuda().requires_grad_(True)
    feats2 = model.encode_image(img2, differentiable=True)
    model.cuda()
    assert model._diff_tower is None
    feats2.backward(d_feats.cuda())
    assert torch.equal(img2.grad, img.grad)
    assert model.encode_image(img2, differentiable=True) is not None     # rebuilt
    tower = model._diff_tower
    assert tower is not None and model.encode_image(img, differentiable=True) is not None and model._diff_tower is tower
    # the default call: the same bits before and after the differentiable tower was built
    assert torch.equal(model.encode_image(imgs.cuda()), before)
    # new weights: both calls follow
    sd2 = eclip.random_state_dict(cfg, seed=2)
    model.load_state_dict(sd2)
    fresh = eclip.CLIP(cfg, sd2, dtype=dtype).cuda().eval()
    after = model.encode_image(img, differentiable=True)
    assert model._diff_tower is tower and not torch.equal(after.detach(), feats.detach())
    assert torch.equal(after.detach(), fresh.encode_image(img, differentiable=True).detach())
    assert torch.equal(model.encode_image(imgs.cuda()), fresh.encode_image(imgs.cuda()))
    with pytest.raises(ValueError, match='encode_image expects'):
        model.encode_image(img[:, :, :16], differentiable=True)


def test_encode_image_differentiable_refuses_the_split_precision_tower(hip):
    from eventclip_amd import clip as eclip
    cfg, n = E2E['tiny32']
    model = eclip.CLIP(cfg, eclip.random_state_dict(cfg, seed=1), image_precise=True).cuda().eval()
    img = torch.randn(1, 3, 32, 32, device='cuda', requires_grad=True)
    with pytest.raises(NotImplementedError, match='the split-precision image tower has no training form'):
        model.encode_image(img, differentiable=True)


# ------------------------------------------------------------------------------------------------
# 7. autograd behaviour
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec', [None, 'qv-3'])
def test_opcheck_on_the_image_ops(hip, spec):
    from eventclip_amd import torch_ops
    ops = torch.ops.eventclip_hip
    tower, params, names, cfg, n, _ = A.tower_with_params('tiny', spec=spec)
    torch.manual_seed(4)
    img = torch.randn(n, 3, cfg['image_size'], cfg['image_size'], device='cuda', requires_grad=True)
    h = torch_ops.handle_of(tower)
    torch.library.opcheck(ops.vit_image_fwd.default, (img, params, h))
    plain = [p.detach() for p in params]
    feats, tape = ops.vit_image_fwd(img.detach(), plain, h)
    need = [i % 3 != 1 for i in range(len(params))]
    torch.library.opcheck(ops.vit_image_bwd.default, (plain, tape, torch.randn_like(feats), h, True, need))
    torch.library.opcheck(ops.vit_image_bwd.default, (plain, tape, torch.randn_like(feats), h, True, [False] * len(need)))
    with pytest.raises(RuntimeError, match='expected'):
        ops.vit_image_fwd(img.detach().half(), plain, h)
    with pytest.raises(RuntimeError, match='do not belong'):
        ops.vit_image_bwd(plain, tape[:-256], torch.randn_like(feats), h, True, need)


def test_two_graphs_alive_and_a_second_backward_doubles_the_gradient(hip):
    from eventclip_amd import torch_ops
    ops = torch.ops.eventclip_hip
    tower, params, names, cfg, n, _ = A.tower_with_params('wide_odd')
    h = torch_ops.handle_of(tower)
    torch.manual_seed(8)
    res = cfg['image_size']
    a = torch.randn(n, 3, res, res, device='cuda', requires_grad=True)
    b = torch.randn(2, 3, res, res, device='cuda', requires_grad=True)
    da, db = torch.randn(n, cfg['embed_dim'], device='cuda'), torch.randn(2, cfg['embed_dim'], device='cuda')
    fa, _ = ops.vit_image_fwd(a, params, h)
    fb, _ = ops.vit_image_fwd(b, params, h)                               # a second graph, alive beside the first
    fa.backward(da, retain_graph=True)
    once, p_once = a.grad.clone(), [p.grad.clone() for p in params]
    assert b.grad is None
    fb.backward(db)
    assert b.grad is not None and torch.equal(a.grad, once)
    # alone, each graph gives the same bits
    a2 = a.detach().clone().requires_grad_(True)
    ops.vit_image_fwd(a2, [p.detach() for p in params], h)[0].backward(da)
    assert torch.equal(a2.grad, once)
    for p in params:
        p.grad = None
    fa.backward(da)                                                       # the retained graph: the tape was only read
    assert torch.equal(a.grad, 2 * once)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, p_once))
    with pytest.raises(RuntimeError):
        fa.backward(da)                                                   # freed now
