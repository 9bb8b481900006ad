"""Fine-tuning the vision tower with ``loss.backward()``: ``eventclip_hip::vit_train_fwd`` / ``::vit_train_bwd`` and
``FTCLIPClassifier(clip_dict=dict(..., autograd=True))`` on the MI355X.

The ops against ``VisualTower.forward`` / ``.backward`` (same kernels: same bits), the reference's loop (``clf(data)``,
``calc_train_loss``, ``loss.backward()``, ``torch.optim.Adam`` with the two parameter groups of method.py:174-180)
against the reference's own autograd (tests/golden/ft_train.npz) and against float64, the repack of operand copies
that went stale, several live graphs, ``torch.amp.GradScaler``, checkpoints, ``DistributedDataParallel``, opcheck.
Tolerances are those of tests/test_ft_train_gpu.py, which checks the same kernels through ``FTTrainer``."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_ft_train_gpu as T

pytestmark = pytest.mark.gpu

CASES = ['full', 'lora_qkvo', 'lora_int', 'lora_qv', 'bias', 'ln', 'conv_cls']


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def autograd_classifier(c, load_factors=True, autograd=True):
    """The classifier of a fixture case as ``test_ft_train_gpu`` builds it, with the ``autograd`` key; the LoRA factors
    of the fixture go into the injected Parameters."""
    c2 = dict(c, clip_dict=dict(c['clip_dict'], **({'autograd': True} if autograd else {})))
    clf = T._classifier_for(c2)
    if autograd and load_factors:
        with torch.no_grad():
            for n, p in clf.named_parameters():
                if '.lora_' in n:
                    p.copy_(c['sd'][n])
    return clf.train()


def two_group_adam(clf, lr, clip_lr, opt=torch.optim.Adam):
    """method.py:165-180."""
    name = 'model.visual'
    own = [p for n, p in clf.named_parameters() if name not in n and p.requires_grad]
    clip = [p for n, p in clf.named_parameters() if name in n and p.requires_grad]
    return opt([{'params': own, 'lr': lr}, {'params': clip, 'lr': clip_lr}])


def batch(c):
    return {'img': c['imgs'].cuda(), 'valid_mask': c['valid'].cuda(), 'label': c['labels'].cuda()}


def other_batch(c):
    return {'img': c['imgs'].flip(0)[:2].cuda() * 0.7, 'valid_mask': c['valid'].flip(0)[:2].cuda(),
            'label': c['labels'].flip(0)[:2].cuda()}


def grads_of(clf):
    return {n: p.grad for n, p in clf.named_parameters() if p.grad is not None}


def train_feats(clf, data):
    """(out, the tower's features of a train-mode forward: what ``_classify`` is handed)."""
    seen = []
    orig = clf._classify
    clf._classify = lambda feats, *a, **k: (seen.append(feats), orig(feats, *a, **k))[1]
    try:
        out = clf(data)
    finally:
        del clf._classify
    return out, seen[0]


def check_grads_against_golden(z, c, tag, grads):
    for name in c['trainable']:
        want = torch.from_numpy(z[f'{tag}/grad:{name}'])
        got = grads[name].reshape(want.shape)
        if name.endswith('attn.in_proj_bias'):             # zero key-bias gradient: see the tower test
            W = c['cfg']['width']
            sel = torch.cat([torch.arange(W), torch.arange(2 * W, 3 * W)])
            e = T.rel_l2(got.cpu()[sel], want[sel])
            print(f'{tag} {name}: rel l2 (q, v rows) {e:.2e}')
            assert e < T.GRAD_REL, name
            continue
        e, cs = T.rel_l2(got, want), T.cosine(got, want)
        print(f'{tag} {name}: rel l2 {e:.2e} cosine {cs:.6f}')
        assert e < T.GRAD_REL and cs > 0.9995, (name, e, cs)


def tower_with_params(name, dtype='float16', seed=0, spec=None):
    """A ``VisualTower`` of ``test_ft_train_gpu.CONFIGS`` with the tensors the ops take: every master trainable, or
    (spec) none of them and LoRA factors with non-zero ``up``.  -> (tower, params in op order, their names, cfg, n, sd)"""
    from eventclip_amd import ft
    cfg, n = T.CONFIGS[name]
    model, tower, sd = T._tower(cfg, seed=seed, dtype=dtype)
    if spec is None:
        for p in tower.param.values():
            p.requires_grad_(True)
        names = tower.trainable()
        return tower, [tower.param[k] for k in names], names, cfg, n, sd
    torch.manual_seed(11)
    lf = ft.LoraFactors(tower, spec)
    for k, p in lf.params.items():
        if 'lora_up' in k:
            p.copy_(torch.randn_like(p) * 0.02)
    lf.params = {k: p.requires_grad_(True) for k, p in lf.params.items()}
    lf.bind()
    return tower, list(lf.params.values()), list(lf.params), cfg, n, sd


def count_launches(monkeypatch):
    from eventclip_amd import _lib
    seen = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda name, *a: (seen.append((name, a)), real(name, *a))[1])
    return seen


REPACKS = ('ec_pack_weight16_batched', 'ec_lora_merge_batched')


# ------------------------------------------------------------------------------------------------
# 1. same kernels, same bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,spec', [('tiny', None), ('l14_2blocks', None), ('tiny', 'qkvo-2')])
def test_ops_are_the_tower_s_passes_bit_for_bit(hip, name, spec):
    from eventclip_amd import torch_ops
    ops = torch.ops.eventclip_hip
    tower, params, names, cfg, n, _ = tower_with_params(name, spec=spec)
    torch.manual_seed(4)
    patches = T._patchify(tower, torch.randn(n, 3, cfg['image_size'], cfg['image_size']))
    d_feats = torch.randn(n, cfg['embed_dim'], device='cuda')
    h = torch_ops.handle_of(tower)
    feats, tape = ops.vit_train_fwd(patches, [p.detach() for p in params], h)
    assert tape.dtype == torch.uint8 and tape.numel() == tower.workspace_bytes(n)
    assert tower._ws.buf is None                              # the shared scratch is not the ops'
    got = ops.vit_train_bwd(patches, [p.detach() for p in params], tape, d_feats, h, [True] * len(params))
    got = [g.clone() for g in got]
    if spec is None:
        assert torch.equal(feats, tower.forward(patches))
        want, _ = tower.backward(d_feats, names)
    else:
        want = {k: torch.full_like(p, float('nan')) for k, p in tower.lora.params.items()}
        struct, keep = tower.lora.struct_for(want)            # noqa: F841 (the struct's block array)
        assert torch.equal(feats, tower.forward(patches))
        tower.backward(d_feats, [], struct)
    for k, g in zip(names, got):
        assert g.shape == want[k].shape and torch.isfinite(g).all(), k
        assert torch.equal(g, want[k]), k
    # a parameter list that is not the tower's is refused
    with pytest.raises(RuntimeError, match='is not the tower'):
        ops.vit_train_fwd(patches, [params[0].detach()[:1]] + [p.detach() for p in params[1:]], h)
    with pytest.raises(RuntimeError, match='expected'):
        ops.vit_train_fwd(patches, [p.detach() for p in params[1:]], h)


# ------------------------------------------------------------------------------------------------
# 2. the reference's loop against the reference's autograd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', CASES)
def test_the_reference_s_loop_matches_the_reference_s_autograd(hip, tag):
    """Loss, features, every gradient and the parameters after two steps of torch.optim.Adam, against the reference's
    FTCLIPClassifier under torch autograd (fp32); the bounds of ``test_training_step_matches_the_reference``."""
    z, c = T._golden_case(tag)
    clf = autograd_classifier(c)
    assert sorted(n for n, p in clf.named_parameters() if p.requires_grad) == c['trainable']
    lr, clip_lr = float(z['lr']), float(z['clip_lr'])
    opt = two_group_adam(clf, lr, clip_lr)
    assert len(opt.param_groups[1]['params']) == sum('model.visual' in n for n in c['trainable'])
    data = batch(c)
    out, feats = train_feats(clf, data)
    loss = clf.calc_train_loss(data, out)['ce_loss']
    loss.backward()
    print(f'{tag}: loss {float(loss.detach()):.6f} (reference {float(z[f"{tag}/loss"]):.6f})')
    assert abs(float(loss.detach()) - float(z[f'{tag}/loss'])) < 2e-3 * max(1.0, abs(float(z[f'{tag}/loss'])))
    np.testing.assert_allclose(feats.detach().cpu().numpy(), z[f'{tag}/feats'], rtol=0,
                               atol=1e-3 * float(np.abs(z[f'{tag}/feats']).max()))
    grads = grads_of(clf)
    assert sorted(grads) == c['trainable']
    check_grads_against_golden(z, c, tag, grads)
    opt.step()
    opt.zero_grad()
    clf.calc_train_loss(data, clf(data))['ce_loss'].backward()
    opt.step()
    sd = clf.state_dict()
    for name in c['trainable']:
        want = z[f'{tag}/step2:{name}']
        got = sd[name].detach().cpu().numpy().reshape(want.shape)
        g0 = np.abs(z[f'{tag}/grad:{name}'])
        live = g0 > 1e-2 * g0.max()        # Adam normalises the step: elements with ~zero gradient follow rounding
        np.testing.assert_allclose(got[live], want[live], rtol=0, atol=0.35 * clip_lr + 1e-6, err_msg=name)
    want_keys = set(z[f'{tag}/sd_keys'].tolist())
    assert {k for k in sd if k.startswith('model.visual.')} == {k for k in want_keys if k.startswith('model.visual.')}


# ------------------------------------------------------------------------------------------------
# 3. float64
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_l14():
    """fp64 autograd of the oracle tower on ``l14_2blocks`` (seed 1), once for both operand types."""
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg, n = T.CONFIGS['l14_2blocks']
    sd = eclip.random_state_dict(cfg, seed=1)
    torch.manual_seed(5)
    imgs = torch.randn(n, 3, cfg['image_size'], cfg['image_size'])
    d_feats = torch.randn(n, cfg['embed_dim'])
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith('visual.')}
    clip_ref.encode_image_autograd(leaves, cfg, imgs.double()).backward(d_feats.double())
    return imgs, d_feats, {k[len('visual.'):]: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_grad_fields_match_the_float64_oracle(hip, dtype):
    """``.grad`` after ``backward`` of a random cotangent on the features of ``vit_train_fwd``; the bounds of
    ``test_tower_gradients_match_the_oracle``."""
    from eventclip_amd import torch_ops
    imgs, d_feats, ref = _oracle_l14()
    tower, params, names, cfg, n, _ = tower_with_params('l14_2blocks', dtype=dtype, seed=1)
    feats, tape = torch.ops.eventclip_hip.vit_train_fwd(T._patchify(tower, imgs), params, torch_ops.handle_of(tower))
    assert feats.requires_grad and not tape.requires_grad
    feats.backward(d_feats.cuda())
    tol, cos = (T.GRAD_REL, 0.9995) if dtype == 'float16' else (8e-2, 0.995)
    W, bad = cfg['width'], {}
    for k, p in zip(names, params):
        got, want = p.grad.reshape(ref[k].shape).cpu().double(), ref[k]
        assert torch.isfinite(got).all(), k
        if k.endswith('attn.in_proj_bias'):    # zero key-bias gradient in exact arithmetic: q, v relatively, k absolutely
            ok = T.rel_l2(torch.cat([got[:W], got[2 * W:]]), torch.cat([want[:W], want[2 * W:]])) < tol and \
                float(got[W:2 * W].abs().max()) < 1e-2 * float(want.abs().max())
        else:
            ok = T.rel_l2(got, want) < tol and T.cosine(got, want) > cos
        if not ok:
            bad[k] = (T.rel_l2(got, want), T.cosine(got, want))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# 4. operand copies that went stale
# ------------------------------------------------------------------------------------------------
def _fresh_tower_feats(clf, data):
    """Train-mode features of a ``VisualTower`` built now from the classifier's masters (and factors)."""
    from eventclip_amd import ft
    t = ft.VisualTower(clf.model)
    spec = clf.clip_dict.get('lora', -1)
    if ft.parse_lora(spec) is not None:
        ft.LoraFactors(t, spec, params={n: p for n, p in clf.model.visual.named_parameters() if '.lora_' in n}).bind()
    t.refresh()
    patches, _, _ = ft.valid_patches(t, data)
    return t.forward(patches)


def test_fingerprints_are_the_position_weighted_sums(hip):
    """``ec_fingerprint_batched`` against the same sum in numpy's uint64 arithmetic: one word, sizes around a wavefront,
    a workgroup and the 64-workgroup grid, all in one launch; one changed word (the last one included) changes it."""
    from eventclip_amd import _lib
    g = torch.Generator().manual_seed(0)
    sizes = [1, 63, 64, 65, 255, 256, 257, 64 * 256 - 1, 64 * 256 + 3, 100003]
    tensors = [torch.randn(n, generator=g).cuda() for n in sizes]

    def run(ts):
        items = (_lib.EcSpanItem * len(ts))()
        for it, t in zip(items, ts):
            it.ptr, it.n = t.data_ptr(), t.numel()
        out = torch.full((len(ts),), -1, dtype=torch.int64, device='cuda')
        _lib.launch('ec_fingerprint_batched', _lib.device_table(items), len(ts), max(t.numel() for t in ts), out)
        return out.cpu().numpy().view(np.uint64)
    got = run(tensors)
    with np.errstate(over='ignore'):
        for t, f in zip(tensors, got):
            w = t.cpu().numpy().view(np.uint32).astype(np.uint64)
            mult = np.uint64(0x9E3779B97F4A7C15) * (np.uint64(2) * np.arange(w.size, dtype=np.uint64) + np.uint64(1))
            assert f == (w * mult).sum(dtype=np.uint64), t.numel()
    assert (run(tensors) == got).all()
    for t in tensors:
        t[-1] *= 1.5
    assert (run(tensors) != got).all()
    before = run(tensors)
    tensors[-1][12345] += 1e-3
    after = run(tensors)
    assert (after[:-1] == before[:-1]).all() and after[-1] != before[-1]


@pytest.mark.parametrize('tag', ['full', 'lora_qkvo', 'lora_qv'])
def test_operand_copies_follow_the_optimiser(hip, tag, monkeypatch):
    z, c = T._golden_case(tag)
    clf = autograd_classifier(c)
    opt = two_group_adam(clf, 1e-2, 5e-3)
    data = batch(c)
    _, before = train_feats(clf, data)
    assert torch.equal(before, _fresh_tower_feats(clf, data))
    clf.calc_train_loss(data, clf(data))['ce_loss'].backward()
    opt.step()
    clf.model._pack()                                   # the inference copies: stale after the next forward's repack
    launches = count_launches(monkeypatch)
    _, after = train_feats(clf, data)
    assert any(name in REPACKS for name, _ in launches)
    assert clf.model._packed is None
    assert not torch.equal(after, before)
    assert torch.equal(after, _fresh_tower_feats(clf, data))
    # nothing changed: no repack
    del launches[:]
    _, again = train_feats(clf, data)
    assert torch.equal(again, after)
    assert launches and not [name for name, _ in launches if name in REPACKS]
    # eval mode runs on the same copies
    clf.eval()
    del launches[:]
    clf(data)
    assert not [name for name, _ in launches if name in REPACKS]


@pytest.mark.parametrize('tag', ['full', 'lora_qkvo'])
def test_operand_copies_follow_writes_outside_the_optimiser(hip, tag):
    """``p.data.mul_(1.5)`` on one frozen (under LoRA) or not-yet-stepped and one trainable master, then a write under
    ``no_grad`` and ``load_state_dict``."""
    z, c = T._golden_case(tag)
    clf = autograd_classifier(c)
    data = batch(c)
    _, before = train_feats(clf, data)
    vis = dict(clf.model.visual.named_parameters())
    frozen = [n for n, p in vis.items() if 'mlp.c_fc.weight' in n or 'merged_proj' in n][0]
    live = [n for n, p in vis.items() if p.requires_grad and p.dim() == 2][0]
    if tag == 'lora_qkvo':
        assert not vis[frozen].requires_grad
    vis[frozen].data.mul_(1.5)
    vis[live].data.mul_(1.5)
    _, after = train_feats(clf, data)
    assert not torch.equal(after, before)
    assert torch.equal(after, _fresh_tower_feats(clf, data))
    with torch.no_grad():
        vis[frozen].mul_(0.5)
        vis[live].add_(0.01)
    _, after2 = train_feats(clf, data)
    assert torch.equal(after2, _fresh_tower_feats(clf, data)) and not torch.equal(after2, after)
    clf.load_state_dict({k: v.detach().clone() * 1.01 for k, v in clf.state_dict().items()})
    _, after3 = train_feats(clf, data)
    assert torch.equal(after3, _fresh_tower_feats(clf, data)) and not torch.equal(after3, after2)


# ------------------------------------------------------------------------------------------------
# 5. live graphs, gradient ownership   6. a second backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['full', 'lora_qkvo'])
def test_two_graphs_alive_at_once(hip, tag):
    z, c = T._golden_case(tag)
    clf = autograd_classifier(c)
    a, b = batch(c), other_batch(c)
    apart = []
    for d in (a, b):
        clf.zero_grad(set_to_none=True)
        clf.calc_train_loss(d, clf(d))['ce_loss'].backward()
        apart.append({n: g.clone() for n, g in grads_of(clf).items()})
    clf.zero_grad(set_to_none=True)
    l1 = clf.calc_train_loss(a, clf(a))['ce_loss']
    l2 = clf.calc_train_loss(b, clf(b))['ce_loss']            # the second forward must leave the first one's tape alone
    (l1 + l2).backward()
    got = grads_of(clf)
    assert sorted(got) == c['trainable']
    for n in got:
        want = apart[0][n] + apart[1][n]
        if n == 'text_feats':
            # torch's own graph feeds this leaf twice per forward (x / x.norm()): four terms, summed in another order
            torch.testing.assert_close(got[n], want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
        else:
            assert torch.equal(got[n], want), n               # one gradient per tape, each from its own tape
        assert not torch.equal(apart[0][n], apart[1][n]), n


def test_gradients_belong_to_the_caller(hip):
    z, c = T._golden_case('lora_qkvo')
    clf = autograd_classifier(c)
    opt = two_group_adam(clf, 1e-2, 5e-3)
    data = batch(c)
    clf.calc_train_loss(data, clf(data))['ce_loss'].backward()
    held = grads_of(clf)
    kept = {n: g.clone() for n, g in held.items()}
    opt.step()
    opt.zero_grad(set_to_none=True)
    clf.calc_train_loss(other_batch(c), clf(other_batch(c)))['ce_loss'].backward()
    now = grads_of(clf)
    for n in held:
        assert torch.equal(held[n], kept[n]), n
        assert now[n].data_ptr() != held[n].data_ptr() and not torch.equal(now[n], held[n]), n
    ptrs = [g.untyped_storage().data_ptr() for g in now.values()]
    assert len(set(ptrs)) == len(ptrs)                        # one allocation each: no two are views of one buffer


@pytest.mark.parametrize('tag', ['full', 'lora_qkvo'])
def test_second_backward_over_a_retained_graph_doubles_the_gradients(hip, tag):
    """``ec_vit_train_backward_stages`` only reads the tape's saved activations (pre, x, xm, qkv, att, u, gact, h1, h2,
    lse); what it writes is the scratch behind them (dx, dh32, g16, ...), which it fills before it reads, and which
    ``vit_train_bwd`` gives it in a buffer of its own (``ec_vit_train_backward_over``).  So the pass leaves its tape
    intact: a second one over a retained graph gives the same bits, and ``.grad`` doubles bit for bit."""
    z, c = T._golden_case(tag)
    clf = autograd_classifier(c)
    data = batch(c)
    loss = clf.calc_train_loss(data, clf(data))['ce_loss']
    loss.backward(retain_graph=True)
    once = {n: g.clone() for n, g in grads_of(clf).items()}
    loss.backward()
    twice = grads_of(clf)
    for n in once:
        assert torch.equal(twice[n], 2 * once[n]), n
    with pytest.raises(RuntimeError):                          # the graph is gone now
        loss.backward()
    # no double backward: the backward op carries no formula
    loss = clf.calc_train_loss(data, clf(data))['ce_loss']
    p = [p for n, p in clf.named_parameters() if p.requires_grad and 'model.visual' in n][-1]
    g, = torch.autograd.grad(loss, p, create_graph=True)
    with pytest.raises(RuntimeError):
        g.square().sum().backward()


# ------------------------------------------------------------------------------------------------
# 7. frozen parts
# ------------------------------------------------------------------------------------------------
def test_only_the_trainable_parts_get_a_gradient(hip):
    z, c = T._golden_case('bias')
    clf = autograd_classifier(c)
    data = batch(c)
    clf.calc_train_loss(data, clf(data))['ce_loss'].backward()
    got = grads_of(clf)
    assert sorted(got) == c['trainable'] and all('bias' in n or n == 'text_feats' for n in got)
    assert [n for n, p in clf.named_parameters() if p.grad is None and 'bias' in n and 'model.visual' in n] == []
    clf.zero_grad(set_to_none=True)
    clf.text_feats.requires_grad_(False)
    out = clf(data)
    clf.calc_train_loss(data, out)['ce_loss'].backward()
    assert clf.text_feats.grad is None and sorted(grads_of(clf)) == [n for n in c['trainable'] if n != 'text_feats']
    for p in clf.parameters():                                # nothing left to train: no graph at all
        p.requires_grad_(False)
    assert clf(data)['logits'].grad_fn is None


def test_the_backward_asks_the_tower_only_for_what_need_names(hip, monkeypatch):
    from eventclip_amd import _lib, ft, torch_ops
    ops = torch.ops.eventclip_hip
    tower, params, names, cfg, n, _ = tower_with_params('wide_odd', seed=2)
    torch.manual_seed(6)
    patches = T._patchify(tower, torch.randn(n, 3, cfg['image_size'], cfg['image_size']))
    d_feats = torch.randn(n, cfg['embed_dim'], device='cuda')
    h = torch_ops.handle_of(tower)
    plain = [p.detach() for p in params]
    feats, tape = ops.vit_train_fwd(patches, plain, h)
    full = [g.clone() for g in ops.vit_train_bwd(patches, plain, tape, d_feats, h, [True] * len(names))]
    subsets = (['proj'], ['ln_post.weight', 'ln_post.bias'],
               ['transformer.resblocks.2.attn.in_proj_weight', 'transformer.resblocks.1.attn.out_proj.weight'],
               [k for k in names if 'bias' in k], ['class_embedding'], ['conv1.weight'],
               ['transformer.resblocks.1.mlp.c_fc.weight'])
    launches = count_launches(monkeypatch)
    fields = {leaf: f for f, leaf in ft._TOP}
    block_fields = {leaf: f for f, leaf in ft._BLOCK}
    for want in subsets:
        del launches[:]
        need = [k in want for k in names]
        got = ops.vit_train_bwd(patches, plain, tape, d_feats, h, need)
        (args,) = [a for name, a in launches if name == 'ec_vit_train_backward_over']
        g = args[5]
        assert isinstance(g, _lib.EcVitGrads)
        for k, b, t, ref in zip(names, need, got, full):
            if k in fields:
                ptr = getattr(g, fields[k])
            else:
                _, _, i, leaf = k.split('.', 3)
                ptr = getattr(g.blocks[int(i)], block_fields[leaf])
            assert bool(ptr) == b, k                          # the struct names exactly the gradients asked for
            assert (torch.equal(t, ref) and ptr == t.data_ptr()) if b else t.numel() == 0, k
    # nothing asked for: no launch
    del launches[:]
    assert all(t.numel() == 0 for t in ops.vit_train_bwd(patches, plain, tape, d_feats, h, [False] * len(names)))
    assert not launches


# ------------------------------------------------------------------------------------------------
# 8. torch.amp.GradScaler
# ------------------------------------------------------------------------------------------------
def test_grad_scaler_skips_backs_off_and_steps(hip):
    z, c = T._golden_case('bias')
    clf = autograd_classifier(c)
    opt = two_group_adam(clf, 1e-3, 1e-3)
    data = batch(c)
    trained = {n: p for n, p in clf.named_parameters() if p.requires_grad}
    before = {n: p.detach().clone() for n, p in trained.items()}
    scaler = torch.amp.GradScaler('cuda', init_scale=2.0 ** 40)
    scaler.scale(clf.calc_train_loss(data, clf(data))['ce_loss']).backward()    # 2^40 overflows the 16-bit gradients
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 39
    assert all(torch.equal(before[n], p.detach()) for n, p in trained.items())
    scaler = torch.amp.GradScaler('cuda', init_scale=256.0)
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        scaler.scale(clf.calc_train_loss(data, clf(data))['ce_loss']).backward()
        scaler.unscale_(opt)
        if step == 0:                                          # the parameters have not moved yet: the fixture's gradients
            check_grads_against_golden(z, c, 'bias', grads_of(clf))
        scaler.step(opt)
        scaler.update()
    assert scaler.get_scale() == 256.0
    moved = [n for n, p in trained.items() if not torch.equal(before[n], p.detach())]
    assert sorted(moved) == sorted(trained)


# ------------------------------------------------------------------------------------------------
# 9. eval, checkpoints, resume
# ------------------------------------------------------------------------------------------------
def test_eval_and_a_served_checkpoint_use_the_trained_weights(hip):
    z, c = T._golden_case('lora_qkvo')
    clf = autograd_classifier(c)
    opt = two_group_adam(clf, 1e-2, 5e-3)
    data = batch(c)
    clf.eval()
    before = clf(data)['logits'].clone()
    clf.train()
    for _ in range(2):
        opt.zero_grad()
        clf.calc_train_loss(data, clf(data))['ce_loss'].backward()
        opt.step()
    clf.eval()
    out = clf(data)
    after = out['logits']
    assert after.grad_fn is None and (after - before).abs().max() > 1e-3
    with torch.no_grad():
        clf.train()
        assert torch.equal(clf(data)['logits'], after)         # no_grad in train mode: the same inference path
        clf.eval()
    ckpt = {k: v.detach().cpu().clone() for k, v in clf.state_dict().items()}
    assert any('.lora_up_q' in k for k in ckpt)
    fresh = autograd_classifier(c, autograd=False)
    fresh.load_state_dict(ckpt)
    fresh.eval()
    torch.testing.assert_close(fresh(data)['logits'], after, rtol=2e-3, atol=2e-3 * float(after.abs().max()))
    # the classifier's own inference copies (clip.py) fold the injected factors the same way
    torch.testing.assert_close(clf.model.encode_image(c['imgs'].cuda()[c['valid']]),
                               fresh.model.encode_image(c['imgs'].cuda()[c['valid']]), rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize('tag', ['full', 'lora_qkvo'])
def test_resume_reproduces_the_next_step(hip, tag):
    z, c = T._golden_case(tag)
    data = batch(c)

    def step(clf, opt):
        opt.zero_grad(set_to_none=True)
        loss = clf.calc_train_loss(data, clf(data))['ce_loss']
        loss.backward()
        opt.step()
        return float(loss.detach())
    torch.manual_seed(21)
    clf = autograd_classifier(c)
    opt = two_group_adam(clf, 1e-2, 5e-3)
    for _ in range(2):
        step(clf, opt)
    ckpt = {k: v.detach().cpu().clone() for k, v in clf.state_dict().items()}
    opt_state = copy.deepcopy(opt.state_dict())
    want_loss = step(clf, opt)
    want = {n: p.detach().clone() for n, p in clf.named_parameters()}

    torch.manual_seed(99)                                   # another draw of the LoRA factors: must not matter
    clf2 = autograd_classifier(c, load_factors=False)
    opt2 = two_group_adam(clf2, 1e-2, 5e-3)                 # nerv builds the optimiser first, then loads the checkpoint
    clf2(data)                                              # ... and operand copies packed before the load must not survive it
    clf2.load_state_dict(ckpt)
    opt2.load_state_dict(opt_state)
    assert step(clf2, opt2) == want_loss
    for n, p in clf2.named_parameters():
        assert torch.equal(p.detach(), want[n]), n


# ------------------------------------------------------------------------------------------------
# 10. DistributedDataParallel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['full', 'lora_qkvo'])
def test_two_ranks_under_distributed_data_parallel(hip, tag):
    """Two gloo ranks sharing the GPU, the classifier in ``DistributedDataParallel``, half a batch each: the averaged
    gradients are the whole batch's within the gradient bound, and both ranks hold the same parameters after a step
    (each rank drew its own LoRA factors: the wrapper's broadcast starts them from rank 0's)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', '29553', 'tests/ft_autograd_ddp_worker.py', tag]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    print(d)
    assert d['world'] == 2 and d['same_names'] and d['tensors'] >= 10
    assert abs(d['loss_mean_of_ranks'] - d['loss_whole']) < 2e-3 * max(1.0, abs(d['loss_whole']))
    assert d['worst_grad_rel_l2'] < T.GRAD_REL and d['worst_grad_cosine'] > 0.9995, d
    assert d['params_equal_after_step'] and d['moved'], d


# ------------------------------------------------------------------------------------------------
# 11. opcheck   12. the default classifier
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec', [None, 'qv-3'])
def test_opcheck_on_the_tower_ops(hip, spec):
    from eventclip_amd import torch_ops
    ops = torch.ops.eventclip_hip
    tower, params, names, cfg, n, _ = tower_with_params('tiny', spec=spec)
    torch.manual_seed(4)
    patches = T._patchify(tower, torch.randn(n, 3, cfg['image_size'], cfg['image_size']))
    h = torch_ops.handle_of(tower)
    torch.library.opcheck(ops.vit_train_fwd.default, (patches, params, h))
    plain = [p.detach() for p in params]
    feats, tape = ops.vit_train_fwd(patches, plain, h)
    need = [i % 3 != 1 for i in range(len(params))]
    torch.library.opcheck(ops.vit_train_bwd.default, (patches, plain, tape, torch.randn_like(feats), h, need))


def test_a_classifier_built_without_the_key_builds_no_graph(hip):
    z, c = T._golden_case('lora_qkvo')
    clf = autograd_classifier(c, autograd=False)
    assert clf.training and torch.is_grad_enabled() and clf.text_feats.requires_grad and not clf.autograd
    out = clf(batch(c))
    assert out['logits'].grad_fn is None and not out['logits'].requires_grad and not out['probs'].requires_grad
    assert clf._tower is None and not any(p.requires_grad for p in clf.model.parameters())
    assert not any('.lora_' in n for n, _ in clf.named_parameters())
