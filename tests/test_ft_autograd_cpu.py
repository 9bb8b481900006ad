"""``FTCLIPClassifier(clip_dict=dict(..., autograd=True))`` without a GPU: fake-kernel shapes of the two tower ops, which
parameters require grad and what ``named_parameters()`` / ``state_dict()`` call them for the seven cases of
tests/golden/ft_train.npz (the reference's own FTCLIPClassifier), and the exclusion against ``FTTrainer``."""
import types

import pytest
import torch

import test_oracle_ft_train as golden

Z = golden.golden()


def _classifier(c, autograd=True, seed=0):
    """The classifier of a fixture case on the CPU (the identity adapter without 'text-': no text encode at
    construction, which would need the device)."""
    from eventclip_amd import clip as eclip
    from eventclip_amd.clip_cls_ft import FTCLIPClassifier
    cfg = dict(image_size=8, patch=4, width=64, layers=2, embed_dim=16, text_width=64, text_heads=1, text_layers=1,
               context_length=77, vocab_size=128)
    cfg.update({k: v for k, v in c['cfg'].items() if k != 'heads'})
    model = eclip.CLIP(cfg, eclip.random_state_dict(cfg, seed=seed), full_last_block=True)
    cd = dict(clip_model=model, prompt='a point cloud image of a {}', class_names=['a', 'b'], agg_func=c['agg'],
              class_tokens=eclip.synthetic_tokens(2), **c['clip_dict'])
    if autograd:
        cd['autograd'] = True
    return FTCLIPClassifier(adapter_dict=dict(adapter_type='identity', residual=True), clip_dict=cd,
                            loss_dict=dict(use_logits_loss=True, use_probs_loss=False))


def test_fake_kernels_of_the_tower_ops_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    for name in ('vit_train_fwd', 'vit_train_bwd'):
        assert name in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, name), name

    class Tower:                         # what the fake kernels ask a tower
        D = 16
        workspace_bytes = staticmethod(lambda n: 4096 * n + 512)
    tower = Tower()
    h = torch_ops.handle_of(tower)
    shapes = [(64, 3, 4, 4), (64,), (192, 64), (4, 64), (64, 4)]
    with FakeTensorMode():
        patches = torch.empty(5, 4, 128, dtype=torch.float16, device='cuda')
        params = [torch.empty(s, device='cuda') for s in shapes]
        feats, tape = torch.ops.eventclip_hip.vit_train_fwd(patches, params, h)
        assert feats.shape == (5, 16) and feats.dtype == torch.float32
        assert tape.dtype == torch.uint8 and tape.shape == (4096 * 5 + 512,)
        need = [True, False, True, False, True]
        grads = torch.ops.eventclip_hip.vit_train_bwd(patches, params, tape, torch.empty(5, 16, device='cuda'), h, need)
        assert len(grads) == len(params) and all(g.dtype == torch.float32 for g in grads)
        assert [tuple(g.shape) for g in grads] == [s if b else (0,) for s, b in zip(shapes, need)]
    # the trainable tensors are real inputs, and neither op writes an input: the backward only reads the tape
    assert 'Tensor[] params' in str(torch.ops.eventclip_hip.vit_train_fwd.default._schema)
    assert '!' not in str(torch.ops.eventclip_hip.vit_train_bwd.default._schema)


@pytest.mark.parametrize('tag', golden.CASES)
def test_trainable_names_are_the_reference_s(tag):
    c = golden.case(Z, tag)
    clf = _classifier(c)
    got = sorted(n for n, p in clf.named_parameters() if p.requires_grad)
    assert got == [n for n in c['trainable'] if n != 'text_feats']      # (text_feats: the 'text-' adapter, below)
    # the filter of method.py:165-172 splits them as it does there: everything that trains here is the tower's
    assert all('model.visual' in n for n in got)
    # ... and the same through a wrapper's prefix, as DistributedDataParallel's named_parameters() spells them
    wrapped = torch.nn.ModuleDict({'module': clf})
    assert sorted(n for n, p in wrapped.named_parameters() if p.requires_grad) == ['module.' + n for n in got]


@pytest.mark.parametrize('tag', golden.CASES)
def test_trainable_rule_with_learned_text_features(tag):
    """The name logic on its own (prompt tuning needs the text tower, i.e. the device, at construction)."""
    from eventclip_amd import ft
    c = golden.case(Z, tag)
    plain = [n for n in map(ft.plain_visual_name, c['visual']) if n is not None]
    names = {'model.visual.' + n for n in ft.trainable_visual(plain, c['clip_dict'])}
    if ft.parse_lora(c['clip_dict']['lora']) is not None:
        shapes = ft.lora_factor_shapes(c['clip_dict']['lora'], c['cfg']['layers'], c['cfg']['width'])
        assert {k: tuple(v.shape) for k, v in c['visual'].items() if '.lora_' in k} == shapes
        names |= {'model.visual.' + k for k in shapes}
    if c['prompt']:
        names.add('text_feats')
    assert sorted(names) == c['trainable']


@pytest.mark.parametrize('tag', golden.CASES)
def test_state_dict_keys_are_the_reference_s(tag):
    c = golden.case(Z, tag)
    clf = _classifier(c)
    sd = clf.state_dict()
    want = {k for k in Z[f'{tag}/sd_keys'].tolist() if k.startswith('model.visual.')}
    assert {k for k in sd if k.startswith('model.visual.')} == want
    assert not any(k.startswith('model.') and not k.startswith('model.visual.') for k in sd)     # the frozen rest of CLIP
    for k in want:
        assert tuple(sd[k].shape) == tuple(c['sd'][k].shape), k
    # the factors start as lora.py:8-11 has them
    ups = [v for k, v in sd.items() if '.lora_up' in k]
    assert all(float(v.abs().max()) == 0.0 for v in ups)
    # load_state_dict goes into the same tensors in place, and their version counters say so
    before = {k: (v.data_ptr(), v._version) for k, v in sd.items()}
    clf.load_state_dict({k: c['sd'][k] for k in sd})
    after = clf.state_dict()
    for k in want:
        assert after[k].data_ptr() == before[k][0] and after[k]._version > before[k][1], k
        assert torch.equal(after[k], c['sd'][k].float()), k
    with pytest.raises(KeyError):
        clf.load_state_dict({k: v for k, v in sd.items() if not k.endswith('ln_pre.weight')})


def test_the_default_classifier_is_untouched():
    c = golden.case(Z, 'lora_qkvo')
    clf = _classifier(c, autograd=False)
    assert not clf.autograd and not clf._differentiable
    assert not any(p.requires_grad for p in clf.model.parameters())
    assert not any('.lora_' in k or 'merged_proj' in k for k in clf.state_dict())


def test_build_model_passes_the_key_through():
    from eventclip_amd.clip_cls import build_model
    c = golden.case(Z, 'bias')
    proto = _classifier(c, autograd=False)
    cd = dict(proto.clip_dict, autograd=True)
    params = types.SimpleNamespace(model='FTCLIP', adapter_dict=dict(adapter_type='identity', residual=True), clip_dict=cd,
                                   loss_dict=dict(use_logits_loss=True, use_probs_loss=False))
    clf = build_model(params)
    assert clf.autograd and clf.clip_dict is cd
    assert all('bias' in n for n, p in clf.named_parameters() if p.requires_grad)


def test_a_trainer_and_autograd_exclude_each_other():
    from eventclip_amd import ft
    c = golden.case(Z, 'lora_qv')
    with pytest.raises(ValueError, match='second owner'):
        ft.FTTrainer(_classifier(c), lr=1e-3)
    clf = _classifier(c, autograd=False)
    clf._trainer = object()                       # what FTTrainer.__init__ leaves on the classifier
    with pytest.raises(ValueError, match='second owner'):
        clf.enable_autograd()
    assert not clf.autograd and not any(p.requires_grad for p in clf.model.parameters())
    # a CLIP model is injected once
    with pytest.raises(ValueError, match='already carries'):
        type(clf)(adapter_dict=dict(adapter_type='identity', residual=True), clip_dict=_classifier(c).clip_dict)
