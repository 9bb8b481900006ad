"""The autograd layer without a GPU: fake-kernel shapes of the new ops, calc_train_loss / calc_eval_loss against the
reference's two formulas (models/clip_cls.py:164-192), and the parameter order the adapter ops rely on."""
import types

import pytest
import torch
import torch.nn.functional as F


def test_fake_kernels_of_the_autograd_ops_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    from eventclip_amd.adapter import TransformerAdapter
    for name in ('classify_bwd', 'adapter_train_fwd', 'adapter_train_bwd'):
        assert name in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, name), name
    ad = TransformerAdapter(in_dim=48, d_model=32, num_heads=2, ffn_dim=64, num_layers=2, residual=0.8)
    shapes = [tuple(p.shape) for p in ad.parameters()]
    with FakeTensorMode():
        B, T, C, K = 3, 5, 48, 9
        rows = torch.empty(B * T, C, device='cuda')
        idx = torch.zeros(B, T, dtype=torch.int32, device='cuda')
        params = [torch.empty(s, device='cuda') for s in shapes]
        out, tape = torch.ops.eventclip_hip.adapter_train_fwd(rows, idx, params, 32, 2, 64, 2, 0.8, 0.1, 5)
        assert out.shape == (B, T, C) and out.dtype == torch.float32
        assert tape.dtype == torch.uint8 and tape.dim() == 1 and tape.numel() % 256 == 0 and tape.numel() > 4 * B * T * C
        mask = (1 << len(params)) | 0b101
        grads = torch.ops.eventclip_hip.adapter_train_bwd(rows, idx, params, tape, out, 32, 2, 64, 2, 0.8, 0.1, 5, mask)
        assert len(grads) == len(params) + 1
        assert tuple(grads[0].shape) == shapes[0] and tuple(grads[2].shape) == shapes[2] and grads[-1].shape == (B * T, C)
        assert all(g.shape == (0,) for i, g in enumerate(grads[:-1]) if i not in (0, 2))
        text_t = torch.empty(C, K, device='cuda')
        full = torch.empty(B, T, K, device='cuda')
        d_feats, d_text = torch.ops.eventclip_hip.classify_bwd(rows, idx, text_t, full, None, torch.empty(B, K, device='cuda'),
                                                               None, 100., 1, True, True, False)
        assert d_feats.shape == (B * T, C) and d_text.shape == (0,)
        d_feats, d_text = torch.ops.eventclip_hip.classify_bwd(rows, idx, text_t, full, full, None, None, 100., 2, False,
                                                               False, True)
        assert d_feats.shape == (0,) and d_text.shape == (C, K)


def test_fake_tape_size_is_the_library_s():
    from eventclip_amd import _lib, torch_ops
    for B, T, C, d, heads, ffn, layers in [(3, 5, 48, 32, 2, 64, 2), (1, 1, 768, 256, 4, 1024, 2), (7, 10, 768, 256, 4, 1024, 3),
                                           (2, 16, 512, 64, 8, 100, 8)]:
        assert _lib.lib().ec_adapter_train_tape_bytes(B, T, C, d, ffn, heads, layers) == \
            torch_ops._tape_numel(B, T, C, d, heads, ffn, layers)
    assert _lib.lib().ec_adapter_train_tape_bytes(2, 3, 48, 32, 64, 2, 9) == 0          # layers <= 8
    assert _lib.lib().ec_classify_backward_workspace_bytes(2, 3, 48, 5) == 2 * 1280 + 256


def test_adapter_ops_take_the_parameters_in_named_parameters_order():
    from eventclip_amd import torch_ops
    from eventclip_amd.adapter import TransformerAdapter
    for layers in (1, 3):
        ad = TransformerAdapter(in_dim=16, d_model=8, num_heads=2, ffn_dim=12, num_layers=layers)
        assert [n for n, _ in ad.named_parameters()] == torch_ops.adapter_param_names(layers)


@pytest.mark.parametrize('use_probs', [False, True])
def test_calc_train_and_eval_loss_are_the_reference_formulas(use_probs):
    from eventclip_amd.clip_cls import FSCLIPClassifier, ZSCLIPClassifier
    assert FSCLIPClassifier.calc_train_loss is ZSCLIPClassifier.calc_train_loss
    me = types.SimpleNamespace(use_logits_loss=not use_probs, use_probs_loss=use_probs)
    me.calc_train_loss = types.MethodType(ZSCLIPClassifier.calc_train_loss, me)
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(6, 7, generator=g) * 3).requires_grad_(True)
    probs = torch.softmax(torch.randn(6, 7, generator=g), -1).requires_grad_(True)
    labels = torch.randint(0, 7, (6,), generator=g)
    data, out = {'label': labels}, {'logits': logits, 'probs': probs}
    got = ZSCLIPClassifier.calc_train_loss(me, data, out)
    assert set(got) == {'ce_loss'}
    want = F.nll_loss((probs + 1e-6).log(), labels) if use_probs else F.cross_entropy(logits, labels)
    assert torch.equal(got['ce_loss'], want) and got['ce_loss'].requires_grad
    by_hand = -(torch.log(probs[torch.arange(6), labels] + 1e-6)).mean() if use_probs else \
        (torch.logsumexp(logits, -1) - logits[torch.arange(6), labels]).mean()
    torch.testing.assert_close(got['ce_loss'], by_hand)
    ev = ZSCLIPClassifier.calc_eval_loss(me, data, out)
    assert set(ev) == {'ce_loss', 'probs_acc', 'logits_acc'} and not ev['ce_loss'].requires_grad
    assert torch.equal(ev['ce_loss'], want.detach())
    assert float(ev['probs_acc']) == float((probs.argmax(-1) == labels).float().mean())
    assert float(ev['logits_acc']) == float((logits.argmax(-1) == labels).float().mean())
