"""The vision tower's input gradient without a GPU: the float64 reference of the stretch below ``ln_pre``
(tests/input_grad_ref.py) is the adjoint it claims to be and equals torch's autograd of ``F.conv2d(stride=patch)``; the
header, the exports and the bindings name the new entry points; the fake kernels of ``eventclip_hip::vit_image_fwd`` /
``vit_image_bwd`` give the shapes."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import input_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('ec_vit_train_backward_image', 'ec_vit_train_backward_image_scratch_bytes', 'ec_patch_embed_backward',
                'ec_unpatchify')


@pytest.mark.parametrize('p', [14, 16, 32])
@pytest.mark.parametrize('g', [1, 2, 3])
def test_unpatchify_is_the_exact_adjoint_of_patchify(p, g):
    """<patchify(x), y> == <x, unpatchify(y)>: on integer-valued float64 inputs both sides are exact sums, so the
    identity holds to the last bit; and unpatchify inverts patchify (a permutation)."""
    gen = torch.Generator().manual_seed(100 * p + g)
    n, res = 2, p * g
    x = torch.randint(-8, 9, (n, 3, res, res), generator=gen).double()
    y = torch.randint(-8, 9, (n, g * g, 3 * p * p), generator=gen).double()
    rows = R.patchify(x, p)
    assert rows.shape == y.shape
    assert float((rows * y).sum()) == float((x * R.unpatchify(y, p, res)).sum())
    assert torch.equal(R.unpatchify(rows, p, res), x)
    assert torch.equal(R.patchify(R.unpatchify(y, p, res), p), y)
    # the layout: row gy g + gx, column (c p + i) p + j
    for (c, yy, xx) in ((0, 0, 0), (1, res - 1, 0), (2, p // 2, res - 1)):
        assert rows[1, (yy // p) * g + xx // p, (c * p + yy % p) * p + xx % p] == x[1, c, yy, xx]


@pytest.mark.parametrize('p,g,W', [(14, 2, 8), (16, 3, 5), (32, 1, 16), (4, 2, 64)])
def test_stage_reference_is_autograd_of_the_strided_convolution(p, g, W):
    gen = torch.Generator().manual_seed(p + g)
    n, res = 3, p * g
    x = torch.randn(n, 3, res, res, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(W, 3, p, p, generator=gen, dtype=torch.float64)
    tok = F.conv2d(x, w, stride=p).reshape(n, W, g * g).permute(0, 2, 1)          # encode_image_autograd's patch rows
    # the forward is the matrix product over patchify's rows ...
    torch.testing.assert_close(tok, R.patchify(x.detach(), p) @ w.reshape(W, -1).T, rtol=1e-12, atol=1e-12)
    d_tok = torch.randn(n, g * g, W, generator=gen, dtype=torch.float64)
    tok.backward(d_tok)
    # ... and the reference is its adjoint
    torch.testing.assert_close(R.embed_data_grad(d_tok, w), x.grad, rtol=1e-12, atol=1e-12)
    # the bound is the same product over magnitudes
    b = R.embed_data_grad_bound(d_tok, w, 2.0 ** -11)
    assert b.shape == x.shape and bool((b > 0).all())
    assert bool((R.embed_data_grad(d_tok, w).abs() <= b / (2.0 ** -11 + (W + 2) * 2.0 ** -24) * (1 + 1e-12)).all())


def test_header_exports_and_bindings_name_the_entry_points():
    from eventclip_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'eventclip_hip.h')).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert f'{name}(' in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert f'#define EC_ABI_VERSION {_lib.ABI_VERSION}' in header and _lib.ABI_VERSION >= 608
    assert _lib.lib().ec_version() == _lib.ABI_VERSION
    # the existing forms keep their argument lists
    assert len(_lib.SIGNATURES['ec_vit_train_backward_over'][1]) == 12
    assert len(_lib.SIGNATURES['ec_vit_train_backward_image'][1]) == 15


def test_scratch_query_needs_no_device_and_covers_the_over_form():
    """The image form's scratch is the ``_over`` form's plus the fp32 [n S, ceil16(3 p^2)] product."""
    from eventclip_amd import _lib
    v = _lib.EcVitWeights()
    v.image_size, v.patch, v.width, v.layers, v.heads, v.out_dim = 28, 14, 64, 2, 1, 16
    v.kpad = (2 * 3 * 14 * 14 + 63) // 64 * 64
    lib = _lib.lib()
    for n in (1, 3):
        over = lib.ec_vit_train_backward_scratch_bytes(ctypes.byref(v), n)
        image = lib.ec_vit_train_backward_image_scratch_bytes(ctypes.byref(v), n)
        pix = n * 5 * ((3 * 14 * 14 + 15) // 16 * 16) * 4
        assert over > 0 and image == over + (pix + 255) // 256 * 256
    assert lib.ec_vit_train_backward_image_scratch_bytes(ctypes.byref(v), 0) == 0


def test_fake_kernels_of_the_image_ops_give_the_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    for name in ('vit_image_fwd', 'vit_image_bwd'):
        assert name in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, name), name

    class Tower:                         # what the fake kernels ask a tower
        D, G, kpad = 16, 4, 128
        cfg = dict(image_size=8)
        workspace_bytes = staticmethod(lambda n: 4096 * n + 500)
    tower = Tower()
    h = torch_ops.handle_of(tower)
    shapes = [(64, 3, 4, 4), (64,), (192, 64)]
    with FakeTensorMode():
        image = torch.empty(5, 3, 8, 8, device='cuda')
        params = [torch.empty(s, device='cuda') for s in shapes]
        feats, tape = torch.ops.eventclip_hip.vit_image_fwd(image, params, h)
        assert feats.shape == (5, 16) and feats.dtype == torch.float32
        # the workspace rounded to 256 bytes, then the 16-bit patch rows
        assert tape.dtype == torch.uint8 and tape.shape == ((4096 * 5 + 500 + 255) // 256 * 256 + 5 * 4 * 128 * 2,)
        d_feats = torch.empty(5, 16, device='cuda')
        for need_image, need in ((True, [False, False, False]), (True, [True, False, True]), (False, [False, True, False])):
            got = torch.ops.eventclip_hip.vit_image_bwd(params, tape, d_feats, h, need_image, need)
            assert len(got) == 1 + len(params) and all(g.dtype == torch.float32 for g in got)
            assert tuple(got[0].shape) == ((5, 3, 8, 8) if need_image else (0,))
            assert [tuple(g.shape) for g in got[1:]] == [s if b else (0,) for s, b in zip(shapes, need)]
    # the image and the trainable tensors are real inputs, and neither op writes an input
    schema = str(torch.ops.eventclip_hip.vit_image_fwd.default._schema)
    assert 'Tensor image' in schema and 'Tensor[] params' in schema
    assert '!' not in schema and '!' not in str(torch.ops.eventclip_hip.vit_image_bwd.default._schema)
    # the 16-bit patch tensor of the older op stays non-differentiable, and says so
    assert 'not differentiable' in torch_ops.vit_train_fwd._init_fn.__doc__


def test_encode_image_keeps_its_default():
    import inspect
    from eventclip_amd import clip as eclip
    sig = inspect.signature(eclip.CLIP.encode_image)
    assert list(sig.parameters) == ['self', 'image', 'differentiable'] and sig.parameters['differentiable'].default is False
