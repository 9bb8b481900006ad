"""ResNet CLIP towers on the MI355X: the kernels of csrc/resnet.hip against torch in fp32, tower parity against the
fp32 restatement (tests/resnet_ref.py) on calibrated random weights, batch invariance, and the classifiers."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {'f16': (torch.float16, 0, 2e-3), 'bf16': (torch.bfloat16, 1, 1e-2)}


def _rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30))


def _conv(hip, x, n, H, W, cin, cout, ks, w, b, resid, relu, out32, code, scale=None):
    from eventclip_amd import _lib
    out = torch.empty((n, H, W, cout), dtype=torch.float32 if out32 else x.dtype, device='cuda')
    rc = hip.ec_resnet_conv(_lib.ptr(x), n, H, W, cin, cout, ks, _lib.ptr(w), _lib.ptr(scale), _lib.ptr(b), _lib.ptr(resid),
                            int(relu), _lib.ptr(out), int(out32), code, _lib.stream_ptr())
    _lib.check(rc, 'ec_resnet_conv')
    return out


# (Cin, Cout, H, n): the 3x3 classes of the five towers -- stage 1..4 at 224 / 288 / 384 / 448 (H 56 / 72 / 96 / 112
# down to 7 / 9 / 12 / 14), each stage's first conv2 at twice the stage resolution, the stems' padded 64 / 128 channels
# at H 112 / 144 / 192 / 224 -- with batch counts whose pixels leave a partial tile
@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('cin,cout,H,n', [(64, 64, 112, 1), (64, 128, 144, 1), (64, 64, 56, 3), (128, 128, 72, 2),
                                          (128, 128, 96, 1), (128, 128, 112, 1), (128, 128, 28, 5), (192, 192, 36, 3),
                                          (256, 256, 14, 3), (320, 320, 24, 2), (512, 512, 7, 5), (640, 640, 9, 3),
                                          (768, 768, 12, 2), (1024, 1024, 14, 1), (512, 512, 28, 1),
                                          (64, 64, 192, 1), (64, 128, 192, 1), (64, 64, 224, 1), (64, 128, 224, 1),
                                          (128, 128, 56, 2), (256, 256, 28, 2), (384, 384, 24, 1)])
def test_conv3x3_matches_conv2d(hip, dt, cin, cout, H, n):
    td, code, tol = DT[dt]
    g = torch.Generator().manual_seed(cin + H + n)
    x = torch.randn(n, H, H, cin, generator=g).to(td)
    w = (torch.randn(cout, 3, 3, cin, generator=g) * (9 * cin) ** -0.5).to(td)
    b = torch.randn(cout, generator=g) * 0.1
    sc = 1 + torch.randn(cout, generator=g) * 0.2                      # the BatchNorm scale of the epilogue
    out = _conv(hip, x.cuda(), n, H, H, cin, cout, 3, w.cuda(), b.cuda(), None, True, False, code, scale=sc.cuda())
    want = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=1) * sc[:, None, None]
                  + b[:, None, None])
    assert _rel(out.cpu().permute(0, 3, 1, 2), want) < tol


@pytest.mark.parametrize('dt', list(DT))
def test_conv_epilogues(hip, dt):
    """1x1: bias + ReLU -> 16 bit; bias + 16-bit residual + ReLU -> 16 bit; fp32 store.  3x3 with the residual."""
    td, code, tol = DT[dt]
    g = torch.Generator().manual_seed(5)
    n, H, cin, cout = 3, 13, 256, 192
    x = torch.randn(n, H, H, cin, generator=g).to(td)
    r = torch.randn(n, H, H, cout, generator=g).to(td)
    b = torch.randn(cout, generator=g) * 0.1
    for ks in (1, 3):
        w = (torch.randn(cout, ks, ks, cin, generator=g) * (ks * ks * cin) ** -0.5).to(td)
        lin = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b,
                       padding=ks // 2).permute(0, 2, 3, 1)
        xc, wc, bc, rc = x.cuda(), w.cuda(), b.cuda(), r.cuda()
        o = _conv(hip, xc, n, H, H, cin, cout, ks, wc, bc, None, True, False, code).cpu()
        assert o.dtype == td and _rel(o, F.relu(lin)) < tol
        o = _conv(hip, xc, n, H, H, cin, cout, ks, wc, bc, rc, True, False, code).cpu()
        assert _rel(o, F.relu(lin + r.float())) < tol
        o = _conv(hip, xc, n, H, H, cin, cout, ks, wc, bc, None, False, True, code).cpu()
        assert o.dtype == torch.float32 and _rel(o, lin) < 1e-5
        assert (o < 0).any()


@pytest.mark.parametrize('dt', list(DT))
def test_stem_rows_both_modes(hip, dt):
    from eventclip_amd import _lib
    td, code, _ = DT[dt]
    n, R = 2, 36
    g = torch.Generator().manual_seed(2)
    u8 = torch.randint(0, 256, (n, R, R, 3), generator=g, dtype=torch.uint8)
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073])
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711])
    img = ((u8.float() / 255 - mean) / std).permute(0, 3, 1, 2).contiguous()
    want = F.unfold(img, 3, padding=1, stride=2)                       # [n, 3*9 (c, ky, kx), L]
    want = want.reshape(n, 3, 9, -1).permute(0, 3, 2, 1).reshape(n, R // 2, R // 2, 27)
    for mode, inp in ((_lib.EC_PRE_CHW_F32, img), (_lib.EC_PRE_HWC_U8, u8)):
        rows = torch.full((n, R // 2, R // 2, 64), 7.0, dtype=td, device='cuda')
        inp = inp.cuda()
        rc = hip.ec_resnet_stem_rows(_lib.ptr(inp), mode, n, R, _lib.ptr(rows), code, _lib.stream_ptr())
        _lib.check(rc)
        rows = rows.cpu()
        assert torch.equal(rows[..., 54:], torch.zeros_like(rows[..., 54:]))
        assert torch.equal(rows[..., :27], want.to(td)), mode
        assert torch.equal(rows[..., 27:54], (want - want.to(td).float()).to(td)), mode


@pytest.mark.parametrize('dt', list(DT))
def test_avgpool_exact(hip, dt):
    from eventclip_amd import _lib
    td, code, _ = DT[dt]
    x = torch.randn(3, 14, 18, 136, generator=torch.Generator().manual_seed(4)).to(td)
    y = torch.empty(3, 7, 9, 136, dtype=td, device='cuda')
    xd = x.cuda()
    _lib.check(hip.ec_resnet_avgpool(_lib.ptr(xd), 3, 14, 18, 136, _lib.ptr(y), code, _lib.stream_ptr()))
    want = F.avg_pool2d(x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).to(td)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('hw', [7, 14])
def test_attention_pool_kernels(hip, dt, hw):
    from eventclip_amd import _lib
    td, code, tol = DT[dt]
    n, C = 3, 512
    L = hw * hw + 1
    g = torch.Generator().manual_seed(hw)
    x = torch.randn(n, hw * hw, C, generator=g).abs().to(td)
    pos = torch.randn(L, C, generator=g) * 0.1
    tok = torch.empty(n, L, C, dtype=td, device='cuda')
    q_in = torch.empty(n, C, dtype=td, device='cuda')
    xd, posd = x.cuda(), pos.cuda()
    _lib.check(hip.ec_resnet_attnpool_tokens(_lib.ptr(xd), n, hw * hw, C, _lib.ptr(posd), _lib.ptr(tok),
                                             _lib.ptr(q_in), code, _lib.stream_ptr()))
    want = torch.cat([x.float().mean(1, keepdim=True), x.float()], 1) + pos
    assert torch.equal(tok.cpu(), want.to(td)) and torch.equal(q_in.cpu(), want[:, 0].to(td))
    q = (torch.randn(n, C, generator=g) * 2).to(td)
    kv = (torch.randn(n, L, 2 * C, generator=g) * 2).to(td)
    out = torch.empty(n, C, dtype=td, device='cuda')
    qd, kvd = q.cuda(), kv.cuda()
    _lib.check(hip.ec_resnet_attnpool_attend(_lib.ptr(qd), _lib.ptr(kvd), n, L, C, _lib.ptr(out), code,
                                             _lib.stream_ptr()))
    qh = q.float().reshape(n, C // 64, 1, 64)
    kh = kv[..., :C].float().reshape(n, L, C // 64, 64).transpose(1, 2)
    vh = kv[..., C:].float().reshape(n, L, C // 64, 64).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qh, kh, vh).reshape(n, C)
    assert _rel(out.cpu(), ref) < tol


# ---- towers ----
_SEEDS = (0, 1)
_TOWERS = [('RN50', None), ('RN101', None), ('RN50x4', (1, 1, 1, 1)), ('RN50x16', (1, 1, 1, 1)),
           ('RN50x64', (1, 1, 1, 1))]


def _model(arch, layers, seed, dtype='float16'):
    from eventclip_amd import clip as eclip
    from eventclip_amd import resnet
    cfg = eclip.resnet_config(arch, **({'vision_layers': layers} if layers else {}))
    sd = eclip.random_state_dict(cfg, seed=seed)
    return cfg, sd, resnet.ResNetCLIP(cfg, sd, dtype=dtype).cuda().eval()


def _maxnorm_err(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('arch,layers', _TOWERS)
def test_tower_parity_against_restatement(arch, layers):
    """Max-normalised error of the HIP features against the fp32 restatement against that of an fp16 emulation of the
    reference's own arithmetic (tests/resnet_ref.py, emulate16), for two weight seeds and 16 images."""
    from eventclip_amd import clip as eclip
    for seed in _SEEDS:
        cfg, sd, m = _model(arch, layers, seed)
        R = cfg['image_size']
        x = torch.randn(16, 3, R, R, generator=torch.Generator().manual_seed(100 + seed))
        ref_m = resnet_ref.from_state_dict(sd, cfg)
        with torch.no_grad():
            ref = ref_m(x)
            emu = ref_m(x, emulate16=True)
        got = m.encode_image(x.cuda()).cpu()
        e_hip, e_emu = _maxnorm_err(got, ref), _maxnorm_err(emu, ref)
        print(f'{arch} layers={layers} seed={seed}: hip {e_hip:.2e}  fp16 emulation {e_emu:.2e}')
        # Full depth: at most the emulation's error (measured 7 - 11 % below it).  Reduced depth: the error of both is
        # dominated by the one rounding of the weights, the same in both; measured 0.96 - 1.04 x the emulation's.
        slack = 1.0 if layers is None else 1.05
        assert e_hip <= slack * e_emu, (arch, seed, e_hip, e_emu)
        # zero-shot top-1 agrees on every image whose reference margin (top-1 minus top-2 cosine) is beyond the
        # logit error of the fp16 emulation (random towers leave some images with near-tied classes)
        text = F.normalize(m.encode_text(eclip.synthetic_tokens(10, seed=seed).cuda()).cpu(), dim=-1)
        lg, lr, le = (F.normalize(f, dim=-1) @ text.t() for f in (got, ref, emu))
        top2 = lr.topk(2, dim=1).values
        decided = (top2[:, 0] - top2[:, 1]) > 2 * float((le - lr).abs().max())
        assert int(decided.sum()) >= 2, (arch, seed, int(decided.sum()))
        assert torch.equal(lg.argmax(1)[decided], lr.argmax(1)[decided])


def test_batch_invariance():
    """A frame's features are bit-identical alone and inside a batch of 257 (chunked by the model)."""
    cfg, sd, m = _model('RN50', None, 2)
    x = torch.randn(257, 3, 224, 224, generator=torch.Generator().manual_seed(9)).cuda()
    full = m.encode_image(x)
    for i in (0, 100, 256):
        assert torch.equal(m.encode_image(x[i:i + 1]), full[i:i + 1]), i


def test_chunked_encode_rn50x64():
    """ec_resnet_encode runs RN50x64 at 448 px in chunks: 5 frames through chunks of 2 give the features of one pass,
    bit for bit, and the same as the frames one at a time."""
    cfg, sd, m = _model('RN50x64', (1, 1, 1, 1), 0)
    x = torch.randn(5, 3, 448, 448, generator=torch.Generator().manual_seed(3)).cuda()
    whole = m.encode_image(x)
    m.chunk = 2
    assert torch.equal(m.encode_image(x), whole)
    assert torch.equal(m.encode_image(x[4:5]), whole[4:5])


def test_bf16_tower():
    """bf16 operands at reduced depth (full-depth random towers amplify 16-bit rounding to 8 - 30 % even in fp16), and
    no further from the fp32 restatement than a bf16 emulation of the reference's arithmetic (the slack rule of
    test_tower_parity_against_restatement)."""
    cfg, sd, m = _model('RN50', (1, 1, 1, 1), 0, dtype='bfloat16')
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    ref_m = resnet_ref.from_state_dict(sd, cfg)
    with torch.no_grad():
        ref = ref_m(x)
        emu = ref_m(x, emulate16=torch.bfloat16)
    e_hip = _maxnorm_err(m.encode_image(x.cuda()).cpu(), ref)
    assert e_hip < 5e-2
    e_emu = _maxnorm_err(emu, ref)
    print(f'RN50 layers=(1, 1, 1, 1) bf16: hip {e_hip:.2e}  bf16 emulation {e_emu:.2e}')
    assert e_hip <= 1.05 * e_emu, (e_hip, e_emu)


@pytest.mark.parametrize('arch,layers', [('RN50x4', (1, 1, 1, 1))])
def test_bf16_tower_against_emulation(arch, layers):
    """The bf16 tower's max-normalised error against the fp32 restatement is at most that of a bf16 emulation of the
    reference's own arithmetic (resnet_ref, emulate16=torch.bfloat16), for two weight seeds and 16 images; the slack
    rule of test_tower_parity_against_restatement.

    Reduced depth only.  At full RN50 depth the bf16 comparison does not decide anything: there the max-normalised
    error moves by about 10 % when only the fp32 summation order changes (the HIP arithmetic emulated on the CPU
    with two conv algorithms: 1.9e-2 and 2.1e-2), while the bf16 emulation's own error (2.2e-2) sits within that
    spread of the tower's (2.3e-2, seed 0).  RN50x4 measures 1.01 and 0.99 x the emulation's error (seeds 0, 1)."""
    for seed in _SEEDS:
        cfg, sd, m = _model(arch, layers, seed, dtype='bfloat16')
        R = cfg['image_size']
        x = torch.randn(16, 3, R, R, generator=torch.Generator().manual_seed(200 + seed))
        ref_m = resnet_ref.from_state_dict(sd, cfg)
        with torch.no_grad():
            ref = ref_m(x)
            emu = ref_m(x, emulate16=torch.bfloat16)
        e_hip, e_emu = _maxnorm_err(m.encode_image(x.cuda()).cpu(), ref), _maxnorm_err(emu, ref)
        print(f'{arch} layers={layers} seed={seed} bf16: hip {e_hip:.2e}  bf16 emulation {e_emu:.2e}')
        slack = 1.0 if layers is None else 1.05
        assert e_hip <= slack * e_emu, (arch, seed, e_hip, e_emu)


# ---- ec_resnet_encode's buffers and input modes ----
_MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073])
_STD = torch.tensor([0.26862954, 0.26130258, 0.27577711])
_GUARD, _GUARD_BYTES = 0x5A, 1 << 20


def _frames(n, R, seed):
    """uint8 HWC frames and the fp32 CHW images CLIP's ToTensor + Normalize make of them (on the CPU)."""
    u8 = torch.randint(0, 256, (n, R, R, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u8, ((u8.float() / 255 - _MEAN) / _STD).permute(0, 3, 1, 2).contiguous()


def _encode_guarded(lib, rw, inp, mode, n, chunk, E, short=0):
    """ec_resnet_encode with a workspace of exactly ec_resnet_workspace_bytes(min(chunk, n)) (less ``short``) bytes
    followed by a guard, and feats followed by guard rows -> (rc, feats [n, E]); asserts both guards intact."""
    import ctypes
    from eventclip_amd import _lib
    need = lib.ec_resnet_workspace_bytes(ctypes.byref(rw), min(chunk, n))
    assert need > 0
    ws = torch.full((need + _GUARD_BYTES,), _GUARD, dtype=torch.uint8, device='cuda')
    feats = torch.empty((n + 4) * E, dtype=torch.float32, device='cuda')
    feats.view(torch.uint8).fill_(_GUARD)
    rc = lib.ec_resnet_encode(ctypes.byref(rw), _lib.ptr(inp), mode, n, _lib.ptr(feats), _lib.ptr(ws), need - short,
                              chunk, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int((ws[need - short:] != _GUARD).sum()) == 0, ('workspace guard', chunk, mode)
    assert int((feats[n * E:].view(torch.uint8) != _GUARD).sum()) == 0, ('feats guard', chunk, mode)
    return rc, feats[:n * E].view(n, E)


@pytest.mark.parametrize('arch,layers', [(a, (1, 1, 1, 1)) for a, _ in _TOWERS] + [('RN50', None)])
def test_encode_stays_in_its_buffers(arch, layers):
    """ec_resnet_encode, called through the C ABI with ResNetCLIP._pack()'s weights, writes nothing past the
    workspace ec_resnet_workspace_bytes(min(chunk, n)) asks for nor past feats, for 5 images in chunks of 1, 2, 5 and
    8 and both input modes; the features are bit-identical across chunk sizes and input modes, and a workspace one
    byte short is refused."""
    from eventclip_amd import _lib
    lib = _lib.lib()
    cfg, sd, m = _model(arch, layers, 0)
    rw = m._pack()['resnet']
    n, R, E = 5, cfg['image_size'], cfg['embed_dim']
    u8, img = _frames(n, R, 7)
    first = None
    for mode, inp in ((_lib.EC_PRE_HWC_U8, u8.cuda()), (_lib.EC_PRE_CHW_F32, img.cuda())):
        for chunk in (1, 2, 5, 8):
            rc, f = _encode_guarded(lib, rw, inp, mode, n, chunk, E)
            _lib.check(rc, 'ec_resnet_encode')
            assert torch.isfinite(f).all()
            if first is None:
                first = f.clone()
            assert torch.equal(f, first), (mode, chunk)
        rc, _ = _encode_guarded(lib, rw, inp, mode, n, 2, E, short=1)
        assert rc == _lib.EC_ERR_INVALID and b'workspace' in lib.ec_last_error()


@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
@pytest.mark.parametrize('arch,layers', [('RN50', None), ('RN50x4', (1, 1, 1, 1))])
def test_input_modes_bit_identical(arch, layers, dtype):
    """encode_frames on uint8 frames and encode_image on ((u8 / 255 - mean) / std) computed on the CPU feed the same
    stem rows, so their features agree bit for bit."""
    cfg, sd, m = _model(arch, layers, 1, dtype=dtype)
    u8, img = _frames(3, cfg['image_size'], 11)
    a = m.encode_frames(u8.cuda())
    b = m.encode_image(img.cuda())
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_zero_shot_classifier_events_match_images():
    """ZSCLIPClassifier on build_random('RN50'): the event pipeline's uint8 frames through the stem kernel give the
    logits of the same classifier fed encode_image on the fp32 images of the same frames."""
    from eventclip_amd import clip as eclip
    from eventclip_amd.clip_cls import ZSCLIPClassifier
    from eventclip_amd.event2img import build_event2img_pipeline
    from eventclip_amd.synthetic import make_batch

    class P:
        quantize_args = dict(max_imgs=2, N=30000, split_method='event_count', convert_method='event_histogram',
                             grayscale=True, count_non_zero=True, background_mask=False)
    model_clip = eclip.build_random('RN50', seed=0)
    assert not hasattr(model_clip, 'kpad') and model_clip.visual.output_dim == 1024
    model = ZSCLIPClassifier(clip_dict=dict(clip_model=model_clip, prompt='a {}', class_names=list('abcde'),
                                            agg_func='mean', class_tokens=eclip.synthetic_tokens(5, seed=0))).cuda().eval()
    res = (100, 120)
    pipe = build_event2img_pipeline(P, res, 60000, clip_model=model_clip)
    evs = make_batch(3, [65000, 12500, 40000], res, seed=1)
    batch = pipe(evs)
    assert 'frames_u8' in batch and 'patches' not in batch and 'img' not in batch
    out = model(batch)
    # the same frames as the reference's fp32 images (ToTensor + Normalize of the uint8 frames)
    u8 = batch['frames_u8'].cpu()
    chw = ((u8.float() / 255 - torch.tensor([0.48145466, 0.4578275, 0.40821073])) /
           torch.tensor([0.26862954, 0.26130258, 0.27577711])).permute(0, 3, 1, 2).cuda()
    vm = batch['valid_mask']
    img = torch.zeros(vm.shape + (3, 224, 224), device='cuda')
    img[vm] = chw
    out2 = model({'img': img, 'valid_mask': vm})
    assert torch.equal(out['logits'].argmax(-1), out2['logits'].argmax(-1))
    assert float((out['logits'] - out2['logits']).abs().max()) < 1e-3


def test_few_shot_text_trans_adapter_at_640():
    from eventclip_amd import clip as eclip
    from eventclip_amd.clip_cls import FSCLIPClassifier
    cfg, sd, m = _model('RN50x4', (1, 1, 1, 1), 0)
    assert m.visual.output_dim == 640
    model = FSCLIPClassifier(adapter_dict=dict(adapter_type='text-trans', in_dim=640, residual=0.8),
                             clip_dict=dict(clip_model=m, prompt='a {}', class_names=list('wxyz'), agg_func='mean',
                                            class_tokens=eclip.synthetic_tokens(4, seed=1)),
                             loss_dict=dict(use_logits_loss=True, use_probs_loss=False)).cuda().eval()
    valid = torch.tensor([[True, True], [True, False]])
    imgs = torch.randn(2, 2, 3, 288, 288, generator=torch.Generator().manual_seed(0)) * valid[:, :, None, None, None]
    out = model({'img': imgs.cuda(), 'valid_mask': valid.cuda()})
    assert out['logits'].shape == (2, 4) and torch.isfinite(out['logits']).all()
    assert np.isfinite(float(out['probs'].sum()))
