"""LayerNorm, attention and the two CLIP towers on the MI355X against torch fp32."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
@pytest.mark.parametrize('width', [256, 512, 640, 768, 1024])
def test_layernorm(width, dt, hip):
    import torch
    import torch.nn.functional as F
    from eventclip_amd import _lib
    dtype = getattr(torch, dt)
    x = torch.randn(301, width, device='cuda') * 3 + 1
    g, b = torch.randn(width, device='cuda'), torch.randn(width, device='cuda')
    out = torch.empty(301, width, dtype=dtype, device='cuda')
    _lib.check(_lib.lib().ec_layernorm(_lib.ptr(x), width, None, _lib.ptr(g), _lib.ptr(b), 301, width,
                                       1e-5, _lib.ptr(out), width,
                                       _lib.EC_F16 if dt == 'float16' else _lib.EC_BF16,
                                       _lib.stream_ptr()))
    want = F.layer_norm(x, (width,), g, b, 1e-5)
    tol = 2e-3 if dt == 'float16' else 1.6e-2
    torch.testing.assert_close(out.float(), want, rtol=tol, atol=tol)
    # gathered rows (ln_post on CLS rows / ln_final on EOT rows)
    idx = torch.tensor([5, 0, 300, 17], dtype=torch.int32, device='cuda')
    out2 = torch.empty(4, width, dtype=dtype, device='cuda')
    _lib.check(_lib.lib().ec_layernorm(_lib.ptr(x), width, _lib.ptr(idx), _lib.ptr(g), _lib.ptr(b), 4,
                                       width, 1e-5, _lib.ptr(out2), width,
                                       _lib.EC_F16 if dt == 'float16' else _lib.EC_BF16,
                                       _lib.stream_ptr()))
    torch.testing.assert_close(out2.float(), want[idx.long()], rtol=tol, atol=tol)


def ref_attention(qkv, n_seq, S, W, heads, causal):
    import torch
    q, k, v = qkv.float().view(n_seq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    att = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        att = att + torch.full((S, S), float('-inf'), device=qkv.device).triu_(1)
    out = att.softmax(-1) @ v
    return out.permute(0, 2, 1, 3).reshape(n_seq * S, W)


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
@pytest.mark.parametrize('rows,width', [(301, 1024), (9, 768), (64, 64), (1000, 1280)])
def test_layernorm_of_the_planes(rows, width, dt, hip):
    """ec_layernorm_hl: LayerNorm of x = hi + lo (the folded chain's residual planes) into hi + lo parts, against fp64."""
    import torch
    from eventclip_amd import ops
    dtype = getattr(torch, dt)
    g = torch.Generator(device='cuda').manual_seed(rows + width)
    x = torch.randn(rows, width, device='cuda', generator=g) * 3 + 0.7
    hi = x.to(dtype)
    lo = (x - hi.float()).half()
    gamma = 1 + 0.2 * torch.randn(width, device='cuda', generator=g)
    beta = 0.3 * torch.randn(width, device='cuda', generator=g)
    o_hi, o_lo = ops.layernorm_hl(hi, lo, gamma, beta)
    want = torch.nn.functional.layer_norm(hi.double() + lo.double(), (width,), gamma.double(), beta.double(), 1e-5)
    err = float(((o_hi.double() + o_lo.double()) - want).abs().max() / want.abs().max())
    assert err < (2e-6 if dt == 'float16' else 4e-5), err           # (bf16 parts carry 16 bits together)
    assert float((o_hi.double() - want).abs().max()) <= (2 ** -10 if dt == 'float16' else 2 ** -7) * float(want.abs().max())


@pytest.mark.parametrize('S,heads,causal,n_seq', [(257, 16, 0, 3), (577, 4, 0, 2), (77, 8, 1, 5), (77, 12, 1, 3),
                                                   (50, 12, 0, 4), (197, 3, 0, 2), (1, 2, 0, 2), (1, 1, 1, 1),
                                                   (33, 2, 1, 3), (64, 1, 0, 2), (65, 1, 1, 2), (129, 2, 1, 2)])
def test_attention_f32_matches_float64(S, heads, causal, n_seq, hip):
    """ec_attention_f32 (the split-precision towers' attention: fp32 qkv in, hi + lo 16-bit planes out) on the fp32
    matrix instruction against a float64 softmax attention: 4e-6 of the largest output (the hi + lo pair itself carries
    2^-22), every sequence length the towers run plus the chunk / tile edges (32-key chunks, 64-query workgroups)."""
    import torch
    from eventclip_amd import _lib
    W = heads * 64
    g = torch.Generator(device='cuda').manual_seed(S * 131 + heads)
    qkv = torch.randn(n_seq * S, 3 * W, device='cuda', generator=g) * 1.7
    hi = torch.full((n_seq * S, W), float('nan'), dtype=torch.float16, device='cuda')
    lo = torch.full((n_seq * S, W), float('nan'), dtype=torch.float16, device='cuda')
    _lib.check(_lib.lib().ec_attention_f32(_lib.ptr(qkv), _lib.ptr(hi), _lib.ptr(lo), n_seq, S, W, heads, causal,
                                           _lib.EC_F16, _lib.stream_ptr()), 'ec_attention_f32')
    q, k, v = qkv.double().view(n_seq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    att = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        att = att + torch.full((S, S), float('-inf'), device='cuda', dtype=torch.float64).triu_(1)
    want = (att.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(n_seq * S, W)
    got = hi.double() + lo.double()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max() / want.abs().max())
    assert err < 4e-6, err


@pytest.mark.parametrize('prescaled', [0, 1])
@pytest.mark.parametrize('S,heads,n_seq', [(257, 16, 3), (577, 4, 2), (50, 12, 4), (197, 3, 2), (1, 2, 2), (64, 1, 2), (65, 1, 2),
                                           (288, 2, 2), (289, 2, 3), (353, 2, 3), (608, 1, 2), (609, 1, 2), (320, 3, 2)])
def test_attention_split_matches_float64(S, heads, n_seq, prescaled, hip):
    """ec_attention_split (the attention of the first split-operand blocks): q | k | v as hi + lo fp16 parts -- a plain q, or
    the q columns pre-multiplied by log2(e) / sqrt(64) -- against a float64 softmax attention of the joined values.  A plain q
    runs on the 16-bit matrix instruction with hi + lo operands: one pass over the keys up to S = 288 (attention_hl_kernel),
    two passes with the tiles' state in registers up to S = 608 (attention_hl2_kernel), the fp32-MFMA kernel beyond and for a
    pre-scaled q: the sequence lengths sit on both sides of each boundary."""
    import torch
    from eventclip_amd import _lib
    W = heads * 64
    g = torch.Generator(device='cuda').manual_seed(S * 17 + heads)
    qkv = torch.randn(n_seq * S, 3 * W, device='cuda', generator=g) * 1.7
    scaled = qkv.clone()
    if prescaled:
        scaled[:, :W] *= 0.125 * 1.4426950408889634
    pair = torch.empty((2, n_seq * S, 3 * W), dtype=torch.float16, device='cuda')
    pair[0] = scaled.half()
    pair[1] = (scaled - pair[0].float()).half()
    joined = pair[0].double() + pair[1].double()
    joined[:, :W] *= (1 / 1.4426950408889634) if prescaled else 0.125       # to q / 8 (natural-log softmax below)
    hi = torch.full((n_seq * S, W), float('nan'), dtype=torch.float16, device='cuda')
    lo = torch.full((n_seq * S, W), float('nan'), dtype=torch.float16, device='cuda')
    _lib.check(_lib.lib().ec_attention_split(_lib.ptr(pair[0]), _lib.ptr(pair[1]), _lib.ptr(hi), _lib.ptr(lo), n_seq, S, W,
                                             heads, prescaled, _lib.EC_F16, _lib.stream_ptr()), 'ec_attention_split')
    q, k, v = joined.view(n_seq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    want = ((q @ k.transpose(-1, -2)).softmax(-1) @ v).permute(0, 2, 1, 3).reshape(n_seq * S, W)
    got = hi.double() + lo.double()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max() / want.abs().max())
    assert err < 4e-6, err


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
@pytest.mark.parametrize('S,heads,causal', [(50, 12, 0), (77, 8, 1), (77, 12, 1), (197, 12, 0),
                                            (257, 16, 0), (577, 16, 0), (17, 1, 0), (1, 2, 1)])
def test_attention(S, heads, causal, dt, hip):
    import torch
    from eventclip_amd import _lib
    dtype = getattr(torch, dt)
    n_seq, W = 3, heads * 64
    qkv = (torch.randn(n_seq * S, 3 * W, device='cuda') * 1.5).to(dtype)
    out = torch.empty(n_seq * S, W, dtype=dtype, device='cuda')
    _lib.check(_lib.lib().ec_attention(_lib.ptr(qkv), _lib.ptr(out), n_seq, S, W, heads, causal,
                                       _lib.EC_F16 if dt == 'float16' else _lib.EC_BF16,
                                       _lib.stream_ptr()))
    want = ref_attention(qkv, n_seq, S, W, heads, causal)
    tol = 4e-3 if dt == 'float16' else 2.5e-2     # P and the output are rounded to 16 bit
    torch.testing.assert_close(out.float(), want, rtol=tol, atol=tol)


def test_fp16_reference_emulation_against_torch_half_on_the_gpu(hip):
    """The yardstick of the logit-parity tests (oracle/clip_ref.py emulate='fp16_reference': the arithmetic the
    reference runs on its GPU, /root/reference/test.py:25-26) against torch's half kernels ON THE GPU -- the vendor
    GEMM library, fused attention and elementwise kernels a `clip.load(arch, 'cuda')` model would run here -- at
    ViT-L/14's width, head count and sequence length, four blocks: both fp16 realisations sit at the same distance
    from fp32 (within 2x) and no further from each other than two such realisations are."""
    from test_oracle_clip import fp16_emulation_distances
    d_emu_torch, d_torch_exact, d_emu_exact = fp16_emulation_distances('cuda', W=1024, heads=16, S=257, N=2, L=4, seed=5)
    print(f'\nfp16 emulation vs torch half on the GPU {d_emu_torch:.2e}; torch half vs fp32 {d_torch_exact:.2e}; '
          f'emulation vs fp32 {d_emu_exact:.2e}')
    assert d_emu_torch < 2.0 * d_torch_exact, (d_emu_torch, d_torch_exact)
    assert 0.5 < d_emu_exact / d_torch_exact < 2.0, (d_emu_exact, d_torch_exact)


@pytest.mark.parametrize('S', [609, 640])
def test_attention_at_the_lds_limit(S, hip):
    """S = 609 .. 640 is twenty 32-key blocks: exactly 160 KiB of K and V.  The merge area of a split query tile is
    only reserved where the kernel can split one, so these lengths fit; one more key does not and says why."""
    import torch
    from eventclip_amd import _lib
    n_seq, heads = 2, 2
    W = heads * 64
    qkv = (torch.randn(n_seq * S, 3 * W, device='cuda') * 1.5).half()
    out = torch.empty(n_seq * S, W, dtype=torch.float16, device='cuda')
    _lib.check(_lib.lib().ec_attention(_lib.ptr(qkv), _lib.ptr(out), n_seq, S, W, heads, 0, _lib.EC_F16, _lib.stream_ptr()))
    torch.testing.assert_close(out.float(), ref_attention(qkv, n_seq, S, W, heads, 0), rtol=4e-3, atol=4e-3)
    if S == 640:
        big = torch.zeros(641, 3 * W, device='cuda', dtype=torch.float16)
        with pytest.raises(RuntimeError, match='S <= 640'):
            _lib.check(_lib.lib().ec_attention(_lib.ptr(big), _lib.ptr(out), 1, 641, W, heads, 0, _lib.EC_F16,
                                               _lib.stream_ptr()), 'ec_attention')


def test_attention_exact_selector(hip):
    """One-hot softmax (huge matching score) must copy the right V row for every query:
    catches any mismatch between the P^T and V^T operand permutations."""
    import torch
    from eventclip_amd import _lib
    S, heads, W = 257, 2, 128
    perm = torch.randperm(S)
    q = torch.zeros(S, W)
    k = torch.zeros(S, W)
    code = (torch.arange(S)[:, None] >> torch.arange(9)[None]) & 1      # 9-bit binary codes
    code = code.float() * 2 - 1
    for h in range(heads):
        q[:, h * 64:h * 64 + 9] = code[perm] * 16
        k[:, h * 64:h * 64 + 9] = code * 16
    v = torch.arange(S)[:, None].float() + torch.arange(W)[None].float() / 256
    qkv = torch.cat([q, k, v], 1).half().cuda()
    out = torch.empty(S, W, dtype=torch.float16, device='cuda')
    _lib.check(_lib.lib().ec_attention(_lib.ptr(qkv), _lib.ptr(out), 1, S, W, heads, 0, _lib.EC_F16,
                                       _lib.stream_ptr()))
    want = v.half()[perm]
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
@pytest.mark.parametrize('S,spike_keys', [(257, (70,)), (257, (5, 130, 256)), (577, (100, 300, 570)),
                                          (197, (64, 128, 196)), (77, (40, 76))])
def test_attention_running_maximum_moves(S, spike_keys, dt, hip):
    """The kernel keeps a query's running maximum where it is while a block's scores stay within 2^10 of it and
    only otherwise moves it (rescaling O and the row sum once).  Bounded random data never takes that branch
    after a tile's first block, so force it: chosen keys, in chosen later blocks, score far above everything
    before them for SOME queries (each spike larger than the last), and the whole output is checked against
    fp32 -- rows that moved, rows that did not, and rows of the same 16-query tile as a row that moved."""
    import torch
    from eventclip_amd import _lib
    dtype = getattr(torch, dt)
    torch.manual_seed(S + len(spike_keys))
    n_seq, heads = 2, 3
    W = heads * 64
    q = torch.randn(n_seq, S, heads, 64)
    k = torch.randn(n_seq, S, heads, 64)
    v = torch.randn(n_seq, S, heads, 64)
    for i, key in enumerate(spike_keys):
        # queries 3 (i + 1) j + 1 line up with key `key`: score ~ 8 * (4 + 3 i) * 64 / 8 natural units above the rest
        rows = torch.arange(1, S, 3 * (i + 1))
        direction = torch.sign(torch.randn(64))
        k[:, key] = direction * (4.0 + 3 * i)
        q[:, rows] = q[:, rows] * 0.25 + direction * 2.0
    qkv = torch.cat([q.reshape(n_seq * S, W), k.reshape(n_seq * S, W), v.reshape(n_seq * S, W)], 1)
    qkv = qkv.to(dtype).cuda()
    out = torch.empty(n_seq * S, W, dtype=dtype, device='cuda')
    _lib.check(_lib.lib().ec_attention(_lib.ptr(qkv), _lib.ptr(out), n_seq, S, W, heads, 0,
                                       _lib.EC_F16 if dt == 'float16' else _lib.EC_BF16, _lib.stream_ptr()))
    want = ref_attention(qkv, n_seq, S, W, heads, 0)
    assert torch.isfinite(out.float()).all()
    # bf16: the spiked scores are O(100) and carry the 2^-9 relative rounding of q, k AND of the pre-scaled q
    tol = 4e-3 if dt == 'float16' else 4e-2
    torch.testing.assert_close(out.float(), want, rtol=tol, atol=tol)


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
@pytest.mark.parametrize('S,heads,q_rows', [(257, 16, 257), (257, 2, 1), (577, 3, 577), (50, 12, 50), (197, 2, 20)])
def test_attention_scaled_q(S, heads, q_rows, dt, hip):
    """ec_attention_scaled_q: the q columns hold q * log2(e) / sqrt(64) (what ec_vit_weights.q_scaled packs);
    softmax(q k^T / 8) v must come out -- checked against fp32 on the rounded operands the kernel sees."""
    import math
    import torch
    from eventclip_amd import _lib
    dtype = getattr(torch, dt)
    torch.manual_seed(S + q_rows)
    n_seq, W = 3, heads * 64
    c = 0.125 * 1.4426950408889634
    qkv32 = torch.randn(n_seq * S, 3 * W, device='cuda') * 1.5
    qkv32[:, :W] *= c
    qkv = qkv32.to(dtype)
    out = torch.empty(n_seq * q_rows, W, dtype=dtype, device='cuda')
    _lib.check(_lib.lib().ec_attention_scaled_q(_lib.ptr(qkv), _lib.ptr(out), n_seq, S, W, heads, 0, q_rows,
                                                _lib.EC_F16 if dt == 'float16' else _lib.EC_BF16,
                                                _lib.stream_ptr()))
    q, k, v = qkv.float().view(n_seq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    att = (q @ k.transpose(-1, -2)) * math.log(2.0)          # exp2(q' k) = exp(ln 2 q' k)
    want = (att.softmax(-1) @ v).permute(0, 2, 1, 3)[:, :q_rows].reshape(n_seq * q_rows, W)
    tol = 4e-3 if dt == 'float16' else 2.5e-2
    torch.testing.assert_close(out.float(), want, rtol=tol, atol=tol)


def test_attention_lse_matches_reference(hip):
    """ec_attention_train's log-sum-exp (log2 domain, scaled scores) against fp32, incl. rows whose maximum moved."""
    import torch
    from eventclip_amd import _lib
    torch.manual_seed(11)
    n_seq, S, heads = 2, 257, 2
    W = heads * 64
    qkv = torch.randn(n_seq * S, 3 * W) * 1.5
    qkv[130, W:W + 64] = 6.0           # key 130 of sequence 0, head 0: a late spike for positive-sum queries
    qkv = qkv.half().cuda()
    out = torch.empty(n_seq * S, W, dtype=torch.float16, device='cuda')
    lse = torch.empty(n_seq, heads, S, dtype=torch.float32, device='cuda')
    _lib.check(_lib.lib().ec_attention_train(_lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), n_seq, S, W, heads,
                                             _lib.EC_F16, _lib.stream_ptr()))
    q, k, v = qkv.float().view(n_seq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    att = (q * 0.125) @ k.transpose(-1, -2)
    want = torch.logsumexp(att, -1) * 1.4426950408889634
    torch.testing.assert_close(lse, want, rtol=2e-3, atol=2e-2)
    torch.testing.assert_close(out.float(), ref_attention(qkv, n_seq, S, W, heads, 0), rtol=4e-3, atol=4e-3)


def load_tiny():
    import torch
    from conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, 'clip_tiny.npz'))
    cfg = {str(k): int(v) for k, v in zip(z['cfg_keys'], z['cfg_vals'])}
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith('w:')}
    sd['logit_scale'] = torch.tensor(float(np.log(100.0)))
    return cfg, sd, z


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
def test_tiny_clip_matches_hf_fixture(dt, hip):
    import torch
    from eventclip_amd import clip as eclip
    cfg, sd, z = load_tiny()
    model = eclip.CLIP(cfg, sd, dtype=dt).cuda().eval()
    img = torch.from_numpy(z['img'].astype(np.float32)).cuda()
    tok = torch.from_numpy(z['tok']).cuda()
    gi = model.encode_image(img).cpu()
    gt = model.encode_text(tok).cpu()
    tol = 2e-3 if dt == 'float16' else 1.5e-2
    assert rel_err(gi, torch.from_numpy(z['hf_img'])) < tol
    assert rel_err(gt, torch.from_numpy(z['hf_txt'])) < tol


def seeded(name):
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, 'towers_seeded.npz'))[name]


@pytest.mark.parametrize('name,arch,ov,n', [
    ('vitl14', 'ViT-L/14', dict(text_layers=1, vocab_size=1024), 2),
    ('vitb32', 'ViT-B/32', dict(text_layers=1, vocab_size=1024), 3),
    ('vitl14_336', 'ViT-L/14@336px', dict(layers=4, text_layers=1, vocab_size=1024), 1)])
@pytest.mark.parametrize('dt,tol', [('float16', 1e-3), ('bfloat16', 1e-2)])
def test_image_tower_matches_oracle_fixture(name, arch, ov, n, dt, tol, hip):
    """Full-width (and for L/14, B/32 full-depth) towers with seeded random weights against
    the fp32 CPU oracle's stored outputs (tools/make_golden_vit.py).  Tolerance: north_star's
    1e-3 relative (max |diff| / max |ref|) with f16 operands; bf16 operands are ~8x coarser."""
    import torch
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config(arch, **ov)
    sd = eclip.random_state_dict(cfg, seed=11)
    model = eclip.CLIP(cfg, sd, dtype=dt).cuda().eval()
    R = cfg['image_size']
    img = torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(5))
    assert abs(float(img.double().sum()) - float(seeded(name + '_img_checksum'))) < 1e-6
    got = model.encode_image(img.cuda()).cpu()
    want = torch.from_numpy(seeded(name))
    assert got.shape == want.shape == (n, cfg['embed_dim'])
    assert rel_err(got, want) < tol
    if dt == 'float16':   # same 16-bit-rounded weights on both sides: arithmetic error only
        assert rel_err(got, torch.from_numpy(seeded(name + '_w16'))) < tol
    # and against HF transformers' CLIP vision tower run on the same weights / images (tools/make_golden_vit.py)
    assert rel_err(got, torch.from_numpy(seeded(name + '_hf'))) < tol


@pytest.mark.parametrize('S,heads,causal,q_rows', [(257, 16, 0, 1), (257, 16, 0, 20), (50, 12, 0, 1),
                                                   (577, 16, 0, 1), (77, 8, 1, 5),
                                                   # S = 577 and 593 on 16 waves (37 and 38 tiles: no tile is split over
                                                   # the waves): q_rows that end inside the waves' third round of tiles
                                                   # (32 ..), part of that round / all of it but the last row requested
                                                   (577, 16, 0, 530), (577, 16, 0, 576), (593, 4, 0, 550)])
def test_attention_rows_is_a_prefix_of_full_attention(S, heads, causal, q_rows, hip):
    """ec_attention_rows(q_rows) == the first q_rows rows of every sequence of ec_attention, bit for bit."""
    import torch
    from eventclip_amd import _lib
    n_seq, W = 5, heads * 64
    qkv = (torch.randn(n_seq * S, 3 * W, device='cuda') * 1.5).half()
    full = torch.empty(n_seq * S, W, dtype=torch.float16, device='cuda')
    part = torch.full((n_seq * q_rows, W), float('nan'), dtype=torch.float16, device='cuda')
    _lib.check(_lib.lib().ec_attention(_lib.ptr(qkv), _lib.ptr(full), n_seq, S, W, heads, causal, _lib.EC_F16,
                                       _lib.stream_ptr()))
    _lib.check(_lib.lib().ec_attention_rows(_lib.ptr(qkv), _lib.ptr(part), n_seq, S, W, heads, causal, q_rows,
                                            _lib.EC_F16, _lib.stream_ptr()))
    want = full.view(n_seq, S, W)[:, :q_rows].reshape(n_seq * q_rows, W)
    assert torch.equal(part.view(torch.int16), want.contiguous().view(torch.int16))


@pytest.mark.parametrize('arch,ov,n', [('ViT-L/14', dict(layers=3, text_layers=1, vocab_size=1024), 5),
                                       ('ViT-B/32', dict(text_layers=1, vocab_size=1024), 7),
                                       ('ViT-B/16', dict(layers=1, text_layers=1, vocab_size=1024), 2)])
def test_class_token_only_last_block_is_bit_identical(arch, ov, n, hip):
    """The default image tower sends only the class-token rows through the last block's attention
    query / out_proj / MLP; computing every token (like the reference) gives the same features."""
    import torch
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config(arch, **ov)
    sd = eclip.random_state_dict(cfg, seed=21)
    img = torch.randn(n, 3, cfg['image_size'], cfg['image_size'], generator=torch.Generator().manual_seed(8)).cuda()
    fast = eclip.CLIP(cfg, sd).cuda().eval()
    full = eclip.CLIP(cfg, sd, full_last_block=True).cuda().eval()
    assert not fast.full_last_block and full.full_last_block
    a, b = fast.encode_image(img), full.encode_image(img)
    assert torch.equal(a, b)


def test_small_tower_matches_live_oracle(hip):
    import torch
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg = eclip.arch_config('ViT-B/16', layers=2, text_layers=1, vocab_size=1024)
    sd = eclip.random_state_dict(cfg, seed=4)
    model = eclip.CLIP(cfg, sd, dtype='float16').cuda().eval()
    img = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(6))
    got = model.encode_image(img.cuda()).cpu()
    assert rel_err(got, clip_ref.encode_image(sd, cfg, img)) < 1e-3


@pytest.mark.parametrize('precise,tol', [(True, 2e-5), (False, 1e-3)])
@pytest.mark.parametrize('name,arch', [('text_l14', 'ViT-L/14'), ('text_b32', 'ViT-B/32')])
def test_text_tower_matches_oracle_fixture(name, arch, precise, tol, hip):
    """Default: split-precision text tower (x.w = xh.wh + xh.wl + xl.wh in fp32, fp32 attention)
    -- text features are computed once and cached, so they are kept at fp32 accuracy."""
    import torch
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config(arch, layers=1)
    sd = eclip.random_state_dict(cfg, seed=12)
    model = eclip.CLIP(cfg, sd, dtype='float16', text_precise=precise).cuda().eval()
    tok = eclip.synthetic_tokens(9, seed=3)
    got = model.encode_text(tok.cuda()).cpu()
    assert rel_err(got, torch.from_numpy(seeded(name))) < tol
    assert rel_err(got, torch.from_numpy(seeded(name + '_hf'))) < tol      # HF transformers, same weights / tokens


def test_precise_image_tower_reproduces_fp32_oracle(hip):
    """The same MFMA kernels in split-precision mode agree with the fp32 oracle to ~1e-5 on a
    full-depth ViT-B/32: what remains in the fast path is 16-bit rounding, not algorithm."""
    import torch
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config('ViT-B/32', text_layers=1, vocab_size=1024)
    sd = eclip.random_state_dict(cfg, seed=11)
    model = eclip.CLIP(cfg, sd, dtype='float16', image_precise=True).cuda().eval()
    img = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(5)).half().float()
    got = model.encode_image(img.cuda()).cpu()
    # the fixture was made with the unrounded images; f16-rounding the input costs ~6e-5
    assert rel_err(got, torch.from_numpy(seeded('vitb32'))) < 2e-4
    from oracle import clip_ref
    small = eclip.arch_config('ViT-B/32', layers=3, text_layers=1, vocab_size=1024)
    sd3 = eclip.random_state_dict(small, seed=3)
    m3 = eclip.CLIP(small, sd3, dtype='float16', image_precise=True).cuda().eval()
    assert rel_err(m3.encode_image(img.cuda()).cpu(), clip_ref.encode_image(sd3, small, img)) < 2e-5


def test_bf16_operands_reach_1e3_only_in_split_mode(hip):
    """north_star names bf16 MFMA operands and 1e-3: bf16 has 8 significant bits, so the plain path is
    ~4e-3 off the fp32 oracle; carried as hi + lo parts (the split-precision tower: three MFMA launches
    per GEMM on the same bf16 instruction) it is inside 1e-3 with two orders to spare."""
    import torch
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg = eclip.arch_config('ViT-B/32', layers=3, text_layers=1, vocab_size=1024)
    sd = eclip.random_state_dict(cfg, seed=3)
    img = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    want = clip_ref.encode_image(sd, cfg, img)
    plain = eclip.CLIP(cfg, sd, dtype='bfloat16').cuda().eval().encode_image(img.cuda()).cpu()
    split = eclip.CLIP(cfg, sd, dtype='bfloat16', image_precise=True).cuda().eval().encode_image(img.cuda()).cpu()
    assert 1e-3 < rel_err(plain, want) < 1e-2
    assert rel_err(split, want) < 1e-4


def test_chunked_encode_is_batch_invariant(hip):
    import torch
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config('ViT-B/32', layers=2, text_layers=1, vocab_size=1024)
    sd = eclip.random_state_dict(cfg, seed=1)
    img = torch.randn(7, 3, 224, 224).cuda()
    a = eclip.CLIP(cfg, sd, chunk=256).cuda().encode_image(img)
    b = eclip.CLIP(cfg, sd, chunk=3).cuda().encode_image(img)
    assert torch.equal(a, b)


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
def test_precise_blocks_tower(dt, hip):
    """ec_vit_weights.precise_blocks on a 4-block ViT-B/32: the error against the fp32 oracle falls with the number of
    leading split-operand blocks (0 -> 1 -> 3), all of them but one is already close to the split-precision tower;
    chunked and whole-batch calls agree bit for bit; the class-token-only last block stays bit-identical; and the
    packing refuses what the mode cannot do (every block, the plain chain, low latency, a bf16 tower: the lo plane of
    the residual stream is fp16 and only an f16 MFMA can multiply it)."""
    import torch
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg = eclip.arch_config('ViT-B/32', layers=4, text_layers=1, vocab_size=1024)
    sd = eclip.random_state_dict(cfg, seed=3, qk_gain=2.0, branch_gain=3.0)
    img = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    if dt == 'bfloat16':
        with pytest.raises(ValueError):
            eclip.CLIP(cfg, sd, dtype=dt, image_precise_blocks=2).cuda().encode_image(img.cuda())
        return
    want = clip_ref.encode_image(sd, cfg, img)
    errs = {}
    for n in (0, 1, 3):
        m = eclip.CLIP(cfg, sd, dtype=dt, image_precise_blocks=n).cuda().eval()
        errs[n] = rel_err(m.encode_image(img.cuda()).cpu(), want)
    print('\n[precise_blocks on 4 blocks, %s] error vs fp32: %s' % (dt, {k: f'{v:.2e}' for k, v in errs.items()}))
    assert errs[3] < errs[1] < errs[0], errs
    assert errs[3] < 0.5 * errs[0], errs
    a = eclip.CLIP(cfg, sd, dtype=dt, image_precise_blocks=2, chunk=256).cuda().encode_image(img.cuda())
    b = eclip.CLIP(cfg, sd, dtype=dt, image_precise_blocks=2, chunk=2).cuda().encode_image(img.cuda())
    c = eclip.CLIP(cfg, sd, dtype=dt, image_precise_blocks=2, full_last_block=True).cuda().encode_image(img.cuda())
    assert torch.equal(a, b) and torch.equal(a, c)
    for kw in (dict(image_precise_blocks=4), dict(image_precise_blocks=2, ln_folded=False),
               dict(image_precise_blocks=2, low_latency=True)):
        with pytest.raises(ValueError):
            eclip.CLIP(cfg, sd, dtype=dt, **kw).cuda().encode_image(img.cuda())


@pytest.mark.parametrize('f16_weights', [False, True])
def test_split_operand_blocks_with_e4m3_lo_products(f16_weights, hip):
    """ec_vit_weights.lo_fp8 (round 6): the lo products of the split-operand blocks' QKV / c_fc / c_proj GEMMs as e4m3
    operands.  On a 4-block ViT-B/32 with three split-operand blocks (two of them with fp32-class attention): the features are as
    close to the fp32 oracle as the 16-bit-lo form's (the two forms differ from EACH OTHER by about that error: the 16-bit
    block behind them rounds a slightly different input differently, so its rounding errors decorrelate -- the reason why
    the max-normalised error moves by +- 15 % between forms of equal accuracy); the e4m3 weights are packed exactly where the C side needs them (lo parts only
    where the matrix has one: none on a checkpoint stored in 16 bit); chunked and whole-batch calls agree bit for bit."""
    import torch
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg = eclip.arch_config('ViT-B/32', layers=4, text_layers=1, vocab_size=1024)
    sd = eclip.random_state_dict(cfg, seed=3, qk_gain=2.0, branch_gain=3.0)
    if f16_weights:
        sd = {k: (v.half().float() if v.dim() >= 2 else v) for k, v in sd.items()}
    img = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    want = clip_ref.encode_image(sd, cfg, img)
    kw = dict(image_precise_blocks=3, image_precise_attn_blocks=2)
    m8 = eclip.CLIP(cfg, sd, image_lo_fp8=True, **kw).cuda().eval()
    m16 = eclip.CLIP(cfg, sd, image_lo_fp8=False, **kw).cuda().eval()
    f8, f16 = m8.encode_image(img.cuda()).cpu(), m16.encode_image(img.cuda()).cpu()
    assert m8._pack()['vit'].lo_fp8 == 1 and m16._pack()['vit'].lo_fp8 == 0
    b8, b16 = m8._pack()['vb'], m16._pack()['vb']
    for l in range(4):
        split = l < 3
        assert (b8[l].qkv_w8 is not None) == split and (b8[l].fc1_w8 is not None) == split and (b8[l].fc2_w8 is not None) == split
        assert (b8[l].qkv_wlo8 is not None) == (split and not f16_weights) and (b8[l].fc1_wlo8 is not None) == (split and not f16_weights)
        assert b16[l].qkv_w8 is None and b16[l].qkv_wlo8 is None
    e8, e16 = rel_err(f8, want), rel_err(f16, want)
    d = float((f8 - f16).abs().max() / f16.abs().max())
    print(f'\n[lo_fp8 on 3 of 4 blocks, f16 weights {f16_weights}] error vs fp32: e4m3 lo {e8:.2e}, 16-bit lo {e16:.2e}; e4m3 vs 16-bit {d:.2e}')
    assert d < 2 * e16 and e8 < 1.25 * e16 + 1e-5, (d, e8, e16)
    e0 = rel_err(eclip.CLIP(cfg, sd).cuda().eval().encode_image(img.cuda()).cpu(), want)
    assert e8 < 0.6 * e0, (e8, e0)
    a = eclip.CLIP(cfg, sd, image_lo_fp8=True, chunk=2, **kw).cuda().eval().encode_image(img.cuda()).cpu()
    assert torch.equal(a, f8)


def test_weights_stored_in_16_bit_skip_the_lo_product(hip):
    """ec_vit_weights.weights_exact16: on a checkpoint whose matrices are 16-bit values already (what clip.load() returns
    on a GPU) the split-precision blocks pass NULL lo parts and run one MFMA product per GEMM less; the skipped product
    is a sum of zeros, so the features are bit-identical to the form that multiplies the zeros.  (In a split-operand
    block -- precise_blocks -- that holds for out_proj / c_proj; in_proj and c_fc are multiplied by the LayerNorm gain
    before the split, which leaves them a lo part.)"""
    import torch
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config('ViT-B/32', layers=3, text_layers=1, vocab_size=1024)
    sd = {k: (v.half().float() if v.dim() >= 2 else v) for k, v in eclip.random_state_dict(cfg, seed=3).items()}
    img = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(5)).cuda()
    for kw in (dict(image_precise=True), dict(image_precise_blocks=2), dict()):
        two = eclip.CLIP(cfg, sd, **kw).cuda().eval()
        three = eclip.CLIP(cfg, sd, **kw).cuda().eval()
        three.keep_zero_lo = True
        a, b = two.encode_image(img), three.encode_image(img)
        assert two._pack()['vit'].weights_exact16 == 1 and three._pack()['vit'].weights_exact16 == 0
        if kw:
            field = 'qkv_w_lo' if 'image_precise' in kw else 'out_w_lo'
            assert getattr(two._pack()['vb'][0], field) is None and getattr(three._pack()['vb'][0], field) is not None
        # conv1 and proj in every mode (the default chain included): no second patch-embedding launch, two products in proj
        for field in ('conv_w_lo', 'proj_w_lo'):
            assert getattr(two._pack()['vit'], field) is None and getattr(three._pack()['vit'], field) is not None
        assert torch.equal(a, b)


def test_cpu_model_fails_loudly(hip):
    import torch
    from eventclip_amd import _lib
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config('ViT-B/32', layers=1, text_layers=1, vocab_size=1024)
    m = eclip.CLIP(cfg, eclip.random_state_dict(cfg, 0))
    with pytest.raises(_lib.HipLibraryError):
        m.encode_image(torch.zeros(1, 3, 224, 224))


@pytest.mark.parametrize('arch,n', [('ViT-B/32', 1), ('ViT-B/32', 7), ('ViT-L/14', 1), ('ViT-L/14', 3)])
def test_low_latency_mode_gives_the_same_features(hip, arch, n):
    """CLIP(low_latency=True) runs the under-filled GEMM launches of a small request K-batched: the features agree
    with the default mode to the fp32 summation order (and so stay inside the 1e-3 of the fp32 oracle)."""
    import torch
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config(arch)
    sd = eclip.random_state_dict(cfg, seed=3)
    torch.manual_seed(n)
    imgs = torch.randn(n, 3, cfg['image_size'], cfg['image_size'])
    # the K-batched launches run the plain LayerNorm chain (their fix-up kernel has no folded epilogue): compare
    # with the same chain in one pass, and with the default (folded) tower at the 16-bit operands' own tolerance
    base = eclip.CLIP(cfg, sd, ln_folded=False).cuda().encode_image(imgs.cuda())
    fast = eclip.CLIP(cfg, sd, low_latency=True).cuda().encode_image(imgs.cuda())
    assert torch.isfinite(fast).all()
    assert float((fast - base).abs().max()) < 3e-4 * float(base.abs().max())
    assert not torch.equal(fast, base)          # the K-batched route really ran
    folded = eclip.CLIP(cfg, sd).cuda().encode_image(imgs.cuda())
    assert float((folded - base).abs().max()) < 1e-3 * float(base.abs().max())


@pytest.mark.parametrize('arch', ['ViT-B/32', 'ViT-L/14'])
def test_folded_layernorm_tower_matches_the_plain_chain_and_the_oracle(hip, arch):
    """ec_vit_weights.ln_folded (the default): LayerNorm finished in the QKV / c_fc epilogues on the raw hi rows of
    a residual stream kept as hi + lo planes, against the plain LayerNorm launches on an fp32 stream and against
    the fp32 oracle: the same distance from the oracle (the A operand is rounded once either way), and the
    class-token-only last block still bit-identical to computing every token."""
    import torch
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg = eclip.arch_config(arch)
    sd = eclip.random_state_dict(cfg, seed=11)
    torch.manual_seed(4)
    imgs = torch.randn(6, 3, cfg['image_size'], cfg['image_size'])
    want = clip_ref.encode_image(sd, cfg, imgs)
    plain = eclip.CLIP(cfg, sd, ln_folded=False).cuda().encode_image(imgs.cuda()).cpu()
    folded = eclip.CLIP(cfg, sd).cuda().encode_image(imgs.cuda()).cpu()
    every = eclip.CLIP(cfg, sd, full_last_block=True).cuda().encode_image(imgs.cuda()).cpu()
    mag = float(want.abs().max())
    e_plain, e_fold = float((plain - want).abs().max()) / mag, float((folded - want).abs().max()) / mag
    print(f'\n[{arch}] feature error vs the fp32 oracle: plain chain {e_plain:.2e}, folded {e_fold:.2e}')
    assert e_fold < 1e-3 and e_fold < 1.5 * e_plain + 1e-4
    assert torch.equal(folded, every)


# per profiler class (gemm.hip groups the epilogues: STORE16 with STORE16_LN, GELU16 with GELU16_LN, RESID32 with RESID_HL;
# LayerNorm, the statistics kernels and ec_split16 share a class), 4 blocks, the last one on the class rows only:
#   STORE16   one QKV launch per full block, k | v + q in the last one
#   RESID32   out_proj and c_proj of every block + the lo half of the patch embedding;  STORE32: patch embedding, proj
#   layernorm plain: 2 per block + ln_post.  folded: ec_row_stats once, a merge behind every residual GEMM that a default
#             block follows (2 + 2 + 2 + 1), ln_post.  three split-operand blocks: 2 per block, one merge behind the
#             last of them, one in the default block, ln_post.  precise: 2 + ec_split16 per block, ln_post
_BLOCK_CHAIN_LAUNCHES = {'gemm_kernel<STORE16>': 5, 'gemm_kernel<GELU16>': 4, 'gemm_kernel<RESID32>': 9, 'gemm_kernel<STORE32>': 2,
                         'layernorm_kernel': 9, 'attention_kernel': 4, 'embed_kernel': 1}
_PRECISE_LAUNCHES = {'gemm_kernel<STORE16>': 4, 'gemm_kernel<RESID32>': 9, 'gemm_kernel<STORE32>': 6,
                     'layernorm_kernel': 13, 'attention_kernel': 4, 'embed_kernel': 1}


@pytest.mark.parametrize('kw,want', [
    (dict(), _BLOCK_CHAIN_LAUNCHES),
    (dict(ln_folded=False), _BLOCK_CHAIN_LAUNCHES),
    (dict(image_precise=True), _PRECISE_LAUNCHES),
    (dict(image_precise_blocks=3, image_precise_attn_blocks=2, image_lo_fp8=True), _BLOCK_CHAIN_LAUNCHES),
    (dict(image_precise_blocks=3, image_precise_attn_blocks=2, image_lo_fp8=False), _BLOCK_CHAIN_LAUNCHES),
], ids=['folded', 'plain', 'precise', 'split_lo8', 'split_lo16'])
def test_tower_launch_counts_by_mode(kw, want, hip):
    """The launches of one ec_vit_encode call (ViT-B/32 with 4 blocks, 3 images, one chunk) per profiler class are what
    the per-block launch lists in csrc/towers.hip say.  The numbers were recorded from the library before the block
    drivers were rewritten and checked by hand against those lists (the three block chains happen to agree per class)."""
    import torch
    from eventclip_amd import _lib
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config('ViT-B/32', layers=4, text_layers=1, vocab_size=1024)
    m = eclip.CLIP(cfg, eclip.random_state_dict(cfg, seed=3), **kw).cuda().eval()
    patches = torch.randn(3, 49, m.kpad, generator=torch.Generator().manual_seed(5)).half().cuda()
    m.encode_patches(patches)           # packs the weights, allocates the workspace
    torch.cuda.synchronize()
    _lib.profile_begin()
    feats = m.encode_patches(patches)
    torch.cuda.synchronize()
    got = {e['name']: e['launches'] for e in _lib.profile_end() if e['launches']}
    assert torch.isfinite(feats).all()
    assert got == want, (got, want)
