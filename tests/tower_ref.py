"""Yardsticks for the two host drivers of csrc/towers.hip (ec_vit_encode, ec_text_encode): the plain mathematical towers in
float64, the tables of tiny towers / chains / prompts that reach every branch of the drivers, and the harness that runs a
driver inside guarded buffers.  CPU only; tests/test_tower_ref_cpu.py checks everything here against a stand-in driver
with one fault injected at a time, tests/test_tower_drivers_gpu.py holds the HIP drivers to the same checks.

A *driver* is anything with the C ABI's calling convention,

    drv.need(chunk) -> workspace bytes          drv.embed -> feature width          drv.device
    drv.call(inp, n, feats, ws, ws_bytes, chunk) -> EC_OK or a negative EC_ERR_* code

over torch buffers: ``inp`` the patch rows [n, G, kpad] or the token ids [n, ctx], ``feats`` fp32, ``ws`` uint8.

Bounds (max-normalised, ``rel_err``) are the project's own and none is taken from the drivers under test:
1e-3 for f16 operands (north_star; tests/test_towers_gpu.py::test_image_tower_matches_oracle_fixture), 1e-2 for bf16
operands (same test), 2e-5 for the split-precision towers in f16 (test_text_tower_matches_oracle_fixture,
test_precise_image_tower_reproduces_fp32_oracle) and 1e-4 for the split-precision towers on bf16 parts, which carry 16
bits together (test_bf16_operands_reach_1e3_only_in_split_mode)."""
import functools
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import clip_ref  # noqa: E402

EC_OK, EC_ERR_INVALID, EC_ERR_WORKSPACE = 0, -1, -4

# ------------------------------------------------------------------------------------------------------------------
# the tiny towers: name -> (image, patch, width, layers, embed); S = (image / patch)^2 + 1
#   s5, s5_l1   one 16-query tile; the class-rows block as the second / the only block
#   s10         two heads, three blocks: room for two split-operand blocks in front of a default one
#   s50         ViT-B/32's sequence length
#   s257        a lone split query tile on 8 waves;  s325: K + V images beyond 80 KiB, 16 waves
# ------------------------------------------------------------------------------------------------------------------
TOWERS = {'s5': (8, 4, 64, 2, 16), 's5_l1': (8, 4, 64, 1, 16), 's10': (48, 16, 128, 3, 32), 's50': (224, 32, 64, 2, 16),
          's257': (256, 16, 64, 2, 16), 's325': (288, 16, 64, 2, 16)}
TEXT_TOWERS = {'t77_w64': (77, 64), 't77_w128': (77, 128), 't17_w64': (17, 64), 't17_w128': (17, 128)}
VOCAB, SOT, EOT = 96, 94, 95
# Weights: clip.random_state_dict(seed, qk_gain, branch_gain) per use.
#   'edges'     sharp, content-dependent attention and strong branches: the bit-for-bit tests (A, B, C2, C3)
#   'accuracy'  the plain init scales, as the full-size fixtures the bounds come from.  On the 'edges' weights the operand
#               rounding ALONE (emulate_image16 below, no kernel involved) puts a 16-bit chain at 0.6e-3 .. 2.4e-3 (f16) and
#               up to 2.3e-2 (bf16) on these towers, outside the 1e-3 / 1e-2 that full-width towers meet: 64 .. 128 columns
#               average nothing away and a gain of 3 per branch multiplies what is left.  At the plain scales it is
#               1.3e-4 .. 4.1e-4 / 1.3e-3 .. 3.0e-3 (seed 4, the best of seeds 0 .. 5, 7 and 8 over all six towers);
#               tests/test_tower_ref_cpu.py asserts that room.  Seeds and gains were chosen on that emulation alone.
WEIGHTS = {'edges': (7, 2.0, 3.0), 'accuracy': (4, 1.0, 1.0)}
# The text tower takes no gains.  At its init scales (token embedding 0.02, positions 0.01) the stream of a two-block tower
# is all branch output and the rounding-only chain sits at 0.6e-3 .. 1.4e-3 whatever the seed; with the embeddings at
# the size of the branch outputs (x 30) it is 3.4e-4 .. 5.2e-4, most of it the head's own 16-bit operands.  Seed per tower:
# the lowest emulated error of seeds 0 .. 11.
TEXT_EMBED_GAIN = 30.0
TEXT_SEEDS = {'t77_w64': 5, 't77_w128': 3, 't17_w64': 5, 't17_w128': 3}


def seq_len(tower):
    R, P = TOWERS[tower][:2]
    return (R // P) ** 2 + 1


def image_cfg(tower, activation='quick_gelu'):
    R, P, W, L, E = TOWERS[tower]
    return dict(image_size=R, patch=P, width=W, layers=L, embed_dim=E, text_width=64, text_heads=1, text_layers=1,
                context_length=77, vocab_size=VOCAB, activation=activation)


def text_cfg(tower, activation='quick_gelu'):
    ctx, W = TEXT_TOWERS[tower]
    return dict(image_size=8, patch=4, width=64, layers=1, embed_dim=16, text_width=W, text_heads=W // 64, text_layers=2,
                context_length=ctx, vocab_size=VOCAB, activation=activation)


# ------------------------------------------------------------------------------------------------------------------
# the chains: name -> dict(kw = CLIP(...) keywords, dtype, activation, w16 = weights rounded to 16 bit first,
#                          towers = where the chain can be built, bound)
# Split-operand blocks need 0 < precise_blocks < layers (two of them: the three blocks of s10) and the e4m3 lo products a
# width that is a multiple of 128 (s10).  A single block (s5_l1) runs the plain, folded and split-precision chains.
# ------------------------------------------------------------------------------------------------------------------
def _chain(kw, towers=('s5', 's10'), dtype='float16', activation='quick_gelu', w16=False, bound=None):
    if bound is None:
        precise = bool(kw.get('image_precise'))
        bound = {('float16', False): 1e-3, ('bfloat16', False): 1e-2, ('float16', True): 2e-5, ('bfloat16', True): 1e-4}[dtype, precise]
    return dict(kw=kw, towers=towers, dtype=dtype, activation=activation, w16=w16, bound=bound)


def _split(pb, pa, fp8=False):
    return dict(image_precise_blocks=pb, image_precise_attn_blocks=pa, image_lo_fp8=fp8)


_PLAIN, _PRECISE = dict(ln_folded=False), dict(image_precise=True)
_ALL3 = ('s5', 's5_l1', 's10')
CHAINS = {
    'plain': _chain(_PLAIN, _ALL3),
    'plain_q_unscaled': _chain(dict(ln_folded=False, q_scaled=False)),
    'folded': _chain({}, _ALL3),
    'folded_full_last_block': _chain(dict(full_last_block=True)),
    'folded_q_unscaled': _chain(dict(q_scaled=False)),
    'split_1_0': _chain(_split(1, 0)),
    'split_2_1': _chain(_split(2, 1), ('s10',)),
    'split_2_2': _chain(_split(2, 2), ('s10',)),
    'split_2_1_fp8': _chain(_split(2, 1, True), ('s10',)),
    'split_1_0_w16': _chain(_split(1, 0), w16=True),
    'split_2_1_w16': _chain(_split(2, 1), ('s10',), w16=True),
    'split_2_1_fp8_w16': _chain(_split(2, 1, True), ('s10',), w16=True),
    'precise': _chain(_PRECISE, _ALL3),
    'precise_w16': _chain(_PRECISE, w16=True),
    'low_latency': _chain(dict(low_latency=True)),
    'plain_gelu': _chain(_PLAIN, activation='gelu'),
    'folded_gelu': _chain({}, activation='gelu'),
    'precise_gelu': _chain(_PRECISE, activation='gelu'),
    'plain_bf16': _chain(_PLAIN, dtype='bfloat16'),
    'folded_bf16': _chain({}, dtype='bfloat16'),
    'precise_bf16': _chain(_PRECISE, dtype='bfloat16'),
}
# (tower, chain) pairs of the chain tests; (n, chunk) with a tail for the guarded runs -- on s10 the 260 rows of the first
# chunk cross a 256-row GEMM tile and the tail is one image -- and n for the chunk-invariance runs
CHAIN_CASES = [(t, c) for c, v in CHAINS.items() for t in v['towers']]
TAIL_CASE = {'s5': (7, 3), 's5_l1': (7, 3), 's10': (27, 26)}
TEXT_TAIL_CASE = (5, 2)
# name -> (text_precise, dtype, activation, bound)
TEXT_CHAINS = {'precise': (True, 'float16', 'quick_gelu', 2e-5), 'plain': (False, 'float16', 'quick_gelu', 1e-3),
               'precise_bf16': (True, 'bfloat16', 'quick_gelu', 1e-4), 'plain_bf16': (False, 'bfloat16', 'quick_gelu', 1e-2),
               'precise_gelu': (True, 'float16', 'gelu', 2e-5), 'plain_gelu': (False, 'float16', 'gelu', 1e-3)}
# QM_RAW (attention_exact_scale: the 16-bit attention of a split-operand block without fp32 attention) at its dispatch
# edges, with the default folded tower on the same weights as the control
QM_RAW_TOWERS = ('s50', 's257', 's325')


def chunks_for(n):
    """chunk in {1, 2, n - 1, n, n + 5}, without repeats and without values below 1"""
    return sorted({c for c in (1, 2, n - 1, n, n + 5) if c >= 1})


@functools.lru_cache(maxsize=None)
def state_dict(kind, tower, w16=False, use='edges'):
    """Seeded weights of a tiny tower (kind 'image' / 'text'; use: WEIGHTS above, image towers only); w16: every matrix
    rounded to fp16 first, as a checkpoint stored in 16 bit."""
    from eventclip_amd import clip as eclip
    if kind == 'image':
        seed, qk_gain, branch_gain = WEIGHTS[use]
        sd = eclip.random_state_dict(image_cfg(tower), seed=seed, qk_gain=qk_gain, branch_gain=branch_gain)
    else:
        sd = eclip.random_state_dict(text_cfg(tower), seed=TEXT_SEEDS[tower])
        sd['token_embedding.weight'] = sd['token_embedding.weight'] * TEXT_EMBED_GAIN
        sd['positional_embedding'] = sd['positional_embedding'] * TEXT_EMBED_GAIN
    if w16:
        sd = {k: (v.half().float() if v.dim() >= 2 else v) for k, v in sd.items()}
    return sd


def images(tower, n, seed):
    R = TOWERS[tower][0]
    return torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(1000 + seed))


# ------------------------------------------------------------------------------------------------------------------
# prompts: random ids in [1, 93] behind SOT = 94, the maximum id 95 at position p
# ------------------------------------------------------------------------------------------------------------------
EOT_POSITIONS = {77: (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 76), 17: (0, 15, 16)}


def first_max(tok):
    """index of the first maximum of every row (torch.argmax's documented tie rule is 'any')"""
    S = tok.shape[1]
    pos = torch.arange(S, device=tok.device).expand_as(tok)
    return torch.where(tok == tok.max(1, keepdim=True).values, pos, torch.full_like(pos, S)).min(1).values


def random_prompts(n, ctx, seed):
    """n prompts with the EOT at random positions 1 .. ctx - 1 (the guarded and chunked runs)"""
    g = torch.Generator().manual_seed(2000 + seed)
    tok = torch.randint(1, 94, (n, ctx), generator=g, dtype=torch.int32)
    tok[:, 0] = SOT
    p = torch.randint(1, ctx, (n,), generator=g)
    tok[torch.arange(n), p] = EOT
    return tok


def eot_prompts(ctx, seed=0):
    """-> (tok int32 [len(EOT_POSITIONS) + 3, ctx], names).  One prompt per position p of the first maximum, then:
    'tie': 95 at p and again at two later positions; 'other_max': a row whose maximum is 90, not 95; 'all_equal':
    every id the same (index 0)."""
    g = torch.Generator().manual_seed(3000 + seed + ctx)
    P = EOT_POSITIONS[ctx]
    tok = torch.randint(1, 94, (len(P) + 3, ctx), generator=g, dtype=torch.int32)
    tok[:, 0] = SOT
    names = []
    for i, p in enumerate(P):
        tok[i, p] = EOT
        names.append(f'p{p}')
    t0, t1, t2 = (5, 20, 40) if ctx == 77 else (3, 8, 16)
    tok[len(P), [t0, t1, t2]] = EOT
    tok[len(P) + 1] = torch.randint(1, 90, (ctx,), generator=g, dtype=torch.int32)
    tok[len(P) + 1, 7] = 90
    tok[len(P) + 2] = 7
    return tok, names + ['tie', 'other_max', 'all_equal']


def replace_suffix(tok, seed=1):
    """Every token behind the first maximum replaced by another id below that maximum (the first one by zero, as padding
    would be); everything up to and including the first maximum kept."""
    g = torch.Generator().manual_seed(4000 + seed)
    idx, top = first_max(tok), tok.max(1, keepdim=True).values
    other = (tok + torch.randint(1, 50, tok.shape, generator=g, dtype=torch.int32)) % top.clamp(min=1)   # in [0, max), != tok where max > 50
    behind = torch.arange(tok.shape[1])[None, :] > idx[:, None]
    out = torch.where(behind, other.to(tok.dtype), tok)
    first_behind = torch.arange(tok.shape[1])[None, :] == idx[:, None] + 1
    return torch.where(first_behind, torch.zeros_like(out), out)


# ------------------------------------------------------------------------------------------------------------------
# the towers in float64
# ------------------------------------------------------------------------------------------------------------------
def activation64(x, name):
    if name in (None, 'quick_gelu'):
        return x * torch.sigmoid(1.702 * x)
    if name == 'gelu':
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))
    raise ValueError(name)


def blocks64(x, sd, prefix, layers, heads, activation, mask=None):
    """oracle/clip_ref._blocks with the activation switch (float64 leaves)"""
    W = x.shape[-1]
    for i in range(layers):
        p = f'{prefix}.resblocks.{i}.'
        h = F.layer_norm(x, (W,), sd[p + 'ln_1.weight'], sd[p + 'ln_1.bias'], 1e-5)
        x = x + clip_ref._mha(h, sd[p + 'attn.in_proj_weight'], sd[p + 'attn.in_proj_bias'],
                              sd[p + 'attn.out_proj.weight'], sd[p + 'attn.out_proj.bias'], heads, mask)
        h = F.layer_norm(x, (W,), sd[p + 'ln_2.weight'], sd[p + 'ln_2.bias'], 1e-5)
        h = activation64(F.linear(h, sd[p + 'mlp.c_fc.weight'], sd[p + 'mlp.c_fc.bias']), activation)
        x = x + F.linear(h, sd[p + 'mlp.c_proj.weight'], sd[p + 'mlp.c_proj.bias'])
    return x


def _double(sd):
    return {k: v.double() for k, v in sd.items()}


@torch.no_grad()
def encode_image64(sd, cfg, img):
    """image [N, 3, R, R] -> float64 [N, embed_dim]: conv1, class token, positions, ln_pre, the blocks, ln_post(x[:, 0]) @ proj"""
    sd = _double(sd)
    W, P = cfg['width'], cfg['patch']
    x = F.conv2d(img.double(), sd['visual.conv1.weight'], stride=P)
    x = x.reshape(x.shape[0], W, -1).permute(0, 2, 1)
    x = torch.cat([sd['visual.class_embedding'].expand(x.shape[0], 1, W), x], dim=1) + sd['visual.positional_embedding']
    x = F.layer_norm(x, (W,), sd['visual.ln_pre.weight'], sd['visual.ln_pre.bias'], 1e-5)
    x = blocks64(x, sd, 'visual.transformer', cfg['layers'], W // 64, cfg.get('activation'))
    x = F.layer_norm(x[:, 0, :], (W,), sd['visual.ln_post.weight'], sd['visual.ln_post.bias'], 1e-5)
    return x @ sd['visual.proj']


def causal_mask(ctx, diagonal=1):
    return torch.full((ctx, ctx), float('-inf'), dtype=torch.float64).triu_(diagonal)


def text_stream64(sd64, cfg, tok, diagonal=1):
    """token ids [n, ctx] -> the residual stream behind the last block, float64 [n, ctx, W]"""
    x = sd64['token_embedding.weight'][tok.long()] + sd64['positional_embedding']
    return blocks64(x, sd64, 'transformer', cfg['text_layers'], cfg['text_heads'], cfg.get('activation'),
                    causal_mask(cfg['context_length'], diagonal))


def text_head64(sd64, rows):
    W = rows.shape[-1]
    return F.layer_norm(rows, (W,), sd64['ln_final.weight'], sd64['ln_final.bias'], 1e-5) @ sd64['text_projection']


@torch.no_grad()
def encode_text64(sd, cfg, tok):
    """token ids [n, ctx] -> float64 [n, embed_dim]: -inf causal mask, the row of the FIRST maximum of the raw ids"""
    sd = _double(sd)
    x = text_stream64(sd, cfg, tok)
    return text_head64(sd, x[torch.arange(x.shape[0]), first_max(tok.long())])


# ------------------------------------------------------------------------------------------------------------------
# The operand rounding alone: the float64 towers with every matrix rounded to 16 bit (clip_ref.round_weights) and every
# GEMM input rounded to 16 bit where the 16-bit chains hold it in 16 bit -- LayerNorm's output, q | k | v, attention's
# output, the MLP activation.  Everything else exact: no fp32 accumulation, no rounding of the softmax weights, the
# residual stream, the patch embedding and the image head unrounded (the chains keep those as fp32 or hi + lo parts).
# What a CORRECT 16-bit chain cannot do better than, whatever its kernels: the yardstick that says whether a tiny
# tower with given weights can meet a bound at all.
#   folded=True: the folded-LayerNorm form of the image tower -- the raw stream rounded to 16 bit (the hi plane), its
#   statistics taken from the rounded rows, the gain folded into the matrix before ITS rounding.
# ------------------------------------------------------------------------------------------------------------------
def _r16(x, dt):
    return x.to(dt).double()


def _emulated_blocks(x, sd, prefix, layers, heads, activation, dt, mask=None, folded=False):
    W = x.shape[-1]

    def ln_linear(x, p, ln, lin):
        g, b = sd[p + ln + '.weight'], sd[p + ln + '.bias']
        w, bias = sd[p + lin + ('_weight' if lin.endswith('in_proj') else '.weight')], sd[p + lin + ('_bias' if lin.endswith('in_proj') else '.bias')]
        if not folded:
            return F.linear(_r16(F.layer_norm(x, (W,), g, b, 1e-5), dt), _r16(w, dt), bias)
        xh = _r16(x, dt)
        return F.linear(F.layer_norm(xh, (W,), None, None, 1e-5), _r16(w * g[None, :], dt), bias + w @ b)

    for i in range(layers):
        p = f'{prefix}.resblocks.{i}.'
        qkv = _r16(ln_linear(x, p, 'ln_1', 'attn.in_proj'), dt)
        N, S, _ = qkv.shape
        q, k, v = (t.view(N, S, heads, 64).transpose(1, 2) for t in qkv.split(W, dim=-1))
        att = (q * 0.125) @ k.transpose(-1, -2)
        if mask is not None:
            att = att + mask
        out = _r16((att.softmax(-1) @ v).transpose(1, 2).reshape(N, S, W), dt)
        x = x + F.linear(out, _r16(sd[p + 'attn.out_proj.weight'], dt), sd[p + 'attn.out_proj.bias'])
        h = _r16(activation64(ln_linear(x, p, 'ln_2', 'mlp.c_fc'), activation), dt)
        x = x + F.linear(h, _r16(sd[p + 'mlp.c_proj.weight'], dt), sd[p + 'mlp.c_proj.bias'])
    return x


@torch.no_grad()
def emulate_image16(sd, cfg, img, dtype=torch.float16, folded=False):
    sd = _double(sd)
    W, P = cfg['width'], cfg['patch']
    x = F.conv2d(img.double(), sd['visual.conv1.weight'], stride=P)
    x = x.reshape(x.shape[0], W, -1).permute(0, 2, 1)
    x = torch.cat([sd['visual.class_embedding'].expand(x.shape[0], 1, W), x], dim=1) + sd['visual.positional_embedding']
    x = F.layer_norm(x, (W,), sd['visual.ln_pre.weight'], sd['visual.ln_pre.bias'], 1e-5)
    x = _emulated_blocks(x, sd, 'visual.transformer', cfg['layers'], W // 64, cfg.get('activation'), dtype, folded=folded)
    x = F.layer_norm(x[:, 0, :], (W,), sd['visual.ln_post.weight'], sd['visual.ln_post.bias'], 1e-5)
    return x @ sd['visual.proj']


@torch.no_grad()
def emulate_text16(sd, cfg, tok, dtype=torch.float16):
    """the plain text chain: its head too runs on 16-bit operands (ln_final's output and text_projection)"""
    sd = _double(sd)
    x = sd['token_embedding.weight'][tok.long()] + sd['positional_embedding']
    x = _emulated_blocks(x, sd, 'transformer', cfg['text_layers'], cfg['text_heads'], cfg.get('activation'), dtype,
                         causal_mask(cfg['context_length']))
    rows = x[torch.arange(x.shape[0]), first_max(tok.long())]
    W = rows.shape[-1]
    h = _r16(F.layer_norm(rows, (W,), sd['ln_final.weight'], sd['ln_final.bias'], 1e-5), dtype)
    return h @ _r16(sd['text_projection'], dtype)


# ------------------------------------------------------------------------------------------------------------------
# comparisons
# ------------------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    """as tests/test_towers_gpu.py: the largest difference over the largest reference value"""
    return float((a - b).abs().max() / b.abs().max())


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same_bits(a, b, what=''):
    """a and b hold the same bytes (NaNs compare by their bits); reports the first element that differs"""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ne = _bits(a) != _bits(b)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        raise AssertionError(f'{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at flat index {i}: '
                             f'{a.flatten()[i].item()!r} != {b.flatten()[i].item()!r}')


def assert_accuracy(got, want, bound, what=''):
    assert bool(torch.isfinite(got).all()), f'{what}: features are not finite'
    err = rel_err(got.double().cpu(), want)
    assert err < bound, f'{what}: {err:.3e} of the largest feature, bound {bound:g}'
    return err


# ------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ------------------------------------------------------------------------------------------------------------------
GUARD_BYTES = 1 << 20
GUARD_ROWS = 4
FILLS = (0x00, 0xFF)        # 0xFF: NaN as f16, bf16 and fp32, -1 as int


@functools.lru_cache(maxsize=None)
def _guard_pattern(nbytes, device):
    g = torch.Generator().manual_seed(99)
    return torch.randint(1, 255, (nbytes,), generator=g, dtype=torch.uint8).to(device)


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


def run_guarded(drv, inp, n, chunk, fill=0xFF, short=0):
    """One call of the driver on n inputs inside guarded buffers -> (rc, feats [n, embed] fp32, the workspace's first
    ``need`` bytes as the call left them).

    The workspace is ``need = drv.need(min(chunk, n))`` bytes holding ``fill`` (a byte value, or a uint8 tensor: what an
    earlier call left) followed by GUARD_BYTES of a fixed pattern; the driver is told ``need - short`` bytes.  feats is n
    rows of 0xFF bytes (NaN: a row the call did not write is not finite) followed by GUARD_ROWS rows of the pattern.
    Asserts that both guards and the input come back bit for bit, and, when the call is refused, that workspace and
    feats still hold their fill: nothing was written before the refusal."""
    dev, E = drv.device, drv.embed
    need = drv.need(max(1, min(chunk, n)))
    assert need > 0
    ws = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=dev)
    if isinstance(fill, torch.Tensor):
        assert fill.numel() >= need, 'the earlier call left fewer bytes than this one needs'
        ws[:need] = fill[:need].to(dev)
    else:
        ws[:need] = fill
    ws[need:] = _guard_pattern(GUARD_BYTES, str(dev))
    before = ws[:need].clone()
    feats = torch.empty((n + GUARD_ROWS) * E, dtype=torch.float32, device=dev)
    _bits(feats).view(torch.uint8)[:n * E * 4] = 0xFF
    _bits(feats).view(torch.uint8)[n * E * 4:] = _guard_pattern(GUARD_ROWS * E * 4, str(dev))
    kept = inp.clone()
    rc = drv.call(inp, n, feats, ws, need - short, chunk)
    _sync(dev)
    what = f'n={n} chunk={chunk} fill={fill if isinstance(fill, int) else "stale"}'
    assert_same_bits(ws[need:], _guard_pattern(GUARD_BYTES, str(dev)), f'bytes behind the workspace ({what})')
    assert_same_bits(_bits(feats).view(torch.uint8)[n * E * 4:], _guard_pattern(GUARD_ROWS * E * 4, str(dev)),
                     f'feature rows behind row n ({what})')
    assert_same_bits(inp, kept, f'the input buffer ({what})')
    if rc != EC_OK:
        assert_same_bits(ws[:need], before, f'workspace of a refused call ({what})')
        assert bool((_bits(feats).view(torch.uint8)[:n * E * 4] == 0xFF).all()), f'feats of a refused call ({what})'
    return rc, feats[:n * E].view(n, E).clone(), ws[:need].clone()


def encode(drv, inp, n, chunk, fill=0xFF):
    """a guarded call that must succeed and leave n finite rows -> feats"""
    rc, feats, _ = run_guarded(drv, inp, n, chunk, fill)
    assert rc == EC_OK, f'n={n} chunk={chunk}: refused with {rc}'
    assert bool(torch.isfinite(feats).all()), f'n={n} chunk={chunk}: features are not finite'
    return feats


def check_workspace_independence(drv, inp, n, chunk, earlier_inp):
    """A: the same call on a workspace of 0x00, of 0xFF and of what a call on more and different inputs (``earlier_inp``,
    same chunk, so the same workspace size) left behind -> bit-identical finite features, guards and inputs intact."""
    assert earlier_inp.shape[0] > n
    rc, _, stale = run_guarded(drv, earlier_inp, earlier_inp.shape[0], chunk, 0x00)
    assert rc == EC_OK, rc
    outs = [encode(drv, inp, n, chunk, fill) for fill in FILLS + (stale,)]
    assert_same_bits(outs[1], outs[0], f'features on a workspace of 0xFF against one of 0x00 (n={n}, chunk={chunk})')
    assert_same_bits(outs[2], outs[0], f'features on a used workspace against one of 0x00 (n={n}, chunk={chunk})')
    return outs[0]


def check_refusals(drv, inp, n, chunk, feats_ok):
    """A: need - 1 bytes -> EC_ERR_WORKSPACE with nothing written; n = 0 -> EC_OK on null buffers; chunk <= 0 refused;
    chunk > n behaves as chunk = n."""
    for fill in FILLS:
        rc, _, _ = run_guarded(drv, inp, n, chunk, fill, short=1)
        assert rc == EC_ERR_WORKSPACE, f'a workspace one byte short: rc {rc}'
    assert drv.call(None, 0, None, None, 0, chunk) == EC_OK, 'n = 0 with null buffers'
    for bad in (0, -1):
        rc, _, _ = run_guarded(drv, inp, n, bad)
        assert rc == EC_ERR_INVALID, f'chunk = {bad}: rc {rc}'
    whole = encode(drv, inp, n, n)
    assert_same_bits(encode(drv, inp, n, n + 3), whole, f'chunk = n + 3 against chunk = n (n={n})')
    assert_same_bits(feats_ok, whole, f'chunk = {chunk} against chunk = n (n={n})')


def check_chunk_invariance(drv, inp, n, chunks=None):
    """B: every chunk size gives the features of chunk = n, bit for bit -> those features"""
    whole = encode(drv, inp, n, n)
    for c in chunks or chunks_for(n):
        if c != n:
            assert_same_bits(encode(drv, inp, n, c), whole, f'chunk = {c} against chunk = n = {n}')
    return whole


def check_suffix_independence(drv, tok, chunk=None):
    """C2: replacing every token behind the first maximum leaves the features bit-identical -> those features"""
    n = tok.shape[0]
    alt = replace_suffix(tok.cpu()).to(tok.device)
    assert bool((first_max(alt.cpu()) == first_max(tok.cpu())).all())
    behind = torch.arange(tok.shape[1])[None, :] > first_max(tok.cpu())[:, None]
    assert bool((alt.cpu() != tok.cpu())[behind].float().mean() > 0.9), 'the replaced suffix is the old one'
    a, b = encode(drv, tok, n, chunk or n), encode(drv, alt, n, chunk or n)
    assert_same_bits(b, a, 'features with the tokens behind the first maximum replaced')
    return a


# ------------------------------------------------------------------------------------------------------------------
# a stand-in driver in plain torch (CPU, float64), with ec_text_encode's calling convention and one optional fault
# ------------------------------------------------------------------------------------------------------------------
FAULTS = ('stale_read', 'workspace_overrun', 'feats_overrun', 'last_max', 'mask_off_by_one', 'tail_offsets', 'eot_not_rebased')


class StandInTextDriver:
    """Encodes like encode_text64, but the way the HIP driver does: in chunks, with the residual stream (as a hi plane
    and a lo plane, the lo plane behind the hi plane of THIS chunk's rows) and the EOT indices kept in the caller's
    workspace.  ``fault`` breaks one thing:

      stale_read         the last EOT index of a chunk is read without having been written
      workspace_overrun  one byte written behind the workspace
      feats_overrun      a feature row written behind row n
      last_max           the EOT row is the last maximum
      mask_off_by_one    every query sees one key too many
      tail_offsets       the lo plane is written at the offset of a full chunk and read at the offset of this chunk's rows
      eot_not_rebased    the EOT index counts rows from the first prompt of the call, not of the chunk"""
    device = torch.device('cpu')

    def __init__(self, sd, cfg, fault=None):
        assert fault is None or fault in FAULTS
        self.sd, self.cfg, self.fault = _double(sd), cfg, fault
        self.S, self.W, self.embed = cfg['context_length'], cfg['text_width'], cfg['embed_dim']

    def need(self, chunk):
        return (2 * chunk * self.S * self.W + chunk) * 8 if chunk > 0 else 0

    @torch.no_grad()
    def call(self, tok, n, feats, ws, ws_bytes, chunk):
        S, W, E, fault = self.S, self.W, self.embed, self.fault
        if n < 0 or chunk <= 0:
            return EC_ERR_INVALID
        if n == 0:
            return EC_OK
        chunk = min(chunk, n)
        need = self.need(chunk)
        if ws_bytes < need:
            return EC_ERR_WORKSPACE
        f64, i64 = ws[:ws.numel() // 8 * 8].view(torch.float64), ws[:ws.numel() // 8 * 8].view(torch.int64)
        idx_at = 2 * chunk * S * W
        out = feats.view(-1, E)
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            t = tok[i0:i0 + m]
            # one prompt at a time: a prompt's arithmetic does not depend on how many share its chunk
            x = torch.cat([text_stream64(self.sd, self.cfg, t[r:r + 1], 2 if fault == 'mask_off_by_one' else 1) for r in range(m)])
            hi = x.float().double()
            rows = m * S * W
            f64[:rows] = hi.flatten()
            lo_written = chunk * S * W if fault == 'tail_offsets' else rows
            f64[lo_written:lo_written + rows] = (x - hi).flatten()
            best = (S - 1 - first_max(t.long().flip(1))) if fault == 'last_max' else first_max(t.long())
            base = i0 if fault == 'eot_not_rebased' else 0
            held = m - 1 if fault == 'stale_read' else m
            i64[idx_at:idx_at + held] = ((base + torch.arange(m)) * S + best)[:held]
            at = (i64[idx_at:idx_at + m, None] * W + torch.arange(W)[None, :]) % idx_at     # (a wild index stays inside the planes)
            eot = f64[at] + f64[(at + rows) % idx_at]
            out[i0:i0 + m] = text_head64(self.sd, eot).float()
        if fault == 'workspace_overrun':
            ws[need] ^= 0xFF
        if fault == 'feats_overrun':
            out[n] = out[n - 1]
        return EC_OK
