"""The two host drivers of csrc/towers.hip, ec_vit_encode and ec_text_encode, called through the C ABI on the test's own
guarded buffers, on tiny towers that reach every chain, chunk and EOT edge (tables, float64 towers and the harness:
tests/tower_ref.py; the harness itself is checked against a faulty stand-in driver in tests/test_tower_ref_cpu.py).

  A  guards and refusals: nothing is written outside ec_*_workspace_bytes or behind feats row n, inputs come back
     untouched, a short workspace is refused before anything is written, and the features do not depend on what the
     workspace held before (0x00, 0xFF = NaN / -1, the leftovers of a larger call): no buffer is read before it is written
  B  chunk invariance, bit for bit, down to chunk = 1: an image's or prompt's features do not depend on its neighbours
  C  the text tower's EOT row (first maximum; positions 0, 76 and both sides of every 16- / 32-row tile edge; ties) and
     its causal mask (suffix independence, bit for bit), in one chunk and across chunks
  D  every chain against the float64 tower, and QM_RAW attention (a split-operand block without fp32 attention) at
     S = 50, on a lone split tile (S = 257) and on 16 waves (S = 325), the default folded tower as the control

A, B, C2 and C3 run on sharp weights (qk_gain 2, branch_gain 3); the comparisons with a bound run on the plain init scales,
because on these narrow towers the operand rounding alone puts a 16-bit chain outside its bound on the sharp ones
(tower_ref.WEIGHTS; tests/test_tower_ref_cpu.py asserts the room that the rounding leaves on the weights used here).

Measured on the MI355X, rel_err against float64 (every D / C1 test prints its figure; n = 3 images, 2 on the QM_RAW towers):
  image, f16 16-bit chains   1.1e-4 .. 4.8e-4 of 1e-3  (worst: s5 folded; plain 2.1e-4 .. 3.4e-4, split-operand 1.1e-4 .. 2.9e-4,
                             exact GELU 2.3e-4 .. 4.0e-4, low_latency 2.2e-4 .. 3.1e-4)
  image, bf16                1.7e-3 .. 4.1e-3 of 1e-2  (worst: s5 folded_bf16)
  image, split-precision     1.8e-7 .. 4.6e-7 of 2e-5; on bf16 parts 4.6e-6 .. 8.3e-6 of 1e-4
  QM_RAW (1, 0) / control    s50 2.5e-4 / 3.4e-4, s257 1.0e-4 / 2.3e-4, s325 2.4e-4 / 2.1e-4
  low_latency vs plain       s5 1.3e-7, s10 2.0e-4 (n = 27, every chunk size) and 3.2e-5 (n = 1), of 3e-4
  text, plain                3.4e-4 .. 5.6e-4 of 1e-3; bf16 3.5e-3 .. 4.2e-3 of 1e-2
  text, split-precision      2.6e-7 .. 5.4e-7 of 2e-5; on bf16 parts 5.8e-6 .. 7.2e-6 of 1e-4"""
import ctypes
import functools
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

_BASE_KW = dict(full_last_block=False, ln_folded=True, q_scaled=True, image_precise=False, low_latency=False,
                image_precise_blocks=0, image_precise_attn_blocks=0, image_lo_fp8=False)


class HipDriver:
    """ec_vit_encode / ec_text_encode behind tower_ref's driver convention, over the packed weights of a CLIP model"""
    device = torch.device('cuda')

    def __init__(self, model, kind):
        from eventclip_amd import _lib
        self.model, self.kind = model, kind
        self.w = model._pack()['vit' if kind == 'image' else 'text']
        self.entry = 'ec_vit_encode' if kind == 'image' else 'ec_text_encode'
        self.sizer = getattr(_lib.lib(), 'ec_vit_workspace_bytes' if kind == 'image' else 'ec_text_workspace_bytes')
        self.embed = model.cfg['embed_dim']

    def need(self, chunk):
        return int(self.sizer(ctypes.byref(self.w), chunk))

    def call(self, inp, n, feats, ws, ws_bytes, chunk):
        from eventclip_amd import _lib
        try:
            _lib.launch(self.entry, self.w, inp, n, feats, ws, ws_bytes, chunk)
        except RuntimeError as e:
            return int(re.search(r'failed \((-?\d+)\)', str(e)).group(1))
        return ref.EC_OK


@functools.lru_cache(maxsize=None)
def _image_driver(tower, chain, use='edges'):
    from eventclip_amd import clip as eclip
    c = ref.CHAINS[chain]
    cfg = ref.image_cfg(tower, c['activation'])
    kw = dict(_BASE_KW, **c['kw'])
    model = eclip.CLIP(cfg, ref.state_dict('image', tower, c['w16'], use), dtype=c['dtype'], text_precise=False, **kw).cuda().eval()
    v = model._pack()['vit']
    # the packed struct says what the chain's name says
    assert (v.precise, v.ln_folded, v.low_latency, v.full_last_block) == \
        (int(kw['image_precise']), int(kw['ln_folded'] and not kw['image_precise']), int(kw['low_latency']), int(kw['full_last_block']))
    assert (v.precise_blocks, v.precise_attn_blocks, v.lo_fp8) == \
        (kw['image_precise_blocks'], kw['image_precise_attn_blocks'], int(kw['image_lo_fp8']))
    assert v.q_scaled == int(kw['q_scaled'] and not kw['image_precise']) and v.weights_exact16 == int(c['w16'])
    assert v.layers == ref.TOWERS[tower][3] and v.heads * 64 == v.width == ref.TOWERS[tower][2]
    return HipDriver(model, 'image')


@functools.lru_cache(maxsize=None)
def _text_driver(tower, chain):
    from eventclip_amd import clip as eclip
    precise, dtype, activation, _ = ref.TEXT_CHAINS[chain]
    cfg = ref.text_cfg(tower, activation)
    model = eclip.CLIP(cfg, ref.state_dict('text', tower), dtype=dtype, text_precise=precise, **_BASE_KW).cuda().eval()
    t = model._pack()['text']
    assert (t.precise, t.ctx, t.width, t.heads, t.layers, t.vocab) == (int(precise), *ref.TEXT_TOWERS[tower], cfg['text_heads'], 2, ref.VOCAB)
    return HipDriver(model, 'text')


@functools.lru_cache(maxsize=None)
def _patches(tower, dtype, n, seed):
    """the patch rows of ref.images(tower, n, seed), as encode_image makes them (ec_patchify)"""
    from eventclip_amd import _lib
    from eventclip_amd.clip_base import patch_row_widths
    R, P = ref.TOWERS[tower][:2]
    kpad = patch_row_widths(P)[1]
    img = ref.images(tower, n, seed).cuda()
    out = torch.empty((n, (R // P) ** 2, kpad), dtype=getattr(torch, dtype), device='cuda')
    _lib.launch('ec_patchify', img, n, R, P, kpad, out, _lib.EC_F16 if dtype == 'float16' else _lib.EC_BF16)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _image_want(tower, activation, w16, n, seed):
    return ref.encode_image64(ref.state_dict('image', tower, w16, 'accuracy'), ref.image_cfg(tower, activation), ref.images(tower, n, seed))


@functools.lru_cache(maxsize=None)
def _text_want(tower, activation):
    cfg = ref.text_cfg(tower, activation)
    return ref.encode_text64(ref.state_dict('text', tower), cfg, ref.eot_prompts(cfg['context_length'])[0])


def _prompts(tower, n, seed):
    return ref.random_prompts(n, ref.TEXT_TOWERS[tower][0], seed).cuda()


_TEXT_CASES = [(t, c) for t in ref.TEXT_TOWERS for c in ref.TEXT_CHAINS]


# ---- A: guards, refusals, independence from the workspace's contents ----
@pytest.mark.parametrize('tower,chain', ref.CHAIN_CASES)
def test_image_driver_stays_in_its_buffers_and_reads_nothing_stale(tower, chain, hip):
    """(n, chunk) with a tail -- (7, 3); on s10 (27, 26): 260 rows cross a 256-row GEMM tile inside the first chunk and the
    tail is one image, n = 1 in the class-rows view -- on workspaces of 0x00, of 0xFF and of a larger call's leftovers."""
    drv, dtype = _image_driver(tower, chain), ref.CHAINS[chain]['dtype']
    n, chunk = ref.TAIL_CASE[tower]
    inp = _patches(tower, dtype, n, 1)
    feats = ref.check_workspace_independence(drv, inp, n, chunk, _patches(tower, dtype, n + 2, 2))
    if chain == 'low_latency':      # K-batched by the tile count: chunks may differ in the last bits (B holds it to the plain chain)
        feats = ref.encode(drv, inp, n, n)
    ref.check_refusals(drv, inp, n, chunk, feats)


@pytest.mark.parametrize('tower,chain', _TEXT_CASES)
def test_text_driver_stays_in_its_buffers_and_reads_nothing_stale(tower, chain, hip):
    drv = _text_driver(tower, chain)
    n, chunk = ref.TEXT_TAIL_CASE
    inp = _prompts(tower, n, 1)
    feats = ref.check_workspace_independence(drv, inp, n, chunk, _prompts(tower, n + 2, 2))
    ref.check_refusals(drv, inp, n, chunk, feats)


# ---- B: chunk invariance ----
@pytest.mark.parametrize('tower,chain', [c for c in ref.CHAIN_CASES if c[1] != 'low_latency'])
def test_image_features_do_not_depend_on_the_chunk(tower, chain, hip):
    """chunk in {1, 2, n - 1, n + 5} against chunk = n, bit for bit, for n = 7 (s10: 27) and n = 1"""
    drv, dtype = _image_driver(tower, chain), ref.CHAINS[chain]['dtype']
    for n in (ref.TAIL_CASE[tower][0], 1):
        ref.check_chunk_invariance(drv, _patches(tower, dtype, n, 3), n)


@pytest.mark.parametrize('tower', ['s5', 's10'])
def test_low_latency_chunks_stay_with_the_plain_chain(tower, hip):
    """low_latency cuts K by the tile count (kbatch_splits), so its features may depend on the rows of a chunk: every
    chunk size stays within 3e-4 of the largest feature of the plain chain (test_low_latency_mode_gives_the_same_features)."""
    fast, plain = _image_driver(tower, 'low_latency', 'accuracy'), _image_driver(tower, 'plain', 'accuracy')
    worst = {}
    for n in (ref.TAIL_CASE[tower][0], 1):
        inp = _patches(tower, 'float16', n, 3)
        base = ref.encode(plain, inp, n, n)
        for chunk in ref.chunks_for(n):
            got = ref.encode(fast, inp, n, chunk)
            worst[n, chunk] = float((got - base).abs().max() / base.abs().max())
    print(f'\n[{tower} low_latency against the plain chain] ' + ', '.join(f'n={n} chunk={c}: {d:.2e}' for (n, c), d in worst.items()), end='')
    assert max(worst.values()) < 3e-4, worst


@pytest.mark.parametrize('tower,chain', _TEXT_CASES)
def test_text_features_do_not_depend_on_the_chunk(tower, chain, hip):
    drv = _text_driver(tower, chain)
    for n in (5, 1):
        ref.check_chunk_invariance(drv, _prompts(tower, n, 3), n)


# ---- C: the EOT row and the causal mask ----
@pytest.mark.parametrize('tower,chain', _TEXT_CASES)
def test_text_tower_at_every_eot_edge_against_float64(tower, chain, hip):
    """The first maximum at position 0 (a causal row with one key), at the last position, on both sides of every 16- and
    32-row attention tile edge, repeated twice later (tie), a maximum that is not the EOT id, and an all-equal row."""
    drv, (_, _, activation, bound) = _text_driver(tower, chain), ref.TEXT_CHAINS[chain]
    tok, names = ref.eot_prompts(ref.TEXT_TOWERS[tower][0])
    got = ref.encode(drv, tok.cuda(), len(tok), len(tok)).double().cpu()
    want = _text_want(tower, activation)
    per_row = (got - want).abs().amax(1) / want.abs().max()
    worst = int(per_row.argmax())
    print(f'\n[{tower} text {chain}] {float(per_row.max()):.2e} (worst prompt: {names[worst]}), bound {bound:g}', end='')
    ref.assert_accuracy(got, want, bound, f'{tower} {chain}')


@pytest.mark.parametrize('tower,chain', _TEXT_CASES)
def test_text_features_do_not_depend_on_tokens_behind_the_eot(tower, chain, hip):
    drv = _text_driver(tower, chain)
    tok, _ = ref.eot_prompts(ref.TEXT_TOWERS[tower][0])
    ref.check_suffix_independence(drv, tok.cuda())


@pytest.mark.parametrize('tower,chain', _TEXT_CASES)
def test_text_chunks_carry_their_own_eot_rows(tower, chain, hip):
    """One call of up to 14 prompts in chunks of 4 (tail 2): every chunk has other EOT rows, the tail's tokens, features
    and indices are offset by its first prompt."""
    drv = _text_driver(tower, chain)
    tok, _ = ref.eot_prompts(ref.TEXT_TOWERS[tower][0])
    n = min(14, len(tok))
    assert n % 4 == 2
    ref.check_chunk_invariance(drv, tok[:n].contiguous().cuda(), n, chunks=(4,))


# ---- D: accuracy ----
def _image_accuracy(tower, chain, n):
    c = ref.CHAINS[chain]
    got = ref.encode(_image_driver(tower, chain, 'accuracy'), _patches(tower, c['dtype'], n, 5), n, n).double().cpu()
    want = _image_want(tower, c['activation'], c['w16'], n, 5)
    err = ref.rel_err(got, want)
    print(f'\n[{tower} {chain}] {err:.2e}, bound {c["bound"]:g}', end='')
    return err, c['bound']


@pytest.mark.parametrize('tower,chain', ref.CHAIN_CASES)
def test_image_chain_against_float64(tower, chain, hip):
    err, bound = _image_accuracy(tower, chain, 3)
    assert err < bound, (tower, chain, err)


@pytest.mark.parametrize('tower', ref.QM_RAW_TOWERS)
def test_raw_q_attention_at_its_dispatch_edges(tower, hip):
    """The (1, 0) split-operand tower is the only route to attention_exact_scale (QM_RAW); the default folded tower on the
    same weights and images is the control: where it meets the bound and the (1, 0) tower does not, the attention route
    is the suspect."""
    control, bound = _image_accuracy(tower, 'folded', 2)
    err, _ = _image_accuracy(tower, 'split_1_0', 2)
    assert control < bound, ('the control misses the bound', tower, control)
    assert err < bound, ('the split-operand tower misses the bound that the folded tower meets', tower, err, control)
