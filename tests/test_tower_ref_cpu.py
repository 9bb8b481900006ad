"""The yardsticks of tests/tower_ref.py, checked on the CPU: the float64 towers agree with oracle/clip_ref (fp32) to fp32
accuracy, the relations the GPU tests assert bit for bit hold exactly in the reference, the case tables hold the towers,
chains and prompts they promise, the bounds can be met on the weights used, and the harness passes a correct stand-in driver (plain torch, the HIP
driver's calling convention) and catches it with one fault injected at a time -- each by the check written for it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_ref as ref  # noqa: E402
from oracle import clip_ref  # noqa: E402

# "fp32 accuracy" as the project states it for a tower: the 2e-5 that the split-precision towers are held to against the
# fp32 oracle (tests/test_towers_gpu.py).  An fp32 dot product of K terms is off by about sqrt(K) 6e-8 of its operands'
# size -- 3e-6 for the 3072 terms of a 32-pixel patch -- and the sharpened attention (qk_gain) multiplies score errors.
FP32_BOUND = 2e-5


@pytest.mark.parametrize('tower', ['s5', 's5_l1', 's10', 's50'])
def test_image_tower64_agrees_with_the_fp32_oracle(tower):
    cfg, sd = ref.image_cfg(tower), ref.state_dict('image', tower)
    img = ref.images(tower, 3, 0)
    want = ref.encode_image64(sd, cfg, img)
    assert want.dtype == torch.float64 and want.shape == (3, cfg['embed_dim'])
    assert ref.rel_err(clip_ref.encode_image(sd, cfg, img).double(), want) < FP32_BOUND
    # the input carries signal: the features of two images differ by far more than any bound below
    assert float((want[0] - want[1]).abs().max() / want.abs().max()) > 0.02


@pytest.mark.parametrize('tower', list(ref.TEXT_TOWERS))
def test_text_tower64_agrees_with_the_fp32_oracle(tower):
    cfg, sd = ref.text_cfg(tower), ref.state_dict('text', tower)
    tok = ref.random_prompts(5, cfg['context_length'], 0)        # no ties: torch.argmax is unambiguous
    want = ref.encode_text64(sd, cfg, tok)
    assert ref.rel_err(clip_ref.encode_text(sd, cfg, tok).double(), want) < FP32_BOUND
    assert float((want[0] - want[1]).abs().max() / want.abs().max()) > 0.02


def test_exact_gelu_switch():
    x = torch.linspace(-9, 9, 4001, dtype=torch.float64)
    assert float((ref.activation64(x, 'gelu') - torch.nn.functional.gelu(x)).abs().max()) < 9 * 2 ** -51    # |x| <= 9, a few float64 roundings
    assert torch.equal(ref.activation64(x, 'quick_gelu'), clip_ref.quick_gelu(x))
    cfg_q, cfg_g, sd = ref.image_cfg('s5'), ref.image_cfg('s5', 'gelu'), ref.state_dict('image', 's5')
    img = ref.images('s5', 2, 1)
    assert ref.rel_err(ref.encode_image64(sd, cfg_g, img), ref.encode_image64(sd, cfg_q, img)) > 1e-3
    with pytest.raises(ValueError):
        ref.activation64(x, 'relu')


def test_first_max_and_prompts():
    tok = torch.tensor([[3, 9, 9, 1], [5, 5, 5, 5], [1, 2, 3, 4], [7, 1, 1, 7]])
    assert ref.first_max(tok).tolist() == [1, 0, 3, 0]
    for ctx in (77, 17):
        tok, names = ref.eot_prompts(ctx)
        P = ref.EOT_POSITIONS[ctx]
        assert tok.shape == (len(P) + 3, ctx) and tok.dtype == torch.int32 and len(names) == len(tok)
        assert int(tok.min()) >= 1 and int(tok.max()) == ref.EOT < ref.VOCAB
        idx = ref.first_max(tok)
        assert idx[:len(P)].tolist() == list(P)
        tie, other, equal = (tok[names.index(k)] for k in ('tie', 'other_max', 'all_equal'))
        assert int((tie == ref.EOT).sum()) == 3 and int(idx[names.index('tie')]) == int((tie == ref.EOT).nonzero()[0])
        assert int(other.max()) == 90 and int(idx[names.index('other_max')]) == 7 and int((other == 90).sum()) == 1
        assert len(set(equal.tolist())) == 1 and int(idx[names.index('all_equal')]) == 0
        alt = ref.replace_suffix(tok)
        assert torch.equal(ref.first_max(alt), idx) and int(alt.min()) >= 0
        for r in range(len(tok)):
            p = int(idx[r])
            assert torch.equal(alt[r, :p + 1], tok[r, :p + 1]) and bool((alt[r, p + 1:] < tok[r].max()).all())
            assert bool((alt[r, p + 1:] != tok[r, p + 1:]).all())
    assert len(ref.eot_prompts(77)[0]) >= 14            # the 14-prompt chunked call covers every position


def test_case_tables():
    assert {t: ref.seq_len(t) for t in ref.TOWERS} == {'s5': 5, 's5_l1': 5, 's10': 10, 's50': 50, 's257': 257, 's325': 325}
    # K + V images of s325 are beyond 80 KiB, those of s257 are not (attention's 16-wave dispatch)
    assert 2 * 325 * 64 * 2 > 80 << 10 > 2 * 257 * 64 * 2
    n, chunk = ref.TAIL_CASE['s10']
    assert chunk * ref.seq_len('s10') > 256 > (chunk - 1) * ref.seq_len('s10') and n - chunk == 1
    for tower, chain in ref.CHAIN_CASES:
        c, layers, W = ref.CHAINS[chain], ref.TOWERS[tower][3], ref.TOWERS[tower][2]
        assert c['kw'].get('image_precise_blocks', 0) < max(layers, 1) or not c['kw'].get('image_precise_blocks')
        assert not c['kw'].get('image_lo_fp8') or W % 128 == 0
    for tower in ('s5', 's10'):
        have = {c for t, c in ref.CHAIN_CASES if t == tower}
        assert {'plain', 'folded', 'folded_full_last_block', 'split_1_0', 'precise', 'low_latency', 'plain_gelu', 'folded_gelu',
                'precise_gelu', 'plain_bf16', 'folded_bf16', 'precise_bf16', 'precise_w16', 'split_1_0_w16'} <= have
    assert {c for t, c in ref.CHAIN_CASES if t == 's5_l1'} == {'plain', 'folded', 'precise'}
    assert ref.chunks_for(7) == [1, 2, 6, 7, 12] and ref.chunks_for(1) == [1, 2, 6] and ref.chunks_for(27) == [1, 2, 26, 27, 32]


# ---- the bounds can be met on the tiny towers ----
# the share of a bound that the operand rounding alone may take on the accuracy weights: the rest is for what a kernel adds
# (fp32 accumulation, the softmax weights' rounding) and for another draw of the same rounding errors
ROOM = 0.6


@pytest.mark.parametrize('tower', list(ref.TOWERS))
def test_operand_rounding_alone_leaves_room_under_the_image_bounds(tower):
    """ref.WEIGHTS['accuracy'] was chosen on this: a float64 tower with nothing but the 16-bit rounding of matrices and
    GEMM inputs stays below ROOM of the 16-bit chains' bounds, plain and folded, f16 and bf16, both activations (the
    QM_RAW towers: f16 QuickGELU, the chains they run).  The 'edges' weights of the bit-for-bit tests do not."""
    small = tower in ('s5', 's5_l1', 's10')
    img = ref.images(tower, 3 if small else 2, 5)
    worst = {}
    for act in (('quick_gelu', 'gelu') if small else ('quick_gelu',)):
        cfg, sd = ref.image_cfg(tower, act), ref.state_dict('image', tower, False, 'accuracy')
        want = ref.encode_image64(sd, cfg, img)
        for dt, bound in ((torch.float16, 1e-3), (torch.bfloat16, 1e-2)) if small else ((torch.float16, 1e-3),):
            for folded in (False, True):
                err = ref.rel_err(ref.emulate_image16(sd, cfg, img, dt, folded), want)
                worst[bound] = max(worst.get(bound, 0.0), err)
                assert err < ROOM * bound, (tower, act, dt, folded, err)
    print(f'\n[{tower}] operand rounding alone: ' + ', '.join(f'{e:.2e} of {b:g}' for b, e in worst.items()), end='')
    if tower == 's10':
        cfg, sd = ref.image_cfg(tower), ref.state_dict('image', tower, False, 'edges')
        assert ref.rel_err(ref.emulate_image16(sd, cfg, img), ref.encode_image64(sd, cfg, img)) > 1e-3


@pytest.mark.parametrize('tower', list(ref.TEXT_TOWERS))
def test_operand_rounding_alone_leaves_room_under_the_text_bounds(tower):
    for act in ('quick_gelu', 'gelu'):
        cfg, sd = ref.text_cfg(tower, act), ref.state_dict('text', tower)
        tok = ref.eot_prompts(cfg['context_length'])[0]
        want = ref.encode_text64(sd, cfg, tok)
        for dt, bound in ((torch.float16, 1e-3), (torch.bfloat16, 1e-2)):
            err = ref.rel_err(ref.emulate_text16(sd, cfg, tok, dt), want)
            print(f'\n[{tower} {act} {dt}] operand rounding alone: {err:.2e} of {bound:g}', end='')
            assert err < ROOM * bound, (tower, act, dt, err)


# ---- the relations hold exactly in the reference ----
@pytest.mark.parametrize('tower', ['t77_w64', 't17_w128'])
def test_suffix_independence_is_exact_in_the_reference(tower):
    """A masked key contributes an exact zero, and every other step is row by row: the features of a prompt do not
    depend on the tokens behind its first maximum, to the last bit of float64."""
    cfg, sd = ref.text_cfg(tower), ref.state_dict('text', tower)
    tok, _ = ref.eot_prompts(cfg['context_length'])
    a, b = ref.encode_text64(sd, cfg, tok), ref.encode_text64(sd, cfg, ref.replace_suffix(tok))
    ref.assert_same_bits(a, b, 'float64 features with the suffix replaced')
    # ... and they do depend on a token in front of it
    front = tok.clone()
    rows = ref.first_max(tok) >= 2
    front[rows, 1] = front[rows, 1] % 90 + 1
    c = ref.encode_text64(sd, cfg, front)
    assert bool(((a - c).abs().amax(1) > 1e-6)[rows].all()) and torch.equal(a[~rows], c[~rows])


# ---- the harness against a stand-in driver ----
def _standin(fault=None, tower='t17_w64'):
    return ref.StandInTextDriver(ref.state_dict('text', tower), ref.text_cfg(tower), fault)


def _check_a(drv):
    n, chunk = ref.TEXT_TAIL_CASE
    ctx = drv.cfg['context_length']
    feats = ref.check_workspace_independence(drv, ref.random_prompts(n, ctx, 1), n, chunk, ref.random_prompts(n + 2, ctx, 2))
    ref.check_refusals(drv, ref.random_prompts(n, ctx, 1), n, chunk, feats)


def _check_b(drv):
    ref.check_chunk_invariance(drv, ref.random_prompts(5, drv.cfg['context_length'], 3), 5)


def _check_c1(drv):
    tok, _ = ref.eot_prompts(drv.cfg['context_length'])
    ref.assert_accuracy(ref.encode(drv, tok, len(tok), len(tok)), ref.encode_text64(drv.sd, drv.cfg, tok), FP32_BOUND)


def _check_c2(drv):
    ref.check_suffix_independence(drv, ref.eot_prompts(drv.cfg['context_length'])[0])


def _check_c3(drv):
    tok = ref.eot_prompts(drv.cfg['context_length'])[0]
    n = min(14, len(tok))
    ref.check_chunk_invariance(drv, tok[:n].contiguous(), n, chunks=(4,))


CHECKS = {'A': _check_a, 'B': _check_b, 'C1': _check_c1, 'C2': _check_c2, 'C3': _check_c3}
# the check each fault was written for
CAUGHT_BY = {'stale_read': 'A', 'workspace_overrun': 'A', 'feats_overrun': 'A', 'last_max': 'C1', 'mask_off_by_one': 'C2',
             'tail_offsets': 'B', 'eot_not_rebased': 'C3'}


@pytest.mark.parametrize('tower', ['t17_w64', 't77_w64'])
def test_harness_passes_a_correct_driver(tower):
    for check in CHECKS.values():
        check(_standin(None, tower))


@pytest.mark.parametrize('fault', ref.FAULTS)
def test_harness_catches_the_fault(fault):
    assert set(CAUGHT_BY) == set(ref.FAULTS)
    with pytest.raises(AssertionError):
        CHECKS[CAUGHT_BY[fault]](_standin(fault))


@pytest.mark.parametrize('fault,message', [('workspace_overrun', 'bytes behind the workspace'), ('feats_overrun', 'feature rows behind row n'),
                                           ('stale_read', 'workspace')])
def test_harness_names_what_it_caught(fault, message):
    with pytest.raises(AssertionError, match=message):
        _check_a(_standin(fault))


def test_refused_call_that_wrote_first_is_caught():
    """A driver that starts writing before it checks the workspace size is caught by the refusal check."""
    class Eager(ref.StandInTextDriver):
        def call(self, tok, n, feats, ws, ws_bytes, chunk):
            if ws is not None:
                ws[0] ^= 0x55
            return super().call(tok, n, feats, ws, ws_bytes, chunk)
    drv = Eager(ref.state_dict('text', 't17_w64'), ref.text_cfg('t17_w64'))
    n, chunk = ref.TEXT_TAIL_CASE
    with pytest.raises(AssertionError, match='workspace of a refused call'):
        ref.run_guarded(drv, ref.random_prompts(n, 17, 1), n, chunk, 0x00, short=1)
