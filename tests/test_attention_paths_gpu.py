"""Every dispatch path of the forward attention kernels (csrc/attention.hip) against float64, on Gaussian and on directed
inputs: tests/attention_ref.py holds the references, the path predicates and the inputs, tests/test_attention_ref_cpu.py
shows that the lengths below reach every path and that the directed inputs are within the tolerances' reach.

The lengths: 1 .. 96 walk the tail kinds and block variants of one wave round; 129, 257 (8 waves) and 513 (16 waves) are
the three lengths whose last query tile is split over the waves -- at 129 four of the eight waves get no key -- and 145,
273, 529 are S = 16 n + 1 lengths that must not split; 288 | 289 is the step from 8 to 16 waves; 608 .. 640 the LDS limit.
Two sequences, two heads, one launch per case."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_SEQ, HEADS, W = 2, 2, 128
DTYPES = {'float16': torch.float16, 'bfloat16': torch.bfloat16}
DIRECTED = ('all_low', 'spike', 'staggered')
GUARD = 3          # rows behind the output that must stay as they were


def _code(dtype):
    from eventclip_amd import _lib
    return _lib.EC_F16 if dtype == torch.float16 else _lib.EC_BF16


def _close(got, want, rtol, atol, what):
    assert torch.isfinite(got).all(), f'{what}: not finite'
    excess = (got - want).abs() - (atol + rtol * want.abs())
    assert float(excess.max()) <= 0, f'{what}: {float((got - want).abs().max()):.3e} off, {float(excess.max()):.3e} over'


def _launch16(api, qkv, S, causal, q_rows, dtype, n_seq=N_SEQ):
    """-> out [n_seq * q_rows, W] float64 on the CPU (and the log-sum-exp for 'train'); the rows behind the output were
    filled with NaN and must come back as NaN."""
    from eventclip_amd import _lib
    dev = qkv.cuda()
    buf = torch.full((n_seq * q_rows + GUARD, W), float('nan'), dtype=dtype, device='cuda')
    lse = None
    args = (n_seq, S, W, HEADS)
    if api == 'plain':
        rc = _lib.lib().ec_attention(_lib.ptr(dev), _lib.ptr(buf), *args, causal, _code(dtype), _lib.stream_ptr())
    elif api == 'rows':
        rc = _lib.lib().ec_attention_rows(_lib.ptr(dev), _lib.ptr(buf), *args, causal, q_rows, _code(dtype), _lib.stream_ptr())
    elif api == 'scaled':
        rc = _lib.lib().ec_attention_scaled_q(_lib.ptr(dev), _lib.ptr(buf), *args, causal, q_rows, _code(dtype), _lib.stream_ptr())
    else:
        lse = torch.full((N_SEQ, HEADS, S), float('nan'), dtype=torch.float32, device='cuda')
        rc = _lib.lib().ec_attention_train(_lib.ptr(dev), _lib.ptr(buf), _lib.ptr(lse), *args, _code(dtype), _lib.stream_ptr())
    _lib.check(rc, api)
    buf = buf.cpu()
    assert torch.isnan(buf[n_seq * q_rows:]).all(), 'rows behind the requested ones were written'
    return buf[:n_seq * q_rows].double(), None if lse is None else lse.cpu().double()


def _check16(kind, api, S, dtype, causal, q_rows=None):
    prescaled = int(api == 'scaled')
    qkv, want, want_lse = ref.case16(kind, S, dtype, prescaled, causal)
    q_rows = S if q_rows is None else q_rows
    got, lse = _launch16(api, qkv, S, causal, q_rows, dtype)
    tol = ref.out_tol(dtype, kind)
    _close(got, want.view(N_SEQ, S, W)[:, :q_rows].reshape(N_SEQ * q_rows, W), tol, tol, f'{api} {kind} S={S} out')
    if lse is not None:
        floor = 0.0 if dtype == torch.float16 else 2 * ref.BF16_LSE_EMULATION_ERR
        assert torch.isfinite(lse).all()
        excess = (lse - want_lse).abs() - torch.clamp(ref.LSE_ATOL + ref.LSE_RTOL * want_lse.abs(), min=floor)
        assert float(excess.max()) <= 0, f'lse {kind} S={S}: {float((lse - want_lse).abs().max()):.3e} off'


@pytest.mark.parametrize('api', ['plain', 'scaled'])
@pytest.mark.parametrize('causal', [0, 1])
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('S', ref.S_16BIT)
def test_gaussian_at_every_length(S, dt, causal, api, hip):
    """ec_attention (f16: the kernel scales and re-rounds q; bf16: fp32 scores scaled) and ec_attention_scaled_q, both
    masks, at every length of the table: 4e-3 (f16) / 2.5e-2 (bf16) of float64."""
    _check16('gaussian', api, S, DTYPES[dt], causal)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('S', ref.S_16BIT)
def test_train_output_and_log_sum_exp(S, dt, hip):
    """ec_attention_train at every length, both types: the output as above and the log-sum-exp (log2 of the softmax
    denominator over the scaled scores) within rtol 2e-3 / atol 2e-2 of float64, the f16 bound of
    test_attention_lse_matches_reference.  bf16 has no bound of its own: the emulation's bf16 log-sum-exp lies
    1.9e-3 from float64 at most over these inputs (attention_ref.BF16_LSE_EMULATION_ERR), so twice that, which
    allows for the fp32 accumulation the emulation leaves out, is below the f16 bound and the f16 bound holds."""
    _check16('gaussian', 'train', S, DTYPES[dt], 0)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('S,q_rows', [(S, r) for S in ref.S_ROWS for r in ref.rows_cases(S)])
def test_rows_at_the_split_lengths(S, q_rows, dt, hip):
    """ec_attention_rows at the three lengths with a split last tile: a prefix inside the first tile, around the tile
    edge, everything but the split tile's row (S - 1: the split is skipped) and everything.  A second launch takes each
    sequence on its own, so that the NaN guard lies right behind ITS rows: row q_rows of a sequence, were it written,
    lands there and not in the next sequence's row 0."""
    dtype = DTYPES[dt]
    _check16('gaussian', 'rows', S, dtype, 0, q_rows)
    qkv, want, _ = ref.case16('gaussian', S, dtype, 0, 0)
    tol = ref.out_tol(dtype, 'gaussian')
    for seq in range(N_SEQ):
        got, _ = _launch16('rows', qkv[seq * S:(seq + 1) * S], S, 0, q_rows, dtype, n_seq=1)
        _close(got, want[seq * S:seq * S + q_rows], tol, tol, f'rows S={S} sequence {seq} alone')


def _directed_cases():
    for kind in DIRECTED:
        for S in (ref.S_DIRECTED if kind != 'staggered' else ref.S_LONE + (289, 577)):
            for api, causal in (('plain', 0), ('plain', 1), ('scaled', 0), ('scaled', 1), ('train', 0)):
                if kind == 'staggered' and causal:
                    continue
                yield kind, S, api, causal


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('kind,S,api,causal', list(_directed_cases()))
def test_directed_inputs(kind, S, api, causal, dt, hip):
    """The running maximum's moves, forced.  all_low: every score of every query far below zero, so each tile's first
    contribution -- whichever block variant, the odd key at S = 1, each wave's share of a split tile -- must move the
    maximum DOWN (without it P underflows and the row is 0 / 0).  spike: chosen keys (the last key among them) score far
    above everything before them for chosen rows (the last row, and for the causal mask the rows on and just below the
    diagonal).  staggered: every 32-key step's maximum more than 2^10 from the one before, rising then falling, so the
    waves of a split tile merge partial results that all stand on different maxima.  Tolerances as for the Gaussian
    cases (bf16 with spikes: 4e-2, test_attention_running_maximum_moves' figure)."""
    _check16(kind, api, S, DTYPES[dt], causal)


def _launch_split(hi, lo, S, prescaled, dtype):
    from eventclip_amd import _lib
    planes = torch.stack([hi, lo]).cuda()
    out = torch.full((2, N_SEQ * S, W), float('nan'), dtype=dtype, device='cuda')
    _lib.check(_lib.lib().ec_attention_split(_lib.ptr(planes[0]), _lib.ptr(planes[1]), _lib.ptr(out[0]), _lib.ptr(out[1]),
                                             N_SEQ, S, W, HEADS, prescaled, _code(dtype), _lib.stream_ptr()),
               'ec_attention_split')
    return out[0].cpu().double() + out[1].cpu().double()


def _check_planes(got, want, dtype, what):
    assert torch.isfinite(got).all(), f'{what}: not finite'
    err = float((got - want).abs().max() / want.abs().max())
    assert err < ref.SPLIT_BOUND[dtype], f'{what}: {err:.3e}'


def _split_cases():
    for pre in (0, 1):
        for S in ref.S_SPLIT:
            yield 'gaussian', S, pre, 'float16'
        for S in ref.S_SPLIT_BF16:
            yield 'gaussian', S, pre, 'bfloat16'
        for kind in DIRECTED:
            for S in ref.S_SPLIT_DIRECTED:
                yield kind, S, pre, 'float16'


@pytest.mark.parametrize('kind,S,prescaled,dt', list(_split_cases()))
def test_split_planes(kind, S, prescaled, dt, hip):
    """ec_attention_split against float64 of the joined planes: a plain f16 q on attention_hl_kernel (one pass, up to
    S = 320), attention_hl2_kernel (two passes: odd-key tails at 353 and 577, a masked one at 600, none at 608, spikes on
    both sides of the pass boundary) or the fp32 kernel (609), a pre-scaled q and bf16 planes on the fp32 kernel.
    4e-6 of the largest output for f16 planes, 4e-5 for bf16 ones (test_layernorm_of_the_planes' figure for 16 bits in
    two parts).  The directed inputs are smaller than the 16-bit kernels' (attention_ref.SPLIT_*): fp32 arithmetic
    itself passes the bound on deeper ones."""
    dtype = DTYPES[dt]
    hi, lo, want = ref.case_split(kind, S, dtype, prescaled)
    _check_planes(_launch_split(hi, lo, S, prescaled, dtype), want, dtype, f'split {kind} S={S} prescaled={prescaled}')


def _f32_cases():
    for causal in (0, 1):
        for S in ref.S_SPLIT:
            yield 'gaussian', S, causal, 'float16'
        for S in ref.S_SPLIT_BF16:
            yield 'gaussian', S, causal, 'bfloat16'
    for kind in DIRECTED:
        for S in ref.S_SPLIT_DIRECTED:
            yield kind, S, 0, 'float16'


@pytest.mark.parametrize('kind,S,causal,dt', list(_f32_cases()))
def test_f32_planes(kind, S, causal, dt, hip):
    """ec_attention_f32 (fp32 q | k | v in, hi + lo planes of either type out), both masks, the same bounds."""
    from eventclip_amd import _lib
    dtype = DTYPES[dt]
    qkv, want = ref.case_f32(kind, S, causal)
    dev = qkv.cuda()
    out = torch.full((2, N_SEQ * S, W), float('nan'), dtype=dtype, device='cuda')
    _lib.check(_lib.lib().ec_attention_f32(_lib.ptr(dev), _lib.ptr(out[0]), _lib.ptr(out[1]), N_SEQ, S, W, HEADS, causal,
                                           _code(dtype), _lib.stream_ptr()), 'ec_attention_f32')
    _check_planes(out[0].cpu().double() + out[1].cpu().double(), want, dtype, f'f32 {kind} S={S} causal={causal}')
