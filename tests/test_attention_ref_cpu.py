"""The attention yardsticks of tests/attention_ref.py, checked without a GPU: the float64 reference against torch's own,
the directed inputs against the tolerances they are used with, the generators against what they promise, and the shape
tables of tests/test_attention_paths_gpu.py against every path of csrc/attention.hip's dispatch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as ref  # noqa: E402

DTYPES = {'float16': torch.float16, 'bfloat16': torch.bfloat16}
DIRECTED = ('all_low', 'spike', 'staggered')


def _s_of(kind):
    return ref.S_DIRECTED if kind != 'staggered' else ref.S_LONE + (289, 577)


@pytest.mark.parametrize('S,heads,causal,q_rows,prescaled', [(1, 1, 0, 1, 0), (17, 2, 1, 17, 0), (77, 3, 1, 5, 1),
                                                             (129, 2, 0, 128, 0), (257, 1, 0, 257, 1)])
def test_exact_is_scaled_dot_product_attention(S, heads, causal, q_rows, prescaled):
    n_seq = 2
    qkv = ref.pack(ref.gaussian(S, n_seq, heads), torch.float16, prescaled)
    out, lse = ref.exact(qkv, n_seq, S, heads, causal, q_rows, prescaled)
    q, k, v = ref.heads_of(qkv.double(), n_seq, S, heads)
    if prescaled:
        q = q / ref.C * 0.125
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=bool(causal), scale=1.0 if prescaled else 0.125)
    want = want[:, :, :q_rows].permute(0, 2, 1, 3).reshape(n_seq * q_rows, heads * 64)
    assert out.dtype == torch.float64 and float((out - want).abs().max()) < 1e-12
    s = q @ k.transpose(-1, -2) * (1.0 if prescaled else 0.125)
    if causal:
        s = s + torch.full((S, S), float('-inf'), dtype=torch.float64).triu_(1)
    assert float((lse - torch.logsumexp(s, -1)[:, :, :q_rows] * ref.LOG2E).abs().max()) < 1e-10


@pytest.mark.parametrize('kind', DIRECTED)
@pytest.mark.parametrize('prescaled', [0, 1])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_directed_inputs_leave_half_the_tolerance(dt, prescaled, kind):
    """The kernel's own three roundings, in float64 otherwise, stay within HALF of the tolerance the GPU test asserts on
    every directed input -- output and log-sum-exp -- so the other half is the kernel's to use."""
    dtype = DTYPES[dt]
    tol = ref.out_tol(dtype, kind)
    for S in _s_of(kind):
        for causal in ((0, 1) if kind != 'staggered' else (0,)):
            qkv, out, lse = ref.case16(kind, S, dtype, prescaled, causal)
            e_out, e_lse = ref.emulated(qkv, 2, S, 2, causal, None, prescaled, dtype)
            assert torch.isfinite(e_out).all()
            assert float(((e_out - out).abs() - 0.5 * (tol + tol * out.abs())).max()) <= 0, (S, causal)
            assert float(((e_lse - lse).abs() - 0.5 * (ref.LSE_ATOL + ref.LSE_RTOL * lse.abs())).max()) <= 0, (S, causal)


def test_bf16_log_sum_exp_emulation_error():
    """The figure behind the bf16 log-sum-exp bound: max |emulated - exact| over every input ec_attention_train gets in
    tests/test_attention_paths_gpu.py.  Twice it stays below the f16 bound's absolute part, so the f16 bound holds."""
    worst = 0.0
    cases = [('gaussian', S) for S in ref.S_16BIT] + [(kind, S) for kind in DIRECTED for S in _s_of(kind)]
    for kind, S in cases:
        qkv, _, lse = ref.case16(kind, S, torch.bfloat16, 0, 0)
        worst = max(worst, float((ref.emulated(qkv, 2, S, 2, 0, None, 0, torch.bfloat16)[1] - lse).abs().max()))
    print(f'\nbf16 log-sum-exp, emulated against exact: {worst:.3e}')
    assert worst <= ref.BF16_LSE_EMULATION_ERR
    assert 2 * ref.BF16_LSE_EMULATION_ERR < ref.LSE_ATOL


@pytest.mark.parametrize('prescaled', [0, 1])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_all_low_is_low_everywhere(dt, prescaled):
    """Every visible score of every query is below -ATTN_LO, a fortiori each tile's first block; at the 16-bit kernels'
    depth an f16 / bf16 P taken against a maximum of 0 would be 0."""
    dtype = DTYPES[dt]
    for S in ref.S_DIRECTED:
        top = ref.step_maxima(ref.case16('all_low', S, dtype, prescaled, 0)[0], 2, S, 2, 0, prescaled).amax()
        assert float(top) < (-24 if dtype == torch.float16 else -133), (S, float(top))
    for S in ref.S_SPLIT_DIRECTED:
        hi, lo, _ = ref.case_split('all_low', S, dtype, prescaled)
        top = ref.step_maxima(hi.double() + lo.double(), 2, S, 2, 0, prescaled).amax()
        assert float(top) < -ref.ATTN_LO - 1, (S, float(top))


def _spike_margin(qkv, S, causal, prescaled):
    """Smallest (score at the spiked key) - max(0, every score of the 32-key steps before the key's) over the plan's rows."""
    q, k, _ = ref.heads_of(qkv.double(), 2, S, 2)
    s = (q @ k.transpose(-1, -2)) * (1.0 if prescaled else ref.C)
    sm = ref.step_maxima(qkv, 2, S, 2, causal, prescaled)
    worst = float('inf')
    for key, rows in ref.spike_plan(S):
        rows = [r for r in rows if not causal or r >= key]
        before = sm[:, :, rows, :key // 32].amax(-1).clamp(min=0) if key >= 32 else torch.zeros(2, 2, len(rows), dtype=torch.float64)
        worst = min(worst, float((s[:, :, rows, key] - before).min()))
    return worst


@pytest.mark.parametrize('prescaled', [0, 1])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_spikes_exceed_the_running_maximum(dt, prescaled):
    """Each spiked key scores more than ATTN_THR above the running maximum its rows bring to the key's step (which starts
    at 0), mask or not; the plan holds the last key, the last row and the diagonal."""
    dtype = DTYPES[dt]
    for S in ref.S_DIRECTED:
        plan = ref.spike_plan(S)
        assert plan[-1][0] == S - 1 and S - 1 in plan[-1][1] and all(key in rows and min(key + 1, S - 1) in rows for key, rows in plan)
        for causal in (0, 1):
            assert _spike_margin(ref.case16('spike', S, dtype, prescaled, causal)[0], S, causal, prescaled) > ref.ATTN_THR, S
    for S in ref.S_SPLIT_DIRECTED:
        hi, lo, _ = ref.case_split('spike', S, dtype, prescaled)
        assert _spike_margin(hi.double() + lo.double(), S, 0, prescaled) > ref.ATTN_THR, S


@pytest.mark.parametrize('dt', list(DTYPES))
def test_staggered_steps_are_more_than_the_threshold_apart(dt):
    """For the staggered rows every step of the rising half tops the running maximum by more than ATTN_THR and every step
    of the falling half lies more than ATTN_THR below the one before; the split kernels' two-level variant rises by
    more than ATTN_THR at step 1 and alternates by that much afterwards."""
    dtype = DTYPES[dt]
    for S in _s_of('staggered'):
        for prescaled in (0, 1):
            sm = ref.step_maxima(ref.case16('staggered', S, dtype, prescaled, 0)[0], 2, S, 2, 0, prescaled)
            sm = sm[:, :, ref.staggered_rows(S)]
            n = sm.shape[-1]
            peak = (n - 1) // 2
            run = torch.cummax(sm, -1)[0]
            assert float((sm[..., 1:peak + 1] - run[..., :peak]).min()) > ref.ATTN_THR, S
            assert float((sm[..., n - peak - 1:-1] - sm[..., n - peak:]).min()) > ref.ATTN_THR, S
            assert S - 1 in ref.staggered_rows(S)
    for S in ref.S_SPLIT_DIRECTED:
        hi, lo, _ = ref.case_split('staggered', S, dtype, 0)
        sm = ref.step_maxima(hi.double() + lo.double(), 2, S, 2)[:, :, ref.staggered_rows(S)]
        odd, even = sm[..., 1::2], sm[..., 0::2]
        assert float((odd - even[..., :odd.shape[-1]]).min()) > ref.ATTN_THR, S
        assert float((odd[..., :even.shape[-1] - 1] - even[..., 1:]).min()) > ref.ATTN_THR, S


@pytest.mark.parametrize('dt', list(DTYPES))
def test_split_inputs_are_within_reach_of_fp32(dt):
    """fp32 scores, exponentials and sums alone (the split kernels' class of arithmetic) keep every input of the split
    tests within the bound asserted there -- deeper all_low inputs, larger spikes or a full staggered ladder do not:
    fp32 carries 2^-24 of the largest score into each, which is why these inputs are smaller than the 16-bit ones."""
    dtype = DTYPES[dt]
    for prescaled in (0, 1):
        for kind in ('gaussian',) + DIRECTED:
            for S in ref.S_SPLIT_DIRECTED:
                hi, lo, want = ref.case_split(kind, S, dtype, prescaled)
                got = ref.emulated_f32(hi.double() + lo.double(), 2, S, 2, 0, prescaled)
                err = float((got - want).abs().max() / want.abs().max())
                assert err < ref.SPLIT_BOUND[torch.float16], (kind, S, prescaled, err)


def test_the_tables_reach_every_dispatch_path():
    """One assert per path of attention.hip's dispatch, named, over the lengths the GPU tests launch: a change to the
    dispatch (or to the tables) that strands a path fails here."""
    f16, bf16 = torch.float16, torch.bfloat16
    S16 = [S for S in ref.S_16BIT]
    assert all(ref.supported(S, c) for S in S16 + list(ref.S_DIRECTED) for c in (0, 1)), 'every length fits the LDS'
    # --- attention_kernel: wave count and its boundary
    assert ref.waves(288) == 8 and ref.waves(289) == 16 and {288, 289} <= set(S16), '8 | 16 waves boundary'
    assert [S for S in range(1, 641) if ref.waves(S) == 8] == list(range(1, 289)), '8 waves up to S = 288'
    # --- the lone tile: exactly three lengths, all launched; S = 16 n + 1 near-misses and the causal mask do not split
    lone_all = [S for S in range(1, 641) if ref.supported(S) and ref.lone(S, 0, ref.waves(S))]
    assert lone_all == [129, 257, 513] == list(ref.S_LONE) == list(ref.S_ROWS), 'the three lone lengths'
    assert set(lone_all) <= set(S16) and set(lone_all) <= set(ref.S_DIRECTED), 'lone lengths, Gaussian and directed'
    assert ref.waves(513) == 16 and ref.waves(129) == ref.waves(257) == 8, 'lone tile on 16 waves: S = 513'
    assert ref.keyless_waves(129, 8) == [0, 2, 4, 6] and not ref.keyless_waves(257, 8) and not ref.keyless_waves(513, 16), \
        'keyless waves: S = 129 only'
    for S in (145, 273, 529):
        assert S in S16 and (S & 15) == 1 and not ref.lone(S, 0, ref.waves(S)), f'near-miss {S}'
    assert not any(ref.lone(S, 1, ref.waves(S)) for S in range(1, 641)), 'causal never splits'
    for S in ref.S_ROWS:
        assert S - 1 in ref.rows_cases(S) and S in ref.rows_cases(S), 'q_rows = S - 1 drops the lone tile'
    # --- tail kinds on both wave counts
    for w in (8, 16):
        assert {ref.tail_kind(S) for S in S16 if ref.waves(S) == w} == {'none', 'odd', 'masked'}, f'tail kinds on {w} waves'
    # --- every block variant as a tile's first contribution (the `down` arm) under the directed inputs
    first = set()
    for S in ref.S_DIRECTED:
        first |= {(v, 0) for v in ref.block_variants(S, 0, ref.waves(S))} | {(v, 1) for v in ref.block_variants(S, 1, ref.waves(S))}
    for variant in (((2, False), 0), ((1, False), 0), ('odd', 0), ((2, False), 1), ((2, True), 1), ((1, True), 1)):
        assert variant in first, f'down in variant {variant}'
    assert ref.block_variants(1, 0, 8) == {'odd'}, 'the odd key first: S = 1'
    assert ref.block_variants(129, 0, 8) == {(2, False), (1, False)} and ref.block_variants(513, 0, 16) == {(2, False), (1, False)}, \
        'per-wave shares of a lone tile'
    assert any(ref.waves(S) == 16 and ref.tail_kind(S) == 'odd' for S in ref.S_DIRECTED), 'spiked odd key on 16 waves'
    # --- ec_attention_split
    paths = {S: ref.hl_path(S, 0, f16) for S in ref.S_SPLIT}
    assert {p[0] for p in paths.values()} == {'hl', 'hl2', 'f32m'}, 'split: the three kernels'
    assert ref.hl_path(320, 0, f16)[0] == 'hl' and ref.hl_path(321, 0, f16)[0] == 'hl2', 'hl | hl2 boundary'
    assert paths[608][0] == 'hl2' and paths[609][0] == 'f32m', 'hl2 | f32m boundary'
    assert {ref.tail_kind(S) for S, p in paths.items() if p[0] == 'hl'} == {'none', 'odd', 'masked'}, 'hl tail kinds'
    assert {ref.tail_kind(p[2]) for p in paths.values() if p[0] == 'hl2'} == {'none', 'odd', 'masked'}, 'hl2 tail kinds'
    assert paths[600][0] == 'hl2' and ref.tail_kind(paths[600][2]) == 'masked' and 600 in ref.S_SPLIT_DIRECTED, 'hl2 masked tail'
    assert paths[129][0] == paths[257][0] == 'hl' and {129, 257} <= set(ref.S_SPLIT_DIRECTED), 'hl lone tile, keyless waves'
    for S in ref.S_SPLIT_DIRECTED:
        kind, split, _ = ref.hl_path(S, 0, f16)
        if kind == 'hl2':
            keys = [key for key, _ in ref.spike_plan(S)]
            assert min(keys) < split <= max(keys), f'spikes on both sides of the pass boundary at {S}'
    assert {'hl', 'hl2', 'f32m'} == {ref.hl_path(S, 0, f16)[0] for S in ref.S_SPLIT_DIRECTED}, 'directed inputs in the three kernels'
    assert all(ref.hl_path(S, 1, f16)[0] == 'f32m' for S in ref.S_SPLIT), 'pre-scaled q: fp32 kernel'
    assert all(ref.hl_path(S, p, bf16)[0] == 'f32m' for S in ref.S_SPLIT_BF16 for p in (0, 1)), 'bf16 planes: fp32 kernel'
    # --- log-sum-exp: both types on both wave counts come with S_16BIT
    assert {ref.waves(S) for S in S16} == {8, 16}, 'log-sum-exp on 8 and 16 waves'
