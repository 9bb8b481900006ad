"""The yardsticks of tests/rowops_ref.py, checked on the CPU: the builders yield the rows they promise, the float64
references agree with torch's own, the constants of the bounds are MEASURED here (the fp32 restatement of each formula
against float64, over every input the GPU tests use) and must stay below the stored figures, and restatements that are
broken on purpose -- eps outside the root, eps ignored, a one-pass variance, a merge without its clamp -- are rejected
by the bounds the kernels are held to, on the directed rows."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as ref  # noqa: E402

F16, BF16 = torch.float16, torch.bfloat16


def _ln_cases():
    """Every (x fp32, kind, eps, what) the LayerNorm GPU tests normalise: the fp32 rows and the joined hi + lo planes."""
    for width in ref.LN_WIDTHS:
        for rows in ref.ROWS:
            for rot in ref.rotations(rows):
                x, kind = ref.ln_rows(rows, width, rot)
                yield x, kind, width, 'fp32'
                for dt in (F16, BF16):
                    hi, lo = ref.split(x, dt, F16)
                    yield hi.float() + lo.float(), kind, width, f'planes {dt}'     # the kernel's join, in fp32
    for width in ref.EMBED_WIDTHS:                                                 # the embeddings' rows: all ordinary
        for n_img, seq in ref.EMBED_SHAPES:
            x = ref.embed_sum(*ref.embed_inputs(n_img, seq, width), n_img, seq)
            yield x, torch.zeros(len(x), dtype=torch.int64), width, 'embedding'


def _per_kind_max(c_row, kind, into):
    for k in range(4):
        if bool((kind == k).any()):
            into[k] = max(into[k], float(c_row[kind == k].max()))


@functools.lru_cache(maxsize=None)
def measured_ln():
    worst = [0.0] * 4
    for x, kind, width, _ in _ln_cases():
        gamma, beta = ref.gamma_beta(width)
        for eps in ref.EPS:
            want, s = ref.layernorm64(x, gamma, beta, eps)
            err = (ref.layernorm32(x, gamma, beta, eps).double() - want).abs().amax(-1)
            _per_kind_max(err / (ref.EPS32 * s), kind, worst)
    return worst


@functools.lru_cache(maxsize=None)
def measured_stats():
    worst = [0.0] * 4
    for width in ref.STATS_WIDTHS:
        for rows in ref.ROWS:
            for rot in ref.rotations(rows):
                x32, kind = ref.ln_rows(rows, width, rot)
                for dt in (F16, BF16):
                    x = x32.to(dt)
                    for eps in ref.EPS:
                        want = ref.row_stats64(x, eps)
                        err = (ref.row_stats32(x, eps).double() - want).abs()
                        xmax = x.double().abs().amax(-1)
                        c = torch.maximum(err[:, 0] / want[:, 0], err[:, 1] / (want[:, 0] * xmax)) / ref.EPS32
                        _per_kind_max(c, kind, worst)
    return worst


def _merge_cases():
    for groups in ref.MERGE_GROUPS:
        for rows in ref.MERGE_ROWS:
            for rot in ref.rotations(rows):
                for dt in (F16, BF16):
                    yield ref.merge_sums(rows, groups, dt, rot) + (64 * groups,)


@functools.lru_cache(maxsize=None)
def measured_merge():
    worst = 0.0
    for sums, kind, width in _merge_cases():
        for eps in ref.EPS:
            want, cond, absum = ref.merge64(sums, width, eps)
            err = (ref.merge32(sums, width, eps)[0].double() - want).abs()
            unit = ref.EPS32 * (1 + cond) * want[:, 0]
            worst = max(worst, float((err[:, 0] / unit).max()), float((err[:, 1] / (unit * absum)).max()))
    return worst


@functools.lru_cache(maxsize=None)
def measured_gelu():
    worst = 0.0
    for n in ref.SPLIT_N + (1 << 20,):
        x = ref.split_input(n)
        want = ref.gelu64(x)
        err = ((ref.gelu32(x).double() - want).abs() - ref.FLOOR_GELU).clamp(min=0)
        worst = max(worst, float((err / (ref.EPS32 * (1 + (1.702 * x.double()).abs()) * want.abs())).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------
def test_builders_yield_the_rows_they_promise():
    """Every LayerNorm / statistics / merge case, over its rotations, holds a constant row (variance exactly 0 in
    float64), a large-mean row (|mean| > 250 deviations) and a near-epsilon row (variance within 2x of 1e-5)."""
    for width in sorted(set(ref.LN_WIDTHS + ref.STATS_WIDTHS + tuple(64 * g for g in ref.MERGE_GROUPS))):
        for rows in sorted(set(ref.ROWS + ref.MERGE_ROWS)):
            seen = set()
            for rot in ref.rotations(rows):
                x, kind = ref.ln_rows(rows, width, rot)
                assert x.shape == (rows, width) and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
                x = x.double()
                var, mean = x.var(-1, unbiased=False), x.mean(-1)
                assert bool((var[kind == ref.CONSTANT] == 0).all())
                if width >= 64:      # four samples say little about a deviation
                    assert bool((mean[kind == ref.LARGE_MEAN].abs() > 250 * var[kind == ref.LARGE_MEAN].sqrt()).all())
                    near = var[kind == ref.NEAR_EPS]
                    assert bool(((near > 0.5e-5) & (near < 2e-5)).all())
                seen |= set(kind.tolist())
            assert seen == {ref.ORDINARY, ref.LARGE_MEAN, ref.NEAR_EPS, ref.CONSTANT}, (rows, width, seen)
    # rows of different scale and an outlier channel
    x, kind = ref.ln_rows(1021, 256, 0)
    spread = x.double().std(-1)[kind == ref.ORDINARY]
    assert float(spread.max() / spread.min()) > 60
    assert float(x[4].abs().max() / x[4].abs().median()) > 20
    # the constant rows stay constant in 16 bit and in the planes
    for dt in (F16, BF16):
        hi, lo = ref.split(x, dt, F16)
        assert bool((lo[kind == ref.CONSTANT] == 0).all()) and bool((hi[kind == ref.CONSTANT].double().var(-1) == 0).all())


def test_merge_builder_goes_below_zero():
    """The merge inputs hold rows whose fp32 E[x^2] - mean^2 is NEGATIVE before the clamp -- by more than eps, so that an
    unclamped merge yields NaN -- among them rows that ARE constant in 16 bit (the large-mean rows; float64 variance 0),
    and the constant rows proper give exactly 0."""
    neg = pos = 0
    for sums, kind, width in _merge_cases():
        assert sums.dtype == torch.float32 and sums.shape[1:] == (width // 64, 2)
        stats, var = ref.merge32(sums, width, 1e-5, clamp=False)
        assert bool((var[kind == ref.CONSTANT] == 0).all())
        flat = ref.merge64(sums, width, 0.0)[1] == float('inf')           # float64 variance of the sums <= 0
        neg += int((var < -1e-5).sum())
        pos += int(((var < 0) & flat).sum())
        assert bool(torch.isfinite(ref.merge32(sums, width, 1e-5)[0]).all())
        assert bool(torch.isfinite(ref.merge64(sums, width, 1e-5)[0]).all())
    assert neg > 50 and pos > 50, (neg, pos)


def test_references_agree_with_torch():
    x, _ = ref.ln_rows(5, 260, 0)
    gamma, beta = ref.gamma_beta(260)
    want = torch.nn.functional.layer_norm(x.double(), (260,), gamma.double(), beta.double(), 1e-5)
    got, s = ref.layernorm64(x, gamma, beta, 1e-5)
    assert float((got - want).abs().max()) < 1e-9
    assert s.shape == (5,) and bool((s >= beta.abs().max()).all())
    st = ref.row_stats64(x, 1e-5)
    rstd = 1 / torch.sqrt(x.double().var(-1, unbiased=False) + 1e-5)
    assert float((st[:, 0] / rstd - 1).abs().max()) < 1e-12 and float((st[:, 1] + rstd * x.double().mean(-1)).abs().max()) < 1e-9
    # group sums -> the same statistics (float64 sums of f16 rows; the fp32 rounding of the sums is all that differs)
    sums, kind = ref.merge_sums(17, 4, F16, 0)
    x16 = ref.ln_rows(17, 256, 0)[0].half()
    m, cond, _ = ref.merge64(sums, 256, 1e-3)
    assert float(((m[:, 0] - ref.row_stats64(x16, 1e-3)[:, 0]).abs() / m[:, 0] - 4 * ref.EPS32 * (1 + cond)).max()) <= 0
    xs = ref.split_input(1028)
    assert float((ref.gelu64(xs) - xs.double() * torch.sigmoid(1.702 * xs.double())).abs().max()) < 1e-12
    assert bool((xs.abs() > 55).any()) and bool(((xs.abs() > 15) & (xs.abs() < 25)).any()) and bool((xs.abs() < 1e-5).any())
    assert torch.equal(ref.tree_sum32(torch.arange(7.0)[None]), torch.tensor([21.0]))


def test_split_is_exact_to_the_pair_bound():
    x = ref.split_input(1 << 16)
    for hi_dt, lo_dt in ((F16, F16), (BF16, BF16), (BF16, F16)):
        hi, lo = ref.split(x, hi_dt, lo_dt)
        bound = ref.bound_pair(x.double(), 0.0, hi_dt, lo_dt)
        assert ref.excess(hi.double() + lo.double(), x.double(), bound) <= 0
    assert ref.pair_u(F16, F16) == 2.0 ** -22 and ref.pair_u(BF16, BF16) == 2.0 ** -16


def test_measured_constants_stay_below_the_stored_ones(capsys):
    ln, st, mg, ge = measured_ln(), measured_stats(), measured_merge(), measured_gelu()
    with capsys.disabled():
        print('\nmeasured C (LayerNorm)  ', {ref.KINDS[k]: round(ln[k], 2) for k in range(4)})
        print('measured C (row stats)  ', {ref.KINDS[k]: round(st[k], 2) for k in range(4)})
        print('measured C (merge)      ', round(mg, 3))
        print('measured C (QuickGELU)  ', round(ge, 3))
    for k in range(4):
        assert ln[k] <= ref.C_LN[k], (ref.KINDS[k], ln[k])
        assert st[k] <= ref.C_STATS[k], (ref.KINDS[k], st[k])
        # ... and the stored figure is the measurement rounded up, not a guess far above it
        if k != ref.CONSTANT:
            assert ref.C_LN[k] <= 1.5 * ln[k] and ref.C_STATS[k] <= 1.5 * st[k], ref.KINDS[k]
    assert mg <= ref.C_MERGE <= 1.5 * mg and ge <= ref.C_GELU <= 1.5 * ge
    assert ln[ref.CONSTANT] == 0          # exact sums: see rowops_ref.C_LN


# ---------------------------------------------------------------------------------------------------------------
# broken restatements: each must FAIL the bound the kernel is held to (KERNEL_FACTOR included), on the rows meant for it
# ---------------------------------------------------------------------------------------------------------------
def _ln_broken(x, gamma, beta, eps, how):
    w = x.shape[-1]
    mean = ref.tree_sum32(x) / w
    d = x - mean[:, None]
    eps = torch.tensor(eps, dtype=torch.float32)
    if how == 'one_pass':
        var = (ref.tree_sum32(x * x) / w - mean * mean).clamp(min=0)
    else:
        var = ref.tree_sum32(d * d) / w
    if how == 'eps_outside':
        rstd = 1 / (torch.sqrt(var) + eps)
    elif how == 'eps_ignored':
        rstd = 1 / torch.sqrt(var + 1e-5)
    elif how == 'unbiased':
        rstd = 1 / torch.sqrt(var * (w / (w - 1)) + eps)
    else:
        rstd = 1 / torch.sqrt(var + eps)
    g = gamma.roll(4) if how == 'gamma_unit_shifted' else gamma
    return d * rstd[:, None] * g + beta


@pytest.mark.parametrize('how,kind,eps', [('one_pass', ref.LARGE_MEAN, 1e-5), ('eps_outside', ref.NEAR_EPS, 1e-5),
                                          ('eps_outside', ref.NEAR_EPS, 1e-3), ('eps_ignored', ref.NEAR_EPS, 1e-3),
                                          ('unbiased', ref.ORDINARY, 1e-5), ('gamma_unit_shifted', ref.ORDINARY, 1e-5)])
@pytest.mark.parametrize('width', [64, 260, 2048])
def test_broken_layernorms_are_rejected(width, how, kind, eps):
    """Against the 16-bit bound (the widest of the three) of BOTH types and against the pair bound: the rows of `kind`
    fail, whatever the other rows do, while the sound restatement passes everywhere with KERNEL_FACTOR = 1."""
    x, kinds = ref.ln_rows(1021, width, 0)
    gamma, beta = ref.gamma_beta(width)
    want, s = ref.layernorm64(x, gamma, beta, eps)
    sound = ref.layernorm32(x, gamma, beta, eps)
    assert ref.excess(sound, want, ref.ln_e(s, kinds, factor=1.0)) <= 0
    got = _ln_broken(x, gamma, beta, eps, how)
    rows = kinds == kind
    e = ref.ln_e(s, kinds)

    def caught(failed):
        if how != 'one_pass':
            return bool(failed.all())
        # the rows around -300 (deviation 0.05) all fail; around 1000 (deviation 1) E[x^2] - mean^2 = 1 +- 0.06, and a row
        # whose roundings happen to cancel gets through: more than half fail
        low = x[rows].mean(-1) < 0
        print('one-pass rows caught:', float(failed.double().mean()))
        return bool(failed[low].all()) and float(failed[~low].double().mean()) > 0.5
    for dt in (F16, BF16):
        if how == 'unbiased' and width == 2048:
            continue                      # 1 / (2 w) = 2.4e-4 is below half a 16-bit ulp: only the pair bound sees it
        over = (got.to(dt).double() - want).abs() - ref.bound16(want, e, dt)
        assert caught((over[rows] > 0).any(-1)), (how, dt)
    over = (got.double() - want).abs() - ref.bound_pair(want, e, F16, F16)
    assert caught((over[rows] > 0).any(-1)), how


def test_broken_statistics_and_merges_are_rejected():
    x32, kinds = ref.ln_rows(1021, 512, 0)
    x = x32.half()
    want = ref.row_stats64(x, 1e-5)
    bound = ref.stats_bound(want, x.double().abs().amax(-1), kinds)
    assert ref.excess(ref.row_stats32(x, 1e-5), want, ref.stats_bound(want, x.double().abs().amax(-1), kinds, factor=1.0)) <= 0
    # a one-pass variance in the statistics kernel: lost on the large-mean rows
    xf = x.float()
    mean = ref.tree_sum32(xf) / 512
    var = (ref.tree_sum32(xf * xf) / 512 - mean * mean).clamp(min=0)
    one_pass = 1 / torch.sqrt(var + 1e-5)
    over = (one_pass.double() - want[:, 0]).abs() - bound[:, 0]
    assert bool((over[kinds == ref.LARGE_MEAN] > 0).all())
    # the merge: without its clamp NaN on constant rows; with eps ignored the near-epsilon rows fail
    sums, kinds = ref.merge_sums(1000, 16, F16, 0)
    want, cond, absum = ref.merge64(sums, 1024, 1e-3)
    assert ref.excess(ref.merge32(sums, 1024, 1e-3)[0], want, ref.merge_bound(want, cond, absum, factor=1.0)) <= 0
    assert ref.excess(ref.merge32(sums, 1024, 1e-5, clamp=False)[0], ref.merge64(sums, 1024, 1e-5)[0],
                      ref.merge_bound(*ref.merge64(sums, 1024, 1e-5))) == float('inf')
    wrong = ref.merge32(sums, 1024, 1e-5)[0]
    over = (wrong.double() - want).abs() - ref.merge_bound(want, cond, absum)
    assert bool((over[kinds == ref.NEAR_EPS, 0] > 0).all())
    # constant rows: 1 / sqrt(eps) within the bound
    const = kinds == ref.CONSTANT
    assert bool((((want[const, 0] - 1e-3 ** -0.5).abs() - ref.merge_bound(want, cond, absum)[const, 0]) <= 0).all())


def test_broken_gelu_is_rejected():
    """QuickGELU with the constant of GELU's tanh form's sigmoid approximation left at 1.7, and the plain split passed off
    as the activation."""
    x = ref.split_input(1028)
    want = ref.gelu64(x)
    assert ref.excess(ref.gelu32(x), want, ref.gelu_e(x, want, factor=1.0)) <= 0
    wrong = x / (1 + torch.exp(-1.7 * x))
    bound = ref.bound_pair(want, ref.gelu_e(x, want), F16, F16)
    assert ref.excess(wrong, want, bound) > 0 and ref.excess(x, want, bound) > 0


def test_embedding_builders():
    for n_img, seq in ref.EMBED_SHAPES:
        patch, cls, pos = ref.embed_inputs(n_img, seq, 260)
        assert patch.shape == (n_img * (seq - 1), 260) and len(torch.unique(patch[:, 0])) == len(patch)
        pre = ref.embed_sum(patch, cls, pos, n_img, seq).view(n_img, seq, 260)
        assert torch.equal(pre[:, 0], (cls + pos[0]).expand(n_img, 260))             # the class row, in every image
        assert torch.equal(pre[n_img - 1, seq - 1], patch[n_img * (seq - 1) - 1] + pos[seq - 1])
    for ctx in ref.TEXT_CTX:
        tok, table, pos = ref.text_inputs(7, ctx, 8)
        assert {-5, 0, ref.TEXT_VOCAB - 1, ref.TEXT_VOCAB, ref.TEXT_VOCAB + 7} <= set(tok.flatten().tolist())
        out = ref.text_embed_ref(tok, table, pos)
        where = (tok.flatten() == ref.TEXT_VOCAB + 7).nonzero()[0, 0]
        assert torch.equal(out.view(-1, 8)[where], table[-1] + pos[where % ctx])
