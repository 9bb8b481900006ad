"""The yardsticks of tests/gemm_ref.py, checked on the CPU.

* The constants of the bounds are MEASURED here: the fp32 restatement (product32 and the epilogues' fp32 operations) against
  float64 over the random inputs the GPU tests use -- every row of the base arrays all their operands are rows of, at every
  K_total up to 576; beyond, up to K = 4096, every base row of A against the first 272 rows of W -- and must lie at or below
  the recorded figure and within 1.5 x of it.
* The exact family keeps its magnitude promise at every shape of the tables, and its fp32 product has the same bits in any
  K order.
* Planted faults: a float64 tile model of the launch (256 x 256 output tiles, K tiles of 64, workgroup b walking tiles
  b, b + grid, ...) takes a named fault; gemm_ref.verify -- the function the GPU tests call -- must reject the model's
  faulty output and accept the fault-free restatement, on the exact and on the random inputs."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as ref  # noqa: E402
import rowops_ref as rr  # noqa: E402

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------------------------------------------
# constants
# ---------------------------------------------------------------------------------------------------------------
def _ratio(got, want, scale):
    return float(((got.double() - want).abs() / (ref.EPS24 * scale)).max())


def _acc_epilogues(acc32, acc64, S, bias, M, N):
    """Worst error of the fp32-level epilogues (acc + bias; + resid; + (hi + lo)) in units of 2^-24 S."""
    b32, b64 = bias[None], bias.double()[None]
    v32, v64, s = acc32 + b32, acc64 + b64, S + b64.abs()
    worst = _ratio(v32, v64, s)
    resid = ref.random_plane(M, N, 1)
    worst = max(worst, _ratio(v32 + resid, v64 + resid.double(), s + resid.double().abs()))
    hi, lo = ref.split(ref.random_plane(M, N, 2), F16, F16)
    return max(worst, _ratio((hi.float() + lo.float()) + v32, v64 + hi.double() + lo.double(),
                             s + hi.double().abs() + lo.double().abs()))


@functools.lru_cache(maxsize=None)
def measured_acc():
    """-> {bound of K_total: worst c}.  Up to 576: single products at every K tile count up to 9 and the segmented products
    (16-bit and e4m3 parts) at K = 64, 128, 192 per segment, over the whole base arrays.  Up to 4096, over every base row of A
    and the first DEEP_N rows of W: every prefix of K tiles up to 64 (the K-batched form, gemm_rows' batches from row 0),
    every single K tile on its own (the batches of the K splits and of gemm_rows lie at a column offset), and the e4m3
    segments at K = 256 and 384 per segment (K_total up to 1152)."""
    a, w, bias = ref._random_base()
    M, N = ref.PERIOD_M, ref.PERIOD_N
    small = 0.0
    for dt in (F16, BF16):
        A, W = a[:, :576].to(dt), w[:, :576].to(dt)
        acc32, acc64, S = None, 0, 0
        for kt in range(9):
            ks = slice(64 * kt, 64 * kt + 64)
            blk = ref.product32([(A[:, ks], W[:, ks])])
            acc32 = blk if acc32 is None else acc32 + blk
            p, s = ref.product([(A[:, ks], W[:, ks])])
            acc64, S = acc64 + p, S + s
            small = max(small, _acc_epilogues(acc32, acc64, S, bias, M, N))
        for K in (64, 128, 192):
            for seg in ref.SEGS16 + (ref.SEGS8 if dt == F16 else ()):
                c = ref.make_case('store32', dt, M, N, K, 'random', seg=seg)
                segs = ref.case_segments(c)
                p, s = ref.product(segs)
                small = max(small, _acc_epilogues(ref.product32(segs), p, s, bias, M, N))
    large, nd = 0.0, DEEP_N
    for dt in (F16, BF16):
        A, W = a.to(dt), w[:nd].to(dt)
        acc32, acc64, S = None, 0, 0
        for kt in range(ref.KMAX // 64):
            ks = slice(64 * kt, 64 * kt + 64)
            blk = ref.product32([(A[:, ks], W[:, ks])])
            acc32 = blk if acc32 is None else acc32 + blk
            p, s = ref.product([(A[:, ks], W[:, ks])])
            acc64, S = acc64 + p, S + s
            large = max(large, _acc_epilogues(acc32, acc64, S, bias[:nd], M, nd), _acc_epilogues(blk, p, s, bias[:nd], M, nd))
    for K in (256, 384):
        for seg in ref.SEGS8:
            c = ref.make_case('store32', F16, M, nd, K, 'random', seg=seg)
            segs = ref.case_segments(c)
            p, s = ref.product(segs)
            large = max(large, _acc_epilogues(ref.product32(segs), p, s, bias[:nd], M, nd))
    return {576: small, 4096: max(small, large)}


DEEP_N = 272     # columns of W in the deep-K measurements: the widest shape of the e4m3 K loop; the K-batched form, the K splits
#                  and gemm_rows go on to 1024, with rows of W that are draws of the same distribution


def test_e4m3_lo_byte_is_within_its_rounding_bound():
    """The bound of the e4m3 lo output has no measured constant: with E = 0 and the restatement's own fp32 value as the
    reference, restate()'s byte must meet it as it stands."""
    for K in (128, 256):
        for seg in ('a_lo8', 'both8'):
            c = ref.make_case('gelu16', F16, 257, 272, K, 'random', seg=seg, lo_out='e4m3')
            ref.case_specs(c)                # (sets aux_exp)
            exp = c['aux_exp']
            v32 = rr.gelu32(ref.product32(ref.case_segments(c)) + c['bias'][None])
            got = ref.case_restate(c)
            lo = v32.double() - got['out'].double()
            assert float(lo.abs().max()) * 2.0 ** exp <= 448
            over = ref.excess(got['aux8'], lo, 2.0 ** -4 * lo.abs() + 2.0 ** (-10 - exp))
            assert over <= 0, (K, seg, over)


@functools.lru_cache(maxsize=None)
def measured_fold():
    """The LN fold on the SAME fp32 accumulator, in units of 2^-24 S_ln."""
    worst = 0.0
    for dt in (F16, BF16):
        for K in (64, 128, 320):
            c = ref.make_case('store16_ln', dt, ref.PERIOD_M, ref.PERIOD_N, K, 'random')
            acc32 = ref.product32(ref.case_segments(c))
            _, S = ref.product(ref.case_segments(c))
            st, cs, b = c['stats'].double(), c['colsum'].double()[None], c['bias'].double()[None]
            want = st[:, :1] * acc32.double() + st[:, 1:] * cs + b
            s_ln = st[:, :1].abs() * S + (st[:, 1:] * cs).abs() + b.abs()
            got = acc32 * c['stats'][:, :1] + (c['colsum'][None] * c['stats'][:, 1:] + c['bias'][None])
            worst = max(worst, _ratio(got, want, s_ln))
    return worst


@functools.lru_cache(maxsize=None)
def measured_grad():
    worst = 0.0
    tails = torch.tensor(ref.GELU_TAILS)
    for dt in (F16, BF16):
        for x in (ref.random_plane(ref.PERIOD_M, 1040, 3, 1.5).to(dt).float(), tails.to(dt).float()):
            d = x.double()
            s = 1 / (1 + torch.exp(-1.702 * d))
            scale = rr.EPS32 * s * (1 + (1.702 * d).abs()) ** 2
            err = ((ref.grad32(x).double() - ref.grad64(x)).abs() - rr.FLOOR_GELU).clamp(min=0)
            worst = max(worst, float((err / scale).max()))
    return worst


@functools.lru_cache(maxsize=None)
def measured_rowsum():
    worst = 0.0
    for dt in (F16, BF16):
        for seed in (1, 2):
            h = ref.random_plane(ref.PERIOD_M, 1088, seed).to(dt).float().view(ref.PERIOD_M, 17, 64)
            d = h.double()
            worst = max(worst, _ratio(ref.seq_sum32(h), d.sum(-1), d.abs().sum(-1)),
                        _ratio(ref.seq_sum32(h * h), (d * d).sum(-1), (d * d).sum(-1)))
    return worst


def _report(name, measured, recorded):
    print(f'{name:28s} measured {measured:8.3f}   recorded {recorded:8.3f}')
    assert measured <= recorded, f'{name}: measured {measured} above the recorded {recorded}'
    assert recorded <= 1.5 * measured, f'{name}: the recorded {recorded} is stale (measured {measured})'


def test_constants_are_the_measured_ones():
    acc = measured_acc()
    for k, c in ref.C_ACC_TABLE:
        _report(f'C_ACC (K_total <= {k})', acc[k], c)
    _report('C_FOLD', measured_fold(), ref.C_FOLD)
    _report('C_GRAD', measured_grad(), ref.C_GRAD)
    _report('C_ROWSUM', measured_rowsum(), ref.C_ROWSUM)
    assert ref.KERNEL_FACTOR == rr.KERNEL_FACTOR == 4.0


def test_largest_slope_of_quickgelu():
    x = torch.linspace(-10, 10, 200001, dtype=torch.float64)
    assert float(ref.grad64(x).abs().max()) <= ref.GELU_SLOPE


# ---------------------------------------------------------------------------------------------------------------
# exact family
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [F16, BF16])
def test_exact_family_keeps_its_magnitudes(dt):
    shapes = [(M, N, 128) for M in ref.EDGE_M for N in ref.EDGE_N] + [(257, 272, 64 * nk) for nk in ref.NK]
    shapes += [(M, N, 64 * nk) for M, N in ref.WS_SHAPES for nk in ref.WS_NK]
    for epi in ('store16', 'store32', 'resid_hl', 'resid32'):
        limit = ref.exact_limit(epi, dt)
        for M, N, K in shapes:
            A, W, bias = ref.exact_operands(M, N, K, limit, extra=10)
            assert bool((W != 0).all()) and bool((A != 0).any(1).all())
            for x in (A, W):
                assert torch.equal(x.to(dt).float(), x)
            s = A.abs() @ W.abs().T + bias.abs()[None] + 10
            assert float(s.max()) <= limit, (epi, M, N, K, float(s.max()))
    # no two rows, no two columns, no two K tiles alike (one K tile of one nonzero among 64 cannot tell 513 rows apart:
    # there, the rows a fault can confuse -- 16 apart, a tile apart -- differ)
    for limit in (256, 2048, 2 ** 24 - 1):
        A, W, _ = ref.exact_operands(513, 528, 320, limit)
        assert len({tuple(r.tolist()) for r in A}) == 513 and len({tuple(r.tolist()) for r in W}) == 528
        for x in (A, W):
            kt = [x[:, 64 * t:64 * t + 64] for t in range(5)]
            assert not any(torch.equal(kt[i], kt[j]) for i in range(5) for j in range(i))
        A, W, _ = ref.exact_operands(513, 528, 64, limit)
        for d in (16, 256):
            assert bool((A[d:] != A[:-d]).any(1).all()) and bool((W[d:] != W[:-d]).any(1).all())
    for seg, nseg in (('both', 3), ('both8', 3)):
        if dt == BF16 and seg == 'both8':
            continue
        for K in (128, 256, 384):
            c = ref.make_case('store16', dt, 257, 272, K, 'exact', seg=seg)
            _, s = ref.product(ref.case_segments(c))
            assert float(s.max()) + 14 <= c['limit']


@pytest.mark.parametrize('dt', [F16, BF16])
def test_exact_family_has_the_same_bits_in_any_k_order(dt):
    g = torch.Generator().manual_seed(5)
    for epi in ('store16', 'store32'):
        for seg in (None, 'both'):
            c = ref.make_case(epi, dt, 129, 80, 192, 'exact', seg=seg)
            acc, _ = ref.product(ref.case_segments(c))
            base = ref.product32(ref.case_segments(c))
            assert torch.equal(base.double(), acc)
            for _ in range(3):
                assert torch.equal(_bits(ref.product32(ref.case_segments(c), torch.randperm(192, generator=g))), _bits(base))


def _bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------
FAULTS = {
    # fault: the (epilogue, seg, row_sums) launches it is planted in
    'k_tile_dropped': [('store16', None, False), ('store32', None, False)],
    'k_tile_twice': [('store16', None, False), ('store32', None, False)],
    'stale_first_k_tile': [('store16', None, False), ('store32', None, False)],
    'row_groups_swapped': [('store16', None, False), ('gelu16', None, False)],
    'col_groups_swapped': [('store16', None, False), ('gelu_bwd16', None, False)],
    'bias_of_neighbour_group': [('store16', None, False), ('store16_ln', None, False)],
    'stats_of_other_slot': [('store16_ln', None, False), ('gelu16_ln', None, False)],
    'last_tile_never_visited': [('store16', None, False), ('resid32', None, False)],
    'tile_visited_twice': [('resid32', None, False), ('resid_hl', None, False)],
    'segment_hi_for_lo': [('store32', 'a_lo', False), ('store32', 'a_lo8', False), ('store16', 'w_lo', False)],
    'guard_row_written': [('store16', None, False), ('resid_hl', None, False)],
    'padding_column_written': [('store32', None, False), ('gelu16_save', None, False)],
    'row_sums_past_last_group': [('resid_hl', None, True)],
}
MODEL_SHAPE = (257, 320, 128)     # 2 x 2 tiles, partial in both directions, N % 64 == 0, N % 256 != 0; two K tiles
MODEL_GRID = 2                    # so that every workgroup runs a second tile


def _pad_rows(x, rows, n):
    """rows `rows` of x, zeros where they do not exist (what a range-checked load returns), n of them."""
    out = torch.zeros((n,) + tuple(x.shape[1:]), dtype=x.dtype)
    r = rows[rows < x.shape[0]]
    out[:len(r)] = x[r]
    return out


def tile_model(c, bufs, fault=None, grid=MODEL_GRID):
    """Writes the launch's result into bufs (gemm_ref.case_buffers), tile by tile."""
    M, N, K, epi, dtype = c['M'], c['N'], c['K'], c['epi'], c['dtype']
    segs = [(a.double(), w.double()) for a, w in ref.case_segments(c)]
    if fault == 'segment_hi_for_lo':
        a0, w0 = segs[0]
        segs[0] = (c['A'].double(), w0) if c['seg'].startswith('a_lo') else (a0, c['W'].double())
    ktiles = [(s, kt) for s in range(len(segs)) for kt in range(segs[s][0].shape[1] // 64)]
    tiles_n = (N + 255) // 256
    ntiles = ((M + 255) // 256) * tiles_n
    out, aux = bufs['out'][1], bufs.get('aux', (None, None))[1]
    for b in range(min(grid, ntiles)):
        prev = None
        for tid in range(b, ntiles, grid):
            rows = torch.arange(256) + 256 * (tid // tiles_n)
            cols = torch.arange(256) + 256 * (tid % tiles_n)
            if fault == 'last_tile_never_visited' and tid == ntiles - 1:
                continue
            acc = torch.zeros(256, 256, dtype=torch.float64)
            order = list(ktiles)
            if fault == 'k_tile_dropped':
                order = order[:-1]
            if fault == 'k_tile_twice':
                order = order[:1] + order
            for i, (s, kt) in enumerate(order):
                ks = slice(64 * kt, 64 * kt + 64)
                r, cc = (prev if fault == 'stale_first_k_tile' and i == 0 and prev is not None else (rows, cols))
                acc += _pad_rows(segs[s][0][:, ks], r, 256) @ _pad_rows(segs[s][1][:, ks], cc, 256).T
            if fault == 'row_groups_swapped':
                acc[:32] = torch.cat([acc[16:32], acc[:16]])
            if fault == 'col_groups_swapped':
                acc[:, :32] = torch.cat([acc[:, 16:32], acc[:, :16]], 1)
            bcols = (cols + 16) if fault == 'bias_of_neighbour_group' else cols
            srows = prev[0] if fault == 'stats_of_other_slot' and prev is not None else rows
            mr, mc = rows[rows < M], cols[cols < N]
            nr, nc = len(mr), len(mc)

            def tile(x):
                return None if x is None else x[mr][:, mc].clone()
            for _ in range(2 if fault == 'tile_visited_twice' and tid == 0 else 1):
                got = ref.restate(epi, dtype, acc[:nr, :nc].float(), _pad_rows(c['bias'], bcols, 256)[:nc],
                                  tile(out) if epi == 'resid32' else tile(c.get('resid')),
                                  tile(out) if epi == 'resid_hl' else None, tile(aux) if epi == 'resid_hl' else None,
                                  tile(c.get('u')),
                                  None if 'stats' not in c else _pad_rows(c['stats'], srows, 256)[:nr],
                                  None if 'colsum' not in c else _pad_rows(c['colsum'], bcols, 256)[:nc],
                                  c['lo_out'], c['aux_exp'])
                out[mr[0]:mr[0] + nr, mc[0]:mc[0] + nc] = got['out']
                if 'aux' in got:
                    aux[mr[0]:mr[0] + nr, mc[0]:mc[0] + nc] = got['aux']
                if 'aux8' in got:
                    q = (got['aux8'] * 2.0 ** c['aux_exp']).float().to(torch.float8_e4m3fn).view(torch.uint8)
                    bufs['aux8'][1][mr[0]:mr[0] + nr, mc[0]:mc[0] + nc] = q
            if 'row_sums' in bufs:
                h = out[mr[0]:mr[0] + nr, mc[0]:mc[0] + nc].float().view(nr, nc // 64, 64)
                sums = torch.stack([ref.seq_sum32(h), ref.seq_sum32(h * h)], -1)
                g0 = int(mc[0]) // 64
                bufs['row_sums'][1][mr[0]:mr[0] + nr, g0:g0 + nc // 64] = sums
                if fault == 'row_sums_past_last_group' and nc < 256:
                    flat = bufs['row_sums'][0].view(-1, 2)          # group N / 64 of row m IS group 0 of row m + 1
                    flat[(mr + 1) * (N // 64)] = sums[:, -1]
            prev = (rows, cols)
    if fault == 'guard_row_written':
        bufs['out'][0][M, :N] = bufs['out'][0][M - 1, :N]
    if fault == 'padding_column_written':
        name = 'aux' if 'aux' in bufs else 'out'
        bufs[name][0][M - 1, N] = 0


def _run(epi, dt, family, seg, row_sums, fault, restated=False):
    M, N, K = MODEL_SHAPE
    c = ref.make_case(epi, dt, M, N, K, family, seg=seg)
    specs = ref.case_specs(c)
    bufs = ref.case_buffers(c, row_sums=row_sums)
    if restated:
        got = ref.case_restate(c)
        for k, v in got.items():
            bufs[k][1].copy_(v)
        if row_sums:
            h = got['out'].float().view(M, N // 64, 64)
            bufs['row_sums'][1].copy_(torch.stack([ref.seq_sum32(h), ref.seq_sum32(h * h)], -1))
    else:
        tile_model(c, bufs, fault)
    ref.verify(c, specs, bufs, f'{epi} {dt} {family} {fault}')


@pytest.mark.parametrize('fault', list(FAULTS))
def test_planted_faults_are_caught(fault):
    for epi, seg, row_sums in FAULTS[fault]:
        for dt in (F16, BF16):
            if seg in ref.SEGS8 and dt == BF16:
                continue
            for family in ('exact', 'random'):
                _run(epi, dt, family, seg, row_sums, None, restated=True)      # the fault-free restatement passes
                _run(epi, dt, family, seg, row_sums, None)                     # ... and so does the model without a fault
                with pytest.raises(AssertionError):
                    _run(epi, dt, family, seg, row_sums, fault)
                print(f'{fault:28s} {epi:12s} {str(seg):6s} {str(dt)[6:]:9s} {family:7s} caught; fault-free restatement passes')
