"""ops.gemm and ops.gemm_rows at every tile, K-loop and hand-over edge of csrc/gemm.hip, against float64 or bit-exact
expectations: tests/gemm_ref.py holds the references, the directed inputs (an exact small-integer family, a random family
with outlier, cancelling and zero rows, the GELU tails) and the per-element bounds, whose constants are measured in
tests/test_gemm_ref_cpu.py; the kernels get four times the fp32 restatement's accumulation error.

Buffer conventions, in every case (gemm_ref.case_buffers / window): out, aux, aux8, the planes and an out-of-place residual
are views [M, N] of NaN-filled buffers [M + 1, N + 64] (0xAA for e4m3), inputs the kernel updates copied in; padding columns
and the guard row must come back bit for bit and nothing inside may be NaN.  A and W are column windows of wider NaN-filled
buffers (lda = ldw = K + 64), row_sums is NaN-filled with a guard row, row statistics end in a NaN pair."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as ref  # noqa: E402
import rowops_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT = ref.DTYPES
NAN = float('nan')

# a mode = an epilogue of gemm_ref.EPILOGUES with what the launch adds: row_sums, the statistics' stride, segments, a lo output
MODES = {e: dict(epi=e) for e in ref.EPILOGUES if not e.endswith('_ln')}
MODES['resid_hl+sums'] = dict(epi='resid_hl', sums=True)
for _e in ('store16_ln', 'gelu16_ln'):
    for _s in (1, 5):                      # 1: the LDS path (DMA into the side area); 5: the global path
        MODES[f'{_e}@{_s}'] = dict(epi=_e, stride=_s)
SEG_MODES = {}
for _seg in ref.SEGS16:
    for _e in ref.SEG_EPILOGUES:
        SEG_MODES[f'{_e}/{_seg}'] = dict(epi=_e, seg=_seg)
    for _e in ('store16', 'gelu16'):
        SEG_MODES[f'{_e}+lo16/{_seg}'] = dict(epi=_e, seg=_seg, lo_out='16')
F8_MODES = {}
for _seg in ref.SEGS8:
    for _e in ref.F8_EPILOGUES:
        F8_MODES[f'{_e}/{_seg}'] = dict(epi=_e, seg=_seg)
    F8_MODES[f'store16+lo16/{_seg}'] = dict(epi='store16', seg=_seg, lo_out='16')
    F8_MODES[f'gelu16+lo16/{_seg}'] = dict(epi='gelu16', seg=_seg, lo_out='16')
    if _seg != 'w_lo8':                    # (the e4m3 lo output goes with A_lo8: ec_gemm refuses it without)
        F8_MODES[f'gelu16+e4m3/{_seg}'] = dict(epi='gelu16', seg=_seg, lo_out='e4m3')


def _ops():
    from eventclip_amd import ops
    return ops


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(mode, dt, M, N, K, family, rot=0):
    c = ref.make_case(mode['epi'], dt, M, N, K, family, rot, mode.get('seg'), mode.get('lo_out'))
    return ref.case_to(c, 'cuda')


def _stats_array(pairs, stride):
    """[M, 2] -> what the launch is handed: M pairs and a NaN pair behind them (stride 1), or every stride-th pair of a
    NaN-interleaved array."""
    M = pairs.shape[0]
    buf = torch.full((M + 1, stride, 2), NAN, dtype=F32, device=pairs.device)
    buf[:M, 0] = pairs
    return buf.view(-1)[:((M - 1) * stride + 1) * 2]


def _launch(c, mode, ws=None, lead=64):
    """One ops.gemm launch of the case into fresh buffers -> bufs."""
    bufs = ref.case_buffers(c, 'cuda', row_sums=mode.get('sums', False))
    epi = c['epi']
    kw = {}
    if epi == 'resid32_oop':
        kw['resid'] = bufs['resid'][1]
    if 'aux' in bufs:
        kw['aux'] = bufs['aux'][1]
    if 'aux8' in bufs:
        kw['aux8'] = (bufs['aux8'][1], c['aux_exp'])
    if 'row_sums' in bufs:
        kw['row_sums'] = bufs['row_sums'][1]
    if epi.endswith('_ln'):
        stride = mode.get('stride', 1)
        kw.update(row_stats=_stats_array(c['stats'], stride), col_sums=c['colsum'], row_stats_stride=stride)
    for k in ('A_lo', 'W_lo'):
        if k in c:
            kw[k] = ref.window(c[k], lead=lead if k == 'A_lo' else 64 - lead)
    for k in ('A_lo8', 'W8', 'A8', 'W_lo8'):
        if k in c:
            kw[k] = c[k]
    _ops().gemm(ref.window(c['A'], lead=lead), ref.window(c['W'], lead=64 - lead), c['bias'], epi.replace('_oop', ''),
                out=bufs['out'][1], ws=ws, **kw)
    return bufs


def _merge_check(c, bufs, what):
    """The group sums the launch wrote give, through ops.row_stats_merge, the statistics of the hi plane it wrote."""
    sums = bufs['row_sums'][1]
    got = _ops().row_stats_merge(sums, c['N'], ref.LN_EPS)
    want, cond, absum = rr.merge64(sums, c['N'], ref.LN_EPS)
    over = rr.excess(got, want, rr.merge_bound(want, cond, absum))
    assert over <= 0, f'{what}: merged statistics {over:.3e} over the bound'


def _run(c, mode, what, acc_s=None, twice=False, ws=None):
    specs = ref.case_specs(c, acc_s)
    bufs = _launch(c, mode, ws)
    ref.verify(c, specs, bufs, what)
    if 'row_sums' in bufs:
        _merge_check(c, bufs, what)
    if twice:
        again = _launch(c, mode, ws)
        _same_bits(bufs, again, what + ': second launch')
    return bufs


def _same_bits(a, b, what, rows=None):
    for name in a:
        x, y = a[name][1], b[name][1]
        if rows is not None:
            x = x[rows[0]:rows[1]]
        assert torch.equal(ref._bits(x), ref._bits(y)), f'{what}: {name} differs in {int((ref._bits(x) != ref._bits(y)).sum())} elements'


def _sums_ok(mode, N):
    return not mode.get('sums') or N % 64 == 0


# ---------------------------------------------------------------------------------------------------------------
# 1. tile edges: every M x every N at K = 128
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('mode', list(MODES))
def test_tile_edges(mode, dt, hip):
    """Smallest shape that reaches the code: M = 1 (one row of one row group), N = 16 (one column group); N = 272 leaves a
    last tile of one group, N = 64, 192, 320 the row_sums of a partial tile."""
    mode, dt = MODES[mode], DT[dt]
    Mx, Nx, K = max(ref.EDGE_M), max(ref.EDGE_N), 128
    for family in ('exact', 'random'):
        full = _case(mode, dt, Mx, Nx, K, family)
        acc, S = ref.product(ref.case_segments(full))
        for M in ref.EDGE_M:
            for N in ref.EDGE_N:
                if _sums_ok(mode, N):
                    _run(ref.slice_case(full, 0, M, N), mode, f'{family} M={M} N={N}', (acc[:M, :N], S[:M, :N]))
    for M in (m for m in ref.EDGE_M if len(ref.rotations(m)) > 1):       # too few rows for every kind: the other rotations
        for rot in ref.rotations(M)[1:]:
            full = _case(mode, dt, M, Nx, K, 'random', rot)
            for N in ref.EDGE_N:
                if _sums_ok(mode, N):
                    _run(ref.slice_case(full, 0, M, N), mode, f'random rot={rot} M={M} N={N}')
    if 'gelu' in mode['epi']:
        full = _case(mode, dt, Mx, Nx, K, 'tails')
        acc, S = ref.product(ref.case_segments(full))
        cold = (ref.tails_bias(Nx) <= -60).to('cuda')
        for M in ref.EDGE_M:
            for N in ref.EDGE_N:
                bufs = _run(ref.slice_case(full, 0, M, N), mode, f'tails M={M} N={N}', (acc[:M, :N], S[:M, :N]))
                # where exp2 overflows (1.702 x 60 > 88.7) the output is zero or tiny, never NaN or the input
                assert float(bufs['out'][1][:, cold[:N]].float().abs().max()) <= 2.0 ** -24, f'tails M={M} N={N}'


# ---------------------------------------------------------------------------------------------------------------
# 2. K loop: nk = 1 (EC_VMCNT(2), nothing carried), 2 and 3 (has1 / has2 change inside the first tile), 4, 5
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('mode', list(MODES))
def test_k_loop(mode, dt, hip):
    mode, dt = MODES[mode], DT[dt]
    M, N = 257, 272
    for nk in ref.NK:
        for family in ('exact', 'random'):
            if _sums_ok(mode, N):
                _run(_case(mode, dt, M, N, 64 * nk, family), mode, f'{family} K={64 * nk}')
    _run(dict(_case(mode, dt, M, 320 if mode.get('sums') else N, 128, 'random'), bias=None), mode, 'random, no bias')
    if mode.get('sums'):
        for nk in ref.NK:                  # (272 % 64 != 0: the sums at the nearest N that has them)
            for family in ('exact', 'random'):
                _run(_case(mode, dt, M, 320, 64 * nk, family), mode, f'{family} N=320 K={64 * nk}')


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('mode', list(SEG_MODES))
def test_k_loop_segmented(mode, dt, hip):
    """A_lo, W_lo and both (nseg 2 and 3) at one, two and three K tiles per segment."""
    mode, dt = SEG_MODES[mode], DT[dt]
    for nk in (1, 2, 3):
        for family in ('exact', 'random'):
            _run(_case(mode, dt, 257, 272, 64 * nk, family), mode, f'{family} K={64 * nk}')


@pytest.mark.parametrize('mode', list(F8_MODES))
def test_k_loop_e4m3(mode, hip):
    """The e4m3 lo products (f16): one, two and three 128-deep K tiles per e4m3 segment in front of the 16-bit ones."""
    mode = F8_MODES[mode]
    for nk in (1, 2, 3):
        for family in ('exact', 'random'):
            _run(_case(mode, F16, 257, 272, 128 * nk, family), mode, f'{family} K={128 * nk}')


# ---------------------------------------------------------------------------------------------------------------
# 3. hand-over: T = 2 CUs + 3 tiles, some workgroups run three tiles and some two
# ---------------------------------------------------------------------------------------------------------------
def _tilings():
    T = 2 * _cus() + 3
    return {'tiles_n=1': (256 * (T - 1) + 77, 240),
            'tiles_n=4': (256 * ((T + 3) // 4 - 1) + 77, 784),       # the grouped raster and its remainder rows
            'tiles_n=5': (256 * ((T + 4) // 5 - 1) + 77, 1040)}      # the N-fastest raster


SUMS_N = {240: 192, 784: 832, 1040: 1088}      # row_sums needs N % 64 == 0: the same tilings, the last tile 192 / 64 / 64 wide
HAND_OVER_MODES = dict(MODES)
HAND_OVER_MODES['store16+lo16/both'] = SEG_MODES['store16+lo16/both']
HAND_OVER_MODES['gelu16+e4m3/both8'] = F8_MODES['gelu16+e4m3/both8']


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('K', [64, 128, 192])
@pytest.mark.parametrize('tiling', ['tiles_n=1', 'tiles_n=4', 'tiles_n=5'])
def test_hand_over(tiling, K, dt, hip):
    """Every epilogue's next_tile(), the counted vmcnt(TAIL) wait and, for the LN epilogues, the alternation of the two
    statistics slots with the statistics DMA in flight; K = 64 hands over with nothing carried.  Each launch runs twice: a
    race shows as a difference before it shows as an error."""
    dt = DT[dt]
    M, N = _tilings()[tiling]
    for family in ('exact', 'random'):
        shared = {}            # the operands on the device and their float64 product, once per (magnitude limit, segments)
        for name, mode in HAND_OVER_MODES.items():
            seg = mode.get('seg')
            if seg in ref.SEGS8 and (dt != F16 or K % 128):
                continue
            n = SUMS_N[N] if mode.get('sums') else N
            key = (ref.exact_limit(mode['epi'], dt) if family == 'exact' else 0, seg, n)
            if key not in shared:
                base = _case(mode, dt, M, n, K, family)
                shared[key] = (base, ref.product(ref.case_segments(base)))
            base, acc_s = shared[key]
            _run(ref.with_epilogue(base, mode['epi'], mode.get('lo_out')), mode, f'{family} {name}', acc_s, twice=True)
        del shared, base, acc_s
        torch.cuda.empty_cache()


@pytest.mark.parametrize('dt', list(DT))
def test_hand_over_k_splits(dt, hip):
    """splits = 32 of K = 64 at M = 513, N = 528: 9 x 32 tiles, each batch a tile range of the same launch."""
    dt = DT[dt]
    M, N, K, splits = 513, 528, 64, 32
    for family in ('exact', 'random'):
        if family == 'exact':
            a, w, _ = ref.exact_operands(M, N, K * splits, 2 ** 24 - 1)
        else:
            a, w, _ = ref.random_operands(M, N, K * splits)
        A, W = a.to(dt).cuda(), w.to(dt).cuda()
        runs = []
        for _ in range(2):
            buf = torch.full((splits, M + 1, N + ref.PAD), NAN, dtype=F32, device='cuda')
            _ops().gemm(ref.window(A), ref.window(W, lead=64), None, 'store32', out=buf[:, :M, :N], splits=splits)
            runs.append(buf)
        assert torch.equal(ref._bits(runs[0]), ref._bits(runs[1])), 'second launch differs'
        for s in range(splits):
            ks = slice(s * K, s * K + K)
            acc, S = ref.product([(A[:, ks], W[:, ks])])
            ref.guards_intact(runs[0][s], M, N, f'{family} batch {s}')
            ref.check(ref.expect('store32', dt, acc, S, K, exact=family == 'exact'), {'out': runs[0][s, :M, :N]}, f'{family} batch {s}')


# ---------------------------------------------------------------------------------------------------------------
# 7. (and the many-tiles case of 3) transposed operands
# ---------------------------------------------------------------------------------------------------------------
def _rows_case(dt, rows, M, N, splits, family):
    """-> (A [rows, M], W [rows, N]) as the first rows of taller NaN buffers with NaN padding columns, K per batch."""
    K = ((rows + splits - 1) // splits + 63) // 64 * 64
    kp = (rows + 63) // 64 * 64
    if family == 'exact':
        a, w, _ = ref.exact_operands(M, N, kp, 2 ** 24 - 1)
    else:
        a, w, _ = ref.random_operands(M, N, kp)
    A = ref.window(a[:, :rows].T.contiguous().to(dt).cuda(), extra_rows=8)
    W = ref.window(w[:, :rows].T.contiguous().to(dt).cuda(), lead=64, extra_rows=8)
    return A, W, K


def _rows_run(dt, rows, M, N, splits, family, twice=False):
    A, W, K = _rows_case(dt, rows, M, N, splits, family)
    what = f'{family} rows={rows} M={M} N={N} splits={splits}'
    runs = []
    for _ in range(2 if twice else 1):
        buf = torch.full((splits, M + 1, N + ref.PAD), NAN, dtype=F32, device='cuda')
        _ops().gemm_rows(A, W, splits, out=buf[:, :M, :N] if splits > 1 else buf[0, :M, :N])
        runs.append(buf)
    if twice:
        assert torch.equal(ref._bits(runs[0]), ref._bits(runs[1])), what + ': second launch differs'
    for s in range(splits):
        rs = slice(min(s * K, rows), min(s * K + K, rows))          # a batch wholly past the last row: zeros
        acc, S = ref.product([(A[rs].T, W[rs].T)])
        ref.guards_intact(runs[0][s], M, N, f'{what} batch {s}')
        ref.check(ref.expect('store32', dt, acc, S, max(K, 64), exact=family == 'exact'), {'out': runs[0][s, :M, :N]},
                  f'{what} batch {s}')


@pytest.mark.parametrize('dt', list(DT))
def test_hand_over_transposed(dt, hip):
    """gemm_rows at M = N = 1024 with splits = 40 over 40 x 64 - 7 rows: 640 tiles."""
    for family in ('exact', 'random'):
        _rows_run(DT[dt], 40 * 64 - 7, 1024, 1024, 40, family, twice=True)


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('splits', [1, 2, 3])
def test_transposed_edges(splits, dt, hip):
    """rows = 1 is the smallest (63 of the K tile's 64 rows read the zero block); rows = 65 with splits = 3 leaves a batch
    wholly past the last row."""
    for rows in ref.ROWS_T:
        for M in ref.ROWS_M:
            for N in ref.ROWS_N:
                for family in ('exact', 'random'):
                    _rows_run(DT[dt], rows, M, N, splits, family)


# ---------------------------------------------------------------------------------------------------------------
# 4. raster and XCD remap: every tile visited once
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['resid32', 'resid_hl'])
def test_raster_and_remap_visit_every_tile_once(mode, hip):
    """tiles_m x tiles_n over the grouped raster's condition (tiles_n % 4 == 0 and tiles_m >= 8) and every ntiles & 7; an
    in-place update applied twice, or a tile never visited, is not the exact expectation."""
    mode = MODES[mode]
    for tm in ref.RASTER_TM:
        for tn in ref.RASTER_TN:
            M, N = 256 * (tm - 1) + 77, 256 * (tn - 1) + 48
            _run(_case(mode, F16, M, N, 64, 'exact'), mode, f'tiles {tm} x {tn}')


# ---------------------------------------------------------------------------------------------------------------
# 5. batch invariance
# ---------------------------------------------------------------------------------------------------------------
INVARIANT_MODES = dict(MODES)
INVARIANT_MODES.update({k: SEG_MODES[k] for k in ('store16+lo16/both', 'store32/a_lo', 'resid_hl/w_lo', 'gelu16/both', 'resid32/both')})
INVARIANT_MODES.update({k: F8_MODES[k] for k in ('gelu16+e4m3/both8', 'store16/a_lo8', 'resid_hl/a_lo8+w_lo', 'store32/w_lo8')})


@pytest.mark.parametrize('mode,dt', [(m, d) for m in INVARIANT_MODES for d in DT
                                     if d == 'float16' or INVARIANT_MODES[m].get('seg') not in ref.SEGS8])
def test_batch_invariance(mode, dt, hip):
    """"A row's result cannot depend on which of the two its tile is in this launch": rows [s, s + r) of a launch of
    2 CUs + 3 tiles are, bit for bit, the launch on those rows alone -- a full tile, an interior tile, a piece that straddles
    no boundary of its own and the last row."""
    name, mode, dt = mode, INVARIANT_MODES[mode], DT[dt]
    M, N = _tilings()['tiles_n=1']
    N = 256 if mode.get('sums') else N
    big = _case(mode, dt, M, N, 128, 'random')
    if mode.get('lo_out') == 'e4m3':
        ref.case_specs(big)                # (sets aux_exp)
    whole = _launch(big, mode)
    for s, r in ((0, 256), (256, 256), (300, 77), (M - 1, 1)):
        part = _launch(ref.slice_case(big, s, s + r), mode)
        _same_bits(whole, part, f'{name} rows [{s}, {s + r})', rows=(s, s + r))


# ---------------------------------------------------------------------------------------------------------------
# 6. the K-batched low-latency form
# ---------------------------------------------------------------------------------------------------------------
def _ws_batches(M, N, nk, cus):
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if tiles * 2 > cus:
        return 1
    s = 1
    while s < 16 and tiles * s * 2 <= cus and nk % (2 * s) == 0 and nk // (2 * s) >= 2:
        s *= 2
    return s


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('epi', ref.WS_EPILOGUES)
def test_k_batched_form(epi, dt, hip):
    """Held to float64 at the full K, not to the single-pass bits; a scratch one byte short runs the single pass."""
    mode, dt = MODES[epi], DT[dt]
    for M, N in ref.WS_SHAPES:
        for nk in ref.WS_NK:
            batches = _ws_batches(M, N, nk, _cus())
            ws32 = torch.empty(max(batches * M * N, 4), dtype=F32, device='cuda')
            ws = ws32.view(torch.uint8)
            for family in ('exact', 'random'):
                c = _case(mode, dt, M, N, 64 * nk, family)
                what = f'{family} M={M} N={N} K={64 * nk} ({batches} batches)'
                # that the K-batched path ran (the batch rule above restates try_kbatched's) shows in the scratch: every
                # partial product written, or, where the launch is a single pass, nothing
                ws32.fill_(NAN)
                _run(c, mode, what, ws=ws)
                used = torch.isfinite(ws32[:batches * M * N])
                assert bool(used.all() if batches > 1 else (~used).all()), what + ': not the form expected'
                if batches > 1:
                    ws32.fill_(NAN)
                    short = _launch(c, mode, ws=ws[:-1])
                    assert bool(torch.isnan(ws32).all()), what + ': a scratch one byte short was used'
                    _same_bits(short, _launch(c, mode), what + ': scratch one byte short')


# ---------------------------------------------------------------------------------------------------------------
# 8. one large-address case
# ---------------------------------------------------------------------------------------------------------------
def test_tile_origins_past_4_gib(hip):
    M, N, K, lda = (1 << 21) + 100, 16, 64, 1032
    a, w, bias = ref.exact_operands(M, N, K, 2 ** 24 - 1, device='cuda')
    buf = torch.full((M, lda), NAN, dtype=F16, device='cuda')
    assert (M - 256) * lda * 2 > 1 << 32
    A = buf[:, :K]
    A.copy_(a)
    a = None
    W = ref.window(w.to(F16), lead=64)
    obuf, out = ref.padded(M, N, F32, 'cuda')
    _ops().gemm(A, W, bias, 'store32', out=out)
    ref.guards_intact(obuf, M, N, 'large address')
    assert bool(torch.isfinite(out).all())
    last = (M - 1) // 256
    for t in [0, last] + [int(x) for x in torch.linspace(1, last - 1, 64)]:
        rows = slice(256 * t, min(256 * t + 256, M))
        want = A[rows].double() @ W.double().T + bias.double()[None]
        assert torch.equal(out[rows].double(), want), f'tile {t}'
    del buf, obuf
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------
def _refused(fragment, call):
    with pytest.raises(RuntimeError, match=re.escape(fragment)):
        call()
    torch.cuda.synchronize()


def test_refusals(hip):
    """What ec_gemm documents as refused stays refused; an option the dispatched kernel would not read is refused, not
    ignored (no caller in csrc/ or eventclip_amd/ passes one: tower_ops.h's Gemm sets aux for the STORE16 / GELU16 / RESID_HL
    / training epilogues, row_sums for RESID_HL and the statistics for the *_LN epilogues only)."""
    ops = _ops()
    from eventclip_amd import _lib
    M, N, K = 64, 64, 128
    c = _case(MODES['store16_ln@1'], F16, M, N, K, 'random')
    A, W, bias = c['A'], c['W'], c['bias']
    ln = dict(row_stats=c['stats'].contiguous(), col_sums=c['colsum'])
    o16, o32 = torch.zeros(M, N, dtype=F16, device='cuda'), torch.zeros(M, N, dtype=F32, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    take_no = 'the folded-LayerNorm epilogues take no splits / ws / resid'
    _refused(take_no, lambda: ops.gemm(A, W, bias, 'store16_ln', ws=ws, **ln))
    _refused(take_no, lambda: ops.gemm(A, W, bias, 'gelu16_ln', splits=2, **ln))
    _refused('args.resid goes with EC_EPI_RESID32', lambda: ops.gemm(A, W, bias, 'store16_ln', resid=o32, **ln))

    def transposed_with_bias():
        a = ops._gemm_args(A, W, o32, 64, 64, 64, _lib.EC_EPI_STORE32, 1)
        a.transposed, a.k_rows, a.bias = 1, 64, bias.data_ptr()
        _lib.launch('ec_gemm', a)
    _refused('transposed operands go with EC_EPI_STORE32, variant 0, no bias, no ws', transposed_with_bias)
    _refused('A_lo / W_lo take no transposed operands, splits, ws or resid', lambda: ops.gemm(A, W, bias, 'store32', A_lo=A.clone(), ws=ws))
    # refused, not ignored
    for epi, out in (('store32', o32), ('resid32', o32), ('store16_ln', o16), ('gelu16_ln', o16)):
        kw = ln if epi.endswith('_ln') else {}
        _refused('args.aux goes with', lambda: ops.gemm(A, W, bias, epi, out=out, aux=torch.zeros_like(o16), **kw))
    sums = torch.zeros(M, N // 64, 2, dtype=F32, device='cuda')
    for epi in ('store16', 'gelu16', 'store32', 'gelu16_ln'):
        kw = ln if epi.endswith('_ln') else {}
        _refused('args.row_sums goes with EC_EPI_RESID_HL', lambda: ops.gemm(A, W, bias, epi, row_sums=sums, **kw))
    for epi in ('store16', 'store32', 'resid_hl'):
        kw = dict(out=o16.clone(), aux=torch.zeros_like(o16)) if epi == 'resid_hl' else {}
        _refused('args.row_stats / col_sums go with', lambda: ops.gemm(A, W, bias, epi, **ln, **kw))


# ---------------------------------------------------------------------------------------------------------------
# 10. the table of refused calls: every message ec_gemm, its dispatch and its K-batched form can give in the product build,
#     and, where two checks fire for one call, which of them is reported
# ---------------------------------------------------------------------------------------------------------------
EPI = dict(store16=0, gelu16=1, resid32=2, store32=3, gelu16_save=4, gelu_bwd16=5, resid_hl=6, store16_ln=7, gelu16_ln=8)
OUT16 = ('store16', 'gelu16', 'gelu16_save', 'gelu_bwd16', 'resid_hl', 'store16_ln', 'gelu16_ln')


class _Pool:
    """The device tensors every pointer of every refused call points into, each large enough for the largest launch of the
    table (M = 256, N = 64, two batches of 192 columns, fp32): a call that is wrongly accepted runs inside allocated memory.
    A misaligned pointer is a view that starts 8 bytes into one of them."""

    def __init__(self):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device='cuda')  # noqa: E731
        self.op = {(n, dt): z((264, 392), dt) for n in ('A', 'W', 'A_lo', 'W_lo') for dt in (F16, BF16)}
        self.op8 = {n: z((264, 784), torch.uint8) for n in ('A_lo8', 'W8', 'A8', 'W_lo8')}
        self.out = {dt: z((2, 264, 72), dt) for dt in (F16, BF16, F32)}
        self.aux = {dt: z((264, 72), dt) for dt in (F16, BF16)}
        self.aux8 = z((264, 144), torch.uint8)
        self.resid, self.bias = z((264, 72), F32), z((72,), F32)
        self.stats, self.colsum, self.sums = z((2 * 264 + 8,), F32), z((72,), F32), z((264 * 2 * 2 + 8,), F32)
        self.ws = z((1 << 20,), torch.uint8)
        # by the name _pr's ('name', offset) fields use
        self.A, self.W, self.A_lo, self.W_lo = (self.op[n, F16] for n in ('A', 'W', 'A_lo', 'W_lo'))
        self.A_lo8, self.W8, self.A8, self.W_lo8 = (self.op8[n] for n in ('A_lo8', 'W8', 'A8', 'W_lo8'))
        self.aux16 = self.aux[F16]


@pytest.fixture(scope='module')
def pool(hip):
    return _Pool()


def _from(t, v, shape, stride):
    """the pool tensor ``t`` (v is True) or ``t`` from v bytes in, as a view of that shape and those strides"""
    flat = t.view(-1)
    return flat[(0 if v is True else v // t.element_size()):].as_strided(shape, stride)


def _pg(p, epi='store16', M=16, N=64, K=128, dt=F16, splits=1, off=0, tight=False, **kw):
    """ops.gemm on the pool's tensors.  Keywords name what the call passes: True = the pool's tensor for it, 8 = that tensor
    from 8 bytes in (for an e4m3 operand a pair with its exponent, for ``ln`` a pair (row_stats, col_sums)); every other
    keyword goes to ops.gemm as it is.  ``off``: A from that many elements in; ``tight``: ldw = K, what the variants other
    than 0 require."""
    KA = K * splits
    ldw = KA if tight else 392
    A, W = p.op['A', dt][:M, off:off + KA], _from(p.op['W', dt], True, (N, KA), (ldw, 1))
    o = p.out[dt if epi in OUT16 else F32]
    out = o[:splits, :M, :N] if splits > 1 else o[0, :M, :N]
    for k, like in (('A_lo', A), ('W_lo', W)):
        if k in kw:
            kw[k] = _from(p.op[k, dt], kw[k], like.shape, like.stride())
    for k, rows, ld in (('A_lo8', M, 392), ('W8', N, ldw), ('A8', M, 392), ('W_lo8', N, ldw)):
        if k in kw:
            v, e = kw[k] if isinstance(kw[k], tuple) else (kw[k], 0)
            kw[k] = (_from(p.op8[k], v, (rows, 2 * K), (2 * ld, 1)), e)
    if 'aux' in kw:
        kw['aux'] = _from(p.aux[F16 if epi == 'resid_hl' else dt], kw['aux'], (M, N), (72, 1))
    if 'aux8' in kw:
        kw['aux8'] = (_from(p.aux8, True, (M, 2 * N), (144, 1)), kw['aux8'])
    if 'resid' in kw:
        kw['resid'] = _from(p.resid, kw['resid'], (M, N), (72, 1))
    if 'ln' in kw:
        v = kw.pop('ln')
        s, c = v if isinstance(v, tuple) else (v, True)
        kw['row_stats'], kw['col_sums'] = _from(p.stats, s, (2 * M,), (1,)), _from(p.colsum, c, (N,), (1,))
    if 'row_sums' in kw:
        kw['row_sums'] = _from(p.sums, kw['row_sums'], (M * (N // 64) * 2,), (1,))
    if 'ws' in kw:
        kw['ws'] = p.ws[(0 if kw['ws'] is True else kw['ws']):]
    _ops().gemm(A, W, p.bias[:N], epi, out=out, splits=splits, **kw)


def _pr(p, epi='store16', M=16, N=64, K=128, dt=F16, splits=1, transposed=False, over=None, **fields):
    """ec_gemm called with an argument block filled by hand, for what ops.gemm's own assertions would stop: the block of
    _pg's call (the pool's A, W, bias and output; rows of operands as ops.gemm_rows passes them when transposed), then
    ``fields`` and ``over`` (the fields named like a parameter here) set as given -- a tensor stands for its address,
    ('name', 8) for the pool's tensor ``name`` from 8 bytes in."""
    from eventclip_amd import _lib
    o = p.out[dt if epi in OUT16 else F32]
    out = o[:splits, :M, :N] if splits > 1 else o[0, :M, :N]
    if transposed:
        A, W = p.op['A', dt][:K * splits, :M], p.op['W', dt][:K * splits, :N]
    else:
        A, W = p.op['A', dt][:M, :K * splits], p.op['W', dt][:N, :K * splits]
    a = _ops()._gemm_args(A, W, out, M, N, K, EPI[epi], splits)
    if transposed:
        a.transposed, a.k_rows = 1, K * splits
    else:
        a.bias = p.bias.data_ptr()
    for k, v in dict(fields, **(over or {})).items():
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        elif isinstance(v, tuple):
            v = getattr(p, v[0]).data_ptr() + v[1]
        setattr(a, k, v)
    _lib.launch('ec_gemm', a)


def _null_args(p):
    from eventclip_amd import _lib
    _lib.launch('ec_gemm', None)


def _row_stats_2_27(p):
    """M = 2^27 is the smallest row count the check refuses; the buffers the launch describes are allocated (not touched)."""
    M, N, K = 1 << 27, 16, 64
    A = torch.empty((M, K), dtype=F16, device='cuda')
    out = torch.empty((M, N), dtype=F16, device='cuda')
    stats = torch.empty((2 * M,), dtype=F32, device='cuda')
    try:
        _ops().gemm(A, p.op['W', F16][:N, :K], p.bias[:N], 'store16_ln', out=out, row_stats=stats, col_sums=p.colsum[:N])
    finally:
        del A, out, stats
        torch.cuda.empty_cache()


def _stride_2_21(p):
    """lda = 2^21 at M = 8: A spans 7 x 2^21 + 64 elements."""
    A = torch.empty((7 * (1 << 21) + 64,), dtype=F16, device='cuda')
    try:
        _pr(p, 'store16', M=8, N=16, K=64, A=A, lda=1 << 21)
    finally:
        del A
        torch.cuda.empty_cache()


LN1 = 'ec_gemm: the folded-LayerNorm epilogues take no splits / ws / resid'
SEG_NO = 'ec_gemm: A_lo / W_lo take no transposed operands, splits, ws or resid, and variant 0'
TN_GOES = 'ec_gemm: transposed operands go with EC_EPI_STORE32, variant 0, no bias, no ws'
AUX_GOES = 'ec_gemm: args.aux goes with the STORE16, GELU16, GELU16_SAVE, GELU_BWD16 and RESID_HL epilogues (epilogue '
RESID_GOES = 'ec_gemm: args.resid goes with EC_EPI_RESID32'
E4M3_AUX = ('ec_gemm: aux_e4m3 goes with EC_EPI_GELU16, an aux buffer, e4m3 lo products (A_lo8) and -60 <= aux_exp <= 60')
UNKNOWN_VARIANT = 'ec_gemm: unknown variant %d (diagnostic variants need an EC_GEMM_DIAG build)'
HL_AUX = 'ec_gemm: EC_EPI_RESID_HL needs args.aux (the lo plane)'
SEG8 = dict(A_lo8=True, W8=True)

# (id, the message, the call).  In the order of the checks in csrc/gemm.hip's check_args, launch_table and launch_row.
REFUSED = [
    # ---- shape and alignment
    ('null-args', 'ec_gemm: args is null', _null_args),
    ('shape-N0', 'ec_gemm: bad shape 16 x 0 x 128', lambda p: _pr(p, over=dict(N=0))),
    ('shape-K0', 'ec_gemm: bad shape 16 x 64 x 0', lambda p: _pr(p, over=dict(K=0))),
    ('shape-M<0', 'ec_gemm: bad shape -1 x 64 x 128', lambda p: _pr(p, over=dict(M=-1))),
    ('K%64', 'ec_gemm: K=96 must be a multiple of 64', lambda p: _pg(p, K=96)),
    ('N%16', 'ec_gemm: N=24 must be a multiple of 16', lambda p: _pg(p, N=24)),
    ('null-A', 'ec_gemm: null buffer', lambda p: _pr(p, A=None)),
    ('null-W', 'ec_gemm: null buffer', lambda p: _pr(p, W=None)),
    ('null-C', 'ec_gemm: null buffer', lambda p: _pr(p, C=None)),
    ('lda%8', 'ec_gemm: lda/ldc must be multiples of 8 elements', lambda p: _pr(p, lda=132)),
    ('ldc%8', 'ec_gemm: lda/ldc must be multiples of 8 elements', lambda p: _pr(p, ldc=68)),
    ('lda>=2^21', 'ec_gemm: row strides must be below 2^21 elements', _stride_2_21),
    ('A-misaligned', 'ec_gemm: buffers must be 16-byte aligned', lambda p: _pg(p, off=4)),
    ('C-misaligned', 'ec_gemm: buffers must be 16-byte aligned', lambda p: _pr(p, C=('resid', 8), epi='store32')),
    # ---- split-precision operands
    ('aux_e4m3-store16', E4M3_AUX, lambda p: _pg(p, 'store16', aux8=0, **SEG8)),
    ('aux_e4m3-no-A_lo8', E4M3_AUX, lambda p: _pg(p, 'gelu16', aux8=0, A8=True, W_lo8=True)),
    ('aux_e4m3-bf16', E4M3_AUX, lambda p: _pg(p, 'gelu16', dt=BF16, aux8=0, **SEG8)),
    ('aux_e4m3-exp', E4M3_AUX, lambda p: _pg(p, 'gelu16', aux8=61, **SEG8)),
    ('seg-ws', SEG_NO, lambda p: _pg(p, 'store32', A_lo=True, ws=True)),
    ('seg-splits', SEG_NO, lambda p: _pg(p, 'store32', K=64, splits=2, W_lo=True)),
    ('seg-resid', SEG_NO, lambda p: _pg(p, 'resid32', A_lo=True, resid=True)),
    ('seg-variant', SEG_NO, lambda p: _pg(p, 'store16', A_lo=True, variant=18)),
    ('seg-transposed', SEG_NO, lambda p: _pr(p, 'store32', transposed=True, A_lo=('A_lo', 0))),
    ('seg8-ws', SEG_NO, lambda p: _pg(p, 'store16', ws=True, **SEG8)),
    ('A_lo-misaligned', 'ec_gemm: A_lo / W_lo must be 16-byte aligned', lambda p: _pg(p, A_lo=8)),
    ('W_lo-misaligned', 'ec_gemm: A_lo / W_lo must be 16-byte aligned', lambda p: _pg(p, W_lo=8)),
    ('seg8-bf16', 'ec_gemm: e4m3 lo products need dtype EC_F16 and K % 128 == 0 (K = 128)', lambda p: _pg(p, dt=BF16, **SEG8)),
    ('seg8-K192', 'ec_gemm: e4m3 lo products need dtype EC_F16 and K % 128 == 0 (K = 192)', lambda p: _pg(p, K=192, **SEG8)),
    ('seg8-and-16', 'ec_gemm: a lo product is given as 16-bit (A_lo / W_lo) OR as e4m3 (A_lo8 / W_lo8), not both',
     lambda p: _pg(p, A_lo=True, **SEG8)),
    ('seg8-and-16-W', 'ec_gemm: a lo product is given as 16-bit (A_lo / W_lo) OR as e4m3 (A_lo8 / W_lo8), not both',
     lambda p: _pg(p, W_lo=True, A8=True, W_lo8=True)),
    ('A_lo8-no-W8', 'ec_gemm: A_lo8 needs W8 (the e4m3 copy of W), W_lo8 needs A8 (the e4m3 copy of A)', lambda p: _pg(p, A_lo8=True)),
    ('W_lo8-no-A8', 'ec_gemm: A_lo8 needs W8 (the e4m3 copy of W), W_lo8 needs A8 (the e4m3 copy of A)', lambda p: _pg(p, W_lo8=True)),
    ('e4m3-misaligned', 'ec_gemm: e4m3 operands must be 16-byte aligned', lambda p: _pg(p, A_lo8=True, W8=8)),
    ('a_lo8-exp', 'ec_gemm: a_lo8_exp + w8_exp = 127 outside -127 .. 126', lambda p: _pg(p, A_lo8=(True, 100), W8=(True, 27))),
    ('w_lo8-exp', 'ec_gemm: a8_exp + w_lo8_exp = -128 outside -127 .. 126', lambda p: _pg(p, A8=(True, -100), W_lo8=(True, -28))),
    # ---- options against the epilogue
    ('row_stats-misaligned', 'ec_gemm: row_stats / col_sums must be 16-byte aligned', lambda p: _pg(p, 'store16_ln', ln=8)),
    ('col_sums-misaligned', 'ec_gemm: row_stats / col_sums must be 16-byte aligned', lambda p: _pg(p, 'gelu16_ln', ln=(True, 8))),
    ('row_stats-M-2^27', 'ec_gemm: row_stats addresses its pairs with 32-bit byte offsets (M = 134217728)', _row_stats_2_27),
    ('row_sums-misaligned', 'ec_gemm: row_sums must be 8-byte aligned', lambda p: _pg(p, 'resid_hl', aux=True, row_sums=4)),
    ('activation-unknown', 'ec_gemm: unknown args.activation 2 (0 = QuickGELU, 1 = exact GELU)', lambda p: _pg(p, 'gelu16', activation=2)),
    ('activation-negative', 'ec_gemm: unknown args.activation -1 (0 = QuickGELU, 1 = exact GELU)', lambda p: _pg(p, 'gelu16', activation=-1)),
    ('activation-store16', 'ec_gemm: args.activation goes with the GELU16, GELU16_LN, GELU16_SAVE and GELU_BWD16 epilogues (epilogue 0)',
     lambda p: _pg(p, 'store16', activation=1)),
    ('activation-resid_hl', 'ec_gemm: args.activation goes with the GELU16, GELU16_LN, GELU16_SAVE and GELU_BWD16 epilogues (epilogue 6)',
     lambda p: _pg(p, 'resid_hl', aux=True, activation=1)),
    ('aux-store32', AUX_GOES + '3)', lambda p: _pg(p, 'store32', aux=True)),
    ('aux-resid32', AUX_GOES + '2)', lambda p: _pg(p, 'resid32', aux=True)),
    ('aux-store16_ln', AUX_GOES + '7)', lambda p: _pg(p, 'store16_ln', aux=True, ln=True)),
    ('aux-gelu16_ln', AUX_GOES + '8)', lambda p: _pg(p, 'gelu16_ln', aux=True, ln=True)),
    ('row_sums-store16', 'ec_gemm: args.row_sums goes with EC_EPI_RESID_HL (epilogue 0)', lambda p: _pg(p, 'store16', row_sums=True)),
    ('row_sums-gelu16_ln', 'ec_gemm: args.row_sums goes with EC_EPI_RESID_HL (epilogue 8)', lambda p: _pg(p, 'gelu16_ln', ln=True, row_sums=True)),
    ('stats-store16', 'ec_gemm: args.row_stats / col_sums go with EC_EPI_STORE16_LN / EC_EPI_GELU16_LN (epilogue 0)',
     lambda p: _pg(p, 'store16', ln=True)),
    ('col_sums-resid_hl', 'ec_gemm: args.row_stats / col_sums go with EC_EPI_STORE16_LN / EC_EPI_GELU16_LN (epilogue 6)',
     lambda p: _pr(p, 'resid_hl', aux=('aux16', 0), col_sums=('colsum', 0))),
    ('row_sums-N16', 'ec_gemm: row_sums needs N % 64 == 0 (N = 16)', lambda p: _pr(p, 'resid_hl', N=16, aux=('aux16', 0), row_sums=('sums', 0))),
    # ---- transposed operands
    ('tn-bias', TN_GOES, lambda p: _pr(p, 'store32', transposed=True, bias=('bias', 0))),
    ('tn-ws', TN_GOES, lambda p: _pr(p, 'store32', transposed=True, ws=('ws', 0), ws_bytes=1 << 20)),
    ('tn-variant', TN_GOES, lambda p: _pr(p, 'store32', transposed=True, variant=18)),
    ('tn-store16', TN_GOES, lambda p: _pr(p, 'store16', transposed=True)),
    ('tn-M%8', 'ec_gemm: transposed operands need M % 8 == 0 and row strides (multiples of 8) covering M and N',
     lambda p: _pr(p, 'store32', transposed=True, over=dict(M=12))),
    ('tn-lda<M', 'ec_gemm: transposed operands need M % 8 == 0 and row strides (multiples of 8) covering M and N',
     lambda p: _pr(p, 'store32', transposed=True, lda=8)),
    ('tn-ldw<N', 'ec_gemm: transposed operands need M % 8 == 0 and row strides (multiples of 8) covering M and N',
     lambda p: _pr(p, 'store32', transposed=True, ldw=56)),
    ('tn-k_rows0', 'ec_gemm: k_rows=0 outside (0, splits * K = 128]', lambda p: _pr(p, 'store32', transposed=True, k_rows=0)),
    ('tn-k_rows>', 'ec_gemm: k_rows=129 outside (0, splits * K = 128]', lambda p: _pr(p, 'store32', K=64, splits=2, transposed=True, k_rows=129)),
    ('tn-split_stride', 'ec_gemm: split_stride 1136 too small for an 16 x 64 output',
     lambda p: _pr(p, 'store32', K=64, splits=2, transposed=True, split_stride=1136)),
    ('tn-split_stride%8', 'ec_gemm: split_stride 19012 too small for an 16 x 64 output',
     lambda p: _pr(p, 'store32', K=64, splits=2, transposed=True, split_stride=19012)),
    ('tn-dtype', 'ec_gemm: unknown dtype 7', lambda p: _pr(p, 'store32', transposed=True, dtype=7)),
    # ---- splits / ldw / resid
    ('ldw<K', 'ec_gemm: lda / ldw must cover splits * K columns and be multiples of 8 elements', lambda p: _pr(p, ldw=64)),
    ('ldw%8', 'ec_gemm: lda / ldw must cover splits * K columns and be multiples of 8 elements', lambda p: _pr(p, ldw=132)),
    ('lda<splits*K', 'ec_gemm: lda / ldw must cover splits * K columns and be multiples of 8 elements',
     lambda p: _pr(p, 'store32', K=64, splits=2, lda=64)),
    ('resid-misaligned', 'ec_gemm: resid / aux must be 16-byte aligned', lambda p: _pg(p, 'resid32', resid=8)),
    ('aux-misaligned', 'ec_gemm: resid / aux must be 16-byte aligned', lambda p: _pg(p, 'gelu16_save', aux=8)),
    ('resid-store32', RESID_GOES, lambda p: _pg(p, 'store32', resid=True)),
    ('resid-resid_hl', RESID_GOES, lambda p: _pg(p, 'resid_hl', aux=True, resid=True)),
    ('splits-variant', 'ec_gemm: ldw / splits / resid need variant 0', lambda p: _pg(p, 'store32', K=64, splits=2, variant=18)),
    ('ldw-variant', 'ec_gemm: ldw / splits / resid need variant 0', lambda p: _pr(p, 'store32', K=64, variant=19)),
    ('resid-variant', 'ec_gemm: ldw / splits / resid need variant 0', lambda p: _pg(p, 'resid32', resid=True, variant=1, tight=True)),
    ('split_stride', 'ec_gemm: split_stride 1136 too small for an 16 x 64 output', lambda p: _pr(p, 'store32', K=64, splits=2, split_stride=1136)),
    ('split_stride%8', 'ec_gemm: split_stride 19012 too small for an 16 x 64 output',
     lambda p: _pr(p, 'store32', K=64, splits=2, split_stride=19012)),
    ('ln-ws', LN1, lambda p: _pg(p, 'store16_ln', ln=True, ws=True)),
    ('ln-splits', LN1, lambda p: _pg(p, 'gelu16_ln', K=64, splits=2, ln=True)),
    ('hl-ws', LN1, lambda p: _pg(p, 'resid_hl', aux=True, ws=True)),
    ('epi9-ws', LN1, lambda p: _pr(p, ws=('ws', 0), ws_bytes=1 << 20, epilogue=9)),
    # ---- K-batch scratch
    ('ws-misaligned', 'ec_gemm: ws must be 16-byte aligned', lambda p: _pg(p, 'store16', ws=8)),
    ('ws-gelu16_save-no-aux', 'ec_gemm: epilogue 4 needs aux', lambda p: _pg(p, 'gelu16_save', ws=True)),
    ('ws-gelu_bwd16-no-aux', 'ec_gemm: epilogue 5 needs aux', lambda p: _pg(p, 'gelu_bwd16', ws=True)),
    ('dtype', 'ec_gemm: unknown dtype 2', lambda p: _pr(p, dtype=2)),
    ('dtype-ws', 'ec_gemm: unknown dtype -1', lambda p: _pr(p, dtype=-1, ws=('ws', 0), ws_bytes=1 << 20)),
    # ---- the table of launches
    ('erf-variant', 'ec_gemm: args.activation = 1 needs variant 0', lambda p: _pg(p, 'gelu16', activation=1, variant=18, tight=True)),
    ('seg8-resid_hl-no-aux', HL_AUX, lambda p: _pr(p, 'resid_hl', A_lo8=('A_lo8', 0), W8=('W8', 0))),
    ('seg8-resid32', 'ec_gemm: e4m3 lo products go with the STORE16, GELU16, STORE32 and RESID_HL epilogues (got 2)',
     lambda p: _pg(p, 'resid32', **SEG8)),
    ('seg8-gelu16_save', 'ec_gemm: e4m3 lo products go with the STORE16, GELU16, STORE32 and RESID_HL epilogues (got 4)',
     lambda p: _pg(p, 'gelu16_save', aux=True, A8=True, W_lo8=True)),
    ('seg-resid_hl-no-aux', HL_AUX, lambda p: _pr(p, 'resid_hl', A_lo=('A_lo', 0))),
    ('seg-gelu_bwd16', 'ec_gemm: A_lo / W_lo go with the STORE16, GELU16, STORE32, RESID32 and RESID_HL epilogues (got 5)',
     lambda p: _pg(p, 'gelu_bwd16', aux=True, W_lo=True)),
    ('seg-store16_ln', 'ec_gemm: A_lo / W_lo go with the STORE16, GELU16, STORE32, RESID32 and RESID_HL epilogues (got 7)',
     lambda p: _pg(p, 'store16_ln', ln=True, A_lo=True)),
    ('seg-epi9', 'ec_gemm: A_lo / W_lo go with the STORE16, GELU16, STORE32, RESID32 and RESID_HL epilogues (got 9)',
     lambda p: _pr(p, A_lo=('A_lo', 0), epilogue=9)),
    ('lo-out-store16', 'ec_gemm: STORE16 / GELU16 write their lo part (args.aux) in the launches that take A_lo / W_lo only',
     lambda p: _pg(p, 'store16', aux=True)),
    ('lo-out-gelu16', 'ec_gemm: STORE16 / GELU16 write their lo part (args.aux) in the launches that take A_lo / W_lo only',
     lambda p: _pg(p, 'gelu16', dt=BF16, aux=True)),
    ('gelu16_save-no-aux', 'ec_gemm: EC_EPI_GELU16_SAVE needs variant 0 and args.aux', lambda p: _pg(p, 'gelu16_save')),
    ('gelu16_save-variant', 'ec_gemm: EC_EPI_GELU16_SAVE needs variant 0 and args.aux', lambda p: _pg(p, 'gelu16_save', aux=True, variant=18, tight=True)),
    ('gelu_bwd16-no-aux', 'ec_gemm: EC_EPI_GELU_BWD16 needs variant 0 and args.aux', lambda p: _pg(p, 'gelu_bwd16')),
    ('gelu_bwd16-variant', 'ec_gemm: EC_EPI_GELU_BWD16 needs variant 0 and args.aux', lambda p: _pg(p, 'gelu_bwd16', aux=True, variant=19, tight=True)),
    ('resid_hl-no-aux', 'ec_gemm: EC_EPI_RESID_HL needs variant 0 and args.aux (the lo plane)', lambda p: _pr(p, 'resid_hl')),
    ('resid_hl-variant', 'ec_gemm: EC_EPI_RESID_HL needs variant 0 and args.aux (the lo plane)', lambda p: _pg(p, 'resid_hl', aux=True, variant=18, tight=True)),
    ('store16_ln-no-stats', 'ec_gemm: EC_EPI_STORE16_LN needs variant 0, row_stats and col_sums', lambda p: _pr(p, 'store16_ln')),
    ('store16_ln-no-col_sums', 'ec_gemm: EC_EPI_STORE16_LN needs variant 0, row_stats and col_sums',
     lambda p: _pr(p, 'store16_ln', row_stats=('stats', 0))),
    ('store16_ln-variant', 'ec_gemm: EC_EPI_STORE16_LN needs variant 0, row_stats and col_sums', lambda p: _pg(p, 'store16_ln', ln=True, variant=19, tight=True)),
    ('gelu16_ln-no-stats', 'ec_gemm: EC_EPI_GELU16_LN needs variant 0, row_stats and col_sums', lambda p: _pr(p, 'gelu16_ln')),
    ('gelu16_ln-variant', 'ec_gemm: EC_EPI_GELU16_LN needs variant 0, row_stats and col_sums', lambda p: _pg(p, 'gelu16_ln', ln=True, variant=18, tight=True)),
    ('epilogue-9', 'ec_gemm: unknown epilogue 9', lambda p: _pr(p, epilogue=9)),
    ('epilogue-negative', 'ec_gemm: unknown epilogue -1', lambda p: _pr(p, epilogue=-1)),
    ('epilogue-negative-ws', 'ec_gemm: unknown epilogue -1', lambda p: _pr(p, epilogue=-1, ws=('ws', 0), ws_bytes=1 << 20)),
] + [
    (f'variant-{v}-{e}-{d}', UNKNOWN_VARIANT % v, lambda p, e=e, v=v, d=d: _pg(p, e, dt=DT[d], variant=v, tight=True))
    for e in ('store16', 'gelu16', 'resid32', 'store32') for v, d in ((18, 'float16'), (19, 'bfloat16'), (1, 'float16'))
] + [
    # a scratch that qualifies for the K-batched form (one tile, 8 K tiles) does not hide the variant from the dispatch
    ('variant-ws', UNKNOWN_VARIANT % 18, lambda p: _pg(p, 'store16', M=256, K=384, ws=True, variant=18, tight=True)),
]

# Two checks fire for one call: which is reported.  (id, the message reported, the call)
REFUSED_FIRST = [
    ('shape>K%64', 'ec_gemm: bad shape 16 x 0 x 96', lambda p: _pr(p, over=dict(N=0, K=96))),
    ('K%64>N%16', 'ec_gemm: K=96 must be a multiple of 64', lambda p: _pg(p, N=24, K=96)),
    ('N%16>null', 'ec_gemm: N=24 must be a multiple of 16', lambda p: _pr(p, N=24, A=None)),
    ('null>lda%8', 'ec_gemm: null buffer', lambda p: _pr(p, W=None, lda=132)),
    ('ld%8>aligned', 'ec_gemm: lda/ldc must be multiples of 8 elements', lambda p: _pr(p, lda=132, A=('A', 8))),
    ('aligned>aux_e4m3', 'ec_gemm: buffers must be 16-byte aligned', lambda p: _pr(p, A=('A', 8), aux_e4m3=1)),
    ('aux_e4m3>seg', E4M3_AUX, lambda p: _pg(p, 'store16', aux8=0, ws=True, **SEG8)),
    ('seg>seg-misaligned', SEG_NO, lambda p: _pg(p, 'store32', A_lo=8, ws=True)),
    ('seg+resid', SEG_NO, lambda p: _pg(p, 'store16', A_lo=True, resid=True)),
    ('seg+resid-misaligned', SEG_NO, lambda p: _pg(p, 'resid32', W_lo=True, resid=8)),
    ('seg+transposed+bias', SEG_NO, lambda p: _pr(p, 'store32', transposed=True, bias=('bias', 0), W_lo=('W_lo', 0))),
    ('seg+activation', SEG_NO, lambda p: _pg(p, 'store16', A_lo=True, ws=True, activation=2)),
    ('seg+ln+ws', SEG_NO, lambda p: _pg(p, 'store16_ln', ln=True, A_lo=True, ws=True)),
    ('seg-misaligned>seg8', 'ec_gemm: A_lo / W_lo must be 16-byte aligned', lambda p: _pg(p, K=192, W_lo=8, **SEG8)),
    ('seg8-K>both', 'ec_gemm: e4m3 lo products need dtype EC_F16 and K % 128 == 0 (K = 192)', lambda p: _pg(p, K=192, A_lo=True, **SEG8)),
    ('both>needs', 'ec_gemm: a lo product is given as 16-bit (A_lo / W_lo) OR as e4m3 (A_lo8 / W_lo8), not both',
     lambda p: _pg(p, A_lo=True, A_lo8=True)),
    ('needs>e4m3-misaligned', 'ec_gemm: A_lo8 needs W8 (the e4m3 copy of W), W_lo8 needs A8 (the e4m3 copy of A)', lambda p: _pg(p, A_lo8=8)),
    ('e4m3-misaligned>exp', 'ec_gemm: e4m3 operands must be 16-byte aligned', lambda p: _pg(p, A_lo8=(8, 100), W8=(True, 100))),
    ('a_lo8-exp>w_lo8-exp', 'ec_gemm: a_lo8_exp + w8_exp = 200 outside -127 .. 126',
     lambda p: _pg(p, A_lo8=(True, 100), W8=(True, 100), A8=(True, 100), W_lo8=(True, 100))),
    ('seg8-exp>stats-misaligned', 'ec_gemm: a8_exp + w_lo8_exp = 200 outside -127 .. 126',
     lambda p: _pg(p, 'store16_ln', ln=8, A8=(True, 100), W_lo8=(True, 100))),
    ('seg-misaligned>activation', 'ec_gemm: A_lo / W_lo must be 16-byte aligned', lambda p: _pg(p, 'store16', A_lo=8, activation=1)),
    ('seg8-bf16>aux', 'ec_gemm: e4m3 lo products need dtype EC_F16 and K % 128 == 0 (K = 128)', lambda p: _pg(p, 'store32', dt=BF16, aux=True, **SEG8)),
    ('stats-misaligned>row_sums-misaligned', 'ec_gemm: row_stats / col_sums must be 16-byte aligned', lambda p: _pg(p, 'store16', ln=(True, 8), row_sums=4)),
    ('row_sums-misaligned>activation', 'ec_gemm: row_sums must be 8-byte aligned', lambda p: _pg(p, 'store16', row_sums=4, activation=2)),
    ('activation-unknown>goes', 'ec_gemm: unknown args.activation 2 (0 = QuickGELU, 1 = exact GELU)', lambda p: _pg(p, 'store16', activation=2)),
    ('activation>aux', 'ec_gemm: args.activation goes with the GELU16, GELU16_LN, GELU16_SAVE and GELU_BWD16 epilogues (epilogue 3)',
     lambda p: _pg(p, 'store32', activation=1, aux=True)),
    ('aux>row_sums', AUX_GOES + '3)', lambda p: _pg(p, 'store32', aux=True, row_sums=True)),
    ('row_sums>stats', 'ec_gemm: args.row_sums goes with EC_EPI_RESID_HL (epilogue 0)', lambda p: _pg(p, 'store16', row_sums=True, ln=True)),
    ('stats>N%64', 'ec_gemm: args.row_stats / col_sums go with EC_EPI_STORE16_LN / EC_EPI_GELU16_LN (epilogue 6)',
     lambda p: _pr(p, 'resid_hl', N=16, aux=('aux16', 0), row_sums=('sums', 0), row_stats=('stats', 0))),
    ('N%64>resid', 'ec_gemm: row_sums needs N % 64 == 0 (N = 16)',
     lambda p: _pr(p, 'resid_hl', N=16, aux=('aux16', 0), row_sums=('sums', 0), resid=('resid', 0))),
    ('aux>tn', AUX_GOES + '3)', lambda p: _pr(p, 'store32', transposed=True, bias=('bias', 0), aux=('aux16', 0))),
    ('activation>tn', 'ec_gemm: args.activation goes with the GELU16, GELU16_LN, GELU16_SAVE and GELU_BWD16 epilogues (epilogue 3)',
     lambda p: _pr(p, 'store32', transposed=True, bias=('bias', 0), activation=1)),
    ('tn+bias+ws', TN_GOES, lambda p: _pr(p, 'store32', transposed=True, bias=('bias', 0), ws=('ws', 8), ws_bytes=1 << 19)),
    ('tn-goes>strides', TN_GOES, lambda p: _pr(p, 'resid32', transposed=True, lda=8)),
    ('tn-goes>resid', TN_GOES, lambda p: _pr(p, 'store16_ln', transposed=True, resid=('resid', 8))),
    ('tn-strides>k_rows', 'ec_gemm: transposed operands need M % 8 == 0 and row strides (multiples of 8) covering M and N',
     lambda p: _pr(p, 'store32', transposed=True, ldw=56, k_rows=0)),
    ('tn-k_rows>split_stride', 'ec_gemm: k_rows=0 outside (0, splits * K = 128]',
     lambda p: _pr(p, 'store32', K=64, splits=2, transposed=True, k_rows=0, split_stride=8)),
    ('tn-split_stride>dtype', 'ec_gemm: split_stride 8 too small for an 16 x 64 output',
     lambda p: _pr(p, 'store32', K=64, splits=2, transposed=True, split_stride=8, dtype=7)),
    ('ldw>resid-misaligned', 'ec_gemm: lda / ldw must cover splits * K columns and be multiples of 8 elements',
     lambda p: _pr(p, 'resid32', ldw=64, resid=('resid', 8))),
    ('misaligned>resid-goes', 'ec_gemm: resid / aux must be 16-byte aligned', lambda p: _pg(p, 'store32', resid=8)),
    ('resid-goes>variant', RESID_GOES, lambda p: _pg(p, 'store16', resid=True, variant=18)),
    ('ln+ws+resid', RESID_GOES, lambda p: _pg(p, 'store16_ln', ln=True, ws=True, resid=True)),
    ('hl+resid+splits', RESID_GOES, lambda p: _pg(p, 'resid_hl', K=64, splits=2, aux=True, resid=True)),
    ('variant>split_stride', 'ec_gemm: ldw / splits / resid need variant 0',
     lambda p: _pr(p, 'store32', K=64, splits=2, split_stride=8, variant=18)),
    ('split_stride>ln', 'ec_gemm: split_stride 8 too small for an 16 x 64 output',
     lambda p: _pr(p, 'gelu16_ln', K=64, splits=2, split_stride=8, row_stats=('stats', 0), col_sums=('colsum', 0))),
    ('ln-splits>no-stats', LN1, lambda p: _pr(p, 'store16_ln', K=64, splits=2, split_stride=19008)),
    ('ln-ws>ws-misaligned', LN1, lambda p: _pg(p, 'gelu16_ln', ln=True, ws=8)),
    ('ln-ws>dtype', LN1, lambda p: _pr(p, 'resid_hl', aux=('aux16', 0), ws=('ws', 0), ws_bytes=1 << 20, dtype=7)),
    ('ws-misaligned>needs-aux', 'ec_gemm: ws must be 16-byte aligned', lambda p: _pg(p, 'gelu16_save', ws=8)),
    ('ws-needs-aux>dtype', 'ec_gemm: epilogue 5 needs aux', lambda p: _pr(p, 'gelu_bwd16', ws=('ws', 0), ws_bytes=1 << 20, dtype=7)),
    ('ws-misaligned>dtype', 'ec_gemm: ws must be 16-byte aligned', lambda p: _pr(p, 'store32', ws=('ws', 8), ws_bytes=1 << 19, dtype=7)),
    ('variant-skips-ws-check', UNKNOWN_VARIANT % 18, lambda p: _pg(p, 'store16', ws=8, variant=18, tight=True)),
    ('splits-skip-ws-check', 'ec_gemm: unknown dtype 7', lambda p: _pr(p, 'store32', K=64, splits=2, ws=('ws', 8), ws_bytes=1 << 19, dtype=7)),
    ('dtype>epilogue', 'ec_gemm: unknown dtype 7', lambda p: _pr(p, epilogue=9, dtype=7)),
    ('dtype>erf-variant', 'ec_gemm: unknown dtype 7', lambda p: _pr(p, 'gelu16', activation=1, variant=18, dtype=7, ldw=0)),
    ('erf-variant>needs-aux', 'ec_gemm: args.activation = 1 needs variant 0', lambda p: _pg(p, 'gelu16_save', activation=1, variant=18, tight=True)),
    ('erf-variant>lo-out', 'ec_gemm: args.activation = 1 needs variant 0', lambda p: _pg(p, 'gelu16', aux=True, activation=1, variant=18, tight=True)),
    ('seg8-gelu_bwd16-no-aux', 'ec_gemm: e4m3 lo products go with the STORE16, GELU16, STORE32 and RESID_HL epilogues (got 5)',
     lambda p: _pr(p, 'gelu_bwd16', A_lo8=('A_lo8', 0), W8=('W8', 0))),
    ('lo-out>variant', 'ec_gemm: STORE16 / GELU16 write their lo part (args.aux) in the launches that take A_lo / W_lo only',
     lambda p: _pg(p, 'store16', aux=True, variant=18, tight=True)),
    ('needs-aux>variant', 'ec_gemm: EC_EPI_GELU16_SAVE needs variant 0 and args.aux', lambda p: _pg(p, 'gelu16_save', variant=18, tight=True)),
]


@pytest.mark.parametrize('case', REFUSED + REFUSED_FIRST, ids=lambda c: c[0])
def test_refused_calls(case, pool):
    """Each refusal by its whole message.  The sites of csrc/gemm.hip that no call reaches in the product build have no case:
    `variant %d needs args.diag` (diagnostic build), `cannot read the device's compute-unit count`, and launch_row's
    `e4m3 lo products need dtype EC_F16`, which keeps the e4m3 kernels from being built for bf16 and which check_args' own
    dtype check for e4m3 operands shadows."""
    _, message, call = case
    _refused(message, lambda: call(pool))
