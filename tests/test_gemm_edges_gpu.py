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
