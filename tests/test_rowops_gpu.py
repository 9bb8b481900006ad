"""Every exported entry point of csrc/layernorm.hip, called directly, at its edges, against float64 or bit-exact
expectations: tests/rowops_ref.py holds the references, the directed inputs and the bounds (per element; their constants
are measured in tests/test_rowops_ref_cpu.py, the kernels get four times the fp32 restatement's error).

Every output buffer is pre-filled with NaN (0xAA bytes for e4m3), has 64 padding columns where the entry point takes a
stride and one guard row (64 guard elements for the flat kernels) behind the last: padding and guard must come back bit
for bit, and nothing that was written may be NaN.  Source rows at a stride have NaN between them."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT = ref.DTYPES
PAD = 64
NAN = float('nan')


def _L():
    from eventclip_amd import _lib
    return _lib


def _code(dtype):
    return ref.EC_F16 if dtype == F16 else ref.EC_BF16


def _p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def _ok(rc, what):
    _L().check(rc, what)


def _refused(rc, needle):
    lib = _L()
    assert rc == lib.EC_ERR_INVALID, rc
    msg = lib.lib().ec_last_error().decode()
    assert needle in msg, msg


def _nan_buf(*shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _untouched(buf, rows, width, what):
    """buf [rows + 1, ld], filled by _nan_buf: the columns from `width` on and the guard row still hold the fill."""
    fill = _bits(torch.full((1,), NAN, dtype=buf.dtype, device='cuda'))[0]
    b = _bits(buf)
    assert bool((b[:rows, width:] == fill).all()), f'{what}: padding columns written'
    assert bool((b[rows:] == fill).all()), f'{what}: guard row written'


def _within(got, want, bound, what):
    over = ref.excess(got, want, bound)
    assert over <= 0, f'{what}: {float((got.double() - want).abs().max()):.3e} off, {over:.3e} over the bound'


def _strided(x, mul):
    """x [rows, width] -> a [rows, mul, width] buffer of NaN with x in [:, 0]: rows at stride mul * width."""
    if mul == 1:
        return x.contiguous()
    buf = _nan_buf(x.shape[0], mul, x.shape[1], dtype=x.dtype)
    buf[:, 0] = x
    return buf


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm family
# ---------------------------------------------------------------------------------------------------------------
def _layernorm(api, x, planes, ldx, row_idx, gamma, beta, rows, width, eps, dtype):
    """-> (hi [rows, width], lo or None), after the padding / guard checks."""
    lib = _L().lib()
    ldo = width + PAD
    hi = _nan_buf(rows + 1, ldo, dtype=dtype)
    lo = None if api == 'plain' else _nan_buf(rows + 1, ldo, dtype=dtype)
    s = _L().stream_ptr()
    if api == 'plain':
        rc = lib.ec_layernorm(_p(x), ldx, _p(row_idx), _p(gamma), _p(beta), rows, width, eps, _p(hi), ldo, _code(dtype), s)
    elif api == 'split':
        rc = lib.ec_layernorm_split(_p(x), ldx, _p(row_idx), _p(gamma), _p(beta), rows, width, eps, _p(hi), _p(lo), ldo,
                                    _code(dtype), s)
    else:
        rc = lib.ec_layernorm_hl(_p(planes[0]), _p(planes[1]), ldx, _p(gamma), _p(beta), rows, width, eps, _p(hi), _p(lo), ldo,
                                 _code(dtype), s)
    _ok(rc, api)
    for buf in (hi, lo):
        if buf is not None:
            _untouched(buf, rows, width, f'{api} rows={rows} width={width}')
    return hi[:rows, :width], None if lo is None else lo[:rows, :width]


def _check_ln(api, hi, lo, want, s, kind, dtype, what):
    e = ref.ln_e(s, kind)
    _within(hi, want, ref.bound16(want, e, dtype), what + ' hi')
    if lo is not None:
        assert bool(torch.isfinite(lo).all()), what + ': lo not finite'
        _within(hi.double() + lo.double(), want, ref.bound_pair(want, e, dtype, dtype), what + ' hi + lo')
    const = (kind == ref.CONSTANT).to(hi.device)
    if bool(const.any()):          # variance exactly 0: beta, to the bound, and finite
        beta = want[const]
        assert bool(torch.isfinite(hi[const]).all())
        _within(hi[const], beta, ref.bound16(beta, e[const], dtype), what + ' constant rows')


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('api', ['plain', 'split', 'hl'])
@pytest.mark.parametrize('width', ref.LN_WIDTHS)
def test_layernorm_family(width, api, dt, hip):
    """ec_layernorm (ec_layernorm_split with lo = NULL), ec_layernorm_split and ec_layernorm_hl: one lane with data
    (width 4), a partial last unit (252, 260, 772, 1284, 2044), all eight vectors per lane (2048); 1 .. 5 rows (four per
    workgroup) and 1021; rows packed and at the class-token stride 5 width; eps 1e-5 and 1e-3; every kind of row."""
    dtype = DT[dt]
    gamma, beta = (t.cuda() for t in ref.gamma_beta(width))
    for rows in ref.ROWS:
        for rot in ref.rotations(rows):
            x, kind = ref.ln_rows(rows, width, rot)
            x = x.cuda()
            planes = ref.split(x, dtype, F16) if api == 'hl' else None
            seen = planes[0].double() + planes[1].double() if api == 'hl' else x
            for mul in (1, 5):
                src = _strided(x, mul) if api != 'hl' else None
                pl = [_strided(p, mul) for p in planes] if api == 'hl' else None
                for eps in ref.EPS:
                    want, s = ref.layernorm64(seen, gamma, beta, eps)
                    hi, lo = _layernorm(api, src, pl, mul * width, None, gamma, beta, rows, width, eps, dtype)
                    _check_ln(api, hi, lo, want, s, kind, dtype, f'{api} {dt} {rows}x{width} rot={rot} ldx={mul}w eps={eps}')


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('api', ['plain', 'split'])
def test_layernorm_gathers_rows(api, dt, hip):
    """row_idx: repeated, descending and last-row indices (ln_final on the end-of-text rows)."""
    dtype = DT[dt]
    width, n = 260, 9
    x, kind = ref.ln_rows(n, width, 1)
    x = x.cuda()
    gamma, beta = (t.cuda() for t in ref.gamma_beta(width))
    idx = torch.tensor([8, 8, 3, 2, 1, 0, 8, 0, 5, 5, 4], dtype=torch.int32, device='cuda')
    want, s = ref.layernorm64(x, gamma, beta, 1e-5)
    hi, lo = _layernorm(api, x, None, width, idx, gamma, beta, len(idx), width, 1e-5, dtype)
    _check_ln(api, hi, lo, want[idx.long()], s[idx.long()], kind[idx.long().cpu()], dtype, f'{api} {dt} gathered')


def test_layernorm_refusals(hip):
    """Each call returns before any launch: widths 2052 and 6, an unknown type, misaligned base pointers; zero rows with
    null pointers is fine."""
    lib, s = _L().lib(), _L().stream_ptr()
    w = 64
    x = torch.zeros(4, w, device='cuda')
    g, b = torch.ones(w, device='cuda'), torch.zeros(w, device='cuda')
    h, l = (torch.zeros(4, w, dtype=F16, device='cuda') for _ in range(2))
    o, o2 = (torch.zeros(4, 2 * w, dtype=F16, device='cuda') for _ in range(2))
    for width in (2052, 6):
        _refused(lib.ec_layernorm(_p(x), width, None, _p(g), _p(b), 1, width, 1e-5, _p(o), width, 0, s), 'multiple of 4')
        _refused(lib.ec_layernorm_split(_p(x), width, None, _p(g), _p(b), 1, width, 1e-5, _p(o), _p(o2), width, 0, s), 'multiple of 4')
        _refused(lib.ec_layernorm_hl(_p(h), _p(l), width, _p(g), _p(b), 1, width, 1e-5, _p(o), _p(o2), width, 0, s), 'multiple of 4')
        _refused(lib.ec_layernorm_hl8(_p(h), _p(l), width, _p(g), _p(b), 1, width, 1e-5, _p(o), _p(o2), None, width, 12, 0, s),
                 'multiple of 4')
    _refused(lib.ec_layernorm(_p(x), w, None, _p(g), _p(b), 4, w, 1e-5, _p(o), w, 7, s), 'unknown dtype')
    _refused(lib.ec_layernorm_hl(_p(h), _p(l), w, _p(g), _p(b), 4, w, 1e-5, _p(o), _p(o2), w, 7, s), 'unknown dtype')
    assert lib.ec_layernorm(None, w, None, None, None, 0, w, 1e-5, None, w, 0, s) == 0
    assert lib.ec_layernorm_split(None, w, None, None, None, 0, w, 1e-5, None, None, w, 0, s) == 0
    assert lib.ec_layernorm_hl(None, None, w, None, None, 0, w, 1e-5, None, None, w, 0, s) == 0
    assert lib.ec_layernorm_hl8(None, None, w, None, None, 0, w, 1e-5, None, None, None, w, 12, 0, s) == 0
    # a base pointer off by one element (fp32: 4 of 16 bytes; 16-bit: 2 of 8 bytes; e4m3: 2 of 4 bytes)
    for i, off in enumerate([(4, 0, 0, 0, 0), (0, 4, 0, 0, 0), (0, 0, 4, 0, 0), (0, 0, 0, 2, 0), (0, 0, 0, 0, 2)]):
        _refused(lib.ec_layernorm_split(_p(x, off[0]), w, None, _p(g, off[1]), _p(b, off[2]), 2, w, 1e-5, _p(o, off[3]),
                                        _p(o2, off[4]), w, 0, s), 'misaligned')
        _refused(lib.ec_layernorm_hl(_p(h, off[3]), _p(l, off[4]), w, _p(g, off[1]), _p(b, off[2]), 2, w, 1e-5,
                                     _p(o, off[0] // 2), _p(o2), w, 0, s), 'misaligned')
    for off in [(2, 0, 0, 0, 0), (0, 2, 0, 0, 0), (0, 0, 2, 0, 0), (0, 0, 0, 2, 0), (0, 0, 0, 0, 2)]:
        _refused(lib.ec_layernorm_hl8(_p(h, off[0]), _p(l, off[1]), w, _p(g), _p(b), 2, w, 1e-5, _p(o, off[2]), _p(o2, off[3]),
                                      _p(x, off[4]), w, 12, 0, s), 'misaligned')
    _refused(lib.ec_layernorm_hl8(_p(h), _p(l), w, _p(g, 4), _p(b), 2, w, 1e-5, _p(o), _p(o2), None, w, 12, 0, s), 'misaligned')


def test_layernorm_hl8_at_a_row_stride(hip):
    """ec_layernorm_hl8 with ldo = width + 64 at width 260: the 16-bit part against float64 and bit-identical to
    ec_layernorm_hl's, the e4m3 bytes at BYTE row pitch 2 ldo -- the hi copy torch's own e4m3 rounding of the 16-bit part,
    the lo bytes the lo part to e4m3's 2^-4 -- and every byte beyond `width` of each 2 ldo-byte row as it was."""
    lib, s = _L().lib(), _L().stream_ptr()
    rows, width, eps = 5, 260, 1e-5
    ldo = width + PAD
    gamma, beta = (t.cuda() for t in ref.gamma_beta(width))
    for rot in ref.rotations(rows):
        x, kind = ref.ln_rows(rows, width, rot)
        x_hi, x_lo = ref.split(x.cuda(), F16, F16)
        want, sc = ref.layernorm64(x_hi.double() + x_lo.double(), gamma, beta, eps)
        o_hi, o_lo = _layernorm('hl', None, [x_hi, x_lo], width, None, gamma, beta, rows, width, eps, F16)
        p_hi = _nan_buf(rows + 1, ldo, dtype=F16)
        lo8, hi8 = (torch.full((rows + 1, 2 * ldo), 0xAA, dtype=torch.uint8, device='cuda') for _ in range(2))
        _ok(lib.ec_layernorm_hl8(_p(x_hi), _p(x_lo), width, _p(gamma), _p(beta), rows, width, eps, _p(p_hi), _p(lo8), _p(hi8),
                                 ldo, 12, 0, s), 'ec_layernorm_hl8')
        _untouched(p_hi, rows, width, 'hl8 16-bit part')
        for b8 in (lo8, hi8):
            assert bool((b8[:rows, width:] == 0xAA).all()) and bool((b8[rows:] == 0xAA).all()), 'e4m3 bytes beyond width written'
        assert torch.equal(p_hi[:rows, :width], o_hi)
        e = ref.ln_e(sc, kind)
        _within(p_hi[:rows, :width], want, ref.bound16(want, e, F16), f'hl8 rot={rot} hi')
        want_hi8 = o_hi.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(hi8[:rows, :width], want_hi8)
        # lo = e4m3((LN - hi) 2^12) 2^-12: half an e4m3 ulp (2^-4) of the true lo part, e4m3's subnormal step (2^-9) at that
        # scale, and the fp32 term
        lo = lo8[:rows, :width].contiguous().view(torch.float8_e4m3fn).float().double() * 2.0 ** -12
        true_lo = want - o_hi.double()
        _within(lo, true_lo, 2.0 ** -4 * true_lo.abs() + 2.0 ** -21 + 2 * e, f'hl8 rot={rot} lo')
        lo8b = torch.full_like(lo8, 0x55)
        _ok(lib.ec_layernorm_hl8(_p(x_hi), _p(x_lo), width, _p(gamma), _p(beta), rows, width, eps, _p(p_hi), _p(lo8b), None,
                                 ldo, 12, 0, s), 'ec_layernorm_hl8 without the hi copy')
        assert torch.equal(lo8b[:rows, :width], lo8[:rows, :width]) and bool((lo8b[:rows, width:] == 0x55).all())


# ---------------------------------------------------------------------------------------------------------------
# row statistics and their merge
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('width', ref.STATS_WIDTHS)
def test_row_stats(width, dt, hip):
    """ec_row_stats: one lane with data (8), a partial last chunk (504, 520, 2040), four chunks per lane (2048); rows packed
    and at stride 5 width; large-mean, near-epsilon and constant rows (1 / sqrt(eps) and -mean / sqrt(eps))."""
    lib, s = _L().lib(), _L().stream_ptr()
    dtype = DT[dt]
    for rows in ref.ROWS:
        for rot in ref.rotations(rows):
            x32, kind = ref.ln_rows(rows, width, rot)
            x = x32.cuda().to(dtype)
            xmax = x.double().abs().amax(-1)
            for mul in (1, 5):
                src = _strided(x, mul)
                for eps in ref.EPS:
                    stats = _nan_buf(rows + 1, 2, dtype=F32)
                    _ok(lib.ec_row_stats(_p(src), mul * width, rows, width, eps, _p(stats), _code(dtype), s), 'ec_row_stats')
                    _untouched(stats, rows, 2, 'ec_row_stats')
                    want = ref.row_stats64(x, eps)
                    what = f'row_stats {dt} {rows}x{width} rot={rot} ldx={mul}w eps={eps}'
                    _within(stats[:rows], want, ref.stats_bound(want, xmax, kind), what)
                    const = (kind == ref.CONSTANT).cuda()
                    if bool(const.any()):
                        flat = torch.stack([torch.full_like(xmax, eps ** -0.5), -x[:, 0].double() * eps ** -0.5], -1)
                        _within(stats[:rows][const], flat[const], ref.stats_bound(flat, xmax, kind)[const], what + ' constant rows')


def test_row_stats_refusals(hip):
    lib, s = _L().lib(), _L().stream_ptr()
    x = torch.zeros(4, 64, dtype=F16, device='cuda')
    st = torch.zeros(4, 2, device='cuda')
    for width in (772, 2056):
        _refused(lib.ec_row_stats(_p(x), width, 1, width, 1e-5, _p(st), 0, s), 'multiple of 8')
    _refused(lib.ec_row_stats(_p(x, 2), 64, 2, 64, 1e-5, _p(st), 0, s), 'misaligned')
    _refused(lib.ec_row_stats(_p(x), 64, 2, 64, 1e-5, _p(st), 7, s), 'unknown dtype')
    assert lib.ec_row_stats(None, 64, 0, 64, 1e-5, None, 0, s) == 0
    _refused(lib.ec_row_stats_merge(_p(st), 1, 4, 320, 1e-5, _p(st), s), '64 x')
    assert lib.ec_row_stats_merge(None, 0, 4, 256, 1e-5, None, s) == 0


@pytest.mark.parametrize('groups', ref.MERGE_GROUPS)
def test_row_stats_merge(groups, hip):
    """ec_row_stats_merge on sums built directly (no GEMM in front): up to and past the sixteen lanes of a row (15, 16,
    17, 31, 32 groups), up to and past the sixteen rows of a workgroup, sums of f16 and of bf16 rows.  Where E[x^2] -
    mean^2 goes below zero (the large-mean rows, all but constant in 16 bit) and on the constant rows the result is
    1 / sqrt(eps) within the bound, and nothing is NaN."""
    lib, s = _L().lib(), _L().stream_ptr()
    width = 64 * groups
    for rows in ref.MERGE_ROWS:
        for rot in ref.rotations(rows):
            for dtype in (F16, BF16):
                sums, kind = ref.merge_sums(rows, groups, dtype, rot)
                sums = sums.cuda()
                for eps in ref.EPS:
                    stats = _nan_buf(rows + 1, 2, dtype=F32)
                    _ok(lib.ec_row_stats_merge(_p(sums), rows, groups, width, eps, _p(stats), s), 'ec_row_stats_merge')
                    _untouched(stats, rows, 2, 'ec_row_stats_merge')
                    want, cond, absum = ref.merge64(sums, width, eps)
                    bound = ref.merge_bound(want, cond, absum)
                    what = f'merge {rows} rows, {groups} groups, sums of {dtype}, rot={rot}, eps={eps}'
                    _within(stats[:rows], want, bound, what)
                    flat = (kind == ref.CONSTANT).cuda() | (ref.merge64(sums, width, 0.0)[1] == float('inf'))
                    if bool(flat.any()):
                        got = stats[:rows, 0][flat].double()
                        assert float(((got - eps ** -0.5).abs() - bound[flat, 0]).max()) <= 0, what + ': flat rows'


# ---------------------------------------------------------------------------------------------------------------
# splits and joins
# ---------------------------------------------------------------------------------------------------------------
def _split(api, x, n, gelu, dtype):
    lib, s = _L().lib(), _L().stream_ptr()
    lo_dtype = F16 if api == 'split_hl' else dtype
    hi, lo = _nan_buf(1, n + PAD, dtype=dtype), _nan_buf(1, n + PAD, dtype=lo_dtype)
    if api == 'split_hl':
        rc = lib.ec_split_hl(_p(x), n, _p(hi), _p(lo), _code(dtype), s)
    else:
        rc = lib.ec_split16(_p(x), n, gelu, _p(hi), _p(lo), _code(dtype), s)
    _ok(rc, api)
    for buf in (hi, lo):
        fill = _bits(torch.full((1,), NAN, dtype=buf.dtype, device='cuda'))[0]
        assert bool((_bits(buf)[0, n:] == fill).all()), f'{api} n={n}: elements behind the last written'
    return hi[0, :n], lo[0, :n], lo_dtype


def _check_split(api, x, n, gelu, dtype, what):
    hi, lo, lo_dtype = _split(api, x, n, gelu, dtype)
    if not gelu:
        want_hi = x.to(dtype)
        assert torch.equal(hi, want_hi), what + ': hi'
        assert torch.equal(lo, (x - want_hi.float()).to(lo_dtype)), what + ': lo'
        return
    want = ref.gelu64(x)
    e = ref.gelu_e(x, want)
    _within(hi, want, ref.bound16(want, e, dtype), what + ' hi')
    assert bool(torch.isfinite(lo).all())
    _within(hi.double() + lo.double(), want, ref.bound_pair(want, e, dtype, lo_dtype), what + ' hi + lo')


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('api,gelu', [('split16', 0), ('split16', 1), ('split_hl', 0)])
def test_splits(api, gelu, dt, hip):
    """ec_split16 and ec_split_hl (lo in fp16 whatever the type) at one vector, just under and just over a workgroup's
    1024 elements: without the activation both parts bit-identical to torch's roundings, with it float64 QuickGELU
    (inputs around +-20 and +-60 among them)."""
    for n in ref.SPLIT_N:
        _check_split(api, ref.split_input(n).cuda(), n, gelu, DT[dt], f'{api} {dt} n={n} gelu={gelu}')


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('api', ['split16', 'split_hl'])
def test_splits_take_a_second_trip(api, dt, hip):
    """n = 65536 x 1024 + 1028: the grid is capped at 65536 workgroups and 257 threads go round a second time (the precise
    chain reaches this at some 64 ViT-L images).  Input and references are built on the device."""
    n = ref.SPLIT_N_LARGE
    x = ref.split_input(n, device='cuda')
    _check_split(api, x, n, 0, DT[dt], f'{api} {dt} n={n}')
    if api == 'split16':
        _check_split(api, x, n, 1, DT[dt], f'{api} {dt} n={n} gelu')


def test_split_refusals(hip):
    lib, s = _L().lib(), _L().stream_ptr()
    x = torch.zeros(64, device='cuda')
    h, l = (torch.zeros(64, dtype=F16, device='cuda') for _ in range(2))
    out = torch.zeros(64, device='cuda')
    _refused(lib.ec_split16(_p(x), 6, 0, _p(h), _p(l), 0, s), 'multiple of 4')
    _refused(lib.ec_split16(_p(x), 8, 0, _p(h), _p(l), 7, s), 'unknown dtype')
    _refused(lib.ec_split_hl(_p(x), 6, _p(h), _p(l), 0, s), 'bad arguments')
    _refused(lib.ec_split_hl(_p(x), 8, _p(h), _p(l), 7, s), 'unknown dtype')
    assert lib.ec_split16(None, 0, 0, None, None, 0, s) == 0
    assert lib.ec_split_hl(_p(x), 0, _p(h), _p(l), 0, s) == 0
    for off in [(4, 0, 0), (0, 2, 0), (0, 0, 2)]:
        _refused(lib.ec_split16(_p(x, off[0]), 8, 0, _p(h, off[1]), _p(l, off[2]), 0, s), 'misaligned')
        _refused(lib.ec_split_hl(_p(x, off[0]), 8, _p(h, off[1]), _p(l, off[2]), 0, s), 'misaligned')
        _refused(lib.ec_join_hl_rows(_p(h, off[1]), _p(l, off[2]), 8, 2, 8, _p(out, off[0]), 0, s), 'misaligned')
    _refused(lib.ec_join_hl_rows(_p(h), _p(l), 8, 2, 6, _p(out), 0, s), 'bad shape')
    _refused(lib.ec_join_hl_rows(_p(h), _p(l), 8, 2, 8, _p(out), 7, s), 'unknown dtype')
    assert lib.ec_join_hl_rows(None, None, 8, 0, 8, None, 0, s) == 0


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('rows,width', ref.JOIN_SHAPES)
def test_join_rows(rows, width, dt, hip):
    """ec_join_hl_rows: bit-identical to hi.float() + lo.float(), planes at row stride width + 64 with NaN between the
    rows; 4104 x 1024 is one trip past the 4096-workgroup cap."""
    lib, s = _L().lib(), _L().stream_ptr()
    dtype = DT[dt]
    g = torch.Generator(device='cuda').manual_seed(rows + width)
    ld = width + PAD
    hi, lo = _nan_buf(rows, ld, dtype=dtype), _nan_buf(rows, ld, dtype=F16)
    hi[:, :width] = (torch.randn(rows, width, device='cuda', generator=g) * 3).to(dtype)
    lo[:, :width] = (torch.randn(rows, width, device='cuda', generator=g) * 2e-3).half()
    out = _nan_buf(rows + 1, width, dtype=F32)
    _ok(lib.ec_join_hl_rows(_p(hi), _p(lo), ld, rows, width, _p(out), _code(dtype), s), 'ec_join_hl_rows')
    _untouched(out, rows, width, 'ec_join_hl_rows')
    assert torch.equal(out[:rows], hi[:, :width].float() + lo[:, :width].float())


# ---------------------------------------------------------------------------------------------------------------
# embeddings
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('api', ['embed', 'embed_train', 'embed_hl float16', 'embed_hl bfloat16'])
@pytest.mark.parametrize('width', ref.EMBED_WIDTHS)
def test_vit_embed(width, api, hip):
    """ec_vit_embed, ec_vit_embed_train and ec_vit_embed_hl: the class row in every image, patch row n (seq - 1) + (s - 1)
    at [n, s]; `pre` bit-identical to the fp32 sum, the normalised rows against float64 LayerNorm of that sum (hi + lo for
    the planes, hi within half a 16-bit ulp besides)."""
    lib, s = _L().lib(), _L().stream_ptr()
    gamma, beta = (t.cuda() for t in ref.gamma_beta(width))
    for n_img, seq in ref.EMBED_SHAPES:
        patch, cls, pos = (t.cuda() for t in ref.embed_inputs(n_img, seq, width))
        rows = n_img * seq
        pre_want = ref.embed_sum(patch, cls, pos, n_img, seq)
        kind = torch.zeros(rows, dtype=torch.int64)
        for eps in ref.EPS:
            want, sc = ref.layernorm64(pre_want, gamma, beta, eps)
            e = ref.ln_e(sc, kind)
            what = f'{api} {n_img}x{seq}x{width} eps={eps}'
            head = (_p(patch), _p(cls), _p(pos), _p(gamma), _p(beta), n_img, seq, width, eps)
            if api.startswith('embed_hl'):
                dtype = DT[api.split()[1]]
                hi, lo = _nan_buf(rows + 1, width, dtype=dtype), _nan_buf(rows + 1, width, dtype=F16)
                _ok(lib.ec_vit_embed_hl(*head, _p(hi), _p(lo), _code(dtype), s), api)
                _untouched(hi, rows, width, what), _untouched(lo, rows, width, what)
                _within(hi[:rows], want, ref.bound16(want, e, dtype), what + ' hi')
                assert bool(torch.isfinite(lo[:rows]).all())
                _within(hi[:rows].double() + lo[:rows].double(), want, ref.bound_pair(want, e, dtype, F16), what + ' hi + lo')
                continue
            x = _nan_buf(rows + 1, width, dtype=F32)
            if api == 'embed':
                _ok(lib.ec_vit_embed(*head, _p(x), s), api)
            else:
                pre = _nan_buf(rows + 1, width, dtype=F32)
                _ok(lib.ec_vit_embed_train(*head, _p(x), _p(pre), s), api)
                _untouched(pre, rows, width, what + ' pre')
                assert torch.equal(pre[:rows], pre_want), what + ': pre'
            _untouched(x, rows, width, what)
            _within(x[:rows], want, e, what)


def test_embed_refusals(hip):
    lib, s = _L().lib(), _L().stream_ptr()
    w = 8
    f = [torch.zeros(4 * w, device='cuda') for _ in range(7)]      # patch, cls, pos, gamma, beta, x, pre
    h, l = (torch.zeros(4 * w, dtype=F16, device='cuda') for _ in range(2))
    ptrs = [_p(t) for t in f]
    _refused(lib.ec_vit_embed(*ptrs[:5], 1, 1, w, 1e-5, ptrs[5], s), 'bad shape')
    _refused(lib.ec_vit_embed_train(*ptrs[:5], 1, 1, w, 1e-5, ptrs[5], ptrs[6], s), 'bad shape')
    _refused(lib.ec_vit_embed_hl(*ptrs[:5], 1, 1, w, 1e-5, _p(h), _p(l), 0, s), 'bad shape')
    _refused(lib.ec_vit_embed(*ptrs[:5], 1, 2, 6, 1e-5, ptrs[5], s), 'bad shape')
    _refused(lib.ec_vit_embed(*ptrs[:5], 1, 2, 2052, 1e-5, ptrs[5], s), 'bad shape')
    _refused(lib.ec_vit_embed_hl(*ptrs[:5], 1, 2, w, 1e-5, _p(h), _p(l), 7, s), 'unknown dtype')
    assert lib.ec_vit_embed(None, None, None, None, None, 0, 2, w, 1e-5, None, s) == 0
    assert lib.ec_vit_embed_train(None, None, None, None, None, 0, 2, w, 1e-5, None, None, s) == 0
    assert lib.ec_vit_embed_hl(None, None, None, None, None, 0, 2, w, 1e-5, None, None, 0, s) == 0
    for k in range(7):
        off = [_p(t, 4 if i == k else 0) for i, t in enumerate(f)]
        _refused(lib.ec_vit_embed_train(*off[:5], 1, 2, w, 1e-5, off[5], off[6], s), 'misaligned')
        if k < 5:
            _refused(lib.ec_vit_embed_hl(*off[:5], 1, 2, w, 1e-5, _p(h), _p(l), 0, s), 'misaligned')
    _refused(lib.ec_vit_embed_hl(*ptrs[:5], 1, 2, w, 1e-5, _p(h, 2), _p(l), 0, s), 'misaligned')
    _refused(lib.ec_vit_embed_hl(*ptrs[:5], 1, 2, w, 1e-5, _p(h), _p(l, 2), 0, s), 'misaligned')
    tok = torch.zeros(8, dtype=torch.int32, device='cuda')
    _refused(lib.ec_text_embed(_p(tok), ptrs[0], ptrs[1], 1, 2, 0, 4, ptrs[2], s), 'bad shape')
    _refused(lib.ec_text_embed(_p(tok), ptrs[0], ptrs[1], 1, 2, 6, 4, ptrs[2], s), 'bad shape')
    _refused(lib.ec_text_embed(_p(tok), ptrs[0], ptrs[1], 1, 0, w, 4, ptrs[2], s), 'bad shape')
    assert lib.ec_text_embed(None, None, None, 0, 2, w, 4, None, s) == 0
    for k in range(3):
        off = [_p(t, 4 if i == k else 0) for i, t in enumerate(f[:3])]
        _refused(lib.ec_text_embed(_p(tok), off[0], off[1], 1, 2, w, 4, off[2], s), 'misaligned')
    _refused(lib.ec_text_embed(_p(tok, 2), ptrs[0], ptrs[1], 1, 2, w, 4, ptrs[2], s), 'misaligned')


@pytest.mark.parametrize('ctx', ref.TEXT_CTX)
@pytest.mark.parametrize('width', ref.TEXT_WIDTHS)
def test_text_embed(width, ctx, hip):
    """ec_text_embed: bit-identical to table[clamp(token, 0, vocab - 1)] + pos[s] in fp32, tokens -5, 0, vocab - 1, vocab
    and vocab + 7 among them; at width 1280 a lane's column loop runs five times."""
    lib, s = _L().lib(), _L().stream_ptr()
    n_txt = 7
    tok, table, pos = (t.cuda() for t in ref.text_inputs(n_txt, ctx, width))
    rows = n_txt * ctx
    x = _nan_buf(rows + 1, width, dtype=F32)
    _ok(lib.ec_text_embed(_p(tok), _p(table), _p(pos), n_txt, ctx, width, ref.TEXT_VOCAB, _p(x), s), 'ec_text_embed')
    _untouched(x, rows, width, 'ec_text_embed')
    assert torch.equal(x[:rows].view(n_txt, ctx, width), ref.text_embed_ref(tok, table, pos))
