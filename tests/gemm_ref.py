"""Float64 yardsticks, directed inputs, error bounds and shape tables for csrc/gemm.hip: the product A W^T + bias with
every epilogue of ops.gemm, the segmented (split-precision and e4m3) products, the lo outputs, K splits and the
transposed form of ops.gemm_rows.

Nothing here touches a GPU or anything compiled: the references are plain torch float64 and run on whatever device their
input lives on, the inputs are built on the CPU from a seed, the fp32 restatements (fp32 products summed in K blocks of
32, a tree inside a block, the blocks in order) give the same bits on any machine.  tests/test_gemm_ref_cpu.py measures
the constants below with them and runs the checks against a tile model with planted faults; tests/test_gemm_edges_gpu.py
holds the kernels to the same checks.

Bounds, per element, never the largest error over the largest value:
    fp32 output:     |got - ref|     <= E
    16-bit output:   |got - ref|     <= u |ref| + FLOOR16 + E
    hi + lo:         |hi + lo - ref| <= pair_u |ref| + FLOOR_PAIR + E
    E = KERNEL_FACTOR c_acc(K_total) 2^-24 S,   S[m, n] = sum_k |a| |w| + |bias| (+ |resid|, + |hi| + |lo|)
S and not |ref|: fp32 accumulation loses against the magnitude that went through the accumulator, and the directed rows
whose product cancels (|ref| << S) are held to what fp32 can give, not to nothing.  Through QuickGELU E is multiplied by
the activation's largest slope (1.1) and rowops_ref's fp32 term of the activation itself is added.
"""
import functools
import math

import torch

import rowops_ref as rr
from rowops_ref import FLOOR16, FLOOR_PAIR, U, excess, pair_u, split  # noqa: F401  (the GPU tests take them from here)

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = rr.DTYPES
EPS24 = 2.0 ** -24
KERNEL_FACTOR = 4.0          # the matrix pipe's unknown summation order inside a 32-deep MFMA and across K tiles, nothing more
GELU_SLOPE = 1.1             # max |QuickGELU'| (1.0999 at x = 1.49)
LN_EPS = 1e-5
PAD = 64                     # padding columns of every output / operand buffer; one guard row behind the last

# ---------------------------------------------------------------------------------------------------------------
# The measured constants (tests/test_gemm_ref_cpu.py; the measurements are in the comments, the figures are those rounded
# up; the test asserts measured <= figure <= 1.5 measured).  No constant is derived from what a kernel returns.
# ---------------------------------------------------------------------------------------------------------------
# Accumulation: the fp32 restatement (product32 + the epilogue's fp32 additions) against float64, in units of 2^-24 S, over
# the random family.  K_total <= 576: single products of 1 .. 9 K tiles and the segmented products (16-bit and e4m3 parts) of
# K = 64, 128, 192, over the whole base arrays.  K_total <= 4096: every prefix of 1 .. 64 K tiles, every single K tile at its
# column offset (K splits, gemm_rows' batches) and the e4m3 segments of K = 256, 384, every base row of A against 272 rows of
# W.  The worst element barely moves with K (3.5 .. 4.0 at one K tile, 2.7 .. 3.0 at nine: the sums are random walks of
# rounding errors against an S that grows linearly; the worst rows are the cancelling ones, whose S sits in 16 columns of a
# K tile), so one figure per range serves.  Measured: 4.34 (K_total <= 576), 4.62 (<= 4096: a single K tile further along).
C_ACC_TABLE = ((576, 4.6), (4096, 4.9))
# The LayerNorm fold rstd acc + (negrm colsum + b) in fp32 given the SAME fp32 acc, in units of 2^-24 S_ln,
# S_ln = |rstd| S + |negrm colsum| + |b|: three roundings, and the cancellation between the two large terms is in S_ln.
# Measured: 1.61.
C_FOLD = 1.8
# QuickGELU' in fp32 (grad32 against grad64) in units of 2^-23 s (1 + |1.702 x|)^2, s = sigmoid(1.702 x).  Measured: 1.74.
C_GRAD = 1.9
# 64-column group sums of the hi plane (left to right in fp32 against float64): the sum in units of 2^-24 sum|h|, the sum of
# squares in units of 2^-24 sum h^2.  Measured: 8.64.
C_ROWSUM = 9.5


def c_acc(k_total):
    for k, c in C_ACC_TABLE:
        if k_total <= k:
            return c
    raise ValueError(f'no accumulation constant measured for K_total = {k_total}')


# ---------------------------------------------------------------------------------------------------------------
# shape tables the CPU and GPU tests share
# ---------------------------------------------------------------------------------------------------------------
EDGE_M = (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 255, 256, 257, 513)
EDGE_N = (16, 48, 64, 192, 240, 256, 272, 320, 528)
NK = (1, 2, 3, 4, 5)                 # K tiles of 64
EPILOGUES = ('store16', 'gelu16', 'store32', 'resid32', 'resid32_oop', 'gelu16_save', 'gelu_bwd16', 'resid_hl',
             'store16_ln', 'gelu16_ln')
OUT32 = ('store32', 'resid32', 'resid32_oop')
WS_EPILOGUES = ('store16', 'gelu16', 'store32', 'resid32', 'resid32_oop', 'gelu16_save', 'gelu_bwd16')
SEG_EPILOGUES = ('store16', 'gelu16', 'store32', 'resid32', 'resid_hl')
F8_EPILOGUES = ('store16', 'gelu16', 'store32', 'resid_hl')
GELU_TAILS = (-100.0, -60.0, -20.0, -1.0, 0.0, 1.0, 20.0, 60.0, 100.0)
ROWS_T = (1, 63, 64, 65, 129, 200)
ROWS_M = (8, 16, 72, 248, 256, 264)
ROWS_N = (16, 80, 256, 272)
RASTER_TM = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)
RASTER_TN = (1, 2, 3, 4, 5, 8)
WS_SHAPES = ((1, 16), (257, 272), (513, 1024))
WS_NK = (2, 4, 6, 8, 64)
KMAX = 4096
PERIOD_M, PERIOD_N = 1031, 1049      # primes: row m of A is row m % 1031 of one base array, row n of W is n % 1049


def exact_limit(epi, dtype):
    """max S at which every partial sum, in any order, and the stored result are exact."""
    if epi in OUT32:
        return 2 ** 24 - 1
    return 256 if dtype == BF16 else 2048


def rotations(M):
    """The row pattern of random_operands has period 8 (ordinary, ordinary, cancelling, zero, ...): a case with fewer than four
    rows is run at the rotations that bring a cancelling and a zero row to the front."""
    return (0, 2, 3) if M < 4 else (0,)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _random_base():
    """-> (A fp32 [PERIOD_M, KMAX], W fp32 [PERIOD_N, KMAX], bias fp32 [PERIOD_N]); read-only.  Base row r of A by r % 8:
    0, 1, 4, 6, 7 Gaussian scaled by 2^(r % 6 - 3) (2^-3 .. 2^2) plus a row mean of 0.25 ((5 r) % 7 - 3) of that scale (the
    LayerNorm epilogues: means and deviations differ from row to row by far more than any bound);  2, 5 rows that CANCEL:
    nonzero only in the first 16 columns of each K tile, a[2 j + 1] = -a[2 j], where W has w[2 j + 1] = w[2 j]: the product is
    exactly 0 and the reference is the bias alone while S is as large as anywhere;  3 all zero.
    Column 7 of every K tile of A is an outlier channel (x 40)."""
    g = _gen(4242)
    r = torch.arange(PERIOD_M)
    k = torch.arange(KMAX)
    scale = (2.0 ** (r % 6 - 3).double())[:, None]
    a = torch.randn(PERIOD_M, KMAX, generator=g, dtype=torch.float64) * scale
    a = a + 0.25 * ((5 * r) % 7 - 3).double()[:, None] * scale
    a[:, k % 64 == 7] *= 40
    w = torch.randn(PERIOD_N, KMAX, generator=g, dtype=torch.float64) / 8
    pair = (k % 64 < 16)
    odd, even = pair & (k % 2 == 1), pair & (k % 2 == 0)
    w[:, odd] = w[:, even]
    cancel = ((r % 8 == 2) | (r % 8 == 5))[:, None]
    c = torch.zeros_like(a)
    c[:, even] = a[:, even]
    c[:, odd] = -a[:, even]
    a = torch.where(cancel, c, a)
    a = torch.where((r % 8 == 3)[:, None], torch.zeros_like(a), a)
    bias = torch.randn(PERIOD_N, generator=g, dtype=torch.float64) * 2
    return a.float(), w.float(), bias.float()


def random_operands(M, N, K, rot=0):
    """-> (A fp32 [M, K], W fp32 [N, K], bias fp32 [N]): row m is base row (m + rot) % PERIOD_M.  Round to the operand dtype
    with .to(dtype) (the cancelling rows stay cancelling: negation and copies survive any rounding) or split()."""
    a, w, b = _random_base()
    rows = (torch.arange(M) + rot) % PERIOD_M
    cols = torch.arange(N) % PERIOD_N
    return a[rows, :K].contiguous(), w[cols, :K].contiguous(), b[cols].contiguous()


def exact_operands(M, N, K, limit, nseg=1, extra=0, device='cpu'):
    """Small-integer operands with max S <= limit: every partial sum in any order is exact.  -> (A, W, bias) fp32 integers.
    A has nz nonzeros per 64-wide K tile (1 when limit <= 256, the bf16 case; 8 up to 2048; all 64 beyond) at positions that
    depend on m and on the K tile, values that depend on m, the K tile and the position; W is nonzero everywhere and depends
    on n, k, n's 16-column group and k's K tile; the bias depends on n and its group.  `extra`: magnitude reserved for what
    the epilogue adds (residual, planes)."""
    nk = K // 64
    nz = 1 if limit <= 256 else 8 if limit <= 2048 else 64
    amax = max(1, min(4, (limit - 4 - extra) // (3 * nz * nk * nseg)))
    assert amax * 3 * nz * nk * nseg + 4 + extra <= limit, (M, N, K, limit)
    ar = functools.partial(torch.arange, device=device)     # (integer rules: the same values wherever they are evaluated)
    m, n, k = ar(M)[:, None], ar(N)[:, None], ar(K)[None]
    t = k >> 6
    h = (131 * n + 31 * k + (n * k) % 239 + 17 * (n >> 4) + 7 * t) % 251
    W = (1 + h % 3) * (1 - 2 * ((h // 3) % 2))
    if nz == 64:
        A = ((137 * m + 29 * k + (m * k) % 251 + 19 * (m >> 4) + 11 * t) % 241) % (2 * amax + 1) - amax
    else:
        A = torch.zeros(M, K, dtype=torch.int64, device=device)
        tt = ar(nk)[None]
        for j in range(nz):
            p = ((7 + 4 * tt) * m + 13 * tt + 17 * j + (m >> 4) * (tt + 1) + 5 * (m >> 8)) % 64
            v = (1 + (m + 2 * tt + j) % amax) * (1 - 2 * ((m + tt + j) % 3 == 0).long())
            A.scatter_(1, tt * 64 + p, v.expand(M, nk))
    nn = ar(N)
    bias = (3 * nn + (nn >> 4)) % 9 - 4
    return A.float(), W.float(), bias.float()


@functools.lru_cache(maxsize=8)
def exact_plane(M, N, mod, mul=1):
    """Integer [M, N] in (-mod / 2, mod / 2) that depends on m and n (residuals, planes); read-only."""
    m, n = torch.arange(M)[:, None], torch.arange(N)[None]
    return (((3 * m + 2 * n + (m >> 4) + (n >> 4)) * mul) % mod - mod // 2).float()


@functools.lru_cache(maxsize=8)
def random_plane(M, N, seed, scale=3.0):
    """fp32 [M, N] Gaussian x scale with a row offset: residuals, planes, saved pre-activations of the random family;
    read-only."""
    g = _gen(8800 + seed)
    base = torch.randn(PERIOD_M, 1100, generator=g) * scale
    base = base + 0.5 * (torch.arange(PERIOD_M) % 5 - 2)[:, None]
    return base[torch.arange(M) % PERIOD_M][:, :N].contiguous()


def tails_bias(N):
    """bias [N] fp32: GELU_TAILS on consecutive columns."""
    return torch.tensor(GELU_TAILS, dtype=torch.float32)[torch.arange(N) % len(GELU_TAILS)]


def quantize_e4m3(x, pitch, exp=None):
    """x [rows, K] -> (uint8 [rows, pitch], exp): the first K bytes of a row hold round_e4m3(x 2^exp) (OCP e4m3fn, saturating
    at +-448), the layout of ec_gemm_args' e4m3 operands; the bytes behind them are 0x7f (an e4m3 NaN: read, they poison).
    exp=None: the largest |x| lands in [128, 256)."""
    xf = x.detach().float()
    if exp is None:
        m = float(xf.abs().max())
        exp = 8 - int(math.ceil(math.log2(m))) if m > 0 else 0
    q = (xf * (2.0 ** exp)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    out = torch.full((x.shape[0], pitch), 0x7f, dtype=torch.uint8, device=x.device)
    out[:, :x.shape[1]] = q
    return out, exp


def dequantize_e4m3(t, exp, K):
    """float64 values an e4m3 operand stands for."""
    return t[:, :K].contiguous().view(torch.float8_e4m3fn).double() * (2.0 ** -exp)


def ln_stats(A16, stride=1):
    """(rstd, -rstd mean) fp32 [M, 2] of the 16-bit rows (float64, rounded once) -> (pairs [M, 2] as the kernel must read them,
    the array to hand over: at stride > 1 a NaN-interleaved [M, stride, 2] whose [:, 0] are the pairs)."""
    st = rr.row_stats64(A16, LN_EPS).float()
    if stride == 1:
        return st, st.contiguous()
    buf = torch.full((A16.shape[0], stride, 2), float('nan'), dtype=torch.float32, device=A16.device)
    buf[:, 0] = st
    return st, buf


def col_sums(W16):
    return W16.double().sum(1).float()


# ---------------------------------------------------------------------------------------------------------------
# references (float64) and the fp32 restatement
# ---------------------------------------------------------------------------------------------------------------
def product(segs):
    """segs: [(a [M, K], w [N, K]), ...] as given to the kernel (16-bit, dequantised e4m3) -> (sum of a w^T, S = sum of
    |a| |w|^T) in float64."""
    acc = s = 0
    for a, w in segs:
        a, w = a.double(), w.double()
        acc = acc + a @ w.T
        s = s + a.abs() @ w.abs().T
    return acc, s


def product32(segs, korder=None):
    """The same in fp32 with a fixed order: the products of a K block of 32 summed as a tree, the blocks added in order, the
    segments in order (each product of two 16-bit or e4m3 values is exact in fp32).  korder: a permutation of K applied to
    both operands of every segment (the exact family: the bits may not depend on it)."""
    acc = None
    for a, w in segs:
        a, w = a.float(), w.float()
        if korder is not None:
            a, w = a[:, korder], w[:, korder]
        for k in range(0, a.shape[1], 32):
            blk = rr.tree_sum32(a[:, None, k:k + 32] * w[None, :, k:k + 32])
            acc = blk if acc is None else acc + blk
    return acc


def segments(A, W, A_lo=None, W_lo=None, a_lo8=None, w8=None, a8=None, w_lo8=None):
    """The kernel's products, the small ones first: a_lo w + a w_lo + a w without lo . lo; an e4m3 pair (already dequantised)
    stands in for its 16-bit product."""
    segs = []
    if a_lo8 is not None:
        segs.append((a_lo8, w8))
    if w_lo8 is not None:
        segs.append((a8, w_lo8))
    if A_lo is not None:
        segs.append((A_lo, W))
    if W_lo is not None:
        segs.append((A, W_lo))
    segs.append((A, W))
    return segs


def k_total(segs):
    return sum(a.shape[1] for a, _ in segs)


def grad64(x):
    x = x.double()
    s = 1 / (1 + torch.exp(-1.702 * x))
    return s * (1 + 1.702 * x * (1 - s))


def grad32(x):
    assert x.dtype == F32
    c = torch.tensor(1.702, dtype=F32)
    s = 1 / (1 + torch.exp(-c * x))
    return s * (1 + c * x * (1 - s))


def grad_e(x, factor=KERNEL_FACTOR):
    x = x.double()
    s = 1 / (1 + torch.exp(-1.702 * x))
    return factor * C_GRAD * rr.EPS32 * s * (1 + (1.702 * x).abs()) ** 2 + rr.FLOOR_GELU


def seq_sum32(x):
    """fp32 sum over the last axis, left to right."""
    acc = x[..., 0].clone()
    for i in range(1, x.shape[-1]):
        acc = acc + x[..., i]
    return acc


def restate(epi, dtype, acc32, bias=None, resid=None, hi=None, lo=None, u=None, stats=None, colsum=None, lo_out=None,
            aux_exp=0):
    """The epilogues in fp32 on an fp32 accumulator, one rounded operation after the other as csrc/gemm.hip writes them ->
    dict of the outputs ('out', 'aux', 'aux8' dequantised).  With product32 in front this is the fault-free restatement the
    constants are measured with and the checks must pass on."""
    assert acc32.dtype == F32
    b = torch.zeros((), dtype=F32) if bias is None else bias.float()[None]
    if epi in ('store16_ln', 'gelu16_ln'):
        v = acc32 * stats[:, :1].float() + (colsum.float()[None] * stats[:, 1:].float() + b)
    else:
        v = acc32 + b
    if epi == 'store32':
        return {'out': v}
    if epi in ('resid32', 'resid32_oop'):
        return {'out': v + resid.float()}
    if epi == 'resid_hl':
        x = (hi.float() + lo.float()) + v
        h = x.to(dtype)
        return {'out': h, 'aux': (x - h.float()).to(F16)}
    if epi == 'gelu_bwd16':
        return {'out': (v.to(dtype).float() * grad32(u.float())).to(dtype)}
    got = {}
    if epi == 'gelu16_save':
        got['aux'] = v.to(dtype)
    if epi in ('gelu16', 'gelu16_ln', 'gelu16_save'):
        v = rr.gelu32(v)
    got['out'] = v.to(dtype)
    if lo_out is not None:
        l32 = v - got['out'].float()
        if lo_out == '16':
            got['aux'] = l32.to(dtype)
        else:
            q = (l32 * 2.0 ** aux_exp).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
            got['aux8'] = q.double() * 2.0 ** -aux_exp
    return got


# ---------------------------------------------------------------------------------------------------------------
# what a launch must return: a list of (name, ref float64, bound float64 or None = bit for bit)
# name: 'out', 'aux', or a sum 'out+aux' (the caller hands aux8 over dequantised, as 'aux8')
# ---------------------------------------------------------------------------------------------------------------
def expect(epi, dtype, acc, S, ktot, bias=None, exact=False, resid=None, hi=None, lo=None, u=None, stats=None,
           colsum=None, lo_out=None):
    """epi: one of EPILOGUES.  acc, S: product().  exact: the exact family (the product is exact: c_acc = 0, and where the
    epilogue is exact too the expectation is bit for bit).  resid: fp32 residual (resid32*);  hi, lo: the planes (resid_hl);
    u: the saved pre-activation (gelu_bwd16);  stats [M, 2], colsum [N]: the LN epilogues;  lo_out: None, '16' or 'e4m3' (the
    lo output of a segmented store16 / gelu16)."""
    c = 0.0 if exact else c_acc(ktot)
    b = 0 if bias is None else bias.double()[None]
    u16 = U[dtype]
    if epi in ('store16_ln', 'gelu16_ln'):
        st = stats.double()
        r0, r1, cs = st[:, :1], st[:, 1:], colsum.double()[None]
        v = r0 * acc + r1 * cs + b
        s_ln = r0.abs() * S + (r1 * cs).abs() + (b.abs() if bias is not None else 0)
        e = KERNEL_FACTOR * EPS24 * (c * r0.abs() * S + C_FOLD * s_ln)
    else:
        v = acc + b
        S = S + (b.abs() if bias is not None else 0)
        if epi in ('resid32', 'resid32_oop'):
            v, S = v + resid.double(), S + resid.double().abs()
        if epi == 'resid_hl':
            v, S = v + hi.double() + lo.double(), S + hi.double().abs() + lo.double().abs()
        e = KERNEL_FACTOR * c * EPS24 * S
    if epi in OUT32:
        return [('out', v, None if exact else e)]
    if epi in ('store16', 'store16_ln'):
        specs = [('out', v, None if exact and epi == 'store16' else rr.bound16(v, e, dtype))]
    elif epi in ('gelu16', 'gelu16_ln', 'gelu16_save'):
        ref = rr.gelu64(v)
        eg = GELU_SLOPE * e + rr.gelu_e(v, ref)
        specs = [('out', ref, rr.bound16(ref, eg, dtype))]
        if epi == 'gelu16_save':
            specs.append(('aux', v, None if exact else rr.bound16(v, e, dtype)))
        v, e = ref, eg
    elif epi == 'gelu_bwd16':
        # out = round16(round16(acc + bias) QuickGELU'(u)): the inner rounding moves the product by u |v| + FLOOR16 + E at the
        # most (nothing in the exact family, where v is a 16-bit number), the derivative is an fp32 formula, the outer
        # rounding is the output's
        gd = grad64(u)
        ref = v * gd
        inner = 0 if exact else u16 * v.abs() + FLOOR16 + e
        eb = gd.abs() * inner * (1 + u16) + (v.abs() + inner) * grad_e(u)
        return [('out', ref, rr.bound16(ref, eb, dtype))]
    elif epi == 'resid_hl':
        if exact:
            return [('out', v, None), ('aux', torch.zeros_like(v), None)]
        return [('out', v, rr.bound16(v, e, dtype)), ('out+aux', v, rr.bound_pair(v, e, dtype, F16))]
    if lo_out == '16':
        specs.append(('out+aux', v, rr.bound_pair(v, e, dtype, dtype)))
    elif lo_out == 'e4m3':
        # aux8 = round_e4m3(lo 2^exp), lo = v32 - hi exactly (Sterbenz).  No measured constant here: the bound of check() is
        # rounding theory -- half an e4m3 ulp (3 mantissa bits: 2^-4 relative; half the subnormal step 2^-9 in scaled units)
        # of a lo that carries v32's own error E, which the rounding can enlarge by the same 2^-4.
        # tests/test_gemm_ref_cpu.py holds restate()'s byte to it with E = 0 against the restatement's own fp32 value.
        specs.append(('out+aux8', v, e))          # E itself: check() builds the bound around the hi part it got
    return specs


def check(specs, got, what, aux_exp=0):
    """got: dict name -> tensor ('out', 'aux', 'aux8' as dequantised float64).  Raises AssertionError naming the first
    output that is not finite, not within its bound, or (bound None) not the expectation itself."""
    for name, ref, bound in specs:
        if name == 'out+aux8':
            lo_true, e = ref - got['out'].double(), bound
            val, ref_, bnd = got['aux8'], lo_true, 2.0 ** -4 * lo_true.abs() + 2.0 ** (-10 - aux_exp) + (1 + 2.0 ** -4) * e
            assert bool((lo_true.abs() * 2.0 ** aux_exp <= 448).all()), f'{what}: aux_exp saturates the e4m3 lo output'
            over = excess(val, ref_, bnd)
            assert over <= 0, f'{what} {name}: {over:.3e} over the bound'
            continue
        val = sum(got[p].double() for p in name.split('+'))
        for p in name.split('+'):
            assert bool(torch.isfinite(got[p].float()).all()), f'{what} {p}: not finite'
        if bound is None:
            bad = val != ref
            assert not bool(bad.any()), f'{what} {name}: {int(bad.sum())} elements differ from the exact expectation, ' \
                                        f'first at {tuple(bad.nonzero()[0].tolist())}'
        else:
            over = excess(val, ref, bound)
            if over > 0:
                d = (val - ref).abs() - bound
                at = tuple((d == d.max()).nonzero()[0].tolist())
                raise AssertionError(f'{what} {name}: {over:.3e} over the bound at {at} '
                                     f'(got {float(val[at]):.6g}, want {float(ref[at]):.6g}, bound {float(bound[at]):.3e})')


def row_sums_check(row_sums, hi_got, what):
    """row_sums [M, N / 64, 2] against float64 sums of the hi plane the launch returned."""
    M, N = hi_got.shape
    h = hi_got.double().view(M, N // 64, 64)
    want = torch.stack([h.sum(-1), (h * h).sum(-1)], -1)
    bound = KERNEL_FACTOR * C_ROWSUM * EPS24 * torch.stack([h.abs().sum(-1), (h * h).sum(-1)], -1)
    assert tuple(row_sums.shape) == tuple(want.shape)
    over = excess(row_sums, want, bound)
    assert over <= 0, f'{what} row_sums: {over:.3e} over the bound'


# ---------------------------------------------------------------------------------------------------------------
# buffers: views [M, N] of NaN-filled [M + 1, N + PAD]; padding columns and the guard row must come back bit for bit
# ---------------------------------------------------------------------------------------------------------------
def padded(M, N, dtype, device='cpu', init=None, pad=PAD):
    """-> (buf [M + 1, N + pad] filled with NaN (0xAA bytes for uint8), view [M, N] holding `init` when given)."""
    if dtype == torch.uint8:
        buf = torch.full((M + 1, N + pad), 0xAA, dtype=dtype, device=device)
    else:
        buf = torch.full((M + 1, N + pad), float('nan'), dtype=dtype, device=device)
    view = buf[:M, :N]
    if init is not None:
        view.copy_(init)
    return buf, view


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def guards_intact(buf, M, N, what):
    fill = _bits(buf.new_full((1,), 0xAA if buf.dtype == torch.uint8 else float('nan')))[0]
    b = _bits(buf)
    assert bool((b[:M, N:] == fill).all()), f'{what}: padding columns written'
    assert bool((b[M:] == fill).all()), f'{what}: guard row written'


def window(x, fill_to=PAD, lead=0, extra_rows=0):
    """x [rows, K] -> a view [rows, K] at column `lead` of a NaN-filled [rows + extra_rows, K + fill_to] buffer (the operands:
    lda = ldw = K + 64, the window starting at column 0 or 64)."""
    rows, K = x.shape
    buf = torch.full((rows + extra_rows, K + fill_to), float('nan'), dtype=x.dtype, device=x.device)
    buf[:rows, lead:lead + K] = x
    return buf[:rows, lead:lead + K]


# ---------------------------------------------------------------------------------------------------------------
# cases: everything one launch is given, built on the CPU; the CPU tile model and the GPU tests run the SAME case through
# the SAME checks
# ---------------------------------------------------------------------------------------------------------------
SEGS16 = ('a_lo', 'w_lo', 'both')
SEGS8 = ('a_lo8', 'w_lo8', 'both8', 'a_lo8+w_lo')


def make_case(epi, dtype, M, N, K, family, rot=0, seg=None, lo_out=None):
    """-> dict of CPU tensors.  family: 'exact' | 'random' | 'tails' (zero rows of A under GELU_TAILS as the bias; gelu_bwd16:
    random rows, the tails as the saved pre-activation).  seg: None, one of SEGS16 (A_lo / W_lo / both) or SEGS8 (the e4m3
    pairs, f16 only)."""
    exact = family == 'exact'
    nseg = 1 if seg is None else 3 if seg in ('both', 'both8', 'a_lo8+w_lo') else 2
    c = dict(epi=epi, dtype=dtype, M=M, N=N, K=K, family=family, exact=exact, seg=seg, lo_out=lo_out, aux_exp=0)
    if exact:
        limit = exact_limit(epi, dtype)
        a32, w32, bias = exact_operands(M, N, K, limit, nseg, extra=10)
        c['limit'] = limit
    else:
        a32, w32, bias = random_operands(M, N, K, rot)
        if family == 'tails':
            bias = tails_bias(N)
            if epi != 'gelu_bwd16':
                a32 = torch.zeros_like(a32)
    c['A'], c['W'], c['bias'] = a32.to(dtype), w32.to(dtype), bias
    if seg is not None:
        if exact:
            a_lo = exact_operands(M + 5, N, K, limit, nseg, extra=10)[0][5:]
            w_lo = exact_operands(M, N + 3, K, limit, nseg, extra=10)[1][3:]
        else:
            a_lo, w_lo = a32 - c['A'].float(), w32 - c['W'].float()
        if seg in ('a_lo', 'both'):
            c['A_lo'] = a_lo.to(dtype)
        if seg in ('w_lo', 'both', 'a_lo8+w_lo'):
            c['W_lo'] = w_lo.to(dtype)
        ex = 0 if exact else None
        if seg in ('a_lo8', 'both8', 'a_lo8+w_lo'):
            c['A_lo8'], c['W8'] = quantize_e4m3(a_lo, 2 * (K + PAD), ex), quantize_e4m3(c['W'].float(), 2 * (K + PAD), ex)
        if seg in ('w_lo8', 'both8'):
            c['A8'], c['W_lo8'] = quantize_e4m3(c['A'].float(), 2 * (K + PAD), ex), quantize_e4m3(w_lo, 2 * (K + PAD), ex)
    return with_epilogue(c, epi, lo_out)


def with_epilogue(base, epi, lo_out=None):
    """The case of another epilogue on the same operands (which may live on a GPU already: what the epilogue adds is built
    on the CPU and moved there)."""
    c = {k: v for k, v in base.items() if k not in ('resid', 'hi', 'lo', 'u', 'stats', 'colsum')}
    c.update(epi=epi, lo_out=lo_out, aux_exp=0)
    M, N, dtype, exact, dev = c['M'], c['N'], c['dtype'], c['exact'], c['A'].device
    if epi in ('resid32', 'resid32_oop'):
        c['resid'] = (exact_plane(M, N, 11) if exact else random_plane(M, N, 1)).to(dev)
    if epi == 'resid_hl':
        x = exact_plane(M, N, 17) if exact else random_plane(M, N, 2)
        hi, lo = (x.to(dtype), exact_plane(M, N, 5, 3).to(F16)) if exact else split(x, dtype, F16)
        c['hi'], c['lo'] = hi.to(dev), lo.to(dev)
    if epi == 'gelu_bwd16':
        u = tails_bias(N)[None].expand(M, N) if c['family'] == 'tails' else random_plane(M, N, 3, 1.5)
        c['u'] = u.to(dtype).contiguous().to(dev)
    if epi.endswith('_ln'):
        c['stats'], c['colsum'] = ln_stats(c['A'])[0], col_sums(c['W'])
    return c


def case_to(c, device):
    def mv(v):
        if torch.is_tensor(v):
            return v.to(device)
        if isinstance(v, tuple) and len(v) == 2 and torch.is_tensor(v[0]):
            return (v[0].to(device), v[1])
        return v
    return {k: mv(v) for k, v in c.items()}


def case_segments(c):
    K = c['K']
    dq = {k: dequantize_e4m3(c[k][0], c[k][1], K) for k in ('A_lo8', 'W8', 'A8', 'W_lo8') if k in c}
    return segments(c['A'], c['W'], c.get('A_lo'), c.get('W_lo'), dq.get('A_lo8'), dq.get('W8'), dq.get('A8'), dq.get('W_lo8'))


def case_specs(c, acc_s=None):
    """-> the specs of expect() for the case (on the device its tensors live on); sets c['aux_exp'] for an e4m3 lo output so
    that the largest lo the reference allows lands below 448.  acc_s: (acc, S) when the caller has the product already."""
    segs = case_segments(c)
    acc, S = product(segs) if acc_s is None else acc_s
    specs = expect(c['epi'], c['dtype'], acc, S, k_total(segs), c['bias'], c['exact'], c.get('resid'), c.get('hi'), c.get('lo'),
                   c.get('u'), c.get('stats'), c.get('colsum'), c['lo_out'])
    if c['lo_out'] == 'e4m3':
        vmax = float(specs[0][1].abs().max())
        lo_max = 2 * U[c['dtype']] * vmax + 2.0 ** -20          # a whole 16-bit ulp of the largest value: twice what lo can be
        c['aux_exp'] = max(-60, min(60, int(math.floor(math.log2(448.0 / lo_max)))))
    return specs


def case_restate(c, korder=None):
    """The fault-free fp32 restatement of the case -> got dict."""
    return restate(c['epi'], c['dtype'], product32(case_segments(c), korder), c['bias'], c.get('resid'), c.get('hi'), c.get('lo'),
                   c.get('u'), c.get('stats'), c.get('colsum'), c['lo_out'], c['aux_exp'])


def case_buffers(c, device='cpu', row_sums=False):
    """The launch's output buffers by the conventions of the GPU tests -> dict name -> (buf, view): 'out' (holding the
    residual / the hi plane where the epilogue updates in place), 'aux' (the lo plane, the saved pre-activation, or NaN for an
    output), 'aux8' (uint8 [M + 1, 2 (N + PAD)] of 0xAA, view [M, 2 N]), 'resid' (out of place), 'row_sums' ([M + 1, N / 64, 2]
    NaN, view [M])."""
    epi, dtype, M, N = c['epi'], c['dtype'], c['M'], c['N']
    b = {}
    init = c['resid'] if epi == 'resid32' else c['hi'] if epi == 'resid_hl' else None
    b['out'] = padded(M, N, F32 if epi in OUT32 else dtype, device, init)
    if epi == 'resid32_oop':
        b['resid'] = padded(M, N, F32, device, c['resid'])
    if epi == 'resid_hl':
        b['aux'] = padded(M, N, F16, device, c['lo'])
    elif epi == 'gelu_bwd16':
        b['aux'] = padded(M, N, dtype, device, c['u'])
    elif epi == 'gelu16_save' or c['lo_out'] == '16':
        b['aux'] = padded(M, N, dtype, device)
    if c['lo_out'] == 'e4m3':
        buf = torch.full((M + 1, 2 * (N + PAD)), 0xAA, dtype=torch.uint8, device=device)
        b['aux8'] = (buf, buf[:M, :2 * N])
    if row_sums:
        buf = torch.full((M + 1, N // 64, 2), float('nan'), dtype=F32, device=device)
        b['row_sums'] = (buf, buf[:M])
    return b


def verify(c, specs, bufs, what):
    """What both the tile model's and the kernel's launch are held to: guards and padding bit for bit, inputs unchanged,
    every output within its bound (or the exact expectation itself), row_sums the sums of the hi plane that came back."""
    M, N = c['M'], c['N']
    for name, (buf, view) in bufs.items():
        if name == 'row_sums':
            assert bool(torch.isnan(buf[M:]).all()), f'{what}: row_sums guard row written'
        elif name == 'aux8':
            assert bool((buf[:M, N:] == 0xAA).all()), f'{what} aux8: bytes past column N written'
            assert bool((buf[M:] == 0xAA).all()), f'{what} aux8: guard row written'
        else:
            guards_intact(buf, M, N, f'{what} {name}')
    got = {k: v for k, (_, v) in bufs.items() if k in ('out', 'aux')}
    if 'aux8' in bufs:
        got['aux8'] = dequantize_e4m3(bufs['aux8'][1], c['aux_exp'], N)
    if c['epi'] == 'gelu_bwd16':
        assert torch.equal(_bits(got.pop('aux')), _bits(c['u'])), f'{what}: the saved pre-activation was changed'
    if 'resid' in bufs:
        assert torch.equal(bufs['resid'][1], c['resid']), f'{what}: the residual input was changed'
    check(specs, got, what, c['aux_exp'])
    if 'row_sums' in bufs:
        row_sums_check(bufs['row_sums'][1], got['out'], what)


def slice_case(c, m0, m1, N=None):
    """Rows [m0, m1) and the first N columns of a case: the inputs of every family are rules in (m, n, k), so this IS the case
    of the smaller shape at a row offset -- and the product of the large case, sliced the same way, is its product."""
    N = c['N'] if N is None else N
    s = dict(c, M=m1 - m0, N=N)
    for k in ('A', 'A_lo', 'stats'):
        if k in c:
            s[k] = c[k][m0:m1]
    for k in ('W', 'W_lo', 'bias', 'colsum'):
        if k in c:
            s[k] = c[k][:N]
    for k in ('A_lo8', 'A8'):
        if k in c:
            s[k] = (c[k][0][m0:m1], c[k][1])
    for k in ('W8', 'W_lo8'):
        if k in c:
            s[k] = (c[k][0][:N], c[k][1])
    for k in ('resid', 'hi', 'lo', 'u'):
        if k in c:
            s[k] = c[k][m0:m1, :N].contiguous()
    return s
