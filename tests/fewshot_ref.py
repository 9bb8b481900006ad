"""Float64 yardsticks, fp32 restatements, the dropout hash, directed inputs, per-element bounds and shape tables for the
few-shot training kernels of csrc/train.hip: the strided fp32 product, column sums, LayerNorm, the adapter's attention,
row normalisation, the text-identity loss head, dZ of classify, Adam.

Nothing here touches a GPU or anything compiled.  Every stage is written once, from the operation's definition, over an
arithmetic ``Arith``: F64 (torch float64 sums and products: the yardstick) or F32 (every sum and product in fp32, added in
index order: the restatement, the same bits on any machine).  tests/test_fewshot_ref_cpu.py confirms the F64 stages against
torch's own float64 modules and autograd, measures the constants below with the F32 ones, and runs every check against an
F32 model with one planted fault; tests/test_fewshot_edges_gpu.py holds the kernels to the same checks (``check_*`` take the
implementation under test as a callable).

Bounds, per element, never the largest error over the largest value:
    |got - ref| <= KERNEL_FACTOR c 2^-24 S + E
S is the magnitude that went through the accumulator (|alpha| sum |a||b| + |beta c| + |bias| for a product) or, for a
stage of several steps, the first-order propagation of one unit roundoff per step through it; c is the stage's measured
constant (F32 against F64 in units of 2^-24 S, over the stage's whole shape table, rounded up); E carries what is not
rounding of this stage: TRANS per __expf / __logf, propagated through the stage, and the propagated bound of an input
that had to be restated because the kernel overwrote it.  Rows that cancel (|ref| << S) are held to what fp32 can give."""
import functools
import math

import numpy as np
import torch

from vit_train_ref import TRANS

EPS24 = 2.0 ** -24
KERNEL_FACTOR = 4.0          # the project's figure for the matrix pipe's unknown summation order (tests/gemm_ref.py)
LN_EPS = 1e-5
F32, F64 = torch.float32, torch.float64
AGG = {'sum': 0, 'mean': 1, 'max': 2}

# ---------------------------------------------------------------------------------------------------------------
# The measured constants (tests/test_fewshot_ref_cpu.py asserts measured <= figure <= 1.5 measured; the measurements are in
# the comments).  No constant is derived from what a kernel returns.
# ---------------------------------------------------------------------------------------------------------------
C = {
    'gemm16': 4.3,       # products of K <= 16, every shape, layout and rotation of gemm_cases.  Measured: 3.62
    'gemm128': 4.6,      # K <= 128 (a cancelling row's S sits in few columns).  Measured: 3.86
    'gemm1100': 6.1,     # K <= 1100.  Measured: 5.11
    'gemm3100': 3.6,     # K <= 3100 (d qkv -> d a at d_model = 1024).  Measured: 3.03
    'colsum': 4.4,       # R <= 1040 rows.  Measured: 3.67
    'ln_fwd': 2.7,       # y, xhat and rstd of widths 8 .. 1024.  Measured: 2.29
    'ln_bwd': 0.95,      # Measured: 0.79
    'attn_fwd': 1.9,     # P and o, T = 1 .. 16, head widths 8 .. 64.  Measured: 1.59
    'attn_bwd': 1.15,    # Measured: 0.96
    'elementwise': 2.2,  # a x + b y: three roundings.  Measured: 1.83
    'head': 1.75,        # loss, aggregated logits and d text of head_cases and the saturated sample.  Measured: 1.47
    'head_dfeats': 0.5,  # d feats of the same cases, scaled by GRAD_SCALE.  Measured: 0.43
    'dz': 2.7,           # Measured: 2.27
    'adam': 1.5,         # p, m and v of adam_cases.  Measured: 1.28
    'chain1': 4.5,       # gradients end to end through 1 layer at R = 1040 (the two-trip dropout case).  Measured: 3.79
    'chain2': 11.0,      # through 2 layers.  Measured: 9.32
    'chain8': 58.0,      # through 8 layers: eight LayerNorm pairs and softmaxes amplify what reaches dy.  Measured: 48.3
}


def c_of(key):
    """'name' or ('gemm', K) -> (the constant's name, its figure)"""
    if isinstance(key, tuple):
        name = 'gemm16' if key[1] <= 16 else 'gemm128' if key[1] <= 128 else 'gemm1100' if key[1] <= 1100 else 'gemm3100'
        assert key[1] <= 3100, key
        return name, C[name]
    return key, C[key]


FLOOR = 2.0 ** -100         # fp32 underflow: below the smallest normal, 2^-126, a result is flushed or loses its bits (a softmax
#                             tail at logit_scale 100 is e^-200); nothing is held tighter than this


def bound(key, S, E=0.0):
    return KERNEL_FACTOR * c_of(key)[1] * EPS24 * S + E + FLOOR


# tests/test_fewshot_ref_cpu.py measures the constants by running the checks below on the F32 restatements with MEASURE a
# dict: every comparison of a stage whose inputs are exact records max |err| / (2^-24 S) under its constant's name, and the
# assertions are off (a wrong figure then shows as a wrong figure).
MEASURE = None


def within(got, ref, key, S, E=0.0, what='', pure=True):
    """Assert |got - ref| <= bound element by element, every element finite -> the worst error / bound."""
    got = torch.as_tensor(got)
    if not got.numel():
        return 0.0
    err = (got.double() - ref).abs()
    bd = bound(key, S, E)
    bd = bd if torch.is_tensor(bd) else torch.tensor(bd, dtype=F64)
    r = float((err / bd.clamp_min(1e-300)).max())
    if MEASURE is not None:
        if pure:
            Sx = S if torch.is_tensor(S) else torch.tensor(S, dtype=F64)
            m = float(((err - FLOOR).clamp_min(0) / (EPS24 * Sx).clamp_min(1e-300)).max())
            MEASURE[c_of(key)[0]] = max(MEASURE.get(c_of(key)[0], 0.0), m)
        return r
    assert torch.isfinite(got).all(), f'{what}: not finite'
    assert r <= 1, f'{what}: error / bound = {r:.3f}'
    return r


def f32(x):
    """A Python float as the fp32 value a `float` argument or constant of the kernels holds."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------------------------------------------
class Arith:
    """dtype float64: torch's sums and products.  float32: every product rounded, every sum added in index order."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.exact = dtype == F64

    def t(self, x):
        return (x if torch.is_tensor(x) else torch.tensor(x, dtype=F64)).to(self.dtype)

    def c(self, x):
        return torch.tensor(f32(x), dtype=self.dtype)

    def exp(self, x):
        """exp and log through float64, rounded once: correctly rounded fp32, the same bits on any machine (torch's fp32 exp is
        a vector library's, good to an ulp and different from CPU to CPU)."""
        return torch.exp(x.double()).to(self.dtype)

    def log(self, x):
        return torch.log(x.double()).to(self.dtype)

    def sqrt(self, x):
        """(torch's fp32 sqrt is not the same bits on every CPU either; the float64 root rounded once is the IEEE fp32 root)"""
        return torch.sqrt(x.double()).to(self.dtype)

    def sum(self, x, dim=-1):
        if self.exact:
            return x.sum(dim)
        x = x.movedim(dim, 0)
        acc = torch.zeros(x.shape[1:], dtype=x.dtype)
        for i in range(x.shape[0]):
            acc = acc + x[i]
        return acc

    def mm(self, a, b):
        """a [..., M, K] @ b [..., K, N]"""
        if self.exact:
            return a @ b
        acc = torch.zeros(torch.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]), dtype=F32)
        for k in range(a.shape[-1]):
            acc = acc + a[..., :, k, None] * b[..., k, None, :]
        return acc


A64, A32 = Arith(F64), Arith(F32)


# ---------------------------------------------------------------------------------------------------------------
# the dropout hash (exact): wrap-around uint64 arithmetic is the definition
# ---------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def drop_keep(seed, site, n, p, start=0):
    """-> bool [n]: element start + i of tensor `site` is kept.  float32(z >> 40) 2^-24 >= float32(p), in float32."""
    base = np.uint64((int(seed) + 0x9E3779B97F4A7C15 * (int(site) + 1)) & M64)
    with np.errstate(over='ignore'):
        i = np.arange(start, start + n, dtype=np.uint64)
        z = base + i * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def keep_scale(p):
    """1 / (1 - p) of the fp32 p the kernels are handed."""
    return 1.0 / (1.0 - f32(p))


def keep_matrix(seed, site, shape, p):
    """float64 keep-scale tensor of a dropout site (1 everywhere when p == 0)."""
    if p <= 0:
        return torch.ones(shape, dtype=F64)
    k = drop_keep(seed, site, int(np.prod(shape)), p)
    return torch.from_numpy(k.astype(np.float64) * keep_scale(p)).reshape(shape)


DROP_N = (1, 255, 256, 257, 4096 * 256 + 300)
DROP_P = (0.0, 2.0 ** -24, 0.1, 0.3, 0.5, float(np.nextafter(np.float32(1), np.float32(0))))
DROP_SITES = (0, 1, 31)
DROP_SEEDS = (0, 1, 2 ** 63 + 5, 2 ** 64 - 1)


def check_dropout(impl, what='dropout'):
    """impl(seed, site, n, p) -> uint8 / bool array [n].  Every n at one (p, site, seed) rotation, every p, site and seed
    at n = 257 and at the two-trip n."""
    cases = [(n, DROP_P[(i + 2) % 6], DROP_SITES[i % 3], DROP_SEEDS[i % 4]) for i, n in enumerate(DROP_N)]
    for n in (257, DROP_N[-1]):
        cases += [(n, p, 1, 2 ** 63 + 5) for p in DROP_P] + [(n, 0.3, s, 1) for s in DROP_SITES]
        cases += [(n, 0.5, 31, sd) for sd in DROP_SEEDS]
    for n, p, site, seed in cases:
        got = np.asarray(impl(seed, site, n, p)).astype(bool)
        want = drop_keep(seed, site, n, p)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f'{what}: n={n} p={p} site={site} seed={seed}: {bad.size} bits differ, first at {bad[0]}'
        if p == 0:
            assert got.all(), f'{what}: p = 0 dropped an element'
    return len(cases)


# ---------------------------------------------------------------------------------------------------------------
# directed inputs
# ---------------------------------------------------------------------------------------------------------------
def rotations(M):
    """The row pattern below has period 8 (ordinary, ordinary, cancelling, zero, ...): a case with fewer than four rows
    is run at the rotations that bring a cancelling and a zero row to the front (gemm_ref.rotations)."""
    return (0, 2, 3) if M < 4 else (0,)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    """float64 Gaussians on a 2^-20 grid: torch's normal sampler runs through a vector library's log / sin / cos and differs in
    the last bits from CPU to CPU; on the grid the inputs, and with them every measured constant, are the same everywhere."""
    return torch.round(torch.randn(*shape, generator=g, dtype=F64) * 2.0 ** 20) / 2.0 ** 20


KMAX, PERIOD = 3104, 131


@functools.lru_cache(maxsize=None)
def _base():
    """(a fp32 [PERIOD, KMAX], b fp32 [KMAX, PERIOD]), read-only.  Row r of a by r % 8: 0, 1, 4, 6, 7 Gaussian scaled by
    2^(r % 5 - 2) with a row mean of 0.5 ((3 r) % 5 - 2) of that scale; 2, 5 rows that CANCEL against b: a[2 j + 1] =
    -a[2 j] where b has b[2 j + 1, :] = b[2 j, :]; 3 all zero.  The last column of an odd K is zero in cancelling rows."""
    g = _gen(777)
    r = torch.arange(PERIOD)
    scale = (2.0 ** (r % 5 - 2).double())[:, None]
    a = (_randn(g, PERIOD, KMAX) + 0.5 * ((3 * r) % 5 - 2).double()[:, None]) * scale
    b = _randn(g, KMAX, PERIOD) / 4
    b[1::2] = b[0::2]
    c = torch.zeros_like(a)
    c[:, 0::2] = a[:, 0::2]
    c[:, 1::2] = -a[:, 0::2]
    a = torch.where(((r % 8 == 2) | (r % 8 == 5))[:, None], c, a)
    a = torch.where((r % 8 == 3)[:, None], torch.zeros_like(a), a)
    return a.float(), b.float()


def rows(M, K, rot=0):
    """fp32 [M, K] of the row pattern (row m is base row (m + rot) % PERIOD)."""
    a = _base()[0][(torch.arange(M) + rot) % PERIOD, :K].clone()
    if K % 2:
        cancel = ((torch.arange(M) + rot) % PERIOD % 8 == 2) | ((torch.arange(M) + rot) % PERIOD % 8 == 5)
        a[cancel, K - 1] = 0
    return a


def random_operands(M, N, K, rot=0):
    """-> A fp32 [M, K] (row pattern), B fp32 [K, N] (rows paired: the cancelling rows of A give exactly 0)."""
    return rows(M, K, rot), _base()[1][:K, torch.arange(N) % PERIOD].clone()


def exact_operands(M, N, K):
    """Small integers, |a| <= 3, |b| <= 2, K <= 1100: every partial sum in any order is exact in fp32 (S <= 6600 < 2^24)."""
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[None], torch.arange(K)
    A = ((137 * m + 29 * k[None] + (m * k[None]) % 251 + 19 * (m >> 4)) % 241) % 7 - 3
    h = (131 * n + 31 * k[:, None] + (n * k[:, None]) % 239 + 17 * (n >> 4)) % 251
    B = (1 + h % 2) * (1 - 2 * ((h // 3) % 2))
    return A.float(), B.float()


def plane(M, N, seed, scale=1.0):
    return (_randn(_gen(9000 + seed), M, N) * scale).float()


# ---------------------------------------------------------------------------------------------------------------
# stages, written once over an arithmetic
# ---------------------------------------------------------------------------------------------------------------
def gemm(ar, A, B, alpha=1.0, beta=0.0, C0=None, bias=None, relu=False):
    """alpha A B + bias + beta C0, optional ReLU.  beta == 0: C0 is not read."""
    v = ar.c(alpha) * ar.mm(A, B)
    if bias is not None:
        v = v + bias
    if beta != 0:
        v = v + ar.c(beta) * C0
    return v.clamp_min(0) if relu else v


def gemm_S(A, B, alpha=1.0, beta=0.0, C0=None, bias=None, eA=None, eB=None):
    """-> (S, E): the magnitude through the accumulator, and the propagated bound of inputs known to within eA / eB."""
    A, B = A.double().abs(), B.double().abs()
    Aw = A if eA is None else A + eA
    Bw = B if eB is None else B + eB
    core = A @ B
    wide = Aw @ Bw
    S = abs(f32(alpha)) * wide
    if bias is not None:
        S = S + bias.double().abs()
    if beta != 0:
        S = S + (f32(beta) * C0.double()).abs()
    return S, abs(f32(alpha)) * (wide - core).clamp_min(0)


def colsum(ar, X, Y=None):
    return ar.sum(X if Y is None else X * Y, 0)


def colsum_S(X, Y=None, eX=None):
    X = X.double().abs()
    Y = 1.0 if Y is None else Y.double().abs()
    return ((X if eX is None else X + eX) * Y).sum(0), (0.0 if eX is None else (eX * Y).sum(0))


def ln_fwd(ar, x, g, b):
    """-> (y, xhat, rstd): torch.nn.LayerNorm (biased variance, eps inside the root); xhat and rstd are what is saved."""
    N = x.shape[-1]
    mean = ar.sum(x) / N
    xc = x - mean[..., None]
    var = ar.sum(xc * xc) / N
    rstd = 1 / ar.sqrt(var + (ar.c(LN_EPS) if not ar.exact else LN_EPS))
    xhat = xc * rstd[..., None]
    return xhat * g + b, xhat, rstd


def ln_fwd_S(x, g, b, ex=None):
    """-> {name: (S, E)}.  One unit roundoff on every term of the mean and of the variance; an input bound ex moves the
    centred row by ex + mean(ex) and the variance by 2 mean(|xc| ex')."""
    x, g, b = x.double(), g.double(), b.double()
    _, xhat, rstd = ln_fwd(A64, x, g, b)
    mabs = x.abs().mean(-1, keepdim=True)
    r = rstd[..., None]
    xc_abs = (xhat / r).abs()
    s_xc = x.abs() + mabs                                   # roundoff magnitude of x - mean
    s_var = 2 * (xc_abs * s_xc).mean(-1, keepdim=True) + (xc_abs ** 2).mean(-1, keepdim=True)
    s_rstd = r * (1 + 0.5 * r * r * s_var)
    s_xhat = r * s_xc + xc_abs * s_rstd + xhat.abs()
    s_y = s_xhat * g.abs() + (xhat * g).abs() + b.abs()
    out = {'xhat': [s_xhat, 0.0], 'rstd': [s_rstd[..., 0], 0.0], 'y': [s_y, 0.0]}
    if ex is not None:
        e_xc = ex + ex.mean(-1, keepdim=True)
        e_var = 2 * (xc_abs * e_xc).mean(-1, keepdim=True) + (e_xc ** 2).mean(-1, keepdim=True)
        e_rstd = 0.5 * r ** 3 * e_var
        e_xhat = r * e_xc + (xc_abs + e_xc) * e_rstd
        out['xhat'][1], out['rstd'][1], out['y'][1] = e_xhat, e_rstd[..., 0], e_xhat * g.abs()
    return {k: tuple(v) for k, v in out.items()}


def ln_bwd(ar, dy, xhat, rstd, g, dx0=None):
    """dx (+ dx0 when accumulating) = rstd (gy - mean(gy) - xhat mean(gy xhat)), gy = dy g, from the SAVED xhat and rstd."""
    N = dy.shape[-1]
    gy = dy * g
    s1 = ar.sum(gy) / N
    s2 = ar.sum(gy * xhat) / N
    v = rstd[..., None] * (gy - s1[..., None] - xhat * s2[..., None])
    return v if dx0 is None else dx0 + v


def ln_bwd_S(dy, xhat, rstd, g, dx0=None, edy=None, edx0=None):
    dy, xhat, r, g = dy.double().abs(), xhat.double().abs(), rstd.double().abs()[..., None], g.double().abs()

    def mag(d):
        gy = d * g
        return r * (gy + gy.mean(-1, keepdim=True) + xhat * (gy * xhat).mean(-1, keepdim=True))
    S = 3 * mag(dy if edy is None else dy + edy)
    E = 0.0 if edy is None else mag(edy)
    if dx0 is not None:
        S = S + dx0.double().abs()
    if edx0 is not None:
        E = E + edx0
    return S, E


def _heads(x, heads):
    B, T, d = x.shape
    return x.reshape(B, T, heads, d // heads).transpose(1, 2)


def attn_fwd(ar, qkv, valid, heads, ks=None, drop_saved_p=False):
    """nn.MultiheadAttention over the T views with key_padding_mask = ~valid.  qkv [B, T, 3d], valid bool [B, T], ks
    [B, heads, T, T] keep-scale of the attention-weight dropout (None: 1) -> (P [B, heads, T, T] the softmax, undropped;
    o [B, T, d] from the dropped one)."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (_heads(qkv[..., i * d:(i + 1) * d], heads) for i in range(3))
    scale = 1 / ar.sqrt(ar.t(float(d // heads)))
    s = ar.mm(q, k.transpose(-1, -2)) * scale
    s = s.masked_fill(~valid[:, None, None, :], float('-inf'))
    e = ar.exp(s - s.max(-1, keepdim=True).values)
    P = e / ar.sum(e)[..., None]
    Pd = P if ks is None else P * ks.to(ar.dtype)
    o = ar.mm(Pd, v).transpose(1, 2).reshape(B, T, d)
    return (Pd if drop_saved_p else P), o


def attn_fwd_S(qkv, valid, heads, ks=None):
    """-> {'P': (S, E), 'o': (S, E)}.  A score is a product (unit roundoff on sum |q||k| scale) plus the rounding of the
    subtraction of the row maximum; the softmax passes a score error e on as P (2 max e); TRANS per __expf (numerator
    and the row sum: 2)."""
    qkv = qkv.double()
    B, T, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (_heads(qkv[..., i * d:(i + 1) * d], heads) for i in range(3))
    P, _ = attn_fwd(A64, qkv, valid, heads)
    scale = 1 / math.sqrt(d // heads)
    s_score = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    s_score = s_score.masked_fill(~valid[:, None, None, :], 0.0)
    smax = s_score.max(-1, keepdim=True).values
    s_p = P * (2 * smax + 4)
    e_p = P * 2 * TRANS
    kk = 1.0 if ks is None else ks.double()
    s_o = ((s_p + P) * kk) @ v.abs()
    e_o = (e_p * kk) @ v.abs()
    fold = lambda t: t.transpose(1, 2).reshape(B, T, d)     # noqa: E731
    return {'P': (s_p, e_p), 'o': (fold(s_o), fold(e_o))}


def attn_bwd(ar, qkv, P, dO, heads, ks=None):
    """dqkv [B, T, 3d] from the saved qkv and P (undropped) and d loss / d o."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (_heads(qkv[..., i * d:(i + 1) * d], heads) for i in range(3))
    do = _heads(dO, heads)
    scale = 1 / ar.sqrt(ar.t(float(d // heads)))
    kk = torch.ones((), dtype=ar.dtype) if ks is None else ks.to(ar.dtype)
    dP = ar.mm(do, v.transpose(-1, -2)) * kk
    dot = ar.sum(P * dP)[..., None]
    ds = P * (dP - dot) * scale
    dq, dk, dv = ar.mm(ds, k), ar.mm(ds.transpose(-1, -2), q), ar.mm((P * kk).transpose(-1, -2), do)
    fold = lambda t: t.transpose(1, 2).reshape(B, T, d)     # noqa: E731
    return torch.cat([fold(dq), fold(dk), fold(dv)], -1)


def attn_bwd_S(qkv, P, dO, heads, ks=None, edO=None):
    """The same map with every operand replaced by its magnitude bounds it and (it is linear in dO) what a bound on dO
    becomes."""
    qkv, P = qkv.double().abs(), P.double().abs()

    def mag(d_abs):
        B, T, d3 = qkv.shape
        d = d3 // 3
        q, k, v = (_heads(qkv[..., i * d:(i + 1) * d], heads) for i in range(3))
        do = _heads(d_abs, heads)
        kk = 1.0 if ks is None else ks.double()
        dP = (do @ v.transpose(-1, -2)) * kk
        ds = P * (dP + (P * dP).sum(-1, keepdim=True)) / math.sqrt(d // heads)
        fold = lambda t: t.transpose(1, 2).reshape(B, T, d)     # noqa: E731
        return torch.cat([fold(ds @ k), fold(ds.transpose(-1, -2) @ q), fold((P * kk).transpose(-1, -2) @ do)], -1)
    d_abs = dO.double().abs()
    return 3 * mag(d_abs if edO is None else d_abs + edO), (0.0 if edO is None else mag(edO))


def axpby(ar, a, x, b=0.0, y=None):
    v = ar.c(a) * x
    return v if y is None else v + ar.c(b) * y


def axpby_S(a, x, b=0.0, y=None):
    S = (f32(a) * x.double()).abs()
    return S if y is None else S + (f32(b) * y.double()).abs()


def normalize_fwd(ar, x, ok):
    """F.normalize of the rows, rows that are not ok zero WHATEVER they hold."""
    x = torch.where(ok[..., None], x, torch.zeros_like(x))
    n = ar.sqrt(ar.sum(x * x)).clamp_min(1e-12)
    return torch.where(ok[..., None], x / n[..., None], torch.zeros_like(x)), 1 / n


def normalize_bwd(ar, m, fn, dfn, ok, scale=1.0):
    """The VJP of normalize_fwd (times scale): (dfn - fn (fn . dfn)) scale / |m| on ok rows."""
    m = torch.where(ok[..., None], m, torch.zeros_like(m))
    inv = ar.c(scale) / ar.sqrt(ar.sum(m * m)).clamp_min(1e-12)
    dot = ar.sum(fn * dfn)
    return torch.where(ok[..., None], (dfn - fn * dot[..., None]) * inv[..., None], torch.zeros_like(m))


def normalize_bwd_S(m, fn, dfn, ok, scale=1.0, edfn=None):
    m, fn, d = m.double(), fn.double().abs(), dfn.double().abs()
    inv = (abs(f32(scale)) / torch.sqrt((m * m).sum(-1)).clamp_min(1e-12))[..., None] * ok[..., None]

    def mag(d):
        return (d + fn * (fn * d).sum(-1, keepdim=True)) * inv
    return 3 * mag(d if edfn is None else d + edfn), (0.0 if edfn is None else mag(edfn))


# ---------------------------------------------------------------------------------------------------------------
# the text-identity head: normalise, logits, loss, dL, d text (clip_cls.py forward, calc_train_loss, autograd)
# ---------------------------------------------------------------------------------------------------------------
def text_head(ar, feats, valid, labels, text, scale, agg, probs, mean_over_T=False, with_S=False, grad_scale=1.0):
    """feats [B, T, D], valid bool [B, T], labels int64 [B], text [K, D] -> dict(loss, agg_logits [B, K], grad_text [K, D],
    d_feats [B, T, D] = grad_scale d loss / d feats: the fine-tuning head's feature gradient).
    with_S (float64 only): also the first-order propagation of one unit roundoff per step ('S_*') and of TRANS per
    __expf / __logf ('E_*') through the chain."""
    B, T, D = feats.shape
    K = text.shape[0]
    sc = ar.c(scale)
    tn = ar.sqrt(ar.sum(text * text)).clamp_min(1e-12)
    u, inv = text / tn[:, None], 1 / tn
    Fn, _ = normalize_fwd(ar, feats, valid)
    L = sc * ar.mm(Fn.reshape(B * T, D), u.T).reshape(B, T, K)
    nv = ar.t(valid.sum(1).double()) if not mean_over_T else ar.t(torch.full((B,), float(T)))
    onehot = torch.nn.functional.one_hot(labels, K).to(ar.dtype)
    wv = (1 / nv if agg == 'mean' else torch.ones_like(nv))[:, None]
    out = {}
    if with_S:
        fa, ua = Fn.abs().reshape(B * T, D), u.abs()
        S_L = (float(sc) * (fa @ ua.T) * 3).reshape(B, T, K)         # 3: the operands' own normalisation, the product
        E_L = torch.zeros_like(S_L)
    if not probs:
        a = ar.sum(L, 1) * wv
        mx = a.max(-1, keepdim=True).values
        se = ar.sum(ar.exp(a - mx))
        lse = mx[:, 0] + ar.log(se)
        loss_b = lse - a[torch.arange(B), labels]
        p = ar.exp(a - lse[:, None])
        g = (p - onehot) / B
        dL = (g * wv)[:, None, :].expand(B, T, K)
        agg_logits = a
        if with_S:
            S_a = S_L.sum(1) * wv + a.abs()
            S_am = S_a.max(-1, keepdim=True).values
            S_lb = 2 * S_am[:, 0] + lse.abs() + loss_b.abs() + 2
            E_lb = TRANS * (2 + torch.log(se).abs())
            S_p = p * (2 * S_am + lse.abs()[:, None] + 2)
            E_p = p * (2 * TRANS + E_lb[:, None])
            S_dL = (((S_p + g.abs() * B) / B) * wv)[:, None, :].expand(B, T, K)
            E_dL = ((E_p / B) * wv)[:, None, :].expand(B, T, K)
            out['S_agg'], out['E_agg'] = S_a, torch.zeros_like(S_a)
    else:
        mx = L.max(-1, keepdim=True).values
        e = ar.exp(L - mx)
        se = ar.sum(e)
        p = e / se[..., None]
        vm = valid.to(ar.dtype)
        pvy = p[torch.arange(B), :, labels]
        Py = ar.sum(pvy * vm) / nv
        loss_b = -ar.log(Py + ar.c(1e-6))
        dPy = -1 / (B * (Py + ar.c(1e-6)))
        cf = (dPy[:, None] * pvy / nv[:, None]) * vm
        dL = cf[..., None] * (onehot[:, None, :] - p)
        a = ar.sum(L, 1)
        agg_logits = a / nv[:, None] if agg == 'mean' else a
        if with_S:
            S_lm = S_L.max(-1, keepdim=True).values
            S_p = p * (2 * S_lm + 4)
            E_p = p * 2 * TRANS
            S_pvy, E_pvy = S_p[torch.arange(B), :, labels], E_p[torch.arange(B), :, labels]
            S_Py = ((S_pvy + pvy) * vm).sum(1) / nv + Py
            E_Py = (E_pvy * vm).sum(1) / nv
            den = Py + 1e-6
            S_lb = S_Py / den + loss_b.abs() + 1
            E_lb = E_Py / den + TRANS * (1 + loss_b.abs())
            S_dPy, E_dPy = dPy.abs() * (S_Py / den + 2), dPy.abs() * E_Py / den
            S_cf = ((S_dPy[:, None] * pvy + dPy.abs()[:, None] * S_pvy) / nv[:, None] + 2 * cf.abs()) * vm
            E_cf = ((E_dPy[:, None] * pvy + dPy.abs()[:, None] * E_pvy) / nv[:, None]) * vm
            om = (onehot[:, None, :] - p).abs()
            S_dL = S_cf[..., None] * om + cf.abs()[..., None] * (S_p + om)
            E_dL = E_cf[..., None] * om + cf.abs()[..., None] * E_p
            S_agg = S_L.sum(1) + a.abs()
            out['S_agg'], out['E_agg'] = (S_agg / nv[:, None] if agg == 'mean' else S_agg), torch.zeros_like(S_agg)
    dU = sc * ar.mm(dL.reshape(B * T, K).T, Fn.reshape(B * T, D))
    dot = ar.sum(u * dU)
    grad = (dU - u * dot[:, None]) * inv[:, None]
    dfn = (sc * ar.mm(dL.reshape(B * T, K), u)).reshape(B, T, D)
    out.update(loss=ar.sum(loss_b, 0) / B, agg_logits=agg_logits, grad_text=grad,
               d_feats=normalize_bwd(ar, feats, Fn, dfn, valid, grad_scale))
    if with_S:
        # d Fn = scale dL u carries S_dL and E_dL through |u| as d U does through |Fn|; the row normalisation's backward
        # propagates both as input errors (its edfn) on top of its own roundoff
        S_dfn = (float(sc) * ((S_dL + 2 * dL.abs()).reshape(B * T, K) @ u.abs())).reshape(B, T, D)
        E_dfn = (float(sc) * (E_dL.reshape(B * T, K) @ u.abs())).reshape(B, T, D)
        out['S_d_feats'] = normalize_bwd_S(feats, Fn, dfn, valid, grad_scale)[0] + \
            normalize_bwd_S(feats, Fn, dfn, valid, grad_scale, S_dfn)[1]
        out['E_d_feats'] = normalize_bwd_S(feats, Fn, dfn, valid, grad_scale, E_dfn)[1]
        fa = Fn.abs().reshape(B * T, D)
        S_dU = float(sc) * ((S_dL + 2 * dL.abs()).reshape(B * T, K).T @ fa)
        E_dU = float(sc) * (E_dL.reshape(B * T, K).T @ fa)
        proj = lambda t: (t + u.abs() * (u.abs() * t).sum(-1, keepdim=True)) * inv[:, None]     # noqa: E731
        out['S_grad_text'], out['E_grad_text'] = proj(S_dU) + 3 * proj(dU.abs()), proj(E_dU)
        out['S_loss'], out['E_loss'] = S_lb.sum() / B + loss_b.abs().sum() / B, E_lb.sum() / B
    return out


HEAD_K = (1, 2, 63, 64, 65, 255, 256, 257)
HEAD_T = (1, 2, 16)
HEAD_B = (1, 63, 64, 65)
HEAD_D = (1, 4, 63, 64, 65)


def head_cases():
    """(B, T, D, K, agg, probs, label rule): every value of each axis against a small and a large value of the others,
    both losses and both aggregations rotating, labels 0 and K - 1."""
    cs = []
    for i, K in enumerate(HEAD_K):
        cs += [(2, 2, 4, K), (65, 16 if K < 200 else 2, 65, K)]
    for T in HEAD_T:
        cs += [(3, T, 5, 3), (64, T, 64, 65)]
    for B in HEAD_B:
        cs += [(B, 1, 4, 2), (B, 3, 63, 64)]
    for D in HEAD_D:
        cs += [(2, 2, D, 3), (33, 3, D, 65)]
    modes = [('sum', False), ('mean', False), ('sum', True), ('mean', True)]
    return [c + modes[i % 4] + (i // 4 % 2,) for i, c in enumerate(dict.fromkeys(cs))] + \
        [(2, 2, 4, 5) + m + (l,) for m in modes for l in (0, 1)]


def head_inputs(B, T, D, K, last_label, seed=0, saturated=False):
    """feats fp32 [B, T, D] (row pattern; views correlate with their class row), valid (view 0 always; sample 1 only view
    0), labels (0 / K - 1 alternating from last_label), text fp32 [K, D]."""
    g = _gen(100 + seed + 7 * B + 3 * K)
    text = (_randn(g, K, D) * 0.5).float()
    labels = torch.where((torch.arange(B) + last_label) % 2 == 1, K - 1, 0).long()
    feats = rows(B * T, D, rot=seed).reshape(B, T, D) * 0.25 + 0.5 * text[labels][:, None]
    valid = torch.rand(B, T, generator=g) < 0.7
    valid[:, 0] = True
    if B > 1:
        valid[1, 1:] = False
    if saturated:
        feats[0] = text[labels[0]] * 3.0
        valid[0] = True
    return feats.float().contiguous(), valid, labels, text


GRAD_SCALE = 1536.0          # a gradient scaler's value that is no power of two: the product with it rounds


def check_head(impl, case, what, poison=None, scale=100.0, saturated=False, grad_scale=None):
    """impl(feats, valid, labels, text, scale, agg, probs) -> (loss [1], grad_text, agg_logits) as CPU tensors.  -> the worst
    error / bound.  poison: invalid views are filled with it first (any value there must change nothing).  grad_scale:
    impl takes it as one more argument and returns d_feats [B, T, D] as a fourth tensor."""
    B, T, D, K, agg, probs, last = case
    feats, valid, labels, text = head_inputs(B, T, D, K, last, saturated=saturated)
    if poison is not None:
        feats = torch.where(valid[..., None], feats, torch.full_like(feats, poison))
    r = text_head(A64, feats.double(), valid, labels, text.double(), scale, agg, probs, with_S=True,
                  grad_scale=grad_scale or 1.0)
    loss, grad, logits, *d_feats = impl(feats, valid, labels, text, scale, agg, probs, *([grad_scale] if grad_scale else []))
    assert len(d_feats) == (1 if grad_scale else 0)
    worst = 0.0
    for name, got in (('loss', loss.reshape(())), ('agg_logits', logits), ('grad_text', grad)):
        key = 'agg' if name == 'agg_logits' else name
        worst = max(worst, within(got, r[name], 'head', r['S_' + key], r['E_' + key], f'{what} {case}: {name}'))
    for got in d_feats:
        worst = max(worst, within(got, r['d_feats'], 'head_dfeats', r['S_d_feats'], r['E_d_feats'], f'{what} {case}: d_feats'))
    return worst


# ---------------------------------------------------------------------------------------------------------------
# dZ of classify
# ---------------------------------------------------------------------------------------------------------------
def classify_dz(ar, full, ok, agg, d_full=None, d_logits=None, d_probs=None, tie_high=False, no_offset=False):
    """full [B, T, K] (invalid views hold the constant 0), ok bool [B, T] -> dZ [B, T, K].  max: d_logits goes to the
    maximal view over l - 1e6 [invalid], the lowest index on a tie."""
    B, T, K = full.shape
    z = torch.zeros_like(full)
    okf = ok.to(ar.dtype)[..., None]
    nv = ar.t(ok.sum(1).double())[:, None, None]
    if d_full is not None:
        z = z + d_full
    if d_logits is not None:
        gl = d_logits[:, None, :]
        if agg == 'sum':
            z = z + gl
        elif agg == 'mean':
            z = z + gl / nv
        else:
            l = full - (0.0 if no_offset else 1e6) * (1 - okf)
            if tie_high:
                am = T - 1 - l.flip(1).argmax(1)
            else:
                am = (l == l.max(1, keepdim=True).values).to(torch.uint8).argmax(1)
            z = z + gl * torch.nn.functional.one_hot(am, T).transpose(1, 2).to(ar.dtype)
    if d_probs is not None:
        e = ar.exp(full - full.max(-1, keepdim=True).values)
        se = ar.sum(e)[..., None]
        dot = ar.sum(d_probs[:, None, :] * e)[..., None] / se
        z = z + e / se * (d_probs[:, None, :] - dot) / nv
    return z * okf


def classify_dz_S(full, ok, agg, d_full=None, d_logits=None, d_probs=None):
    full = full.double()
    S = torch.zeros_like(full)
    nv = ok.sum(1).double()[:, None, None]
    if d_full is not None:
        S = S + d_full.double().abs()
    if d_logits is not None:
        S = S + d_logits.double().abs()[:, None, :] / (nv if agg == 'mean' else 1.0)
    if d_probs is not None:
        p = torch.softmax(full, -1)
        gp = d_probs.double().abs()[:, None, :]
        spread = (full - full.max(-1, keepdim=True).values).abs() + full.abs()
        S = S + p * (gp + (gp * p).sum(-1, keepdim=True)) / nv * (4 + spread + (p * spread).sum(-1, keepdim=True))
    return S * ok[..., None]


DZ_K = (2, 255, 256, 257)
DZ_T = (1, 16)


def dz_directed(K, T):
    """Three samples of small-integer logits (exact in any arithmetic), max aggregation, integer d_logits:
    0  an exact tie of the maximum between two views (1 and 3 of 16; at T = 1 the single view), every other view lower;
    1  view 0 INVALID (its logit row is the constant 0 of the scatter) and every valid logit negative;
    2  a single valid view, the last.
    -> (full fp32 [3, T, K], ok bool [3, T], d_logits fp32 [3, K])"""
    k = torch.arange(K)
    full = torch.zeros(3, T, K)
    ok = torch.ones(3, T, dtype=torch.bool)
    for v in range(T):
        full[0, v] = ((k * 7 + v * 3) % 11).float() - 8          # <= 2
        full[1, v] = -1.0 - ((k * 5 + v) % 9).float()            # all negative
        full[2, v] = ((k + v) % 5).float() - 2
    if T > 1:
        full[0, 1] = ((k * 3) % 4).float() + 3                   # the maximum of every class, twice
        full[0, 3] = full[0, 1]
        ok[1, 0] = False
        ok[2, :T - 1] = False
    full = full * ok[..., None]
    d_logits = (((torch.arange(3)[:, None] * 5 + k[None] * 3) % 13) - 6).float()
    d_logits[d_logits == 0] = 7.0
    return full, ok, d_logits


def check_dz_directed(impl, K, T, what):
    """impl(full, ok, agg, d_full, d_logits, d_probs) -> dZ fp32 [B, T, K] (zero rows where it cannot see an invalid view)."""
    full, ok, gl = dz_directed(K, T)
    got = impl(full, ok, 'max', None, gl, None)
    want = classify_dz(A64, full.double(), ok, 'max', d_logits=gl.double())
    assert torch.equal(got.double().sum(1), gl.double()), f"{what}: the views' dZ do not sum to d_logits per class"
    if T > 1:
        assert torch.equal(got[0, 1], gl[0]), f'{what}: a tie did not go to the lowest index'
        assert not bool(got[0, 3].any()), f'{what}: the tied view of the higher index got a gradient'
        assert not bool(got[1, 0].any()), f'{what}: an invalid view won over all-negative valid logits'
        assert torch.equal(got[2, T - 1], gl[2]), f'{what}: the single valid view did not get d_logits'
    assert torch.equal(got.double(), want), f'{what}: dZ differs from the yardstick'


def check_dz_random(impl, K, T, agg, what):
    """All three upstream gradients at once on Gaussian logits (scale 6: sharp and flat softmaxes) under the bound."""
    g = _gen(K * 31 + T)
    B = 4
    ok = torch.rand(B, T, generator=g) < 0.7
    ok[:, 0] = True
    full = (_randn(g, B, T, K) * 6).float() * ok[..., None]
    d_full, gl, gp = (_randn(g, *sh).float() for sh in ((B, T, K), (B, K), (B, K)))
    got = impl(full, ok, agg, d_full, gl, gp)
    want = classify_dz(A64, full.double(), ok, agg, d_full.double(), gl.double(), gp.double())
    return within(got, want, 'dz', classify_dz_S(full, ok, agg, d_full, gl, gp), 0.0, what)


# ---------------------------------------------------------------------------------------------------------------
# Adam, as torch.optim.Adam states it (no amsgrad); the hyper-parameters are the fp32 values the ABI is handed
# ---------------------------------------------------------------------------------------------------------------
def adam(ar, p, g, m, v, step, lr, b1, b2, eps, wd, cap=None):
    """-> (p, m, v) after the step.  cap: only the first cap elements move (the planted grid fault)."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    t = ar.t
    gi = g + t(wd) * p if wd != 0 else g
    mn = m * t(b1) + t(1 - b1) * gi
    vn = v * t(b2) + t(1 - b2) * gi * gi
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    pn = p - t(lr) / t(bc1) * mn / (ar.sqrt(vn) / t(math.sqrt(bc2)) + t(eps))
    if cap is not None and p.numel() > cap:
        pn, mn, vn = (torch.cat([a[:cap], b[cap:]]) for a, b in ((pn, p), (mn, m), (vn, v)))
    return pn, mn, vn


def adam_S(p, g, m, v, step, lr, b1, b2, eps, wd):
    p, g, m, v = (x.double() for x in (p, g, m, v))
    pn, mn, vn = adam(A64, p, g, m, v, step, lr, b1, b2, eps, wd)
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    gi = g.abs() + abs(wd) * p.abs()
    S_m = b1 * m.abs() + (1 - b1) * gi + mn.abs()
    S_v = b2 * v.abs() + 2 * (1 - b2) * gi * gi + vn
    upd = (p - pn).abs()
    rel_m = S_m / mn.abs().clamp_min(1e-300)
    rel_v = S_v / vn.clamp_min(1e-300)
    S_p = p.abs() + pn.abs() + upd * (5 + torch.where(mn == 0, torch.zeros_like(rel_m), rel_m + 0.5 * rel_v))
    return (pn, mn, vn), (S_p, S_m, S_v)


ADAM_N = (1, 255, 257, 2048 * 256 + 77)
ADAM_STEPS = (1, 2, 1000)


def adam_inputs(n, directed):
    g_ = _gen(31 + n)
    p = _randn(g_, n)
    if directed:
        # g spanning 1e-12 .. 1e6 by decades with both signs; every 5th element (0, 5, ...) has g = m = v = 0 and must not move
        dec = 10.0 ** ((torch.arange(n) % 19) - 12).double()
        g = (dec * (1 + torch.rand(n, generator=g_, dtype=F64)) * (1 - 2 * (torch.arange(n) % 2))).float()
        m = (g.double() * 0.5 * _randn(g_, n)).float()
        v = (g.double() ** 2 * torch.rand(n, generator=g_, dtype=F64)).float()
        still = torch.arange(n) % 5 == 0
        g[still], m[still], v[still] = 0, 0, 0
    else:
        g = _randn(g_, n) * 0.3
        m = _randn(g_, n) * 0.1
        v = torch.rand(n, generator=g_) * 0.05
    return p.float(), g.float(), m.float(), v.float()


def adam_cases():
    cs = []
    for i, n in enumerate(ADAM_N):
        cs.append((n, ADAM_STEPS[i % 3], (0.0, 0.02)[i % 2], 1e-8, False))
        cs.append((n, ADAM_STEPS[(i + 1) % 3], 0.0, (1e-8, 1e-3)[i % 2], True))
    cs += [(257, s, wd, 1e-8, False) for s in ADAM_STEPS for wd in (0.0, 0.02)]
    cs += [(257, 2, 0.0, 1e-3, True), (257, 1000, 0.0, 1e-8, True)]
    return cs


def check_adam(impl, case, what):
    """impl(p, g, m, v, step, lr, b1, b2, eps, wd) -> (p, m, v) CPU fp32.  -> worst error / bound."""
    n, step, wd, eps, directed = case
    p, g, m, v = adam_inputs(n, directed)
    hp = (step, 2e-3, 0.9, 0.98, eps, wd)
    want, S = adam_S(p, g, m, v, *hp)
    got = impl(p.clone(), g.clone(), m.clone(), v.clone(), *hp)
    worst = 0.0
    for name, gt, w, s in zip('pmv', got, want, S):
        worst = max(worst, within(gt, w, 'adam', s, 0.0, f'{what} {case}: {name}'))
    if directed:
        still = (g == 0) & (m == 0) & (v == 0)
        assert still.any() and torch.equal(got[0][still], p[still]), f'{what}: an element with g = m = v = 0 moved'
        assert not bool(got[1][still].any()) and not bool(got[2][still].any())
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the strided product: shapes, layouts, checks
# ---------------------------------------------------------------------------------------------------------------
GEMM_MN = (1, 31, 32, 33, 63, 64, 65, 129)
GEMM_K = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 100)
LAYOUTS = ('kk', 'kr', 'rk', 'rr')       # a_kfast x b_kfast: 'k' = the k index is the fast one in memory, 'r' = the row index
PAD = 8


def gemm_shapes():
    """Every value of each axis against a small and a large value of the others."""
    s = []
    for m in GEMM_MN:
        s += [(m, 3, 5), (m, 65, 33)]
    for n in GEMM_MN:
        s += [(3, n, 5), (65, n, 33)]
    for k in GEMM_K:
        s += [(3, 2, k), (65, 129, k)]
    return list(dict.fromkeys(s))


def gemm_cases():
    """(M, N, K, layout, family, rot, window, alpha, beta, ldc_pad, equal): every shape of gemm_shapes in both families with
    the layout, alpha / beta and ldc rotating; the four layouts plain and as windows at three shapes; equal strides at M = 1,
    N = 1 and K = 1; three deeper K for the constants of the adapter's products."""
    cs = []
    for i, (M, N, K) in enumerate(gemm_shapes()):
        lay, pad = LAYOUTS[i % 4], (0, 5)[i % 2]
        cs.append((M, N, K, lay, 'exact', 0, i % 3 == 2, (1.0, 2.0, -3.0)[i % 3], (0.0, 1.0, -2.0)[(i + 1) % 3], pad, False))
        for rot in rotations(M):
            cs.append((M, N, K, lay, 'random', rot, i % 3 == 1, (1.0, -0.75, 2.5)[i % 3], (0.0, 0.5, -1.25)[(i + 1) % 3], pad, False))
    for M, N, K in ((65, 33, 17), (3, 129, 100), (33, 65, 48)):
        for lay in LAYOUTS:
            for window in (False, True):
                cs.append((M, N, K, lay, 'exact', 0, window, 2.0, 0.0, 3, False))
                cs.append((M, N, K, lay, 'random', 0, window, -0.75, 0.5, 3, False))
    for M, N, K in ((1, 33, 17), (33, 1, 17), (5, 7, 1), (1, 1, 1)):
        for lay in LAYOUTS:
            cs.append((M, N, K, lay, 'random', 2, False, 1.0, 0.0, 0, True))
    for M, N, K in ((65, 33, 256), (16, 40, 1024), (33, 65, 3072)):
        cs.append((M, N, K, 'kr', 'random', 0, False, 1.0, 0.0, 0, False))
        cs.append((M, N, K, 'rk', 'exact', 0, False, 1.0, 0.0, 0, False))
    return cs


def place(x, fast_last, window, fill=float('nan')):
    """The logical matrix x [R, C] laid out in a fresh buffer -> (buffer, element offset, stride of axis 0, stride of
    axis 1).  fast_last: axis 1 is the fast one.  window: x is a window of a wider buffer with BOTH strides non-unit (the
    fast axis takes every second element, the slow one a padded pitch), the rest NaN."""
    xs = x if fast_last else x.T
    r, c = xs.shape
    if window:
        buf = torch.full((r + 2, 2 * c + PAD), fill, dtype=F32)
        buf[1:r + 1, 3:3 + 2 * c:2] = xs
        off, s_slow, s_fast = buf.shape[1] + 3, buf.shape[1], 2
    else:
        buf = xs.contiguous().clone()
        off, s_slow, s_fast = 0, max(c, 1), 1
    return (buf, off, s_slow, s_fast) if fast_last else (buf, off, s_fast, s_slow)


def gemm_case(M, N, K, layout, family, rot=0, window=False, alpha=1.0, beta=0.0, ldc_pad=0, equal=False):
    """-> dict: the operands (logical and placed), C0, the float64 reference and S.  equal: an axis of size 1 is given the
    other axis' stride (the equal-stride views of M = 1, N = 1 or K = 1)."""
    A, B = exact_operands(M, N, K) if family == 'exact' else random_operands(M, N, K, rot)
    if family == 'exact':
        C0 = ((torch.arange(M)[:, None] * 3 + torch.arange(N)[None] * 5) % 9 - 4).float()
    else:
        C0 = plane(M, N, 1, 2.0)
    ab, ao, sam, sak = place(A, layout[0] == 'k', window)
    bb, bo, sbn, sbk = place(B.T.contiguous(), layout[1] == 'k', window)        # B as [N, K]: axis 1 is k
    if equal:
        sam, sak = (sak, sak) if M == 1 else (sam, sam) if K == 1 else (sam, sak)
        sbn, sbk = (sbk, sbk) if N == 1 else (sbn, sbn) if K == 1 else (sbn, sbk)
    ref = gemm(A64, A.double(), B.double(), alpha, beta, C0.double())
    S, _ = gemm_S(A, B, alpha, beta, C0)
    return dict(M=M, N=N, K=K, A=A, B=B, C0=C0, pa=(ab, ao, sam, sak), pb=(bb, bo, sbn, sbk), alpha=alpha, beta=beta, ref=ref,
                S=S, family=family, ldc_pad=ldc_pad)


def strides_layout(case):
    """The a_kfast x b_kfast combination the strides of a case select (sak <= sam, sbk < sbn): the named layout, except where
    an axis of size 1 or an equal-stride view decides otherwise."""
    (_, _, sam, sak), (_, _, sbn, sbk) = case['pa'], case['pb']
    return ('k' if sak <= sam else 'r') + ('k' if sbk < sbn else 'r')


def check_gemm(impl, case, what):
    """impl(Abuf, a_off, sam, sak, Bbuf, b_off, sbk, sbn, M, N, K, alpha, beta, Cbuf [M + 1, ldc]) fills Cbuf in place (CPU
    tensors in, CPU tensor out).  C starts NaN-filled when beta == 0; the padding columns and the guard row hold a bit
    pattern that must come back.  -> error / bound (0 for the exact family: bit for bit)."""
    M, N, K = case['M'], case['N'], case['K']
    ldc = N + case['ldc_pad']
    guard = torch.tensor(-0x12345679, dtype=torch.int32).view(F32)       # a NaN with a payload
    Cb = torch.full((M + 1, ldc), float(guard)).view(torch.int32)
    Cb[:] = -0x12345679
    Cb = Cb.view(F32)
    if case['beta'] != 0:
        Cb[:M, :N] = case['C0']
    else:
        Cb[:M, :N] = float('nan')
    (ab, ao, sam, sak), (bb, bo, sbn, sbk) = case['pa'], case['pb']
    out = impl(ab, ao, sam, sak, bb, bo, sbk, sbn, M, N, K, case['alpha'], case['beta'], Cb.clone())
    got = out[:M, :N]
    oi = out.view(torch.int32)
    assert bool((oi[M] == -0x12345679).all()) and bool((oi[:M, N:] == -0x12345679).all()), f'{what}: guard overwritten'
    assert MEASURE is not None or not torch.isnan(got).any(), f'{what}: NaN in the output'
    if case['family'] == 'exact':
        assert torch.equal(got.double(), case['ref']), \
            f'{what}: exact family differs, max |err| {float((got.double() - case["ref"]).abs().max())}'
        return 0.0
    return within(got, case['ref'], ('gemm', K), case['S'], 0.0, what)


def gemm_model(fault=None):
    """The F32 restatement behind check_gemm's interface, with one planted fault:
    'ktail' the last k of a K that is no multiple of 16 dropped; 'beta0' beta C read when beta == 0; ('slab', layout) the
    16 x 16 blocks of A's slabs read transposed in that layout combination."""
    def impl(ab, ao, sam, sak, bb, bo, sbk, sbn, M, N, K, alpha, beta, Cb):
        A = torch.as_strided(ab.reshape(-1), (M, K), (sam, sak), ao) if K else torch.zeros(M, 0)
        B = torch.as_strided(bb.reshape(-1), (K, N), (sbk, sbn), bo) if K else torch.zeros(0, N)
        a_kfast, b_kfast = sak <= sam, sbk < sbn
        if fault == 'ktail' and K % 16:
            A, B = A[:, :K - 1], B[:K - 1]
        if isinstance(fault, tuple) and fault[1] == ('k' if a_kfast else 'r') + ('k' if b_kfast else 'r') and M > 1 and K > 1:
            Ap = torch.zeros((M + 15) // 16 * 16, (K + 15) // 16 * 16)
            Ap[:M, :K] = A
            Ap = Ap.reshape(Ap.shape[0] // 16, 16, Ap.shape[1] // 16, 16).transpose(1, 3).reshape(Ap.shape)
            A = Ap[:M, :K]
        C0 = Cb[:M, :N].clone()
        v = gemm(A32, A, B, alpha, beta, C0)
        if fault == 'beta0' and beta == 0:
            v = v + 0.0 * C0
        Cb[:M, :N] = v
        return Cb
    return impl


# ---------------------------------------------------------------------------------------------------------------
# the adapter (models/adapter.py TransformerAdapter: in_proj -> norm_first encoder layers -> out_proj -> residual mix)
# ---------------------------------------------------------------------------------------------------------------
LAYER_FIELDS = ('ln1_g', 'ln1_b', 'qkv_w', 'qkv_b', 'o_w', 'o_b', 'ln2_g', 'ln2_b', 'w1', 'b1', 'w2', 'b2')
PROJ_FIELDS = ('in_w', 'in_b', 'out_w', 'out_b')
GEOMETRIES = ((50, 40, 5, 72), (1, 8, 1, 1), (100, 72, 2, 24), (64, 1024, 16, 8))      # (D, d_model, heads, ffn)
ROW_COUNTS = ((1, 1), (3, 1), (2, 2), (5, 1), (14, 2), (29, 1), (2, 16), (33, 1), (12, 3), (61, 1), (4, 16), (5, 13))
# layers, (B, T, geometry), dropout_p, residual: the deep chains checked end to end
E2E_CASES = ((2, (3, 5, GEOMETRIES[0]), 0.3, 0.8), (8, (2, 16, GEOMETRIES[2]), 0.0, 0.8), (8, (3, 4, GEOMETRIES[0]), 0.3, 0.0))
BIG_DROPOUT = dict(B=65, T=16, geom=(8, 8, 1, 1024), layers=1, p=0.3, residual=0.8)


def adapter_cases():
    """(B, T, geometry, layers, dropout_p, residual): every geometry at two row counts, every row count at geometry 0, T = 15
    and 16, residual and dropout rotating."""
    cs = []
    for i, (B, T) in enumerate(ROW_COUNTS):
        cs.append((B, T, GEOMETRIES[0], 1, (0.0, 0.3)[i % 2], (0.0, 0.8)[i // 2 % 2]))
    cs.append((3, 15, GEOMETRIES[0], 1, 0.3, 0.8))
    for i, g in enumerate(GEOMETRIES[1:]):
        cs += [(3, 1, g, 1, 0.0, 0.8), (2, 16, g, 1, 0.3, 0.0)] if g[1] < 1024 else [(3, 1, g, 1, 0.3, 0.8), (1, 16, g, 1, 0.0, 0.0)]
    return cs


def adapter_params(D, d, heads, ffn, layers, seed=0):
    """{field: fp32} and [{field: fp32}] per layer, torch layouts ([out, in] weights); LayerNorm gains around 1."""
    g = _gen(500 + seed)

    def w(o, i):
        return (_randn(g, o, i) / math.sqrt(i)).float()

    def b(n, base=0.0):
        return (base + 0.2 * _randn(g, n)).float()
    top = dict(in_w=w(d, D), in_b=b(d), out_w=w(D, d), out_b=b(D))
    blocks = [dict(ln1_g=b(d, 1.0), ln1_b=b(d), qkv_w=w(3 * d, d), qkv_b=b(3 * d), o_w=w(d, d), o_b=b(d),
                   ln2_g=b(d, 1.0), ln2_b=b(d), w1=w(ffn, d), b1=b(ffn), w2=w(d, ffn), b2=b(d)) for _ in range(layers)]
    return top, blocks


def adapter_inputs(B, T, D, seed=0):
    """img fp32 [B, T, D] of the row pattern with ZERO rows on invalid views; valid: view 0 always, the last sample only
    view 0; d_out fp32 [B, T, D]."""
    g = _gen(900 + seed + B * 17 + T)
    valid = torch.rand(B, T, generator=g) < 0.7
    valid[:, 0] = True
    valid[B - 1, 1:] = False
    img = rows(B * T, D, rot=seed).reshape(B, T, D) * valid[..., None]
    d_out = rows(B * T, D, rot=seed + 5).reshape(B, T, D).flip(-1) * 0.5
    return img.float().contiguous(), valid, d_out.float().contiguous()


def _keeps(seed, p, l, B, T, d, heads, ffn, site_shift=0):
    R = B * T
    shapes = ((B, heads, T, T), (R, d), (R, ffn), (R, d))
    return [keep_matrix(seed, 4 * l + s + site_shift, sh, p) for s, sh in enumerate(shapes)]


def adapter_forward(ar, img, valid, top, blocks, heads, residual, p=0.0, seed=0, fault=None):
    """The whole forward over an arithmetic -> (out [B, T, D], tape dict: h0, hfin, y and per layer the LayerBufs slots).
    fault: 'rstd_eps' rstd saved without eps; 'p_dropped' the dropped P saved; 'site' the masks of the next site."""
    B, T, D = img.shape
    R = B * T
    d, ffn = top['in_w'].shape[0], blocks[0]['w1'].shape[0]
    cv = lambda t: t.to(ar.dtype)     # noqa: E731
    x = cv(img).reshape(R, D)
    h = gemm(ar, x, cv(top['in_w']).T, bias=cv(top['in_b']))
    tape = {'h0': h, 'L': []}
    for l, bp in enumerate(blocks):
        w = {k: cv(v) for k, v in bp.items()}
        ks = [cv(k) for k in _keeps(seed, p, l, B, T, d, heads, ffn, 1 if fault == 'site' else 0)]
        a, xhat1, rstd1 = ln_fwd(ar, h, w['ln1_g'], w['ln1_b'])
        if fault == 'rstd_eps':
            rstd1 = 1 / ar.sqrt(((h - h.mean(-1, keepdim=True)) ** 2).mean(-1))
        qkv = gemm(ar, a, w['qkv_w'].T, bias=w['qkv_b'])
        P, o = attn_fwd(ar, qkv.reshape(B, T, 3 * d), valid, heads, ks[0] if p > 0 else None, drop_saved_p=fault == 'p_dropped')
        o = o.reshape(R, d)
        h1 = h + ks[1] * gemm(ar, o, w['o_w'].T, bias=w['o_b'])
        bn, xhat2, rstd2 = ln_fwd(ar, h1, w['ln2_g'], w['ln2_b'])
        f = ks[2] * gemm(ar, bn, w['w1'].T, bias=w['b1'], relu=True)
        h = h1 + ks[3] * gemm(ar, f, w['w2'].T, bias=w['b2'])
        tape['L'].append(dict(xhat1=xhat1, rstd1=rstd1, a=a, qkv=qkv, P=P, o=o, h1=h1, xhat2=xhat2, rstd2=rstd2, bn=bn, f=f))
    y = gemm(ar, h, cv(top['out_w']).T, bias=cv(top['out_b']))
    tape['hfin'], tape['y'] = h, y
    out = axpby(ar, residual, x, 1 - f32(residual), y)
    return out.reshape(B, T, D), tape


def adapter_backward(ar, img, valid, top, blocks, heads, residual, tape, d_out, p=0.0, seed=0, colsum_tail_fault=False,
                     S=None):
    """The whole backward over an arithmetic from a tape -> (grads: (top dict, [layer dicts]), d_img, scratch dict as the
    FIRST layer leaves it: dy, dh, dh1, dtmp_d, dqkv, df).  S (a dict): filled, under flat_grads' names, with the magnitude
    through the last accumulator of every gradient with each upstream row at its largest magnitude (an element of dy carries
    the rounding of the whole row that the LayerNorms, the attention and the products before it mixed) and, for d w2, the
    activations f and o at the magnitude through THEIR accumulators."""
    B, T, D = img.shape
    R = B * T
    d, ffn = top['in_w'].shape[0], blocks[0]['w1'].shape[0]
    cv = lambda t: t.to(ar.dtype)     # noqa: E731
    x = cv(img).reshape(R, D)
    S = {} if S is None else S

    def rowmax(t):
        return t.abs().max(-1, keepdim=True).values.expand_as(t)

    def csum(name, X, Y=None):
        S[name] = (rowmax(X) * (1.0 if Y is None else Y.abs())).sum(0)
        if colsum_tail_fault:
            n = X.shape[0] // 32 * 32
            X, Y = X[:n], (None if Y is None else Y[:n])
        return colsum(ar, X, Y)

    def dw(name, dyv, xin, xmag=None):
        S[name] = rowmax(dyv).T @ (xin.abs() if xmag is None else xmag)
        return gemm(ar, dyv.T, xin)
    dy = axpby(ar, 1 - f32(residual), cv(d_out).reshape(R, D))
    gt = dict(out_w=dw('out_w', dy, tape['hfin']), out_b=csum('out_b', dy))
    dh = gemm(ar, dy, cv(top['out_w']))
    gl = [None] * len(blocks)
    sc = {}
    for l in range(len(blocks) - 1, -1, -1):
        w = {k: cv(v) for k, v in blocks[l].items()}
        t = tape['L'][l]
        ks = [cv(k) for k in _keeps(seed, p, l, B, T, d, heads, ffn)]
        dlin2 = dh * ks[3]
        # f is what a ReLU left of a sum that cancels: its rounding is that of the sum, |bn| |w1|^T + |b1|, not of |f|
        g = dict(w2=dw(f'{l}.w2', dlin2, t['f'], ks[2] * (t['bn'].abs() @ w['w1'].abs().T + w['b1'].abs())),
                 b2=csum(f'{l}.b2', dlin2))
        df = gemm(ar, dlin2, w['w2'])
        df = torch.where(t['f'] > 0, df * ar.t(keep_scale(p) if p > 0 else 1.0), torch.zeros_like(df))
        g.update(w1=dw(f'{l}.w1', df, t['bn']), b1=csum(f'{l}.b1', df))
        dbn = gemm(ar, df, w['w1'])
        g.update(ln2_g=csum(f'{l}.ln2_g', dbn, t['xhat2']), ln2_b=csum(f'{l}.ln2_b', dbn))
        dh1 = ln_bwd(ar, dbn, t['xhat2'], t['rstd2'], w['ln2_g'], dx0=dh)
        dlin_o = dh1 * ks[1]
        Pk = t['P'].abs() * (ks[0] if p > 0 else 1.0)           # o is a sum over the views that cancels: P |v|, not |o|
        o_mag = (Pk @ _heads(t['qkv'].reshape(B, T, 3 * d)[..., 2 * d:], heads).abs()).transpose(1, 2).reshape(R, d)
        g.update(o_w=dw(f'{l}.o_w', dlin_o, t['o'], o_mag), o_b=csum(f'{l}.o_b', dlin_o))
        dO = gemm(ar, dlin_o, w['o_w'])
        dqkv = attn_bwd(ar, t['qkv'].reshape(B, T, 3 * d), t['P'], dO.reshape(B, T, d), heads,
                        ks[0] if p > 0 else None).reshape(R, 3 * d)
        g.update(qkv_w=dw(f'{l}.qkv_w', dqkv, t['a']), qkv_b=csum(f'{l}.qkv_b', dqkv))
        da = gemm(ar, dqkv, w['qkv_w'])
        g.update(ln1_g=csum(f'{l}.ln1_g', da, t['xhat1']), ln1_b=csum(f'{l}.ln1_b', da))
        dh = ln_bwd(ar, da, t['xhat1'], t['rstd1'], w['ln1_g'], dx0=dh1)
        gl[l] = g
        sc = dict(dy=dy, dh=dh, dh1=dh1, dtmp_d=da, dqkv=dqkv, df=df)
    gt.update(in_w=dw('in_w', dh, x), in_b=csum('in_b', dh))
    C0 = axpby(ar, residual, cv(d_out).reshape(R, D))
    d_img = gemm(ar, dh, cv(top['in_w']), beta=1.0, C0=C0)
    # d h0 ends two sums that cancel (d a = d qkv W over 3 d terms, then norm1's backward): its unit is their magnitude
    S_dh, _ = ln_bwd_S(dqkv.abs() @ w['qkv_w'].abs(), t['xhat1'], t['rstd1'], w['ln1_g'], dx0=dh1)
    S['d_img'] = (rowmax(S_dh.to(ar.dtype)) @ cv(top['in_w']).abs() + C0.abs()).reshape(B, T, D)
    return (gt, gl), d_img.reshape(B, T, D), sc


def check_adapter_forward(img, valid, top, blocks, heads, residual, p, seed, out, tape, what):
    """Every tape slot of every layer (and out) against the float64 yardstick of that ONE stage applied to the implementation's
    own previous slot.  A layer's input beyond the first is restated from the previous layer's h1 and f (the slot was
    reused), its bound carried along.  -> {group: worst error / bound}."""
    B, T, D = img.shape
    R = B * T
    d, ffn = top['in_w'].shape[0], blocks[0]['w1'].shape[0]
    dd = lambda t: t.double()     # noqa: E731
    x = dd(img).reshape(R, D)
    W = {k: dd(v) for k, v in top.items()}
    worst = {}

    def rec(group, got, ref, key, S, E=0.0, name='', pure=True):
        worst[group] = max(worst.get(group, 0.0), within(got, ref, key, S, E, f'{what}: {name}', pure))
    S, _ = gemm_S(x, W['in_w'].T, bias=W['in_b'])
    rec('gemm', tape['h0'], gemm(A64, x, W['in_w'].T, bias=W['in_b']), ('gemm', D), S, name='h0')
    h, eh = dd(tape['h0']), None
    for l, bp in enumerate(blocks):
        w = {k: dd(v) for k, v in bp.items()}
        t = {k: dd(v) for k, v in tape['L'][l].items()}
        g = tape['L'][l]
        ks = _keeps(seed, p, l, B, T, d, heads, ffn)
        nm = lambda s: dict(name=f'layer {l} {s}')     # noqa: E731
        y, xhat, rstd = ln_fwd(A64, h, w['ln1_g'], w['ln1_b'])
        Sl = ln_fwd_S(h, w['ln1_g'], w['ln1_b'], eh)
        for k_, ref_ in (('a', y), ('xhat1', xhat), ('rstd1', rstd)):
            rec('ln_fwd', g[k_], ref_, 'ln_fwd', *Sl[{'a': 'y', 'xhat1': 'xhat', 'rstd1': 'rstd'}[k_]], pure=eh is None, **nm(k_))
        S, _ = gemm_S(t['a'], w['qkv_w'].T, bias=w['qkv_b'])
        rec('gemm', g['qkv'], gemm(A64, t['a'], w['qkv_w'].T, bias=w['qkv_b']), ('gemm', d), S, **nm('qkv'))
        k0 = ks[0] if p > 0 else None
        P, o = attn_fwd(A64, t['qkv'].reshape(B, T, 3 * d), valid, heads, k0)
        Sa = attn_fwd_S(t['qkv'].reshape(B, T, 3 * d), valid, heads, k0)
        rec('attn_fwd', g['P'], P, 'attn_fwd', *Sa['P'], **nm('P'))
        # o from the implementation's OWN saved P: one stage
        Pd = t['P'] if k0 is None else t['P'] * k0
        vh = _heads(t['qkv'].reshape(B, T, 3 * d)[..., 2 * d:], heads)
        o_ref = (Pd @ vh).transpose(1, 2).reshape(R, d)
        S_o = (2 * Pd @ vh.abs()).transpose(1, 2).reshape(R, d)
        rec('attn_fwd', g['o'], o_ref, 'attn_fwd', S_o, **nm('o'))
        lin = gemm(A64, t['o'], w['o_w'].T, bias=w['o_b'])
        S, _ = gemm_S(t['o'], w['o_w'].T, bias=w['o_b'])
        rec('gemm', g['h1'], h + ks[1] * lin, ('gemm', d), h.abs() + ks[1] * S + (h + ks[1] * lin).abs(),
            0.0 if eh is None else eh, pure=eh is None, **nm('h1'))
        y, xhat, rstd = ln_fwd(A64, t['h1'], w['ln2_g'], w['ln2_b'])
        Sl = ln_fwd_S(t['h1'], w['ln2_g'], w['ln2_b'])
        for k_, ref_, s_ in (('bn', y, 'y'), ('xhat2', xhat, 'xhat'), ('rstd2', rstd, 'rstd')):
            rec('ln_fwd', g[k_], ref_, 'ln_fwd', *Sl[s_], **nm(k_))
        S, _ = gemm_S(t['bn'], w['w1'].T, bias=w['b1'])
        rec('gemm', g['f'], ks[2] * gemm(A64, t['bn'], w['w1'].T, bias=w['b1'], relu=True), ('gemm', d), 2 * ks[2] * S, **nm('f'))
        lin = gemm(A64, t['f'], w['w2'].T, bias=w['b2'])
        S, _ = gemm_S(t['f'], w['w2'].T, bias=w['b2'])
        h = t['h1'] + ks[3] * lin                                   # the next layer's input, restated
        eh = bound(('gemm', ffn), t['h1'].abs() + ks[3] * S + h.abs())
    rec('gemm', tape['hfin'], h, ('gemm', ffn), 0.0, eh, name='hfin', pure=False)
    hf = dd(tape['hfin'])
    S, _ = gemm_S(hf, W['out_w'].T, bias=W['out_b'])
    rec('gemm', tape['y'], gemm(A64, hf, W['out_w'].T, bias=W['out_b']), ('gemm', d), S, name='y')
    yk = dd(tape['y'])
    rec('elementwise', out.reshape(R, D), axpby(A64, residual, x, 1 - f32(residual), yk), 'elementwise',
        axpby_S(residual, x, 1 - f32(residual), yk), name='out')
    return worst


def check_adapter_backward(img, valid, top, blocks, heads, residual, p, seed, tape, d_out, grads, d_img, scr, what):
    """layers = 1.  The scratch slots the layer leaves (df, dqkv, dtmp_d, dh1, dh, dy), every parameter gradient and d_img
    against ONE float64 stage applied to the implementation's own slots; where the direct input was overwritten (dh before
    the layer, d bn, d o) it is restated once from the slot before it, with its bound.  -> {group: worst}."""
    assert len(blocks) == 1
    B, T, D = img.shape
    R = B * T
    d, ffn = top['in_w'].shape[0], blocks[0]['w1'].shape[0]
    dd = lambda t: t.double()     # noqa: E731
    x, do = dd(img).reshape(R, D), dd(d_out).reshape(R, D)
    W = {k: dd(v) for k, v in top.items()}
    w = {k: dd(v) for k, v in blocks[0].items()}
    t = {k: dd(v) for k, v in tape['L'][0].items()}
    s = {k: dd(v) for k, v in scr.items()}
    gt, gl = grads
    ks = _keeps(seed, p, 0, B, T, d, heads, ffn)
    kscale = keep_scale(p) if p > 0 else 1.0
    worst = {}

    def rec(group, name, got, ref, key, S, E=0.0):
        pure = not torch.is_tensor(E)
        worst[group] = max(worst.get(group, 0.0), within(got, ref, key, S, E, f'{what}: {name}', pure))

    def lin_grads(name_w, name_b, dyv, xin, e=None, gw=None, gb=None):
        """dW = dy^T x, db = colsum(dy), dy known to within e"""
        S, E = gemm_S(dyv.T, xin, eA=None if e is None else e.T)
        rec('gemm', name_w, gw, dyv.T @ xin, ('gemm', R), S, E)
        S, E = colsum_S(dyv, eX=e)
        rec('colsum', name_b, gb, dyv.sum(0), 'colsum', S, E)
    rec('elementwise', 'dy', scr['dy'], axpby(A64, 1 - f32(residual), do), 'elementwise', axpby_S(1 - f32(residual), do))
    dy, hf = s['dy'], dd(tape['hfin'])
    lin_grads('d out_w', 'd out_b', dy, hf, gw=gt['out_w'], gb=gt['out_b'])
    dh0 = dy @ W['out_w']                                           # restated: the slot ends as d h0
    S, _ = gemm_S(dy, W['out_w'])
    e0 = bound(('gemm', D), S)
    dlin2, e2 = dh0 * ks[3], e0 * ks[3] + bound('elementwise', (dh0 * ks[3]).abs()) * (p > 0)
    lin_grads('d w2', 'd b2', dlin2, t['f'], e2, gw=gl[0]['w2'], gb=gl[0]['b2'])
    S, E = gemm_S(dlin2, w['w2'], eA=e2)
    on = (t['f'] > 0).double() * kscale
    rec('gemm', 'df', scr['df'], (dlin2 @ w['w2']) * on, ('gemm', d), 2 * S * on, E * on)
    df = s['df']
    lin_grads('d w1', 'd b1', df, t['bn'], gw=gl[0]['w1'], gb=gl[0]['b1'])
    dbn = df @ w['w1']                                              # restated: dtmp_d ends as d a
    S, _ = gemm_S(df, w['w1'])
    ebn = bound(('gemm', ffn), S)
    for nm_, Y in (('d ln2_g', t['xhat2']), ('d ln2_b', None)):
        S, E = colsum_S(dbn, Y, eX=ebn)
        rec('colsum', nm_, gl[0]['ln2_g' if Y is not None else 'ln2_b'], (dbn * (1.0 if Y is None else Y)).sum(0), 'colsum', 2 * S, E)
    S, E = ln_bwd_S(dbn, t['xhat2'], t['rstd2'], w['ln2_g'], dx0=dh0, edy=ebn, edx0=e0)
    rec('ln_bwd', 'dh1', scr['dh1'], ln_bwd(A64, dbn, t['xhat2'], t['rstd2'], w['ln2_g'], dx0=dh0), 'ln_bwd', S, E)
    dh1 = s['dh1']
    dlo, elo = dh1 * ks[1], bound('elementwise', (dh1 * ks[1]).abs()) * (p > 0)
    lin_grads('d o_w', 'd o_b', dlo, t['o'], elo if p > 0 else None, gw=gl[0]['o_w'], gb=gl[0]['o_b'])
    dO = dlo @ w['o_w']                                             # restated: dtmp_d is overwritten
    S, E = gemm_S(dlo, w['o_w'], eA=elo if p > 0 else None)
    eO = bound(('gemm', d), S, E)
    k0 = ks[0] if p > 0 else None
    q3 = t['qkv'].reshape(B, T, 3 * d)
    S, E = attn_bwd_S(q3, t['P'], dO.reshape(B, T, d), heads, k0, edO=eO.reshape(B, T, d))
    rec('attn_bwd', 'dqkv', scr['dqkv'].reshape(B, T, 3 * d), attn_bwd(A64, q3, t['P'], dO.reshape(B, T, d), heads, k0),
        'attn_bwd', S, E)
    dq = s['dqkv']
    lin_grads('d qkv_w', 'd qkv_b', dq, t['a'], gw=gl[0]['qkv_w'], gb=gl[0]['qkv_b'])
    S, _ = gemm_S(dq, w['qkv_w'])
    rec('gemm', 'dtmp_d', scr['dtmp_d'], dq @ w['qkv_w'], ('gemm', 3 * d), S)
    da = s['dtmp_d']
    for nm_, Y in (('d ln1_g', t['xhat1']), ('d ln1_b', None)):
        S, E = colsum_S(da, Y)
        rec('colsum', nm_, gl[0]['ln1_g' if Y is not None else 'ln1_b'], (da * (1.0 if Y is None else Y)).sum(0), 'colsum', 2 * S)
    S, E = ln_bwd_S(da, t['xhat1'], t['rstd1'], w['ln1_g'], dx0=dh1)
    rec('ln_bwd', 'dh', scr['dh'], ln_bwd(A64, da, t['xhat1'], t['rstd1'], w['ln1_g'], dx0=dh1), 'ln_bwd', S, E)
    dh = s['dh']
    lin_grads('d in_w', 'd in_b', dh, x, gw=gt['in_w'], gb=gt['in_b'])
    C0 = axpby(A32, residual, d_out.reshape(R, D)).double()         # r d_out as the fp32 value the first launch left
    S, _ = gemm_S(dh, W['in_w'], beta=1.0, C0=C0)
    rec('gemm', 'd_img', d_img.reshape(R, D), dh @ W['in_w'] + C0, ('gemm', d), S)
    return worst


def check_grads_end_to_end(got, want, S, layers, what):
    """Gradients of a deep chain against the float64 replay (itself confirmed against torch autograd), per element:
    |got - want| <= KERNEL_FACTOR c 2^-24 S with S the magnitude through the LAST accumulator of each gradient (rowmax|dy|^T
    |x|, sum rowmax|dy|, ...: adapter_backward) from the float64 replay and c = 'chain<layers>': what the F32 restatement of the whole chain loses against
    float64 in that unit -- the rounding of every earlier stage arrives through dy.  -> worst ratio."""
    worst = 0.0
    for k in want:
        worst = max(worst, within(got[k], want[k].double(), f'chain{layers}', S[k], 0.0, f'{what}: {k}'))
    return worst


def flat_grads(grads, d_img):
    gt, gl = grads
    out = {k: v for k, v in gt.items()}
    for l, g in enumerate(gl):
        out.update({f'{l}.{k}': v for k, v in g.items()})
    out['d_img'] = d_img
    return out
