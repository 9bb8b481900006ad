"""Float64 yardsticks, directed inputs and error bounds for the row kernels of csrc/layernorm.hip: the LayerNorm family,
the row statistics and their merge, the hi / lo splits and joins, the two embeddings.

Nothing here touches a GPU or anything compiled: the references are plain torch float64 and run on whatever device their
input lives on, the inputs are built on the CPU from a seed, the fp32 restatements (what an fp32 implementation of the
same formula loses against float64) are written with a fixed summation order, so that they give the same bits on any
machine.  tests/test_rowops_ref_cpu.py measures the constants below with them; tests/test_rowops_gpu.py holds the
kernels to the bounds.

Bounds, per element, never the largest error over the largest value:
    16-bit output:   |out - ref|     <= u |ref| + FLOOR16 + E          u = 2^-11 (f16) / 2^-8 (bf16)
    hi + lo, fp32:   |hi + lo - ref| <= pair |ref| + pair floor + E    pair = 2^-22 / 2^-16 / 2^-19 (bf16 hi, fp16 lo)
    E = KERNEL_FACTOR C 2^-23 s,   s = max_c |gamma xhat| + max_c |beta| of the row
C depends on the kind of row (its conditioning: an fp32 mean of a row around 1000 is off by some 1e-4, which is
1e-4 rstd in every output): one constant per kind, measured, so that the ordinary rows are not held to the bound the
large-mean rows need.
"""
import functools

import torch

EC_F16, EC_BF16 = 0, 1
DTYPES = {'float16': torch.float16, 'bfloat16': torch.bfloat16}
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # half an ulp, relative
FLOOR16 = 2.0 ** -24                                            # the f16 subnormal step
FLOOR_PAIR = 2.0 ** -25       # a pair whose lo part is fp16 (or whose hi part is): half a subnormal step where lo underflows
# QuickGELU in fp32: beyond 1.702 |x| = 88.7 expf overflows and the quotient is 0 where the true value is |x| / e^88.7 =
# 1.5e-37 at most (and below 2^-126 an fp32 result may be flushed)
FLOOR_GELU = 2.0 ** -120
EPS32 = 2.0 ** -23


def pair_u(hi_dtype, lo_dtype):
    """Relative error of hi = round(v), lo = round(v - hi): the product of the two half-ulps."""
    return U[hi_dtype] * U[lo_dtype]


# Kinds of rows (ln_rows).  A bound met because hard rows were left out is no bound: every case holds all four.
ORDINARY, LARGE_MEAN, NEAR_EPS, CONSTANT = 0, 1, 2, 3
KINDS = ('ordinary', 'large_mean', 'near_eps', 'constant')

# ---------------------------------------------------------------------------------------------------------------
# The measured constants.  tests/test_rowops_ref_cpu.py computes, over every input the GPU tests use, the smallest C
# with which the fp32 restatement below (two passes, a butterfly sum, 1 / sqrt) stays within C 2^-23 s of float64, and
# asserts that it is below the figure here (the measured value, rounded up; the measurements are in the comments).
# The kernels are held to KERNEL_FACTOR times that: the factor covers a different summation order (a 64-lane butterfly
# over per-lane partial sums against the restatement's tree) and one differently rounded reciprocal root, nothing more.
# ---------------------------------------------------------------------------------------------------------------
KERNEL_FACTOR = 4.0
# LayerNorm (layernorm32 against layernorm64), by kind of row.  Constant rows are built from values whose fp32 sums are
# exact in ANY order (2.5 2^k and -0.75 2^k over <= 2048 columns): mean exact, variance 0, the output is beta itself
# and the restatement's error is 0; the stored 1 allows one rounding.
# Measured: ordinary 5.27, large mean 4600 (the mean of a row around -300 is off by a few 2^-24 of 300, and that over a
# deviation of 0.05 is in every output; the figure is set at width 4, where s is smallest), near epsilon 4.85, constant 0.
C_LN = {ORDINARY: 5.8, LARGE_MEAN: 5100.0, NEAR_EPS: 5.4, CONSTANT: 1.0}
# Row statistics of 16-bit rows (row_stats32 against row_stats64): relative error of rstd in units of 2^-23, and error of
# -rstd mean in units of 2^-23 rstd max|x|.  Measured: 1.64, 3.13, 1.13, 0.66.
C_STATS = {ORDINARY: 1.8, LARGE_MEAN: 3.5, NEAR_EPS: 1.2, CONSTANT: 1.0}
# The merge of group sums (merge32 against merge64): var = E[x^2] - mean^2 loses 2^-23 sum(q) / width ABSOLUTE, so rstd
# loses that over 2 (var + eps) relative; the bound is C 2^-23 (1 + (sum(q) / width) / (2 (var + eps))), the 1 for the
# roundings of the root and the division where the subtraction loses nothing
# (-rstd mean: the same relative figure against rstd sum|group sums| / width).  Measured: 1.93.
C_MERGE = 2.1
# QuickGELU in fp32 (gelu32 against gelu64): relative error in units of 2^-23 (1 + |1.702 x|): the exponent's rounding
# is relative to the exponent, so it grows with it.  Measured: 1.20.
C_GELU = 1.35

# ---------------------------------------------------------------------------------------------------------------
# shapes the CPU and GPU tests share
# ---------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (4, 64, 252, 256, 260, 772, 1024, 1284, 2044, 2048)
ROWS = (1, 3, 4, 5, 1021)
STATS_WIDTHS = (8, 504, 512, 520, 2040, 2048)
MERGE_GROUPS = (1, 4, 15, 16, 17, 20, 31, 32)
MERGE_ROWS = (1, 15, 16, 17, 1000)
EPS = (1e-5, 1e-3)
SPLIT_N = (4, 1020, 1028)
SPLIT_N_LARGE = 65536 * 1024 + 1028          # one trip of the capped grid and 1028 elements of a second
EMBED_SHAPES = ((1, 2), (3, 5), (2, 50))     # (n_img, seq)
EMBED_WIDTHS = (4, 260, 768, 1284)
TEXT_CTX = (1, 77)
TEXT_WIDTHS = (4, 260, 512, 1280)
JOIN_SHAPES = ((1, 4), (5, 260), (4104, 1024))   # 4104 x 1024 / 4 float4 units: one trip past 4096 workgroups of 256


def rotations(rows):
    """The row pattern of ln_rows has period 8; a case with fewer rows is run at every rotation, so that it still meets
    every kind of row."""
    return tuple(range(8)) if rows < 8 else (0, 3)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gamma_beta(width):
    """Column identity: a vector unit that is swapped, dropped or read from the wrong column shows far above tolerance."""
    c = torch.arange(width, dtype=torch.float64)
    return (1 + c / width).float(), (0.01 * c).float()


_PATTERN_KIND = (ORDINARY, LARGE_MEAN, NEAR_EPS, CONSTANT, ORDINARY, LARGE_MEAN, ORDINARY, CONSTANT)


@functools.lru_cache(maxsize=256)
def ln_rows(rows, width, rot=0):
    """-> (x fp32 [rows, width], kind int64 [rows]) on the CPU; read-only.  Row r follows pattern (r + rot) % 8:
    0, 6 Gaussian (mean 0.3, deviation 1) scaled by 2^((r + rot) % 7 - 3);  4 the same with one outlier channel x 40;
    1 mean 1000, deviation 1;  5 mean -300, deviation 0.05 (a one-pass variance is lost on both);
    2 mean 0.02, deviation 3e-3: the variance 9e-6 beside eps = 1e-5 (the noise of 1, 5 and 2 is divided by its own deviation,
    so that the row has the promised deviation at every width, four columns included);
    3, 7 constant 2.5 2^k and -0.75 2^k: variance exactly 0 in any summation order."""
    z = torch.randn(rows, width, generator=_gen(9000 + 31 * width + 7 * rows + rot), dtype=torch.float64)
    r = torch.arange(rows) + rot
    scale = (2.0 ** (r % 7 - 3).double())[:, None]
    pat = r % 8
    x = (z + 0.3) * scale
    z = z / z.std(-1, unbiased=False, keepdim=True)
    oc = min(7, width - 1)
    x[pat == 4, oc] *= 40
    x = torch.where((pat == 1)[:, None], 1000 + z, x)
    x = torch.where((pat == 5)[:, None], -300 + 0.05 * z, x)
    x = torch.where((pat == 2)[:, None], 0.02 + 3e-3 * z, x)
    x = torch.where((pat == 3)[:, None], 2.5 * scale.expand_as(x), x)
    x = torch.where((pat == 7)[:, None], -0.75 * scale.expand_as(x), x)
    return x.float(), torch.tensor(_PATTERN_KIND)[pat]


def split(x, hi_dtype, lo_dtype):
    """fp32 -> (hi, lo): hi = round(x), lo = round(x - hi) (x - hi is exact in fp32)."""
    hi = x.to(hi_dtype)
    return hi, (x - hi.float()).to(lo_dtype)


def split_input(n, seed=0, device='cpu'):
    """fp32 [n] for the split kernels: Gaussian x 3 with stretches around +-20 (1 + e^34 = e^34 in fp32), +-60 (expf
    overflows: the quotient is x / inf) and tiny values (the lo part underflows)."""
    g = torch.Generator(device=device).manual_seed(7000 + seed)
    x = torch.randn(n, generator=g, device=device) * 3
    k = torch.arange(n, device=device)
    x = torch.where(k % 16 == 3, 20 + 0.5 * x, x)
    x = torch.where(k % 16 == 7, -20 + 0.5 * x, x)
    x = torch.where(k % 16 == 11, 60 + x, x)
    x = torch.where(k % 16 == 13, -60 + x, x)
    return torch.where(k % 16 == 15, x * 1e-6, x)


def merge_sums(rows, groups, dtype=torch.float16, rot=0):
    """-> (sums fp32 [rows, groups, 2], kind): float64 (sum, sum of squares) over each 64-column group of ln_rows
    rounded to `dtype` (what EC_EPI_RESID_HL leaves: sums of the hi plane), rounded to fp32.  No GEMM in front.
    The sums of a truly constant 16-bit row are exact in fp32 (a square of 11 bits has 22) and its E[x^2] - mean^2 is 0
    on the dot; the rows that go BELOW zero are the large-mean ones, which 16 bits leave all but constant (-300 +- 0.05
    in steps of 0.25 or 2): sum(q) / width = 9e4 carries 5e-3 of rounding beside a variance of 1e-3 or 0."""
    x, kind = ln_rows(rows, 64 * groups, rot)
    x = x.to(dtype).double().view(rows, groups, 64)
    return torch.stack([x.sum(-1), (x * x).sum(-1)], -1).float(), kind


def embed_inputs(n_img, seq, width):
    """patch [n_img (seq - 1), width], cls [width], pos [seq, width] fp32: patch rows differ by image and position (an
    offset 0.25 n + 0.01 p on top of the noise), the class row is unlike any patch row."""
    g = _gen(5000 + 131 * n_img + 17 * seq + width)
    patch = torch.randn(n_img, seq - 1, width, generator=g, dtype=torch.float64)
    patch = patch * (2.0 ** (torch.arange(seq - 1) % 7 - 3).double())[None, :, None]
    patch = patch + 0.25 * torch.arange(n_img)[:, None, None] + 0.01 * torch.arange(seq - 1)[None, :, None]
    cls = 3 + torch.randn(width, generator=g, dtype=torch.float64)
    pos = 0.5 * torch.randn(seq, width, generator=g, dtype=torch.float64)
    return patch.reshape(-1, width).float(), cls.float(), pos.float()


def embed_sum(patch, cls, pos, n_img, seq):
    """The fp32 sum src + pos the embedding kernels normalise ([n_img seq, width]; `pre` of ec_vit_embed_train)."""
    width = pos.shape[1]
    src = torch.cat([cls.expand(n_img, 1, width), patch.view(n_img, seq - 1, width)], 1)
    return (src + pos[None]).reshape(n_img * seq, width)


TEXT_VOCAB = 37


def text_inputs(n_txt, ctx, width):
    """tokens int32 [n_txt, ctx] with -5, 0, vocab - 1, vocab and vocab + 7 among them, table [vocab, width], pos."""
    g = _gen(6000 + 77 * n_txt + ctx + width)
    n = n_txt * ctx
    assert n >= 5
    tok = torch.randint(0, TEXT_VOCAB, (n,), generator=g, dtype=torch.int32)
    tok[torch.arange(5) * (n // 5)] = torch.tensor([-5, 0, TEXT_VOCAB - 1, TEXT_VOCAB, TEXT_VOCAB + 7], dtype=torch.int32)
    table = torch.randn(TEXT_VOCAB, width, generator=g) + torch.arange(TEXT_VOCAB)[:, None]
    return tok.view(n_txt, ctx), table, torch.randn(ctx, width, generator=g)


def text_embed_ref(tok, table, pos):
    t = tok.long().clamp(0, table.shape[0] - 1)
    return table[t] + pos[None]


# ---------------------------------------------------------------------------------------------------------------
# references (float64) and the quantities the bounds scale with
# ---------------------------------------------------------------------------------------------------------------
def layernorm64(x, gamma, beta, eps):
    """-> (LayerNorm of x in float64: biased variance, eps inside the root;  s [rows] = max |gamma xhat| + max |beta|)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    xhat = d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return xhat * gamma + beta, (xhat * gamma).abs().amax(-1) + beta.abs().max()


def row_stats64(x, eps):
    """-> (rstd, -rstd mean) [rows, 2] in float64."""
    x = x.double()
    mean = x.mean(-1)
    d = x - mean[:, None]
    rstd = 1 / torch.sqrt((d * d).mean(-1) + eps)
    return torch.stack([rstd, -rstd * mean], -1)


def merge64(sums, width, eps):
    """Group sums -> (stats [rows, 2], cond [rows], absum [rows]) in float64.  The variance of the sums AS GIVEN (fp32
    numbers), clamped at 0 like the kernel's: below 0 the data cannot be, only the rounded sums.  cond = (sum(q) / width)
    / (2 (var + eps)); absum = sum |group sums| / width."""
    s, q = sums.double()[..., 0], sums.double()[..., 1]
    mean, eq = s.sum(-1) / width, q.sum(-1) / width
    var = (eq - mean * mean).clamp(min=0)
    rstd = 1 / torch.sqrt(var + eps)
    return torch.stack([rstd, -rstd * mean], -1), eq / (2 * (var + eps)), s.abs().sum(-1) / width


def gelu64(x):
    x = x.double()
    return x / (1 + torch.exp(-1.702 * x))


# ---------------------------------------------------------------------------------------------------------------
# fp32 restatements: the same formulas in fp32 with a FIXED summation order (a tree over the zero-padded row), the
# yardstick for what fp32 arithmetic itself loses
# ---------------------------------------------------------------------------------------------------------------
def tree_sum32(x):
    """Sum over the last axis in fp32, halves added elementwise until one column is left: the same bits everywhere."""
    assert x.dtype == torch.float32
    n = 1
    while n < x.shape[-1]:
        n *= 2
    x = torch.nn.functional.pad(x, (0, n - x.shape[-1]))
    while n > 1:
        n //= 2
        x = x[..., :n] + x[..., n:]
    return x[..., 0]


def layernorm32(x, gamma, beta, eps):
    assert x.dtype == torch.float32
    w = x.shape[-1]
    mean = tree_sum32(x) / w
    d = x - mean[:, None]
    rstd = 1 / torch.sqrt(tree_sum32(d * d) / w + torch.tensor(eps, dtype=torch.float32))
    return d * rstd[:, None] * gamma + beta


def row_stats32(x, eps):
    x = x.float()
    w = x.shape[-1]
    mean = tree_sum32(x) / w
    d = x - mean[:, None]
    rstd = 1 / torch.sqrt(tree_sum32(d * d) / w + torch.tensor(eps, dtype=torch.float32))
    return torch.stack([rstd, -rstd * mean], -1)


def merge32(sums, width, eps, clamp=True):
    """-> (stats, var before the clamp) in fp32."""
    mean = tree_sum32(sums[..., 0].contiguous()) / width
    var = tree_sum32(sums[..., 1].contiguous()) / width - mean * mean
    rstd = 1 / torch.sqrt((var.clamp(min=0) if clamp else var) + torch.tensor(eps, dtype=torch.float32))
    return torch.stack([rstd, -rstd * mean], -1), var


def gelu32(x):
    assert x.dtype == torch.float32
    return x / (1 + torch.exp(torch.tensor(-1.702, dtype=torch.float32) * x))


# ---------------------------------------------------------------------------------------------------------------
# bounds: each returns a tensor of the reference's shape, float64
# ---------------------------------------------------------------------------------------------------------------
def _c_of(kind, table, device):
    return torch.tensor([table[k] for k in range(4)], dtype=torch.float64, device=device)[kind.to(device)]


def ln_e(s, kind, factor=KERNEL_FACTOR):
    """E [rows, 1] of the LayerNorm outputs."""
    return (factor * _c_of(kind, C_LN, s.device) * EPS32 * s)[:, None]


def bound16(ref, e, dtype):
    return U[dtype] * ref.abs() + FLOOR16 + e


def bound_pair(ref, e, hi_dtype, lo_dtype):
    floor = FLOOR_PAIR if torch.float16 in (hi_dtype, lo_dtype) else 0.0
    return pair_u(hi_dtype, lo_dtype) * ref.abs() + floor + e


def stats_bound(ref, xmax, kind, factor=KERNEL_FACTOR):
    """[rows, 2]: rstd relative, -rstd mean against rstd max|x| (the mean may be 0)."""
    c = factor * _c_of(kind, C_STATS, ref.device) * EPS32
    return torch.stack([c * ref[:, 0], c * ref[:, 0] * xmax], -1)


def merge_bound(ref, cond, absum, factor=KERNEL_FACTOR):
    rel = factor * C_MERGE * EPS32 * (1 + cond)
    return torch.stack([rel * ref[:, 0], rel * ref[:, 0] * absum], -1)


def gelu_e(x, ref, factor=KERNEL_FACTOR):
    return factor * C_GELU * EPS32 * (1 + (1.702 * x.double()).abs()) * ref.abs() + FLOOR_GELU


def excess(got, ref, bound):
    """Largest amount by which |got - ref| passes the bound (<= 0: within), as a float; NaN anywhere -> inf."""
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    return float(((got.double() - ref).abs() - bound).max())
