"""Float64 yardsticks, directed inputs and error bounds for the forward tail: ec_classify_v2 (csrc/classify.hip: logits
on the matrix pipe from hi + lo fp16 parts, the scatter by row_idx, the view aggregations, the per-view softmax mean)
and ec_pseudo_label (csrc/pseudo_label.hip).

Nothing here touches a GPU or anything compiled.  The references are plain torch float64; the inputs are built on the
CPU from a seed; the restatements (`classify32`, `pseudo_label32`: the kernels' arithmetic step by step) use a fixed
summation order and take exp through float64, so that they give the same bits on any machine.
tests/test_classify_ref_cpu.py measures the constants below with them and shows that restatements broken on purpose
fail the bounds; tests/test_classify_edges_gpu.py holds the kernels to the bounds.

Bounds, per element, never the largest error over the largest value.  With f the feature row (after F.normalize in
float64 where that applies), t the class row, S = sum_c |f_c| |t_c| and F = max|f| sum|t| + sum|f| max|t|:

    |logit - ref| <= KERNEL_FACTOR ( |scale| ( C_REP (2^-22 S + 2^-35 F) + C_ACC 2^-24 S + [normalize] 2^-24 S )
                                     + [normalize] C_NORM 2^-23 |ref| + 2^-24 |ref| )

  2^-22 S        two fp16 parts hold 22 bits of each operand; the lo . lo product, which is never formed, is 2^-22 S too
  2^-35 F        the lo part of an element far below its row's maximum is an fp16 subnormal: steps of 2^-24 (half a
                 step: 2^-25) under a row maximum scaled into [2^10, 2^11), i.e. 2^-35 of the row's maximum per element
  C_ACC 2^-24 S  the fp32 accumulation of the three products
  2^-24 S        under normalize: the rounding of each element's division by the norm (one rounding: not measured)
  C_NORM         under normalize: the relative error of the fp32 norm (sum of squares, root), common to the whole row
  2^-24 |ref|    the one rounded multiplication that undoes the scales (everything else there is a power of two)
Aggregated logits take the sum of their views' bounds and 2^-24 sum|views| per addition (mean: over the count, and one
more rounding); max takes the largest view bound.  A probability p = softmax(l)_k of a view is bounded by
    the distance p can move when every logit of the view moves by the view's largest logit bound L (computed exactly:
      p / (p + (1 - p) e^(+-2L)), which is 2 L p (1 - p) to first order and stays a bound when L is large)
    + KERNEL_FACTOR C_SM 2^-23 (1 + |l - max|) p    (the subtraction's rounding is relative to the exponent)
    + FLOOR_PROB                                    (expf underflows below e^-87: the quotient is 0 or flushed)
and the sample's probability by the mean of its valid views' bounds and (T + 1) 2^-24 p for the additions and the division.
"""
import collections
import functools

import torch

AGGS = ('sum', 'mean', 'max')
AGG_CODE = {'sum': 0, 'mean': 1, 'max': 2}
CL_MAXT = 16
LOGIT_SCALE = 100.0
EPS32 = 2.0 ** -23
FLOOR_PROB = 2.0 ** -120      # as rowops_ref.FLOOR_GELU: below 2^-126 an fp32 quotient may be flushed; e^-87.3 = 2^-126
F32, F64 = torch.float32, torch.float64

# ---------------------------------------------------------------------------------------------------------------
# The measured constants.  tests/test_classify_ref_cpu.py computes each over every input the GPU tests use -- the
# restatement against float64, never the kernel -- and asserts that it is below the figure here (the measured value,
# rounded up; the measurements are in the comments).  The kernels are held to KERNEL_FACTOR times the bound: the factor
# covers a different summation order (the MFMA chain over three segments of C / 16 steps against the restatement's
# tree, a 64-lane butterfly against a tree) and one differently rounded operation (expf, log2f at a power of two).
# ---------------------------------------------------------------------------------------------------------------
KERNEL_FACTOR = 4.0
# three exact products of the hi / lo parts against the product of the fp32 operands that were split: each part pair
# rounds its lo at 2^-23 of the element and the lo . lo product is missing.  Measured: 1.43 un-normalised (the massive-channel
# rows), 1.23 under normalize
C_REP = 1.5
# fp32 tree accumulation (eight levels at C = 192) of the three products against their exact sum; the rows with one
# dominant channel round at the size of S on every level.  Measured: 5.18
C_ACC = 5.5
# relative error of the fp32 norm, in units of 2^-23.  Measured: 1.05
C_NORM = 1.1
# per-view softmax of the restatement against the float64 softmax of the same fp32 logits.  Measured: 1.02
C_SM = 1.1


# ---------------------------------------------------------------------------------------------------------------
# shapes the CPU and GPU tests share
# ---------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'B T K C layout masked m4')
TS = (1, 2, 15, 16)
KS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
CS = (1, 3, 63, 64, 65, 129, 192)
LAYOUTS = ('compact', 'dense', 'permuted')


def _cases():
    """A covering list, not the product: 40 cases in which every T, K, C, B, layout and n_rows % 4 occurs, every K with
    masked views (the multiples of 16 among them: Kp == K), T = 16 masked.  tests/test_classify_ref_cpu.py asserts it."""
    out = []
    for i in range(40):
        T = TS[(i + i // 4) % 4]
        out.append(Case(B=(1, 3)[(i // 2 + i // 12) % 2], T=T, K=KS[i % 12], C=CS[(i + i // 7) % 7],
                        layout=LAYOUTS[(i + i // 12) % 3], masked=T > 1 and i % 5 != 4, m4=(i + i // 4 + i // 16) % 4))
    return tuple(out)


CASES = _cases()


def valid_mask(case):
    """[B, T] bool.  Masked: view (b, t) is invalid where (b T + t) % 3 == 1 -- every sample keeps a valid view, and at
    T = 16 sample 1 loses its first."""
    B, T = case.B, case.T
    if not case.masked:
        return torch.ones(B, T, dtype=torch.bool)
    return (torch.arange(B * T) % 3 != 1).view(B, T)


def layout(case, valid=None):
    """-> (row_idx int32 [B, T], n_rows).  compact: the valid views numbered in order;  dense: row b T + t, the rows of
    invalid views exist and hold data;  permuted: the compact numbering reversed, and the last valid view reads the row
    of the first (one row used twice, one by nobody).  Unused rows are appended until n_rows % 4 == case.m4."""
    valid = valid_mask(case) if valid is None else valid
    B, T = valid.shape
    nv = int(valid.sum())
    idx = torch.full((B * T,), -1, dtype=torch.int64)
    where = valid.flatten().nonzero().flatten()
    if case.layout == 'dense':
        idx[where] = where
        n = B * T
    else:
        rows = torch.arange(nv)
        if case.layout == 'permuted':
            rows = rows.flip(0)
            if nv >= 2:
                rows[-1] = rows[0]
        idx[where] = rows
        n = nv
    return idx.view(B, T).to(torch.int32), n + (case.m4 - n) % 4


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
ORDINARY, MASSIVE, RANGE, POW2, POW2_BELOW, POW2_ABOVE, ZERO, ORTHO, BIG, SMALL = range(10)
KINDS = ('ordinary', 'massive', 'range', 'pow2', 'pow2_below', 'pow2_above', 'zero', 'ortho', 'big', 'small')
N_KINDS = len(KINDS)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def magnitude(normalize):
    """The exponent of the BIG / SMALL rows: 2^+-80 un-normalised (every logit against a class row of up to 1e3 stays
    finite: 100 x 2^80 x 1e3 x C = 2e34), 2^+-40 under normalize (the fp32 sum of squares, 2^+-80 C, stays normal)."""
    return 40 if normalize else 80


@functools.lru_cache(maxsize=None)
def text_rows(K, C):
    """fp32 [K, C], read-only.  Class k: a unit row; k % 4 == 1: a unit row x 10^-3, 10^3, 10^-2, 10^2, 10^-1, 10, 1 in
    turn (both ends from K = 6 on);  class K // 2 (K >= 2): all zero."""
    t = torch.randn(K, C, generator=_gen(4000 + 13 * K + C), dtype=F64)
    t = t / t.norm(dim=-1, keepdim=True)
    k = torch.arange(K)
    mag = torch.tensor([-3.0, 3.0, -2.0, 2.0, -1.0, 1.0, 0.0], dtype=F64)[(k // 4) % 7]
    t = torch.where((k % 4 == 1)[:, None], t * (10.0 ** mag)[:, None], t)
    if K >= 2:
        t[K // 2] = 0
    return t.float()


@functools.lru_cache(maxsize=None)
def feature_rows(n, C, normalize, rot=0):
    """-> (feats fp32 [n, C], kind int64 [n]), read-only.  Row r is of kind (r + rot) % 10:
    ordinary   Gaussian (deviation 0.5) x 2^((r + rot) % 5 - 2)
    massive    the same with channel min(7, C - 1) at 2^12 times an ordinary element (a deviation or more: never small by chance)
    range      +-10^-6u, u uniform: 1e-6 .. 1 within the row, both ends present (C >= 2)
    pow2, pow2_below, pow2_above   |elements| <= 0.9 x 2^k and one element +-2^k, one fp32 step below it, one above
               (k = (r + rot) % 7 - 3): floor(log2(max)) decides the scale.  Under normalize the maximum lands where the
               division leaves it
    zero       all zero, on whatever view reads it
    ortho      an ordinary row made orthogonal to class row 0 in float64 (C >= 2; at C = 1 it stays ordinary): the
               reference logit is the fp32 rounding's leftover, S is as large as any
    big, small an ordinary row x 2^+-magnitude(normalize)."""
    g = _gen(3000 + 101 * n + 7 * C + rot + 50 * int(normalize))
    z = 0.5 * torch.randn(n, C, generator=g, dtype=F64)
    u = torch.rand(n, C, generator=g, dtype=F64)
    r = torch.arange(n) + rot
    kind = r % N_KINDS
    x = z * (2.0 ** (r % 5 - 2).double())[:, None]
    oc = min(7, C - 1)
    x[:, oc] = torch.where(kind == MASSIVE, torch.sign(z[:, oc]) * (0.5 + z[:, oc].abs()) * 2.0 ** (r % 5 + 10).double(), x[:, oc])
    rng = torch.sign(z) * 10.0 ** (-6 * u)
    rng[:, 0] = 1.0
    if C >= 2:
        rng[:, C - 1] = -1e-6
    x = torch.where((kind == RANGE)[:, None], rng, x)
    top = 2.0 ** (r % 7 - 3).double()
    p2 = (z * 0.5).clamp(-0.9, 0.9) * top[:, None]
    top32 = top.float()
    peak = torch.where(kind == POW2_BELOW, torch.nextafter(top32, torch.zeros(n)),
                       torch.where(kind == POW2_ABOVE, torch.nextafter(top32, torch.full((n,), float('inf'))), top32)).double()
    p2[torch.arange(n), r % C] = peak * torch.where(r % 2 == 0, 1.0, -1.0).double()
    x = torch.where(((kind >= POW2) & (kind <= POW2_ABOVE))[:, None], p2, x)
    x = torch.where((kind == ZERO)[:, None], torch.zeros_like(x), x)
    x = torch.where((kind == BIG)[:, None], x * 2.0 ** magnitude(normalize), x)
    x = torch.where((kind == SMALL)[:, None], x * 2.0 ** -magnitude(normalize), x)
    kind = kind.clone()
    if C < 2:
        kind[kind == ORTHO] = ORDINARY
    return x, kind


Inputs = collections.namedtuple('Inputs', 'feats text row_idx valid kind n_rows scale')


@functools.lru_cache(maxsize=None)
def inputs(case, rot, normalize):
    """Everything one call of a shared case takes, on the CPU, read-only: feats fp32 [n_rows, C], text fp32 [K, C],
    row_idx int32 [B, T], valid bool [B, T], kind int64 [n_rows]."""
    valid = valid_mask(case)
    row_idx, n_rows = layout(case, valid)
    x, kind = feature_rows(n_rows, case.C, bool(normalize), rot)
    text = text_rows(case.K, case.C)
    t0 = text[0].double()
    if case.C >= 2 and float(t0.abs().max()) > 0:
        orth = x - (x @ t0 / (t0 @ t0))[:, None] * t0
        x = torch.where((kind == ORTHO)[:, None], orth, x)
    return Inputs(x.float(), text, row_idx, valid, kind, n_rows, LOGIT_SCALE)


def kinds_seen(case, rot, normalize=False):
    """The kinds of the rows that VALID views read."""
    row_idx, n_rows = layout(case)
    kind = feature_rows(n_rows, case.C, bool(normalize), rot)[1]
    return set(kind[row_idx[row_idx >= 0].long()].tolist())


@functools.lru_cache(maxsize=None)
def rotations(case):
    """The fewest rotations of the row pattern (greedy, lowest first) at which the valid views of `case` have read a row
    of every kind: a bound met because the hard rows were left out is no bound."""
    want = set(range(N_KINDS)) - ({ORTHO} if case.C < 2 else set())
    seen, rots = set(), []
    while seen != want:
        gain = [len((kinds_seen(case, r) & want) - seen) for r in range(N_KINDS)]
        best = max(range(N_KINDS), key=lambda r: (gain[r], -r))
        assert gain[best] > 0, (case, seen)
        rots.append(best)
        seen |= kinds_seen(case, best) & want
    return tuple(rots)


EXACT_SCALE = 0.125


@functools.lru_cache(maxsize=None)
def exact_inputs(case):
    """Small integers, logit_scale a power of two: every product hi . hi, lo . hi is an integer (x the rows' powers of
    two), every partial sum in any order is below 2^24 of them, so fp32 accumulation is exact whatever its order and so
    are the view sums.  Features: integers within +-63, four columns of each row within +-4095 (twelve bits: hi AND
    lo parts), row 2 all zero; classes within +-15 (lo = 0: the lo . lo product that is never formed is 0), class K // 2
    zero.  Asserted: sum_c |f_c| |t_c| x T < 2^24."""
    valid = valid_mask(case)
    row_idx, n_rows = layout(case, valid)
    g = _gen(8000 + 17 * case.K + case.C + n_rows)
    f = torch.randint(-63, 64, (n_rows, case.C), generator=g)
    wide = torch.randint(-4095, 4096, (n_rows, case.C), generator=g)
    cols = (torch.arange(case.C)[None, :] + torch.arange(n_rows)[:, None]) % 48 < 4
    f = torch.where(cols, wide, f)
    f[:, 0] = torch.where(torch.arange(n_rows) % 2 == 0, 4095, -4093)[:n_rows]
    if n_rows > 2:
        f[2] = 0
    t = torch.randint(-15, 16, (case.K, case.C), generator=g)
    if case.K >= 2:
        t[case.K // 2] = 0
    S = f.abs().double() @ t.abs().double().t()
    assert float(S.max()) * case.T < 2.0 ** 24, (case, float(S.max()))
    return Inputs(f.float(), t.float(), row_idx, valid, torch.zeros(n_rows, dtype=torch.int64), n_rows, EXACT_SCALE)


# ---------------------------------------------------------------------------------------------------------------
# references (float64)
# ---------------------------------------------------------------------------------------------------------------
def normalize64(feats):
    """F.normalize(p=2, dim=-1, eps=1e-12) in float64 from the fp32 input."""
    f = feats.double()
    return f / f.norm(dim=-1, keepdim=True).clamp(min=1e-12)


def logits64(feats, text, scale, normalize):
    """-> (logits [n_rows, K], S, F) in float64: one logit per feature row and class, and what its bound scales with."""
    f = normalize64(feats) if normalize else feats.double()
    t = text.double()
    fa, ta = f.abs(), t.abs()
    S = fa @ ta.t()
    Fq = fa.amax(-1)[:, None] * ta.sum(-1)[None] + fa.sum(-1)[:, None] * ta.amax(-1)[None]
    return scale * (f @ t.t()), S, Fq


def scatter(rows, row_idx):
    """[n_rows, K] -> [B, T, K] by row_idx; invalid views (-1) zero.  Any layout: compact, dense, permuted, shared rows."""
    B, T = row_idx.shape
    out = rows.new_zeros(B * T, rows.shape[-1])
    flat = row_idx.flatten().long()
    ok = flat >= 0
    out[ok] = rows[flat[ok]]
    return out.view(B, T, -1)


def aggregate64(full, valid, agg):
    """models/clip_cls.py:104-121 in float64: sum | sum / #valid (0 / 0 = NaN without a valid view) | max with -1e6 on
    the invalid views."""
    if agg == 'sum':
        return full.sum(1)
    if agg == 'mean':
        return full.sum(1) / valid.double().sum(1, keepdim=True)
    assert agg == 'max'
    return (full - (1.0 - valid.double())[..., None] * 1e6).max(1).values


def view_probs64(full):
    return torch.softmax(full.double(), -1)


def probs64(full, valid):
    """:123-129: per-view softmax, mask, mean over the valid views (NaN without one)."""
    vm = valid.double()
    return (view_probs64(full) * vm[..., None]).sum(1) / vm.sum(1, keepdim=True)


def classify64(feats, text, row_idx, scale, agg, normalize):
    """-> dict(full_logits [B, T, K], logits, probs [B, K], and S, F scattered like full_logits), float64."""
    rows, S, Fq = logits64(feats, text, scale, normalize)
    valid = row_idx >= 0
    full = scatter(rows, row_idx)
    return dict(full_logits=full, logits=aggregate64(full, valid, agg), probs=probs64(full, valid), valid=valid,
                S=scatter(S, row_idx), F=scatter(Fq, row_idx))


# ---------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic, restated (fixed summation order: the same bits everywhere)
# ---------------------------------------------------------------------------------------------------------------
def tree_sum32(x):
    """Sum over the last axis in fp32, halves added elementwise until one column is left."""
    assert x.dtype == F32
    n = 1
    while n < x.shape[-1]:
        n *= 2
    x = torch.nn.functional.pad(x, (0, n - x.shape[-1]))
    while n > 1:
        n //= 2
        x = x[..., :n] + x[..., n:]
    return x[..., 0]


def pow2_exponent(mx):
    """e = 10 - floor(log2(mx)) clamped to +-100 (mx 2^e in [2^10, 2^11)); 0 for a zero or non-finite maximum.  The
    floor is taken exactly (frexp); the kernel's floorf(log2f()) may say one more for a maximum one step below a power
    of two, which scales that row into [2^9, 2^10) and loses nothing."""
    ok = (mx > 0) & torch.isfinite(mx)
    ex = torch.frexp(torch.where(ok, mx, torch.ones_like(mx)))[1]       # mx = m 2^ex, m in [0.5, 1)
    e = (10 - (ex - 1)).clamp(-100, 100)
    return torch.where(ok, e, torch.zeros_like(e)).to(torch.int32)


def split16(v):
    hi = v.half()
    return hi, (v - hi.float()).half()


def _pad_cols(v, Cp, poison):
    pad = v.new_full((v.shape[0], Cp - v.shape[1]), float('nan') if poison else 0.0)
    return torch.cat([v, pad], -1)


def prep_rows32(feats, normalize, Cp, poison=False):
    """classify_prep_rows -> (hi, lo fp16 [n, Cp], inv_scale fp32 [n], d fp32 [n] the norm the rows were divided by)."""
    assert feats.dtype == F32
    mx = feats.abs().amax(-1)
    d = torch.ones_like(mx)
    if normalize:
        d = torch.sqrt(tree_sum32(feats * feats)).clamp(min=torch.tensor(1e-12, dtype=F32))
        mx = mx / d
    e = pow2_exponent(mx)
    sc = torch.ldexp(torch.ones_like(mx), e)
    v = ((feats / d[:, None]) if normalize else feats) * sc[:, None]
    hi, lo = split16(_pad_cols(v, Cp, poison))
    return hi, lo, torch.ldexp(torch.ones_like(mx), -e), d


def prep_text32(text, Cp, Kp, poison=False):
    """classify_prep_text -> (hi, lo fp16 [Kp, Cp], inv_class fp32 [Kp]); rows K .. Kp - 1 zero with scale 1."""
    assert text.dtype == F32
    K = text.shape[0]
    t = torch.cat([text, text.new_zeros(Kp - K, text.shape[1])])
    e = pow2_exponent(t.abs().amax(-1))
    hi, lo = split16(_pad_cols(torch.ldexp(t, e[:, None]), Cp, poison))
    return hi, lo, torch.ldexp(torch.ones(Kp), -e)


def _dot32(a, b):
    return tree_sum32(a.float()[:, None, :] * b.float()[None, :, :])


def _dot64(a, b):
    return a.double() @ b.double().t()


FAULTS = ('lo_dropped', 'neighbour_scale', 'pad_poison', 'pad_classes', 'no_max', 'mean_over_T', 'max_unmasked',
          'invalid_in_probs', 'norm_skipped', 'row_idx_compact')


def classify32(feats, text, row_idx, scale, agg, normalize, fault=None, parts=False):
    """ec_classify_v2 step by step in fp32 -> dict(full_logits, logits, probs) (+ the intermediates with parts=True).
    `fault` breaks one step on purpose (FAULTS); the CPU test shows that the bounds reject each."""
    assert fault is None or fault in FAULTS
    n_rows, C = feats.shape
    K = text.shape[0]
    B, T = row_idx.shape
    Cp, Kp = (C + 63) // 64 * 64, (K + 15) // 16 * 16
    poison = fault == 'pad_poison'
    a_hi, a_lo, inv, d = prep_rows32(feats, normalize and fault != 'norm_skipped', Cp, poison)
    w_hi, w_lo, invk = prep_text32(text, Cp, Kp, poison)
    hh, lh, hl = _dot32(a_hi, w_hi), _dot32(a_lo, w_hi), _dot32(a_hi, w_lo)
    raw = hh + hl if fault == 'lo_dropped' else (hh + lh) + hl                                  # [n_rows, Kp]
    flat = row_idx.flatten().long()
    ok = flat >= 0
    if fault == 'row_idx_compact':
        flat = torch.where(ok, torch.cumsum(ok.long(), 0) - 1, flat)
    rows = flat.clamp(min=0)
    s_mul = torch.tensor(scale, dtype=F32) * (inv.roll(-1) if fault == 'neighbour_scale' else inv)[rows]
    Ks = Kp if fault == 'pad_classes' else K
    fl = torch.where(ok[:, None], s_mul[:, None] * (invk[None, :Ks] * raw[rows, :Ks]), torch.zeros(1)).view(B, T, Ks)
    valid = ok.view(B, T)
    vmax = torch.zeros(B, T, 1) if fault == 'no_max' else fl.amax(-1, keepdim=True)
    ex = torch.exp((fl - vmax).double()).float()                 # expf: through float64, correctly rounded everywhere
    vp = (ex / tree_sum32(ex)[..., None])[..., :K]
    fl = fl[..., :K].contiguous()
    lsum, lmax, psum = torch.zeros(B, K), torch.full((B, K), float('-inf')), torch.zeros(B, K)
    in_probs = torch.ones_like(valid) if fault == 'invalid_in_probs' else valid
    for t in range(T):                                           # the views in order, as the kernel adds them
        lsum = lsum + fl[:, t]
        off = torch.zeros(B, 1) if fault == 'max_unmasked' else (~valid[:, t, None]).float() * 1e6
        lmax = torch.maximum(lmax, fl[:, t] - off)
        psum = torch.where(in_probs[:, t, None], psum + vp[:, t], psum)
    nv = valid.float().sum(1, keepdim=True)
    logits = {'sum': lsum, 'mean': lsum / (float(T) if fault == 'mean_over_T' else nv), 'max': lmax}[agg]
    out = dict(full_logits=fl, logits=logits, probs=psum / nv)
    if parts:
        out.update(view_probs=vp, a=(a_hi, a_lo, inv, d), w=(w_hi, w_lo, invk), raw=raw)
    return out


# ---------------------------------------------------------------------------------------------------------------
# bounds: float64 tensors of the reference's shape
# ---------------------------------------------------------------------------------------------------------------
def logit_bound(ref, S, Fq, scale, normalize, factor=KERNEL_FACTOR):
    n = 1.0 if normalize else 0.0
    prod = C_REP * (2.0 ** -22 * S + 2.0 ** -35 * Fq) + C_ACC * 2.0 ** -24 * S + n * 2.0 ** -24 * S
    return factor * (abs(scale) * prod + (n * C_NORM * EPS32 + 2.0 ** -24) * ref.abs())


def agg_bound(want, view_bound, agg, factor=KERNEL_FACTOR):
    """want: classify64's dict; view_bound: logit_bound of full_logits with the invalid views at 0."""
    full, valid = want['full_logits'], want['valid']
    T = full.shape[1]
    if agg == 'max':
        return view_bound.amax(1)
    b = view_bound.sum(1) + factor * T * 2.0 ** -24 * full.abs().sum(1)
    if agg == 'mean':
        nv = valid.double().sum(1, keepdim=True)
        b = b / nv + factor * 2.0 ** -24 * (full.sum(1) / nv).abs()
    return b


def view_prob_bound(full, view_bound, factor=KERNEL_FACTOR, c_sm=None):
    """[B, T, K]: how far each view's probabilities may be from softmax(full) (see the module's docstring)."""
    c_sm = C_SM if c_sm is None else c_sm
    full = full.double()
    logp = torch.log_softmax(full, -1)
    p = logp.exp()
    logq = torch.log(-torch.expm1(logp.clamp(max=-1e-300)))                  # log(1 - p); p == 1 -> -inf
    odds = logp - logq
    L2 = 2 * view_bound.amax(-1, keepdim=True)
    moved = torch.maximum(torch.sigmoid(odds + L2) - p, p - torch.sigmoid(odds - L2)).clamp(min=0)
    dist = (full - full.amax(-1, keepdim=True)).abs()
    return moved + factor * c_sm * EPS32 * (1 + dist) * p + FLOOR_PROB


def prob_bound(want, view_bound, factor=KERNEL_FACTOR):
    full, valid = want['full_logits'], want['valid']
    vm = valid.double()[..., None]
    nv = valid.double().sum(1, keepdim=True)
    vb = view_prob_bound(full, view_bound, factor)
    return (vb * vm).sum(1) / nv + factor * (full.shape[1] + 1) * 2.0 ** -24 * want['probs'].abs()


def bounds(want, scale, agg, normalize, factor=KERNEL_FACTOR):
    """-> dict(full_logits, logits, probs) of bounds for classify64's dict `want`."""
    vb = logit_bound(want['full_logits'], want['S'], want['F'], scale, normalize, factor)
    return dict(full_logits=vb, logits=agg_bound(want, vb, agg, factor), probs=prob_bound(want, vb, factor))


def excess(got, ref, bound):
    """Largest amount by which |got - ref| passes the bound (<= 0: within), as a float.  Where the reference is NaN (a
    sample without a valid view under mean, and its probabilities) the result must be NaN, and nowhere else: else inf."""
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), nan) or bool(torch.isinf(got).any()):
        return float('inf')
    if bool(nan.all()):
        return 0.0
    over = (got.double() - ref).abs() - bound
    return float(over[~nan].max())


def ulp32(x):
    """The spacing of fp32 at |x| (x fp32)."""
    a = x.abs()
    return torch.nextafter(a, torch.full_like(a, float('inf'))) - a


# ---------------------------------------------------------------------------------------------------------------
# ec_pseudo_label
# ---------------------------------------------------------------------------------------------------------------
PL_VIEWS = (1, 2, 3, 4, 5, 7, 8)
PL_KS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000)
PL_FLAGS = ((0, 0), (0, 1), (1, 0), (1, 1))                # (tta_consistent, tta_min_prob)
PL_THRESH = 0.5
PL_STEP = 2.0 ** -10
WINNERS = (0, 63, 64, 255, 256, -1)                        # -1: K - 1
TIES = ((63, 64), (255, 256), (0, -1), (44, 300))          # (44, 300): one thread, two trips


def thresholds():
    """The planted equality and one fp32 step below it."""
    t = torch.tensor(PL_THRESH, dtype=F32)
    return float(t), float(torch.nextafter(t, torch.zeros(())))


PlInputs = collections.namedtuple('PlInputs', 'probs tags')


@functools.lru_cache(maxsize=None)
def pl_inputs(V, K):
    """-> (probs fp32 [B, V, K], tags: one string per sample), read-only.  Every probability is a multiple of 2^-10
    (view sums are exact in fp32 and float64); background 0 .. 16/1024.  Samples:
      win@k     every view's top at k (0.75 + v 2^-10), for k in WINNERS that exist
      low@k     the same at 0.25: never selected at 0.5
      tie@i,j   classes i and j equal (0.75) in every view: the lower index wins, per view and in the mean
      eq_mean   every view's top exactly 0.5: not > 0.5, selected one step below
      eq_low    view v0's top exactly 0.5, the others 0.875 (one sample per position v0 = 0 and V - 1): the mean is
                clear of 0.5, the smallest view top is not
      dissent@v view v votes for another class (0.875 there, 0.625 on the sample's), one sample per view
      nan_all   every entry NaN (what the classifier returns for a sample without a valid view)
      nan_one@k one NaN, in the last view at class k (k = 0, K // 2 and K - 1), beside a clear finite winner
    (ties and dissent need K >= 2, dissent and eq_low V >= 2)."""
    g = _gen(6000 + 31 * V + K)
    rows, tags = [], []

    def sample(tag):
        rows.append(torch.randint(0, 17, (V, K), generator=g).double() * PL_STEP)
        tags.append(tag)
        return rows[-1]

    step = torch.arange(V).double() * PL_STEP
    for k in sorted({w % K for w in WINNERS if w < K}):
        sample(f'win@{k}')[:, k] = 0.75 + step
        sample(f'low@{k}')[:, k] = 0.25 + step
    for i, j in TIES:
        if i >= K or j >= K or i == j % K:
            continue
        j = j % K
        s = sample(f'tie@{i},{j}')
        s[:, i] = s[:, j] = 0.75
    c = 5 % K
    sample('eq_mean')[:, c] = PL_THRESH
    if V >= 2:
        for v0 in sorted({0, V - 1}):
            s = sample(f'eq_low@{v0}')
            s[:, c] = 0.875
            s[v0, c] = PL_THRESH
    if V >= 2 and K >= 2:
        for v in range(V):
            s = sample(f'dissent@{v}')
            s[:, c] = 0.75
            s[v, c], s[v, (c + 1) % K] = 0.625, 0.875
    sample('nan_all')[:] = float('nan')
    for k in sorted({0, K // 2, K - 1}):
        s = sample(f'nan_one@{k}')
        s[:, c] = 0.75
        s[V - 1, k] = float('nan')
    return PlInputs(torch.stack(rows).float(), tuple(tags))


def _max_first(x):
    """max over the last axis with torch.max's semantics made explicit: NaN is the maximum, the first of equals wins."""
    nan = torch.isnan(x)
    key = torch.where(nan, torch.full_like(x, float('inf')), x)
    top = key.amax(-1, keepdim=True)
    idx = (key == top).double().argmax(-1)                  # first position of the maximum
    return torch.gather(x, -1, idx[..., None])[..., 0], idx


def pseudo_label64(probs, thresh, consistent, min_prob):
    """gen_data.py:132-164 for any number of views, float64, torch's NaN semantics: probs [B, V, K] ->
    dict(mean [B, K], pred, max_prob, selected).  The flags count only with more than one view (:134-150)."""
    p = probs.double()
    V = p.shape[1]
    mean = p.sum(1) / V if V > 1 else p[:, 0]
    max_prob, pred = _max_first(mean)
    sel = max_prob > thresh
    if V > 1:
        top, arg = _max_first(p)
        if consistent:
            sel &= (arg == arg[:, :1]).all(1)
        if min_prob:
            low = torch.where(torch.isnan(top).any(1), torch.full_like(top[:, 0], float('nan')), top.amin(1))
            sel &= low > thresh
    return dict(mean=mean, pred=pred, max_prob=max_prob, selected=sel)


PL_FAULTS = ('tie_high', 'ge', 'first_256', 'wave_0', 'mean_over_8', 'flags_at_v1')


def pseudo_label32(probs, thresh, consistent, min_prob, fault=None):
    """The kernel's arithmetic: the views added in order in fp32, x fl(1 / V); a maximum in which NaN wins and ties go to
    the lower index.  `fault` breaks one step (PL_FAULTS)."""
    assert fault is None or fault in PL_FAULTS
    p = probs.float()
    B, V, K = p.shape
    s = torch.zeros(B, K)
    for v in range(V):
        s = s + p[:, v]
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(8 if fault == 'mean_over_8' else V), dtype=F32)
    mean = s if V == 1 else s * inv
    k = torch.arange(K)
    seen = (k < 256) if fault == 'first_256' else (k % 256 < 64) if fault == 'wave_0' else torch.ones(K, dtype=torch.bool)

    def best(x):
        x = torch.where(seen, x, torch.full_like(x, float('-inf')))
        if fault == 'tie_high':
            v, i = _max_first(x.flip(-1))
            return v, K - 1 - i
        return _max_first(x)

    max_prob, pred = best(mean)
    t = torch.tensor(thresh, dtype=F32)
    sel = (max_prob >= t) if fault == 'ge' else (max_prob > t)
    if V > 1 or fault == 'flags_at_v1':
        top, arg = best(p)
        if consistent:
            sel &= (arg == arg[:, :1]).all(1)
        if min_prob:
            low = torch.where(torch.isnan(top), torch.full_like(top, float('inf')), top).amin(1)      # fminf
            sel &= (low >= t) if fault == 'ge' else (low > t)
    return dict(mean=mean, pred=pred, max_prob=max_prob, selected=sel)


def pl_same(got, want, V):
    """What the GPU test asks of ec_pseudo_label's outputs `got` (mean, max_prob fp32; pred; selected) against
    pseudo_label64's `want`: pred and selected equal on EVERY sample, mean and max_prob bit-equal to the float64 result
    cast to fp32 for V a power of two and within one ulp otherwise, NaN exactly where the reference has NaN."""
    if not (torch.equal(got['pred'], want['pred']) and torch.equal(got['selected'], want['selected'])):
        return False
    for k in ('mean', 'max_prob'):
        w32 = want[k].float()
        if not torch.equal(torch.isnan(got[k]), torch.isnan(w32)):
            return False
        ok = ~torch.isnan(w32)
        tol = 0 if V & (V - 1) == 0 else ulp32(w32[ok])
        if bool(((got[k][ok] - w32[ok]).abs() > tol).any()):
            return False
    return True
