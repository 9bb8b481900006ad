"""Float64 yardsticks, dispatch predicates and directed inputs for the attention kernels (csrc/attention.hip).

Nothing here touches a GPU or anything compiled: the references are plain torch float64 (they run on whatever device
their input lives on), the predicates restate the host code's dispatch as data, and the generators build their
tensors on the CPU from a seed.

Layout as the kernels see it: qkv is [n_seq * S, 3 W], q | k | v, a head is a 64-wide column block of each third.
Scores are kept in log2 units throughout: s = c <q, k> with c = log2(e) / sqrt(64), so softmax = 2^s / sum 2^s and
the kernels' log-sum-exp is log2 sum 2^s.
"""
import functools
import math

import torch

LOG2E = 1.4426950408889634
C = 0.125 * LOG2E                                  # log2(e) / sqrt(64)
C32 = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))   # the kernels' fp32 c

QM_RAW, QM_KERNEL, QM_INPUT = 0, 1, 2              # attention.hip: where c enters the scores
ATTN_THR, ATTN_LO, ATTN_PART = 10.0, 4.0, 66
LDS = 160 * 1024


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def heads_of(x, n_seq, S, heads):
    """[n_seq * S, 3 W] -> q, k, v as [n_seq, heads, S, 64] (same dtype)."""
    return x.view(n_seq, S, 3, heads, 64).permute(2, 0, 3, 1, 4)


def _softmax_v(s, v, n_seq, S, heads, causal, q_rows, round_p=None, round_out=None):
    """s [n_seq, heads, S, S] in log2 units (float64) -> out [n_seq * q_rows, W], lse [n_seq, heads, q_rows]."""
    q_rows = S if q_rows is None else q_rows
    s = s[:, :, :q_rows]
    if causal:
        s = s + torch.full((S, S), float('-inf'), dtype=s.dtype, device=s.device).triu_(1)[:q_rows]
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    if round_p is not None:
        p = round_p(p)
    l = p.sum(-1, keepdim=True)
    out = (p @ v) / l
    if round_out is not None:
        out = round_out(out)
    return out.permute(0, 2, 1, 3).reshape(n_seq * q_rows, heads * 64), (m + torch.log2(l)).squeeze(-1)


def exact(qkv, n_seq, S, heads, causal=0, q_rows=None, prescaled=0):
    """softmax(q k^T / 8) v and log2 sum 2^s in float64, of the already-rounded values the kernel reads (for the split
    entry points: the joined hi + lo planes).  prescaled: the q columns hold c q."""
    q, k, v = heads_of(qkv.double(), n_seq, S, heads)
    s = (q @ k.transpose(-1, -2)) * (1.0 if prescaled else C)
    return _softmax_v(s, v, n_seq, S, heads, causal, q_rows)


def emulated(qkv, n_seq, S, heads, causal=0, q_rows=None, prescaled=0, dtype=torch.float16, qmode=None):
    """The same with the 16-bit kernel's three rounding points, everything else in float64: c q rounded to the operand
    type (QM_KERNEL only; QM_RAW scales the fp32 scores, QM_INPUT reads c q), P rounded to the operand type, the output
    rounded.  The maximum is the row's true one: where the kernel's running maximum stands is not modelled."""
    if qmode is None:
        qmode = QM_INPUT if prescaled else (QM_KERNEL if dtype == torch.float16 else QM_RAW)
    assert qkv.dtype == dtype and (qmode == QM_INPUT) == bool(prescaled)
    q, k, v = heads_of(qkv, n_seq, S, heads)
    if qmode == QM_KERNEL:
        q = (q.float() * C32).to(dtype)
    s = q.double() @ k.double().transpose(-1, -2)
    if qmode == QM_RAW:
        s = s * C32
    rnd = lambda x: x.to(dtype).double()
    return _softmax_v(s, v.double(), n_seq, S, heads, causal, q_rows, round_p=rnd, round_out=rnd)


def emulated_f32(qkv, n_seq, S, heads, causal=0, prescaled=0):
    """The split-precision kernels' arithmetic class: fp32 scores, exponentials, sums and output (the yardstick that
    says whether a directed input is within reach of an fp32 kernel at all).  Output only."""
    q, k, v = heads_of(qkv.double().float(), n_seq, S, heads)
    s = (q * (1.0 if prescaled else 0.125)) @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((S, S), float('-inf'), device=s.device).triu_(1)
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m) if prescaled else torch.exp(s - m)
    out = (p @ v) / p.sum(-1, keepdim=True)
    return out.permute(0, 2, 1, 3).reshape(n_seq * S, heads * 64).double()


def step_maxima(qkv, n_seq, S, heads, causal=0, prescaled=0):
    """[n_seq, heads, S, ceil(S / 32)] float64: the maximum visible score (log2 units) of every query in every 32-key
    step; -inf where the step holds no visible key."""
    q, k, _ = heads_of(qkv.double(), n_seq, S, heads)
    s = (q @ k.transpose(-1, -2)) * (1.0 if prescaled else C)
    if causal:
        s = s + torch.full((S, S), float('-inf'), dtype=s.dtype).triu_(1)
    n32 = (S + 31) // 32
    s = torch.nn.functional.pad(s, (0, 32 * n32 - S), value=float('-inf'))
    return s.view(n_seq, heads, S, n32, 32).amax(-1)


# ---------------------------------------------------------------------------------------------------------------
# dispatch, as attention.hip's host code decides it
# ---------------------------------------------------------------------------------------------------------------
def waves(S):
    """Waves per workgroup of attention_kernel: 16 once K + V and the merge area pass 80 KiB (S >= 289)."""
    kv = 32 * ((S + 31) // 32) * 128 * 2
    return 16 if kv + 16 * ATTN_PART * 4 > 80 * 1024 else 8


def lone(S, causal, n_waves):
    """attn_lone_tile: the last query tile holds one row and is left over after whole rounds of the waves."""
    tiles = (S + 15) // 16
    return (not causal) and (S & 15) == 1 and tiles > n_waves and tiles % n_waves == 1


def supported(S, causal=0):
    kv = 32 * ((S + 31) // 32) * 128 * 2
    return kv + (16 * ATTN_PART * 4 if lone(S, causal, waves(S)) else 0) <= LDS


def tail_kind(S):
    """What lies behind the last full 32-key step: 'none', 'odd' (one key: the rank-one update) or 'masked'."""
    return ('none', 'odd')[S & 31] if (S & 31) < 2 else 'masked'


def keyless_waves(S, n_waves):
    """Waves that get no key of a lone tile."""
    steps = S >> 5
    return [w for w in range(n_waves) if w * steps // n_waves == (w + 1) * steps // n_waves and w != n_waves - 1]


def hl_path(S, prescaled, dtype):
    """ec_attention_split -> ('hl', None, None) | ('hl2', split, sl) | ('f32m', None, None)."""
    sp = 32 * ((S + 31) // 32)
    plain16 = dtype == torch.float16 and not prescaled
    if plain16 and 4 * sp * 128 + (8 * ATTN_PART * 4 if lone(S, 0, 8) else 0) <= LDS:
        return 'hl', None, None
    split = (S // 2) & ~31
    sl = S - split
    spl = ((sl + 30) // 16) * 16 if (sl & 31) == 1 else ((sl + 31) // 32) * 32
    if plain16 and split >= 32 and 4 * spl * 128 <= LDS and (S + 15) // 16 <= 8 * 5:
        return 'hl2', split, sl
    return 'f32m', None, None


def block_variants(S, causal, n_waves):
    """The (KSTEPS, MASK) variants of attn_block2 / 'odd' that are some tile's FIRST contribution at this length: the
    ones whose `down` arm an all-low input takes."""
    first = set()
    if causal:
        sp = 32 * ((S + 31) // 32)
        for qt in range((S + 15) // 16):
            kend = min(sp, ((qt * 16 + 16 + 31) // 32) * 32)
            kfree = min(qt * 16 + 1, kend)
            first.add((2, False) if 64 <= kfree else (2, True) if 64 <= kend else (1, True))
        return first

    def keys(s0, s1, tail):
        if s1 - s0 >= 2:
            return (2, False)
        if s1 - s0 == 1:
            return (1, False)
        return {'none': None, 'odd': 'odd', 'masked': (1, True)}[tail_kind(S)] if tail else None
    first.add(keys(0, S >> 5, True))
    if lone(S, causal, n_waves):
        steps = S >> 5
        for w in range(n_waves):
            first.add(keys(w * steps // n_waves, (w + 1) * steps // n_waves, w == n_waves - 1))
    first.discard(None)
    return first


# ---------------------------------------------------------------------------------------------------------------
# inputs: q, k, v as float64 [n_seq, S, heads, 64] (a PLAIN q), seeded, built on the CPU
# ---------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def gaussian(S, n_seq=2, heads=2, seed=0, sigma=1.5):
    g = _gen(1000 + 7 * S + seed)
    return tuple(_randn(g, n_seq, S, heads, 64) * sigma for _ in range(3))


def all_low(S, level, n_seq=2, heads=2, seed=0):
    """Every score of every query near -level log2 units: q = a u + noise, k = -a u + noise, u a vector of +-1 per head
    (8 a^2 log2(e) = level).  The noise (0.3 on both) leaves the softmax spread over many keys."""
    g = _gen(2000 + 7 * S + seed)
    a = math.sqrt(level / (8 * LOG2E))
    u = torch.sign(_randn(g, 1, 1, heads, 64))
    q = a * u + 0.3 * _randn(g, n_seq, S, heads, 64)
    k = -a * u + 0.3 * _randn(g, n_seq, S, heads, 64)
    return q, k, _randn(g, n_seq, S, heads, 64) * 1.5


def spike_plan(S):
    """Default (key, rows) lists: three keys with the last key of the sequence among them; the rows of key i are every
    3 (i + 1)-th from 1, the key's own row and the next (for a causal mask: on and just below the diagonal), and for the
    last key the last row."""
    keys = sorted({S // 3, (2 * S) // 3, S - 1})
    plan = []
    for i, key in enumerate(keys):
        rows = set(range(1, S, 3 * (i + 1))) | {key, min(key + 1, S - 1)}
        if key == S - 1:
            rows.add(S - 1)
        plan.append((key, sorted(rows)))
    return plan


def spike(S, plan=None, gain=1.0, n_seq=2, heads=2, seed=0):
    """tests/test_towers_gpu.py test_attention_running_maximum_moves' construction with explicit keys and rows: key i
    is gain (4 + 3 i) d_i and its rows get q / 4 + 2 d_i (d_i of +-1, at most six), so they score 16 gain (4 + 3 i) natural units
    there, each spike larger than the one before."""
    g = _gen(3000 + 7 * S + seed)
    q, k, v = (_randn(g, n_seq, S, heads, 64) for _ in range(3))
    plan = spike_plan(S) if plan is None else plan
    listed = sorted({r for _, rows in plan for r in rows})
    q[:, listed] *= 0.25
    base = torch.sign(_randn(g, 64))
    for i, (key, rows) in enumerate(plan):
        d = base * (1 - 2 * ((torch.arange(64) >> i) & 1)).double()      # mutually orthogonal: no cross terms between the keys
        k[:, key] = d * (4.0 + 3 * i) * gain
        q[:, rows] += d * 2.0          # a row of several lists lines up with each of their keys
    return q, k, v


def staggered_rows(S):
    return [r for r in range(S) if r % 3 or r == S - 1]


def staggered(S, rise=2.0, period=None, noise=1.0, n_seq=2, heads=2, seed=0):
    """The key maxima of consecutive 32-key steps differ by more than ATTN_THR, rising over the first half of the
    steps and falling over the second (the odd key of S = 32 n + 1 continues the fall): k = noise + h(step) u, and the
    rows of staggered_rows get q = u + noise / 2 (so they score 8 rise log2(e) more or less per step).  In a tile whose
    keys are split over the waves every wave ends on a maximum of its own.  With a period the levels repeat (period = 2:
    0, rise, 0, rise ..), which bounds the largest score whatever the length."""
    g = _gen(4000 + 7 * S + seed)
    q, k, v = (_randn(g, n_seq, S, heads, 64) for _ in range(3))
    q, k = q * noise, k * noise
    u = torch.sign(_randn(g, 1, 1, heads, 64))
    n = (S + 31) // 32
    step = torch.arange(S) // 32
    if period:
        step, n = step % period, period + 1
    h = rise * torch.minimum(step, (n - 1) - step).double()
    k = k + h[None, :, None, None] * u
    rows = staggered_rows(S)
    q[:, rows] = u + 0.5 * q[:, rows]
    return q, k, v


def pack(qkv3, dtype, prescaled=0):
    """q, k, v -> the [n_seq * S, 3 W] tensor of `dtype` a kernel reads (prescaled: c q in the q columns, rounded once)."""
    q, k, v = qkv3
    n_seq, S, heads, _ = q.shape
    W = heads * 64
    q = q * C if prescaled else q
    return torch.cat([x.reshape(n_seq * S, W) for x in (q, k, v)], 1).float().to(dtype)


def pack_split(qkv3, dtype, prescaled=0):
    """-> hi, lo planes of `dtype` (what ec_attention_split reads: both parts in the operand type) and their float64 sum."""
    x = pack(qkv3, torch.float32, prescaled)
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    return hi, lo, hi.double() + lo.double()


# ---------------------------------------------------------------------------------------------------------------
# the shape tables and magnitudes the CPU and GPU tests share
# ---------------------------------------------------------------------------------------------------------------
S_16BIT = (1, 2, 16, 17, 31, 32, 33, 64, 65, 96, 129, 145, 257, 273, 288, 289, 320, 321, 513, 529, 577, 608, 640)
S_DIRECTED = (1, 33, 64, 129, 257, 289, 513, 577)
S_LONE = (129, 257, 513)
S_ROWS = (129, 257, 513)
S_SPLIT = (1, 33, 64, 65, 129, 257, 288, 289, 300, 320, 353, 577, 600, 608, 609)
S_SPLIT_BF16 = (65, 129, 289, 609)
S_SPLIT_DIRECTED = (129, 257, 300, 577, 600, 609)      # 600: attention_hl2_kernel with a masked tail (300 fits one pass)


def rows_cases(S):
    return (1, 15, 16, 17, S - 1, S)


def low_level(dtype, prescaled):
    """Depth of all_low in log2 units.  f16 with a plain q (QM_KERNEL) rounds c q a second time, so its score error grows
    with |score|: -36 there, where an f16 P without the move is already 0; bf16's P only underflows far lower (2^-133),
    and neither a pre-scaled q nor QM_RAW adds error with depth: -300."""
    return 36.0 if dtype == torch.float16 and not prescaled else 300.0


# The fp32-class kernels carry about 2^-24 of the LARGEST score into every score, so their directed inputs stay near
# the Gaussian ones' range (tests/test_attention_ref_cpu.py test_split_inputs_are_within_reach_of_fp32): all_low at -12
# (an f16 hi + lo P without the move would keep 13 bits there), spikes of 46 .. 115, and the staggered steps alternate
# between two levels 17 apart (every second step moves nothing, neighbouring waves of a split tile still differ).
SPLIT_LOW, SPLIT_GAIN, SPLIT_STAGGER = 12.0, 0.5, dict(rise=1.5, period=2, noise=0.5)

TOL = {torch.float16: 4e-3, torch.bfloat16: 2.5e-2}    # tests/test_towers_gpu.py test_attention
TOL_SPIKED_BF16 = 4e-2                                 # ... test_attention_running_maximum_moves
LSE_RTOL, LSE_ATOL = 2e-3, 2e-2                        # ... test_attention_lse_matches_reference (f16)
# max |emulated - exact| of the bf16 log-sum-exp over every input of the train cases, rounded up (test_attention_ref_cpu.py
# measures it: 1.86e-3)
BF16_LSE_EMULATION_ERR = 1.9e-3
SPLIT_BOUND = {torch.float16: 4e-6, torch.bfloat16: 4e-5}


def out_tol(dtype, kind):
    return TOL_SPIKED_BF16 if dtype == torch.bfloat16 and kind == 'spike' else TOL[dtype]


def make(kind, S, dtype=torch.float16, prescaled=0, split=False, n_seq=2, heads=2):
    """The q, k, v of a named input at the magnitude its consumer (16-bit kernel of dtype / q mode, or split kernels) takes."""
    if kind == 'gaussian':
        return gaussian(S, n_seq, heads, sigma=1.7 if split else 1.5)
    if kind == 'all_low':
        return all_low(S, SPLIT_LOW if split else low_level(dtype, prescaled), n_seq, heads)
    if kind == 'spike':
        # QM_KERNEL's second rounding of q again: half the existing test's magnitudes keep the yardstick's own error
        # within half the tolerance there
        half = split or (dtype == torch.float16 and not prescaled)
        return spike(S, None, SPLIT_GAIN if half else 1.0, n_seq, heads)
    if kind == 'staggered':
        return staggered(S, n_seq=n_seq, heads=heads, **(SPLIT_STAGGER if split else {}))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case16(kind, S, dtype, prescaled, causal):
    """(qkv of dtype on the CPU, exact out, exact lse), computed once and shared; treat as read-only."""
    qkv = pack(make(kind, S, dtype, prescaled), dtype, prescaled)
    out, lse = exact(qkv, 2, S, 2, causal, None, prescaled)
    return qkv, out, lse


@functools.lru_cache(maxsize=None)
def case_split(kind, S, dtype, prescaled):
    """(hi, lo planes on the CPU, exact out of the joined planes)."""
    hi, lo, joined = pack_split(make(kind, S, dtype, prescaled, split=True), dtype, prescaled)
    return hi, lo, exact(joined, 2, S, 2, 0, None, prescaled)[0]


@functools.lru_cache(maxsize=None)
def case_f32(kind, S, causal):
    """(fp32 qkv on the CPU, exact out): ec_attention_f32 reads fp32 and a plain q."""
    qkv = pack(make(kind, S, split=True), torch.float32)
    return qkv, exact(qkv, 2, S, 2, causal)[0]
