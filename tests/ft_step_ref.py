"""Float64 yardsticks, per-element bounds, directed inputs, shape tables and checks for the kernels of csrc/vit_train.hip
that turn a gradient into a weight update: ec_adam_step_multi, ec_grad_unscale_check, ec_lora_merge_batched /
ec_lora_grad_batched, ec_pack_weight16_batched and the public ec_layernorm_backward (with the two reduction kernels behind
it).

Nothing here touches a GPU or anything compiled.  Every operation is written once, from its definition, over an arithmetic
(fewshot_ref.A64: torch float64, the yardstick; fewshot_ref.A32: every product rounded, sums in index order, the fp32
restatement).  tests/test_ft_step_ref_cpu.py confirms the float64 forms against torch's own, holds the restatement to every
bound over the whole tables, and runs every check against an fp32 model with one planted fault;
tests/test_ft_step_edges_gpu.py holds the kernels to the same checks.

A ``check_<family>(impl, case, what)`` takes the implementation under test as a callable on a ``call``: a dict of CPU
tensors and of the scalar arguments as the entry point takes them.  ``impl(call)`` returns ``(outputs, refusal)``: every
buffer the entry point could have written, read back whole (guards included), and the RuntimeError the entry point raised
(None when it ran).  It never changes the call's own tensors.

Bounds are per element, derived, with no floor term, and no element is left out:
* sums and products: vit_train_ref.gamma(k) sum |terms|, k the number of terms that meet in the element.  Every addition
  rounds once relative to a partial sum no larger than the sum of the magnitudes, whatever the order (slabs, waves, LDS);
* Adam: fewshot_ref.adam_S and its constant C['adam'], as ec_adam_step is held (the kernel states the same formula);
* unscale, pack and every skip path are exact: bit for bit, NaN by isnan;
* LayerNorm backward: vit_train_ref.ln_backward plus the term its bound leaves out, the rounding of x - mean (``ln_bound``).

Buffers.  An fp32 output is a flat tensor [GUARD x G | data | GUARD x G]; the data starts as NaN where the entry point
must overwrite it.  G = 8 words keeps the data 16-byte aligned for the kernels' float4 accesses."""
import math

import numpy as np
import torch

import fewshot_ref as fr
import vit_train_ref as vr
from fewshot_ref import A32, A64, F32, F64, f32  # noqa: F401

G = 8
GUARD = -9876543.0            # exact in fp32
GUARD16 = 0x5A5A              # the fill of a 16-bit output buffer, guards and data alike
PADV = 24681357.0 / 8         # what the padding columns of a strided output hold
NAN = float('nan')
# the device step scalars (include/eventclip_hip.h: EC_STEP_*; the GPU test asserts they are the header's)
STEP_LR0, STEP_LR1, STEP_BC1, STEP_BC2_SQRT, STEP_GRAD_SCALE, STEP_INV_SCALE, STEP_COUNT = 0, 1, 2, 3, 4, 5, 8


# ---------------------------------------------------------------------------------------------------------------
# buffers and comparisons
# ---------------------------------------------------------------------------------------------------------------
def guarded(data):
    g = torch.full((G,), GUARD, dtype=F32)
    return torch.cat([g, data.reshape(-1).to(F32), g])


def nan_buf(n):
    return guarded(torch.full((int(n),), NAN))


def body(buf, *shape):
    return buf[G:G + math.prod(shape)].view(*shape)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_or_nan(got, want):
    """Bit for bit; where ``want`` is NaN any NaN will do."""
    nan = torch.isnan(want)
    return got.shape == want.shape and torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])


def guards_back(buf, n, what):
    assert buf.numel() == n + 2 * G, f'{what}: buffer of {buf.numel()} words for {n}'
    g = torch.full((G,), GUARD, dtype=F32)
    assert same_bits(buf[:G], g), f'{what}: wrote before the buffer'
    assert same_bits(buf[G + n:], g), f'{what}: wrote past the end'


def untouched(buf, orig, what):
    assert same_or_nan(buf, orig), f'{what}: was written'


def held(got, ref, bd, what):
    """Assert |got - ref| <= bd element by element (bd = 0: the element is exact) -> the worst error / bound."""
    got = torch.as_tensor(got)
    if not got.numel():
        return 0.0
    assert torch.isfinite(got).all(), f'{what}: not finite'
    err = (got.double() - ref).abs()
    bd = torch.as_tensor(bd, dtype=F64).expand_as(err)
    ratio = torch.where(bd > 0, err / bd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = float(ratio.max())
    assert r <= 1, f'{what}: error / bound = {r:.3f} at element {int(ratio.argmax())} of {tuple(got.shape)}'
    return r


def ran(ret, what):
    out, refusal = ret
    assert refusal is None, f'{what}: refused: {refusal}'
    return out


def refused(ret, entry, what):
    out, refusal = ret
    assert isinstance(refusal, RuntimeError), f'{what}: not refused'
    assert entry in str(refusal), f'{what}: the error does not name {entry}: {refusal}'
    return out


def axis_shapes(axes, small, large):
    """Every value of each axis against one small and one larger value of the others (fewshot_ref.gemm_shapes)."""
    s = []
    for a, values in enumerate(axes):
        for x in values:
            for other in (small, large):
                s.append(tuple(x if i == a else other[i] for i in range(len(axes))))
    return list(dict.fromkeys(s))


# ---------------------------------------------------------------------------------------------------------------
# Adam over a tensor list
# ---------------------------------------------------------------------------------------------------------------
ADAM_TRIP = 512 * 256                 # elements one trip of the capped grid covers
# (n, group): the small tensors sit beside the large ones, so most workgroups of their blockIdx.y are idle
ADAM_LIST = ((ADAM_TRIP + 77, 1), (0, 0), (1, 1), (ADAM_TRIP - 1, 0), (255, 0), (256, 1), (ADAM_TRIP, 1), (257, 0),
             (ADAM_TRIP + 1, 0))
ADAM_LR = (2e-3, 5e-4)
ADAM_BETAS = (0.9, 0.98)
# (step, wd, eps, directed); the directed inputs hold elements with g = m = v = 0, which stand still only without decay
ADAM_CASES = ((1, 0.0, 1e-8, False), (2, 0.02, 1e-3, False), (1000, 0.02, 1e-8, False), (1000, 0.0, 1e-3, False),
              (1, 0.02, 1e-8, False), (2, 0.0, 1e-8, False), (1, 0.0, 1e-8, True), (2, 0.0, 1e-3, True), (1000, 0.0, 1e-8, True))


def bias_corrections(b1, b2, step):
    """The two fp32 values the kernel receives, as ec_adam_step_multi's host code computes them from `step`."""
    return f32(1.0 - f32(b1) ** step), f32(math.sqrt(1.0 - f32(b2) ** step))


def adam_step(ar, p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s):
    """torch.optim.Adam's step with the bias corrections handed in -> (p, m, v)."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    t = ar.t
    gi = g + t(wd) * p if wd != 0 else g
    mn = m * t(b1) + t(1 - b1) * gi
    vn = v * t(b2) + t(1 - b2) * gi * gi
    pn = p - t(lr) / t(bc1) * mn / (ar.sqrt(vn) / t(bc2s) + t(eps))
    return pn, mn, vn


def adam_call(case):
    step, wd, eps, directed = case
    items = []
    for n, group in ADAM_LIST:
        p, g, m, v = fr.adam_inputs(n, directed)
        items.append(dict(p=guarded(p), g=guarded(g), m=guarded(m), v=guarded(v), n=n, group=group))
    return dict(items=items, n_items=len(items), max_n=max(n for n, _ in ADAM_LIST), lr0=ADAM_LR[0], lr1=ADAM_LR[1],
                b1=ADAM_BETAS[0], b2=ADAM_BETAS[1], eps=eps, wd=wd, step=step, skip=None, scalars=None)


def _adam_same(out, want, names, what):
    for i, (o, w) in enumerate(zip(out, want)):
        for k in names:
            assert same_bits(o[k], w[k]), f'{what}: tensor {i} ({k}) differs'


def check_adam_list(impl, case, what, variants=True):
    """impl(call) -> [{p, g, m, v}: the guarded buffers after the launch].  The by-value form under the bound with guards
    on both sides of every buffer; the device-scalars form with poisoned by-value arguments gives the same bits; a raised
    skip flag, no items or max_n = 0 leave everything as it was.  -> worst error / bound."""
    step, wd, eps, directed = case
    call = adam_call(case)
    b1, b2 = call['b1'], call['b2']
    bc1, bc2s = bias_corrections(b1, b2, step)
    out = ran(impl(call), what)
    worst = 0.0
    for i, (it, o) in enumerate(zip(call['items'], out)):
        n, lr = it['n'], ADAM_LR[it['group']]
        p, g, m, v = (body(it[k], n) for k in 'pgmv')
        want = adam_step(A64, p.double(), g.double(), m.double(), v.double(), lr, b1, b2, eps, wd, bc1, bc2s)
        _, S = fr.adam_S(p, g, m, v, step, lr, b1, b2, eps, wd)
        for k, w, s in zip('pmv', want, S):
            guards_back(o[k], n, f'{what} {case} tensor {i} ({k})')
            worst = max(worst, held(body(o[k], n), w, fr.KERNEL_FACTOR * fr.C['adam'] * fr.EPS24 * s, f'{what} {case} tensor {i} n={n}: {k}'))
        assert same_bits(o['g'], it['g']), f'{what}: tensor {i}: the gradient changed'
        if directed and n:
            still = (g == 0) & (m == 0) & (v == 0)
            assert still.any() and same_bits(body(o['p'], n)[still], p[still]), f'{what}: an element with g = m = v = 0 moved'
            assert not bool(body(o['m'], n)[still].any()) and not bool(body(o['v'], n)[still].any())
    # the scalars form wins over whatever the by-value arguments hold
    sc = [0.0] * STEP_COUNT
    sc[STEP_LR0], sc[STEP_LR1], sc[STEP_BC1], sc[STEP_BC2_SQRT] = f32(ADAM_LR[0]), f32(ADAM_LR[1]), bc1, bc2s
    _adam_same(ran(impl(dict(call, lr0=NAN, lr1=NAN, step=0, scalars=sc)), what), out, 'pgmv', f'{what} {case}: scalars form')
    if variants:
        for flag in (1, -1):
            _adam_same(ran(impl(dict(call, skip=flag)), what), call['items'], 'pgmv', f'{what} {case}: skip flag {flag}')
        _adam_same(ran(impl(dict(call, skip=0)), what), out, 'pgmv', f'{what} {case}: skip flag 0')
        _adam_same(ran(impl(dict(call, n_items=0)), what), call['items'], 'pgmv', f'{what} {case}: n_items = 0')
        _adam_same(ran(impl(dict(call, max_n=0)), what), call['items'], 'pgmv', f'{what} {case}: max_n = 0')
    return worst


# ---------------------------------------------------------------------------------------------------------------
# unscale and check
# ---------------------------------------------------------------------------------------------------------------
UNSCALE_TRIP = 2048 * 256
UNSCALE_N = (1, 63, 64, 65, 255, 256, 257, UNSCALE_TRIP - 1, UNSCALE_TRIP, UNSCALE_TRIP + 1)
UNSCALE_INV = (1.0, 2.0 ** -16, f32(1.0 / 3.0))
# element 0, the last element of the first wave, the first of the second workgroup, the first of the second grid trip
# (and element n - 1, added per n)
PLANT_AT = (0, 63, 256, UNSCALE_TRIP)
PLANTS = (math.inf, -math.inf, NAN)


def unscale_data(n):
    """Gaussians over six decades; every 7th element near 2^-118 (times 2^-16: an fp32 subnormal), every 7th near 2^-126
    (times 1/3: a subnormal), every 11th an fp32 subnormal itself."""
    g_ = fr._gen(77 + n)
    i = torch.arange(n)
    x = fr._randn(g_, n) * 10.0 ** (torch.rand(n, generator=g_, dtype=F64) * 6 - 3)
    u = 1 + torch.rand(n, generator=g_, dtype=F64)
    x = torch.where(i % 7 == 3, 2.0 ** -118 * u, x)
    x = torch.where(i % 7 == 5, -(2.0 ** -126) * u, x)
    x = torch.where(i % 11 == 7, 2.0 ** -140 * u, x)
    return x.float()


def unscale_product(x, inv):
    """The IEEE fp32 product, subnormal results included (numpy: no flush to zero)."""
    with np.errstate(all='ignore'):
        return torch.from_numpy(x.numpy() * np.float32(inv))


def check_unscale(impl, n, what):
    """impl(call) -> (buffer, flag).  Every product bit for bit; the flag is left alone on finite data (whether it was
    0 or 1) and raised by one non-finite element wherever it sits, by an overflow of the product, not by a finite value
    that the scale brings back; the scalars form wins over a poisoned by-value scale.  -> number of launches."""
    x = unscale_data(n)
    count = 0

    def one(data, inv, flag0, want_flag, tag, scalars=None, by_value=None):
        nonlocal count
        call = dict(buf=guarded(data), n=n, inv_scale=inv if by_value is None else by_value, flag=flag0, scalars=scalars)
        buf, flag = ran(impl(call), what)
        count += 1
        guards_back(buf, n, f'{what} n={n} {tag}')
        assert same_or_nan(body(buf, n), unscale_product(data, inv)), f'{what} n={n} {tag}: the products differ'
        assert flag == want_flag, f'{what} n={n} {tag}: flag {flag0} -> {flag}, expected {want_flag}'

    for inv in UNSCALE_INV:
        for flag0 in (0, 1):
            one(x, inv, flag0, flag0, f'clean inv={inv}')
    at = list(dict.fromkeys([p for p in PLANT_AT if p < n] + [n - 1]))
    k = 0
    for pos in at:
        for val in PLANTS:
            d = x.clone()
            d[pos] = val
            one(d, UNSCALE_INV[k % 3], 0, 1, f'{val} at {pos}')
            k += 1
    d = x.clone()
    d[n - 1] = 3e38
    one(d, 2.0, 0, 1, '3e38 * 2')
    one(d, 2.0 ** -16, 0, 0, '3e38 * 2^-16')
    sc = [0.0] * STEP_COUNT
    sc[STEP_INV_SCALE] = UNSCALE_INV[2]
    one(x, UNSCALE_INV[2], 0, 0, 'scalars form', scalars=sc, by_value=NAN)
    return count


# ---------------------------------------------------------------------------------------------------------------
# LoRA: merge, d up, d down
# ---------------------------------------------------------------------------------------------------------------
LORA_ROWS = (1, 3, 4, 5, 15, 16, 17, 31, 33, 200)
LORA_COLS = (4, 252, 256, 260, 1024, 1028)
LORA_R = (1, 7, 8, 9, 15, 16, 17, 63, 64)
LORA_KINDS = ('random', 'cancel', 'one_factor', 'one_row')


def lora_cases():
    """(rows, cols, r, n_items, kind)"""
    cs = [s + ((1, 3)[i % 2], 'random') for i, s in enumerate(axis_shapes((LORA_ROWS, LORA_COLS, LORA_R), (3, 8, 2), (33, 260, 17)))]
    for kind in LORA_KINDS[1:]:
        cs += [(17, 260, 9, 1, kind), (33, 1028, 17, 3, kind)]
    return cs


def lora_call(case):
    rows, cols, r, n_items, kind = case
    items = []
    for i in range(n_items):
        g_ = fr._gen(5000 + 7919 * i + 131 * rows + 17 * cols + r)
        base = fr._randn(g_, rows, cols).float()
        up = (fr._randn(g_, rows, r) * 0.5).float()
        down = (fr._randn(g_, r, cols) * 2.0).float()
        dW = (fr._randn(g_, rows, cols) * 0.25 * (i + 1)).float()
        if kind == 'cancel':           # base = -up down in float64, rounded: held to the bound, not to zero
            sel = torch.arange(rows) % 3 == (rows - 1) % 3
            base[sel] = (-(up.double() @ down.double())).float()[sel]
        elif kind == 'one_factor':     # only the last factor acts
            up[:, :r - 1] = 0
        elif kind == 'one_row':        # only the last row of dW
            dW[:rows - 1] = 0
        items.append(dict(base=base, up=up, down=down, dW=dW, out=nan_buf(rows * cols), d_up=nan_buf(rows * r),
                          d_down=nan_buf(r * cols)))
    return dict(items=items, rows=rows, cols=cols, r=r, n_items=n_items, null_table=False)


def lora_merge(ar, base, up, down):
    return ar.mm(up, down) + base


def lora_dup(ar, dW, down):
    return ar.mm(dW, down.transpose(-1, -2))


def lora_ddown(ar, up, dW):
    return ar.mm(up.transpose(-1, -2), dW)


def check_lora(impl, case, what):
    """impl(op, call), op 'merge' | 'grad' -> [{out, d_up, d_down}: guarded buffers].  -> {part: worst error / bound}"""
    rows, cols, r, n_items, kind = case
    call = lora_call(case)
    worst = dict(merge=0.0, d_up=0.0, d_down=0.0)
    merged, grads = ran(impl('merge', call), what), ran(impl('grad', call), what)
    for i, it in enumerate(call['items']):
        b, u, d, w = (it[k].double() for k in ('base', 'up', 'down', 'dW'))
        tag = f'{what} {case} item {i}'
        for k, n in (('out', rows * cols), ('d_up', rows * r), ('d_down', r * cols)):
            guards_back(merged[i][k], n, f'{tag} merge: {k}')
            guards_back(grads[i][k], n, f'{tag} grad: {k}')
        for k in ('d_up', 'd_down'):
            untouched(merged[i][k], it[k], f'{tag} merge: {k}')
        untouched(grads[i]['out'], it['out'], f'{tag} grad: out')
        worst['merge'] = max(worst['merge'], held(body(merged[i]['out'], rows, cols), lora_merge(A64, b, u, d),
                                                  vr.gamma(r + 1) * (b.abs() + u.abs() @ d.abs()), f'{tag}: out'))
        worst['d_up'] = max(worst['d_up'], held(body(grads[i]['d_up'], rows, r), lora_dup(A64, w, d),
                                                vr.gamma(cols) * (w.abs() @ d.abs().T), f'{tag}: d_up'))
        worst['d_down'] = max(worst['d_down'], held(body(grads[i]['d_down'], r, cols), lora_ddown(A64, u, w),
                                                    vr.gamma(rows) * (u.abs().T @ w.abs()), f'{tag}: d_down'))
    return worst


def check_lora_refusals(impl, what):
    """cols % 4 != 0, r = 0, r = 65, no items, a null table: a RuntimeError that names the entry point, nothing written."""
    n = 0
    for rows, cols, r, n_items, null in ((5, 6, 3, 1, False), (5, 8, 0, 1, False), (5, 8, 65, 1, False), (5, 8, 3, 0, False),
                                         (5, 8, 3, 1, True)):
        call = lora_call((rows, cols, max(r, 1), max(n_items, 1), 'random'))
        call.update(r=r, n_items=n_items, null_table=null)
        for op, entry in (('merge', 'ec_lora_merge_batched'), ('grad', 'ec_lora_grad_batched')):
            tag = f'{what} {op} rows={rows} cols={cols} r={r} n_items={n_items} null={null}'
            out = refused(impl(op, call), entry, tag)
            for o, it in zip(out, call['items']):
                for k in ('out', 'd_up', 'd_down'):
                    untouched(o[k], it[k], f'{tag}: {k}')
            n += 1
    return n


# ---------------------------------------------------------------------------------------------------------------
# pack: fp32 -> hi, lo, hi transposed (16 bit).  IEEE round to nearest even with subnormals is the definition:
# hi = rne16(v), lo = rne16(v - float(hi)) with the fp32 difference -- so a value whose hi is +inf has lo = -inf
# (v - inf), one whose hi is -inf has lo = +inf, and +-inf itself has lo = NaN.
# ---------------------------------------------------------------------------------------------------------------
PACK_AXIS = (1, 63, 64, 65, 129)
PACK_DTYPES = (torch.float16, torch.bfloat16)
SUBSETS = ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 0))    # hi, lo, hi_t
PACK_LAUNCHES = ((0, 1, 2), (3, 4, 5), (6, 7, 0))      # three same-shape items per launch, their subsets


def pack_shapes():
    return axis_shapes((PACK_AXIS, PACK_AXIS), (3, 3), (65, 65))


def pack_cases():
    """(rows, cols, dtype, launch)"""
    return [(rows, cols, dt, l) for dt in PACK_DTYPES for rows, cols in pack_shapes() for l in range(len(PACK_LAUNCHES))]


def rne16(v, dtype):
    """np.float32 array -> uint16 bit patterns, IEEE round to nearest even (NaN -> a NaN)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dtype == torch.float16:
        with np.errstate(all='ignore'):
            return v.astype(np.float16).view(np.uint16)
    b = v.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)     # the integer rule on the 32-bit word
    r[np.isnan(v)] = 0x7FC0
    return r


def decode16(b, dtype):
    """uint16 bit patterns -> np.float32"""
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if dtype == torch.float16:
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def pack_reference(w, dtype):
    """fp32 tensor [rows, cols] -> (hi, lo, hi_t) uint16 arrays"""
    v = w.numpy()
    hi = rne16(v, dtype)
    with np.errstate(all='ignore'):
        lo = rne16(v - decode16(hi, dtype), dtype)
    return hi, lo, np.ascontiguousarray(hi.T)


def directed_values(dtype):
    """fp32 values on and beside every rounding edge of the 16-bit format: exact ties whose lower neighbour is even and
    odd; the largest finite value, the point that rounds to infinity and its fp32 neighbours; the subnormal range with
    the tie to zero and the value just above it; zeros, fp32 subnormals, infinities, NaN.  Both signs."""
    mant = 10 if dtype == torch.float16 else 7
    one = (15 if dtype == torch.float16 else 127) << mant                 # the pattern of 1.0 (even)
    top = (0x7C00 if dtype == torch.float16 else 0x7F80) - 1              # the largest finite value
    minnorm = 1 << mant
    dec = lambda h: float(decode16(np.array([h], dtype=np.uint16), dtype)[0])       # noqa: E731
    vals = []
    for h in (one, one + 1, one + 2, one + 0x55, one - 1, 0, 1, 2, 3, 4, minnorm - 2, minnorm - 1, minnorm, minnorm + 1, top - 1):
        a, b = dec(h), dec(h + 1)
        mid = np.float32((a + b) / 2)
        assert float(mid) == (a + b) / 2            # the tie is an fp32 value
        vals += [mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)), np.float32(a)]
    over = np.float32(dec(top) + (dec(top) - dec(top - 1)) / 2)     # the tie between the largest finite value and 2^(emax + 1)
    vals += [np.float32(dec(top)), over, np.nextafter(over, np.float32(0)), np.nextafter(over, np.float32(np.inf))]
    vals += [np.float32(0), np.float32(1e-40), np.float32(2.0 ** -149), np.float32(np.inf)]
    vals = np.array(vals, dtype=np.float32)
    return np.concatenate([vals, -vals, np.array([np.nan], dtype=np.float32)])


def pack_matrix(rows, cols, dtype, seed, directed):
    """Gaussians over 1e-3 .. 1e3; directed: the directed values first (as many as fit), then Gaussians in the format's
    subnormal range, near 2^-130 and ordinary ones in turn."""
    n = rows * cols
    g_ = fr._gen(seed)
    x = (fr._randn(g_, n) * 10.0 ** (torch.rand(n, generator=g_, dtype=F64) * 6 - 3)).float()
    if directed:
        i = torch.arange(n)
        z = fr._randn(g_, n)
        x = torch.where(i % 3 == 0, (z * 2.0 ** -17).float(), x)       # float16's subnormal range
        x = torch.where(i % 3 == 1, (z * 2.0 ** -130).float(), x)      # bfloat16's (fp32 subnormals)
        d = torch.from_numpy(directed_values(dtype))
        x[:min(n, d.numel())] = d[:n]
        if n < d.numel():                # a small matrix takes the window of the directed list its seed picks
            start = (seed * 7) % (d.numel() - n)
            x = d[start:start + n].clone()
    return x.view(rows, cols)


def pack_call(case):
    rows, cols, dtype, launch = case
    ws, present, bufs = [], [], []
    for j, s in enumerate(PACK_LAUNCHES[launch]):
        seed = 3 * (rows * 131 + cols) + j + 1000 * launch
        ws.append(pack_matrix(rows, cols, dtype, seed, directed=(j + launch) % 2 == 0))
        present.append(SUBSETS[s])
        bufs.append({k: torch.full((rows * cols + 2 * G,), GUARD16, dtype=torch.int16) for k in ('hi', 'lo', 'hi_t')})
    return dict(ws=ws, present=present, bufs=bufs, rows=rows, cols=cols, dtype=dtype)


def check_pack(impl, case, what):
    """impl(call) -> [{hi, lo, hi_t}: int16 buffers, the would-be buffers of absent outputs included].  Bit for bit,
    NaN by isnan; an absent output's buffer and every guard still hold the fill.  -> elements compared"""
    rows, cols, dtype, launch = case
    call = pack_call(case)
    out = ran(impl(call), what)
    n, count = rows * cols, 0
    for j, (w, pres, o) in enumerate(zip(call['ws'], call['present'], out)):
        ref = pack_reference(w, dtype)
        for k, on, want in zip(('hi', 'lo', 'hi_t'), pres, ref):
            tag = f'{what} {case} item {j}: {k}'
            got = o[k].numpy().view(np.uint16)
            assert got.shape == (n + 2 * G,), tag
            assert (got[:G] == GUARD16).all() and (got[G + n:] == GUARD16).all(), f'{tag}: wrote outside the matrix'
            if not on:
                assert (got == GUARD16).all(), f'{tag}: an absent output was written'
                continue
            got, want = got[G:G + n], want.reshape(-1)
            gv, wv = decode16(got, dtype), decode16(want, dtype)
            nan = np.isnan(wv)
            bad = np.where(nan, ~np.isnan(gv), got != want)
            assert not bad.any(), (f'{tag}: {int(bad.sum())} elements differ, the first at {int(bad.argmax())}: got '
                                   f'{int(got[bad.argmax()]):#06x}, expected {int(want[bad.argmax()]):#06x}')
            count += n
    return count


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm backward, the public entry
# ---------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (4, 8, 252, 256, 260, 1024, 2044, 2048)          # at rows 1 and 5
LN_ROWS = (3, 4, 252, 253, 256, 257, 260, 4096, 4097, 4101)   # at width 256: 63 / 64 / 65 workgroups, the 1024 cap
LN_OUTS = ('adjacent', 'separate', 'gamma', 'beta', 'none')
LN_PADS = ((0, 0, 0), (4, 0, 0), (0, 8, 0), (0, 0, 12), (8, 4, 16))     # ldx, ldy, ldo beyond the width
LN_KINDS = ('gauss', 'offset', 'directed', 'gamma0')


def ln_cases():
    """(rows, width, (pad x, pad dy, pad dx), accumulate, outs, kind, index)"""
    cs = []

    def add(rows, width, acc, outs):
        i = len(cs)
        cs.append((rows, width, LN_PADS[i % 5], acc, outs, LN_KINDS[(i // 2 + i // 7) % 4], i))
    for j, width in enumerate(LN_WIDTHS):
        for k, rows in enumerate((1, 5)):
            for acc in (0, 1):
                add(rows, width, acc, LN_OUTS[(4 * j + 2 * k + acc) % 5])
    for j, rows in enumerate(LN_ROWS):     # both reduction launches (one over 2 W, two over W) at every partial count
        add(rows, 256, 0, 'adjacent')
        add(rows, 256, 1, 'separate')
        add(rows, 256, j % 2, LN_OUTS[2 + j % 3])
    return cs


def ln_rows(ar, x, dy, gamma_w, dx0=None, mean_over=None):
    """-> (dx [+ dx0], d gamma, d beta) from the saved input: statistics recomputed, sums in the arithmetic's order."""
    W = mean_over or x.shape[-1]
    mean = ar.sum(x) / W
    xc = x - mean[..., None]
    var = ar.sum(xc * xc) / W
    rstd = 1 / ar.sqrt(var + (vr.LN_EPS if ar.exact else ar.c(vr.LN_EPS)))
    xh = xc * rstd[..., None]
    g = dy * gamma_w
    s1, s2 = ar.sum(g) / W, ar.sum(g * xh) / W
    dx = rstd[..., None] * (g - s1[..., None] - xh * s2[..., None])
    return (dx if dx0 is None else dx0 + dx), ar.sum(dy * xh, 0), ar.sum(dy, 0)


def ln_bound(x, dy, gamma_w, dx0=None):
    """vit_train_ref.ln_backward's values and bounds (exact fp32 inputs, float64 here) with the term that bound leaves
    out: x - mean is rounded, and the mean it subtracts is a rounded sum of W terms,
        d xc <= gamma(W) mean|x| + 2^-24 (|x| + mean|x|),
    which moves the variance by 2 mean(|xc| d xc) + mean(d xc^2) (the square matters on a constant row, where xc = 0),
    rstd by rstd^3 / 2 of that and x hat by rstd d xc + (|xc| + d xc) d rstd; dx and d gamma take x hat's error to first
    order through every place x hat and rstd enter.  An accumulated dx rounds once more."""
    (dx, e_dx), (dg, e_dg), (db, e_db) = vr.ln_backward(x, dy, None, gamma_w)
    W = x.shape[-1]
    mabs = x.abs().mean(-1, keepdim=True)
    xc = x - x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + vr.LN_EPS)
    xh = xc * rstd
    d_xc = vr.gamma(W) * mabs + vr.U32 * (x.abs() + mabs)
    d_var = 2 * (xc.abs() * d_xc).mean(-1, keepdim=True) + (d_xc ** 2).mean(-1, keepdim=True)
    d_rstd = 0.5 * rstd ** 3 * d_var
    d_xh = rstd * d_xc + (xc.abs() + d_xc) * d_rstd
    g = dy * gamma_w
    m1, m2 = g.mean(-1, keepdim=True).abs(), (g * xh).mean(-1, keepdim=True).abs()
    d_m2 = (g.abs() * d_xh).mean(-1, keepdim=True)
    xw = xh.abs() + d_xh
    e_dx = e_dx + rstd * (d_xh * m2 + xw * d_m2) + d_rstd * (g.abs() + m1 + xw * (m2 + d_m2))
    e_dg = e_dg + (dy.abs() * d_xh).sum(0)
    if dx0 is not None:
        e_dx = e_dx + vr.U32 * (dx0.abs() + dx.abs() + e_dx)
        dx = dx0 + dx
    return (dx, e_dx), (dg, e_dg), (db, e_db)


def ln_call(case):
    rows, width, (px, py, po), acc, outs, kind, idx = case
    g_ = fr._gen(900 + 13 * idx)
    x = fr._randn(g_, rows, width) * 1.5 + 0.3
    dy = fr._randn(g_, rows, width) * 0.5
    gam = 1 + 0.2 * fr._randn(g_, width)
    if kind == 'offset':
        x = 8 + fr._randn(g_, rows, width)
    if kind == 'gamma0':
        gam[::3] = 0
        gam[width - 1] = 0
    x, dy, gam = x.float(), dy.float(), gam.float()
    if kind == 'directed':
        # by (row + idx) % 4: 0 a constant row (variance 0, rstd = 1 / sqrt(eps)); 1 dy = 0; 2 dy = 0.7 xhat / gamma, so
        # that g is proportional to x hat and dx cancels; 3 an ordinary row
        t = (torch.arange(rows) + idx) % 4
        x[t == 0] = 1.7
        dy[t == 1] = 0
        xd = x.double()
        xc = xd - xd.mean(-1, keepdim=True)
        xh = xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + vr.LN_EPS)
        dy[t == 2] = (0.7 * xh / gam.double()).float()[t == 2]
    dx0 = fr._randn(g_, rows, width).float() if acc else torch.full((rows, width), NAN)

    def strided(t, pad, fill):
        b = torch.full((rows, width + pad), fill, dtype=F32)
        b[:, :width] = t
        return b
    n_g = 2 * width if outs == 'adjacent' else width
    return dict(x=guarded(strided(x, px, NAN)), dy=guarded(strided(dy, py, NAN)), gamma=guarded(gam),
                dx=guarded(strided(dx0, po, PADV)), dg=nan_buf(n_g), db=nan_buf(width), rows=rows, width=width,
                ldx=width + px, ldy=width + py, ldo=width + po, accumulate=acc, eps=1e-5, outs=outs, no_partials=outs == 'none')


def ln_view(call, key, ld):
    return body(call[key], call['rows'], ld)[:, :call['width']]


def check_ln(impl, case, what):
    """impl(call) -> {dx, dg, db}: guarded buffers.  outs: 'adjacent' d gamma | d beta side by side in ``dg`` (one
    reduction launch), 'separate' in ``dg`` and ``db``, 'gamma' / 'beta' only one, 'none' neither and no partials; a
    buffer not asked for comes back as it was.  -> worst error / bound"""
    rows, width, pads, acc, outs, kind, idx = case
    call = ln_call(case)
    o = ran(impl(call), what)
    tag = f'{what} {case}'
    x, dy, dx0 = (ln_view(call, k, call[ld]) for k, ld in (('x', 'ldx'), ('dy', 'ldy'), ('dx', 'ldo')))
    gam = body(call['gamma'], width)
    (dx, e_dx), (dg, e_dg), (db, e_db) = ln_bound(x.double(), dy.double(), gam.double(), dx0.double() if acc else None)
    ldo = call['ldo']
    guards_back(o['dx'], rows * ldo, f'{tag}: dx')
    got = body(o['dx'], rows, ldo)
    assert same_bits(got[:, width:], body(call['dx'], rows, ldo)[:, width:]), f'{tag}: dx wrote into the row padding'
    worst = held(got[:, :width], dx, e_dx, f'{tag}: dx')
    zero = (dy == 0).all(-1)
    if zero.any():       # dy = 0: nothing is added, exactly
        want = dx0[zero] if acc else torch.zeros_like(dx0[zero])
        assert torch.equal(got[:, :width][zero], want), f'{tag}: dx of a row with dy = 0'
    n_g = 2 * width if outs == 'adjacent' else width
    guards_back(o['dg'], n_g, f'{tag}: d gamma')
    guards_back(o['db'], width, f'{tag}: d beta')
    got_g = body(o['dg'], n_g)[:width] if outs in ('adjacent', 'separate', 'gamma') else None
    got_b = body(o['dg'], n_g)[width:] if outs == 'adjacent' else body(o['db'], width) if outs in ('separate', 'beta') else None
    if got_g is None:
        untouched(o['dg'], call['dg'], f'{tag}: d gamma, not asked for')
    else:
        worst = max(worst, held(got_g, dg, e_dg, f'{tag}: d gamma'))
    if outs not in ('separate', 'beta'):
        untouched(o['db'], call['db'], f'{tag}: the separate d beta, not asked for')
    if got_b is not None:
        worst = max(worst, held(got_b, db, e_db, f'{tag}: d beta'))
    return worst


def check_ln_refusals(impl, what):
    """width 6, width 2052, a stride that is no multiple of 4 (each of the three), d gamma without the partials scratch,
    eps != 1e-5: a RuntimeError that names the entry point, nothing written."""
    base = (5, 8, (0, 0, 0), 1, 'separate', 'gauss', 0)
    variants = [dict(case=(5, 6, (2, 2, 2), 1, 'separate', 'gauss', 0)), dict(case=(5, 2052, (0, 0, 0), 1, 'separate', 'gauss', 0)),
                dict(case=(5, 8, (2, 0, 0), 1, 'separate', 'gauss', 0)), dict(case=(5, 8, (0, 2, 0), 1, 'separate', 'gauss', 0)),
                dict(case=(5, 8, (0, 0, 2), 1, 'separate', 'gauss', 0)), dict(case=base, no_partials=True), dict(case=base, eps=1e-4)]
    for v in variants:
        call = ln_call(v.pop('case'))
        call.update(v)
        tag = f"{what} width={call['width']} ld=({call['ldx']}, {call['ldy']}, {call['ldo']}) {v}"
        o = refused(impl(call), 'ec_layernorm_backward', tag)
        for k in ('dx', 'dg', 'db'):
            untouched(o[k], call[k], f'{tag}: {k}')
    return len(variants)
