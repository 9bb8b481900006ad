"""The kernels of csrc/resnet.hip, element by element, against float64 arithmetic on the exact 16-bit operands.

Every output is allocated with guard rows after its valid region, filled with one byte pattern (0x5A), and the guards
must come back unchanged: an overrunning tail store overwrites them instead of faulting.

Convolutions run at every (ks, Cin, Cout, H) class the five towers launch, taken from OpenAI's module tree
(resnet_ref.conv_classes, a meta-device walk) with the epilogue the tower uses there, plus the attention pool's
projections and an edge matrix (partial tiles, Cout % 128 = 64, H != W, 1 x 1 images under a 3x3 kernel, no scale,
no images).  The attention pool, the stem rows and the 2x2 pooling run at the towers' shapes and at the edges of
their APIs.  The references never use the project's kernels or MIOpen: im2col and float64 matmuls in torch."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref  # noqa: E402

from eventclip_amd import resnet  # noqa: E402

pytestmark = pytest.mark.gpu

# dtype name -> (torch dtype, EC dtype code, u: unit roundoff of a 16-bit store)
DT = {'f16': (torch.float16, 0, 2.0 ** -11), 'bf16': (torch.bfloat16, 1, 2.0 ** -8)}
U32 = 2.0 ** -24                # unit roundoff of fp32
FLOOR = 2.0 ** -25              # half the f16 subnormal step
GUARD = 0x5A                    # the guard byte
ARCHS = list(resnet.RESNET_ARCHS)


def _lib():
    from eventclip_amd import _lib as lib
    return lib


def _call(fn, *args):
    lib = _lib()
    rc = getattr(lib.lib(), fn)(*args, lib.stream_ptr())
    lib.check(rc, fn)


def _guarded(shape, dtype, guard_rows=128):
    """(view, whole): a tensor of ``shape`` at the front of an allocation ``guard_rows`` rows (of shape[-1]) longer,
    every byte of it GUARD."""
    n = math.prod(shape)
    whole = torch.empty(n + guard_rows * shape[-1], dtype=dtype, device='cuda')
    whole.view(torch.uint8).fill_(GUARD)
    return whole[:n].view(shape), whole


def _assert_guard(whole, n_valid, what=''):
    g = whole[n_valid:].view(torch.uint8)
    bad = int((g != GUARD).sum())
    assert bad == 0, f'{what}: {bad} guard bytes overwritten'


def _assert_within(got, ref, bound, what=''):
    """Element by element |got - ref| <= bound (NaN fails); reports the worst element."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        ratio = torch.where(ok, torch.zeros_like(err), (err / bound).nan_to_num(float('inf')))
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f'{what}: {int((~ok).sum())} of {err.numel()} elements outside the bound; worst at {idx}: '
                             f'got {float(got.flatten()[i]):.8g} want {float(ref.flatten()[i]):.8g} '
                             f'err {float(err.flatten()[i]):.3g} bound {float(bound.flatten()[i]):.3g}')


# ---- ec_resnet_conv ----
def _im2col64(x, ks):
    """x [n, H, W, Cin] -> float64 [n*H*W, ks*ks*Cin] in the kernel's tap-major K order, zero padding (ks-1)/2."""
    n, H, W, cin = x.shape
    x = x.double()
    if ks == 1:
        return x.reshape(-1, cin)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.stack([xp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], 3).reshape(-1, 9 * cin)


def _check_conv(got, x, w, scale, bias, resid, relu, out32, u, what):
    """got [M, Cout] against y64, the convolution in float64 on the exact 16-bit x and w with the epilogue in float64.

    The kernel multiplies 16-bit operands exactly (11 x 11 or 8 x 8 significand bits fit fp32) and sums them in the
    MFMA's fp32 accumulator: one rounding per 32-product MFMA step, K / 32 steps in sequence, then at most four more
    in the epilogue (acc * scale, + bias, + residual).  Each rounding is relative to a partial sum no larger than
    m64 = conv(|x|, |w|) |scale| + |bias| + |resid|, so before the store |v - y64| <= gamma m64 with
    gamma = (K / 32 + 4) 2^-24.  ReLU is 1-Lipschitz.  The store rounds v to 16 bit (u = 2^-11 f16, 2^-8 bf16; 0 for
    an fp32 store): |got - v| <= u |v| <= u (|y64| + gamma m64), and a subnormal f16 result adds at most half its
    step.  Together: |got - y64| <= u |y64| + (1 + u) gamma m64 + 2^-25."""
    cout, ks = w.shape[0], w.shape[1]
    A = _im2col64(x, ks)
    Wm = w.double().reshape(cout, -1)
    y, m = A @ Wm.t(), A.abs() @ Wm.abs().t()
    del A
    if scale is not None:
        y, m = y * scale.double(), m * scale.double().abs()
    y, m = y + bias.double(), m + bias.double().abs()
    if resid is not None:
        r = resid.double().reshape(-1, cout)
        y, m = y + r, m + r.abs()
    if relu:
        y = y.clamp_min(0)
    gamma = (Wm.shape[1] / 32 + 4) * U32
    uu = 0.0 if out32 else u
    _assert_within(got.reshape(-1, cout), y, uu * y.abs() + (1 + uu) * gamma * m + FLOOR, what)


def _conv_case(dt, ks, n, H, W, cin, cout, *, scale=True, resid=False, relu=True, out32=False, seed=0, what=''):
    td, code, u = DT[dt]
    g = torch.Generator(device='cuda').manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, device='cuda') * std
    x = rn(n, H, W, cin).to(td)
    w = rn(cout, ks, ks, cin, std=(ks * ks * cin) ** -0.5).to(td)
    sc = 1 + rn(cout, std=0.2) if scale else None                        # the BatchNorm scale of the epilogue
    b = rn(cout, std=0.1)
    r = rn(n, H, W, cout).to(td) if resid else None
    M = n * H * W
    out, whole = _guarded((max(M, 1), cout), torch.float32 if out32 else td)
    lib = _lib()
    _call('ec_resnet_conv', lib.ptr(x), n, H, W, cin, cout, ks, lib.ptr(w), lib.ptr(sc), lib.ptr(b), lib.ptr(r),
          int(relu), lib.ptr(out), int(out32), code)
    torch.cuda.synchronize()
    if M == 0:
        _assert_guard(whole, 0, what)          # wrote nothing
        return
    _assert_guard(whole, M * cout, what)
    _check_conv(out, x, w, sc, b, r, relu, out32, u, what)


# role -> epilogue as ec_resnet_encode runs it: BatchNorm scale + bias (+ residual) (+ ReLU); the attention pool's
# projections carry no scale (q, kv: 16-bit store; c_proj: fp32 store)
EPILOGUE = {'relu': dict(), 'resid': dict(resid=True), 'ds': dict(relu=False),
            'q': dict(scale=False, relu=False), 'kv': dict(scale=False, relu=False),
            'c': dict(scale=False, relu=False, out32=True)}


def _n_img(H, W):
    """Images per conv case: one at large H, three at small; more while n H W fills whole 128-row tiles (where any
    count can leave a partial one)."""
    n = 1 if H >= 28 else 3
    while (n * H * W) % 128 == 0 and (H * W) % 128 != 0:
        n += 1
    return n


def _tower_conv_cases():
    classes, projs = {}, set()
    for arch in ARCHS:
        c, p = resnet_ref.conv_classes(resnet.resnet_config(arch))
        for k, v in c.items():
            classes.setdefault(k, set()).update(v)
        projs.update(p)
    cases = []
    for (ks, cin, cout, H), roles in sorted(classes.items()):
        for role in sorted(roles):
            cases.append(pytest.param(role, ks, _n_img(H, H), H, H, cin, cout,
                                      id=f'{role}-{ks}x{ks}-{cin}-{cout}-H{H}'))
    for role, C, cout, L in sorted(projs):
        n = 5 if role != 'kv' else 3                 # kv: n * L token rows (a 1x1 image each)
        cases.append(pytest.param(role, 1, n * L if role == 'kv' else n, 1, 1, C, cout,
                                  id=f'{role}-{C}-{cout}-L{L}'))
    return cases


TOWER_CONVS = _tower_conv_cases()


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('role,ks,n,H,W,cin,cout', TOWER_CONVS)
def test_conv_tower_shapes(dt, role, ks, n, H, W, cin, cout):
    _conv_case(dt, ks, n, H, W, cin, cout, seed=ks * 7 + cin + 3 * cout + H, what=f'{dt} {role}',
               **EPILOGUE[role])


# (ks, n, H, W, Cin, Cout, epilogue): M % 128 in {1, 64, 127}; Cout % 128 = 64; H != W under a 3x3 kernel; a 1 x 1
# image under a 3x3 kernel (every tap but the centre is padding); no BatchNorm scale; no images at all
EDGES = [
    (1, 1, 1, 129, 64, 128, dict()),                        # M = 129: one row in the last tile
    (3, 1, 8, 8, 64, 128, dict(resid=True)),                # M = 64: half a tile
    (3, 1, 1, 127, 128, 64, dict(relu=False)),              # M = 127, a 1-row image, Cout = 64
    (1, 3, 5, 17, 128, 192, dict(out32=True, scale=False)),  # M = 255, Cout % 128 = 64, fp32 store
    (3, 2, 7, 12, 64, 192, dict()),                         # H != W, Cout % 128 = 64
    (3, 1, 12, 7, 192, 320, dict(resid=True)),
    (3, 1, 1, 130, 64, 64, dict(resid=True)),               # 1 x 130
    (3, 1, 130, 1, 128, 64, dict()),                        # 130 x 1
    (3, 5, 1, 1, 256, 192, dict()),                         # H = W = 1: only the centre tap is inside
    (3, 3, 1, 1, 64, 64, dict(resid=True, relu=False)),
    (3, 2, 9, 9, 128, 128, dict(scale=False)),              # scale = NULL under a 3x3 kernel
    (1, 2, 9, 9, 128, 320, dict(scale=False, relu=False, out32=True)),
    (1, 0, 7, 7, 64, 128, dict()),                          # no images: EC_OK, nothing written
    (3, 0, 7, 7, 64, 128, dict(out32=True, scale=False)),
]


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('i', range(len(EDGES)))
def test_conv_edges(dt, i):
    ks, n, H, W, cin, cout, epi = EDGES[i]
    _conv_case(dt, ks, n, H, W, cin, cout, seed=100 + i, what=f'{dt} edge {EDGES[i]}', **epi)


# ---- ec_resnet_attnpool_attend ----
def _attend_ref(q, kv, n, L, C):
    """-> (out64, budget, vmax), each [n, C]: the attention in float64 on the exact operands; eps max_t |v_t|, the
    error budget of the kernel's fp32 arithmetic, eps for each (image, head) as below; and max_t |v_t|.

    Scores: q * 0.125 is exact, each product of two 16-bit values is exact in fp32, and the 64 sums round:
    |ds_t| <= 64 2^-24 S_t with S_t = sum |q_j k_tj| / 8.  The weight e_t = __expf(s_t - max) carries the score
    errors of t and of the max key, the rounding of the difference x = s_t - max (|x| 2^-24), the multiply by log2 e
    inside __expf (|x| 2^-24, and as much again for log2 e itself) and v_exp_f32 (2^-23): a relative error
    d_t <= 64 2^-24 (S_t + S_max) + (3 |x| + 4) 2^-24.  A relative error d_t in each weight moves the normalised
    output by at most 2 sum_t p_t d_t max|v|.  Then sum_t e_t v_t sums L products in sequence (L + 1 roundings of
    terms no larger than e_t max|v|), the denominator sums ceil(L / 64) terms a lane and 6 butterfly steps, and the
    division rounds once: (L + ceil(L / 64) + 8) 2^-24 max|v|.  So

        eps = 2 sum_t p_t d_t + (L + ceil(L / 64) + 8) 2^-24.

    eps exceeds 1e-5 from L = 160 on (the sequential value sum alone is L 2^-24), and where ordinary scores make
    S_t large; a flat score row (q = 0) leaves only the second term."""
    Hh = C // 64
    qh = q.double().reshape(n, Hh, 64) * 0.125
    k = kv[..., :C].double().reshape(n, L, Hh, 64)
    v = kv[..., C:].double().reshape(n, L, Hh, 64)
    s = torch.einsum('nhd,nlhd->nhl', qh, k)
    S = torch.einsum('nhd,nlhd->nhl', qh.abs(), k.abs())
    p = torch.softmax(s, -1)
    out = torch.einsum('nhl,nlhd->nhd', p, v).reshape(n, C)
    smax, imax = s.max(-1, keepdim=True)
    d = 64 * U32 * (S + S.gather(-1, imax)) + (3 * (s - smax).abs() + 4) * U32
    eps = 2 * (p * d).sum(-1) + (L + math.ceil(L / 64) + 8) * U32
    vmax = v.abs().amax(1)                                               # [n, heads, 64]
    return out, (eps[..., None] * vmax).reshape(n, C), vmax.reshape(n, C)


ATTEND = [(2048, 50), (2560, 82), (3072, 145), (4096, 197)] + [(64, L) for L in (1, 2, 63, 64, 65, 128, 129, 255, 256)]


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('C,L', ATTEND)
def test_attnpool_attend(dt, C, L):
    """Three score regimes: q = 0 (the output is the plain mean of v), ordinary scores, and peaked scores with a gap
    of 30 between one key (the first, a middle or the last) and the rest.  Bound: u |ref| + (1 + u) eps max|v| +
    2^-25 with eps of _attend_ref."""
    td, code, u = DT[dt]
    n = 3 if C == 64 else 2
    g = torch.Generator(device='cuda').manual_seed(C + L)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g, device='cuda') * std
    cases = [('flat', torch.zeros(n, C, device='cuda'), rn(n, L, 2 * C)),
             ('ordinary', rn(n, C, std=2.0), rn(n, L, 2 * C))]
    for b in sorted({0, L // 2, L - 1}):
        q = torch.where(rn(n, C) < 0, -1.0, 1.0)
        kv = torch.cat([rn(n, L, C, std=0.1), rn(n, L, C)], -1)
        # the best key: 3.75 sign(q) in every head, so its score is 0.125 * 3.75 * 64 = 30; the others' are ~N(0, 0.1)
        kv[:, b, :C] = 3.75 * q
        cases.append((f'peaked@{b}', q, kv))
    for name, q, kv in cases:
        q, kv = q.to(td), kv.to(td)
        out, whole = _guarded((n, C), td, guard_rows=2)
        lib = _lib()
        _call('ec_resnet_attnpool_attend', lib.ptr(q), lib.ptr(kv), n, L, C, lib.ptr(out), code)
        torch.cuda.synchronize()
        _assert_guard(whole, n * C, f'{dt} C={C} L={L} {name}')
        ref, budget, vmax = _attend_ref(q, kv, n, L, C)
        _assert_within(out, ref, u * ref.abs() + (1 + u) * budget + FLOOR, f'{dt} C={C} L={L} {name}')
        if name == 'flat':
            mean = kv[..., C:].double().mean(1)
            assert float((ref - mean).abs().max()) <= 1e-12 * float(vmax.max())
        if name.startswith('peaked'):       # the output is the best key's value (the rest weigh e^-30 together)
            vb = kv[:, int(name.split('@')[1]), C:].double()
            assert float((ref - vb).abs().max()) <= 1e-11 * L * float(vmax.max())


# ---- ec_resnet_attnpool_tokens ----
@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('HW,C', [(49, 2048), (81, 2560), (144, 3072), (196, 4096), (49, 320), (9, 72)])
def test_attnpool_tokens(dt, HW, C):
    """tokens = [mean_HW(x); x] + pos and q_in = token 0.  Token 0 against float64: the kernel sums HW values in
    sequence in fp32 (HW - 1 roundings, each at most 2^-24 sum |x|), divides (2^-24) and adds pos (2^-24 of
    |mean| + |pos|), then rounds to 16 bit: |got - ref| <= u |ref| + (1 + u) ((HW + 1) 2^-24 mean|x| +
    2^-24 (|mean| + |pos|)) + 2^-25.  Tokens 1.. are one fp32 addition and one rounding: bit-exact."""
    td, code, u = DT[dt]
    n = 3
    g = torch.Generator(device='cuda').manual_seed(HW * C)
    x = (torch.randn(n, HW, C, generator=g, device='cuda').abs() + 0.5).to(td)   # post-ReLU features
    pos = torch.randn(HW + 1, C, generator=g, device='cuda') * C ** -0.5
    tok, tw = _guarded((n, HW + 1, C), td, guard_rows=2)
    q_in, qw = _guarded((n, C), td, guard_rows=2)
    lib = _lib()
    _call('ec_resnet_attnpool_tokens', lib.ptr(x), n, HW, C, lib.ptr(pos), lib.ptr(tok), lib.ptr(q_in), code)
    torch.cuda.synchronize()
    _assert_guard(tw, n * (HW + 1) * C, 'tokens')
    _assert_guard(qw, n * C, 'q_in')
    assert torch.equal(tok[:, 1:], (x.float() + pos[1:]).to(td))
    assert torch.equal(q_in, tok[:, 0])
    x64 = x.double()
    mean = x64.mean(1)
    ref = mean + pos[0].double()
    absmean = x64.abs().mean(1)
    bound = u * ref.abs() + (1 + u) * ((HW + 1) * U32 * absmean + U32 * (mean.abs() + pos[0].double().abs())) + FLOOR
    _assert_within(tok[:, 0], ref, bound, f'{dt} token 0 HW={HW} C={C}')


# ---- ec_resnet_stem_rows ----
@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('R', [2, 224, 288, 384, 448])
def test_stem_rows_sizes(dt, R):
    """Both input modes, bit-exact: the 27 taps rounded to 16 bit, what that rounding lost, zeros beyond; uint8
    normalised as (v / 255 - mean) / std in fp32."""
    lib = _lib()
    td, code, _ = DT[dt]
    n = 2 if R <= 288 else 1
    g = torch.Generator().manual_seed(R)
    u8 = torch.randint(0, 256, (n, R, R, 3), generator=g, dtype=torch.uint8)
    mean = torch.tensor([0.48145466, 0.4578275, 0.40821073])
    std = torch.tensor([0.26862954, 0.26130258, 0.27577711])
    img = ((u8.float() / 255 - mean) / std).permute(0, 3, 1, 2).contiguous()
    want = F.unfold(img, 3, padding=1, stride=2)                       # [n, 3*9 (c, ky, kx), L]
    want = want.reshape(n, 3, 9, -1).permute(0, 3, 2, 1).reshape(n, R // 2, R // 2, 27)
    hi = want.to(td)
    want16 = torch.cat([hi, (want - hi.float()).to(td), torch.zeros(n, R // 2, R // 2, 10, dtype=td)], -1)
    for mode, inp in ((lib.EC_PRE_CHW_F32, img), (lib.EC_PRE_HWC_U8, u8)):
        rows, whole = _guarded((n, R // 2, R // 2, 64), td, guard_rows=64)
        inp = inp.cuda()
        _call('ec_resnet_stem_rows', lib.ptr(inp), mode, n, R, lib.ptr(rows), code)
        torch.cuda.synchronize()
        _assert_guard(whole, rows.numel(), f'stem rows R={R} mode={mode}')
        assert torch.equal(rows.cpu(), want16), (R, mode)


# ---- ec_resnet_avgpool ----
def _pool_widths():
    p = resnet.pad64
    ws = set()
    for arch in ARCHS:
        cfg = resnet.resnet_config(arch)
        ws.add(p(cfg['vision_width']))
        for _, inp, planes, stride, _ds in resnet.blocks_of(cfg):
            if stride > 1:
                ws.update({p(planes), p(inp)})
    return sorted(ws)


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('C', [8] + _pool_widths())
def test_avgpool_odd_sizes(dt, C):
    """AvgPool2d(2) at odd H and W drops the last row and column (F.avg_pool2d's floor), bit for bit."""
    lib = _lib()
    td, code, _ = DT[dt]
    n = 2
    g = torch.Generator(device='cuda').manual_seed(C)
    for H, W in ((7, 9), (13, 5), (3, 3), (5, 2), (2, 11)):
        x = torch.randn(n, H, W, C, generator=g, device='cuda').to(td)
        y, whole = _guarded((n, H // 2, W // 2, C), td, guard_rows=16)
        _call('ec_resnet_avgpool', lib.ptr(x), n, H, W, C, lib.ptr(y), code)
        torch.cuda.synchronize()
        _assert_guard(whole, y.numel(), f'avgpool {H}x{W} C={C}')
        want = F.avg_pool2d(x.cpu().float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).to(td)
        assert torch.equal(y.cpu(), want), (H, W, C)
