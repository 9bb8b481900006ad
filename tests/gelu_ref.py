"""Float64 yardsticks, the fp32 restatement and the per-element bounds of the EXACT GELU, x Phi(x) (ec_gemm_args.activation
= 1, ec_split16's gelu = 2, cfg['activation'] = 'gelu'): csrc/activation.h.

Nothing here touches a GPU or anything compiled.  The operand families, padding and guard helpers are tests/gemm_ref.py's
(imported, not edited); expect() below has the form of gemm_ref.expect for the four GELU epilogues with
    * the float64 reference x Phi(x) from erfc (no cancellation on either side),
    * the slope constant 1.13 (max |GELU'| = 1.129 at x = sqrt 2; the minimum is -0.129),
    * the formula's own term: |gelu_erf(x) - x Phi(x)| <= 2^-21 |x| for the fp32 value x the epilogue holds, and
      |gelu_erf_grad(x) - (Phi + x phi)| <= 2^-20 -- conditions of the feature, checked on the restatement in
      tests/test_gelu_ref_cpu.py, not figures read off a kernel.
"""
import math

import numpy as np
import torch

import gemm_ref as gr
import rowops_ref as rr
from gemm_ref import (BF16, EPS24, F16, F32, FLOOR16, KERNEL_FACTOR, U, c_acc, case_buffers, case_segments, case_to,  # noqa: F401
                      guards_intact, k_total, make_case, padded, product, random_operands, tails_bias, verify, window)

GELU_SLOPE = 1.13            # max |GELU'| (1.129 at x = sqrt 2)
FWD_REL = 2.0 ** -21         # |gelu_erf(x) - x Phi(x)| <= FWD_REL |x|
GRAD_ABS = 2.0 ** -20        # |gelu_erf_grad(x) - (Phi(x) + x phi(x))| <= GRAD_ABS
EPILOGUES = ('gelu16', 'gelu16_ln', 'gelu16_save', 'gelu_bwd16')


# ---------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------
def phi64(x):
    """Phi(x) in float64 without cancellation: erfc(|x| / sqrt 2) / 2 for x < 0, 1 - that otherwise."""
    x = x.double()
    h = 0.5 * torch.special.erfc(x.abs() / math.sqrt(2.0))
    return torch.where(x < 0, h, 1 - h)


def gelu64(x):
    x = x.double()
    return x * phi64(x)


def grad64(x):
    x = x.double()
    return phi64(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def exact_gelu(x):
    """What the tests put in place of oracle.clip_ref.quick_gelu: torch's own erf GELU, in the dtype of x (float64 and
    autograd come with it)."""
    return torch.nn.functional.gelu(x)


# ---------------------------------------------------------------------------------------------------------------
# the device formula restated in numpy fp32 (csrc/activation.h, line for line).  An fma is restated as the float64 product
# (exact: two 24-bit factors) plus the addend, rounded to fp32 once more (a double rounding in 1 case of ~2^29, half an ulp
# of an ulp); exp2 and the reciprocal are numpy's (v_exp_f32 / v_rcp_f32: 1 ulp each).
# ---------------------------------------------------------------------------------------------------------------
f32 = np.float32
P = f32(f32(0.3275911) * f32(0.70710678118654752))
E = f32(f32(-0.5) * f32(1.4426950408889634))
A = [f32(f32(0.5) * f32(a)) for a in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)]
PHI0 = f32(0.3989422804014327)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _tail32(x):
    """-> (h = Phi(-|x|), e = exp(-x^2 / 2)) in fp32."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(over='ignore', under='ignore', invalid='raise'):
        t = (f32(1) / _fma(np.abs(x), P, f32(1))).astype(f32)
        e = np.exp2(((x * x).astype(f32) * E).astype(f32)).astype(f32)
        p = _fma(t, A[4], A[3])
        for a in (A[2], A[1], A[0]):
            p = _fma(t, p, a)
        return ((p * t).astype(f32) * e).astype(f32), e


def gelu32(x):
    x = np.asarray(x, dtype=f32)
    h, _ = _tail32(x)
    with np.errstate(over='ignore', under='ignore'):
        return (x * np.where(x < 0, h, (f32(1) - h).astype(f32))).astype(f32)


def grad32(x):
    x = np.asarray(x, dtype=f32)
    h, e = _tail32(x)
    with np.errstate(over='ignore', under='ignore'):
        return _fma((x * PHI0).astype(f32), e, np.where(x < 0, h, (f32(1) - h).astype(f32)))


def gelu32_t(x):
    """torch fp32 in, torch fp32 out (the restatement of a GEMM epilogue on an fp32 accumulator)."""
    return torch.from_numpy(gelu32(x.detach().cpu().float().numpy())).to(x.device)


def grad32_t(x):
    return torch.from_numpy(grad32(x.detach().cpu().float().numpy())).to(x.device)


def grid():
    """The grid the two conditions are stated on: 2 M points on [-12, 12] and every finite fp16 value with |x| <= 64."""
    lin = np.linspace(-12.0, 12.0, 2_000_001).astype(f32)
    h = np.arange(65536, dtype=np.uint16).view(np.float16).astype(f32)
    h = h[np.isfinite(h) & (np.abs(h) <= 64)]
    return np.concatenate([lin, h])


def formula_errors(x):
    """-> (max of |gelu32 - x Phi| / |x| over x != 0, max of |grad32 - (Phi + x phi)|) against float64."""
    xt = torch.from_numpy(np.asarray(x, dtype=f32))
    fwd = (torch.from_numpy(gelu32(x)).double() - gelu64(xt)).abs()
    nz = xt != 0
    rel = float((fwd[nz] / xt[nz].double().abs()).max())
    assert float(fwd[~nz].max() if bool((~nz).any()) else 0.0) == 0.0
    return rel, float((torch.from_numpy(grad32(x)).double() - grad64(xt)).abs().max())


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def gelu_e(v, e):
    """Error of gelu_erf on an fp32 value within e of v, against gelu64(v): the slope times e, and the formula's term at
    a point within e of v."""
    return GELU_SLOPE * e + FWD_REL * (v.abs() + e)


# The negative tail.  FWD_REL |x| is an absolute bound: at x = -6 it allows 2.9e-6 where x Phi(x) = -5.9e-9, so it cannot
# tell a Phi computed as (1 + erf) / 2 in fp32 (erf(-4.24) rounds to -1: Phi = 0, everything cancelled) from one computed
# without cancellation.  What can: a result of the right sign and size.  Any formula of the form erfc(z) = q(z) exp(-z^2) with a
# bounded q keeps a bounded RELATIVE error out there; Abramowitz-Stegun 7.1.26's tends to a1 sqrt(pi) / p - 1 = 0.379 as z grows
# (t -> 1 / (p z) against erfc(z) -> exp(-z^2) / (z sqrt pi)), hence 0.4.  Held on [-12, 0) (x Phi(x) >= 2e-32 in size, far
# inside fp32's and bf16's normal range), above `floor` (an f16 part: its subnormal step, which hides the tail from -5.5 on).
TAIL_REL = 0.4
TAIL_LO = -12.0


def tail_check(val, x, floor, what):
    """val: float64 results (a formula's fp32 value, or hi + lo of a split) at the fp32 inputs x."""
    sel = (x < 0) & (x >= TAIL_LO)
    ref = gelu64(x[sel])
    over = rr.excess(val[sel].double(), ref, TAIL_REL * ref.abs() + floor)
    assert over <= 0, f'{what}: the negative tail is {over:.3e} outside {TAIL_REL} of x Phi(x) (cancellation?)'


def split_input(n, device='cpu', huge=False):
    """fp32 [n] for ec_split16(gelu = 2): rowops_ref.split_input (Gaussian x 3 with stretches around +-20 and +-60 and tiny
    values) with gemm_ref.GELU_TAILS, zero of both signs, -6 (the planted cancellation) and the end of the tail range at
    the front; huge (a bf16 output, which can hold them): values whose square overflows fp32 behind them."""
    x = rr.split_input(n, device=device)
    head = gr.GELU_TAILS + (-0.0, -6.0, -8.0, TAIL_LO) + ((3.0e38, -3.0e38, 2.0e19, -2.0e19) if huge else ())
    head = torch.tensor(head, dtype=F32, device=device)
    k = min(n, head.numel())
    x[:k] = head[:k]
    return x


def split_bounds(x, dtype, lo_dtype):
    """ec_split16(gelu = 2) on the fp32 input x itself (e = 0) -> (ref, bound of hi, bound of hi + lo)."""
    ref = gelu64(x)
    e = gelu_e(x.double(), 0.0)
    return ref, rr.bound16(ref, e, dtype), rr.bound_pair(ref, e, dtype, lo_dtype)


def expect(epi, dtype, acc, S, ktot, bias=None, u=None, stats=None, colsum=None, lo_out=None):
    """gemm_ref.expect for the random / tails families of the GELU epilogues with activation = 1 -> specs for
    gemm_ref.check / verify.  acc, S: gemm_ref.product()."""
    assert epi in EPILOGUES
    c = c_acc(ktot)
    b = 0 if bias is None else bias.double()[None]
    u16 = U[dtype]
    if epi == 'gelu16_ln':
        st = stats.double()
        r0, r1, cs = st[:, :1], st[:, 1:], colsum.double()[None]
        v = r0 * acc + r1 * cs + b
        s_ln = r0.abs() * S + (r1 * cs).abs() + (b.abs() if bias is not None else 0)
        e = KERNEL_FACTOR * EPS24 * (c * r0.abs() * S + gr.C_FOLD * s_ln)
    else:
        v = acc + b
        S = S + (b.abs() if bias is not None else 0)
        e = KERNEL_FACTOR * c * EPS24 * S
    if epi == 'gelu_bwd16':
        # out = round16(round16(acc + bias) GELU'(u)): the inner rounding as in gemm_ref.expect; the derivative is the fp32
        # formula on the 16-bit u itself (GRAD_ABS), the product one fp32 rounding, the outer rounding the output's
        gd = grad64(u)
        ref = v * gd
        inner = u16 * v.abs() + FLOOR16 + e
        eb = gd.abs() * inner * (1 + u16) + (v.abs() + inner) * GRAD_ABS + EPS24 * (v.abs() + inner) * (gd.abs() + GRAD_ABS)
        return [('out', ref, rr.bound16(ref, eb, dtype))]
    ref = gelu64(v)
    eg = gelu_e(v, e)
    specs = [('out', ref, rr.bound16(ref, eg, dtype))]
    if epi == 'gelu16_save':
        specs.append(('aux', v, rr.bound16(v, e, dtype)))
    if lo_out == '16':
        specs.append(('out+aux', ref, rr.bound_pair(ref, eg, dtype, dtype)))
    elif lo_out == 'e4m3':
        specs.append(('out+aux8', ref, eg))
    return specs


def case_specs(c, acc_s=None):
    """gemm_ref.case_specs with expect() above (sets c['aux_exp'] for an e4m3 lo output the same way)."""
    segs = case_segments(c)
    acc, S = product(segs) if acc_s is None else acc_s
    specs = expect(c['epi'], c['dtype'], acc, S, k_total(segs), c['bias'], c.get('u'), c.get('stats'), c.get('colsum'), c['lo_out'])
    if c['lo_out'] == 'e4m3':
        vmax = float(specs[0][1].abs().max())
        lo_max = 2 * U[c['dtype']] * vmax + 2.0 ** -20
        c['aux_exp'] = max(-60, min(60, int(math.floor(math.log2(448.0 / lo_max)))))
    return specs


def restate(c, gelu=None, grad=None):
    """The fp32 restatement of the case's epilogue on gemm_ref.product32's accumulator, with ``gelu`` / ``grad`` (fp32 torch
    -> fp32 torch) as the activation and its derivative: the restatement of the device formula by default, a planted fault
    otherwise -> got dict for gemm_ref.check."""
    gelu, grad = gelu or gelu32_t, grad or grad32_t
    epi, dtype = c['epi'], c['dtype']
    acc32 = gr.product32(case_segments(c))
    b = torch.zeros((), dtype=F32) if c['bias'] is None else c['bias'].float()[None]
    if epi == 'gelu16_ln':
        v = acc32 * c['stats'][:, :1].float() + (c['colsum'].float()[None] * c['stats'][:, 1:].float() + b)
    else:
        v = acc32 + b
    if epi == 'gelu_bwd16':
        return {'out': (v.to(dtype).float() * grad(c['u'].float())).to(dtype)}
    got = {}
    if epi == 'gelu16_save':
        got['aux'] = v.to(dtype)
    v = gelu(v)
    got['out'] = v.to(dtype)
    l32 = v - got['out'].float()
    if c['lo_out'] == '16':
        got['aux'] = l32.to(dtype)
    elif c['lo_out'] == 'e4m3':
        q = (l32 * 2.0 ** c['aux_exp']).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        got['aux8'] = q.double() * 2.0 ** -c['aux_exp']
    return got


def rel_err(got, ref):
    """tests/test_towers_gpu.py's: the largest difference over the largest reference value."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
