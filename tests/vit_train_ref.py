"""Float64 restatements of the fine-tuning backward pass of csrc/vit_train.hip, stage by stage, each carrying a
per-element error bound next to its value.  Test infrastructure only: plain torch float64 (on whatever device the
inputs live), never the project's kernels.

A restated quantity is a pair (v, e): v the float64 value, e a float64 tensor that bounds |kernel - v| element by
element, or None when the kernel reads exactly v (a tape entry, a 16-bit weight copy, an fp32 master).  The rules:

* Products.  The kernels multiply 16-bit operands exactly in fp32 and add K products in fp32, in whatever order
  (MFMA steps, K-batches and their reduction, one more addition for a bias or a residual): every addition rounds
  once, relative to a partial sum no larger than the sum of the magnitudes, so an exact-input product is within
  gamma(K) sum |a||b| with gamma(K) = (K + 4) 2^-24 of the float64 one, whatever the order.  An input that is only
  known to within e contributes sum |a| e_b + e_a |b| + e_a e_b on top, and gamma applies to the magnitudes widened
  by the bounds (``mm``).
* 16-bit stores.  Kernel and restatement round their own values to 16 bit, each by at most half an ulp
  (u = 2^-11 f16, 2^-8 bf16 of the value, plus half the f16 subnormal step): e' = e + u (2 |v| + e) + 2^-24 (``r16``).
  A value the kernel rounds inside a kernel (the attention backward's P and dS) is treated the same way.
* fp32 elementwise steps add 2^-24 of their result; fp32 transcendental functions (exp2, the QuickGELU sigmoid) are
  allowed 2^-20 relative: their hardware approximations are within a few ulp.
* LayerNorm (fp32, one row of W per wave): every sum of the row is a sum of W terms, so each is within
  gamma(W) of its magnitude; the statistics' errors scale x hat by at most the same relative amount.

Layout of the stages (ec_vit_train_backward_stages): 0 = the head, 1 .. L = blocks L - 1 .. 0, L + 1 = the
embedding."""
import torch

U32 = 2.0 ** -24
SUB16 = 2.0 ** -25                 # half the f16 subnormal step (bf16's is far below anything here)
TRANS = 2.0 ** -20                 # relative error allowed to an fp32 exp2 / sigmoid
LN_EPS = 1e-5
# exp2 argument scale of the attention kernels: 0.125 * log2(e) rounded to fp32 (the kernel's constant)
SCALE_LOG2E = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))
LOG2E = 1.4426950408889634


# The shapes the stage tests run (2-block towers): arch geometry (image_size, patch, width), images, why.
ARCH = {'B/16': (224, 16, 768), 'L/14': (224, 14, 1024), 'L/14@336': (336, 14, 1024), 'wide_odd': (48, 16, 128),
        'tiny': (8, 4, 64)}
CASES = {
    'b16_n32': ('B/16', 32, 'shipped ftclip batch (M = 6304)'),
    'b16_n128': ('B/16', 128, 'shipped ftclip batch (M = 25216)'),
    'l14_n32': ('L/14', 32, 'shipped per-GPU batch (M = 8224)'),
    'l14_n64': ('L/14', 64, 'gemm_rows32 tail split: rem 64, extra round, K = 4096 (M = 16448)'),
    'l14_336_n2': ('L/14@336', 2, 'S = 577: attention backward chunks of 288 + 1 (M = 1154)'),
    'wide_odd_n9': ('wide_odd', 9, '64-row padding, one K-batch, W < 256 (M = 90)'),
    'tiny_n5': ('tiny', 5, 'smallest tower (M = 25)'),
}


def case_geometry(case):
    """-> (image_size, patch, width, n_img, S, M)"""
    arch, n, _ = CASES[case]
    R, P, W = ARCH[arch]
    S = (R // P) ** 2 + 1
    return R, P, W, n, S, n * S


def u16(dtype):
    """Unit roundoff of a 16-bit store."""
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def gamma(k):
    return (k + 4) * U32


def r16(v, e, dtype):
    """(v, e) stored as 16 bit by both sides."""
    e = torch.zeros_like(v) if e is None else e
    return v.to(dtype).double(), e + u16(dtype) * (2 * v.abs() + e) + 2 * SUB16


def mm(a, ea, b, eb):
    """a [.., m, K] @ b [.., K, n] with the bound of an fp32-accumulated product of the kernel's versions."""
    K = a.shape[-1]
    v = a @ b
    A, B = a.abs(), b.abs()
    if ea is None and eb is None:
        return v, gamma(K) * (A @ B)
    Aw = A if ea is None else A + ea
    Bw = B if eb is None else B + eb
    wide = Aw @ Bw
    return v, gamma(K) * wide + (wide - A @ B).clamp_min(0)


def colsum(x, ex):
    """Column sums over the rows (the bias gradients: fp32 partial sums of slabs, reduced in a fixed order)."""
    v = x.sum(0)
    mag = (x.abs() + (0 if ex is None else ex)).sum(0)
    return v, gamma(x.shape[0]) * mag + (0 if ex is None else ex.sum(0))


def add(a, ea, b, eb):
    v = a + b
    e = U32 * v.abs()
    for t in (ea, eb):
        if t is not None:
            e = e + t
    return v, e


def ln_forward(x, g, b):
    """fp32 LayerNorm of exact fp32 rows (ln_f32_kernel): value and bound."""
    W = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + LN_EPS)
    xh = xc * rstd
    v = xh * g + b
    return v, 2 * gamma(W) * (xh.abs() * g.abs() + b.abs())


def ln_backward(x, dy, edy, gamma_w):
    """LayerNorm backward (ln_bwd_kernel) from the saved input x (exact fp32 rows) and dy (bounded):
    dx = rstd (g - mean(g) - xh mean(g xh)) with g = dy gamma, d gamma = sum dy xh, d beta = sum dy.
    -> ((dx, e), (dgamma, e), (dbeta, e))."""
    W = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + LN_EPS)
    xh = xc * rstd
    g = dy * gamma_w
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    dx = rstd * (g - m1 - xh * m2)
    gw = gamma(W)
    # rounding of the fp32 sums and products of the row (relative gw to the magnitudes of every term), and the
    # statistics' relative error gw on x hat and rstd
    mag = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    e_dx = 4 * gw * mag
    e_dg = gamma(x.shape[0]) * (dy * xh).abs().sum(0) + 2 * gw * (dy * xh).abs().sum(0)
    e_db = gamma(x.shape[0]) * dy.abs().sum(0)
    if edy is not None:
        eg = edy * gamma_w.abs()
        e_dx = e_dx + rstd * (eg + eg.mean(-1, keepdim=True) + xh.abs() * (eg * xh.abs()).mean(-1, keepdim=True))
        e_dg = e_dg + (edy * xh.abs()).sum(0)
        e_db = e_db + edy.sum(0)
    return (dx, e_dx), ((dy * xh).sum(0), e_dg), (dy.sum(0), e_db)


def quick_gelu(y):
    return y * torch.sigmoid(1.702 * y)


def quick_gelu_grad(u):
    s = torch.sigmoid(1.702 * u)
    return s * (1 + 1.702 * u * (1 - s))


# ---------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------
def attention_backward(qkv, out, lse, dout, edout, n, S, heads, dtype, chunk=8):
    """ec_attention_backward on the 16-bit q | k | v, the forward output, the kernel's own lse (log2 units) and dO
    (bounded by edout, or exact): P = exp2(s * SCALE_LOG2E - lse), D = <dO, O>, dS = P (dP - D); the kernels
    round P and dS to 16 bit as MFMA operands; dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO, stored as 16 bit.
    -> (dqkv [n S, 3 W], bound, delta [n, heads, S], bound).  ``chunk`` images at a time."""
    W = heads * 64
    dq_all, e_all, d_all, ed_all = [], [], [], []
    for i0 in range(0, n, chunk):
        m = min(chunk, n - i0)
        rows = slice(i0 * S, (i0 + m) * S)

        def heads_of(t, j):        # [m S, 3W or W] -> [m, heads, S, 64] of projection j
            return t[rows, j * W:(j + 1) * W].reshape(m, S, heads, 64).transpose(1, 2)
        q, k, v = (heads_of(qkv, j) for j in range(3))
        o, do = heads_of(out, 0), heads_of(dout, 0)
        edo = None if edout is None else heads_of(edout, 0)
        l2 = lse[i0:i0 + m].unsqueeze(-1)                               # [m, h, S, 1]
        delta, e_delta = mm(do.unsqueeze(-2), None if edo is None else edo.unsqueeze(-2), o.unsqueeze(-1), None)
        delta, e_delta = delta[..., 0], e_delta[..., 0]                 # [m, h, S, 1]
        s, e_s = mm(q, None, k.transpose(-1, -2), None)                 # [m, h, Sq, Sk]
        t = s * SCALE_LOG2E - l2
        e_t = e_s * SCALE_LOG2E + U32 * (s.abs() * SCALE_LOG2E + l2.abs())
        P = torch.exp2(t)
        e_P = P * (torch.expm1(e_t / LOG2E) + TRANS)
        dp, e_dp = mm(do, edo, v.transpose(-1, -2), None)
        dd = dp - delta
        ds = P * dd
        e_ds = e_P * dd.abs() + (P + e_P) * (e_dp + e_delta) + 2 * U32 * ds.abs()
        P16, e_P16 = r16(P, e_P, dtype)
        ds16, e_ds16 = r16(ds, e_ds, dtype)
        dqv, dqe = mm(ds16, e_ds16, k, None)
        dkv, dke = mm(ds16.transpose(-1, -2), e_ds16.transpose(-1, -2), q, None)
        dvv, dve = mm(P16.transpose(-1, -2), e_P16.transpose(-1, -2), do, edo)
        outs = [r16(0.125 * dqv, 0.125 * dqe, dtype), r16(0.125 * dkv, 0.125 * dke, dtype), r16(dvv, dve, dtype)]
        dq_all.append(torch.cat([t[0].transpose(1, 2).reshape(m * S, W) for t in outs], 1))
        e_all.append(torch.cat([t[1].transpose(1, 2).reshape(m * S, W) for t in outs], 1))
        d_all.append(delta[..., 0])
        ed_all.append(e_delta[..., 0])
        del s, e_s, t, e_t, P, e_P, dp, e_dp, dd, ds, e_ds, P16, e_P16, ds16, e_ds16
    return torch.cat(dq_all), torch.cat(e_all), torch.cat(d_all), torch.cat(ed_all)


def attention_lse(qkv, n, S, heads, dtype, chunk=8):
    """The forward's log-sum-exp in log2 units, and its bound: the kernel sums the probabilities as the 16-bit MFMA
    operands they become (relative u each, a subnormal f16 one absolutely), after a score error of gamma(64)."""
    W = heads * 64
    out, err = [], []
    for i0 in range(0, n, chunk):
        m = min(chunk, n - i0)
        rows = slice(i0 * S, (i0 + m) * S)
        q, k = (qkv[rows, j * W:(j + 1) * W].reshape(m, S, heads, 64).transpose(1, 2) for j in range(2))
        s, e_s = mm(q, None, k.transpose(-1, -2), None)
        t = s * SCALE_LOG2E
        lse = torch.logsumexp(t / LOG2E, -1) * LOG2E
        e_t = (e_s * SCALE_LOG2E).amax(-1) + U32 * t.abs().amax(-1)
        out.append(lse)
        err.append(e_t + LOG2E * (2 * u16(dtype) + S * 2 * SUB16 + gamma(S)) + 1e-6)
    return torch.cat(out), torch.cat(err)


# ---------------------------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------------------------
def d64(t):
    return t.double()


def block_forward(tape, w16, master, dtype, n, S, heads):
    """The tape entries a block's forward writes, from the tape's own inputs (x, att, h2, gact, qkv):
    xm = x + att out_w^T + out_b, u = 16(h2 fc1_w^T + fc1_b), gact = 16(QuickGELU(h2 fc1_w^T + fc1_b)),
    x_next = xm + gact fc2_w^T + fc2_b (the RESID32 GEMM, with gemm_rows32's K-batched tail), lse."""
    xm, exm = mm(d64(tape['att']), None, d64(w16['out_w']).T, None)
    xm, exm = xm + d64(tape['x']) + d64(master['out_b']), exm + gamma(0) * (d64(tape['x']).abs() + d64(master['out_b']).abs())
    pre, epre = mm(d64(tape['h2']), None, d64(w16['fc1_w']).T, None)
    pre, epre = pre + d64(master['fc1_b']), epre + gamma(0) * d64(master['fc1_b']).abs()
    u = r16(pre, epre, dtype)
    gl = quick_gelu(pre)
    g = r16(gl, 1.13 * epre + TRANS * pre.abs() * (1 + 1.702 * pre.abs()), dtype)   # |QuickGELU'| <= 1.13
    xn, exn = mm(d64(tape['gact']), None, d64(w16['fc2_w']).T, None)
    xn, exn = xn + d64(tape['xm']) + d64(master['fc2_b']), exn + gamma(0) * (d64(tape['xm']).abs() + d64(master['fc2_b']).abs())
    lse = attention_lse(d64(tape['qkv']), n, S, heads, dtype)
    return dict(xm=(xm, exm), u=u, gact=g, x_next=(xn, exn), lse=lse)


def block_backward(tape, dx_in, dx16_in, w16, master, dtype, n, S, heads):
    """Stage of block l (csrc/vit_train.hip: ec_vit_train_backward_stages, the block loop) from the tape, the entry
    dx (fp32) and dx16 (its 16-bit copy, what the dX GEMMs read) snapshotted from the workspace, the 16-bit weight
    copies (``w16``: qkv_w, out_w, fc1_w, fc2_w in their state-dict layouts) and the fp32 LayerNorm masters.
    -> dict of (value, bound): the block's twelve gradients, the exit dx and dx16, and what the stage leaves in the
    workspace: g16 (dq | dk | dv), da16, dh32, delta."""
    dx, dx16 = d64(dx_in), d64(dx16_in)
    r = {}
    # x[l + 1] = xm + c_proj(QuickGELU(c_fc(ln_2(xm))))
    r['fc2_b'] = colsum(dx, None)
    r['fc2_w'] = mm(dx16.T, None, d64(tape['gact']), None)
    acc = mm(dx16, None, d64(w16['fc2_w']), None)
    a16, ea16 = r16(*acc, dtype)
    gg = quick_gelu_grad(d64(tape['u']))
    du_pre = a16 * gg
    egg = TRANS * (1 + gg.abs() + 1.702 * d64(tape['u']).abs())
    du, edu = r16(du_pre, ea16 * gg.abs() + (a16.abs() + ea16) * egg + U32 * du_pre.abs(), dtype)
    r['fc1_b'] = colsum(du, edu)
    r['fc1_w'] = mm(du.T, edu.T, d64(tape['h2']), None)
    dh, edh = mm(du, edu, d64(w16['fc1_w']), None)
    (d_ln, e_ln), r['ln2_g'], r['ln2_b'] = ln_backward(d64(tape['xm']), dh, edh, d64(master['ln2_g']))
    dxm, edxm = add(dx, None, d_ln, e_ln)
    dxm16, edxm16 = r16(dxm, edxm, dtype)
    # xm = x[l] + out_proj(attention(in_proj(ln_1(x[l]))))
    r['out_b'] = colsum(dxm, edxm)
    r['out_w'] = mm(dxm16.T, edxm16.T, d64(tape['att']), None)
    da16 = r16(*mm(dxm16, edxm16, d64(w16['out_w']), None), dtype)
    r['da16'] = da16
    g16, eg16, delta, edelta = attention_backward(d64(tape['qkv']), d64(tape['att']), d64(tape['lse']), da16[0], da16[1],
                                                  n, S, heads, dtype)
    r['g16'], r['delta'] = (g16, eg16), (delta, edelta)
    r['qkv_b'] = colsum(g16, eg16)
    r['qkv_w'] = mm(g16.T, eg16.T, d64(tape['h1']), None)
    dh, edh = mm(g16, eg16, d64(w16['qkv_w']), None)
    r['dh32'] = (dh, edh)
    (d_ln, e_ln), r['ln1_g'], r['ln1_b'] = ln_backward(d64(tape['x']), dh, edh, d64(master['ln1_g']))
    r['dx'] = add(dxm, edxm, d_ln, e_ln)
    r['dx16'] = r16(*r['dx'], dtype)
    r['dxm16'] = (dxm16, edxm16)
    return r


def head_backward(x_last, clsln_k, dclsln_k, d_feats, master, n, S, dtype):
    """Stage 0: clsln = ln_post(class rows of x[L]) (fp32), d proj = clsln^T d_feats, d cls_ln = d_feats proj^T
    (fp32 products), ln_post backward into the class rows of dx (every other row zero) and its 16-bit copy.  The
    products and the LayerNorm backward take the kernel's own clsln / dclsln (read back from the workspace): each
    step is checked on exact inputs."""
    W = x_last.shape[1]
    cls = d64(x_last).view(n, S, W)[:, 0]
    r = {'clsln': ln_forward(cls, d64(master['ln_post.weight']), d64(master['ln_post.bias']))}
    r['proj'] = mm(d64(clsln_k).T, None, d64(d_feats), None)
    r['dclsln'] = mm(d64(d_feats), None, d64(master['proj']).T, None)
    (dcls, edcls), r['ln_post.weight'], r['ln_post.bias'] = ln_backward(cls, d64(dclsln_k), None,
                                                                         d64(master['ln_post.weight']))
    dx = torch.zeros(n, S, W, dtype=torch.float64, device=cls.device)
    edx = torch.zeros_like(dx)
    dx[:, 0], edx[:, 0] = dcls, edcls
    r['dx'] = (dx.view(n * S, W), edx.view(n * S, W))
    r['dx16'] = r16(*r['dx'], dtype)
    return r


def embedding_backward(pre, dx_in, dh32_k, patches, master, n, S, k, dtype):
    """Stage L + 1: de = ln_pre backward of the entry dx (into dh32), d ln_pre; d positional_embedding = sum over
    images of de, d class_embedding its row 0; d conv1 = 16(de)^T [hi | lo] folded over the two halves of the patch
    row.  The sums over images and the conv1 product take the kernel's own de (dh32, read back)."""
    W = pre.shape[1]
    r = {}
    r['dh32'], r['ln_pre.weight'], r['ln_pre.bias'] = ln_backward(d64(pre), d64(dx_in), None, d64(master['ln_pre.weight']))
    de = d64(dh32_k).view(n, S, W)
    pos = de.sum(0)
    r['positional_embedding'] = (pos, gamma(n) * de.abs().sum(0))
    r['class_embedding'] = (pos[0], r['positional_embedding'][1][0])
    rows = de[:, 1:].reshape(-1, W).to(dtype).double()           # the patch rows, rounded as the transpose stores them
    p = d64(patches).reshape(rows.shape[0], -1)
    fold = torch.cat([p[:, :k], p[:, k:2 * k]], 0)
    r['conv1.weight'] = mm(torch.cat([rows, rows], 0).T, None, fold, None)
    return r


def lora_grads(x, dy, edy, down16, up16t, r, dtype):
    """Factor gradients of one projection y = x (W + up down)^T straight from the activations: P = x down^T,
    d up = dy^T P [W, r]; Q = dy up, d down = Q^T x [r, W].  down16 / up16t: the 16-bit factor copies [>= r, W].
    The kernels keep P and Q as hi / lo 16-bit planes (lo scaled by LoShift): about 22 significand bits for f16,
    16 for bf16 (relative u^2 each, twice for the two roundings) besides the fp32 product's own error."""
    u2 = 2 * u16(dtype) ** 2
    dn, upt = d64(down16)[:r], d64(up16t)[:r]
    P, eP = mm(x, None, dn.T, None)
    eP = eP + u2 * (P.abs() + eP) + 2.0 ** -36
    Q, eQ = mm(dy, edy, upt.T, None)
    eQ = eQ + u2 * (Q.abs() + eQ) + 2.0 ** -36
    d_up = mm(dy.T, None if edy is None else edy.T, P, eP)
    d_down = mm(Q.T, eQ.T, x, None)
    return d_up, d_down
