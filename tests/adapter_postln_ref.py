"""The post-LN feature adapter and the max-aggregation loss head, written once over tests/fewshot_ref.py's arithmetic.

Post-LN is nn.TransformerEncoderLayer(norm_first=False) with torch defaults, per layer
    s1 = x + dropout1(out_proj(attn(in_proj(x), key_padding_mask)));   a = norm1(s1)
    s2 = a + dropout2(linear2(dropout(relu(linear1(a)))));              x' = norm2(s2)
over the stages of fewshot_ref (gemm, ln_fwd, ln_bwd, attn_fwd, attn_bwd, colsum, keep_matrix): A64 is the yardstick, A32
(fp32, index order) the restatement.  The tape uses the slots of the pre-LN one (include/eventclip_hip.h): h1 = s1, xhat1 /
rstd1 / a of norm1, qkv = in_proj of the layer's input, P, o, f, xhat2 / rstd2 / bn of norm2; s2 is not kept.

tests/test_adapter_postln_cpu.py confirms the A64 functions against torch's float64 module and autograd and runs the checks
below against planted faults; tests/test_adapter_postln_gpu.py and tests/test_train_max_gpu.py hold the kernels to them.
Nothing here touches a GPU or anything compiled."""
import torch

import fewshot_ref as fr
from fewshot_ref import (A64, F64, _heads, _keeps, attn_bwd, attn_bwd_S, attn_fwd, attn_fwd_S, axpby, axpby_S, bound, colsum,
                         colsum_S, f32, gemm, gemm_S, keep_scale, ln_bwd, ln_bwd_S, ln_fwd, ln_fwd_S, within)

# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
# serving kernel: (B, T, D, d, heads, ffn, layers, residual)
SERVE_CASES = ((1, 1, 8, 8, 1, 4, 1, 0.0),            # the smallest shape
               (3, 5, 64, 32, 4, 48, 2, 0.5),         # ffn < 3 d
               (2, 16, 64, 32, 4, 160, 8, 0.5),       # T = AD_MAXT, ffn > 3 d, 8 layers
               (3, 15, 52, 40, 5, 72, 1, 0.8),        # width no multiple of 64
               (2, 3, 64, 320, 5, 64, 1, 0.0),        # a Linear wider than the workgroup
               (4, 16, 768, 256, 4, 1024, 2, 0.95))   # the only shape that takes the LDS opt-in above 64 KB
SERVE_RTOL, SERVE_ATOL = 1e-4, 1e-5                    # the project's for this kernel (tests/test_models_gpu.py)
# training end to end: (B, T, D, K, d, heads, ffn, layers)
E2E_SHAPES = ((3, 5, 64, 7, 32, 4, 48, 2), (2, 16, 64, 5, 32, 4, 160, 8), (5, 3, 64, 2, 32, 4, 48, 1))
MAX_SHAPES = E2E_SHAPES + ((4, 1, 64, 3, 32, 4, 48, 1),)          # + T = 1
FIXTURE_GEOMETRY = dict(D=64, d=32, heads=4, ffn=48, layers=2, B=3, T=5)
LOGIT_SCALE = 100.0
MIN_GAP = 0.05            # logit units between the two best valid views of every (sample, class) of a max case
MIN_LOSS = 0.05           # a saturated problem (every sample classified with p = 1) has gradients that are all cancellation:
#                           a tolerance relative to the largest gradient means nothing there
# seeds of max_inputs per shape of MAX_SHAPES, the first from 0 whose float64 gap (identity, pre-LN and post-LN adapter) is
# at least 0.1 and whose float64 loss is at least 0.1 in every configuration the GPU tests run:
# tests/test_adapter_postln_cpu.py asserts MIN_GAP and MIN_LOSS on them
MAX_SEEDS = (1, 0, 0, 0)
# (layout, agg, probs loss) of every end-to-end comparison on these inputs
E2E_CONFIGS = tuple((l, 'max', p) for l in (None, 'pre', 'post') for p in (False, True)) + (('post', 'sum', False), ('post', 'mean', True))


def loss_tol(loss):
    return 2e-4 * max(1.0, abs(float(loss)))


LOGITS_RTOL, LOGITS_ATOL, GRAD_TOL = 2e-4, 2e-3, 3e-4   # the project's for these steps (tests/test_train_gpu.py)


def assert_e2e(got_loss, got_logits, got_grads, want_loss, want_logits, want_grads, what):
    """loss, aggregated logits and every gradient of a training step against float64 at the project's tolerances."""
    assert abs(float(got_loss) - float(want_loss)) <= loss_tol(want_loss), f'{what}: loss {float(got_loss)} vs {float(want_loss)}'
    if got_logits is not None:
        torch.testing.assert_close(got_logits.double().cpu(), want_logits, rtol=LOGITS_RTOL, atol=LOGITS_ATOL, msg=f'{what}: logits')
    assert set(got_grads) == set(want_grads), f'{what}: {set(got_grads) ^ set(want_grads)}'
    worst = 0.0
    for k, w in want_grads.items():
        err = float((got_grads[k].double().cpu() - w).abs().max())
        lim = GRAD_TOL * float(w.abs().max())
        assert err <= lim, f'{what}: d {k}: error {err:.3e} > {lim:.3e}'
        worst = max(worst, err / max(lim, 1e-300))
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the post-LN adapter over an arithmetic
# ---------------------------------------------------------------------------------------------------------------
def postln_forward(ar, img, valid, top, blocks, heads, residual, p=0.0, seed=0, fault=None):
    """-> (out [B, T, D], tape dict: h0, hfin, y and per layer the slots named above).
    fault: 'pre_ln' the pre-LN layer; 'no_last_norm2' the last layer's norm2 left out; 'res2_from_s1' the second residual
    taken from norm1's input."""
    if fault == 'pre_ln':
        return fr.adapter_forward(ar, img, valid, top, blocks, heads, residual, p, seed)
    B, T, D = img.shape
    R = B * T
    d, ffn = top['in_w'].shape[0], blocks[0]['w1'].shape[0]
    cv = lambda t: t.to(ar.dtype)     # noqa: E731
    x = cv(img).reshape(R, D)
    h = gemm(ar, x, cv(top['in_w']).T, bias=cv(top['in_b']))
    tape = {'h0': h, 'L': []}
    for l, bp in enumerate(blocks):
        w = {k: cv(v) for k, v in bp.items()}
        ks = [cv(k) for k in _keeps(seed, p, l, B, T, d, heads, ffn)]
        qkv = gemm(ar, h, w['qkv_w'].T, bias=w['qkv_b'])
        P, o = attn_fwd(ar, qkv.reshape(B, T, 3 * d), valid, heads, ks[0] if p > 0 else None)
        o = o.reshape(R, d)
        s1 = h + ks[1] * gemm(ar, o, w['o_w'].T, bias=w['o_b'])
        a, xhat1, rstd1 = ln_fwd(ar, s1, w['ln1_g'], w['ln1_b'])
        f = ks[2] * gemm(ar, a, w['w1'].T, bias=w['b1'], relu=True)
        s2 = (s1 if fault == 'res2_from_s1' else a) + ks[3] * gemm(ar, f, w['w2'].T, bias=w['b2'])
        bn, xhat2, rstd2 = ln_fwd(ar, s2, w['ln2_g'], w['ln2_b'])
        if fault == 'no_last_norm2' and l == len(blocks) - 1:
            bn = s2
        tape['L'].append(dict(xhat1=xhat1, rstd1=rstd1, a=a, qkv=qkv, P=P, o=o, h1=s1, xhat2=xhat2, rstd2=rstd2, bn=bn, f=f))
        h = bn
    y = gemm(ar, h, cv(top['out_w']).T, bias=cv(top['out_b']))
    tape['hfin'], tape['y'] = h, y
    out = axpby(ar, residual, x, 1 - f32(residual), y)
    return out.reshape(B, T, D), tape


def postln_backward(ar, img, valid, top, blocks, heads, residual, tape, d_out, p=0.0, seed=0, fault=None):
    """-> (grads: (top dict, [layer dicts]), d_img, scratch dict as the FIRST layer leaves it: dy, dh = d h0, dh1 = d a
    (p > 0: d s1 through dropout1), dtmp_d = d o, dqkv, df).  fault: 'qkv_w_against_a' in_proj_weight's gradient taken
    against norm1's output instead of the layer's input."""
    B, T, D = img.shape
    R = B * T
    d, ffn = top['in_w'].shape[0], blocks[0]['w1'].shape[0]
    cv = lambda t: t.to(ar.dtype)     # noqa: E731
    x = cv(img).reshape(R, D)
    dy = axpby(ar, 1 - f32(residual), cv(d_out).reshape(R, D))
    gt = dict(out_w=gemm(ar, dy.T, tape['hfin']), out_b=colsum(ar, dy))
    dh = gemm(ar, dy, cv(top['out_w']))
    gl = [None] * len(blocks)
    sc = {}
    for l in range(len(blocks) - 1, -1, -1):
        w = {k: cv(v) for k, v in blocks[l].items()}
        t = tape['L'][l]
        hin = tape['L'][l - 1]['bn'] if l else tape['h0']
        ks = [cv(k) for k in _keeps(seed, p, l, B, T, d, heads, ffn)]
        g = dict(ln2_g=colsum(ar, dh, t['xhat2']), ln2_b=colsum(ar, dh))
        ds2 = ln_bwd(ar, dh, t['xhat2'], t['rstd2'], w['ln2_g'])
        dlin2 = ds2 * ks[3]
        g.update(w2=gemm(ar, dlin2.T, t['f']), b2=colsum(ar, dlin2))
        df = gemm(ar, dlin2, w['w2'])
        df = torch.where(t['f'] > 0, df * ar.t(keep_scale(p) if p > 0 else 1.0), torch.zeros_like(df))
        g.update(w1=gemm(ar, df.T, t['a']), b1=colsum(ar, df))
        da = gemm(ar, df, w['w1'], beta=1.0, C0=ds2)
        g.update(ln1_g=colsum(ar, da, t['xhat1']), ln1_b=colsum(ar, da))
        ds1 = ln_bwd(ar, da, t['xhat1'], t['rstd1'], w['ln1_g'])
        dlo = ds1 * ks[1]
        g.update(o_w=gemm(ar, dlo.T, t['o']), o_b=colsum(ar, dlo))
        dO = gemm(ar, dlo, w['o_w'])
        dqkv = attn_bwd(ar, t['qkv'].reshape(B, T, 3 * d), t['P'], dO.reshape(B, T, d), heads,
                        ks[0] if p > 0 else None).reshape(R, 3 * d)
        g.update(qkv_w=gemm(ar, dqkv.T, t['a'] if fault == 'qkv_w_against_a' else hin), qkv_b=colsum(ar, dqkv))
        dh = gemm(ar, dqkv, w['qkv_w'], beta=1.0, C0=ds1)
        gl[l] = g
        sc = dict(dy=dy, dh=dh, dh1=dlo if p > 0 else da, dtmp_d=dO, dqkv=dqkv, df=df)
    gt.update(in_w=gemm(ar, dh.T, x), in_b=colsum(ar, dh))
    C0 = axpby(ar, residual, cv(d_out).reshape(R, D))
    d_img = gemm(ar, dh, cv(top['in_w']), beta=1.0, C0=C0)
    return (gt, gl), d_img.reshape(B, T, D), sc


# ---------------------------------------------------------------------------------------------------------------
# stage by stage: every slot against ONE float64 stage applied to the implementation's own previous slot
# ---------------------------------------------------------------------------------------------------------------
def check_postln_forward(img, valid, top, blocks, heads, residual, p, seed, out, tape, what):
    """A layer's input is kept (h0, the previous layer's bn), so only norm2's input has to be restated, from a and f, with
    its bound carried into norm2's three outputs.  hfin is the last bn, bit for bit.  -> {group: worst error / bound}."""
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
    h = dd(tape['h0'])
    for l, bp in enumerate(blocks):
        w = {k: dd(v) for k, v in bp.items()}
        t = {k: dd(v) for k, v in tape['L'][l].items()}
        g = tape['L'][l]
        ks = _keeps(seed, p, l, B, T, d, heads, ffn)
        nm = lambda s: dict(name=f'layer {l} {s}')     # noqa: E731
        S, _ = gemm_S(h, w['qkv_w'].T, bias=w['qkv_b'])
        rec('gemm', g['qkv'], gemm(A64, h, w['qkv_w'].T, bias=w['qkv_b']), ('gemm', d), S, **nm('qkv'))
        k0 = ks[0] if p > 0 else None
        q3 = t['qkv'].reshape(B, T, 3 * d)
        P, _ = attn_fwd(A64, q3, valid, heads, k0)
        Sa = attn_fwd_S(q3, valid, heads, k0)
        rec('attn_fwd', g['P'], P, 'attn_fwd', *Sa['P'], **nm('P'))
        Pd = t['P'] if k0 is None else t['P'] * k0
        vh = _heads(q3[..., 2 * d:], heads)
        rec('attn_fwd', g['o'], (Pd @ vh).transpose(1, 2).reshape(R, d), 'attn_fwd',
            (2 * Pd @ vh.abs()).transpose(1, 2).reshape(R, d), **nm('o'))
        lin = gemm(A64, t['o'], w['o_w'].T, bias=w['o_b'])
        S, _ = gemm_S(t['o'], w['o_w'].T, bias=w['o_b'])
        rec('gemm', g['h1'], h + ks[1] * lin, ('gemm', d), h.abs() + ks[1] * S + (h + ks[1] * lin).abs(), **nm('h1 (s1)'))
        y, xhat, rstd = ln_fwd(A64, t['h1'], w['ln1_g'], w['ln1_b'])
        Sl = ln_fwd_S(t['h1'], w['ln1_g'], w['ln1_b'])
        for k_, ref_, s_ in (('a', y, 'y'), ('xhat1', xhat, 'xhat'), ('rstd1', rstd, 'rstd')):
            rec('ln_fwd', g[k_], ref_, 'ln_fwd', *Sl[s_], **nm(k_))
        S, _ = gemm_S(t['a'], w['w1'].T, bias=w['b1'])
        rec('gemm', g['f'], ks[2] * gemm(A64, t['a'], w['w1'].T, bias=w['b1'], relu=True), ('gemm', d), 2 * ks[2] * S, **nm('f'))
        lin = gemm(A64, t['f'], w['w2'].T, bias=w['b2'])
        S, _ = gemm_S(t['f'], w['w2'].T, bias=w['b2'])
        s2 = t['a'] + ks[3] * lin                                    # norm2's input, restated: the slot is not kept
        es2 = bound(('gemm', ffn), t['a'].abs() + ks[3] * S + s2.abs())
        y, xhat, rstd = ln_fwd(A64, s2, w['ln2_g'], w['ln2_b'])
        Sl = ln_fwd_S(s2, w['ln2_g'], w['ln2_b'], es2)
        for k_, ref_, s_ in (('bn', y, 'y'), ('xhat2', xhat, 'xhat'), ('rstd2', rstd, 'rstd')):
            rec('ln_fwd', g[k_], ref_, 'ln_fwd', *Sl[s_], pure=False, **nm(k_))
        h = t['bn']
    assert torch.equal(tape['hfin'].double(), h), f'{what}: hfin is not the last norm2 output'
    S, _ = gemm_S(h, W['out_w'].T, bias=W['out_b'])
    rec('gemm', tape['y'], gemm(A64, h, W['out_w'].T, bias=W['out_b']), ('gemm', d), S, name='y')
    yk = dd(tape['y'])
    rec('elementwise', out.reshape(R, D), axpby(A64, residual, x, 1 - f32(residual), yk), 'elementwise',
        axpby_S(residual, x, 1 - f32(residual), yk), name='out')
    return worst


def check_postln_backward(img, valid, top, blocks, heads, residual, p, seed, tape, d_out, grads, d_img, scr, what):
    """layers = 1.  The scratch slots the layer leaves, every parameter gradient and d_img against ONE float64 stage applied
    to the implementation's own slots; a stage's input that was overwritten (d bn, d s2, d s1; with dropout d a) is restated
    once from the slot before it and its bound carried.  -> {group: worst}."""
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
    h0 = dd(tape['h0'])
    gt, gl = grads
    ks = _keeps(seed, p, 0, B, T, d, heads, ffn)
    kscale = keep_scale(p) if p > 0 else 1.0
    worst = {}

    def rec(group, name, got, ref, key, S, E=0.0):
        pure = not torch.is_tensor(E)
        worst[group] = max(worst.get(group, 0.0), within(got, ref, key, S, E, f'{what}: {name}', pure))

    def lin_grads(name_w, name_b, dyv, xin, e=None, gw=None, gb=None):
        S, E = gemm_S(dyv.T, xin, eA=None if e is None else e.T)
        rec('gemm', name_w, gw, dyv.T @ xin, ('gemm', R), S, E)
        S, E = colsum_S(dyv, eX=e)
        rec('colsum', name_b, gb, dyv.sum(0), 'colsum', S, E)

    def ln_params(name, dyv, xhat, e, gg, gb):
        for nm_, Y, got in ((f'd {name}_g', xhat, gg), (f'd {name}_b', None, gb)):
            S, E = colsum_S(dyv, Y, eX=e)
            rec('colsum', nm_, got, (dyv * (1.0 if Y is None else Y)).sum(0), 'colsum', 2 * S, E)
    rec('elementwise', 'dy', scr['dy'], axpby(A64, 1 - f32(residual), do), 'elementwise', axpby_S(1 - f32(residual), do))
    dy, hf = s['dy'], dd(tape['hfin'])
    lin_grads('d out_w', 'd out_b', dy, hf, gw=gt['out_w'], gb=gt['out_b'])
    dbn = dy @ W['out_w']                                          # restated: the slot ends as d h0
    S, _ = gemm_S(dy, W['out_w'])
    e0 = bound(('gemm', D), S)
    ln_params('ln2', dbn, t['xhat2'], e0, gl[0]['ln2_g'], gl[0]['ln2_b'])
    ds2 = ln_bwd(A64, dbn, t['xhat2'], t['rstd2'], w['ln2_g'])     # restated: d a is accumulated onto it
    S, E = ln_bwd_S(dbn, t['xhat2'], t['rstd2'], w['ln2_g'], edy=e0)
    es2 = bound('ln_bwd', S, E)
    dlin2, e2 = ds2 * ks[3], es2 * ks[3] + bound('elementwise', (ds2 * ks[3]).abs()) * (p > 0)
    lin_grads('d w2', 'd b2', dlin2, t['f'], e2, gw=gl[0]['w2'], gb=gl[0]['b2'])
    S, E = gemm_S(dlin2, w['w2'], eA=e2)
    on = (t['f'] > 0).double() * kscale
    rec('gemm', 'df', scr['df'], (dlin2 @ w['w2']) * on, ('gemm', d), 2 * S * on, E * on)
    df = s['df']
    lin_grads('d w1', 'd b1', df, t['a'], gw=gl[0]['w1'], gb=gl[0]['b1'])
    da = df @ w['w1'] + ds2                                         # d a = d f W1 + d s2, the second residual
    S, _ = gemm_S(df, w['w1'], beta=1.0, C0=ds2)
    ea = bound(('gemm', ffn), S, es2)
    if p == 0:
        rec('gemm', 'dh1 (d a)', scr['dh1'], da, ('gemm', ffn), S, es2)
        da, ea = s['dh1'], None
    ln_params('ln1', da, t['xhat1'], ea, gl[0]['ln1_g'], gl[0]['ln1_b'])
    ds1 = ln_bwd(A64, da, t['xhat1'], t['rstd1'], w['ln1_g'])      # restated: d qkv Wqkv is accumulated onto it
    S, E = ln_bwd_S(da, t['xhat1'], t['rstd1'], w['ln1_g'], edy=ea)
    es1 = bound('ln_bwd', S, E)
    dlo, elo = ds1 * ks[1], es1 * ks[1]
    if p > 0:
        rec('elementwise', 'dh1 (d s1 through dropout1)', scr['dh1'], dlo, 'elementwise', dlo.abs(), elo)
        dlo, elo = s['dh1'], None
    lin_grads('d o_w', 'd o_b', dlo, t['o'], elo, gw=gl[0]['o_w'], gb=gl[0]['o_b'])
    S, E = gemm_S(dlo, w['o_w'], eA=elo)
    rec('gemm', 'dtmp_d (d o)', scr['dtmp_d'], dlo @ w['o_w'], ('gemm', d), S, E)
    dO = s['dtmp_d']
    k0 = ks[0] if p > 0 else None
    q3 = t['qkv'].reshape(B, T, 3 * d)
    S, E = attn_bwd_S(q3, t['P'], dO.reshape(B, T, d), heads, k0)
    rec('attn_bwd', 'dqkv', scr['dqkv'].reshape(B, T, 3 * d), attn_bwd(A64, q3, t['P'], dO.reshape(B, T, d), heads, k0),
        'attn_bwd', S, E)
    dq = s['dqkv']
    lin_grads('d qkv_w (against the layer input)', 'd qkv_b', dq, h0, gw=gl[0]['qkv_w'], gb=gl[0]['qkv_b'])
    S, _ = gemm_S(dq, w['qkv_w'], beta=1.0, C0=ds1)
    rec('gemm', 'dh (d h0)', scr['dh'], dq @ w['qkv_w'] + ds1, ('gemm', 3 * d), S, es1)
    dh = s['dh']
    lin_grads('d in_w', 'd in_b', dh, x, gw=gt['in_w'], gb=gt['in_b'])
    C0 = axpby(fr.A32, residual, d_out.reshape(R, D)).double()
    S, _ = gemm_S(dh, W['in_w'], beta=1.0, C0=C0)
    rec('gemm', 'd_img', d_img.reshape(R, D), dh @ W['in_w'] + C0, ('gemm', d), S)
    return worst


# ---------------------------------------------------------------------------------------------------------------
# torch's own float64 module (the yardstick of the end-to-end tests) and the loss head with max, in float64 autograd
# ---------------------------------------------------------------------------------------------------------------
NAMES = dict(ln1_g='norm1.weight', ln1_b='norm1.bias', qkv_w='self_attn.in_proj_weight', qkv_b='self_attn.in_proj_bias',
             o_w='self_attn.out_proj.weight', o_b='self_attn.out_proj.bias', ln2_g='norm2.weight', ln2_b='norm2.bias',
             w1='linear1.weight', b1='linear1.bias', w2='linear2.weight', b2='linear2.bias')
TOP_NAMES = dict(in_w='in_proj.weight', in_b='in_proj.bias', out_w='out_proj.weight', out_b='out_proj.bias')


def state_dict_of(top, blocks):
    """{state-dict key of TransformerAdapter: tensor} of fewshot_ref.adapter_params' dicts."""
    sd = {f'transformer_encoder.layers.{l}.{NAMES[k]}': v for l, bp in enumerate(blocks) for k, v in bp.items()}
    sd.update({TOP_NAMES[k]: v for k, v in top.items()})
    return sd


def named_grads(grads):
    """(top dict, [layer dicts]) -> {state-dict key: gradient}"""
    gt, gl = grads
    return state_dict_of(gt, gl)


def torch_adapter(top, blocks, heads, norm_first, img, valid, residual, dtype=F64):
    """torch's nn.TransformerEncoder (dropout 0, no nested tensors) around in_proj / out_proj and the residual mix ->
    (out [B, T, D] with autograd, {state-dict key: leaf parameter}, the leaf input)."""
    d, ffn = top['in_w'].shape[0], blocks[0]['w1'].shape[0]
    layer = torch.nn.TransformerEncoderLayer(d, heads, ffn, dropout=0.0, batch_first=True, norm_first=norm_first, dtype=dtype)
    enc = torch.nn.TransformerEncoder(layer, len(blocks), enable_nested_tensor=False)
    enc.load_state_dict({k[len('transformer_encoder.'):]: v.to(dtype) for k, v in state_dict_of({}, blocks).items()})
    enc.train()                      # with dropout 0: the math path, never the fused inference kernel
    P = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state_dict_of(top, []).items()}
    P.update({'transformer_encoder.' + k: v for k, v in enc.named_parameters()})
    x = img.to(dtype).clone().requires_grad_(True)
    h = torch.nn.functional.linear(x, P['in_proj.weight'], P['in_proj.bias'])
    h = enc(h, src_key_padding_mask=~valid)
    y = torch.nn.functional.linear(h, P['out_proj.weight'], P['out_proj.bias'])
    r = f32(residual)
    return x * r + y * (1 - r), P, x


def head64(feats, valid, labels, text, scale, agg, probs_loss):
    """The reference's classifier tail and train loss (clip_cls.py:104-129, :164-175, :325-343) in torch, differentiable:
    feats [B, T, D], text [K, D] -> (loss, aggregated logits [B, K], full logits [B, T, K]).  max is
    (logits - (1 - valid) * 1e6).max over the views."""
    vm = valid.to(feats.dtype)
    fn = torch.nn.functional.normalize(feats, dim=-1) * vm[..., None]
    full = scale * fn @ torch.nn.functional.normalize(text, dim=-1).T
    nv = vm.sum(1, keepdim=True)
    if agg == 'max':
        logits = (full - (1 - vm)[..., None] * 1e6).max(1).values
    else:
        logits = full.sum(1) / (nv if agg == 'mean' else 1.0)
    if probs_loss:
        pr = (torch.softmax(full, -1) * vm[..., None]).sum(1) / nv
        loss = torch.nn.functional.nll_loss(torch.log(pr + 1e-6), labels)
    else:
        loss = torch.nn.functional.cross_entropy(logits, labels)
    return loss, logits, full


def view_gap(full, valid):
    """The smallest distance, over every (sample, class), between the two largest logits among the valid views (inf where a
    sample has one valid view): what keeps an fp32 forward from picking another maximal view than float64."""
    l = full.double().masked_fill(~valid[..., None], float('-inf'))
    if l.shape[1] < 2:
        return float('inf')
    top2 = l.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    return float(gap[torch.isfinite(gap)].min()) if torch.isfinite(gap).any() else float('inf')


def max_inputs(B, T, D, K, seed):
    """feats fp32 [B, T, D] with ZERO rows on invalid views, valid (view 0 always, the last sample only view 0), labels,
    text fp32 [K, D]; views lean towards their class row, lightly: some samples stay misclassified, so the loss and its
    gradients are of ordinary size."""
    g = fr._gen(4000 + seed)
    text = (fr._randn(g, K, D) * 0.5).float()
    labels = (torch.arange(B) % K).long()
    feats = (fr._randn(g, B, T, D) + 0.3 * text[labels][:, None]).float()
    valid = torch.rand(B, T, generator=g) < 0.7
    valid[:, 0] = True
    valid[B - 1, 1:] = False
    return (feats * valid[..., None]).contiguous(), valid, labels, text


def max_case(i, layout):
    """Shape i of MAX_SHAPES at its committed seed, layout None (identity adapter), 'pre' or 'post' -> dict(feats, valid,
    labels, text, top, blocks, heads, residual)."""
    B, T, D, K, d, heads, ffn, layers = MAX_SHAPES[i]
    feats, valid, labels, text = max_inputs(B, T, D, K, MAX_SEEDS[i])
    top, blocks = fr.adapter_params(D, d, heads, ffn, layers, seed=i)
    return dict(feats=feats, valid=valid, labels=labels, text=text, top=top, blocks=blocks, heads=heads, residual=0.5)


def max_yardstick(c, layout, agg, probs_loss):
    """float64 autograd of a case -> dict(loss, logits, full, gap, grads {name: tensor, 'text_feats', 'feats'})."""
    text = c['text'].double().clone().requires_grad_(True)
    if layout is None:
        x = c['feats'].double().clone().requires_grad_(True)
        mixed, P = x, {}
    else:
        mixed, P, x = torch_adapter(c['top'], c['blocks'], c['heads'], layout == 'pre', c['feats'], c['valid'], c['residual'])
    loss, logits, full = head64(mixed, c['valid'], c['labels'], text, LOGIT_SCALE, agg, probs_loss)
    loss.backward()
    grads = {k: v.grad.detach() for k, v in P.items()}
    grads['text_feats'] = text.grad.detach()
    return dict(loss=loss.detach(), logits=logits.detach(), full=full.detach(), gap=view_gap(full.detach(), c['valid']),
                grads=grads, d_feats=x.grad.detach())


def check_max_head(full, valid, d_logits, dL, what):
    """dL [B, T, K]: the per-view logit gradient a max head produced for the upstream gradient d_logits [B, K] of its
    aggregated logits, on full logits [B, T, K] whose gap is at least MIN_GAP: exactly d_logits on the maximal VALID view of
    each (sample, class) -- compared within fp32 rounding of d_logits -- and an exact zero on every other view."""
    assert view_gap(full, valid) >= MIN_GAP, f'{what}: near tie, gap {view_gap(full, valid)}'
    l = full.double().masked_fill(~valid[..., None], float('-inf'))
    win = torch.nn.functional.one_hot(l.argmax(1), full.shape[1]).transpose(1, 2).bool()       # [B, T, K]
    dL = dL.double()
    assert not bool(dL[~valid].any()), f'{what}: a padded view got a gradient'
    assert not bool(dL[~win].any()), f'{what}: a view that is not the maximum got a gradient'
    got = (dL * win).sum(1)
    err = (got - d_logits.double()).abs()
    lim = GRAD_TOL * float(d_logits.abs().max())
    assert float(err.max()) <= lim, f'{what}: the maximal view got {float(err.max()):.3e} off d_logits (limit {lim:.3e})'
    return float(err.max()) / max(lim, 1e-300)
