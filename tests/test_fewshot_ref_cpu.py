"""tests/fewshot_ref.py on the CPU: its float64 yardsticks are the operations (torch's own float64 modules, losses, optimiser
and autograd agree to ~1e-12), its constants are what the fp32 restatements lose against them over the whole shape tables
(measured <= figure <= 1.5 measured), and every check the GPU tests run rejects an fp32 model with one planted fault."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fewshot_ref as fr  # noqa: E402

A32, A64 = fr.A32, fr.A64
SEED = 987654321
E2E = fr.E2E_CASES


# ---------------------------------------------------------------------------------------------------------------
# the F32 models behind the checks' interfaces, with their planted faults
# ---------------------------------------------------------------------------------------------------------------
def head_model(mean_over_T=False):
    def impl(feats, valid, labels, text, scale, agg, probs, grad_scale=None):
        r = fr.text_head(A32, feats, valid, labels, text, scale, agg, probs, mean_over_T=mean_over_T, grad_scale=grad_scale or 1.0)
        return (r['loss'], r['grad_text'], r['agg_logits']) + ((r['d_feats'],) if grad_scale else ())
    return impl


def adam_model(cap=None):
    return lambda p, g, m, v, *hp: fr.adam(A32, p, g, m, v, *hp, cap=cap)


def dz_model(**fault):
    def impl(full, ok, agg, d_full, d_logits, d_probs):
        return fr.classify_dz(A32, full, ok, agg, d_full, d_logits, d_probs, **fault)
    return impl


def dropout_model(site_shift=0, cap=None):
    def impl(seed, site, n, p):
        k = fr.drop_keep(seed, site + site_shift, n, p)
        if cap is not None:
            k[cap:] = False
        return k
    return impl


def run_adapter(case, fwd_fault=None, colsum_tail_fault=False, ar=A32):
    """One adapter case through the model and both stage checks -> {group: worst}"""
    B, T, (D, d, heads, ffn), layers, p, r = case
    top, blocks = fr.adapter_params(D, d, heads, ffn, layers)
    img, valid, d_out = fr.adapter_inputs(B, T, D)
    out, tape = fr.adapter_forward(ar, img, valid, top, blocks, heads, r, p, SEED, fault=fwd_fault)
    w = fr.check_adapter_forward(img, valid, top, blocks, heads, r, p, SEED, out, tape, f'adapter {case}')
    if layers == 1:
        grads, d_img, scr = fr.adapter_backward(ar, img, valid, top, blocks, heads, r, tape, d_out, p, SEED,
                                                colsum_tail_fault=colsum_tail_fault)
        wb = fr.check_adapter_backward(img, valid, top, blocks, heads, r, p, SEED, tape, d_out, grads, d_img, scr,
                                       f'adapter backward {case}')
        for k, v in wb.items():
            w[k] = max(w.get(k, 0.0), v)
        # the attention backward alone on exact inputs (in the chain its d o is a restated intermediate)
        t0, dO = tape['L'][0], fr.plane(B * T, d, 3).reshape(B, T, d)
        q3, k0 = t0['qkv'].reshape(B, T, 3 * d), (fr.keep_matrix(SEED, 0, (B, heads, T, T), p) if p > 0 else None)
        want = fr.attn_bwd(A64, q3.double(), t0['P'].double(), dO.double(), heads, k0)
        fr.within(fr.attn_bwd(ar, q3, t0['P'], dO.to(ar.dtype), heads, k0), want, 'attn_bwd',
                  fr.attn_bwd_S(q3, t0['P'], dO, heads, k0)[0], 0.0, f'attention backward {case}')
    return w


def run_e2e(layers, shape, p, r, ar=A32):
    B, T, (D, d, heads, ffn) = shape
    top, blocks = fr.adapter_params(D, d, heads, ffn, layers)
    img, valid, d_out = fr.adapter_inputs(B, T, D)
    S = {}
    _, tape = fr.adapter_forward(A64, img, valid, top, blocks, heads, r, p, SEED)
    g64, di64, _ = fr.adapter_backward(A64, img, valid, top, blocks, heads, r, tape, d_out, p, SEED, S=S)
    _, tape32 = fr.adapter_forward(ar, img, valid, top, blocks, heads, r, p, SEED)
    g32, di32, _ = fr.adapter_backward(ar, img, valid, top, blocks, heads, r, tape32, d_out, p, SEED)
    return fr.check_grads_end_to_end(fr.flat_grads(g32, di32), fr.flat_grads(g64, di64), S, layers, f'e2e layers={layers}')


def run_all_checks():
    """Every check of the GPU tests on the F32 restatements, over the whole shape tables."""
    gm = fr.gemm_model()
    for c in fr.gemm_cases():
        fr.check_gemm(gm, fr.gemm_case(*c), f'gemm {c}')
    for c in fr.head_cases():
        fr.check_head(head_model(), c, 'head', grad_scale=fr.GRAD_SCALE)
    fr.check_head(head_model(), (3, 2, 64, 5, 'mean', True, 0), 'head saturated', saturated=True, grad_scale=fr.GRAD_SCALE)
    fr.check_head(head_model(), (3, 2, 64, 5, 'sum', False, 1), 'head saturated', saturated=True, grad_scale=fr.GRAD_SCALE)
    for c in fr.adam_cases():
        fr.check_adam(adam_model(), c, 'adam')
    for K in fr.DZ_K:
        for T in fr.DZ_T:
            for agg in fr.AGG:
                fr.check_dz_random(dz_model(), K, T, agg, f'dz K={K} T={T} {agg}')
    for c in fr.adapter_cases():
        run_adapter(c)
    for layers, shape, p, r in E2E:
        run_e2e(layers, shape, p, r)
    big = fr.BIG_DROPOUT
    run_e2e(1, (big['B'], big['T'], big['geom']), big['p'], big['residual'])


@pytest.fixture(scope='module')
def measured():
    fr.MEASURE = {}
    try:
        run_all_checks()
        return dict(fr.MEASURE)
    finally:
        fr.MEASURE = None


@pytest.mark.parametrize('name', sorted(fr.C))
def test_constant_is_what_the_restatement_loses(name, measured):
    m = measured[name]
    print(f'{name}: measured {m:.3f}, figure {fr.C[name]}')
    assert m <= fr.C[name] <= 1.5 * m, (name, m, fr.C[name])


def test_tables_reach_every_edge():
    cs = fr.gemm_cases()
    for fam in ('exact', 'random'):
        assert {c[0] for c in cs if c[4] == fam} >= set(fr.GEMM_MN) and {c[1] for c in cs if c[4] == fam} >= set(fr.GEMM_MN)
        assert {c[2] for c in cs if c[4] == fam} >= set(fr.GEMM_K)
        for window in (False, True):
            assert {fr.strides_layout(fr.gemm_case(*c)) for c in cs if c[4] == fam and c[6] == window} == set(fr.LAYOUTS)
    eq = [fr.gemm_case(*c) for c in cs if c[10]]
    assert any(c['pa'][2] == c['pa'][3] for c in eq) and any(c['pb'][2] == c['pb'][3] for c in eq)
    assert any(c[8] == 0 for c in cs) and any(c[8] not in (0, 1) for c in cs) and any(c[7] not in (0, 1) for c in cs)
    assert any(c[9] > 0 for c in cs)
    hs = fr.head_cases()
    for i, vals in ((0, fr.HEAD_B), (1, fr.HEAD_T), (2, fr.HEAD_D), (3, fr.HEAD_K)):
        assert {c[i] for c in hs} >= set(vals)
    assert {(c[4], c[5], c[6]) for c in hs} == {(a, p, l) for a in ('sum', 'mean') for p in (False, True) for l in (0, 1)}
    ad = fr.adapter_cases()
    assert {c[0] * c[1] for c in ad} >= {1, 3, 4, 5, 28, 29, 32, 33, 36, 61, 64, 65}
    assert {c[2] for c in ad} == set(fr.GEOMETRIES) and {c[1] for c in ad} >= {15, 16}
    assert all(sum(1 for c in ad if c[2] == g) >= 2 for g in fr.GEOMETRIES)
    assert {c[4] for c in ad} == {0.0, 0.3} and {c[5] for c in ad} == {0.0, 0.8}
    img, valid, _ = fr.adapter_inputs(4, 16, 50)
    assert valid[3].sum() == 1 and valid[3, 0] and bool(valid.any(1).all())          # only view 0 valid out of 16
    assert {c[0] for c in fr.adam_cases()} == set(fr.ADAM_N) and {c[1] for c in fr.adam_cases()} == set(fr.ADAM_STEPS)


def test_checks_accept_the_restatements():
    assert fr.MEASURE is None
    run_all_checks()
    assert fr.check_dropout(dropout_model()) > 20
    for K in fr.DZ_K:
        for T in fr.DZ_T:
            fr.check_dz_directed(dz_model(), K, T, f'dz directed K={K} T={T}')


# ---------------------------------------------------------------------------------------------------------------
# the yardsticks are the operations
# ---------------------------------------------------------------------------------------------------------------
def close(a, b, what, tol=1e-11):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol * max(1.0, float(b.abs().max()) if b.numel() else 1.0), (what, err)


class TorchAdapter(torch.nn.Module):
    def __init__(self, D, d, heads, ffn, layers):
        super().__init__()
        self.in_proj, self.out_proj = torch.nn.Linear(D, d), torch.nn.Linear(d, D)
        self.layers = torch.nn.ModuleList(torch.nn.TransformerEncoderLayer(d, heads, ffn, dropout=0.1, activation='relu',
                                                                           batch_first=True, norm_first=True)
                                          for _ in range(layers))

    def load(self, top, blocks):
        names = dict(ln1_g='norm1.weight', ln1_b='norm1.bias', qkv_w='self_attn.in_proj_weight', qkv_b='self_attn.in_proj_bias',
                     o_w='self_attn.out_proj.weight', o_b='self_attn.out_proj.bias', ln2_g='norm2.weight', ln2_b='norm2.bias',
                     w1='linear1.weight', b1='linear1.bias', w2='linear2.weight', b2='linear2.bias')
        sd = {'in_proj.weight': top['in_w'], 'in_proj.bias': top['in_b'], 'out_proj.weight': top['out_w'],
              'out_proj.bias': top['out_b']}
        for l, b in enumerate(blocks):
            sd.update({f'layers.{l}.{names[k]}': v for k, v in b.items()})
        self.load_state_dict(sd)
        self.names = names
        return self.double().eval()

    def forward(self, x, valid, r):
        h = self.in_proj(x)
        for layer in self.layers:
            h = layer(h, src_key_padding_mask=~valid)
        return fr.f32(r) * x + (1 - fr.f32(r)) * self.out_proj(h)


@pytest.mark.parametrize('layers,shape,r', [(1, (3, 5, fr.GEOMETRIES[0]), 0.8), (2, (2, 16, fr.GEOMETRIES[2]), 0.0),
                                            (8, (3, 4, fr.GEOMETRIES[1]), 0.8)])
def test_adapter_yardstick_is_the_torch_module(layers, shape, r):
    B, T, (D, d, heads, ffn) = shape
    top, blocks = fr.adapter_params(D, d, heads, ffn, layers)
    img, valid, d_out = fr.adapter_inputs(B, T, D)
    mod = TorchAdapter(D, d, heads, ffn, layers).load(top, blocks)
    x = img.double().requires_grad_(True)
    out_t = mod(x, valid, r)
    (out_t * d_out.double()).sum().backward()
    out, tape = fr.adapter_forward(A64, img, valid, top, blocks, heads, r)
    close(out, out_t.detach(), 'out')
    (gt, gl), d_img, _ = fr.adapter_backward(A64, img, valid, top, blocks, heads, r, tape, d_out)
    close(d_img, x.grad, 'd_img')
    sd = dict(mod.named_parameters())
    for k, n in (('in_w', 'in_proj.weight'), ('in_b', 'in_proj.bias'), ('out_w', 'out_proj.weight'), ('out_b', 'out_proj.bias')):
        close(gt[k], sd[n].grad, k)
    for l in range(layers):
        for k, n in mod.names.items():
            close(gl[l][k], sd[f'layers.{l}.{n}'].grad, f'{l}.{k}')


def test_stage_yardsticks_are_torch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 40, generator=g, dtype=torch.float64, requires_grad=True)
    gam, bet, dy = (torch.randn(40, generator=g, dtype=torch.float64) for _ in range(3))
    dyf = torch.randn(7, 40, generator=g, dtype=torch.float64)
    y_t = torch.nn.functional.layer_norm(x, (40,), gam, bet, 1e-5)
    y_t.backward(dyf)
    y, xhat, rstd = fr.ln_fwd(A64, x.detach(), gam, bet)
    close(y, y_t.detach(), 'ln y')
    close(fr.ln_bwd(A64, dyf, xhat, rstd, gam), x.grad, 'ln dx')
    close(fr.ln_bwd(A64, dyf, xhat, rstd, gam, dx0=dyf), x.grad + dyf, 'ln dx accumulate')
    close(fr.colsum(A64, dyf, xhat), (dyf * xhat).sum(0), 'colsum')
    # nn.MultiheadAttention with a keep-scale matrix: dropout on the attention weights is P * ks
    B, T, d, heads = 3, 6, 24, 4
    mha = torch.nn.MultiheadAttention(d, heads, batch_first=True).double().eval()
    a = torch.randn(B, T, d, generator=g, dtype=torch.float64)
    valid = torch.rand(B, T, generator=g) < 0.6
    valid[:, 0] = True
    with torch.no_grad():
        mha.out_proj.weight.copy_(torch.eye(d))
        mha.out_proj.bias.zero_()
        qkv = a @ mha.in_proj_weight.T + mha.in_proj_bias
        o_t, P_t = mha(a, a, a, key_padding_mask=~valid, average_attn_weights=False)
    P, o = fr.attn_fwd(A64, qkv, valid, heads)
    close(P, P_t, 'P')
    close(o, o_t, 'o')
    ks = fr.keep_matrix(5, 0, (B, heads, T, T), 0.3)
    q = qkv.clone().requires_grad_(True)
    P2, o2 = fr.attn_fwd(A64, q, valid, heads, ks)
    dO = torch.randn(B, T, d, generator=g, dtype=torch.float64)
    o2.backward(dO)
    close(fr.attn_bwd(A64, qkv, P2.detach(), dO, heads, ks), q.grad, 'dqkv (autograd of the yardstick forward)')
    # row normalisation
    m = torch.randn(9, 17, generator=g, dtype=torch.float64, requires_grad=True)
    ok = torch.tensor([1, 1, 0, 1, 0, 1, 1, 1, 1], dtype=torch.bool)
    fn_t = torch.nn.functional.normalize(m, dim=-1) * ok[:, None]
    dfn = torch.randn(9, 17, generator=g, dtype=torch.float64)
    fn_t.backward(dfn)
    fn, _ = fr.normalize_fwd(A64, m.detach(), ok)
    close(fn, fn_t.detach(), 'normalize')
    close(fr.normalize_bwd(A64, m.detach(), fn, dfn, ok, 0.25), 0.25 * m.grad, 'normalize backward')


@pytest.mark.parametrize('agg,probs', [('sum', False), ('mean', False), ('sum', True), ('mean', True)])
def test_head_yardstick_is_torch(agg, probs):
    B, T, D, K = 5, 4, 33, 7
    feats, valid, labels, text = fr.head_inputs(B, T, D, K, 1)
    t = text.double().requires_grad_(True)
    f = feats.double().requires_grad_(True)
    Fn = torch.nn.functional.normalize(f, dim=-1) * valid[..., None]
    L = 100.0 * Fn @ torch.nn.functional.normalize(t, dim=-1).T
    nv = valid.sum(1, keepdim=True).double()
    logits = L.sum(1) / (nv if agg == 'mean' else 1.0)
    if probs:
        pr = (torch.softmax(L, -1) * valid[..., None]).sum(1) / nv
        loss = torch.nn.functional.nll_loss(torch.log(pr + fr.f32(1e-6)), labels)      # the kernels' 1e-6f
    else:
        loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    r = fr.text_head(A64, feats.double(), valid, labels, text.double(), 100.0, agg, probs, grad_scale=fr.GRAD_SCALE)
    close(r['loss'], loss.detach(), 'loss')
    close(r['agg_logits'], logits.detach(), 'logits')
    close(r['grad_text'], t.grad, 'grad_text')
    assert not bool(valid.all()) and float(f.grad.abs().max()) > 0
    close(r['d_feats'], fr.GRAD_SCALE * f.grad, 'd_feats')


@pytest.mark.parametrize('agg', list(fr.AGG))
def test_dz_yardstick_is_torch_autograd(agg):
    g = torch.Generator().manual_seed(3)
    B, T, K = 4, 5, 9
    ok = torch.rand(B, T, generator=g) < 0.6
    ok[:, 0] = True
    full = (torch.randn(B, T, K, generator=g, dtype=torch.float64) * 3 * ok[..., None]).requires_grad_(True)
    d_full, gl, gp = (torch.randn(sh, generator=g, dtype=torch.float64) for sh in ((B, T, K), (B, K), (B, K)))
    okf = ok[..., None].double()
    nv = ok.sum(1).double()[:, None]
    masked = full * okf
    logits = masked.sum(1) if agg == 'sum' else masked.sum(1) / nv if agg == 'mean' else (masked - 1e6 * (1 - okf)).max(1).values
    pr = (torch.softmax(full, -1) * okf).sum(1) / nv
    ((masked * d_full).sum() + (logits * gl).sum() + (pr * gp).sum()).backward()
    close(fr.classify_dz(A64, full.detach(), ok, agg, d_full, gl, gp), full.grad * okf, 'dZ')


@pytest.mark.parametrize('wd,eps', [(0.0, 1e-8), (0.02, 1e-3)])
def test_adam_yardstick_is_torch_adam(wd, eps):
    p0, g, m, v = fr.adam_inputs(257, False)
    lr, b1, b2 = fr.f32(2e-3), fr.f32(0.9), fr.f32(0.98)
    ref = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=fr.f32(eps), weight_decay=fr.f32(wd))
    p, m, v = p0.double(), torch.zeros(257, dtype=torch.float64), torch.zeros(257, dtype=torch.float64)
    for step in range(1, 5):
        grad = g.double() * step
        ref.grad = grad.clone()
        opt.step()
        p, m, v = fr.adam(A64, p, grad, m, v, step, 2e-3, 0.9, 0.98, eps, wd)
        close(p, ref.data, f'p after step {step}')
    st = opt.state[ref]
    close(m, st['exp_avg'], 'm')
    close(v, st['exp_avg_sq'], 'v')


def test_dropout_hash_restatement():
    """The hash in Python integers (wrap-around by masking) gives the numpy uint64 bits; p = 0 keeps everything; the largest
    p below 1 keeps only draws of exactly 2^24 - 1."""
    M = fr.M64
    for seed, site in ((0, 0), (2 ** 64 - 1, 31), (2 ** 63 + 5, 1)):
        want = []
        for i in range(300):
            z = (seed + 0x9E3779B97F4A7C15 * (site + 1) + i * 0xD1B54A32D192ED03) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            want.append(np.float32(z >> 40) * np.float32(2.0 ** -24) >= np.float32(0.3))
        assert np.array_equal(fr.drop_keep(seed, site, 300, 0.3), np.array(want))
        assert np.array_equal(fr.drop_keep(seed, site, 100, 0.3, start=200), np.array(want[200:]))
    assert fr.drop_keep(7, 3, 100000, 0.0).all()
    assert abs(fr.drop_keep(7, 3, 100000, 0.3).mean() - 0.7) < 0.01
    assert fr.drop_keep(7, 3, 100000, fr.DROP_P[-1]).sum() <= 1


# ---------------------------------------------------------------------------------------------------------------
# every check rejects its planted fault
# ---------------------------------------------------------------------------------------------------------------
def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def gemm_rejects(fault, cases):
    m = fr.gemm_model(fault)
    return [c for c in cases if rejected(lambda: fr.check_gemm(m, fr.gemm_case(*c), 'planted'))]


def test_fault_k_tail_dropped():
    cases = fr.gemm_cases()
    bad = gemm_rejects('ktail', cases)
    # every case with a K tail is rejected unless its dropped products are all zero (K = 1 .. : zero rows only at M < 4)
    assert all(c[2] % 16 for c in bad)
    for fam in ('exact', 'random'):
        for K in (1, 3, 5, 15, 17, 31, 33, 100):
            assert any(c[2] == K and c[4] == fam and c[0] >= 31 for c in bad), (fam, K)


@pytest.mark.parametrize('layout', fr.LAYOUTS)
def test_fault_slab_transposed_in_one_layout(layout):
    cases = [c for c in fr.gemm_cases() if c[2] > 1 and c[0] > 1]
    bad = gemm_rejects(('slab', layout), cases)
    assert bad and all(fr.strides_layout(fr.gemm_case(*c)) == layout for c in bad)
    assert {c[6] for c in bad} == {False, True}, 'plain and window cases of the layout both reject it'


def test_fault_beta_c_read_at_beta_zero():
    cases = [c for c in fr.gemm_cases() if c[8] == 0.0][:40]
    assert len(gemm_rejects('beta0', cases)) == len(cases)


def test_fault_colsum_row_tail_skipped():
    for c in fr.adapter_cases():
        R = c[0] * c[1]
        if c[3] == 1 and c[2] == fr.GEOMETRIES[0]:
            assert rejected(lambda: run_adapter(c, colsum_tail_fault=True)) == (R % 32 != 0), c


def test_fault_mean_over_T():
    case = (3, 4, 8, 5, 'mean', False, 0)
    fr.check_head(head_model(), case, 'head')
    assert rejected(lambda: fr.check_head(head_model(mean_over_T=True), case, 'planted'))
    case = (3, 4, 8, 5, 'sum', True, 0)
    assert rejected(lambda: fr.check_head(head_model(mean_over_T=True), case, 'planted'))


def test_fault_tie_to_the_highest_index_and_offset_left_out():
    for K in fr.DZ_K:
        assert rejected(lambda: fr.check_dz_directed(dz_model(tie_high=True), K, 16, 'planted'))
        assert rejected(lambda: fr.check_dz_directed(dz_model(no_offset=True), K, 16, 'planted'))


def test_fault_second_grid_trip_missing():
    big = [c for c in fr.adam_cases() if c[0] > 2048 * 256]
    assert len(big) == 2
    for c in big:
        fr.check_adam(adam_model(), c, 'adam')
        assert rejected(lambda: fr.check_adam(adam_model(cap=2048 * 256), c, 'planted'))
    assert rejected(lambda: fr.check_dropout(dropout_model(cap=4096 * 256)))


def test_fault_mask_of_the_wrong_site():
    assert rejected(lambda: fr.check_dropout(dropout_model(site_shift=1)))
    case = (5, 13, fr.GEOMETRIES[0], 1, 0.3, 0.8)
    run_adapter(case)
    assert rejected(lambda: run_adapter(case, fwd_fault='site'))


@pytest.mark.parametrize('fault', ['rstd_eps', 'p_dropped'])
def test_fault_in_a_saved_activation(fault):
    case = (5, 13, fr.GEOMETRIES[0], 1, 0.3, 0.8)
    assert rejected(lambda: run_adapter(case, fwd_fault=fault))


# ---------------------------------------------------------------------------------------------------------------
# ec_adapter_train_layout (host code only: runs without a GPU)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,geom,layers', [(3, 5, fr.GEOMETRIES[0], 2), (1, 1, fr.GEOMETRIES[1], 1), (65, 16, (8, 8, 1, 1024), 8)])
def test_adapter_layout_is_the_carve(B, T, geom, layers):
    """The slots follow each other in the carve's order, each 256-byte aligned and as large as its tensor, and end at the
    size functions' byte counts."""
    import ctypes
    from eventclip_amd import _lib as L
    lib = L.lib()
    D, d, heads, ffn = geom
    R = B * T
    n = L.EC_AT_LAYER0 + L.EC_AT_PER_LAYER * layers
    assert lib.ec_adapter_train_layout(B, T, D, d, ffn, heads, layers, None, 0, None, 0) == n
    t_off, s_off = (ctypes.c_int64 * n)(), (ctypes.c_int64 * L.EC_AS_COUNT)()
    assert lib.ec_adapter_train_layout(B, T, D, d, ffn, heads, layers, t_off, n, s_off, L.EC_AS_COUNT) == n
    align = lambda x: (4 * x + 255) // 256 * 256     # noqa: E731
    sizes = [R * d, R * d, R * D, R * d] + [R * d, R, R * d, R * 3 * d, B * heads * T * T, R * d, R * d, R * d, R, R * d, R * ffn] * layers
    off = 0
    for i, sz in enumerate(sizes):
        assert t_off[i] == off, i
        off += align(sz)
    assert off == lib.ec_adapter_train_tape_bytes(B, T, D, d, ffn, heads, layers)
    off = 0
    for i, sz in enumerate([R * D, R * d, R * d, R * d, R * 3 * d, R * ffn]):
        assert s_off[i] == off, i
        off += align(sz)
    assert off == lib.ec_adapter_train_backward_workspace_bytes(B, T, D, d, ffn)
    assert lib.ec_adapter_train_layout(B, T, D, d, ffn, heads, 9, None, 0, None, 0) == L.EC_ERR_INVALID
    assert lib.ec_adapter_train_layout(B, T, D, d, ffn, heads, layers, t_off, n - 1, None, 0) == L.EC_ERR_INVALID
    assert lib.ec_adapter_train_layout(B, T, D, d, ffn, heads, layers, None, 0, s_off, L.EC_AS_COUNT - 1) == L.EC_ERR_INVALID
