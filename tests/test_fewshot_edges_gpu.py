"""The few-shot training kernels of csrc/train.hip at every loop, tile and launch edge, against float64 or bit-exact
expectations: tests/fewshot_ref.py holds the yardsticks, the directed inputs, the shape tables and the per-element bounds
(constants measured in tests/test_fewshot_ref_cpu.py, which also runs every check below against planted faults); the kernels
get KERNEL_FACTOR times the fp32 restatement's error.  The adapter is checked stage by stage through
ec_adapter_train_layout: every slot of the tape and of the backward's workspace against ONE float64 stage applied to the
kernels' own previous slot.  Every test prints the worst error / bound it saw."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fewshot_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = torch.float32
SEED = 2 ** 63 + 987654321


def _L():
    from eventclip_amd import _lib
    return _lib


def _report(name, worst):
    print(f'\n[fewshot edges] {name}: worst error / bound = {worst if isinstance(worst, dict) else round(worst, 4)}')


def _dev(t):
    """A CPU tensor on the GPU; an empty one becomes one element (the entry points refuse null pointers)."""
    return (t if t.numel() else torch.zeros(1, dtype=t.dtype)).contiguous().cuda()


def _pattern(shape, dtype=F32):
    """A device buffer of a NaN bit pattern that an untouched output must still hold."""
    return torch.full(shape, -0x12345679, dtype=torch.int32, device='cuda').view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == F32 else t


# ---------------------------------------------------------------------------------------------------------------
# (a) ec_sgemm
# ---------------------------------------------------------------------------------------------------------------
def _sgemm(ab, ao, sam, sak, bb, bo, sbk, sbn, M, N, K, alpha, beta, Cb):
    a, b, c = _dev(ab), _dev(bb), Cb.cuda()
    _L().launch('ec_sgemm', a.data_ptr() + 4 * ao, sam, sak, b.data_ptr() + 4 * bo, sbk, sbn, M, N, K, float(alpha), float(beta),
                c, c.shape[1])
    torch.cuda.synchronize()
    return c.cpu()


def _gemm_groups():
    cs = fr.gemm_cases()
    return [cs[i::8] for i in range(8)]


@pytest.mark.parametrize('group', range(8))
def test_sgemm_edges(group, hip):
    """Every M, N and K edge, the four slab layouts plain and as windows with both strides non-unit, equal strides, ldc > N
    with guards, beta == 0 over a NaN-filled C, alpha and beta off 0 and 1: the exact family bit for bit, the random /
    cancelling family under the bound; the same call again gives the same bits."""
    worst = 0.0
    for i, c in enumerate(_gemm_groups()[group]):
        case = fr.gemm_case(*c)
        worst = max(worst, fr.check_gemm(_sgemm, case, f'ec_sgemm {c}'))
        if i % 4 == 0:
            (ab, ao, sam, sak), (bb, bo, sbn, sbk) = case['pa'], case['pb']
            c0 = torch.full((c[0] + 1, c[1] + c[9]), 0.5)
            args = (ab, ao, sam, sak, bb, bo, sbk, sbn, c[0], c[1], c[2], c[7], c[8])
            assert torch.equal(_bits(_sgemm(*args, c0.clone())), _bits(_sgemm(*args, c0.clone()))), f'{c}: second call differs'
    _report(f'sgemm group {group}', worst)


# ---------------------------------------------------------------------------------------------------------------
# (b) the dropout hash
# ---------------------------------------------------------------------------------------------------------------
def test_dropout_hash_bits(hip):
    def impl(seed, site, n, p):
        m = torch.full((n + 64,), 7, dtype=torch.uint8, device='cuda')
        _L().launch('ec_dropout_mask', ctypes.c_uint64(seed), int(site), int(n), float(p), m)
        torch.cuda.synchronize()
        m = m.cpu().numpy()
        assert (m[n:] == 7).all(), 'ec_dropout_mask wrote past n'
        assert set(np.unique(m[:n])) <= {0, 1}
        return m[:n]
    n = fr.check_dropout(impl, 'ec_dropout_mask')
    _report(f'dropout hash ({n} cases, bit for bit)', 0.0)


# ---------------------------------------------------------------------------------------------------------------
# (c) ec_adam_step
# ---------------------------------------------------------------------------------------------------------------
def _adam(p, g, m, v, step, lr, b1, b2, eps, wd):
    n = p.numel()
    bufs = [torch.cat([x, torch.full((8,), float('nan'))]).cuda() for x in (p, g, m, v)]
    _L().launch('ec_adam_step', bufs[0], bufs[1], bufs[2], bufs[3], n, lr, b1, b2, eps, wd, int(step))
    torch.cuda.synchronize()
    out = [b.cpu() for b in bufs]
    assert all(torch.isnan(o[n:]).all() for o in out), 'ec_adam_step wrote past n'
    assert torch.equal(out[1][:n], g), 'ec_adam_step changed the gradient'
    return out[0][:n], out[2][:n], out[3][:n]


@pytest.mark.parametrize('case', fr.adam_cases(), ids=lambda c: f'n{c[0]}-s{c[1]}-wd{c[2]}-eps{c[3]}-{"dir" if c[4] else "rnd"}')
def test_adam_step(case, hip):
    _report(f'adam {case}', fr.check_adam(_adam, case, 'ec_adam_step'))


# ---------------------------------------------------------------------------------------------------------------
# (d) ec_fs_text_loss_grad
# ---------------------------------------------------------------------------------------------------------------
def _head_raw(feats, valid, labels, text, scale, agg, probs, expect_fail=False):
    B, T, D = feats.shape
    K = text.shape[0]
    lib = _L().lib()
    need = int(lib.ec_fs_text_train_workspace_bytes(B, T, D, K))
    ws = torch.empty(need + 256, dtype=torch.uint8, device='cuda')
    loss, grad, logits = _pattern((1,)), _pattern((K, D)), _pattern((B, K))
    f, v8, lab, t = feats.cuda(), valid.to(torch.uint8).cuda(), labels.to(torch.int32).cuda(), text.cuda()
    rc = lib.ec_fs_text_loss_grad(f.data_ptr(), v8.data_ptr(), lab.data_ptr(), t.data_ptr(), B, T, D, K, float(scale), fr.AGG[agg],
                                  int(probs), loss.data_ptr(), grad.data_ptr(), logits.data_ptr(), ws.data_ptr(), need,
                                  _L().stream_ptr())
    torch.cuda.synchronize()
    if expect_fail:
        return rc, loss.cpu(), grad.cpu()
    assert rc == 0, lib.ec_last_error()
    return loss.cpu(), grad.cpu(), logits.cpu()


def _head_groups():
    cs = fr.head_cases()
    return [cs[i::6] for i in range(6)]


@pytest.mark.parametrize('group', range(6))
def test_text_head_edges(group, hip):
    """K, T, B and D edges, both losses and aggregations, labels 0 and K - 1: loss, aggregated logits and d text per element."""
    worst = max(fr.check_head(_head_raw, c, 'ec_fs_text_loss_grad') for c in _head_groups()[group])
    _report(f'text head group {group}', worst)


@pytest.mark.parametrize('agg,probs', [('sum', False), ('mean', True)])
def test_text_head_ignores_invalid_views(agg, probs, hip):
    """NaN and Inf on invalid views change no bit of any output."""
    case = (5, 4, 65, 7, agg, probs, 1)
    feats, valid, labels, text = fr.head_inputs(*case[:4], case[6])
    assert not bool(valid.all())
    clean = _head_raw(torch.where(valid[..., None], feats, torch.zeros_like(feats)), valid, labels, text, 100.0, agg, probs)
    for poison in (float('nan'), float('inf'), -float('inf')):
        got = _head_raw(torch.where(valid[..., None], feats, torch.full_like(feats, poison)), valid, labels, text, 100.0, agg, probs)
        for name, a, b in zip(('loss', 'grad_text', 'agg_logits'), got, clean):
            assert torch.equal(_bits(a), _bits(b)), f'{name} changed with {poison} on invalid views'
        fr.check_head(_head_raw, case, 'poisoned', poison=poison)


@pytest.mark.parametrize('agg,probs', [('mean', True), ('sum', False)])
def test_text_head_saturated_sample(agg, probs, hip):
    """Every view of sample 0 exactly along its class row at logit_scale 100: finite and within the bound."""
    _report(f'text head saturated {agg} {probs}',
            fr.check_head(_head_raw, (3, 2, 64, 5, agg, probs, 0), 'saturated', saturated=True))


def test_text_head_lds_opt_in_and_limit(hip):
    """The loss kernel's dynamic LDS, (T K + 4 + 3 T) 4 bytes: K just below and just above the 64 KB opt-in and just below the
    160 KB limit, in the order small, above the opt-in, small, near the limit, small, below the opt-in -- each against
    float64; one K above the limit is refused with the LDS named and the outputs untouched."""
    B, D, T = 2, 8, 16
    lds = lambda K: (T * K + 4 + 3 * T) * 4     # noqa: E731
    k_opt = (64 * 1024 // 4 - 4 - 3 * T) // T
    k_max = (160 * 1024 // 4 - 4 - 3 * T) // T
    assert lds(k_opt) <= 64 * 1024 < lds(k_opt + 1) and lds(k_max) <= 160 * 1024 < lds(k_max + 1)
    worst = 0.0
    for i, K in enumerate((5, k_opt + 1, 5, k_max, 5, k_opt)):
        worst = max(worst, fr.check_head(_head_raw, (B, T, D, K, ('mean', 'sum')[i % 2], i % 4 != 1, i % 2), f'LDS K={K}'))
    feats, valid, labels, text = fr.head_inputs(B, T, D, k_max + 1, 0)
    rc, loss, grad = _head_raw(feats, valid, labels, text, 100.0, 'mean', True, expect_fail=True)
    assert rc != 0 and b'LDS' in _L().lib().ec_last_error()
    assert bool((_bits(loss) == -0x12345679).all()) and bool((_bits(grad) == -0x12345679).all())
    worst = max(worst, fr.check_head(_head_raw, (B, T, D, 5, 'mean', True, 0), 'after the refusal'))
    _report('text head LDS edges', worst)


# ---------------------------------------------------------------------------------------------------------------
# (d') ec_ft_loss_grad: the same head plus the feature gradient, dense or compact over the valid views
# ---------------------------------------------------------------------------------------------------------------
def _ft_head_raw(feats, valid, labels, text, scale, agg, probs, grad_scale, compact=False, scalars=False):
    """-> (loss [1], grad_text, agg_logits, grad_img) as CPU tensors.  compact: the valid views' rows alone, in REVERSED view
    order, with row_idx; grad_img comes back in that layout.  scalars: grad_scale travels in a device step_scalars array
    (every other entry NaN) and the by-value argument holds another value."""
    B, T, D = feats.shape
    K = text.shape[0]
    L = _L()
    lib = L.lib()
    need = int(lib.ec_fs_text_train_workspace_bytes(B, T, D, K)) + max(B * T, K) * D * 4
    ws = torch.empty(need + 256, dtype=torch.uint8, device='cuda')
    f, row_idx = feats, None
    if compact:
        okf = valid.reshape(-1)
        n = int(okf.sum())
        row_idx = torch.where(okf, n - torch.cumsum(okf.int(), 0), torch.full((B * T,), -1)).to(torch.int32).cuda()
        f = feats.reshape(B * T, D)[okf].flip(0)
    step = None
    if scalars:
        step = torch.full((L.EC_STEP_COUNT,), float('nan'))
        step[L.EC_STEP_GRAD_SCALE] = grad_scale
        step = step.cuda()
    rows = f.numel() // D
    loss, grad, logits, gimg = _pattern((1,)), _pattern((K, D)), _pattern((B, K)), _pattern((rows + 1, D))
    f, v8, lab, t = f.contiguous().cuda(), valid.to(torch.uint8).cuda(), labels.to(torch.int32).cuda(), text.cuda()
    rc = lib.ec_ft_loss_grad(f.data_ptr(), row_idx.data_ptr() if compact else None, v8.data_ptr(), lab.data_ptr(), t.data_ptr(),
                             B, T, D, K, float(scale), fr.AGG[agg], int(probs), -7.0 if scalars else float(grad_scale),
                             step.data_ptr() if scalars else None, loss.data_ptr(), grad.data_ptr(), gimg.data_ptr(),
                             logits.data_ptr(), ws.data_ptr(), need, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.ec_last_error()
    assert bool((_bits(gimg[rows]) == -0x12345679).all()), 'ec_ft_loss_grad wrote past the last feature row'
    return loss.cpu(), grad.cpu(), logits.cpu(), gimg[:rows].cpu()


@pytest.mark.parametrize('group', range(6))
def test_ft_head_edges(group, hip):
    """The head's K, T, B and D edges through ec_ft_loss_grad: loss, aggregated logits, d text and the feature gradient per
    element on dense features, invalid views exactly zero; compact rows with row_idx give the bits of the dense result
    gathered; grad_scale read from step_scalars gives the bits of the same value passed by value."""
    worst = 0.0
    for c in _head_groups()[group]:
        dense = []

        def impl(*a):
            out = _ft_head_raw(*a)
            dense.append((a, out))
            return out[:3] + (out[3].reshape(a[0].shape),)
        worst = max(worst, fr.check_head(impl, c, 'ec_ft_loss_grad', grad_scale=fr.GRAD_SCALE))
        (a, want), = dense
        valid, d_dense = a[1], want[3].reshape(a[0].shape)
        assert bool((d_dense[~valid] == 0).all()), f'{c}: gradient on an invalid view'
        gathered = want[:3] + (d_dense[valid].flip(0),)
        for scalars in (False, True):
            got = _ft_head_raw(*a, compact=True, scalars=scalars)
            for name, g, w in zip(('loss', 'grad_text', 'agg_logits', 'grad_img'), got, gathered):
                assert torch.equal(_bits(g), _bits(w)), f'{c}: compact {name} differs from the dense one (step_scalars {scalars})'
    _report(f'ft head group {group}', worst)


# ---------------------------------------------------------------------------------------------------------------
# (e) ec_classify_backward, directed: dZ read back exactly through d_feats (text_t the identity, no normalisation, scale 1)
# ---------------------------------------------------------------------------------------------------------------
def _classify_dz(full, ok, agg, d_full, d_logits, d_probs, want_text=False):
    B, T, K = full.shape
    C = (K + 3) // 4 * 4
    okf = ok.reshape(-1)
    n_rows = int(okf.sum())
    row_idx = torch.where(okf, torch.cumsum(okf.int(), 0) - 1, torch.full((B * T,), -1)).to(torch.int32)
    feats = torch.zeros(n_rows, C)
    feats[:, :K] = full.reshape(B * T, K)[okf]              # what the forward read: two tied views hold identical rows
    text_t = torch.zeros(C, K)
    text_t[:K] = torch.eye(K)
    lib = _L().lib()
    need = int(lib.ec_classify_backward_workspace_bytes(B, T, C, K))
    ws = torch.empty(need + 256, dtype=torch.uint8, device='cuda')
    d_feats, d_text = _pattern((n_rows, C)), _pattern((C, K))
    dv = lambda t: None if t is None else t.cuda()     # noqa: E731
    _L().launch('ec_classify_backward', feats.cuda(), n_rows, row_idx.cuda(), text_t.cuda(), B, T, C, K, 1.0, fr.AGG[agg], 0,
                full.cuda(), dv(d_full), dv(d_logits), dv(d_probs), d_feats, d_text, ws, need)
    torch.cuda.synchronize()
    d_feats = d_feats.cpu()
    assert not bool(d_feats[:, K:].any()), 'd_feats beyond K must be exact zeros'
    dZ = torch.zeros(B * T, K)
    dZ[okf] = d_feats[:, :K]
    if want_text:
        return dZ.reshape(B, T, K), d_text.cpu(), feats
    return dZ.reshape(B, T, K)


@pytest.mark.parametrize('K', fr.DZ_K)
@pytest.mark.parametrize('T', fr.DZ_T)
def test_classify_backward_max_directed(K, T, hip):
    """Exact ties (the lowest valid index wins, the other row gets exact zeros), all-negative valid logits next to an invalid
    view, a single valid view; the views' dZ sum to d_logits per class; d_text_t is the exact integer product."""
    fr.check_dz_directed(_classify_dz, K, T, f'ec_classify_backward K={K} T={T}')
    full, ok, gl = fr.dz_directed(K, T)
    dZ, d_text, feats = _classify_dz(full, ok, 'max', None, gl, None, want_text=True)
    want = feats.double().T @ dZ.reshape(-1, K)[ok.reshape(-1)].double()
    assert torch.equal(d_text.double(), want)
    worst = max(fr.check_dz_random(_classify_dz, K, T, agg, f'ec_classify_backward K={K} T={T} {agg}') for agg in fr.AGG)
    _report(f'classify dZ K={K} T={T}', worst)


def test_classify_backward_empty_batches(hip):
    lib = _L().lib()
    C, K, T = 8, 5, 3
    d_feats, d_text = _pattern((4, C)), _pattern((C, K))
    rc = lib.ec_classify_backward(None, 4, None, None, 0, T, C, K, 1.0, 2, 1, None, None, None, None, d_feats.data_ptr(),
                                  d_text.data_ptr(), None, 0, _L().stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and not bool(d_feats.any()) and not bool(d_text.any())
    d_text = _pattern((C, K))
    rc = lib.ec_classify_backward(None, 0, None, None, 2, T, C, K, 1.0, 2, 1, None, None, None, None, None, d_text.data_ptr(),
                                  None, 0, _L().stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and not bool(d_text.any())


# ---------------------------------------------------------------------------------------------------------------
# (f) the adapter stage by stage
# ---------------------------------------------------------------------------------------------------------------
class Adapter:
    """One geometry on the device: parameters, gradient buffers, the two structs, tape and workspace with their slot views."""

    def __init__(self, B, T, geom, layers, residual, struct_layers=None, struct_heads=None):
        from eventclip_amd import adapter as ad
        L = _L()
        self.B, self.T, (self.D, self.d, self.heads, self.ffn), self.layers, self.r = B, T, geom, layers, residual
        D, d, heads, ffn = geom
        self.top, self.blocks = fr.adapter_params(D, d, heads, ffn, layers)
        order = [(l, f) for l in range(layers) for _, f, _ in ad.LAYER_PARAMS] + [(None, f) for _, f, _ in ad.PROJ_PARAMS]
        self.order = order
        self.params = [(self.top if l is None else self.blocks[l])[f].cuda() for l, f in order]
        self.grads = [_pattern(tuple(p.shape)) for p in self.params]
        sl = struct_layers or layers
        pad = [self.params[0]] * (len(ad.LAYER_PARAMS) * (sl - layers))
        self.w, self._wb = ad._adapter_struct(pad + self.params if sl != layers else self.params, D, d, struct_heads or heads,
                                              ffn, sl, residual)
        self.g, self._gb = ad._adapter_struct(pad + self.grads if sl != layers else self.grads, D, d, struct_heads or heads, ffn,
                                              sl, residual)
        lib = L.lib()
        self.tape_bytes = int(lib.ec_adapter_train_tape_bytes(B, T, D, d, ffn, heads, layers))
        self.ws_bytes = int(lib.ec_adapter_train_backward_workspace_bytes(B, T, D, d, ffn))
        self.tape = torch.full((self.tape_bytes // 4 + 64,), float('nan'), device='cuda')
        self.ws = torch.full((self.ws_bytes // 4 + 64,), float('nan'), device='cuda')
        n_t = L.EC_AT_LAYER0 + L.EC_AT_PER_LAYER * layers
        self.t_off, self.s_off = (ctypes.c_int64 * n_t)(), (ctypes.c_int64 * L.EC_AS_COUNT)()
        assert lib.ec_adapter_train_layout(B, T, D, d, ffn, heads, layers, self.t_off, n_t, self.s_off, L.EC_AS_COUNT) == n_t

    def forward(self, img, valid, p, seed, expect_fail=False):
        out = _pattern(tuple(img.shape))
        self.img, self.v8 = img.cuda(), valid.to(torch.uint8).cuda()
        rc = _L().lib().ec_adapter_train_forward(self.img.data_ptr(), self.v8.data_ptr(), self.B, self.T, ctypes.byref(self.w),
                                                 float(p), ctypes.c_uint64(seed), out.data_ptr(), self.tape.data_ptr(),
                                                 self.tape_bytes, _L().stream_ptr())
        torch.cuda.synchronize()
        if expect_fail:
            return rc, out
        assert rc == 0, _L().lib().ec_last_error()
        assert bool(torch.isnan(self.tape[self.tape_bytes // 4:]).all()), 'the forward wrote past its tape'
        return out.cpu()

    def backward(self, d_out, p, seed):
        d_img = _pattern(tuple(d_out.shape))
        _L().launch('ec_adapter_train_backward', self.img, self.B, self.T, self.w, float(p), ctypes.c_uint64(seed), self.tape,
                    self.tape_bytes, d_out.cuda(), self.g, d_img, self.ws, self.ws_bytes)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.ws[self.ws_bytes // 4:]).all()), 'the backward wrote past its workspace'
        gt, gl = {}, [dict() for _ in range(self.layers)]
        for (l, f), g in zip(self.order, self.grads):
            (gt if l is None else gl[l])[f] = g.cpu()
        return (gt, gl), d_img.cpu()

    def _view(self, buf, off, *shape):
        n = int(np.prod(shape))
        return buf[off // 4:off // 4 + n].reshape(shape).cpu()

    def tape_views(self):
        L = _L()
        B, T, D, d, ffn, H = self.B, self.T, self.D, self.d, self.ffn, self.heads
        R = B * T
        v = lambda i, *s: self._view(self.tape, self.t_off[i], *s)     # noqa: E731
        tape = dict(h0=v(L.EC_AT_H0, R, d), hfin=v(L.EC_AT_HFIN, R, d), y=v(L.EC_AT_Y, R, D), L=[])
        for l in range(self.layers):
            o = L.EC_AT_LAYER0 + L.EC_AT_PER_LAYER * l
            tape['L'].append(dict(xhat1=v(o + L.EC_AT_L_XHAT1, R, d), rstd1=v(o + L.EC_AT_L_RSTD1, R), a=v(o + L.EC_AT_L_A, R, d),
                                  qkv=v(o + L.EC_AT_L_QKV, R, 3 * d), P=v(o + L.EC_AT_L_P, B, H, T, T), o=v(o + L.EC_AT_L_O, R, d),
                                  h1=v(o + L.EC_AT_L_H1, R, d), xhat2=v(o + L.EC_AT_L_XHAT2, R, d),
                                  rstd2=v(o + L.EC_AT_L_RSTD2, R), bn=v(o + L.EC_AT_L_BN, R, d), f=v(o + L.EC_AT_L_F, R, ffn)))
        return tape

    def scratch_views(self):
        L = _L()
        R, D, d, ffn = self.B * self.T, self.D, self.d, self.ffn
        v = lambda i, *s: self._view(self.ws, self.s_off[i], *s)     # noqa: E731
        return dict(dy=v(L.EC_AS_DY, R, D), dh=v(L.EC_AS_DH, R, d), dh1=v(L.EC_AS_DH1, R, d), dtmp_d=v(L.EC_AS_DTMP_D, R, d),
                    dqkv=v(L.EC_AS_DQKV, R, 3 * d), df=v(L.EC_AS_DF, R, ffn))


def test_adapter_layout_matches_the_size_functions(hip):
    L = _L()
    a = Adapter(3, 5, fr.GEOMETRIES[0], 2, 0.8)
    offs = list(a.t_off)
    assert offs[L.EC_AT_H0] == 0 and sorted(set(offs)) == sorted(offs) and all(o % 256 == 0 for o in offs)
    assert max(offs) + 4 * 15 * 72 <= a.tape_bytes and max(offs) == offs[L.EC_AT_LAYER0 + L.EC_AT_PER_LAYER + L.EC_AT_L_F]
    so = list(a.s_off)
    assert so[L.EC_AS_DY] == 0 and so == sorted(so) and max(so) + 4 * 15 * 72 <= a.ws_bytes
    lib = L.lib()
    assert lib.ec_adapter_train_layout(3, 5, 50, 40, 72, 5, 2, None, 0, None, 0) == L.EC_AT_LAYER0 + 2 * L.EC_AT_PER_LAYER
    assert lib.ec_adapter_train_layout(3, 5, 50, 40, 72, 5, 9, None, 0, None, 0) == L.EC_ERR_INVALID
    assert lib.ec_adapter_train_layout(3, 5, 50, 40, 72, 5, 2, a.t_off, 3, None, 0) == L.EC_ERR_INVALID


@pytest.mark.parametrize('case', fr.adapter_cases(), ids=lambda c: f'B{c[0]}T{c[1]}-{"x".join(map(str, c[2]))}-p{c[4]}-r{c[5]}')
def test_adapter_stage_by_stage(case, hip):
    """layers = 1: every tape slot and out after the forward; df, dqkv, dtmp_d, dh1, dh, dy, every parameter gradient and
    d_img_feats after the backward; a second backward gives the same bits and leaves the tape bit-unchanged."""
    B, T, geom, layers, p, r = case
    a = Adapter(B, T, geom, layers, r)
    img, valid, d_out = fr.adapter_inputs(B, T, geom[0])
    out = a.forward(img, valid, p, SEED)
    tape = a.tape_views()
    worst = fr.check_adapter_forward(img, valid, a.top, a.blocks, geom[2], r, p, SEED, out, tape, f'forward {case}')
    before = a.tape.clone()
    grads, d_img = a.backward(d_out, p, SEED)
    scr = a.scratch_views()
    wb = fr.check_adapter_backward(img, valid, a.top, a.blocks, geom[2], r, p, SEED, tape, d_out, grads, d_img, scr,
                                   f'backward {case}')
    for k, v in wb.items():
        worst[k] = max(worst.get(k, 0.0), v)
    grads2, d_img2 = a.backward(d_out, p, SEED)
    assert torch.equal(_bits(d_img), _bits(d_img2))
    for k, v in fr.flat_grads(grads, d_img).items():
        assert torch.equal(_bits(v), _bits(fr.flat_grads(grads2, d_img2)[k])), f'second backward: {k} differs'
    assert torch.equal(before.view(torch.int32), a.tape.view(torch.int32)), 'the backward wrote into the tape'
    _report(f'adapter {case}', {k: round(v, 4) for k, v in worst.items()})


def _end_to_end(layers, B, T, geom, p, r, stage_check=True):
    a = Adapter(B, T, geom, layers, r)
    img, valid, d_out = fr.adapter_inputs(B, T, geom[0])
    out = a.forward(img, valid, p, SEED)
    worst = {}
    if stage_check:
        worst = fr.check_adapter_forward(img, valid, a.top, a.blocks, geom[2], r, p, SEED, out, a.tape_views(), f'forward L={layers}')
    grads, d_img = a.backward(d_out, p, SEED)
    S = {}
    out64, tape64 = fr.adapter_forward(fr.A64, img, valid, a.top, a.blocks, geom[2], r, p, SEED)
    g64, di64, _ = fr.adapter_backward(fr.A64, img, valid, a.top, a.blocks, geom[2], r, tape64, d_out, p, SEED, S=S)
    worst['chain'] = fr.check_grads_end_to_end(fr.flat_grads(grads, d_img), fr.flat_grads(g64, di64), S, layers, f'L={layers}')
    return worst


@pytest.mark.parametrize('layers,shape,p,r', fr.E2E_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_adapter_deep(layers, shape, p, r, hip):
    """layers 2 and 8 (the tape's limit): the forward slots of every layer (the hfin slot is reused from layer to layer), all
    gradients end to end against the float64 replay (tests/test_fewshot_ref_cpu.py: equal to torch autograd of the module)."""
    _report(f'adapter layers={layers} {shape}', _end_to_end(layers, *shape, p, r))


def test_adapter_two_trip_dropout(hip):
    """R ffn > 4096 * 256: dropout_add, relu_bwd and axpby take their second grid trip; end to end against the replay."""
    b = fr.BIG_DROPOUT
    assert b['B'] * b['T'] * b['geom'][3] > 4096 * 256
    _report('adapter two-trip dropout', _end_to_end(b['layers'], b['B'], b['T'], b['geom'], b['p'], b['residual']))


@pytest.mark.parametrize('what', ['layers9', 'T17', 'heads'])
def test_adapter_refusals(what, hip):
    """layers = 9, T = 17 and d_model % heads != 0 are refused with an error code; out stays untouched."""
    geom = fr.GEOMETRIES[0]
    if what == 'layers9':
        a = Adapter(2, 3, geom, 8, 0.8, struct_layers=9)
    elif what == 'T17':
        a = Adapter(1, 16, geom, 1, 0.8)
        a.T = 17
    else:
        a = Adapter(2, 3, geom, 1, 0.8, struct_heads=3)
    img = torch.zeros(a.B, a.T, geom[0])
    a.tape = torch.full((a.tape.numel() * 2,), float('nan'), device='cuda')
    rc, out = a.forward(img, torch.ones(a.B, a.T, dtype=torch.bool), 0.0, 1, expect_fail=True)
    assert rc != 0 and b'geometry' in _L().lib().ec_last_error()
    assert bool((_bits(out) == -0x12345679).all()) and bool(torch.isnan(a.tape).all())
