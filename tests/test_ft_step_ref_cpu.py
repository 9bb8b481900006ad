"""tests/ft_step_ref.py on the CPU: (a) its float64 forms are the operations (torch's own float64 optimiser, autograd,
products and 16-bit casts agree), (b) the fp32 restatement (every product rounded, sums in index order) passes every
check over the whole tables with worst error / bound < 1, nothing excluded, and (c) every check rejects an fp32 model
with one planted fault."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ft_step_ref as ref  # noqa: E402
import vit_train_ref as vr  # noqa: E402

A32, A64, F32, F64, G = ref.A32, ref.A64, ref.F32, ref.F64, ref.G


# ---------------------------------------------------------------------------------------------------------------
# the fp32 models behind the checks' interfaces, with their planted faults
# ---------------------------------------------------------------------------------------------------------------
def adam_model(fault=None):
    def impl(call):
        out = [{k: it[k].clone() for k in 'pgmv'} for it in call['items']]
        if call['n_items'] == 0 or call['max_n'] == 0 or (call['skip'] and fault != 'skip_ignored'):
            return out, None
        lr = [call['lr0'], call['lr1']]
        if call['scalars'] is not None and fault != 'scalars_ignored':
            sc = call['scalars']
            lr, bc1, bc2s = [sc[ref.STEP_LR0], sc[ref.STEP_LR1]], sc[ref.STEP_BC1], sc[ref.STEP_BC2_SQRT]
        else:
            bc1, bc2s = ref.bias_corrections(call['b1'], call['b2'], max(call['step'], 1))
        for it, o in zip(call['items'][:call['n_items']], out):
            n = it['n']
            p, g, m, v = (ref.body(it[k], n) for k in 'pgmv')
            new = ref.adam_step(A32, p, g, m, v, lr[0 if fault == 'group_ignored' else it['group']], call['b1'], call['b2'],
                                call['eps'], 0.0 if fault == 'wd_dropped' else call['wd'], bc1, bc2s)
            cap = ref.ADAM_TRIP if fault == 'one_trip' else n
            for k, t in zip('pmv', new):
                ref.body(o[k], n)[:cap] = t[:cap]
            if fault == 'write_past':
                o['v'][G + n] = 0.0
        return out, None
    return impl


def unscale_model(fault=None):
    def impl(call):
        buf, n, flag = call['buf'].clone(), call['n'], call['flag']
        inv = call['inv_scale'] if call['scalars'] is None else call['scalars'][ref.STEP_INV_SCALE]
        x = ref.body(buf, n)
        y = x * torch.tensor(inv, dtype=F32)
        scan = x if fault == 'tested_before_scaling' else y
        bad = torch.isinf(scan) if fault == 'isinf_only' else ~torch.isfinite(scan)
        if fault == 'last_not_scanned':
            bad[n - 1] = False
        if fault == 'one_trip':
            bad[ref.UNSCALE_TRIP:] = False
        if bad.any():
            flag |= 1
        elif fault == 'flag_cleared':
            flag = 0
        x.copy_(y)
        return (buf, flag), None
    return impl


def lora_model(fault=None):
    def impl(op, call):
        rows, cols, r, n_items = call['rows'], call['cols'], call['r'], call['n_items']
        out = [{k: it[k].clone() for k in ('out', 'd_up', 'd_down')} for it in call['items']]
        entry = 'ec_lora_merge_batched' if op == 'merge' else 'ec_lora_grad_batched'
        if not (n_items > 0 and rows > 0 and cols > 0 and cols % 4 == 0 and 0 < r <= 64) or call['null_table']:
            return out, RuntimeError(f'{entry}: {n_items} items of {rows} x {cols}, r = {r}')
        for i in range(n_items):
            it = call['items'][0 if fault == 'item0' else i]
            base, up, down, dW = it['base'], it['up'], it['down'], it['dW']
            if op == 'merge':
                u = up.clone()
                if fault == 'factor16' and r % 16:
                    u[:, r - 1] = 0
                o = ref.lora_merge(A32, base, u, down)
                if fault == 'row16' and rows % 16:
                    o[rows - 1] = base[rows - 1]
                if fault == 'cols1024':
                    o[:, 1024:] = base[:, 1024:]
                ref.body(out[i]['out'], rows, cols).copy_(o)
            else:
                w = dW.clone()
                if fault == 'cols1024':
                    w[:, 1024:] = 0
                du = ref.lora_dup(A32, w, down)
                if fault == 'factor8' and r % 8:
                    du[:, r - 1] = 0
                if fault == 'row4' and rows % 4:
                    du[rows - 1] = 0
                if fault == 'slab':
                    slab = (rows + 15) // 16
                    w[(rows - 1) // slab * slab:] = 0
                dd = ref.lora_ddown(A32, up, w)
                if fault == 'factor16' and r % 16:
                    dd[r - 1] = 0
                ref.body(out[i]['d_up'], rows, r).copy_(du)
                ref.body(out[i]['d_down'], r, cols).copy_(dd)
        return out, None
    return impl


def _trunc16(v, dtype):
    """toward zero: the nearest-even pattern, stepped back where it overshot"""
    r = ref.rne16(v, dtype)
    with np.errstate(all='ignore'):
        over = np.abs(ref.decode16(r, dtype).astype(np.float64)) > np.abs(v.astype(np.float64))
    return np.where(over, r - 1, r).astype(np.uint16)


def _round16(v, dtype, fault):
    r = ref.rne16(v, dtype)
    if fault == 'truncate':
        r = _trunc16(v, dtype)
    if fault == 'ties_away':
        lo = _trunc16(v, dtype)
        with np.errstate(all='ignore'):
            a = np.abs(ref.decode16(lo, dtype).astype(np.float64))
            b = np.abs(ref.decode16(lo + 1, dtype).astype(np.float64))
            b = np.where(np.isinf(b), 2 * a - np.abs(ref.decode16(lo - 1, dtype).astype(np.float64)), b)     # 2^(emax + 1)
            tie = np.isfinite(v) & (np.abs(v.astype(np.float64)) == (a + b) / 2) & (a != b)
        r = np.where(tie, lo + 1, r).astype(np.uint16)
    if fault == 'flush_subnormals':
        emask = 0x7C00 if dtype == torch.float16 else 0x7F80
        r = np.where((r & emask) == 0, r & 0x8000, r).astype(np.uint16)
    return r


def pack_model(fault=None):
    """numpy, the definition again (with faults); ``torch_pack_model`` is the independent one."""
    def impl(call):
        rows, cols, dt = call['rows'], call['cols'], call['dtype']
        out = [{k: b[k].clone() for k in b} for b in call['bufs']]
        for w, pres, o in zip(call['ws'], call['present'], out):
            v = w.numpy()
            hi = _round16(v, dt, fault)
            with np.errstate(all='ignore'):
                against = _trunc16(v, dt) if fault == 'lo_from_unrounded_hi' else hi
                lo = _round16(v - ref.decode16(against, dt), dt, fault)
            hi_t = np.ascontiguousarray(hi.T)
            if fault == 'edge_tile_not_transposed':
                for r0 in range(0, rows, 64):
                    for c0 in range(0, cols, 64):
                        r1, c1 = min(r0 + 64, rows), min(c0 + 64, cols)
                        if r1 - r0 < 64 or c1 - c0 < 64:
                            hi_t[c0:c1, r0:r1] = hi[r0:r1, c0:c1].reshape(c1 - c0, r1 - r0)
            for k, on, val in zip(('hi', 'lo', 'hi_t'), pres, (hi, lo, hi_t)):
                if on or (fault == 'absent_written' and k == 'hi'):
                    o[k][G:G + rows * cols] = torch.from_numpy(val.reshape(-1).view(np.int16).copy())
        return out, None
    return impl


def torch_pack_model(call):
    rows, cols, dt = call['rows'], call['cols'], call['dtype']
    out = [{k: b[k].clone() for k in b} for b in call['bufs']]
    for w, pres, o in zip(call['ws'], call['present'], out):
        hi = w.to(dt)
        vals = (hi, (w - hi.float()).to(dt), hi.t().contiguous())
        for k, on, val in zip(('hi', 'lo', 'hi_t'), pres, vals):
            if on:
                o[k][G:G + rows * cols] = val.reshape(-1).view(torch.int16)
    return out, None


def ln_model(fault=None):
    def impl(call):
        rows, width, outs = call['rows'], call['width'], call['outs']
        out = {k: call[k].clone() for k in ('dx', 'dg', 'db')}
        want = outs != 'none'
        if (width % 4 or width > 2048 or call['ldx'] % 4 or call['ldy'] % 4 or call['ldo'] % 4 or (want and call['no_partials'])
                or np.float32(call['eps']) != np.float32(1e-5)):
            return out, RuntimeError(f'ec_layernorm_backward: width={width}')
        x, dy, dx0 = (ref.ln_view(call, k, call[ld]) for k, ld in (('x', 'ldx'), ('dy', 'ldy'), ('dx', 'ldo')))
        gam = ref.body(call['gamma'], width)
        acc = call['accumulate'] and fault != 'accumulate_ignored'
        dx, dg, db = ref.ln_rows(A32, x, dy, gam, dx0 if acc else None, mean_over=256 if fault == 'mean256' else None)
        if fault == 'last_partial_missing':
            wgs = min((rows + 3) // 4, 1024)
            keep = (torch.arange(rows) // 4) % wgs != wgs - 1
            _, dg, _ = ref.ln_rows(A32, x[keep], dy[keep], gam) if keep.any() else (0, torch.zeros(width), 0)
        if fault == 'beta_from_gamma':
            db = dg
        ref.body(out['dx'], rows, call['ldo'])[:, :width] = dx
        if outs in ('adjacent', 'separate', 'gamma'):
            ref.body(out['dg'], out['dg'].numel() - 2 * G)[:width] = dg
        if outs == 'adjacent':
            ref.body(out['dg'], 2 * width)[width:] = db
        if outs in ('separate', 'beta'):
            ref.body(out['db'], width).copy_(db)
        return out, None
    return impl


# ---------------------------------------------------------------------------------------------------------------
# (a) the float64 forms are the operations
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wd', [0.0, 0.02])
def test_adam_is_torch_adam(wd):
    p0, g, m0, v0 = (t.double() for t in ref.fr.adam_inputs(257, False))
    lr, (b1, b2), eps = ref.f32(2e-3), (ref.f32(0.9), ref.f32(0.98)), ref.f32(1e-3)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=ref.f32(wd))
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for step in (1, 2, 3):
        q.grad = g * step
        opt.step()
        p, m, v = ref.adam_step(A64, p, g * step, m, v, lr, b1, b2, eps, wd, 1 - b1 ** step, (1 - b2 ** step) ** 0.5)
    assert float((p - q.detach()).abs().max()) < 1e-13
    st = opt.state[q]
    assert float((m - st['exp_avg']).abs().max()) < 1e-13 and float((v - st['exp_avg_sq']).abs().max()) < 1e-13


def test_bias_corrections_are_the_fp32_values_of_the_host_code():
    for step in (1, 2, 1000):
        bc1, bc2s = ref.bias_corrections(0.9, 0.98, step)
        b1, b2 = np.float64(np.float32(0.9)), np.float64(np.float32(0.98))
        assert bc1 == float(np.float32(1 - b1 ** step)) and bc2s == float(np.float32(np.sqrt(1 - b2 ** step)))
    assert ref.bias_corrections(0.9, 0.98, 1)[0] == float(np.float32(1) - np.float32(0.9))


def test_layernorm_backward_is_autograd():
    g_ = ref.fr._gen(5)
    x, dy, gam = ref.fr._randn(g_, 7, 260) * 2 + 0.5, ref.fr._randn(g_, 7, 260), 1 + 0.2 * ref.fr._randn(g_, 260)
    dx0 = ref.fr._randn(g_, 7, 260)
    xa, ga, ba = x.clone().requires_grad_(True), gam.clone().requires_grad_(True), torch.zeros(260, dtype=F64, requires_grad=True)
    F.layer_norm(xa, (260,), ga, ba, 1e-5).backward(dy)
    for dx, dg, db in (ref.ln_rows(A64, x, dy, gam, dx0), [t[0] for t in ref.ln_bound(x, dy, gam, dx0)]):
        assert float((dx - dx0 - xa.grad).abs().max()) < 1e-12
        assert float((dg - ga.grad).abs().max()) < 1e-12 and float((db - ba.grad).abs().max()) < 1e-12


def test_lora_products_are_autograd():
    it = ref.lora_call((17, 260, 9, 1, 'random'))['items'][0]
    base, up, down, dW = (it[k].double() for k in ('base', 'up', 'down', 'dW'))
    ua, da = up.clone().requires_grad_(True), down.clone().requires_grad_(True)
    out = base + ua @ da
    (out * dW).sum().backward()
    assert float((ref.lora_merge(A64, base, up, down) - out.detach()).abs().max()) < 1e-13
    assert float((ref.lora_dup(A64, dW, down) - ua.grad).abs().max()) < 1e-12
    assert float((ref.lora_ddown(A64, up, dW) - da.grad).abs().max()) < 1e-12


@pytest.mark.parametrize('dtype', ref.PACK_DTYPES, ids=str)
def test_rne16_is_torch_cast(dtype):
    rng = np.random.default_rng(3)
    v = np.concatenate([ref.directed_values(dtype), rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        ref.pack_matrix(65, 129, dtype, 9, True).numpy().reshape(-1)])
    got = ref.rne16(v, dtype)
    want = torch.from_numpy(v).to(dtype).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(v)
    assert (got[~nan] == want[~nan]).all() and np.isnan(ref.decode16(got[nan], dtype)).all()
    back = ref.decode16(want, dtype)
    assert (back[~nan] == torch.from_numpy(v).to(dtype).float().numpy()[~nan]).all()
    # the definition's corner: a finite value whose hi is +inf has lo = -inf
    d = ref.directed_values(dtype)
    over = torch.from_numpy(d[np.isfinite(d) & np.isinf(ref.decode16(ref.rne16(d, dtype), dtype)) & (d > 0)]).view(1, -1)
    assert over.numel() >= 2
    hi, lo, _ = ref.pack_reference(over, dtype)
    assert np.isposinf(ref.decode16(hi, dtype)).all() and np.isneginf(ref.decode16(lo, dtype)).all()


def test_unscale_product_is_the_rounded_exact_product():
    x = ref.unscale_data(4096)
    for inv in ref.UNSCALE_INV:
        want = (x.double() * inv).float()
        assert ref.same_bits(ref.unscale_product(x, inv), want)
        assert inv == 1.0 or bool(((want != 0) & (want.abs() < 2.0 ** -126)).any()), 'no subnormal result in the data'


# ---------------------------------------------------------------------------------------------------------------
# (b) the restatement is inside every bound over the whole tables
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_adam():
    worst = max(ref.check_adam_list(adam_model(), c, 'adam', variants=i in (0, 6)) for i, c in enumerate(ref.ADAM_CASES))
    print(f'\n[ft step ref] adam: worst error / bound = {worst:.4f}')
    assert worst < 1


def test_restatement_unscale():
    n = sum(ref.check_unscale(unscale_model(), n, 'unscale') for n in ref.UNSCALE_N)
    print(f'\n[ft step ref] unscale: {n} launches, bit for bit')


def test_restatement_lora():
    worst = dict(merge=0.0, d_up=0.0, d_down=0.0)
    for c in ref.lora_cases():
        for k, v in ref.check_lora(lora_model(), c, 'lora').items():
            worst[k] = max(worst[k], v)
    print(f'\n[ft step ref] lora: worst error / bound = { {k: round(v, 4) for k, v in worst.items()} }')
    assert max(worst.values()) < 1
    assert ref.check_lora_refusals(lora_model(), 'lora') == 10


@pytest.mark.parametrize('model', [torch_pack_model, pack_model()], ids=['torch', 'numpy'])
def test_restatement_pack(model):
    n = sum(ref.check_pack(model, c, 'pack') for c in ref.pack_cases())
    print(f'\n[ft step ref] pack: {n} elements, bit for bit')


def test_restatement_layernorm():
    worst = max(ref.check_ln(ln_model(), c, 'ln') for c in ref.ln_cases())
    print(f'\n[ft step ref] layernorm backward: worst error / bound = {worst:.4f}')
    assert worst < 1
    assert ref.check_ln_refusals(ln_model(), 'ln') == 7


def test_tables_reach_what_they_are_for():
    cs = ref.ln_cases()
    assert {c[4] for c in cs} == set(ref.LN_OUTS) and {c[5] for c in cs if c[1] != 256} == set(ref.LN_KINDS)
    assert {c[5] for c in cs if c[0] > 5} == set(ref.LN_KINDS)
    for i in range(3):
        assert any(c[2][i] for c in cs if c[0] >= 4096), 'a stride beyond the width on the second trip'
    assert {(c[0], c[3], c[4]) for c in cs if c[1] == 256 and c[0] in ref.LN_ROWS} >= {(r, a, o) for r in ref.LN_ROWS
                                                                                      for a, o in ((0, 'adjacent'), (1, 'separate'))}
    ls = ref.lora_cases()
    assert {c[0] for c in ls} >= set(ref.LORA_ROWS) and {c[1] for c in ls} >= set(ref.LORA_COLS) and {c[2] for c in ls} >= set(ref.LORA_R)
    assert {c[3] for c in ls} == {1, 3} and {c[4] for c in ls} == set(ref.LORA_KINDS)
    for dt in ref.PACK_DTYPES:
        d = ref.directed_values(dt)
        assert ref.pack_matrix(65, 129, dt, 1, True).numpy().reshape(-1)[:d.size].tobytes() == d.tobytes()
    assert len({s for s in ref.SUBSETS}) == 8


# ---------------------------------------------------------------------------------------------------------------
# (c) every check rejects one planted fault
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fault,case', [('group_ignored', 0), ('wd_dropped', 1), ('one_trip', 0), ('skip_ignored', 0),
                                        ('scalars_ignored', 0), ('write_past', 0)])
def test_adam_check_catches(fault, case):
    with pytest.raises(AssertionError):
        ref.check_adam_list(adam_model(fault), ref.ADAM_CASES[case], fault)


@pytest.mark.parametrize('fault,n', [('last_not_scanned', 257), ('one_trip', ref.UNSCALE_TRIP + 1), ('isinf_only', 65),
                                     ('tested_before_scaling', 64), ('flag_cleared', 1)])
def test_unscale_check_catches(fault, n):
    with pytest.raises(AssertionError):
        ref.check_unscale(unscale_model(fault), n, fault)


@pytest.mark.parametrize('fault,case', [('factor16', (33, 260, 17, 3, 'random')), ('factor16', (17, 260, 9, 1, 'one_factor')),
                                        ('factor8', (33, 260, 9, 3, 'random')), ('row16', (17, 260, 17, 3, 'random')),
                                        ('row4', (5, 8, 2, 1, 'random')), ('row4', (17, 260, 9, 1, 'one_row')),
                                        ('slab', (33, 260, 17, 3, 'random')), ('slab', (200, 8, 2, 1, 'random')),
                                        ('cols1024', (33, 1028, 17, 3, 'random')), ('item0', (3, 8, 2, 3, 'random'))])
def test_lora_check_catches(fault, case):
    assert case in ref.lora_cases() or case[:3] + (1, 'random') in ref.lora_cases() or case[:3] + (3, 'random') in ref.lora_cases(), case
    with pytest.raises(AssertionError):
        ref.check_lora(lora_model(fault), case, fault)


@pytest.mark.parametrize('dtype', ref.PACK_DTYPES, ids=str)
@pytest.mark.parametrize('fault', ['truncate', 'ties_away', 'flush_subnormals', 'lo_from_unrounded_hi', 'edge_tile_not_transposed',
                                   'absent_written'])
def test_pack_check_catches(fault, dtype):
    caught = 0
    for c in ref.pack_cases():
        if c[2] == dtype and c[:2] in ((65, 65), (129, 65), (63, 3)):
            try:
                ref.check_pack(pack_model(fault), c, fault)
            except AssertionError:
                caught += 1
    assert caught, fault


@pytest.mark.parametrize('fault,pick', [('accumulate_ignored', lambda c: c[3] == 1 and c[0] <= 5),
                                        ('last_partial_missing', lambda c: c[0] in (253, 4097) and c[4] in ('adjacent', 'separate')),
                                        ('beta_from_gamma', lambda c: c[4] in ('adjacent', 'separate', 'beta') and c[0] == 5),
                                        ('mean256', lambda c: c[1] in (252, 260) and c[0] == 5)], ids=lambda v: v if isinstance(v, str) else '')
def test_layernorm_check_catches(fault, pick):
    cases = [c for c in ref.ln_cases() if pick(c)]
    assert cases
    for c in cases:
        with pytest.raises(AssertionError):
            ref.check_ln(ln_model(fault), c, fault)


def test_refusal_checks_catch_an_entry_that_runs():
    """... or that refuses after it has written, or under another name."""
    def lora_runs(op, call):
        return [{k: it[k].clone() for k in ('out', 'd_up', 'd_down')} for it in call['items']], None

    def lora_writes(op, call):
        out, err = lora_model()(op, call)
        out[0]['out'][G] = 1.0
        return out, err

    def ln_anonymous(call):
        return ln_model()(call)[0], RuntimeError('invalid argument')
    for impl in (lora_runs, lora_writes):
        with pytest.raises(AssertionError):
            ref.check_lora_refusals(impl, 'lora')
    for impl in (lambda call: ({k: call[k].clone() for k in ('dx', 'dg', 'db')}, None), ln_anonymous):
        with pytest.raises(AssertionError):
            ref.check_ln_refusals(impl, 'ln')
