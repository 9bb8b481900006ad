"""The kernels of csrc/vit_train.hip that turn a gradient into a weight update, at every loop, grid and dispatch edge:
ec_adam_step_multi, ec_grad_unscale_check, ec_lora_merge_batched / ec_lora_grad_batched, ec_pack_weight16_batched and the
public ec_layernorm_backward, against the float64 or bit-exact expectations of tests/ft_step_ref.py (whose checks
tests/test_ft_step_ref_cpu.py runs against the fp32 restatement and against planted faults).  Each callable below moves one
call to the device, runs the entry point once and reads every buffer back whole; each test prints the worst error / bound.

ec_lora_merge_batched is run as the trainer runs it (ft.LoraFactors.bind): ``out`` is a buffer of its own that starts
uninitialised, never ``base`` itself."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ft_step_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, G = torch.float32, ref.G


def _L():
    from eventclip_amd import _lib
    return _lib


def _report(name, worst):
    if isinstance(worst, str):          # an exact family: what was compared
        print(f'\n[ft step edges] {name}: {worst}')
    else:
        print(f'\n[ft step edges] {name}: worst error / bound = {worst if isinstance(worst, dict) else round(worst, 4)}')


def _try(name, *args):
    """Run the entry point -> the RuntimeError it raised, or None; the device is idle afterwards."""
    try:
        _L().launch(name, *args)
        err = None
    except RuntimeError as e:
        err = e
    torch.cuda.synchronize()
    return err


def _opt(values, dtype):
    return None if values is None else torch.tensor(values, dtype=dtype, device='cuda')


def _scratch(n):
    """A guarded NaN buffer on the device and the function that checks its guards."""
    buf = ref.nan_buf(n).cuda()
    return buf, lambda what: ref.guards_back(buf.cpu(), n, what)


def test_step_scalar_indices_are_the_headers(hip):
    L = _L()
    assert (L.EC_STEP_LR0, L.EC_STEP_LR1, L.EC_STEP_BC1, L.EC_STEP_BC2_SQRT, L.EC_STEP_GRAD_SCALE, L.EC_STEP_INV_SCALE,
            L.EC_STEP_COUNT) == (ref.STEP_LR0, ref.STEP_LR1, ref.STEP_BC1, ref.STEP_BC2_SQRT, ref.STEP_GRAD_SCALE,
                                 ref.STEP_INV_SCALE, ref.STEP_COUNT)


# ---------------------------------------------------------------------------------------------------------------
# ec_adam_step_multi
# ---------------------------------------------------------------------------------------------------------------
def _adam(call):
    L = _L()
    dev = [{k: it[k].cuda() for k in 'pgmv'} for it in call['items']]
    items = (L.EcAdamItem * len(dev))()
    for it, d, c in zip(items, dev, call['items']):
        it.param, it.grad, it.exp_avg, it.exp_avg_sq = (d[k].data_ptr() + 4 * G for k in 'pgmv')
        it.n, it.group = c['n'], c['group']
    table = L.device_table(items)
    err = _try('ec_adam_step_multi', table, call['n_items'], call['max_n'], float(call['lr0']), float(call['lr1']),
               float(call['b1']), float(call['b2']), float(call['eps']), float(call['wd']), int(call['step']),
               _opt(None if call['skip'] is None else [call['skip']], torch.int32), _opt(call['scalars'], F32))
    return [{k: d[k].cpu() for k in 'pgmv'} for d in dev], err


@pytest.mark.parametrize('i', range(len(ref.ADAM_CASES)), ids=lambda i: 's{}-wd{}-eps{}-{}'.format(*ref.ADAM_CASES[i][:3], 'dir' if ref.ADAM_CASES[i][3] else 'rnd'))
def test_adam_list_edges(hip, i):
    """One launch over nine tensors of 0 .. 131 072 + 77 elements in two groups, small ones beside the large: both sides
    of the 512-workgroup grid cap, weight decay on and off, both eps, steps 1, 2 and 1000, Gaussian and directed inputs,
    guards around every buffer; the device-scalars form against poisoned by-value arguments, bit for bit; on the first
    Gaussian and the first directed case the skip flag (1, -1, 0), n_items = 0 and max_n = 0."""
    _report(f'adam {ref.ADAM_CASES[i]}', ref.check_adam_list(_adam, ref.ADAM_CASES[i], 'ec_adam_step_multi', variants=i in (0, 6)))


# ---------------------------------------------------------------------------------------------------------------
# ec_grad_unscale_check
# ---------------------------------------------------------------------------------------------------------------
def _unscale(call):
    buf, flag = call['buf'].cuda(), torch.tensor([call['flag']], dtype=torch.int32, device='cuda')
    err = _try('ec_grad_unscale_check', buf[G:], call['n'], float(call['inv_scale']), flag, _opt(call['scalars'], F32))
    return (buf.cpu(), int(flag.cpu())), err


@pytest.mark.parametrize('n', ref.UNSCALE_N)
def test_unscale_and_check_edges(hip, n):
    """Products bit for bit (subnormal results included) at three scales; the flag left alone on finite data; one +inf,
    -inf or NaN alone at element 0, n - 1, the end of the first wave, the start of the second workgroup and of the second
    grid trip; the overflow of the product itself; the device scalar over a poisoned by-value scale."""
    _report(f'unscale n={n}', f'{ref.check_unscale(_unscale, n, "ec_grad_unscale_check")} launches, bit for bit')


# ---------------------------------------------------------------------------------------------------------------
# ec_lora_merge_batched, ec_lora_grad_batched
# ---------------------------------------------------------------------------------------------------------------
def _lora(op, call):
    L = _L()
    rows, cols, r, n_items = call['rows'], call['cols'], call['r'], call['n_items']
    dev = [{k: v.cuda() for k, v in it.items()} for it in call['items']]
    items = (L.EcLoraItem * len(dev))()
    for it, d in zip(items, dev):
        it.base, it.up, it.down, it.dW = (d[k].data_ptr() for k in ('base', 'up', 'down', 'dW'))
        it.out, it.d_up, it.d_down = (d[k].data_ptr() + 4 * G for k in ('out', 'd_up', 'd_down'))
    table = None if call['null_table'] else L.device_table(items)
    if op == 'merge':
        err = _try('ec_lora_merge_batched', table, n_items, rows, cols, r)
    else:
        n = int(L.lib().ec_lora_grad_scratch_floats(n_items, rows, cols, r))
        scratch, scratch_ok = _scratch(n)
        err = _try('ec_lora_grad_batched', table, n_items, rows, cols, r, scratch[G:])
        scratch_ok(f'ec_lora_grad_batched {rows} x {cols}, r = {r}: scratch of ec_lora_grad_scratch_floats')
    return [{k: d[k].cpu() for k in ('out', 'd_up', 'd_down')} for d in dev], err


LORA_GROUPS = 6


@pytest.mark.parametrize('group', range(LORA_GROUPS))
def test_lora_edges(hip, group):
    """Every row count around the 16-row blocks (merge), the 4 rows of a wave (d up) and the slabs (d down), every rank
    around the 16- and 8-factor rounds, every width around the 256-column lane stride and the second column workgroup,
    one and three items with data of their own; outputs start as NaN between guards; a cancelling row, an `up` with
    only its last factor, a dW with only its last row."""
    worst = dict(merge=0.0, d_up=0.0, d_down=0.0)
    for c in ref.lora_cases()[group::LORA_GROUPS]:
        for k, v in ref.check_lora(_lora, c, 'ec_lora').items():
            worst[k] = max(worst[k], round(v, 4))
    _report(f'lora group {group}', worst)


def test_lora_refusals(hip):
    assert ref.check_lora_refusals(_lora, 'ec_lora') == 10


# ---------------------------------------------------------------------------------------------------------------
# ec_pack_weight16_batched
# ---------------------------------------------------------------------------------------------------------------
def _pack(call):
    from eventclip_amd import ops
    L = _L()
    ws = [w.contiguous().cuda() for w in call['ws']]
    dev = [{k: b[k].cuda() for k in b} for b in call['bufs']]
    items = (L.EcPackItem * len(ws))()
    for it, w, d, pres in zip(items, ws, dev, call['present']):
        it.w = w.data_ptr()
        it.hi, it.lo, it.hi_t = (d[k].data_ptr() + 2 * G if on else None for k, on in zip(('hi', 'lo', 'hi_t'), pres))
    err = _try('ec_pack_weight16_batched', L.device_table(items), len(ws), call['rows'], call['cols'], ops.dtype_code(call['dtype']))
    return [{k: d[k].cpu() for k in d} for d in dev], err


@pytest.mark.parametrize('launch', range(len(ref.PACK_LAUNCHES)))
@pytest.mark.parametrize('dtype', ref.PACK_DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_pack_edges(hip, dtype, launch):
    """hi, lo and hi transposed bit for bit against IEEE round-to-nearest-even with subnormals, at every shape around the
    64-tile, on ties, the overflow edge, the subnormal range, zeros, infinities and NaN; three items per launch with
    different subsets of the outputs, every subset reached, the buffers of the absent ones untouched."""
    n = sum(ref.check_pack(_pack, c, 'ec_pack_weight16_batched') for c in ref.pack_cases() if c[2] == dtype and c[3] == launch)
    _report(f'pack {dtype} launch {launch}', f'{n} elements, bit for bit')


# ---------------------------------------------------------------------------------------------------------------
# ec_layernorm_backward
# ---------------------------------------------------------------------------------------------------------------
def _ln(call):
    L = _L()
    rows, width, outs = call['rows'], call['width'], call['outs']
    d = {k: call[k].cuda() for k in ('x', 'dy', 'gamma', 'dx', 'dg', 'db')}
    part, part_ok = _scratch(int(L.lib().ec_layernorm_backward_partials(rows, width)))
    dg = d['dg'][G:] if outs in ('adjacent', 'separate', 'gamma') else None
    db = d['dg'][G + width:] if outs == 'adjacent' else d['db'][G:] if outs in ('separate', 'beta') else None
    err = _try('ec_layernorm_backward', d['x'][G:], call['ldx'], d['dy'][G:], call['ldy'], d['gamma'][G:], rows, width,
               float(call['eps']), d['dx'][G:], call['ldo'], int(call['accumulate']), dg, db,
               None if call['no_partials'] else part[G:])
    part_ok(f'ec_layernorm_backward {rows} x {width}: partials of ec_layernorm_backward_partials')
    return {k: d[k].cpu() for k in ('dx', 'dg', 'db')}, err


LN_GROUPS = 4


@pytest.mark.parametrize('group', range(LN_GROUPS))
def test_layernorm_backward_edges(hip, group):
    """Widths that leave lanes without a unit, row counts either side of the 1024-workgroup cap and of the switch between
    the two reduction kernels, strides beyond the width (NaN in the padding of x and dy, a pattern in dx's), accumulate on
    and off, d gamma / d beta adjacent, separate, alone or absent (then without the partials scratch); an offset row, a
    constant row, dy = 0, dy proportional to x hat, gamma with zero columns."""
    worst = max(ref.check_ln(_ln, c, 'ec_layernorm_backward') for c in ref.ln_cases()[group::LN_GROUPS])
    _report(f'layernorm backward group {group}', worst)


def test_layernorm_backward_refusals(hip):
    assert ref.check_ln_refusals(_ln, 'ec_layernorm_backward') == 7
