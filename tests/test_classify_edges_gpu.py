"""ec_classify_v2 and ec_pseudo_label through the C ABI at their edges, against float64: tests/classify_ref.py holds the
references, the directed inputs, the shared cases and the bounds (per element; their constants are measured in
tests/test_classify_ref_cpu.py, the kernels get KERNEL_FACTOR times the restatement's error).

Every classify call here fills both workspaces with 0xFF bytes (fp16 / fp32 NaN) before ec_classify_prep_text and before
ec_classify_v2, with 256 guard bytes behind each, and carves the three outputs from one buffer of sentinels with guard
bands in front, between and behind: a padded row or column that the GEMM reads and nobody wrote shows as NaN, a write
beyond an output as a changed guard.

Measured on an MI355X when these tests were written, error over bound (KERNEL_FACTOR included) across every shared call:
full_logits 0.20 (the massive-channel rows; every other kind of row below 0.12), aggregated logits 0.20, probabilities
0.06 -- the fp16 subnormal floor 2^-35 F of the lo parts holds on the matrix pipe."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classify_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A            # 1.5e16 as fp32, 1515870810 as int32
GUARD = 61                       # elements; odd, so that the outputs start at no special alignment
NAN, INF = float('nan'), float('inf')


def _L():
    from eventclip_amd import _lib
    return _lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _refused(rc, needle):
    lib = _L()
    assert rc == lib.EC_ERR_INVALID, rc
    msg = lib.lib().ec_last_error().decode()
    assert needle in msg, msg


def _poisoned(nbytes):
    """A device buffer of `nbytes` 0xFF bytes and 256 more behind them."""
    return torch.full((max(int(nbytes), 256) + 256,), 0xFF, dtype=torch.uint8, device='cuda')


def _guard_intact(buf, nbytes, what):
    assert bool((buf[max(int(nbytes), 256):] == 0xFF).all()), f'{what}: bytes behind the workspace written'


class Carved:
    """Outputs carved from one sentinel-filled buffer: guard | out 0 | guard | out 1 | ... | guard."""

    def __init__(self, shapes, dtypes=None):
        dtypes = dtypes or [torch.float32] * len(shapes)
        self.sizes = [(math.prod(s) * d.itemsize + 3) // 4 * 4 for s, d in zip(shapes, dtypes)]      # bytes, whole int32s
        self.buf = torch.full((sum(self.sizes) // 4 + GUARD * (len(shapes) + 1),), SENTINEL, dtype=torch.int32, device='cuda')
        self.out, self.guards, at = [], [], 0
        for s, d, b in zip(shapes, dtypes, self.sizes):
            self.guards.append((at, at + GUARD))
            at += GUARD
            self.out.append(self.buf[at:at + b // 4].view(torch.uint8)[:math.prod(s) * d.itemsize].view(d).view(*s))
            at += b // 4
        self.guards.append((at, at + GUARD))

    def intact(self, what):
        for i, (a, b) in enumerate(self.guards):
            assert bool((self.buf[a:b] == SENTINEL).all()), f'{what}: guard band {i} written'


def run_classify(feats, text, row_idx, scale, agg, normalize, what=''):
    """feats [n_rows, C], text [K, C], row_idx [B, T] on the device -> (full_logits, logits, probs) on the CPU, after the
    guard checks."""
    lib, s = _L().lib(), _L().stream_ptr()
    n_rows, C = feats.shape
    K = text.shape[0]
    B, T = row_idx.shape
    text_t = text.t().contiguous()
    tb, wb = lib.ec_classify_text_bytes(C, K), lib.ec_classify_v2_workspace_bytes(n_rows, C, K)
    tws, ws = _poisoned(tb), _poisoned(wb)
    _L().check(lib.ec_classify_prep_text(_p(text_t), C, K, _p(tws), tb, s), 'ec_classify_prep_text')
    out = Carved([(B, T, K), (B, K), (B, K)])
    _L().check(lib.ec_classify_v2(_p(feats), n_rows, _p(row_idx), _p(tws), B, T, C, K, scale, ref.AGG_CODE[agg], int(normalize),
                                  _p(out.out[0]), _p(out.out[1]), _p(out.out[2]), _p(ws), max(wb, 256), s), 'ec_classify_v2')
    out.intact(what)
    _guard_intact(tws, tb, what + ' text planes')
    _guard_intact(ws, wb, what + ' workspace')
    return tuple(o.cpu() for o in out.out)


def _dev(inp):
    return inp.feats.cuda(), inp.text.cuda(), inp.row_idx.cuda()


def _within(got, want, bound, what):
    over = ref.excess(got, want, bound)
    if over > 0:
        ok = ~torch.isnan(want)
        err = (got.double() - want).abs()
        ratio = float((err[ok] / bound[ok].clamp(min=1e-300)).max()) if bool(ok.any()) else NAN
        raise AssertionError(f'{what}: {float(err[ok].max()) if bool(ok.any()) else NAN:.3e} off, {over:.3e} over the bound, '
                             f'error / bound up to {ratio:.3g} (the bound already holds KERNEL_FACTOR = {ref.KERNEL_FACTOR})')


def _check(got, inp, agg, normalize, what):
    full, logits, probs = got
    want = ref.classify64(inp.feats, inp.text, inp.row_idx, inp.scale, agg, normalize)
    b = ref.bounds(want, inp.scale, agg, normalize)
    _within(full, want['full_logits'], b['full_logits'], what + ' full_logits')
    _within(logits, want['logits'], b['logits'], what + ' logits')
    _within(probs, want['probs'], b['probs'], what + ' probs')
    assert bool((full[~want['valid']] == 0).all()), what + ': an invalid view is not 0'
    return want


# ---------------------------------------------------------------------------------------------------------------
# ec_classify_v2
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.CASES, ids=lambda c: f'B{c.B}-T{c.T}-K{c.K}-C{c.C}-{c.layout}-{"masked" if c.masked else "all"}-r{c.m4}')
def test_classify_at_every_shared_case(case, hip):
    """Every shared case x the rotations that bring every kind of row in front of a valid view x both normalize values x
    the three aggregations: full_logits, logits and probs within their bounds, invalid views exactly 0, two views of one
    row bit-equal."""
    for rot in ref.rotations(case):
        for normalize in (False, True):
            inp = ref.inputs(case, rot, normalize)
            dev = _dev(inp)
            flat = inp.row_idx.flatten().tolist()
            for agg in ref.AGGS:
                what = f'{case} rot={rot} normalize={normalize} {agg}'
                got = run_classify(*dev, inp.scale, agg, normalize, what)
                _check(got, inp, agg, normalize, what)
                rows = got[0].view(len(flat), case.K)
                first = {}
                for v, r in enumerate(flat):
                    if r >= 0 and first.setdefault(r, v) != v:
                        assert torch.equal(rows[v].view(torch.int32), rows[first[r]].view(torch.int32)), what + ': shared row'


@pytest.mark.parametrize('agg', ref.AGGS)
def test_classify_exact_integers(agg, hip):
    """The exact builder at every shared case: full_logits, sum and max bit-equal to the float64 result cast to fp32, mean
    within one ulp (one division).  Masking and indexing errors show here at zero tolerance."""
    for case in ref.CASES:
        inp = ref.exact_inputs(case)
        full, logits, probs = run_classify(*_dev(inp), inp.scale, agg, False, f'exact {case}')
        want = ref.classify64(inp.feats, inp.text, inp.row_idx, inp.scale, agg, False)
        w_full, w_logits = want['full_logits'].float(), want['logits'].float()
        assert torch.equal(full, w_full), f'exact {case}: full_logits'
        if agg == 'mean':
            assert bool(((logits - w_logits).abs() <= ref.ulp32(w_logits)).all()), f'exact {case}: mean'
        else:
            assert torch.equal(logits, w_logits), f'exact {case}: {agg}'
        b = ref.bounds(want, inp.scale, agg, False)
        _within(probs, want['probs'], b['probs'], f'exact {case} probs')


# three samples of three views each in their own rows, pad columns (129 -> 192) and pad classes (65 -> 80), a masked view
# per sample: for the tests that change one sample and watch its neighbours
DENSE = ref.Case(B=3, T=3, K=65, C=129, layout='dense', masked=True, m4=1)


@pytest.mark.parametrize('normalize', [False, True])
@pytest.mark.parametrize('agg', ref.AGGS)
def test_sample_without_a_valid_view(agg, normalize, hip):
    """Sample 1 of 3 loses every view: sum 0, mean 0 / 0 = NaN, max -1e6, probabilities NaN, as in the reference; its
    full_logits are 0 and the neighbours stay within their bounds."""
    case = DENSE
    inp = ref.inputs(case, 0, normalize)
    idx = inp.row_idx.clone()
    idx[1] = -1
    inp = inp._replace(row_idx=idx, valid=idx >= 0)
    got = run_classify(*_dev(inp), inp.scale, agg, normalize, 'empty sample')
    want = _check(got, inp, agg, normalize, f'empty sample {agg} normalize={normalize}')
    full, logits, probs = got
    assert bool((full[1] == 0).all()) and bool(torch.isnan(probs[1]).all()) and bool(torch.isnan(want['probs'][1]).all())
    assert not bool(torch.isnan(probs[[0, 2]]).any()) and not bool(torch.isnan(logits[[0, 2]]).any())
    if agg == 'sum':
        assert bool((logits[1] == 0).all())
    elif agg == 'mean':
        assert bool(torch.isnan(logits[1]).all())
    else:
        assert bool((logits[1] == -1e6).all())


@pytest.mark.parametrize('bad', [NAN, INF, -INF])
def test_a_non_finite_row_stays_in_its_sample(bad, hip):
    """One feature row of NaN (or with one infinite element): the samples that do not read it keep every bit of all three
    outputs, under every aggregation and both normalize values."""
    case = DENSE
    for normalize in (False, True):
        inp = ref.inputs(case, 0, normalize)
        feats, text, idx = _dev(inp)
        row = int(inp.row_idx[1][inp.row_idx[1] >= 0][0])
        broken = feats.clone()
        if bad != bad:
            broken[row] = bad
        else:
            broken[row, case.C // 2] = bad
        for agg in ref.AGGS:
            clean = run_classify(feats, text, idx, inp.scale, agg, normalize, 'clean')
            got = run_classify(broken, text, idx, inp.scale, agg, normalize, 'non-finite row')
            for a, b in zip(got, clean):
                assert torch.equal(a[[0, 2]].view(torch.int32), b[[0, 2]].view(torch.int32)), (bad, agg, normalize)
            assert not bool(torch.isfinite(got[0][1]).all())


def test_classify_refusals(hip):
    """T = 17 (one past CL_MAXT), T = 0, K = 0 and C = 0: refused before any launch, with the shape in the message."""
    lib, s = _L().lib(), _L().stream_ptr()
    f = torch.zeros(64, 64, device='cuda')
    idx = torch.zeros(4, 17, dtype=torch.int32, device='cuda')
    out = torch.zeros(4 * 17 * 16, device='cuda')
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')

    def call(T, C, K):
        return lib.ec_classify_v2(_p(f), 4, _p(idx), _p(ws), 4, T, C, K, 100.0, 0, 0, _p(out), _p(out), _p(out), _p(ws), ws.numel(), s)
    _refused(call(17, 64, 16), 'bad shape')
    _refused(call(17, 64, 16), 'T=17')
    _refused(call(17, 64, 16), '(T <= 16)')
    _refused(call(0, 64, 16), 'T=0')
    _refused(call(1, 64, 0), 'K=0')
    _refused(call(1, 0, 16), 'C=0')
    _refused(lib.ec_classify_v2(_p(f), 4, _p(idx), _p(ws), 4, 1, 64, 16, 100.0, 3, 0, _p(out), _p(out), _p(out), _p(ws), ws.numel(), s),
             'unknown agg 3')
    _refused(lib.ec_classify_prep_text(_p(f), 64, 0, _p(ws), ws.numel(), s), 'bad arguments')
    _refused(lib.ec_classify_prep_text(_p(f), 0, 16, _p(ws), ws.numel(), s), 'bad arguments')
    assert lib.ec_classify_text_bytes(64, 0) == 0 and lib.ec_classify_v2_workspace_bytes(4, 0, 16) == 0


def test_classify_through_the_torch_op(hip):
    """torch.ops.eventclip_hip.classify (scratch from torch.empty, text planes cached) on a case with pad columns and pad
    classes, after a call that left other data in the allocator's blocks: the same bounds."""
    from eventclip_amd import torch_ops
    case = DENSE
    torch_ops._TEXT_PLANES.clear()
    for normalize in (False, True):
        for rot in ref.rotations(case):
            inp = ref.inputs(case, rot, normalize)
            feats, text, idx = _dev(inp)
            text_t = text.t().contiguous()
            junk = torch.full((1 << 20,), NAN, device='cuda')
            del junk
            for agg in ref.AGGS:
                got = torch.ops.eventclip_hip.classify(feats, idx, text_t, inp.scale, ref.AGG_CODE[agg], normalize)
                _check(tuple(g.cpu() for g in got), inp, agg, normalize, f'op {case} rot={rot} normalize={normalize} {agg}')


# ---------------------------------------------------------------------------------------------------------------
# ec_pseudo_label
# ---------------------------------------------------------------------------------------------------------------
def run_pseudo_label(probs, thresh, consistent, min_prob, with_mean=True):
    """probs [B, V, K] on the device -> dict(mean, max_prob fp32; pred int64; selected bool) on the CPU."""
    lib, s = _L().lib(), _L().stream_ptr()
    B, V, K = probs.shape
    out = Carved([(B, K), (B,), (B,), (B,)], [torch.float32, torch.int32, torch.float32, torch.uint8])
    mean, pred, mx, sel = out.out
    _L().check(lib.ec_pseudo_label(_p(probs), B, V, K, thresh, consistent, min_prob, _p(mean) if with_mean else None, _p(pred), _p(mx),
                                   _p(sel), s), 'ec_pseudo_label')
    out.intact(f'pseudo_label V={V} K={K}')
    if not with_mean:
        assert bool((mean.view(torch.int32) == SENTINEL).all())
    assert bool((sel <= 1).all())
    return dict(mean=mean.cpu(), pred=pred.cpu().long(), max_prob=mx.cpu(), selected=sel.cpu().bool())


@pytest.mark.parametrize('K', ref.PL_KS)
@pytest.mark.parametrize('V', ref.PL_VIEWS)
def test_pseudo_label_planted(V, K, hip):
    """Winners, ties, dissenting views, thresholds exactly at and one fp32 step below the mean's and the smallest view's
    top, all-NaN and one-NaN rows (classify_ref.pl_inputs), under the four flag pairs: pred and selected equal to the
    float64 reference on EVERY sample, mean_probs and max_prob bit-equal for V a power of two and within one ulp
    otherwise.  With V = 1 the flags change nothing (the reference ignores them).  mean_probs = NULL is accepted."""
    inp = ref.pl_inputs(V, K)
    probs = inp.probs.cuda()
    for cons, minp in ref.PL_FLAGS:
        for thr in ref.thresholds():
            want = ref.pseudo_label64(inp.probs, thr, cons, minp)
            got = run_pseudo_label(probs, thr, cons, minp)
            if not ref.pl_same(got, want, V):
                bad = [(t, int(got['pred'][b]), int(want['pred'][b]), bool(got['selected'][b]), bool(want['selected'][b]),
                        float(got['max_prob'][b]), float(want['max_prob'][b])) for b, t in enumerate(inp.tags)
                       if not ref.pl_same({k: v[b:b + 1] for k, v in got.items()}, {k: v[b:b + 1] for k, v in want.items()}, V)]
                raise AssertionError(f'V={V} K={K} consistent={cons} min_prob={minp} thresh={thr!r}: (sample, pred got / want, '
                                     f'selected got / want, max_prob got / want) {bad}')
    with_mean = run_pseudo_label(probs, ref.PL_THRESH, 1, 1)
    without = run_pseudo_label(probs, ref.PL_THRESH, 1, 1, with_mean=False)
    assert torch.equal(without['pred'], with_mean['pred']) and torch.equal(without['selected'], with_mean['selected'])
    assert torch.equal(without['max_prob'].view(torch.int32), with_mean['max_prob'].view(torch.int32))


def test_pseudo_label_refusals(hip):
    lib, s = _L().lib(), _L().stream_ptr()
    p = torch.zeros(4 * 9 * 8, device='cuda')
    pred = torch.zeros(4, dtype=torch.int32, device='cuda')
    mx = torch.zeros(4, device='cuda')
    sel = torch.zeros(4, dtype=torch.uint8, device='cuda')

    def call(B, V, K):
        return lib.ec_pseudo_label(_p(p), B, V, K, 0.5, 1, 1, None, _p(pred), _p(mx), _p(sel), s)
    _refused(call(4, 0, 8), 'V=0 views (1..8)')
    _refused(call(4, 9, 8), 'V=9 views (1..8)')
    _refused(call(4, 4, 0), 'bad shape')
    _refused(call(-1, 4, 8), 'bad shape')
    assert lib.ec_pseudo_label(None, 0, 4, 8, 0.5, 1, 1, None, None, None, None, s) == 0       # B = 0: nothing to do
    _refused(lib.ec_pseudo_label(None, 4, 4, 8, 0.5, 1, 1, None, _p(pred), _p(mx), _p(sel), s), 'null buffer')
    assert call(4, 8, 8) == 0 and call(4, 1, 8) == 0
    torch.cuda.synchronize()


def test_classifier_nan_rows_are_labelled_as_torch_labels_them(hip):
    """The chain the NaN rule exists for: a sample without a valid view leaves ec_classify_v2 as a row of NaN
    probabilities; eventclip_amd.pseudo_label.select gives it max_prob NaN, label 0 (the first NaN) and never selects it,
    with and without test-time augmentation, exactly as oracle.pseudo_label (torch) does."""
    from eventclip_amd import pseudo_label as pl
    from oracle import pseudo_label as opl
    case = DENSE
    inp = ref.inputs(case, 0, True)
    idx = inp.row_idx.clone()
    idx[1] = -1
    feats, text, _ = _dev(inp)
    probs = run_classify(feats, text, idx.cuda(), inp.scale, 'mean', True, 'empty sample')[2]
    assert bool(torch.isnan(probs[1]).all())
    for tta in (False, True):
        p = probs.repeat_interleave(4, 0) if tta else probs
        for cons, minp in ref.PL_FLAGS:
            want = opl.select(p, 0.0, tta, bool(cons), bool(minp))
            got = pl.select(p.cuda(), 0.0, tta, bool(cons), bool(minp))
            assert torch.equal(got['pred'].cpu(), want['pred']) and int(got['pred'][1]) == 0
            assert torch.equal(got['selected'].cpu(), want['selected']) and not bool(got['selected'][1])
            assert bool(torch.isnan(got['max_prob'][1])) and bool(torch.isnan(want['max_prob'][1]))
