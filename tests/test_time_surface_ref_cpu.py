"""The time-surface yardstick (tests/time_surface_ref.py) without a GPU: its two restatements of the definition agree, the
flags equal the explicit flips, its check catches every fault planted in a model of the kernel, and the layers around
the kernel exist: the header's two entries exported, the custom op with its fake kernel, the pipeline's dispatch."""
import ctypes
import os
import re

import numpy as np
import pytest

import time_surface_ref as ts
from eventclip_amd import _lib, vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(ts.cases())
FLAGS = [dict(flip_x=fx, negate_p=ng, reverse_t=rv) for fx in (False, True) for ng in (False, True) for rv in (False, True)]


def _inputs(case):
    return [case['events']] + ([ts.packed(case)] if case['packable'] else [])


@pytest.mark.parametrize('name', CASES)
def test_the_two_restatements_agree(name):
    """Vectorised against event by event, float rows and packed events, both decays; every flag combination on the
    smallest random case and on the directed ones that were built for a flag."""
    c = ts.cases()[name]
    flags = FLAGS if name in ('n_cars', 'frac', 'skip', 'sentinel') else [FLAGS[0], FLAGS[-1]]
    for events in _inputs(c):
        for kw in flags:
            for decay, gray, mask in (('linear', True, True), ('exp', False, False)):
                a = ts.oracle(events, c['ranges'], c['shape'], decay, c['tau'], gray, mask, **kw)
                b = ts.oracle_loop(events, c['ranges'], c['shape'], decay, c['tau'], gray, mask, **kw)
                for k in ('frames', 'pre', 'last', 'stats'):
                    np.testing.assert_array_equal(a[k], b[k], err_msg=f'{k} {kw} {decay}')
                assert ts.check(a, b, decay) == 0           # no pixel of any case sits in the tie window
    a = ts.oracle(c['events'], c['ranges'], c['shape'])
    if c['packable']:
        np.testing.assert_array_equal(a['frames'], ts.oracle(ts.packed(c), c['ranges'], c['shape'])['frames'])


def test_directed_cases_hold_what_they_claim():
    cs = ts.cases()
    st = ts.oracle(cs['skip']['events'], cs['skip']['ranges'], (36, 52))['stats'][0]
    assert (st['dropped'], st['counted'], st['t0'], st['t1']) == (2, 3, 10 * 15625, 20 * 15625)
    r = ts.oracle(cs['sentinel']['events'], cs['sentinel']['ranges'], (36, 52), background_mask=False)
    assert r['stats']['t0'][0] == 0 and r['stats']['t1'][0] == ts.TICK_MAX
    assert r['last'][0, 1, 1, 0] == 0 and r['last'][0, 0, 0, 0] == -1 and r['last'][0, 3, 3, 0] == ts.TICK_MAX
    r = ts.oracle(cs['same_tick']['events'], cs['same_tick']['ranges'], (36, 52), background_mask=False)
    assert r['stats']['t0'][0] == r['stats']['t1'][0] == 3 * 10 ** 6 and r['frames'][0, 4, 3].tolist() == [254] * 3
    for mask, bg in ((True, 255), (False, 0)):
        r = ts.oracle(cs['lengths']['events'], cs['lengths']['ranges'], (36, 52), background_mask=mask)
        assert (r['frames'][0] == bg).all() and r['stats'][0].tolist() == (0, 0, 0, 0) and (r['last'][0] == -1).all()
    r = ts.oracle(cs['frac']['events'], cs['frac']['ranges'], (36, 52))
    assert sorted(map(tuple, np.argwhere(r['last'][0] >= 0))) == [(0, 0, 1), (3, 5, 0), (35, 51, 0)] and r['stats']['dropped'][0] == 1
    r = ts.oracle(cs['frac']['events'], cs['frac']['ranges'], (36, 52), flip_x=True)
    assert sorted(map(tuple, np.argwhere(r['last'][0] >= 0))) == [(0, 51, 1), (3, 45, 0), (35, 0, 0)]
    assert len(cs['exp_edge']['events']) > 4        # the search found ages that tell a float32 exp
    for g in ts.GEOMETRIES:                 # every row holds an event: both sides of every band boundary
        assert (ts.oracle(**{k: ts.case_rows(g)[k] for k in ('events', 'ranges', 'shape')})['last'].max(axis=(0, 2, 3)) >= 0).all()


@pytest.mark.parametrize('name', ['rows36x52', 'pile', 'many', 'n_cars'])
def test_flags_equal_the_explicit_flips(name):
    """flip_x against oracle.event_utils.hflip_events on the array; reverse_t + negate_p against tflip_events (reversed
    order, t' = t[last] - t, p' = -p) with the ranges taken on the reversed order.  The random case's timestamps are put
    on the 1/64 s grid first: there float32's t[last] - t is exact and the flipped array's ticks are tick[last] - tick."""
    from oracle import event_utils as eu
    c = ts.cases()[name]
    ev, shape, n = c['events'].copy(), c['shape'], len(c['events'])
    scale = 1000 if name == 'n_cars' else 1                             # 0.3 s of random timestamps -> 300 s on the grid
    ev[:, 2] = np.sort(np.rint(ev[:, 2] * scale * 64) / 64)             # (sorted: the flip takes t[last] for the largest)
    for decay in ('linear', 'exp'):
        kw = dict(decay=decay, tau=c['tau'] * scale, grayscale=False)
        want = ts.oracle(eu.hflip_events(ev.copy(), shape), c['ranges'], shape, **kw)
        ts.check(ts.oracle(ev, c['ranges'], shape, flip_x=True, **kw), want, decay)
        want = ts.oracle(eu.tflip_events(ev.copy()), [(n - e, n - b) for b, e in c['ranges']], shape, **kw)
        got = ts.oracle(ev, c['ranges'], shape, reverse_t=True, negate_p=True, **kw)
        np.testing.assert_array_equal(got['frames'], want['frames'])
        np.testing.assert_array_equal(got['last'] >= 0, want['last'] >= 0)
        for k in ('dropped', 'counted'):
            np.testing.assert_array_equal(got['stats'][k], want['stats'][k])
        np.testing.assert_array_equal(got['stats']['t1'] - got['stats']['t0'], want['stats']['t1'] - want['stats']['t0'])


# which case and settings show each fault
PLANTED = dict(skipped_event_moves_t1=('skip', {}), tick0_is_untouched=('sentinel', {}), min_for_max=('pile', {}),
               band_last_row_missing=('rows36x52', {}), w_not_clipped=('n_cars', dict(background_mask=True)),
               exp_float32=('exp_edge', dict(decay='exp', background_mask=False)))


def test_the_model_of_the_kernel_computes_the_definition():
    for name in CASES:
        c = ts.cases()[name]
        for kw in (dict(decay='linear'), dict(decay='exp', reverse_t=True, grayscale=False, background_mask=False)):
            for rows in (7, c['shape'][0]):
                got = ts.kernel_model(c['events'], c['ranges'], c['shape'], tau=c['tau'], rows_per_band=rows, **kw)
                ts.check(got, ts.oracle(c['events'], c['ranges'], c['shape'], tau=c['tau'], **kw), kw['decay'])


@pytest.mark.parametrize('fault', ts.FAULTS)
def test_the_check_catches_a_planted_fault(fault):
    assert set(PLANTED) == set(ts.FAULTS)
    name, kw = PLANTED[fault]
    c = ts.cases()[name]
    kw = dict(dict(decay='linear', tau=c['tau']), **kw)
    want = ts.oracle(c['events'], c['ranges'], c['shape'], **kw)
    ts.check(ts.kernel_model(c['events'], c['ranges'], c['shape'], **kw), want, kw['decay'])
    with pytest.raises(AssertionError):
        ts.check(ts.kernel_model(c['events'], c['ranges'], c['shape'], fault=fault, **kw), want, kw['decay'])


def test_the_check_allows_a_tie_either_way_and_only_there():
    want = dict(frames=np.array([[[[3, 10, 200]]]], np.uint8), pre=np.array([[[[2.5 + 2e-10, 10.2, 199.5000001]]]]))
    for b, ok in ((2, True), (3, True), (4, False)):
        got = dict(frames=np.array([[[[b, 10, 200]]]], np.uint8))
        if ok:
            assert ts.check(got, want, 'exp') == 1
        else:
            with pytest.raises(AssertionError):
                ts.check(got, want, 'exp')
    with pytest.raises(AssertionError):                                  # 1e-7 from the tie is outside the window
        ts.check(dict(frames=np.array([[[[3, 10, 199]]]], np.uint8)), want, 'exp')
    with pytest.raises(AssertionError):                                  # linear frames have no window
        ts.check(dict(frames=np.array([[[[2, 10, 200]]]], np.uint8)), want, 'linear')
    many = dict(frames=np.zeros((1, 3, 3, 3), np.uint8), pre=np.full((1, 3, 3, 3), 0.5))
    with pytest.raises(AssertionError, match='another seed'):
        ts.check(dict(frames=many['frames']), many, 'exp')


# ---- the layers around the kernel ----
def test_header_declares_the_entries_and_the_library_exports_them(tmp_path):
    text = open(vis.SURFACE_HEADER).read()
    names = sorted(set(re.findall(r'EC_API\s+[\w\s\*]+?\b(ec_\w+)\s*\(', text)))
    assert names == ['ec_events_to_time_surface', 'ec_events_to_time_surface_packed'] == sorted(vis.SURFACE_SIGNATURES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f'{n} declared in include/eventclip_time_surface.h but not exported'
    assert _lib.lib().ec_version() == _lib.ABI_VERSION >= 609
    # the bindings against what the host compiler makes of the same text
    import shutil
    import subprocess
    cc = shutil.which(os.environ.get('CC', 'cc'))
    if cc is None:
        pytest.skip('no cc')
    body, want = [], []
    for c_name, cls in (('ec_time_surface_params', vis.EcTimeSurfaceParams), ('ec_surface_stats', vis.EcSurfaceStats)):
        body.append(f'printf("S {c_name} %zu\\n", sizeof({c_name}));')
        want.append(f'S {c_name} {ctypes.sizeof(cls)}')
        for field, _ in cls._fields_:
            body.append(f'printf("F {field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name} *)0)->{field}));')
            want.append(f'F {field} {getattr(cls, field).offset} {getattr(cls, field).size}')
    for k, v in vis.DECAYS.items():
        body.append(f'printf("E %d\\n", (int)EC_DECAY_{k.upper()});')
        want.append(f'E {v}')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eventclip_time_surface.h"\nint main(void) {\n'
                   + '\n'.join(body) + '\nreturn 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'prog')], check=True)
    assert subprocess.run([str(tmp_path / 'prog')], capture_output=True, text=True, check=True).stdout.splitlines() == want
    assert ctypes.sizeof(vis.EcSurfaceStats) == vis.SURFACE_STATS_DTYPE.itemsize == 16
    for n in names:
        assert vis.SURFACE_SIGNATURES[n][1][3] is ctypes.POINTER(vis.EcTimeSurfaceParams)
        assert vis.SURFACE_SIGNATURES[n][1][6] is ctypes.c_void_p                  # EC_DEVICE stats: an address


def test_custom_op_is_registered_with_a_fake_kernel():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    assert 'events_to_time_surface' in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, 'events_to_time_surface')
    with FakeTensorMode():
        fr = torch.zeros(5, 2, dtype=torch.int64, device='cuda')
        for ev in (torch.empty(1000, 4, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')):
            frames = torch.ops.eventclip_hip.events_to_time_surface(ev, fr, 180, 240, 'exp', 0.03, [255, 0, 0], [0, 0, 255],
                                                                    True, 0, False, False, True, 0)
            assert frames.shape == (5, 180, 240, 3) and frames.dtype == torch.uint8
    with pytest.raises(NotImplementedError):                             # no CPU kernel
        torch.ops.eventclip_hip.events_to_time_surface(torch.zeros(4, 4), torch.zeros(1, 2, dtype=torch.int64), 8, 8, 'linear',
                                                       0.03, [127] * 3, [127] * 3, True, 0, False, False, False, 0)


def test_pipeline_and_params_accept_the_representation():
    from eventclip_amd.event2img import Event2ImagePipeline
    qa = dict(max_imgs=2, N=20000, split_method='event_count', convert_method='time_surface', grayscale=True,
              count_non_zero=False, background_mask=True, thresh=3., float_stage='float64')     # (the last three: ignored)
    pipe = Event2ImagePipeline((180, 240), 225000, qa)
    assert (pipe.event_rep, pipe.decay, pipe.tau) == ('time_surface', 'linear', 0.03)
    pipe = Event2ImagePipeline((180, 240), 225000, dict(qa, decay='exp', tau=0.05))
    assert (pipe.decay, pipe.tau) == ('exp', 0.05)
    assert Event2ImagePipeline((180, 240), 225000, dict(qa, convert_method='event_histogram')).event_rep == 'event_histogram'
    with pytest.raises(NotImplementedError):
        Event2ImagePipeline((180, 240), 225000, dict(qa, convert_method='voxel'))
    with pytest.raises(ValueError):
        Event2ImagePipeline((180, 240), 225000, dict(qa, decay='quadratic'))
    p = vis.time_surface_params((100, 120), [255, 0, 0], [0, 0, 255], 'exp', 0.03, True, 7, True, False, True, 11)
    assert (p.H, p.W, p.decay, p.tau_us, p.flip_x, p.negate_p, p.reverse_t) == (100, 120, 1, 0.03 * 1e6, 1, 0, 1)
    assert (list(p.red), list(p.blue), p.max_frame_events, p.total_events) == ([255, 0, 0], [0, 0, 255], 7, 11)
    with pytest.raises(ValueError):
        vis.time_surface_params((100, 120), [0] * 3, [0] * 3, 'voxel', 0.03, True, 0, False, False, False, 0)
