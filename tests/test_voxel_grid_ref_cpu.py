"""The voxel-grid yardstick (tests/voxel_grid_ref.py) without a GPU: its two restatements of the definition agree, mass is
conserved, the flags equal explicitly rewritten streams, its check catches every fault planted in a model of the
kernel, and the layers around the kernel exist: the header's entries exported, the refusals of the Python layer, the
custom op with its fake kernel, the pipeline's dispatch."""
import ctypes
import os
import re

import numpy as np
import pytest

import voxel_grid_ref as vg
from eventclip_amd import _lib, vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(vg.cases())
FLAGS = [dict(flip_x=fx, negate_p=ng, reverse_t=rv) for fx in (False, True) for ng in (False, True) for rv in (False, True)]


def _inputs(case):
    return [case['events']] + ([vg.packed(case)] if case['packable'] else [])


@pytest.mark.parametrize('name', CASES)
def test_the_two_restatements_agree(name):
    """Vectorised against event by event; every flag combination on the small cases, none and all three on the rest."""
    c = vg.cases()[name]
    small = c['shape'] == (36, 52) and name != 'many'
    for kw in (FLAGS if small else [FLAGS[0], FLAGS[-1]]):
        for mask in ((True, False) if small else (True,)):
            a = vg.oracle(c['events'], c['ranges'], c['shape'], c['bins'], mask, **kw)
            b = vg.oracle_loop(c['events'], c['ranges'], c['shape'], c['bins'], mask, **kw)
            vg.check(a, b)
            assert (a['frames'] is None) == (c['bins'] != 3)


@pytest.mark.parametrize('name', [n for n in CASES if vg.cases()[n]['packable']])
def test_float_rows_and_packed_events_agree(name):
    c = vg.cases()[name]
    for kw in (FLAGS[0], FLAGS[-1]):
        vg.check(vg.oracle(vg.packed(c), c['ranges'], c['shape'], c['bins'], **kw),
                 vg.oracle(c['events'], c['ranges'], c['shape'], c['bins'], **kw))


def test_directed_cases_hold_what_they_claim():
    cs = vg.cases()
    r = {n: vg.oracle(c['events'], c['ranges'], c['shape'], c['bins']) for n, c in cs.items() if c['shape'] == (36, 52)}
    assert r['single']['stats'][0].tolist() == (0, 1, 33 * 15625, 33 * 15625, 256) and r['single']['grid'][0, 5, 7].tolist() == [-256, 0, 0]
    assert r['single']['frames'][0, 5, 7].tolist() == [0, 128, 128] and (r['single']['frames'][0, 0, 0] == 255).all()
    st = r['same_tick']['stats'][0]
    assert st['t0'] == st['t1'] == 3 * 10 ** 6 and st['peak'] == 512 and (r['same_tick']['grid'][0, ..., 1:] == 0).all()
    assert r['same_tick']['grid'][0, 30, 9].tolist() == [0, 0, 0]          # + and - on the one tick
    for f in (0, 1):                                                      # m == 0: white under the mask, grey without
        assert r['nothing']['stats'][f].tolist() == (0 if f == 0 else 3, 0, 0, 0, 0)
        assert (r['nothing']['frames'][f] == 255).all() and (r['nothing']['grid'][f] == 0).all()
    c = cs['nothing']
    assert (vg.oracle(c['events'], c['ranges'], c['shape'], 3, background_mask=False)['frames'] == 128).all()
    g = r['ends']['grid'][0]
    assert g[1, 1].tolist() == [256, 0, 0] and g[2, 2].tolist() == [-256, 0, 0] and g[35, 51].tolist() == [256, 0, 0]
    assert g[3, 3].tolist() == [0, 0, 256] and g[5, 5].tolist() == [0, 0, -256]     # d == span: the last bin alone
    g = vg.oracle(cs['ends']['events'], cs['ends']['ranges'], (36, 52), 3, reverse_t=True)['grid'][0]
    assert g[1, 1].tolist() == [0, 0, 256] and g[3, 3].tolist() == [256, 0, 0]
    assert r['wide']['stats'][0]['t1'] - r['wide']['stats'][0]['t0'] == vg.TICK_MAX
    x, y, p, tick = vg.parse(cs['wide']['events'], (36, 52))
    assert int((tick * 7 * 256).max()) >= 2 ** 40
    x, y, p, tick = vg.parse(cs['floor_edge']['events'], (36, 52))
    assert ((tick - tick.min()) * 512 % (tick.max() - tick.min()) == 0).all() and len(tick) > 2000
    for mask, bg in ((True, 255), (False, 128)):
        fr = vg.oracle(cs['cancel']['events'], cs['cancel']['ranges'], (36, 52), 3, mask)
        assert fr['grid'][0, 4, 9].tolist() == [0, 0, 0] and fr['frames'][0, 4, 9].tolist() == [bg] * 3
        assert fr['grid'][0, 5, 9].tolist() == [256, 0, -256] and fr['frames'][0, 5, 9].tolist() == [255, 128, 0]
    assert (r['negative_only']['grid'] <= 0).all() and r['negative_only']['frames'].max() == 255
    assert (r['negative_only']['frames'][r['negative_only']['grid'].any(axis=-1)] <= 128).all()
    assert (r['skip']['stats'][0]['dropped'], r['skip']['stats'][0]['counted']) == (2, 3)
    assert (r['skip']['stats'][0]['t0'], r['skip']['stats'][0]['t1']) == (10 * 15625, 20 * 15625)
    assert sorted(map(tuple, np.argwhere(r['frac']['grid'][0].any(axis=-1)))) == [(0, 0), (3, 5), (35, 51)]
    for (shape, B), bands in vg.BANDS.items():                            # the plan the band counts were worked out from
        rows = min(shape[0], 156 * 1024 // (shape[1] * B * 4))
        assert -(-shape[0] // rows) == bands


def test_mass_is_conserved_and_agrees_with_the_histogram_oracle():
    """sum_b G[y, x, b] == 256 (positives - negatives) of the pixel, the right-hand side from the histogram oracle's
    raw counts on the same events and chunks."""
    from oracle import events as hist
    for name, N in (('cars', 1500), ('small8', 700), ('small2', 3040)):
        c = vg.cases()[name]
        _, raw, _ = hist.events2frames(c['events'], shape=c['shape'], N=N, return_counts=True)
        i0, i1 = vis.chunk_bounds(len(c['events']), N)
        for kw in (FLAGS[0], dict(reverse_t=True)):
            got = vg.oracle(c['events'], list(zip(i0, i1)), c['shape'], c['bins'], **kw)
            assert got['grid'].shape[0] == raw.shape[0]
            np.testing.assert_array_equal(got['grid'].astype(np.int64).sum(axis=-1), 256 * (raw[..., 0] - raw[..., 1]))
            np.testing.assert_array_equal(got['stats']['counted'], raw.sum(axis=(1, 2, 3)))


@pytest.mark.parametrize('name', ['small3', 'small8', 'ends', 'floor_edge', 'cars'])
def test_flags_equal_the_rewritten_stream(name):
    """Every combination of flip_x, negate_p and reverse_t against ``rewrite``; the time flip also against
    oracle.event_utils.tflip_events (reversed order, t' = t[last] - t, p' = -p) with the ranges of the reversed order."""
    from oracle import event_utils as eu
    c = vg.cases()[name]
    ev, shape, n = c['events'], c['shape'], len(c['events'])
    for kw in FLAGS:
        vg.check_rewritten(vg.oracle(ev, c['ranges'], shape, c['bins'], **kw),
                           vg.oracle(vg.rewrite(ev, shape, **kw), c['ranges'], shape, c['bins']))
    np.testing.assert_array_equal(vg.rewrite(ev, shape, flip_x=True), eu.hflip_events(ev.copy(), shape))
    ev = ev[np.argsort(ev[:, 2], kind='stable')]                          # the flip takes t[last] for the largest
    want = vg.oracle(eu.tflip_events(ev.copy()), [(n - e, n - b) for b, e in c['ranges']], shape, c['bins'])
    vg.check_rewritten(vg.oracle(ev, c['ranges'], shape, c['bins'], reverse_t=True, negate_p=True), want)


def test_the_grid_does_not_depend_on_the_order_of_the_events():
    for name in ('small3', 'wide', 'cars'):
        c = vg.cases()[name]
        assert len(c['ranges']) == 1 or name == 'small3'
        b, e = c['ranges'][0]
        ev = c['events'][b:e]
        shuffled = ev[np.random.default_rng(1).permutation(len(ev))]
        for kw in (FLAGS[0], FLAGS[-1]):
            vg.check(vg.oracle(shuffled, [(0, len(ev))], c['shape'], c['bins'], **kw),
                     vg.oracle(ev, [(0, len(ev))], c['shape'], c['bins'], **kw))


# which case and settings show each fault
PLANTED = dict(end_event_out_of_range=('ends', {}), end_event_dropped=('ends', {}), round_not_floor=('small3', {}),
               t0_over_all_events=('skip', {}), reverse_mirrored=('small3', dict(reverse_t=True)),
               peak_per_band=('small3', {}), lost_sign=('small3', {}), mask_any_zero=('small3', {}))


def test_the_model_of_the_kernel_computes_the_definition():
    for name in CASES:
        c = vg.cases()[name]
        if c['shape'][0] * c['shape'][1] > 50000 or name == 'many':
            continue
        for kw in (dict(), dict(reverse_t=True, negate_p=True, background_mask=False)):
            for rows in (7, c['shape'][0]):
                got = vg.kernel_model(c['events'], c['ranges'], c['shape'], c['bins'], rows_per_band=rows, **kw)
                vg.check(got, vg.oracle(c['events'], c['ranges'], c['shape'], c['bins'], **kw))


@pytest.mark.parametrize('fault', vg.FAULTS)
def test_the_check_catches_a_planted_fault(fault):
    assert set(PLANTED) == set(vg.FAULTS)
    name, kw = PLANTED[fault]
    c = vg.cases()[name]
    want = vg.oracle(c['events'], c['ranges'], c['shape'], c['bins'], **kw)
    vg.check(vg.kernel_model(c['events'], c['ranges'], c['shape'], c['bins'], **kw), want)
    with pytest.raises(AssertionError):
        vg.check(vg.kernel_model(c['events'], c['ranges'], c['shape'], c['bins'], fault=fault, **kw), want)
    if fault in ('peak_per_band', 'mask_any_zero'):                       # a fault of the bytes alone: the grid passes
        got = vg.kernel_model(c['events'], c['ranges'], c['shape'], c['bins'], fault=fault, **kw)
        vg.check(dict(grid=got['grid'], stats=got['stats']), want)


# ---- the layers around the kernel ----
def test_header_declares_the_entries_and_the_library_exports_them(tmp_path):
    text = open(vis.VOXEL_HEADER).read()
    names = sorted(set(re.findall(r'EC_API\s+[\w\s\*]+?\b(ec_\w+)\s*\(', text)))
    assert names == ['ec_events_to_voxel_grid', 'ec_events_to_voxel_grid_packed', 'ec_voxel_grid_bands'] == sorted(vis.VOXEL_SIGNATURES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f'{n} declared in include/eventclip_voxel_grid.h but not exported'
    assert _lib.lib().ec_version() == _lib.ABI_VERSION >= 610
    for step in ('1. parse', '2. t0, t1', '3. position', '4. grid', '5. peak', '6. bytes', '7. time flip', 'hot'):
        assert step in text, f'the header states the definition step by step: {step!r} is missing'
    # the bindings against what the host compiler makes of the same text
    import shutil
    import subprocess
    cc = shutil.which(os.environ.get('CC', 'cc'))
    assert cc is not None, 'no host C compiler'
    body, want = [], []
    for c_name, cls in (('ec_voxel_grid_params', vis.EcVoxelGridParams), ('ec_voxel_stats', vis.EcVoxelStats)):
        body.append(f'printf("S {c_name} %zu\\n", sizeof({c_name}));')
        want.append(f'S {c_name} {ctypes.sizeof(cls)}')
        for field, _ in cls._fields_:
            body.append(f'printf("F {field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name} *)0)->{field}));')
            want.append(f'F {field} {getattr(cls, field).offset} {getattr(cls, field).size}')
    body.append('printf("E %d %d %d\\n", (int)EC_VOXEL_MIN_BINS, (int)EC_VOXEL_MAX_BINS, (int)EC_VOXEL_MAX_FRAME_EVENTS);')
    want.append('E 2 8 8388607')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eventclip_voxel_grid.h"\nint main(void) {\n'
                   + '\n'.join(body) + '\nreturn 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'prog')], check=True)
    assert subprocess.run([str(tmp_path / 'prog')], capture_output=True, text=True, check=True).stdout.splitlines() == want
    assert [f for f, _ in vis.EcVoxelStats._fields_] == list(vis.VOXEL_STATS_DTYPE.names) == list(vg.STATS)
    assert ctypes.sizeof(vis.EcVoxelStats) == vis.VOXEL_STATS_DTYPE.itemsize == 20
    assert [f for f, _ in vis.EcVoxelGridParams._fields_] == ['H', 'W', 'bins', 'background_mask', 'flip_x', 'negate_p', 'reverse_t',
                                                              'max_frame_events', 'total_events']
    for n in names[:2]:
        assert vis.VOXEL_SIGNATURES[n][1][3] is ctypes.POINTER(vis.EcVoxelGridParams)
        assert vis.VOXEL_SIGNATURES[n][1][6] is ctypes.c_void_p                    # EC_DEVICE stats: an address


def test_the_band_query_and_the_host_side_refusals():
    """ec_voxel_grid_bands is host only: the band counts the GPU tests name, and 0 for what the entry points refuse.  The
    entry points check their arguments before they touch the device: every refusal is EC_ERR_INVALID with its message."""
    for (shape, B), bands in vg.BANDS.items():
        assert vis.voxel_grid_bands(shape, B) == bands, (shape, B)
    assert vis.voxel_grid_bands((8, 8), 1) == vis.voxel_grid_bands((8, 8), 9) == vis.voxel_grid_bands((0, 8), 3) == 0
    assert vis.voxel_grid_bands((8, 13312), 3) == 8 and vis.voxel_grid_bands((8, 13313), 3) == 0       # 156 KB / 12 bytes
    lib = _lib.lib()
    big = np.zeros(64, np.uint8)                                          # an aligned address; no refused call reads it
    addr = big.ctypes.data + (-big.ctypes.data) % 16

    def prm(shape=(8, 8), bins=3, max_frame_events=0):
        p = vis.voxel_grid_params(shape, 3, True, 0, False, False, False, 0)
        p.bins, p.max_frame_events = bins, max_frame_events
        return p

    f, p = 'ec_events_to_voxel_grid', 'ec_events_to_voxel_grid_packed'
    for name, args, msg in (
            (f, (None, addr, 1, prm(), addr, None), b'null buffer'),
            (f, (addr, None, 1, prm(), addr, None), b'null buffer'),
            (p, (addr, addr, 1, prm(), None, None), b'neither frames nor grid'),
            (f, (addr, addr, 1, None, addr, None), b'params is null'),
            (f, (addr + 4, addr, 1, prm(), addr, None), b'16-byte aligned'),
            (p, (addr + 4, addr, 1, prm(), addr, None), b'8-byte aligned'),
            (f, (addr, addr, 1, prm(bins=1), None, addr), b'bins=1 outside 2 .. 8'),
            (f, (addr, addr, 1, prm(bins=9), None, addr), b'bins=9 outside 2 .. 8'),
            (f, (addr, addr, 1, prm(bins=2), addr, addr), b'frames need bins == 3, not 2'),
            (p, (addr, addr, 1, prm(bins=8), addr, None), b'frames need bins == 3, not 8'),
            (f, (addr, addr, 1, prm(max_frame_events=8388608), addr, None), b'max_frame_events=8388608 above 8388607'),
            (f, (addr, addr, 1, prm((8, 13313)), addr, None), b'W=13313 too wide for one LDS row band at bins=3'),
            (f, (addr, addr, -1, prm(), addr, None), b'F=-1')):
        events, rng, F, pr, frames, grid = args
        rc = getattr(lib, name)(events, rng, F, ctypes.byref(pr) if pr is not None else None, frames, grid, None, None)
        assert rc == _lib.EC_ERR_INVALID, msg
        assert msg in lib.ec_last_error(), (msg, lib.ec_last_error())
    assert lib.ec_events_to_voxel_grid(None, None, 0, ctypes.byref(prm()), None, None, None, None) == _lib.EC_OK     # F == 0
    # the Python layer says the same before any launch
    for bins in (1, 9):
        with pytest.raises(ValueError, match='bins'):
            vis.voxel_grid_params((8, 8), bins, True, 0, False, False, False, 0)
    with pytest.raises(ValueError, match='max_frame_events'):
        vis.voxel_grid_params((8, 8), 3, True, 8388608, False, False, False, 0)
    p8 = vis.voxel_grid_params((100, 120), 8, True, 8388607, True, False, True, 11)
    assert (p8.H, p8.W, p8.bins, p8.background_mask, p8.flip_x, p8.negate_p, p8.reverse_t) == (100, 120, 8, 1, 1, 0, 1)
    assert (p8.max_frame_events, p8.total_events) == (8388607, 11)


def test_voxel_stays_refused_and_voxel_grid_is_accepted():
    from eventclip_amd.event2img import Event2ImagePipeline
    assert 'voxel_grid' in vis.CONVERT_METHODS and 'voxel' not in vis.CONVERT_METHODS
    ev = vg.cases()['small3']['events']
    with pytest.raises(NotImplementedError):
        vis.events2frames(ev, 'event_count', 'voxel', shape=(36, 52), N=1000)
    with pytest.raises(AssertionError):
        vis.events2frames(ev, 'time', 'voxel_grid', shape=(36, 52), N=1000)
    qa = dict(max_imgs=2, N=20000, split_method='event_count', convert_method='voxel_grid', grayscale=True,
              count_non_zero=False, background_mask=True, thresh=3., float_stage='float64')     # (the last three: ignored)
    pipe = Event2ImagePipeline((180, 240), 225000, qa)
    assert (pipe.event_rep, pipe.bins) == ('voxel_grid', 3)
    assert Event2ImagePipeline((180, 240), 225000, dict(qa, bins=3)).bins == 3
    with pytest.raises(ValueError, match='bins=5'):
        Event2ImagePipeline((180, 240), 225000, dict(qa, bins=5))
    with pytest.raises(NotImplementedError):
        Event2ImagePipeline((180, 240), 225000, dict(qa, convert_method='voxel'))
    assert Event2ImagePipeline((180, 240), 225000, dict(qa, convert_method='event_histogram', bins=5)).event_rep == 'event_histogram'


def test_custom_op_is_registered_with_a_fake_kernel():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    assert 'events_to_voxel_grid' in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, 'events_to_voxel_grid')
    with FakeTensorMode():
        fr = torch.zeros(5, 2, dtype=torch.int64, device='cuda')
        for ev in (torch.empty(1000, 4, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')):
            frames = torch.ops.eventclip_hip.events_to_voxel_grid(ev, fr, 180, 240, 3, True, 0, False, False, True, 0)
            assert frames.shape == (5, 180, 240, 3) and frames.dtype == torch.uint8
    with pytest.raises(NotImplementedError):                             # no CPU kernel
        torch.ops.eventclip_hip.events_to_voxel_grid(torch.zeros(4, 4), torch.zeros(1, 2, dtype=torch.int64), 8, 8, 3, True, 0,
                                                     False, False, False, 0)
