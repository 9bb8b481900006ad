"""The time-surface kernel (csrc/events.hip: time_surface_kernel) and the layers above it on the MI355X, against the
float64 restatement of the definition in tests/time_surface_ref.py: every case of its tables, float rows and packed
events, both decays; the surface, t0, t1, dropped and counted exactly, the bytes by ``ts.check``."""
import ctypes
import functools

import numpy as np
import pytest

import time_surface_ref as ts

pytestmark = pytest.mark.gpu

GUARD = 0xA5
NO_FLAGS = dict(flip_x=False, negate_p=False, reverse_t=False)
ALL_FLAGS = [dict(flip_x=fx, negate_p=ng, reverse_t=rv) for fx in (False, True) for ng in (False, True) for rv in (False, True)]


@functools.lru_cache(None)
def want(name, packed, decay, grayscale, background_mask, flags):
    """The oracle's answer, computed once and shared (float rows and packed events have their own: the same, which
    test_float_rows_and_packed_events_give_the_same_bytes pins on the kernel's side)."""
    c = ts.cases()[name]
    return ts.oracle(ts.packed(c) if packed else c['events'], c['ranges'], c['shape'], decay, c['tau'], grayscale,
                     background_mask, **dict(flags))


def run(name, packed, decay, grayscale=True, background_mask=True, **flags):
    """Straight to the C ABI with every output, each buffer prefilled with a guard pattern and one frame longer than
    the launch writes; -> dict(frames, last, stats) as numpy."""
    import torch
    from eventclip_amd import _lib, vis
    c = ts.cases()[name]
    H, W = c['shape']
    F = len(c['ranges'])
    ev = torch.from_numpy(ts.packed(c).view(np.int64) if packed else c['events']).cuda()
    rng = torch.tensor(c['ranges'], dtype=torch.int64).reshape(-1, 2).cuda()
    frames = torch.full((F + 1, H, W, 3), GUARD, dtype=torch.uint8, device='cuda')
    last = torch.full((F + 1, H, W, 2), -0x5A5A5A5A, dtype=torch.int32, device='cuda')
    stats = torch.full((F + 1, ctypes.sizeof(vis.EcSurfaceStats)), GUARD, dtype=torch.uint8, device='cuda')
    red, blue = vis.colour_map(grayscale)
    prm = vis.time_surface_params(c['shape'], red, blue, decay, c['tau'], background_mask, max(e - b for b, e in c['ranges']),
                                  flags.get('flip_x', False), flags.get('negate_p', False), flags.get('reverse_t', False),
                                  sum(e - b for b, e in c['ranges']))
    _lib.launch('ec_events_to_time_surface_packed' if packed else 'ec_events_to_time_surface', ev, rng, F, prm, frames, last, stats)
    torch.cuda.synchronize()
    assert (frames[F] == GUARD).all() and (last[F] == -0x5A5A5A5A).all() and (stats[F] == GUARD).all(), 'wrote past the last frame'
    return dict(frames=frames[:F].cpu().numpy(), last=last[:F].cpu().numpy(),
                stats=stats[:F].cpu().numpy().view(vis.SURFACE_STATS_DTYPE).reshape(F))


def run_and_check(name, packed, decay, grayscale=True, background_mask=True, **flags):
    got = run(name, packed, decay, grayscale, background_mask, **flags)
    full = dict(NO_FLAGS, **flags)
    ts.check(got, want(name, packed, decay, grayscale, background_mask, tuple(sorted(full.items()))), decay)
    return got


DIRECTED = [n for n in sorted(ts.cases()) if n not in ('n_cars', 'n_caltech', 'n_imagenet')]


@pytest.mark.parametrize('name', DIRECTED)
def test_directed_cases(name, hip):
    """rows* at the four geometries (one band, one band, 3 bands, 16 bands: an event on both sides of every band boundary)
    and at an odd one, off the four-pixel store path (rows37x53, odd); the frame lengths around the load unroll (the empty
    frame: all background, zero stats); pile, sentinel, same_tick, skip, frac, exp_edge; the 600 frames that trip the
    grid.  Forward and with all three flags."""
    c = ts.cases()[name]
    for packed in ((False, True) if c['packable'] else (False,)):
        for decay, gray, mask in (('linear', True, True), ('exp', False, False)):
            for flags in (NO_FLAGS, ALL_FLAGS[-1]):
                got = run_and_check(name, packed, decay, gray, mask, **flags)
            if name == 'lengths':                                         # its first frame is the empty one
                assert (got['frames'][0] == (255 if mask else 0)).all() and (got['last'][0] == -1).all()
                assert got['stats'][0].tolist() == (0, 0, 0, 0)


@pytest.mark.parametrize('name,combos', [('n_cars', 'all'), ('n_caltech', 'some'), ('n_imagenet', 'some')])
def test_random_cases(name, combos, hip):
    """make_events(seed=7) at the three dataset geometries; gray and RGB, mask on and off, every flag combination at the
    smallest."""
    for packed in (False, True):
        for decay in ('linear', 'exp'):
            for gray, mask in ((True, True), (False, False)) if combos == 'some' else ((True, True), (False, False), (True, False), (False, True)):
                run_and_check(name, packed, decay, gray, mask)
    for flags in (ALL_FLAGS if combos == 'all' else ALL_FLAGS[-1:]):
        run_and_check(name, False, 'exp', False, True, **flags)
        run_and_check(name, True, 'linear', True, False, **flags)


@pytest.mark.parametrize('name', ['rows180x240', 'sentinel', 'many', 'n_cars', 'n_imagenet'])
def test_float_rows_and_packed_events_give_the_same_bytes(name, hip):
    for decay in ('linear', 'exp'):
        a, b = run(name, False, decay, False, True, reverse_t=True), run(name, True, decay, False, True, reverse_t=True)
        for k in ('frames', 'last', 'stats'):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_numpy_drop_in_and_production_op(hip):
    """vis.events2frames(..., 'time_surface') chunks by N like the histogram path and raises on events outside the
    sensor; the production form (the custom op, frames only) gives the debug form's bytes; the refused methods stay
    refused."""
    import torch
    from eventclip_amd import vis
    from eventclip_amd.synthetic import make_events
    ev = make_events(52000, (100, 120), seed=7)
    idx0, idx1 = vis.chunk_bounds(len(ev), 20000)
    assert len(idx0) == 3 and idx0[-1] == 32000                           # the overlapping last chunk
    for kw in (dict(), dict(decay='exp', tau=0.05, grayscale=False, background_mask=False, thresh=2., count_non_zero=True)):
        got = vis.events2frames(ev, 'event_count', 'time_surface', shape=(100, 120), N=20000, **dict(kw))
        w = ts.oracle(ev, list(zip(idx0, idx1)), (100, 120), kw.get('decay', 'linear'), kw.get('tau', 0.03),
                      kw.get('grayscale', True), kw.get('background_mask', True))
        ts.check(dict(frames=got), w, kw.get('decay', 'linear'))
    d = dict(x=ev[:, 0], y=ev[:, 1], t=ev[:, 2], p=ev[:, 3])
    np.testing.assert_array_equal(vis.events2frames(d, 'event_count', 'time_surface', shape=(100, 120), N=20000),
                                  vis.events2frames(ev, 'event_count', 'time_surface', shape=(100, 120), N=20000))
    with pytest.raises(ValueError, match='outside the sensor'):
        vis.events2frames(ts.cases()['skip']['events'], 'event_count', 'time_surface', shape=(36, 52), N=100)
    with pytest.raises(NotImplementedError):
        vis.events2frames(ev, 'event_count', 'voxel', shape=(100, 120), N=20000)
    with pytest.raises(AssertionError):
        vis.events2frames(ev, 'time', 'time_surface', shape=(100, 120), N=20000)
    # production form against debug form, packed too
    c = ts.cases()['n_caltech']
    rng = torch.tensor(c['ranges'], dtype=torch.int64).cuda()
    for events in (torch.from_numpy(c['events']).cuda(), torch.from_numpy(ts.packed(c).view(np.int64)).cuda()):
        a = vis.time_surface_device(events, rng, c['shape'], decay='exp', tau=c['tau'], reverse_t=True)
        b, last, stats = vis.time_surface_device(events, rng, c['shape'], decay='exp', tau=c['tau'], reverse_t=True,
                                                 return_last=True, return_stats=True)
        assert torch.equal(a, b) and stats['counted'][0] == 20000 and last.shape == (1, 180, 240, 2)


def _grid_samples(n_list, shape, seed):
    """Samples with sorted timestamps on the 1/64 s grid (see time_surface_ref: explicit flips are exact there)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in n_list:
        ev = ts._scatter(n, shape, int(rng.integers(1 << 30)), 2000)
        ev[:, 2] = np.sort(ev[:, 2])
        out.append(ev)
    return out


def test_pipeline_views_against_explicit_flips(hip):
    """Event2ImagePipeline(convert_method='time_surface'): hflip is flip_x, tflip is reverse_t + negate_p on the stored
    rows with the reversed ranges of plan() -- against the oracle on arrays flipped by oracle.event_utils; tta(), the
    patch-row and frames_u8 outputs and the HostFeeder run behind it unchanged."""
    import torch
    from eventclip_amd import vis
    from eventclip_amd.event2img import Event2ImagePipeline
    from oracle import event_utils as eu
    shape, N = (36, 52), 300
    qa = dict(max_imgs=4, N=N, split_method='event_count', convert_method='time_surface', grayscale=False,
              background_mask=True, decay='exp', tau=8.0)
    samples = _grid_samples([1100, 250, 701], shape, seed=5)      # 4 (the last overlapping), 1 and 2 frames
    pipe = Event2ImagePipeline(shape, 1200, qa, n_px=32)
    for hflip, tflip in ((False, False), (True, False), (False, True), (True, True)):
        n_events = [len(s) for s in samples]
        fr, ri, vm = pipe.plan(n_events, tflip=tflip)
        ev_d = torch.from_numpy(np.concatenate(samples)).cuda()
        got = pipe.frames(ev_d, fr.cuda(), hflip=hflip, tflip=tflip).cpu().numpy()
        frames = []
        for s in samples:
            e = s.copy()
            e = eu.hflip_events(e, shape) if hflip else e
            e = eu.tflip_events(e) if tflip else e
            i0, i1 = vis.chunk_bounds(len(e), N)
            frames.append(ts.oracle(e, list(zip(i0, i1)), shape, 'exp', 8.0, False, True))
        w = dict(frames=np.concatenate([f['frames'] for f in frames]), pre=np.concatenate([f['pre'] for f in frames]))
        assert got.shape == w['frames'].shape == (4 + 1 + 2, 36, 52, 3)
        ts.check(dict(frames=got), w, 'exp')
    views = pipe.tta(samples)
    assert len(views) == 4 and all(v['img'].shape == (3, 4, 3, 32, 32) for v in views)
    assert not torch.equal(views[0]['img'], views[2]['img'])
    packed = [vis.pack_events(s) for s in samples]
    assert torch.equal(pipe(packed, tflip=True)['img'], views[2]['img'])
    u8 = Event2ImagePipeline(shape, 1200, qa, n_px=32, frames_u8=True)(samples)
    assert u8['frames_u8'].shape == (7, 32, 32, 3) and u8['frames_u8'].dtype == torch.uint8
    rows = Event2ImagePipeline(shape, 1200, qa, n_px=32, patch=16, kpad=1536)(samples)
    assert rows['patches'].shape == (7, 4, 1536)
    fed = list(pipe.stream([samples, samples[:2]]))
    assert len(fed) == 2 and torch.equal(fed[0]['img'], views[0]['img']) and fed[1]['img'].shape[0] == 2
    pipe.strict = True
    with pytest.raises(ValueError, match='outside the sensor'):
        pipe([ts.cases()['skip']['events']])


def test_refusals(hip):
    """EC_ERR_INVALID with its message for: null buffers, misaligned events, a W too wide for one LDS row, an unknown
    decay, tau_us <= 0 in exp mode; F == 0 is EC_OK whatever the buffers."""
    import torch
    from eventclip_amd import _lib, vis
    lib = _lib.lib()
    ev = torch.zeros((64, 4), dtype=torch.float32, device='cuda')
    pk = torch.zeros((64,), dtype=torch.int64, device='cuda')
    rng = torch.tensor([[0, 64]], dtype=torch.int64, device='cuda')
    frames = torch.full((2, 8, 8, 3), GUARD, dtype=torch.uint8, device='cuda')

    def prm(shape=(8, 8), decay='linear', tau=0.03):
        return vis.time_surface_params(shape, [127] * 3, [127] * 3, decay, tau, True, 0, False, False, False, 0)

    def call(name, events, r, F, p, out):
        return getattr(lib, name)(events, r, F, ctypes.byref(p) if p is not None else None, out, None, None, _lib.stream_ptr())

    f, p = 'ec_events_to_time_surface', 'ec_events_to_time_surface_packed'
    bad_decay, bad_tau = prm(), prm(decay='exp')
    bad_decay.decay, bad_tau.tau_us = 7, 0.
    for name, args, msg in (
            (f, (None, rng.data_ptr(), 1, prm(), frames.data_ptr()), b'null buffer'),
            (f, (ev.data_ptr(), None, 1, prm(), frames.data_ptr()), b'null buffer'),
            (p, (pk.data_ptr(), rng.data_ptr(), 1, prm(), None), b'null buffer'),
            (f, (ev.data_ptr(), rng.data_ptr(), 1, None, frames.data_ptr()), b'params is null'),
            (f, (ev.data_ptr() + 4, rng.data_ptr(), 1, prm(), frames.data_ptr()), b'16-byte aligned'),
            (p, (pk.data_ptr() + 4, rng.data_ptr(), 1, prm(), frames.data_ptr()), b'8-byte aligned'),
            (f, (ev.data_ptr(), rng.data_ptr(), 1, prm((8, 19969)), frames.data_ptr()), b'W=19969 too wide for one LDS row band'),
            (f, (ev.data_ptr(), rng.data_ptr(), 1, bad_decay, frames.data_ptr()), b'unknown decay 7'),
            (p, (pk.data_ptr(), rng.data_ptr(), 1, bad_tau, frames.data_ptr()), b'tau_us=0 must be positive'),
            (f, (ev.data_ptr(), rng.data_ptr(), -1, prm(), frames.data_ptr()), b'F=-1')):
        assert call(name, *args) == _lib.EC_ERR_INVALID, msg
        assert msg in lib.ec_last_error(), (msg, lib.ec_last_error())
    assert call(f, None, None, 0, prm(), None) == _lib.EC_OK
    assert call(p, pk.data_ptr(), rng.data_ptr(), 1, prm(decay='exp', tau=1e-9), frames.data_ptr()) == _lib.EC_OK
    torch.cuda.synchronize()
    assert (frames[0] == 255).all() and (frames[1] == GUARD).all()       # 64 events with p == 0: all background


def test_opcheck_on_the_op(hip):
    import torch
    c = ts.cases()['rows36x52']
    rng = torch.tensor(c['ranges'], dtype=torch.int64).cuda()
    for events in (torch.from_numpy(c['events']).cuda(), torch.from_numpy(ts.packed(c).view(np.int64)).cuda()):
        torch.library.opcheck(torch.ops.eventclip_hip.events_to_time_surface.default,
                              (events, rng, 36, 52, 'exp', 2.0, [255, 0, 0], [0, 0, 255], True, len(c['events']), True, False, True,
                               len(c['events'])))
