"""The fixed-duration windows (csrc/events.hip: time_windows_kernel) and the layers above them on the MI355X, against the
restatement of the definition in tests/time_windows_ref.py: every case of its table, both anchors, packed events and float
rows; bounds and stats exactly, with guards wherever the call may not write.  Everything is integer equality."""
import functools

import numpy as np
import pytest

import time_windows_ref as tw

pytestmark = pytest.mark.gpu

GUARD64, GUARD32 = -0x5A5A5A5A5A5A5A5B, 0x5A5A5A5A
SHAPE = (36, 52)


@functools.lru_cache(None)
def want(name, from_last):
    """The oracle's answer, computed once and shared."""
    c = tw.cases()[name]
    return tw.oracle(c['ticks'], c['ranges'], c['dt_us'], c['stride_us'], c['max_windows'], from_last)


def launch(events, ranges, dt_us, stride_us, max_windows, from_last, total_events=None):
    """Straight to the C ABI on numpy events (float32 [n, 4] or uint64 [n]).  bounds is prefilled with PREFILL and stats with
    GUARD32, each between one guard sample before and one behind, which must come back untouched.
    -> dict(bounds int64 [B, max_windows, 2], stats STATS_DTYPE [B], raw int32 [B, 4])."""
    import torch
    from eventclip_amd import _lib, vis
    packed = vis.is_packed(events)
    B = len(ranges)
    ev = torch.from_numpy(events.view(np.int64) if packed else events).cuda()
    if len(events) == 0:
        ev = torch.zeros((1,) if packed else (1, 4), dtype=ev.dtype, device='cuda')
    rng = torch.tensor(ranges, dtype=torch.int64).reshape(-1, 2).cuda()
    bounds = torch.full((B + 2, max_windows, 2), GUARD64, dtype=torch.int64, device='cuda')
    bounds[1:B + 1] = tw.PREFILL
    stats = torch.full((B + 2, 4), GUARD32, dtype=torch.int32, device='cuda')
    total = sum(max(e - b, 0) for b, e in ranges) if total_events is None else total_events
    prm = vis.time_windows_params(dt_us, stride_us, max_windows, from_last, total)
    _lib.launch('ec_time_windows_packed' if packed else 'ec_time_windows', ev, rng, B, prm, bounds[1:], stats[1:])
    torch.cuda.synchronize()
    for g in (0, B + 1):
        assert (bounds[g] == GUARD64).all(), 'bounds written outside the samples'
        assert (stats[g] == GUARD32).all(), 'stats written outside the samples'
    raw = stats[1:B + 1].cpu().numpy()
    return dict(bounds=bounds[1:B + 1].cpu().numpy(), stats=raw.view(tw.STATS_DTYPE).reshape(B), raw=raw)


def run(name, from_last, packed, **kw):
    c = tw.cases()[name]
    ev = tw.packed_events(c['ticks']) if packed else tw.float_events(c['ticks'])
    return launch(ev, c['ranges'], c['dt_us'], c['stride_us'], c['max_windows'], from_last, **kw)


def test_the_tables_are_cut_at_the_kernels_own_sizes(hip):
    from eventclip_amd import vis
    assert (vis.TIME_WINDOWS_SLICE_ROWS, vis.TIME_WINDOWS_UNROLL) == (tw.SLICE, tw.UNROLL)
    S = vis.TIME_WINDOWS_SLICE_ROWS
    for n in (1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1, S // vis.TIME_WINDOWS_UNROLL - 1, S // vis.TIME_WINDOWS_UNROLL + 1):
        assert f'n{n}' in tw.cases()


@pytest.mark.parametrize('from_last', [0, 1])
@pytest.mark.parametrize('name', sorted(tw.cases()))
def test_every_case_packed_and_float(name, from_last, hip):
    """Lengths around the wave, the unroll round and the slice; a tick step on a slice boundary and none; equal ticks; events
    on lower and upper edges; stride below, at and above the window; silent gaps; windows above max_windows with the prefill
    behind the written rows; unit windows and 2^30 - 1 windows at the top of the tick range; gapped, empty and reversed
    ranges; one unsorted sample among sorted ones; descents on every boundary; 32 random batches."""
    c = tw.cases()[name]
    got = run(name, from_last, True)
    tw.check(got, want(name, from_last), c['ranges'])
    for b, (e0, e1) in enumerate(c['ranges']):
        if e1 <= e0:                                                      # an empty sample: windows = 0 and nothing else
            assert got['raw'][b].tolist() == [GUARD32, GUARD32, GUARD32, 0]
    if c['floatable']:
        gf = run(name, from_last, False)
        tw.check(gf, want(name, from_last), c['ranges'])
        np.testing.assert_array_equal(gf['stats'], got['stats'])
        ok = want(name, from_last)['sorted']
        np.testing.assert_array_equal(gf['bounds'][ok], got['bounds'][ok])


def test_the_unsorted_sample_is_told_and_its_neighbours_are_exact(hip):
    c = tw.cases()['one_unsorted']
    t = c['ticks'][500:1300]
    descents = int((t[1:] < t[:-1]).sum())
    assert descents == 3                                                  # rows 5, 400 and 799; row 6 equals its predecessor
    for from_last in (0, 1):
        for packed in (True, False):
            got = run('one_unsorted', from_last, packed)
            assert got['stats']['unsorted'].tolist() == [0, descents, 0] and got['stats']['windows'][1] == -1
            assert (got['stats']['windows'][[0, 2]] > 0).all()
            w = want('one_unsorted', from_last)
            np.testing.assert_array_equal(got['bounds'][[0, 2]], w['bounds'][[0, 2]])
            # unspecified, but its own rows and row numbers of its own sample (or the prefill)
            own = got['bounds'][1]
            assert ((own == tw.PREFILL) | ((own >= 500) & (own <= 1300))).all()


@pytest.mark.parametrize('name', ['n1', f'n{2 * tw.SLICE + 1}', 'gapped', 'descents_at_boundaries', 'rand07'])
def test_the_grid_hint_changes_nothing(name, hip):
    """total_events sizes the grid only: one walker per sample (1), the default (0: unknown), far too many."""
    c = tw.cases()[name]
    for from_last in (0, 1):
        for total in (0, 1, 10 ** 9):
            tw.check(run(name, from_last, True, total_events=total), want(name, from_last), c['ranges'])


def test_float_ticks_saturate_at_both_ends_of_the_range(hip):
    ev = tw.float_saturation_events()
    ticks = tw.ticks_of(ev)
    assert ticks[0] == ticks[1] == 0 and ticks[-1] == ticks[-2] == ticks[-3] == tw.TICK_MAX and (np.diff(ticks) >= 0).all()
    for dt, stride, mw in ((2 ** 29, 2 ** 29, 4), (1, 1, 5), (tw.TICK_MAX, tw.TICK_MAX, 3), (1000, 2 ** 30 - 7, 3)):
        for from_last in (0, 1):
            got = launch(ev, [(0, len(ev))], dt, stride, mw, from_last)
            tw.check(got, tw.oracle(ticks, [(0, len(ev))], dt, stride, mw, from_last), [(0, len(ev))])
    assert launch(ev, [(0, len(ev))], 1, 1, 5, 0)['stats']['windows'][0] == 2 ** 30                 # the full count


# ---- the layers ----
def _stream(n, seed, span, lo=0):
    """n float rows inside SHAPE, sorted ticks over [lo, lo + span)."""
    r = np.random.default_rng(seed)
    ticks = lo + np.sort(r.integers(0, span, n))
    ticks[0] = lo
    return tw.float_events(ticks, seed)


@functools.lru_cache(None)
def samples():
    s0 = np.concatenate([_stream(200, 1, 2500), _stream(150, 2, 3000, lo=9000)])       # windows 1 and 2 of 3000 us are empty
    s1 = np.concatenate([_stream(900, 3, 30000), tw.float_events([30001, 30001], 4)])   # 11 windows, the last of 2 events
    s2 = _stream(40, 5, 2000)
    return s0, s1, s2


def test_device_entry_and_custom_op_give_the_same_bytes(hip):
    import torch
    from eventclip_amd import vis
    c = tw.cases()['gapped']
    for ev in (tw.float_events(c['ticks']), tw.packed_events(c['ticks'])):
        ev_d = torch.from_numpy(ev.view(np.int64) if ev.ndim == 1 else ev).cuda()
        sr = torch.tensor(c['ranges'], dtype=torch.int64)
        for from_last in (False, True):
            w = tw.oracle(c['ticks'], c['ranges'], 3000, 1700, 20, from_last)
            bounds, stats = vis.time_windows_device(ev_d, sr, 0.003, 0.0017, 20, from_last)
            assert bounds.is_cuda and bounds.dtype == torch.int64 and stats.dtype == vis.TIME_WINDOWS_STATS_DTYPE
            b2, s2 = torch.ops.eventclip_hip.events_time_windows(ev_d, sr.cuda(), 3000, 1700, 20, from_last, 0)
            assert torch.equal(bounds, b2) and stats.tobytes() == s2.cpu().numpy().tobytes()
            b3, s3 = vis.time_windows_device(ev_d, sr.cuda(), 0.003, 0.0017, 20, from_last)        # ranges on the device
            assert torch.equal(bounds, b3) and stats.tobytes() == s3.tobytes()
            tw.check(dict(bounds=bounds.cpu().numpy(), stats=stats), w, c['ranges'])
            np.testing.assert_array_equal(stats, w['stats'])                 # an empty sample's words are zero here
    bounds, stats = vis.time_windows_device(ev_d, sr, 0.003)                  # stride = window, 64 rows
    w = tw.oracle(c['ticks'], c['ranges'], 3000, 3000, 64, 0)
    np.testing.assert_array_equal(bounds.cpu().numpy(), w['bounds'])


def test_split_time_window_is_the_reference(hip):
    from eventclip_amd import vis
    ev = samples()[1]
    ticks = tw.ticks_of(ev)
    for window, stride, dt_us, st_us in ((0.003, None, 3000, 3000), (0.004, 0.001, 4000, 1000), (0.0001, 0.0001, 100, 100)):
        _, rows = tw.sample_by_search(ticks, 0, dt_us, st_us, 0)              # 11, 31 and 301 windows: more than one launch's 64
        for arg in (ev, ev[:, 2].astype(np.float64), vis.pack_events(ev), dict(x=ev[:, 0], y=ev[:, 1], t=ev[:, 2], p=ev[:, 3])):
            idx0, idx1, t0, t1 = vis.split_time_window(arg, window, stride)
            assert idx0 == rows[:, 0].tolist() and idx1 == rows[:, 1].tolist()
            np.testing.assert_array_equal(np.rint(t0 * 1e6), ticks[0] + np.arange(len(rows)) * st_us)
            np.testing.assert_array_equal(np.rint((t1 - t0) * 1e6), dt_us)
    with pytest.raises(ValueError, match='not sorted'):
        vis.split_time_window(ev[::-1].copy(), 0.003)
    with pytest.raises(IndexError):
        vis.split_time_window(ev[:0], 0.003)


def _device_frames(vis, ev_d, ranges, method, **kw):
    import torch
    rng = torch.tensor(np.asarray(ranges).reshape(-1, 2), dtype=torch.int64, device='cuda')
    if method == 'time_surface':
        return vis.time_surface_device(ev_d, rng, SHAPE, **kw)
    if method == 'voxel_grid':
        return vis.voxel_grid_device(ev_d, rng, SHAPE, **kw)
    return vis.events_to_frames_device(ev_d, rng, SHAPE, **kw)


@pytest.mark.parametrize('method', ['event_histogram', 'time_surface', 'voxel_grid'])
def test_events2frames_by_time_window_is_the_device_entry_on_the_reference_ranges(method, hip):
    import torch
    from eventclip_amd import vis
    ev = samples()[0]
    for denoise, window, stride, min_events in ((None, 0.003, None, 1), (None, 0.002, 0.0007, 30), (dict(dt=0.002, radius=2), 0.003, 0.001, 1)):
        kept = ev if denoise is None else vis.denoise_events(ev, SHAPE, denoise['dt'], denoise['radius'])
        dt_us = int(round(window * 1e6))
        st_us = dt_us if stride is None else int(round(stride * 1e6))
        _, rows = tw.sample_by_counting(tw.ticks_of(kept), 0, dt_us, st_us, 0)
        rows = rows[rows[:, 1] - rows[:, 0] >= min_events]
        assert 0 < len(rows) and (denoise is not None or min_events > 1 or len(rows) < 5)          # the empty windows are no frames
        got = vis.events2frames(ev, 'time_window', method, SHAPE, window=window, stride=stride, min_events=min_events,
                                denoise=denoise)
        ref = _device_frames(vis, torch.from_numpy(kept).cuda(), rows, method)
        assert got.shape == (len(rows), *SHAPE, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, ref.cpu().numpy())
    with pytest.raises(ValueError, match='min_events=5000'):
        vis.events2frames(ev, 'time_window', method, SHAPE, window=0.003, min_events=5000)
    with pytest.raises(ValueError, match='not sorted'):
        vis.events2frames(ev[::-1].copy(), 'time_window', method, SHAPE, window=0.003)
    with pytest.raises(AssertionError):
        vis.events2frames(ev, 'time', method, SHAPE, window=0.003, N=100)


QA = dict(split_method='time_window', window=0.003, max_imgs=4, grayscale=True, count_non_zero=False, background_mask=True)


def _expected(vis, method, smp, qa, hflip, tflip, gen):
    """The reference composition: the oracle's windows per sample, the valid ones in window order, the draw chunks get,
    the existing device entry on those ranges, the existing preprocess, padded views zero."""
    import torch
    from eventclip_amd.preprocess import preprocess_frames
    T, dt_us = qa['max_imgs'], int(round(qa['window'] * 1e6))
    st_us = int(round(qa.get('stride', qa['window']) * 1e6))
    ranges, off = [], 0
    ri, wi = np.full((len(smp), T), -1, np.int32), np.full((len(smp), T), -1, np.int32)
    for b, s in enumerate(smp):
        _, rows = tw.sample_by_search(tw.ticks_of(s), off, dt_us, st_us, int(tflip))
        valid = [k for k in range(len(rows)) if rows[k, 1] - rows[k, 0] >= qa.get('min_events', 1)]
        if len(valid) > T:
            valid = [valid[i] for i in torch.randperm(len(valid), generator=gen)[:T].tolist()]
        for t, k in enumerate(valid):
            ri[b, t], wi[b, t] = len(ranges), k
            ranges.append(rows[k])
        off += len(s)
    kw = dict(flip_x=hflip, negate_p=tflip)
    if method != 'event_histogram':
        kw['reverse_t'] = tflip
    frames = _device_frames(vis, torch.from_numpy(np.concatenate(smp)).cuda(), ranges, method, **kw)
    img = torch.zeros((len(smp), T, 3, 32, 32), dtype=torch.float32, device='cuda')
    img[torch.from_numpy(ri >= 0).cuda()] = preprocess_frames(frames, 32, mode='chw')
    return dict(img=img, row_idx=torch.from_numpy(ri).cuda(), window_index=torch.from_numpy(wi).cuda(),
                valid_mask=torch.from_numpy(ri >= 0).cuda())


@pytest.mark.parametrize('method', ['event_histogram', 'time_surface', 'voxel_grid'])
def test_the_pipeline_on_a_ragged_batch_is_the_reference_composition(method, hip):
    import torch
    from eventclip_amd import vis
    from eventclip_amd.event2img import Event2ImagePipeline
    smp = list(samples())
    for extra in (dict(), dict(stride=0.0015, min_events=3)):
        qa = dict(QA, convert_method=method, **extra)
        for hflip, tflip in ((False, False), (True, True)):
            pipe = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32, generator=torch.Generator().manual_seed(11))
            got = pipe(smp, hflip=hflip, tflip=tflip)
            ref = _expected(vis, method, smp, qa, hflip, tflip, torch.Generator().manual_seed(11))
            assert set(got) == {'valid_mask', 'row_idx', 'window_index', 'img'}
            for k in ref:
                assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (k, extra, tflip)
            if not extra:
                # sample 0: windows 1 and 2 are empty, sample 1: a draw of 4 from 11, sample 2: one window
                wi = got['window_index'].cpu().tolist()
                assert wi[0] == [0, 3, -1, -1] and wi[2] == [0, -1, -1, -1]                 # from either end
                assert len(set(wi[1])) == 4 and min(wi[1]) >= 0
    # tta(): the four views, two from each anchor, the draws in call order
    qa = dict(QA, convert_method=method, min_events=3)
    views = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32, generator=torch.Generator().manual_seed(5)).tta(smp)
    single = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32, generator=torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(5)
    for v, (h, t) in zip(views, ((False, False), (True, False), (False, True), (True, True))):
        s, ref = single(smp, hflip=h, tflip=t), _expected(vis, method, smp, qa, h, t, gen)
        for k in ref:
            assert torch.equal(v[k], s[k]) and torch.equal(v[k], ref[k]), (k, h, t)


def test_the_pipeline_with_denoise_and_packed_events_and_gapped_starts(hip):
    import torch
    from eventclip_amd import vis
    from eventclip_amd.event2img import Event2ImagePipeline
    smp = list(samples())
    qa = dict(QA, convert_method='time_surface', max_imgs=12, denoise=dict(dt=0.002, radius=3))
    surv = [vis.denoise_events(s, SHAPE, 0.002, 3) for s in smp]
    got = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32)(smp)
    ref = Event2ImagePipeline(SHAPE, 3000, {k: v for k, v in qa.items() if k != 'denoise'}, n_px=32)(surv)
    assert got['n_events'] == [len(s) for s in surv]
    for k in ('img', 'valid_mask', 'window_index'):                         # the windows are cut from the survivors, in place
        assert torch.equal(got[k], ref[k]), k
    qa = dict(QA, convert_method='event_histogram', max_imgs=12)
    a = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32)(smp)
    b = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32)([vis.pack_events(s) for s in smp])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_the_three_value_errors_name_the_samples(hip):
    from eventclip_amd.event2img import Event2ImagePipeline
    s0, s1, s2 = samples()
    qa = dict(QA, convert_method='event_histogram')
    pipe = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32)
    bad = s1.copy()
    bad[[10, 500]] = bad[[500, 10]]
    with pytest.raises(ValueError, match=r'samples \[1, 3\] are not sorted'):
        pipe([s0, bad, s2, s1[::-1].copy()])
    with pytest.raises(ValueError, match=r'samples \[1\] span \[11\] windows.*max_windows=10'):
        Event2ImagePipeline(SHAPE, 3000, dict(qa, max_windows=10), n_px=32)([s0, s1, s2])
    with pytest.raises(ValueError, match=r'no window of samples \[1, 2\] holds min_events=120'):
        Event2ImagePipeline(SHAPE, 3000, dict(qa, min_events=120), n_px=32)([s0, s1, s2])
    with pytest.raises(ValueError, match=r'samples \[0\] span'):
        Event2ImagePipeline(SHAPE, 3000, dict(qa, max_windows=3), n_px=32).tta([s0])
    with pytest.raises(IndexError):
        pipe([s0, np.zeros((0, 4), np.float32)])


def test_the_event_count_output_is_what_it_was(hip):
    """split_method='event_count' on the same samples: the chunk plan, the draw and the frames of the existing entries, and no
    new key in the result."""
    import torch
    from eventclip_amd import vis
    from eventclip_amd.event2img import Event2ImagePipeline
    from eventclip_amd.preprocess import preprocess_frames
    smp = list(samples())
    qa = dict(max_imgs=3, N=200, split_method='event_count', convert_method='event_histogram', grayscale=True,
              count_non_zero=False, background_mask=True)
    got = Event2ImagePipeline(SHAPE, 3000, qa, n_px=32, generator=torch.Generator().manual_seed(3))(smp)
    assert set(got) == {'valid_mask', 'row_idx', 'img'}
    gen, ranges, off = torch.Generator().manual_seed(3), [], 0
    ri = np.full((3, 3), -1, np.int32)
    for b, s in enumerate(smp):
        idx0, idx1 = vis.chunk_bounds(len(s), 200)
        sel = list(range(len(idx0)))
        if len(sel) > 3:
            sel = torch.randperm(len(sel), generator=gen)[:3].tolist()
        for t, f in enumerate(sel):
            ri[b, t] = len(ranges)
            ranges.append((off + idx0[f], off + idx1[f]))
        off += len(s)
    frames = _device_frames(vis, torch.from_numpy(np.concatenate(smp)).cuda(), ranges, 'event_histogram', max_frame_events=200)
    img = torch.zeros((3, 3, 3, 32, 32), dtype=torch.float32, device='cuda')
    img[torch.from_numpy(ri >= 0).cuda()] = preprocess_frames(frames, 32, mode='chw')
    assert torch.equal(got['img'], img) and torch.equal(got['row_idx'].cpu(), torch.from_numpy(ri))
