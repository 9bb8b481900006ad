"""The refractory-period filter (csrc/events.hip: refractory_kernel) and the layers above it on the MI355X, against the
restatement of the definition in tests/refractory_ref.py: every case of its table, float rows and packed events, pixel-wide
and per polarity; the survivors, counts, keep bytes and stats exactly, with guard bytes wherever the call may not write."""
import ctypes
import functools

import numpy as np
import pytest

import denoise_ref as dn
import refractory_ref as rf

pytestmark = pytest.mark.gpu

GUARD = rf.GUARD
TAIL = 64              # guard rows behind the last event, and one guard sample behind the last
MODES = (False, True)


@functools.lru_cache(None)
def want(name, per_polarity, packed=False):
    """The oracle's answer, computed once and shared."""
    c = rf.cases()[name]
    return rf.oracle(rf.packed(c) if packed else c['events'], c['ranges'], c['shape'], c['period_us'], per_polarity)


def launch(events, ranges, shape, period_us, per_polarity, outputs=('keep', 'stats'), cap=None):
    """Straight to the C ABI on numpy events (float32 [n, 4] or uint64 [n]); every output prefilled with GUARD, TAIL rows
    and one sample longer than the launch may write.  -> dict(events_out, counts, keep, stats) as numpy (None where not
    asked for), shaped like the oracle's."""
    import torch
    from eventclip_amd import _lib, vis
    packed = vis.is_packed(events)
    n, B = len(events), len(ranges)
    ev = torch.from_numpy(events.view(np.int64) if packed else events).cuda()
    rng = torch.tensor(ranges, dtype=torch.int64).reshape(-1, 2).cuda()
    fill = int(np.frombuffer(bytes([GUARD]) * 8, np.int64)[0])
    out = torch.full((n + TAIL,), fill, dtype=torch.int64, device='cuda') if packed else \
        torch.full(((n + TAIL) * 16,), GUARD, dtype=torch.uint8, device='cuda').view(torch.float32).view(-1, 4)
    counts = torch.full((B + 1,), fill, dtype=torch.int64, device='cuda')
    keep = torch.full((n + TAIL,), GUARD, dtype=torch.uint8, device='cuda') if 'keep' in outputs else None
    stats = torch.full((B + 1, ctypes.sizeof(vis.EcRefractoryStats)), GUARD, dtype=torch.uint8, device='cuda') if 'stats' in outputs else None
    longest = max([e - b for b, e in ranges] + [1])
    prm = vis.refractory_params(shape, period_us, per_polarity, cap or longest, sum(e - b for b, e in ranges))
    ws = torch.empty((max(256, vis.refractory_workspace_bytes(prm, B)),), dtype=torch.uint8, device='cuda')
    _lib.launch('ec_refractory_events_packed' if packed else 'ec_refractory_events', ev, rng, B, prm, out, counts, keep, stats,
                ws, ws.numel())
    torch.cuda.synchronize()
    assert (out.reshape(-1).view(torch.uint8)[n * (8 if packed else 16):] == GUARD).all(), 'events_out written past the last event'
    assert counts[B] == fill, 'counts written past the last sample'
    assert keep is None or (keep[n:] == GUARD).all(), 'keep written past the last event'
    assert stats is None or (stats[B] == GUARD).all(), 'stats written past the last sample'
    return dict(events_out=out[:n].cpu().numpy().view(np.uint64 if packed else np.float32), counts=counts[:B].cpu().numpy(),
                keep=None if keep is None else keep[:n].cpu().numpy(),
                stats=None if stats is None else stats[:B].cpu().numpy().view(rf.STATS_DTYPE).reshape(B))


def run(name, per_polarity, packed=False, outputs=('keep', 'stats')):
    c = rf.cases()[name]
    return launch(rf.packed(c) if packed else c['events'], c['ranges'], c['shape'], c['period_us'], per_polarity, outputs)


def test_band_counts(hip):
    """one band (the two small sensors), two / three (180 x 240), ten / twenty (480 x 640), and a partial last band"""
    from eventclip_amd import vis
    assert [vis.refractory_bands(s, pp) for s in rf.SHAPES for pp in MODES] == [1, 1, 2, 3, 10, 20, 1, 1]
    assert vis.refractory_bands((100, 700), False) == 3 and rf.plan((100, 700), False) == (34, 3)       # a partial last band


@pytest.mark.parametrize('name', sorted(rf.cases()))
def test_every_case_float_and_packed_pixel_wide_and_per_polarity(name, hip):
    """Random streams at the four shapes; the directed properties (lone, gaps of period and period - 1, a removed event
    extending nothing, equal ticks, unsorted rows, ON / OFF alternation, uncounted rows, the wrapped index, corners), a
    period of one tick, the tick range's ends, a class per row boundary of every shape, class lists of every length around
    the wave and the lane / wave threshold up to 4096 at periods that keep all, half and one, a hot pixel, sample lengths
    around the wave, the workgroup and the unroll, 600 samples, gapped ranges, skipped rows, truncating coordinates."""
    c = rf.cases()[name]
    for pp in MODES:
        for packed in ((False, True) if c['packable'] else (False,)):
            got = run(name, pp, packed)
            rf.check(got, want(name, pp, packed))
            if c['expect'] is not None:
                np.testing.assert_array_equal(got['keep'], rf.expected_keep(c, pp))


def test_the_list_cases_sit_on_the_thresholds_edges(hip):
    from eventclip_amd import vis
    L = vis.REFRACTORY_LONG_LIST
    assert {1, 2, 63, 64, 65, L - 1, L, L + 1, 127, 128, 129, 4096} <= set(rf.list_lengths())
    for name, lo, hi in (('lists_all', 1.0, 1.0), ('lists_half', 0.49, 0.52), ('lists_one', 0.0, 0.003)):
        share = rf.kept_share(want(name, False))
        assert lo <= share <= hi, (name, share)
    assert want('lists_one', False)['stats']['kept'][0] == len(rf.list_lengths())


@pytest.mark.parametrize('name', ['rand_small', 'rand_180', 'rand_480', 'lengths', 'many', 'gapped', 'skip'])
def test_each_optional_output_alone(name, hip):
    for pp in MODES:
        for outputs in ((), ('keep',), ('stats',)):
            rf.check(run(name, pp, False, outputs), want(name, pp))
            rf.check(run(name, pp, True, outputs), want(name, pp, True))


@pytest.mark.parametrize('name', ['rand_small', 'rand_180_three', 'rand_480', 'hot', 'skip', 'lists_half', 'lengths'])
def test_input_the_caller_shuffles_is_filtered_as_the_definition_says(name, hip):
    """row order enters through the tie rule only: the shuffled stream against the oracle on the shuffled stream, and the
    same counts wherever no ticks tie inside a class"""
    c = rf.cases()[name]
    perm = np.arange(len(c['events']))
    rng = np.random.default_rng(7)
    for b, e in c['ranges']:
        perm[b:e] = b + rng.permutation(e - b)
    for pp in MODES:
        for packed in (False, True):
            ev = (rf.packed(c) if packed else c['events'])[perm]
            got = launch(ev, c['ranges'], c['shape'], c['period_us'], pp)
            w = rf.oracle(ev, c['ranges'], c['shape'], c['period_us'], pp)
            rf.check(got, w)
            np.testing.assert_array_equal(w['stats'], want(name, pp, packed)['stats'])   # ties move the kept row, not the count


def test_a_sample_longer_than_the_bound_is_not_filtered_and_nothing_else_is_touched(hip):
    """max_sample_events sizes the workspace: a longer sample gets counts -1 and zero stats, stays unwritten, and the
    samples beside it are filtered as ever."""
    c = rf.cases()['gapped']                                             # lengths 900, 1400, 1, 699
    for pp in MODES:
        got = launch(c['events'], c['ranges'], c['shape'], c['period_us'], pp, cap=900)
        w = {k: v.copy() for k, v in want('gapped', pp).items()}
        b, e = c['ranges'][1]
        w['counts'][1], w['stats'][1] = -1, (0, 0, 0)
        w['keep'][b:e] = GUARD
        w['events_out'][b:e].reshape(-1).view(np.uint8)[:] = GUARD
        rf.check(got, w)


def test_b_zero_and_the_refusals_write_nothing(hip):
    import torch
    from eventclip_amd import _lib, vis
    lib = _lib.lib()
    ev = torch.zeros((64, 4), dtype=torch.float32, device='cuda')
    rng = torch.tensor([[0, 64]], dtype=torch.int64, device='cuda')
    out = torch.full((64 * 16,), GUARD, dtype=torch.uint8, device='cuda')
    counts = torch.full((8,), GUARD, dtype=torch.uint8, device='cuda')
    keep = torch.full((64,), GUARD, dtype=torch.uint8, device='cuda')
    stats = torch.full((12,), GUARD, dtype=torch.uint8, device='cuda')
    ws = torch.full((4096,), GUARD, dtype=torch.uint8, device='cuda')

    def call(B, p, o=out, ws_bytes=4096, e=ev):
        return lib.ec_refractory_events(e.data_ptr(), rng.data_ptr(), B, ctypes.byref(p), o.data_ptr(), counts.data_ptr(),
                                        keep.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())

    prm = vis.refractory_params((8, 8), 100, False, 64)
    assert call(0, prm) == _lib.EC_OK
    bad_p, bad_pp, bad_cap, bad_w = (vis.refractory_params((8, 8), 100, False, 64) for _ in range(4))
    bad_p.period_us, bad_pp.per_polarity, bad_cap.max_sample_events, bad_w.W = 0, 2, 0, 40000
    assert call(1, bad_p) == _lib.EC_ERR_INVALID and b'period_us=0' in lib.ec_last_error()
    assert call(1, bad_pp) == _lib.EC_ERR_INVALID and b'per_polarity=2' in lib.ec_last_error()
    assert call(1, bad_cap) == _lib.EC_ERR_INVALID and b'max_sample_events=0' in lib.ec_last_error()
    assert call(1, bad_w) == _lib.EC_ERR_INVALID and b'too wide' in lib.ec_last_error()
    assert call(1, prm, o=ev) == _lib.EC_ERR_INVALID and b'in-place' in lib.ec_last_error()
    assert call(1, prm, e=ev.view(-1)[1:]) == _lib.EC_ERR_INVALID and b'16-byte aligned' in lib.ec_last_error()
    assert call(1, prm, ws_bytes=575) == _lib.EC_ERR_WORKSPACE and b'workspace 575 < 576 bytes' in lib.ec_last_error()
    torch.cuda.synchronize()
    for t in (out, counts, keep, stats, ws):
        assert (t == GUARD).all()
    assert call(1, prm) == _lib.EC_OK
    torch.cuda.synchronize()
    assert counts.view(torch.int64)[0] == 64 and (keep == 1).all() and (out == 0).all()        # p == 0: every row passes
    assert stats.view(torch.int32).tolist() == [0, 0, 64]


def test_the_op_against_the_c_abi_under_fake_tensors_and_opcheck(hip):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops, vis  # noqa: F401
    with FakeTensorMode():
        sr = torch.zeros(5, 2, dtype=torch.int64, device='cuda')
        for ev in (torch.empty(1000, 4, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')):
            out, counts = torch.ops.eventclip_hip.events_refractory(ev, sr, 181, 240, 5000, True)
            assert out.shape == ev.shape and out.dtype == ev.dtype and counts.shape == (5,) and counts.dtype == torch.int64
    for name in ('gapped', 'rand_180_three', 'lengths'):
        c = rf.cases()[name]
        rng = torch.tensor(c['ranges'], dtype=torch.int64).cuda()
        for pp in MODES:
            for packed in (False, True):
                events = torch.from_numpy(rf.packed(c).view(np.int64) if packed else c['events']).cuda()
                w = want(name, pp, packed)
                out, counts = torch.ops.eventclip_hip.events_refractory(events, rng, *c['shape'], c['period_us'], pp)
                np.testing.assert_array_equal(counts.cpu().numpy(), w['counts'])
                o = out.cpu().numpy().view(w['events_out'].dtype)
                written = np.zeros(len(o), bool)
                for (b, e), n in zip(c['ranges'], w['counts']):
                    np.testing.assert_array_equal(o[b:b + n].view(np.uint8), w['events_out'][b:b + n].view(np.uint8))
                    written[b:b + n] = True
                assert not o[~written].view(np.uint8).any()                  # the op's other rows are zero
                # the same through the device entry, which goes to the C ABI itself when asked for the mask or the stats
                out2, counts2, keep, stats = vis.refractory_events_device(events, rng.cpu(), c['shape'], c['period_us'] / 1e6, pp,
                                                                          return_mask=True, return_stats=True)
                out3, counts3 = vis.refractory_events_device(events, rng, c['shape'], c['period_us'] / 1e6, pp)
                assert torch.equal(counts2, counts) and torch.equal(counts3, counts) and torch.equal(out3, out)
                inside = w['keep'] != GUARD
                np.testing.assert_array_equal(keep.cpu().numpy()[inside], w['keep'][inside])
                assert not keep.cpu().numpy()[~inside].any()
                np.testing.assert_array_equal(stats, w['stats'])
                for (b, e), n in zip(c['ranges'], w['counts']):
                    assert torch.equal(out2[b:b + n], out[b:b + n])
    c = rf.cases()['rand_small']
    rng = torch.tensor(c['ranges'], dtype=torch.int64).cuda()
    for events in (torch.from_numpy(c['events']).cuda(), torch.from_numpy(rf.packed(c).view(np.int64)).cuda()):
        torch.library.opcheck(torch.ops.eventclip_hip.events_refractory.default, (events, rng, 37, 53, c['period_us'], True))


def _survivors(c, per_polarity=False, packed=False):
    ev = rf.packed(c) if packed else c['events']
    w = rf.oracle(ev, c['ranges'], c['shape'], c['period_us'], per_polarity)
    return [ev[b:e][w['keep'][b:e] == 1] for b, e in c['ranges']]


def test_numpy_drop_ins_against_the_oracle_and_the_frame_oracles(hip):
    """vis.refractory_events, and events2frames(refractory=...) = the oracle's survivors through the existing device entries
    and frame oracles, for the three forms and both split methods; refractory then denoise = the two oracles composed."""
    import time_surface_ref as ts
    import voxel_grid_ref as vg
    from eventclip_amd import vis
    from oracle import events as oe
    for name in ('rand_small', 'rand_100', 'frac', 'skip'):
        c = rf.cases()[name]
        for pp in MODES:
            surv = _survivors(c, pp)[0]
            got = vis.refractory_events(c['events'], c['shape'], c['period_us'] / 1e6, pp)
            assert got.dtype == np.float32 and got.tobytes() == surv.tobytes()
            if c['packable']:
                got = vis.refractory_events(rf.packed(c), c['shape'], c['period_us'] / 1e6, pp)
                assert got.dtype == np.uint64 and got.tobytes() == _survivors(c, pp, True)[0].tobytes()
    d = dict(zip('xytp', rf.cases()['rand_small']['events'].T))
    assert vis.refractory_events(d, (37, 53), 0.02).tobytes() == _survivors(rf.cases()['rand_small'])[0].tobytes()
    assert vis.refractory_events(np.zeros((0, 4), np.float32), (37, 53), 1e-3).shape == (0, 4)
    for name, N, pp in (('rand_small', 400, False), ('rand_100', 1000, True)):
        c = rf.cases()[name]
        surv = _survivors(c, pp)[0]
        rz = dict(period=c['period_us'] / 1e6, per_polarity=pp)
        i0, i1 = vis.chunk_bounds(len(surv), N)
        assert len(i0) >= 3 and len(vis.chunk_bounds(len(c['events']), N)[0]) > len(i0)        # the filter moves every boundary
        ranges = list(zip(i0, i1))
        kw = dict(shape=c['shape'], N=N)
        np.testing.assert_array_equal(vis.events2frames(c['events'], 'event_count', 'event_histogram', refractory=rz, **kw),
                                      oe.events2frames(surv, 'event_count', 'event_histogram', **kw))
        np.testing.assert_array_equal(vis.events2frames(c['events'], 'event_count', 'time_surface', refractory=rz, **kw),
                                      ts.oracle(surv, ranges, c['shape'])['frames'])
        np.testing.assert_array_equal(vis.events2frames(c['events'], 'event_count', 'voxel_grid', refractory=rz, **kw),
                                      vg.oracle(surv, ranges, c['shape'], 3)['frames'])
        for method in vis.CONVERT_METHODS:                                   # fixed-duration windows of the survivors
            tw = dict(shape=c['shape'], window=0.01, stride=0.005)
            np.testing.assert_array_equal(vis.events2frames(c['events'], 'time_window', method, refractory=rz, **tw),
                                          vis.events2frames(surv, 'time_window', method, **tw))
        np.testing.assert_array_equal(vis.events2frames(c['events'], 'event_count', 'event_histogram', refractory=None, **kw),
                                      vis.events2frames(c['events'], 'event_count', 'event_histogram', **kw))
        # refractory first, then denoise: the composition of the two oracles
        dz = dict(dt=0.002, radius=1)
        w2 = dn.oracle(surv, [(0, len(surv))], c['shape'], 2000, 1)
        both = surv[w2['keep'] == 1]
        assert 0 < len(both) < len(surv)
        other = dn.oracle(c['events'], [(0, len(c['events']))], c['shape'], 2000, 1)
        assert int(other['counts'][0]) != len(both)                          # (the two filters do not commute here)
        np.testing.assert_array_equal(vis.events2frames(c['events'], 'event_count', 'event_histogram', refractory=rz, denoise=dz, **kw),
                                      oe.events2frames(both, 'event_count', 'event_histogram', **kw))


QA = dict(max_imgs=10, N=300, split_method='event_count', grayscale=False, count_non_zero=False, background_mask=True)
RZ = dict(period=0.02, per_polarity=True)
DZ = dict(dt=0.002, radius=1)


def _samples(shape=(36, 52)):
    from eventclip_amd import synthetic
    return [synthetic.make_events(n, shape, seed=20 + i, max_t=0.05, hot_pixels=2) for i, n in enumerate((3000, 1200, 2000))]


def _filtered(s, shape, rz=RZ):
    return s[rf.oracle(s, [(0, len(s))], shape, round(rz['period'] * 1e6), rz['per_polarity'])['keep'] == 1]


@pytest.mark.parametrize('method', ['event_histogram', 'time_surface', 'voxel_grid'])
def test_pipeline_with_the_filter_is_the_unfiltered_pipeline_on_the_oracles_survivors(method, hip):
    import torch
    from eventclip_amd import vis
    from eventclip_amd.event2img import Event2ImagePipeline
    shape = (36, 52)
    samples = _samples()
    plain = Event2ImagePipeline(shape, 3000, dict(QA, convert_method=method), n_px=32)
    pipe = Event2ImagePipeline(shape, 3000, dict(QA, convert_method=method, refractory=RZ), n_px=32)
    surv = [_filtered(s, shape) for s in samples]
    for s, f in zip(samples, surv):
        assert 0.1 < len(f) / len(s) < 0.97 and len(vis.chunk_bounds(len(f), 300)[0]) <= 10     # (no random subset of views)
    got, ref = pipe(samples), plain(surv)
    assert got['n_events'] == [len(s) for s in surv] and 'n_events' not in ref
    for k in ('img', 'valid_mask', 'row_idx'):
        assert torch.equal(got[k], ref[k]), k
    # the four views come from ONE filtering: the views of the survivors, not the survivors of the views
    views, ref_views = pipe.tta(samples), plain.tta(surv)
    for v, r in zip(views, ref_views):
        assert torch.equal(v['img'], r['img']) and v['n_events'] == got['n_events']
    assert torch.equal(pipe(samples, hflip=True, tflip=True)['img'], ref_views[3]['img'])
    # packed events, centring first, and a caller's own starts
    packed = [vis.pack_events(s) for s in samples]
    assert torch.equal(pipe(packed)['img'], got['img'])
    from oracle import event_utils as eu
    c_got = pipe(samples, center=True)
    centred = [eu.center_events(s.copy(), shape) for s in samples]              # (the oracle centres in place)
    c_surv = [_filtered(s, shape) for s in centred]
    assert torch.equal(c_got['img'], plain(c_surv)['img']) and c_got['n_events'] == [len(s) for s in c_surv]
    gap = np.zeros((17, 4), np.float32)
    cat = torch.from_numpy(np.concatenate([gap, samples[0], gap, gap, samples[1], samples[2], gap])).cuda()
    starts = [17, 17 + len(samples[0]) + 34, 17 + len(samples[0]) + 34 + len(samples[1])]
    g2 = pipe(cat, [len(s) for s in samples], starts=starts)
    assert torch.equal(g2['img'], got['img']) and g2['n_events'] == got['n_events']
    # refractory, then denoise: the composition of the two oracles
    both = Event2ImagePipeline(shape, 3000, dict(QA, convert_method=method, refractory=RZ, denoise=DZ), n_px=32)
    b_surv = [s[dn.oracle(s, [(0, len(s))], shape, 2000, 1)['keep'] == 1] for s in surv]
    b_got = both(samples)
    assert b_got['n_events'] == [len(s) for s in b_surv] and torch.equal(b_got['img'], plain(b_surv)['img'])
    assert [torch.equal(v['img'], r['img']) for v, r in zip(both.tta(samples), plain.tta(b_surv))] == [True] * 4


def test_pipeline_time_windows_refusals_and_the_untouched_paths(hip):
    import torch
    from eventclip_amd.event2img import Event2ImagePipeline
    shape = (36, 52)
    samples = _samples()
    qa = dict(QA, convert_method='event_histogram', max_imgs=10)         # every chunk a view: no random subset
    # a quantize_args without the key, or with None: bytes identical to today's, and no new key in the result
    a, b = Event2ImagePipeline(shape, 3000, qa, n_px=32)(samples), Event2ImagePipeline(shape, 3000, dict(qa, refractory=None), n_px=32)(samples)
    assert set(a) == set(b) == {'valid_mask', 'row_idx', 'img'} and all(torch.equal(a[k], b[k]) for k in a)
    d = Event2ImagePipeline(shape, 3000, dict(qa, denoise=DZ, refractory=None), n_px=32)(samples)
    e = Event2ImagePipeline(shape, 3000, dict(qa, denoise=DZ), n_px=32)(samples)
    assert set(d) == set(e) and all(torch.equal(d[k], e[k]) if torch.is_tensor(d[k]) else d[k] == e[k] for k in d)
    # fixed-duration windows are cut from the survivors
    tw = dict(QA, convert_method='time_surface', split_method='time_window', window=0.01, max_imgs=8)
    surv = [_filtered(s, shape) for s in samples]
    got = Event2ImagePipeline(shape, 3000, dict(tw, refractory=RZ), n_px=32)(samples)
    ref = Event2ImagePipeline(shape, 3000, tw, n_px=32)(surv)
    assert all(torch.equal(got[k], ref[k]) for k in ('img', 'valid_mask', 'row_idx', 'window_index'))
    pipe = Event2ImagePipeline(shape, 3000, dict(qa, refractory=RZ), n_px=32)
    # the filter cannot empty a sample that has a counted event: one pixel firing inside one dead time keeps its first
    hot = rf.rows([5] * 50, [5] * 50, np.arange(50) * 10, p=np.ones(50))
    assert pipe([samples[0], hot])['n_events'][1] == 1
    # a sample longer than max_n: the error the background-activity filter raises
    short = Event2ImagePipeline(shape, 1500, dict(qa, refractory=RZ), n_px=32)
    with pytest.raises(ValueError, match=r'samples \[0, 2\] hold more than max_n=1500'):
        short(samples)
    assert Event2ImagePipeline(shape, 1500, qa, n_px=32)(samples)['img'].shape[0] == 3          # ... only with the filter
    with pytest.raises(IndexError):                                      # an empty sample stays what it was
        pipe([samples[0], np.zeros((0, 4), np.float32)])
