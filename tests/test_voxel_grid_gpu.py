"""The voxel-grid kernel (csrc/events.hip: voxel_grid_kernel) and the layers above it on the MI355X, against the int64
restatement of the definition in tests/voxel_grid_ref.py: every case of its table, float rows and packed events; grid,
stats and bytes exactly."""
import ctypes
import functools

import numpy as np
import pytest

import voxel_grid_ref as vg

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GRID_GUARD = -0x5A5A5A5A
NO_FLAGS = dict(flip_x=False, negate_p=False, reverse_t=False)
ALL_FLAGS = [dict(flip_x=fx, negate_p=ng, reverse_t=rv) for fx in (False, True) for ng in (False, True) for rv in (False, True)]


@functools.lru_cache(None)
def want(name, background_mask, flags):
    """The oracle's answer on the float rows, computed once and shared (the packed form has the same:
    test_voxel_grid_ref_cpu.test_float_rows_and_packed_events_agree)."""
    c = vg.cases()[name]
    return vg.oracle(c['events'], c['ranges'], c['shape'], c['bins'], background_mask, **dict(flags))


def run(name, packed=False, background_mask=True, outputs=('frames', 'grid', 'stats'), **flags):
    """Straight to the C ABI, each asked-for buffer prefilled with a guard pattern and one frame longer than the launch
    writes; -> dict(frames, grid, stats) as numpy (None where not asked for, and frames where bins != 3)."""
    import torch
    from eventclip_amd import _lib, vis
    c = vg.cases()[name]
    (H, W), B, F = c['shape'], c['bins'], len(c['ranges'])
    ev = torch.from_numpy(vg.packed(c).view(np.int64) if packed else c['events']).cuda()
    rng = torch.tensor(c['ranges'], dtype=torch.int64).reshape(-1, 2).cuda()
    frames = torch.full((F + 1, H, W, 3), GUARD, dtype=torch.uint8, device='cuda') if 'frames' in outputs and B == 3 else None
    grid = torch.full((F + 1, H, W, B), GRID_GUARD, dtype=torch.int32, device='cuda') if 'grid' in outputs else None
    stats = torch.full((F + 1, ctypes.sizeof(vis.EcVoxelStats)), GUARD, dtype=torch.uint8, device='cuda') if 'stats' in outputs else None
    prm = vis.voxel_grid_params(c['shape'], B, background_mask, max(e - b for b, e in c['ranges']), flags.get('flip_x', False),
                                flags.get('negate_p', False), flags.get('reverse_t', False), sum(e - b for b, e in c['ranges']))
    _lib.launch('ec_events_to_voxel_grid_packed' if packed else 'ec_events_to_voxel_grid', ev, rng, F, prm, frames, grid, stats)
    torch.cuda.synchronize()
    assert frames is None or (frames[F] == GUARD).all(), 'frames written past the last frame'
    assert grid is None or (grid[F] == GRID_GUARD).all(), 'grid written past the last frame'
    assert stats is None or (stats[F] == GUARD).all(), 'stats written past the last frame'
    return dict(frames=None if frames is None else frames[:F].cpu().numpy(), grid=None if grid is None else grid[:F].cpu().numpy(),
                stats=None if stats is None else stats[:F].cpu().numpy().view(vis.VOXEL_STATS_DTYPE).reshape(F))


def run_and_check(name, packed=False, background_mask=True, outputs=('frames', 'grid', 'stats'), **flags):
    got = run(name, packed, background_mask, outputs, **flags)
    vg.check(got, want(name, background_mask, tuple(sorted(dict(NO_FLAGS, **flags).items()))))
    return got


def test_band_counts(hip):
    """1 band, a few and many with a partial last band, as the cases below name them."""
    from eventclip_amd import vis
    for (shape, B), bands in vg.BANDS.items():
        assert vis.voxel_grid_bands(shape, B) == bands, (shape, B)
    used = {(c['shape'], c['bins']) for c in vg.cases().values()}
    assert used == set(vg.BANDS)
    assert 181 % -(-181 // 4) != 0 and 100 % -(-100 // 15) != 0           # bands4 and bands15x8 end on a partial band


@pytest.mark.parametrize('name', sorted(vg.cases()))
def test_every_case_float_and_packed(name, hip):
    """Band counts 1 / 4 / 24 / 15 (cars, bands4, bands24, bands15x8), bins 2 / 3 / 8 (small*), span == 0 (single,
    same_tick), m == 0 (nothing: grey, white under the mask), events at t0 and t1 (ends), the 64-bit product (wide,
    wide3), the floor's edge (floor_edge), the cancelling pixel (cancel), negative_only, overlapping and gapped
    ranges (ranges), skip, frac, more frames than compute units (many), frame lengths around the
    scan's unroll (lengths).  Forward and with all three flags, mask on
    and off, every output."""
    c = vg.cases()[name]
    for packed in ((False, True) if c['packable'] else (False,)):
        for mask, flags in ((True, NO_FLAGS), (False, ALL_FLAGS[-1])):
            got = run_and_check(name, packed, mask, **flags)
            if name == 'nothing':
                assert (got['frames'] == (255 if mask else 128)).all() and (got['grid'] == 0).all()
                assert got['stats']['peak'].tolist() == [0, 0]


@pytest.mark.parametrize('name', ['cars', 'bands4', 'bands24', 'small3', 'many'])
def test_each_output_alone(name, hip):
    """frames without grid (a banded sensor then bins every band twice: the kernel's other pass 2), grid without
    frames, and neither with stats: the same values as with everything asked for."""
    for outputs in (('frames',), ('grid',), ('frames', 'stats'), ('grid', 'stats')):
        run_and_check(name, False, True, outputs, reverse_t=True)
        run_and_check(name, True, False, outputs)


@pytest.mark.parametrize('name', ['small3', 'small8', 'ends', 'floor_edge', 'cars', 'bands4'])
def test_every_flag_combination_against_the_rewritten_stream(name, hip):
    c = vg.cases()[name]
    for flags in ALL_FLAGS:
        w = vg.oracle(vg.rewrite(c['events'], c['shape'], **flags), c['ranges'], c['shape'], c['bins'])
        vg.check_rewritten(run(name, False, True, **flags), w)
        vg.check_rewritten(run(name, True, True, **flags), w)


def test_f_zero_and_the_device_side_refusals(hip):
    """F == 0 is EC_OK and touches nothing; a refused call touches nothing either."""
    import torch
    from eventclip_amd import _lib, vis
    lib = _lib.lib()
    ev = torch.zeros((64, 4), dtype=torch.float32, device='cuda')
    rng = torch.tensor([[0, 64]], dtype=torch.int64, device='cuda')
    frames = torch.full((2, 8, 8, 3), GUARD, dtype=torch.uint8, device='cuda')
    grid = torch.full((2, 8, 8, 3), GRID_GUARD, dtype=torch.int32, device='cuda')
    prm = vis.voxel_grid_params((8, 8), 3, True, 0, False, False, False, 0)

    def call(F, p, fr, g):
        return lib.ec_events_to_voxel_grid(ev.data_ptr(), rng.data_ptr(), F, ctypes.byref(p), fr, g, None, _lib.stream_ptr())

    assert call(0, prm, frames.data_ptr(), grid.data_ptr()) == _lib.EC_OK
    p2 = vis.voxel_grid_params((8, 8), 2, True, 0, False, False, False, 0)
    assert call(1, p2, frames.data_ptr(), grid.data_ptr()) == _lib.EC_ERR_INVALID and b'frames need bins == 3' in lib.ec_last_error()
    assert call(1, prm, None, None) == _lib.EC_ERR_INVALID and b'neither frames nor grid' in lib.ec_last_error()
    torch.cuda.synchronize()
    assert (frames == GUARD).all() and (grid == GRID_GUARD).all()
    assert call(1, prm, frames.data_ptr(), grid.data_ptr()) == _lib.EC_OK
    torch.cuda.synchronize()
    assert (frames[0] == 255).all() and (grid[0] == 0).all()             # 64 events with p == 0: all background
    assert (frames[1] == GUARD).all() and (grid[1] == GRID_GUARD).all()


def test_numpy_drop_in_and_production_op(hip):
    """vis.events2frames(..., 'voxel_grid') chunks by N like the other forms and raises on events outside the sensor; the
    production form (the custom op, frames only) gives the debug form's bytes, one band and banded; 'voxel' and
    split_method='time' stay refused."""
    import torch
    from eventclip_amd import vis
    c = vg.cases()['cars']
    ev = c['events']
    idx0, idx1 = vis.chunk_bounds(len(ev), 1500)
    assert len(idx0) == 3 and idx0[-1] == len(ev) - 1500                  # the overlapping last chunk
    for kw in (dict(), dict(bins=3, grayscale=False, background_mask=False, thresh=2., count_non_zero=True)):
        got = vis.events2frames(ev, 'event_count', 'voxel_grid', shape=c['shape'], N=1500, **dict(kw))
        vg.check(dict(frames=got), vg.oracle(ev, list(zip(idx0, idx1)), c['shape'], 3, kw.get('background_mask', True)))
    d = dict(x=ev[:, 0], y=ev[:, 1], t=ev[:, 2], p=ev[:, 3])
    np.testing.assert_array_equal(vis.events2frames(d, 'event_count', 'voxel_grid', shape=c['shape'], N=1500),
                                  vis.events2frames(ev, 'event_count', 'voxel_grid', shape=c['shape'], N=1500))
    with pytest.raises(ValueError, match='outside the sensor'):
        vis.events2frames(vg.cases()['skip']['events'], 'event_count', 'voxel_grid', shape=(36, 52), N=100)
    with pytest.raises(ValueError, match='bins=4'):
        vis.events2frames(ev, 'event_count', 'voxel_grid', shape=c['shape'], N=1500, bins=4)
    with pytest.raises(NotImplementedError):
        vis.events2frames(ev, 'event_count', 'voxel', shape=c['shape'], N=1500)
    with pytest.raises(AssertionError):
        vis.events2frames(ev, 'time', 'voxel_grid', shape=c['shape'], N=1500)
    for name in ('cars', 'bands4'):
        c = vg.cases()[name]
        rng = torch.tensor(c['ranges'], dtype=torch.int64).cuda()
        w = want(name, True, tuple(sorted(dict(NO_FLAGS, reverse_t=True).items())))
        for events in (torch.from_numpy(c['events']).cuda(), torch.from_numpy(vg.packed(c).view(np.int64)).cuda()):
            a = vis.voxel_grid_device(events, rng, c['shape'], reverse_t=True)
            b, grid, stats = vis.voxel_grid_device(events, rng, c['shape'], reverse_t=True, return_grid=True, return_stats=True)
            assert torch.equal(a, b)
            vg.check(dict(frames=a.cpu().numpy(), grid=grid.cpu().numpy(), stats=stats), w)
    # bins != 3: the grid alone
    c = vg.cases()['small8']
    rng = torch.tensor(c['ranges'], dtype=torch.int64).cuda()
    grid, stats = vis.voxel_grid_device(torch.from_numpy(c['events']).cuda(), rng, c['shape'], bins=8, return_grid=True, return_stats=True)
    vg.check(dict(grid=grid.cpu().numpy(), stats=stats), want('small8', True, tuple(sorted(NO_FLAGS.items()))))
    with pytest.raises(ValueError, match='bins=8'):
        vis.voxel_grid_device(torch.from_numpy(c['events']).cuda(), rng, c['shape'], bins=8)


def _grid_samples(n_list, shape, seed):
    """Samples with sorted timestamps on the 1/64 s grid (explicit flips are exact there)."""
    import time_surface_ref as ts
    rng = np.random.default_rng(seed)
    out = []
    for n in n_list:
        ev = ts._scatter(n, shape, int(rng.integers(1 << 30)), 2000)
        ev[:, 2] = np.sort(ev[:, 2])
        out.append(ev)
    return out


def test_pipeline_views_against_explicit_flips(hip):
    """Event2ImagePipeline(convert_method='voxel_grid'): hflip is flip_x, tflip is reverse_t + negate_p on the stored rows
    with the reversed ranges of plan() -- the four test-time-augmentation views against the restatement on arrays
    flipped by oracle.event_utils and chunked as planned; tta() and the other outputs run behind it unchanged."""
    import torch
    from eventclip_amd import vis
    from eventclip_amd.event2img import Event2ImagePipeline
    from oracle import event_utils as eu
    shape, N = (36, 52), 300
    qa = dict(max_imgs=4, N=N, split_method='event_count', convert_method='voxel_grid', grayscale=False,
              background_mask=True, bins=3)
    samples = _grid_samples([1100, 250, 701], shape, seed=5)      # 4 (the last overlapping), 1 and 2 frames
    pipe = Event2ImagePipeline(shape, 1200, qa, n_px=32)
    for hflip, tflip in ((False, False), (True, False), (False, True), (True, True)):
        fr, ri, vm = pipe.plan([len(s) for s in samples], tflip=tflip)
        ev_d = torch.from_numpy(np.concatenate(samples)).cuda()
        got = pipe.frames(ev_d, fr.cuda(), hflip=hflip, tflip=tflip).cpu().numpy()
        frames = []
        for s in samples:
            e = s.copy()
            e = eu.hflip_events(e, shape) if hflip else e
            e = eu.tflip_events(e) if tflip else e
            i0, i1 = vis.chunk_bounds(len(e), N)
            frames.append(vg.oracle(e, list(zip(i0, i1)), shape, 3, True)['frames'])
        w = np.concatenate(frames)
        assert got.shape == w.shape == (4 + 1 + 2, 36, 52, 3)
        np.testing.assert_array_equal(got, w)
    views = pipe.tta(samples)
    assert len(views) == 4 and all(v['img'].shape == (3, 4, 3, 32, 32) for v in views)
    assert not torch.equal(views[0]['img'], views[2]['img'])
    packed = [vis.pack_events(s) for s in samples]
    assert torch.equal(pipe(packed, tflip=True)['img'], views[2]['img'])
    u8 = Event2ImagePipeline(shape, 1200, qa, n_px=32, frames_u8=True)(samples)
    assert u8['frames_u8'].shape == (7, 32, 32, 3) and u8['frames_u8'].dtype == torch.uint8
    pipe.strict = False                                                   # the production op instead of the debug form
    assert torch.equal(pipe(samples)['img'], views[0]['img'])
    pipe.strict = True
    with pytest.raises(ValueError, match='outside the sensor'):
        pipe([vg.cases()['skip']['events']])


def test_the_op_under_fake_tensors_and_opcheck(hip):
    """Shape and dtype through torch.compile's fake tensors, and torch.library.opcheck on the registration."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        fr = torch.zeros(5, 2, dtype=torch.int64, device='cuda')
        for ev in (torch.empty(1000, 4, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')):
            frames = torch.ops.eventclip_hip.events_to_voxel_grid(ev, fr, 181, 240, 3, True, 0, False, False, True, 0)
            assert frames.shape == (5, 181, 240, 3) and frames.dtype == torch.uint8
    c = vg.cases()['small3']
    rng = torch.tensor(c['ranges'], dtype=torch.int64).cuda()
    for events in (torch.from_numpy(c['events']).cuda(), torch.from_numpy(vg.packed(c).view(np.int64)).cuda()):
        torch.library.opcheck(torch.ops.eventclip_hip.events_to_voxel_grid.default,
                              (events, rng, 36, 52, 3, True, len(c['events']), True, False, True, len(c['events'])))
