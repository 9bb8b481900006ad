"""The event-space kernels past their first tile and in their unrolled loops (tests/datapath_cases.py), bit for bit against
the reference-pinned oracles (MI355X): csrc/augment.hip's cross-tile carry and reversed read, the 4 x / 8 x unrolled loops
of the centring kernels of csrc/events.hip, and the grid-stride second pass of its packer."""
import numpy as np
import pytest

import datapath_cases as dc

pytestmark = pytest.mark.gpu


def _ranges(lens):
    import torch
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return offs, torch.from_numpy(np.stack([offs[:-1], offs[1:]], 1)).cuda()


def test_augment_carries_survivors_across_tiles(hip):
    import torch
    from eventclip_amd import augment
    from oracle import event_utils as eu
    res = dc.AUGMENT_RES
    evs = [dc.augment_sample(n, seed=n + 1) for n in dc.AUGMENT_N]
    lens = [len(e) for e in evs]
    cat = torch.from_numpy(np.concatenate(evs)).cuda()
    configs = [(dx, dy, fx, ft) for ft in (0, 1) for dx, dy, fx in dc.AUGMENT_SHIFTS]
    kept = {c: {} for c in configs}                              # config -> {n: share of the events that survive}
    # one launch per round, every sample in it; sample b takes config (b + r) % 8 in round r, so each sample meets each
    for r in range(len(configs)):
        prm = np.array([configs[(b + r) % len(configs)] for b in range(len(evs))], dtype=np.int32)
        out, counts, starts = augment.augment_events_device(cat, lens, prm, res)
        out = out.cpu().numpy()
        for b, e in enumerate(evs):
            if len(e) == 0:
                assert counts[b] == 0                            # the reference has no first event to flip about
                continue
            want = eu.augment_events(e, prm[b], res)
            assert counts[b] == len(want), (lens[b], prm[b].tolist())
            np.testing.assert_array_equal(out[starts[b]:starts[b] + counts[b]], want, err_msg=f'{lens[b]} {prm[b]}')
            kept[tuple(prm[b].tolist())][len(e)] = len(want) / len(e)
    # the cases are what they are meant to be: all kept, about half, none, some; every sample met every one
    for ft in (0, 1):
        (a, b, c, d) = [kept[(dx, dy, fx, ft)] for dx, dy, fx in dc.AUGMENT_SHIFTS]
        assert all(set(k) == set(dc.AUGMENT_N) - {0} for k in (a, b, c, d))
        assert all(v == 1.0 for v in a.values()) and all(v == 0.0 for v in c.values())
        assert all(0.3 < v < 0.7 for n, v in b.items() if n > 1000)
        assert all(0.0 < v < 1.0 for n, v in d.items() if n > 1000)


def test_center_float_unrolled_loops_see_every_event_once(hip):
    import torch
    from eventclip_amd import vis
    from oracle import event_utils as eu
    samples = dc.center_samples(packed=False)
    offs, sr = _ranges([s[1] for s in samples])
    ev = torch.from_numpy(np.concatenate([s[0] for s in samples])).cuda()
    got = vis.center_events_device(ev, sr, dc.CENTER_RES).cpu().numpy()
    for i, (e, n, rot, box) in enumerate(samples):
        want = eu.center_events(e.copy(), dc.CENTER_RES)         # float32 in, float32 arithmetic
        assert want.dtype == np.float32
        np.testing.assert_array_equal(got[offs[i]:offs[i + 1]], want, err_msg=f'n {n} rotation {rot} box {box}')


def test_center_packed_unrolled_loops_see_every_event_once(hip):
    import torch
    from eventclip_amd import vis
    from oracle import event_utils as eu
    samples = dc.center_samples(packed=True)
    offs, sr = _ranges([s[1] for s in samples])
    pk_in = np.concatenate([vis.pack_events(s[0]) for s in samples])
    pk = torch.from_numpy(pk_in.view(np.int64)).cuda()
    vis.center_events_device(pk, sr, dc.CENTER_RES)
    out = pk.cpu().numpy().view(np.uint64)
    got = vis.unpack_events(out)
    for i, (e, n, rot, box) in enumerate(samples):
        want = eu.center_events(e.copy(), dc.CENTER_RES)
        g = got[offs[i]:offs[i + 1]]
        msg = f'n {n} rotation {rot} box {box}'
        np.testing.assert_array_equal(g[:, :2], want[:, :2], err_msg=msg)
        np.testing.assert_array_equal(g[:, 3], want[:, 3], err_msg=msg)
        np.testing.assert_allclose(g[:, 2], want[:, 2], rtol=0, atol=2e-6, err_msg=msg)   # whole microseconds
        # and in integers: every time is the packed input's minus the sample's smallest
        t_in = pk_in[offs[i]:offs[i + 1]] >> np.uint64(34)
        np.testing.assert_array_equal(out[offs[i]:offs[i + 1]] >> np.uint64(34), t_in - t_in.min(), err_msg=msg)


def test_center_packed_wraps_below_zero_like_the_float_path_drops(hip):
    """A shift larger than the smallest coordinate: the packed coordinate wraps past 32768 and the binning kernel drops
    the event, as it drops the float path's negative coordinate; the frames are those of the float-centred sample."""
    import torch
    from eventclip_amd import vis
    from oracle import event_utils as eu
    from oracle import events as oe
    H, W = dc.CENTER_RES
    n = 8193
    e, _ = dc.center_sample(n, dc.center_holders(n, True), 3, dc.CENTER_BOX_WRAPS, seed=5)
    want = eu.center_events(e.copy(), dc.CENTER_RES)
    assert want[:, 0].min() < 0 and want[:, 1].min() < 0
    _, sr = _ranges([n])
    pk = torch.from_numpy(vis.pack_events(e).view(np.int64)).cuda()
    vis.center_events_device(pk, sr, dc.CENTER_RES)
    got = vis.unpack_events(pk.cpu().numpy().view(np.uint64))
    neg = (want[:, 0] < 0) | (want[:, 1] < 0)
    np.testing.assert_array_equal(got[:, 0], np.where(want[:, 0] < 0, want[:, 0] + 65536, want[:, 0]))
    np.testing.assert_array_equal(got[:, 1], np.where(want[:, 1] < 0, want[:, 1] + 65536, want[:, 1]))
    inside = ~neg & (want[:, 0] < W) & (want[:, 1] < H)
    assert 0 < inside.sum() < n
    frames = vis.events_to_frames_device(pk, sr, dc.CENTER_RES, grayscale=False, max_frame_events=n)
    ref = oe.events2frames(want[inside], shape=dc.CENTER_RES, N=int(inside.sum()) + 1, grayscale=False)
    assert ref.shape[0] == 1
    np.testing.assert_array_equal(frames.cpu().numpy(), ref)
    # the float kernel on the same sample, through the same frames
    ev = vis.center_events_device(torch.from_numpy(e).cuda(), sr, dc.CENTER_RES)
    np.testing.assert_array_equal(ev.cpu().numpy(), want)
    frames = vis.events_to_frames_device(ev, sr, dc.CENTER_RES, grayscale=False, max_frame_events=n)
    np.testing.assert_array_equal(frames.cpu().numpy(), ref)


def test_pack_second_grid_stride_pass(hip):
    import torch
    from eventclip_amd import vis
    n = dc.PACK_N
    assert dc.pack_path(n)['passes'] == 2
    rng = np.random.default_rng(12)
    ev = np.empty((n, 4), dtype=np.float32)
    ev[:, 0] = rng.integers(0, 640, size=n)
    ev[:, 1] = rng.integers(0, 480, size=n)
    ev[:, 2] = np.sort(rng.uniform(0.0, 0.5, size=n))
    ev[:, 3] = rng.integers(-1, 2, size=n)
    # in the last 300, read by the second pass alone: three events with no packed form and a time that saturates
    first = dc.PACK_GRID
    ev[first + 17, 0] = 11.5
    ev[first + 101, 1] = -3.0
    ev[first + 257, 0] = 70000.0
    ev[first + 299, 2] = 2000.0                                  # 2e9 us > 2^30 - 1
    bad_at = [first + 17, first + 101, first + 257]
    good = np.ones(n, dtype=bool)
    good[bad_at] = False
    got, bad = vis.pack_events_device(torch.from_numpy(ev).cuda(), return_bad=True)
    got = got.cpu().numpy().view(np.uint64)
    assert bad == len(bad_at)
    with pytest.raises(ValueError):
        vis.pack_events(ev)
    np.testing.assert_array_equal(got[good], vis.pack_events(ev[good]))
    assert int(got[first + 299] >> np.uint64(34)) == vis.PACKED_T_MAX
    # the unrepresentable ones are neutralised (polarity code 0) and keep their time
    np.testing.assert_array_equal((got[bad_at] >> np.uint64(32)) & np.uint64(3), [0, 0, 0])
    t_us = np.rint(ev[bad_at, 2].astype(np.float64) * 1e6).astype(np.uint64)
    np.testing.assert_array_equal(got[bad_at] >> np.uint64(34), t_us)
