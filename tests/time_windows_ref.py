"""The yardstick of the fixed-duration windows (include/eventclip_time_windows.h, steps 1 - 7): the definition restated in
numpy int64, twice -- by counting, ``(ticks < e).sum()``, and by ``np.searchsorted`` -- and the case tables the CPU and the
GPU tests share.  Nothing here touches the device or the library."""
import functools

import numpy as np

TICK_MAX = 2 ** 30 - 1
STATS_DTYPE = np.dtype([('t_first', '<u4'), ('t_last', '<u4'), ('unsorted', '<u4'), ('windows', '<i4')])
PREFILL = -1          # what the Python layers put into the rows of bounds a call does not write
SLICE, UNROLL = 2048, 8               # EC_TIME_WINDOWS_SLICE_ROWS, EC_TIME_WINDOWS_UNROLL: the GPU test checks them against the header
THREADS = SLICE // UNROLL


# ---- step 1: ticks ----
def ticks_of(events):
    """float32 [n, 4] rows -> clip(rint((double)t * 1e6), 0, 2^30 - 1); packed uint64 [n] -> the upper 30 bits."""
    ev = np.asarray(events)
    if ev.ndim == 1:
        return (ev.astype(np.uint64) >> np.uint64(34)).astype(np.int64)
    return np.clip(np.rint(ev[:, 2].astype(np.float32).astype(np.float64) * 1e6), 0, TICK_MAX).astype(np.int64)


def float_events(ticks, seed=0):
    """float32 [n, 4] rows whose ticks are exactly ``ticks`` (checked), x, y, p seeded: integers a packed event holds."""
    ticks = np.asarray(ticks, dtype=np.int64)
    r = np.random.default_rng(seed)
    ev = np.zeros((len(ticks), 4), dtype=np.float32)
    ev[:, 0], ev[:, 1] = r.integers(0, 52, len(ticks)), r.integers(0, 36, len(ticks))
    ev[:, 2] = (ticks.astype(np.float64) / 1e6).astype(np.float32)
    ev[:, 3] = r.choice([-1., 1.], len(ticks))
    assert (ticks_of(ev) == ticks).all(), 'these ticks are not float32 seconds: use smaller ones'
    return ev


def packed_events(ticks, seed=0):
    """uint64 [n] packed events (x | y << 16 | code << 32 | t_us << 34) with the x, y, p of ``float_events``."""
    ticks = np.asarray(ticks, dtype=np.int64)
    r = np.random.default_rng(seed)
    x, y = r.integers(0, 52, len(ticks)).astype(np.uint64), r.integers(0, 36, len(ticks)).astype(np.uint64)
    code = np.where(r.choice([-1., 1.], len(ticks)) > 0, 1, 2).astype(np.uint64)
    return x | (y << np.uint64(16)) | (code << np.uint64(32)) | (ticks.astype(np.uint64) << np.uint64(34))


# ---- steps 2 - 6, by counting ----
def sample_by_counting(t, begin, dt_us, stride_us, from_last, most=None):
    """ticks of one sample (int64 [n], n > 0) -> (stats tuple, bounds int64 [windows, 2]); bounds None if unsorted.
    most: state the first ``most`` windows only (stats.windows stays the full count)."""
    t = np.asarray(t, dtype=np.int64)
    unsorted = int((t[1:] < t[:-1]).sum())
    t_first, t_last = int(t[0]), int(t[-1])
    if unsorted:
        return (t_first, t_last, unsorted, -1), None
    windows = (t_last - t_first) // stride_us + 1
    stated = windows if most is None else min(windows, most)
    out = np.zeros((stated, 2), dtype=np.int64)
    for k in range(stated):
        if not from_last:
            lo = t_first + k * stride_us
            out[k] = begin + int((t < lo).sum()), begin + int((t < lo + dt_us).sum())
        else:
            d = t_last - t
            out[k] = begin + int((d >= k * stride_us + dt_us).sum()), begin + int((d >= k * stride_us).sum())
    return (t_first, t_last, 0, windows), out


# ---- the same by binary search ----
def sample_by_search(t, begin, dt_us, stride_us, from_last, most=None):
    t = np.asarray(t, dtype=np.int64)
    unsorted = int(np.count_nonzero(np.diff(t) < 0))
    t_first, t_last = int(t[0]), int(t[-1])
    if unsorted:
        return (t_first, t_last, unsorted, -1), None
    windows = (t_last - t_first) // stride_us + 1
    k = np.arange(windows if most is None else min(windows, most), dtype=np.int64)
    if not from_last:
        lo = t_first + k * stride_us
        out = np.stack([np.searchsorted(t, lo, 'left'), np.searchsorted(t, lo + dt_us, 'left')], 1)
    else:
        # d_i >= x  <=>  t_i <= t_last - x: the rows up to the last such tick
        out = np.stack([np.searchsorted(t, t_last - k * stride_us - dt_us, 'right'),
                        np.searchsorted(t, t_last - k * stride_us, 'right')], 1)
    return (t_first, t_last, 0, windows), begin + out.astype(np.int64)


def oracle(ticks, ranges, dt_us, stride_us, max_windows, from_last, how=sample_by_counting):
    """ticks int64 [n_total]; ranges [(begin, end)] -> dict(bounds int64 [B, max_windows, 2] with PREFILL where the definition
    writes nothing, stats STATS_DTYPE [B], sorted bool [B]).  An empty sample: windows 0, the other words 0 here (the
    kernel leaves them alone: the tests compare ``windows`` only there)."""
    B = len(ranges)
    bounds = np.full((B, max_windows, 2), PREFILL, dtype=np.int64)
    stats = np.zeros(B, dtype=STATS_DTYPE)
    for b, (e0, e1) in enumerate(ranges):
        if e1 <= e0:
            continue
        st, rows = how(ticks[e0:e1], e0, dt_us, stride_us, from_last, max_windows)
        stats[b] = st
        if rows is not None:
            bounds[b, :len(rows)] = rows
    return dict(bounds=bounds, stats=stats, sorted=stats['windows'] >= 0)


def check(got, want, ranges):
    """bounds of the sorted samples (prefill behind the written rows included) and stats, exactly.  An unsorted sample's
    bounds are unspecified; an empty sample's stats are compared in ``windows`` alone."""
    for b, (e0, e1) in enumerate(ranges):
        if e1 <= e0:
            assert got['stats']['windows'][b] == 0, f'sample {b}: empty, windows {got["stats"]["windows"][b]}'
            np.testing.assert_array_equal(got['bounds'][b], want['bounds'][b], err_msg=f'bounds of the empty sample {b}')
            continue
        assert got['stats'][b] == want['stats'][b], f'stats of sample {b}: {got["stats"][b]} != {want["stats"][b]}'
        if want['sorted'][b]:
            np.testing.assert_array_equal(got['bounds'][b], want['bounds'][b], err_msg=f'bounds of sample {b}')


# ---- the case tables ----
def _steps(n, seed, lo=0, most=400):
    """n sorted ticks from `lo` with random steps 0 .. most (many equal neighbours)."""
    r = np.random.default_rng(seed)
    return lo + np.concatenate([[0], np.cumsum(r.integers(0, most + 1, max(n - 1, 0)) * r.integers(0, 2, max(n - 1, 0)))])[:n]


def _case(ticks, ranges, dt_us, stride_us, max_windows=16, floatable=True):
    return dict(ticks=np.asarray(ticks, dtype=np.int64), ranges=[tuple(map(int, r)) for r in ranges], dt_us=int(dt_us),
                stride_us=int(stride_us), max_windows=int(max_windows), floatable=floatable)


@functools.lru_cache(None)
def cases():
    """name -> dict(ticks, ranges, dt_us, stride_us, max_windows, floatable).  Every case runs with from_last 0 and 1, on
    packed events and (floatable: ticks that float32 seconds hold exactly) on float rows."""
    c = {}
    # sample lengths around the wave, the slice and the unroll round
    for n in (1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1):
        t = _steps(n, n, lo=1000, most=60)
        c[f'n{n}'] = _case(t, [(0, n)], 5000, 5000, max_windows=24)
        c[f'n{n}_hop'] = _case(t, [(0, n)], 9000, 4000, max_windows=40)
    # a tick step exactly at a slice boundary (rows SLICE - 1 | SLICE), an edge on it; and none there
    t = np.repeat([100, 5100], [SLICE, 700])
    c['step_at_slice'] = _case(t, [(0, len(t))], 5000, 5000)
    t = np.repeat([100, 5100], [SLICE - 5, 705])
    c['no_step_at_slice'] = _case(t, [(0, len(t))], 5000, 5000)
    # the virtual row is the first of a slice (n == SLICE) and the upper edges land on it
    c['end_at_slice'] = _case(np.full(SLICE, 777), [(0, SLICE)], 10, 10)
    c['all_equal'] = _case(np.full(300, 123456), [(0, 300)], 1000, 1000)
    # events exactly on a lower edge (they belong) and on an upper edge (they do not), both anchors
    c['on_edges'] = _case([0, 0, 999, 1000, 1000, 1001, 1999, 2000, 2999, 3000], [(0, 10)], 1000, 1000)
    c['on_edges_hop'] = _case([10, 510, 1009, 1010, 1011, 1510, 2010, 2011], [(0, 8)], 1000, 500)
    c['stride_lt'] = _case(_steps(900, 5, most=90), [(0, 900)], 7000, 2500, max_windows=32)
    c['stride_eq'] = _case(_steps(900, 6, most=90), [(0, 900)], 4000, 4000, max_windows=32)
    c['stride_gt'] = _case(_steps(900, 7, most=90), [(0, 900)], 1500, 6000, max_windows=32)       # events in no window
    # a silent gap spanning more windows than max_windows; and in mid-stream with windows behind it
    c['gap_over'] = _case(np.concatenate([_steps(100, 8, most=20), 10 ** 6 + _steps(100, 9, most=20)]), [(0, 200)], 1000, 1000, 16)
    c['gap_mid'] = _case(np.concatenate([_steps(100, 8, most=20), 9000 + _steps(100, 9, most=20)]), [(0, 200)], 1000, 1000, 32)
    c['over_max'] = _case(_steps(500, 10, most=300), [(0, 500)], 2000, 1000, 8)                   # windows > max_windows
    # dt = stride = 1 with ticks near 2^30 - 1: the edges pass 2^30; and a window of 2^30 - 1 from there: the edges pass 2^31
    near = TICK_MAX - np.array([9, 9, 7, 6, 6, 3, 1, 0, 0])
    c['unit_near_max'] = _case(near, [(0, 9)], 1, 1, 16, floatable=False)
    c['huge_near_max'] = _case(near, [(0, 9)], TICK_MAX, 3, 16, floatable=False)
    c['huge_stride'] = _case([0, 5, TICK_MAX - 1, TICK_MAX], [(0, 4)], TICK_MAX, TICK_MAX, 4, floatable=False)
    # samples not back to back, odd begins, an empty sample and a reversed range among them
    t = np.concatenate([_steps(700, 11, most=50), _steps(1, 12), _steps(333, 13, lo=50, most=70), _steps(129, 14, most=10)])
    c['gapped'] = _case(t, [(3, 640), (701, 701), (700, 701), (711, 1001), (1040, 1035), (1035, 1163)], 3000, 1700, 20)
    # sorted samples around one unsorted sample
    a, b, d = _steps(500, 15, most=40), _steps(800, 16, most=40).copy(), _steps(300, 17, most=40)
    b[[5, 6, 400, 799]] = [0, 0, 3, 1]
    c['one_unsorted'] = _case(np.concatenate([a, b, d]), [(0, 500), (500, 1300), (1300, 1600)], 2500, 2500, 24)
    # descents across the wave, the round and the slice boundary
    t = _steps(2 * SLICE + 100, 18, lo=10 ** 5, most=3).copy()
    for i in (64, THREADS, SLICE, 2 * SLICE):
        t[i] = t[i - 1] - 1
    c['descents_at_boundaries'] = _case(t, [(0, len(t))], 800, 800, 16)
    # 32 seeded random small batches
    for s in range(32):
        r = np.random.default_rng(1000 + s)
        lens = r.integers(1, 400, r.integers(1, 6))
        gaps = r.integers(0, 7, len(lens))
        ranges, parts, at = [], [], 0
        for n, g in zip(lens, gaps):
            parts.append(np.zeros(g, dtype=np.int64))
            parts.append(_steps(int(n), 2000 + 10 * s + len(ranges), lo=int(r.integers(0, 5000)), most=int(r.integers(1, 200))))
            ranges.append((at + g, at + g + int(n)))
            at += g + int(n)
        dt = int(r.integers(1, 4000))
        c[f'rand{s:02d}'] = _case(np.concatenate(parts), ranges, dt, int(r.integers(1, 2 * dt + 1)), int(r.integers(1, 40)))
    return c


def float_saturation_events():
    """float rows whose seconds pass the tick range: t >= 1073.741823 s saturates at 2^30 - 1, t < 0 at 0."""
    t = np.array([-2., -0.5, 0., 1e-6, 5e-6, 1073.7, 1073.75, 1100., 3e4, np.float32(3e9)], dtype=np.float32)
    ev = np.zeros((len(t), 4), dtype=np.float32)
    ev[:, 2], ev[:, 3] = t, 1
    return ev
