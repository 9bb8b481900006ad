"""The yardstick of the refractory-period filter (include/eventclip_refractory.h, steps 1 - 4): the definition restated
twice (``oracle``: one lexsort by (class, tick, row) and a walk over every class run, all runs at once; ``oracle_loop``: a
plain Python walk over the rows in (tick, row) order with a dict of last kept ticks), a numpy model of the kernel's
structure -- row bands without a halo, per-band class lists in scatter order, the chain by selection, one lane or one wave
a list -- with switches that plant faults (``kernel_model``), the case table, and the check function the CPU and the GPU
tests share (``check``: tests/denoise_ref.py's, as are the guarded buffers and ``rows``).  The reference has no such
filter: these restatements ARE the reference answer, and every comparison is exact -- the definition has no float stage."""
import functools

import numpy as np

import denoise_ref as dn
import time_surface_ref as ts
from eventclip_amd import synthetic, vis

TICK_MAX = ts.TICK_MAX
GUARD = dn.GUARD
STATS_DTYPE = dn.STATS_DTYPE                # kept, removed, passed: the same three words
SHAPES = dn.SHAPES
CLASS_WORDS = 32 * 1024                     # the kernel's LDS words: the classes of a band + 1
FAULTS = ('strict', 'retrigger', 'tie_high', 'row_order', 'ignore_polarity', 'split_polarity', 'uncounted_dead_time',
          'x_wrap', 'restart_long', 'reorder')
check, rows, guarded, write_sample, max_sample_events, packed = (dn.check, dn.rows, dn.guarded, dn.write_sample,
                                                                 dn.max_sample_events, dn.packed)


def parse(events, shape):
    """step 1: int64 x, y, p, tick, the bool `counted` and `inside` (no flip, no negation)."""
    H, W = shape
    x, y, p, tick = ts.parse(events, shape)
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return x, y, p, tick, (p != 0) & inside, inside


def classes(x, y, p, W, per_polarity):
    """step 2: the class of every row (meaningful for the counted ones)"""
    return (y * W + x) * 2 + ((p < 0) & bool(per_polarity))


def plan(shape, per_polarity):
    """(rows per band, bands) as ec_refractory_bands plans them; (0, 0) for what is refused"""
    H, W = shape
    rows_fit = (CLASS_WORDS - 1) // (W * (2 if per_polarity else 1))
    if rows_fit < 1:
        return 0, 0
    bands = -(-H // min(H, rows_fit))
    return -(-H // bands), bands


def oracle(events, ranges, shape, period_us, per_polarity=False):
    """The definition, vectorised: the counted events of a sample lexsorted by (class, tick, row); every class run is
    walked from its first event, all runs in step: the next kept event of a run is the first one whose key
    class * 2^32 + tick is at or above that of the last kept one + period."""
    H, W = shape
    period = int(period_us)
    x, y, p, tick, counted, _ = parse(events, shape)
    cls = classes(x, y, p, W, per_polarity)
    out = guarded(events, ranges)
    for s, (b, e) in enumerate(ranges):
        c = counted[b:e]
        idx = np.flatnonzero(c)
        order = np.lexsort((idx, tick[b:e][idx], cls[b:e][idx]))
        key = (cls[b:e][idx][order] << 32) + tick[b:e][idx][order]
        kept_sorted = np.zeros(len(idx), bool)
        first = np.flatnonzero(np.concatenate([[True], key[1:] >> 32 != key[:-1] >> 32])) if len(idx) else np.zeros(0, np.int64)
        end = np.concatenate([first[1:], [len(idx)]]) if len(idx) else first
        at = first.copy()
        while len(at):
            kept_sorted[at] = True
            nxt = np.searchsorted(key, key[at] + period, 'left')
            alive = nxt < end
            at, end = nxt[alive], end[alive]
        kept = np.zeros(e - b, bool)
        kept[idx[order]] = kept_sorted
        write_sample(out, events, s, b, e, c, kept)
    return out


def oracle_loop(events, ranges, shape, period_us, per_polarity=False):
    """The definition as it is written: the rows of a sample in (tick, row) order, a dict class -> last kept tick, in
    Python's integers.  -> {row: kept} for the counted rows of every sample."""
    H, W = shape
    period = int(period_us)
    x, y, p, tick, counted, _ = (a.tolist() for a in parse(events, shape))
    out = {}
    for b, e in ranges:
        last = {}
        for t, i in sorted((tick[i], i) for i in range(b, e) if counted[i]):
            k = (x[i], y[i], p[i] < 0) if per_polarity else (x[i], y[i])
            out[i] = k not in last or t - last[k] >= period
            if out[i]:
                last[k] = t
    return out


def _select_chain(keys, period, strict=False, lanes=1):
    """The kernel's chain on one list of keys (tick << 32 | row) in ANY order: the first kept key is the minimum, the next
    the smallest one >= (last kept tick + period) << 32; `lanes` lanes each take a strided share and the candidates meet in
    a minimum.  -> the kept keys."""
    none = np.iinfo(np.int64).max
    if len(keys) == 0:
        return []
    share = np.full((-(-len(keys) // lanes)) * lanes, none, np.int64)
    share[:len(keys)] = keys
    share = share.reshape(-1, lanes)                                        # column l: the keys of lane l
    kept, bound = [], 0
    while True:
        cand = int(np.where(share >= bound, share, none).min(axis=0).min())   # every lane's minimum, then the wave's
        if cand == none:
            return kept
        kept.append(cand)
        bound = ((cand >> 32) + period + (1 if strict else 0)) << 32


def kernel_model(events, ranges, shape, period_us, per_polarity=False, rows_per_band=None, fault=None, long_list=None):
    """The kernel's structure in numpy: per sample, row bands of ``rows_per_band`` rows (default: the plan's); per band the
    counted events scattered into class lists (in an order no one promises: here reversed), every list's chain solved by
    selection -- by one lane below ``long_list`` keys (default: the header's EC_REFRACTORY_LONG_LIST), by 64 lanes from
    there on.  ``fault`` plants one of FAULTS."""
    assert fault is None or fault in FAULTS
    H, W = shape
    period = int(period_us)
    long_list = int(long_list or vis.REFRACTORY_LONG_LIST)
    split = bool(per_polarity)
    if fault == 'ignore_polarity':
        split = False
    if fault == 'split_polarity':
        split = True
    cpp = 2 if split else 1
    rpb = int(rows_per_band or plan(shape, split)[0])
    x, y, p, tick, counted, inside = parse(events, shape)
    out = guarded(events, ranges)
    for s, (b, e) in enumerate(ranges):
        c = counted[b:e]
        xs, ys, ps, tk = x[b:e], y[b:e], p[b:e], tick[b:e]
        listed = c
        if fault == 'uncounted_dead_time':
            listed = inside[b:e]                                            # p == 0 rows stand in the lists too
        if fault == 'x_wrap':
            listed = (ps != 0) & (xs >= 0) & (xs <= W) & (ys >= 0) & (ys < H)   # x == W: the next row's first pixel
        kept = np.zeros(e - b, bool)
        row = np.arange(e - b, dtype=np.int64)
        for y0 in range(0, H, rpb):
            y1 = min(H, y0 + rpb)
            ncls = (y1 - y0) * W * cpp
            q = ((ys - y0) * W + xs) * cpp + ((ps < 0) & split)
            member = np.flatnonzero(listed & (ys >= y0) & (ys < y1) & (q < ncls))[::-1]
            tie = (0xFFFFFFFF - row) if fault == 'tie_high' else row
            keys = (tk[member] << 32) | tie[member]
            by_class = np.argsort(q[member], kind='stable')
            qs = q[member][by_class]
            starts = np.flatnonzero(np.concatenate([[True], qs[1:] != qs[:-1]])) if len(qs) else []
            ends = list(starts[1:]) + [len(qs)]
            for k0, k1 in zip(starts, ends):
                lst = keys[by_class[k0:k1]]
                if fault == 'retrigger':                                    # against the event before, kept or not
                    srt = np.sort(lst)
                    good = srt[np.concatenate([[True], (srt[1:] >> 32) - (srt[:-1] >> 32) >= period])].tolist()
                elif fault == 'row_order':                                  # the list walked by row, not by tick
                    good, last = [], None
                    for key in sorted(lst.tolist(), key=lambda v: v & 0xFFFFFFFF):
                        if last is None or (key >> 32) - last >= period:
                            good.append(key)
                            last = key >> 32
                elif fault == 'restart_long' and len(lst) >= long_list:     # the chain forgets its last kept event there
                    srt = np.sort(lst)
                    good = _select_chain(srt[:long_list], period) + _select_chain(srt[long_list:], period)
                else:
                    good = _select_chain(lst, period, strict=fault == 'strict', lanes=64 if len(lst) >= long_list else 1)
                good = np.asarray(good, np.int64) & 0xFFFFFFFF
                kept[(0xFFFFFFFF - good) if fault == 'tie_high' else good] = True
        write_sample(out, events, s, b, e, c, kept & c, reorder=fault == 'reorder')
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------
def _case(samples, shape, period_us, gaps=None, random=False, packable=True, expect=None, fast=True):
    """dn._case with this filter's parameter.  expect: None, one keep array for both modes, or (pixel-wide, per-polarity);
    fast: small enough for the Python restatement and the model."""
    c = dn._case(samples, shape, 0, 1, gaps=gaps, random=random, packable=packable)
    del c['dt_us'], c['radius']
    if expect is not None and not isinstance(expect, tuple):
        expect = (expect, expect)
    c.update(period_us=int(period_us), expect=expect, fast=fast)
    return c


def strip(shape, n, width, seed=2, max_t=0.05):
    """synthetic.make_events on a column strip `width` pixels wide, moved to the middle of the sensor: every row, hence
    every band, and few enough pixels that the dead time bites"""
    H, W = shape
    ev = synthetic.make_events(n, (H, width), seed=seed, max_t=max_t)
    ev[:, 0] += (W - width) // 2
    return ev


def _directed(shape, P):
    """One tiny sample per property, all in one launch; -> (samples, expected keep per sample: pixel-wide, per-polarity)."""
    H, W = shape
    S, K0, K1 = [], [], []

    def add(x, y, tick, keep, keep_pp=None, p=None):
        S.append(rows(x, y, tick, p))
        K0.append(list(keep))
        K1.append(list(keep if keep_pp is None else keep_pp))

    cx, cy = W // 2, H // 2
    one = [1, 1, 1, 1, 1, 1, 1, 1]
    add([cx], [cy], [500], [1])                                                          # a lone event
    add([cx] * 2, [cy] * 2, [500, 500 + P], [1, 1], p=one[:2])                           # a gap of exactly the period
    add([cx] * 2, [cy] * 2, [500, 499 + P], [1, 0], p=one[:2])                           # ... and of period - 1
    add([cx] * 5, [cy] * 5, [0, P - 1, P, 2 * P - 1, 2 * P], [1, 0, 1, 0, 1], p=one[:5])  # a removed event extends nothing
    add([cx] * 2, [cy] * 2, [500 + P, 500], [1, 1], p=one[:2])                           # the later one stored first
    add([cx] * 2, [cy] * 2, [499 + P, 500], [0, 1], p=one[:2])
    add([cx] * 3, [cy] * 3, [700, 700, 700], [1, 0, 0], p=one[:3])                       # equal ticks: the lowest row
    add([cx] * 4, [cy] * 4, [700 + P, 700, 700 + P, 700], [1, 1, 0, 0], p=one[:4])       # ... with the later tick stored first
    add([cx] * 6, [cy] * 6, [5 * P, 3 * P + 1, 0, P - 1, 3 * P, 2 * P - 2], [1, 0, 1, 0, 1, 1], p=one[:6])   # unsorted
    # ON / OFF alternation: one dead time pixel-wide, two per polarity
    add([cx] * 6, [cy] * 6, [0, 1, P, P + 1, 2 * P - 1, 2 * P + 1], [1, 0, 1, 0, 0, 1], [1, 1, 1, 1, 0, 1], p=[1, -1, 1, -1, 1, -1])
    add([cx] * 4, [cy] * 4, [10, 10, 11, 11], [1, 0, 0, 0], [1, 1, 0, 0], p=[-1, 1, 1, -1])
    # p == 0 and out-of-sensor rows between two events of one pixel: they pass (1) and start no dead time
    add([cx, cx, W, cx, cx, cx], [cy, cy, cy, H + 3, H, cy], [500, 501, 502, 503, 504, 505], [1, 1, 1, 1, 1, 0],
        p=[1, 0, 1, -1, 1, 1])
    add([cx, cx, cx], [cy, cy, cy], [500, 500 + P, 550 + P], [1, 1, 1], p=[1, 0, 1])     # the p == 0 row blinds no one
    # x == W of a row against the first pixel of the next: two pixels only for an index that wraps
    add([W, 0], [cy, cy + 1], [500, 505], [1, 1], p=[1, 1])
    add([W - 1, 0, W - 1, 0], [cy, cy + 1, cy, cy + 1], [500, 501, 502, 503], [1, 1, 0, 0], p=one[:4])
    for x0, y0 in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):                      # corners
        add([x0] * 3, [y0] * 3, [500, 500 + P - 1, 500 + P], [1, 0, 1], p=one[:3])
    add([0, W - 1, 0, W - 1], [0, H - 1, 0, H - 1], [500, 501, 502, 503], [1, 1, 0, 0], p=one[:4])   # first and last class
    add([], [], [], [])                                                                  # an empty sample
    return S, (K0, K1)


def _row_pairs(shape):
    """For EVERY row boundary y | y + 1: the pixels (x, y) and (x, y + 1) fire 1 tick apart, then each again inside its own
    dead time.  Whatever band cut a kernel makes, a pair straddles it: the first two are kept (two classes), the second two
    removed; a class that leaked across the cut, or was split by it, shows."""
    H, W = shape
    xs, ys, tt, keep = [], [], [], []
    for y in range(H - 1):
        x = (7 * y) % W
        up_first = y % 2 == 0
        a, b = ((x, y), (x, y + 1)) if up_first else ((x, y + 1), (x, y))
        xs += [a[0], b[0], b[0], a[0]]
        ys += [a[1], b[1], b[1], a[1]]
        tt += [1000 * (y + 1), 1000 * (y + 1) + 1, 1000 * (y + 1) + 40, 1000 * (y + 1) + 41]
        keep += [1, 1, 0, 0]
    return rows(xs, ys, tt, p=np.ones(len(xs))), np.array(keep)


LIST_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 4096)


def list_lengths():
    """the class-list lengths of the `lists_*` cases: around the wave, around EC_REFRACTORY_LONG_LIST wherever it stands, and
    the most events any test feeds one class"""
    L = vis.REFRACTORY_LONG_LIST
    return tuple(sorted(set(LIST_LENGTHS) | {max(1, L - 1), L, L + 1}))


def _lists(shape, spacing=10):
    """One pixel per length of list_lengths(), its events `spacing` ticks apart from a start of its own, all shuffled."""
    H, W = shape
    rng = np.random.default_rng(31)
    xs, ys, tt = [], [], []
    for k, n in enumerate(list_lengths()):
        xs += [(5 * k + 1) % W] * n
        ys += [(3 * k + 2) % H] * n
        tt += (k + spacing * np.arange(n)).tolist()
    order = rng.permutation(len(xs))
    return rows(np.array(xs)[order], np.array(ys)[order], np.array(tt)[order], p=np.where(rng.random(len(xs)) < 0.5, 1., -1.)[order])


@functools.lru_cache(None)
def cases():
    """name -> dict(events float32 [n, 4], ranges, shape, period_us, random, packable, expect, fast).  `expect`: the keep
    bytes of every row inside a range for (pixel-wide, per-polarity), known by construction (None where only the
    restatements say)."""
    C = {}
    small = (37, 53)
    # random streams: 10 % .. 90 % kept in both modes, asserted by the CPU test.  The two large sensors as column strips:
    # over the whole sensor 20 000 events keep more than 95 %
    C['rand_small'] = _case([synthetic.make_events(3000, small, seed=2, max_t=0.05)], small, 20000, random=True)
    C['rand_100'] = _case([synthetic.make_events(8000, (100, 120), seed=2, max_t=0.05)], (100, 120), 20000, random=True)
    C['rand_180'] = _case([strip((180, 240), 20000, 24)], (180, 240), 15000, random=True, fast=False)
    C['rand_480'] = _case([strip((480, 640), 20000, 16)], (480, 640), 15000, random=True, fast=False)
    three = [strip((180, 240), n, 24, seed=5 + i) for i, n in enumerate((9000, 15000, 4000))]
    C['rand_180_three'] = _case(three, (180, 240), 10000, random=True, fast=False)
    sh = synthetic.make_events(4000, small, seed=9, max_t=0.05, p_zero_frac=0.1)
    C['rand_small_unsorted'] = _case([sh[np.random.default_rng(3).permutation(len(sh))]], small, 20000, random=True)
    # directed
    for shape in SHAPES:
        S, (K0, K1) = _directed(shape, 100)
        C[f'directed_{shape[0]}'] = _case(S, shape, 100, expect=tuple(np.concatenate([np.array(k, np.int64) for k in K]) for K in (K0, K1)))
        ev, keep = _row_pairs(shape)
        C[f'rows_{shape[0]}'] = _case([ev], shape, 100, expect=keep)
    # a sensor whose last band is a partial one (100 x 700 pixel-wide: bands of 34, 34 and 32 rows)
    S, (K0, K1) = _directed((100, 700), 100)
    C['directed_partial'] = _case(S, (100, 700), 100, expect=tuple(np.concatenate([np.array(k, np.int64) for k in K]) for K in (K0, K1)))
    ev, keep = _row_pairs((100, 700))
    C['rows_partial'] = _case([ev], (100, 700), 100, expect=keep)
    C['period1'] = _case([rows([5] * 7, [5] * 7, [300, 300, 301, 302, 302, 302, 303], p=[1, 1, 1, -1, 1, -1, 1])], small, 1,
                         expect=(np.array([1, 0, 1, 1, 0, 0, 1]), np.array([1, 0, 1, 1, 1, 0, 1])))
    C['extremes'] = _case([rows([5, 5, 6, 6, 7, 7], [5] * 6, [0, 5, 1, 5, 0, 5], p=np.ones(6))], small, TICK_MAX,
                          expect=np.array([1, 1, 1, 0, 1, 0]))
    C['extremes']['events'][1, 2] = 2000.                                       # float seconds past the clip: tick 2^30 - 1
    C['extremes']['events'][3, 2] = 1073.741822                                 # ... and just short of it
    # class lists of every length the chain treats differently, on one pixel each, shuffled; periods that keep all, about
    # half and one of them
    lists = _lists(small)
    for name, period in (('lists_all', 10), ('lists_half', 11), ('lists_one', 50000)):
        C[name] = _case([lists], small, period, fast=False)
    hot_t = np.sort(np.random.default_rng(21).integers(0, 50000, 2000))
    hot = rows([10] * 2000 + [11] * 5, [10] * 2005, np.concatenate([hot_t, [40, 10000, 20000, 30000, 49990]]))
    C['hot'] = _case([hot[np.random.default_rng(22).permutation(2005)]], small, 200, fast=False)
    # sample lengths around the wave, the workgroup and the scan's 8 x 1024 rows per round
    pool = synthetic.make_events(9000, small, seed=4, max_t=0.1)
    lens, at, S = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4097), 0, []
    for n in lens:
        S.append(pool[at:at + n])
        at += n
    C['lengths'] = _case(S, small, 20000)
    pool = synthetic.make_events(8191 + 8192 + 8193, small, seed=14, max_t=0.3)
    C['lengths_unroll'] = _case([pool[:8191], pool[8191:8191 + 8192], pool[8191 + 8192:]], small, 20000, random=True, fast=False)
    many = synthetic.make_events(600 * 40, (8, 8), seed=6, max_t=0.02 * 600)
    C['many'] = _case([many[40 * i:40 * i + 40] for i in range(600)], small, 5000)          # 600 samples in one launch
    g = synthetic.make_events(3000, small, seed=8, max_t=0.05)
    C['gapped'] = _case([g[:900], g[900:2300], g[2300:2301], g[2301:]], small, 20000, gaps=(5, 0, 130, 1))
    sk = synthetic.make_events(2500, small, seed=10, max_t=0.05, p_zero_frac=0.15)
    out_of = np.random.default_rng(5).random(2500)
    sk[out_of < 0.05, 0] = small[1]                                              # x == W, and y == H + 3: outside the sensor
    sk[out_of > 0.96, 1] = small[0] + 3
    C['skip'] = _case([sk], small, 20000)
    fr = synthetic.make_events(2000, small, seed=12, max_t=0.05)
    fr[:, 0] += np.float32(0.7) * (np.arange(2000) % 3 == 0)                     # truncating casts: 3.7 -> 3
    fr[::17, 0] = -0.5                                                           # -> 0: inside
    fr[::19, 1] = -1.0                                                           # outside
    fr[::23, 3] = 0.4                                                            # p -> 0: not counted
    fr[::29, 3] = -1.6                                                           # p -> -1
    C['frac'] = _case([fr], small, 20000, packable=False)
    return C


def expected_keep(c, per_polarity):
    """`expect` laid out like the keep output: GUARD outside every range"""
    return dn.expected_keep(dict(c, expect=c['expect'][int(bool(per_polarity))]))


def kept_share(w):
    """kept / counted over a launch's stats"""
    return float(w['stats']['kept'].sum()) / max(1, int(w['stats']['kept'].sum() + w['stats']['removed'].sum()))
