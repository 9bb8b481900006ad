"""The refractory-period filter without a device: the two restatements of include/eventclip_refractory.h agree on every
case in both modes, the keep set has the property that makes it unique, filtering is idempotent, per-polarity is the
pixel-wide filter on the ON and the OFF rows apart, a period of one tick removes exactly the duplicates, a shuffle changes
nothing where no ticks tie, float rows and packed events decide alike, the random cases are not vacuous, `check` catches
every planted fault of the kernel's model -- and the layers around the kernel that need no GPU: the header against its
bindings, the band plan, the workspace query, every refusal, the custom op's registration, the pipeline's arguments."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import refractory_ref as rf
from eventclip_amd import _lib, vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (False, True)
FAST = sorted(n for n, c in rf.cases().items() if c['fast'])


@functools.lru_cache(None)
def want(name, per_polarity, packed=False):
    c = rf.cases()[name]
    return rf.oracle(rf.packed(c) if packed else c['events'], c['ranges'], c['shape'], c['period_us'], per_polarity)


def inside(c):
    m = np.zeros(len(c['events']), bool)
    for b, e in c['ranges']:
        m[b:e] = True
    return m


@pytest.mark.parametrize('name', sorted(rf.cases()))
def test_the_two_restatements_agree_and_match_what_is_known_by_construction(name):
    c = rf.cases()[name]
    _, _, _, _, counted, _ = rf.parse(c['events'], c['shape'])
    for pp in MODES:
        w = want(name, pp)
        loop = rf.oracle_loop(c['events'], c['ranges'], c['shape'], c['period_us'], pp)
        assert sorted(loop) == np.flatnonzero(counted & inside(c)).tolist()
        assert all(bool(w['keep'][i]) == k for i, k in loop.items())
        assert ((w['keep'] == 1) | counted)[inside(c)].all()                   # uncounted rows pass
        st = w['stats']
        np.testing.assert_array_equal(st['kept'].astype(np.int64) + st['passed'], w['counts'])
        np.testing.assert_array_equal(st['kept'].astype(np.int64) + st['removed'] + st['passed'], [e - b for b, e in c['ranges']])
        if c['expect'] is not None:
            np.testing.assert_array_equal(w['keep'], rf.expected_keep(c, pp))


@pytest.mark.parametrize('name', sorted(rf.cases()))
def test_the_keep_set_is_the_one_the_definition_allows(name):
    """kept ticks of a class pairwise >= period apart, the first of every class kept, every removed event < period after
    the most recent kept event of its class: one keep set only has all three"""
    c = rf.cases()[name]
    x, y, p, tick, counted, _ = rf.parse(c['events'], c['shape'])
    for pp in MODES:
        cls = rf.classes(x, y, p, c['shape'][1], pp)
        keep = want(name, pp)['keep']
        for b, e in c['ranges']:
            idx = b + np.flatnonzero(counted[b:e])
            order = idx[np.lexsort((idx, tick[idx], cls[idx]))]
            k, t, q = keep[order] == 1, tick[order], cls[order]
            first = np.concatenate([[True], q[1:] != q[:-1]]) if len(order) else np.zeros(0, bool)
            assert k[first].all()
            last_kept = np.maximum.accumulate(np.where(k, np.arange(len(order)), -1))      # (inside a run: its first is kept)
            prev_kept = np.concatenate([[-1], last_kept[:-1]]) if len(order) else last_kept
            later = ~first
            assert (t[later & k] - t[prev_kept[later & k]] >= c['period_us']).all()
            assert (t[~k] - t[prev_kept[~k]] < c['period_us']).all() and (q[~k] == q[prev_kept[~k]]).all()


@pytest.mark.parametrize('name', ['rand_small', 'rand_small_unsorted', 'rand_180', 'hot', 'lists_half', 'skip', 'directed_37'])
def test_filtering_the_survivors_again_removes_nothing(name):
    c = rf.cases()[name]
    for pp in MODES:
        w = want(name, pp)
        surv = [c['events'][b:e][w['keep'][b:e] == 1] for b, e in c['ranges']]
        again = rf._case(surv, c['shape'], c['period_us'])
        w2 = rf.oracle(again['events'], again['ranges'], c['shape'], c['period_us'], pp)
        assert not w2['stats']['removed'].any()
        np.testing.assert_array_equal(w2['counts'], w['counts'])


@pytest.mark.parametrize('name', ['rand_small', 'rand_small_unsorted', 'rand_480', 'directed_100', 'period1', 'frac'])
def test_per_polarity_is_the_pixel_wide_filter_on_the_on_rows_and_the_off_rows_apart(name):
    c = rf.cases()[name]
    p = rf.parse(c['events'], c['shape'])[2]
    keep = np.zeros(len(c['events']), bool)
    for sign in (1, -1):
        ev = c['events'].copy()
        ev[np.sign(p) != sign, 3] = 0                                          # the other polarity: not counted
        keep |= (rf.oracle(ev, c['ranges'], c['shape'], c['period_us'], False)['keep'] == 1) & (np.sign(p) == sign)
    got = want(name, True)['keep']
    np.testing.assert_array_equal((got == 1)[p != 0], keep[p != 0])


def test_a_period_of_one_tick_removes_exactly_the_same_tick_duplicates_and_keeps_the_lowest_row():
    for name in ('rand_small', 'hot', 'many', 'period1'):
        c = rf.cases()[name]
        x, y, p, tick, counted, _ = rf.parse(c['events'], c['shape'])
        for pp in MODES:
            cls = rf.classes(x, y, p, c['shape'][1], pp)
            w = rf.oracle(c['events'], c['ranges'], c['shape'], 1, pp)
            for s, (b, e) in enumerate(c['ranges']):
                seen, expect = set(), np.ones(e - b, bool)
                for i in range(b, e):
                    if counted[i]:
                        expect[i - b] = (cls[i], tick[i]) not in seen
                        seen.add((cls[i], tick[i]))
                np.testing.assert_array_equal(w['keep'][b:e] == 1, expect)
    assert rf.oracle(rf.cases()['hot']['events'], rf.cases()['hot']['ranges'], (37, 53), 1)['stats']['removed'][0] > 0


@pytest.mark.parametrize('name', ['rand_small', 'rand_180_three', 'lists_half', 'lists_one', 'gapped'])
def test_a_shuffle_of_a_stream_without_equal_ticks_in_a_class_leaves_the_keep_set(name):
    c = rf.cases()[name]
    x, y, p, tick, counted, _ = rf.parse(c['events'], c['shape'])
    ev = c['events'].copy()
    for b, e in c['ranges']:                                                   # take the ties out: uncount all but one of each
        cls = rf.classes(x, y, p, c['shape'][1], False)
        _, firsts = np.unique(np.stack([cls[b:e], tick[b:e]]), axis=1, return_index=True)
        dup = np.ones(e - b, bool)
        dup[firsts] = False
        ev[b:e][dup, 3] = 0
    perm = np.arange(len(ev))
    rng = np.random.default_rng(7)
    for b, e in c['ranges']:
        perm[b:e] = b + rng.permutation(e - b)
    for pp in MODES:
        a = rf.oracle(ev, c['ranges'], c['shape'], c['period_us'], pp)
        bb = rf.oracle(ev[perm], c['ranges'], c['shape'], c['period_us'], pp)
        np.testing.assert_array_equal(bb['keep'], a['keep'][perm])
        np.testing.assert_array_equal(bb['stats'], a['stats'])
        assert a['stats']['removed'].sum() > 0


def test_float_rows_and_packed_events_decide_alike():
    for name, c in rf.cases().items():
        if c['packable'] and (c['fast'] or name in ('rand_180', 'lists_half')):
            for pp in MODES:
                a, b = want(name, pp), want(name, pp, True)
                for k in ('keep', 'counts', 'stats'):
                    np.testing.assert_array_equal(a[k], b[k])
                assert b['events_out'].dtype == np.uint64


def test_the_random_cases_are_not_vacuous():
    """every case marked random keeps between 10 % and 90 % of its counted events in both modes; the four of the table keep
    what the table says"""
    shares = {}
    for name, c in rf.cases().items():
        if c['random']:
            for pp in MODES:
                shares[name, pp] = rf.kept_share(want(name, pp))
                assert 0.10 < shares[name, pp] < 0.90, (name, pp, shares[name, pp])
    for name, a, b in (('rand_small', 0.66, 0.79), ('rand_100', 0.81, 0.89), ('rand_180', 0.45, 0.61), ('rand_480', 0.58, 0.72)):
        assert abs(shares[name, False] - a) < 0.006 and abs(shares[name, True] - b) < 0.006, (name, shares[name, False], shares[name, True])


# ---- the kernel's model and its planted faults ----
MODEL_CASES = FAST + ['lists_half', 'hot']


@pytest.mark.parametrize('name', MODEL_CASES)
def test_the_kernel_model_is_the_definition_at_any_band_cut_and_threshold(name):
    c = rf.cases()[name]
    H = c['shape'][0]
    for pp in MODES:
        w = want(name, pp)
        rf.check(rf.kernel_model(c['events'], c['ranges'], c['shape'], c['period_us'], pp), w)
        if name in ('rand_small', 'directed_37', 'rows_37', 'rows_100', 'lists_half'):
            for rpb, ll in ((1, 2), (7, 3), (H - 1, 64), (H, 10 ** 9)):
                rf.check(rf.kernel_model(c['events'], c['ranges'], c['shape'], c['period_us'], pp, rows_per_band=rpb, long_list=ll), w)


CATCHES = {   # fault -> (case, per_polarity) pairs on which it must show
    'strict': [('directed_37', False), ('directed_480', True), ('lists_all', False)],
    'retrigger': [('directed_37', False), ('rand_small', True), ('hot', False)],
    'tie_high': [('directed_37', False), ('period1', True)],
    'row_order': [('directed_37', False), ('rand_small_unsorted', False), ('lists_half', True)],
    'ignore_polarity': [('directed_37', True), ('rand_small', True), ('period1', True)],
    'split_polarity': [('directed_37', False), ('rand_small', False), ('period1', False)],
    'uncounted_dead_time': [('directed_37', False), ('rand_small_unsorted', False)],
    'x_wrap': [('directed_37', False), ('directed_480', True), ('skip', False)],
    'restart_long': [('lists_one', False), ('lists_one', True), ('hot', False)],
    'reorder': [('directed_37', False), ('rand_small', True), ('many', False)],
}


def test_every_fault_has_its_catches():
    assert sorted(CATCHES) == sorted(rf.FAULTS)


@pytest.mark.parametrize('fault', rf.FAULTS)
def test_check_catches_every_planted_fault(fault):
    for name, pp in CATCHES[fault]:
        c = rf.cases()[name]
        bad = rf.kernel_model(c['events'], c['ranges'], c['shape'], c['period_us'], pp, fault=fault)
        with pytest.raises(AssertionError):
            rf.check(bad, want(name, pp))
        if fault == 'reorder':                                                  # the same rows, another order: only events_out tells
            rf.check({k: bad[k] for k in ('counts', 'keep', 'stats')}, want(name, pp))


def test_check_reads_every_output_and_the_guards():
    w = want('gapped', False)
    for k in ('events_out', 'counts', 'keep', 'stats'):
        bad = {n: v.copy() for n, v in w.items()}
        bad[k].reshape(-1).view(np.uint8)[-1] ^= 1
        with pytest.raises(AssertionError, match=k):
            rf.check(bad, w)
    b, e = rf.cases()['gapped']['ranges'][0]
    assert (w['keep'][:b] == rf.GUARD).all() and w['counts'][0] < e - b
    assert (w['events_out'][b + w['counts'][0]:e].view(np.uint8) == rf.GUARD).all()        # behind the count: not written
    rf.check({'counts': w['counts'], 'keep': None}, w)                          # an output not asked for is not compared


# ---- the layers around the kernel ----
def test_header_declares_the_entries_and_the_library_exports_them(tmp_path):
    text = open(vis.REFRACTORY_HEADER).read()
    names = sorted(set(re.findall(r'EC_API\s+[\w\s\*]+?\b(ec_\w+)\s*\(', text)))
    assert names == ['ec_refractory_bands', 'ec_refractory_events', 'ec_refractory_events_packed',
                     'ec_refractory_workspace_bytes'] == sorted(vis.REFRACTORY_SIGNATURES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f'{n} declared in include/eventclip_refractory.h but not exported'
    assert _lib.lib().ec_version() == _lib.ABI_VERSION >= 613
    main = open(_lib.HEADER).read()
    assert re.search(r'^ \*   613  \+ ec_refractory_events', main, re.M), 'the history line of ABI 613'
    for step in ('1. parse, tick, counted', '2. class(i)', '3. chain', '4. output', 'not retriggerable', 'lowest row index',
                 'period_us + 1', 'quadratic', '4096', 'BOUND', '2 bands + 1'):
        assert step in text, f'the header states the definition step by step: {step!r} is missing'
    # the bindings against what the host compiler makes of the same text
    import shutil
    import subprocess
    cc = shutil.which(os.environ.get('CC', 'cc'))
    assert cc is not None, 'no host C compiler'
    body, expect = [], []
    for c_name, cls in (('ec_refractory_params', vis.EcRefractoryParams), ('ec_refractory_stats', vis.EcRefractoryStats)):
        body.append(f'printf("S {c_name} %zu\\n", sizeof({c_name}));')
        expect.append(f'S {c_name} {ctypes.sizeof(cls)}')
        for field, _ in cls._fields_:
            body.append(f'printf("F {field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name} *)0)->{field}));')
            expect.append(f'F {field} {getattr(cls, field).offset} {getattr(cls, field).size}')
    body.append('printf("E %d %d %d\\n", (int)EC_REFRACTORY_MAX_PERIOD_US, (int)EC_REFRACTORY_MAX_GROUPS, (int)EC_REFRACTORY_LONG_LIST);')
    expect.append(f'E {2 ** 30 - 1} 256 {vis.REFRACTORY_LONG_LIST}')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eventclip_refractory.h"\nint main(void) {\n'
                   + '\n'.join(body) + '\nreturn 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'prog')], check=True)
    assert subprocess.run([str(tmp_path / 'prog')], capture_output=True, text=True, check=True).stdout.splitlines() == expect
    assert [f for f, _ in vis.EcRefractoryStats._fields_] == list(vis.REFRACTORY_STATS_DTYPE.names) == list(rf.STATS_DTYPE.names)
    assert ctypes.sizeof(vis.EcRefractoryStats) == vis.REFRACTORY_STATS_DTYPE.itemsize == 12
    assert [f for f, _ in vis.EcRefractoryParams._fields_] == ['H', 'W', 'period_us', 'per_polarity', 'max_sample_events', 'total_events']
    assert vis.REFRACTORY_MAX_PERIOD_US == rf.TICK_MAX and 2 <= vis.REFRACTORY_LONG_LIST <= 4096
    for n in ('ec_refractory_events', 'ec_refractory_events_packed'):
        res, args = vis.REFRACTORY_SIGNATURES[n]
        assert res is ctypes.c_int and len(args) == 11
        assert args[3] is ctypes.POINTER(vis.EcRefractoryParams)
        assert args[7] is ctypes.c_void_p                                 # EC_DEVICE stats: an address
        assert args[9] is ctypes.c_size_t
    assert vis.REFRACTORY_SIGNATURES['ec_refractory_workspace_bytes'] == (ctypes.c_size_t, [ctypes.POINTER(vis.EcRefractoryParams), ctypes.c_int])
    assert vis.REFRACTORY_SIGNATURES['ec_refractory_bands'] == (ctypes.c_int, [ctypes.c_int] * 3)


def test_the_band_plan_the_workspace_query_and_the_host_side_refusals():
    """ec_refractory_workspace_bytes and ec_refractory_bands are host only.  The entry points check their arguments before
    they touch the device: every refusal comes back with its code and its message."""
    lib = _lib.lib()
    # 32 K LDS words less one, a word per class: W classes a row, 2 W per polarity; no halo
    for (shape, pp), bands in {((37, 53), 0): 1, ((37, 53), 1): 1, ((100, 120), 0): 1, ((100, 120), 1): 1, ((180, 240), 0): 2,
                               ((180, 240), 1): 3, ((480, 640), 0): 10, ((480, 640), 1): 20, ((1, 32767), 0): 1, ((5, 32767), 0): 5,
                               ((1, 32767), 1): 0, ((1, 32768), 0): 0, ((3, 16383), 1): 3, ((3, 16384), 1): 0, ((0, 8), 0): 0,
                               ((8, 0), 1): 0, ((8, 8), 2): 0, ((8, 8), -1): 0}.items():
        assert lib.ec_refractory_bands(shape[0], shape[1], pp) == bands, (shape, pp)
        if pp in (0, 1) and bands:
            assert rf.plan(shape, pp)[1] == bands == vis.refractory_bands(shape, pp)
    p = vis.refractory_params((180, 240), 5000, False, 1000)
    slot = 1000 * 8 + 1008                                               # the keys, and the keep bytes to 16
    assert vis.refractory_workspace_bytes(p, 1) == slot and vis.refractory_workspace_bytes(p, 7) == 7 * slot
    assert vis.refractory_workspace_bytes(p, 256) == vis.refractory_workspace_bytes(p, 100000) == 256 * slot
    assert vis.refractory_workspace_bytes(p, 0) == 0 and lib.ec_refractory_workspace_bytes(None, 4) == 0
    p.max_sample_events = 0
    assert vis.refractory_workspace_bytes(p, 4) == 0
    big = np.zeros(64, np.uint8)                                          # an aligned address; no refused call reads it
    addr = big.ctypes.data + (-big.ctypes.data) % 16

    def prm(shape=(8, 8), period_us=100, pp=0, cap=100):
        q = vis.refractory_params(shape, 100, False, 100)
        q.period_us, q.per_polarity, q.max_sample_events = period_us, pp, cap
        return q

    f, k = 'ec_refractory_events', 'ec_refractory_events_packed'
    INV, WS = _lib.EC_ERR_INVALID, _lib.EC_ERR_WORKSPACE
    for name, args, rc_want, msg in (
            (f, (None, addr, 1, prm(), addr + 16, addr, addr, 4096), INV, b'null buffer'),
            (f, (addr, None, 1, prm(), addr + 16, addr, addr, 4096), INV, b'null buffer'),
            (k, (addr, addr, 1, prm(), None, addr, addr, 4096), INV, b'null buffer'),
            (f, (addr, addr, 1, prm(), addr + 16, None, addr, 4096), INV, b'null buffer'),
            (f, (addr, addr, 1, prm(), addr + 16, addr, None, 4096), INV, b'null buffer'),
            (f, (addr, addr, 1, None, addr + 16, addr, addr, 4096), INV, b'params is null'),
            (f, (addr, addr, 1, prm(), addr, addr, addr, 4096), INV, b'in-place'),
            (f, (addr + 8, addr, 1, prm(), addr + 16, addr, addr, 4096), INV, b'16-byte aligned'),
            (k, (addr, addr, 1, prm(), addr + 20, addr, addr, 4096), INV, b'8-byte aligned'),
            (f, (addr, addr, 1, prm(), addr + 16, addr + 4, addr, 4096), INV, b'counts must be 8-byte'),
            (f, (addr, addr, 1, prm(), addr + 16, addr, addr + 8, 4096), INV, b'workspace 16-byte aligned'),
            (f, (addr, addr, 1, prm(period_us=0), addr + 16, addr, addr, 4096), INV, b'period_us=0 outside 1 .. 1073741823'),
            (k, (addr, addr, 1, prm(period_us=2 ** 30), addr + 16, addr, addr, 4096), INV, b'period_us=1073741824 outside'),
            (f, (addr, addr, 1, prm(pp=2), addr + 16, addr, addr, 4096), INV, b'per_polarity=2'),
            (f, (addr, addr, 1, prm(pp=-1), addr + 16, addr, addr, 4096), INV, b'per_polarity=-1'),
            (f, (addr, addr, 1, prm(cap=0), addr + 16, addr, addr, 4096), INV, b'max_sample_events=0'),
            (f, (addr, addr, 1, prm(cap=-5), addr + 16, addr, addr, 4096), INV, b'max_sample_events=-5'),
            (f, (addr, addr, 1, prm((0, 8)), addr + 16, addr, addr, 4096), INV, b'bad shape (0,8)'),
            (f, (addr, addr, 1, prm((3, 16384), pp=1), addr + 16, addr, addr, 4096), INV, b'W=16384 too wide'),
            (f, (addr, addr, 1, prm((1, 32768)), addr + 16, addr, addr, 4096), INV, b'W=32768 too wide'),
            (f, (addr, addr, -1, prm(), addr + 16, addr, addr, 4096), INV, b'B=-1'),
            (f, (addr, addr, 1, prm(), addr + 16, addr, addr, 911), WS, b'workspace 911 < 912 bytes'),
            (k, (addr, addr, 3, prm(), addr + 16, addr, addr, 2735), WS, b'workspace 2735 < 2736 bytes')):
        events, rng, B, pr, out, counts, ws, ws_bytes = args
        rc = getattr(lib, name)(events, rng, B, ctypes.byref(pr) if pr is not None else None, out, counts, None, None, ws, ws_bytes, None)
        assert rc == rc_want, msg
        assert msg in lib.ec_last_error(), (msg, lib.ec_last_error())
    assert lib.ec_refractory_events(None, None, 0, ctypes.byref(prm()), None, None, None, None, None, 0, None) == _lib.EC_OK   # B == 0
    # the Python layer says the same before any launch
    for us in (0, 2 ** 30):
        with pytest.raises(ValueError, match='period_us'):
            vis.refractory_params((8, 8), us, False, 10)
    assert vis.refractory_period_us(0.005) == 5000 and vis.refractory_period_us(1e-6) == 1
    for s in (0, -1e-3, 1100.):
        with pytest.raises(ValueError, match='refractory period'):
            vis.refractory_period_us(s)
    q = vis.refractory_params((100, 120), 5000, True, 70000, 11)
    assert (q.H, q.W, q.period_us, q.per_polarity, q.max_sample_events, q.total_events) == (100, 120, 5000, 1, 70000, 11)


def test_the_pipeline_reads_the_key():
    from eventclip_amd.event2img import Event2ImagePipeline
    qa = dict(max_imgs=4, N=300, split_method='event_count', convert_method='event_histogram', grayscale=True,
              count_non_zero=False, background_mask=True)
    assert Event2ImagePipeline((36, 52), 1200, qa).refractory is None and not Event2ImagePipeline((36, 52), 1200, qa).filters
    assert Event2ImagePipeline((36, 52), 1200, dict(qa, refractory=None)).refractory is None
    pipe = Event2ImagePipeline((36, 52), 1200, dict(qa, refractory=dict(period=0.002)))
    assert pipe.refractory == dict(period=0.002, per_polarity=False) and pipe.denoise is None and pipe.filters
    both = Event2ImagePipeline((36, 52), 1200, dict(qa, refractory=dict(period=0.01, per_polarity=True), denoise=dict(dt=0.002),
                                                    convert_method='time_surface'))
    assert both.refractory == dict(period=0.01, per_polarity=True) and both.denoise == dict(dt=0.002, radius=1)
    for bad in (dict(per_polarity=True), dict(period=0.), dict(period=-1.), dict(period=1100.), dict(period=0.002, polarity=True),
                dict(period=0.002, per_polarity=2), 0.002, (0.002,), 'on'):
        with pytest.raises(ValueError):
            Event2ImagePipeline((36, 52), 1200, dict(qa, refractory=bad))
    with pytest.raises(ValueError, match='row band'):
        Event2ImagePipeline((2, 40000), 1200, dict(qa, refractory=dict(period=0.002)))


def test_custom_op_is_registered_with_a_fake_kernel():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    assert 'events_refractory' in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, 'events_refractory')
    with FakeTensorMode():
        sr = torch.zeros(5, 2, dtype=torch.int64, device='cuda')
        for ev in (torch.empty(1000, 4, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')):
            out, counts = torch.ops.eventclip_hip.events_refractory(ev, sr, 180, 240, 5000, True)
            assert out.shape == ev.shape and out.dtype == ev.dtype
            assert counts.shape == (5,) and counts.dtype == torch.int64
    with pytest.raises(NotImplementedError):                             # no CPU kernel
        torch.ops.eventclip_hip.events_refractory(torch.zeros(4, 4), torch.zeros(1, 2, dtype=torch.int64), 8, 8, 100, False)
