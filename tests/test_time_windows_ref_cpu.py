"""The fixed-duration windows without a device: the two restatements of include/eventclip_time_windows.h agree on every
case, the bindings are the header's, the library exports the entries under ABI 612, every refusal comes back from the host
side, the pipeline validates its keys, 'time' is still no split method, and the custom op has its fake kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

import time_windows_ref as tw
from eventclip_amd import _lib, vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QA = dict(max_imgs=4, N=300, split_method='time_window', convert_method='time_surface', window=0.03, grayscale=True,
          count_non_zero=False, background_mask=True)


@pytest.mark.parametrize('name', sorted(tw.cases()))
def test_counting_and_searching_state_the_same_windows(name):
    c = tw.cases()[name]
    for from_last in (0, 1):
        a = tw.oracle(c['ticks'], c['ranges'], c['dt_us'], c['stride_us'], c['max_windows'], from_last)
        b = tw.oracle(c['ticks'], c['ranges'], c['dt_us'], c['stride_us'], c['max_windows'], from_last, tw.sample_by_search)
        np.testing.assert_array_equal(a['bounds'], b['bounds'])
        np.testing.assert_array_equal(a['stats'], b['stats'])
        tw.check(a, b, c['ranges'])
    assert (tw.ticks_of(tw.packed_events(c['ticks'])) == c['ticks']).all()
    if c['floatable']:
        assert (tw.ticks_of(tw.float_events(c['ticks'])) == c['ticks']).all()


def test_the_definition_on_a_case_worked_by_hand():
    """ticks 0 0 999 1000 1000 1001 1999 2000 2999 3000, windows of 1000 us back to back.  From the first event: [0, 1000)
    holds rows 0 .. 2, the event on 1000 opens the next window.  From the last (3000): d = 3000 .. 0, window 0 is d in
    [0, 1000), ticks 2001 .. 3000; the event on 2000 (d = 1000) opens window 1, and so does 1001 (d = 1999)."""
    c = tw.cases()['on_edges']
    fwd = tw.oracle(c['ticks'], c['ranges'], 1000, 1000, 8, 0)
    assert fwd['stats'][0].tolist() == (0, 3000, 0, 4)
    assert fwd['bounds'][0, :4].tolist() == [[0, 3], [3, 7], [7, 9], [9, 10]] and (fwd['bounds'][0, 4:] == tw.PREFILL).all()
    back = tw.oracle(c['ticks'], c['ranges'], 1000, 1000, 8, 1)
    assert back['bounds'][0, :4].tolist() == [[8, 10], [5, 8], [2, 5], [0, 2]]
    # stride > window: the events between two windows are in none; stride < window: in several
    gt = tw.oracle(c['ticks'], c['ranges'], 500, 1500, 8, 0)
    assert gt['stats']['windows'][0] == 3 and gt['bounds'][0, :3].tolist() == [[0, 2], [6, 7], [9, 10]]
    lt = tw.oracle(c['ticks'], c['ranges'], 1000, 500, 2, 0)
    assert lt['stats']['windows'][0] == 7 and lt['bounds'][0].tolist() == [[0, 3], [2, 6]]       # the full count above max_windows
    # an unsorted sample: the descents are counted and there are no windows
    un = tw.oracle(np.array([5, 4, 4, 3, 9]), [(0, 5)], 10, 10, 4, 0)
    assert un['stats'][0].tolist() == (5, 9, 2, -1) and (un['bounds'] == tw.PREFILL).all()
    with pytest.raises(AssertionError, match='bounds of sample 0'):
        bad = dict(fwd, bounds=fwd['bounds'].copy())
        bad['bounds'][0, 5, 1] = 0
        tw.check(bad, fwd, c['ranges'])


def test_header_declares_the_entries_and_the_library_exports_them(tmp_path):
    text = open(vis.TIME_WINDOWS_HEADER).read()
    names = sorted(set(re.findall(r'EC_API\s+[\w\s\*]+?\b(ec_\w+)\s*\(', text)))
    assert names == ['ec_time_windows', 'ec_time_windows_packed'] == sorted(vis.TIME_WINDOWS_SIGNATURES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f'{n} declared in include/eventclip_time_windows.h but not exported'
    assert _lib.lib().ec_version() == _lib.ABI_VERSION >= 612
    main = open(_lib.HEADER).read()
    assert '612  + ec_time_windows' in main and 'ec_time_windows(' not in main       # the main header: the history line alone
    for step in ('1. tick', '2. order', '3. span', '4. window k, from_last == 0', '5. window k, from_last != 0', '6. output',
                 '7. arithmetic', 'exactly once', 'No workspace'):
        assert step in text, f'the header states the definition step by step: {step!r} is missing'
    import shutil
    import subprocess
    cc = shutil.which(os.environ.get('CC', 'cc'))
    assert cc is not None, 'no host C compiler'
    body, want = [], []
    for c_name, cls in (('ec_time_windows_params', vis.EcTimeWindowsParams), ('ec_time_windows_stats', vis.EcTimeWindowsStats)):
        body.append(f'printf("S {c_name} %zu\\n", sizeof({c_name}));')
        want.append(f'S {c_name} {ctypes.sizeof(cls)}')
        for field, _ in cls._fields_:
            body.append(f'printf("F {field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name} *)0)->{field}));')
            want.append(f'F {field} {getattr(cls, field).offset} {getattr(cls, field).size}')
    body.append('printf("E %d %d %d\\n", (int)EC_TIME_WINDOWS_MAX_US, (int)EC_TIME_WINDOWS_SLICE_ROWS, (int)EC_TIME_WINDOWS_UNROLL);')
    want.append(f'E {2 ** 30 - 1} {vis.TIME_WINDOWS_SLICE_ROWS} {vis.TIME_WINDOWS_UNROLL}')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eventclip_time_windows.h"\nint main(void) {\n'
                   + '\n'.join(body) + '\nreturn 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'prog')], check=True)
    assert subprocess.run([str(tmp_path / 'prog')], capture_output=True, text=True, check=True).stdout.splitlines() == want
    assert [f for f, _ in vis.EcTimeWindowsStats._fields_] == list(vis.TIME_WINDOWS_STATS_DTYPE.names) == list(tw.STATS_DTYPE.names)
    assert ctypes.sizeof(vis.EcTimeWindowsStats) == vis.TIME_WINDOWS_STATS_DTYPE.itemsize == tw.STATS_DTYPE.itemsize == 16
    assert vis.TIME_WINDOWS_STATS_DTYPE == tw.STATS_DTYPE
    assert [f for f, _ in vis.EcTimeWindowsParams._fields_] == ['dt_us', 'stride_us', 'max_windows', 'from_last', 'total_events']
    assert ctypes.sizeof(vis.EcTimeWindowsParams) == 24
    assert (vis.TIME_WINDOWS_MAX_US, vis.TIME_WINDOWS_SLICE_ROWS, vis.TIME_WINDOWS_UNROLL) == (tw.TICK_MAX, tw.SLICE, tw.UNROLL)
    assert tw.SLICE % (64 * tw.UNROLL) == 0                              # a slice is UNROLL rounds of whole waves
    for n in names:
        res, args = vis.TIME_WINDOWS_SIGNATURES[n]
        assert res is ctypes.c_int and len(args) == 7
        assert args[2] is ctypes.c_int and args[3] is ctypes.POINTER(vis.EcTimeWindowsParams)
        assert args[5] is ctypes.c_void_p                                 # EC_DEVICE stats: an address


def test_the_host_side_refusals_and_the_empty_batch():
    """The entry points check their arguments before they touch the device: every refusal comes back with its code and its
    message, and writes nothing (the buffers are host memory no refused call may look at)."""
    lib = _lib.lib()
    big = np.full(64, 0x5A, np.uint8)
    addr = big.ctypes.data + (-big.ctypes.data) % 16

    def prm(dt_us=1000, stride_us=1000, max_windows=8):
        q = vis.time_windows_params(1000, 1000, 8)
        q.dt_us, q.stride_us, q.max_windows = dt_us, stride_us, max_windows
        return q

    f, k = 'ec_time_windows', 'ec_time_windows_packed'
    INV = _lib.EC_ERR_INVALID
    for name, args, msg in (
            (f, (None, addr, 1, prm(), addr, addr), b'null buffer'),
            (k, (addr, None, 1, prm(), addr, addr), b'null buffer'),
            (f, (addr, addr, 1, prm(), None, addr), b'null buffer'),
            (k, (addr, addr, 1, prm(), addr, None), b'null buffer'),
            (f, (addr, addr, 1, None, addr, addr), b'params is null'),
            (f, (addr + 8, addr, 1, prm(), addr, addr), b'ec_time_windows: events must be 16-byte aligned'),
            (k, (addr + 4, addr, 1, prm(), addr, addr), b'ec_time_windows_packed: events must be 8-byte aligned'),
            (f, (addr, addr + 4, 1, prm(), addr, addr), b'sample_range and bounds must be 8-byte'),
            (f, (addr, addr, 1, prm(), addr + 4, addr), b'sample_range and bounds must be 8-byte'),
            (f, (addr, addr, 1, prm(), addr, addr + 2), b'stats 4-byte aligned'),
            (f, (addr, addr, 1, prm(dt_us=0), addr, addr), b'dt_us=0 outside 1 .. 1073741823'),
            (k, (addr, addr, 1, prm(dt_us=2 ** 30), addr, addr), b'dt_us=1073741824 outside 1 .. 1073741823'),
            (f, (addr, addr, 1, prm(stride_us=0), addr, addr), b'stride_us=0 outside 1 .. 1073741823'),
            (f, (addr, addr, 1, prm(stride_us=2 ** 31), addr, addr), b'stride_us=2147483648 outside'),
            (f, (addr, addr, 1, prm(max_windows=0), addr, addr), b'max_windows=0'),
            (k, (addr, addr, 1, prm(max_windows=-3), addr, addr), b'max_windows=-3'),
            (f, (addr, addr, -1, prm(), addr, addr), b'B=-1')):
        events, rng, B, pr, bounds, stats = args
        rc = getattr(lib, name)(events, rng, B, ctypes.byref(pr) if pr is not None else None, bounds, stats, None)
        assert rc == INV, msg
        assert msg in lib.ec_last_error(), (msg, lib.ec_last_error())
    assert (big == 0x5A).all()
    for name in (f, k):                                                   # B == 0: fine, and nothing is looked at
        assert getattr(lib, name)(None, None, 0, ctypes.byref(prm()), None, None, None) == _lib.EC_OK
    # the Python layer says the same before any launch
    for bad in (dict(dt_us=0), dict(dt_us=2 ** 30), dict(stride_us=0), dict(stride_us=2 ** 30), dict(max_windows=0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            vis.time_windows_params(**dict(dict(dt_us=5, stride_us=5, max_windows=5), **bad))
    assert vis.time_window_us(0.03) == 30000 and vis.time_window_us(1e-6) == 1 and vis.time_window_us(1073.741823) == 2 ** 30 - 1
    for s in (0, -0.01, 4e-7, 1073.75):
        with pytest.raises(ValueError, match='microseconds'):
            vis.time_window_us(s)
    q = vis.time_windows_params(30000, 10000, 64, True, 777)
    assert (q.dt_us, q.stride_us, q.max_windows, q.from_last, q.total_events) == (30000, 10000, 64, 1, 777)


def test_the_pipeline_reads_and_validates_its_keys():
    from eventclip_amd.event2img import Event2ImagePipeline
    pipe = Event2ImagePipeline((36, 52), 1200, QA)
    assert (pipe.window, pipe.stride, pipe.min_events, pipe.max_windows, pipe.max_imgs, pipe.N) == (0.03, 0.03, 1, 64, 4, None)
    pipe = Event2ImagePipeline((36, 52), 1200, dict(QA, stride=0.01, min_events=5, max_windows=9, max_imgs=30))
    assert (pipe.stride, pipe.min_events, pipe.max_windows, pipe.max_imgs) == (0.01, 5, 9, 30)      # T = max_imgs itself
    no_n = {k: v for k, v in QA.items() if k not in ('N', 'max_imgs')}
    assert Event2ImagePipeline((36, 52), 1200, no_n).max_imgs == 10                                   # N is not read
    for cm in vis.CONVERT_METHODS:
        assert Event2ImagePipeline((36, 52), 1200, dict(QA, convert_method=cm, denoise=dict(dt=0.002))).split_method == 'time_window'
    for bad in (dict(window=0), dict(window=-1.), dict(window=2000.), dict(stride=0), dict(stride=1e4), dict(min_events=0),
                dict(max_windows=0)):
        with pytest.raises(ValueError):
            Event2ImagePipeline((36, 52), 1200, dict(QA, **bad))
    with pytest.raises(ValueError, match='window'):
        Event2ImagePipeline((36, 52), 1200, {k: v for k, v in QA.items() if k != 'window'})
    # the event_count pipeline is what it was
    ec = Event2ImagePipeline((36, 52), 1200, dict(QA, split_method='event_count'))
    assert (ec.N, ec.max_imgs) == (300, 4) and not hasattr(ec, 'window')
    fr, ri, vm = ec.plan([1100, 250])
    assert fr.tolist() == [[0, 300], [300, 600], [600, 900], [800, 1100], [1100, 1350]]


def test_time_and_every_other_unknown_split_method_are_still_refused():
    from eventclip_amd.event2img import Event2ImagePipeline
    assert vis.SPLIT_METHODS == ('event_count', 'time_window')
    ev = tw.float_events(np.arange(10) * 100)
    for name in ('time', 'time_windows', 'window', ''):
        with pytest.raises(AssertionError):
            Event2ImagePipeline((36, 52), 1200, dict(QA, split_method=name))
        with pytest.raises(AssertionError):
            vis.events2frames(ev, name, 'event_histogram', (36, 52), N=5, window=0.001)


def test_custom_op_is_registered_with_a_fake_kernel():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    assert 'events_time_windows' in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, 'events_time_windows')
    assert 'events_time_windows' in torch_ops.__doc__ and 'ec_time_windows[_packed]' in torch_ops.__doc__
    with FakeTensorMode():
        sr = torch.zeros(5, 2, dtype=torch.int64, device='cuda')
        for ev in (torch.empty(1000, 4, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')):
            bounds, stats = torch.ops.eventclip_hip.events_time_windows(ev, sr, 30000, 10000, 48, False, 1000)
            assert bounds.shape == (5, 48, 2) and bounds.dtype == torch.int64 and bounds.device.type == 'cuda'
            assert stats.shape == (5, 4) and stats.dtype == torch.int32
    with pytest.raises(NotImplementedError):                             # no CPU kernel
        torch.ops.eventclip_hip.events_time_windows(torch.zeros(4, 4), torch.zeros(1, 2, dtype=torch.int64), 5, 5, 4, False, 0)
