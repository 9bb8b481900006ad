"""The yardstick of the background-activity filter checked against itself, and the filter's layers that need no GPU:
the two restatements of include/eventclip_denoise.h agree on every case, the result does not depend on the order of the
events, the check catches every planted fault of the kernel's model, float rows and packed events decide alike, the
bindings are the header's, the library exports the entries under ABI 611, the workspace query and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_ref as dn
from eventclip_amd import _lib, vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(dn.cases())
LOOP_MAX = 700          # samples up to this length go through the double loop whole, longer ones on a draw of rows


def oracle(name):
    c = dn.cases()[name]
    return dn.oracle(c['events'], c['ranges'], c['shape'], c['dt_us'], c['radius'])


def test_the_case_table_holds_what_it_promises():
    C = dn.cases()
    assert {c['shape'] for c in C.values()} == set(dn.SHAPES) and (37, 53) in dn.SHAPES          # an odd width
    for name, c in C.items():
        st = oracle(name)['stats']
        kept, removed = int(st['kept'].sum()), int(st['removed'].sum())
        if c['random']:
            assert max(e - b for b, e in c['ranges']) <= 20000
            assert 0.1 <= kept / (kept + removed) <= 0.9, (name, kept, removed)
        assert (st['kept'].astype(np.int64) + st['passed'] == oracle(name)['counts']).all()
    assert sorted(e - b for b, e in C['lengths']['ranges']) == [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4097]
    assert len(C['many']['ranges']) == 600
    assert C['gapped']['ranges'][0][0] > 0 and C['gapped']['ranges'][2][0] > C['gapped']['ranges'][1][1]
    t = C['rand_100_unsorted']['events'][:, 2]
    assert (np.diff(t) < 0).any()
    for shape in dn.SHAPES:                                              # every row boundary of every shape, r 1 and r 3
        for r in (1, 3):
            c = C[f'rows_{shape[0]}_r{r}']
            _, y, _, _, _ = dn.parse(c['events'], shape)
            lo, hi = np.minimum(y[0::2], y[1::2]), np.maximum(y[0::2], y[1::2])
            assert c['shape'] == shape and (hi - lo == r).all()
            assert all(((lo <= b) & (hi > b)).any() for b in range(shape[0] - 1))
    # no two adjacent pixels of any case hold more than 4096 events (the header's worst case)
    for name, c in C.items():
        x, y, _, counted, _ = dn.parse(c['events'], c['shape'])
        for b, e in c['ranges']:
            per = np.bincount((y[b:e] * c['shape'][1] + x[b:e])[counted[b:e]], minlength=1)
            assert np.sort(per)[-2:].sum() <= 4096, name


@pytest.mark.parametrize('name', CASES)
def test_the_two_restatements_agree(name):
    c = dn.cases()[name]
    want = oracle(name)
    rng = np.random.default_rng(1)
    rows = []
    for b, e in c['ranges']:
        rows += list(range(b, e)) if e - b <= LOOP_MAX else rng.choice(np.arange(b, e), 100, replace=False).tolist()
    if name == 'many':
        rows = [i for b, e in c['ranges'][::20] for i in range(b, e)]
    loop = dn.oracle_loop(c['events'], c['ranges'], c['shape'], c['dt_us'], c['radius'], rows=rows)
    _, _, _, counted, _ = dn.parse(c['events'], c['shape'])
    assert set(loop) == {i for i in rows if counted[i]}
    for i, sup in loop.items():
        assert want['keep'][i] == int(sup), (name, i)
    for i in rows:
        if not counted[i]:
            assert want['keep'][i] == 1                                  # passes
    if c['expect'] is not None:                                          # ... and with what the construction says
        np.testing.assert_array_equal(want['keep'], dn.expected_keep(c))


@pytest.mark.parametrize('name', ['rand_small_r2', 'rand_100_r1', 'hot', 'skip', 'bar_37_r1', 'lengths', 'frac'])
def test_a_shuffled_stream_gives_the_same_keep_set(name):
    c = dn.cases()[name]
    want = oracle(name)
    perm = np.arange(len(c['events']))
    rng = np.random.default_rng(7)
    for b, e in c['ranges']:
        perm[b:e] = b + rng.permutation(e - b)
    for f in (dn.oracle, dn.kernel_model):
        got = f(c['events'][perm], c['ranges'], c['shape'], c['dt_us'], c['radius'])
        np.testing.assert_array_equal(got['keep'], want['keep'][perm])
        np.testing.assert_array_equal(got['counts'], want['counts'])
        np.testing.assert_array_equal(got['stats'], want['stats'])


@pytest.mark.parametrize('name', CASES)
def test_the_model_of_the_kernel_computes_the_definition(name):
    c = dn.cases()[name]
    for rows in (5, 16, c['shape'][0]):
        if rows == 5 and (c['shape'][0] > 100 or name == 'many'):
            continue
        dn.check(dn.kernel_model(c['events'], c['ranges'], c['shape'], c['dt_us'], c['radius'], rows_per_band=rows), oracle(name))


# which cases show each fault
PLANTED = dict(own_pixel=('directed_37_r1', 'hot'), open_window=('directed_37_r2', 'dt0'), future=('directed_37_r1', 'rows_37_r1'),
               no_halo=('rows_37_r1', 'rows_480_r3'), uncounted_support=('directed_37_r3', 'skip'), x_wrap=('directed_37_r1', 'directed_480_r3'),
               manhattan=('directed_37_r2', 'rows_180_r3'), reorder=('rand_small_r1', 'lengths'))


@pytest.mark.parametrize('fault', dn.FAULTS)
def test_the_check_catches_a_planted_fault(fault):
    assert set(PLANTED) == set(dn.FAULTS)
    for name in PLANTED[fault]:
        c = dn.cases()[name]
        args = (c['events'], c['ranges'], c['shape'], c['dt_us'], c['radius'])
        dn.check(dn.kernel_model(*args, rows_per_band=16), oracle(name))
        with pytest.raises(AssertionError):
            dn.check(dn.kernel_model(*args, rows_per_band=16, fault=fault), oracle(name))
    if fault == 'reorder':                                               # a fault of the rows alone: the rest passes
        c = dn.cases()['rand_small_r1']
        got = dn.kernel_model(c['events'], c['ranges'], c['shape'], c['dt_us'], c['radius'], fault=fault)
        dn.check(dict(keep=got['keep'], counts=got['counts'], stats=got['stats']), oracle('rand_small_r1'))


def test_the_check_sees_every_output_and_every_guard():
    c = dn.cases()['gapped']
    want = oracle('gapped')
    for k, at in (('keep', 2), ('keep', c['ranges'][2][0] - 1), ('counts', 1), ('events_out', 0),
                  ('events_out', c['ranges'][0][0] + int(want['counts'][0]))):
        got = {n: v.copy() for n, v in want.items()}
        got[k].reshape(-1).view(np.uint8)[at * got[k][0].nbytes] ^= 1
        with pytest.raises(AssertionError, match=k):
            dn.check(got, want)
        dn.check({n: v for n, v in got.items() if n != k}, want)
    got = {n: v.copy() for n, v in want.items()}
    got['stats']['removed'][3] += 1
    with pytest.raises(AssertionError, match='stats'):
        dn.check(got, want)


@pytest.mark.parametrize('name', [n for n in CASES if dn.cases()[n]['packable']])
def test_float_rows_and_packed_events_decide_alike(name):
    c = dn.cases()[name]
    pk = dn.packed(c)
    w, wp = oracle(name), dn.oracle(pk, c['ranges'], c['shape'], c['dt_us'], c['radius'])
    for k in ('keep', 'counts', 'stats'):
        np.testing.assert_array_equal(w[k], wp[k])
    for (b, e), n in zip(c['ranges'], w['counts']):
        np.testing.assert_array_equal(wp['events_out'][b:b + n], vis.pack_events(w['events_out'][b:b + n]))
    assert wp['events_out'].dtype == np.uint64


# ---- the layers around the kernel ----
def test_header_declares_the_entries_and_the_library_exports_them(tmp_path):
    text = open(vis.DENOISE_HEADER).read()
    names = sorted(set(re.findall(r'EC_API\s+[\w\s\*]+?\b(ec_\w+)\s*\(', text)))
    assert names == ['ec_denoise_bands', 'ec_denoise_events', 'ec_denoise_events_packed', 'ec_denoise_workspace_bytes'] == sorted(vis.DENOISE_SIGNATURES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f'{n} declared in include/eventclip_denoise.h but not exported'
    assert _lib.lib().ec_version() == _lib.ABI_VERSION >= 611
    for step in ('1. parse', '2. tick', '3. counted(i)', '4. supported(i)', '5. output', 'quadratic', '4096', 'BOUND'):
        assert step in text, f'the header states the definition step by step: {step!r} is missing'
    # the bindings against what the host compiler makes of the same text
    import shutil
    import subprocess
    cc = shutil.which(os.environ.get('CC', 'cc'))
    assert cc is not None, 'no host C compiler'
    body, want = [], []
    for c_name, cls in (('ec_denoise_params', vis.EcDenoiseParams), ('ec_denoise_stats', vis.EcDenoiseStats)):
        body.append(f'printf("S {c_name} %zu\\n", sizeof({c_name}));')
        want.append(f'S {c_name} {ctypes.sizeof(cls)}')
        for field, _ in cls._fields_:
            body.append(f'printf("F {field} %zu %zu\\n", offsetof({c_name}, {field}), sizeof((({c_name} *)0)->{field}));')
            want.append(f'F {field} {getattr(cls, field).offset} {getattr(cls, field).size}')
    body.append('printf("E %d %d %d %d\\n", (int)EC_DENOISE_MIN_RADIUS, (int)EC_DENOISE_MAX_RADIUS, (int)EC_DENOISE_MAX_DT_US, (int)EC_DENOISE_MAX_GROUPS);')
    want.append(f'E 1 3 {2 ** 30 - 1} 256')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eventclip_denoise.h"\nint main(void) {\n'
                   + '\n'.join(body) + '\nreturn 0; }\n')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'prog')], check=True)
    assert subprocess.run([str(tmp_path / 'prog')], capture_output=True, text=True, check=True).stdout.splitlines() == want
    assert [f for f, _ in vis.EcDenoiseStats._fields_] == list(vis.DENOISE_STATS_DTYPE.names) == list(dn.STATS_DTYPE.names)
    assert ctypes.sizeof(vis.EcDenoiseStats) == vis.DENOISE_STATS_DTYPE.itemsize == dn.STATS_DTYPE.itemsize == 12
    assert [f for f, _ in vis.EcDenoiseParams._fields_] == ['H', 'W', 'radius', 'dt_us', 'max_sample_events', 'total_events']
    assert (vis.DENOISE_RADIUS, vis.DENOISE_MAX_DT_US) == ((1, 3), dn.TICK_MAX)
    for n in ('ec_denoise_events', 'ec_denoise_events_packed'):
        res, args = vis.DENOISE_SIGNATURES[n]
        assert res is ctypes.c_int and len(args) == 11
        assert args[3] is ctypes.POINTER(vis.EcDenoiseParams)
        assert args[7] is ctypes.c_void_p                                 # EC_DEVICE stats: an address
        assert args[9] is ctypes.c_size_t
    assert vis.DENOISE_SIGNATURES['ec_denoise_workspace_bytes'] == (ctypes.c_size_t, [ctypes.POINTER(vis.EcDenoiseParams), ctypes.c_int])


def test_the_workspace_query_the_bands_and_the_host_side_refusals():
    """ec_denoise_workspace_bytes and ec_denoise_bands are host only.  The entry points check their arguments before they
    touch the device: every refusal comes back with its code and its message."""
    lib = _lib.lib()
    # 32 K LDS words less one: a sensor that fits has one band and no halo, a larger one bands of rows - 2 r
    for (shape, r), bands in {((37, 53), 1): 1, ((100, 120), 3): 1, ((180, 240), 1): 2, ((180, 240), 3): 2, ((480, 640), 1): 10,
                              ((480, 640), 3): 11, ((1, 32767), 1): 1, ((2, 32767), 1): 0, ((3, 16383), 1): 0, ((8, 8), 0): 0, ((8, 8), 4): 0,
                              ((0, 8), 1): 0, ((1, 32768), 1): 0}.items():
        assert lib.ec_denoise_bands(shape[0], shape[1], r) == bands, (shape, r)
    p = vis.denoise_params((180, 240), 5000, 1, 1000)
    slot = 1000 * 4 + 1008                                               # the ticks, and the keep bytes to 16
    assert vis.denoise_workspace_bytes(p, 1) == slot and vis.denoise_workspace_bytes(p, 7) == 7 * slot
    assert vis.denoise_workspace_bytes(p, 256) == vis.denoise_workspace_bytes(p, 100000) == 256 * slot
    assert vis.denoise_workspace_bytes(p, 0) == 0 and lib.ec_denoise_workspace_bytes(None, 4) == 0
    p.max_sample_events = 0
    assert vis.denoise_workspace_bytes(p, 4) == 0
    big = np.zeros(64, np.uint8)                                          # an aligned address; no refused call reads it
    addr = big.ctypes.data + (-big.ctypes.data) % 16

    def prm(shape=(8, 8), radius=1, dt_us=100, cap=100):
        q = vis.denoise_params(shape, 100, 1, 100)
        q.radius, q.dt_us, q.max_sample_events = radius, dt_us, cap
        return q

    f, k = 'ec_denoise_events', 'ec_denoise_events_packed'
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
            (f, (addr, addr, 1, prm(radius=0), addr + 16, addr, addr, 4096), INV, b'radius=0 outside 1 .. 3'),
            (k, (addr, addr, 1, prm(radius=4), addr + 16, addr, addr, 4096), INV, b'radius=4 outside 1 .. 3'),
            (f, (addr, addr, 1, prm(dt_us=2 ** 30), addr + 16, addr, addr, 4096), INV, b'dt_us=1073741824 above 1073741823'),
            (f, (addr, addr, 1, prm(cap=0), addr + 16, addr, addr, 4096), INV, b'max_sample_events=0'),
            (f, (addr, addr, 1, prm(cap=-5), addr + 16, addr, addr, 4096), INV, b'max_sample_events=-5'),
            (f, (addr, addr, 1, prm((3, 16383)), addr + 16, addr, addr, 4096), INV, b'W=16383 too wide'),
            (f, (addr, addr, -1, prm(), addr + 16, addr, addr, 4096), INV, b'B=-1'),
            (f, (addr, addr, 1, prm(), addr + 16, addr, addr, 511), WS, b'workspace 511 < 512 bytes'),
            (k, (addr, addr, 3, prm(), addr + 16, addr, addr, 1535), WS, b'workspace 1535 < 1536 bytes')):
        events, rng, B, pr, out, counts, ws, ws_bytes = args
        rc = getattr(lib, name)(events, rng, B, ctypes.byref(pr) if pr is not None else None, out, counts, None, None, ws, ws_bytes, None)
        assert rc == rc_want, msg
        assert msg in lib.ec_last_error(), (msg, lib.ec_last_error())
    assert lib.ec_denoise_events(None, None, 0, ctypes.byref(prm()), None, None, None, None, None, 0, None) == _lib.EC_OK   # B == 0
    # the Python layer says the same before any launch
    for r in (0, 4):
        with pytest.raises(ValueError, match='radius'):
            vis.denoise_params((8, 8), 100, r, 10)
    with pytest.raises(ValueError, match='dt'):
        vis.denoise_params((8, 8), 2 ** 30, 1, 10)
    assert vis.denoise_dt_us(0.005) == 5000 and vis.denoise_dt_us(0) == 0
    for dt in (-1e-3, 1100.):
        with pytest.raises(ValueError, match='support window'):
            vis.denoise_dt_us(dt)
    q = vis.denoise_params((100, 120), 5000, 3, 70000, 11)
    assert (q.H, q.W, q.radius, q.dt_us, q.max_sample_events, q.total_events) == (100, 120, 3, 5000, 70000, 11)


def test_the_pipeline_reads_the_key_and_plans_on_filtered_counts_with_unchanged_starts():
    from eventclip_amd.event2img import Event2ImagePipeline
    qa = dict(max_imgs=4, N=300, split_method='event_count', convert_method='event_histogram', grayscale=True,
              count_non_zero=False, background_mask=True)
    assert Event2ImagePipeline((36, 52), 1200, qa).denoise is None
    assert Event2ImagePipeline((36, 52), 1200, dict(qa, denoise=None)).denoise is None
    pipe = Event2ImagePipeline((36, 52), 1200, dict(qa, denoise=dict(dt=0.002)))
    assert pipe.denoise == dict(dt=0.002, radius=1) and pipe.max_n == 1200
    assert Event2ImagePipeline((36, 52), 1200, dict(qa, denoise=dict(dt=0.002, radius=3), convert_method='voxel_grid')).denoise['radius'] == 3
    for bad in (dict(radius=1), dict(dt=0.002, radius=4), dict(dt=-1.), dict(dt=0.002, r=1), 0.002):
        with pytest.raises(ValueError):
            Event2ImagePipeline((36, 52), 1200, dict(qa, denoise=bad))
    # the filter compacts every sample at its own first row: plan() takes the filtered counts with those starts
    n, kept = [1100, 250, 701], [640, 3, 350]
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    fr, ri, vm = pipe.plan(kept, starts=starts)
    assert fr.tolist() == [[0, 300], [300, 600], [1100, 1103], [1350, 1650]]        # 640: two chunks, no overlapping third
    assert ri.tolist() == [[0, 1, -1, -1], [2, -1, -1, -1], [3, -1, -1, -1]] and vm.sum() == 4
    fr, _, _ = pipe.plan(kept, tflip=True, starts=starts)
    assert fr.tolist() == [[340, 640], [40, 340], [1100, 1103], [1400, 1700]]
    fr, _, _ = pipe.plan(kept, starts=[10, 2000, 5000])                              # a caller's own starts
    assert fr[:, 0].tolist() == [10, 310, 2000, 5000]


def test_custom_op_is_registered_with_a_fake_kernel():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from eventclip_amd import torch_ops
    assert 'events_denoise' in torch_ops.OPS and hasattr(torch.ops.eventclip_hip, 'events_denoise')
    with FakeTensorMode():
        sr = torch.zeros(5, 2, dtype=torch.int64, device='cuda')
        for ev in (torch.empty(1000, 4, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')):
            out, counts = torch.ops.eventclip_hip.events_denoise(ev, sr, 180, 240, 5000, 1)
            assert out.shape == ev.shape and out.dtype == ev.dtype
            assert counts.shape == (5,) and counts.dtype == torch.int64
    with pytest.raises(NotImplementedError):                             # no CPU kernel
        torch.ops.eventclip_hip.events_denoise(torch.zeros(4, 4), torch.zeros(1, 2, dtype=torch.int64), 8, 8, 100, 1)
