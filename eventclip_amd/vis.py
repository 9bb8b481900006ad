"""events -> 2-D frames on the MI355X; host-side mirror of the reference's datasets/vis.py.

Same names and argument meaning as the reference:

* ``events2frames(events, split_method, convert_method, shape, **kwargs)``
  (vis.py:75-117) -- numpy in, numpy uint8 [F, H, W, 3] out, computed by the HIP
  kernel behind ``ec_events_to_frames``.
* ``split_event_count(t, N)`` (vis.py:55-72), ``parse_events`` (vis.py:44-52).

plus the batched device entries ``events_to_frames_device`` (polarity histogram), ``time_surface_device``
(latest-timestamp frames, ``convert_method='time_surface'``: not in the reference, defined in
include/eventclip_time_surface.h) and ``voxel_grid_device`` (temporal-bin frames, ``convert_method='voxel_grid'``:
not in the reference either, defined in include/eventclip_voxel_grid.h) used by the pipeline, and in front of all three
``denoise_events_device`` / ``denoise_events`` (the background-activity filter of include/eventclip_denoise.h) and
``refractory_events_device`` / ``refractory_events`` (the refractory-period filter of include/eventclip_refractory.h).
``split_method='time_window'`` (not in the reference either) cuts a stream into windows of fixed duration instead of
fixed event count: ``time_windows_device`` / ``split_time_window`` (include/eventclip_time_windows.h).
There is no CPU fallback.
"""
import collections
import ctypes
import os

import numpy as np

from . import _lib


# Which numpy the float stage of make_event_histogram (vis.py:27-39) agrees with when the caller does not say.
# The reference pins numpy 1.25.2 (/root/reference/environment.yml:49), whose value-based casting keeps
# `hist.astype(np.float32) / hist.max()` -- and everything after it -- in float32; under numpy >= 2 (NEP 50, this
# image) the same line promotes to float64.  The two differ by 1 LSB at exact .5 ties only.  Default: the pinned
# reference environment; quantize_args['float_stage'] = 'float64' gives what this image's numpy makes of the
# reference (both are pinned by every events fixture).
DEFAULT_FLOAT_STAGE = 'float32'


def parse_events(events):
    """vis.py:44-52: accept an [n, 4] (x, y, t, p) array or a dict of columns.
    Returns one contiguous float32 [n, 4] array (the integer truncation of
    x, y, p happens in the kernel)."""
    if isinstance(events, dict):
        cols = [np.asarray(events[k]) for k in ('x', 'y', 't', 'p')]
        events = np.stack(cols, axis=1)
    ev = np.ascontiguousarray(events, dtype=np.float32)
    if ev.ndim != 2 or ev.shape[1] != 4:
        raise ValueError(f'events must be [n, 4] (x, y, t, p), got {ev.shape}')
    return ev


def chunk_bounds(tot_cnt, N):
    """Chunk index pairs of vis.py:55-72 from the event count alone."""
    tot_cnt, N = int(tot_cnt), int(N)
    if tot_cnt < N:                       # vis.py:60-61
        return [0], [tot_cnt]
    idx = list(range(0, tot_cnt, N))      # vis.py:64
    idx1, idx0 = idx[1:], idx[:-1]        # vis.py:65
    if tot_cnt - idx[-1] > N * 0.5:       # vis.py:67-69: overlapping last chunk
        idx0.append(tot_cnt - N)
        idx1.append(tot_cnt)
    return idx0, idx1


def split_event_count(t, N=30000):
    """Same return as the reference: (idx0, idx1, t0, t1)."""
    t = np.asarray(t)
    idx0, idx1 = chunk_bounds(len(t), N)
    if len(t) < N:
        return idx0, idx1, [t[0]], [t[-1]]
    return idx0, idx1, t[idx0], t[np.array(idx1) - 1]


def colour_map(grayscale=True):
    """vis.py:95-104 -> (red, blue) uint8[3]."""
    if grayscale:
        v = 127 if isinstance(grayscale, bool) else np.array(grayscale)
        red = np.round(np.ones(3) * v).astype(np.uint8)
        blue = np.round(np.ones(3) * v).astype(np.uint8)
    else:
        red = np.array([255, 0, 0], dtype=np.uint8)
        blue = np.array([0, 0, 255], dtype=np.uint8)
    return red, blue


def make_params(shape, grayscale=True, thresh=10., count_non_zero=False, background_mask=True,
                max_frame_events=0, flip_x=False, negate_p=False, float_stage=DEFAULT_FLOAT_STAGE,
                total_events=0):
    red, blue = colour_map(grayscale)
    return events_params(shape, red, blue, thresh, count_non_zero, background_mask, max_frame_events, flip_x, negate_p,
                         _float32_stage(float_stage), total_events)


def _float32_stage(float_stage):
    if float_stage not in ('float64', 'float32'):
        raise ValueError(f'float_stage {float_stage!r}: float64 (numpy >= 2) or float32 (numpy 1.x)')
    return float_stage == 'float32'


def events_params(shape, red, blue, thresh, count_non_zero, background_mask, max_frame_events, flip_x, negate_p,
                  float32_stage, total_events):
    """EcEventsParams with the (red, blue) colours given: what ``make_params`` and the custom op both fill."""
    p = _lib.EcEventsParams()
    p.H, p.W = int(shape[0]), int(shape[1])
    p.thresh = float(thresh)
    p.count_non_zero = int(bool(count_non_zero))
    p.background_mask = int(bool(background_mask))
    p.max_frame_events = int(max_frame_events)
    p.flip_x, p.negate_p = int(bool(flip_x)), int(bool(negate_p))
    p.float32_stage = int(bool(float32_stage))
    p.total_events = int(total_events)
    for c in range(3):
        p.red[c] = int(red[c])
        p.blue[c] = int(blue[c])
    return p


_sort_scratch = collections.defaultdict(_lib.Scratch)   # device index -> the sort workspace, reused by every call


def attach_sort_workspace(prm, device, enable=True):
    """Long frames (N-ImageNet: 70 000 events on 480 x 640) are bucketed by row band in a device
    scratch instead of being re-read for every band pass; the library says how much pays off."""
    import torch
    need = int(_lib.lib().ec_events_sort_workspace_bytes(ctypes.byref(prm))) if enable else 0
    if need <= 0:
        return None
    key = device.index if device.index is not None else torch.cuda.current_device()
    ws = _sort_scratch[key].get(need, device)
    prm.sort_workspace, prm.sort_workspace_bytes = ws.data_ptr(), ws.numel()
    return ws


# ---- packed 8-byte events (include/eventclip_hip.h: x | y << 16 | code << 32 | t_us << 34) ----
PACKED_T_MAX = (1 << 30) - 1


def is_packed(events):
    """Packed events travel as 1-D int64 (torch) / uint64 or int64 (numpy) arrays."""
    return events.ndim == 1 and str(events.dtype).split('.')[-1] in ('int64', 'uint64')


def pack_events(events):
    """Host packer: float [n, 4] (x, y, t [s], p) -> uint64 [n].  Same bits as ec_pack_events.
    Raises when a coordinate is not an integer in [0, 65535] (the float path flips x before it
    truncates, datasets/utils.py:22, so such events have no packed equivalent)."""
    ev = np.asarray(events)
    if ev.dtype.names:   # structured (x, y, t, p) record array
        ev = np.stack([ev['x'], ev['y'], ev['t'], ev['p']], 1)
    ev = ev.astype(np.float32, copy=False)
    x, y = ev[:, 0].astype(np.int32), ev[:, 1].astype(np.int32)     # vis.py:50
    if not ((x == ev[:, 0]) & (y == ev[:, 1]) & (x >= 0) & (y >= 0) & (x < 65536) & (y < 65536)).all():
        raise ValueError('pack_events: coordinates must be integers in [0, 65535]')
    p = ev[:, 3].astype(np.int32)
    code = np.where(p == 0, 0, np.where(p > 0, 1, 2)).astype(np.uint64)
    t_us = np.clip(np.rint(ev[:, 2].astype(np.float64) * 1e6), 0, PACKED_T_MAX).astype(np.uint64)
    return (x.astype(np.uint64) | (y.astype(np.uint64) << np.uint64(16)) | (code << np.uint64(32)) |
            (t_us << np.uint64(34)))


def pack_structured(x, y, t_us, p):
    """Packed events straight from integer fields (N-ImageNet's event_data, imagenet.py:8-27:
    t already in microseconds, polarity 0/1 where 0 means negative unless negatives are present)."""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    if x.size and (x.min() < 0 or y.min() < 0 or x.max() > 65535 or y.max() > 65535):
        raise ValueError('pack_structured: coordinates must lie in [0, 65535]')
    p = np.asarray(p).astype(np.uint8).astype(np.float64)   # imagenet.py:15 (uint8 cast first)
    if p.size and p.min() >= -0.5:                         # imagenet.py:24-25
        p = np.where(p <= 0.5, -1., p)
    code = np.where(p == 0, 0, np.where(p > 0, 1, 2)).astype(np.uint64)
    t = np.clip(np.asarray(t_us).astype(np.int64), 0, PACKED_T_MAX).astype(np.uint64)
    return (x.astype(np.uint64) | (y.astype(np.uint64) << np.uint64(16)) | (code << np.uint64(32)) |
            (t << np.uint64(34)))


def unpack_events(packed):
    """uint64 [n] -> float32 [n, 4] (x, y, t [s], p in {-1, 0, +1})."""
    e = np.asarray(packed).astype(np.uint64)
    code = (e >> np.uint64(32)) & np.uint64(3)
    p = np.where(code == 0, 0., np.where(code == 1, 1., -1.))
    return np.stack([(e & np.uint64(0xffff)).astype(np.float64),
                     ((e >> np.uint64(16)) & np.uint64(0xffff)).astype(np.float64),
                     (e >> np.uint64(34)).astype(np.float64) / 1e6, p], 1).astype(np.float32)


def pack_events_device(events, return_bad=False):
    """float32 CUDA [n, 4] -> packed int64 CUDA [n] (ec_pack_events)."""
    import torch
    dev = _lib.require_gpu()
    assert events.is_cuda and events.dtype == torch.float32 and events.is_contiguous()
    n = int(events.shape[0])
    out = torch.empty((n,), dtype=torch.int64, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.launch('ec_pack_events', events, n, out, bad)
    return (out, int(bad.item())) if return_bad else out


def _check_device_events(events, ranges, on_device=True):
    """What every device entry asks of (events, frame_range / sample_range) -> (the device, whether events are packed).
    on_device=False: the ranges may live on the host (the filter moves them itself)."""
    import torch
    dev = _lib.require_gpu()
    packed = is_packed(events)
    assert events.is_cuda and events.is_contiguous()
    assert packed or (events.dtype == torch.float32 and events.dim() == 2 and events.shape[1] == 4)
    if on_device:
        assert ranges.is_cuda and ranges.dtype == torch.int64 and ranges.is_contiguous()
    else:
        assert ranges.dtype == torch.int64 and ranges.dim() == 2 and ranges.shape[1] == 2
    return dev, packed


def _first_or_tuple(res):
    return res[0] if len(res) == 1 else tuple(res)


def events_to_frames_device(events, frame_range, shape, grayscale=True, thresh=10.,
                            count_non_zero=False, background_mask=True, return_counts=False,
                            return_stats=False, out=None, max_frame_events=0, flip_x=False,
                            negate_p=False, sort_workspace=True, float_stage=DEFAULT_FLOAT_STAGE,
                            total_events=0):
    """Batched device entry.

    events:      float32 CUDA tensor [n_total, 4], or packed events: int64 CUDA tensor [n_total]
                 (pack_events / pack_events_device, layout in include/eventclip_hip.h).
    frame_range: int64 CUDA tensor [F, 2] of (begin, end) rows per frame.
    float_stage: 'float32' runs vis.py:27-39 as the reference's pinned numpy 1.25 does (the default,
                 DEFAULT_FLOAT_STAGE), 'float64' as numpy >= 2 does.
    total_events: sum of the frame lengths when known (profiling: the launch's algorithmic bytes).
    Returns uint8 CUDA tensor [F, H, W, 3] (+ raw, kept int32 [F, H, W, 2] and a
    stats structured array when asked).
    """
    import torch
    dev, packed = _check_device_events(events, frame_range)
    H, W = shape
    F = int(frame_range.shape[0])
    if out is None and not return_counts and not return_stats and sort_workspace:
        # the production form: the registered custom op (eventclip_hip::events_to_frames)
        from . import torch_ops  # noqa: F401  (registers the namespace)
        red, blue = colour_map(grayscale)
        return torch.ops.eventclip_hip.events_to_frames(
            events, frame_range, int(H), int(W), float(thresh), [int(v) for v in red],
            [int(v) for v in blue], bool(count_non_zero), bool(background_mask), int(max_frame_events),
            bool(flip_x), bool(negate_p), _float32_stage(float_stage), int(total_events))
    # debug form (raw / kept counts, per-frame statistics, caller-owned output): straight to the C ABI
    frames = out if out is not None else torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    raw = kept = stats = None
    if return_counts:
        raw = torch.empty((F, H, W, 2), dtype=torch.int32, device=dev)
        kept = torch.empty((F, H, W, 2), dtype=torch.int32, device=dev)
    if return_stats:
        stats = torch.zeros((F, ctypes.sizeof(_lib.EcFrameStats)), dtype=torch.uint8, device=dev)
    prm = make_params(shape, grayscale, thresh, count_non_zero, background_mask, max_frame_events,
                      flip_x, negate_p, float_stage, total_events)
    attach_sort_workspace(prm, events.device, sort_workspace)
    _lib.launch('ec_events_to_frames_packed' if packed else 'ec_events_to_frames', events, frame_range, F, prm, frames,
                raw, kept, stats)
    res = [frames]
    if return_counts:
        res += [raw, kept]
    if return_stats:
        dt = np.dtype([('sum', '<u8'), ('sumsq', '<u8'), ('nnz', '<u4'), ('max_kept', '<u4'),
                       ('dropped', '<u4'), ('ambiguous', '<u4'), ('thr', '<f8')])
        res.append(stats.cpu().numpy().view(dt).reshape(F))
    return _first_or_tuple(res)


# ---- time-surface frames (include/eventclip_time_surface.h: the definition, steps 1 - 7) ----
SURFACE_HEADER = os.path.join(os.path.dirname(_lib.HEADER), 'eventclip_time_surface.h')
_surface_constants, _surface_structs, SURFACE_SIGNATURES = _lib.bind_header(os.path.basename(SURFACE_HEADER))
EcTimeSurfaceParams, EcSurfaceStats = _surface_structs['EcTimeSurfaceParams'], _surface_structs['EcSurfaceStats']
DECAYS = {'linear': _surface_constants['EC_DECAY_LINEAR'], 'exp': _surface_constants['EC_DECAY_EXP']}
SURFACE_STATS_DTYPE = np.dtype([('dropped', '<u4'), ('counted', '<u4'), ('t0', '<u4'), ('t1', '<u4')])
CONVERT_METHODS = ('event_histogram', 'time_surface', 'voxel_grid')
# the names callers once had to go through to find a side header's entries typed: the handle itself, typed for everyone
surface_lib = voxel_lib = denoise_lib = _lib.lib


def time_surface_params(shape, red, blue, decay, tau, background_mask, max_frame_events, flip_x, negate_p, reverse_t,
                        total_events):
    """EcTimeSurfaceParams: what ``time_surface_device`` and the custom op both fill.  tau in seconds."""
    if decay not in DECAYS:
        raise ValueError(f"decay {decay!r}: 'linear' (timestamp image) or 'exp' (time surface)")
    p = EcTimeSurfaceParams()
    p.H, p.W = int(shape[0]), int(shape[1])
    p.decay, p.tau_us = DECAYS[decay], float(tau) * 1e6
    p.background_mask = int(bool(background_mask))
    p.max_frame_events = int(max_frame_events)
    p.flip_x, p.negate_p, p.reverse_t = int(bool(flip_x)), int(bool(negate_p)), int(bool(reverse_t))
    p.total_events = int(total_events)
    for c in range(3):
        p.red[c] = int(red[c])
        p.blue[c] = int(blue[c])
    return p


def time_surface_device(events, frame_range, shape, decay='linear', tau=0.03, grayscale=True, background_mask=True,
                        return_last=False, return_stats=False, out=None, max_frame_events=0, flip_x=False,
                        negate_p=False, reverse_t=False, total_events=0):
    """Batched device entry of the time-surface frames; events and frame_range as ``events_to_frames_device`` takes them.

    decay: 'linear', the timestamp image (a pixel's latest event scaled to the frame's time span), or 'exp', the time
           surface exp(-age / tau) with tau in seconds.
    reverse_t: keep each pixel's EARLIEST event and age from the frame's first: with negate_p and frame ranges of the
           reversed order, the time flip of test-time augmentation.
    Returns uint8 CUDA tensor [F, H, W, 3] (+ last int32 [F, H, W, 2], -1 where untouched, and a stats structured
    array -- dropped, counted, t0, t1 -- when asked).
    """
    import torch
    dev, packed = _check_device_events(events, frame_range)
    H, W = shape
    F = int(frame_range.shape[0])
    red, blue = colour_map(grayscale)
    if out is None and not return_last and not return_stats:
        # the production form: the registered custom op (eventclip_hip::events_to_time_surface)
        from . import torch_ops  # noqa: F401  (registers the namespace)
        return torch.ops.eventclip_hip.events_to_time_surface(
            events, frame_range, int(H), int(W), decay, float(tau), [int(v) for v in red], [int(v) for v in blue],
            bool(background_mask), int(max_frame_events), bool(flip_x), bool(negate_p), bool(reverse_t),
            int(total_events))
    # debug form (the surface itself, per-frame statistics, caller-owned output): straight to the C ABI
    frames = out if out is not None else torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    last = torch.empty((F, H, W, 2), dtype=torch.int32, device=dev) if return_last else None
    stats = torch.zeros((F, ctypes.sizeof(EcSurfaceStats)), dtype=torch.uint8, device=dev) if return_stats else None
    prm = time_surface_params(shape, red, blue, decay, tau, background_mask, max_frame_events, flip_x, negate_p,
                              reverse_t, total_events)
    _lib.launch('ec_events_to_time_surface_packed' if packed else 'ec_events_to_time_surface', events, frame_range, F,
                prm, frames, last, stats)
    res = [frames]
    if return_last:
        res.append(last)
    if return_stats:
        res.append(stats.cpu().numpy().view(SURFACE_STATS_DTYPE).reshape(F))
    return _first_or_tuple(res)


# ---- voxel-grid frames (include/eventclip_voxel_grid.h: the definition, steps 1 - 7) ----
VOXEL_HEADER = os.path.join(os.path.dirname(_lib.HEADER), 'eventclip_voxel_grid.h')
_voxel_constants, _voxel_structs, VOXEL_SIGNATURES = _lib.bind_header(os.path.basename(VOXEL_HEADER))
EcVoxelGridParams, EcVoxelStats = _voxel_structs['EcVoxelGridParams'], _voxel_structs['EcVoxelStats']
VOXEL_BINS = (_voxel_constants['EC_VOXEL_MIN_BINS'], _voxel_constants['EC_VOXEL_MAX_BINS'])
VOXEL_MAX_FRAME_EVENTS = _voxel_constants['EC_VOXEL_MAX_FRAME_EVENTS']
VOXEL_STATS_DTYPE = np.dtype([('dropped', '<u4'), ('counted', '<u4'), ('t0', '<u4'), ('t1', '<u4'), ('peak', '<u4')])


def voxel_grid_bands(shape, bins=3):
    """Row bands the kernel cuts a sensor into (``ec_voxel_grid_bands``; host only, 0 = refused)."""
    return int(_lib.lib().ec_voxel_grid_bands(int(shape[0]), int(shape[1]), int(bins)))


def voxel_grid_params(shape, bins, background_mask, max_frame_events, flip_x, negate_p, reverse_t, total_events):
    """EcVoxelGridParams: what ``voxel_grid_device`` and the custom op both fill."""
    if not VOXEL_BINS[0] <= int(bins) <= VOXEL_BINS[1]:
        raise ValueError(f'bins={bins}: {VOXEL_BINS[0]} .. {VOXEL_BINS[1]}')
    if int(max_frame_events) > VOXEL_MAX_FRAME_EVENTS:
        raise ValueError(f'max_frame_events={max_frame_events}: a voxel-grid frame holds at most {VOXEL_MAX_FRAME_EVENTS} '
                         'events (256 per event in int32)')
    p = EcVoxelGridParams()
    p.H, p.W, p.bins = int(shape[0]), int(shape[1]), int(bins)
    p.background_mask = int(bool(background_mask))
    p.max_frame_events = int(max_frame_events)
    p.flip_x, p.negate_p, p.reverse_t = int(bool(flip_x)), int(bool(negate_p)), int(bool(reverse_t))
    p.total_events = int(total_events)
    return p


def voxel_grid_device(events, frame_range, shape, bins=3, background_mask=True, return_grid=False, return_stats=False,
                      out=None, max_frame_events=0, flip_x=False, negate_p=False, reverse_t=False, total_events=0):
    """Batched device entry of the voxel-grid frames; events and frame_range as ``events_to_frames_device`` takes them.

    bins: temporal bins B, 2 .. 8.  Every event spreads its signed unit (256) over the two bins nearest to its place in
          the frame's time span.  Frames exist for B == 3 (channel k = bin k, 128 = zero, scaled to the frame's peak
          |G|); any other B gives the grid alone and wants ``return_grid``.
    reverse_t: the place is counted back from the frame's last event: with negate_p and frame ranges of the reversed
          order, the time flip of test-time augmentation.
    Returns uint8 CUDA tensor [F, H, W, 3] (B == 3; + grid int32 [F, H, W, B] and a stats structured array -- dropped,
    counted, t0, t1, peak -- when asked), or the grid (+ stats) alone when B != 3.
    """
    import torch
    dev, packed = _check_device_events(events, frame_range)
    H, W = shape
    F, bins = int(frame_range.shape[0]), int(bins)
    if bins != 3 and not return_grid:
        raise ValueError(f'bins={bins}: the image form exists for 3 bins only; ask for the grid (return_grid=True)')
    if bins != 3 and out is not None:
        raise ValueError(f'bins={bins}: `out` is the image, which exists for 3 bins only')
    if out is None and not return_grid and not return_stats:
        # the production form: the registered custom op (eventclip_hip::events_to_voxel_grid)
        from . import torch_ops  # noqa: F401  (registers the namespace)
        return torch.ops.eventclip_hip.events_to_voxel_grid(
            events, frame_range, int(H), int(W), bins, bool(background_mask), int(max_frame_events), bool(flip_x),
            bool(negate_p), bool(reverse_t), int(total_events))
    # debug form (the grid itself, per-frame statistics, caller-owned output): straight to the C ABI
    prm = voxel_grid_params(shape, bins, background_mask, max_frame_events, flip_x, negate_p, reverse_t, total_events)
    frames = None
    if bins == 3:
        frames = out if out is not None else torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    # (a banded sensor's bytes are coloured from its grid: without one the kernel bins every band twice)
    want_grid = return_grid or (frames is not None and voxel_grid_bands(shape, bins) > 1)
    grid = torch.empty((F, H, W, bins), dtype=torch.int32, device=dev) if want_grid else None
    stats = torch.zeros((F, ctypes.sizeof(EcVoxelStats)), dtype=torch.uint8, device=dev) if return_stats else None
    _lib.launch('ec_events_to_voxel_grid_packed' if packed else 'ec_events_to_voxel_grid', events, frame_range, F, prm,
                frames, grid, stats)
    res = [frames] if frames is not None else []
    if return_grid:
        res.append(grid)
    if return_stats:
        res.append(stats.cpu().numpy().view(VOXEL_STATS_DTYPE).reshape(F))
    return _first_or_tuple(res)


# ---- background-activity denoising (include/eventclip_denoise.h: the definition, steps 1 - 5) ----
DENOISE_HEADER = os.path.join(os.path.dirname(_lib.HEADER), 'eventclip_denoise.h')
_denoise_constants, _denoise_structs, DENOISE_SIGNATURES = _lib.bind_header(os.path.basename(DENOISE_HEADER))
EcDenoiseParams, EcDenoiseStats = _denoise_structs['EcDenoiseParams'], _denoise_structs['EcDenoiseStats']
DENOISE_RADIUS = (_denoise_constants['EC_DENOISE_MIN_RADIUS'], _denoise_constants['EC_DENOISE_MAX_RADIUS'])
DENOISE_MAX_DT_US = _denoise_constants['EC_DENOISE_MAX_DT_US']
DENOISE_STATS_DTYPE = np.dtype([('kept', '<u4'), ('removed', '<u4'), ('passed', '<u4')])

_denoise_scratch = collections.defaultdict(_lib.Scratch)   # device index -> the filter's workspace, reused by every call


def denoise_dt_us(dt):
    """The support window: seconds -> the integer microseconds of ``ec_denoise_params.dt_us``."""
    dt_us = int(round(float(dt) * 1e6))
    if not 0 <= dt_us <= DENOISE_MAX_DT_US:
        raise ValueError(f'dt={dt} s: the support window is 0 .. {DENOISE_MAX_DT_US} microseconds')
    return dt_us


def denoise_params(shape, dt_us, radius, max_sample_events, total_events=0):
    """EcDenoiseParams: what ``denoise_events_device`` and the custom op both fill."""
    if not DENOISE_RADIUS[0] <= int(radius) <= DENOISE_RADIUS[1]:
        raise ValueError(f'radius={radius}: {DENOISE_RADIUS[0]} .. {DENOISE_RADIUS[1]}')
    if not 0 <= int(dt_us) <= DENOISE_MAX_DT_US:
        raise ValueError(f'dt_us={dt_us}: 0 .. {DENOISE_MAX_DT_US}')
    p = EcDenoiseParams()
    p.H, p.W, p.radius, p.dt_us = int(shape[0]), int(shape[1]), int(radius), int(dt_us)
    p.max_sample_events = max(1, int(max_sample_events))
    p.total_events = int(total_events)
    return p


def denoise_workspace_bytes(prm, B):
    """``ec_denoise_workspace_bytes``: host only, 0 for parameters the entry points refuse."""
    return int(_lib.lib().ec_denoise_workspace_bytes(ctypes.byref(prm), int(B)))


def denoise_launch(events, sample_range, prm, events_out, counts, keep=None, stats=None):
    """The C ABI call with the workspace this module keeps per device (the custom op and the debug form share it)."""
    import torch
    B = int(sample_range.shape[0])
    need = denoise_workspace_bytes(prm, B)
    key = events.device.index if events.device.index is not None else torch.cuda.current_device()
    ws = _denoise_scratch[key].get(max(need, 256), torch.device('cuda', key))
    _lib.launch('ec_denoise_events_packed' if is_packed(events) else 'ec_denoise_events', events, sample_range, B, prm,
                events_out, counts, keep, stats, ws, ws.numel())


def denoise_events_device(events, sample_range, shape, dt, radius=1, return_mask=False, return_stats=False):
    """Batched device entry of the background-activity filter (include/eventclip_denoise.h).

    events:       float32 CUDA tensor [n_total, 4] or packed events, int64 CUDA tensor [n_total]; not modified.
    sample_range: int64 tensor [B, 2] of (begin, end) rows per sample (disjoint), on the host or the device.
    dt:           the support window in SECONDS (no default: it is the sensor's and the scene's); radius 1 .. 3.
    An event stays if a pixel within ``radius`` (not its own) fired in the ``dt`` before it; rows the frame kernels would
    not count (p == 0, outside the sensor) pass through.
    Returns (events_out, counts): the survivors of sample b are events_out[begin_b : begin_b + counts[b]], in stored
    order, the rows behind them unspecified; counts int64 CUDA [B].  + keep uint8 CUDA [n_total] (1 = written; rows outside
    every sample 0) with ``return_mask``, + a stats structured array (kept, removed, passed) with ``return_stats``.
    """
    import torch
    dev, _ = _check_device_events(events, sample_range, on_device=False)
    B = int(sample_range.shape[0])
    dt_us = denoise_dt_us(dt)
    if not return_mask and not return_stats:
        # the production form: the registered custom op (eventclip_hip::events_denoise)
        from . import torch_ops  # noqa: F401  (registers the namespace)
        return torch.ops.eventclip_hip.events_denoise(events, sample_range.to(dev).contiguous(), int(shape[0]), int(shape[1]),
                                                      dt_us, int(radius))
    host = sample_range.cpu()
    lengths = host[:, 1] - host[:, 0]
    prm = denoise_params(shape, dt_us, radius, int(lengths.max()) if B else 1, int(lengths.sum()) if B else 0)
    events_out = torch.empty_like(events)
    counts = torch.zeros((B,), dtype=torch.int64, device=dev)
    keep = torch.zeros((int(events.shape[0]),), dtype=torch.uint8, device=dev) if return_mask else None
    stats = torch.zeros((B, ctypes.sizeof(EcDenoiseStats)), dtype=torch.uint8, device=dev) if return_stats else None
    denoise_launch(events, sample_range.to(dev).contiguous(), prm, events_out, counts, keep, stats)
    res = [events_out, counts]
    if return_mask:
        res.append(keep)
    if return_stats:
        res.append(stats.cpu().numpy().view(DENOISE_STATS_DTYPE).reshape(B))
    return _first_or_tuple(res)


def denoise_events(events, resolution, dt, radius=1):
    """The filter for one sample, numpy in, numpy out: [n, 4] rows (or the dict form, or packed uint64 [n]) -> the
    surviving rows in stored order."""
    import torch
    dev = _lib.require_gpu()
    if not isinstance(events, dict) and is_packed(np.asarray(events)):
        arr = np.ascontiguousarray(events)
        ev = torch.from_numpy(arr.view(np.int64)).to(dev)
    else:
        arr = parse_events(events)
        ev = torch.from_numpy(arr).to(dev)
    rng = torch.tensor([[0, ev.shape[0]]], dtype=torch.int64)
    if ev.shape[0] == 0:
        return arr.copy()
    out, counts = denoise_events_device(ev, rng, resolution, dt, radius)
    return out[:int(counts[0])].cpu().numpy().view(arr.dtype)


# ---- refractory-period filtering (include/eventclip_refractory.h: the definition, steps 1 - 4) ----
REFRACTORY_HEADER = os.path.join(os.path.dirname(_lib.HEADER), 'eventclip_refractory.h')
_refractory_constants, _refractory_structs, REFRACTORY_SIGNATURES = _lib.bind_header(os.path.basename(REFRACTORY_HEADER))
EcRefractoryParams, EcRefractoryStats = _refractory_structs['EcRefractoryParams'], _refractory_structs['EcRefractoryStats']
REFRACTORY_MAX_PERIOD_US = _refractory_constants['EC_REFRACTORY_MAX_PERIOD_US']
# the class-list length from which a whole wave walks the list: the size at which the kernel's chain takes its other path
REFRACTORY_LONG_LIST = _refractory_constants['EC_REFRACTORY_LONG_LIST']
REFRACTORY_STATS_DTYPE = np.dtype([('kept', '<u4'), ('removed', '<u4'), ('passed', '<u4')])

_refractory_scratch = collections.defaultdict(_lib.Scratch)   # device index -> the filter's workspace, reused by every call


def refractory_period_us(seconds):
    """The dead time: seconds -> the integer microseconds of ``ec_refractory_params.period_us``."""
    us = int(round(float(seconds) * 1e6))
    if not 1 <= us <= REFRACTORY_MAX_PERIOD_US:
        raise ValueError(f'period={seconds} s: the refractory period is 1 .. {REFRACTORY_MAX_PERIOD_US} microseconds')
    return us


def refractory_bands(shape, per_polarity=False):
    """Row bands the kernel cuts a sensor into (``ec_refractory_bands``; host only, 0 = refused)."""
    return int(_lib.lib().ec_refractory_bands(int(shape[0]), int(shape[1]), int(bool(per_polarity))))


def refractory_params(shape, period_us, per_polarity, max_sample_events, total_events=0):
    """EcRefractoryParams: what ``refractory_events_device`` and the custom op both fill."""
    if not 1 <= int(period_us) <= REFRACTORY_MAX_PERIOD_US:
        raise ValueError(f'period_us={period_us}: 1 .. {REFRACTORY_MAX_PERIOD_US}')
    p = EcRefractoryParams()
    p.H, p.W, p.period_us, p.per_polarity = int(shape[0]), int(shape[1]), int(period_us), int(bool(per_polarity))
    p.max_sample_events = max(1, int(max_sample_events))
    p.total_events = int(total_events)
    return p


def refractory_workspace_bytes(prm, B):
    """``ec_refractory_workspace_bytes``: host only, 0 for parameters the entry points refuse."""
    return int(_lib.lib().ec_refractory_workspace_bytes(ctypes.byref(prm), int(B)))


def refractory_launch(events, sample_range, prm, events_out, counts, keep=None, stats=None):
    """The C ABI call with the workspace this module keeps per device (the custom op and the debug form share it)."""
    import torch
    B = int(sample_range.shape[0])
    need = refractory_workspace_bytes(prm, B)
    key = events.device.index if events.device.index is not None else torch.cuda.current_device()
    ws = _refractory_scratch[key].get(max(need, 256), torch.device('cuda', key))
    _lib.launch('ec_refractory_events_packed' if is_packed(events) else 'ec_refractory_events', events, sample_range, B, prm,
                events_out, counts, keep, stats, ws, ws.numel())


def refractory_events_device(events, sample_range, shape, period, per_polarity=False, return_mask=False, return_stats=False):
    """Batched device entry of the refractory-period filter (include/eventclip_refractory.h).

    events:       float32 CUDA tensor [n_total, 4] or packed events, int64 CUDA tensor [n_total]; not modified.
    sample_range: int64 tensor [B, 2] of (begin, end) rows per sample (disjoint), on the host or the device.
    period:       the dead time in SECONDS (no default: it is the sensor's and the scene's); per_polarity: ON and OFF
                  events of a pixel have separate dead times.
    After a kept event its pixel is blind for ``period``: a later event of the pixel stays only if it comes at least
    ``period`` after the last KEPT one (a removed event does not extend the dead time).  The rows need not be sorted by
    time; rows the frame kernels would not count (p == 0, outside the sensor) pass through.
    Returns (events_out, counts): the survivors of sample b are events_out[begin_b : begin_b + counts[b]], in stored
    order, the rows behind them unspecified; counts int64 CUDA [B].  + keep uint8 CUDA [n_total] (1 = written; rows outside
    every sample 0) with ``return_mask``, + a stats structured array (kept, removed, passed) with ``return_stats``.
    """
    import torch
    dev, _ = _check_device_events(events, sample_range, on_device=False)
    B = int(sample_range.shape[0])
    period_us = refractory_period_us(period)
    if not return_mask and not return_stats:
        # the production form: the registered custom op (eventclip_hip::events_refractory)
        from . import torch_ops  # noqa: F401  (registers the namespace)
        return torch.ops.eventclip_hip.events_refractory(events, sample_range.to(dev).contiguous(), int(shape[0]), int(shape[1]),
                                                         period_us, bool(per_polarity))
    host = sample_range.cpu()
    lengths = host[:, 1] - host[:, 0]
    prm = refractory_params(shape, period_us, per_polarity, int(lengths.max()) if B else 1, int(lengths.sum()) if B else 0)
    events_out = torch.empty_like(events)
    counts = torch.zeros((B,), dtype=torch.int64, device=dev)
    keep = torch.zeros((int(events.shape[0]),), dtype=torch.uint8, device=dev) if return_mask else None
    stats = torch.zeros((B, ctypes.sizeof(EcRefractoryStats)), dtype=torch.uint8, device=dev) if return_stats else None
    refractory_launch(events, sample_range.to(dev).contiguous(), prm, events_out, counts, keep, stats)
    res = [events_out, counts]
    if return_mask:
        res.append(keep)
    if return_stats:
        res.append(stats.cpu().numpy().view(REFRACTORY_STATS_DTYPE).reshape(B))
    return _first_or_tuple(res)


def refractory_events(events, resolution, period, per_polarity=False):
    """The filter for one sample, numpy in, numpy out: [n, 4] rows (or the dict form, or packed uint64 [n]) -> the
    surviving rows in stored order."""
    import torch
    dev = _lib.require_gpu()
    if not isinstance(events, dict) and is_packed(np.asarray(events)):
        arr = np.ascontiguousarray(events)
        ev = torch.from_numpy(arr.view(np.int64)).to(dev)
    else:
        arr = parse_events(events)
        ev = torch.from_numpy(arr).to(dev)
    rng = torch.tensor([[0, ev.shape[0]]], dtype=torch.int64)
    if ev.shape[0] == 0:
        return arr.copy()
    out, counts = refractory_events_device(ev, rng, resolution, period, per_polarity)
    return out[:int(counts[0])].cpu().numpy().view(arr.dtype)


# ---- fixed-duration windows (include/eventclip_time_windows.h: the definition, steps 1 - 7) ----
TIME_WINDOWS_HEADER = os.path.join(os.path.dirname(_lib.HEADER), 'eventclip_time_windows.h')
_windows_constants, _windows_structs, TIME_WINDOWS_SIGNATURES = _lib.bind_header(os.path.basename(TIME_WINDOWS_HEADER))
EcTimeWindowsParams, EcTimeWindowsStats = _windows_structs['EcTimeWindowsParams'], _windows_structs['EcTimeWindowsStats']
TIME_WINDOWS_MAX_US = _windows_constants['EC_TIME_WINDOWS_MAX_US']
# rows of one workgroup's slice and loads in flight per thread: the sizes at which the kernel's loops turn over
TIME_WINDOWS_SLICE_ROWS = _windows_constants['EC_TIME_WINDOWS_SLICE_ROWS']
TIME_WINDOWS_UNROLL = _windows_constants['EC_TIME_WINDOWS_UNROLL']
TIME_WINDOWS_STATS_DTYPE = np.dtype([('t_first', '<u4'), ('t_last', '<u4'), ('unsorted', '<u4'), ('windows', '<i4')])
SPLIT_METHODS = ('event_count', 'time_window')


def time_window_us(seconds, what='window'):
    """A window or a stride: seconds -> the integer microseconds of ``ec_time_windows_params`` (as ``denoise_dt_us``)."""
    us = int(round(float(seconds) * 1e6))
    if not 1 <= us <= TIME_WINDOWS_MAX_US:
        raise ValueError(f'{what}={seconds} s: 1 .. {TIME_WINDOWS_MAX_US} microseconds')
    return us


def time_windows_params(dt_us, stride_us, max_windows, from_last=False, total_events=0):
    """EcTimeWindowsParams: what the custom op fills."""
    for what, us in (('dt_us', dt_us), ('stride_us', stride_us)):
        if not 1 <= int(us) <= TIME_WINDOWS_MAX_US:
            raise ValueError(f'{what}={us}: 1 .. {TIME_WINDOWS_MAX_US}')
    if int(max_windows) <= 0:
        raise ValueError(f'max_windows={max_windows}: at least 1')
    p = EcTimeWindowsParams()
    p.dt_us, p.stride_us, p.max_windows = int(dt_us), int(stride_us), int(max_windows)
    p.from_last, p.total_events = int(bool(from_last)), int(total_events)
    return p


def time_windows_device(events, sample_range, window, stride=None, max_windows=64, from_last=False):
    """Batched device entry of the fixed-duration windows (include/eventclip_time_windows.h).

    events:       float32 CUDA tensor [n_total, 4] or packed events, int64 CUDA tensor [n_total]; not modified.
    sample_range: int64 tensor [B, 2] of (begin, end) rows per sample, on the host or the device.
    window, stride: SECONDS; ``stride=None`` means ``window`` (windows back to back).  Window k of a sample covers the
                  ticks [t_first + k stride, t_first + k stride + window); with ``from_last`` the windows are counted back
                  from the sample's last event (the time flip of test-time augmentation, as stored rows).
    Returns (bounds, stats): bounds int64 CUDA [B, max_windows, 2], the (begin, end) event rows of every window, -1 in the
    rows the call does not write (behind a sample's windows; of an empty sample); stats a numpy structured array
    (t_first, t_last, unsorted, windows) -- windows is the full count even above max_windows, and -1 for a sample whose
    ticks are not sorted, whose bounds mean nothing.  Reading stats waits for the kernel.
    """
    import torch
    from . import torch_ops  # noqa: F401  (registers the namespace)
    dev, _ = _check_device_events(events, sample_range, on_device=False)
    dt_us = time_window_us(window)
    stride_us = dt_us if stride is None else time_window_us(stride, 'stride')
    # (sizes the grid and states the bytes; no sample is longer than the array)
    total = int((sample_range[:, 1] - sample_range[:, 0]).clamp(min=0).sum()) if not sample_range.is_cuda else int(events.shape[0])
    bounds, stats = torch.ops.eventclip_hip.events_time_windows(
        events, sample_range.to(dev).contiguous(), dt_us, stride_us, int(max_windows), bool(from_last), total)
    return bounds, stats.cpu().numpy().view(TIME_WINDOWS_STATS_DTYPE).reshape(int(sample_range.shape[0]))


def _all_time_windows(ev_d, window, stride, from_last=False):
    """Every window of ONE sample (all rows of ``ev_d``) -> (bounds numpy int64 [windows, 2], its stats record); a second
    launch when there are more than the first one's 64.  Unsorted timestamps raise."""
    import torch
    rng = torch.tensor([[0, int(ev_d.shape[0])]], dtype=torch.int64)
    bounds, stats = time_windows_device(ev_d, rng, window, stride, 64, from_last)
    if stats['unsorted'][0] > 0:
        raise ValueError(f"time_window: the timestamps are not sorted ({int(stats['unsorted'][0])} rows earlier than the row "
                         'before them); nothing is sorted for the caller')
    if stats['windows'][0] > 64:
        bounds, stats = time_windows_device(ev_d, rng, window, stride, int(stats['windows'][0]), from_last)
    return bounds[0, :int(stats['windows'][0])].cpu().numpy(), stats[0]


def split_time_window(events_or_t, window, stride=None):
    """The windows of one sample, numpy in: ``events_or_t`` is [n, 4] rows (or the dict form), packed uint64 / int64 [n],
    or a 1-D float array of timestamps in seconds.  ``window`` and ``stride`` (default: ``window``) in seconds.
    Returns (idx0, idx1, t0, t1) like ``split_event_count``: window k is rows [idx0[k], idx1[k]) -- every window, the empty
    ones (idx0[k] == idx1[k]) too -- and t0[k], t1[k] are its edges in seconds, [t0, t1), on the kernel's microsecond ticks.
    Computed by the kernel behind ``ec_time_windows``."""
    import torch
    dev = _lib.require_gpu()
    arr = events_or_t if isinstance(events_or_t, dict) else np.asarray(events_or_t)
    if not isinstance(arr, dict) and is_packed(arr):
        ev = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(dev)
    elif not isinstance(arr, dict) and arr.ndim == 1:
        rows = np.zeros((arr.shape[0], 4), dtype=np.float32)
        rows[:, 2] = arr
        ev = torch.from_numpy(rows).to(dev)
    else:
        ev = torch.from_numpy(parse_events(arr)).to(dev)
    if ev.shape[0] == 0:
        raise IndexError('split_time_window: empty event array')
    bounds, stats = _all_time_windows(ev, window, stride)
    dt_us = time_window_us(window)
    stride_us = dt_us if stride is None else time_window_us(stride, 'stride')
    lo = int(stats['t_first']) + np.arange(len(bounds), dtype=np.int64) * stride_us
    return bounds[:, 0].tolist(), bounds[:, 1].tolist(), lo / 1e6, (lo + dt_us) / 1e6


def events2frames(events, split_method, convert_method, shape=(180, 240), **kwargs):
    """Drop-in for the reference's events2frames (vis.py:75-117): numpy in, numpy out.

    convert_method='time_surface' (not in the reference) takes ``decay`` ('linear' or 'exp') and ``tau`` (seconds) and
    ignores ``thresh``, ``count_non_zero`` and ``float_stage``: there is no hot-pixel threshold and no frame maximum.
    convert_method='voxel_grid' (not in the reference) takes ``bins`` (3: the image form has three channels) and ignores
    those three and ``grayscale``: channel k is temporal bin k.
    ``denoise=dict(dt=seconds, radius=1)`` (not in the reference) runs the background-activity filter of
    include/eventclip_denoise.h first: the chunks are cut from the survivors.
    ``refractory=dict(period=seconds, per_polarity=False)`` (not in the reference) runs the refractory-period filter of
    include/eventclip_refractory.h first of all, before ``denoise`` when both are given.
    split_method='time_window' (not in the reference) takes ``window`` and ``stride`` (seconds; stride defaults to window)
    and ``min_events`` (1) instead of ``N``: one frame per window of include/eventclip_time_windows.h that holds at least
    ``min_events`` events, in window order."""
    import torch
    grayscale = kwargs.pop('grayscale', True)
    denoise = kwargs.pop('denoise', None)
    refractory = kwargs.pop('refractory', None)
    ev = parse_events(events)
    assert split_method in SPLIT_METHODS                 # vis.py:90, + 'time_window'
    if convert_method not in CONVERT_METHODS:            # vis.py:113
        raise NotImplementedError(f'{convert_method} not implemented!')
    if refractory is not None:
        ev = refractory_events(ev, shape, refractory['period'], refractory.get('per_polarity', False))
    if denoise is not None:
        ev = denoise_events(ev, shape, denoise['dt'], denoise.get('radius', 1))
    N = int(kwargs['N']) if split_method == 'event_count' else None      # 'time_window' neither needs nor reads it
    if ev.shape[0] == 0:
        raise IndexError('events2frames: empty event array')
    dev = _lib.require_gpu()
    ev_d = torch.from_numpy(ev).to(dev)
    if split_method == 'time_window':
        bounds, _ = _all_time_windows(ev_d, kwargs['window'], kwargs.get('stride'))
        bounds = bounds[bounds[:, 1] - bounds[:, 0] >= max(1, int(kwargs.get('min_events', 1)))]
        if len(bounds) == 0:
            raise ValueError(f"events2frames: no window of {kwargs['window']} s holds min_events={kwargs.get('min_events', 1)} events")
        idx0, idx1 = bounds[:, 0].tolist(), bounds[:, 1].tolist()
    else:
        idx0, idx1 = chunk_bounds(ev.shape[0], N)
    rng = torch.tensor(np.stack([idx0, idx1], 1), dtype=torch.int64, device=dev)
    common = dict(grayscale=grayscale, background_mask=kwargs.get('background_mask', True), return_stats=True,
                  max_frame_events=max(b - a for a, b in zip(idx0, idx1)),
                  total_events=sum(b - a for a, b in zip(idx0, idx1)))
    if convert_method == 'time_surface':
        frames, stats = time_surface_device(ev_d, rng, shape, decay=kwargs.get('decay', 'linear'),
                                            tau=float(kwargs.get('tau', 0.03)), **common)
    elif convert_method == 'voxel_grid':
        if int(kwargs.get('bins', 3)) != 3:
            raise ValueError(f"bins={kwargs['bins']}: voxel-grid frames have 3 bins, one per colour channel "
                             '(voxel_grid_device returns the grid of 2 .. 8 bins)')
        del common['grayscale']
        frames, stats = voxel_grid_device(ev_d, rng, shape, bins=3, **common)
    else:
        frames, stats = events_to_frames_device(
            ev_d, rng, shape, thresh=float(kwargs.get('thresh', 10.)),
            count_non_zero=kwargs.get('count_non_zero', False),
            float_stage=kwargs.get('float_stage', DEFAULT_FLOAT_STAGE), **common)
    if int(stats['dropped'].sum()) > 0:
        # the reference's bincount/reshape raises on such input (vis.py:11)
        raise ValueError('events2frames: events outside the sensor '
                         f'({int(stats["dropped"].sum())} dropped)')
    return frames.cpu().numpy()


def center_events_device(events, sample_range, resolution):
    """In-place center_events (datasets/utils.py:38-57) for a batch: events float32 CUDA
    [n_total, 4] (or packed int64 [n_total]), sample_range int64 CUDA [B, 2]."""
    import torch
    _lib.require_gpu()
    packed = is_packed(events)
    assert events.is_cuda and events.is_contiguous() and (packed or events.dtype == torch.float32)
    assert sample_range.is_cuda and sample_range.dtype == torch.int64
    H, W = resolution
    _lib.launch('ec_center_events_packed' if packed else 'ec_center_events', events, sample_range.contiguous(),
                int(sample_range.shape[0]), int(H), int(W))
    return events


def center_events(events, resolution=(180, 240)):
    """Drop-in for datasets/utils.py center_events: numpy [n, 4] in, centred copy out."""
    import torch
    dev = _lib.require_gpu()
    ev = torch.from_numpy(parse_events(events)).to(dev)
    rng = torch.tensor([[0, ev.shape[0]]], dtype=torch.int64, device=dev)
    return center_events_device(ev, rng, resolution).cpu().numpy()
