"""Events -> model-ready views on the MI355X: device-side mirror of the reference's
``Event2ImageDataset`` (datasets/event2img.py:14-145) plus the DataLoader collate.

The reference converts ONE sample per ``__getitem__`` in CPU worker processes:
``events2frames`` (:118) -> PIL -> ``self.transforms`` per frame (:119-122) ->
``_subsample_imgs`` (:80-92, pad with zero tensors / random subset to ``max_imgs``)
and the loader stacks samples into ``img [B, T, 3, R, R]``, ``valid_mask [B, T]``.
Here a whole batch goes through two kernels (events->frames, preprocess) with the
chunk bookkeeping (``split_event_count``, ``max_imgs``, padding, masks) done on the
host from event counts alone (``split_method='time_window'``: from the window bounds a third kernel
finds on the device).  No CPU fallback.
"""
import copy

import numpy as np
import torch

from . import _lib
from . import vis
from .preprocess import preprocess_frames


class Event2ImagePipeline:
    """Batched ``_event2img`` (event2img.py:114-128).

    resolution, max_n: the event dataset's constants (caltech.py:52-58 etc.).
    quantize_args: same dict as the reference's configs (``max_imgs``, ``N``,
        ``split_method``, ``convert_method``, ``grayscale``, ``count_non_zero``,
        ``background_mask``).  ``convert_method`` is ``'event_histogram'`` or ``'time_surface'`` (not in the
        reference: the latest-timestamp frames of include/eventclip_time_surface.h), which reads ``decay``
        (``'linear'``, the default, or ``'exp'``) and ``tau`` (seconds, 0.03) and accepts but ignores ``thresh``,
        ``count_non_zero`` and ``float_stage``: it has no hot-pixel threshold and no frame maximum.  Or
        ``'voxel_grid'`` (not in the reference either: the temporal-bin frames of include/eventclip_voxel_grid.h),
        which reads ``bins`` (3, the only value with an image form) and ignores those three and ``grayscale``.
        ``denoise`` (not in the reference; absent or ``None`` = off): ``dict(dt=seconds, radius=1)`` puts the
        background-activity filter of include/eventclip_denoise.h in front of whichever form is chosen: an event stays
        only if a neighbouring pixel fired in the ``dt`` before it, and the chunks are cut from the survivors.
        ``refractory`` (not in the reference; absent or ``None`` = off): ``dict(period=seconds, per_polarity=False)`` puts
        the refractory-period filter of include/eventclip_refractory.h first of all, in front of ``denoise`` when both are
        given: after a kept event its pixel (with ``per_polarity``: its pixel and polarity) is blind for ``period``.
        ``split_method`` is ``'event_count'`` (views of ``N`` events) or ``'time_window'`` (not in the reference: the
        fixed-duration windows of include/eventclip_time_windows.h), which reads ``window`` (seconds, required), ``stride``
        (seconds, default ``window``), ``min_events`` (1: a window with fewer rows is no view), ``max_windows`` (64: a
        sample that spans more raises) and ``max_imgs`` (T itself, default 10) and ignores ``N``.  The events of a
        sample must be sorted by time.  The result gains ``window_index`` [B, T] (CUDA int32): the window k of every
        view, -1 for a padded one; window k starts ``k * stride`` after the sample's first event (with tflip: ends
        ``k * stride`` before its last).
    n_px: CLIP input resolution.  patch/kpad/dtype: when given, ``__call__`` emits the
        16-bit im2col rows for ``CLIP.encode_patches`` instead of fp32 images.
    frames_u8: emit the resized + cropped uint8 frames (``frames_u8`` [Fv, R, R, 3]) instead, the input of
        ``ResNetCLIP.encode_frames`` (ToTensor and Normalize run in its stem kernel).
    """

    def __init__(self, resolution, max_n, quantize_args, n_px=224, patch=None, kpad=None,
                 dtype=torch.float16, generator=None, augment=False, frames_u8=False):
        qa = copy.deepcopy(quantize_args)
        self.resolution = tuple(resolution)
        self.split_method = qa['split_method']
        self.event_rep = qa['convert_method']
        assert self.split_method in vis.SPLIT_METHODS                   # event2img.py:69, + 'time_window'
        if self.event_rep not in vis.CONVERT_METHODS:                    # vis.py:113
            raise NotImplementedError(f'{self.event_rep} not implemented!')
        if self.split_method == 'time_window':
            # views are windows of fixed duration (include/eventclip_time_windows.h); N is not read, T = max_imgs
            if 'window' not in qa:
                raise ValueError("split_method='time_window' reads quantize_args['window'] (seconds)")
            self.window = float(qa['window'])
            self.stride = float(qa['stride']) if qa.get('stride') is not None else self.window
            vis.time_window_us(self.window), vis.time_window_us(self.stride, 'stride')
            self.min_events, self.max_windows = int(qa.get('min_events', 1)), int(qa.get('max_windows', 64))
            if self.min_events < 1 or self.max_windows < 1:
                raise ValueError(f'min_events={self.min_events}, max_windows={self.max_windows}: at least 1 each')
            self.N = None
            self.max_imgs = max(int(qa.pop('max_imgs', 10)), 1)
        else:
            self.N = int(qa['N'])
            max_imgs = round(max_n / self.N)                             # event2img.py:70
            max_max_imgs = qa.pop('max_imgs', 10)                        # event2img.py:71
            self.max_imgs = max(min(max_imgs, max_max_imgs), 1)          # event2img.py:72
        self.grayscale = qa.get('grayscale', True)
        self.thresh = float(qa.get('thresh', 10.))
        self.count_non_zero = bool(qa.get('count_non_zero', False))
        self.background_mask = bool(qa.get('background_mask', True))
        # not a key of the reference's configs: which numpy the frames should agree with (vis.py:27)
        self.float_stage = qa.get('float_stage', vis.DEFAULT_FLOAT_STAGE)
        # convert_method='time_surface' only
        self.decay, self.tau = qa.get('decay', 'linear'), float(qa.get('tau', 0.03))
        if self.decay not in vis.DECAYS:
            raise ValueError(f"decay {self.decay!r}: 'linear' or 'exp'")
        # convert_method='voxel_grid' only
        self.bins = int(qa.get('bins', 3))
        if self.event_rep == 'voxel_grid' and self.bins != 3:
            raise ValueError(f'bins={self.bins}: voxel-grid frames have 3 temporal bins, one per colour channel '
                             '(vis.voxel_grid_device returns the grid of 2 .. 8 bins)')
        # the background-activity filter in front of every form (None = off: nothing below changes)
        self.max_n = int(max_n)
        self.denoise = qa.get('denoise')
        if self.denoise is not None:
            if not isinstance(self.denoise, dict) or 'dt' not in self.denoise or set(self.denoise) - {'dt', 'radius'}:
                raise ValueError(f"denoise {self.denoise!r}: dict(dt=seconds, radius=1)")
            self.denoise = dict(dt=float(self.denoise['dt']), radius=int(self.denoise.get('radius', 1)))
            vis.denoise_params(self.resolution, vis.denoise_dt_us(self.denoise['dt']), self.denoise['radius'], 1)
        # the refractory-period filter, in front of the background-activity one (None = off: nothing below changes)
        self.refractory = qa.get('refractory')
        if self.refractory is not None:
            if (not isinstance(self.refractory, dict) or 'period' not in self.refractory
                    or set(self.refractory) - {'period', 'per_polarity'}
                    or not isinstance(self.refractory.get('per_polarity', False), (bool, np.bool_))):
                raise ValueError(f"refractory {self.refractory!r}: dict(period=seconds, per_polarity=False)")
            self.refractory = dict(period=float(self.refractory['period']),
                                   per_polarity=bool(self.refractory.get('per_polarity', False)))
            prm = vis.refractory_params(self.resolution, vis.refractory_period_us(self.refractory['period']),
                                        self.refractory['per_polarity'], 1)
            if vis.refractory_workspace_bytes(prm, 1) == 0:
                raise ValueError(f'refractory: a sensor of {self.resolution} does not fit the filter\'s row band')
        self.n_px, self.patch, self.kpad, self.dtype = int(n_px), patch, kpad, dtype
        self.frames_u8 = bool(frames_u8)
        assert not (self.frames_u8 and self.patch), 'frames_u8 and patch rows are two different outputs'
        self.generator = generator
        self.strict = True   # raise on events outside the sensor, as the reference does
        # training-time RandAugment on the frames (event2img.py:34-42, :120-121): two ops per sample,
        # bicubic, white fill on masked-background frames, black otherwise
        self.augment = bool(augment)
        if self.augment:
            from .randaugment import RandAugment
            self.augmentation = RandAugment(
                num_ops=2, interpolation='bicubic',
                fill=[255, 255, 255] if self.background_mask else [0, 0, 0])

    @property
    def filters(self):
        """does an event filter (refractory, denoise) stand in front of the views?"""
        return self.refractory is not None or self.denoise is not None

    # ---- host bookkeeping: which event rows make which view ----
    def plan(self, n_events, tflip=False, starts=None):
        """n_events: per-sample event counts.  Returns (frame_range int64 [Fv, 2],
        row_idx int32 [B, T], valid_mask bool [B, T]) as CPU tensors; row_idx[b, t] is the
        compact frame number of view t of sample b, or -1 for a padded view.
        tflip: chunk the time-reversed stream (utils.py:26-35): chunk [a, b) of the reversed
        order covers rows [n - b, n - a) of the stored order (a histogram ignores order, and a time surface
        takes the reversed time as ``reverse_t``).
        starts: first event row of every sample when the samples are not back to back (after
        eventclip_amd.augment.augment_events_device has dropped events)."""
        T = self.max_imgs
        B = len(n_events)
        ranges, row_idx = [], np.full((B, T), -1, dtype=np.int32)
        off = 0
        for b, n in enumerate(n_events):
            n = int(n)
            if starts is not None:
                off = int(starts[b])
            if n <= 0:
                raise IndexError('sample with no events (the reference resamples these upstream, '
                                 'caltech.py:181-182)')
            idx0, idx1 = vis.chunk_bounds(n, self.N)
            sel = list(range(len(idx0)))
            if len(sel) > T:                                             # event2img.py:83-86
                sel = torch.randperm(len(sel), generator=self.generator)[:T].tolist()
            for t, f in enumerate(sel):                                  # event2img.py:87-91
                row_idx[b, t] = len(ranges)
                if tflip:
                    ranges.append((off + n - idx1[f], off + n - idx0[f]))
                else:
                    ranges.append((off + idx0[f], off + idx1[f]))
            off += n
        fr = torch.tensor(ranges, dtype=torch.int64).reshape(-1, 2)
        ri = torch.from_numpy(row_idx)
        return fr, ri, ri >= 0

    def plan_time_windows(self, events, n_events, tflip=False, starts=None):
        """split_method='time_window': ``plan`` for windows of fixed duration.  The windows are found on the device
        (vis.time_windows_device) and the plan is built from the bounds copied back: one small synchronisation.
        A sample's views are its windows with at least ``min_events`` rows, in window order; more than T of them are
        thinned by the draw chunks get.  tflip: the windows are counted back from the last event (``from_last``), which are
        the windows of the time-reversed stream as stored rows.
        Returns (frame_range, row_idx, valid_mask, window_index int32 [B, T]): the k of every view, -1 for a padded one."""
        T, B = self.max_imgs, len(n_events)
        n = np.asarray(n_events, dtype=np.int64)
        if (n <= 0).any():
            raise IndexError('sample with no events (the reference resamples these upstream, caltech.py:181-182)')
        o0 = np.asarray(starts if starts is not None else np.concatenate([[0], np.cumsum(n)[:-1]]), dtype=np.int64)
        sr = torch.tensor(np.stack([o0, o0 + n], 1), dtype=torch.int64)
        bounds, stats = vis.time_windows_device(events, sr, self.window, self.stride, self.max_windows, from_last=tflip)
        unsorted = np.flatnonzero(stats['unsorted'] > 0)
        if len(unsorted):
            raise ValueError(f'time_window: the timestamps of samples {unsorted.tolist()} are not sorted '
                             f"({stats['unsorted'][unsorted].tolist()} rows earlier than the row before them)")
        over = np.flatnonzero(stats['windows'] > self.max_windows)
        if len(over):
            raise ValueError(f"time_window: samples {over.tolist()} span {stats['windows'][over].tolist()} windows of stride "
                             f'{self.stride} s, more than max_windows={self.max_windows}')
        bounds = bounds.cpu().numpy()
        ranges, empty = [], []
        row_idx, window_index = np.full((B, T), -1, dtype=np.int32), np.full((B, T), -1, dtype=np.int32)
        for b in range(B):
            rows = bounds[b, :int(stats['windows'][b])]
            sel = np.flatnonzero(rows[:, 1] - rows[:, 0] >= self.min_events).tolist()
            if not sel:
                empty.append(b)
                continue
            if len(sel) > T:                                             # event2img.py:83-86
                sel = [sel[i] for i in torch.randperm(len(sel), generator=self.generator)[:T].tolist()]
            for t, k in enumerate(sel):
                row_idx[b, t], window_index[b, t] = len(ranges), k
                ranges.append((int(rows[k, 0]), int(rows[k, 1])))
        if empty:
            raise ValueError(f'time_window: no window of samples {empty} holds min_events={self.min_events} events')
        fr = torch.tensor(ranges, dtype=torch.int64).reshape(-1, 2)
        ri = torch.from_numpy(row_idx)
        return fr, ri, ri >= 0, torch.from_numpy(window_index)

    def frames(self, events, frame_range, hflip=False, tflip=False, total_events=0, max_frame_events=None):
        """uint8 [Fv, H, W, 3] for the planned views (vis.events2frames, batched).  The time flip of a time surface or
        a voxel grid (utils.py:26-35: t' = t_last - t, p' = -p) is reverse_t with negate_p on the stored rows.
        max_frame_events: the longest planned view (N when the views are chunks of N events)."""
        common = dict(grayscale=self.grayscale, background_mask=self.background_mask, return_stats=self.strict,
                      max_frame_events=self.N if max_frame_events is None else int(max_frame_events), flip_x=hflip,
                      negate_p=tflip, total_events=total_events)
        if self.event_rep == 'time_surface':
            out = vis.time_surface_device(events, frame_range, self.resolution, decay=self.decay, tau=self.tau,
                                          reverse_t=tflip, **common)
        elif self.event_rep == 'voxel_grid':
            del common['grayscale']                                       # channel k is temporal bin k
            out = vis.voxel_grid_device(events, frame_range, self.resolution, bins=self.bins, reverse_t=tflip, **common)
        else:
            out = vis.events_to_frames_device(
                events, frame_range, self.resolution, thresh=self.thresh, count_non_zero=self.count_non_zero,
                float_stage=self.float_stage, **common)
        if self.strict:
            frames, stats = out
            if int(stats['dropped'].sum()) > 0:
                raise ValueError('events outside the sensor '
                                 f'({int(stats["dropped"].sum())} dropped; vis.py:11 would raise)')
            return frames
        return out

    @staticmethod
    def _concat(samples, dev):
        """Per-sample arrays -> one device tensor + counts.  Samples are float [n_i, 4] (or the
        reference's dict form) or packed uint64 / int64 [n_i] (vis.pack_events)."""
        n_events = [int(e.shape[0]) for e in samples]
        host = [e.cpu().numpy() if torch.is_tensor(e) else e for e in samples]
        if all(not isinstance(e, dict) and vis.is_packed(e) for e in host):
            cat = np.concatenate([np.asarray(e).view(np.int64) for e in host])
        else:
            cat = np.concatenate([vis.parse_events(e) for e in host], axis=0)
        return torch.from_numpy(cat).to(dev), n_events

    def filter(self, events, n_events, starts=None):
        """quantize_args['refractory'], then quantize_args['denoise']: the survivors of every sample, compacted at the
        sample's unchanged first row.  -> (events_out, filtered counts, starts).  Both filters look at the stored ticks;
        flips are view transforms and come after."""
        n = np.asarray(n_events, dtype=np.int64)
        o0 = np.asarray(starts if starts is not None else np.concatenate([[0], np.cumsum(n)[:-1]]), dtype=np.int64)
        too_long = np.flatnonzero(n > self.max_n)
        if len(too_long):
            raise ValueError(f'denoise: samples {too_long.tolist()} hold more than max_n={self.max_n} events')
        if self.refractory is not None:
            # (cannot empty a sample that has a counted event: the first event of every class is kept)
            sr = torch.tensor(np.stack([o0, o0 + n], 1), dtype=torch.int64)
            events, counts = vis.refractory_events_device(events, sr, self.resolution, self.refractory['period'],
                                                          self.refractory['per_polarity'])
            n = counts.cpu().numpy().astype(np.int64)
            if self.denoise is None:
                return events, [int(c) for c in n], o0
        sr = torch.tensor(np.stack([o0, o0 + n], 1), dtype=torch.int64)
        out, counts = vis.denoise_events_device(events, sr, self.resolution, self.denoise['dt'], self.denoise['radius'])
        counts = counts.cpu().numpy()
        emptied = np.flatnonzero((counts <= 0) & (n > 0))
        if len(emptied):
            raise ValueError(f"denoise: no event of samples {emptied.tolist()} has a neighbour within dt={self.denoise['dt']} s "
                             f"(radius {self.denoise['radius']}): the filter would empty them")
        return out, [int(c) for c in counts], o0

    def __call__(self, events, n_events=None, hflip=False, tflip=False, center=False, starts=None, filtered=False):
        """events: list of per-sample float32 [n_i, 4] arrays/tensors (or packed uint64 [n_i],
        vis.pack_events), or one CUDA tensor [sum n_i, 4] (packed: int64 [sum n_i]) with
        ``n_events`` giving the per-sample counts.
        hflip / tflip: the test-time-augmentation views of event2img.py:94-112;
        center: apply center_events (utils.py:38-57, in place) first, as the N-Caltech /
        N-ImageNet readers do (caltech.py:176).
        With ``quantize_args['refractory']`` or ``quantize_args['denoise']`` the events are filtered after centring and
        before chunking, the refractory filter first (``filtered``: they are the filters' survivors already, as ``tta``
        passes them), and the result gains ``n_events``, the filtered counts.

        Returns a dict with ``valid_mask`` [B, T] (CUDA bool), ``row_idx`` [B, T] (CUDA
        int32) and either ``patches`` [Fv, G, kpad] (fused path), ``frames_u8`` [Fv, R, R, 3] or ``img``
        [B, T, 3, R, R] float32 (the reference's batch layout, padded views all-zero)."""
        dev = _lib.require_gpu()
        if isinstance(events, (list, tuple)):
            events, n_events = self._concat(events, dev)
        assert events.is_cuda and n_events is not None
        assert vis.is_packed(events) or events.dtype == torch.float32
        if center:
            o0 = np.asarray(starts if starts is not None else np.concatenate([[0], np.cumsum(n_events)[:-1]]))
            offs = np.stack([o0, o0 + np.asarray(n_events)], 1)
            sr = torch.tensor(offs, dtype=torch.int64, device=dev)
            vis.center_events_device(events, sr, self.resolution)
        if self.filters and not filtered:
            events, n_events, starts = self.filter(events, n_events, starts)
        wi = longest = None
        if self.split_method == 'time_window':
            fr, ri, vm, wi = self.plan_time_windows(events, n_events, tflip=tflip, starts=starts)
            longest = int((fr[:, 1] - fr[:, 0]).max())
        else:
            fr, ri, vm = self.plan(n_events, tflip=tflip, starts=starts)
        fr_d = fr.to(dev)
        frames = self.frames(events, fr_d, hflip=hflip, tflip=tflip,
                             total_events=int((fr[:, 1] - fr[:, 0]).sum()), max_frame_events=longest)
        out = dict(valid_mask=vm.to(dev), row_idx=ri.to(dev))
        if wi is not None:
            out['window_index'] = wi.to(dev)
        if self.filters:
            out['n_events'] = [int(n) for n in n_events]
        if self.augment:
            frames = self._augment_frames(frames, ri)
        if self.frames_u8:
            out['frames_u8'] = preprocess_frames(frames, self.n_px, mode='u8')
        elif self.patch:
            out['patches'] = preprocess_frames(frames, self.n_px, mode='patches', patch=self.patch,
                                               kpad=self.kpad, dtype=self.dtype)
        else:
            chw = preprocess_frames(frames, self.n_px, mode='chw')
            B, T = ri.shape
            img = torch.zeros((B, T, 3, self.n_px, self.n_px), dtype=torch.float32, device=dev)
            img[out['valid_mask']] = chw                                 # event2img.py:88-91
            out['img'] = img
        return out


    def _augment_frames(self, frames, row_idx):
        """One RandAugment draw per sample, in sample order (the reference draws inside
        ``__getitem__``, once per sample), the same ops for all of the sample's views."""
        from .randaugment import apply_ops
        per_frame = [None] * int(frames.shape[0])
        for b in range(row_idx.shape[0]):
            self.augmentation.randomize_ops(self.resolution)
            ops, self.augmentation.cur_ops = self.augmentation.cur_ops, None
            for r in row_idx[b].tolist():
                if r >= 0:
                    per_frame[r] = ops
        return apply_ops(frames, per_frame, self.augmentation._fill())

    def tta(self, events, n_events=None):
        """The four views of _load_tta_data (event2img.py:94-112): identity, h-flip, t-flip,
        h+t-flip, as a list of batches in that order."""
        if isinstance(events, (list, tuple)):
            events, n_events = self._concat(events, _lib.require_gpu())
        starts = None
        if self.filters:                  # once, on the stored rows: the four views are views of the same survivors
            events, n_events, starts = self.filter(events, n_events)
        return [self(events, n_events, hflip=h, tflip=t, starts=starts, filtered=True)
                for h, t in ((False, False), (True, False), (False, True), (True, True))]


def build_event2img_pipeline(params, resolution, max_n, clip_model=None):
    """Counterpart of build_event2img_dataset (event2img.py:148-156) for the device path."""
    kw = {}
    n_px = 224
    if clip_model is not None:
        c = clip_model.cfg
        n_px = c['image_size']
        if 'patch' in c:
            kw = dict(patch=c['patch'], kpad=clip_model.kpad, dtype=clip_model.compute_dtype)
        else:                       # ResNet tower: uint8 frames for its stem kernel
            kw = dict(frames_u8=True)
    return Event2ImagePipeline(resolution, max_n, params.quantize_args, n_px=n_px, **kw)


class _FeederClosed(Exception):
    """raised inside the producer thread when the feeder is closed while it waits for a slot"""


class HostFeeder:
    """Batches that start in HOST memory, overlapped with the GPU's work on the batch before.

    The reference hides its CPU event -> image work behind the GPU with DataLoader worker processes
    (/root/reference/test.py:36-38, ``num_workers`` 8 / 16 in configs/zsclip/*.py:15) and then uploads fp32 images
    with a synchronous ``.cuda()`` (test.py:60).  Here the image work is on the GPU and what is left for the host
    is moving the raw events; ``Event2ImagePipeline.__call__`` on a list of arrays does that with one
    single-threaded ``np.concatenate`` and a pageable, synchronous copy.  This class does it the way a loader
    would:

      * a ring of ``depth`` pinned staging buffers and as many device buffers, all allocated once;
      * a producer thread takes the next batch from the iterable, copies every sample into the staging buffer at
        its offset with a small thread pool (torch's CPU copy releases the GIL), and issues ONE asynchronous
        host-to-device copy on a copy stream, followed by an event;
      * ``__next__`` makes the caller's stream wait for that event, runs the pipeline on the device buffer, and
        records on the caller's stream the event after which the producer may overwrite the slot.

    Samples: float32 [n_i, 4] rows (16 B per event, as the dataset readers store them) or packed uint64 [n_i]
    (8 B per event, ``vis.pack_events``) -- whatever the batch holds is uploaded as it is.  The batches are
    bit-identical to ``pipe(list_of_arrays)``.
    """

    CLOSE_WAIT_S = 5.0      # how long close() waits for the producer thread

    def __init__(self, pipe, batches, depth=2, copy_threads=8, capacity_bytes=None, **call_kw):
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor
        self.pipe, self.call_kw = pipe, call_kw
        self.dev = _lib.require_gpu()
        self.depth = max(2, int(depth))
        self.capacity = capacity_bytes
        self._slots = None
        self._pool = ThreadPoolExecutor(max(1, int(copy_threads)))
        self._copy_stream = torch.cuda.Stream(device=self.dev)
        self._ready = queue.Queue(maxsize=self.depth - 1)     # the producer runs at most depth - 1 batches ahead
        self._free = queue.Queue()
        self._batches = iter(batches)
        self._err = None
        self._stop = threading.Event()
        self._closed = False
        # The producer holds a WEAK reference to the feeder (and the queues / stop flag themselves): a feeder the
        # consumer simply drops is collected, its __del__ closes it, and the thread ends -- with a bound method as the
        # target the thread kept the feeder, its pinned and device rings alive for ever (advisor, round 4)
        import weakref
        self._th = threading.Thread(target=HostFeeder._produce, daemon=True,
                                    args=(weakref.ref(self), self._batches, self._ready, self._free, self._stop))
        self._th.start()

    # ---- life time -----------------------------------------------------------------------------------
    def close(self):
        """Stop the producer and release the pinned / device rings and the copy pool.  Called when the iteration
        ends; call it (or use the feeder as a context manager) when the consumer leaves the loop early."""
        if self._closed:
            return
        self._closed = True
        self._stop.set()
        # the producer may be blocked handing a batch over or waiting for a free slot: make room for both.  Bounded:
        # a producer stuck inside the USER's iterator (a loader that never yields again) cannot be woken from here --
        # after CLOSE_WAIT_S the daemon thread is left behind rather than hanging the caller (harness.evaluate calls
        # this from a `finally`, where a hang would hide the exception that got it there)
        import queue
        import threading
        import time
        deadline = time.monotonic() + self.CLOSE_WAIT_S
        # (a feeder whose last reference the producer itself dropped is finalised ON the producer thread: nothing to join)
        while self._th.is_alive() and time.monotonic() < deadline and threading.current_thread() is not self._th:
            try:
                while True:
                    self._ready.get_nowait()
            except queue.Empty:
                pass
            self._free.put(-1)
            self._th.join(timeout=0.05)
        self._pool.shutdown(wait=False)
        # Batches the producer staged but the consumer never took still have their host-to-device copy in flight on the
        # copy stream, into device buffers that were allocated on another stream: the ring may only be released (the
        # caching allocator may hand the blocks to anyone) once the copy engine is done with them, and the kernels
        # that read the consumed ones too
        self._copy_stream.synchronize()
        if self._slots is not None:
            for sl in self._slots:
                if sl['consumed'] is not None:
                    sl['consumed'].synchronize()
        if not self._th.is_alive():
            self._slots = None      # (a producer that is still alive keeps its ring: it may yet write into it)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass

    # ---- producer side -------------------------------------------------------------------------------
    def _alloc(self, nbytes):
        cap = max(int(nbytes), int(self.capacity or 0))
        cap = (cap + (1 << 20) - 1) >> 20 << 20
        self._slots = []
        for i in range(self.depth):
            host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            devb = torch.empty(cap, dtype=torch.uint8, device=self.dev)
            self._slots.append(dict(host=host, dev=devb, consumed=None))
            self._free.put(i)
        self.capacity = cap

    def _parse(self, samples):
        """host-side part of staging a batch: contiguous per-sample arrays, their sizes, the ring allocated for them"""
        host = [e.cpu() if torch.is_tensor(e) else e for e in samples]
        packed = all(not isinstance(e, dict) and vis.is_packed(e) for e in host)
        if packed:
            arrs = [np.ascontiguousarray(np.asarray(e).view(np.int64)) for e in host]
        else:
            arrs = [vis.parse_events(e) for e in host]          # float32 [n, 4], contiguous (no copy if it already is)
        n_events = [int(a.shape[0]) for a in arrs]
        esz = 8 if packed else 16
        total = sum(n_events) * esz
        if self._slots is None:
            self._alloc(total)
        # (a batch larger than the ring: the producer collects every slot -- waiting on the queues alone, without a
        # reference to the feeder -- and then calls _regrow)
        return dict(arrs=arrs, n_events=n_events, esz=esz, total=total, packed=packed)

    def _regrow(self, total, held):
        """a batch larger than any before it (pass capacity_bytes= to avoid this): every slot index is in `held`, i.e.
        no batch is staged or being consumed; wait for the kernels that read the slots, then allocate the ring again"""
        assert len(held) == self.depth
        for j in held:
            if self._slots[j]['consumed'] is not None:
                self._slots[j]['consumed'].synchronize()
        self._copy_stream.synchronize()
        self._slots = None
        self._alloc(total + total // 4)

    def _fill(self, prep, i):
        """copy the parsed batch into slot i's pinned buffer and issue its upload"""
        arrs, n_events, esz, total, packed = prep['arrs'], prep['n_events'], prep['esz'], prep['total'], prep['packed']
        slot = self._slots[i]
        if slot['consumed'] is not None:
            slot['consumed'].synchronize()        # the kernels that read this slot's device buffer are done
        offs = np.concatenate([[0], np.cumsum(n_events)]) * esz

        def put(j):
            src = torch.from_numpy(arrs[j].reshape(-1).view(np.uint8))
            slot['host'][int(offs[j]):int(offs[j + 1])].copy_(src)
        list(self._pool.map(put, range(len(arrs))))
        with torch.cuda.stream(self._copy_stream):
            slot['dev'][:total].copy_(slot['host'][:total], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._copy_stream)
        return dict(slot=i, total=total, packed=packed, n_events=n_events, done=done)

    @staticmethod
    def _produce(ref, batches, ready, free, stop):
        """Producer thread.  Holds the feeder only while it works on a batch; every wait (for the user's iterator, for a
        free slot, for room in the ready queue) runs on the queues and the stop flag alone."""
        import queue

        def alive():
            return not stop.is_set() and ref() is not None

        def put(item):          # queue.put that gives up when the feeder is closed or gone (-> False)
            while alive():
                try:
                    ready.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        def take_free():
            while alive():
                try:
                    i = free.get(timeout=0.1)
                except queue.Empty:
                    continue
                if i < 0:
                    break
                return i
            raise _FeederClosed()

        err = None
        try:
            dev_set = False
            for samples in batches:
                if not alive():
                    break
                feeder = ref()
                if feeder is None:
                    break
                if not dev_set:
                    torch.cuda.set_device(feeder.dev)
                    dev_set = True
                extra = None
                if isinstance(samples, dict):               # harness-style data_dict: events + anything else
                    if 'events' not in samples:
                        # a batch that is model-ready already (the reference's img / valid_mask): handed on as it is
                        del feeder
                        if not put(dict(passthrough=samples)):
                            break
                        continue
                    extra = {k: v for k, v in samples.items() if k != 'events'}
                    samples = samples['events']
                if torch.is_tensor(samples) or isinstance(samples, np.ndarray):
                    raise TypeError('HostFeeder: a batch is a LIST of per-sample event arrays (or a dict with such a '
                                    "list under 'events'); got a single array / tensor")
                prep = feeder._parse(samples)
                regrow, depth = prep['total'] > feeder.capacity, feeder.depth
                del feeder
                if regrow:
                    # the wait for ALL slots runs here, on the queue and the stop flag, with no reference to the feeder
                    # held: a consumer that drops the feeder meanwhile ends this thread (advisor, round 5 -- the wait used
                    # to sit in _parse, under a strong reference and without a timeout)
                    held = [take_free() for _ in range(depth)]
                    feeder = ref()
                    if feeder is None:
                        break
                    feeder._regrow(prep['total'], held)
                    del feeder
                i = take_free()
                feeder = ref()
                if feeder is None:
                    break
                item = feeder._fill(prep, i)
                del feeder
                item['extra'] = extra
                if not put(item):
                    break
        except _FeederClosed:
            pass
        except BaseException as e:   # noqa: BLE001 -- handed to the consumer
            err = e
        finally:
            feeder = ref()
            if feeder is not None:
                feeder._err = err
                del feeder
            put(None)

    # ---- consumer side -------------------------------------------------------------------------------
    def __iter__(self):
        return self

    def __next__(self):
        if self._closed:
            raise StopIteration
        item = self._ready.get()
        if item is None:
            err = self._err
            self.close()
            if err is not None:
                raise err
            raise StopIteration
        if 'passthrough' in item:
            return item['passthrough']
        slot = self._slots[item['slot']]
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(item['done'])
        buf = slot['dev'][:item['total']]
        events = buf.view(torch.int64) if item['packed'] else buf.view(torch.float32).view(-1, 4)
        out = self.pipe(events, item['n_events'], **self.call_kw)
        consumed = torch.cuda.Event()
        consumed.record(cur)
        slot['consumed'] = consumed
        self._free.put(item['slot'])
        if item['extra']:
            out.update(item['extra'])
        return out


def _stream(self, batches, depth=2, copy_threads=8, capacity_bytes=None, **call_kw):
    """Iterate over model-ready batches for an iterable of host-resident sample lists (or harness data_dicts
    with an ``events`` entry), the upload of batch i + 1 overlapped with whatever the GPU does for batch i."""
    return HostFeeder(self, batches, depth=depth, copy_threads=copy_threads, capacity_bytes=capacity_bytes, **call_kw)


Event2ImagePipeline.stream = _stream
