"""PyTorch-ROCm custom ops over the C ABI: the ``eventclip_hip::`` namespace.

north_star: "called from Python via PyTorch-ROCm custom ops so models/clip_cls.py's forward/classify
API is a drop-in".  Each op below is a ``torch.library.custom_op`` registered for CUDA (= HIP)
tensors only -- there is no CPU kernel, a CPU tensor raises -- whose body hands device pointers and
torch's current stream to one entry point of libeventclip_hip.so (include/eventclip_hip.h).  The
mirrors of the reference's interface (vis / preprocess / clip / adapter / clip_cls) call these:

    torch.ops.eventclip_hip.events_to_frames   ec_events_to_frames[_packed]    datasets/vis.py:75-117
    torch.ops.eventclip_hip.events_to_time_surface   ec_events_to_time_surface[_packed]   (no counterpart: eventclip_time_surface.h)
    torch.ops.eventclip_hip.events_to_voxel_grid     ec_events_to_voxel_grid[_packed]     (no counterpart: eventclip_voxel_grid.h)
    torch.ops.eventclip_hip.events_denoise           ec_denoise_events[_packed]           (no counterpart: eventclip_denoise.h)
    torch.ops.eventclip_hip.events_refractory        ec_refractory_events[_packed]        (no counterpart: eventclip_refractory.h)
    torch.ops.eventclip_hip.events_time_windows      ec_time_windows[_packed]             (no counterpart: eventclip_time_windows.h)
    torch.ops.eventclip_hip.preprocess         ec_preprocess                   datasets/event2img.py:119-122
    torch.ops.eventclip_hip.vit_encode         ec_vit_encode                   models/clip_cls.py:101
    torch.ops.eventclip_hip.text_encode        ec_text_encode                  models/clip_cls.py:84
    torch.ops.eventclip_hip.adapter_fwd        ec_adapter_forward              models/adapter.py:82-105
    torch.ops.eventclip_hip.classify           ec_classify_v2                   models/clip_cls.py:139-154, :319-343
    torch.ops.eventclip_hip.classify_bwd       ec_classify_backward            its vector-Jacobian product (loss.backward())
    torch.ops.eventclip_hip.adapter_train_fwd  ec_adapter_train_forward        models/adapter.py:82-105 in train mode
    torch.ops.eventclip_hip.adapter_train_bwd  ec_adapter_train_backward       its backward, over the forward's tape
    torch.ops.eventclip_hip.resnet_encode      ec_resnet_encode                models/clip_cls.py:101 (ResNet backbones)
    torch.ops.eventclip_hip.vit_train_fwd      ec_vit_train_forward            models/clip_cls_ft.py:196-243, the tower with a tape
    torch.ops.eventclip_hip.vit_train_bwd      ec_vit_train_backward_over      its backward, over the forward's tape
    torch.ops.eventclip_hip.vit_image_fwd      ec_patchify + ec_vit_train_forward   the same tower from the fp32 image
    torch.ops.eventclip_hip.vit_image_bwd      ec_vit_train_backward_image     its backward: d image and the parameter gradients

Weights live in packed C structs owned by the Python modules; an op receives them as an integer
handle into a registry of live modules (tensors-only signatures keep the ops traceable, and the
registered fake kernels give their output shapes without touching the device).

``classify``, ``adapter_train_fwd``, ``vit_train_fwd`` and ``vit_image_fwd`` carry autograd formulas (``torch.library.register_autograd``)
whose backward passes are the ``*_bwd`` ops, so ``loss.backward()`` reaches ``text_feats``, the adapter's parameters and
the vision tower's, which ``adapter_train_fwd`` / ``vit_train_fwd`` take as real tensor inputs.  The ``*_bwd`` ops have no formula of their own: there is no double
backward, and asking for one raises.
"""
import ctypes
import weakref
from typing import List, Optional, Tuple

import torch
from torch.library import custom_op

from . import _lib
from .adapter import _adapter_struct, adapter_param_names

NAMESPACE = 'eventclip_hip'

# ---- handles: id -> weak reference to the module that owns the packed weights ----
_handles = weakref.WeakValueDictionary()


def handle_of(module):
    """Integer handle of a module with packed weights (CLIP, TransformerAdapter)."""
    h = id(module)
    _handles[h] = module
    return h


def _resolve(handle, what):
    m = _handles.get(int(handle))
    if m is None:
        raise RuntimeError(f'{NAMESPACE}::{what}: handle {handle} does not name a live module')
    return m


def _plans():
    from . import preprocess
    return preprocess


# ------------------------------------------------------------------------------------------
# events -> frames
# ------------------------------------------------------------------------------------------
@custom_op(f'{NAMESPACE}::events_to_frames', mutates_args=(), device_types='cuda')
def events_to_frames(events: torch.Tensor, frame_range: torch.Tensor, H: int, W: int, thresh: float,
                     red: List[int], blue: List[int], count_non_zero: bool, background_mask: bool,
                     max_frame_events: int, flip_x: bool, negate_p: bool, float32_stage: bool,
                     total_events: int) -> torch.Tensor:
    """events float32 [n, 4] or packed int64 [n]; frame_range int64 [F, 2] -> uint8 [F, H, W, 3]."""
    from . import vis
    F = int(frame_range.shape[0])
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=events.device)
    prm = vis.events_params((H, W), red, blue, thresh, count_non_zero, background_mask, max_frame_events, flip_x,
                            negate_p, float32_stage, total_events)
    vis.attach_sort_workspace(prm, events.device, True)
    _lib.launch('ec_events_to_frames_packed' if vis.is_packed(events) else 'ec_events_to_frames', events, frame_range,
                F, prm, frames, None, None, None)
    return frames


@events_to_frames.register_fake
def _(events, frame_range, H, W, thresh, red, blue, count_non_zero, background_mask, max_frame_events,
      flip_x, negate_p, float32_stage, total_events):
    return events.new_empty((frame_range.shape[0], H, W, 3), dtype=torch.uint8)


@custom_op(f'{NAMESPACE}::events_to_time_surface', mutates_args=(), device_types='cuda')
def events_to_time_surface(events: torch.Tensor, frame_range: torch.Tensor, H: int, W: int, decay: str, tau: float,
                           red: List[int], blue: List[int], background_mask: bool, max_frame_events: int,
                           flip_x: bool, negate_p: bool, reverse_t: bool, total_events: int) -> torch.Tensor:
    """events float32 [n, 4] or packed int64 [n]; frame_range int64 [F, 2] -> uint8 [F, H, W, 3]: the latest-timestamp
    frames of include/eventclip_time_surface.h, decay 'linear' or 'exp', tau in seconds."""
    from . import vis
    F = int(frame_range.shape[0])
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=events.device)
    prm = vis.time_surface_params((H, W), red, blue, decay, tau, background_mask, max_frame_events, flip_x, negate_p,
                                  reverse_t, total_events)
    _lib.launch('ec_events_to_time_surface_packed' if vis.is_packed(events) else 'ec_events_to_time_surface', events,
                frame_range, F, prm, frames, None, None)
    return frames


@events_to_time_surface.register_fake
def _(events, frame_range, H, W, decay, tau, red, blue, background_mask, max_frame_events, flip_x, negate_p,
      reverse_t, total_events):
    return events.new_empty((frame_range.shape[0], H, W, 3), dtype=torch.uint8)


@custom_op(f'{NAMESPACE}::events_to_voxel_grid', mutates_args=(), device_types='cuda')
def events_to_voxel_grid(events: torch.Tensor, frame_range: torch.Tensor, H: int, W: int, bins: int,
                         background_mask: bool, max_frame_events: int, flip_x: bool, negate_p: bool, reverse_t: bool,
                         total_events: int) -> torch.Tensor:
    """events float32 [n, 4] or packed int64 [n]; frame_range int64 [F, 2] -> uint8 [F, H, W, 3]: the temporal-bin
    frames of include/eventclip_voxel_grid.h (bins == 3).  A sensor of more than one row band is coloured from its grid,
    which lives in a temporary of torch's allocator for the length of the call."""
    from . import vis
    F = int(frame_range.shape[0])
    prm = vis.voxel_grid_params((H, W), bins, background_mask, max_frame_events, flip_x, negate_p, reverse_t, total_events)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=events.device)
    grid = None
    if vis.voxel_grid_bands((H, W), bins) > 1:
        grid = torch.empty((F, H, W, bins), dtype=torch.int32, device=events.device)
    _lib.launch('ec_events_to_voxel_grid_packed' if vis.is_packed(events) else 'ec_events_to_voxel_grid', events,
                frame_range, F, prm, frames, grid, None)
    return frames


@events_to_voxel_grid.register_fake
def _(events, frame_range, H, W, bins, background_mask, max_frame_events, flip_x, negate_p, reverse_t, total_events):
    return events.new_empty((frame_range.shape[0], H, W, 3), dtype=torch.uint8)


@custom_op(f'{NAMESPACE}::events_denoise', mutates_args=(), device_types='cuda')
def events_denoise(events: torch.Tensor, sample_range: torch.Tensor, H: int, W: int, dt_us: int,
                   radius: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """events float32 [n, 4] or packed int64 [n]; sample_range int64 [B, 2] -> (events_out like events, counts int64 [B]):
    the background-activity filter of include/eventclip_denoise.h.  The survivors of sample b are
    events_out[begin_b : begin_b + counts[b]]; the rows behind them, and rows outside every sample, are zero.  The
    longest sample sizes the workspace, so the ranges are read back once."""
    from . import vis
    B = int(sample_range.shape[0])
    host = sample_range.cpu()
    lengths = host[:, 1] - host[:, 0]
    prm = vis.denoise_params((H, W), dt_us, radius, int(lengths.max()) if B else 1, int(lengths.sum()) if B else 0)
    events_out = torch.zeros_like(events)
    counts = torch.zeros((B,), dtype=torch.int64, device=events.device)
    vis.denoise_launch(events, sample_range.contiguous(), prm, events_out, counts)
    return events_out, counts


@events_denoise.register_fake
def _(events, sample_range, H, W, dt_us, radius):
    return torch.empty_like(events), events.new_empty((sample_range.shape[0],), dtype=torch.int64)


@custom_op(f'{NAMESPACE}::events_refractory', mutates_args=(), device_types='cuda')
def events_refractory(events: torch.Tensor, sample_range: torch.Tensor, H: int, W: int, period_us: int,
                      per_polarity: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """events float32 [n, 4] or packed int64 [n]; sample_range int64 [B, 2] -> (events_out like events, counts int64 [B]):
    the refractory-period filter of include/eventclip_refractory.h.  The survivors of sample b are
    events_out[begin_b : begin_b + counts[b]]; the rows behind them, and rows outside every sample, are zero.  The
    longest sample sizes the workspace, so the ranges are read back once."""
    from . import vis
    B = int(sample_range.shape[0])
    host = sample_range.cpu()
    lengths = host[:, 1] - host[:, 0]
    prm = vis.refractory_params((H, W), period_us, per_polarity, int(lengths.max()) if B else 1, int(lengths.sum()) if B else 0)
    events_out = torch.zeros_like(events)
    counts = torch.zeros((B,), dtype=torch.int64, device=events.device)
    vis.refractory_launch(events, sample_range.contiguous(), prm, events_out, counts)
    return events_out, counts


@events_refractory.register_fake
def _(events, sample_range, H, W, period_us, per_polarity):
    return torch.empty_like(events), events.new_empty((sample_range.shape[0],), dtype=torch.int64)


@custom_op(f'{NAMESPACE}::events_time_windows', mutates_args=(), device_types='cuda')
def events_time_windows(events: torch.Tensor, sample_range: torch.Tensor, dt_us: int, stride_us: int, max_windows: int,
                        from_last: bool, total_events: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """events float32 [n, 4] or packed int64 [n]; sample_range int64 [B, 2] -> (bounds int64 [B, max_windows, 2], stats int32
    [B, 4]): the fixed-duration windows of include/eventclip_time_windows.h.  bounds[b, k] are the (begin, end) event rows of
    window k of sample b, -1 in the rows the kernel does not write; stats[b] are the four words of ec_time_windows_stats
    (t_first, t_last, unsorted, windows).  Nothing is read back: total_events (0 = unknown) only sizes the grid."""
    from . import vis
    B = int(sample_range.shape[0])
    prm = vis.time_windows_params(dt_us, stride_us, max_windows, from_last, total_events)
    bounds = torch.full((B, max_windows, 2), -1, dtype=torch.int64, device=events.device)
    stats = torch.zeros((B, 4), dtype=torch.int32, device=events.device)
    _lib.launch('ec_time_windows_packed' if vis.is_packed(events) else 'ec_time_windows', events, sample_range.contiguous(), B,
                prm, bounds, stats)
    return bounds, stats


@events_time_windows.register_fake
def _(events, sample_range, dt_us, stride_us, max_windows, from_last, total_events):
    B = sample_range.shape[0]
    return events.new_empty((B, max_windows, 2), dtype=torch.int64), events.new_empty((B, 4), dtype=torch.int32)


# ------------------------------------------------------------------------------------------
# CLIP preprocess
# ------------------------------------------------------------------------------------------
@custom_op(f'{NAMESPACE}::preprocess', mutates_args=(), device_types='cuda')
def preprocess(frames: torch.Tensor, n_px: int, mode: int, patch: int, kpad: int,
               dtype_code: int) -> torch.Tensor:
    """frames uint8 [F, H, W, 3] -> fp32 [F, 3, R, R] (mode EC_PRE_CHW_F32), 16-bit patch rows
    [F, G, kpad] (EC_PRE_PATCHES16) or uint8 [F, R, R, 3] (EC_PRE_HWC_U8)."""
    F, H, W, _ = frames.shape
    host, plan = _plans()._plan(H, W, n_px, frames.device)
    out = frames.new_empty(_pre_shape(F, n_px, mode, patch, kpad), dtype=_pre_dtype(mode, dtype_code))
    _lib.launch('ec_preprocess', frames, F, host.ctypes.data, plan, out, mode, max(patch, 1), kpad, dtype_code)
    return out


def _pre_shape(F, n_px, mode, patch, kpad):
    if mode == _lib.EC_PRE_CHW_F32:
        return (F, 3, n_px, n_px)
    if mode == _lib.EC_PRE_HWC_U8:
        return (F, n_px, n_px, 3)
    return (F, (n_px // patch) ** 2, kpad)


def _pre_dtype(mode, dtype_code):
    if mode == _lib.EC_PRE_CHW_F32:
        return torch.float32
    if mode == _lib.EC_PRE_HWC_U8:
        return torch.uint8
    return torch.float16 if dtype_code == _lib.EC_F16 else torch.bfloat16


@preprocess.register_fake
def _(frames, n_px, mode, patch, kpad, dtype_code):
    return frames.new_empty(_pre_shape(frames.shape[0], n_px, mode, patch, kpad),
                            dtype=_pre_dtype(mode, dtype_code))


# ------------------------------------------------------------------------------------------
# towers
# ------------------------------------------------------------------------------------------
@custom_op(f'{NAMESPACE}::vit_encode', mutates_args=(), device_types='cuda')
def vit_encode(patches: torch.Tensor, clip_handle: int) -> torch.Tensor:
    """patches 16-bit [N, G, kpad] (EC_PRE_PATCHES16 layout) -> fp32 features [N, D]."""
    m = _resolve(clip_handle, 'vit_encode')
    pk = m._pack()
    n = int(patches.shape[0])
    feats = torch.empty((n, m.cfg['embed_dim']), dtype=torch.float32, device=patches.device)
    if n == 0:
        return feats
    chunk = max(1, min(m.chunk, n))
    need = _lib.lib().ec_vit_workspace_bytes(ctypes.byref(pk['vit']), chunk)
    if need > m.workspace_budget:     # keep the scratch bounded (e.g. 336-px inputs)
        chunk = max(1, int(chunk * m.workspace_budget / need))
        need = _lib.lib().ec_vit_workspace_bytes(ctypes.byref(pk['vit']), chunk)
    ws = m._ws.get(need, pk['dev'])
    _lib.launch('ec_vit_encode', pk['vit'], patches, n, feats, ws, ws.numel(), chunk)
    return feats


@vit_encode.register_fake
def _(patches, clip_handle):
    return patches.new_empty((patches.shape[0], _resolve(clip_handle, 'vit_encode').cfg['embed_dim']),
                             dtype=torch.float32)


@custom_op(f'{NAMESPACE}::text_encode', mutates_args=(), device_types='cuda')
def text_encode(tokens: torch.Tensor, clip_handle: int) -> torch.Tensor:
    """tokens int32 [K, ctx] -> fp32 [K, D] (not normalised)."""
    m = _resolve(clip_handle, 'text_encode')
    pk = m._pack()
    n = int(tokens.shape[0])
    feats = torch.empty((n, m.cfg['embed_dim']), dtype=torch.float32, device=tokens.device)
    if n == 0:
        return feats
    chunk = max(1, min(512, n))
    need = _lib.lib().ec_text_workspace_bytes(ctypes.byref(pk['text']), chunk)
    ws = m._ws.get(need, pk['dev'])
    _lib.launch('ec_text_encode', pk['text'], tokens, n, feats, ws, ws.numel(), chunk)
    return feats


@text_encode.register_fake
def _(tokens, clip_handle):
    return tokens.new_empty((tokens.shape[0], _resolve(clip_handle, 'text_encode').cfg['embed_dim']),
                            dtype=torch.float32)


# ------------------------------------------------------------------------------------------
# adapter, classifier tail
# ------------------------------------------------------------------------------------------
@custom_op(f'{NAMESPACE}::adapter_fwd', mutates_args=(), device_types='cuda')
def adapter_fwd(feats: torch.Tensor, row_idx: torch.Tensor, adapter_handle: int) -> torch.Tensor:
    """feats fp32 [Nv, C] (compact valid views), row_idx int32 [B, T] (-1 = padded) -> [B, T, C]."""
    a = _resolve(adapter_handle, 'adapter_fwd')
    pk = a._pack()
    B, T = row_idx.shape
    out = torch.empty((B, T, a.in_dim), dtype=torch.float32, device=feats.device)
    _lib.launch('ec_adapter_forward', pk['w'], feats, row_idx, B, T, out)
    return out


@adapter_fwd.register_fake
def _(feats, row_idx, adapter_handle):
    return feats.new_empty((row_idx.shape[0], row_idx.shape[1], feats.shape[-1]))


# prepared text planes of ec_classify_prep_text, keyed on the identity and version of the text_t tensor: the text
# features are constant across batches (cached prompts) or change once per optimiser step (learned parameter, a new
# tensor each time: clip_cls.FSCLIPClassifier._text_transposed), so the transposed hi + lo planes are built once
_TEXT_PLANES = {}
_TEXT_PLANES_MAX = 8


def _text_planes(text_t):
    C, K = text_t.shape
    key = (text_t.data_ptr(), text_t._version, C, K, text_t.device.index)
    hit = _TEXT_PLANES.get(key)
    if hit is not None and hit[1]() is text_t:
        return hit[0]
    ws = _lib.scratch(_lib.lib().ec_classify_text_bytes(C, K), text_t.device)
    _lib.launch('ec_classify_prep_text', text_t, C, K, ws, ws.numel())
    for k in [k for k, v in _TEXT_PLANES.items() if v[1]() is None]:        # tensors that are gone
        del _TEXT_PLANES[k]
    while len(_TEXT_PLANES) >= _TEXT_PLANES_MAX:
        del _TEXT_PLANES[next(iter(_TEXT_PLANES))]
    _TEXT_PLANES[key] = (ws, weakref.ref(text_t))
    return ws


@custom_op(f'{NAMESPACE}::classify', mutates_args=(), device_types='cuda')
def classify(feats: torch.Tensor, row_idx: torch.Tensor, text_t: torch.Tensor, logit_scale: float,
             agg: int, normalize: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """feats fp32 [Nv, C], row_idx int32 [B, T], text_t fp32 [C, K] -> (full_logits [B, T, K],
    logits [B, K], probs [B, K])."""
    B, T = row_idx.shape
    C, K = text_t.shape
    full = torch.empty((B, T, K), dtype=torch.float32, device=feats.device)
    logits = torch.empty((B, K), dtype=torch.float32, device=feats.device)
    probs = torch.empty((B, K), dtype=torch.float32, device=feats.device)
    n_rows = int(feats.shape[0])
    text_ws = _text_planes(text_t)
    ws = _lib.scratch(_lib.lib().ec_classify_v2_workspace_bytes(n_rows, C, K), feats.device)
    _lib.launch('ec_classify_v2', feats, n_rows, row_idx, text_ws, B, T, C, K, logit_scale, agg, int(normalize), full,
                logits, probs, ws, ws.numel())
    return full, logits, probs


@classify.register_fake
def _(feats, row_idx, text_t, logit_scale, agg, normalize):
    B, T = row_idx.shape
    K = text_t.shape[1]
    return feats.new_empty((B, T, K)), feats.new_empty((B, K)), feats.new_empty((B, K))


def _f32c(t):
    return None if t is None else t.float().contiguous()


@custom_op(f'{NAMESPACE}::classify_bwd', mutates_args=(), device_types='cuda')
def classify_bwd(feats: torch.Tensor, row_idx: torch.Tensor, text_t: torch.Tensor, full_logits: torch.Tensor,
                 d_full_logits: Optional[torch.Tensor], d_logits: Optional[torch.Tensor], d_probs: Optional[torch.Tensor],
                 logit_scale: float, agg: int, normalize: bool, need_feats: bool,
                 need_text: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The vector-Jacobian product of ``classify``: (d_feats [Nv, C], d_text_t [C, K]); an upstream gradient that is
    None is zero, a gradient that is not needed comes back as an empty tensor and costs no launch."""
    B, T = row_idx.shape
    C, K = text_t.shape
    n_rows = int(feats.shape[0])
    feats, text_t, full_logits = _f32c(feats), _f32c(text_t), _f32c(full_logits)
    row_idx = row_idx.contiguous()
    ups = [_f32c(g) for g in (d_full_logits, d_logits, d_probs)]
    d_feats = torch.empty((n_rows, C) if need_feats else (0,), dtype=torch.float32, device=feats.device)
    d_text = torch.empty((C, K) if need_text else (0,), dtype=torch.float32, device=feats.device)
    ws = _lib.scratch(_lib.lib().ec_classify_backward_workspace_bytes(B, T, C, K), feats.device)
    _lib.launch('ec_classify_backward', feats, n_rows, row_idx, text_t, B, T, C, K, logit_scale, agg, int(normalize),
                full_logits, *ups, d_feats if need_feats else None, d_text if need_text else None, ws, ws.numel())
    return d_feats, d_text


@classify_bwd.register_fake
def _(feats, row_idx, text_t, full_logits, d_full_logits, d_logits, d_probs, logit_scale, agg, normalize, need_feats,
      need_text):
    return (feats.new_empty(tuple(feats.shape) if need_feats else (0,), dtype=torch.float32),
            feats.new_empty(tuple(text_t.shape) if need_text else (0,), dtype=torch.float32))


def _classify_setup(ctx, inputs, output):
    feats, row_idx, text_t, logit_scale, agg, normalize = inputs
    ctx.save_for_backward(feats, row_idx, text_t, output[0])
    ctx.tail = (logit_scale, agg, normalize)
    ctx.set_materialize_grads(False)          # an output the loss does not use sends None, not a tensor of zeros


def _classify_backward(ctx, d_full_logits, d_logits, d_probs):
    feats, row_idx, text_t, full_logits = ctx.saved_tensors
    need_feats, need_text = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
    d_feats, d_text = torch.ops.eventclip_hip.classify_bwd(feats, row_idx, text_t, full_logits, d_full_logits, d_logits,
                                                           d_probs, *ctx.tail, need_feats, need_text)
    return d_feats if need_feats else None, None, d_text if need_text else None, None, None, None


classify.register_autograd(_classify_backward, setup_context=_classify_setup)


# ---- the transformer adapter under autograd: forward and backward as two ops with a tape between them ----
def _train_struct(params, *geometry):
    """_adapter_struct over an op's ``params`` list (geometry: in_dim, d_model, heads, ffn_dim, layers, residual,
    post_norm)."""
    want = len(adapter_param_names(geometry[4]))
    if len(params) != want:
        raise RuntimeError(f'{NAMESPACE}: {len(params)} adapter parameters, {want} expected (named_parameters() order)')
    return _adapter_struct(params, *geometry)


@custom_op(f'{NAMESPACE}::adapter_train_fwd', mutates_args=(), device_types='cuda')
def adapter_train_fwd(feats: torch.Tensor, row_idx: torch.Tensor, params: List[torch.Tensor], d_model: int, heads: int,
                      ffn_dim: int, layers: int, residual: float, dropout_p: float,
                      seed: int, post_norm: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """feats fp32 [B * T, C] with zero rows on invalid views, row_idx int32 [B, T] (< 0 = invalid view), params the
    adapter's parameters in ``adapter_param_names`` order -> (out [B, T, C], the residual mix of adapter.py:22-25;
    tape uint8 [n]: the saved activations ``adapter_train_bwd`` reads).  post_norm: 0 the pre-LN encoder layer
    (norm_first=True), 1 the post-LN one; the tape has the same size for both."""
    B, T = row_idx.shape
    C = int(feats.shape[-1])
    if tuple(feats.shape) != (B * T, C):
        raise RuntimeError(f'{NAMESPACE}::adapter_train_fwd: feats {tuple(feats.shape)} is not [B * T = {B * T}, C]')
    feats = _f32c(feats)
    params = [_f32c(p) for p in params]
    w, keep = _train_struct(params, C, d_model, heads, ffn_dim, layers, residual, post_norm)   # noqa: F841 (the layer array)
    out = torch.empty((B, T, C), dtype=torch.float32, device=feats.device)
    need = int(_lib.lib().ec_adapter_train_tape_bytes(B, T, C, d_model, ffn_dim, heads, layers))
    tape = _lib.scratch(need, feats.device).zero_()       # its alignment gaps too: an output
    _lib.launch('ec_adapter_train_forward', feats, (row_idx >= 0).to(torch.uint8).contiguous(), B, T, w, dropout_p, seed,
                out, tape, tape.numel())
    return out, tape


def _tape_numel(B, T, C, d_model, heads, ffn_dim, layers):
    """ec_adapter_train_tape_bytes restated for the fake kernel (no library call while tracing)."""
    R, up = B * T, lambda n: (n * 4 + 255) // 256 * 256
    per_layer = 6 * up(R * d_model) + 2 * up(R) + up(R * 3 * d_model) + up(B * heads * T * T) + up(R * ffn_dim)
    return max(3 * up(R * d_model) + up(R * C) + layers * per_layer, 256)


@adapter_train_fwd.register_fake
def _(feats, row_idx, params, d_model, heads, ffn_dim, layers, residual, dropout_p, seed, post_norm=0):
    B, T = row_idx.shape
    C = feats.shape[-1]
    return (feats.new_empty((B, T, C), dtype=torch.float32),
            feats.new_empty((_tape_numel(B, T, C, d_model, heads, ffn_dim, layers),), dtype=torch.uint8))


_MASK_BITS = 62


def _join_mask(lo, hi):
    return int(lo) | (int(hi) << _MASK_BITS)


@custom_op(f'{NAMESPACE}::adapter_train_bwd', mutates_args=(), device_types='cuda')
def adapter_train_bwd(feats: torch.Tensor, row_idx: torch.Tensor, params: List[torch.Tensor], tape: torch.Tensor,
                      d_out: torch.Tensor, d_model: int, heads: int, ffn_dim: int, layers: int, residual: float,
                      dropout_p: float, seed: int, need_mask: int, post_norm: int = 0,
                      need_mask_hi: int = 0) -> List[torch.Tensor]:
    """The backward of ``adapter_train_fwd`` over its tape (only read: a second call gives the same bits); post_norm is
    the forward's.  need_mask holds bits 0 .. 61 of the mask below, need_mask_hi bits 62 and up (an adapter of more than 4
    layers has more tensors than a 64-bit argument has bits).  Returns
    len(params) + 1 tensors: the gradient of params[i] where bit i of need_mask is set, d_feats [B * T, C] where bit
    len(params) is set, an empty tensor (and no launch) otherwise."""
    B, T = row_idx.shape
    C = int(feats.shape[-1])
    feats, d_out = _f32c(feats), _f32c(d_out)
    params = [_f32c(p) for p in params]
    n = len(params)
    need_mask = _join_mask(need_mask, need_mask_hi)
    grads = [torch.empty_like(p) if need_mask >> i & 1 else None for i, p in enumerate(params)]
    d_feats = torch.empty_like(feats) if need_mask >> n & 1 else None
    geometry = (C, d_model, heads, ffn_dim, layers, residual, post_norm)
    w, keep_w = _train_struct(params, *geometry)      # noqa: F841 (the struct's layer array)
    g, keep_g = _train_struct(grads, *geometry)       # noqa: F841
    ws = _lib.scratch(_lib.lib().ec_adapter_train_backward_workspace_bytes(B, T, C, d_model, ffn_dim), feats.device)
    _lib.launch('ec_adapter_train_backward', feats, B, T, w, dropout_p, seed, tape, tape.numel(), d_out, g, d_feats, ws,
                ws.numel())
    empty = feats.new_empty((0,))
    return [empty.clone() if t is None else t for t in grads + [d_feats]]


@adapter_train_bwd.register_fake
def _(feats, row_idx, params, tape, d_out, d_model, heads, ffn_dim, layers, residual, dropout_p, seed, need_mask,
      post_norm=0, need_mask_hi=0):
    like = list(params) + [feats]
    need_mask = _join_mask(need_mask, need_mask_hi)
    return [feats.new_empty(tuple(t.shape) if need_mask >> i & 1 else (0,), dtype=torch.float32)
            for i, t in enumerate(like)]


def _adapter_setup(ctx, inputs, output):
    feats, row_idx, params = inputs[:3]
    ctx.save_for_backward(feats, row_idx, output[1], *params)
    ctx.tail = tuple(inputs[3:10])          # d_model .. seed
    ctx.post_norm = inputs[10]
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)


def _adapter_backward(ctx, d_out, d_tape):
    feats, row_idx, tape, *params = ctx.saved_tensors
    n = len(params)
    need = list(ctx.needs_input_grad[2]) + [ctx.needs_input_grad[0]]
    # one None per scalar argument the call carried: the dispatcher drops a trailing post_norm that equals its default
    tail = (None,) * (len(ctx.needs_input_grad) - 3)
    if d_out is None or not any(need):
        return (None, None, [None] * n) + tail
    mask = sum(1 << i for i, b in enumerate(need) if b)
    got = torch.ops.eventclip_hip.adapter_train_bwd(feats, row_idx, params, tape, d_out, *ctx.tail,
                                                    mask & ((1 << _MASK_BITS) - 1), ctx.post_norm, mask >> _MASK_BITS)
    grads = [t if b else None for t, b in zip(got, need)]
    return (grads[n], None, grads[:n]) + tail


adapter_train_fwd.register_autograd(_adapter_backward, setup_context=_adapter_setup)


@custom_op(f'{NAMESPACE}::resnet_encode', mutates_args=(), device_types='cuda')
def resnet_encode(inp: torch.Tensor, input_mode: int, clip_handle: int) -> torch.Tensor:
    """ResNet image tower: fp32 [N, 3, R, R] (EC_PRE_CHW_F32) or uint8 [N, R, R, 3] (EC_PRE_HWC_U8) -> fp32 [N, D].
    The model's mode travels in its packed weights (ec_resnet_weights.precise_blocks: the split-precision form, whose
    workspace ec_resnet_workspace_bytes sizes with the second plane)."""
    m = _resolve(clip_handle, 'resnet_encode')
    pk = m._pack()
    n = int(inp.shape[0])
    feats = torch.empty((n, m.cfg['embed_dim']), dtype=torch.float32, device=inp.device)
    if n == 0:
        return feats
    chunk = max(1, min(int(m.chunk), n))
    need = _lib.lib().ec_resnet_workspace_bytes(ctypes.byref(pk['resnet']), chunk)
    if need == 0:
        _lib.check(_lib.EC_ERR_INVALID, 'ec_resnet_workspace_bytes')
    ws = m._ws.get(need, pk['dev'])
    _lib.launch('ec_resnet_encode', pk['resnet'], inp, int(input_mode), n, feats, ws, ws.numel(), chunk)
    return feats


@resnet_encode.register_fake
def _(inp, input_mode, clip_handle):
    return inp.new_empty((inp.shape[0], _resolve(clip_handle, 'resnet_encode').cfg['embed_dim']), dtype=torch.float32)


# ---- the vision tower under autograd: forward and backward as two ops with a tape between them ----
def _tower_params(t, params, what):
    """-> (names of the masters among ``params``, keys of the LoRA factors among them): the fp32 masters of
    ``clip.visual`` that require grad in ``VisualTower.canonical()`` order, then the factors.  They are inputs so that
    autograd routes their gradients; the kernels read them where the tower bound them (and their operand copies)."""
    names = t.trainable()
    keys = list(t.lora.params) if t.lora is not None else []
    own = t.op_params()
    if len(params) != len(own):
        raise RuntimeError(f'{NAMESPACE}::{what}: {len(params)} parameters, {len(own)} expected (the trainable masters '
                           'in canonical() order, then the LoRA factors)')
    for i, (p, o) in enumerate(zip(params, own)):
        if p.shape != o.shape or p.dtype != o.dtype:
            raise RuntimeError(f'{NAMESPACE}::{what}: params[{i}] {tuple(p.shape)} is not the tower\'s '
                               f'{(names + keys)[i]} {tuple(o.shape)}')
    return names, keys


def _image_tape(t, n):
    """``vit_image_fwd``'s tape -> (bytes of the training workspace rounded to 256, bytes of the tape: the workspace, then
    the patch rows)"""
    ws = (t.workspace_bytes(n) + 255) // 256 * 256
    return ws, ws + n * t.G * t.kpad * 2


def _forward_begin(what, x, params, tower_handle, image):
    """The common start of ``vit_train_fwd`` (x: the patch rows) and ``vit_image_fwd`` (image: x is the fp32 image): the
    tower behind the handle with its operand copies up to date (``VisualTower.refresh``), x checked, this call's outputs.
    -> (tower, N, x contiguous, feats fp32 [N, D], the tape -- zeroed, its alignment gaps and scratch too: an output --,
    (bytes of the training workspace at its head, bytes in all: ``_image_tape``))"""
    t = _resolve(tower_handle, what)
    _tower_params(t, params, what)
    t.refresh()
    n, R = int(x.shape[0]), t.cfg['image_size']
    noun, dtype, row = ('image', torch.float32, (3, R, R)) if image else ('patches', t.cd, (t.G, t.kpad))
    if x.dtype != dtype or tuple(x.shape) != (n,) + row or n == 0:
        raise RuntimeError(f'{NAMESPACE}::{what}: {noun} {tuple(x.shape)} {x.dtype}, '
                           f'[N > 0, {", ".join(map(str, row))}] {dtype} expected')
    ws, total = _image_tape(t, n) if image else (t.workspace_bytes(n),) * 2
    feats = torch.empty((n, t.D), dtype=torch.float32, device=x.device)
    return t, n, x.contiguous(), feats, _lib.scratch(total, x.device).zero_(), (ws, total)


@custom_op(f'{NAMESPACE}::vit_train_fwd', mutates_args=(), device_types='cuda')
def vit_train_fwd(patches: torch.Tensor, params: List[torch.Tensor],
                  tower_handle: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """patches 16-bit [N, G, kpad], params the trainable tensors of the ``ft.VisualTower`` behind ``tower_handle``
    (``_tower_params``) -> (feats fp32 [N, D]; tape uint8 [ec_vit_train_workspace_bytes]: the saved activations
    ``vit_train_bwd`` reads, followed by the scratch of both passes).  The tape is this call's own, so several forwards
    may be alive at once.  Operand copies of masters or factors written since they were packed are rebuilt first
    (``VisualTower.refresh``).  ``patches`` is not differentiable: a gradient in its 16 bits would underflow, and a patch
    row carries every pixel twice (hi | lo).  The gradient with respect to the image is ``vit_image_fwd``'s, in fp32."""
    t, n, patches, feats, tape, _ = _forward_begin('vit_train_fwd', patches, params, tower_handle, image=False)
    _lib.launch('ec_vit_train_forward', t._vit, patches, n, feats, tape, tape.numel())
    return feats, tape


@vit_train_fwd.register_fake
def _(patches, params, tower_handle):
    t = _resolve(tower_handle, 'vit_train_fwd')
    n = patches.shape[0]
    return (patches.new_empty((n, t.D), dtype=torch.float32),
            patches.new_empty((max(t.workspace_bytes(n), 256),), dtype=torch.uint8))


def _tower_backward(t, what, params, need, patches, n, d_feats, tape, tape_bytes, need_image):
    """The backward pass behind ``vit_train_bwd`` and ``vit_image_bwd`` over the first ``tape_bytes`` of a forward's tape
    and its patch rows: ``ec_vit_train_backward_image`` with need_image, ``ec_vit_train_backward_over`` when only a
    parameter gradient is needed, no launch when nothing is.  -> [d image, the gradient of params[0], params[1], ...],
    every one a fresh allocation, an empty tensor for what is not needed."""
    names, keys = _tower_params(t, params, what)
    if len(need) != len(params):
        raise RuntimeError(f'{NAMESPACE}::{what}: need has {len(need)} entries for {len(params)} parameters')
    if n == 0 or tuple(d_feats.shape) != (n, t.D) or tape_bytes < t.workspace_bytes(n) or \
            patches.numel() * patches.element_size() < n * t.G * t.kpad * 2:
        raise RuntimeError(f'{NAMESPACE}::{what}: d_feats {tuple(d_feats.shape)} / tape of {tape.numel()} bytes do '
                           f'not belong to a forward over {n} images')
    d_feats, dev = _f32c(d_feats), d_feats.device
    grads = [torch.empty_like(p) if b else None for p, b in zip(params, need)]
    tower_grads = {k: g for k, g in zip(names, grads) if g is not None}
    factor_grads = {k: g for k, g in zip(keys, grads[len(names):]) if g is not None}
    # the kernels write both factors of a projection: the partner of a factor whose own gradient is not asked for gets a
    # buffer that is dropped
    for _, _, kd, ku in t.lora.projections() if factor_grads else ():
        for a, b in ((kd, ku), (ku, kd)):
            if a in factor_grads and b not in factor_grads:
                factor_grads[b] = torch.empty_like(t.lora.params[b])
    g, keep_g = t.grads_over(tower_grads)                                   # noqa: F841 (the struct's block array)
    lora, keep_l = t.lora.struct_for(factor_grads) if factor_grads else (None, None)   # noqa: F841
    d_image = None
    if need_image:
        R = t.cfg['image_size']
        d_image = torch.empty((n, 3, R, R), dtype=torch.float32, device=dev)
        scr = _lib.scratch(_lib.lib().ec_vit_train_backward_image_scratch_bytes(ctypes.byref(t._vit), n), dev)
        conv_t, conv_lo_t = t.conv_operands()
        _lib.launch('ec_vit_train_backward_image', t._vit, t._vit_t, patches, n, d_feats, g, lora, conv_t, conv_lo_t,
                    d_image, tape, tape_bytes, scr, scr.numel())
    elif tower_grads or factor_grads:
        scr = _lib.scratch(_lib.lib().ec_vit_train_backward_scratch_bytes(ctypes.byref(t._vit), n), dev)
        _lib.launch('ec_vit_train_backward_over', t._vit, t._vit_t, patches, n, d_feats, g, lora, tape, tape_bytes, scr,
                    scr.numel())
    return [d_feats.new_empty((0,), dtype=torch.float32) if x is None else x for x in [d_image] + grads]


@custom_op(f'{NAMESPACE}::vit_train_bwd', mutates_args=(), device_types='cuda')
def vit_train_bwd(patches: torch.Tensor, params: List[torch.Tensor], tape: torch.Tensor, d_feats: torch.Tensor,
                  tower_handle: int, need: List[bool]) -> List[torch.Tensor]:
    """The backward of ``vit_train_fwd`` over its tape: len(params) tensors, the gradient of params[i] where need[i], an
    empty tensor otherwise; the pass stops at the lowest block a needed gradient lives in.  Every gradient is a fresh
    allocation the caller owns.  The tape is only read (``ec_vit_train_backward_over``: the pass's scratch is this
    call's own), so a second call gives the same bits."""
    t = _resolve(tower_handle, 'vit_train_bwd')
    n = int(patches.shape[0])
    return _tower_backward(t, 'vit_train_bwd', params, need, patches.contiguous(), n, d_feats, tape, tape.numel(), False)[1:]


@vit_train_bwd.register_fake
def _(patches, params, tape, d_feats, tower_handle, need):
    return [p.new_empty(tuple(p.shape) if b else (0,), dtype=torch.float32) for p, b in zip(params, need)]


def _tower_setup(ctx, tower_handle, tape, *saved):
    ctx.save_for_backward(tape, *saved)
    ctx.tower_handle = tower_handle
    ctx.mark_non_differentiable(tape)
    ctx.set_materialize_grads(False)


def _vit_setup(ctx, inputs, output):
    patches, params, tower_handle = inputs
    _tower_setup(ctx, tower_handle, output[1], patches, *params)


def _vit_backward(ctx, d_feats, d_tape):
    tape, patches, *params = ctx.saved_tensors
    need = list(ctx.needs_input_grad[1])
    if d_feats is None or not any(need):
        return None, [None] * len(params), None
    got = torch.ops.eventclip_hip.vit_train_bwd(patches, params, tape, d_feats, ctx.tower_handle, need)
    return None, [g if b else None for g, b in zip(got, need)], None


vit_train_fwd.register_autograd(_vit_backward, setup_context=_vit_setup)


# ---- the same tower from the fp32 image, differentiable with respect to it ----
@custom_op(f'{NAMESPACE}::vit_image_fwd', mutates_args=(), device_types='cuda')
def vit_image_fwd(image: torch.Tensor, params: List[torch.Tensor], tower_handle: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """image fp32 [N, 3, R, R] (what ``ec_patchify`` takes), params as ``vit_train_fwd`` takes them -> (feats fp32 [N, D];
    tape uint8: the training workspace of ``vit_train_fwd`` followed by the 16-bit patch rows, which conv1's weight
    gradient reads).  The same launches as ``vit_train_fwd`` on ``patchify(image)``: the same bits.  The autograd formula
    returns d image (``vit_image_bwd``) next to the parameter gradients."""
    t, n, image, feats, tape, (ws, total) = _forward_begin('vit_image_fwd', image, params, tower_handle, image=True)
    patches = t.patchify(image, out=tape[ws:total])
    _lib.launch('ec_vit_train_forward', t._vit, patches, n, feats, tape, ws)
    return feats, tape


@vit_image_fwd.register_fake
def _(image, params, tower_handle):
    t = _resolve(tower_handle, 'vit_image_fwd')
    n = image.shape[0]
    return (image.new_empty((n, t.D), dtype=torch.float32),
            image.new_empty((max(_image_tape(t, n)[1], 256),), dtype=torch.uint8))


@custom_op(f'{NAMESPACE}::vit_image_bwd', mutates_args=(), device_types='cuda')
def vit_image_bwd(params: List[torch.Tensor], tape: torch.Tensor, d_feats: torch.Tensor, tower_handle: int,
                  need_image: bool, need: List[bool]) -> List[torch.Tensor]:
    """The backward of ``vit_image_fwd`` over its tape: 1 + len(params) tensors -- d image fp32 [N, 3, R, R] where
    need_image, then the gradient of params[i] where need[i]; an empty tensor for what is not needed.  With need_image the
    chain runs down to the embedding whatever ``need`` says (``ec_vit_train_backward_image``); weight-, bias- and
    LoRA-gradient kernels run only for what ``need`` names, none at all for a frozen tower.  Without it this is
    ``vit_train_bwd`` on the tape's patch rows.  The tape is only read."""
    t = _resolve(tower_handle, 'vit_image_bwd')
    n = int(d_feats.shape[0])
    ws, total = _image_tape(t, n)
    return _tower_backward(t, 'vit_image_bwd', params, need, tape[ws:total], n, d_feats, tape, ws, need_image)


@vit_image_bwd.register_fake
def _(params, tape, d_feats, tower_handle, need_image, need):
    t = _resolve(tower_handle, 'vit_image_bwd')
    n, R = d_feats.shape[0], t.cfg['image_size']
    return ([d_feats.new_empty((n, 3, R, R) if need_image else (0,), dtype=torch.float32)] +
            [p.new_empty(tuple(p.shape) if b else (0,), dtype=torch.float32) for p, b in zip(params, need)])


def _vit_image_setup(ctx, inputs, output):
    _, params, tower_handle = inputs
    _tower_setup(ctx, tower_handle, output[1], *params)
    # the graph keeps its tower alive (handles are weak): an owner that drops or rebuilds its cached tower -- CLIP.cuda() /
    # .to() after encode_image(differentiable=True) -- leaves a live graph able to run its backward
    ctx.tower = _resolve(tower_handle, 'vit_image_fwd')


def _vit_image_backward(ctx, d_feats, d_tape):
    tape, *params = ctx.saved_tensors
    need_image, need = bool(ctx.needs_input_grad[0]), list(ctx.needs_input_grad[1])
    if d_feats is None or not (need_image or any(need)):
        return None, [None] * len(params), None
    got = torch.ops.eventclip_hip.vit_image_bwd(params, tape, d_feats, ctx.tower_handle, need_image, need)
    return got[0] if need_image else None, [g if b else None for g, b in zip(got[1:], need)], None


vit_image_fwd.register_autograd(_vit_image_backward, setup_context=_vit_image_setup)


OPS = ('events_to_frames', 'events_to_time_surface', 'events_to_voxel_grid', 'events_denoise', 'events_refractory', 'events_time_windows', 'preprocess', 'vit_encode', 'text_encode', 'adapter_fwd', 'classify', 'resnet_encode',
       'classify_bwd', 'adapter_train_fwd', 'adapter_train_bwd', 'vit_train_fwd', 'vit_train_bwd', 'vit_image_fwd', 'vit_image_bwd')
