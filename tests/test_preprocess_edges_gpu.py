"""csrc/preprocess.hip at every loop and layout edge (tests/datapath_cases.py), bit for bit against the Pillow-pinned oracle
(MI355X): the generic horizontal loop, LDS past the 64 KiB opt-in, the single-pixel vertical path, row-major patch stores,
half-to-even crops, portrait and tiny inputs, short last bands and the ResNet towers' input sizes."""
import functools

import numpy as np
import pytest

import datapath_cases as dc

pytestmark = pytest.mark.gpu

F = 3


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _frames_and_u8(shape, n_px):
    """F random frames of `shape` and the oracle's resized + cropped uint8 frames, computed once per geometry."""
    from oracle import preprocess as op
    rng = np.random.default_rng(shape[0] * 4099 + shape[1] + n_px)
    frames = rng.integers(0, 256, size=(F, *shape, 3), dtype=np.uint8)
    want = op.resize_crop_u8(frames, n_px)
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, want


def _chw(u8):
    from oracle import preprocess as op
    lut = op.normalise_lut()
    return np.stack([lut[c][u8[..., c]] for c in range(3)], axis=1)


def _assert_plan_is_the_classifiers(shape, n_px, path):
    import torch
    from eventclip_amd import preprocess as pp
    assert pp.plan_geometry(*shape, n_px) == path['geometry']
    host, _ = pp._plan(*shape, n_px, torch.device('cuda', torch.cuda.current_device()))
    assert (int(host[8]), int(host[9])) == (path['ks_h'], path['ks_v'])


@pytest.mark.parametrize('shape,n_px', dc.PREPROCESS_CASES, ids=_id)
def test_u8_and_chw_bit_exact_at_every_branch(shape, n_px, hip):
    import torch
    from eventclip_amd import preprocess as pp
    path = dc.preprocess_path(*shape, n_px, 'chw')
    _assert_plan_is_the_classifiers(shape, n_px, path)
    frames, want = _frames_and_u8(shape, n_px)
    dev = torch.from_numpy(frames.copy()).cuda()
    got = pp.preprocess_frames(dev, n_px, mode='u8').cpu().numpy()
    np.testing.assert_array_equal(got, want)
    got = pp.preprocess_frames(dev, n_px, mode='chw').cpu().numpy()
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, _chw(want))               # the same fp32 values, bit for bit


@pytest.mark.parametrize('dt', ['float16', 'bfloat16'])
@pytest.mark.parametrize('geo,shape', dc.PATCH_CASES, ids=_id)
def test_patch_rows_bit_exact_padding_zero_tail_untouched(geo, shape, dt, hip):
    import torch
    from eventclip_amd import preprocess as pp
    from oracle import preprocess as op
    patch, n_px, kpad = geo
    dtype = getattr(torch, dt)
    path = dc.preprocess_path(*shape, n_px, 'patches', patch, kpad)
    _assert_plan_is_the_classifiers(shape, n_px, path)
    frames, u8 = _frames_and_u8(shape, n_px)
    g = (n_px // patch) ** 2
    numel, tail = F * g * kpad, 4096
    out = torch.full((numel + tail,), 7., dtype=dtype, device='cuda')      # sentinel everywhere, and past the last row
    pp.preprocess_frames(torch.from_numpy(frames.copy()).cuda(), n_px, mode='patches', patch=patch, kpad=kpad,
                         dtype=dtype, out=out)
    host = out.cpu()
    got = host[:numel].view(F, g, kpad)
    want = op.patchify_split(_chw(u8), patch, kpad, dtype)
    assert torch.equal(got, want)
    k = 6 * patch * patch
    assert torch.equal(got[:, :, k:], torch.zeros(F, g, kpad - k, dtype=dtype))     # the K padding reads zero
    assert torch.equal(host[numel:], torch.full((tail,), 7., dtype=dtype))          # nothing written past the rows


def test_no_frames_give_an_empty_tensor(hip):
    import torch
    from eventclip_amd import preprocess as pp
    empty = torch.empty((0, 100, 120, 3), dtype=torch.uint8, device='cuda')
    assert tuple(pp.preprocess_frames(empty, 224, mode='chw').shape) == (0, 3, 224, 224)
    assert tuple(pp.preprocess_frames(empty, 224, mode='u8').shape) == (0, 224, 224, 3)
    got = pp.preprocess_frames(empty, 224, mode='patches', patch=14, kpad=1216)
    assert tuple(got.shape) == (0, 256, 1216) and got.dtype == torch.float16


def test_a_band_over_the_lds_limit_is_refused_before_any_launch(hip):
    """(1520, 2000) -> 224 needs 166 736 B of LDS, over the 160 KiB the launcher allows: an argument check, the
    library's own error; the next ordinary call is unaffected."""
    import torch
    from eventclip_amd import preprocess as pp
    shape, n_px = dc.PREPROCESS_TOO_LARGE
    path = dc.preprocess_path(*shape, n_px, 'u8')
    assert path['lds_refused'] and path['lds'] == 166736
    frames = torch.zeros((1, *shape, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match=f'ec_preprocess.*{path["lds"]} bytes of LDS'):
        pp.preprocess_frames(frames, n_px, mode='u8')
    shape, n_px = (181, 240), 224
    frames, want = _frames_and_u8(shape, n_px)
    got = pp.preprocess_frames(torch.from_numpy(frames.copy()).cuda(), n_px, mode='u8').cpu().numpy()
    np.testing.assert_array_equal(got, want)
