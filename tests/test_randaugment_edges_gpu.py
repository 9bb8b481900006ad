"""csrc/randaugment.hip past one band and off the four-pixel path (tests/datapath_cases.py), bit for bit against the
Pillow-pinned oracle (MI355X): per-frame statistics summed across workgroups, a band boundary in the middle of a row,
the scalar per-pixel loop with frames at odd byte offsets, and frames with a one-pixel-wide or no Sharpness interior."""
import numpy as np
import pytest

import datapath_cases as dc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('shape', dc.RA_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_operator_at_the_band_and_layout_edges(shape, hip):
    import torch
    from eventclip_amd import randaugment as ra
    from oracle import randaugment as ora
    cases = dc.ra_cases(*shape)
    imgs = dc.ra_images(*shape)
    # one launch: frame i of the stack is image i // len(cases) under case i % len(cases) as a single-op list
    frames = np.concatenate([np.repeat(img[None], len(cases), axis=0) for img in imgs])
    got = ra.apply_ops(torch.from_numpy(frames).cuda(), [[c] for c in cases] * len(imgs), dc.RA_FILL).cpu().numpy()
    for k, img in enumerate(imgs):
        for i, (name, mag) in enumerate(cases):
            want = ora.apply_op(img, name, mag, dc.RA_FILL)
            g = got[k * len(cases) + i]
            if not np.array_equal(g, want):
                d = np.argwhere(g != want)
                raise AssertionError(f'{name} {mag} image {k} {img.shape}: {len(d)} bytes differ, first at '
                                     f'{d[0].tolist()}: {g[tuple(d[0])]} vs {want[tuple(d[0])]}')


def test_three_op_chain_on_unaligned_two_band_frames(hip):
    """The ping-pong workspace with frames at odd byte offsets, statistics recomputed at every step from what the step
    before wrote, a different operator list per frame."""
    import torch
    from eventclip_amd import randaugment as ra
    from oracle import randaugment as ora
    H, W = dc.RA_CHAIN_SHAPE
    lists = [list(ops) for ops in dc.RA_CHAIN]
    frames = np.stack(dc.ra_images(H, W)[:2] + [np.random.default_rng(9).integers(0, 256, (H, W, 3), dtype=np.uint8)])
    got = ra.apply_ops(torch.from_numpy(frames).cuda(), lists, dc.RA_FILL).cpu().numpy()
    for f, ops, g in zip(frames, lists, got):
        np.testing.assert_array_equal(g, ora.randaugment(f[None], ops, dc.RA_FILL)[0], err_msg=str(ops))
