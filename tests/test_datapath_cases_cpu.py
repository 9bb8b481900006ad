"""tests/datapath_cases.py without a GPU: the case tables reach every class their classifiers can return, and the oracles
the GPU edge suites compare with agree with a live Pillow at every shape of the tables."""
import numpy as np
import pytest
from PIL import Image, ImageEnhance

import datapath_cases as dc
from oracle import preprocess as op
from oracle import randaugment as ora
from test_oracle_randaugment import pil_op


def _paths(mode):
    if mode == 'patches':
        return [dc.preprocess_path(*shape, n_px, 'patches', patch, kpad) for (patch, n_px, kpad), shape in dc.PATCH_CASES]
    return [dc.preprocess_path(*shape, n_px, mode) for shape, n_px in dc.PREPROCESS_CASES]


# ---------------------------------------------------------------------------------------------------------------
# coverage of the tables
# ---------------------------------------------------------------------------------------------------------------
def test_preprocess_table_reaches_every_class():
    chw, pat = _paths('chw'), _paths('patches')
    assert _paths('u8') == chw                                           # the mode changes the store alone
    assert {p['horizontal'] for p in chw} == {'6tap', '12tap', 'generic'}
    assert {p['horizontal'] for p in pat} >= {'6tap', '12tap'}
    assert {5, 7, 9, 11, 13, 19} <= {p['ks_h'] for p in chw}
    assert any(p['ks_h'] != p['ks_v'] for p in chw)
    # the vertical pass: pairs or single pixels, and why
    assert {p['pairs'] for p in chw} == {True, False}
    assert {(p['pairs'], p['by_patch']) for p in pat} == {(True, True), (False, False)}
    odd = {(patch % 2, kpad % 2) for (patch, _, kpad), _ in dc.PATCH_CASES}
    assert {(1, 0), (0, 1), (0, 0)} <= odd                               # odd patch, odd kpad, neither
    # bands: a full and a short last band in both layouts, down to one row / one patch row
    for paths in (chw, pat):
        assert {p['last_rows'] < p['band_rows'] for p in paths} == {True, False}
    assert any(p['last_rows'] == 1 for p in chw)
    assert any(p['last_rows'] == patch and p['last_rows'] < p['band_rows']
               for p, ((patch, _, _), _) in zip(pat, dc.PATCH_CASES))
    # the patch loop's band_rows rule: below 32 several patch rows per band, from 32 on one
    assert {patch >= 32 for (patch, _, _), _ in dc.PATCH_CASES} == {True, False}
    # LDS: under the opt-in, over it, and (one geometry, refused before any launch) over the limit
    assert {p['lds_opt_in'] for p in chw} == {True, False}
    assert not any(p['lds_refused'] for p in chw + pat)
    big = dc.preprocess_path(*dc.PREPROCESS_TOO_LARGE[0], dc.PREPROCESS_TOO_LARGE[1], 'chw')
    assert big['lds_refused'] and big['lds'] == 166736
    # the crop: even difference, and .5 rounded to even in both directions
    assert {p['half_rounds'] for p in chw} == {None, 'down', 'up'}
    # orientation and scaling direction
    assert {p['orientation'] for p in chw} == {'portrait', 'landscape', 'square'}
    assert {(p['orientation'], p['upscale_v']) for p in chw} >= {('portrait', True), ('portrait', False),
                                                                 ('landscape', True), ('landscape', False)}
    assert any(p['orientation'] == 'portrait' and p['horizontal'] == '12tap' for p in pat)
    assert any(p['first_row'] > 0 for p in chw) and any(p['first_col'] > 0 for p in chw)
    assert {p['narrow'] for p in chw} == {True, False}
    # every tower's input size (eventclip_amd/resnet.py and the ViTs' 224 / 336 of test_preprocess_gpu.py)
    from eventclip_amd.resnet import RESNET_ARCHS
    assert {a['image_size'] for a in RESNET_ARCHS.values()} <= {n_px for _, n_px in dc.PREPROCESS_CASES}


def test_preprocess_classifier_restates_the_issue_figures():
    """The figures the table's comments quote, so that an edit to the classifier shows."""
    p = dc.preprocess_path(620, 800, 224, 'chw')
    assert (p['ks_h'], p['lds'], p['horizontal']) == (13, 69936, 'generic')
    p = dc.preprocess_path(1000, 1400, 224, 'chw')
    assert (p['ks_h'], p['lds']) == (19, 110352)
    assert dc.preprocess_path(400, 533, 224)['ks_h'] == 9
    p = dc.preprocess_path(336, 337, 224)
    assert (p['ks_h'], p['ks_v']) == (9, 7)
    assert dc.preprocess_path(181, 240, 224)['geometry'] == (224, 297, 0, 36)      # 73 / 2 -> 36
    assert dc.preprocess_path(180, 241, 224)['geometry'] == (224, 299, 0, 38)      # 75 / 2 -> 38
    assert dc.preprocess_path(240, 180, 224)['geometry'][2] == 37
    assert dc.preprocess_path(640, 480, 224)['geometry'][2] == 37
    p = dc.preprocess_path(180, 240, 225)
    assert (p['pairs'], p['bands'], p['last_rows']) == (False, 8, 1)
    p = dc.preprocess_path(100, 120, 223)
    assert (p['pairs'], p['last_rows']) == (False, 31)
    p = dc.preprocess_path(100, 120, 336, 'patches', 16, 1536)
    assert (p['bands'], p['last_rows']) == (11, 16)
    # the shapes test_preprocess_gpu.py already runs reach none of the branches this table is for
    for shape, n_px in (((180, 240), 224), ((100, 120), 224), ((480, 640), 224), ((480, 640), 336), ((180, 240), 336),
                        ((224, 224), 224), ((300, 224), 224)):
        p = dc.preprocess_path(*shape, n_px)
        assert p['horizontal'] != 'generic' and p['pairs'] and not p['lds_opt_in'] and not p['crop_odd']
        assert p['ks_h'] in (5, 7, 11) and not p['narrow']


def test_randaugment_table_reaches_every_class():
    paths = {s: dc.randaugment_path(*s) for s in dc.RA_SHAPES}
    assert {(p['bands'] > 1, p['quads']) for p in paths.values()} == {(False, False), (False, True), (True, False),
                                                                     (True, True)}
    assert any(p['frame_bytes_odd'] and p['bands'] == 1 for p in paths.values())
    assert any(p['mid_row_boundary'] and p['quads'] for p in paths.values())
    assert any(p['mid_row_boundary'] and not p['quads'] for p in paths.values())
    # the two kernels split a frame differently when the per-band count is no multiple of four
    assert any(p['stats_starts'] != p['apply_starts'] for p in paths.values())
    assert any(p['square'] and p['bands'] > 1 and not p['quads'] for p in paths.values())
    interiors = {p['interior'] for p in paths.values()}
    assert (1, 1) in interiors and any(h > 1 and w == 1 for h, w in interiors) \
        and any(h == 1 and w > 1 for h, w in interiors)
    assert {h * w == 0 for h, w in interiors} == {True, False}
    assert {p['contiguous_taps'] for p in paths.values()} == {True, False}
    assert set(dc.RA_TINY) <= set(dc.RA_SHAPES) and all(0 in paths[s]['interior'] for s in dc.RA_TINY)
    assert paths[(129, 128)]['apply_starts'] == (0, 8256) and paths[(131, 127)]['apply_starts'] == (0, 8320)
    assert paths[(127, 129)]['bands'] == 1 and 127 * 129 == 16383
    # the shapes test_randaugment_gpu.py builds: one band, four pixels at a time; its reference fixture's 100 x 120 and
    # 180 x 240 frames likewise go four pixels at a time, the latter in three bands that each start a row
    for s in ((45, 60), (90, 120), (20, 33), (32, 32), (50, 70), (100, 120)):
        p = dc.randaugment_path(*s)
        assert p['bands'] == 1 and p['quads']
    p = dc.randaugment_path(180, 240)
    assert p['bands'] == 3 and p['quads'] and not p['mid_row_boundary'] and p['stats_starts'] == p['apply_starts']
    p = dc.randaugment_path(*dc.RA_CHAIN_SHAPE)
    assert p['bands'] == 2 and not p['quads'] and p['frame_bytes_odd']
    names = {name for ops in dc.RA_CHAIN for name, _ in ops}
    assert {'Contrast', 'Equalize', 'AutoContrast', 'Sharpness', 'Rotate'} <= names
    assert len({tuple(ops) for ops in dc.RA_CHAIN}) == len(dc.RA_CHAIN) == 3 and all(len(o) == 3 for o in dc.RA_CHAIN)
    for s in dc.RA_SHAPES:
        cases = dc.ra_cases(*s)
        assert {name for name, _ in cases} == set(ora.OPS)
        for name in ora.SIGNED:
            mags = [m for n_, m in cases if n_ == name]
            assert any(m > 0 for m in mags) and any(m < 0 for m in mags)
        assert {('Rotate', 90.0), ('Rotate', 180.0), ('Rotate', 270.0)} <= set(cases)


def test_event_tables_reach_every_class():
    flt = {n: dc.center_path(n, False) for n in dc.CENTER_N}
    pk = {n: dc.center_path(n, True) for n in dc.CENTER_N}
    for paths in (flt, pk):
        # no thread, some threads, every thread in the unrolled loop; with and without a remainder; one and several passes
        assert {p['unrolled_threads'] for p in paths.values()} == {'none', 'some', 'all'}
        assert {p['remainder_threads'] for p in paths.values()} >= {'none', 'some'}
        assert any(p['unrolled_threads'] == 'all' and p['remainder_threads'] == 'none' for p in paths.values())
        assert any(p['unrolled_threads'] == 'all' and p['n_remainder'] == 1 for p in paths.values())
        assert {min(p['unrolled_iters'], 2) for p in paths.values()} == {0, 1, 2}
    assert flt[3073]['n_unrolled'] == 4 and flt[7169]['unrolled_iters'] == 2 and pk[7169]['n_unrolled'] == 8
    assert pk[4097]['unrolled_threads'] == 'none' and pk[8193]['n_remainder'] == 1
    # the sizes test_events_gpu.py / test_ingest_gpu.py centre: only remainder loops
    assert dc.center_path(1900, False)['unrolled_threads'] == 'none'
    assert dc.center_path(700, True)['unrolled_threads'] == 'none'
    for packed in (False, True):
        for n in dc.CENTER_N:
            slots, holders = dc.center_slots(n, packed), dc.center_holders(n, packed)
            assert len(holders) == len(set(holders)) and all(0 <= h < n for h in holders)
            assert len(holders) >= min(n, 5) and holders[0] == 0 and (n - 1) in holders
            assert {int(slots[h]) for h in holders} >= set(np.unique(slots).tolist())   # every slot and the remainder
    tiles = {n: dc.augment_tiles(n) for n in dc.AUGMENT_N}
    assert {min(t['tiles'], 3) for t in tiles.values()} == {0, 1, 2, 3}
    assert {t['last'] for t in tiles.values()} >= {0, 1, dc.AUGMENT_TILE - 1, dc.AUGMENT_TILE}
    assert any(t['tiles'] > 1 and 1 < t['last'] < dc.AUGMENT_TILE for t in tiles.values())
    assert all(dc.augment_tiles(n)['tiles'] == 1 for n in (700, 500, 300))              # the golden samples
    assert dc.pack_path(dc.PACK_N) == dict(grid=4096, passes=2) and dc.pack_path(dc.PACK_GRID)['passes'] == 1


def test_center_samples_put_each_extreme_on_one_event():
    for packed in (False, True):
        samples = dc.center_samples(packed)
        assert {s[1] for s in samples} == set(dc.CENTER_N)
        seen = {}
        for ev, n, rot, box in samples:
            holders = dc.center_holders(n, packed)
            _, at = dc.center_sample(n, holders, rot, box, seed=31 * n + rot)
            if n >= 5:
                assert len(set(at)) == 5
                for col, lo, hi in ((0, at[0], at[1]), (1, at[2], at[3])):
                    assert np.flatnonzero(ev[:, col] == ev[:, col].min()).tolist() == [lo]
                    assert np.flatnonzero(ev[:, col] == ev[:, col].max()).tolist() == [hi]
                assert np.flatnonzero(ev[:, 2] == ev[:, 2].min()).tolist() == [at[4]]
                for j, a in enumerate(at):
                    seen.setdefault((n, j), set()).add(a)
                assert (ev[:, 0].min(), ev[:, 0].max(), ev[:, 1].min(), ev[:, 1].max()) == box
            assert (ev[:, :2] == np.trunc(ev[:, :2])).all() and ev[:, :2].min() >= 0   # packable
        for n in dc.CENTER_N[1:]:
            for j in range(5):                                           # every extreme visits every holder
                assert seen[(n, j)] == set(dc.center_holders(n, packed))
    H, W = dc.CENTER_RES
    sums = [(x1 + x0 + 1 - W, y1 + y0 + 1 - H) for x0, x1, y0, y1 in dc.CENTER_BOXES]
    assert any(s < 0 and s % 2 for pair in sums for s in pair)           # floor division != truncation there
    assert any(s > 0 and s % 2 for pair in sums for s in pair) and any(s % 2 == 0 for pair in sums for s in pair)
    x0, x1, y0, y1 = dc.CENTER_BOX_WRAPS
    assert (x1 + x0 + 1 - W) // 2 > x0 and (y1 + y0 + 1 - H) // 2 > y0 and x1 < 65536 and y1 < 65536


# ---------------------------------------------------------------------------------------------------------------
# the oracles against Pillow at the tables' shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,n_px', dict.fromkeys(dc.PREPROCESS_CASES + tuple((s, p[1]) for p, s in dc.PATCH_CASES)),
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_resize_crop_oracle_matches_pillow(shape, n_px):
    rng = np.random.default_rng(shape[0] * 4099 + shape[1] + n_px)
    img = rng.integers(0, 256, size=(*shape, 3), dtype=np.uint8)
    nh, nw, top, left = dc.preprocess_path(*shape, n_px)['geometry']
    want = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC).crop((left, top, left + n_px, top + n_px)))
    np.testing.assert_array_equal(op.resize_crop_u8(img[None], n_px)[0], want)


@pytest.mark.parametrize('shape', dc.RA_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_randaugment_oracle_matches_pillow(shape):
    cases = dc.ra_cases(*shape)
    for img in dc.ra_images(*shape):
        pil = Image.fromarray(img)
        for name, mag in cases:
            want = np.asarray(pil_op(pil, name, mag, dc.RA_FILL))
            got = ora.apply_op(img, name, mag, dc.RA_FILL)
            assert got.dtype == np.uint8 and got.shape == img.shape
            if not np.array_equal(got, want):
                d = np.argwhere(got != want)
                raise AssertionError(f'{name} {mag} image {img.shape}: {len(d)} values differ, first at '
                                     f'{d[0].tolist()}: {got[tuple(d[0])]} vs {want[tuple(d[0])]}')


def test_event_frame_of_a_two_band_shape_leaves_band_one_background():
    for shape in dc.RA_SHAPES:
        p = dc.randaugment_path(*shape)
        event = dc.ra_images(*shape)[1].reshape(-1, 3)
        assert len(np.unique(event, axis=0)) > 1 or shape[0] * shape[1] < 16          # it has events
        if p['bands'] > 1:
            assert (event[p['apply_starts'][1]:] == 255).all() and (event[p['stats_starts'][1]:] == 255).all()


@pytest.mark.parametrize('shape', dc.RA_TINY, ids=lambda s: f'{s[0]}x{s[1]}')
def test_smooth_of_an_image_without_interior_is_the_image(shape):
    """ImageFilter.SMOOTH leaves an image with a side under 3 unchanged, so Sharpness is the identity there."""
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    img = rng.integers(0, 256, size=(*shape, 3), dtype=np.uint8)
    np.testing.assert_array_equal(ora.smooth(img), img)
    for mag in (-0.9, -0.3, 0.45, 0.9):
        want = np.asarray(ImageEnhance.Sharpness(Image.fromarray(img)).enhance(1.0 + mag))
        np.testing.assert_array_equal(want, img)
        np.testing.assert_array_equal(ora.apply_op(img, 'Sharpness', mag, dc.RA_FILL), want)
