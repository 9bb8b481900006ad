"""Case tables and branch classifiers for the kernels that turn events into model input: csrc/preprocess.hip,
csrc/randaugment.hip, csrc/augment.hip and the centring / packing kernels of csrc/events.hip.

Nothing here touches torch, a GPU or anything compiled from the package.  Every check on these kernels is bit for bit
against the Pillow- and reference-pinned oracles (oracle/preprocess.py, oracle/randaugment.py, oracle/event_utils.py), so
there is no bound in this file: what it holds is WHERE to look.  The classifiers restate, from the oracle's geometry, which
loop, layout and launch branch of a kernel a case takes; tests/test_datapath_cases_cpu.py asserts that the tables reach
every class a classifier can return (an edit to a table cannot silently lose a branch) and pins the oracles against a live
Pillow at every shape, and the three GPU files (test_preprocess_edges_gpu.py, test_randaugment_edges_gpu.py,
test_event_ingest_edges_gpu.py) hold the kernels to the oracles at them and tie preprocess_path to the launcher's own plan.
"""
import functools
import math

import numpy as np

from oracle import preprocess as op

# ---------------------------------------------------------------------------------------------------------------
# csrc/preprocess.hip
# ---------------------------------------------------------------------------------------------------------------
LDS_OPT_IN = 64 * 1024          # above it the launcher raises the kernel's dynamic-LDS attribute
LDS_LIMIT = 160 * 1024          # above it the launcher refuses
LUT_BYTES = 3 * 256 * 4

# (H, W), n_px: run in modes 'u8' and 'chw'
PREPROCESS_CASES = (
    ((620, 800), 224),          # ks 13: generic horizontal loop; 69 936 B of LDS
    ((1000, 1400), 224),        # ks 19; 110 352 B
    ((400, 533), 224),          # ks 9
    ((336, 337), 224),          # ks_h 9 with ks_v 7
    ((181, 240), 224),          # crop difference 73 -> 36 (half to even, down)
    ((180, 241), 224),          # crop difference 75 -> 38 (half to even, up)
    ((240, 180), 224),          # portrait upscale, top = 37: band 0's window starts inside the image
    ((640, 480), 224),          # portrait downscale
    ((3, 4), 224),              # windows clipped on both sides, byte tails of the unaligned dword reads
    ((4, 3), 224),
    ((1, 1), 224),
    ((180, 240), 225),          # odd n_px: non-pair vertical path, a last band of one row
    ((100, 120), 223),          # odd n_px, 31-row last band
    ((480, 640), 288),          # the ResNet towers' input sizes
    ((180, 240), 384),
    ((480, 640), 448),
    ((180, 240), 448),
)
# (patch, n_px, kpad), (H, W): mode 'patches', f16 and bf16
PATCH_CASES = (
    ((7, 224, 320), (100, 120)),        # odd patch: scalar stores, row-major item order
    ((14, 224, 1177), (100, 120)),      # odd kpad: non-pair path
    ((16, 336, 1536), (100, 120)),      # 11 bands, the last band is one patch row
    ((32, 288, 6144), (100, 120)),      # the 288-px towers' patch layout
    ((14, 224, 1216), (640, 480)),      # portrait and downscale in patch mode
)
# needs 166 736 B: refused before any launch
PREPROCESS_TOO_LARGE = ((1520, 2000), 224)


def _ksize(in_size, out_size):
    return int(math.ceil(2.0 * max(float(in_size) / out_size, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=None)
def preprocess_path(H, W, n_px, mode='chw', patch=1, kpad=0):
    """The branch csrc/preprocess.hip takes for uint8 [H, W, 3] frames -> n_px, from oracle.preprocess's geometry.
    mode is 'u8', 'chw' or 'patches' (then with patch and kpad)."""
    nh, nw = op.resized_size(H, W, n_px)
    top, left = op.center_crop_offsets(nh, nw, n_px)
    ks_h, ks_v = _ksize(W, nw), _ksize(H, nh)
    bv = op.precompute_coeffs(H, nh)[0][top:top + n_px]            # (ymin, count) of the cropped output rows
    bh = op.precompute_coeffs(W, nw)[0][left:left + n_px]
    patches = mode == 'patches'
    band_rows = patch * (1 if patch >= 32 else 32 // patch) if patches else 32
    bands = -(-n_px // band_rows)
    last_rows = n_px - (bands - 1) * band_rows
    max_ny = 0
    for b in range(bands):
        o0, o1 = b * band_rows, min(n_px, (b + 1) * band_rows) - 1
        max_ny = max(max_ny, int(bv[o1, 0] + bv[o1, 1] - bv[o0, 0]))
    tmp_bytes = (max_ny * n_px * 3 + 8 + 15) // 16 * 16
    lds = tmp_bytes + LUT_BYTES + (band_rows * ks_v * 4 + 15) // 16 * 16
    pairs = n_px % 2 == 0 and (not patches or (patch % 2 == 0 and kpad % 2 == 0))
    d_h, d_w = nh - n_px, nw - n_px
    return dict(
        ks_h=ks_h, ks_v=ks_v,
        horizontal='6tap' if ks_h <= 6 else ('12tap' if ks_h <= 12 else 'generic'),
        pairs=pairs,
        by_patch=pairs and patches and last_rows % patch == 0,
        bands=bands, band_rows=band_rows, last_rows=last_rows,
        lds=lds, lds_opt_in=lds > LDS_OPT_IN, lds_refused=lds > LDS_LIMIT,
        geometry=(nh, nw, top, left),
        crop_diff=max(d_h, d_w), crop_odd=max(d_h, d_w) % 2 == 1,
        # .5 rounds to the even neighbour: down when (d - 1) / 2 is even, up when it is odd
        half_rounds=None if max(d_h, d_w) % 2 == 0 else ('down' if (max(d_h, d_w) - 1) // 2 % 2 == 0 else 'up'),
        orientation='portrait' if H > W else ('landscape' if W > H else 'square'),
        upscale_h=nw >= W, upscale_v=nh >= H,
        # an input narrower than a filter window: every window is clipped on both sides
        narrow=W < ks_h or H < ks_v,
        first_row=int(bv[0, 0]), first_col=int(bh[0, 0]),          # where the cropped output's windows start in the input
    )


# ---------------------------------------------------------------------------------------------------------------
# csrc/randaugment.hip
# ---------------------------------------------------------------------------------------------------------------
RA_BAND_PIXELS = 16384
RA_FILL = (10, 200, 77)
RA_BINS = (3, 15, 30)           # counted from 1: entries 2, 14 and 29 of the 30-entry magnitude tables
RA_SHAPES = (
    (127, 129),                 # 16 383 px: one band, scalar loop, frames at odd byte offsets
    (129, 128),                 # 2 bands with quads, boundary at pixel 8256 = the middle of row 64
    (131, 127),                 # 2 bands, scalar loop, band 1 starts at pixel 8320
    (129, 129),                 # square and odd: ROT90 / 270 through the scalar loop across 2 bands
    (3, 3), (7, 3), (3, 9),     # Sharpness interior of one pixel, one column, one row; affine taps never contiguous
    (1, 5), (2, 2), (5, 2),     # no interior at all
)
RA_TINY = ((1, 5), (2, 2), (5, 2))
RA_CHAIN_SHAPE = (131, 127)
RA_CHAIN = (
    [('Contrast', 0.9), ('Rotate', 13.0), ('Equalize', 0.0)],
    [('AutoContrast', 0.0), ('Sharpness', -0.6), ('Contrast', -0.45)],
    [('Sharpness', 0.75), ('Equalize', 0.0), ('Rotate', 13.0)],
)


def randaugment_path(H, W):
    """Bands, the four-pixel fast path and every band's first pixel in aug_stats_kernel and aug_apply_kernel (buffers
    from the allocator are at least dword aligned, so `quads` is decided by the frame's byte size)."""
    npix = H * W
    bands = -(-npix // RA_BAND_PIXELS)
    per_stats = -(-npix // bands)
    per_apply = (per_stats + 3) // 4 * 4
    return dict(
        bands=bands, quads=npix * 3 % 4 == 0,
        frame_bytes_odd=npix * 3 % 2 == 1,
        stats_starts=tuple(b * per_stats for b in range(bands)),
        apply_starts=tuple(min(b * per_apply, npix) for b in range(bands)),
        mid_row_boundary=any(min(b * per_apply, npix) % W != 0 for b in range(1, bands)),
        interior=(max(H - 2, 0), max(W - 2, 0)),                   # Sharpness's filtered region
        contiguous_taps=W >= 4,                                    # the affine row read as three dwords is possible
        square=H == W,
    )


def ra_cases(H, W):
    """[(operator, magnitude)]: every operator at RA_BINS with both signs, Rotate 90 / 180 / 270 where the frame is square
    (elsewhere 180 alone is a fast path; 90 and 270 go through the affine kernel and are kept as such)."""
    from oracle import randaugment as ora
    cases = []
    for name in ora.OPS:
        table = ora.magnitude_table(name, (H, W))
        mags = [0.0] if table is None else [float(table[b - 1]) for b in RA_BINS]
        if name in ora.SIGNED:
            mags = mags + [-m for m in mags if m]
        if name == 'Rotate':
            mags += [90.0, 180.0, 270.0]
        cases += [(name, m) for m in mags]
    return cases


def ra_images(H, W):
    """Random uint8, a sparse event frame whose events all lie in the upper third (the second band's slice of a
    two-band frame holds only background) and a constant frame."""
    from eventclip_amd.synthetic import make_events
    from oracle import events as oe
    rng = np.random.default_rng(1000 * H + W)
    n = max(4, H * W // 12)
    ev = make_events(n, (max(1, H // 3), W), seed=H * 7 + W, hot_pixels=0)
    event = oe.events2frames(ev, shape=(H, W), N=n + 1, grayscale=False, count_non_zero=False, background_mask=True)[0]
    return [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), event, np.full((H, W, 3), 77, dtype=np.uint8)]


# ---------------------------------------------------------------------------------------------------------------
# csrc/events.hip: center_events_kernel (float, 4 x unrolled), center_packed_kernel (8 x), pack_events_kernel;
# csrc/augment.hip
# ---------------------------------------------------------------------------------------------------------------
CENTER_THREADS = 1024
CENTER_N = (1, 3073, 4095, 4096, 4097, 7169, 8192, 8193, 12289, 20000)
CENTER_RES = (180, 240)
AUGMENT_TILE = 1024
AUGMENT_N = (0, 1, 1023, 1024, 1025, 2048, 2049, 5000)
AUGMENT_RES = (36, 52)
PACK_GRID = 4096 * 256
PACK_N = PACK_GRID + 300


def center_unroll(packed):
    return 8 if packed else 4


def center_slots(n, packed):
    """int [n]: the unrolled slot u that reads event i in the centring kernels' loops, -1 where the remainder loop does.
    Thread tid takes `for (i = tid; i + (U - 1) 1024 < n; i += U 1024)` unrolled, then `for (; i < n; i += 1024)`."""
    U, T = center_unroll(packed), CENTER_THREADS
    idx = np.arange(n, dtype=np.int64)
    tid, row = idx % T, idx // T
    iters = np.where(tid + (U - 1) * T < n, (n - 1 - tid - (U - 1) * T) // (U * T) + 1, 0)
    return np.where(row < iters * U, row % U, -1)


def center_path(n, packed):
    """Which threads take the unrolled loop and which the remainder loop ('none', 'some', 'all' of the 1024), the most
    unrolled iterations any thread makes, and how many events each loop reads."""
    slots = center_slots(n, packed)
    U, T = center_unroll(packed), CENTER_THREADS

    def share(mask):
        k = int(np.unique(np.flatnonzero(mask) % T).size)
        return 'none' if k == 0 else ('all' if k == T else 'some')
    n_unrolled = int((slots >= 0).sum())
    return dict(unroll=U, unrolled_threads=share(slots >= 0), remainder_threads=share(slots < 0),
                unrolled_iters=-(-n_unrolled // (U * T)), n_unrolled=n_unrolled, n_remainder=n - n_unrolled)


def augment_tiles(n):
    """Tiles of 1024 events augment_events_kernel walks, and the events in the last one."""
    tiles = -(-n // AUGMENT_TILE)
    return dict(tiles=tiles, last=n - (tiles - 1) * AUGMENT_TILE if tiles else 0)


def pack_path(n):
    blocks = -(-n // 256)
    return dict(grid=min(blocks, 4096), passes=-(-n // (min(blocks, 4096) * 256)))


def center_holders(n, packed):
    """Candidate indices that hold an extreme: the first and the last event, one index read by each unrolled slot, one
    read by the remainder loop; filled up to five distinct indices (when n allows) so that the five extremes of a sample
    sit on five different events."""
    slots = center_slots(n, packed)
    cand = [0, n - 1]
    for u in range(center_unroll(packed)):
        at = np.flatnonzero(slots == u)
        if at.size:
            cand.append(int(at[(2 * u + 1) * at.size // (2 * center_unroll(packed))]))
    rem = np.flatnonzero(slots < 0)
    if rem.size:
        cand.append(int(rem[rem.size // 2]))
    for extra in (n // 3, n // 5, 2 * n // 3, n // 7, 4 * n // 5):
        if len(set(cand)) >= 5:
            break
        cand.append(extra)
    out = []
    for c in cand:
        if c not in out:
            out.append(c)
    return out


# (x_min, x_max, y_min, y_max) of a centring sample, CENTER_RES = (180, 240)
CENTER_BOXES = (
    (20, 200, 15, 150),         # shifts (-10, -8): even sums
    (4, 100, 2, 61),            # (x_max + x_min + 1 - W) = -135, (.. - H) = -116: negative and odd / even
    (31, 239, 10, 179),         # 31: positive and odd
    (7, 9, 3, 120),             # -223: negative and odd, a narrow box
)
CENTER_BOX_WRAPS = (10, 600, 5, 420)        # packed only: shifts (185, 123) move x_min and y_min below zero


def center_sample(n, holders, rot, box, seed):
    """float32 [n, 4] events with integral coordinates strictly inside `box` and whole-microsecond times, except that
    x_min, x_max, y_min, y_max and t_min are each held by exactly one event: extreme j by holders[(j + rot) % len]
    (n < 5: by whichever events there are).  A loop slice that is skipped, or read twice with another's index, changes
    the sample's shift or its first time."""
    x0, x1, y0, y1 = box
    rng = np.random.default_rng(seed)
    ev = np.empty((n, 4), dtype=np.float64)
    ev[:, 0] = rng.integers(x0 + 1, x1, size=n)
    ev[:, 1] = rng.integers(y0 + 1, y1, size=n)
    ev[:, 2] = rng.integers(2000, 300000, size=n) / 1e6          # not sorted: the kernels do not need it to be
    ev[:, 3] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    L = len(holders)
    at = [holders[(j + rot) % L] for j in range(5)]
    ev[at[0], 0] = x0
    ev[at[1], 0] = x1
    ev[at[2], 1] = y0
    ev[at[3], 1] = y1
    ev[at[4], 2] = 1000 / 1e6
    if n == 1:                                                    # one event holds everything
        ev[0, :3] = (x0, y0, 1000 / 1e6)
    return ev.astype(np.float32), at


def center_samples(packed):
    """[(events, n, rot, box)] for every n of CENTER_N and every rotation of its holders, boxes taken in turn."""
    out = []
    k = 0
    for n in CENTER_N:
        holders = center_holders(n, packed)
        for rot in range(len(holders)):
            box = CENTER_BOXES[k % len(CENTER_BOXES)]
            out.append((center_sample(n, holders, rot, box, seed=31 * n + rot)[0], n, rot, box))
            k += 1
    return out


# (dx, dy, flip_x) of csrc/augment.hip's cases on events confined to x in [6, W - 7], y in [5, H - 6], each with both
# flip_t states
AUGMENT_SHIFTS = (
    (6, -5, 0),                             # keeps every event (they reach the sensor's edge)
    (-(AUGMENT_RES[1] // 2), 0, 0),         # drops about half
    (AUGMENT_RES[1], 0, 0),                 # drops all
    (-10, 7, 1),                            # flip_x, with some dropped
)


def augment_sample(n, seed):
    H, W = AUGMENT_RES
    rng = np.random.default_rng(seed)
    ev = np.empty((n, 4), dtype=np.float32)
    ev[:, 0] = rng.integers(6, W - 6, size=n)
    ev[:, 1] = rng.integers(5, H - 5, size=n)
    ev[:, 2] = np.sort(rng.uniform(0.0, 0.3, size=n)).astype(np.float32)
    ev[:, 3] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return ev
