"""The voxel-grid kernel next to the histogram and the time-surface paths on the same events (run on the GPU box).

    python tools/bench_voxel_grid.py [--frames 2560] [--rounds 5] [--out FILE]

2560 frames at the three dataset geometries, float rows and packed events, 3 bins.  After a warm-up of every launch the
variants of a (geometry, layout) are timed in turn, round after round (device events around each launch), and the
median round is reported: ms, GB/s over the algorithmic bytes, 16 (packed: 8) per event in plus 3 H W per frame out,
that rate as a share of the histogram path's in the same run, and the time ratio.  Voxel-grid variants: the frames
(the production op; a banded sensor's grid lives in a temporary), the frames with the grid returned, and the grid alone.
Prints a markdown table; --out also writes it to a file.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eventclip_amd import _lib, vis  # noqa: E402
from eventclip_amd.synthetic import make_events  # noqa: E402

GEOMETRIES = (('n_cars', (100, 120), 12500), ('n_caltech', (180, 240), 20000), ('n_imagenet', (480, 640), 70000))
HBM_GBS = 8000.          # the MI355X's peak, for the share column


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2560)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    uniq = 8
    lines = [f'| geometry | bands | events / frame | layout | variant | ms / {a.frames} frames | GB/s algorithmic | of HBM peak | vs histogram |',
             '|---|---|---|---|---|---|---|---|---|']
    for name, shape, n in GEOMETRIES:
        H, W = shape
        samples = [make_events(n, shape, seed=i) for i in range(uniq)]
        rng = torch.tensor([[i * n, (i + 1) * n] for i in range(a.frames)], dtype=torch.int64).cuda()
        bands = vis.voxel_grid_bands(shape, 3)
        for packed in (False, True):
            parts = [vis.pack_events(s).view(np.int64) if packed else s for s in samples]
            e = torch.from_numpy(np.concatenate(parts)).cuda().repeat((a.frames // uniq + 1,) + (1,) * (parts[0].ndim - 1))[:a.frames * n]
            kw = dict(max_frame_events=n, total_events=a.frames * n)
            # caller-owned outputs for the grid variants: their allocation is not the kernel's time
            frames = torch.empty((a.frames, H, W, 3), dtype=torch.uint8, device='cuda')
            grid = torch.empty((a.frames, H, W, 3), dtype=torch.int32, device='cuda')
            prm = vis.voxel_grid_params(shape, 3, True, n, False, False, False, a.frames * n)
            entry = 'ec_events_to_voxel_grid_packed' if packed else 'ec_events_to_voxel_grid'
            variants = (('histogram', lambda: vis.events_to_frames_device(e, rng, shape, **kw)),
                        ('time surface, linear', lambda: vis.time_surface_device(e, rng, shape, decay='linear', **kw)),
                        ('voxel grid, frames (op)', lambda: vis.voxel_grid_device(e, rng, shape, **kw)),
                        ('voxel grid, frames + grid', lambda: _lib.launch(entry, e, rng, a.frames, prm, frames, grid, None)),
                        ('voxel grid, grid alone', lambda: _lib.launch(entry, e, rng, a.frames, prm, None, grid, None)),
                        ('voxel grid, frames, no grid', lambda: _lib.launch(entry, e, rng, a.frames, prm, frames, None, None)))
            for _, fn in variants:
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            ms = {v: [] for v, _ in variants}
            for _ in range(a.rounds):
                for v, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[v].append(e0.elapsed_time(e1))
            alg = a.frames * ((8 if packed else 16) * n + 3 * H * W)
            base = statistics.median(ms['histogram'])
            for v, _ in variants:
                m = statistics.median(ms[v])
                gbs = alg / m / 1e6
                lines.append(f'| {name} {H}x{W} | {bands} | {n} | {"packed" if packed else "float"} | {v} | {m:.3f} '
                             f'(min {min(ms[v]):.3f}, max {max(ms[v]):.3f}) | {gbs:.0f} | {100 * gbs / HBM_GBS:.1f} % | {base / m:.2f}x |')
                print(lines[-1], flush=True)
            del e, frames, grid
    table = '\n'.join(lines) + '\n'
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)


if __name__ == '__main__':
    main()
