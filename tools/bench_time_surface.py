"""The time-surface kernel next to the histogram path on the same events (run on the GPU box).

    python tools/bench_time_surface.py [--frames 2560] [--rounds 5] [--gray] [--out FILE]

2560 frames at the three dataset geometries, float rows and packed events, both decays.  After a warm-up of every
launch the variants of a (geometry, layout) are timed in turn, round after round (device events around each launch),
and the median round is reported: ms and GB/s over the algorithmic bytes, 16 (packed: 8) per event in plus 3 H W per
frame out.  Red / blue colours unless --gray (the grayscale=True default of the configs, whose three channels are one
computation).  Prints a markdown table; --out also writes it to a file.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eventclip_amd import vis  # noqa: E402
from eventclip_amd.synthetic import make_events  # noqa: E402

GEOMETRIES = (('n_cars', (100, 120), 12500), ('n_caltech', (180, 240), 20000), ('n_imagenet', (480, 640), 70000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2560)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--gray', action='store_true', help='grayscale=True instead of the red / blue map')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    uniq = 8
    lines = [f'| geometry | events / frame | layout | variant | ms / {a.frames} frames | GB/s algorithmic | vs histogram |',
             '|---|---|---|---|---|---|---|']
    for name, shape, n in GEOMETRIES:
        samples = [make_events(n, shape, seed=i) for i in range(uniq)]
        rng = torch.tensor([[i * n, (i + 1) * n] for i in range(a.frames)], dtype=torch.int64).cuda()
        for packed in (False, True):
            parts = [vis.pack_events(s).view(np.int64) if packed else s for s in samples]
            e = torch.from_numpy(np.concatenate(parts)).cuda().repeat((a.frames // uniq + 1,) + (1,) * (parts[0].ndim - 1))[:a.frames * n]
            kw = dict(grayscale=a.gray, max_frame_events=n, total_events=a.frames * n)
            variants = (('histogram', lambda: vis.events_to_frames_device(e, rng, shape, **kw)),
                        ('time surface, linear', lambda: vis.time_surface_device(e, rng, shape, decay='linear', **kw)),
                        ('time surface, exp', lambda: vis.time_surface_device(e, rng, shape, decay='exp', tau=0.03, **kw)))
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
            alg = a.frames * ((8 if packed else 16) * n + 3 * shape[0] * shape[1])
            base = statistics.median(ms['histogram'])
            for v, _ in variants:
                m = statistics.median(ms[v])
                lines.append(f'| {name} {shape[0]}x{shape[1]} | {n} | {"packed" if packed else "float"} | {v} | {m:.3f} '
                             f'(min {min(ms[v]):.3f}, max {max(ms[v]):.3f}) | {alg / m / 1e6:.0f} | {base / m:.2f}x |')
                print(lines[-1], flush=True)
            del e
    table = '\n'.join(lines) + '\n'
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)


if __name__ == '__main__':
    main()
