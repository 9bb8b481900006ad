"""The background-activity filter next to the other read-and-compact kernel (ec_augment_events) and the histogram
frames on the same events (run on the GPU box).

    python tools/bench_denoise.py [--samples 256] [--rounds 5] [--out FILE]

Samples of the three dataset geometries at their sample sizes (synthetic.GEOMETRY: max_n events over max_t seconds),
float rows and packed events, radius 1 with dt 5 ms and 10 ms, and radius 3 with dt 5 ms.  After a warm-up of every launch
the variants of a (geometry, layout) are timed in turn, round after round (device events around each launch), and the
median round is reported: ms, events per second, GB/s over the algorithmic bytes (every event read once and at most
written once; the frames: 16 / 8 per event in plus 3 H W per frame out), and the share of events the filter keeps.
ec_augment_events takes float rows only and runs with a zero shift (nothing dropped).
Prints a markdown table; --out also writes it to a file.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eventclip_amd import _lib, vis  # noqa: E402
from eventclip_amd.synthetic import GEOMETRY, make_events  # noqa: E402

FILTERS = ((1, 5000), (1, 10000), (3, 5000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    uniq, B = 8, a.samples
    lines = [f'| geometry | bands (r 1 / r 3) | events / sample | layout | variant | ms / {B} samples | M events / s | GB/s algorithmic | kept |',
             '|---|---|---|---|---|---|---|---|---|']
    lib = _lib.lib()
    for name in ('n_cars', 'n_caltech', 'n_imagenet'):
        g = GEOMETRY[name]
        (H, W), n, N = g['resolution'], g['max_n'], g['N']
        samples = [make_events(n, (H, W), seed=i, max_t=g['max_t']) for i in range(uniq)]
        sr = torch.tensor([[i * n, (i + 1) * n] for i in range(B)], dtype=torch.int64).cuda()
        i0, i1 = vis.chunk_bounds(n, N)
        fr = torch.tensor([[s * n + b, s * n + e] for s in range(B) for b, e in zip(i0, i1)], dtype=torch.int64).cuda()
        frame_events = int((fr[:, 1] - fr[:, 0]).sum())
        bands = f'{lib.ec_denoise_bands(H, W, 1)} / {lib.ec_denoise_bands(H, W, 3)}'
        for packed in (False, True):
            parts = [vis.pack_events(s).view(np.int64) if packed else s for s in samples]
            e = torch.from_numpy(np.concatenate(parts)).cuda().repeat((B // uniq + 1,) + (1,) * (parts[0].ndim - 1))[:B * n]
            esz = 8 if packed else 16
            # caller-owned outputs: their allocation is not the kernels' time
            out, counts = torch.empty_like(e), torch.zeros((B,), dtype=torch.int64, device='cuda')
            stats = torch.zeros((B, ctypes.sizeof(vis.EcDenoiseStats)), dtype=torch.uint8, device='cuda')
            prms = {f: vis.denoise_params((H, W), f[1], f[0], n, B * n) for f in FILTERS}
            ws = torch.empty((vis.denoise_workspace_bytes(prms[FILTERS[0]], B),), dtype=torch.uint8, device='cuda')
            entry = 'ec_denoise_events_packed' if packed else 'ec_denoise_events'
            variants = [(f'denoise r {r}, dt {dt // 1000} ms', B * n, 2 * esz * B * n,
                         lambda p=prms[(r, dt)]: _lib.launch(entry, e, sr, B, p, out, counts, None, stats, ws, ws.numel()))
                        for r, dt in FILTERS]
            if not packed:
                zero = torch.zeros((B, 4), dtype=torch.int32, device='cuda')
                variants.append(('augment, zero shift', B * n, 2 * esz * B * n,
                                 lambda: _lib.launch('ec_augment_events', e, sr, B, zero, H, W, out, counts)))
            variants.append((f'histogram frames, N {N}', frame_events, esz * frame_events + 3 * H * W * int(fr.shape[0]),
                             lambda: vis.events_to_frames_device(e, fr, (H, W), max_frame_events=N, total_events=frame_events)))
            kept = {}
            for v, _, _, fn in variants:
                for _ in range(2):
                    fn()
                if v.startswith('denoise'):
                    st = stats.cpu().numpy().view(vis.DENOISE_STATS_DTYPE).reshape(B)
                    kept[v] = f"{100. * st['kept'].sum() / max(1, st['kept'].sum() + st['removed'].sum()):.1f} %"
            torch.cuda.synchronize()
            ms = {v: [] for v, _, _, _ in variants}
            for _ in range(a.rounds):
                for v, _, _, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[v].append(e0.elapsed_time(e1))
            for v, events, alg, _ in variants:
                m = statistics.median(ms[v])
                lines.append(f'| {name} {H}x{W} | {bands} | {n} | {"packed" if packed else "float"} | {v} | {m:.3f} '
                             f'(min {min(ms[v]):.3f}, max {max(ms[v]):.3f}) | {events / m / 1e3:.0f} | {alg / m / 1e6:.0f} | {kept.get(v, "")} |')
                print(lines[-1], flush=True)
            del e, out, ws
    table = '\n'.join(lines) + '\n'
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(table)


if __name__ == '__main__':
    main()
