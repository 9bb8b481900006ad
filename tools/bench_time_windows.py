"""The fixed-duration windows next to the nearest one-pass kernel over the same rows (ec_center_events) and the histogram
frames on the same events (run on the GPU box).

    python tools/bench_time_windows.py [--samples 256] [--rounds 7] [--out profiles/time_windows.jsonl]

Samples of the three dataset geometries at their sample sizes (synthetic.GEOMETRY: max_n events over max_t seconds, sorted),
float rows and packed events, at B = 1 (one recording: the kernel's own use case) and at the bench batch; windows of a
tenth of the sample's span, back to back and hopped by half, from the first event and from the last.  After a warm-up of
every launch the variants of a (geometry, layout, B) are timed in turn, round after round (device events around each
launch, outputs caller-owned), and the median round is reported: ms, events per second, GB/s over the algorithmic bytes
(windows: every event read once + 16 B per row of bounds; center: every event read twice and written once -- its first
pass alone is the comparable read, so its rate over ONE read is given too; frames: 16 / 8 B per event in + 3 H W out).
The first line of the file is the device, its compute units and the shader and memory clocks the box reports.
Every timed launch's bounds are checked against numpy on the first sample before anything is timed.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eventclip_amd import _lib, vis  # noqa: E402
from eventclip_amd.synthetic import GEOMETRY, make_events  # noqa: E402


def box():
    cu = ctypes.c_int(0)
    _lib.check(_lib.lib().ec_device_info(ctypes.byref(cu), None, 0), 'ec_device_info')
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=60)
        clocks = '; '.join(' '.join(ln.split()) for ln in r.stdout.splitlines() if 'sclk' in ln or 'mclk' in ln)[:600]
    except (OSError, subprocess.SubprocessError) as e:
        clocks = f'not read: {e}'
    return dict(device=torch.cuda.get_device_name(), compute_units=cu.value, clocks=clocks, torch=torch.__version__)


def reference(ticks, dt_us, stride_us, from_last, most):
    windows = int((ticks[-1] - ticks[0]) // stride_us + 1)
    k = np.arange(min(windows, most), dtype=np.int64)
    if not from_last:
        lo = ticks[0] + k * stride_us
        return windows, np.stack([np.searchsorted(ticks, lo, 'left'), np.searchsorted(ticks, lo + dt_us, 'left')], 1)
    return windows, np.stack([np.searchsorted(ticks, ticks[-1] - k * stride_us - dt_us, 'right'),
                              np.searchsorted(ticks, ticks[-1] - k * stride_us, 'right')], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=256, help='the bench batch')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    uniq, MW = 8, 64
    records = [dict(box=box(), samples=a.samples, rounds=a.rounds)]
    print(json.dumps(records[0]), flush=True)
    for name in ('n_cars', 'n_caltech', 'n_imagenet'):
        g = GEOMETRY[name]
        (H, W), n, N = g['resolution'], g['max_n'], g['N']
        samples = [make_events(n, (H, W), seed=i, max_t=g['max_t']) for i in range(uniq)]
        dt_us = max(1, int(g['max_t'] * 1e6) // 10)
        i0, i1 = vis.chunk_bounds(n, N)
        for packed in (False, True):
            parts = [vis.pack_events(s).view(np.int64) if packed else s for s in samples]
            ticks0 = (parts[0].view(np.uint64) >> np.uint64(34)).astype(np.int64) if packed else \
                np.clip(np.rint(parts[0][:, 2].astype(np.float64) * 1e6), 0, 2 ** 30 - 1).astype(np.int64)
            esz = 8 if packed else 16
            for B in (1, a.samples):
                e = torch.from_numpy(np.concatenate(parts)).cuda().repeat((B // uniq + 1,) + (1,) * (parts[0].ndim - 1))[:B * n]
                sr = torch.tensor([[i * n, (i + 1) * n] for i in range(B)], dtype=torch.int64).cuda()
                fr = torch.tensor([[s * n + b, s * n + c] for s in range(B) for b, c in zip(i0, i1)], dtype=torch.int64).cuda()
                frame_events = int((fr[:, 1] - fr[:, 0]).sum())
                bounds = torch.full((B, MW, 2), -1, dtype=torch.int64, device='cuda')
                stats = torch.zeros((B, 4), dtype=torch.int32, device='cuda')
                entry = 'ec_time_windows_packed' if packed else 'ec_time_windows'
                scratch = e.clone()                      # centring works in place: on a copy, which it may shift as it likes
                variants = []
                for label, stride_us, from_last in (('windows', dt_us, 0), ('windows, hop 1/2', dt_us // 2, 0), ('windows, from last', dt_us, 1)):
                    prm = vis.time_windows_params(dt_us, stride_us, MW, from_last, B * n)
                    variants.append((label, B * n, esz * B * n + 16 * B * MW,
                                     lambda p=prm: _lib.launch(entry, e, sr, B, p, bounds, stats)))
                    variants[-1][3]()                    # and checked before it is timed
                    windows, ref = reference(ticks0, dt_us, stride_us, from_last, MW)
                    st = stats.cpu().numpy()
                    assert (st[:, 2] == 0).all() and st[0, 3] == windows, (label, st[0])
                    assert np.array_equal(bounds[0, :len(ref)].cpu().numpy(), ref), label
                variants.append(('center (2 reads + 1 write)', B * n, 3 * esz * B * n,
                                 lambda: _lib.launch('ec_center_events_packed' if packed else 'ec_center_events', scratch, sr, B, H, W)))
                variants.append((f'histogram frames, N {N}', frame_events, esz * frame_events + 3 * H * W * int(fr.shape[0]),
                                 lambda: vis.events_to_frames_device(e, fr, (H, W), max_frame_events=N, total_events=frame_events)))
                for _, _, _, fn in variants:
                    for _ in range(2):
                        fn()
                torch.cuda.synchronize()
                ms = {v: [] for v, _, _, _ in variants}
                for _ in range(a.rounds):
                    for v, _, _, fn in variants:
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        fn()
                        t1.record()
                        torch.cuda.synchronize()
                        ms[v].append(t0.elapsed_time(t1))
                for v, events, alg, _ in variants:
                    m = statistics.median(ms[v])
                    rec = dict(geometry=name, resolution=[H, W], events_per_sample=n, layout='packed' if packed else 'float', B=B,
                               variant=v, window_us=dt_us, ms_median=round(m, 4), ms_min=round(min(ms[v]), 4),
                               ms_max=round(max(ms[v]), 4), m_events_per_s=round(events / m / 1e3, 1),
                               algorithmic_bytes=alg, gb_per_s_algorithmic=round(alg / m / 1e6, 1))
                    if v.startswith('center'):
                        rec['gb_per_s_over_one_read'] = round(esz * B * n / m / 1e6, 1)
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
                del e, scratch, bounds
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(''.join(json.dumps(r) + '\n' for r in records))


if __name__ == '__main__':
    main()
