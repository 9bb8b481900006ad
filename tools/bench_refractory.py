"""The refractory-period filter next to the background-activity filter, the other read-and-compact kernel
(ec_augment_events) and the histogram frames on the same events (run on the GPU box).

    python tools/bench_refractory.py [--samples 256] [--rounds 7] [--out profiles/refractory.jsonl]

Samples of the three dataset geometries at their sample sizes (synthetic.GEOMETRY: max_n events over max_t seconds),
float rows and packed events; the filter with periods of 1 ms and 10 ms, pixel-wide and per polarity.  After a warm-up of
every launch the variants of a (geometry, layout) are timed in turn, round after round (device events around each launch),
and the median round is reported with its smallest and largest: ms, events per second, GB/s over the algorithmic bytes
(every event read once and at most written once; the frames: 16 / 8 per event in plus 3 H W per frame out), and the share
of counted events a filter keeps.  ec_denoise_events runs at radius 1, dt 5 ms; ec_augment_events takes float rows only and
runs with a zero shift (nothing dropped).  All outputs and workspaces are the caller's, allocated before the timed window.
Prints one JSON record per line; --out also writes them to a file.
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

FILTERS = ((1000, False), (1000, True), (10000, False), (10000, True))      # (period_us, per_polarity)


def box():
    cu = ctypes.c_int(0)
    _lib.check(_lib.lib().ec_device_info(ctypes.byref(cu), None, 0), 'ec_device_info')
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=60)
        clocks = '; '.join(' '.join(ln.split()) for ln in r.stdout.splitlines() if 'sclk' in ln or 'mclk' in ln)[:600]
    except (OSError, subprocess.SubprocessError) as e:
        clocks = f'not read: {e}'
    return dict(device=torch.cuda.get_device_name(), compute_units=cu.value, clocks=clocks, torch=torch.__version__)


def kept_share(stats, dtype, B):
    st = stats.cpu().numpy().view(dtype).reshape(B)
    return float(st['kept'].sum()) / max(1, int(st['kept'].sum() + st['removed'].sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    uniq, B = 8, a.samples
    records = [dict(box=box(), samples=B, rounds=a.rounds, long_list=vis.REFRACTORY_LONG_LIST)]
    print(json.dumps(records[0]), flush=True)
    for name in ('n_cars', 'n_caltech', 'n_imagenet'):
        g = GEOMETRY[name]
        (H, W), n, N = g['resolution'], g['max_n'], g['N']
        samples = [make_events(n, (H, W), seed=i, max_t=g['max_t']) for i in range(uniq)]
        sr = torch.tensor([[i * n, (i + 1) * n] for i in range(B)], dtype=torch.int64).cuda()
        i0, i1 = vis.chunk_bounds(n, N)
        fr = torch.tensor([[s * n + b, s * n + e] for s in range(B) for b, e in zip(i0, i1)], dtype=torch.int64).cuda()
        frame_events = int((fr[:, 1] - fr[:, 0]).sum())
        bands = {pp: vis.refractory_bands((H, W), pp) for pp in (False, True)}
        for packed in (False, True):
            parts = [vis.pack_events(s).view(np.int64) if packed else s for s in samples]
            e = torch.from_numpy(np.concatenate(parts)).cuda().repeat((B // uniq + 1,) + (1,) * (parts[0].ndim - 1))[:B * n]
            esz = 8 if packed else 16
            out, counts = torch.empty_like(e), torch.zeros((B,), dtype=torch.int64, device='cuda')
            stats = torch.zeros((B, ctypes.sizeof(vis.EcRefractoryStats)), dtype=torch.uint8, device='cuda')
            prms = {f: vis.refractory_params((H, W), f[0], f[1], n, B * n) for f in FILTERS}
            ws = torch.empty((max(vis.refractory_workspace_bytes(p, B) for p in prms.values()),), dtype=torch.uint8, device='cuda')
            entry = 'ec_refractory_events_packed' if packed else 'ec_refractory_events'
            variants = [(f"refractory {us // 1000} ms, {'per polarity' if pp else 'pixel-wide'}", B * n, 2 * esz * B * n, bands[pp],
                         lambda p=prms[(us, pp)]: _lib.launch(entry, e, sr, B, p, out, counts, None, stats, ws, ws.numel()))
                        for us, pp in FILTERS]
            dprm = vis.denoise_params((H, W), 5000, 1, n, B * n)
            dws = torch.empty((vis.denoise_workspace_bytes(dprm, B),), dtype=torch.uint8, device='cuda')
            dentry = 'ec_denoise_events_packed' if packed else 'ec_denoise_events'
            variants.append(('denoise r 1, dt 5 ms', B * n, 2 * esz * B * n, _lib.lib().ec_denoise_bands(H, W, 1),
                             lambda: _lib.launch(dentry, e, sr, B, dprm, out, counts, None, stats, dws, dws.numel())))
            if not packed:
                zero = torch.zeros((B, 4), dtype=torch.int32, device='cuda')
                variants.append(('augment, zero shift', B * n, 2 * esz * B * n, None,
                                 lambda: _lib.launch('ec_augment_events', e, sr, B, zero, H, W, out, counts)))
            variants.append((f'histogram frames, N {N}', frame_events, esz * frame_events + 3 * H * W * int(fr.shape[0]), None,
                             lambda: vis.events_to_frames_device(e, fr, (H, W), max_frame_events=N, total_events=frame_events)))
            kept = {}
            for v, _, _, _, fn in variants:
                for _ in range(2):
                    fn()
                if v.startswith(('refractory', 'denoise')):         # (the two stats structs have the same three words)
                    kept[v] = kept_share(stats, vis.REFRACTORY_STATS_DTYPE, B)
            torch.cuda.synchronize()
            ms = {v: [] for v, *_ in variants}
            for _ in range(a.rounds):
                for v, _, _, _, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[v].append(e0.elapsed_time(e1))
            for v, events, alg, nb, _ in variants:
                m = statistics.median(ms[v])
                rec = dict(geometry=name, H=H, W=W, events_per_sample=n, layout='packed' if packed else 'float', variant=v,
                           bands=nb, ms_median=round(m, 4), ms_min=round(min(ms[v]), 4), ms_max=round(max(ms[v]), 4),
                           mevents_per_s=round(events / m / 1e3), gbps_algorithmic=round(alg / m / 1e6),
                           kept=None if v not in kept else round(kept[v], 4))
                records.append(rec)
                print(json.dumps(rec), flush=True)
            del e, out, ws, dws
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(''.join(json.dumps(r) + '\n' for r in records))


if __name__ == '__main__':
    main()
