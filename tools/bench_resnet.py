"""ResNet CLIP image towers on one MI355X: HIP tower against torch's own fp16 channels_last forward (MIOpen).

    python tools/bench_resnet.py [--archs RN50,RN101] [--frames 2560] [--out profiles/resnet_bench.json]

Per arch: frames/s and ms per step of ResNetCLIP.encode_image over --frames normalised images (RN50x64: a quarter of
them), a per-kernel-class table from ec_profile_* (TFLOP/s and the fraction of the 2.5 PFLOP/s dense 16-bit MFMA peak;
HBM fraction of 8 TB/s for the stem rows and pooling), and the same module in torch fp16 channels_last (the restatement
of tests/resnet_ref.py) on the same GPU with its time and its max-normalised error against fp32, next to the HIP
tower's.  Weights are calibrated random weights (eventclip_amd.clip.random_state_dict).

    python tools/bench_resnet.py --precise-blocks all[,N...] [--layers 1,1,1,1] [--precise-out profiles/resnet_precise.txt]

prices the split-precision form instead: per arch, ms per --frames images of the default path and of each count in the
same process (every model warmed up, --reps timed passes each, median and min .. max), the ratio to the default, and the
max-normalised error of each against the float64 restatement on the inputs of tests/test_resnet_precise_gpu.py (16
images, weight seeds 0 and 1; --err-seeds adds held-out ones)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def bench(arch, frames, chunk):
    import resnet_ref
    from eventclip_amd import _lib, resnet
    from eventclip_amd import clip as eclip
    cfg = eclip.resnet_config(arch)
    sd = eclip.random_state_dict(cfg, seed=0)
    m = resnet.ResNetCLIP(cfg, sd, chunk=chunk).cuda().eval()
    R = cfg['image_size']
    x = torch.randn(frames, 3, R, R, generator=torch.Generator().manual_seed(0)).cuda()
    t_hip = timed(lambda: m.encode_image(x), 2)
    _lib.profile_begin()
    m.encode_image(x)
    torch.cuda.synchronize()
    prof = _lib.profile_end()
    table = []
    for p in prof:
        row = dict(kernel=p['name'], launches=p['launches'], ms=round(p['total_ms'], 3))
        if p['flops']:
            row['tflops'] = round(p['flops'] / p['total_ms'] / 1e9, 1)
            row['mfma_peak_frac'] = round(p['flops'] / p['total_ms'] * 1e3 / PEAK_FLOPS, 3)
        if p['bytes']:
            row['hbm_frac'] = round(p['bytes'] / p['total_ms'] * 1e3 / PEAK_BYTES, 3)
        table.append(row)
    ref = resnet_ref.from_state_dict(sd, cfg)
    xs = x[:2].cpu()
    with torch.no_grad():
        want = ref(xs)
    err_hip = float((m.encode_image(xs.cuda()).cpu() - want).abs().max() / want.abs().max())
    tm = ref.cuda().half().to(memory_format=torch.channels_last)
    xh = x.half().contiguous(memory_format=torch.channels_last)

    def torch_fwd():
        with torch.no_grad():
            for i in range(0, frames, chunk):
                tm(xh[i:i + chunk])
    t_torch = timed(torch_fwd, 2)
    with torch.no_grad():
        err_torch = float((tm(xh[:2]).float().cpu() - want).abs().max() / want.abs().max())
    flops = resnet.resnet_flops(cfg) * frames
    return dict(arch=arch, frames=frames, chunk=chunk, hip_ms=round(t_hip * 1e3, 2),
                hip_frames_per_s=round(frames / t_hip, 1), hip_tflops=round(flops / t_hip / 1e12, 1),
                torch_fp16_ms=round(t_torch * 1e3, 2), torch_over_hip=round(t_torch / t_hip, 3),
                err_hip=err_hip, err_torch_fp16=err_torch,
                padded_flop_overhead=round(resnet.padded_flop_overhead(cfg), 4), kernels=table)


def bench_precise(arch, frames, chunk, counts, reps, layers, err_seeds, say):
    import statistics
    import resnet_ref
    from eventclip_amd import resnet
    from eventclip_amd import clip as eclip
    cfg = eclip.resnet_config(arch, **({'vision_layers': layers} if layers else {}))
    nb = sum(cfg['vision_layers'])
    counts = [0] + sorted({nb if c == 'all' else min(int(c), nb) for c in counts} - {0})
    R = cfg['image_size']
    x = torch.randn(frames, 3, R, R, generator=torch.Generator().manual_seed(0)).cuda()
    sd0 = eclip.random_state_dict(cfg, seed=0)
    ms = {}
    for c in counts:
        m = resnet.ResNetCLIP(cfg, sd0, chunk=chunk, precise_blocks=c).cuda().eval()
        for _ in range(2):
            m.encode_image(x)
        ts = [timed(lambda: m.encode_image(x), 1) * 1e3 for _ in range(reps)]
        ms[c] = (statistics.median(ts), min(ts), max(ts))
        del m
    errs = {c: [] for c in counts}
    floors = []
    for seed in err_seeds:
        sd = sd0 if seed == 0 else eclip.random_state_dict(cfg, seed=seed)
        xs = torch.randn(16, 3, R, R, generator=torch.Generator().manual_seed(100 + seed))
        ref_m = resnet_ref.from_state_dict(sd, cfg)
        with torch.no_grad():
            ref32 = ref_m(xs).double()
            ref = ref_m.double()(xs.double())
        floors.append(float((ref32 - ref).abs().max() / ref.abs().max()))
        for c in counts:
            m = resnet.ResNetCLIP(cfg, sd, precise_blocks=c).cuda().eval()
            got = m.encode_image(xs.cuda()).cpu().double()
            errs[c].append(float((got - ref).abs().max() / ref.abs().max()))
            del m
    say(f'{arch} layers={cfg["vision_layers"]} ({nb} blocks), {frames} images, chunk {chunk}, {reps} timed passes; '
        f'error against float64 on seeds {list(err_seeds)}; fp32 restatement: ' + ' '.join(f'{e:.2e}' for e in floors))
    for c in counts:
        med, lo, hi = ms[c]
        say(f'  precise_blocks={c:3d}  {med:9.2f} ms (min {lo:.2f} .. max {hi:.2f})  x{med / ms[0][0]:.2f} of default   err '
            + ' '.join(f'{e:.2e}' for e in errs[c]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--archs', default='RN50,RN101,RN50x4,RN50x16,RN50x64')
    ap.add_argument('--frames', type=int, default=2560)
    ap.add_argument('--chunk', type=int, default=128)
    ap.add_argument('--out', default=None)
    ap.add_argument('--precise-blocks', default=None, help="counts to price, e.g. 'all' or '4,8,all'")
    ap.add_argument('--layers', default=None, help='vision_layers override for --precise-blocks, e.g. 1,1,1,1')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--err-seeds', default='0,1')
    ap.add_argument('--precise-out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.precise_blocks:
        lines = []

        def say(t):
            print(t, flush=True)
            lines.append(t)
        layers = tuple(int(v) for v in a.layers.split(',')) if a.layers else None
        for arch in a.archs.split(','):
            n = a.frames // 4 if arch == 'RN50x64' else a.frames
            bench_precise(arch, n, a.chunk, a.precise_blocks.split(','), a.reps, layers,
                          [int(v) for v in a.err_seeds.split(',')], say)
        if a.precise_out:
            os.makedirs(os.path.dirname(os.path.abspath(a.precise_out)), exist_ok=True)
            with open(a.precise_out, 'a') as f:
                f.write('\n'.join(lines) + '\n')
        return
    res = []
    for arch in a.archs.split(','):
        n = a.frames // 4 if arch == 'RN50x64' else a.frames
        r = bench(arch, n, a.chunk)
        res.append(r)
        print(json.dumps({k: v for k, v in r.items() if k != 'kernels'}), flush=True)
        for row in r['kernels']:
            print('   ', json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
