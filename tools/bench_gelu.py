"""The price of the exact GELU (cfg['activation'] = 'gelu', ec_gemm_args.activation = 1) against QuickGELU on the MI355X.

    python tools/bench_gelu.py [--frames 2560] [--arch ViT-L/14] [--launches 50] [--rounds 7] [--steps 3] [--out FILE]

Two measurements, each with the two activations INTERLEAVED in one process (round by round, so that clock and neighbour
drift hits both alike) and reported as the median over the rounds with the spread (min .. max):
  * c_fc at the bench shape: ec_gemm, EC_EPI_GELU16, M = frames x 257, N = 4096, K = 1024, f16; a round is `launches`
    back-to-back launches between two device events;
  * one ViT-L/14 step of `frames` frames through encode_patches (the default folded chain: EC_EPI_GELU16_LN), one model
    per activation on the same seeded weights and patches; a round is `steps` steps between two device events.
Synthetic operands (seeded; no checkpoints on the box).  Every shape is warmed up before it is timed.  Prints one JSON
line; --out also writes it to a file.  No GPU: fails (there is no CPU fallback and a CPU time would say nothing)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ACTS = ('quick_gelu', 'gelu')


def _timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def interleaved(fns, per_round, rounds):
    """fns: {name: callable}.  -> {name: summary of the per-call ms over the rounds}; the names alternate inside a round."""
    for fn in fns.values():                     # warm-up: code objects, the persistent kernel's LDS opt-in, allocator
        _timed(fn, 2)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(_timed(fn, per_round))
    return {k: _summary(v) for k, v in ms.items()}


def bench_c_fc(frames, launches, rounds):
    from eventclip_amd import ops
    M, N, K = frames * 257, 4096, 1024
    g = torch.Generator(device='cuda').manual_seed(0)
    A = torch.randn(M, K, device='cuda', generator=g).half()
    W = (torch.randn(N, K, device='cuda', generator=g) * K ** -0.5).half()
    bias = torch.randn(N, device='cuda', generator=g) - 1.0
    out = torch.empty(M, N, dtype=torch.float16, device='cuda')
    res = interleaved({a: (lambda a=a: ops.gemm(A, W, bias, 'gelu16', out=out, activation=a)) for a in ACTS}, launches, rounds)
    flops = 2.0 * M * N * K
    for a in ACTS:
        res[a]['tflops'] = round(flops / (res[a]['median_ms'] * 1e-3) / 1e12, 1)
    return dict(M=M, N=N, K=K, launches_per_round=launches, rounds=rounds, **res,
                gelu_over_quick=round(res['gelu']['median_ms'] / res['quick_gelu']['median_ms'], 4))


def bench_step(arch, frames, steps, rounds):
    from eventclip_amd import clip as eclip
    cfg = eclip.arch_config(arch)
    sd = eclip.random_state_dict(cfg, seed=0)
    models = {a: eclip.CLIP(dict(cfg, activation=a), sd, dtype='float16', chunk=frames).cuda().eval() for a in ACTS}
    m = models['quick_gelu']
    G = (cfg['image_size'] // cfg['patch']) ** 2
    k = 3 * cfg['patch'] ** 2
    g = torch.Generator(device='cuda').manual_seed(1)
    patches = (torch.randn(frames, G, m.kpad, device='cuda', generator=g) * 0.5).half()
    patches[:, :, 2 * k:] = 0
    res = interleaved({a: (lambda a=a: models[a].encode_patches(patches)) for a in ACTS}, steps, rounds)
    for a in ACTS:
        res[a]['frames_per_s'] = round(frames / (res[a]['median_ms'] * 1e-3), 1)
    return dict(arch=arch, frames=frames, steps_per_round=steps, rounds=rounds, **res,
                gelu_over_quick=round(res['gelu']['median_ms'] / res['quick_gelu']['median_ms'], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2560)
    ap.add_argument('--arch', default='ViT-L/14')
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from eventclip_amd import _lib
    _lib.require_gpu()
    row = dict(tool='bench_gelu', device=torch.cuda.get_device_name(0), c_fc=bench_c_fc(a.frames, a.launches, a.rounds),
               step=bench_step(a.arch, a.frames, a.steps, a.rounds))
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
