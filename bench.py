"""Headline benchmark: event-frames/sec through the whole hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One step = one batch of the BASELINE.json config "N-Caltech101 zero-shot, ViT-L/14,
RGB-polarity event2img, batch=256" (SURVEY.md 8(d) C2): raw events already resident
in HBM -> histogram frames -> CLIP preprocess -> ViT-L/14 image tower -> logits against
the cached text features -> per-sample aggregation (-> RCCL all-gather of the logits
when N > 1).  Every sample has 10 x 20000 events, i.e. 10 valid views, so a step
pushes 2560 frames per GPU; weak scaling (each rank gets its own 256 samples).
Weights are seeded random (no checkpoints ship), data is synthetic.

`--config 2|3|4` runs the other BASELINE.json configs through the same step (default 1 = the line above):
2 = N-Cars few-shot adapter, ViT-L/14, 512 samples per GPU (weak scaling, like 1); 3 = N-ImageNet zero-shot,
ViT-L/14@336px, GLOBAL batch 2048 x 2 views; 4 = N-ImageNet few-shot adapter, ViT-L/14, GLOBAL batch 4096 x 5
views -- 3 and 4 split their global batch over the ranks (harness.shard_range: strong scaling, as BASELINE words
them: "DP-sharded across 8").  The line also carries every rank's own ms per step and the time the all-gather
of the logits took on rank 0's stream.

Rank 0 prints one JSON line; `roofline` comes from HIP events the library records
around its own launches during the timed steps.  `--dump-outputs DIR` writes what the
last timed step returned (rank 0's out_dict) as DIR/<name>.npy: the inputs are seeded,
so two builds run with the same arguments can be compared output for output.

A plain run sets up, warms up, times the steps, dumps and prints: nothing else.  `--full`
adds, on one GPU and after the timed region (never part of `value`), what `extras` lists:
the host-fed steps, clock / power sampling, the tolerance mode's price, the strict
pipeline's price, `cpu_baseline` (the CPU oracle, test infrastructure, timed on a bounded
sample on the host) and BASELINE configs[2..4] as `other_configs`.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_MFMA_TFLOPS = 2500.0   # dense bf16/f16 MFMA, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0       # HBM3E spec, MI355X_MICROARCH.md
MFMA_KERNELS = ('gemm_kernel', 'attention_kernel')


# BASELINE.json configs[1..4].  batch: samples per step -- per GPU where scaling is
# 'weak', over the whole job where it is 'strong'; n_ev: events per sample (T views of N, or fewer than N)
CONFIGS = {
    1: dict(name='N-Caltech101 zero-shot, {arch}, RGB-polarity event2img', geo='n_caltech', arch='ViT-L/14',
            batch=256, T=10, n_ev=200000, K=101, adapter=None, max_n=None, grayscale=False, scaling='weak'),
    2: dict(name='N-Cars few-shot (text-trans adapter), {arch}, gray event2img', geo='n_cars', arch='ViT-L/14',
            batch=512, T=1, n_ev=12500, K=2, adapter=0.8, max_n=None, grayscale=True, scaling='weak'),
    3: dict(name='N-ImageNet zero-shot, {arch}, gray event2img', geo='n_imagenet', arch='ViT-L/14@336px',
            batch=2048, T=2, n_ev=140000, K=1000, adapter=None, max_n=None, grayscale=True, scaling='strong'),
    4: dict(name='N-ImageNet few-shot (text-trans adapter), {arch}, T=5 event frames', geo='n_imagenet',
            arch='ViT-L/14', batch=4096, T=5, n_ev=350000, K=1000, adapter=0.95, max_n=350000, grayscale=True,
            scaling='strong'),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--config', type=int, default=1, choices=sorted(CONFIGS),
                    help='BASELINE.json configs[i]; 1 (default) is the headline line')
    ap.add_argument('--steps', type=int, default=5, help='timed steps (>= 1)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=None,
                    help='samples per step: per GPU for configs 1 / 2, over all GPUs for 3 / 4 (default: the config\'s)')
    ap.add_argument('--arch', default=None, help='default: the config\'s')
    ap.add_argument('--dtype', default='float16', choices=['float16', 'bfloat16'])
    ap.add_argument('--chunk', type=int, default=2560, help='frames per pass through the tower')
    ap.add_argument('--classes', type=int, default=None, help='default: the config\'s')
    ap.add_argument('--unique-samples', type=int, default=None,
                    help='distinct synthetic event streams per rank, tiled to the batch (default: the batch for config 1, else 16)')
    ap.add_argument('--cpu-baseline-samples', type=int, default=3)
    ap.add_argument('--cpu-baseline-frames', type=int, default=10, help='views per baseline sample')
    ap.add_argument('--packed-events', action='store_true',
                    help='feed the 8-byte packed event form (SURVEY 8(f)) instead of float32 [n, 4]')
    ap.add_argument('--full', action='store_true',
                    help='also measure, after the timed region, what the headline does not need (single GPU): '
                         'value_from_host, dvfs, tolerance_mode, ms_per_step_strict, cpu_baseline, other_configs; '
                         'each --no-* option below drops one of them')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without cpu_baseline')
    ap.add_argument('--from-host', action='store_true',
                    help='also time the step with every batch starting in HOST memory (pinned staging ring + copy '
                         'stream, the upload of batch i + 1 under the tower of batch i): value_from_host')
    ap.add_argument('--no-from-host', action='store_true', help='--full without the host-fed steps')
    ap.add_argument('--no-other-configs', action='store_true',
                    help='--full without BASELINE configs[2..4] at their per-GPU shards: other_configs')
    ap.add_argument('--no-strict-line', action='store_true', help='--full without the 3 steps with pipe.strict = True: ms_per_step_strict')
    ap.add_argument('--no-dvfs', action='store_true', help='--full without the clock / power sampling steps')
    ap.add_argument('--precise', action='store_true',
                    help='image tower with hi + lo operands in every GEMM (ec_vit_weights.precise, 3 x the MFMA work): '
                         'the mode that meets 1e-3 on input-dependent weights; a line of its own, never the headline')
    ap.add_argument('--f16-weights', action='store_true',
                    help='round the seeded random weights to 16 bit first: a checkpoint stored in 16 bit, as released CLIP '
                         'weights are (split-precision blocks then skip the product with the weights\' lo parts)')
    ap.add_argument('--precise-blocks', type=int, default=0,
                    help='the FIRST n blocks of the image tower as split-operand blocks (ec_vit_weights.precise_blocks; '
                         'n = 8 meets 1e-3 on the input-dependent weights of every config): a line of its own, never the headline')
    ap.add_argument('--tolerance-mode', action='store_true',
                    help='time the headline config IN the tolerance mode (eventclip_amd.clip.TOLERANCE_MODE): a line of its own, never the headline')
    ap.add_argument('--no-tolerance-mode', action='store_true',
                    help='--full without the extra steps that price the 1e-3 mode: tolerance_mode')
    ap.add_argument('--other-configs-batch', type=int, default=None,
                    help='samples per step of each of other_configs (tests; default: the per-GPU shard of BASELINE\'s batch)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write the arrays the last one returned (rank 0) as DIR/<name>.npy, '
                         'float32 (float64 where computed so), at most 64 MB in all (a fixed, seeded sample of rows beyond)')
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error(f'--steps must be >= 1 and --warmup >= 0 (got {a.steps}, {a.warmup})')
    a.arch_given, a.classes_given = a.arch, a.classes        # overrides (tests) also apply to other_configs
    c = CONFIGS[a.config]
    a.batch = a.batch or c['batch']
    a.arch = a.arch or c['arch']
    a.classes = a.classes or c['K']
    return a


def extras(a, world):
    """The keys of what this run measures besides its headline, all of it after the timed region.  A plain run adds
    only what --from-host asks for; --full adds the rest on one GPU, less what the --no-* options drop and what does not
    apply to a line of its own (--precise, --precise-blocks, --tolerance-mode, --f16-weights)."""
    run = {'value_from_host'} if a.from_host else set()
    if not a.full or world > 1:
        return run
    headline = a.config == 1
    split = a.precise or a.precise_blocks or a.tolerance_mode
    wanted = {'value_from_host': headline and not a.no_from_host,
              'dvfs': not a.no_dvfs,
              'tolerance_mode': headline and not (a.no_tolerance_mode or split),
              'ms_per_step_strict': not a.no_strict_line,
              'cpu_baseline': not a.no_cpu_baseline,
              'other_configs': headline and not (a.no_other_configs or split or a.f16_weights)}
    return run | {k for k, on in wanted.items() if on}


DUMP_LIMIT_BYTES = 64 << 20      # --dump-outputs: bytes in all, .npy headers included
NPY_HEADER_BYTES = 4096          # an upper bound of one .npy header


def dump_outputs(out, path, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every tensor of the step's out_dict as path/<name>.npy -- float64 stays float64, everything else
    (logits, probs, the boolean valid_masks as 0 / 1) is written as float32.  When the arrays exceed `limit` bytes in all,
    each keeps the same fraction of its rows (first axis), drawn by a fixed seed from the shapes alone, so that runs of
    two builds with the same arguments write the same rows.  Returns {name: (shape as computed, rows written)}."""
    arrays = {}
    for name, v in sorted(out.items()):
        if torch.is_tensor(v):
            t = v.detach().cpu()
            arrays[name] = (t.double() if t.dtype == torch.float64 else t.float()).numpy()
    rowed = sum(x.nbytes for x in arrays.values() if x.ndim)
    budget = limit - NPY_HEADER_BYTES * len(arrays) - sum(x.nbytes for x in arrays.values() if not x.ndim)
    frac = budget / rowed if rowed > budget else 1.0
    os.makedirs(path, exist_ok=True)
    written = {}
    for name, x in arrays.items():
        shape = list(x.shape)
        if frac < 1.0 and x.ndim:
            assert int(x.shape[0] * frac) >= 1, f'{name} {shape}: a single row exceeds the --dump-outputs limit'
            rows = np.random.default_rng(0).choice(x.shape[0], int(x.shape[0] * frac), replace=False)
            x = x[np.sort(rows)]
        np.save(os.path.join(path, name + '.npy'), x)
        written[name] = (shape, x.shape[0] if x.ndim else None)
    return written


def _cpu_event2img(args):
    """One sample through the CPU event2img stage (what a DataLoader worker of the reference does,
    datasets/event2img.py:114-128): events -> frames -> CLIP preprocess.  Returns the frame count."""
    ev, qa, n_px, shape = args
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import events as oe
    from oracle import preprocess as op
    frames = oe.events2frames(ev, 'event_count', 'event_histogram', shape=tuple(shape), **qa)
    op.preprocess(frames, n_px)
    return frames.shape[0]


def tolerance_mode(a, cfg, sd, clip_dict, step, fence, pipe, events, n_events, frames_per_step, default_ms):
    """The price of north_star's 1e-3 on input-dependent weights, measured AFTER the timed region on the same box and
    batch (never part of `value`): the image tower in the tolerance mode (eventclip_amd.clip.TOLERANCE_MODE: the first
    blocks as split-operand blocks, ec_vit_weights.precise_blocks / precise_attn_blocks -- the settings
    tests/test_configs_gpu.py::test_tolerance_mode_meets_1e3_over_draws holds to 1e-3 on three (weights, events) draws per
    BASELINE config and profiles/r6_parity_seeds.txt measures on eight), a few steps each on the run's own weights and
    on the same weights rounded to 16 bit first (what a released checkpoint is: the lo products of the exact matrices
    are skipped), interleaved with steps of the default model."""
    from eventclip_amd import clip as eclip
    from eventclip_amd.clip_cls import ZSCLIPClassifier
    cdt = torch.float16 if a.dtype == 'float16' else torch.bfloat16
    if cdt != torch.float16:
        return None
    sd16 = {k: (v.to(cdt).float() if v.dim() >= 2 else v) for k, v in sd.items()}
    kw = eclip.tolerance_mode_kwargs(cfg)
    pb, pa = kw['image_precise_blocks'], kw['image_precise_attn_blocks']
    out = {'precise_blocks': pb, 'precise_attn_blocks': pa, 'steps': 3,
           'settings': {'up_to_288_tokens': list(eclip.TOLERANCE_MODE[0]), 'beyond': list(eclip.TOLERANCE_MODE[1])},
           'configs_within_1e3': parity_seeds_summary(),
           'what': f'first {pb} image-tower blocks as split-operand blocks: LayerNorm of both planes of the residual stream into '
                   'hi + lo parts, QKV / c_fc multiply both parts, every GEMM adds the product with its weight\'s lo part '
                   f'(one launch per GEMM; none where the matrix is its 16-bit value); the first {pa} of them with attention in '
                   'fp32 on hi + lo q, k, v and the MLP activation as hi + lo into c_proj '
                   '(ec_vit_weights.precise_blocks / precise_attn_blocks)' +
                   ('; the lo products of QKV / c_fc / c_proj as e4m3 operands on v_mfma_scale_f32_16x16x128_f8f6f4 (ec_vit_weights.lo_fp8)'
                    if eclip.DEFAULT_LO_FP8 else ''),
           'lo_fp8': bool(eclip.DEFAULT_LO_FP8)}

    def timed(fn, n):
        fence()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        fence()
        return (time.perf_counter() - t0) / n * 1e3

    lines = []
    for name, weights in (('as_run', sd), ('rounded_to_16_bit', sd16)):
        if name == 'as_run' and a.f16_weights:
            continue
        m = eclip.CLIP(cfg, weights, dtype=a.dtype, chunk=a.chunk, **kw).cuda().eval()
        cls = ZSCLIPClassifier(clip_dict=dict(clip_dict, clip_model=m)).cuda().eval()
        cls.get_text_feats()

        def tol_step():
            return cls(pipe(events, n_events))
        tol_step()                                   # packs the weights, warms the workspace
        ms_tol = timed(tol_step, out['steps'])
        ms_def = timed(step, out['steps'])           # the default model right behind it: same clock state
        lines.append({'weights': name, 'ms_per_step': ms_tol, 'value': frames_per_step / ms_tol * 1e3,
                      'default_ms_per_step_interleaved': ms_def, 'ratio_to_default': ms_tol / ms_def})
        del cls, m
        torch.cuda.empty_cache()
    out['lines'] = lines
    return out


def parity_seeds_summary():
    """What profiles/r6_parity_seeds.json (tools/sweep_tolerance.py --seeds 8 --json) measured for the shipped
    tolerance-mode settings: per BASELINE config the median and the WORST of the eight (weight seed, event seed) draws of
    full_logits' max-normalised error against the fp32 oracle, and how many draws are inside 1e-3 -- next to the same for
    the default path, for the same draws on weights rounded to 16 bit, and for eight HELD-OUT draws per config that no setting
    was chosen on.  A measurement made in the build round, quoted here; not re-measured by this run."""
    path = os.path.join(ROOT, 'profiles', 'r6_parity_seeds.json')
    if not os.path.exists(path):
        return 'profiles/r6_parity_seeds.json missing: not measured'
    out = dict(json.load(open(path)), source='profiles/r6_parity_seeds.json (+ .txt: every draw)')
    p16 = os.path.join(ROOT, 'profiles', 'r6_parity_seeds_16bit_weights.json')
    if os.path.exists(p16):      # the same draws on weights rounded to 16 bit first (what a released checkpoint is)
        out['on_weights_rounded_to_16_bit'] = dict(json.load(open(p16))['settings'], source='profiles/r6_parity_seeds_16bit_weights.json')
    ph = os.path.join(ROOT, 'profiles', 'r6_parity_seeds_held_out.json')
    if os.path.exists(ph):       # eight more draws per config that no setting was chosen on
        out['held_out_draws_8_to_15'] = dict(json.load(open(ph))['settings'], source='profiles/r6_parity_seeds_held_out.json')
    ph16 = os.path.join(ROOT, 'profiles', 'r6_parity_seeds_16bit_weights_held_out.json')
    if os.path.exists(ph16):     # ... and those held-out draws on weights rounded to 16 bit
        out['held_out_draws_8_to_15_on_16_bit_weights'] = dict(json.load(open(ph16))['settings'],
                                                               source='profiles/r6_parity_seeds_16bit_weights_held_out.json')
    return out


def cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def cpu_baseline(cfg, sd, tokens, events, quantize_args, n_samples, max_frames, workers=16, shape=(180, 240),
                 pool=True, max_classes=None):
    """The CPU oracle chain on a bounded sample of the same workload (rank 0, N=1 only), plus the
    event2img stage alone in one process and in a pool of `workers` processes, the way the
    reference's DataLoader runs it (num_workers=16, configs/zsclip/zsclip_nin_params.py:15).
    shape = the config's sensor (synthetic.GEOMETRY); the few-shot configs' adapter (0.01 % of the flops) is left out of the
    CPU chain, the zero-shot tail stands in for it; pool=False skips the worker-pool number (other_configs)."""
    import multiprocessing as mp
    from oracle import classify as oc
    from oracle import clip_ref
    from oracle import events as oe
    from oracle import preprocess as op
    oe.build()
    threads = min(os.cpu_count() or 1, 64)   # more threads than this slow torch's CPU GEMMs down
    torch.set_num_threads(threads)
    qa = {k: v for k, v in quantize_args.items()
          if k not in ('max_imgs', 'split_method', 'convert_method')}
    # (the text features are cached by the reference too -- outside the timed sample; other_configs computes them for a few
    # classes only: the CPU text tower over 1000 prompts is ~20 s of wall time that measures nothing)
    if max_classes is not None:
        tokens = tokens[:max_classes]
    text = torch.nn.functional.normalize(clip_ref.encode_text(sd, cfg, tokens), dim=-1)  # cached
    t0 = time.perf_counter()
    n_frames = 0
    for ev in events[:n_samples]:
        ev = ev[:max_frames * qa['N']]
        frames = oe.events2frames(ev, 'event_count', 'event_histogram', shape=tuple(shape), **qa)
        imgs = torch.from_numpy(op.preprocess(frames, cfg['image_size']))
        feats = clip_ref.encode_image(sd, cfg, imgs)
        valid = torch.ones(1, frames.shape[0], dtype=torch.bool)
        oc.zs_forward(feats, valid, text, 100.0, 'mean')
        n_frames += frames.shape[0]
    dt = time.perf_counter() - t0
    res = {'value': n_frames / dt, 'unit': 'frames/s', 'cores': threads, 'kind': 'port',
           'cpu_model': cpu_model(), 'host_cores': os.cpu_count(),
           'sample': f'{n_samples} sample(s) cut to {n_frames} frames of the same workload through the '
                     f'CPU oracle (C events2frames + numpy Pillow-bicubic + torch fp32 '
                     f'{threads}-thread ViT), {dt:.1f} s'}
    # event2img stage alone: one process, then a worker pool.  'spawn', not 'fork': the parent holds a HIP
    # context, runtime threads and a 64-thread OpenMP pool, and a forked child can inherit a lock one of those
    # threads held; every wait has a timeout, so a stuck worker costs the pool number, not the bench line
    jobs = [(np.ascontiguousarray(ev[:max_frames * qa['N']]), qa, cfg['image_size'], tuple(shape))
            for ev in events[:max(n_samples, 2)]]
    t0 = time.perf_counter()
    single = sum(_cpu_event2img(j) for j in jobs)
    res['event2img_frames_per_s_1proc'] = single / (time.perf_counter() - t0)
    if not pool:
        return res
    try:
        workers = min(workers, os.cpu_count() or 1)
        pool_jobs = [jobs[i % len(jobs)] for i in range(2 * workers)]
        with mp.get_context('spawn').Pool(workers) as pool:
            pool.map_async(_cpu_event2img, pool_jobs[:workers]).get(timeout=180)   # start the workers, build caches
            t0 = time.perf_counter()
            done = sum(pool.map_async(_cpu_event2img, pool_jobs).get(timeout=180))
            res[f'event2img_frames_per_s_pool{workers}'] = done / (time.perf_counter() - t0)
    except Exception as e:   # noqa: BLE001 -- a baseline must never take the bench line down
        res['event2img_pool_error'] = repr(e)
    return res


def _amdgpu_sysfs(device=0):
    """(pp_dpm_sclk path, power path) of the GPU this rank runs on, or None.  The box's sysfs lists
    every GPU of the node, not only the visible one: the card is found by the PCI address of the HIP
    device; without it, all cards are candidates and the one drawing the most power is the loaded one."""
    import glob

    def files(dev_dir):
        sclk = os.path.join(dev_dir, 'pp_dpm_sclk')
        pw = glob.glob(os.path.join(dev_dir, 'hwmon', 'hwmon*', 'power1_average')) + \
            glob.glob(os.path.join(dev_dir, 'hwmon', 'hwmon*', 'power1_input'))
        return (sclk, pw[0]) if os.path.exists(sclk) and pw else None

    try:
        pr = torch.cuda.get_device_properties(device)
        bdf = f'{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0'
        got = files(os.path.join('/sys/bus/pci/devices', bdf))
        if got:
            return [got]
    except Exception:   # noqa: BLE001
        pass
    cands = [files(c) for c in sorted(glob.glob('/sys/class/drm/card[0-9]*/device'))]
    return [c for c in cands if c] or None


def _under_profiler():
    return any(k == 'LD_PRELOAD' or k.startswith(('ROCP_', 'ROCPROFILER_', 'ROCPROF')) for k in os.environ)


def sample_dvfs(step, fence, n_steps=6, device=0):
    """Shader clock and socket power while the step runs (untimed extra steps, after the timed
    region), polled from a thread that never touches the HIP context.  Source: the amdgpu sysfs
    files (pp_dpm_sclk, hwmon power1_average) -- no child process; only when they are unreadable and
    no profiler is preloaded does it fall back to the rocm-smi script (run by this interpreter
    directly, with a clean environment: under rocprofv3 a child inherits the profiler's preload, and
    an `env`-shebang hop after the GPU is initialised is exactly what the GPU pool forbids).
    The MFMA peak in `roofline` is quoted at the 2.4 GHz boost clock; under its 1400 W cap the chip
    sustains less on this workload.  These samples are informational: the sysfs clock is an average over whole steps
    and is not the clock inside the GEMMs (profiles/r5_gemm.md has the in-kernel one)."""
    import re
    import threading
    sysfs = _amdgpu_sysfs(device)
    smi = '/opt/rocm/libexec/rocm_smi/rocm_smi.py'
    use_smi = sysfs is None and not _under_profiler() and os.path.exists(smi)
    if sysfs is None and not use_smi:
        return None
    samples, stop = [], threading.Event()

    def poll():
        clean = {k: v for k, v in os.environ.items()
                 if k != 'LD_PRELOAD' and not k.startswith(('ROCP_', 'ROCPROFILER_', 'ROCPROF'))}
        while not stop.is_set():
            try:
                if sysfs:
                    best = None
                    for sclk_path, pw_path in sysfs:     # several candidates: the loaded card draws the most
                        pw = float(open(pw_path).read()) * 1e-6
                        if best is None or pw > best[1]:
                            best = (sclk_path, pw)
                    cur = [ln for ln in open(best[0]).read().splitlines() if ln.rstrip().endswith('*')]
                    clk = re.search(r'(\d+)\s*Mhz', cur[0], re.I) if cur else None
                    if clk:
                        samples.append((int(clk.group(1)), best[1]))
                    time.sleep(0.05)
                else:
                    out = subprocess.run([sys.executable, smi, '--showclocks', '--showpower'],
                                         capture_output=True, text=True, timeout=20, env=clean).stdout
                    clk = re.search(r'GPU\[0\].*sclk clock level.*\((\d+)Mhz\)', out)
                    pw = re.search(r'GPU\[0\].*Power \(W\): ([\d.]+)', out)
                    if clk and pw:
                        samples.append((int(clk.group(1)), float(pw.group(1))))
            except Exception:   # noqa: BLE001
                return

    th = threading.Thread(target=poll, daemon=True)
    th.start()
    for _ in range(n_steps):
        step()
    fence()
    stop.set()
    th.join(timeout=30)
    busy = [s for s in samples if s[1] > 600.]      # samples taken while the GPU was loaded
    if not busy:
        return None
    sclk = sum(s[0] for s in busy) / len(busy)
    # (informational: the sysfs clock is NOT the clock inside the GEMMs -- profiles/r5_gemm.md has that one, stamped in
    # the kernels of the diagnostic build: 1.74 - 1.92 GHz on random operands, 2.39 on zeros -- and no fraction is built on it)
    return {'sclk_mhz': sclk, 'socket_power_w': sum(s[1] for s in busy) / len(busy),
            'samples': len(busy), 'boost_mhz': 2400, 'source': 'sysfs' if sysfs else 'rocm-smi',
            'in_kernel_clock': 'profiles/r5_gemm.md (s_memtime / s_memrealtime stamps, diagnostic build)'}


def self_launch(a):
    """`python bench.py --gpus N` with no launcher around it: start one rank per GPU through
    torch.distributed.run (the reference's own launch line, scripts/sbatch_run.sh:48-51) as a CHILD
    and exit with its code.  This parent has not touched the GPU (importing torch does not) and
    never re-execs."""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)       # (the ranks themselves decide about HSA_ENABLE_IPC_MODE_LEGACY: dist_env below)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={a.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def dist_diag(rank, local, what):
    """One readable block on stderr when the collective library does not come up: which rank, which device, and the
    environment RCCL / the HSA runtime read."""
    keys = sorted(k for k in os.environ if k.startswith(('HSA_', 'NCCL_', 'RCCL_', 'MASTER_', 'HIP_VISIBLE', 'ROCR_VISIBLE',
                                                         'CUDA_VISIBLE', 'GPU_DEVICE')) or
                  k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'EVENTCLIP_DIST_BACKEND'))
    env = ' '.join(f'{k}={os.environ[k]}' for k in keys)
    sys.stderr.write(f'[bench] rank {rank} on {socket.gethostname()}:cuda{local} ({torch.cuda.device_count()} visible GPU(s)): '
                     f'{what}\n[bench]   env: {env}\n')
    sys.stderr.flush()


def dist_init(a, world, rank, local, backend):
    """init_process_group with a SHORT timeout and, right behind it, one 4-byte all-gather under a watchdog -- before
    any weight packing or data generation, so that a fabric / IPC set-up that does not work costs seconds and leaves a
    readable diagnostic instead of the driver's time limit.  On expiry the watchdog prints and leaves with a fresh
    exit (never a re-exec: the GPU is initialised)."""
    import datetime
    import threading
    limit = float(os.environ.get('EVENTCLIP_DIST_TIMEOUT', '240'))

    def expired():
        dist_diag(rank, local, f'no answer from the {backend} first all-gather within {limit:.0f} s -- giving up '
                               '(P2P / IPC set-up between the ranks? see DESIGN.md 5)')
        os._exit(3)
    dog = threading.Timer(limit, expired)
    dog.daemon = True
    dog.start()
    try:
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local),
                                    timeout=datetime.timedelta(seconds=limit))
        else:
            dist.init_process_group(backend, timeout=datetime.timedelta(seconds=limit))
        mine = torch.full((1,), rank, dtype=torch.int32, device='cuda')
        seen = torch.empty(world, dtype=torch.int32, device='cuda')
        dist.all_gather_into_tensor(seen, mine)
        torch.cuda.synchronize()
        assert seen.tolist() == list(range(world)), f'first all-gather returned {seen.tolist()}'
    except BaseException as e:      # noqa: BLE001 -- whatever the library raises: say where, then fail
        dog.cancel()
        dist_diag(rank, local, f'{backend} did not come up: {type(e).__name__}: {str(e)[:500]}')
        raise SystemExit(3)
    dog.cancel()


def build_workload(config, world, rank, batch=None, arch=None, classes=None, dtype='float16', chunk=2560,
                   unique_samples=None, f16_weights=False, packed_events=False, clip_kw=None, tolerance_mode=False):
    """Model + pipeline + this rank's share of one batch of BASELINE configs[config] as event streams resident in HBM."""
    from eventclip_amd import clip as eclip
    from eventclip_amd.clip_cls import FSCLIPClassifier, ZSCLIPClassifier
    from eventclip_amd.event2img import Event2ImagePipeline
    from eventclip_amd.harness import shard_range
    from eventclip_amd.synthetic import GEOMETRY, make_events
    c = CONFIGS[config]
    batch, arch, classes = batch or c['batch'], arch or c['arch'], classes or c['K']
    geo = GEOMETRY[c['geo']]
    T, N = c['T'], geo['N']
    quantize_args = dict(max_imgs=T, N=N, split_method='event_count',
                         convert_method='event_histogram', grayscale=c['grayscale'],
                         count_non_zero=geo['count_non_zero'],
                         background_mask=geo['background_mask'])

    # ---- model: seeded random CLIP, text features cached once ----
    cfg = eclip.arch_config(arch)
    sd = eclip.random_state_dict(cfg, seed=2)
    if f16_weights:
        cdt = torch.float16 if dtype == 'float16' else torch.bfloat16
        sd = {k: (v.to(cdt).float() if v.dim() >= 2 else v) for k, v in sd.items()}
    clip_kw = dict(clip_kw or {})
    if tolerance_mode:
        clip_kw.update(eclip.tolerance_mode_kwargs(cfg))
    clip_model = eclip.CLIP(cfg, sd, dtype=dtype, chunk=chunk, **clip_kw).cuda().eval()
    tokens = eclip.synthetic_tokens(classes, seed=2)
    clip_dict = dict(clip_model=clip_model, prompt='a point cloud image of a {}',
                     class_names=[f'class {i}' for i in range(classes)], agg_func='mean', class_tokens=tokens)
    if c['adapter'] is None:
        model = ZSCLIPClassifier(clip_dict=clip_dict)
    else:
        torch.manual_seed(2)
        model = FSCLIPClassifier(adapter_dict=dict(adapter_type='text-trans', in_dim=cfg['embed_dim'], d_model=256,
                                                   num_heads=4, ffn_dim=1024, norm_first=True, num_layers=2,
                                                   residual=c['adapter']),
                                 clip_dict=clip_dict, loss_dict=dict(use_logits_loss=True, use_probs_loss=False))
    model = model.cuda().eval()
    model.get_text_feats()

    # ---- data: this rank's share of the batch as event streams resident in HBM ----
    if c['scaling'] == 'strong':       # a GLOBAL batch, contiguous shards (harness.shard_range)
        shard_sizes = [shard_range(batch, r, world)[1] - shard_range(batch, r, world)[0] for r in range(world)]
        local_batch, global_batch = shard_sizes[rank], batch
    else:                              # the batch is per GPU
        shard_sizes = [batch] * world
        local_batch, global_batch = batch, batch * world
    assert local_batch > 0, f'rank {rank} has no samples: batch {batch} over {world} ranks'
    # config 1: every sample of the batch is its own seeded stream (no tiling: the events kernel's HBM number is
    # then not flattered by a reuse pattern); the big configs tile a few distinct streams ON THE DEVICE
    uniq_n = min(local_batch, unique_samples or (local_batch if config == 1 else 16))
    # (generated on a few threads -- numpy releases the GIL in the generator and the sort: 256 streams of 200 000
    # events are ~8 s of single-threaded host work per rank otherwise, and the ranks of a node do this at once)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 8) // max(1, world)))) as ex:
        evs = list(ex.map(lambda i: make_events(c['n_ev'], geo['resolution'], seed=2 * 100003 + rank * 1000 + i),
                          range(uniq_n)))
    if uniq_n == local_batch:
        events = torch.from_numpy(np.concatenate(evs)).cuda()
    else:
        u = torch.from_numpy(np.stack(evs)).cuda()                                  # [uniq, n_ev, 4]
        events = u[torch.arange(local_batch, device='cuda') % uniq_n].reshape(-1, 4).contiguous()
        del u
    n_events = [c['n_ev']] * local_batch
    if packed_events:
        from eventclip_amd.vis import pack_events_device
        events = pack_events_device(events)
    pipe = Event2ImagePipeline(geo['resolution'], c['max_n'] or geo['max_n'], quantize_args,
                               n_px=cfg['image_size'], patch=cfg['patch'], kpad=clip_model.kpad,
                               dtype=clip_model.compute_dtype)
    pipe.strict = False   # no host sync inside the step (bounds are checked by the tests; ms_per_step_strict prices it)
    views = T if c['n_ev'] >= N else 1          # frames per sample (vis.py:55-72: fewer than N events = one chunk)
    return dict(c=c, geo=geo, cfg=cfg, sd=sd, T=T, N=N, clip_model=clip_model, model=model, tokens=tokens, clip_dict=clip_dict,
                quantize_args=quantize_args, evs=evs, events=events, n_events=n_events, pipe=pipe, uniq_n=uniq_n,
                shard_sizes=shard_sizes, local_batch=local_batch, global_batch=global_batch, views=views,
                frames_per_step=local_batch * views, batch=batch, arch=arch, classes=classes)


def dominant_kernel(prof, steps):
    """(roofline dict of the kernel class with the largest summed duration, its record) from ec_profile records."""
    dom = max(prof, key=lambda e: e['total_ms'])
    avg_ms = dom['total_ms'] / dom['launches']
    if dom['name'].startswith(MFMA_KERNELS):
        achieved = dom['flops'] / dom['launches'] / (avg_ms * 1e-3) / 1e12
        roof = {'bound': 'mfma', 'achieved': achieved, 'peak': PEAK_MFMA_TFLOPS,
                'unit': 'TFLOP/s', 'frac': achieved / PEAK_MFMA_TFLOPS}
    else:
        achieved = dom['bytes'] / dom['launches'] / (avg_ms * 1e-3) / 1e9
        roof = {'bound': 'hbm', 'achieved': achieved, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s',
                'frac': achieved / PEAK_HBM_GBS}
    roof.update(kernel=dom['name'], launches_per_step=dom['launches'] / steps, avg_launch_ms=avg_ms, traffic=None)
    return roof, dom


# per-GPU shard of BASELINE's batch on an 8-GPU node for the configs the default line does not time
OTHER_CONFIG_BATCH = {2: 512, 3: 2048 // 8, 4: 4096 // 8}


def other_configs(a, fence, cpu=True):
    """BASELINE configs[2..4] on this one GPU, AFTER the timed region of the headline (never part of `value`): each at
    the per-GPU shard of its BASELINE batch (configs[2]: 512 samples per GPU; configs[3] / [4]: their global batch over 8
    GPUs = 256 x 2 / 512 x 5 views), one warm-up and two timed steps of the same step function (events resident in HBM
    -> logits), with the dominant kernel class and its roofline fraction from the library's HIP-event records, and a
    small CPU baseline on the config's own sensor shape (reference test.py:59-61 runs every config through the same
    loop).  The builder-run full-size lines are profiles/r6_configs_bench.jsonl."""
    from eventclip_amd import _lib
    res = {}

    def one(cid, batch):
        t_all = time.perf_counter()
        batch = a.other_configs_batch or batch
        w = build_workload(cid, 1, 0, batch=batch, arch=a.arch_given, classes=a.classes_given, dtype=a.dtype, chunk=a.chunk)

        t_setup = time.perf_counter() - t_all

        def step():
            return w['model'](w['pipe'](w['events'], w['n_events']))
        step()
        fence()
        steps = 2
        _lib.profile_begin()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        fence()
        dt = (time.perf_counter() - t0) / steps
        prof = _lib.profile_end()
        assert int(out['valid_masks'].sum()) == w['frames_per_step']
        roof, dom = dominant_kernel(prof, steps)
        line = {'workload': f'{w["c"]["name"].format(arch=w["arch"])}, {batch} samples x {w["views"]} view(s) = the per-GPU '
                            f'shard of BASELINE configs[{cid}] on 8 GPUs',
                'value': w['frames_per_step'] / dt, 'unit': 'frames/s', 'ms_per_step': dt * 1e3, 'steps': steps,
                'frames_per_step': w['frames_per_step'], 'dominant_kernel': roof['kernel'], 'bound': roof['bound'],
                'frac': roof['frac'], 'dominant_ms_per_step': dom['total_ms'] / steps,
                'kernel_ms_per_step': {e['name']: round(e['total_ms'] / steps, 3) for e in prof}}
        if cpu:
            try:
                cb = cpu_baseline(w['cfg'], w['sd'], w['tokens'], w['evs'], w['quantize_args'], 1,
                                  min(w['T'], 4 if cid != 3 else 2), shape=w['geo']['resolution'], pool=False, max_classes=16)
                line['cpu_baseline'] = {k: cb[k] for k in ('value', 'unit', 'cores', 'kind', 'sample', 'event2img_frames_per_s_1proc')}
            except Exception as e:   # noqa: BLE001 -- a baseline must never take the bench line down
                line['cpu_baseline_error'] = repr(e)
        line['wall_s'] = time.perf_counter() - t_all
        line['setup_s'] = t_setup
        return line

    for cid, batch in OTHER_CONFIG_BATCH.items():
        try:
            res[str(cid)] = one(cid, batch)
        except Exception as e:   # noqa: BLE001 -- one config's failure costs that config's entry only
            res[str(cid)] = {'error': repr(e)}
        torch.cuda.empty_cache()
    return res


def main():
    a = parse()
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(a))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    # one process per GPU over RCCL; EVENTCLIP_DIST_BACKEND=gloo lets two ranks share one GPU so the
    # N > 1 code path can be exercised on a single-GPU box (a functional check, not a measurement)
    backend = os.environ.get('EVENTCLIP_DIST_BACKEND', 'nccl')
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        # HSA_ENABLE_IPC_MODE_LEGACY: this pool's host driver supports dmabuf IPC only (the platform note of this build:
        # without the variable at 0, RCCL's P2P set-up fails in hipIpcGetMemHandle).  The launch environment's value is
        # never overridden; when there is none, 0 is set and said so.
        if 'HSA_ENABLE_IPC_MODE_LEGACY' not in os.environ:
            os.environ['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
            if rank == 0:
                sys.stderr.write('[bench] HSA_ENABLE_IPC_MODE_LEGACY was unset: using 0 (dmabuf IPC)\n')
    n_dev = torch.cuda.device_count()
    # EVENTCLIP_DIST_SHARE_DEVICE=1 (tests): ranks wrap around the devices that exist even under nccl
    share = backend != 'nccl' or os.environ.get('EVENTCLIP_DIST_SHARE_DEVICE', '0') not in ('', '0')
    if world > 1 and not share and local >= n_dev:
        dist_diag(rank, local, f'LOCAL_RANK {local} has no GPU of its own ({n_dev} visible): RCCL needs one device per rank')
        sys.exit(3)
    local = local % max(n_dev, 1) if share else local
    torch.cuda.set_device(local)
    if world > 1:
        dist_init(a, world, rank, local, backend)
    assert world == a.gpus, f'--gpus {a.gpus} but WORLD_SIZE={world}'
    # proof that the collective library saw every rank: world size after init and each rank's device
    ranks_seen, devices = 1, [local]
    if world > 1:
        ranks_seen = dist.get_world_size()
        devs = [None] * world
        dist.all_gather_object(devs, f'{socket.gethostname()}:cuda{local}')
        devices = devs

    from eventclip_amd import _lib
    from eventclip_amd.harness import all_gather_rows

    w = build_workload(a.config, world, rank, batch=a.batch, arch=a.arch, classes=a.classes, dtype=a.dtype, chunk=a.chunk,
                       unique_samples=a.unique_samples, f16_weights=a.f16_weights, packed_events=a.packed_events,
                       clip_kw=dict(image_precise=a.precise, image_precise_blocks=0 if a.precise else a.precise_blocks),
                       tolerance_mode=a.tolerance_mode)
    c, geo, cfg, sd, T, N = w['c'], w['geo'], w['cfg'], w['sd'], w['T'], w['N']
    clip_model, model, tokens, clip_dict, quantize_args = w['clip_model'], w['model'], w['tokens'], w['clip_dict'], w['quantize_args']
    evs, events, n_events, pipe, uniq_n = w['evs'], w['events'], w['n_events'], w['pipe'], w['uniq_n']
    shard_sizes, local_batch, global_batch = w['shard_sizes'], w['local_batch'], w['global_batch']
    views, frames_per_step = w['views'], w['frames_per_step']
    gather_events = []                          # HIP event pairs around the all-gather (rank-local stream)

    def step():
        batch = pipe(events, n_events)
        out = model(batch)
        if world > 1:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out['logits'] = all_gather_rows(out['logits'], shard_sizes)
            e1.record()
            gather_events.append((e0, e1))
        return out

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(a.warmup):
        step()
    fence()
    gather_events.clear()
    _lib.profile_begin()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0           # this rank's own time, before it waits for the others
    fence()
    dt = time.perf_counter() - t0
    prof = _lib.profile_end()
    assert int(out['valid_masks'].sum()) == frames_per_step
    assert out['logits'].shape[0] == global_batch
    rank_ms = [dt_own / a.steps * 1e3]
    gather_ms = None
    if world > 1:
        t = torch.tensor([dt], device='cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        rank_ms = [None] * world
        dist.all_gather_object(rank_ms, dt_own / a.steps * 1e3)
        gather_ms = sum(e0.elapsed_time(e1) for e0, e1 in gather_events) / a.steps
    total_frames = sum(shard_sizes) * views     # all ranks, one step
    if a.dump_outputs and rank == 0:
        # what the last timed step returned (the logits all-gathered over the ranks; the rest is rank 0's shard)
        for name, (shape, rows) in dump_outputs(out, a.dump_outputs).items():
            sys.stderr.write(f'[bench] --dump-outputs: {name} {shape}, {rows} rows written\n')

    # ---- the same steps with every batch starting in host memory (never part of `value`) ----
    host_line = None
    run = extras(a, world)
    # (in every --full line of the headline on one GPU -- VERDICT r5 item 3: the host-fed number in the driver's record)
    if 'value_from_host' in run:
        # (measured after the timed region: a failure here must not cost the line its `value`; an explicit --from-host run raises)
        try:
            host_samples = [evs[i % uniq_n] for i in range(local_batch)]      # numpy float32 [n_ev, 4] each
            if a.packed_events:
                from eventclip_amd.vis import pack_events
                packed = [pack_events(e) for e in evs]
                host_samples = [packed[i % uniq_n] for i in range(local_batch)]

            t0h = None
            host_warm = min(a.warmup, 1) if not a.from_host else a.warmup
            host_steps = min(a.steps, 5) if not a.from_host else a.steps

            def host_batches():
                for _ in range(host_warm + host_steps):
                    yield host_samples
            for i, batch in enumerate(pipe.stream(host_batches(), depth=2)):
                if i == host_warm:
                    fence()
                    t0h = time.perf_counter()
                out_h = model(batch)
                if world > 1:
                    out_h['logits'] = all_gather_rows(out_h['logits'], shard_sizes)
            fence()
            dth = time.perf_counter() - t0h
            if world > 1:
                t = torch.tensor([dth], device='cuda')
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dth = float(t.item())
            assert torch.equal(out_h['logits'], out['logits'])                 # same batch, same bits
            host_bytes = sum(e.nbytes for e in host_samples)
            host_line = {'value_from_host': total_frames * host_steps / dth, 'ms_per_step_from_host': dth / host_steps * 1e3,
                         'from_host': {'bytes_per_step_per_gpu': host_bytes, 'steps': host_steps, 'warmup': host_warm,
                                       'path': 'per-sample copies into a pinned staging ring (8 threads), one async H2D '
                                               'copy per batch on a copy stream, batch i + 1 uploaded under the GPU work of '
                                               'batch i (eventclip_amd.event2img.HostFeeder)'}}
        except Exception as e:   # noqa: BLE001
            if a.from_host or world > 1:
                raise
            host_line = {'from_host_error': repr(e)}

    if rank == 0:
        value = total_frames * a.steps / dt
        # ---- roofline of the dominant kernel, from the live HIP-event records ----
        roof, dom = dominant_kernel(prof, a.steps)
        # HBM-side bytes per launch come from the committed PMC passes (separate rocprofv3 --pmc runs
        # of this command, tools/profile_round.sh), not from this run: say which file and which commit
        traffic_file = os.path.join(ROOT, 'profiles', 'traffic.json')
        tr = json.load(open(traffic_file)) if os.path.exists(traffic_file) else {}
        per_kernel = tr.get('all_kernels', {})
        if dom['name'] in per_kernel:
            roof['traffic'] = per_kernel[dom['name']].get('hbm_bytes_per_launch')
            roof['traffic_source'] = f"profiles/traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes at commit " \
                                     f"{tr.get('commit', 'unrecorded')})"
        # north_star asks for the achieved HBM rate of event2img next to the MFMA number
        ev_rec = next((e for e in prof if e['name'] == 'events_to_frames_kernel'), None)
        roof_events = None
        if ev_rec:
            ev_ms = ev_rec['total_ms'] / ev_rec['launches']
            ev_bytes = ev_rec['bytes'] / ev_rec['launches']
            roof_events = {'bound': 'hbm', 'kernel': 'events_to_frames_kernel',
                           'algorithmic_bytes_per_launch': ev_bytes, 'avg_launch_ms': ev_ms,
                           'achieved_GBps': ev_bytes / (ev_ms * 1e-3) / 1e9, 'peak_GBps': PEAK_HBM_GBS,
                           'frac': ev_bytes / (ev_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                           'traffic': per_kernel.get('events_to_frames_kernel', {}).get('hbm_bytes_per_launch')}
        gpu_ms = sum(e['total_ms'] for e in prof) / a.steps
        breakdown = {e['name']: round(e['total_ms'] / a.steps, 3) for e in prof}
        metric = 'event-frames/sec (whole node) ViT-L/14 zero-shot @224' if a.config == 1 else \
            f'event-frames/sec (whole node), BASELINE configs[{a.config}]'
        if a.precise:
            metric += ' -- split-precision image tower (validation mode, not the headline)'
        elif a.tolerance_mode:
            metric += f' -- tolerance mode: first {clip_model.image_precise_blocks} blocks of the image tower as split-operand blocks (not the headline)'
        elif a.precise_blocks:
            metric += f' -- first {a.precise_blocks} blocks of the image tower as split-operand blocks (not the headline)'
        if c['scaling'] == 'weak':
            batch_txt = f'batch={a.batch} samples x {views} view{"s" if views > 1 else ""} per GPU'
        else:
            batch_txt = f'global batch={a.batch} samples x {views} views, sharded over the GPUs'
        res = {
            'metric': metric,
            'value': value, 'unit': 'frames/s', 'n_gpus': world, 'steps': a.steps,
            'warmup': a.warmup, 'ms_per_step': dt / a.steps * 1e3, 'higher_is_better': True,
            'scaling': c['scaling'], 'vs_baseline': None, 'dtype': 'f16' if a.dtype == 'float16' else 'bf16',
            'data': 'synthetic',
            'config': {'workload': f'{c["name"].format(arch=a.arch)}, {batch_txt} (configs[{a.config}])',
                       'frames_per_step_per_gpu': frames_per_step, 'classes': a.classes,
                       'events_per_frame': min(N, c['n_ev']), 'resolution': list(geo['resolution']),
                       'event_format': 'packed 8 B' if a.packed_events else 'float32 [n, 4]',
                       'unique_samples': uniq_n,
                       'tower_chunk_frames': a.chunk,
                       'weights': 'seeded random' + (', rounded to 16 bit first (a checkpoint stored in 16 bit)' if a.f16_weights else ''),
                       'precision': (('split precision: hi + lo 16-bit operands in every GEMM of the image tower '
                                      '(ec_vit_weights.precise, 3 x the MFMA work), fp32 residual stream and LayerNorm'
                                      if a.precise else
                                      '16-bit MFMA operands, fp32 accumulate / softmax; residual stream as hi + lo '
                                      '16-bit planes (~2^-22), LayerNorm folded into the QKV / c_fc GEMMs (statistics '
                                      'of the 16-bit hi plane); patch embedding and ln_post @ proj with hi + lo operands')
                                     + (f'; the first {clip_model.image_precise_blocks} blocks as split-operand blocks (LayerNorm of both planes '
                                        'into hi + lo parts, QKV / c_fc multiply both, every GEMM adds its weight\'s lo product '
                                        f'in the same launch; fp32 attention on hi + lo q, k, v in the first '
                                        f'{clip_model.image_precise_attn_blocks}: ec_vit_weights.precise_blocks / precise_attn_blocks)'
                                        + (', their lo products as e4m3 operands on the FP8 matrix path (ec_vit_weights.lo_fp8)' if clip_model.image_lo_fp8 else '')
                                        if clip_model.image_precise_blocks and not a.precise else '')
                                     + '; text tower split-precision (cached)'),
                       # the EFFECTIVE tolerance-mode setting of the timed model (0 = the headline's 16-bit path; EVENTCLIP_PRECISE_BLOCKS
                       # in the environment would change it without a flag on the command line)
                       'precise_blocks_effective': [clip_model.image_precise_blocks, clip_model.image_precise_attn_blocks],
                       'last_block': ('every token' if clip_model.full_last_block else
                                      'keys/values for every token; query projection, attention, out_proj, '
                                      'MLP for the class token only (bit-identical encode_image output)'),
                       'parallelism': f'dp{world}, all-gather of logits' if world > 1 else 'single GPU',
                       'collective_backend': (backend if world > 1 else None),
                       'collective_ranks': ranks_seen, 'rank_devices': devices},
            'roofline': roof, 'roofline_events': roof_events,
            'kernel_ms_per_step': breakdown, 'kernel_ms_per_step_total': gpu_ms,
            'kernel_launches_per_step': {e['name']: e['launches'] / a.steps for e in prof},
            'kernel_algorithmic_bytes_per_launch': {e['name']: e['bytes'] / e['launches'] for e in prof},
        }
        if a.config != 1 or world > 1:
            res['config'].update(adapter=(None if c['adapter'] is None else f'text-trans, residual {c["adapter"]}'),
                                 samples_per_rank=shard_sizes, frames_per_step_total=total_frames)
            # each rank's own time per step (before it waits for the slowest) and what the all-gather of the
            # logits cost on rank 0's stream: what a scaling run needs to attribute its loss
            res['ms_per_step_per_rank'] = rank_ms
            res['all_gather_ms_per_step'] = gather_ms
        if host_line is not None:
            res.update(host_line)
        if 'dvfs' in run:
            dv = sample_dvfs(step, fence, device=local)
            if dv:
                res['dvfs'] = dv
        def extra(key, fn):
            """the measurements behind the timed region never take the line down: a failure is recorded under key_error"""
            try:
                res[key] = fn()
            except Exception as e:   # noqa: BLE001
                res[key + '_error'] = repr(e)
                sys.stderr.write(f'[bench] {key} failed: {e!r}\n')
        if 'tolerance_mode' in run:
            extra('tolerance_mode', lambda: tolerance_mode(a, cfg, sd, clip_dict, step, fence, pipe, events, n_events,
                                                           frames_per_step, res['ms_per_step']))
        if 'ms_per_step_strict' in run:
            # Event2ImagePipeline's DEFAULT (strict = True) reads the events kernel's out-of-sensor count back to the
            # host every batch (event2img.py:106-110; the reference syncs per batch too, test.py:66); the timed region
            # runs strict = False: this is what the default costs on the same batch
            def strict_ms():
                pipe.strict = True
                try:
                    step()
                    fence()
                    t0s = time.perf_counter()
                    for _ in range(3):
                        step()
                    fence()
                    return (time.perf_counter() - t0s) / 3 * 1e3
                finally:
                    pipe.strict = False
            extra('ms_per_step_strict', strict_ms)
            res['strict_note'] = ('pipe.strict = True (the pipeline default: one 4-byte read-back of the dropped-event count per '
                                  'batch), 3 steps after the timed region; `value` is timed with strict = False')
        if 'cpu_baseline' in run:
            extra('cpu_baseline', lambda: cpu_baseline(cfg, sd, tokens, evs, quantize_args,
                                                       a.cpu_baseline_samples if a.config == 1 else 1,
                                                       min(a.cpu_baseline_frames, T) if a.config != 3 else 2,
                                                       shape=geo['resolution'], pool=(a.config == 1)))
        if 'other_configs' in run:
            # release the headline's model / workspace / events first: the other configs build their own
            del w, model, clip_model, clip_dict, pipe, events, out, step
            torch.cuda.empty_cache()
            extra('other_configs', lambda: other_configs(a, fence, cpu=not a.no_cpu_baseline))
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
