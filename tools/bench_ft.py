"""Time one fine-tuning step of the vision tower on the MI355X (the reference's FTCLIP configs:
configs/ftclip/ft_text_fsclip_nin_params*.py -- ViT-L/14, N-ImageNet geometry, 128 // 4 gpus = 32 samples x
2 views per GPU, K = 1000, Adam, `lora='qkvo-16'` or every visual parameter).

    python tools/bench_ft.py [--arch ViT-L/14] [--samples 32] [--views 2] [--classes 1000] [--steps 5]
                             [--modes lora,full,bias] [--dtype float16] [--graph | --autograd | --input-grad]

Prints one JSON line per mode: ms per step, frames/s, the split forward / loss / backward / update, the
algorithmic flops (3 x the forward's 2 M N K for a full step; LoRA skips the MLP's weight gradients) and the
rate they amount to, and `cpu_baseline`: forward + backward of the oracle's tower (torch CPU fp32 autograd over
oracle/clip_ref.py, every visual gradient, no optimiser) on a few frames with the box's host cores.  Synthetic
frames, seeded random weights (no datasets / checkpoints on the box).  The CPU leg is the only place the oracle is
touched.

`--autograd` prints one line per mode with the same step three ways, interleaved in one process: `FTTrainer` with eager
launches, `FTTrainer(graph=True)`, and the reference's loop on `FTCLIPClassifier(clip_dict=dict(..., autograd=True))`
(`clf(data)`, `calc_train_loss`, `torch.amp.GradScaler`, `loss.backward()`, `torch.optim.Adam` over the two parameter
groups of method.py:165-180): ms per step (the median of `--rounds` rounds of `--steps` steps) and the host's share of
it (until the last step is queued).

`--input-grad` prints one line: a FROZEN tower differentiated with respect to its input image (`CLIP.encode_image(image,
differentiable=True)`, `eventclip_hip::vit_image_fwd` / `vit_image_bwd`: forward + backward to `image.grad`) beside the
`--autograd` full step (every visual parameter trainable), interleaved round by round in one process on the same number
of frames (`--samples` x `--views`, default 64): ms of forward + backward and of the backward alone for both (device
time between events, medians over the rounds), and the kernels the frozen backward launched -- which must hold no
weight-gradient, bias-gradient or LoRA launch (checked: the tool fails otherwise)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def cpu_baseline(arch, frames=4, repeat=2):
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    cfg = eclip.arch_config(arch)
    sd = eclip.random_state_dict(cfg, 0)
    leaves = {k: v.float().clone().requires_grad_(True) for k, v in sd.items() if k.startswith('visual.')}
    threads = min(64, os.cpu_count() or 8)
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    imgs = torch.randn(frames, 3, cfg['image_size'], cfg['image_size'])
    best = float('inf')
    for _ in range(repeat):
        for v in leaves.values():
            v.grad = None
        t0 = time.perf_counter()
        feats = clip_ref.encode_image_autograd(leaves, cfg, imgs)
        feats.backward(torch.ones_like(feats))
        best = min(best, time.perf_counter() - t0)
    return dict(frames_per_s=round(frames / best, 2), kind='port', dtype='float32', cores=threads,
                sample='%d frames, forward + backward of every visual parameter, best of %d (%.1f s)' % (frames, repeat, best))


def _batch(t, B, T, K, dev):
    torch.manual_seed(0)
    n = B * T
    patches = (torch.randn(n, t.G, t.kpad, device=dev) * 0.5).to(t.cd)
    patches[:, :, 2 * t.k:] = 0
    return {'patches': patches, 'row_idx': torch.arange(n, device=dev, dtype=torch.int32).view(B, T),
            'valid_mask': torch.ones(B, T, dtype=torch.bool, device=dev), 'label': torch.randint(0, K, (B,), device=dev)}


def autograd_rows(a):
    """FTTrainer eager / hipGraph and the autograd loop on the same batch, interleaved round by round."""
    import statistics
    from eventclip_amd import _lib, clip as eclip, ft
    from eventclip_amd.clip_cls_ft import FTCLIPClassifier
    dev = _lib.require_gpu()
    B, T, K = a.samples, a.views, a.classes
    for mode in a.modes.split(','):
        extra = dict(lora='qkvo-16') if mode == 'lora' else (dict(lora=-1, only_bias=True) if mode == 'bias' else dict(lora=-1))

        def classifier(**more):
            model = eclip.build_random(a.arch, seed=0, dtype=a.dtype)
            cd = dict(clip_model=model, prompt='a point cloud image of a {}', class_names=[f'c{i}' for i in range(K)],
                      agg_func='mean', class_tokens=eclip.synthetic_tokens(K), only_conv1=False, only_bias=False,
                      only_ln=False, **extra, **more)
            return FTCLIPClassifier(adapter_dict=dict(adapter_type='text-identity', residual=0.95), clip_dict=cd,
                                    loss_dict=dict(use_logits_loss=True, use_probs_loss=False)).cuda().train()
        kw = dict(lr=2e-5, clip_lr=2e-5, total_steps=1000, init_scale=4096.0)
        trainers = {'trainer_eager': ft.FTTrainer(classifier(), **kw), 'trainer_graph': ft.FTTrainer(classifier(), graph=True, **kw)}
        clf = classifier(autograd=True)
        named = [(n, p) for n, p in clf.named_parameters() if p.requires_grad]
        opt = torch.optim.Adam([{'params': [p for n, p in named if 'model.visual' not in n], 'lr': 2e-5},
                                {'params': [p for n, p in named if 'model.visual' in n], 'lr': 2e-5}])
        scaler = torch.amp.GradScaler('cuda', init_scale=4096.0)
        data = _batch(trainers['trainer_eager'].tower, B, T, K, dev)

        def autograd_step():
            opt.zero_grad(set_to_none=True)
            loss = clf.calc_train_loss(data, clf(data))['ce_loss']
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            return loss.detach()
        steps = {k: (lambda tr=tr: tr.step(data)) for k, tr in trainers.items()}
        steps['autograd'] = autograd_step
        for fn in steps.values():
            for _ in range(max(a.warmup, 4)):
                fn()
        torch.cuda.synchronize()
        total, host, loss = {k: [] for k in steps}, {k: [] for k in steps}, {}
        for _ in range(a.rounds):
            for k, fn in steps.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss[k] = fn()
                t1 = time.perf_counter()
                if k in trainers:
                    trainers[k].resolve()
                torch.cuda.synchronize()
                host[k].append((t1 - t0) / a.steps * 1e3)
                total[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        print(json.dumps(dict(mode=mode, arch=a.arch, frames_per_step=B * T, classes=K, dtype=a.dtype, steps=a.steps,
                              rounds=a.rounds, trainable_tensors=len(named),
                              ms_per_step={k: round(statistics.median(v), 2) for k, v in total.items()},
                              ms_per_step_rounds={k: [round(x, 2) for x in v] for k, v in total.items()},
                              host_ms_per_step={k: round(statistics.median(v), 2) for k, v in host.items()},
                              loss={k: round(float(v), 4) for k, v in loss.items()},
                              loss_scale=dict(trainer_eager=trainers['trainer_eager'].scaler.scale,
                                              autograd=scaler.get_scale()))), flush=True)
        del trainers, clf, opt, steps
        torch.cuda.empty_cache()


# every weight-, bias- and LayerNorm-gradient ends in a partial-sum reduction, conv1's starts with transposed copies
# (K-batched GEMMs are no sign of one: the dX products' last row tiles run in K-batches too, gemm_rows32)
WEIGHT_GRAD_KERNELS = ('transpose_kernel', 'colsum_kernel + reduce_kernel')


def input_grad_row(a):
    """A frozen tower's forward + backward to the image beside the full autograd step, interleaved."""
    import statistics
    from eventclip_amd import _lib, clip as eclip
    from eventclip_amd.clip_cls_ft import FTCLIPClassifier
    dev = _lib.require_gpu()
    B, T, K = a.samples, a.views, a.classes
    n = B * T
    frozen = eclip.build_random(a.arch, seed=0, dtype=a.dtype)
    R = frozen.cfg['image_size']
    torch.manual_seed(0)
    image = (torch.randn(n, 3, R, R, device=dev) * 0.5).requires_grad_(True)
    d_feats = torch.randn(n, frozen.cfg['embed_dim'], device=dev)
    model = eclip.build_random(a.arch, seed=0, dtype=a.dtype)
    cd = dict(clip_model=model, prompt='a point cloud image of a {}', class_names=[f'c{i}' for i in range(K)],
              agg_func='mean', class_tokens=eclip.synthetic_tokens(K), only_conv1=False, only_bias=False, only_ln=False,
              lora=-1, autograd=True)
    clf = FTCLIPClassifier(adapter_dict=dict(adapter_type='text-identity', residual=0.95), clip_dict=cd,
                           loss_dict=dict(use_logits_loss=True, use_probs_loss=False)).cuda().train()
    named = [(k, p) for k, p in clf.named_parameters() if p.requires_grad]
    opt = torch.optim.Adam([{'params': [p for k, p in named if 'model.visual' not in k], 'lr': 2e-5},
                            {'params': [p for k, p in named if 'model.visual' in k], 'lr': 2e-5}])
    scaler = torch.amp.GradScaler('cuda', init_scale=4096.0)
    data = _batch(clf._operand_tower(), B, T, K, dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731

    def frozen_pass():
        image.grad = None
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        feats = frozen.encode_image(image, differentiable=True)
        e1.record()
        feats.backward(d_feats)
        e2.record()
        return e0, e1, e2

    def full_step():
        opt.zero_grad(set_to_none=True)
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        loss = clf.calc_train_loss(data, clf(data))['ce_loss']
        e1.record()
        scaler.scale(loss).backward()
        e2.record()
        scaler.step(opt)
        scaler.update()
        return e0, e1, e2
    passes = {'frozen_image': frozen_pass, 'full_step': full_step}
    for fn in passes.values():
        for _ in range(max(a.warmup, 3)):
            fn()
    torch.cuda.synchronize()
    both, bwd = {k: [] for k in passes}, {k: [] for k in passes}
    for _ in range(a.rounds):
        for k, fn in passes.items():
            marks = [fn() for _ in range(a.steps)]
            torch.cuda.synchronize()
            both[k].append(statistics.median(e0.elapsed_time(e2) for e0, _, e2 in marks))
            bwd[k].append(statistics.median(e1.elapsed_time(e2) for _, e1, e2 in marks))
    # the structural condition: what the frozen backward launches
    image.grad = None
    feats = frozen.encode_image(image, differentiable=True)
    torch.cuda.synchronize()
    _lib.profile_begin()
    feats.backward(d_feats)
    torch.cuda.synchronize()
    entries = [p for p in _lib.profile_end() if p['launches']]
    prof = {p['name']: p['launches'] for p in entries}
    # counted: the launches of the weight-gradient classes, and ec_sgemm's beyond the head's one (the LoRA products)
    weight_grad = sum(prof.get(k, 0) for k in WEIGHT_GRAD_KERNELS) + max(prof.get('sgemm_kernel', 0) - 1, 0)
    un = [p for p in entries if p['name'] == 'unpatchify_kernel']
    print(json.dumps(dict(mode='input_grad', arch=a.arch, frames=n, dtype=a.dtype, steps=a.steps, rounds=a.rounds,
                          fwd_bwd_ms={k: round(statistics.median(v), 2) for k, v in both.items()},
                          bwd_ms={k: round(statistics.median(v), 2) for k, v in bwd.items()},
                          bwd_ms_rounds={k: [round(x, 2) for x in v] for k, v in bwd.items()},
                          full_step_trainable_tensors=len(named), frozen_backward_launches=prof,
                          frozen_backward_kernel_ms={p['name']: round(p['total_ms'], 3) for p in entries},
                          unpatchify_gb_per_s=round(un[0]['bytes'] / un[0]['total_ms'] / 1e6, 1) if un else None,
                          frozen_weight_grad_launches=weight_grad)), flush=True)
    assert weight_grad == 0, f'the frozen backward launched weight-gradient kernels: {prof}'
    assert image.grad is not None and bool(torch.isfinite(image.grad).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='ViT-L/14')
    ap.add_argument('--samples', type=int, default=32)
    ap.add_argument('--views', type=int, default=2)
    ap.add_argument('--classes', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--modes', default='lora,full,bias')
    ap.add_argument('--dtype', default='float16')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--graph', action='store_true', help='replay the step from a hipGraph (recorded after 2 eager steps)')
    ap.add_argument('--autograd', action='store_true',
                    help='the step through torch autograd beside FTTrainer eager and graph=True, interleaved')
    ap.add_argument('--input-grad', action='store_true',
                    help='a frozen tower forward + backward to the image beside the --autograd full step, interleaved')
    ap.add_argument('--rounds', type=int, default=3, help='--autograd / --input-grad: rounds of --steps steps per path')
    a = ap.parse_args()
    if a.input_grad:
        return input_grad_row(a)
    if a.autograd:
        return autograd_rows(a)
    from eventclip_amd import _lib, clip as eclip, ft
    from eventclip_amd.clip_cls_ft import FTCLIPClassifier
    dev = _lib.require_gpu()
    B, T, K = a.samples, a.views, a.classes
    cb = None if a.no_cpu_baseline else cpu_baseline(a.arch)
    for mode in a.modes.split(','):
        model = eclip.build_random(a.arch, seed=0, dtype=a.dtype)
        extra = dict(lora='qkvo-16') if mode == 'lora' else (dict(lora=-1, only_bias=True) if mode == 'bias' else dict(lora=-1))
        cd = dict(clip_model=model, prompt='a point cloud image of a {}', class_names=[f'c{i}' for i in range(K)],
                  agg_func='mean', class_tokens=eclip.synthetic_tokens(K), only_conv1=False, only_bias=False,
                  only_ln=False)
        cd.update(extra)
        clf = FTCLIPClassifier(adapter_dict=dict(adapter_type='text-identity', residual=0.95), clip_dict=cd,
                               loss_dict=dict(use_logits_loss=True, use_probs_loss=False)).cuda().train()
        tr = ft.FTTrainer(clf, lr=2e-5, clip_lr=2e-5, total_steps=1000, init_scale=4096.0, graph=a.graph)
        t = tr.tower
        torch.manual_seed(0)
        n = B * T
        patches = (torch.randn(n, t.G, t.kpad, device=dev) * 0.5).to(t.cd)
        patches[:, :, 2 * t.k:] = 0
        valid = torch.ones(B, T, dtype=torch.bool, device=dev)
        labels = torch.randint(0, K, (B,), device=dev)
        row_idx = torch.arange(n, device=dev, dtype=torch.int32).view(B, T)
        data = {'patches': patches, 'row_idx': row_idx, 'valid_mask': valid, 'label': labels}
        for _ in range(max(a.warmup, 4) if a.graph else a.warmup):
            tr.step(data)
        torch.cuda.synchronize()
        _lib.profile_begin()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = tr.step(data)
        tr.resolve()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        prof = _lib.profile_end()
        c = model.cfg
        W, L, S = c['width'], c['layers'], t.S
        M = n * S
        lin = 2.0 * M * 12 * W * W * L                       # the four nn.Linear of every block, forward
        att = 4.0 * S * S * 64 * (W // 64) * n * L
        if mode == 'full':
            flops = 3 * lin + 3.5 * att
        elif mode == 'lora':
            flops = 2 * lin + 2.0 * M * 4 * W * W * L + 3.5 * att      # dX everywhere, dW for q k v o only
        else:
            flops = 2 * lin + 3.5 * att
        ws_gb = t._ws.buf.numel() / 2 ** 30
        print(json.dumps(dict(mode=mode, arch=a.arch, frames_per_step=n, classes=K, dtype=a.dtype,
                              graph=bool(a.graph), ms_per_step=round(dt * 1e3, 2), frames_per_s=round(n / dt, 1),
                              algorithmic_tflop_per_step=round(flops / 1e12, 2),
                              tflops=round(flops / dt / 1e12, 1), trainable_tensors=len(tr.tensors),
                              workspace_gib=round(ws_gb, 2), loss=round(float(loss), 4),
                              loss_scale=tr.scaler.scale, skipped_last=bool(tr.last['skipped']),
                              cpu_baseline=cb,
                              kernel_ms_per_step={p['name']: round(p['total_ms'] / a.steps, 2) for p in prof
                                                  if p['launches']})), flush=True)
        del tr, clf, model
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
