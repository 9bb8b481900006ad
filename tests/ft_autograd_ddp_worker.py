"""Worker of tests/test_ft_autograd_gpu.py::test_two_ranks_under_distributed_data_parallel (not a test itself): an
autograd-enabled FTCLIPClassifier inside DistributedDataParallel, two gloo ranks on the one GPU, each with half of a
batch; rank 0 also steps a second classifier alone on the whole batch and prints one JSON line."""
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def build(case, seed):
    import test_ft_autograd_gpu as A
    z, c = A.T._golden_case(case)
    torch.manual_seed(seed)                       # the LoRA down factors are drawn at construction, the up factors below
    clf = A.autograd_classifier(c, load_factors=False)
    with torch.no_grad():                         # (up = 0 as injected would leave every down factor without a gradient)
        for n, p in clf.named_parameters():
            if '.lora_up' in n:
                p.normal_(0, 0.02)
    imgs = torch.cat([c['imgs'], c['imgs'].flip(0)])[:4]
    valid = torch.cat([c['valid'], c['valid'].flip(0)])[:4]
    labels = torch.cat([c['labels'], c['labels'].flip(0)])[:4]
    return clf, {'img': imgs.cuda(), 'valid_mask': valid.cuda(), 'label': labels.cuda()}, float(z['lr']), float(z['clip_lr'])


def step(clf, model, data, opt):
    opt.zero_grad(set_to_none=True)
    loss = clf.calc_train_loss(data, model(data))['ce_loss']
    loss.backward()
    grads = {n: p.grad.clone() for n, p in clf.named_parameters() if p.grad is not None}
    opt.step()
    return float(loss), grads


def main():
    import test_ft_autograd_gpu as A
    case = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    dist.init_process_group('gloo')
    # every rank draws its own factors: DistributedDataParallel starts them all from rank 0's
    clf, data, lr, clip_lr = build(case, seed=100 + rank)
    ddp = torch.nn.parallel.DistributedDataParallel(clf, device_ids=[0])
    half = {k: v[2 * rank:2 * rank + 2] for k, v in data.items()}
    loss, grads = step(clf, ddp, half, A.two_group_adam(clf, lr, clip_lr))
    after = torch.cat([p.detach().flatten() for p in clf.parameters()]).cpu()
    gathered = [torch.empty_like(after) for _ in range(world)]
    dist.all_gather(gathered, after)
    losses = [torch.zeros(1) for _ in range(world)]
    dist.all_gather(losses, torch.tensor([loss]))
    if rank == 0:
        alone, data, lr, clip_lr = build(case, seed=100)
        loss_whole, whole = step(alone, alone, data, A.two_group_adam(alone, lr, clip_lr))
        worst, worst_cos, W = 0.0, 1.0, alone.model.cfg['width']
        for n, g in whole.items():
            a, b = grads[n].flatten().cpu(), g.flatten().cpu()
            if n.endswith('attn.in_proj_bias'):               # zero key-bias gradient: q and v rows only
                sel = torch.cat([torch.arange(W), torch.arange(2 * W, 3 * W)])
                a, b = a[sel], b[sel]
            else:
                worst_cos = min(worst_cos, A.T.cosine(a, b))
            worst = max(worst, A.T.rel_l2(a, b))
        print(json.dumps(dict(world=world, tensors=len(whole), same_names=sorted(whole) == sorted(grads),
                              loss_mean_of_ranks=float(sum(losses)) / world, loss_whole=loss_whole,
                              worst_grad_rel_l2=worst, worst_grad_cosine=worst_cos,
                              params_equal_after_step=bool(torch.equal(gathered[0], gathered[1])),
                              moved=bool((after - torch.cat([p.detach().flatten() for p in alone.parameters()]).cpu()).abs().max()
                                         < 1e-2))))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
