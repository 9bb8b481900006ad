"""Golden vectors of the REFERENCE's own models/adapter.py TransformerAdapter(norm_first=False): the post-LN layout.
The reference module is loaded by path (build container only).  Writes tests/golden/adapter_postln.npz: the state dict
('w:<key>', and 'keys'), inputs ('feats' with zero rows on padded views, 'valid', 'd_out'), the output and, for the loss
sum(out * d_out) over the valid views, every parameter gradient ('g:<key>') and the input gradient ('g_feats').  fp32, the
module in eval mode with grad enabled, so torch runs its plain math path.

    python tools/make_golden_adapter_postln.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLD = os.path.join(ROOT, 'tests', 'golden')
REF_ADAPTER = '/root/reference/models/adapter.py'

from adapter_postln_ref import FIXTURE_GEOMETRY as G  # noqa: E402
import fewshot_ref as fr  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location('ref_adapter', REF_ADAPTER)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(20)
    residual = 0.5
    ad = ref.TransformerAdapter(in_dim=G['D'], d_model=G['d'], num_heads=G['heads'], ffn_dim=G['ffn'], norm_first=False,
                                num_layers=G['layers'], residual=residual).float().eval()
    with torch.no_grad():           # LayerNorm gains and biases off their 1 / 0 init, so that a swapped pair shows
        for n, p in ad.named_parameters():
            if 'norm' in n or n.endswith('bias'):
                p.add_(0.2 * torch.randn_like(p))
    feats, valid, d_out = fr.adapter_inputs(G['B'], G['T'], G['D'], seed=3)
    x = feats.clone().requires_grad_(True)
    with torch.enable_grad():
        out = ad(x, valid)
        (out * d_out * valid[..., None]).sum().backward()
    z = {'w:' + k: v.numpy() for k, v in ad.state_dict().items()}
    z['keys'] = np.array(list(ad.state_dict()))
    z.update({'g:' + k: p.grad.numpy() for k, p in ad.named_parameters()})
    z.update(feats=feats.numpy(), valid=valid.numpy(), d_out=d_out.numpy(), out=out.detach().numpy(), g_feats=x.grad.numpy(),
             residual=np.float32(residual))
    path = os.path.join(GOLD, 'adapter_postln.npz')
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
