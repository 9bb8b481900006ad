"""fp32 CPU restatement of OpenAI CLIP's ModifiedResNet image tower (Bottleneck, AttentionPool2d), built from
nn.Conv2d / nn.BatchNorm2d (eval) / nn.AvgPool2d and F.multi_head_attention_forward, loading the state dict in
OpenAI's key layout.  ``emulate16=True`` rounds as the reference's fp16 GPU model does: conv inputs, weights and
outputs in fp16, BatchNorm in fp32 with an fp16 output, the attention pool's tokens, projections and output in fp16.
``emulate16=torch.bfloat16`` rounds at the same places to bf16.  ``conv_classes`` walks the module tree for the shapes
the packed tower launches.  Test infrastructure only."""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F


def _r16(t, on):
    """t rounded to 16 bit when on: torch.bfloat16 rounds to bf16, any other true value to fp16."""
    if not on:
        return t
    return t.to(torch.bfloat16 if on is torch.bfloat16 else torch.float16).float()


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.avgpool = nn.AvgPool2d(stride) if stride > 1 else nn.Identity()
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = None
        if stride > 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(OrderedDict([
                ('-1', nn.AvgPool2d(stride)), ('0', nn.Conv2d(inplanes, planes * 4, 1, bias=False)),
                ('1', nn.BatchNorm2d(planes * 4))]))

    def forward(self, x, e=False):
        cb = _ConvBN(e)
        out = F.relu(cb(self.conv1, self.bn1, x))
        out = F.relu(cb(self.conv2, self.bn2, out))
        out = _r16(self.avgpool(out), e)
        out = cb(self.conv3, self.bn3, out)
        idt = x
        if self.downsample is not None:
            ds = self.downsample
            idt = cb(ds[1], ds[2], _r16(ds[0](x), e))
        return _r16(F.relu(out + idt), e)


class _ConvBN:
    def __init__(self, e):
        self.e = e

    def __call__(self, conv, bn, x):
        e = self.e
        if not e:
            return bn(conv(x))
        y = _r16(F.conv2d(_r16(x, e), _r16(conv.weight, e), None, conv.stride, conv.padding), e)
        return _r16(bn(y), e)


class AttentionPool2d(nn.Module):
    def __init__(self, spacial_dim, embed_dim, num_heads, output_dim):
        super().__init__()
        self.positional_embedding = nn.Parameter(torch.zeros(spacial_dim ** 2 + 1, embed_dim))
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.c_proj = nn.Linear(embed_dim, output_dim)
        self.num_heads = num_heads

    def forward(self, x, e=False):
        x = x.flatten(start_dim=2).permute(2, 0, 1)
        x = torch.cat([x.mean(dim=0, keepdim=True), x], dim=0)
        x = _r16(x + self.positional_embedding[:, None, :], e)
        if e:       # fp16 projections, fp32 softmax-attention core on them, fp16 output
            C, H = x.shape[-1], self.num_heads
            q = _r16(F.linear(x[:1], _r16(self.q_proj.weight, e), self.q_proj.bias), e)
            k = _r16(F.linear(x, _r16(self.k_proj.weight, e), self.k_proj.bias), e)
            v = _r16(F.linear(x, _r16(self.v_proj.weight, e), self.v_proj.bias), e)
            L, N = x.shape[:2]
            qh = q.reshape(1, N * H, 64).transpose(0, 1) * 0.125
            kh = k.reshape(L, N * H, 64).transpose(0, 1)
            vh = v.reshape(L, N * H, 64).transpose(0, 1)
            a = torch.softmax(qh @ kh.transpose(1, 2), -1) @ vh
            a = _r16(a.transpose(0, 1).reshape(1, N, C), e)
            return F.linear(a, _r16(self.c_proj.weight, e), self.c_proj.bias)[0]
        x, _ = F.multi_head_attention_forward(
            query=x[:1], key=x, value=x, embed_dim_to_check=x.shape[-1], num_heads=self.num_heads,
            q_proj_weight=self.q_proj.weight, k_proj_weight=self.k_proj.weight, v_proj_weight=self.v_proj.weight,
            in_proj_weight=None, in_proj_bias=torch.cat([self.q_proj.bias, self.k_proj.bias, self.v_proj.bias]),
            bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0, out_proj_weight=self.c_proj.weight,
            out_proj_bias=self.c_proj.bias, use_separate_proj_weight=True, training=False, need_weights=False)
        return x.squeeze(0)


class ModifiedResNet(nn.Module):
    def __init__(self, layers, output_dim, heads, input_resolution=224, width=64):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width // 2, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width // 2)
        self.conv2 = nn.Conv2d(width // 2, width // 2, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width // 2)
        self.conv3 = nn.Conv2d(width // 2, width, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(width)
        self.avgpool = nn.AvgPool2d(2)
        self._inplanes = width
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2)
        self.attnpool = AttentionPool2d(input_resolution // 32, width * 32, heads, output_dim)

    def _make_layer(self, planes, blocks, stride=1):
        layers = [Bottleneck(self._inplanes, planes, stride)]
        self._inplanes = planes * 4
        layers += [Bottleneck(self._inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x, emulate16=False, bn_outputs=None):
        e = emulate16
        if bn_outputs is not None:          # records |max| of every BatchNorm output
            hooks = [m.register_forward_hook(lambda m, i, o: bn_outputs.append(float(o.abs().max())))
                     for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        cb = _ConvBN(e)
        x = F.relu(cb(self.conv1, self.bn1, _r16(x, e)))
        x = F.relu(cb(self.conv2, self.bn2, x))
        x = F.relu(cb(self.conv3, self.bn3, x))
        x = _r16(self.avgpool(x), e)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                x = blk(x, e)
        out = self.attnpool(x, e)
        if bn_outputs is not None:
            for h in hooks:
                h.remove()
        return out


def from_state_dict(sd, cfg):
    """The restatement with the ``visual.*`` weights of an OpenAI-layout state dict loaded (eval mode)."""
    w = cfg['vision_width']
    m = ModifiedResNet(cfg['vision_layers'], cfg['embed_dim'], w * 32 // 64, cfg['image_size'], w)
    vis = {k[len('visual.'):]: v for k, v in sd.items() if k.startswith('visual.')}
    m.load_state_dict(vis, strict=True)
    return m.eval()


def flops_by_walk(model, image_size):
    """2 x MACs of every Conv2d and of the attention pool's projections, from forward hooks on one image."""
    total = [0]

    def conv_hook(m, i, o):
        total[0] += 2 * o.numel() * m.in_channels * m.kernel_size[0] * m.kernel_size[1] // m.groups

    hooks = [m.register_forward_hook(conv_hook) for m in model.modules() if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        x = torch.zeros(1, 3, image_size, image_size)
        feat = x
        for name in ('conv1', 'bn1', 'conv2', 'bn2', 'conv3', 'bn3', 'avgpool', 'layer1', 'layer2', 'layer3',
                     'layer4'):
            feat = getattr(model, name)(feat)
    for h in hooks:
        h.remove()
    ap = model.attnpool
    L, C = feat.shape[2] * feat.shape[3] + 1, feat.shape[1]
    total[0] += 2 * (C * ap.q_proj.out_features + 2 * L * C * C + C * ap.c_proj.out_features)
    return total[0]


def _pad64(c):
    return (c + 63) // 64 * 64


def conv_classes(cfg):
    """The convolutions of the tower of ``cfg`` (full ModifiedResNet module tree, built on the meta device) as the
    packed tower launches them, from forward hooks on a meta-device forward (nothing is computed): {(ks, cin, cout, H_in): set of roles} with the channels padded to multiples of 64, and the
    attention pool's projections [(role, cin, cout, L)].  Every convolution runs at stride 1 on its input's H: the
    stem's stride-2 conv1 is the 1x1 product over the 64-wide stem rows at R / 2, and a downsample or a stride-2
    conv3 reads the AvgPool2d's output.  Roles: 'relu' (BatchNorm + ReLU), 'resid' (BatchNorm + residual + ReLU),
    'ds' (BatchNorm, no ReLU); projections 'q' (M = n images), 'kv' (M = n * L), 'c' (M = n, fp32 store)."""
    with torch.device('meta'):
        w = cfg['vision_width']
        meta = ModifiedResNet(cfg['vision_layers'], cfg['embed_dim'], w * 32 // 64, cfg['image_size'], w)
    image_size = cfg['image_size']
    roles = {}
    for name, m in meta.named_modules():
        if isinstance(m, nn.Conv2d):
            leaf = name.rsplit('.', 1)[-1]
            roles[m] = 'resid' if leaf == 'conv3' and name.startswith('layer') else \
                'ds' if name.endswith('downsample.0') else 'relu'
    out, pool_in = {}, []

    def conv_hook(m, i, o):
        h = i[0].shape[2]
        if m.stride[0] == 2:          # the stem's conv1 on the stem rows
            key = (1, 64, _pad64(m.out_channels), h // 2)
        else:
            key = (m.kernel_size[0], _pad64(m.in_channels), _pad64(m.out_channels), h)
        out.setdefault(key, set()).add(roles[m])

    hooks = [m.register_forward_hook(conv_hook) for m in roles]
    hooks.append(meta.attnpool.register_forward_pre_hook(lambda m, i: pool_in.append(i[0].shape)))
    try:
        with torch.no_grad():
            meta(torch.zeros(1, 3, image_size, image_size, device='meta'))
    finally:
        for h in hooks:
            h.remove()
    _, C, h, w = pool_in[0]
    ap = meta.attnpool
    L = h * w + 1
    assert ap.q_proj.in_features == ap.k_proj.in_features == ap.v_proj.in_features == C
    proj = [('q', C, ap.q_proj.out_features, L), ('kv', C, ap.k_proj.out_features + ap.v_proj.out_features, L),
            ('c', C, ap.c_proj.out_features, L)]
    return out, proj
