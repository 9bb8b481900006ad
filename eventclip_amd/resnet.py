"""ResNet CLIP (OpenAI ``ModifiedResNet`` image tower + the transformer text tower) on HIP kernels.

The image tower runs on csrc/resnet.hip: NHWC 16-bit activations, every convolution an implicit GEMM on MFMA
with BatchNorm as an fp32 per-channel scale and bias in its epilogue, fused ReLU / residual
epilogues, 2x2 average pooling, and the attention pool (token building, q / k+v / c projections as 1x1
GEMMs, one query per head), all driven by ec_resnet_encode (torch.ops.eventclip_hip.resnet_encode).  Channel
counts that are not multiples of 64 are padded with zero channels at pack time.  The text tower is ``ec_text_encode``, as for the ViT models.

``precise_blocks`` selects the tower's split-precision form (csrc/resnet_hl.hip): activations and weights as f16 hi + lo
planes, three MFMA products per convolution, fp32 in between -- the ResNet side of ``clip.tolerance_mode_kwargs``.

Architecture facts follow OpenAI's ``clip/model.py`` (``ModifiedResNet``, ``Bottleneck``, ``AttentionPool2d``,
``build_model``)."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .clip_base import ClipBase, Packer

# layers, width w, image size, embed dim, text width / heads (text layers 12, context 77, vocab 49408 for all)
RESNET_ARCHS = {
    'RN50': dict(vision_layers=(3, 4, 6, 3), vision_width=64, image_size=224, embed_dim=1024,
                 text_width=512, text_heads=8, text_layers=12),
    'RN101': dict(vision_layers=(3, 4, 23, 3), vision_width=64, image_size=224, embed_dim=512,
                  text_width=512, text_heads=8, text_layers=12),
    'RN50x4': dict(vision_layers=(4, 6, 10, 6), vision_width=80, image_size=288, embed_dim=640,
                   text_width=640, text_heads=10, text_layers=12),
    'RN50x16': dict(vision_layers=(6, 8, 18, 8), vision_width=96, image_size=384, embed_dim=768,
                    text_width=768, text_heads=12, text_layers=12),
    'RN50x64': dict(vision_layers=(3, 15, 36, 10), vision_width=128, image_size=448, embed_dim=1024,
                    text_width=1024, text_heads=16, text_layers=12),
}
BN_EPS = 1e-5
LO_SCALE = 2048.0       # the lo plane of a split value holds (v - hi) * 2^11 (csrc/resnet_hl.hip)


def split_hl(t):
    """fp32 tensor -> (hi, lo) f16 planes of the split-precision kernels: hi = f16(t), lo = f16((t - hi) * 2^11).
    t - hi is exact in fp32, the scaling is exact, so hi + lo / 2^11 restores t to 2^-22 |t| + 2^-36 (one f16 rounding
    of lo, which is at most 2^-11 |t| before the scaling and normal wherever hi is; 2^-25 / 2^11 below that)."""
    t = t.float()
    hi = t.to(torch.float16)
    lo = ((t - hi.float()) * LO_SCALE).to(torch.float16)
    return hi, lo


def is_resnet_config(cfg):
    return 'vision_layers' in cfg


def resnet_config(name, **override):
    from .clip import CONTEXT_LENGTH, VOCAB_SIZE
    if name not in RESNET_ARCHS:
        raise RuntimeError(f'{name} is not a ResNet CLIP architecture; one of {list(RESNET_ARCHS)}')
    cfg = dict(RESNET_ARCHS[name], context_length=CONTEXT_LENGTH, vocab_size=VOCAB_SIZE)
    cfg.update(override)
    cfg['vision_layers'] = tuple(cfg['vision_layers'])
    return cfg


def pad64(c):
    return (c + 63) // 64 * 64


def blocks_of(cfg):
    """(key prefix, inplanes, planes, stride, has downsample) of every Bottleneck, in order."""
    w = cfg['vision_width']
    inplanes, out = w, []
    for li, n in enumerate(cfg['vision_layers']):
        planes = w * (1 << li)
        for i in range(n):
            stride = (1 if li == 0 else 2) if i == 0 else 1
            out.append((f'visual.layer{li + 1}.{i}', inplanes, planes, stride,
                        stride > 1 or inplanes != planes * 4))
            inplanes = planes * 4
    return out


def resnet_flops(cfg, padded=False):
    """Multiply-add FLOPs (2 per MAC) of one image through the convolutions and the attention pool's four
    projections.  padded=True counts the channels as the kernels run them (padded to 64; the stem's 27-wide
    K padded to 64)."""
    p = pad64 if padded else (lambda c: c)
    w, R = cfg['vision_width'], cfg['image_size']
    h = R // 2
    macs = h * h * (64 if padded else 27) * p(w // 2)
    macs += h * h * 9 * p(w // 2) * p(w // 2) + h * h * 9 * p(w // 2) * p(w)
    h //= 2
    for _, inp, planes, stride, ds in blocks_of(cfg):
        ho = h // stride
        macs += h * h * p(inp) * p(planes) + h * h * 9 * p(planes) ** 2 + ho * ho * p(planes) * p(4 * planes)
        if ds:
            macs += ho * ho * p(inp) * p(4 * planes)
        h = ho
    C, L = 32 * w, h * h + 1
    macs += C * C + 2 * L * C * C + C * cfg['embed_dim']
    return 2 * macs


# ---- seeded random weights in OpenAI's key layout, BatchNorm statistics calibrated ----
def _bn_keys(prefix):
    return [f'{prefix}.{k}' for k in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')]


def random_state_dict(cfg, seed=0, calib_images=2, branch_gain=0.25):
    """Seeded random ResNet CLIP weights (fp32, CPU) with OpenAI's key names.  Convolutions get He-style scales,
    BatchNorm affine terms are perturbed, and the BatchNorm running statistics are then calibrated: a seeded batch
    of ``calib_images`` N(0, 1) images runs through the fp32 tower and every BatchNorm takes the batch mean and
    variance of its input, so that every BatchNorm output is about unit scale at any depth (uncalibrated random
    statistics overflow fp16 within a few blocks).  ``branch_gain`` scales every Bottleneck's last BatchNorm gain
    (bn3.weight) against the identity path: with 1 the random towers amplify a 16-bit rounding to 8 - 30 % of the
    features at full RN50 / RN101 depth, which would hide a real error in a deep block.  The text tower's weights are
    those of the ViT generator."""
    from . import clip
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    sd = {}

    def conv(key, cout, cin, k):
        sd[key] = rn(cout, cin, k, k, std=(cin * k * k) ** -0.5)

    def bn(prefix, c):
        kw, kb, km, kv, kn = _bn_keys(prefix)
        sd[kw] = 1 + rn(c, std=0.1)
        sd[kb] = rn(c, std=0.1)
        sd[km] = torch.zeros(c)
        sd[kv] = torch.ones(c)
        sd[kn] = torch.tensor(0, dtype=torch.long)

    w = cfg['vision_width']
    conv('visual.conv1.weight', w // 2, 3, 3)
    bn('visual.bn1', w // 2)
    conv('visual.conv2.weight', w // 2, w // 2, 3)
    bn('visual.bn2', w // 2)
    conv('visual.conv3.weight', w, w // 2, 3)
    bn('visual.bn3', w)
    for pre, inp, planes, stride, ds in blocks_of(cfg):
        conv(f'{pre}.conv1.weight', planes, inp, 1)
        bn(f'{pre}.bn1', planes)
        conv(f'{pre}.conv2.weight', planes, planes, 3)
        bn(f'{pre}.bn2', planes)
        conv(f'{pre}.conv3.weight', planes * 4, planes, 1)
        bn(f'{pre}.bn3', planes * 4)
        sd[f'{pre}.bn3.weight'] *= branch_gain
        if ds:
            conv(f'{pre}.downsample.0.weight', planes * 4, inp, 1)
            bn(f'{pre}.downsample.1', planes * 4)
    C, E = 32 * w, cfg['embed_dim']
    sp = cfg['image_size'] // 32
    sd['visual.attnpool.positional_embedding'] = rn(sp * sp + 1, C, std=C ** -0.5)
    for n, o in (('q', C), ('k', C), ('v', C), ('c', E)):
        sd[f'visual.attnpool.{n}_proj.weight'] = rn(o, C, std=C ** -0.5)
        sd[f'visual.attnpool.{n}_proj.bias'] = rn(o, std=0.02)
    # text tower (and logit_scale): the ViT generator's, with a stub vision tower that is dropped
    stub = {k: v for k, v in cfg.items() if k != 'vision_layers'}
    stub.update(width=64, patch=32, image_size=32, layers=1)
    for k, v in clip.random_state_dict(stub, seed=seed + 1).items():
        if not k.startswith('visual.'):
            sd[k] = v
    if calib_images:            # (0: running statistics left at 0 / 1 -- key-layout tests only)
        x = torch.randn(calib_images, 3, cfg['image_size'], cfg['image_size'], generator=g)
        with torch.no_grad():
            forward_fp32(sd, cfg, x, calibrate=True)
    return sd


def forward_fp32(sd, cfg, x, calibrate=False):
    """The image tower in fp32 on the CPU with torch.nn.functional (x: normalised [N, 3, R, R] -> [N, embed_dim]).
    calibrate=True writes every BatchNorm's running statistics from its input batch first (random_state_dict)."""
    def bn(t, prefix):
        kw, kb, km, kv, _ = _bn_keys(prefix)
        if calibrate:
            sd[km] = t.mean((0, 2, 3))
            sd[kv] = t.var((0, 2, 3), unbiased=False)
        return F.batch_norm(t, sd[km], sd[kv], sd[kw], sd[kb], False, 0.0, BN_EPS)

    x = F.relu(bn(F.conv2d(x, sd['visual.conv1.weight'], stride=2, padding=1), 'visual.bn1'))
    x = F.relu(bn(F.conv2d(x, sd['visual.conv2.weight'], padding=1), 'visual.bn2'))
    x = F.relu(bn(F.conv2d(x, sd['visual.conv3.weight'], padding=1), 'visual.bn3'))
    x = F.avg_pool2d(x, 2)
    for pre, _, _, stride, ds in blocks_of(cfg):
        o = F.relu(bn(F.conv2d(x, sd[f'{pre}.conv1.weight']), f'{pre}.bn1'))
        o = F.relu(bn(F.conv2d(o, sd[f'{pre}.conv2.weight'], padding=1), f'{pre}.bn2'))
        if stride > 1:
            o = F.avg_pool2d(o, stride)
        o = bn(F.conv2d(o, sd[f'{pre}.conv3.weight']), f'{pre}.bn3')
        idt = x
        if ds:
            idt = F.avg_pool2d(x, stride) if stride > 1 else x
            idt = bn(F.conv2d(idt, sd[f'{pre}.downsample.0.weight']), f'{pre}.downsample.1')
        x = F.relu(o + idt)
    n, C = x.shape[:2]
    t = x.flatten(2).permute(2, 0, 1)                                   # [HW, N, C]
    t = torch.cat([t.mean(0, keepdim=True), t]) + sd['visual.attnpool.positional_embedding'][:, None, :]
    a = 'visual.attnpool.'
    out, _ = F.multi_head_attention_forward(
        query=t[:1], key=t, value=t, embed_dim_to_check=C, num_heads=C // 64,
        q_proj_weight=sd[a + 'q_proj.weight'], k_proj_weight=sd[a + 'k_proj.weight'],
        v_proj_weight=sd[a + 'v_proj.weight'], in_proj_weight=None,
        in_proj_bias=torch.cat([sd[a + 'q_proj.bias'], sd[a + 'k_proj.bias'], sd[a + 'v_proj.bias']]),
        bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=sd[a + 'c_proj.weight'],
        out_proj_bias=sd[a + 'c_proj.bias'], use_separate_proj_weight=True, training=False, need_weights=False)
    return out[0]


def config_from_state_dict(sd):
    """OpenAI build_model's rules for a ResNet checkpoint."""
    layers = tuple(len({k.split('.')[2] for k in sd if k.startswith(f'visual.layer{b}.')}) for b in (1, 2, 3, 4))
    w = sd['visual.layer1.0.conv1.weight'].shape[0]
    grid = round((sd['visual.attnpool.positional_embedding'].shape[0] - 1) ** 0.5)
    assert grid ** 2 + 1 == sd['visual.attnpool.positional_embedding'].shape[0]
    TW = sd['ln_final.weight'].shape[0]
    return dict(vision_layers=layers, vision_width=w, image_size=grid * 32, embed_dim=sd['text_projection'].shape[1],
                text_width=TW, text_heads=TW // 64,
                text_layers=len({k.split('.')[2] for k in sd if k.startswith('transformer.resblocks.')}),
                context_length=sd['positional_embedding'].shape[0], vocab_size=sd['token_embedding.weight'].shape[0])


class ResNetCLIP(ClipBase):
    """Frozen ResNet CLIP on HIP kernels: the surface of ``clip.CLIP`` the classifiers read (encode_image,
    encode_text, visual.output_dim / input_resolution, logit_scale, state_dict in OpenAI's keys), plus
    ``encode_frames`` for the uint8 frames of ``ec_preprocess`` (EC_PRE_HWC_U8)."""

    def __init__(self, cfg, state_dict, dtype='float16', chunk=64, precise_blocks=0, precise=False):
        """precise_blocks: 0, the 16-bit tower; n_blocks (or precise=True), the stem, every Bottleneck and the attention
        pool on split-precision (hi + lo) operands; 0 < n < n_blocks, the stem and the first n Bottlenecks."""
        super().__init__(cfg, state_dict, dtype, chunk)
        n_blocks = sum(cfg['vision_layers'])
        self.precise_blocks = n_blocks if precise else int(precise_blocks)
        if not 0 <= self.precise_blocks <= n_blocks:
            raise ValueError(f'precise_blocks={precise_blocks} outside 0 .. {n_blocks} (the Bottlenecks of this tower)')
        if self.precise_blocks and self.compute_dtype != torch.float16:
            raise ValueError(f'precise_blocks={self.precise_blocks} needs dtype float16 (the split-precision kernels '
                             'carry f16 hi + lo planes; bfloat16 is not supported)')

    @property
    def dtype_code(self):
        return _lib.EC_F16 if self.compute_dtype == torch.float16 else _lib.EC_BF16

    # ---- device packing ----
    def _pack(self):
        if self._packed is not None:
            return self._packed
        dev = self._pack_device()
        sd = {k: v.detach().float().cpu() for k, v in self.state_dict().items()}
        cd = self.compute_dtype
        keep = []

        def up(t, dtype):
            t = t.to(dev).to(dtype).contiguous()
            keep.append(t)
            return t

        pb = self.precise_blocks

        def cw(wp, scale, bias, ks, cin, cout, split=False):
            r = _lib.EcResnetConvW()
            if split:       # hi is the 16-bit path's weight bit for bit; lo what that rounding lost
                hi, lo = split_hl(wp)
                r.w, r.w_lo = up(hi, cd).data_ptr(), up(lo, cd).data_ptr()
            else:
                r.w = up(wp, cd).data_ptr()
            r.scale = None if scale is None else up(scale, torch.float32).data_ptr()
            r.bias = up(bias, torch.float32).data_ptr()
            r.ks, r.cin, r.cout = ks, cin, cout
            return r

        def conv(wkey, bn_prefix, cin_p, cout_p, rows27=False, split=False):
            # the weights as the checkpoint holds them (one rounding to 16 bit); BatchNorm as an fp32 per-channel
            # scale and bias in the epilogue -- folding the scale into the weights would add a rounding of w * scale
            wt = sd[wkey]
            cout, cin, k, _ = wt.shape
            kw, kb, km, kv, _ = _bn_keys(bn_prefix)
            s = sd[kw] / torch.sqrt(sd[kv] + BN_EPS)
            scale, bias = torch.zeros(cout_p), torch.zeros(cout_p)
            scale[:cout], bias[:cout] = s, sd[kb] - sd[km] * s
            wf = wt.permute(0, 2, 3, 1)                                 # [Cout, ky, kx, Cin]
            if rows27:      # the stem's rows (ec_resnet_stem_rows): a 1x1 product over k = (ky*3 + kx)*3 + c
                wp = torch.zeros(cout_p, 64)
                wp[:cout, :27] = wf.reshape(cout, 27)
                if not split:   # (split: ec_resnet_stem_rows_hl carries the remainders in the rows' lo plane)
                    wp[:cout, 27:54] = wf.reshape(cout, 27)             # times the rows' rounding remainders
                return cw(wp, scale, bias, 1, 64, cout_p, split)
            wp = torch.zeros(cout_p, k, k, cin_p)
            wp[:cout, :, :, :cin] = wf
            return cw(wp, scale, bias, k, cin_p, cout_p, split)

        def linear(wt, b):
            return cw(wt, None, b, 1, wt.shape[1], wt.shape[0], pb == len(spec))

        c = self.cfg
        w = c['vision_width']
        rw = _lib.EcResnetWeights()
        rw.struct_bytes = ctypes.sizeof(_lib.EcResnetWeights)
        rw.dtype, rw.image_size, rw.embed_dim = self.dtype_code, c['image_size'], c['embed_dim']
        spec = blocks_of(c)
        sp = pb > 0
        rw.stem[0] = conv('visual.conv1.weight', 'visual.bn1', 64, pad64(w // 2), rows27=True, split=sp)
        rw.stem[1] = conv('visual.conv2.weight', 'visual.bn2', pad64(w // 2), pad64(w // 2), split=sp)
        rw.stem[2] = conv('visual.conv3.weight', 'visual.bn3', pad64(w // 2), pad64(w), split=sp)
        blocks = (_lib.EcResnetBlock * len(spec))()
        for i, (bk, (pre, inp, planes, stride, ds)) in enumerate(zip(blocks, spec)):
            sp = i < pb
            bk.stride = stride
            bk.c1 = conv(f'{pre}.conv1.weight', f'{pre}.bn1', pad64(inp), pad64(planes), split=sp)
            bk.c2 = conv(f'{pre}.conv2.weight', f'{pre}.bn2', pad64(planes), pad64(planes), split=sp)
            bk.c3 = conv(f'{pre}.conv3.weight', f'{pre}.bn3', pad64(planes), pad64(4 * planes), split=sp)
            if ds:
                bk.ds = conv(f'{pre}.downsample.0.weight', f'{pre}.downsample.1', pad64(inp), pad64(4 * planes), split=sp)
        rw.n_blocks = len(spec)
        rw.precise_blocks = pb
        rw.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.EcResnetBlock))
        a = 'visual.attnpool.'
        rw.pos = up(sd[a + 'positional_embedding'], torch.float32).data_ptr()
        rw.q = linear(sd[a + 'q_proj.weight'], sd[a + 'q_proj.bias'])
        rw.kv = linear(torch.cat([sd[a + 'k_proj.weight'], sd[a + 'v_proj.weight']]),
                       torch.cat([sd[a + 'k_proj.bias'], sd[a + 'v_proj.bias']]))
        rw.c = linear(sd[a + 'c_proj.weight'], sd[a + 'c_proj.bias'])
        # the transformer text tower, split-precision (hi + lo) as CLIP packs it by default
        text, tb = Packer(sd, dev, cd, c, keep=keep).text(precise=True)
        self._packed = dict(resnet=rw, blocks=blocks, text=text, tb=tb, keep=keep, dev=dev, code=self.dtype_code)
        return self._packed

    # ---- image tower ----
    def _encode(self, inp, mode):
        from . import torch_ops
        return torch.ops.eventclip_hip.resnet_encode(inp.contiguous(), int(mode), torch_ops.handle_of(self))

    @torch.no_grad()
    def encode_image(self, image):
        """image: float tensor [N, 3, R, R] as CLIP's preprocess produces -> fp32 [N, D]."""
        pk = self._pack()
        R = self.cfg['image_size']
        if image.dim() != 4 or tuple(image.shape[1:]) != (3, R, R):
            raise ValueError(f'encode_image expects [N, 3, {R}, {R}], got {tuple(image.shape)}')
        return self._encode(image.to(pk['dev'], torch.float32).contiguous(), _lib.EC_PRE_CHW_F32)

    @torch.no_grad()
    def encode_frames(self, frames):
        """frames: uint8 CUDA tensor [N, R, R, 3] (preprocess_frames(..., mode='u8')) -> fp32 [N, D]; ToTensor and
        Normalize run inside the stem kernel."""
        self._pack()
        R = self.cfg['image_size']
        if frames.dtype != torch.uint8 or tuple(frames.shape[1:]) != (R, R, 3) or not frames.is_cuda:
            raise ValueError(f'encode_frames expects uint8 CUDA [N, {R}, {R}, 3], got {tuple(frames.shape)}')
        return self._encode(frames.contiguous(), _lib.EC_PRE_HWC_U8)


def padded_flop_overhead(cfg):
    """Fraction of extra FLOPs the zero channels of the packed tower cost (0 for RN50 / RN101 / RN50x64 but for
    the stem's 27 -> 64 K padding)."""
    return resnet_flops(cfg, padded=True) / resnet_flops(cfg) - 1.0

