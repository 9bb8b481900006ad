"""The `clip` module surface the reference uses, backed by the HIP towers.

The reference imports OpenAI's ``clip`` package (un-vendored) and touches exactly
this much of it:

* ``clip.load(arch, device) -> (model, preprocess)``          test.py:26
* ``clip.tokenize(str) -> IntTensor[1, 77]``                   models/clip_cls.py:81-83
* ``model.encode_image(FloatTensor[N,3,R,R]) -> [N, D]``      models/clip_cls.py:101
* ``model.encode_text(IntTensor[K,77]) -> [K, D]``            models/clip_cls.py:84
* ``model.logit_scale`` (0-dim Parameter), ``model.visual.output_dim``,
  ``.parameters()``, ``.eval()``, ``.state_dict()``           models/clip_cls.py:40-44,217; test.py:44

``CLIP`` below provides the same, with OpenAI's state-dict key names so released
checkpoints load unchanged.  The parameters are fp32 masters; 16-bit copies for
the MFMA GEMMs are packed once per device/dtype.  The ResNet backbones (RN50 ..
RN50x64) are ``resnet.ResNetCLIP``; ``build_random``, ``build_from_state_dict``
and ``load`` return one for a ResNet name or checkpoint.  Everything numeric runs
in libeventclip_hip.so; there is no CPU fallback.
"""
import ctypes
import gzip
import html
import os
from functools import lru_cache

import numpy as np
import torch

from . import _lib
from . import resnet as _resnet
from .clip_base import ATTN_Q_SCALE, ClipBase, Packer, _assign, _block_keys, patch_row_widths   # noqa: F401 (re-exported)
from .preprocess import Preprocess
from .resnet import RESNET_ARCHS, resnet_config

_RESNETS = tuple(RESNET_ARCHS)

# (image_size, patch, vision width, vision layers, embed dim, text width, text heads, text layers)
ARCHS = {
    'ViT-B/32': dict(image_size=224, patch=32, width=768, layers=12, embed_dim=512,
                     text_width=512, text_heads=8, text_layers=12),
    'ViT-B/16': dict(image_size=224, patch=16, width=768, layers=12, embed_dim=512,
                     text_width=512, text_heads=8, text_layers=12),
    'ViT-L/14': dict(image_size=224, patch=14, width=1024, layers=24, embed_dim=768,
                     text_width=768, text_heads=12, text_layers=12),
    'ViT-L/14@336px': dict(image_size=336, patch=14, width=1024, layers=24, embed_dim=768,
                           text_width=768, text_heads=12, text_layers=12),
}
CONTEXT_LENGTH = 77
VOCAB_SIZE = 49408

# The MLP activation, cfg['activation']: 'quick_gelu' = x sigmoid(1.702 x), OpenAI's checkpoints and the default everywhere;
# 'gelu' = x Phi(x), torch.nn.GELU(): every CLIP that open_clip trained without a -quickgelu suffix (LAION-400M / LAION-2B /
# DataComp / CommonPool ViT-B/32, B/16, L/14) and Hugging Face configs with hidden_act "gelu".  The key layout of the two
# families is the same and NOTHING in a state dict names the activation: the caller has to (build_from_state_dict / load
# take activation=...; an open_clip architecture name or an HF config.json say it themselves).
ACTIVATIONS = tuple(_lib.ACTIVATIONS)
# open_clip's spellings -> (architecture here, activation)
OPEN_CLIP_ARCHS = {
    'ViT-B-32': ('ViT-B/32', 'gelu'), 'ViT-B-16': ('ViT-B/16', 'gelu'), 'ViT-L-14': ('ViT-L/14', 'gelu'),
    'ViT-L-14-336': ('ViT-L/14@336px', 'gelu'),
    'ViT-B-32-quickgelu': ('ViT-B/32', 'quick_gelu'), 'ViT-B-16-quickgelu': ('ViT-B/16', 'quick_gelu'),
    'ViT-L-14-quickgelu': ('ViT-L/14', 'quick_gelu'), 'ViT-L-14-336-quickgelu': ('ViT-L/14@336px', 'quick_gelu'),
}
# open_clip towers whose attention heads are not 64 wide (width / heads): the attention kernels are built for 64
_OTHER_HEAD_DIM = {'ViT-H-14': 80, 'ViT-g-14': 88, 'ViT-bigG-14': 104}


def available_models():
    return list(_RESNETS) + list(ARCHS) + list(OPEN_CLIP_ARCHS)


def _check_activation(activation):
    if activation not in ACTIVATIONS:
        raise ValueError(f'unknown activation {activation!r}: one of {ACTIVATIONS}')
    return activation


def resolve_arch(name):
    """An architecture name in OpenAI's or open_clip's spelling -> (name in ARCHS, the activation the name implies or None).
    OpenAI's names and the ResNets imply nothing (None: the default, QuickGELU); open_clip's 'ViT-B-32' / 'ViT-B-16' / 'ViT-L-14'
    say exact GELU, '...-quickgelu' says QuickGELU; ViT-H / g / bigG raise (head dimension 80 / 88 / 104)."""
    base = name[:-len('-quickgelu')] if name.endswith('-quickgelu') else name
    if base in _OTHER_HEAD_DIM:
        raise NotImplementedError(f'{name}: its attention heads are {_OTHER_HEAD_DIM[base]} wide and the attention kernels are '
                                  'built for a head dimension of 64 (ViT-B/32, B/16, L/14)')
    if name in OPEN_CLIP_ARCHS:
        return OPEN_CLIP_ARCHS[name]
    return name, None


def arch_config(arch, **override):
    """Config of a ViT architecture (OpenAI's name, or open_clip's, which also sets cfg['activation']); ResNet names raise
    (their configs come from resnet_config)."""
    if arch in _RESNETS:
        raise NotImplementedError(f'{arch}: arch_config holds the ViT architectures; '
                                  f'use resnet_config({arch!r}) for the ResNet backbones')
    arch, implied = resolve_arch(arch)
    if arch not in ARCHS:
        raise RuntimeError(f'Model {arch} not found; available models = {available_models()}')
    cfg = dict(ARCHS[arch], context_length=CONTEXT_LENGTH, vocab_size=VOCAB_SIZE, activation=implied or 'quick_gelu')
    cfg.update(override)
    _check_activation(cfg['activation'])
    return cfg


def random_state_dict(cfg, seed=0, qk_gain=1.0, branch_gain=1.0):
    """Seeded random weights with OpenAI CLIP's key names and init scales (fp32, CPU).
    Biases and LayerNorm affine terms are perturbed too so every code path carries signal.

    At the plain init scales the image features of a random tower are ~98 % the same vector whatever the
    input (uniform attention averages the tokens; the (2 L)^-1/2 branch scaling keeps the class token's
    constant start dominant).  ``qk_gain`` scales the vision tower's query / key projections (sharper,
    content-dependent attention) and ``branch_gain`` its out_proj / c_proj (the branches against the residual
    stream): (6, 4) makes a third of the ViT-L/14 feature norm input-dependent -- the weights the logit-parity
    tests use, so that their error is measured against a signal and not against a constant."""
    if _resnet.is_resnet_config(cfg):
        if qk_gain != 1.0:
            raise ValueError('qk_gain applies to the ViT tower only')
        return _resnet.random_state_dict(cfg, seed=seed, **({} if branch_gain == 1.0 else dict(branch_gain=branch_gain)))
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    sd = {}

    def blocks(prefix, width, layers):
        attn_std = width ** -0.5
        proj_std = (width ** -0.5) * ((2 * layers) ** -0.5)
        fc_std = (2 * width) ** -0.5
        for i in range(layers):
            p = f'{prefix}.resblocks.{i}.'
            sd[p + 'ln_1.weight'] = 1 + rn(width, std=0.1)
            sd[p + 'ln_1.bias'] = rn(width, std=0.1)
            sd[p + 'attn.in_proj_weight'] = rn(3 * width, width, std=attn_std)
            sd[p + 'attn.in_proj_bias'] = rn(3 * width, std=0.02)
            sd[p + 'attn.out_proj.weight'] = rn(width, width, std=proj_std)
            sd[p + 'attn.out_proj.bias'] = rn(width, std=0.02)
            sd[p + 'ln_2.weight'] = 1 + rn(width, std=0.1)
            sd[p + 'ln_2.bias'] = rn(width, std=0.1)
            sd[p + 'mlp.c_fc.weight'] = rn(4 * width, width, std=fc_std)
            sd[p + 'mlp.c_fc.bias'] = rn(4 * width, std=0.02)
            sd[p + 'mlp.c_proj.weight'] = rn(width, 4 * width, std=proj_std)
            sd[p + 'mlp.c_proj.bias'] = rn(width, std=0.02)

    W, P, R = cfg['width'], cfg['patch'], cfg['image_size']
    scale = W ** -0.5
    sd['visual.conv1.weight'] = rn(W, 3, P, P, std=(3 * P * P) ** -0.5)
    sd['visual.class_embedding'] = rn(W, std=scale)
    sd['visual.positional_embedding'] = rn((R // P) ** 2 + 1, W, std=scale)
    sd['visual.ln_pre.weight'] = 1 + rn(W, std=0.1)
    sd['visual.ln_pre.bias'] = rn(W, std=0.1)
    blocks('visual.transformer', W, cfg['layers'])
    if qk_gain != 1.0 or branch_gain != 1.0:
        for i in range(cfg['layers']):
            p = f'visual.transformer.resblocks.{i}.'
            sd[p + 'attn.in_proj_weight'][:2 * W] *= qk_gain
            sd[p + 'attn.in_proj_bias'][:2 * W] *= qk_gain
            sd[p + 'attn.out_proj.weight'] *= branch_gain
            sd[p + 'mlp.c_proj.weight'] *= branch_gain
    sd['visual.ln_post.weight'] = 1 + rn(W, std=0.1)
    sd['visual.ln_post.bias'] = rn(W, std=0.1)
    sd['visual.proj'] = rn(W, cfg['embed_dim'], std=scale)
    TW = cfg['text_width']
    sd['token_embedding.weight'] = rn(cfg['vocab_size'], TW, std=0.02)
    sd['positional_embedding'] = rn(cfg['context_length'], TW, std=0.01)
    blocks('transformer', TW, cfg['text_layers'])
    sd['ln_final.weight'] = 1 + rn(TW, std=0.1)
    sd['ln_final.bias'] = rn(TW, std=0.1)
    sd['text_projection'] = rn(TW, cfg['embed_dim'], std=TW ** -0.5)
    sd['logit_scale'] = torch.tensor(float(np.log(100.0)))   # exp() = 100 for released weights
    return sd


def config_from_state_dict(sd):
    """Recover the architecture from an OpenAI-format state dict (ViT or ResNet)."""
    if 'visual.attnpool.positional_embedding' in sd:
        return _resnet.config_from_state_dict(sd)
    if 'visual.proj' not in sd:
        raise NotImplementedError('not an OpenAI CLIP checkpoint (neither visual.proj nor visual.attnpool)')
    W = sd['visual.conv1.weight'].shape[0]
    P = sd['visual.conv1.weight'].shape[-1]
    g = round((sd['visual.positional_embedding'].shape[0] - 1) ** 0.5)
    layers = len({k.split('.')[3] for k in sd if k.startswith('visual.transformer.resblocks.')})
    TW = sd['ln_final.weight'].shape[0]
    if W % 64 or TW % 64:
        raise NotImplementedError(f'widths {W} / {TW} are not multiples of the head dimension 64 the attention kernels are built for')
    return dict(image_size=g * P, patch=P, width=W, layers=layers,
                embed_dim=sd['text_projection'].shape[1], text_width=TW, text_heads=TW // 64,
                text_layers=len({k.split('.')[2] for k in sd
                                 if k.startswith('transformer.resblocks.')}),
                context_length=sd['positional_embedding'].shape[0],
                vocab_size=sd['token_embedding.weight'].shape[0])


# of the split-operand blocks (image_precise_blocks), how many run fp32-class attention (+ the MLP activation as hi + lo):
# (up to 288 tokens, beyond) -- measured, profiles/r5_tolerance_sweep.txt: at S = 577 (configs[3], sharp attention over 2.2 x
# the keys) five such blocks leave the logits at 1.0 - 1.4e-3, seven at 7e-4; at S = 257 five are enough
DEFAULT_PRECISE_ATTN_BLOCKS = (5, 7)
# THE TOLERANCE MODE: (image_precise_blocks, image_precise_attn_blocks) up to 288 tokens / beyond.  Round 6 put the
# claim on a distribution -- (weight seed, event seed) draws per BASELINE config (tests/config_cases.py), fp32 oracle logits shipped:
#   * round 5's (8, 5) / (8, 7) held 1e-3 on the ONE draw per config it was chosen on and on 6 of 8 draws of configs[2], [3], [4]
#     (worst 2.4e-3 / 1.05e-3 / 1.5e-3, profiles/r6_tolerance_sweep.txt).  With every block split but only five with fp32-class
#     attention the error stays at 1.0e-3 (tools/tolerance_model.py: the 16-bit q and k of the later blocks are the largest
#     remaining term), so the attention count had to grow with the block count;
#   * (12, 10) / (12, 12), picked on draws 0 .. 7, then failed on eight HELD-OUT draws of configs[4] (6 of 8, worst 1.2e-3,
#     profiles/r6_tolerance_sweep_held_out.txt): picking on the test set, as VERDICT r5 said;
#   * (16, 12) for both lengths, lo products as e4m3 (DEFAULT_LO_FP8): 159 of the 160 (config, draw) pairs measured are inside 1e-3
#     -- draws 0 .. 7 and the held-out draws 8 .. 15, each on fp32 weights and on weights rounded to 16 bit -- the worst of them
#     at 8.0e-4 (profiles/r6_parity_seeds*.txt).  The pair outside is configs[2] draw 5 on fp32 weights (1.3e-3): two classes, its
#     largest |logit| is 1.5 of a possible 100 -- a denominator 5 x smaller than the other draws', not a larger error; the same draw on
#     16-bit weights is inside (7.9e-4).
# Price on the bench config (profiles/r6_g_bench.json): 1.43 x the default step on a checkpoint stored in 16 bit, 1.77 x on
# fp32 weights; with 16-bit lo products 1.64 x / 2.09 x.  bench.py prices exactly these counts.
TOLERANCE_MODE = ((16, 12), (16, 12))
# ... with the lo products of those blocks as e4m3 operands (ec_vit_weights.lo_fp8, round 6): an e4m3 lo product costs 0.51 - 0.52 of
# the f16 one (~80 / ~125 ms of the mode's step on 16-bit / fp32 weights) and costs the mode's error + 4 % on average, + 17 % on
# configs[4] (profiles/r6_tolerance_sweep_fp8.txt; profiles/r6_parity_seeds*.txt measure the mode as shipped)
DEFAULT_LO_FP8 = True


def tolerance_mode_kwargs(arch_or_cfg):
    """CLIP(...) / ResNetCLIP(...) keyword arguments of the tolerance mode for an architecture name or config dict.

    ResNet towers: every Bottleneck (and the stem and the attention pool) on split-precision operands.  No smaller count
    has been chosen yet: that needs a sweep over tuning and held-out weight draws (tools/bench_resnet.py
    --precise-blocks prices and measures the counts), and a count picked on the tuning draws alone is what failed for the
    ViT mode above."""
    if isinstance(arch_or_cfg, str) and arch_or_cfg in RESNET_ARCHS:
        arch_or_cfg = resnet_config(arch_or_cfg)
    if not isinstance(arch_or_cfg, str) and _resnet.is_resnet_config(arch_or_cfg):
        return dict(precise_blocks=sum(arch_or_cfg['vision_layers']))
    cfg = arch_config(arch_or_cfg) if isinstance(arch_or_cfg, str) else arch_or_cfg
    tokens = (cfg['image_size'] // cfg['patch']) ** 2 + 1
    pb, pa = TOLERANCE_MODE[0 if tokens <= 288 else 1]
    if os.environ.get('EVENTCLIP_TOLERANCE_MODE'):       # 'B:A' (experiments: tools/sweep_tolerance.py, bench.py A / B lines)
        pb, pa = (int(v) for v in os.environ['EVENTCLIP_TOLERANCE_MODE'].split(':'))
    pb = min(pb, cfg['layers'] - 1)
    return dict(image_precise_blocks=pb, image_precise_attn_blocks=min(pa, pb))


class CLIP(ClipBase):
    """Frozen CLIP (ViT image tower + text tower) running on hand-written HIP kernels."""

    def __init__(self, cfg, state_dict, dtype='float16', chunk=2560, text_precise=True,
                 image_precise=False, full_last_block=None, low_latency=False, ln_folded=None, q_scaled=True,
                 image_precise_blocks=None, image_precise_attn_blocks=None, image_lo_fp8=None):
        super().__init__(cfg, state_dict, dtype, chunk)
        self.cfg['activation'] = _check_activation(self.cfg.get('activation') or 'quick_gelu')
        # split-precision (~fp32) arithmetic: on for the text tower (run once, cached by the
        # classifiers), off for the image tower (3x the GEMM work; validation only)
        self.text_precise, self.image_precise = bool(text_precise), bool(image_precise)
        # encode_image returns ln_post(x[:, 0]) @ proj: of the last block only the class-token rows are
        # read, so by default only those go through its attention query / out_proj / MLP (identical
        # features); True (or EVENTCLIP_FULL_LAST_BLOCK=1) computes every token like the reference
        if full_last_block is None:
            full_last_block = os.environ.get('EVENTCLIP_FULL_LAST_BLOCK', '0') not in ('', '0')
        self.full_last_block = bool(full_last_block)
        # serving a few frames at a time: under-filled GEMM launches run K-batched (about half the latency of a
        # single frame); a frame's features then differ from its large-batch ones in the last fp32 bits
        self.low_latency = bool(low_latency)
        # LayerNorm of the image tower's blocks folded into the GEMMs around it (include/eventclip_hip.h,
        # ec_vit_weights.ln_folded); EVENTCLIP_LN_FOLDED=0 runs the plain LayerNorm launches
        if ln_folded is None:
            ln_folded = os.environ.get('EVENTCLIP_LN_FOLDED', '1') not in ('', '0')
        self.ln_folded = bool(ln_folded)
        # softmax scale folded into the q rows of in_proj before their rounding (ec_vit_weights.q_scaled); False packs
        # the weights exactly as the training path holds them (plain q, plain LayerNorm with ln_folded=False too)
        self.q_scaled = bool(q_scaled)
        # split precision in the FIRST n blocks of the image tower only (ec_vit_weights.precise_blocks): an early
        # block's rounding error is carried through every later block, so a few such blocks buy most of what
        # image_precise buys (every config inside 1e-3 on input-dependent weights with n = 8) at a fraction of its price
        # (EVENTCLIP_PRECISE_BLOCKS=n sets it for models built without the argument, where the mode applies)
        if image_precise_blocks is None:
            image_precise_blocks = int(os.environ.get('EVENTCLIP_PRECISE_BLOCKS', '0') or 0)
            if image_precise_blocks and (not self.ln_folded or self.low_latency or image_precise_blocks >= cfg['layers']
                                         or self.compute_dtype != torch.float16 or self.image_precise):
                # (the explicit argument raises in _pack for the same conditions; the environment variable addresses
                # every model of the process, some of which the mode does not apply to -- say so)
                import warnings
                warnings.warn(f'EVENTCLIP_PRECISE_BLOCKS={image_precise_blocks} ignored for this model (needs ln_folded, '
                              f'float16, no low_latency / image_precise, and fewer than layers={cfg["layers"]} blocks)')
                image_precise_blocks = 0
        self.image_precise_blocks = 0 if self.image_precise else int(image_precise_blocks)
        # ... of which the first few also run attention in fp32 on hi + lo q, k, v (ec_vit_weights.precise_attn_blocks)
        if image_precise_attn_blocks is None:
            tokens = (cfg['image_size'] // cfg['patch']) ** 2 + 1
            image_precise_attn_blocks = int(os.environ.get('EVENTCLIP_PRECISE_ATTN_BLOCKS',
                                                           str(DEFAULT_PRECISE_ATTN_BLOCKS[0 if tokens <= 288 else 1])))
        self.image_precise_attn_blocks = max(0, min(int(image_precise_attn_blocks), self.image_precise_blocks))
        # the lo products of the split-operand blocks on the FP8 matrix path (ec_vit_weights.lo_fp8; EVENTCLIP_LO_FP8=0 / 1)
        if image_lo_fp8 is None:
            image_lo_fp8 = os.environ.get('EVENTCLIP_LO_FP8', str(int(DEFAULT_LO_FP8))) not in ('', '0')
        self.image_lo_fp8 = bool(image_lo_fp8) and self.image_precise_blocks > 0 and cfg['width'] % 128 == 0
        # bytes of tower scratch at most
        self.workspace_budget = 24 << 30

    # ---- device packing ----
    def _pack(self):
        if self._packed is not None:
            return self._packed
        dev = self._pack_device()
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        if any('.lora_' in k for k in sd):
            # an autograd-enabled FTCLIPClassifier injected LoRA modules into ``visual``: the inference copies hold the
            # effective weights base + up @ down under the plain names
            from .lora import merge_lora_visual
            vis = merge_lora_visual({k[len('visual.'):]: v for k, v in sd.items() if k.startswith('visual.')})
            sd = {k: v for k, v in sd.items() if not k.startswith('visual.')}
            sd.update({'visual.' + k: v for k, v in vis.items()})
        cd = self.compute_dtype
        pk = Packer(sd, dev, cd, self.cfg, keep_zero_lo=getattr(self, 'keep_zero_lo', False))
        dev32, dev16, dev16_pair = pk.dev32, pk.dev16, pk.dev16_pair
        c = self.cfg
        P, W = c['patch'], c['width']
        k, kpad, klo = patch_row_widths(P)
        cw = sd['visual.conv1.weight'].reshape(W, k).float().cpu()
        conv = torch.zeros(W, kpad)
        conv[:, :k] = cw
        conv[:, k:2 * k] = cw
        conv_lo = torch.zeros(W, klo)
        conv_lo[:, :k] = cw
        v = _lib.EcVitWeights()
        v.dtype, v.image_size, v.patch, v.width = pk.code, c['image_size'], P, W
        v.layers, v.heads, v.out_dim, v.kpad = c['layers'], W // 64, c['embed_dim'], kpad
        v.conv_w = dev16(conv)
        v.cls, v.pos = dev32(sd['visual.class_embedding']), dev32(sd['visual.positional_embedding'])
        v.ln_pre_g, v.ln_pre_b = dev32(sd['visual.ln_pre.weight']), dev32(sd['visual.ln_pre.bias'])
        v.ln_post_g, v.ln_post_b = (dev32(sd['visual.ln_post.weight']),
                                    dev32(sd['visual.ln_post.bias']))
        v.proj_w, v.proj_w_lo = dev16_pair(sd['visual.proj'].t(), null_if_exact=True)
        v.precise = int(self.image_precise)
        v.full_last_block = int(self.full_last_block)
        v.low_latency = int(self.low_latency)
        v.q_scaled = int(self.q_scaled and not self.image_precise)
        v.ln_folded = int(self.ln_folded and not self.image_precise)
        if self.image_precise_blocks:
            if not (0 < self.image_precise_blocks < c['layers']) or not v.ln_folded or self.low_latency or cd != torch.float16:
                raise ValueError(f'image_precise_blocks={self.image_precise_blocks} needs 0 < n < layers={c["layers"]}, '
                                 'ln_folded, float16 and no low_latency')
        v.precise_blocks = self.image_precise_blocks
        v.precise_attn_blocks = self.image_precise_attn_blocks
        v.lo_fp8 = int(self.image_lo_fp8)
        v.activation = _lib.activation_code(c.get('activation'))
        v.conv_w_lo = dev16_pair(conv_lo, null_if_exact=True)[1]
        vb = pk.blocks('visual.transformer', c['layers'], self.image_precise, q_scaled_all=bool(v.q_scaled),
                       ln_folded=bool(v.ln_folded), precise_first=self.image_precise_blocks, lo_fp8=self.image_lo_fp8)
        v.blocks = ctypes.cast(vb, ctypes.POINTER(_lib.EcBlockWeights))
        # (a mixed checkpoint -- some matrices exact, some not -- sets the flag and relies on the per-matrix NULL lo
        # pointers: the C side checks every pointer it is about to use, the flag only says that NULL is allowed)
        v.weights_exact16 = int(any(pk.exact))
        t, tb = pk.text(self.text_precise)
        self._packed = dict(vit=v, text=t, keep=pk.keep, vb=vb, tb=tb, kpad=kpad, code=pk.code, dev=dev)
        return self._packed

    @property
    def kpad(self):
        return self._pack()['kpad']

    @property
    def dtype_code(self):
        return self._pack()['code']

    # ---- towers ----
    @torch.no_grad()
    def encode_patches(self, patches, n_img=None):
        """patches: 16-bit CUDA tensor [N, G, kpad] (ec_preprocess / ec_patchify layout)."""
        from . import torch_ops
        self._pack()
        if n_img is not None and int(n_img) != int(patches.shape[0]):
            patches = patches[:int(n_img)]
        assert patches.dtype == self.compute_dtype and patches.is_contiguous()
        return torch.ops.eventclip_hip.vit_encode(patches, torch_ops.handle_of(self))

    def encode_image(self, image, differentiable=False):
        """image: float tensor [N, 3, R, R] as CLIP's preprocess produces -> fp32 [N, D].

        differentiable=True: the features stay attached to the autograd graph of ``image`` (saliency, adversarial probes, a
        learnable front end): they come from a frozen training-form tower (``ft.VisualTower``, built on first use, its
        operand copies re-packed when the weights were written) through ``eventclip_hip::vit_image_fwd``, whose backward
        is ``ec_vit_train_backward_image`` with no weight gradient asked for.  The parameters receive no gradient.  The
        training form is the plain chain (plain q, LayerNorm not folded into the GEMMs), so its features differ from the
        default call's in the last bits (below 1e-3 max-normalised in float16).  The split-precision tower has no training form.
        Costs: the cached tower holds its own 16-bit operand copies of the vision weights beside the serving ones (twice the
        memory), and building or re-packing it marks the serving copies stale, so the first default call after it re-packs
        them (the same bits).  ``.cuda()`` / ``.to()`` drop the cached tower; a graph built before stays valid -- it keeps
        the tower it ran through alive and differentiates the weights as they were."""
        if differentiable:
            return self._encode_image_differentiable(image)
        return self._encode_image(image)

    def _apply(self, fn, *a, **k):
        self._diff_tower = None          # built over the parameters where they were
        return super()._apply(fn, *a, **k)

    def _encode_image_differentiable(self, image):
        from . import ft, torch_ops
        c = self.cfg
        R = c['image_size']
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != R or image.shape[3] != R:
            raise ValueError(f'encode_image expects [N, 3, {R}, {R}], got {tuple(image.shape)}')
        t = getattr(self, '_diff_tower', None)
        if t is None:
            t = self._diff_tower = ft.VisualTower(self)     # refuses image_precise: no training form
        img = image.to(t.dev, torch.float32)
        # a frozen tower: parameters that require grad elsewhere go in detached
        params = [p.detach() for p in t.op_params()]
        return torch.ops.eventclip_hip.vit_image_fwd(img, params, torch_ops.handle_of(t))[0]

    @torch.no_grad()
    def _encode_image(self, image):
        pk = self._pack()
        c = self.cfg
        R, P = c['image_size'], c['patch']
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] != R or image.shape[3] != R:
            raise ValueError(f'encode_image expects [N, 3, {R}, {R}], got {tuple(image.shape)}')
        img = image.to(pk['dev'], torch.float32).contiguous()
        n = img.shape[0]
        patches = torch.empty((n, (R // P) ** 2, pk['kpad']), dtype=self.compute_dtype,
                              device=pk['dev'])
        _lib.launch('ec_patchify', img, n, R, P, pk['kpad'], patches, pk['code'])
        return self.encode_patches(patches)


def _refuse_resnet_gelu(activation):
    if activation not in (None, 'quick_gelu'):
        _check_activation(activation)
        raise NotImplementedError("the ResNet towers take no activation='gelu': their convolutions use ReLU and their text tower "
                                  'runs QuickGELU only')


def build_random(arch, seed=0, dtype='float16', device='cuda', chunk=2560, **override):
    """Random-weight CLIP of a named architecture (benchmarks / tests: no checkpoints ship).  activation='gelu' (or an
    open_clip name such as 'ViT-B-32') builds the exact-GELU network."""
    if override.get('activation', '') is None:
        override.pop('activation')
    if arch in RESNET_ARCHS:
        _refuse_resnet_gelu(override.pop('activation', None))
        mode = {k: override.pop(k) for k in ('precise_blocks', 'precise') if k in override}   # tolerance_mode_kwargs(arch)
        cfg = resnet_config(arch, **override)
        model = _resnet.ResNetCLIP(cfg, random_state_dict(cfg, seed), dtype=dtype, **mode)
    else:
        cfg = arch_config(arch, **override)
        model = CLIP(cfg, random_state_dict(cfg, seed), dtype=dtype, chunk=chunk)
    if device is not None:
        model = model.to(device)
    return model.eval()


def build_from_state_dict(sd, dtype='float16', device='cuda', chunk=2560, precise_blocks=0, activation=None):
    """precise_blocks: the split-precision form of a ResNet tower (tolerance_mode_kwargs); ViT checkpoints refuse it.
    activation: 'quick_gelu' or 'gelu' (ACTIVATIONS above); the state dict cannot say which, so None means QuickGELU."""
    sd = {k: v for k, v in sd.items() if k not in ('input_resolution', 'context_length',
                                                   'vocab_size')}
    cfg = config_from_state_dict(sd)
    if _resnet.is_resnet_config(cfg):
        _refuse_resnet_gelu(activation)
        model = _resnet.ResNetCLIP(cfg, sd, dtype=dtype, precise_blocks=precise_blocks)
    else:
        cfg['activation'] = _check_activation(activation or 'quick_gelu')
        if precise_blocks:
            raise ValueError('precise_blocks is the ResNet towers\' keyword; a ViT takes CLIP(cfg, sd, '
                             '**tolerance_mode_kwargs(cfg))')
        model = CLIP(cfg, sd, dtype=dtype, chunk=chunk)
    if device is not None:
        model = model.to(device)
    return model.eval()


# ------------------------------------------------------------------------------------------
# Hugging Face (transformers.CLIPModel) layout -> OpenAI's
# ------------------------------------------------------------------------------------------
_HF_LAYER = (('layer_norm1', 'ln_1'), ('layer_norm2', 'ln_2'), ('self_attn.out_proj', 'attn.out_proj'), ('mlp.fc1', 'mlp.c_fc'),
             ('mlp.fc2', 'mlp.c_proj'))
_HF_TOP = (('vision_model.embeddings.class_embedding', 'visual.class_embedding'),
           ('vision_model.embeddings.patch_embedding.weight', 'visual.conv1.weight'),
           ('vision_model.embeddings.position_embedding.weight', 'visual.positional_embedding'),
           ('vision_model.pre_layrnorm.weight', 'visual.ln_pre.weight'), ('vision_model.pre_layrnorm.bias', 'visual.ln_pre.bias'),
           ('vision_model.post_layernorm.weight', 'visual.ln_post.weight'), ('vision_model.post_layernorm.bias', 'visual.ln_post.bias'),
           ('text_model.embeddings.token_embedding.weight', 'token_embedding.weight'),
           ('text_model.embeddings.position_embedding.weight', 'positional_embedding'),
           ('text_model.final_layer_norm.weight', 'ln_final.weight'), ('text_model.final_layer_norm.bias', 'ln_final.bias'),
           ('logit_scale', 'logit_scale'))


def state_dict_from_hf(hf_sd):
    """transformers' CLIPModel state dict -> OpenAI's key layout: q / k / v_proj concatenated into
    attn.in_proj_*, layer_norm1 / 2 -> ln_1 / 2, mlp.fc1 / fc2 -> mlp.c_fc / c_proj, the two projection matrices transposed
    ([out, in] Linear weights -> [in, out] parameters), (transformers' spelling) pre_layrnorm -> ln_pre.  position_ids buffers
    are dropped; any other key that has no counterpart raises."""
    hf = {k: v for k, v in hf_sd.items() if not k.endswith('position_ids')}
    out, used = {}, set()

    def take(k):
        if k not in hf:
            raise KeyError(f'state_dict_from_hf: {k} is missing: not a transformers CLIPModel state dict')
        used.add(k)
        return hf[k]
    for src, dst in _HF_TOP:
        out[dst] = take(src)
    out['visual.proj'] = take('visual_projection.weight').t().contiguous()
    out['text_projection'] = take('text_projection.weight').t().contiguous()
    for tower, prefix in (('vision_model', 'visual.transformer'), ('text_model', 'transformer')):
        head = f'{tower}.encoder.layers.'
        layers = len({k[len(head):].split('.')[0] for k in hf if k.startswith(head)})
        for i in range(layers):
            s, d = f'{head}{i}.', f'{prefix}.resblocks.{i}.'
            for leaf in ('weight', 'bias'):
                out[f'{d}attn.in_proj_{leaf}'] = torch.cat([take(f'{s}self_attn.{p}_proj.{leaf}') for p in 'qkv'], 0)
                for a, b in _HF_LAYER:
                    out[f'{d}{b}.{leaf}'] = take(f'{s}{a}.{leaf}')
    extra = sorted(set(hf) - used)
    if extra:
        raise KeyError(f'state_dict_from_hf: no counterpart for {extra[:4]}{" ..." if len(extra) > 4 else ""}')
    return out


def _read_state_dict(path):
    """A checkpoint file -> state dict on the CPU: *.safetensors, a TorchScript archive, or a torch.save'd dict."""
    if path.endswith('.safetensors'):
        try:
            from safetensors.torch import load_file
        except ImportError as e:
            raise ImportError(f'{path}: reading *.safetensors needs the safetensors package, which is not installed; '
                              'convert the file to a torch.save\'d state dict, or install safetensors') from e
        return load_file(path, device='cpu')
    try:
        return torch.jit.load(path, map_location='cpu').state_dict()
    except RuntimeError:
        sd = torch.load(path, map_location='cpu')
        if isinstance(sd, dict) and 'state_dict' in sd:
            sd = sd['state_dict']
        return sd


_HF_ACT = {'gelu': 'gelu', 'quick_gelu': 'quick_gelu'}


def hf_activation(config):
    """A transformers CLIP config (the dict of config.json) -> 'gelu' / 'quick_gelu'; refuses any other hidden_act, towers
    that disagree, and attention heads that are not 64 wide."""
    acts = []
    for part in ('vision_config', 'text_config'):
        c = config.get(part) or {}
        act = c.get('hidden_act', 'quick_gelu')             # transformers' CLIP default
        if act not in _HF_ACT:
            raise NotImplementedError(f'{part}.hidden_act = {act!r}: the towers run {sorted(_HF_ACT)} only')
        acts.append(_HF_ACT[act])
        hidden, heads = c.get('hidden_size'), c.get('num_attention_heads')
        if hidden is not None and heads is not None and hidden != 64 * heads:
            raise NotImplementedError(f'{part}: head dimension {hidden} / {heads} = {hidden / heads:g}; the attention kernels '
                                      'are built for 64')
    if acts[0] != acts[1]:
        raise NotImplementedError(f'vision_config.hidden_act {acts[0]!r} and text_config.hidden_act {acts[1]!r} differ: a model '
                                  'has one activation here')
    return acts[0]


def _load_hf_directory(path, activation):
    import json
    with open(os.path.join(path, 'config.json')) as f:
        act = hf_activation(json.load(f))
    if activation is not None and _check_activation(activation) != act:
        raise ValueError(f"activation={activation!r} contradicts {os.path.join(path, 'config.json')} (hidden_act -> {act!r})")
    for leaf in ('model.safetensors', 'pytorch_model.bin'):
        if os.path.isfile(os.path.join(path, leaf)):
            return state_dict_from_hf(_read_state_dict(os.path.join(path, leaf))), act
    raise FileNotFoundError(f'{path}: neither model.safetensors nor pytorch_model.bin beside config.json')


def load(name, device='cuda', jit=False, download_root=None, dtype='float16', activation=None):
    """``clip.load`` of the reference (test.py:26) -> (model, preprocess).

    ``name`` is an architecture name whose checkpoint ``<name with / -> ->.pt`` sits in
    ``download_root`` (default ``~/.cache/clip``), or a path to a checkpoint (TorchScript
    archive, plain state dict in OpenAI's key layout -- open_clip's ``open_clip_pytorch_model.bin`` is one --
    or ``*.safetensors`` of the same), or a directory in Hugging Face layout (``config.json`` beside
    ``model.safetensors`` / ``pytorch_model.bin``).  Nothing is downloaded.

    ``activation``: 'quick_gelu' / 'gelu'.  A checkpoint FILE cannot say which network it holds, so None means
    QuickGELU (OpenAI's): pass 'gelu' for open_clip's models without a -quickgelu suffix.  An open_clip architecture
    name and an HF directory's config.json say it themselves (None takes their word; a contradiction raises)."""
    path = name
    if os.path.isdir(path) and os.path.isfile(os.path.join(path, 'config.json')):
        sd, activation = _load_hf_directory(path, activation)
    else:
        if not os.path.isfile(path):
            cfg = resnet_config(name) if name in RESNET_ARCHS else arch_config(name)   # raises for unknown names
            if name not in RESNET_ARCHS:
                implied = resolve_arch(name)[1]
                if activation is not None and implied is not None and _check_activation(activation) != implied:
                    raise ValueError(f'activation={activation!r} contradicts the architecture name {name!r} ({implied!r})')
                activation = activation or implied
            root = download_root or os.path.expanduser('~/.cache/clip')
            path = os.path.join(root, name.replace('/', '-') + '.pt')
            if not os.path.isfile(path):
                raise FileNotFoundError(
                    f'CLIP checkpoint {path} not found and this build never downloads; place the '
                    f'OpenAI checkpoint there or use eventclip_amd.clip.build_random({name!r}) '
                    f'(image {cfg["image_size"]}px) for synthetic weights')
        sd = _read_state_dict(path)
    model = build_from_state_dict(sd, dtype=dtype, device=device, activation=activation)
    return model, Preprocess(model.cfg['image_size'])


# ------------------------------------------------------------------------------------------
# tokenizer: byte-level BPE of OpenAI CLIP.  Needs the published vocabulary file
# bpe_simple_vocab_16e6.txt.gz, which does not ship here (no network); benchmarks use
# synthetic token ids instead (synthetic_tokens).
# ------------------------------------------------------------------------------------------
def _bytes_to_unicode():
    bs = list(range(ord('!'), ord('~') + 1)) + list(range(ord('¡'), ord('¬') + 1)) + \
        list(range(ord('®'), ord('ÿ') + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


class SimpleTokenizer:
    def __init__(self, bpe_path):
        import regex as re
        self.byte_encoder = _bytes_to_unicode()
        merges = gzip.open(bpe_path).read().decode('utf-8').split('\n')
        merges = [tuple(m.split()) for m in merges[1:49152 - 256 - 2 + 1]]
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + '</w>' for v in vocab]
        vocab += [''.join(m) for m in merges]
        vocab += ['<|startoftext|>', '<|endoftext|>']
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {'<|startoftext|>': '<|startoftext|>', '<|endoftext|>': '<|endoftext|>'}
        self.pat = re.compile(
            r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""",
            re.IGNORECASE)
        self._re = re

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + '</w>',)
        pairs = set(zip(word[:-1], word[1:]))
        if not pairs:
            return token + '</w>'
        while True:
            bigram = min(pairs, key=lambda p: self.bpe_ranks.get(p, float('inf')))
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            new, i = [], 0
            while i < len(word):
                try:
                    j = word.index(first, i)
                except ValueError:
                    new.extend(word[i:])
                    break
                new.extend(word[i:j])
                i = j
                if word[i] == first and i < len(word) - 1 and word[i + 1] == second:
                    new.append(first + second)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
            if len(word) == 1:
                break
            pairs = set(zip(word[:-1], word[1:]))
        out = ' '.join(word)
        self.cache[token] = out
        return out

    def encode(self, text):
        text = html.unescape(html.unescape(text)).strip()
        text = self._re.sub(r'\s+', ' ', text).strip().lower()
        ids = []
        for tok in self._re.findall(self.pat, text):
            tok = ''.join(self.byte_encoder[b] for b in tok.encode('utf-8'))
            ids.extend(self.encoder[t] for t in self.bpe(tok).split(' '))
        return ids


@lru_cache()
def _tokenizer():
    cands = [os.environ.get('EVENTCLIP_BPE_PATH', ''),
             os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bpe_simple_vocab_16e6.txt.gz'),
             os.path.expanduser('~/.cache/clip/bpe_simple_vocab_16e6.txt.gz')]
    for p in cands:
        if p and os.path.isfile(p):
            return SimpleTokenizer(p)
    raise FileNotFoundError(
        'clip.tokenize needs OpenAI CLIP\'s bpe_simple_vocab_16e6.txt.gz (set EVENTCLIP_BPE_PATH); '
        'it is not shipped and nothing is downloaded.  Pass token ids directly '
        '(clip_dict["class_tokens"]) or use synthetic_tokens() for benchmarks.')


def tokenize(texts, context_length=CONTEXT_LENGTH, truncate=False):
    """``clip.tokenize``: str or list of str -> IntTensor [n, context_length]."""
    if isinstance(texts, str):
        texts = [texts]
    tk = _tokenizer()
    sot, eot = tk.encoder['<|startoftext|>'], tk.encoder['<|endoftext|>']
    out = torch.zeros(len(texts), context_length, dtype=torch.int)
    for i, t in enumerate(texts):
        ids = [sot] + tk.encode(t) + [eot]
        if len(ids) > context_length:
            if not truncate:
                raise RuntimeError(f'Input {t} is too long for context length {context_length}')
            ids = ids[:context_length]
            ids[-1] = eot
        out[i, :len(ids)] = torch.tensor(ids)
    return out


def synthetic_tokens(n_classes, seed=0, context_length=CONTEXT_LENGTH):
    """Stand-in prompts: SOT, 4-8 random ids < 49406, EOT, zero padding."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_classes, context_length), dtype=np.int32)
    for i in range(n_classes):
        n = int(rng.integers(4, 9))
        out[i, 0] = 49406
        out[i, 1:1 + n] = rng.integers(1, 49406, size=n)
        out[i, 1 + n] = 49407
    return torch.from_numpy(out)
