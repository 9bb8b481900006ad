"""What ``clip.CLIP`` and ``resnet.ResNetCLIP`` share: the ``nn.Module`` shell around the packed weight structs (OpenAI's
state-dict key names, lazy packing, the workspace, ``encode_text`` / ``forward``) and the packing of transformer blocks
and of the text tower into ``ec_block_weights`` / ``ec_text_weights``."""
import ctypes

import torch
import torch.nn as nn

from . import _lib


def _block_keys(prefix, i):
    p = f'{prefix}.resblocks.{i}.'
    return [p + k for k in ('ln_1.weight', 'ln_1.bias', 'attn.in_proj_weight', 'attn.in_proj_bias',
                            'attn.out_proj.weight', 'attn.out_proj.bias', 'ln_2.weight',
                            'ln_2.bias', 'mlp.c_fc.weight', 'mlp.c_fc.bias', 'mlp.c_proj.weight',
                            'mlp.c_proj.bias')]


def patch_row_widths(patch):
    """-> (k, kpad, klo) of a patch size: the 3 p^2 values of a patch; the width of a patch row, which carries every pixel
    as hi + lo 16-bit parts [hi | lo | 0], and of conv1.weight packed against it as [w_hi | w_hi | 0]; the width of
    conv1.weight's lo part [w_lo | 0] (ec_vit_encode, patch_embed)."""
    k = 3 * patch * patch
    return k, (2 * k + 63) // 64 * 64, (k + 63) // 64 * 64


# log2(e) / sqrt(head dim 64): what ec_attention_scaled_q expects in the q columns (include/eventclip_hip.h)
ATTN_Q_SCALE = 0.125 * 1.4426950408889634


class _Holder(nn.Module):
    """Plain container so parameters appear under OpenAI's dotted key names."""


def _assign(root, key, tensor):
    parts = key.split('.')
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, _Holder())
        m = m._modules[p]
    m.register_parameter(parts[-1], nn.Parameter(tensor.clone().float(), requires_grad=False))


class Packer:
    """Device copies of a state dict's tensors as the weight structs want them; ``keep`` owns every tensor handed out."""

    def __init__(self, sd, dev, cd, cfg, keep=None, keep_zero_lo=False):
        self.sd, self.dev, self.cd, self.cfg = sd, dev, cd, cfg
        self.code = _lib.EC_F16 if cd == torch.float16 else _lib.EC_BF16
        self.keep = [] if keep is None else keep
        self.keep_zero_lo = keep_zero_lo      # (tests)
        self.exact = []     # per split-precision matrix packed with null_if_exact: is it its 16-bit value?

    def dev32(self, t):
        t = t.to(self.dev, torch.float32).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def dev16(self, t):
        t = t.to(self.dev, torch.float32).to(self.cd).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def dev16_pair(self, t, null_if_exact=False):
        # (hi, lo) = (round16(w), round16(w - hi)), the operands of a split-precision GEMM (ec_gemm_args.W_lo).  null_if_exact
        # (ec_vit_weights.weights_exact16): a matrix that IS its 16-bit value -- a checkpoint stored in 16 bit --
        # has no lo part: NULL, and the product with it is skipped
        t32 = t.to(self.dev, torch.float32)
        pair = torch.empty((2,) + tuple(t32.shape), dtype=self.cd, device=self.dev)
        pair[0] = t32.to(self.cd)
        pair[1] = (t32 - pair[0].float()).to(self.cd)
        self.keep.append(pair)
        if null_if_exact:
            is_exact = bool((pair[1] == 0).all()) and not self.keep_zero_lo
            self.exact.append(is_exact)
            if is_exact:
                return pair[0].data_ptr(), None
        return pair[0].data_ptr(), pair[1].data_ptr()

    def blocks(self, prefix, layers, precise_all, q_scaled_all=False, ln_folded=False, precise_first=0, lo_fp8=False):
        from . import ops
        sd, dev, cd, c, keep = self.sd, self.dev, self.cd, self.cfg, self.keep
        dev32, dev16, dev16_pair = self.dev32, self.dev16, self.dev16_pair
        arr = (_lib.EcBlockWeights * layers)()
        for i in range(layers):
            ks = _block_keys(prefix, i)
            b = arr[i]
            # precise_first (ec_vit_weights.precise_blocks): the first blocks are split-operand blocks -- PLAIN matrices
            # (no softmax scale, no LayerNorm gain folded in) with their lo parts; the rest as asked
            split_ops = i < precise_first and not precise_all
            precise = precise_all or split_ops
            q_scaled = q_scaled_all and not precise
            b.ln1_g, b.ln1_b = dev32(sd[ks[0]]), dev32(sd[ks[1]])
            wqkv, bqkv = sd[ks[2]], sd[ks[3]]
            if q_scaled:
                # ec_vit_weights.q_scaled: softmax temperature and base change folded into the q rows in
                # fp32, before the one rounding to 16 bit
                width = wqkv.shape[1]
                heads = c.get('heads', width // 64) if prefix.startswith('visual') else c.get('text_heads', width // 64)
                assert width == 64 * heads, \
                    'q_scaled folds log2(e) / sqrt(64) into in_proj: the attention kernels are built for head dim 64'
                wqkv, bqkv = wqkv.float().clone(), bqkv.float().clone()
                wqkv[:width] *= ATTN_Q_SCALE
                bqkv[:width] *= ATTN_Q_SCALE
            vis = prefix.startswith('visual')
            b.qkv_b = dev32(bqkv)
            b.out_b = dev32(sd[ks[5]])
            b.ln2_g, b.ln2_b = dev32(sd[ks[6]]), dev32(sd[ks[7]])
            b.fc1_b, b.fc2_b = dev32(sd[ks[9]]), dev32(sd[ks[11]])
            if precise:     # plain matrices with their lo parts (NULL where the matrix is its 16-bit value)
                b.qkv_w, b.qkv_w_lo = dev16_pair(wqkv, vis)
                b.out_w, b.out_w_lo = dev16_pair(sd[ks[4]], vis)
                b.fc1_w, b.fc1_w_lo = dev16_pair(sd[ks[8]], vis)
                b.fc2_w, b.fc2_w_lo = dev16_pair(sd[ks[10]], vis)
                if split_ops and lo_fp8:
                    # e4m3 copies of the 16-bit matrices and of the lo parts that exist (ec_block_weights.*_w8 / *_wlo8)
                    def f8(t32, lo):
                        hi = t32.to(dev, torch.float32).to(cd)
                        src = (t32.to(dev, torch.float32) - hi.float()).to(cd).float() if lo else hi.float()
                        q, e = ops.quantize_e4m3(src)
                        keep.append(q)
                        return q.data_ptr(), e
                    b.qkv_w8, b.qkv_w8_exp = f8(wqkv, False)
                    b.fc1_w8, b.fc1_w8_exp = f8(sd[ks[8]], False)
                    b.fc2_w8, b.fc2_w8_exp = f8(sd[ks[10]], False)
                    if b.qkv_w_lo:
                        b.qkv_wlo8, b.qkv_wlo8_exp = f8(wqkv, True)
                    if b.fc1_w_lo:
                        b.fc1_wlo8, b.fc1_wlo8_exp = f8(sd[ks[8]], True)
                continue
            b.qkv_w = dev16(wqkv)
            b.out_w, b.fc1_w, b.fc2_w = dev16(sd[ks[4]]), dev16(sd[ks[8]]), dev16(sd[ks[10]])
            if ln_folded:
                # ec_vit_weights.ln_folded: W' = W diag(gamma) rounded once, its row sums AS ROUNDED, b + W beta
                def fold(wt, bias, gamma, beta):
                    wt, bias = wt.float().to(dev), bias.float().to(dev)
                    wp = (wt * gamma.float().to(dev)[None, :]).to(cd).contiguous()
                    keep.append(wp)
                    cs = wp.float().sum(1).contiguous()
                    bf = (bias + wt @ beta.float().to(dev)).contiguous()
                    keep.extend([cs, bf])
                    return wp.data_ptr(), cs.data_ptr(), bf.data_ptr()
                b.qkv_w_ln, b.qkv_cs, b.qkv_bf = fold(wqkv, bqkv, sd[ks[0]], sd[ks[1]])
                b.fc1_w_ln, b.fc1_cs, b.fc1_bf = fold(sd[ks[8]], sd[ks[9]], sd[ks[6]], sd[ks[7]])
        return arr

    def text(self, precise):
        """-> (ec_text_weights, its ec_block_weights array); precise: every matrix as hi + lo parts (the split-precision tower)."""
        sd, c, dev32 = self.sd, self.cfg, self.dev32
        t = _lib.EcTextWeights()
        t.dtype, t.ctx, t.vocab, t.width = self.code, c['context_length'], c['vocab_size'], c['text_width']
        t.layers, t.heads, t.out_dim = c['text_layers'], c['text_heads'], c['embed_dim']
        t.token_embedding = dev32(sd['token_embedding.weight'])
        t.pos = dev32(sd['positional_embedding'])
        t.ln_final_g, t.ln_final_b = dev32(sd['ln_final.weight']), dev32(sd['ln_final.bias'])
        t.proj_w, proj_lo = self.dev16_pair(sd['text_projection'].t())
        t.precise = int(precise)
        t.activation = _lib.activation_code(c.get('activation'))
        if precise:
            t.proj_w_lo = proj_lo
        tb = self.blocks('transformer', c['text_layers'], precise)
        t.blocks = ctypes.cast(tb, ctypes.POINTER(_lib.EcBlockWeights))
        return t, tb


class ClipBase(nn.Module):
    """Frozen CLIP with fp32 master parameters under OpenAI's key names; the towers' 16-bit copies are packed once per
    device (``_pack``, by the subclass) and dropped when the parameters move or change."""

    def __init__(self, cfg, state_dict, dtype, chunk):
        super().__init__()
        self.cfg = dict(cfg)
        for k, v in state_dict.items():
            if k not in ('input_resolution', 'context_length', 'vocab_size'):
                _assign(self, k, v)
        self.visual.output_dim = cfg['embed_dim']
        self.visual.input_resolution = cfg['image_size']
        self.compute_dtype = {'float16': torch.float16, 'fp16': torch.float16,
                              'bfloat16': torch.bfloat16, 'bf16': torch.bfloat16}[str(dtype)]
        self.chunk = int(chunk)        # images per pass through the tower (bounds the activation workspace)
        self._packed = None
        self._ws = _lib.Scratch()      # the towers' activation workspace

    # ---- protocol bits the reference's classifiers read ----
    @property
    def dtype(self):
        return self.logit_scale.dtype

    @property
    def device(self):
        return self.logit_scale.device

    def _apply(self, fn, *a, **k):
        self._packed = None          # .cuda() / .to(): repack lazily
        self._ws.buf = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, sd, strict=True):
        self._packed = None
        return super().load_state_dict(sd, strict=strict)

    def _pack_device(self):
        dev = _lib.require_gpu()
        if self.logit_scale.device.type != 'cuda':
            raise _lib.HipLibraryError('CLIP weights are on the CPU: call model.cuda() first '
                                       '(there is no CPU fallback)')
        return dev

    @torch.no_grad()
    def encode_text(self, text):
        """text: int tensor [K, 77] of BPE ids -> fp32 [K, D] (not normalised)."""
        pk = self._pack()
        if text.dim() != 2 or text.shape[1] != self.cfg['context_length']:
            raise ValueError(f'encode_text expects [K, {self.cfg["context_length"]}]')
        from . import torch_ops
        tok = text.to(pk['dev'], torch.int32).contiguous()
        return torch.ops.eventclip_hip.text_encode(tok, torch_ops.handle_of(self))

    def forward(self, image, text):
        """Cosine-similarity logits, as OpenAI's CLIP.forward."""
        i = self.encode_image(image)
        t = self.encode_text(text)
        i = i / i.norm(dim=1, keepdim=True)
        t = t / t.norm(dim=1, keepdim=True)
        li = self.logit_scale.exp() * i @ t.t()
        return li, li.t()
