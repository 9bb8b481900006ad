"""Feature adapters with the reference's API (models/adapter.py), forward on HIP.

``TransformerAdapter`` keeps its parameters in the same torch modules as the
reference (``in_proj``, ``transformer_encoder.layers.{i}.*``, ``out_proj``) so that
checkpoints written by the reference's trainer load key for key; those modules are
parameter holders only -- ``forward`` runs ``ec_adapter_forward`` (fp32, the fused inference kernel) in eval mode
or with grad disabled, and the differentiable ``eventclip_hip::adapter_train_fwd`` (``ec_adapter_train_forward`` /
``_backward``, with the encoder layers' dropout of 0.1) in train mode with grad enabled.  Both layouts of the encoder
layer are built, ``norm_first=True`` (pre-LN, the reference configs') and ``norm_first=False`` (post-LN): the state-dict
keys are the same, the C structs carry the layout as ``post_norm``.

The map from a parameter to its C struct field (``LAYER_PARAMS`` / ``PROJ_PARAMS``, ``adapter_param_names``,
``_adapter_struct``) lives here, next to the module whose ``named_parameters()`` order it restates; ``train`` and
``torch_ops`` import it from here, which is why this module reaches ``torch_ops`` only inside its methods.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib


class Adapter(nn.Module):
    """Base adapter: residual weight handling (adapter.py:5-32)."""

    def __init__(self, residual=True):
        super().__init__()
        assert isinstance(residual, (bool, float))
        if isinstance(residual, bool):
            residual = 0.5 if residual else 0.
        if isinstance(residual, float):
            assert 0. <= residual <= 1.
        self.residual = residual

    def residual_add(self, in_feats, new_feats):
        assert isinstance(self.residual, float)
        return in_feats * self.residual + new_feats * (1. - self.residual)

    def forward(self, *args, **kwargs):
        raise NotImplementedError

    @property
    def dtype(self):
        raise NotImplementedError

    # ---- fused entry used by FSCLIPClassifier.forward ----
    def forward_rows(self, feats, row_idx):
        """feats [Nv, C] (valid views, compact) + row_idx [B, T] -> [B, T, C]: the zero
        scatter of clip_cls.py:319-321 followed by ``forward``."""
        raise NotImplementedError


def _scatter(feats, row_idx):
    B, T = row_idx.shape
    full = torch.zeros((B, T, feats.shape[-1]), dtype=feats.dtype, device=feats.device)
    valid = row_idx >= 0
    full[valid] = feats[row_idx[valid].long()]
    return full, valid


def compact_row_idx(valid):
    """valid bool [B, T] -> int32 [B, T]: a valid view's rank among the valid views (its row in a compact [Nv, C]
    feature matrix), -1 on padded views."""
    flat = valid.reshape(-1)
    idx = torch.where(flat, torch.cumsum(flat.int(), 0) - 1, torch.full_like(flat, -1, dtype=torch.int64))
    return idx.to(torch.int32).reshape(valid.shape)


def dense_row_idx(valid):
    """valid bool [B, T] -> int32 [B, T]: a valid view's own position b * T + t (its row in the [B * T, C] matrix with
    zero rows on padded views), -1 on padded views."""
    B, T = valid.shape
    return torch.where(valid, torch.arange(B * T, device=valid.device).view(B, T),
                       torch.full((B, T), -1, device=valid.device)).to(torch.int32)


# The parameters of one encoder layer in ``named_parameters()`` order: (leaf under transformer_encoder.layers.{i}., field
# of EcAdapterTrainLayer, is it a matrix -- EcAdapterLayer, the inference struct, reads the transposed copy ``<field>_t``).
# The four projection tensors follow the layers: (leaf, field of EcAdapterTrainParams, matrix).
LAYER_PARAMS = (('self_attn.in_proj_weight', 'qkv_w', True), ('self_attn.in_proj_bias', 'qkv_b', False),
                ('self_attn.out_proj.weight', 'o_w', True), ('self_attn.out_proj.bias', 'o_b', False),
                ('linear1.weight', 'w1', True), ('linear1.bias', 'b1', False),
                ('linear2.weight', 'w2', True), ('linear2.bias', 'b2', False),
                ('norm1.weight', 'ln1_g', False), ('norm1.bias', 'ln1_b', False),
                ('norm2.weight', 'ln2_g', False), ('norm2.bias', 'ln2_b', False))
PROJ_PARAMS = (('in_proj.weight', 'in_w', True), ('in_proj.bias', 'in_b', False),
               ('out_proj.weight', 'out_w', True), ('out_proj.bias', 'out_b', False))


def adapter_param_names(layers):
    """``TransformerAdapter.named_parameters()`` order: the order of the ``params`` list of the two training ops."""
    return [f'transformer_encoder.layers.{i}.{leaf}' for i in range(layers) for leaf, _, _ in LAYER_PARAMS] + \
        [leaf for leaf, _, _ in PROJ_PARAMS]


def _adapter_struct(tensors, in_dim, d_model, heads, ffn_dim, layers, residual, post_norm=0):
    """EcAdapterTrainParams over ``tensors`` (fp32 CUDA tensors in ``adapter_param_names`` order; None -> NULL, a
    gradient the split backward skips) -> (struct, the layer array its ``blocks`` points to).  post_norm: 0 the pre-LN
    layer (norm_first=True), 1 the post-LN one."""
    tensors = iter(tensors)
    blocks = (_lib.EcAdapterTrainLayer * layers)()
    p = _lib.EcAdapterTrainParams()
    p.in_dim, p.d_model, p.heads, p.ffn_dim, p.layers, p.residual = in_dim, d_model, heads, ffn_dim, layers, float(residual)
    p.post_norm = int(post_norm)
    for dst, table in [(b, LAYER_PARAMS) for b in blocks] + [(p, PROJ_PARAMS)]:
        for _, field, _ in table:
            t = next(tensors)
            setattr(dst, field, None if t is None else t.data_ptr())
    p.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.EcAdapterTrainLayer))
    return p, blocks


class IdentityAdapter(Adapter):
    """Trivial adapter that does nothing (adapter.py:35-50)."""

    def __init__(self, *args, **kwargs):
        super().__init__(residual=False)
        self.dummy = nn.Parameter(torch.zeros(1), requires_grad=False)

    def forward(self, feats, valid_masks):
        return feats

    def forward_rows(self, feats, row_idx):
        return _scatter(feats, row_idx)[0]

    @property
    def dtype(self):
        return self.dummy.dtype


class TransformerAdapter(Adapter):
    """Order-invariant Transformer over the views of one sample (adapter.py:53-109)."""

    def __init__(self, in_dim, d_model=256, num_heads=4, ffn_dim=256 * 4, norm_first=True,
                 num_layers=2, residual=False):
        super().__init__(residual=residual)
        self.in_dim, self.d_model, self.num_heads = in_dim, d_model, num_heads
        self.norm_first = bool(norm_first)
        self.ffn_dim, self.num_layers = ffn_dim, num_layers
        enc_layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=num_heads,
                                               dim_feedforward=ffn_dim, norm_first=norm_first,
                                               batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer=enc_layer,
                                                         num_layers=num_layers,
                                                         enable_nested_tensor=False)
        self.in_proj = nn.Linear(in_dim, d_model)
        self.out_proj = nn.Linear(d_model, in_dim)
        self._packed = None

    TRAIN_DROPOUT = 0.1       # nn.TransformerEncoderLayer's default, what the reference trains with

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        return super().load_state_dict(*a, **k)

    def _param_key(self):
        """Changes when a parameter is updated in place (an optimiser step bumps ``_version``) or replaced."""
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _pack(self):
        key = self._param_key()
        if self._packed is not None and self._packed['key'] == key:
            return self._packed
        dev = _lib.require_gpu()
        if self.in_proj.weight.device.type != 'cuda':
            raise _lib.HipLibraryError('adapter weights are on the CPU: call .cuda() first')
        keep = []

        def d(t, transpose=False):
            t = t.detach().to(dev, torch.float32)
            t = (t.t() if transpose else t).contiguous()
            keep.append(t)
            return t.data_ptr()

        layers = (_lib.EcAdapterLayer * self.num_layers)()
        w = _lib.EcAdapterWeights()
        w.in_dim, w.d_model, w.heads, w.ffn = self.in_dim, self.d_model, self.num_heads, self.ffn_dim
        w.layers, w.residual, w.post_norm = self.num_layers, float(self.residual), int(not self.norm_first)
        for dst, mod, table in [(e, m, LAYER_PARAMS) for e, m in zip(layers, self.transformer_encoder.layers)] + \
                [(w, self, PROJ_PARAMS)]:
            for leaf, field, matrix in table:
                setattr(dst, field + ('_t' if matrix else ''), d(mod.get_parameter(leaf), matrix))
        w.layer = ctypes.cast(layers, ctypes.POINTER(_lib.EcAdapterLayer))
        self._packed = dict(w=w, layers=layers, keep=keep, key=key)
        return self._packed

    @torch.no_grad()
    def forward_rows(self, feats, row_idx):
        """The fused inference kernel, in every mode (FSCLIPClassifier's eval forward and the trainers' checks)."""
        from . import torch_ops
        self._pack()
        return torch.ops.eventclip_hip.adapter_fwd(feats.float().contiguous(), row_idx.contiguous(),
                                                    torch_ops.handle_of(self))

    def train_rows(self, rows, idx):
        """The differentiable forward: rows fp32 [B * T, C] with zero rows on padded views, idx int32 [B, T] (-1 =
        padded) -> [B, T, C], with autograd into every parameter that requires grad (and into ``rows``).  Dropout is
        ``TRAIN_DROPOUT`` while this module is in train mode, seeded once per call from torch's default generator
        (``torch.manual_seed`` reproduces a run), else 0: the deterministic eval-mode function."""
        from . import torch_ops  # noqa: F401  (registers eventclip_hip::adapter_train_fwd)
        names = [n for n, _ in self.named_parameters()]
        assert names == adapter_param_names(self.num_layers), names
        p = self.TRAIN_DROPOUT if self.training else 0.
        seed = int(torch.empty((), dtype=torch.int64).random_().item()) if p > 0. else 0
        out, _ = torch.ops.eventclip_hip.adapter_train_fwd(rows.contiguous(), idx.contiguous(), list(self.parameters()),
                                                           self.d_model, self.num_heads, self.ffn_dim, self.num_layers,
                                                           float(self.residual), p, seed, int(not self.norm_first))
        return out

    def forward(self, feats, valid_masks):
        """feats [B, T, C], valid_masks [B, T] (True = valid view), as adapter.py:82-105.
        Padded views must hold zeros, which is what the reference's classifier passes."""
        B, T, C = feats.shape
        idx = dense_row_idx(valid_masks)
        if self.training and torch.is_grad_enabled():
            return self.train_rows(feats.float().reshape(B * T, C), idx)
        return self.forward_rows(feats.reshape(B * T, C), idx)

    @property
    def dtype(self):
        return self.in_proj.weight.dtype
