"""``FTCLIPClassifier`` of the reference (models/clip_cls_ft.py): serving fine-tuned checkpoints, and the model
side of fine-tuning (the optimisation step itself is ``eventclip_amd.ft.FTTrainer``).

The reference fine-tunes CLIP's vision tower (all of it, sub-sets, or LoRA factors injected into
every attention block, clip_cls_ft.py:44-80, lora.py:384-403) and saves ``model.visual.*`` next to
``text_feats`` / ``adapter.*`` (clip_cls_ft.py:313-321).  Its forward (:196-243) is the few-shot forward
with the identity adapter: encode the valid views, L2-normalise, logits against the (learned) text
features, aggregate.  This class is that forward on the HIP path plus the checkpoint format:
``load_state_dict`` takes a reference checkpoint as it is -- LoRA-injected keys included, folded into
plain weights once (eventclip_amd.lora) -- and repacks the tower; ``state_dict`` emits the reference's
key set.  With an ``FTTrainer`` attached the classifier is in the middle of a fine-tuning run: ``forward``
then encodes through the trainer's (LoRA-merged) operand copies and ``state_dict`` writes the trainer's
``model.visual.*`` entries, LoRA factors under the reference's key names included.

``clip_dict['autograd'] = True`` makes the classifier what the reference's constructor makes it (clip_cls_ft.py:44-80):
the parameters of ``model.visual`` the flags select require grad, LoRA factors are injected as ``nn.Parameter``s under
the reference's module names, and ``forward`` in train mode builds an autograd graph over
``eventclip_hip::vit_train_fwd`` / ``::classify``, so the reference's loop (``loss.backward()``, any torch optimiser,
``torch.amp.GradScaler``, ``DistributedDataParallel``) trains it.  ``FTTrainer`` stays the fast path.
"""
import torch
import torch.nn as nn

from . import ft
from . import lora as elora
from .clip_base import _Holder
from .clip_cls import FSCLIPClassifier

FT_ADAPTER_DEFAULTS = dict(adapter_type='text-identity', residual=True)
FT_LOSS_DEFAULTS = dict(use_logits_loss=True, use_probs_loss=False)


def inject_lora_modules(visual, spec):
    """The module surgery of ``inject_trainable_lora`` (lora.py:384-403) on this package's ``visual`` (plain holders
    of parameters under OpenAI's names): in every block ``attn.in_proj_weight`` becomes a module holding the base
    weight as ``merged_proj`` and the factors ``lora_down_q`` / ``lora_up_q`` / ``_v`` (/ ``_k``), and with 'o' in the
    spec ``attn.out_proj`` holds ``linear.weight`` / ``linear.bias`` and ``lora_down.weight`` / ``lora_up.weight``.  The
    base tensors stay the same ``Parameter`` objects, frozen; the factors are new trainable ones on the base's device,
    initialised as lora.py:8-11.  Needs no device."""
    r, lora_k, lora_o = ft.parse_lora(spec)

    def factor(down, like):
        W = like.shape[1]
        t = torch.randn(r, W) / r if down else torch.zeros(W, r)
        return nn.Parameter(t.to(like.device), requires_grad=True)
    for blk in visual.transformer.resblocks.children():
        attn = blk.attn
        if 'in_proj_weight' not in attn._parameters:
            raise ValueError('this CLIP model already carries injected LoRA modules: build a fresh one')
        base = attn._parameters.pop('in_proj_weight')
        base.requires_grad_(False)
        h = _Holder()
        attn.add_module('in_proj_weight', h)
        h.register_parameter('merged_proj', base)
        for nm in ('q', 'v') + (('k',) if lora_k else ()):
            h.register_parameter('lora_down_' + nm, factor(True, base))
            h.register_parameter('lora_up_' + nm, factor(False, base))
        if lora_o:
            op = attn.out_proj
            w, b = op._parameters.pop('weight'), op._parameters.pop('bias')
            w.requires_grad_(False)
            lin, down, up = _Holder(), _Holder(), _Holder()
            lin.register_parameter('weight', w)
            lin.register_parameter('bias', b)
            down.register_parameter('weight', factor(True, w))
            up.register_parameter('weight', factor(False, w))
            op.add_module('linear', lin)
            op.add_module('lora_down', down)
            op.add_module('lora_up', up)


class FTCLIPClassifier(FSCLIPClassifier):
    """Fine-tuned CLIP for few-shot classification (clip_cls_ft.py:15-333).

    By default ``forward`` is the inference path in every mode, train mode with grad enabled included: it builds no
    autograd graph, and the vision tower trains through ``eventclip_amd.ft.FTTrainer``.  With
    ``clip_dict['autograd'] = True`` (``enable_autograd``) ``forward`` in train mode with grad enabled is differentiable
    into the tower's trainable parameters, the LoRA factors and ``text_feats``."""

    _differentiable = False

    def __init__(self, adapter_dict=None, clip_dict=None, loss_dict=None):
        ad = dict(FT_ADAPTER_DEFAULTS if adapter_dict is None else adapter_dict)
        kind = ad['adapter_type'].lower()
        if (kind[len('text-'):] if kind.startswith('text-') else kind) != 'identity':
            raise AssertionError('FTCLIPClassifier only supports the identity adapter (clip_cls_ft.py:119)')
        super().__init__(adapter_dict=ad, clip_dict=clip_dict,
                         loss_dict=dict(FT_LOSS_DEFAULTS) if loss_dict is None else loss_dict)
        # which parts of the tower were trained (lora / only_conv1 / only_bias / ..., clip_cls_ft.py:50-80)
        # is a property of the checkpoint being served; kept for API parity
        self.lora = self.clip_dict.get('lora', -1)
        self._tower = None        # eventclip_amd.ft.VisualTower while an FTTrainer is attached, or the autograd one
        self._trainer = None
        self.autograd = False
        if self.clip_dict.get('autograd', False):
            self.enable_autograd()

    # ---- training under torch autograd ----
    def enable_autograd(self):
        """What the reference's ``_build_clip`` does to ``model.visual`` (clip_cls_ft.py:50-80): ``requires_grad`` by
        the flags of ``clip_dict`` (``ft.trainable_visual``), LoRA modules injected.  Needs no device."""
        if self._trainer is not None:
            raise ValueError("an FTTrainer is attached: it owns the tower's operand copies, and the autograd path "
                             'would be their second owner')
        if self.autograd:
            return
        cd, visual = self.clip_dict, self.model.visual
        names = [n for n, _ in visual.named_parameters()]
        if any(ft.plain_visual_name(n) != n for n in names):
            raise ValueError('this CLIP model already carries injected LoRA modules: build a fresh one')
        train = set(ft.trainable_visual(names, cd))
        for n, p in visual.named_parameters():
            p.requires_grad_(n in train)
        if ft.parse_lora(cd.get('lora', -1)) is not None:
            inject_lora_modules(visual, cd['lora'])
        self.model._packed = None
        self.autograd = self._differentiable = True

    def _apply(self, fn, *args, **kwargs):
        if getattr(self, 'autograd', False):
            self._tower = None          # rebuilt over the parameters where ``fn`` leaves them
        return super()._apply(fn, *args, **kwargs)

    def _operand_tower(self):
        """The tower whose operand copies ``forward`` encodes through: an attached trainer's, the autograd path's own
        (built on first use, brought up to date with its parameters), or None for plain serving."""
        if not self.autograd:
            return self._tower
        if self._tower is None:
            t = ft.VisualTower(self.model)
            spec = self.clip_dict.get('lora', -1)
            if ft.parse_lora(spec) is not None:
                factors = {n: p for n, p in self.model.visual.named_parameters() if ft.plain_visual_name(n) is None}
                ft.LoraFactors(t, spec, params=factors).bind()
            self._tower = t
        self._tower.refresh()
        return self._tower

    def _forward_train(self, data_dict):
        """clip_cls_ft.py:196-243 with autograd: the valid views as patch rows under ``no_grad`` (``ec_patchify``), the
        tower through ``vit_train_fwd`` with its trainable tensors as inputs, ``text_feats = F.normalize(parameter)``
        in torch, then ``classify`` with the live text (its ``row_idx`` is the identity adapter's zero scatter).
        When ``data_dict['img']`` requires grad the valid views go through ``vit_image_fwd`` as fp32 images instead, and
        ``loss.backward()`` fills ``img.grad`` (padded views: exact zeros, the gradient of the indexing)."""
        if not self.autograd:
            return super()._forward_train(data_dict)
        from . import torch_ops
        t = self._operand_tower()
        params = t.op_params()
        img = data_dict.get('img')
        if 'patches' not in data_dict and torch.is_tensor(img) and img.requires_grad:
            valid_masks = data_dict['valid_mask'].to(t.dev)
            row_idx = ft.compact_row_idx(valid_masks)
            x = img[valid_masks.to(img.device)].to(t.dev, torch.float32)
            feats, _ = torch.ops.eventclip_hip.vit_image_fwd(x, params, torch_ops.handle_of(t))
        else:
            with torch.no_grad():
                patches, valid_masks, row_idx = ft.valid_patches(t, data_dict)
            feats, _ = torch.ops.eventclip_hip.vit_train_fwd(patches, params, torch_ops.handle_of(t))
        text_t = self.get_text_feats().float().t().contiguous()          # [C, K], differentiable under prompt tuning
        full_logits, logits, probs = self._classify(feats, row_idx.to(torch.int32).contiguous(), normalize=True,
                                                    text_t=text_t)
        return dict(full_logits=full_logits, valid_masks=valid_masks, logits=logits, probs=probs)

    def _view_feats(self, data_dict):
        t = self._operand_tower()
        if t is None or 'patches' not in data_dict:
            return super()._view_feats(data_dict)
        feats = t.encode_patches(data_dict['patches'])
        return feats.float().contiguous(), data_dict['row_idx'].contiguous(), data_dict['valid_mask']

    def get_img_feats(self, imgs):
        t = self._operand_tower()
        if t is None:
            return super().get_img_feats(imgs)
        return self._adjust_dtype(t.encode_patches(t.patchify(imgs)))

    # ---- checkpoints: model.visual.* travels with the classifier (clip_cls_ft.py:313-333) ----
    def state_dict(self, *args, **kwargs):
        if self.autograd:       # the module tree carries the reference's names: everything but the frozen rest of CLIP
            w = nn.Module.state_dict(self, *args, **kwargs)
            return {k: v for k, v in w.items() if k.startswith('model.visual.') or not k.startswith('model.')}
        w = super(FSCLIPClassifier, self).state_dict(*args, **kwargs)    # the ZS filter drops model.*
        if self._trainer is not None:
            vis = {k: v.detach() for k, v in self._trainer.visual_state_dict().items()}
        else:
            vis = {'model.visual.' + k: v for k, v in self.model.visual.state_dict().items()}
        return {**vis, **w}

    def load_state_dict(self, state_dict, strict=True):
        if self.autograd:
            # in place into the masters and the factors (the resume flow): the next forward sees their contents
            # changed, re-merges and repacks
            own = self.state_dict()
            sd = {k: v for k, v in state_dict.items() if k.startswith('model.visual.') or not k.startswith('model.')}
            odd = sorted(set(own) ^ set(sd))
            if odd and strict:
                raise KeyError(f'checkpoint and classifier disagree on {odd[:3]} ...')
            with torch.no_grad():
                for k in own.keys() & sd.keys():
                    own[k].copy_(torch.as_tensor(sd[k]).to(own[k].device, own[k].dtype))
            self._text_t = None
            return nn.modules.module._IncompatibleKeys([k for k in own if k not in sd], [k for k in sd if k not in own])
        sd = dict(state_dict)
        vis = {k[len('model.visual.'):]: v for k, v in sd.items() if k.startswith('model.visual.')}
        rest = {k: v for k, v in sd.items() if not k.startswith('model.')}
        if vis and self._trainer is not None:
            # the resume flow (nerv builds the optimiser first, then loads the checkpoint): the weights go INTO the
            # trainer -- masters in place, LoRA factors as factors (not folded into an already-merged base) --
            # and its 16-bit operand copies are rebuilt
            self._trainer.load_visual_state_dict(vis, strict=strict)
        elif vis:
            merged = elora.merge_lora_visual(vis)        # plain checkpoints pass through unchanged
            clip_sd = self.model.state_dict()
            new = {k: v for k, v in clip_sd.items() if not k.startswith('visual.')}
            missing = [k for k in clip_sd if k.startswith('visual.') and k[len('visual.'):] not in merged]
            if missing and strict:
                raise KeyError(f'fine-tuned checkpoint lacks {missing[:3]} ...')
            for k, v in clip_sd.items():
                if k.startswith('visual.'):
                    new[k] = torch.as_tensor(merged.get(k[len('visual.'):], v)).to(v.dtype)
            self.model.load_state_dict(new, strict=strict)               # repacks the 16-bit copies lazily
        elif strict:
            raise KeyError('no model.visual.* entries: not an FTCLIPClassifier checkpoint')
        return super().load_state_dict(rest, strict=strict)

    def train(self, mode=True):
        """clip_cls_ft.py:300-306: CLIP stays in eval mode except for its vision tower -- which has no
        train-mode behaviour of its own (no dropout, no batch statistics)."""
        return super().train(mode)
