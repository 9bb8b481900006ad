"""The exact GELU (csrc/activation.h, cfg['activation'] = 'gelu') without a GPU: the restated device formula against float64,
the float64 yardstick of the GPU tests (the project's oracle with its activation swapped) against torch.nn.GELU modules and
against Hugging Face's CLIP, planted faults that the checks of tests/test_gelu_gpu.py must reject, and the names, loaders
and refusals of the Python seam."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gelu_ref as ref  # noqa: E402
import gemm_ref as gr  # noqa: E402
import rowops_ref as rr  # noqa: E402

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TINY = dict(image_size=32, patch=16, width=64, layers=2, embed_dim=32, text_width=64, text_heads=1, text_layers=2,
            context_length=8, vocab_size=64)


@pytest.fixture
def swapped(monkeypatch):
    """oracle.clip_ref with x Phi(x) in place of QuickGELU: _blocks calls the module-level name."""
    from oracle import clip_ref
    monkeypatch.setattr(clip_ref, 'quick_gelu', ref.exact_gelu)
    return clip_ref


# ---------------------------------------------------------------------------------------------------------------
# the formula
# ---------------------------------------------------------------------------------------------------------------
def test_restated_formula_meets_both_conditions_on_the_grid():
    """|gelu_erf(x) - x Phi(x)| <= 2^-21 |x| and |gelu_erf_grad(x) - (Phi + x phi)| <= 2^-20 over 2 M points on [-12, 12] and
    every finite fp16 value up to 64 (measured here: 2.9e-7 |x| and 2.8e-7)."""
    rel, grad = ref.formula_errors(ref.grid())
    print(f'\nforward {rel:.3e} |x| (bound {ref.FWD_REL:.3e}), gradient {grad:.3e} (bound {ref.GRAD_ABS:.3e})')
    assert rel <= ref.FWD_REL and grad <= ref.GRAD_ABS


def test_restated_formula_is_finite_everywhere_and_maps_zero_to_zero():
    """Every finite fp16 and bf16 value, 2 M random fp32 bit patterns, the largest and smallest fp32 values, the values around
    which x^2 and GELU_P |x| overflow: finite results, no invalid operation on the way (np.errstate raises), zero -> zero
    (of the same sign), positive overflow side = x itself, negative = -0."""
    h = np.arange(65536, dtype=np.uint16)
    bits = np.random.default_rng(0).integers(0, 2 ** 32, size=2_000_000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([3.4028235e38, -3.4028235e38, 1.8446743e19, 1.8446745e19, -1.8446745e19, 1e38, -1e38, 1e-45, -1e-45,
                     1.1754944e-38, 13.0, -13.0, 14.5, -14.5, 88.0, -88.0], dtype=np.float32)
    x = np.concatenate([h.view(np.float16).astype(np.float32), (h.astype(np.uint32) << 16).view(np.float32),
                        bits.view(np.float32), edge])
    x = x[np.isfinite(x)]
    y, g = ref.gelu32(x), ref.grad32(x)
    assert np.isfinite(y).all() and np.isfinite(g).all()
    z = ref.gelu32(np.array([0.0, -0.0], dtype=np.float32))
    assert (z == 0).all() and not np.signbit(z[0]) and np.signbit(z[1])
    big = np.abs(x) > 14.5
    assert (y[big & (x > 0)] == x[big & (x > 0)]).all() and (y[big & (x < 0)] == 0).all()
    assert (g[big & (x > 0)] == 1).all() and (np.abs(g[big & (x < 0)]) <= 2.0 ** -100).all()
    assert (g >= -0.13).all() and (g <= 1.13).all()            # the slope constant of the bounds


def test_negative_tail_is_computed_without_cancellation():
    x = torch.linspace(ref.TAIL_LO, -1e-3, 100001)
    ref.tail_check(torch.from_numpy(ref.gelu32(x.numpy())).double(), x, 0.0, 'restatement')


# ---------------------------------------------------------------------------------------------------------------
# the float64 yardstick
# ---------------------------------------------------------------------------------------------------------------
class _Block(torch.nn.Module):
    def __init__(self, W, heads):
        super().__init__()
        self.ln_1, self.ln_2 = torch.nn.LayerNorm(W), torch.nn.LayerNorm(W)
        self.attn = torch.nn.MultiheadAttention(W, heads, batch_first=True)
        self.c_fc, self.gelu, self.c_proj = torch.nn.Linear(W, 4 * W), torch.nn.GELU(), torch.nn.Linear(4 * W, W)

    def forward(self, x):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False)[0]
        return x + self.c_proj(self.gelu(self.c_fc(self.ln_2(x))))


def test_swapped_oracle_equals_torch_gelu_modules_in_float64(swapped):
    """A 2-layer vision tower of torch modules (nn.LayerNorm, nn.MultiheadAttention, nn.Linear, nn.GELU()) in float64 with
    the oracle's weights against oracle.clip_ref.encode_image_autograd with its activation swapped, and its gradient."""
    from eventclip_amd import clip as eclip
    cfg = TINY
    sd = {k: v.double() for k, v in eclip.random_state_dict(cfg, seed=5).items()}
    W, P = cfg['width'], cfg['patch']
    blocks = [_Block(W, W // 64).double() for _ in range(cfg['layers'])]
    for i, b in enumerate(blocks):
        p = f'visual.transformer.resblocks.{i}.'
        b.load_state_dict({'ln_1.weight': sd[p + 'ln_1.weight'], 'ln_1.bias': sd[p + 'ln_1.bias'],
                           'ln_2.weight': sd[p + 'ln_2.weight'], 'ln_2.bias': sd[p + 'ln_2.bias'],
                           'attn.in_proj_weight': sd[p + 'attn.in_proj_weight'], 'attn.in_proj_bias': sd[p + 'attn.in_proj_bias'],
                           'attn.out_proj.weight': sd[p + 'attn.out_proj.weight'], 'attn.out_proj.bias': sd[p + 'attn.out_proj.bias'],
                           'c_fc.weight': sd[p + 'mlp.c_fc.weight'], 'c_fc.bias': sd[p + 'mlp.c_fc.bias'],
                           'c_proj.weight': sd[p + 'mlp.c_proj.weight'], 'c_proj.bias': sd[p + 'mlp.c_proj.bias']})
    img = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(1)).double().requires_grad_()
    F = torch.nn.functional
    x = F.conv2d(img, sd['visual.conv1.weight'], stride=P).reshape(3, W, -1).permute(0, 2, 1)
    x = torch.cat([sd['visual.class_embedding'].expand(3, 1, W), x], 1) + sd['visual.positional_embedding']
    x = F.layer_norm(x, (W,), sd['visual.ln_pre.weight'], sd['visual.ln_pre.bias'], 1e-5)
    for b in blocks:
        x = b(x)
    want = F.layer_norm(x[:, 0], (W,), sd['visual.ln_post.weight'], sd['visual.ln_post.bias'], 1e-5) @ sd['visual.proj']
    gw, = torch.autograd.grad(want.square().sum(), img)
    img2 = img.detach().clone().requires_grad_()
    got = swapped.encode_image_autograd(sd, cfg, img2)
    assert got.dtype == torch.float64
    gg, = torch.autograd.grad(got.square().sum(), img2)
    assert float((got - want).detach().abs().max()) <= 1e-12 * float(want.detach().abs().max())
    assert float((gg - gw).abs().max()) <= 1e-11 * float(gw.abs().max())


def test_swap_changes_the_features(monkeypatch):
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    sd = eclip.random_state_dict(TINY, seed=5)
    img = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    quick = clip_ref.encode_image(sd, TINY, img)
    monkeypatch.setattr(clip_ref, 'quick_gelu', ref.exact_gelu)
    exact = clip_ref.encode_image(sd, TINY, img)
    assert ref.rel_err(exact, quick) > 1e-3


@pytest.mark.parametrize('act', ['gelu', 'quick_gelu'])
def test_hf_clip_agrees_with_the_oracle_through_state_dict_from_hf(act, monkeypatch):
    """A tiny random transformers.CLIPModel with hidden_act = act against the oracle on state_dict_from_hf of its weights:
    1e-5 in fp32, both towers."""
    transformers = pytest.importorskip('transformers')
    from eventclip_amd import clip as eclip
    from oracle import clip_ref
    torch.manual_seed(3)
    vc = dict(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1, image_size=32, patch_size=16,
              hidden_act=act, projection_dim=32)
    tc = dict(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=8,
              vocab_size=64, hidden_act=act, projection_dim=32, eos_token_id=63, bos_token_id=62, pad_token_id=0)
    config = transformers.CLIPConfig(vision_config=vc, text_config=tc, projection_dim=32)
    model = transformers.CLIPModel(config).eval().float()
    with torch.no_grad():
        for p in model.parameters():          # biases and LayerNorm terms away from their 0 / 1 init
            p.add_(0.05 * torch.randn_like(p))
    assert eclip.hf_activation(config.to_dict()) == act
    sd = eclip.state_dict_from_hf(model.state_dict())
    cfg = eclip.config_from_state_dict(sd)
    assert (cfg['width'], cfg['layers'], cfg['patch'], cfg['text_layers']) == (64, 2, 16, 2)
    if act == 'gelu':
        monkeypatch.setattr(clip_ref, 'quick_gelu', ref.exact_gelu)
    img = torch.randn(3, 3, 32, 32)
    tok = torch.randint(1, 60, (4, 8))
    tok[:, 5] = 63                            # the EOT id is the largest: argmax finds it, as HF's eos_token_id lookup does
    with torch.no_grad():
        want_i = model.get_image_features(pixel_values=img)
        want_t = model.get_text_features(input_ids=tok)
    want_i = getattr(want_i, 'pooler_output', want_i)
    want_t = getattr(want_t, 'pooler_output', want_t)
    assert ref.rel_err(clip_ref.encode_image(sd, cfg, img), want_i) < 1e-5
    assert ref.rel_err(clip_ref.encode_text(sd, cfg, tok), want_t) < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# planted faults: the checks the GPU tests run, on the fp32 restatement of the epilogues with a faulty activation
# ---------------------------------------------------------------------------------------------------------------
def _quick32(v):
    return rr.gelu32(v)


def _cancelling32(v):
    """x Phi(x) with Phi = (1 + erf(x / sqrt 2)) / 2, every operation in fp32."""
    return v * (0.5 * (1 + torch.erf(v * torch.tensor(0.70710678118654752, dtype=F32))))


def _grad_without_x_phi(u):
    h = torch.from_numpy(ref._tail32(u.numpy())[0])        # Phi alone
    return torch.where(u < 0, h, 1 - h)


CASES = [('gelu16', None, None), ('gelu16', 'both', '16'), ('gelu16', 'a_lo8', 'e4m3'), ('gelu16_ln', None, None),
         ('gelu16_save', None, None), ('gelu_bwd16', None, None)]


# (the e4m3 lo products are f16 only)
@pytest.mark.parametrize('epi,seg,lo_out,dt', [c + (d,) for c in CASES for d in (F16, BF16) if d == F16 or c[1] != 'a_lo8'],
                         ids=lambda v: str(v).replace('torch.', ''))
@pytest.mark.parametrize('family', ['random', 'tails'])
def test_checks_pass_the_restatement_and_reject_planted_faults(epi, seg, lo_out, family, dt):
    """gelu_ref.case_specs + gemm_ref.check, what tests/test_gelu_gpu.py holds ec_gemm(activation = 1) to: the fault-free
    restatement passes; QuickGELU in place of GELU and a gradient without its x phi(x) term do not."""
    c = ref.make_case(epi, dt, 33, 48, 128, family, 0, seg, lo_out)
    specs = ref.case_specs(c)
    gr.check(specs, ref.restate(c), 'restatement', c['aux_exp'])
    fault = dict(grad=_grad_without_x_phi) if epi == 'gelu_bwd16' else dict(gelu=_quick32)
    with pytest.raises(AssertionError, match='over the bound'):
        gr.check(specs, ref.restate(c, **fault), 'planted', c['aux_exp'])


def test_quick_gelu_specs_reject_the_exact_gelu_and_the_other_way_round():
    """The two activations' expectations exclude each other on the same case (a swap cannot pass either suite)."""
    c = ref.make_case('gelu16', F16, 33, 48, 128, 'random')
    with pytest.raises(AssertionError):
        gr.check(gr.case_specs(c), ref.restate(c), 'exact GELU against QuickGELU specs')
    gr.check(gr.case_specs(c), gr.case_restate(c), 'QuickGELU against its own specs')


@pytest.mark.parametrize('dt,floor', [(BF16, 0.0), (F32, 0.0)], ids=['bfloat16 pair', 'fp32'])
def test_split_checks_reject_phi_by_cancellation_at_minus_6(dt, floor):
    """What the row-kernel test of tests/test_gelu_gpu.py runs on ec_split16(gelu = 2): the bounds of gelu_ref.split_bounds
    and the tail check.  (1 + erf) / 2 in fp32 is exactly 0 at x = -6: inside every absolute bound (2^-21 |x| = 2.9e-6 against
    x Phi(x) = -5.9e-9), caught by the tail check alone."""
    x = ref.split_input(64)
    assert float(x[10]) == -6.0

    def parts(v):
        if dt == F32:
            return v.double()
        hi, lo = rr.split(v, dt, dt)
        return hi.double() + lo.double()
    good, bad = parts(ref.gelu32_t(x)), parts(_cancelling32(x))
    want, _, b_pair = ref.split_bounds(x, BF16, BF16)
    assert rr.excess(good, want, b_pair) <= 0 and rr.excess(bad, want, b_pair) <= 0
    ref.tail_check(good, x, floor, 'restatement')
    with pytest.raises(AssertionError, match='cancellation'):
        ref.tail_check(bad, x, floor, 'planted')


# ---------------------------------------------------------------------------------------------------------------
# names, loaders, refusals (no GPU: nothing is packed)
# ---------------------------------------------------------------------------------------------------------------
def test_activation_names_and_config_key():
    from eventclip_amd import _lib
    from eventclip_amd import clip as eclip
    assert eclip.ACTIVATIONS == ('quick_gelu', 'gelu')
    assert (_lib.activation_code(None), _lib.activation_code('quick_gelu'), _lib.activation_code('gelu')) == (0, 1 - 1, 1)
    for name in eclip.ARCHS:
        assert eclip.arch_config(name)['activation'] == 'quick_gelu'
        assert eclip.arch_config(name, activation='gelu')['activation'] == 'gelu'
    for oc, ours in (('ViT-B-32', 'ViT-B/32'), ('ViT-B-16', 'ViT-B/16'), ('ViT-L-14', 'ViT-L/14')):
        want = dict(eclip.arch_config(ours), activation='gelu')
        assert eclip.arch_config(oc) == want
        assert eclip.arch_config(oc + '-quickgelu') == eclip.arch_config(ours)
    with pytest.raises(ValueError, match='tanh'):
        eclip.arch_config('ViT-B/32', activation='tanh')
    with pytest.raises(ValueError):
        _lib.activation_code('gelu_new')


@pytest.mark.parametrize('name,dim', [('ViT-H-14', 80), ('ViT-g-14', 88), ('ViT-bigG-14', 104), ('ViT-H-14-quickgelu', 80)])
def test_other_head_dimensions_are_refused_by_name(name, dim):
    from eventclip_amd import clip as eclip
    with pytest.raises(NotImplementedError, match=f'{dim} wide.*64'):
        eclip.arch_config(name)
    with pytest.raises(NotImplementedError, match='64'):
        eclip.load(name)


def test_resnet_towers_refuse_gelu():
    from eventclip_amd import clip as eclip
    from eventclip_amd.resnet import resnet_config
    with pytest.raises(NotImplementedError, match='ResNet'):
        eclip.build_random('RN50', device=None, activation='gelu')
    cfg = resnet_config('RN50', vision_layers=(1, 1, 1, 1))
    sd = eclip.random_state_dict(cfg, seed=0)
    with pytest.raises(NotImplementedError, match='ResNet'):
        eclip.build_from_state_dict(sd, device=None, activation='gelu')
    with pytest.raises(ValueError):
        eclip.build_from_state_dict(sd, device=None, activation='tanh')


def test_loaders_take_the_activation(tmp_path):
    """build_from_state_dict / load: None means QuickGELU (a state dict cannot say), 'gelu' lands in cfg['activation']; a plain
    torch.save'd state dict and *.safetensors read the same; unknown values raise."""
    from eventclip_amd import clip as eclip
    sd = eclip.random_state_dict(TINY, seed=2)
    assert eclip.build_from_state_dict(sd, device=None).cfg['activation'] == 'quick_gelu'
    assert eclip.build_from_state_dict(sd, device=None, activation='gelu').cfg['activation'] == 'gelu'
    with pytest.raises(ValueError):
        eclip.build_from_state_dict(sd, device=None, activation='relu')
    assert eclip.CLIP(TINY, sd).cfg['activation'] == 'quick_gelu'
    assert eclip.CLIP(dict(TINY, activation='gelu'), sd).cfg['activation'] == 'gelu'
    path = str(tmp_path / 'open_clip_pytorch_model.bin')
    torch.save(sd, path)
    m, pre = eclip.load(path, device=None, activation='gelu')
    assert m.cfg['activation'] == 'gelu' and eclip.load(path, device=None)[0].cfg['activation'] == 'quick_gelu'
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v.float())
    st = pytest.importorskip('safetensors.torch')
    spath = str(tmp_path / 'open_clip_model.safetensors')
    st.save_file({k: v.contiguous() for k, v in sd.items()}, spath)
    m2 = eclip.load(spath, device=None, activation='gelu')[0]
    assert m2.cfg == m.cfg and all(torch.equal(m2.state_dict()[k], m.state_dict()[k]) for k in sd)


def test_safetensors_missing_gives_a_clear_error(tmp_path, monkeypatch):
    from eventclip_amd import clip as eclip
    path = tmp_path / 'model.safetensors'
    path.write_bytes(b'\0' * 16)
    monkeypatch.setitem(sys.modules, 'safetensors', None)
    monkeypatch.setitem(sys.modules, 'safetensors.torch', None)
    with pytest.raises(ImportError, match='safetensors package'):
        eclip.load(str(path), device=None)


def hf_state_dict(sd):
    """The inverse of clip.state_dict_from_hf (OpenAI's layout -> transformers'), with the position_ids buffers HF saves."""
    out = {}
    top = {v: k for k, v in __import__('eventclip_amd.clip', fromlist=['_HF_TOP'])._HF_TOP}
    leaf = {'ln_1': 'layer_norm1', 'ln_2': 'layer_norm2', 'attn.out_proj': 'self_attn.out_proj', 'mlp.c_fc': 'mlp.fc1',
            'mlp.c_proj': 'mlp.fc2'}
    for k, v in sd.items():
        if k in top:
            out[top[k]] = v
        elif k == 'visual.proj':
            out['visual_projection.weight'] = v.t().contiguous()
        elif k == 'text_projection':
            out['text_projection.weight'] = v.t().contiguous()
        else:
            tower, rest = ('vision_model', k[len('visual.transformer.resblocks.'):]) if k.startswith('visual.') else \
                ('text_model', k[len('transformer.resblocks.'):])
            i, name = rest.split('.', 1)
            pre = f'{tower}.encoder.layers.{i}.'
            if name.startswith('attn.in_proj_'):
                kind = name[len('attn.in_proj_'):]
                for j, p in enumerate('qkv'):
                    out[f'{pre}self_attn.{p}_proj.{kind}'] = v.chunk(3, 0)[j].contiguous()
            else:
                mod, kind = name.rsplit('.', 1)
                out[f'{pre}{leaf[mod]}.{kind}'] = v
    out['vision_model.embeddings.position_ids'] = torch.arange(sd['visual.positional_embedding'].shape[0])[None]
    out['text_model.embeddings.position_ids'] = torch.arange(sd['positional_embedding'].shape[0])[None]
    return out


def hf_config(cfg, act):
    return dict(model_type='clip', projection_dim=cfg['embed_dim'],
                vision_config=dict(hidden_size=cfg['width'], num_attention_heads=cfg['width'] // 64, hidden_act=act,
                                   image_size=cfg['image_size'], patch_size=cfg['patch'], num_hidden_layers=cfg['layers']),
                text_config=dict(hidden_size=cfg['text_width'], num_attention_heads=cfg['text_heads'], hidden_act=act,
                                 num_hidden_layers=cfg['text_layers'], vocab_size=cfg['vocab_size']))


def write_hf_directory(path, sd, cfg, act, leaf='pytorch_model.bin'):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(hf_config(cfg, act), f)
    if leaf.endswith('.safetensors'):
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in hf_state_dict(sd).items()}, os.path.join(path, leaf))
    else:
        torch.save(hf_state_dict(sd), os.path.join(path, leaf))


def test_hf_directory_round_trip_and_refusals(tmp_path):
    from eventclip_amd import clip as eclip
    sd = eclip.random_state_dict(TINY, seed=2)
    back = eclip.state_dict_from_hf(hf_state_dict(sd))
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    for act in ('gelu', 'quick_gelu'):
        d = str(tmp_path / act)
        write_hf_directory(d, sd, TINY, act)
        m = eclip.load(d, device=None)[0]
        assert m.cfg['activation'] == act and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
        with pytest.raises(ValueError, match='contradicts'):
            eclip.load(d, device=None, activation='gelu' if act == 'quick_gelu' else 'quick_gelu')
    if pytest.importorskip('safetensors'):
        d = str(tmp_path / 'st')
        write_hf_directory(d, sd, TINY, 'gelu', 'model.safetensors')
        assert eclip.load(d, device=None)[0].cfg['activation'] == 'gelu'
    # refusals
    with pytest.raises(NotImplementedError, match='gelu_new'):
        eclip.hf_activation(hf_config(TINY, 'gelu_new'))
    wide = hf_config(TINY, 'gelu')
    wide['vision_config'].update(hidden_size=1280, num_attention_heads=16)
    with pytest.raises(NotImplementedError, match='80'):
        eclip.hf_activation(wide)
    mixed = hf_config(TINY, 'gelu')
    mixed['text_config']['hidden_act'] = 'quick_gelu'
    with pytest.raises(NotImplementedError, match='differ'):
        eclip.hf_activation(mixed)
    d = str(tmp_path / 'empty')
    os.makedirs(d)
    with open(os.path.join(d, 'config.json'), 'w') as f:
        json.dump(hf_config(TINY, 'gelu'), f)
    with pytest.raises(FileNotFoundError, match='model.safetensors'):
        eclip.load(d, device=None)
    extra = dict(hf_state_dict(sd), **{'vision_model.unknown.weight': torch.zeros(1)})
    with pytest.raises(KeyError, match='no counterpart'):
        eclip.state_dict_from_hf(extra)


def test_abi_carries_the_activation_fields():
    """The header, the ctypes mirrors and the library agree (ec_abi_check runs on load), ABI >= 607; the new field is the LAST one
    of the three weight structs and, in ec_gemm_args, fills the alignment padding behind `splits` (no field moved, the size is
    what it was); a zero-initialised struct means QuickGELU."""
    from eventclip_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'eventclip_hip.h')).read()
    assert f'#define EC_ABI_VERSION {_lib.ABI_VERSION}' in header and _lib.ABI_VERSION >= 607
    for t in (_lib.EcVitWeights, _lib.EcTextWeights, _lib.EcVitTrainWeights):
        assert t._fields_[-1][0] == 'activation' and t().activation == _lib.EC_ACT_QUICK_GELU == 0
    g = _lib.EcGemmArgs
    assert (g.splits.offset, g.activation.offset, g.split_stride.offset) == (104, 108, 112) and g().activation == 0
    assert ctypes.sizeof(g) == 248 and g._fields_[-1][0] == 'aux_exp'
    assert _lib.lib().ec_version() == _lib.ABI_VERSION
