"""ResNet CLIP towers on the CPU: configs, OpenAI key layout, FLOP count, calibrated random weights, and the
kernels of csrc/resnet.hip compiled for gfx950."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref  # noqa: E402

from eventclip_amd import clip as eclip  # noqa: E402
from eventclip_amd import resnet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPENAI = {   # OpenAI clip/model.py: (layers, width, image, embed_dim, text width)
    'RN50': ((3, 4, 6, 3), 64, 224, 1024, 512), 'RN101': ((3, 4, 23, 3), 64, 224, 512, 512),
    'RN50x4': ((4, 6, 10, 6), 80, 288, 640, 640), 'RN50x16': ((6, 8, 18, 8), 96, 384, 768, 768),
    'RN50x64': ((3, 15, 36, 10), 128, 448, 1024, 1024)}


@pytest.mark.parametrize('arch', list(OPENAI))
def test_config_and_state_dict_round_trip(arch):
    cfg = eclip.resnet_config(arch)
    layers, w, r, e, tw = OPENAI[arch]
    assert (cfg['vision_layers'], cfg['vision_width'], cfg['image_size'], cfg['embed_dim'], cfg['text_width'],
            cfg['text_heads']) == (layers, w, r, e, tw, tw // 64)
    sd = eclip.random_state_dict(cfg, seed=0) if arch == 'RN50' else resnet.random_state_dict(cfg, 0, calib_images=0)
    assert eclip.config_from_state_dict(sd) == cfg
    # OpenAI's key layout: the restatement (OpenAI's module tree) loads the visual keys strictly
    resnet_ref.from_state_dict(sd, cfg)
    for k in ('visual.conv1.weight', 'visual.bn3.running_var', 'visual.layer1.0.downsample.0.weight',
              'visual.layer1.0.downsample.1.weight', f'visual.layer4.{layers[3] - 1}.conv3.weight',
              'visual.attnpool.positional_embedding', 'visual.attnpool.q_proj.weight', 'visual.attnpool.c_proj.bias',
              'text_projection', 'logit_scale'):
        assert k in sd, k
    assert not any(k.startswith('visual.layer2.1.downsample') for k in sd)
    assert sd['visual.attnpool.positional_embedding'].shape == ((r // 32) ** 2 + 1, 32 * w)


def test_arch_config_keeps_raising_and_names_listed():
    with pytest.raises(NotImplementedError, match='resnet_config'):
        eclip.arch_config('RN50')
    names = eclip.available_models()
    for n in ('RN50', 'RN101', 'RN50x4', 'RN50x16', 'RN50x64', 'ViT-B/32', 'ViT-B/16', 'ViT-L/14'):
        assert n in names
    assert eclip.RESNET_ARCHS is resnet.RESNET_ARCHS


@pytest.mark.parametrize('arch,layers', [('RN50', None), ('RN101', None), ('RN50x4', (1, 1, 1, 1)),
                                         ('RN50x16', (2, 1, 1, 2)), ('RN50x64', (1, 1, 1, 1))])
def test_flop_count_matches_module_walk(arch, layers):
    cfg = eclip.resnet_config(arch, **({'vision_layers': layers} if layers else {}))
    m = resnet_ref.ModifiedResNet(cfg['vision_layers'], cfg['embed_dim'], cfg['vision_width'] // 2,
                                  cfg['image_size'], cfg['vision_width'])
    assert resnet.resnet_flops(cfg) == resnet_ref.flops_by_walk(m, cfg['image_size'])


def test_padded_flop_overhead():
    """What the zero channels cost: RN50x64 only the stem's 27 -> 64 K; RN50 / RN101 also the stem's w/2 = 32 channels
    (padded to 64); RN50x4 / RN50x16 their 40 / 48 / 80 / 96 / 160-channel convolutions."""
    ov = {a: resnet.padded_flop_overhead(eclip.resnet_config(a)) for a in OPENAI}
    assert 0 < ov['RN50x64'] < 0.001, ov
    want = {'RN50': 0.107, 'RN101': 0.065, 'RN50x4': 0.269, 'RN50x16': 0.094}
    for a, v in want.items():
        assert abs(ov[a] - v) < 0.001, (a, ov[a])


def test_calibrated_bn_outputs_bounded_through_rn101():
    """Every BatchNorm output of the restatement stays inside |x| < 32 through RN101's 33 blocks on a fresh input
    (fp16 holds 65504): the calibrated statistics keep them about unit scale."""
    cfg = eclip.resnet_config('RN101')
    sd = eclip.random_state_dict(cfg, seed=3)
    m = resnet_ref.from_state_dict(sd, cfg)
    outs = []
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        f = m(x, bn_outputs=outs)
    assert len(outs) == 3 + 2 * 0 + 3 * 33 + 4
    assert max(outs) < 32, max(outs)
    assert torch.isfinite(f).all() and f.shape == (2, 512)
    # the package's own fp32 forward (used for the calibration) is the restatement
    ref = resnet.forward_fp32(dict(sd), cfg, x)
    assert float((ref - f).abs().max()) < 1e-3 * float(f.abs().max())


def _hipcc():
    h = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    return h if (os.path.exists(h) or shutil.which(h)) else None


def test_resnet_kernels_compile_without_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('no hipcc')
    src = os.path.join(ROOT, 'eventclip_amd', 'csrc', 'resnet.hip')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc',
                        '-I', os.path.join(ROOT, 'include'), '-c', src, '-o', str(tmp_path / 'resnet.o'),
                        '-save-temps=obj'],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    asm = open(next(str(p) for p in tmp_path.iterdir() if p.name.endswith('gfx950.s'))).read()
    kernels = re.findall(r'^(_ZN2ec12_GLOBAL__N_1\d+(\w+?)_kernel\w*):', asm, re.M)
    names = {k[1] for k in kernels}
    assert {'conv_igemm', 'stem_rows', 'avgpool2', 'attnpool_tokens', 'attnpool_attend'} <= names, names
    assert len(kernels) == 12
    sizes = re.findall(r'\.amdhsa_private_segment_fixed_size (\d+)', asm)
    assert len(sizes) == 12 and all(s == '0' for s in sizes), sizes
    # the conv main loop runs on the gfx950 16x16x32 MFMA (f16 and bf16)
    assert 'v_mfma_f32_16x16x32_f16' in asm and 'v_mfma_f32_16x16x32_bf16' in asm


def test_gemm_isa_check_still_passes():
    if _hipcc() is None:
        pytest.skip('no hipcc')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_gemm_isa
    assert check_gemm_isa.main() == 0


def test_resnet_weights_struct_bytes_checked():
    """ec_resnet_weights carries its own size first; the library refuses a struct of another size (no GPU needed: the
    check runs before any launch)."""
    import ctypes
    from eventclip_amd import _lib
    lib = _lib.lib()
    w = _lib.EcResnetWeights()
    w.struct_bytes = ctypes.sizeof(_lib.EcResnetWeights) - 8
    assert lib.ec_resnet_workspace_bytes(ctypes.byref(w), 4) == 0
    assert lib.ec_resnet_encode(ctypes.byref(w), None, 0, 1, None, None, 0, 1, None) == _lib.EC_ERR_INVALID
    assert b'struct_bytes' in lib.ec_last_error()
    w.struct_bytes = ctypes.sizeof(_lib.EcResnetWeights)           # right size, but no blocks: still refused
    assert lib.ec_resnet_encode(ctypes.byref(w), None, 0, 1, None, None, 0, 1, None) == _lib.EC_ERR_INVALID


def test_random_state_dict_gains():
    cfg = eclip.resnet_config('RN50', vision_layers=(1, 1, 1, 1))
    a = resnet.random_state_dict(cfg, 0, calib_images=0, branch_gain=1.0)
    b = resnet.random_state_dict(cfg, 0, calib_images=0)
    assert torch.allclose(b['visual.layer2.0.bn3.weight'], 0.25 * a['visual.layer2.0.bn3.weight'])
    assert torch.equal(b['visual.layer2.0.bn2.weight'], a['visual.layer2.0.bn2.weight'])
    with pytest.raises(ValueError):
        eclip.random_state_dict(cfg, 0, qk_gain=2.0)
