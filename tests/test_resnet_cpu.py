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


def _packer_classes(cfg):
    """{(ks, cin, cout, H_in): roles} and the projections as the packer (blocks_of + pad64) and ec_resnet_encode lay
    the tower out."""
    p = resnet.pad64
    w, R = cfg['vision_width'], cfg['image_size']
    h = R // 2
    out = {}

    def add(key, role):
        out.setdefault(key, set()).add(role)
    add((1, 64, p(w // 2), h), 'relu')
    add((3, p(w // 2), p(w // 2), h), 'relu')
    add((3, p(w // 2), p(w), h), 'relu')
    h //= 2
    for _, inp, planes, stride, ds in resnet.blocks_of(cfg):
        ho = h // stride
        add((1, p(inp), p(planes), h), 'relu')
        add((3, p(planes), p(planes), h), 'relu')
        add((1, p(planes), p(4 * planes), ho), 'resid')
        if ds:
            add((1, p(inp), p(4 * planes), ho), 'ds')
        h = ho
    C, L = 32 * w, h * h + 1
    return out, [('q', C, C, L), ('kv', C, 2 * C, L), ('c', C, cfg['embed_dim'], L)]


def test_launch_shapes_match_module_walk():
    """The packer's block spec against OpenAI's module tree: the convolutions that forward hooks see in a full-depth
    meta-device forward of the restatement (resnet_ref.conv_classes) are, for every arch, the classes that
    blocks_of + pad64 give ec_resnet_encode, with the same epilogue roles; 99 conv classes over the five towers."""
    every, projs = {}, set()
    for arch in OPENAI:
        cfg = eclip.resnet_config(arch)
        walk, walk_proj = resnet_ref.conv_classes(cfg)
        packed, packed_proj = _packer_classes(cfg)
        assert walk == packed, arch
        assert walk_proj == packed_proj, arch
        for k, v in walk.items():
            every.setdefault(k, set()).update(v)
        projs.update(walk_proj)
    assert len(every) == 99, len(every)
    assert len(projs) == 13, sorted(projs)        # RN50 and RN101 share q and kv
    assert sum(k[0] == 1 for k in every) > sum(k[0] == 3 for k in every)
    assert (1, 4096, 8192, 197) in {(1, ci, co, L) for r, ci, co, L in projs if r == 'kv'}


def _refused(rc, fn):
    from eventclip_amd import _lib
    assert rc == _lib.EC_ERR_INVALID, (fn, rc)
    msg = _lib.lib().ec_last_error()
    assert msg and fn.encode() in msg, (fn, msg)


def test_resnet_kernel_arguments_checked():
    """Every EC_REQUIRE of the five ResNet kernel entry points refuses before any launch (EC_ERR_INVALID, and
    ec_last_error names the function); n_img = 0 is a no-op that returns EC_OK even with null buffers."""
    import ctypes
    from eventclip_amd import _lib
    lib = _lib.lib()
    F16, BF16 = _lib.EC_F16, _lib.EC_BF16
    buf = ctypes.c_void_p(256)            # never dereferenced: every call below returns before a launch
    fn = 'ec_resnet_conv'

    def conv(n=1, H=4, W=4, cin=64, cout=64, ks=1, resid=None, out32=0, dt=F16):
        return lib.ec_resnet_conv(buf, n, H, W, cin, cout, ks, buf, None, buf, resid, 1, buf, out32, dt, None)
    for ks in (0, 2, 5, -1):
        _refused(conv(ks=ks), fn)
    for cin, cout in ((32, 64), (96, 64), (0, 64), (64, 32), (64, 200), (64, 0), (-64, 64)):
        _refused(conv(cin=cin, cout=cout), fn)
    _refused(conv(resid=buf, out32=1), fn)
    for dt in (-1, 2, 7):
        _refused(conv(dt=dt), fn)
    for n, H, W in ((-1, 4, 4), (1, 0, 4), (1, 4, 0)):
        _refused(conv(n=n, H=H, W=W), fn)
    _refused(lib.ec_resnet_conv(None, 1, 4, 4, 64, 64, 1, None, None, None, None, 1, None, 0, F16, None), fn)

    fn = 'ec_resnet_stem_rows'
    for R in (3, 225, 0, -2):
        _refused(lib.ec_resnet_stem_rows(buf, _lib.EC_PRE_HWC_U8, 1, R, buf, F16, None), fn)
    _refused(lib.ec_resnet_stem_rows(buf, _lib.EC_PRE_PATCHES16, 1, 224, buf, F16, None), fn)
    _refused(lib.ec_resnet_stem_rows(buf, _lib.EC_PRE_CHW_F32, 1, 224, buf, 2, None), fn)
    _refused(lib.ec_resnet_stem_rows(None, _lib.EC_PRE_CHW_F32, 1, 224, None, F16, None), fn)

    fn = 'ec_resnet_avgpool'
    for H, W, C in ((1, 4, 8), (4, 1, 8), (4, 4, 12), (4, 4, 0)):
        _refused(lib.ec_resnet_avgpool(buf, 1, H, W, C, buf, F16, None), fn)
    _refused(lib.ec_resnet_avgpool(buf, 1, 4, 4, 8, buf, 3, None), fn)
    _refused(lib.ec_resnet_avgpool(None, 1, 4, 4, 8, None, BF16, None), fn)

    fn = 'ec_resnet_attnpool_tokens'
    _refused(lib.ec_resnet_attnpool_tokens(buf, 1, 49, 64, buf, buf, buf, 2, None), fn)
    _refused(lib.ec_resnet_attnpool_tokens(buf, 65536, 49, 64, buf, buf, buf, F16, None), fn)
    _refused(lib.ec_resnet_attnpool_tokens(buf, 1, 0, 64, buf, buf, buf, F16, None), fn)
    _refused(lib.ec_resnet_attnpool_tokens(None, 1, 49, 64, None, None, None, F16, None), fn)

    fn = 'ec_resnet_attnpool_attend'
    for L, C in ((257, 64), (0, 64), (50, 96), (50, 32), (50, 0)):
        _refused(lib.ec_resnet_attnpool_attend(buf, buf, 1, L, C, buf, F16, None), fn)
    _refused(lib.ec_resnet_attnpool_attend(buf, buf, 1, 50, 64, buf, -1, None), fn)
    _refused(lib.ec_resnet_attnpool_attend(buf, buf, 65536, 50, 64, buf, F16, None), fn)
    _refused(lib.ec_resnet_attnpool_attend(None, None, 1, 50, 64, None, BF16, None), fn)

    # n_img = 0: nothing to do, and no buffer is needed
    for dt in (F16, BF16):
        assert lib.ec_resnet_conv(None, 0, 7, 7, 64, 128, 3, None, None, None, None, 1, None, 0, dt, None) == _lib.EC_OK
        assert lib.ec_resnet_stem_rows(None, _lib.EC_PRE_HWC_U8, 0, 224, None, dt, None) == _lib.EC_OK
        assert lib.ec_resnet_avgpool(None, 0, 14, 14, 64, None, dt, None) == _lib.EC_OK
        assert lib.ec_resnet_attnpool_tokens(None, 0, 49, 2048, None, None, None, dt, None) == _lib.EC_OK
        assert lib.ec_resnet_attnpool_attend(None, None, 0, 50, 2048, None, dt, None) == _lib.EC_OK
