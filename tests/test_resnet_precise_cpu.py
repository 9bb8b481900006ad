"""The ResNet towers' split-precision form on the CPU: the tolerance mode's keywords, the hi + lo weight split, the new
ABI entries and struct sizes, and the kernels of csrc/resnet_hl.hip compiled for gfx950."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from eventclip_amd import _lib
from eventclip_amd import clip as eclip
from eventclip_amd import resnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HL_SYMBOLS = ('ec_resnet_conv_hl', 'ec_resnet_stem_rows_hl', 'ec_resnet_avgpool_hl', 'ec_resnet_attnpool_tokens_hl',
              'ec_resnet_attnpool_attend_hl')


@pytest.mark.parametrize('arch', list(resnet.RESNET_ARCHS))
def test_tolerance_mode_kwargs_answers_for_resnets(arch):
    """Every ResNet name and config gets keywords ResNetCLIP accepts (packing is lazy: no GPU needed); until a sweep over
    held-out draws has picked smaller counts the mode is every block."""
    kw = eclip.tolerance_mode_kwargs(arch)
    cfg = eclip.resnet_config(arch)
    assert kw == eclip.tolerance_mode_kwargs(cfg) == dict(precise_blocks=sum(cfg['vision_layers']))
    small = eclip.resnet_config(arch, vision_layers=(1, 1, 1, 1))
    assert eclip.tolerance_mode_kwargs(small) == dict(precise_blocks=4)
    sd = resnet.random_state_dict(small, 0, calib_images=0)
    m = resnet.ResNetCLIP(small, sd, **eclip.tolerance_mode_kwargs(small))
    assert m.precise_blocks == 4
    assert resnet.ResNetCLIP(small, sd, precise=True).precise_blocks == 4
    assert resnet.ResNetCLIP(small, sd).precise_blocks == 0
    assert resnet.ResNetCLIP(small, sd, precise_blocks=2).precise_blocks == 2
    for bad in (-1, 5):
        with pytest.raises(ValueError, match='precise_blocks'):
            resnet.ResNetCLIP(small, sd, precise_blocks=bad)
    with pytest.raises(ValueError, match='float16'):
        resnet.ResNetCLIP(small, sd, dtype='bfloat16', precise_blocks=1)
    resnet.ResNetCLIP(small, sd, dtype='bfloat16')            # the 16-bit path keeps bf16


def test_builders_pass_the_mode_through():
    m = eclip.build_random('RN50', seed=0, device=None, vision_layers=(1, 1, 1, 1), precise_blocks=3)
    assert m.precise_blocks == 3 and m.cfg['vision_layers'] == (1, 1, 1, 1)
    m2 = eclip.build_from_state_dict(m.state_dict(), device=None, precise_blocks=4)
    assert m2.precise_blocks == 4
    assert eclip.build_from_state_dict(m.state_dict(), device=None).precise_blocks == 0


def test_vit_answers_unchanged_and_arch_config_keeps_raising():
    short, long_ = eclip.TOLERANCE_MODE
    assert eclip.tolerance_mode_kwargs('ViT-L/14') == dict(image_precise_blocks=short[0],
                                                           image_precise_attn_blocks=short[1])
    assert eclip.tolerance_mode_kwargs('ViT-L/14@336px') == dict(image_precise_blocks=long_[0],
                                                                 image_precise_attn_blocks=long_[1])
    assert eclip.tolerance_mode_kwargs('ViT-B/32')['image_precise_blocks'] == 11
    with pytest.raises(NotImplementedError):
        eclip.arch_config('RN50')
    with pytest.raises(Exception):
        eclip.tolerance_mode_kwargs('RN51')


def test_weight_split_restores_fp32():
    """resnet.split_hl, the split _pack uses: hi = f16(w), lo = f16((w - hi) * 2^11).

    Bound.  w - hi is exact in fp32 (hi keeps the leading 11 bits of w's 24) and at most half an f16 step of w:
    2^-11 |w| where hi is normal, 2^-25 below 2^-14.  The scaling by 2^11 is exact.  lo is then one f16 rounding of a
    number no larger than |w| (normal hi) or 2^-14 (subnormal hi): relative 2^-11 where lo is normal, absolute 2^-25
    where it is not.  Undoing the scale: |hi + lo / 2^11 - w| <= 2^-22 |w| + 2^-36 -- twice as tight as the 2^-21 of an
    unscaled f16 lo plane, and without that plane's floor of 2^-25 absolute (2^-19 of a weight of 0.02)."""
    g = torch.Generator().manual_seed(0)
    cfg = eclip.resnet_config('RN50x64')
    shapes = [(64, 3, 3, 3)]                                   # the stem, then the largest classes of RN50x64, c_proj
    w = cfg['vision_width']
    shapes += [(w * 8, w * 8, 3, 3), (w * 32, w * 8, 1, 1), (w * 8, w * 32, 1, 1), (cfg['embed_dim'], 32 * w, 1, 1)]
    worst = 0.0
    for sh in shapes:
        fan = sh[1] * sh[2] * sh[3]
        t = torch.randn(*sh, generator=g) * fan ** -0.5
        t.view(-1)[:7] = torch.tensor([0.0, 1.0, -65504.0, 2.0 ** -14, 3e-6, -1e-7, 2.0 ** -24 * 1.4])
        hi, lo = resnet.split_hl(t)
        assert hi.dtype == lo.dtype == torch.float16 and torch.equal(hi, t.half())
        assert torch.isfinite(lo.float()).all()
        err = (hi.double() + lo.double() / resnet.LO_SCALE - t.double()).abs()
        bound = 2.0 ** -22 * t.double().abs() + 2.0 ** -36
        assert bool((err <= bound).all()), (sh, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f'worst err / bound {worst:.3f}')
    assert resnet.LO_SCALE == 2048.0


def test_new_symbols_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'eventclip_hip.h')).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in HL_SYMBOLS:
        assert re.search(r'EC_API\s+int\s+' + s + r'\s*\(', text), s
        assert hasattr(handle, s), s
        assert s in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 602 and _lib.lib().ec_version() == _lib.ABI_VERSION


def test_struct_sizes_match_header():
    """The library's own check of ec_resnet_weights.struct_bytes.  (The sizes and offsets of these structs, like every
    other's, against a C program compiled from the header: tests/test_capi_symbols.py.)"""
    lib = _lib.lib()
    w = _lib.EcResnetWeights()
    w.struct_bytes = ctypes.sizeof(_lib.EcResnetWeights) - 8          # the struct of ABI 601
    assert lib.ec_resnet_workspace_bytes(ctypes.byref(w), 4) == 0
    assert b'struct_bytes' in lib.ec_last_error()


def _fake_weights(precise_blocks, dtype=_lib.EC_F16, lo=True):
    """A shape-complete RN50 (1, 1, 1, 1) ec_resnet_weights whose pointers are never dereferenced (the workspace size
    and the argument checks run on the host)."""
    p = 256
    cfg = eclip.resnet_config('RN50', vision_layers=(1, 1, 1, 1))

    def cw(ks, cin, cout):
        r = _lib.EcResnetConvW()
        r.w, r.scale, r.bias, r.ks, r.cin, r.cout = p, p, p, ks, cin, cout
        r.w_lo = p if lo else None
        return r
    spec = resnet.blocks_of(cfg)
    blocks = (_lib.EcResnetBlock * len(spec))()
    for bk, (_, inp, planes, stride, ds) in zip(blocks, spec):
        bk.stride = stride
        bk.c1, bk.c2, bk.c3 = cw(1, inp, planes), cw(3, planes, planes), cw(1, planes, 4 * planes)
        if ds:
            bk.ds = cw(1, inp, 4 * planes)
    w = _lib.EcResnetWeights()
    w.struct_bytes = ctypes.sizeof(_lib.EcResnetWeights)
    w.dtype, w.image_size, w.n_blocks, w.embed_dim = dtype, 224, len(spec), 1024
    w.stem[0], w.stem[1], w.stem[2] = cw(1, 64, 64), cw(3, 64, 64), cw(3, 64, 64)
    w.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.EcResnetBlock))
    w.pos = p
    w.q, w.kv, w.c = cw(1, 2048, 2048), cw(1, 2048, 4096), cw(1, 2048, 1024)
    w.precise_blocks = precise_blocks
    return w, blocks


def test_workspace_accounts_for_the_second_plane_and_mode_is_checked():
    lib = _lib.lib()
    w0, keep0 = _fake_weights(0)
    base = lib.ec_resnet_workspace_bytes(ctypes.byref(w0), 8)
    assert base > 0
    for pb in (1, 3, 4):
        w, keep = _fake_weights(pb)
        assert lib.ec_resnet_workspace_bytes(ctypes.byref(w), 8) == 2 * base, pb
    for pb in (-1, 5):
        w, keep = _fake_weights(pb)
        assert lib.ec_resnet_workspace_bytes(ctypes.byref(w), 8) == 0
        assert b'precise_blocks' in lib.ec_last_error()
    w, keep = _fake_weights(2, dtype=_lib.EC_BF16)
    assert lib.ec_resnet_workspace_bytes(ctypes.byref(w), 8) == 0 and b'EC_F16' in lib.ec_last_error()
    w, keep = _fake_weights(2, lo=False)
    assert lib.ec_resnet_workspace_bytes(ctypes.byref(w), 8) == 0 and b'w_lo' in lib.ec_last_error()
    w, keep = _fake_weights(0, lo=False)                               # the 16-bit path needs no lo planes
    assert lib.ec_resnet_workspace_bytes(ctypes.byref(w), 8) == base


def test_split_kernel_arguments_checked():
    """The split entry points refuse bf16 and bad shapes before any launch; n_img = 0 is a no-op."""
    lib = _lib.lib()
    F16, BF16 = _lib.EC_F16, _lib.EC_BF16
    b = ctypes.c_void_p(256)

    def refused(rc, fn):
        assert rc == _lib.EC_ERR_INVALID and fn.encode() in lib.ec_last_error(), (fn, rc, lib.ec_last_error())

    def conv(n=1, H=4, W=4, cin=64, cout=64, ks=1, rh=None, rl=None, out_lo=b, out32=0, dt=F16):
        return lib.ec_resnet_conv_hl(b, b, n, H, W, cin, cout, ks, b, b, None, b, rh, rl, 1, b, out_lo, out32, dt, None)
    fn = 'ec_resnet_conv_hl'
    refused(conv(dt=BF16), fn)
    refused(conv(ks=2), fn)
    refused(conv(cin=96), fn)
    refused(conv(cout=32), fn)
    refused(conv(rh=b, rl=None), fn)
    refused(conv(rh=b, rl=b, out32=1), fn)
    refused(conv(out_lo=None), fn)
    refused(conv(H=0), fn)
    assert conv(n=0) == _lib.EC_OK
    refused(lib.ec_resnet_stem_rows_hl(b, _lib.EC_PRE_HWC_U8, 1, 224, b, b, BF16, None), 'ec_resnet_stem_rows_hl')
    refused(lib.ec_resnet_stem_rows_hl(b, _lib.EC_PRE_HWC_U8, 1, 225, b, b, F16, None), 'ec_resnet_stem_rows_hl')
    refused(lib.ec_resnet_stem_rows_hl(b, _lib.EC_PRE_HWC_U8, 1, 224, b, None, F16, None), 'ec_resnet_stem_rows_hl')
    refused(lib.ec_resnet_avgpool_hl(b, b, 1, 4, 4, 12, b, b, F16, None), 'ec_resnet_avgpool_hl')
    refused(lib.ec_resnet_avgpool_hl(b, b, 1, 4, 4, 8, b, b, BF16, None), 'ec_resnet_avgpool_hl')
    refused(lib.ec_resnet_avgpool_hl(b, None, 1, 4, 4, 8, b, b, F16, None), 'ec_resnet_avgpool_hl')
    refused(lib.ec_resnet_attnpool_tokens_hl(b, b, 1, 0, 64, b, b, b, b, b, F16, None), 'ec_resnet_attnpool_tokens_hl')
    refused(lib.ec_resnet_attnpool_tokens_hl(b, b, 1, 49, 64, b, b, b, b, b, BF16, None), 'ec_resnet_attnpool_tokens_hl')
    refused(lib.ec_resnet_attnpool_attend_hl(b, b, b, b, 1, 257, 64, b, b, F16, None), 'ec_resnet_attnpool_attend_hl')
    refused(lib.ec_resnet_attnpool_attend_hl(b, b, b, b, 1, 50, 96, b, b, F16, None), 'ec_resnet_attnpool_attend_hl')
    refused(lib.ec_resnet_attnpool_attend_hl(b, b, b, b, 1, 50, 64, b, b, BF16, None), 'ec_resnet_attnpool_attend_hl')
    assert lib.ec_resnet_stem_rows_hl(None, _lib.EC_PRE_HWC_U8, 0, 224, None, None, F16, None) == _lib.EC_OK
    assert lib.ec_resnet_avgpool_hl(None, None, 0, 14, 14, 64, None, None, F16, None) == _lib.EC_OK
    assert lib.ec_resnet_attnpool_tokens_hl(None, None, 0, 49, 2048, None, None, None, None, None, F16, None) == _lib.EC_OK
    assert lib.ec_resnet_attnpool_attend_hl(None, None, None, None, 0, 50, 2048, None, None, F16, None) == _lib.EC_OK


def test_split_kernels_compile_without_scratch(tmp_path):
    """The condition tests/test_resnet_cpu.py puts on csrc/resnet.hip, on csrc/resnet_hl.hip: six kernels, none with
    scratch, the convolution on the gfx950 16x16x32 f16 MFMA with conv_igemm_kernel's 36 KiB of LDS."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip('no hipcc')
    src = os.path.join(ROOT, 'eventclip_amd', 'csrc', 'resnet_hl.hip')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc',
                        '-I', os.path.join(ROOT, 'include'), '-c', src, '-o', str(tmp_path / 'resnet_hl.o'),
                        '-save-temps=obj'],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    asm = open(next(str(p) for p in tmp_path.iterdir() if p.name.endswith('gfx950.s'))).read()
    kernels = re.findall(r'^(_ZN2ec12_GLOBAL__N_1\d+(\w+?)_kernel\w*):', asm, re.M)
    names = {k[1] for k in kernels}
    assert names == {'conv_igemm_hl', 'stem_rows_hl', 'avgpool2_hl', 'attnpool_tokens_hl', 'attnpool_attend_hl'}, names
    assert len(kernels) == 6
    sizes = re.findall(r'\.amdhsa_private_segment_fixed_size (\d+)', asm)
    assert len(sizes) == 6 and all(s == '0' for s in sizes), sizes
    assert 'v_mfma_f32_16x16x32_f16' in asm
    lds = [int(v) for v in re.findall(r'\.amdhsa_group_segment_fixed_size (\d+)', asm)]
    assert max(lds) == 2 * 128 * 72 * 2, lds
