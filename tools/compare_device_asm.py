"""Do two trees compile a HIP source to the same device code?  Kernel by kernel, whatever order the kernels are emitted in.

    python tools/compare_device_asm.py OTHER_TREE [csrc file ...] [--diag]      # default: gemm.hip vit_train.hip

Compiles each file device-only to gfx950 assembly in both trees (the flags of eventclip_amd/build.py plus -fuse-cuid=none;
--diag adds the diagnostic build's macros) and compares the kernel symbol lists and, per kernel, the assembly text.  The
order in which hipcc emits template instantiations follows the host code that names them, so a host-only change can
move kernels around in the file; the numbers of local labels (.LBB<function>_<block>) move with them.  Both are
normalised, nothing else is.  Exit code 1 if a symbol or any kernel's text differs."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eventclip_amd import build as hip_build  # noqa: E402


def assembly(tree, name, diag, tmp):
    out = os.path.join(tmp, f'{abs(hash(tree))}_{name}.s')
    flags = [f if f != hip_build.INCLUDE else os.path.join(tree, 'include') for f in hip_build.FLAGS]
    cmd = [hip_build.HIPCC] + flags + (hip_build.DIAG_FLAGS if diag else []) + [
        '-fuse-cuid=none', '--cuda-device-only', '-S', os.path.join(tree, 'eventclip_amd', 'csrc', name), '-o', out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """-> {symbol: text of the function and its kernel descriptor}, {symbol: its metadata block}"""
    text = re.sub(r'BB\d+_', 'BB_', re.sub(r'[ \t]+;', ' ;', text))
    text = re.sub(r'\.L(func_end|func_begin|tmp|JTI)\d+', r'.L\1', text)
    meta_at = text.index('\t.amdgpu_metadata')
    body = text[:meta_at].split('\t.section\t.AMDGPU.gpr_maximums')[0]
    funcs = {}
    for chunk in re.split(r'(?m)^(?=\t\.section[^\n]*\n\t\.(?:globl|protected)\t)', body):
        m = re.search(r'(?m)^\t\.globl\t(\S+)', chunk)
        if m:
            funcs[m.group(1)] = chunk
    meta = {}
    for block in re.split(r'(?m)^(?=  - \.agpr_count:|  - \.args:)', text[meta_at:].split('amdhsa.target:')[0])[1:]:
        meta[re.search(r'\.symbol:\s+(\S+)', block).group(1)] = block
    return funcs, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('other')
    ap.add_argument('files', nargs='*', default=['gemm.hip', 'vit_train.hip'])
    ap.add_argument('--diag', action='store_true')
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.files:
            (f0, m0), (f1, m1) = (kernels(assembly(t, name, a.diag, tmp)) for t in (os.path.abspath(a.other), ROOT))
            differ = [k for k in f0 if k in f1 and (f0[k] != f1[k] or m0.get(k + '.kd', m0.get(k)) != m1.get(k + '.kd', m1.get(k)))]
            only = sorted(set(f0) ^ set(f1))
            print(f'{name}{" (diag)" if a.diag else ""}: {len(f0)} / {len(f1)} device functions, {len(only)} only on one side, '
                  f'{len(differ)} with different text')
            for k in only + differ:
                print('   ', k)
            bad += len(only) + len(differ)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
