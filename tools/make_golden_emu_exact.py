"""tests/golden/configs_oracle_0_signal_emu_exact.npz: the exact form of the fp16-reference emulation
(oracle/clip_ref.py, emulate='fp16_reference_exact': float64 carriers, every op exact before its fp16 rounding) on
BASELINE configs[0], signal weights, draw 0 -- the case tests/test_configs_cpu.py runs.  Unlike the fp32-carried form
in configs_oracle_0_signal.npz, these values do not depend on the host's BLAS path or thread count.

    python tools/make_golden_emu_exact.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import config_cases as cc   # noqa: E402

PATH = os.path.join(cc.GOLDEN_DIR, 'configs_oracle_0_signal_emu_exact.npz')


def main():
    inp = cc.build_inputs(0, 'signal', 0)
    emu, _ = cc.oracle_case(inp, emulate='fp16_reference_exact')
    # fp16 values: float32 holds them exactly
    np.savez_compressed(PATH, d0_fingerprint=cc.fingerprint(inp),
                        d0_emu_full_logits=emu['full_logits'].float().numpy(),
                        d0_emu_logits=emu['logits'].float().numpy())
    print(PATH)


if __name__ == '__main__':
    main()
