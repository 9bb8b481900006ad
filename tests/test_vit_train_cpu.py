"""Host-side choices of the fine-tuning backward pass (csrc/vit_train.hip) that depend on the row count M = n S, and
the workspace layout query the stage tests read the tape through.  No GPU needed.

The row-count choices are restated here at the 256 CUs the MI355X has, and the shape set of
tests/test_vit_train_stages_gpu.py must reach every branch of them: both padding rules, one and several K-batches
with a ragged last row batch, gemm_rows32's K-batched tail taken and not taken, more than one LoRA row slab."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_train_ref as ref  # noqa: E402

CUS = 256


# ---- restatements of the host functions (csrc/vit_train.hip) ----
def padded_rows(M):
    mp = (M + 63) // 64 * 64
    return (M + 1023) // 1024 * 1024 if M >= 2048 else mp


def pick_splits(n_out, n_in, mp, cus=CUS):
    tiles = ((n_out + 255) // 256) * ((n_in + 255) // 256)
    s = 1
    while s < 16 and tiles * s * 2 <= cus and (mp // 64) % (s * 2) == 0 and mp // (s * 2) >= 256:
        s *= 2
    return s


def pick_splits_rows(n_out, n_in, rows, cus=CUS):
    tiles = ((n_out + 255) // 256) * ((n_in + 255) // 256)
    s = min(cus // tiles, 16)
    while s > 1 and rows // s < 256:
        s -= 1
    return max(s, 1)


def row_batches(rows, splits):
    """weight_grad_rows: K per batch (a multiple of 64) and the rows of the last batch that has any (batches past the
    end read only zeros)."""
    K = ((rows + splits - 1) // splits + 63) // 64 * 64
    return K, rows - (rows - 1) // K * K


def rows32_splits(M, N, K, cus=CUS):
    """gemm_rows32: the K-batch count of the tail (1 = the single launch)."""
    rem, tiles_n = M % 256, (N + 255) // 256
    full = M - rem
    tiles_main = (full // 256) * tiles_n
    extra = full > 0 and 0 < rem <= 128 and (tiles_main + cus - 1) // cus < (tiles_main + tiles_n + cus - 1) // cus
    s = 1
    if extra and K >= 2048:
        while s < 8 and tiles_n * s * 2 <= cus and (K // 64) % (s * 2) == 0 and K // (s * 2) >= 256:
            s *= 2
    return s


def lora_slabs(M, W, r, n_outer, shared, cus=CUS):
    """lora_grads: row slabs of the outer products (slab at least 256 rows)."""
    RT = (r + 15) // 16
    Mp = (M + 31) // 32 * 32
    want = max((2 if shared or RT > 1 else 4) * cus // (n_outer * ((W + 255) // 256)), 1)
    slab = max(((Mp + want - 1) // want + 31) // 32 * 32, 256)
    return (Mp + slab - 1) // slab


def _shapes():
    for case in ref.CASES:
        R, P, W, n, S, M = ref.case_geometry(case)
        yield case, W, M


def test_restated_choices_at_the_issue_shapes():
    """Spot values: the tail split at 64 frames of L/14 (rem 64, 256 + 4 tiles: a second round) and not at 32."""
    assert rows32_splits(16448, 1024, 4096) == 8 and rows32_splits(16448, 1024, 3072) == 8
    assert rows32_splits(8224, 1024, 4096) == 1 and rows32_splits(6304, 768, 3072) == 1
    assert padded_rows(1154) == 1216 and padded_rows(6304) == 7168
    assert pick_splits_rows(3 * 768, 768, 6304) == 9 and pick_splits_rows(64, 64, 25) == 1


def test_stage_shapes_reach_every_branch():
    seen = set()
    for case, W, M in _shapes():
        seen.add('pad1024' if M >= 2048 else 'pad64')
        for n_out, n_in in ((3 * W, W), (W, W), (4 * W, W), (W, 4 * W)):
            s = pick_splits_rows(n_out, n_in, M)
            if s == 1:
                seen.add('rows_splits1')
            else:
                seen.add('rows_splits>1')
                K, last = row_batches(M, s)
                assert 0 < last <= K, (case, n_out, n_in)
                if last < K:
                    seen.add('ragged_last_batch')
        kpad = 64
        if pick_splits(W, kpad, padded_rows(M)) > 1:
            seen.add('conv_splits>1')
        for K in (3 * W, 4 * W):              # the dX GEMMs of q k v and c_fc, the forward's c_proj
            seen.add('tail_split' if rows32_splits(M, W, K) > 1 else 'single_launch')
        if lora_slabs(M, W, 16, 1, True) > 1:
            seen.add('lora_slabs>1')
    want = {'pad64', 'pad1024', 'rows_splits1', 'rows_splits>1', 'ragged_last_batch', 'conv_splits>1', 'tail_split',
            'single_launch', 'lora_slabs>1'}
    assert want <= seen, want - seen


# ---- ec_vit_train_layout ----
def _weights(image_size, patch, width, layers):
    from eventclip_amd import _lib
    w = _lib.EcVitWeights()
    w.image_size, w.patch, w.width, w.layers, w.heads = image_size, patch, width, layers, width // 64
    w.kpad = ((2 * 3 * patch * patch + 63) // 64) * 64
    w.out_dim = 512
    return w


@pytest.mark.parametrize('case,layers', [('b16_n32', 2), ('l14_n64', 2), ('wide_odd_n9', 3), ('tiny_n5', 1)])
def test_layout_slots_tile_the_workspace(case, layers):
    """Every slot lies inside ec_vit_train_workspace_bytes, 256-byte aligned, at its documented size, and no two
    overlap; the tape comes first (pre at 0)."""
    from eventclip_amd import _lib
    R, P, W, n, S, M = ref.case_geometry(case)
    w = _weights(R, P, W, layers)
    lib = _lib.lib()
    total = int(lib.ec_vit_train_workspace_bytes(ctypes.byref(w), n))
    cnt = lib.ec_vit_train_layout(ctypes.byref(w), n, None, 0)
    assert cnt == _lib.EC_VT_BLOCK0 + _lib.EC_VT_PER_BLOCK * layers
    assert lib.ec_vit_train_layout(ctypes.byref(w), n, (ctypes.c_int64 * 1)(), 1) == _lib.EC_ERR_INVALID
    offs = (ctypes.c_int64 * cnt)()
    assert lib.ec_vit_train_layout(ctypes.byref(w), n, offs, cnt) == cnt
    H = W // 64
    size = {_lib.EC_VT_PRE: 4 * M * W, _lib.EC_VT_X_LAST: 4 * M * W, _lib.EC_VT_DX: 4 * M * W, _lib.EC_VT_DX16: 2 * M * W,
            _lib.EC_VT_DH32: 4 * M * W, _lib.EC_VT_DA16: 2 * M * W, _lib.EC_VT_G16: 8 * M * W,
            _lib.EC_VT_DELTA: 4 * n * H * S, _lib.EC_VT_CLSLN: 4 * n * W, _lib.EC_VT_DCLSLN: 4 * n * W}
    per = {_lib.EC_VT_B_X: 4 * M * W, _lib.EC_VT_B_XM: 4 * M * W, _lib.EC_VT_B_QKV: 6 * M * W, _lib.EC_VT_B_ATT: 2 * M * W,
           _lib.EC_VT_B_U: 8 * M * W, _lib.EC_VT_B_GACT: 8 * M * W, _lib.EC_VT_B_H1: 2 * M * W, _lib.EC_VT_B_H2: 2 * M * W,
           _lib.EC_VT_B_LSE: 4 * n * H * S}
    for l in range(layers):
        for k, v in per.items():
            size[_lib.EC_VT_BLOCK0 + _lib.EC_VT_PER_BLOCK * l + k] = v
    assert sorted(size) == list(range(cnt))
    spans = sorted((offs[i], offs[i] + size[i], i) for i in range(cnt))
    assert offs[_lib.EC_VT_PRE] == 0
    assert all(o % 256 == 0 for o, _, _ in spans)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), 'overlapping slots'
    assert spans[-1][1] <= total
    # the tape in carve order: x[0] right after pre, block 0's x before x[L]
    assert offs[_lib.EC_VT_BLOCK0 + _lib.EC_VT_B_X] == 4 * M * W
    assert offs[_lib.EC_VT_X_LAST] > offs[_lib.EC_VT_BLOCK0 + _lib.EC_VT_PER_BLOCK * (layers - 1)]
