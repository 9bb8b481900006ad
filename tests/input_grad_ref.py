"""Float64 restatement of the vision tower's input gradient below ``ln_pre`` (csrc/vit_train.hip: ``embed_data_grad``,
``unpatchify_kernel``), for tests/test_input_grad_cpu.py and tests/test_input_grad_gpu.py.

``conv1`` has kernel = stride = patch and no bias, so the embedding is a matrix product over im2col rows: patch
(gy, gx) of an image is the row of its 3 p^2 pixels in ``conv1.weight``'s (c, i, j) order, and
``tok[n, gy g + gx, :] = row . conv1.weight.reshape(W, 3 p^2)^T``.  The data gradient is the adjoint of both steps:
``d_pix = d_tok . conv1.weight.reshape(W, 3 p^2)`` and ``d_image = unpatchify(d_pix)``, the rows put back where
``patchify`` took them from.  (On the device a patch row carries each pixel twice, as hi | lo 16-bit parts; here a
row holds the pixel's value once -- the gradient with respect to the pixel is formed once.)"""
import torch


def patchify(x, p):
    """[n, 3, R, R] -> [n, g g, 3 p p]: row gy g + gx holds x[n, c, gy p + i, gx p + j] at column (c p + i) p + j."""
    n, c, R, _ = x.shape
    g = R // p
    assert c == 3 and g * p == R and x.shape[3] == R
    return x.reshape(n, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, 3 * p * p)


def unpatchify(rows, p, R):
    """[n, g g, 3 p p] -> [n, 3, R, R]: the adjoint (and, patches not overlapping, the inverse) of ``patchify``."""
    n, G, k = rows.shape
    g = R // p
    assert G == g * g and k == 3 * p * p and g * p == R
    return rows.reshape(n, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(n, 3, R, R)


def embed_data_grad(d_tok, conv_w):
    """d_tok [n, g g, W] (the patch rows of d loss / d pre), conv1.weight [W, 3, p, p] -> d_image [n, 3, R, R]."""
    W, _, p, _ = conv_w.shape
    g = int(round(d_tok.shape[1] ** 0.5))
    assert g * g == d_tok.shape[1] and d_tok.shape[2] == W
    return unpatchify(d_tok @ conv_w.reshape(W, 3 * p * p), p, g * p)


def embed_data_grad_bound(d_tok, conv_w, unit):
    """The per-element bound of the device's product: one operand rounding (``unit``: 2^-11 f16, 2^-8 bf16; the weight
    goes in as hi + lo parts, its rounding does not enter) plus fp32 accumulation of W products,
    (unit + (W + 2) 2^-24) sum |d_tok| |w|, laid out as the image."""
    W, _, p, _ = conv_w.shape
    g = int(round(d_tok.shape[1] ** 0.5))
    mag = d_tok.abs() @ conv_w.reshape(W, 3 * p * p).abs()
    return (unit + (W + 2) * 2.0 ** -24) * unpatchify(mag, p, g * p)
