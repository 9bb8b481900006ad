// Few-shot `text-identity` training step on cached image features (gfx950, fp32).
//
// Replaces, for adapter_type = 'text-identity' (configs/fsclip/text_adapter/*), what one optimisation
// step of the reference does around its frozen encoder:
//   forward   FSCLIPClassifier.forward, models/clip_cls.py:302-350: identity adapter, F.normalize of
//             the image features (:325-327), invalid views zeroed (:329), text_feats =
//             F.normalize(parameter) (:285-288), full_logits = logit_scale * feats @ text^T (:332),
//             aggregation (:104-129): sum, mean or max over the valid views;
//   loss      calc_train_loss, :164-175: cross-entropy on the aggregated logits, or NLL of
//             log(probs + 1e-6);
//   backward  d loss / d text_feats (torch autograd upstream), written out in closed form here:
//             dL[b,v,:] per view -> dU = logit_scale * dL^T . Fn (one fp32 GEMM over the B*T views)
//             -> through the row normalisation: dT = (dU - u (u . dU)) / |t|;
//   update    torch.optim.Adam (`optimizer = 'Adam'` in the configs).
// The encoder is frozen, so its features are an input (cached once per epoch); everything here is a
// few MFLOP per sample and latency / launch bound: six small launches on one stream (head_launches).
// The same head serves 'text-trans' behind the adapter (ec_fs_trans_loss_grad) and fine-tuning, where the features'
// own gradient goes back into the vision tower (ec_ft_loss_grad, models/clip_cls_ft.py:196-256).
#include "common.h"
#include "mfma.h"
#include "rowops.h"

namespace {

using ec::wave_max;
using ec::wave_sum;

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;

// the four wave results added in sequence (classify.hip's block_reduce pairs them: other bits)
__device__ float block_sum_f(float v, float *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < TR_WAVES; w++) t += red[w];
    return t;
}
__device__ float block_max_f(float v, float *red)
{
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = -INFINITY;
#pragma unroll
    for (int w = 0; w < TR_WAVES; w++) t = fmaxf(t, red[w]);
    return t;
}

// u[k, :] = t[k, :] / max(|t_k|, 1e-12)  (F.normalize, clip_cls.py:287); one wave per row
__global__ __launch_bounds__(64) void text_norm_kernel(const float *t, int D, float *u, float *inv_norm)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float x = t[(long)k * D + d];
        s += x * x;
    }
    const float inv = 1.f / fmaxf(__builtin_sqrtf(wave_sum(s)), 1e-12f);
    for (int d = lane; d < D; d += 64) u[(long)k * D + d] = t[(long)k * D + d] * inv;
    if (lane == 0) inv_norm[k] = inv;
}

// F.normalize per view, invalid views zero (clip_cls.py:325-329): one wave per view row.
// row_idx (optional): the features are compact over the valid views, row_idx[b, v] = their row.  valid == nullptr:
// a view is valid iff its row_idx names one of the n_rows rows.  normalize == 0: the rows are only gathered and masked.
__global__ __launch_bounds__(TR_THREADS) void fs_normalize_kernel(const float *feats, const unsigned char *valid,
                                                                  const int *row_idx, int n_rows, int normalize, int R,
                                                                  int D, float *Fn)
{
    const int lane = threadIdx.x & 63, r = blockIdx.x * TR_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;
    const int ri = row_idx ? row_idx[r] : r;
    const bool ok = valid ? valid[r] != 0 : (ri >= 0 && ri < n_rows);
    const long frow = row_idx ? (ok ? ri : 0) : (long)r;
    const float *f = feats + frow * D;
    float s = 0.f;
    if (ok && normalize)
        for (int d = lane; d < D; d += 64) s += f[d] * f[d];
    float inv = ok ? 1.f / fmaxf(__builtin_sqrtf(wave_sum(s)), 1e-12f) : 0.f;
    if (ok && !normalize) inv = 1.f;
    for (int d = lane; d < D; d += 64) Fn[(long)r * D + d] = ok ? f[d] * inv : 0.f;
}

// One workgroup per sample: its per-view logits (full_logits[v][k] = scale * fn_v . u_k, :332 -- an fp32 MFMA
// product of all view rows at once, left in the dL rows) into LDS, loss and dL rows.
// EC_AGG_MAX (:116-121, logits - 1e6 [invalid], then max): per class the maximum over the valid views; its gradient goes
// to that view alone, the lowest index on a tie, every other view gets an exact zero (classify_dz_kernel's rule).
// LDS: logits [T][K] | reduction scratch
__global__ __launch_bounds__(TR_THREADS) void fs_loss_grad_kernel(
    const unsigned char *valid, const int *labels, int B, int T, int K, int agg, int probs_loss, float *dL,
    float *loss_b, float *agg_logits)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *lg = sm, *red = lg + (size_t)T * K;
    float *pvy = red + TR_WAVES;          // [T] softmax probability of the label, per view
    float *vmax = pvy + T, *vsum = vmax + T;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = labels[b];
    float n_valid = 0.f;
    for (int v = 0; v < T; v++) n_valid += valid[b * T + v] ? 1.f : 0.f;
    for (int i = threadIdx.x; i < T * K; i += TR_THREADS) lg[i] = dL[(long)b * T * K + i];
    __syncthreads();

    float loss = 0.f;
    if (!probs_loss) {
        // ---- aggregated logits (:104-115), softmax cross-entropy (:171) ----
        const float wv = agg == EC_AGG_MEAN ? 1.f / n_valid : 1.f;   // every view, valid or not, gets wv
        float mx = -INFINITY;
        for (int k = threadIdx.x; k < K; k += TR_THREADS) {
            float s = 0.f;
            if (agg == EC_AGG_MAX) {
                s = -INFINITY;
                for (int v = 0; v < T; v++)
                    if (valid[b * T + v]) s = fmaxf(s, lg[v * K + k]);
            } else {
                for (int v = 0; v < T; v++) s += lg[v * K + k];
                s *= wv;
            }
            lg[k] = s;                      // row 0 now holds the aggregated logits (each k by one thread)
            mx = fmaxf(mx, s);
        }
        mx = block_max_f(mx, red);
        float se = 0.f;
        for (int k = threadIdx.x; k < K; k += TR_THREADS) se += __expf(lg[k] - mx);
        se = block_sum_f(se, red);
        const float lse = mx + __logf(se);
        loss = lse - lg[y];
        for (int k = threadIdx.x; k < K; k += TR_THREADS) {
            const float g = (__expf(lg[k] - lse) - (k == y ? 1.f : 0.f)) / (float)B;
            if (agg_logits) agg_logits[(long)b * K + k] = lg[k];
            if (agg == EC_AGG_MAX) {
                // the dL rows still hold this class's logits (only this thread writes column k): find the winner again
                int amax = -1;
                float best = -INFINITY;
                for (int v = 0; v < T; v++) {
                    const float l = dL[((long)b * T + v) * K + k];
                    if (valid[b * T + v] && l > best) best = l, amax = v;
                }
                for (int v = 0; v < T; v++) dL[((long)b * T + v) * K + k] = v == amax ? g : 0.f;
                continue;
            }
            for (int v = 0; v < T; v++) dL[((long)b * T + v) * K + k] = g * wv;
        }
    } else {
        // ---- per-view softmax, masked mean (:123-129), NLL of log(probs + 1e-6) (:172-174) ----
        for (int v = wave; v < T; v += TR_WAVES) {
            float mx = -INFINITY;
            for (int k = lane; k < K; k += 64) mx = fmaxf(mx, lg[v * K + k]);
            mx = wave_max(mx);
            float se = 0.f;
            for (int k = lane; k < K; k += 64) se += __expf(lg[v * K + k] - mx);
            se = wave_sum(se);
            if (lane == 0) vmax[v] = mx, vsum[v] = se, pvy[v] = __expf(lg[v * K + y] - mx) / se;
        }
        __syncthreads();
        float Py = 0.f;
        for (int v = 0; v < T; v++) Py += valid[b * T + v] ? pvy[v] : 0.f;
        Py /= n_valid;
        loss = -__logf(Py + 1e-6f);
        const float dPy = -1.f / ((float)B * (Py + 1e-6f));
        for (int k = threadIdx.x; k < K; k += TR_THREADS) {
            float agg_k = 0.f, max_k = -INFINITY;
            for (int v = 0; v < T; v++) {
                const float p = __expf(lg[v * K + k] - vmax[v]) / vsum[v];
                const float c = valid[b * T + v] ? dPy * pvy[v] / n_valid : 0.f;
                dL[((long)b * T + v) * K + k] = c * ((k == y ? 1.f : 0.f) - p);
                agg_k += lg[v * K + k];
                if (valid[b * T + v]) max_k = fmaxf(max_k, lg[v * K + k]);
            }
            if (agg_logits)
                agg_logits[(long)b * K + k] = agg == EC_AGG_MAX ? max_k : (agg == EC_AGG_MEAN ? agg_k / n_valid : agg_k);
        }
    }
    if (threadIdx.x == 0) loss_b[b] = loss;
}

// through F.normalize: dT_k = (dU_k - u_k (u_k . dU_k)) / |t_k|; block 0 also reduces the loss
__global__ __launch_bounds__(64) void text_grad_finish_kernel(const float *u, const float *dU,
                                                              const float *inv_norm, int D, const float *loss_b,
                                                              int B, float *grad, float *loss)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    float dot = 0.f;
    for (int d = lane; d < D; d += 64) dot += u[(long)k * D + d] * dU[(long)k * D + d];
    dot = wave_sum(dot);
    const float inv = inv_norm[k];
    for (int d = lane; d < D; d += 64)
        grad[(long)k * D + d] = (dU[(long)k * D + d] - u[(long)k * D + d] * dot) * inv;
    if (k == 0) {
        float s = 0.f;
        for (int b = lane; b < B; b += 64) s += loss_b[b];
        s = wave_sum(s);
        if (lane == 0) loss[0] = s / (float)B;                       // F.cross_entropy / nll_loss: mean
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float *p, const float *g, float *m, float *v, long n,
                                                   float lr, float b1, float b2, float eps, float wd,
                                                   float bc1, float bc2_sqrt)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float gi = g[i];
        if (wd != 0.f) gi += wd * p[i];
        const float mi = m[i] * b1 + (1.f - b1) * gi;
        const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
        m[i] = mi, v[i] = vi;
        p[i] -= lr / bc1 * mi / (__builtin_sqrtf(vi) / bc2_sqrt + eps);
    }
}

// ---- generic fp32 pieces of the transformer-adapter ('text-trans') step --------------------------
// C[M, N] (row stride ldc) = alpha * sum_k A(m, k) B(k, n) + beta * C + bias[n], optional ReLU.
// A(m, k) = A[m * sam + k * sak], B(k, n) = B[k * sbk + n * sbn]: one kernel for x W^T, dy W and dy^T x.
// 64 x 64 tiles, four waves of 32 x 32, fp32 MFMA (v_mfma_f32_16x16x4_f32: full fp32 products and sums); K in
// slabs of 16 through two LDS buffers, the next slab's global loads in flight while this one multiplies (these
// products are a few hundred k-steps on a handful of workgroups: un-pipelined they ran at the memory latency,
// 104 us each).  An operand whose k index is the fast one in memory is kept [row][k] in LDS (pitch 17), the other
// way round [k][row] (pitch 80): conflict-free stores and fragment reads in both.
template <bool RELU>
__global__ __launch_bounds__(256) void sgemm_kernel(const float *A, long sam, long sak, const float *Bm, long sbk,
                                                    long sbn, int M, int N, int K, float alpha, float beta,
                                                    const float *bias, float *C, long ldc)
{
    constexpr int BK = 16, TILE = 1280;               // max(64 * 17, 16 * 80) floats
    __shared__ float sa[2][TILE], sb[2][TILE];
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c16 = lane & 15;
    const int wy = wave >> 1, wx = wave & 1;
    const bool a_kfast = sak <= sam, b_kfast = sbk < sbn;
    // element u of this thread in a slab: (k, row) with the fast index following the smaller stride
    int ak[4], am[4], bk[4], bn[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int i = threadIdx.x + 256 * u;
        if (a_kfast) ak[u] = i & 15, am[u] = i >> 4; else am[u] = i & 63, ak[u] = i >> 6;
        if (b_kfast) bk[u] = i & 15, bn[u] = i >> 4; else bn[u] = i & 63, bk[u] = i >> 6;
    }
    float ra[4], rb[4];
    auto gload = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            ra[u] = (k0 + ak[u] < K && m0 + am[u] < M) ? A[(long)(m0 + am[u]) * sam + (long)(k0 + ak[u]) * sak] : 0.f;
            rb[u] = (k0 + bk[u] < K && n0 + bn[u] < N) ? Bm[(long)(k0 + bk[u]) * sbk + (long)(n0 + bn[u]) * sbn] : 0.f;
        }
    };
    auto at = [](bool kfast, int k, int row) { return kfast ? row * 17 + k : k * 80 + row; };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            sa[buf][at(a_kfast, ak[u], am[u])] = ra[u];
            sb[buf][at(b_kfast, bk[u], bn[u])] = rb[u];
        }
    };
    ec::f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = ec::f32x4{0.f, 0.f, 0.f, 0.f};
    gload(0);
    sstore(0);
    __syncthreads();
    for (int k0 = 0, buf = 0; k0 < K; k0 += BK, buf ^= 1) {
        const bool more = k0 + BK < K;
        if (more) gload(k0 + BK);
#pragma unroll
        for (int ks = 0; ks < BK / 4; ks++) {
            const int kq = ks * 4 + g;
            float a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                a[t] = sa[buf][at(a_kfast, kq, wy * 32 + t * 16 + c16)];
                b[t] = sb[buf][at(b_kfast, kq, wx * 32 + t * 16 + c16)];
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) sstore(buf ^ 1);
        __syncthreads();
    }
    // acc[i][j][r] = row m0 + 32 wy + 16 i + 4 g + r, column n0 + 32 wx + 16 j + c16
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int n = n0 + wx * 32 + j * 16 + c16;
            if (n >= N) continue;
            const float bv = bias ? bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = m0 + wy * 32 + i * 16 + 4 * g + r;
                if (m >= M) continue;
                float v = alpha * acc[i][j][r] + bv;
                if (beta != 0.f) v += beta * C[(long)m * ldc + n];
                if (RELU) v = fmaxf(v, 0.f);
                C[(long)m * ldc + n] = v;
            }
        }
}

// out[j] = sum_r X[r, j] (* Y[r, j] when Y): bias gradients and LayerNorm gamma / beta gradients.  A workgroup
// owns 64 columns; its 256 threads are 64 columns x 4 row lanes, eight independent loads in flight per thread
// (one dependent load per row was the whole cost: R / 4 memory latencies in a row).  Fixed order: reproducible.
__global__ __launch_bounds__(256) void colsum_kernel(const float *X, const float *Y, int R, int N, float *out)
{
    __shared__ float red[4][64];
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; u++) acc[u] = 0.f;
    if (j < N) {
        int r = part;
        for (; r + 28 < R; r += 32) {
            float x[8], y[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                x[u] = X[(long)(r + 4 * u) * N + j];
                y[u] = Y ? Y[(long)(r + 4 * u) * N + j] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) acc[u] += x[u] * y[u];
        }
        for (; r < R; r += 4) acc[0] += Y ? X[(long)r * N + j] * Y[(long)r * N + j] : X[(long)r * N + j];
    }
    red[part][threadIdx.x & 63] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    __syncthreads();
    if (part == 0 && j < N) out[j] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// LayerNorm over rows of width N <= 1024 (eps 1e-5, torch defaults): y, xhat, rstd; one wave per row
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *x, const float *g, const float *b, int R, int N,
                                                     float *y, float *xhat, float *rstd)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;
    const float *xr = x + (long)r * N;
    float s = 0.f;
    for (int j = lane; j < N; j += 64) s += xr[j];
    const float mean = wave_sum(s) / (float)N;
    float q = 0.f;
    for (int j = lane; j < N; j += 64) q += (xr[j] - mean) * (xr[j] - mean);
    const float rs = 1.f / __builtin_sqrtf(wave_sum(q) / (float)N + 1e-5f);
    for (int j = lane; j < N; j += 64) {
        const float h = (xr[j] - mean) * rs;
        xhat[(long)r * N + j] = h;
        y[(long)r * N + j] = h * g[j] + b[j];
    }
    if (lane == 0) rstd[r] = rs;
}

// dx[r, :] (+)= rstd * (gy - mean(gy) - xhat * mean(gy * xhat)), gy = dy * gamma
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float *dy, const float *xhat, const float *rstd,
                                                     const float *g, int R, int N, float *dx, int accumulate)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;
    float s1 = 0.f, s2 = 0.f;
    for (int j = lane; j < N; j += 64) {
        const float gy = dy[(long)r * N + j] * g[j];
        s1 += gy, s2 += gy * xhat[(long)r * N + j];
    }
    s1 = wave_sum(s1) / (float)N, s2 = wave_sum(s2) / (float)N;
    const float rs = rstd[r];
    for (int j = lane; j < N; j += 64) {
        const float v = rs * (dy[(long)r * N + j] * g[j] - s1 - xhat[(long)r * N + j] * s2);
        dx[(long)r * N + j] = accumulate ? dx[(long)r * N + j] + v : v;
    }
}

// Dropout (nn.TransformerEncoderLayer's p = 0.1 in train mode) without stored masks: element i of
// tensor `id` is kept iff a stateless hash of (seed, id, i) clears p; the backward pass recomputes it.
__device__ __forceinline__ bool drop_keep(unsigned long long seed, unsigned id, unsigned long long i, float p)
{
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)id + 1) + i * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.f / 16777216.f) >= p;     // 24 uniform bits
}
// out = base + dropout(x) (base may be null): the residual adds after self-attention and the MLP
__global__ __launch_bounds__(256) void dropout_add_kernel(const float *base, const float *x, long n, float p,
                                                          unsigned long long seed, unsigned id, float *out)
{
    const float k = 1.f / (1.f - p);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = drop_keep(seed, id, i, p) ? x[i] * k : 0.f;
        out[i] = base ? base[i] + v : v;
    }
}
__global__ __launch_bounds__(256) void dropout_mask_kernel(long n, float p, unsigned long long seed, unsigned id,
                                                           unsigned char *mask)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        mask[i] = drop_keep(seed, id, i, p) ? 1 : 0;
}

// nn.MultiheadAttention over the T <= 16 views of a sample with src_key_padding_mask = ~valid
// (adapter.py:97-99): one 64-thread block per (sample, head).  qkv [B*T, 3d]; P [B, heads, T, T].
constexpr int AD_MAXT = 16;
__global__ __launch_bounds__(64) void adapter_attn_fwd_kernel(const float *qkv, const unsigned char *valid, int T,
                                                              int d, int heads, float *P, float *O, float drop_p,
                                                              unsigned long long seed, unsigned drop_id)
{
    __shared__ float sp[AD_MAXT][AD_MAXT];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, hd = d / heads;
    const float scale = 1.f / __builtin_sqrtf((float)hd);
    const float *base = qkv + (long)b * T * 3 * d + h * hd;
    for (int i = threadIdx.x; i < T * T; i += 64) {
        const int t = i / T, j = i % T;
        float s = 0.f;
        for (int c = 0; c < hd; c++) s += base[(long)t * 3 * d + c] * base[(long)j * 3 * d + d + c];
        sp[t][j] = valid[b * T + j] ? s * scale : -INFINITY;
    }
    __syncthreads();
    if (threadIdx.x < T) {
        const int t = threadIdx.x;
        float mx = -INFINITY, se = 0.f;
        for (int j = 0; j < T; j++) mx = fmaxf(mx, sp[t][j]);
        for (int j = 0; j < T; j++) se += __expf(sp[t][j] - mx);
        for (int j = 0; j < T; j++) {
            const float p = __expf(sp[t][j] - mx) / se;
            const long pi = (((long)b * heads + h) * T + t) * T + j;
            P[pi] = p;                                   // the softmax output (its backward needs it undropped)
            // MultiheadAttention's dropout on the attention weights
            sp[t][j] = drop_p > 0.f ? (drop_keep(seed, drop_id, pi, drop_p) ? p / (1.f - drop_p) : 0.f) : p;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T * hd; i += 64) {
        const int t = i / hd, c = i % hd;
        float o = 0.f;
        for (int j = 0; j < T; j++) o += sp[t][j] * base[(long)j * 3 * d + 2 * d + c];
        O[((long)b * T + t) * d + h * hd + c] = o;
    }
}

__global__ __launch_bounds__(64) void adapter_attn_bwd_kernel(const float *qkv, const float *P, const float *dO,
                                                              int T, int d, int heads, float *dqkv, float drop_p,
                                                              unsigned long long seed, unsigned drop_id)
{
    __shared__ float sp[AD_MAXT][AD_MAXT], ds[AD_MAXT][AD_MAXT], sk[AD_MAXT][AD_MAXT];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads, hd = d / heads;
    const float scale = 1.f / __builtin_sqrtf((float)hd);
    const float *base = qkv + (long)b * T * 3 * d + h * hd;
    const float *dob = dO + (long)b * T * d + h * hd;
    float *dq = dqkv + (long)b * T * 3 * d + h * hd;
    for (int i = threadIdx.x; i < T * T; i += 64) {
        const int t = i / T, j = i % T;
        const long pi = (((long)b * heads + h) * T + t) * T + j;
        sp[t][j] = P[pi];
        // keep-scale of the attention-weight dropout: P_drop = P * sk
        sk[t][j] = drop_p > 0.f ? (drop_keep(seed, drop_id, pi, drop_p) ? 1.f / (1.f - drop_p) : 0.f) : 1.f;
        float dp = 0.f;
        for (int c = 0; c < hd; c++) dp += dob[(long)t * d + c] * base[(long)j * 3 * d + 2 * d + c];
        ds[t][j] = dp * sk[t][j];                        // dP (through the dropout) for now
    }
    __syncthreads();
    if (threadIdx.x < T) {
        const int t = threadIdx.x;
        float dot = 0.f;
        for (int j = 0; j < T; j++) dot += sp[t][j] * ds[t][j];
        for (int j = 0; j < T; j++) ds[t][j] = sp[t][j] * (ds[t][j] - dot) * scale;   // dS (scaled)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T * hd; i += 64) {
        const int t = i / hd, c = i % hd;
        float gq = 0.f, gk = 0.f, gv = 0.f;
        for (int j = 0; j < T; j++) {
            gq += ds[t][j] * base[(long)j * 3 * d + d + c];        // dQ[t] = sum_j dS[t, j] K[j]
            gk += ds[j][t] * base[(long)j * 3 * d + c];            // dK[t] = sum_j dS[j, t] Q[j]
            gv += sp[j][t] * sk[j][t] * dob[(long)j * d + c];      // dV[t] = sum_j P_drop[j, t] dO[j]
        }
        dq[(long)t * 3 * d + c] = gq;
        dq[(long)t * 3 * d + d + c] = gk;
        dq[(long)t * 3 * d + 2 * d + c] = gv;
    }
}

// out = a * x + b * y (y may be null)
__global__ __launch_bounds__(256) void axpby_kernel(const float *x, const float *y, long n, float a, float b, float *out)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = a * x[i] + (y ? b * y[i] : 0.f);
}
// g[i] = f[i] > 0 ? g[i] * scale : 0: backward of dropout(ReLU(.)) on the saved, already dropped
// post-activation (a dropped or clamped element is 0 there; scale = 1 / (1 - p))
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float *f, long n, float scale, float *g)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        g[i] = f[i] > 0.f ? g[i] * scale : 0.f;
}
// through F.normalize + the validity mask (clip_cls.py:325-329): dm = valid ? (dfn - fn (fn . dfn)) / |m| : 0,
// scaled by `scale` (the (1 - residual) of Adapter.residual_add on the way to out_proj).
// row_idx (optional): mixed / dmixed are compact rows, view r lives in row row_idx[r]; only the rows that a valid view
// names are written (the caller clears dmixed first).  valid == nullptr: valid iff row_idx names one of the n_rows rows.
// normalize == 0: the forward only gathered and masked, dm = valid ? dfn * scale : 0.
// scalars (optional): the device step_scalars array, scalars[EC_STEP_GRAD_SCALE] replaces scale.
__global__ __launch_bounds__(256) void normalize_bwd_kernel(const float *mixed, const float *fn, const float *dfn,
                                                            const unsigned char *valid, const int *row_idx, int n_rows,
                                                            int normalize, int R, int D, float scale,
                                                            const float *scalars, float *dmixed)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;
    if (scalars) scale = scalars[EC_STEP_GRAD_SCALE];
    const int ri = row_idx ? row_idx[r] : r;
    const bool ok = valid ? valid[r] != 0 : (ri >= 0 && ri < n_rows);
    if (row_idx && !ok) return;
    const long mr = row_idx ? (long)ri : (long)r;
    float s = 0.f, dot = 0.f;
    for (int j = lane; j < D; j += 64) {
        const float m = mixed[mr * D + j];
        s += m * m, dot += fn[(long)r * D + j] * dfn[(long)r * D + j];
    }
    float inv = ok ? scale / fmaxf(__builtin_sqrtf(wave_sum(s)), 1e-12f) : 0.f;
    dot = wave_sum(dot);
    if (!normalize) inv = ok ? scale : 0.f, dot = 0.f;
    for (int j = lane; j < D; j += 64)
        dmixed[mr * D + j] = (dfn[(long)r * D + j] - fn[(long)r * D + j] * dot) * inv;
}

// The three upstream gradients of ec_classify_v2's outputs folded into dZ = d loss / d full_logits [B, T, K]; one
// workgroup per sample.  A null upstream gradient is zero.  Valid view v, class k:
//   dZ = d_full                                                        identity
//      + d_logits | d_logits / n_valid | d_logits on the maximal view   _aggregate_logits (clip_cls.py:104-121); max: over
//                                                                      l - 1e6 [invalid], the lowest index on a tie
//      + p (d_probs - <d_probs, p>) / n_valid,  p = softmax_k(full[v]) _aggregate_probs (:123-129)
// Invalid views get zero: their logits are the constant 0 of the scatter (:151-152).
__global__ __launch_bounds__(TR_THREADS) void classify_dz_kernel(const float *full, const int *row_idx, int n_rows, int T,
                                                                 int K, int agg, const float *d_full,
                                                                 const float *d_logits, const float *d_probs, float *dZ)
{
    __shared__ float vmax[AD_MAXT], vsum[AD_MAXT], vdot[AD_MAXT];
    __shared__ int ok[AD_MAXT];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < T) {
        const int r = row_idx[b * T + threadIdx.x];
        ok[threadIdx.x] = r >= 0 && r < n_rows;
    }
    __syncthreads();
    float nv = 0.f;
    for (int v = 0; v < T; v++) nv += ok[v] ? 1.f : 0.f;
    const float *fl = full + (long)b * T * K;
    if (d_probs) {
        const float *g = d_probs + (long)b * K;
        for (int v = wave; v < T; v += TR_WAVES) {       // a wave per view: its softmax statistics and <g, p>
            if (!ok[v]) continue;
            float mx = -INFINITY;
            for (int k = lane; k < K; k += 64) mx = fmaxf(mx, fl[(long)v * K + k]);
            mx = wave_max(mx);
            float se = 0.f, dot = 0.f;
            for (int k = lane; k < K; k += 64) {
                const float e = expf(fl[(long)v * K + k] - mx);
                se += e, dot += g[k] * e;
            }
            se = wave_sum(se), dot = wave_sum(dot);
            if (lane == 0) vmax[v] = mx, vsum[v] = se, vdot[v] = dot / se;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += TR_THREADS) {
        const float gl = d_logits ? d_logits[(long)b * K + k] : 0.f;
        const float gp = d_probs ? d_probs[(long)b * K + k] : 0.f;
        int amax = -1;
        if (d_logits && agg == EC_AGG_MAX) {
            float best = -INFINITY;
            for (int v = 0; v < T; v++) {
                const float l = fl[(long)v * K + k] - (ok[v] ? 0.f : 1.f) * 1e6f;
                if (l > best) best = l, amax = v;
            }
        }
        for (int v = 0; v < T; v++) {
            float z = 0.f;
            if (ok[v]) {
                if (d_full) z = d_full[((long)b * T + v) * K + k];
                if (d_logits) z += agg == EC_AGG_SUM ? gl : (agg == EC_AGG_MEAN ? gl / nv : (v == amax ? gl : 0.f));
                if (d_probs) z += expf(fl[(long)v * K + k] - vmax[v]) / vsum[v] * (gp - vdot[v]) / nv;
            }
            dZ[((long)b * T + v) * K + k] = z;
        }
    }
}

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// Hands out the fp32 buffers of a workspace in call order, each 256-byte aligned; on a null base it only counts bytes.
struct Carve {
    unsigned char *p;
    size_t off;
    float *f(size_t n)
    {
        float *r = p ? reinterpret_cast<float *>(p + off) : nullptr;
        off += align256(n * 4);
        return r;
    }
};

// The loss head's buffers: carve_head puts them at the front of every fused step's workspace.
struct HeadBufs {
    float *Fn, *dL, *u, *dU, *inv_norm, *loss_b;
};
void carve_head(Carve &c, int B, int T, int D, int K, HeadBufs &h)
{
    const size_t R = (size_t)B * T;
    h.Fn = c.f(R * D), h.dL = c.f(R * K), h.u = c.f((size_t)K * D), h.dU = c.f((size_t)K * D);
    h.inv_norm = c.f(K), h.loss_b = c.f(B);
}

// The loss head on feats [B * T, D]: loss, grad_text, agg_logits (optional); h.Fn (normalised views), h.dL (per-view
// logit gradients) and h.u (normalised text) stay behind for the caller's own backward.
// row_idx (optional, int32 [B, T]): feats holds only the valid views, row_idx[b, v] = the row of view (b, v)
int head_launches(hipStream_t s, const char *who, const float *feats, const int *row_idx, const unsigned char *valid,
                  const int *labels, const float *text_param, int B, int T, int D, int K, float logit_scale, int agg,
                  int use_probs_loss, const HeadBufs &h, float *loss, float *grad_text, float *agg_logits)
{
    const size_t lds = ((size_t)T * K + TR_WAVES + 3 * (size_t)T) * 4;
    EC_REQUIRE(lds <= 160 * 1024, "%s: T * K = %d floats exceed the LDS", who, T * K);
    if (lds > 64 * 1024)
        if (int rc = ec::ensure_dynamic_lds(reinterpret_cast<const void *>(fs_loss_grad_kernel), 160 * 1024)) return rc;
    const int R = B * T;
    hipLaunchKernelGGL(text_norm_kernel, dim3(K), dim3(64), 0, s, text_param, D, h.u, h.inv_norm);
    hipLaunchKernelGGL(fs_normalize_kernel, dim3((unsigned)((R + TR_WAVES - 1) / TR_WAVES)), dim3(TR_THREADS), 0, s, feats, valid,
                       row_idx, 0, 1, R, D, h.Fn);
    // full_logits [R, K] = logit_scale * Fn u^T, into the dL rows
    hipLaunchKernelGGL(sgemm_kernel<false>, dim3((K + 63) / 64, (unsigned)((R + 63) / 64)), dim3(256), 0, s, h.Fn, (long)D, 1L, h.u,
                       1L, (long)D, R, K, D, logit_scale, 0.f, static_cast<const float *>(nullptr), h.dL, (long)K);
    hipLaunchKernelGGL(fs_loss_grad_kernel, dim3(B), dim3(TR_THREADS), lds, s, valid, labels, B, T, K, agg, use_probs_loss, h.dL,
                       h.loss_b, agg_logits);
    // dU[K, D] = logit_scale * dL^T Fn: the reduction runs over the R view rows
    hipLaunchKernelGGL(sgemm_kernel<false>, dim3((D + 63) / 64, (K + 63) / 64), dim3(256), 0, s, h.dL, 1L, (long)K, h.Fn, (long)D,
                       1L, K, D, R, logit_scale, 0.f, static_cast<const float *>(nullptr), h.dU, (long)D);
    hipLaunchKernelGGL(text_grad_finish_kernel, dim3(K), dim3(64), 0, s, h.u, h.dU, h.inv_norm, D, h.loss_b, B,
                       grad_text, loss);
    return EC_OK;
}

}  // namespace

extern "C" EC_API size_t ec_fs_text_train_workspace_bytes(int B, int T, int D, int K)
{
    if (B <= 0 || T <= 0 || D <= 0 || K <= 0) return 0;
    Carve c{nullptr, 0};
    HeadBufs h;
    carve_head(c, B, T, D, K, h);
    return c.off;
}

extern "C" EC_API int ec_fs_text_loss_grad(const float *img_feats, const uint8_t *valid, const int32_t *labels,
                                           const float *text_param, int B, int T, int D, int K,
                                           float logit_scale, int agg, int use_probs_loss, float *loss,
                                           float *grad_text, float *agg_logits, void *workspace,
                                           size_t workspace_bytes, ec_stream_t stream)
{
    EC_REQUIRE(B > 0 && T > 0 && D > 0 && K > 0, "ec_fs_text_loss_grad: bad shape");
    EC_REQUIRE(agg == EC_AGG_SUM || agg == EC_AGG_MEAN || agg == EC_AGG_MAX, "ec_fs_text_loss_grad: unknown agg %d", agg);
    EC_REQUIRE(img_feats && valid && labels && text_param && loss && grad_text && workspace,
               "ec_fs_text_loss_grad: null buffer");
    Carve c{static_cast<unsigned char *>(workspace), 0};
    HeadBufs h;
    carve_head(c, B, T, D, K, h);
    EC_REQUIRE(workspace_bytes >= c.off, "ec_fs_text_loss_grad: workspace too small");
    if (int rc = head_launches(static_cast<hipStream_t>(stream), "ec_fs_text_loss_grad", img_feats, nullptr, valid, labels,
                               text_param, B, T, D, K, logit_scale, agg, use_probs_loss, h, loss, grad_text, agg_logits))
        return rc;
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

// The fine-tuning head (models/clip_cls_ft.py:196-256): ec_fs_text_loss_grad on features that may be compact over the
// valid views, plus grad_img = grad_scale * d loss / d img_feats in the features' own layout.  dFn lives behind the
// head's buffers; with a null grad_text the unused text gradient is written there first.
extern "C" EC_API int ec_ft_loss_grad(const float *img_feats, const int32_t *row_idx, const uint8_t *valid,
                                      const int32_t *labels, const float *text_param, int B, int T, int D, int K,
                                      float logit_scale, int agg, int use_probs_loss, float grad_scale,
                                      const float *step_scalars, float *loss, float *grad_text, float *grad_img,
                                      float *agg_logits, void *workspace, size_t workspace_bytes, ec_stream_t stream)
{
    EC_REQUIRE(B > 0 && T > 0 && D > 0 && K > 0, "ec_ft_loss_grad: bad shape");
    EC_REQUIRE(agg == EC_AGG_SUM || agg == EC_AGG_MEAN || agg == EC_AGG_MAX, "ec_ft_loss_grad: unknown agg %d", agg);
    EC_REQUIRE(img_feats && valid && labels && text_param && loss && grad_img && workspace, "ec_ft_loss_grad: null buffer");
    Carve c{static_cast<unsigned char *>(workspace), 0};
    HeadBufs h;
    carve_head(c, B, T, D, K, h);
    const size_t R = (size_t)B * T, n_dfn = (R > (size_t)K ? R : (size_t)K) * D;
    EC_REQUIRE(workspace_bytes >= c.off + n_dfn * 4, "ec_ft_loss_grad: workspace too small");
    float *dfn = c.f(n_dfn);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = head_launches(s, "ec_ft_loss_grad", img_feats, row_idx, valid, labels, text_param, B, T, D, K, logit_scale,
                               agg, use_probs_loss, h, loss, grad_text ? grad_text : dfn, agg_logits))
        return rc;
    // dFn[R, D] = logit_scale * dL[R, K] . u[K, D]
    if (int rc = ec_sgemm(h.dL, K, 1, h.u, D, 1, (int)R, D, K, logit_scale, 0.f, dfn, D, stream)) return rc;
    hipLaunchKernelGGL(normalize_bwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, img_feats, h.Fn, dfn, valid,
                       row_idx, 0, 1, (int)R, D, grad_scale, step_scalars, grad_img);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

extern "C" EC_API int ec_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                   int64_t n, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int step, ec_stream_t stream)
{
    EC_REQUIRE(n >= 0 && step >= 1, "ec_adam_step: n=%lld step=%d", (long long)n, step);
    if (n == 0) return EC_OK;
    EC_REQUIRE(param && grad && exp_avg && exp_avg_sq, "ec_adam_step: null buffer");
    const double bc1 = 1.0 - __builtin_pow((double)beta1, (double)step);
    const double bc2 = 1.0 - __builtin_pow((double)beta2, (double)step);
    const long blocks = (n + 255) / 256;
    ec::ProfScope prof(ec::PROF_OPTIMIZER, static_cast<hipStream_t>(stream), 0, 28.0 * n);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), param, grad, exp_avg, exp_avg_sq, (long)n, lr, beta1,
                       beta2, eps, weight_decay, (float)bc1, (float)__builtin_sqrt(bc2));
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

// ---------------------------------------------------------------------------------------------------
// 'text-trans': TransformerAdapter (models/adapter.py:52-110, norm_first or not) + text_feats.  Layer-wise over all
// R = B * T view rows: every nn.Linear is one sgemm_kernel launch (x W^T forward, dy W and dy^T x
// backward), the saved activations live in the workspace.  dropout_p = 0 is the deterministic function the
// eval-mode module computes, the one the golden gradients differentiate; dropout_p > 0 adds the four train-mode
// dropouts of nn.TransformerEncoderLayer from a stateless hash.  The adapter's forward and backward are written once
// (adapter_train_fwd_launches / adapter_train_bwd_launches): ec_fs_trans_loss_grad runs them around its loss head,
// ec_adapter_train_forward / _backward run them as two calls over a caller-owned tape (torch autograd), and
// ec_classify_backward is the classifier tail's backward for an arbitrary upstream gradient.
// ---------------------------------------------------------------------------------------------------
namespace {

struct LayerBufs {
    float *xhat1, *rstd1, *a, *qkv, *P, *o, *h1, *xhat2, *rstd2, *bn, *f;
};

// What the adapter's forward leaves for its backward (hfin and the layers' saved activations) and its own scratch
// (h0, y, ftmp): the backward half only reads it.
struct AdapterTape {
    float *h0, *hfin, *y, *ftmp;
    LayerBufs L[8];
};
// Everything the adapter's backward overwrites.  dy = d loss / d out_proj's output on entry.
struct AdapterScratch {
    float *dy, *dh, *dh1, *dtmp_d, *dqkv, *df;
};

struct TransBufs {
    float *mixed, *dfn;
    AdapterTape tape;
    AdapterScratch bw;
    HeadBufs head;
};

void carve_tape(Carve &c, int B, int T, int D, int d, int ffn, int heads, int layers, AdapterTape &t)
{
    const size_t R = (size_t)B * T;
    t.h0 = c.f(R * d), t.hfin = c.f(R * d), t.y = c.f(R * D), t.ftmp = c.f(R * d);
    for (int l = 0; l < layers; l++) {
        LayerBufs &b = t.L[l];
        b.xhat1 = c.f(R * d), b.rstd1 = c.f(R), b.a = c.f(R * d), b.qkv = c.f(R * 3 * d);
        b.P = c.f((size_t)B * heads * T * T), b.o = c.f(R * d), b.h1 = c.f(R * d), b.xhat2 = c.f(R * d);
        b.rstd2 = c.f(R), b.bn = c.f(R * d), b.f = c.f(R * ffn);
    }
}
void carve_scratch(Carve &c, int B, int T, int D, int d, int ffn, AdapterScratch &t)
{
    const size_t R = (size_t)B * T;
    t.dy = c.f(R * D), t.dh = c.f(R * d), t.dh1 = c.f(R * d), t.dtmp_d = c.f(R * d), t.dqkv = c.f(R * 3 * d);
    t.df = c.f(R * ffn);
}

size_t carve_trans(Carve &c, int B, int T, int D, int K, int d, int ffn, int heads, int layers, TransBufs &t)
{
    const size_t R = (size_t)B * T;
    carve_head(c, B, T, D, K, t.head);
    t.mixed = c.f(R * D), t.dfn = c.f(R * D);
    carve_tape(c, B, T, D, d, ffn, heads, layers, t.tape);
    carve_scratch(c, B, T, D, d, ffn, t.bw);
    return c.off;
}

void gemm(hipStream_t s, bool relu, const float *A, long sam, long sak, const float *Bm, long sbk, long sbn, int M,
          int N, int K, float alpha, float beta, const float *bias, float *C)
{
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    if (relu)
        hipLaunchKernelGGL(sgemm_kernel<true>, grid, dim3(256), 0, s, A, sam, sak, Bm, sbk, sbn, M, N, K, alpha, beta,
                           bias, C, (long)N);
    else
        hipLaunchKernelGGL(sgemm_kernel<false>, grid, dim3(256), 0, s, A, sam, sak, Bm, sbk, sbn, M, N, K, alpha, beta,
                           bias, C, (long)N);
}
// y[R, out] = x[R, in] W[out, in]^T + b (+ beta * y)
void linear_fwd(hipStream_t s, const float *x, const float *W, const float *b, int R, int in, int out, float *y,
                float beta = 0.f, bool relu = false)
{
    gemm(s, relu, x, in, 1, W, 1, in, R, out, in, 1.f, beta, b, y);
}
// dx[R, in] = dy[R, out] W (+ beta dx);  dW[out, in] = dy^T x;  db[out] = colsum(dy).  A null output is skipped.
void linear_bwd(hipStream_t s, const float *x, const float *W, const float *dy, int R, int in, int out, float *dx,
                float dx_beta, float *dW, float *db)
{
    if (dx) gemm(s, false, dy, out, 1, W, in, 1, R, in, out, 1.f, dx_beta, nullptr, dx);
    if (dW) gemm(s, false, dy, 1, out, x, in, 1, out, in, R, 1.f, 0.f, nullptr, dW);
    if (db) hipLaunchKernelGGL(colsum_kernel, dim3((out + 63) / 64), dim3(256), 0, s, dy, (const float *)nullptr, R, out, db);
}
// d gamma[j] = sum_r dy[r, j] xhat[r, j], d beta[j] = sum_r dy[r, j]; a null output is skipped
void ln_param_bwd(hipStream_t s, const float *dy, const float *xhat, int R, int d, float *dg, float *db)
{
    if (dg) hipLaunchKernelGGL(colsum_kernel, dim3((d + 63) / 64), dim3(256), 0, s, dy, xhat, R, d, dg);
    if (db) hipLaunchKernelGGL(colsum_kernel, dim3((d + 63) / 64), dim3(256), 0, s, dy, (const float *)nullptr, R, d, db);
}
unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

bool adapter_geometry_ok(const ec_adapter_train_params *w, int T)
{
    return w->in_dim > 0 && w->d_model > 0 && w->d_model <= 1024 && w->ffn_dim > 0 && w->heads > 0 &&
           w->d_model % w->heads == 0 && w->layers >= 1 && w->layers <= 8 && T <= AD_MAXT &&
           (w->post_norm == 0 || w->post_norm == 1);
}

// dropout sites of layer l (nn.TransformerEncoderLayer, either layout): 4 l + {0 attention weights,
// 1 dropout1 after out_proj, 2 dropout inside the MLP, 3 dropout2 after linear2}
//
// w->post_norm picks the layer's layout; both are launch sequences over the same kernels, tape slots and scratch:
//   pre-LN   h1 = h + drop1(out_proj(attn(in_proj(norm1(h))))),  h' = h1 + drop2(linear2(drop(relu(linear1(norm2(h1))))))
//   post-LN  a = norm1(h + drop1(out_proj(attn(in_proj(h))))),   h' = norm2(a + drop2(linear2(drop(relu(linear1(a))))))
// Post-LN keeps norm1's input in h1, norm1's output in a (linear1's input and the second residual base), norm2's output
// in bn (the next layer's input; the last layer's also in hfin); norm2's input passes through hfin and is not kept.  Its
// backward takes norm2's gradients from the layer's output gradient alone (no residual skips the norm), then linear2,
// ReLU, linear1, d a = d f W1 + d s2, norm1, out_proj, attention, and in_proj_weight's gradient against the layer's INPUT
// (h0, or the previous layer's bn), d h = d qkv Wqkv + d s1.

// What every launch of one adapter pass shares.
struct AdapterRun {
    hipStream_t s;
    int B, T, R, d, ffn, heads;
    float dp;
    unsigned long long seed;
};

void copy(hipStream_t s, const float *x, long n, float *out)
{
    hipLaunchKernelGGL(axpby_kernel, dim3(blocks_for(n)), dim3(256), 0, s, x, (const float *)nullptr, n, 1.f, 0.f, out);
}
// out = base + dropout(x) at dropout site `site` (base may be null)
void dropout_add(const AdapterRun &a, unsigned site, const float *base, const float *x, long n, float *out)
{
    hipLaunchKernelGGL(dropout_add_kernel, dim3(blocks_for(n)), dim3(256), 0, a.s, base, x, n, a.dp, a.seed, site, out);
}
void layer_norm_fwd(const AdapterRun &a, const float *x, const float *g, const float *b, float *y, float *xhat, float *rstd)
{
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)((a.R + 3) / 4)), dim3(256), 0, a.s, x, g, b, a.R, a.d, y, xhat, rstd);
}
// dst = base + dropout(linear(x)): through ftmp with dropout, else a copy of base and the linear accumulating onto it
void residual_linear_fwd(const AdapterRun &a, unsigned site, const float *x, const float *W, const float *bias, int in,
                         const float *base, float *ftmp, float *dst)
{
    if (a.dp > 0.f) {
        linear_fwd(a.s, x, W, bias, a.R, in, a.d, ftmp);
        dropout_add(a, site, base, ftmp, (long)a.R * a.d, dst);
    } else {
        copy(a.s, base, (long)a.R * a.d, dst);
        linear_fwd(a.s, x, W, bias, a.R, in, a.d, dst, 1.f);
    }
}
// b.h1 = base + dropout1(out_proj(attn(in_proj(x))))
void attn_branch_fwd(const AdapterRun &a, int l, const ec_adapter_train_layer &p, const LayerBufs &b,
                     const unsigned char *valid, const float *x, const float *base, float *ftmp)
{
    linear_fwd(a.s, x, p.qkv_w, p.qkv_b, a.R, a.d, 3 * a.d, b.qkv);
    hipLaunchKernelGGL(adapter_attn_fwd_kernel, dim3(a.B * a.heads), dim3(64), 0, a.s, b.qkv, valid, a.T, a.d, a.heads, b.P,
                       b.o, a.dp, a.seed, (unsigned)(4 * l));
    residual_linear_fwd(a, 4 * l + 1, b.o, p.o_w, p.o_b, a.d, base, ftmp, b.h1);
}
// dst = base + dropout2(linear2(dropout(relu(linear1(x))))), the dropped post-activation kept in b.f
void mlp_branch_fwd(const AdapterRun &a, int l, const ec_adapter_train_layer &p, const LayerBufs &b, const float *x,
                    const float *base, float *ftmp, float *dst)
{
    linear_fwd(a.s, x, p.w1, p.b1, a.R, a.d, a.ffn, b.f, 0.f, true);
    if (a.dp > 0.f) dropout_add(a, 4 * l + 2, nullptr, b.f, (long)a.R * a.ffn, b.f);
    residual_linear_fwd(a, 4 * l + 3, b.f, p.w2, p.b2, a.ffn, base, ftmp, dst);
}

// The adapter's forward (adapter.py:82-105) over all R = B * T view rows, saving what the backward reads:
// mixed [R, D] = r img_feats + (1 - r) out_proj(encoder(in_proj(img_feats))).  The one launch sequence behind
// ec_fs_trans_loss_grad and ec_adapter_train_forward.
void adapter_train_fwd_launches(hipStream_t s, const float *img_feats, const unsigned char *valid, int B, int T,
                                const ec_adapter_train_params *w, float dp, unsigned long long seed, AdapterTape &t,
                                float *mixed)
{
    const AdapterRun a{s, B, T, B * T, w->d_model, w->ffn_dim, w->heads, dp, seed};
    const int D = w->in_dim, d = a.d, R = a.R;
    const float r = w->residual;
    linear_fwd(s, img_feats, w->in_w, w->in_b, R, D, d, t.h0);
    const float *h = t.h0;
    for (int l = 0; l < w->layers; l++) {
        const ec_adapter_train_layer &p = w->blocks[l];
        const LayerBufs &b = t.L[l];
        if (w->post_norm) {
            attn_branch_fwd(a, l, p, b, valid, h, h, t.ftmp);
            layer_norm_fwd(a, b.h1, p.ln1_g, p.ln1_b, b.a, b.xhat1, b.rstd1);
            mlp_branch_fwd(a, l, p, b, b.a, b.a, t.ftmp, t.hfin);      // s2 lives in hfin until norm2 has read it
            layer_norm_fwd(a, t.hfin, p.ln2_g, p.ln2_b, b.bn, b.xhat2, b.rstd2);
            h = b.bn;
            if (l == w->layers - 1) {   // out_proj (and its backward) read the encoder's output from hfin, as pre-LN
                copy(s, b.bn, (long)R * d, t.hfin);
                h = t.hfin;
            }
        } else {
            layer_norm_fwd(a, h, p.ln1_g, p.ln1_b, b.a, b.xhat1, b.rstd1);
            attn_branch_fwd(a, l, p, b, valid, b.a, h, t.ftmp);
            layer_norm_fwd(a, b.h1, p.ln2_g, p.ln2_b, b.bn, b.xhat2, b.rstd2);
            mlp_branch_fwd(a, l, p, b, b.bn, b.h1, t.ftmp, t.hfin);
            h = t.hfin;      // this layer's input is dead (ln_1 consumed it, h1 took its copy): reuse its slot
        }
    }
    linear_fwd(s, h, w->out_w, w->out_b, R, d, D, t.y);
    hipLaunchKernelGGL(axpby_kernel, dim3(blocks_for((long)R * D)), dim3(256), 0, s, img_feats, t.y, (long)R * D, r,
                       1.f - r, mixed);                                             // Adapter.residual_add
}

// The gradient below a residual branch's dropout: dsum itself without dropout, else masked and rescaled into tmp.
const float *dropout_bwd(const AdapterRun &a, unsigned site, const float *dsum, float *tmp)
{
    if (a.dp <= 0.f) return dsum;
    dropout_add(a, site, nullptr, dsum, (long)a.R * a.d, tmp);
    return tmp;
}
// Backward of mlp_branch_fwd's branch from dsum = d loss / d its residual sum: linear2, ReLU, linear1 with x the
// tape slot linear1 read; dx = dx_beta * dx + d f W1.
void mlp_branch_bwd(const AdapterRun &a, int l, const ec_adapter_train_layer &p, const ec_adapter_train_layer &q,
                    const LayerBufs &b, const AdapterScratch &x, const float *dsum, const float *lin1_in, float *dx,
                    float dx_beta)
{
    const float *dlin2 = dropout_bwd(a, 4 * l + 3, dsum, x.dtmp_d);
    linear_bwd(a.s, b.f, p.w2, dlin2, a.R, a.ffn, a.d, x.df, 0.f, q.w2, q.b2);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks_for((long)a.R * a.ffn)), dim3(256), 0, a.s, b.f, (long)a.R * a.ffn,
                       1.f / (1.f - a.dp), x.df);
    linear_bwd(a.s, lin1_in, p.w1, x.df, a.R, a.d, a.ffn, dx, dx_beta, q.w1, q.b1);
}
// Backward of attn_branch_fwd's branch from dsum = d loss / d its residual sum (its dropout undone into `undo`):
// out_proj, attention, in_proj with qkv_in the slot in_proj read; dx = dx_beta * dx + d qkv Wqkv.
void attn_branch_bwd(const AdapterRun &a, int l, const ec_adapter_train_layer &p, const ec_adapter_train_layer &q,
                     const LayerBufs &b, const AdapterScratch &x, const float *dsum, float *undo, const float *qkv_in,
                     float *dx, float dx_beta)
{
    const float *dlin_o = dropout_bwd(a, 4 * l + 1, dsum, undo);
    linear_bwd(a.s, b.o, p.o_w, dlin_o, a.R, a.d, a.d, x.dtmp_d, 0.f, q.o_w, q.o_b);
    hipLaunchKernelGGL(adapter_attn_bwd_kernel, dim3(a.B * a.heads), dim3(64), 0, a.s, b.qkv, b.P, x.dtmp_d, a.T, a.d,
                       a.heads, x.dqkv, a.dp, a.seed, (unsigned)(4 * l));
    linear_bwd(a.s, qkv_in, p.qkv_w, x.dqkv, a.R, a.d, 3 * a.d, dx, dx_beta, q.qkv_w, q.qkv_b);
}
// LayerNorm's backward from dy: its parameter gradients, then dx = (skip, the gradient of a residual around the
// norm, copied in first) + the norm's input gradient.
void layer_norm_bwd(const AdapterRun &a, const float *dy, const float *xhat, const float *rstd, const float *g, float *dg,
                    float *db, const float *skip, float *dx)
{
    ln_param_bwd(a.s, dy, xhat, a.R, a.d, dg, db);
    if (skip) copy(a.s, skip, (long)a.R * a.d, dx);
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)((a.R + 3) / 4)), dim3(256), 0, a.s, dy, xhat, rstd, g, a.R, a.d, dx,
                       skip ? 1 : 0);
}

// The adapter's backward from x.dy = d loss / d out_proj's output: every non-null gradient of g, and (d_img non-null)
// d_img = d_img_beta * d_img + d h0 in_proj.weight.  Reads the tape, writes only x and the gradients.  The one launch
// sequence behind ec_fs_trans_loss_grad and ec_adapter_train_backward.
void adapter_train_bwd_launches(hipStream_t s, const float *img_feats, int B, int T, const ec_adapter_train_params *w,
                                const ec_adapter_train_params *g, float dp, unsigned long long seed,
                                const AdapterTape &t, const AdapterScratch &x, float *d_img, float d_img_beta)
{
    const AdapterRun a{s, B, T, B * T, w->d_model, w->ffn_dim, w->heads, dp, seed};
    const int D = w->in_dim, d = a.d, R = a.R;
    linear_bwd(s, t.hfin, w->out_w, x.dy, R, d, D, x.dh, 0.f, g->out_w, g->out_b);
    for (int l = w->layers - 1; l >= 0; l--) {
        // x.dh = d loss / d the layer's output on entry, d loss / d the layer's input on exit
        const ec_adapter_train_layer &p = w->blocks[l];
        const ec_adapter_train_layer &q = g->blocks[l];
        const LayerBufs &b = t.L[l];
        if (w->post_norm) {
            // bn = norm2(s2): nothing skips norm2, so its input gradient is d s2 alone
            layer_norm_bwd(a, x.dh, b.xhat2, b.rstd2, p.ln2_g, q.ln2_g, q.ln2_b, nullptr, x.dh1);
            mlp_branch_bwd(a, l, p, q, b, x, x.dh1, b.a, x.dh1, 1.f);                  // d a = d f W1 + d s2
            layer_norm_bwd(a, x.dh1, b.xhat1, b.rstd1, p.ln1_g, q.ln1_g, q.ln1_b, nullptr, x.dh);
            // x.dh = d s1, the residual's share of d h; d a is consumed, dh1 takes the undone dropout
            attn_branch_bwd(a, l, p, q, b, x, x.dh, x.dh1, l ? t.L[l - 1].bn : t.h0, x.dh, 1.f);   // d h = d qkv Wqkv + d s1
        } else {
            mlp_branch_bwd(a, l, p, q, b, x, x.dh, b.bn, x.dtmp_d, 0.f);
            layer_norm_bwd(a, x.dtmp_d, b.xhat2, b.rstd2, p.ln2_g, q.ln2_g, q.ln2_b, x.dh, x.dh1);
            // dh takes the undone dropout: it is rebuilt from dh1 below
            attn_branch_bwd(a, l, p, q, b, x, x.dh1, x.dh, b.a, x.dtmp_d, 0.f);
            layer_norm_bwd(a, x.dtmp_d, b.xhat1, b.rstd1, p.ln1_g, q.ln1_g, q.ln1_b, x.dh1, x.dh);
        }
    }
    linear_bwd(s, img_feats, w->in_w, x.dh, R, D, d, d_img, d_img_beta, g->in_w, g->in_b);
}

}  // namespace

extern "C" EC_API size_t ec_fs_trans_train_workspace_bytes(int B, int T, int D, int K, int d_model, int ffn_dim,
                                                           int heads, int layers)
{
    if (B <= 0 || T <= 0 || D <= 0 || K <= 0 || d_model <= 0 || ffn_dim <= 0 || layers <= 0 || layers > 8) return 0;
    Carve c{nullptr, 0};
    TransBufs t;
    return carve_trans(c, B, T, D, K, d_model, ffn_dim, heads, layers, t);
}

extern "C" EC_API int ec_fs_trans_loss_grad(const float *img_feats, const uint8_t *valid, const int32_t *labels,
                                            const float *text_param, int B, int T, int D, int K, float logit_scale,
                                            int agg, int use_probs_loss, const ec_adapter_train_params *w,
                                            const ec_adapter_train_params *g, float dropout_p,
                                            uint64_t dropout_seed, float *loss, float *grad_text,
                                            float *agg_logits, void *workspace, size_t workspace_bytes,
                                            ec_stream_t stream)
{
    EC_REQUIRE(B > 0 && T > 0 && D > 0 && K > 0, "ec_fs_trans_loss_grad: bad shape");
    EC_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "ec_fs_trans_loss_grad: dropout_p=%g", (double)dropout_p);
    EC_REQUIRE(w && g && w->blocks && g->blocks, "ec_fs_trans_loss_grad: null parameter / gradient structs");
    EC_REQUIRE(agg == EC_AGG_SUM || agg == EC_AGG_MEAN || agg == EC_AGG_MAX, "ec_fs_trans_loss_grad: unknown agg %d", agg);
    const int d = w->d_model, ffn = w->ffn_dim, heads = w->heads, layers = w->layers;
    EC_REQUIRE(w->in_dim == D && adapter_geometry_ok(w, T),
               "ec_fs_trans_loss_grad: unsupported adapter geometry (T <= %d, layers <= 8)", AD_MAXT);
    EC_REQUIRE(img_feats && valid && labels && text_param && loss && grad_text && workspace,
               "ec_fs_trans_loss_grad: null buffer");
    Carve c{static_cast<unsigned char *>(workspace), 0};
    TransBufs t;
    const size_t need = carve_trans(c, B, T, D, K, d, ffn, heads, layers, t);
    if (need > workspace_bytes)
        return ec::fail(EC_ERR_WORKSPACE, "ec_fs_trans_loss_grad: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int R = B * T;
    const float r = w->residual;

    adapter_train_fwd_launches(s, img_feats, valid, B, T, w, dropout_p, dropout_seed, t.tape, t.mixed);
    if (int rc = head_launches(s, "ec_fs_trans_loss_grad", t.mixed, nullptr, valid, labels, text_param, B, T, D, K,
                               logit_scale, agg, use_probs_loss, t.head, loss, grad_text, agg_logits))
        return rc;

    // ---------------- backward into the adapter ----------------
    gemm(s, false, t.head.dL, K, 1, t.head.u, D, 1, R, D, K, logit_scale, 0.f, nullptr, t.dfn);   // dFn = s dL u
    hipLaunchKernelGGL(normalize_bwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, t.mixed, t.head.Fn, t.dfn, valid,
                       (const int *)nullptr, 0, 1, R, D, 1.f - r, (const float *)nullptr, t.bw.dy);   // dY = (1 - r) dMixed
    adapter_train_bwd_launches(s, img_feats, B, T, w, g, dropout_p, dropout_seed, t.tape, t.bw, nullptr, 0.f);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

// ---- the same forward and backward as two calls over a caller-owned tape (torch autograd) ----
extern "C" EC_API size_t ec_adapter_train_tape_bytes(int B, int T, int D, int d_model, int ffn_dim, int heads, int layers)
{
    if (B <= 0 || T <= 0 || D <= 0 || d_model <= 0 || ffn_dim <= 0 || heads <= 0 || layers <= 0 || layers > 8) return 0;
    Carve c{nullptr, 0};
    AdapterTape t;
    carve_tape(c, B, T, D, d_model, ffn_dim, heads, layers, t);
    return c.off;
}

extern "C" EC_API size_t ec_adapter_train_backward_workspace_bytes(int B, int T, int D, int d_model, int ffn_dim)
{
    if (B <= 0 || T <= 0 || D <= 0 || d_model <= 0 || ffn_dim <= 0) return 0;
    Carve c{nullptr, 0};
    AdapterScratch x;
    carve_scratch(c, B, T, D, d_model, ffn_dim, x);
    return c.off;
}

// The offsets come from carve_tape / carve_scratch themselves, run on a sentinel base address (a null base would hand
// out null pointers): the two cannot drift apart.
extern "C" EC_API int ec_adapter_train_layout(int B, int T, int D, int d_model, int ffn_dim, int heads, int layers,
                                              int64_t *tape_offsets, int n_tape, int64_t *scratch_offsets, int n_scratch)
{
    EC_REQUIRE(B > 0 && T > 0 && D > 0 && d_model > 0 && ffn_dim > 0 && heads > 0 && layers >= 1 && layers <= 8,
               "ec_adapter_train_layout: bad geometry (B %d T %d layers %d)", B, T, layers);
    const int need = EC_AT_LAYER0 + EC_AT_PER_LAYER * layers;
    if (tape_offsets) {
        EC_REQUIRE(n_tape >= need, "ec_adapter_train_layout: %d tape slots for %d", n_tape, need);
        unsigned char *const sentinel = reinterpret_cast<unsigned char *>(uintptr_t(1) << 40);
        auto off = [&](const void *p) { return (int64_t)(static_cast<const unsigned char *>(p) - sentinel); };
        Carve c{sentinel, 0};
        AdapterTape t;
        carve_tape(c, B, T, D, d_model, ffn_dim, heads, layers, t);
        tape_offsets[EC_AT_H0] = off(t.h0), tape_offsets[EC_AT_HFIN] = off(t.hfin), tape_offsets[EC_AT_Y] = off(t.y);
        tape_offsets[EC_AT_FTMP] = off(t.ftmp);
        for (int l = 0; l < layers; l++) {
            int64_t *o = tape_offsets + EC_AT_LAYER0 + EC_AT_PER_LAYER * l;
            const LayerBufs &b = t.L[l];
            o[EC_AT_L_XHAT1] = off(b.xhat1), o[EC_AT_L_RSTD1] = off(b.rstd1), o[EC_AT_L_A] = off(b.a);
            o[EC_AT_L_QKV] = off(b.qkv), o[EC_AT_L_P] = off(b.P), o[EC_AT_L_O] = off(b.o), o[EC_AT_L_H1] = off(b.h1);
            o[EC_AT_L_XHAT2] = off(b.xhat2), o[EC_AT_L_RSTD2] = off(b.rstd2), o[EC_AT_L_BN] = off(b.bn);
            o[EC_AT_L_F] = off(b.f);
        }
    }
    if (scratch_offsets) {
        EC_REQUIRE(n_scratch >= EC_AS_COUNT, "ec_adapter_train_layout: %d scratch slots for %d", n_scratch, EC_AS_COUNT);
        unsigned char *const sentinel = reinterpret_cast<unsigned char *>(uintptr_t(1) << 40);
        auto off = [&](const void *p) { return (int64_t)(static_cast<const unsigned char *>(p) - sentinel); };
        Carve c{sentinel, 0};
        AdapterScratch x;
        carve_scratch(c, B, T, D, d_model, ffn_dim, x);
        scratch_offsets[EC_AS_DY] = off(x.dy), scratch_offsets[EC_AS_DH] = off(x.dh), scratch_offsets[EC_AS_DH1] = off(x.dh1);
        scratch_offsets[EC_AS_DTMP_D] = off(x.dtmp_d), scratch_offsets[EC_AS_DQKV] = off(x.dqkv);
        scratch_offsets[EC_AS_DF] = off(x.df);
    }
    return need;
}

extern "C" EC_API int ec_adapter_train_forward(const float *img_feats, const uint8_t *valid, int B, int T,
                                               const ec_adapter_train_params *w, float dropout_p,
                                               uint64_t dropout_seed, float *out, void *tape, size_t tape_bytes,
                                               ec_stream_t stream)
{
    EC_REQUIRE(B > 0 && T > 0, "ec_adapter_train_forward: bad shape B=%d T=%d", B, T);
    EC_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "ec_adapter_train_forward: dropout_p=%g", (double)dropout_p);
    EC_REQUIRE(w && w->blocks, "ec_adapter_train_forward: null parameter struct");
    EC_REQUIRE(adapter_geometry_ok(w, T), "ec_adapter_train_forward: unsupported adapter geometry (T <= %d, layers <= 8)",
               AD_MAXT);
    EC_REQUIRE(img_feats && valid && out && tape, "ec_adapter_train_forward: null buffer");
    Carve c{static_cast<unsigned char *>(tape), 0};
    AdapterTape t;
    carve_tape(c, B, T, w->in_dim, w->d_model, w->ffn_dim, w->heads, w->layers, t);
    if (c.off > tape_bytes)
        return ec::fail(EC_ERR_WORKSPACE, "ec_adapter_train_forward: tape %zu < %zu bytes", tape_bytes, c.off);
    adapter_train_fwd_launches(static_cast<hipStream_t>(stream), img_feats, valid, B, T, w, dropout_p, dropout_seed, t, out);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

extern "C" EC_API int ec_adapter_train_backward(const float *img_feats, int B, int T, const ec_adapter_train_params *w,
                                                float dropout_p, uint64_t dropout_seed, const void *tape,
                                                size_t tape_bytes, const float *d_out,
                                                const ec_adapter_train_params *g, float *d_img_feats, void *workspace,
                                                size_t workspace_bytes, ec_stream_t stream)
{
    EC_REQUIRE(B > 0 && T > 0, "ec_adapter_train_backward: bad shape B=%d T=%d", B, T);
    EC_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "ec_adapter_train_backward: dropout_p=%g", (double)dropout_p);
    EC_REQUIRE(w && g && w->blocks && g->blocks, "ec_adapter_train_backward: null parameter / gradient structs");
    EC_REQUIRE(adapter_geometry_ok(w, T), "ec_adapter_train_backward: unsupported adapter geometry (T <= %d, layers <= 8)",
               AD_MAXT);
    EC_REQUIRE(img_feats && tape && d_out && workspace, "ec_adapter_train_backward: null buffer");
    const int D = w->in_dim, R = B * T;
    Carve ct{static_cast<unsigned char *>(const_cast<void *>(tape)), 0};
    AdapterTape t;
    carve_tape(ct, B, T, D, w->d_model, w->ffn_dim, w->heads, w->layers, t);
    if (ct.off > tape_bytes)
        return ec::fail(EC_ERR_WORKSPACE, "ec_adapter_train_backward: tape %zu < %zu bytes", tape_bytes, ct.off);
    Carve cx{static_cast<unsigned char *>(workspace), 0};
    AdapterScratch x;
    carve_scratch(cx, B, T, D, w->d_model, w->ffn_dim, x);
    if (cx.off > workspace_bytes)
        return ec::fail(EC_ERR_WORKSPACE, "ec_adapter_train_backward: workspace %zu < %zu bytes", workspace_bytes, cx.off);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float r = w->residual;
    // out = r img_feats + (1 - r) y (Adapter.residual_add): dY = (1 - r) d_out, d_img_feats = r d_out + (through in_proj)
    hipLaunchKernelGGL(axpby_kernel, dim3(blocks_for((long)R * D)), dim3(256), 0, s, d_out, (const float *)nullptr,
                       (long)R * D, 1.f - r, 0.f, x.dy);
    if (d_img_feats)
        hipLaunchKernelGGL(axpby_kernel, dim3(blocks_for((long)R * D)), dim3(256), 0, s, d_out, (const float *)nullptr,
                           (long)R * D, r, 0.f, d_img_feats);
    adapter_train_bwd_launches(s, img_feats, B, T, w, g, dropout_p, dropout_seed, t, x, d_img_feats, 1.f);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

// ---- the VJP of ec_classify_v2 (csrc/classify.hip) with respect to feats and text_t ----
extern "C" EC_API size_t ec_classify_backward_workspace_bytes(int B, int T, int C, int K)
{
    if (B <= 0 || T <= 0 || C <= 0 || K <= 0) return 0;
    const size_t R = (size_t)B * T;
    return 2 * align256(R * C * 4) + align256(R * K * 4);
}

extern "C" EC_API int ec_classify_backward(const float *feats, int n_rows, const int32_t *row_idx, const float *text_t,
                                           int B, int T, int C, int K, float logit_scale, int agg, int normalize,
                                           const float *full_logits, const float *d_full_logits, const float *d_logits,
                                           const float *d_probs, float *d_feats, float *d_text_t, void *workspace,
                                           size_t workspace_bytes, ec_stream_t stream)
{
    EC_REQUIRE(B >= 0 && T > 0 && T <= AD_MAXT && C > 0 && C % 4 == 0 && K >= 2 && n_rows >= 0,
               "ec_classify_backward: bad shape n_rows=%d B=%d T=%d C=%d K=%d (T <= %d, C a multiple of 4, K >= 2)", n_rows,
               B, T, C, K, AD_MAXT);
    EC_REQUIRE(agg == EC_AGG_SUM || agg == EC_AGG_MEAN || agg == EC_AGG_MAX, "ec_classify_backward: unknown agg %d", agg);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // rows of feats that no valid view names keep a zero gradient: normalize_bwd_kernel writes the others
    if (d_feats && n_rows > 0) EC_CHECK_HIP(hipMemsetAsync(d_feats, 0, (size_t)n_rows * C * 4, s));
    if (B == 0 || n_rows == 0) {
        if (d_text_t) EC_CHECK_HIP(hipMemsetAsync(d_text_t, 0, (size_t)C * K * 4, s));
        return EC_OK;
    }
    EC_REQUIRE(feats && row_idx && text_t && full_logits && workspace, "ec_classify_backward: null buffer");
    const size_t need = ec_classify_backward_workspace_bytes(B, T, C, K);
    if (workspace_bytes < need)
        return ec::fail(EC_ERR_WORKSPACE, "ec_classify_backward: workspace %zu < %zu bytes", workspace_bytes, need);
    const int R = B * T;
    Carve c{static_cast<unsigned char *>(workspace), 0};
    float *Fn = c.f((size_t)R * C), *dFn = c.f((size_t)R * C), *dZ = c.f((size_t)R * K);
    hipLaunchKernelGGL(classify_dz_kernel, dim3(B), dim3(TR_THREADS), 0, s, full_logits, row_idx, n_rows, T, K, agg,
                       d_full_logits, d_logits, d_probs, dZ);
    hipLaunchKernelGGL(fs_normalize_kernel, dim3((unsigned)((R + TR_WAVES - 1) / TR_WAVES)), dim3(TR_THREADS), 0, s, feats,
                       (const unsigned char *)nullptr, row_idx, n_rows, normalize, R, C, Fn);
    if (d_text_t)       // d text_t [C, K] = scale Fn^T dZ: the reduction runs over the R view rows
        gemm(s, false, Fn, 1, C, dZ, K, 1, C, K, R, logit_scale, 0.f, nullptr, d_text_t);
    if (d_feats) {
        gemm(s, false, dZ, K, 1, text_t, 1, K, R, C, K, logit_scale, 0.f, nullptr, dFn);   // dFn = scale dZ text
        hipLaunchKernelGGL(normalize_bwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, feats, Fn, dFn,
                           (const unsigned char *)nullptr, row_idx, n_rows, normalize, R, C, 1.f, (const float *)nullptr,
                           d_feats);
    }
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

extern "C" EC_API int ec_sgemm(const float *A, long sam, long sak, const float *B, long sbk, long sbn, int M, int N,
                               int K, float alpha, float beta, float *C, long ldc, ec_stream_t stream)
{
    EC_REQUIRE(M >= 0 && N >= 0 && K >= 0 && ldc >= N, "ec_sgemm: bad shape %d x %d x %d (ldc %ld)", M, N, K, ldc);
    if (M == 0 || N == 0) return EC_OK;
    EC_REQUIRE(A && B && C, "ec_sgemm: null buffer");
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    ec::ProfScope prof(ec::PROF_SGEMM, static_cast<hipStream_t>(stream), 2.0 * M * N * K, 0);
    hipLaunchKernelGGL(sgemm_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), A, sam, sak, B, sbk,
                       sbn, M, N, K, alpha, beta, (const float *)nullptr, C, ldc);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

extern "C" EC_API int ec_dropout_mask(uint64_t seed, uint32_t site, int64_t n, float p, uint8_t *mask,
                                      ec_stream_t stream)
{
    EC_REQUIRE(n >= 0 && p >= 0.f && p < 1.f, "ec_dropout_mask: n=%lld p=%g", (long long)n, (double)p);
    if (n == 0) return EC_OK;
    EC_REQUIRE(mask, "ec_dropout_mask: null buffer");
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks_for((long)n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (long)n, p, (unsigned long long)seed, (unsigned)site, mask);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}
