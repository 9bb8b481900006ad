// The split-precision ("precise") form of the ResNet CLIP image tower's kernels (csrc/resnet.hip holds the 16-bit ones and
// the tower driver): activations and weights travel as two f16 planes,
//     hi = f16(v),   lo = f16((v - hi) * 2^11),
// so that v ~ hi + lo * 2^-11 to 2^-22 |v| + 2^-36.  The lo plane is scaled by 2^11 (as LoShift does for the LoRA coefficient
// planes of csrc/vit_train.hip): it then has the exponent range of hi and stays a normal f16 number wherever hi is one --
// unscaled, the lo part of a weight of 0.02 (a 1x1 convolution over 2048 channels) would sit in f16's subnormal range and
// carry 5 bits instead of 11.
//
// The convolution runs its K loop three times over the same LDS tiles and into the same fp32 accumulators, the way
// gemm.hip's split GEMM walks [a_lo | a_hi | a_hi] . [w_hi | w_lo | w_hi] by offsetting the operand pointers per segment:
//     acc  = x_lo . w_hi + x_hi . w_lo      (both carry the factor 2^11)
//     acc *= 2^-11                          (exact)
//     acc += x_hi . w_hi
// lo . lo (2^-22 of the result) is dropped.  LDS (36 KiB) and registers are those of conv_igemm_kernel; staging and
// MFMAs triple.  Everything between the convolutions is fp32.  f16 only.
#include "common.h"
#include "mfma.h"
#include "rowops.h"

namespace ec {
namespace {

constexpr int CB_M = 128, CB_N = 128, CB_K = 64, CB_LD = CB_K + 8;   // as conv_igemm_kernel
constexpr float LO_UP = 2048.f, LO_DOWN = 1.f / 2048.f;

__device__ __forceinline__ float join_hl(_Float16 hi, _Float16 lo) { return (float)hi + (float)lo * LO_DOWN; }
__device__ __forceinline__ void split_hl(float v, _Float16 &hi, _Float16 &lo)   // mfma.h's split16 with lo scaled up
{
    hi = (_Float16)v;
    lo = (_Float16)((v - (float)hi) * LO_UP);
}

// conv_igemm_kernel's tiling and operand order (256 threads = 2 x 2 waves of 64 x 64; first MFMA operand the weight tile, so a
// lane's accumulator holds 4 consecutive channels of one pixel), with three K segments.
template <int KS>
__global__ __launch_bounds__(256) void conv_igemm_hl_kernel(const _Float16 *__restrict__ x_hi, const _Float16 *__restrict__ x_lo,
                                                            const _Float16 *__restrict__ w_hi, const _Float16 *__restrict__ w_lo,
                                                            const float *__restrict__ scale, const float *__restrict__ bias,
                                                            const _Float16 *__restrict__ resid_hi,
                                                            const _Float16 *__restrict__ resid_lo, void *__restrict__ out,
                                                            _Float16 *__restrict__ out_lo, int M, int H, int W, int Cin, int Cout,
                                                            int relu, int out32)
{
    typedef _Float16 E;
    typedef f16x8 V8;
    __shared__ __attribute__((aligned(16))) E As[CB_M * CB_LD];
    __shared__ __attribute__((aligned(16))) E Ws[CB_N * CB_LD];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m0 = blockIdx.x * CB_M, n0 = blockIdx.y * CB_N;
    const long K = (long)KS * KS * Cin;
    const int cpt = Cin / CB_K, nkt = KS * KS * cpt;
    const int chunk = tid & 7, r0 = tid >> 3;   // staging: 16 bytes of rows r0 + 32 i

    int pn[4], py[4], px[4];
    bool pm[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = m0 + r0 + 32 * i;
        pm[i] = m < M;
        if (KS == 1) {
            pn[i] = m, py[i] = 0, px[i] = 0;
        } else {
            const int hw = H * W, mm = pm[i] ? m : 0;
            pn[i] = mm / hw;
            py[i] = (mm % hw) / W;
            px[i] = mm % W;
        }
    }

    uint4 ra[4], rw[4];
    // segment 0: x_lo . w_hi, 1: x_hi . w_lo, 2: x_hi . w_hi; kt counts the K tiles of one segment
    auto load = [&](int seg, int kt) {
        const E *x = seg == 0 ? x_lo : x_hi, *w = seg == 1 ? w_lo : w_hi;
        const int tap = kt / cpt, c0 = (kt - tap * cpt) * CB_K + chunk * 8;
        const int dy = tap / KS - KS / 2, dx = tap % KS - KS / 2;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            ra[i] = make_uint4(0, 0, 0, 0);
            if (KS == 1) {
                if (pm[i]) ra[i] = *(const uint4 *)(x + (long)pn[i] * Cin + c0);
            } else {
                const int yy = py[i] + dy, xx = px[i] + dx;
                if (pm[i] && yy >= 0 && yy < H && xx >= 0 && xx < W)
                    ra[i] = *(const uint4 *)(x + (((long)pn[i] * H + yy) * W + xx) * Cin + c0);
            }
            const int n = n0 + r0 + 32 * i;
            rw[i] = n < Cout ? *(const uint4 *)(w + (long)n * K + (long)kt * CB_K + chunk * 8) : make_uint4(0, 0, 0, 0);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *(uint4 *)(As + (r0 + 32 * i) * CB_LD + chunk * 8) = ra[i];
            *(uint4 *)(Ws + (r0 + 32 * i) * CB_LD + chunk * 8) = rw[i];
        }
    };

    f32x4 acc[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wm = (wv & 1) * 64, wn = (wv >> 1) * 64;
    const int fr = lane & 15, fk = 8 * (lane >> 4);
    load(0, 0);
    for (int seg = 0; seg < 3; seg++) {
        if (seg == 2) {   // the two lo products carry 2^11
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] *= LO_DOWN;
        }
        for (int kt = 0; kt < nkt; kt++) {
            stage();
            __syncthreads();
            // the next tile's global reads overlap this tile's MFMAs
            if (kt + 1 < nkt) load(seg, kt + 1);
            else if (seg < 2) load(seg + 1, 0);
#pragma unroll
            for (int s = 0; s < CB_K; s += 32) {
                V8 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; i++) a[i] = *(const V8 *)(Ws + (wn + 16 * i + fr) * CB_LD + s + fk);
#pragma unroll
                for (int j = 0; j < 4; j++) b[j] = *(const V8 *)(As + (wm + 16 * j + fr) * CB_LD + s + fk);
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
            }
            __syncthreads();
        }
    }

#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int m = m0 + wm + 16 * j + fr;
        if (m >= M) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int n = n0 + wn + 16 * i + 4 * (lane >> 4);
            if (n >= Cout) continue;
            const long o = (long)m * Cout + n;
            float v[4];
            for (int r = 0; r < 4; r++) v[r] = scale ? acc[i][j][r] * scale[n + r] + bias[n + r] : acc[i][j][r] + bias[n + r];
            if (resid_hi) {
                const f16x4 rh = *(const f16x4 *)(resid_hi + o), rl = *(const f16x4 *)(resid_lo + o);
                for (int r = 0; r < 4; r++) v[r] += join_hl(rh[r], rl[r]);
            }
            if (relu)
                for (int r = 0; r < 4; r++) v[r] = fmaxf(v[r], 0.f);
            if (out32) {
                *(f32x4 *)((float *)out + o) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
                f16x4 h, l;
                for (int r = 0; r < 4; r++) {
                    E a, b;
                    split_hl(v[r], a, b);
                    h[r] = a, l[r] = b;
                }
                *(f16x4 *)((E *)out + o) = h;
                *(f16x4 *)(out_lo + o) = l;
            }
        }
    }
}

// Stem rows, split: pixel (n, oy, ox) of the stride-2 3x3 convolution -> two 64-wide rows, the 27 taps
// k = (ky*3 + kx)*3 + c as hi and as lo, zeros beyond; the first convolution is then the KS = 1 split product over them
// (x_hi w_hi + x_lo w_hi + x_hi w_lo).  Input modes and normalisation as stem_rows_kernel.
__global__ __launch_bounds__(256) void stem_rows_hl_kernel(const void *__restrict__ in, int mode, int N, int R,
                                                           _Float16 *__restrict__ rows_hi, _Float16 *__restrict__ rows_lo)
{
    const int Ro = R / 2;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long)N * Ro * Ro) return;
    const int n = (int)(p / ((long)Ro * Ro)), oy = (int)(p / Ro % Ro), ox = (int)(p % Ro);
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    float f[27];
#pragma unroll
    for (int ky = 0; ky < 3; ky++)
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
            const int iy = 2 * oy + ky - 1, ix = 2 * ox + kx - 1;
            const bool ok = iy >= 0 && iy < R && ix >= 0 && ix < R;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float v = 0.f;
                if (ok) {
                    if (mode == EC_PRE_HWC_U8) {
                        const uint8_t u = ((const uint8_t *)in)[(((long)n * R + iy) * R + ix) * 3 + c];
                        v = __fdiv_rn(__fdiv_rn((float)u, 255.0f) - mean[c], stdv[c]);   // IEEE-rounded, as the host LUT
                    } else {
                        v = ((const float *)in)[(((long)n * 3 + c) * R + iy) * R + ix];
                    }
                }
                f[(ky * 3 + kx) * 3 + c] = v;
            }
        }
    f16x8 *dh = (f16x8 *)(rows_hi + p * 64), *dl = (f16x8 *)(rows_lo + p * 64);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        f16x8 h, l;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int k = 8 * q + j;
            _Float16 a = (_Float16)0.f, b = (_Float16)0.f;
            if (k < 27) split_hl(f[k], a, b);
            h[j] = a, l[j] = b;
        }
        dh[q] = h;
        dl[q] = l;
    }
}

// AvgPool2d(2) on split activations: fp32 sum of the four joined values, split store.  8 channels a thread.
__global__ __launch_bounds__(256) void avgpool2_hl_kernel(const _Float16 *__restrict__ x_hi, const _Float16 *__restrict__ x_lo,
                                                          int N, int H, int W, int C, _Float16 *__restrict__ y_hi,
                                                          _Float16 *__restrict__ y_lo)
{
    const int Ho = H / 2, Wo = W / 2, c8 = C / 8;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)N * Ho * Wo * c8) return;
    const int c = (int)(t % c8) * 8;
    const long p = t / c8;
    const int ox = (int)(p % Wo), oy = (int)(p / Wo % Ho);
    const long n = p / ((long)Wo * Ho);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < 2; dy++)
        for (int dx = 0; dx < 2; dx++) {
            const long o = ((n * H + 2 * oy + dy) * W + 2 * ox + dx) * C + c;
            const f16x8 a = *(const f16x8 *)(x_hi + o), b = *(const f16x8 *)(x_lo + o);
            for (int j = 0; j < 8; j++) s[j] += join_hl(a[j], b[j]);
        }
    f16x8 h, l;
    for (int j = 0; j < 8; j++) {
        _Float16 a, b;
        split_hl(0.25f * s[j], a, b);
        h[j] = a, l[j] = b;
    }
    *(f16x8 *)(y_hi + p * C + c) = h;
    *(f16x8 *)(y_lo + p * C + c) = l;
}

// Attention-pool tokens on split activations: tokens = [mean_HW(x); x] + pos in fp32, split store; token 0 again in q_in.
__global__ __launch_bounds__(256) void attnpool_tokens_hl_kernel(const _Float16 *__restrict__ x_hi,
                                                                 const _Float16 *__restrict__ x_lo, int HW, int C,
                                                                 const float *__restrict__ pos, _Float16 *__restrict__ tok_hi,
                                                                 _Float16 *__restrict__ tok_lo, _Float16 *__restrict__ q_hi,
                                                                 _Float16 *__restrict__ q_lo)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long n = blockIdx.y;
    const long xo = n * HW * C + c, to = n * (HW + 1) * C + c;
    float s = 0.f;
    _Float16 a, b;
    for (int p = 0; p < HW; p++) {
        const float v = join_hl(x_hi[xo + (long)p * C], x_lo[xo + (long)p * C]);
        s += v;
        split_hl(v + pos[(long)(p + 1) * C + c], a, b);
        tok_hi[to + (long)(p + 1) * C] = a;
        tok_lo[to + (long)(p + 1) * C] = b;
    }
    split_hl(s / (float)HW + pos[c], a, b);
    tok_hi[to] = a, tok_lo[to] = b;
    q_hi[n * C + c] = a, q_lo[n * C + c] = b;
}

// attnpool_attend_kernel on split q and kv: one query per (image, head), fp32 throughout, split store.
__global__ __launch_bounds__(64) void attnpool_attend_hl_kernel(const _Float16 *__restrict__ q_hi, const _Float16 *__restrict__ q_lo,
                                                                const _Float16 *__restrict__ kv_hi,
                                                                const _Float16 *__restrict__ kv_lo, int L, int C,
                                                                _Float16 *__restrict__ out_hi, _Float16 *__restrict__ out_lo)
{
    __shared__ float qs[64];
    __shared__ float ps[256];
    const int d = threadIdx.x, h = blockIdx.x;
    const long n = blockIdx.y;
    qs[d] = join_hl(q_hi[n * C + h * 64 + d], q_lo[n * C + h * 64 + d]) * 0.125f;
    __syncthreads();
    const long kb = n * L * 2 * C + h * 64;
    float mx = -INFINITY;
    for (int t = d; t < L; t += 64) {
        float s = 0.f;
        const long kr = kb + (long)t * 2 * C;
        for (int j = 0; j < 64; j += 8) {
            const f16x8 k8 = *(const f16x8 *)(kv_hi + kr + j), l8 = *(const f16x8 *)(kv_lo + kr + j);
            for (int u = 0; u < 8; u++) s += qs[j + u] * join_hl(k8[u], l8[u]);
        }
        ps[t] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int t = d; t < L; t += 64) {
        const float e = __expf(ps[t] - mx);
        ps[t] = e;
        sum += e;
    }
    // (rowops.h's wave_sum, written out: through the call this kernel's scalar code comes out in another order)
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    __syncthreads();
    const long vb = kb + C + d;
    float acc = 0.f;
    for (int t = 0; t < L; t++) acc += ps[t] * join_hl(kv_hi[vb + (long)t * 2 * C], kv_lo[vb + (long)t * 2 * C]);
    _Float16 a, b;
    split_hl(acc / sum, a, b);
    out_hi[n * C + h * 64 + d] = a;
    out_lo[n * C + h * 64 + d] = b;
}

}  // namespace
}  // namespace ec

using namespace ec;

EC_API int ec_resnet_conv_hl(const void *x_hi, const void *x_lo, int n_img, int H, int W, int Cin, int Cout, int ks,
                             const void *w_hi, const void *w_lo, const float *scale, const float *bias, const void *resid_hi,
                             const void *resid_lo, int relu, void *out, void *out_lo, int out32, int dtype, ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && H > 0 && W > 0, "ec_resnet_conv_hl: n_img=%d H=%d W=%d", n_img, H, W);
    EC_REQUIRE(ks == 1 || ks == 3, "ec_resnet_conv_hl: ks=%d (1 or 3)", ks);
    EC_REQUIRE(Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0,
               "ec_resnet_conv_hl: Cin=%d Cout=%d must be positive multiples of 64 (pad channels at pack time)", Cin, Cout);
    EC_REQUIRE(dtype == EC_F16, "ec_resnet_conv_hl: dtype=%d (the split form is f16 only)", dtype);
    EC_REQUIRE(!(out32 && resid_hi), "ec_resnet_conv_hl: the residual epilogue stores hi + lo");
    EC_REQUIRE(!resid_hi == !resid_lo, "ec_resnet_conv_hl: the residual needs both planes or neither");
    const long M = (long)n_img * H * W;
    EC_REQUIRE(M < (1L << 31), "ec_resnet_conv_hl: %ld pixel rows (chunk the batch)", M);
    if (M == 0) return EC_OK;
    EC_REQUIRE(x_hi && x_lo && w_hi && w_lo && bias && out && (out32 || out_lo), "ec_resnet_conv_hl: null buffer");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)ceil_div(M, (long)CB_M), (unsigned)ceil_div(Cout, CB_N));
    const double flops = 3 * 2.0 * M * Cout * ks * ks * Cin;
    const double bytes = 4.0 * (M * Cin + (double)Cout * ks * ks * Cin + M * Cout * (resid_hi ? 2 : 1));
    ProfScope prof(ks == 3 ? PROF_CONV3X3 : PROF_CONV1X1, s, flops, bytes);
#define EC_CONV_HL_LAUNCH(KS)                                                                                      \
    conv_igemm_hl_kernel<KS><<<grid, 256, 0, s>>>((const _Float16 *)x_hi, (const _Float16 *)x_lo,                  \
                                                  (const _Float16 *)w_hi, (const _Float16 *)w_lo, scale, bias,     \
                                                  (const _Float16 *)resid_hi, (const _Float16 *)resid_lo, out,     \
                                                  (_Float16 *)out_lo, (int)M, H, W, Cin, Cout, relu, out32)
    if (ks == 3) EC_CONV_HL_LAUNCH(3);
    else EC_CONV_HL_LAUNCH(1);
#undef EC_CONV_HL_LAUNCH
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_stem_rows_hl(const void *input, int input_mode, int n_img, int R, void *rows_hi, void *rows_lo,
                                  int dtype, ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && R > 0 && R % 2 == 0, "ec_resnet_stem_rows_hl: n_img=%d R=%d (even)", n_img, R);
    EC_REQUIRE(input_mode == EC_PRE_CHW_F32 || input_mode == EC_PRE_HWC_U8,
               "ec_resnet_stem_rows_hl: input_mode=%d (EC_PRE_CHW_F32 or EC_PRE_HWC_U8)", input_mode);
    EC_REQUIRE(dtype == EC_F16, "ec_resnet_stem_rows_hl: dtype=%d (the split form is f16 only)", dtype);
    const long P = (long)n_img * (R / 2) * (R / 2);
    if (P == 0) return EC_OK;
    EC_REQUIRE(input && rows_hi && rows_lo, "ec_resnet_stem_rows_hl: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const double in_bytes = (double)n_img * 3 * R * R * (input_mode == EC_PRE_HWC_U8 ? 1 : 4);
    ProfScope prof(PROF_STEM, s, 0.0, in_bytes + 256.0 * P);
    stem_rows_hl_kernel<<<(unsigned)ceil_div(P, 256L), 256, 0, s>>>(input, input_mode, n_img, R, (_Float16 *)rows_hi,
                                                                    (_Float16 *)rows_lo);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_avgpool_hl(const void *x_hi, const void *x_lo, int n_img, int H, int W, int C, void *y_hi, void *y_lo,
                                int dtype, ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0,
               "ec_resnet_avgpool_hl: n_img=%d H=%d W=%d C=%d (C a multiple of 8)", n_img, H, W, C);
    EC_REQUIRE(dtype == EC_F16, "ec_resnet_avgpool_hl: dtype=%d (the split form is f16 only)", dtype);
    const long T = (long)n_img * (H / 2) * (W / 2) * (C / 8);
    if (T == 0) return EC_OK;
    EC_REQUIRE(x_hi && x_lo && y_hi && y_lo, "ec_resnet_avgpool_hl: null buffer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_AVGPOOL, s, 0.0, 4.0 * n_img * C * ((double)H * W + (H / 2) * (W / 2)));
    avgpool2_hl_kernel<<<(unsigned)ceil_div(T, 256L), 256, 0, s>>>((const _Float16 *)x_hi, (const _Float16 *)x_lo, n_img, H,
                                                                   W, C, (_Float16 *)y_hi, (_Float16 *)y_lo);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_attnpool_tokens_hl(const void *x_hi, const void *x_lo, int n_img, int HW, int C, const float *pos,
                                        void *tokens_hi, void *tokens_lo, void *q_in_hi, void *q_in_lo, int dtype,
                                        ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && HW > 0 && C > 0, "ec_resnet_attnpool_tokens_hl: n_img=%d HW=%d C=%d", n_img, HW, C);
    EC_REQUIRE(dtype == EC_F16, "ec_resnet_attnpool_tokens_hl: dtype=%d (the split form is f16 only)", dtype);
    EC_REQUIRE(n_img < 65536, "ec_resnet_attnpool_tokens_hl: n_img=%d (chunk the batch)", n_img);
    if (n_img == 0) return EC_OK;
    EC_REQUIRE(x_hi && x_lo && pos && tokens_hi && tokens_lo && q_in_hi && q_in_lo, "ec_resnet_attnpool_tokens_hl: null buffer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_ATTNPOOL, s, 0.0, 4.0 * n_img * C * (2.0 * HW + 2));
    dim3 grid((unsigned)ceil_div(C, 256), (unsigned)n_img);
    attnpool_tokens_hl_kernel<<<grid, 256, 0, s>>>((const _Float16 *)x_hi, (const _Float16 *)x_lo, HW, C, pos,
                                                   (_Float16 *)tokens_hi, (_Float16 *)tokens_lo, (_Float16 *)q_in_hi,
                                                   (_Float16 *)q_in_lo);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_attnpool_attend_hl(const void *q_hi, const void *q_lo, const void *kv_hi, const void *kv_lo, int n_img,
                                        int L, int C, void *out_hi, void *out_lo, int dtype, ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && L > 0 && L <= 256 && C > 0 && C % 64 == 0,
               "ec_resnet_attnpool_attend_hl: n_img=%d L=%d (<= 256) C=%d (heads of 64)", n_img, L, C);
    EC_REQUIRE(dtype == EC_F16, "ec_resnet_attnpool_attend_hl: dtype=%d (the split form is f16 only)", dtype);
    EC_REQUIRE(n_img < 65536, "ec_resnet_attnpool_attend_hl: n_img=%d (chunk the batch)", n_img);
    if (n_img == 0) return EC_OK;
    EC_REQUIRE(q_hi && q_lo && kv_hi && kv_lo && out_hi && out_lo, "ec_resnet_attnpool_attend_hl: null buffer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_ATTNPOOL, s, 4.0 * n_img * L * C, 4.0 * n_img * C * (2.0 * L + 2));
    dim3 grid((unsigned)(C / 64), (unsigned)n_img);
    attnpool_attend_hl_kernel<<<grid, 64, 0, s>>>((const _Float16 *)q_hi, (const _Float16 *)q_lo, (const _Float16 *)kv_hi,
                                                  (const _Float16 *)kv_lo, L, C, (_Float16 *)out_hi, (_Float16 *)out_lo);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}
