// ResNet CLIP image tower (OpenAI ModifiedResNet): implicit-GEMM convolutions on MFMA, the stem's
// stride-2 rows, 2x2 average pooling and the attention pool, NHWC 16-bit activations throughout.
//
// The convolution kernel is its own kernel and not an A-staging mode of ec_gemm's gemm2pp_kernel:
// gemm.hip stays untouched, so every instantiation it had keeps its ISA by construction.  It computes
// OUT[m, n] = sum_k A[m, k] W[n, k] with M = N*H*W pixels, N = Cout and K = KS*KS*Cin in tap-major
// order (a 64-wide K tile is 64 channels of one tap), stride 1, zero padding (KS-1)/2; a tap that falls
// outside the image stages zeros, so no im2col buffer exists in HBM.  1x1 convolutions and the
// attention pool's projections are the KS = 1 case (a plain row-major GEMM over pixel rows).
#include "common.h"
#include "mfma.h"
#include "rowops.h"

#include <initializer_list>

namespace ec {
namespace {

constexpr int CB_M = 128, CB_N = 128, CB_K = 64, CB_LD = CB_K + 8;   // +8 halves: rows do not share LDS banks

// 256 threads = 4 waves in a 2 x 2 grid of 64 x 64 wave tiles.  The MFMA's first operand is the weight
// tile (rows n) and its second the pixel tile (columns m), so a lane's accumulator holds 4 consecutive
// channels of one pixel: the epilogue stores 8 (16-bit) or 16 (fp32) contiguous bytes per lane.
template <int DT, int KS>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const typename T16<DT>::elem *__restrict__ x,
                                                         const typename T16<DT>::elem *__restrict__ w,
                                                         const float *__restrict__ scale,
                                                         const float *__restrict__ bias,
                                                         const typename T16<DT>::elem *__restrict__ resid,
                                                         void *__restrict__ out, int M, int H, int W, int Cin,
                                                         int Cout, int relu, int out32)
{
    typedef typename T16<DT>::elem E;
    typedef typename T16<DT>::v8 V8;
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
    auto load = [&](int kt) {
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
    load(0);
    for (int kt = 0; kt < nkt; kt++) {
        stage();
        __syncthreads();
        if (kt + 1 < nkt) load(kt + 1);   // the next tile's global reads overlap this tile's MFMAs
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
            if (resid) {
                const E *rp = resid + o;
                for (int r = 0; r < 4; r++) v[r] += (float)rp[r];
            }
            if (relu)
                for (int r = 0; r < 4; r++) v[r] = fmaxf(v[r], 0.f);
            if (out32) {
                *(f32x4 *)((float *)out + o) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
                typename T16<DT>::v4 h;
                for (int r = 0; r < 4; r++) h[r] = to16(v[r], E());
                *(typename T16<DT>::v4 *)((E *)out + o) = h;
            }
        }
    }
}

// Stem rows: pixel (n, oy, ox) of the stride-2 3x3 convolution -> 64 values: the 27 taps k = (ky*3 + kx)*3 + c
// rounded to 16 bit, in k + 27 what that rounding lost (also 16 bit), zeros beyond -- the stem weights carry the same
// 27 columns twice, so the first convolution sees the image at ~fp32 precision in the K = 64 it pays anyway.  A tap
// outside the image is 0 (the normalised image's zero padding).
// mode EC_PRE_CHW_F32: fp32 [N, 3, R, R] (normalised);  EC_PRE_HWC_U8: uint8 [N, R, R, 3], normalised here
// as the preprocess kernel does ((v / 255 - mean) / std in fp32, torch's order).
template <int DT>
__global__ __launch_bounds__(256) void stem_rows_kernel(const void *__restrict__ in, int mode, int N, int R,
                                                        typename T16<DT>::elem *__restrict__ rows)
{
    typedef typename T16<DT>::elem E;
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
    typename T16<DT>::v8 *dst = (typename T16<DT>::v8 *)(rows + p * 64);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        typename T16<DT>::v8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int k = 8 * q + j;
            o[j] = k < 27 ? to16(f[k], E()) : k < 54 ? to16(f[k - 27] - (float)to16(f[k - 27], E()), E()) : to16(0.f, E());
        }
        dst[q] = o;
    }
}

// AvgPool2d(2): NHWC [N, H, W, C] -> [N, H/2, W/2, C], fp32 sum of the four, one rounding.  8 channels a thread.
template <int DT>
__global__ __launch_bounds__(256) void avgpool2_kernel(const typename T16<DT>::elem *__restrict__ x, int N, int H,
                                                       int W, int C, typename T16<DT>::elem *__restrict__ y)
{
    typedef typename T16<DT>::elem E;
    typedef typename T16<DT>::v8 V8;
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
            const V8 a = *(const V8 *)(x + ((n * H + 2 * oy + dy) * W + 2 * ox + dx) * C + c);
            for (int j = 0; j < 8; j++) s[j] += (float)a[j];
        }
    V8 o;
    for (int j = 0; j < 8; j++) o[j] = to16(0.25f * s[j], E());
    *(V8 *)(y + p * C + c) = o;
}

// Attention-pool tokens: x NHWC [N, HW, C] -> tokens [N, HW + 1, C] = [mean_HW(x); x] + pos (fp32 math, one
// rounding), and the query row (token 0) again in q_in [N, C].
template <int DT>
__global__ __launch_bounds__(256) void attnpool_tokens_kernel(const typename T16<DT>::elem *__restrict__ x, int HW,
                                                              int C, const float *__restrict__ pos,
                                                              typename T16<DT>::elem *__restrict__ tok,
                                                              typename T16<DT>::elem *__restrict__ q_in)
{
    typedef typename T16<DT>::elem E;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long n = blockIdx.y;
    const E *xi = x + n * HW * C + c;
    E *ti = tok + n * (HW + 1) * C + c;
    float s = 0.f;
    for (int p = 0; p < HW; p++) {
        const float v = (float)xi[(long)p * C];
        s += v;
        ti[(long)(p + 1) * C] = to16(v + pos[(long)(p + 1) * C + c], E());
    }
    const E t0 = to16(s / (float)HW + pos[c], E());
    ti[0] = t0;
    q_in[n * C + c] = t0;
}

// One query per (image, head): out[n, h*64 + d] = softmax_t(q . k_t / 8) v_t[d] over the L tokens, fp32.
// q [N, C] (q_proj output), kv [N, L, 2C] (k_proj | v_proj), out [N, C] 16-bit.  One wave per (n, h).
template <int DT>
__global__ __launch_bounds__(64) void attnpool_attend_kernel(const typename T16<DT>::elem *__restrict__ q,
                                                             const typename T16<DT>::elem *__restrict__ kv, int L,
                                                             int C, typename T16<DT>::elem *__restrict__ out)
{
    typedef typename T16<DT>::elem E;
    typedef typename T16<DT>::v8 V8;
    __shared__ float qs[64];
    __shared__ float ps[256];
    const int d = threadIdx.x, h = blockIdx.x;
    const long n = blockIdx.y;
    qs[d] = (float)q[n * C + h * 64 + d] * 0.125f;
    __syncthreads();
    const E *kb = kv + n * L * 2 * C + h * 64;
    float mx = -INFINITY;
    for (int t = d; t < L; t += 64) {
        float s = 0.f;
        const E *kr = kb + (long)t * 2 * C;
        for (int j = 0; j < 64; j += 8) {
            const V8 k8 = *(const V8 *)(kr + j);
            for (int u = 0; u < 8; u++) s += qs[j + u] * (float)k8[u];
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
    sum = wave_sum(sum);
    __syncthreads();
    const E *vb = kb + C + d;
    float acc = 0.f;
    for (int t = 0; t < L; t++) acc += ps[t] * (float)vb[(long)t * 2 * C];
    out[n * C + h * 64 + d] = to16(acc / sum, E());
}

}  // namespace
}  // namespace ec

using namespace ec;

EC_API int ec_resnet_conv(const void *x, int n_img, int H, int W, int Cin, int Cout, int ks, const void *w,
                          const float *scale, const float *bias, const void *resid, int relu, void *out, int out32, int dtype,
                          ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && H > 0 && W > 0, "ec_resnet_conv: n_img=%d H=%d W=%d", n_img, H, W);
    EC_REQUIRE(ks == 1 || ks == 3, "ec_resnet_conv: ks=%d (1 or 3)", ks);
    EC_REQUIRE(Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0,
               "ec_resnet_conv: Cin=%d Cout=%d must be positive multiples of 64 (pad channels at pack time)", Cin, Cout);
    EC_REQUIRE(dtype == EC_F16 || dtype == EC_BF16, "ec_resnet_conv: dtype=%d", dtype);
    EC_REQUIRE(!(out32 && resid), "ec_resnet_conv: the residual epilogue stores 16 bit");
    const long M = (long)n_img * H * W;
    EC_REQUIRE(M < (1L << 31), "ec_resnet_conv: %ld pixel rows (chunk the batch)", M);
    if (M == 0) return EC_OK;
    EC_REQUIRE(x && w && bias && out, "ec_resnet_conv: null buffer");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)ceil_div(M, (long)CB_M), (unsigned)ceil_div(Cout, CB_N));
    const double flops = 2.0 * M * Cout * ks * ks * Cin;
    const double bytes = 2.0 * (M * Cin + (double)Cout * ks * ks * Cin + M * Cout * (resid ? 2 : 1) * (out32 ? 2 : 1));
    ProfScope prof(ks == 3 ? PROF_CONV3X3 : PROF_CONV1X1, s, flops, bytes);
#define EC_CONV_LAUNCH(DT, KS)                                                                                     \
    conv_igemm_kernel<DT, KS><<<grid, 256, 0, s>>>((const T16<DT>::elem *)x, (const T16<DT>::elem *)w, scale,    \
                                                   bias, (const T16<DT>::elem *)resid, out, (int)M, H, W, Cin,   \
                                                   Cout, relu, out32)
    if (dtype == EC_F16) {
        if (ks == 3) EC_CONV_LAUNCH(0, 3);
        else EC_CONV_LAUNCH(0, 1);
    } else {
        if (ks == 3) EC_CONV_LAUNCH(1, 3);
        else EC_CONV_LAUNCH(1, 1);
    }
#undef EC_CONV_LAUNCH
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_stem_rows(const void *input, int input_mode, int n_img, int R, void *rows, int dtype,
                               ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && R > 0 && R % 2 == 0, "ec_resnet_stem_rows: n_img=%d R=%d (even)", n_img, R);
    EC_REQUIRE(input_mode == EC_PRE_CHW_F32 || input_mode == EC_PRE_HWC_U8,
               "ec_resnet_stem_rows: input_mode=%d (EC_PRE_CHW_F32 or EC_PRE_HWC_U8)", input_mode);
    EC_REQUIRE(dtype == EC_F16 || dtype == EC_BF16, "ec_resnet_stem_rows: dtype=%d", dtype);
    const long P = (long)n_img * (R / 2) * (R / 2);
    if (P == 0) return EC_OK;
    EC_REQUIRE(input && rows, "ec_resnet_stem_rows: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const double in_bytes = (double)n_img * 3 * R * R * (input_mode == EC_PRE_HWC_U8 ? 1 : 4);
    ProfScope prof(PROF_STEM, s, 0.0, in_bytes + 128.0 * P);
    const unsigned blocks = (unsigned)ceil_div(P, 256L);
    if (dtype == EC_F16) stem_rows_kernel<0><<<blocks, 256, 0, s>>>(input, input_mode, n_img, R, (_Float16 *)rows);
    else stem_rows_kernel<1><<<blocks, 256, 0, s>>>(input, input_mode, n_img, R, (__bf16 *)rows);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_avgpool(const void *x, int n_img, int H, int W, int C, void *y, int dtype, ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0,
               "ec_resnet_avgpool: n_img=%d H=%d W=%d C=%d (C a multiple of 8)", n_img, H, W, C);
    EC_REQUIRE(dtype == EC_F16 || dtype == EC_BF16, "ec_resnet_avgpool: dtype=%d", dtype);
    const long T = (long)n_img * (H / 2) * (W / 2) * (C / 8);
    if (T == 0) return EC_OK;
    EC_REQUIRE(x && y, "ec_resnet_avgpool: null buffer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_AVGPOOL, s, 0.0, 2.0 * n_img * C * ((double)H * W + (H / 2) * (W / 2)));
    const unsigned blocks = (unsigned)ceil_div(T, 256L);
    if (dtype == EC_F16) avgpool2_kernel<0><<<blocks, 256, 0, s>>>((const _Float16 *)x, n_img, H, W, C, (_Float16 *)y);
    else avgpool2_kernel<1><<<blocks, 256, 0, s>>>((const __bf16 *)x, n_img, H, W, C, (__bf16 *)y);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_attnpool_tokens(const void *x, int n_img, int HW, int C, const float *pos, void *tokens,
                                     void *q_in, int dtype, ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && HW > 0 && C > 0, "ec_resnet_attnpool_tokens: n_img=%d HW=%d C=%d", n_img, HW, C);
    EC_REQUIRE(dtype == EC_F16 || dtype == EC_BF16, "ec_resnet_attnpool_tokens: dtype=%d", dtype);
    EC_REQUIRE(n_img < 65536, "ec_resnet_attnpool_tokens: n_img=%d (chunk the batch)", n_img);
    if (n_img == 0) return EC_OK;
    EC_REQUIRE(x && pos && tokens && q_in, "ec_resnet_attnpool_tokens: null buffer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_ATTNPOOL, s, 0.0, 2.0 * n_img * C * (2.0 * HW + 2));
    dim3 grid((unsigned)ceil_div(C, 256), (unsigned)n_img);
    if (dtype == EC_F16)
        attnpool_tokens_kernel<0><<<grid, 256, 0, s>>>((const _Float16 *)x, HW, C, pos, (_Float16 *)tokens,
                                                       (_Float16 *)q_in);
    else
        attnpool_tokens_kernel<1><<<grid, 256, 0, s>>>((const __bf16 *)x, HW, C, pos, (__bf16 *)tokens,
                                                       (__bf16 *)q_in);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

EC_API int ec_resnet_attnpool_attend(const void *q, const void *kv, int n_img, int L, int C, void *out, int dtype,
                                     ec_stream_t stream)
{
    EC_REQUIRE(n_img >= 0 && L > 0 && L <= 256 && C > 0 && C % 64 == 0,
               "ec_resnet_attnpool_attend: n_img=%d L=%d (<= 256) C=%d (heads of 64)", n_img, L, C);
    EC_REQUIRE(dtype == EC_F16 || dtype == EC_BF16, "ec_resnet_attnpool_attend: dtype=%d", dtype);
    EC_REQUIRE(n_img < 65536, "ec_resnet_attnpool_attend: n_img=%d (chunk the batch)", n_img);
    if (n_img == 0) return EC_OK;
    EC_REQUIRE(q && kv && out, "ec_resnet_attnpool_attend: null buffer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_ATTNPOOL, s, 4.0 * n_img * L * C, 2.0 * n_img * C * (2.0 * L + 2));
    dim3 grid((unsigned)(C / 64), (unsigned)n_img);
    if (dtype == EC_F16)
        attnpool_attend_kernel<0><<<grid, 64, 0, s>>>((const _Float16 *)q, (const _Float16 *)kv, L, C, (_Float16 *)out);
    else
        attnpool_attend_kernel<1><<<grid, 64, 0, s>>>((const __bf16 *)q, (const __bf16 *)kv, L, C, (__bf16 *)out);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

// ---- the whole tower: ec_resnet_workspace_bytes / ec_resnet_encode ----
namespace {

struct TowerPlan {
    size_t act_elems;   // the largest 16-bit activation of one chunk (every ping-pong buffer has this size)
    size_t tok_elems, c_elems, kv_elems;
    int C, L, hw_last;
};

int check_weights(const ec_resnet_weights *w, const char *fn)
{
    EC_REQUIRE(w, "%s: null weights", fn);
    EC_REQUIRE(w->struct_bytes == sizeof(ec_resnet_weights),
               "%s: ec_resnet_weights.struct_bytes = %zu, this library's is %zu (rebuild against include/eventclip_hip.h)",
               fn, w->struct_bytes, sizeof(ec_resnet_weights));
    EC_REQUIRE(w->dtype == EC_F16 || w->dtype == EC_BF16, "%s: dtype=%d", fn, w->dtype);
    EC_REQUIRE(w->image_size >= 64 && w->image_size % 32 == 0, "%s: image_size=%d (a multiple of 32)", fn, w->image_size);
    EC_REQUIRE(w->n_blocks > 0 && w->blocks, "%s: n_blocks=%d", fn, w->n_blocks);
    EC_REQUIRE(w->stem[0].ks == 1 && w->stem[0].cin == 64, "%s: stem[0] is the 1x1 product over the 64-wide stem rows", fn);
    const int C = w->q.cin;
    EC_REQUIRE(C % 64 == 0 && w->kv.cin == C && w->kv.cout == 2 * C && w->q.cout == C && w->c.cin == C &&
               w->c.cout == w->embed_dim && w->pos, "%s: attention pool shapes (C=%d, embed_dim=%d)", fn, C, w->embed_dim);
    const int g = w->image_size / 32;
    EC_REQUIRE(g * g + 1 <= 256, "%s: %d attention-pool tokens (at most 256)", fn, g * g + 1);
    const int pb = w->precise_blocks;
    EC_REQUIRE(pb >= 0 && pb <= w->n_blocks, "%s: precise_blocks=%d (0 .. n_blocks=%d)", fn, pb, w->n_blocks);
    if (pb > 0) {
        EC_REQUIRE(w->dtype == EC_F16, "%s: precise_blocks=%d needs dtype EC_F16 (the split form is f16 only)", fn, pb);
        bool lo = w->stem[0].w_lo && w->stem[1].w_lo && w->stem[2].w_lo;
        for (int b = 0; b < pb; b++) {
            const ec_resnet_block &k = w->blocks[b];
            lo = lo && k.c1.w_lo && k.c2.w_lo && k.c3.w_lo && (!k.ds.w || k.ds.w_lo);
        }
        if (pb == w->n_blocks) lo = lo && w->q.w_lo && w->kv.w_lo && w->c.w_lo;
        EC_REQUIRE(lo, "%s: precise_blocks=%d needs w_lo of every convolution that runs split", fn, pb);
    }
    return EC_OK;
}

TowerPlan plan_of(const ec_resnet_weights *w, int n)
{
    TowerPlan p{};
    size_t m = 0;
    int h = w->image_size / 2;
    auto see = [&](size_t e) { m = e > m ? e : m; };
    see((size_t)n * h * h * 64);
    for (int i = 0; i < 3; i++) see((size_t)n * h * h * w->stem[i].cout);
    h /= 2;
    for (int b = 0; b < w->n_blocks; b++) {
        const ec_resnet_block &k = w->blocks[b];
        see((size_t)n * h * h * k.c1.cout);
        see((size_t)n * h * h * k.c2.cout);
        const int ho = h / k.stride;
        see((size_t)n * ho * ho * k.c3.cout);
        if (k.ds.w) see((size_t)n * h * h * k.ds.cin);
        h = ho;
    }
    p.act_elems = (m + 127) / 128 * 128;
    p.C = w->q.cin;
    p.hw_last = h * h;
    p.L = h * h + 1;
    p.tok_elems = ((size_t)n * p.L * p.C + 127) / 128 * 128;
    p.c_elems = ((size_t)n * p.C + 127) / 128 * 128;
    p.kv_elems = ((size_t)n * p.L * 2 * p.C + 127) / 128 * 128;
    return p;
}

// 16-bit elements of one plane of the workspace; the split form keeps a second plane (lo) right behind the first
size_t plane_elems_of(const TowerPlan &p) { return 4 * p.act_elems + p.tok_elems + 2 * p.c_elems + p.kv_elems; }

size_t ws_bytes_of(const TowerPlan &p, int precise_blocks = 0)
{
    return 2 * plane_elems_of(p) * (precise_blocks > 0 ? 2 : 1);
}

int conv_w(const void *x, int n, int H, const ec_resnet_conv_w &c, const void *resid, int relu, void *out, int out32,
           int dtype, ec_stream_t s)
{
    return ec_resnet_conv(x, n, H, H, c.cin, c.cout, c.ks, c.w, c.scale, c.bias, resid, relu, out, out32, dtype, s);
}

}  // namespace

EC_API size_t ec_resnet_workspace_bytes(const ec_resnet_weights *w, int chunk)
{
    if (check_weights(w, "ec_resnet_workspace_bytes") != EC_OK || chunk <= 0) return 0;
    return ws_bytes_of(plan_of(w, chunk), w->precise_blocks);
}

#define EC_TRY(expr)                                                                                               \
    do {                                                                                                           \
        int _rc = (expr);                                                                                          \
        if (_rc != EC_OK) return _rc;                                                                              \
    } while (0)

EC_API int ec_resnet_encode(const ec_resnet_weights *w, const void *input, int input_mode, int n_img, float *feats,
                            void *ws, size_t ws_bytes, int chunk, ec_stream_t stream)
{
    EC_TRY(check_weights(w, "ec_resnet_encode"));
    EC_REQUIRE(input_mode == EC_PRE_CHW_F32 || input_mode == EC_PRE_HWC_U8, "ec_resnet_encode: input_mode=%d", input_mode);
    EC_REQUIRE(n_img >= 0 && chunk > 0, "ec_resnet_encode: n_img=%d chunk=%d", n_img, chunk);
    if (n_img == 0) return EC_OK;
    EC_REQUIRE(input && feats && ws, "ec_resnet_encode: null buffer");
    const int cn = chunk < n_img ? chunk : n_img;
    const TowerPlan p = plan_of(w, cn);
    const int pb = w->precise_blocks;
    EC_REQUIRE(ws_bytes >= ws_bytes_of(p, pb), "ec_resnet_encode: workspace %zu bytes, %zu needed for chunk %d", ws_bytes,
               ws_bytes_of(p, pb), cn);
    const int dt = w->dtype, R = w->image_size;
    const size_t in_img = (size_t)3 * R * R * (input_mode == EC_PRE_HWC_U8 ? 1 : 4);
    uint16_t *base = (uint16_t *)ws;
    void *buf[4];
    for (int i = 0; i < 4; i++) buf[i] = base + i * p.act_elems;
    uint16_t *tok = base + 4 * p.act_elems, *q_in = tok + p.tok_elems, *att = q_in + p.c_elems;
    uint16_t *kv = att + p.c_elems;
    auto other = [&](std::initializer_list<void *> used) -> void * {
        for (void *b : buf) {
            bool u = false;
            for (void *x : used) u = u || x == b;
            if (!u) return b;
        }
        return nullptr;
    };
    // the split form (precise_blocks > 0): every buffer's lo plane lies plane_elems behind its hi plane
    const size_t plane = plane_elems_of(p);
    auto lo = [&](const void *hi) -> void * { return hi ? (uint16_t *)hi + plane : nullptr; };
    // one convolution / pooling step, split (pr) or 16-bit; the 16-bit calls are those of the default path
    auto conv = [&](bool pr, const void *x, int n, int H, const ec_resnet_conv_w &c, const void *resid, int relu, void *out,
                    int out32) -> int {
        if (pr)
            return ec_resnet_conv_hl(x, lo(x), n, H, H, c.cin, c.cout, c.ks, c.w, c.w_lo, c.scale, c.bias, resid, lo(resid),
                                     relu, out, out32 ? nullptr : lo(out), out32, dt, stream);
        return conv_w(x, n, H, c, resid, relu, out, out32, dt, stream);
    };
    auto pool = [&](bool pr, const void *x, int n, int H, int C, void *y) -> int {
        if (pr) return ec_resnet_avgpool_hl(x, lo(x), n, H, H, C, y, lo(y), dt, stream);
        return ec_resnet_avgpool(x, n, H, H, C, y, dt, stream);
    };
    for (int i0 = 0; i0 < n_img; i0 += cn) {
        const int n = n_img - i0 < cn ? n_img - i0 : cn;
        const void *in = (const char *)input + (size_t)i0 * in_img;
        int h = R / 2;
        bool pr = pb > 0;
        if (pr) EC_TRY(ec_resnet_stem_rows_hl(in, input_mode, n, R, buf[0], lo(buf[0]), dt, stream));
        else EC_TRY(ec_resnet_stem_rows(in, input_mode, n, R, buf[0], dt, stream));
        EC_TRY(conv(pr, buf[0], n, h, w->stem[0], nullptr, 1, buf[1], 0));
        EC_TRY(conv(pr, buf[1], n, h, w->stem[1], nullptr, 1, buf[0], 0));
        EC_TRY(conv(pr, buf[0], n, h, w->stem[2], nullptr, 1, buf[1], 0));
        EC_TRY(pool(pr, buf[1], n, h, w->stem[2].cout, buf[0]));
        h /= 2;
        void *x = buf[0];
        for (int b = 0; b < w->n_blocks; b++) {
            const ec_resnet_block &k = w->blocks[b];
            EC_REQUIRE(k.stride == 1 || k.stride == 2, "ec_resnet_encode: block %d stride %d", b, k.stride);
            EC_REQUIRE(k.stride == 1 || k.ds.w, "ec_resnet_encode: block %d strides without a downsample", b);
            pr = b < pb;   // past the last split block the 16-bit path goes on from the hi plane
            void *o1 = other({x});
            EC_TRY(conv(pr, x, n, h, k.c1, nullptr, 1, o1, 0));
            void *o2 = other({x, o1});
            EC_TRY(conv(pr, o1, n, h, k.c2, nullptr, 1, o2, 0));
            void *o = o2;
            if (k.stride > 1) {
                EC_TRY(pool(pr, o2, n, h, k.c2.cout, o1));
                o = o1;
            }
            const int ho = h / k.stride;
            void *idt = x;
            if (k.ds.w) {
                void *t = other({x, o});
                const void *src = x;
                if (k.stride > 1) {
                    void *t2 = other({x, o, t});
                    EC_TRY(pool(pr, x, n, h, k.ds.cin, t2));
                    src = t2;
                }
                EC_TRY(conv(pr, src, n, ho, k.ds, nullptr, 0, t, 0));
                idt = t;
            }
            void *y = other({o, idt});
            EC_TRY(conv(pr, o, n, ho, k.c3, idt, 1, y, 0));
            x = y;
            h = ho;
        }
        float *f = feats + (size_t)i0 * w->embed_dim;
        if (pb == w->n_blocks) {
            EC_TRY(ec_resnet_attnpool_tokens_hl(x, lo(x), n, p.hw_last, p.C, w->pos, tok, lo(tok), q_in, lo(q_in), dt, stream));
            EC_TRY(ec_resnet_conv_hl(q_in, lo(q_in), n, 1, 1, p.C, p.C, 1, w->q.w, w->q.w_lo, w->q.scale, w->q.bias, nullptr,
                                     nullptr, 0, att, lo(att), 0, dt, stream));
            EC_TRY(ec_resnet_conv_hl(tok, lo(tok), n * p.L, 1, 1, p.C, 2 * p.C, 1, w->kv.w, w->kv.w_lo, w->kv.scale, w->kv.bias,
                                     nullptr, nullptr, 0, kv, lo(kv), 0, dt, stream));
            EC_TRY(ec_resnet_attnpool_attend_hl(att, lo(att), kv, lo(kv), n, p.L, p.C, q_in, lo(q_in), dt, stream));
            EC_TRY(ec_resnet_conv_hl(q_in, lo(q_in), n, 1, 1, p.C, w->embed_dim, 1, w->c.w, w->c.w_lo, w->c.scale, w->c.bias,
                                     nullptr, nullptr, 0, f, nullptr, 1, dt, stream));
            continue;
        }
        EC_TRY(ec_resnet_attnpool_tokens(x, n, p.hw_last, p.C, w->pos, tok, q_in, dt, stream));
        EC_TRY(ec_resnet_conv(q_in, n, 1, 1, p.C, p.C, 1, w->q.w, w->q.scale, w->q.bias, nullptr, 0, att, 0, dt, stream));
        EC_TRY(ec_resnet_conv(tok, n * p.L, 1, 1, p.C, 2 * p.C, 1, w->kv.w, w->kv.scale, w->kv.bias, nullptr, 0, kv, 0,
                              dt, stream));
        EC_TRY(ec_resnet_attnpool_attend(att, kv, n, p.L, p.C, q_in, dt, stream));
        EC_TRY(ec_resnet_conv(q_in, n, 1, 1, p.C, w->embed_dim, 1, w->c.w, w->c.scale, w->c.bias, nullptr, 0, f, 1, dt, stream));
    }
    return EC_OK;
}
