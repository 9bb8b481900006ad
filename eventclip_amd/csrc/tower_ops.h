// Host-side pieces shared by the tower drivers (towers.hip: inference, vit_train.hip: fine-tuning):
// scratch carving, the ec_gemm call forms, the split-precision patch embedding.
#pragma once
#include "common.h"

namespace ec_tower {

constexpr float LN_EPS = 1e-5f;

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Scratch {
    unsigned char *base;
    size_t off, cap;
    void *take(size_t bytes)
    {
        void *p = base ? base + off : nullptr;
        off += align_up(bytes);
        return p;
    }
};

// K-batch scratch of the low-latency mode (ec_vit_weights.low_latency): set by the tower driver for the duration of
// one call on the calling thread; NULL = every launch in a single pass
struct LatencyScratch {
    void *ws;
    size_t bytes;
};
inline LatencyScratch &latency_scratch()
{
    static thread_local LatencyScratch s = {nullptr, 0};
    return s;
}
constexpr size_t LATENCY_WS_BYTES = (size_t)80 << 20;   // 256 workgroups x one 256 x 256 fp32 tile, with slack

// The K-batch split rule, for ec_gemm's low-latency form (gemm.hip: try_kbatched, cap 16, 2 K tiles) and the short last
// row of tiles of the training GEMMs (vit_train.hip: gemm_rows32, cap 8, 4 K tiles): into how many K-batches `tiles`
// under-filling output tiles of `nk` K tiles (of 64) are cut on `cus` compute units -- doubled while the workgroups
// still fit twice, the batches stay equal, and each keeps at least `min_nk` K tiles; at most `cap`.  1: no cut.
inline int kbatch_splits(int tiles, int nk, int cus, int cap, int min_nk)
{
    int splits = 1;
    while (splits < cap && tiles * splits * 2 <= cus && nk % (splits * 2) == 0 && nk / (splits * 2) >= min_nk) splits *= 2;
    return splits;
}

constexpr int LO8_EXP = 12;    // lo parts of activations as e4m3 of lo . 2^12: saturates where the activation exceeds 256
constexpr int HI8_EXP = 0;     // e4m3 copies of hi parts at scale 1: saturates beyond 448
// the lo products on the FP8 matrix path (ec_vit_weights.lo_fp8): A_lo8 = the e4m3 lo part of A (ec_layernorm_hl8 / the
// e4m3 lo output of c_fc), W8 = the e4m3 copy of W; where the weight has a lo part: A8 (e4m3 copy of A) with W_lo8, or
// the 16-bit W_lo where no A8 exists (c_proj)
struct Fp8Parts {
    const void *A_lo8, *W8, *A8, *W_lo8;
    int w8_exp, w_lo8_exp;
};
// One ec_gemm launch: the operands every launch has, then one named setter per optional group.  Every ec_gemm_args
// field is assigned here and nowhere else in the tower drivers.
struct Gemm {
    ec_gemm_args g = {};
    Gemm(int M, int N, int K, int dtype, int epi, const void *A, const void *W, const float *bias, void *C)
    {
        g.M = M, g.N = N, g.K = K, g.dtype = dtype, g.epilogue = epi, g.variant = 0;
        g.A = A, g.W = W, g.bias = bias, g.C = C;
    }
    // row strides of A / C in elements (0 = dense: K / N)
    Gemm &ld(long lda, long ldc) { return g.lda = lda, g.ldc = ldc, *this; }
    // Split-precision product: x.w = xl.wh + xh.wl + xh.wh accumulated in fp32 -- ONE launch since round 5 (ec_gemm_args.A_lo /
    // W_lo: the three products run into the same accumulators; rounds 1 - 4 launched three GEMMs that read and wrote the
    // fp32 C twice more).  W_lo == NULL: the weight IS its 16-bit value (ec_vit_weights.weights_exact16), the product with
    // its lo part -- a sum of zeros -- is skipped, the same bits out.  A_lo == NULL: the activation has no lo part.
    Gemm &lo(const void *A_lo, const void *W_lo) { return g.A_lo = A_lo, g.W_lo = W_lo, *this; }
    // EC_EPI_RESID_HL: the lo plane; STORE16 / GELU16 with split operands: the output's lo part (e4m3: as e4m3 of
    // lo . 2^LO8_EXP); the training epilogues: their second output / input
    Gemm &aux(void *p, bool e4m3 = false)
    {
        g.aux = p;
        if (p && e4m3) g.aux_e4m3 = 1, g.aux_exp = LO8_EXP;
        return *this;
    }
    // the GELU epilogues: QuickGELU (0) or the exact GELU (1), ec_vit_weights.activation / ec_text_weights.activation
    Gemm &act(int activation) { return g.activation = activation, *this; }
    // EC_EPI_*_LN (folded LayerNorm): row statistics + column sums
    Gemm &ln(const float *row_stats, long stride, const float *col_sums)
    {
        return g.row_stats = row_stats, g.row_stats_stride = stride, g.col_sums = col_sums, *this;
    }
    // EC_EPI_RESID_HL: per-group sums of the new hi plane (ec_row_stats_merge), or NULL
    Gemm &row_sums(float *p) { return g.row_sums = p, *this; }
    Gemm &fp8(const Fp8Parts &f)
    {
        g.A_lo8 = f.A_lo8, g.W8 = f.W8, g.a_lo8_exp = LO8_EXP, g.w8_exp = f.w8_exp;
        if (f.A8 && f.W_lo8) g.A8 = f.A8, g.W_lo8 = f.W_lo8, g.a8_exp = HI8_EXP, g.w_lo8_exp = f.w_lo8_exp;
        return *this;
    }
    // low-latency mode: an under-filled launch runs K-batched through the call's scratch (single pass where none is set)
    Gemm &k_batched() { return g.ws = latency_scratch().ws, g.ws_bytes = latency_scratch().bytes, *this; }
    // EC_EPI_RESID32 out of place (training): C = resid + acc + bias
    Gemm &resid(const float *r) { return g.resid = r, *this; }
    int run(ec_stream_t s) const { return ec_gemm(&g, s); }
};

// layernorm.hip: ln_pre'd embedding straight into the hi / lo planes; class rows of the planes back to fp32
int vit_embed_hl(const float *patch, const float *cls, const float *pos, const float *gamma, const float *beta,
                 int n_img, int seq, int width, float eps, void *x_hi, void *x_lo, int dtype, ec_stream_t stream);
int split_hl(const float *x, long n, void *x_hi, void *x_lo, int dtype, ec_stream_t stream);
int join_hl_rows(const void *x_hi, const void *x_lo, long ld, int rows, int width, float *out, int dtype,
                 ec_stream_t stream);

// attention.hip: 16-bit attention on a PLAIN q with every score scaled in fp32 (q rounded once; ec_attention's kernel
// multiplies q by the scale and rounds it again)
int attention_exact_scale(const void *qkv, void *out, int n_seq, int S, int width, int heads, int dtype, ec_stream_t stream);

#define EC_TRY(expr)                  \
    do {                              \
        int _rc = (expr);             \
        if (_rc != EC_OK) return _rc; \
    } while (0)

// conv1 (kernel = stride = patch, no bias) as a GEMM over im2col rows, to fp32 accuracy: a patch
// row is [hi | lo | 0] (kpad wide) and conv_w = [w_hi | w_hi | 0], so the first launch gives
// x_hi.w_hi + x_lo.w_hi; the second adds x_hi.w_lo over the row's first klo columns (conv_w_lo =
// [w_lo | 0]: the lo values the row holds beyond 3 p^2 meet zeros).  0.6 % of the tower's flops; the
// rounding of pixels and conv1.weight to 16 bits would otherwise be ~8 % of the logit error budget
// (tools/rounding_budget.py).
inline int patch_embed(const ec_vit_weights *w, const void *patches, int rows, float *out, ec_stream_t s)
{
    const int klo = ((3 * w->patch * w->patch + 63) / 64) * 64;
    EC_TRY(Gemm(rows, w->width, w->kpad, w->dtype, EC_EPI_STORE32, patches, w->conv_w, nullptr, out).k_batched().run(s));
    if (!w->conv_w_lo) return EC_OK;   // conv1.weight IS its 16-bit value (weights_exact16): a sum of zeros skipped, the same bits
    return Gemm(rows, w->width, klo, w->dtype, EC_EPI_RESID32, patches, w->conv_w_lo, nullptr, out).ld(w->kpad, 0).k_batched().run(s);
}

}  // namespace ec_tower
