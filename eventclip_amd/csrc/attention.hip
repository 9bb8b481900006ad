// Fused multi-head self-attention for the CLIP towers (gfx950), head dim 64.
//
// Replaces nn.MultiheadAttention inside the ResidualAttentionBlocks of
// un-vendored openai/CLIP clip/model.py (reached through
// models/clip_cls.py:84 encode_text / :101 encode_image).  Sequences are short
// and fixed (50..577 vision tokens, 77 text tokens), so one workgroup owns one
// (sequence, head): the head's whole K and V (<= 608 x 64 x 16 bit each) sit in
// LDS and every wave takes 16-query tiles.  Keys are walked in 64-key blocks with
// an online softmax (running max / sum per query, O rescaled per block: 16
// registers), which keeps the kernel near 100 VGPRs for any sequence length.
//
//  * S^T = K . Q^T with v_mfma_f32_16x16x32: K rows from LDS (ds_read_b128,
//    XOR-swizzled 128-B rows), Q straight from HBM as the B operand.  A lane then
//    holds one query column: softmax reductions are in-lane plus two xor-shuffles.
//  * O^T = V^T . P^T: the exponentiated score registers ARE the B operand (the k
//    index inside each 32-key step is permuted consistently on both operands), so
//    P never moves between lanes or through LDS.  V stays row-major in LDS and is
//    read transposed with ds_read_b64_tr_b16; its 8-byte slots are XOR-swizzled
//    by (row >> 1) & 3 so the transposed reads are bank-conflict free.  The V^T
//    row order is permuted so each lane ends with 16 contiguous head-dim outputs
//    (two 16-B stores).
//  * fp32 scores / softmax / accumulation; the 1/sqrt(64) scale is a power of two.
#include <type_traits>

#include "common.h"
#include "mfma.h"
#include "tower_ops.h"

#ifdef EC_ATTN_DIAG
// diagnostic build only (python -m eventclip_amd.build --diag, tools/timeline_attn.py): s_memtime at
// workgroup start / K and V staged / done, and the CU the workgroup ran on
__device__ unsigned long long ec_attn_stamps[4 * 65536];
#endif

namespace {

using namespace ec;

#ifdef EC_ATTN_DIAG
__device__ __forceinline__ void attn_stamp(int i)
{
    unsigned long long now;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    if (threadIdx.x == 0 && blockIdx.x < 65536) ec_attn_stamps[blockIdx.x * 4 + i] = now;
}
#else
__device__ __forceinline__ void attn_stamp(int) {}
#endif

// Waves per workgroup, as dispatch() picks them: 8 while K + V and the 4224-byte merge area of a split tile stay within
// 80 KiB, so that two workgroups fit a CU's LDS (nine 32-key steps: S <= 288), 16 from S = 289 on, where the sequence's K
// and V leave room for one workgroup only (S = 577: 148 KiB) -- four waves per SIMD either way.

struct AttnArgs {
    const void *qkv;  // [n_seq * S, 3W] 16-bit: q | k | v, heads are 64-wide column blocks
    void *out;        // [n_seq * S, W] 16-bit
    int S, W, heads, causal;
    int q_rows;       // only the first q_rows query rows of every sequence are computed; out is
                      // [n_seq * q_rows, W] (q_rows = S: the whole sequence)
    float scale_log2e;
    int q_scaled;     // 1: the q columns already hold q * scale_log2e (QM_INPUT); 2: plain q, scores scaled in fp32 (QM_RAW)
    float *lse;       // LSE kernels only: [n_seq, heads, S] fp32, log2 of the softmax denominator in the
                      // scaled-score domain (m * scale_log2e + log2 l), kept for ec_attention_backward
};

// One block of the online softmax: scores -> running max / sum -> P^T as the B operand -> O^T += V^T . P^T.
// The vector ALU is the saturated pipe of this kernel (profiles/r2_attention.md), so the block is
// arranged to leave it only what no other unit can do -- one exp2, half a max3 and half a convert per score:
//  * the query fragment arrives pre-multiplied by log2(e) / sqrt(64), so the MFMA result is already the
//    exponent's argument up to the row offset;
//  * the row offset is the MFMA's C operand: mneg = {-m, -m, -m, -m} for the lane's query (a lane's four
//    accumulator rows belong to ONE query column), so the matrix pipe delivers s - m and no per-score
//    subtract is left;
//  * m is the running maximum as of the last time it MOVED, not of the block.  It starts at 0; a block whose
//    scores stay below m + ATTN_THR (log2 units; and, for a tile's first block only, whose maximum is not
//    below m - ATTN_LO) keeps m, O and the row sum as they are -- P <= 2^ATTN_THR is exact in either 16-bit
//    type, and nothing is rescaled.  Only when some lane sees a larger score (a wave-uniform branch, seldom
//    taken) are m, the scores of this block, O and the row sum moved to the new maximum, all of them
//    exactly once, BEFORE this block's P is formed (cdna_hip_programming.md T13's safe order);
//  * the row sum comes from the matrix pipe too: a fifth "V^T" tile of ones, so l = sum of the ROUNDED
//    P the output was built from.
// Where the factor c = log2(e) / sqrt(64) of the scores comes from (template parameter QM of the block):
//  QM_INPUT  the q columns of qkv already hold c q: the image tower folds c into the q rows of in_proj_weight /
//            in_proj_bias BEFORE they are rounded to 16 bit (ec_vit_weights.q_scaled), so the product is rounded
//            once, like an unscaled q -- no work and no error in the kernel;
//  QM_KERNEL the kernel multiplies its query fragment by c and rounds it to the operand type a second time: f16
//            callers that pass a plain q (ec_attention, the training forward).  +20 % on the kernel's own
//            rounding error on unit-variance data (6.3e-4 against 4.8e-4), +25 % on the logits of a tower with
//            sharp attention (tests/test_configs_gpu.py configs[3]), which is why the tower uses QM_INPUT;
//  QM_RAW    scores stay in raw units and every score is multiplied by c in fp32: bf16 callers with a plain q
//            (8 bits of a twice-rounded q would put 2e-2 on the log-sum-exp the training forward saves).
enum { QM_RAW = 0, QM_KERNEL = 1, QM_INPUT = 2 };
constexpr float ATTN_THR = 10.f;
constexpr float ATTN_LO = 4.f;   // first block: P of the row maximum >= 2^-4, the rest of a 16-bit float's range below it

// O += A . B IN PLACE (tied operand), one asm statement per MFMA.  Through the builtin hipcc lets the
// loop-carried accumulators wander (D != C) and pays for it with a copy of all of O in every block once the
// block has the seldom-taken branch below in it; an asm statement's "+v" operand cannot move (one statement
// with all five accumulators tied brings the copies back: one each).  What hipcc does not pad for an asm
// statement (cdna_hip_programming.md 5.7 item 2) is handled by hand:
//  pad 1 = two wait states in front -- a just-written vector result needs them before an MFMA reads it (a
//          step's first MFMA: the converted P);
//  pad 2 = twelve behind -- a block's last MFMA: hipcc may read O right behind the block (copies at loop
//          exits, spills, the epilogue) and pads nothing for a producer inside an asm string.
// Elsewhere O arrives from the previous step's MFMAs (an accumulate chain on the whole of D needs none) and the
// V^T fragments from ds_reads (the compiler's own s_waitcnt covers asm inputs).  tools/check_attn_isa.py
// checks the compiled kernels for vector writes right in front of the unpadded statements.
template <int pad> __device__ __forceinline__ void mfma16_acc(const f16x8 &a, const f16x8 &b, f32x4 &c)
{
    if (pad == 1)
        asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
    else if (pad == 2)
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\ts_nop 11" : "+v"(c) : "v"(a), "v"(b));
    else
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
template <int pad> __device__ __forceinline__ void mfma16_acc(const bf16x8 &a, const bf16x8 &b, f32x4 &c)
{
    if (pad == 1)
        asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
    else if (pad == 2)
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n\ts_nop 11" : "+v"(c) : "v"(a), "v"(b));
    else
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}

// The seldom-taken arm: move the lane's query to a new maximum.  d = how far in the units of the scores,
// d_log2 = in log2 units (the same where the query arrives pre-scaled); everything still
// at the old m moves with it exactly once: the caller's pending scores (by the caller), O and the row sum
// (scaled by 2^-d; by 0 while they are still empty: `down`), and -m.  O and -m IN PLACE like the MFMAs'
// accumulate; O was last written by the previous block's MFMAs, whose last statement waited for them.
__device__ __forceinline__ void attn_move(float d, float d_log2, bool down, f32x4 &mneg, f32x4 (&o)[5])
{
    float alpha = __builtin_amdgcn_exp2f(-d_log2);
    alpha = down ? 0.f : alpha;
#pragma unroll
    for (int dt = 0; dt < 5; dt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float t = o[dt][r];
            asm volatile("s_nop 0\n\tv_mul_f32 %0, %0, %1" : "+v"(t) : "v"(alpha));   // s_nop: alpha is fresh from v_exp / v_cndmask
            o[dt][r] = t;
        }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float t = mneg[r];
        asm volatile("v_sub_f32 %0, %0, %1" : "+v"(t) : "v"(d));
        mneg[r] = t;
    }
}

// Position of a key row's 16-byte K chunk c / 8-byte V slot u inside its 128-byte LDS row: c ^ kkey(row), u ^ vkey(row)
// (conflict-free for the fragment reads of a 16-query tile)
__device__ __forceinline__ int kkey(int row) { return row & 7; }
__device__ __forceinline__ int vkey(int row) { return (row >> 1) & 3; }
// ... as byte offsets inside the row, which lies at image + 128 row (the hi + lo kernels keep four planes in this layout)
__device__ __forceinline__ int k_chunk(int row, int c) { return (c ^ kkey(row)) << 4; }
__device__ __forceinline__ int v_slot(int row, int u) { return (u ^ vkey(row)) * 8; }
// Stage 16-byte chunk ch (the 8-byte slots 2 ch, 2 ch + 1) of a V row: slot u -> u ^ vkey(row), so the chunk moves by
// bit 1 of the key (bit 2 of the row) and its halves swap by bit 0 (bit 1 of the row)
__device__ __forceinline__ void v_put(unsigned char *ldsV, int row, int ch, u32x4 t)
{
    if ((row >> 1) & 1) t = u32x4{t[2], t[3], t[0], t[1]};
    *reinterpret_cast<u32x4 *>(ldsV + row * 128 + ((ch ^ ((row >> 2) & 1)) << 4)) = t;
}

// A vector of ones (the fifth "V^T" tile: the row sum from the matrix pipe), pinned: it stays in four VGPRs (else
// rebuilt from SGPRs in every block)
template <int DT> __device__ __forceinline__ typename T16<DT>::v8 ones16()
{
    typename T16<DT>::v8 ones;
#pragma unroll
    for (int j = 0; j < 8; j++) ones[j] = to16(1.f, typename T16<DT>::elem());
    asm volatile("" : "+v"(ones));
    return ones;
}

// One block of KSTEPS 32-key steps.  `down`: the tile has added nothing yet (m may move down too).
template <int DT, int KSTEPS, bool MASK, int QM>
__device__ __forceinline__ void attn_block2(const unsigned char *ldsK, const unsigned char *ldsV,
                                            int key0, int klimit, const typename T16<DT>::v8 (&qf)[2],
                                            const typename T16<DT>::v8 &ones, bool down, float c, f32x4 &mneg,
                                            f32x4 (&o)[5], int g, int c16)
{
    constexpr bool PRE = QM != QM_RAW;   // else: scores in raw units, c = log2(e) / sqrt(64) applied per score
    const float thr = PRE ? ATTN_THR : ATTN_THR / c, lo = PRE ? ATTN_LO : ATTN_LO / c;
    typedef typename T16<DT>::elem elem;
    typedef typename T16<DT>::v8 v8;
    typedef typename T16<DT>::v4 v4;
    constexpr int NT = 2 * KSTEPS;
    // ---- acc[kt][r] = c <k[key0 + 16 kt + 4 g + r], q[c16]> - m[c16] ----
    f32x4 acc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; kt++) {
        const int row = key0 + kt * 16 + c16;
        const v8 k0 = *reinterpret_cast<const v8 *>(ldsK + row * 128 + k_chunk(row, 0 + g));
        const v8 k1 = *reinterpret_cast<const v8 *>(ldsK + row * 128 + k_chunk(row, 4 + g));
        acc[kt] = mfma16(k0, qf[0], mneg);
        acc[kt] = mfma16(k1, qf[1], acc[kt]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (MASK) {   // only blocks that reach past klimit (padding, causal diagonal)
                const int key = key0 + kt * 16 + 4 * g + r;
                acc[kt][r] = key < klimit ? acc[kt][r] : -INFINITY;
            }
            mx = fmaxf(mx, acc[kt][r]);
        }
    if (__builtin_amdgcn_ballot_w64(mx > thr || (down && mx < -lo)) != 0) {
        // the four lane groups hold different keys of the same query and all hold parts of its O column:
        // one distance for all of them; up only, unless nothing has been added yet.  Only the queries that
        // need it move (d = 0, scale 1 for the others: bit for bit as if the branch had not been taken), so a
        // query's result never depends on which other queries share its tile (ec_attention_rows computes a
        // prefix of the rows next to whatever the caller left in the others)
        const float mq = xor_max(mx);
        const float d = (mq > thr || (down && mq < -lo)) ? mq : 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; kt++) acc[kt] -= d;
        attn_move(d, PRE ? d : d * c, down, mneg, o);
    }
    // ---- O^T += V^T . P^T, row sum += 1^T . P^T ----
#pragma unroll
    for (int s = 0; s < KSTEPS; s++) {
        // the step's four V^T fragments are requested first: their LDS latency passes under the
        // exponentials.  A operand row i <-> head dim (i >> 2) * 16 + 4 dt + (i & 3), key order as below
        v8 vf[4];
#pragma unroll
        for (int dt = 0; dt < 4; dt++)
#pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                const int row = key0 + 32 * s + 16 * hh + 4 * g + (c16 >> 2);
                const int u = v_slot(row, (c16 & 3) * 4 + dt);
                const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4 *)(ldsV + row * 128 + u));
                const v4 tv = __builtin_bit_cast(v4, t);
                vf[dt][4 * hh] = tv[0], vf[dt][4 * hh + 1] = tv[1], vf[dt][4 * hh + 2] = tv[2],
                            vf[dt][4 * hh + 3] = tv[3];
            }
        // B operand element j <-> key key0 + 32 s + 16 (j >> 2) + 4 g + (j & 3)
        v8 pf;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            pf[r] = to16(__builtin_amdgcn_exp2f(PRE ? acc[2 * s][r] : acc[2 * s][r] * c), elem());
            pf[4 + r] = to16(__builtin_amdgcn_exp2f(PRE ? acc[2 * s + 1][r] : acc[2 * s + 1][r] * c), elem());
        }
        mfma16_acc<1>(ones, pf, o[4]);
#pragma unroll
        for (int dt = 0; dt < 3; dt++) mfma16_acc<0>(vf[dt], pf, o[dt]);
        if (s == KSTEPS - 1)
            mfma16_acc<2>(vf[3], pf, o[3]);
        else
            mfma16_acc<0>(vf[3], pf, o[3]);
    }
}

// A single key (the 257th / 577th token of the ViT sequences: S = 32 n + 1) as a rank-one update instead of
// a masked 32-key step: two MFMAs for its 16 scores -- the LDS rows behind the last key are copies of it, so
// every row of the key tile, hence every accumulator register of a lane, is the lane's query against THIS
// key -- one exp2, and 16 multiply-adds of the key's V row (head dims 16 g .. 16 g + 15 for this lane, as the
// epilogue stores them) instead of 8 masked scores, 5 MFMAs and 16 LDS reads.  P is rounded to 16 bit like
// every other P.  Must follow the tile's last block (its last MFMA waited for O to settle).
template <int DT, int QM>
__device__ __forceinline__ void attn_odd_key(const unsigned char *ldsK, const unsigned char *ldsV, int key,
                                             const typename T16<DT>::v8 (&qf)[2], bool down, float c, f32x4 &mneg,
                                             f32x4 (&o)[5], int g, int c16)
{
    typedef typename T16<DT>::elem elem;
    typedef typename T16<DT>::v8 v8;
    typedef typename T16<DT>::v4 v4;
    constexpr bool PRE = QM != QM_RAW;
    const float thr = PRE ? ATTN_THR : ATTN_THR / c, lo = PRE ? ATTN_LO : ATTN_LO / c;
    const int row = key + c16;
    const v8 k0 = *reinterpret_cast<const v8 *>(ldsK + row * 128 + k_chunk(row, 0 + g));
    const v8 k1 = *reinterpret_cast<const v8 *>(ldsK + row * 128 + k_chunk(row, 4 + g));
    v4 vv[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++)   // logical 8-byte slot 4 g + dt of V's row
        vv[dt] = *reinterpret_cast<const v4 *>(ldsV + key * 128 + v_slot(key, 4 * g + dt));
    f32x4 acc = mfma16(k0, qf[0], mneg);
    acc = mfma16(k1, qf[1], acc);
    float sc = acc[0];
    if (__builtin_amdgcn_ballot_w64(sc > thr || (down && sc < -lo)) != 0) {
        const float d = (sc > thr || (down && sc < -lo)) ? sc : 0.f;   // the same in the query's four lane groups
        sc -= d;
        attn_move(d, PRE ? d : d * c, down, mneg, o);
    }
    const float p = (float)to16(__builtin_amdgcn_exp2f(PRE ? sc : sc * c), elem());
    o[4][0] += p;    // the epilogue reads register 0 of the row-sum tile
#pragma unroll
    for (int dt = 0; dt < 4; dt++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[dt][r] = __builtin_fmaf(p, (float)vv[dt][r], o[dt][r]);
}

// Keys of one tile, not causal: the full 32-key steps [step0, step1) in blocks of two, then (`tail`) whatever
// lies behind the last full step of the sequence: nothing, one key (rank-one update) or a masked step.
template <int DT, int QM>
__device__ __forceinline__ void attn_keys(const unsigned char *ldsK, const unsigned char *ldsV, int S, int step0,
                                          int step1, bool tail, const typename T16<DT>::v8 (&qf)[2],
                                          const typename T16<DT>::v8 &ones, float c, f32x4 &mneg, f32x4 (&o)[5],
                                          int g, int c16)
{
    bool down = true;
    int s = step0;
    for (; s + 2 <= step1; s += 2) {
        attn_block2<DT, 2, false, QM>(ldsK, ldsV, 32 * s, S, qf, ones, down, c, mneg, o, g, c16);
        down = false;
    }
    if (s < step1) {
        attn_block2<DT, 1, false, QM>(ldsK, ldsV, 32 * s, S, qf, ones, down, c, mneg, o, g, c16);
        down = false;
    }
    if (tail) {
        const int full = S >> 5, nt = S - 32 * full;
        if (nt == 1)
            attn_odd_key<DT, QM>(ldsK, ldsV, S - 1, qf, down, c, mneg, o, g, c16);
        else if (nt > 1)
            attn_block2<DT, 1, true, QM>(ldsK, ldsV, 32 * full, S, qf, ones, down, c, mneg, o, g, c16);
    }
}

// Floats per wave in the merge area of a tile whose keys are split over the waves: O (64), m, l
constexpr int ATTN_PART = 66;
// Is the sequence's LAST query tile (a single row, S = 16 n + 1) split over the waves?  ONE predicate for the kernel (which
// writes the merge area behind the K / V images) and for the host (which reserves it): depends on S, the mask and the wave
// count alone, never on q_rows.
__host__ __device__ constexpr bool attn_lone_tile(int S, int causal, int waves)
{
    return !causal && (S & 15) == 1 && (S + 15) / 16 > waves && ((S + 15) / 16) % waves == 1;
}

// The split tile, shared by attention_kernel and attention_hl_kernel.  Its 32-key steps are dealt out evenly: wave w takes
// [s0, s1) -- none, where there are fewer steps than waves -- and the last wave also what lies behind the last full step.
template <int WAVES> __device__ __forceinline__ void lone_share(int S, int wave, int &s0, int &s1, bool &tail)
{
    const int steps = S >> 5;
    s0 = wave * steps / WAVES, s1 = (wave + 1) * steps / WAVES;
    tail = wave == WAVES - 1;
}
// This wave's partial (O, m in log2 units, l) of the tile's one valid query (row S - 1: lanes 0, 16, 32, 48, head dims
// 16 g .. 16 g + 15 each) into the merge area; a barrier, then lone_merge
__device__ __forceinline__ void lone_put(float *part, int wave, int g, int c16, const f32x4 (&o)[5], float m_log2, bool has_keys)
{
    if (c16 == 0) {
        float *dst = part + wave * ATTN_PART;
#pragma unroll
        for (int dt = 0; dt < 4; dt++) *reinterpret_cast<f32x4 *>(dst + 16 * g + 4 * dt) = o[dt];
        if (g == 0) {
            dst[64] = has_keys ? m_log2 : -1e30f;   // a wave without keys: weight 0
            dst[65] = o[4][0];
        }
    }
}
// One wave merges, lane = head dim: the output is num / den, the row's log-sum-exp (log2) m + log2 den
struct LoneRow {
    float num, den, m;
};
template <int WAVES> __device__ __forceinline__ LoneRow lone_merge(const float *part, int lane)
{
    float m = -1e30f;
#pragma unroll
    for (int w = 0; w < WAVES; w++) m = fmaxf(m, part[w * ATTN_PART + 64]);
    const float *col = part + lane;
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const float f = __builtin_amdgcn_exp2f(part[w * ATTN_PART + 64] - m);
        num = __builtin_fmaf(f, col[w * ATTN_PART], num);
        den = __builtin_fmaf(f, part[w * ATTN_PART + 65], den);
    }
    return LoneRow{num, den, m};
}

template <int DT, int AT_WAVES, bool LSE = false, int QM = (DT == 0 ? QM_KERNEL : QM_RAW)>
__global__ __launch_bounds__(AT_WAVES * 64, 4) void attention_kernel(const AttnArgs a)
{
    typedef typename T16<DT>::elem elem;
    typedef typename T16<DT>::v8 v8;

    constexpr int AT_THREADS = AT_WAVES * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int S = a.S, W = a.W;
    const int n32 = (S + 31) / 32;       // 32-key steps; keys padded to 32 * n32
    const int SP = 32 * n32;
    unsigned char *ldsK = smem;
    unsigned char *ldsV = smem + SP * 128;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g_lane = lane >> 4, c_lane = lane & 15;
    const int head = blockIdx.x % a.heads, seq = blockIdx.x / a.heads;
    const long ld = 3L * W;
    const elem *base = (const elem *)a.qkv + (long)seq * S * ld + head * 64;
    attn_stamp(0);

    // ---- stage K and V of this head: AT_THREADS / 8 rows x 8 chunks of 16 B per pass, at most five passes
    // (room for 320 rows on 8 waves, 640 on 16; dispatch() sends S <= 288 to 8 waves and 289 .. 640 to 16).
    // Every load of the head is requested before the first LDS write, so the staging costs one memory round
    // trip instead of one per pass (a third of a workgroup's life at S = 257 otherwise) ----
    {
        const int r_in = threadIdx.x >> 3, ch = threadIdx.x & 7;
        u32x4 kv[5], vv[5];
#pragma unroll
        for (int p = 0; p < 5; p++) {
            const int row = r_in + p * (AT_THREADS / 8);
            if (row < SP) {
                const int srow = row < S ? row : S - 1;  // padded keys: finite data, masked below
                const elem *src = base + (long)srow * ld + ch * 8;
                kv[p] = *reinterpret_cast<const u32x4 *>(src + W);
                vv[p] = *reinterpret_cast<const u32x4 *>(src + 2 * W);
            }
        }
#pragma unroll
        for (int p = 0; p < 5; p++) {
            const int row = r_in + p * (AT_THREADS / 8);
            if (row < SP) {
                *reinterpret_cast<u32x4 *>(ldsK + row * 128 + k_chunk(row, ch)) = kv[p];
                v_put(ldsV, row, ch, vv[p]);
            }
        }
    }
    // Query tiles.  A sequence of 16 n + 1 tokens whose tile count leaves ONE tile over after whole rounds of
    // the waves (S = 257 on 8 waves: 17 tiles) would keep seven waves idle for a third round that holds a
    // single query row: that tile's KEYS are split over all waves instead and the partial (m, l, O) merged
    // through LDS (not causal).  Whether a tile is split depends on S alone, never on q_rows, so
    // ec_attention_rows stays a bit-exact prefix of ec_attention.
    const int n_qt_all = (S + 15) / 16;
    const bool lone = attn_lone_tile(S, a.causal, AT_WAVES);
    const int n_qt_req = (a.q_rows + 15) / 16;                           // tiles the caller asked for
    const int n_qt = lone ? min(n_qt_req, n_qt_all - 1) : n_qt_req;      // ... that are walked tile by tile
    const bool do_lone = lone && n_qt_req == n_qt_all;
    // first Q tile of this wave, issued before the barrier so its latency hides behind staging
    v8 qf[2], qn[2];
    auto load_q = [&](int qt, v8(&dst)[2]) {
        int qsrc = qt * 16 + c_lane;
        qsrc = qsrc < S ? qsrc : S - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
            dst[ks] = *reinterpret_cast<const v8 *>(base + (long)qsrc * ld + ks * 32 + g_lane * 8);
    };
    if (wave < n_qt)
        load_q(wave, qn);
    else if (do_lone)
        load_q(n_qt_all - 1, qn);
    __syncthreads();
    attn_stamp(1);

    const v8 ones = ones16<DT>();
    // q <- q * log2(e) / sqrt(64), rounded to the operand type once per tile
    auto scale_q = [&](v8(&q)[2]) {
        if (QM != QM_KERNEL) return;
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int j = 0; j < 8; j++) q[ks][j] = to16((float)q[ks][j] * a.scale_log2e, elem());
    };
    for (int qt = wave; qt < n_qt; qt += AT_WAVES) {
        qf[0] = qn[0], qf[1] = qn[1];
        // prefetch the next tile's Q (after the last one: the split tile's)
        if (qt + AT_WAVES < n_qt)
            load_q(qt + AT_WAVES, qn);
        else if (do_lone)
            load_q(n_qt_all - 1, qn);
        const int qrow = qt * 16 + c_lane;
        // lane coordinates made opaque per tile: otherwise hipcc hoists the per-lane LDS addresses of EVERY
        // block variant out of the tile loop, keeps them live across it and spills (scratch reloads in the
        // tile path cost a memory round trip each)
        int g = g_lane, c16 = c_lane;
        asm volatile("" : "+v"(g), "+v"(c16));
        f32x4 o[5];
#pragma unroll
        for (int dt = 0; dt < 5; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 mneg = f32x4{0.f, 0.f, 0.f, 0.f};
        scale_q(qf);
        if (!a.causal) {
            attn_keys<DT, QM>(ldsK, ldsV, S, 0, S >> 5, true, qf, ones, a.scale_log2e, mneg, o, g, c16);
        } else {
            const int klimit = qrow < S ? qrow + 1 : S;   // keys < klimit are visible
            // rows of this tile see no key beyond 16 qt + 15: skip the blocks past it; blocks entirely
            // below every lane's klimit (16 qt + 1 ..) need no masking
            const int kend = min(SP, ((qt * 16 + 16 + 31) / 32) * 32);
            const int kfree = min(qt * 16 + 1, kend);
            bool down = true;
            int key0 = 0;
            for (; key0 + 64 <= kfree; key0 += 64, down = false)
                attn_block2<DT, 2, false, QM>(ldsK, ldsV, key0, klimit, qf, ones, down, a.scale_log2e, mneg, o, g, c16);
            for (; key0 + 64 <= kend; key0 += 64, down = false)
                attn_block2<DT, 2, true, QM>(ldsK, ldsV, key0, klimit, qf, ones, down, a.scale_log2e, mneg, o, g, c16);
            if (key0 < kend)
                attn_block2<DT, 1, true, QM>(ldsK, ldsV, key0, klimit, qf, ones, down, a.scale_log2e, mneg, o, g, c16);
        }
        // softmax denominator (every row of the ones tile carries the query's row sum) and maximum (log2 domain,
        // scaled scores)
        const float lsum = o[4][0];
        const float m_log2 = QM != QM_RAW ? -mneg[0] : -mneg[0] * a.scale_log2e;

        // ---- normalise and store: lane owns query c16, head dims 16 g .. 16 g + 15 ----
        const float inv = 1.f / lsum;
        if (LSE && qrow < a.q_rows && g == 0)
            a.lse[((long)seq * a.heads + head) * S + qrow] = m_log2 + __builtin_amdgcn_logf(lsum);
        if (qrow < a.q_rows) {
            elem ov[16];
#pragma unroll
            for (int dt = 0; dt < 4; dt++)
#pragma unroll
                for (int r = 0; r < 4; r++) ov[4 * dt + r] = to16(o[dt][r] * inv, elem());
            elem *dst = (elem *)a.out + ((long)seq * a.q_rows + qrow) * W + head * 64 + g * 16;
            *reinterpret_cast<u32x4 *>(dst) = *reinterpret_cast<const u32x4 *>(&ov[0]);
            *reinterpret_cast<u32x4 *>(dst + 8) = *reinterpret_cast<const u32x4 *>(&ov[8]);
        }
    }
    if (do_lone) {
        // ---- the tile left over: this wave's share of its keys, then the merge ----
        float *part = reinterpret_cast<float *>(smem + 2 * SP * 128);
        int s0, s1;
        bool tail;
        lone_share<AT_WAVES>(S, wave, s0, s1, tail);
        int g = g_lane, c16 = c_lane;
        asm volatile("" : "+v"(g), "+v"(c16));
        qf[0] = qn[0], qf[1] = qn[1];
        scale_q(qf);
        f32x4 o[5];
#pragma unroll
        for (int dt = 0; dt < 5; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 mneg = f32x4{0.f, 0.f, 0.f, 0.f};
        attn_keys<DT, QM>(ldsK, ldsV, S, s0, s1, tail, qf, ones, a.scale_log2e, mneg, o, g, c16);
        lone_put(part, wave, g, c16, o, QM != QM_RAW ? -mneg[0] : -mneg[0] * a.scale_log2e, s1 > s0 || tail);
        __syncthreads();
        if (wave == 0) {
            const LoneRow r = lone_merge<AT_WAVES>(part, lane);
            const int qrow = S - 1;
            ((elem *)a.out)[((long)seq * a.q_rows + qrow) * W + head * 64 + lane] = to16(r.num / r.den, elem());
            if (LSE && lane == 0)
                a.lse[((long)seq * a.heads + head) * S + qrow] = r.m + __builtin_amdgcn_logf(r.den);
        }
    }
    attn_stamp(2);
#ifdef EC_ATTN_DIAG
    if (threadIdx.x == 0 && blockIdx.x < 65536) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        ec_attn_stamps[blockIdx.x * 4 + 3] = ((unsigned long long)xcc << 32) | hw;
    }
#endif
}


// ---------------------------------------------------------------------------------------
// Attention on hi + lo fp16 operands (round 5): the fp32-class attention of the tolerance mode's first blocks
// (ec_vit_weights.precise_attn_blocks) on the 16-bit matrix instruction instead of the fp32 one -- 2.5 PFLOP/s against
// 157 TFLOP/s of peak, three products per tile:
//   scores   s = q_hi k_hi + q_lo k_hi + q_hi k_lo            (q = c (q_hi + q_lo) re-split in registers, c = log2 e / 8)
//   P V      o += v_hi p_hi + v_hi p_lo + v_lo p_hi,  l += 1 p_hi + 1 p_lo     (p = exp2(s - m) as p_hi + p_lo)
// (the lo . lo products, 2^-22 of the result, are left out).  Structure of attention_kernel: one 8-wave workgroup per
// (sequence, head), K_hi, K_lo, V_hi, V_lo of the head in LDS (4 x S x 128 B: S <= 288 in 160 KiB -- longer sequences take
// ec_attention_split's fp32 kernel), S^T = K Q^T so that a lane holds one query column, P as the B operand of O^T = V^T P^T,
// the running maximum that moves only when a score exceeds it by 2^10, the odd key of S = 32 n + 1 as a rank-one update (in
// fp32 on the vector ALU), the lone 17th tile of S = 257 split over the waves.  Plain builtin MFMAs and plain C++ for the
// seldom-taken rescale (no inline-asm accumulators: nothing for tools/check_attn_isa.py to check here).
// ---------------------------------------------------------------------------------------
struct AttnHlArgs {
    const _Float16 *qkv_hi, *qkv_lo;   // [n_seq * S, 3W]: q | k | v, a PLAIN q
    _Float16 *out_hi, *out_lo;         // [n_seq * S, W]
    int S, W, heads;
};

// attn_move's job in plain C++.  The two stay separate on purpose: attn_move is tied-operand asm, because attention_kernel's
// accumulators must not leave their registers; here the MFMAs are builtins and the compiler is free to place O.
__device__ __forceinline__ void hl_move(float d, bool down, f32x4 &mneg, f32x4 (&o)[5])
{
    float alpha = __builtin_amdgcn_exp2f(-d);
    alpha = down ? 0.f : alpha;
#pragma unroll
    for (int dt = 0; dt < 5; dt++) o[dt] *= alpha;
    mneg -= d;
}

// one 32-key step.  `down`: the tile has added nothing yet (m may move down too)
template <bool MASK>
__device__ __forceinline__ void attn_step_hl(const unsigned char *kh, const unsigned char *kl, const unsigned char *vh,
                                             const unsigned char *vl, int key0, int klimit, const f16x8 (&qh)[2],
                                             const f16x8 (&ql)[2], const f16x8 &ones, bool down, f32x4 &mneg, f32x4 (&o)[5],
                                             int g, int c16)
{
    f32x4 acc[2];
#pragma unroll
    for (int kt = 0; kt < 2; kt++) {
        const int row = key0 + kt * 16 + c16;
        const int o0 = row * 128 + k_chunk(row, 0 + g), o1 = row * 128 + k_chunk(row, 4 + g);
        const f16x8 k0h = *reinterpret_cast<const f16x8 *>(kh + o0), k1h = *reinterpret_cast<const f16x8 *>(kh + o1);
        const f16x8 k0l = *reinterpret_cast<const f16x8 *>(kl + o0), k1l = *reinterpret_cast<const f16x8 *>(kl + o1);
        f32x4 a = mfma16(k0l, qh[0], mneg);       // the small products first
        a = mfma16(k1l, qh[1], a);
        a = mfma16(k0h, ql[0], a);
        a = mfma16(k1h, ql[1], a);
        a = mfma16(k0h, qh[0], a);
        acc[kt] = mfma16(k1h, qh[1], a);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (MASK) {
                const int key = key0 + kt * 16 + 4 * g + r;
                acc[kt][r] = key < klimit ? acc[kt][r] : -INFINITY;
            }
            mx = fmaxf(mx, acc[kt][r]);
        }
    if (__builtin_amdgcn_ballot_w64(mx > ATTN_THR || (down && mx < -ATTN_LO)) != 0) {
        const float mq = xor_max(mx);
        const float d = (mq > ATTN_THR || (down && mq < -ATTN_LO)) ? mq : 0.f;      // only the queries that need it move
        acc[0] -= d, acc[1] -= d;
        hl_move(d, down, mneg, o);
    }
    // V^T fragments of both parts: A operand row i <-> head dim (i >> 2) * 16 + 4 dt + (i & 3)
    f16x8 vfh[4], vfl[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++)
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int row = key0 + 16 * hh + 4 * g + (c16 >> 2);
            const int off = row * 128 + v_slot(row, (c16 & 3) * 4 + dt);
            const f16x4 th = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vh + off)));
            const f16x4 tl = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vl + off)));
#pragma unroll
            for (int e = 0; e < 4; e++) vfh[dt][4 * hh + e] = th[e], vfl[dt][4 * hh + e] = tl[e];
        }
    // P = exp2(s - m) as hi + lo; B operand element j <-> key key0 + 16 (j >> 2) + 4 g + (j & 3)
    f16x8 ph, pl;
#pragma unroll
    for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float pv = __builtin_amdgcn_exp2f(acc[kt][r]);
            const _Float16 h = (_Float16)pv;
            ph[4 * kt + r] = h;
            pl[4 * kt + r] = (_Float16)(pv - (float)h);
        }
    o[4] = mfma16(ones, pl, o[4]);
    o[4] = mfma16(ones, ph, o[4]);
#pragma unroll
    for (int dt = 0; dt < 4; dt++) {
        f32x4 t = mfma16(vfl[dt], ph, o[dt]);
        t = mfma16(vfh[dt], pl, t);
        o[dt] = mfma16(vfh[dt], ph, t);
    }
}

// the single key behind the last full step (S = 32 n + 1): the LDS rows behind it are copies of it, so every accumulator
// register of a lane is the lane's query against THIS key; P V in fp32 on the vector ALU (no rounding of p at all)
__device__ __forceinline__ void attn_odd_key_hl(const unsigned char *kh, const unsigned char *kl, const unsigned char *vh,
                                                const unsigned char *vl, int key, const f16x8 (&qh)[2], const f16x8 (&ql)[2],
                                                bool down, f32x4 &mneg, f32x4 (&o)[5], int g, int c16)
{
    const int row = key + c16;
    const int o0 = row * 128 + k_chunk(row, 0 + g), o1 = row * 128 + k_chunk(row, 4 + g);
    const f16x8 k0h = *reinterpret_cast<const f16x8 *>(kh + o0), k1h = *reinterpret_cast<const f16x8 *>(kh + o1);
    const f16x8 k0l = *reinterpret_cast<const f16x8 *>(kl + o0), k1l = *reinterpret_cast<const f16x8 *>(kl + o1);
    f16x4 vvh[4], vvl[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++) {      // logical 8-byte slot 4 g + dt of V's row
        const int off = key * 128 + v_slot(key, 4 * g + dt);
        vvh[dt] = *reinterpret_cast<const f16x4 *>(vh + off), vvl[dt] = *reinterpret_cast<const f16x4 *>(vl + off);
    }
    f32x4 a = mfma16(k0l, qh[0], mneg);
    a = mfma16(k1l, qh[1], a);
    a = mfma16(k0h, ql[0], a);
    a = mfma16(k1h, ql[1], a);
    a = mfma16(k0h, qh[0], a);
    a = mfma16(k1h, qh[1], a);
    float sc = a[0];
    if (__builtin_amdgcn_ballot_w64(sc > ATTN_THR || (down && sc < -ATTN_LO)) != 0) {
        const float d = (sc > ATTN_THR || (down && sc < -ATTN_LO)) ? sc : 0.f;
        sc -= d;
        hl_move(d, down, mneg, o);
    }
    const float pv = __builtin_amdgcn_exp2f(sc);
    o[4][0] += pv;
#pragma unroll
    for (int dt = 0; dt < 4; dt++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[dt][r] = __builtin_fmaf(pv, (float)vvh[dt][r] + (float)vvl[dt][r], o[dt][r]);
}

// keys of one tile: the full 32-key steps [step0, step1), then (`tail`) what lies behind the last full step
__device__ __forceinline__ void attn_keys_hl(const unsigned char *kh, const unsigned char *kl, const unsigned char *vh,
                                             const unsigned char *vl, int S, int step0, int step1, bool tail,
                                             const f16x8 (&qh)[2], const f16x8 (&ql)[2], const f16x8 &ones, f32x4 &mneg,
                                             f32x4 (&o)[5], int g, int c16, bool down = true)
{
    for (int s = step0; s < step1; s++) {
        attn_step_hl<false>(kh, kl, vh, vl, 32 * s, S, qh, ql, ones, down, mneg, o, g, c16);
        down = false;
    }
    if (tail) {
        const int full = S >> 5, nt = S - 32 * full;
        if (nt == 1)
            attn_odd_key_hl(kh, kl, vh, vl, S - 1, qh, ql, down, mneg, o, g, c16);
        else if (nt > 1)
            attn_step_hl<true>(kh, kl, vh, vl, 32 * full, S, qh, ql, ones, down, mneg, o, g, c16);
    }
}

constexpr int HL_WAVES = 8;

// Stage K_hi, K_lo, V_hi, V_lo of the keys [key0, key0 + n_keys) of the workgroup's head (`base`: its first q element) into
// `rows` LDS rows per plane; the rows behind the last key are copies of it.  HL_WAVES x 8 rows x 8 chunks of 16 B per pass,
// every load of a pass pair in flight before its LDS writes.
__device__ __forceinline__ void stage_hl(const AttnHlArgs &a, long base, unsigned char *kh, unsigned char *kl, unsigned char *vh,
                                         unsigned char *vl, int key0, int n_keys, int rows)
{
    constexpr int PASS = HL_WAVES * 64 / 8;
    const int W = a.W;
    const long ld = 3L * W;
    const int r_in = threadIdx.x >> 3, ch = threadIdx.x & 7;
    for (int p0 = 0; p0 < rows; p0 += 2 * PASS) {
        u32x4 t[2][4];
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const int row = p0 + r_in + p * PASS;
            if (row < rows) {
                const long src = base + (long)(key0 + (row < n_keys ? row : n_keys - 1)) * ld + ch * 8;
                t[p][0] = *reinterpret_cast<const u32x4 *>(a.qkv_hi + src + W), t[p][1] = *reinterpret_cast<const u32x4 *>(a.qkv_lo + src + W);
                t[p][2] = *reinterpret_cast<const u32x4 *>(a.qkv_hi + src + 2 * W), t[p][3] = *reinterpret_cast<const u32x4 *>(a.qkv_lo + src + 2 * W);
            }
        }
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const int row = p0 + r_in + p * PASS;
            if (row < rows) {
                const int ko = row * 128 + k_chunk(row, ch);
                *reinterpret_cast<u32x4 *>(kh + ko) = t[p][0];
                *reinterpret_cast<u32x4 *>(kl + ko) = t[p][1];
                v_put(vh, row, ch, t[p][2]);
                v_put(vl, row, ch, t[p][3]);
            }
        }
    }
}

// q of one tile: c (q_hi + q_lo) in fp32, split again (the softmax scale and the base change enter before the split)
__device__ __forceinline__ void load_q_hl(const AttnHlArgs &a, long base, int qt, int c_lane, int g_lane, f16x8 (&qh)[2],
                                          f16x8 (&ql)[2])
{
    constexpr float C = 0.125f * 1.4426950408889634f;
    const long ld = 3L * a.W;
    int qsrc = qt * 16 + c_lane;
    qsrc = qsrc < a.S ? qsrc : a.S - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
        const f16x8 h = *reinterpret_cast<const f16x8 *>(a.qkv_hi + base + (long)qsrc * ld + ks * 32 + g_lane * 8);
        const f16x8 l = *reinterpret_cast<const f16x8 *>(a.qkv_lo + base + (long)qsrc * ld + ks * 32 + g_lane * 8);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            _Float16 xh, xl;
            split16(((float)h[j] + (float)l[j]) * C, xh, xl);
            qh[ks][j] = xh, ql[ks][j] = xl;
        }
    }
}

// normalise a query's 16 head dims 16 g .. 16 g + 15 and store them as hi + lo; `row`: the query's row of out
__device__ __forceinline__ void store_hl(const AttnHlArgs &a, long row, int head, int g, const f32x4 (&o)[5])
{
    const float inv = 1.f / o[4][0];
    _Float16 hi[16], lo[16];
#pragma unroll
    for (int dt = 0; dt < 4; dt++)
#pragma unroll
        for (int r = 0; r < 4; r++) split16(o[dt][r] * inv, hi[4 * dt + r], lo[4 * dt + r]);
    const long off = row * a.W + head * 64 + g * 16;
    *reinterpret_cast<u32x4 *>(a.out_hi + off) = *reinterpret_cast<const u32x4 *>(&hi[0]);
    *reinterpret_cast<u32x4 *>(a.out_hi + off + 8) = *reinterpret_cast<const u32x4 *>(&hi[8]);
    *reinterpret_cast<u32x4 *>(a.out_lo + off) = *reinterpret_cast<const u32x4 *>(&lo[0]);
    *reinterpret_cast<u32x4 *>(a.out_lo + off + 8) = *reinterpret_cast<const u32x4 *>(&lo[8]);
}

__global__ __launch_bounds__(HL_WAVES * 64, 1) void attention_hl_kernel(const AttnHlArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int S = a.S, W = a.W;
    const int SP = 32 * ((S + 31) / 32);
    unsigned char *kh = smem, *kl = smem + SP * 128, *vh = smem + 2 * SP * 128, *vl = smem + 3 * SP * 128;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g_lane = lane >> 4, c_lane = lane & 15;
    const int head = blockIdx.x % a.heads, seq = blockIdx.x / a.heads;
    const long base = (long)seq * S * (3L * W) + head * 64;
    stage_hl(a, base, kh, kl, vh, vl, 0, S, SP);
    const int n_qt_all = (S + 15) / 16;
    const bool lone = attn_lone_tile(S, 0, HL_WAVES);
    const int n_qt = lone ? n_qt_all - 1 : n_qt_all;
    const f16x8 ones = ones16<EC_F16>();
    __syncthreads();
    for (int qt = wave; qt < n_qt; qt += HL_WAVES) {
        f16x8 qh[2], ql[2];
        load_q_hl(a, base, qt, c_lane, g_lane, qh, ql);
        int g = g_lane, c16 = c_lane;
        asm volatile("" : "+v"(g), "+v"(c16));
        f32x4 o[5];
#pragma unroll
        for (int dt = 0; dt < 5; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 mneg = f32x4{0.f, 0.f, 0.f, 0.f};
        attn_keys_hl(kh, kl, vh, vl, S, 0, S >> 5, true, qh, ql, ones, mneg, o, g, c16);
        const int qrow = qt * 16 + c16;
        if (qrow < S) store_hl(a, (long)seq * S + qrow, head, g, o);
    }
    if (lone) {
        // the tile left over (one query row): this wave's share of its keys, then the merge through LDS
        float *part = reinterpret_cast<float *>(smem + 4 * SP * 128);
        int s0, s1;
        bool tail;
        lone_share<HL_WAVES>(S, wave, s0, s1, tail);
        f16x8 qh[2], ql[2];
        load_q_hl(a, base, n_qt_all - 1, c_lane, g_lane, qh, ql);
        int g = g_lane, c16 = c_lane;
        asm volatile("" : "+v"(g), "+v"(c16));
        f32x4 o[5];
#pragma unroll
        for (int dt = 0; dt < 5; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 mneg = f32x4{0.f, 0.f, 0.f, 0.f};
        attn_keys_hl(kh, kl, vh, vl, S, s0, s1, tail, qh, ql, ones, mneg, o, g, c16);
        lone_put(part, wave, g, c16, o, -mneg[0], s1 > s0 || tail);
        __syncthreads();
        if (wave == 0) {
            const LoneRow r = lone_merge<HL_WAVES>(part, lane);
            _Float16 h, l;
            split16(r.num / r.den, h, l);
            const long off = ((long)seq * S + S - 1) * W + head * 64 + lane;
            a.out_hi[off] = h;
            a.out_lo[off] = l;
        }
    }
}

// The same for sequences whose four planes do not fit the LDS but half of them does (288 < S <= 608: S = 577): the keys in
// TWO passes of one workgroup -- stage K_hi, K_lo, V_hi, V_lo of keys [0, split), walk every query tile of the wave against
// them, stage the rest, walk the tiles again -- with each tile's (m, l, O) kept in registers between the passes (at most five
// tiles per wave x 24 registers: the 8-wave workgroup has 256 per lane).  No exchange, no merge: a tile's running maximum
// simply goes on where the first pass left it.
constexpr int HL2_TILES = 5;      // query tiles per wave at most: S <= 8 x 5 x 16 = 640
__global__ __launch_bounds__(HL_WAVES * 64, 1) void attention_hl2_kernel(const AttnHlArgs a, int split, int SPL)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int S = a.S, W = a.W;
    unsigned char *kh = smem, *kl = smem + SPL * 128, *vh = smem + 2 * SPL * 128, *vl = smem + 3 * SPL * 128;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g_lane = lane >> 4, c_lane = lane & 15;
    const int head = blockIdx.x % a.heads, seq = blockIdx.x / a.heads;
    const long base = (long)seq * S * (3L * W) + head * 64;
    const int n_qt = (S + 15) / 16;
    const f16x8 ones = ones16<EC_F16>();
    f32x4 o[HL2_TILES][5];
    float mneg[HL2_TILES];          // (-m of a tile: one register between the passes, the MFMA's C operand inside one)
#pragma unroll
    for (int t = 0; t < HL2_TILES; t++) {
        mneg[t] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 5; dt++) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int half = 0; half < 2; half++) {
        const int key0 = half ? split : 0, Sl = half ? S - split : split;
        if (half) __syncthreads();      // every wave is done with the first pass's planes
        stage_hl(a, base, kh, kl, vh, vl, key0, Sl, SPL);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < HL2_TILES; t++) {
            const int qt = wave + HL_WAVES * t;
            if (qt < n_qt) {      // (wave-uniform)
                f16x8 qh[2], ql[2];
                load_q_hl(a, base, qt, c_lane, g_lane, qh, ql);
                int g = g_lane, c16 = c_lane;
                asm volatile("" : "+v"(g), "+v"(c16));
                f32x4 mn = f32x4{mneg[t], mneg[t], mneg[t], mneg[t]};
                attn_keys_hl(kh, kl, vh, vl, Sl, 0, Sl >> 5, true, qh, ql, ones, mn, o[t], g, c16, half == 0);
                mneg[t] = mn[0];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < HL2_TILES; t++) {
        const int qt = wave + HL_WAVES * t, qrow = qt * 16 + c_lane;
        if (qt < n_qt && qrow < S) store_hl(a, (long)seq * S + qrow, head, g_lane, o[t]);
    }
}

template <int DT> int dispatch(const AttnArgs &a, int n_seq, hipStream_t s)
{
    const int n32 = (a.S + 31) / 32;
    // K and V images, plus the merge area of a tile whose keys are split over the waves -- reserved only where the
    // kernel can take that path for this S (its `lone` condition: not causal, S = 16 n + 1, the tile count one more
    // than a multiple of the wave count), so that S = 609 .. 640 (n32 = 20: exactly 160 KiB of K and V) still fits
    const int kv = 32 * n32 * 128 * 2;
    // Waves per workgroup: 16 when K + V (and the merge area: the full carve) leave room for one workgroup per CU only,
    // else 8.  (9..12 waves, which would spread the 17 query tiles of S = 257 over two even passes, measure 0.22 ms
    // against 0.17 ms for 8: the second workgroup no longer co-resides.)
    const bool wide = kv + 16 * ATTN_PART * 4 > 80 * 1024;
    const bool may_split = attn_lone_tile(a.S, a.causal, wide ? 16 : 8);
    const int lds = kv + (may_split ? 16 * ATTN_PART * 4 : 0);
    if (lds > 160 * 1024)
        return ec::fail(EC_ERR_UNSUPPORTED, "ec_attention: sequence length %d needs %d bytes of LDS (K and V images%s), "
                        "the CU has 163840: S <= 640%s", a.S, lds, may_split ? " + the split-tile merge area" : "",
                        may_split ? " (608 for this S, whose last query tile is split over the waves)" : "");
    // The kernel by [q_scaled, or 3 for a log-sum-exp][wide]:
    //  0  the type's default QM
    //  1  the inference towers (never with a log-sum-exp)
    //  2  a plain q, every score scaled in fp32: q is rounded ONCE (the split-operand blocks behind the
    //     fp32-attention ones; QM_KERNEL's second rounding of q cost configs[2] 30 % there)
    //  3  the type's default QM with the log-sum-exp (ec_attention_train: q_scaled = 0)
    static void (*const table[4][2])(const AttnArgs) = {
        {attention_kernel<DT, 8>, attention_kernel<DT, 16>},
        {attention_kernel<DT, 8, false, QM_INPUT>, attention_kernel<DT, 16, false, QM_INPUT>},
        {attention_kernel<DT, 8, false, QM_RAW>, attention_kernel<DT, 16, false, QM_RAW>},
        {attention_kernel<DT, 8, true>, attention_kernel<DT, 16, true>}};
    void (*const kern)(const AttnArgs) = table[a.lse && a.q_scaled == 0 ? 3 : a.q_scaled][wide];
    const int nw = wide ? 16 : 8;
    // always the full carve (one attribute call per kernel and device, thread-safe)
    if (int rc = ec::ensure_dynamic_lds(reinterpret_cast<const void *>(kern), 160 * 1024)) return rc;
    // algorithmic work: QK^T and PV, 2 * 2 * S^2 * 64 flops per head; bytes: read qkv, write out
    ec::ProfScope prof(ec::PROF_ATTENTION, s, 4.0 * a.q_rows * a.S * 64.0 * a.heads * n_seq,
                       (double)n_seq * a.W * 2.0 * (2.0 * a.S + 2.0 * a.q_rows));
    hipLaunchKernelGGL(kern, dim3((unsigned)a.heads * (unsigned)n_seq), dim3(nw * 64), lds, s, a);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}


// ---------------------------------------------------------------------------------------
// fp32 attention for the split-precision towers on the fp32 matrix instruction (round 4): v_mfma_f32_16x16x4_f32 takes fp32 operands and is bit for bit an
// fmaf chain (cdna_hip_programming.md, FP32-input MFMA), at the vector ALU's peak rate but with the operands read
// once per 16 x 16 tile instead of once per product.  One workgroup = 64 queries of one (sequence, head), one
// 16-query tile per wave, keys in chunks of 32 through two LDS buffers (the next chunk's rows are in flight in
// registers during the chunk's MFMAs; one barrier per chunk), online softmax in fp32 (e^t through v_exp_f32, see exp_e).
//  * S^T = K . Q^T: A = the chunk's key rows (lane: key l & 15, head dims 16 c + 4 (l >> 4) + e), B = the wave's
//    queries in the same dim order (held in registers, pre-scaled by 1/8: exact), so a lane's accumulators are four
//    keys (4 (l >> 4) + r of each 16-key tile) of ONE query (l & 15);
//  * O^T += V^T . P^T: step (t, r) takes the keys 16 t + 4 g + r (g = 0 .. 3), whose P values are exactly register r of
//    tile t in lane group g: no lane movement; A = V read down its columns (one float per lane and step).
// LDS rows are 64 floats with the 16-byte chunk index XORed with row & 15: the 16 key rows of a b128 read and the
// column reads of V are spread over the banks.  2560 sequences x 16 heads x S = 257: 96 ms -> see profiles/r4_attention.md.
// ---------------------------------------------------------------------------------------
// SIN (round 5, the split-operand blocks of ec_vit_weights.precise_attn_blocks): q | k | v arrive as hi + lo 16-bit parts
// (two [rows, 3W] tensors, what EC_EPI_STORE16 leaves with args.aux) and are joined to fp32 on the way in.  PRE: the q
// columns already hold q log2(e) / sqrt(64) (ec_vit_weights.q_scaled), so the scores are the exponent's arguments in
// log2 units and e^t is one v_exp_f32.
constexpr int F32_KCH = 32;
template <int DT, bool SIN = false, bool PRE = false>
__global__ __launch_bounds__(256) void attention_f32m_kernel(const void *qkv_v, const void *qkv_lo_v, void *out_hi, void *out_lo,
                                                             int S, int W, int heads, int causal)
{
    typedef typename T16<DT>::elem elem;
    typedef typename T16<DT>::v4 v4;
    typedef typename std::conditional<SIN, elem, float>::type in_t;
    const in_t *qkv = static_cast<const in_t *>(qkv_v), *qkv_lo = static_cast<const in_t *>(qkv_lo_v);
    // four consecutive values of q | k | v at element offset `off` as fp32 (SIN: hi + lo)
    auto ld4 = [&](long off) -> f32x4 {
        if constexpr (SIN) {
            const v4 h = *reinterpret_cast<const v4 *>(qkv + off), l = *reinterpret_cast<const v4 *>(qkv_lo + off);
            return f32x4{(float)h[0] + (float)l[0], (float)h[1] + (float)l[1], (float)h[2] + (float)l[2], (float)h[3] + (float)l[3]};
        } else {
            return *reinterpret_cast<const f32x4 *>(qkv + off);
        }
    };
    __shared__ __attribute__((aligned(16))) float lk[2][F32_KCH * 64];
    __shared__ __attribute__((aligned(16))) float lv[2][F32_KCH * 64];
    const int n_qb = (S + 63) / 64;
    const int qb = blockIdx.x % n_qb, head = (blockIdx.x / n_qb) % heads, seq = blockIdx.x / (n_qb * heads);
    const long ld = 3L * W;
    const long base = (long)seq * S * ld + head * 64;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, j = lane & 15, g = lane >> 4;
    const int q0 = qb * 64 + wave * 16;
    const bool active = q0 < S;                    // wave-uniform: the tile has a query that exists
    const int query = q0 + j, qsrc = query < S ? query : S - 1;
    f32x4 qf[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const f32x4 v = ld4(base + (long)qsrc * ld + 16 * c + 4 * g);
        qf[c] = PRE ? v : v * 0.125f;
    }
    // keys this workgroup needs: all of them, or (causal) those up to its last query
    const int s_eff = causal ? (qb * 64 + 64 < S ? qb * 64 + 64 : S) : S;
    const int nch = (s_eff + F32_KCH - 1) / F32_KCH;
    // staging: thread -> (key row, 16-byte chunk) pairs idx = t, t + 256 of the chunk's 32 x 16
    f32x4 rk[2], rv[2];
    auto fetch = [&](int ch) {
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int idx = t + 256 * n, key = ch * F32_KCH + (idx >> 4);
            const int ks = key < S ? key : S - 1;
            const long src = base + (long)ks * ld + (idx & 15) * 4;
            rk[n] = ld4(src + W);
            rv[n] = ld4(src + 2 * W);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int idx = t + 256 * n, row = idx >> 4, chunk = (idx & 15) ^ (row & 15);
            *reinterpret_cast<f32x4 *>(&lk[buf][row * 64 + chunk * 4]) = rk[n];
            *reinterpret_cast<f32x4 *>(&lv[buf][row * 64 + chunk * 4]) = rv[n];
        }
    };
    float m = -INFINITY, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // e^t as 2^(t log2 e) on v_exp_f32 (1 ulp), the product with log2 e = hi + lo carried to ~2^-48 relative (one fma):
    // three vector instructions and one transcendental instead of expf's twenty, the same accuracy class
    auto exp_e = [](float t) {
        if constexpr (PRE) return __builtin_amdgcn_exp2f(t);
        return __builtin_amdgcn_exp2f(__builtin_fmaf(t, 1.4426950216293335f, t * 1.92596298909109e-8f));
    };
    fetch(0);
    stash(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ch++) {
        const int buf = ch & 1;
        if (ch + 1 < nch) fetch(ch + 1);
        if (active) {
            const float *K = lk[buf], *V = lv[buf];
            f32x4 sc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                f32x4 kf[2];
#pragma unroll
                for (int tt = 0; tt < 2; tt++) {
                    const int row = tt * 16 + j;
                    kf[tt] = *reinterpret_cast<const f32x4 *>(K + row * 64 + (((4 * c + g) ^ (row & 15)) << 2));
                }
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int tt = 0; tt < 2; tt++)
                        sc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[tt][e], qf[c][e], sc[tt], 0, 0, 0);
            }
            float mx = -INFINITY;
#pragma unroll
            for (int tt = 0; tt < 2; tt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int key = ch * F32_KCH + tt * 16 + 4 * g + r;
                    const bool ok = key < S && (!causal || key <= query);
                    sc[tt][r] = ok ? sc[tt][r] : -INFINITY;
                    mx = fmaxf(mx, sc[tt][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);
            // nothing of this query's row seen so far (mn = -inf: only rows that do not exist or a causal row whose
            // keys all lie ahead, which cannot happen from chunk 0 on): keep everything at zero
            const float alpha = mn == -INFINITY ? 0.f : exp_e(m - mn);
            const float sub = mn == -INFINITY ? 0.f : mn;
            float ps = 0.f;
#pragma unroll
            for (int tt = 0; tt < 2; tt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    sc[tt][r] = exp_e(sc[tt][r] - sub);
                    ps += sc[tt][r];
                }
            l = l * alpha + ps;
            m = mn;
#pragma unroll
            for (int dt = 0; dt < 4; dt++) o[dt] *= alpha;
#pragma unroll
            for (int tt = 0; tt < 2; tt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = tt * 16 + 4 * g + r;
#pragma unroll
                    for (int dt = 0; dt < 4; dt++) {
                        const float a = V[row * 64 + (((4 * dt + (j >> 2)) ^ (row & 15)) << 2) + (j & 3)];
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sc[tt][r], o[dt], 0, 0, 0);
                    }
                }
        }
        if (ch + 1 < nch) stash(buf ^ 1);
        __syncthreads();
    }
    if (active) {
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (query < S) {
            const float inv = 1.f / l;
#pragma unroll
            for (int dt = 0; dt < 4; dt++) {
                v4 hi, lo;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    elem h, l;
                    split16(o[dt][r] * inv, h, l);
                    hi[r] = h, lo[r] = l;
                }
                const long off = ((long)seq * S + query) * W + head * 64 + 16 * dt + 4 * g;
                *reinterpret_cast<v4 *>((elem *)out_hi + off) = hi;
                *reinterpret_cast<v4 *>((elem *)out_lo + off) = lo;
            }
        }
    }
}

}  // namespace

#ifdef EC_ATTN_DIAG
// diagnostic build only (not part of the public header): copy the stamp records to the host
extern "C" __attribute__((visibility("default"))) int ec_attn_stamps_read(unsigned long long *host, int n)
{
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(ec_attn_stamps), (size_t)n * 8) == hipSuccess ? 0 : 1;
}
#endif

// the checks every entry point makes first, under the entry point's own name
static int check_shape(const char *api, int n_seq, int S, int width, int heads)
{
    EC_REQUIRE(n_seq >= 0 && S > 0 && heads > 0, "%s: bad shape", api);
    EC_REQUIRE(width == heads * 64, "%s: head dim must be 64 (width %d, heads %d)", api, width, heads);
    return EC_OK;
}

static AttnArgs make_args(const void *qkv, void *out, float *lse, int S, int width, int heads, int causal, int q_rows, int q_scaled)
{
    AttnArgs a;
    a.qkv = qkv, a.out = out, a.S = S, a.W = width, a.heads = heads, a.causal = causal;
    a.q_rows = q_rows;
    a.lse = lse;
    a.scale_log2e = 0.125f * 1.4426950408889634f;
    a.q_scaled = q_scaled;
    return a;
}

static int launch16(const char *api, const AttnArgs &a, int n_seq, int dtype, ec_stream_t stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == EC_F16) return dispatch<EC_F16>(a, n_seq, s);
    if (dtype == EC_BF16) return dispatch<EC_BF16>(a, n_seq, s);
    return ec::fail(EC_ERR_INVALID, "%s: unknown dtype %d", api, dtype);
}

// ec_attention_rows and ec_attention_scaled_q
static int attention_rows(const char *api, const void *qkv, void *out, int n_seq, int S, int width, int heads, int causal,
                          int q_rows, int q_scaled, int dtype, ec_stream_t stream)
{
    if (int rc = check_shape(api, n_seq, S, width, heads)) return rc;
    EC_REQUIRE(q_rows >= 1 && q_rows <= S, "%s: q_rows=%d outside 1..%d", api, q_rows, S);
    if (n_seq == 0) return EC_OK;
    EC_REQUIRE(qkv && out, "%s: null buffer", api);
    return launch16(api, make_args(qkv, out, nullptr, S, width, heads, causal, q_rows, q_scaled), n_seq, dtype, stream);
}

// tower_ops.h: a plain q whose scores are scaled in fp32 (no second rounding of q), no mask
int ec_tower::attention_exact_scale(const void *qkv, void *out, int n_seq, int S, int width, int heads, int dtype,
                                    ec_stream_t stream)
{
    return attention_rows("attention_exact_scale", qkv, out, n_seq, S, width, heads, 0, S, 2, dtype, stream);
}

extern "C" EC_API int ec_attention(const void *qkv, void *out, int n_seq, int S, int width,
                                   int heads, int causal, int dtype, ec_stream_t stream)
{
    return ec_attention_rows(qkv, out, n_seq, S, width, heads, causal, S, dtype, stream);
}

extern "C" EC_API int ec_attention_rows(const void *qkv, void *out, int n_seq, int S, int width,
                                        int heads, int causal, int q_rows, int dtype,
                                        ec_stream_t stream)
{
    return attention_rows("ec_attention", qkv, out, n_seq, S, width, heads, causal, q_rows, 0, dtype, stream);
}

extern "C" EC_API int ec_attention_scaled_q(const void *qkv, void *out, int n_seq, int S, int width, int heads,
                                            int causal, int q_rows, int dtype, ec_stream_t stream)
{
    return attention_rows("ec_attention_scaled_q", qkv, out, n_seq, S, width, heads, causal, q_rows, 1, dtype, stream);
}

extern "C" EC_API int ec_attention_train(const void *qkv, void *out, float *lse, int n_seq, int S, int width,
                                         int heads, int dtype, ec_stream_t stream)
{
    if (int rc = check_shape("ec_attention_train", n_seq, S, width, heads)) return rc;
    if (n_seq == 0) return EC_OK;
    EC_REQUIRE(qkv && out && lse, "ec_attention_train: null buffer");
    return launch16("ec_attention_train", make_args(qkv, out, lse, S, width, heads, 0, S, 0), n_seq, dtype, stream);
}

extern "C" EC_API int ec_attention_f32(const float *qkv, void *out_hi, void *out_lo, int n_seq, int S,
                                       int width, int heads, int causal, int dtype,
                                       ec_stream_t stream)
{
    if (int rc = check_shape("ec_attention_f32", n_seq, S, width, heads)) return rc;
    if (n_seq == 0) return EC_OK;
    EC_REQUIRE(qkv && out_hi && out_lo, "ec_attention_f32: null buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ec::ProfScope prof(ec::PROF_ATTENTION, s, 4.0 * S * S * 64.0 * heads * n_seq, 0);
    const long blocks = (long)n_seq * heads * ((S + 63) / 64);
    EC_REQUIRE(blocks < (1L << 31), "ec_attention_f32: %ld workgroups", blocks);
    if (dtype == EC_F16)
        hipLaunchKernelGGL((attention_f32m_kernel<EC_F16, false, false>), dim3((unsigned)blocks), dim3(256), 0, s, qkv, nullptr, out_hi,
                           out_lo, S, width, heads, causal);
    else if (dtype == EC_BF16)
        hipLaunchKernelGGL((attention_f32m_kernel<EC_BF16, false, false>), dim3((unsigned)blocks), dim3(256), 0, s, qkv, nullptr, out_hi,
                           out_lo, S, width, heads, causal);
    else
        return ec::fail(EC_ERR_INVALID, "ec_attention_f32: unknown dtype %d", dtype);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

// Which kernel ec_attention_split takes and its LDS carve: the only place these predicates live (tests/attention_ref.hl_path
// restates them).  `plain_f16`: f16 planes with a plain q -- three products per tile on the 16-bit matrix instruction:
//  HL_ONE   the four planes (and the merge area of a split last tile) fit the CU's LDS: attention_hl_kernel
//  HL_TWO   they fit in two passes over the keys, [0, split) and [split, S), of `spl` LDS rows per plane (the longer second
//           pass: whole 32-key steps, or behind an odd key its 16 copies), and a wave has at most HL2_TILES query tiles
//           (S <= 608): attention_hl2_kernel
//  HL_FP32  anything longer, a pre-scaled q, bf16 planes: attention_f32m_kernel on v_mfma_f32_16x16x4_f32
struct HlPlan {
    enum { HL_ONE, HL_TWO, HL_FP32 } kind;
    int lds, split, spl;
};
static HlPlan hl_plan(int S, bool plain_f16)
{
    if (!plain_f16) return {HlPlan::HL_FP32, 0, 0, 0};
    const int sp = 32 * ((S + 31) / 32);
    const int one = 4 * sp * 128 + (attn_lone_tile(S, 0, HL_WAVES) ? HL_WAVES * ATTN_PART * 4 : 0);
    if (one <= 160 * 1024) return {HlPlan::HL_ONE, one, 0, 0};
    const int split = (S / 2) & ~31, sl = S - split;
    const int spl = (sl & 31) == 1 ? ((sl + 15 + 15) / 16) * 16 : ((sl + 31) / 32) * 32;
    if (split >= 32 && 4 * spl * 128 <= 160 * 1024 && (S + 15) / 16 <= HL_WAVES * HL2_TILES) return {HlPlan::HL_TWO, 4 * spl * 128, split, spl};
    return {HlPlan::HL_FP32, 0, 0, 0};
}

extern "C" EC_API int ec_attention_split(const void *qkv_hi, const void *qkv_lo, void *out_hi, void *out_lo, int n_seq, int S,
                                         int width, int heads, int q_prescaled, int dtype, ec_stream_t stream)
{
    if (int rc = check_shape("ec_attention_split", n_seq, S, width, heads)) return rc;
    if (n_seq == 0) return EC_OK;
    EC_REQUIRE(qkv_hi && qkv_lo && out_hi && out_lo, "ec_attention_split: null buffer");
    EC_REQUIRE((((uintptr_t)qkv_hi | (uintptr_t)qkv_lo | (uintptr_t)out_hi | (uintptr_t)out_lo) & 15) == 0,
               "ec_attention_split: buffers must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ec::ProfScope prof(ec::PROF_ATTENTION, s, 4.0 * S * S * 64.0 * heads * n_seq, (double)n_seq * S * width * 2.0 * 8.0);
    const HlPlan plan = hl_plan(S, dtype == EC_F16 && !q_prescaled);
    if (plan.kind != HlPlan::HL_FP32) {
        AttnHlArgs h;
        h.qkv_hi = static_cast<const _Float16 *>(qkv_hi), h.qkv_lo = static_cast<const _Float16 *>(qkv_lo);
        h.out_hi = static_cast<_Float16 *>(out_hi), h.out_lo = static_cast<_Float16 *>(out_lo);
        h.S = S, h.W = width, h.heads = heads;
        const dim3 grid((unsigned)heads * (unsigned)n_seq), block(HL_WAVES * 64);
        if (plan.kind == HlPlan::HL_ONE) {
            if (int rc = ec::ensure_dynamic_lds(reinterpret_cast<const void *>(attention_hl_kernel), 160 * 1024)) return rc;
            hipLaunchKernelGGL(attention_hl_kernel, grid, block, plan.lds, s, h);
        } else {
            if (int rc = ec::ensure_dynamic_lds(reinterpret_cast<const void *>(attention_hl2_kernel), 160 * 1024)) return rc;
            hipLaunchKernelGGL(attention_hl2_kernel, grid, block, plan.lds, s, h, plan.split, plan.spl);
        }
        EC_CHECK_HIP(hipGetLastError());
        return EC_OK;
    }
    const long blocks = (long)n_seq * heads * ((S + 63) / 64);
    EC_REQUIRE(blocks < (1L << 31), "ec_attention_split: %ld workgroups", blocks);
    void (*kern)(const void *, const void *, void *, void *, int, int, int, int) = nullptr;
    if (dtype == EC_F16) kern = q_prescaled ? attention_f32m_kernel<EC_F16, true, true> : attention_f32m_kernel<EC_F16, true, false>;
    else if (dtype == EC_BF16) kern = q_prescaled ? attention_f32m_kernel<EC_BF16, true, true> : attention_f32m_kernel<EC_BF16, true, false>;
    if (kern)
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, qkv_hi, qkv_lo, out_hi, out_lo, S, width, heads, 0);
    else
        return ec::fail(EC_ERR_INVALID, "ec_attention_split: unknown dtype %d", dtype);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}
