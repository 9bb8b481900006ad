// events -> polarity-histogram frames on gfx950 (and, in the last four sections, -> time-surface and -> voxel-grid frames,
// the background-activity filter in front of all three and the fixed-duration windows that cut a stream into their ranges:
// they share parse(), the packed format, the tick and the reductions of this file).
//
// Replaces /root/reference/datasets/vis.py make_event_histogram (:6-41) +
// parse_events (:44-52) as driven by events2frames (:75-117).
//
// One 1024-thread workgroup owns one frame.  The [rows, W, 2] uint32 histogram
// of a row band lives in LDS and is filled with LDS atomics; a frame that does
// not fit is walked band by band.  The reference needs two frame-wide
// reductions before it can colour a pixel (the hot-pixel threshold from
// mean/std, vis.py:17-24, then the max of what is left, vis.py:27), so a
// multi-band frame re-bins its events for each of the three passes instead of
// spilling a histogram to HBM.  To keep that off the memory system the events of
// the frame are first reduced to 4-byte bin indices in an LDS cache (20 000
// events = 80 KB beside a 36-row band for N-Caltech): HBM sees each event once,
// the re-binning passes scan LDS, and the only HBM write is the uint8 frame.
// Frames too long for the cache (N-ImageNet's 70 000 events) re-read their
// events from L2 / Infinity Cache; frames that fit one band (N-Cars) bin once.
//
// Exactness: counts are integers.  mean/std come from exact integer sums
// (numpy's float64 pairwise summation agrees to ~1e-15 relative; bins whose
// count sits within 1e-9 of the threshold are reported in stats.ambiguous).
// The float stage is the float64 sequence numpy >= 2 executes for
// vis.py:27-39, including the fused multiply-add of the dgemm behind
// `hist @ cmap`, with FP contraction disabled everywhere else.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "common.h"
#include "eventclip_time_surface.h"
#include "eventclip_voxel_grid.h"
#include "eventclip_denoise.h"
#include "eventclip_refractory.h"
#include "eventclip_time_windows.h"

// numpy evaluates every ufunc with one rounding per operation: no FMA contraction anywhere in
// this file (the one fused multiply-add of the reference is written out explicitly).
#pragma clang fp contract(off)

namespace {

constexpr int EV_THREADS = 1024;
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int EV_BIN_BYTES = 156 * 1024;          // histogram band
constexpr int EV_LUT_N = 16;                       // colour look-up table over counts 0..15 x 0..15
constexpr int EV_REDUCE_BYTES = 8 * EV_WAVES * 4;  // block-reduction scratch (u64 per wave, up to 3 values at once)
constexpr int EV_SCRATCH_BYTES = EV_REDUCE_BYTES + EV_LUT_N * EV_LUT_N * 4;   // + the LUT

struct EvArgs {
    const void *events;      // float4 (x, y, t, p) or packed 8-byte events
    const long long *range;  // [F,2]
    int H, W;
    double thresh;
    int count_non_zero, background_mask;
    double red[3], blue[3];
    uint8_t *frames;
    int *raw;
    int *kept;
    ec_frame_stats *stats;
    int rows_per_band, bands;
    int flip_x, negate_p; // test-time-augmentation views (utils.py:18-35)
    int float32_stage;    // vis.py:27-39 in float32 (numpy 1.x value-based casting) instead of float64
    int bin_bytes;       // LDS bytes of the histogram band (scratch and the event cache follow)
    int cache_events;    // capacity of the LDS event cache, 0 = none
    int F;               // frames; a workgroup takes frames blockIdx.x, + gridDim.x, ...
    unsigned *sort_ws;   // band-sorted bin indices, sort_cap per workgroup (long frames), or null
    int sort_cap;
    unsigned band_magic; // ceil(2^32 / rows_per_band): y / rows_per_band == (y * magic) >> 32 for y < 2^16
    unsigned *b10_ws;    // events_band10_kernel: [workgroup][band][wave][b10_cap] band-local bin codes
    int b10_rows, b10_bands, b10_cap, b10_events;   // rows per band, bands, region capacity, most events per frame
    uint8_t *redo;       // per-frame flags shared with events_pack10_kernel: that kernel sets redo[f] to 1 for
                         // a frame it could not finish (0 otherwise), this one then processes ONLY those frames
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned t = __shfl_down(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// 32-bit sums / maxima over a wave without LDS traffic: four DPP steps leave every lane with its row's (16 lanes)
// value, the four rows meet on the scalar unit.  (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror)
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
    v += dpp_u32<0xB1>(v), v += dpp_u32<0x4E>(v), v += dpp_u32<0x141>(v), v += dpp_u32<0x140>(v);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
           (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ unsigned wave_max_dpp(unsigned v)
{
    auto mx = [](unsigned x, unsigned y) { return x > y ? x : y; };
    v = mx(v, dpp_u32<0xB1>(v)), v = mx(v, dpp_u32<0x4E>(v)), v = mx(v, dpp_u32<0x141>(v)), v = mx(v, dpp_u32<0x140>(v));
    return mx(mx((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
              mx((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48)));
}

// Sum over the workgroup, result in every thread.  scratch: EV_WAVES u64.
__device__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long *scratch)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum_u64(v);
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; w++) t += scratch[w];
    return t;
}

__device__ unsigned block_max_u32(unsigned v, unsigned long long *scratch)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_max_u32(v);
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; w++) t = scratch[w] > t ? (unsigned)scratch[w] : t;
    return t;
}

// parse_events (vis.py:50: astype(int32) truncates toward zero), after the optional TTA
// transforms of utils.py: x -> W - 1 - x in float32 (:22), p -> -p (:34).
__device__ __forceinline__ void parse(const float4 e, int W, int flip_x, int negate_p, int &x, int &y,
                                      int &p)
{
    const float xf = flip_x ? (float)(W - 1) - e.x : e.x;
    x = (int)xf, y = (int)e.y, p = (int)(negate_p ? -e.w : e.w);
}

// Packed 8-byte event (include/eventclip_hip.h, EC_PACKED_*): x and y are already the truncated
// integers of parse_events, the polarity code is 0 (p == 0), 1 (p > 0) or 2 (p < 0).
typedef unsigned long long packed_t;
__device__ __forceinline__ void parse(const packed_t e, int W, int flip_x, int negate_p, int &x, int &y,
                                      int &p)
{
    x = (int)(e & 0xffffu), y = (int)((e >> 16) & 0xffffu);
    if (flip_x) x = W - 1 - x;
    const int code = (int)((e >> 32) & 3u);
    p = code == 0 ? 0 : ((code == 1) != (negate_p != 0) ? 1 : -1);
}

// vis.py:10-14 restricted to rows [y0, y1): LDS atomics, one per in-band event.
template <typename EV>
__device__ __forceinline__ void bin_one(const EV e, int y0, int y1, int H, int W, int flip_x,
                                        int negate_p, unsigned *bins, unsigned &dropped)
{
    int x, y, p;
    parse(e, W, flip_x, negate_p, x, y, p);
    if (p == 0) return;  // counted in neither channel (vis.py:10,12)
    if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) {
        dropped++;
        return;
    }
    if (y >= y0 && y < y1) atomicAdd(&bins[((y - y0) * W + x) * 2 + (p < 0 ? 1 : 0)], 1u);
}

template <typename EV>
__device__ void bin_band(const EV *ev, long long n, int y0, int y1, int H, int W, int flip_x,
                         int negate_p, unsigned *bins, unsigned &dropped)
{
    const int nb = (y1 - y0) * W * 2;
    for (int i = threadIdx.x; i < nb; i += EV_THREADS) bins[i] = 0;
    __syncthreads();
    long long i = threadIdx.x;
    for (; i + 3 * EV_THREADS < n; i += 4 * EV_THREADS) {
        const EV e0 = ev[i], e1 = ev[i + EV_THREADS], e2 = ev[i + 2 * EV_THREADS],
                 e3 = ev[i + 3 * EV_THREADS];
        bin_one(e0, y0, y1, H, W, flip_x, negate_p, bins, dropped);
        bin_one(e1, y0, y1, H, W, flip_x, negate_p, bins, dropped);
        bin_one(e2, y0, y1, H, W, flip_x, negate_p, bins, dropped);
        bin_one(e3, y0, y1, H, W, flip_x, negate_p, bins, dropped);
    }
    for (; i < n; i += EV_THREADS) bin_one(ev[i], y0, y1, H, W, flip_x, negate_p, bins, dropped);
    __syncthreads();
}

// Event cache: every event of the frame is read from HBM ONCE, reduced to its bin index
// (((y * W + x) << 1) | channel, or EV_SKIP for p == 0 / outside the sensor) and kept in LDS,
// so the band / pass loops below re-scan 4 B per event from LDS instead of 16 B from L2.
constexpr unsigned EV_SKIP = 0xFFFFFFFFu;

template <typename EV>
__device__ void fill_cache(const EV *ev, long long n, int H, int W, int flip_x, int negate_p,
                           unsigned *cache, unsigned &dropped)
{
    auto encode = [&](const EV e) {
        int x, y, p;
        parse(e, W, flip_x, negate_p, x, y, p);
        if (p == 0) return EV_SKIP;
        if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) {
            dropped++;
            return EV_SKIP;
        }
        return ((unsigned)(y * W + x) << 1) | (p < 0 ? 1u : 0u);
    };
    // eight loads in flight per thread: this phase is the frame's only HBM read and nothing overlaps it
    long long i = threadIdx.x;
    for (; i + 7 * EV_THREADS < n; i += 8 * EV_THREADS) {
        EV e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) e[k] = ev[i + k * EV_THREADS];
#pragma unroll
        for (int k = 0; k < 8; k++) cache[i + k * EV_THREADS] = encode(e[k]);
    }
    for (; i < n; i += EV_THREADS) cache[i] = encode(ev[i]);
}

__device__ void bin_band_cached(const unsigned *cache, int n, int y0, int y1, int W, unsigned *bins)
{
    const int nb = (y1 - y0) * W * 2;
    const unsigned lo = (unsigned)(y0 * W * 2);
    for (int i = threadIdx.x; i < nb; i += EV_THREADS) bins[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += EV_THREADS) {
        const unsigned c = cache[i] - lo;          // EV_SKIP and other bands wrap far above nb
        if (c < (unsigned)nb) atomicAdd(&bins[c], 1u);
    }
    __syncthreads();
}

// Long frames (more events than the LDS cache holds, several bands: N-ImageNet's 70 000 events
// on 480 x 640) used to re-scan every event from L2 for each of the 3 passes x 16 bands.  Instead the
// events are bucketed ONCE by band into a global scratch slot owned by the workgroup (4-B bin
// indices; two scans of the events: count, then place), and each (pass, band) reads only its own
// contiguous bucket.  Slots inside a bucket come from 16 sub-counters per band (one per wave), so
// the LDS atomics that hand them out are spread like the binning atomics themselves.
constexpr int EV_SORT_MAX_BANDS = 64;
constexpr int EV_CC_N = 1024;      // count-of-counts histogram (sorted mode): how many bins hold the count c < 1023
constexpr int EV_SORT_BYTES = (EV_SORT_MAX_BANDS * EV_WAVES + EV_SORT_MAX_BANDS + 1 + EV_CC_N) * 4;

template <typename EV>
__device__ void sort_by_band(const EV *ev, long long n, int H, int W, int flip_x, int negate_p,
                             int bands, unsigned magic, unsigned *cnt, unsigned *start, unsigned *ws,
                             unsigned &dropped)
{
    const int wave = threadIdx.x >> 6;
    const int entries = bands * EV_WAVES;
    for (int i = threadIdx.x; i < entries; i += EV_THREADS) cnt[i] = 0;
    __syncthreads();
    // (both scans: eight loads in flight per thread -- one dependent load per iteration made each scan of a
    // 70 000-event frame 68 memory latencies long)
    unsigned out_of_sensor = 0;
    for (long long i = threadIdx.x; i < n; i += 8 * EV_THREADS) {
        EV e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const long long j = i + (long long)k * EV_THREADS;
            e[k] = ev[j < n ? j : n - 1];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int x, y, p;
            parse(e[k], W, flip_x, negate_p, x, y, p);
            const bool there = i + (long long)k * EV_THREADS < n && p != 0;
            const bool inside = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
            out_of_sensor += there && !inside;
            if (there && inside) {
                const unsigned band = (unsigned)(((unsigned long long)(unsigned)y * magic) >> 32);
                atomicAdd(&cnt[band * EV_WAVES + wave], 1u);
            }
        }
    }
    dropped += out_of_sensor;
    __syncthreads();
    // exclusive scan of the (band, wave) counts by the first wave: lane l owns a run of entries
    if (threadIdx.x < 64) {
        const int per = (entries + 63) / 64;
        const int lo = threadIdx.x * per, hi = min(entries, lo + per);
        unsigned sum = 0;
        for (int i = lo; i < hi; i++) sum += cnt[i];
        unsigned incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(incl, o, 64);
            if ((int)threadIdx.x >= o) incl += t;
        }
        unsigned run = incl - sum;
        for (int i = lo; i < hi; i++) {
            const unsigned c = cnt[i];
            cnt[i] = run;
            if ((i % EV_WAVES) == 0) start[i / EV_WAVES] = run;
            run += c;
        }
        if (threadIdx.x == 63) start[bands] = incl;
    }
    __syncthreads();
    for (long long i = threadIdx.x; i < n; i += 8 * EV_THREADS) {
        EV e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const long long j = i + (long long)k * EV_THREADS;
            e[k] = ev[j < n ? j : n - 1];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int x, y, p;
            parse(e[k], W, flip_x, negate_p, x, y, p);
            if (i + (long long)k * EV_THREADS >= n || p == 0 || (unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) continue;
            const unsigned band = (unsigned)(((unsigned long long)(unsigned)y * magic) >> 32);
            const unsigned slot = atomicAdd(&cnt[band * EV_WAVES + wave], 1u);
            ws[slot] = ((unsigned)(y * W + x) << 1) | (p < 0 ? 1u : 0u);
        }
    }
    __syncthreads();   // the stores are visible to the whole workgroup (one CU, one L1)
}

__device__ void bin_band_sorted(const unsigned *ws, unsigned begin, unsigned end, int y0, int y1, int W,
                                unsigned *bins)
{
    const int nb = (y1 - y0) * W * 2;
    const unsigned lo = (unsigned)(y0 * W * 2);
    for (int i = threadIdx.x; i < nb; i += EV_THREADS) bins[i] = 0;
    __syncthreads();
    for (unsigned i = begin + threadIdx.x; i < end; i += 4 * EV_THREADS) {      // four loads in flight
        unsigned c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned j = i + k * EV_THREADS;
            c[k] = ws[j < end ? j : end - 1];
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k * EV_THREADS < end) atomicAdd(&bins[c[k] - lo], 1u);
    }
    __syncthreads();
}

// Walks over a band's bucket of bin codes (four loads in flight), for the passes of long, sparse frames that
// touch only the bins the events name instead of zeroing and scanning the whole band: OP 0 counts the events into
// bins that are all zero, OP 1 reads every event's final count h back (the sum over EVENTS of h is the sum over
// BINS of h^2; cc[h] grows by h per bin with that count), OP 2 puts the touched bins back to zero.
template <int OP>
__device__ __forceinline__ void walk_bucket(const unsigned *ws, unsigned begin, unsigned end, unsigned lo, unsigned *bins,
                                            unsigned *cc, unsigned long long &s2)
{
    for (unsigned i = begin + threadIdx.x; i < end; i += 4 * EV_THREADS) {
        unsigned c[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned j = i + k * EV_THREADS;
            c[k] = ws[j < end ? j : end - 1];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i + k * EV_THREADS >= end) continue;
            unsigned *bin = &bins[c[k] - lo];
            if (OP == 0) {
                atomicAdd(bin, 1u);
            } else if (OP == 1) {
                const unsigned h = *bin;
                s2 += h;
                atomicAdd(&cc[h < EV_CC_N - 1 ? h : EV_CC_N - 1], 1u);
            } else {
                *bin = 0;
            }
        }
    }
}

// vis.py:27-39 for one pixel in float32: what the reference's pinned numpy 1.25 computes (value-based
// casting keeps `float32 array / int64 scalar` and everything after it in float32; sgemm's K = 2
// inner product is fmaf(q, blue, p * red), every ufunc after it rounds once).  FP contraction is off.
__device__ __forceinline__ void colour_pixel_f32(unsigned c0, unsigned c1, float fmx, const EvArgs &a,
                                                 uint8_t out[3])
{
    const float p = (float)c0 / fmx;
    const float q = (float)c1 / fmx;
    float w = 0.f;
    if (a.background_mask) {
        w = p + q;
        if (w < 0.f) w = 0.f;
        if (w > 1.f) w = 1.f;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float t = p * (float)a.red[c];
        float v = __builtin_fmaf(q, (float)a.blue[c], t);
        if (a.background_mask) {
            const float t1 = v * w;
            const float om = 1.f - w;
            const float t2 = 255.f * om;
            v = t1 + t2;
        }
        const float r = __builtin_rintf(v);
        out[c] = (r != r) ? (uint8_t)0 : (uint8_t)(int)r;
    }
}

// vis.py:27-39 for one pixel, float64, numpy's operation order.
__device__ __forceinline__ void colour_pixel(unsigned c0, unsigned c1, double dmx, const EvArgs &a,
                                             uint8_t out[3])
{
    if (a.float32_stage) return colour_pixel_f32(c0, c1, (float)dmx, a, out);
    const double p = (double)(float)c0 / dmx;  // vis.py:27 (astype(float32) then / int64 max)
    const double q = (double)(float)c1 / dmx;
    double w = 0.;
    if (a.background_mask) {                   // vis.py:35
        w = p + q;
        if (w < 0.) w = 0.;
        if (w > 1.) w = 1.;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double t = p * a.red[c];
        double v = __builtin_fma(q, a.blue[c], t);  // vis.py:31 (dgemm inner product)
        if (a.background_mask) {                     // vis.py:36-37
            const double t1 = v * w;
            const double om = 1. - w;
            const double t2 = 255. * om;
            v = t1 + t2;
        }
        const double r = __builtin_rint(v);          // vis.py:39, half to even
        out[c] = (r != r) ? (uint8_t)0 : (uint8_t)(int)r;
    }
}

// ---- hot-pixel threshold, vis.py:17-24 ----
// mean = S1/cnt; sum of squared deviations = S2 - S1^2/cnt = (cnt*S2 - S1^2)/cnt, exact in 128-bit
// integers, then numpy's own sequence: /cnt, sqrt, thresh*std + mean.
// The comparison `count > thr` (vis.py:24) in integers: for a non-negative integer h and a finite
// thr >= 0, h > thr <=> h > floor(thr); a NaN or infinite thr removes nothing.  The one count whose
// comparison could depend on numpy's summation order (|h - thr| <= 1e-9 |thr|) is rint(thr).
struct HotPixel {
    double thr;
    bool use_thr;
    unsigned thr_hi;     // counts above this are removed
    long long amb_h;     // the ambiguous count, or -1
};

__device__ __forceinline__ HotPixel hot_pixel_threshold(const EvArgs &a, unsigned long long s1,
                                                        unsigned long long s2, unsigned nnz, long long M2)
{
    HotPixel r;
    r.thr = __builtin_inf();
    r.use_thr = a.thresh > 0.;
    r.thr_hi = 0xFFFFFFFFu;
    r.amb_h = -1;
    bool spread = false;  // population not constant: numpy's summation order can matter
    if (r.use_thr) {
        const unsigned long long cnt = a.count_non_zero ? (unsigned long long)nnz : (unsigned long long)M2;
        if (cnt == 0) {
            r.thr = __builtin_nan("");  // empty population: comparisons are all false
        } else {
            const unsigned __int128 num = (unsigned __int128)cnt * s2 - (unsigned __int128)s1 * s1;
            spread = num != 0;
            const double mean = (double)s1 / (double)cnt;
            const double ss = (double)num / (double)cnt;
            const double var = ss / (double)cnt;
            const double sd = __builtin_sqrt(var);
            const double tsd = a.thresh * sd;
            r.thr = tsd + mean;
        }
    }
    if (r.use_thr && r.thr == r.thr && r.thr < 4294967295.) {
        r.thr_hi = (unsigned)__builtin_floor(r.thr);
        const double hr = __builtin_rint(r.thr);
        if (spread && __builtin_fabs(hr - r.thr) <= 1e-9 * __builtin_fabs(r.thr)) r.amb_h = (long long)hr;
    }
    return r;
}

template <typename EV>
__global__ __launch_bounds__(EV_THREADS) void events_to_frames_kernel(const EvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *bins = reinterpret_cast<unsigned *>(smem);
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem + a.bin_bytes);
    unsigned *cache = reinterpret_cast<unsigned *>(smem + a.bin_bytes + EV_SCRATCH_BYTES);
    unsigned *sort_cnt = cache;                                   // sorted mode: no event cache
    unsigned *sort_start = cache + EV_SORT_MAX_BANDS * EV_WAVES;
    unsigned *cc = sort_start + EV_SORT_MAX_BANDS + 1;            // sorted mode: EV_CC_N words
    unsigned *ws = a.sort_ws ? a.sort_ws + (size_t)blockIdx.x * a.sort_cap : nullptr;

    if (a.redo) {       // behind events_pack10_kernel: ordinarily none of this workgroup's frames is flagged -- one look, together
        int any = 0;
        for (int f = blockIdx.x + (int)threadIdx.x * (int)gridDim.x; f < a.F; f += EV_THREADS * (int)gridDim.x) any |= a.redo[f];
        // (through the dynamic LDS the kernel owns: __syncthreads_or takes static LDS on top of the CU's 160 KB)
        const unsigned long long flagged = __ballot(any != 0);        // (every lane's frames: taken outside the branch)
        if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = flagged;
        __syncthreads();
        unsigned long long all = 0;
#pragma unroll
        for (int w = 0; w < EV_WAVES; w++) all |= scratch[w];
        if (all == 0) return;
        __syncthreads();
    }
  for (int f = blockIdx.x; f < a.F; f += gridDim.x) {
    if (a.redo && !a.redo[f]) continue;   // finished by events_pack10_kernel (workgroup-uniform)
    const long long e0 = a.range[2 * f], e1 = a.range[2 * f + 1];
    const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
    const long long n = e1 - e0;
    const int H = a.H, W = a.W;
    const long long M2 = (long long)H * W * 2;
    const int rpb = a.rows_per_band, bands = a.bands;

    // frames that fit the LDS event cache read their events from HBM exactly once
    const bool cached = n <= (long long)a.cache_events;
    // longer multi-band frames are bucketed by band into this workgroup's scratch slot
    const bool sorted = !cached && ws != nullptr && bands > 1 && n <= (long long)a.sort_cap;
    unsigned long long s1 = 0, s2 = 0;
    unsigned nnz = 0, dropped = 0;
    // Long frames re-bin every band for every pass; the second pass only wants the largest count that survives
    // the hot-pixel threshold (and how many bins hold the one ambiguous count).  Both follow from how many bins
    // hold each count, which pass 1 can tally on the side (non-zero bins only: ~ one LDS atomic per event): the
    // frame then takes 2 x bands re-binnings instead of 3 x.  Counts of 1023 and more share the last slot; a
    // frame that has one runs the real pass 2.
    const bool use_cc = sorted && !a.kept;
    // ... and a long frame is sparse (70 000 events on 614 400 bins): with the bins all zero at the start of a
    // band, pass 1 counts the bucket in, reads each event's count back and puts the touched bins back to zero --
    // three walks of ~4 events per thread instead of zeroing and scanning 38 000 words; pass 3 likewise clears what
    // it binned after colouring the band.  Not with the debug outputs, and not for a frame with a count >= 1023
    // (its tallies by count cannot be divided back into bins): those take the dense passes.
    bool lean = use_cc && !a.raw;
    if (use_cc) {
        for (int i = threadIdx.x; i < EV_CC_N; i += EV_THREADS) cc[i] = 0;   // (visible after the first band's barriers)
    }
    if (lean) {
        const int nbw = rpb * W * 2;
        for (int i = threadIdx.x; i < nbw; i += EV_THREADS) bins[i] = 0;
    }
    if (cached) {
        fill_cache(ev, n, H, W, a.flip_x, a.negate_p, cache, dropped);
        __syncthreads();
    } else if (sorted) {
        sort_by_band(ev, n, H, W, a.flip_x, a.negate_p, bands, a.band_magic, sort_cnt, sort_start, ws,
                     dropped);
    }
    if (lean) {
        for (int b = 0; b < bands; b++) {
            const unsigned lo = (unsigned)(b * rpb * W * 2), begin = sort_start[b], end = sort_start[b + 1];
            walk_bucket<0>(ws, begin, end, lo, bins, cc, s2);
            __syncthreads();
            walk_bucket<1>(ws, begin, end, lo, bins, cc, s2);
            __syncthreads();
            walk_bucket<2>(ws, begin, end, lo, bins, cc, s2);
            __syncthreads();
        }
        if (cc[EV_CC_N - 1] != 0) {          // (uniform) a count of 1023 or more: start over with the dense passes
            lean = false;
            s2 = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < EV_CC_N; i += EV_THREADS) cc[i] = 0;
            __syncthreads();
        } else {
            // cc[h] holds h per bin with count h: back to bins per count, whose sum is the non-zero bins
            __syncthreads();
            for (int h = threadIdx.x; h < EV_CC_N - 1; h += EV_THREADS)
                if (h > 0) {
                    const unsigned per = cc[h] / (unsigned)h;
                    cc[h] = per;
                    nnz += per;
                }
            if (threadIdx.x == 0) s1 = sort_start[bands];      // every event that was binned
        }
    }
    // ---- pass 1: counts -> sum, sum of squares, non-zero bins ----
    for (int b = 0; b < bands && !lean; b++) {
        const int y0 = b * rpb, y1 = min(H, y0 + rpb);
        unsigned dr = 0;
        if (cached)
            bin_band_cached(cache, (int)n, y0, y1, W, bins);
        else if (sorted)
            bin_band_sorted(ws, sort_start[b], sort_start[b + 1], y0, y1, W, bins);
        else
            bin_band(ev, n, y0, y1, H, W, a.flip_x, a.negate_p, bins, dr);
        if (b == 0 && !cached && !sorted) dropped = dr;
        const int nb = (y1 - y0) * W * 2;
        for (int i = threadIdx.x; i < nb; i += EV_THREADS) {
            const unsigned h = bins[i];
            s1 += h;
            s2 += (unsigned long long)h * h;
            nnz += h > 0;
            if (use_cc && h > 0) atomicAdd(&cc[h < EV_CC_N - 1 ? h : EV_CC_N - 1], 1u);
            if (a.raw) a.raw[f * M2 + (long long)y0 * W * 2 + i] = (int)h;
        }
    }
    s1 = block_sum_u64(s1, scratch);
    s2 = block_sum_u64(s2, scratch);
    nnz = (unsigned)block_sum_u64(nnz, scratch);
    dropped = (unsigned)block_sum_u64(dropped, scratch);

    const HotPixel hp = hot_pixel_threshold(a, s1, s2, nnz, M2);
    const double thr = hp.thr;
    const bool use_thr = hp.use_thr;
    const unsigned thr_hi = hp.thr_hi;
    const long long amb_h = hp.amb_h;

    // ---- pass 2: max of the counts that survive (vis.py:24,27) ----
    unsigned mx = 0, amb = 0;
    const bool from_cc = use_cc && cc[EV_CC_N - 1] == 0;      // (workgroup-uniform: every thread reads the same word)
    if (from_cc) {
        for (int c = threadIdx.x; c < EV_CC_N - 1; c += EV_THREADS)
            if (c > 0 && cc[c] > 0 && (unsigned)c <= thr_hi) mx = (unsigned)c > mx ? (unsigned)c : mx;
        if (threadIdx.x == 0 && amb_h >= 0) {
            if (amb_h == 0) amb = (unsigned)(M2 - (long long)nnz);
            else if (amb_h < EV_CC_N - 1) amb = cc[amb_h];
        }
    }
    for (int b = 0; b < bands && !from_cc; b++) {
        const int y0 = b * rpb, y1 = min(H, y0 + rpb);
        unsigned dr = 0;
        if (bands > 1) {
            if (cached)
                bin_band_cached(cache, (int)n, y0, y1, W, bins);
            else if (sorted)
                bin_band_sorted(ws, sort_start[b], sort_start[b + 1], y0, y1, W, bins);
            else
                bin_band(ev, n, y0, y1, H, W, a.flip_x, a.negate_p, bins, dr);
        }
        const int nb = (y1 - y0) * W * 2;
        for (int i = threadIdx.x; i < nb; i += EV_THREADS) {
            unsigned h = bins[i];
            amb += (long long)h == amb_h;
            if (h > thr_hi) h = 0;
            mx = h > mx ? h : mx;
            if (bands == 1) bins[i] = h;  // single band: keep the thresholded counts for pass 3
            if (a.kept) a.kept[f * M2 + (long long)y0 * W * 2 + i] = (int)h;
        }
    }
    mx = block_max_u32(mx, scratch);
    amb = (unsigned)block_sum_u64(amb, scratch);
    const double dmx = (double)mx;

    if (a.stats && threadIdx.x == 0) {
        ec_frame_stats st;
        st.sum = s1;
        st.sumsq = s2;
        st.nnz = nnz;
        st.max_kept = mx;
        st.dropped = dropped;
        st.ambiguous = amb;
        st.thr = use_thr ? thr : __builtin_nan("");
        a.stats[f] = st;
    }

    // Event frames are mostly 0 .. few counts per pixel: the float64 colour stage is evaluated once per
    // frame for every pair of counts below 16 and looked up (same function, same bytes)
    unsigned *lut = reinterpret_cast<unsigned *>(smem + a.bin_bytes + EV_REDUCE_BYTES);
    if (threadIdx.x < EV_LUT_N * EV_LUT_N) {
        uint8_t px[4] = {0, 0, 0, 0};
        colour_pixel(threadIdx.x / EV_LUT_N, threadIdx.x % EV_LUT_N, dmx, a, px);
        lut[threadIdx.x] = (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16);
    }
    __syncthreads();
    auto colour = [&](unsigned h0, unsigned h1, uint8_t *px) {
        if (h0 > thr_hi) h0 = 0;                       // bands > 1: the counts were re-binned, threshold again
        if (h1 > thr_hi) h1 = 0;
        if (h0 < EV_LUT_N && h1 < EV_LUT_N) {
            const unsigned v = lut[h0 * EV_LUT_N + h1];
            px[0] = (uint8_t)v, px[1] = (uint8_t)(v >> 8), px[2] = (uint8_t)(v >> 16);
        } else {
            colour_pixel(h0, h1, dmx, a, px);
        }
    };

    // ---- pass 3: normalise, colour, blend, round -> uint8 (vis.py:27-39) ----
    uint8_t *out = a.frames + (long long)f * H * W * 3;
    for (int b = 0; b < bands; b++) {
        const int y0 = b * rpb, y1 = min(H, y0 + rpb);
        unsigned dr = 0;
        if (bands > 1) {
            if (cached)
                bin_band_cached(cache, (int)n, y0, y1, W, bins);
            else if (sorted && lean)
                walk_bucket<0>(ws, sort_start[b], sort_start[b + 1], (unsigned)(y0 * W * 2), bins, cc, s2);   // (bins all zero)
            else if (sorted)
                bin_band_sorted(ws, sort_start[b], sort_start[b + 1], y0, y1, W, bins);
            else
                bin_band(ev, n, y0, y1, H, W, a.flip_x, a.negate_p, bins, dr);
        }
        __syncthreads();
        const int npix = (y1 - y0) * W;
        uint8_t *o = out + (long long)y0 * W * 3;
        if ((W & 3) == 0) {
            // 4 pixels = 12 bytes = three dwords per thread, 4-byte aligned
            for (int g = threadIdx.x; g < npix / 4; g += EV_THREADS) {
                unsigned words[3];
                uint8_t *bytes = reinterpret_cast<uint8_t *>(words);
                const uint4 ca = *reinterpret_cast<const uint4 *>(&bins[g * 8]);
                const uint4 cb = *reinterpret_cast<const uint4 *>(&bins[g * 8 + 4]);
                unsigned c[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    colour(c[2 * k], c[2 * k + 1], bytes + 3 * k);
                }
                unsigned *dst = reinterpret_cast<unsigned *>(o + (long long)g * 12);
                dst[0] = words[0];
                dst[1] = words[1];
                dst[2] = words[2];
            }
        } else {
            for (int q = threadIdx.x; q < npix; q += EV_THREADS) {
                uint8_t px[3];
                colour(bins[2 * q], bins[2 * q + 1], px);
                o[3 * q] = px[0];
                o[3 * q + 1] = px[1];
                o[3 * q + 2] = px[2];
            }
        }
        __syncthreads();
        if (lean) {                                   // leave the band's bins zero for the next one
            walk_bucket<2>(ws, sort_start[b], sort_start[b + 1], (unsigned)(y0 * W * 2), bins, cc, s2);
            __syncthreads();
        }
    }
  }   // frames of this workgroup
}

// ---------------------------------------------------------------------------------------------
// Whole frame in LDS: three 10-bit counts per 32-bit word.
//
// A sensor of up to ~59 000 pixels (N-Caltech: 180 x 240 x 2 bins -> 113 KiB) holds its complete
// histogram on chip in this form: the events are read from HBM ONCE and binned ONCE with LDS atomics
// (no event cache, no bands).  The atomics RETURN the word as it was, and the statistics the reference
// takes from the finished histogram (sum, sum of squares, non-zero bins, max) are tallied from those
// previous counts event by event, so no pass walks the histogram for them; a pass for the max of what
// survives the hot-pixel threshold runs only in frames that lose a pixel to it, and the colour pass
// reads 12 pixels = 8 words at a time through a 256-entry table of the float stage.
// An event that finds its 10-bit field at 1023 overflows it (a pixel with more than 1023 events of one
// polarity): such a frame writes no pixels and sets redo[f] (every frame writes its flag, 0 or 1);
// events_to_frames_kernel, launched behind this kernel over the same frames, processes exactly those
// with 32-bit bins.
// Its own kernel rather than a mode of the one above so that its registers are its own (as a mode it
// pushed both paths into scratch spills).
// ---------------------------------------------------------------------------------------------
constexpr unsigned P10_MASK = 1023u;

#ifdef EC_EVENTS_DIAG
// phase stamps of the first 4096 frames of a launch (diagnostic build only; tools/events_phases.py)
__device__ unsigned long long g_ev_phase[4096 * 8];
#define EV_STAMP(k)                                                                   \
    do {                                                                              \
        if (threadIdx.x == 0 && f >= 0 && f < 4096) g_ev_phase[f * 8 + (k)] = wall_clock64(); \
    } while (0)
#else
#define EV_STAMP(k)
#endif

// the frame's statistics (four sums and a max of per-thread tallies) behind one pair of barriers
struct P10Stats {
    unsigned long long total, s2, nnz, dropped;
    unsigned max;
};
__device__ __forceinline__ P10Stats block_stats(unsigned hmax, unsigned total, unsigned s2, unsigned nnz, unsigned dropped,
                                                unsigned long long *scratch)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // per-wave sums of the 32-bit partials fit 32 bits (s2: <= 64 threads x 20 events x 2047)
    const unsigned long long p01 = (unsigned long long)wave_sum_u32(total) | ((unsigned long long)wave_sum_u32(nnz) << 32);
    const unsigned long long p2 = wave_sum_u32(s2);
    const unsigned long long p3 = (unsigned long long)wave_sum_u32(dropped) | ((unsigned long long)wave_max_dpp(hmax) << 32);
    __syncthreads();
    if (lane == 0) scratch[wave] = p01, scratch[EV_WAVES + wave] = p2, scratch[2 * EV_WAVES + wave] = p3;
    __syncthreads();
    P10Stats r = {0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < EV_WAVES; w++) {
        const unsigned long long a01 = scratch[w], a3 = scratch[2 * EV_WAVES + w];
        r.total += a01 & 0xffffffffull, r.nnz += a01 >> 32, r.s2 += scratch[EV_WAVES + w];
        r.dropped += a3 & 0xffffffffull;
        const unsigned m = (unsigned)(a3 >> 32);
        r.max = m > r.max ? m : r.max;
    }
    return r;
}

template <typename EV>
__global__ __launch_bounds__(EV_THREADS) void events_pack10_kernel(const EvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *bins = reinterpret_cast<unsigned *>(smem);
    uint4 *bins4 = reinterpret_cast<uint4 *>(smem);
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem + a.bin_bytes);
    unsigned *lut = reinterpret_cast<unsigned *>(smem + a.bin_bytes + EV_REDUCE_BYTES);
    const int H = a.H, W = a.W;
    const int M2 = H * W * 2;
    const int words = (M2 + 2) / 3;
    const int words4 = (words + 3) / 4;                  // (a.bin_bytes is a multiple of 16)
    constexpr int PF = 4;                                // events per thread per round; two rounds in flight
    constexpr int ROUND = PF * EV_THREADS;
    constexpr unsigned EV_NOT_BINNED = 0xFFFFFFFFu, EV_DROPPED = 0xFFFFFFFEu;

    // One workgroup per CU (the histogram takes the CU's LDS) walks frames blockIdx.x, + gridDim.x, ...  A frame's
    // events come in rounds of 4 096 through two register buffers: while one round is binned the next is in flight,
    // and behind a frame's last rounds the buffers are refilled with the first two rounds of the NEXT frame, which
    // land behind the statistics, the threshold and the LDS passes.  The workgroups of a launch drift apart on their
    // own, so the memory system sees reads all the time instead of in bursts.
    EV ea[PF], eb[PF];
    auto request = [&](EV (&e)[PF], const EV *ev, long long n, long long i) {   // clamped: a masked slot re-reads the last event
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const long long j = i + (long long)k * EV_THREADS;
            e[k] = ev[j < n ? j : n - 1];
        }
    };
    // (the frame ranges through the constant address space: scalar loads.  As ordinary global memory -- the kernel
    // stores to other global memory -- they were vector loads behind an s_waitcnt vmcnt(0) at the top of every
    // frame, which also waited for the previous frame's pixel stores)
    typedef const __attribute__((address_space(4))) long long *range_ptr;
    const range_ptr range = (range_ptr)(a.range);
    // events of a frame that this kernel bins: a frame of more than 2^24 events is left to the 32-bit kernel (the
    // per-wave tallies are sized for less)
    auto binnable = [](long long n) { return n > (1ll << 24) ? 0ll : n; };
    // (the walk starts one frame early with an empty frame of no output, whose only effect is the request for the
    // first real frame's rounds: one place per buffer that loads events -- with more, the compiler kept copies of the
    // buffers alive and spilled)
    long long e0 = 0, n = 0;
    bool dirty = true;                                   // the histogram is not all zero
    for (int f = (int)blockIdx.x - (int)gridDim.x; f < a.F; f += gridDim.x) {
        const bool real = f >= 0;
        EV_STAMP(0);
        const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
        const int fn = f + (int)gridDim.x;               // the frame after this one
        long long e0n = 0, nn = 0;
        if (fn < a.F) e0n = range[2 * fn], nn = range[2 * fn + 1] - e0n;
        const EV *evn = reinterpret_cast<const EV *>(a.events) + e0n;

        if (dirty) {                                     // (ordinarily the colour pass leaves it zero, below)
            for (int i = threadIdx.x; i < words4; i += EV_THREADS) bins4[i] = make_uint4(0, 0, 0, 0);
            __syncthreads();
        }
        dirty = real;
        EV_STAMP(1);
        // The statistics the reference takes from the finished histogram (vis.py:17-24: sum, sum of squares,
        // non-zero bins; vis.py:27: max) come out of the binning itself: the atomic returns the word as it was, h =
        // the field's count before this event, and over the events of a frame  sum of (2 h + 1) = sum over bins of
        // count^2, number of h == 0 = non-zero bins, max of h + 1 = largest count -- no pass over the 28 800 words.
        // An event that finds h == 1023 overflows its 10-bit field: the first overflow of a word sees the true 1023
        // (fields are only ever wrong after one), so `some event saw 1023` == `some field overflowed`.
        // (the tallies are selects on the lambda's return value, not increments inside its divergent branches)
        unsigned dropped = 0, binned = 0, s2t = 0, nnzt = 0, hmax = 0;
        auto bin_event = [&](const EV ek) -> unsigned {     // previous count of the event's bin, or one of the codes
            int x, y, p;
            parse(ek, W, a.flip_x, a.negate_p, x, y, p);
            const bool inside = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
            unsigned h = p == 0 || inside ? EV_NOT_BINNED : EV_DROPPED;
            if (p != 0 && inside) {
                const unsigned bin = (unsigned)(y * W + x) * 2u + (p < 0 ? 1u : 0u);
                const unsigned w = bin / 3u, sh = 10u * (bin - 3u * w);
                h = (atomicAdd(&bins[w], 1u << sh) >> sh) & P10_MASK;
            }
            return h;
        };
        const bool too_long = n > (1ll << 24);
        const long long nb = binnable(n), nnb = binnable(nn);
        // Every thread runs the same number of rounds, two per iteration (slots past the frame's end are masked, a
        // round past it is skipped): the frame's only HBM read.
        const int pairs = nb > 0 ? (int)((nb + 2 * ROUND - 1) / (2 * ROUND)) : 1;
        auto bin_round = [&](const EV (&e)[PF], int r) {
            const long long i = threadIdx.x + (long long)r * ROUND;
            unsigned h[PF];
#pragma unroll
            for (int k = 0; k < PF; k++) h[k] = i + (long long)k * EV_THREADS < nb ? bin_event(e[k]) : EV_NOT_BINNED;
#pragma unroll
            for (int k = 0; k < PF; k++) {
                const bool there = h[k] < EV_DROPPED;
                binned += there ? 1u : 0u;
                dropped += h[k] == EV_DROPPED ? 1u : 0u;
                s2t += there ? 2u * h[k] + 1u : 0u;
                nnzt += h[k] == 0u ? 1u : 0u;
                const unsigned now = there ? h[k] + 1u : 0u;   // 1024 = this event overflowed its field
                hmax = now > hmax ? now : hmax;
            }
        };
        // round g of this frame into a buffer, or -- past this frame's iterations -- round g - 2 pairs of the next
        auto refill = [&](EV (&e)[PF], int g) {
            const bool mine = g < 2 * pairs;
            const long long first = (long long)(mine ? g : g - 2 * pairs) * ROUND;
            const EV *src = mine ? ev : evn;
            const long long ns = mine ? nb : nnb;
            if (first < ns) request(e, src, ns, first + threadIdx.x);
        };
        for (int t = 0; t < pairs; t++) {
            bin_round(ea, 2 * t);
            refill(ea, 2 * t + 2);
            bin_round(eb, 2 * t + 1);
            refill(eb, 2 * t + 3);
        }
        EV_STAMP(2);
        if (!real) {                                     // the lead-in frame: nothing but the requests above
            e0 = e0n, n = nn;
            continue;
        }
        const P10Stats sums = block_stats(hmax, binned, s2t, nnzt, dropped, scratch);   // (its first barrier ends the binning)
        const bool overflow = too_long || sums.max > P10_MASK;   // a field overflowed: the 32-bit kernel takes the frame
        if (threadIdx.x == 0) a.redo[f] = overflow ? 1 : 0;
        const unsigned gmax = sums.max;
        const unsigned long long s1 = sums.total, s2 = sums.s2;
        const unsigned nnz = (unsigned)sums.nnz;
        dropped = (unsigned)sums.dropped;
        const HotPixel hp = hot_pixel_threshold(a, s1, s2, nnz, M2);
        const unsigned thr_hi = hp.thr_hi;
        EV_STAMP(3);

        if (!overflow) {
        // ---- pass 2: max of the counts that survive; debug outputs ----
        // Only when the answer is not known already: the largest count survives the threshold in an ordinary frame
        // (then it is the max of what is left, vis.py:27), and no count sits within 1e-9 of the threshold.
        unsigned mx = gmax, amb = 0;
        const bool amb_possible = hp.amb_h >= 0 && hp.amb_h <= (long long)gmax;
        if (a.raw || a.kept || amb_possible) {               // debug outputs, or a count within 1e-9 of the threshold
            mx = 0;
            for (int w = threadIdx.x; w < words; w += EV_THREADS) {
                const unsigned v = bins[w];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const int idx = 3 * w + k;
                    unsigned h = (v >> (10 * k)) & P10_MASK;
                    if (a.raw && idx < M2) a.raw[(long long)f * M2 + idx] = (int)h;
                    amb += (long long)h == hp.amb_h;
                    if (h > thr_hi) h = 0;
                    mx = h > mx ? h : mx;
                    if (a.kept && idx < M2) a.kept[(long long)f * M2 + idx] = (int)h;
                }
            }
            // max and the ambiguous-count tally behind one pair of barriers
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            mx = wave_max_dpp(mx);
            amb = wave_sum_u32(amb);
            __syncthreads();
            if (lane == 0) scratch[wave] = (unsigned long long)mx | ((unsigned long long)amb << 32);
            __syncthreads();
            mx = 0, amb = 0;
#pragma unroll
            for (int w = 0; w < EV_WAVES; w++) {
                const unsigned long long t = scratch[w];
                const unsigned m = (unsigned)(t & 0xffffffffull);
                mx = m > mx ? m : mx;
                amb += (unsigned)(t >> 32);
            }
        } else if (gmax > thr_hi) {
            // hot pixels were removed: the largest count that is left.  t = h - (thr_hi + 1) wraps to the top of the
            // unsigned range exactly for the survivors, in their order, so one unsigned max per field finds it
            // (thr_hi < gmax <= 1023 here)
            const unsigned off = thr_hi + 1u;
            unsigned t = 0;
            for (int i = threadIdx.x; i < words4; i += EV_THREADS) {
                const uint4 q = bins4[i];
                const unsigned v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned t0 = (v[j] & P10_MASK) - off, t1 = ((v[j] >> 10) & P10_MASK) - off,
                                   t2 = ((v[j] >> 20) & P10_MASK) - off;
                    const unsigned m01 = t0 > t1 ? t0 : t1, m2 = t2 > t ? t2 : t;
                    t = m01 > m2 ? m01 : m2;
                }
            }
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            t = wave_max_dpp(t);
            __syncthreads();
            if (lane == 0) scratch[wave] = t;
            __syncthreads();
            t = 0;
#pragma unroll
            for (int w = 0; w < EV_WAVES; w++) t = (unsigned)scratch[w] > t ? (unsigned)scratch[w] : t;
            mx = t >= 0x80000000u ? t + off : 0u;
        }
        const double dmx = (double)mx;
        if (a.stats && threadIdx.x == 0) {
            ec_frame_stats st;
            st.sum = s1;
            st.sumsq = s2;
            st.nnz = nnz;
            st.max_kept = mx;
            st.dropped = dropped;
            st.ambiguous = amb;
            st.thr = hp.use_thr ? hp.thr : __builtin_nan("");
            a.stats[f] = st;
        }

        // ---- pass 3: colour through the per-frame look-up table for small counts ----
        // lut[h0 | h1 << 4] = the pixel of the counts (h0, h1) < 16 AFTER the threshold (a count above it is 0), so
        // the look-up path does not compare against the threshold at all
        EV_STAMP(4);
        if (threadIdx.x < EV_LUT_N * EV_LUT_N) {
            uint8_t px[4] = {0, 0, 0, 0};
            const unsigned h0 = threadIdx.x % EV_LUT_N, h1 = threadIdx.x / EV_LUT_N;
            colour_pixel(h0 > thr_hi ? 0u : h0, h1 > thr_hi ? 0u : h1, dmx, a, px);
            lut[threadIdx.x] = (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16);
        }
        __syncthreads();
        EV_STAMP(5);
        uint8_t *out = a.frames + (long long)f * H * W * 3;
        const int npix = H * W;
        // one pixel the long way: counts cut out of the words wherever they lie, threshold, table or float stage,
        // three byte stores.  (One copy of the float stage in the loop: unrolled into the group loop below it took
        // the kernel past 128 registers, and a spill next to the prefetch waits for the prefetch.)
        auto pixel = [&](int q) {
            const unsigned b0 = 2u * q, wa = b0 / 3u, wb = (b0 + 1u) / 3u;
            unsigned h0 = (bins[wa] >> (10u * (b0 - 3u * wa))) & P10_MASK, h1 = (bins[wb] >> (10u * (b0 + 1u - 3u * wb))) & P10_MASK;
            unsigned v;
            if (h0 < EV_LUT_N && h1 < EV_LUT_N) {
                v = lut[h0 | (h1 << 4)];
            } else {
                if (h0 > thr_hi) h0 = 0;
                if (h1 > thr_hi) h1 = 0;
                uint8_t px[3];
                colour_pixel(h0, h1, dmx, a, px);
                v = (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16);
            }
            out[3 * q] = (uint8_t)v, out[3 * q + 1] = (uint8_t)(v >> 8), out[3 * q + 2] = (uint8_t)(v >> 16);
        };
        // 12 pixels = 24 counts = exactly 8 words (two 16-byte LDS reads, every field at a fixed place), 36 bytes =
        // nine dwords out; frames whose byte size is not a multiple of 4 take the byte path.  A group whose 24 counts
        // are all below 16 (bits 4..9 of every field clear) is twelve look-ups with the index cut straight out of
        // the words; any other group goes pixel by pixel.
        // A frame that is all groups leaves its histogram zero for the next frame: each group clears the words it read.
        const int groups = (((long long)npix * 3) & 3) == 0 ? npix / 12 : 0;
        const bool clears = groups * 12 == npix;
        dirty = !clears;
        for (int g = threadIdx.x; g < groups; g += EV_THREADS) {
            const uint4 qa = bins4[2 * g], qb = bins4[2 * g + 1];
            const unsigned w[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
            const unsigned any = (w[0] | w[1]) | (w[2] | w[3]) | (w[4] | w[5]) | (w[6] | w[7]);
            if ((any & 0x3F0FC3F0u) == 0) {
                unsigned c[12];
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const int fa = 2 * k, wa = fa / 3, pa = fa % 3;      // pixel k: fields 2 k and 2 k + 1
                    unsigned idx;
                    if (pa == 0) idx = (w[wa] & 0xFu) | ((w[wa] >> 6) & 0xF0u);
                    else if (pa == 1) idx = ((w[wa] >> 10) & 0xFu) | ((w[wa] >> 16) & 0xF0u);
                    else idx = ((w[wa] >> 20) & 0xFu) | ((w[wa + 1] & 0xFu) << 4);
                    c[k] = lut[idx];
                }
                unsigned *dst = reinterpret_cast<unsigned *>(out + (long long)g * 36);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    dst[3 * k] = c[4 * k] | (c[4 * k + 1] << 24);
                    dst[3 * k + 1] = (c[4 * k + 1] >> 8) | (c[4 * k + 2] << 16);
                    dst[3 * k + 2] = (c[4 * k + 2] >> 16) | (c[4 * k + 3] << 8);
                }
            } else {
#pragma unroll 1
                for (int k = 0; k < 12; k++) pixel(12 * g + k);
            }
            if (clears) bins4[2 * g] = make_uint4(0, 0, 0, 0), bins4[2 * g + 1] = make_uint4(0, 0, 0, 0);
        }
        for (int q = groups * 12 + threadIdx.x; q < npix; q += EV_THREADS) pixel(q);
        }   // !overflow
        EV_STAMP(6);
        __syncthreads();                                 // the passes are done with the histogram and the table
        e0 = e0n, n = nn;
    }
}

// ---------------------------------------------------------------------------------------------
// Large sensors (N-ImageNet: 480 x 640, 70 000 events per frame): row bands of 10-bit counts.
//
// The frame's histogram (614 400 counts) does not fit a CU, so the frame is walked in row bands of packed 10-bit
// counts (81 rows = 135 KiB: 6 bands, where 32-bit bins take 17) and its events are routed to their bands ONCE, in the
// scan that reads them from HBM: each wave appends the band-local bin codes (4 B) of its events to a region of its own
// per band in the caller's workspace ([band][wave][cap] per workgroup -- sized for the worst case, every event in one
// band, so there is no counting scan and no prefix sum; the lanes of a wave that meet in a band find their slots
// from one ballot per band and one LDS add by the band's first lane).  Every later walk of a band is each wave
// reading its own region back, coalesced, from L2.
// As in the whole-frame kernel the statistics come from the binning (returning atomics); the max of what survives the
// hot-pixel threshold and the tally of the one ambiguous count follow from how many events found their bin at count
// v - 1 (= bins with a final count >= v), counted per value v on the side (v <= 4 with ballots, the rare rest with an
// LDS add), so there is no pass over the bands for them.  The colour pass re-bins a band (fire-and-forget atomics),
// colours 12 pixels = 8 words at a time and leaves the band zero.  An overflowing 10-bit field, or a frame with more
// events than the regions were sized for, flags the frame for events_to_frames_kernel.
// ---------------------------------------------------------------------------------------------
constexpr int B10_MAX_BANDS = 16;
constexpr int B10_CNT_BYTES = EV_WAVES * B10_MAX_BANDS * 4;
constexpr int B10_CC_BYTES = (EV_CC_N + 4) * 4;          // events per count value 0 .. 1024
constexpr int B10_SIDE_BYTES = EV_SCRATCH_BYTES + B10_CNT_BYTES + B10_CC_BYTES;

template <typename EV>
__global__ __launch_bounds__(EV_THREADS) void events_band10_kernel(const EvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *bins = reinterpret_cast<unsigned *>(smem);
    uint4 *bins4 = reinterpret_cast<uint4 *>(smem);
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem + a.bin_bytes);
    unsigned *lut = reinterpret_cast<unsigned *>(smem + a.bin_bytes + EV_REDUCE_BYTES);
    unsigned *cnt = lut + EV_LUT_N * EV_LUT_N;           // [wave][band]: codes in the wave's region of the band
    unsigned *cc = cnt + EV_WAVES * B10_MAX_BANDS;       // [v]: events that brought their bin to the count v
    const int H = a.H, W = a.W;
    const long long M2 = (long long)H * W * 2;
    const int rpb = a.b10_rows, bands = a.b10_bands, cap = a.b10_cap;
    const int band_words4 = (int)(((long long)rpb * W * 2 + 2) / 3 + 3) / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *region = a.b10_ws + ((size_t)blockIdx.x * bands * EV_WAVES + wave) * cap;   // + band * EV_WAVES * cap
    const size_t band_stride = (size_t)EV_WAVES * cap;
    constexpr int PF = 4;
    constexpr int ROUND = PF * EV_THREADS;
    constexpr unsigned NO_BAND = 0xFFu;

    EV ea[PF], eb[PF];                                   // (the two-buffer scheme of events_pack10_kernel)
    auto request = [&](EV (&e)[PF], const EV *ev, long long n, long long i) {
#pragma unroll
        for (int k = 0; k < PF; k++) {
            const long long j = i + (long long)k * EV_THREADS;
            e[k] = ev[j < n ? j : n - 1];
        }
    };
    typedef const __attribute__((address_space(4))) long long *range_ptr;
    const range_ptr range = (range_ptr)(a.range);
    const long long most = a.b10_events < (1 << 24) ? a.b10_events : (1 << 24);
    auto routable = [&](long long n) { return n > most ? 0ll : n; };
    long long e0 = 0, n = 0;
    bool dirty = true;
    for (int f = (int)blockIdx.x - (int)gridDim.x; f < a.F; f += gridDim.x) {
        const bool real = f >= 0;
        const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
        const int fn = f + (int)gridDim.x;
        long long e0n = 0, nn = 0;
        if (fn < a.F) e0n = range[2 * fn], nn = range[2 * fn + 1] - e0n;
        const EV *evn = reinterpret_cast<const EV *>(a.events) + e0n;
        const bool too_long = n > most;
        const long long nb = routable(n), nnb = routable(nn);

        if (dirty) {
            for (int i = threadIdx.x; i < band_words4; i += EV_THREADS) bins4[i] = make_uint4(0, 0, 0, 0);
            dirty = false;
        }
        for (int i = threadIdx.x; i < EV_CC_N + 4; i += EV_THREADS) cc[i] = 0;
        if (lane < B10_MAX_BANDS) cnt[wave * B10_MAX_BANDS + lane] = 0;       // (only this wave touches them)

        // ---- the scan: the frame's only HBM read; every event to its band's region of this wave ----
        unsigned dropped = 0;
        auto place = [&](const EV ek, bool there) {
            int x, y, p;
            parse(ek, W, a.flip_x, a.negate_p, x, y, p);
            const bool inside = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
            const bool ok = there && p != 0 && inside;
            dropped += there && p != 0 && !inside ? 1u : 0u;
            const unsigned band = ok ? (unsigned)(((unsigned long long)(unsigned)y * a.band_magic) >> 32) : NO_BAND;
            unsigned long long mine = 0;                 // the lanes whose event falls in this lane's band
            for (int b = 0; b < bands; b++) {
                const unsigned long long m = __ballot(band == (unsigned)b);
                if (band == (unsigned)b) mine = m;
            }
            const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mine >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mine, 0u));
            unsigned base = 0;
            if (ok && rank == 0) base = atomicAdd(&cnt[wave * B10_MAX_BANDS + band], (unsigned)__popcll(mine));
            base = __shfl(base, ok ? __ffsll((long long)mine) - 1 : lane, 64);
            if (ok) {
                const unsigned local = (unsigned)((y - (int)band * rpb) * W + x) * 2u + (p < 0 ? 1u : 0u);
                region[band * band_stride + base + rank] = local;
            }
        };
        const int pairs = nb > 0 ? (int)((nb + 2 * ROUND - 1) / (2 * ROUND)) : 1;
        auto place_round = [&](const EV (&e)[PF], int r) {
            const long long i = threadIdx.x + (long long)r * ROUND;
#pragma unroll
            for (int k = 0; k < PF; k++) place(e[k], i + (long long)k * EV_THREADS < nb);
        };
        auto refill = [&](EV (&e)[PF], int g) {
            const bool mine = g < 2 * pairs;
            const long long first = (long long)(mine ? g : g - 2 * pairs) * ROUND;
            const EV *src = mine ? ev : evn;
            const long long ns = mine ? nb : nnb;
            if (first < ns) request(e, src, ns, first + threadIdx.x);
        };
        for (int t = 0; t < pairs; t++) {
            place_round(ea, 2 * t);
            refill(ea, 2 * t + 2);
            place_round(eb, 2 * t + 1);
            refill(eb, 2 * t + 3);
        }
        if (!real) {                                     // the lead-in frame: nothing but the requests above
            e0 = e0n, n = nn;
            __syncthreads();
            continue;
        }
        __syncthreads();                                 // codes stored, bins / cc zero

        // ---- pass 1: every band binned once for the statistics ----
        unsigned binned = 0, s2t = 0, nnzt = 0, hmax = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        for (int b = 0; b < bands; b++) {
            const unsigned count = cnt[wave * B10_MAX_BANDS + b];
            const unsigned *codes = region + b * band_stride;
            for (unsigned i0 = 0; i0 < count; i0 += 4 * 64) {          // four loads in flight; wave-uniform trips
                const unsigned i = i0 + lane;
                unsigned c[4], h[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned j = i + k * 64;
                    c[k] = codes[j < count ? j : count - 1];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const bool there = i + k * 64 < count;
                    h[k] = 0xFFFFFFFFu;
                    if (there) {
                        const unsigned w = c[k] / 3u, sh = 10u * (c[k] - 3u * w);
                        h[k] = (atomicAdd(&bins[w], 1u << sh) >> sh) & P10_MASK;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const bool there = h[k] != 0xFFFFFFFFu;
                    const unsigned now = there ? h[k] + 1u : 0u;       // 1024 = this event overflowed its field
                    binned += there ? 1u : 0u;
                    s2t += there ? 2u * h[k] + 1u : 0u;
                    nnzt += h[k] == 0u ? 1u : 0u;
                    hmax = now > hmax ? now : hmax;
                    // events per value of `now`: the common small values by ballot (a wave's lanes would all hit the
                    // same LDS word), the rest by an LDS add
                    c1 += (unsigned)__popcll(__ballot(now == 1u)), c2 += (unsigned)__popcll(__ballot(now == 2u));
                    c3 += (unsigned)__popcll(__ballot(now == 3u)), c4 += (unsigned)__popcll(__ballot(now == 4u));
                    if (now >= 5u) atomicAdd(&cc[now], 1u);
                }
            }
            __syncthreads();
            for (int i = threadIdx.x; i < band_words4; i += EV_THREADS) bins4[i] = make_uint4(0, 0, 0, 0);
            __syncthreads();
        }
        if (lane == 0) atomicAdd(&cc[1], c1), atomicAdd(&cc[2], c2), atomicAdd(&cc[3], c3), atomicAdd(&cc[4], c4);
        const P10Stats sums = block_stats(hmax, binned, s2t, nnzt, dropped, scratch);   // (its barriers publish cc)
        const bool overflow = too_long || sums.max > P10_MASK;
        if (threadIdx.x == 0) a.redo[f] = overflow ? 1 : 0;
        if (!overflow) {
            const unsigned gmax = sums.max;
            const unsigned long long s1 = sums.total, s2 = sums.s2;
            const unsigned nnz = (unsigned)sums.nnz;
            const HotPixel hp = hot_pixel_threshold(a, s1, s2, nnz, M2);
            const unsigned thr_hi = hp.thr_hi;
            // cc[v] events brought a bin to v = bins whose final count is >= v, so cc[v] - cc[v + 1] bins end at v
            unsigned mx = gmax, amb = 0;
            if (gmax > thr_hi) {
                const unsigned v = threadIdx.x;            // 1024 threads: one count value each
                unsigned cand = v >= 1u && v <= thr_hi && cc[v] > cc[v + 1] ? v : 0u;
                cand = wave_max_dpp(cand);
                __syncthreads();
                if (lane == 0) scratch[wave] = cand;
                __syncthreads();
                mx = 0;
#pragma unroll
                for (int w = 0; w < EV_WAVES; w++) mx = (unsigned)scratch[w] > mx ? (unsigned)scratch[w] : mx;
            }
            if (hp.amb_h == 0) amb = (unsigned)(M2 - (long long)nnz);
            else if (hp.amb_h > 0 && hp.amb_h <= (long long)P10_MASK) amb = cc[hp.amb_h] - cc[hp.amb_h + 1];
            const double dmx = (double)mx;
            if (a.stats && threadIdx.x == 0) {
                ec_frame_stats st;
                st.sum = s1;
                st.sumsq = s2;
                st.nnz = nnz;
                st.max_kept = mx;
                st.dropped = (unsigned)sums.dropped;
                st.ambiguous = amb;
                st.thr = hp.use_thr ? hp.thr : __builtin_nan("");
                a.stats[f] = st;
            }
            if (threadIdx.x < EV_LUT_N * EV_LUT_N) {     // the table of events_pack10_kernel: lut[h0 | h1 << 4], thresholded
                uint8_t px[4] = {0, 0, 0, 0};
                const unsigned h0 = threadIdx.x % EV_LUT_N, h1 = threadIdx.x / EV_LUT_N;
                colour_pixel(h0 > thr_hi ? 0u : h0, h1 > thr_hi ? 0u : h1, dmx, a, px);
                lut[threadIdx.x] = (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16);
            }
            // ---- pass 3: every band binned again and coloured ----
            const bool aligned = (((long long)H * W * 3) & 3) == 0;        // every frame starts on a dword
            for (int b = 0; b < bands; b++) {
                const unsigned count = cnt[wave * B10_MAX_BANDS + b];
                const unsigned *codes = region + b * band_stride;
                for (unsigned i0 = 0; i0 < count; i0 += 4 * 64) {
                    const unsigned i = i0 + lane;
                    unsigned c[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const unsigned j = i + k * 64;
                        c[k] = codes[j < count ? j : count - 1];
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (i + k * 64 < count) {
                            const unsigned w = c[k] / 3u, sh = 10u * (c[k] - 3u * w);
                            atomicAdd(&bins[w], 1u << sh);
                        }
                }
                __syncthreads();                         // (also: the table is written)
                const int y0 = b * rpb, rows = min(H - y0, rpb);
                const int npix = rows * W;
                uint8_t *out = a.frames + ((long long)f * H + y0) * W * 3;
                auto pixel = [&](int q) {                // (events_pack10_kernel's: one pixel the long way)
                    const unsigned b0 = 2u * q, wa = b0 / 3u, wb = (b0 + 1u) / 3u;
                    unsigned h0 = (bins[wa] >> (10u * (b0 - 3u * wa))) & P10_MASK, h1 = (bins[wb] >> (10u * (b0 + 1u - 3u * wb))) & P10_MASK;
                    unsigned v;
                    if (h0 < EV_LUT_N && h1 < EV_LUT_N) {
                        v = lut[h0 | (h1 << 4)];
                    } else {
                        if (h0 > thr_hi) h0 = 0;
                        if (h1 > thr_hi) h1 = 0;
                        uint8_t px[3];
                        colour_pixel(h0, h1, dmx, a, px);
                        v = (unsigned)px[0] | ((unsigned)px[1] << 8) | ((unsigned)px[2] << 16);
                    }
                    out[3 * q] = (uint8_t)v, out[3 * q + 1] = (uint8_t)(v >> 8), out[3 * q + 2] = (uint8_t)(v >> 16);
                };
                // (a band of rpb rows starts on a multiple of 36 bytes: rpb * W is a multiple of 12 by the host's plan)
                const int groups = aligned && (((long long)y0 * W * 3) & 3) == 0 ? npix / 12 : 0;
                const bool clears = groups * 12 == npix;
                for (int g = threadIdx.x; g < groups; g += EV_THREADS) {
                    const uint4 qa = bins4[2 * g], qb = bins4[2 * g + 1];
                    const unsigned w[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                    const unsigned any = (w[0] | w[1]) | (w[2] | w[3]) | (w[4] | w[5]) | (w[6] | w[7]);
                    if (any == 0) {                      // a long frame is sparse: mostly this
                        const unsigned z = lut[0];
                        unsigned *dst = reinterpret_cast<unsigned *>(out + (long long)g * 36);
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            dst[3 * k] = z | (z << 24);
                            dst[3 * k + 1] = (z >> 8) | (z << 16);
                            dst[3 * k + 2] = (z >> 16) | (z << 8);
                        }
                        continue;
                    }
                    if ((any & 0x3F0FC3F0u) == 0) {
                        unsigned c[12];
#pragma unroll
                        for (int k = 0; k < 12; k++) {
                            const int fa = 2 * k, wa = fa / 3, pa = fa % 3;
                            unsigned idx;
                            if (pa == 0) idx = (w[wa] & 0xFu) | ((w[wa] >> 6) & 0xF0u);
                            else if (pa == 1) idx = ((w[wa] >> 10) & 0xFu) | ((w[wa] >> 16) & 0xF0u);
                            else idx = ((w[wa] >> 20) & 0xFu) | ((w[wa + 1] & 0xFu) << 4);
                            c[k] = lut[idx];
                        }
                        unsigned *dst = reinterpret_cast<unsigned *>(out + (long long)g * 36);
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            dst[3 * k] = c[4 * k] | (c[4 * k + 1] << 24);
                            dst[3 * k + 1] = (c[4 * k + 1] >> 8) | (c[4 * k + 2] << 16);
                            dst[3 * k + 2] = (c[4 * k + 2] >> 16) | (c[4 * k + 3] << 8);
                        }
                    } else {
#pragma unroll 1
                        for (int k = 0; k < 12; k++) pixel(12 * g + k);
                    }
                    if (clears) bins4[2 * g] = make_uint4(0, 0, 0, 0), bins4[2 * g + 1] = make_uint4(0, 0, 0, 0);
                }
                for (int q = groups * 12 + threadIdx.x; q < npix; q += EV_THREADS) pixel(q);
                __syncthreads();
                if (!clears) {
                    for (int i = threadIdx.x; i < band_words4; i += EV_THREADS) bins4[i] = make_uint4(0, 0, 0, 0);
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        e0 = e0n, n = nn;
    }
}

// center_events, datasets/utils.py:38-57, one workgroup per sample, in place:
// t -= min t; x -= ((x_max + x_min + 1) - W) // 2; y likewise (float32 arithmetic).
// (1024 threads, four events in flight per thread per pass: one workgroup per sample has to keep a CU's share of
// the HBM bandwidth busy on its own)
__global__ __launch_bounds__(1024) void center_events_kernel(float4 *events, const long long *range,
                                                            int H, int W)
{
    __shared__ float red[5][16];
    const long long e0 = range[2 * blockIdx.x], e1 = range[2 * blockIdx.x + 1];
    float4 *ev = events + e0;
    const long long n = e1 - e0;
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, tmin = INFINITY;
    long long i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        float4 e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = ev[i + u * 1024];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            xmin = fminf(xmin, e[u].x), xmax = fmaxf(xmax, e[u].x);
            ymin = fminf(ymin, e[u].y), ymax = fmaxf(ymax, e[u].y);
            tmin = fminf(tmin, e[u].z);
        }
    }
    for (; i < n; i += 1024) {
        const float4 e = ev[i];
        xmin = fminf(xmin, e.x), xmax = fmaxf(xmax, e.x);
        ymin = fminf(ymin, e.y), ymax = fmaxf(ymax, e.y);
        tmin = fminf(tmin, e.z);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        xmin = fminf(xmin, __shfl_xor(xmin, o, 64)), xmax = fmaxf(xmax, __shfl_xor(xmax, o, 64));
        ymin = fminf(ymin, __shfl_xor(ymin, o, 64)), ymax = fmaxf(ymax, __shfl_xor(ymax, o, 64));
        tmin = fminf(tmin, __shfl_xor(tmin, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        red[0][wave] = xmin, red[1][wave] = xmax, red[2][wave] = ymin, red[3][wave] = ymax,
        red[4][wave] = tmin;
    __syncthreads();
    xmin = red[0][0], xmax = red[1][0], ymin = red[2][0], ymax = red[3][0], tmin = red[4][0];
#pragma unroll
    for (int w = 1; w < 16; w++) {
        xmin = fminf(xmin, red[0][w]), xmax = fmaxf(xmax, red[1][w]);
        ymin = fminf(ymin, red[2][w]), ymax = fmaxf(ymax, red[3][w]);
        tmin = fminf(tmin, red[4][w]);
    }
    const float xs = floorf(((xmax + xmin + 1.f) - (float)W) / 2.f);   // utils.py:53
    const float ys = floorf(((ymax + ymin + 1.f) - (float)H) / 2.f);   // utils.py:54
    i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        float4 e[4];
#pragma unroll
        for (int u = 0; u < 4; u++) e[u] = ev[i + u * 1024];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            e[u].x -= xs, e[u].y -= ys, e[u].z -= tmin;
            ev[i + u * 1024] = e[u];
        }
    }
    for (; i < n; i += 1024) {
        float4 e = ev[i];
        e.x -= xs, e.y -= ys, e.z -= tmin;
        ev[i] = e;
    }
}


// center_events on packed events: the same shift in integers (coordinates are integral, so
// utils.py:53-54's float floor-division equals the arithmetic shift of the integer sum);
// a coordinate shifted below zero wraps to >= 32768 and is dropped by the binning kernel like
// any other out-of-sensor event.  t is kept relative to the sample's first event.
__global__ __launch_bounds__(1024) void center_packed_kernel(packed_t *events, const long long *range,
                                                            int H, int W)
{
    __shared__ unsigned red[5][16];
    const long long e0 = range[2 * blockIdx.x], e1 = range[2 * blockIdx.x + 1];
    packed_t *ev = events + e0;
    const long long n = e1 - e0;
    unsigned xmin = ~0u, xmax = 0, ymin = ~0u, ymax = 0, tmin = ~0u;
    auto see = [&](packed_t e) {
        const unsigned x = (unsigned)(e & 0xffffu), y = (unsigned)((e >> 16) & 0xffffu), t = (unsigned)(e >> 34);
        xmin = min(xmin, x), xmax = max(xmax, x), ymin = min(ymin, y), ymax = max(ymax, y);
        tmin = min(tmin, t);
    };
    long long i = threadIdx.x;
    for (; i + 7 * 1024 < n; i += 8 * 1024) {
        packed_t e[8];
#pragma unroll
        for (int u = 0; u < 8; u++) e[u] = ev[i + u * 1024];
#pragma unroll
        for (int u = 0; u < 8; u++) see(e[u]);
    }
    for (; i < n; i += 1024) see(ev[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        xmin = min(xmin, (unsigned)__shfl_xor((int)xmin, o, 64));
        xmax = max(xmax, (unsigned)__shfl_xor((int)xmax, o, 64));
        ymin = min(ymin, (unsigned)__shfl_xor((int)ymin, o, 64));
        ymax = max(ymax, (unsigned)__shfl_xor((int)ymax, o, 64));
        tmin = min(tmin, (unsigned)__shfl_xor((int)tmin, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        red[0][wave] = xmin, red[1][wave] = xmax, red[2][wave] = ymin, red[3][wave] = ymax,
        red[4][wave] = tmin;
    __syncthreads();
    xmin = red[0][0], xmax = red[1][0], ymin = red[2][0], ymax = red[3][0], tmin = red[4][0];
#pragma unroll
    for (int w = 1; w < 16; w++) {
        xmin = min(xmin, red[0][w]), xmax = max(xmax, red[1][w]);
        ymin = min(ymin, red[2][w]), ymax = max(ymax, red[3][w]);
        tmin = min(tmin, red[4][w]);
    }
    const int xs = ((int)(xmax + xmin + 1) - W) >> 1;   // floor division by 2 (utils.py:53)
    const int ys = ((int)(ymax + ymin + 1) - H) >> 1;   // utils.py:54
    auto moved = [&](packed_t e) {
        const unsigned x = ((unsigned)(e & 0xffffu) - (unsigned)xs) & 0xffffu;
        const unsigned y = ((unsigned)((e >> 16) & 0xffffu) - (unsigned)ys) & 0xffffu;
        const packed_t t = (e >> 34) - tmin;
        return (packed_t)x | ((packed_t)y << 16) | (e & (3ull << 32)) | (t << 34);
    };
    i = threadIdx.x;
    for (; i + 7 * 1024 < n; i += 8 * 1024) {
        packed_t e[8];
#pragma unroll
        for (int u = 0; u < 8; u++) e[u] = ev[i + u * 1024];
#pragma unroll
        for (int u = 0; u < 8; u++) ev[i + u * 1024] = moved(e[u]);
    }
    for (; i < n; i += 1024) ev[i] = moved(ev[i]);
}

// float32 (x, y, t, p) -> packed: parse_events' truncating casts (vis.py:50), t in microseconds
// rounded to nearest and saturated to 30 bits.  Events whose coordinates are not integral or do
// not fit 16 bits cannot be represented: they are counted in *bad and packed with polarity code 0
// (binned nowhere).
__global__ __launch_bounds__(256) void pack_events_kernel(const float4 *events, long long n,
                                                          packed_t *out, unsigned *bad)
{
    unsigned nbad = 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += 256ll * gridDim.x) {
        const float4 e = events[i];
        const int x = (int)e.x, y = (int)e.y, p = (int)e.w;
        unsigned code = p == 0 ? 0u : (p > 0 ? 1u : 2u);
        const bool ok = (float)x == e.x && (float)y == e.y && x >= 0 && y >= 0 && x < 65536 && y < 65536;
        if (!ok) nbad++, code = 0;
        double tu = __builtin_rint((double)e.z * 1e6);
        tu = tu < 0. ? 0. : (tu > 1073741823. ? 1073741823. : tu);
        out[i] = (packed_t)((unsigned)x & 0xffffu) | ((packed_t)((unsigned)y & 0xffffu) << 16) |
                 ((packed_t)code << 32) | ((packed_t)(unsigned)tu << 34);
    }
    if (bad) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nbad += __shfl_down(nbad, o, 64);
        if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
    }
}

// ---------------------------------------------------------------------------------------------
// Host side.  events_plan() is the one statement of which kernels a launch runs, how each of them carves its LDS and
// how the caller's workspace is laid out: launch_events() marshals it into EvArgs and walks its chunks,
// ec_events_sort_workspace_bytes() answers with its worth_bytes.  Neither decides anything about the geometry itself.
// ---------------------------------------------------------------------------------------------

template <typename EV, void (*KERNEL)(EV *, const long long *, int, int)>
int center_events(const char *name, void *events, const int64_t *sample_range, int B, int H, int W, ec_stream_t stream)
{
    EC_REQUIRE(B >= 0 && H > 0 && W > 0, "%s: bad arguments", name);
    if (B == 0) return EC_OK;
    EC_REQUIRE(events && sample_range, "%s: null buffer", name);
    EC_REQUIRE(((uintptr_t)events & (sizeof(EV) - 1)) == 0, "%s: events must be %d-byte aligned", name, (int)sizeof(EV));
    hipLaunchKernelGGL(KERNEL, dim3(B), dim3(1024), 0, static_cast<hipStream_t>(stream), static_cast<EV *>(events),
                       reinterpret_cast<const long long *>(sample_range), H, W);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

// EC_EVENTS_NO_BAND10 / EC_EVENTS_NO_PACK10 (fall back to the 32-bit band kernel: A/B timing) are read by the diagnostic build
// only; the product library's kernel choice never depends on the process environment
#ifdef EC_EVENTS_DIAG
bool events_env_off(const char *name) { return getenv(name) != nullptr; }
#else
constexpr bool events_env_off(const char *) { return false; }
#endif

constexpr int EV_LDS_TOTAL = 160 * 1024;     // a CU's LDS; the 32-bit kernel always asks for all of it (one workgroup per CU)
constexpr long EV_FLAG_BYTES = 65536;        // per-frame redo flags of the 10-bit kernels: the most frames of one chunk

// compute units of the current device; 256 where there is none to ask (a size queried before a device exists)
inline int events_cus() { const int n = ec::cu_count(); return n > 0 ? n : 256; }
// EvArgs.band_magic for bands of `rows` rows
inline unsigned band_magic_of(int rows) { return (unsigned)((0x100000000ull + (unsigned)rows - 1) / (unsigned)rows); }

// LDS bytes of the whole-frame 10-bit histogram, and whether that path applies: the frame fits as packed
// counts next to the reduction scratch and the LUT.  (Also for sensors whose 32-bit histogram would fit:
// the packed kernel takes its statistics from the binning and keeps the next frame's events in flight,
// and two of its workgroups share a CU when the histogram is small, N-Cars: 32 KB.)
inline long pack10_bytes(int H, int W) { return (((long)H * W * 2 + 2) / 3 * 4 + 15) / 16 * 16; }
inline bool pack10_fits(int H, int W) { return pack10_bytes(H, W) + EV_SCRATCH_BYTES <= EV_LDS_TOTAL; }

// Row bands of 10-bit counts for sensors whose whole histogram does not fit (events_band10_kernel): rows per band a
// multiple of 12 / gcd(W, 12) so that every band is whole groups of 12 pixels, as many as fit the LDS next to the
// side arrays, then evened out over the bands.
struct B10Plan {
    bool ok;
    int rows, bands, cap;
    long bin_bytes;
    size_t region_bytes;     // per workgroup
};
inline B10Plan b10_plan(int H, int W, int max_frame_events)
{
    B10Plan p = {false, 0, 0, 0, 0, 0};
    if (max_frame_events <= 0 || pack10_fits(H, W)) return p;
    int gcd = W % 12, t = 12;
    while (gcd) { const int r = t % gcd; t = gcd; gcd = r; }          // t = gcd(W, 12)
    const int unit = 12 / t;
    const long budget_fields = ((long)EV_LDS_TOTAL - B10_SIDE_BYTES) / 16 * 16 / 4 * 3;
    int rows = (int)(budget_fields / ((long)W * 2)) / unit * unit;
    if (rows < unit) return p;
    const int bands = ec::ceil_div(H, rows);
    if (bands > B10_MAX_BANDS) return p;
    rows = ec::ceil_div(ec::ceil_div(H, bands), unit) * unit;
    p.rows = rows, p.bands = ec::ceil_div(H, rows);
    p.bin_bytes = (((long)rows * W * 2 + 2) / 3 * 4 + 15) / 16 * 16;
    p.cap = 64 * ec::ceil_div(max_frame_events, EV_THREADS);
    p.region_bytes = (size_t)p.bands * EV_WAVES * p.cap * 4;
    p.ok = p.bin_bytes + B10_SIDE_BYTES <= (long)EV_LDS_TOTAL;
    return p;
}

struct EvPlan {
    // the 32-bit kernel alone, or behind a 10-bit kernel (whole frame / row bands) that flags the frames it leaves to it
    enum Path { ONLY32, WHOLE10, BAND10 } path;
    // events_to_frames_kernel, EV_LDS_TOTAL bytes: [histogram band | reduction scratch | event cache or sort counters].
    // With the per-frame event count bounded (max_frame_events, known to the caller from split_event_count's N) the
    // cache takes 4 B per event and the band gets what is left.  Frames too long for that are bucketed by band in the
    // workspace (sorts: one slot of sort_cap indices per workgroup, which then walks several frames); without a
    // workspace, or for frames longer than the bound, every band pass re-reads the events from L2.
    int cache_events, bin_bytes, rows_per_band, bands;
    unsigned band_magic;
    bool sorts;
    int sort_cap;
    int grid_cap;            // its grid is min(frames of the chunk, grid_cap)
    // the 10-bit kernel in front: dynamic LDS, bytes of its histogram, most workgroups; BAND10: b10.rows / bands / cap
    int front_lds, front_bin_bytes, front_wgs;
    unsigned front_magic;    // BAND10: band_magic_of(b10.rows)
    B10Plan b10;
    // workspace: [redo flags, a byte per frame of a chunk | BAND10: b10.region_bytes per workgroup of the banded kernel].
    // The words behind the flags (ONLY32: all of it) are the sort slots of the 32-bit kernel, which runs after the regions' use
    long chunk_frames;       // frames per pair of launches
    size_t words_offset;     // flag bytes in front of the regions / slots
    size_t worth_bytes;      // all that this geometry can put to use on `cus` compute units
};

// ws_bytes: of the caller's workspace, 0 without one; counts: raw / kept counts are asked for
inline EvPlan events_plan(int H, int W, int max_frame_events, size_t ws_bytes, bool counts, int cus)
{
    EvPlan p = {};
    p.grid_cap = INT_MAX, p.chunk_frames = LONG_MAX;
    const long row_bytes = (long)W * 2 * 4;
    if (H <= 0 || W <= 0 || row_bytes > EV_BIN_BYTES) return p;      // no launch takes it
    const bool fits = pack10_fits(H, W);
    p.b10 = b10_plan(H, W, max_frame_events);                         // (ok only where the whole frame does not fit)
    if (p.b10.ok && !counts && ws_bytes >= (size_t)EV_FLAG_BYTES + p.b10.region_bytes && !events_env_off("EC_EVENTS_NO_BAND10")) {
        p.path = EvPlan::BAND10;
        p.front_bin_bytes = (int)p.b10.bin_bytes, p.front_lds = p.front_bin_bytes + B10_SIDE_BYTES;
        p.front_magic = band_magic_of(p.b10.rows);
        p.chunk_frames = EV_FLAG_BYTES, p.words_offset = (size_t)EV_FLAG_BYTES;
        const size_t wgs_fit = (ws_bytes - p.words_offset) / p.b10.region_bytes;
        p.front_wgs = wgs_fit < (size_t)cus ? (int)wgs_fit : cus;
    } else if (fits && ws_bytes >= 256 && !events_env_off("EC_EVENTS_NO_PACK10")) {
        p.path = EvPlan::WHOLE10;       // the workspace is the flag array, however long: no sort slots here
        p.front_bin_bytes = (int)pack10_bytes(H, W), p.front_lds = p.front_bin_bytes + EV_SCRATCH_BYTES;
        p.chunk_frames = (long)ws_bytes;
        // one persistent workgroup per CU for the 10-bit kernel (it writes every frame's flag), two where two fit its LDS
        // (1024 threads each: at most two fit a CU); the 32-bit kernel behind it walks the flags with one per CU
        p.front_wgs = cus * (2 * p.front_lds <= EV_LDS_TOTAL ? 2 : 1);
        p.grid_cap = cus;
    }
    int bin_budget = EV_BIN_BYTES;
    if (max_frame_events > 0) {
        const long left = (long)EV_BIN_BYTES - ((long)max_frame_events * 4 + 15) / 16 * 16;
        // worth it when the whole frame then needs at most 8 bands
        if (left >= row_bytes && ec::ceil_div(H, (int)(left / row_bytes)) <= 8) p.cache_events = max_frame_events, bin_budget = (int)left;
    }
    const int sort_budget = std::min((EV_LDS_TOTAL - EV_SCRATCH_BYTES - EV_SORT_BYTES) / 16 * 16, EV_BIN_BYTES);
    const int sort_rows = (int)(sort_budget / row_bytes);
    const bool sortable = p.cache_events == 0 && max_frame_events > 0 && sort_rows >= 1 && ec::ceil_div(H, sort_rows) > 1 &&
                          ec::ceil_div(H, sort_rows) <= EV_SORT_MAX_BANDS;
    const size_t slots = sortable && p.path != EvPlan::WHOLE10 ? (ws_bytes - p.words_offset) / ((size_t)max_frame_events * 4) : 0;
    if (slots >= 1) {
        p.sorts = true, p.sort_cap = max_frame_events, bin_budget = sort_budget;
        p.grid_cap = slots < (size_t)cus ? (int)slots : cus;
    }
    p.bands = ec::ceil_div(H, (int)(bin_budget / row_bytes));
    p.rows_per_band = ec::ceil_div(H, p.bands);
    p.bin_bytes = (int)((p.rows_per_band * row_bytes + 15) / 16 * 16);
    p.band_magic = band_magic_of(p.rows_per_band);
    p.worth_bytes = fits ? (size_t)EV_FLAG_BYTES
                  : p.b10.ok ? (size_t)EV_FLAG_BYTES + (size_t)cus * p.b10.region_bytes
                  : sortable ? (size_t)cus * (size_t)max_frame_events * 4 : 0;
    return p;
}

// What every launch_* opens with, under the entry's name: params, the count (`letter`: F frames or B samples), nothing to do
// for a count of 0, the buffers the entry cannot do without.  True: the entry returns rc at once (refused, or EC_OK for 0).
inline bool launch_is_over(const char *name, const void *prm, char letter, int count, bool buffers, int &rc)
{
    rc = prm == nullptr ? ec::fail(EC_ERR_INVALID, "%s: params is null", name)
         : count < 0    ? ec::fail(EC_ERR_INVALID, "%s: %c=%d", name, letter, count)
         : count == 0 || buffers ? EC_OK : ec::fail(EC_ERR_INVALID, "%s: null buffer", name);
    return rc != EC_OK || count == 0;
}

// algorithmic bytes of a launch: 16 B (packed: 8 B) per event in + 3*H*W out per frame.  The ranges live
// on the device; the caller states their total length in prm->total_events (0 = unknown: only the output part is reported)
template <typename EV>
inline double event_bytes(int F, int H, int W, int64_t total_events)
{
    return (double)F * H * W * 3.0 + (double)(total_events > 0 ? total_events : 0) * sizeof(EV);
}

// One launch of a band-walking kernel (1024 threads, the full LDS as its limit) on `stream`, under the profiler's class
template <typename ARGS>
int launch_form(void (*kernel)(const ARGS), long grid, int lds, ec::ProfClass cls, double bytes, ec_stream_t stream, const ARGS &a)
{
    if (int rc = ec::ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), EV_LDS_TOTAL)) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    ec::ProfScope prof(cls, hs, 0, bytes);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(EV_THREADS), lds, hs, a);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

template <typename EV>
int launch_events(const void *events, const int64_t *frame_range, int F, const ec_events_params *prm,
                  uint8_t *frames, int32_t *raw_counts, int32_t *kept_counts, ec_frame_stats *stats,
                  ec_stream_t stream)
{
    int rc;
    if (launch_is_over("ec_events_to_frames", prm, 'F', F, events && frame_range && frames, rc)) return rc;
    EC_REQUIRE(prm->H > 0 && prm->W > 0, "ec_events_to_frames: bad shape (%d,%d)", prm->H, prm->W);
    EC_REQUIRE(((uintptr_t)events & (sizeof(EV) - 1)) == 0,
               "ec_events_to_frames: events must be %d-byte aligned", (int)sizeof(EV));
    EC_REQUIRE((long)prm->W * 2 * 4 <= EV_BIN_BYTES, "ec_events_to_frames: W=%d too wide for one LDS row band", prm->W);

    const EvPlan plan = events_plan(prm->H, prm->W, prm->max_frame_events, prm->sort_workspace ? prm->sort_workspace_bytes : 0,
                                    raw_counts || kept_counts, events_cus());
    unsigned char *ws = static_cast<unsigned char *>(prm->sort_workspace);
    const bool words = plan.sorts || plan.path == EvPlan::BAND10;       // the workspace holds 32-bit words, not only flags
    EC_REQUIRE(!words || ((uintptr_t)ws & 3) == 0, "ec_events_to_frames: sort workspace alignment");

    EvArgs a = {};
    a.events = events;
    a.range = reinterpret_cast<const long long *>(frame_range);
    a.H = prm->H;
    a.W = prm->W;
    a.thresh = prm->thresh;
    a.count_non_zero = prm->count_non_zero;
    a.flip_x = prm->flip_x, a.negate_p = prm->negate_p;
    a.float32_stage = prm->float32_stage;
    a.background_mask = prm->background_mask;
    for (int c = 0; c < 3; c++) {
        a.red[c] = (double)(float)prm->red[c];    // cmap.astype(float32), vis.py:30
        a.blue[c] = (double)(float)prm->blue[c];
    }
    a.frames = frames;
    a.raw = raw_counts;
    a.kept = kept_counts;
    a.stats = stats;
    a.rows_per_band = plan.rows_per_band, a.bands = plan.bands;
    a.bin_bytes = plan.bin_bytes;
    a.cache_events = plan.cache_events;
    a.band_magic = plan.band_magic;
    a.sort_ws = plan.sorts ? reinterpret_cast<unsigned *>(ws + plan.words_offset) : nullptr;
    a.sort_cap = plan.sort_cap;
    if (plan.path != EvPlan::ONLY32) a.redo = ws;
    if (plan.path == EvPlan::BAND10) {
        a.b10_ws = reinterpret_cast<unsigned *>(ws + plan.words_offset);
        a.b10_rows = plan.b10.rows, a.b10_bands = plan.b10.bands, a.b10_cap = plan.b10.cap, a.b10_events = prm->max_frame_events;
    }

    void (*const front)(const EvArgs) = plan.path == EvPlan::WHOLE10 ? events_pack10_kernel<EV>
                                        : plan.path == EvPlan::BAND10 ? events_band10_kernel<EV> : nullptr;
    // (the full LDS as every kernel's limit: one attribute call each)
    if ((rc = ec::ensure_dynamic_lds(reinterpret_cast<const void *>(events_to_frames_kernel<EV>), EV_LDS_TOTAL))) return rc;
    if (front)
        if ((rc = ec::ensure_dynamic_lds(reinterpret_cast<const void *>(front), EV_LDS_TOTAL))) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    ec::ProfScope prof(ec::PROF_EVENTS, hs, 0, event_bytes<EV>(F, prm->H, prm->W, prm->total_events));
    // per chunk of frames: the 10-bit kernel, if any, then the 32-bit kernel for the frames it flagged (none, for ordinary
    // data: its workgroups return at once).  Without a front kernel the one chunk is all F frames
    const long M = (long)prm->H * prm->W;
    for (long f0 = 0; f0 < F; f0 += plan.chunk_frames) {
        EvArgs g = a;
        g.F = (int)std::min<long>(F - f0, plan.chunk_frames);
        g.range += 2 * f0;
        g.frames += f0 * M * 3;
        if (g.raw) g.raw += f0 * M * 2;
        if (g.kept) g.kept += f0 * M * 2;
        if (g.stats) g.stats += f0;
        if (front) {
            EvArgs p = g;
            p.bin_bytes = plan.front_bin_bytes, p.band_magic = plan.front_magic;
            hipLaunchKernelGGL(front, dim3(std::min(g.F, plan.front_wgs)), dim3(EV_THREADS), plan.front_lds, hs, p);
        }
        hipLaunchKernelGGL(events_to_frames_kernel<EV>, dim3(std::min(g.F, plan.grid_cap)), dim3(EV_THREADS), EV_LDS_TOTAL, hs, g);
        EC_CHECK_HIP(hipGetLastError());
    }
    return EC_OK;
}

// ---------------------------------------------------------------------------------------------
// Shared by the band-walking kernels of the three sections below (time surface, voxel grid, denoise) and their host sides:
// the scan of a range's events, the counted-event test, the frame's tallies, the band in LDS and its plan, the bytes out.
// (What every launch_* opens with stands in front of launch_events, its first user.)  The histogram kernels above have
// their own forms of these steps and are not touched.
// ---------------------------------------------------------------------------------------------
constexpr unsigned TS_TICK_MAX = (1u << 30) - 1;          // EC_PACKED_T's range
constexpr unsigned TS_REVERSED = 1u << 30;                // reverse_t: the word of tick t is TS_REVERSED - t, in 1 .. 2^30

// the event's tick
__device__ __forceinline__ unsigned tick_of(const float4 e)
{
    double tu = __builtin_rint((double)e.z * 1e6);        // (pack_events_kernel's rule)
    tu = tu < 0. ? 0. : (tu > (double)TS_TICK_MAX ? (double)TS_TICK_MAX : tu);
    return (unsigned)tu;
}
__device__ __forceinline__ unsigned tick_of(const packed_t e) { return (unsigned)(e >> 34); }

// the event with p == 0 unless `there`: a row that nothing counts (one select: of p, or of the packed event's upper half)
__device__ __forceinline__ float4 only_if(bool there, float4 e) { e.w = there ? e.w : 0.f; return e; }
__device__ __forceinline__ packed_t only_if(bool there, packed_t e)
{
    return (e & 0xffffffffull) | ((packed_t)(there ? (unsigned)(e >> 32) : 0u) << 32);
}

// f(event, row) for every row of [0, n): eight loads in flight per thread, row j always with thread j % EV_THREADS.  A slot
// past the end re-reads the last event and hands it on with p == 0, without a branch around f: f sees a few rows >= n, none
// of them counted.  (Measured against handing f a `there` flag instead, profiles/event_forms_refactor.jsonl: the flag was
// about 1 % slower on float rows in the large sensors' time surfaces and voxel frames, 1 % faster on packed voxel grids.)
template <typename EV, typename F>
__device__ __forceinline__ void for_events(const EV *ev, long long n, F f)
{
    for (long long i = threadIdx.x; i < n; i += 8 * EV_THREADS) {
        EV e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const long long j = i + (long long)k * EV_THREADS;
            e[k] = ev[j < n ? j : n - 1];
        }
        // (the loads stay whole and here: moved down into a branch of f as single dwords, the first one waited for all eight)
        __asm__ volatile("" ::: "memory");
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const long long j = i + (long long)k * EV_THREADS;
            f(only_if(j < n, e[k]), j);
        }
    }
}

// Is the event counted: p != 0 and inside the sensor?  x, y, p are parse()'s; an event that is not counted was dropped
// (p != 0, outside) or is none at all (p == 0).
template <typename EV>
__device__ __forceinline__ bool counted_event(const EV e, int H, int W, int flip_x, int negate_p, int &x, int &y, int &p)
{
    parse(e, W, flip_x, negate_p, x, y, p);
    return p != 0 && (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
}

// the frame's reduction: per-thread tallies in, the frame's values in every thread out
struct TsTally {
    unsigned hi, lo;         // max of tick + 1, max of TS_REVERSED - tick over the counted events; 0 = none
    unsigned dropped, counted;
};
// one event (counted_event's answer and p, its tick) into a thread's tallies
__device__ __forceinline__ void tally_event(TsTally &t, bool counted, int p, unsigned tick)
{
    t.dropped += !counted && p != 0;
    t.counted += counted;
    const unsigned hi = counted ? tick + 1u : 0u, lo = counted ? TS_REVERSED - tick : 0u;
    t.hi = hi > t.hi ? hi : t.hi, t.lo = lo > t.lo ? lo : t.lo;
}
__device__ __forceinline__ TsTally block_tally(const TsTally t, unsigned long long *scratch)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = (unsigned long long)wave_max_dpp(t.hi) | ((unsigned long long)wave_max_dpp(t.lo) << 32);
    const unsigned long long s = (unsigned long long)wave_sum_u32(t.dropped) | ((unsigned long long)wave_sum_u32(t.counted) << 32);
    __syncthreads();
    if (lane == 0) scratch[wave] = m, scratch[EV_WAVES + wave] = s;
    __syncthreads();
    TsTally r = {0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < EV_WAVES; w++) {
        const unsigned long long a = scratch[w], b = scratch[EV_WAVES + w];
        const unsigned hi = (unsigned)a, lo = (unsigned)(a >> 32);
        r.hi = hi > r.hi ? hi : r.hi, r.lo = lo > r.lo ? lo : r.lo;
        r.dropped += (unsigned)b, r.counted += (unsigned)(b >> 32);
    }
    return r;
}
// the reduced tallies -> the first and the last tick of the frame's counted events (0, 0 without any)
struct FrameSpan {
    unsigned t0, t1;
};
__device__ __forceinline__ FrameSpan frame_span(const TsTally t)
{
    return t.counted ? FrameSpan{TS_REVERSED - t.lo, t.hi - 1u} : FrameSpan{0u, 0u};
}

// the band in LDS (band_bytes: a multiple of 16) to zero, visible to the workgroup
__device__ __forceinline__ void zero_band(void *state, int band_bytes)
{
    for (int i = threadIdx.x; i < band_bytes / 16; i += EV_THREADS) reinterpret_cast<uint4 *>(state)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
}

// npix pixels of WPP state words each at src (the LDS band, or device memory) -> 3 npix bytes at o (a whole number of rows
// into a 4-byte aligned frame); pixel(q, its WPP words, its three bytes) is the one pixel.  Where the rows are whole groups
// of four pixels and src is 16-byte aligned, a thread takes four pixels: WPP 16-byte loads in, 12 bytes = three dwords out.
template <int WPP, typename F>
__device__ __forceinline__ void store_pixels(const unsigned *src, int npix, int W, uint8_t *o, F pixel)
{
    if ((W & 3) == 0 && ((uintptr_t)src & 15) == 0) {
        for (int g = threadIdx.x; g < npix / 4; g += EV_THREADS) {
            unsigned words[3], s[4 * WPP];
            uint8_t *bytes = reinterpret_cast<uint8_t *>(words);
#pragma unroll
            for (int k = 0; k < WPP; k++) {
                const uint4 c = *reinterpret_cast<const uint4 *>(&src[(g * WPP + k) * 4]);
                s[4 * k] = c.x, s[4 * k + 1] = c.y, s[4 * k + 2] = c.z, s[4 * k + 3] = c.w;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) pixel(4 * g + k, s + WPP * k, bytes + 3 * k);
            unsigned *dst = reinterpret_cast<unsigned *>(o + (long long)g * 12);
            dst[0] = words[0];
            dst[1] = words[1];
            dst[2] = words[2];
        }
    } else {
        for (int q = threadIdx.x; q < npix; q += EV_THREADS) {
            unsigned s[WPP];
            uint8_t px[3];
#pragma unroll
            for (int k = 0; k < WPP; k++) s[k] = src[WPP * q + k];
            pixel(q, s, px);
            o[3 * q] = px[0];
            o[3 * q + 1] = px[1];
            o[3 * q + 2] = px[2];
        }
    }
}

// Row bands of row_bytes per sensor row: as many rows as fit EV_BIN_BYTES, evened out over the bands, the band rounded up to
// 16 bytes, the reduction scratch behind.  bands == 0: refused (no sensor, or a row wider than a band).
struct RowBands {
    int rows_per_band, bands, band_bytes, lds;
};
inline RowBands row_bands(int H, long row_bytes)
{
    RowBands p = {};
    if (H <= 0 || row_bytes <= 0 || row_bytes > EV_BIN_BYTES) return p;
    p.bands = ec::ceil_div(H, (int)std::min<long>(H, EV_BIN_BYTES / row_bytes));
    p.rows_per_band = ec::ceil_div(H, p.bands);
    p.band_bytes = (int)((p.rows_per_band * row_bytes + 15) / 16 * 16);
    p.lds = p.band_bytes + EV_REDUCE_BYTES;
    return p;
}

// ---------------------------------------------------------------------------------------------
// events -> time-surface frames (include/eventclip_time_surface.h states the definition, steps 1 - 7).
//
// The surface of a row band lives in LDS as one 32-bit word per (pixel, polarity), filled with LDS atomic max: a counted
// event stores tick + 1 -- with reverse_t, 2^30 - tick, so that the earliest tick is the largest word -- and 0 is
// "untouched".  A maximum does not depend on the order of the events.  A sensor that does not fit is cut into row bands
// (N-Caltech: 3, N-ImageNet: 16); there is no HBM intermediate, so every band scans all events of its frame, and the only
// global writes are the frame and the two debug outputs.
// One 1024-thread workgroup owns one (frame, band) at a time and walks items blockIdx.x, + gridDim.x, ...  It needs t0 / t1
// over ALL events of the frame before it can colour a pixel, and has them for nothing: the one scan that fills its band
// also takes the frame's tallies (t0, t1, dropped, counted), one block reduction behind it; band 0 writes the stats.  Per
// (frame, band) rather than per frame with a loop over the bands: the work is the same scan per band either way, a small
// batch of a large sensor spreads over bands x frames compute units, and the kernel has no second form of its scan.
// One workgroup per compute unit: at ~100 VGPRs a second 1024-thread workgroup does not fit a CU's registers.
// Measured (profiles/time_surface.md): an item costs 22 - 39 us whatever its event count, so the multi-band sensors fall
// short of the histogram path by about their band count.  Bands of a frame kept on one XCD for its L2, and two register
// buffers of events in flight, were both measured and moved it by 7 % at most: neither bandwidth nor load latency bounds it.
// ---------------------------------------------------------------------------------------------
struct TsArgs {
    const void *events;      // float4 (x, y, t, p) or packed 8-byte events
    const long long *range;  // [F,2]
    int H, W, F;
    int exp_decay, background_mask, flip_x, negate_p, reverse_t;
    double tau_us;
    double red[3], blue[3];
    int same_as[3];          // channel k has the colours of channel same_as[k] < k (a gray map: 0, 0, 0), else k
    uint8_t *frames;
    int *last;               // optional [F,H,W,2]
    ec_surface_stats *stats; // optional [F]
    int rows_per_band, bands, band_bytes;
};

// steps 1 - 4 for the events of a frame and the rows [y0, y1): one LDS atomic per counted event of the band, and the
// frame's tallies
template <typename EV>
__device__ __forceinline__ void surface_band(const EV *ev, long long n, int y0, int y1, const TsArgs &a, unsigned *state,
                                             TsTally &t)
{
    for_events(ev, n, [&](const EV e, long long) {
        int x, y, p;
        const bool counted = counted_event(e, a.H, a.W, a.flip_x, a.negate_p, x, y, p);
        const unsigned tick = tick_of(e);
        tally_event(t, counted, p, tick);
        if (counted && y >= y0 && y < y1)
            atomicMax(&state[((y - y0) * a.W + x) * 2 + (p < 0 ? 1 : 0)], a.reverse_t ? TS_REVERSED - tick : tick + 1u);
    });
}

// steps 5 - 7 for one pixel: its two state words -> three bytes; l[] receives L (-1 = untouched)
struct TsFrame {
    unsigned t0, t1;
    double span;
};
__device__ __forceinline__ void surface_pixel(unsigned s0, unsigned s1, const TsFrame &fr, const TsArgs &a, uint8_t out[3],
                                              int l[2])
{
    double v[2];
    const unsigned s[2] = {s0, s1};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        v[c] = 0., l[c] = -1;
        if (s[c] == 0) continue;
        const unsigned L = a.reverse_t ? TS_REVERSED - s[c] : s[c] - 1u;
        const unsigned age = a.reverse_t ? L - fr.t0 : fr.t1 - L;
        l[c] = (int)L;
        if (a.exp_decay) {
            const double q = (double)age / a.tau_us;
            v[c] = exp(-q);
        } else {
            const unsigned span = fr.t1 - fr.t0;
            v[c] = span == 0 ? 1. : (double)(span - age) / fr.span;
        }
    }
    double w = 0.;
    if (a.background_mask) {
        w = v[0] + v[1];
        if (w > 1.) w = 1.;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (a.same_as[k] != k) {                             // (uniform) the same operations on the same operands
            out[k] = a.same_as[k] == 0 ? out[0] : out[1];    // (no runtime index into the registers)
            continue;
        }
        const double tp = v[0] * a.red[k];
        const double tn = v[1] * a.blue[k];
        double img = tp + tn;
        if (a.background_mask) {
            const double t1 = img * w;
            const double om = 1. - w;
            const double t2 = 255. * om;
            img = t1 + t2;
        }
        out[k] = (uint8_t)(int)__builtin_rint(img);
    }
}

template <typename EV>
__global__ __launch_bounds__(EV_THREADS) void time_surface_kernel(const TsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *state = reinterpret_cast<unsigned *>(smem);
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem + a.band_bytes);
    const int H = a.H, W = a.W, rpb = a.rows_per_band;
    const long long M = (long long)H * W;

    for (long long item = blockIdx.x; item < (long long)a.F * a.bands; item += gridDim.x) {
        const int f = (int)(item / a.bands), b = (int)(item % a.bands);
        const long long e0 = a.range[2 * f], n = a.range[2 * f + 1] - e0;
        const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
        uint8_t *out = a.frames + (long long)f * M * 3;
        const int y0 = b * rpb, y1 = min(H, y0 + rpb);
        zero_band(state, a.band_bytes);
        TsTally t = {0, 0, 0, 0};
        surface_band(ev, n, y0, y1, a, state, t);
        t = block_tally(t, scratch);                                      // (its first barrier ends the band's atomics)
        const FrameSpan sp = frame_span(t);
        const TsFrame fr = {sp.t0, sp.t1, (double)(sp.t1 - sp.t0)};
        if (a.stats && b == 0 && threadIdx.x == 0) {
            ec_surface_stats st;
            st.dropped = t.dropped, st.counted = t.counted, st.t0 = fr.t0, st.t1 = fr.t1;
            a.stats[f] = st;
        }
        int *lo = a.last ? a.last + ((long long)f * M + (long long)y0 * W) * 2 : nullptr;
        store_pixels<2>(state, (y1 - y0) * W, W, out + (long long)y0 * W * 3, [&](int q, const unsigned *s, uint8_t *px) {
            int l[2];
            surface_pixel(s[0], s[1], fr, a, px, l);
            if (lo) lo[2 * (long long)q] = l[0], lo[2 * (long long)q + 1] = l[1];
        });
        __syncthreads();                                                  // the band is read: the next item may zero it
    }
}

template <typename EV>
int launch_time_surface(const void *events, const int64_t *frame_range, int F, const ec_time_surface_params *prm,
                        uint8_t *frames, int32_t *last, ec_surface_stats *stats, ec_stream_t stream)
{
    int rc;
    if (launch_is_over("ec_events_to_time_surface", prm, 'F', F, events && frame_range && frames, rc)) return rc;
    EC_REQUIRE(prm->H > 0 && prm->W > 0, "ec_events_to_time_surface: bad shape (%d,%d)", prm->H, prm->W);
    EC_REQUIRE(((uintptr_t)events & (sizeof(EV) - 1)) == 0,
               "ec_events_to_time_surface: events must be %d-byte aligned", (int)sizeof(EV));
    EC_REQUIRE(((uintptr_t)frames & 3) == 0 && ((uintptr_t)last & 3) == 0, "ec_events_to_time_surface: frames and last must be 4-byte aligned");
    EC_REQUIRE((long)prm->W * 2 * 4 <= EV_BIN_BYTES, "ec_events_to_time_surface: W=%d too wide for one LDS row band", prm->W);
    EC_REQUIRE(prm->decay == EC_DECAY_LINEAR || prm->decay == EC_DECAY_EXP, "ec_events_to_time_surface: unknown decay %d", prm->decay);
    EC_REQUIRE(prm->decay != EC_DECAY_EXP || prm->tau_us > 0., "ec_events_to_time_surface: tau_us=%g must be positive", prm->tau_us);

    const RowBands plan = row_bands(prm->H, (long)prm->W * 2 * 4);          // 8 bytes per pixel
    TsArgs a = {};
    a.events = events;
    a.range = reinterpret_cast<const long long *>(frame_range);
    a.H = prm->H, a.W = prm->W, a.F = F;
    a.exp_decay = prm->decay == EC_DECAY_EXP;
    a.tau_us = prm->tau_us;
    a.background_mask = prm->background_mask;
    a.flip_x = prm->flip_x, a.negate_p = prm->negate_p, a.reverse_t = prm->reverse_t;
    for (int c = 0; c < 3; c++) {
        a.red[c] = (double)prm->red[c], a.blue[c] = (double)prm->blue[c];
        a.same_as[c] = c;
        for (int d = c - 1; d >= 0; d--)
            if (prm->red[d] == prm->red[c] && prm->blue[d] == prm->blue[c]) a.same_as[c] = d;
    }
    a.frames = frames, a.last = last, a.stats = stats;
    a.rows_per_band = plan.rows_per_band, a.bands = plan.bands, a.band_bytes = plan.band_bytes;

    return launch_form(time_surface_kernel<EV>, std::min<long>((long)F * plan.bands, events_cus()), plan.lds, ec::PROF_TIME_SURFACE,
                       event_bytes<EV>(F, prm->H, prm->W, prm->total_events), stream, a);
}

// ---------------------------------------------------------------------------------------------
// events -> voxel-grid frames (include/eventclip_voxel_grid.h states the definition, steps 1 - 7).
//
// G of a row band lives in LDS as one int32 per (pixel, bin), filled with integer LDS atomic adds: two per counted event,
// on neighbouring words (neighbouring banks).  Integer sums do not depend on the order of the events.
// Two values have to exist before the part that uses them: t0 / t1 before any event is binned, the frame's peak before any
// byte is written.  Both are reductions over the whole frame, so ONE 1024-thread workgroup owns a whole frame (frames
// blockIdx.x, + gridDim.x, ...) and walks its row bands itself: nothing is ever awaited from another workgroup, and the
// library needs no scratch in device memory.  Per frame:
//   pass 0   one scan of the events for t0, t1, dropped, counted (the time surface's tallies and block reduction);
//   pass 1   per band: zero the band, scan the events, bin those of the band; then read the band once for max |G| and,
//            when the caller asked for grid, store it (the band is a contiguous piece of [H, W, B]);
//   peak     one block reduction;
//   pass 2   the bytes: of a one-band sensor straight from the LDS band of pass 1; of a banded sensor from the grid the
//            workgroup itself wrote (behind a workgroup barrier: one compute unit, one L1), or, when the caller gave no
//            grid, by binning every band a second time.
// Traffic beyond the algorithmic 16 n (packed 8 n) + 3 H W bytes per frame: the events are read 1 + bands times (2 bands + 1
// without grid on a banded sensor) -- from L2 / MALL after the first -- and grid costs 4 B H W written plus, banded, as
// much read back.  N-Cars has 1 band at B = 3, N-Caltech 4, N-ImageNet 24.
// The floors of steps 3 and 6 are float64 products with the reciprocal, fixed up by one step either way against the exact
// 64-bit integer products (floor_ratio): exact, and without a 64-bit integer division per event and per byte.
// ---------------------------------------------------------------------------------------------
struct VgArgs {
    const void *events;      // float4 (x, y, t, p) or packed 8-byte events
    const long long *range;  // [F,2]
    int H, W, F, B;
    int background_mask, flip_x, negate_p, reverse_t;
    uint8_t *frames;         // optional [F,H,W,3] (B == 3)
    int *grid;               // optional [F,H,W,B]
    ec_voxel_stats *stats;   // optional [F]
    int rows_per_band, bands, band_bytes;
};

struct VgFrame {
    unsigned t0, t1, span;
    unsigned scale;          // (B - 1) * 256: u of an event at d == span
    double inv_span;
};

// floor(num / den) for num < 2^53, den > 0 and a quotient below 2^31; inv = 1. / (double)den.  The product is within
// 2^-51 relative of the quotient, far less than 1 absolute, so its truncation is the floor or a neighbour of it.
__device__ __forceinline__ unsigned floor_ratio(unsigned long long num, unsigned long long den, double inv)
{
    unsigned q = (unsigned)((double)num * inv);
    if ((unsigned long long)q * den > num) q--;
    else if ((unsigned long long)(q + 1u) * den <= num) q++;
    return q;
}

// steps 3 - 4 for the rows [y0, y1): the band zeroed, then two LDS atomic adds per counted event of the band (one when
// f == 0).  u is clamped to `scale`, which the exact floor never exceeds: b <= B - 1, and b == B - 1 only with f == 0.
template <typename EV>
__device__ __forceinline__ void voxel_band(const EV *ev, long long n, int y0, int y1, const VgArgs &a, const VgFrame &fr,
                                           int *state)
{
    zero_band(state, a.band_bytes);
    for_events(ev, n, [&](const EV e, long long) {
        int x, y, p;
        if (!(counted_event(e, a.H, a.W, a.flip_x, a.negate_p, x, y, p) && y >= y0 && y < y1)) return;
        const unsigned tick = tick_of(e);
        const unsigned d = a.reverse_t ? fr.t1 - tick : tick - fr.t0;
        unsigned u = fr.span ? floor_ratio((unsigned long long)d * fr.scale, fr.span, fr.inv_span) : 0u;
        u = u < fr.scale ? u : fr.scale;
        const int b = (int)(u >> 8), f = (int)(u & 255u), s = p > 0 ? 1 : -1;
        int *g = &state[((y - y0) * a.W + x) * a.B + b];
        atomicAdd(g, s * (256 - f));
        if (f) atomicAdd(g + 1, s * f);
    });
    __syncthreads();
}

// step 6 for one pixel
__device__ __forceinline__ void voxel_pixel(int g0, int g1, int g2, unsigned m, double inv_2m, int background_mask, uint8_t out[3])
{
    const int g[3] = {g0, g1, g2};
    const bool empty = (g0 | g1 | g2) == 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        unsigned byte = 128u;
        if (m) byte = floor_ratio(255ull * (unsigned long long)((long long)g[k] + (long long)m) + m, 2ull * m, inv_2m);
        out[k] = (uint8_t)(background_mask && empty ? 255u : byte);
    }
}

// step 6 for npix pixels of [.., 3] words at src (the LDS band or the grid in device memory) -> 3 npix bytes at o
__device__ __forceinline__ void voxel_colour(const int *src, int npix, int W, unsigned m, int background_mask, uint8_t *o)
{
    const double inv_2m = m ? 1. / (2. * (double)m) : 0.;
    store_pixels<3>(reinterpret_cast<const unsigned *>(src), npix, W, o, [&](int, const unsigned *s, uint8_t *px) {
        voxel_pixel((int)s[0], (int)s[1], (int)s[2], m, inv_2m, background_mask, px);
    });
}

template <typename EV>
__global__ __launch_bounds__(EV_THREADS) void voxel_grid_kernel(const VgArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *state = reinterpret_cast<int *>(smem);
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem + a.band_bytes);
    const int H = a.H, W = a.W, B = a.B, rpb = a.rows_per_band;
    const long long M = (long long)H * W;

    for (int f = blockIdx.x; f < a.F; f += gridDim.x) {
        const long long e0 = a.range[2 * f], n = a.range[2 * f + 1] - e0;
        const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
        // pass 0 (steps 1 - 2): the tallies behind t0, t1, dropped, counted
        TsTally t = {0, 0, 0, 0};
        for_events(ev, n, [&](const EV e, long long) {
            int x, y, p;
            const bool counted = counted_event(e, H, W, a.flip_x, a.negate_p, x, y, p);
            tally_event(t, counted, p, tick_of(e));
        });
        t = block_tally(t, scratch);
        const FrameSpan sp = frame_span(t);
        const unsigned span = sp.t1 - sp.t0;
        const VgFrame fr = {sp.t0, sp.t1, span, (unsigned)(B - 1) * 256u, span ? 1. / (double)span : 0.};
        // passes 1 and 2 over the bands, through one copy of the scan: pass 1 bins every band and takes the peak (and
        // stores grid), pass 2 writes the bytes -- from the band still in LDS (one band), from grid, or binned again
        const bool rebin = a.bands > 1 && !a.grid;
        unsigned peak = 0, m = 0;
        for (int pass = 1; pass <= (a.frames ? 2 : 1); pass++) {
            for (int b = 0; b < a.bands; b++) {
                const int y0 = b * rpb, y1 = min(H, y0 + rpb);
                const int nwords = (y1 - y0) * W * B;
                int *g = a.grid ? a.grid + ((long long)f * M + (long long)y0 * W) * B : nullptr;
                if (pass == 1 || rebin) voxel_band(ev, n, y0, y1, a, fr, state);
                if (pass == 1) {
                    for (int i = threadIdx.x; i < nwords; i += EV_THREADS) {
                        const int v = state[i];
                        const unsigned mag = (unsigned)(v < 0 ? -v : v);
                        peak = mag > peak ? mag : peak;
                        if (g) g[i] = v;
                    }
                } else {
                    voxel_colour(a.bands > 1 && g ? g : state, (y1 - y0) * W, W, m, a.background_mask,
                                 a.frames + ((long long)f * M + (long long)y0 * W) * 3);
                }
                if (a.bands > 1) __syncthreads();                          // the band is read: the next one may zero it
            }
            // (grid is read back by the workgroup that stored it, behind the barriers above and of the reduction: waves of
            // one workgroup share their compute unit's L1, so workgroup scope is all the ordering this needs.  Fences at
            // agent scope here were measured: they write back the whole L2 and took the N-Caltech launch from 1.1 to 4.4 ms.)
            if (pass == 1) m = block_max_u32(peak, scratch);
        }
        if (a.stats && threadIdx.x == 0) {
            ec_voxel_stats st;
            st.dropped = t.dropped, st.counted = t.counted, st.t0 = fr.t0, st.t1 = fr.t1, st.peak = m;
            a.stats[f] = st;
        }
        __syncthreads();                                                   // the band is read: the next frame may zero it
    }
}

// Row bands of 4 B bytes per pixel.  bands == 0: the entry points refuse this sensor or bin count.
inline RowBands voxel_grid_plan(int H, int W, int B)
{
    if (W <= 0 || B < EC_VOXEL_MIN_BINS || B > EC_VOXEL_MAX_BINS) return RowBands{};
    return row_bands(H, (long)W * B * 4);
}

template <typename EV>
int launch_voxel_grid(const void *events, const int64_t *frame_range, int F, const ec_voxel_grid_params *prm,
                      uint8_t *frames, int32_t *grid, ec_voxel_stats *stats, ec_stream_t stream)
{
    int rc;
    if (launch_is_over("ec_events_to_voxel_grid", prm, 'F', F, events && frame_range, rc)) return rc;
    EC_REQUIRE(frames || grid, "ec_events_to_voxel_grid: neither frames nor grid");
    EC_REQUIRE(prm->H > 0 && prm->W > 0, "ec_events_to_voxel_grid: bad shape (%d,%d)", prm->H, prm->W);
    EC_REQUIRE(prm->bins >= EC_VOXEL_MIN_BINS && prm->bins <= EC_VOXEL_MAX_BINS, "ec_events_to_voxel_grid: bins=%d outside %d .. %d",
               prm->bins, (int)EC_VOXEL_MIN_BINS, (int)EC_VOXEL_MAX_BINS);
    EC_REQUIRE(!frames || prm->bins == 3, "ec_events_to_voxel_grid: frames need bins == 3, not %d", prm->bins);
    EC_REQUIRE(prm->max_frame_events <= EC_VOXEL_MAX_FRAME_EVENTS, "ec_events_to_voxel_grid: max_frame_events=%d above %d",
               prm->max_frame_events, (int)EC_VOXEL_MAX_FRAME_EVENTS);
    EC_REQUIRE(((uintptr_t)events & (sizeof(EV) - 1)) == 0,
               "ec_events_to_voxel_grid: events must be %d-byte aligned", (int)sizeof(EV));
    EC_REQUIRE(((uintptr_t)frames & 3) == 0 && ((uintptr_t)grid & 3) == 0 && ((uintptr_t)stats & 3) == 0,
               "ec_events_to_voxel_grid: frames, grid and stats must be 4-byte aligned");
    const RowBands plan = voxel_grid_plan(prm->H, prm->W, prm->bins);
    EC_REQUIRE(plan.bands > 0, "ec_events_to_voxel_grid: W=%d too wide for one LDS row band at bins=%d", prm->W, prm->bins);

    VgArgs a = {};
    a.events = events;
    a.range = reinterpret_cast<const long long *>(frame_range);
    a.H = prm->H, a.W = prm->W, a.F = F, a.B = prm->bins;
    a.background_mask = prm->background_mask;
    a.flip_x = prm->flip_x, a.negate_p = prm->negate_p, a.reverse_t = prm->reverse_t;
    a.frames = frames, a.grid = grid, a.stats = stats;
    a.rows_per_band = plan.rows_per_band, a.bands = plan.bands, a.band_bytes = plan.band_bytes;

    return launch_form(voxel_grid_kernel<EV>, std::min<long>(F, events_cus()), plan.lds, ec::PROF_VOXEL_GRID,
                       event_bytes<EV>(F, prm->H, prm->W, prm->total_events), stream, a);
}

// ---------------------------------------------------------------------------------------------
// background-activity denoising (include/eventclip_denoise.h states the definition, steps 1 - 5).
//
// supported(i) asks every neighbour pixel "did you fire in [tick_i - dt, tick_i]?".  A per-pixel latest-timestamp map
// answers that only for events taken in time order -- sequential, and wrong on unsorted rows.  Here the ticks are SORTED BY
// PIXEL instead (a counting sort), and an event scans its neighbours' lists: exact, and independent of the row order.
// One 1024-thread workgroup owns a whole sample (samples blockIdx.x, + gridDim.x, ...) and walks its row bands itself;
// a band is rows [y0, y1) extended by a halo of r rows on either side, so that every neighbour of a band's event is in
// the band's lists.  Per band:
//   count    one LDS word per pixel of the extended band, LDS atomic adds over the counted events;
//   scan     a block-wide exclusive scan turns the counts into list offsets (word q + 1 holds the start of pixel q);
//   scatter  every counted event of the extended band takes a place with an LDS atomic add on its pixel's word -- a cursor,
//            which ends as the END of the list, i.e. the start of the next pixel's: word q is then the start of pixel q and
//            word q + 1 its end, with no second array -- and stores its tick there, in the workgroup's own slot of the
//            workspace: plain stores, read back by the same workgroup behind a barrier (one compute unit, one L1: the
//            scoping voxel_grid_kernel uses for its own grid);
//   query    every counted event of the band proper scans, per neighbour row, the ticks of pixels x - r .. x + r, which
//            are ONE contiguous run of the sorted array (two runs in its own row, around its own pixel), leaves at the
//            first supporter and writes its keep byte into the workspace.
// Then one in-order pass compacts the survivors: a ballot gives the place inside the wave, the waves' counts go through
// LDS (augment_events_kernel's scheme); each thread reads the keep bytes it wrote itself.
// No global atomics, no waiting on another workgroup; every loop is bounded by the range or by a count read from LDS, and
// the list offsets never exceed the sample's length, which the kernel checks against the slot's capacity first.
// Traffic: the events are read 3 bands + 1 times (L2 / MALL after the first), the ticks written and read once per band.
// ---------------------------------------------------------------------------------------------
constexpr int DN_PIX_WORDS = 32 * 1024;                // LDS words of the offsets: the pixels of an extended band + 1
constexpr int DN_LDS_BYTES = DN_PIX_WORDS * 4 + EV_REDUCE_BYTES;

struct DnArgs {
    const void *events;      // float4 (x, y, t, p) or packed 8-byte events
    const long long *range;  // [B,2]
    int H, W, B, r;
    unsigned dt;
    void *out;               // the survivors, same type as events
    long long *counts;       // [B]
    uint8_t *keep;           // optional [n_events_total]
    ec_denoise_stats *stats; // optional [B]
    unsigned char *ws;       // slot g of workgroup g: cap ticks (u32), then cap keep bytes
    long long slot_bytes;
    int cap;                 // max_sample_events
    int rows_per_band, bands;
};

// v[0 .. n) -> its exclusive prefix sums, in place.  Every thread owns `chunk` consecutive words (odd: neighbouring threads
// on different banks); the threads' sums meet in a wave scan and the waves' in scratch.
__device__ void block_exclusive_scan(unsigned *v, int n, unsigned long long *scratch)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = ((n + EV_THREADS - 1) / EV_THREADS) | 1;
    const int lo = min(n, (int)threadIdx.x * chunk), hi = min(n, lo + chunk);
    unsigned s = 0;
    for (int i = lo; i < hi; i++) s += v[i];
    unsigned inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        inc += lane >= o ? t : 0u;
    }
    __syncthreads();
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    unsigned run = inc - s;
#pragma unroll
    for (int w = 0; w < EV_WAVES; w++) run += w < wave ? (unsigned)scratch[w] : 0u;
    for (int i = lo; i < hi; i++) {
        const unsigned c = v[i];
        v[i] = run;
        run += c;
    }
    __syncthreads();
}

// is there a tick in [ti - dt, ti] among ticks[k0 .. k1)?  Four loads in flight (the last ones clamped to k1 - 1, a repeat
// that changes nothing): the lists are short, and one load after the other was a trip to L2 each (profiles/denoise.md).
__device__ __forceinline__ bool any_support(const unsigned *ticks, unsigned k0, unsigned k1, unsigned ti, unsigned dt)
{
    for (unsigned k = k0; k < k1; k += 4) {
        const unsigned last = k1 - 1;
        const unsigned t0 = ticks[k], t1 = ticks[min(k + 1, last)], t2 = ticks[min(k + 2, last)], t3 = ticks[min(k + 3, last)];
        const bool s0 = t0 <= ti && ti - t0 <= dt, s1 = t1 <= ti && ti - t1 <= dt;
        const bool s2 = t2 <= ti && ti - t2 <= dt, s3 = t3 <= ti && ti - t3 <= dt;
        if (s0 | s1 | s2 | s3) return true;
    }
    return false;
}

template <typename EV>
__global__ __launch_bounds__(EV_THREADS) void denoise_kernel(const DnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *offs = reinterpret_cast<unsigned *>(smem);       // word 0 stays 0; word q + 1 belongs to pixel q
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem + DN_PIX_WORDS * 4);
    int *wave_cnt = reinterpret_cast<int *>(scratch);          // [2][EV_WAVES] of the compaction
    const int H = a.H, W = a.W, r = a.r;
    const unsigned dt = a.dt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *ticks = reinterpret_cast<unsigned *>(a.ws + (long long)blockIdx.x * a.slot_bytes);
    uint8_t *flags = reinterpret_cast<uint8_t *>(ticks + a.cap);

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const long long e0 = a.range[2 * b], n = a.range[2 * b + 1] - e0;
        if (n < 0 || n > (long long)a.cap) {                   // longer than the slot: not filtered (the header says so)
            if (threadIdx.x == 0) {
                a.counts[b] = -1;
                if (a.stats) a.stats[b] = ec_denoise_stats{0, 0, 0};
            }
            continue;
        }
        const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
        for (int band = 0; band < a.bands && n > 0; band++) {
            const int y0 = band * a.rows_per_band, y1 = min(H, y0 + a.rows_per_band);
            const int ylo = max(0, y0 - r), yhi = min(H, y1 + r);
            const int npix = (yhi - ylo) * W;                  // < DN_PIX_WORDS by the plan
            for (int i = threadIdx.x; i <= npix; i += EV_THREADS) offs[i] = 0;
            __syncthreads();
            for_events(ev, n, [&](const EV e, long long) {
                int x, y, p;
                if (counted_event(e, H, W, 0, 0, x, y, p) && y >= ylo && y < yhi) atomicAdd(&offs[1 + (y - ylo) * W + x], 1u);
            });
            __syncthreads();
            block_exclusive_scan(offs + 1, npix, scratch);
            for_events(ev, n, [&](const EV e, long long) {
                int x, y, p;
                if (counted_event(e, H, W, 0, 0, x, y, p) && y >= ylo && y < yhi) {
                    const unsigned pos = atomicAdd(&offs[1 + (y - ylo) * W + x], 1u);
                    if (pos < (unsigned)a.cap) ticks[pos] = tick_of(e);    // (always: pos < the band's events <= n <= cap)
                }
            });
            __syncthreads();                                   // the ticks are stored: this workgroup may read them
            for_events(ev, n, [&](const EV e, long long j) {
                int x, y, p;
                if (!(counted_event(e, H, W, 0, 0, x, y, p) && y >= y0 && y < y1)) return;
                const unsigned ti = tick_of(e);
                const int xa = max(0, x - r), xb = min(W - 1, x + r);
                bool s = false;
                for (int yy = max(0, y - r); yy <= min(H - 1, y + r) && !s; yy++) {
                    const unsigned *row = offs + (yy - ylo) * W;       // row[q]: start of pixel q, row[q + 1]: its end
                    if (yy != y) {
                        s = any_support(ticks, row[xa], row[xb + 1], ti, dt);
                    } else {
                        s = any_support(ticks, row[xa], row[x], ti, dt) || any_support(ticks, row[x + 1], row[xb + 1], ti, dt);
                    }
                }
                flags[j] = s ? 1 : 0;
            });
            __syncthreads();                                   // the offsets are read: the next band may zero them
        }
        // step 5: the survivors in stored order.  flags[i] was written by this thread (for_events' row-to-thread rule).
        EV *dst = reinterpret_cast<EV *>(a.out) + e0;
        long long done = 0;
        unsigned kept = 0, removed = 0, passed = 0;
        int buf = 0;
        for (long long t0 = 0; t0 < n; t0 += EV_THREADS, buf ^= 1) {
            const long long i = t0 + threadIdx.x;
            bool ok = false;
            EV e = {};
            if (i < n) {
                e = ev[i];
                int x, y, p;
                const bool cnt = counted_event(e, H, W, 0, 0, x, y, p);
                ok = !cnt || flags[i] != 0;
                kept += cnt && ok, removed += cnt && !ok, passed += !cnt;
                if (a.keep) a.keep[e0 + i] = ok ? 1 : 0;
            }
            const unsigned long long mask = __ballot(ok);
            const int before = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wave_cnt[buf * EV_WAVES + wave] = __popcll(mask);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int w = 0; w < EV_WAVES; w++) {
                const int c = wave_cnt[buf * EV_WAVES + w];
                base += w < wave ? c : 0;
                total += c;
            }
            if (ok) dst[done + base + before] = e;
            done += total;
        }
        if (a.stats) {
            const unsigned long long kr = block_sum_u64((unsigned long long)kept | ((unsigned long long)removed << 32), scratch);
            const unsigned long long ps = block_sum_u64(passed, scratch);
            if (threadIdx.x == 0) a.stats[b] = ec_denoise_stats{(unsigned)kr, (unsigned)(kr >> 32), (unsigned)ps};
        }
        if (threadIdx.x == 0) a.counts[b] = done;
        __syncthreads();                                       // scratch is read: the next sample may write it
    }
}

// Row bands: as many rows as DN_PIX_WORDS - 1 pixels hold, 2 r of them halo, evened out over the bands.  A sensor that
// fits whole has one band and no halo.  bands == 0: the entry points refuse this sensor or radius.
struct DnPlan {
    int rows_per_band, bands;
};
inline DnPlan denoise_plan(int H, int W, int r)
{
    DnPlan p = {};
    if (H <= 0 || W <= 0 || W > 65536 || r < EC_DENOISE_MIN_RADIUS || r > EC_DENOISE_MAX_RADIUS) return p;
    const int rows = (DN_PIX_WORDS - 1) / W;
    if (H <= rows) {
        p.bands = 1, p.rows_per_band = H;
    } else if (rows >= 2 * r + 1) {
        p.bands = ec::ceil_div(H, rows - 2 * r);
        p.rows_per_band = ec::ceil_div(H, p.bands);
    }
    return p;
}

inline size_t denoise_slot_bytes(int cap) { return (size_t)cap * 4 + ((size_t)cap + 15) / 16 * 16; }

inline size_t denoise_workspace_bytes(const ec_denoise_params *prm, int B)
{
    if (!prm || B <= 0 || prm->max_sample_events <= 0 || denoise_plan(prm->H, prm->W, prm->radius).bands == 0) return 0;
    return denoise_slot_bytes(prm->max_sample_events) * (size_t)std::min<int>(B, EC_DENOISE_MAX_GROUPS);
}

template <typename EV>
int launch_denoise(const void *events, const int64_t *sample_range, int B, const ec_denoise_params *prm, void *events_out,
                   int64_t *counts, uint8_t *keep, ec_denoise_stats *stats, void *workspace, size_t workspace_bytes,
                   ec_stream_t stream)
{
    int rc;
    if (launch_is_over("ec_denoise_events", prm, 'B', B, events && sample_range && events_out && counts && workspace, rc)) return rc;
    EC_REQUIRE(events != events_out, "ec_denoise_events: in-place operation is not supported");
    EC_REQUIRE(prm->H > 0 && prm->W > 0, "ec_denoise_events: bad shape (%d,%d)", prm->H, prm->W);
    EC_REQUIRE(prm->radius >= EC_DENOISE_MIN_RADIUS && prm->radius <= EC_DENOISE_MAX_RADIUS,
               "ec_denoise_events: radius=%d outside %d .. %d", prm->radius, (int)EC_DENOISE_MIN_RADIUS, (int)EC_DENOISE_MAX_RADIUS);
    EC_REQUIRE(prm->dt_us <= (uint32_t)EC_DENOISE_MAX_DT_US, "ec_denoise_events: dt_us=%u above %d", prm->dt_us, (int)EC_DENOISE_MAX_DT_US);
    EC_REQUIRE(prm->max_sample_events > 0, "ec_denoise_events: max_sample_events=%d (a bound: it sizes the workspace)",
               prm->max_sample_events);
    EC_REQUIRE((((uintptr_t)events | (uintptr_t)events_out) & (sizeof(EV) - 1)) == 0,
               "ec_denoise_events: events and events_out must be %d-byte aligned", (int)sizeof(EV));
    EC_REQUIRE(((uintptr_t)counts & 7) == 0 && ((uintptr_t)stats & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
               "ec_denoise_events: counts must be 8-byte, stats 4-byte and workspace 16-byte aligned");
    const DnPlan plan = denoise_plan(prm->H, prm->W, prm->radius);
    EC_REQUIRE(plan.bands > 0, "ec_denoise_events: W=%d too wide for an LDS band of %d rows", prm->W, 2 * prm->radius + 1);
    const size_t need = denoise_workspace_bytes(prm, B);
    if (workspace_bytes < need)
        return ec::fail(EC_ERR_WORKSPACE, "ec_denoise_events: workspace %zu < %zu bytes (ec_denoise_workspace_bytes)", workspace_bytes, need);

    DnArgs a = {};
    a.events = events;
    a.range = reinterpret_cast<const long long *>(sample_range);
    a.H = prm->H, a.W = prm->W, a.B = B, a.r = prm->radius;
    a.dt = prm->dt_us;
    a.out = events_out, a.counts = reinterpret_cast<long long *>(counts), a.keep = keep, a.stats = stats;
    a.ws = static_cast<unsigned char *>(workspace);
    a.slot_bytes = (long long)denoise_slot_bytes(prm->max_sample_events);
    a.cap = prm->max_sample_events;
    a.rows_per_band = plan.rows_per_band, a.bands = plan.bands;

    // algorithmic bytes: every event read once and at most written once
    return launch_form(denoise_kernel<EV>, std::min<int>(B, EC_DENOISE_MAX_GROUPS), DN_LDS_BYTES, ec::PROF_DENOISE,
                       2.0 * event_bytes<EV>(0, 0, 0, prm->total_events), stream, a);
}

// ---------------------------------------------------------------------------------------------
// refractory-period filtering (include/eventclip_refractory.h states the definition, steps 1 - 4).
//
// Whether an event survives depends on which earlier events of its class survived: a sequential chain, but one per CLASS
// (pixel, or pixel and polarity), and the classes are independent.  A per-pixel last-kept-tick map solves the chain only
// for events taken in time order -- wrong on unsorted rows, and a race among the threads of one pixel.  Here the events are
// SORTED BY CLASS instead (denoise_kernel's counting sort, on classes rather than halo pixels), and every class's chain is
// solved by selection inside its own list: exact, and independent of the row order but for the tie rule.
// One 1024-thread workgroup owns a whole sample (samples blockIdx.x, + gridDim.x, ...) and walks its row bands itself; a
// class lies in exactly one band, so there is no halo.  Per band:
//   count    one LDS word per class of the band, LDS atomic adds over the band's counted events;
//   scan     block_exclusive_scan turns the counts into list offsets (word q + 1 holds the start of class q);
//   scatter  every counted event of the band takes a place with an LDS atomic add on its class's word (the cursor: word q
//            ends as the start of class q and word q + 1 as its end) and stores the key (tick << 32) | row-in-sample there,
//            in the workgroup's own slot of the workspace: plain stores, read back by the same workgroup behind a barrier
//            (one compute unit, one L1: the scoping denoise_kernel and voxel_grid_kernel use);
//   chain    the 64-bit key order is the (tick, row) order of step 3.  The first kept key of a list is its minimum; the
//            next kept key is the smallest one >= (last kept tick + period) << 32 (a sum below 2^31).  One pass over the
//            list finds it and, on its way, writes the keep byte 0 of every key strictly between the last kept key and
//            that bound -- the events this dead time removes -- so every counted row's byte is written exactly once, 1 when
//            it is selected or 0 in the pass behind the kept event that blinds it; kept + 1 passes in all.
//            Thread t takes the classes t, t + 1024, ...: a list of one key writes its 1 and is done, a list shorter than
//            EC_REFRACTORY_LONG_LIST is walked by its lane alone, and the longer ones of a wave's 64 classes are then
//            walked one after the other by the whole wave (lane-strided passes, a wave minimum of the candidates): a hot
//            pixel of 4096 events costs (kept + 1) x 64 loads per lane rather than (kept + 1) x 4096 in one.
// Then denoise_kernel's in-order compaction.  Here a thread reads keep bytes other threads wrote: the band loop's closing
// barrier stands between.  Rows that are not counted never read a byte.
// No global atomics, no waiting on another workgroup; every loop is bounded by the range or by a count read from LDS (the
// passes of a list by its length + 1), list ends are clamped to the slot's capacity, and a key's row is checked against the
// sample's length before its byte is written.
// Traffic: the events are read 2 bands + 1 times (L2 / MALL after the first), the keys written once and read kept + 1 times.
// ---------------------------------------------------------------------------------------------
constexpr int RF_CLASS_WORDS = 32 * 1024;              // LDS words of the offsets: the classes of a band + 1
constexpr int RF_LDS_BYTES = RF_CLASS_WORDS * 4 + EV_REDUCE_BYTES;
constexpr unsigned long long RF_NONE = ~0ull;          // no key: above every (tick << 32) | row with tick < 2^31

struct RfArgs {
    const void *events;      // float4 (x, y, t, p) or packed 8-byte events
    const long long *range;  // [B,2]
    int H, W, B, cpp;        // cpp: classes per pixel, 1 or 2 (per_polarity)
    unsigned period;
    void *out;               // the survivors, same type as events
    long long *counts;       // [B]
    uint8_t *keep;           // optional [n_events_total]
    ec_refractory_stats *stats; // optional [B]
    unsigned char *ws;       // slot g of workgroup g: cap keys (u64), then cap keep bytes
    long long slot_bytes;
    int cap;                 // max_sample_events
    int rows_per_band, bands;
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

// One pass of the chain over keys[k0 .. k1) in steps of `step`: the keys strictly between `last` and `bound` lie in the dead
// time of `last` and get their keep byte 0; -> the smallest key >= bound of this thread's share, or RF_NONE.
__device__ __forceinline__ unsigned long long chain_pass(const unsigned long long *keys, unsigned k0, unsigned k1, unsigned step,
                                                         unsigned long long last, unsigned long long bound, uint8_t *flags,
                                                         unsigned n)
{
    unsigned long long m = RF_NONE;
    for (unsigned k = k0; k < k1; k += step) {
        const unsigned long long key = keys[k];
        if (key >= bound) {
            m = key < m ? key : m;
        } else if (key > last && (unsigned)key < n) {
            flags[(unsigned)key] = 0;
        }
    }
    return m;
}

// the bound behind a kept key: (its tick + period) << 32
__device__ __forceinline__ unsigned long long chain_bound(unsigned long long kept, unsigned period)
{
    return (unsigned long long)((unsigned)(kept >> 32) + period) << 32;
}

template <typename EV>
__global__ __launch_bounds__(EV_THREADS) void refractory_kernel(const RfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *offs = reinterpret_cast<unsigned *>(smem);       // word 0 stays 0; word q + 1 belongs to class q
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem + RF_CLASS_WORDS * 4);
    int *wave_cnt = reinterpret_cast<int *>(scratch);          // [2][EV_WAVES] of the compaction
    const int H = a.H, W = a.W, cpp = a.cpp;
    const unsigned period = a.period;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(a.ws + (long long)blockIdx.x * a.slot_bytes);
    uint8_t *flags = reinterpret_cast<uint8_t *>(keys + a.cap);

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const long long e0 = a.range[2 * b], n = a.range[2 * b + 1] - e0;
        if (n < 0 || n > (long long)a.cap) {                   // longer than the slot: not filtered (the header says so)
            if (threadIdx.x == 0) {
                a.counts[b] = -1;
                if (a.stats) a.stats[b] = ec_refractory_stats{0, 0, 0};
            }
            continue;
        }
        const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
        const unsigned un = (unsigned)n;
        for (int band = 0; band < a.bands && n > 0; band++) {
            const int y0 = band * a.rows_per_band, y1 = min(H, y0 + a.rows_per_band);
            const int ncls = (y1 - y0) * W * cpp;              // < RF_CLASS_WORDS by the plan
            for (int i = threadIdx.x; i <= ncls; i += EV_THREADS) offs[i] = 0;
            __syncthreads();
            for_events(ev, n, [&](const EV e, long long) {
                int x, y, p;
                if (counted_event(e, H, W, 0, 0, x, y, p) && y >= y0 && y < y1)
                    atomicAdd(&offs[1 + ((y - y0) * W + x) * cpp + (cpp == 2 && p < 0)], 1u);
            });
            __syncthreads();
            block_exclusive_scan(offs + 1, ncls, scratch);
            for_events(ev, n, [&](const EV e, long long j) {
                int x, y, p;
                if (counted_event(e, H, W, 0, 0, x, y, p) && y >= y0 && y < y1) {
                    const unsigned pos = atomicAdd(&offs[1 + ((y - y0) * W + x) * cpp + (cpp == 2 && p < 0)], 1u);
                    if (pos < (unsigned)a.cap)                 // (always: pos < the band's events <= n <= cap)
                        keys[pos] = ((unsigned long long)tick_of(e) << 32) | (unsigned long long)(unsigned)j;
                }
            });
            __syncthreads();                                   // the keys are stored: this workgroup may read them
            for (int q0 = wave * 64; q0 < ncls; q0 += EV_THREADS) {
                const int q = q0 + lane;
                unsigned s = 0, e = 0;
                if (q < ncls) e = min(offs[q + 1], (unsigned)a.cap), s = min(offs[q], e);
                const unsigned len = e - s;
                if (len == 1) {
                    const unsigned row = (unsigned)keys[s];
                    if (row < un) flags[row] = 1;
                } else if (len > 1 && len < (unsigned)EC_REFRACTORY_LONG_LIST) {
                    unsigned long long last = 0, bound = 0;
                    for (unsigned pass = 0; pass <= len; pass++) {
                        const unsigned long long m = chain_pass(keys, s, e, 1u, last, bound, flags, un);
                        if (m == RF_NONE) break;
                        if ((unsigned)m < un) flags[(unsigned)m] = 1;
                        last = m, bound = chain_bound(m, period);
                    }
                }
                // the long lists of these 64 classes, one after the other, by the whole wave
                unsigned long long todo = __ballot(len >= (unsigned)EC_REFRACTORY_LONG_LIST);
                while (todo) {
                    const int src = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const unsigned ws = (unsigned)__shfl((int)s, src, 64), we = (unsigned)__shfl((int)e, src, 64);
                    unsigned long long last = 0, bound = 0;
                    for (unsigned pass = 0; pass <= we - ws; pass++) {
                        const unsigned long long m = wave_min_u64(chain_pass(keys, ws + lane, we, 64u, last, bound, flags, un));
                        if (m == RF_NONE) break;
                        if (lane == 0 && (unsigned)m < un) flags[(unsigned)m] = 1;
                        last = m, bound = chain_bound(m, period);
                    }
                }
            }
            __syncthreads();                                   // the offsets are read, the keep bytes stored
        }
        // step 4: the survivors in stored order.  flags[i] was written by whichever thread walked row i's class: behind
        // the band loop's last barrier
        EV *dst = reinterpret_cast<EV *>(a.out) + e0;
        long long done = 0;
        unsigned kept = 0, removed = 0, passed = 0;
        int buf = 0;
        for (long long t0 = 0; t0 < n; t0 += EV_THREADS, buf ^= 1) {
            const long long i = t0 + threadIdx.x;
            bool ok = false;
            EV e = {};
            if (i < n) {
                e = ev[i];
                int x, y, p;
                const bool cnt = counted_event(e, H, W, 0, 0, x, y, p);
                ok = !cnt || flags[i] != 0;
                kept += cnt && ok, removed += cnt && !ok, passed += !cnt;
                if (a.keep) a.keep[e0 + i] = ok ? 1 : 0;
            }
            const unsigned long long mask = __ballot(ok);
            const int before = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wave_cnt[buf * EV_WAVES + wave] = __popcll(mask);
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int w = 0; w < EV_WAVES; w++) {
                const int c = wave_cnt[buf * EV_WAVES + w];
                base += w < wave ? c : 0;
                total += c;
            }
            if (ok) dst[done + base + before] = e;
            done += total;
        }
        if (a.stats) {
            const unsigned long long kr = block_sum_u64((unsigned long long)kept | ((unsigned long long)removed << 32), scratch);
            const unsigned long long ps = block_sum_u64(passed, scratch);
            if (threadIdx.x == 0) a.stats[b] = ec_refractory_stats{(unsigned)kr, (unsigned)(kr >> 32), (unsigned)ps};
        }
        if (threadIdx.x == 0) a.counts[b] = done;
        __syncthreads();                                       // scratch is read: the next sample may write it
    }
}

// Row bands: as many rows as RF_CLASS_WORDS - 1 classes hold (W, per polarity 2 W, classes a row), evened out over the bands.
// No halo: a class never leaves its band.  bands == 0: the entry points refuse this sensor.
struct RfPlan {
    int rows_per_band, bands;
};
inline RfPlan refractory_plan(int H, int W, int per_polarity)
{
    RfPlan p = {};
    if (H <= 0 || W <= 0 || W > 65536 || (per_polarity != 0 && per_polarity != 1)) return p;
    const int rows = (RF_CLASS_WORDS - 1) / (W * (per_polarity + 1));
    if (rows < 1) return p;
    p.bands = ec::ceil_div(H, std::min(H, rows));
    p.rows_per_band = ec::ceil_div(H, p.bands);
    return p;
}

inline size_t refractory_slot_bytes(int cap) { return (size_t)cap * 8 + ((size_t)cap + 15) / 16 * 16; }

inline size_t refractory_workspace_bytes(const ec_refractory_params *prm, int B)
{
    if (!prm || B <= 0 || prm->max_sample_events <= 0 || refractory_plan(prm->H, prm->W, prm->per_polarity).bands == 0) return 0;
    return refractory_slot_bytes(prm->max_sample_events) * (size_t)std::min<int>(B, EC_REFRACTORY_MAX_GROUPS);
}

template <typename EV>
int launch_refractory(const void *events, const int64_t *sample_range, int B, const ec_refractory_params *prm, void *events_out,
                      int64_t *counts, uint8_t *keep, ec_refractory_stats *stats, void *workspace, size_t workspace_bytes,
                      ec_stream_t stream)
{
    int rc;
    if (launch_is_over("ec_refractory_events", prm, 'B', B, events && sample_range && events_out && counts && workspace, rc)) return rc;
    EC_REQUIRE(events != events_out, "ec_refractory_events: in-place operation is not supported");
    EC_REQUIRE(prm->H > 0 && prm->W > 0, "ec_refractory_events: bad shape (%d,%d)", prm->H, prm->W);
    EC_REQUIRE(prm->period_us >= 1u && prm->period_us <= (uint32_t)EC_REFRACTORY_MAX_PERIOD_US,
               "ec_refractory_events: period_us=%u outside 1 .. %d", prm->period_us, (int)EC_REFRACTORY_MAX_PERIOD_US);
    EC_REQUIRE(prm->per_polarity == 0 || prm->per_polarity == 1, "ec_refractory_events: per_polarity=%d is neither 0 nor 1",
               prm->per_polarity);
    EC_REQUIRE(prm->max_sample_events > 0, "ec_refractory_events: max_sample_events=%d (a bound: it sizes the workspace)",
               prm->max_sample_events);
    EC_REQUIRE((((uintptr_t)events | (uintptr_t)events_out) & (sizeof(EV) - 1)) == 0,
               "ec_refractory_events: events and events_out must be %d-byte aligned", (int)sizeof(EV));
    EC_REQUIRE(((uintptr_t)counts & 7) == 0 && ((uintptr_t)stats & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
               "ec_refractory_events: counts must be 8-byte, stats 4-byte and workspace 16-byte aligned");
    const RfPlan plan = refractory_plan(prm->H, prm->W, prm->per_polarity);
    EC_REQUIRE(plan.bands > 0, "ec_refractory_events: W=%d too wide for an LDS band of one row (%d classes a pixel)", prm->W,
               prm->per_polarity + 1);
    const size_t need = refractory_workspace_bytes(prm, B);
    if (workspace_bytes < need)
        return ec::fail(EC_ERR_WORKSPACE, "ec_refractory_events: workspace %zu < %zu bytes (ec_refractory_workspace_bytes)", workspace_bytes, need);

    RfArgs a = {};
    a.events = events;
    a.range = reinterpret_cast<const long long *>(sample_range);
    a.H = prm->H, a.W = prm->W, a.B = B, a.cpp = prm->per_polarity + 1;
    a.period = prm->period_us;
    a.out = events_out, a.counts = reinterpret_cast<long long *>(counts), a.keep = keep, a.stats = stats;
    a.ws = static_cast<unsigned char *>(workspace);
    a.slot_bytes = (long long)refractory_slot_bytes(prm->max_sample_events);
    a.cap = prm->max_sample_events;
    a.rows_per_band = plan.rows_per_band, a.bands = plan.bands;

    // algorithmic bytes: every event read once and at most written once
    return launch_form(refractory_kernel<EV>, std::min<int>(B, EC_REFRACTORY_MAX_GROUPS), RF_LDS_BYTES, ec::PROF_REFRACTORY,
                       2.0 * event_bytes<EV>(0, 0, 0, prm->total_events), stream, a);
}

// ---------------------------------------------------------------------------------------------
// fixed-duration event windows (include/eventclip_time_windows.h states the definition, steps 1 - 7).
//
// bounds[b, k] are counts of ticks below an edge, i.e. the first row at or above it.  In a sorted sample that row is the one
// place where the ticks step over the edge: the thread holding row i looks at tick_{i-1} and tick_i -- which is also the
// whole order check -- and, where the tick rises, writes i into every edge e with tick_{i-1} < e <= tick_i.  Row `begin` has
// no predecessor (tick -inf), and one virtual row at `end` carries tick +inf: every edge of a sorted sample is written
// exactly once, by a plain store, with no atomics on the bounds and no search.  The edges of kind `side` are an arithmetic
// progression A + k stride (from_last: A - k stride), so the k of (tick_{i-1}, tick_i] are a range between two integer
// divisions, clipped to the rows of bounds the sample owns; a silent gap makes one thread write all the edges inside it, at
// most max_windows of each kind.
// A sample's n + 1 rows are cut into slices of TW_SLICE rows; workgroup (sample, w) walks slices w, w + walkers, ...  (the
// grid is sized from total_events, but whatever it is every slice is walked once).  Per slice a thread takes TW_UNROLL rows
// TW_THREADS apart, all loads in flight at once (for_events' pattern); the predecessor's tick comes from the lane below, for
// lane 0 from the wave below through LDS, and for the slice's first row from the one row before the slice.
// Descents are counted per thread, summed per wave, and added with one atomic per wave that saw any; that wave also puts
// windows to -1.  time_windows_init_kernel has zeroed both words before.
// ---------------------------------------------------------------------------------------------
constexpr int TW_SLICE = EC_TIME_WINDOWS_SLICE_ROWS, TW_UNROLL = EC_TIME_WINDOWS_UNROLL;
constexpr int TW_THREADS = TW_SLICE / TW_UNROLL, TW_WAVES = TW_THREADS / 64;
constexpr int TW_MAX_GROUPS = 4096;                    // workgroups of one launch, unless B alone is more
static_assert(TW_THREADS * TW_UNROLL == TW_SLICE && TW_WAVES * 64 == TW_THREADS && TW_THREADS <= 1024, "slice = unroll x whole waves");

struct TwArgs {
    const void *events;      // float4 (x, y, t, p) or packed 8-byte events
    const long long *range;  // [B,2]
    int B, walkers;          // workgroups per sample
    unsigned dt, stride;
    unsigned magic;          // floor(x / stride) == (x * magic) >> shift for 0 <= x < 2^31 (tw_magic)
    int shift;
    int max_windows, from_last;
    long long *bounds;       // [B, max_windows, 2]
    ec_time_windows_stats *stats;
};

__global__ void time_windows_init_kernel(const TwArgs a)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    a.stats[b].windows = 0;                                              // an empty sample: this and nothing else
    if (a.range[2 * b] < a.range[2 * b + 1]) a.stats[b].unsorted = 0;
}

// floor(x / stride) for 0 <= x < 2^31 -- the operands of every division below are a difference of two of tick, tick + 1 and
// tick - dt, plus stride - 1 where the quotient is rounded up -- as a multiplication by the host's round-up reciprocal (Granlund & Montgomery 1994: magic = ceil(2^(31 + l) /
// stride), l = ceil(log2 stride), is below 2^32 and exact for every 31-bit x; the product stays below 2^63).  A 32-bit
// division is some 30 instructions, and a row asks for up to four.
__device__ __forceinline__ long long tw_div(const TwArgs &a, long long x)
{
    return (long long)(((unsigned long long)(unsigned)x * a.magic) >> a.shift);
}
inline void tw_magic(unsigned stride, unsigned &magic, int &shift)
{
    int l = 0;
    while ((1ull << l) < stride) l++;
    shift = 31 + l;
    magic = (unsigned)(((1ull << shift) + stride - 1) / stride);
}

// Row `row` (tick c, predecessor's tick p; first: no predecessor, last: the virtual row) into the edges it is the first
// row at or above.  windows K of the sample are written: k in 0 .. K - 1.
__device__ __forceinline__ void tw_scatter(const TwArgs &a, long long t_first, long long t_last, long long K, long long *bounds,
                                           bool first, bool last, long long p, long long c, long long row)
{
    const long long dt = a.dt;
    const unsigned stride = a.stride;
#pragma unroll
    for (int side = 0; side < 2; side++) {
        long long klo, khi;
        if (!a.from_last) {                            // edge k = A + k stride, rising with k
            const long long A = t_first + (side ? dt : 0);
            klo = first || p < A ? 0 : tw_div(a, p - A) + 1;
            khi = last ? K - 1 : c < A ? -1 : min(tw_div(a, c - A), K - 1);
        } else {                                       // edge k = A - k stride, falling with k: the first row with d < ...
            const long long A = t_last + 1 - (side ? 0 : dt);
            klo = last || A <= c ? 0 : tw_div(a, A - c + stride - 1);
            khi = first ? K - 1 : A <= p ? -1 : min(tw_div(a, A - p + stride - 1) - 1, K - 1);
        }
        for (int k = (int)min(klo, K); k <= (int)khi; k++) bounds[2 * k + side] = row;          // (khi < K <= max_windows)
    }
}

template <typename EV>
__global__ __launch_bounds__(TW_THREADS) void time_windows_kernel(const TwArgs a)
{
    __shared__ unsigned tail[TW_UNROLL][TW_WAVES];     // the tick of every wave's last lane, per round
    const int b = blockIdx.x / a.walkers, w = blockIdx.x - b * a.walkers;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long e0 = a.range[2 * b], n = a.range[2 * b + 1] - e0;
    if (n <= 0 || (long long)w * TW_SLICE > n) return;                   // (uniform) rows 0 .. n: n is the virtual one
    const EV *ev = reinterpret_cast<const EV *>(a.events) + e0;
    const long long t_first = tick_of(ev[0]), t_last = tick_of(ev[n - 1]);
    // (t_last < t_first only in an unsorted sample, whose bounds mean nothing: any count that keeps the stores in its rows)
    const long long windows = t_last >= t_first ? tw_div(a, t_last - t_first) + 1 : 1;
    const long long K = min(windows, (long long)a.max_windows);
    long long *bounds = a.bounds + (long long)b * a.max_windows * 2;
    unsigned descents = 0;
    for (long long s = w; s * TW_SLICE <= n; s += a.walkers) {
        const long long j0 = s * TW_SLICE + threadIdx.x;
        EV e[TW_UNROLL];
#pragma unroll
        for (int k = 0; k < TW_UNROLL; k++) {
            const long long j = j0 + (long long)k * TW_THREADS;
            e[k] = ev[j < n ? j : n - 1];                                // (rows >= n re-read the last event)
        }
        unsigned before = 0;                                             // the one row before the slice (s TW_SLICE - 1 < n)
        if (threadIdx.x == 0 && s > 0) before = tick_of(ev[s * TW_SLICE - 1]);
        __asm__ volatile("" ::: "memory");
        unsigned c[TW_UNROLL];
#pragma unroll
        for (int k = 0; k < TW_UNROLL; k++) {
            c[k] = tick_of(e[k]);
            if (lane == 63) tail[k][wave] = c[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TW_UNROLL; k++) {
            const long long j = j0 + (long long)k * TW_THREADS;
            unsigned p = __shfl_up(c[k], 1, 64);
            if (lane == 0) p = wave > 0 ? tail[k][wave - 1] : k > 0 ? tail[k - 1][TW_WAVES - 1] : before;
            const bool first = j == 0, last = j == n;
            if (j <= n) {
                descents += !first && !last && c[k] < p;
                if (first || last || c[k] > p) tw_scatter(a, t_first, t_last, K, bounds, first, last, p, c[k], e0 + j);
            }
        }
        __syncthreads();                                                 // tail is read: the next slice may write it
    }
    const unsigned in_wave = wave_sum_u32(descents);
    if (lane == 0 && in_wave > 0) {
        atomicAdd(&a.stats[b].unsorted, in_wave);
        atomicExch(&a.stats[b].windows, -1);
    }
    if (w == 0 && threadIdx.x == 0) {
        a.stats[b].t_first = (unsigned)t_first, a.stats[b].t_last = (unsigned)t_last;
        atomicCAS(&a.stats[b].windows, 0, (int)windows);                 // unless a wave has put -1 there (windows >= 1)
    }
}

template <typename EV>
int launch_time_windows(const char *name, const void *events, const int64_t *sample_range, int B, const ec_time_windows_params *prm,
                        int64_t *bounds, ec_time_windows_stats *stats, ec_stream_t stream)
{
    int rc;
    if (launch_is_over(name, prm, 'B', B, events && sample_range && bounds && stats, rc)) return rc;
    EC_REQUIRE(prm->dt_us >= 1 && prm->dt_us <= (uint32_t)EC_TIME_WINDOWS_MAX_US, "%s: dt_us=%u outside 1 .. %d", name, prm->dt_us,
               (int)EC_TIME_WINDOWS_MAX_US);
    EC_REQUIRE(prm->stride_us >= 1 && prm->stride_us <= (uint32_t)EC_TIME_WINDOWS_MAX_US, "%s: stride_us=%u outside 1 .. %d", name,
               prm->stride_us, (int)EC_TIME_WINDOWS_MAX_US);
    EC_REQUIRE(prm->max_windows > 0, "%s: max_windows=%d", name, prm->max_windows);
    EC_REQUIRE(((uintptr_t)events & (sizeof(EV) - 1)) == 0, "%s: events must be %d-byte aligned", name, (int)sizeof(EV));
    EC_REQUIRE((((uintptr_t)sample_range | (uintptr_t)bounds) & 7) == 0 && ((uintptr_t)stats & 3) == 0,
               "%s: sample_range and bounds must be 8-byte and stats 4-byte aligned", name);

    TwArgs a = {};
    a.events = events;
    a.range = reinterpret_cast<const long long *>(sample_range);
    a.B = B;
    a.dt = prm->dt_us, a.stride = prm->stride_us;
    tw_magic(a.stride, a.magic, a.shift);
    a.max_windows = prm->max_windows, a.from_last = prm->from_last != 0;
    a.bounds = reinterpret_cast<long long *>(bounds), a.stats = stats;
    // no sample is longer than total_events: that many slices' worth of workgroups per sample, while the launch has them
    const long most = std::max(1L, (long)TW_MAX_GROUPS / B);
    a.walkers = (int)(prm->total_events > 0 ? std::min<long>(most, (long)(prm->total_events / TW_SLICE) + 1) : most);

    hipStream_t hs = static_cast<hipStream_t>(stream);
    // algorithmic bytes: every event read once, every pair of bounds written once
    ec::ProfScope prof(ec::PROF_EVENTS, hs, 0, event_bytes<EV>(0, 0, 0, prm->total_events) + 16.0 * B * prm->max_windows);
    hipLaunchKernelGGL(time_windows_init_kernel, dim3((unsigned)ec::ceil_div(B, 256)), dim3(256), 0, hs, a);
    hipLaunchKernelGGL(time_windows_kernel<EV>, dim3((unsigned)((long)B * a.walkers)), dim3(TW_THREADS), 0, hs, a);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}

}  // namespace

#ifdef EC_EVENTS_DIAG
extern "C" EC_API int ec_events_phase_times(unsigned long long *host, int frames)
{
    EC_REQUIRE(host && frames > 0 && frames <= 4096, "ec_events_phase_times: bad arguments");
    EC_CHECK_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_ev_phase), (size_t)frames * 8 * sizeof(unsigned long long)));
    return EC_OK;
}
#endif

extern "C" EC_API size_t ec_events_sort_workspace_bytes(const ec_events_params *prm)
{
    return prm ? events_plan(prm->H, prm->W, prm->max_frame_events, 0, false, events_cus()).worth_bytes : 0;
}

extern "C" EC_API int ec_events_to_frames(const float *events, const int64_t *frame_range, int F,
                                          const ec_events_params *prm, uint8_t *frames,
                                          int32_t *raw_counts, int32_t *kept_counts,
                                          ec_frame_stats *stats, ec_stream_t stream)
{
    return launch_events<float4>(events, frame_range, F, prm, frames, raw_counts, kept_counts, stats,
                                 stream);
}

extern "C" EC_API int ec_events_to_frames_packed(const uint64_t *events, const int64_t *frame_range,
                                                 int F, const ec_events_params *prm, uint8_t *frames,
                                                 int32_t *raw_counts, int32_t *kept_counts,
                                                 ec_frame_stats *stats, ec_stream_t stream)
{
    return launch_events<packed_t>(events, frame_range, F, prm, frames, raw_counts, kept_counts, stats,
                                   stream);
}

extern "C" EC_API int ec_events_to_time_surface(const float *events, const int64_t *frame_range, int F,
                                                const ec_time_surface_params *prm, uint8_t *frames, int32_t *last,
                                                ec_surface_stats *stats, ec_stream_t stream)
{
    return launch_time_surface<float4>(events, frame_range, F, prm, frames, last, stats, stream);
}

extern "C" EC_API int ec_events_to_time_surface_packed(const uint64_t *events, const int64_t *frame_range, int F,
                                                       const ec_time_surface_params *prm, uint8_t *frames, int32_t *last,
                                                       ec_surface_stats *stats, ec_stream_t stream)
{
    return launch_time_surface<packed_t>(events, frame_range, F, prm, frames, last, stats, stream);
}

extern "C" EC_API int ec_events_to_voxel_grid(const float *events, const int64_t *frame_range, int F,
                                              const ec_voxel_grid_params *prm, uint8_t *frames, int32_t *grid,
                                              ec_voxel_stats *stats, ec_stream_t stream)
{
    return launch_voxel_grid<float4>(events, frame_range, F, prm, frames, grid, stats, stream);
}

extern "C" EC_API int ec_events_to_voxel_grid_packed(const uint64_t *events, const int64_t *frame_range, int F,
                                                     const ec_voxel_grid_params *prm, uint8_t *frames, int32_t *grid,
                                                     ec_voxel_stats *stats, ec_stream_t stream)
{
    return launch_voxel_grid<packed_t>(events, frame_range, F, prm, frames, grid, stats, stream);
}

extern "C" EC_API int ec_voxel_grid_bands(int H, int W, int bins) { return voxel_grid_plan(H, W, bins).bands; }

extern "C" EC_API int ec_denoise_events(const float *events, const int64_t *sample_range, int B, const ec_denoise_params *prm,
                                        float *events_out, int64_t *counts, uint8_t *keep, ec_denoise_stats *stats,
                                        void *workspace, size_t workspace_bytes, ec_stream_t stream)
{
    return launch_denoise<float4>(events, sample_range, B, prm, events_out, counts, keep, stats, workspace, workspace_bytes, stream);
}

extern "C" EC_API int ec_denoise_events_packed(const uint64_t *events, const int64_t *sample_range, int B,
                                               const ec_denoise_params *prm, uint64_t *events_out, int64_t *counts,
                                               uint8_t *keep, ec_denoise_stats *stats, void *workspace,
                                               size_t workspace_bytes, ec_stream_t stream)
{
    return launch_denoise<packed_t>(events, sample_range, B, prm, events_out, counts, keep, stats, workspace, workspace_bytes, stream);
}

extern "C" EC_API size_t ec_denoise_workspace_bytes(const ec_denoise_params *prm, int B) { return denoise_workspace_bytes(prm, B); }

extern "C" EC_API int ec_denoise_bands(int H, int W, int radius) { return denoise_plan(H, W, radius).bands; }

extern "C" EC_API int ec_refractory_events(const float *events, const int64_t *sample_range, int B, const ec_refractory_params *prm,
                                           float *events_out, int64_t *counts, uint8_t *keep, ec_refractory_stats *stats,
                                           void *workspace, size_t workspace_bytes, ec_stream_t stream)
{
    return launch_refractory<float4>(events, sample_range, B, prm, events_out, counts, keep, stats, workspace, workspace_bytes, stream);
}

extern "C" EC_API int ec_refractory_events_packed(const uint64_t *events, const int64_t *sample_range, int B,
                                                  const ec_refractory_params *prm, uint64_t *events_out, int64_t *counts,
                                                  uint8_t *keep, ec_refractory_stats *stats, void *workspace,
                                                  size_t workspace_bytes, ec_stream_t stream)
{
    return launch_refractory<packed_t>(events, sample_range, B, prm, events_out, counts, keep, stats, workspace, workspace_bytes, stream);
}

extern "C" EC_API size_t ec_refractory_workspace_bytes(const ec_refractory_params *prm, int B) { return refractory_workspace_bytes(prm, B); }

extern "C" EC_API int ec_refractory_bands(int H, int W, int per_polarity) { return refractory_plan(H, W, per_polarity).bands; }

extern "C" EC_API int ec_time_windows(const float *events, const int64_t *sample_range, int B, const ec_time_windows_params *prm,
                                      int64_t *bounds, ec_time_windows_stats *stats, ec_stream_t stream)
{
    return launch_time_windows<float4>("ec_time_windows", events, sample_range, B, prm, bounds, stats, stream);
}

extern "C" EC_API int ec_time_windows_packed(const uint64_t *events, const int64_t *sample_range, int B,
                                             const ec_time_windows_params *prm, int64_t *bounds, ec_time_windows_stats *stats,
                                             ec_stream_t stream)
{
    return launch_time_windows<packed_t>("ec_time_windows_packed", events, sample_range, B, prm, bounds, stats, stream);
}

extern "C" EC_API int ec_center_events(float *events, const int64_t *sample_range, int B, int H, int W,
                                       ec_stream_t stream)
{
    return center_events<float4, center_events_kernel>("ec_center_events", events, sample_range, B, H, W, stream);
}

extern "C" EC_API int ec_center_events_packed(uint64_t *events, const int64_t *sample_range, int B,
                                              int H, int W, ec_stream_t stream)
{
    return center_events<packed_t, center_packed_kernel>("ec_center_events_packed", events, sample_range, B, H, W, stream);
}

extern "C" EC_API int ec_pack_events(const float *events, int64_t n, uint64_t *packed,
                                     uint32_t *n_unrepresentable, ec_stream_t stream)
{
    EC_REQUIRE(n >= 0, "ec_pack_events: n=%lld", (long long)n);
    if (n == 0) return EC_OK;
    EC_REQUIRE(events && packed, "ec_pack_events: null buffer");
    EC_REQUIRE(((uintptr_t)events & 15) == 0 && ((uintptr_t)packed & 7) == 0,
               "ec_pack_events: events must be 16-byte and packed 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_unrepresentable) EC_CHECK_HIP(hipMemsetAsync(n_unrepresentable, 0, 4, s));
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(pack_events_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                       s, reinterpret_cast<const float4 *>(events), (long long)n,
                       reinterpret_cast<packed_t *>(packed), n_unrepresentable);
    EC_CHECK_HIP(hipGetLastError());
    return EC_OK;
}
