/*
 * eventclip_time_windows.h -- fixed-duration event windows: the part of libeventclip_hip.so's C ABI that ABI 612 added.
 *
 * The image forms (eventclip_hip.h, eventclip_time_surface.h, eventclip_voxel_grid.h) take arbitrary (begin, end) row
 * ranges; the only way the project cut a recording into such ranges was every N events (split_method='event_count', the
 * reference's only method), on the host, from event counts alone.  This is the other standard way to frame an event stream:
 * a window of fixed DURATION, optionally hopped by less than its length (split_method='time_window').  The ranges are found
 * on the device, where the events live, exactly, and with the ordering they presuppose checked.  The reference has no such
 * split; the definition below is the specification, restated in numpy by tests/time_windows_ref.py.
 *
 * Conventions (stream, return codes, ec_last_error, EC_DEVICE, the packed 8-byte event) are eventclip_hip.h's, and
 * EC_ABI_VERSION there covers this file.  Its own file so that eventclip_hip.h stays declaration for declaration what
 * ABI 608 stated; eventclip_amd/vis.py derives its bindings from this text the way eventclip_amd/_lib.py does from that one.
 *
 * A sample is the event rows [begin, end) of its sample_range, n = end - begin > 0.  Parameters: dt_us (the window) and
 * stride_us (the hop) in 1 .. 2^30 - 1, max_windows > 0, from_last.
 *   1. tick     integer microseconds by rule 2 of eventclip_time_surface.h: EC_PACKED_T(e) of a packed event,
 *               clip(rint((double)t * 1e6), 0, 2^30 - 1) of a float row.
 *   2. order    unsorted = #{ i in (begin, end) : tick_i < tick_{i-1} }.  Steps 4 and 5 hold for samples with
 *               unsorted == 0.  Nothing is sorted for the caller.
 *   3. span     t_first = tick_begin, t_last = tick_{end-1}, windows = (t_last - t_first) / stride_us + 1 by integer
 *               division.  With stride_us <= dt_us every event lies in at least one window; with stride_us > dt_us the
 *               events between two windows lie in none.
 *   4. window k, from_last == 0    covers the ticks [lo_k, hi_k) = [t_first + k stride_us, t_first + k stride_us + dt_us):
 *                   bounds[b, k] = (begin + #{tick_i < lo_k}, begin + #{tick_i < hi_k}).
 *               An event on a lower edge belongs to that window, an event on an upper edge does not.
 *   5. window k, from_last != 0    with d_i = t_last - tick_i, the rows with k stride_us <= d_i < k stride_us + dt_us:
 *                   bounds[b, k] = (begin + #{d_i >= k stride_us + dt_us}, begin + #{d_i >= k stride_us}).
 *               These are the windows of the time-flipped stream (the t' = t_last - t of test-time augmentation), given as
 *               STORED rows: window 0 ends at the last event.
 *   6. output   bounds is int64 [B, max_windows, 2]; rows k < min(windows, max_windows) of sample b are written, the rows
 *               behind them are not touched.  stats[b] = {t_first, t_last, unsorted, windows}: windows is the full count
 *               even when it exceeds max_windows.  For a sample with unsorted > 0, stats.windows = -1 and its own
 *               max_windows rows of bounds are unspecified.  A sample with begin >= end gets windows = 0 and nothing else of
 *               it is written, not even the other words of its stats.  Whatever the input, nothing outside a sample's own rows of bounds and
 *               stats is written.  An empty window (begin == end in its pair) is a legal result.
 *   7. arithmetic   the edges reach 2^31 and beyond (a tick of 2^30 - 1 plus dt_us of 2^30 - 1 plus k stride_us): every edge
 *               is formed and compared in 64-bit integers.
 *
 * Cost.  One pass over the events, each read once: the thread holding row i compares tick_{i-1} with tick_i (that is the
 * order check) and, where the tick rises, writes i into every window edge e with tick_{i-1} < e <= tick_i -- for a sorted
 * sample every edge is written exactly once, by plain stores, so the result is deterministic.  A sample is cut into slices
 * of EC_TIME_WINDOWS_SLICE_ROWS rows, one workgroup per (sample, slice) while the launch has them: one long recording
 * (B == 1) spreads over the device.  A silent gap makes one thread write the edges of all the windows inside it, a loop
 * bounded by max_windows.  No workspace.
 */
#ifndef EVENTCLIP_TIME_WINDOWS_H
#define EVENTCLIP_TIME_WINDOWS_H

#include "eventclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { EC_TIME_WINDOWS_MAX_US = 1073741823,     /* the most of dt_us and of stride_us: 2^30 - 1, the range of a tick */
       EC_TIME_WINDOWS_SLICE_ROWS = 2048,       /* rows of one slice: a workgroup's share of a sample at a time */
       EC_TIME_WINDOWS_UNROLL = 8 /* loads in flight per thread: a slice is this many rounds of SLICE_ROWS / UNROLL threads */ };

typedef struct {
    uint32_t t_first;    /* tick of row begin */
    uint32_t t_last;     /* tick of row end - 1 */
    uint32_t unsorted;   /* rows whose tick is below their predecessor's */
    int32_t windows;     /* (t_last - t_first) / stride_us + 1; -1 if unsorted > 0; 0 for an empty sample */
} ec_time_windows_stats;

typedef struct {
    uint32_t dt_us, stride_us;   /* the window and the hop, 1 .. EC_TIME_WINDOWS_MAX_US */
    int max_windows;          /* rows of bounds per sample, > 0 */
    int from_last;            /* 0: windows counted from the first event; else from the last, backwards (step 5) */
    int64_t total_events;     /* sum of (end - begin) over sample_range if the caller knows it, else 0: sizes the grid
                                 (any value gives the same result) and states the launch's algorithmic bytes */
} ec_time_windows_params;

/*
 * events:       float32 [n_events_total, 4] rows (x, y, t, p), device, 16-byte aligned.
 * sample_range: int64 [B, 2] (begin, end) event-row indices per sample, device, 8-byte aligned.  B == 0 is EC_OK and
 *               touches nothing.
 * bounds:       int64 [B, max_windows, 2], device, 8-byte aligned (out).
 * stats:        ec_time_windows_stats [B], device, 4-byte aligned (out).
 * EC_ERR_INVALID: a null or misaligned buffer, dt_us == 0, stride_us == 0, either above EC_TIME_WINDOWS_MAX_US,
 * max_windows <= 0.  A refused call writes nothing.
 */
EC_API int ec_time_windows(const float *events, const int64_t *sample_range, int B, const ec_time_windows_params *prm,
                           int64_t *bounds, EC_DEVICE ec_time_windows_stats *stats, ec_stream_t stream);

/* the same on packed events (eventclip_hip.h, EC_PACKED_*), 8-byte aligned */
EC_API int ec_time_windows_packed(const uint64_t *events, const int64_t *sample_range, int B,
                                  const ec_time_windows_params *prm, int64_t *bounds,
                                  EC_DEVICE ec_time_windows_stats *stats, ec_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* EVENTCLIP_TIME_WINDOWS_H */
