/*
 * eventclip_denoise.h -- background-activity event denoising: the part of libeventclip_hip.so's C ABI that ABI 611 added.
 *
 * The three image forms (eventclip_hip.h, eventclip_time_surface.h, eventclip_voxel_grid.h) take an event stream as it
 * arrives; the only noise handling is the histogram's hot-pixel threshold, which catches pixels that fire too OFTEN.  The
 * dominant noise of a real DVS sensor is the opposite: isolated background-activity events.  This is the standard first
 * stage of an event pipeline, the spatio-temporal correlation filter (background-activity filter, Delbruck 2008): an
 * event stays only if a NEIGHBOURING pixel fired shortly before it.  It works on the events themselves, before any
 * binning, so it serves all three forms and every other consumer of events.  The reference has no such filter; the
 * definition below is the specification, restated in numpy by tests/denoise_ref.py.
 *
 * Conventions (stream, return codes, ec_last_error, EC_DEVICE, the packed 8-byte event) are eventclip_hip.h's, and
 * EC_ABI_VERSION there covers this file.  Its own file so that eventclip_hip.h stays declaration for declaration what
 * ABI 608 stated; eventclip_amd/vis.py derives its bindings from this text the way eventclip_amd/_lib.py does from that one.
 *
 * A sample is the event rows [begin, end) of its sample_range on a sensor of (H, W).  Parameters: radius r in 1 .. 3,
 * dt_us in 0 .. 2^30 - 1.
 *   1. parse    x, y, p exactly as ec_events_to_frames does, of float rows (truncating casts) and of packed events, with
 *               no flip and no negation: flips are view transforms, applied later to the survivors.
 *   2. tick     integer microseconds by rule 2 of eventclip_time_surface.h: EC_PACKED_T(e) of a packed event,
 *               clip(rint((double)t * 1e6), 0, 2^30 - 1) of a float event.
 *   3. counted(i)    p_i != 0 and the pixel lies inside the sensor: the events a frame kernel would count.
 *   4. supported(i)  counted(i) and there is a j != i in the same sample with
 *                        counted(j),
 *                        max(|x_j - x_i|, |y_j - y_i|) <= r,
 *                        (x_j, y_j) != (x_i, y_i),
 *                        tick_i - dt_us <= tick_j <= tick_i.
 *               The polarity of j does not matter.  The own pixel never supports: a hot pixel does not vouch for itself,
 *               and an isolated one is removed whatever its rate (the classic filter; it complements `thresh`).  Equal
 *               ticks support each other.  The predicate uses ticks only, never row order: the result does NOT depend on
 *               the order of the events.
 *   5. output   the rows with supported(i) or not counted(i) are copied bit for bit to events_out[begin : begin + count],
 *               in stored order.  Rows that are not counted pass through and support nothing, so the frame kernels'
 *               `dropped` statistic sees them as before.  counts[b] = count.  keep[i] = 1 for a written row, 0 for a
 *               removed one.  stats[b] = {kept, removed, passed}: supported counted, unsupported counted, not counted;
 *               kept + passed == count.
 * Samples are disjoint.  Rows outside every sample, and events_out rows behind a sample's count, are not written.
 * events_out must not alias events.  B == 0 is EC_OK and touches nothing.
 *
 * max_sample_events is a BOUND, not a hint: it sizes the workspace.  A sample with more rows than that is not filtered:
 * its counts[b] is -1, its stats are {0, 0, 0}, and nothing else of it is written (the Python layers refuse such a call
 * on the host).
 *
 * Cost.  The kernel sorts the ticks of a row band by pixel (a counting sort in LDS and the workspace) and every event
 * scans the tick lists of its (2r+1)^2 - 1 neighbour pixels, with an early exit at the first supporter.  The work is the
 * sum over events of their neighbours' list lengths: linear in the events for a stream spread over the sensor, and
 * quadratic only when most of a sample sits on two adjacent pixels (n/2 events each: n^2 / 4 comparisons when none
 * supports).  No test feeds more than 4096 events to any two adjacent pixels.  The events are read 3 times per row band
 * (ec_denoise_bands) plus once to compact.
 */
#ifndef EVENTCLIP_DENOISE_H
#define EVENTCLIP_DENOISE_H

#include "eventclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { EC_DENOISE_MIN_RADIUS = 1, EC_DENOISE_MAX_RADIUS = 3, EC_DENOISE_MAX_DT_US = 1073741823,
       EC_DENOISE_MAX_GROUPS = 256 /* the most workgroups of one launch: each owns one slot of the workspace */ };

typedef struct {
    uint32_t kept;       /* counted and supported: written */
    uint32_t removed;    /* counted and not supported: the noise */
    uint32_t passed;     /* not counted (p == 0 or outside the sensor): written */
} ec_denoise_stats;

typedef struct {
    int H, W;                 /* sensor resolution */
    int radius;               /* r, EC_DENOISE_MIN_RADIUS .. EC_DENOISE_MAX_RADIUS (Chebyshev distance) */
    uint32_t dt_us;           /* the support window, 0 .. EC_DENOISE_MAX_DT_US */
    int max_sample_events;    /* upper bound of (end - begin) over sample_range, > 0: sizes the workspace */
    int64_t total_events;     /* sum of (end - begin) over sample_range if the caller knows it, else 0:
                                 only states the launch's algorithmic bytes to ec_profile_end */
} ec_denoise_params;

/*
 * events:       float32 [n_events_total, 4] rows (x, y, t, p), device, 16-byte aligned.
 * sample_range: int64 [B, 2] (begin, end) event-row indices per sample, device.  B == 0 is EC_OK and touches nothing.
 * events_out:   float32 [n_events_total, 4], device, 16-byte aligned (out); not events.
 * counts:       int64 [B], device (out).
 * keep:         optional uint8 [n_events_total], device (out).
 * stats:        optional ec_denoise_stats [B] (out).
 * workspace:    device, 16-byte aligned, at least ec_denoise_workspace_bytes(prm, B) bytes; its contents mean nothing
 *               before or after the call.
 * EC_ERR_INVALID: a null or misaligned buffer, events_out == events, a radius outside 1 .. 3, dt_us above
 * EC_DENOISE_MAX_DT_US, max_sample_events <= 0, a sensor the kernel's LDS band cannot hold 2 radius + 1 rows of
 * (ec_denoise_bands == 0).  EC_ERR_WORKSPACE: workspace_bytes too small.  A refused call writes nothing.
 */
EC_API int ec_denoise_events(const float *events, const int64_t *sample_range, int B, const ec_denoise_params *prm,
                             float *events_out, int64_t *counts, uint8_t *keep, EC_DEVICE ec_denoise_stats *stats,
                             void *workspace, size_t workspace_bytes, ec_stream_t stream);

/* the same on packed events (eventclip_hip.h, EC_PACKED_*), in and out, 8-byte aligned */
EC_API int ec_denoise_events_packed(const uint64_t *events, const int64_t *sample_range, int B,
                                    const ec_denoise_params *prm, uint64_t *events_out, int64_t *counts, uint8_t *keep,
                                    EC_DEVICE ec_denoise_stats *stats, void *workspace, size_t workspace_bytes,
                                    ec_stream_t stream);

/* host only: the bytes of workspace a launch of B samples with these parameters needs; 0 for parameters or a B the entry
 * points refuse */
EC_API size_t ec_denoise_workspace_bytes(const ec_denoise_params *prm, int B);

/* host only: the number of row bands the kernel cuts a sensor of (H, W) into at this radius; 0 for what is refused */
EC_API int ec_denoise_bands(int H, int W, int radius);

#ifdef __cplusplus
}
#endif

#endif /* EVENTCLIP_DENOISE_H */
