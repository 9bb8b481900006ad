/*
 * eventclip_refractory.h -- per-pixel refractory-period event filtering: the part of libeventclip_hip.so's C ABI that ABI 613
 * added.
 *
 * The second of the two filters an event pipeline puts in front of a representation (jAER, DV and Tonic ship it beside the
 * background-activity filter of eventclip_denoise.h): after a pixel fires it is blind for `period` microseconds.  That caps
 * every pixel's rate at 1 / period whatever its neighbours do -- the hot pixel with live neighbours that `denoise` keeps,
 * the one hot pixel that sets a voxel grid's contrast -- and makes a time surface show the onset of an edge rather than its
 * last ringing event.  It works on the events themselves, before any binning, so it serves all three forms and every other
 * consumer of events.  The reference has no such filter; the definition below is the specification, restated twice in numpy
 * by tests/refractory_ref.py.
 *
 * Conventions (stream, return codes, ec_last_error, EC_DEVICE, the packed 8-byte event) are eventclip_hip.h's, and
 * EC_ABI_VERSION there covers this file.  eventclip_amd/vis.py derives its bindings from this text.
 *
 * A sample is the event rows [begin, end) of its sample_range on a sensor of (H, W).  Parameters: period_us in
 * 1 .. 2^30 - 1, per_polarity 0 or 1.
 *   1. parse, tick, counted    exactly steps 1 - 3 of eventclip_denoise.h: x, y, p as ec_events_to_frames parses them (float
 *               rows: truncating casts), no flip and no negation; the tick is EC_PACKED_T(e) of a packed event and
 *               clip(rint((double)t * 1e6), 0, 2^30 - 1) of a float row; counted(i) means p_i != 0 and the pixel lies
 *               inside the sensor.
 *   2. class(i) the pixel (x_i, y_i); with per_polarity the pair (pixel, sign of p_i): ON and OFF events have separate
 *               dead times, which matters for the two-channel time surface.
 *   3. chain    order the counted events of one class of one sample by (tick, row index) ascending: e_1, e_2, ...
 *               e_1 is kept.  e_m is kept iff  tick(e_m) - tick(the last KEPT event before e_m) >= period_us.
 *               The dead time is not retriggerable: a removed event does not extend it.  Among events of one class with
 *               equal ticks the lowest row index is kept (period_us >= 1 removes the others).  Row order enters through
 *               that tie rule ONLY: on a stream with no equal ticks inside a class the keep set does not depend on the
 *               order of the rows, and the rows need not be sorted by time.
 *               (Tonic's rule t > last + period is this rule with period_us + 1.)
 *   4. output   the rows that are kept or not counted are copied bit for bit to events_out[begin : begin + count], in
 *               stored order.  Rows that are not counted pass through and start no dead time, so the frame kernels'
 *               `dropped` statistic sees them as before.  counts[b] = count.  keep[i] = 1 for a written row, 0 for a
 *               removed one.  stats[b] = {kept, removed, passed}: counted and kept, counted and removed, not counted;
 *               kept + passed == count.
 * Samples are disjoint.  Rows outside every sample, and events_out rows behind a sample's count, are not written.
 * events_out must not alias events.  B == 0 is EC_OK and touches nothing.
 *
 * max_sample_events is a BOUND, not a hint: it sizes the workspace.  A sample with more rows than that is not filtered:
 * its counts[b] is -1, its stats are {0, 0, 0}, and nothing else of it is written (the Python layers refuse such a call
 * on the host).
 *
 * Cost.  The kernel sorts the keys (tick, row) of a row band by class (a counting sort in LDS and the workspace) and
 * solves every class's chain by selection, with no sort inside the list: the next kept event is the smallest key at or
 * above (last kept tick + period_us), found by one pass over the list.  The chain costs the sum over the classes of
 * len x (kept + 1) key loads; a list of EC_REFRACTORY_LONG_LIST keys or more is walked by a whole wave, which divides its
 * share by 64.  Linear in the events for a stream spread over the sensor, quadratic only for one pixel that fires
 * thousands of times at intervals above the period.  No test feeds more than 4096 events to one class.  The events are
 * read 2 times per row band (ec_refractory_bands: count, scatter -- the chain reads keys, not events; denoise's third
 * read per band is its neighbour query) plus once to compact: 2 bands + 1.
 */
#ifndef EVENTCLIP_REFRACTORY_H
#define EVENTCLIP_REFRACTORY_H

#include "eventclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { EC_REFRACTORY_MAX_PERIOD_US = 1073741823,
       EC_REFRACTORY_MAX_GROUPS = 256,  /* the most workgroups of one launch: each owns one slot of the workspace */
       EC_REFRACTORY_LONG_LIST = 16     /* a class list of this many keys or more is walked by a whole wave, a shorter
                                           one by one lane (measured at 64 and 16: profiles/refractory.md) */ };

typedef struct {
    uint32_t kept;       /* counted and kept: written */
    uint32_t removed;    /* counted and inside a dead time */
    uint32_t passed;     /* not counted (p == 0 or outside the sensor): written */
} ec_refractory_stats;

typedef struct {
    int H, W;                 /* sensor resolution */
    uint32_t period_us;       /* the dead time, 1 .. EC_REFRACTORY_MAX_PERIOD_US */
    int per_polarity;         /* 0: one dead time per pixel; 1: one per (pixel, sign of p) */
    int max_sample_events;    /* upper bound of (end - begin) over sample_range, > 0: sizes the workspace */
    int64_t total_events;     /* sum of (end - begin) over sample_range if the caller knows it, else 0:
                                 only states the launch's algorithmic bytes to ec_profile_end */
} ec_refractory_params;

/*
 * events:       float32 [n_events_total, 4] rows (x, y, t, p), device, 16-byte aligned.
 * sample_range: int64 [B, 2] (begin, end) event-row indices per sample, device.  B == 0 is EC_OK and touches nothing.
 * events_out:   float32 [n_events_total, 4], device, 16-byte aligned (out); not events.
 * counts:       int64 [B], device (out).
 * keep:         optional uint8 [n_events_total], device (out).
 * stats:        optional ec_refractory_stats [B] (out).
 * workspace:    device, 16-byte aligned, at least ec_refractory_workspace_bytes(prm, B) bytes; its contents mean nothing
 *               before or after the call.
 * EC_ERR_INVALID: a null or misaligned buffer, events_out == events, period_us outside 1 .. EC_REFRACTORY_MAX_PERIOD_US,
 * per_polarity neither 0 nor 1, max_sample_events <= 0, a sensor of which the kernel's LDS band cannot hold one row
 * (ec_refractory_bands == 0).  EC_ERR_WORKSPACE: workspace_bytes too small.  A refused call writes nothing.
 */
EC_API int ec_refractory_events(const float *events, const int64_t *sample_range, int B, const ec_refractory_params *prm,
                                float *events_out, int64_t *counts, uint8_t *keep, EC_DEVICE ec_refractory_stats *stats,
                                void *workspace, size_t workspace_bytes, ec_stream_t stream);

/* the same on packed events (eventclip_hip.h, EC_PACKED_*), in and out, 8-byte aligned */
EC_API int ec_refractory_events_packed(const uint64_t *events, const int64_t *sample_range, int B,
                                       const ec_refractory_params *prm, uint64_t *events_out, int64_t *counts,
                                       uint8_t *keep, EC_DEVICE ec_refractory_stats *stats, void *workspace,
                                       size_t workspace_bytes, ec_stream_t stream);

/* host only: the bytes of workspace a launch of B samples with these parameters needs; 0 for parameters or a B the entry
 * points refuse */
EC_API size_t ec_refractory_workspace_bytes(const ec_refractory_params *prm, int B);

/* host only: the number of row bands the kernel cuts a sensor of (H, W) into (per_polarity: two classes a pixel, so half
 * the rows a band); 0 for what is refused */
EC_API int ec_refractory_bands(int H, int W, int per_polarity);

#ifdef __cplusplus
}
#endif

#endif /* EVENTCLIP_REFRACTORY_H */
