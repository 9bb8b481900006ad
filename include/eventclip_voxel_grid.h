/*
 * eventclip_voxel_grid.h -- events -> voxel-grid frames: the part of libeventclip_hip.so's C ABI that ABI 610 added.
 *
 * The third image form of an event stream, next to the polarity histogram of eventclip_hip.h (how often a pixel fired)
 * and the time surface of eventclip_time_surface.h (when it last fired): how the firing was DISTRIBUTED over the
 * frame's time span.  Every event spreads its signed unit over the two nearest of B temporal bins (the discretised
 * event volume of Zhu et al., the input of E2VID and most learned event pipelines).  With B = 3 the grid is a
 * 3-channel image whose colour shows the direction of motion.  The reference has no such representation; the
 * definition below is the specification, restated in int64 numpy by tests/voxel_grid_ref.py.
 *
 * Conventions (stream, return codes, ec_last_error, EC_DEVICE, the packed 8-byte event) are eventclip_hip.h's, and
 * EC_ABI_VERSION there covers this file.  Its own file so that eventclip_hip.h stays declaration for declaration what
 * ABI 608 stated; eventclip_amd/vis.py derives its bindings from this text the way eventclip_amd/_lib.py does from that one.
 *
 * One frame is built from the event rows [begin, end) of its frame_range on a sensor of (H, W), with B = bins:
 *   1. parse    x, y, p, tick, `dropped` and "counted" exactly as steps 1 - 2 of eventclip_time_surface.h state them:
 *               flip_x as W - 1 - x in float32 before the truncating cast, negate_p as p -> -p; an event with p == 0
 *               counts nowhere; an event outside the sensor counts in `dropped` and nowhere else; the tick is integer
 *               microseconds, EC_PACKED_T(e) of a packed event and clip(rint((double)t * 1e6), 0, 2^30 - 1) of a float
 *               event, so a float batch and its packed form give the same bytes.
 *   2. t0, t1   the smallest and largest tick over the counted events of the frame; 0 and 0 when there is none.
 *               span = t1 - t0.
 *   3. position d = tick - t0, with reverse_t d = t1 - tick.  u = floor(d * (B - 1) * 256 / span) in exact integer
 *               arithmetic (the product reaches 2^41: 64 bits), and u = 0 when span == 0.  b = u >> 8, f = u & 255.
 *   4. grid     G[y, x, b] += s * (256 - f) with s = +1 for p > 0 and -1 for p < 0, and, if f > 0,
 *               G[y, x, b + 1] += s * f.  G is int32 and every operation an integer addition: G does not depend on the
 *               order of the events.  An event at d == span has u = (B - 1) * 256, b = B - 1, f = 0: it writes the
 *               last bin only.  Precondition: at most 8 388 607 events per frame (256 n fits int32).
 *   5. peak     m = the maximum of |G| over the whole frame: all pixels, all bins.
 *   6. bytes    (B == 3 only) channel k of the image is bin k: byte = (255 * (G + m) + m) // (2 * m) in int64, and 128
 *               when m == 0: round-half-up of 127.5 + 127.5 * G / m in integers, no float stage, no tie window.  With
 *               background_mask a pixel whose three G are all 0 becomes (255, 255, 255).
 *   7. time flip  of test-time augmentation (datasets/utils.py:26-35): reverse_t = 1 with negate_p = 1 on the stored
 *               rows and frame ranges taken on the reversed order, as for the time surface.  d is recomputed from t1,
 *               not mirrored from u (the two differ by the floor): exactly what the rewritten stream would give.
 * There is no hot-pixel removal: the peak m, and with it the contrast of the whole frame, is sensitive to one hot
 * pixel.  (A clipping option is not part of ABI 610.)
 */
#ifndef EVENTCLIP_VOXEL_GRID_H
#define EVENTCLIP_VOXEL_GRID_H

#include "eventclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { EC_VOXEL_MIN_BINS = 2, EC_VOXEL_MAX_BINS = 8, EC_VOXEL_MAX_FRAME_EVENTS = 8388607 };

typedef struct {
    uint32_t dropped;    /* events outside the sensor */
    uint32_t counted;    /* events with p != 0 inside the sensor */
    uint32_t t0, t1;     /* smallest / largest tick over the counted events, 0 and 0 without one */
    uint32_t peak;       /* m of step 5 */
} ec_voxel_stats;

typedef struct {
    int H, W;                 /* sensor resolution */
    int bins;                 /* B, EC_VOXEL_MIN_BINS .. EC_VOXEL_MAX_BINS */
    int background_mask;      /* a pixel with G == 0 in every bin becomes white */
    int flip_x, negate_p;     /* as in ec_events_params */
    int reverse_t;            /* d = t1 - tick */
    int max_frame_events;     /* upper bound of events per frame, 0 = unknown; more than EC_VOXEL_MAX_FRAME_EVENTS is
                                 refused (step 4's precondition) */
    int64_t total_events;     /* sum of (end - begin) over frame_range if the caller knows it, else 0:
                                 only states the launch's algorithmic bytes to ec_profile_end */
} ec_voxel_grid_params;

/*
 * events:      float32 [n_events_total, 4] rows (x, y, t, p), device, 16-byte aligned.
 * frame_range: int64 [F, 2] (begin, end) event-row indices per frame, device.  F == 0 is EC_OK and touches nothing.
 * frames:      optional uint8 [F, H, W, 3], device (out); bins must be 3.
 * grid:        optional int32 [F, H, W, bins], device (out): G itself, for callers who feed other models.
 *              At least one of frames and grid.  A sensor of more than one row band (ec_voxel_grid_bands) whose frames
 *              are asked for without grid has its events binned twice; with grid the bytes are coloured from it.
 * stats:       optional ec_voxel_stats [F] (out).
 * EC_ERR_INVALID: null or misaligned events, no frame_range, neither frames nor grid, frames with bins != 3, bins
 * outside 2 .. 8, max_frame_events above EC_VOXEL_MAX_FRAME_EVENTS, a W whose one row of state (4 * bins bytes per
 * pixel) does not fit the kernel's LDS band.
 */
EC_API int ec_events_to_voxel_grid(const float *events, const int64_t *frame_range, int F,
                                   const ec_voxel_grid_params *prm, uint8_t *frames, int32_t *grid,
                                   EC_DEVICE ec_voxel_stats *stats, ec_stream_t stream);

/* the same on packed events (eventclip_hip.h, EC_PACKED_*), 8-byte aligned */
EC_API int ec_events_to_voxel_grid_packed(const uint64_t *events, const int64_t *frame_range, int F,
                                          const ec_voxel_grid_params *prm, uint8_t *frames, int32_t *grid,
                                          EC_DEVICE ec_voxel_stats *stats, ec_stream_t stream);

/* host only: the number of row bands the launch cuts a sensor of (H, W) with `bins` bins into; 0 for a shape or a
 * bin count the entry points refuse */
EC_API int ec_voxel_grid_bands(int H, int W, int bins);

#ifdef __cplusplus
}
#endif

#endif /* EVENTCLIP_VOXEL_GRID_H */
