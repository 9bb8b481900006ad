/*
 * eventclip_time_surface.h -- events -> time-surface frames: the part of libeventclip_hip.so's C ABI that ABI 609 added.
 *
 * The second standard image form of an event stream next to the polarity histogram of eventclip_hip.h: where the
 * histogram records how often a pixel fired, this records WHEN it last did, per pixel and polarity (the "timestamp
 * image" of the N-ImageNet benchmark; with an exponential decay, the "time surface").  The reference has no such
 * representation; the definition below is the specification, restated in float64 numpy by tests/time_surface_ref.py.
 *
 * Conventions (stream, return codes, ec_last_error, EC_DEVICE, the packed 8-byte event) are eventclip_hip.h's, and
 * EC_ABI_VERSION there covers this file.  Its own file so that eventclip_hip.h stays declaration for declaration what
 * ABI 608 stated; eventclip_amd/vis.py derives its bindings from this text the way eventclip_amd/_lib.py does from that one.
 *
 * One frame is built from the event rows [begin, end) of its frame_range on a sensor of (H, W):
 *   1. parse    x, y, p exactly as ec_events_to_frames does, for float rows and packed events: flip_x as W - 1 - x in
 *               float32 before the truncating cast, negate_p as p -> -p.  An event with p == 0 counts nowhere.  An event
 *               with x or y outside the sensor is counted in `dropped` and nowhere else.  All others are "counted".
 *   2. tick     integer microseconds: EC_PACKED_T(e) of a packed event; clip(rint((double)t * 1e6), 0, 2^30 - 1) of a
 *               float event (ec_pack_events' rule: a float batch and its packed form give the same bytes).  t is finite.
 *   3. t0, t1   the smallest and largest tick over the counted events of the frame; 0 and 0 when there is none.
 *   4. surface  L[y, x, c], c = 0 for p > 0 and 1 for p < 0: the largest tick over the counted events of that pixel and
 *               polarity -- the smallest with reverse_t.  It does not depend on the order of the events.  "Untouched"
 *               (no such event) is a state of its own, distinct from tick 0.
 *   5. age      a = t1 - L, with reverse_t a = L - t0; span = t1 - t0.  Integers.
 *   6. value    in float64, one rounding per operation, no contraction:
 *                 EC_DECAY_LINEAR  v = (double)(span - a) / (double)span, and 1 when span == 0    (timestamp image)
 *                 EC_DECAY_EXP     v = exp(-((double)a / tau_us)), the float64 exp                 (time surface)
 *               and v = 0 for an untouched L.
 *   7. colour   per channel k in float64: img = v_pos * red[k] + v_neg * blue[k] (two products, one sum, each rounded);
 *               with background_mask, w = min(v_pos + v_neg, 1) and img = img * w + 255 * (1 - w); the byte is
 *               (uint8)rint(img), ties to even.  No hot-pixel threshold and no division by a frame maximum.
 * The time flip of test-time augmentation (datasets/utils.py:26-35: reversed order, t' = t_last - t, p' = -p) is
 * reverse_t = 1 with negate_p = 1 on the stored rows and frame ranges taken on the reversed order: the latest t' is the
 * earliest t, and the age becomes t - t_min.  No event is rewritten.
 */
#ifndef EVENTCLIP_TIME_SURFACE_H
#define EVENTCLIP_TIME_SURFACE_H

#include "eventclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { EC_DECAY_LINEAR = 0, EC_DECAY_EXP = 1 };

typedef struct {
    uint32_t dropped;    /* events outside the sensor */
    uint32_t counted;    /* events with p != 0 inside the sensor */
    uint32_t t0, t1;     /* smallest / largest tick over the counted events, 0 and 0 without one */
} ec_surface_stats;

typedef struct {
    int H, W;                 /* sensor resolution */
    int decay;                /* EC_DECAY_LINEAR or EC_DECAY_EXP */
    double tau_us;            /* EC_DECAY_EXP: the time constant in microseconds, > 0 */
    int background_mask;      /* alpha-blend onto white */
    int flip_x, negate_p;     /* as in ec_events_params */
    int reverse_t;            /* the surface keeps the EARLIEST tick and ages from t0 */
    uint8_t red[3], blue[3];  /* colour of the positive / negative channel */
    int max_frame_events;     /* upper bound of events per frame, 0 = unknown.  A hint, as in ec_events_params; the
                                 kernel of ABI 609 reads a frame's events once per row band and makes no use of it */
    int64_t total_events;     /* sum of (end - begin) over frame_range if the caller knows it, else 0:
                                 only states the launch's algorithmic bytes to ec_profile_end */
} ec_time_surface_params;

/*
 * events:      float32 [n_events_total, 4] rows (x, y, t, p), device, 16-byte aligned.
 * frame_range: int64 [F, 2] (begin, end) event-row indices per frame, device.  F == 0 is EC_OK and touches nothing.
 * frames:      uint8 [F, H, W, 3], device (out).
 * last:        optional int32 [F, H, W, 2] (out): L, -1 where untouched.
 * stats:       optional ec_surface_stats [F] (out).
 * EC_ERR_INVALID: a null buffer, misaligned events, a W whose one row of state (8 bytes per pixel) does not fit the
 * kernel's LDS band, an unknown decay, tau_us <= 0 with EC_DECAY_EXP.
 */
EC_API int ec_events_to_time_surface(const float *events, const int64_t *frame_range, int F,
                                     const ec_time_surface_params *prm, uint8_t *frames, int32_t *last,
                                     EC_DEVICE ec_surface_stats *stats, ec_stream_t stream);

/* the same on packed events (eventclip_hip.h, EC_PACKED_*), 8-byte aligned */
EC_API int ec_events_to_time_surface_packed(const uint64_t *events, const int64_t *frame_range, int F,
                                            const ec_time_surface_params *prm, uint8_t *frames, int32_t *last,
                                            EC_DEVICE ec_surface_stats *stats, ec_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* EVENTCLIP_TIME_SURFACE_H */
