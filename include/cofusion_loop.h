/* cofusion_loop.h -- the loop-closure seam of the fern keyframe database (part of cofusion_hip.h, which includes it):
 * Ferns::findFrame for a camera that is NOT lost (Ferns.cpp:144-262).  The per-frame part is one small launch behind the search and
 * one wait on a 32-byte record in pinned memory; the candidate part (photometric check, accept rule, surface constraints) is one
 * launch that leaves its constraints in device buffers cf_deform_weights_device reads without a host round trip. */
#ifndef COFUSION_LOOP_H_
#define COFUSION_LOOP_H_
#ifndef COFUSION_HIP_H_
#error "include cofusion_hip.h"
#endif

/* Loop closure draws the samples i = 0, s, 2s, ... < n_ferns with s = n_ferns / 50 (Ferns.cpp:240) and every sample may add a constraint
 * and its pin: n_ferns >= 50 and ceil(n_ferns / s) <= CF_FERNS_MAX_SAMPLES (2 * 64 = CF_DEFORM_MAX_CONSTRAINTS).  500 ferns give 50
 * samples, 2048 give 52, 127 give 64, 99 are refused. */
#define CF_FERNS_MAX_SAMPLES 64
typedef struct {             /* written by ferns_gate_kernel into pinned memory, serial last */
    uint32_t serial;         /* number of the cf_ferns_gate_async call that wrote the record (1, 2, ...) */
    int32_t match_id;        /* the published match of the last search, -1: none */
    float dissimilarity;     /* of the match; FLT_MAX: none */
    float overlap;           /* blockHDAware (Ferns.cpp:321-336): f32(val) / f32(count) by IEEE division; NaN (0 / 0): no candidate; 0 without a match */
    int32_t good_q;          /* good codes of the current slot */
    int32_t keyframe_time;   /* srcTime of the match (0 without one) */
    int32_t count;           /* ferns good in the current slot AND in the match */
    int32_t keyframes;       /* keyframes the search scanned */
} cf_ferns_gate;             /* 32 bytes; a candidate: match_id >= 0 && overlap > 0.3f */
typedef struct {
    int32_t accepted;        /* icp_error < 3e-4 && icp_count > (lost ? 1400 : 2400) && photo_error < photo_threshold */
    int32_t n_constraints;   /* rows written to the constraint buffers, pins included (0 when rejected or lost) */
    int64_t photo_sum;       /* Ferns::photometricCheck: sum of |dR| + |dG| + |dB| over the correspondences, exact */
    int64_t photo_count;     /* ... and their number */
    double photo_error;      /* f64(sum) / f64(count); +inf with no correspondence */
    int32_t keyframe;        /* -1: no such keyframe (nothing else is a result then) */
    int32_t keyframe_time;   /* its srcTime: the time of the pins */
    float icp_error, icp_count;   /* as passed in */
} cf_ferns_closure;          /* 48 bytes */

/* blockHDAware of the current slot against the published match, ONE launch of one wave behind cf_ferns_search; enqueues, and records
 * an event behind the launch.  cf_ferns_gate_wait waits for THAT event (not for work enqueued later) and copies the record out. */
int cf_ferns_gate_async(cf_ferns *f);
int cf_ferns_gate_wait(cf_ferns *f, cf_ferns_gate *out);
/* The candidate part against keyframe `keyframe`, ONE launch of one workgroup, synchronous: (a) Ferns::photometricCheck of the current
 * slot with est_pose, in f64 from the f32 inputs exactly as cf_ferns_relocalise states it; (b) the accept rule from the tracker's
 * icp_error / icp_count handed in; (c) when accepted and not lost, the surface constraints of Ferns.cpp:240-255 in the interleaved
 * layout of a pinned closure: row 2j = (src curr_pose * v, dst est_pose * v, time `time`), row 2j + 1 = (src = dst = est_pose * v, time =
 * the keyframe's srcTime), j counting the valid samples (z > 0 && int(z * 1000.0f) < max_depth_mm) in order; each coordinate
 * ((m0 x + m1 y) + m2 z) + m3 in f32.  lost == 0 needs a fern count loop closure accepts (above), CF_EINVAL otherwise. */
int cf_ferns_constraints(cf_ferns *f, int keyframe, const float curr_pose[16], const float est_pose[16], float icp_error, float icp_count,
                         int lost, int time, cf_ferns_closure *out);
/* Ferns::findFrame whole for a slot that has been encoded, searched and gated (cf_ferns_gate_wait): no candidate -> result as
 * cf_ferns_relocalise leaves it and an all-zero closure with keyframe -1; a candidate -> the small tracker exactly as
 * cf_ferns_relocalise drives it, then the launch of cf_ferns_constraints.  result is filled as cf_ferns_relocalise fills it.  min_age
 * is the one the search ran with (kept for the symmetry of the two calls; the decision was made on the device). */
int cf_ferns_find_frame(cf_ferns *f, const float curr_pose[16], int time, int min_age, int lost, cf_ferns_result *result,
                        cf_ferns_closure *closure);
/* device buffers of the last accepted closure: src, dst f32 [CF_DEFORM_MAX_CONSTRAINTS][3], time f32 [CF_DEFORM_MAX_CONSTRAINTS]
 * (what cf_deform_weights_device takes); rows past n_constraints keep what an earlier closure left */
int cf_ferns_constraint_buffers(cf_ferns *f, float **src, float **dst, float **time);
/* the database's pose [capacity][16] and srcTime [capacity] arrays on the device, for cf_deform_apply_poses */
int cf_ferns_keyframe_buffers(cf_ferns *f, float **poses, int32_t **times);

/* ---- local (model-to-model) loop closure: the constraint stage (csrc/local_loop.hip, DESIGN.md 4.14 "The local half") ---- */
typedef struct cf_local_loop cf_local_loop;
typedef struct { float cov_thresh; int32_t icp_count_thresh; float icp_err_thresh; } cf_local_loop_thresholds;   /* 1e-5, 40000, 5e-5 */
typedef struct {             /* a tracker result handed in from the host instead of a cf_odom (tests) */
    float rot[9], trans[3];  /* the estimated pose, rotation row-major */
    float icp_error, icp_count;
    double lastA[36];
} cf_local_loop_track;
typedef struct {
    int32_t accepted;        /* every diagonal entry of inverse(lastA) <= cov_thresh (a NaN rejects) && icp_count > icp_count_thresh &&
                              * icp_error < icp_err_thresh */
    int32_t n_constraints;   /* rows written to the constraint buffers, pins included (0 when rejected) */
    double max_covariance;   /* the largest diagonal entry (a NaN if there is one) */
    float icp_error, icp_count;
    float est_pose[16];      /* the tracker's pose, row-major */
    uint32_t covered;        /* the word covered_dev points at when the kernel ran (0 without one) */
    uint32_t serial;         /* written last, behind a system fence */
} cf_local_loop_record;      /* 96 bytes */
/* (width / 20) * (height / 20) must lie in 1..768: one workgroup takes one sample per thread, and with pins the rows fill a graph object
 * of CF_DEFORM_MAX_CONSTRAINTS_SIZED */
int cf_local_loop_create(cf_ctx *ctx, cf_local_loop **out);
void cf_local_loop_destroy(cf_local_loop *l);
/* ONE launch of one workgroup on the context's MAIN stream -- the one the tracker's calls enqueue on, also from a thread bound to a lane
 * (cf_thread_lane): the maps handed in must have been written on that stream or be complete -- and an event behind it.  The tracker's result is read in device memory: from
 * `od` (its last tracking call, enqueued on the same stream) or, with od NULL, from `track` (copied up; test access); exactly one of
 * the two.  vertex_conf_dev: f32x4 [rows * cols], the ACTIVE splat vertexConf; old_time_dev: u16 [rows * cols], the inactive
 * prediction's time; covered_dev: nullable.  Accept rule: above.  Accepted: both maps are sampled at texel (20 x + 10, 20 y + 10),
 * x < cols / 20, y < rows / 20, visited column by column (x outer); a sample is valid when z > 0 && z < max_depth && old time > 0; row
 * k of the valid samples in that order is src = curr_pose * p, dst = est_pose * p (each coordinate ((m0 x + m1 y) + m2 z) + m3 in f32),
 * time = tick; with pin != 0 rows are interleaved as (constraint, pin): row 2k as before, row 2k + 1 = (dst, dst, the old time).  The
 * layout is the one cf_deform_weights_device reads. */
int cf_local_loop_constraints_async(cf_local_loop *l, const cf_odom *od, const cf_local_loop_track *track, const float *vertex_conf_dev,
                                    const uint16_t *old_time_dev, const uint32_t *covered_dev, const float curr_pose[16], int tick,
                                    float max_depth, int pin, const cf_local_loop_thresholds *th);
/* waits for THAT event (not for the stream) and copies the record out */
int cf_local_loop_wait(cf_local_loop *l, cf_local_loop_record *out);
/* device arrays the kernel writes: src, dst f32 [1536][3], time f32 [1536] */
int cf_local_loop_constraint_buffers(cf_local_loop *l, float **src, float **dst, float **time);
/* a fourth device array of the same launch: target_time f32 [768], the old time of constraint k (one per constraint, pin rows not
 * counted), written with or without pins -- what cf_deform_pick_relative keeps as dstTime */
int cf_local_loop_target_times(cf_local_loop *l, float **target_time);

#endif /* COFUSION_LOOP_H_ */
