/*
 * cofusion.h -- flat C wrapper of the C++ facade (co_fusion_amd/host/CoFusion.h) for language bindings
 * (ctypes in bench.py / tests).  Mirrors the calls GUI/MainController.cpp makes on the reference's CoFusion
 * object: construct (MainController.cpp:328-331), setters (:449-473), processFrame (:390), getters.
 * Poses are ROW-major float[16]; 0 = success, negative = error (message via cofusion_last_error()).
 */
#ifndef COFUSION_H_
#define COFUSION_H_
#include <stdint.h>
#include "cofusion_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cofusion_handle cofusion_handle;

typedef struct {
    int width, height;
    float fx, fy, cx, cy;
    int device, max_surfels, max_models; /* at most min(max_models, 255) models are active at a time (default 16): the context's tracker
                                          * staging and the segmentation's label dimension are sized by it; ids are 8 bits and 255 marks
                                          * a rejected superpixel (the reference's own limit, CoFusion.cpp:631-634).  Beyond the cap new
                                          * objects are not spawned (reported once on stderr) */
    float conf_global_init, conf_object_init, depth_cutoff, icp_weight, outlier_coefficient;
    int fast_odom, so3, frame_to_frame_rgb, pyramid, rgb_only;
    unsigned model_spawn_offset;
    int enable_multiple_models;
    int enable_pose_logging; /* CoFusion ctor argument enablePoseLogging (CoFusion.h:59); needed by cofusion_export_poses */
    int rank, world;         /* model-parallel operation over `world` processes / GPUs (default 0, 1); see cofusion_set_allreduce */
    int device_frames_complete; /* 1: buffers given to cofusion_process_frame_device are complete at call time (uploaded ahead), so the
                                 * new frame's depth filter may run beside the previous frame's fusion passes; 0 (default): they may be
                                 * produced by work queued on the context's stream and are consumed in stream order */
    int mid_frame_predict;      /* 1: also run the reference's prediction between tracking and fusion (CoFusion.cpp:346); its outputs are
                                 * overwritten by the end-of-frame prediction before the frame loop reads them (GUI only).  Default 0. */
    int shard_background;       /* model-parallel operation (world > 1): 1 = every rank keeps a replica of the background map and takes a
                                 * share of its index-map rasterisation (surfel range, MIN all-reduce of the z-keys) and of its ICP
                                 * reduction (image rows, SUM all-reduce of the accumulators after every launch of the Gauss-Newton
                                 * loop); needs cf_set_collective on the context (cofusion_context).  Default 0. */
    int enqueue_threads;        /* model-parallel operation (world > 1) only: helper threads that enqueue the per-model surfel passes (one
                                 * model's launch chain each) beside the calling thread; 0 = none (default).  A single process runs the
                                 * passes of all models as one chain of batched launches and ignores it.  Results do not depend on it. */
    int colocate_background;    /* model-parallel operation: 1 = object models round-robin over ALL ranks, the background shares rank 0
                                 * (BASELINE.json configs[3]: one object model per GPU); 0 (default) = the background alone on rank 0 */
    int reloc;                  /* CoFusion's `reloc` constructor argument (CoFusion.h:47): failure detection of the frame loop -- frames
                                 * with a background ICP error >= 1e-4 or a pose-covariance diagonal entry > 1e-4 are not fused, after
                                 * more than ten in a row the camera is lost (no fusion, the clock stops; CoFusion.cpp:225,301-338).
                                 * cofusion_is_lost reports it; cofusion_set_relocalisation adds the recovery.  Default 0. */
    int early_index_maps;       /* 1 (default): the index maps of the tracked models are rasterised with the poses the trackers left ON THE
                                 * DEVICE, behind the segmentation and before the frame's host wait (cf_models_preindex), so the GPU works
                                 * while the host reads poses and decisions; 0: with the rest of the surfel chain, after the wait.  Results are
                                 * identical either way. */
    int time_delta;             /* ElasticFusion's timeDelta: a surfel not seen for more than this many ticks is inactive (it is neither
                                 * tracked against nor fused into).  <= 0 (default): never, the open-loop operation of the reference
                                 * (MainController.cpp:328).  Loop closure (cofusion_set_loop_closure) wants a finite value, ElasticFusion
                                 * runs with 200: a camera that returns then fuses fresh surfels, which the closure moves onto the old ones. */
} cofusion_config;

void cofusion_default_config(cofusion_config *cfg);
int cofusion_create(const cofusion_config *cfg, cofusion_handle **out);
void cofusion_destroy(cofusion_handle *h);
const char *cofusion_last_error(void);
/* work is enqueued on this hipStream_t (NULL = legacy default stream) */
int cofusion_set_stream(cofusion_handle *h, void *hip_stream);
/* CoFusion::processFrame with host buffers (rgb 3 B/px, depth f32 metres, mask u8 or NULL, in_pose or NULL) */
int cofusion_process_frame(cofusion_handle *h, int64_t timestamp, const uint8_t *rgb, const float *depth, const uint8_t *mask,
                           const float *in_pose);
/* same with the frame already resident in HBM (depth f32, rgba u8x4) */
int cofusion_process_frame_device(cofusion_handle *h, int64_t timestamp, const float *depth_dev, const uint8_t *rgba_dev,
                                  const float *in_pose);
/* ... and its label mask as well (u8 [H*W], one value per object, 0 = background; 16-byte aligned): the mask branch of the
 * segmentation (the reference's pre-processed Mask#### input) runs as kernels beside the tracking, no pixel visits the host.  Results
 * are those of cofusion_process_frame with the same mask, bit for bit.  mask_dev follows the frame's rule (device_frames_complete: it
 * is complete at call time, or consumed in stream order).  mask_dev == NULL is cofusion_process_frame_device.  Refused for world > 1
 * (pass the mask from the host there). */
int cofusion_process_frame_device_masked(cofusion_handle *h, int64_t timestamp, const float *depth_dev, const uint8_t *rgba_dev,
                                         const uint8_t *mask_dev, const float *in_pose);
int cofusion_num_models(cofusion_handle *h);
int cofusion_tick(cofusion_handle *h);
/* CoFusion::getLost (CoFusion.h:183-185): 1 while the camera is lost (cofusion_config.reloc) */
int cofusion_is_lost(cofusion_handle *h);
/* The recovery half of `reloc` (ElasticFusion's fern keyframe relocaliser, CoFusion.cpp:349-367 and 321-337; cf_ferns in
 * cofusion_hip.h): with on = 1 every tracked frame offers the background's fill-in maps to a device-resident keyframe database (no host
 * wait), a lost camera asks it for a keyframe and, when one is accepted, continues from the recovered pose; the next frame's covariance
 * check ends the lost state.  Reference values: 500 ferns, fernThresh 0.3095, photoThresh 115, min age 300 ticks; n_ferns <= 0,
 * photo_threshold <= 0, min_age < 0 and capacity <= 0 select them (capacity: 1024 keyframes).  fern_threshold is taken as given: a
 * frame becomes a keyframe when its dissimilarity to every keyframe is greater, so a negative value keeps every frame.  The table is
 * generated from `seed`.  Calling it again replaces the database and resets the statistics.
 * Needs cfg.reloc = 1 and world == 1; refused for a sequence handle of a lock-step group.  Off (the default): the frame loop is
 * unchanged.  The frame width must be a multiple of 128, the height of 32. */
int cofusion_set_relocalisation(cofusion_handle *h, int on, int n_ferns, float fern_threshold, float photo_threshold, int min_age,
                                uint64_t seed, int capacity);
/* keyframes in the database, the keyframe the last relocalisation accepted (-1: none), lost -> tracked transitions so far, 1 when an
 * append was dropped because the database is full; each nullable.  Waits for the stream. */
int cofusion_reloc_stats(cofusion_handle *h, int *keyframes, int *last_closest, int *recoveries, int *database_full);
/* Loop closure of the background map from caller-supplied constraints (Deformation::addConstraint + constrain with
 * fernMatch): constraint i moves the surface point src[i] (seen at tick src_time[i]) to dst[i]; with pin != 0 every constraint adds
 * the pin dst[i] -> dst[i] at tick dst_time[i].  The deformation graph is sampled from the background map (every sample_rate-th
 * surfel; <= 0: 25000), optimised (the reference's thresholds), and -- when the optimisation is accepted -- applied to every surfel of
 * the map, with the reactivation stamp against the last frame's filtered depth at the current pose; the prediction is then redone as
 * after a relocalisation.  Object models and poses of past frames are left alone.  src, dst: host [n][3]; src_time, dst_time: host [n]
 * (dst_time may be NULL without pins); n (2 n with pins) <= 128.  result (nullable): 8 words -- optimised, accepted, failed,
 * iterations (int32), error and mean constraint error before and after (f32), as cf_deform_result.  nodes (nullable): the node count;
 * fewer than 5 nodes or a non-monotone sample: nothing is done and optimised = 0.  Needs a processed frame and world == 1; refused for
 * a sequence handle of a lock-step group.  Waits for the stream. */
int cofusion_deform_background(cofusion_handle *h, const float *src, const float *dst, const float *src_time, const float *dst_time, int n,
                               int pin, int sample_rate, void *result, int *nodes);
/* Global loop closure in the frame loop (the closeLoops branch of CoFusion.cpp:345-384): with it on, every tracked frame
 * is encoded, searched and gated against the keyframe database (one small launch and one host wait on a 32-byte record, skipped while
 * no keyframe can be older than min_age); a candidate (a match with overlap > 0.3) runs Ferns::findFrame; an accepted one deforms the
 * background map from the constraints the fern kernel left on the device, and an accepted graph moves the map (with the reactivation
 * stamp) and the keyframe poses, overrides the camera pose with the tracker's estimate and redoes the prediction.  It runs at the end of
 * the frame: the corrected map is first tracked against in the next frame.  sample_rate <= 0: 25000.  Needs cofusion_set_relocalisation
 * on (calling that again switches this off) with at least 50 ferns that give at most 64 samples of stride n / 50 (500: 50, 2048: 52,
 * 127: 64; 99 is refused); world == 1; refused for a sequence handle of a lock-step group.  Off (the default): the frame loop is
 * unchanged. */
int cofusion_set_loop_closure(cofusion_handle *h, int on, int sample_rate);
typedef struct {
    int32_t gated, candidates, fern_accepts;        /* frames gated, candidates, Ferns::findFrame accepts */
    int32_t optimised, accepted, failed;            /* deformation graphs */
    int32_t last_keyframe, last_keyframe_time, last_nodes, last_tick;   /* of the last fern accept (-1, -1, 0, -1: none): the keyframe, its srcTime,
                                                                          * the graph's nodes, the frame's tick */
    int32_t last_result[8];                         /* its cf_deform_result as cofusion_deform_background returns it */
} cofusion_loop_stats_t;
int cofusion_loop_stats(cofusion_handle *h, cofusion_loop_stats_t *out);
/* Local (model-to-model) loop closure in the frame loop (DESIGN.md 4.14 "The local half"; CoFusion.cpp:386-461, ElasticFusion's): with it
 * on, every tracked frame from tick time_delta + 1 on in which the fern seam closed no loop predicts the INACTIVE part of the background
 * map (surfels not seen for time_delta ticks) from the current pose, registers the ACTIVE prediction onto it with a second tracker
 * (rgb_only 0, icp_weight 10, so3 0) and runs one constraint launch behind it -- all enqueued unconditionally at the end of the frame --
 * and waits ONCE, on that launch's record.  The cost is therefore a second Gauss-Newton loop and a drained queue in every such frame.
 * Fewer covered inactive texels than min_inactive_pixels: nothing more (a stated departure; < 0: icp_count_thresh, 0: the reference's
 * behaviour).  A registration that passes the accept rule (every covariance diagonal <= cov_thresh, ICP count > icp_count_thresh, ICP
 * error < icp_err_thresh) and leaves >= 1 constraint deforms the map with a graph sampled at sample_rate in the graph's local mode (only
 * nodes younger than the last deformation move); an accepted graph moves the map, reactivates the old surfels in view of the estimated
 * pose (read from a depth image synthesized from the un-deformed map), moves the keyframe poses when there is a database, overrides the
 * camera pose and redoes the prediction.  Pins are added while no local closure has been accepted yet.  Values <= 0 of sample_rate,
 * icp_err_thresh, cov_thresh and < 0 of icp_count_thresh select the defaults 5000, 5e-5, 1e-5, 40000.  Needs time_delta > 0 and
 * (width / 20) * (height / 20) <= 768; needs no fern database; world == 1; refused for a sequence handle of a lock-step group.  Calling
 * it resets the statistics, deforms and last_deform_time included.  Off (the default): the frame loop is unchanged.  Relative
 * constraints: cofusion_set_relative_constraints.  Not built: the pose graph, object models. */
int cofusion_set_local_loop_closure(cofusion_handle *h, int on, int sample_rate, int icp_count_thresh, float icp_err_thresh, float cov_thresh,
                                    int min_inactive_pixels);
typedef struct {
    int32_t examined, skipped_by_gate, tracker_accepts;   /* frames examined, stopped by the pixel gate, accept rule passed with >= 1 constraint */
    int32_t optimised, accepted, failed;                  /* deformation graphs */
    int32_t last_nodes, last_constraints, last_pinned, last_tick;   /* of the last tracker accept: graph nodes, constraint rows (pins included),
                                                                      * whether they carried pins, the frame's tick (-1: none) */
    int32_t deforms, last_deform_time;                    /* accepted local closures, the tick of the last one (0: none) */
    uint32_t last_covered;                                /* covered inactive texels of the last examined frame */
    int32_t last_tracker_accepted;                        /* the accept rule in the last examined frame, and its three figures: */
    float last_icp_error, last_icp_count;
    double last_max_covariance;
    float last_est_pose[16];                              /* the second tracker's pose in the last examined frame, row-major */
    int32_t last_result[8];                               /* cf_deform_result of the last optimised graph */
} cofusion_local_loop_stats_t;                            /* 168 bytes */
int cofusion_local_loop_stats(cofusion_handle *h, cofusion_local_loop_stats_t *out);
/* Relative constraints (DESIGN.md 4.14 "Relative rows"; CoFusion.cpp:373, 445-458): what makes the two closures cooperate.  With it on,
 * every accepted LOCAL closure leaves a few of its constraints behind -- of its n constraints the indices 0, s, 2s, .. < n with
 * s = max(1, n / 3), as pairs (source moved by the accepted graph, target, srcTime, the old time of the target's texel) -- in a store
 * on the device: a ring of 128 pairs in which the newest overwrites the oldest.  Every later GLOBAL closure (the fern seam's and
 * cofusion_deform_background's) adds the stored pairs as rows 10 (phi(src) - phi(tgt)) to its system, so it cannot pull apart surfaces
 * a local closure has registered; its mean constraint error then divides by the number of ALL constraints, the stored pairs included
 * (the reference's nonRelativeConstraintError), which lowers what the 0.06 gate and the 3e-4 accept rule see.  The pairs are world
 * points and are not moved by later deformations, as in the reference.  Off (the default), or with an empty store: every closure is
 * what it is without this call, launch for launch.  Switching it off empties the store.  The first call allocates 38 MB.  world == 1;
 * refused for a sequence handle of a lock-step group. */
int cofusion_set_relative_constraints(cofusion_handle *h, int on);
/* caller-supplied pairs, appended to the store as cofusion_deform_background takes caller-supplied constraints: src, dst host [n][3],
 * src_time, dst_time host [n], n <= 128.  Needs cofusion_set_relative_constraints on. */
int cofusion_add_relative_constraints(cofusion_handle *h, const float *src, const float *dst, const float *src_time, const float *dst_time, int n);
/* the stored pairs in store order: out (nullable) [capacity][8] = source xyz, srcTime, target xyz, dstTime; *n = how many the store holds */
int cofusion_relative_constraints(cofusion_handle *h, float *out, int capacity, int *n);
typedef struct {
    int64_t appended, overwritten;       /* pairs ever appended; of those, lost to newer ones */
    int32_t stored;                      /* pairs the store holds */
    int32_t used_by_last_closure;        /* pairs in the system of the last global closure that reached the optimiser */
    int32_t last_picked;                 /* pairs the last accepted local closure left */
    int32_t pad;
} cofusion_relative_stats_t;             /* 32 bytes */
int cofusion_relative_stats(cofusion_handle *h, cofusion_relative_stats_t *out);
/* Test access: what the last accepted local closure worked on, readable until the next frame is processed.  Host outputs, each nullable:
 * rows (constraint rows, pins included), pinned (rows 2 k are constraints, 2 k + 1 their pins), last_deform_time (what its graph was
 * optimised with), src, dst [row_capacity][3], time [row_capacity], target_time [row_capacity] (the old time of every constraint: rows
 * or rows / 2 values), nodes (the graph's node count), node_pos [node_capacity][4], params [node_capacity][12] (the accepted ones).
 * *found = 0 and nothing written when no local closure has been accepted. */
int cofusion_local_closure_download(cofusion_handle *h, int *found, int *rows, int *pinned, int *last_deform_time, float *src, float *dst, float *time,
                                    float *target_time, int row_capacity, int *nodes, float *node_pos, float *params, int node_capacity);
/* Re-detection of inactive object models (the reference's CoFusion::redetectModels is an empty hook, CoFusion.cpp:599-602).
 * A model whose label gets no superpixels is deactivated; kept models (surfel count >= keep_min_surfels and confidence threshold >
 * keep_conf_threshold -- 4000 / 0.3, the reference's rule) wait in a list.  Off (the default) nothing reads that list: an object that
 * is labelled again is spawned as an empty map under a new id.  On: a frame whose segmentation reports a new label scores the most
 * recent max_candidates (1..16, default 8) kept models against it before anything is spawned, each at the pose it would have now HAD
 * IT NOT MOVED IN THE WORLD since it was deactivated (M_now = (G_d M_d^-1)^-1 G_now).  Per candidate (cf_redetect_score, cofusion_hip.h),
 * over its stable surfels projected into the frame:
 *     fit   = agree_on_label / (agree + seen_through)     surfels whose depth agrees within depth_tol AND whose pixel has the new label,
 *                                                         of those the frame could have seen (occluded ones are neutral)
 *     cover = covered / label_pixels                      distinct pixels of the new label the map explains
 * A candidate with fit >= min_fit and cover >= min_cover is eligible; the one with the largest agree_on_label (ties: the earlier in the
 * list) is reactivated -- old id, map, confidence threshold and pose log; no id is consumed; the frame's label image is rewritten to the
 * old id; with label masks the mask value is mapped to the old id.  In that frame its map is not touched (prediction only); the next
 * frame's tracker refines the pose, which has to pull it in from anywhere inside depth_tol (default 0.10 m, the tracker's own
 * correspondence gate).  Nobody eligible: the frame spawns as before.  Costs such a frame one more host wait.
 * Limits: an object that moved further than the gate while unseen is spawned anew; with a finite time window (not the default open
 * loop) a map reactivated after more than that many ticks is outside the window of the index pass; refused for world > 1.
 * Negative min_fit / min_cover / depth_tol / keep_* and max_candidates <= 0 select the defaults (0.5, 0.044, 0.10, 4000, 0.3, 8).  Works
 * on a sequence handle of a lock-step group.  Calling it resets the statistics. */
int cofusion_set_redetection(cofusion_handle *h, int on, float min_fit, float min_cover, float depth_tol, int max_candidates,
                             int keep_min_surfels, float keep_conf_threshold);
/* frames that scored candidates, reactivations, id of the last reactivated model (-1: none); each nullable */
int cofusion_redetect_stats(cofusion_handle *h, int *attempts, int *reactivations, int *last_id);
typedef struct {
    unsigned id;
    uint32_t projected, occluded, seen_through, agree, agree_on_label, covered;
    float fit, cover;
    int eligible;
} cofusion_redetect_candidate;
/* the candidates of the last attempt in list order (at most `capacity` are written, *n is their number), the pixels its new label had and
 * the position of the accepted candidate (-1: none); out, label_pixels, winner nullable */
int cofusion_redetect_last(cofusion_handle *h, cofusion_redetect_candidate *out, int capacity, int *n, uint32_t *label_pixels, int *winner);
/* The search behind the static hypothesis (DESIGN.md 4.13 "Search"): an object that comes back SOMEWHERE ELSE.  Needs
 * cofusion_set_redetection on (an error otherwise); off by default and then without any effect.  It runs only in a frame whose static
 * pass found nobody eligible -- a parked object is handled exactly as before.  The kept models whose colour histogram (512 bins: the top
 * three bits of R, G, B of their stable surfels) intersects that of the new label's pixels by at least min_colour (default 0.175, measured: DESIGN.md 4.13) are ranked by that
 * similarity; the first max_registered (1..16, default 2) are registered onto the label's pixels -- point-to-plane, twist about the
 * label's centroid, Tikhonov damped, at most `iterations` (default 10) steps with one host wait each, seeded with the static orientation
 * and the centroids aligned (cf_redetect_register, cofusion_hip.h) --, scored again at the registered pose and judged by min_fit /
 * min_cover as above; the winner is reactivated at the registered pose.  Envelope: any translation that keeps the object in view, turns
 * of up to about 10 degrees while unseen (degrading towards 20).  iterations / max_registered <= 0 and min_colour < 0 select the
 * defaults.  Refused for world > 1. */
int cofusion_set_redetection_search(cofusion_handle *h, int on, int iterations, float min_colour, int max_registered);
typedef struct {
    unsigned id;
    float colour;                 /* histogram intersection with the label's pixels, 0..1 */
    int registered, converged;    /* passed the colour gate and was within max_registered; its registration did not fail */
    int iterations;
    uint32_t first_inliers, last_inliers;
    float rms;                    /* of the point-to-plane residuals of the last step (m) */
    float moved;                  /* its front-facing centroid: registered against static pose (m) */
    uint32_t projected, occluded, seen_through, agree, agree_on_label, covered;   /* the score at the registered pose */
    float fit, cover;
    int eligible;
} cofusion_redetect_search_candidate;
/* the search of the last attempt, candidates in the order of cofusion_redetect_last (*n = 0 when that attempt did not search); winner:
 * the position of the reactivated candidate (-1: none); attempts: frames that searched so far; out, winner, attempts nullable */
int cofusion_redetect_search_last(cofusion_handle *h, cofusion_redetect_search_candidate *out, int capacity, int *n, int *winner, int *attempts);
int cofusion_num_inactive_models(cofusion_handle *h);
/* per model (list order, 0 = background): id, surfel count, pose T(model <- camera), confidence threshold */
int cofusion_model_info(cofusion_handle *h, int index, unsigned *id, unsigned *count, float pose[16], float *conf_threshold);
int cofusion_model_download(cofusion_handle *h, int index, float *surfels, uint32_t capacity, uint32_t *count);
int cofusion_model_icp_stats(cofusion_handle *h, int index, float *icp_error, float *icp_count);
/* the level-0 pixel rectangle [x0, y0, x1, y1] the model's last ICP iteration was restricted to (cf_track_stats::cull_box) */
int cofusion_model_cull_box(cofusion_handle *h, int index, int box[4]);
/* pixels the level-0 {ICP || residual} launch of the model's last tracking call visited for it (cf_odom_level0_visited) */
int cofusion_model_level0_visited(cofusion_handle *h, int index, uint64_t *icp_pixels, uint64_t *residual_pixels);
/* host copies of what the NEXT frame's tracking of this model reads (Model::initICP, Model.cpp:350-367): the predicted
 * vertex+conf / normal+radius maps (f32x4 [H*W]) and the predicted image (rgba8 [H*W]); any pointer may be NULL */
int cofusion_model_tracking_inputs(cofusion_handle *h, int index, float *vertex4, float *normal4, uint8_t *image_rgba);
/* device pointer of the full-resolution label mask (u8 [H*W]) */
const uint8_t *cofusion_mask_device(cofusion_handle *h);
/* the underlying C-ABI context (profiling hooks etc.) */
void *cofusion_context(cofusion_handle *h);
/* CRF / segmentation parameters (CoFusion.h:205-248 setters) */
int cofusion_set_crf(cofusion_handle *h, float unary_weight_error, float unary_k_error, float threshold_new, float weight_appearance,
                     float weight_smoothness, float sigma_rgb, float sigma_depth, float sigma_pos, float min_rel_size_new,
                     float max_rel_size_new, unsigned iterations);
/* The motion segmentation's tracking-independent half (superpixel sums of the frame and of the models' confidences, their statistics,
 * the appearance kernel) runs beside the tracking launches: on (default) / off.  The results are the same bit for bit; off is the
 * whole chain behind the tracker, for A/B measurements.  Sequences of a lock-step group and model-parallel runs always use the latter. */
int cofusion_set_seg_early(cofusion_handle *h, int on);

/* Several independent RGB-D sequences on ONE GPU in lock-step (throughput mode): the sequences share one context, and every set of
 * tracking launches (map preparation, SO(3) pre-alignment, the Gauss-Newton loop) carries the trackers of all of them, up to 16 per
 * launch -- the kernels of a 640x480 frame run at their launch floor, more trackers per launch is what fills the GPU.  Each sequence
 * keeps its own maps, models, segmentation and clock; its results are those of a cofusion_handle of its own, bit for bit.  One
 * configuration for all sequences (cfg->max_models is per sequence).  cofusion_group_sequence returns a BORROWED handle for the
 * per-sequence getters (model info, download, mask, export ...): do not pass it to cofusion_destroy / cofusion_process_frame*. */
typedef struct cofusion_group cofusion_group;
int cofusion_group_create(const cofusion_config *cfg, int sequences /* 1..16 */, cofusion_group **out);
void cofusion_group_destroy(cofusion_group *g);
int cofusion_group_size(cofusion_group *g);
cofusion_handle *cofusion_group_sequence(cofusion_group *g, int s);
int cofusion_group_set_stream(cofusion_group *g, void *hip_stream);
/* one frame of EVERY sequence: entry s of each array belongs to sequence s (timestamps / mask: nullable, mask entries nullable) */
int cofusion_group_process_frames(cofusion_group *g, const int64_t *timestamps, const uint8_t *const *rgb, const float *const *depth_m,
                                  const uint8_t *const *mask);
int cofusion_group_process_frames_device(cofusion_group *g, const int64_t *timestamps, const float *const *depth_dev,
                                         const uint8_t *const *rgba_dev);
/* ... with device masks (see cofusion_process_frame_device_masked): mask_dev nullable, its entries nullable -- a sequence without a
 * mask runs the motion segmentation as before.  The mask kernels of all masked sequences are ONE chain of three launches. */
int cofusion_group_process_frames_device_masked(cofusion_group *g, const int64_t *timestamps, const float *const *depth_dev,
                                                const uint8_t *const *rgba_dev, const uint8_t *const *mask_dev);

/* Model-parallel mode (cfg.world > 1, one process per GPU, every rank fed the same frames): the object models are placed
 * round-robin on ranks 1.., the background on rank 0; every rank runs the same frame loop and keeps data-less shadows of
 * the models it does not own.  All inter-rank traffic (poses after tracking, per-superpixel ICP / confidence sums for
 * the CRF, surfel counts at retirement) goes through this one callback: an in-place SUM all-reduce of `n` int64 values
 * over all ranks (e.g. ncclAllReduce / torch.distributed.all_reduce); return 0 on success.  Register before frame 1. */
typedef int (*cofusion_allreduce_i64_fn)(int64_t *buf, uint64_t n, void *user);
int cofusion_set_allreduce(cofusion_handle *h, cofusion_allreduce_i64_fn fn, void *user);
/* Optional second form of the same collective for buffers that live in HBM (the per-superpixel segmentation sums, 2*16*K
 * int64): an in-place SUM all-reduce of `n` int64 values at device address `dev_buf`, ENQUEUED on `hip_stream` (ncclAllReduce on
 * that stream, or on a stream ordered after it and before whatever is enqueued next) -- no host visit.  Without it such
 * buffers are staged through the host callback. */
typedef int (*cofusion_allreduce_dev_fn)(int64_t *dev_buf, uint64_t n, void *hip_stream, void *user);
int cofusion_set_allreduce_device(cofusion_handle *h, cofusion_allreduce_dev_fn fn, void *user);
/* RCCL inside the library: instead of the two callbacks above, give the instance its own ncclComm_t (created on the instance's
 * device, one process per GPU).  Rank 0 creates the 128-byte ncclUniqueId (cofusion_rccl_unique_id) and hands it to the other
 * ranks over any side channel (a file, MPI, a torch.distributed broadcast); then EVERY rank of cfg.world calls cofusion_init_rccl
 * (collective).  From then on the segmentation sums / tracked poses, the split reductions of a sharded background and the host-side
 * exchanges run ncclAllReduce in place on the context's stream -- no staging copies, no callback into the host language.
 * cofusion_broadcast sends a device buffer (a frame: depth + colour) from rank `root` to every rank with ncclBroadcast on the same
 * stream, so a following cofusion_process_frame_device consumes it in stream order (device_frames_complete = 0). */
int cofusion_rccl_unique_id(void *id128 /* 128 bytes */);
int cofusion_init_rccl(cofusion_handle *h, const void *id128);
int cofusion_broadcast(cofusion_handle *h, void *dev_buf, uint64_t bytes, int root);
/* 1 if the model at `index` lives on this rank, 0 if it is a shadow (count reads 0, download is empty) */
int cofusion_model_owned(cofusion_handle *h, int index);
/* diagnostics: accumulated host wall-clock (ms) per processFrame phase on the calling thread -- prepare, track, slic+sums,
 * unaries, crf, segmentation post-processing, model logic, fuse+clean, predict; returns the number of phases */
int cofusion_debug_phase_ms(double *out, int n, long *frames, int reset);
/* CoFusion::savePly / exportPoses (CoFusion.cpp:646-783): writes <prefix>cloud-<id>.ply / <prefix>poses-<id>.txt; returns the
 * number of files written or a negative error */
int cofusion_save_ply(cofusion_handle *h, const char *export_dir_prefix);
int cofusion_export_poses(cofusion_handle *h, const char *export_dir_prefix);
/* Mesh export (CoFusion::saveMesh over cf_mesh_*, include/cofusion_hip.h): writes <prefix>mesh-<id>.ply per owned
 * active model -- binary little-endian, vertices x y z nx ny nz red green blue, faces list uchar int vertex_indices --, a triangle mesh
 * of the model's confident surfels extracted on the device.  voxel 0: the model's mean confident radius.  Positions are mapped by
 * Tp = globalPose * modelPose^-1 as in savePly, normals by Tp's rotation block; normals point outside (the side the surface was seen
 * from).  Returns the number of files written or a negative error.  Off unless called; the first call creates the mesher (64 bytes per
 * voxel of cofusion_set_mesh_max_voxels, default 2^24), which the instance keeps. */
int cofusion_save_mesh(cofusion_handle *h, const char *export_dir_prefix, float voxel);
/* one model's mesh in the MODEL's frame (before Tp).  index >= 0: the active models in list order (0 = background); index < 0: the kept
 * inactive model number -1 - index (-1 is the first of cofusion_num_inactive_models).  Counts first: a call with vertices and triangles
 * NULL extracts the mesh, keeps it on the device and returns the counts; a call with arrays (capacities in records / triangles) copies
 * the kept mesh of the same index and voxel out, extracting first when none is kept or a frame was processed since.  transform
 * (nullable): the Tp cofusion_save_mesh applies.  A model this rank does not own: counts 0. */
int cofusion_model_mesh(cofusion_handle *h, int index, float voxel, uint32_t *n_vertices, uint32_t *n_triangles, cf_mesh_vertex *vertices,
                        uint32_t vertex_capacity, uint32_t *triangles, uint32_t triangle_capacity, float transform[16]);
int cofusion_set_mesh_max_voxels(cofusion_handle *h, uint64_t max_voxels);   /* 1 .. 2^28; drops a mesher of another size */
/* the PLY writer alone (host code): n_vertices records and n_triangles x 3 indices to `path` */
int cofusion_write_mesh_ply(const char *path, const cf_mesh_vertex *vertices, uint32_t n_vertices, const uint32_t *triangles, uint32_t n_triangles);
/* exportSegmentation (CoFusion.cpp:235-240): every segmented frame writes <prefix>Segmentation<tick>.png; NULL / "" switches it off */
int cofusion_set_export_segmentation(cofusion_handle *h, const char *export_dir_prefix);

/* Scene rendering (CoFusion::renderScene over cf_render, include/cofusion_hip.h): every active model drawn into one view as disc
 * splats, depth-tested against each other; the background in background_mode, the objects in object_mode (CF_RENDER_GREY ..
 * CF_RENDER_LABEL), objects placed by globalPose * modelPose^-1.  view NULL: the current camera at the frame intrinsics and size;
 * otherwise its pose (camera -> world), intrinsics, size and near / far are used.  flags: CF_RENDER_UNSTABLE | _WINDOW | _PHONG (the
 * view's own flags, tick and time_delta are replaced by `flags` and the instance's clock).  Semantics: DESIGN.md "Scene rendering".
 * Model-parallel / sharded-background operation: an error.
 * cofusion_render: host outputs, each nullable -- rgba u8x4, depth f32 (0 = empty), labels u8 (model id, 255 = empty), [h*w] each.
 * cofusion_render_device: the same into images the instance owns (device pointers valid until the next render of this instance). */
int cofusion_render(cofusion_handle *h, const cf_render_view *view, int background_mode, int object_mode, int flags, uint8_t *rgba,
                    float *depth, uint8_t *labels);
int cofusion_render_device(cofusion_handle *h, const cf_render_view *view, int background_mode, int object_mode, int flags,
                           const uint8_t **rgba, const float **depth, const uint8_t **labels);
/* the head-less view export (-el / -en / -ev): after every processed frame write <prefix>Labels<n>.png (background in colour, objects
 * in label colour), <prefix>Normals<n>.png (normals) and / or <prefix>Viewport<n>.png (colour) -- RGBA PNG from the current camera,
 * <n> the frame's number as in Segmentation<n>.png.  which: 1 labels | 2 normals | 4 viewport; 0 or an empty prefix: off. */
int cofusion_set_export_views(cofusion_handle *h, const char *export_dir_prefix, int which);
/* The per-frame exports above through the device PNG encoder (cf_png_encoder, include/cofusion_hip.h) and `workers` (1..8) writer
 * threads instead of a read-back and zlib on the calling thread: same file names, numbering and pixels.  Off by default.  The frame
 * loop waits for a file only when all `slots` (2..16) are busy -- nothing is dropped; a failed write is reported by the next
 * cofusion_process_frame* or by cofusion_export_flush.  on = 0 writes what is in flight and returns to the synchronous exports. */
int cofusion_set_export_async(cofusion_handle *h, int on, int workers, int slots);
/* returns when every file submitted so far is closed */
int cofusion_export_flush(cofusion_handle *h);
/* images and bytes written, submits that found every slot busy (each nullable).  device_ms / device_images: the encoding kernel's
 * device-event time over the images submitted since the last call while timing was on; timing: that diagnostics mode from here on.
 * Waits for the files in flight. */
int cofusion_export_stats(cofusion_handle *h, uint64_t *images, uint64_t *bytes, uint64_t *stalls, double *device_ms, uint64_t *device_images,
                          int timing);

/* .klg RGB-D logs (GUI/Tools/KlgLogReader.cpp:22-87): u16-mm depth raw or zlib, 8-bit x3 colour raw (JPEG frames are
 * rejected: no libjpeg in this build).  depth_m [H*W] metres, rgb [H*W*3]. */
typedef struct cofusion_klg_reader cofusion_klg_reader;
typedef struct cofusion_klg_writer cofusion_klg_writer;
int cofusion_klg_open(const char *file, int width, int height, int flip_colors, cofusion_klg_reader **out, int *num_frames);
int cofusion_klg_next(cofusion_klg_reader *r, int64_t *timestamp, float *depth_m, uint8_t *rgb);
/* 1: stop one frame early like the reference's KlgLogReader::hasMore() (`currentFrame + 1 < numFrames`); default 0 = play every frame */
int cofusion_klg_set_reference_compatible(cofusion_klg_reader *r, int on);
void cofusion_klg_close(cofusion_klg_reader *r);
int cofusion_klg_create(const char *file, int width, int height, int compress_depth, cofusion_klg_writer **out);
int cofusion_klg_write(cofusion_klg_writer *w, int64_t timestamp, const float *depth_m, const uint8_t *rgb);
int cofusion_klg_finish(cofusion_klg_writer *w);

/* .klg log player (host/KlgPlayer.h): worker threads read the log ahead (inflate, JPEG entropy decoding) into the
 * pinned slots of a cf_frame_decoder, the device finishes the frames, and they go into cofusion_process_frame_device -- the same
 * frames cofusion_klg_next delivers, byte for byte, without the decoding in front of every frame.  workers 1..16 (<= 0: 4).
 * Refused for world > 1 and for a sequence handle of a lock-step group.  The player must be closed before its instance is destroyed.
 * _next / _process return 0, 1 at the end of the log, -1 on error (a frame that cannot be decoded fails at its position: the frames
 * before it are played).  _next: the frame's device buffers (depth f32 [H*W] metres, rgba u8x4 [H*W]), complete or ordered on the
 * instance's stream as cofusion_config.device_frames_complete says, intact until the next call on this player.
 * _set_limits: reference_compatible as cofusion_klg_set_reference_compatible; frame_limit >= 0: play at most so many frames. */
typedef struct cofusion_klg_player cofusion_klg_player;
int cofusion_klg_player_open(cofusion_handle *h, const char *file, int flip_colors, int workers, cofusion_klg_player **out, int *num_frames);
int cofusion_klg_player_next(cofusion_klg_player *p, int64_t *timestamp, const float **depth_dev, const uint8_t **rgba_dev);
int cofusion_klg_player_process(cofusion_klg_player *p);
int cofusion_klg_player_rewind(cofusion_klg_player *p);
int cofusion_klg_player_set_limits(cofusion_klg_player *p, int reference_compatible, int frame_limit);
void cofusion_klg_player_close(cofusion_klg_player *p);

/* Test access to the two host halves of the player, usable without a GPU.
 * The JPEG decoder split at the coefficient boundary (host/Jpeg.cpp): _front writes the header and the quantised coefficients
 * (coef_blocks * 64 int16, CF_JPEG_MAX_BLOCKS(width, height) blocks always suffice) and returns 0, 1 when it refuses the stream (a
 * 16-bit quantisation table, a DC predictor outside int16: the player decodes such a frame on the host), -1 on a decoding error;
 * _finish_host is the host back end from that representation: rgb [H*W*3] in libjpeg's channel order. */
int cofusion_jpeg_front(const uint8_t *stream, uint64_t size, int width, int height, cf_jpeg_header *header, int16_t *coef,
                        uint64_t coef_blocks);
int cofusion_jpeg_finish_host(const cf_jpeg_header *header, const int16_t *coef, uint8_t *rgb);
/* The prefetcher alone over slots from malloc: _next delivers the next frame in log order (0; 1 at the end; -1 on error) and takes
 * back the slot of the previous one; slot (nullable) receives the frame's staging: depth u16 mm, and by *color_kind (CF_FRAME_COLOR_*)
 * header + coef or rgb. */
typedef struct cofusion_klg_prefetcher cofusion_klg_prefetcher;
int cofusion_klg_prefetch_open(const char *file, int width, int height, int workers, int slots, cofusion_klg_prefetcher **out,
                               int *num_frames);
int cofusion_klg_prefetch_next(cofusion_klg_prefetcher *p, int64_t *timestamp, int *color_kind, cf_frame_slot *slot);
int cofusion_klg_prefetch_rewind(cofusion_klg_prefetcher *p);
void cofusion_klg_prefetch_close(cofusion_klg_prefetcher *p);

/* Image-sequence datasets (host/ImageIO.h; GUI/Tools/ImageLogReader.cpp): a directory of colour .jpg/.png/.ppm, depth
 * .exr/.png and optional mask .png/.pgm files, <prefix><index, zero-padded to index_width><ext>.  Host-only code, usable without a GPU.
 * Empty depth_dir / mask_dir: the colour directory; directories that overlap without distinct prefixes take "Color", "Depth", "Mask".
 * Colour and depth counts must agree, and mask counts with them where masks exist.  start_index < 0: the first of 0, 1 that exists.
 * flip_colors 0 delivers the file's R, G, B (what the reference's reader hands on), 1 reverses them.  depth_scale turns 16-bit PNG depth
 * into metres with one f32 product (<= 0: the reference's 0.0006f; 0.001 for millimetre data, 0.0002 for TUM's 5000 per metre); EXR depth
 * is passed on as the file has it.  rate_hz <= 0: 24; timestamp = int64(f32(frame) * 1000.0f / rate_hz). */
typedef struct {
    const char *color_dir, *depth_dir, *mask_dir;
    const char *color_prefix, *depth_prefix, *mask_prefix;   /* each nullable = "" */
    int32_t index_width, start_index, flip_colors;
    float depth_scale, rate_hz;
    int32_t max_masks;   /* > 0: masks are read for the first so many frames only (the reference's maxMasks, which its own count rule
                          * keeps at the frame count); 0: for every frame that has a mask file */
} cofusion_image_options;
typedef struct { int32_t width, height, num_frames, start_index, has_masks, max_masks; } cofusion_image_info;
/* The serial reader: every file is read and decoded on the calling thread.  _next: depth_m [H*W], rgb [H*W*3], mask [H*W] (nullable);
 * *has_mask 0 for a frame without one (masks stop after max_masks frames).  0, 1 at the end, -1 on error (the message names the file). */
typedef struct cofusion_image_reader cofusion_image_reader;
int cofusion_image_reader_open(const cofusion_image_options *opt, cofusion_image_reader **out, cofusion_image_info *info);
int cofusion_image_reader_next(cofusion_image_reader *r, int64_t *timestamp, float *depth_m, uint8_t *rgb, uint8_t *mask, int *has_mask);
int cofusion_image_reader_rewind(cofusion_image_reader *r);
void cofusion_image_reader_close(cofusion_image_reader *r);
/* The image player (host/ImagePlayer.h), the counterpart of cofusion_klg_player_* for a directory: worker threads read
 * the files ahead (read, inflate, PNG unfilter, JPEG entropy decoding) into the pinned slots of a cf_frame_decoder with images enabled,
 * the device finishes the frames (csrc/image_decode.hip), and they go into cofusion_process_frame_device_masked where the frame has a
 * mask, into cofusion_process_frame_device otherwise -- the frames cofusion_image_reader_next delivers, byte for byte.  The set's frames
 * must have the instance's size.  workers 1..16 (<= 0: 4).  Refused for world > 1 and for a sequence handle of a lock-step group; close
 * the player before its instance.  _next / _process: 0, 1 at the end of the set, -1 on error (a frame that cannot be decoded fails at
 * its position, with a message that names the file; the frames before it are played).  _next: the frame's device buffers (depth f32
 * [H*W], rgba u8x4 [H*W], mask u8 [H*W] or NULL), complete or ordered on the instance's stream as device_frames_complete says, intact
 * until the next call on this player.  _set_limits: frame_limit >= 0 plays at most so many frames.  _times: seconds the workers spent
 * so far, all workers summed: reading files, inside zlib's inflate(), in the PNG unfilter loop, and in the rest of the parsers (chunk
 * walk, CRC-32, headers, copies of raw EXR blocks). */
typedef struct cofusion_image_player cofusion_image_player;
int cofusion_image_player_open(cofusion_handle *h, const cofusion_image_options *opt, int workers, cofusion_image_player **out,
                               cofusion_image_info *info);
int cofusion_image_player_next(cofusion_image_player *p, int64_t *timestamp, const float **depth_dev, const uint8_t **rgba_dev,
                               const uint8_t **mask_dev);
int cofusion_image_player_process(cofusion_image_player *p);
int cofusion_image_player_rewind(cofusion_image_player *p);
int cofusion_image_player_set_limits(cofusion_image_player *p, int frame_limit);
int cofusion_image_player_times(cofusion_image_player *p, double *read_s, double *inflate_s, double *unfilter_s, double *parse_s);
void cofusion_image_player_close(cofusion_image_player *p);
/* Test access to the host half of the player, usable without a GPU: the prefetcher over slots from malloc.  _next delivers the next
 * frame in order, FINISHED ON THE HOST by the host statements of the device's kernels, into the caller's buffers (depth_m [H*W], rgba
 * [H*W*4], mask [H*W] nullable; *has_mask): what the player's device frames must equal.  0, 1 at the end, -1 on error. */
typedef struct cofusion_image_prefetcher cofusion_image_prefetcher;
int cofusion_image_prefetch_open(const cofusion_image_options *opt, int workers, int slots, cofusion_image_prefetcher **out,
                                 cofusion_image_info *info);
int cofusion_image_prefetch_next(cofusion_image_prefetcher *p, int64_t *timestamp, float *depth_m, uint8_t *rgba, uint8_t *mask, int *has_mask);
int cofusion_image_prefetch_rewind(cofusion_image_prefetcher *p);
void cofusion_image_prefetch_close(cofusion_image_prefetcher *p);
/* The parsers alone.  role: 0 colour (8-bit grey / RGB / palette / RGBA), 1 depth (16-bit grey), 2 mask (8-bit grey).
 * _png_decode: non-interlaced PNG -> unfiltered scanlines in file layout (row stride 1 + bpp * width, 16-bit big-endian) in scan[cap],
 * the palette (768 bytes, nullable unless colour) beside it.  _exr_decode: single-part scanline OpenEXR (NONE / ZIPS / ZIP; HALF /
 * FLOAT) -> the inflated blocks in raw[cap] and their table (max_blocks >= height always suffices).  _ppm_decode: binary P6 -> where the
 * pixels start.  The _finish_host entries are the host statements of csrc/image_decode.hip: role 0 -> out = rgba u8x4, 1 -> f32
 * depth, 2 -> u8 mask.  0, or -1 with the reason in cofusion_last_error(). */
typedef struct { int32_t width, height, bit_depth, color_type, bpp, palette_entries; } cofusion_png_info;
typedef struct { int32_t width, height, compression, lines_per_block, blocks, line_bytes, chan_offset, chan_half; } cofusion_exr_info;
int cofusion_png_decode(const uint8_t *data, uint64_t size, int role, cofusion_png_info *info, uint8_t *scan, uint64_t cap, uint8_t *palette);
int cofusion_png_finish_host(const cofusion_png_info *info, int role, const uint8_t *scan, const uint8_t *palette, int flip_colors,
                             float depth_scale, void *out);
int cofusion_exr_decode(const uint8_t *data, uint64_t size, cofusion_exr_info *info, uint8_t *raw, uint64_t cap, cf_exr_block *blocks,
                        uint64_t max_blocks);
int cofusion_exr_finish_host(const cofusion_exr_info *info, const uint8_t *raw, const cf_exr_block *blocks, float *depth);
int cofusion_ppm_decode(const uint8_t *data, uint64_t size, int *width, int *height, uint64_t *pixel_offset);

#ifdef __cplusplus
}
#endif
#endif
