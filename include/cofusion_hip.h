/*
 * cofusion_hip.h -- C-ABI of the MI355X-native Co-Fusion hot path (libcofusion_hip.so).
 *
 * Drop-in boundary.  The reference's lower seam is the set of free
 * functions in Core/Cuda/cudafuncs.cuh:64-193 (called from Core/Utils/RGBDOdometry.cpp and
 * Core/Model/Model.cpp:341-343) plus the GLSL passes driven by Core/Model/Model.cpp and
 * Core/Model/ModelProjection.cpp.  Every entry point below names the reference interface it
 * replaces.  Signatures are plain C: device pointers, sizes, host PODs; no torch, no Eigen,
 * no OpenGL.  All functions return 0 on success or a negative CF_E* code; cf_last_error()
 * gives the message (the reference printf+exit(-1)s instead, Core/Cuda/convenience.cuh:74-83).
 *
 * Layouts
 *   depth           f32  [H*W] metres, 0 = invalid            (FrameData.depth, CV_32FC1)
 *   rgba            u8x4 [H*W] R,G,B,A                        (GL_RGBA texture of CoFusion.cpp:179)
 *   vertex4/normal4 f32x4 [H*W]                               (RGBA32F splat outputs)
 *   planar map      f32  [3*H*W]: x rows, y rows, z rows      (DeviceArray2D<float>(3*rows, cols))
 *   pose            f32[16] ROW-major T(model <- camera)      (Eigen::Matrix4f in the reference)
 *   SE3 sums        int64[32]: 27 upper-triangular products row_i*row_j (i<6, i<=j<7) in
 *                   Q31.32 fixed point, [27] = sum r^2 (Q31.32), [28] = inlier count.  The RGB step's sums use
 *                   CF_FIX_RGB_BITS(sigma) fraction bits (see below)
 *   surfel          12 f32 (48 B): [x y z conf][colour24 0 initTime lastTime][nx ny nz radius]
 *                   (Core/Shaders/Vertex.cpp:21-43)
 */
#ifndef COFUSION_HIP_H_
#define COFUSION_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_OK 0
#define CF_EINVAL (-1)
#define CF_EHIP (-2)
#define CF_ENOMEM (-3)
#define CF_ESTATE (-4)

#define CF_NUM_PYRS 3        /* RGBDOdometry::NUM_PYRS, RGBDOdometry.h:69 */
#define CF_SE3_WORDS 32
#define CF_SO3_WORDS 16
#define CF_FIX_ICP 32
/* Fraction bits of the RGB step's sums are NOT a constant: they follow the sigma handed to rgbStep --
 * 8 + 2*floor(log2 sigma) capped at 32, and 8 for sigma in {-1, < 2}.  Readers of cf_rgb_step's sums_host must use
 * CF_FIX_RGB_BITS(sigma); CF_FIX_RGB_MAX is only the cap (reached for sigma >= 4096). */
#define CF_FIX_RGB_MAX 32
static inline int CF_FIX_RGB_BITS(float sigma)
{
    union { float f; uint32_t u; } v;
    int F;
    if (sigma == -1.0f || !(sigma >= 2.0f)) return 8;
    v.f = sigma;
    F = 8 + 2 * ((int)((v.u >> 23) & 255u) - 127);
    return F > CF_FIX_RGB_MAX ? CF_FIX_RGB_MAX : F;
}
#define CF_FIX_SO3 12

typedef struct cf_ctx cf_ctx;
typedef struct cf_odom cf_odom;
typedef struct cf_model cf_model;

typedef struct { float fx, fy, cx, cy; } cf_cam; /* CameraModel, Core/Cuda/types.cuh:83-99 */

/* one surfel of a model map, byte-compatible with the reference's VBO vertex (Core/Shaders/Vertex.cpp:21-43):
 * what cf_model_download_map / cf_model_upload_map move */
typedef struct {
    float x, y, z, conf;
    float colour24, unused, init_time, last_time; /* colour: r<<16 | g<<8 | b stored as a float (color_encoding.glsl) */
    float nx, ny, nz, radius;
} cf_surfel;
#ifdef __cplusplus
static_assert(sizeof(cf_surfel) == 48, "surfel record is 3 x float4");
#else
_Static_assert(sizeof(cf_surfel) == 48, "surfel record is 3 x float4");
#endif

/* DataTerm, Core/Cuda/types.cuh:75-81 */
typedef struct {
    int16_t zero_x, zero_y;
    int16_t one_x, one_y;
    float diff;
    int32_t valid;
} cf_dataterm;

typedef struct {
    int width, height;
    float fx, fy, cx, cy;     /* Intrinsics singleton, Core/Utils/Intrinsics.h */
    int device;               /* HIP device ordinal */
    int max_models;           /* concurrently tracked models (background + objects) */
    int max_surfels;          /* per model; reference default 3072*3072 (Model.cpp:92-98) */
} cf_config;

/* ------------------------------------------------------------------ context ---- */
int cf_create(const cf_config *cfg, cf_ctx **out);
void cf_destroy(cf_ctx *ctx);
const char *cf_last_error(const cf_ctx *ctx);
/* all work is enqueued on one stream: by default a ctx-owned non-blocking stream; cf_set_stream
 * switches to a caller-owned hipStream_t (NULL = the legacy default stream), cf_use_own_stream back */
int cf_set_stream(cf_ctx *ctx, void *hip_stream);
int cf_use_own_stream(cf_ctx *ctx);
void *cf_get_stream(cf_ctx *ctx);
int cf_synchronize(cf_ctx *ctx);
/* Overlap independent work of one frame (e.g. the surfel passes of different models): cf_fork(lane) routes the following
 * calls to auxiliary stream `lane` (0..7), ordered after everything enqueued so far on the context's stream; cf_main
 * returns to that stream without waiting (the lanes keep running beside what follows); cf_join returns to it and orders
 * it after all lanes used since the last join.  Calls routed to a lane must not wait on the host. */
int cf_fork(cf_ctx *ctx, int lane);
int cf_main(cf_ctx *ctx);
int cf_join(cf_ctx *ctx);
/* the same for ONE lane: the stream waits for that lane only (the other lanes keep running beside what follows) */
int cf_join_lane(cf_ctx *ctx, int lane);
/* Enqueue from several host threads: the owning thread forks the lanes (cf_fork(lane) for each, then cf_main), helper threads
 * call cf_thread_lane(ctx, lane) and then issue the cf_model_* calls of ONE model each -- those go to the lane, the context's
 * current stream is untouched -- and unbind with lane < 0; the owning thread waits for the helpers and calls cf_join.  Only the
 * cf_model_* entry points honour the binding. */
int cf_thread_lane(cf_ctx *ctx, int lane);
/* cf_mark(slot 0..3) remembers the current point of the stream; cf_fork_after(lane, slot) routes the following calls to `lane`
 * ordered after that point only (slot < 0: after nothing): for work that does not depend on what the stream still has queued,
 * e.g. filtering the next frame while the previous frame's fusion passes run.  cf_join orders the stream after the lane. */
int cf_mark(cf_ctx *ctx, int slot);
int cf_event_wait_host(cf_ctx *ctx, int slot); /* block the host until the stream has passed cf_mark(slot) */
int cf_fork_after(cf_ctx *ctx, int lane, int slot);
/* device memory helpers for hosts that do not link HIP themselves */
int cf_malloc(cf_ctx *ctx, uint64_t bytes, void **dptr);
int cf_free(cf_ctx *ctx, void *dptr);
int cf_memcpy_h2d(cf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int cf_memcpy_d2h(cf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
/* pinned host memory + copies that are only ENQUEUED on the context's stream (the host side of the buffer must stay
 * untouched until the stream has passed the copy: cf_mark / cf_synchronize) */
int cf_malloc_host(cf_ctx *ctx, uint64_t bytes, void **hptr);
int cf_free_host(cf_ctx *ctx, void *hptr);
int cf_memcpy_h2d_async(cf_ctx *ctx, void *dst, const void *src_pinned, uint64_t bytes);
int cf_memcpy_d2h_async(cf_ctx *ctx, void *dst_pinned, const void *src, uint64_t bytes);
int cf_memcpy_d2d_async(cf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
/* FrameData.rgb (3 B/pixel, device copy) -> RGBA8 with alpha 255: the GL_RGBA upload of CoFusion.cpp:179 */
int cf_rgb_to_rgba(cf_ctx *ctx, const uint8_t *rgb_dev, int cols, int rows, uint8_t *rgba_dev);

/* --------------------------------------------- map preparation (cudafuncs.cuh) ---- */
/* createVMap  cudafuncs.cuh:125-130 */
int cf_create_vmap(cf_ctx *ctx, const float *depth, int cols, int rows, cf_cam intr, float depth_cutoff, float *vmap);
/* createNMap  cudafuncs.cuh:132-133 */
int cf_create_nmap(cf_ctx *ctx, const float *vmap, int cols, int rows, float *nmap);
/* copyMaps    cudafuncs.cuh:142-145 */
int cf_copy_maps(cf_ctx *ctx, const float *vertex4, const float *normal4, int cols, int rows, float *vmap, float *nmap);
/* resizeVMap / resizeNMap  cudafuncs.cuh:147-151 */
int cf_resize_map(cf_ctx *ctx, const float *in, int in_cols, int in_rows, float *out, int normalize);
/* tranformMaps cudafuncs.cuh:135-140 (in place) */
int cf_transform_maps(cf_ctx *ctx, float *vmap, float *nmap, int cols, int rows, const float R[9], const float t[3]);
/* verticesToDepth cudafuncs.cuh:156-158 */
int cf_vertices_to_depth(cf_ctx *ctx, const float *vertex4, int cols, int rows, float cutoff, float *depth);
/* pyrDownGaussF cudafuncs.cuh:174-175, pyrDownUcharGauss :177-178 */
int cf_pyrdown_gauss_f32(cf_ctx *ctx, const float *src, int src_cols, int src_rows, float *dst);
int cf_pyrdown_gauss_u8(cf_ctx *ctx, const uint8_t *src, int src_cols, int src_rows, uint8_t *dst);
/* imageBGRToIntensity cudafuncs.cuh:153-154 */
int cf_rgba_to_intensity(cf_ctx *ctx, const uint8_t *rgba, int cols, int rows, uint8_t *dst);
/* computeDerivativeImages cudafuncs.cuh:184-186 */
int cf_sobel(cf_ctx *ctx, const uint8_t *src, int cols, int rows, int16_t *dx, int16_t *dy);
/* projectToPointCloud cudafuncs.cuh:161-164 (intr already divided by 2^level) */
int cf_project_cloud(cf_ctx *ctx, const float *depth, int cols, int rows, cf_cam intr_level, float *cloud3);

/* ------------------------------------------------- reductions (cudafuncs.cuh) ---- */
/* icpStep cudafuncs.cuh:64-82.  Device maps in, host A[36] (row-major, symmetric filled),
 * b[6], residual[2] = {sum r^2, inliers} out (synchronous, like the reference).  sums_host
 * (nullable) additionally receives the exact int64[32] sums.  err_surface: device f32 [rows*cols]
 * or NULL (the cudaSurfaceObject_t of the reference). */
int cf_icp_step(cf_ctx *ctx, const float Rcurr[9], const float tcurr[3], const float *vmap_curr,
                const float *nmap_curr, const float Rprev_inv[9], const float tprev[3], cf_cam intr,
                const float *vmap_g_prev, const float *nmap_g_prev, float dist_thres, float angle_thres,
                int cols, int rows, float *A_host, float *b_host, float *residual_host, int64_t *sums_host,
                float *err_surface);
/* The same reduction over the row band [row_begin, row_end) only: a rank's share when ONE model's reduction is split
 * over several GPUs.  The int64 sums of the bands add up to the full-image sums exactly (integer arithmetic), so an
 * all-reduce(SUM) of sums_host over the ranks reproduces cf_icp_step bit for bit.  A/b/residual are the band's own. */
int cf_icp_step_band(cf_ctx *ctx, const float Rcurr[9], const float tcurr[3], const float *vmap_curr,
                     const float *nmap_curr, const float Rprev_inv[9], const float tprev[3], cf_cam intr,
                     const float *vmap_g_prev, const float *nmap_g_prev, float dist_thres, float angle_thres,
                     int cols, int rows, int row_begin, int row_end, float *A_host, float *b_host,
                     float *residual_host, int64_t *sums_host, float *err_surface);
/* computeRgbResidual cudafuncs.cuh:102-121 */
int cf_rgb_residual(cf_ctx *ctx, float min_scale, const int16_t *dIdx, const int16_t *dIdy, const float *last_depth,
                    const float *next_depth, const uint8_t *last_image, const uint8_t *next_image,
                    cf_dataterm *corres, float max_depth_delta, const float kt[3], const float krkinv[9],
                    int cols, int rows, int *sigma_sum_host, int *count_host);
/* rgbStep cudafuncs.cuh:84-97.  sigma: the correspondence count (RGBDOdometry.cpp:373-374), 1 or -1 (rgbOnly);
 * sums_host are fixed point with 8 + 2*floor(log2 sigma) fraction bits (max 32; 8 for sigma -1 or < 2) */
int cf_rgb_step(cf_ctx *ctx, const cf_dataterm *corres, float sigma, const float *cloud3, float fx, float fy,
                const int16_t *dIdx, const int16_t *dIdy, float sobel_scale, int cols, int rows, float *A_host,
                float *b_host, int64_t *sums_host);
/* so3Step cudafuncs.cuh:99-110 */
int cf_so3_step(cf_ctx *ctx, const uint8_t *last_image, const uint8_t *next_image, const float image_basis[9],
                const float kinv[9], const float krlr[9], int cols, int rows, float *A_host, float *b_host,
                float *residual_host, int64_t *sums_host);

/* ------------------------------- RGBDOdometry (Core/Utils/RGBDOdometry.h:42-60) ---- */
typedef struct {
    int rgb_only, pyramid, fast_odom, so3;
    float icp_weight;
} cf_track_opts;
typedef struct {
    float last_icp_error, last_icp_count, last_rgb_error, last_rgb_count, last_so3_error, last_so3_count;
    double lastA[36], lastb[6];
    int so3_iterations;
    int fault;              /* non-zero: a bounded device-side wait expired (cf_odom_fetch_result returns CF_ESTATE) */
    int cull_box[4];        /* cf_odom_set_culling: level-0 pixel rectangle [x0, y0, x1, y1] (inclusive, may exceed the image) the last ICP
                             * iteration was restricted to -- pixels outside cannot find a correspondence; x0 > x1: empty; the whole
                             * image when culling is off */
} cf_track_stats;

int cf_odom_create(cf_ctx *ctx, cf_odom **out);
void cf_odom_destroy(cf_odom *od);
/* initICPModel(predictedVertices, predictedNormals, depthCutoff, modelPose) RGBDOdometry.h:53 */
int cf_odom_init_icp_model(cf_odom *od, const float *pred_vertex4, const float *pred_normal4, const float pose[16]);
/* initRGBModel(rgb) :57 / initRGB(rgb) :55 / initFirstRGB(rgb) :59 -- rgba is a device RGBA8 image */
int cf_odom_init_rgb_model(cf_odom *od, const uint8_t *pred_rgba);
int cf_odom_init_rgb(cf_odom *od, const uint8_t *rgba);
int cf_odom_init_first_rgb(cf_odom *od, const uint8_t *rgba);
/* initICPModel + initRGBModel(pred_rgba[k]) + initRGB(frame_rgba) of `n` trackers at once: one launch per preparation
 * kernel with one grid row per tracker instead of seven launches per tracker (what a frame with several active models
 * needs before cf_odom_track_batch_async); identical results to the three single calls per tracker */
int cf_odom_init_models_batch(cf_ctx *ctx, cf_odom *const *ods, int n, const float *const *pred_vertex4,
                              const float *const *pred_normal4, const uint8_t *const *pred_rgba, const float *const *poses /* n x [16] */,
                              const uint8_t *frame_rgba);
/* ... with one frame image per tracker (frame_rgba[k] for ods[k]): the trackers of several sequences prepared by the same launches */
int cf_odom_init_models_batch_frames(cf_ctx *ctx, cf_odom *const *ods, int n, const float *const *pred_vertex4,
                                     const float *const *pred_normal4, const uint8_t *const *pred_rgba, const float *const *poses /* n x [16] */,
                                     const uint8_t *const *frame_rgba /* n */);
/* ... and with the choice between two sets of predictions per tracker made ON THE DEVICE: Model::initICP (Model.cpp:350-367) tracks against
 * the fill-in images when CoFusion::requiresFillIn (CoFusion.cpp:547-565) says so, and that answer comes from a count over the
 * previous frame's last prediction -- a host that asks for it (cf_model_requires_fill_in) has to wait for the previous frame to
 * drain before it can enqueue this one.  Here tracker k uses alt_*[k] instead of pred_*[k] when
 * (float)counts[0] / (float)counts[1] < ratio with counts = fill_counts[k] (device, from cf_model_fill_ratio_device; the very
 * expression of cf_model_requires_fill_in); fill_counts[k] == NULL (or the arrays NULL): no choice, pred_*[k]. */
int cf_odom_init_models_batch_select(cf_ctx *ctx, cf_odom *const *ods, int n, const float *const *pred_vertex4,
                                     const float *const *pred_normal4, const uint8_t *const *pred_rgba,
                                     const float *const *alt_vertex4, const float *const *alt_normal4, const uint8_t *const *alt_rgba,
                                     const uint32_t *const *fill_counts, float ratio, const float *const *poses /* n x [16] */,
                                     const uint8_t *const *frame_rgba /* n */);
/* initICP(depthPyramid, maskPyramid, depthCutoff) :48-49 (frame -> model); the mask pyramid is dead in the
 * reference (cudafuncs.cu:119) and therefore not part of the ABI */
int cf_odom_init_icp(cf_odom *od, const float *const depth_pyr[CF_NUM_PYRS], float depth_cutoff);
/* getIncrementalTransformation :62-64.  trans/rot host in-out.  The whole Gauss-Newton loop (SO3
 * pre-alignment, 4/5/10 pyramid schedule, f64 6x6 solve, SE3 update) runs device-resident; the host
 * waits once at the end.  icp_err_surface: device f32 [H*W] or NULL. */
int cf_odom_get_incremental_transformation(cf_odom *od, float trans[3], float rot[9], const cf_track_opts *opts,
                                           float *icp_err_surface, cf_track_stats *stats);
/* batched, asynchronous flavour used by the orchestrator: all `n` models advance through the
 * GN schedule in lock-step inside the same launches (grid.y = model).  Poses are read from /
 * written to the odom objects' device state; call cf_odom_fetch_result after cf_synchronize. */
int cf_odom_track_batch_async(cf_ctx *ctx, cf_odom *const *ods, int n, const float *const *poses_in /* n x [16] */,
                              const cf_track_opts *opts, float *const *icp_err_surfaces /* nullable entries */);
int cf_odom_fetch_result(cf_odom *od, float trans[3], float rot[9], cf_track_stats *stats);
/* RGBDOdometry::getCovariance (RGBDOdometry.h:60, RGBDOdometry.cpp:479: lastA.cast<double>().lu().inverse()) of a tracking call's
 * statistics: partial-pivot LU inverse of the 6x6 normal matrix, row-major f64 [36], on the host (the caller already holds lastA).
 * A singular lastA gives inf / NaN entries, as Eigen's does. */
int cf_odom_get_covariance(const cf_track_stats *stats, double cov[36]);

/* The per-iteration Gauss-Newton solve on its own (a stand-alone step like cf_icp_step / cf_rgb_step / cf_so3_step): the kernel the
 * tracking schedule launches behind every {ICP reduction, RGB step}, given sums and a state the caller wrote by hand.
 * cf_gn_state: the words of the device-resident tracker state the solve reads and writes (RGBDOdometry.cpp:371-467 keeps them in
 * host locals).  In and out are the same struct: a returned state can be handed straight to the next call. */
typedef struct {
    cf_cam intr;                      /* level-0 intrinsics: K of `next_level` is derived from them */
    int32_t width, height;
    int32_t icp, rgb, rgbOnly;
    float icpWeight;
    float Rprev[9], tprev[3], Rprev_inv[9], Rcurr[9], tcurr[3];
    double resultRt[16];
    float krkInv[9], kt[3];
    float lastRGBError;
    int32_t level_done, solves;
    float residual[2];
    float cull_z[2];
    float pose_inv[16];
    cf_track_stats stats;
} cf_gn_state;
typedef struct {
    int64_t icp_acc[64 * 32];         /* in: the grouped ICP sums [64 groups][32 words] (words 29 / 30 of the group totals: RGB count, sigma);
                                       * out: as the kernel left them */
    int64_t rgb_acc[64 * 32];         /* ... and the grouped RGB sums */
    cf_gn_state state;                /* in: the state before the solve; out: read back from the device */
    cf_gn_state twin;                 /* in: what the tracker's pinned host copy holds before; out: what it holds afterwards (the solve that ends
                                       * a schedule, next_level < 0, publishes its result there; configuration words are never written) */
    uint32_t hot[48];                 /* out: the derived block the per-iteration launches read pose and flags from */
} cf_gn_system;
/* One launch of `n` workgroups (1 <= n <= 16), system k in workgroup k, each on a temporary device state (screen-box culling off).
 * next_level: pyramid level of the NEXT iteration (2, 1, 0; -1: the schedule ends, the divergence guard and the inverse pose are
 * evaluated); last_of_level: the iteration ends its level (re-arms the RGB-only stop rule); icp_fix: fraction bits of the ICP sums
 * (CF_FIX_ICP), or -1 for the Gram form's per-word bits.  Synchronous.  n out of range or a null pointer: CF_EINVAL, nothing enqueued. */
int cf_gn_solve_step(cf_ctx *ctx, int n, cf_gn_system *systems, int next_level, int last_of_level, int icp_fix);
/* The first launch of a tracking call on its own: the SO(3) pre-alignment (RGBDOdometry.cpp:239-310) with the state hand-over around
 * it, as the schedule launches it -- 16 workgroups per system on one XCD, meeting at the context's sync blocks -- without the RGB
 * preparation workgroups that share the launch in production, screen-box culling off. */
typedef struct {
    const uint8_t *last_next_image;   /* device, level 2: (width >> 2) x (height >> 2) intensities (lastNextImage[2]); not read unless do_so3 */
    const uint8_t *next_image;        /* ... nextImage[2] */
    cf_gn_state state_in;             /* what the tracker's pinned host state holds: width, height and intr (level 0) are read, every word
                                       * is handed to the device state */
    cf_gn_state state_out;            /* out: the device state after the launch (pre-filled with a pattern before it) */
    uint32_t hot[48];                 /* out: the derived block of that state */
    uint64_t sync[418];               /* out: this system's sync block as the launch left it, every word (all zero between launches) */
} cf_so3_system;
/* One launch for `n` systems, 1 <= n <= min(16, max_models), system k on sync block k of the context.  do_so3 == 0: the launch of a
 * tracking call without pre-alignment (one workgroup per system: hand-over and seeding only).  first_level: the pyramid level (0..2)
 * krkInv / kt are prepared for.  Synchronous.  n or first_level out of range, a null pointer (the images when do_so3), a width that is
 * no multiple of 16 or a height that is no multiple of 4: CF_EINVAL, nothing enqueued. */
int cf_so3_prealign_step(cf_ctx *ctx, int n, cf_so3_system *systems, int do_so3, int first_level);
/* The record-slot path of the photometric term on its own (test-only, off the hot path): the two launches the schedule issues per
 * iteration of an rgb_only call under cf_set_gn_mode 1 / 2 -- (a) the compact residual pass, four pixels per thread, which packs the
 * valid correspondences of every workgroup into that workgroup's record slot (slot = 4 x cf_set_icp_launch threads pixels; record
 * x = pixel k of the next image, y = pixel g of the last image | (diff + 256) << 22) and adds count and sum (int)(diff^2) to words
 * 29 / 30 of the ICP accumulator; (b) the RGB step over the slots: rgb_slot_step_kernel (mode 1) or rgb_step_solve_kernel (mode 2,
 * whose last workgroup runs the solve) -- on temporary device states, accumulators, record buffers and sync blocks. */
typedef struct {
    /* in: the level's images on the device, cols x rows */
    const uint8_t *cand;              /* candidate mask of the frame preparation */
    const float *next_depth, *last_depth;
    const uint8_t *last_image, *next_image;
    const float *cloud;               /* 3 floats per pixel of the last image */
    const int16_t *dIdx, *dIdy;
    int32_t no_counts;                /* the residual pass leaves words 29 / 30 alone (RgbModelArgs::no_counts) */
    int32_t ranged;                   /* 0: every slot; 1: the slots of res_range only (a culled tracker) */
    uint32_t res_range[2];            /* ~(first 256-pixel chunk with a candidate), last such chunk + 1 (0: none), as the preparation leaves them */
    int32_t res_blocks;               /* residual workgroups of this system when ranged (<= 0 or more than the level's slots: one per slot) */
    uint64_t *records;                /* host [cols * rows]: in, what the record buffer holds before (a) (x in the low word); out, after (a) */
    uint32_t *slot_counts;            /* host [slots of the level]: in / out likewise */
    int64_t count_seed[64], sigma_seed[64];   /* in: words 29 / 30 of the 64 accumulator groups before (a) */
    int64_t count_total, sigma_total; /* out: the 64-group totals of words 29 / 30 after (a) */
    int64_t rgb_sums[32];             /* out, mode 1: the 64-group totals of the RGB accumulator after (b); mode 2: zero (the solve clears the sums) */
    cf_gn_state state;                /* in: the tracker state the launches read (rgb, rgbOnly, level_done, krkInv, kt; mode 2: all the solve reads);
                                       * out, mode 2: after the solve, as cf_gn_solve_step returns it */
    cf_gn_state twin;                 /* mode 2: the pinned host copy before / after, as cf_gn_system::twin */
    uint32_t hot[48];                 /* out: the derived hot block (mode 1: as the launches read it) */
} cf_rgb_system;
/* `n` systems (1 <= n <= 16) in one call.  cols, rows, max_depth_delta, sobel_scale and the level's fx, fy travel once per launch (the
 * trackers of a lock-step batch share a level); next_level / last_of_level: of the solve under mode 2, as cf_gn_solve_step.
 * Synchronous.  n out of range, cols % 4 != 0, cols * rows above the context's size, a null pointer, cf_set_gn_mode 0 or the
 * reference-order arithmetic (no record slots), mode 2 without round-robin workgroup placement: CF_EINVAL, nothing enqueued. */
int cf_rgb_records_step(cf_ctx *ctx, int n, cf_rgb_system *systems, int cols, int rows, float max_depth_delta, float sobel_scale,
                        float fx, float fy, int next_level, int last_of_level);
/* pixels the level-0 {ICP reduction || RGB residual} launch of the last fetched tracking call visited for this tracker: the 64-pixel
 * runs inside its final screen box and the record slots between its first and last RGB candidate (the whole image for a tracker
 * that is not culled) -- the physical byte count of a roofline figure, as opposed to SURVEY 8(d)'s every-pixel-to-every-tracker */
int cf_odom_level0_visited(cf_odom *od, uint64_t *icp_pixels, uint64_t *residual_pixels);
/* Workgroups the launcher gave this tracker in its LAST tracking call (host bookkeeping, readable as soon as the call returned), per
 * pyramid level.  icp_blocks[l] > 0: the ICP reduction of level l ran on the culled-slot mapping -- that many workgroups dealt the
 * 64-pixel runs of the tracker's screen box, sized from the box the previous fetched call ended with --; 0: one workgroup per run of the
 * whole image (no culling, no hint yet, Gram form, row band, or the level did not run).  The LAST level-0 iteration, which also writes
 * the error surfaces, is reported apart in *icp_blocks_err: it keeps the culled-slot mapping only when a culled tracker of the batch
 * has an error surface (written aside then); otherwise every tracker of that one launch runs on the whole-image mapping.
 * residual_blocks[l] > 0: the tracker's residual pass ran on that many workgroups over the record slots between its first and last
 * candidate, sized from the slots the previous fetched call needed; 0: one workgroup per slot of the level (no culling, no count from a
 * previous call, a count as large as the level, or no RGB term).  It is the figure of the level's LAST launch -- at level 0 the
 * error-surface iteration, whose residual pass is sized like every other's.  Any of the three pointers may be NULL. */
int cf_odom_last_launch_shape(cf_odom *od, int icp_blocks[3], int residual_blocks[3], int *icp_blocks_err);
/* share the frame-wide current vertex/normal pyramids between models (all models track the same frame,
 * cudafuncs.cu:119); pass NULL arrays to return to the odom-private maps written by cf_odom_init_icp */
/* Skip the model-map gathers of pixels that project into empty 4x4 blocks of the prediction (an occupancy bitmap written by
 * initICPModel) and, since round 5, every pixel outside the screen box of the prediction's frustum piece.  Results are unchanged; it
 * pays for models that cover a small part of the image (object models) and costs a dependent look-up for one that covers all of it
 * (background).  Default off.  Precondition of the screen box: the tracking call starts from the pose the model maps were prepared with
 * (cf_odom_init_icp_model's `pose` == the pose handed to cf_odom_track_batch_async / _get_incremental_transformation, bit for bit -- what
 * Model::performTracking does); a call that starts elsewhere is tracked WITHOUT the screen box (checked per call; the occupancy look-up
 * does not depend on it). */
int cf_odom_set_culling(cf_odom *od, int on);
/* Multi-GPU hooks.  cf_set_collective registers the caller's in-place all-reduce over its ranks (RCCL): op 0 = SUM of int64 words,
 * op 1 = MIN of unsigned 64-bit words; dev_buf is a device address, the call must only ENQUEUE on `hip_stream` (or order itself
 * after it and before later work on it); 0 = success.  cf_odom_set_band splits one model's reductions over the ranks by image
 * rows (level-0 rows, multiples of 4; add_counts = 1 on exactly one rank of the split): inside the device-resident loop the
 * collective sums that model's normal equations after every {ICP || residual} launch -- 32 words (256 bytes): the library folds the
 * rank's grouped partial sums first (round 6; 16 KB until then) --, so all ranks solve the same system. */
typedef int (*cf_collective_fn)(void *user, int op, void *dev_buf, uint64_t words, void *hip_stream);
int cf_set_collective(cf_ctx *ctx, cf_collective_fn fn, void *user);
int cf_odom_set_band(cf_odom *od, int row_begin, int row_end, int add_counts);
/* RCCL inside the library (one process per GPU; north_star: "RCCL all-reduce of the 6x6 system over xGMI").  cf_rccl_unique_id
 * wraps ncclGetUniqueId (rank 0 creates the 128-byte id, the caller hands it to the other ranks over any side channel);
 * cf_rccl_init creates the context's own ncclComm_t on the context's device (collective call: every rank of `world`) and registers
 * the library's own collective in place of cf_set_collective: the split reductions then run ncclAllReduce in place on the stream
 * their kernels are enqueued on -- no staging copy, no callback.  cf_rccl_allreduce: op 0 = SUM of int64 words, op 1 = MIN of
 * unsigned 64-bit words, in place, enqueued on hip_stream (NULL: the context's stream); cf_rccl_broadcast: `bytes` bytes from
 * rank `root` (a frame from the ingest GPU).  cf_destroy releases the communicator. */
#define CF_RCCL_ID_BYTES 128
int cf_rccl_unique_id(void *id128);
int cf_rccl_init(cf_ctx *ctx, const void *id128, int rank, int world);
int cf_rccl_allreduce(cf_ctx *ctx, void *dev_buf, uint64_t words, int op, void *hip_stream);
int cf_rccl_broadcast(cf_ctx *ctx, void *dev_buf, uint64_t bytes, int root, void *hip_stream);
int cf_rccl_info(const cf_ctx *ctx, int *rank, int *world, int *rccl_version);
int cf_rccl_destroy(cf_ctx *ctx);
int cf_odom_bind_frame_maps(cf_odom *od, const float *const vmaps[CF_NUM_PYRS], const float *const nmaps[CF_NUM_PYRS]);
/* ... or, when another tracker of the same context computed them with cf_odom_init_icp: share that tracker's current-frame pyramids
 * (and the per-run depth intervals the culled reduction uses) */
int cf_odom_share_frame_maps(cf_odom *od, cf_odom *owner);
/* test access to internal device pyramids: which 0..12 use the numbering of the oracle's orc_odom_buffer (0/1 current vertex / normal
 * maps, 2/3 model maps, 4/5 last / next depth, 6/7/8 last / next / lastNext intensity, 9/10 dIdx / dIdy, 11 cloud, 12 DataTerm records),
 * n = (width >> level) * (height >> level).  Reading which == 0 of a tracker's own maps hands out a writable pointer and therefore
 * drops the per-run depth intervals beside them (the next tracking call does not depth-cull).  What the culling decides with, read
 * only -- no tracker state changes:
 *   13  cand[level]    u8, n bytes: the candidate mask of the RGB residual pass (written by the first launch of a tracking call)
 *   14  zrange[level]  float2 (min, max), (n + 63) / 64 entries: depth interval of every 64-pixel run (cf_odom_init_icp)
 *   15  occ            u8, (width / 4) * (height / 4) entries, level must be 0: occupancy of the 4x4 blocks of the prediction
 *   16  aabb           six u32 order-preserving keys, level must be 0: bounding frustum of the prediction (x0, y0, z0 complemented,
 *                      x1, y1, z1; all zero = empty or culling off); latched and zeroed by the next tracking call */
int cf_odom_buffer(cf_odom *od, int which, int level, void **dptr, uint64_t *bytes);
/* initICP(predictedVertices, predictedNormals, cutoff), RGBDOdometry.cpp:120-141: the frame side of a model-to-model tracker from
 * device maps (f32x4 [rows * cols] each, e.g. the ACTIVE splat vertexConf / normalRad) instead of a depth pyramid: copyMaps into level
 * 0, resizeVMap / resizeNMap down the pyramid.  The vertices also become what the next cf_odom_init_rgb derives nextDepth from, so in
 * the reference's order (init_icp_model, init_rgb_model, init_icp_maps, init_rgb) nextDepth is the frame side's own depth, not the
 * model's.  A later cf_odom_init_icp replaces the frame side as before. */
int cf_odom_init_icp_maps(cf_odom *od, const float *vertex4, const float *normal4);
/* Model::generateCUDATextures depth half (Model.cpp:341-343): l1/l2 device outputs */
int cf_depth_pyramid(cf_ctx *ctx, const float *depth_filtered, int cols, int rows, float *l1, float *l2);

/* ------------------------------------------------ frame pre-processing + surfel Model ---- */
/* CoFusion::filterDepth + depth_bilateral_metric.frag (CoFusion.cpp:567-574): 13x13 bilateral, zero outside [0.3, maxD] */
int cf_bilateral(cf_ctx *ctx, const float *depth, int cols, int rows, float maxD, float *out);

/* Model (Core/Model/Model.h:117-235).  The pose lives with the caller (the CoFusion facade) and is passed
 * explicitly, ROW-major T(model <- camera).  Two surfel buffers are ping-ponged exactly like Model::vbos[2]. */
int cf_model_create(cf_ctx *ctx, int max_surfels, cf_model **out);
void cf_model_destroy(cf_model *m);
/* computeFeedbackBuffers + Model::initialise (CoFusion.cpp:157-169, Model.cpp:227-272); frame 1 only */
int cf_model_initialise(cf_model *m, const uint8_t *rgba, const float *depth_raw, const float *depth_filtered, int time,
                        float maxDepth);
/* Model::lastCount (Model.cpp:815) */
int cf_model_count(cf_model *m, uint32_t *count);
/* Model::predictIndices -> ModelProjection::predictIndices (ModelProjection.cpp:105-157) */
int cf_model_predict_indices(cf_model *m, const float pose[16], int time, float maxDepth, int timeDelta);
/* predictIndices in two halves for a surfel map sharded over GPUs: rasterise the surfels [surfel_begin, surfel_end) into
 * keys_dev (u64 [H*W], filled by the call; smaller key = nearer surfel, ties -> lower id, empty = all ones), MIN-all-reduce
 * the key maps over the ranks as unsigned 64-bit integers, then resolve the reduced map into the model's index textures. */
int cf_model_index_keys(cf_model *m, const float pose[16], int time, float maxDepth, int timeDelta, uint32_t surfel_begin,
                        uint32_t surfel_end, uint64_t *keys_dev);
int cf_model_index_resolve(cf_model *m, const float pose[16], uint64_t *keys_dev);
/* the three steps in one call for a REPLICATED map whose rasterisation is split over `nshards` ranks: this rank's range of the exact
 * surfel count, the registered collective (cf_set_collective, op 1) on the key map, resolve */
int cf_model_predict_indices_sharded(cf_model *m, const float pose[16], int time, float maxDepth, int timeDelta, int shard, int nshards);
/* Model::combinedPredict -> ModelProjection::combinedPredict (ModelProjection.cpp:192-273), ACTIVE prediction */
int cf_model_combined_predict(cf_model *m, const float pose[16], float maxDepth, float confThreshold, int time, int maxTime,
                              int timeDelta);
/* The INACTIVE prediction of local loop closure (ModelProjection::combinedPredict(..., INACTIVE) as CoFusion.cpp:390 calls it: time = 0,
 * maxTime = tick - timeDelta) into a second target set, the reference's oldFrameBuffer (cf_model_buffer 15..18, allocated by the first
 * call); the ACTIVE targets are not touched.  The resolve also leaves the number of covered texels (time > 0) in a device word
 * (cf_model_buffer 19).  Enqueued only. */
int cf_model_predict_inactive(cf_model *m, const float pose[16], float maxDepth, float confThreshold, int maxTime, int timeDelta);
/* ModelProjection::synthesizeDepth (splat.vert + depth_splat.frag: the acceptance rule of the colour splat, one output): corrected_pos.z
 * per texel into depth_out_dev (device, f32 [rows * cols]), 0 where nothing lands.  No other buffer of the model is written.  Enqueued only. */
int cf_model_synthesize_depth(cf_model *m, const float pose[16], float maxDepth, float confThreshold, int time, int maxTime, int timeDelta,
                              float *depth_out_dev);
/* optional: count the covered pixels of the latest splat prediction now and read them back asynchronously, so that the
 * next cf_model_requires_fill_in does not wait (call it after the frame's last cf_model_combined_predict) */
int cf_model_prefetch_fill_ratio(cf_model *m);
/* Model::performFillIn (Model.cpp:901-909) */
int cf_model_perform_fill_in(cf_model *m, const uint8_t *rgba, const float *depth_filtered, int passthrough_geom,
                             int passthrough_rgb);
/* CoFusion::requiresFillIn (CoFusion.cpp:547-565); out = 1 when fewer than `ratio` of the sampled pixels are set */
int cf_model_requires_fill_in(cf_model *m, float ratio, int *out);
/* device address of the two counts (covered, total) the last cf_model_prefetch_fill_ratio left, for cf_odom_init_models_batch_select;
 * *counts_dev = NULL when no prefetch is pending (the caller then asks cf_model_requires_fill_in).  Does not wait. */
int cf_model_fill_ratio_device(cf_model *m, const uint32_t **counts_dev);
/* Model::fuse (Model.cpp:408-563); weighting = Model::computeFusionWeight; maxDepth = min(depthCutoff, model maxDepth) */
int cf_model_fuse(cf_model *m, const float pose[16], int time, const uint8_t *rgba, const uint8_t *mask, const float *depth_raw,
                  const float *depth_filtered, float maxDepth, float weighting, int maskID);
/* Model::clean (Model.cpp:565-697); count_out = surfels written (the GL_TRANSFORM_FEEDBACK_PRIMITIVES_WRITTEN query) */
int cf_model_clean(cf_model *m, const float pose[16], int time, float confThreshold, float outlierCoeff, int timeDelta,
                   const float *depth_filtered, const uint8_t *mask, int maskID, uint32_t *count_out);
/* The second half of a frame for SEVERAL models in lock-step (CoFusion.cpp:316-330 and 346 / 533-545): what the reference runs as six
 * loops over the models -- predictIndices, fuse, predictIndices, clean for every model that fuses, combinedPredict(time, time) for all --
 * as ONE chain of launches whose workgroups are dealt to the models (the way the tracking launches carry all trackers): an object
 * model's share of a pass is a few dozen workgroups, and a chain of ~16 launch-floor kernels per model, one model after another,
 * was a third of a multi-object frame.  The items may belong to different sequences (own frame images, own clock).  Identical
 * results to the per-model calls in the same order; the surfel counts travel back asynchronously as with cf_model_clean. */
typedef struct {
    cf_model *model;
    const float *pose;                       /* [16] row-major T(model <- camera) */
    const uint8_t *rgba, *mask;              /* the model's frame: RGBA8, label mask (device) */
    const float *depth_raw, *depth_filtered;
    int do_fuse;                             /* 0: prediction only (CoFusion.cpp:463: !rgbOnly && trackingOk && !lost) */
    int time;                                /* the sequence's tick */
    float fuse_max_depth;                    /* min(depthCutoff, model maxDepth) (Model.cpp:443) */
    float weighting;                         /* Model::computeFusionWeight */
    int mask_id;
    float conf_threshold;
    /* fill_in != 0: the chain also does what cf_model_prefetch_fill_ratio + cf_model_perform_fill_in(rgba, depth_filtered,
     * passthrough_geom, passthrough_rgb) behind it would -- inside the last launch of the prediction, from the registers that hold the
     * texel, instead of two more launches that read it back.  Identical fill maps and counts; cf_model_requires_fill_in and
     * cf_model_fill_ratio_device answer as after the prefetch.  All zero: the chain as before. */
    int fill_in, passthrough_geom, passthrough_rgb;
} cf_model_pass;
int cf_models_frame_passes(cf_ctx *ctx, const cf_model_pass *items, int n, float depth_cutoff, float outlier_coeff, int time_delta);
/* The first index pass of that chain (Model::predictIndices before Model::fuse, CoFusion.cpp:316-318) for models that were tracked this
 * frame, enqueued BEFORE the host waits for the tracking results: the pose comes from the tracker's device state (inverted by a small
 * kernel), so the GPU rasterises the index maps while the host wakes up, reads poses and segmentation decisions and prepares the rest
 * of the chain (a 45-60 us hole in the queue per frame until round 5).  cf_models_frame_passes skips its first index pass for such a
 * model when the pose it is given equals the tracker's result bit for bit, and rasterises again otherwise (overridden pose).  A model
 * that is not fused afterwards (tracking lost, deactivated) just had its index map overwritten early: nothing reads it in between. */
typedef struct {
    cf_model *model;
    const cf_odom *odom;   /* the tracker whose result is the model's pose for this frame */
    int time;              /* the sequence's tick, as cf_model_pass::time */
} cf_model_preindex;
int cf_models_preindex(cf_ctx *ctx, const cf_model_preindex *items, int n, float depth_cutoff, int time_delta);
/* Model::downloadMap (Model.cpp:867-899): `count` surfels of 12 floats */
int cf_model_download_map(cf_model *m, float *host_surfels, uint32_t capacity, uint32_t *count);
int cf_model_upload_map(cf_model *m, const float *host_surfels, uint32_t count);
/* device views of the projection outputs.  which: 0 index(u32) 1 vertConf 2 colorTime 3 normRad (f32x4) | 4 splat image
 * (rgba8) 5 splat vertexConf 6 splat normalRad (f32x4) 7 splat time (u16) | 8 fill vertex 9 fill normal (f32x4)
 * 10 fill image (rgba8) | 11 surfels
 * Test access, read only -- no model state changes:
 *   12  the new unstable surfels the last cf_model_fuse / cf_models_frame_passes appended behind the map before its clean stage
 *       (f32x12 in column-major pixel order; bytes = 48 x their count; waits for the stream)
 *   13  the packed per-texel records cf_models_frame_passes leaves for its clean stage: vertConf | colorTime.z, colorTime.w, index (u32
 *       bits), filtered depth -- 32 bytes per texel (never written by the per-model calls)
 *   14  the z-keys of the rasterisers (u64 per texel): all ones between passes, every resolve leaves them so */
int cf_model_buffer(cf_model *m, int which, void **dptr, uint64_t *bytes);
/* Extent culling of the batched index passes (cf_models_preindex, cf_models_frame_passes).  Every model keeps the pixel rectangle its
 * index maps were last rasterised into; the resolve launches skip the 64-texel runs outside this pass's and the previous pass's
 * rectangle, which hold the empty value already (a model with more surfels than half the image has texels is left out: it covers the
 * screen).  Every buffer holds the same bytes as without it after every launch.
 * Default on; never under a collective (cf_set_collective, cf_rccl_init).  The per-model entry points always run unculled, and a batched
 * pass behind one of them -- or behind anything else that leaves the maps in a state the library has not seen -- handles every texel.
 * CF_NO_EXTENT_CULL in the environment switches it off for the process (diagnostic). */
int cf_set_extent_culling(cf_ctx *ctx, int on);
/* for a caller that writes a model's device buffers itself (through the pointers of cf_model_buffer): the next batched pass handles every texel */
int cf_model_extents_unknown(cf_model *m);
/* Re-detection of inactive models (CoFusion::redetectModels; the reference left the hook empty, CoFusion.cpp:599-602):
 * how well does a kept map, placed at a hypothesis pose, explain the pixels of a frame that carry a NEW label?  For every surfel i below
 * the model's count with confidence >= conf_threshold: projected as the index pass projects it (index_map.vert:38-63 without the time
 * window; rejects z < 0, z >= depth_cutoff, outside the image -- a rejected surfel counts nowhere) onto pixel q -> projected++; d =
 * depth[q]; !(d > 0) or d > depth_cutoff: nothing more; d < z - depth_tol: occluded++; d > z + depth_tol: seen_through++; otherwise
 * agree++ and, when label[q] == new_label, agree_on_label++ with pixel q marked.  covered = the number of DISTINCT marked pixels,
 * label_pixels = pixels with label == new_label.  All counts are exact integers, independent of execution order.
 * The image (depth f32 metres, 0 = invalid; label u8), its size and its camera are arguments: they need not be the context's.  One launch
 * scores all candidates (n <= 16), a second one finishes the counts; enqueued on the context's stream, then waited for (the counts
 * travel through pinned memory).  The models are only read. */
typedef struct { uint32_t projected, occluded, seen_through, agree, agree_on_label, covered; } cf_redetect_counts;
typedef struct {
    cf_model *model;
    float pose[16];          /* the hypothesis: row-major T(model <- camera), as cf_model_pass::pose */
    float conf_threshold;
} cf_redetect_candidate;
typedef struct {
    const float *depth;      /* device, [rows * cols] */
    const uint8_t *label;    /* device, [rows * cols] */
    int cols, rows;
    cf_cam cam;
    int new_label;
    float depth_cutoff, depth_tol;
} cf_redetect_frame;
int cf_redetect_score(cf_ctx *ctx, const cf_redetect_candidate *candidates, int n, const cf_redetect_frame *frame, cf_redetect_counts *counts /* [n] */,
                      uint32_t *label_pixels);
/* measurement (tools/redetect_bench.py): on = 1 puts a device event in front of and behind the launches of every cf_redetect_score from
 * here on (the counters' fill, the score and the finishing launch; not the read-back); last_ms (nullable): what the last call took */
int cf_redetect_timing(cf_ctx *ctx, int on, float *last_ms);
/* label_dev[i] == from -> to for i < n, 16 bytes per lane (label_dev: device, 16-byte aligned; from, to: 0..255); enqueued only */
int cf_relabel(cf_ctx *ctx, uint8_t *label_dev, uint64_t n, int from, int to);
/* Re-detection search (CoFusion::setRedetectionSearch, DESIGN.md 4.13 "Search"; kernels in csrc/redetect_search.hip, the numpy statement
 * in tests/redetect_search_ref.py): for an object that came back somewhere else.  Every device result is an integer -- a count, or a sum
 * of values rounded once to a fixed-point grid -- and so independent of launch shape and atomic order.  Each entry enqueues on the
 * context's stream and waits (the results travel through pinned memory); cf_redetect_timing covers their launches too.
 *
 * cf_redetect_frame_moments: over the pixels with label == new_label and 0 < depth <= depth_cutoff (depth_tol is not read):
 *   moments[0] their number, moments[1..3] the sum of rint(clamp(c, +-64) * 2^16) over the coordinates c of their vertices (createVMap's
 *   arithmetic: (d * (u - cx)) * (1 / fx), ...), hist[512] the histogram of (R >> 5) << 6 | (G >> 5) << 3 | (B >> 5) of rgba (device, u8 x 4). */
#define CF_REDETECT_BINS 512
int cf_redetect_frame_moments(cf_ctx *ctx, const cf_redetect_frame *frame, const uint8_t *rgba_dev, int64_t moments[4], uint32_t hist[CF_REDETECT_BINS]);
/* cf_redetect_model_moments: n <= 16 candidates in ONE launch (candidates[k].pose: the static hypothesis, as cf_redetect_score takes it).
 * Over the surfels with confidence >= conf_threshold: hist[k] the histogram of their decoded colours; over those of them whose normal,
 * rotated into the camera, has a POSITIVE dot product with dhat, the unit vector towards the label's centroid (the maps' normals point
 * away from the camera that saw them, as createNMap's do: such a surfel faces the camera): moments[k][0] their
 * number, moments[k][1..3] the sum of their MODEL-frame positions on the same grid. */
int cf_redetect_model_moments(cf_ctx *ctx, const cf_redetect_candidate *candidates, int n, const float dhat[3], int64_t *moments /* [n][4] */,
                              uint32_t *hist /* [n][CF_REDETECT_BINS] */);
/* cf_redetect_register_step: one candidate at one pose, cam_from_model = row-major T(camera <- model) -- the INVERSE of the convention of
 * cf_redetect_candidate::pose: the registration's state is the transform it applies.  A surfel with confidence >= conf_threshold is an
 * inlier when p = R p_m + t projects (as the score projects it) onto a pixel q with label[q] == new_label and 0 < depth[q] <=
 * depth_cutoff, |v - p| <= depth_tol for the frame's vertex v at q, and dot(n, p) > 0 for n = R n_m (it faces the camera).  Row J = [n, (p - centre) x n],
 * residual r = n . (v - p), entries clamped to +-4; sums[0..26]: the upper triangle of [J | r]^T [J | r] row by row without its last
 * entry, sums[27] = sum r^2, sums[28] the inliers, each product rounded once to 2^-32 (the layout and grid of the ICP sums). */
int cf_redetect_register_step(cf_ctx *ctx, cf_model *model, float conf_threshold, const float cam_from_model[16], const cf_redetect_frame *frame,
                              const float centre[3], int64_t sums[32]);
/* cf_redetect_register: the loop over that step, host f64 from the exact sums: (A + 1e-3 tr(A) / 6 I) xi = b by Cholesky, xi = (tau,
 * omega); R <- exp(omega) R, t <- exp(omega) (t - centre) + centre + tau (the twist is about `centre`, the label's centroid).  Ends when
 * |tau| < 1e-5 m and |omega| < 1e-5 rad or after max_iterations steps; FAILS (ok = 0) when a step has fewer than 6 inliers or fewer than
 * half of the first step's, or no positive definite system.  One host wait per step.  rms: sqrt(sum r^2 / inliers) of the last step
 * evaluated; cam_from_model: the pose after the last update (the seed when the first step fails). */
typedef struct {
    int ok, iterations;                       /* steps whose update was applied */
    uint32_t first_inliers, last_inliers;
    float rms;
    float cam_from_model[16];
} cf_redetect_registration;
int cf_redetect_register(cf_ctx *ctx, cf_model *model, float conf_threshold, const float seed_cam_from_model[16], const cf_redetect_frame *frame,
                         const float centre[3], int max_iterations, cf_redetect_registration *out);
/* Model::computeFusionWeight (Model.cpp:391-406); pure host math */
float cf_fusion_weight(const float pose[16], const float lastPose[16], float weightMultiplier);

/* ------------------------------------------------------------- motion segmentation ---- */
/* GPU side of Core/Segmentation (SLIC -> per-superpixel sums -> dense-CRF mean field -> up-sampling).
 * gSLICr / densecrf are third party and absent from the reference tree (Scripts/install.sh:84-85); they are
 * replaced by the published algorithms stated in oracle/orc_segment.c.  Superpixels are 16x16 on a regular
 * grid (Slic.cpp:33-43): K = (width/16)*(height/16) nodes. */
typedef struct cf_segmenter cf_segmenter;
int cf_seg_create(cf_ctx *ctx, cf_segmenter **out);
void cf_seg_destroy(cf_segmenter *s);
/* Slic::setInputImage + processFrame (Slic.cpp:48-81) */
int cf_seg_slic(cf_segmenter *s, const uint8_t *rgba);
/* DenseCRF2D inference of Segmentation.cpp:436-480: unary [K*L], Gaussian features [K*2] and bilateral
 * features [K*6] from the host, marginals Q [K*L] back to the host. */
int cf_seg_crf(cf_segmenter *s, const float *unary_host, int L, const float *feat_smooth_host, const float *feat_app_host,
               float w_smooth, float w_app, int iterations, float *Q_host);
/* The device-resident chain (what the facade uses).  cf_seg_sums: Slic::downsample / downsampleThresholded sums (Slic.h:48-120) as
 * exact Q32 fixed point, left on the device -- per superpixel the pixel count, count and sum of depth > 0.02, and per model the sums of
 * the ICP error surface and of the splat confidence (vertexConf.w).  cf_seg_infer (Segmentation.cpp:160-706): unary construction, the
 * mean field, arg-max, connected components (ConnectedLabels.hpp:50-172), the largest-component / size / border gates, bounding boxes,
 * depth statistics and Slic::upsample<unsigned char> (Slic.h:127-139) into full_dev, all as kernels; only the decisions come back
 * (cf_seg_fetch, the one host wait). */
typedef struct {
    float unaryWeightError, unaryKError, unaryThresholdNew;        /* GUI defaults 75, 0.0375, 5.5 (GUI.h:222-224) */
    float weightAppearance, weightSmoothness;                      /* 7, 2 */
    float scaleFeaturesRGB, scaleFeaturesDepth, scaleFeaturesPos;  /* 1/10, 1/0.9, 1/1.8 */
    float minRelSizeNew, maxRelSizeNew;                            /* 0.015, 0.4 */
    int crfIterations;                                             /* 10 */
} cf_seg_params;
#define CF_SEG_MAX_ENTRIES 256   /* model ids are 8 bits (CoFusion.cpp:631-634) and 255 marks a rejected superpixel: at most 255 models + the new label */
typedef struct {  /* SegmentationResult::ModelData (Segmentation.h:45-71) */
    uint32_t id, superPixelCount;
    float avgConfidence, depthMean, depthStd;
    int32_t top, right, bottom, left;
} cf_seg_model;
typedef struct {
    int32_t has_new_label, n_models;   /* n_models: rows of model[] (the new label's row is dropped when it got no superpixel) */
    float depth_range;
    cf_seg_model model[CF_SEG_MAX_ENTRIES];   /* rows [0, n_models) are valid */
} cf_seg_result;
int cf_seg_sums(cf_segmenter *s, const float *depth, int n_models, const float *const *icp_err, const float *const *vertconf4,
                int64_t **sums_dev, uint64_t *sums_words);
int cf_seg_infer(cf_segmenter *s, const cf_seg_params *params, const uint8_t *rgba, int n_models, const uint32_t *model_ids,
                 uint32_t next_model_id, int allow_new, uint8_t *full_dev);
int cf_seg_fetch(cf_segmenter *s, cf_seg_result *out, uint8_t *low_map_host);
/* The half of cf_seg_sums + cf_seg_infer that does not need the frame's tracking: the frame's own sums and the models' confidence sums
 * (vertconf4[m]: the previous frame's prediction), their means, the depth range, the average confidences, the appearance features and
 * the appearance kernel matrix.  Only enqueues, on the context's current stream, behind cf_seg_slic -- for a caller that puts it on a
 * lane beside the tracking launches.  The segmenter remembers depth, rgba, n_models, the vertconf4 pointers and params' three
 * scaleFeatures*; a following cf_seg_sums + cf_seg_infer with the same values enqueue the rest only (ICP-error sums, unaries, first
 * marginals, mean field, post-processing, up-sampling) -- the block cf_seg_sums hands out then holds the ICP-error sums alone, so no
 * collective can be placed there.  Calls that do not match run the whole chain (the results are those of the plain chain either way,
 * bit for bit); an early half that no inference follows is dropped by the segmenter's next cf_seg_early / cf_seg_sums. */
int cf_seg_early(cf_segmenter *s, const float *depth, const uint8_t *rgba, int n_models, const float *const *vertconf4,
                 const cf_seg_params *params);
/* cf_seg_sums + cf_seg_infer of SEVERAL segmenters of one context -- the sequences of a lock-step group (the reference runs one
 * performSegmentation per CoFusion instance, Segmentation.cpp:124-706) -- through shared launches: the chain of ~30 small kernels is
 * issued once per 8 segmenters (all of one image size, <= 16 labels each; otherwise one chain per segmenter) instead of once per
 * segmenter.  Per segmenter the results are those of the two single calls, bit for bit; each segmenter's decisions arrive with its
 * own cf_seg_fetch.  Single-process callers only: no collective can sit between the sums and the inference. */
typedef struct cf_seg_job {
    cf_segmenter *seg;
    const float *depth;                 /* cf_seg_sums' arguments */
    int32_t n_models;
    const float *const *icp_err;
    const float *const *vertconf4;
    const uint8_t *rgba;                /* cf_seg_infer's arguments */
    const uint32_t *model_ids;
    uint32_t next_model_id;
    int32_t allow_new;
    uint8_t *full_dev;
} cf_seg_job;
int cf_seg_run_batch(cf_ctx *ctx, const cf_seg_params *params, const cf_seg_job *jobs, int n_jobs);
/* Model-parallel callers (one process per GPU, each tracking some of the models): the block cf_seg_sums hands out ends in a tail of
 * max_models x 18 words.  cf_seg_publish_poses (between cf_seg_sums and the caller's in-place SUM all-reduce of the block) writes there, for
 * every model tracked by THIS process (trackers[m] != NULL), the tracked pose (row-major 4x4) + ICP error + ICP inlier count as f32
 * bit patterns, zeros for the others; the all-reduce then leaves every model's pose on every rank, and cf_seg_fetch_poses hands
 * them out after cf_seg_infer / cf_seg_fetch ([n_models][18] words) -- no separate pose exchange, no extra host wait. */
int cf_seg_publish_poses(cf_segmenter *s, int n_models, cf_odom *const *trackers);
int cf_seg_fetch_poses(cf_segmenter *s, int n_models, int64_t *words_host);
/* device view of the SLIC labels, int32 [H*W] */
int cf_seg_labels(cf_segmenter *s, void **dptr, uint64_t *bytes);
/* Test access, read only -- no segmenter state changes: device views of what the chain holds between its stages (K superpixels, n and
 * L = the models and labels of the last inference, Lcap = max(16, the context's max_models)).  Only hands out addresses: the caller
 * reads them in stream order (cf_memcpy_d2d_async on the context's stream).  which:
 *    0 spix_count  u32 [K]        1 depth_count  u32 [K]         2 depth_sum  i64 [K] (Q32)
 *    3 icp_sum     i64 [Lcap][K]  4 conf_sum     i64 [Lcap][K]   (Q32; model m's row at [m][.])
 *        0-4 are valid BETWEEN cf_seg_sums and cf_seg_infer: the unary kernel zeroes them for the next frame.  Behind a matching
 *        cf_seg_early only 0 and 3 are (the early half consumed and zeroed the others).
 *    5 low_mean    f32 [1 + 2n][K]: lowDepth | lowICP[n] (after the weak-confidence substitution) | lowConf[n] (non-finite entries zeroed)
 *    6 unary       f32 [K][L]     7 feat2        f32 [K][6]      8 avg_conf   f32 [n]      9 depth_range  f32 [1]
 *   10 low_map     u8 [K], the map behind the component analysis and the gates
 *   11 the marginals of the last inference (cf_seg_infer, cf_seg_run_batch or cf_seg_crf), f32 [K][L]: the one of the two buffers the
 *      mean field's last step wrote
 *        5-11 are valid behind cf_seg_infer / cf_seg_run_batch until the segmenter's next call (6, 7 and 11 also behind cf_seg_crf).
 *   12 centres     f32 [K][5] (x y r g b): the centres of SLIC's fifth update, the ones its sixth (last) assignment pass used
 *   13 slic_sums   u64 [K][6] (x y r g b count): the sums of the sixth assignment pass -- cf_seg_slic leaves them there, no update
 *      consumes them; column 5 is the labels' pixel count per superpixel
 *        12 and 13 are valid behind cf_seg_slic until the segmenter's next cf_seg_slic (no other call touches them).
 *   14 resample    i32 [K]: the label at superpixel k's resample pixel (what an empty superpixel reads, Slic.h:192-206)
 *        14 is valid behind cf_seg_sums, cf_seg_early and cf_seg_run_batch until the next of them (it follows the labels at that
 *        call; the inference reads it and leaves it). */
int cf_seg_buffer(cf_segmenter *s, int which, void **dptr, uint64_t *bytes);
/* The label-mask branch (Segmentation.cpp:59-119; the reference's "pre-processed segmentation" input, Mask####.png) as kernels: a mask
 * with one value per object arrives with the frame (u8 [H*W], device memory), `mapping` binds mask values to model ids (0 = unmapped)
 * and, when allow_new is set, the value of the raster-first pixel that is non-zero and unmapped becomes next_model_id -- at most one new
 * label per frame; pixels of other unmapped values get label 0.  cf_seg_masks only ENQUEUES (three launches on the context's current
 * stream, no host wait): the label image goes to full_dev, the decisions arrive through cf_seg_fetch -- has_new_label, n_models, the
 * models' rows in list order and the new label's row last (superPixelCount = pixels / 256, at least 1 for the new label; avgConfidence
 * 0.4; depthMean / depthStd: the sequential f32 sums of the RAW depth in raster order, bit for bit those of the reference's loops;
 * boxes and depth_range zero).  cf_seg_new_mask_value (after that fetch; CF_ESTATE before it) gives the mask value that was bound to
 * next_model_id, -1 when none was: the caller owns the mapping and enters it there.
 * mask_dev, depth_dev and full_dev are 16-byte aligned; full_dev is not mask_dev; 1 <= n_models <= 255 (CF_EINVAL otherwise).
 * cf_seg_masks_batch: the jobs of several segmenters of one context (the sequences of a lock-step group) in shared launches, the
 * chain issued once per 8 jobs; per segmenter the results of the single call.
 * cf_seg_create_masks: a segmenter that serves this branch ONLY (the other cf_seg_* calls return CF_EINVAL) and therefore has no
 * superpixel grid: any image size the context accepts, not only multiples of 16. */
typedef struct cf_seg_mask_job {
    cf_segmenter *seg;
    const uint8_t *mask_dev;            /* u8 [H*W] */
    const float *depth_dev;             /* the frame's raw depth, f32 [H*W] */
    int32_t n_models;
    const uint32_t *model_ids;          /* in list order (host) */
    uint32_t next_model_id;
    int32_t allow_new;
    const uint8_t *mapping;             /* [256] (host): mask value -> model id, 0 = unmapped; read before the call returns */
    uint8_t *full_dev;                  /* out: u8 [H*W] label image */
} cf_seg_mask_job;
int cf_seg_create_masks(cf_ctx *ctx, cf_segmenter **out);
int cf_seg_masks(const cf_seg_mask_job *job);
int cf_seg_masks_batch(cf_ctx *ctx, const cf_seg_mask_job *jobs, int n_jobs);
int cf_seg_new_mask_value(cf_segmenter *s, int *value);

/* data path between the RGB residual pass and the RGB step inside the device-resident Gauss-Newton loop.  1 (default): the
 * residual pass packs the valid correspondences of each workgroup into 8 B records, RGB step and 6x6 solve are launches of their
 * own (three launches per iteration); 2: the same records, the RGB step's workgroups of a tracker share one XCD and the last of
 * them to finish runs the solve (two launches per iteration; measured slower at 640x480, kept as an option); 0: the reference's
 * 16 B DataTerm record per pixel (diagnostic / comparison).  Results are bit-identical in all three. */
/* (mode 2 needs hardware workgroup b of a launch to run on XCD b mod 8; checked on the device once per context -- CF_ESTATE and the mode
 * unchanged where that does not hold.  Whatever the mode: a tracking call one of whose solves never ran is reported by
 * cf_odom_fetch_result as CF_ESTATE, not returned as a pose.) */
int cf_set_gn_mode(cf_ctx *ctx, int mode);
/* launch-shape tuning of the ICP reduction (GPUConfig.h:51-58 in the reference): threads per workgroup (64..1024, default 256) and
 * pixels per lane of trackers that reduce their whole image (1, 2, 4; 0 = default: two at pyramid level 0, one below).  The sums are
 * integers: every shape gives the same bits. */
int cf_set_icp_launch(cf_ctx *ctx, int threads, int pixels_per_thread);
/* Rounding specification of the ICP normal equations (icpStep's 27 products + residual, reduce.cu:334-394), a property of the context:
 *   CF_ICP_ARITH_PRODUCT (default): each product row_i*row_j is formed exactly in f64 and rounded once to 2^-CF_FIX_ICP;
 *   CF_ICP_ARITH_GRAM: each row ENTRY is rounded once to a fixed-point grid (2^-20 normal, 2^-17 moment, 2^-22 residual) and the
 *     integer products are summed exactly -- the Gram matrix of an integer matrix, contracted over the pixels on the matrix cores
 *     (signed 8-bit limbs, v_mfma_i32_32x32x32_i8).  Fewer vector instructions per pixel; both forms are exact integer sums
 *     (independent of launch shape and GPU count) and both have an oracle (oracle/orc.h: orc_set_icp_arith).
 * The 64-bit sums cf_icp_step returns are in the units of the chosen form.  Also: CF_ICP_ARITH=product|gram|reference in the environment. */
#define CF_ICP_ARITH_PRODUCT 0
#define CF_ICP_ARITH_GRAM 1
/*   CF_ICP_ARITH_REFERENCE: the reference's OWN order, for every reduction of the tracker (ICP, RGB, SO3), not only the ICP sums:
 *     thread-strided f32 partial sums, 32-lane shuffle-down tree, block tree and second-stage reduceSum of Core/Cuda/reduce.cu:90-185,
 *     396-417, 475-499 at the launch shapes of Core/Utils/GPUConfig.h:51-58, and the host loop of RGBDOdometry.cpp:217-477 around them
 *     (device synchronisation and a read-back per step, host LDL^T).  Not launch-shape independent -- that is the point: its poses,
 *     and with them whole trajectories and surfel counts, equal those of the reference's RGBDOdometry class bit for bit
 *     (tests/test_refpin_gpu.py).  A parity mode: synchronous, ~60 host round trips per tracker and frame; no culling, no split
 *     reductions; cf_icp_step / cf_rgb_step / cf_so3_step return A, b, residual of the f32 trees (sums_host is zero-filled). */
#define CF_ICP_ARITH_REFERENCE 2
int cf_set_icp_arith(cf_ctx *ctx, int mode);
int cf_get_icp_arith(cf_ctx *ctx);

/* ---------------------------------------------------------------- scene rendering ---- */
/* Draws the surfel maps of several models (background and objects) into one view as disc splats, depth-tested against each
 * other: what the reference's viewer shows (Model.cpp:274-314, draw_global_surface.*).  Coverage, depth test and colours are
 * specified exactly in DESIGN.md ("Scene rendering"); in short:
 *   - a surfel is drawn when conf > conf_threshold, or always with CF_RENDER_UNSTABLE;
 *   - it covers pixel (px, py) when the ray through (px + 0.5, py + 0.5) meets its plane within `radius` of its centre at view
 *     depth near < z < far; a surfel with a corner of its quad (half-diagonal radius * sqrt 2) at z <= near is skipped;
 *   - the nearest z wins; ties go to the earlier item, then to the lower surfel index.
 * A cf_renderer object owns every buffer of a call (keys, rays, overflow list) for views up to max_w x max_h; nothing is allocated
 * per call.  cf_render only ENQUEUES, on the context's stream, ordered after every lane of the frame (cf_fork); it reads the
 * surfel buffers and writes the caller's output images, nothing else. */
typedef struct cf_renderer cf_renderer;   /* the object; cf_render is the call */
#define CF_RENDER_MAX_ITEMS 256
#define CF_RENDER_MAX_COLOUR 8      /* RGBA outputs per call */
/* view flags */
#define CF_RENDER_UNSTABLE 1        /* draw surfels at or below their threshold too (in the times colour) */
#define CF_RENDER_WINDOW 2          /* dim surfels with tick - last_time > time_delta by 0.25 */
#define CF_RENDER_PHONG 4           /* ambient 0.3 + diffuse + specular (exponent 32), light at the camera centre */
/* colour modes */
#define CF_RENDER_GREY 0
#define CF_RENDER_NORMALS 1         /* world-frame normal */
#define CF_RENDER_COLOUR 2
#define CF_RENDER_TIMES 3
#define CF_RENDER_LABEL 4           /* label palette entry of the item's model id (cf_render_palette) */
#define CF_RENDER_ITEM_MODE (-1)    /* cf_render_output.mode: each item's own colour_mode */
/* output kinds */
#define CF_RENDER_RGBA 0            /* u8x4 [height*width], alpha 255 where covered, all zero where empty */
#define CF_RENDER_DEPTH 1           /* f32 [height*width] view depth, 0 where empty */
#define CF_RENDER_LABELS 2          /* u8 [height*width] model id of the winning item, 255 where empty */
typedef struct {
    float pose[16];                 /* camera -> world, row-major, rigid (its inverse is taken as [R^T | -R^T t]) */
    float fx, fy, cx, cy;
    int width, height;              /* at most the render object's max_w x max_h */
    float near_z, far_z;            /* 0: the defaults 0.1 / 1000 */
    int flags;                      /* CF_RENDER_UNSTABLE | CF_RENDER_WINDOW | CF_RENDER_PHONG */
    int tick, time_delta;           /* the sequence's clock (times colour, window) */
} cf_render_view;
typedef struct {
    const float *surfels;           /* device, `count` surfels of 12 f32 (cf_model_buffer 11) */
    uint32_t count;
    float pose[16];                 /* model -> world, row-major: globalPose * modelPose^-1 (identity for the background) */
    float conf_threshold;
    int model_id;                   /* 0..254 */
    int colour_mode;                /* CF_RENDER_GREY .. CF_RENDER_LABEL */
} cf_render_item;
typedef struct {
    void *dst;                      /* device, dense [height*width] elements of the kind */
    int kind;                       /* CF_RENDER_RGBA / _DEPTH / _LABELS */
    int mode;                       /* RGBA only: one colour mode for every item, or CF_RENDER_ITEM_MODE */
} cf_render_output;
int cf_render_create(cf_ctx *ctx, int max_w, int max_h, cf_renderer **out);
void cf_render_destroy(cf_renderer *r);
/* Items are drawn in list order (draw index = surfel index + the counts of the items before it).  At most CF_RENDER_MAX_ITEMS
 * items, 2^32 - 1 surfels in all, CF_RENDER_MAX_COLOUR RGBA outputs, one depth and one label output. */
int cf_render(cf_renderer *r, const cf_render_view *view, const cf_render_item *items, int n_items, const cf_render_output *outputs,
              int n_outputs);
/* the label palette: RGB8 [256][3]; entry 255 means "none" (black) */
int cf_render_palette(uint8_t *rgb768);

/* ------------------------------------------------ keyframe relocalisation (Core/Ferns.h) ---- */
/* ElasticFusion's random-fern keyframe database, device resident.  A cf_ferns object belongs to a context of the FULL
 * frame size and works on 8x reduced maps (nearest sampling at source texel (8x + 4, 8y + 4)).  Restrictions, CF_EINVAL otherwise:
 * the frame width is a multiple of 128 and the height a multiple of 32 (the reduced frame must itself be a valid cf_create size:
 * the object owns a second context and a tracker at (W/8) x (H/8), intrinsics divided by 8, enqueueing on the parent's stream);
 * n_ferns in 1..CF_FERNS_MAX; capacity >= 1; max_depth_mm >= 400.  Everything is allocated at creation: per keyframe of capacity
 * round_up(n_ferns, 16) + 27 * (W/8) * (H/8) + 76 bytes. */
#define CF_FERNS_MAX 2048
typedef struct cf_ferns cf_ferns;
typedef struct {
    int32_t x, y;        /* position in the reduced image: 0..W/8-1, 0..H/8-1 */
    int32_t r, g, b;     /* colour thresholds 0..255 */
    int32_t d;           /* depth threshold in millimetres, 400..max_depth_mm */
} cf_fern;               /* Ferns::Fern (Ferns.h) */
typedef struct {
    int n_ferns;            /* reference: 500 */
    int capacity;           /* keyframes */
    int max_depth_mm;       /* Ferns::maxDepth: depth cut-off in millimetres */
    float photo_threshold;  /* Ferns::photoThresh, reference: 115 */
} cf_ferns_config;
typedef struct {
    int accepted;           /* all three acceptance tests of Ferns.cpp:237 passed */
    int keyframe;           /* the match (lowest dissimilarity among keyframes older than min_age), -1: none */
    float dissimilarity;    /* of the match; FLT_MAX: none */
    float overlap;          /* blockHDAware of the current codes and the match's (Ferns.cpp:321-336); the tracker runs when > 0.3 */
    float pose[16];         /* the tracker's estimate, row-major (identity when the tracker did not run) */
    float icp_error, icp_count;
    int icp_ran;            /* 1: the tracker ran (pose, icp_*, photo_* are results) */
    int photo_count;        /* correspondences of the photometric check */
    double photo_error;     /* Ferns::photometricCheck in f64; +inf with no correspondence */
} cf_ferns_result;
/* host helper: the table cf_ferns_create generates from `seed` when none is given (splitmix64, six draws per fern in the order
 * x, y, r, g, b, d, each lo + draw % (hi - lo + 1): DESIGN.md 4.8) */
int cf_ferns_table(uint64_t seed, int n_ferns, int reduced_width, int reduced_height, int max_depth_mm, cf_fern *out);
/* table: n_ferns entries (host) or NULL to generate one from `seed` */
int cf_ferns_create(cf_ctx *ctx, const cf_ferns_config *cfg, const cf_fern *table, uint64_t seed, cf_ferns **out);
void cf_ferns_destroy(cf_ferns *f);
int cf_ferns_get_table(const cf_ferns *f, cf_fern *out /* n_ferns */);
/* Fill the CURRENT slot from a model's fill-in maps (device, full size: f32x4, f32x4, rgba8), ONE launch: reduced vertex / normal
 * maps in the planar layout (z == 0 -> NaN, as cf_copy_maps), reduced rgb, the fern codes of Ferns.cpp:89-109 (255 when the reduced
 * vertex z is not > 0, else (R>r)<<3 | (G>g)<<2 | (B>b)<<1 | (int(z*1000.0f) > d)) and the count of good codes.  Enqueues only. */
int cf_ferns_encode(cf_ferns *f, const float *vertex4, const float *normal4, const uint8_t *rgba);
/* Scan the database for the current slot, ONE launch: co[k] = #{i: q[i] != 255 and q[i] == c[k][i]}, dissimilarity
 * (min(good_q, good_k) - co[k]) / min(good_q, good_k) in f32, (a) its minimum over all keyframes and (b) over the keyframes with
 * time - srcTime > min_age, lowest index on ties (Ferns.cpp:111-127, 184-196).  Enqueues only; cf_ferns_last_search reads. */
int cf_ferns_search(cf_ferns *f, int time, int min_age);
/* Conditional append of the current slot after a search (Ferns.cpp:127: (minimum > threshold || empty) && good > 0), decided and
 * done on the device, ONE launch; at count == capacity nothing is appended and the `full` flag is raised.  Enqueues only. */
int cf_ferns_append(cf_ferns *f, const float pose[16], int src_time, float threshold);
/* Ferns::addFrame: encode -> search -> append, three launches, no host wait (it runs in every tracked frame) */
int cf_ferns_add_async(cf_ferns *f, const float *vertex4, const float *normal4, const uint8_t *rgba, const float pose[16], int src_time,
                       float threshold);
/* Ferns::findFrame (Ferns.cpp:144-262) for the current slot (cf_ferns_encode first); synchronous.  Search; if a match exists and
 * its overlap is > 0.3: ICP of the current reduced maps against the keyframe's stored maps on the small tracker (model side
 * cf_odom_init_icp_model with the keyframe's pose, frame side cf_odom_bind_frame_maps, options rgb_only 0, icp_weight 100, pyramid 0,
 * fast_odom 0, so3 0, starting from the keyframe's pose), then the photometric check; accepted when icp_error < 3e-4, icp_count >
 * (lost ? 1400 : 2400) and photo_error < photo_threshold.  curr_pose is unused (it only feeds loop-closure constraints). */
int cf_ferns_relocalise(cf_ferns *f, const float curr_pose[16], int time, int min_age, int lost, cf_ferns_result *result);
/* the getters wait for the stream */
int cf_ferns_count(cf_ferns *f, int *count, int *full);
/* test access.  id = -1: the current slot (pose identity, time 0).  Host outputs, each nullable: codes u8 [n_ferns], good count,
 * pose, time, reduced vertex / normal maps planar f32 [3 * H/8 * W/8], reduced rgb u8 [H/8 * W/8 * 3] */
int cf_ferns_download(cf_ferns *f, int id, uint8_t *codes, int *good, float pose[16], int *time, float *vmap, float *nmap, uint8_t *rgb);
/* results of the last search: co[0..searched) (co_capacity entries available), the keyframes it scanned, the two minima (FLT_MAX:
 * none), the match (-1: none) and the decision of the last append; each nullable */
int cf_ferns_last_search(cf_ferns *f, int32_t *co_host, int co_capacity, int *searched, float *min_all, float *min_match, int *match_id,
                         int *appended);
/* the loop-closure seam of the database (gate, constraints, findFrame for a camera that is not lost) */
#include "cofusion_loop.h"

/* ------------------------------------------- frame decoder of the .klg log player ---- */
/* Finishes the frames of a .klg log on the device (csrc/frame_decode.hip): host threads inflate the depth and
 * entropy-decode the JPEG into a pinned slot, two launches do the rest -- dequantisation + libjpeg's "islow" IDCT, then chroma
 * upsampling + colour conversion to RGBA8 side by side with u16 mm -> f32 metres.  Integer arithmetic throughout: the outputs equal
 * host/KlgIO.cpp + host/Jpeg.cpp byte for byte.
 * cf_jpeg_header + coefficients are what the JPEG front end (host/Jpeg.cpp) leaves: QUANTISED int16 coefficients, 64 per block in
 * natural (de-zigzagged) order, blocks in raster order per component, components planar (comp[c].first = block offset). */
typedef struct { int32_t h, v, bw, bh, first; } cf_jpeg_comp;  /* sampling factors, block grid (mx*h x my*v), first block */
typedef struct {
    int32_t width, height, ncomp /* 1 or 3 */, hmax, vmax, total_blocks;
    cf_jpeg_comp comp[3];
    uint8_t qt[3][64];      /* per component, natural order */
} cf_jpeg_header;
/* blocks a width x height frame can have at most, whatever its sampling factors (<= 4): three components at the density of the
 * densest, MCUs of at most 32 x 32 */
#define CF_JPEG_MAX_BLOCKS(w, h) (48ull * (uint64_t)(((w) + 31) / 32) * (uint64_t)(((h) + 31) / 32))
#define CF_FRAME_COLOR_NONE 0     /* no colour block in the log: RGBA = 0, 0, 0, 255 */
#define CF_FRAME_COLOR_JPEG 1     /* slot header + coef */
#define CF_FRAME_COLOR_RAW 2      /* slot rgb = the log's 3 B/px block (KlgLogReader::getNext: channels reversed only with flip_colors) */
#define CF_FRAME_COLOR_DECODED 3  /* slot rgb = a host-decoded JPEG in libjpeg's order (reversed UNLESS flip_colors, like _JPEG) */
typedef struct {
    int32_t width, height;        /* 1..max of the decoder */
    int32_t color_kind;           /* CF_FRAME_COLOR_* */
    int32_t flip_colors;          /* LogReader::flipColors */
} cf_frame_desc;
typedef struct {                  /* pinned host staging of one slot */
    cf_jpeg_header *header;
    int16_t *coef;                /* coef_blocks * 64 entries */
    uint64_t coef_blocks;         /* CF_JPEG_MAX_BLOCKS(max_w, max_h) */
    uint16_t *depth;              /* max_w * max_h, millimetres */
    uint8_t *rgb;                 /* max_w * max_h * 3 */
} cf_frame_slot;
typedef struct cf_frame_decoder cf_frame_decoder;
/* slots: 2..16.  Owns the pinned slots, as many device input buffers and output frames (depth f32 [H*W], rgba u8x4 [H*W], alpha 255),
 * a non-blocking stream of its own and one event per slot; nothing is allocated per frame.  Any max_w, max_h >= 1. */
int cf_frame_decoder_create(cf_ctx *ctx, int max_w, int max_h, int slots, cf_frame_decoder **out);
void cf_frame_decoder_destroy(cf_frame_decoder *dec);
int cf_frame_decoder_slot(cf_frame_decoder *dec, int slot, cf_frame_slot *out);
/* Copies the slot's staging to the device and launches the two kernels on the decoder's stream, ordered after what the context's
 * stream holds at this moment (the reader of the output frame this slot produced before), then records the slot's event.
 * The slot's host memory must stay untouched until the event has passed (cf_frame_decoder_acquire with complete = 1). */
int cf_frame_decoder_submit(cf_frame_decoder *dec, int slot, const cf_frame_desc *desc);
/* The output frame of the slot's last submit.  complete = 1: the host blocks on the slot's event (buffers complete at return:
 * cofusion_config.device_frames_complete = 1); complete = 0: the context's stream waits for it (consumed in stream order).
 * The pointers (each nullable) stay valid, and the frame intact, until the slot's next submit. */
int cf_frame_decoder_acquire(cf_frame_decoder *dec, int slot, int complete, const float **depth_dev, const uint8_t **rgba_dev);
/* accumulated device-event durations of the two kernels over all submits while timing is on (cf_frame_decoder_timing(dec, 1): a
 * diagnostics mode that adds event pairs to every submit); reading waits for the decoder's stream and resets the sums */
int cf_frame_decoder_timing(cf_frame_decoder *dec, int on, double *idct_ms, double *finish_ms, uint64_t *frames);

/* ---- image-sequence frames on the same decoder (csrc/image_decode.hip) ----
 * Frames of a directory dataset (PNG / OpenEXR / JPEG / PPM / PGM files): host threads read, inflate and PNG-unfilter into the image
 * staging of a slot (host/ImageIO.cpp), the device turns that into the same output frame cf_frame_decoder_acquire hands out, plus a
 * u8 label mask.  Opt-in: a decoder on which cf_frame_decoder_enable_images was never called allocates nothing for it. */
#define CF_IMAGE_NONE 0   /* colour: RGBA = 0, 0, 0, 255; depth: 0; mask: the frame has none */
#define CF_IMAGE_PNG 1    /* unfiltered scanlines in file layout: row stride 1 + bytes_per_pixel * width (the filter byte stays),
                           * 16-bit samples big-endian.  colour: 8-bit grey / RGB / palette / RGBA; depth: 16-bit grey; mask: 8-bit grey */
#define CF_IMAGE_EXR 2    /* depth only: inflated blocks in cf_image_slot.depth + the table in cf_image_slot.blocks */
#define CF_IMAGE_JPEG 3   /* colour only: header + coef of cf_frame_decoder_slot (the .klg path's kernels; R, G, B unless flip_colors) */
#define CF_IMAGE_RAW 4    /* colour: 3 B/px in cf_frame_slot.rgb (PPM; R, G, B unless flip_colors); mask: 1 B/px in cf_image_slot.mask (PGM) */
/* one block of scanlines of an OpenEXR file as it lies in cf_image_slot.depth.  stored_raw: the file kept the block uncompressed
 * (deflate did not shrink it): the bytes are the pixels, with neither predictor nor interleave to undo */
typedef struct { uint32_t offset, bytes, stored_raw, first_line; } cf_exr_block;
typedef struct {
    int32_t width, height;            /* 1..max of the decoder */
    int32_t color_kind, depth_kind, mask_kind;   /* CF_IMAGE_* */
    int32_t flip_colors;              /* store B, G, R instead of the file's R, G, B */
    int32_t png_color_type;           /* colour PNG: 0 grey, 2 RGB, 3 palette, 6 RGBA */
    int32_t png_palette_entries;      /* colour type 3: 1..256 entries of 3 bytes in cf_image_slot.palette */
    float depth_scale;                /* 16-bit PNG depth: metres = f32(u16) * depth_scale, one f32 product */
    int32_t exr_blocks;               /* entries of cf_image_slot.blocks */
    int32_t exr_lines_per_block;      /* 1 (NONE, ZIPS) or 16 (ZIP) */
    int32_t exr_line_bytes;           /* all channels of one scanline */
    int32_t exr_chan_offset;          /* where the depth channel's run of `width` samples starts inside a scanline */
    int32_t exr_chan_half;            /* 1: HALF, 0: FLOAT */
} cf_image_desc;
typedef struct {                      /* pinned host staging of one slot, beside cf_frame_slot's */
    uint8_t *color;  uint64_t color_bytes;    /* (1 + 4 * max_w) * max_h */
    uint8_t *depth;  uint64_t depth_bytes;    /* 16 * max_w * max_h: a PNG's (1 + 2w) * h, or up to four FLOAT channels of an EXR */
    uint8_t *mask;   uint64_t mask_bytes;     /* (1 + max_w) * max_h */
    uint8_t *palette;                         /* 768 */
    cf_exr_block *blocks;  uint32_t max_blocks;   /* max_h */
} cf_image_slot;
/* allocates, once, the image staging of every slot (pinned), its device mirror and a u8 mask frame per slot */
int cf_frame_decoder_enable_images(cf_frame_decoder *dec);
int cf_frame_decoder_image_slot(cf_frame_decoder *dec, int slot, cf_image_slot *out);
/* cf_frame_decoder_submit for an image frame: same stream, event and ordering rules.  Everything the kernels index with (row strides,
 * the block table, the channel's place) is checked against the slot's sizes first; nothing is launched on an inconsistent frame. */
int cf_frame_decoder_submit_images(cf_frame_decoder *dec, int slot, const cf_image_desc *desc);
/* the mask frame (u8 [H*W]) of the slot's last frame, ordered like cf_frame_decoder_acquire; *mask_dev is
 * NULL where the slot's last frame had no mask (a .klg frame submitted with cf_frame_decoder_submit has none) */
int cf_frame_decoder_acquire_mask(cf_frame_decoder *dec, int slot, int complete, const uint8_t **mask_dev);
/* Device-event durations of the two image kernels, accumulated over the image frames submitted while cf_frame_decoder_timing is on
 * (the same diagnostics mode: the slot's event pairs lie around exr_depth_kernel and around png_finish_kernel, every copy in front
 * of them): the sums in milliseconds and how many frames launched each kernel.  Reading waits for the decoder's stream and resets
 * the sums; the .klg sums of cf_frame_decoder_timing are kept apart and count no image frame. */
int cf_frame_decoder_image_timing(cf_frame_decoder *dec, double *exr_ms, uint64_t *exr_frames, double *finish_ms, uint64_t *finish_frames);

/* ---- PNG encoder of the per-frame exports (csrc/png_encode.hip) ----
 * A device image (8-bit grey or RGBA8) becomes the bands of a complete PNG data stream -- adaptive row filtering, then deflate with
 * the fixed code over runs of equal bytes, or a stored block where that is shorter -- in a pinned slot; the host adds the chunk
 * framing and the CRC (host/ExportWriter.cpp).  The stream is a function of the pixels, channels, rows_per_band and flags alone. */
#define CF_PNG_LABELS 1     /* grey only: a byte > 254 is encoded as 0 (the rejected label of Segmentation<n>.png) */
typedef struct {
    uint32_t offset;        /* of the band's bytes in cf_png_stream.data */
    uint32_t bytes;         /* of the encoded band: whole deflate blocks, ending on a byte */
    uint32_t adler;         /* Adler-32 of the band's filtered scanlines alone ... */
    uint32_t stream_bytes;  /* ... and their length: (1 + channels * width) * rows of the band */
} cf_png_band;
typedef struct {
    int32_t width, height, channels, rows_per_band, bands;
    const cf_png_band *table;   /* bands entries, in the pinned slot */
    const uint8_t *data;        /* the pinned slot's band area */
    uint64_t data_bytes;        /* its extent: every offset + bytes lies inside */
} cf_png_stream;
typedef struct cf_png_encoder cf_png_encoder;
/* slots: 2..16; rows_per_band >= 1 with (1 + 4 * max_w) * rows_per_band <= 65535 (a band is one stored block at most) and a band pair
 * that fits the LDS.  Owns the pinned slots, their device mirrors, a copy stream and one event per slot; nothing is allocated per
 * image.  Any max_w, max_h >= 1. */
int cf_png_encoder_create(cf_ctx *ctx, int max_w, int max_h, int slots, int rows_per_band, cf_png_encoder **out);
void cf_png_encoder_destroy(cf_png_encoder *enc);
/* Encodes src_dev (height rows of width * channels bytes, channels 1 or 4) into the slot without a host wait.  The kernel is launched
 * on the context's stream: it is ordered after what that stream holds at the call, and work enqueued there after the return may
 * overwrite src_dev.  The copy to the pinned slot runs on the encoder's stream behind it; the slot's event follows the copy.  Sizes
 * beyond the encoder's, other channel counts, unknown flags or CF_PNG_LABELS on RGBA: CF_EINVAL, nothing is launched. */
int cf_png_encoder_submit(cf_png_encoder *enc, int slot, const void *src_dev, int width, int height, int channels, int flags);
/* The host blocks on the slot's event.  The band table and the bytes stay intact until the slot's next submit.  May be called from
 * another thread than the one that submits. */
int cf_png_encoder_acquire(cf_png_encoder *enc, int slot, cf_png_stream *out);
/* accumulated device-event duration of the encoding kernel over the submits while timing is on (a diagnostics mode that adds an event
 * pair to every submit); reading waits for the slots submitted so far and resets the sums.  Call it from the submitting thread. */
int cf_png_encoder_timing(cf_png_encoder *enc, int on, double *kernel_ms, uint64_t *images);

/* micro-benchmark of the ICP reduction on the state of the last tracking call (level 0..2) */
int cf_odom_bench_icp(cf_odom *od, int level, int iters, float *avg_us);

/* timing of the most recent reductions, measured with hipEvents on the ctx stream */
typedef struct {
    double icp_ms_total;   /* accumulated GPU time of ICP-reduce launches since last reset */
    uint64_t icp_launches;
    uint64_t icp_bytes;    /* algorithmic bytes of those launches: per level-0 pixel (24 + 24*M) for the ICP reduction of the M
                            * lock-step models + 11*M for the residual passes that share the launch (27*M with
                            * cf_set_gn_mode 0, which writes the 16 B DataTerm records) */
    double surfel_ms_total;   /* stream time of the sampled cf_models_frame_passes chains (index maps, fuse, clean, compactions, prediction) */
    uint64_t surfel_calls;
    uint64_t surfel_bytes;    /* algorithmic bytes of those chains: 8 passes x 48 B per surfel of every fusing model (2 index + 2
                               * splat reads, update read + write, clean read + write), 2 x 48 B per surfel of a model that is only predicted */
} cf_profile;
/* on = 0: off; on = N >= 1: attach begin/end events to the level-0 launches of every N-th tracking call (sampling keeps the host cost
 * of the event pairs out of the measured frame rate) */
int cf_profile_enable(cf_ctx *ctx, int on);
int cf_profile_read(cf_ctx *ctx, cf_profile *out, int reset);

/* ------------------------------------------------------------- loop closure: deformation graph ---- */
/* ElasticFusion's deformation graph (Core/Model/Deformation.*, Core/Utils/DeformationGraph.*, the node branch of copy_unstable.vert),
 * device resident: closure of ONE surfel map from absolute constraints, in the global mode (a fern match: every node is free) and in
 * the graph's local mode (the *_local calls: only the nodes younger than the last deformation are free).  DESIGN.md 4.14 states every
 * rule and every order of operations; tests/deform_ref.py and tests/local_loop_ref.py restate them in numpy.  Everything is allocated at
 * creation, for CF_DEFORM_MAX_NODES nodes and CF_DEFORM_MAX_CONSTRAINTS constraints (pins included; cf_deform_create_sized: up to
 * CF_DEFORM_MAX_CONSTRAINTS_SIZED): about 24 MB, nearly all of it the band of the normal matrix.  The calls are rare and synchronous
 * (each waits for the context's stream) except cf_deform_apply and cf_deform_apply_poses, which only enqueue.  The constraints of a local
 * closure come from cf_local_loop_* (cofusion_loop.h) behind the model-to-model tracker (cf_odom_init_icp_maps); the frame loop that strings
 * them together is CoFusion::setLocalLoopClosure.  Relative constraints: below cf_deform_download.  Not built: the pose graph, object
 * models. */
#define CF_DEFORM_MAX_NODES 1024
#define CF_DEFORM_MAX_CONSTRAINTS 128
#define CF_DEFORM_MAX_CONSTRAINTS_SIZED 1536   /* a local closure at 640x480: 768 constraints and 768 pins */
#define CF_DEFORM_BAND 240          /* band entries per row of A, diagonal included: A_band[i][d] = A[i][i - d] */
typedef struct cf_deform cf_deform;
typedef struct {                    /* the reference's figures: 0.06, 3, 1e-2, 1e-3, 1e-5, 10, 3e-4, 0.12 */
    float min_cons_error; int max_iterations; float min_delta, min_error, min_change, max_first_error, accept_cons_error, accept_error;
} cf_deform_thresholds;
typedef struct { float error; double delta_norm; int failed; float mean_cons_error; } cf_deform_step;
typedef struct {
    int optimised, accepted, failed, iterations;
    float error_before, mean_cons_error_before, error, mean_cons_error;
} cf_deform_result;
typedef struct {                    /* the reactivation stamp of cf_deform_apply (copy_unstable.vert:318-333) */
    float pose[16];                 /* the corrected camera pose, row-major T(world <- camera) */
    cf_cam cam; int cols, rows;
    float max_depth;
    const float *depth;             /* device, [rows * cols]: the frame's filtered depth */
    float conf_threshold;
    int tick;
} cf_deform_reactivate;
int cf_deform_create(cf_ctx *ctx, cf_deform **out);
/* the same object with room for max_constraints (1 .. CF_DEFORM_MAX_CONSTRAINTS_SIZED) constraints; every call takes either kind */
int cf_deform_create_sized(cf_ctx *ctx, int max_constraints, cf_deform **out);
void cf_deform_destroy(cf_deform *d);
void cf_deform_default_thresholds(cf_deform_thresholds *out);
/* every surfel of map_dev (device, `count` records of 12 f32) whose index is a multiple of stride becomes a node; stride = the smallest
 * multiple of sample_rate that leaves at most CF_DEFORM_MAX_NODES.  Parameters become the identity.  nodes < 5: there is no graph, and
 * every later call but sample / set_nodes answers CF_ESTATE.  monotone = 0: node times decrease somewhere (no closure from this graph). */
int cf_deform_sample(cf_deform *d, const float *map_dev, uint32_t count, int sample_rate, int *nodes, int *stride, int *monotone);
/* test access: a crafted graph.  nodes_host [n][4] x y z time; params_host [n][12] (3x3 column-major, translation) or NULL: identity */
int cf_deform_set_nodes(cf_deform *d, const float *nodes_host, const float *params_host, int n);
/* the constraints (host: src, dst [n][3], src_time [n]; a pin is the constraint dst -> dst at dst's time) and their weight sets */
int cf_deform_weights(cf_deform *d, const float *src, const float *dst, const float *src_time, int n);
/* the same from device arrays of the same shapes (cf_ferns_constraint_buffers): no host-to-device copy */
int cf_deform_weights_device(cf_deform *d, const float *src_dev, const float *dst_dev, const float *src_time_dev, int n);
/* residuals, A = J^T J in band storage and b = -J^T r for the current parameters */
int cf_deform_assemble(cf_deform *d);
/* one Gauss-Newton step: assemble, band Cholesky, parameters += delta, the new error.  failed = 1: a pivot <= 0, parameters unchanged */
int cf_deform_iterate(cf_deform *d, cf_deform_step *out);
/* optimiseGraphSparse (fernMatch) from the current parameters + the acceptance of Deformation::constrain; th NULL: the defaults */
int cf_deform_optimise(cf_deform *d, const cf_deform_thresholds *th, cf_deform_result *out);
/* The local mode (lastDeformTime, DeformationGraph.cpp:401-410): node i is enabled iff int(time_i) > last_deform_time.  A disabled
 * node's 12 unknowns leave the system (its blocks of A_band are zero, its diagonal block the identity, its part of b zero: delta = 0
 * there); the rotation rows of a disabled node, an edge between two disabled nodes and a constraint none of whose four nodes is
 * enabled are dropped from J and from `error`; mean_cons_error stays the mean over all constraints.  With every node enabled the
 * three calls compute what cf_deform_assemble / cf_deform_iterate compute, bit for bit. */
int cf_deform_assemble_local(cf_deform *d, int last_deform_time);
int cf_deform_iterate_local(cf_deform *d, int last_deform_time, cf_deform_step *out);
/* optimiseGraphSparse (fernMatch = false) + the acceptance of Deformation::constrain for it: no min_cons_error gate, no
 * max_first_error stop (both fields of th are ignored), the other stop rules as in cf_deform_optimise; accepted = 1 unless a step
 * failed on a pivot <= 0 (failed = 1) or no node is enabled (optimised = 0).  Those two leave the parameters as they were at the call. */
int cf_deform_optimise_local(cf_deform *d, int last_deform_time, const cf_deform_thresholds *th, cf_deform_result *out);
/* the map pass over map_dev in place; re NULL: no reactivation stamp.  Enqueued only.  When the parameters were left by
 * cf_deform_optimise_local (no cf_deform_sample / cf_deform_set_nodes / cf_deform_optimise since), a surfel none of whose four nodes is
 * enabled keeps position and normal bit for bit (a stated departure: the identity of its nodes would still round (p - g) + g); the
 * stamp is applied to it as to every other. */
int cf_deform_apply(cf_deform *d, float *map_dev, uint32_t count, const cf_deform_reactivate *re);
/* applyGraphToPoses over device arrays: poses [n][16] row-major, times [n].  Enqueued only. */
int cf_deform_apply_poses(cf_deform *d, float *poses_dev, const int32_t *times_dev, int n);
/* test access, host outputs, each nullable: nodes [n][4], params [n][12], edges [n][4], ids and weights [constraints][4] (a NaN weight:
 * the point does not move), A_band [12 n][CF_DEFORM_BAND] (after cf_deform_iterate: its Cholesky factor), b [12 n] (after
 * cf_deform_iterate: delta) */
int cf_deform_download(cf_deform *d, int *n_nodes, int *n_constraints, float *nodes, float *params, int32_t *edges, int32_t *ids, float *weights,
                       double *A_band, double *b);

/* Relative constraints (CoFusion.cpp:373, 445-458; DeformationGraph.cpp:578-654): every accepted LOCAL closure leaves a few pairs
 * (moved source, target, srcTime, dstTime) behind, and every later GLOBAL step takes them as rows 10 (phi(src) - phi(tgt)) behind the
 * absolute constraints, so that a fern closure cannot pull apart what a local closure registered.  The pairs live in a device ring of
 * `capacity` (CF_DEFORM_MIN_RELATIVE .. CF_DEFORM_MAX_RELATIVE) slots: pair number k ever appended is in slot k mod capacity, the
 * newest overwrites the oldest, and the rows follow slot order.  The pairs are world points; later deformations do not move them.
 * A relative row couples node groups arbitrarily far apart, which the band cannot hold: with pairs in the ring cf_deform_assemble /
 * cf_deform_iterate / cf_deform_optimise solve A = B + U^T U on the band factor of B (y = L^-1 b, Y = L^-1 U^T, C = I + Y^T Y,
 * t = C^-1 Y^T y, delta = L^-T (y - Y t)); error counts the relative rows, and mean_cons_error divides the sum over the absolute
 * constraints by the number of ALL constraints (nonRelativeConstraintError).  With the ring empty every launch is the one of an
 * object without it.  The *_local calls answer CF_EINVAL while the ring holds pairs.  Off until enabled: the storage (38 MB at 128
 * pairs, nearly all of it Y) is allocated by this call, not by cf_deform_create. */
#define CF_DEFORM_MAX_RELATIVE 128
#define CF_DEFORM_MIN_RELATIVE 8
int cf_deform_enable_relative(cf_deform *d, int capacity);
/* n pairs from host arrays (src, dst [n][3], src_time, dst_time [n]); append = 0: the ring is emptied first (n = 0 only empties it) */
int cf_deform_set_relative(cf_deform *d, const float *src, const float *dst, const float *src_time, const float *dst_time, int n, int append);
/* the same from device arrays: one scatter launch, no copy through the host.  Enqueued only. */
int cf_deform_set_relative_device(cf_deform *d, const float *src_dev, const float *dst_dev, const float *src_time_dev, const float *dst_time_dev,
                                  int n, int append);
/* what an accepted closure of the graph `from` leaves, no host round trip: of its n constraints (device rows row_stride * i of src, dst
 * [.][3] and time [.]; dst_time_dev [n], one per constraint) the indices 0, s, 2s, .. < n with s = max(1, n / 3); each source is moved by
 * `from` as cf_deform_apply would move a surfel there and appended to d's ring with its target.  Enqueued only.  picked: how many. */
int cf_deform_pick_relative(cf_deform *d, cf_deform *from, const float *src_dev, const float *dst_dev, const float *time_dev, const float *dst_time_dev,
                            int n, int row_stride, int *picked);
/* test access, host outputs, each nullable: the ring's capacity, the pairs it holds, the pairs ever appended, the pairs in the system of
 * the last cf_deform_optimise; pairs [count][8] (source xyz, srcTime, target xyz, dstTime) in slot order; after cf_deform_assemble or
 * later: ids and weights [2][count][4] (sources, then targets), U in compact form u_ids [count][8] (node of each slot, -1: unused) and
 * u_vals [count][8][4], r_rel [3 count]; after cf_deform_iterate: C [3 count + 1][3 count] = I + Y^T Y (symmetric) with Y^T y as its
 * last row */
int cf_deform_download_relative(cf_deform *d, int *capacity, int *count, int64_t *appended, int *used, float *pairs, int32_t *ids, float *weights,
                                int32_t *u_ids, double *u_vals, double *r_rel, double *C);
/* test access: the 32-byte record the last residual pass / solve left on the device (error, mean_cons_error f32; delta_norm f64;
 * failed, enabled i32; two words of padding), copied out as it stands */
int cf_deform_download_out(cf_deform *d, void *out32);
/* benchmark access: only the launch Y = L^-1 U^T of a step with relative rows, on the state the last cf_deform_iterate left (its band
 * factor and its rows); it rewrites Y with the same bytes.  Enqueued only. */
int cf_deform_bench_relative_y(cf_deform *d);

/* ------------------------------------------------ mesh export ---- */
/* A triangle mesh of one surfel map, extracted on the device in two stages (csrc/mesh.hip; tests/mesh_ref.py states both in numpy
 * and the device equals it bit for bit, order of the output included):
 *   (a) every confident surfel (conf > conf_threshold, savePly's rule) adds a quantised weight and signed distance to the samples of
 *       a dense grid inside its support, with 64-bit INTEGER atomics (sums that commute: no dependence on launch shape or arrival);
 *   (b) marching tetrahedra on Kuhn's six tetrahedra per cell: shared vertices on 7 edge kinds per sample, ordered by (sample, kind);
 *       triangles ordered by (cell, tetrahedron, triangle), wound so that the geometric normal points outside.
 * Positive distance = outside = the side a surfel was observed from (stored normals point away from the camera; they are negated here
 * as savePly negates them).  A cell emits only when its 8 corners are valid: unobserved space leaves an open boundary.  Triangles of
 * zero area (a sample exactly on the surface) are kept: the topology comes first.  A voxel far below the surfel radius leaves holes
 * once the support radius hits its cap of max_support_voxels.
 * A cf_mesher owns the grid and the scan scratch for max_voxels samples (64 bytes each); vertices and triangles are allocated after the
 * counting pass.  Every launch is enqueued on the context's stream behind the frame's lanes (as cf_render); the host waits only for
 * the counts, the default grid's bounds and the downloads.  Nothing of the frame loop is touched. */
#define CF_ERANGE (-5)              /* a grid over max_voxels, or a vertex / triangle count over 2^32 - 1 */
typedef struct cf_mesher cf_mesher;
typedef struct {
    float origin[3];                /* sample (0, 0, 0) */
    float voxel;                    /* > 0 */
    int32_t nx, ny, nz;             /* corner samples per axis; sample (x, y, z) has the linear index (z * ny + y) * nx + x */
} cf_mesh_grid;
typedef struct {                    /* NULL where a call takes one: 3, 4, 100 */
    float trunc_voxels;             /* tau = trunc_voxels * voxel */
    float max_support_voxels;       /* rho = clamp(radius, 1.5 voxel, max_support_voxels * voxel) */
    float conf_cap;                 /* w = min(conf, conf_cap) * (1 - t^2 / rho^2) */
} cf_mesh_params;
typedef struct { float x, y, z, nx, ny, nz; uint8_t r, g, b, a; } cf_mesh_vertex;   /* 28 bytes */
#define CF_MESH_MAX_VOXELS (1u << 28)
int cf_mesh_create(cf_ctx *ctx, uint64_t max_voxels, cf_mesher **out);   /* 1 .. CF_MESH_MAX_VOXELS */
void cf_mesh_destroy(cf_mesher *m);
/* the default placement: the exact box of the confident surfels padded by tau; voxel = 0: the mean confident radius (an exact integer
 * sum of radii quantised to 2^-16); the voxel grows by a quarter at a time until the grid fits max_voxels.  No confident surfel: a grid
 * of 0 x 0 x 0 samples, which the other calls accept and turn into an empty mesh.  One host wait (the bounds). */
int cf_mesh_default_grid(cf_mesher *m, cf_model *model, float conf_threshold, float voxel, cf_mesh_grid *grid);
/* stage (a): clears the grid, then adds the surfels of `model`, or, with model NULL, the `count` surfels at surfels_dev (device, 12 f32
 * each).  CF_ERANGE when the grid has more samples than max_voxels.  Enqueued only. */
int cf_mesh_accumulate(cf_mesher *m, cf_model *model, const float *surfels_dev, uint32_t count, float conf_threshold, const cf_mesh_grid *grid,
                       const cf_mesh_params *params);
/* stage (b) on the accumulated grid: a sample is valid iff its weight sum is at least max(rint(w_min * 2^12), 1); its distance is
 * (float)((double)sum(wq dq) / (double)sum(wq)).  Waits for the two counts. */
int cf_mesh_extract(cf_mesher *m, float w_min, uint32_t *n_vertices, uint32_t *n_triangles);
/* host arrays of the last extraction: n_vertices records, n_triangles x 3 indices; either may be NULL */
int cf_mesh_download(cf_mesher *m, cf_mesh_vertex *vertices, uint32_t *triangles);
/* test access: the integer accumulators of the last cf_mesh_accumulate, int64 [5][nz * ny * nx]: sum wq dq, sum wq, sum wq {r, g, b} */
int cf_mesh_grid_download(cf_mesher *m, int64_t *acc_host);
/* test access: stage (b) on a caller's field (host arrays: sdf f32 [n], valid u8 [n], rgb f32 [n][3] or NULL for black) */
int cf_mesh_extract_grid(cf_mesher *m, const cf_mesh_grid *grid, const float *sdf_host, const uint8_t *valid_host, const float *rgb_host,
                         uint32_t *n_vertices, uint32_t *n_triangles);
/* benchmark access: milliseconds of the last cf_mesh_accumulate and of the last extraction, by device events (waits for them) */
int cf_mesh_timing(cf_mesher *m, float *accumulate_ms, float *extract_ms);

#ifdef __cplusplus
}
#endif
#endif /* COFUSION_HIP_H_ */
