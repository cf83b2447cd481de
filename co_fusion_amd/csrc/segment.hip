// segment.hip -- GPU side of the motion segmentation (Core/Segmentation/*): SLIC superpixels, the
// per-superpixel accumulations that replace the reference's full-resolution texture downloads
// (Segmentation.cpp:184-188: 6.1 MB of glGetTexImage per model per frame), the dense-CRF mean field over
// the 40x30 superpixel grid, and the label up-sampling.  Plus its C-ABI (cf_seg_*).
//
// gSLICr and densecrf are third-party and not vendored by the reference (Scripts/install.sh:84-85); they are
// replaced by their published algorithms exactly as stated in oracle/orc_segment.c (same arithmetic, same
// summation order => bit-identical to the oracle):
//   * SLIC (gSLICr's published engine: metric, normalisers, schedule -- see the oracle's header): one 16x16-pixel workgroup per grid cell; a pixel can only join one of the 3x3 neighbouring
//     clusters, so each workgroup privatises 9 x 6 integer accumulators in LDS and issues 54 global atomics.
//   * accumulation: same tiling; exact Q32 fixed-point sums (order independent).
//   * CRF: the two 1200x1200 Gaussian kernels are evaluated exactly (no permutohedral lattice), stored
//     transposed so that the sequential-in-j mean-field sums read coalesced rows.
//
// One translation unit, one stage per file; this file keeps the segmenter's set-up and tear-down, the C-ABI and its enqueue helpers:
//   seg_slic_dev.h    SLIC, the Q32 sums per superpixel (+ the resample labels), the label up-sampling
//   seg_unary_dev.h   means, unaries and CRF features in one workgroup per segmenter; the grid's smoothness features
//   seg_crf_dev.h     kernel matrices, first marginals, the mean-field step and its launchers
//   seg_post_dev.h    arg-max, components, gates, statistics, the published decisions; the pose words of model-parallel callers
// (cf_segment.h: what they share with each other and with segment_masks.hip.)
//
// The chain (cf_seg_sums + cf_seg_infer, or cf_seg_run_batch for the segmenters of a lock-step group) is seg_accumulate -> seg_unary ->
// crf_rownorm + crf_kernel_matrix (+ first marginals) -> iterations x (crf_message, crf_update) -> seg_post -> seg_upsample, one stream,
// behind the frame's tracking, no host wait: cf_seg_fetch collects the decisions seg_post left in pinned memory.  Of its inputs
// only the models' ICP error surfaces come from the tracker; the frame's depth and colour, the SLIC labels and the models' confidence
// projections (the previous frame's prediction) exist when the frame starts.  cf_seg_early therefore runs, beside the tracking launches,
//   seg_accumulate<kAccFrame | kAccConf> -> seg_unary<kUnaryFrame> -> crf_rownorm + crf_kernel_matrix
// and leaves behind the tracker
//   seg_accumulate<kAccIcp> -> seg_unary<kUnaryTrack> (+ first marginals) -> iterations x (crf_message, crf_update) -> seg_post -> seg_upsample
// Both halves are flavours of the SAME kernel texts (compile-time masks), all sums are exact integers or keep their sequential order: the
// split chain's results are the plain chain's bit for bit (tests/test_segment_early_gpu.py; DESIGN-NOTES R7).
// cf_seg_slic and cf_seg_crf are the unit-level entries to SLIC and to the mean field (host arrays in and out, synchronous).
#include <string.h>

#include <string>
#include <vector>

#include "cf_host.h"
#include "cf_segment.h"
#ifdef CF_ABLATE
namespace cf { __device__ unsigned long long g_seg_trace[2][16]; }   // GSTAMP's stamps (cf_segment.h), printed by enqueue_infer
#endif
#include "seg_slic_dev.h"
#include "seg_unary_dev.h"
#include "seg_crf_dev.h"
#include "seg_post_dev.h"

using namespace cf;

template <typename T>
static int seg_malloc(cf_ctx* ctx, T** p, size_t count)
{
    if (count == 0) return CF_OK;   // (a segmenter of the mask branch alone has no superpixel grid: K == 0)
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    HIPCHK(ctx, hipMemsetAsync(*p, 0, count * sizeof(T), ctx->stream));
    return CF_OK;
}

// the labels of an inference: one per model and, where a new model may spawn, its label
static int label_count(int n_models, int allow_new) { return n_models + (allow_new ? 1 : 0); }
// ... which the segmenter's buffers must hold
static int check_labels(cf_segmenter* s, int L)
{
    if (L <= s->Lcap) return CF_OK;
    s->ctx->set_error("segmentation: more labels than the context's max_models (" + std::to_string(s->Lcap) + ")");
    return CF_EINVAL;
}
// [Lcap][kPoseWords] behind the ICP-error and confidence sums, in their block (seg_create; cf_seg_publish_poses)
static long long* pose_tail(cf_segmenter* s) { return reinterpret_cast<long long*>(s->icp_sum) + 2 * (size_t)s->Lcap * s->K; }

// the models' image pointers of the accumulation launch: kernel arguments for up to kAccTile models, a device table beyond
// (icp_err / vertconf4 may be NULL where the launch does not take that part: the table keeps what an earlier call put there)
static int acc_pointers(cf_segmenter* s, AccArgs& a, int n_models, const float* const* icp_err, const float* const* vertconf4)
{
    if (n_models <= kAccTile) {
        for (int m = 0; m < n_models; m++) {
            if (icp_err) a.icp[m] = icp_err[m];
            if (vertconf4) a.vconf[m] = reinterpret_cast<const float4*>(vertconf4[m]);
        }
        return CF_OK;
    }
    cf_ctx* ctx = s->ctx;
    for (int m = 0; m < n_models; m++) {
        if (icp_err) s->h_acc_ptrs[m] = icp_err[m];
        if (vertconf4) s->h_acc_ptrs[s->Lcap + m] = vertconf4[m];
    }
    HIPCHK(ctx, hipMemcpyAsync(s->d_acc_ptrs, s->h_acc_ptrs, sizeof(void*) * 2 * (size_t)s->Lcap, hipMemcpyHostToDevice, ctx->stream));
    a.icp_dev = reinterpret_cast<const float* const*>(s->d_acc_ptrs);
    a.vconf_dev = reinterpret_cast<const float4* const*>(s->d_acc_ptrs + s->Lcap);
    return CF_OK;
}

extern "C" {

// masks_only: no superpixel grid (K == 0) -- the label-mask branch works on whole images of any size the context accepts
static int seg_create(cf_ctx* ctx, cf_segmenter** out, bool masks_only)
{
    if (!ctx || !out) return CF_EINVAL;
    if (!masks_only) {
        if ((ctx->cfg.width % kSpix) || (ctx->cfg.height % kSpix)) { ctx->set_error("segmentation needs width/height multiples of 16"); return CF_EINVAL; }
        if ((ctx->cfg.width / kSpix) * (ctx->cfg.height / kSpix) > kSegMaxK) { ctx->set_error("segmentation supports at most 4800 superpixels (1280x960)"); return CF_EINVAL; }
    }
    cf_segmenter* s = new cf_segmenter();
    s->ctx = ctx;
    if (!masks_only) { s->gx = ctx->cfg.width / kSpix; s->gy = ctx->cfg.height / kSpix; s->K = s->gx * s->gy; }
    *out = s;
    s->Lcap = ctx->cfg.max_models < 16 ? 16 : (ctx->cfg.max_models > kMaxL - 1 ? kMaxL - 1 : ctx->cfg.max_models);   // at least 16 (as before round 4); ids 0..254, 255 = rejected
    const size_t N = (size_t)ctx->cfg.width * ctx->cfg.height, K = (size_t)s->K, Lc = (size_t)s->Lcap;
    if (int r = seg_malloc(ctx, &s->d_acc_ptrs, 2 * Lc)) return r;
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&s->h_acc_ptrs), sizeof(void*) * 2 * Lc));
    if (int r = seg_malloc(ctx, &s->labels, masks_only ? (size_t)0 : N)) return r;
    if (int r = seg_malloc(ctx, &s->centres, K * 5)) return r;
    if (int r = seg_malloc(ctx, &s->slic_sums, K * 6)) return r;
    if (int r = seg_malloc(ctx, &s->spix_count, K)) return r;
    if (int r = seg_malloc(ctx, &s->depth_count, K)) return r;
    if (int r = seg_malloc(ctx, &s->depth_sum, K)) return r;
    // [icp | conf | pose tail] in one block: one collective of a model-parallel caller covers all of it (cf_seg_publish_poses)
    if (int r = seg_malloc(ctx, &s->icp_sum, 2 * K * Lc + Lc * kPoseWords)) return r;
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&s->h_pose_tail), sizeof(long long) * Lc * kPoseWords));
    s->conf_sum = s->icp_sum + K * Lc;
    if (int r = seg_malloc(ctx, &s->resample, K)) return r;
    if (int r = seg_malloc(ctx, &s->low_map, K)) return r;
    if (int r = seg_malloc(ctx, &s->feat1, K * 2)) return r;
    if (int r = seg_malloc(ctx, &s->feat2, K * 6)) return r;
    if (int r = seg_malloc(ctx, &s->norm, K)) return r;
    if (int r = seg_malloc(ctx, &s->K1t, K * K)) return r;
    if (int r = seg_malloc(ctx, &s->K2t, K * K)) return r;
    if (int r = seg_malloc(ctx, &s->partial, (size_t)kCrfChunks * K * 2 * Lc)) return r;
    if (int r = seg_malloc(ctx, &s->unary, K * Lc)) return r;
    if (int r = seg_malloc(ctx, &s->Q0, K * Lc)) return r;
    if (int r = seg_malloc(ctx, &s->Q1, K * Lc)) return r;
    if (int r = seg_malloc(ctx, &s->raw_mean, K ? K * (3 + 2 * Lc) + 2 : (size_t)0)) return r;  // raw sums + the two lists of empty superpixels + their lengths
    if (int r = seg_malloc(ctx, &s->low_mean, K * (1 + 2 * Lc))) return r;
    if (int r = seg_malloc(ctx, &s->avg_conf, Lc)) return r;
    if (int r = seg_malloc(ctx, &s->depth_range, (size_t)1)) return r;
    if (int r = seg_malloc(ctx, &s->cc, 6 * K)) return r;
    if (int r = seg_malloc(ctx, &s->d_result, (size_t)1)) return r;
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&s->h_result), sizeof(cf_seg_result), hipHostMallocCoherent));  // seg_post_kernel stores into it
    if (K) HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&s->h_low_map), ((size_t)K + 3) / 4 * 4, hipHostMallocCoherent));  // written as 32-bit words by seg_post_kernel
    memset(s->h_result, 0, sizeof(cf_seg_result));
    // the mask branch: two work blocks, both in the state a job expects to find (cf_segment.h: kMaskWork)
    if (int r = seg_malloc(ctx, &s->mask_work, (size_t)2 * kMaskWork)) return r;
    {
        const unsigned none = 0xffffffffu;
        for (int b = 0; b < 2; b++) HIPCHK(ctx, hipMemcpyAsync(s->mask_work + b * kMaskWork, &none, sizeof(none), hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&s->h_mask_new), sizeof(int), hipHostMallocCoherent));  // stored by mask_stats_kernel
    *s->h_mask_new = -1;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}

int cf_seg_create(cf_ctx* ctx, cf_segmenter** out) { return seg_create(ctx, out, false); }
int cf_seg_create_masks(cf_ctx* ctx, cf_segmenter** out) { return seg_create(ctx, out, true); }

void cf_seg_destroy(cf_segmenter* s)
{
    if (!s) return;
    (void)hipStreamSynchronize(s->ctx->stream);
    void* ptrs[] = {s->labels, s->centres, s->slic_sums, s->spix_count, s->depth_count, s->depth_sum, s->icp_sum, s->resample,
                    s->low_map, s->feat1, s->feat2, s->norm, s->K1t, s->K2t, s->partial, s->unary, s->Q0, s->Q1,
                    s->raw_mean, s->low_mean, s->avg_conf, s->depth_range, s->cc, s->d_result, (void*)s->d_acc_ptrs,
                    s->mask_work};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (s->h_mask_new) (void)hipHostFree(s->h_mask_new);
    if (s->h_result) (void)hipHostFree(s->h_result);
    if (s->h_low_map) (void)hipHostFree(s->h_low_map);
    if (s->h_pose_tail) (void)hipHostFree(s->h_pose_tail);
    if (s->h_acc_ptrs) (void)hipHostFree(s->h_acc_ptrs);
    delete s;
}

// Slic::setInputImage + processFrame (Slic.cpp:48-81): labels stay on the device
int cf_seg_slic(cf_segmenter* s, const uint8_t* rgba)
{
    if (!s || !rgba || !s->K) return CF_EINVAL;
    cf_ctx* ctx = s->ctx; hipStream_t st = ctx->stream;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    const uchar4* img = reinterpret_cast<const uchar4*>(rgba);
    slic_init_kernel<<<(s->K + 255) / 256, 256, 0, st>>>(img, W, s->gx, s->K, s->centres);
    HIPCHK(ctx, hipMemsetAsync(s->slic_sums, 0, sizeof(unsigned long long) * 6 * s->K, st));
    // gSLICr's Perform_Segmentation: assign; no_iters (5, Slic.cpp:38) x {update; assign} -- the labels are the sixth pass's
    for (int it = 0; it <= 5; it++) {
        if (it > 0) slic_update_kernel<<<(s->K + 255) / 256, 256, 0, st>>>(s->slic_sums, s->K, s->centres);
        slic_assign_kernel<<<dim3(s->gx, s->gy), 256, 0, st>>>(img, W, H, s->gx, s->gy, s->centres, s->labels, s->slic_sums);
    }
    LAUNCHCHK(ctx);
    return CF_OK;
}

static CrfSeq crf_seq(cf_segmenter* s, int L)
{
    CrfSeq m{};
    m.feat = s->feat2; m.norm = s->norm; m.Kt = s->K2t; m.K1t = s->K1t; m.K2t = s->K2t;
    m.unary = s->unary; m.Q0 = s->Q0; m.Q1 = s->Q1; m.partial = s->partial; m.L = L;
    return m;
}
// the smoothness kernel K1t from feat1 (make_features: the grid's own features first -- seg_feat1_kernel)
static void build_grid_kernel(cf_segmenter* s, bool make_features)
{
    hipStream_t st = s->ctx->stream;
    const int n = s->K;
    if (make_features) seg_feat1_kernel<<<(n + 255) / 256, 256, 0, st>>>(s->gx, n, s->feat1);
    CrfBatch B;
    memset(&B, 0, sizeof(B));
    B.m[0] = crf_seq(s, 0);
    B.m[0].feat = s->feat1; B.m[0].Kt = s->K1t;
    launch_crf_kernel_matrix<2>(st, B, 1, n, false);
}

// DenseCRF2D inference as used by Segmentation.cpp:436-480 (exact kernels, see the file header).
// unary [K*L] row-per-node, feat_smooth [K*2], feat_app [K*6] host in; Q [K*L] host out (synchronous).
int cf_seg_crf(cf_segmenter* s, const float* unary_host, int L, const float* feat_smooth_host, const float* feat_app_host,
               float w_smooth, float w_app, int iterations, float* Q_host)
{
    if (!s || !s->K || !unary_host || !Q_host || L <= 0 || L > s->Lcap) return CF_EINVAL;
    cf_ctx* ctx = s->ctx; hipStream_t st = ctx->stream;
    const int n = s->K;
    HIPCHK(ctx, hipMemcpyAsync(s->unary, unary_host, sizeof(float) * n * L, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(s->feat2, feat_app_host, sizeof(float) * n * 6, hipMemcpyHostToDevice, st));
    // the smoothness kernel only depends on the superpixel grid: rebuilt only when its features change
    const bool same_smooth = s->smooth_cache.size() == (size_t)n * 2 && memcmp(s->smooth_cache.data(), feat_smooth_host, sizeof(float) * n * 2) == 0;
    if (!same_smooth) {
        HIPCHK(ctx, hipMemcpyAsync(s->feat1, feat_smooth_host, sizeof(float) * n * 2, hipMemcpyHostToDevice, st));
        build_grid_kernel(s, false);
        s->smooth_cache.assign(feat_smooth_host, feat_smooth_host + (size_t)n * 2);
        s->grid_kernel_built = false;
    }
    CrfBatch B;
    memset(&B, 0, sizeof(B));
    B.m[0] = crf_seq(s, L);
    launch_crf_kernel_matrix<6>(st, B, 1, n, true);
    s->last_flip = launch_mean_field(st, B, 1, n, iterations, w_smooth, w_app);
    s->last_n = 0; s->last_L = L;
    const float* q = s->last_flip ? s->Q1 : s->Q0;
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(Q_host, q, sizeof(float) * n * L, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return CF_OK;
}

// ---- device-resident flavour: sums -> [collective] -> unaries -> mean field -> post-processing -> mask, no host wait ----
// One entry of a batched segmentation: what cf_seg_sums + cf_seg_infer take for one segmenter
struct SegJob {
    cf_segmenter* s; const float* depth; int n_models; const float* const* icp_err; const float* const* vertconf4;
    const uint8_t* rgba; const uint32_t* model_ids; uint32_t next_model_id; int allow_new; uint8_t* full_dev;
};
// An early half (cf_seg_early) that no inference will finish: what it left for the late half goes, so that the accumulators are
// clean again (the early unary kernel zeroed the ones it consumed)
static int early_discard(cf_segmenter* s)
{
    const int was = s->early;
    if (!was) return CF_OK;
    s->early = 0;
    HIPCHK(s->ctx, hipMemsetAsync(s->spix_count, 0, sizeof(unsigned) * (size_t)s->K, s->ctx->stream));
    if (was >= 2) HIPCHK(s->ctx, hipMemsetAsync(s->icp_sum, 0, sizeof(unsigned long long) * (size_t)s->K * s->early_n, s->ctx->stream));
    return CF_OK;
}
// the sums of S <= kSegBatch segmenters of one image size in ONE launch (+ the resample labels in its extra grid row); parts: kAcc*
static int enqueue_accumulate(cf_ctx* ctx, const SegJob* jobs, int S, int parts = kAccAll)
{
    hipStream_t st = ctx->stream;
    cf_segmenter* s0 = jobs[0].s;
    SegBatch<AccArgs> B;
    memset(&B, 0, sizeof(B));
    const bool frame = (parts & kAccFrame) != 0;
    const bool ride = frame && s0->gy <= 256;  // (gx workgroups of 256 threads cover the K = gx * gy resample points)
    for (int e = 0; e < S; e++) {
        cf_segmenter* s = jobs[e].s;
        AccArgs& a = B.m[e];
        a.labels = s->labels; a.depth = jobs[e].depth; a.n_models = jobs[e].n_models; a.cols = ctx->cfg.width; a.rows = ctx->cfg.height; a.gx = s->gx; a.gy = s->gy;
        if (int r = acc_pointers(s, a, jobs[e].n_models, jobs[e].icp_err, jobs[e].vertconf4)) return r;
        a.spix_count = s->spix_count; a.depth_count = s->depth_count; a.depth_sum = s->depth_sum; a.icp_sum = s->icp_sum; a.conf_sum = s->conf_sum;
        a.resample = ride ? s->resample : nullptr;
    }
    const dim3 grid(s0->gx, s0->gy + (ride ? 1 : 0), S);
    if (parts == kAccAll) seg_accumulate_kernel<kAccAll><<<grid, 256, 0, st>>>(B);
    else if (parts == (kAccFrame | kAccConf)) seg_accumulate_kernel<kAccFrame | kAccConf><<<grid, 256, 0, st>>>(B);
    else if (parts == kAccIcp) seg_accumulate_kernel<kAccIcp><<<grid, 256, 0, st>>>(B);
    else { ctx->set_error("segmentation: no accumulation kernel for these parts"); return CF_EINVAL; }
    if (frame && !ride)
        for (int e = 0; e < S; e++)
            seg_resample_kernel<<<(jobs[e].s->K + 255) / 256, 256, 0, st>>>(jobs[e].s->labels, ctx->cfg.width, ctx->cfg.height, s0->gx, s0->gy, jobs[e].s->resample);
    LAUNCHCHK(ctx);
    return CF_OK;
}

// Slic::downsample* sums of the frame and of every model (Slic.h:48-120), left on the device.  *sums_dev (nullable) receives the
// device address of the per-model sums -- int64 [2][max_models][K]: ICP-error sums of model m at [0][m][.], confidence sums at [1][m][.] --
// which a model-parallel caller SUM-all-reduces in place over the ranks before cf_seg_infer (owners contribute, everybody else
// passes zero images).  The accumulators are expected zero on entry; cf_seg_infer leaves them zero again.
int cf_seg_sums(cf_segmenter* s, const float* depth, int n_models, const float* const* icp_err, const float* const* vertconf4,
                int64_t** sums_dev, uint64_t* sums_words)
{
    if (!s || !s->K || !depth || n_models <= 0 || n_models > s->Lcap || !icp_err || !vertconf4) return CF_EINVAL;
    SegJob job{};
    job.s = s; job.depth = depth; job.n_models = n_models; job.icp_err = icp_err; job.vertconf4 = vertconf4;
    // behind a matching cf_seg_early only the ICP-error sums are left (the block then holds those alone: the confidence sums were
    // consumed beside the tracking); an early half that does not match is dropped and the whole launch runs
    bool late = s->early == 1 && s->early_n == n_models && s->early_depth == depth;
    for (int m = 0; late && m < n_models; m++) late = s->early_vconf[m] == vertconf4[m];
    if (late) {
        if (int r = enqueue_accumulate(s->ctx, &job, 1, kAccIcp)) return r;
        s->early = 2;
    } else {
        if (int r = early_discard(s)) return r;
        if (int r = enqueue_accumulate(s->ctx, &job, 1)) return r;
    }
    if (sums_dev) *sums_dev = reinterpret_cast<int64_t*>(s->icp_sum);
    if (sums_words) *sums_words = 2ull * (uint64_t)s->Lcap * (uint64_t)s->K + (uint64_t)s->Lcap * kPoseWords;  // the pose tail rides along (zeros unless published)
    return CF_OK;
}

// Model-parallel callers: put the poses the trackers hold on THIS process behind the sums (trackers[m] == NULL: model m is tracked
// elsewhere), between cf_seg_sums and the all-reduce; after cf_seg_infer + cf_seg_fetch, cf_seg_fetch_poses hands out all of them.
// Replaces a separate (blocking) pose exchange per frame.
int cf_seg_publish_poses(cf_segmenter* s, int n_models, cf_odom* const* trackers)
{
    if (!s || n_models <= 0 || n_models > s->Lcap || !trackers) return CF_EINVAL;
    PosePublishArgs a{};
    a.n = n_models;
    for (int m = 0; m < n_models; m++) a.st[m] = trackers[m] ? trackers[m]->d_state : nullptr;
    pose_publish_kernel<<<s->Lcap, 64, 0, s->ctx->stream>>>(a, pose_tail(s));
    LAUNCHCHK(s->ctx);
    s->poses_published = true;
    return CF_OK;
}
// words: [n_models][18] (16 pose words row-major, ICP error, ICP inlier count) as written by the owners; valid after cf_seg_fetch
int cf_seg_fetch_poses(cf_segmenter* s, int n_models, int64_t* words_host)
{
    if (!s || n_models <= 0 || n_models > s->Lcap || !words_host) return CF_EINVAL;
    if (!s->poses_published) { s->ctx->set_error("cf_seg_fetch_poses: no poses were published for this inference"); return CF_ESTATE; }
    HIPCHK(s->ctx, hipStreamSynchronize(s->ctx->stream));
    memcpy(words_host, s->h_pose_tail, sizeof(int64_t) * (size_t)n_models * kPoseWords);
    s->poses_published = false;
    return CF_OK;
}

}  // extern "C"
// Everything after the sums (Segmentation.cpp:160-706) for S <= kSegBatch segmenters of one image size in one chain of launches: unaries,
// kernel matrices, mean-field steps, arg-max / connected components / gates / statistics, up-sampling into full_dev.  CAP: the capacity
// of the id table in the post-processing arguments (17 for a batch, 257 for one segmenter with many labels).
static void unary_args(SegUnaryArgs& u, cf_segmenter* s, const SegJob& job, const cf_seg_params* P)
{
    const int n_models = job.n_models, L = label_count(n_models, job.allow_new);
    u.K = s->K; u.gx = s->gx; u.gy = s->gy; u.n_models = n_models; u.L = L; u.allow_new = job.allow_new ? 1 : 0;
    u.unaryWeightError = P->unaryWeightError; u.unaryKError = P->unaryKError; u.unaryThresholdNew = P->unaryThresholdNew;
    u.scaleFeaturesRGB = P->scaleFeaturesRGB; u.scaleFeaturesDepth = P->scaleFeaturesDepth; u.scaleFeaturesPos = P->scaleFeaturesPos;
    u.spix_count = s->spix_count; u.depth_count = s->depth_count; u.depth_sum = s->depth_sum; u.icp_sum = s->icp_sum; u.conf_sum = s->conf_sum;
    u.resample = s->resample; u.rgba = reinterpret_cast<const uchar4*>(job.rgba);
    u.raw = s->raw_mean; u.low = s->low_mean; u.unary = s->unary; u.feat2 = s->feat2; u.avg_conf = s->avg_conf; u.depth_range = s->depth_range;
    u.empties = reinterpret_cast<int*>(s->raw_mean + (size_t)(1 + 2 * s->Lcap) * s->K);   // behind the rows of every model count
    u.Q0 = s->Q0;
}
// the smoothness kernel only depends on the superpixel grid: built once per segmenter
static void ensure_grid_kernel(cf_segmenter* s)
{
    if (s->grid_kernel_built) return;
    build_grid_kernel(s, true);
    s->grid_kernel_built = true;
    s->smooth_cache.clear();
}
// `late`: the jobs' early halves ran (cf_seg_early) -- the unary kernel's kUnaryTrack flavour, and the appearance kernels exist
template <int CAP, int N>
static int enqueue_infer(cf_ctx* ctx, const cf_seg_params* P, const SegJob* jobs, int S, bool late = false)
{
    hipStream_t st = ctx->stream;
    const int n = jobs[0].s->K;
    SegBatch<SegUnaryArgs> U;
    CrfBatch C;
    SegBatch<SegPostArgsT<CAP>, N> PB;
    SegBatch<UpsampleArgs> UP;
    memset(&U, 0, sizeof(U)); memset(&C, 0, sizeof(C)); memset(&PB, 0, sizeof(PB)); memset(&UP, 0, sizeof(UP));
    for (int e = 0; e < S; e++) {
        cf_segmenter* s = jobs[e].s;
        unary_args(U.m[e], s, jobs[e], P);
        C.m[e] = crf_seq(s, U.m[e].L);
    }
    if (late) seg_unary_kernel<kUnaryTrack><<<S, 1024, 0, st>>>(U);   // (+ the first marginals)
    else {
        seg_unary_kernel<kUnaryAll><<<S, 1024, 0, st>>>(U);
        for (int e = 0; e < S; e++) ensure_grid_kernel(jobs[e].s);
        launch_crf_kernel_matrix<6>(st, C, S, n, true);
    }
    const int flip = launch_mean_field(st, C, S, n, P->crfIterations, P->weightSmoothness, P->weightAppearance);
    for (int e = 0; e < S; e++) {
        cf_segmenter* s = jobs[e].s;
        const int n_models = jobs[e].n_models, L = label_count(n_models, jobs[e].allow_new);
        s->last_flip = flip; s->last_n = n_models; s->last_L = L;   // (cf_seg_buffer)
        SegPostArgsT<CAP>& p = PB.m[e];
        p.K = n; p.gx = s->gx; p.gy = s->gy; p.n_models = n_models; p.L = L; p.allow_new = jobs[e].allow_new ? 1 : 0;
        p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.next_id = jobs[e].next_model_id;
        p.minRelSizeNew = P->minRelSizeNew; p.maxRelSizeNew = P->maxRelSizeNew;
        for (int m = 0; m < n_models; m++) p.ids[m] = jobs[e].model_ids[m];
        if (jobs[e].allow_new) p.ids[n_models] = jobs[e].next_model_id;
        p.Q = flip ? s->Q1 : s->Q0; p.low_depth = s->low_mean; p.avg_conf = s->avg_conf; p.depth_range = s->depth_range;
        p.cc = s->cc; p.low_map = s->low_map; p.result = s->d_result;
        p.result_host = s->h_result; p.low_map_host = reinterpret_cast<unsigned*>(s->h_low_map);
        UP.m[e] = UpsampleArgs{s->labels, s->low_map, jobs[e].full_dev};
    }
    seg_post_kernel<CAP, N><<<S, 1024, 0, st>>>(PB);
    const int Npx = ctx->cfg.width * ctx->cfg.height;
    seg_upsample_kernel<<<dim3((Npx + 255) / 256, S), 256, 0, st>>>(UP, Npx);
    LAUNCHCHK(ctx);
#ifdef CF_ABLATE
    {
        static const int trace_call = getenv("CF_SEG_TRACE") ? atoi(getenv("CF_SEG_TRACE")) : -1;
        static int seen = 0;
        if (trace_call >= 0 && seen++ == trace_call) {
            HIPCHK(ctx, hipStreamSynchronize(st));
            unsigned long long h[2][16];
            HIPCHK(ctx, hipMemcpyFromSymbol(h, HIP_SYMBOL(g_seg_trace), sizeof(h)));
            const char* un[] = {"raw sums", "ordered lists", "empty superpixels", "depth range", "average confidence", "unaries + features", "zeroing"};
            const char* pn[] = {"arg-max + components", "roots numbered", "component statistics", "gates", "label map", "depth statistics", "publish"};
            for (int k = 0; k < 7; k++) fprintf(stderr, "[seg trace] unary %-22s %6lld ns\n", un[k], (long long)(h[0][k + 1] - h[0][k]) * 10);
            for (int k = 0; k < 7; k++) fprintf(stderr, "[seg trace] post  %-22s %6lld ns\n", pn[k], (long long)(h[1][k + 1] - h[1][k]) * 10);
            fprintf(stderr, "[seg trace] post  arg-max alone %6lld ns; component sweeps since the start: %lld\n", (long long)(h[1][8] - h[1][0]) * 10, (long long)h[1][9]);
            for (int k = 0; k < 3; k++)
                fprintf(stderr, "[seg trace] post  component sweep %d: hooks done at %6lld ns, walks done at %6lld ns (from the kernel's first stamp; stale if the sweep did not run)\n", k,
                        (long long)(h[1][10 + 2 * k] - h[1][0]) * 10, (long long)(h[1][11 + 2 * k] - h[1][0]) * 10);
        }
    }
#endif
    for (int e = 0; e < S; e++) {
        cf_segmenter* s = jobs[e].s;
        if (s->poses_published) {  // the tail now holds what the caller's all-reduce made of it; the next frame starts from zeros again
            HIPCHK(ctx, hipMemcpyAsync(s->h_pose_tail, pose_tail(s), sizeof(long long) * (size_t)s->Lcap * kPoseWords, hipMemcpyDeviceToHost, st));
        }
    }
    return CF_OK;
}

extern "C" {
// Only enqueues; the decisions arrive with cf_seg_fetch.
int cf_seg_infer(cf_segmenter* s, const cf_seg_params* P, const uint8_t* rgba, int n_models, const uint32_t* model_ids, uint32_t next_model_id,
                 int allow_new, uint8_t* full_dev)
{
    if (!s || !s->K || !P || !rgba || !model_ids || !full_dev || n_models <= 0) return CF_EINVAL;
    const int L = label_count(n_models, allow_new);
    if (int r = check_labels(s, L)) return r;
    SegJob job{};
    job.s = s; job.n_models = n_models; job.rgba = rgba; job.model_ids = model_ids; job.next_model_id = next_model_id; job.allow_new = allow_new; job.full_dev = full_dev;
    // the late half, when the early half ran with what this call would have given it; otherwise the whole chain
    bool late = false;
    if (s->early == 2) {
        late = s->early_n == n_models && s->early_rgba == rgba && s->early_scale[0] == P->scaleFeaturesRGB && s->early_scale[1] == P->scaleFeaturesDepth &&
               s->early_scale[2] == P->scaleFeaturesPos;
        if (!late) {
            // the ICP sums are in place; the frame's and the confidences' (consumed early) are formed again from the recorded images
            if (s->early_n != n_models) { s->ctx->set_error("cf_seg_infer: n_models differs from cf_seg_sums'"); return CF_EINVAL; }
            HIPCHK(s->ctx, hipMemsetAsync(s->spix_count, 0, sizeof(unsigned) * (size_t)s->K, s->ctx->stream));
            SegJob again{};
            again.s = s; again.depth = s->early_depth; again.n_models = n_models; again.vertconf4 = s->early_vconf.data();
            if (int r = enqueue_accumulate(s->ctx, &again, 1, kAccFrame | kAccConf)) return r;
        }
        s->early = 0;
    } else if (int r = early_discard(s)) return r;
    if (L <= 16) return enqueue_infer<17, kSegBatch>(s->ctx, P, &job, 1, late);
    return enqueue_infer<kMaxL + 1, 1>(s->ctx, P, &job, 1, late);
}

// The half of cf_seg_sums + cf_seg_infer that does not need the frame's tracking, for a caller that has another stream to put it on
// beside the tracking launches (behind cf_seg_slic): the frame's and the confidences' sums, their means / replay / depth range /
// average confidences / appearance features (seg_unary_kernel<kUnaryFrame>) and the appearance kernel matrix.  vertconf4[m] must hold
// what cf_seg_sums will be given (the previous frame's prediction), rgba and the three scaleFeatures* what cf_seg_infer will be given:
// the segmenter remembers them, and calls that match enqueue the late half only; calls that do not match fall back to the whole chain.
// An early half nobody finishes is dropped by the next cf_seg_early / cf_seg_sums / cf_seg_infer / cf_seg_run_batch.
int cf_seg_early(cf_segmenter* s, const float* depth, const uint8_t* rgba, int n_models, const float* const* vertconf4, const cf_seg_params* P)
{
    if (!s || !s->K || !depth || !rgba || !P || n_models <= 0 || n_models > s->Lcap || !vertconf4) return CF_EINVAL;
    cf_ctx* ctx = s->ctx;
    if (int r = early_discard(s)) return r;
    SegJob job{};
    job.s = s; job.depth = depth; job.n_models = n_models; job.vertconf4 = vertconf4; job.rgba = rgba;
    if (int r = enqueue_accumulate(ctx, &job, 1, kAccFrame | kAccConf)) return r;
    SegBatch<SegUnaryArgs> U;
    memset(&U, 0, sizeof(U));
    unary_args(U.m[0], s, job, P);
    seg_unary_kernel<kUnaryFrame><<<1, 1024, 0, ctx->stream>>>(U);
    ensure_grid_kernel(s);
    CrfBatch C;
    memset(&C, 0, sizeof(C));
    C.m[0] = crf_seq(s, 0);
    launch_crf_kernel_matrix<6>(ctx->stream, C, 1, s->K, false);
    LAUNCHCHK(ctx);
    s->early = 1; s->early_n = n_models; s->early_depth = depth; s->early_rgba = rgba;
    s->early_vconf.assign(vertconf4, vertconf4 + n_models);
    s->early_scale[0] = P->scaleFeaturesRGB; s->early_scale[1] = P->scaleFeaturesDepth; s->early_scale[2] = P->scaleFeaturesPos;
    return CF_OK;
}

// cf_seg_sums + cf_seg_infer of several segmenters of ONE context (the sequences of a lock-step group) through shared launches: the
// chain of ~30 launch-floor kernels is issued once per kSegBatch segmenters instead of once per segmenter.  Per segmenter the results
// are those of the two single calls, bit for bit; the decisions arrive with each segmenter's cf_seg_fetch.  No collective can sit between
// the sums and the inference here (single-process callers).
int cf_seg_run_batch(cf_ctx* ctx, const cf_seg_params* P, const cf_seg_job* jobs_in, int n_jobs)
{
    if (!ctx || !P || !jobs_in || n_jobs <= 0) return CF_EINVAL;
    std::vector<SegJob> jobs((size_t)n_jobs);
    bool batchable = true;
    for (int e = 0; e < n_jobs; e++) {
        const cf_seg_job& j = jobs_in[e];
        if (!j.seg || !j.seg->K || j.seg->ctx != ctx || !j.depth || !j.icp_err || !j.vertconf4 || !j.rgba || !j.model_ids || !j.full_dev || j.n_models <= 0) return CF_EINVAL;
        const int L = label_count(j.n_models, j.allow_new);
        if (int r = check_labels(j.seg, L)) return r;
        for (int k = 0; k < e; k++) if (jobs_in[k].seg == j.seg) return CF_EINVAL;
        batchable = batchable && L <= 16 && j.seg->K == jobs_in[0].seg->K && j.seg->gx == jobs_in[0].seg->gx;
        jobs[e] = SegJob{j.seg, j.depth, j.n_models, j.icp_err, j.vertconf4, j.rgba, j.model_ids, j.next_model_id, j.allow_new, j.full_dev};
        if (int r = early_discard(j.seg)) return r;   // (the batched chain is the whole chain)
    }
    if (!batchable) {  // (a sequence with more than 16 labels: one chain per segmenter)
        for (int e = 0; e < n_jobs; e++) {
            if (int r = enqueue_accumulate(ctx, &jobs[e], 1)) return r;
            if (int r = cf_seg_infer(jobs[e].s, P, jobs[e].rgba, jobs[e].n_models, jobs[e].model_ids, jobs[e].next_model_id, jobs[e].allow_new, jobs[e].full_dev)) return r;
        }
        return CF_OK;
    }
    for (int base = 0; base < n_jobs; base += kSegBatch) {
        const int S = n_jobs - base < kSegBatch ? n_jobs - base : kSegBatch;
        if (int r = enqueue_accumulate(ctx, &jobs[base], S)) return r;
        if (int r = enqueue_infer<17, kSegBatch>(ctx, P, &jobs[base], S)) return r;
    }
    return CF_OK;
}

// waits for the stream and hands out the decisions of the last cf_seg_infer (low_map_host: nullable [K])
int cf_seg_fetch(cf_segmenter* s, cf_seg_result* out, uint8_t* low_map_host)
{
    if (!s || !out) return CF_EINVAL;
    if (int r = cf_wait_stream(s->ctx)) return r;
    *out = *s->h_result;
    if (low_map_host && s->K) memcpy(low_map_host, s->h_low_map, (size_t)s->K);
    if (s->mask_pending) {  // the rows are those of a mask job (segment_masks.hip): its new mask value came with them
        s->mask_pending = false;
        s->mask_new_value = *s->h_mask_new;
        s->mask_value_valid = true;
    }
    return CF_OK;
}

int cf_seg_labels(cf_segmenter* s, void** dptr, uint64_t* bytes)
{
    if (!s || !dptr) return CF_EINVAL;
    *dptr = s->labels;
    if (bytes) *bytes = (uint64_t)s->ctx->cfg.width * s->ctx->cfg.height * 4;
    return CF_OK;
}

// Test access, read only: device views of what the chain holds between its stages (layouts and validity: include/cofusion_hip.h).
// Hands out addresses; the caller reads them in stream order (cf_memcpy_d2d_async on the context's stream).
int cf_seg_buffer(cf_segmenter* s, int which, void** dptr, uint64_t* bytes)
{
    if (!s || !dptr || !s->K) return CF_EINVAL;
    const uint64_t K = (uint64_t)s->K, Lc = (uint64_t)s->Lcap, n = (uint64_t)s->last_n, L = (uint64_t)s->last_L;
    void* p = nullptr; uint64_t b = 0;
    switch (which) {
    case 0: p = s->spix_count; b = K * 4; break;
    case 1: p = s->depth_count; b = K * 4; break;
    case 2: p = s->depth_sum; b = K * 8; break;
    case 3: p = s->icp_sum; b = Lc * K * 8; break;
    case 4: p = s->conf_sum; b = Lc * K * 8; break;
    case 5: p = s->low_mean; b = (1 + 2 * n) * K * 4; break;
    case 6: p = s->unary; b = K * L * 4; break;
    case 7: p = s->feat2; b = K * 6 * 4; break;
    case 8: p = s->avg_conf; b = n * 4; break;
    case 9: p = s->depth_range; b = 4; break;
    case 10: p = s->low_map; b = K; break;
    case 11: p = s->last_flip ? s->Q1 : s->Q0; b = K * L * 4; break;
    case 12: p = s->centres; b = K * 5 * 4; break;
    case 13: p = s->slic_sums; b = K * 6 * 8; break;
    case 14: p = s->resample; b = K * 4; break;
    default: s->ctx->set_error("cf_seg_buffer: no such buffer"); return CF_EINVAL;
    }
    *dptr = p;
    if (bytes) *bytes = b;
    return CF_OK;
}

}  // extern "C"
