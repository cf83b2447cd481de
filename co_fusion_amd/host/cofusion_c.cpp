// cofusion_c.cpp -- flat C wrapper (include/cofusion.h) around the C++ facade.
#include "../../include/cofusion.h"

#include <cstring>
#include <exception>
#include <iterator>
#include <string>
#include <vector>


#include "CoFusion.h"
#include "ImageIO.h"
#include "ImagePlayer.h"
#include "KlgIO.h"
#include "KlgPlayer.h"

namespace cofusion {   // Jpeg.cpp: the decoder split at the coefficient boundary
std::string jpegFront(const uint8_t* data, size_t size, int width, int height, cf_jpeg_header* hdr, int16_t* coef, size_t capBlocks, bool* refused);
void jpegFinishHost(const cf_jpeg_header* hdr, const int16_t* coef, uint8_t* rgb);
}
using namespace cofusion;

struct cofusion_handle { CoFusion* cf; bool borrowed = false; };  // borrowed: a sequence of a lock-step group (owned and stepped by the group)
struct cofusion_group { CoFusionGroup* g; std::vector<cofusion_handle> handles; };  // handles: borrowed views of the sequences
static thread_local std::string g_err;

#define GUARD(expr)                                  \
    try { expr; }                                    \
    catch (const std::exception& e) { g_err = e.what(); return -1; } \
    catch (...) { g_err = "unknown exception"; return -1; }

extern "C" {

void cofusion_default_config(cofusion_config* c)
{
    const CoFusion::Config d;
    c->width = d.width; c->height = d.height; c->fx = d.fx; c->fy = d.fy; c->cx = d.cx; c->cy = d.cy; c->device = d.device;
    c->max_surfels = d.maxSurfels; c->max_models = d.maxModels; c->conf_global_init = d.confGlobalInit;
    c->conf_object_init = d.confObjectInit; c->depth_cutoff = d.depthCutoff; c->icp_weight = d.icpWeight;
    c->outlier_coefficient = d.outlierCoefficient; c->fast_odom = d.fastOdom; c->so3 = d.so3; c->frame_to_frame_rgb = d.frameToFrameRGB;
    c->pyramid = d.pyramid; c->rgb_only = d.rgbOnly; c->model_spawn_offset = d.modelSpawnOffset;
    c->enable_multiple_models = d.enableMultipleModels;
    c->enable_pose_logging = d.enablePoseLogging;
    c->rank = d.rank; c->world = d.world;
    c->device_frames_complete = d.deviceFramesComplete;
    c->mid_frame_predict = d.midFramePredict;
    c->shard_background = d.shardBackground;
    c->enqueue_threads = d.enqueueThreads;
    c->colocate_background = d.colocateBackground;
    c->reloc = d.reloc;
    c->early_index_maps = d.earlyIndexMaps;
    c->time_delta = 0;   // (open loop: Config::timeDelta's default)
}

static CoFusion::Config to_config(const cofusion_config* c)
{
    CoFusion::Config d;
    d.width = c->width; d.height = c->height; d.fx = c->fx; d.fy = c->fy; d.cx = c->cx; d.cy = c->cy; d.device = c->device;
    d.maxSurfels = c->max_surfels; d.maxModels = c->max_models; d.confGlobalInit = c->conf_global_init;
    d.confObjectInit = c->conf_object_init; d.depthCutoff = c->depth_cutoff; d.icpWeight = c->icp_weight;
    d.outlierCoefficient = c->outlier_coefficient; d.fastOdom = c->fast_odom; d.so3 = c->so3; d.frameToFrameRGB = c->frame_to_frame_rgb;
    d.pyramid = c->pyramid; d.rgbOnly = c->rgb_only; d.modelSpawnOffset = c->model_spawn_offset;
    d.enableMultipleModels = c->enable_multiple_models;
    d.enablePoseLogging = c->enable_pose_logging != 0;
    d.rank = c->rank; d.world = c->world < 1 ? 1 : c->world;
    d.deviceFramesComplete = c->device_frames_complete != 0;
    d.midFramePredict = c->mid_frame_predict != 0;
    d.shardBackground = c->shard_background != 0;
    d.enqueueThreads = c->enqueue_threads < 0 ? 0 : c->enqueue_threads;
    d.colocateBackground = c->colocate_background != 0;
    d.reloc = c->reloc != 0;
    d.earlyIndexMaps = c->early_index_maps != 0;
    if (c->time_delta > 0) d.timeDelta = c->time_delta;
    return d;
}

int cofusion_create(const cofusion_config* c, cofusion_handle** out)
{
    if (!c || !out) { g_err = "null argument"; return -1; }
    const CoFusion::Config d = to_config(c);
    GUARD(*out = new cofusion_handle{new CoFusion(d)});
    return 0;
}
void cofusion_destroy(cofusion_handle* h)
{
    if (!h || h->borrowed) return;  // a group's sequence belongs to the group (cofusion_group_destroy)
    delete h->cf; delete h;
}
const char* cofusion_last_error(void) { return g_err.c_str(); }
int cofusion_set_stream(cofusion_handle* h, void* s) { return cf_set_stream(h->cf->context(), s); }

static int run_frame(cofusion_handle* h, const FrameData& f, const float* in_pose)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->borrowed) { g_err = "this handle is a sequence of a lock-step group: step it with cofusion_group_process_frames"; return -1; }
    Mat4f p;
    if (in_pose) for (int i = 0; i < 16; i++) p.m[i] = in_pose[i];
    GUARD(h->cf->processFrame(f, in_pose ? &p : nullptr));
    return 0;
}
int cofusion_process_frame(cofusion_handle* h, int64_t ts, const uint8_t* rgb, const float* depth, const uint8_t* mask, const float* in_pose)
{
    FrameData f; f.timestamp = ts; f.rgb = rgb; f.depth = depth; f.mask = mask;
    return run_frame(h, f, in_pose);
}
int cofusion_process_frame_device(cofusion_handle* h, int64_t ts, const float* depth_dev, const uint8_t* rgba_dev, const float* in_pose)
{
    FrameData f; f.timestamp = ts; f.depth_dev = depth_dev; f.rgba_dev = rgba_dev;
    return run_frame(h, f, in_pose);
}
// ... with the frame's label mask in device memory as well: the mask branch of the segmentation runs as kernels (csrc/segment_masks.hip)
int cofusion_process_frame_device_masked(cofusion_handle* h, int64_t ts, const float* depth_dev, const uint8_t* rgba_dev, const uint8_t* mask_dev,
                                         const float* in_pose)
{
    if (h && mask_dev && h->cf->cfg.world > 1) { g_err = "device masks are a single-GPU option (world == 1): pass the mask from the host (cofusion_process_frame)"; return -1; }
    FrameData f; f.timestamp = ts; f.depth_dev = depth_dev; f.rgba_dev = rgba_dev; f.mask_dev = mask_dev;
    return run_frame(h, f, in_pose);
}
int cofusion_num_models(cofusion_handle* h) { return (int)h->cf->getModels().size(); }
int cofusion_tick(cofusion_handle* h) { return h->cf->getTick(); }
int cofusion_is_lost(cofusion_handle* h) { return h && h->cf->getLost() ? 1 : 0; }
int cofusion_set_relocalisation(cofusion_handle* h, int on, int n_ferns, float fern_threshold, float photo_threshold, int min_age, uint64_t seed, int capacity)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->borrowed) { g_err = "relocalisation is not available for a sequence of a lock-step group"; return -1; }
    GUARD(h->cf->setRelocalisation(on != 0, n_ferns > 0 ? n_ferns : 500, fern_threshold,
                                   photo_threshold > 0 ? photo_threshold : 115.0f, min_age >= 0 ? min_age : 300, seed, capacity > 0 ? capacity : 1024));
    return 0;
}
int cofusion_set_redetection(cofusion_handle* h, int on, float min_fit, float min_cover, float depth_tol, int max_candidates, int keep_min_surfels,
                             float keep_conf_threshold)
{
    if (!h) { g_err = "null handle"; return -1; }
    GUARD(h->cf->setRedetection(on != 0, min_fit >= 0 ? min_fit : 0.5f, min_cover >= 0 ? min_cover : 0.044f, depth_tol >= 0 ? depth_tol : 0.10f,
                                max_candidates > 0 ? max_candidates : 8, keep_min_surfels >= 0 ? (unsigned)keep_min_surfels : 4000u,
                                keep_conf_threshold >= 0 ? keep_conf_threshold : 0.3f));
    return 0;
}
int cofusion_redetect_stats(cofusion_handle* h, int* attempts, int* reactivations, int* last_id)
{
    if (!h) { g_err = "null handle"; return -1; }
    const CoFusion::RedetectStats& s = h->cf->redetectStats();
    if (attempts) *attempts = s.attempts;
    if (reactivations) *reactivations = s.reactivations;
    if (last_id) *last_id = s.lastId;
    return 0;
}
int cofusion_redetect_last(cofusion_handle* h, cofusion_redetect_candidate* out, int capacity, int* n, uint32_t* label_pixels, int* winner)
{
    if (!h || !n) { g_err = "cofusion_redetect_last: bad arguments"; return -1; }
    const std::vector<CoFusion::RedetectCandidate>& c = h->cf->redetectLast(label_pixels, winner);
    *n = (int)c.size();
    for (int k = 0; out && k < capacity && k < (int)c.size(); k++) {
        const cf_redetect_counts& q = c[(size_t)k].counts;
        out[k] = cofusion_redetect_candidate{c[(size_t)k].id, q.projected, q.occluded, q.seen_through, q.agree, q.agree_on_label, q.covered,
                                             c[(size_t)k].fit, c[(size_t)k].cover, c[(size_t)k].eligible ? 1 : 0};
    }
    return 0;
}
int cofusion_set_redetection_search(cofusion_handle* h, int on, int iterations, float min_colour, int max_registered)
{
    if (!h) { g_err = "null handle"; return -1; }
    GUARD(h->cf->setRedetectionSearch(on != 0, iterations > 0 ? iterations : 10, min_colour >= 0 ? min_colour : CoFusion::kRedetectMinColour,
                                      max_registered > 0 ? max_registered : 2));
    return 0;
}
int cofusion_redetect_search_last(cofusion_handle* h, cofusion_redetect_search_candidate* out, int capacity, int* n, int* winner, int* attempts)
{
    if (!h || !n) { g_err = "cofusion_redetect_search_last: bad arguments"; return -1; }
    const std::vector<CoFusion::RedetectSearchCandidate>& c = h->cf->redetectSearchLast(winner, attempts);
    *n = (int)c.size();
    for (int k = 0; out && k < capacity && k < (int)c.size(); k++) {
        const CoFusion::RedetectSearchCandidate& r = c[(size_t)k];
        const cf_redetect_counts& q = r.counts;
        out[k] = cofusion_redetect_search_candidate{r.id, r.colour, r.registered ? 1 : 0, r.converged ? 1 : 0, r.iterations, r.firstInliers, r.lastInliers,
                                                    r.rms, r.moved, q.projected, q.occluded, q.seen_through, q.agree, q.agree_on_label, q.covered,
                                                    r.fit, r.cover, r.eligible ? 1 : 0};
    }
    return 0;
}
int cofusion_num_inactive_models(cofusion_handle* h) { return h ? (int)h->cf->numInactiveModels() : -1; }
int cofusion_reloc_stats(cofusion_handle* h, int* keyframes, int* last_closest, int* recoveries, int* database_full)
{
    if (!h) { g_err = "null handle"; return -1; }
    GUARD(h->cf->relocStats(keyframes, last_closest, recoveries, database_full));
    return 0;
}

int cofusion_deform_background(cofusion_handle* h, const float* src, const float* dst, const float* src_time, const float* dst_time, int n, int pin,
                               int sample_rate, void* result, int* nodes)
{
    if (!h) { g_err = "null handle"; return -1; }
    int got = 0;
    GUARD(got = h->cf->deformBackground(src, dst, src_time, dst_time, n, pin != 0, sample_rate, static_cast<cf_deform_result*>(result)));
    if (nodes) *nodes = got;
    return 0;
}
int cofusion_set_loop_closure(cofusion_handle* h, int on, int sample_rate)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->borrowed) { g_err = "loop closure is not available for a sequence of a lock-step group"; return -1; }
    GUARD(h->cf->setLoopClosure(on != 0, sample_rate > 0 ? sample_rate : 25000));
    return 0;
}
int cofusion_loop_stats(cofusion_handle* h, cofusion_loop_stats_t* out)
{
    if (!h || !out) { g_err = "cofusion_loop_stats: bad arguments"; return -1; }
    const CoFusion::LoopStats& s = h->cf->loopStats();
    *out = cofusion_loop_stats_t{s.gated, s.candidates, s.fernAccepts, s.optimised, s.accepted, s.failed, s.lastKeyframe, s.lastKeyframeTime, s.lastNodes, s.lastTick, {}};
    static_assert(sizeof(s.last) == sizeof(out->last_result), "cf_deform_result is 8 words");
    memcpy(out->last_result, &s.last, sizeof(out->last_result));
    return 0;
}

int cofusion_set_local_loop_closure(cofusion_handle* h, int on, int sample_rate, int icp_count_thresh, float icp_err_thresh, float cov_thresh,
                                    int min_inactive_pixels)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->borrowed) { g_err = "local loop closure is not available for a sequence of a lock-step group"; return -1; }
    GUARD(h->cf->setLocalLoopClosure(on != 0, sample_rate > 0 ? sample_rate : 5000, icp_count_thresh >= 0 ? icp_count_thresh : 40000,
                                     icp_err_thresh > 0 ? icp_err_thresh : 5e-5f, cov_thresh > 0 ? cov_thresh : 1e-5f, min_inactive_pixels));
    return 0;
}
int cofusion_local_loop_stats(cofusion_handle* h, cofusion_local_loop_stats_t* out)
{
    if (!h || !out) { g_err = "cofusion_local_loop_stats: bad arguments"; return -1; }
    const CoFusion::LocalLoopStats& s = h->cf->localLoopStats();
    *out = cofusion_local_loop_stats_t{};
    out->examined = s.examined; out->skipped_by_gate = s.skippedByGate; out->tracker_accepts = s.trackerAccepts;
    out->optimised = s.optimised; out->accepted = s.accepted; out->failed = s.failed;
    out->last_nodes = s.lastNodes; out->last_constraints = s.lastConstraints; out->last_pinned = s.lastPinned; out->last_tick = s.lastTick;
    out->deforms = s.deforms; out->last_deform_time = s.lastDeformTime; out->last_covered = s.lastCovered;
    out->last_tracker_accepted = s.lastRecord.accepted; out->last_icp_error = s.lastRecord.icp_error; out->last_icp_count = s.lastRecord.icp_count;
    out->last_max_covariance = s.lastRecord.max_covariance;
    memcpy(out->last_est_pose, s.lastRecord.est_pose, sizeof(out->last_est_pose));
    static_assert(sizeof(s.last) == sizeof(out->last_result), "cf_deform_result is 8 words");
    memcpy(out->last_result, &s.last, sizeof(out->last_result));
    return 0;
}

int cofusion_set_relative_constraints(cofusion_handle* h, int on)
{
    if (!h) { g_err = "null handle"; return -1; }
    if (h->borrowed) { g_err = "relative constraints are not available for a sequence of a lock-step group"; return -1; }
    GUARD(h->cf->setRelativeConstraints(on != 0));
    return 0;
}
int cofusion_add_relative_constraints(cofusion_handle* h, const float* src, const float* dst, const float* src_time, const float* dst_time, int n)
{
    if (!h) { g_err = "null handle"; return -1; }
    GUARD(h->cf->addRelativeConstraints(src, dst, src_time, dst_time, n));
    return 0;
}
int cofusion_relative_constraints(cofusion_handle* h, float* out, int capacity, int* n)
{
    if (!h || !n) { g_err = "cofusion_relative_constraints: bad arguments"; return -1; }
    GUARD(*n = h->cf->relativeConstraints(out, capacity));
    return 0;
}
int cofusion_local_closure_download(cofusion_handle* h, int* found, int* rows, int* pinned, int* last_deform_time, float* src, float* dst, float* time,
                                    float* target_time, int row_capacity, int* nodes, float* node_pos, float* params, int node_capacity)
{
    if (!h || !found) { g_err = "cofusion_local_closure_download: bad arguments"; return -1; }
    GUARD(*found = h->cf->localClosureDownload(rows, pinned, last_deform_time, src, dst, time, target_time, row_capacity, nodes, node_pos, params,
                                               node_capacity) ? 1 : 0);
    return 0;
}
int cofusion_relative_stats(cofusion_handle* h, cofusion_relative_stats_t* out)
{
    if (!h || !out) { g_err = "cofusion_relative_stats: bad arguments"; return -1; }
    CoFusion::RelativeStats s;
    GUARD(s = h->cf->relativeStats());
    *out = cofusion_relative_stats_t{s.appended, s.overwritten, s.stored, s.usedByLastClosure, s.lastPicked, 0};
    return 0;
}

static Model* model_at(cofusion_handle* h, int index)
{
    auto& l = h->cf->getModels();
    if (index < 0 || index >= (int)l.size()) return nullptr;
    auto it = l.begin();
    std::advance(it, index);
    return it->get();
}
int cofusion_model_info(cofusion_handle* h, int index, unsigned* id, unsigned* count, float pose[16], float* conf)
{
    Model* m = model_at(h, index);
    if (!m) { g_err = "model index out of range"; return -1; }
    if (id) *id = m->getID();
    if (count) *count = m->lastCount();
    if (pose) for (int i = 0; i < 16; i++) pose[i] = m->getPose().m[i];
    if (conf) *conf = m->getConfidenceThreshold();
    return 0;
}
int cofusion_model_download(cofusion_handle* h, int index, float* surfels, uint32_t capacity, uint32_t* count)
{
    Model* m = model_at(h, index);
    if (!m) { g_err = "model index out of range"; return -1; }
    if (!m->isOwned()) { if (count) *count = 0; return 0; }
    return cf_model_download_map(m->handle(), surfels, capacity, count);
}
int cofusion_model_icp_stats(cofusion_handle* h, int index, float* err, float* cnt)
{
    Model* m = model_at(h, index);
    if (!m) { g_err = "model index out of range"; return -1; }
    if (err) *err = m->lastStats.last_icp_error;
    if (cnt) *cnt = m->lastStats.last_icp_count;
    return 0;
}
int cofusion_model_cull_box(cofusion_handle* h, int index, int box[4])
{
    Model* m = model_at(h, index);
    if (!m || !box) { g_err = "model index out of range"; return -1; }
    for (int k = 0; k < 4; k++) box[k] = m->lastStats.cull_box[k];
    return 0;
}
int cofusion_model_level0_visited(cofusion_handle* h, int index, uint64_t* icp_pixels, uint64_t* residual_pixels)
{
    Model* m = model_at(h, index);
    if (!m || !m->getFrameOdometry()) { g_err = "model index out of range"; return -1; }
    if (cf_odom_level0_visited(m->getFrameOdometry(), icp_pixels, residual_pixels)) { g_err = "cf_odom_level0_visited"; return -1; }
    return 0;
}
int cofusion_model_tracking_inputs(cofusion_handle* h, int index, float* vertex4, float* normal4, uint8_t* image_rgba)
{
    Model* m = model_at(h, index);
    if (!m) { g_err = "model index out of range"; return -1; }
    if (!m->isOwned()) { g_err = "model is a shadow on this rank"; return -1; }
    const float* v; const float* n; const uint8_t* img;
    GUARD(m->trackingInputs(m->requiresFillIn(), h->cf->cfg.frameToFrameRGB, v, n, img));
    cf_ctx* ctx = h->cf->context();
    const uint64_t N = (uint64_t)h->cf->cfg.width * h->cf->cfg.height;
    if (vertex4 && cf_memcpy_d2h(ctx, vertex4, v, N * 16)) { g_err = cf_last_error(ctx); return -1; }
    if (normal4 && cf_memcpy_d2h(ctx, normal4, n, N * 16)) { g_err = cf_last_error(ctx); return -1; }
    if (image_rgba && cf_memcpy_d2h(ctx, image_rgba, img, N * 4)) { g_err = cf_last_error(ctx); return -1; }
    return 0;
}
const uint8_t* cofusion_mask_device(cofusion_handle* h) { return h->cf->maskDevice(); }
void* cofusion_context(cofusion_handle* h) { return h->cf->context(); }
int cofusion_set_crf(cofusion_handle* h, float uwe, float uke, float thn, float wa, float ws, float srgb, float sdepth, float spos, float minr,
                     float maxr, unsigned its)
{
    Segmentation& s = h->cf->segmentation();
    s.unaryWeightError = uwe; s.unaryKError = uke; s.unaryThresholdNew = thn; s.weightAppearance = wa; s.weightSmoothness = ws;
    s.scaleFeaturesRGB = 1.0f / srgb; s.scaleFeaturesDepth = 1.0f / sdepth; s.scaleFeaturesPos = 1.0f / spos;
    s.minRelSizeNew = minr; s.maxRelSizeNew = maxr; s.crfIterations = its;
    return 0;
}
int cofusion_set_seg_early(cofusion_handle* h, int on)
{
    if (!h) { g_err = "null argument"; return -1; }
    h->cf->setSegEarly(on != 0);
    return 0;
}

int cofusion_set_allreduce(cofusion_handle* h, cofusion_allreduce_i64_fn fn, void* user)
{
    h->cf->setAllreduce(fn, user);
    return 0;
}
int cofusion_set_allreduce_device(cofusion_handle* h, cofusion_allreduce_dev_fn fn, void* user)
{
    h->cf->setAllreduceDevice(fn, user);
    return 0;
}
// ---- lock-step group of sequences on one GPU (CoFusionGroup) ----
int cofusion_group_create(const cofusion_config* c, int sequences, cofusion_group** out)
{
    if (!c || !out) { g_err = "null argument"; return -1; }
    const CoFusion::Config d = to_config(c);
    try {
        cofusion_group* g = new cofusion_group{new CoFusionGroup(d, sequences), std::vector<cofusion_handle>()};
        for (int s = 0; s < sequences; s++) g->handles.push_back(cofusion_handle{&g->g->sequence(s), true});
        *out = g;
    }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
    catch (...) { g_err = "unknown exception"; return -1; }
    return 0;
}
void cofusion_group_destroy(cofusion_group* g) { if (g) { delete g->g; delete g; } }
int cofusion_group_size(cofusion_group* g) { return g ? g->g->size() : 0; }
cofusion_handle* cofusion_group_sequence(cofusion_group* g, int s)
{
    if (!g || s < 0 || s >= g->g->size()) { g_err = "sequence index out of range"; return nullptr; }
    return &g->handles[(size_t)s];
}
int cofusion_group_set_stream(cofusion_group* g, void* s) { return g ? cf_set_stream(g->g->context(), s) : -1; }
int cofusion_group_process_frames(cofusion_group* g, const int64_t* ts, const uint8_t* const* rgb, const float* const* depth, const uint8_t* const* mask)
{
    if (!g || !rgb || !depth) { g_err = "null argument"; return -1; }
    std::vector<FrameData> f((size_t)g->g->size());
    for (size_t s = 0; s < f.size(); s++) { f[s].timestamp = ts ? ts[s] : 0; f[s].rgb = rgb[s]; f[s].depth = depth[s]; f[s].mask = mask ? mask[s] : nullptr; }
    GUARD(g->g->processFrames(f.data()));
    return 0;
}
int cofusion_group_process_frames_device(cofusion_group* g, const int64_t* ts, const float* const* depth_dev, const uint8_t* const* rgba_dev)
{
    if (!g || !rgba_dev || !depth_dev) { g_err = "null argument"; return -1; }
    std::vector<FrameData> f((size_t)g->g->size());
    for (size_t s = 0; s < f.size(); s++) { f[s].timestamp = ts ? ts[s] : 0; f[s].depth_dev = depth_dev[s]; f[s].rgba_dev = rgba_dev[s]; }
    GUARD(g->g->processFrames(f.data()));
    return 0;
}

int cofusion_group_process_frames_device_masked(cofusion_group* g, const int64_t* ts, const float* const* depth_dev, const uint8_t* const* rgba_dev,
                                                const uint8_t* const* mask_dev)
{
    if (!g || !rgba_dev || !depth_dev) { g_err = "null argument"; return -1; }
    std::vector<FrameData> f((size_t)g->g->size());
    for (size_t s = 0; s < f.size(); s++) {
        f[s].timestamp = ts ? ts[s] : 0; f[s].depth_dev = depth_dev[s]; f[s].rgba_dev = rgba_dev[s];
        f[s].mask_dev = mask_dev ? mask_dev[s] : nullptr;   // (a null entry: that sequence runs the motion segmentation as before)
    }
    GUARD(g->g->processFrames(f.data()));
    return 0;
}

int cofusion_rccl_unique_id(void* id128)
{
    // (creating the id needs no context: rank 0 calls this before any instance exists.  Forwarded to the C-ABI library, the only one
    // of the two that links RCCL)
    if (!id128) { g_err = "null id buffer"; return -1; }
    if (cf_rccl_unique_id(id128) != CF_OK) { g_err = "cf_rccl_unique_id (ncclGetUniqueId) failed"; return -1; }
    return 0;
}
int cofusion_init_rccl(cofusion_handle* h, const void* id128)
{
    if (!h || !id128) { g_err = "null argument"; return -1; }
    GUARD(h->cf->initRccl(id128));
    return 0;
}
int cofusion_broadcast(cofusion_handle* h, void* dev_buf, uint64_t bytes, int root)
{
    if (!h || !dev_buf) { g_err = "null argument"; return -1; }
    GUARD(h->cf->broadcast(dev_buf, bytes, root));
    return 0;
}
int cofusion_model_owned(cofusion_handle* h, int index)
{
    Model* m = model_at(h, index);
    if (!m) { g_err = "model index out of range"; return -1; }
    return m->isOwned() ? 1 : 0;
}
/* diagnostics: host wall-clock per processFrame phase of the calling thread (PhaseTimes order), frames counted */
int cofusion_debug_phase_ms(double* out, int n, long* frames, int reset)
{
    PhaseTimes& t = phaseTimes();
    for (int i = 0; i < n && i < PhaseTimes::Count; i++) out[i] = t.ms[i];
    if (frames) *frames = t.frames;
    if (reset) t = PhaseTimes();
    return PhaseTimes::Count;
}
int cofusion_set_export_segmentation(cofusion_handle* h, const char* prefix)
{
    h->cf->setExportSegmentation(prefix ? prefix : "");
    return 0;
}
int cofusion_render_device(cofusion_handle* h, const cf_render_view* view, int background_mode, int object_mode, int flags,
                           const uint8_t** rgba, const float** depth, const uint8_t** labels)
{
    if (!h) { g_err = "cofusion_render: no instance"; return -1; }
    GUARD(h->cf->renderSceneOwned(view, background_mode, object_mode, flags, rgba, depth, labels, nullptr, nullptr));
    return 0;
}
int cofusion_render(cofusion_handle* h, const cf_render_view* view, int background_mode, int object_mode, int flags, uint8_t* rgba,
                    float* depth, uint8_t* labels)
{
    const uint8_t* r = nullptr; const float* d = nullptr; const uint8_t* l = nullptr;
    if (int rc = cofusion_render_device(h, view, background_mode, object_mode, flags, &r, &d, &l)) return rc;
    cf_ctx* ctx = h->cf->context();
    const uint64_t N = view ? (uint64_t)view->width * view->height : (uint64_t)h->cf->cfg.width * h->cf->cfg.height;
    if (rgba && cf_memcpy_d2h(ctx, rgba, r, N * 4)) { g_err = cf_last_error(ctx); return -1; }
    if (depth && cf_memcpy_d2h(ctx, depth, d, N * 4)) { g_err = cf_last_error(ctx); return -1; }
    if (labels && cf_memcpy_d2h(ctx, labels, l, N)) { g_err = cf_last_error(ctx); return -1; }
    return 0;
}
int cofusion_set_export_views(cofusion_handle* h, const char* prefix, int which)
{
    if (!h) { g_err = "cofusion_set_export_views: no instance"; return -1; }
    GUARD(h->cf->setExportViews(prefix ? prefix : "", which));
    return 0;
}
int cofusion_set_export_async(cofusion_handle* h, int on, int workers, int slots)
{
    if (!h) { g_err = "cofusion_set_export_async: no instance"; return -1; }
    GUARD(h->cf->setExportAsync(on != 0, workers, slots));
    return 0;
}
int cofusion_export_flush(cofusion_handle* h)
{
    if (!h) { g_err = "cofusion_export_flush: no instance"; return -1; }
    GUARD(h->cf->exportFlush());
    return 0;
}
int cofusion_export_stats(cofusion_handle* h, uint64_t* images, uint64_t* bytes, uint64_t* stalls, double* device_ms, uint64_t* device_images, int timing)
{
    if (!h) { g_err = "cofusion_export_stats: no instance"; return -1; }
    GUARD(h->cf->exportStats(images, bytes, stalls, device_ms, device_images, timing != 0));
    return 0;
}
int cofusion_save_ply(cofusion_handle* h, const char* prefix)
{
    try { const int n = h->cf->savePly(prefix ? prefix : ""); if (n < 0) g_err = "savePly: cannot write"; return n; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int cofusion_save_mesh(cofusion_handle* h, const char* prefix, float voxel)
{
    if (!h) { g_err = "cofusion_save_mesh: no instance"; return -1; }
    try { const int n = h->cf->saveMesh(prefix ? prefix : "", voxel); if (n < 0) g_err = "saveMesh: cannot write"; return n; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int cofusion_model_mesh(cofusion_handle* h, int index, float voxel, uint32_t* n_vertices, uint32_t* n_triangles, cf_mesh_vertex* vertices,
                        uint32_t vertex_capacity, uint32_t* triangles, uint32_t triangle_capacity, float transform[16])
{
    if (!h || !n_vertices || !n_triangles) { g_err = "cofusion_model_mesh: bad arguments"; return -1; }
    Model* m = h->cf->meshModel(index);
    if (!m) { g_err = "model index out of range"; return -1; }
    const bool copy = vertices || triangles;
    // counts first: a call without arrays extracts and keeps the mesh; a call with arrays copies the kept one (or extracts, if none fits)
    GUARD(if (!copy || !h->cf->keptMesh(index, voxel, n_vertices, n_triangles)) h->cf->extractMesh(index, voxel, n_vertices, n_triangles));
    if (transform) { const Mat4f T = h->cf->meshTransform(*m); for (int i = 0; i < 16; i++) transform[i] = T.m[i]; }
    if (!copy || (*n_vertices == 0 && *n_triangles == 0)) return 0;
    if (!vertices || !triangles || vertex_capacity < *n_vertices || triangle_capacity < *n_triangles) { g_err = "cofusion_model_mesh: arrays too small"; return -1; }
    GUARD(h->cf->downloadMesh(vertices, triangles));
    return 0;
}
int cofusion_set_mesh_max_voxels(cofusion_handle* h, uint64_t max_voxels)
{
    if (!h) { g_err = "cofusion_set_mesh_max_voxels: no instance"; return -1; }
    GUARD(h->cf->setMeshMaxVoxels(max_voxels));
    return 0;
}
int cofusion_write_mesh_ply(const char* path, const cf_mesh_vertex* vertices, uint32_t n_vertices, const uint32_t* triangles, uint32_t n_triangles)
{
    if (!path) { g_err = "cofusion_write_mesh_ply: no path"; return -1; }
    if (!writeMeshPly(path, vertices, n_vertices, triangles, n_triangles)) { g_err = std::string("cannot write ") + path; return -1; }
    return 0;
}
int cofusion_export_poses(cofusion_handle* h, const char* prefix)
{
    try { const int n = h->cf->exportPoses(prefix ? prefix : ""); if (n < 0) g_err = "exportPoses: cannot write"; return n; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}

struct cofusion_klg_reader { KlgLogReader r; cofusion_klg_reader(const char* f, int w, int hh, bool fl) : r(f, w, hh, fl) {} };
struct cofusion_klg_writer { KlgLogWriter w; cofusion_klg_writer(const char* f, int ww, int hh, bool c) : w(f, ww, hh, c) {} };
int cofusion_klg_open(const char* file, int width, int height, int flip, cofusion_klg_reader** out, int* num_frames)
{
    if (!file || !out || width <= 0 || height <= 0) { g_err = "cofusion_klg_open: bad arguments"; return -1; }
    auto* r = new cofusion_klg_reader(file, width, height, flip != 0);
    if (!r->r.ok()) { g_err = r->r.error(); delete r; return -1; }
    if (num_frames) *num_frames = r->r.getNumFrames();
    *out = r;
    return 0;
}
int cofusion_klg_next(cofusion_klg_reader* r, int64_t* ts, float* depth_m, uint8_t* rgb)
{
    if (!r) return -1;
    if (!r->r.hasMore()) return 1;  // end of log
    if (!r->r.getNext()) { g_err = r->r.error(); return -1; }
    if (ts) *ts = r->r.timestamp;
    if (depth_m) memcpy(depth_m, r->r.depth.data(), r->r.depth.size() * sizeof(float));
    if (rgb) memcpy(rgb, r->r.rgb.data(), r->r.rgb.size());
    return 0;
}
int cofusion_klg_set_reference_compatible(cofusion_klg_reader* r, int on) { if (!r) return -1; r->r.referenceCompatible = on != 0; return 0; }
void cofusion_klg_close(cofusion_klg_reader* r) { delete r; }
int cofusion_klg_create(const char* file, int width, int height, int compress_depth, cofusion_klg_writer** out)
{
    if (!file || !out || width <= 0 || height <= 0) { g_err = "cofusion_klg_create: bad arguments"; return -1; }
    auto* w = new cofusion_klg_writer(file, width, height, compress_depth != 0);
    if (!w->w.ok()) { g_err = std::string("cannot create ") + file; delete w; return -1; }
    *out = w;
    return 0;
}
int cofusion_klg_write(cofusion_klg_writer* w, int64_t ts, const float* depth_m, const uint8_t* rgb)
{
    if (!w || !depth_m) return -1;
    if (!w->w.write(ts, depth_m, rgb)) { g_err = "klg write failed"; return -1; }
    return 0;
}
int cofusion_klg_finish(cofusion_klg_writer* w) { if (!w) return -1; w->w.close(); delete w; return 0; }

// ---- .klg log player (KlgPlayer.h) ----
struct cofusion_klg_player { KlgPlayer p; cofusion_klg_player(CoFusion& cf, const char* f, bool fl, int w) : p(cf, f, fl, w) {} };
int cofusion_klg_player_open(cofusion_handle* h, const char* file, int flip, int workers, cofusion_klg_player** out, int* num_frames)
{
    if (!h || !file || !out) { g_err = "cofusion_klg_player_open: bad arguments"; return -1; }
    if (h->borrowed) { g_err = "the log player is not available for a sequence of a lock-step group"; return -1; }
    GUARD(*out = new cofusion_klg_player(*h->cf, file, flip != 0, workers > 0 ? workers : 4));
    if (num_frames) *num_frames = (*out)->p.getNumFrames();
    return 0;
}
int cofusion_klg_player_next(cofusion_klg_player* p, int64_t* ts, const float** depth_dev, const uint8_t** rgba_dev)
{
    if (!p) { g_err = "null player"; return -1; }
    bool more = false;
    GUARD(more = p->p.next(ts, depth_dev, rgba_dev));
    return more ? 0 : 1;
}
int cofusion_klg_player_process(cofusion_klg_player* p)
{
    if (!p) { g_err = "null player"; return -1; }
    bool more = false;
    GUARD(more = p->p.process());
    return more ? 0 : 1;
}
int cofusion_klg_player_rewind(cofusion_klg_player* p)
{
    if (!p) { g_err = "null player"; return -1; }
    GUARD(p->p.rewind());
    return 0;
}
int cofusion_klg_player_set_limits(cofusion_klg_player* p, int reference_compatible, int frame_limit)
{
    if (!p) { g_err = "null player"; return -1; }
    p->p.setLimits(reference_compatible != 0, frame_limit);
    return 0;
}
void cofusion_klg_player_close(cofusion_klg_player* p) { delete p; }

// ---- test access: the JPEG split and the prefetcher alone (no GPU) ----
int cofusion_jpeg_front(const uint8_t* stream, uint64_t size, int width, int height, cf_jpeg_header* header, int16_t* coef, uint64_t coef_blocks)
{
    if (!stream || !header || !coef || width <= 0 || height <= 0) { g_err = "cofusion_jpeg_front: bad arguments"; return -1; }
    bool refused = false;
    const std::string e = jpegFront(stream, (size_t)size, width, height, header, coef, (size_t)coef_blocks, &refused);
    if (!e.empty()) { g_err = e; return -1; }
    return refused ? 1 : 0;
}
int cofusion_jpeg_finish_host(const cf_jpeg_header* header, const int16_t* coef, uint8_t* rgb)
{
    if (!header || !coef || !rgb) { g_err = "cofusion_jpeg_finish_host: bad arguments"; return -1; }
    jpegFinishHost(header, coef, rgb);
    return 0;
}
struct cofusion_klg_prefetcher {
    std::vector<std::vector<uint8_t>> store;
    std::vector<cf_frame_slot> mem;
    KlgPrefetcher* p = nullptr;
    int held = -1;
    ~cofusion_klg_prefetcher() { delete p; }
};
int cofusion_klg_prefetch_open(const char* file, int width, int height, int workers, int slots, cofusion_klg_prefetcher** out, int* num_frames)
{
    if (!file || !out || width <= 0 || height <= 0 || slots < 2 || slots > 64) { g_err = "cofusion_klg_prefetch_open: bad arguments"; return -1; }
    auto* q = new cofusion_klg_prefetcher();
    const size_t N = (size_t)width * height, blocks = (size_t)CF_JPEG_MAX_BLOCKS(width, height);
    const size_t offCoef = 512, offDepth = offCoef + blocks * 128, offRgb = offDepth + ((N * 2 + 15) & ~(size_t)15);
    for (int s = 0; s < slots; s++) {
        q->store.emplace_back(offRgb + N * 3);
        uint8_t* b = q->store.back().data();
        q->mem.push_back(cf_frame_slot{reinterpret_cast<cf_jpeg_header*>(b), reinterpret_cast<int16_t*>(b + offCoef), blocks,
                                       reinterpret_cast<uint16_t*>(b + offDepth), b + offRgb});
    }
    q->p = new KlgPrefetcher(file, width, height, q->mem, workers > 0 ? workers : 4);
    if (!q->p->ok()) { g_err = q->p->error(); delete q; return -1; }
    if (num_frames) *num_frames = q->p->getNumFrames();
    *out = q;
    return 0;
}
int cofusion_klg_prefetch_next(cofusion_klg_prefetcher* q, int64_t* ts, int* color_kind, cf_frame_slot* slot)
{
    if (!q) { g_err = "null prefetcher"; return -1; }
    if (q->held >= 0) { q->p->release(q->held); q->held = -1; }
    if (!q->p->hasMore()) return 1;
    KlgFrame f;
    if (!q->p->next(&f)) { g_err = q->p->error(); return -1; }
    q->held = f.slot;
    if (ts) *ts = f.timestamp;
    if (color_kind) *color_kind = f.colorKind;
    if (slot) *slot = q->mem[(size_t)f.slot];
    return 0;
}
int cofusion_klg_prefetch_rewind(cofusion_klg_prefetcher* q) { if (!q) return -1; q->held = -1; q->p->rewind(); return 0; }
void cofusion_klg_prefetch_close(cofusion_klg_prefetcher* q) { delete q; }

// ---- image-sequence datasets: the serial reader and the parsers alone (no GPU) ----
struct cofusion_image_reader {
    imageio::ImageSequenceReader r;
    explicit cofusion_image_reader(const imageio::SequenceOptions& o) : r(o) {}
};
static imageio::SequenceOptions image_options(const cofusion_image_options* o)
{
    imageio::SequenceOptions s;
    auto str = [](const char* c) { return std::string(c ? c : ""); };
    s.colorDir = str(o->color_dir); s.depthDir = str(o->depth_dir); s.maskDir = str(o->mask_dir);
    s.colorPrefix = str(o->color_prefix); s.depthPrefix = str(o->depth_prefix); s.maskPrefix = str(o->mask_prefix);
    s.indexWidth = o->index_width > 0 ? o->index_width : 4;
    s.startIndex = o->start_index;
    s.flipColors = o->flip_colors != 0;
    if (o->depth_scale > 0) s.depthScale = o->depth_scale;
    if (o->rate_hz > 0) s.rateHz = o->rate_hz;
    s.maxMasks = o->max_masks > 0 ? o->max_masks : 0;
    return s;
}
int cofusion_image_reader_open(const cofusion_image_options* opt, cofusion_image_reader** out, cofusion_image_info* info)
{
    if (!opt || !out || !opt->color_dir) { g_err = "cofusion_image_reader_open: bad arguments"; return -1; }
    cofusion_image_reader* r = nullptr;
    GUARD(r = new cofusion_image_reader(image_options(opt)));
    if (!r->r.ok()) { g_err = r->r.error(); delete r; return -1; }
    if (info) {
        const imageio::SequenceLayout& l = r->r.layout();
        *info = cofusion_image_info{r->r.width(), r->r.height(), l.numFrames, l.startIndex, l.hasMasks ? 1 : 0, l.maxMasks};
    }
    *out = r;
    return 0;
}
int cofusion_image_reader_next(cofusion_image_reader* r, int64_t* ts, float* depth_m, uint8_t* rgb, uint8_t* mask, int* has_mask)
{
    if (!r || !depth_m || !rgb) { g_err = "cofusion_image_reader_next: bad arguments"; return -1; }
    if (!r->r.hasMore()) return 1;
    bool ok = false;
    GUARD(ok = r->r.next(ts, depth_m, rgb, mask, has_mask));
    if (!ok) { g_err = r->r.error(); return -1; }
    return 0;
}
int cofusion_image_reader_rewind(cofusion_image_reader* r) { if (!r) return -1; r->r.rewind(); return 0; }
void cofusion_image_reader_close(cofusion_image_reader* r) { delete r; }

struct cofusion_image_player {
    ImageSequencePlayer p;
    cofusion_image_player(CoFusion& cf, const imageio::SequenceOptions& o, int w) : p(cf, o, w) {}
};
static void fill_info(cofusion_image_info* info, const imageio::SequenceLayout& l, int w, int h)
{
    if (info) *info = cofusion_image_info{w, h, l.numFrames, l.startIndex, l.hasMasks ? 1 : 0, l.maxMasks};
}
int cofusion_image_player_open(cofusion_handle* h, const cofusion_image_options* opt, int workers, cofusion_image_player** out, cofusion_image_info* info)
{
    if (!h || !opt || !opt->color_dir || !out) { g_err = "cofusion_image_player_open: bad arguments"; return -1; }
    if (h->borrowed) { g_err = "the image player is not available for a sequence of a lock-step group"; return -1; }
    GUARD(*out = new cofusion_image_player(*h->cf, image_options(opt), workers > 0 ? workers : 4));
    fill_info(info, (*out)->p.layout(), h->cf->cfg.width, h->cf->cfg.height);
    return 0;
}
int cofusion_image_player_next(cofusion_image_player* p, int64_t* ts, const float** depth_dev, const uint8_t** rgba_dev, const uint8_t** mask_dev)
{
    if (!p) { g_err = "null player"; return -1; }
    bool more = false;
    GUARD(more = p->p.next(ts, depth_dev, rgba_dev, mask_dev));
    return more ? 0 : 1;
}
int cofusion_image_player_process(cofusion_image_player* p)
{
    if (!p) { g_err = "null player"; return -1; }
    bool more = false;
    GUARD(more = p->p.process());
    return more ? 0 : 1;
}
int cofusion_image_player_rewind(cofusion_image_player* p)
{
    if (!p) { g_err = "null player"; return -1; }
    GUARD(p->p.rewind());
    return 0;
}
int cofusion_image_player_set_limits(cofusion_image_player* p, int frame_limit)
{
    if (!p) { g_err = "null player"; return -1; }
    p->p.setLimits(frame_limit);
    return 0;
}
int cofusion_image_player_times(cofusion_image_player* p, double* read_s, double* inflate_s, double* unfilter_s, double* parse_s)
{
    if (!p) { g_err = "null player"; return -1; }
    const imageio::DecodeTimes t = p->p.times();
    if (read_s) *read_s = t.read;
    if (inflate_s) *inflate_s = t.inflate;
    if (unfilter_s) *unfilter_s = t.unfilter;
    if (parse_s) *parse_s = t.parse;
    return 0;
}
void cofusion_image_player_close(cofusion_image_player* p) { delete p; }

struct cofusion_image_prefetcher {
    std::vector<std::vector<uint8_t>> store;
    std::vector<ImageSlotMem> mem;
    ImagePrefetcher* p = nullptr;
    int width = 0, height = 0, held = -1;
    ~cofusion_image_prefetcher() { delete p; }
};
int cofusion_image_prefetch_open(const cofusion_image_options* opt, int workers, int slots, cofusion_image_prefetcher** out, cofusion_image_info* info)
{
    if (!opt || !opt->color_dir || !out || slots < 2 || slots > 64) { g_err = "cofusion_image_prefetch_open: bad arguments"; return -1; }
    imageio::SequenceLayout lay;
    int w = 0, h = 0;
    {
        imageio::ImageSequenceReader probe(image_options(opt));
        if (!probe.ok()) { g_err = probe.error(); return -1; }
        lay = probe.layout(); w = probe.width(); h = probe.height();
    }
    auto* q = new cofusion_image_prefetcher();
    q->width = w; q->height = h;
    const size_t N = (size_t)w * h, blocks = (size_t)CF_JPEG_MAX_BLOCKS(w, h);
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t offCoef = 512, offRgb = offCoef + blocks * 128, offColor = offRgb + up(N * 3), colorBytes = (1 + 4 * (size_t)w) * h,
                 offDepth = offColor + up(colorBytes), depthBytes = 16 * N, offMask = offDepth + up(depthBytes), maskBytes = (1 + (size_t)w) * h,
                 offPal = offMask + up(maskBytes), offBlocks = offPal + 768, total = offBlocks + (size_t)h * sizeof(cf_exr_block);
    for (int s = 0; s < slots; s++) {
        q->store.emplace_back(total);
        uint8_t* b = q->store.back().data();
        ImageSlotMem m;
        m.frame = cf_frame_slot{reinterpret_cast<cf_jpeg_header*>(b), reinterpret_cast<int16_t*>(b + offCoef), blocks, nullptr, b + offRgb};
        m.image.color = b + offColor; m.image.color_bytes = colorBytes; m.image.depth = b + offDepth; m.image.depth_bytes = depthBytes;
        m.image.mask = b + offMask; m.image.mask_bytes = maskBytes; m.image.palette = b + offPal;
        m.image.blocks = reinterpret_cast<cf_exr_block*>(b + offBlocks); m.image.max_blocks = (uint32_t)h;
        q->mem.push_back(m);
    }
    q->p = new ImagePrefetcher(lay, w, h, q->mem, workers > 0 ? workers : 4);
    fill_info(info, lay, w, h);
    *out = q;
    return 0;
}
int cofusion_image_prefetch_next(cofusion_image_prefetcher* q, int64_t* ts, float* depth_m, uint8_t* rgba, uint8_t* mask, int* has_mask)
{
    if (!q || !depth_m || !rgba) { g_err = "cofusion_image_prefetch_next: bad arguments"; return -1; }
    if (q->held >= 0) { q->p->release(q->held); q->held = -1; }
    if (!q->p->hasMore()) return 1;
    ImageFrame f;
    if (!q->p->next(&f)) { g_err = q->p->error(); return -1; }
    q->held = f.slot;
    const ImageSlotMem& m = q->mem[(size_t)f.slot];
    const cf_image_desc& d = f.desc;
    const size_t N = (size_t)q->width * q->height;
    imageio::PngInfo pi;
    pi.width = d.width; pi.height = d.height;
    // the device's kernels, stated on the host
    if (d.color_kind == CF_IMAGE_PNG) {
        pi.bitDepth = 8; pi.colorType = d.png_color_type; pi.bpp = pi.colorType == 2 ? 3 : (pi.colorType == 6 ? 4 : 1); pi.paletteEntries = d.png_palette_entries;
        imageio::pngColorFinishHost(pi, m.image.color, m.image.palette, d.flip_colors != 0, rgba);
    } else {
        std::vector<uint8_t> rgb;
        const uint8_t* src = m.frame.rgb;
        if (d.color_kind == CF_IMAGE_JPEG) { rgb.resize(N * 3); jpegFinishHost(m.frame.header, m.frame.coef, rgb.data()); src = rgb.data(); }
        for (size_t k = 0; k < N; k++) {
            rgba[4 * k + 0] = src[3 * k + (d.flip_colors ? 2 : 0)]; rgba[4 * k + 1] = src[3 * k + 1];
            rgba[4 * k + 2] = src[3 * k + (d.flip_colors ? 0 : 2)]; rgba[4 * k + 3] = 255;
        }
    }
    if (d.depth_kind == CF_IMAGE_PNG) {
        pi.bitDepth = 16; pi.colorType = 0; pi.bpp = 2;
        imageio::pngDepthFinishHost(pi, m.image.depth, d.depth_scale, depth_m);
    } else {
        imageio::ExrInfo x;
        x.width = d.width; x.height = d.height; x.linesPerBlock = d.exr_lines_per_block; x.blocks = d.exr_blocks; x.lineBytes = d.exr_line_bytes;
        x.chanOffset = d.exr_chan_offset; x.chanHalf = d.exr_chan_half;
        imageio::exrFinishHost(x, m.image.depth, m.image.blocks, depth_m);
    }
    if (has_mask) *has_mask = d.mask_kind != CF_IMAGE_NONE;
    if (mask && d.mask_kind == CF_IMAGE_PNG) { pi.bitDepth = 8; pi.colorType = 0; pi.bpp = 1; imageio::pngMaskFinishHost(pi, m.image.mask, mask); }
    else if (mask && d.mask_kind == CF_IMAGE_RAW) memcpy(mask, m.image.mask, N);
    if (ts) *ts = f.timestamp;
    return 0;
}
int cofusion_image_prefetch_rewind(cofusion_image_prefetcher* q) { if (!q) return -1; q->held = -1; q->p->rewind(); return 0; }
void cofusion_image_prefetch_close(cofusion_image_prefetcher* q) { delete q; }

static imageio::PngInfo png_info(const cofusion_png_info* i)
{
    imageio::PngInfo p;
    p.width = i->width; p.height = i->height; p.bitDepth = i->bit_depth; p.colorType = i->color_type; p.bpp = i->bpp; p.paletteEntries = i->palette_entries;
    return p;
}
int cofusion_png_decode(const uint8_t* data, uint64_t size, int role, cofusion_png_info* info, uint8_t* scan, uint64_t cap, uint8_t* palette)
{
    if (!data || !info || !scan || role < 0 || role > 2 || (role == 0 && !palette)) { g_err = "cofusion_png_decode: bad arguments"; return -1; }
    imageio::PngInfo p;
    std::string e;
    GUARD(e = imageio::pngDecode(data, (size_t)size, (imageio::Role)role, &p, scan, (size_t)cap, palette));
    if (!e.empty()) { g_err = e; return -1; }
    *info = cofusion_png_info{p.width, p.height, p.bitDepth, p.colorType, p.bpp, p.paletteEntries};
    return 0;
}
int cofusion_png_finish_host(const cofusion_png_info* info, int role, const uint8_t* scan, const uint8_t* palette, int flip, float depth_scale, void* out)
{
    if (!info || !scan || !out || role < 0 || role > 2 || info->width < 1 || info->height < 1) { g_err = "cofusion_png_finish_host: bad arguments"; return -1; }
    const imageio::PngInfo p = png_info(info);
    const bool colour = p.bitDepth == 8 && ((p.colorType == 0 && p.bpp == 1) || (p.colorType == 2 && p.bpp == 3) || (p.colorType == 6 && p.bpp == 4) ||
                                            (p.colorType == 3 && p.bpp == 1 && palette && p.paletteEntries >= 1 && p.paletteEntries <= 256));
    if (role == 0 ? !colour : (p.colorType != 0 || p.bitDepth != (role == 1 ? 16 : 8) || p.bpp != (role == 1 ? 2 : 1))) {
        g_err = "cofusion_png_finish_host: the description does not fit the role";
        return -1;
    }
    if (role == 0) imageio::pngColorFinishHost(p, scan, palette, flip != 0, static_cast<uint8_t*>(out));
    else if (role == 1) imageio::pngDepthFinishHost(p, scan, depth_scale, static_cast<float*>(out));
    else imageio::pngMaskFinishHost(p, scan, static_cast<uint8_t*>(out));
    return 0;
}
int cofusion_exr_decode(const uint8_t* data, uint64_t size, cofusion_exr_info* info, uint8_t* raw, uint64_t cap, cf_exr_block* blocks, uint64_t max_blocks)
{
    if (!data || !info || !raw || !blocks) { g_err = "cofusion_exr_decode: bad arguments"; return -1; }
    imageio::ExrInfo x;
    std::string e;
    GUARD(e = imageio::exrDecode(data, (size_t)size, &x, raw, (size_t)cap, blocks, (size_t)max_blocks));
    if (!e.empty()) { g_err = e; return -1; }
    *info = cofusion_exr_info{x.width, x.height, x.compression, x.linesPerBlock, x.blocks, x.lineBytes, x.chanOffset, x.chanHalf};
    return 0;
}
int cofusion_exr_finish_host(const cofusion_exr_info* info, const uint8_t* raw, const cf_exr_block* blocks, float* depth)
{
    if (!info || !raw || !blocks || !depth) { g_err = "cofusion_exr_finish_host: bad arguments"; return -1; }
    imageio::ExrInfo x;
    x.width = info->width; x.height = info->height; x.compression = info->compression; x.linesPerBlock = info->lines_per_block; x.blocks = info->blocks;
    x.lineBytes = info->line_bytes; x.chanOffset = info->chan_offset; x.chanHalf = info->chan_half;
    // the table decides addresses: check it as cf_frame_decoder_submit_images does
    const int sample = x.chanHalf ? 2 : 4;
    bool ok = x.width >= 1 && x.height >= 1 && x.blocks >= 1 && x.lineBytes >= 1 && x.chanOffset >= 0 &&
              (int64_t)x.chanOffset + (int64_t)x.width * sample <= x.lineBytes;
    for (int i = 0; ok && i < x.blocks; i++) {
        const cf_exr_block& b = blocks[i];
        ok = b.bytes >= (uint32_t)x.lineBytes && b.bytes % (uint32_t)x.lineBytes == 0 && b.offset == (uint64_t)b.first_line * x.lineBytes &&
             (uint64_t)b.first_line + b.bytes / (uint32_t)x.lineBytes <= (uint64_t)x.height;
    }
    if (!ok) { g_err = "cofusion_exr_finish_host: the block table does not describe a frame of this size"; return -1; }
    GUARD(imageio::exrFinishHost(x, raw, blocks, depth));
    return 0;
}
int cofusion_ppm_decode(const uint8_t* data, uint64_t size, int* width, int* height, uint64_t* pixel_offset)
{
    if (!data || !width || !height || !pixel_offset) { g_err = "cofusion_ppm_decode: bad arguments"; return -1; }
    const uint8_t* px = nullptr;
    const std::string e = imageio::ppmDecode(data, (size_t)size, width, height, &px);
    if (!e.empty()) { g_err = e; return -1; }
    *pixel_offset = (uint64_t)(px - data);
    return 0;
}

}  // extern "C"
