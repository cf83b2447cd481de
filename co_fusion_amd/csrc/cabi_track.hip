// cabi_track.hip -- C-ABI: the per-frame tracking call.  Preparation of every tracker's pinned state, the kernel arguments of the three
// levels, the enqueue of the device-resident Gauss-Newton schedule (launch_gn_track), the fetch of its result.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>

#include "cf_host.h"

using namespace cf;

// ---------------------------------------------------------------- diagnostics build ----
// make ABLATE=1: A/B switches of the culling and traces / replays of single launches of one tracking call, chosen by its number.  The
// tracking call runs TrackDiag::begin in front of its schedule and TrackDiag::end behind it; in the product build both are empty and the
// switches are constants.
#ifdef CF_ABLATE
static bool diag_no_box() { static const bool v = getenv("CF_NO_SCREEN_BOX") != nullptr; return v; }   // A/B of the screen-box culling on one box
static bool diag_no_zcull() { static const bool v = getenv("CF_NO_ZCULL") != nullptr; return v; }       // ... of the depth-interval culling
static bool diag_no_occ() { static const bool v = getenv("CF_NO_OCC") != nullptr; return v; }           // ... and of the occupancy look-up
static const char* diag_icp_ablate() { return getenv("CF_ICP_ABLATE"); }   // cf_odom_bench_icp: ablation bits of the launch (track_reduce.hip: ABL)
static const char* diag_trace_out(const char* name) { const char* e = getenv("CF_ICP_TRACE_OUT"); return e ? e : name; }
// does this tracking call carry the number the switch `name` asks for?  (one counter per switch; unset: none does)
struct DiagCall {
    const char* name; int call = -2, seen = 0;
    bool hit() { if (call == -2) call = getenv(name) ? atoi(getenv(name)) : -1; return call >= 0 && seen++ == call; }
};
static int clear_accumulators(cf_ctx* ctx, cf_odom* const* ods, int n)
{
    for (int m = 0; m < n; m++) {
        if (int r = clear_acc(ctx, ods[m]->icp_acc)) return r;
        if (int r = clear_acc(ctx, ods[m]->rgb_acc)) return r;
    }
    return CF_OK;
}
struct TrackDiag {
    bool solve_trace = false;
    int begin(cf_ctx* ctx);
    int end(cf_ctx* ctx, cf_odom* const* ods, int n, const IcpArgs& icp0, const RgbArgs& rgb0);   // (the level-0 arguments of the call)
};
int TrackDiag::begin(cf_ctx* ctx)
{
    static DiagCall solve{"CF_SOLVE_TRACE"};   // phase stamps of that call's solves (tracker 0)
    solve_trace = solve.hit();
    if (solve_trace) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); trace_solve_begin(); }
    return CF_OK;
}
int TrackDiag::end(cf_ctx* ctx, cf_odom* const* ods, int n, const IcpArgs& icp0, const RgbArgs& rgb0)
{
    if (solve_trace) trace_solve_end(ctx->stream, diag_trace_out("solve_trace.txt"));
    static DiagCall so3{"CF_SO3_TRACE"};   // stamps of that call's SO(3) pre-alignment (tracker 0)
    if (so3.hit()) trace_so3_dump(ctx->stream);
    static DiagCall step{"CF_STEP_TRACE"};   // phases of that call's fused RGB step + solve launch
    if (step.hit()) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        trace_step_solve(ctx->stream, ctx->icp_launch, icp0, rgb0, ctx->d_so3_sync, n, diag_trace_out("step_trace.txt"));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    static DiagCall trace{"CF_ICP_TRACE"};   // per-workgroup stamps of that call's level-0 launch
    if (trace.hit()) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        trace_icp_level0(ctx->stream, ctx->icp_launch, icp0, rgb0, n, ctx->gn_mode, diag_trace_out("icp_trace.txt"));
        if (int r = clear_accumulators(ctx, ods, n)) return r;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // CF_ICP_REPLAY=<call> re-launches the level-0 {ICP || residual} launch of that tracking call (its converged state) back to back
    // under a list of ablation masks and prints the durations -- the decomposition of the launch quoted in DESIGN.md 4.1
    static DiagCall replay{"CF_ICP_REPLAY"};
    if (replay.hit()) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const int masks[] = {0, 8, 16, 32, 8 | 32, 256, 256 | 32, 256 | 16 | 8, 8 | 256 | 32, 256 | 32 | 512, 256 | 32 | 1024, 1024};
        const char* names[] = {"full", "culled models: no ICP", "culled models: no residual", "no residual at all", "unculled ICP only",
                               "unculled models: no ICP", "culled ICP only", "unculled residual + culled nothing", "nothing (empty workgroups)",
                               "culled ICP: the cull test only", "culled ICP only, XCD bands", "full, XCD bands for culled models"};
        for (int k = 0; k < 12; k++) {
            const float us = replay_icp_level0(ctx->stream, ctx->icp_launch, icp0, rgb0, n, ctx->gn_mode, masks[k], 200,
                                               ctx->prof.events[ctx->prof.capacity - 2], ctx->prof.events[ctx->prof.capacity - 1]);
            fprintf(stderr, "[icp replay] %d trackers, mask %3d  %-40s %7.2f us\n", n, masks[k], names[k], us);
        }
        if (int r = clear_accumulators(ctx, ods, n)) return r;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CF_OK;
}
#else
constexpr bool diag_no_box() { return false; }
constexpr bool diag_no_zcull() { return false; }
constexpr bool diag_no_occ() { return false; }
constexpr const char* diag_icp_ablate() { return nullptr; }
struct TrackDiag {
    int begin(cf_ctx*) { return CF_OK; }
    int end(cf_ctx*, cf_odom* const*, int, const IcpArgs&, const RgbArgs&) { return CF_OK; }
};
#endif

static void inv33f_host(const float a[9], float o[9])
{  // Rprev.inverse() (RGBDOdometry.cpp:316), cofactor form
    float c00 = a[4] * a[8] - a[5] * a[7];
    float c01 = a[5] * a[6] - a[3] * a[8];
    float c02 = a[3] * a[7] - a[4] * a[6];
    float det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    float id = 1.0f / det;
    o[0] = c00 * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    o[3] = c01 * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    o[6] = c02 * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}

// enqueue everything one model needs before the lock-step GN loop
static int odom_prepare(cf_odom* od, const float pose[16], const cf_track_opts* opts, float* err_surface, RgbPrepArgs* prep)
{
    cf_ctx* ctx = od->ctx;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    const auto [icp, rgb] = track_terms(opts);
    const cf_cam intr = ctx_cam(ctx);
    if (rgb) {
        RgbPrepArgs a{};  // computeDerivativeImages (RGBDOdometry.cpp:231-235) + candidate mask + projectToPointCloud (:333)
        for (int i = 0; i < CF_NUM_PYRS; i++) {
            const cf_cam il = cam_level(intr, i);
            a.nextImage[i] = od->nextImage[i]; a.nextDepth[i] = od->next_depth(i); a.lastDepth[i] = od->lastDepth[i];
            a.dIdx[i] = od->dIdx[i]; a.dIdy[i] = od->dIdy[i]; a.cand[i] = od->cand[i]; a.cloud[i] = od->cloud[i];
            a.minScale[i] = (float)(pow((double)od->minGrad[i], 2.0) / pow((double)od->sobelScale, 2.0));
            a.fx_inv[i] = 1.0f / il.fx; a.fy_inv[i] = 1.0f / il.fy; a.cx[i] = il.cx; a.cy[i] = il.cy;
        }
        *prep = a;  // launched once for all models of the batch by the caller
    }
    OdomDev* h = od->h_state;
    for (int i = 0; i < CF_NUM_PYRS; i++) {
        h->vmap_curr[i] = od->cur_vmap(i); h->nmap_curr[i] = od->cur_nmap(i);
        h->vmap_g_prev[i] = od->vmap_g_prev[i]; h->nmap_g_prev[i] = od->nmap_g_prev[i];
        h->lastDepth[i] = od->lastDepth[i]; h->nextDepth[i] = od->next_depth(i);
        h->lastImage[i] = od->lastImage[i]; h->nextImage[i] = od->nextImage[i]; h->lastNextImage[i] = od->lastNextImage[i];
        h->dIdx[i] = od->dIdx[i]; h->dIdy[i] = od->dIdy[i]; h->cloud[i] = od->cloud[i]; h->corres[i] = od->corres[i];
        h->cand[i] = od->cand[i];
        h->minGrad[i] = od->minGrad[i];
    }
    h->icp_acc = od->icp_acc; h->rgb_acc = od->rgb_acc; h->err_surface = err_surface;
    h->intr = intr; h->width = W; h->height = H;
    h->distThres = od->distThres; h->angleThres = od->angleThres; h->sobelScale = od->sobelScale;
    h->maxDepthDeltaRGB = od->maxDepthDeltaRGB; h->icpWeight = opts->icp_weight;
    h->icp = icp; h->rgb = rgb; h->rgbOnly = opts->rgb_only;
    // the screen box the previous tracking call ended with sizes this call's launches (launch_icp_rgbres); the pinned host state
    // holds it once that call's results were fetched
    if (h->cull && !od->result_pending) memcpy(od->box_hint, h->stats.cull_box, sizeof(od->box_hint));
    else od->box_hint[0] = kNoBoxHint;
    // ... and likewise the record slots its residual passes needed (a culled tracker's candidate mask is empty outside its prediction)
    for (int i = 0; i < CF_NUM_PYRS; i++) od->res_hint[i] = (h->cull && h->res_range && !od->result_pending) ? h->res_seen[i] : -1;
    // The screen box is the projection of a frustum piece expressed in the camera the model maps were prepared with (map_pose), while the
    // reduction projects with the pose of THIS call: the culling is conservative only if the two are the same pose -- which
    // Model::performTracking guarantees (both are the model's pose) and a C-ABI caller tracking from another initial guess does not.
    float Rt_call[12];
    pose_split(pose, Rt_call, Rt_call + 9);
    // (compared as VALUES: a -0.0f in one of the two poses is the same pose, and a bitwise comparison switched the culling off for it)
    bool same_pose = true;
    for (int i = 0; i < 12; i++) same_pose = same_pose && Rt_call[i] == od->map_pose[i];
    h->aabb_acc = od->aabb; h->cull = (od->use_occ && od->box_valid && od->band_end == 0 && !diag_no_box() && same_pose) ? 1 : 0;
    memcpy(h->box_R, od->map_pose, 36); memcpy(h->box_t, od->map_pose + 9, 12);
    h->res_range = (h->cull && rgb) ? od->res_range : nullptr;
    h->host_twin = od->h_state;
    for (int i = 0; i < CF_NUM_PYRS; i++) h->res_seen[i] = -1;
    if (rgb) prep->res_range = h->res_range;
    // the first launch of a tracking call latches the accumulator and zeroes it (so3_prealign_kernel): a second tracking call on the
    // same preparation would read an empty box and cull every workgroup.  It falls back to the whole image instead.
    od->box_valid = false;
    const float* R = Rt_call; const float* t = Rt_call + 9;
    memcpy(h->Rprev, R, 36); memcpy(h->tprev, t, 12); memcpy(h->Rcurr, R, 36); memcpy(h->tcurr, t, 12);
    inv33f_host(R, h->Rprev_inv);
    memset(&h->stats, 0, sizeof(h->stats));
    h->solves = 0;
    {   // the Gauss-Newton launches this call will enqueue (launch_gn_track): every one of them runs one solve per tracker
        const int its = (opts->fast_odom ? 3 : 10) + (opts->pyramid ? 9 : 0);
        od->expected_solves = its;
    }
    // the accumulators are zero here: dmalloc clears them and every solve leaves them cleared
    od->pending_so3_swap = opts->so3 != 0;
    od->launch_shape = LaunchShape{};
    LAUNCHCHK(ctx);
    return CF_OK;
}

static void fill_rgb_args(cf_ctx* ctx, cf_odom* const* ods, int n, RgbArgs out[3])
{
    for (int l = 0; l < 3; l++) {
        RgbArgs& a = out[l];
        memset(&a, 0, sizeof(a));
        a.cols = ctx->cfg.width >> l; a.rows = ctx->cfg.height >> l;
        a.il = cam_level(ctx_cam(ctx), l);
        a.sobelScale = ods[0]->sobelScale; a.maxDepthDelta = ods[0]->maxDepthDeltaRGB;
        for (int m = 0; m < n; m++) {
            a.m[m] = rgb_model_args(ods[m]->h_state, ods[m]->d_state, l);
            a.m[m].no_counts = (ods[m]->band_end > 0 && !ods[m]->band_counts) ? 1 : 0;
            a.m[m].res_blocks = a.m[m].res_range ? residual_blocks_for(ods[m]->res_hint[l]) : 0;
        }
    }
}

static void fill_icp_args(cf_ctx* ctx, cf_odom* const* ods, int n, IcpArgs out[3])
{
    for (int l = 0; l < CF_NUM_PYRS; l++) {
        IcpArgs& a = out[l];
        memset(&a, 0, sizeof(a));
        a.cols = ctx->cfg.width >> l; a.rows = ctx->cfg.height >> l;
        a.intr = cam_level(ctx_cam(ctx), l);
        a.distThres = ods[0]->distThres; a.angleThres = ods[0]->angleThres;
        a.angleSqLt = ods[0]->angleSqLt; a.distSqLe = ods[0]->distSqLe;
        a.occ_w = ctx->cfg.width >> 2; a.occ_shift = 2 - l;
        for (int m = 0; m < n; m++) {
            cf_odom* od = ods[m];
            a.m[m] = IcpModelArgs{od->cur_vmap(l), od->cur_nmap(l), od->vmap_g_prev[l], od->nmap_g_prev[l], od->d_state, od->icp_acc,
                                  od->h_state->err_surface, (od->use_occ && od->occ_valid && !diag_no_occ()) ? od->occ : nullptr,
                                  od->band_end > 0 ? (od->band_begin >> l) : 0, od->band_end > 0 ? (od->band_end >> l) : 0,
                                  od->h_state->cull,
                                  diag_no_zcull() ? nullptr : od->cur_zrange(l),
                                  od->h_state->cull ? box_blocks_for(od->box_hint, l, a.cols, a.rows, ctx->icp_launch.threads) : 0};
        }
    }
}

// odom_prepare of every tracker of a tracking call, in chunks of kPrepBatch -- what one preparation launch holds, enqueued behind each
// chunk where `launch_prep`; `prep` is left holding the last chunk.  `reference`: for the reference-order tracker, which culls nothing.
static int prepare_trackers(cf_ctx* ctx, cf_odom* const* ods, int n, const float* const* poses_in, const cf_track_opts* opts,
                            float* const* err_surfaces, RgbPrepBatch& prep, bool launch_prep, bool reference)
{
    for (int base = 0; base < n; base += kPrepBatch) {
        const int nb = n - base < kPrepBatch ? n - base : kPrepBatch;
        if (base) prep = RgbPrepBatch{};
        for (int m = base; m < base + nb; m++) {
            if (int r = odom_prepare(ods[m], poses_in[m], opts, err_surfaces ? err_surfaces[m] : nullptr, &prep.m[m - base])) return r;
            if (reference) {
                ods[m]->h_state->cull = 0; ods[m]->h_state->res_range = nullptr; prep.m[m - base].res_range = nullptr;
                ods[m]->box_hint[0] = kNoBoxHint;
                HIPCHK(ctx, hipMemsetAsync(ods[m]->aabb, 0, 8 * sizeof(unsigned), ctx->stream));   // (the default tracker's first launch latches and clears it)
            }
        }
        if (launch_prep) launch_rgb_prep(ctx->stream, prep, nb, ctx->cfg.width, ctx->cfg.height);
    }
    return CF_OK;
}

extern "C" {

int cf_odom_track_batch_async(cf_ctx* ctx, cf_odom* const* ods, int n, const float* const* poses_in,
                              const cf_track_opts* opts, float* const* err_surfaces)
{
    if (!ctx || !ods || n <= 0 || n > ctx->cfg.max_models || n > kMaxBatch || !poses_in || !opts) return CF_EINVAL;
    const TrackTerms terms = track_terms(opts);
    // The pinned host state of a tracker is rewritten below and read / written by the launches of its tracking call: a tracker whose
    // PREVIOUS call has not been fetched yet must drain first.  Per tracker (round 6): the chunks of a frame with more than kMaxBatch
    // trackers hold different trackers, so chunk k + 1 is prepared and enqueued while chunk k runs -- until round 5 a context-wide flag
    // drained the GPU between the chunks.
    {
        bool drain = false;
        for (int m = 0; m < n; m++) drain = drain || (ods[m] && ods[m]->result_pending);
        if (drain) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            for (int m = 0; m < n; m++) if (ods[m]) ods[m]->result_pending = false;   // (landed: what the launches wrote is in the pinned states)
        }
    }
    RgbPrepBatch prep{};
    if (ctx->icp_arith == CF_ICP_ARITH_REFERENCE) {
        // THE REFERENCE'S OWN ORDER (track_ref.hip): per tracker the reference's host loop -- kernel, second-stage kernel, read-back, host
        // solve -- over the same prepared pyramids; nothing is culled (every thread's partial sum is part of the result), nothing is
        // split over GPUs (a rank's band would be another launch shape).  Synchronous; the results are where the default tracker's last
        // solve leaves them, so cf_odom_fetch_result and everything behind it are unchanged.
        for (int m = 0; m < n; m++)
            if (ods[m]->band_end > 0) { ctx->set_error("the reference-order arithmetic (cf_set_icp_arith 2) does not split a tracker's reductions over GPUs"); return CF_ESTATE; }
        if (int r = prepare_trackers(ctx, ods, n, poses_in, opts, err_surfaces, prep, terms.rgb, true)) return r;
        LAUNCHCHK(ctx);
        for (int m = 0; m < n; m++)
            if (int r = ref_track(ctx, ods[m], poses_in[m], opts, err_surfaces ? err_surfaces[m] : nullptr)) return r;
        for (int m = 0; m < n; m++) ods[m]->result_pending = true;
        return CF_OK;
    }
    for (int m = 0; m < n; m++)   // (modes 0 / 1 expect zeroed sums where mode 2 left per-workgroup rows, and the other way round)
        if (ods[m]->gn_epoch_seen != ctx->gn_mode_epoch) {
            HIPCHK(ctx, hipMemsetAsync(ods[m]->rgb_acc, 0, sizeof(unsigned long long) * ods[m]->rgb_acc_words, ctx->stream));
            ods[m]->gn_epoch_seen = ctx->gn_mode_epoch;
        }
    // a batch of <= kPrepBatch trackers with the SO3 pre-alignment: the RGB preparation rides in the pre-alignment's launch
    const bool prep_fused = terms.rgb && opts->so3 != 0 && n <= kPrepBatch;
    if (int r = prepare_trackers(ctx, ods, n, poses_in, opts, err_surfaces, prep, terms.rgb && !prep_fused, false)) return r;
    if (prep_fused) rgb_prep_levels(prep, n, ctx->cfg.width, ctx->cfg.height);
    // (no state upload here: the first launch of the schedule reads the pinned host states itself -- so3_prealign_kernel)
    TrackerStates states{};
    for (int m = 0; m < n; m++) { states.dev[m] = ods[m]->d_state; states.host[m] = ods[m]->h_state; }
    IcpArgs icp_args[3];
    fill_icp_args(ctx, ods, n, icp_args);
    RgbArgs rgb_args[3];
    fill_rgb_args(ctx, ods, n, rgb_args);
    OdomDev* h_states[kMaxBatch];
    for (int m = 0; m < n; m++) h_states[m] = ods[m]->h_state;
    GnHook hook{};
    hook.fn = ctx->collective; hook.user = ctx->collective_user;
    bool any_split = false;
    for (int m = 0; m < n; m++) { hook.split[m] = ods[m]->band_end > 0 ? 1 : 0; any_split = any_split || hook.split[m]; }
    if (any_split && !ctx->collective) { ctx->set_error("a tracker has a row band (cf_odom_set_band) but no collective is registered (cf_set_collective)"); return CF_ESTATE; }
    if (any_split && ctx->gn_mode == 0) { ctx->set_error("split reductions need the record-slot data path (cf_set_gn_mode 1)"); return CF_ESTATE; }
    // timing events on the level-0 launches of every prof.enabled-th tracking call (cf_profile_enable(ctx, N)): the event pairs cost
    // host time (static 640x480: 1275 frames/s without, 1210 with events on every call), sampling keeps the figure and the cost apart
    cf::ProfSink* prof = nullptr;
    if (ctx->prof.enabled > 0 && (ctx->prof_calls++ % (unsigned)ctx->prof.enabled) == 0) prof = &ctx->prof;
    TrackDiag diag;   // (diagnostics build only: empty in the product)
    if (int r = diag.begin(ctx)) return r;
    LaunchShape* shapes[kMaxBatch];
    for (int m = 0; m < n; m++) shapes[m] = &ods[m]->launch_shape;
    IcpLaunch launch_cfg = ctx->icp_launch; launch_cfg.shape = shapes;
    if (!launch_gn_track(ctx->stream, launch_cfg, states, ctx->d_so3_sync, any_split ? &hook : nullptr, icp_args, rgb_args, n,
                         ctx->cfg.width, ctx->cfg.height, opts->so3 != 0, opts->pyramid != 0, opts->fast_odom != 0, terms.rgb, terms.icp, ctx->gn_mode, prof,
                         h_states, prep_fused ? &prep : nullptr)) {
        ctx->set_error("tracking: the registered collective failed inside the Gauss-Newton loop");
        return CF_ESTATE;
    }
    LAUNCHCHK(ctx);
    if (int r = diag.end(ctx, ods, n, icp_args[0], rgb_args[0])) return r;
    // no read-back copy: the last solve of the schedule wrote every tracker's result into its pinned host state (h_states)
    for (int m = 0; m < n; m++) ods[m]->result_pending = true;
    return CF_OK;
}

// The frame's host wait (a polling variant on hipEventQuery was measured in round 3 and bought nothing: DESIGN-NOTES.md).
int cf_wait_stream(cf_ctx* ctx)
{
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}

int cf_odom_fetch_result(cf_odom* od, float trans[3], float rot[9], cf_track_stats* stats)
{
    if (!od) return CF_EINVAL;
    cf_ctx* ctx = od->ctx;
    if (int r = cf_wait_stream(ctx)) return r;
    od->result_pending = false;
    if (trans) memcpy(trans, od->h_state->tcurr, 12);
    if (rot) memcpy(rot, od->h_state->Rcurr, 36);
    if (stats) *stats = od->h_state->stats;
    bool fault = od->h_state->stats.fault != 0;
    if (ctx->icp_arith != CF_ICP_ARITH_REFERENCE && od->expected_solves >= 0 && od->h_state->solves != od->expected_solves) {
        // a launch of the schedule ended without a solve: under cf_set_gn_mode 2 the tracker's workgroups did not meet in one L2 (nobody
        // drew the last ticket); the tickets they left behind would corrupt the next call -- cleared here
        (void)hipMemsetAsync(ctx->d_so3_sync, 0, sizeof(So3Sync) * ((size_t)ctx->cfg.max_models + 1), ctx->stream);
        fault = true;
    }
    od->expected_solves = -1;
    if (od->pending_so3_swap) {  // RGBDOdometry.cpp:469-473
        for (int i = 0; i < CF_NUM_PYRS; i++) std::swap(od->lastNextImage[i], od->nextImage[i]);
        od->pending_so3_swap = false;
    }
    if (fault) {  // a device-side wait between co-resident workgroups expired: the pose was computed from partial sums
        ctx->set_error("tracking: a bounded device-side wait expired (workgroups of one launch were not co-resident)");
        return CF_ESTATE;
    }
    return CF_OK;
}

// RGBDOdometry::getCovariance, RGBDOdometry.cpp:479.  Eigen's lu() is PartialPivLU: per column the row with the largest |entry| at or
// below the diagonal is the pivot (first maximum wins), the column below it is divided by the pivot, rank-1 update of the trailing
// block; inverse() = P e_j through the unit-lower and the upper triangle, column by column.  Host arithmetic in f64, as the reference's.
int cf_odom_get_covariance(const cf_track_stats* stats, double cov[36])
{
    if (!stats || !cov) return CF_EINVAL;
    constexpr int N = 6;
    double lu[N * N];
    int perm[N];
    memcpy(lu, stats->lastA, sizeof(lu));
    for (int i = 0; i < N; i++) perm[i] = i;
    for (int k = 0; k < N; k++) {
        int piv = k;
        double big = fabs(lu[k * N + k]);
        for (int r = k + 1; r < N; r++) { const double a = fabs(lu[r * N + k]); if (a > big) { big = a; piv = r; } }
        if (piv != k) {
            for (int c = 0; c < N; c++) std::swap(lu[k * N + c], lu[piv * N + c]);
            std::swap(perm[k], perm[piv]);
        }
        if (big != 0.0)
            for (int r = k + 1; r < N; r++) lu[r * N + k] /= lu[k * N + k];
        for (int r = k + 1; r < N; r++)
            for (int c = k + 1; c < N; c++) lu[r * N + c] -= lu[r * N + k] * lu[k * N + c];
    }
    for (int j = 0; j < N; j++) {
        double x[N];
        for (int i = 0; i < N; i++) x[i] = (perm[i] == j) ? 1.0 : 0.0;
        for (int i = 0; i < N; i++)
            for (int c = 0; c < i; c++) x[i] -= lu[i * N + c] * x[c];
        for (int i = N - 1; i >= 0; i--) {
            for (int c = i + 1; c < N; c++) x[i] -= lu[i * N + c] * x[c];
            x[i] /= lu[i * N + i];
        }
        for (int i = 0; i < N; i++) cov[i * N + j] = x[i];
    }
    return CF_OK;
}

int cf_set_gn_mode(cf_ctx* ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return CF_EINVAL;
    if (mode == 2) {
        // mode 2 is only correct where hardware workgroup b runs on XCD b mod 8 (rgb_step_solve_kernel: the tracker's workgroups meet in ONE
        // L2).  Checked once per context on the device at hand; refused -- the mode stays what it was -- where it does not hold (another
        // XCD count, a partition mode, CU masking).  ADVICE r5.
        if (ctx->xcd_round_robin < 0) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); ctx->xcd_round_robin = probe_xcd_round_robin(ctx->stream) ? 1 : 0; }
        if (!ctx->xcd_round_robin) { ctx->set_error("cf_set_gn_mode 2: workgroups of a launch are not dealt round-robin over 8 XCDs on this device; the mode needs that"); return CF_ESTATE; }
    }
    if (mode != ctx->gn_mode) {
        // the RGB accumulators mean different things under mode 2 (one row per step workgroup, overwritten) and modes 0 / 1 (kGroups rows of
        // zeroed sums): a switch starts from clean ones.  Trackers created later start clean anyway.
        ctx->gn_mode_epoch++;
    }
    ctx->gn_mode = mode;
    return CF_OK;
}

int cf_odom_get_incremental_transformation(cf_odom* od, float trans[3], float rot[9], const cf_track_opts* opts,
                                           float* icp_err_surface, cf_track_stats* stats)
{
    if (!od || !trans || !rot || !opts) return CF_EINVAL;
    const float pose[16] = {rot[0], rot[1], rot[2], trans[0], rot[3], rot[4], rot[5], trans[1],
                            rot[6], rot[7], rot[8], trans[2], 0, 0, 0, 1};
    const float* poses[1] = {pose};
    float* errs[1] = {icp_err_surface};
    cf_odom* ods[1] = {od};
    if (int r = cf_odom_track_batch_async(od->ctx, ods, 1, poses, opts, errs)) return r;
    return cf_odom_fetch_result(od, trans, rot, stats);
}

// Micro-benchmark: `iters` back-to-back ICP-reduce launches at `level` on the state left by the last
// tracking call (same maps, same pose); returns the average microseconds per launch (hipEvents on the
// launch stream, one pair around the whole batch so event overhead does not pollute the figure).
int cf_odom_bench_icp(cf_odom* od, int level, int iters, float* avg_us)
{
    if (!od || level < 0 || level >= CF_NUM_PYRS || iters <= 0 || !avg_us) return CF_EINVAL;
    cf_ctx* ctx = od->ctx;
    const char* ab = diag_icp_ablate();
    IcpArgs all[3];
    cf_odom* ods[1] = {od};
    fill_icp_args(ctx, ods, 1, all);
    IcpArgs a = all[level];
    a.flags = ab ? (atoi(ab) << 8) : 0;
    for (int i = 0; i < 3; i++) launch_icp_level(ctx->stream, ctx->icp_launch, a, 1, level);
    HIPCHK(ctx, hipEventRecord(ctx->prof.events[ctx->prof.capacity - 2], ctx->stream));
    for (int i = 0; i < iters; i++) launch_icp_level(ctx->stream, ctx->icp_launch, a, 1, level);
    HIPCHK(ctx, hipEventRecord(ctx->prof.events[ctx->prof.capacity - 1], ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->prof.events[ctx->prof.capacity - 2], ctx->prof.events[ctx->prof.capacity - 1]));
    *avg_us = ms * 1000.f / iters;
    return clear_acc(ctx, od->icp_acc);
}

}  // extern "C"
