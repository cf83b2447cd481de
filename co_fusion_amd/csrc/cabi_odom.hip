// cabi_odom.hip -- C-ABI: the tracker object (device-resident RGBDOdometry).  Creation, the cf_odom_init_* family that prepares model
// and frame pyramids, frame-map binding and sharing, row bands, and the read-only views of its buffers and bookkeeping.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "cf_host.h"

using namespace cf;

// The per-level buffers of a tracker with their element counts at a level of n pixels: cf_odom_create and cf_odom_destroy walk this list.
template <typename F>
static int each_level_buffer(cf_odom* od, int i, size_t n, F f)
{
    if (int r = f(od->vmap_g_prev[i], n * 3)) return r;
    if (int r = f(od->nmap_g_prev[i], n * 3)) return r;
    if (int r = f(od->vmap_curr[i], n * 3)) return r;
    if (int r = f(od->nmap_curr[i], n * 3)) return r;
    if (int r = f(od->lastDepth[i], n)) return r;
    if (int r = f(od->nextDepth[i], n)) return r;
    if (int r = f(od->lastImage[i], n)) return r;
    if (int r = f(od->nextImage[i], n)) return r;
    if (int r = f(od->lastNextImage[i], n)) return r;
    if (int r = f(od->dIdx[i], n)) return r;
    if (int r = f(od->dIdy[i], n)) return r;
    if (int r = f(od->cloud[i], n * 3)) return r;
    if (int r = f(od->corres[i], n)) return r;
    if (int r = f(od->cand[i], n)) return r;
    return f(od->zrange[i], (n + 63) / 64);
}

extern "C" {

// ----------------------------------------------------------------------- RGBDOdometry ----
int cf_odom_create(cf_ctx* ctx, cf_odom** out)
{
    if (!ctx || !out) return CF_EINVAL;
    if ((size_t)ctx->cfg.width * ctx->cfg.height > (1u << 22)) { ctx->set_error("tracker: frames above 2^22 pixels are not supported (22-bit pixel index in the correspondence records)"); return CF_EINVAL; }
    cf_odom* od = new cf_odom();
    od->ctx = ctx;
    *out = od;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    const size_t n0 = (size_t)W * H;
    if (int r = dmalloc(ctx, &od->vmaps_tmp, n0 * 4)) return r;
    if (int r = dmalloc(ctx, &od->nmaps_tmp, n0 * 4)) return r;
    for (int i = 0; i < CF_NUM_PYRS; i++) {
        const size_t n = (size_t)(W >> i) * (H >> i);
        if (int r = each_level_buffer(od, i, n, [&](auto*& p, size_t count) { return dmalloc(ctx, &p, count); })) return r;
    }
    if (int r = dmalloc(ctx, &od->icp_acc, (size_t)kGroups * 32)) return r;
    od->rgb_acc_words = rgb_acc_rows(n0) * 32;
    if (int r = dmalloc(ctx, &od->rgb_acc, od->rgb_acc_words)) return r;
    if (int r = dmalloc(ctx, &od->occ, ((size_t)(W >> 2) * (H >> 2) + 3) / 4 * 4)) return r;
    if (int r = dmalloc(ctx, &od->aabb, 8)) return r;
    if (int r = dmalloc(ctx, &od->res_range, 8)) return r;
    for (int k = 0; k < cf_ctx::kStateSlots && od->slot < 0; k++)
        if (!ctx->slot_used[k]) { ctx->slot_used[k] = true; od->slot = k; }
    if (od->slot >= 0) {
        od->d_state = ctx->d_state_pool + od->slot; od->h_state = ctx->h_state_pool + od->slot;
        HIPCHK(ctx, hipMemsetAsync(od->d_state, 0, sizeof(OdomDev), ctx->stream));
    } else {
        if (int r = dmalloc(ctx, &od->d_state, 1)) return r;
        HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&od->h_state), sizeof(OdomDev), hipHostMallocCoherent));
    }
    memset(od->h_state, 0, sizeof(OdomDev));
    // RGBDOdometry ctor defaults: RGBDOdometry.h:45-46, RGBDOdometry.cpp:31-36,103-105
    od->distThres = 0.10f;
    od->distSqLe = sqrt_gate_le(od->distThres);
    od->angleThres = (float)sin(20.f * 3.14159254f / 180.f);
    od->angleSqLt = sqrt_gate_lt(od->angleThres);
    od->sobelScale = (float)(1.0 / pow(2.0, 3));
    od->maxDepthDeltaRGB = 0.07f; od->maxDepthRGB = 6.0f;
    od->minGrad[0] = 5; od->minGrad[1] = 3; od->minGrad[2] = 1;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}

void cf_odom_destroy(cf_odom* od)
{
    if (!od) return;
    (void)hipStreamSynchronize(od->ctx->stream);
    (void)hipFree(od->vmaps_tmp); (void)hipFree(od->nmaps_tmp);
    for (int i = 0; i < CF_NUM_PYRS; i++) (void)each_level_buffer(od, i, 0, [](auto*& p, size_t) { (void)hipFree(p); return 0; });
    (void)hipFree(od->icp_acc); (void)hipFree(od->rgb_acc); (void)hipFree(od->occ); (void)hipFree(od->aabb); (void)hipFree(od->res_range);
    if (od->slot >= 0) od->ctx->slot_used[od->slot] = false;
    else { (void)hipFree(od->d_state); (void)hipHostFree(od->h_state); }
    delete od;
}

// RGBDOdometry::initICPModel, RGBDOdometry.cpp:143-175.  The reference copies the GL textures into
// vmaps_tmp/nmaps_tmp first (two 4.9 MB interop copies); vmaps_tmp is kept because initRGBModel /
// initRGB read depth from it afterwards (:179).
static ModelMapsArgs model_maps_args(cf_odom* od, const float* pred_v4, const float* pred_n4, const float pose[16])
{
    ModelMapsArgs a{};
    a.pred_v4 = pred_v4; a.pred_n4 = pred_n4; a.snapshot = od->vmaps_tmp; a.cols = od->ctx->cfg.width; a.rows = od->ctx->cfg.height;
    for (int i = 0; i < CF_NUM_PYRS; ++i) { a.vmap[i] = od->vmap_g_prev[i]; a.nmap[i] = od->nmap_g_prev[i]; }
    pose_split(pose, a.R, a.t);
    memcpy(od->map_pose, a.R, sizeof(a.R)); memcpy(od->map_pose + 9, a.t, sizeof(a.t));
    a.occ = od->occ; od->occ_valid = true;
    // the bounding box only pays for models that are culled (a model that fills the image would add atomics for nothing)
    a.aabb = od->use_occ ? od->aabb : nullptr; od->box_valid = a.aabb != nullptr;
    return a;
}
static RgbdChain rgbd_chain(cf_odom* od, const uint8_t* rgba, float* const* depths, uint8_t* const* images)
{
    RgbdChain c{};
    c.v4 = od->vmaps_tmp; c.rgba = rgba;
    for (int i = 0; i < CF_NUM_PYRS; ++i) { c.depth[i] = depths[i]; c.image[i] = images[i]; }
    return c;
}

int cf_odom_init_icp_model(cf_odom* od, const float* pred_v4, const float* pred_n4, const float pose[16])
{
    if (!od || !pred_v4 || !pred_n4 || !pose) return CF_EINVAL;
    cf_ctx* ctx = od->ctx;
    ModelMapsBatch b{};   // one launch: snapshot + copyMaps + resize chain + transform of every level
    b.m[0] = model_maps_args(od, pred_v4, pred_n4, pose);
    launch_model_maps(ctx->stream, b, 1);
    LAUNCHCHK(ctx);
    return CF_OK;
}

// RGBDOdometry::populateRGBDData, RGBDOdometry.cpp:177-194
static int populate_rgbd(cf_odom* od, const uint8_t* rgba, float* const* depths, uint8_t* const* images)
{
    cf_ctx* ctx = od->ctx; hipStream_t s = ctx->stream;
    // verticesToDepth + imageBGRToIntensity, then both Gaussian pyramids: three launches for the two chains
    RgbdBatch b{};
    b.c[0] = rgbd_chain(od, rgba, depths, images);
    launch_rgbd_pyramids(s, b, 1, ctx->cfg.width, ctx->cfg.height, od->maxDepthRGB);
    LAUNCHCHK(ctx);
    return CF_OK;
}
int cf_odom_init_rgb_model(cf_odom* od, const uint8_t* pred_rgba) { if (!od || !pred_rgba) return CF_EINVAL; return populate_rgbd(od, pred_rgba, od->lastDepth, od->lastImage); }
int cf_odom_init_rgb(cf_odom* od, const uint8_t* rgba) { if (!od || !rgba) return CF_EINVAL; od->next_depth_is_last = false; return populate_rgbd(od, rgba, od->nextDepth, od->nextImage); }

// initICPModel + initRGBModel + initRGB of `n` trackers in four launches (one grid row per tracker / chain) instead of
// seven per tracker: what CoFusion::trackModels issues for every active model of a frame.
int cf_odom_init_models_batch(cf_ctx* ctx, cf_odom* const* ods, int n, const float* const* pred_v4, const float* const* pred_n4,
                              const uint8_t* const* pred_rgba, const float* const* poses, const uint8_t* frame_rgba)
{
    if (!ctx || n <= 0 || !frame_rgba) return CF_EINVAL;
    std::vector<const uint8_t*> frames((size_t)n, frame_rgba);
    return cf_odom_init_models_batch_frames(ctx, ods, n, pred_v4, pred_n4, pred_rgba, poses, frames.data());
}

// ... with one frame image per tracker: the trackers of SEVERAL sequences (each tracking its own frame) prepared by the same launches
int cf_odom_init_models_batch_frames(cf_ctx* ctx, cf_odom* const* ods, int n, const float* const* pred_v4, const float* const* pred_n4,
                                     const uint8_t* const* pred_rgba, const float* const* poses, const uint8_t* const* frame_rgba)
{
    return cf_odom_init_models_batch_select(ctx, ods, n, pred_v4, pred_n4, pred_rgba, nullptr, nullptr, nullptr, nullptr, 0.f, poses, frame_rgba);
}

// ... and with the fill-in decision of every tracker taken by the kernels (see the header): no host wait for the previous frame
int cf_odom_init_models_batch_select(cf_ctx* ctx, cf_odom* const* ods, int n, const float* const* pred_v4, const float* const* pred_n4,
                                     const uint8_t* const* pred_rgba, const float* const* alt_v4, const float* const* alt_n4,
                                     const uint8_t* const* alt_rgba, const uint32_t* const* fill_counts, float ratio,
                                     const float* const* poses, const uint8_t* const* frame_rgba)
{
    if (!ctx || !ods || n <= 0 || !pred_v4 || !pred_n4 || !pred_rgba || !poses || !frame_rgba) return CF_EINVAL;
    const bool choose = alt_v4 && alt_n4 && alt_rgba && fill_counts;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    hipStream_t s = ctx->stream;
    for (int base = 0; base < n; base += kPrepBatch) {
        const int nb = n - base < kPrepBatch ? n - base : kPrepBatch;
        ModelMapsBatch mb{};
        RgbdBatch rb{};
        for (int k = 0; k < nb; k++) {
            cf_odom* od = ods[base + k];
            if (!od || !pred_v4[base + k] || !pred_n4[base + k] || !pred_rgba[base + k] || !poses[base + k] || !frame_rgba[base + k]) return CF_EINVAL;
            mb.m[k] = model_maps_args(od, pred_v4[base + k], pred_n4[base + k], poses[base + k]);
            rb.c[k] = rgbd_chain(od, pred_rgba[base + k], od->lastDepth, od->lastImage);   // initRGBModel
            rb.c[k].v4 = pred_v4[base + k];  // (the snapshot vmaps_tmp is written by the same launch: read the prediction it copies)
            if (choose && fill_counts[base + k]) {
                if (!alt_v4[base + k] || !alt_n4[base + k] || !alt_rgba[base + k]) return CF_EINVAL;
                mb.m[k].alt_v4 = alt_v4[base + k]; mb.m[k].alt_n4 = alt_n4[base + k]; mb.m[k].sel = fill_counts[base + k]; mb.m[k].sel_ratio = ratio;
                rb.c[k].alt_v4 = alt_v4[base + k]; rb.c[k].alt_rgba = alt_rgba[base + k]; rb.c[k].sel = fill_counts[base + k]; rb.c[k].sel_ratio = ratio;
            }
            od->next_depth_is_last = true;
        }
        // initRGB: the intensity pyramid of the tracker's frame (its depth pyramid would be a second copy of the first chain's -- same source,
        // same cutoff --: intensity only).  The trackers of one sequence track the same frame: ONE chain per distinct frame, which stores every
        // level into the pyramids of all trackers of that frame (RgbdBatch::fan_owner) -- five models were five identical full-resolution grid rows
        int n_chains = nb;
        for (int k = 0; k < nb; k++) {
            cf_odom* od = ods[base + k];
            int owner = -1;
            for (int j = nb; j < n_chains; j++)
                if (rb.c[j].rgba == frame_rgba[base + k]) { owner = j; break; }
            if (owner < 0) {
                owner = n_chains++;
                rb.c[owner] = rgbd_chain(od, frame_rgba[base + k], od->nextDepth, od->nextImage);
                for (int i = 0; i < CF_NUM_PYRS; ++i) rb.c[owner].depth[i] = nullptr;
            }
            rb.fan_owner[k] = (signed char)(owner + 1);
            for (int i = 0; i < CF_NUM_PYRS; ++i) rb.fan_image[i][k] = od->nextImage[i];
        }
        launch_model_maps_and_pyramids(s, mb, nb, rb, n_chains, W, H, ods[base]->maxDepthRGB);
    }
    LAUNCHCHK(ctx);
    return CF_OK;
}

int cf_odom_init_first_rgb(cf_odom* od, const uint8_t* rgba)
{  // RGBDOdometry.cpp:206-215
    if (!od || !rgba) return CF_EINVAL;
    cf_ctx* ctx = od->ctx; hipStream_t s = ctx->stream;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    launch_intensity(s, rgba, W, H, od->lastNextImage[0]);
    for (int i = 0; i + 1 < CF_NUM_PYRS; i++) launch_pyrdown_u8(s, od->lastNextImage[i], W >> i, H >> i, od->lastNextImage[i + 1]);
    LAUNCHCHK(ctx);
    return CF_OK;
}

int cf_odom_init_icp(cf_odom* od, const float* const depth_pyr[CF_NUM_PYRS], float depth_cutoff)
{  // RGBDOdometry.cpp:110-118
    if (!od || !depth_pyr) return CF_EINVAL;
    cf_ctx* ctx = od->ctx; hipStream_t s = ctx->stream;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    FrameMapsArgs a{};
    a.cutoff = depth_cutoff;
    for (int i = 0; i < CF_NUM_PYRS; ++i) {
        const cf_cam il = cam_level(ctx_cam(ctx), i);
        a.depth[i] = depth_pyr[i]; a.vmap[i] = od->vmap_curr[i]; a.nmap[i] = od->nmap_curr[i]; a.zrange[i] = od->zrange[i];
        a.fx_inv[i] = 1.f / il.fx; a.fy_inv[i] = 1.f / il.fy; a.cx[i] = il.cx; a.cy[i] = il.cy;
        od->ext_vmap_curr[i] = nullptr; od->ext_nmap_curr[i] = nullptr; od->ext_zrange[i] = nullptr;
    }
    launch_frame_maps(s, a, W, H);  // createVMap + createNMap of the three levels in one launch
    od->zrange_valid = true;
    LAUNCHCHK(ctx);
    return CF_OK;
}

// The initICP(GPUTexture*, GPUTexture*, cutoff) overload of RGBDOdometry.cpp:120-141, the frame side of the model-to-model tracker:
// the vertices into vmaps_tmp (so that the cf_odom_init_rgb behind it derives a genuine nextDepth from them), copyMaps into level 0 of the
// frame-side maps, resizeVMap / resizeNMap down the pyramid.  The existing preparation kernels, composed: no new arithmetic.  The
// depth intervals of cf_odom_init_icp do not describe these maps (zrange_valid = false, as after a caller wrote the maps); a later
// cf_odom_init_icp restores them.
int cf_odom_init_icp_maps(cf_odom* od, const float* vertex4, const float* normal4)
{
    if (!od || !vertex4 || !normal4) return CF_EINVAL;
    cf_ctx* ctx = od->ctx; hipStream_t s = ctx->stream;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    HIPCHK(ctx, hipMemcpyAsync(od->vmaps_tmp, vertex4, sizeof(float) * 4 * (size_t)W * H, hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < CF_NUM_PYRS; ++i) { od->ext_vmap_curr[i] = nullptr; od->ext_nmap_curr[i] = nullptr; od->ext_zrange[i] = nullptr; }
    launch_copy_maps(s, vertex4, normal4, W, H, od->vmap_curr[0], od->nmap_curr[0]);
    for (int i = 1; i < CF_NUM_PYRS; ++i) {
        launch_resize_map(s, od->vmap_curr[i - 1], W >> (i - 1), H >> (i - 1), od->vmap_curr[i], false);
        launch_resize_map(s, od->nmap_curr[i - 1], W >> (i - 1), H >> (i - 1), od->nmap_curr[i], true);
    }
    od->zrange_valid = false;
    LAUNCHCHK(ctx);
    return CF_OK;
}

int cf_odom_set_culling(cf_odom* od, int on)
{
    if (!od) return CF_EINVAL;
    od->use_occ = on != 0;
    return CF_OK;
}

// One model's reductions split over GPUs: this rank reduces the image rows [row_begin, row_end) (level-0 rows, multiples of 4) inside the
// device-resident Gauss-Newton loop; after every {ICP || residual} launch the registered collective (cf_set_collective, op 0) sums
// the model's accumulators over the ranks, so every rank solves the same system and holds the same pose.  add_counts: exactly one
// rank of the split passes 1 (the RGB residual pass, which every rank runs in full, adds its count / sigma only there).
int cf_odom_set_band(cf_odom* od, int row_begin, int row_end, int add_counts)
{
    if (!od || row_begin < 0 || row_end < row_begin || row_end > od->ctx->cfg.height || (row_begin & 3) || (row_end & 3)) return CF_EINVAL;
    od->band_begin = row_begin; od->band_end = row_end; od->band_counts = add_counts != 0;
    return CF_OK;
}
int cf_set_collective(cf_ctx* ctx, int (*fn)(void*, int, void*, uint64_t, void*), void* user)
{
    if (!ctx) return CF_EINVAL;
    ctx->collective = fn; ctx->collective_user = user;
    return CF_OK;
}

int cf_odom_bind_frame_maps(cf_odom* od, const float* const vmaps[CF_NUM_PYRS], const float* const nmaps[CF_NUM_PYRS])
{
    if (!od) return CF_EINVAL;
    for (int i = 0; i < CF_NUM_PYRS; i++) { od->ext_vmap_curr[i] = vmaps ? vmaps[i] : nullptr; od->ext_nmap_curr[i] = nmaps ? nmaps[i] : nullptr; od->ext_zrange[i] = nullptr; }
    return CF_OK;
}
// the frame maps `owner` computed with cf_odom_init_icp (all models of a frame track the same frame), incl. their per-run depth
// intervals -- what lets the culled ICP reduction of `od` skip runs at other depths
int cf_odom_share_frame_maps(cf_odom* od, cf_odom* owner)
{
    if (!od || !owner || od->ctx != owner->ctx) return CF_EINVAL;
    for (int i = 0; i < CF_NUM_PYRS; i++) {
        od->ext_vmap_curr[i] = owner->cur_vmap(i); od->ext_nmap_curr[i] = owner->cur_nmap(i); od->ext_zrange[i] = owner->cur_zrange(i);
    }
    return CF_OK;
}

// What the level-0 {ICP || residual} launch of the LAST fetched tracking call visited for this tracker, in pixels: the 64-pixel runs inside
// its final screen box (the whole image when it was not culled) and the record slots between its first and last RGB candidate x the
// pixels per slot (the whole image likewise).  The physical byte count of bench.py's roofline is made of these.
int cf_odom_level0_visited(cf_odom* od, uint64_t* icp_pixels, uint64_t* residual_pixels)
{
    if (!od || !icp_pixels || !residual_pixels) return CF_EINVAL;
    const cf_ctx* ctx = od->ctx;
    const OdomDev* h = od->h_state;
    const uint64_t N = (uint64_t)ctx->cfg.width * ctx->cfg.height;
    *icp_pixels = N; *residual_pixels = h->rgb ? N : 0;
    if (!h->icp) *icp_pixels = 0;
    if (h->cull && ctx->icp_arith != CF_ICP_ARITH_REFERENCE) {
        if (h->icp) { const CullRuns cr = cull_runs(h->stats.cull_box, 0, ctx->cfg.width, ctx->cfg.height); *icp_pixels = (uint64_t)cr.total * 64 < N ? (uint64_t)cr.total * 64 : N; }
        if (h->rgb && h->res_range && h->res_seen[0] >= 0) { const uint64_t px = (uint64_t)h->res_seen[0] * (uint64_t)(ctx->icp_launch.threads * 4); *residual_pixels = px < N ? px : N; }
    }
    return CF_OK;
}

// Workgroups the launcher (launch_icp_rgbres) gave this tracker in its last tracking call: host bookkeeping, no device access.
int cf_odom_last_launch_shape(cf_odom* od, int icp_blocks[3], int residual_blocks[3], int* icp_blocks_err)
{
    if (!od) return CF_EINVAL;
    for (int l = 0; l < CF_NUM_PYRS; l++) {
        if (icp_blocks) icp_blocks[l] = od->launch_shape.icp[l];
        if (residual_blocks) residual_blocks[l] = od->launch_shape.res[l];
    }
    if (icp_blocks_err) *icp_blocks_err = od->launch_shape.icp_err;
    return CF_OK;
}

int cf_odom_buffer(cf_odom* od, int which, int level, void** dptr, uint64_t* bytes)
{
    if (!od || level < 0 || level >= CF_NUM_PYRS || !dptr) return CF_EINVAL;
    const size_t n = (size_t)(od->ctx->cfg.width >> level) * (od->ctx->cfg.height >> level);
    void* p = nullptr; size_t b = 0;
    // a caller that takes the pointer of the current vertex map may write it: the depth intervals cf_odom_init_icp stored beside the
    // map no longer describe it (the culled reduction would skip runs that now hold matching depths)
    if (which == 0 && !od->ext_vmap_curr[level]) od->zrange_valid = false;
    switch (which) {
        case 0: p = (void*)od->cur_vmap(level); b = n * 12; break;
        case 1: p = (void*)od->cur_nmap(level); b = n * 12; break;
        case 2: p = od->vmap_g_prev[level]; b = n * 12; break;
        case 3: p = od->nmap_g_prev[level]; b = n * 12; break;
        case 4: p = od->lastDepth[level]; b = n * 4; break;
        case 5: p = od->next_depth(level); b = n * 4; break;
        case 6: p = od->lastImage[level]; b = n; break;
        case 7: p = od->nextImage[level]; b = n; break;
        case 8: p = od->lastNextImage[level]; b = n; break;
        case 9: p = od->dIdx[level]; b = n * 2; break;
        case 10: p = od->dIdy[level]; b = n * 2; break;
        case 11: p = od->cloud[level]; b = n * 12; break;
        case 12: p = od->corres[level]; b = n * 16; break;
        // what the culling decides with (read only: no tracker state changes)
        case 13: p = od->cand[level]; b = n; break;
        case 14: p = od->zrange[level]; b = (n + 63) / 64 * sizeof(float2); break;
        case 15: if (level != 0) return CF_EINVAL; p = od->occ; b = (size_t)(od->ctx->cfg.width >> 2) * (od->ctx->cfg.height >> 2); break;
        case 16: if (level != 0) return CF_EINVAL; p = od->aabb; b = 6 * sizeof(unsigned); break;
        default: return CF_EINVAL;
    }
    *dptr = p; if (bytes) *bytes = b;
    return CF_OK;
}

}  // extern "C"
