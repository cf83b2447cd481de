// cabi_steps.hip -- C-ABI: the single-function entries.  Map-preparation wrappers, the stand-alone reduction steps on the context's
// scratch state (C-ABI parity with icpStep / computeRgbResidual / rgbStep / so3Step), one Gauss-Newton solve and the SO3 pre-alignment
// launch on their own.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "cf_host.h"
#include "gn_ref_host.h"

using namespace cf;

// ------------------------------------------------------------ helpers of the stand-alone reductions ----
// The upper triangle of the N x (N + 1) system [A | b] as the reductions store it, row by row (reduce.cu:481-498, :1161-1172), into the
// symmetric A and b (either may be null); word(k, i, j) converts stored word k, entry (i, j).
template <int N, typename Word>
static void unpack_upper(float* A, float* b, Word word)
{
    int shift = 0;
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N + 1; ++j) {
            const float value = word(shift, i, j);
            shift++;
            if (j == N) { if (b) b[i] = value; }
            else if (A) A[j * N + i] = A[i * N + j] = value;
        }
}
static void se3_unpack_host(const unsigned long long* t, int F, float* A, float* b, float* residual)
{  // F < 0: the Gram form of the ICP sums, word (i, j) carries kGramBits[i] + kGramBits[j] fraction bits
    unpack_upper<6>(A, b, [&](int k, int i, int j) { return (float)ldexp((double)(long long)t[k], -(F >= 0 ? F : kGramBits[i] + kGramBits[j])); });
    if (residual) { residual[0] = (float)ldexp((double)(long long)t[27], -(F >= 0 ? F : 2 * kGramBits[6])); residual[1] = (float)(long long)t[28]; }
}

// Runs one kernel family on the ctx scratch state (single model, level 0 geometry = cols x rows).
static int scratch_begin(cf_ctx* ctx, int cols, int rows)
{
    OdomDev* h = ctx->h_scratch_state;
    memset(h, 0, sizeof(*h));
    h->width = cols; h->height = rows;
    h->icp_acc = ctx->d_acc_a; h->rgb_acc = ctx->d_acc_b;
    h->icp = 1; h->rgb = 1;
    if (int r = clear_acc(ctx, ctx->d_acc_a)) return r;
    return clear_acc(ctx, ctx->d_acc_b);
}
static int scratch_commit(cf_ctx* ctx)
{
    refresh_hot(ctx->h_scratch_state);   // the kernels read pose / flags through the hot block (cf_kernels.h: GnHot)
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_scratch_state, ctx->h_scratch_state, sizeof(OdomDev), hipMemcpyHostToDevice, ctx->stream));
    return CF_OK;
}
// A stand-alone step under the reference-order arithmetic (cf_set_icp_arith 2): `step` fills the 29 f32 totals of the reference's own tree
// (track_ref.hip); there are no fixed-point sums in this mode, sums_host reads zero.
template <typename Step>
static int ref_step29(float* A_host, float* b_host, float* residual_host, int64_t* sums_host, Step step)
{
    if (sums_host) memset(sums_host, 0, sizeof(int64_t) * 32);
    float out29[29] = {};   // (the RGB step has no residual words)
    if (int r = step(out29)) return r;
    float A[36], b[6], res[2];
    refhost::unpack29(out29, A, b, res);
    if (A_host) memcpy(A_host, A, sizeof(A));
    if (b_host) memcpy(b_host, b, sizeof(b));
    if (residual_host) memcpy(residual_host, res, sizeof(res));
    return CF_OK;
}
static int fetch_totals(cf_ctx* ctx, const unsigned long long* acc, int words)
{
    launch_acc_total(ctx->stream, acc, ctx->d_out);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}

// fraction bits of the RGB sums for a given sigma: same integer rule as cf::rgb_fix_bits (cf_device.h)
static int rgb_fix_bits_host(float sigma)
{
    if (sigma == -1.0f || !(sigma >= 2.0f)) return 8;
    unsigned u; memcpy(&u, &sigma, 4);
    const int F = 8 + 2 * ((int)((u >> 23) & 255u) - 127);
    return F > 32 ? 32 : F;
}

// cf_gn_solve_step: device states filled from the caller's words, and back
namespace {
void gn_state_to_dev(const cf_gn_state& g, OdomDev* h)   // (configuration words included: used for states and twins alike)
{
    h->intr = g.intr; h->width = g.width; h->height = g.height; h->icp = g.icp; h->rgb = g.rgb; h->rgbOnly = g.rgbOnly; h->icpWeight = g.icpWeight;
    memcpy(h->Rprev, g.Rprev, 36); memcpy(h->tprev, g.tprev, 12); memcpy(h->Rprev_inv, g.Rprev_inv, 36); memcpy(h->Rcurr, g.Rcurr, 36); memcpy(h->tcurr, g.tcurr, 12);
    memcpy(h->resultRt, g.resultRt, sizeof(g.resultRt)); memcpy(h->krkInv, g.krkInv, 36); memcpy(h->kt, g.kt, 12);
    h->lastRGBError = g.lastRGBError; h->level_done = g.level_done; h->solves = g.solves; memcpy(h->residual, g.residual, 8);
    memcpy(h->cull_z, g.cull_z, 8); memcpy(h->pose_inv, g.pose_inv, sizeof(g.pose_inv)); h->stats = g.stats;
}
void gn_state_from_dev(const OdomDev* h, cf_gn_state* g)  // every word back, the configuration the solve must leave alone included
{
    g->intr = h->intr; g->width = h->width; g->height = h->height; g->icp = h->icp; g->rgb = h->rgb; g->rgbOnly = h->rgbOnly; g->icpWeight = h->icpWeight;
    memcpy(g->Rprev, h->Rprev, 36); memcpy(g->tprev, h->tprev, 12); memcpy(g->Rprev_inv, h->Rprev_inv, 36); memcpy(g->Rcurr, h->Rcurr, 36); memcpy(g->tcurr, h->tcurr, 12);
    memcpy(g->resultRt, h->resultRt, sizeof(g->resultRt)); memcpy(g->krkInv, h->krkInv, 36); memcpy(g->kt, h->kt, 12);
    g->lastRGBError = h->lastRGBError; g->level_done = h->level_done; g->solves = h->solves; memcpy(g->residual, h->residual, 8);
    memcpy(g->cull_z, h->cull_z, 8); memcpy(g->pose_inv, h->pose_inv, sizeof(g->pose_inv)); g->stats = h->stats;
}
struct GnStepBuffers {   // temporaries of one cf_gn_solve_step / cf_so3_prealign_step / cf_rgb_records_step call
    hipStream_t stream = nullptr;
    OdomDev* d_states = nullptr; unsigned long long* d_acc = nullptr; OdomDev* h_twins = nullptr;
    cf_dataterm* d_recs = nullptr; unsigned* d_range = nullptr; So3Sync* d_sync = nullptr;   // (cf_rgb_records_step)
    // (an entry that fails half way returns with copies and the launch still enqueued: nothing they touch is released before the stream is idle)
    ~GnStepBuffers()
    {
        (void)hipStreamSynchronize(stream); (void)hipFree(d_states); (void)hipFree(d_acc); if (h_twins) (void)hipHostFree(h_twins);
        (void)hipFree(d_recs); (void)hipFree(d_range); (void)hipFree(d_sync);
    }
};
}  // namespace

extern "C" {

// ---------------------------------------------------------------- map preparation ----
#define PREP_PROLOGUE if (!ctx) return CF_EINVAL
int cf_create_vmap(cf_ctx* ctx, const float* depth, int cols, int rows, cf_cam intr, float cutoff, float* vmap)
{ PREP_PROLOGUE; launch_vmap(ctx->stream, depth, cols, rows, intr, cutoff, vmap); LAUNCHCHK(ctx); return CF_OK; }
int cf_create_nmap(cf_ctx* ctx, const float* vmap, int cols, int rows, float* nmap)
{ PREP_PROLOGUE; launch_nmap(ctx->stream, vmap, cols, rows, nmap); LAUNCHCHK(ctx); return CF_OK; }
int cf_copy_maps(cf_ctx* ctx, const float* v4, const float* n4, int cols, int rows, float* vmap, float* nmap)
{ PREP_PROLOGUE; launch_copy_maps(ctx->stream, v4, n4, cols, rows, vmap, nmap); LAUNCHCHK(ctx); return CF_OK; }
int cf_resize_map(cf_ctx* ctx, const float* in, int in_cols, int in_rows, float* out, int normalize)
{ PREP_PROLOGUE; launch_resize_map(ctx->stream, in, in_cols, in_rows, out, normalize != 0); LAUNCHCHK(ctx); return CF_OK; }
int cf_transform_maps(cf_ctx* ctx, float* vmap, float* nmap, int cols, int rows, const float R[9], const float t[3])
{ PREP_PROLOGUE; launch_transform_maps(ctx->stream, vmap, nmap, cols, rows, R, t); LAUNCHCHK(ctx); return CF_OK; }
int cf_vertices_to_depth(cf_ctx* ctx, const float* v4, int cols, int rows, float cutoff, float* depth)
{ PREP_PROLOGUE; launch_vertices_to_depth(ctx->stream, v4, cols, rows, cutoff, depth); LAUNCHCHK(ctx); return CF_OK; }
int cf_pyrdown_gauss_f32(cf_ctx* ctx, const float* src, int scols, int srows, float* dst)
{ PREP_PROLOGUE; launch_pyrdown_f32(ctx->stream, src, scols, srows, dst); LAUNCHCHK(ctx); return CF_OK; }
int cf_pyrdown_gauss_u8(cf_ctx* ctx, const uint8_t* src, int scols, int srows, uint8_t* dst)
{ PREP_PROLOGUE; launch_pyrdown_u8(ctx->stream, src, scols, srows, dst); LAUNCHCHK(ctx); return CF_OK; }
int cf_rgba_to_intensity(cf_ctx* ctx, const uint8_t* rgba, int cols, int rows, uint8_t* dst)
{ PREP_PROLOGUE; launch_intensity(ctx->stream, rgba, cols, rows, dst); LAUNCHCHK(ctx); return CF_OK; }
int cf_sobel(cf_ctx* ctx, const uint8_t* src, int cols, int rows, int16_t* dx, int16_t* dy)
{ PREP_PROLOGUE; launch_sobel(ctx->stream, src, cols, rows, dx, dy); LAUNCHCHK(ctx); return CF_OK; }
int cf_project_cloud(cf_ctx* ctx, const float* depth, int cols, int rows, cf_cam il, float* cloud3)
{ PREP_PROLOGUE; launch_cloud(ctx->stream, depth, cols, rows, il, cloud3); LAUNCHCHK(ctx); return CF_OK; }
int cf_depth_pyramid(cf_ctx* ctx, const float* depth_filtered, int cols, int rows, float* l1, float* l2)
{
    PREP_PROLOGUE;
    launch_pyrdown_f32(ctx->stream, depth_filtered, cols, rows, l1);
    launch_pyrdown_f32(ctx->stream, l1, cols / 2, rows / 2, l2);
    LAUNCHCHK(ctx);
    return CF_OK;
}

// ------------------------------------------------------------ stand-alone reductions ----
int cf_icp_step(cf_ctx* ctx, const float Rcurr[9], const float tcurr[3], const float* vmap_curr, const float* nmap_curr,
                const float Rprev_inv[9], const float tprev[3], cf_cam intr, const float* vmap_g_prev,
                const float* nmap_g_prev, float dist_thres, float angle_thres, int cols, int rows, float* A_host,
                float* b_host, float* residual_host, int64_t* sums_host, float* err_surface)
{
    return cf_icp_step_band(ctx, Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, dist_thres, angle_thres,
                            cols, rows, 0, rows, A_host, b_host, residual_host, sums_host, err_surface);
}

int cf_icp_step_band(cf_ctx* ctx, const float Rcurr[9], const float tcurr[3], const float* vmap_curr, const float* nmap_curr,
                     const float Rprev_inv[9], const float tprev[3], cf_cam intr, const float* vmap_g_prev,
                     const float* nmap_g_prev, float dist_thres, float angle_thres, int cols, int rows, int row_begin, int row_end,
                     float* A_host, float* b_host, float* residual_host, int64_t* sums_host, float* err_surface)
{
    if (!ctx || !vmap_curr || !nmap_curr || !vmap_g_prev || !nmap_g_prev || (cols % 4)) return CF_EINVAL;
    if (row_begin < 0 || row_end > rows || row_begin >= row_end) return CF_EINVAL;
    if (ctx->icp_arith == CF_ICP_ARITH_REFERENCE) {   // the reference's own f32 tree (track_ref.hip): no fixed-point sums, no row bands
        if (row_begin != 0 || row_end != rows) { ctx->set_error("cf_icp_step_band: the reference-order arithmetic has no row bands (a band is another launch shape)"); return CF_EINVAL; }
        return ref_step29(A_host, b_host, residual_host, sums_host, [&](float* out29) {
            return ref_icp_step(ctx, Rcurr, tcurr, vmap_curr, nmap_curr, Rprev_inv, tprev, intr, vmap_g_prev, nmap_g_prev, dist_thres, angle_thres, cols, rows, err_surface, out29);
        });
    }
    if (int r = scratch_begin(ctx, cols, rows)) return r;
    OdomDev* h = ctx->h_scratch_state;
    memcpy(h->Rcurr, Rcurr, 36); memcpy(h->tcurr, tcurr, 12); memcpy(h->Rprev_inv, Rprev_inv, 36); memcpy(h->tprev, tprev, 12);
    h->intr = intr; h->vmap_curr[0] = vmap_curr; h->nmap_curr[0] = nmap_curr; h->vmap_g_prev[0] = vmap_g_prev;
    h->nmap_g_prev[0] = nmap_g_prev; h->distThres = dist_thres; h->angleThres = angle_thres; h->err_surface = err_surface;
    if (int r = scratch_commit(ctx)) return r;
    IcpArgs a{};
    a.m[0] = IcpModelArgs{vmap_curr, nmap_curr, vmap_g_prev, nmap_g_prev, ctx->d_scratch_state, ctx->d_acc_a, err_surface, nullptr, 0, 0};
    a.cols = cols; a.rows = rows; a.intr = intr; a.distThres = dist_thres; a.angleThres = angle_thres;
    a.angleSqLt = sqrt_gate_lt(angle_thres); a.distSqLe = sqrt_gate_le(dist_thres);
    a.flags = err_surface ? 1 : 0;
    a.row_begin = row_begin; a.row_end = row_end;
    launch_icp_level(ctx->stream, ctx->icp_launch, a, 1, 0);
    LAUNCHCHK(ctx);
    if (int r = fetch_totals(ctx, ctx->d_acc_a, 32)) return r;
    se3_unpack_host(ctx->h_out, ctx->icp_launch.gram ? -1 : CF_FIX_ICP, A_host, b_host, residual_host);
    if (sums_host) memcpy(sums_host, ctx->h_out, sizeof(int64_t) * 32);
    return CF_OK;
}

int cf_rgb_residual(cf_ctx* ctx, float min_scale, const int16_t* dIdx, const int16_t* dIdy, const float* last_depth,
                    const float* next_depth, const uint8_t* last_image, const uint8_t* next_image, cf_dataterm* corres,
                    float max_depth_delta, const float kt[3], const float krkinv[9], int cols, int rows,
                    int* sigma_sum_host, int* count_host)
{
    if (!ctx || !corres || (size_t)cols * rows > (size_t)ctx->cfg.width * ctx->cfg.height) return CF_EINVAL;
    if (int r = scratch_begin(ctx, cols, rows)) return r;
    launch_rgb_cand(ctx->stream, dIdx, dIdy, next_depth, next_image, min_scale, cols, rows, ctx->d_cand_scratch);
    OdomDev* h = ctx->h_scratch_state;
    h->cand[0] = ctx->d_cand_scratch; h->lastDepth[0] = last_depth; h->nextDepth[0] = next_depth;
    h->lastImage[0] = last_image; h->nextImage[0] = next_image; h->corres[0] = corres;
    h->maxDepthDeltaRGB = max_depth_delta; memcpy(h->kt, kt, 12); memcpy(h->krkInv, krkinv, 36);
    if (int r = scratch_commit(ctx)) return r;
    RgbArgs ra{};
    ra.m[0] = rgb_model_args(h, ctx->d_scratch_state, 0);
    ra.cols = cols; ra.rows = rows; ra.maxDepthDelta = max_depth_delta;
    launch_rgb_residual(ctx->stream, ra, 1);
    LAUNCHCHK(ctx);
    if (int r = fetch_totals(ctx, ctx->d_acc_a, 32)) return r;
    if (count_host) *count_host = (int)ctx->h_out[29];
    if (sigma_sum_host) *sigma_sum_host = (int)ctx->h_out[30];
    return CF_OK;
}

int cf_rgb_step(cf_ctx* ctx, const cf_dataterm* corres, float sigma, const float* cloud3, float fx, float fy,
                const int16_t* dIdx, const int16_t* dIdy, float sobel_scale, int cols, int rows, float* A_host,
                float* b_host, int64_t* sums_host)
{
    if (!ctx || !corres) return CF_EINVAL;
    if (ctx->icp_arith == CF_ICP_ARITH_REFERENCE)
        return ref_step29(A_host, b_host, nullptr, sums_host, [&](float* out29) { return ref_rgb_step(ctx, corres, sigma, cloud3, fx, fy, dIdx, dIdy, sobel_scale, cols, rows, out29); });
    if (int r = scratch_begin(ctx, cols, rows)) return r;
    OdomDev* h = ctx->h_scratch_state;
    h->corres[0] = const_cast<cf_dataterm*>(corres); h->cloud[0] = cloud3; h->dIdx[0] = dIdx; h->dIdy[0] = dIdy;
    h->sobelScale = sobel_scale; h->intr = cf_cam{fx, fy, 0, 0};
    // rgb_step_kernel derives sigma from words 29/30 of the ICP accumulator (count, sum diff^2);
    // encode the caller's sigma so that the same rule reproduces it: sigma == -1 -> rgbOnly,
    // sigma == 1 -> (count 1, sigma 0) [tmpError == 0 branch], otherwise count = sigma.
    unsigned long long seed[2] = {0, 0};
    if (sigma == -1.f) h->rgbOnly = 1;
    else if (sigma == 1.f) { seed[0] = 1; seed[1] = 0; }
    else { seed[0] = (unsigned long long)(long long)(int)sigma; seed[1] = 1; }
    if ((float)(int)sigma != sigma) return CF_EINVAL;  // the reference only ever passes -1, 1 or an integer count
    if (int r = scratch_commit(ctx)) return r;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_acc_a + 29, seed, sizeof(seed), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // seed is on the host stack
    RgbArgs ra{};
    ra.m[0] = rgb_model_args(h, ctx->d_scratch_state, 0);
    ra.cols = cols; ra.rows = rows; ra.il = cf_cam{fx, fy, 0, 0}; ra.sobelScale = sobel_scale;
    launch_rgb_step(ctx->stream, ra, 1);
    LAUNCHCHK(ctx);
    if (int r = fetch_totals(ctx, ctx->d_acc_b, 32)) return r;
    se3_unpack_host(ctx->h_out, rgb_fix_bits_host(sigma), A_host, b_host, nullptr);
    if (sums_host) memcpy(sums_host, ctx->h_out, sizeof(int64_t) * 32);
    return CF_OK;
}

int cf_so3_step(cf_ctx* ctx, const uint8_t* last_image, const uint8_t* next_image, const float image_basis[9],
                const float kinv[9], const float krlr[9], int cols, int rows, float* A_host, float* b_host,
                float* residual_host, int64_t* sums_host)
{
    if (!ctx) return CF_EINVAL;
    if (ctx->icp_arith == CF_ICP_ARITH_REFERENCE) {
        if (sums_host) memset(sums_host, 0, sizeof(int64_t) * 16);
        float o[11];
        if (int r = ref_so3_step(ctx, last_image, next_image, image_basis, kinv, krlr, cols, rows, o)) return r;
        unpack_upper<3>(A_host, b_host, [&](int k, int, int) { return o[k]; });
        if (residual_host) { residual_host[0] = o[9]; residual_host[1] = o[10]; }
        return CF_OK;
    }
    launch_so3_step(ctx->stream, last_image, next_image, image_basis, kinv, krlr, cols, rows, ctx->d_out);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned long long* t = ctx->h_out;
    unpack_upper<3>(A_host, b_host, [&](int k, int, int) { return (float)ldexp((double)(long long)t[k], -CF_FIX_SO3); });
    if (residual_host) { residual_host[0] = (float)ldexp((double)(long long)t[9], -CF_FIX_SO3); residual_host[1] = (float)(long long)t[10]; }
    if (sums_host) memcpy(sums_host, t, sizeof(int64_t) * 16);
    return CF_OK;
}

// The solve of one Gauss-Newton iteration on its own: gn_solve_kernel as the schedule launches it (launch_gn_solve), on temporary
// device states filled from the caller's words.
int cf_gn_solve_step(cf_ctx* ctx, int n, cf_gn_system* systems, int next_level, int last_of_level, int icp_fix)
{
    if (!ctx || !systems || n < 1 || n > kMaxBatch || next_level < -1 || next_level > 2 || (icp_fix != -1 && icp_fix != CF_FIX_ICP)) return CF_EINVAL;
    constexpr size_t kAccWords = (size_t)kGroups * 32;
    static_assert(sizeof(systems->icp_acc) == kAccWords * 8 && sizeof(systems->hot) == sizeof(GnHot), "cf_gn_system mirrors the accumulators and the hot block");
    std::vector<OdomDev> h((size_t)n);   // (declared in front of buf: destroyed behind its synchronisation)
    GnStepBuffers buf;
    buf.stream = ctx->stream;
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_states), sizeof(OdomDev) * n));
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_acc), 8 * kAccWords * 2 * n));
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&buf.h_twins), sizeof(OdomDev) * n, hipHostMallocCoherent));  // the solve stores into them
    GnArgs gn{};
    gn.icp_gram = icp_fix < 0 ? 1 : 0;
    gn.slot_px = ctx->icp_launch.threads * 4;
    for (int k = 0; k < n; k++) {
        OdomDev* s = &h[(size_t)k];
        memset(s, 0, sizeof(*s));
        gn_state_to_dev(systems[k].state, s);
        s->icp_acc = buf.d_acc + kAccWords * 2 * k; s->rgb_acc = s->icp_acc + kAccWords;
        refresh_hot(s);
        memset(&buf.h_twins[k], 0, sizeof(OdomDev));
        gn_state_to_dev(systems[k].twin, &buf.h_twins[k]);
        gn.od[k] = buf.d_states + k; gn.icp_acc[k] = s->icp_acc; gn.rgb_acc[k] = s->rgb_acc; gn.od_host[k] = &buf.h_twins[k];
        HIPCHK(ctx, hipMemcpyAsync(s->icp_acc, systems[k].icp_acc, 8 * kAccWords, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(s->rgb_acc, systems[k].rgb_acc, 8 * kAccWords, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(buf.d_states, h.data(), sizeof(OdomDev) * n, hipMemcpyHostToDevice, ctx->stream));
    launch_gn_solve(ctx->stream, gn, n, next_level, last_of_level);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), buf.d_states, sizeof(OdomDev) * n, hipMemcpyDeviceToHost, ctx->stream));
    for (int k = 0; k < n; k++) {
        HIPCHK(ctx, hipMemcpyAsync(systems[k].icp_acc, gn.icp_acc[k], 8 * kAccWords, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(systems[k].rgb_acc, gn.rgb_acc[k], 8 * kAccWords, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++) {
        gn_state_from_dev(&h[(size_t)k], &systems[k].state);
        gn_state_from_dev(&buf.h_twins[k], &systems[k].twin);
        memcpy(systems[k].hot, &h[(size_t)k].hot, sizeof(GnHot));
    }
    return CF_OK;
}

// The record-slot path of the photometric term on its own, two launches as the schedule issues them for an rgb_only call: (a) the compact
// residual pass (launch_rgb_records_residual: the {ICP || residual} launch without its ICP half), (b) the RGB step over the slots it left
// (launch_rgb_slot_step: rgb_slot_step_kernel under cf_set_gn_mode 1, rgb_step_solve_kernel -- whose last workgroup solves -- under 2), on
// temporary device states, accumulators, record buffers and sync blocks filled from the caller's words.
int cf_rgb_records_step(cf_ctx* ctx, int n, cf_rgb_system* systems, int cols, int rows, float max_depth_delta, float sobel_scale, float fx, float fy,
                        int next_level, int last_of_level)
{
    if (!ctx || !systems || n < 1 || n > kMaxBatch || cols <= 0 || rows <= 0 || (cols % 4) || next_level < -1 || next_level > 2) return CF_EINVAL;
    const size_t N = (size_t)cols * rows;
    if (N > (size_t)ctx->cfg.width * ctx->cfg.height || N > (1u << 22)) return CF_EINVAL;   // (22-bit pixel index in the records)
    const int mode = ctx->gn_mode;
    if (mode == 0 || ctx->icp_arith == CF_ICP_ARITH_REFERENCE) { ctx->set_error("cf_rgb_records_step: the record slots exist under cf_set_gn_mode 1 and 2 of the fixed-point arithmetic only"); return CF_EINVAL; }
    if (mode == 2 && ctx->xcd_round_robin != 1) { ctx->set_error("cf_rgb_records_step: cf_set_gn_mode 2 needs workgroups dealt round-robin over 8 XCDs"); return CF_EINVAL; }
    for (int k = 0; k < n; k++) {
        const cf_rgb_system& y = systems[k];
        if (!y.cand || !y.next_depth || !y.last_depth || !y.last_image || !y.next_image || !y.cloud || !y.dIdx || !y.dIdy || !y.records || !y.slot_counts) return CF_EINVAL;
    }
    static_assert(sizeof(systems->hot) == sizeof(GnHot) && sizeof(systems->count_seed) == 8 * kGroups, "cf_rgb_system mirrors the hot block and the accumulator groups");
    constexpr size_t kAccWords = (size_t)kGroups * 32;
    const size_t rgb_words = rgb_acc_rows(N) * 32, acc_words = kAccWords + rgb_words;
    const int slot_px = ctx->icp_launch.threads * 4, n_slots = (int)((N + slot_px - 1) / slot_px);
    std::vector<OdomDev> h((size_t)n);   // (declared in front of buf: destroyed behind its synchronisation)
    std::vector<unsigned long long> seeds((size_t)n * kAccWords), acc_a((size_t)n * kAccWords), acc_b((size_t)n * kAccWords);
    std::vector<unsigned> ranges((size_t)n * 2);
    GnStepBuffers buf;
    buf.stream = ctx->stream;
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_states), sizeof(OdomDev) * n));
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_acc), 8 * acc_words * n));
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_recs), sizeof(cf_dataterm) * N * n));   // (a tracker's corres image: the records alias it)
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_range), sizeof(unsigned) * 2 * n));
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_sync), sizeof(So3Sync) * n));
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&buf.h_twins), sizeof(OdomDev) * n, hipHostMallocCoherent));  // the solve stores into them
    // the sums start from zero under mode 1 (grouped atomics add to them); under mode 2 every row read is a row stored by the same launch:
    // a pattern where the rows start
    HIPCHK(ctx, hipMemsetAsync(buf.d_acc, 0, 8 * acc_words * n, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(buf.d_recs, 0, sizeof(cf_dataterm) * N * n, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(buf.d_sync, 0, sizeof(So3Sync) * n, ctx->stream));   // (zero between launches)
    RgbArgs ra{};
    ra.cols = cols; ra.rows = rows; ra.il = cf_cam{fx, fy, 0, 0}; ra.sobelScale = sobel_scale; ra.maxDepthDelta = max_depth_delta;
    ra.compact = 1; ra.slot_px = slot_px;
    for (int k = 0; k < n; k++) {
        cf_rgb_system& y = systems[k];
        OdomDev* s = &h[(size_t)k];
        memset(s, 0, sizeof(*s));
        gn_state_to_dev(y.state, s);
        s->icp_acc = buf.d_acc + acc_words * k; s->rgb_acc = s->icp_acc + kAccWords;
        s->sobelScale = sobel_scale; s->maxDepthDeltaRGB = max_depth_delta;
        s->host_twin = &buf.h_twins[k];   // (what the solve of mode 2 publishes to when the schedule ends)
        refresh_hot(s);
        memset(&buf.h_twins[k], 0, sizeof(OdomDev));
        gn_state_to_dev(y.twin, &buf.h_twins[k]);
        if (mode == 2) HIPCHK(ctx, hipMemsetAsync(s->rgb_acc, 0xA5, 8 * rgb_words, ctx->stream));
        unsigned long long* seed = &seeds[(size_t)k * kAccWords];
        for (int g = 0; g < kGroups; g++) { seed[(size_t)g * 32 + 29] = (unsigned long long)y.count_seed[g]; seed[(size_t)g * 32 + 30] = (unsigned long long)y.sigma_seed[g]; }
        HIPCHK(ctx, hipMemcpyAsync(s->icp_acc, seed, 8 * kAccWords, hipMemcpyHostToDevice, ctx->stream));
        OdomDev level = *s;   // the level's view of the tracker for rgb_model_args: its images, its record buffer, its size
        level.width = cols; level.height = rows;
        level.cand[0] = y.cand; level.nextDepth[0] = y.next_depth; level.lastDepth[0] = y.last_depth; level.lastImage[0] = y.last_image;
        level.nextImage[0] = y.next_image; level.cloud[0] = y.cloud; level.dIdx[0] = y.dIdx; level.dIdy[0] = y.dIdy;
        level.corres[0] = buf.d_recs + N * k;
        level.res_range = y.ranged ? buf.d_range + 2 * k : nullptr;
        ra.m[k] = rgb_model_args(&level, buf.d_states + k, 0);
        ra.m[k].no_counts = y.no_counts ? 1 : 0;
        ra.m[k].res_blocks = y.ranged ? y.res_blocks : 0;
        ranges[(size_t)2 * k] = y.res_range[0]; ranges[(size_t)2 * k + 1] = y.res_range[1];
        HIPCHK(ctx, hipMemcpyAsync(ra.m[k].recs, y.records, 8 * N, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ra.m[k].slot_counts, y.slot_counts, sizeof(unsigned) * n_slots, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(buf.d_range, ranges.data(), sizeof(unsigned) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(buf.d_states, h.data(), sizeof(OdomDev) * n, hipMemcpyHostToDevice, ctx->stream));
    launch_rgb_records_residual(ctx->stream, ctx->icp_launch, ra, n, 0);                                   // (a)
    LAUNCHCHK(ctx);
    for (int k = 0; k < n; k++) {
        HIPCHK(ctx, hipMemcpyAsync(systems[k].records, ra.m[k].recs, 8 * N, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(systems[k].slot_counts, ra.m[k].slot_counts, sizeof(unsigned) * n_slots, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&acc_a[(size_t)k * kAccWords], ra.m[k].icp_acc, 8 * kAccWords, hipMemcpyDeviceToHost, ctx->stream));
    }
    launch_rgb_slot_step(ctx->stream, ra, buf.d_sync, n, mode, ctx->icp_launch.gram ? -1 : CF_FIX_ICP, next_level, last_of_level ? 1 : 0);   // (b)
    LAUNCHCHK(ctx);
    if (mode == 2) HIPCHK(ctx, hipMemcpyAsync(h.data(), buf.d_states, sizeof(OdomDev) * n, hipMemcpyDeviceToHost, ctx->stream));
    else for (int k = 0; k < n; k++)
        HIPCHK(ctx, hipMemcpyAsync(&acc_b[(size_t)k * kAccWords], ra.m[k].rgb_acc, 8 * kAccWords, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++) {
        cf_rgb_system& y = systems[k];
        unsigned long long c = 0, g2 = 0;
        for (int g = 0; g < kGroups; g++) { c += acc_a[(size_t)k * kAccWords + (size_t)g * 32 + 29]; g2 += acc_a[(size_t)k * kAccWords + (size_t)g * 32 + 30]; }
        y.count_total = (int64_t)c; y.sigma_total = (int64_t)g2;
        for (int w = 0; w < 32; w++) {
            unsigned long long t = 0;
            for (int g = 0; g < kGroups && mode != 2; g++) t += acc_b[(size_t)k * kAccWords + (size_t)g * 32 + w];
            y.rgb_sums[w] = (int64_t)t;   // (mode 2: the solve has consumed and cleared them)
        }
        if (mode == 2) {
            gn_state_from_dev(&h[(size_t)k], &y.state);
            gn_state_from_dev(&buf.h_twins[k], &y.twin);
            memcpy(y.hot, &h[(size_t)k].hot, sizeof(GnHot));
        } else memcpy(y.hot, &h[(size_t)k].hot, sizeof(GnHot));   // (no solve: the block the two launches read)
    }
    return CF_OK;
}

// The first launch of a tracking call on its own: so3_prealign_kernel as the schedule launches it (launch_so3_prealign), on temporary
// pinned host states filled from the caller's words and temporary device states filled with a pattern -- the launch uploads them.
int cf_so3_prealign_step(cf_ctx* ctx, int n, cf_so3_system* systems, int do_so3, int first_level)
{
    if (!ctx || !systems || n < 1 || n > kMaxBatch || n > ctx->cfg.max_models || first_level < 0 || first_level > 2) return CF_EINVAL;
    static_assert(sizeof(systems->sync) == sizeof(So3Sync) && sizeof(systems->hot) == sizeof(GnHot), "cf_so3_system mirrors the sync and the hot block");
    for (int k = 0; k < n; k++) {
        const cf_gn_state& g = systems[k].state_in;
        if (g.width <= 0 || g.height <= 0 || (g.width % 16) || (g.height % 4)) return CF_EINVAL;
        if (do_so3 && (!systems[k].last_next_image || !systems[k].next_image)) return CF_EINVAL;
    }
    std::vector<OdomDev> back((size_t)n);   // (declared in front of buf: destroyed behind its synchronisation)
    GnStepBuffers buf;
    buf.stream = ctx->stream;
    HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&buf.d_states), sizeof(OdomDev) * n));
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&buf.h_twins), sizeof(OdomDev) * n, hipHostMallocCoherent));  // the launch reads them
    HIPCHK(ctx, hipMemsetAsync(buf.d_states, 0xA5, sizeof(OdomDev) * n, ctx->stream));   // a word the launch does not upload keeps the pattern
    TrackerStates states{};
    for (int k = 0; k < n; k++) {
        OdomDev* s = &buf.h_twins[k];
        memset(s, 0, sizeof(*s));   // (cull 0, no bounding-box accumulator)
        gn_state_to_dev(systems[k].state_in, s);
        s->lastNextImage[2] = systems[k].last_next_image; s->nextImage[2] = systems[k].next_image;
        states.dev[k] = buf.d_states + k; states.host[k] = s;
    }
    launch_so3_prealign(ctx->stream, states, ctx->d_so3_sync, n, do_so3 != 0, first_level, nullptr);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(back.data(), buf.d_states, sizeof(OdomDev) * n, hipMemcpyDeviceToHost, ctx->stream));
    for (int k = 0; k < n; k++)
        HIPCHK(ctx, hipMemcpyAsync(systems[k].sync, ctx->d_so3_sync + k, sizeof(So3Sync), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++) {
        gn_state_from_dev(&back[(size_t)k], &systems[k].state_out);
        memcpy(systems[k].hot, &back[(size_t)k].hot, sizeof(GnHot));
    }
    return CF_OK;
}

}  // extern "C"
