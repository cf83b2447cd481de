// cabi_deform.hip -- C-ABI of the deformation graph (cf_deform_*; kernels in deform.hip).  Everything is allocated when the
// object is created (the storage of relative constraints when cf_deform_enable_relative switches them on); a closure allocates nothing.
#include <math.h>

#include <string>
#include <vector>

#include "cf_host.h"
#include "cf_deform.h"

using namespace cf;

struct cf_deform {
    cf_ctx* ctx = nullptr;
    DeformGraph g{};
    DeformMeta* d_meta = nullptr;
    DeformMeta* h_meta = nullptr;   // pinned
    DeformOut* h_out = nullptr;     // pinned
    float4* h_cons = nullptr;       // pinned [2][max_cons]: sources, targets
    float* params0 = nullptr;       // device [kDeformMaxNodes][12]: the parameters cf_deform_optimise_local started from
    int n = 0, n_cons = 0, max_cons = kDeformMaxCons;
    int local_time = -1;            // last_deform_time of the cf_deform_optimise_local that left the parameters (-1: none since the graph was made)
    // relative constraints: off (rel.capacity == 0) until cf_deform_enable_relative
    DeformRel rel{};
    long long rel_total = 0;        // pairs ever appended: pair k lives in slot k mod capacity
    bool rel_ready = false;         // the weight sets and U belong to the ring and the nodes as they are
    int rel_used = 0;               // pairs in the system of the last cf_deform_optimise
    int rel_n() const { return rel.capacity && rel_total > rel.capacity ? rel.capacity : (int)rel_total; }
};

static int need_graph(cf_deform* d, const char* who)
{
    if (d->n >= kDeformMinNodes) return CF_OK;
    d->ctx->set_error(std::string(who) + ": no graph (fewer than 5 nodes; cf_deform_sample or cf_deform_set_nodes first)");
    return CF_ESTATE;
}
static int read_out(cf_deform* d)
{
    cf_ctx* ctx = d->ctx;
    HIPCHK(ctx, hipMemcpyAsync(d->h_out, d->g.out, sizeof(DeformOut), hipMemcpyDeviceToHost, ctx->cur()));
    HIPCHK(ctx, hipStreamSynchronize(ctx->cur()));
    return CF_OK;
}
// the relative rows take part when the ring holds pairs: in the global mode only (the reference gives them to the global graph alone)
static int relative_mode(cf_deform* d, int ldt, const char* who)
{
    if (d->rel_n() == 0) return CF_OK;
    if (ldt == kDeformAllEnabled) return CF_OK;
    d->ctx->set_error(std::string(who) + ": relative constraints are set and the graph's local mode does not take them");
    return CF_EINVAL;
}
static void residual(cf_deform* d, int ldt)
{
    const int nr = d->rel_n();
    if (nr == 0) { launch_deform_residual(d->ctx->cur(), d->g, d->n, d->n_cons, ldt); return; }
    if (!d->rel_ready) { launch_deform_rel_weights(d->ctx->cur(), d->g, d->rel, d->n, nr); d->rel_ready = true; }
    launch_deform_residual_rel(d->ctx->cur(), d->g, d->rel, d->n, d->n_cons, nr);
}
static int assemble(cf_deform* d, int ldt)
{
    residual(d, ldt);
    launch_deform_assemble(d->ctx->cur(), d->g, d->n, d->n_cons, ldt);
    if (const int nr = d->rel_n()) launch_deform_rel_rhs(d->ctx->cur(), d->g, d->rel, d->n, d->n_cons, nr);
    LAUNCHCHK(d->ctx);
    return CF_OK;
}
static int iterate(cf_deform* d, int ldt, cf_deform_step* out)
{
    if (int r = assemble(d, ldt)) return r;
    hipStream_t s = d->ctx->cur();
    if (const int nr = d->rel_n()) {
        launch_deform_solve_factor(s, d->g, d->n);
        launch_deform_rel_y(s, d->g, d->rel, d->n, nr);
        launch_deform_rel_gram(s, d->g, d->rel, d->n, nr);
        launch_deform_rel_c(s, d->g, d->rel, nr);
        launch_deform_rel_correct(s, d->g, d->rel, d->n, nr);
        launch_deform_solve_finish(s, d->g, d->n);
    } else launch_deform_solve(s, d->g, d->n);
    residual(d, ldt);
    LAUNCHCHK(d->ctx);
    if (int r = read_out(d)) return r;
    *out = cf_deform_step{d->h_out->error, d->h_out->delta_norm, d->h_out->failed, d->h_out->mean_cons_error};
    return CF_OK;
}

// constraint rows in device arrays of cf_deform_weights' host shapes (src, dst [n][3], time [n]) -> the graph's (x y z time), (x y z 0)
__global__ void __launch_bounds__(kDeformMaxCons) deform_pack_constraints_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                                                const float* __restrict__ time, int n, float4* __restrict__ cons_src,
                                                                                float4* __restrict__ cons_dst)
{
    const int l = (int)(blockIdx.x * kDeformMaxCons + threadIdx.x);
    if (l >= n) return;
    cons_src[l] = make_float4(src[3 * l], src[3 * l + 1], src[3 * l + 2], time[l]);
    cons_dst[l] = make_float4(dst[3 * l], dst[3 * l + 1], dst[3 * l + 2], 0.f);
}
// n pairs in device arrays of the same shapes -> the ring, pair k in slot (head + k) mod capacity
__global__ void __launch_bounds__(kDeformRelMax) deform_rel_store_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                                         const float* __restrict__ src_time, const float* __restrict__ dst_time, int n,
                                                                         DeformRel rel, int head)
{
    const int k = (int)threadIdx.x;
    if (k >= n) return;
    const int slot = (head + k) % rel.capacity;
    rel.src[slot] = make_float4(src[3 * k], src[3 * k + 1], src[3 * k + 2], src_time[k]);
    rel.dst[slot] = make_float4(dst[3 * k], dst[3 * k + 1], dst[3 * k + 2], dst_time[k]);
}
// the body cf_deform_weights and cf_deform_weights_device share: the n rows are in g.cons_src / g.cons_dst (enqueued)
static int weight_constraints(cf_deform* d, int n)
{
    cf_ctx* ctx = d->ctx;
    d->n_cons = n;
    if (n) {
        launch_deform_weights(ctx->cur(), d->g, d->n, n);
        LAUNCHCHK(ctx);
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->cur()));
    return CF_OK;
}

extern "C" {

void cf_deform_default_thresholds(cf_deform_thresholds* t)
{
    if (t) *t = cf_deform_thresholds{0.06f, 3, 1e-2f, 1e-3f, 1e-5f, 10.0f, 3e-4f, 0.12f};   // DeformationGraph.cpp:392-439, Deformation.cpp:134
}

void cf_deform_destroy(cf_deform* d)
{
    if (!d) return;
    (void)hipStreamSynchronize(d->ctx->cur());
    void* ptrs[] = {d->g.nodes, d->g.params, d->g.edges, d->g.cons_src, d->g.cons_dst, d->g.ids, d->g.w, d->g.AB, d->g.b, d->g.r, d->g.out, d->d_meta};
    for (void* p : ptrs) (void)hipFree(p);
    (void)hipFree(d->params0);
    void* rels[] = {d->rel.src, d->rel.dst, d->rel.ids, d->rel.w, d->rel.uid, d->rel.uval, d->rel.Y, d->rel.C, d->rel.Lc};
    for (void* p : rels) (void)hipFree(p);
    (void)hipHostFree(d->h_meta); (void)hipHostFree(d->h_out); (void)hipHostFree(d->h_cons);
    delete d;
}

int cf_deform_create(cf_ctx* ctx, cf_deform** out) { return cf_deform_create_sized(ctx, kDeformMaxCons, out); }

int cf_deform_create_sized(cf_ctx* ctx, int max_constraints, cf_deform** out)
{
    if (!ctx || !out || max_constraints < 1 || max_constraints > kDeformMaxConsSized) return CF_EINVAL;
    *out = nullptr;
    cf_deform* d = new cf_deform;
    d->ctx = ctx;
    d->max_cons = max_constraints;
    const size_t nv = (size_t)kDeformMaxNodes * kDeformVars, mc = (size_t)max_constraints;
    const size_t rows = (size_t)kDeformMaxNodes * 18 + mc * 3;
    int r = dmalloc(ctx, &d->g.nodes, kDeformMaxNodes);
    if (!r) r = dmalloc(ctx, &d->g.params, nv);
    if (!r) r = dmalloc(ctx, &d->g.edges, (size_t)kDeformMaxNodes * kDeformK);
    if (!r) r = dmalloc(ctx, &d->g.cons_src, mc);
    if (!r) r = dmalloc(ctx, &d->g.cons_dst, mc);
    if (!r) r = dmalloc(ctx, &d->g.ids, mc);
    if (!r) r = dmalloc(ctx, &d->g.w, mc);
    if (!r) r = dmalloc(ctx, &d->g.AB, nv * kDeformBand);
    if (!r) r = dmalloc(ctx, &d->g.b, nv);
    if (!r) r = dmalloc(ctx, &d->g.r, rows);
    if (!r) r = dmalloc(ctx, &d->g.out, 1);
    if (!r) r = dmalloc(ctx, &d->d_meta, 1);
    if (!r) r = dmalloc(ctx, &d->params0, nv);
    auto pinned = [&](void** p, size_t bytes) {
        if (r) return;
        const hipError_t e = hipHostMalloc(p, bytes);
        if (e != hipSuccess) { ctx->set_error(std::string("cf_deform_create: hipHostMalloc: ") + hipGetErrorString(e)); r = CF_EHIP; }
    };
    pinned(reinterpret_cast<void**>(&d->h_meta), sizeof(DeformMeta));
    pinned(reinterpret_cast<void**>(&d->h_out), sizeof(DeformOut));
    pinned(reinterpret_cast<void**>(&d->h_cons), sizeof(float4) * 2 * mc);
    if (!r && hipStreamSynchronize(ctx->cur()) != hipSuccess) { ctx->set_error("cf_deform_create: the fills failed"); r = CF_EHIP; }
    if (r) { cf_deform_destroy(d); return r; }
    *out = d;
    return CF_OK;
}

int cf_deform_sample(cf_deform* d, const float* map_dev, uint32_t count, int sample_rate, int* nodes, int* stride, int* monotone)
{
    if (!d || (!map_dev && count) || sample_rate < 1) return CF_EINVAL;
    cf_ctx* ctx = d->ctx;
    d->local_time = -1; d->rel_ready = false;
    if (reinterpret_cast<uintptr_t>(map_dev) & 15u) { ctx->set_error("cf_deform_sample: the map must be 16-byte aligned"); return CF_EINVAL; }
    uint64_t st = (uint64_t)sample_rate;
    while (((uint64_t)count + st - 1) / st > (uint64_t)kDeformMaxNodes) st += (uint64_t)sample_rate;
    d->n = 0; d->n_cons = 0;
    if (count) {
        launch_deform_sample(ctx->cur(), map_dev, count, (unsigned)st, d->g, d->d_meta);
        LAUNCHCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(d->h_meta, d->d_meta, sizeof(DeformMeta), hipMemcpyDeviceToHost, ctx->cur()));
        HIPCHK(ctx, hipStreamSynchronize(ctx->cur()));
    } else *d->h_meta = DeformMeta{0, 1};
    if (d->h_meta->count < 0 || d->h_meta->count > kDeformMaxNodes) { ctx->set_error("cf_deform_sample: node count out of range"); return CF_ESTATE; }
    d->n = d->h_meta->count;
    if (nodes) *nodes = d->n;
    if (stride) *stride = (int)st;
    if (monotone) *monotone = d->h_meta->monotone;
    return CF_OK;
}

int cf_deform_set_nodes(cf_deform* d, const float* nodes_host, const float* params_host, int n)
{
    if (!d || !nodes_host || n < 0 || n > kDeformMaxNodes) return CF_EINVAL;
    cf_ctx* ctx = d->ctx;
    d->local_time = -1; d->rel_ready = false;
    d->n = 0; d->n_cons = 0;
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(d->g.nodes, nodes_host, sizeof(float4) * n, hipMemcpyHostToDevice, ctx->cur()));
        if (params_host) HIPCHK(ctx, hipMemcpyAsync(d->g.params, params_host, sizeof(float) * kDeformVars * n, hipMemcpyHostToDevice, ctx->cur()));
        launch_deform_init_graph(ctx->cur(), d->g, n, params_host == nullptr);
        LAUNCHCHK(ctx);
        HIPCHK(ctx, hipStreamSynchronize(ctx->cur()));
    }
    d->n = n;
    return CF_OK;
}

int cf_deform_weights(cf_deform* d, const float* src, const float* dst, const float* src_time, int n)
{
    if (!d || n < 0 || n > d->max_cons || (n && (!src || !dst || !src_time))) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_weights")) return r;
    cf_ctx* ctx = d->ctx;
    HIPCHK(ctx, hipStreamSynchronize(ctx->cur()));   // (the staging block of the previous call)
    for (int l = 0; l < n; l++) {
        d->h_cons[l] = make_float4(src[3 * l], src[3 * l + 1], src[3 * l + 2], src_time[l]);
        d->h_cons[d->max_cons + l] = make_float4(dst[3 * l], dst[3 * l + 1], dst[3 * l + 2], 0.f);
    }
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(d->g.cons_src, d->h_cons, sizeof(float4) * n, hipMemcpyHostToDevice, ctx->cur()));
        HIPCHK(ctx, hipMemcpyAsync(d->g.cons_dst, d->h_cons + d->max_cons, sizeof(float4) * n, hipMemcpyHostToDevice, ctx->cur()));
    }
    return weight_constraints(d, n);
}

int cf_deform_weights_device(cf_deform* d, const float* src_dev, const float* dst_dev, const float* src_time_dev, int n)
{
    if (!d || n < 0 || n > d->max_cons || (n && (!src_dev || !dst_dev || !src_time_dev))) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_weights_device")) return r;
    if (n) {
        hipLaunchKernelGGL(deform_pack_constraints_kernel, dim3((n + kDeformMaxCons - 1) / kDeformMaxCons), dim3(kDeformMaxCons), 0, d->ctx->cur(), src_dev, dst_dev, src_time_dev, n,
                           d->g.cons_src, d->g.cons_dst);
        LAUNCHCHK(d->ctx);
    }
    return weight_constraints(d, n);
}

int cf_deform_assemble(cf_deform* d)
{
    if (!d) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_assemble")) return r;
    if (int r = assemble(d, kDeformAllEnabled)) return r;
    HIPCHK(d->ctx, hipStreamSynchronize(d->ctx->cur()));
    return CF_OK;
}

int cf_deform_assemble_local(cf_deform* d, int last_deform_time)
{
    if (!d) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_assemble_local")) return r;
    if (int r = relative_mode(d, last_deform_time, "cf_deform_assemble_local")) return r;
    if (int r = assemble(d, last_deform_time)) return r;
    HIPCHK(d->ctx, hipStreamSynchronize(d->ctx->cur()));
    return CF_OK;
}

int cf_deform_iterate(cf_deform* d, cf_deform_step* out)
{
    if (!d || !out) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_iterate")) return r;
    return iterate(d, kDeformAllEnabled, out);
}

int cf_deform_iterate_local(cf_deform* d, int last_deform_time, cf_deform_step* out)
{
    if (!d || !out) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_iterate_local")) return r;
    if (int r = relative_mode(d, last_deform_time, "cf_deform_iterate_local")) return r;
    return iterate(d, last_deform_time, out);
}

int cf_deform_optimise(cf_deform* d, const cf_deform_thresholds* th_in, cf_deform_result* out)
{
    if (!d || !out) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_optimise")) return r;
    d->local_time = -1;
    cf_deform_thresholds th;
    cf_deform_default_thresholds(&th);
    if (th_in) th = *th_in;
    d->rel_used = d->rel_n();
    residual(d, kDeformAllEnabled);
    LAUNCHCHK(d->ctx);
    if (int r = read_out(d)) return r;
    *out = cf_deform_result{0, 0, 0, 0, d->h_out->error, d->h_out->mean_cons_error, d->h_out->error, d->h_out->mean_cons_error};
    if (!(out->mean_cons_error_before >= th.min_cons_error)) return CF_OK;   // (no constraints: NaN, not optimised)
    out->optimised = 1;
    double last = (double)out->error;
    for (int it = 1; it <= th.max_iterations; it++) {
        cf_deform_step st;
        if (int r = iterate(d, kDeformAllEnabled, &st)) return r;
        out->iterations = it;
        if (st.failed) { out->failed = 1; return CF_OK; }
        out->error = st.error; out->mean_cons_error = st.mean_cons_error;
        const double e = (double)st.error;
        if (e > last || st.delta_norm < (double)th.min_delta || e < (double)th.min_error || fabs(e - last) < (double)th.min_change * e ||
            (it == 1 && e > (double)th.max_first_error))
            break;
        last = e;
    }
    out->accepted = out->mean_cons_error < th.accept_cons_error && out->error < th.accept_error;
    return CF_OK;
}

// optimiseGraphSparse(fernMatch = false): no 0.06 gate, no `error > 10` stop; Deformation::constrain accepts whatever it leaves
int cf_deform_optimise_local(cf_deform* d, int last_deform_time, const cf_deform_thresholds* th_in, cf_deform_result* out)
{
    if (!d || !out) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_optimise_local")) return r;
    if (int r = relative_mode(d, last_deform_time, "cf_deform_optimise_local")) return r;
    cf_ctx* ctx = d->ctx;
    d->local_time = last_deform_time < 0 ? -1 : last_deform_time;
    cf_deform_thresholds th;
    cf_deform_default_thresholds(&th);
    if (th_in) th = *th_in;
    const size_t pbytes = sizeof(float) * kDeformVars * (size_t)d->n;
    HIPCHK(ctx, hipMemcpyAsync(d->params0, d->g.params, pbytes, hipMemcpyDeviceToDevice, ctx->cur()));
    launch_deform_residual(ctx->cur(), d->g, d->n, d->n_cons, last_deform_time);
    LAUNCHCHK(ctx);
    if (int r = read_out(d)) return r;
    *out = cf_deform_result{0, 0, 0, 0, d->h_out->error, d->h_out->mean_cons_error, d->h_out->error, d->h_out->mean_cons_error};
    if (d->h_out->enabled <= 0) return CF_OK;   // every node is older than the last deformation: nothing to solve
    out->optimised = 1;
    double last = (double)out->error;
    for (int it = 1; it <= th.max_iterations; it++) {
        cf_deform_step st;
        if (int r = iterate(d, last_deform_time, &st)) return r;
        out->iterations = it;
        if (st.failed) {   // (a failed step leaves the parameters of ITS start; an earlier step of this call may have moved them)
            out->failed = 1;
            HIPCHK(ctx, hipMemcpyAsync(d->g.params, d->params0, pbytes, hipMemcpyDeviceToDevice, ctx->cur()));
            HIPCHK(ctx, hipStreamSynchronize(ctx->cur()));
            return CF_OK;
        }
        out->error = st.error; out->mean_cons_error = st.mean_cons_error;
        const double e = (double)st.error;
        if (e > last || st.delta_norm < (double)th.min_delta || e < (double)th.min_error || fabs(e - last) < (double)th.min_change * e) break;
        last = e;
    }
    out->accepted = 1;
    return CF_OK;
}

int cf_deform_apply(cf_deform* d, float* map_dev, uint32_t count, const cf_deform_reactivate* re)
{
    if (!d || (!map_dev && count)) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_apply")) return r;
    cf_ctx* ctx = d->ctx;
    if (reinterpret_cast<uintptr_t>(map_dev) & 15u) { ctx->set_error("cf_deform_apply: the map must be 16-byte aligned"); return CF_EINVAL; }
    DeformReactivate ra{};
    if (re) {
        if (!re->depth || re->cols <= 0 || re->rows <= 0) return CF_EINVAL;
        inv44f(re->pose, ra.t_inv);
        ra.cam = re->cam; ra.cols = re->cols; ra.rows = re->rows; ra.max_depth = re->max_depth; ra.depth = re->depth;
        ra.threshold = re->conf_threshold; ra.tick = (float)re->tick;
    }
    launch_deform_apply(ctx->cur(), d->g, d->n, map_dev, count, re ? &ra : nullptr, d->local_time);
    LAUNCHCHK(ctx);
    return CF_OK;
}

int cf_deform_apply_poses(cf_deform* d, float* poses_dev, const int32_t* times_dev, int n)
{
    if (!d || n < 0 || (n && (!poses_dev || !times_dev))) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_apply_poses")) return r;
    launch_deform_poses(d->ctx->cur(), d->g, d->n, poses_dev, times_dev, n);
    LAUNCHCHK(d->ctx);
    return CF_OK;
}

int cf_deform_download(cf_deform* d, int* n_nodes, int* n_constraints, float* nodes, float* params, int32_t* edges, int32_t* ids, float* weights,
                       double* A_band, double* b)
{
    if (!d) return CF_EINVAL;
    cf_ctx* ctx = d->ctx; hipStream_t s = ctx->cur();
    const size_t n = (size_t)d->n, c = (size_t)d->n_cons, nv = n * kDeformVars;
    if (n_nodes) *n_nodes = d->n;
    if (n_constraints) *n_constraints = d->n_cons;
    if (nodes && n) HIPCHK(ctx, hipMemcpyAsync(nodes, d->g.nodes, sizeof(float4) * n, hipMemcpyDeviceToHost, s));
    if (params && n) HIPCHK(ctx, hipMemcpyAsync(params, d->g.params, sizeof(float) * nv, hipMemcpyDeviceToHost, s));
    if (edges && n) HIPCHK(ctx, hipMemcpyAsync(edges, d->g.edges, sizeof(int) * kDeformK * n, hipMemcpyDeviceToHost, s));
    if (ids && c) HIPCHK(ctx, hipMemcpyAsync(ids, d->g.ids, sizeof(int4) * c, hipMemcpyDeviceToHost, s));
    if (weights && c) HIPCHK(ctx, hipMemcpyAsync(weights, d->g.w, sizeof(float4) * c, hipMemcpyDeviceToHost, s));
    if (A_band && n) HIPCHK(ctx, hipMemcpyAsync(A_band, d->g.AB, sizeof(double) * nv * kDeformBand, hipMemcpyDeviceToHost, s));
    if (b && n) HIPCHK(ctx, hipMemcpyAsync(b, d->g.b, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return CF_OK;
}

// ------------------------------------------------------------------------------------------------ relative constraints
int cf_deform_enable_relative(cf_deform* d, int capacity)
{
    if (!d || capacity < kDeformRelMin || capacity > kDeformRelMax) return CF_EINVAL;
    cf_ctx* ctx = d->ctx;
    if (d->rel.capacity) {
        if (d->rel.capacity == capacity) return CF_OK;
        ctx->set_error("cf_deform_enable_relative: already enabled with another capacity");
        return CF_ESTATE;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->cur()));
    const size_t cap = (size_t)capacity, nv = (size_t)kDeformMaxNodes * kDeformVars;
    DeformRel rel{};
    double* r_rows = nullptr;   // the residual rows grow by 3 per pair
    int r = dmalloc(ctx, &rel.src, cap);
    if (!r) r = dmalloc(ctx, &rel.dst, cap);
    if (!r) r = dmalloc(ctx, &rel.ids, 2 * cap);
    if (!r) r = dmalloc(ctx, &rel.w, 2 * cap);
    if (!r) r = dmalloc(ctx, &rel.uid, cap * kDeformRelSlots);
    if (!r) r = dmalloc(ctx, &rel.uval, cap * kDeformRelSlots * 4);
    if (!r) r = dmalloc(ctx, &rel.Y, 3 * cap * nv);
    if (!r) r = dmalloc(ctx, &rel.C, (size_t)kDeformRelLd * kDeformRelLd);
    if (!r) r = dmalloc(ctx, &rel.Lc, (size_t)kDeformRelLd * kDeformRelLd);
    if (!r) r = dmalloc(ctx, &r_rows, (size_t)kDeformMaxNodes * 18 + (size_t)d->max_cons * 3 + cap * 3);
    if (!r && hipStreamSynchronize(ctx->cur()) != hipSuccess) { ctx->set_error("cf_deform_enable_relative: the fills failed"); r = CF_EHIP; }
    if (r) {
        void* ptrs[] = {rel.src, rel.dst, rel.ids, rel.w, rel.uid, rel.uval, rel.Y, rel.C, rel.Lc, r_rows};
        for (void* p : ptrs) (void)hipFree(p);
        return r;
    }
    (void)hipFree(d->g.r);   // (scratch of one pass: nothing in it outlives a call)
    d->g.r = r_rows;
    rel.capacity = capacity;
    d->rel = rel;
    d->rel_total = 0; d->rel_ready = false; d->rel_used = 0;
    return CF_OK;
}

// pair k of the n new ones -> slot (total + k) mod capacity, from host arrays (staged on the device first) or device arrays of
// cf_deform_weights' shapes: one scatter launch either way
static int store_relative(cf_deform* d, const float* src, const float* dst, const float* src_time, const float* dst_time, int n, int append, bool device,
                          const char* who)
{
    if (!d || n < 0 || (n && (!src || !dst || !src_time || !dst_time))) return CF_EINVAL;
    cf_ctx* ctx = d->ctx;
    if (!d->rel.capacity) { ctx->set_error(std::string(who) + ": cf_deform_enable_relative first"); return CF_ESTATE; }
    if (n > d->rel.capacity) { ctx->set_error(std::string(who) + ": more pairs than the ring holds"); return CF_EINVAL; }
    if (!append) d->rel_total = 0;
    d->rel_ready = false;
    if (!n) return CF_OK;
    hipStream_t s = ctx->cur();
    if (!device) {   // (rel.uval is rewritten by the next step's rows launch: until then its first 8 n floats stage the host arrays)
        float* stage = reinterpret_cast<float*>(d->rel.uval);
        HIPCHK(ctx, hipStreamSynchronize(s));
        HIPCHK(ctx, hipMemcpy(stage, src, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(stage + 3 * n, dst, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(stage + 6 * n, src_time, sizeof(float) * n, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(stage + 7 * n, dst_time, sizeof(float) * n, hipMemcpyHostToDevice));
        src = stage; dst = stage + 3 * n; src_time = stage + 6 * n; dst_time = stage + 7 * n;
    }
    hipLaunchKernelGGL(deform_rel_store_kernel, dim3(1), dim3(kDeformRelMax), 0, s, src, dst, src_time, dst_time, n, d->rel, (int)(d->rel_total % d->rel.capacity));
    LAUNCHCHK(ctx);
    d->rel_total += n;
    if (!device) HIPCHK(ctx, hipStreamSynchronize(s));   // (the staging area is free again)
    return CF_OK;
}

int cf_deform_set_relative(cf_deform* d, const float* src, const float* dst, const float* src_time, const float* dst_time, int n, int append)
{
    return store_relative(d, src, dst, src_time, dst_time, n, append, false, "cf_deform_set_relative");
}

int cf_deform_set_relative_device(cf_deform* d, const float* src_dev, const float* dst_dev, const float* src_time_dev, const float* dst_time_dev, int n,
                                  int append)
{
    return store_relative(d, src_dev, dst_dev, src_time_dev, dst_time_dev, n, append, true, "cf_deform_set_relative_device");
}

int cf_deform_pick_relative(cf_deform* d, cf_deform* from, const float* src_dev, const float* dst_dev, const float* time_dev, const float* dst_time_dev,
                            int n, int row_stride, int* picked)
{
    if (!d || !from || n < 0 || row_stride < 1 || (n && (!src_dev || !dst_dev || !time_dev || !dst_time_dev))) return CF_EINVAL;
    cf_ctx* ctx = d->ctx;
    if (from->ctx != ctx) return CF_EINVAL;
    if (!d->rel.capacity) { ctx->set_error("cf_deform_pick_relative: cf_deform_enable_relative first"); return CF_ESTATE; }
    if (int r = need_graph(from, "cf_deform_pick_relative")) return r;
    const int step = n / 3 > 1 ? n / 3 : 1, picks = n ? (n + step - 1) / step : 0;
    if (picked) *picked = picks;
    if (!picks) return CF_OK;
    launch_deform_rel_pick(ctx->cur(), from->g, from->n, from->local_time, src_dev, dst_dev, time_dev, dst_time_dev, n, row_stride, d->rel,
                           (int)(d->rel_total % d->rel.capacity));
    LAUNCHCHK(ctx);
    d->rel_total += picks;
    d->rel_ready = false;
    return CF_OK;
}

int cf_deform_download_relative(cf_deform* d, int* capacity, int* count, int64_t* appended, int* used, float* pairs, int32_t* ids, float* weights,
                                int32_t* u_ids, double* u_vals, double* r_rel, double* C)
{
    if (!d) return CF_EINVAL;
    cf_ctx* ctx = d->ctx; hipStream_t s = ctx->cur();
    const int nr = d->rel_n();
    if (capacity) *capacity = d->rel.capacity;
    if (count) *count = nr;
    if (appended) *appended = (int64_t)d->rel_total;
    if (used) *used = d->rel_used;
    if (!nr) return CF_OK;
    const size_t c = (size_t)nr, cap = (size_t)d->rel.capacity, m = 3 * c;
    std::vector<float4> ring(2 * c);
    std::vector<double> dense;
    if (pairs) {
        HIPCHK(ctx, hipMemcpyAsync(ring.data(), d->rel.src, sizeof(float4) * c, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(ring.data() + c, d->rel.dst, sizeof(float4) * c, hipMemcpyDeviceToHost, s));
    }
    if (ids) {
        HIPCHK(ctx, hipMemcpyAsync(ids, d->rel.ids, sizeof(int4) * c, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(ids + 4 * c, d->rel.ids + cap, sizeof(int4) * c, hipMemcpyDeviceToHost, s));
    }
    if (weights) {
        HIPCHK(ctx, hipMemcpyAsync(weights, d->rel.w, sizeof(float4) * c, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(weights + 4 * c, d->rel.w + cap, sizeof(float4) * c, hipMemcpyDeviceToHost, s));
    }
    if (u_ids) HIPCHK(ctx, hipMemcpyAsync(u_ids, d->rel.uid, sizeof(int) * kDeformRelSlots * c, hipMemcpyDeviceToHost, s));
    if (u_vals) HIPCHK(ctx, hipMemcpyAsync(u_vals, d->rel.uval, sizeof(double) * kDeformRelSlots * 4 * c, hipMemcpyDeviceToHost, s));
    if (r_rel && d->n) HIPCHK(ctx, hipMemcpyAsync(r_rel, d->g.r + (size_t)18 * d->n + (size_t)3 * d->n_cons, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    if (C) {
        dense.resize((size_t)kDeformRelLd * (m + 1));
        HIPCHK(ctx, hipMemcpyAsync(dense.data(), d->rel.C, sizeof(double) * dense.size(), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (pairs)
        for (size_t k = 0; k < c; k++) {
            const float4 a = ring[k], b = ring[c + k];
            const float row[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            memcpy(pairs + 8 * k, row, sizeof(row));
        }
    if (C)   // the lower triangle of C as the device holds it, mirrored; then the row of Y^T y
        for (size_t i = 0; i <= m; i++)
            for (size_t j = 0; j < m; j++) C[i * m + j] = j <= i ? dense[i * kDeformRelLd + j] : dense[j * kDeformRelLd + i];
    return CF_OK;
}

int cf_deform_download_out(cf_deform* d, void* out32)
{
    if (!d || !out32) return CF_EINVAL;
    static_assert(sizeof(DeformOut) == 32, "the record a pass leaves is 32 bytes");
    if (int r = read_out(d)) return r;
    memcpy(out32, d->h_out, sizeof(DeformOut));
    return CF_OK;
}

int cf_deform_bench_relative_y(cf_deform* d)
{
    if (!d) return CF_EINVAL;
    if (int r = need_graph(d, "cf_deform_bench_relative_y")) return r;
    if (d->rel_n() == 0 || !d->rel_ready) { d->ctx->set_error("cf_deform_bench_relative_y: no pairs, or no cf_deform_iterate with them yet"); return CF_ESTATE; }
    launch_deform_rel_y(d->ctx->cur(), d->g, d->rel, d->n, d->rel_n());
    LAUNCHCHK(d->ctx);
    return CF_OK;
}

}  // extern "C"
