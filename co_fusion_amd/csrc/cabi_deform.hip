// cabi_deform.hip -- C-ABI of the deformation graph (cf_deform_*; kernels in deform.hip).  Everything is allocated when the
// object is created; a closure allocates nothing.
#include <math.h>

#include <string>

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
static int assemble(cf_deform* d, int ldt)
{
    launch_deform_residual(d->ctx->cur(), d->g, d->n, d->n_cons, ldt);
    launch_deform_assemble(d->ctx->cur(), d->g, d->n, d->n_cons, ldt);
    LAUNCHCHK(d->ctx);
    return CF_OK;
}
static int iterate(cf_deform* d, int ldt, cf_deform_step* out)
{
    if (int r = assemble(d, ldt)) return r;
    launch_deform_solve(d->ctx->cur(), d->g, d->n);
    launch_deform_residual(d->ctx->cur(), d->g, d->n, d->n_cons, ldt);
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
    d->local_time = -1;
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
    d->local_time = -1;
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
    launch_deform_residual(d->ctx->cur(), d->g, d->n, d->n_cons, kDeformAllEnabled);
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

}  // extern "C"
