// local_loop.hip -- local (model-to-model) loop closure, the constraint stage (cf_local_loop_*; DESIGN.md 4.14 "The local half";
// tests/local_loop_ref.py restates it in numpy).  ONE launch of one workgroup behind the model-to-model tracker:
//
//   (a) the accept rule of CoFusion.cpp:407-422 from the tracker's result in device memory: every diagonal entry of the covariance
//       (the partial-pivot LU inverse of lastA in f64, the operation order of cf_odom_get_covariance) <= covThresh, lastICPCount >
//       icpCountThresh, lastICPError < icpErrThresh;
//   (b) when it accepts, the constraints of :423-443: the ACTIVE vertex map and the old time map sampled at texel (20 x + 10, 20 y + 10),
//       visited column by column, valid when z > 0 && z < maxDepth && oldTime > 0, compacted in that order with a ballot per wave and the
//       counts of the waves before (no atomics); src = currPose * p, dst = estPose * p (ElasticFusion's rule: the reference's text uses
//       currPose for both, which gives constraints of zero length), each coordinate ((m0 x + m1 y) + m2 z) + m3 in f32; srcTime = tick,
//       dstTime = the old time; with `pin` the pin row (dst, dst, dstTime) follows each constraint;
//   (c) one record in pinned host memory: plain stores, a system fence, the serial word last.
#include <string>

#include "cf_host.h"

using namespace cf;

namespace {

constexpr int kLocalT = 1024;          // threads of the workgroup = the most samples ((W / 20) * (H / 20): 768 at 640x480)
constexpr int kLocalMaxSamples = 768;  // with pins 1536 rows: the capacity of cf_deform_create_sized
constexpr int kConsSample = 20;

struct LocalArgs {
    const float* R; const float* t;        // the tracker's Rcurr [9], tcurr [3] (device)
    const cf_track_stats* stats;           // ... and its statistics (device)
    const float4* vertex; const unsigned short* old_time;   // ACTIVE splat vertexConf, INACTIVE time [rows * cols]
    const unsigned* covered;               // nullable: the covered-texel word of the inactive prediction, copied into the record
    float curr[16];
    int cols, rows, tick, pin;
    float max_depth, cov_thresh, icp_err_thresh; int icp_count_thresh;
    float *src, *dst, *time;               // f32 [1536][3], [1536][3], [1536]
    float* ttime;                          // f32 [768]: the old time of every constraint (pin rows excluded), pinned or not
    unsigned serial;
};

__device__ __forceinline__ float3 mul_pose(const float* m, float x, float y, float z)
{
    return make_float3(((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
                       ((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
}

// the diagonal of inverse(lastA): cf_odom_get_covariance's operations in its order (f64, no contraction)
__device__ void covariance_diagonal(const double* A, double (&diag)[6])
{
    constexpr int N = 6;
    double lu[N * N];
    int perm[N];
    for (int i = 0; i < N * N; i++) lu[i] = A[i];
    for (int i = 0; i < N; i++) perm[i] = i;
    for (int k = 0; k < N; k++) {
        int piv = k;
        double big = fabs(lu[k * N + k]);
        for (int r = k + 1; r < N; r++) { const double a = fabs(lu[r * N + k]); if (a > big) { big = a; piv = r; } }
        if (piv != k) {
            for (int c = 0; c < N; c++) { const double v = lu[k * N + c]; lu[k * N + c] = lu[piv * N + c]; lu[piv * N + c] = v; }
            const int v = perm[k]; perm[k] = perm[piv]; perm[piv] = v;
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
        diag[j] = x[j];
    }
}

// Every thread reaches every barrier: no early exit before the last one.
__global__ void __launch_bounds__(kLocalT) local_constraints_kernel(const LocalArgs a, cf_local_loop_record* __restrict__ out)
{
    __shared__ int s_accept;
    __shared__ int wave_n[kLocalT / 64];
    __shared__ float est[16];
    const int tid = (int)threadIdx.x;
    if (tid == 0) {
        double diag[6];
        covariance_diagonal(a.stats->lastA, diag);
        bool cov_ok = true;
        double worst = diag[0];
        for (int i = 0; i < 6; i++) {
            if (!(diag[i] <= (double)a.cov_thresh)) cov_ok = false;   // (NaN: rejected)
            if (diag[i] != diag[i] || (worst == worst && diag[i] > worst)) worst = diag[i];   // the largest entry, a NaN if there is one
        }
        const float count = a.stats->last_icp_count, err = a.stats->last_icp_error;
        const int accepted = cov_ok && count > (float)a.icp_count_thresh && err < a.icp_err_thresh;
        s_accept = accepted;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) est[4 * r + c] = a.R[3 * r + c];
            est[4 * r + 3] = a.t[r];
        }
        est[12] = 0.f; est[13] = 0.f; est[14] = 0.f; est[15] = 1.f;
        out->accepted = accepted;
        out->max_covariance = worst; out->icp_count = count; out->icp_error = err;
        for (int k = 0; k < 16; k++) out->est_pose[k] = est[k];
        out->covered = a.covered ? *a.covered : 0u;
    }
    __syncthreads();
    const int dw = a.cols / kConsSample, dh = a.rows / kConsSample;
    const int i = tid / dh, j = tid - i * dh;   // column by column: columns outer, rows inner
    bool valid = false;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned short ot = 0;
    if (s_accept && tid < dw * dh) {
        const size_t q = (size_t)(kConsSample * j + kConsSample / 2) * a.cols + (kConsSample * i + kConsSample / 2);
        v = a.vertex[q]; ot = a.old_time[q];
        valid = v.z > 0.f && v.z < a.max_depth && ot > 0;
    }
    const unsigned long long mask = __ballot(valid);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kLocalT / 64; w++) { const int n = wave_n[w]; before += w < wave ? n : 0; total += n; }
    if (valid) {
        const int stride = a.pin ? 2 : 1;
        const int row = stride * (before + __popcll(mask & ((1ull << lane) - 1ull)));
        const float3 s = mul_pose(a.curr, v.x, v.y, v.z), d = mul_pose(est, v.x, v.y, v.z);
        float* ps = a.src + 3 * row; float* pd = a.dst + 3 * row;
        ps[0] = s.x; ps[1] = s.y; ps[2] = s.z; pd[0] = d.x; pd[1] = d.y; pd[2] = d.z;
        a.time[row] = (float)a.tick;
        a.ttime[row / stride] = (float)ot;
        if (a.pin) {
            ps[3] = d.x; ps[4] = d.y; ps[5] = d.z; pd[3] = d.x; pd[4] = d.y; pd[5] = d.z;
            a.time[row + 1] = (float)ot;
        }
    }
    if (tid == 0) {
        out->n_constraints = (a.pin ? 2 : 1) * total;
        __threadfence_system();
        __hip_atomic_store(&out->serial, a.serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

struct cf_local_loop {
    cf_ctx* ctx = nullptr;
    cf_local_loop_record* h_rec = nullptr;   // pinned: written by the kernel
    float *src = nullptr, *dst = nullptr, *time = nullptr, *ttime = nullptr;
    void* d_in = nullptr;                    // [R 9 | t 3 f32][cf_track_stats]: a tracker result handed in from the host (tests)
    hipEvent_t event = nullptr;
    unsigned serial = 0;
    bool pending = false;
};

constexpr size_t kInStats = 64;   // offset of the statistics in d_in (8-byte aligned, behind the 12 floats)

extern "C" {

void cf_local_loop_destroy(cf_local_loop* l)
{
    if (!l) return;
    (void)hipStreamSynchronize(l->ctx->stream);
    (void)hipFree(l->src); (void)hipFree(l->dst); (void)hipFree(l->time); (void)hipFree(l->ttime); (void)hipFree(l->d_in);
    (void)hipHostFree(l->h_rec);
    if (l->event) (void)hipEventDestroy(l->event);
    delete l;
}

int cf_local_loop_create(cf_ctx* ctx, cf_local_loop** out)
{
    if (!ctx || !out) return CF_EINVAL;
    *out = nullptr;
    const int samples = (ctx->cfg.width / kConsSample) * (ctx->cfg.height / kConsSample);
    if (samples < 1 || samples > kLocalMaxSamples) {
        ctx->set_error("cf_local_loop_create: (width / 20) * (height / 20) must lie in 1..768");
        return CF_EINVAL;
    }
    cf_local_loop* l = new cf_local_loop;
    l->ctx = ctx;
    const size_t rows = 2 * (size_t)kLocalMaxSamples;
    int r = dmalloc(ctx, &l->src, rows * 3);
    if (!r) r = dmalloc(ctx, &l->dst, rows * 3);
    if (!r) r = dmalloc(ctx, &l->time, rows);
    if (!r) r = dmalloc(ctx, &l->ttime, (size_t)kLocalMaxSamples);
    if (!r && hipMalloc(&l->d_in, kInStats + sizeof(cf_track_stats)) != hipSuccess) r = CF_ENOMEM;
    if (!r && hipHostMalloc(reinterpret_cast<void**>(&l->h_rec), sizeof(cf_local_loop_record)) != hipSuccess) r = CF_ENOMEM;
    if (!r && hipEventCreateWithFlags(&l->event, hipEventDisableTiming) != hipSuccess) r = CF_EHIP;
    if (r) { ctx->set_error("cf_local_loop_create: allocation failed"); cf_local_loop_destroy(l); return r; }
    memset(l->h_rec, 0, sizeof(cf_local_loop_record));
    *out = l;
    return CF_OK;
}

int cf_local_loop_constraints_async(cf_local_loop* l, const cf_odom* od, const cf_local_loop_track* track, const float* vertex_conf_dev,
                                    const uint16_t* old_time_dev, const uint32_t* covered_dev, const float curr_pose[16], int tick,
                                    float max_depth, int pin, const cf_local_loop_thresholds* th)
{
    if (!l || (!od == !track) || !vertex_conf_dev || !old_time_dev || !curr_pose || !th) return CF_EINVAL;
    cf_ctx* ctx = l->ctx;
    hipStream_t s = ctx->stream;   // the tracker's (cf_odom_init_*, cf_odom_track_batch_async), whatever lane the calling thread is bound to
    LocalArgs a{};
    if (od) {
        a.R = od->d_state->Rcurr; a.t = od->d_state->tcurr; a.stats = &od->d_state->stats;
    } else {
        if (l->pending) HIPCHK(ctx, hipEventSynchronize(l->event));   // (the staging copies below read caller memory at enqueue time)
        float rt[12];
        memcpy(rt, track->rot, 36); memcpy(rt + 9, track->trans, 12);
        cf_track_stats st{};
        st.last_icp_error = track->icp_error; st.last_icp_count = track->icp_count;
        memcpy(st.lastA, track->lastA, sizeof(st.lastA));
        HIPCHK(ctx, hipMemcpy(l->d_in, rt, sizeof(rt), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(static_cast<char*>(l->d_in) + kInStats, &st, sizeof(st), hipMemcpyHostToDevice));
        a.R = static_cast<const float*>(l->d_in); a.t = a.R + 9;
        a.stats = reinterpret_cast<const cf_track_stats*>(static_cast<const char*>(l->d_in) + kInStats);
    }
    a.vertex = reinterpret_cast<const float4*>(vertex_conf_dev); a.old_time = old_time_dev; a.covered = covered_dev;
    memcpy(a.curr, curr_pose, sizeof(a.curr));
    a.cols = ctx->cfg.width; a.rows = ctx->cfg.height; a.tick = tick; a.pin = pin ? 1 : 0;
    a.max_depth = max_depth; a.cov_thresh = th->cov_thresh; a.icp_err_thresh = th->icp_err_thresh; a.icp_count_thresh = th->icp_count_thresh;
    a.src = l->src; a.dst = l->dst; a.time = l->time; a.ttime = l->ttime;
    a.serial = ++l->serial;
    hipLaunchKernelGGL(local_constraints_kernel, dim3(1), dim3(kLocalT), 0, s, a, l->h_rec);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipEventRecord(l->event, s));
    l->pending = true;
    return CF_OK;
}

int cf_local_loop_wait(cf_local_loop* l, cf_local_loop_record* out)
{
    if (!l || !out) return CF_EINVAL;
    if (!l->pending) { l->ctx->set_error("cf_local_loop_wait: nothing enqueued (cf_local_loop_constraints_async first)"); return CF_ESTATE; }
    HIPCHK(l->ctx, hipEventSynchronize(l->event));
    l->pending = false;
    *out = *l->h_rec;
    if (out->serial != l->serial) { l->ctx->set_error("cf_local_loop_wait: the record does not carry the serial of the last launch"); return CF_ESTATE; }
    return CF_OK;
}

int cf_local_loop_constraint_buffers(cf_local_loop* l, float** src, float** dst, float** time)
{
    if (!l) return CF_EINVAL;
    if (src) *src = l->src;
    if (dst) *dst = l->dst;
    if (time) *time = l->time;
    return CF_OK;
}

int cf_local_loop_target_times(cf_local_loop* l, float** target_time)
{
    if (!l || !target_time) return CF_EINVAL;
    *target_time = l->ttime;
    return CF_OK;
}

}  // extern "C"
