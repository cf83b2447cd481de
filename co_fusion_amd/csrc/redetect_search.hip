// redetect_search.hip -- re-detection of objects that MOVED while unseen (CoFusion::setRedetectionSearch, DESIGN.md 4.13 "Search"):
// from "a new label appeared" to a pose hypothesis inside the tracker's gates, and a pose-independent colour check.
// tests/redetect_search_ref.py restates every line in numpy.
//
//   frame_moments_kernel   the pixels of the new label: their number, the sum of their vertices (createVMap's arithmetic) and a 512-bin
//                          histogram of their colours (top three bits of R, G, B)
//   model_moments_kernel   up to 16 candidate maps in one launch (the slot table of redetect_score_kernel): number and position sum of the
//                          stable surfels that face the camera under the static hypothesis (normal along the viewing ray: the maps' sign), colour histogram of all stable surfels
//   register_step_kernel   one candidate at one pose: the 29 sums of a point-to-plane Gauss-Newton step whose twist is taken about the
//                          label's centroid, over the surfels that land on the label within depth_tol of the frame's vertex
//   redetect_register_solve  the damped solve and pose update of one such step: host f64 from the exact sums
//
// Every device result is an integer: counts, sums of values rounded ONCE to a fixed-point grid (2^-16 for positions, 2^-32 for the
// products of the step).  Integer sums do not depend on launch shape or on the order the atomics land in.  Per-element arithmetic is
// plain f32, one operation per statement.
#include "cf_surfel_device.h"
#include "cf_kernels.h"

#include <math.h>

namespace cf {

static constexpr int kSB = 256;              // threads per workgroup (4 waves)
static constexpr int kPerThread = 8;         // elements a thread walks (grid-stride) when the host's bound is exact
static constexpr float kPosLim = 64.0f;      // positions are clamped to +-64 m, then rounded to 2^-16 m
static constexpr float kPosScale = 65536.0f;
static constexpr float kRowLim = 4.0f;       // entries of a step row are clamped to +-4 (an object-sized lever never gets there)

// K 64-bit values summed over the workgroup, each added to dst[k] by ONE atomic (none when the sum is zero).  Every thread calls it.
template <int K>
__device__ __forceinline__ void block_add64(const unsigned long long (&v)[K], unsigned long long* __restrict__ dst)
{
    __shared__ unsigned long long part[K][kSB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        unsigned long long s = v[k];
        for (int o = 32; o > 0; o >>= 1) s += shfl_xor_u64(s, o);
        if (lane == 0) part[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kSB / 64; w++) s += part[threadIdx.x][w];
        if (s) atomicAdd(&dst[threadIdx.x], s);
    }
}

// the workgroup's histogram (LDS) into the global one: an atomic per non-zero bin
__device__ __forceinline__ void hist_commit(const unsigned* h, unsigned* __restrict__ dst)
{
    __syncthreads();
    for (int b = threadIdx.x; b < kRedetectBins; b += kSB) {
        const unsigned n = h[b];
        if (n) atomicAdd(&dst[b], n);
    }
}
__device__ __forceinline__ void hist_clear(unsigned* h)
{
    for (int b = threadIdx.x; b < kRedetectBins; b += kSB) h[b] = 0;
    __syncthreads();
}
__device__ __forceinline__ int colour_bin(unsigned r, unsigned g, unsigned b) { return (int)(((r >> 5) << 6) | ((g >> 5) << 3) | (b >> 5)); }

__device__ __forceinline__ long long pos_fix(float x)
{
    float c = fmaxf(x, -kPosLim);
    c = fminf(c, kPosLim);
    return (long long)rintf(c * kPosScale);   // (a power-of-two scale: exact; |value| <= 2^22)
}

// the vertex createVMap gives pixel (px, py) for depth d (track_prep.hip: vmap_kernel)
__device__ __forceinline__ f3 pixel_vertex(int px, int py, float d, cf_cam cam, float fx_inv, float fy_inv)
{
    const float x = d * ((float)px - cam.cx) * fx_inv;
    const float y = d * ((float)py - cam.cy) * fy_inv;
    return f3{x, y, d};
}

__global__ void __launch_bounds__(kSB) frame_moments_kernel(const RedetectFrame f, const uint8_t* __restrict__ rgba, unsigned long long* __restrict__ moments,
                                                            unsigned* __restrict__ hist)
{
    __shared__ unsigned h[kRedetectBins];
    hist_clear(h);
    const float fx_inv = 1.0f / f.cam.fx, fy_inv = 1.0f / f.cam.fy;
    const unsigned n_px = (unsigned)(f.cols * f.rows);
    const uchar4* __restrict__ c4 = reinterpret_cast<const uchar4*>(rgba);
    unsigned long long m[kMomentWords] = {0, 0, 0, 0};
    for (unsigned i = blockIdx.x * kSB + threadIdx.x; i < n_px; i += gridDim.x * kSB) {
        if ((int)f.label[i] != f.new_label) continue;
        const float d = f.depth[i];
        if (!(d > 0.0f) || d > f.cutoff) continue;
        const int py = (int)(i / (unsigned)f.cols), px = (int)(i - (unsigned)py * (unsigned)f.cols);
        const f3 v = pixel_vertex(px, py, d, f.cam, fx_inv, fy_inv);
        m[0] += 1;
        m[1] += (unsigned long long)pos_fix(v.x);
        m[2] += (unsigned long long)pos_fix(v.y);
        m[3] += (unsigned long long)pos_fix(v.z);
        const uchar4 c = c4[i];
        atomicAdd(&h[colour_bin(c.x, c.y, c.z)], 1u);
    }
    hist_commit(h, hist);
    block_add64(m, moments);
}

struct ModelMomentsArgs {
    RedetectCand c[kRedetectBatch];
    int slot_end[kRedetectBatch];    // running totals of the workgroups per candidate; unused slots end at INT_MAX
    float dhat[3];                   // unit vector camera -> centroid of the label
    unsigned long long* moments;     // [kRedetectBatch][kMomentWords], zero on entry
    unsigned* hist;                  // [kRedetectBatch][kRedetectBins], zero on entry
};

__global__ void __launch_bounds__(kSB) model_moments_kernel(const ModelMomentsArgs a)
{
    __shared__ unsigned h[kRedetectBins];
    hist_clear(h);
    const int b = (int)blockIdx.x;
    int slot = 0;
#pragma unroll
    for (int k = 0; k < kRedetectBatch - 1; k++) slot += (b >= a.slot_end[k]) ? 1 : 0;
    const int start = slot ? a.slot_end[slot - 1] : 0;
    const unsigned bid = (unsigned)(b - start), nblk = (unsigned)(a.slot_end[slot] - start);
    const RedetectCand& c = a.c[slot];
    const float4* __restrict__ surfels = reinterpret_cast<const float4*>(c.surfels);
    unsigned count = *c.count;
    if (count > c.count_bound) count = c.count_bound;
    Mat4 T;
#pragma unroll
    for (int k = 0; k < 16; k++) T.m[k] = c.t_inv[k];
    const f3 dhat{a.dhat[0], a.dhat[1], a.dhat[2]};
    unsigned long long m[kMomentWords] = {0, 0, 0, 0};
    for (unsigned i = bid * kSB + threadIdx.x; i < count; i += nblk * kSB) {
        const float4 pc = surfels[(size_t)i * 3];
        if (!(pc.w >= c.theta)) continue;
        const float4 ct = surfels[(size_t)i * 3 + 1], nr = surfels[(size_t)i * 3 + 2];
        const int ci = (int)ct.x;   // decode_color (cf_surfel_device.h) before its division by 255
        atomicAdd(&h[colour_bin((unsigned)(ci >> 16) & 255u, (unsigned)(ci >> 8) & 255u, (unsigned)ci & 255u)], 1u);
        const f3 n = xform_dir(T, f3{nr.x, nr.y, nr.z});
        if (!(dot(n, dhat) > 0.0f)) continue;   // (the maps' normals point AWAY from the camera that saw them: createNMap's sign)
        m[0] += 1;
        m[1] += (unsigned long long)pos_fix(pc.x);
        m[2] += (unsigned long long)pos_fix(pc.y);
        m[3] += (unsigned long long)pos_fix(pc.z);
    }
    hist_commit(h, a.hist + (size_t)slot * kRedetectBins);
    block_add64(m, a.moments + (size_t)slot * kMomentWords);
}

__device__ __forceinline__ float row_clamp(float v)
{
    const float c = fmaxf(v, -kRowLim);
    return fminf(c, kRowLim);
}

// c.t_inv: T(camera <- model), the pose the step is taken at; out: [kSE3Words], zero on entry (word layout: se3_unpack -- row i of the
// upper triangle of [J | r]^T [J | r] for i < 6, then sum r^2, then the inlier count)
__global__ void __launch_bounds__(kSB) register_step_kernel(const RedetectCand c, const RedetectFrame f, const f3 centre, unsigned long long* __restrict__ out)
{
    const float4* __restrict__ surfels = reinterpret_cast<const float4*>(c.surfels);
    unsigned count = *c.count;
    if (count > c.count_bound) count = c.count_bound;
    Mat4 T;
#pragma unroll
    for (int k = 0; k < 16; k++) T.m[k] = c.t_inv[k];
    const float fx_inv = 1.0f / f.cam.fx, fy_inv = 1.0f / f.cam.fy;
    unsigned long long acc[kSE3Words];
#pragma unroll
    for (int k = 0; k < kSE3Words; k++) acc[k] = 0;
    for (unsigned i = blockIdx.x * kSB + threadIdx.x; i < count; i += gridDim.x * kSB) {
        const float4 pc = surfels[(size_t)i * 3];
        if (!(pc.w >= c.theta)) continue;
        f3 p; int q;
        if (!surfel_project(pc, T, f.cam, f.cols, f.rows, f.cutoff, p, q)) continue;
        if ((int)f.label[q] != f.new_label) continue;
        const float d = f.depth[q];
        if (!(d > 0.0f) || d > f.cutoff) continue;
        const int py = q / f.cols, px = q - py * f.cols;
        const f3 v = pixel_vertex(px, py, d, f.cam, fx_inv, fy_inv);
        const f3 diff = v - p;
        const float dist = sqrtf(dot(diff, diff));
        if (!(dist <= f.tol)) continue;
        const float4 nr = surfels[(size_t)i * 3 + 2];
        const f3 n = xform_dir(T, f3{nr.x, nr.y, nr.z});
        if (!(dot(n, p) > 0.0f)) continue;
        const f3 lever = p - centre;
        const f3 cr = cross(lever, n);
        const float r = dot(n, diff);
        const float row[7] = {row_clamp(n.x), row_clamp(n.y), row_clamp(n.z), row_clamp(cr.x), row_clamp(cr.y), row_clamp(cr.z), row_clamp(r)};
        int w = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double sa = (double)row[a] * 4294967296.0;
#pragma unroll
            for (int b = a; b < 7; b++) acc[w++] += fix_bits<kFixICP>(sa, (double)row[b]) - kMagicBits;
        }
        acc[27] += fix_bits<kFixICP>((double)row[6] * 4294967296.0, (double)row[6]) - kMagicBits;
        acc[28] += 1;
    }
    // wave totals by the transpose-reduce (lane l: word (l >> 1) & 31), the workgroup's in LDS, one atomic per non-zero word
    __shared__ unsigned long long part[kSB / 64][kSE3Words];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long t = wave_reduce32_u64(acc, lane);
    if ((lane & 1) == 0) part[wave][lane >> 1] = t;
    __syncthreads();
    if (threadIdx.x < kSE3Words) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kSB / 64; w++) s += part[w][threadIdx.x];
        if (s) atomicAdd(&out[threadIdx.x], s);
    }
}

static int blocks_for(long long n)
{
    long long blocks = (n + kSB * kPerThread - 1) / (kSB * kPerThread);
    return (int)(blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks);
}

void launch_redetect_frame_moments(hipStream_t s, const RedetectFrame& f, const uint8_t* rgba, unsigned long long* moments, unsigned* hist)
{
    hipLaunchKernelGGL(frame_moments_kernel, dim3(blocks_for((long long)f.cols * f.rows)), dim3(kSB), 0, s, f, rgba, moments, hist);
}

void launch_redetect_model_moments(hipStream_t s, const RedetectCand* cands, int n, const float dhat[3], unsigned long long* moments, unsigned* hist)
{
    ModelMomentsArgs a{};
    int total = 0;
    for (int k = 0; k < kRedetectBatch; k++) {
        if (k < n) {
            a.c[k] = cands[k];
            total += blocks_for((long long)cands[k].count_bound);   // (an empty candidate keeps one workgroup: its slot must exist)
        }
        a.slot_end[k] = k < n ? total : 0x7fffffff;
    }
    for (int k = 0; k < 3; k++) a.dhat[k] = dhat[k];
    a.moments = moments; a.hist = hist;
    hipLaunchKernelGGL(model_moments_kernel, dim3(total), dim3(kSB), 0, s, a);
}

void launch_redetect_register_step(hipStream_t s, const RedetectCand& c, const RedetectFrame& f, const float centre[3], unsigned long long* out)
{
    hipLaunchKernelGGL(register_step_kernel, dim3(blocks_for((long long)c.count_bound)), dim3(kSB), 0, s, c, f, f3{centre[0], centre[1], centre[2]}, out);
}

// ---- the host half of a step: f64, every operation spelled out (tests/redetect_search_ref.py: solve_step) ----
// sin / cos of cf_device.h's det_sincos: the same polynomials, so that the host loop does not depend on a C library
static void det_sincos_host(double x, double* s, double* c)
{
    const double two_over_pi = 0.63661977236758134308;
    const double pio2_1 = 1.57079632673412561417e+00;
    const double pio2_1t = 6.07710050650619224932e-11;
    const double fn = rint(x * two_over_pi);
    const double r = (x - fn * pio2_1) - fn * pio2_1t;
    const long long n = (long long)fn;
    const double r2 = r * r;
    double sp = -1.0 / 355687428096000.0;
    sp = sp * r2 + 1.0 / 1307674368000.0;
    sp = sp * r2 - 1.0 / 6227020800.0;
    sp = sp * r2 + 1.0 / 39916800.0;
    sp = sp * r2 - 1.0 / 362880.0;
    sp = sp * r2 + 1.0 / 5040.0;
    sp = sp * r2 - 1.0 / 120.0;
    sp = sp * r2 + 1.0 / 6.0;
    const double sr = r - r * r2 * sp;
    double cp = 1.0 / 20922789888000.0;
    cp = cp * r2 - 1.0 / 87178291200.0;
    cp = cp * r2 + 1.0 / 479001600.0;
    cp = cp * r2 - 1.0 / 3628800.0;
    cp = cp * r2 + 1.0 / 40320.0;
    cp = cp * r2 - 1.0 / 720.0;
    cp = cp * r2 + 1.0 / 24.0;
    cp = cp * r2 - 1.0 / 2.0;
    const double cr = 1.0 + r2 * cp;
    switch ((int)(n & 3)) {
        case 0: *s = sr; *c = cr; break;
        case 1: *s = cr; *c = -sr; break;
        case 2: *s = -sr; *c = -cr; break;
        default: *s = -cr; *c = sr; break;
    }
}

static double norm3(const double v[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

bool redetect_register_solve(const long long sums[kSE3Words], double lambda, const double centre[3], double R[9], double t[3], double* tau_norm, double* omega_norm)
{
    double A[6][6], b[6];
    int w = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 7; j++) {
            const double v = ldexp((double)sums[w++], -kFixICP);
            if (j == 6) b[i] = v;
            else { A[i][j] = v; A[j][i] = v; }
        }
    double tr = A[0][0];
    for (int i = 1; i < 6; i++) tr = tr + A[i][i];
    const double mu = (lambda * tr) / 6.0;
    for (int i = 0; i < 6; i++) A[i][i] = A[i][i] + mu;
    double L[6][6] = {};
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
        for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; i++) {
            double u = A[i][j];
            for (int k = 0; k < j; k++) u = u - L[i][k] * L[j][k];
            L[i][j] = u / L[j][j];
        }
    }
    double y[6], x[6];
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    const double tau[3] = {x[0], x[1], x[2]}, om[3] = {x[3], x[4], x[5]};
    const double theta = norm3(om);
    double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (theta >= 2.2204460492503131e-16) {
        double sn, cs;
        det_sincos_host(theta, &sn, &cs);
        const double c1 = 1.0 - cs, it = 1.0 / theta;
        const double rx = om[0] * it, ry = om[1] * it, rz = om[2] * it;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int k = 0; k < 9; k++) E[k] = (cs * I[k] + c1 * rrt[k]) + sn * r_x[k];
    }
    double Rn[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = E[i * 3] * R[j];
            s = s + E[i * 3 + 1] * R[3 + j];
            s = s + E[i * 3 + 2] * R[6 + j];
            Rn[i * 3 + j] = s;
        }
    const double u[3] = {t[0] - centre[0], t[1] - centre[1], t[2] - centre[2]};
    for (int i = 0; i < 3; i++) {
        double s = E[i * 3] * u[0];
        s = s + E[i * 3 + 1] * u[1];
        s = s + E[i * 3 + 2] * u[2];
        s = s + centre[i];
        t[i] = s + tau[i];
    }
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
    *tau_norm = norm3(tau); *omega_norm = theta;
    return true;
}

}  // namespace cf
