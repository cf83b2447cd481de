// seg_slic_dev.h -- SLIC superpixels and the per-superpixel sums (part of segment.hip's translation unit).
// Stage: what turns full-resolution images into values per superpixel and back -- gSLICr's assignment / update passes
// (Slic::processFrame), the exact Q32 sums of Slic::downsample* with the labels at the resample coordinates, and Slic::upsample.
#pragma once
#include "cf_surfel_device.h"
#include "cf_segment.h"

namespace cf {

constexpr int kSpix = 16;
constexpr int kAccTile = 16;  // models per pass of the accumulation kernel (their pointers travel in the kernel arguments up to this many)

// ---------------------------------------------------------------------------------- SLIC ----
__global__ void slic_init_kernel(const uchar4* __restrict__ rgba, int cols, int gx, int K, float* __restrict__ centres)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int cx = k % gx, cy = k / gx;
    const int px = cx * kSpix + kSpix / 2, py = cy * kSpix + kSpix / 2;
    const uchar4 p = rgba[py * cols + px];
    float* c = centres + k * 5;
    c[0] = (float)px; c[1] = (float)py; c[2] = (float)p.x; c[3] = (float)p.y; c[4] = (float)p.z;
}

// one 16x16 workgroup per grid cell
__global__ void __launch_bounds__(256) slic_assign_kernel(const uchar4* __restrict__ rgba, int cols, int rows, int gx, int gy,
                                                          const float* __restrict__ centres, int* __restrict__ labels,
                                                          unsigned long long* __restrict__ sums /* [K][6] */)
{
    __shared__ float s_c[9][5];
    __shared__ int s_lab[9];
    __shared__ unsigned s_acc[9][6];
    const int cx0 = blockIdx.x, cy0 = blockIdx.y;
    const int t = threadIdx.x;
    if (t < 9) {
        const int dx = t % 3 - 1, dy = t / 3 - 1;
        const int cx = cx0 + dx, cy = cy0 + dy;
        const bool ok = !(cx < 0 || cy < 0 || cx >= gx || cy >= gy);
        s_lab[t] = ok ? cy * gx + cx : -1;
        for (int q = 0; q < 5; q++) s_c[t][q] = ok ? centres[(cy * gx + cx) * 5 + q] : 0.f;
    }
    if (t < 54) s_acc[t / 6][t % 6] = 0;
    __syncthreads();
    const int x = cx0 * kSpix + (t & 15), y = cy0 * kSpix + (t >> 4);
    const uchar4 p = rgba[y * cols + x];
    // gSLICr's normalisers (seg_engine_GPU constructor, RGB case) and coherence weight (Slic.cpp:37), as in oracle/orc_segment.c
    float max_color_dist = 5.0f / (1.7321f * 255), max_xy_dist = 1.0f / (1.4142f * kSpix);
    max_color_dist *= max_color_dist; max_xy_dist *= max_xy_dist;
    const float weight = 0.6f;
    float best = 999999.9999f; int bi = 4;
#pragma unroll
    for (int n = 0; n < 9; n++) {  // dy-major, dx-minor: same scan order as the oracle
        if (s_lab[n] < 0) continue;
        const float dr = (float)p.x - s_c[n][2], dg = (float)p.y - s_c[n][3], db = (float)p.z - s_c[n][4];
        const float ex = (float)x - s_c[n][0], ey = (float)y - s_c[n][1];
        const float dcolor = dr * dr + dg * dg + db * db, dxy = ex * ex + ey * ey;
        const float d = sqrtf(dcolor * max_color_dist + weight * dxy * max_xy_dist);  // compute_slic_distance
        if (d < best) { best = d; bi = n; }
    }
    labels[y * cols + x] = s_lab[bi];
    atomicAdd(&s_acc[bi][0], (unsigned)x); atomicAdd(&s_acc[bi][1], (unsigned)y); atomicAdd(&s_acc[bi][2], (unsigned)p.x);
    atomicAdd(&s_acc[bi][3], (unsigned)p.y); atomicAdd(&s_acc[bi][4], (unsigned)p.z); atomicAdd(&s_acc[bi][5], 1u);
    __syncthreads();
    if (t < 54) {
        const int n = t / 6, q = t % 6;
        if (s_lab[n] >= 0 && s_acc[n][q]) atomicAdd(&sums[(size_t)s_lab[n] * 6 + q], (unsigned long long)s_acc[n][q]);
    }
}

__global__ void slic_update_kernel(unsigned long long* __restrict__ sums, int K, float* __restrict__ centres)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    unsigned long long* s = sums + (size_t)k * 6;
    // finalize_reduction_result_shared: a cluster without pixels stays at its reset value (centre (0,0), colour 0)
    for (int q = 0; q < 5; q++) centres[k * 5 + q] = s[5] ? (float)(long long)s[q] / (float)(long long)s[5] : 0.f;
    for (int q = 0; q < 6; q++) s[q] = 0;
}

// -------------------------------------------------------------- per-superpixel sums ----
__device__ __forceinline__ long long q32(float v)
{
    if (!is_finite(v)) return 0;
    const float c = fminf(fmaxf(v, -1048576.0f), 1048576.0f);
    return __double2ll_rn((double)c * 4294967296.0);
}

// the pixel whose label stands in for an "empty" superpixel k (Slic.h:192-206; index / spixelY -- k / gy, not k / gx -- is the reference's)
__device__ __forceinline__ int resample_pixel(int k, int cols, int rows, int gx, int gy)
{
    int x = (int)((k % gx) * kSpix + kSpix * 0.5), y = (int)((k / gy) * kSpix + kSpix * 0.5);
    if (y >= rows) y = rows - 1;
    if (x >= cols) x = cols - 1;
    return y * cols + x;
}

// (kSegBatch / SegBatch: cf_segment.h)

struct AccArgs {
    const int* labels; const float* depth;
    const float* icp[kAccTile]; const float4* vconf[kAccTile];   // the first kAccTile models' images (kernel arguments: no pointer chasing)
    const float* const* icp_dev; const float4* const* vconf_dev;  // all n_models of them in device memory when there are more
    int n_models, cols, rows, gx, gy;
    int* resample;                   // nullable: [K] labels at the resample coordinates, written by the launch's extra grid row
    unsigned* spix_count;            // [K]
    unsigned* depth_count;           // [K]
    unsigned long long* depth_sum;   // [K]
    unsigned long long* icp_sum;     // [n][K]
    unsigned long long* conf_sum;    // [n][K]
};

// PARTS selects the sums of a launch.  Only the ICP error surfaces wait for the frame's tracking; the frame's own sums (pixel and depth
// counts, depth sums, resample labels) and the models' confidence sums read what exists at the start of the frame (the confidences are
// the PREVIOUS frame's prediction), so cf_seg_early takes kAccFrame | kAccConf beside the tracking launches and the launch behind the
// tracker is left with the slot search and one atomic per model.  kAccAll is the single launch of the plain chain; the three share one text.
constexpr int kAccFrame = 1, kAccConf = 2, kAccIcp = 4, kAccAll = 7;
template <int PARTS>
__global__ void __launch_bounds__(256) seg_accumulate_kernel(const SegBatch<AccArgs> B)
{
    constexpr bool kFrame = (PARTS & kAccFrame) != 0, kConf = (PARTS & kAccConf) != 0, kIcp = (PARTS & kAccIcp) != 0;
    const AccArgs& a = B.m[blockIdx.z];
    __shared__ int s_lab[9];
    __shared__ unsigned s_cnt[9], s_dcnt[9];
    __shared__ unsigned long long s_dsum[9];
    __shared__ unsigned long long s_icp[kAccTile][9], s_conf[kAccTile][9];
    const int cx0 = blockIdx.x, cy0 = blockIdx.y, t = threadIdx.x;
    if (cy0 == a.gy) {  // the extra grid row: labels at the "empty superpixel" resample coordinates (resample_pixel)
        const int k = cx0 * 256 + t;
        if (!kFrame || k >= a.gx * a.gy) return;   // (a launch without the frame's part has no such row)
        a.resample[k] = a.labels[resample_pixel(k, a.cols, a.rows, a.gx, a.gy)];
        return;
    }
    const int K = a.gx * a.gy;
    if (t < 9) {
        const int dx = t % 3 - 1, dy = t / 3 - 1, cx = cx0 + dx, cy = cy0 + dy;
        s_lab[t] = (cx < 0 || cy < 0 || cx >= a.gx || cy >= a.gy) ? -1 : cy * a.gx + cx;
        if (kFrame) { s_cnt[t] = 0; s_dcnt[t] = 0; s_dsum[t] = 0; }
    }
    for (int k = t; k < kAccTile * 9; k += 256) { if (kIcp) s_icp[k / 9][k % 9] = 0; if (kConf) s_conf[k / 9][k % 9] = 0; }
    __syncthreads();
    const int x = cx0 * kSpix + (t & 15), y = cy0 * kSpix + (t >> 4);
    const int q = y * a.cols + x;
    const int lab = a.labels[q];
    int slot = 4;
#pragma unroll
    for (int n = 0; n < 9; n++) if (s_lab[n] == lab) slot = n;
    if (kFrame) {
        atomicAdd(&s_cnt[slot], 1u);
        const float d = a.depth[q];
        if (d > 0.02f) { atomicAdd(&s_dcnt[slot], 1u); atomicAdd(&s_dsum[slot], (unsigned long long)q32(d)); }
    }
    // the models in tiles of kAccTile (one pass for up to 16 models: what a frame normally has)
    for (int m0 = 0; (kIcp || kConf) && m0 < a.n_models; m0 += kAccTile) {
        const int nm = min(kAccTile, a.n_models - m0);
        if (m0 > 0) {
            __syncthreads();
            for (int k = t; k < kAccTile * 9; k += 256) { if (kIcp) s_icp[k / 9][k % 9] = 0; if (kConf) s_conf[k / 9][k % 9] = 0; }
            __syncthreads();
        }
        for (int m = 0; m < nm; m++) {
            if (kIcp) {
                const float* icp = a.n_models <= kAccTile ? a.icp[m] : a.icp_dev[m0 + m];
                atomicAdd(&s_icp[m][slot], (unsigned long long)q32(icp[q]));
            }
            if (kConf) {
                const float4* vc = a.n_models <= kAccTile ? a.vconf[m] : a.vconf_dev[m0 + m];
                atomicAdd(&s_conf[m][slot], (unsigned long long)q32(vc[q].w));
            }
        }
        __syncthreads();
        if (t < 9 && s_lab[t] >= 0) {
            const int L = s_lab[t];
            for (int m = 0; m < nm; m++) {
                if (kIcp && s_icp[m][t]) atomicAdd(&a.icp_sum[(size_t)(m0 + m) * K + L], s_icp[m][t]);
                if (kConf && s_conf[m][t]) atomicAdd(&a.conf_sum[(size_t)(m0 + m) * K + L], s_conf[m][t]);
            }
        }
    }
    __syncthreads();
    if (kFrame && t < 9 && s_lab[t] >= 0) {
        const int L = s_lab[t];
        if (s_cnt[t]) atomicAdd(&a.spix_count[L], s_cnt[t]);
        if (s_dcnt[t]) { atomicAdd(&a.depth_count[L], s_dcnt[t]); atomicAdd(&a.depth_sum[L], s_dsum[t]); }
    }
}

// labels at the resample coordinates for grids the accumulation launch's extra row cannot cover (gy > 256)
__global__ void seg_resample_kernel(const int* __restrict__ labels, int cols, int rows, int gx, int gy, int* __restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= gx * gy) return;
    out[k] = labels[resample_pixel(k, cols, rows, gx, gy)];
}

struct UpsampleArgs { const int* labels; const unsigned char* low_map; unsigned char* full; };
__global__ void __launch_bounds__(256) seg_upsample_kernel(const SegBatch<UpsampleArgs> B, int N)
{
    const UpsampleArgs& a = B.m[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) a.full[i] = a.low_map[a.labels[i]];
}

}  // namespace cf
