// surf_boot_dev.h -- the per-frame depth filter and the frame-1 bootstrap of a map (part of surfel.hip's translation unit).
// Stage: depth_bilateral_metric.frag, vertex_feedback.* and Model::initialise -- per frame or per model, no batch form -- with their launchers
// (the compaction between feedback and init is surf_scan_dev.h's).
#pragma once
#include "surf_batch_dev.h"

namespace cf {

// ================================================================================ bilateral ====
// depth_bilateral_metric.frag:30-75
__global__ void __launch_bounds__(kB) bilateral_kernel(const float* __restrict__ depth, int cols, int rows, float maxD,
                                                       float* __restrict__ out)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= cols * rows) return;
    const int y = i / cols, x = i - y * cols;
    const float value = depth[i];
    if (value > maxD || value < 0.3f) { out[i] = 0; return; }
    // The kernel is VALU-bound (169 taps x exp per pixel), so the 13x13 window is fully unrolled: the spatial term
    // ((float)x-(float)cx)^2 + ((float)y-(float)cy)^2 is an exact small integer, hence space2 * 0.024691358f folds to
    // a per-tap constant with the same value the shader computes at run time.  Taps outside the image are skipped
    // (the shader's loop bounds), in the same row-major order.
    float sum1 = 0, sum2 = 0;
#pragma unroll
    for (int dy = -6; dy <= 6; ++dy) {
        const int cy = y + dy;
        if (cy < 0 || cy >= rows) continue;
        const float* __restrict__ rowp = depth + cy * cols + x;
#pragma unroll
        for (int dx = -6; dx <= 6; ++dx) {
            const int cx = x + dx;
            if (cx < 0 || cx >= cols) continue;
            const float tmp = rowp[dx];
            const float space2 = (float)(dx * dx + dy * dy);
            const float color2 = (value - tmp) * (value - tmp);
            const float weight = det_expf(-(space2 * 0.024691358f + color2 * 555.556f));
            sum1 += tmp * weight;
            sum2 += weight;
        }
    }
    out[i] = sum1 / sum2;
}

// ============================================================================ frame-1 bootstrap ====
// vertex_feedback.vert:40-68 (+ .geom): thread per pixel (row-major for coalescing); the record and
// its flag are stored at the COLUMN-major rank i*rows+j, the order the reference draws the points in.
__global__ void __launch_bounds__(kB) feedback_kernel(const uchar4* __restrict__ rgba, const float* __restrict__ depth, int cols, int rows,
                                                      float cx, float cy, float inv_fx, float inv_fy, const float* __restrict__ tcx,
                                                      const float* __restrict__ tcy, int time, float maxDepth,
                                                      float4* __restrict__ rec /* [N*3] by rank */, unsigned* __restrict__ flags)
{
    const int q = blockIdx.x * kB + threadIdx.x;
    if (q >= cols * rows) return;
    const int j = q / cols, i = q - j * cols;
    const int rank = i * rows + j;
    const float x = tcx[i] * (float)cols, y = tcy[j] * (float)rows;
    const f3 p = get_vertex(depth, cols, rows, i, j, x, y, cx, cy, inv_fx, inv_fy);
    if (p.z <= 0 || p.z > maxDepth) { flags[rank] = 0; return; }
    const f3 n = get_normal_central(p, depth, cols, rows, i, j, x, y, cx, cy, inv_fx, inv_fy);
    const uchar4 c = rgba[q];
    flags[rank] = 1;
    rec[rank * 3 + 0] = make_float4(p.x, p.y, p.z, confidence(x, y, cx, cy, 1.0f));
    rec[rank * 3 + 1] = make_float4(encode_color((float)c.x / 255.0f, (float)c.y / 255.0f, (float)c.z / 255.0f), 0.f, (float)c.z / 255.0f, (float)time);
    rec[rank * 3 + 2] = make_float4(n.x, n.y, n.z, get_radius(p.z, n.z, inv_fx, inv_fy));
}


// Model::initialise (Model.cpp:227-272) + init_unstable.vert: attr 0/1 raw, attr 2 filtered, same index
__global__ void __launch_bounds__(kB) init_kernel(const float4* __restrict__ raw, const float4* __restrict__ filt,
                                                  const unsigned* __restrict__ raw_count, float4* __restrict__ out)
{
    const unsigned k = blockIdx.x * kB + threadIdx.x;
    if (k >= *raw_count) return;
    const float4 c = raw[k * 3 + 1];
    out[k * 3] = raw[k * 3];
    out[k * 3 + 1] = make_float4(c.x, 0.f, 1.f, c.w);
    out[k * 3 + 2] = filt[k * 3 + 2];
}

void launch_bilateral(hipStream_t s, const float* depth, int cols, int rows, float maxD, float* out)
{
    bilateral_kernel<<<gridFor((long long)cols * rows), kB, 0, s>>>(depth, cols, rows, maxD, out);
}
void launch_feedback(hipStream_t s, const uint8_t* rgba, const float* depth, int cols, int rows, cf_cam cam, float inv_fx, float inv_fy,
                     const float* tcx, const float* tcy, int time, float maxDepth, float* rec, unsigned* flags)
{
    feedback_kernel<<<gridFor((long long)cols * rows), kB, 0, s>>>(reinterpret_cast<const uchar4*>(rgba), depth, cols, rows, cam.cx, cam.cy, inv_fx,
                                                                   inv_fy, tcx, tcy, time, maxDepth, reinterpret_cast<float4*>(rec), flags);
}
void launch_init(hipStream_t s, const float* raw, const float* filt, const unsigned* raw_count, long long max_n, float* out)
{
    init_kernel<<<gridFor(max_n), kB, 0, s>>>(reinterpret_cast<const float4*>(raw), reinterpret_cast<const float4*>(filt), raw_count,
                                              reinterpret_cast<float4*>(out));
}

}  // namespace cf
