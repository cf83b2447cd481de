// surf_splat_dev.h -- the splat prediction of a model, the fill-in of its holes and the fill ratio (part of surfel.hip's translation unit).
// Stage: splat.vert / combo_splat.frag (ModelProjection::combinedPredict; depth_splat.frag for synthesizeDepth) -- splat_raster_kernel
// (atomicMin) + splat_resolve_kernel<mode> --, fill_*.frag (Model::performFillIn) and CoFusion::requiresFillIn, with their launchers.
#pragma once
#include "surf_index_dev.h"

namespace cf {

// ============================================================================ splat prediction ====
// splat.vert:54-88 + combo_splat.frag:37-65
struct SplatSetup { f3 ph, n; float rad, pn; int x_lo, x_hi, y_lo, y_hi; };

__device__ __forceinline__ bool splat_setup(const float4 pc, const float4 ct, const float4 nr, const Mat4& t_inv, cf_cam cam, int cols,
                                            int rows, float maxDepth, float confThreshold, int time, int maxTime, int timeDelta,
                                            SplatSetup& s)
{
    s.ph = xform_point(t_inv, f3{pc.x, pc.y, pc.z});
    if (s.ph.z > maxDepth || s.ph.z < 0 || pc.w < confThreshold || (float)time - ct.w > (float)timeDelta || ct.w > (float)maxTime) return false;
    s.n = normalized(xform_dir(t_inv, f3{nr.x, nr.y, nr.z}));
    s.rad = nr.w;
    const f3 x1n = normalized(f3{s.n.y - s.n.z, -s.n.x, s.n.x});
    const f3 x1 = {x1n.x * s.rad * 1.41421356f, x1n.y * s.rad * 1.41421356f, x1n.z * s.rad * 1.41421356f};
    const f3 y1 = cross(s.n, x1);
    const f3 c[4] = {s.ph + x1, s.ph + y1, s.ph - y1, s.ph - x1};
    float px_[4], py_[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { px_[k] = ((cam.fx * c[k].x) / c[k].z) + cam.cx; py_[k] = ((cam.fy * c[k].y) / c[k].z) + cam.cy; }
    const float xmin = fminf(px_[0], fminf(px_[1], fminf(px_[2], px_[3]))), xmax = fmaxf(px_[0], fmaxf(px_[1], fmaxf(px_[2], px_[3])));
    const float ymin = fminf(py_[0], fminf(py_[1], fminf(py_[2], py_[3]))), ymax = fmaxf(py_[0], fmaxf(py_[1], fmaxf(py_[2], py_[3])));
    const float size = fmaxf(0.0f, fmaxf(fabsf(xmax - xmin), fabsf(ymax - ymin)));
    if (!(size > 0.0f) || !(size <= 4096.0f)) return false;
    const float u = ((cam.fx * s.ph.x) / s.ph.z) + cam.cx, v = ((cam.fy * s.ph.y) / s.ph.z) + cam.cy;
    if (!(u >= 0.0f && v >= 0.0f && u <= (float)cols && v <= (float)rows)) return false;  // points are clipped by their centre
    const float half = size * 0.5f;
    s.x_lo = max((int)ceilf(u - half - 0.5f), 0); s.x_hi = min((int)ceilf(u + half - 0.5f) - 1, cols - 1);
    s.y_lo = max((int)ceilf(v - half - 0.5f), 0); s.y_hi = min((int)ceilf(v + half - 0.5f) - 1, rows - 1);
    s.pn = dot(s.ph, s.n);
    return true;
}

// fragment: returns false when discarded; z = corrected depth
// `rays` holds normalized((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1) per pixel (splat_rays_kernel): the
// fragment shader's view ray depends only on the pixel, and its two divisions + normalisation (sqrt + 3 IEEE
// divisions) were half of the VALU work of every fragment.
__device__ __forceinline__ bool splat_fragment(const SplatSetup& s, const float4* __restrict__ rays, int cols, int px, int py, float maxDepth,
                                               float& z)
{
    const float4 lr = rays[py * cols + px];
    const f3 l = {lr.x, lr.y, lr.z};
    const float k = s.pn / dot(l, s.n);
    const f3 cp = {k * l.x, k * l.y, k * l.z};
    const f3 diff = cp - s.ph;
    if (!(dot(diff, diff) <= s.rad * s.rad)) return false;
    if (!(cp.z < maxDepth)) return false;
    z = cp.z;
    return true;
}

__global__ void __launch_bounds__(kB) splat_rays_kernel(cf_cam cam, int cols, int rows, float4* __restrict__ rays)
{
    const int q = blockIdx.x * kB + threadIdx.x;
    if (q >= cols * rows) return;
    const int py = q / cols, px = q - py * cols;
    const float fx_ = (float)px + 0.5f, fy_ = (float)py + 0.5f;
    const f3 l = normalized(f3{(fx_ - cam.cx) / cam.fx, (fy_ - cam.cy) / cam.fy, 1.0f});
    rays[q] = make_float4(l.x, l.y, l.z, 0.f);
}

struct SplatArgs {   // combinedPredict of one model (both kernels)
    const float4* surfels; const unsigned* count; Mat4 t_inv; float maxDepth, confThreshold; int time, maxTime, timeDelta;
    const float4* rays; unsigned long long* keys; uchar4* image; float4* vertexConf; float4* normalRad; unsigned short* time16;
    SplatFillArgs fill;   // (resolve only)
};

__global__ void __launch_bounds__(kB) splat_raster_kernel(const Batch<SplatArgs> B, const FrameGeom g)
{
    const VBlock vb = batch_decode(B.h);
    const SplatArgs& a = B.m[vb.model];
    const float4* __restrict__ surfels = a.surfels; const float4* __restrict__ rays = a.rays; unsigned long long* __restrict__ keys = a.keys;
    const int cols = g.cols, rows = g.rows;
    // four lanes per surfel: the fragments of a point sprite are independent (the z-test is an atomicMin), and a
    // lane walking a 5x5 footprint alone is a chain of 25 dependent ray loads; the set-up is recomputed per lane
    const unsigned gt = vb.bid * kB + threadIdx.x;
    const unsigned id = gt >> 2;
    const int sub = (int)(gt & 3u);
    if (id >= *a.count) return;
    SplatSetup s;
    if (!splat_setup(surfels[id * 3], surfels[id * 3 + 1], surfels[id * 3 + 2], a.t_inv, g.cam, cols, rows, a.maxDepth, a.confThreshold, a.time,
                     a.maxTime, a.timeDelta, s))
        return;
    const int w = s.x_hi - s.x_lo + 1, h = s.y_hi - s.y_lo + 1;
    if (w <= 0 || h <= 0) return;
    int fx = sub, fy = 0;
    while (fx >= w) { fx -= w; fy++; }
    while (fy < h) {
        const int px = s.x_lo + fx, py = s.y_lo + fy;
        float z;
        if (splat_fragment(s, rays, cols, px, py, a.maxDepth, z)) {
            // (Measured and dropped, late in round 6: `if (zk < keys[q])` in front of the atomic -- a key only ever decreases, so a fragment
            // that does not beat what the pixel holds now never will, and ~11 of a pixel's ~14 atomics would go: 48.4 against 35.0 us.  The
            // fire-and-forget atomics are not what the kernel waits for; a load in every fragment's chain is.)
            atomicMin(&keys[py * cols + px], zkey(z, id));
        }
        fx += 4;
        while (fx >= w) { fx -= w; fy++; }
    }
}

// ==================================================================================== fill-in ====
// fill_vertex.frag / fill_normal.frag / fill_rgb.frag on texel q = (x, y) of a prediction: v, n, e are its vertex, normal and colour
__device__ __forceinline__ void fill_in_px(float4 v, float4 n, uchar4 e, const float* __restrict__ depth, const uchar4* __restrict__ rgba, int cols,
                                           int rows, int x, int y, int q, float cx, float cy, float inv_fx, float inv_fy, int pass_geom, int pass_rgb,
                                           float4* __restrict__ ov, float4* __restrict__ on, uchar4* __restrict__ oi)
{
    const float z = depth[q];
    const f3 p = {((float)x - cx) * z * inv_fx, ((float)y - cy) * z * inv_fy, z};
    ov[q] = (v.z == 0 || pass_geom) ? make_float4(p.x, p.y, p.z, 1.f) : v;
    if (n.z == 0 || pass_geom) {
        const float zx = depth[y * cols + min(x + 1, cols - 1)], zy = depth[min(y + 1, rows - 1) * cols + x];
        const f3 vx = {((float)(x + 1) - cx) * zx * inv_fx, ((float)y - cy) * zx * inv_fy, zx};
        const f3 vy = {((float)x - cx) * zy * inv_fx, ((float)(y + 1) - cy) * zy * inv_fy, zy};
        const f3 nn = normalized(cross(vx - p, vy - p));
        on[q] = make_float4(nn.x, nn.y, nn.z, 1.f);
    } else
        on[q] = n;
    oi[q] = (((int)e.x + (int)e.y + (int)e.z) == 0 || pass_rgb) ? rgba[q] : e;
}
__global__ void __launch_bounds__(kB) fill_in_kernel(const float4* __restrict__ pv, const float4* __restrict__ pn, const uchar4* __restrict__ pimg,
                                                     const float* __restrict__ depth, const uchar4* __restrict__ rgba, int cols, int rows,
                                                     float cx, float cy, float inv_fx, float inv_fy, int pass_geom, int pass_rgb,
                                                     float4* __restrict__ ov, float4* __restrict__ on, uchar4* __restrict__ oi)
{
    const int q = blockIdx.x * kB + threadIdx.x;
    if (q >= cols * rows) return;
    const int y = q / cols, x = q - y * cols;
    fill_in_px(pv[q], pn[q], pimg[q], depth, rgba, cols, rows, x, y, q, cx, cy, inv_fx, inv_fy, pass_geom, pass_rgb, ov, on, oi);
}
// is coordinate p one of the dn sample positions nearest_texel((i + .5) / dn, size) of fill_ratio_kernel along an axis?  The positions
// are 20 texels or more apart and the i-th lies in [i size / dn, (i + 1) size / dn): only i = p dn / size and its neighbours can hit p.
__device__ __forceinline__ bool fill_ratio_sample(int p, int dn, int size)
{
    const int i0 = p * dn / size;
    bool hit = false;
    for (int i = max(i0 - 1, 0); i <= min(i0 + 1, dn - 1); i++) hit = hit || nearest_texel(((float)i + 0.5f) / (float)dn, size) == p;
    return hit;
}

// host twin of nearest_texel / of the sample positions: how many workgroups of kB consecutive texels hold at least one of them
int fill_ratio_sample_blocks(int cols, int rows)
{
    const int dw = cols / 20, dh = rows / 20;
    int blocks = 0, last = -1;
    for (int j = 0; j < dh; j++)
        for (int i = 0; i < dw; i++) {   // (row-major: the texel index only grows)
            const auto texel = [](float u, int size) { const int t = (int)floorf(u * (float)size); return t < 0 ? 0 : (t > size - 1 ? size - 1 : t); };
            const int b = (texel(((float)j + 0.5f) / (float)dh, rows) * cols + texel(((float)i + 0.5f) / (float)dw, cols)) / kB;
            if (b != last) { blocks++; last = b; }
        }
    return blocks;
}

// The resolve of the splat pass.  A model whose arguments carry SplatFillArgs also gets, from the same registers, its fill-in maps and
// the covered count of CoFusion::requiresFillIn (see SplatFillArgs): such a share runs without early exits, so that every thread of
// a workgroup meets the barriers of the count.
// kMode: kSplatFull is combinedPredict.  kSplatCount is the same into another target set (the INACTIVE prediction of local loop closure)
// and adds the number of covered texels (time > 0) to the word fill.out2 points at, which the host zeroed in front of the launch (integer
// adds: the same count in any order; like the fill share it relies on the kernel having NO early exit in front of its barrier: the
// threads past the last texel fall through to __syncthreads_count).  kSplatDepth is synthesizeDepth (splat.vert + depth_splat.frag: the vertex stage, the disc test and
// the depth range of the colour splat, one output): corrected_pos.z into the f32 plane `vertexConf` points at, 0 where nothing lands.
// (the modes themselves: cf_kernels.h, beside launch_combined_predict_batch)
template <int kMode>
__global__ void __launch_bounds__(kB) splat_resolve_kernel(const Batch<SplatArgs> B, const FrameGeom g)
{
    const VBlock vb = batch_decode(B.h);
    const SplatArgs& a = B.m[vb.model];
    const float4* __restrict__ surfels = a.surfels; const float4* __restrict__ rays = a.rays; unsigned long long* __restrict__ keys = a.keys;
    uchar4* __restrict__ image = a.image; float4* __restrict__ vertexConf = a.vertexConf; float4* __restrict__ normalRad = a.normalRad;
    unsigned short* __restrict__ time16 = a.time16;
    const int cols = g.cols, rows = g.rows;
    const cf_cam cam = g.cam;
    const int q = vb.bid * kB + threadIdx.x;
    const bool fill = a.fill.depth_filt != nullptr;   // (uniform)
    bool covered = false, sample = false, timed = false;
    if (q < cols * rows) {
        const int py = q / cols, px = q - py * cols;
        const unsigned long long k = keys[q];
        keys[q] = kEmptyKey;  // leave the z-buffer cleared for the next pass (no memset launch per projection)
        uchar4 img = make_uchar4(0, 0, 0, 0);
        float4 vc = make_float4(0, 0, 0, 0), nrad = make_float4(0, 0, 0, 0);
        unsigned short t16 = 0;
        if (k != kEmptyKey) {
            const unsigned id = (unsigned)k;
            const float4 pc = surfels[id * 3], ct = surfels[id * 3 + 1], nr = surfels[id * 3 + 2];
            SplatSetup s;
            splat_setup(pc, ct, nr, a.t_inv, cam, cols, rows, a.maxDepth, a.confThreshold, a.time, a.maxTime, a.timeDelta, s);
            float z;
            splat_fragment(s, rays, cols, px, py, a.maxDepth, z);
            const f3 col = decode_color(ct.x);
            img = make_uchar4((unsigned char)glsl_round(col.x * 255.0f), (unsigned char)glsl_round(col.y * 255.0f),
                              (unsigned char)glsl_round(col.z * 255.0f), 255);
            const float fx_ = (float)px + 0.5f, fy_ = (float)py + 0.5f;
            vc = make_float4((fx_ - cam.cx) * z * (1.f / cam.fx), (fy_ - cam.cy) * z * (1.f / cam.fy), z, pc.w);
            nrad = make_float4(s.n.x, s.n.y, s.n.z, s.rad);
            t16 = (unsigned short)(unsigned)ct.z;
        }
        if constexpr (kMode == kSplatDepth) {
            reinterpret_cast<float*>(vertexConf)[q] = vc.z;
        } else {
            image[q] = img; vertexConf[q] = vc; normalRad[q] = nrad; time16[q] = t16;
        }
        timed = t16 > 0;
        if (fill) {
            fill_in_px(vc, nrad, img, a.fill.depth_filt, reinterpret_cast<const uchar4*>(a.fill.rgba), cols, rows, px, py, q, cam.cx, cam.cy,
                       a.fill.inv_fx, a.fill.inv_fy, a.fill.pass_geom, a.fill.pass_rgb, reinterpret_cast<float4*>(a.fill.fill_vertex),
                       reinterpret_cast<float4*>(a.fill.fill_normal), reinterpret_cast<uchar4*>(a.fill.fill_image));
            const int dw = cols / 20, dh = rows / 20;
            sample = dw > 0 && dh > 0 && fill_ratio_sample(py, dh, rows) && fill_ratio_sample(px, dw, cols);
            covered = sample && img.x > 0 && img.y > 0 && img.z > 0;
        }
    }
    if constexpr (kMode == kSplatCount) {
        const int n_timed = __syncthreads_count(timed ? 1 : 0);
        if (threadIdx.x == 0 && n_timed > 0) atomicAdd(a.fill.out2, (unsigned)n_timed);
        return;
    }
    if (!fill) return;
    // Only the workgroups that hold a sample position take part (the host counted them: sample_blocks), each with ONE atomic that
    // carries its covered count in the high word and its ticket in the low one.  The adds to one address are totally ordered, so the
    // value the last one gets back already holds every other workgroup's count: no fence, no second read.  (A ticket drawn by every
    // workgroup of the share -- 1200 same-address atomics behind a fence each -- made this launch 70 us instead of 19.)
    const unsigned samples = (unsigned)((cols / 20) * (rows / 20));
    unsigned total = 0;
    if (a.fill.sample_blocks > 0) {
        const int n_covered = __syncthreads_count(covered ? 1 : 0);
        if (!__syncthreads_or(sample ? 1 : 0) || threadIdx.x != 0) return;
        const unsigned long long old = atomicAdd(a.fill.acc, ((unsigned long long)(unsigned)n_covered << 32) | 1ull);
        if ((unsigned)old != (unsigned)a.fill.sample_blocks - 1u) return;
        total = (unsigned)(old >> 32) + (unsigned)n_covered;
        __hip_atomic_store(a.fill.acc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // zero again for the next launch
    } else if (vb.bid != 0 || threadIdx.x != 0)
        return;   // (an image without sample positions: the first workgroup publishes (0, 0))
    a.fill.out2[0] = total; a.fill.out2[1] = samples;
    if (a.fill.out2_host) { a.fill.out2_host[0] = total; a.fill.out2_host[1] = samples; }
}

// CoFusion::requiresFillIn (CoFusion.cpp:547-565): one workgroup counts the 20x down-sampled image
__global__ void __launch_bounds__(1024) fill_ratio_kernel(const uchar4* __restrict__ pimg, int cols, int rows, unsigned* __restrict__ out2,
                                                          unsigned* __restrict__ out2_host)
{
    const int dw = cols / 20, dh = rows / 20;
    unsigned s = 0;
    for (int k = threadIdx.x; k < dw * dh; k += 1024) {
        const int j = k / dw, i = k - j * dw;
        const int sx = nearest_texel(((float)i + 0.5f) / (float)dw, cols), sy = nearest_texel(((float)j + 0.5f) / (float)dh, rows);
        const uchar4 p = pimg[sy * cols + sx];
        s += (p.x > 0 && p.y > 0 && p.z > 0) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor((int)s, o, 64);
    __shared__ unsigned w[16];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int k = 0; k < 16; k++) t += w[k];
        out2[0] = t; out2[1] = (unsigned)(dw * dh);
        if (out2_host) { out2_host[0] = t; out2_host[1] = (unsigned)(dw * dh); }
    }
}

void launch_combined_predict_batch(hipStream_t s, const SplatPassArgs* items, int n_items, cf_cam cam, int cols, int rows, int mode)
{
    const FrameGeom g{cam, cols, rows};
    for_each_batch<SplatArgs>(items, n_items,
        [](const SplatPassArgs& h, SplatArgs& a) {
            a = SplatArgs{reinterpret_cast<const float4*>(h.surfels), h.count, mat4_from(h.t_inv), h.maxDepth, h.confThreshold, h.time, h.maxTime,
                          h.timeDelta, reinterpret_cast<const float4*>(h.rays), h.keys, reinterpret_cast<uchar4*>(h.image),
                          reinterpret_cast<float4*>(h.vertexConf), reinterpret_cast<float4*>(h.normalRad), h.time16, h.fill};
            return gridFor(4ll * h.count_bound);
        },
        [&](Batch<SplatArgs>& B, int* blocks, int nb, const SplatPassArgs*) {
            if (const int grid = batch_layout(B, blocks, nb)) splat_raster_kernel<<<grid, kB, 0, s>>>(B, g);
            for (int k = 0; k < nb; k++) blocks[k] = gridFor((long long)cols * rows);
            const int grid = batch_layout(B, blocks, nb);   // (always: the resolve also clears the keys)
            if (mode == kSplatCount) splat_resolve_kernel<kSplatCount><<<grid, kB, 0, s>>>(B, g);
            else if (mode == kSplatDepth) splat_resolve_kernel<kSplatDepth><<<grid, kB, 0, s>>>(B, g);
            else splat_resolve_kernel<kSplatFull><<<grid, kB, 0, s>>>(B, g);
        });
}
void launch_splat_rays(hipStream_t s, cf_cam cam, int cols, int rows, float* rays)
{
    splat_rays_kernel<<<gridFor((long long)cols * rows), kB, 0, s>>>(cam, cols, rows, reinterpret_cast<float4*>(rays));
}
void launch_fill_in(hipStream_t s, const float* pv, const float* pn, const uint8_t* pimg, const float* depth, const uint8_t* rgba, int cols,
                    int rows, cf_cam cam, float inv_fx, float inv_fy, int pass_geom, int pass_rgb, float* ov, float* on, uint8_t* oi)
{
    fill_in_kernel<<<gridFor((long long)cols * rows), kB, 0, s>>>(
        reinterpret_cast<const float4*>(pv), reinterpret_cast<const float4*>(pn), reinterpret_cast<const uchar4*>(pimg), depth,
        reinterpret_cast<const uchar4*>(rgba), cols, rows, cam.cx, cam.cy, inv_fx, inv_fy, pass_geom, pass_rgb, reinterpret_cast<float4*>(ov),
        reinterpret_cast<float4*>(on), reinterpret_cast<uchar4*>(oi));
}
void launch_fill_ratio(hipStream_t s, const uint8_t* pimg, int cols, int rows, unsigned* out2, unsigned* out2_host)
{
    fill_ratio_kernel<<<1, 1024, 0, s>>>(reinterpret_cast<const uchar4*>(pimg), cols, rows, out2, out2_host);
}

}  // namespace cf
