// mesh.hip -- mesh export: a triangle mesh of one surfel map, extracted on the device (include/cofusion_hip.h).
//
// Two stages, both stated in numpy by tests/mesh_ref.py in this file's operation order (f32, no contraction: -ffp-contract=off):
//   (a) mesh_accumulate_kernel   one wave per surfel, its lanes over the samples of the surfel's clipped box; every (surfel, sample)
//                                pair inside the support adds a quantised weight wq and wq * {dq, r, g, b} to five planes of 64-bit
//                                integers with atomics.  Integer sums commute: the grid does not depend on launch shape or arrival.
//       mesh_field_kernel        the planes -> distance (f32), validity, mean colour per sample
//   (b) mesh_classify_kernel     one thread per cell: triangles of its six tetrahedra counted, used edges marked with plain stores of 1
//       mesh_vcount_kernel       used edges per sample
//       scan_tile_kernel / scan_sums_kernel   exclusive scans of the two counts (tiles of 1024, then the tile sums by one workgroup
//                                with a 64-bit carry: any number of tiles)
//       mesh_vertex_kernel       one thread per sample: its vertices in (sample, kind) order
//       mesh_triangle_kernel     one thread per cell: its triangles in (cell, tetrahedron, triangle) order, and per vertex the lowest
//                                triangle that uses it (integer atomicMin)
//       mesh_face_normal_kernel  vertices whose gradient needs an invalid neighbour take the face normal of that triangle
// Sign: stored normals point away from the camera that saw the surfel (cf_surfel_device.h: get_normal_central), so n_out = -n and
// d = n_out . (c - p) is positive on the observed side: positive = outside.
#include <math.h>
#include <string.h>

#include <string>

#include "cf_device.h"
#include "cf_host.h"
#include "cf_mesh.h"

namespace cf {
namespace mesh {

constexpr int kB = 256;
constexpr int kTile = 1024;            // scan tile: kB threads x 4 items
constexpr int kAccBlocks = 16384;      // workgroups of the accumulation at most (its waves stride over the surfels)

__constant__ unsigned char kTet[6][4] = CF_MESH_TET_CORNERS;
__constant__ unsigned char kTetNeg[6] = CF_MESH_TET_NEGATIVE;
__constant__ unsigned char kEnds[6][2] = CF_MESH_EDGE_ENDS;
__constant__ unsigned char kCases[16][7] = CF_MESH_CASES;

struct GridDev {
    float ox, oy, oz, voxel;
    int nx, ny, nz;
    size_t n;
};

__device__ __forceinline__ size_t code_offset(const GridDev& g, int code)
{
    return (size_t)(code & 1) + (size_t)g.nx * ((size_t)(code >> 1 & 1) + (size_t)g.ny * (size_t)(code >> 2 & 1));
}

// ---- the default grid's bounds: min / max of order-preserving keys, exact sum of quantised radii ----
struct Bounds { unsigned lo[3], hi[3]; unsigned pad[2]; unsigned long long rsum, count; };

__global__ void __launch_bounds__(kB) mesh_bounds_kernel(const float4* __restrict__ surfels, unsigned count, float thresh, Bounds* out)
{
    const unsigned i = blockIdx.x * kB + threadIdx.x;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    unsigned long long rs = 0, c = 0;
    if (i < count) {
        const float4 pc = surfels[(size_t)i * 3];
        if (pc.w > thresh) {
            const float rad = surfels[(size_t)i * 3 + 2].w;
            lo[0] = hi[0] = fkey(pc.x); lo[1] = hi[1] = fkey(pc.y); lo[2] = hi[2] = fkey(pc.z);
            rs = (unsigned long long)(long long)rintf(fminf(fmaxf(rad, 0.0f), kRadiusLimit) * kRScale);
            c = 1;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], m, 64));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], m, 64));
        }
        rs += shfl_xor_u64(rs, m);
        c += shfl_xor_u64(c, m);
    }
    if ((threadIdx.x & 63) == 0 && c) {
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(&out->lo[a], lo[a]); atomicMax(&out->hi[a], hi[a]); }
        atomicAdd(&out->rsum, rs);
        atomicAdd(&out->count, c);
    }
}

// ---- stage (a) ----
struct AccParams { float thresh, tau, support_lo, support_hi, conf_cap; };

__device__ __forceinline__ void axis_range(float p, float reach, float o, float voxel, int n, int& lo, int& hi)
{
    const float fl = fminf(fmaxf(floorf(((p - reach) - o) / voxel), -1.0f), (float)n);
    const float fh = fminf(fmaxf(ceilf(((p + reach) - o) / voxel), -1.0f), (float)n);
    lo = max((int)fl, 0);
    hi = min((int)fh, n - 1);
}

__global__ void __launch_bounds__(kB) mesh_accumulate_kernel(const float4* __restrict__ surfels, unsigned count, const GridDev g, const AccParams q,
                                                             unsigned long long* __restrict__ acc)
{
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * (kB / 64);
    for (unsigned i = blockIdx.x * (kB / 64) + (threadIdx.x >> 6); i < count; i += waves) {
        const float4 pc = surfels[(size_t)i * 3];
        if (!(pc.w > q.thresh)) continue;
        const float4 ct = surfels[(size_t)i * 3 + 1], nr = surfels[(size_t)i * 3 + 2];
        const float rho = fminf(fmaxf(nr.w, q.support_lo), q.support_hi);
        const float rho2 = rho * rho;
        const float reach = q.tau + rho;
        int x0, x1, y0, y1, z0, z1;
        axis_range(pc.x, reach, g.ox, g.voxel, g.nx, x0, x1);
        axis_range(pc.y, reach, g.oy, g.voxel, g.ny, y0, y1);
        axis_range(pc.z, reach, g.oz, g.voxel, g.nz, z0, z1);
        if (x0 > x1 || y0 > y1 || z0 > z1) continue;
        const float nx_ = -nr.x, ny_ = -nr.y, nz_ = -nr.z;
        const float cw = fminf(pc.w, q.conf_cap);
        const int c24 = (int)fminf(fmaxf(ct.x, 0.0f), 16777215.0f);
        const unsigned long long cr = (unsigned)(c24 >> 16 & 255), cg = (unsigned)(c24 >> 8 & 255), cb = (unsigned)(c24 & 255);
        const unsigned bw = (unsigned)(x1 - x0 + 1), bh = (unsigned)(y1 - y0 + 1);
        const size_t cells = (size_t)bw * bh * (size_t)(z1 - z0 + 1);
        for (size_t t = lane; t < cells; t += 64) {
            const unsigned fx = (unsigned)(t % bw);
            const size_t r = t / bw;
            const int ix = x0 + (int)fx, iy = y0 + (int)(r % bh), iz = z0 + (int)(r / bh);
            const float ex = (g.ox + (float)ix * g.voxel) - pc.x, ey = (g.oy + (float)iy * g.voxel) - pc.y, ez = (g.oz + (float)iz * g.voxel) - pc.z;
            const float d = (nx_ * ex + ny_ * ey) + nz_ * ez;
            const float t2 = fmaxf(((ex * ex + ey * ey) + ez * ez) - d * d, 0.0f);
            if (!(fabsf(d) <= q.tau && t2 <= rho2)) continue;
            const float w = fmaxf(cw * (1.0f - t2 / rho2), 0.0f);
            const long long wq = (long long)rintf(w * kWScale);
            if (wq == 0) continue;
            const long long dq = (long long)rintf((d / q.tau) * kDScale);
            const size_t lin = ((size_t)iz * g.ny + iy) * g.nx + ix;   // (clipped indices: inside the grid)
            atomicAdd(&acc[lin], (unsigned long long)(wq * dq));
            atomicAdd(&acc[g.n + lin], (unsigned long long)wq);
            atomicAdd(&acc[2 * g.n + lin], (unsigned long long)wq * cr);
            atomicAdd(&acc[3 * g.n + lin], (unsigned long long)wq * cg);
            atomicAdd(&acc[4 * g.n + lin], (unsigned long long)wq * cb);
        }
    }
}

__global__ void __launch_bounds__(kB) mesh_field_kernel(const unsigned long long* __restrict__ acc, size_t n, unsigned long long w_min, float* __restrict__ sdf,
                                                        uint8_t* __restrict__ valid, float* __restrict__ rgb)
{
    const size_t i = (size_t)blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const unsigned long long sw = acc[n + i];
    const bool ok = sw >= w_min;
    const double den = ok ? (double)sw : 1.0;
    valid[i] = ok ? 1 : 0;
    sdf[i] = ok ? (float)((double)(long long)acc[i] / den) : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) rgb[i * 3 + k] = ok ? (float)((double)acc[(2 + k) * n + i] / den) : 0.0f;
}

// ---- stage (b) ----
// the cell whose lowest corner is sample idx: emits only when it is a cell (not on an upper face) and all corners are valid
__device__ __forceinline__ bool cell_inside_bits(const GridDev& g, size_t idx, const float* __restrict__ sdf, const uint8_t* __restrict__ valid, unsigned& bits)
{
    const int x = (int)(idx % g.nx), y = (int)(idx / g.nx % g.ny), z = (int)(idx / ((size_t)g.nx * g.ny));
    if (x >= g.nx - 1 || y >= g.ny - 1 || z >= g.nz - 1) return false;
    bits = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t j = idx + code_offset(g, c);
        if (!valid[j]) return false;
        bits |= (sdf[j] < 0.0f ? 1u : 0u) << c;
    }
    return true;
}

__device__ __forceinline__ unsigned tet_mask(unsigned bits, int t)
{
    return (bits >> kTet[t][0] & 1u) | (bits >> kTet[t][1] & 1u) << 1 | (bits >> kTet[t][2] & 1u) << 2 | (bits >> kTet[t][3] & 1u) << 3;
}

// triangle j of tetrahedron t in case m: its three (owner offset code, kind) pairs in output order
__device__ __forceinline__ void tet_triangle(int t, unsigned m, int j, int (&owner)[3], int (&kind)[3])
{
    int e[3] = {kCases[m][1 + 3 * j], kCases[m][2 + 3 * j], kCases[m][3 + 3 * j]};
    if (kTetNeg[t]) { const int s = e[1]; e[1] = e[2]; e[2] = s; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int ci = kTet[t][kEnds[e[k]][0]], cj = kTet[t][kEnds[e[k]][1]];
        owner[k] = ci; kind[k] = (ci ^ cj) - 1;
    }
}

__global__ void __launch_bounds__(kB) mesh_classify_kernel(const GridDev g, const float* __restrict__ sdf, const uint8_t* __restrict__ valid,
                                                           uint8_t* __restrict__ eflags, unsigned* __restrict__ tcnt)
{
    const size_t idx = (size_t)blockIdx.x * kB + threadIdx.x;
    if (idx >= g.n) return;
    unsigned bits, ntri = 0;
    if (cell_inside_bits(g, idx, sdf, valid, bits) && bits != 0 && bits != 255u) {
        for (int t = 0; t < 6; t++) {
            const unsigned m = tet_mask(bits, t);
            const int nt = kCases[m][0];
            for (int j = 0; j < nt; j++) {
                int owner[3], kind[3];
                tet_triangle(t, m, j, owner, kind);
#pragma unroll
                for (int k = 0; k < 3; k++) eflags[(idx + code_offset(g, owner[k])) * kKinds + kind[k]] = 1;   // (idempotent: every writer stores 1)
            }
            ntri += nt;
        }
    }
    tcnt[idx] = ntri;
}

__global__ void __launch_bounds__(kB) mesh_vcount_kernel(const uint8_t* __restrict__ eflags, size_t n, unsigned* __restrict__ vcnt)
{
    const size_t idx = (size_t)blockIdx.x * kB + threadIdx.x;
    if (idx >= n) return;
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < kKinds; k++) c += eflags[idx * kKinds + k];
    vcnt[idx] = c;
}

// in place: cnt[i] becomes the exclusive sum inside its tile of kTile; the tile's total goes to tile_sums
__global__ void __launch_bounds__(kB) scan_tile_kernel(unsigned* __restrict__ cnt, size_t n, unsigned* __restrict__ tile_sums)
{
    __shared__ unsigned s[kB];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kTile + (size_t)tid * 4;
    unsigned v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = base + k < n ? cnt[base + k] : 0u; sum += v[k]; }
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kB; off <<= 1) {
        const unsigned t = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    unsigned run = s[tid] - sum;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) cnt[base + k] = run;
        run += v[k];
    }
    if (tid == kB - 1) tile_sums[blockIdx.x] = s[kB - 1];
}

// one workgroup: tile_sums becomes its exclusive scan (low 32 bits; the caller checks the 64-bit total before it uses them)
__global__ void __launch_bounds__(kB) scan_sums_kernel(unsigned* __restrict__ tile_sums, unsigned ntiles, unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long s[kB];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (unsigned base = 0; base < ntiles; base += kB) {
        const unsigned long long v = base + tid < ntiles ? tile_sums[base + tid] : 0ull;
        s[tid] = v;
        __syncthreads();
        for (int off = 1; off < kB; off <<= 1) {
            const unsigned long long t = tid >= off ? s[tid - off] : 0ull;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        if (base + tid < ntiles) tile_sums[base + tid] = (unsigned)(s[tid] - v + carry);
        __syncthreads();
        if (tid == 0) carry += s[kB - 1];
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

__device__ __forceinline__ bool sample_gradient(const GridDev& g, size_t idx, const float* __restrict__ sdf, const uint8_t* __restrict__ valid, f3& out)
{
    const int x = (int)(idx % g.nx), y = (int)(idx / g.nx % g.ny), z = (int)(idx / ((size_t)g.nx * g.ny));
    if (x <= 0 || x >= g.nx - 1 || y <= 0 || y >= g.ny - 1 || z <= 0 || z >= g.nz - 1) return false;
    const size_t sx = 1, sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
    if (!(valid[idx + sx] && valid[idx - sx] && valid[idx + sy] && valid[idx - sy] && valid[idx + sz] && valid[idx - sz])) return false;
    out = f3{sdf[idx + sx] - sdf[idx - sx], sdf[idx + sy] - sdf[idx - sy], sdf[idx + sz] - sdf[idx - sz]};
    return true;
}

// v * (1 / sqrt(|v|^2)); false when |v|^2 is zero or not finite
__device__ __forceinline__ bool unit(f3 v, f3& out)
{
    const float l2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
    if (!(l2 > 0.0f) || !is_finite(l2)) return false;
    const float rn = 1.0f / sqrtf(l2);
    out = f3{v.x * rn, v.y * rn, v.z * rn};
    return true;
}

__device__ __forceinline__ unsigned char colour_u8(float c) { return (unsigned char)rintf(fminf(fmaxf(c, 0.0f), 255.0f)); }

__global__ void __launch_bounds__(kB) mesh_vertex_kernel(const GridDev g, const float* __restrict__ sdf, const uint8_t* __restrict__ valid, const float* __restrict__ rgb,
                                                         const uint8_t* __restrict__ eflags, const unsigned* __restrict__ vcnt, const unsigned* __restrict__ vtile,
                                                         unsigned n_vertices, cf_mesh_vertex* __restrict__ verts, uint8_t* __restrict__ need_face)
{
    const size_t idx = (size_t)blockIdx.x * kB + threadIdx.x;
    if (idx >= g.n) return;
    unsigned v = vcnt[idx] + vtile[idx / kTile];
    const int ax = (int)(idx % g.nx), ay = (int)(idx / g.nx % g.ny), az = (int)(idx / ((size_t)g.nx * g.ny));
    f3 ga{0.f, 0.f, 0.f};
    bool ga_known = false, ga_ok = false;
    for (int k = 0; k < kKinds; k++) {
        if (!eflags[idx * kKinds + k]) continue;
        if (v >= n_vertices) return;   // (cannot happen with the counts of these flags; never write past the arrays)
        const int code = k + 1, dx = code & 1, dy = code >> 1 & 1, dz = code >> 2 & 1;
        const size_t b = idx + code_offset(g, code);   // (in the grid: the edge was marked by a cell that owns both ends)
        const float sa = sdf[idx], sb = sdf[b];
        const float tt = sa / (sa - sb);
        const float Ax = g.ox + (float)ax * g.voxel, Ay = g.oy + (float)ay * g.voxel, Az = g.oz + (float)az * g.voxel;
        const float Bx = g.ox + (float)(ax + dx) * g.voxel, By = g.oy + (float)(ay + dy) * g.voxel, Bz = g.oz + (float)(az + dz) * g.voxel;
        cf_mesh_vertex o;
        o.x = Ax + (Bx - Ax) * tt; o.y = Ay + (By - Ay) * tt; o.z = Az + (Bz - Az) * tt;
        const float* ca = rgb + idx * 3; const float* cb = rgb + b * 3;
        o.r = colour_u8(ca[0] + (cb[0] - ca[0]) * tt);
        o.g = colour_u8(ca[1] + (cb[1] - ca[1]) * tt);
        o.b = colour_u8(ca[2] + (cb[2] - ca[2]) * tt);
        o.a = 255;
        if (!ga_known) { ga_ok = sample_gradient(g, idx, sdf, valid, ga); ga_known = true; }
        f3 gb, n{0.f, 0.f, 0.f};
        bool ok = ga_ok && sample_gradient(g, b, sdf, valid, gb);
        if (ok) ok = unit(f3{ga.x + (gb.x - ga.x) * tt, ga.y + (gb.y - ga.y) * tt, ga.z + (gb.z - ga.z) * tt}, n);
        o.nx = n.x; o.ny = n.y; o.nz = n.z;
        verts[v] = o;
        need_face[v] = ok ? 0 : 1;
        v++;
    }
}

__device__ __forceinline__ unsigned vertex_index(const GridDev& g, size_t owner, int kind, const uint8_t* __restrict__ eflags, const unsigned* __restrict__ vcnt,
                                                 const unsigned* __restrict__ vtile)
{
    unsigned v = vcnt[owner] + vtile[owner / kTile];
    for (int k = 0; k < kind; k++) v += eflags[owner * kKinds + k];
    return v;
}

__global__ void __launch_bounds__(kB) mesh_triangle_kernel(const GridDev g, const float* __restrict__ sdf, const uint8_t* __restrict__ valid,
                                                           const uint8_t* __restrict__ eflags, const unsigned* __restrict__ vcnt, const unsigned* __restrict__ vtile,
                                                           const unsigned* __restrict__ tcnt, const unsigned* __restrict__ ttile, unsigned n_vertices,
                                                           unsigned n_triangles, uint32_t* __restrict__ tris, unsigned* __restrict__ first_tri)
{
    const size_t idx = (size_t)blockIdx.x * kB + threadIdx.x;
    if (idx >= g.n) return;
    unsigned bits;
    if (!cell_inside_bits(g, idx, sdf, valid, bits) || bits == 0 || bits == 255u) return;
    unsigned ti = tcnt[idx] + ttile[idx / kTile];
    for (int t = 0; t < 6; t++) {
        const unsigned m = tet_mask(bits, t);
        const int nt = kCases[m][0];
        for (int j = 0; j < nt; j++) {
            int owner[3], kind[3];
            tet_triangle(t, m, j, owner, kind);
            if (ti >= n_triangles) return;   // (cannot happen with the counts of this field; never write past the arrays)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const unsigned v = vertex_index(g, idx + code_offset(g, owner[k]), kind[k], eflags, vcnt, vtile);
                tris[(size_t)ti * 3 + k] = v;
                if (v < n_vertices) atomicMin(&first_tri[v], ti);
            }
            ti++;
        }
    }
}

__global__ void __launch_bounds__(kB) mesh_face_normal_kernel(cf_mesh_vertex* __restrict__ verts, unsigned n_vertices, const uint32_t* __restrict__ tris,
                                                              unsigned n_triangles, const unsigned* __restrict__ first_tri, const uint8_t* __restrict__ need_face)
{
    const unsigned v = blockIdx.x * kB + threadIdx.x;
    if (v >= n_vertices || !need_face[v]) return;
    const unsigned t = first_tri[v];
    f3 n{0.f, 0.f, 0.f};
    if (t < n_triangles) {
        const unsigned i0 = tris[(size_t)t * 3], i1 = tris[(size_t)t * 3 + 1], i2 = tris[(size_t)t * 3 + 2];
        if (i0 < n_vertices && i1 < n_vertices && i2 < n_vertices) {
            const f3 p0{verts[i0].x, verts[i0].y, verts[i0].z}, p1{verts[i1].x, verts[i1].y, verts[i1].z}, p2{verts[i2].x, verts[i2].y, verts[i2].z};
            f3 u;
            if (unit(cross(p1 - p0, p2 - p0), u)) n = u;
        }
    }
    verts[v].nx = n.x; verts[v].ny = n.y; verts[v].nz = n.z;
}

}  // namespace mesh
}  // namespace cf

using namespace cf;
using namespace cf::mesh;

struct cf_mesher {
    cf_ctx* ctx = nullptr;
    uint64_t max_voxels = 0;
    unsigned long long* acc = nullptr;      // [kPlanes][n] of the current grid
    float* sdf = nullptr; uint8_t* valid = nullptr; float* rgb = nullptr;
    uint8_t* eflags = nullptr;              // [max_voxels][kKinds]
    unsigned *vcnt = nullptr, *tcnt = nullptr, *vtile = nullptr, *ttile = nullptr;
    unsigned long long* totals = nullptr;   // device [2]: vertices, triangles
    unsigned long long* h_totals = nullptr; // pinned [2]
    Bounds* bounds = nullptr; Bounds* h_bounds = nullptr;
    cf_mesh_grid grid{};                    // of the last accumulation / caller's field
    bool have_acc = false, have_mesh = false;
    cf_mesh_vertex* verts = nullptr; uint32_t* tris = nullptr; unsigned* first_tri = nullptr; uint8_t* need_face = nullptr;
    uint32_t n_vertices = 0, n_triangles = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // accumulate begin / end, extraction begin / end
    bool timed[2] = {false, false};
};

static int mesh_fail(cf_ctx* ctx, int code, const char* msg)
{
    ctx->set_error(std::string("cf_mesh: ") + msg);
    return code;
}

// samples of a grid, or -1 for a malformed one, or -2 for one over `limit`
static long long grid_samples(const cf_mesh_grid* g, uint64_t limit)
{
    if (g->nx < 0 || g->ny < 0 || g->nz < 0) return -1;
    if (g->nx == 0 || g->ny == 0 || g->nz == 0) return 0;
    if (!(g->voxel > 0.0f) || !(fabsf(g->voxel) < INFINITY)) return -1;
    const uint64_t xy = (uint64_t)g->nx * (uint64_t)g->ny;
    if (xy > limit || xy * (uint64_t)g->nz > limit) return -2;
    return (long long)(xy * (uint64_t)g->nz);
}

static GridDev grid_dev(const cf_mesh_grid& g, size_t n)
{
    return GridDev{g.origin[0], g.origin[1], g.origin[2], g.voxel, g.nx, g.ny, g.nz, n};
}

// the context's stream, ordered after every lane of the frame (as cf_render)
static int mesh_stream(cf_ctx* ctx, hipStream_t* out)
{
    const hipStream_t s = ctx->forked ? ctx->forked_from : ctx->stream;
    for (int lane = 0; lane < cf_ctx::kLanes; lane++)
        if (ctx->lanes_used & (1u << lane)) {
            HIPCHK(ctx, hipEventRecord(ctx->lane_done[lane], ctx->lanes[lane]));
            HIPCHK(ctx, hipStreamWaitEvent(s, ctx->lane_done[lane], 0));
        }
    *out = s;
    return CF_OK;
}

static void free_outputs(cf_mesher* m)
{
    void* ptrs[] = {m->verts, m->tris, m->first_tri, m->need_face};
    for (void* p : ptrs) (void)hipFree(p);
    m->verts = nullptr; m->tris = nullptr; m->first_tri = nullptr; m->need_face = nullptr;
    m->n_vertices = 0; m->n_triangles = 0; m->have_mesh = false;
}

static unsigned blocks_for(size_t n) { return (unsigned)((n + kB - 1) / kB); }

// stage (b) on m->sdf / valid / rgb of m->grid (n samples)
static int run_extract(cf_mesher* m, hipStream_t s, size_t n, uint32_t* n_vertices, uint32_t* n_triangles)
{
    cf_ctx* ctx = m->ctx;
    free_outputs(m);
    *n_vertices = 0; *n_triangles = 0;
    if (n == 0 || m->grid.nx < 2 || m->grid.ny < 2 || m->grid.nz < 2) { m->have_mesh = true; HIPCHK(ctx, hipEventRecord(m->ev[3], s)); m->timed[1] = true; return CF_OK; }
    const GridDev g = grid_dev(m->grid, n);
    const unsigned nb = blocks_for(n), ntiles = (unsigned)((n + kTile - 1) / kTile);
    HIPCHK(ctx, hipMemsetAsync(m->eflags, 0, n * kKinds, s));
    mesh_classify_kernel<<<nb, kB, 0, s>>>(g, m->sdf, m->valid, m->eflags, m->tcnt);
    mesh_vcount_kernel<<<nb, kB, 0, s>>>(m->eflags, n, m->vcnt);
    scan_tile_kernel<<<ntiles, kB, 0, s>>>(m->vcnt, n, m->vtile);
    scan_sums_kernel<<<1, kB, 0, s>>>(m->vtile, ntiles, m->totals);
    scan_tile_kernel<<<ntiles, kB, 0, s>>>(m->tcnt, n, m->ttile);
    scan_sums_kernel<<<1, kB, 0, s>>>(m->ttile, ntiles, m->totals + 1);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(m->h_totals, m->totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));   // the two counts
    const unsigned long long nv = m->h_totals[0], nt = m->h_totals[1];
    if (nv > 0xFFFFFFFFull || nt > 0xFFFFFFFFull) return mesh_fail(ctx, CF_ERANGE, "more than 2^32 - 1 vertices or triangles");
    if (nv && nt) {
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&m->verts), nv * sizeof(cf_mesh_vertex)));
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&m->tris), nt * 3 * sizeof(uint32_t)));
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&m->first_tri), nv * sizeof(unsigned)));
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&m->need_face), nv));
        HIPCHK(ctx, hipMemsetAsync(m->first_tri, 0xFF, nv * sizeof(unsigned), s));
        mesh_vertex_kernel<<<nb, kB, 0, s>>>(g, m->sdf, m->valid, m->rgb, m->eflags, m->vcnt, m->vtile, (unsigned)nv, m->verts, m->need_face);
        mesh_triangle_kernel<<<nb, kB, 0, s>>>(g, m->sdf, m->valid, m->eflags, m->vcnt, m->vtile, m->tcnt, m->ttile, (unsigned)nv, (unsigned)nt, m->tris,
                                               m->first_tri);
        mesh_face_normal_kernel<<<blocks_for(nv), kB, 0, s>>>(m->verts, (unsigned)nv, m->tris, (unsigned)nt, m->first_tri, m->need_face);
        LAUNCHCHK(ctx);
        m->n_vertices = (uint32_t)nv; m->n_triangles = (uint32_t)nt;
    }
    HIPCHK(ctx, hipEventRecord(m->ev[3], s));
    m->timed[1] = true;
    m->have_mesh = true;
    *n_vertices = m->n_vertices; *n_triangles = m->n_triangles;
    return CF_OK;
}

static float fkey_inv_host(unsigned k)
{
    const unsigned u = k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu);
    float f; memcpy(&f, &u, 4);
    return f;
}

extern "C" {

void cf_mesh_destroy(cf_mesher* m)
{
    if (!m) return;
    (void)hipStreamSynchronize(m->ctx->forked ? m->ctx->forked_from : m->ctx->stream);
    free_outputs(m);
    void* ptrs[] = {m->acc, m->sdf, m->valid, m->rgb, m->eflags, m->vcnt, m->tcnt, m->vtile, m->ttile, m->totals, m->bounds};
    for (void* p : ptrs) (void)hipFree(p);
    if (m->h_totals) (void)hipHostFree(m->h_totals);
    if (m->h_bounds) (void)hipHostFree(m->h_bounds);
    for (hipEvent_t e : m->ev) if (e) (void)hipEventDestroy(e);
    delete m;
}

int cf_mesh_create(cf_ctx* ctx, uint64_t max_voxels, cf_mesher** out)
{
    if (!ctx || !out || max_voxels < 1 || max_voxels > CF_MESH_MAX_VOXELS) return CF_EINVAL;
    *out = nullptr;
    cf_mesher* m = new cf_mesher();
    m->ctx = ctx; m->max_voxels = max_voxels;
    const size_t N = (size_t)max_voxels, tiles = (N + kTile - 1) / kTile;
    auto fail = [&](hipError_t e, const char* what) {
        ctx->set_error(std::string("cf_mesh_create: ") + what + ": " + hipGetErrorString(e));
        cf_mesh_destroy(m);
        return e == hipErrorOutOfMemory ? CF_ENOMEM : CF_EHIP;
    };
    hipError_t e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->acc), N * kPlanes * sizeof(unsigned long long)))) return fail(e, "accumulators");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->sdf), N * sizeof(float)))) return fail(e, "distances");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->valid), N))) return fail(e, "validity");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->rgb), N * 3 * sizeof(float)))) return fail(e, "colours");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->eflags), N * kKinds))) return fail(e, "edge flags");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->vcnt), N * sizeof(unsigned)))) return fail(e, "vertex counts");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->tcnt), N * sizeof(unsigned)))) return fail(e, "triangle counts");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->vtile), tiles * sizeof(unsigned)))) return fail(e, "vertex tiles");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->ttile), tiles * sizeof(unsigned)))) return fail(e, "triangle tiles");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->totals), 2 * sizeof(unsigned long long)))) return fail(e, "totals");
    if ((e = hipMalloc(reinterpret_cast<void**>(&m->bounds), sizeof(Bounds)))) return fail(e, "bounds");
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&m->h_totals), 2 * sizeof(unsigned long long), 0))) return fail(e, "pinned totals");
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&m->h_bounds), sizeof(Bounds), 0))) return fail(e, "pinned bounds");
    for (hipEvent_t& ev : m->ev)
        if ((e = hipEventCreate(&ev))) return fail(e, "event");
    *out = m;
    return CF_OK;
}

int cf_mesh_default_grid(cf_mesher* m, cf_model* model, float conf_threshold, float voxel, cf_mesh_grid* grid)
{
    if (!m || !model || !grid) return CF_EINVAL;
    cf_ctx* ctx = m->ctx;
    memset(grid, 0, sizeof(*grid));
    void* p = nullptr; uint64_t bytes = 0;
    if (int r = cf_model_buffer(model, 11, &p, &bytes)) return r;
    const unsigned count = (unsigned)(bytes / 48);
    if (!count) return CF_OK;
    hipStream_t s;
    if (int r = mesh_stream(ctx, &s)) return r;
    Bounds init{};
    for (int a = 0; a < 3; a++) { init.lo[a] = 0xffffffffu; init.hi[a] = 0u; }
    *m->h_bounds = init;
    HIPCHK(ctx, hipMemcpyAsync(m->bounds, m->h_bounds, sizeof(Bounds), hipMemcpyHostToDevice, s));
    mesh_bounds_kernel<<<blocks_for(count), kB, 0, s>>>(static_cast<const float4*>(p), count, conf_threshold, m->bounds);
    LAUNCHCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(m->h_bounds, m->bounds, sizeof(Bounds), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));   // the bounds
    const Bounds b = *m->h_bounds;
    if (!b.count) return CF_OK;
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = fkey_inv_host(b.lo[a]); hi[a] = fkey_inv_host(b.hi[a]); }
    if (!(voxel > 0.0f)) voxel = (float)((double)b.rsum / (double)b.count / 65536.0);
    if (!(voxel > 0.0f) || !(voxel < INFINITY)) return CF_OK;
    for (int step = 0; step < kGrowthSteps; step++) {
        const float tau = kDefaultTrunc * voxel;
        float o[3]; unsigned __int128 total = 1; int dims[3];
        for (int a = 0; a < 3; a++) {
            o[a] = lo[a] - tau;
            dims[a] = (int)fminf(ceilf(((hi[a] + tau) - o[a]) / voxel), 1073741824.0f) + 1;
            total *= (unsigned __int128)(unsigned)dims[a];
        }
        if (total <= (unsigned __int128)m->max_voxels) {
            for (int a = 0; a < 3; a++) grid->origin[a] = o[a];
            grid->voxel = voxel; grid->nx = dims[0]; grid->ny = dims[1]; grid->nz = dims[2];
            return CF_OK;
        }
        voxel = voxel * kVoxelGrowth;
    }
    return mesh_fail(ctx, CF_ERANGE, "no voxel size fits the map's box into max_voxels");
}

int cf_mesh_accumulate(cf_mesher* m, cf_model* model, const float* surfels_dev, uint32_t count, float conf_threshold, const cf_mesh_grid* grid,
                       const cf_mesh_params* params)
{
    if (!m || !grid) return CF_EINVAL;
    cf_ctx* ctx = m->ctx;
    m->have_acc = false;
    const long long n = grid_samples(grid, m->max_voxels);
    if (n == -1) return mesh_fail(ctx, CF_EINVAL, "malformed grid (negative size, or no positive finite voxel)");
    if (n == -2) return mesh_fail(ctx, CF_ERANGE, "the grid has more samples than the mesher's max_voxels");
    const cf_mesh_params q = params ? *params : cf_mesh_params{kDefaultTrunc, kDefaultSupport, kDefaultConfCap};
    if (!(q.trunc_voxels > 0.0f) || !(q.max_support_voxels > 0.0f) || !(q.conf_cap > 0.0f)) return mesh_fail(ctx, CF_EINVAL, "parameters must be positive");
    if (model) {
        void* p = nullptr; uint64_t bytes = 0;
        if (int r = cf_model_buffer(model, 11, &p, &bytes)) return r;
        surfels_dev = static_cast<const float*>(p); count = (uint32_t)(bytes / 48);
    } else if (count && !surfels_dev) return CF_EINVAL;
    hipStream_t s;
    if (int r = mesh_stream(ctx, &s)) return r;
    m->grid = *grid;
    HIPCHK(ctx, hipEventRecord(m->ev[0], s));
    if (n) HIPCHK(ctx, hipMemsetAsync(m->acc, 0, (size_t)n * kPlanes * sizeof(unsigned long long), s));
    if (n && count) {
        const AccParams a{conf_threshold, q.trunc_voxels * grid->voxel, 1.5f * grid->voxel, q.max_support_voxels * grid->voxel, q.conf_cap};
        const unsigned want = (count + (kB / 64) - 1) / (kB / 64);
        mesh_accumulate_kernel<<<want < (unsigned)kAccBlocks ? want : (unsigned)kAccBlocks, kB, 0, s>>>(reinterpret_cast<const float4*>(surfels_dev), count,
                                                                                                       grid_dev(*grid, (size_t)n), a, m->acc);
        LAUNCHCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(m->ev[1], s));
    m->timed[0] = true;
    m->have_acc = true;
    return CF_OK;
}

int cf_mesh_extract(cf_mesher* m, float w_min, uint32_t* n_vertices, uint32_t* n_triangles)
{
    if (!m || !n_vertices || !n_triangles) return CF_EINVAL;
    cf_ctx* ctx = m->ctx;
    if (!m->have_acc) return mesh_fail(ctx, CF_ESTATE, "cf_mesh_extract before cf_mesh_accumulate");
    hipStream_t s;
    if (int r = mesh_stream(ctx, &s)) return r;
    const size_t n = (size_t)grid_samples(&m->grid, m->max_voxels);
    double wq = rint((double)w_min * 4096.0);
    if (!(wq >= 1.0)) wq = 1.0;
    if (wq > 9.0e18) wq = 9.0e18;
    HIPCHK(ctx, hipEventRecord(m->ev[2], s));
    if (n) {
        mesh_field_kernel<<<blocks_for(n), kB, 0, s>>>(m->acc, n, (unsigned long long)wq, m->sdf, m->valid, m->rgb);
        LAUNCHCHK(ctx);
    }
    return run_extract(m, s, n, n_vertices, n_triangles);
}

int cf_mesh_extract_grid(cf_mesher* m, const cf_mesh_grid* grid, const float* sdf_host, const uint8_t* valid_host, const float* rgb_host,
                         uint32_t* n_vertices, uint32_t* n_triangles)
{
    if (!m || !grid || !n_vertices || !n_triangles) return CF_EINVAL;
    cf_ctx* ctx = m->ctx;
    const long long n = grid_samples(grid, m->max_voxels);
    if (n == -1) return mesh_fail(ctx, CF_EINVAL, "malformed grid (negative size, or no positive finite voxel)");
    if (n == -2) return mesh_fail(ctx, CF_ERANGE, "the grid has more samples than the mesher's max_voxels");
    if (n && (!sdf_host || !valid_host)) return CF_EINVAL;
    hipStream_t s;
    if (int r = mesh_stream(ctx, &s)) return r;
    m->grid = *grid;
    m->have_acc = false;   // (the field no longer belongs to the accumulators)
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(m->sdf, sdf_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(m->valid, valid_host, (size_t)n, hipMemcpyHostToDevice, s));
        if (rgb_host) HIPCHK(ctx, hipMemcpyAsync(m->rgb, rgb_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
        else HIPCHK(ctx, hipMemsetAsync(m->rgb, 0, (size_t)n * 3 * sizeof(float), s));
        HIPCHK(ctx, hipStreamSynchronize(s));   // (the caller's arrays are pageable: they are free again on return)
    }
    HIPCHK(ctx, hipEventRecord(m->ev[2], s));
    return run_extract(m, s, (size_t)n, n_vertices, n_triangles);
}

int cf_mesh_download(cf_mesher* m, cf_mesh_vertex* vertices, uint32_t* triangles)
{
    if (!m) return CF_EINVAL;
    cf_ctx* ctx = m->ctx;
    if (!m->have_mesh) return mesh_fail(ctx, CF_ESTATE, "cf_mesh_download before an extraction");
    const hipStream_t s = ctx->forked ? ctx->forked_from : ctx->stream;
    if (vertices && m->n_vertices) HIPCHK(ctx, hipMemcpyAsync(vertices, m->verts, (size_t)m->n_vertices * sizeof(cf_mesh_vertex), hipMemcpyDeviceToHost, s));
    if (triangles && m->n_triangles) HIPCHK(ctx, hipMemcpyAsync(triangles, m->tris, (size_t)m->n_triangles * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return CF_OK;
}

int cf_mesh_grid_download(cf_mesher* m, int64_t* acc_host)
{
    if (!m || !acc_host) return CF_EINVAL;
    cf_ctx* ctx = m->ctx;
    if (!m->have_acc) return mesh_fail(ctx, CF_ESTATE, "cf_mesh_grid_download before cf_mesh_accumulate");
    const size_t n = (size_t)grid_samples(&m->grid, m->max_voxels);
    const hipStream_t s = ctx->forked ? ctx->forked_from : ctx->stream;
    if (n) HIPCHK(ctx, hipMemcpyAsync(acc_host, m->acc, n * kPlanes * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return CF_OK;
}

int cf_mesh_timing(cf_mesher* m, float* accumulate_ms, float* extract_ms)
{
    if (!m) return CF_EINVAL;
    cf_ctx* ctx = m->ctx;
    if (accumulate_ms) {
        *accumulate_ms = 0.0f;
        if (m->timed[0]) { HIPCHK(ctx, hipEventSynchronize(m->ev[1])); HIPCHK(ctx, hipEventElapsedTime(accumulate_ms, m->ev[0], m->ev[1])); }
    }
    if (extract_ms) {
        *extract_ms = 0.0f;
        if (m->timed[1]) { HIPCHK(ctx, hipEventSynchronize(m->ev[3])); HIPCHK(ctx, hipEventElapsedTime(extract_ms, m->ev[2], m->ev[3])); }
    }
    return CF_OK;
}

}  // extern "C"
