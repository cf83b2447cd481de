// surf_index_dev.h -- the index maps of a model: EXTENTS, the z-key rasteriser and the resolve (part of surfel.hip's translation unit).
// Stage: index_map.* (Model::predictIndices) -- index_splat_kernel (64-bit atomicMin z|id keys) + index_resolve_kernel -- with their
// batch launchers.  (index_splat_body also runs beside the compaction in surfel.hip's indexsplat_scatter_kernel.)
#pragma once
#include "surf_batch_dev.h"

namespace cf {

// ==================================================================================== extents ====
// EXTENTS (round 9).  An object model covers a small part of the screen, and the resolve of the index pass used to rewrite every texel
// outside it with the empty value it already held.  The index maps of a model keep a ring of three pixel rectangles in device memory,
// four words each: ~xmin, ~ymin, xmax + 1, ymax + 1 -- complemented lower bounds, so that zero is the empty rectangle and
// every update is an atomicMax (as ModelMapsArgs::aabb).  The rasteriser of pass k extends slot k mod 3 by every pixel whose key it may
// write; the resolve of pass k handles the waves that meet that rectangle (keys to clear, texels to write) or the one of pass k - 1
// (texels to put back to empty), and one of its threads zeroes slot (k + 1) mod 3 for the next rasteriser -- nothing else touches that
// slot at that point of the stream, so there are no fences, no tickets and no workgroup waits for another.  Every other wave returns:
// its texels hold the empty value already.  The host counts k and says when the previous rectangle is not known (bit 2 of ext_slot:
// the pass then handles every texel and leaves a known state); ext == nullptr is the launch without any of this.  (The prediction's two
// kernels had the same for a while: its resolve gained 2.4 us per frame, its rasteriser -- four lanes per surfel, so four times the waves
// and the same-address atomics of the index rasteriser -- lost 5-9 us whichever way the rectangle was reduced and published.  Taken out.)
extern "C" __device__ unsigned int __ockl_wfred_max_u32(unsigned int);   // the device library's wave reduction (row shifts and broadcasts, no LDS)
// The rasteriser's half, in two steps.  extent_peek at the head of the kernel: lane l reads word l & 3 of the slot, in the same flight as
// the surfel.  extent_extend once the lane knows its pixels: the wave's rectangle, and lanes 0-3 raise the words it exceeds -- against the
// value read at the head (read before the atomic: after the first waves almost no wave still extends the rectangle -- track_prep.hip, the
// aabb keys -- and a stale value only costs an atomic that changes nothing), without waiting for anything: the atomics return no value.
__device__ __forceinline__ unsigned extent_peek(const unsigned* e) { return __hip_atomic_load(&e[threadIdx.x & 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void extent_extend(unsigned* __restrict__ e, unsigned peeked, bool ok, int x_lo, int y_lo, int x_hi, int y_hi)
{   // (every lane of the wave arrives here: lanes without a pixel carry the empty rectangle)
    const unsigned k0 = __ockl_wfred_max_u32(ok ? ~(unsigned)x_lo : 0u), k1 = __ockl_wfred_max_u32(ok ? ~(unsigned)y_lo : 0u);
    const unsigned k2 = __ockl_wfred_max_u32(ok ? (unsigned)x_hi + 1u : 0u), k3 = __ockl_wfred_max_u32(ok ? (unsigned)y_hi + 1u : 0u);
    const int lane = threadIdx.x & 63;
    if (lane < 4) {
        const unsigned key = lane == 0 ? k0 : lane == 1 ? k1 : lane == 2 ? k2 : k3;
        if (key > peeked) atomicMax(&e[lane], key);
    }
}
__device__ __forceinline__ bool extent_meets(const unsigned* __restrict__ e, int x0, int x1, int y0, int y1)
{
    const unsigned nx = e[0], ny = e[1], mx = e[2], my = e[3];   // (uniform address: scalar loads)
    return (unsigned)x0 < mx && (unsigned)y0 < my && (unsigned)x1 >= ~nx && (unsigned)y1 >= ~ny;   // (empty: mx == 0)
}
// May the wave that holds texels [q0, q0 + 64) of a resolve pass leave?  Also zeroes the ring's next slot (one thread quartet of the share).
// Conservative for any width: a run that straddles two rows counts as both rows in full.
__device__ __forceinline__ bool extent_culled(unsigned* __restrict__ ext, int ext_slot, int bid, int q0, int cols, int n_texels)
{
    const int slot = ext_slot & 3, next = slot == 2 ? 0 : slot + 1, prev = slot == 0 ? 2 : slot - 1;
    if (bid == 0 && threadIdx.x < 4) ext[4 * next + threadIdx.x] = 0u;
    if (ext_slot & 4) return false;   // the previous rectangle is not known: every texel
    const int q1 = min(q0 + 63, n_texels - 1), y0 = q0 / cols, y1 = q1 / cols;
    const int x0 = y0 == y1 ? q0 - y0 * cols : 0, x1 = y0 == y1 ? q1 - y0 * cols : cols - 1;
    return !extent_meets(ext + 4 * slot, x0, x1, y0, y1) && !extent_meets(ext + 4 * prev, x0, x1, y0, y1);
}

// ================================================================================= index map ====
// index_map.vert:38-63
__device__ __forceinline__ bool index_project(const float4 pc, const float4 ct, const Mat4& t_inv, cf_cam cam, int cols, int rows,
                                              float maxDepth, int time, int timeDelta, f3& ph, int& q)
{
    if ((float)time - ct.w > (float)timeDelta) return false;
    return surfel_project(pc, t_inv, cam, cols, rows, maxDepth, ph, q);   // (cf_surfel_device.h)
}

struct IndexArgs {   // predictIndices of one model (both kernels)
    const float4* surfels; const unsigned* count; Mat4 t_inv; float maxDepth; int time, timeDelta; unsigned id_begin, id_end;
    int ext_slot;             // the ring slot of this pass (bits 0-1), bit 2: the previous rectangle is not known (EXTENTS above; in what was padding)
    unsigned long long* keys; unsigned* index; float4* vertConf; float4* colorTime; float4* normRad;
    const float* t_inv_dev;   // nullable: the matrix in device memory instead (IndexPassArgs::t_inv_dev)
    float4* clean_rec; const float* clean_depth;   // nullable: the clean pass's packed per-texel records (IndexPassArgs::clean_rec)
    unsigned* ext;            // nullable: the ring of three rectangles of the model's index maps, [3][4]
};
__device__ __forceinline__ Mat4 index_matrix(const IndexArgs& a)
{
    if (!a.t_inv_dev) return a.t_inv;
    Mat4 m;
#pragma unroll
    for (int k = 0; k < 16; k++) m.m[k] = a.t_inv_dev[k];   // (uniform address: one request per wave)
    return m;
}
// (the inverse of a tracked pose is left in the tracker's state by the last solve of its schedule -- OdomDev::pose_inv -- since round 6: a
// kernel of its own, pose_tinv_kernel, until then)
struct FrameGeom { cf_cam cam; int cols, rows; };   // what the models of a launch share

__device__ __forceinline__ void index_splat_body(const Batch<IndexArgs>& B, const FrameGeom& g, int blk)
{
    const VBlock vb = batch_decode_at(B.h, blk);
    const IndexArgs& a = B.m[vb.model];
    const float4* __restrict__ surfels = a.surfels;
    // [id_begin, id_end): the surfel range of this launch (the whole map, or a rank's shard of it)
    const unsigned id = a.id_begin + vb.bid * kB + threadIdx.x;
    unsigned* const slot = a.ext ? a.ext + 4 * (a.ext_slot & 3) : nullptr;
    const unsigned peeked = slot ? extent_peek(slot) : 0u;
    bool ok = id < *a.count && id < a.id_end;
    f3 ph; int q = 0;
    if (ok) {
        const Mat4 T = index_matrix(a);
        ok = index_project(surfels[id * 3], surfels[id * 3 + 1], T, g.cam, g.cols, g.rows, a.maxDepth, a.time, a.timeDelta, ph, q);
    }
    if (ok) atomicMin(&a.keys[q], zkey(ph.z, id));
    if (!slot || __ballot(ok) == 0) return;   // (uniform: the wave stays whole for the reduction)
    const int y = q / g.cols, x = q - y * g.cols;
    extent_extend(slot, peeked, ok, x, y, x, y);
}
__global__ void __launch_bounds__(kB) index_splat_kernel(const Batch<IndexArgs> B, const FrameGeom g) { index_splat_body(B, g, (int)blockIdx.x); }

__global__ void __launch_bounds__(kB) index_resolve_kernel(const Batch<IndexArgs> B, const FrameGeom g)
{
    const VBlock vb = batch_decode(B.h);
    const IndexArgs& a = B.m[vb.model];
    const float4* __restrict__ surfels = a.surfels; unsigned long long* __restrict__ keys = a.keys; unsigned* __restrict__ index = a.index;
    float4* __restrict__ vertConf = a.vertConf; float4* __restrict__ colorTime = a.colorTime; float4* __restrict__ normRad = a.normRad;
    const int q = vb.bid * kB + threadIdx.x;
    if (a.ext) {   // (uniform) EXTENTS: a wave outside this pass's and the previous pass's rectangle has nothing to read or to change ...
        const int q0 = __builtin_amdgcn_readfirstlane(q & ~63);
        if (q0 >= g.cols * g.rows) return;
        if (extent_culled(a.ext, a.ext_slot, vb.bid, q0, g.cols, g.cols * g.rows)) {
            // ... except the clean stage's records: their eighth word is THIS frame's filtered depth, and clean_kernel reads patches far from
            // the map's footprint (around fresh surfels, around surfels the index pass gated out)
            if (a.clean_rec && q < g.cols * g.rows) {
                a.clean_rec[2 * q] = make_float4(0, 0, 0, 0); a.clean_rec[2 * q + 1] = make_float4(0, 0, __uint_as_float(0u), a.clean_depth[q]);
            }
            return;
        }
    }
    if (q >= g.cols * g.rows) return;
    const unsigned long long k = keys[q];
    keys[q] = kEmptyKey;  // leave the z-buffer cleared for the next pass (no memset launch per projection)
    // The pass in front of the clean stage also leaves what clean_kernel stages per texel as ONE 32-byte record (vertConf | colorTime.zw, index,
    // the frame's filtered depth) beside the arrays the other passes read (late in round 6: +7 us here, -17 us there).  Measured as well:
    // the two halves changing lanes so that every store instruction of a wave writes 1 KB in one piece (no gain: 23.4 against 22.8 us -- it
    // is the bytes, not the store pattern), and a 16-byte record without vertConf (clean_kernel's comment).
    float4* __restrict__ const rec = a.clean_rec;
    const float dflt = rec ? a.clean_depth[q] : 0.f;
    if (k == kEmptyKey) {
        index[q] = 0;
        vertConf[q] = colorTime[q] = normRad[q] = make_float4(0, 0, 0, 0);
        if (rec) { rec[2 * q] = make_float4(0, 0, 0, 0); rec[2 * q + 1] = make_float4(0, 0, __uint_as_float(0u), dflt); }
        return;
    }
    const unsigned id = (unsigned)k;
    const float4 pc = surfels[id * 3], ct = surfels[id * 3 + 1], nr = surfels[id * 3 + 2];
    const Mat4 T = index_matrix(a);
    const f3 ph = xform_point(T, f3{pc.x, pc.y, pc.z});
    const f3 n = normalized(xform_dir(T, f3{nr.x, nr.y, nr.z}));
    index[q] = id;
    vertConf[q] = make_float4(ph.x, ph.y, ph.z, pc.w);
    colorTime[q] = ct;
    normRad[q] = make_float4(n.x, n.y, n.z, nr.w);
    if (rec) { rec[2 * q] = make_float4(ph.x, ph.y, ph.z, pc.w); rec[2 * q + 1] = make_float4(ct.z, ct.w, __uint_as_float(id), dflt); }
}

static IndexArgs index_args(const IndexPassArgs& h)
{
    return IndexArgs{reinterpret_cast<const float4*>(h.surfels), h.count, mat4_from(h.t_inv), h.maxDepth, h.time, h.timeDelta, h.id_begin, h.id_end,
                     h.ext_slot, h.keys, h.index, reinterpret_cast<float4*>(h.vertConf), reinterpret_cast<float4*>(h.colorTime),
                     reinterpret_cast<float4*>(h.normRad), h.t_inv_dev, reinterpret_cast<float4*>(h.clean_rec), h.clean_depth, h.ext};
}
static int index_blocks(const IndexPassArgs& h) { return h.id_end > h.id_begin ? gridFor(h.id_end - h.id_begin) : 0; }   // the rasteriser's
void launch_index_keys_batch(hipStream_t s, const IndexPassArgs* items, int n_items, cf_cam cam, int cols, int rows)
{
    const FrameGeom g{cam, cols, rows};
    for_each_batch<IndexArgs>(items, n_items, [](const IndexPassArgs& h, IndexArgs& a) { a = index_args(h); return index_blocks(h); },
        [&](Batch<IndexArgs>& B, const int* blocks, int nb, const IndexPassArgs*) {
            if (const int grid = batch_layout(B, blocks, nb)) index_splat_kernel<<<grid, kB, 0, s>>>(B, g);
        });
}
void launch_index_resolve_batch(hipStream_t s, const IndexPassArgs* items, int n_items, cf_cam cam, int cols, int rows)
{
    const FrameGeom g{cam, cols, rows};
    for_each_batch<IndexArgs>(items, n_items, [&](const IndexPassArgs& h, IndexArgs& a) { a = index_args(h); return gridFor((long long)cols * rows); },
        [&](Batch<IndexArgs>& B, const int* blocks, int nb, const IndexPassArgs*) {
            index_resolve_kernel<<<batch_layout(B, blocks, nb), kB, 0, s>>>(B, g);   // (always: the resolve also clears the keys)
        });
}

}  // namespace cf
