// surfel.hip -- the surfel half of the hot path as HIP compute kernels (no OpenGL, no interop).
//
// MI355X-native replacement of the GLSL passes driven by Core/Model/Model.cpp and
// Core/Model/ModelProjection.cpp:
//   depth_bilateral_metric.frag  -> bilateral_kernel
//   vertex_feedback.* / init     -> feedback_kernel + ordered compaction + init_kernel
//   index_map.*                  -> index_splat_kernel (64-bit atomicMin z|id keys) + index_resolve_kernel
//   splat.vert/combo_splat.frag  -> splat_raster_kernel (atomicMin) + splat_resolve_kernel
//   fill_*.frag                  -> fill_in_kernel
//   data.* + update.vert         -> associate_kernel (+ owner atomicMin) + update_kernel
//   copy_unstable.*              -> clean_kernel + ordered (stable) stream compaction
//
// The rasteriser's "nearest fragment wins, first primitive wins ties" becomes an atomicMin on a
// 64-bit key (order-preserving depth bits << 32 | surfel id); the transform-feedback append becomes
// a three-phase exclusive scan that preserves primitive order, so surfel ids and counts are exactly
// those of the reference's pipeline.  All passes are streaming / gather-scatter and HBM-bound:
// 48 B surfel records are read as 3 x float4 (16 B/lane), images are walked row-major by 256-thread
// workgroups.  Arithmetic is bit-identical to the CPU oracle (same operation order, no FMA contraction).
//
// One translation unit, one stage per file, every stage's launchers beside its kernels; this file keeps what spans stages: the two
// side-by-side kernels with their launcher, and the bound of the kernel-argument segment.
//   surf_batch_dev.h   workgroup counts, XCD orders, the lock-step batch (table, decode, layout, the host loop of every batched pass), z-keys
//   surf_scan_dev.h    the ordered compaction; set_count*, fill_zero
//   surf_boot_dev.h    bilateral filter, feedback and init (per frame / per model: no batch form)
//   surf_index_dev.h   EXTENTS, the index map: rasteriser and resolve
//   surf_splat_dev.h   the splat prediction: rays, rasteriser, resolve<mode> (+ fill-in and covered count); fill-in, fill ratio
//   surf_fuse_dev.h    association, update
//   surf_clean_dev.h   clean
// (cf_kernels.h: the launchers' declarations and the host-side pass arguments; cf_surfel_device.h: the shaders' helper functions.)
#include "surf_batch_dev.h"
#include "surf_scan_dev.h"
#include "surf_boot_dev.h"
#include "surf_index_dev.h"
#include "surf_splat_dev.h"
#include "surf_fuse_dev.h"
#include "surf_clean_dev.h"

namespace cf {

// the arguments of a batched launch travel in the 4 KB kernel-argument segment
static_assert(sizeof(Batch<FuseArgs>) + 16 <= 4096 && sizeof(Batch<CleanArgs>) + 16 <= 4096 && sizeof(Batch<IndexArgs>) + sizeof(FrameGeom) <= 4096 &&
              sizeof(Batch<SplatArgs>) + sizeof(FrameGeom) <= 4096 && sizeof(Batch<ScanArgs>) <= 4096, "lower kSurfBatch");
static_assert(sizeof(Batch<IndexArgs>) + sizeof(FrameGeom) + sizeof(Batch<ScanArgs>) + 16 <= 4096 && sizeof(Batch<UpdateArgs>) + sizeof(Batch<ScanArgs>) + 16 <= 4096,
              "the side-by-side launches carry two batches' arguments in one 4 KB kernel-argument segment");

// Launches that do not depend on each other, side by side in ONE grid (late in round 6).  Behind the association the frame's chain was
// block sums -> compaction -> update -> index keys -> ...: the compaction of the new surfels (flags / records of the association -> `fresh`)
// and the update of the old ones (-> the other surfel buffer) never read what the other writes, and neither does the second index pass's
// rasterisation, which only needs the update.  So: {update || block sums}, then {index keys || compaction} -- two launches of 5-6 us and their
// boundaries off the chain.  The longer part comes first in the grid.
__global__ void __launch_bounds__(kB) update_blocksums_kernel(const Batch<UpdateArgs> U, const Batch<ScanArgs> S, int u_blocks)
{
    const int b = (int)blockIdx.x;
    if (b < u_blocks) update_body(U, b);
    else scan_block_sums_body(S, b - u_blocks);
}
__global__ void __launch_bounds__(kB) indexsplat_scatter_kernel(const Batch<IndexArgs> I, const FrameGeom g, const Batch<ScanArgs> S, int i_blocks)
{
    const int b = (int)blockIdx.x;
    if (b < i_blocks) index_splat_body(I, g, b);
    else scan_scatter_body(S, b - i_blocks);
}

// {update || block sums of the new surfels' compaction}, {index keys of the pass behind the update || that compaction} (update_blocksums_kernel):
// what launch_scan_scatter_batch + launch_update_batch + launch_index_keys_batch enqueue as four launches, as two.  false (nothing
// enqueued) when the batch does not fit one launch or a compaction has no elements: the caller then takes the separate launches.
bool launch_update_compaction_index_keys(hipStream_t s, const UpdatePassArgs* up, const ScanPassArgs* sc, const IndexPassArgs* ix, int n, cf_cam cam, int cols,
                                         int rows)
{
    if (n <= 0 || n > kSurfBatch) return false;
    Batch<UpdateArgs> U; Batch<ScanArgs> S; Batch<IndexArgs> I;
    int ub[kSurfBatch], sb[kSurfBatch], ib[kSurfBatch];
    for (int k = 0; k < n; k++) {
        U.m[k] = update_args(up[k]); ub[k] = update_blocks(up[k]);
        S.m[k] = scan_args(sc[k]); sb[k] = scan_blocks(sc[k]);
        if (sb[k] == 0) return false;
        I.m[k] = index_args(ix[k]); ib[k] = index_blocks(ix[k]);
    }
    const int ug = batch_layout(U, ub, n), sg = batch_layout(S, sb, n), ig = batch_layout(I, ib, n);
    const FrameGeom g{cam, cols, rows};
    update_blocksums_kernel<<<ug + sg, kB, 0, s>>>(U, S, ug);
    indexsplat_scatter_kernel<<<ig + sg, kB, 0, s>>>(I, g, S, ig);
    return true;
}

}  // namespace cf
