// surf_batch_dev.h -- what every stage of surfel.hip shares: workgroup counts, the XCD-aware workgroup orders, the lock-step batch
// (table, decode, layout and THE host loop over the batches of a pass) and the 64-bit z-keys.  (Part of surfel.hip's translation unit.)
#pragma once

#include "cf_surfel_device.h"
#include "cf_kernels.h"

namespace cf {

static constexpr int kB = 256;
static inline int gridFor(long long n, int wg = kB) { return (int)((n + wg - 1) / wg); }
// XCD-aware workgroup order for passes that gather from the index-map images: the hardware deals consecutive workgroups round-robin
// over the 8 XCDs, each with its own L2, so neighbouring workgroups -- neighbouring surfels / pixels, which read the same image
// lines -- would pull every line into all eight L2s.  With a grid that is a multiple of 8, XCD x is given the x-th contiguous range
// of logical workgroups (a band of the image / a run of the surfel buffer) instead.
static inline int gridXcd(long long n, int chunk = 1, int wg = kB) { const int q = 8 * (chunk > 1 ? chunk : 1); return (gridFor(n, wg) + q - 1) / q * q; }  // xcd_block is a bijection on it
// chunk > 0: the XCDs take turns on runs of `chunk` consecutive logical workgroups (locality inside a run, balance between the XCDs
// when the cost per workgroup drifts along the buffer); chunk < 0: one band per XCD; 0: plain round-robin (the hardware's order).
// (the orders in use were chosen by measurement, DESIGN-NOTES.md; a diagnostics build -- make ABLATE=1 -- reads them from the environment)
#ifdef CF_ABLATE
static int xcd_env(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
#else
static constexpr int xcd_env(const char*, int dflt) { return dflt; }
#endif
// LOCK-STEP BATCHES (round 4).  The surfel passes of a frame are the same chain of ~16 kernels for every model, and an object model's
// share of each is a few dozen workgroups: as one chain per model on its own stream (rounds 1-3) the five chains of configs[2] took
// 450 us of a 1.5 ms frame -- the HIP streams share a handful of hardware queues, so chains ran one after another, 100 launch-floor
// kernels in all (profiles/r4e timeline).  Now every stage is ONE launch for all models of the batch, exactly as the tracking
// launches have been since round 1: a one-dimensional grid [model 0's workgroups | model 1's | ...], the running totals in the
// kernel arguments (BatchHdr), each model's arguments beside them.  A workgroup finds its model with 15 scalar compares and then
// runs the unchanged per-model code on its virtual block index.  Every model's share starts at a multiple of 8 workgroups, so the
// XCD of a workgroup (hardware id mod 8) is also that of its virtual index (xcd_block).
struct BatchHdr { int n; int blk_end[kSurfBatch]; };
template <class A> struct Batch { BatchHdr h; A m[kSurfBatch]; };
struct VBlock { int model, bid, nblk; };
__device__ __forceinline__ VBlock batch_decode_at(const BatchHdr& h, int b)
{
    int slot = 0;
#pragma unroll
    for (int k = 0; k < kSurfBatch - 1; k++) slot += (b >= h.blk_end[k]) ? 1 : 0;
    const int start = slot ? h.blk_end[slot - 1] : 0;
    return VBlock{slot, b - start, h.blk_end[slot] - start};
}
__device__ __forceinline__ VBlock batch_decode(const BatchHdr& h) { return batch_decode_at(h, (int)blockIdx.x); }
// host side: the table of a launch from the models' workgroup counts (each padded to a multiple of 8); returns the grid size -- zero
// exactly when no model has a workgroup
template <class A>
static int batch_layout(Batch<A>& B, const int* blocks, int n)
{
    int total = 0;
    B.h.n = n;
    for (int k = 0; k < kSurfBatch; k++) {
        if (k < n) total += (blocks[k] + 7) / 8 * 8;
        B.h.blk_end[k] = k < n ? total : 0x7fffffff;
    }
    return total;
}
// host side: the loop of every batched pass.  The models' host arguments go out kSurfBatch at a time: item(h, a) turns one model's
// arguments h into its device arguments a and returns its workgroup count, launch(B, blocks, nb, h) enqueues the nb models of one
// batch (h: their host arguments) -- it lays the table out (batch_layout) and decides what an empty batch means for its pass.
template <class A, class H, class Item, class Launch>
static void for_each_batch(const H* items, int n_items, Item item, Launch launch)
{
    for (int base = 0; base < n_items; base += kSurfBatch) {
        const int nb = n_items - base < kSurfBatch ? n_items - base : kSurfBatch;
        Batch<A> B;
        int blocks[kSurfBatch];
        for (int k = 0; k < nb; k++) blocks[k] = item(items[base + k], B.m[k]);
        launch(B, blocks, nb, items + base);
    }
}

__device__ __forceinline__ int xcd_block(int chunk, int b, int nblk)
{
    if (chunk == 0) return b;
    const int per = nblk >> 3, x = b & 7, r = b >> 3;  // XCD, rank inside the XCD
    if (chunk < 0) return x * per + r;
    const int lb = ((r / chunk) * 8 + x) * chunk + (r % chunk);
    return lb;  // (the grid is a multiple of 8 * chunk: a bijection)
}

__device__ __forceinline__ unsigned sortable_bits(float z)
{  // order-preserving float -> uint
    const unsigned b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long zkey(float z, unsigned id) { return ((unsigned long long)sortable_bits(z) << 32) | id; }
constexpr unsigned long long kEmptyKey = ~0ull;

static Mat4 mat4_from(const float m[16]) { Mat4 r; for (int i = 0; i < 16; i++) r.m[i] = m[i]; return r; }

}  // namespace cf
