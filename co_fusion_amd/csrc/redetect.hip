// redetect.hip -- re-detection of inactive object models (CoFusion::redetectModels; the reference left the hook empty,
// Core/CoFusion.cpp:599-602).  DESIGN.md 4.13 states the arithmetic; tests/redetect_ref.py restates it in numpy.
//
//   redetect_score_kernel    every stable surfel of every candidate map, projected under the candidate's hypothesis pose exactly as the
//                            index pass projects it (surfel_project, cf_surfel_device.h), compared with the frame's raw depth and label
//                            image: five u32 counters per candidate and a bitmap of the labelled pixels it explains
//   redetect_finish_kernel   popcount of the bitmaps (= distinct pixels), the number of pixels that carry the new label; leaves the
//                            bitmaps cleared for the next call -- the ONE place that keeps "bitmaps are zero between calls"
//   relabel_kernel           label image from -> to, 16 bytes per lane
//
// All results are integer counts: independent of launch shape and of the order the atomics land in.  The passes stream 16 B per surfel
// (row 0 of the 48 B record: position | confidence) and gather 5 B per projected surfel; the five counters are reduced per wave, then
// per workgroup in LDS, then ONE atomic per counter and workgroup.
#include "cf_surfel_device.h"
#include "cf_kernels.h"

namespace cf {

static constexpr int kRB = 256;             // threads per workgroup (4 waves)
static constexpr int kScorePerThread = 8;   // surfels a thread walks (grid-stride) when the host's count bound is exact
static constexpr int kFinishBlocks = 4;     // workgroups per candidate bitmap
static constexpr int kLabelBlocks = 8;      // workgroups counting the labelled pixels

// v summed over the workgroup and added to *dst by ONE atomic (none when the sum is zero).  Every thread of the workgroup calls it.
template <int K>
__device__ __forceinline__ void block_add(unsigned (&v)[K], unsigned* __restrict__ dst)
{
    __shared__ unsigned part[K][kRB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        unsigned s = v[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) part[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < kRB / 64; w++) s += part[threadIdx.x][w];
        if (s) atomicAdd(&dst[threadIdx.x], s);
    }
}

struct RedetectArgs {
    RedetectCand c[kRedetectBatch];
    int slot_end[kRedetectBatch];    // running totals of the workgroups per candidate; unused slots end at INT_MAX
    RedetectFrame f;
    unsigned* bits; unsigned words;  // [n][words] pixel bitmaps, zero on entry
    unsigned* counts;                // [kRedetectBatch][kRedetectWords] + label_pixels, zero on entry
};

__global__ void __launch_bounds__(kRB) redetect_score_kernel(const RedetectArgs a)
{
    const int b = (int)blockIdx.x;
    int slot = 0;
#pragma unroll
    for (int k = 0; k < kRedetectBatch - 1; k++) slot += (b >= a.slot_end[k]) ? 1 : 0;
    const int start = slot ? a.slot_end[slot - 1] : 0;
    const unsigned bid = (unsigned)(b - start), nblk = (unsigned)(a.slot_end[slot] - start);
    const RedetectCand& c = a.c[slot];
    const float4* __restrict__ surfels = reinterpret_cast<const float4*>(c.surfels);
    const float* __restrict__ depth = a.f.depth; const uint8_t* __restrict__ label = a.f.label;
    unsigned* __restrict__ bits = a.bits + (size_t)slot * a.words;
    unsigned count = *c.count;                       // the true count; the host's bound only sized the launch ...
    if (count > c.count_bound) count = c.count_bound;   // ... and bounds the reads (an upper bound of a count still in flight)
    Mat4 T;
#pragma unroll
    for (int k = 0; k < 16; k++) T.m[k] = c.t_inv[k];
    // projected, occluded, seen_through, agree, agree_on_label
    unsigned n[5] = {0, 0, 0, 0, 0};
    for (unsigned i = bid * kRB + threadIdx.x; i < count; i += nblk * kRB) {
        const float4 pc = surfels[(size_t)i * 3];
        if (!(pc.w >= c.theta)) continue;
        f3 ph; int q;
        if (!surfel_project(pc, T, a.f.cam, a.f.cols, a.f.rows, a.f.cutoff, ph, q)) continue;
        n[0]++;
        const float d = depth[q];
        if (!(d > 0.0f) || d > a.f.cutoff) continue;
        const float lo = ph.z - a.f.tol, hi = ph.z + a.f.tol;
        if (d < lo) n[1]++;
        else if (d > hi) n[2]++;
        else {
            n[3]++;
            if ((int)label[q] == a.f.new_label) { n[4]++; atomicOr(&bits[(unsigned)q >> 5], 1u << (q & 31)); }
        }
    }
    block_add(n, a.counts + slot * kRedetectWords);
}

__device__ __forceinline__ unsigned count_bytes_equal(unsigned w, unsigned v)
{
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) n += (((w >> (8 * k)) & 255u) == v) ? 1u : 0u;
    return n;
}

// blocks [0, n * kFinishBlocks): popcount + clear of candidate (b / kFinishBlocks)'s bitmap; the kLabelBlocks after them count label == L
__global__ void __launch_bounds__(kRB) redetect_finish_kernel(unsigned* __restrict__ bits, unsigned words, int n, const uint8_t* __restrict__ label,
                                                              unsigned n_px, unsigned new_label, unsigned* __restrict__ counts)
{
    const int b = (int)blockIdx.x;
    unsigned s[1] = {0};
    if (b < n * kFinishBlocks) {
        const int c = b / kFinishBlocks, part = b - c * kFinishBlocks;
        unsigned* __restrict__ w = bits + (size_t)c * words;
        for (unsigned i = part * kRB + threadIdx.x; i < words; i += kFinishBlocks * kRB) {
            const unsigned v = w[i];
            if (v) { s[0] += __popc(v); w[i] = 0; }
        }
        block_add(s, counts + c * kRedetectWords + 5);
        return;
    }
    const unsigned lb = (unsigned)(b - n * kFinishBlocks);
    // 16-byte pieces where the image starts on a 16-byte boundary, the bytes behind the last whole piece one by one
    const bool vec = (reinterpret_cast<uintptr_t>(label) & 15u) == 0;
    const unsigned n_vec = vec ? n_px / 16 : 0;
    const uint4* __restrict__ l4 = reinterpret_cast<const uint4*>(label);
    for (unsigned i = lb * kRB + threadIdx.x; i < n_vec; i += kLabelBlocks * kRB) {
        const uint4 v = l4[i];
        s[0] += count_bytes_equal(v.x, new_label) + count_bytes_equal(v.y, new_label) + count_bytes_equal(v.z, new_label) + count_bytes_equal(v.w, new_label);
    }
    for (unsigned i = n_vec * 16 + lb * kRB + threadIdx.x; i < n_px; i += kLabelBlocks * kRB) s[0] += (label[i] == new_label) ? 1u : 0u;
    block_add(s, counts + kRedetectBatch * kRedetectWords);
}

__device__ __forceinline__ unsigned relabel_word(unsigned w, unsigned from, unsigned to)
{
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (((w >> (8 * k)) & 255u) == from) w = (w & ~(255u << (8 * k))) | (to << (8 * k));
    return w;
}
// label (16-byte aligned) [n]: thread t < n / 16 rewrites piece t, the threads behind them one byte each of the last n % 16
__global__ void __launch_bounds__(kRB) relabel_kernel(uint8_t* __restrict__ label, unsigned long long n, unsigned from, unsigned to)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * kRB + threadIdx.x, n_vec = n / 16;
    if (t < n_vec) {
        uint4* p = reinterpret_cast<uint4*>(label) + t;
        const uint4 v = *p;
        const uint4 r = make_uint4(relabel_word(v.x, from, to), relabel_word(v.y, from, to), relabel_word(v.z, from, to), relabel_word(v.w, from, to));
        if (r.x != v.x || r.y != v.y || r.z != v.z || r.w != v.w) *p = r;
        return;
    }
    const unsigned long long i = n_vec * 16 + (t - n_vec);
    if (i < n && label[i] == from) label[i] = (uint8_t)to;
}

void launch_redetect_score(hipStream_t s, const RedetectCand* cands, int n, const RedetectFrame& f, unsigned* bits, unsigned words, unsigned* counts)
{
    RedetectArgs a{};
    int total = 0;
    for (int k = 0; k < kRedetectBatch; k++) {
        if (k < n) {
            a.c[k] = cands[k];
            // (an empty candidate keeps one workgroup: its slot must exist for the table's compares)
            long long blocks = ((long long)cands[k].count_bound + kRB * kScorePerThread - 1) / (kRB * kScorePerThread);
            blocks = blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks;
            total += (int)blocks;
        }
        a.slot_end[k] = k < n ? total : 0x7fffffff;
    }
    a.f = f; a.bits = bits; a.words = words; a.counts = counts;
    hipLaunchKernelGGL(redetect_score_kernel, dim3(total), dim3(kRB), 0, s, a);
    hipLaunchKernelGGL(redetect_finish_kernel, dim3(n * kFinishBlocks + kLabelBlocks), dim3(kRB), 0, s, bits, words, n, f.label,
                       (unsigned)(f.cols * f.rows), (unsigned)f.new_label, counts);
}

void launch_relabel(hipStream_t s, uint8_t* label, unsigned long long n, unsigned from, unsigned to)
{
    const unsigned long long threads = n / 16 + n % 16;
    if (!threads) return;
    hipLaunchKernelGGL(relabel_kernel, dim3((unsigned)((threads + kRB - 1) / kRB)), dim3(kRB), 0, s, label, n, from, to);
}

}  // namespace cf
