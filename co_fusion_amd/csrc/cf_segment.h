// cf_segment.h -- what segment.hip (the motion branch) and segment_masks.hip (the label-mask branch) share: the batching of kernel
// arguments over the sequences of a lock-step group, the blocked sequential f32 chain, the workgroup scan and the phase stamps of the
// single-workgroup kernels, the capacities of their tables, and the segmenter itself.
#pragma once
#include <vector>

#include "cf_host.h"

namespace cf {

// The kernels of the segmentation chain take the arguments of up to kSegBatch segmenters (the sequences of a lock-step group, all of
// one image size) in the kernel-argument segment and pick theirs with the grid's last dimension: one chain of launches for the group
// instead of one per sequence.  A single segmenter is a batch of one.
constexpr int kSegBatch = 8;
template <class A, int N = kSegBatch> struct SegBatch { A m[N]; };

// Sequential f32 sum init + t[0] + t[1] + ... + t[n-1] (this order) by ONE wave.  term(j) -> the j-th term, 0.0f for "skip" (x + 0.0f == x
// for every x these sums can reach -- a running sum that starts at +0.0f is never -0.0f --, so skipping an element and adding zero agree).
// Returns the sum in every lane.
// Rounds 3-6 moved ONE term per step to the adder (v_readlane, an LDS broadcast, a lane shift): 11-14 ns per addition whichever way, because
// every step pays a cross-lane operation on top of the addition.  Late in round 6 the terms are BLOCKED instead: lane l owns kSeqBlock
// consecutive terms of a super-block of 64 x kSeqBlock; in "phase" l every lane adds its own block to the running sum -- sixteen dependent
// plain v_add_f32 from registers -- and the value lane l arrives at (the only one that started from the true prefix and added the right
// terms) is read back as the running sum of phase l + 1.  One cross-lane operation per sixteen additions: 8 ns per addition (what a
// dependent v_add_f32 of a lone wave costs here), 13.4 -> 9.8 us for the average confidences of 1 200 superpixels.  A lane whose block
// holds only zeros has no phase at all.  The additions and their order are exactly those of the serial loop.
constexpr int kSeqBlock = 16;
// the phases of one super-block: lane l holds its kSeqBlock consecutive terms in t[], `any` = one of them is not zero
__device__ __forceinline__ float seq_block_phases(float sum, const float (&t)[kSeqBlock], bool any)
{
    unsigned long long nz = __ballot(any);
    while (nz) {   // (uniform)
        const int ph = __builtin_ctzll(nz);
        nz &= nz - 1;
        float x = sum;
#pragma unroll
        for (int c = 0; c < kSeqBlock; c++) x = x + t[c];
        sum = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), ph));
    }
    return sum;
}

// label capacity of the kernels' static tables (labels incl. the "new model" label): model ids are 8 bits and 255 marks a rejected
// superpixel, the reference's own limit (CoFusion.cpp:631-634, Segmentation.cpp).  A segmenter's buffers are sized for
// cf_segmenter::Lcap = the context's max_models (cf_config), 16 by default.
constexpr int kMaxL = 256;
constexpr int kSegMaxK = 4800;   // superpixels of the largest supported image (1280x960): what the single-workgroup kernels hold in LDS

#ifdef CF_ABLATE
// diagnostics build (CF_SEG_TRACE=<inference>): phase stamps of segmenter 0's two single-workgroup kernels, 100 MHz constant clock, into
// g_seg_trace[2][16] -- defined once, by the translation unit whose kernels stamp (segment.hip, ahead of its stage headers)
#define GSTAMP(which, k) do { __syncthreads(); if (threadIdx.x == 0 && blockIdx.x == 0) g_seg_trace[which][k] = wall_clock64(); } while (0)
#else
#define GSTAMP(which, k) do {} while (0)
#endif

// Inclusive scan of one int per thread over the workgroup (<= 1024 threads): a wave-level scan (six shuffle steps), the waves' totals
// through LDS, every thread adds the totals of the waves in front of it -- two barriers instead of the 2 x log2(T) of the
// Hillis-Steele loop these kernels used until round 6 (twenty with sixteen waves, a few hundred ns each).  Returns the inclusive prefix;
// *total = the sum over the workgroup.  s_wave: >= 16 ints of LDS, free before and after.
__device__ __forceinline__ int block_scan_inclusive(int v, int* s_wave, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x + 63) >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    __syncthreads();   // (s_wave may still be read from a previous scan)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < nw; w++) { const int t = s_wave[w]; all += t; if (w < wave) before += t; }
    *total = all;
    return incl + before;
}
}  // namespace cf

struct cf_segmenter {
    cf_ctx* ctx = nullptr;
    int gx = 0, gy = 0, K = 0;
    int Lcap = 16;                       // label capacity of the buffers = max(16, the context's max_models) (a new label needs a free model slot)
    const void** d_acc_ptrs = nullptr;   // [2][Lcap] device copies of the models' ICP-error / vertex-confidence image pointers (> kAccTile models)
    const void** h_acc_ptrs = nullptr;   // pinned staging of the same
    int* labels = nullptr;
    float* centres = nullptr;
    unsigned long long* slic_sums = nullptr;
    unsigned* spix_count = nullptr; unsigned* depth_count = nullptr;
    unsigned long long *depth_sum = nullptr, *icp_sum = nullptr, *conf_sum = nullptr;
    int* resample = nullptr;
    unsigned char* low_map = nullptr;
    float *feat1 = nullptr, *feat2 = nullptr, *norm = nullptr, *K1t = nullptr, *K2t = nullptr;
    float* partial = nullptr;            // chunk partial sums [kCrfChunks][K][2][Lcap]
    std::vector<float> smooth_cache;     // host copy of the smoothness features K1t was built from
    float *unary = nullptr, *Q0 = nullptr, *Q1 = nullptr;
    // device-side unaries / post-processing (cf_seg_sums / cf_seg_infer / cf_seg_fetch)
    float *raw_mean = nullptr, *low_mean = nullptr;   // [(1 + 2 Lcap)][K]
    float *avg_conf = nullptr, *depth_range = nullptr;
    int* cc = nullptr;                   // [6][K]: seg_post_kernel's component statistics when they outgrow LDS
    cf_seg_result* d_result = nullptr;
    cf_seg_result* h_result = nullptr;   // pinned
    unsigned char* h_low_map = nullptr;  // pinned [K]
    long long* h_pose_tail = nullptr;    // pinned [Lcap][kPoseWords]: the tail of the sums block after the caller's all-reduce
    bool poses_published = false;
    bool grid_kernel_built = false;      // K1t holds the kernel of the grid's own smoothness features (seg_feat1_kernel)
    // cf_seg_early: 0 nothing pending, 1 the early half is enqueued, 2 cf_seg_sums put the ICP sums behind it -- and what it ran with
    int early = 0, early_n = 0;
    const float* early_depth = nullptr; const uint8_t* early_rgba = nullptr;
    std::vector<const float*> early_vconf;
    float early_scale[3] = {0.f, 0.f, 0.f};
    // the last inference, for cf_seg_buffer: which of Q0 / Q1 holds its marginals (launch_mean_field's flip), its models and labels
    int last_flip = 0, last_n = 0, last_L = 0;
    // label-mask branch (segment_masks.hip; cf_seg_masks / cf_seg_masks_batch / cf_seg_new_mask_value)
    unsigned* mask_work = nullptr;       // [2][kMaskWork] first new pixel + histograms: job k works in block k & 1 and leaves the other one reset
    int* h_mask_new = nullptr;           // pinned [1]: the mask value bound to the new label (-1: none), stored by mask_stats_kernel
    unsigned mask_jobs = 0;              // mask jobs enqueued so far (the parity picks the work block)
    bool mask_pending = false;           // a mask job is in flight: the next cf_seg_fetch collects its new mask value
    bool mask_value_valid = false;       // cf_seg_new_mask_value has something to hand out
    int mask_new_value = -1;
};

namespace cf {
// words of one work block of the mask branch: [0] the raster-first unmapped pixel (~0u: none), [1, 257) outIds, [257] the pixels whose
// unmapped mask value became label 0 (they count in no outIds bucket but in the depth statistics of label 0's row)
constexpr int kMaskWork = 260;
}  // namespace cf
