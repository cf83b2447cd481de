// segment_masks.hip -- the label-mask branch of the segmentation (Segmentation.cpp:59-119) on the device: a mask with one value per
// object comes in with the frame, a 256-entry table maps mask values to model ids, at most one unmapped value per frame becomes a new
// model.  Until now this was three host loops over a host mask and a host depth image followed by an upload (Segmentation::
// performSegmentationGT); frames that already live in device memory could not use masks at all.  The results are those of
// oracle/orc_segment.c (orc_segment_gt) bit for bit.
//
// Three launches, ordered by the stream alone (no device-side wait, no meeting of workgroups; every loop is bounded by the image):
//   mask_first_new_kernel   the raster-first pixel whose value is non-zero and unmapped (wave minimum, one atomicMin per workgroup);
//                           not launched when no job of the chain may spawn a label
//   mask_label_kernel       the label image and the integer histograms (outIds; the pixels an unmapped value sent to label 0)
//   mask_stats_kernel       one wave per result row: pixel count, the two SEQUENTIAL f32 sums of the raw depth in raster order
//                           (depthMean, depthStd -- they become setMaxDepth of every object model, so their bits decide what is fused)
// The pixel count of a row is the sum of the label histogram over the labels that map to the row (integers: any order), formed by the
// row's own wave -- the table model id -> row index does not fit into the label kernel's arguments beside the mapping (8 x 256 bytes each).
//
// A job works in one of the segmenter's two work blocks (cf_segment.h: kMaskWork) and its label kernel leaves the OTHER block in the
// state the next job expects (first = none, histograms zero): the last reader of that block, the previous job's mask_stats_kernel, has
// finished by stream order.  No memset per frame.
#include <string.h>

#include <string>
#include <vector>

#include "cf_host.h"
#include "cf_segment.h"

using namespace cf;

namespace cf {

constexpr int kMaskPx = 16;           // pixels per thread of the two image kernels = pixels per lane and super-block of the sums (kSeqBlock)
constexpr unsigned kMaskNone = 0xffffffffu;
constexpr int kMaskBatchIds = 17;     // model ids per job of a batched chain (beyond: one chain per job with the full table, as cf_seg_run_batch does)
static_assert(kMaskPx == kSeqBlock, "a lane's 16-byte label load is one block of the sequential chain");

struct MaskLabelArgs {
    const unsigned char* mask; unsigned char* full;
    unsigned* work; unsigned* work_next;
    int allow_new; unsigned next_id;
    unsigned char mapping[256];        // mask value -> model id, 0 = unmapped
};
template <int CAP>
struct MaskStatsArgs {
    const unsigned char* full; const float* depth; const unsigned char* mask;
    const unsigned* work;
    cf_seg_result* result_host; int* new_host;
    int n_models; unsigned next_id;
    unsigned ids[CAP];                 // model ids in list order
    unsigned char m2i[256];            // modelIdToIndex (Segmentation.cpp:63-68): default 0, ids & 255, [next id] = n_models
};

__device__ __forceinline__ unsigned mask_byte(const uint4& v, int c)
{
    const unsigned w = (c >> 2) == 0 ? v.x : ((c >> 2) == 1 ? v.y : ((c >> 2) == 2 ? v.z : v.w));
    return (w >> ((c & 3) * 8)) & 255u;
}

// min over { i : mask[i] != 0 and mapping[mask[i]] == 0 } -> work[0] (atomicMin; ~0u on entry)
__global__ void __launch_bounds__(256) mask_first_new_kernel(const SegBatch<MaskLabelArgs> B, int nchunks)
{
    const MaskLabelArgs& a = B.m[blockIdx.y];
    if (!a.allow_new) return;   // (uniform)
    __shared__ unsigned char s_map[256];
    __shared__ unsigned s_min[4];
    const int t = threadIdx.x;
    s_map[t] = a.mapping[t];
    __syncthreads();
    const int ch = blockIdx.x * 256 + t;
    unsigned best = kMaskNone;
    if (ch < nchunks) {
        const uint4 v = reinterpret_cast<const uint4*>(a.mask)[ch];
#pragma unroll
        for (int c = kMaskPx - 1; c >= 0; c--) {
            const unsigned m = mask_byte(v, c);
            if (m && !s_map[m]) best = (unsigned)ch * kMaskPx + c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned other = __shfl_xor(best, o, 64); best = other < best ? other : best; }
    if ((t & 63) == 0) s_min[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; w++) best = s_min[w] < best ? s_min[w] : best;
        if (best != kMaskNone) atomicMin(&a.work[0], best);
    }
}

// full[i] and the histograms.  A thread owns 16 consecutive pixels (one 16-byte load, one 16-byte store); runs of one label inside them
// go to the LDS histogram as one addition (most of an image is a few long runs), the workgroup's histogram to memory with one atomic
// per label it met.
__global__ void __launch_bounds__(256) mask_label_kernel(const SegBatch<MaskLabelArgs> B, int nchunks)
{
    const MaskLabelArgs& a = B.m[blockIdx.y];
    __shared__ unsigned char s_map[256];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_unmapped;
    const int t = threadIdx.x;
    s_map[t] = a.mapping[t];
    s_hist[t] = 0;
    if (t == 0) s_unmapped = 0;
    if (blockIdx.x == 0)   // the other work block, for the segmenter's next job (see the head of this file)
        for (int k = t; k < kMaskWork; k += 256) a.work_next[k] = k == 0 ? kMaskNone : 0u;
    const unsigned first = a.work[0];                                      // (uniform)
    const unsigned new_value = first != kMaskNone ? a.mask[first] : 0u;    // the one value that spawns; 0: none
    const unsigned new_label = a.next_id & 255u;
    __syncthreads();
    const int ch = blockIdx.x * 256 + t;
    if (ch < nchunks) {
        const uint4 v = reinterpret_cast<const uint4*>(a.mask)[ch];
        unsigned out[4] = {0u, 0u, 0u, 0u};
        unsigned run_label = 0, run = 0, unmapped = 0;
#pragma unroll
        for (int c = 0; c < kMaskPx; c++) {
            const unsigned m = mask_byte(v, c);
            unsigned label = 0;
            bool counted = true;   // Segmentation.cpp:72-86: an unmapped value that does not spawn leaves label 0 and counts in no bucket
            if (m) {
                const unsigned mapped = s_map[m];
                if (mapped) label = mapped;
                else if (m == new_value) label = new_label;
                else counted = false;
            }
            out[c >> 2] |= label << ((c & 3) * 8);
            if (!counted) unmapped++;
            else if (run && label == run_label) run++;
            else {
                if (run) atomicAdd(&s_hist[run_label], run);
                run_label = label; run = 1;
            }
        }
        if (run) atomicAdd(&s_hist[run_label], run);
        if (unmapped) atomicAdd(&s_unmapped, unmapped);
        reinterpret_cast<uint4*>(a.full)[ch] = make_uint4(out[0], out[1], out[2], out[3]);
    }
    __syncthreads();
    if (s_hist[t]) atomicAdd(&a.work[1 + t], s_hist[t]);
    if (t == 0 && s_unmapped) atomicAdd(&a.work[257], s_unmapped);
}

// One of the two sums of a row: term(d) over the pixels whose label maps to the row, in raster order, from +0.0f.
// The chain is segment.hip's (cf_segment.h: seq_block_phases): lane l owns the 16 consecutive pixels [1024 b + 16 l, + 16) of super-block
// b, its terms are term(depth) where the label maps to this row and 0.0f elsewhere, a lane whose block holds no non-zero term has no
// phase.  Leaving a pixel out and adding 0.0f to the running sum agree because the sum starts at +0.0f: x + 0.0f == x for every x but
// -0.0f, and a sum that starts at +0.0f never becomes -0.0f (x + y is -0.0f only when both are) -- a label whose first depth is -0.0f
// included: (+0.0f) + (-0.0f) = +0.0f, what the serial loop holds after that pixel too.  (All depths are finite.)
// The next super-block's labels and depths (16-byte loads) are in flight during the phases of the current one, as in
// wave_sequential_sum_finite16.
// seq_block_phases for a super-block in which EVERY lane has a phase (the background's row over most of an image): the 64 phases unrolled,
// the lane a constant.  A lone wave issues one instruction of ANY kind per four cycles (the issue slot of its SIMD comes round every
// fourth cycle), so the six scalar instructions the loop spends per phase (find the lowest lane, clear its bit, test, branch) cost as
// much as six of the sixteen dependent additions: 24 issue slots per phase in the loop, 17-18 here (measured at 640x480, 5 rows:
// mask_stats_kernel 1.97 ms with the loop alone).  The additions and their order are the same.
__device__ __forceinline__ float seq_block_phases_all(float sum, const float (&t)[kSeqBlock])
{
#pragma unroll
    for (int ph = 0; ph < 64; ph++) {
        float x = sum;
#pragma unroll
        for (int c = 0; c < kSeqBlock; c++) x = x + t[c];
        sum = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), ph));
    }
    return sum;
}

template <class F>
__device__ __forceinline__ float mask_row_sum(const unsigned char* __restrict__ full, const float* __restrict__ depth, int nchunks, int lane,
                                              const unsigned char* s_mine, F term)
{
    float sum = 0.f;
    uint4 cur_l = make_uint4(0u, 0u, 0u, 0u), nxt_l;
    float4 cur_d[4], nxt_d[4];
#pragma unroll
    for (int q = 0; q < 4; q++) cur_d[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < nchunks) {
        cur_l = reinterpret_cast<const uint4*>(full)[lane];
#pragma unroll
        for (int q = 0; q < 4; q++) cur_d[q] = reinterpret_cast<const float4*>(depth)[(size_t)lane * 4 + q];
    }
    for (int j0 = 0; j0 < nchunks; j0 += 64) {
        const int jn = j0 + 64 + lane;
        nxt_l = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int q = 0; q < 4; q++) nxt_d[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jn < nchunks) {
            nxt_l = reinterpret_cast<const uint4*>(full)[jn];
#pragma unroll
            for (int q = 0; q < 4; q++) nxt_d[q] = reinterpret_cast<const float4*>(depth)[(size_t)jn * 4 + q];
        }
        const bool inside = j0 + lane < nchunks;   // (a lane past the image holds label 0, which may well map to this row)
        const float d[kSeqBlock] = {cur_d[0].x, cur_d[0].y, cur_d[0].z, cur_d[0].w, cur_d[1].x, cur_d[1].y, cur_d[1].z, cur_d[1].w,
                                    cur_d[2].x, cur_d[2].y, cur_d[2].z, cur_d[2].w, cur_d[3].x, cur_d[3].y, cur_d[3].z, cur_d[3].w};
        float t[kSeqBlock];
        unsigned mine[kSeqBlock];
        bool any = false;
        // (the sixteen table reads first and unconditionally -- the index is a byte, always inside the table -- so that they are in
        // flight together: behind `inside &&` each one was a branch and a round trip to LDS of its own)
#pragma unroll
        for (int c = 0; c < kSeqBlock; c++) mine[c] = s_mine[mask_byte(cur_l, c)];
#pragma unroll
        for (int c = 0; c < kSeqBlock; c++) {
            t[c] = (inside && mine[c] != 0) ? term(d[c]) : 0.f;
            any = any || (t[c] != 0.f);
        }
        sum = __ballot(any) == ~0ull ? seq_block_phases_all(sum, t) : seq_block_phases(sum, t, any);   // (uniform)
        cur_l = nxt_l;
#pragma unroll
        for (int q = 0; q < 4; q++) cur_d[q] = nxt_d[q];
    }
    return sum;
}

// grid (rows, segmenters), one wave each: row r < n_models is model r of the list, row n_models the new label (when there is one)
template <int CAP, int N>
__global__ void __launch_bounds__(64) mask_stats_kernel(const SegBatch<MaskStatsArgs<CAP>, N> B, int nchunks)
{
    const MaskStatsArgs<CAP>& a = B.m[blockIdx.y];
    const int r = blockIdx.x, lane = threadIdx.x;
    const unsigned first = a.work[0];
    const int has_new = first != kMaskNone ? 1 : 0;
    const int rows = a.n_models + has_new;
    if (r >= rows) return;   // (uniform)
    __shared__ unsigned char s_mine[256];   // label -> "its pixels belong to this row"
    unsigned cnt = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int label = lane * 4 + q;
        const bool mine = (int)a.m2i[label] == r;
        s_mine[label] = mine ? 1 : 0;
        if (mine) cnt += a.work[1 + label] + (label == 0 ? a.work[257] : 0u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __syncthreads();
    const float div = cnt ? (float)cnt : 1.0f;   // Segmentation.cpp:107, 113
    const float mean = mask_row_sum(a.full, a.depth, nchunks, lane, s_mine, [](float d) { return d; }) / div;
    const float dev = mask_row_sum(a.full, a.depth, nchunks, lane, s_mine, [mean](float d) { return fabsf(mean - d); }) / div;
    if (lane == 0) {
        const unsigned id = r < a.n_models ? a.ids[r] : a.next_id;
        unsigned spc = a.work[1 + (id & 255u)] / 256u;   // outIds / (16 * 16), :91
        if (r >= a.n_models && spc < 1u) spc = 1u;   // :96-97
        cf_seg_model md;
        md.id = id; md.superPixelCount = spc; md.avgConfidence = 0.4f; md.depthMean = mean; md.depthStd = dev;
        md.top = 0; md.right = 0; md.bottom = 0; md.left = 0;
        a.result_host->model[r] = md;
        if (r == 0) {
            a.result_host->has_new_label = has_new;
            a.result_host->n_models = rows;
            a.result_host->depth_range = 0.f;
            *a.new_host = has_new ? (int)a.mask[first] : -1;
        }
    }
}

}  // namespace cf

// ===================================================================================== C-ABI ====
static int check_mask_job(cf_ctx* ctx, const cf_seg_mask_job& j)
{
    if (!j.seg || j.seg->ctx != ctx || !j.mask_dev || !j.depth_dev || !j.model_ids || !j.mapping || !j.full_dev || j.n_models <= 0) return CF_EINVAL;
    if (j.full_dev == j.mask_dev) { ctx->set_error("cf_seg_masks: the label image cannot be the mask (every workgroup reads the first new pixel's value)"); return CF_EINVAL; }
    // model ids are 8 bits: at most 255 models and the new label's row (CF_SEG_MAX_ENTRIES rows)
    if (j.n_models > CF_SEG_MAX_ENTRIES - 1) { ctx->set_error("cf_seg_masks: more rows than CF_SEG_MAX_ENTRIES"); return CF_EINVAL; }
    if ((reinterpret_cast<size_t>(j.mask_dev) | reinterpret_cast<size_t>(j.depth_dev) | reinterpret_cast<size_t>(j.full_dev)) & 15) {
        ctx->set_error("cf_seg_masks: mask, depth and label image must be 16-byte aligned");
        return CF_EINVAL;
    }
    return CF_OK;
}

// the chain of S <= kSegBatch jobs (N = kSegBatch: up to kMaskBatchIds models each; N = 1: the full table)
template <int CAP, int N>
static int enqueue_masks(cf_ctx* ctx, const cf_seg_mask_job* jobs, int S)
{
    hipStream_t st = ctx->stream;
    const int nchunks = ctx->cfg.width * ctx->cfg.height / kMaskPx;   // (cf_create: width a multiple of 16)
    SegBatch<MaskLabelArgs> L;
    SegBatch<MaskStatsArgs<CAP>, N> T;
    memset(&L, 0, sizeof(L)); memset(&T, 0, sizeof(T));
    int rows = 0, any_new = 0;
    for (int e = 0; e < S; e++) {
        const cf_seg_mask_job& j = jobs[e];
        cf_segmenter* s = j.seg;
        unsigned* work = s->mask_work + (s->mask_jobs & 1u) * kMaskWork;
        unsigned* work_next = s->mask_work + ((s->mask_jobs + 1) & 1u) * kMaskWork;
        MaskLabelArgs& l = L.m[e];
        l.mask = j.mask_dev; l.full = j.full_dev; l.work = work; l.work_next = work_next;
        l.allow_new = j.allow_new ? 1 : 0; l.next_id = j.next_model_id;
        memcpy(l.mapping, j.mapping, 256);
        l.mapping[0] = 0;   // (mask value 0 is never looked up)
        MaskStatsArgs<CAP>& t = T.m[e];
        t.full = j.full_dev; t.depth = j.depth_dev; t.mask = j.mask_dev; t.work = work;
        t.result_host = s->h_result; t.new_host = s->h_mask_new;
        t.n_models = j.n_models; t.next_id = j.next_model_id;
        for (int m = 0; m < j.n_models; m++) { t.ids[m] = j.model_ids[m]; t.m2i[j.model_ids[m] & 255u] = (unsigned char)m; }
        t.m2i[j.next_model_id & 255u] = (unsigned char)j.n_models;   // also without a new label, as in the reference
        const int r = j.n_models + (j.allow_new ? 1 : 0);
        rows = r > rows ? r : rows;
        any_new |= l.allow_new;
    }
    const dim3 grid((nchunks + 255) / 256, S);
    if (any_new) mask_first_new_kernel<<<grid, 256, 0, st>>>(L, nchunks);
    mask_label_kernel<<<grid, 256, 0, st>>>(L, nchunks);
    mask_stats_kernel<CAP, N><<<dim3(rows, S), 64, 0, st>>>(T, nchunks);
    LAUNCHCHK(ctx);
    for (int e = 0; e < S; e++) { jobs[e].seg->mask_jobs++; jobs[e].seg->mask_pending = true; jobs[e].seg->mask_value_valid = false; }
    return CF_OK;
}

extern "C" {

// Only enqueues; rows, has_new_label and n_models arrive with cf_seg_fetch, the new mask value with cf_seg_new_mask_value after it.
int cf_seg_masks(const cf_seg_mask_job* job)
{
    if (!job || !job->seg) return CF_EINVAL;
    cf_ctx* ctx = job->seg->ctx;
    if (int r = check_mask_job(ctx, *job)) return r;
    if (job->n_models <= kMaskBatchIds) return enqueue_masks<kMaskBatchIds, kSegBatch>(ctx, job, 1);
    return enqueue_masks<CF_SEG_MAX_ENTRIES, 1>(ctx, job, 1);
}

// The jobs of several segmenters of one context (the sequences of a lock-step group) through shared launches: the three kernels are
// issued once per kSegBatch jobs.  Per segmenter the results are those of the single call, bit for bit.
int cf_seg_masks_batch(cf_ctx* ctx, const cf_seg_mask_job* jobs, int n_jobs)
{
    if (!ctx || !jobs || n_jobs <= 0) return CF_EINVAL;
    bool batchable = true;
    for (int e = 0; e < n_jobs; e++) {
        if (int r = check_mask_job(ctx, jobs[e])) return r;
        for (int k = 0; k < e; k++) if (jobs[k].seg == jobs[e].seg) return CF_EINVAL;
        batchable = batchable && jobs[e].n_models <= kMaskBatchIds;
    }
    if (!batchable) {   // (a sequence with more models than a batched launch carries ids for: one chain per job)
        for (int e = 0; e < n_jobs; e++) if (int r = cf_seg_masks(&jobs[e])) return r;
        return CF_OK;
    }
    for (int base = 0; base < n_jobs; base += kSegBatch) {
        const int S = n_jobs - base < kSegBatch ? n_jobs - base : kSegBatch;
        if (int r = enqueue_masks<kMaskBatchIds, kSegBatch>(ctx, &jobs[base], S)) return r;
    }
    return CF_OK;
}

int cf_seg_new_mask_value(cf_segmenter* s, int* value)
{
    if (!s || !value) return CF_EINVAL;
    if (!s->mask_value_valid) { s->ctx->set_error("cf_seg_new_mask_value: no mask job has been fetched (cf_seg_masks, then cf_seg_fetch)"); return CF_ESTATE; }
    *value = s->mask_new_value;
    return CF_OK;
}

}  // extern "C"
