// seg_unary_dev.h -- per-superpixel means, unaries and CRF features on the device (part of segment.hip's translation unit).
// Stage: Segmentation.cpp:160-300 and 437-450 between the sums and the mean field -- one workgroup per segmenter (seg_unary_kernel, with
// the one-wave sequential sums it keeps in the reference's order) and the grid's smoothness features.
#pragma once
#include "cf_surfel_device.h"
#include "cf_segment.h"
#include "seg_crf_dev.h"   // crf_init_node: the late half writes the mean field's first marginals

namespace cf {

// --------------------------------------------------- device-side unaries and post-processing ----
// Everything Segmentation::performSegmentationCRF does around SLIC and the mean field (Segmentation.cpp:160-300, 475-646), on the
// device: the host no longer reads the sums back to build the unaries, uploads them, reads the marginals back for the component
// analysis and uploads the label map (four host waits per multi-object frame); only the decisions come back.  Sequential f32 sums of
// the reference (average confidence, depth statistics) stay sequential -- one lane per model walks the K superpixels in index order --
// so the results are those of the host code (and of the oracle) bit for bit.
constexpr float kSegMaxDepth = 100.f;  // Segmentation::MAX_DEPTH

struct SegUnaryArgs {
    int K, gx, gy, n_models, L, allow_new;
    float unaryWeightError, unaryKError, unaryThresholdNew, scaleFeaturesRGB, scaleFeaturesDepth, scaleFeaturesPos;
    unsigned* spix_count; unsigned* depth_count;
    unsigned long long* depth_sum; unsigned long long* icp_sum; unsigned long long* conf_sum;   // [K], [n][K], [n][K]; zeroed on exit
    const int* resample;
    const uchar4* rgba;              // the CRF colour features read the first K pixels of the full-resolution image (sic, :445-447)
    float* raw;                      // scratch [(1 + 2n)][K]
    int* empties;                    // scratch [2][K] + [2]: the ordered lists of the depth-empty and the pixel-empty superpixels, their lengths
    float* Q0;                       // [K][L]: the mean field's first marginals (kUnaryTrack alone)
    float* low;                      // [(1 + 2n)][K]: lowDepth, lowICP[m], lowConf[m]
    float* unary; float* feat2;      // [K][L], [K][6]
    float* avg_conf;                 // [n]
    float* depth_range;              // [1]
};

// (the blocked sequential chain -- kSeqBlock, seq_block_phases and why skipping zero terms is exact -- lives in cf_segment.h: the mask
// branch of segment_masks.hip walks its sums with the same chain)
template <class F>
__device__ __forceinline__ float wave_sequential_sum(float init, int n, int lane, F term)
{
    float sum = init;
    for (int base = 0; base < n; base += 64 * kSeqBlock) {
        float t[kSeqBlock];
        bool any = false;
#pragma unroll
        for (int c = 0; c < kSeqBlock; c++) {
            const int j = base + lane * kSeqBlock + c;
            t[c] = j < n ? term(j) : 0.f;
            any = any || (t[c] != 0.f);
        }
        sum = seq_block_phases(sum, t, any);
    }
    return sum;
}
// What a dependent addition really costs (tools/microbench/dep_chain.hip, late in round 6): 1.70 ns -- four cycles at 2.35 GHz, the same
// with the rest of the chip busy or idle, cold or warm; v_add_f64 / v_fma_f64 1.97 ns; `s_nop 1` + v_add_f32_dpp wave_shr:1 5.1 ns; two
// interleaved chains on one wave 3.4 ns per pair (a lone wave issues one VALU instruction per four cycles whatever it depends on).  The
// "8 ns per addition" above was the whole pass divided by its terms: at K = 1 200 most of it were the two flights of sixteen strided
// 4-byte loads per lane in front of each super-block's phases and a second walk over the array to zero the non-finite entries.  This
// flavour -- n a multiple of kSeqBlock, p 16-byte aligned -- fetches a lane's block as four 16-byte loads, has the NEXT super-block's
// loads in flight during the phases of the current one, and takes the non-finite entries out on the way (zero in the sum, zero stored
// back: what the caller's second walk did).  Same additions, same order.
__device__ __forceinline__ float wave_sequential_sum_finite16(float* __restrict__ p, int n, int lane)
{
    const int nch = n / kSeqBlock;
    float sum = 0.f;
    float4 cur[4], nxt[4];
#pragma unroll
    for (int q = 0; q < 4; q++) cur[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < nch) {
#pragma unroll
        for (int q = 0; q < 4; q++) cur[q] = reinterpret_cast<const float4*>(p + (size_t)lane * kSeqBlock)[q];
    }
    for (int j0 = 0; j0 < nch; j0 += 64) {
        const int jn = j0 + 64 + lane;
#pragma unroll
        for (int q = 0; q < 4; q++) nxt[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jn < nch) {
#pragma unroll
            for (int q = 0; q < 4; q++) nxt[q] = reinterpret_cast<const float4*>(p + (size_t)jn * kSeqBlock)[q];
        }
        float t[kSeqBlock];
        bool any = false, bad = false;
#pragma unroll
        for (int q = 0; q < 4; q++) { t[q * 4] = cur[q].x; t[q * 4 + 1] = cur[q].y; t[q * 4 + 2] = cur[q].z; t[q * 4 + 3] = cur[q].w; }
#pragma unroll
        for (int c = 0; c < kSeqBlock; c++) {
            if (!is_finite(t[c])) { t[c] = 0.f; bad = true; }
            any = any || (t[c] != 0.f);
        }
        if (bad) {   // (rare)
            float4* o = reinterpret_cast<float4*>(p + (size_t)(j0 + lane) * kSeqBlock);
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = make_float4(t[q * 4], t[q * 4 + 1], t[q * 4 + 2], t[q * 4 + 3]);
        }
        sum = seq_block_phases(sum, t, any);
#pragma unroll
        for (int q = 0; q < 4; q++) cur[q] = nxt[q];
    }
    return sum;
}

// Slic::downsample<float> normalisation incl. the empty-superpixel fallback (Slic.h:63-76, 192-206) evaluated in place and in index
// order by the reference: an empty superpixel k reads entry `read`, which has ALREADY been divided when read < k and is still the
// raw sum when read > k.  Non-empty entries do not depend on anything else (phase 1, parallel); the rare empty ones are replayed in
// index order by one lane per array (phase 2) from a list built with an ordered scan.
//
// PHASES: what of this needs the frame's tracking is little -- the ICP-error rows (raw -> mean, their replay), the unaries and the first
// marginals.  kUnaryFrame (cf_seg_early, beside the tracking launches) does everything else for the depth row and the confidence rows:
// means, both lists, replay, depth range, the sequential average confidences, the appearance features; it zeroes the accumulators it
// consumed and leaves spix_count, resample and the pixel-empty list for kUnaryTrack, which runs behind the tracker on the ICP rows, forms
// the unaries from the stored depth range and the confidence rows (non-finite entries already zeroed) and writes the first marginals
// (crf_init_node: the kernel matrices were built early, so no launch carries them).  The replay rule is per array -- each replay reads
// its own array, spix_count and resample only -- so the split changes no bit.  kUnaryAll is the plain chain's kernel; one text for all.
constexpr int kUnaryFrame = 1, kUnaryTrack = 2, kUnaryAll = 3;
template <int PHASES>
__global__ void __launch_bounds__(1024) seg_unary_kernel(const SegBatch<SegUnaryArgs> B)
{
    constexpr bool kF = (PHASES & kUnaryFrame) != 0, kT = (PHASES & kUnaryTrack) != 0;
    const SegUnaryArgs a = B.m[blockIdx.x];  // (by value: the fields are loaded into scalar registers once, ahead of the phases)
    const int K = a.K, n = a.n_models, A = 1 + 2 * n, L = a.L;
    // the arrays of this flavour: row r of `rows` is array row_array(r) of [depth | icp[n] | conf[n]]
    const int rows = PHASES == kUnaryAll ? A : (kF ? 1 + n : n);
    auto row_array = [n](int r) { return PHASES == kUnaryAll ? r : (kF ? (r == 0 ? 0 : r + n) : r + 1); };
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float s_min[16], s_max[16];
    __shared__ float s_range;
    __shared__ int s_scan[16];
    __shared__ int s_nempty[2];
    int* empties = a.empties;   // [2][K] (depth-empty, pixel-empty), then the two lengths
    GSTAMP(0, 0);
    // A: raw sums as f32, phase 1 of the normalisation
    // (eight entries per lane in flight -- sixteen, one round at five models, measured slower late in round 6: 9.6 against 7.2 us --: this workgroup is alone on the GPU, a loop of dependent round trips to HBM -- 13 of them at five
    // models -- was a third of the kernel)
    for (int base = 0; base < rows * K; base += 8 * T) {
        unsigned long long sv[8]; int cv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int idx = base + u * T + tid;
            sv[u] = 0; cv[u] = 0;
            if (idx < rows * K) {
                const int r = idx / K, k = idx - r * K, arr = row_array(r);
                const unsigned long long* sums = arr == 0 ? a.depth_sum : (arr <= n ? a.icp_sum + (size_t)(arr - 1) * K : a.conf_sum + (size_t)(arr - 1 - n) * K);
                sv[u] = sums[k];
                cv[u] = (int)(arr == 0 ? a.depth_count[k] : a.spix_count[k]);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int idx = base + u * T + tid;
            if (idx < rows * K) {
                const int r = idx / K, at = row_array(r) * K + (idx - r * K);
                const float raw = (float)((double)(long long)sv[u] * 2.3283064365386963e-10 /* 2^-32 */);
                a.raw[at] = raw;
                a.low[at] = cv[u] != 0 ? raw / (float)cv[u] : raw;
            }
        }
    }
    GSTAMP(0, 1);   // raw sums -> f32, phase 1
    // ordered lists of the empty superpixels (which == 0: no depth sample, which == 1: no pixel at all): both counts ride through ONE
    // scan, sixteen bits each (K <= 4800)
    const int per = (K + T - 1) / T;
    if (kF) {
        int c0 = 0, c1 = 0;
        for (int k = tid * per; k < min(K, (tid + 1) * per); k++) { c0 += a.depth_count[k] == 0; c1 += a.spix_count[k] == 0; }
        int total = 0;
        const int incl = block_scan_inclusive(c0 | (c1 << 16), s_scan, &total);
        int pos0 = (incl & 0xffff) - c0, pos1 = (incl >> 16) - c1;
        for (int k = tid * per; k < min(K, (tid + 1) * per); k++) {
            if (a.depth_count[k] == 0) empties[pos0++] = k;
            if (a.spix_count[k] == 0) empties[K + pos1++] = k;
        }
        if (tid == 0) {
            s_nempty[0] = total & 0xffff; s_nempty[1] = total >> 16;
            if (!kT) empties[2 * K + 1] = total >> 16;   // (the pixel-empty list outlives this launch)
        }
        __syncthreads();
    } else {
        if (tid == 0) { s_nempty[0] = 0; s_nempty[1] = empties[2 * K + 1]; }
        __syncthreads();
    }
    GSTAMP(0, 2);   // ordered lists
    // phase 2: empty superpixels in index order, one lane per array
    if (tid < rows) {
        const int arr = row_array(tid);
        float* low = a.low + (size_t)arr * K;
        const float* raw = a.raw + (size_t)arr * K;
        const int which = arr == 0 ? 0 : 1, ne = s_nempty[which];
        for (int e = 0; e < ne; e++) {
            const int k = empties[which * K + e];
            const int read = a.resample[k];
            const int cnt = (int)a.spix_count[read];
            const float base = read < k ? low[read] : raw[read];
            low[k] = base / (float)cnt;
        }
    }
    __syncthreads();
    GSTAMP(0, 3);   // empty superpixels replayed
    // depth range over the valid low-resolution depths (Segmentation.cpp:165-176) BESIDE the average confidence per model (a sequential
    // f32 sum in index order, :193-203, one WAVE per model; non-finite entries count as zero and are zeroed in place): with fewer models
    // than waves, waves [0, n) take the sums and waves [n, T / 64) the range -- neither reads what the other writes
    const int nw = T >> 6;
    const bool beside = n < nw;
    auto average_confidence = [&](int m) {
        float* conf = a.low + (size_t)(1 + n + m) * K;
        float avg;
        if ((K % kSeqBlock) == 0 && (reinterpret_cast<size_t>(conf) & 15) == 0) avg = wave_sequential_sum_finite16(conf, K, lane);
        else {
            avg = wave_sequential_sum(0.f, K, lane, [&](int j) { const float c = conf[j]; return is_finite(c) ? c : 0.f; });
            for (int j = lane; j < K; j += 64) if (!is_finite(conf[j])) conf[j] = 0;
        }
        if (lane == 0) a.avg_conf[m] = avg / (float)K;
    };
    if (kF) {
        float mn = 3.402823466e+38f, mx = 0.f;
        if (beside && wave < n) average_confidence(wave);
        else {
            const int first = beside ? n * 64 : 0;
            for (int k = tid - first; k < K; k += T - first) {
                const float d = a.low[k];
                if (d > kSegMaxDepth || d < 0 || !is_finite(d)) continue;
                if (mx < d) mx = d;
                if (mn > d) mn = d;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float omn = __shfl_xor(mn, o, 64), omx = __shfl_xor(mx, o, 64);
                if (omn < mn) mn = omn;
                if (mx < omx) mx = omx;
            }
        }
        if (lane == 0) { s_min[wave] = mn; s_max[wave] = mx; }   // (the waves with the sums file the neutral elements)
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < nw; w++) { if (s_min[w] < mn) mn = s_min[w]; if (mx < s_max[w]) mx = s_max[w]; }
            s_range = mx - mn;
            a.depth_range[0] = s_range;
        }
    }
    GSTAMP(0, 4);   // depth range (+ the average confidences beside it)
    if (kF && !beside)
        for (int m = wave; m < n; m += nw) average_confidence(m);
    __syncthreads();
    GSTAMP(0, 5);   // average confidences
    const float depthRange = kF ? s_range : a.depth_range[0];
    // unaries (:237-298, 458-460) and the appearance features (:441-450), one lane per superpixel -- and per lane TWO superpixels (k and
    // k + T: K = 1200 against 1024 lanes was two rounds) with every input of both in one flight of loads: the confidences and errors of
    // eight models at a time instead of one dependent round trip per model (8.8 -> 4.5 us, late in round 6).  The stores go to elements only
    // this lane reads.
    {
        float* const icp = a.low + (size_t)K;           // [n][K]
        const float* const conf = a.low + (size_t)(1 + n) * K;
        const float fill0 = (float)((double)depthRange * 0.01), fillN = depthRange * a.unaryKError;
        const int nn = n > 0 ? n : 1;   // (model 0's rule and the first lowest error are formed whatever n is)
        for (int k0 = tid; k0 < K; k0 += 2 * T) {
            const int kk[2] = {k0, k0 + T};
            const bool ok[2] = {true, k0 + T < K};
            const int kc[2] = {k0, ok[1] ? k0 + T : k0};
            uchar4 px[2] = {}; float lowd[2] = {0.f, 0.f}, lowest[2] = {0.f, 0.f};
            if (kF) {
#pragma unroll
                for (int r = 0; r < 2; r++) { px[r] = a.rgba[kc[r]]; lowd[r] = a.low[kc[r]]; }
            }
            for (int i0 = 0; kT && i0 < nn; i0 += 8) {
                float cf[8][2], ic[8][2];
#pragma unroll
                for (int u = 0; u < 8; u++)
#pragma unroll
                    for (int r = 0; r < 2; r++) {
                        const size_t at = (size_t)min(i0 + u, nn - 1) * K + kc[r];
                        cf[u][r] = conf[at]; ic[u][r] = icp[at];
                    }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int i = i0 + u;
                    if (i < nn) {   // (uniform)
#pragma unroll
                        for (int r = 0; r < 2; r++)
                            if (ok[r]) {
                                float e = ic[u][r];
                                const bool weak = i == 0 ? (double)cf[u][r] < 0.3 : (double)cf[u][r] <= 0.4;
                                if (weak) { e = i == 0 ? fill0 : fillN; icp[(size_t)i * K + kk[r]] = e; }
                                if (i == 0) lowest[r] = e / depthRange;
                                if (i < n) {
                                    const float error = e / depthRange;
                                    if (error < lowest[r]) lowest[r] = error;
                                    float un = a.unaryWeightError * error;
                                    if (un <= 1e-5f) un = 1e-5f;
                                    a.unary[(size_t)kk[r] * L + i] = un;
                                }
                            }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 2; r++)
                if (ok[r]) {
                    const int k = kk[r];
                    if (kT && a.allow_new) {
                        float un = fmaxf(a.unaryThresholdNew - a.unaryWeightError * lowest[r], 0.01f);
                        if (un <= 1e-5f) un = 1e-5f;
                        a.unary[(size_t)k * L + n] = un;
                    }
                    if (kF) {
                        const int i = k % a.gx, j = k / a.gx;
                        float* f = a.feat2 + (size_t)k * 6;
                        f[0] = (float)i * a.scaleFeaturesPos; f[1] = (float)j * a.scaleFeaturesPos;
                        f[2] = (float)px[r].x * a.scaleFeaturesRGB; f[3] = (float)px[r].y * a.scaleFeaturesRGB; f[4] = (float)px[r].z * a.scaleFeaturesRGB;
                        f[5] = fminf(lowd[r] * a.scaleFeaturesDepth, 100.0f);
                    }
                    if (!kF) crf_init_node(a.unary, L, k, a.Q0);   // (the node's unaries are this lane's own stores)
                }
        }
    }
    __syncthreads();
    GSTAMP(0, 6);   // unaries + features
    // leave the accumulators clean for the next frame
    for (int k = tid; k < K; k += T) { if (kT) a.spix_count[k] = 0; if (kF) { a.depth_count[k] = 0; a.depth_sum[k] = 0; } }
    for (int idx = tid; idx < n * K; idx += T) { if (kT) a.icp_sum[idx] = 0; if (kF) a.conf_sum[idx] = 0; }
    GSTAMP(0, 7);
}

// smoothness features of the superpixel grid: addPairwiseGaussian(2, 2) (:437)
__global__ void seg_feat1_kernel(int gx, int K, float* __restrict__ feat1)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    feat1[k * 2 + 0] = (float)(k % gx) / 2.0f; feat1[k * 2 + 1] = (float)(k / gx) / 2.0f;
}

}  // namespace cf
