// seg_post_dev.h -- from the marginals to the frame's decisions (part of segment.hip's translation unit).
// Stage: Segmentation.cpp:475-646 in one workgroup per segmenter (seg_post_kernel: arg-max, connected components, gates, boxes, depth
// statistics, published into pinned memory) with the LDS-blocked sums it walks, and the pose words a model-parallel caller sends along.
#pragma once
#include "cf_surfel_device.h"
#include "cf_segment.h"
#include "seg_slic_dev.h"   // kSpix: Slic::mapToHigh

namespace cf {

// seg_post_kernel's sums: the terms are predicates over arrays in LDS.  Rounds 5-6 moved them to the adder one by one with a lane shift
// (`s_nop 1` + `v_add_f32_dpp wave_shr:1`: 5.1 ns per term by the micro-benchmark, 63 per 64 terms), because the blocked chain read its
// sixteen terms per lane with a lane stride of sixteen words -- bank conflicts in three arrays, 25.1 against 21.8 us.  Now the arrays are
// LAID OUT for the blocked chain: the depths padded by four words per sixteen (entry k at k + 4 * (k >> 4): lane l's block starts at
// word 20 l, four conflict-free 16-byte reads), the model entry of every superpixel as 16 bits (lane l's sixteen are 32 consecutive bytes).
// `term(mine, depth, out[NCH])` forms the NCH chains' terms of one superpixel; a lane whose block holds only zeros has no phase.
constexpr int kSegDepthPad(int k) { return k + 4 * (k >> 4); }
template <int NCH, class F>
__device__ __forceinline__ void lds_blocked_sums(float (&sum)[NCH], int nch, int lane, const float* s_depth, const unsigned short* s_entry, unsigned entry, F term)
{
    for (int j0 = 0; j0 < nch; j0 += 64) {
        const int j = j0 + lane;
        float t[NCH][kSeqBlock];
        bool any = false;
#pragma unroll
        for (int h = 0; h < NCH; h++)
#pragma unroll
            for (int c = 0; c < kSeqBlock; c++) t[h][c] = 0.f;
        if (j < nch) {
            const float4* dq = reinterpret_cast<const float4*>(s_depth + 20 * j);
            const uint4* eq = reinterpret_cast<const uint4*>(s_entry + 16 * j);
            const float4 d0 = dq[0], d1 = dq[1], d2 = dq[2], d3 = dq[3];
            const uint4 e0 = eq[0], e1 = eq[1];
            const float d[kSeqBlock] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w, d2.x, d2.y, d2.z, d2.w, d3.x, d3.y, d3.z, d3.w};
            const unsigned w[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
            for (int c = 0; c < kSeqBlock; c++) {
                const bool mine = ((w[c >> 1] >> ((c & 1) * 16)) & 0xffffu) == entry;
                float v[NCH];
                term(mine, d[c], v);
#pragma unroll
                for (int h = 0; h < NCH; h++) { t[h][c] = v[h]; any = any || (v[h] != 0.f); }
            }
        }
        unsigned long long nz = __ballot(any);
        while (nz) {   // (uniform)
            const int ph = __builtin_ctzll(nz);
            nz &= nz - 1;
            float x[NCH];
#pragma unroll
            for (int h = 0; h < NCH; h++) x[h] = sum[h];
#pragma unroll
            for (int c = 0; c < kSeqBlock; c++)
#pragma unroll
                for (int h = 0; h < NCH; h++) x[h] = x[h] + t[h][c];
#pragma unroll
            for (int h = 0; h < NCH; h++) sum[h] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[h]), ph));
        }
    }
}

template <int CAP>
struct SegPostArgsT {
    int K, gx, gy, n_models, L, allow_new, width, height;
    unsigned next_id;
    float minRelSizeNew, maxRelSizeNew;
    unsigned ids[CAP];               // model ids in list order (+ the new label's id)
    const float* Q;                  // [K][L] marginals
    const float* low_depth;          // [K]
    const float* avg_conf;           // [n]
    const float* depth_range;
    int* cc;                         // scratch [6][K]: label, size, top, right, bottom, left per component
    unsigned char* low_map;          // [K] out
    cf_seg_result* result;           // device copy of the result
    cf_seg_result* result_host;      // pinned: the kernel publishes the decisions itself (no copy command behind it on the stream)
    unsigned* low_map_host;          // pinned, [ceil(K / 4)] words
};

// arg-max labels -> connected components (ConnectedLabels.hpp:50-172: 4-connectivity, components numbered by their first pixel in
// raster order) -> largest-component / size / border gates -> bounding boxes, depth statistics, super-pixel counts (:475-646).
// One workgroup: the label image has K = 1200 superpixels (4800 at 1280x960, the largest supported); labels, union-find parents and
// component numbers live in LDS, the sequential sums of the statistics run one wave per model (wave_sequential_sum).
constexpr int kPoseWords = 18;   // cf_seg_publish_poses: 16 pose words + ICP error + ICP inlier count, one 64-bit slot per f32 bit pattern
constexpr int kCcLds = 256;   // components whose statistics fit in LDS (a frame has tens)
template <int CAP, int N>
__global__ void __launch_bounds__(1024) seg_post_kernel(const SegBatch<SegPostArgsT<CAP>, N> B)
{
    const SegPostArgsT<CAP>& a = B.m[blockIdx.x];
    const int K = a.K, gx = a.gx, L = a.L, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int n_md = a.n_models + (a.allow_new ? 1 : 0);
    __shared__ int s_changed, s_min_label;
    __shared__ int s_scan[16];
    __shared__ int s_id2idx[256];
    __shared__ int s_box[kMaxL + 1][4];   // top, right, bottom, left per model entry (full-resolution pixels after mapToHigh)
    __shared__ unsigned s_spc[kMaxL + 1];
    __shared__ unsigned s_best[256];
    __shared__ int s_reject[kMaxL + 1];
    __shared__ __attribute__((aligned(4))) unsigned char map[kSegMaxK];
    __shared__ __attribute__((aligned(16))) int s_pc[2 * kSegMaxK];   // union-find parents | component numbers; later the statistics' arrays
    int* const parent = s_pc;
    int* const comp = s_pc + kSegMaxK;
    __shared__ int s_cc[6 * kCcLds];
    if (tid == 0) s_min_label = 256;
    GSTAMP(1, 0);
    // 1. label with the highest marginal (first maximum), as model id
    // (two superpixels per lane with eight marginals of each in one flight of loads instead of two rounds: 3.0 us of this phase either
    // way, late in round 6; the three sweeps of the component loop below are the other 8.7 us)
    for (int k = tid; k < K; k += T) {
        int m = 0; float best = a.Q[(size_t)k * L];
        for (int l = 1; l < L; l++) { const float q = a.Q[(size_t)k * L + l]; if (q > best) { best = q; m = l; } }
        map[k] = (unsigned char)a.ids[m];
        parent[k] = k;
    }
    if (tid < 256) s_id2idx[tid] = 0;
    __syncthreads();
    if (tid < a.n_models) s_id2idx[a.ids[tid] & 255] = tid;
    __syncthreads();
    if (tid == 0 && a.allow_new) s_id2idx[a.next_id & 255] = a.n_models;
    GSTAMP(1, 8);   // (arg-max alone)
    // 2. connected components: min-label propagation over the 4-neighbourhood + pointer jumping until nothing changes; the root of a
    //    component is its smallest index = its first pixel in raster order
#ifdef CF_ABLATE
    int cc_sweep = 0;
#endif
    for (;;) {
        __syncthreads();
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int k = tid; k < K; k += T) {
            const int x = k % gx, y = k / gx;
            const unsigned char v = map[k];
            const int own = parent[k];
            int p = own;
            if (x > 0 && map[k - 1] == v) p = min(p, parent[k - 1]);
            if (x + 1 < gx && map[k + 1] == v) p = min(p, parent[k + 1]);
            if (y > 0 && map[k - gx] == v) p = min(p, parent[k - gx]);
            if (y + 1 < a.gy && map[k + gx] == v) p = min(p, parent[k + gx]);
            if (p < own) { atomicMin(&parent[own], p); atomicMin(&parent[k], p); s_changed = 1; }
        }
        __syncthreads();
#ifdef CF_ABLATE
        if (tid == 0 && blockIdx.x == 0 && cc_sweep < 3) g_seg_trace[1][10 + 2 * cc_sweep] = wall_clock64();   // (hooks of this sweep done)
#endif
        if (!s_changed) break;   // (nothing hooked: every entry is still the root the last sweep's walk left -- or itself, in the first sweep)
        // walks to the roots.  After the first sweep's hooks a superpixel's chain runs up its column and along a row -- up to 70 hops of one
        // dependent LDS read each, 4.5 of this loop's 8.7 us (per-sweep stamps, late in round 6).  Every step of a walk is now WRITTEN to the
        // walker's own entry: the walkers that pass through it later jump where it has got to, so the lanes double each other's strides
        // (pointer jumping without its barriers).  Racy and monotone: during this pass nothing hooks, an entry only ever moves to an ancestor,
        // and a walk ends at an entry that is its own parent -- the same roots.
        for (int k = tid; k < K; k += T) {
            int p = parent[k];
            for (;;) {
                const int q = parent[p];
                if (q == p) break;
                parent[k] = q;
                p = q;
            }
            parent[k] = p;
        }
#ifdef CF_ABLATE
        __syncthreads();
        if (tid == 0 && blockIdx.x == 0) { g_seg_trace[1][9]++; if (cc_sweep < 3) g_seg_trace[1][11 + 2 * cc_sweep] = wall_clock64(); }   // (sweeps of the component loop; walks done)
        cc_sweep++;
#endif
    }   // (the barrier at the top of the next sweep stands between this sweep's walks and its hooks)
    GSTAMP(1, 1);   // arg-max + connected components
    // 3. number the roots in index order (exclusive scan of the root flags); a root also files its label under its number
    const int per = (K + T - 1) / T;
    int cnt3 = 0;
    for (int k = tid * per; k < min(K, (tid + 1) * per); k++) cnt3 += parent[k] == k;
    int ncc = 0;
    const int scan3 = block_scan_inclusive(cnt3, s_scan, &ncc);
    // per-component label, size, top, right, bottom, left: in LDS unless the label image is unusually fragmented
    int* const ccb = ncc <= kCcLds ? s_cc : a.cc;
    const int ccs = ncc <= kCcLds ? kCcLds : K;
    int *c_label = ccb, *c_size = ccb + ccs, *c_top = ccb + 2 * ccs, *c_right = ccb + 3 * ccs, *c_bottom = ccb + 4 * ccs, *c_left = ccb + 5 * ccs;
    {
        int base = scan3 - cnt3;
        for (int k = tid * per; k < min(K, (tid + 1) * per); k++)
            if (parent[k] == k) { comp[k] = base; c_label[base] = map[k]; atomicMin(&s_min_label, (int)map[k]); base++; }
    }
    for (int i = tid; i < ncc; i += T) { c_size[i] = 0; c_top[i] = 2147483647; c_right[i] = 0; c_bottom[i] = 0; c_left[i] = 2147483647; }
    __syncthreads();
    for (int k = tid; k < K; k += T) if (parent[k] != k) comp[k] = comp[parent[k]];  // roots wrote their own entry; read-only for them
    __syncthreads();
    GSTAMP(1, 2);   // roots numbered
    // 4. component statistics.  A wave first combines the lanes that belong to the same component (usually one or two per wave), so
    //    that one lane per (wave, component) touches the shared counters: a thousand atomics on the background's five words otherwise
    //    queue up behind each other
    for (int kb = 0; kb < K; kb += T) {
        const int k = kb + tid;
        const bool in = k < K;
        const int c = in ? comp[k] : -1, x = in ? k % gx : 0, y = in ? k / gx : 0;
        unsigned long long todo = __ballot(in);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int c0 = __builtin_amdgcn_readlane(c, leader);
            const bool member = in && c == c0;
            const unsigned long long grp = __ballot(member);
            int ymin = member ? y : 2147483647, ymax = member ? y : 0, xmin = member ? x : 2147483647, xmax = member ? x : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                ymin = min(ymin, __shfl_xor(ymin, o, 64)); ymax = max(ymax, __shfl_xor(ymax, o, 64));
                xmin = min(xmin, __shfl_xor(xmin, o, 64)); xmax = max(xmax, __shfl_xor(xmax, o, 64));
            }
            if (lane == leader) {
                atomicAdd(&c_size[c0], (int)__popcll(grp));
                atomicMin(&c_top[c0], ymin); atomicMax(&c_bottom[c0], ymax); atomicMin(&c_left[c0], xmin); atomicMax(&c_right[c0], xmax);
            }
            todo &= ~grp;
        }
    }
    __threadfence_block();
    __syncthreads();
    GSTAMP(1, 3);   // component statistics
    // 5. onlyKeepLargest (:496-517): every label but the smallest keeps its largest component, the earlier one on ties -- the
    //    sequential rule "replace the kept component only by a strictly larger one" picks exactly the maximum of (size, -index)
    if (tid < 256) s_best[tid] = 0;
    if (tid < kMaxL + 1) { s_box[tid][0] = 65535; s_box[tid][1] = 0; s_box[tid][2] = 0; s_box[tid][3] = 65535; s_reject[tid] = 0; }
    __syncthreads();
    const int minLabel = s_min_label;
    for (int i = tid; i < ncc; i += T) {
        const int lab = c_label[i];
        if (lab != minLabel && lab != 255) atomicMax(&s_best[lab], ((unsigned)c_size[i] << 16) | (unsigned)(65535 - i));
    }
    __syncthreads();
    // 6. ... and a new label must have a plausible size (:521-530)
    {
        const int minSize = (int)((float)K * a.minRelSizeNew), maxSize = (int)((float)K * a.maxRelSizeNew);
        for (int i = tid; i < ncc; i += T) {
            int lab = c_label[i];
            if (lab != minLabel && lab != 255 && (int)(65535u - (s_best[lab] & 0xffffu)) != i) lab = 255;
            if (a.allow_new && lab == (int)a.next_id && (c_size[i] < minSize || c_size[i] > maxSize)) lab = 255;
            c_label[i] = lab;
            // 7. bounding boxes over the surviving components of every model entry (:532-547)
            if (lab != 255) {
                const int e = s_id2idx[lab];
                if ((int)(a.ids[e] & 255u) == lab) {
                    atomicMin(&s_box[e][0], c_top[i]); atomicMax(&s_box[e][1], c_right[i]); atomicMax(&s_box[e][2], c_bottom[i]); atomicMin(&s_box[e][3], c_left[i]);
                }
            }
        }
    }
    __syncthreads();
    // Slic::mapToHigh, then 8. labels whose box lies inside the border strip are rejected (:549-563)
    if (tid < n_md) {
        const int top = (int)(unsigned short)(int)(s_box[tid][0] * kSpix + kSpix * 0.5), right = (int)(unsigned short)(int)(s_box[tid][1] * kSpix + kSpix * 0.5);
        const int bottom = (int)(unsigned short)(int)(s_box[tid][2] * kSpix + kSpix * 0.5), left = (int)(unsigned short)(int)(s_box[tid][3] * kSpix + kSpix * 0.5);
        s_box[tid][0] = top; s_box[tid][1] = right; s_box[tid][2] = bottom; s_box[tid][3] = left;
        if (a.ids[tid] != 0) {
            const unsigned borderSize = 20, fullHeight = (unsigned)a.height, fullWidth = (unsigned)a.width;
            const unsigned t = (unsigned)top, r = (unsigned)right, bo = (unsigned)bottom, l = (unsigned)left;
            if ((t < borderSize && bo < borderSize) || (l < borderSize && r < borderSize) ||
                (t > fullHeight - borderSize && bo > fullHeight - borderSize) || (l > fullWidth - borderSize && r > fullWidth - borderSize))
                s_reject[tid] = 1;
        }
    }
    __syncthreads();
    for (int i = tid; i < ncc; i += T) {
        const int lab = c_label[i];
        if (lab == 255) continue;
        const int e = s_id2idx[lab];
        if ((int)(a.ids[e] & 255u) == lab && s_reject[e]) c_label[i] = 255;
    }
    __threadfence_block();
    __syncthreads();
    GSTAMP(1, 4);   // gates
    // 9. final low-resolution label map
    for (int k = tid; k < K; k += T) { const unsigned char v = (unsigned char)c_label[comp[k]]; map[k] = v; a.low_map[k] = v; }
    __syncthreads();
    // (parents and component numbers are dead: their storage holds the low-resolution depths and every superpixel's model entry in the
    // layout of lds_blocked_sums; the tail up to a multiple of sixteen belongs to nobody)
    float* const s_depth = reinterpret_cast<float*>(s_pc);
    unsigned short* const s_entry = reinterpret_cast<unsigned short*>(s_pc + kSegDepthPad(kSegMaxK));
    const int nch = (K + kSeqBlock - 1) / kSeqBlock;
    for (int k = tid; k < nch * kSeqBlock; k += T) {
        const unsigned char v = k < K ? map[k] : (unsigned char)255;
        s_entry[k] = v == 255 ? (unsigned short)0xffff : (unsigned short)s_id2idx[v];
        s_depth[kSegDepthPad(k)] = k < K ? a.low_depth[k] : 0.f;
    }
    __syncthreads();
    GSTAMP(1, 5);   // label map
    // 10. depth statistics with one trimming pass (:570-621) and super-pixel counts (:624-627): sequential f32 sums in index order,
    //     one wave per model entry
    for (int ix = wave; ix < n_md; ix += (T >> 6)) {
        auto mine_at = [&](int i) { return s_entry[i] == (unsigned short)ix; };
        unsigned cnt = 0;
        for (int i = lane; i < K; i += 64) cnt += mine_at(i) ? 1u : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        const unsigned spc = cnt;
        float s1[1] = {0.f};
        lds_blocked_sums<1>(s1, nch, lane, s_depth, s_entry, (unsigned)ix, [&](bool mine, float d, float (&v)[1]) { v[0] = mine ? d : 0.f; });
        float sumDepth = s1[0];
        float mean = cnt ? sumDepth / (float)cnt : 0;
        s1[0] = 0.f;
        lds_blocked_sums<1>(s1, nch, lane, s_depth, s_entry, (unsigned)ix, [&](bool mine, float d, float (&v)[1]) { v[0] = mine ? fabsf(mean - d) : 0.f; });
        float sumDev = s1[0];
        float dev = cnt ? sumDev / (float)cnt : 0;
        if (ix != 0) {
            // trimming pass: elements beyond mean + 1.1 dev are taken out of the running sums, in index order (x - d == x + (-d))
            const double limit = 1.1 * (double)dev + (double)mean;
            unsigned out = 0;
            for (int i = lane; i < K; i += 64) out += (mine_at(i) && (double)s_depth[kSegDepthPad(i)] > limit) ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) out += __shfl_xor(out, o, 64);
            if (out) {
                float s2[2] = {sumDepth, sumDev};
                lds_blocked_sums<2>(s2, nch, lane, s_depth, s_entry, (unsigned)ix, [&](bool mine, float d, float (&v)[2]) {
                    const bool trimmed = mine && (double)d > limit;
                    v[0] = trimmed ? -d : 0.f; v[1] = trimmed ? -fabsf(mean - d) : 0.f;
                });
                sumDepth = s2[0]; sumDev = s2[1];
            }
            cnt -= out;
        }
        mean = cnt ? sumDepth / (float)cnt : 0;
        dev = cnt ? sumDev / (float)cnt : 0;
        if (lane == 0) {
            cf_seg_model& o = a.result->model[ix];
            o.id = a.ids[ix]; o.superPixelCount = spc; o.avgConfidence = ix < a.n_models ? a.avg_conf[ix] : 0.f;
            o.depthMean = mean; o.depthStd = dev;
            o.top = s_box[ix][0]; o.right = s_box[ix][1]; o.bottom = s_box[ix][2]; o.left = s_box[ix][3];
            s_spc[ix] = spc;
        }
    }
    __syncthreads();
    GSTAMP(1, 6);   // depth statistics
    if (tid == 0) {
        int has_new = 0, n_out = n_md;
        if (a.allow_new) { if (s_spc[n_md - 1] > 0) has_new = 1; else n_out = n_md - 1; }
        a.result->has_new_label = has_new; a.result->n_models = n_out; a.result->depth_range = a.depth_range[0];
    }
    // publish: decisions and the low-resolution map into pinned host memory (what the frame's one host wait collects)
    __threadfence_block();
    __syncthreads();
    if (a.result_host) {
        const unsigned* src = reinterpret_cast<const unsigned*>(a.result);
        unsigned* dst = reinterpret_cast<unsigned*>(a.result_host);
        const int words = (int)((offsetof(cf_seg_result, model) + sizeof(cf_seg_model) * (size_t)n_md) / 4);   // header + the rows in use
        for (int k = tid; k < words; k += T) dst[k] = src[k];
    }
    if (a.low_map_host)
        for (int k = tid; k < (K + 3) / 4; k += T) a.low_map_host[k] = reinterpret_cast<const unsigned*>(map)[k];
    GSTAMP(1, 7);
}

}  // namespace cf

// cf_seg_publish_poses: model m's tracked pose (T = [Rcurr | tcurr], row-major 4x4) and ICP statistics as f32 bit patterns, one 64-bit
// slot each, behind the segmentation sums -- zeros for models this process does not own, so that the caller's SUM all-reduce of the
// block leaves every model's pose on every rank (exact: one contributor per word).  (Outside cf: the symbol keeps its name.)
struct PosePublishArgs { const cf::OdomDev* st[cf::kMaxL]; int n; };
__global__ void __launch_bounds__(64) pose_publish_kernel(const PosePublishArgs a, long long* __restrict__ tail)
{
    const int m = blockIdx.x, w = threadIdx.x;
    if (w >= cf::kPoseWords) return;
    long long v = 0;
    const cf::OdomDev* st = m < a.n ? a.st[m] : nullptr;
    if (st) {
        float f;
        if (w < 12) { const int r = w >> 2, c = w & 3; f = c < 3 ? st->Rcurr[r * 3 + c] : st->tcurr[r]; }
        else if (w < 16) f = w == 15 ? 1.f : 0.f;
        else f = w == 16 ? st->stats.last_icp_error : st->stats.last_icp_count;
        v = (long long)__float_as_uint(f);
    }
    tail[m * cf::kPoseWords + w] = v;
}
