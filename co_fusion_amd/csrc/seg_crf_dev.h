// seg_crf_dev.h -- the dense-CRF mean field over the superpixel grid (part of segment.hip's translation unit).
// Stage: DenseCRF2D as used by Segmentation.cpp:436-480 -- the two Gaussian kernel matrices evaluated exactly, expAndNormalize, and the
// message / update launches of a mean-field step, with their launchers.
#pragma once
#include "cf_surfel_device.h"
#include "cf_segment.h"

namespace cf {

// ------------------------------------------------------------------------------- dense CRF ----
// The symmetric-normalised Gaussian kernel K[i][j] = norm_i * exp(-|f_i - f_j|^2 / 2) * norm_j of a feature set, stored transposed.
// All sums over the n nodes (normalisation and message passing) run in kCrfChunks contiguous chunks of ceil(n / kCrfChunks) indices:
// sequential inside a chunk, chunk totals added in chunk order (the oracle states the same order).  A thread that walks all n nodes
// alone made the 1200-node mean field 61 % of a multi-object frame (10 x 192 us + 2 x 294 us, measured); with the chunked order one
// wave covers 64 nodes x one chunk.
// Until round 4 the build was four launches (raw matrix, chunk partials, norm, scale: 5.9 + 4.7 + 4.6 + 9.6 us and three boundaries for
// 1200 nodes, re-reading the 5.8 MB raw matrix twice, once transposed).  Now two: the exponentials are cheap, so both passes recompute
// them from the features (the SAME expression: raw[i][j] and raw[j][i] agree bit for bit, (a - b)^2 == (b - a)^2) and no raw matrix exists.
constexpr int kCrfChunks = 16;
template <int D>
__device__ __forceinline__ float crf_raw(const float* fi, const float* fj)
{
    float d2 = 0;
#pragma unroll
    for (int d = 0; d < D; d++) { const float t = fi[d] - fj[d]; d2 += t * t; }
    return det_expf(-0.5f * d2);
}
// One segmenter's buffers of the mean field (a batch entry of every CRF launch)
struct CrfSeq {
    const float* feat; float* norm; float* Kt;      // kernel-matrix build: features in, normalisation scratch, matrix out
    const float* K1t; const float* K2t;             // mean field: smoothness and appearance kernels
    const float* unary; float* Q0; float* Q1; float* partial;
    int L;
};
struct CrfBatch { CrfSeq m[kSegBatch]; };
// norm_i = 1/sqrt(sum_c (sum over chunk c of raw[i][j]) + 1e-20).  A workgroup owns R nodes: its 1024 threads fill the R rows of the raw
// matrix in LDS (the exponentials, fully parallel), then one thread per (row, chunk) adds its chunk in node order and one per row the
// chunk totals in chunk order.  (One lane per (node, chunk) evaluating its 75 exponentials one after the other took 21.9 us.)
template <int D>
__global__ void __launch_bounds__(1024) crf_rownorm_kernel(const CrfBatch B, int n, int R)
{
    const float* __restrict__ feat = B.m[blockIdx.y].feat; float* __restrict__ norm = B.m[blockIdx.y].norm;
    extern __shared__ float s_raw[];  // [R][n]
    __shared__ float s_fi[8 * D];
    __shared__ float s_part[8][kCrfChunks];
    const int tid = threadIdx.x, i0 = blockIdx.x * R;
    if (tid < R * D && i0 * D + tid < n * D) s_fi[tid] = feat[i0 * D + tid];
    __syncthreads();
    for (int e = tid; e < R * n; e += 1024) {
        const int il = e / n, j = e - il * n;
        float fj[D];
#pragma unroll
        for (int d = 0; d < D; d++) fj[d] = feat[j * D + d];
        s_raw[e] = (i0 + il < n) ? crf_raw<D>(s_fi + il * D, fj) : 0.f;
    }
    __syncthreads();
    if (tid < R * kCrfChunks) {
        const int il = tid / kCrfChunks, c = tid - il * kCrfChunks;
        const int len = (n + kCrfChunks - 1) / kCrfChunks, j0 = c * len, j1 = min(n, j0 + len);
        const float* row = s_raw + il * n;
        float sum = 0;
        for (int j = j0; j < j1; j++) sum += row[j];
        s_part[il][c] = sum;
    }
    __syncthreads();
    if (tid < R && i0 + tid < n) {
        float t = 0;
        for (int k = 0; k < kCrfChunks; k++) t += s_part[tid][k];
        norm[i0 + tid] = 1.0f / sqrtf(t + 1e-20f);
    }
}
// expAndNormalize of -unary
__device__ __forceinline__ void crf_init_node(const float* __restrict__ unary, int L, int i, float* __restrict__ Q)
{
    float mx = -unary[i * L];
    for (int l = 1; l < L; l++) if (-unary[i * L + l] > mx) mx = -unary[i * L + l];
    float s = 0;
    for (int l = 0; l < L; l++) s += det_expf(-unary[i * L + l] - mx);
    for (int l = 0; l < L; l++) Q[i * L + l] = det_expf(-unary[i * L + l] - mx) / s;   // (the same expression: the same bits as the summand)
}
// Kt[j][i] = (norm_i * raw[i][j]) * norm_j.  Workgroups beyond the matrix's (g2 of them) run expAndNormalize of -unary for the mean
// field's first marginals (with_init): independent work that was a 4.7 us launch of its own.
template <int D>
__global__ void __launch_bounds__(256) crf_kernel_matrix_kernel(const CrfBatch B, int n, int g2, int with_init)
{
    const CrfSeq& m = B.m[blockIdx.y];
    if ((int)blockIdx.x >= g2) {
        const int i = ((int)blockIdx.x - g2) * 256 + threadIdx.x;
        if (with_init && i < n) crf_init_node(m.unary, m.L, i, m.Q0);
        return;
    }
    const float* __restrict__ feat = m.feat; const float* __restrict__ norm = m.norm; float* __restrict__ Kt = m.Kt;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const int j = idx / n, i = idx - j * n;
    float fi[D], fj[D];
#pragma unroll
    for (int d = 0; d < D; d++) { fi[d] = feat[i * D + d]; fj[d] = feat[j * D + d]; }
    Kt[idx] = norm[i] * crf_raw<D>(fi, fj) * norm[j];
}
// the kernel matrices of S feature sets (+ the first marginals beside them)
template <int D>
static void launch_crf_kernel_matrix(hipStream_t st, const CrfBatch& B, int S, int n, bool with_init)
{
    const int g2 = (n * n + 255) / 256, g1 = (n + 255) / 256;
    int R = (int)(48u * 1024u / (sizeof(float) * (size_t)n));  // rows of the raw matrix per workgroup: what 48 KB of LDS hold, at most 8
    R = R > 8 ? 8 : (R < 1 ? 1 : R);                          // (n <= 12288 nodes; 640x480 has 1200, 1280x960 4800)
    crf_rownorm_kernel<D><<<dim3((n + R - 1) / R, S), 1024, sizeof(float) * (size_t)R * n, st>>>(B, n, R);
    crf_kernel_matrix_kernel<D><<<dim3(g2 + (with_init ? g1 : 0), S), 256, 0, st>>>(B, n, g2, with_init ? 1 : 0);
}
// one mean-field step, part 1: chunk partials of K1*Q and K2*Q; partial[((c*n + i)*2 + which)*L + l].
// One lane per (node i, chunk c, label l) -- grid (n/64, chunks x labels, batch entries): the sums inside a chunk are sequential
// by definition, so the only parallelism is across nodes, chunks and labels, and with one lane per (node, chunk) only ~300 waves existed
// for 1024 SIMDs.  The chunk is walked 25 nodes at a time so that the kernel-matrix loads of a group are in flight together (the sums
// stay in node order).  flip: the marginals are read from Q1 (odd steps) / Q0 (even steps).
// Measured and dropped in round 5 (both bit-identical, DESIGN-NOTES R5): message + update as ONE launch -- a 1024-thread workgroup owning
// 8 nodes, wave = chunk, lane = (node, label), chunk sums through LDS: 13.8 us per step against 7.6 + 4.9 -- and four nodes per lane
// with 16-byte kernel-matrix loads: 8.2 against 7.6 us.  The step is three dependent rounds of loads behind a launch, not load issue.
// A third fusion (the workgroup's columns of both kernel matrices and all marginals staged in 106 KB of LDS with 16-byte loads, chunk sums
// out of LDS, update in place): 13.9 us per step, 768 against 781 frames/s (profiles/r5an_*).  Two launches it stays.
// Late in round 6, on top of the lean addresses below (bit-identical all): the whole 75-node chunk in one flight of loads (159 VGPRs, three
// waves per SIMD: message 7.2 + update 4.1 us against 6.65 + 4.64, the same sum) and two / three labels per lane, so that a (node block,
// chunk)'s kernel-matrix tiles leave the L2 once per two / three labels instead of once per label (839 / 811 against 843 frames/s on one
// box): the step waits neither for round trips nor for L2 bandwidth any more.
__global__ void __launch_bounds__(64) crf_message_kernel(const CrfBatch B, int n, int flip)
{
    const CrfSeq& m = B.m[blockIdx.z];
    const int L = m.L, l = blockIdx.y / kCrfChunks, c = blockIdx.y % kCrfChunks;  // grid.y = chunks x the batch's largest label count
    if (l >= L) return;
    const float* __restrict__ K1t = m.K1t; const float* __restrict__ K2t = m.K2t;
    const float* __restrict__ Q = flip ? m.Q1 : m.Q0; float* __restrict__ partial = m.partial;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int len = (n + kCrfChunks - 1) / kCrfChunks, j0 = c * len, j1 = min(n, j0 + len);
    float a = 0, b = 0;
    int j = j0;
    // the chunk is a chain of dependent additions but its loads are independent: 25 nodes' worth in flight at a time (a 75-node chunk
    // is three memory round trips instead of fifteen).
    // Addresses (late in round 6): `K1t[(j + u) * n + i]` made every load form a 64-bit address on the vector unit -- 65 v_lshl_add_u64 and
    // 93 v_add_u32 for 50 loads, ~1 300 instructions per wave and two waves per SIMD: the kernel was waiting for instruction issue as much
    // as for memory.  A uniform row pointer plus the lane's 32-bit node offset leaves one 64-bit addition per load (the uniform part is
    // formed on the scalar unit): 743 -> 488 instructions, 7.6 -> 6.5 us.
    const unsigned ib = (unsigned)i * 4u;
    auto at = [ib](const float* row) { return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row) + ib); };
    const float* r1 = K1t + (size_t)j0 * n;   // row j of the transposed kernels (uniform)
    const float* r2 = K2t + (size_t)j0 * n;
    const float* qp = Q + (size_t)j0 * L + l;  // (uniform: scalar loads)
    for (; j + 25 <= j1; j += 25, r1 += (size_t)25 * n, r2 += (size_t)25 * n, qp += (size_t)25 * L) {
        float k1[25], k2[25], q[25];
#pragma unroll
        for (int u = 0; u < 25; u++) { k1[u] = at(r1 + (size_t)u * n); k2[u] = at(r2 + (size_t)u * n); q[u] = qp[(size_t)u * L]; }
#pragma unroll
        for (int u = 0; u < 25; u++) { a += k1[u] * q[u]; b += k2[u] * q[u]; }
    }
    for (; j + 5 <= j1; j += 5, r1 += (size_t)5 * n, r2 += (size_t)5 * n, qp += (size_t)5 * L) {
        float k1[5], k2[5], q[5];
#pragma unroll
        for (int u = 0; u < 5; u++) { k1[u] = at(r1 + (size_t)u * n); k2[u] = at(r2 + (size_t)u * n); q[u] = qp[(size_t)u * L]; }
#pragma unroll
        for (int u = 0; u < 5; u++) { a += k1[u] * q[u]; b += k2[u] * q[u]; }
    }
    for (; j < j1; j++, r1 += n, r2 += n, qp += L) {
        const float q = qp[0];
        a += at(r1) * q;
        b += at(r2) * q;
    }
    float* out = partial + ((size_t)(c * n + i) * 2) * L;
    out[l] = a; out[L + l] = b;
}
// part 2: chunk totals in chunk order, unary, softmax over the labels.  Thread (node g, label l): 256 / LS nodes x LS label slots per
// workgroup (LS = 16 for up to 16 labels, a power of two up to 256 beyond); the chunk partials of a (node, label) are loaded
// independently and summed in chunk order, the softmax runs over the node's LDS row exactly like expAndNormalize.
template <int LS>
__global__ void __launch_bounds__(256) crf_update_kernel(const CrfBatch B, int n, float w_smooth, float w_app, int flip)
{
    const CrfSeq& m = B.m[blockIdx.y];
    const int L = m.L;
    const float* __restrict__ unary = m.unary; const float* __restrict__ partial = m.partial; float* __restrict__ Qn = flip ? m.Q0 : m.Q1;
    constexpr int G = 256 / LS;
    __shared__ float s_t[G][LS];
    const int g = threadIdx.x / LS, l = threadIdx.x % LS;
    const int i = blockIdx.x * G + g;
    float tmp = 0;
    if (i < n && l < L) {
        float pa[kCrfChunks], pb[kCrfChunks];
#pragma unroll
        for (int c = 0; c < kCrfChunks; c++) {
            const float* in = partial + ((size_t)(c * n + i) * 2) * L;
            pa[c] = in[l]; pb[c] = in[L + l];
        }
        float a = 0, b = 0;
#pragma unroll
        for (int c = 0; c < kCrfChunks; c++) { a += pa[c]; b += pb[c]; }
        tmp = (-unary[i * L + l] - (-w_smooth * a)) - (-w_app * b);
        s_t[g][l] = tmp;
    }
    __syncthreads();
    if (i < n && l < L) {
        float mx = s_t[g][0];
        for (int k = 1; k < L; k++) if (s_t[g][k] > mx) mx = s_t[g][k];
        float sum = 0;
        for (int k = 0; k < L; k++) sum += det_expf(s_t[g][k] - mx);
        Qn[i * L + l] = det_expf(tmp - mx) / sum;
    }
}
// `iterations` mean-field steps of S batch entries from Q0; returns 1 when the last marginals are in Q1
static int launch_mean_field(hipStream_t st, CrfBatch& B, int S, int n, int iterations, float w_smooth, float w_app)
{
    int Lmax = 0;
    for (int e = 0; e < S; e++) Lmax = B.m[e].L > Lmax ? B.m[e].L : Lmax;
    const dim3 gm((n + 63) / 64, kCrfChunks * Lmax, S);
    int flip = 0;
    for (int it = 0; it < iterations; it++) {
        crf_message_kernel<<<gm, 64, 0, st>>>(B, n, flip);
        if (Lmax <= 16) crf_update_kernel<16><<<dim3((n + 15) / 16, S), 256, 0, st>>>(B, n, w_smooth, w_app, flip);
        else if (Lmax <= 32) crf_update_kernel<32><<<dim3((n + 7) / 8, S), 256, 0, st>>>(B, n, w_smooth, w_app, flip);
        else if (Lmax <= 64) crf_update_kernel<64><<<dim3((n + 3) / 4, S), 256, 0, st>>>(B, n, w_smooth, w_app, flip);
        else if (Lmax <= 128) crf_update_kernel<128><<<dim3((n + 1) / 2, S), 256, 0, st>>>(B, n, w_smooth, w_app, flip);
        else crf_update_kernel<256><<<dim3(n, S), 256, 0, st>>>(B, n, w_smooth, w_app, flip);
        flip ^= 1;
    }
    return flip;
}

}  // namespace cf
