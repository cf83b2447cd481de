// track_so3_dev.h -- the SO(3) pre-alignment of the dense tracking (part of track_reduce.hip's translation unit, included behind the
// residual pass: it runs the preparation bodies of track_prep_dev.h in the same launch).  Also screen_box, which this launch and the solve call.
// Stage: the rotation-only photometric alignment at level 2 that seeds the Gauss-Newton loop, one launch per frame.  Replaces
// SO3Reduction / so3Step of Core/Cuda/reduce.cu (:1007-1175) and the host loop RGBDOdometry.cpp:239-310.
#pragma once
#include "track_prep_dev.h"
#include "track_sums_dev.h"

namespace cf {

// ------------------------------------------------------------------------------------------------
// Screen-box culling.  A pixel of the current frame finds a correspondence only if its vertex, taken into the camera the prediction was
// rendered from (vcurr_cp = Rprev^-1 (Rcurr vcurr + tcurr - tprev)), projects onto a VALID pixel of the prediction -- i.e. lies inside
// that pixel's pyramid -- and is within distThres of the model vertex there (reduce.cu:321-325), hence at a depth within distThres of it.
// All such vertices lie in one frustum piece of the prediction camera: the pixel rectangle of the valid predicted vertices (lo / hi [0..1],
// level-0 pixels; model_maps_tiled_body) between the depths lo[2] - distThres and hi[2] + distThres.  Its eight corners, taken into the
// current camera and projected, bound the pixels that can contribute (a projective map takes the convex piece into the convex hull of
// the corners' images): everything outside adds exact zeros and is skipped before it loads anything.
// Conservative: the rectangle is widened by 3 pixels (a level-l pixel of the model maps is valid only if its 2^l x 2^l level-0 sources
// are, and its pyramid overhangs them by 2^(l-1) level-0 pixels; + rounding of the per-pixel f32 projection), the depths by 1 % + 1 mm on
// top of distThres, the projected rectangle by 3 pixels, and a near plane that is not clearly in front of either camera (or anything
// not finite) gives the whole image.  Called by a whole wave; the result is valid in every lane.
// Rb / tb: pose of the prediction camera (OdomDev::box_R / box_t).
__device__ __forceinline__ void screen_box(const float* lo, const float* hi, const float* Rb, const float* tb, const float* Rcurr, const float* tcurr,
                                           cf_cam intr, float distThres, int W, int H, int lane, int (&out)[4], float (&zout)[2])
{
    const float finf = __int_as_float(0x7f800000);
    zout[0] = -finf; zout[1] = finf;
    if (!(lo[0] <= hi[0])) { out[0] = 1; out[1] = 1; out[2] = 0; out[3] = 0; return; }  // no predicted vertex: nothing can match
    const float m = distThres * 1.01f + 1e-3f;
    const float px = (lane & 1) ? hi[0] + 3.f : lo[0] - 3.f, py = (lane & 2) ? hi[1] + 3.f : lo[1] - 3.f;
    const float znear = lo[2] - m, pz = (lane & 4) ? hi[2] + m : znear;
    const float cx_ = (px - intr.cx) / intr.fx * pz, cy_ = (py - intr.cy) / intr.fy * pz;
    // into the global frame, then into the current camera: Rcurr^T (Rcurr is a rotation up to f32 rounding)
    const float dx = (Rb[0] * cx_ + Rb[1] * cy_ + Rb[2] * pz + tb[0]) - tcurr[0];
    const float dy = (Rb[3] * cx_ + Rb[4] * cy_ + Rb[5] * pz + tb[1]) - tcurr[1];
    const float dz = (Rb[6] * cx_ + Rb[7] * cy_ + Rb[8] * pz + tb[2]) - tcurr[2];
    const float xc = Rcurr[0] * dx + Rcurr[3] * dy + Rcurr[6] * dz;
    const float yc = Rcurr[1] * dx + Rcurr[4] * dy + Rcurr[7] * dz;
    const float zc = Rcurr[2] * dx + Rcurr[5] * dy + Rcurr[8] * dz;
    const float u = intr.fx * xc / zc + intr.cx, v = intr.fy * yc / zc + intr.cy;
    const bool bad = !(znear > 0.05f) || !(zc > 0.05f) || !is_finite(u) || !is_finite(v);
    float u0 = u, u1 = u, v0 = v, v1 = v, z0 = zc, z1 = zc;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        u0 = fminf(u0, __shfl_xor(u0, o, 64)); u1 = fmaxf(u1, __shfl_xor(u1, o, 64));
        v0 = fminf(v0, __shfl_xor(v0, o, 64)); v1 = fmaxf(v1, __shfl_xor(v1, o, 64));
        z0 = fminf(z0, __shfl_xor(z0, o, 64)); z1 = fmaxf(z1, __shfl_xor(z1, o, 64));
    }
    if (__any(bad)) { out[0] = 0; out[1] = 0; out[2] = W - 1; out[3] = H - 1; return; }
    // the depth (z in the current camera) of a matching vertex lies between the extreme corners: a linear map of a box
    zout[0] = z0 - (1e-3f + 1e-3f * fabsf(z0)); zout[1] = z1 + (1e-3f + 1e-3f * fabsf(z1));
    const float fw = (float)(W + 16), fh = (float)(H + 16);
    out[0] = (int)floorf(fminf(fmaxf(u0, -16.f), fw)) - 3; out[1] = (int)floorf(fminf(fmaxf(v0, -16.f), fh)) - 3;
    out[2] = (int)ceilf(fminf(fmaxf(u1, -16.f), fw)) + 3; out[3] = (int)ceilf(fminf(fmaxf(v1, -16.f), fh)) + 3;
}

// ================================================================================================
// SO3: SO3Reduction::getProducts, reduce.cu:1007-1090
// ================================================================================================
__device__ __forceinline__ void so3_gradient(const uint8_t* __restrict__ img, int cols, int x, int y, float& gx, float& gy)
{  // reduce.cu:989-1005
    const float actu = (float)img[y * cols + x];
    float back = (float)img[y * cols + x - 1], fore = (float)img[y * cols + x + 1];
    gx = ((back + actu) / 2.0f) - ((fore + actu) / 2.0f);
    back = (float)img[(y - 1) * cols + x]; fore = (float)img[(y + 1) * cols + x];
    gy = ((back + actu) / 2.0f) - ((fore + actu) / 2.0f);
}

// one (grid-strided over blockIdx.x) pass over the level-2 images; this workgroup's totals[0..10] end up in LDS
__device__ __forceinline__ void so3_pass(const uint8_t* __restrict__ lastImage, const uint8_t* __restrict__ nextImage,
                                         const m33& B, const m33& Ki, const float* __restrict__ krlr, int cols, int rows,
                                         unsigned long long (*lds)[16], unsigned long long* totals, int block, int blocks)
{
    constexpr float lim = (float)(1 << ((50 - kFixSO3) / 2));
    constexpr float scale = (float)(1 << kFixSO3);
    const int N = cols * rows, T = blockDim.x;
    unsigned long long acc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = 0;
    const float a = krlr[0], b = krlr[1], c = krlr[2], d = krlr[3], e = krlr[4], f = krlr[5], g = krlr[6], h = krlr[7],
                ii = krlr[8];
    // (Measured and dropped, round 6: four pixels of a thread at a time -- their warps first, the 4 x 10 byte loads of the gradient stencils in
    // flight together, then the rows: so3_prealign_kernel 82.0 against 63.1 us on one box, profiles/r6u_*.  The registers of four stencils
    // cost the launch's other half, the RGB preparation workgroups, their occupancy; the pass itself is 4-7 us of a 9 us iteration.)
    for (int k = block * T + threadIdx.x; k < N; k += blocks * T) {
        const int y = k / cols, x = k - y * cols;
        const f3 unwarped = {(float)x, (float)y, 1.0f};
        const f3 warped = mul(B, unwarped);
        const int wx = f2i_rn(warped.x / warped.z), wy = f2i_rn(warped.y / warped.z);
        if (!(wx >= 1 && wx < cols - 1 && wy >= 1 && wy < rows - 1 && x >= 1 && x < cols - 1 && y >= 1 && y < rows - 1))
            continue;
        float gnx, gny, glx, gly;
        so3_gradient(nextImage, cols, wx, wy, gnx, gny);
        so3_gradient(lastImage, cols, x, y, glx, gly);
        const float gx = (gnx + glx) / 2.0f, gy = (gny + gly) / 2.0f;
        const f3 point = mul(Ki, unwarped);
        const float z2 = point.z * point.z;
        const f3 left = {((point.z * (d * gy + a * gx)) - (gy * g * y) - (gx * g * x)) / z2,
                         ((point.z * (e * gy + b * gx)) - (gy * h * y) - (gx * h * x)) / z2,
                         ((point.z * (f * gy + c * gx)) - (gy * ii * y) - (gx * ii * x)) / z2};
        const f3 jac = cross(left, point);
        const float row[4] = {jac.x, jac.y, jac.z, -((float)nextImage[wy * cols + wx] - (float)lastImage[y * cols + x])};
        double r[4], rs[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { r[q] = (double)clamp_row(row[q], lim); rs[q] = (double)(clamp_row(row[q], lim) * scale); }
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q >= p)  // k(p,q) = 4p - p(p-1)/2 + (q-p)
                    acc[4 * p - (p * (p - 1)) / 2 + (q - p)] += (unsigned long long)__double_as_longlong(fma(rs[p], r[q], kMagic)) - kMagicBits;
        acc[9] += (unsigned long long)__double_as_longlong(fma(rs[3], r[3], kMagic)) - kMagicBits;
        acc[10] += 1;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long v = wave_reduce16_u64(acc, lane);
    if ((lane & 3) == 0) lds[wave][lane >> 2] = v;
    __syncthreads();
    if (threadIdx.x < 16) {
        unsigned long long t = 0;
        for (int w = 0; w < (T >> 6); w++) t += lds[w][threadIdx.x];
        totals[threadIdx.x] = t;
    }
    __syncthreads();
}

// reduce.cu:1158-1175 host unpack, on device
__device__ inline void so3_unpack(const unsigned long long* t, float A[9], float b[3], float residual[2])
{
    int shift = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 4; ++j) {
            const float value = fix_to_f32((long long)t[shift++], kFixSO3);
            if (j == 3) b[i] = value;
            else A[j * 3 + i] = A[i * 3 + j] = value;
        }
    residual[0] = fix_to_f32((long long)t[9], kFixSO3);
    residual[1] = (float)(long long)t[10];
}

__device__ inline void k_matrix(cf_cam c, double K[9])
{
    for (int i = 0; i < 9; i++) K[i] = 0;
    K[0] = c.fx; K[4] = c.fy; K[2] = c.cx; K[5] = c.cy; K[8] = 1;
}

// krkInv / kt for the next iteration (RGBDOdometry.cpp:347-358)
__device__ inline void prepare_iteration(OdomDev* od, int level)
{
    double K[9], Kinv[9], Rt[16];
    k_matrix(cam_level(od->intr, level), K);
    inv33<double>(K, Kinv);
    inv44_affine(od->resultRt, Rt);
    const double R[9] = {Rt[0], Rt[1], Rt[2], Rt[4], Rt[5], Rt[6], Rt[8], Rt[9], Rt[10]};
    double tmp[9], KRK[9];
    mul33<double>(K, R, tmp);
    mul33<double>(tmp, Kinv, KRK);
    for (int k = 0; k < 9; k++) od->krkInv[k] = (float)KRK[k];
    const double tv[3] = {Rt[3], Rt[7], Rt[11]};
    for (int r = 0; r < 3; r++) od->kt[r] = (float)(K[r * 3 + 0] * tv[0] + K[r * 3 + 1] * tv[1] + K[r * 3 + 2] * tv[2]);
}

// Stand-alone single SO3 step (C-ABI so3Step): one workgroup, totals to out16
__global__ void __launch_bounds__(1024) so3_step_kernel(const uint8_t* __restrict__ lastImage,
                                                        const uint8_t* __restrict__ nextImage, m33 B, m33 Ki, m33 krlr,
                                                        int cols, int rows, unsigned long long* __restrict__ out16)
{
    __shared__ unsigned long long lds[16][16];
    __shared__ unsigned long long totals[16];
    so3_pass(lastImage, nextImage, B, Ki, krlr.m, cols, rows, lds, totals, blockIdx.x, gridDim.x);
    if (threadIdx.x < 16) out16[threadIdx.x] = totals[threadIdx.x];
}

// Whole SO3 pre-alignment (RGBDOdometry.cpp:239-310) in ONE launch.  The pass over the 160x120 level is VALU-bound
// on a single CU (10.5 us per iteration, measured), so kSo3Blocks co-resident workgroups per model share it:
// each reduces its pixels, adds its 11 fixed-point totals to the iteration's slot of a global accumulator and
// meets the others at an atomic arrival counter; every workgroup then reads the totals and runs the identical 3x3
// solve + Rodrigues on its own LDS copy of the state, so nothing but integer atomics crosses workgroups and the
// data-dependent early exits stay uniform.  The last workgroup to leave re-zeroes the sync block for the next frame.
// Also seeds resultRt and the first iteration's krkInv/kt.
//
// ONE XCD PER MODEL (round 4).  Until round 4 the meeting was device-scope: atomics through the fabric, a release fence that writes the
// XCD's L2 back, polling loads that bypass it -- tools/microbench/xcd_barrier.hip measures 9.1 us for such a barrier of 32 workgroups
// (11.3 us across the chip) against 1.1 us when the workgroups share an XCD and meet in its L2 (atomics at workgroup scope execute in
// the L2, and so do the returning atomics the counters and sums are read with; nothing is written back).  The launch therefore has 8 x
// kSo3Blocks workgroups per model and keeps those whose index is (model mod 8) modulo 8: the dispatcher deals consecutive workgroups
// round-robin over the XCDs (what xcd_logical_block relies on too), so they share one.  Should that ever not hold, the arrival
// counters live in different L2s, the bounded wait below expires and raises the fault word -- cf_odom_fetch_result returns CF_ESTATE
// instead of a pose from partial sums.  The sums are integers: the bits do not depend on any of this.
// The launch is one-dimensional: [gx workgroups per model of the pre-alignment | prep_bx workgroups per model of the RGB preparation
// (Sobel + candidate mask + cloud: rgb_prep_body)].  The two read the same pyramids and depend on nothing of each other; the
// pre-alignment is a latency chain on 16 workgroups per model, the preparation fills the rest of the chip meanwhile.
//
// The tracker state of the call arrives here as well: the host fills its pinned copy, every pre-alignment workgroup stages that copy into
// LDS (one coalesced read over PCIe, hidden beside the preparation workgroups) and the lead workgroup of each tracker stores it into the
// device state the rest of the schedule reads -- no copy command in front of the loop (two of them cost ~10 us on the stream per frame).
#ifdef CF_ABLATE
// diagnostics build (CF_SO3_TRACE): stamps of tracker 0's lead workgroup in the pre-alignment loop, [iteration][8]
__device__ unsigned long long g_so3_trace[12][8];
#define OSTAMP(it, k) do { if (lead && by == 0 && threadIdx.x == 0) g_so3_trace[it][k] = wall_clock64(); } while (0)
#else
#define OSTAMP(it, k) do {} while (0)
#endif
__global__ void __launch_bounds__(256) so3_prealign_kernel(const TrackerStates ts, So3Sync* __restrict__ syncs, int do_so3,
                                                           int first_level, int gx, int so3_blocks, const RgbPrepBatch prep, int prep_bx)
{
    if ((int)blockIdx.x >= so3_blocks) {
        const int r = (int)blockIdx.x - so3_blocks, m = r / prep_bx;
        rgb_prep_body(prep.m[m], r - m * prep_bx);
        return;
    }
    const int by = (int)blockIdx.x / gx, bxx = (int)blockIdx.x - by * gx;  // gx is 1 or a multiple of 8: bxx mod 8 is the XCD
    OdomDev* const god = ts.dev[by];
    So3Sync* sync = syncs + by;
    __shared__ OdomDev s_od;
    __shared__ unsigned long long lds[16][16];
    __shared__ unsigned long long totals[16];
    __shared__ float s_basis[9], s_kinv[9], s_krlr[9];
    __shared__ int s_done;
    __shared__ double s_resultR[9];
    __shared__ double s_K[9], s_Kinv[9];
    __shared__ float s_Rlr[9];
    __shared__ float s_lastError, s_lastCount;
    __shared__ double s_lastResultR[9];
    __shared__ float s_jtj[9], s_jtr[3], s_delta[3], s_fws[15];
    __shared__ int s_iws[3];
    // with the pre-alignment the launch is 8 x kSo3Blocks wide: this model's workgroups are the ones on XCD (model mod 8)
    const bool one_xcd = do_so3 && gx > 1;
    if (one_xcd && (bxx & 7) != (by & 7)) return;
    const int bx = one_xcd ? (bxx >> 3) : bxx;
    const bool lead = bx == 0;  // the workgroup that uploads the state, publishes statistics and the final state
    const unsigned G = one_xcd ? (unsigned)gx >> 3 : (unsigned)gx;
    {
        static_assert(sizeof(OdomDev) % 4 == 0, "OdomDev is staged as 32-bit words");
        constexpr int kWords = (int)(sizeof(OdomDev) / 4);
        const unsigned* __restrict__ src = reinterpret_cast<const unsigned*>(ts.host[by]);
        constexpr int kPer = (kWords + 255) / 256;   // (both loads of a thread in flight together: they cross PCIe)
        unsigned w[kPer];
#pragma unroll
        for (int q = 0; q < kPer; q++) w[q] = ((int)threadIdx.x + 256 * q < kWords) ? src[threadIdx.x + 256 * q] : 0u;
#pragma unroll
        for (int q = 0; q < kPer; q++) if ((int)threadIdx.x + 256 * q < kWords) reinterpret_cast<unsigned*>(&s_od)[threadIdx.x + 256 * q] = w[q];
        __syncthreads();
        if (lead) for (int k = threadIdx.x; k < kWords; k += 256) reinterpret_cast<unsigned*>(god)[k] = reinterpret_cast<const unsigned*>(&s_od)[k];
        __syncthreads();  // (the lead's later stores into the device state follow the upload)
    }
    const OdomDev* const od = &s_od;  // what the host passed; results go to the device state (god)
    const int L = 2, cols = od->width >> L, rows = od->height >> L;
    if (threadIdx.x == 0) {
        for (int k = 0; k < 9; k++) { s_resultR[k] = (k % 4 == 0) ? 1.0 : 0.0; s_lastResultR[k] = s_resultR[k]; s_Rlr[k] = (k % 4 == 0) ? 1.f : 0.f; }
        k_matrix(cam_level(od->intr, L), s_K);
        inv33<double>(s_K, s_Kinv);
        s_lastError = 3.402823466e+38F / 2; s_lastCount = 3.402823466e+38F / 2;
        s_done = 0;
        if (lead) { god->stats.so3_iterations = 0; god->stats.last_so3_error = 0; god->stats.last_so3_count = 0; }
    }
    __syncthreads();
    if (do_so3) {
        const uint8_t* __restrict__ lastNext = od->lastNextImage[L];
        const uint8_t* __restrict__ next = od->nextImage[L];
        OSTAMP(11, 0);
        for (int it = 0; it < 10; it++) {
            OSTAMP(it, 0);
            if (threadIdx.x == 0) {
                double tmp[9], H[9];
                mul33<double>(s_K, s_resultR, tmp);
                mul33<double>(tmp, s_Kinv, H);
                for (int k = 0; k < 9; k++) { s_basis[k] = (float)H[k]; s_kinv[k] = (float)s_Kinv[k]; s_krlr[k] = (float)tmp[k]; }
            }
            __syncthreads();
            m33 B, Ki;
            for (int k = 0; k < 9; k++) { B.m[k] = s_basis[k]; Ki.m[k] = s_kinv[k]; }
            OSTAMP(it, 1);
            so3_pass(lastNext, next, B, Ki, s_krlr, cols, rows, lds, totals, bx, (int)G);  // ends with this workgroup's totals in LDS
            OSTAMP(it, 2);
            if (G > 1) {
                if (threadIdx.x < 64) {  // wave 0: publish, arrive, wait, collect -- everything in this XCD's L2
                    unsigned long long* slot = sync->acc[it];
                    if (threadIdx.x < 11 && totals[threadIdx.x] != 0)
                        __hip_atomic_fetch_add(&slot[threadIdx.x], totals[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the L2 has taken this wave's sums before it arrives
                    if (threadIdx.x == 0) {
                        __hip_atomic_fetch_add(&sync->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const unsigned target = (unsigned)(it + 1) * G;
                        unsigned spins = 0;
                        while (l2_read_u32(&sync->arrive) < target) {
                            if (++spins > (1u << 22)) { god->stats.fault = 1; break; }  // never hang the GPU; the host reports CF_ESTATE
                            __builtin_amdgcn_s_sleep(1);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    if (threadIdx.x < 16) totals[threadIdx.x] = l2_read_u64(&slot[threadIdx.x]);
                }
                __syncthreads();
            }
            OSTAMP(it, 3);
            if (threadIdx.x == 0) {
                float jtj[9], jtr[3], residual[2];
                so3_unpack(totals, jtj, jtr, residual);
                if (lead) god->stats.so3_iterations = it + 1;
                float err = sqrtf(residual[0]) / residual[1];
                float cnt = residual[1];
                if (err < s_lastError && (double)fabsf(s_lastError - cnt) < 0.001) {
                    s_done = 1;  // "converged" (compares error with COUNT, RGBDOdometry.cpp:285)
                } else if ((double)err > (double)s_lastError + 0.001) {
                    err = s_lastError; cnt = s_lastCount;
                    for (int k = 0; k < 9; k++) s_resultR[k] = s_lastResultR[k];
                    s_done = 1;
                } else {
                    s_lastError = err; s_lastCount = cnt;
                    for (int k = 0; k < 9; k++) s_lastResultR[k] = s_resultR[k];
                    for (int k = 0; k < 9; k++) s_jtj[k] = jtj[k];
                    for (int k = 0; k < 3; k++) s_jtr[k] = jtr[k];
                    ldlt_solve<float, 3>(s_jtj, s_jtr, s_delta, 1.17549435e-38f, s_fws, s_iws);
                    const float delta[3] = {s_delta[0], s_delta[1], s_delta[2]};
                    const double dd[3] = {delta[0], delta[1], delta[2]};
                    double rotUpdate[9];
                    rodrigues(dd, rotUpdate);
                    float ru[9], nr[9];
                    for (int k = 0; k < 9; k++) ru[k] = (float)rotUpdate[k];
                    mul33<float>(ru, s_Rlr, nr);
                    for (int k = 0; k < 9; k++) { s_Rlr[k] = nr[k]; s_resultR[k] = nr[k]; }
                }
                if (lead) { god->stats.last_so3_error = err; god->stats.last_so3_count = cnt; }
            }
            __syncthreads();
            OSTAMP(it, 4);
            if (s_done) break;
        }
        OSTAMP(11, 1);
        if (G > 1 && threadIdx.x == 0) {  // last one out resets the sync block (all workgroups are past their final read)
            if (__hip_atomic_fetch_add(&sync->depart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == G - 1) {
                for (int it = 0; it < 10; it++)
                    for (int w = 0; w < 16; w++) sync->acc[it][w] = 0;
                sync->arrive = 0; sync->depart = 0;
            }
        }
    }
    if (lead && threadIdx.x < 64) {
        // latch the bounding box the model-map pass accumulated (and clear the accumulator for the next frame); first screen box
        const int lane = threadIdx.x;
        unsigned key = 0;
        if (od->cull && lane < 6) { key = od->aabb_acc[lane]; od->aabb_acc[lane] = 0; }
        const float val = lane < 3 ? fkey_inv(~key) : fkey_inv(key);
        float lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { lo[k] = __shfl(val, k, 64); hi[k] = __shfl(val, 3 + k, 64); }
        if (__shfl((int)key, 3, 64) == 0) { lo[0] = 1.f; hi[0] = 0.f; }  // never written: empty
        int ib[4] = {0, 0, od->width - 1, od->height - 1};
        float zb[2] = {-__int_as_float(0x7f800000), __int_as_float(0x7f800000)};
        if (od->cull) screen_box(lo, hi, od->box_R, od->box_t, od->Rcurr, od->tcurr, od->intr, od->distThres, od->width, od->height, lane, ib, zb);
        if (lane == 0) {
            for (int k = 0; k < 3; k++) { god->box_lo[k] = lo[k]; god->box_hi[k] = hi[k]; }
            for (int k = 0; k < 4; k++) god->stats.cull_box[k] = ib[k];
            god->cull_z[0] = zb[0]; god->cull_z[1] = zb[1];
        }
    }
    if (lead && threadIdx.x == 0) {
        for (int k = 0; k < 16; k++) god->resultRt[k] = (k % 5 == 0) ? 1.0 : 0.0;
        if (do_so3)
            for (int x = 0; x < 3; x++)
                for (int y = 0; y < 3; y++) god->resultRt[x * 4 + y] = s_resultR[x * 3 + y];
        god->lastRGBError = 3.402823466e+38F;
        god->level_done = 0;
        god->residual[0] = 0; god->residual[1] = 0;
        prepare_iteration(god, first_level);
        refresh_hot(god);   // what the workgroups of the per-iteration launches read (cf_kernels.h: GnHot)
    }
}

}  // namespace cf
