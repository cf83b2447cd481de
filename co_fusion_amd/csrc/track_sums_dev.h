// track_sums_dev.h -- the fixed-point sum primitives of the dense tracking (part of track_reduce.hip's translation unit).
// Stage: what every reduction is built from -- the 27 + 1 triangular SE(3) products as integers, the workgroup's LDS accumulators, the
// cross-wave commits into the grouped 64-bit accumulators, and the reads / unpacking of their totals.  Replaces the warp / block
// reduceSum of Core/Cuda/reduce.cu (JtJJtrSE3, :167) and the host unpack of its result (:481-498).
#pragma once
#include "cf_device.h"
#include "cf_kernels.h"

namespace cf {

__device__ __forceinline__ float clamp_row(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// sink.add(k, a, b) with a * b = row_i*row_j*2^F (the sink adds se3_term(a, b), its integer bits) for the 27 upper-triangular SE3 products (k(i,j) = 7i - i(i-1)/2 + (j-i)) and the
// squared residual (k = 27).  lim / scale = 2^((50-F)/2) / 2^F: compile-time constants for the ICP sums, wave-uniform values for the RGB
// step (F follows sigma, rgb_fix_bits).  A sink says where a term is added: a register word or the LDS column of a lane.
__device__ __forceinline__ unsigned long long se3_term(double a, double b) { return (unsigned long long)__double_as_longlong(fma(a, b, kMagic)); }   // bits of RNE(a * b) + kMagic
template <class Sink>
__device__ __forceinline__ void se3_products(const float (&row)[7], float lim, float scale, const Sink& sink)
{
    double r[7];
#pragma unroll
    for (int i = 0; i < 7; i++) r[i] = (double)clamp_row(row[i], lim);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double rs = (double)(clamp_row(row[i], lim) * scale);
#pragma unroll
        for (int j = 0; j < 7; j++)
            if (j >= i) sink.add(7 * i - (i * (i - 1)) / 2 + (j - i), rs, r[j]);
    }
    sink.add(27, r[6] * (double)scale, r[6]);
}
struct RegSink { unsigned long long (&acc)[32]; __device__ __forceinline__ void add(int k, double a, double b) const { acc[k] += se3_term(a, b); } };
__device__ __forceinline__ void se3_accumulate_dyn(const float (&row)[7], unsigned long long (&acc)[32], float lim, float scale) { se3_products(row, lim, scale, RegSink{acc}); }

// ------------------------------------------------------------------------------------------------
// Product form of the ICP sums, round 5: the lanes add their products into the WORKGROUP's accumulators in LDS -- word k of lane l at
// [k][l], 64-bit LDS atomics without return, no bank conflicts -- and the butterfly runs ONCE per workgroup over what all waves (and
// all runs of a wave) left there, split over four waves (seven or eight words each).  Until then every wave ran the 32 x u64 butterfly
// on its own registers: 190 of the ~510 VALU instructions of a wave that the launch is bound by, and the 64 accumulator registers
// that set its occupancy.  Only lanes with a correspondence add; each adds the magic number's bits once per word, so the count of
// correspondences (word 28: a counter of its own, one LDS add per wave) times those bits comes off behind the butterfly.  Integer
// sums: who adds what in which order does not change a bit.
constexpr int kIcpLdsWords = 28;
__shared__ unsigned long long s_icp_acc[kIcpLdsWords][64];
__shared__ unsigned s_icp_found;
__device__ __forceinline__ void lds_add_u64(unsigned long long* p, unsigned long long v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void icp_lds_zero()   // (workgroup-uniform; the barrier behind it is the caller's)
{
    for (int i = threadIdx.x; i < kIcpLdsWords * 64; i += blockDim.x) (&s_icp_acc[0][0])[i] = 0;
    if (threadIdx.x == 0) s_icp_found = 0;
}
struct LdsSink { unsigned long long* col; __device__ __forceinline__ void add(int k, double a, double b) const { lds_add_u64(col + 64 * k, se3_term(a, b)); } };
template <int F>
__device__ __forceinline__ void se3_accumulate_lds(const float (&row)[7], int lane)
{
    constexpr float lim = (float)(1 << ((50 - F) / 2));
    constexpr float scale = (F == 32) ? 4294967296.0f : (float)(1u << (F & 31));
    se3_products(row, lim, scale, LdsSink{&s_icp_acc[0][lane]});
}
// ... and the workgroup's totals to its accumulator group in memory (all waves call it: the barrier is inside).  Wave g of the first
// four reduces words 8 g .. 8 g + 7 (fewer than four waves: they take turns); lanes 8 i of a wave end with word 8 g + i.
__device__ __forceinline__ void icp_lds_commit(int lane, int wave, int nwaves, unsigned long long* __restrict__ dst /* [32] of this group */)
{
    __syncthreads();
    const unsigned found = s_icp_found;
    if (found == 0) return;
    for (int g = wave; g < 4; g += nwaves) {
        unsigned long long acc[8];
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] = (g < 3 || k < 4) ? s_icp_acc[(g < 3 || k < 4) ? 8 * g + k : 0][lane] : 0ull;
        unsigned long long v = wave_reduce8_u64(acc, lane);
        const int w = 8 * g + (lane >> 3);
        if (w < 28) v -= (unsigned long long)found * kMagicBits;
        else v = w == 28 ? (unsigned long long)found : 0ull;
        if ((lane & 7) == 0 && v != 0) atomicAdd(&dst[w], v);
    }
}

// ------------------------------------------------------------------------------------------------
// cross-wave combine + grouped atomics.  v = wave total of word ((lane>>1)&31) (wave_reduce32_u64).
// XCD_LOCAL: the atomics are performed in the L2 of THIS XCD (workgroup scope) -- for sums that only workgroups of the same XCD add to and
// read back (rgb_step_solve_kernel).
template <int MAXW, bool XCD_LOCAL = false>
__device__ __forceinline__ void block_commit32(unsigned long long v, int lane, int wave, int nwaves,
                                               unsigned long long* __restrict__ dst /* [32] of this group */)
{
    __shared__ unsigned long long lds[MAXW][32];
    if ((lane & 1) == 0) lds[wave][lane >> 1] = v;
    __syncthreads();
    if (threadIdx.x < 32) {
        unsigned long long t = 0;
        for (int w = 0; w < nwaves; w++) t += lds[w][threadIdx.x];
        if (t != 0) {
            if constexpr (XCD_LOCAL) __hip_atomic_fetch_add(&dst[threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else atomicAdd(&dst[threadIdx.x], t);
        }
    }
}

// ... the workgroup's 32 totals (4 waves) stored as one row: no atomic, no read-modify-write in the L2 (rgb_step_solve_kernel)
__device__ __forceinline__ void block_store32(unsigned long long v, int lane, int wave, unsigned long long* __restrict__ row /* [32] */)
{
    __shared__ unsigned long long lds[4][32];
    if ((lane & 1) == 0) lds[wave][lane >> 1] = v;
    __syncthreads();
    if (threadIdx.x < 32) row[threadIdx.x] = lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] + lds[3][threadIdx.x];
}

// sum of word `w` over the groups (wave 0 only; result valid in all lanes of wave 0)
__device__ __forceinline__ unsigned long long group_sum(const unsigned long long* acc, int w, int lane)
{
    unsigned long long v = acc[(size_t)lane * 32 + w];  // kGroups == 64 == lanes
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
    return v;
}

// wrapping 32-bit sum over the 64 lanes of a wave, the same value in every lane: DPP inside each row of 16 lanes (two quad permutations, the
// mirrors of the half row and of the row), then the four row totals through scalar registers
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);    // quad_perm [1, 0, 3, 2]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);    // quad_perm [2, 3, 0, 1]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);   // row_half_mirror
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);   // row_mirror
    return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) + (unsigned)__builtin_amdgcn_readlane((int)v, 32) +
           (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

// Reads that are answered by the L2 itself: a RETURNING read-modify-write (OR with 0).  A load marked sc0 is a group-scope load, which
// the CU's vector L1 may serve -- with it the workgroups spun on a stale arrival count (reproduced in tools/microbench/xcd_barrier.hip).
__device__ __forceinline__ unsigned l2_read_u32(unsigned* p)
{
    unsigned v;
    const unsigned zero = 0;
    asm volatile("global_atomic_or %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p), "v"(zero) : "memory");
    return v;
}
__device__ __forceinline__ unsigned long long l2_read_u64(unsigned long long* p)
{
    unsigned long long v;
    const unsigned long long zero = 0;
    asm volatile("global_atomic_or_x2 %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p), "v"(zero) : "memory");
    return v;
}

// sigma handed to rgbStep (RGBDOdometry.cpp:373-385): (tmpError == 0) ? 1 : count   (sic: the COUNT)
__device__ __forceinline__ float sigma_val_from(int count, int sigma, int rgbOnly)
{
    if (rgbOnly) return -1.f;
    // tmpError = sqrt(sigma)/count is 0 iff sigma == 0 and count != 0 (0/0 is NaN, NaN != 0)
    return (sigma == 0 && count != 0) ? 1.f : (float)count;
}

// the 32-word accumulator layout, unpacked (reduce.cu:481-498)
__device__ inline void se3_unpack(const unsigned long long* t, int F, float A[36], float b[6], float residual[2])
{
    int shift = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 7; ++j) {
            const float value = fix_to_f32((long long)t[shift++], F);
            if (j == 6) b[i] = value;
            else A[j * 6 + i] = A[i * 6 + j] = value;
        }
    residual[0] = fix_to_f32((long long)t[27], F);
    residual[1] = (float)(long long)t[28];
}

// one word of se3_unpack: t < 27 -> A / b entry, 27 -> sum of squared residuals, 28 -> inlier count
// F < 0: the Gram form of the ICP sums (cf_device.h: word (i, j) carries kGramBits[i] + kGramBits[j] fraction bits)
__device__ __forceinline__ void se3_unpack_word(const unsigned long long* sums, int t, int F, float* A, float* b, float* residual)
{
    if (t < 27) {
        int i = 0, rem = t;
        while (rem >= 7 - i) { rem -= 7 - i; i++; }
        const int j = i + rem;
        const int bits = F >= 0 ? F : (i < 3 ? 20 : 17) + (j < 3 ? 20 : j < 6 ? 17 : 22);
        const float value = fix_to_f32((long long)sums[t], bits);
        if (j == 6) b[i] = value;
        else A[j * 6 + i] = A[i * 6 + j] = value;
    } else if (residual) {
        if (t == 27) residual[0] = fix_to_f32((long long)sums[27], F >= 0 ? F : 44);
        else if (t == 28) residual[1] = (float)(long long)sums[28];
    }
}
static_assert(kGramBits[0] == 20 && kGramBits[2] == 20 && kGramBits[3] == 17 && kGramBits[5] == 17 && kGramBits[6] == 22, "se3_unpack_word spells the Gram scales out");

// total of the grouped accumulator -> out[32] (stand-alone steps)
__global__ void __launch_bounds__(64) acc_total_kernel(const unsigned long long* __restrict__ acc, unsigned long long* __restrict__ out)
{
    for (int w = 0; w < 32; w++) {
        const unsigned long long v = group_sum(acc, w, threadIdx.x);
        if (threadIdx.x == 0) out[w] = v;
    }
}

// Split reductions (one tracker's image rows over several GPUs): a rank's partial sums are FOLDED before they travel -- the 64 accumulator
// groups of every split tracker summed into group 0, the other groups cleared -- so that the all-reduce of the Gauss-Newton loop carries
// the 32 words of the 6x6 system (256 bytes: north_star's "RCCL all-reduce of the 6x6 system") instead of the 16 KB of grouped partial
// sums it carried until round 5.  Everybody downstream (the RGB step's sigma, the solve) sums the groups as before
// and finds the totals in group 0 and zeros elsewhere: integer sums, the same bits.
struct FoldArgs { unsigned long long* acc[kMaxBatch]; };
__global__ void __launch_bounds__(64) acc_fold_kernel(const FoldArgs a)
{
    unsigned long long* __restrict__ acc = a.acc[blockIdx.x];
    const int lane = threadIdx.x;
    unsigned long long tot = 0;
#pragma unroll 4
    for (int w = 0; w < 32; w++) { const unsigned long long v = group_sum(acc, w, lane); if (lane == w) tot = v; }
    for (int w = 0; w < 32; w++) acc[(size_t)lane * 32 + w] = 0;   // (every load above has been consumed by a shuffle: the wave is past them)
    if (lane < 32) acc[lane] = tot;                                  // (same wave, program order: behind the zeroes of group 0)
}

}  // namespace cf
