// track_rgb_step_dev.h -- the RGB step of the dense tracking (part of track_reduce.hip's translation unit, included behind the
// residual pass and track_solve_dev.h).  From track_reduce.hip it uses idiv, rgb_hot / rgb_hot_and_range, residual_slot_range and
// icp_error_surface_body; from track_solve_dev.h gn_solve_body.
// Stage: the photometric Jacobian rows of the correspondences the residual pass left, summed into the RGB accumulators; three variants
// (cf_set_gn_mode 0 / 1 / 2).  Replaces RGBReduction / rgbStep of Core/Cuda/reduce.cu (:521-604, :635).
#pragma once
#include "track_solve_dev.h"

namespace cf {

// ================================================================================================
// RGB step: RGBReduction::getProducts, reduce.cu:521-604
// ================================================================================================
// Jacobian row of one valid correspondence (o = flat index in the next image, g = in the last image / point cloud)
__device__ __forceinline__ void rgb_step_row(const RgbArgs& ra, const RgbModelArgs& m, float sigma, float diff, int o, int g, float (&row)[7])
{
    const cf_cam il = ra.il;
    float w = sigma + fabsf(diff);
    w = w > 1.19209290E-07F ? 1.0f / w : 1.0f;
    if (sigma == -1) w = 1;
    row[6] = -w * diff;
    const float* cp = m.cloud + (size_t)g * 3;
    const float px = cp[0], py = cp[1], pz = cp[2];
    const float invz = 1.0f / pz;
    const float dI_dx_val = w * ra.sobelScale * (float)m.dIdx[o];
    const float dI_dy_val = w * ra.sobelScale * (float)m.dIdy[o];
    const float v0 = dI_dx_val * il.fx * invz;
    const float v1 = dI_dy_val * il.fy * invz;
    const float v2 = -(v0 * px + v1 * py) * invz;
    row[0] = v0; row[1] = v1; row[2] = v2;
    row[3] = -pz * v1 + py * v2;
    row[4] = pz * v0 - px * v2;
    row[5] = -py * v0 + px * v1;
}

// the fixed-point format the RGB sums are taken in, from sigma (sigma_val_from of the residual pass's two totals; how a kernel gets the
// totals is its own, measured choice): F = rgb_fix_bits(sigma) fraction bits, rows clamped to lim = 2^((50-F)/2)
struct RgbScale { float sigma; int F; float lim, scale; };
__device__ __forceinline__ RgbScale rgb_sigma_scale(float sigma)
{
    const int F = rgb_fix_bits(sigma);
    return RgbScale{sigma, F, ldexpf(1.0f, (50 - F) / 2), ldexpf(1.0f, F)};
}

// One wave's share of a record slot: records first, first + stride, ... of the slot's nrec (rc: record `first`, loaded by the caller
// together with the count) -> rows -> products; returns the wave's total of word ((lane>>1)&31) (wave_reduce32_u64), 0 without a record.
// Each record adds the magic number's bits once per word: the lane's count of records times those bits comes off in front of the butterfly.
__device__ __forceinline__ unsigned long long rgb_slot_wave_sum(const RgbArgs& ra, const RgbModelArgs& m, const RgbScale& sc, uint2 rc, size_t slot0, unsigned first,
                                                                unsigned nrec, unsigned stride, int lane)
{
    unsigned long long acc[32];
#pragma unroll
    for (int k = 0; k < 32; k++) acc[k] = 0;
    unsigned long long terms = 0;
    for (unsigned r = first; r < nrec; r += stride) {
        if (r >= stride) rc = m.recs[slot0 + r];
        float row[7];
        rgb_step_row(ra, m, sc.sigma, (float)((int)(rc.y >> 22) - 256), (int)rc.x, (int)(rc.y & 0x3fffffu), row);
        se3_accumulate_dyn(row, acc, sc.lim, sc.scale);
        terms++;
    }
    unsigned long long v = 0;
    if (__any(terms != 0)) {
#pragma unroll
        for (int k = 0; k < 28; k++) acc[k] -= terms * kMagicBits;
        acc[28] = terms;
        v = wave_reduce32_u64(acc, lane);
    }
    return v;
}

__global__ void __launch_bounds__(256) rgb_step_kernel(const RgbArgs ra)
{
    const RgbModelArgs& m = ra.m[blockIdx.y];
    const RgbHot hs = rgb_hot((StatePtr)m.st);
    if (hs.rgb && !hs.level_done) {
        const int cols = ra.cols, rows = ra.rows, N = cols * rows;
        __shared__ float s_sigma;
        if (threadIdx.x < 64) {
            const long long cnt = (long long)group_sum(m.icp_acc, 29, threadIdx.x);
            const long long sg = (long long)group_sum(m.icp_acc, 30, threadIdx.x);
            if (threadIdx.x == 0) s_sigma = sigma_val_from((int)cnt, (int)sg, hs.rgbOnly);
        }
        const int i = blockIdx.x * 256 + threadIdx.x;
        int4 raw = make_int4(0, 0, 0, 0);
        if (i < N) raw = *reinterpret_cast<const int4*>(&m.corres[i]);
        __syncthreads();
        const float sigma = s_sigma;
        unsigned long long acc[32];
#pragma unroll
        for (int k = 0; k < 28; k++) acc[k] = 0ull - kMagicBits;
        acc[28] = acc[29] = acc[30] = acc[31] = 0;
        float row[7] = {0, 0, 0, 0, 0, 0, 0};
        int found = 0;
        if (i < N) {
            const cf_dataterm c = *reinterpret_cast<const cf_dataterm*>(&raw);
            if (c.valid) {
                found = 1;
                rgb_step_row(ra, m, sigma, c.diff, c.one_y * cols + c.one_x, c.zero_y * cols + c.zero_x, row);
            }
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        unsigned long long v = 0;
        if (__any(found)) {  // a wave without a valid correspondence adds exact zeros
            const RgbScale sc = rgb_sigma_scale(sigma);
            se3_accumulate_dyn(row, acc, sc.lim, sc.scale);
            acc[28] = (unsigned long long)found;
            v = wave_reduce32_u64(acc, lane);
        }
        block_commit32<4>(v, lane, wave, 4, m.rgb_acc + (size_t)(blockIdx.x % kGroups) * 32);
    }
}

// RGB step over the per-workgroup record slots the residual pass left (grid: one workgroup per slot x models).  A slot holds at
// most 4 x producer-workgroup-size records and typically < 10 % of that; thread r reads record r of its slot speculatively together
// with the slot's count, so the pass has the same two dependent memory round trips as rgb_step_kernel on a tenth of the bytes.
//
// Measured and dropped (round 2, profiles/r02b): running this pass and the solve in ONE launch -- 32 workgroups per model reduce a
// global list, fence, arrive at a counter, workgroup 0 waits and solves.  22.6 us per launch against 6.3 + 8.4 us for the two
// separate kernels plus one boundary: the device-scope release fence and the arrival wait cost more than a kernel boundary does.
__device__ __forceinline__ void rgb_slot_step_body(const RgbArgs& ra, int n_slots)
{
    const RgbModelArgs m = ra.m[blockIdx.y];
    asm volatile("" :: "s"(m.st), "s"(m.icp_acc), "s"(m.rgb_acc), "s"(m.recs), "s"(m.slot_counts), "s"(m.res_range), "s"(m.cloud), "s"(m.dIdx), "s"(m.dIdy),
                 "s"(ra.cols), "s"(ra.rows), "s"(ra.slot_px), "s"(ra.sobelScale), "s"(ra.il.fx), "s"(ra.il.fy));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t slot0 = (size_t)blockIdx.x * ra.slot_px;
    // ONE flight of loads: the slot's count, this thread's record (speculative: valid if tid < n) and -- first wave -- the two words of the
    // accumulator groups that give sigma, all pinned in front of the uniform `n == 0` exit.  Without the pin the compiler sinks the record
    // and accumulator loads below that exit: three dependent round trips (count -> records + sums -> gathers) where two will do (round 6,
    // from the ISA: the `speculative` load of round 2 had not been speculative in the binary).
    unsigned n = m.slot_counts[blockIdx.x];
    const size_t Npx = (size_t)ra.cols * ra.rows;
    uint2 rc = m.recs[slot0 + tid < Npx ? slot0 + tid : Npx - 1];   // (unconditional, address clamped: a load under a branch is waited for at its end)
    unsigned long long g_cnt = 0, g_sig = 0;
    if (tid < 64) { g_cnt = m.icp_acc[(size_t)tid * 32 + 29]; g_sig = m.icp_acc[(size_t)tid * 32 + 30]; }   // kGroups == 64 == lanes
    asm volatile("" ::: "memory");   // (the vector loads are issued in front of the scalar round trip of the tracker's hot state, not behind it)
    SlotRange sr;
    const RgbHot hs = rgb_hot_and_range(ra, m, n_slots, sr);
    asm volatile("" : "+v"(n), "+v"(rc.x), "+v"(rc.y), "+v"(g_cnt), "+v"(g_sig));
    // (a slot outside a culled tracker's candidate range was not visited by the residual pass: its count is stale, it holds nothing)
    if ((int)blockIdx.x < sr.first || (int)blockIdx.x > sr.last) n = 0;
    if (!(hs.rgb && !hs.level_done) || n == 0) return;  // uniform
    __shared__ float s_sigma;
    if (tid < 64) {
        // sigma_val_from takes the LOW 32 bits of the two totals (the reference's `int` count and sigma), and the low word of a sum is the
        // wrapping sum of the low words: a 32-bit reduction over the 64 groups -- four DPP steps inside the rows of 16 lanes, the four row
        // totals added on the scalar unit -- instead of twelve dependent LDS shuffles of 64-bit values (0.35 us of this launch)
        const unsigned c32 = wave_sum_u32((unsigned)g_cnt), s32 = wave_sum_u32((unsigned)g_sig);
        if (tid == 0) s_sigma = sigma_val_from((int)c32, (int)s32, hs.rgbOnly);
    }
    __syncthreads();
    const unsigned long long v = rgb_slot_wave_sum(ra, m, rgb_sigma_scale(s_sigma), rc, slot0, tid, n, 256, lane);
    block_commit32<4>(v, lane, wave, 4, m.rgb_acc + (size_t)(blockIdx.x % kGroups) * 32);
}
__global__ void __launch_bounds__(256) rgb_slot_step_kernel(const RgbArgs ra, int n_slots) { rgb_slot_step_body(ra, n_slots); }
// ... and, on the last level-0 iteration, the error surfaces of the culled trackers in the SAME launch (workgroups behind the record
// slots; until late in round 6 icp_error_surface_kernel ran as a launch of its own between the {ICP || residual} launch and this one:
// 6.5 us + a launch boundary on the Gauss-Newton chain of every frame).  Both read the tracker state the solve has not touched yet.
__global__ void __launch_bounds__(256) rgb_slot_step_err_kernel(const RgbArgs ra, int n_slots, const IcpArgs e)
{
    if ((int)blockIdx.x >= n_slots) { icp_error_surface_body(e, e.m[blockIdx.y], (int)blockIdx.x - n_slots); return; }
    rgb_slot_step_body(ra, n_slots);
}

// MODE 2 (round 5): the RGB step and the solve in ONE launch.  Rounds 2-3 measured this twice with device-scope synchronisation and lost
// both times (a release fence per workgroup writes the XCD's L2 back; returning device-scope atomics cost a memory round trip each).
// What round 4's SO(3) kernel showed is that workgroups of ONE XCD can meet in its L2 for ~1.5 us: so the step workgroups of tracker m
// are placed on XCD m mod 8 (hardware workgroup b runs on XCD b mod 8: tools/microbench/xcc_map.hip), add their sums with
// workgroup-scope atomics -- performed in that L2 --, wait for them, and take a ticket there.  Nobody waits for anybody: the workgroup
// that draws the last ticket runs the solve (gn_solve_body reads the RGB sums back from the L2 with agent-scope loads), the others
// leave.  What the solve writes (state, cleared accumulators, the ticket counter) is written back at the end of the kernel like any
// other store.  One launch boundary (~2.5 us) and the solve kernel's own ramp less per Gauss-Newton iteration: 57 -> 38 launches per
// frame.  The sums are integers: which workgroup adds what, and who solves, does not change a bit.
// Grid: 8 x n_quads x ceil(n / 8) workgroups, n_quads = ceil(n_slots / 2) (two record slots per workgroup), b = 8 * (quad + n_quads * (m / 8)) + m % 8.
__global__ void __launch_bounds__(256) rgb_step_solve_kernel(const RgbArgs ra, So3Sync* __restrict__ syncs, int n_slots, int n_quads, IDiv quad_div,
                                                             int n, int icp_fix, int next_level, int last_of_level)
{
    const int b = (int)blockIdx.x;
#ifdef CF_ABLATE
    unsigned long long* const tr = g_icp_trace ? g_icp_trace + (size_t)b * 8 : nullptr;
    if (tr && threadIdx.x == 0) { tr[0] = wall_clock64(); tr[1] = tr[2] = tr[3] = tr[4] = 0; tr[5] = 0xffff; }
#define STAMP(k) do { if (tr && threadIdx.x == 0) tr[k] = wall_clock64(); } while (0)
#else
#define STAMP(k) do {} while (0)
#endif
    const int q = b >> 3, hi = n_quads > 1 ? idiv(q, quad_div) : q;
    const int model = (b & 7) + 8 * hi, quad = q - hi * n_quads;
    if (model >= n) return;
    const RgbModelArgs& m = ra.m[model];
    const RgbHot hs = rgb_hot((StatePtr)m.st);
    SlotRange sr = residual_slot_range(ra, m, n_slots);
    const bool no_slot = sr.last < sr.first;   // a culled tracker without a single candidate: its first workgroup stands in (and solves)
    if (no_slot) { sr.first = 0; sr.last = 0; }
    const int qf = sr.first >> 1, ql = sr.last >> 1;
    if (quad < qf || quad > ql) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Two record slots per workgroup, two waves per slot (`quad`: the pair's index).  The tracker's workgroups share ONE XCD: a workgroup
    // per slot (round 4's shape) makes the background's 300 slots two rounds of residency there (measured: +4 us), a WAVE per slot leaves a
    // slot with 700 records to eleven dependent passes of one wave (measured: +8 us).  150 workgroups x 4 waves fit the XCD in one round.
    const int slot = quad * 2 + (wave >> 1), half = tid & 127;
    const bool slot_ok = !no_slot && slot >= sr.first && slot <= sr.last;
    const size_t slot0 = (size_t)slot * ra.slot_px;
    const unsigned nrec = slot_ok ? m.slot_counts[slot] : 0u;
    uint2 rc = make_uint2(0, 0);
    if (slot_ok && slot0 + half < (size_t)ra.cols * ra.rows) rc = m.recs[slot0 + half];   // speculative: valid if half < nrec
    if (hs.rgb && !hs.level_done) {  // uniform
        unsigned long long v = 0;
        if (nrec != 0) {   // (wave-uniform)
            const long long cnt = (long long)group_sum(m.icp_acc, 29, lane);
            const long long sg = (long long)group_sum(m.icp_acc, 30, lane);
            v = rgb_slot_wave_sum(ra, m, rgb_sigma_scale(sigma_val_from((int)cnt, (int)sg, hs.rgbOnly)), rc, slot0, half, nrec, 128, lane);
        }
        STAMP(1);
        block_store32(v, lane, wave, m.rgb_acc + (size_t)quad * 32);
    } else if (tid < 32) m.rgb_acc[(size_t)quad * 32 + tid] = 0;
#ifdef CF_ABLATE
    if (tr && threadIdx.x == 0) tr[5] = (unsigned long long)model;
#endif
    // The tickets, drawn by the wave that issued the atomics, once the L2 has taken them.  Two levels: returning atomics on ONE address
    // take the L2 ~17 ns each, so a workgroup draws from the counter of its quad's residue class mod kStepSubs (each in a cache line of
    // its own), and the last of a class draws from the tracker's top counter.
    __shared__ int s_last;
    So3Sync* const sync = syncs + model;
    if (tid < 64) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        STAMP(2);
        if (tid == 0) {
            static_assert(kStepSubs == 16, "the class arithmetic below shifts by 4");
            const int j = quad & (kStepSubs - 1);
            // quads = j (mod kStepSubs) inside [qf, ql]; classes that have any
            const unsigned in_class = (unsigned)(((ql - j) >> 4) - ((qf - 1 - j) >> 4));
            const int span = ql - qf + 1;
            const unsigned classes = (unsigned)(span < kStepSubs ? span : kStepSubs);
            int last = 0;
            if (__hip_atomic_fetch_add(&sync->step_sub[j][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == in_class - 1u) {
                sync->step_sub[j][0] = 0;   // (every ticket of this class is drawn; the next launch finds the counter cleared)
                if (__hip_atomic_fetch_add(&sync->step_top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == classes - 1u) { sync->step_top = 0; last = 1; }
            }
            s_last = last;
        }
    }
    STAMP(3);
    __syncthreads();
    if (!s_last) return;
    OdomDev* const god = m.st;
    gn_solve_body<true>(icp_fix, god, m.icp_acc, m.rgb_acc, next_level, last_of_level, nullptr, ra.slot_px, qf, ql);
    STAMP(4);
#undef STAMP
}

}  // namespace cf
