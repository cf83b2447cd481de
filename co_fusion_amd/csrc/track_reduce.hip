// track_reduce.hip -- the dense-tracking reductions and the device-resident Gauss-Newton loop.
//
// MI355X-native replacement of Core/Cuda/reduce.cu (icpStep / computeRgbResidual / rgbStep /
// so3Step) and of the host loop RGBDOdometry::getIncrementalTransformation
// (Core/Utils/RGBDOdometry.cpp:217-477).
//
// Design (DESIGN.md "tracking"):
//  * The reference does, per GN iteration, 3 x (kernel -> 1-block reduceSum -> cudaDeviceSynchronize
//    -> D2H) and solves the 6x6 system on the host: <= 67 host round trips per model per frame.
//    Here the pose, the 6x6 solve (f64 LDL^T) and the SE3 update live on the device; one frame's
//    whole schedule (SO3 pre-alignment + 4/5/10 iterations) is enqueued without any host wait,
//    and all active models advance in lock-step inside the same launches (blockIdx.y = model).
//  * Reductions are wave64 butterflies over *integer* (fixed-point) partial sums followed by
//    grouped 64-bit atomics: exact, order independent, identical for every launch shape / GPU count.
//  * ICP is HBM/L2-bound streaming (48 B/pixel: 6 coalesced plane loads + 6 gathered loads);
//    blockIdx -> pixel-range mapping is XCD-aware: workgroup b runs on XCD b%8, and XCD x owns
//    the x-th horizontal band of the image, so the gathered model-map rows stay in that XCD's
//    4 MiB L2 across the 19 iterations of a frame.
//
// One translation unit, five files (the headers are included by this file only):
//   track_sums_dev.h      the fixed-point sum primitives: SE(3) products, LDS accumulators, commits, reads of the totals
//   track_reduce.hip      the {ICP reduction || RGB residual} launch, the error surfaces, the candidate mask, the XCD probe; every launcher
//   track_so3_dev.h       the SO(3) pre-alignment
//   track_solve_dev.h     the per-iteration Gauss-Newton solve
//   track_rgb_step_dev.h  the RGB step in its three variants (cf_set_gn_mode 0 / 1 / 2)
#include "cf_device.h"
#include "cf_kernels.h"
#include "track_prep_dev.h"
#include "track_sums_dev.h"

namespace cf {

__device__ __forceinline__ int idiv(int n, IDiv d) { return (int)(__umulhi((unsigned)n, d.M) >> d.s); }  // n / cols, cf_kernels.h: make_idiv

// ================================================================================================
// ICP:  ICPReduction::search + getProducts, reduce.cu:283-394
// ================================================================================================
// The two gates of the correspondence test compare square roots with constants (reduce.cu:321-325:
// sine < angleThres, dist <= distThres).  sqrtf is correctly rounded and monotonic, so each gate is decided
// exactly by comparing the radicand with a precomputed f32 bound (IcpArgs::angleSqLt / distSqLe, sqrt_gate_* below):
// no square root per pixel unless the error surface (which stores dist itself) is requested.
struct IcpProj { f3 vcurr_g; int g; int inb; int ux, uy; };

__device__ __forceinline__ IcpProj icp_project(const m33& Rcurr, const f3& tcurr, const m33& Rprev_inv, const f3& tprev, const cf_cam& intr,
                                               int cols, int rows, f3 vcurr)
{
    IcpProj o;
    o.vcurr_g = mul(Rcurr, vcurr) + tcurr;
    const f3 vcurr_cp = mul(Rprev_inv, o.vcurr_g - tprev);
    const int ux = f2i_rn(vcurr_cp.x * intr.fx / vcurr_cp.z + intr.cx);
    const int uy = f2i_rn(vcurr_cp.y * intr.fy / vcurr_cp.z + intr.cy);
    o.inb = !(ux < 0 || uy < 0 || ux >= cols || uy >= rows || vcurr_cp.z < 0);
    o.g = o.inb ? uy * cols + ux : 0;
    o.ux = o.inb ? ux : 0; o.uy = o.inb ? uy : 0;
    return o;
}

template <int PPT> struct VecF;
template <> struct VecF<1> { using T = float; };
template <> struct VecF<2> { using T = float2; };
template <> struct VecF<4> { using T = float4; };

template <int PPT>
__device__ __forceinline__ void load_vec(const float* p, float (&o)[PPT])
{
    using V = typename VecF<PPT>::T;
    const V v = *reinterpret_cast<const V*>(p);
    const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
    for (int i = 0; i < PPT; i++) o[i] = f[i];
}

// XCD-aware logical block id: hardware block b lands on XCD b%8; give XCD x the x-th contiguous
// range of logical blocks (= a horizontal band of the image).
__device__ __forceinline__ int xcd_logical_block(int b, int nlog)
{
    const int per = (nlog + 7) >> 3;
    return (b & 7) * per + (b >> 3);
}

template <bool COMPACT> __device__ void rgb_residual_body(const RgbArgs& ra, int model, int blk, int nblk);

// One launch per Gauss-Newton iteration carries BOTH pose-dependent streaming passes, which are independent
// of each other: workgroups [0, n_icp_blocks) run the ICP reduction, the rest the RGB residual pass
// (rgb_residual_body).  At 640x480 either pass alone is launch/latency-bound (5-8 us for 8-15 MB); sharing
// a launch overlaps their ramp-up, gather latency and atomics tail.
//
// Kernel arguments by value: every pointer the kernel dereferences arrives in the kernarg segment
// (scalar loads, global-address-space vector loads, no pointer chasing through device structs).
// Only the pose/flags, which the solve updates on the device every iteration, are read from
// memory -- as scalar loads issued in parallel with the first coalesced map loads.
//
// VALU budget (the kernel is VALU-bound once several models share a launch): the lanes' products go to the workgroup's accumulators in
// LDS and ONE butterfly per workgroup reduces them (se3_accumulate_lds / icp_lds_commit; until round 5 every wave ran a 32 x u64
// butterfly on its registers); a wave whose pixels cannot produce a correspondence (projection out of view, model map empty
// there -- the common case for object models, which cover a small part of the image) leaves after the projection.
static_assert(sizeof(IcpArgs) + sizeof(RgbArgs) + 64 <= 4096, "the kernel-argument segment holds 4 KB: lower kMaxBatch");  // (rgb_slot_step_kernel takes both as well)
//
// GRAM (cf_set_icp_arith 1): the accumulation and the butterfly are replaced by the matrix cores -- the rows are rounded to integers,
// staged through LDS as signed 8-bit limbs and contracted over the wave's pixels by v_mfma_i32_32x32x32_i8 (cf_device.h: gram_*);
// dynamic LDS = kGramWaveDwords * 4 bytes per wave (gram_block_commit adds the waves' tiles and recombines the limbs).  A different rounding specification (ORC_ICP_ARITH_GRAM in the oracle).
// Timing ablations of the launch (CF_ICP_REPLAY, DESIGN-NOTES): bits 8.. of IcpArgs::flags switch parts of the kernel off.  They exist in
// a diagnostics build only (make ABLATE=1 -> -DCF_ABLATE); in the production kernel ABL() is the constant 0 and the tests vanish.
#ifdef CF_ABLATE
#define ABL(bits) ((args.flags >> 8) & (bits))
#else
#define ABL(bits) 0
#endif
extern __shared__ int gram_lds[];
// One run of pixels of one model: the 6 plane loads, projection, gather, gates, rows, accumulation and the wave butterfly.
// i0 = this lane's first pixel, in_range = the lane's pixels take part.  Returns false when the tracker has nothing to do at this level
// (workgroup-uniform: the caller leaves).  Product form: the sums are left in the workgroup's LDS accumulators (icp_lds_commit); Gram form: gram_has.
// The tracker state is written by the solve kernel of the PREVIOUS launch and only read here: through the constant address space its
// (wave-uniform) loads are scalar loads whatever the compiler can prove about the stores around them -- with the run loop in the kernel
// it fell back to per-lane vector loads of the pose, 44 more VGPRs and three waves of occupancy less.
typedef const __attribute__((address_space(4))) OdomDev* StatePtr;
// the hot state (cf_kernels.h: GnHot), one 64-byte line per s_load_dwordx16; hot_pin() keeps the loads of a clause together in front of
// ONE wait (without it the compiler sinks each load to its first use: a chain of dependent round trips to memory again)
typedef int hot16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ hot16 hot_line(StatePtr st, int line)
{
    return *(reinterpret_cast<const __attribute__((address_space(4))) hot16*>(&st->hot) + line);
}
__device__ __forceinline__ void hot_pin(const hot16& a) { asm volatile("" :: "s"(a)); }
__device__ __forceinline__ void hot_pin(const hot16& a, const hot16& b) { asm volatile("" :: "s"(a), "s"(b)); }
// (by value through __int_as_float: __builtin_bit_cast(float, l[k]) on a vector ELEMENT reads element 0 with this compiler -- ROCm 7.2 clang)
__device__ __forceinline__ float hot_f(const hot16& l, int k) { const int v = l[k]; return __int_as_float(v); }
struct IcpHot {   // lines 0 + 1
    int icp, level_done; float zlo, zhi; m33 Rcurr, Rprev_inv; f3 tcurr, tprev; int box[4];
};
__device__ __forceinline__ IcpHot icp_hot(StatePtr st)
{
    hot16 l0 = hot_line(st, 0), l1 = hot_line(st, 1);
    hot_pin(l0, l1);
    IcpHot h;
    h.icp = l0[0]; h.level_done = l0[1]; h.zlo = hot_f(l0, 2); h.zhi = hot_f(l0, 3);
#pragma unroll
    for (int k = 0; k < 9; k++) { h.Rcurr.m[k] = hot_f(l0, 4 + k); h.Rprev_inv.m[k] = hot_f(l1, k); }
    h.tcurr = f3{hot_f(l0, 13), hot_f(l0, 14), hot_f(l0, 15)};
    h.tprev = f3{hot_f(l1, 9), hot_f(l1, 10), hot_f(l1, 11)};
#pragma unroll
    for (int k = 0; k < 4; k++) h.box[k] = l1[12 + k];
    return h;
}
struct RgbHot { int rgb, rgbOnly, level_done; float krk[9], kt[3]; };   // line 2
__device__ __forceinline__ RgbHot rgb_hot(StatePtr st)
{
    hot16 l2 = hot_line(st, 2);
    hot_pin(l2);
    RgbHot h;
    h.rgb = l2[0]; h.rgbOnly = l2[1]; h.level_done = l2[2];
#pragma unroll
    for (int k = 0; k < 9; k++) h.krk[k] = hot_f(l2, 4 + k);
#pragma unroll
    for (int k = 0; k < 3; k++) h.kt[k] = hot_f(l2, 13 + k);
    return h;
}
static_assert(offsetof(GnHot, Rcurr) == 16 && offsetof(GnHot, tcurr) == 52 && offsetof(GnHot, Rprev_inv) == 64 && offsetof(GnHot, tprev) == 100 &&
              offsetof(GnHot, cull_box) == 112 && offsetof(GnHot, rgb) == 128 && offsetof(GnHot, krkInv) == 144 && offsetof(GnHot, kt) == 180, "icp_hot / rgb_hot spell the layout out");

template <int PPT, bool GRAM>
__device__ __forceinline__ bool icp_run(const IcpArgs& args, const IcpModelArgs& ma, StatePtr st, const IcpHot& pre, bool have_pre, int i0, bool in_range,
                                        bool whole, int band0, int band1, float* __restrict__ errs, int abl, int lane, int wave,
                                        unsigned long long& v, bool& gram_has, bool& done)
{
    const int cols = args.cols, rows = args.rows, N = cols * rows;
    const float* __restrict__ vc = ma.vc;
    const float* __restrict__ nc = ma.nc;
    const float* __restrict__ vp = ma.vp;
    const float* __restrict__ np = ma.np;
    float vx[PPT], vy[PPT], vz[PPT], nx[PPT], ny[PPT], nz[PPT];
#pragma unroll
    for (int p = 0; p < PPT; p++) { vx[p] = vy[p] = vz[p] = nx[p] = ny[p] = nz[p] = qnan(); }
    if (in_range) {  // the frame maps do not depend on the tracker state: issued before the state is looked at
        load_vec<PPT>(vc + i0, vx); load_vec<PPT>(vc + i0 + N, vy); load_vec<PPT>(vc + i0 + 2 * N, vz);
        load_vec<PPT>(nc + i0, nx); load_vec<PPT>(nc + i0 + N, ny); load_vec<PPT>(nc + i0 + 2 * N, nz);
    }
    IcpHot hs = pre;                              // (a caller that had to look at the box first hands the state in; otherwise its one
                                                  // scalar round trip runs beside the plane loads just issued)
    if (!have_pre) hs = icp_hot(st);
    if (!hs.icp || hs.level_done) return false;
    const m33 Rcurr = hs.Rcurr, Rprev_inv = hs.Rprev_inv;
    const f3 tcurr = hs.tcurr, tprev = hs.tprev;

    // projection + gather of the model maps
    IcpProj pr[PPT];
    f3 vprev[PPT], nprev[PPT];
    int cand = 0;
#pragma unroll
    for (int p = 0; p < PPT; p++) { pr[p].vcurr_g = f3{qnan(), qnan(), qnan()}; pr[p].g = 0; pr[p].inb = 0; pr[p].ux = pr[p].uy = 0; vprev[p] = pr[p].vcurr_g; nprev[p] = pr[p].vcurr_g; }
    if (__any(in_range))  // (a wave culled by the screen box skips the projection as well)
#pragma unroll
    for (int p = 0; p < PPT; p++) {
        pr[p] = icp_project(Rcurr, tcurr, Rprev_inv, tprev, args.intr, cols, rows, f3{vx[p], vy[p], vz[p]});
        if (!in_range) pr[p].inb = 0;
        bool occupied = pr[p].inb != 0;
        if (occupied && ma.occ) {  // the model map is invalid (NaN) everywhere inside an empty 4x4 block: no gather needed
            const int tile = (pr[p].uy >> args.occ_shift) * args.occ_w + (pr[p].ux >> args.occ_shift);
            occupied = ma.occ[tile] != 0;
        }
        if (occupied) {
            const int g = pr[p].g;
            vprev[p] = f3{vp[g], vp[g + N], vp[g + 2 * N]};
            nprev[p] = f3{np[g], np[g + N], np[g + 2 * N]};
        }
        // necessary for a correspondence: in view, both normals valid, a finite model vertex
        if (whole && (i0 + p < band0 || i0 + p >= band1)) continue;  // outside this rank's band: error surface only
        cand |= (pr[p].inb && !is_nan(nx[p]) && !is_nan(nprev[p].x) && !is_nan(vprev[p].x)) ? 1 : 0;
    }
    const bool wave_cand = __any(cand) != 0;
    if (errs) {  // last level-0 iteration: the error surface stores dist for every pixel (0 if not finite / out of view)
#pragma unroll
        for (int p = 0; p < PPT; p++)
            if (in_range) {
                float err = 0.f;
                if (pr[p].inb) { const float dist = norm(vprev[p] - pr[p].vcurr_g); err = is_finite(dist) ? dist : 0.0f; }
                errs[i0 + p] = err;
            }
    }
    // A wave without a single candidate contributes exact zeros (all rows are zero): skip the rows, the accumulation and
    // the butterfly.  Object models cover a small part of the image, so most of their waves take this exit.
    if (wave_cand || abl) {
        float row[PPT][7];
        int fnd[PPT], any_found = 0;
#pragma unroll
        for (int p = 0; p < PPT; p++) {
#pragma unroll
            for (int k = 0; k < 7; k++) row[p][k] = 0.f;
            const f3 ncurr_g = mul(Rcurr, f3{nx[p], ny[p], nz[p]});
            const f3 dv = vprev[p] - pr[p].vcurr_g;
            const float dist2 = dot(dv, dv);
            const f3 cr0 = cross(ncurr_g, nprev[p]);
            const float sine2 = dot(cr0, cr0);
            fnd[p] = (pr[p].inb && sine2 < args.angleSqLt && dist2 <= args.distSqLe && !is_nan(nx[p]) && !is_nan(nprev[p].x)) ? 1 : 0;
            if (whole && (i0 + p < band0 || i0 + p >= band1)) fnd[p] = 0;
            any_found |= fnd[p];
            if (fnd[p]) {
                const f3 s_cp = mul(Rprev_inv, pr[p].vcurr_g - tprev);
                const f3 d_cp = mul(Rprev_inv, vprev[p] - tprev);
                const f3 n_cp = mul(Rprev_inv, nprev[p]);
                const f3 cr = cross(s_cp, n_cp);
                row[p][0] = n_cp.x; row[p][1] = n_cp.y; row[p][2] = n_cp.z;
                row[p][3] = cr.x; row[p][4] = cr.y; row[p][5] = cr.z;
                row[p][6] = dot(n_cp, s_cp - d_cp);
            }
        }
        if constexpr (GRAM) {
            if (__any(any_found) || abl != 0) {
                int* wl = gram_lds + wave * kGramWaveDwords;
                gram_v16i macc;
#pragma unroll
                for (int r = 0; r < 16; r++) macc[r] = 0;
#pragma unroll
                for (int p = 0; p < PPT; p++) {
#pragma unroll
                    for (int k = 0; k < 7; k++)
                        wl[k * kGramRowStride + lane] = (int)gram_limbs((int)rintf(clamp_row(row[p][k], kGramLim[k]) * (float)(1 << kGramBits[k])));
                    wl[7 * kGramRowStride + lane] = (int)gram_limbs(fnd[p]);
                    __builtin_amdgcn_wave_barrier();   // (one wave, LDS in program order: the reads below see every lane's dwords)
                    macc = gram_wave_mfma(wl, lane, macc);
                    __builtin_amdgcn_wave_barrier();
                }
                gram_wave_store(wl, macc, lane);   // (after the last read of the staging area; LDS runs in program order)
                gram_has = true;
            }
        } else
        if (__any(any_found) || abl != 0) {
#pragma unroll
            for (int p = 0; p < PPT; p++) {
                if (fnd[p] && !(abl & 1)) se3_accumulate_lds<kFixICP>(row[p], lane);
                const int nf = __popcll(__ballot(fnd[p] != 0));
                if (lane == 0 && nf) (void)__hip_atomic_fetch_add(&s_icp_found, (unsigned)nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (abl & 2) { done = true; return true; }
        }
    }
    return true;
}

// The ICP error surface (icpStep's optional output, reduce.cu:327-331 / RGBDOdometry.cpp:414-431: the distance between every pixel's
// vertex and the model vertex it projects onto, 0 when not finite / out of view) of the last level-0 iteration, one pixel per lane.
// Until round 4 that iteration's ICP pass wrote it for every tracker, which kept the launch from culling anything (23.8 us against
// 15.4 us for the nine iterations before it); now the culled trackers stay culled and THEIR surfaces are written by a launch of its own
// between that iteration's {ICP || residual} launch and its RGB step (icp_error_surface_kernel) -- the same pose, the expressions of
// icp_run, the same bits.  (Round 4 had these workgroups in the RGB step's launch; with the solve inside that launch --
// rgb_step_solve_kernel, cf_set_gn_mode 2 -- the pose would change under them.)  Unculled trackers write theirs in the ICP pass as before.
__device__ __forceinline__ void icp_error_surface_body(const IcpArgs& args, const IcpModelArgs& ma, int blk)
{
    float* __restrict__ errs = ma.err;
    if (!errs || !ma.cull) return;  // (an unculled tracker wrote its surface in the ICP pass it ran over the whole image anyway)
    StatePtr st = (StatePtr)ma.st;
    const int cols = args.cols, rows = args.rows, N = cols * rows;
    const int i = blk * (int)blockDim.x + (int)threadIdx.x;
    const bool in_range = i < N;
    float vx = qnan(), vy = qnan(), vz = qnan();
    if (in_range) { vx = ma.vc[i]; vy = ma.vc[i + N]; vz = ma.vc[i + 2 * N]; }
    const IcpHot hs = icp_hot(st);
    if (!hs.icp || hs.level_done) return;  // (icp_run leaves before it writes anything)
    const m33 Rcurr = hs.Rcurr, Rprev_inv = hs.Rprev_inv;
    const f3 tcurr = hs.tcurr, tprev = hs.tprev;
    if (!in_range) return;
    const IcpProj pr = icp_project(Rcurr, tcurr, Rprev_inv, tprev, args.intr, cols, rows, f3{vx, vy, vz});
    f3 vprev = {qnan(), qnan(), qnan()};
    bool occupied = pr.inb != 0;
    if (occupied && ma.occ) occupied = ma.occ[(pr.uy >> args.occ_shift) * args.occ_w + (pr.ux >> args.occ_shift)] != 0;
    if (occupied) vprev = f3{ma.vp[pr.g], ma.vp[pr.g + N], ma.vp[pr.g + 2 * N]};
    float err = 0.f;
    if (pr.inb) { const float dist = norm(vprev - pr.vcurr_g); err = is_finite(dist) ? dist : 0.0f; }
    errs[i] = err;
}

__global__ void __launch_bounds__(256) icp_error_surface_kernel(const IcpArgs args) { icp_error_surface_body(args, args.m[blockIdx.y], (int)blockIdx.x); }

// Culling tests of a run of consecutive pixels against a tracker's screen box (level-0 pixels, IcpHot::box) at pyramid level L
struct PixBox { int x0, y0, x1, y1; };
__device__ __forceinline__ PixBox dilated_box(const int (&box)[4], int L) { return PixBox{(box[0] >> L) - 1, (box[1] >> L) - 1, (box[2] >> L) + 1, (box[3] >> L) + 1}; }
// does the run [first, last] of flat pixel indices (it may straddle rows) miss the rectangle?  The test of the run's first / last pixel
__device__ __forceinline__ bool span_misses_box(int first, int last, int cols, IDiv cdiv, int bx0, int by0, int bx1, int by1)
{
    const int q0 = idiv(first, cdiv), q1 = idiv(last, cdiv);
    return q1 < by0 || q0 > by1 || (q0 == q1 && (last - q0 * cols < bx0 || first - q0 * cols > bx1));
}

// GRID.  One-dimensional, in SLOTS: a slot is the ICP reduction or the RGB residual pass of one model.  IcpArgs::slot_end holds the running
// totals of the workgroups, IcpArgs::slot_desc what every slot is; the launcher orders them longest work first (launch_icp_rgbres).
// Every slot starts at a multiple of 8, so hardware workgroup b and its slot-local index agree on the XCD (b % 8).
//  * A model that is not culled gets one workgroup per run of T * PPT pixels of its image (or row band), XCD x owning the x-th
//    horizontal band (xcd_logical_block).
//  * A CULLED model (IcpModelArgs::box_blocks > 0) gets box_blocks workgroups -- sized by the host from the screen box the model ended
//    the previous frame with -- whose waves are dealt the 64-pixel runs INSIDE the model's current screen box (cull_runs: the rectangle
//    in units of runs when the image width is a multiple of 64, the rows of the box otherwise); a wave walks on by the number of waves
//    when the box has more runs than the host expected.  Until round 4 a culled model had the whole image's workgroups, 80 % of
//    which read the box and left: 4 800 of the 7 500 workgroups of a five-model level-0 launch, dispatched ahead of the work that the
//    launch waits for.  Sums are integers: which wave adds which pixel does not change a bit.
template <int PPT, bool GRAM>
__device__ __forceinline__ void icp_reduce_body(const IcpArgs& args, const RgbArgs& ra, int n_icp_blocks)
{
    const int b = blockIdx.x;
    // Slot decode on the scalar unit, from ONE clause of kernel-argument loads: table entries and descriptor bytes by static index (a
    // dynamic index into the argument segment is a dependent load each), the slot's bounds picked up along the way.  Then the model's
    // argument block as one more clause (pinned: the compiler otherwise loads field by field at first use -- ten dependent scalar
    // round trips in front of a wave's first vector load, each a miss for the first wave on a CU).
    int slot0 = 0, send, desc;
    {
        int e[12], d[12];
#pragma unroll
        for (int k = 0; k < 12; k++) { e[k] = args.slot_end[k]; d[k] = args.slot_desc[k]; }
        asm volatile("" :: "s"(e[0]), "s"(e[1]), "s"(e[2]), "s"(e[3]), "s"(e[4]), "s"(e[5]), "s"(e[6]), "s"(e[7]), "s"(e[8]), "s"(e[9]), "s"(e[10]), "s"(e[11]),
                     "s"(d[0]), "s"(d[4]), "s"(d[8]), "s"(args.slots_used), "s"(ra.compact), "s"(ra.slot_px), "s"((int)blockDim.x));
        send = e[0]; desc = d[0];
#pragma unroll
        for (int k = 1; k < 12; k++) { const bool ge = b >= e[k - 1]; slot0 = ge ? e[k - 1] : slot0; send = ge ? e[k] : send; desc = ge ? d[k] : desc; }
    }
    if (args.slots_used > 12) {   // (more than six trackers: the rest of the table)
#pragma unroll
        for (int k = 12; k < kMaxSlots; k++) { const bool ge = b >= args.slot_end[k - 1]; slot0 = ge ? args.slot_end[k - 1] : slot0; send = ge ? args.slot_end[k] : send; desc = ge ? (int)args.slot_desc[k] : desc; }
    }
    const int bx = b - slot0;
    const int model = (int)(desc & 0x7fu);
    if (desc & kResidualSlot) {
        if (ABL(32) || (ABL(16) && args.m[model].cull)) return;  // timing ablations (CF_ICP_REPLAY)
        if (ra.compact) rgb_residual_body<true>(ra, model, bx, send - slot0);
        else rgb_residual_body<false>(ra, model, bx, 0);
        return;
    }
    const IcpModelArgs ma = args.m[model];
    asm volatile("" :: "s"(ma.vc), "s"(ma.nc), "s"(ma.vp), "s"(ma.np), "s"(ma.st), "s"(ma.acc), "s"(ma.err), "s"(ma.occ), "s"(ma.zr), "s"(ma.row_begin), "s"(ma.row_end),
                 "s"(ma.cull), "s"(ma.box_blocks), "s"(args.cols), "s"(args.rows), "s"(args.flags), "s"(args.occ_shift), "s"(args.occ_w), "s"(args.cdiv.M), "s"(args.cdiv.s),
                 "s"(args.row_begin), "s"(args.row_end), "s"(args.intr.fx), "s"(args.intr.fy), "s"(args.intr.cx), "s"(args.intr.cy), "s"(args.angleSqLt), "s"(args.distSqLe));
    if (ABL(256) && !ma.cull) return;  // timing ablation (CF_ICP_REPLAY): unculled models do nothing
    if constexpr (!GRAM) { icp_lds_zero(); __syncthreads(); }   // (behind the argument clause, in front of the first vector load: the waves of a workgroup start together)
    StatePtr st = (StatePtr)ma.st;
    const int cols = args.cols, rows = args.rows, N = cols * rows;
    const int T = blockDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int abl = ABL(7);  // micro-benchmark ablation bits (0 in production)
    unsigned long long v = 0;
    bool gram_has = false, done = false;

    if (ma.box_blocks > 0) {  // culled model, runs of its screen box, one pixel per lane (the launcher: product form, no error surface)
        if (ABL(8)) return;  // timing ablation: culled models do nothing
        const IcpHot hs = icp_hot(st);
        if (!hs.icp || hs.level_done) return;
        const int L = 2 - args.occ_shift;
        const int box[4] = {hs.box[0], hs.box[1], hs.box[2], hs.box[3]};
        const CullRuns cr = cull_runs(box, L, cols, rows);
        if (ABL(512)) return;  // timing ablation (CF_ICP_REPLAY): the cull test alone
        const int wpb = T >> 6, stride = ma.box_blocks * wpb;
        const float rcp = __builtin_amdgcn_rcpf((float)(cr.nrx > 0 ? cr.nrx : 1));
        const float zlo = hs.zlo, zhi = hs.zhi;
#pragma nounroll
        for (int r = bx * wpb + __builtin_amdgcn_readfirstlane(wave); r < cr.total; r += stride) {
            int start;
            bool in_range = true;
            if (cr.nrx > 0) {  // rectangle of runs: r / nrx exactly ((r + 0.5) / nrx is at least 0.5 / nrx away from an integer, r < 2^16)
                const int q = (int)(((float)r + 0.5f) * rcp);
                start = (cr.y0 + q) * cols + ((cr.x0 + (r - q * cr.nrx)) << 6);
            } else {           // runs of the box's rows; a run may straddle rows: the rectangle test of the run's first / last pixel
                start = (cr.y0 + r) << 6;
                const PixBox db = dilated_box(box, L);
                if (span_misses_box(start, min(start + 63, N - 1), cols, args.cdiv, db.x0, db.y0, db.x1, db.y1)) in_range = false;
            }
            // ... and by depth: the run carries the interval of its valid depths (frame_maps_kernel); if it misses the interval the
            // model's dilated box spans in this camera, no pixel of the run can match
            if (in_range && ma.zr) { const float2 zz = ma.zr[start >> 6]; if (!(zz.x <= zhi && zz.y >= zlo)) in_range = false; }
            const int i0 = start + lane;
            if (!icp_run<1, false>(args, ma, st, hs, true, i0, in_range && i0 < N, false, 0, N, nullptr, abl, lane, wave, v, gram_has, done)) return;
            if (done) return;
        }
        if constexpr (!GRAM) icp_lds_commit(lane, wave, T >> 6, ma.acc + (size_t)(bx % kGroups) * 32);
        return;
    }

    // optional row band [row_begin, row_end) (a rank's share when one model's reduction is split over GPUs): of the whole launch
    // (stand-alone band step) or of this model (split background inside the lock-step loop)
    const int rb = ma.row_end > 0 ? ma.row_begin : args.row_begin, re = ma.row_end > 0 ? ma.row_end : args.row_end;
    const int band0 = rb * cols, band1 = (re > 0 ? re : rows) * cols;
    // the error surface (last level-0 iteration) is written for the WHOLE image on every rank of a split model -- the segmentation
    // reads all of it -- while only the band's pixels enter the sums
    // (flags & 1: this launch writes the error surfaces; & 2: ... except those of culled trackers, which icp_error_surface_kernel
    // writes right behind this launch, so that their ICP pass stays culled)
    const bool err_here = (args.flags & 1) && !((args.flags & 2) && ma.cull);
    const bool whole = err_here && ma.err != nullptr && ma.row_end > 0;
    const int pix0 = whole ? 0 : band0, pix1 = whole ? N : band1;
    const int nlog = (pix1 - pix0 + T * PPT - 1) >> __builtin_ctz(T * PPT);  // (workgroup sizes are powers of two: cf_set_icp_launch)
    // (the slot is sized for the whole image; a model with a row band has fewer logical blocks, and the XCD interleave below is a
    // bijection only on the first 8 * ceil(nlog / 8) hardware blocks)
    if ((bx >> 3) >= ((nlog + 7) >> 3)) return;
    // A culled model keeps the workgroups of a few image rows only: giving every XCD a horizontal band would leave that work on
    // the XCDs whose bands the rectangle crosses.  Its workgroups are dealt round-robin instead (neighbouring pixel runs on
    // different XCDs), so what survives the culling is spread over the whole chip.
    const int lb = (ma.cull && !ABL(1024)) ? bx : xcd_logical_block(bx, nlog);  // (1024: timing ablation, bands for everybody)
    if (lb >= nlog) return;
    float* __restrict__ errs = err_here ? ma.err : nullptr;

    const int i0 = pix0 + (lb * T + threadIdx.x) * PPT;
    bool in_range = i0 < pix1;  // cols is a multiple of PPT, so the whole vector is in range
    const bool cull_here = ma.cull && !err_here;
    IcpHot hs{};
    if (cull_here) hs = icp_hot(st);
    // (Measured and dropped, round 3: issuing the plane loads BEFORE the box test, so that in-box waves would not pay the box's scalar
    // round trip in front of them: 22.3 against 21.5 us.)
    // Screen-box culling on the whole-image mapping (Gram form, several pixels per lane, stand-alone steps): a workgroup whose pixel
    // run misses the rectangle leaves after one scalar load; inside a workgroup that straddles it, the waves outside load nothing and
    // go straight to the commit.  Not on the error-surface iteration, which writes every pixel.
    if (cull_here) {
        if (ABL(8)) return;  // timing ablation: culled models do nothing
        const int L = 2 - args.occ_shift;
        const PixBox db = dilated_box(hs.box, L);
        const int p0 = pix0 + lb * T * PPT, p1 = min(p0 + T * PPT, pix1) - 1;  // first / last pixel of this workgroup
        if (span_misses_box(p0, p1, cols, args.cdiv, db.x0, db.y0, db.x1, db.y1)) return;
        const int w0 = p0 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) * 64 * PPT, w1 = min(w0 + 64 * PPT, pix1) - 1;   // ... of this wave
        if (ABL(512)) return;  // timing ablation (CF_ICP_REPLAY): the cull test alone
        if (w0 > w1 || span_misses_box(w0, max(w1, 0), cols, args.cdiv, db.x0, db.y0, db.x1, db.y1)) in_range = false;
        // ... and by depth: the run of 64 pixels this wave owns (per pixel of a lane) carries the interval of its valid depths
        // (frame_maps_kernel); if it misses the interval the model's dilated box spans in this camera, no pixel of the run can match
        if (in_range && ma.zr && w0 <= w1) {
            const float zlo = hs.zlo, zhi = hs.zhi;
            bool any = false;
#pragma unroll
            for (int p = 0; p < PPT; p++) {
                const int c = (w0 >> 6) + p;   // runs are aligned: pix0 == 0 for a culled model, w0 a multiple of 64 * PPT
                if (c * 64 <= w1) { const float2 r = ma.zr[c]; any = any || (r.x <= zhi && r.y >= zlo); }
            }
            if (!any) in_range = false;
        }
    }
    if (!icp_run<PPT, GRAM>(args, ma, st, hs, cull_here, i0, in_range, whole, band0, band1, errs, abl, lane, wave, v, gram_has, done)) return;
    if (done) return;
    if constexpr (GRAM) gram_block_commit(gram_lds, gram_has, lane, wave, T >> 6, ma.acc + (size_t)(lb % kGroups) * 32);
    else icp_lds_commit(lane, wave, T >> 6, ma.acc + (size_t)(lb % kGroups) * 32);
}

#ifdef CF_ABLATE
// diagnostics build: per-workgroup begin / end stamps of one launch (CF_ICP_TRACE, cabi_track.hip) -- [workgroup][4] = begin, end (100 MHz
// constant clock), XCC_ID | HW_ID << 8, 0
__device__ unsigned long long* g_icp_trace = nullptr;
#endif
// (waves_per_eu 6: the register allocator then lands on 71 VGPRs = seven waves per SIMD with the full scalar register file; asked for
// seven it caps the SGPRs at 94 and spills them through VGPR lanes -- 327 against 45 v_readlane / v_writelane in the kernel.)
template <int PPT, int LEVEL_TAG, bool GRAM>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(PPT <= 2 && !GRAM ? 6 : 1))) icp_reduce_kernel(const IcpArgs args, const RgbArgs ra, int n_icp_blocks)
{
#ifdef CF_ABLATE
    unsigned long long* const tr = g_icp_trace;
    unsigned long long t0 = 0;
    if (tr) t0 = wall_clock64();
#endif
    icp_reduce_body<PPT, GRAM>(args, ra, n_icp_blocks);
#ifdef CF_ABLATE
    if (tr) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long t1 = wall_clock64();
            const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u, hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            unsigned long long* o = tr + (size_t)blockIdx.x * 4;
            o[0] = t0; o[1] = t1; o[2] = xcc | ((unsigned long long)hwid << 8); o[3] = 0;
        }
    }
#endif
}

// Where do workgroups land?  The one-XCD meetings (SO(3) pre-alignment, cf_set_gn_mode 2) and the XCD bands rely on hardware workgroup b
// running on XCD b mod 8 (tools/microbench/xcc_map.hip measured it on the MI355X).  The probe states it for the device at hand: 64
// workgroups write their XCC_ID; true iff the first eight are all different and workgroup b repeats workgroup b mod 8's.
__global__ void __launch_bounds__(64) xcc_probe_kernel(unsigned* __restrict__ out)
{
    if (threadIdx.x == 0) out[blockIdx.x] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;   // HW_REG_XCC_ID[3:0]
}
bool probe_xcd_round_robin(hipStream_t s)
{
    unsigned* d = nullptr;
    unsigned h[64];
    if (hipMalloc(reinterpret_cast<void**>(&d), sizeof(h)) != hipSuccess) return false;
    xcc_probe_kernel<<<64, 64, 0, s>>>(d);
    const bool ok = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    (void)hipFree(d);
    if (!ok) return false;
    unsigned seen = 0;
    for (int b = 0; b < 8; b++) seen |= 1u << h[b];
    if (__builtin_popcount(seen) != 8) return false;
    for (int b = 8; b < 64; b++) if (h[b] != h[b & 7]) return false;
    return true;
}

// host side: the f32 bounds that decide "sqrtf(x) < T" and "sqrtf(x) <= T" exactly (sqrtf is correctly rounded, monotonic)
float sqrt_gate_lt(float T)
{   // smallest x with sqrtf(x) >= T  =>  sqrtf(x) < T  <=>  x < bound
    if (!(T > 0.f)) return 0.f;
    float x = T * T;
    while (sqrtf(x) >= T && x > 0.f) x = nextafterf(x, 0.f);
    while (sqrtf(x) < T) x = nextafterf(x, INFINITY);
    return x;
}
float sqrt_gate_le(float T)
{   // largest x with sqrtf(x) <= T  =>  sqrtf(x) <= T  <=>  x <= bound
    if (!(T >= 0.f)) return -1.f;
    if (std::isinf(T)) return INFINITY;  // gate disabled: every radicand passes (x <= inf)
    float x = T * T;
    while (sqrtf(x) <= T && std::isfinite(x)) x = nextafterf(x, INFINITY);
    while (sqrtf(x) > T) x = nextafterf(x, 0.f);
    return x;
}

// ================================================================================================
// RGB residual: RGBResidual::getProducts, reduce.cu:785-865
// ================================================================================================
// The iteration-invariant half of the validity test (window non-zero, gradient magnitude, d1 valid)
// is hoisted into a per-frame candidate mask; the reference re-evaluates it every iteration.
__global__ void __launch_bounds__(256) rgb_cand_kernel(const int16_t* __restrict__ dIdx, const int16_t* __restrict__ dIdy,
                                                       const float* __restrict__ next_depth,
                                                       const uint8_t* __restrict__ next_image, float min_scale, int cols,
                                                       int rows, uint8_t* __restrict__ cand)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= cols * rows) return;
    const int i = k / cols, j0 = k - i * cols;
    uint8_t ok = 0;
    if (j0 < cols - 5 && i < rows - 1) {
        bool valid = true;
        for (int u = max(i - 2, 0); u < min(i + 2, rows); u++)
            for (int v = max(j0 - 2, 0); v < min(j0 + 2, cols); v++) valid = valid && (next_image[u * cols + v] > 0);
        if (valid) {
            const int valx = dIdx[k], valy = dIdy[k];
            const float mTwo = (float)((valx * valx) + (valy * valy));
            if (mTwo >= min_scale && !is_nan(next_depth[k])) ok = 1;
        }
    }
    cand[k] = ok;
}

// One candidate pixel of the residual pass: the pose-dependent half of RGBResidual::getProducts.
// Returns validity; g = flat index of the matched pixel in the last image, diff = next - last intensity.
__device__ __forceinline__ bool rgb_residual_pixel(const RgbArgs& ra, const RgbModelArgs& m, const float* __restrict__ krk,
                                                   const float* __restrict__ kt, int k, float d1, float ni, int& u0, int& v0, float& diff)
{
    const int cols = ra.cols, rows = ra.rows;
    const int y = idiv(k, ra.cdiv), x = k - y * cols;
    const float transformed_d1 = (float)(d1 * (krk[6] * x + krk[7] * y + krk[8]) + kt[2]);
    u0 = f2i_rn((d1 * (krk[0] * x + krk[1] * y + krk[2]) + kt[0]) / transformed_d1);
    v0 = f2i_rn((d1 * (krk[3] * x + krk[4] * y + krk[5]) + kt[1]) / transformed_d1);
    if (u0 >= 0 && v0 >= 0 && u0 < cols && v0 < rows) {
        const float d0 = m.lastDepth[v0 * cols + u0];
        const uint8_t li = m.lastImage[v0 * cols + u0];
        if (d0 > 0 && fabsf(transformed_d1 - d0) <= ra.maxDepthDelta && li != 0) {
            diff = ni - (float)li;
            return true;
        }
    }
    return false;
}

// COMPACT == false: the reference's output format, one DataTerm record per pixel (valid or not), read back by
// rgb_step_kernel -- 16 B/pixel written and re-read although < 10 % of the records are valid.
// COMPACT == true (the device-resident Gauss-Newton loop): four pixels per thread, and the valid correspondences of a
// workgroup are packed into that workgroup's own slot of the record buffer (8 B records, slot = 4 x workgroup size; places
// inside the slot come from LDS atomics, the count goes to slot_counts[workgroup]) -- no global atomic and no extra memory
// round trip on the producer side.  The order inside a slot depends on the schedule, the sums taken over it do not.
//
// Slots of a culled tracker (round 5).  An object model's candidate mask is empty outside its prediction, and until round 5 the
// ~1200 waves per object that found nothing but an empty mask word were 4 800 of the level-0 launch's 16 700.  The preparation now
// records the first and the last 256-pixel chunk with a candidate (RgbModelArgs::res_range); this tracker's `nblk` workgroups -- sized by
// the host from what the previous call saw -- take the slots in between, walking on by nblk when there are more than expected.
// Slots outside hold no record: the RGB step applies the same test instead of reading their (stale) counts.
struct SlotRange { int first, last; };
// (the two words through the constant address space -- the preparation wrote them launches ago --, from a dummy address when the tracker
// has no range, so that the load is unconditional and can share a clause with the hot state's: rgb_hot_and_range)
__device__ __forceinline__ SlotRange residual_slot_range_from(const RgbArgs& ra, bool ranged, unsigned lo_inv, unsigned hi_p1, int n_slots)
{
    if (!ranged) return SlotRange{0, n_slots - 1};
    if (hi_p1 == 0) return SlotRange{0, -1};
    const int sh = __builtin_ctz(ra.slot_px) - 8;                     // slot_px = 4 x workgroup size: a power of two >= 256
    return SlotRange{(int)((~lo_inv) >> sh), min((int)((hi_p1 - 1u) >> sh), n_slots - 1)};
}
__device__ __forceinline__ RgbHot rgb_hot_and_range(const RgbArgs& ra, const RgbModelArgs& m, int n_slots, SlotRange& sr)
{
    StatePtr st = (StatePtr)m.st;
    typedef const __attribute__((address_space(4))) unsigned* U4;
    U4 rp = m.res_range ? (U4)m.res_range : (U4)&st->hot;
    const hot16 l2 = hot_line(st, 2);
    const unsigned lo_inv = rp[0], hi_p1 = rp[1];
    asm volatile("" :: "s"(l2), "s"(lo_inv), "s"(hi_p1));
    sr = residual_slot_range_from(ra, m.res_range != nullptr, lo_inv, hi_p1, n_slots);
    RgbHot h;
    h.rgb = l2[0]; h.rgbOnly = l2[1]; h.level_done = l2[2];
#pragma unroll
    for (int k = 0; k < 9; k++) h.krk[k] = hot_f(l2, 4 + k);
#pragma unroll
    for (int k = 0; k < 3; k++) h.kt[k] = hot_f(l2, 13 + k);
    return h;
}
__device__ __forceinline__ SlotRange residual_slot_range(const RgbArgs& ra, const RgbModelArgs& m, int n_slots)
{
    if (!m.res_range) return SlotRange{0, n_slots - 1};
    const unsigned lo_inv = m.res_range[0], hi_p1 = m.res_range[1];   // (uniform: scalar loads)
    if (hi_p1 == 0) return SlotRange{0, -1};
    const int sh = __builtin_ctz(ra.slot_px) - 8;                     // slot_px = 4 x workgroup size: a power of two >= 256
    return SlotRange{(int)((~lo_inv) >> sh), min((int)((hi_p1 - 1u) >> sh), n_slots - 1)};
}

template <bool COMPACT>
__device__ void rgb_residual_body(const RgbArgs& ra, int model, int blk, int nblk)
{
    const RgbModelArgs m = ra.m[model];   // (one clause of kernel-argument loads: see icp_reduce_body)
    asm volatile("" :: "s"(m.st), "s"(m.cand), "s"(m.nextDepth), "s"(m.lastDepth), "s"(m.lastImage), "s"(m.nextImage), "s"(m.icp_acc), "s"(m.recs), "s"(m.slot_counts),
                 "s"(m.res_range), "s"(m.no_counts), "s"(m.corres), "s"(ra.cols), "s"(ra.rows), "s"(ra.slot_px), "s"(ra.cdiv.M), "s"(ra.cdiv.s), "s"(ra.maxDepthDelta));
    StatePtr st = (StatePtr)m.st;
    const int cols = ra.cols, rows = ra.rows, N = cols * rows;
    const int T = blockDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (!COMPACT) {
        const RgbHot hs = rgb_hot(st);
        if (!hs.rgb || hs.level_done) return;
        const int k = blk * T + threadIdx.x;
        int cnt = 0, sig = 0;
        if (k < N) {
            cf_dataterm c; c.zero_x = c.zero_y = c.one_x = c.one_y = 0; c.diff = 0.f; c.valid = 0;
            if (m.cand[k]) {
                int u0, v0; float diff;
                if (rgb_residual_pixel(ra, m, hs.krk, hs.kt, k, m.nextDepth[k], (float)m.nextImage[k], u0, v0, diff)) {
                    const int y = idiv(k, ra.cdiv), x = k - y * cols;
                    c.zero_x = (int16_t)u0; c.zero_y = (int16_t)v0; c.one_x = (int16_t)x; c.one_y = (int16_t)y;
                    c.diff = diff; c.valid = 1;
                    cnt = 1; sig = (int)(diff * diff);
                }
            }
            *reinterpret_cast<int4*>(&m.corres[k]) = *reinterpret_cast<const int4*>(&c);
        }
        // block reduce (count, sigma) -> grouped atomics into words 29/30 of the ICP accumulator
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); sig += __shfl_xor(sig, o, 64); }
        __shared__ int s_cnt[16], s_sig[16];
        if (lane == 0) { s_cnt[wave] = cnt; s_sig[wave] = sig; }
        __syncthreads();
        if (threadIdx.x == 0) {
            int c4 = 0, g4 = 0;
            for (int w = 0; w < (T >> 6); w++) { c4 += s_cnt[w]; g4 += s_sig[w]; }
            unsigned long long* dst = m.icp_acc + (size_t)(blk % kGroups) * 32;
            if (c4) atomicAdd(&dst[29], (unsigned long long)c4);
            if (g4) atomicAdd(&dst[30], (unsigned long long)(long long)g4);
        }
    } else {
        __shared__ int s_n, s_sig;
        const int n_slots = (N + T * 4 - 1) / (T * 4);
        SlotRange sr;
        const RgbHot hs = rgb_hot_and_range(ra, m, n_slots, sr);   // (one scalar clause for the state and the range)
        const bool on = hs.rgb && !hs.level_done;  // uniform
        if (!on) return;
#pragma nounroll
        for (blk += sr.first; blk <= sr.last; blk += max(nblk, 1)) {
        const int k0 = (blk * T + threadIdx.x) * 4;  // cols % 4 == 0: the four pixels share a row
        unsigned cw = 0;
        if (k0 < N) cw = *reinterpret_cast<const unsigned*>(m.cand + k0);
        if (threadIdx.x == 0) { s_n = 0; s_sig = 0; }
        __syncthreads();
        if (__any(cw != 0)) {
            int g[4], dq[4], nvalid = 0, sig = 0;
            float d1[4] = {0, 0, 0, 0}; unsigned iw = 0;
            if (cw) {
                const float4 dv = *reinterpret_cast<const float4*>(m.nextDepth + k0);
                d1[0] = dv.x; d1[1] = dv.y; d1[2] = dv.z; d1[3] = dv.w;
                iw = *reinterpret_cast<const unsigned*>(m.nextImage + k0);
            }
            // RGBResidual::getProducts (reduce.cu:785-865), the pose-dependent half, in three phases so that the gathers of a thread's four
            // pixels are in flight TOGETHER: until round 5 each pixel ran project -> gather depth -> test -> gather intensity before the
            // next one started -- eight dependent round trips per thread, 6 us per background workgroup (tools/icp_trace_summary.py).
            const int y = idiv(k0, ra.cdiv), x0 = k0 - y * cols;
            float td1[4]; int gi[4]; bool inb[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int x = x0 + p;
                td1[p] = (float)(d1[p] * (hs.krk[6] * x + hs.krk[7] * y + hs.krk[8]) + hs.kt[2]);
                const int u0 = f2i_rn((d1[p] * (hs.krk[0] * x + hs.krk[1] * y + hs.krk[2]) + hs.kt[0]) / td1[p]);
                const int v0 = f2i_rn((d1[p] * (hs.krk[3] * x + hs.krk[4] * y + hs.krk[5]) + hs.kt[1]) / td1[p]);
                inb[p] = ((cw >> (8 * p)) & 0xffu) != 0 && u0 >= 0 && v0 >= 0 && u0 < cols && v0 < rows;
                gi[p] = inb[p] ? v0 * cols + u0 : 0;
            }
            float d0[4]; unsigned li[4];
#pragma unroll
            for (int p = 0; p < 4; p++) { d0[p] = 0.f; li[p] = 0; if (inb[p]) { d0[p] = m.lastDepth[gi[p]]; li[p] = m.lastImage[gi[p]]; } }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                g[p] = -1; dq[p] = 0;
                if (inb[p] && d0[p] > 0 && fabsf(td1[p] - d0[p]) <= ra.maxDepthDelta && li[p] != 0) {
                    const float diff = (float)((iw >> (8 * p)) & 0xffu) - (float)li[p];
                    g[p] = gi[p]; dq[p] = (int)diff;  // next - last intensity: an integer in [-255, 255]
                    nvalid++; sig += (int)(diff * diff);
                }
            }
            int wn = nvalid, ws = sig;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { wn += __shfl_xor(wn, o, 64); ws += __shfl_xor(ws, o, 64); }
            if (wn) {
                int incl = nvalid;  // inclusive prefix of nvalid inside the wave
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                int wbase = 0;
                if (lane == 0) { wbase = atomicAdd(&s_n, wn); atomicAdd(&s_sig, ws); }  // LDS: the wave's place inside the slot
                wbase = __shfl(wbase, 0, 64);
                uint2* __restrict__ out = m.recs + (size_t)blk * T * 4 + wbase + incl - nvalid;
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (g[p] >= 0) { *out++ = make_uint2((unsigned)(k0 + p), (unsigned)g[p] | ((unsigned)(dq[p] + 256) << 22)); }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int bn = s_n, g4 = s_sig;
            m.slot_counts[blk] = (unsigned)bn;  // every workgroup publishes its count: the list pass reads it unconditionally
            unsigned long long* dst = m.icp_acc + (size_t)(blk % kGroups) * 32;
            if (bn && !m.no_counts) atomicAdd(&dst[29], (unsigned long long)bn);
            if (g4 && !m.no_counts) atomicAdd(&dst[30], (unsigned long long)(long long)g4);
        }
        }   // (thread 0 has read s_n / s_sig before it clears them for the next slot; everybody else meets it at the barrier behind that)
    }
}

__global__ void __launch_bounds__(1024) rgb_residual_kernel(const RgbArgs ra) { rgb_residual_body<false>(ra, blockIdx.y, blockIdx.x, 0); }

}  // namespace cf

// the stages behind the {ICP || residual} launch (see the map at the top); they use what is defined above
#include "track_so3_dev.h"
#include "track_solve_dev.h"
#include "track_rgb_step_dev.h"

namespace cf {

// ------------------------------------------------------------------------------ launchers ----
// ev0/ev1 (nullable) receive the dispatch's own begin/end timestamps (the figures rocprofv3 reports), not the
// stream time around it.  n_res_blocks > 0 appends the RGB residual workgroups to the same launch.
#ifdef CF_ABLATE
static IcpArgs g_last_icp_args; static int g_last_n_icp_blocks = 0, g_last_grid = 0;
#endif
static IcpArgs with_cdiv(IcpArgs a) { a.cdiv = make_idiv(a.cols); return a; }
// the instantiations of icp_reduce_kernel, [tag][pixels per lane 1 / 2 / 4][gram]: distinct symbols per pyramid level so that
// rocprofv3 --stats separates them (tag = level for one model, level + 4 for lock-step batches of several models; no tag 3)
typedef void (*IcpKernel)(const IcpArgs, const RgbArgs, int);
#define ICP_TAG(T) {{icp_reduce_kernel<1, T, false>, icp_reduce_kernel<1, T, true>}, {icp_reduce_kernel<2, T, false>, icp_reduce_kernel<2, T, true>}, \
                    {icp_reduce_kernel<4, T, false>, icp_reduce_kernel<4, T, true>}}
static constexpr IcpKernel kIcpKernels[7][3][2] = {ICP_TAG(0), ICP_TAG(1), ICP_TAG(2), {}, ICP_TAG(4), ICP_TAG(5), ICP_TAG(6)};
#undef ICP_TAG
// plain launch when both events are null (also what a stream capture records), hipExtLaunchKernelGGL with the events otherwise
static void launch_plain_or_timed(IcpKernel kernel, dim3 grid, dim3 block, unsigned lds, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const IcpArgs& args,
                              const RgbArgs& ra, int n_icp_blocks)
{
    if (!ev0 && !ev1) kernel<<<grid, block, lds, s>>>(args, ra, n_icp_blocks);
    else hipExtLaunchKernelGGL(kernel, grid, block, lds, s, ev0, ev1, 0, args, ra, n_icp_blocks);
}

static void launch_icp_rgbres(hipStream_t s, IcpLaunch cfg, const IcpArgs& args_in, const RgbArgs& ra_in, bool icp, bool rgb, int n, int level,
                              hipEvent_t ev0, hipEvent_t ev1)
{
    // pixels per lane of unculled trackers, 0 = the library's choice: two at level 0 in the product form -- half the waves of the launch's
    // largest slot for the same loads in flight, 12.4 against 13.0 us with five trackers since the accumulators live in LDS (round 5; with
    // them in registers two pixels cost a wave of occupancy and lost) --, one on the small levels and in the Gram form
    if (cfg.ppt == 0) cfg.ppt = (level == 0 && !cfg.gram) ? 2 : 1;
    const int res_per_block = cfg.threads * (ra_in.compact ? 4 : 1);  // compact list pass: four pixels per thread
    const int n_res_blocks = rgb ? ((icp ? args_in.cols * args_in.rows : ra_in.cols * ra_in.rows) + res_per_block - 1) / res_per_block : 0;
    IcpArgs args = with_cdiv(args_in);
    RgbArgs ra = ra_in; ra.cdiv = make_idiv(ra.cols);
    const int N = ((args.row_end > 0 ? args.row_end : args.rows) - args.row_begin) * args.cols;
    const int per_block = cfg.threads * cfg.ppt;
    const int nlog = (N + per_block - 1) / per_block;
    const int full = icp ? ((nlog + 7) / 8) * 8 : 0;
    // culled models: the workgroups the caller asked for (IcpModelArgs::box_blocks, box_blocks_for), at most the whole image's.  The
    // mapping walks its runs one pixel per lane whatever the launch's pixels per lane are (those apply to unculled models), is built for
    // the product form, and not used on the error-surface iteration (which writes every pixel) nor with row bands.
    int blocks[kMaxBatch];
    for (int m = 0; m < n; m++) {
        IcpModelArgs& ma = args.m[m];
        const bool ok = icp && ma.cull && ma.box_blocks > 0 && !cfg.gram && (!(args.flags & 1) || (args.flags & 2)) && args.row_end == 0 && ma.row_end == 0;
        ma.box_blocks = ok ? (ma.box_blocks < full ? ((ma.box_blocks + 7) / 8) * 8 : full) : 0;
        blocks[m] = ok ? ma.box_blocks : full;
    }
    // residual workgroups: one per record slot of the level, or the caller's RgbModelArgs::res_blocks (culled trackers: the slots between
    // the first and the last candidate the previous call saw, residual_blocks_for)
    int res_compact[kMaxBatch] = {};   // (cf_odom_last_launch_shape: the caller's count where it was taken, 0 where the tracker got one workgroup per slot)
    for (int m = 0; m < n && n_res_blocks > 0; m++) {
        RgbModelArgs& rm = ra.m[m];
        if (!ra.compact || !rm.res_range || rm.res_blocks <= 0 || rm.res_blocks > n_res_blocks) rm.res_blocks = n_res_blocks;
        else res_compact[m] = rm.res_blocks;
        if (!ra.compact) rm.res_range = nullptr;
    }
    if (cfg.shape) {   // cf_odom_last_launch_shape: what was just decided, per tracker (host ints)
        const int L = 2 - args.occ_shift;
        for (int m = 0; m < n; m++) {
            LaunchShape* sh = cfg.shape[m];
            if (!sh || L < 0 || L > 2) continue;
            if (args.flags & 1) sh->icp_err = args.m[m].box_blocks; else sh->icp[L] = args.m[m].box_blocks;
            sh->res[L] = res_compact[m];
        }
    }
    // ORDER OF THE SLOTS = order of dispatch: the culled trackers' runs (the longest chain of dependent round trips: box, depth interval,
    // planes, occupancy, gather), the unculled ICP reductions, then the residual passes.  Seven orders were measured in round 5 (longest work
    // first, residual passes first, ...; profiles/r5v_bench_icp_slot_orders.txt): 13.8-14.0 us for this one, 14.0-14.5 us for the others --
    // the launch is a little over one round of resident workgroups and its length is the sum of everybody's residency, not its tail
    // (tools/icp_trace_summary.py).  Every slot is padded to a multiple of 8 workgroups so that the hardware workgroup id and the
    // slot-local index agree on the XCD; the padding leaves at once.
    int total = 0, slot = 0, n_icp_blocks = 0;
    auto add = [&](int m, bool residual, int count) {
        total += ((count + 7) / 8) * 8;
        args.slot_end[slot] = total; args.slot_desc[slot] = (unsigned char)(m | (residual ? kResidualSlot : 0)); slot++;
        if (!residual) n_icp_blocks += count;
    };
    for (int pass = 0; pass < 2 && icp; pass++) for (int m = 0; m < n; m++) if ((args.m[m].box_blocks > 0) == (pass == 0)) add(m, false, blocks[m]);
    for (int m = 0; m < n && n_res_blocks > 0; m++) add(m, true, ra.m[m].res_blocks);
    args.slots_used = slot;
    for (; slot < kMaxSlots; slot++) { args.slot_end[slot] = 0x7fffffff; args.slot_desc[slot] = 0; }
    const dim3 grid(total);
#ifdef CF_ABLATE
    g_last_icp_args = args; g_last_n_icp_blocks = n_icp_blocks; g_last_grid = (int)grid.x;
#endif
    const unsigned lds = cfg.gram ? (unsigned)(cfg.threads / 64) * kGramWaveDwords * sizeof(int) : 0u;
    const int tag = (level == 0 ? 0 : level == 1 ? 1 : 2) + (n > 1 ? 4 : 0), ppt_index = cfg.ppt == 4 ? 2 : cfg.ppt == 2 ? 1 : 0;
    static_assert(kIcpKernels[3][0][0] == nullptr && kIcpKernels[2][2][1] && kIcpKernels[4][0][0], "tags are level (0..2) or level + 4: row 3 is never looked up");
    launch_plain_or_timed(kIcpKernels[tag][ppt_index][cfg.gram ? 1 : 0], grid, dim3(cfg.threads), lds, s, ev0, ev1, args, ra, n_icp_blocks);
}

void launch_icp_level(hipStream_t s, IcpLaunch cfg, const IcpArgs& args, int n, int level, hipEvent_t ev0, hipEvent_t ev1)
{
    launch_icp_rgbres(s, cfg, args, RgbArgs{}, true, false, n, level, ev0, ev1);
}

// Per Gauss-Newton iteration: ONE launch for {ICP reduction || RGB residual}, then rgbStep, then the one-workgroup
// solve.  Letting rgbStep's last workgroup run the solve was measured twice and lost both times: with a device-scope
// release fence per workgroup (it writes back the XCD's L2: 53 us instead of 6 + 8 us), and with returning atomics +
// a ticket instead of the fence (correct and deterministic, but 946 instead of 1061 frames/s: every workgroup then
// waits for its atomics' round trip).  A third experiment ran the WHOLE 4/5/10 schedule as one persistent launch (256 resident
// workgroups per model, registers carrying the partial sums across a thread's pixels, two grid barriers per iteration built
// from integer atomics + an arrival counter, every workgroup repeating the solve on its own LDS copy of the state): bit-exact
// for all option sets, but 640 us per frame instead of 420 us for the 57 launches -- an in-kernel timer showed ~8 us per
// grid barrier, a chain of about five device-scope memory round trips of ~1.5 us each across the XCDs, whereas a dependent
// launch costs ~2.5 us (tools/microbench/launch_floor.hip).  On this part the kernel boundary IS the cheapest grid barrier.
// Kept as separate launches.
// The first launch of the schedule (so3_prealign_kernel): state hand-over, the SO3 pre-alignment when `so3`, the RGB preparation of
// `prep` beside it.  On its own behind cf_so3_prealign_step.
void launch_so3_prealign(hipStream_t s, const TrackerStates& states, So3Sync* so3_syncs, int n, bool so3, int first_level, const RgbPrepBatch* prep)
{
    const int gx = so3 ? 8 * kSo3Blocks : 1;  // (8x: one XCD per model)
    static const RgbPrepBatch none{};
    const int prep_bx = prep ? prep->m[0].L.blk_end[2] : 0;
    so3_prealign_kernel<<<gx * n + prep_bx * n, 256, 0, s>>>(states, so3_syncs, so3 ? 1 : 0, first_level, gx, gx * n, prep ? *prep : none, prep_bx);
}

// The RGB step over the record slots of ra's level, the grid of either slot mode: 1 -- a workgroup per slot x trackers; 2 -- a workgroup per
// two slots, the tracker's on ONE XCD, the last of them solves (rgb_step_solve_kernel).  For the schedule and for cf_rgb_records_step.
void launch_rgb_slot_step(hipStream_t s, const RgbArgs& ra, So3Sync* so3_syncs, int n, int mode, int icp_fix, int next_level, int last_of_level)
{
    const int N = ra.cols * ra.rows, n_slots = (N + ra.slot_px - 1) / ra.slot_px;
    if (mode == 2) {
        const int n_quads = (n_slots + 1) / 2;
        rgb_step_solve_kernel<<<8 * n_quads * ((n + 7) / 8), 256, 0, s>>>(ra, so3_syncs, n_slots, n_quads, make_idiv(n_quads > 1 ? n_quads : 2), n,
                                                                         icp_fix, next_level, last_of_level);
    } else rgb_slot_step_kernel<<<dim3(n_slots, n), 256, 0, s>>>(ra, n_slots);
}
// The compact residual pass of an rgb_only call on its own (cf_rgb_records_step): the {ICP || residual} launch without its ICP half
void launch_rgb_records_residual(hipStream_t s, IcpLaunch cfg, const RgbArgs& ra_in, int n, int level)
{
    RgbArgs ra = ra_in; ra.compact = 1; ra.slot_px = cfg.threads * 4;
    IcpArgs a{}; a.cols = ra.cols; a.rows = ra.rows;
    launch_icp_rgbres(s, cfg, a, ra, false, true, n, level, nullptr, nullptr);
}

bool launch_gn_track(hipStream_t s, IcpLaunch cfg, const TrackerStates& states, So3Sync* so3_syncs, const GnHook* hook, const IcpArgs icp_args[3],
                     const RgbArgs rgb_args[3], int n, int width, int height, bool so3, bool pyramid, bool fast_odom, bool rgb, bool icp, int mode,
                     ProfSink* prof, OdomDev* const* h_states, const RgbPrepBatch* prep)
{
    int iterations[3];
    iterations[0] = fast_odom ? 3 : 10;
    iterations[1] = pyramid ? 5 : 0;
    iterations[2] = pyramid ? 4 : 0;
    int first_level = 2;
    while (first_level > 0 && iterations[first_level] == 0) first_level--;
    launch_so3_prealign(s, states, so3_syncs, n, so3, first_level, prep);
    GnArgs gn{};
    gn.icp_gram = cfg.gram;
    gn.slot_px = cfg.threads * 4;
    for (int m = 0; m < n; m++) {
        gn.od[m] = const_cast<OdomDev*>(icp_args[0].m[m].st);
        gn.icp_acc[m] = icp_args[0].m[m].acc;
        gn.rgb_acc[m] = rgb_args[0].m[m].rgb_acc;
        gn.od_host[m] = h_states ? h_states[m] : nullptr;
    }
    const bool slots = mode != 0;
    // the error surfaces of the last level-0 iteration: those of culled trackers by a launch of its own behind that iteration's
    // {ICP || residual} launch (these trackers stay culled in their ICP pass: IcpArgs::flags 3), the others by their ICP pass (flags 1)
    bool any_culled = false;
    for (int m = 0; m < n; m++) any_culled = any_culled || (icp_args[0].m[m].cull && icp_args[0].m[m].err);
    const bool err_aside = icp && any_culled;
    bool hook_failed = false;
    for (int i = 2; i >= 0; i--) {
        const int N = (width >> i) * (height >> i);
        for (int j = 0; j < iterations[i]; j++) {
            const bool last_of_level = (j == iterations[i] - 1);
            int next_level = i;
            if (last_of_level) {
                next_level = i - 1;
                while (next_level >= 0 && iterations[next_level] == 0) next_level--;
            }
            RgbArgs ra = rgb_args[i];
            ra.compact = slots ? 1 : 0;
            ra.slot_px = cfg.threads * 4;
            {
                // the roofline figure is quoted on the dominant kernel: the level-0 instantiation
                const bool timed = prof && prof->enabled && i == 0 && prof->used + 4 <= prof->capacity;
                IcpArgs a = icp_args[i];
                a.flags = (i == 0 && last_of_level) ? (err_aside ? 3 : 1) : 0;
                launch_icp_rgbres(s, cfg, a, ra, icp, rgb, n, i, timed ? prof->events[prof->used] : nullptr,
                                  timed ? prof->events[prof->used + 1] : nullptr);
                if (timed) {
                    prof->used += 2;
                    prof->bytes += (uint64_t)N * ((icp ? 24 + 24 * (uint64_t)n : 0) + (rgb ? (slots ? kRgbResidualBytesCompact : kRgbResidualBytes) * (uint64_t)n : 0));
                    prof->launches += 1;
                }
            }
            // (the culled trackers' error surfaces ride in the RGB step's launch when there is one: rgb_slot_step_err_kernel)
            const bool err_here = err_aside && i == 0 && last_of_level;
            const bool err_with_step = err_here && rgb && slots && mode != 2;
            if (err_here && !err_with_step) {
                icp_error_surface_kernel<<<dim3((N + 255) / 256, n), 256, 0, s>>>(with_cdiv(icp_args[i]));
            }
            if (hook && hook->fn) {  // split reductions: the partial sums of this rank's row band become the totals on every rank
                FoldArgs fa{}; int nf = 0;
                for (int m = 0; m < n; m++) if (hook->split[m]) fa.acc[nf++] = gn.icp_acc[m];
                if (nf) acc_fold_kernel<<<nf, 64, 0, s>>>(fa);   // 64 groups -> group 0: 256 bytes per tracker cross the links, not 16 KB
                for (int m = 0; m < n; m++)
                    if (hook->split[m] && hook->fn(hook->user, 0, gn.icp_acc[m], 32, (void*)s) != 0) hook_failed = true;
            }
            if (rgb && mode == 2) {   // the RGB step's last workgroup of every tracker solves
                launch_rgb_slot_step(s, ra, so3_syncs, n, 2, cfg.gram ? -1 : kFixICP, next_level, last_of_level ? 1 : 0);
                continue;
            }
            if (rgb) {
                if (slots) {
                    const int n_slots = (N + ra.slot_px - 1) / ra.slot_px;
                    if (err_with_step) rgb_slot_step_err_kernel<<<dim3(n_slots + (N + 255) / 256, n), 256, 0, s>>>(ra, n_slots, with_cdiv(icp_args[i]));
                    else launch_rgb_slot_step(s, ra, so3_syncs, n, 1, 0, next_level, last_of_level ? 1 : 0);
                }
                else rgb_step_kernel<<<dim3((N + 255) / 256, n), 256, 0, s>>>(ra);
            }
            gn_solve_kernel<<<n, 256, 0, s>>>(gn, next_level, last_of_level ? 1 : 0);
        }
    }
    return !hook_failed;
}

// diagnostics (CF_ICP_REPLAY): the level-0 {ICP || residual} launch of a batch, `reps` times back to back with the given ablation mask;
// returns the average duration in us.  The sums it leaves in the accumulators are garbage: the caller zeroes them.
float replay_icp_level0(hipStream_t s, IcpLaunch cfg, const IcpArgs& a0, const RgbArgs& r0, int n, int slots, int ablate, int reps, hipEvent_t e0, hipEvent_t e1)
{
    IcpArgs a = a0; a.flags = ablate << 8;
    RgbArgs ra = r0; ra.compact = slots ? 1 : 0; ra.slot_px = cfg.threads * 4;
    for (int i = 0; i < 3; i++) launch_icp_rgbres(s, cfg, a, ra, true, true, n, 0, nullptr, nullptr);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < reps; i++) launch_icp_rgbres(s, cfg, a, ra, true, true, n, 0, nullptr, nullptr);
    (void)hipEventRecord(e1, s);
    (void)hipStreamSynchronize(s);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    return ms * 1000.f / reps;
}

#ifdef CF_ABLATE
// diagnostics (CF_SO3_TRACE): the stamps of the last pre-alignment, printed
void trace_so3_dump(hipStream_t s)
{
    (void)hipStreamSynchronize(s);
    unsigned long long h[12][8];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_so3_trace), sizeof(h)) != hipSuccess) return;
    fprintf(stderr, "[so3 trace] loop %lld ns\n", (long long)(h[11][1] - h[11][0]) * 10);
    for (int it = 0; it < 10; it++) {
        if (!h[it][0] || h[it][4] < h[it][0]) continue;
        fprintf(stderr, "[so3 trace] it %d: basis %5lld  pass %5lld  meeting %5lld  solve %5lld ns\n", it, (long long)(h[it][1] - h[it][0]) * 10,
                (long long)(h[it][2] - h[it][1]) * 10, (long long)(h[it][3] - h[it][2]) * 10, (long long)(h[it][4] - h[it][3]) * 10);
    }
    unsigned long long z[12][8] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_so3_trace), z, sizeof(z));
}
// diagnostics (CF_SOLVE_TRACE): phase stamps of tracker 0's solves of the tracking call enqueued between begin and end
static unsigned long long* g_solve_trace_dev = nullptr;
void trace_solve_begin()
{
    if (!g_solve_trace_dev && hipMalloc(reinterpret_cast<void**>(&g_solve_trace_dev), 64 * 16 * 8) != hipSuccess) return;
    (void)hipMemset(g_solve_trace_dev, 0, 64 * 16 * 8);
    const unsigned zero = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_solve_iter), &zero, sizeof(zero));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_solve_trace), &g_solve_trace_dev, sizeof(g_solve_trace_dev));
}
void trace_solve_end(hipStream_t s, const char* path)
{
    (void)hipStreamSynchronize(s);
    unsigned long long* none = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_solve_trace), &none, sizeof(none));
    if (!g_solve_trace_dev) return;
    std::vector<unsigned long long> h(64 * 16);
    (void)hipMemcpy(h.data(), g_solve_trace_dev, h.size() * 8, hipMemcpyDeviceToHost);
    FILE* f = fopen(path, "a");
    if (!f) return;
    fprintf(f, "# solve: ns from the kernel's first stamp -- loaded | totals | unpacked | LDLT | rodrigues | pose | next-iteration | write-back\n");
    for (int it = 0; it < 64; it++) {
        const unsigned long long* o = &h[(size_t)it * 16];
        if (!o[0]) continue;
        fprintf(f, "%2d", it);
        for (int k = 1; k <= 8; k++) fprintf(f, " %6lld", o[k] ? (long long)(o[k] - o[0]) * 10 : -1ll);
        fprintf(f, "\n");
    }
    fclose(f);
}
// diagnostics (CF_STEP_TRACE): one level-0 {ICP || residual} launch + one traced rgb_step_solve_kernel launch (next_level 0: the state moves
// on by one iteration; the caller's results are garbage afterwards); lines "workgroup model begin step commit ticket solve_end" in ns
void trace_step_solve(hipStream_t s, IcpLaunch cfg, const IcpArgs& a0, const RgbArgs& r0, So3Sync* syncs, int n, const char* path)
{
    IcpArgs a = a0; a.flags = 0;
    RgbArgs ra = r0; ra.compact = 1; ra.slot_px = cfg.threads * 4;
    const int N = ra.cols * ra.rows, n_slots = (N + ra.slot_px - 1) / ra.slot_px, n_quads = (n_slots + 1) / 2, grid = 8 * n_quads * ((n + 7) / 8);
    unsigned long long* d = nullptr; unsigned long long* none = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), (size_t)grid * 64) != hipSuccess) return;
    FILE* f = fopen(path, "w");
    for (int rep = 0; rep < 3 && f; rep++) {
        (void)hipMemset(d, 0, (size_t)grid * 64);
        launch_icp_rgbres(s, cfg, a, ra, true, true, n, 0, nullptr, nullptr);
        (void)hipStreamSynchronize(s);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_icp_trace), &d, sizeof(d));
        rgb_step_solve_kernel<<<grid, 256, 0, s>>>(ra, syncs, n_slots, n_quads, make_idiv(n_quads > 1 ? n_quads : 2), n, cfg.gram ? -1 : kFixICP, 0, 0);
        (void)hipStreamSynchronize(s);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_icp_trace), &none, sizeof(none));
        std::vector<unsigned long long> h((size_t)grid * 8);
        (void)hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
        unsigned long long tmin = ~0ull;
        for (int b = 0; b < grid; b++) if (h[(size_t)b * 8] && h[(size_t)b * 8] < tmin) tmin = h[(size_t)b * 8];
        fprintf(f, "# rep %d grid %d trackers %d\n", rep, grid, n);
        for (int b = 0; b < grid; b++) {
            const unsigned long long* o = &h[(size_t)b * 8];
            if (!o[0] || o[5] == 0xffff) continue;
            auto rel = [&](unsigned long long t) { return t ? (long long)(t - tmin) * 10 : -1ll; };
            fprintf(f, "%d %d %lld %lld %lld %lld %lld\n", b, (int)o[5], rel(o[0]), rel(o[1]), rel(o[2]), rel(o[3]), rel(o[4]));
        }
    }
    if (f) fclose(f);
    (void)hipFree(d);
}
// diagnostics (CF_ICP_TRACE): the level-0 {ICP || residual} launch of a batch three times back to back, the third with per-workgroup
// stamps; writes "workgroup kind model begin_ns end_ns xcc hwid" lines (kind: 0 culled ICP, 1 unculled ICP, 2 residual) to `path`
void trace_icp_level0(hipStream_t s, IcpLaunch cfg, const IcpArgs& a0, const RgbArgs& r0, int n, int slots, const char* path)
{
    IcpArgs a = a0; a.flags = 0;
    RgbArgs ra = r0; ra.compact = slots ? 1 : 0; ra.slot_px = cfg.threads * 4;
    unsigned long long* d = nullptr; unsigned long long* none = nullptr;
    const size_t cap = 1u << 16;
    if (hipMalloc(reinterpret_cast<void**>(&d), cap * 32) != hipSuccess) return;
    (void)hipMemset(d, 0, cap * 32);
    for (int i = 0; i < 2; i++) launch_icp_rgbres(s, cfg, a, ra, true, true, n, 0, nullptr, nullptr);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_icp_trace), &d, sizeof(d));
    launch_icp_rgbres(s, cfg, a, ra, true, true, n, 0, nullptr, nullptr);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_icp_trace), &none, sizeof(none));
    std::vector<unsigned long long> h((size_t)g_last_grid * 4);
    (void)hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    FILE* f = fopen(path, "w");
    if (!f) return;
    unsigned long long tmin = ~0ull;
    for (int b = 0; b < g_last_grid; b++) if (h[(size_t)b * 4] && h[(size_t)b * 4] < tmin) tmin = h[(size_t)b * 4];
    fprintf(f, "# grid %d icp_blocks %d trackers %d\n", g_last_grid, g_last_n_icp_blocks, n);
    for (int b = 0; b < g_last_grid; b++) {
        int slot = 0; while (slot < kMaxSlots - 1 && b >= g_last_icp_args.slot_end[slot]) slot++;
        const int model = g_last_icp_args.slot_desc[slot] & 0x7f;
        const int kind = (g_last_icp_args.slot_desc[slot] & kResidualSlot) ? 2 : (g_last_icp_args.m[model].box_blocks > 0 ? 0 : 1);
        const unsigned long long* o = &h[(size_t)b * 4];
        fprintf(f, "%d %d %d %lld %lld %u %u\n", b, kind, model, (long long)(o[0] - tmin) * 10, (long long)(o[1] - tmin) * 10, (unsigned)(o[2] & 255u), (unsigned)(o[2] >> 8));
    }
    fclose(f);
}
#endif

// ---- stand-alone steps (C-ABI parity with computeRgbResidual / rgbStep) -------------------
void launch_rgb_residual(hipStream_t s, const RgbArgs& ra, int n)
{
    const int N = ra.cols * ra.rows;
    RgbArgs a = ra; a.compact = 0; a.cdiv = make_idiv(a.cols);
    rgb_residual_kernel<<<dim3((N + 255) / 256, n), 256, 0, s>>>(a);
}
void launch_rgb_step(hipStream_t s, const RgbArgs& ra, int n)
{
    const int N = ra.cols * ra.rows;
    rgb_step_kernel<<<dim3((N + 255) / 256, n), 256, 0, s>>>(ra);
}
void launch_gn_solve(hipStream_t s, const GnArgs& gn, int n, int next_level, int last_of_level)
{
    gn_solve_kernel<<<n, 256, 0, s>>>(gn, next_level, last_of_level ? 1 : 0);
}
void launch_acc_total(hipStream_t s, const unsigned long long* acc, unsigned long long* out)
{
    acc_total_kernel<<<1, 64, 0, s>>>(acc, out);
}
void launch_rgb_cand(hipStream_t s, const int16_t* dIdx, const int16_t* dIdy, const float* next_depth,
                     const uint8_t* next_image, float min_scale, int cols, int rows, uint8_t* cand)
{
    rgb_cand_kernel<<<(cols * rows + 255) / 256, 256, 0, s>>>(dIdx, dIdy, next_depth, next_image, min_scale, cols, rows, cand);
}
void launch_so3_step(hipStream_t s, const uint8_t* last_image, const uint8_t* next_image, const float basis[9],
                     const float kinv[9], const float krlr[9], int cols, int rows, unsigned long long* out16)
{
    m33 B, Ki, Kr;
    for (int i = 0; i < 9; i++) { B.m[i] = basis[i]; Ki.m[i] = kinv[i]; Kr.m[i] = krlr[i]; }
    so3_step_kernel<<<1, 1024, 0, s>>>(last_image, next_image, B, Ki, Kr, cols, rows, out16);
}

}  // namespace cf
