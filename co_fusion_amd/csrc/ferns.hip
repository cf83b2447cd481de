// ferns.hip -- device-resident random-fern keyframe database (Core/Ferns.cpp, ElasticFusion's relocaliser): encode a frame's fill-in
// maps into fern codes, scan the database for the most similar keyframes, append on the device, and relocalise against the match
// with the small tracker.  DESIGN.md section 4.8 states the conventions (sampling, code bits, row layout, tie rules).  The loop-closure
// seam (include/cofusion_loop.h): a per-frame gate behind the scan, and the candidate part of Ferns::findFrame
// (photometric check, accept rule, surface constraints) on the device.
//
// Database layout (HBM, all sized by `capacity` at creation):
//   codes  u8  [capacity][row_bytes]   one byte per fern, row padded with 255 to a multiple of 16 B (a row is whole uint4 loads)
//   good   i32 [capacity]              codes != 255 of the keyframe
//   time   i32 [capacity]              srcTime
//   pose   f32 [capacity][16]
//   vmap / nmap f32 [capacity][3 * rw * rh]   reduced maps, planar (what cf_odom_bind_frame_maps takes; z == 0 -> NaN like copyMaps)
//   rgb    u8  [capacity][rw * rh * 3]
// plus one "current" slot of the same shape, the per-keyframe co-occurrences of the last search, and a small state block (count, the
// two armed minima, the published results).  The host never needs the count to enqueue: it sizes the scan by the number of appends
// it has enqueued so far (an upper bound) and the kernels read the real count from the state block.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cf_device.h"
#include "cf_host.h"

using namespace cf;

namespace {

constexpr unsigned long long kArmed = ~0ull;
constexpr int kSearchBlock = 256;   // four waves
constexpr int kMaxSearchGrid = 512;    // two workgroups per CU of a 256-CU device; the scan strides over the rest

struct FernState {
    unsigned long long key_all, key_match;   // running minima of the scan: f32 bits of the dissimilarity << 32 | keyframe; kArmed between scans
    unsigned ticket_search, ticket_append;
    int count;                               // keyframes in the database
    int full;                                // an append was wanted at count == capacity
    int good_cur;                            // good codes of the current slot
    int appended;                            // decision of the last cf_ferns_add_async
    float min_all, min_match;                // published by the last scan (FLT_MAX: none)
    int match_id;                            // ... -1: none
    int searched;                            // ... the count it scanned
};

struct FernsDev {
    const cf_fern* table;
    uint8_t *codes, *cur_codes, *rgb, *cur_rgb;
    int *good, *time, *co;
    float *pose, *vmap, *nmap, *cur_v, *cur_n;
    FernState* state;
    int n, row_bytes, row16, lanes, lane_shift;   // lanes: lanes of a wave that share one keyframe (power of two <= 64)
    int W, H, rw, rh, npx, capacity;
};

// ---- encode: 8x reduction with nearest sampling at source texel (8x + 4, 8y + 4) and the fern codes, one launch.  Block 0 evaluates
// the ferns (a fern's reduced pixel IS the source texel, so it does not wait for the other blocks), blocks 1.. write the reduced maps.
__global__ void __launch_bounds__(256) ferns_encode_kernel(const FernsDev d, const float4* __restrict__ v4, const float4* __restrict__ n4,
                                                           const uchar4* __restrict__ rgba)
{
    if (blockIdx.x == 0) {
        __shared__ int wave_good[4];
        int good = 0;
        for (int i = threadIdx.x; i < d.row_bytes; i += 256) {
            unsigned code = 255u;   // badCode, and the padding of the row
            if (i < d.n) {
                const cf_fern f = d.table[i];
                const size_t src = (size_t)(8 * f.y + 4) * d.W + (8 * f.x + 4);
                const float z = v4[src].z;
                if (z > 0) {   // Ferns.cpp:92-99
                    const uchar4 pix = rgba[src];
                    code = (unsigned)((int)pix.x > f.r) << 3 | (unsigned)((int)pix.y > f.g) << 2 | (unsigned)((int)pix.z > f.b) << 1 |
                           (unsigned)((int)(z * 1000.0f) > f.d);
                    good++;
                }
            }
            d.cur_codes[i] = (uint8_t)code;
        }
        for (int o = 32; o; o >>= 1) good += __shfl_xor(good, o, 64);
        if ((threadIdx.x & 63) == 0) wave_good[threadIdx.x >> 6] = good;
        __syncthreads();
        if (threadIdx.x == 0) d.state->good_cur = wave_good[0] + wave_good[1] + wave_good[2] + wave_good[3];
        return;
    }
    const int p = (blockIdx.x - 1) * 256 + threadIdx.x;
    if (p >= d.npx) return;
    const int y = p / d.rw, x = p - y * d.rw;
    const size_t src = (size_t)(8 * y + 4) * d.W + (8 * x + 4);
    const float4 vs = v4[src], ns = n4[src];
    const uchar4 c = rgba[src];
    float vx = qnan(), vy = vx, vz = vx, nx = vx, ny = vx, nz = vx;   // copyMaps: z == 0 -> NaN in all planes
    if (!(vs.z == 0)) { vx = vs.x; vy = vs.y; vz = vs.z; nx = ns.x; ny = ns.y; nz = ns.z; }
    d.cur_v[p] = vx; d.cur_v[p + d.npx] = vy; d.cur_v[p + 2 * d.npx] = vz;
    d.cur_n[p] = nx; d.cur_n[p + d.npx] = ny; d.cur_n[p + 2 * d.npx] = nz;
    d.cur_rgb[3 * p] = c.x; d.cur_rgb[3 * p + 1] = c.y; d.cur_rgb[3 * p + 2] = c.z;
}

// bytes of `c` equal to the byte of `q` at positions where `qm` has 0x80 (q != 255): four at a time.
__device__ __forceinline__ int eq_bytes(unsigned q, unsigned qm, unsigned c)
{
    const unsigned x = q ^ c;
    const unsigned nz = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;   // bit 7 of a byte set <=> the byte of x is non-zero
    return __popc(~nz & qm);
}
__device__ __forceinline__ unsigned good_mask(unsigned q)
{   // 0x80 in every byte of q that is not 255
    const unsigned x = ~q;   // byte == 0 <=> code 255
    return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}
__device__ __forceinline__ int eq_bytes16(const uint4& q, const uint4& qm, const uint4& c)
{
    return eq_bytes(q.x, qm.x, c.x) + eq_bytes(q.y, qm.y, c.y) + eq_bytes(q.z, qm.z, c.z) + eq_bytes(q.w, qm.w, c.w);
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o)
{
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    return (unsigned long long)hi << 32 | lo;
}

// ---- search: ONE pass over the code rows.  `lanes` lanes of a wave share a keyframe (32 for 500 ferns: two keyframes per wave and
// trip), each lane holds its 16 B piece(s) of the query and of the query's good mask in registers for the whole scan, loads the same
// piece of the keyframe's row with one 16 B load, counts equal good bytes four at a time, and the pieces are summed with xor
// shuffles.  Rows are at most 128 pieces (2048 ferns), so a lane holds at most two.  The minima travel as 64-bit keys (f32 bits of
// a non-negative float order like the float; the keyframe in the low word makes the lowest index win ties): a running minimum per
// lane, one wave reduction, one LDS step and one pair of atomics per workgroup at the end.  The last workgroup to finish publishes the results and re-arms the
// accumulators and its own ticket, so the scan needs no launch before or after it.
// Visibility ACROSS launches (count and good_cur read here with plain loads, co[] and the published results written with plain stores)
// rests on stream order alone: encode, search and append of one object go to one stream; only the minima and the ticket are atomics.
__global__ void __launch_bounds__(kSearchBlock) ferns_search_kernel(const FernsDev d, int time, int min_age)
{
    FernState* st = d.state;
    const int count = st->count, good_q = st->good_cur;
    const int lane = threadIdx.x & 63, sub = lane & (d.lanes - 1), grp = lane >> d.lane_shift;
    const int per_wave = 64 >> d.lane_shift;
    const int wave = blockIdx.x * (kSearchBlock / 64) + (threadIdx.x >> 6), waves = gridDim.x * (kSearchBlock / 64);
    const uint4* qrow = reinterpret_cast<const uint4*>(d.cur_codes);
    const bool has0 = sub < d.row16, has1 = sub + d.lanes < d.row16;
    uint4 q0 = make_uint4(~0u, ~0u, ~0u, ~0u), q1 = q0;
    if (has0) q0 = qrow[sub];
    if (has1) q1 = qrow[sub + d.lanes];
    const uint4 m0 = make_uint4(good_mask(q0.x), good_mask(q0.y), good_mask(q0.z), good_mask(q0.w));
    const uint4 m1 = make_uint4(good_mask(q1.x), good_mask(q1.y), good_mask(q1.z), good_mask(q1.w));
    unsigned long long best_all = kArmed, best_match = kArmed;
    for (int kb = wave * per_wave; kb < count; kb += waves * per_wave) {   // (uniform per wave: every lane takes part in the shuffles)
        const int k = kb + grp;
        const bool valid = k < count;
        int co = 0;
        if (valid) {
            const uint4* row = reinterpret_cast<const uint4*>(d.codes + (size_t)k * d.row_bytes);
            if (has0) co = eq_bytes16(q0, m0, row[sub]);
            if (has1) co += eq_bytes16(q1, m1, row[sub + d.lanes]);
        }
        for (int o = d.lanes >> 1; o; o >>= 1) co += __shfl_xor(co, o, 64);
        if (valid && sub == 0) {
            d.co[k] = co;
            const int gk = d.good[k];
            const int max_co = good_q < gk ? good_q : gk;   // Ferns.cpp:115-117 / 188-190
            if (max_co > 0) {
                const float dissim = (float)(max_co - co) / (float)max_co;
                const unsigned long long key = (unsigned long long)__float_as_uint(dissim) << 32 | (unsigned)k;
                if (key < best_all) best_all = key;
                if (time - d.time[k] > min_age && key < best_match) best_match = key;
            }
        }
    }
    for (int o = 32; o; o >>= 1) {
        const unsigned long long a = shfl_xor_u64(best_all, o), b = shfl_xor_u64(best_match, o);
        if (a < best_all) best_all = a;
        if (b < best_match) best_match = b;
    }
    // one pair of atomics per workgroup: ten thousand waves hitting the same two words one after another cost more than the scan itself
    __shared__ unsigned long long wave_all[kSearchBlock / 64], wave_match[kSearchBlock / 64];
    if (lane == 0) { wave_all[threadIdx.x >> 6] = best_all; wave_match[threadIdx.x >> 6] = best_match; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kSearchBlock / 64; w++) {
            if (wave_all[w] < best_all) best_all = wave_all[w];
            if (wave_match[w] < best_match) best_match = wave_match[w];
        }
        if (best_all != kArmed) atomicMin(&st->key_all, best_all);
        if (best_match != kArmed) atomicMin(&st->key_match, best_match);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&st->ticket_search, 1u) == gridDim.x - 1) {
            __threadfence();
            const unsigned long long ka = atomicExch(&st->key_all, kArmed), km = atomicExch(&st->key_match, kArmed);
            st->min_all = ka == kArmed ? 3.402823466e+38f : __uint_as_float((unsigned)(ka >> 32));
            st->min_match = km == kArmed ? 3.402823466e+38f : __uint_as_float((unsigned)(km >> 32));
            st->match_id = km == kArmed ? -1 : (int)(unsigned)km;
            st->searched = count;
            st->ticket_search = 0;
        }
    }
}

struct PoseArg { float m[16]; };

// ---- conditional append (Ferns.cpp:127): every workgroup reads the decision's inputs, copies its share of the current slot into
// slot `count`, and the last one to finish moves the count.
__global__ void __launch_bounds__(256) ferns_append_kernel(const FernsDev d, const PoseArg pose, int src_time, float threshold)
{
    FernState* st = d.state;
    const int count = st->count, good = st->good_cur;
    const float minimum = st->min_all;
    const bool want = (minimum > threshold || count == 0) && good > 0;
    const bool go = want && count < d.capacity;
    if (go) {
        const int c16 = d.row16, m16 = d.npx * 3 / 4, r16 = d.npx * 3 / 16;   // uint4 pieces of a code row, a planar map, the rgb image
        const uint4* sc = reinterpret_cast<const uint4*>(d.cur_codes);
        const uint4* sv = reinterpret_cast<const uint4*>(d.cur_v);
        const uint4* sn = reinterpret_cast<const uint4*>(d.cur_n);
        const uint4* sr = reinterpret_cast<const uint4*>(d.cur_rgb);
        uint4* dc = reinterpret_cast<uint4*>(d.codes + (size_t)count * d.row_bytes);
        uint4* dv = reinterpret_cast<uint4*>(d.vmap + (size_t)count * d.npx * 3);
        uint4* dn = reinterpret_cast<uint4*>(d.nmap + (size_t)count * d.npx * 3);
        uint4* dr = reinterpret_cast<uint4*>(d.rgb + (size_t)count * d.npx * 3);
        const int total = c16 + 2 * m16 + r16;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
            if (i < c16) dc[i] = sc[i];
            else if (i < c16 + m16) dv[i - c16] = sv[i - c16];
            else if (i < c16 + 2 * m16) dn[i - c16 - m16] = sn[i - c16 - m16];
            else dr[i - c16 - 2 * m16] = sr[i - c16 - 2 * m16];
        }
        if (blockIdx.x == 0 && threadIdx.x < 16) d.pose[(size_t)count * 16 + threadIdx.x] = pose.m[threadIdx.x];
        if (blockIdx.x == 0 && threadIdx.x == 16) { d.good[count] = good; d.time[count] = src_time; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&st->ticket_append, 1u) == gridDim.x - 1) {   // every workgroup has read `count` by now
            st->appended = go ? 1 : 0;
            if (want && !go) st->full = 1;
            if (go) st->count = count + 1;
            st->ticket_append = 0;
        }
    }
}

// planar reduced maps of a keyframe -> the RGBA32F images cf_odom_init_icp_model takes (NaN, i.e. z == 0 at encode time, -> zeros)
__global__ void __launch_bounds__(256) ferns_planar_to_x4_kernel(const float* __restrict__ v, const float* __restrict__ n, int npx,
                                                                 float4* __restrict__ v4, float4* __restrict__ n4)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const float z = v[p + 2 * npx];
    float4 a = make_float4(0, 0, 0, 0), b = a;
    if (!is_nan(z)) { a = make_float4(v[p], v[p + npx], z, 0); b = make_float4(n[p], n[p + npx], n[p + 2 * npx], 0); }
    v4[p] = a; n4[p] = b;
}

// ---- gate (loop closure, every tracked frame): blockHDAware (Ferns.cpp:321-336) of the current codes against the published match's
// row, one wave: a lane takes 16 B pieces of both rows, counts the ferns good in both and those of them with equal codes four at a
// time, xor shuffles sum the pieces.  The padding of a row is 255 in both and counts in neither.  The record goes to PINNED memory
// with plain stores, a system-scope fence, and the serial last: the host reads nothing else to learn of a candidate.
__global__ void __launch_bounds__(64) ferns_gate_kernel(const FernsDev d, unsigned serial, cf_ferns_gate* __restrict__ rec)
{
    const FernState* st = d.state;
    const int id = st->match_id, lane = threadIdx.x;
    int count = 0, val = 0;
    if (id >= 0) {   // (uniform)
        const uint4* qrow = reinterpret_cast<const uint4*>(d.cur_codes);
        const uint4* krow = reinterpret_cast<const uint4*>(d.codes + (size_t)id * d.row_bytes);
        for (int p = lane; p < d.row16; p += 64) {
            const uint4 q = qrow[p], c = krow[p];
            const uint4 m = make_uint4(good_mask(q.x) & good_mask(c.x), good_mask(q.y) & good_mask(c.y), good_mask(q.z) & good_mask(c.z),
                                       good_mask(q.w) & good_mask(c.w));
            count += __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
            val += eq_bytes16(q, m, c);
        }
        for (int o = 32; o; o >>= 1) { count += __shfl_xor(count, o, 64); val += __shfl_xor(val, o, 64); }
    }
    if (lane == 0) {
        rec->match_id = id;
        rec->dissimilarity = st->min_match;
        rec->overlap = id >= 0 ? (float)val / (float)count : 0.0f;   // 0 / 0 -> NaN: no candidate
        rec->good_q = st->good_cur;
        rec->keyframe_time = id >= 0 ? d.time[id] : 0;
        rec->count = count;
        rec->keyframes = st->searched;
        __threadfence_system();
        rec->serial = serial;
    }
}

// ---- the candidate part of Ferns::findFrame (Ferns.cpp:231-256) on the device, one workgroup of 256.
struct CloseArgs {
    float curr[16], est[16];
    float icp_error, icp_count, photo_threshold;
    float fx, fy, cx, cy;   // of the reduced frame
    int keyframe, lost, time, max_depth_mm;
    int samples_ok;         // the fern count fits CF_FERNS_MAX_SAMPLES (else no constraints are written)
};
struct ConsBuffers { float *src, *dst, *time; };   // f32 [128][3], [128][3], [128]

__device__ __forceinline__ float3 mul_pose(const float* m, float x, float y, float z)
{
    return make_float3(((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
                       ((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
}

// (a) photometricCheck (Ferns.cpp:264-307) as the host block of cf_ferns_relocalise states it: f64 from the f32 inputs, the same
// association (the build has no FMA contraction), truncation towards zero; sum and count are integers, reduced exactly.  (b) the accept
// rule.  (c) when accepted and not lost, wave 0 takes the samples i = lane * (n / 50), compacts the valid ones IN ORDER with a ballot and
// the count of valid lanes below, and writes a constraint row and its pin per valid sample.
__global__ void __launch_bounds__(256) ferns_close_kernel(const FernsDev d, const CloseArgs a, const ConsBuffers cons, cf_ferns_closure* __restrict__ out)
{
    __shared__ int wave_sum[4], wave_cnt[4];
    __shared__ int s_accept;
    const int tid = threadIdx.x, id = a.keyframe;
    const size_t npx = (size_t)d.npx;
    const bool have = id >= 0 && id < d.state->count;
    int sum = 0, cnt = 0;   // (at most 2048 ferns x 765: no overflow)
    if (have) {
        const float* F = d.pose + (size_t)id * 16;
        const float* P = a.est;
        const double fx = (double)a.fx, fy = (double)a.fy, cx = (double)a.cx, cy = (double)a.cy;
        double Rd[9], td[3];   // [R^T R', R^T (t' - t)]: fernPose^-1 * estPose
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++)
                Rd[i * 3 + j] = ((double)F[0 * 4 + i] * (double)P[0 * 4 + j] + (double)F[1 * 4 + i] * (double)P[1 * 4 + j]) +
                                (double)F[2 * 4 + i] * (double)P[2 * 4 + j];
            td[i] = ((double)F[0 * 4 + i] * ((double)P[3] - (double)F[3]) + (double)F[1 * 4 + i] * ((double)P[7] - (double)F[7])) +
                    (double)F[2 * 4 + i] * ((double)P[11] - (double)F[11]);
        }
        const uint8_t* krgb = d.rgb + (size_t)id * npx * 3;
        for (int i = tid; i < d.n; i += 256) {
            const cf_fern t = d.table[i];
            const size_t p = (size_t)t.y * d.rw + t.x;
            const float z = d.cur_v[p + 2 * npx];
            if (!(z > 0) || !((int)(z * 1000.0f) < a.max_depth_mm)) continue;
            const double x = (double)d.cur_v[p], y = (double)d.cur_v[p + npx], zz = (double)z;
            const double wx = ((Rd[0] * x + Rd[1] * y) + Rd[2] * zz) + td[0];
            const double wy = ((Rd[3] * x + Rd[4] * y) + Rd[5] * zz) + td[1];
            const double wz = ((Rd[6] * x + Rd[7] * y) + Rd[8] * zz) + td[2];
            const double u = wx * fx / wz + cx, v = wy * fy / wz + cy;
            if (!(fabs(u) < 1e9) || !(fabs(v) < 1e9)) continue;   // (not finite or far outside: no correspondence)
            const int iu = (int)u, iv = (int)v;                   // truncation towards zero
            if (iu < 0 || iv < 0 || iu >= d.rw || iv >= d.rh) continue;
            const uint8_t* kp = krgb + ((size_t)iv * d.rw + iu) * 3;
            const int k0 = kp[0], k1 = kp[1], k2 = kp[2];
            if (!(k0 > 0 || k1 > 0 || k2 > 0)) continue;
            const uint8_t* cp = d.cur_rgb + p * 3;
            sum += abs(k0 - (int)cp[0]) + abs(k1 - (int)cp[1]) + abs(k2 - (int)cp[2]);
            cnt++;
        }
    }
    for (int o = 32; o; o >>= 1) { sum += __shfl_xor(sum, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    if ((tid & 63) == 0) { wave_sum[tid >> 6] = sum; wave_cnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        sum = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
        cnt = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
        const double photo = cnt ? (double)sum / (double)cnt : (double)INFINITY;
        const int thresh = a.lost ? 1400 : 2400;
        const int accepted = have && (double)a.icp_error < 0.0003 && a.icp_count > (float)thresh && photo < (double)a.photo_threshold;
        s_accept = accepted;
        out->accepted = accepted;
        out->photo_sum = sum; out->photo_count = cnt; out->photo_error = photo;
        out->keyframe = have ? id : -1;
        out->keyframe_time = have ? d.time[id] : 0;
        out->icp_error = a.icp_error; out->icp_count = a.icp_count;
    }
    __syncthreads();
    if (tid >= 64) return;
    int rows = 0;
    if (s_accept && !a.lost && a.samples_ok) {   // (uniform: the whole wave takes part in the ballot)
        const int step = d.n / 50;               // Ferns.cpp:240 (samples_ok: step >= 1 and at most 64 samples)
        const long long i = (long long)tid * step;
        bool valid = false;
        float x = 0, y = 0, z = 0;
        if (i < d.n) {
            const cf_fern t = d.table[i];
            const size_t p = (size_t)t.y * d.rw + t.x;
            z = d.cur_v[p + 2 * npx];
            valid = z > 0 && (int)(z * 1000.0f) < a.max_depth_mm;   // NaN z: invalid
            if (valid) { x = d.cur_v[p]; y = d.cur_v[p + npx]; }
        }
        const unsigned long long mask = __ballot(valid);
        rows = 2 * __popcll(mask);
        if (valid) {
            const int j = __popcll(mask & ((1ull << tid) - 1ull));
            const float3 raw = mul_pose(a.curr, x, y, z), model = mul_pose(a.est, x, y, z);
            float* s = cons.src + 6 * j; float* t = cons.dst + 6 * j;
            s[0] = raw.x; s[1] = raw.y; s[2] = raw.z; t[0] = model.x; t[1] = model.y; t[2] = model.z;
            s[3] = model.x; s[4] = model.y; s[5] = model.z; t[3] = model.x; t[4] = model.y; t[5] = model.z;
            cons.time[2 * j] = (float)a.time;
            cons.time[2 * j + 1] = (float)d.time[id];
        }
    }
    if (tid == 0) out->n_constraints = rows;
}

}  // namespace

struct cf_ferns {
    cf_ctx* ctx = nullptr;
    cf_ctx* small = nullptr;       // (W/8) x (H/8) context of the relocalisation tracker, enqueueing on the parent's stream
    cf_odom* odom = nullptr;
    cf_ferns_config cfg{};
    FernsDev d{};
    cf_fern* d_table = nullptr;
    float *kf_v4 = nullptr, *kf_n4 = nullptr;   // the matched keyframe's maps as RGBA32F (model side of the tracker)
    FernState* h_state = nullptr;               // pinned
    std::vector<cf_fern> table;
    long long adds_enqueued = 0;                // upper bound of the device-side count
    // the loop-closure seam
    cf_ferns_gate* h_gate = nullptr;            // pinned: written by ferns_gate_kernel
    cf_ferns_closure* h_close = nullptr;        // pinned: written by ferns_close_kernel
    ConsBuffers cons{};
    hipEvent_t gate_event = nullptr;
    unsigned gate_serial = 0;                   // of the last cf_ferns_gate_async
    bool gate_pending = false;
    cf_ferns_gate gate{};                       // what the last cf_ferns_gate_wait read
    bool gated = false;
};

static uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int search_grid(const cf_ferns* f)
{
    long long ub = f->adds_enqueued < f->cfg.capacity ? f->adds_enqueued : f->cfg.capacity;
    const int per_block = (kSearchBlock / 64) * (64 >> f->d.lane_shift);
    long long g = (ub + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : g > kMaxSearchGrid ? kMaxSearchGrid : g);
}

static int fetch_state(cf_ferns* f)
{
    cf_ctx* ctx = f->ctx;
    hipStream_t s = ctx->cur();   // the stream the kernels of the calling thread went to (a lane after cf_fork / cf_thread_lane)
    HIPCHK(ctx, hipMemcpyAsync(f->h_state, f->d.state, sizeof(FernState), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return CF_OK;
}

// every allocation of the object (the caller destroys it when this fails)
static int ferns_build(cf_ctx* ctx, cf_ferns* f)
{
    const int W = ctx->cfg.width, H = ctx->cfg.height, rw = W / 8, rh = H / 8;
    FernsDev& d = f->d;
    d.n = f->cfg.n_ferns; d.row_bytes = (f->cfg.n_ferns + 15) / 16 * 16; d.row16 = d.row_bytes / 16;
    d.lanes = 1; d.lane_shift = 0;
    while (d.lanes < d.row16 && d.lanes < 64) { d.lanes <<= 1; d.lane_shift++; }
    d.W = W; d.H = H; d.rw = rw; d.rh = rh; d.npx = rw * rh; d.capacity = f->cfg.capacity;
    const size_t cap = (size_t)f->cfg.capacity, npx = (size_t)d.npx;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMalloc((void**)&f->d_table, sizeof(cf_fern) * f->table.size()));
    HIPCHK(ctx, hipMemcpyAsync(f->d_table, f->table.data(), sizeof(cf_fern) * f->table.size(), hipMemcpyHostToDevice, s));
    d.table = f->d_table;
    HIPCHK(ctx, hipMalloc((void**)&d.codes, cap * d.row_bytes));
    HIPCHK(ctx, hipMalloc((void**)&d.cur_codes, (size_t)d.row_bytes));
    HIPCHK(ctx, hipMemsetAsync(d.cur_codes, 255, (size_t)d.row_bytes, s));
    HIPCHK(ctx, hipMalloc((void**)&d.good, cap * sizeof(int)));
    HIPCHK(ctx, hipMalloc((void**)&d.time, cap * sizeof(int)));
    HIPCHK(ctx, hipMalloc((void**)&d.co, cap * sizeof(int)));
    HIPCHK(ctx, hipMemsetAsync(d.co, 0, cap * sizeof(int), s));
    HIPCHK(ctx, hipMalloc((void**)&d.pose, cap * 16 * sizeof(float)));
    HIPCHK(ctx, hipMalloc((void**)&d.vmap, cap * npx * 3 * sizeof(float)));
    HIPCHK(ctx, hipMalloc((void**)&d.nmap, cap * npx * 3 * sizeof(float)));
    HIPCHK(ctx, hipMalloc((void**)&d.rgb, cap * npx * 3));
    HIPCHK(ctx, hipMalloc((void**)&d.cur_v, npx * 3 * sizeof(float)));
    HIPCHK(ctx, hipMalloc((void**)&d.cur_n, npx * 3 * sizeof(float)));
    HIPCHK(ctx, hipMalloc((void**)&d.cur_rgb, npx * 3));
    HIPCHK(ctx, hipMemsetAsync(d.cur_v, 0, npx * 3 * sizeof(float), s));
    HIPCHK(ctx, hipMemsetAsync(d.cur_n, 0, npx * 3 * sizeof(float), s));
    HIPCHK(ctx, hipMemsetAsync(d.cur_rgb, 0, npx * 3, s));
    HIPCHK(ctx, hipMalloc((void**)&f->kf_v4, npx * 4 * sizeof(float)));
    HIPCHK(ctx, hipMalloc((void**)&f->kf_n4, npx * 4 * sizeof(float)));
    HIPCHK(ctx, hipMalloc((void**)&d.state, sizeof(FernState)));
    HIPCHK(ctx, hipHostMalloc((void**)&f->h_state, sizeof(FernState)));
    FernState init{};
    init.key_all = kArmed; init.key_match = kArmed; init.min_all = 3.402823466e+38f; init.min_match = 3.402823466e+38f; init.match_id = -1;
    *f->h_state = init;
    HIPCHK(ctx, hipMemcpyAsync(d.state, f->h_state, sizeof(FernState), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipHostMalloc((void**)&f->h_gate, sizeof(cf_ferns_gate)));
    HIPCHK(ctx, hipHostMalloc((void**)&f->h_close, sizeof(cf_ferns_closure)));
    memset(f->h_gate, 0, sizeof(cf_ferns_gate)); memset(f->h_close, 0, sizeof(cf_ferns_closure));
    HIPCHK(ctx, hipMalloc((void**)&f->cons.src, sizeof(float) * 3 * CF_DEFORM_MAX_CONSTRAINTS));
    HIPCHK(ctx, hipMalloc((void**)&f->cons.dst, sizeof(float) * 3 * CF_DEFORM_MAX_CONSTRAINTS));
    HIPCHK(ctx, hipMalloc((void**)&f->cons.time, sizeof(float) * CF_DEFORM_MAX_CONSTRAINTS));
    HIPCHK(ctx, hipMemsetAsync(f->cons.src, 0, sizeof(float) * 3 * CF_DEFORM_MAX_CONSTRAINTS, s));
    HIPCHK(ctx, hipMemsetAsync(f->cons.dst, 0, sizeof(float) * 3 * CF_DEFORM_MAX_CONSTRAINTS, s));
    HIPCHK(ctx, hipMemsetAsync(f->cons.time, 0, sizeof(float) * CF_DEFORM_MAX_CONSTRAINTS, s));
    HIPCHK(ctx, hipEventCreateWithFlags(&f->gate_event, hipEventDisableTiming));
    HIPCHK(ctx, hipStreamSynchronize(s));
    // the relocalisation tracker: RGBDOdometry at (W/8) x (H/8) with the intrinsics divided by 8 (Ferns.cpp:34-35)
    cf_config sc{};
    sc.width = rw; sc.height = rh; sc.fx = ctx->cfg.fx / 8; sc.fy = ctx->cfg.fy / 8; sc.cx = ctx->cfg.cx / 8; sc.cy = ctx->cfg.cy / 8;
    sc.device = ctx->cfg.device; sc.max_models = 1; sc.max_surfels = 0;
    if (int r = cf_create(&sc, &f->small)) { ctx->set_error(std::string("cf_ferns_create: small context: ") + (f->small ? cf_last_error(f->small) : "cf_create failed")); return r; }
    // bound here and again at the head of every cf_ferns_relocalise, the only user of the small context: after a cf_set_stream of the
    // parent it holds the old stream until then, and re-binding drains that stream (cf_set_stream synchronises the one it leaves)
    if (int r = cf_set_stream(f->small, ctx->stream)) return r;
    if (int r = cf_odom_create(f->small, &f->odom)) { ctx->set_error(std::string("cf_ferns_create: small tracker: ") + cf_last_error(f->small)); return r; }
    return CF_OK;
}

// ICP of the current reduced maps against keyframe `id`'s (Ferns.cpp:205-229), shared by cf_ferns_relocalise and cf_ferns_find_frame:
// fetches the keyframe's pose, fills result->pose and icp_*.  The reference never initialises the colour side of this tracker and runs
// it with icpWeight 100, which switches the RGB term off: its (all-zero) images are never read.
static int track_against_keyframe(cf_ferns* f, int id, const char* who, float fern_pose[16], cf_ferns_result* result, cf_track_stats* stats)
{
    cf_ctx* ctx = f->ctx;
    const FernsDev& d = f->d;
    const size_t npx = (size_t)d.npx;
    HIPCHK(ctx, hipMemcpy(fern_pose, d.pose + (size_t)id * 16, 64, hipMemcpyDeviceToHost));
    hipStream_t s = ctx->cur();
    if (f->small->stream != s) if (int r = cf_set_stream(f->small, s)) return r;
    hipLaunchKernelGGL(ferns_planar_to_x4_kernel, dim3((d.npx + 255) / 256), dim3(256), 0, s, d.vmap + (size_t)id * npx * 3,
                       d.nmap + (size_t)id * npx * 3, d.npx, reinterpret_cast<float4*>(f->kf_v4), reinterpret_cast<float4*>(f->kf_n4));
    HIPCHK(ctx, hipGetLastError());
    auto sub = [&](int r, const char* what) { if (r) ctx->set_error(std::string(who) + ": " + what + ": " + cf_last_error(f->small)); return r; };
    if (int r = sub(cf_odom_init_icp_model(f->odom, f->kf_v4, f->kf_n4, fern_pose), "initICPModel")) return r;
    const float* vm[CF_NUM_PYRS] = {d.cur_v, nullptr, nullptr};
    const float* nm[CF_NUM_PYRS] = {d.cur_n, nullptr, nullptr};
    if (int r = sub(cf_odom_bind_frame_maps(f->odom, vm, nm), "bind")) return r;
    float trans[3] = {fern_pose[3], fern_pose[7], fern_pose[11]};
    float rot[9] = {fern_pose[0], fern_pose[1], fern_pose[2], fern_pose[4], fern_pose[5], fern_pose[6], fern_pose[8], fern_pose[9], fern_pose[10]};
    cf_track_opts opts{};
    opts.rgb_only = 0; opts.icp_weight = 100; opts.pyramid = 0; opts.fast_odom = 0; opts.so3 = 0;
    if (int r = sub(cf_odom_get_incremental_transformation(f->odom, trans, rot, &opts, nullptr, stats), "getIncrementalTransformation")) return r;
    float* P = result->pose;
    P[0] = rot[0]; P[1] = rot[1]; P[2] = rot[2]; P[3] = trans[0];
    P[4] = rot[3]; P[5] = rot[4]; P[6] = rot[5]; P[7] = trans[1];
    P[8] = rot[6]; P[9] = rot[7]; P[10] = rot[8]; P[11] = trans[2];
    P[12] = 0; P[13] = 0; P[14] = 0; P[15] = 1;
    result->icp_ran = 1; result->icp_error = stats->last_icp_error; result->icp_count = stats->last_icp_count;
    return CF_OK;
}

static bool loop_samples_ok(int n_ferns)
{
    if (n_ferns < 50) return false;
    const int step = n_ferns / 50;
    return (n_ferns + step - 1) / step <= CF_FERNS_MAX_SAMPLES;
}

// the launch of ferns_close_kernel and the read of its record
static int close_candidate(cf_ferns* f, int keyframe, const float curr_pose[16], const float est_pose[16], float icp_error, float icp_count,
                           int lost, int time, cf_ferns_closure* out)
{
    cf_ctx* ctx = f->ctx;
    CloseArgs a{};
    memcpy(a.curr, curr_pose, sizeof(a.curr)); memcpy(a.est, est_pose, sizeof(a.est));
    a.icp_error = icp_error; a.icp_count = icp_count; a.photo_threshold = f->cfg.photo_threshold;
    a.fx = f->small->cfg.fx; a.fy = f->small->cfg.fy; a.cx = f->small->cfg.cx; a.cy = f->small->cfg.cy;
    a.keyframe = keyframe; a.lost = lost ? 1 : 0; a.time = time; a.max_depth_mm = f->cfg.max_depth_mm;
    a.samples_ok = loop_samples_ok(f->d.n) ? 1 : 0;
    hipStream_t s = ctx->cur();
    hipLaunchKernelGGL(ferns_close_kernel, dim3(1), dim3(256), 0, s, f->d, a, f->cons, f->h_close);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(s));
    *out = *f->h_close;
    return CF_OK;
}

extern "C" {

int cf_ferns_table(uint64_t seed, int n_ferns, int reduced_width, int reduced_height, int max_depth_mm, cf_fern* out)
{
    if (!out || n_ferns < 1 || n_ferns > CF_FERNS_MAX || reduced_width < 1 || reduced_height < 1 || max_depth_mm < 400) return CF_EINVAL;
    uint64_t s = seed;
    for (int i = 0; i < n_ferns; i++) {   // six draws per fern, in this order; value = lo + draw % (hi - lo + 1)
        out[i].x = (int32_t)(splitmix64(s) % (uint64_t)reduced_width);
        out[i].y = (int32_t)(splitmix64(s) % (uint64_t)reduced_height);
        out[i].r = (int32_t)(splitmix64(s) % 256u);
        out[i].g = (int32_t)(splitmix64(s) % 256u);
        out[i].b = (int32_t)(splitmix64(s) % 256u);
        out[i].d = 400 + (int32_t)(splitmix64(s) % (uint64_t)(max_depth_mm - 400 + 1));
    }
    return CF_OK;
}

int cf_ferns_create(cf_ctx* ctx, const cf_ferns_config* cfg, const cf_fern* table, uint64_t seed, cf_ferns** out)
{
    if (!ctx || !cfg || !out) return CF_EINVAL;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    if (W % 128 || H % 32) { ctx->set_error("cf_ferns_create: the frame width must be a multiple of 128 and the height of 32 (the 8x reduced frame is a tracker frame)"); return CF_EINVAL; }
    if (cfg->n_ferns < 1 || cfg->n_ferns > CF_FERNS_MAX) { ctx->set_error("cf_ferns_create: n_ferns must lie in 1..2048"); return CF_EINVAL; }
    if (cfg->capacity < 1 || cfg->max_depth_mm < 400) { ctx->set_error("cf_ferns_create: capacity >= 1 and max_depth_mm >= 400"); return CF_EINVAL; }
    const int rw = W / 8, rh = H / 8;
    std::vector<cf_fern> tab((size_t)cfg->n_ferns);
    if (table) {
        for (int i = 0; i < cfg->n_ferns; i++) {
            const cf_fern& t = table[i];
            if (t.x < 0 || t.x >= rw || t.y < 0 || t.y >= rh || t.r < 0 || t.r > 255 || t.g < 0 || t.g > 255 || t.b < 0 || t.b > 255) {
                ctx->set_error("cf_ferns_create: a fern of the table lies outside the reduced image or has a colour threshold outside 0..255");
                return CF_EINVAL;
            }
            tab[i] = t;
        }
    } else if (int r = cf_ferns_table(seed, cfg->n_ferns, rw, rh, cfg->max_depth_mm, tab.data())) return r;

    cf_ferns* f = new cf_ferns();
    f->ctx = ctx; f->cfg = *cfg; f->table = tab;
    const int rc = ferns_build(ctx, f);
    if (rc != CF_OK) {   // nothing half-built is handed out: its kernels would run on null buffers
        (void)hipGetLastError();
        cf_ferns_destroy(f);
        *out = nullptr;
        return rc;
    }
    *out = f;
    return CF_OK;
}

void cf_ferns_destroy(cf_ferns* f)
{
    if (!f) return;
    (void)hipStreamSynchronize(f->ctx->stream);
    if (f->odom) cf_odom_destroy(f->odom);
    if (f->small) cf_destroy(f->small);
    FernsDev& d = f->d;
    (void)hipFree(f->d_table); (void)hipFree(d.codes); (void)hipFree(d.cur_codes); (void)hipFree(d.good); (void)hipFree(d.time); (void)hipFree(d.co);
    (void)hipFree(d.pose); (void)hipFree(d.vmap); (void)hipFree(d.nmap); (void)hipFree(d.rgb); (void)hipFree(d.cur_v); (void)hipFree(d.cur_n);
    (void)hipFree(d.cur_rgb); (void)hipFree(f->kf_v4); (void)hipFree(f->kf_n4); (void)hipFree(d.state);
    (void)hipFree(f->cons.src); (void)hipFree(f->cons.dst); (void)hipFree(f->cons.time);
    if (f->gate_event) (void)hipEventDestroy(f->gate_event);
    if (f->h_state) (void)hipHostFree(f->h_state);
    if (f->h_gate) (void)hipHostFree(f->h_gate);
    if (f->h_close) (void)hipHostFree(f->h_close);
    delete f;
}

int cf_ferns_get_table(const cf_ferns* f, cf_fern* out)
{
    if (!f || !out) return CF_EINVAL;
    memcpy(out, f->table.data(), sizeof(cf_fern) * f->table.size());
    return CF_OK;
}

int cf_ferns_encode(cf_ferns* f, const float* vertex4, const float* normal4, const uint8_t* rgba)
{
    if (!f || !vertex4 || !normal4 || !rgba) return CF_EINVAL;
    cf_ctx* ctx = f->ctx;
    const int blocks = 1 + (f->d.npx + 255) / 256;
    hipLaunchKernelGGL(ferns_encode_kernel, dim3(blocks), dim3(256), 0, ctx->cur(), f->d, reinterpret_cast<const float4*>(vertex4),
                       reinterpret_cast<const float4*>(normal4), reinterpret_cast<const uchar4*>(rgba));
    HIPCHK(ctx, hipGetLastError());
    return CF_OK;
}

int cf_ferns_search(cf_ferns* f, int time, int min_age)
{
    if (!f) return CF_EINVAL;
    cf_ctx* ctx = f->ctx;
    hipLaunchKernelGGL(ferns_search_kernel, dim3(search_grid(f)), dim3(kSearchBlock), 0, ctx->cur(), f->d, time, min_age);
    HIPCHK(ctx, hipGetLastError());
    return CF_OK;
}

int cf_ferns_append(cf_ferns* f, const float pose[16], int src_time, float threshold)
{
    if (!f || !pose) return CF_EINVAL;
    cf_ctx* ctx = f->ctx;
    PoseArg p;
    memcpy(p.m, pose, sizeof(p.m));
    const int total16 = f->d.row16 + f->d.npx * 3 / 4 * 2 + f->d.npx * 3 / 16;
    int blocks = (total16 + 255) / 256;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(ferns_append_kernel, dim3(blocks), dim3(256), 0, ctx->cur(), f->d, p, src_time, threshold);
    HIPCHK(ctx, hipGetLastError());
    f->adds_enqueued++;
    return CF_OK;
}

// Ferns::addFrame (Ferns.cpp:72-142) without a host wait: encode -> search -> conditional append, three launches
int cf_ferns_add_async(cf_ferns* f, const float* vertex4, const float* normal4, const uint8_t* rgba, const float pose[16], int src_time,
                       float threshold)
{
    if (!f || !pose) return CF_EINVAL;
    if (int r = cf_ferns_encode(f, vertex4, normal4, rgba)) return r;
    if (int r = cf_ferns_search(f, src_time, 0)) return r;
    return cf_ferns_append(f, pose, src_time, threshold);
}

int cf_ferns_count(cf_ferns* f, int* count, int* full)
{
    if (!f) return CF_EINVAL;
    if (int r = fetch_state(f)) return r;
    if (count) *count = f->h_state->count;
    if (full) *full = f->h_state->full;
    return CF_OK;
}

int cf_ferns_last_search(cf_ferns* f, int32_t* co_host, int co_capacity, int* searched, float* min_all, float* min_match, int* match_id,
                         int* appended)
{
    if (!f) return CF_EINVAL;
    cf_ctx* ctx = f->ctx;
    if (int r = fetch_state(f)) return r;
    const FernState& s = *f->h_state;
    if (co_host) {
        if (co_capacity < s.searched) { ctx->set_error("cf_ferns_last_search: co_host is smaller than the searched database"); return CF_EINVAL; }
        if (s.searched > 0) HIPCHK(ctx, hipMemcpy(co_host, f->d.co, sizeof(int) * (size_t)s.searched, hipMemcpyDeviceToHost));
    }
    if (searched) *searched = s.searched;
    if (min_all) *min_all = s.min_all;
    if (min_match) *min_match = s.min_match;
    if (match_id) *match_id = s.match_id;
    if (appended) *appended = s.appended;
    return CF_OK;
}

int cf_ferns_download(cf_ferns* f, int id, uint8_t* codes, int* good, float pose[16], int* time, float* vmap, float* nmap, uint8_t* rgb)
{
    if (!f) return CF_EINVAL;
    cf_ctx* ctx = f->ctx;
    if (int r = fetch_state(f)) return r;
    if (id < -1 || id >= f->h_state->count) { ctx->set_error("cf_ferns_download: no such keyframe"); return CF_EINVAL; }
    const FernsDev& d = f->d;
    const size_t npx = (size_t)d.npx, k = id < 0 ? 0 : (size_t)id;
    const bool cur = id < 0;
    if (codes) HIPCHK(ctx, hipMemcpy(codes, cur ? d.cur_codes : d.codes + k * d.row_bytes, (size_t)d.n, hipMemcpyDeviceToHost));
    if (good) { if (cur) *good = f->h_state->good_cur; else HIPCHK(ctx, hipMemcpy(good, d.good + k, sizeof(int), hipMemcpyDeviceToHost)); }
    if (pose) {
        if (cur) { memset(pose, 0, 64); pose[0] = pose[5] = pose[10] = pose[15] = 1.0f; }   // (Ferns.cpp:156: identity, time 0)
        else HIPCHK(ctx, hipMemcpy(pose, d.pose + k * 16, 64, hipMemcpyDeviceToHost));
    }
    if (time) { if (cur) *time = 0; else HIPCHK(ctx, hipMemcpy(time, d.time + k, sizeof(int), hipMemcpyDeviceToHost)); }
    if (vmap) HIPCHK(ctx, hipMemcpy(vmap, cur ? d.cur_v : d.vmap + k * npx * 3, npx * 12, hipMemcpyDeviceToHost));
    if (nmap) HIPCHK(ctx, hipMemcpy(nmap, cur ? d.cur_n : d.nmap + k * npx * 3, npx * 12, hipMemcpyDeviceToHost));
    if (rgb) HIPCHK(ctx, hipMemcpy(rgb, cur ? d.cur_rgb : d.rgb + k * npx * 3, npx * 3, hipMemcpyDeviceToHost));
    return CF_OK;
}

// Ferns::findFrame (Ferns.cpp:144-262) for the current slot.  A rare, synchronous call: the host reads the match, decides on
// blockHDAware, runs the small tracker and evaluates the photometric check (f64 from the f32 inputs) itself.
int cf_ferns_relocalise(cf_ferns* f, const float curr_pose[16], int time, int min_age, int lost, cf_ferns_result* result)
{
    if (!f || !result) return CF_EINVAL;
    (void)curr_pose;   // (only the surface constraints of a loop closure read it, Ferns.cpp:240-255: cf_ferns_find_frame)
    cf_ctx* ctx = f->ctx;
    const FernsDev& d = f->d;
    memset(result, 0, sizeof(*result));
    result->keyframe = -1;
    result->pose[0] = result->pose[5] = result->pose[10] = result->pose[15] = 1.0f;
    result->photo_error = INFINITY;
    if (int r = cf_ferns_search(f, time, min_age)) return r;
    if (int r = fetch_state(f)) return r;
    result->dissimilarity = f->h_state->min_match;
    const int id = f->h_state->match_id;
    if (id < 0) return CF_OK;
    result->keyframe = id;
    const size_t npx = (size_t)d.npx;
    std::vector<uint8_t> cq((size_t)d.n), ck((size_t)d.n);
    HIPCHK(ctx, hipMemcpy(cq.data(), d.cur_codes, (size_t)d.n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(ck.data(), d.codes + (size_t)id * d.row_bytes, (size_t)d.n, hipMemcpyDeviceToHost));
    {   // blockHDAware, Ferns.cpp:321-336
        int count = 0; float val = 0;
        for (int i = 0; i < d.n; i++)
            if (cq[i] != 255 && ck[i] != 255) { count++; if (cq[i] == ck[i]) val += 1.0f; }
        result->overlap = val / (float)count;
    }
    if (!(result->overlap > 0.3f)) return CF_OK;
    float fern_pose[16];
    cf_track_stats stats{};
    if (int r = track_against_keyframe(f, id, "cf_ferns_relocalise", fern_pose, result, &stats)) return r;
    const float* P = result->pose;
    // photometricCheck, Ferns.cpp:264-307, in f64 from the f32 inputs
    std::vector<float> cv(npx * 3);
    std::vector<uint8_t> crgb(npx * 3), krgb(npx * 3);
    HIPCHK(ctx, hipMemcpy(cv.data(), d.cur_v, npx * 12, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(crgb.data(), d.cur_rgb, npx * 3, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(krgb.data(), d.rgb + (size_t)id * npx * 3, npx * 3, hipMemcpyDeviceToHost));
    {
        const double fx = (double)f->small->cfg.fx, fy = (double)f->small->cfg.fy, cx = (double)f->small->cfg.cx, cy = (double)f->small->cfg.cy;
        double Rd[9], td[3];   // [R^T R', R^T (t' - t)]: fernPose^-1 * estPose
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++)
                Rd[i * 3 + j] = ((double)fern_pose[0 * 4 + i] * (double)P[0 * 4 + j] + (double)fern_pose[1 * 4 + i] * (double)P[1 * 4 + j]) +
                                (double)fern_pose[2 * 4 + i] * (double)P[2 * 4 + j];
            td[i] = ((double)fern_pose[0 * 4 + i] * ((double)P[3] - (double)fern_pose[3]) + (double)fern_pose[1 * 4 + i] * ((double)P[7] - (double)fern_pose[7])) +
                    (double)fern_pose[2 * 4 + i] * ((double)P[11] - (double)fern_pose[11]);
        }
        long long sum = 0, cnt = 0;
        for (int i = 0; i < d.n; i++) {
            const cf_fern& t = f->table[i];
            const size_t p = (size_t)t.y * d.rw + t.x;
            const float z = cv[p + 2 * npx];
            if (!(z > 0) || !((int)(z * 1000.0f) < f->cfg.max_depth_mm)) continue;
            const double x = (double)cv[p], y = (double)cv[p + npx], zz = (double)z;
            const double wx = ((Rd[0] * x + Rd[1] * y) + Rd[2] * zz) + td[0];
            const double wy = ((Rd[3] * x + Rd[4] * y) + Rd[5] * zz) + td[1];
            const double wz = ((Rd[6] * x + Rd[7] * y) + Rd[8] * zz) + td[2];
            const double u = wx * fx / wz + cx, v = wy * fy / wz + cy;
            if (!(fabs(u) < 1e9) || !(fabs(v) < 1e9)) continue;   // (not finite or far outside: no correspondence)
            const int iu = (int)u, iv = (int)v;                   // truncation towards zero
            if (iu < 0 || iv < 0 || iu >= d.rw || iv >= d.rh) continue;
            const uint8_t* kp = &krgb[((size_t)iv * d.rw + iu) * 3];
            if (!(kp[0] > 0 || kp[1] > 0 || kp[2] > 0)) continue;
            const uint8_t* cp = &crgb[p * 3];
            sum += abs((int)kp[0] - (int)cp[0]) + abs((int)kp[1] - (int)cp[1]) + abs((int)kp[2] - (int)cp[2]);
            cnt++;
        }
        result->photo_count = (int)cnt;
        result->photo_error = cnt ? (double)sum / (double)cnt : (double)INFINITY;
    }
    const int icp_count_thresh = lost ? 1400 : 2400;
    result->accepted = ((double)stats.last_icp_error < 0.0003 && stats.last_icp_count > (float)icp_count_thresh &&
                        result->photo_error < (double)f->cfg.photo_threshold) ? 1 : 0;
    return CF_OK;
}

// ---- the loop-closure seam (include/cofusion_loop.h)
int cf_ferns_gate_async(cf_ferns* f)
{
    if (!f) return CF_EINVAL;
    cf_ctx* ctx = f->ctx;
    hipStream_t s = ctx->cur();
    hipLaunchKernelGGL(ferns_gate_kernel, dim3(1), dim3(64), 0, s, f->d, ++f->gate_serial, f->h_gate);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(f->gate_event, s));
    f->gate_pending = true; f->gated = false;
    return CF_OK;
}

int cf_ferns_gate_wait(cf_ferns* f, cf_ferns_gate* out)
{
    if (!f || !out) return CF_EINVAL;
    cf_ctx* ctx = f->ctx;
    if (!f->gate_pending) { ctx->set_error("cf_ferns_gate_wait: no cf_ferns_gate_async is outstanding"); return CF_ESTATE; }
    HIPCHK(ctx, hipEventSynchronize(f->gate_event));
    f->gate_pending = false;
    f->gate = *f->h_gate;
    if (f->gate.serial != f->gate_serial) { ctx->set_error("cf_ferns_gate_wait: the record is not the one of the last gate launch"); return CF_ESTATE; }
    f->gated = true;
    *out = f->gate;
    return CF_OK;
}

int cf_ferns_constraints(cf_ferns* f, int keyframe, const float curr_pose[16], const float est_pose[16], float icp_error, float icp_count,
                         int lost, int time, cf_ferns_closure* out)
{
    if (!f || !curr_pose || !est_pose || !out) return CF_EINVAL;
    if (!lost && !loop_samples_ok(f->d.n)) {
        f->ctx->set_error("cf_ferns_constraints: loop closure needs n_ferns >= 50 and at most 64 samples of stride n_ferns / 50");
        return CF_EINVAL;
    }
    if (keyframe < 0 || keyframe >= f->cfg.capacity) { f->ctx->set_error("cf_ferns_constraints: no such keyframe"); return CF_EINVAL; }
    return close_candidate(f, keyframe, curr_pose, est_pose, icp_error, icp_count, lost, time, out);
}

int cf_ferns_find_frame(cf_ferns* f, const float curr_pose[16], int time, int min_age, int lost, cf_ferns_result* result,
                        cf_ferns_closure* closure)
{
    if (!f || !curr_pose || !result || !closure) return CF_EINVAL;
    (void)min_age;
    cf_ctx* ctx = f->ctx;
    if (!f->gated) { ctx->set_error("cf_ferns_find_frame: gate the slot first (cf_ferns_gate_async, cf_ferns_gate_wait)"); return CF_ESTATE; }
    if (!lost && !loop_samples_ok(f->d.n)) {
        ctx->set_error("cf_ferns_find_frame: loop closure needs n_ferns >= 50 and at most 64 samples of stride n_ferns / 50");
        return CF_EINVAL;
    }
    memset(result, 0, sizeof(*result));
    memset(closure, 0, sizeof(*closure));
    closure->keyframe = -1;
    result->keyframe = -1;
    result->pose[0] = result->pose[5] = result->pose[10] = result->pose[15] = 1.0f;
    result->photo_error = INFINITY;
    result->dissimilarity = f->gate.dissimilarity;
    const int id = f->gate.match_id;
    if (id < 0) return CF_OK;
    if (id >= f->cfg.capacity) { ctx->set_error("cf_ferns_find_frame: the gate record names no keyframe of the database"); return CF_ESTATE; }
    result->keyframe = id;
    result->overlap = f->gate.overlap;
    if (!(result->overlap > 0.3f)) return CF_OK;
    float fern_pose[16];
    cf_track_stats stats{};
    if (int r = track_against_keyframe(f, id, "cf_ferns_find_frame", fern_pose, result, &stats)) return r;
    if (int r = close_candidate(f, id, curr_pose, result->pose, stats.last_icp_error, stats.last_icp_count, lost, time, closure)) return r;
    result->photo_count = (int)closure->photo_count;
    result->photo_error = closure->photo_error;
    result->accepted = closure->accepted;
    return CF_OK;
}

int cf_ferns_constraint_buffers(cf_ferns* f, float** src, float** dst, float** time)
{
    if (!f) return CF_EINVAL;
    if (src) *src = f->cons.src;
    if (dst) *dst = f->cons.dst;
    if (time) *time = f->cons.time;
    return CF_OK;
}

int cf_ferns_keyframe_buffers(cf_ferns* f, float** poses, int32_t** times)
{
    if (!f) return CF_EINVAL;
    if (poses) *poses = f->d.pose;
    if (times) *times = f->d.time;
    return CF_OK;
}

}  // extern "C"
