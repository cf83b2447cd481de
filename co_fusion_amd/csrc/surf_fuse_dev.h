// surf_fuse_dev.h -- fusing a frame into a map: association and update (part of surfel.hip's translation unit).
// Stage: data.* (Model::fuse's association: associate_kernel + the owner atomicMin) and update.vert (update_kernel), with their batch
// launchers.  (update_body also runs in surfel.hip's update_blocksums_kernel; bilerp is shared with surf_clean_dev.h.)
#pragma once
#include "surf_scan_dev.h"

namespace cf {

// ===================================================================================== fusion ====
// data.vert:78-211.  Thread per pixel (row-major); merge candidates race for their surfel with an
// atomicMin on the column-major rank (= "first drawn fragment wins" on the reference's update maps).
__device__ __forceinline__ float angle_between(f3 a, f3 b) { return det_acosf(dot(a, b) / (norm(a) * norm(b))); }

struct FuseArgs {
    const unsigned* index; const float4* vertConf; const float4* normRad;
    const uchar4* rgba; const float* depth_raw; const float* depth_filt; const unsigned char* mask;
    const float* tcx; const float* tcy;
    Mat4 pose; cf_cam cam; float inv_fx, inv_fy;
    int cols, rows, time; float weighting; int maskID; float maxDepth;
    float4* records;      // [N*3] by rank
    unsigned* new_flags;  // [N] by rank
    unsigned* owner;      // [max_surfels], 0xFFFFFFFF = none
};

// one channel of tex4_linear (same expression), fed from staged texels
__device__ __forceinline__ float bilerp(float a, float b, float c, float d, float wx, float wy)
{
    const float top = a * (1.0f - wx) + b * wx, bot = c * (1.0f - wx) + d * wx;
    return top * (1.0f - wy) + bot * wy;
}

// Four lanes per pixel.  A lane alone walks 16 window samples, each a chain of IEEE sqrt / divisions / acos (about
// 4400 VALU instructions per wave with only ~1 wave per SIMD in flight: 30 us of single-wave latency, measured).
// Here the quad (a) stages the 4x4 texel neighbourhood of the window once -- index, vertConf.xyz, normRad.xyz, one
// patch row per lane, all loads independent -- in LDS, and (b) splits the OUTER window loop: lane s evaluates the
// outer iterations s, s+4, ... with the shader's own f32 loop counters, then the quad reduces to the candidate the
// sequential loop would have kept (smallest distance, earliest on ties).  Lane 0 writes the record.
static constexpr int kAssocItems = kB / 4;   // pixels per workgroup
static constexpr int kPatchStride = 7 * 16 + 1;  // words per staged neighbourhood (+1: odd stride, no bank conflicts)

__global__ void __launch_bounds__(kB) associate_kernel(const Batch<FuseArgs> B, int xcd)
{
    __shared__ float s_patch[kAssocItems * kPatchStride];
    const VBlock vb = batch_decode(B.h);
    const FuseArgs& a = B.m[vb.model];
    const int cols = a.cols, rows = a.rows;
    // Only pixels whose integer coordinates share the parity of `time` survive the shader's first test
    // ((int)x == i, (int)y == j: the texcoords are pixel centres), so the launch enumerates just that quarter of
    // the image; new_flags is cleared by a memset beforehand.
    const int par = a.time % 2;
    const int n_i = (cols - par + 1) / 2, n_j = (rows - par + 1) / 2;
    const int gt = xcd_block(xcd, vb.bid, vb.nblk) * kB + threadIdx.x;
    const int t = gt >> 2, sub = gt & 3;
    float* const P = s_patch + (threadIdx.x >> 2) * kPatchStride;  // word c of texel k: P[c * 16 + k]
    bool alive = t < n_i * n_j;
    int i = 0, j = 0, q = 0, rank = 0;
    float tcx = 0, tcy = 0, x = 0, y = 0;
    f3 vPosLocal{0, 0, 0};
    if (alive) {
        j = 2 * (t / n_i) + par; i = 2 * (t % n_i) + par;
        q = j * cols + i; rank = i * rows + j;
        tcx = a.tcx[i]; tcy = a.tcy[j];
        x = tcx * (float)cols; y = tcy * (float)rows;
        alive = (((int)x % 2 == a.time % 2) && ((int)y % 2 == a.time % 2)) && ((int)a.mask[q] == a.maskID);
    }
    const float* dr = a.depth_raw;
    if (alive)
        alive = !(dr[j * cols + iclamp(i - 1, 0, cols - 1)] == 0 || dr[iclamp(j - 1, 0, rows - 1) * cols + i] == 0 ||
                  dr[j * cols + iclamp(i + 1, 0, cols - 1)] == 0 || dr[iclamp(j + 1, 0, rows - 1) * cols + i] == 0);
    const float cx = a.cam.cx, cy = a.cam.cy;
    if (alive) {
        vPosLocal = get_vertex(dr, cols, rows, i, j, x, y, cx, cy, a.inv_fx, a.inv_fy);
        alive = (vPosLocal.z > 0 && vPosLocal.z <= a.maxDepth);
    }
    const float scale = 1.0f;  // ModelProjection::FACTOR
    const float indexXStep = (1.0f / ((float)cols * scale)) * 0.5f, indexYStep = (1.0f / ((float)rows * scale)) * 0.5f;
    const float windowMultiplier = 2;
    const float iBeg = tcx - (scale * indexXStep * windowMultiplier), jBeg = tcy - (scale * indexYStep * windowMultiplier);
    const int X0 = (int)floorf(iBeg * (float)cols - 0.5f), Y0 = (int)floorf(jBeg * (float)rows - 0.5f);
    if (alive) {  // patch row `sub`
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int k = sub * 4 + c;
            const int g = iclamp(Y0 + sub, 0, rows - 1) * cols + iclamp(X0 + c, 0, cols - 1);
            const float4 vcf = a.vertConf[g];
            const float4 nrd = a.normRad[g];
            const unsigned idx = a.index[g];
            P[0 * 16 + k] = vcf.x; P[1 * 16 + k] = vcf.y; P[2 * 16 + k] = vcf.z;
            P[3 * 16 + k] = nrd.x; P[4 * 16 + k] = nrd.y; P[5 * 16 + k] = nrd.z;
            P[6 * 16 + k] = __uint_as_float(idx);
        }
    }
    __syncthreads();
    if (!alive) return;  // the four lanes of a pixel take the same decision

    const f3 vPos = xform_point(a.pose, vPosLocal);
    const f3 vPos_f = get_vertex(a.depth_filt, cols, rows, i, j, x, y, cx, cy, a.inv_fx, a.inv_fy);
    const f3 vNormLocal = get_normal_central(vPos_f, a.depth_filt, cols, rows, i, j, x, y, cx, cy, a.inv_fx, a.inv_fy);
    const float xl = (x - cx) * a.inv_fx, yl = (y - cy) * a.inv_fy;
    const float lambda = sqrtf(xl * xl + yl * yl + 1);
    const f3 ray = {xl, yl, 1};
    float bestDist = 1000;
    unsigned best = 0; int operation = 0, bestSeq = 0;
    // lane `sub` owns the outer iterations sub, sub+4, ...: it reaches its counter value by the same sequence of
    // f32 additions as the shader's loop and tests the same bound (the counter is monotonic, so the test of its
    // own value decides whether the iteration exists); the four lanes then run their inner loops simultaneously
    float ii = iBeg;
    for (int s4 = 0; s4 < sub; s4++) ii += indexXStep;
    for (int outer = sub; ii < tcx + (scale * indexXStep * windowMultiplier);
         outer += 4, ii += indexXStep, ii += indexXStep, ii += indexXStep, ii += indexXStep) {
        int inner = 0;
        for (float jj = jBeg; jj < tcy + (scale * indexYStep * windowMultiplier); jj += indexYStep, inner++) {
            const int nlx = (int)floorf(ii * (float)cols) - X0, nly = (int)floorf(jj * (float)rows) - Y0;
            const unsigned current = ((unsigned)nlx < 4u && (unsigned)nly < 4u)
                                         ? __float_as_uint(P[6 * 16 + nly * 4 + nlx])
                                         : a.index[nearest_texel(jj, rows) * cols + nearest_texel(ii, cols)];
            if (current > 0U) {
                const float fu = ii * (float)cols - 0.5f, fv = jj * (float)rows - 0.5f;
                const float x0f = floorf(fu), y0f = floorf(fv);
                const int lx = (int)x0f - X0, ly = (int)y0f - Y0;
                const bool staged = (unsigned)lx < 3u && (unsigned)ly < 3u;
                const float wx = fu - x0f, wy = fv - y0f;
                const float* qd = P + (ly * 4 + lx);
                float4 vertConf;
                if (staged) {
                    vertConf.x = bilerp(qd[0 * 16], qd[0 * 16 + 1], qd[0 * 16 + 4], qd[0 * 16 + 5], wx, wy);
                    vertConf.y = bilerp(qd[1 * 16], qd[1 * 16 + 1], qd[1 * 16 + 4], qd[1 * 16 + 5], wx, wy);
                    vertConf.z = bilerp(qd[2 * 16], qd[2 * 16 + 1], qd[2 * 16 + 4], qd[2 * 16 + 5], wx, wy);
                } else
                    vertConf = tex4_linear(a.vertConf, cols, rows, ii, jj);
                const float zdiff = (vertConf.z - vPosLocal.z);
                if (fabsf(zdiff * lambda) < 0.05f) {
                    const float dist = norm(cross(ray, f3{vertConf.x, vertConf.y, vertConf.z}));
                    float4 normRad;
                    if (staged) {
                        normRad.x = bilerp(qd[3 * 16], qd[3 * 16 + 1], qd[3 * 16 + 4], qd[3 * 16 + 5], wx, wy);
                        normRad.y = bilerp(qd[4 * 16], qd[4 * 16 + 1], qd[4 * 16 + 4], qd[4 * 16 + 5], wx, wy);
                        normRad.z = bilerp(qd[5 * 16], qd[5 * 16 + 1], qd[5 * 16 + 4], qd[5 * 16 + 5], wx, wy);
                    } else
                        normRad = tex4_linear(a.normRad, cols, rows, ii, jj);
                    if (dist < bestDist && (fabsf(normRad.z) < 0.75f || fabsf(angle_between(f3{normRad.x, normRad.y, normRad.z}, vNormLocal)) < 0.5f)) {
                        operation = 1; bestDist = dist; best = current; bestSeq = outer * 64 + inner;
                    }
                }
            }
        }
    }
    // quad reduction to the sequential loop's survivor: smallest distance, earliest (outer, inner) on ties
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        const int oOp = __shfl_xor(operation, o, 4), oSeq = __shfl_xor(bestSeq, o, 4);
        const float oDist = __shfl_xor(bestDist, o, 4);
        const unsigned oBest = (unsigned)__shfl_xor((int)best, o, 4);
        const bool take = oOp && (!operation || oDist < bestDist || (oDist == bestDist && oSeq < bestSeq));
        if (take) { operation = 1; bestDist = oDist; best = oBest; bestSeq = oSeq; }
    }
    if (sub != 0) return;
    const uchar4 c = a.rgba[q];
    const f3 nG = xform_dir(a.pose, vNormLocal);
    const float radius = get_radius(vPos_f.z, vNormLocal.z, a.inv_fx, a.inv_fy);
    const float conf = confidence(x, y, cx, cy, a.weighting);
    const float col = (float)(((int)c.x << 16) + ((int)c.y << 8) + (int)c.z);
    a.records[rank * 3 + 0] = make_float4(vPos.x, vPos.y, vPos.z, conf);
    a.records[rank * 3 + 1] = make_float4(col, 0.f, (float)a.time, operation == 1 ? -1.f : -2.f);
    a.records[rank * 3 + 2] = make_float4(nG.x, nG.y, nG.z, radius);
    if (operation == 1) atomicMin(&a.owner[best], (unsigned)rank);
    else a.new_flags[rank] = 1;
}

// update.vert:38-111 (reads the winning record through the owner index; resets the owner slot)
struct UpdateArgs { const float4* in; const unsigned* count; unsigned* owner; const float4* records; int time; float4* out; };
__device__ __forceinline__ void update_body(const Batch<UpdateArgs>& B, int blk)
{
    const VBlock vb = batch_decode_at(B.h, blk);
    const UpdateArgs& ua = B.m[vb.model];
    const float4* __restrict__ in = ua.in; unsigned* __restrict__ owner = ua.owner; const float4* __restrict__ records = ua.records;
    float4* __restrict__ out = ua.out; const int time = ua.time;
    const unsigned id = vb.bid * kB + threadIdx.x;
    if (id >= *ua.count) return;
    const float4 pc = in[id * 3], ct = in[id * 3 + 1], nr = in[id * 3 + 2];
    const unsigned ow = owner[id];
    if (ow == 0xFFFFFFFFu) { out[id * 3] = pc; out[id * 3 + 1] = ct; out[id * 3 + 2] = nr; return; }
    owner[id] = 0xFFFFFFFFu;
    const float4 rp = records[ow * 3], rc = records[ow * 3 + 1], rn = records[ow * 3 + 2];
    const float c_k = pc.w, a = rp.w;
    if (rn.w < (1.0f + 0.5f) * nr.w) {
        float4 op, oc, on;
        op.x = ((c_k * pc.x) + (a * rp.x)) / (c_k + a);
        op.y = ((c_k * pc.y) + (a * rp.y)) / (c_k + a);
        op.z = ((c_k * pc.z) + (a * rp.z)) / (c_k + a);
        op.w = c_k + a;
        const f3 oldc = decode_color(ct.x), newc = decode_color(rc.x);
        oc.x = encode_color(((c_k * oldc.x) + (a * newc.x)) / (c_k + a), ((c_k * oldc.y) + (a * newc.y)) / (c_k + a),
                            ((c_k * oldc.z) + (a * newc.z)) / (c_k + a));
        oc.y = ct.y; oc.z = ct.z; oc.w = (float)time;
        const float n0 = ((c_k * nr.x) + (a * rn.x)) / (c_k + a), n1 = ((c_k * nr.y) + (a * rn.y)) / (c_k + a);
        const float n2 = ((c_k * nr.z) + (a * rn.z)) / (c_k + a), n3 = ((c_k * nr.w) + (a * rn.w)) / (c_k + a);
        const f3 nn = normalized(f3{n0, n1, n2});
        on = make_float4(nn.x, nn.y, nn.z, n3);
        out[id * 3] = op; out[id * 3 + 1] = oc; out[id * 3 + 2] = on;
    } else {
        out[id * 3] = make_float4(pc.x, pc.y, pc.z, c_k + a);
        out[id * 3 + 1] = make_float4(ct.x, ct.y, ct.z, (float)time);
        out[id * 3 + 2] = nr;
    }
}
__global__ void __launch_bounds__(kB) update_kernel(const Batch<UpdateArgs> B) { update_body(B, (int)blockIdx.x); }

// association (+ the flag buffers zeroed in one launch in front of it)
void launch_associate_batch(hipStream_t s, const SurfelFuseArgs* items, int n_items)
{
    const int chunk = xcd_env("CF_XCD_ASSOC", 0);
    for_each_batch<FuseArgs>(items, n_items,
        [=](const SurfelFuseArgs& h, FuseArgs& a) {
            a.index = h.index; a.vertConf = reinterpret_cast<const float4*>(h.vertConf); a.normRad = reinterpret_cast<const float4*>(h.normRad);
            a.rgba = reinterpret_cast<const uchar4*>(h.rgba); a.depth_raw = h.depth_raw; a.depth_filt = h.depth_filt; a.mask = h.mask;
            a.tcx = h.tcx; a.tcy = h.tcy; a.pose = mat4_from(h.pose); a.cam = h.cam; a.inv_fx = h.inv_fx; a.inv_fy = h.inv_fy;
            a.cols = h.cols; a.rows = h.rows; a.time = h.time; a.weighting = h.weighting; a.maskID = h.maskID; a.maxDepth = h.maxDepth;
            a.records = reinterpret_cast<float4*>(h.records); a.new_flags = h.new_flags; a.owner = h.owner;
            const int par = h.time % 2;
            const long long n = (long long)((h.cols - par + 1) / 2) * ((h.rows - par + 1) / 2);
            return gridXcd(4 * n, chunk);
        },
        [=](Batch<FuseArgs>& B, const int* blocks, int nb, const SurfelFuseArgs* h) {
            Batch<FillArgs> Z;
            int zblocks[kSurfBatch];
            for (int k = 0; k < nb; k++) {
                const long long n16 = ((long long)h[k].cols * h[k].rows + 3) / 4;   // (new_flags holds cols * rows words: cf_model_create rounds it up)
                Z.m[k] = FillArgs{reinterpret_cast<uint4*>(h[k].new_flags), n16};
                zblocks[k] = h[k].flags_clean ? 0 : gridFor(n16);   // (left clean by the last compaction: ScanPassArgs::zero_flags)
            }
            if (const int zgrid = batch_layout(Z, zblocks, nb)) fill_zero_kernel<<<zgrid, kB, 0, s>>>(Z);
            associate_kernel<<<batch_layout(B, blocks, nb), kB, 0, s>>>(B, chunk);
        });
}
static UpdateArgs update_args(const UpdatePassArgs& h)
{
    return UpdateArgs{reinterpret_cast<const float4*>(h.in), h.count, h.owner, reinterpret_cast<const float4*>(h.records), h.time, reinterpret_cast<float4*>(h.out)};
}
static int update_blocks(const UpdatePassArgs& h) { return gridFor(h.count_bound); }
void launch_update_batch(hipStream_t s, const UpdatePassArgs* items, int n_items)
{
    for_each_batch<UpdateArgs>(items, n_items, [](const UpdatePassArgs& h, UpdateArgs& a) { a = update_args(h); return update_blocks(h); },
        [s](Batch<UpdateArgs>& B, const int* blocks, int nb, const UpdatePassArgs*) {
            if (const int grid = batch_layout(B, blocks, nb)) update_kernel<<<grid, kB, 0, s>>>(B);
        });
}

}  // namespace cf
