// surf_clean_dev.h -- cleaning a map after fusion (part of surfel.hip's translation unit).
// Stage: copy_unstable.* (Model::clean) -- clean_kernel stages every tested / modified surfel with its keep flag -- with its batch
// launcher; the ordered compaction behind it is surf_scan_dev.h's.  (bilerp: surf_fuse_dev.h.)
#pragma once
#include "surf_fuse_dev.h"

namespace cf {

// ====================================================================================== clean ====
// copy_unstable.vert:53-149 (deformation-graph branch dead: nodes == 0).  The tested/modified surfel
// is written to `staged` at its input position together with its keep flag; an ordered scan + scatter
// then reproduces the transform-feedback output order (old surfels first, appended ones after).
struct CleanArgs {
    const unsigned* index; const float4* vertConf; const float4* colorTime;
    const float* depth_filt; const unsigned char* mask;
    Mat4 t_inv; cf_cam cam; int cols, rows, time; float confThreshold, outlierCoeff; int timeDelta, maskID;
    const float4* rec;   // nullable: [rows * cols][2] vertConf | colorTime.zw, index, filtered depth per texel, packed by the index pass in front of this one (IndexArgs::clean_rec)
    // (the launch's per-model buffers, kernel parameters until round 4)
    const float4* surfels; const unsigned* count; const float4* fresh; const unsigned* n_fresh; unsigned total_bound; float4* staged; unsigned* flags;
    int xcd;   // workgroup order of THIS model's share (xcd_block): runs of 64 per XCD for a large map, the hardware's order for a small one
#ifdef CF_ABLATE
    int abl;   // diagnostics build (CF_CLEAN_ABLATE): 1 no staging of the texel patch, 2 no 4x4 window, 4 no 3x3 depth window -- timing only, results are wrong
#endif
};

// The 4x4 half-pixel window touches at most a 4x4 texel neighbourhood of the index map textures.  Reading it
// sample by sample (16 x (1 + 2x4) gathers per surfel) thrashes L1 and the XCD's L2 (measured: 560 MB of fabric
// reads per launch for 275 k surfels).  As in associate_kernel, four lanes share a surfel: the quad stages the
// neighbourhood -- vertConf.xyzw, colorTime.zw and the index, one patch row per lane -- in LDS with independent
// loads, splits the outer window loop (lane s takes iterations s, s+4, ...; the shader's f32 loop counters are
// kept), and adds up the two vote counts, which do not depend on the order.  Texels outside the staged patch
// (only reachable through the f32 loop-counter corner cases) fall back to the global fetch.
// Late in round 6 ("measure the rewrite"): timing ablations of this kernel (diagnostics build, CF_CLEAN_ABLATE;
// profiles/r6zd_*) put its 70 us at 17 us for loading / projecting / storing the surfels, 24 us for STAGING the neighbourhood -- twelve loads
// per lane from three arrays, every lane of a wave on a row of its own: 64 segments per instruction --, 14 us for the 4x4 window's
// arithmetic and 12 us for the 3x3 depth window's nine gathers per lane.  So the staging reads ONE array now, packed by the index pass in
// front of this one (index_resolve_kernel: vertConf | colorTime.zw, index, filtered depth = 32 bytes per texel), in 16-byte pieces dealt to the
// quad's lanes so that a quad reads 64 consecutive bytes per instruction (eight loads per lane, 16 segments per instruction), and the depth
// window is served from the staged patch (an eighth word per texel).  Without the records (cf_model_clean called alone) the old staging runs.
// (Measured as well: only colorTime.zw | index | depth in the record, 16 bytes, vertConf staged from its own array -- the index pass cheaper
// by 2.4 us, this kernel 64.9 against 52.2 us.)
// The eighth word makes a 256-thread workgroup's patches 33 KB: four workgroups per CU where 29 KB allowed five, and the kernel lives on its
// occupancy (81 against 70 us for the old staging with the larger stride).  Workgroups of kCleanB threads (8.3 KB each at 64) fill the
// CU's 160 KB to within a wave of the old occupancy.
#ifndef CF_CLEAN_B
#define CF_CLEAN_B 64
#endif
static constexpr int kCleanB = CF_CLEAN_B;
static constexpr int kCleanItems = kCleanB / 4;
static constexpr int kCleanStride = 8 * 16 + 1;  // words per staged neighbourhood: 8 words x 16 texels (+1: odd stride)

__global__ void __launch_bounds__(kCleanB) clean_kernel(const Batch<CleanArgs> B)
{
    __shared__ float s_patch[kCleanItems * kCleanStride];
    const VBlock vb = batch_decode(B.h);
    const CleanArgs& a = B.m[vb.model];
    const float4* __restrict__ surfels = a.surfels; const unsigned* __restrict__ count = a.count; const float4* __restrict__ fresh = a.fresh;
    const unsigned* __restrict__ n_fresh = a.n_fresh; const unsigned total_bound = a.total_bound; float4* __restrict__ staged = a.staged;
    unsigned* __restrict__ flags = a.flags;
    float* const P = s_patch + (threadIdx.x >> 2) * kCleanStride;  // word c of texel t: P[c * 16 + t]
    const float4* __restrict__ const rec = a.rec;
    const unsigned gt = (unsigned)xcd_block(a.xcd, vb.bid, vb.nblk) * kCleanB + threadIdx.x;
    const unsigned k = gt >> 2;
    const int sub = (int)(gt & 3u);
    const unsigned n_old = *count, n_all = n_old + *n_fresh;
    const bool exists = k < n_all;
    if (!exists && sub == 0 && k < total_bound) flags[k] = 0;
    const int cols = a.cols, rows = a.rows;
    const float scale = 1.0f;
    float4 pc = make_float4(0, 0, 0, 0), ct = pc, nr = pc;
    f3 localPos{0, 0, 0}, localNorm{0, 0, 0};
    float x = 0, y = 0, x_n = 0, y_n = 0;
    const float stepX = 1.0f / (float)cols, stepY = 1.0f / (float)rows;
    const float indexXStep = stepX * 0.5f / scale, indexYStep = stepY * 0.5f / scale;
    const float windowMultiplier = 2;
    bool window = false;
    if (exists) {
        const float4* src = (k < n_old) ? surfels + (size_t)k * 3 : fresh + (size_t)(k - n_old) * 3;
        pc = src[0]; ct = src[1]; nr = src[2];
        localPos = xform_point(a.t_inv, f3{pc.x, pc.y, pc.z});
        x = ((a.cam.fx * localPos.x) / localPos.z) + a.cam.cx; y = ((a.cam.fy * localPos.y) / localPos.z) + a.cam.cy;
        localNorm = normalized(xform_dir(a.t_inv, f3{nr.x, nr.y, nr.z}));
        x_n = x / (float)cols; y_n = y / (float)rows;
        window = (float)a.time - ct.w < (float)a.timeDelta && localPos.z > 0 && x > 0 && y > 0 && x < (float)cols && y < (float)rows;
    }
    const float iBeg = x_n - (scale * indexXStep * windowMultiplier), jBeg = y_n - (scale * indexYStep * windowMultiplier);
    const int X0 = (int)floorf(iBeg * (float)cols - 0.5f), Y0 = (int)floorf(jBeg * (float)rows - 0.5f);
#ifdef CF_ABLATE
    const int abl = a.abl;
#else
    constexpr int abl = 0;
#endif
    if (window && rec && !(abl & 1)) {  // the quad's 32 pieces of 16 bytes (4 rows x 4 texels x 2 halves): lane `sub` takes pieces sub, sub + 4, ...
        const int half = sub & 1;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int row = q >> 1, tex = (sub >> 1) + 2 * (q & 1), t = row * 4 + tex;
            const int g = iclamp(Y0 + row, 0, rows - 1) * cols + iclamp(X0 + tex, 0, cols - 1);
            const float4 v = rec[2 * g + half];
            float* const o = P + half * 64 + t;   // words 0..3 (vertConf) or 4..7 (colorTime.z, .w, index, depth)
            o[0] = v.x; o[16] = v.y; o[32] = v.z; o[48] = v.w;
        }
    } else
    if (window && !(abl & 1)) {  // patch row `sub`
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int t = sub * 4 + c;
            const int g = iclamp(Y0 + sub, 0, rows - 1) * cols + iclamp(X0 + c, 0, cols - 1);
            const float4 vcf = a.vertConf[g];
            const float4 ctm = a.colorTime[g];
            const unsigned idx = a.index[g];
            P[0 * 16 + t] = vcf.x; P[1 * 16 + t] = vcf.y; P[2 * 16 + t] = vcf.z; P[3 * 16 + t] = vcf.w;
            P[4 * 16 + t] = ctm.z; P[5 * 16 + t] = ctm.w;
            P[6 * 16 + t] = __uint_as_float(idx);
        }
    }
    __syncthreads();
    if (!exists) return;
    int test = 1;
    int cnt = 0, zCount = 0, violationCount = 0;
    float avgViolation = 0;
    if (window && !(abl & 2)) {
        // lane `sub` owns the outer iterations sub, sub+4, ... (see associate_kernel)
        float i = iBeg;
        for (int s4 = 0; s4 < sub; s4++) i += indexXStep;
        for (; i < x_n + (scale * indexXStep * windowMultiplier); i += indexXStep, i += indexXStep, i += indexXStep, i += indexXStep) {
            for (float j = jBeg; j < y_n + (scale * indexYStep * windowMultiplier); j += indexYStep) {
                const int nlx = (int)floorf(i * (float)cols) - X0, nly = (int)floorf(j * (float)rows) - Y0;
                const unsigned current = ((unsigned)nlx < 4u && (unsigned)nly < 4u)
                                             ? __float_as_uint(P[6 * 16 + nly * 4 + nlx])
                                             : a.index[nearest_texel(j, rows) * cols + nearest_texel(i, cols)];
                if (current > 0U) {
                    float4 vertConf, colorTime;
                    const float fu = i * (float)cols - 0.5f, fv = j * (float)rows - 0.5f;
                    const float x0f = floorf(fu), y0f = floorf(fv);
                    const int lx = (int)x0f - X0, ly = (int)y0f - Y0;
                    if ((unsigned)lx < 3u && (unsigned)ly < 3u) {
                        const float wx = fu - x0f, wy = fv - y0f;
                        const float* q = P + (ly * 4 + lx);
                        vertConf.x = bilerp(q[0 * 16], q[0 * 16 + 1], q[0 * 16 + 4], q[0 * 16 + 5], wx, wy);
                        vertConf.y = bilerp(q[1 * 16], q[1 * 16 + 1], q[1 * 16 + 4], q[1 * 16 + 5], wx, wy);
                        vertConf.z = bilerp(q[2 * 16], q[2 * 16 + 1], q[2 * 16 + 4], q[2 * 16 + 5], wx, wy);
                        vertConf.w = bilerp(q[3 * 16], q[3 * 16 + 1], q[3 * 16 + 4], q[3 * 16 + 5], wx, wy);
                        colorTime.z = bilerp(q[4 * 16], q[4 * 16 + 1], q[4 * 16 + 4], q[4 * 16 + 5], wx, wy);
                        colorTime.w = bilerp(q[5 * 16], q[5 * 16 + 1], q[5 * 16 + 4], q[5 * 16 + 5], wx, wy);
                    } else {
                        vertConf = tex4_linear(a.vertConf, cols, rows, i, j);
                        colorTime = tex4_linear(a.colorTime, cols, rows, i, j);
                    }
                    const float dx = vertConf.x - localPos.x, dy = vertConf.y - localPos.y;
                    if (colorTime.z < ct.z && vertConf.w > a.confThreshold && vertConf.z > localPos.z && vertConf.z - localPos.z < 0.01f &&
                        sqrtf(dx * dx + dy * dy) < nr.w * 1.4f)
                        cnt++;
                    if (colorTime.w == (float)a.time && vertConf.w > a.confThreshold && vertConf.z > localPos.z &&
                        vertConf.z - localPos.z > 0.01f && fabsf(localNorm.z) > 0.85f)
                        zCount++;
                }
            }
        }
    }
    if (window && !(abl & 4)) {
        // every lane of the quad walks the 3x3 depth window (sequential f32 sum) so that all four hold the result
        for (float i = x_n - stepX; i <= x_n + stepX; i += stepX)
            for (float j = y_n - stepY; j <= y_n + stepY; j += stepY) {
                const int tx = nearest_texel(i, cols), ty = nearest_texel(j, rows);
                const int lx = tx - X0, ly = ty - Y0;   // (inside the staged patch unless the f32 loop counters stray)
                const float dv = (rec && (unsigned)lx < 4u && (unsigned)ly < 4u) ? P[7 * 16 + ly * 4 + lx] : a.depth_filt[ty * cols + tx];
                const float d = dv - localPos.z;
                if (d > 0.03f) { violationCount++; avgViolation += d; }
            }
    }
    cnt += __shfl_xor(cnt, 1, 4); cnt += __shfl_xor(cnt, 2, 4);
    zCount += __shfl_xor(zCount, 1, 4); zCount += __shfl_xor(zCount, 2, 4);
    if (sub != 0) return;
    if (cnt > 8 || zCount > 4) test = 0;
    if (ct.w == -2) ct.w = (float)a.time;
    if ((ct.w == -1 || (((float)a.time - ct.w) > 20 && pc.w < a.confThreshold))) test = 0;
    if (ct.w > 0 && (float)a.time - ct.w > (float)a.timeDelta) test = 1;
    if (violationCount > 0) {
        avgViolation /= (float)violationCount;
        pc.w *= 1.0f / (1 + a.outlierCoeff * avgViolation);
        const int mx = nearest_texel(x_n, cols), my = nearest_texel(y_n, rows);
        const int maskValue = a.mask[my * cols + mx];
        const float wDepth = a.depth_filt[my * cols + mx];
        if (maskValue != a.maskID && (wDepth > localPos.z - 0.05f && wDepth < localPos.z + 0.05f))
            pc.w *= (0.5f + 0.5f * (1 - a.outlierCoeff / 10.0f));
    }
    flags[k] = (unsigned)test;
    staged[(size_t)k * 3] = pc; staged[(size_t)k * 3 + 1] = ct; staged[(size_t)k * 3 + 2] = nr;
}

void launch_clean_batch(hipStream_t s, const CleanPassArgs* items, int n_items)
{
    const int chunk = xcd_env("CF_XCD_CLEAN", 64);
    for_each_batch<CleanArgs>(items, n_items,
        [=](const CleanPassArgs& p, CleanArgs& a) {
            a.index = p.index; a.vertConf = reinterpret_cast<const float4*>(p.vertConf); a.colorTime = reinterpret_cast<const float4*>(p.colorTime);
            a.rec = reinterpret_cast<const float4*>(p.rec);
            a.depth_filt = p.depth_filt; a.mask = p.mask; a.t_inv = mat4_from(p.t_inv); a.cam = p.cam; a.cols = p.cols; a.rows = p.rows; a.time = p.time;
            a.confThreshold = p.confThreshold; a.outlierCoeff = p.outlierCoeff; a.timeDelta = p.timeDelta; a.maskID = p.maskID;
            a.surfels = reinterpret_cast<const float4*>(p.surfels); a.count = p.count; a.fresh = reinterpret_cast<const float4*>(p.fresh);
            a.n_fresh = p.n_fresh; a.total_bound = p.total_bound; a.staged = reinterpret_cast<float4*>(p.staged); a.flags = p.flags;
            // (the XCD-ordered runs need a share that is a multiple of 8 x 64 workgroups: for an object model of a few thousand surfels
            // that padding would be a third again of its workgroups, all of them empty)
            // (in workgroups of kCleanB threads: the runs cover the same surfels as `chunk` workgroups of kB did)
            const int cchunk = chunk * (kB / kCleanB);
            a.xcd = gridFor(4ll * p.total_bound, kCleanB) >= 4ll * 8 * cchunk ? cchunk : 0;
#ifdef CF_ABLATE
            static const int clean_abl = getenv("CF_CLEAN_ABLATE") ? atoi(getenv("CF_CLEAN_ABLATE")) : 0;
            a.abl = clean_abl;
#endif
            return gridXcd(4ll * p.total_bound, a.xcd, kCleanB);
        },
        [s](Batch<CleanArgs>& B, const int* blocks, int nb, const CleanPassArgs*) {
            if (const int grid = batch_layout(B, blocks, nb)) clean_kernel<<<grid, kCleanB, 0, s>>>(B);
        });
}

}  // namespace cf
