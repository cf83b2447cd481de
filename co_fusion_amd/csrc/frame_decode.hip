// frame_decode.hip -- the device half of the .klg log player (cf_frame_decoder_*).  Host threads inflate the
// depth and entropy-decode the JPEG of a frame into a pinned slot (host/KlgPlayer.cpp, host/Jpeg.cpp: jpegFront); two launches on
// the decoder's own stream finish it:
//   jpeg_idct_kernel    dequantisation + libjpeg's "islow" IDCT (jidctint.c; idct8x8 of host/Jpeg.cpp), all blocks of all components
//                       in one grid, one u8 plane per component at its padded size
//   jpeg_finish_kernel  chroma upsampling + YCbCr -> RGBA8 (or the raw-colour branch), and in the same grid u16 mm -> f32 metres
// Integer arithmetic only (the one float operation is the single multiply of the depth conversion), stated to equal host/Jpeg.cpp and
// host/KlgIO.cpp byte for byte.  Width: the host computes the IDCT in `long`; so does the device (long long).  With int16 quantised
// coefficients and 8-bit tables |dequantised| <= 32768 * 255 < 2^23; pass 1 multiplies sums of at most four such terms by constants
// < 2^15 and adds at most eight products (< 2^42), leaves them >> 11 (< 2^31), pass 2 does the same once more (< 2^50): no 64-bit
// overflow for ANY input the front end hands over, so it refuses nothing on account of the arithmetic.  (32 bits would overflow in
// pass 1 from |dequantised| ~ 2^14 on; at 7 200 blocks per frame the 64-bit multiplies cost microseconds.)
#include <stdlib.h>
#include <string.h>

#include <string>

#include "cf_frame_decoder.h"

using namespace cf;

namespace {

constexpr int kIdctBlocksPerGroup = 32;   // eight lanes per 8x8 block: 256 threads
constexpr int kWsPitch = 9;               // row pitch of the transposition buffer in 8-byte words (8 + 1: rows start on different banks)
constexpr int kHeaderBytes = kDecHeaderBytes;

typedef long long i64;

__device__ __forceinline__ i64 descale(i64 x, int n) { return (x + ((i64)1 << (n - 1))) >> n; }

// One pass of jidctint.c over eight values: the even part, the odd part, and the eight sums / differences BEFORE the descale, in
// output order 0..7.
__device__ __forceinline__ void islow_pass(const i64 in[8], i64 out[8])
{
    constexpr int CB = 13;
    constexpr i64 F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                  F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    i64 z2 = in[2], z3 = in[6];
    i64 z1 = (z2 + z3) * F0541;
    i64 tmp2 = z1 + z3 * (-F1847), tmp3 = z1 + z2 * F0765;
    i64 tmp0 = (in[0] + in[4]) * ((i64)1 << CB), tmp1 = (in[0] - in[4]) * ((i64)1 << CB);
    const i64 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2; i64 z4 = tmp1 + tmp3; const i64 z5 = (z3 + z4) * F1175;
    tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3; out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1; out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// Eight lanes per block: lane c runs column c (pass 1), the columns meet in LDS, lane r runs row r (pass 2) and stores its eight
// pixels with one 8-byte store.  The blocks of all components are dealt from one grid through the header's prefix table
// (comp[].first).  The host's shortcut for a column whose AC terms are all zero gives what the full pass gives
// (descale(x * 2^13, 11) = 4x), so there is no branch for it.
__global__ void __launch_bounds__(256) jpeg_idct_kernel(const cf_jpeg_header* __restrict__ hdr, const int16_t* __restrict__ coef,
                                                        uint8_t* __restrict__ planes, int total_blocks)
{
    __shared__ i64 ws[kIdctBlocksPerGroup][8 * kWsPitch];
    const int slot = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const int g = blockIdx.x * kIdctBlocksPerGroup + slot;
    const bool live = g < total_blocks;
    int ci = 0;
    if (live) {
        const int nc = hdr->ncomp;
        ci = (nc > 1 && g >= hdr->comp[1].first) + (nc > 2 && g >= hdr->comp[2].first);
        const int16_t* blk = coef + (size_t)g * 64;
        const uint8_t* q = hdr->qt[ci];
        i64 in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; r++) in[r] = (i64)((int)blk[r * 8 + lane] * (int)q[r * 8 + lane]);
        islow_pass(in, out);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[slot][r * kWsPitch + lane] = descale(out[r], 13 - 2);
    }
    __syncthreads();
    if (!live) return;
    i64 in[8], out[8];
#pragma unroll
    for (int c = 0; c < 8; c++) in[c] = ws[slot][lane * kWsPitch + c];
    islow_pass(in, out);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        i64 p = descale(out[c], 13 + 2 + 3) + 128;
        p = p < 0 ? 0 : (p > 255 ? 255 : p);
        if (c < 4) lo |= (unsigned)p << (8 * c); else hi |= (unsigned)p << (8 * (c - 4));
    }
    const cf_jpeg_comp cc = hdr->comp[ci];
    const int local = g - cc.first, by = local / cc.bw, bx = local - by * cc.bw;
    const size_t stride = (size_t)cc.bw * 8;
    uint2* dst = reinterpret_cast<uint2*>(planes + (size_t)cc.first * 64 + (size_t)(by * 8 + lane) * stride + (size_t)bx * 8);
    *dst = make_uint2(lo, hi);
}

struct FinishArgs {
    const cf_jpeg_header* hdr;   // device copy (CF_FRAME_COLOR_JPEG)
    const uint8_t* planes;       // jpeg_idct_kernel's output
    const uint8_t* rgb;          // 3 B/px (CF_FRAME_COLOR_RAW / _DECODED)
    const uint16_t* depth_mm;
    float* depth_out;
    uint8_t* rgba_out;
    int W, H, N, kind, swap, colour_groups;   // swap: store the triple reversed; colour_groups: workgroups of the colour half of the grid
};

// One component of one pixel at full resolution: libjpeg's default upsampling (jdsample.c) exactly as host/Jpeg.cpp states it -- the
// component itself at full sampling, "fancy" h2v1 and h2v2 (triangle filter; the +1 / +2 and +8 / +7 rounding alternation, the first
// and last column without a neighbour, rows clamped), replication for every other factor pair.
__device__ __forceinline__ int jpeg_sample(const uint8_t* __restrict__ plane, const cf_jpeg_comp c, int hmax, int vmax, int W, int H, int x, int y)
{
    const int stride = c.bw * 8;
    const int cw = (W * c.h + hmax - 1) / hmax, ch = (H * c.v + vmax - 1) / vmax;
    auto at = [&](int xx, int yy) {
        yy = yy < 0 ? 0 : (yy >= ch ? ch - 1 : yy);
        xx = xx < 0 ? 0 : (xx >= cw ? cw - 1 : xx);
        return (int)plane[(size_t)yy * stride + xx];
    };
    if (c.h == hmax && c.v == vmax) return at(x, y);
    if (c.h * 2 == hmax && c.v == vmax) {
        const int i = x >> 1;
        if (x & 1) return (i == cw - 1) ? at(i, y) : (3 * at(i, y) + at(i + 1, y) + 2) >> 2;
        return (i == 0) ? at(0, y) : (3 * at(i, y) + at(i - 1, y) + 1) >> 2;
    }
    if (c.h * 2 == hmax && c.v * 2 == vmax) {
        const int r = y >> 1, rn = (y & 1) ? r + 1 : r - 1, i = x >> 1;
        const int cur = 3 * at(i, r) + at(i, rn);
        if (x & 1) return (i == cw - 1) ? (cur * 4 + 7) >> 4 : (cur * 3 + 3 * at(i + 1, r) + at(i + 1, rn) + 7) >> 4;
        return (i == 0) ? (cur * 4 + 8) >> 4 : (cur * 3 + 3 * at(i - 1, r) + at(i - 1, rn) + 8) >> 4;
    }
    return at(x * c.h / hmax, y * c.v / vmax);
}

__device__ __forceinline__ unsigned pack_rgba(int r, int g, int b, int swap)
{
    return swap ? ((unsigned)b | (unsigned)g << 8 | (unsigned)r << 16 | 0xff000000u) : ((unsigned)r | (unsigned)g << 8 | (unsigned)b << 16 | 0xff000000u);
}
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Four pixels per thread and one 16-byte store, colour in the first `colour_groups` workgroups and depth in the rest (the
// update_blocksums_kernel idiom: a frame needs no third launch).  Colour conversion: libjpeg's 16-bit fixed point (jdcolor.c:
// FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF on the Cb term of green).
__global__ void __launch_bounds__(256) jpeg_finish_kernel(const FinishArgs a)
{
    const bool depth_half = (int)blockIdx.x >= a.colour_groups;
    const int q0 = (((int)blockIdx.x - (depth_half ? a.colour_groups : 0)) * 256 + (int)threadIdx.x) * 4;
    if (q0 >= a.N) return;
    const bool whole = q0 + 4 <= a.N;
    if (depth_half) {
        if (whole) {
            const uint2 m = *reinterpret_cast<const uint2*>(a.depth_mm + q0);
            float4 d;
            d.x = (float)(m.x & 0xffffu) * 0.001f; d.y = (float)(m.x >> 16) * 0.001f;
            d.z = (float)(m.y & 0xffffu) * 0.001f; d.w = (float)(m.y >> 16) * 0.001f;
            *reinterpret_cast<float4*>(a.depth_out + q0) = d;
        } else {
            for (int q = q0; q < a.N; q++) a.depth_out[q] = (float)a.depth_mm[q] * 0.001f;
        }
        return;
    }
    unsigned px[4] = {0xff000000u, 0xff000000u, 0xff000000u, 0xff000000u};
    const int n = whole ? 4 : a.N - q0;
    if (a.kind == CF_FRAME_COLOR_JPEG) {
        const int nc = a.hdr->ncomp, hmax = a.hdr->hmax, vmax = a.hdr->vmax;
        const cf_jpeg_comp c0 = a.hdr->comp[0], c1 = a.hdr->comp[1], c2 = a.hdr->comp[2];
        const uint8_t *p0 = a.planes + (size_t)c0.first * 64, *p1 = a.planes + (size_t)c1.first * 64, *p2 = a.planes + (size_t)c2.first * 64;
        int y = q0 / a.W, x = q0 - y * a.W;
        for (int k = 0; k < n; k++) {
            const int Y = jpeg_sample(p0, c0, hmax, vmax, a.W, a.H, x, y);
            if (nc == 1) px[k] = pack_rgba(Y, Y, Y, 0);
            else {
                const int cb = jpeg_sample(p1, c1, hmax, vmax, a.W, a.H, x, y) - 128, cr = jpeg_sample(p2, c2, hmax, vmax, a.W, a.H, x, y) - 128;
                const int r = clamp255(Y + ((91881 * cr + 32768) >> 16));
                const int g = clamp255(Y + ((-22554 * cb + 32768 + -46802 * cr) >> 16));
                const int b = clamp255(Y + ((116130 * cb + 32768) >> 16));
                px[k] = pack_rgba(r, g, b, a.swap);
            }
            if (++x == a.W) { x = 0; y++; }
        }
    } else if (a.kind != CF_FRAME_COLOR_NONE) {
        if (whole) {   // twelve bytes, 4-byte aligned (q0 is a multiple of four)
            const unsigned* s = reinterpret_cast<const unsigned*>(a.rgb + (size_t)q0 * 3);
            const unsigned w0 = s[0], w1 = s[1], w2 = s[2];
            px[0] = pack_rgba(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, a.swap);
            px[1] = pack_rgba(w0 >> 24, w1 & 255, (w1 >> 8) & 255, a.swap);
            px[2] = pack_rgba((w1 >> 16) & 255, w1 >> 24, w2 & 255, a.swap);
            px[3] = pack_rgba((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24, a.swap);
        } else {
            for (int k = 0; k < n; k++) {
                const uint8_t* s = a.rgb + (size_t)(q0 + k) * 3;
                px[k] = pack_rgba(s[0], s[1], s[2], a.swap);
            }
        }
    }
    unsigned* out = reinterpret_cast<unsigned*>(a.rgba_out) + q0;
    if (whole) *reinterpret_cast<uint4*>(out) = make_uint4(px[0], px[1], px[2], px[3]);
    else for (int k = 0; k < n; k++) out[k] = px[k];
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

namespace {

int harvest(cf_frame_decoder* d, int s)
{
    if (int r = image_ext_harvest(d, s)) return r;   // an image frame timed in this slot (the slot's events are shared)
    if (!d->timed[s]) return CF_OK;
    HIPCHK(d->ctx, hipEventSynchronize(d->tev[s][2]));
    float a = 0, b = 0;
    HIPCHK(d->ctx, hipEventElapsedTime(&a, d->tev[s][0], d->tev[s][1]));
    HIPCHK(d->ctx, hipEventElapsedTime(&b, d->tev[s][1], d->tev[s][2]));
    d->idct_ms += a; d->finish_ms += b; d->frames++;
    d->timed[s] = false;
    return CF_OK;
}

// the header a slot carries decides addresses on the device: everything the kernels index with is checked here
bool header_fits(const cf_jpeg_header& h, const cf_frame_desc& desc, uint64_t cap_blocks)
{
    if (h.width != desc.width || h.height != desc.height || (h.ncomp != 1 && h.ncomp != 3)) return false;
    int hmax = 1, vmax = 1;
    for (int c = 0; c < h.ncomp; c++) {
        if (h.comp[c].h < 1 || h.comp[c].h > 4 || h.comp[c].v < 1 || h.comp[c].v > 4) return false;
        hmax = h.comp[c].h > hmax ? h.comp[c].h : hmax; vmax = h.comp[c].v > vmax ? h.comp[c].v : vmax;
    }
    if (h.hmax != hmax || h.vmax != vmax) return false;
    const int mx = (h.width + 8 * hmax - 1) / (8 * hmax), my = (h.height + 8 * vmax - 1) / (8 * vmax);
    int64_t total = 0;
    for (int c = 0; c < h.ncomp; c++) {
        if (h.comp[c].bw != mx * h.comp[c].h || h.comp[c].bh != my * h.comp[c].v || h.comp[c].first != total) return false;
        total += (int64_t)h.comp[c].bw * h.comp[c].bh;
    }
    return total == h.total_blocks && (uint64_t)total <= cap_blocks;
}

}  // namespace

namespace cf {

int frame_decoder_harvest(cf_frame_decoder* d, int slot) { return harvest(d, slot); }

// The copies and the two launches of a frame whose colour lies in the slot's .klg staging, shared by cf_frame_decoder_submit
// (with_depth: u16 mm depth converted in the depth half of the finishing grid, timing events recorded) and
// cf_frame_decoder_submit_images (colour alone).  swap: store the triple reversed.
int frame_decoder_colour(cf_frame_decoder* d, int slot, int width, int height, int color_kind, bool swap, bool with_depth)
{
    cf_ctx* ctx = d->ctx;
    const size_t N = (size_t)width * height;
    uint8_t *hs = d->h_slot[slot], *ds = d->d_slot[slot];
    const cf_jpeg_header hdr = *reinterpret_cast<const cf_jpeg_header*>(hs);   // a copy: what is checked is what sizes the launch
    const bool jpeg = color_kind == CF_FRAME_COLOR_JPEG;
    cf_frame_desc desc;
    desc.width = width; desc.height = height; desc.color_kind = color_kind; desc.flip_colors = 0;
    if (jpeg && !header_fits(hdr, desc, d->cap_blocks)) {
        ctx->set_error("cf_frame_decoder_submit: the slot's JPEG header does not describe a frame of this size");
        return CF_EINVAL;
    }
    const bool timing = d->timing && with_depth;
    if (with_depth) HIPCHK(ctx, hipMemcpyAsync(ds + d->off_depth, hs + d->off_depth, N * 2, hipMemcpyHostToDevice, d->stream));
    if (jpeg) {
        memcpy(hs, &hdr, sizeof(hdr));
        HIPCHK(ctx, hipMemcpyAsync(ds, hs, kHeaderBytes + (size_t)hdr.total_blocks * 128, hipMemcpyHostToDevice, d->stream));
    } else if (color_kind != CF_FRAME_COLOR_NONE) {
        HIPCHK(ctx, hipMemcpyAsync(ds + d->off_rgb, hs + d->off_rgb, N * 3, hipMemcpyHostToDevice, d->stream));
    }
    if (timing) HIPCHK(ctx, hipEventRecord(d->tev[slot][0], d->stream));
    if (jpeg) {
        const int groups = (hdr.total_blocks + kIdctBlocksPerGroup - 1) / kIdctBlocksPerGroup;
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(groups), dim3(256), 0, d->stream, reinterpret_cast<const cf_jpeg_header*>(ds),
                           reinterpret_cast<const int16_t*>(ds + kHeaderBytes), d->d_planes, hdr.total_blocks);
        HIPCHK(ctx, hipGetLastError());
    }
    if (timing) HIPCHK(ctx, hipEventRecord(d->tev[slot][1], d->stream));
    FinishArgs a;
    a.hdr = reinterpret_cast<const cf_jpeg_header*>(ds); a.planes = d->d_planes; a.rgb = ds + d->off_rgb;
    a.depth_mm = reinterpret_cast<const uint16_t*>(ds + d->off_depth);
    a.depth_out = d->d_depth[slot]; a.rgba_out = d->d_rgba[slot];
    a.W = width; a.H = height; a.N = (int)N; a.kind = color_kind;
    a.swap = swap ? 1 : 0;
    a.colour_groups = (int)((N + 1023) / 1024);
    // colour in the first colour_groups workgroups, depth in as many more: without them the colour half runs alone
    hipLaunchKernelGGL(jpeg_finish_kernel, dim3((with_depth ? 2 : 1) * a.colour_groups), dim3(256), 0, d->stream, a);
    HIPCHK(ctx, hipGetLastError());
    if (timing) { HIPCHK(ctx, hipEventRecord(d->tev[slot][2], d->stream)); d->timed[slot] = true; }
    return CF_OK;
}

}  // namespace cf

extern "C" {

int cf_frame_decoder_create(cf_ctx* ctx, int max_w, int max_h, int slots, cf_frame_decoder** out)
{
    if (!ctx || !out) return CF_EINVAL;
    if (max_w < 1 || max_h < 1 || max_w > 16384 || max_h > 16384 || slots < 2 || slots > kMaxDecSlots) {
        ctx->set_error("cf_frame_decoder_create: a frame of 1..16384 pixels a side and 2..16 slots");
        return CF_EINVAL;
    }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    cf_frame_decoder* d = new cf_frame_decoder();
    d->ctx = ctx; d->max_w = max_w; d->max_h = max_h; d->slots = slots;
    d->cap_blocks = CF_JPEG_MAX_BLOCKS(max_w, max_h);
    const size_t N = (size_t)max_w * max_h;
    d->off_depth = align256(kHeaderBytes + (size_t)d->cap_blocks * 128);
    d->off_rgb = d->off_depth + align256(N * 2);
    d->slot_bytes = d->off_rgb + align256(N * 3);
    auto fail = [&](hipError_t e, const char* what) {
        ctx->set_error(std::string("cf_frame_decoder_create: ") + what + ": " + hipGetErrorString(e));
        cf_frame_decoder_destroy(d);
        return e == hipErrorOutOfMemory ? CF_ENOMEM : CF_EHIP;
    };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "stream");
    if ((e = hipEventCreateWithFlags(&d->consumed, hipEventDisableTiming)) != hipSuccess) return fail(e, "event");
    if ((e = hipMalloc(reinterpret_cast<void**>(&d->d_planes), (size_t)d->cap_blocks * 64)) != hipSuccess) return fail(e, "planes");
    for (int s = 0; s < slots; s++) {
        if ((e = hipEventCreateWithFlags(&d->done[s], hipEventDisableTiming)) != hipSuccess) return fail(e, "event");
        for (int k = 0; k < 3; k++) if ((e = hipEventCreate(&d->tev[s][k])) != hipSuccess) return fail(e, "event");
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&d->h_slot[s]), d->slot_bytes)) != hipSuccess) return fail(e, "pinned slot");
        memset(d->h_slot[s], 0, kHeaderBytes);
        if ((e = hipMalloc(reinterpret_cast<void**>(&d->d_slot[s]), d->slot_bytes)) != hipSuccess) return fail(e, "device slot");
        if ((e = hipMalloc(reinterpret_cast<void**>(&d->d_depth[s]), align256(N * 4))) != hipSuccess) return fail(e, "depth frame");
        if ((e = hipMalloc(reinterpret_cast<void**>(&d->d_rgba[s]), align256(N * 4))) != hipSuccess) return fail(e, "rgba frame");
    }
    static_assert(sizeof(cf_jpeg_header) <= kHeaderBytes, "the header's place in a slot");
    *out = d;
    return CF_OK;
}

void cf_frame_decoder_destroy(cf_frame_decoder* d)
{
    if (!d) return;
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    for (int s = 0; s < kMaxDecSlots; s++) {
        if (d->done[s]) (void)hipEventDestroy(d->done[s]);
        for (int k = 0; k < 3; k++) if (d->tev[s][k]) (void)hipEventDestroy(d->tev[s][k]);
        if (d->h_slot[s]) (void)hipHostFree(d->h_slot[s]);
        if (d->d_slot[s]) (void)hipFree(d->d_slot[s]);
        if (d->d_depth[s]) (void)hipFree(d->d_depth[s]);
        if (d->d_rgba[s]) (void)hipFree(d->d_rgba[s]);
    }
    if (d->d_planes) (void)hipFree(d->d_planes);
    image_ext_destroy(d->img);
    if (d->consumed) (void)hipEventDestroy(d->consumed);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

int cf_frame_decoder_slot(cf_frame_decoder* d, int slot, cf_frame_slot* out)
{
    if (!d || !out || slot < 0 || slot >= d->slots) return CF_EINVAL;
    uint8_t* base = d->h_slot[slot];
    out->header = reinterpret_cast<cf_jpeg_header*>(base);
    out->coef = reinterpret_cast<int16_t*>(base + kHeaderBytes);
    out->coef_blocks = d->cap_blocks;
    out->depth = reinterpret_cast<uint16_t*>(base + d->off_depth);
    out->rgb = base + d->off_rgb;
    return CF_OK;
}

int cf_frame_decoder_submit(cf_frame_decoder* d, int slot, const cf_frame_desc* desc)
{
    if (!d || !desc || slot < 0 || slot >= d->slots) return CF_EINVAL;
    cf_ctx* ctx = d->ctx;
    if (desc->width < 1 || desc->height < 1 || desc->width > d->max_w || desc->height > d->max_h ||
        desc->color_kind < CF_FRAME_COLOR_NONE || desc->color_kind > CF_FRAME_COLOR_DECODED) {
        ctx->set_error("cf_frame_decoder_submit: frame size outside the decoder's maximum, or an unknown colour kind");
        return CF_EINVAL;
    }
    if (d->timing) { if (int r = harvest(d, slot)) return r; }
    // the output frame (and the device input) of this slot may still be read by work the context's stream holds
    HIPCHK(ctx, hipEventRecord(d->consumed, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(d->stream, d->consumed, 0));
    // KlgLogReader::getNext: a JPEG is stored reversed (JPEGLoader::readData) and flip_colors reverses once more; raw colour is
    // reversed by flip_colors alone
    const bool swap = desc->color_kind == CF_FRAME_COLOR_RAW ? (desc->flip_colors != 0) : (desc->flip_colors == 0);
    if (int r = frame_decoder_colour(d, slot, desc->width, desc->height, desc->color_kind, swap, true)) return r;
    image_ext_clear_mask(d->img, slot);   // a .klg frame has no mask: cf_frame_decoder_acquire_mask answers NULL for it
    HIPCHK(ctx, hipEventRecord(d->done[slot], d->stream));
    d->submitted[slot] = true;
    return CF_OK;
}

int cf_frame_decoder_acquire(cf_frame_decoder* d, int slot, int complete, const float** depth_dev, const uint8_t** rgba_dev)
{
    if (!d || slot < 0 || slot >= d->slots) return CF_EINVAL;
    if (!d->submitted[slot]) { d->ctx->set_error("cf_frame_decoder_acquire: nothing was submitted to this slot"); return CF_ESTATE; }
    if (complete) HIPCHK(d->ctx, hipEventSynchronize(d->done[slot]));
    else HIPCHK(d->ctx, hipStreamWaitEvent(d->ctx->stream, d->done[slot], 0));
    if (depth_dev) *depth_dev = d->d_depth[slot];
    if (rgba_dev) *rgba_dev = d->d_rgba[slot];
    return CF_OK;
}

int cf_frame_decoder_timing(cf_frame_decoder* d, int on, double* idct_ms, double* finish_ms, uint64_t* frames)
{
    if (!d) return CF_EINVAL;
    HIPCHK(d->ctx, hipStreamSynchronize(d->stream));
    for (int s = 0; s < d->slots; s++) if (int r = harvest(d, s)) return r;
    if (idct_ms) *idct_ms = d->idct_ms;
    if (finish_ms) *finish_ms = d->finish_ms;
    if (frames) *frames = d->frames;
    d->idct_ms = d->finish_ms = 0; d->frames = 0;
    d->timing = on != 0;
    return CF_OK;
}

}  // extern "C"
