// image_decode.hip -- the device half of the image-sequence reader (cf_frame_decoder_*_images).  Host threads
// read the files of a frame, inflate them and undo the PNG filters (host/ImageIO.cpp) into the image staging of a decoder slot; the
// launches below, on the decoder's own stream, turn that into the frame cf_frame_decoder_acquire hands out:
//   exr_depth_kernel    one workgroup per block of scanlines of an OpenEXR file: the ZIP predictor (an inclusive byte prefix sum
//                       modulo 256 with a -128 bias per step) undone in place by a chunked workgroup scan, then the half-split
//                       interleave, the depth channel's run of every scanline and HALF -> f32 folded into one gather.  A block the
//                       file stores raw skips the scan and the interleave.
//   png_finish_kernel   unfiltered PNG scanlines (row stride 1 + bpp * width) -> RGBA8 / f32 depth / u8 mask, the three planes in
//                       one grid (the jpeg_finish_kernel idiom).  Rows start at any byte, so four pixels are fetched with aligned
//                       32-bit loads and a funnel shift.
// Colour that comes as JPEG or raw bytes goes through frame_decode.hip's kernels (frame_decoder_colour).  Everything is integer
// work except the single f32 product of the 16-bit depth conversion: the outputs equal host/ImageIO.cpp's *FinishHost byte for byte.
// PNG unfiltering stays on the host on purpose (a byte recurrence through the left, upper and upper-left neighbours).
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "cf_frame_decoder.h"

using namespace cf;

namespace cf {

struct ImageExt {
    size_t off_depth = 0, off_mask = 0, off_palette = 0, off_blocks = 0, bytes = 0;   // staging: colour | depth | mask | palette | block table
    size_t colour_bytes = 0, depth_bytes = 0, mask_bytes = 0;
    uint8_t* h[kMaxDecSlots]{};   // pinned
    uint8_t* d[kMaxDecSlots]{};
    uint8_t* d_mask[kMaxDecSlots]{};
    bool has_mask[kMaxDecSlots]{};
    // diagnostics (cf_frame_decoder_timing switches it on, cf_frame_decoder_image_timing reads): the slot's three events of
    // cf_frame_decoder lie around the two launches of an image frame
    bool timed[kMaxDecSlots]{}, timed_exr[kMaxDecSlots]{}, timed_finish[kMaxDecSlots]{};
    double exr_ms = 0, finish_ms = 0;
    uint64_t exr_frames = 0, finish_frames = 0;
};

void image_ext_destroy(ImageExt* e)
{
    if (!e) return;
    for (int s = 0; s < kMaxDecSlots; s++) {
        if (e->h[s]) (void)hipHostFree(e->h[s]);
        if (e->d[s]) (void)hipFree(e->d[s]);
        if (e->d_mask[s]) (void)hipFree(e->d_mask[s]);
    }
    delete e;
}

void image_ext_clear_mask(ImageExt* e, int slot)
{
    if (e) e->has_mask[slot] = false;
}

int image_ext_harvest(cf_frame_decoder* d, int s)
{
    ImageExt* e = d->img;
    if (!e || !e->timed[s]) return CF_OK;
    HIPCHK(d->ctx, hipEventSynchronize(d->tev[s][2]));
    float a = 0, b = 0;
    HIPCHK(d->ctx, hipEventElapsedTime(&a, d->tev[s][0], d->tev[s][1]));
    HIPCHK(d->ctx, hipEventElapsedTime(&b, d->tev[s][1], d->tev[s][2]));
    if (e->timed_exr[s]) { e->exr_ms += a; e->exr_frames++; }
    if (e->timed_finish[s]) { e->finish_ms += b; e->finish_frames++; }
    e->timed[s] = false;
    return CF_OK;
}

}  // namespace cf

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanChunk = kScanThreads * 16;   // bytes a workgroup scans per step: 16 per thread

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

__device__ __forceinline__ float half_bits_to_float(unsigned h)
{
    const unsigned s = (h >> 15) << 31, e = (h >> 10) & 31u;
    unsigned m = h & 1023u, bits;
    if (e == 0) {
        if (m == 0) bits = s;
        else {
            const int sh = __clz(m) - 21;   // shifts that bring the leading one to bit 10
            m <<= sh;
            bits = s | (unsigned)(113 - sh) << 23 | (m & 1023u) << 13;
        }
    } else if (e == 31) bits = s | 0x7f800000u | m << 13;
    else bits = s | (e + 112u) << 23 | m << 13;
    return __uint_as_float(bits);
}

struct ExrArgs {
    uint8_t* raw;                  // the slot's depth staging on the device: un-predicted in place
    const cf_exr_block* blocks;
    float* depth_out;
    int W, line_bytes, chan_offset, chan_half;
};

// Workgroup b owns block b.  Step 1 (compressed blocks): t[i] = (d[0] + ... + d[i] - 128 * i) mod 256.  The block starts at any even
// byte of the staging, so the scan walks 16-byte ALIGNED cells from the cell that holds the block's first byte: bytes of a cell
// outside the block count as zero and are never written (they belong to a neighbouring block's workgroup).  Per step of 4 KB: a
// serial sum of the thread's 16 bytes, a wave scan of those sums, the four wave totals through LDS, and the carry of the steps
// before.  Step 2: every pixel of the block's lines gathers its 2 or 4 bytes (byte p of the pixel data lies at p / 2 of the first
// half for even p, of the second half -- which starts at (n + 1) / 2 -- for odd p).
__global__ void __launch_bounds__(kScanThreads) exr_depth_kernel(const ExrArgs a)
{
    __shared__ unsigned wave_total[kScanThreads / 64];
    const cf_exr_block blk = a.blocks[blockIdx.x];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint8_t* base = a.raw + blk.offset;
    const int n = (int)blk.bytes;
    if (!blk.stored_raw) {
        const int lead = (int)(blk.offset & 15u);   // the staging itself is 256-byte aligned
        uint8_t* cell0 = base - lead;
        const int span = lead + n;                  // bytes from cell0 to the block's end
        unsigned carry = 0;
        for (int c0 = 0; c0 < span; c0 += kScanChunk) {   // uniform trip count: every thread meets the barriers
            const int at = c0 + tid * 16;                  // this thread's cell, relative to cell0
            unsigned char v[16];
            unsigned sum = 0;
            const bool any = at < span;
            if (any) {
                const uint4 q = *reinterpret_cast<const uint4*>(cell0 + at);
                const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int i = at + k - lead;           // index inside the block
                    const unsigned b = (i >= 0 && i < n) ? (w[k >> 2] >> (8 * (k & 3))) & 255u : 0u;
                    sum += b;
                    v[k] = (unsigned char)sum;             // the running sum modulo 256
                }
            }
            unsigned incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (lane == 63) wave_total[wave] = incl;
            __syncthreads();
            unsigned before = carry + incl - sum, total = 0;
#pragma unroll
            for (int k = 0; k < kScanThreads / 64; k++) {
                const unsigned t = wave_total[k];
                if (k < wave) before += t;
                total += t;
            }
            carry += total;
            __syncthreads();   // wave_total is rewritten by the next step
            if (any) {
                const int i0 = at - lead;
                if (i0 >= 0 && i0 + 16 <= n) {
                    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const unsigned t = (before + v[k] - (((unsigned)(i0 + k) & 1u) << 7)) & 255u;
                        w[k >> 2] |= t << (8 * (k & 3));
                    }
                    *reinterpret_cast<uint4*>(cell0 + at) = make_uint4(w[0], w[1], w[2], w[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const int i = i0 + k;
                        if (i >= 0 && i < n) base[i] = (unsigned char)((before + v[k] - (((unsigned)i & 1u) << 7)) & 255u);
                    }
                }
            }
        }
        __syncthreads();   // step 2 reads what other waves of this workgroup stored
    }
    const int lines = n / a.line_bytes, pixels = lines * a.W, half = (n + 1) >> 1;
    float* out = a.depth_out + (size_t)blk.first_line * a.W;
    for (int idx = tid; idx < pixels; idx += kScanThreads) {
        const int l = idx / a.W, x = idx - l * a.W;
        const int p = l * a.line_bytes + a.chan_offset + x * (a.chan_half ? 2 : 4);   // even: every run is a multiple of two bytes
        unsigned bits;
        if (blk.stored_raw) {
            bits = (unsigned)base[p] | (unsigned)base[p + 1] << 8;
            if (!a.chan_half) bits |= (unsigned)base[p + 2] << 16 | (unsigned)base[p + 3] << 24;
        } else {
            const uint8_t *lo = base + (p >> 1), *hi = base + half + (p >> 1);
            bits = (unsigned)lo[0] | (unsigned)hi[0] << 8;
            if (!a.chan_half) bits |= (unsigned)lo[1] << 16 | (unsigned)hi[1] << 24;
        }
        out[idx] = a.chan_half ? half_bits_to_float(bits) : __uint_as_float(bits);
    }
}

enum { SEC_OFF = 0, SEC_COLOUR_BLACK, SEC_COLOUR_GREY, SEC_COLOUR_RGB, SEC_COLOUR_PALETTE, SEC_COLOUR_RGBA, SEC_DEPTH_ZERO, SEC_DEPTH_PNG,
       SEC_MASK_PNG, SEC_MASK_RAW };

struct PngArgs {
    const uint8_t* colour;    // scanlines, 256-byte aligned, at least 4 bytes of slack behind the last row
    const uint8_t* palette;   // 768 bytes
    const uint8_t* depth;
    const uint8_t* mask;
    uint8_t* rgba_out;
    float* depth_out;
    uint8_t* mask_out;
    int W, N, flip, groups;   // groups: workgroups per section
    int sec[3];               // what each third of the grid does (SEC_*)
    float depth_scale;
};

// four bytes from any byte offset: two aligned 32-bit loads and a funnel shift
__device__ __forceinline__ unsigned load4(const uint8_t* __restrict__ base, size_t off)
{
    const unsigned* w = reinterpret_cast<const unsigned*>(base) + (off >> 2);
    const unsigned sh = (unsigned)(off & 3) * 8;
    const unsigned lo = w[0];
    return sh ? (lo >> sh) | (w[1] << (32 - sh)) : lo;
}
__device__ __forceinline__ unsigned rgba_of(unsigned r, unsigned g, unsigned b, int flip)
{
    return flip ? (b | g << 8 | r << 16 | 0xff000000u) : (r | g << 8 | b << 16 | 0xff000000u);
}

// Four pixels per thread, one 16-byte store for colour and depth, one 4-byte store for the mask.  Four pixels of ONE row are fetched
// with load4; a group that straddles a row end (widths that are no multiple of four) or the frame's end goes byte by byte.
__global__ void __launch_bounds__(256) png_finish_kernel(const PngArgs a)
{
    const int section = (int)blockIdx.x / a.groups, kind = a.sec[section];
    const int q0 = (((int)blockIdx.x - section * a.groups) * 256 + (int)threadIdx.x) * 4;
    if (kind == SEC_OFF || q0 >= a.N) return;
    const bool whole = q0 + 4 <= a.N;
    const int n = whole ? 4 : a.N - q0;
    const int y = q0 / a.W, x = q0 - y * a.W;
    const bool one_row = whole && x + 4 <= a.W;
    if (kind == SEC_DEPTH_ZERO || kind == SEC_DEPTH_PNG) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (kind == SEC_DEPTH_PNG) {
            const size_t stride = (size_t)2 * a.W + 1;
            if (one_row) {
                const size_t off = (size_t)y * stride + 1 + (size_t)2 * x;
                const unsigned w0 = load4(a.depth, off), w1 = load4(a.depth, off + 4);
                d[0] = (float)((w0 & 255u) << 8 | ((w0 >> 8) & 255u)) * a.depth_scale;     // big-endian samples
                d[1] = (float)(((w0 >> 16) & 255u) << 8 | (w0 >> 24)) * a.depth_scale;
                d[2] = (float)((w1 & 255u) << 8 | ((w1 >> 8) & 255u)) * a.depth_scale;
                d[3] = (float)(((w1 >> 16) & 255u) << 8 | (w1 >> 24)) * a.depth_scale;
            } else {
                int yy = y, xx = x;
                for (int k = 0; k < n; k++) {
                    const uint8_t* s = a.depth + (size_t)yy * stride + 1 + (size_t)2 * xx;
                    d[k] = (float)((unsigned)s[0] << 8 | s[1]) * a.depth_scale;
                    if (++xx == a.W) { xx = 0; yy++; }
                }
            }
        }
        if (whole) *reinterpret_cast<float4*>(a.depth_out + q0) = make_float4(d[0], d[1], d[2], d[3]);
        else for (int k = 0; k < n; k++) a.depth_out[q0 + k] = d[k];
        return;
    }
    if (kind == SEC_MASK_PNG || kind == SEC_MASK_RAW) {
        const size_t stride = (size_t)a.W + (kind == SEC_MASK_PNG ? 1 : 0), lead = kind == SEC_MASK_PNG ? 1 : 0;
        if (one_row) {
            *reinterpret_cast<unsigned*>(a.mask_out + q0) = load4(a.mask, (size_t)y * stride + lead + x);
        } else {
            int yy = y, xx = x;
            for (int k = 0; k < n; k++) {
                a.mask_out[q0 + k] = a.mask[(size_t)yy * stride + lead + xx];
                if (++xx == a.W) { xx = 0; yy++; }
            }
        }
        return;
    }
    unsigned px[4] = {0xff000000u, 0xff000000u, 0xff000000u, 0xff000000u};
    if (kind != SEC_COLOUR_BLACK) {
        const int bpp = kind == SEC_COLOUR_RGB ? 3 : (kind == SEC_COLOUR_RGBA ? 4 : 1);
        const size_t stride = (size_t)bpp * a.W + 1;
        if (one_row) {
            const size_t off = (size_t)y * stride + 1 + (size_t)bpp * x;
            if (bpp == 1) {
                const unsigned w = load4(a.colour, off);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned v = (w >> (8 * k)) & 255u;
                    if (kind == SEC_COLOUR_GREY) px[k] = rgba_of(v, v, v, 0);
                    else { const uint8_t* p = a.palette + 3 * v; px[k] = rgba_of(p[0], p[1], p[2], a.flip); }
                }
            } else if (bpp == 3) {
                const unsigned w0 = load4(a.colour, off), w1 = load4(a.colour, off + 4), w2 = load4(a.colour, off + 8);
                px[0] = rgba_of(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, a.flip);
                px[1] = rgba_of(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, a.flip);
                px[2] = rgba_of((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, a.flip);
                px[3] = rgba_of((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, a.flip);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned w = load4(a.colour, off + 4 * (size_t)k);   // alpha dropped
                    px[k] = rgba_of(w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, a.flip);
                }
            }
        } else {
            int yy = y, xx = x;
            for (int k = 0; k < n; k++) {
                const uint8_t* s = a.colour + (size_t)yy * stride + 1 + (size_t)bpp * xx;
                if (kind == SEC_COLOUR_GREY) px[k] = rgba_of(s[0], s[0], s[0], 0);
                else if (kind == SEC_COLOUR_PALETTE) { const uint8_t* p = a.palette + 3 * (unsigned)s[0]; px[k] = rgba_of(p[0], p[1], p[2], a.flip); }
                else px[k] = rgba_of(s[0], s[1], s[2], a.flip);
                if (++xx == a.W) { xx = 0; yy++; }
            }
        }
    }
    unsigned* out = reinterpret_cast<unsigned*>(a.rgba_out) + q0;
    if (whole) *reinterpret_cast<uint4*>(out) = make_uint4(px[0], px[1], px[2], px[3]);
    else for (int k = 0; k < n; k++) out[k] = px[k];
}

// the block table decides addresses on the device: every entry must be where a frame of this size puts it
bool exr_table_fits(const cf_image_desc& d, const cf_exr_block* t, size_t depth_bytes, uint32_t max_blocks)
{
    const int lpb = d.exr_lines_per_block, sample = d.exr_chan_half ? 2 : 4;
    if ((lpb != 1 && lpb != 16) || (d.exr_chan_half != 0 && d.exr_chan_half != 1)) return false;
    if (d.exr_line_bytes < d.width * sample || d.exr_line_bytes > 16 * d.width || (d.exr_line_bytes & 1)) return false;
    if (d.exr_chan_offset < 0 || (d.exr_chan_offset & 1) || (int64_t)d.exr_chan_offset + (int64_t)d.width * sample > d.exr_line_bytes) return false;
    if ((size_t)d.exr_line_bytes * d.height > depth_bytes) return false;
    const int blocks = (d.height + lpb - 1) / lpb;
    if (d.exr_blocks != blocks || (uint32_t)blocks > max_blocks) return false;
    for (int i = 0; i < blocks; i++) {
        const int first = i * lpb, lines = d.height - first < lpb ? d.height - first : lpb;
        if (t[i].first_line != (uint32_t)first || t[i].offset != (uint64_t)first * d.exr_line_bytes || t[i].bytes != (uint64_t)lines * d.exr_line_bytes ||
            t[i].stored_raw > 1)
            return false;
    }
    return true;
}

}  // namespace

extern "C" {

int cf_frame_decoder_enable_images(cf_frame_decoder* d)
{
    if (!d) return CF_EINVAL;
    if (d->img) return CF_OK;
    cf_ctx* ctx = d->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    ImageExt* e = new ImageExt();
    const size_t w = (size_t)d->max_w, h = (size_t)d->max_h;
    // every plane is followed by slack: the kernels fetch aligned 16-byte cells and 32-bit words that may reach past the last byte
    e->colour_bytes = (1 + 4 * w) * h; e->depth_bytes = 16 * w * h; e->mask_bytes = (1 + w) * h;
    e->off_depth = align256(e->colour_bytes + 16);
    e->off_mask = e->off_depth + align256(e->depth_bytes + 16);
    e->off_palette = e->off_mask + align256(e->mask_bytes + 16);
    e->off_blocks = e->off_palette + align256(768);
    e->bytes = e->off_blocks + align256(h * sizeof(cf_exr_block));
    auto fail = [&](hipError_t err, const char* what) {
        ctx->set_error(std::string("cf_frame_decoder_enable_images: ") + what + ": " + hipGetErrorString(err));
        image_ext_destroy(e);
        return err == hipErrorOutOfMemory ? CF_ENOMEM : CF_EHIP;
    };
    hipError_t err;
    for (int s = 0; s < d->slots; s++) {
        if ((err = hipHostMalloc(reinterpret_cast<void**>(&e->h[s]), e->bytes)) != hipSuccess) return fail(err, "pinned slot");
        memset(e->h[s], 0, e->bytes);
        if ((err = hipMalloc(reinterpret_cast<void**>(&e->d[s]), e->bytes)) != hipSuccess) return fail(err, "device slot");
        if ((err = hipMemset(e->d[s], 0, e->bytes)) != hipSuccess) return fail(err, "device slot");
        if ((err = hipMalloc(reinterpret_cast<void**>(&e->d_mask[s]), align256(w * h))) != hipSuccess) return fail(err, "mask frame");
    }
    d->img = e;
    return CF_OK;
}

int cf_frame_decoder_image_slot(cf_frame_decoder* d, int slot, cf_image_slot* out)
{
    if (!d || !out || slot < 0 || slot >= d->slots) return CF_EINVAL;
    if (!d->img) { d->ctx->set_error("cf_frame_decoder_image_slot: images were not enabled on this decoder"); return CF_ESTATE; }
    const ImageExt* e = d->img;
    uint8_t* base = e->h[slot];
    out->color = base; out->color_bytes = e->colour_bytes;
    out->depth = base + e->off_depth; out->depth_bytes = e->depth_bytes;
    out->mask = base + e->off_mask; out->mask_bytes = e->mask_bytes;
    out->palette = base + e->off_palette;
    out->blocks = reinterpret_cast<cf_exr_block*>(base + e->off_blocks); out->max_blocks = (uint32_t)d->max_h;
    return CF_OK;
}

int cf_frame_decoder_submit_images(cf_frame_decoder* d, int slot, const cf_image_desc* desc)
{
    if (!d || !desc || slot < 0 || slot >= d->slots) return CF_EINVAL;
    cf_ctx* ctx = d->ctx;
    if (!d->img) { ctx->set_error("cf_frame_decoder_submit_images: images were not enabled on this decoder"); return CF_ESTATE; }
    ImageExt* e = d->img;
    const cf_image_desc q = *desc;
    if (q.width < 1 || q.height < 1 || q.width > d->max_w || q.height > d->max_h) {
        ctx->set_error("cf_frame_decoder_submit_images: frame size outside the decoder's maximum");
        return CF_EINVAL;
    }
    const int ck = q.color_kind, dk = q.depth_kind, mk = q.mask_kind;
    const bool colour_ok = ck == CF_IMAGE_NONE || ck == CF_IMAGE_JPEG || ck == CF_IMAGE_RAW ||
                           (ck == CF_IMAGE_PNG && (q.png_color_type == 0 || q.png_color_type == 2 || q.png_color_type == 6 ||
                                                   (q.png_color_type == 3 && q.png_palette_entries >= 1 && q.png_palette_entries <= 256)));
    if (!colour_ok || (dk != CF_IMAGE_NONE && dk != CF_IMAGE_PNG && dk != CF_IMAGE_EXR) || (mk != CF_IMAGE_NONE && mk != CF_IMAGE_PNG && mk != CF_IMAGE_RAW)) {
        ctx->set_error("cf_frame_decoder_submit_images: a plane kind (or PNG colour type) this plane does not accept");
        return CF_EINVAL;
    }
    const size_t W = (size_t)q.width, H = (size_t)q.height, N = W * H;
    uint8_t *hs = e->h[slot], *ds = e->d[slot];
    std::vector<cf_exr_block> table;
    if (dk == CF_IMAGE_EXR) {
        const size_t blocks = q.exr_blocks >= 1 && q.exr_blocks <= d->max_h ? (size_t)q.exr_blocks : 0;
        const cf_exr_block* t = reinterpret_cast<const cf_exr_block*>(hs + e->off_blocks);
        table.assign(t, t + blocks);   // a copy: what is checked is what the kernel reads
        if (!blocks || !exr_table_fits(q, table.data(), e->depth_bytes, (uint32_t)d->max_h)) {
            ctx->set_error("cf_frame_decoder_submit_images: the slot's EXR block table does not describe a frame of this size");
            return CF_EINVAL;
        }
        memcpy(hs + e->off_blocks, table.data(), blocks * sizeof(cf_exr_block));
    }
    if (d->timing) { if (int r = frame_decoder_harvest(d, slot)) return r; }
    // as cf_frame_decoder_submit: the slot's frames may still be read by work the context's stream holds
    HIPCHK(ctx, hipEventRecord(d->consumed, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(d->stream, d->consumed, 0));
    PngArgs a;
    a.colour = ds; a.palette = ds + e->off_palette; a.depth = ds + e->off_depth; a.mask = ds + e->off_mask;
    a.rgba_out = d->d_rgba[slot]; a.depth_out = d->d_depth[slot]; a.mask_out = e->d_mask[slot];
    a.W = q.width; a.N = (int)N; a.flip = q.flip_colors != 0; a.groups = (int)((N + 1023) / 1024);
    a.depth_scale = q.depth_scale;
    a.sec[0] = a.sec[1] = a.sec[2] = SEC_OFF;
    // colour and copies first, so that the two launches below lie between the slot's timing events without a copy among them
    if (ck == CF_IMAGE_JPEG || ck == CF_IMAGE_RAW) {
        // the .klg path's kernels, storing the file's R, G, B unless flip_colors
        const int kind = ck == CF_IMAGE_JPEG ? CF_FRAME_COLOR_JPEG : CF_FRAME_COLOR_RAW;
        if (int r = frame_decoder_colour(d, slot, q.width, q.height, kind, q.flip_colors != 0, false)) return r;
    } else if (ck == CF_IMAGE_PNG) {
        const int ct = q.png_color_type, bpp = ct == 2 ? 3 : (ct == 6 ? 4 : 1);
        HIPCHK(ctx, hipMemcpyAsync(ds, hs, (1 + bpp * W) * H, hipMemcpyHostToDevice, d->stream));
        if (ct == 3) HIPCHK(ctx, hipMemcpyAsync(ds + e->off_palette, hs + e->off_palette, 768, hipMemcpyHostToDevice, d->stream));
        a.sec[0] = ct == 0 ? SEC_COLOUR_GREY : (ct == 2 ? SEC_COLOUR_RGB : (ct == 3 ? SEC_COLOUR_PALETTE : SEC_COLOUR_RGBA));
    } else {
        a.sec[0] = SEC_COLOUR_BLACK;
    }
    if (dk == CF_IMAGE_EXR) {
        HIPCHK(ctx, hipMemcpyAsync(ds + e->off_depth, hs + e->off_depth, (size_t)q.exr_line_bytes * H, hipMemcpyHostToDevice, d->stream));
        HIPCHK(ctx, hipMemcpyAsync(ds + e->off_blocks, hs + e->off_blocks, table.size() * sizeof(cf_exr_block), hipMemcpyHostToDevice, d->stream));
    } else if (dk == CF_IMAGE_PNG) {
        HIPCHK(ctx, hipMemcpyAsync(ds + e->off_depth, hs + e->off_depth, (1 + 2 * W) * H, hipMemcpyHostToDevice, d->stream));
        a.sec[1] = SEC_DEPTH_PNG;
    } else {
        a.sec[1] = SEC_DEPTH_ZERO;
    }
    if (mk != CF_IMAGE_NONE) {
        HIPCHK(ctx, hipMemcpyAsync(ds + e->off_mask, hs + e->off_mask, ((mk == CF_IMAGE_PNG ? 1 : 0) + W) * H, hipMemcpyHostToDevice, d->stream));
        a.sec[2] = mk == CF_IMAGE_PNG ? SEC_MASK_PNG : SEC_MASK_RAW;
    }
    const bool finish = a.sec[0] != SEC_OFF || a.sec[1] != SEC_OFF || a.sec[2] != SEC_OFF;
    if (d->timing) HIPCHK(ctx, hipEventRecord(d->tev[slot][0], d->stream));
    if (dk == CF_IMAGE_EXR) {
        ExrArgs x;
        x.raw = ds + e->off_depth; x.blocks = reinterpret_cast<const cf_exr_block*>(ds + e->off_blocks); x.depth_out = d->d_depth[slot];
        x.W = q.width; x.line_bytes = q.exr_line_bytes; x.chan_offset = q.exr_chan_offset; x.chan_half = q.exr_chan_half;
        hipLaunchKernelGGL(exr_depth_kernel, dim3((unsigned)table.size()), dim3(kScanThreads), 0, d->stream, x);
        HIPCHK(ctx, hipGetLastError());
    }
    if (d->timing) HIPCHK(ctx, hipEventRecord(d->tev[slot][1], d->stream));
    if (finish) {
        hipLaunchKernelGGL(png_finish_kernel, dim3(3 * a.groups), dim3(256), 0, d->stream, a);
        HIPCHK(ctx, hipGetLastError());
    }
    if (d->timing) {
        HIPCHK(ctx, hipEventRecord(d->tev[slot][2], d->stream));
        e->timed[slot] = true; e->timed_exr[slot] = dk == CF_IMAGE_EXR; e->timed_finish[slot] = finish;
    }
    HIPCHK(ctx, hipEventRecord(d->done[slot], d->stream));
    d->submitted[slot] = true;
    e->has_mask[slot] = mk != CF_IMAGE_NONE;
    return CF_OK;
}

int cf_frame_decoder_acquire_mask(cf_frame_decoder* d, int slot, int complete, const uint8_t** mask_dev)
{
    if (!d || !mask_dev || slot < 0 || slot >= d->slots) return CF_EINVAL;
    if (!d->img || !d->submitted[slot]) { d->ctx->set_error("cf_frame_decoder_acquire_mask: no image frame was submitted to this slot"); return CF_ESTATE; }
    if (complete) HIPCHK(d->ctx, hipEventSynchronize(d->done[slot]));
    else HIPCHK(d->ctx, hipStreamWaitEvent(d->ctx->stream, d->done[slot], 0));
    *mask_dev = d->img->has_mask[slot] ? d->img->d_mask[slot] : nullptr;
    return CF_OK;
}

int cf_frame_decoder_image_timing(cf_frame_decoder* d, double* exr_ms, uint64_t* exr_frames, double* finish_ms, uint64_t* finish_frames)
{
    if (!d) return CF_EINVAL;
    if (!d->img) { d->ctx->set_error("cf_frame_decoder_image_timing: images were not enabled on this decoder"); return CF_ESTATE; }
    HIPCHK(d->ctx, hipStreamSynchronize(d->stream));
    for (int s = 0; s < d->slots; s++) if (int r = frame_decoder_harvest(d, s)) return r;
    ImageExt* e = d->img;
    if (exr_ms) *exr_ms = e->exr_ms;
    if (exr_frames) *exr_frames = e->exr_frames;
    if (finish_ms) *finish_ms = e->finish_ms;
    if (finish_frames) *finish_frames = e->finish_frames;
    e->exr_ms = e->finish_ms = 0; e->exr_frames = e->finish_frames = 0;
    return CF_OK;
}

}  // extern "C"
