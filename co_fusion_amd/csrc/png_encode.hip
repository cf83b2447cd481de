// png_encode.hip -- the device half of the per-frame exports (cf_png_encoder_*): a device image becomes the
// bands of a complete PNG data stream in a pinned slot; host threads add the chunk framing and write (host/ExportWriter.cpp).
// One launch, one workgroup of 256 per band of R rows:
//   load      the band's rows and the row above them, as aligned words, into LDS (CF_PNG_LABELS: 255 -> 0 on the way)
//   filter    a wave per row: the five costs (sum of |int8| of the filtered bytes) reduced in the wave, the cheapest type (ties: the
//             lowest) written as [type][filtered bytes] into the band's stream S, also in LDS
//   runs      every thread owns a contiguous piece of S; per piece its first and last byte and the lengths of its leading and
//             trailing run are scanned over the workgroup, forward and backward (a segmented scan: eight steps each), which
//             gives a run that leaves its piece the full extent
//   tokens    a run of n is its literal, matches (258, distance 1) while 258 or more remain, then one match or up to two literals;
//             a token belongs to the thread that owns its first byte.  First walk: bit lengths; workgroup prefix sum; the fixed
//             form's size against the stored form's; second walk (fixed form only): the tokens are ORed into LDS words
//   Adler-32  of S from two 64-bit sums per thread (sum s_i and sum (L - i) s_i), added up in LDS, reduced mod 65521 once
//   output    the band's bytes as words to its place in the slot's device mirror, one table entry per band
// Integer arithmetic only; the stream is a function of the pixels, the channel count, R and the flags, stated byte for byte by
// tests/png_encode_ref.py.
#include <stdlib.h>
#include <string.h>

#include <string>

#include "cf_device.h"
#include "cf_host.h"

using namespace cf;

namespace {

constexpr int kMaxPngSlots = 16;
constexpr int kThreads = 256;
constexpr int kStoredHeader = 5;   // 00 LEN ~LEN

struct PngArgs {
    const uint8_t* src;
    uint8_t* data;         // the slot's band area (device mirror), 256-byte aligned
    cf_png_band* table;
    int rb;                // bytes of an image row: width * channels
    int height, channels, rows, labels;
    uint32_t stride;       // of a band's place in the band area, a multiple of 4
    uint32_t off_b;        // where the second LDS region starts (bytes, a multiple of 4)
};

typedef unsigned long long u64;

__device__ __forceinline__ int abs8(int f) { const int v = f & 255; return v < 128 ? v : 256 - v; }

__device__ __forceinline__ int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filtered(int type, int x, int a, int b, int c)
{
    switch (type) {
    case 0: return x;
    case 1: return x - a;
    case 2: return x - b;
    case 3: return x - ((a + b) >> 1);
    default: return x - paeth(a, b, c);
    }
}

// a token of the fixed code (RFC 1951 3.2.6) as it lies in the stream: the Huffman code reversed (it is sent most significant bit
// first), extra bits and the 5-bit distance code 0 above it.  At most 8 + 5 + 5 bits.
__device__ __forceinline__ uint32_t literal_token(int v, int* nbits)
{
    if (v < 144) { *nbits = 8; return __brev((uint32_t)(0x30 + v)) >> 24; }
    *nbits = 9;
    return __brev((uint32_t)(0x190 + v - 144)) >> 23;
}
__device__ __forceinline__ uint32_t match_token(int len, int* nbits)   // 3 <= len <= 258, distance 1
{
    const int l = len - 3;
    int sym, eb = 0, ev = 0;
    if (len == 258) sym = 285;
    else if (l < 8) sym = 257 + l;
    else {
        eb = (31 - __clz(l)) - 2;
        sym = 257 + 4 * (eb + 1) + ((l >> eb) & 3);
        ev = l & ((1 << eb) - 1);
    }
    int n;
    uint32_t code;
    if (sym < 280) { n = 7; code = __brev((uint32_t)(sym - 256)) >> 25; }
    else { n = 8; code = __brev((uint32_t)(0xC0 + sym - 280)) >> 24; }
    *nbits = n + eb + 5;
    return code | ((uint32_t)ev << n);
}

__device__ __forceinline__ void put_bits(uint32_t* out, uint32_t pos, uint32_t val, int nbits)
{
    const uint32_t w = pos >> 5, sh = pos & 31;
    atomicOr(&out[w], val << sh);
    if (sh + (uint32_t)nbits > 32) atomicOr(&out[w + 1], val >> (32 - sh));
}

// The tokens that START in [b0, b1) of the band's stream, in order: counted (EMIT = false) or ORed into `out` from bit `pos` on.
// back: how many bytes in front of b0 belong to the run of S[b0]; fwd: how many behind b1 - 1 to the run of S[b1 - 1].
template <bool EMIT>
__device__ __forceinline__ uint32_t walk(const uint8_t* S, int b0, int b1, int back, int fwd, uint32_t* out, uint32_t pos)
{
    uint32_t bits = 0;
    auto emit = [&](uint32_t val, int n) {
        if constexpr (EMIT) put_bits(out, pos + bits, val, n);
        bits += (uint32_t)n;
    };
    int i = b0;
    while (i < b1) {
        const int v = S[i];
        int j = i + 1;
        while (j < b1 && S[j] == v) j++;
        const int head = i - (i == b0 ? back : 0), end = j + (j == b1 ? fwd : 0);
        const int m = end - head - 1;                  // what follows the run's literal
        const int lo = i - head, hi = j - head;        // this thread's part of the run, relative to its head
        const int full = m >= 258 ? m / 258 : 0, rest = m - full * 258;   // (most runs are short: no division for them)
        int n;
        if (lo == 0) { const uint32_t t = literal_token(v, &n); emit(t, n); }
        if (full > 0) {
            const uint32_t t = match_token(258, &n);
            for (int k = lo <= 1 ? 0 : (lo - 1 + 257) / 258; k < full && 1 + 258 * k < hi; k++) emit(t, n);
        }
        const int base = 1 + 258 * full;
        if (rest >= 3) {
            if (base >= lo && base < hi) { const uint32_t t = match_token(rest, &n); emit(t, n); }
        } else {
            const int q0 = base > lo ? base : lo, q1 = base + rest < hi ? base + rest : hi;
            if (q0 < q1) {
                const uint32_t t = literal_token(v, &n);
                for (int q = q0; q < q1; q++) emit(t, n);
            }
        }
        i = j;
    }
    return bits;
}

// A stretch of the stream as the run search sees it: its first and last byte, whether it is one run, its length and the length of the
// run it ends with.  x: first | last << 8 | one run << 16 | not empty << 17; y: length | run at the end << 16 (both <= 65535).
__device__ __forceinline__ uint2 make_stretch(int first, int last, bool one_run, int len, int tail)
{
    return make_uint2((uint32_t)first | (uint32_t)last << 8 | (one_run ? 1u << 16 : 0u) | (len > 0 ? 1u << 17 : 0u), (uint32_t)len | (uint32_t)tail << 16);
}
// the stretch A followed by the stretch B (associative; an empty stretch is the identity)
__device__ __forceinline__ uint2 join_stretches(uint2 A, uint2 B)
{
    if (!(A.x >> 17 & 1)) return B;
    if (!(B.x >> 17 & 1)) return A;
    const bool meet = (A.x >> 8 & 255) == (B.x & 255), b_one = B.x >> 16 & 1;
    const uint32_t tail = (b_one && meet) ? (A.y >> 16) + (B.y & 0xffffu) : B.y >> 16;
    const uint32_t one = (A.x >> 16 & 1) && b_one && meet;
    return make_uint2((A.x & 255) | (B.x & 0xff00u) | one << 16 | 1u << 17, ((A.y & 0xffffu) + (B.y & 0xffffu)) | tail << 16);
}
// Exclusive scan of the workgroup's stretches in the order of `at` (a permutation of 0..255 over the threads): what lies in front of
// this thread's stretch, joined.  Eight steps in two LDS buffers; every thread of the workgroup calls it.
__device__ __forceinline__ uint2 stretch_in_front(uint2 (*buf)[kThreads], int at, uint2 mine)
{
    int cur = 0;
    buf[0][at] = mine;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        uint2 v = buf[cur][at];
        if (at >= d) v = join_stretches(buf[cur][at - d], v);
        buf[cur ^ 1][at] = v;
        __syncthreads();
        cur ^= 1;
    }
    const uint2 front = at > 0 ? buf[cur][at - 1] : make_uint2(0, 0);
    __syncthreads();   // (the buffers are free again)
    return front;
}

__global__ void __launch_bounds__(kThreads) png_band_kernel(const PngArgs a)
{
    extern __shared__ uint32_t lds[];
    __shared__ uint2 s_stretch[2][kThreads];
    __shared__ uint32_t s_wave[kThreads / 64];
    __shared__ u64 s_adler[2];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int band = blockIdx.x, rb = a.rb;
    const int y0 = band * a.rows;
    const int nr = a.height - y0 < a.rows ? a.height - y0 : a.rows;
    const int L = nr * (rb + 1);                               // <= 65535 (checked at creation)
    uint8_t* const front = reinterpret_cast<uint8_t*>(lds);    // [stored header][S]
    uint8_t* const S = front + kStoredHeader;
    uint8_t* const region_b = front + a.off_b;                 // the raw rows, later the packed fixed form

    // ---- load: rows y0 - 1 .. y0 + nr - 1 are contiguous in the image; whole aligned words, LDS and global equally misaligned ----
    const bool top = y0 == 0;
    const uint8_t* g0 = a.src + (top ? (size_t)0 : (size_t)(y0 - 1) * rb);
    const int nbytes = (nr + (top ? 0 : 1)) * rb;
    const int mis = (int)(reinterpret_cast<uintptr_t>(g0) & 3);
    const int lead_rows = top ? rb : 0;                        // the row above the image: zeros, written below
    const int pad = (mis - lead_rows) & 3;
    uint8_t* const raw = region_b + pad;                       // raw[(r + 1) * rb + x]: byte x of the band's row r
    {
        uint32_t* lw = reinterpret_cast<uint32_t*>(raw + lead_rows - mis);
        const uint32_t* gw = reinterpret_cast<const uint32_t*>(g0 - mis);
        const int nw = (mis + nbytes + 3) >> 2;
        for (int i = tid; i < nw; i += kThreads) {
            uint32_t v = gw[i];
            if (a.labels) {
                if ((v & 0x000000ffu) == 0x000000ffu) v &= ~0x000000ffu;
                if ((v & 0x0000ff00u) == 0x0000ff00u) v &= ~0x0000ff00u;
                if ((v & 0x00ff0000u) == 0x00ff0000u) v &= ~0x00ff0000u;
                if ((v & 0xff000000u) == 0xff000000u) v &= ~0xff000000u;
            }
            lw[i] = v;
        }
    }
    if (tid == 0) { s_adler[0] = 0; s_adler[1] = 0; }
    __syncthreads();
    if (top) for (int i = tid; i < rb; i += kThreads) raw[i] = 0;   // (after the load: its first word may reach into this row)
    __syncthreads();

    // ---- filter: a wave per row ----
    const int bpp = a.channels;
    for (int r = wave; r < nr; r += kThreads / 64) {
        const uint8_t *cur = raw + (size_t)(r + 1) * rb, *up = raw + (size_t)r * rb;
        int cost[5] = {0, 0, 0, 0, 0};
        for (int x = lane; x < rb; x += 64) {
            const int X = cur[x], B = up[x], A = x >= bpp ? cur[x - bpp] : 0, Cc = x >= bpp ? up[x - bpp] : 0;
            cost[0] += abs8(X); cost[1] += abs8(X - A); cost[2] += abs8(X - B); cost[3] += abs8(X - ((A + B) >> 1));
            cost[4] += abs8(X - paeth(A, B, Cc));
        }
#pragma unroll
        for (int k = 0; k < 5; k++)
            for (int d = 32; d >= 1; d >>= 1) cost[k] += __shfl_xor(cost[k], d, 64);
        int type = 0, best = cost[0];
#pragma unroll
        for (int k = 1; k < 5; k++) if (cost[k] < best) { best = cost[k]; type = k; }
        uint8_t* dst = S + (size_t)r * (rb + 1);
        if (lane == 0) dst[0] = (uint8_t)type;
        for (int x = lane; x < rb; x += 64) {
            const int X = cur[x], B = up[x], A = x >= bpp ? cur[x - bpp] : 0, Cc = x >= bpp ? up[x - bpp] : 0;
            dst[1 + x] = (uint8_t)filtered(type, X, A, B, Cc);
        }
    }
    __syncthreads();   // S is complete; the raw rows are dead from here on

    // ---- runs: each thread's piece of S ----
    const int chunk = (L + kThreads - 1) / kThreads;
    const int b0 = tid * chunk < L ? tid * chunk : L, b1 = b0 + chunk < L ? b0 + chunk : L;
    int first = 0, last = 0, lead = 0, trail = 0;
    if (b0 < b1) {
        u64 sa = 0, sb = 0;
        first = S[b0]; last = S[b1 - 1];
        lead = 1; while (b0 + lead < b1 && S[b0 + lead] == first) lead++;
        trail = 1; while (b1 - 1 - trail >= b0 && S[b1 - 1 - trail] == last) trail++;
        for (int i = b0; i < b1; i++) { const u64 s = S[i]; sa += s; sb += s * (u64)(L - i); }
        atomicAdd(&s_adler[0], sa); atomicAdd(&s_adler[1], sb);
    }
    // how far the run of the piece's first byte reaches back into the pieces in front, and that of its last byte on into the pieces
    // behind: two scans over the pieces, the second in reversed order with the ends exchanged
    const bool one_run = lead == b1 - b0;
    const uint2 ahead = stretch_in_front(s_stretch, tid, make_stretch(first, last, one_run, b1 - b0, trail));
    const uint2 behind = stretch_in_front(s_stretch, kThreads - 1 - tid, make_stretch(last, first, one_run, b1 - b0, lead));
    const int back = (b0 < b1 && (ahead.x >> 17 & 1) && (int)(ahead.x >> 8 & 255) == first) ? (int)(ahead.y >> 16) : 0;
    const int fwd = (b0 < b1 && (behind.x >> 17 & 1) && (int)(behind.x >> 8 & 255) == last) ? (int)(behind.y >> 16) : 0;

    // ---- tokens: bit lengths, their prefix sum, the choice of the form ----
    const uint32_t mine = walk<false>(S, b0, b1, back, fwd, nullptr, 0);
    uint32_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < kThreads / 64; k++) { if (k < wave) before += s_wave[k]; total += s_wave[k]; }
    const uint32_t fixed_bits = 3 + total + 7 + 3;             // header, tokens, end-of-block, the header of the empty stored block
    const uint32_t fixed_bytes = ((fixed_bits + 7) >> 3) + 4, stored_bytes = (uint32_t)L + kStoredHeader;
    const bool stored = stored_bytes < fixed_bytes;
    uint32_t* const dst = reinterpret_cast<uint32_t*>(a.data + (size_t)band * a.stride);
    uint32_t bytes;
    if (stored) {
        if (tid == 0) {
            front[0] = 0; front[1] = (uint8_t)(L & 255); front[2] = (uint8_t)(L >> 8);
            front[3] = (uint8_t)(~L & 255); front[4] = (uint8_t)((~L >> 8) & 255);
        }
        __syncthreads();
        bytes = stored_bytes;
        for (uint32_t i = tid; i < (bytes + 3) >> 2; i += kThreads) dst[i] = lds[i];
    } else {
        uint32_t* const out = reinterpret_cast<uint32_t*>(region_b);
        bytes = fixed_bytes;
        const uint32_t words = (bytes + 3) >> 2;
        for (uint32_t i = tid; i <= words; i += kThreads) out[i] = 0;      // (one more: a token's second word)
        __syncthreads();
        if (tid == 0) put_bits(out, 0, 2u, 3);                             // BFINAL = 0, BTYPE = 01
        walk<true>(S, b0, b1, back, fwd, out, 3 + before + incl - mine);
        __syncthreads();
        if (tid == 0) {   // 00 00 FF FF of the empty stored block, behind the padded bits
            uint8_t* o8 = reinterpret_cast<uint8_t*>(out);
            o8[bytes - 2] = 0xff; o8[bytes - 1] = 0xff;
        }
        __syncthreads();
        for (uint32_t i = tid; i < words; i += kThreads) dst[i] = out[i];
    }
    if (tid == 0) {
        cf_png_band e;
        e.offset = (uint32_t)band * a.stride; e.bytes = bytes;
        e.adler = (uint32_t)(((u64)L + s_adler[1]) % 65521u) << 16 | (uint32_t)((1 + s_adler[0]) % 65521u);
        e.stream_bytes = (uint32_t)L;
        a.table[band] = e;
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t round4(uint32_t v) { return (v + 3) & ~3u; }

// LDS of a launch: [stored header + S, rounded] [the raw rows with their alignment slack | the packed fixed form]
void lds_layout(int rb, int rows, uint32_t* off_b, uint32_t* total)
{
    const uint32_t L = (uint32_t)rows * (uint32_t)(rb + 1);
    *off_b = round4(L + kStoredHeader) + 4;
    const uint32_t raw = round4((uint32_t)(rows + 1) * (uint32_t)rb + 3 + 3) + 4, packed = round4(L + kStoredHeader) + 8;
    *total = *off_b + (raw > packed ? raw : packed);
}

}  // namespace

struct cf_png_encoder {
    cf_ctx* ctx = nullptr;
    int max_w = 0, max_h = 0, slots = 0, rows = 0;
    int max_bands = 0;
    size_t table_bytes = 0, slot_bytes = 0;
    hipStream_t stream = nullptr;           // the copies to the pinned slots
    hipEvent_t encoded = nullptr;           // the kernel on the context's stream -> the copy
    hipEvent_t done[kMaxPngSlots]{};
    uint8_t* h_slot[kMaxPngSlots]{};        // pinned: [band table][band area]
    uint8_t* d_slot[kMaxPngSlots]{};
    bool submitted[kMaxPngSlots]{};
    cf_png_stream info[kMaxPngSlots]{};
    // diagnostics (cf_png_encoder_timing)
    bool timing = false;
    hipEvent_t tev[kMaxPngSlots][2]{};
    bool timed[kMaxPngSlots]{};
    double kernel_ms = 0;
    uint64_t images = 0;
};

namespace {

int harvest(cf_png_encoder* e, int s)
{
    if (!e->timed[s]) return CF_OK;
    HIPCHK(e->ctx, hipEventSynchronize(e->tev[s][1]));
    float ms = 0;
    HIPCHK(e->ctx, hipEventElapsedTime(&ms, e->tev[s][0], e->tev[s][1]));
    e->kernel_ms += ms; e->images++;
    e->timed[s] = false;
    return CF_OK;
}

}  // namespace

extern "C" {

int cf_png_encoder_create(cf_ctx* ctx, int max_w, int max_h, int slots, int rows_per_band, cf_png_encoder** out)
{
    if (!ctx || !out) return CF_EINVAL;
    if (max_w < 1 || max_h < 1 || max_w > 16384 || max_h > 16384 || slots < 2 || slots > kMaxPngSlots) {
        ctx->set_error("cf_png_encoder_create: an image of 1..16384 pixels a side and 2..16 slots");
        return CF_EINVAL;
    }
    if (rows_per_band < 1 || (int64_t)(1 + 4 * (int64_t)max_w) * rows_per_band > 65535) {
        ctx->set_error("cf_png_encoder_create: rows_per_band >= 1 with (1 + 4 * max_w) * rows_per_band <= 65535 (a band is at most one stored block)");
        return CF_EINVAL;
    }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int rows = rows_per_band < max_h ? rows_per_band : max_h;
    uint32_t off_b = 0, lds_bytes = 0;
    lds_layout(4 * max_w, rows, &off_b, &lds_bytes);
    int lds_limit = 0;
    HIPCHK(ctx, hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->cfg.device));
    if ((int64_t)lds_bytes + 4096 > lds_limit) {
        ctx->set_error("cf_png_encoder_create: a band of rows_per_band rows of max_w RGBA pixels and its output do not fit the LDS of a workgroup");
        return CF_EINVAL;
    }
    cf_png_encoder* e = new cf_png_encoder();
    e->ctx = ctx; e->max_w = max_w; e->max_h = max_h; e->slots = slots; e->rows = rows_per_band;
    e->max_bands = (max_h + rows_per_band - 1) / rows_per_band;
    e->table_bytes = align256((size_t)e->max_bands * sizeof(cf_png_band));
    e->slot_bytes = e->table_bytes + (size_t)e->max_bands * round4((uint32_t)rows * (uint32_t)(4 * max_w + 1) + 16);
    auto fail = [&](hipError_t err, const char* what) {
        ctx->set_error(std::string("cf_png_encoder_create: ") + what + ": " + hipGetErrorString(err));
        cf_png_encoder_destroy(e);
        return err == hipErrorOutOfMemory ? CF_ENOMEM : CF_EHIP;
    };
    hipError_t err;
    if (lds_bytes > 48 * 1024) {   // (a launch is checked on its own; this only lifts the default ceiling of dynamic LDS where there is one)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(png_band_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        (void)hipGetLastError();
    }
    if ((err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return fail(err, "stream");
    if ((err = hipEventCreateWithFlags(&e->encoded, hipEventDisableTiming)) != hipSuccess) return fail(err, "event");
    for (int s = 0; s < slots; s++) {
        if ((err = hipEventCreateWithFlags(&e->done[s], hipEventDisableTiming)) != hipSuccess) return fail(err, "event");
        for (int k = 0; k < 2; k++) if ((err = hipEventCreate(&e->tev[s][k])) != hipSuccess) return fail(err, "event");
        if ((err = hipHostMalloc(reinterpret_cast<void**>(&e->h_slot[s]), e->slot_bytes)) != hipSuccess) return fail(err, "pinned slot");
        if ((err = hipMalloc(reinterpret_cast<void**>(&e->d_slot[s]), e->slot_bytes)) != hipSuccess) return fail(err, "device slot");
    }
    *out = e;
    return CF_OK;
}

void cf_png_encoder_destroy(cf_png_encoder* e)
{
    if (!e) return;
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (int s = 0; s < kMaxPngSlots; s++) {
        if (e->timed[s]) (void)hipEventSynchronize(e->tev[s][1]);
        if (e->done[s]) (void)hipEventDestroy(e->done[s]);
        for (int k = 0; k < 2; k++) if (e->tev[s][k]) (void)hipEventDestroy(e->tev[s][k]);
        if (e->h_slot[s]) (void)hipHostFree(e->h_slot[s]);
        if (e->d_slot[s]) (void)hipFree(e->d_slot[s]);
    }
    if (e->encoded) (void)hipEventDestroy(e->encoded);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int cf_png_encoder_submit(cf_png_encoder* e, int slot, const void* src_dev, int width, int height, int channels, int flags)
{
    if (!e || slot < 0 || slot >= e->slots) return CF_EINVAL;
    cf_ctx* ctx = e->ctx;
    if (!src_dev || width < 1 || height < 1 || width > e->max_w || height > e->max_h || (channels != 1 && channels != 4) ||
        (flags & ~CF_PNG_LABELS) || ((flags & CF_PNG_LABELS) && channels != 1)) {
        ctx->set_error("cf_png_encoder_submit: an image of 1 or 4 channels within the encoder's maximum size; CF_PNG_LABELS on grey only");
        return CF_EINVAL;
    }
    if (e->timing) { if (int r = harvest(e, slot)) return r; }
    hipStream_t cs = ctx->cur();
    // a copy of this slot's last image may still read the device mirror the kernel is about to write
    if (e->submitted[slot]) HIPCHK(ctx, hipStreamWaitEvent(cs, e->done[slot], 0));
    PngArgs a;
    a.src = static_cast<const uint8_t*>(src_dev);
    a.table = reinterpret_cast<cf_png_band*>(e->d_slot[slot]);
    a.data = e->d_slot[slot] + e->table_bytes;
    a.rb = width * channels; a.height = height; a.channels = channels; a.rows = e->rows; a.labels = (flags & CF_PNG_LABELS) ? 1 : 0;
    const int rows = e->rows < height ? e->rows : height;
    a.stride = round4((uint32_t)rows * (uint32_t)(a.rb + 1) + 16);
    uint32_t lds_bytes = 0;
    lds_layout(a.rb, rows, &a.off_b, &lds_bytes);
    const int bands = (height + e->rows - 1) / e->rows;
    const size_t used = e->table_bytes + (size_t)bands * a.stride;   // <= slot_bytes: the maximum image has the widest stride and the most bands
    if (e->timing) HIPCHK(ctx, hipEventRecord(e->tev[slot][0], cs));
    hipLaunchKernelGGL(png_band_kernel, dim3(bands), dim3(kThreads), lds_bytes, cs, a);
    HIPCHK(ctx, hipGetLastError());
    if (e->timing) { HIPCHK(ctx, hipEventRecord(e->tev[slot][1], cs)); e->timed[slot] = true; }
    HIPCHK(ctx, hipEventRecord(e->encoded, cs));
    HIPCHK(ctx, hipStreamWaitEvent(e->stream, e->encoded, 0));
    HIPCHK(ctx, hipMemcpyAsync(e->h_slot[slot], e->d_slot[slot], used, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(ctx, hipEventRecord(e->done[slot], e->stream));
    cf_png_stream& i = e->info[slot];
    i.width = width; i.height = height; i.channels = channels; i.rows_per_band = e->rows; i.bands = bands;
    i.table = reinterpret_cast<const cf_png_band*>(e->h_slot[slot]);
    i.data = e->h_slot[slot] + e->table_bytes;
    i.data_bytes = (uint64_t)bands * a.stride;
    e->submitted[slot] = true;
    return CF_OK;
}

int cf_png_encoder_acquire(cf_png_encoder* e, int slot, cf_png_stream* out)
{
    if (!e || !out || slot < 0 || slot >= e->slots) return CF_EINVAL;
    if (!e->submitted[slot]) { e->ctx->set_error("cf_png_encoder_acquire: nothing was submitted to this slot"); return CF_ESTATE; }
    HIPCHK(e->ctx, hipEventSynchronize(e->done[slot]));
    *out = e->info[slot];
    return CF_OK;
}

int cf_png_encoder_timing(cf_png_encoder* e, int on, double* kernel_ms, uint64_t* images)
{
    if (!e) return CF_EINVAL;
    for (int s = 0; s < e->slots; s++) if (int r = harvest(e, s)) return r;
    if (kernel_ms) *kernel_ms = e->kernel_ms;
    if (images) *images = e->images;
    e->kernel_ms = 0; e->images = 0;
    e->timing = on != 0;
    return CF_OK;
}

}  // extern "C"
