// render.hip -- the scene renderer: every model's surfel map drawn as disc splats into one view, depth-tested against the others.
//
// What the reference's viewer draws (Core/Model/Model.cpp:274-314 with draw_global_surface.{vert,geom,frag}, objects placed by
// view * globalPose * modelPose^-1, GUI/MainController.cpp:570-600), restated as three compute passes in the style of the splat
// prediction (surf_splat_dev.h):
//   render_rays_kernel     the per-pixel view rays of the call's intrinsics (they depend on the view only)
//   render_raster_kernel   all items' surfels in one launch, four lanes per surfel, 64-bit (depth bits << 32 | draw index) atomicMin
//                          keys; a footprint of more than kBigArea pixels is appended to an overflow list instead, in tiles of kTile
//   render_big_kernel      one workgroup per listed tile: a 300 x 300 close-up splat is 90 000 fragments, which would serialise
//                          the four lanes of one surfel for the whole launch
//   render_resolve_kernel  one thread per pixel: decodes the key, recomputes the winning fragment, writes every requested output and
//                          leaves the key buffer cleared (and the overflow list empty) for the next call
// Coverage, depth test and colours are specified in DESIGN.md ("Scene rendering"); tests/render_ref.py restates them in numpy f32 in
// this file's operation order (no FMA contraction: the library's -ffp-contract=off), and the GPU tests compare bit for bit.
// The renderer owns all of its memory and touches nothing the frame loop reads or writes.
#include <math.h>
#include <string.h>

#include <string>

#include "cf_host.h"
#include "cf_surfel_device.h"

namespace cf {
namespace rnd {

constexpr int kB = 256;
constexpr int kBigArea = 256;                // bounding boxes of more pixels go to the overflow list ...
constexpr int kTile = 4096;                  // ... as tiles of this many pixels (row-major over the box), one workgroup each
constexpr unsigned kBigCap = 1u << 18;       // overflow list entries; beyond them the four lanes draw the surfel themselves
constexpr int kBigGrid = 1024;               // workgroups of the overflow pass (they stride over the list)
constexpr unsigned long long kEmpty = ~0ull;

__device__ __forceinline__ unsigned long long zkey(float z, unsigned id)
{  // order-preserving depth bits (z > near > 0 here) above the draw index
    return ((unsigned long long)(__float_as_uint(z) | 0x80000000u) << 32) | id;
}

struct ItemDev {             // one model of a call (uploaded per call; the resolve pass finds a draw index's item by `base`)
    const float4* surfels;
    unsigned count, base;    // base: draw index of surfel 0
    int blk_begin;           // first workgroup of the raster grid
    float thresh;
    int model_id, mode;
    Mat4 M;                  // model -> camera
    float R[9];              // model -> world rotation (world-frame normals)
    int pad[3];
};

struct ViewDev {
    cf_cam cam; int W, H;
    float near_z, far_z;
    int flags, tick, time_delta;
    int n_items;
    const ItemDev* items;
    float4* rays;
    unsigned long long* keys;
    uint2* big; unsigned* big_count;
};

struct OutDev {
    uchar4* rgba[CF_RENDER_MAX_COLOUR];
    int mode[CF_RENDER_MAX_COLOUR];
    int n_rgba;
    float* depth;
    uint8_t* label;
};

// the label palette: 16 colours of well separated hue and lightness, repeated over the 255 ids; entry 255 ("none") is black
__constant__ unsigned char kPaletteBase[16][3] = {
    {230, 25, 75}, {60, 180, 75}, {255, 225, 25}, {0, 130, 200}, {245, 130, 48}, {145, 30, 180}, {70, 240, 240}, {240, 50, 230},
    {210, 245, 60}, {250, 190, 212}, {0, 128, 128}, {220, 190, 255}, {170, 110, 40}, {255, 250, 200}, {128, 0, 0}, {170, 255, 195}};
static const unsigned char kPaletteHost[16][3] = {
    {230, 25, 75}, {60, 180, 75}, {255, 225, 25}, {0, 130, 200}, {245, 130, 48}, {145, 30, 180}, {70, 240, 240}, {240, 50, 230},
    {210, 245, 60}, {250, 190, 212}, {0, 128, 128}, {220, 190, 255}, {170, 110, 40}, {255, 250, 200}, {128, 0, 0}, {170, 255, 195}};

// the splat of one surfel in the view: camera-frame centre and normal, squared radius, plane offset, pixel bounding box
struct Setup { f3 ph, n; float r2, pn; int x_lo, x_hi, y_lo, y_hi; };

__device__ __forceinline__ bool render_setup(const float4 pc, const float4 nr, const Mat4& M, const ViewDev& v, Setup& s)
{
    s.ph = xform_point(M, f3{pc.x, pc.y, pc.z});
    s.n = normalized(xform_dir(M, f3{nr.x, nr.y, nr.z}));
    const float rad = nr.w;
    s.r2 = rad * rad;
    // the reference's quad: half-diagonals x1, y1 of length radius * sqrt 2 in the surfel's plane
    const f3 x1n = normalized(f3{s.n.y - s.n.z, -s.n.x, s.n.x});
    const float h = rad * 1.41421356f;
    const f3 x1 = {x1n.x * h, x1n.y * h, x1n.z * h};
    const f3 y1 = cross(s.n, x1);
    const f3 c[4] = {s.ph + x1, s.ph + y1, s.ph - y1, s.ph - x1};
    float xmin = 0, xmax = 0, ymin = 0, ymax = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!(c[k].z > v.near_z)) return false;   // a corner at or behind the near plane: skipped (GL would clip the quad)
        const float px = ((v.cam.fx * c[k].x) / c[k].z) + v.cam.cx, py = ((v.cam.fy * c[k].y) / c[k].z) + v.cam.cy;
        xmin = k ? fminf(xmin, px) : px; xmax = k ? fmaxf(xmax, px) : px;
        ymin = k ? fminf(ymin, py) : py; ymax = k ? fmaxf(ymax, py) : py;
    }
    // the disc lies inside the quad, so the centres of its pixels lie inside the quad's box; 0.01 pixel of margin keeps the box
    // conservative under rounding (the fragment test alone decides coverage)
    const float xl = fmaxf(xmin - 0.51f, -1.0f), xh = fminf(xmax - 0.49f, (float)v.W);
    const float yl = fmaxf(ymin - 0.51f, -1.0f), yh = fminf(ymax - 0.49f, (float)v.H);
    if (!(xl <= xh) || !(yl <= yh)) return false;
    s.x_lo = max((int)ceilf(xl), 0); s.x_hi = min((int)floorf(xh), v.W - 1);
    s.y_lo = max((int)ceilf(yl), 0); s.y_hi = min((int)floorf(yh), v.H - 1);
    if (s.x_lo > s.x_hi || s.y_lo > s.y_hi) return false;
    s.pn = dot(s.ph, s.n);
    return true;
}

// the ray through the pixel centre meets the surfel's plane at cp: covered when |cp - centre| <= radius and near < cp.z < far
__device__ __forceinline__ bool render_fragment(const Setup& s, const float4 lr, float near_z, float far_z, f3& cp)
{
    const f3 l = {lr.x, lr.y, lr.z};
    const float k = s.pn / dot(l, s.n);
    cp = f3{k * l.x, k * l.y, k * l.z};
    const f3 diff = cp - s.ph;
    if (!(dot(diff, diff) <= s.r2)) return false;
    return cp.z > near_z && cp.z < far_z;
}

__device__ __forceinline__ int find_item_by_block(const ViewDev& v, int b)
{  // last item whose first workgroup is <= b
    int lo = 0, hi = v.n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (v.items[mid].blk_begin <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int find_item_by_index(const ViewDev& v, unsigned gid)
{  // last item whose first draw index is <= gid (an empty item shares its base with the next one, which then wins)
    int lo = 0, hi = v.n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (v.items[mid].base <= gid) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool drawn(const ItemDev& it, const float4 pc, int flags)
{
    return pc.w > it.thresh || (flags & CF_RENDER_UNSTABLE);
}

__global__ void __launch_bounds__(kB) render_rays_kernel(const ViewDev v)
{
    const int q = blockIdx.x * kB + threadIdx.x;
    if (q >= v.W * v.H) return;
    const int py = q / v.W, px = q - py * v.W;
    const float fx_ = (float)px + 0.5f, fy_ = (float)py + 0.5f;
    const f3 l = normalized(f3{(fx_ - v.cam.cx) / v.cam.fx, (fy_ - v.cam.cy) / v.cam.fy, 1.0f});
    v.rays[q] = make_float4(l.x, l.y, l.z, 0.f);
}

// four lanes per surfel (as splat_raster_kernel); the grid is [item 0's workgroups | item 1's | ...]
__global__ void __launch_bounds__(kB) render_raster_kernel(const ViewDev v)
{
    const int b = (int)blockIdx.x;
    const int k = find_item_by_block(v, b);
    const ItemDev& it = v.items[k];
    const unsigned gt = (unsigned)(b - it.blk_begin) * kB + threadIdx.x;
    const unsigned id = gt >> 2;
    const int sub = (int)(gt & 3u);
    if (id >= it.count) return;
    const float4* __restrict__ sp = it.surfels + (size_t)id * 3;
    const float4 pc = sp[0];
    if (!drawn(it, pc, v.flags)) return;
    Setup s;
    if (!render_setup(pc, sp[2], it.M, v, s)) return;
    const int w = s.x_hi - s.x_lo + 1, h = s.y_hi - s.y_lo + 1;
    if (w * h > kBigArea) {
        // the four lanes of the surfel are neighbours in the wave and took the same decisions: lane 0 reserves the tiles, all learn
        // where they start
        const unsigned tiles = (unsigned)((w * h + kTile - 1) / kTile);
        unsigned slot = 0;
        if (sub == 0) slot = atomicAdd(v.big_count, tiles);
        slot = (unsigned)__shfl((int)slot, (int)(threadIdx.x & 63u) & ~3, 64);
        for (unsigned t = sub; t < tiles && slot + t < kBigCap; t += 4) v.big[slot + t] = make_uint2(id, (unsigned)k | (t << 8));
        if (slot + tiles <= kBigCap) return;
        // list full: the lanes draw the surfel themselves (tiles that did get listed draw the same fragments again: atomicMin)
    }
    const unsigned gid = it.base + id;
    int fx = sub, fy = 0;
    while (fx >= w) { fx -= w; fy++; }
    while (fy < h) {
        const int px = s.x_lo + fx, py = s.y_lo + fy;
        const int q = py * v.W + px;
        f3 cp;
        if (render_fragment(s, v.rays[q], v.near_z, v.far_z, cp)) atomicMin(&v.keys[q], zkey(cp.z, gid));
        fx += 4;
        while (fx >= w) { fx -= w; fy++; }
    }
}

// one workgroup per listed tile (kTile consecutive pixels of the surfel's box, row-major), its 256 threads over the tile
__global__ void __launch_bounds__(kB) render_big_kernel(const ViewDev v)
{
    const unsigned n = min(*v.big_count, kBigCap);
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const uint2 ent = v.big[e];   // surfel index | item + (tile << 8)
        const ItemDev& it = v.items[ent.y & 255u];
        const float4* __restrict__ sp = it.surfels + (size_t)ent.x * 3;
        Setup s;
        if (!render_setup(sp[0], sp[2], it.M, v, s)) continue;   // (uniform: the whole workgroup reads the same surfel)
        const unsigned gid = it.base + ent.x;
        const int w = s.x_hi - s.x_lo + 1, area = w * (s.y_hi - s.y_lo + 1);
        const int t0 = (int)(ent.y >> 8) * kTile, t1 = min(area, t0 + kTile);
        for (int t = t0 + (int)threadIdx.x; t < t1; t += kB) {
            const int fy = t / w, fx = t - fy * w;
            const int q = (s.y_lo + fy) * v.W + s.x_lo + fx;
            f3 cp;
            if (render_fragment(s, v.rays[q], v.near_z, v.far_z, cp)) atomicMin(&v.keys[q], zkey(cp.z, gid));
        }
    }
}

__device__ __forceinline__ f3 scale3(f3 a, float k) { return f3{a.x * k, a.y * k, a.z * k}; }

// blue -> green -> red over init_time in [1, tick]
__device__ __forceinline__ f3 times_colour(float init_time, int tick)
{
    float t = 0.0f;
    if (tick > 1) t = (init_time - 1.0f) / ((float)tick - 1.0f);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float t2 = t * 2.0f;
    return t < 0.5f ? f3{0.0f, t2, 1.0f - t2} : f3{t2 - 1.0f, 2.0f - t2, 0.0f};
}

__device__ __forceinline__ f3 base_colour(int mode, const ItemDev& it, const float4 pc, const float4 ct, f3 nw, int flags, int tick)
{
    const float s = fabsf(nw.x + nw.y + nw.z);
    if (!(pc.w > it.thresh)) return scale3(times_colour(ct.z, tick), s + 0.1f);   // drawn below the threshold (CF_RENDER_UNSTABLE)
    switch (mode) {
        case CF_RENDER_GREY: { const float g = 0.5f * s + 0.1f; return f3{g, g, g}; }
        case CF_RENDER_NORMALS: return nw;
        case CF_RENDER_COLOUR: return decode_color(ct.x);
        case CF_RENDER_TIMES: return scale3(times_colour(ct.z, tick), s + 0.1f);
        default: {
            const unsigned char* p = kPaletteBase[it.model_id & 15];   // (ids are 0..254: entry id of the palette)
            return f3{((float)p[0] / 255.0f) * s + 0.1f, ((float)p[1] / 255.0f) * s + 0.1f, ((float)p[2] / 255.0f) * s + 0.1f};
        }
    }
}

__device__ __forceinline__ unsigned char to_u8(float c) { return (unsigned char)glsl_round(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f); }

__global__ void __launch_bounds__(kB) render_resolve_kernel(const ViewDev v, const OutDev o)
{
    const int q = blockIdx.x * kB + threadIdx.x;
    if (q == 0) *v.big_count = 0;   // (the overflow pass of this call is done: the list is empty for the next one)
    if (q >= v.W * v.H) return;
    const unsigned long long key = v.keys[q];
    v.keys[q] = kEmpty;             // leave the z-buffer cleared for the next call (no memset launch)
    if (key == kEmpty) {
        for (int j = 0; j < o.n_rgba; j++) o.rgba[j][q] = make_uchar4(0, 0, 0, 0);
        if (o.depth) o.depth[q] = 0.0f;
        if (o.label) o.label[q] = 255;
        return;
    }
    const unsigned gid = (unsigned)key;
    const ItemDev& it = v.items[find_item_by_index(v, gid)];
    const float4* __restrict__ sp = it.surfels + (size_t)(gid - it.base) * 3;
    const float4 pc = sp[0], ct = sp[1], nr = sp[2];
    Setup s;
    render_setup(pc, nr, it.M, v, s);
    f3 cp;
    render_fragment(s, v.rays[q], v.near_z, v.far_z, cp);
    if (o.depth) o.depth[q] = cp.z;
    if (o.label) o.label[q] = (uint8_t)it.model_id;
    if (!o.n_rgba) return;
    const f3 nw = normalized(f3{it.R[0] * nr.x + it.R[1] * nr.y + it.R[2] * nr.z, it.R[3] * nr.x + it.R[4] * nr.y + it.R[5] * nr.z,
                                it.R[6] * nr.x + it.R[7] * nr.y + it.R[8] * nr.z});
    // Phong terms (view frame, light at the camera centre, normal faced towards it)
    float shade = 1.0f, spec = 0.0f;
    if (v.flags & CF_RENDER_PHONG) {
        f3 nn = s.n;
        if (dot(nn, cp) > 0.0f) nn = f3{-nn.x, -nn.y, -nn.z};
        const f3 L = normalized(f3{-cp.x, -cp.y, -cp.z});
        const float nl = dot(nn, L);
        const float d2 = 2.0f * nl;
        const f3 R = {d2 * nn.x - L.x, d2 * nn.y - L.y, d2 * nn.z - L.z};
        const float rv = fmaxf(dot(R, L), 0.0f);
        const float r2 = rv * rv, r4 = r2 * r2, r8 = r4 * r4, r16 = r8 * r8;
        spec = r16 * r16;
        shade = 0.3f + fmaxf(nl, 0.0f);
    }
    const bool dim = (v.flags & CF_RENDER_WINDOW) && ((float)v.tick - ct.w > (float)v.time_delta);
    for (int j = 0; j < o.n_rgba; j++) {
        f3 c = base_colour(o.mode[j] < 0 ? it.mode : o.mode[j], it, pc, ct, nw, v.flags, v.tick);
        if (v.flags & CF_RENDER_PHONG) c = f3{c.x * shade + spec, c.y * shade + spec, c.z * shade + spec};
        if (dim) c = scale3(c, 0.25f);
        o.rgba[j][q] = make_uchar4(to_u8(c.x), to_u8(c.y), to_u8(c.z), 255);
    }
}

}  // namespace rnd
}  // namespace cf

using namespace cf;
using namespace cf::rnd;

struct cf_renderer {
    cf_ctx* ctx = nullptr;
    int max_w = 0, max_h = 0;
    float4* rays = nullptr;
    unsigned long long* keys = nullptr;
    uint2* big = nullptr;
    unsigned* big_count = nullptr;
    ItemDev* d_items = nullptr;
    ItemDev* h_items[2] = {nullptr, nullptr};  // pinned staging of the item table, alternating between calls
    hipEvent_t staged[2] = {nullptr, nullptr}; // ... each free again once the copy out of it has run
    int slot = 0;
    bool rays_valid = false;                   // the rays hold the intrinsics and size of ray_key
    float ray_key[6] = {0, 0, 0, 0, 0, 0};
};

static int render_fail(cf_ctx* ctx, const char* msg)
{
    ctx->set_error(std::string("cf_render: ") + msg);
    return CF_EINVAL;
}

// camera -> world [R | t] to world -> camera [R^T | -R^T t], in f64 (products of f32 are exact there)
static void view_inverse(const float* C, double* V)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) V[i * 4 + j] = (double)C[j * 4 + i];
        V[i * 4 + 3] = -((double)C[0 * 4 + i] * (double)C[3] + (double)C[1 * 4 + i] * (double)C[7] + (double)C[2 * 4 + i] * (double)C[11]);
    }
    V[12] = 0; V[13] = 0; V[14] = 0; V[15] = 1;
}

extern "C" {

int cf_render_palette(uint8_t* rgb768)
{
    if (!rgb768) return CF_EINVAL;
    for (int i = 0; i < 256; i++)
        for (int c = 0; c < 3; c++) rgb768[i * 3 + c] = i == 255 ? 0 : kPaletteHost[i % 16][c];
    return CF_OK;
}

void cf_render_destroy(cf_renderer* r)
{
    if (!r) return;
    (void)hipStreamSynchronize(r->ctx->stream);
    void* ptrs[] = {r->rays, r->keys, r->big, r->big_count, r->d_items};
    for (void* p : ptrs) (void)hipFree(p);
    for (int k = 0; k < 2; k++) {
        if (r->h_items[k]) (void)hipHostFree(r->h_items[k]);
        if (r->staged[k]) (void)hipEventDestroy(r->staged[k]);
    }
    delete r;
}

int cf_render_create(cf_ctx* ctx, int max_w, int max_h, cf_renderer** out)
{
    if (!ctx || !out || max_w <= 0 || max_h <= 0 || (long long)max_w * max_h > (1ll << 28)) return CF_EINVAL;
    *out = nullptr;
    cf_renderer* r = new cf_renderer();
    r->ctx = ctx; r->max_w = max_w; r->max_h = max_h;
    const size_t N = (size_t)max_w * max_h;
    auto fail = [&](hipError_t e, const char* what) {
        ctx->set_error(std::string("cf_render_create: ") + what + ": " + hipGetErrorString(e));
        cf_render_destroy(r);
        return CF_EHIP;
    };
    hipError_t e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&r->rays), N * sizeof(float4)))) return fail(e, "rays");
    if ((e = hipMalloc(reinterpret_cast<void**>(&r->keys), N * sizeof(unsigned long long)))) return fail(e, "keys");
    if ((e = hipMalloc(reinterpret_cast<void**>(&r->big), kBigCap * sizeof(uint2)))) return fail(e, "overflow list");
    if ((e = hipMalloc(reinterpret_cast<void**>(&r->big_count), sizeof(unsigned)))) return fail(e, "overflow count");
    if ((e = hipMalloc(reinterpret_cast<void**>(&r->d_items), CF_RENDER_MAX_ITEMS * sizeof(ItemDev)))) return fail(e, "items");
    for (int k = 0; k < 2; k++) {
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&r->h_items[k]), CF_RENDER_MAX_ITEMS * sizeof(ItemDev), 0))) return fail(e, "staging");
        if ((e = hipEventCreateWithFlags(&r->staged[k], hipEventDisableTiming))) return fail(e, "event");
    }
    const hipStream_t s = ctx->forked ? ctx->forked_from : ctx->stream;
    if ((e = hipMemsetAsync(r->keys, 0xFF, N * sizeof(unsigned long long), s))) return fail(e, "keys");   // empty; every resolve re-clears
    if ((e = hipMemsetAsync(r->big_count, 0, sizeof(unsigned), s))) return fail(e, "overflow count");
    if ((e = hipStreamSynchronize(s))) return fail(e, "sync");
    *out = r;
    return CF_OK;
}

int cf_render(cf_renderer* r, const cf_render_view* view, const cf_render_item* items, int n_items, const cf_render_output* outputs,
              int n_outputs)
{
    if (!r || !view || (n_items && !items) || (n_outputs && !outputs)) return CF_EINVAL;
    cf_ctx* ctx = r->ctx;
    const int W = view->width, H = view->height;
    if (W <= 0 || H <= 0 || W > r->max_w || H > r->max_h) return render_fail(ctx, "view size outside the render object's maximum");
    if (n_items < 0 || n_items > CF_RENDER_MAX_ITEMS) return render_fail(ctx, "0..256 items");
    if (n_outputs < 0) return render_fail(ctx, "negative output count");
    const float near_z = view->near_z > 0 ? view->near_z : 0.1f, far_z = view->far_z > 0 ? view->far_z : 1000.0f;
    if (!(near_z < far_z)) return render_fail(ctx, "near must lie in front of far");
    if (!(view->fx != 0 && view->fy != 0)) return render_fail(ctx, "zero focal length");
    OutDev o{};
    for (int j = 0; j < n_outputs; j++) {
        const cf_render_output& d = outputs[j];
        if (!d.dst) return render_fail(ctx, "output without a buffer");
        if (d.kind == CF_RENDER_RGBA) {
            if (o.n_rgba == CF_RENDER_MAX_COLOUR) return render_fail(ctx, "more than CF_RENDER_MAX_COLOUR colour outputs");
            if (d.mode < CF_RENDER_ITEM_MODE || d.mode > CF_RENDER_LABEL) return render_fail(ctx, "unknown colour mode");
            o.rgba[o.n_rgba] = static_cast<uchar4*>(d.dst); o.mode[o.n_rgba++] = d.mode;
        } else if (d.kind == CF_RENDER_DEPTH) {
            if (o.depth) return render_fail(ctx, "more than one depth output");
            o.depth = static_cast<float*>(d.dst);
        } else if (d.kind == CF_RENDER_LABELS) {
            if (o.label) return render_fail(ctx, "more than one label output");
            o.label = static_cast<uint8_t*>(d.dst);
        } else return render_fail(ctx, "unknown output kind");
    }
    uint64_t total = 0;
    for (int k = 0; k < n_items; k++) {
        const cf_render_item& it = items[k];
        if (it.count && !it.surfels) return render_fail(ctx, "item without a surfel buffer");
        if (it.model_id < 0 || it.model_id > 254) return render_fail(ctx, "model id outside 0..254");
        if (it.colour_mode < CF_RENDER_GREY || it.colour_mode > CF_RENDER_LABEL) return render_fail(ctx, "unknown colour mode");
        total += it.count;
    }
    if (total > 0xFFFFFFFFull) return render_fail(ctx, "more than 2^32 - 1 surfels in one call (the draw index is 32 bits)");

    // the context's stream, ordered after every lane of the frame (the lane bookkeeping of the frame loop is left as it is)
    const hipStream_t s = ctx->forked ? ctx->forked_from : ctx->stream;
    for (int lane = 0; lane < cf_ctx::kLanes; lane++)
        if (ctx->lanes_used & (1u << lane)) {
            HIPCHK(ctx, hipEventRecord(ctx->lane_done[lane], ctx->lanes[lane]));
            HIPCHK(ctx, hipStreamWaitEvent(s, ctx->lane_done[lane], 0));
        }

    // the item table: model -> camera = view^-1 * Tp in f64, rounded once to f32
    double V[16];
    view_inverse(view->pose, V);
    const int slot = r->slot; r->slot ^= 1;
    HIPCHK(ctx, hipEventSynchronize(r->staged[slot]));   // (the copy out of this staging buffer two calls ago has run)
    ItemDev* h = r->h_items[slot];
    int blocks = 0;
    uint64_t base = 0;
    for (int k = 0; k < n_items; k++) {
        const cf_render_item& it = items[k];
        ItemDev& d = h[k];
        memset(&d, 0, sizeof(d));
        d.surfels = reinterpret_cast<const float4*>(it.surfels);
        d.count = it.count; d.base = (unsigned)base; d.blk_begin = blocks;
        d.thresh = it.conf_threshold; d.model_id = it.model_id; d.mode = it.colour_mode;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++)
                d.M.m[i * 4 + j] = (float)(V[i * 4 + 0] * (double)it.pose[0 * 4 + j] + V[i * 4 + 1] * (double)it.pose[1 * 4 + j] +
                                           V[i * 4 + 2] * (double)it.pose[2 * 4 + j] + V[i * 4 + 3] * (double)it.pose[3 * 4 + j]);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) d.R[i * 3 + j] = it.pose[i * 4 + j];
        blocks += (int)(((uint64_t)it.count * 4 + kB - 1) / kB);
        base += it.count;
    }
    if (n_items) HIPCHK(ctx, hipMemcpyAsync(r->d_items, h, sizeof(ItemDev) * n_items, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipEventRecord(r->staged[slot], s));

    ViewDev v{};
    v.cam = cf_cam{view->fx, view->fy, view->cx, view->cy};
    v.W = W; v.H = H; v.near_z = near_z; v.far_z = far_z;
    v.flags = view->flags; v.tick = view->tick; v.time_delta = view->time_delta;
    v.n_items = n_items; v.items = r->d_items;
    v.rays = r->rays; v.keys = r->keys; v.big = r->big; v.big_count = r->big_count;
    const int px_grid = (int)(((long long)W * H + kB - 1) / kB);
    // the rays depend on the intrinsics and the size only: recomputed when they change
    const float ray_key[6] = {view->fx, view->fy, view->cx, view->cy, (float)W, (float)H};
    if (!r->rays_valid || memcmp(ray_key, r->ray_key, sizeof(ray_key))) {
        render_rays_kernel<<<px_grid, kB, 0, s>>>(v);
        memcpy(r->ray_key, ray_key, sizeof(ray_key));
        r->rays_valid = true;
    }
    if (blocks) {
        render_raster_kernel<<<blocks, kB, 0, s>>>(v);
        render_big_kernel<<<kBigGrid, kB, 0, s>>>(v);
    }
    render_resolve_kernel<<<px_grid, kB, 0, s>>>(v, o);
    HIPCHK(ctx, hipGetLastError());
    return CF_OK;
}

}  // extern "C"
