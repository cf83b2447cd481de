// cabi.hip -- C-ABI (include/cofusion_hip.h) over the gfx950 kernels: the context.  Streams, lanes, marks, memory helpers, settings, the
// profile read-out.  The single-function entries are in cabi_steps.hip, the tracker object in cabi_odom.hip, the per-frame tracking call in
// cabi_track.hip, the surfel models in cabi_model.hip.  No allocation happens on the per-frame path: every device buffer is created
// with the ctx / odom / model object that owns it.
#include <stdlib.h>
#include <string.h>

#include <string>

#include "cf_host.h"

using namespace cf;

void cf_ctx::set_error(const std::string& m)
{
    std::lock_guard<std::mutex> lk(error_mutex);
    last_error = m;
}

// the stream and the done-event of an auxiliary lane, created at its first use
static int lane_ready(cf_ctx* ctx, int lane)
{
    if (!ctx->lanes[lane]) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->lanes[lane], hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->lane_done[lane], hipEventDisableTiming));
    }
    return CF_OK;
}
// back on the stream the lanes were forked from; their work keeps running
static void leave_lane(cf_ctx* ctx)
{
    if (ctx->forked) { ctx->stream = ctx->forked_from; ctx->forked = false; }
}
// the main stream waits for what `lane` holds
static int join_lane(cf_ctx* ctx, int lane)
{
    HIPCHK(ctx, hipEventRecord(ctx->lane_done[lane], ctx->lanes[lane]));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->lane_done[lane], 0));
    return CF_OK;
}

extern "C" {

int cf_create(const cf_config* cfg, cf_ctx** out)
{
    if (!cfg || !out || cfg->width <= 0 || cfg->height <= 0 || (cfg->width % 16) || (cfg->height % 4)) return CF_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CF_EHIP;  // fail loudly: no CPU fallback
    cf_ctx* ctx = new cf_ctx();
    ctx->cfg = *cfg;
    if (ctx->cfg.max_models <= 0) ctx->cfg.max_models = 1;
    *out = ctx;
    HIPCHK(ctx, hipSetDevice(cfg->device));
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    ctx->icp_launch = IcpLaunch{256, 0, 0};   // (0 pixels per lane: launch_icp_rgbres chooses by level)
    if (int r = dmalloc(ctx, &ctx->d_acc_a, (size_t)kGroups * 32)) return r;
    if (int r = dmalloc(ctx, &ctx->d_acc_b, (size_t)kGroups * 32)) return r;
    if (int r = dmalloc(ctx, &ctx->d_out, 64)) return r;
    if (int r = dmalloc(ctx, &ctx->d_scratch_state, 1)) return r;
    if (int r = dmalloc(ctx, &ctx->d_state_pool, (size_t)cf_ctx::kStateSlots)) return r;
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_state_pool), sizeof(OdomDev) * cf_ctx::kStateSlots, hipHostMallocCoherent));  // the last solve stores into it
    memset(ctx->h_state_pool, 0, sizeof(OdomDev) * cf_ctx::kStateSlots);
    if (int r = dmalloc(ctx, &ctx->d_so3_sync, (size_t)ctx->cfg.max_models + 1)) return r;
    // the ONE environment switch of the library: CF_ICP_ARITH = "product" (default) / "gram" / "reference", the rounding specification of the tracker's sums
    // for every context of the process (cf_set_icp_arith sets it per context; launch shape and data path have setters only)
    if (const char* e = getenv("CF_ICP_ARITH")) {
        if (cf_set_icp_arith(ctx, (!strcmp(e, "gram") || !strcmp(e, "1")) ? CF_ICP_ARITH_GRAM : (!strcmp(e, "reference") || !strcmp(e, "2")) ? CF_ICP_ARITH_REFERENCE
                                  : (!strcmp(e, "product") || !strcmp(e, "0")) ? CF_ICP_ARITH_PRODUCT : -1) != CF_OK) {
            ctx->set_error("CF_ICP_ARITH: product | gram | reference"); return CF_EINVAL;
        }
    }
    if (int r = dmalloc(ctx, &ctx->d_cand_scratch, (size_t)cfg->width * cfg->height)) return r;
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_scratch_state), sizeof(OdomDev)));
    HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_out), sizeof(unsigned long long) * 64));
    ctx->prof.capacity = 8192;
    ctx->prof.events = new hipEvent_t[ctx->prof.capacity];
    for (int i = 0; i < ctx->prof.capacity; i++) HIPCHK(ctx, hipEventCreate(&ctx->prof.events[i]));
    ctx->prof.used = 0; ctx->prof.enabled = 0; ctx->prof.bytes = 0; ctx->prof.launches = 0;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}

void cf_destroy(cf_ctx* ctx)
{
    if (ctx && ctx->batch_event) (void)hipEventDestroy(ctx->batch_event);
    if (ctx) for (int i = 0; i < cf_ctx::kSurfEvents; i++) if (ctx->surf_events[i]) (void)hipEventDestroy(ctx->surf_events[i]);
    if (!ctx) return;
    (void)hipStreamSynchronize(ctx->stream);
    (void)cf_rccl_destroy(ctx);
    (void)hipFree(ctx->d_acc_a); (void)hipFree(ctx->d_acc_b); (void)hipFree(ctx->d_out);
    (void)hipFree(ctx->d_scratch_state); (void)hipFree(ctx->d_so3_sync); (void)hipFree(ctx->d_cand_scratch);
    (void)hipFree(ctx->d_state_pool); (void)hipHostFree(ctx->h_state_pool);
    (void)hipHostFree(ctx->h_scratch_state); (void)hipHostFree(ctx->h_out);
    if (ctx->d_ref) (void)hipFree(ctx->d_ref);
    if (ctx->h_ref) (void)hipHostFree(ctx->h_ref);
    if (ctx->d_redetect_bits) (void)hipFree(ctx->d_redetect_bits);
    if (ctx->d_redetect_counts) (void)hipFree(ctx->d_redetect_counts);
    if (ctx->h_redetect_counts) (void)hipHostFree(ctx->h_redetect_counts);
    if (ctx->d_search) (void)hipFree(ctx->d_search);
    if (ctx->h_search) (void)hipHostFree(ctx->h_search);
    for (hipEvent_t e : ctx->redetect_ev) if (e) (void)hipEventDestroy(e);
    if (ctx->prof.events) {
        for (int i = 0; i < ctx->prof.capacity; i++) (void)hipEventDestroy(ctx->prof.events[i]);
        delete[] ctx->prof.events;
    }
    for (int i = 0; i < cf_ctx::kLanes; i++) {
        if (ctx->lanes[i]) (void)hipStreamDestroy(ctx->lanes[i]);
        if (ctx->lane_done[i]) (void)hipEventDestroy(ctx->lane_done[i]);
    }
    if (ctx->fork_point) (void)hipEventDestroy(ctx->fork_point);
    for (int i = 0; i < cf_ctx::kMarks; i++) if (ctx->marks[i]) (void)hipEventDestroy(ctx->marks[i]);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char* cf_last_error(const cf_ctx* ctx)
{
    if (!ctx) return "null ctx";
    // helper threads bound with cf_thread_lane may fail (and rewrite last_error) at the same time: hand out a per-thread copy taken
    // under the lock, valid until the calling thread's next cf_last_error
    static thread_local std::string copy;
    {
        std::lock_guard<std::mutex> lk(const_cast<cf_ctx*>(ctx)->error_mutex);
        copy = ctx->last_error;
    }
    return copy.c_str();
}
// Switching streams drains the old one first: allocations zero-fill asynchronously on the stream that was current when they
// were made, and nothing else would order that before the first use on the new stream.
int cf_set_stream(cf_ctx* ctx, void* s)  // NULL = the legacy default stream
{
    if (!ctx || ctx->forked) return CF_EINVAL;
    if (ctx->stream != (hipStream_t)s) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = (hipStream_t)s;
    return CF_OK;
}
int cf_use_own_stream(cf_ctx* ctx)
{
    if (!ctx || ctx->forked) return CF_EINVAL;
    if (ctx->stream != ctx->own_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = ctx->own_stream;
    return CF_OK;
}

// Independent pieces of one frame (the surfel passes of different models) may overlap on the GPU: cf_fork(lane) routes
// the following calls to auxiliary stream `lane`, ordered after everything enqueued on the context's stream at the first
// fork; cf_join returns to that stream and orders it after all lanes used since.
extern "C++" { thread_local cf_thread_binding cf_tls_binding; }

int cf_fork(cf_ctx* ctx, int lane)
{
    if (!ctx || lane < 0) return CF_EINVAL;
    lane %= cf_ctx::kLanes;
    if (int r = lane_ready(ctx, lane)) return r;
    if (!ctx->fork_point) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->fork_point, hipEventDisableTiming));
    if (!ctx->forked) {  // leaving the main stream: everything enqueued on it so far precedes the lane's work
        ctx->forked_from = ctx->stream;
        HIPCHK(ctx, hipEventRecord(ctx->fork_point, ctx->forked_from));
        ctx->forked = true;
    }
    HIPCHK(ctx, hipStreamWaitEvent(ctx->lanes[lane], ctx->fork_point, 0));
    ctx->lanes_used |= 1u << lane;
    ctx->stream = ctx->lanes[lane];
    return CF_OK;
}
// cf_mark(slot) remembers the current point of the stream; cf_fork_after(lane, slot) routes the following calls to `lane`
// ordered after that point ONLY (slot < 0: after nothing) -- for work that does not depend on what the main stream still has
// queued, e.g. filtering the next frame while the previous frame's fusion passes run.  cf_join orders the main stream after it.
int cf_mark(cf_ctx* ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= cf_ctx::kMarks) return CF_EINVAL;
    if (!ctx->marks[slot]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->marks[slot], hipEventDisableTiming));
    HIPCHK(ctx, hipEventRecord(ctx->marks[slot], ctx->stream));
    ctx->mark_set[slot] = true;
    return CF_OK;
}
// host wait for a mark (e.g. before re-using a pinned staging buffer whose transfer was enqueued before the mark)
int cf_event_wait_host(cf_ctx* ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= cf_ctx::kMarks) return CF_EINVAL;
    if (ctx->mark_set[slot]) HIPCHK(ctx, hipEventSynchronize(ctx->marks[slot]));
    return CF_OK;
}
int cf_fork_after(cf_ctx* ctx, int lane, int slot)
{
    if (!ctx || lane < 0 || slot >= cf_ctx::kMarks || ctx->forked) return CF_EINVAL;
    lane %= cf_ctx::kLanes;
    if (int r = lane_ready(ctx, lane)) return r;
    if (slot >= 0 && ctx->mark_set[slot]) HIPCHK(ctx, hipStreamWaitEvent(ctx->lanes[lane], ctx->marks[slot], 0));
    ctx->forked_from = ctx->stream;
    ctx->forked = true;
    ctx->lanes_used |= 1u << lane;
    ctx->stream = ctx->lanes[lane];
    return CF_OK;
}
// back to the main stream WITHOUT waiting for the lanes (their work keeps running beside what follows); cf_join waits
int cf_main(cf_ctx* ctx)
{
    if (!ctx) return CF_EINVAL;
    leave_lane(ctx);
    return CF_OK;
}
int cf_join(cf_ctx* ctx)
{
    if (!ctx) return CF_EINVAL;
    leave_lane(ctx);
    for (int lane = 0; lane < cf_ctx::kLanes; lane++)
        if (ctx->lanes_used & (1u << lane))
            if (int r = join_lane(ctx, lane)) return r;
    ctx->lanes_used = 0;
    return CF_OK;
}
// ... for one lane only: the main stream waits for what that lane holds, the other lanes keep running beside it
int cf_join_lane(cf_ctx* ctx, int lane)
{
    if (!ctx || lane < 0) return CF_EINVAL;
    lane %= cf_ctx::kLanes;
    leave_lane(ctx);
    if (ctx->lanes_used & (1u << lane)) {
        if (int r = join_lane(ctx, lane)) return r;
        ctx->lanes_used &= ~(1u << lane);
    }
    return CF_OK;
}
// Bind the calling thread to lane `lane` of the context (lane < 0: unbind).  The owning thread forks the lane first (cf_fork, then
// cf_main), which orders the lane after the stream and books it for the next cf_join; the bound thread's model calls then go to
// the lane without touching the context's current stream.
int cf_thread_lane(cf_ctx* ctx, int lane)
{
    if (!ctx) return CF_EINVAL;
    if (lane < 0) { cf_tls_binding = cf_thread_binding{}; return CF_OK; }
    lane %= cf_ctx::kLanes;
    if (!ctx->lanes[lane] || !(ctx->lanes_used & (1u << lane))) { ctx->set_error("cf_thread_lane: lane was not forked"); return CF_ESTATE; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    cf_tls_binding.ctx = ctx;
    cf_tls_binding.stream = ctx->lanes[lane];
    return CF_OK;
}
void* cf_get_stream(cf_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
int cf_synchronize(cf_ctx* ctx) { if (!ctx) return CF_EINVAL; HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return CF_OK; }
int cf_malloc(cf_ctx* ctx, uint64_t bytes, void** dptr)
{
    if (!ctx || !dptr) return CF_EINVAL;
    HIPCHK(ctx, hipMalloc(dptr, bytes));
    HIPCHK(ctx, hipMemsetAsync(*dptr, 0, bytes, ctx->stream));
    return CF_OK;
}
int cf_free(cf_ctx* ctx, void* dptr) { if (!ctx) return CF_EINVAL; HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(dptr)); return CF_OK; }
int cf_memcpy_h2d(cf_ctx* ctx, void* dst, const void* src, uint64_t bytes)
{
    if (!ctx) return CF_EINVAL;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}
int cf_memcpy_d2h(cf_ctx* ctx, void* dst, const void* src, uint64_t bytes)
{
    if (!ctx) return CF_EINVAL;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}

// pinned host staging + asynchronous upload: the host-input path of the facade copies a frame into pinned memory and
// enqueues the transfer without waiting for it
int cf_malloc_host(cf_ctx* ctx, uint64_t bytes, void** hptr)
{
    if (!ctx || !hptr) return CF_EINVAL;
    HIPCHK(ctx, hipHostMalloc(hptr, bytes));
    return CF_OK;
}
int cf_free_host(cf_ctx* ctx, void* hptr) { if (!ctx) return CF_EINVAL; HIPCHK(ctx, hipHostFree(hptr)); return CF_OK; }
int cf_memcpy_h2d_async(cf_ctx* ctx, void* dst, const void* src_pinned, uint64_t bytes)
{
    if (!ctx) return CF_EINVAL;
    HIPCHK(ctx, hipMemcpyAsync(dst, src_pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
    return CF_OK;
}
int cf_memcpy_d2h_async(cf_ctx* ctx, void* dst_pinned, const void* src, uint64_t bytes)
{
    if (!ctx) return CF_EINVAL;
    HIPCHK(ctx, hipMemcpyAsync(dst_pinned, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return CF_OK;
}
int cf_memcpy_d2d_async(cf_ctx* ctx, void* dst, const void* src, uint64_t bytes)
{
    if (!ctx) return CF_EINVAL;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return CF_OK;
}
int cf_rgb_to_rgba(cf_ctx* ctx, const uint8_t* rgb_dev, int cols, int rows, uint8_t* rgba_dev)
{
    if (!ctx || !rgb_dev || !rgba_dev || cols <= 0 || rows <= 0) return CF_EINVAL;
    launch_rgb_expand(ctx->stream, rgb_dev, cols * rows, rgba_dev);
    LAUNCHCHK(ctx);
    return CF_OK;
}

int cf_set_icp_launch(cf_ctx* ctx, int threads, int ppt)
{
    if (!ctx || (threads != 64 && threads != 128 && threads != 256 && threads != 512 && threads != 1024) ||
        (ppt != 0 && ppt != 1 && ppt != 2 && ppt != 4))
        return CF_EINVAL;
    ctx->icp_launch = IcpLaunch{threads, ppt, ctx->icp_launch.gram};
    return CF_OK;
}

int cf_set_icp_arith(cf_ctx* ctx, int mode)
{
    if (!ctx || (mode != CF_ICP_ARITH_PRODUCT && mode != CF_ICP_ARITH_GRAM && mode != CF_ICP_ARITH_REFERENCE)) return CF_EINVAL;
    ctx->icp_arith = mode;
    ctx->icp_launch.gram = mode == CF_ICP_ARITH_GRAM ? 1 : 0;
    return CF_OK;
}
int cf_get_icp_arith(cf_ctx* ctx) { return ctx ? ctx->icp_arith : CF_EINVAL; }

int cf_profile_enable(cf_ctx* ctx, int on) { if (!ctx || on < 0) return CF_EINVAL; ctx->prof.enabled = on; ctx->prof_calls = 0; return CF_OK; }
int cf_profile_read(cf_ctx* ctx, cf_profile* out, int reset)
{
    if (!ctx || !out) return CF_EINVAL;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    double ms = ctx->prof_ms_accum;
    for (int i = 0; i + 1 < ctx->prof.used; i += 2) {
        float t = 0;
        HIPCHK(ctx, hipEventElapsedTime(&t, ctx->prof.events[i], ctx->prof.events[i + 1]));
        ms += t;
    }
    ctx->prof_ms_accum = ms;
    ctx->prof.used = 0;
    out->icp_ms_total = ms; out->icp_launches = ctx->prof.launches; out->icp_bytes = ctx->prof.bytes;
    for (int i = 0; i + 1 < ctx->surf_used; i += 2) {
        float t = 0;
        HIPCHK(ctx, hipEventElapsedTime(&t, ctx->surf_events[i], ctx->surf_events[i + 1]));
        ctx->surf_ms_accum += t;
    }
    ctx->surf_used = 0;
    out->surfel_ms_total = ctx->surf_ms_accum; out->surfel_calls = ctx->surf_calls; out->surfel_bytes = ctx->surf_bytes;
    if (reset) { ctx->prof_ms_accum = 0; ctx->prof.launches = 0; ctx->prof.bytes = 0; ctx->surf_ms_accum = 0; ctx->surf_calls = 0; ctx->surf_bytes = 0; }
    return CF_OK;
}

}  // extern "C"
