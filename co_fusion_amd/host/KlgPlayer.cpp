// KlgPlayer.cpp -- KlgPlayer (KlgPlayer.h): the prefetcher over the pinned slots of a cf_frame_decoder, in front of
// CoFusion::processFrame's device entry.  A slot index means the same slot on both sides: the prefetcher's staging memory IS the
// decoder's pinned slot, and the decoder's output frame of that slot is what processFrame reads.
#include "KlgPlayer.h"

#include <stdexcept>

#include "CoFusion.h"

namespace cofusion {

static void chk(cf_ctx* ctx, int rc, const char* what)
{
    if (rc != CF_OK) throw std::runtime_error(std::string(what) + ": " + cf_last_error(ctx));
}

KlgPlayer::KlgPlayer(CoFusion& c, const std::string& file, bool flipColors, int workers, int nslots)
    : cf(c), ctx(c.context()), width(c.cfg.width), height(c.cfg.height), flip(flipColors)
{
    if (cf.cfg.world > 1) throw std::runtime_error("KlgPlayer: not available for a model-parallel instance (world > 1)");
    workers = workers < 1 ? 1 : (workers > 16 ? 16 : workers);
    slots = nslots > 0 ? nslots : workers + 3;
    slots = slots < 4 ? 4 : (slots > 16 ? 16 : slots);
    chk(ctx, cf_frame_decoder_create(ctx, width, height, slots, &dec), "cf_frame_decoder_create");
    std::vector<cf_frame_slot> mem((size_t)slots);
    for (int s = 0; s < slots; s++) cf_frame_decoder_slot(dec, s, &mem[(size_t)s]);
    prefetch = new KlgPrefetcher(file, width, height, mem, workers);
    if (!prefetch->ok()) {
        const std::string e = prefetch->error();
        delete prefetch; prefetch = nullptr;
        cf_frame_decoder_destroy(dec); dec = nullptr;
        throw std::runtime_error(e);
    }
}

KlgPlayer::~KlgPlayer()
{
    delete prefetch;                 // the workers write into the decoder's pinned slots: they go first
    cf_frame_decoder_destroy(dec);   // (waits for the decoder's stream)
}

void KlgPlayer::setLimits(bool referenceCompatible, int frameLimit) { prefetch->setLimits(referenceCompatible, frameLimit); }

// The frame handed out last goes back to the workers.  Its staging memory was read by copies on the decoder's stream: the host waits
// for the slot's event first (long passed when the frame has been processed; with deviceFramesComplete = 0 nobody has waited yet).
void KlgPlayer::releaseCurrent()
{
    if (current < 0) return;
    chk(ctx, cf_frame_decoder_acquire(dec, current, 1, nullptr, nullptr), "cf_frame_decoder_acquire");
    prefetch->release(current);
    current = -1;
}

bool KlgPlayer::next(int64_t* timestamp, const float** depth_dev, const uint8_t** rgba_dev)
{
    releaseCurrent();
    // submit ahead: wait only for the frame that is needed now, take the others as far as they are ready
    while ((int)submitted.size() < slots - 2 && pendingError.empty()) {
        KlgFrame f;
        int rc;
        if (submitted.empty()) {
            if (!prefetch->hasMore()) break;
            rc = prefetch->next(&f) ? 0 : -1;
        } else {
            rc = prefetch->tryNext(&f);
        }
        if (rc > 0) break;
        if (rc < 0) { pendingError = prefetch->error(); break; }
        cf_frame_desc d;
        d.width = width; d.height = height; d.color_kind = f.colorKind; d.flip_colors = flip ? 1 : 0;
        chk(ctx, cf_frame_decoder_submit(dec, f.slot, &d), "cf_frame_decoder_submit");
        submitted.push_back(f);
    }
    if (submitted.empty()) {
        if (!pendingError.empty()) { const std::string e = pendingError; pendingError.clear(); throw std::runtime_error(e); }
        return false;
    }
    const KlgFrame f = submitted.front();
    submitted.pop_front();
    chk(ctx, cf_frame_decoder_acquire(dec, f.slot, cf.cfg.deviceFramesComplete ? 1 : 0, depth_dev, rgba_dev), "cf_frame_decoder_acquire");
    current = f.slot;
    if (timestamp) *timestamp = f.timestamp;
    return true;
}

bool KlgPlayer::process()
{
    FrameData f;
    if (!next(&f.timestamp, &f.depth_dev, &f.rgba_dev)) return false;
    cf.processFrame(f, nullptr);
    return true;
}

void KlgPlayer::rewind()
{
    // every slot goes back to the workers: first let the copies out of the slots that were submitted finish
    releaseCurrent();
    for (const KlgFrame& f : submitted) chk(ctx, cf_frame_decoder_acquire(dec, f.slot, 1, nullptr, nullptr), "cf_frame_decoder_acquire");
    submitted.clear();
    pendingError.clear();
    prefetch->rewind();
}

}  // namespace cofusion
