// ImagePlayer.cpp -- ImagePrefetcher and ImageSequencePlayer (ImagePlayer.h): KlgPrefetch.cpp's worker pattern over the files of an
// image directory, and KlgPlayer.cpp's submit-ahead loop over cf_frame_decoder_submit_images.  A slot index means the same slot on
// both sides: the prefetcher's staging memory IS the decoder's pinned slot.
#include "ImagePlayer.h"

#include <chrono>
#include <cstring>
#include <stdexcept>

#include "CoFusion.h"

namespace cofusion {

std::string decodeJpegRGB(const uint8_t* data, size_t size, int width, int height, uint8_t* rgb);  // Jpeg.cpp
std::string jpegFront(const uint8_t* data, size_t size, int width, int height, cf_jpeg_header* hdr, int16_t* coef, size_t capBlocks, bool* refused);

using namespace imageio;

ImagePrefetcher::ImagePrefetcher(const SequenceLayout& layout, int w, int h, const std::vector<ImageSlotMem>& slots, int workers)
    : lay(layout), width(w), height(h), mem(slots)
{
    if (w <= 0 || h <= 0 || slots.size() < 2) { err = "ImagePrefetcher: a frame size and at least two slots"; return; }
    for (int s = (int)mem.size() - 1; s >= 0; s--) freeSlots.push_back(s);
    workers = workers < 1 ? 1 : (workers > 16 ? 16 : workers);
    for (int t = 0; t < workers; t++) threads.emplace_back([this] { work(); });
}

ImagePrefetcher::~ImagePrefetcher()
{
    {
        std::lock_guard<std::mutex> lk(m);
        stop = true;
    }
    cvWork.notify_all(); cvReady.notify_all();
    for (auto& t : threads) t.join();
}

int ImagePrefetcher::limit() const
{
    int n = lay.numFrames;
    if (frameLimit >= 0 && frameLimit < n) n = frameLimit;
    return n < 0 ? 0 : n;
}

void ImagePrefetcher::setLimits(int maxFrames)
{
    {
        std::lock_guard<std::mutex> lk(m);
        frameLimit = maxFrames;
    }
    cvWork.notify_all();
}

bool ImagePrefetcher::hasMore() const { return !threads.empty() && nextDeliver < limit(); }

DecodeTimes ImagePrefetcher::times()
{
    std::lock_guard<std::mutex> lk(m);
    return sum;
}

// One frame into a slot, as ImageSequenceReader::next decodes it (same parsers, same checks, same error texts) up to the boundary
// where the device takes over: unfiltered scanlines, inflated EXR blocks, JPEG coefficients.
std::string ImagePrefetcher::decode(int i, const ImageSlotMem& s, std::vector<uint8_t>& file, cf_image_desc* d, DecodeTimes* t)
{
    const size_t N = (size_t)width * height;
    const std::string size = std::to_string(width) + " x " + std::to_string(height);
    memset(d, 0, sizeof(*d));
    d->width = width; d->height = height;
    d->flip_colors = lay.opt.flipColors ? 1 : 0;
    d->depth_scale = lay.opt.depthScale;
    auto load = [&](const std::string& p) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string e = readFile(p, &file);
        t->read += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return e;
    };
    std::string e, p = lay.path(ROLE_COLOR, i);
    if (!(e = load(p)).empty()) return p + ": " + e;
    if (lay.colorExt == ".png") {
        PngInfo pi;
        if (!(e = pngDecode(file.data(), file.size(), ROLE_COLOR, &pi, s.image.color, (size_t)s.image.color_bytes, s.image.palette, t)).empty()) return p + ": " + e;
        if (pi.width != width || pi.height != height) return p + ": the frame is not " + size;
        d->color_kind = CF_IMAGE_PNG; d->png_color_type = pi.colorType; d->png_palette_entries = pi.paletteEntries;
    } else if (lay.colorExt == ".ppm") {
        int pw, ph;
        const uint8_t* px;
        if (!(e = ppmDecode(file.data(), file.size(), &pw, &ph, &px)).empty()) return p + ": " + e;
        if (pw != width || ph != height) return p + ": the frame is not " + size;
        memcpy(s.frame.rgb, px, N * 3);
        d->color_kind = CF_IMAGE_RAW;
    } else {
        bool refused = false;
        e = jpegFront(file.data(), file.size(), width, height, s.frame.header, s.frame.coef, (size_t)s.frame.coef_blocks, &refused);
        d->color_kind = CF_IMAGE_JPEG;
        if (e.empty() && refused) {   // not a stream the device path reproduces: the whole host decoder, handed on as raw colour
            e = decodeJpegRGB(file.data(), file.size(), width, height, s.frame.rgb);
            d->color_kind = CF_IMAGE_RAW;
        }
        if (!e.empty()) return p + ": " + e;
    }
    p = lay.path(ROLE_DEPTH, i);
    if (!(e = load(p)).empty()) return p + ": " + e;
    if (lay.depthExt == ".png") {
        PngInfo pi;
        if (!(e = pngDecode(file.data(), file.size(), ROLE_DEPTH, &pi, s.image.depth, (size_t)s.image.depth_bytes, nullptr, t)).empty()) return p + ": " + e;
        if (pi.width != width || pi.height != height) return p + ": the frame is not " + size;
        d->depth_kind = CF_IMAGE_PNG;
    } else {
        ExrInfo ei;
        if (!(e = exrDecode(file.data(), file.size(), &ei, s.image.depth, (size_t)s.image.depth_bytes, s.image.blocks, s.image.max_blocks, t)).empty()) return p + ": " + e;
        if (ei.width != width || ei.height != height) return p + ": the frame is not " + size;
        d->depth_kind = CF_IMAGE_EXR;
        d->exr_blocks = ei.blocks; d->exr_lines_per_block = ei.linesPerBlock; d->exr_line_bytes = ei.lineBytes;
        d->exr_chan_offset = ei.chanOffset; d->exr_chan_half = ei.chanHalf;
    }
    if (lay.hasMasks && i < lay.maxMasks) {
        p = lay.path(ROLE_MASK, i);
        if (!(e = load(p)).empty()) return p + ": " + e;
        if (lay.maskExt == ".png") {
            PngInfo pi;
            if (!(e = pngDecode(file.data(), file.size(), ROLE_MASK, &pi, s.image.mask, (size_t)s.image.mask_bytes, nullptr, t)).empty()) return p + ": " + e;
            if (pi.width != width || pi.height != height) return p + ": the mask is not " + size;
            d->mask_kind = CF_IMAGE_PNG;
        } else {
            int pw, ph;
            const uint8_t* px;
            if (!(e = pgmDecode(file.data(), file.size(), &pw, &ph, &px)).empty()) return p + ": " + e;
            if (pw != width || ph != height) return p + ": the mask is not " + size;
            memcpy(s.image.mask, px, N);
            d->mask_kind = CF_IMAGE_RAW;
        }
    }
    return "";
}

void ImagePrefetcher::work()
{
    std::vector<uint8_t> file;
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
        // a frame number and a slot are taken together, in order: the frame whose turn it is always owns a slot
        cvWork.wait(lk, [&] { return stop || (!freeSlots.empty() && nextClaim < limit()); });
        if (stop) return;
        const int i = nextClaim++;
        const unsigned gen = generation;
        Result r;
        r.slot = freeSlots.back(); freeSlots.pop_back();
        busy++;
        lk.unlock();
        DecodeTimes t;
        r.err = decode(i, mem[(size_t)r.slot], file, &r.desc, &t);
        lk.lock();
        busy--;
        sum.read += t.read; sum.inflate += t.inflate; sum.unfilter += t.unfilter; sum.parse += t.parse;
        if (gen != generation || stop) {   // rewound meanwhile: rewind() takes the slot back itself
            cvReady.notify_all();
            continue;
        }
        ready[i] = r;
        cvReady.notify_all();
    }
}

int ImagePrefetcher::deliver(ImageFrame* out, std::unique_lock<std::mutex>& lk, bool block)
{
    if (threads.empty()) return -1;
    if (nextDeliver >= limit()) { err = "no more frames"; return block ? -1 : 1; }
    auto it = ready.find(nextDeliver);
    if (it == ready.end()) {
        if (!block) return 1;
        cvReady.wait(lk, [&] { return stop || (it = ready.find(nextDeliver)) != ready.end(); });
        if (it == ready.end()) return -1;
    }
    const Result r = it->second;
    ready.erase(it);
    if (!r.err.empty()) {
        err = "frame " + std::to_string(nextDeliver) + ": " + r.err;
        freeSlots.push_back(r.slot);
        nextDeliver = 0x7ffffff0;   // nothing is played behind a frame that failed, as the serial reader stays at it
        nextClaim = 0x7fffffff;
        return -1;
    }
    out->index = nextDeliver; out->slot = r.slot; out->desc = r.desc; out->timestamp = lay.timestamp(nextDeliver);
    nextDeliver++;
    return 0;
}

bool ImagePrefetcher::next(ImageFrame* out)
{
    std::unique_lock<std::mutex> lk(m);
    return deliver(out, lk, true) == 0;
}

int ImagePrefetcher::tryNext(ImageFrame* out)
{
    std::unique_lock<std::mutex> lk(m);
    return deliver(out, lk, false);
}

void ImagePrefetcher::release(int slot)
{
    if (slot < 0 || slot >= (int)mem.size()) return;
    {
        std::lock_guard<std::mutex> lk(m);
        for (int s : freeSlots) if (s == slot) return;
        freeSlots.push_back(slot);
    }
    cvWork.notify_all();
}

void ImagePrefetcher::rewind()
{
    std::unique_lock<std::mutex> lk(m);
    generation++;
    nextClaim = 0x7fffffff;                         // nobody starts a frame while the ones in flight drain
    cvReady.wait(lk, [&] { return busy == 0; });
    ready.clear();
    freeSlots.clear();
    for (int s = (int)mem.size() - 1; s >= 0; s--) freeSlots.push_back(s);
    nextClaim = 0; nextDeliver = 0;
    lk.unlock();
    cvWork.notify_all();
}

// ---- the player ----
static void chk(cf_ctx* ctx, int rc, const char* what)
{
    if (rc != CF_OK) throw std::runtime_error(std::string(what) + ": " + cf_last_error(ctx));
}

ImageSequencePlayer::ImageSequencePlayer(CoFusion& c, const SequenceOptions& opt, int workers, int nslots)
    : cf(c), ctx(c.context()), width(c.cfg.width), height(c.cfg.height)
{
    if (cf.cfg.world > 1) throw std::runtime_error("ImageSequencePlayer: not available for a model-parallel instance (world > 1)");
    {
        ImageSequenceReader probe(opt);   // the directory rules, and the frame size from the first colour file
        if (!probe.ok()) throw std::runtime_error(probe.error());
        if (probe.width() != width || probe.height() != height)
            throw std::runtime_error("ImageSequencePlayer: the set's frames are " + std::to_string(probe.width()) + " x " + std::to_string(probe.height()) +
                                     ", the instance's " + std::to_string(width) + " x " + std::to_string(height));
        lay = probe.layout();
    }
    workers = workers < 1 ? 1 : (workers > 16 ? 16 : workers);
    slots = nslots > 0 ? nslots : workers + 3;
    slots = slots < 4 ? 4 : (slots > 16 ? 16 : slots);
    chk(ctx, cf_frame_decoder_create(ctx, width, height, slots, &dec), "cf_frame_decoder_create");
    const int rc = cf_frame_decoder_enable_images(dec);
    if (rc != CF_OK) {
        const std::string e = cf_last_error(ctx);
        cf_frame_decoder_destroy(dec); dec = nullptr;
        throw std::runtime_error("cf_frame_decoder_enable_images: " + e);
    }
    std::vector<ImageSlotMem> mem((size_t)slots);
    for (int s = 0; s < slots; s++) {
        cf_frame_decoder_slot(dec, s, &mem[(size_t)s].frame);
        cf_frame_decoder_image_slot(dec, s, &mem[(size_t)s].image);
    }
    prefetch = new ImagePrefetcher(lay, width, height, mem, workers);
}

ImageSequencePlayer::~ImageSequencePlayer()
{
    delete prefetch;                 // the workers write into the decoder's pinned slots: they go first
    cf_frame_decoder_destroy(dec);   // (waits for the decoder's stream)
}

// The frame handed out last goes back to the workers.  Its staging memory was read by copies on the decoder's stream: the host waits
// for the slot's event first.
void ImageSequencePlayer::releaseCurrent()
{
    if (current < 0) return;
    chk(ctx, cf_frame_decoder_acquire(dec, current, 1, nullptr, nullptr), "cf_frame_decoder_acquire");
    prefetch->release(current);
    current = -1;
}

bool ImageSequencePlayer::next(int64_t* timestamp, const float** depth_dev, const uint8_t** rgba_dev, const uint8_t** mask_dev)
{
    releaseCurrent();
    // submit ahead: wait only for the frame that is needed now, take the others as far as they are ready
    while ((int)submitted.size() < slots - 2 && pendingError.empty()) {
        ImageFrame f;
        int rc;
        if (submitted.empty()) {
            if (!prefetch->hasMore()) break;
            rc = prefetch->next(&f) ? 0 : -1;
        } else {
            rc = prefetch->tryNext(&f);
        }
        if (rc > 0) break;
        if (rc < 0) { pendingError = prefetch->error(); break; }
        chk(ctx, cf_frame_decoder_submit_images(dec, f.slot, &f.desc), "cf_frame_decoder_submit_images");
        submitted.push_back(f);
    }
    if (submitted.empty()) {
        if (!pendingError.empty()) { const std::string e = pendingError; pendingError.clear(); throw std::runtime_error(e); }
        return false;
    }
    const ImageFrame f = submitted.front();
    submitted.pop_front();
    const int complete = cf.cfg.deviceFramesComplete ? 1 : 0;
    chk(ctx, cf_frame_decoder_acquire(dec, f.slot, complete, depth_dev, rgba_dev), "cf_frame_decoder_acquire");
    const uint8_t* mask = nullptr;
    chk(ctx, cf_frame_decoder_acquire_mask(dec, f.slot, complete, &mask), "cf_frame_decoder_acquire_mask");
    if (mask_dev) *mask_dev = mask;
    current = f.slot;
    if (timestamp) *timestamp = f.timestamp;
    return true;
}

bool ImageSequencePlayer::process()
{
    FrameData f;
    if (!next(&f.timestamp, &f.depth_dev, &f.rgba_dev, &f.mask_dev)) return false;
    cf.processFrame(f, nullptr);
    return true;
}

void ImageSequencePlayer::rewind()
{
    // every slot goes back to the workers: first let the copies out of the slots that were submitted finish
    releaseCurrent();
    for (const ImageFrame& f : submitted) chk(ctx, cf_frame_decoder_acquire(dec, f.slot, 1, nullptr, nullptr), "cf_frame_decoder_acquire");
    submitted.clear();
    pendingError.clear();
    prefetch->rewind();
}

}  // namespace cofusion
