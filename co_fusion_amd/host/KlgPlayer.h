// KlgPlayer.h -- plays a .klg log at tracker speed.  KlgLogReader::getNext inflates and JPEG-decodes every
// frame on the calling thread, serially with the GPU work.  The frames of a log do not depend on each other, so here
//   KlgPrefetcher  reads ahead on worker threads: pread, inflate the depth, run the JPEG front end (host/Jpeg.cpp: jpegFront) into
//                  slot memory the owner hands in; frames are delivered strictly in log order.  No GPU calls.
//   KlgPlayer      a prefetcher over the pinned slots of a cf_frame_decoder (csrc/frame_decode.hip), which finishes the frames on
//                  the device, feeding CoFusion::processFrame through its device entry.
// Both produce exactly what KlgLogReader produces: the same timestamps, depth and colour bytes.
#pragma once

#include <sys/types.h>

#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cofusion_hip.h"

namespace cofusion {

class CoFusion;

struct KlgFrame {
    int index = -1;         // frame number in the log
    int slot = -1;          // the slot that holds it (cf_frame_slot: depth u16 mm, and by colorKind header + coef or rgb)
    int64_t timestamp = 0;
    int colorKind = CF_FRAME_COLOR_NONE;   // _JPEG: front end output; _RAW: the log's 3 B/px; _DECODED: a JPEG the front end refused,
                                           // decoded on the host (decodeJpegRGB, libjpeg's channel order); _NONE: no colour block
};

class KlgPrefetcher {
  public:
    // slots: memory of at least two slots for width x height frames (coef_blocks >= 1; a JPEG with more blocks is decoded on the
    // host).  workers is clamped to 1..16 -- never sized by the machine's CPU count.
    KlgPrefetcher(const std::string& file, int width, int height, const std::vector<cf_frame_slot>& slots, int workers = 4);
    ~KlgPrefetcher();   // joins the workers; one that is mid-frame finishes that frame (milliseconds), none starts another
    KlgPrefetcher(const KlgPrefetcher&) = delete;
    bool ok() const { return fd >= 0; }
    const std::string& error() const { return err; }
    int getNumFrames() const { return numFrames; }
    int currentFrameIndex() const { return nextDeliver; }
    // referenceCompatible as KlgLogReader has it (stop one frame early like the reference's hasMore()); frameLimit >= 0: play at
    // most so many frames
    void setLimits(bool referenceCompatible, int frameLimit);
    bool hasMore() const;
    // The next frame in log order, whichever worker finished first: blocks until it is ready.  false: that frame failed (error()
    // names it; the frames before it were delivered), or there are no more frames.
    bool next(KlgFrame* out);
    // ... without blocking: 0 delivered, 1 not ready yet (or no more frames), -1 that frame failed
    int tryNext(KlgFrame* out);
    void release(int slot);   // the slot's memory goes back to the workers
    // Back to frame 0.  Every slot returns to the workers, those the caller still holds included.
    void rewind();

  private:
    struct Entry { uint64_t offset; int32_t depthSize, rgbSize; int64_t timestamp; };
    struct Result { int slot; int colorKind; std::string err; };
    void work();
    std::string decode(int index, const cf_frame_slot& mem, std::vector<uint8_t>& raw, int* colorKind);
    int deliver(KlgFrame* out, std::unique_lock<std::mutex>& lk, bool block);
    int limit() const;

    int fd = -1;
    std::string err;
    int width, height, numFrames = 0;
    std::vector<Entry> index;       // the frames whose header and payload lie inside the file
    std::string indexError;         // why frame index.size() cannot be read, if the log promises more frames than that
    std::vector<cf_frame_slot> mem;
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cvWork, cvReady;
    std::vector<int> freeSlots;
    std::map<int, Result> ready;    // finished frames waiting for their turn
    int nextClaim = 0, nextDeliver = 0, busy = 0;
    bool referenceCompatible = false;
    int frameLimit = -1;
    unsigned generation = 0;        // bumped by rewind(): results of an older generation are dropped
    bool stop = false;
};

class KlgPlayer {
  public:
    // Refused for a model-parallel instance (world > 1).  slots 0: workers + 3, at least 4, at most 16.
    KlgPlayer(CoFusion& cf, const std::string& file, bool flipColors = false, int workers = 4, int slots = 0);
    ~KlgPlayer();
    KlgPlayer(const KlgPlayer&) = delete;
    int getNumFrames() const { return prefetch->getNumFrames(); }
    void setLimits(bool referenceCompatible, int frameLimit);
    // The oldest frame: submits what the prefetcher has ready, up to slots - 2 frames ahead, and returns the frame's device buffers
    // (depth f32 [H*W] metres, rgba u8x4 [H*W]) acquired as the instance's deviceFramesComplete says: complete at return, or ordered
    // on the context's stream.  They stay intact until the next call of next() / process() / rewind().  false: end of the log.
    // Throws std::runtime_error at a frame that cannot be decoded (the frames before it were played).
    bool next(int64_t* timestamp, const float** depth_dev, const uint8_t** rgba_dev);
    bool process();   // next() + CoFusion::processFrame on the device entry
    void rewind();
    cf_frame_decoder* decoder() { return dec; }

  private:
    void releaseCurrent();
    CoFusion& cf;
    cf_ctx* ctx;
    cf_frame_decoder* dec = nullptr;
    KlgPrefetcher* prefetch = nullptr;
    int width, height, slots;
    bool flip;
    std::deque<KlgFrame> submitted;
    int current = -1;
    std::string pendingError;
};

}  // namespace cofusion
