// ImagePlayer.h -- plays an image-sequence dataset at tracker speed, the counterpart of KlgPlayer.h for
// directories of image files.  The reference decodes these files with OpenCV on one buffering thread; the frames of a set do not
// depend on each other, so here
//   ImagePrefetcher      reads ahead on worker threads: read the files of a frame, inflate, undo the PNG filters, run the JPEG front
//                        end (host/ImageIO.cpp, host/Jpeg.cpp) into slot memory the owner hands in, and describe the frame as a
//                        cf_image_desc; frames are delivered strictly in order.  No GPU calls.
//   ImageSequencePlayer  a prefetcher over the pinned slots of a cf_frame_decoder with images enabled (csrc/image_decode.hip), which
//                        finishes the frames on the device, feeding CoFusion::processFrame through its device entry -- the masked one
//                        where the set has masks.
// Both produce exactly what ImageSequenceReader produces: the same timestamps, depth, colour and mask bytes.
#pragma once

#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ImageIO.h"

namespace cofusion {

class CoFusion;

struct ImageSlotMem { cf_frame_slot frame; cf_image_slot image; };   // one slot's staging: the .klg half (JPEG, raw colour) and the image half

struct ImageFrame {
    int index = -1, slot = -1;
    int64_t timestamp = 0;
    cf_image_desc desc{};
};

class ImagePrefetcher {
  public:
    // slots: memory of at least two slots for width x height frames.  workers is clamped to 1..16 -- never sized by the CPU count.
    ImagePrefetcher(const imageio::SequenceLayout& layout, int width, int height, const std::vector<ImageSlotMem>& slots, int workers = 4);
    ~ImagePrefetcher();   // joins the workers; one that is mid-frame finishes that frame, none starts another
    ImagePrefetcher(const ImagePrefetcher&) = delete;
    const std::string& error() const { return err; }
    int getNumFrames() const { return lay.numFrames; }
    void setLimits(int frameLimit);   // >= 0: play at most so many frames
    bool hasMore() const;
    // The next frame in order, whichever worker finished first: blocks until it is ready.  false: that frame failed (error() names
    // the file; the frames before it were delivered), or there are no more frames.
    bool next(ImageFrame* out);
    int tryNext(ImageFrame* out);   // without blocking: 0 delivered, 1 not ready yet (or no more frames), -1 that frame failed
    void release(int slot);         // the slot's memory goes back to the workers
    void rewind();                  // back to frame 0; every slot returns to the workers, those the caller still holds included
    imageio::DecodeTimes times();   // accumulated over all workers: seconds spent reading, in inflate(), unfiltering, and in the rest of the parsers

  private:
    struct Result { int slot; cf_image_desc desc; std::string err; };
    void work();
    std::string decode(int index, const ImageSlotMem& mem, std::vector<uint8_t>& file, cf_image_desc* desc, imageio::DecodeTimes* t);
    int deliver(ImageFrame* out, std::unique_lock<std::mutex>& lk, bool block);
    int limit() const;

    imageio::SequenceLayout lay;
    std::string err;
    int width, height;
    std::vector<ImageSlotMem> mem;
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cvWork, cvReady;
    std::vector<int> freeSlots;
    std::map<int, Result> ready;    // finished frames waiting for their turn
    int nextClaim = 0, nextDeliver = 0, busy = 0;
    int frameLimit = -1;
    unsigned generation = 0;        // bumped by rewind(): results of an older generation are dropped
    bool stop = false;
    imageio::DecodeTimes sum;
};

class ImageSequencePlayer {
  public:
    // Refused for a model-parallel instance (world > 1) and for a set whose frames are not the instance's size.  slots 0: workers + 3,
    // at least 4, at most 16.
    ImageSequencePlayer(CoFusion& cf, const imageio::SequenceOptions& opt, int workers = 4, int slots = 0);
    ~ImageSequencePlayer();
    ImageSequencePlayer(const ImageSequencePlayer&) = delete;
    const imageio::SequenceLayout& layout() const { return lay; }
    int getNumFrames() const { return lay.numFrames; }
    void setLimits(int frameLimit) { prefetch->setLimits(frameLimit); }
    // The oldest frame: submits what the prefetcher has ready, up to slots - 2 frames ahead, and returns the frame's device buffers
    // (depth f32 [H*W], rgba u8x4 [H*W], mask u8 [H*W] or null) acquired as the instance's deviceFramesComplete says.  They stay intact
    // until the next call of next() / process() / rewind().  false: end of the set.  Throws std::runtime_error at a frame that cannot
    // be decoded (the frames before it were played); the message names the file.
    bool next(int64_t* timestamp, const float** depth_dev, const uint8_t** rgba_dev, const uint8_t** mask_dev);
    bool process();   // next() + CoFusion::processFrame on the device entry, masked where the frame has a mask
    void rewind();
    imageio::DecodeTimes times() { return prefetch->times(); }

  private:
    void releaseCurrent();
    CoFusion& cf;
    cf_ctx* ctx;
    cf_frame_decoder* dec = nullptr;
    ImagePrefetcher* prefetch = nullptr;
    imageio::SequenceLayout lay;
    int width, height, slots = 0;
    std::deque<ImageFrame> submitted;
    int current = -1;
    std::string pendingError;
};

}  // namespace cofusion
