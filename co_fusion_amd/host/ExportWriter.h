// ExportWriter.h -- the host half of the asynchronous per-frame exports.  The device encodes an image into the
// bands of a PNG data stream (csrc/png_encode.hip: cf_png_encoder); here
//   assemblePng   a pure function: signature, IHDR, one IDAT (78 01, the bands, 03 00, the Adler-32 combined over the band table),
//                 IEND.  zlib's crc32 over the chunk is the only pass a host core makes over an image.  No GPU calls.
//   ExportWriter  a ring of encoder slots and writer threads, each doing acquire -> assemble -> write -> close -> free the slot.  The
//                 frame thread only submits; it blocks when every slot is busy (counted), nothing is dropped.  A failed write is
//                 remembered and thrown by check() / flush().
#pragma once

#include <condition_variable>
#include <cstdint>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cofusion_hip.h"

namespace cofusion {

// "" or why the stream is refused (a table that does not describe the image, a band outside the slot).  `out` is replaced.
std::string assemblePng(const cf_png_stream& stream, std::vector<uint8_t>* out);

class ExportWriter {
  public:
    struct Stats { uint64_t images = 0, bytes = 0, stalls = 0, deviceImages = 0; double deviceMs = 0; };
    // 2: the fastest of 2 / 4 / 8 / 16 at 640x480 on every kind of image (240 workgroups instead of 60; a band costs
    // 5 bytes, or a file of label masks a fifth more than with 8)
    static constexpr int kDefaultRowsPerBand = 2;
    ExportWriter(cf_ctx* ctx, int maxWidth, int maxHeight, int workers, int slots, int rowsPerBand = kDefaultRowsPerBand);
    ~ExportWriter();   // writes what was submitted; a failure at this point is dropped
    ExportWriter(const ExportWriter&) = delete;
    ExportWriter& operator=(const ExportWriter&) = delete;
    // the calling (frame) thread: encodes src_dev on the context's stream into a free slot and queues the file; no host wait unless
    // every slot is busy
    void submit(const std::string& path, const void* src_dev, int width, int height, int channels, int flags);
    void flush();      // returns when every submitted file is closed; throws the remembered failure
    void check();      // throws the remembered failure, if there is one (and forgets it)
    // timing: the encoder's diagnostics mode from here on; the device sums are those since the last call
    Stats stats(bool timing);

  private:
    struct Job { int slot; std::string path; };
    void work();
    cf_ctx* ctx;
    cf_png_encoder* enc = nullptr;
    std::mutex m;
    std::condition_variable jobReady, slotFree;
    std::deque<Job> jobs;
    std::vector<int> freeSlots;
    int slots, busy = 0;     // busy: submitted and not yet closed
    bool stop = false;
    std::string failure;
    Stats st;
    std::vector<std::thread> threads;
};

}  // namespace cofusion
