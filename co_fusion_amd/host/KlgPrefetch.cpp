// KlgPrefetch.cpp -- KlgPrefetcher (KlgPlayer.h): worker threads that read a .klg log ahead.  Host code only: no GPU calls, so it
// links without the C-ABI library (tests/native/klg_prefetch_check.cpp runs it under the thread and address sanitizers).
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <cstring>

#include "KlgPlayer.h"

namespace cofusion {

std::string decodeJpegRGB(const uint8_t* data, size_t size, int width, int height, uint8_t* rgb);  // Jpeg.cpp
std::string jpegFront(const uint8_t* data, size_t size, int width, int height, cf_jpeg_header* hdr, int16_t* coef, size_t capBlocks, bool* refused);

namespace {
bool preadAll(int fd, void* dst, size_t n, uint64_t off)
{
    uint8_t* p = static_cast<uint8_t*>(dst);
    while (n) {
        const ssize_t r = pread(fd, p, n, (off_t)off);
        if (r <= 0) return false;
        p += r; n -= (size_t)r; off += (uint64_t)r;
    }
    return true;
}
}  // namespace

KlgPrefetcher::KlgPrefetcher(const std::string& file, int w, int h, const std::vector<cf_frame_slot>& slots, int workers)
    : width(w), height(h), mem(slots)
{
    if (w <= 0 || h <= 0 || slots.size() < 2) { err = "KlgPrefetcher: a frame size and at least two slots"; return; }
    fd = open(file.c_str(), O_RDONLY);
    if (fd < 0) { err = "could not open log-file: " + file; return; }
    int32_t n = 0;
    if (!preadAll(fd, &n, sizeof(n), 0)) { err = "could not read the frame count of " + file; close(fd); fd = -1; return; }
    numFrames = n < 0 ? 0 : n;
    // one walk over the frame headers: the offset index.  A log that ends early keeps the frames that are whole; the first one that
    // is not is reported at its position (KlgLogReader fails there too, and plays the frames before it).
    const uint64_t fileSize = (uint64_t)lseek(fd, 0, SEEK_END);
    const size_t N = (size_t)w * h;
    uint64_t off = sizeof(int32_t);
    for (int i = 0; i < numFrames; i++) {
        uint8_t hd[16];
        if (off + 16 > fileSize || !preadAll(fd, hd, 16, off)) { indexError = "truncated frame header"; break; }
        Entry e;
        memcpy(&e.timestamp, hd, 8); memcpy(&e.depthSize, hd + 8, 4); memcpy(&e.rgbSize, hd + 12, 4);
        if (e.depthSize < 0 || e.rgbSize < 0 || (size_t)e.depthSize > N * 2 + 1024 || (size_t)e.rgbSize > N * 3 + 1024) { indexError = "implausible frame sizes"; break; }
        e.offset = off + 16;
        if (e.offset + (uint64_t)e.depthSize > fileSize) { indexError = "truncated depth block"; break; }
        if (e.offset + (uint64_t)e.depthSize + (uint64_t)e.rgbSize > fileSize) { indexError = "truncated rgb block"; break; }
        index.push_back(e);
        off = e.offset + (uint64_t)e.depthSize + (uint64_t)e.rgbSize;
    }
    for (int s = (int)mem.size() - 1; s >= 0; s--) freeSlots.push_back(s);
    workers = workers < 1 ? 1 : (workers > 16 ? 16 : workers);
    for (int t = 0; t < workers; t++) threads.emplace_back([this] { work(); });
}

KlgPrefetcher::~KlgPrefetcher()
{
    {
        std::lock_guard<std::mutex> lk(m);
        stop = true;
    }
    cvWork.notify_all(); cvReady.notify_all();
    for (auto& t : threads) t.join();
    if (fd >= 0) close(fd);
}

int KlgPrefetcher::limit() const
{
    int n = referenceCompatible ? numFrames - 1 : numFrames;
    if (frameLimit >= 0 && frameLimit < n) n = frameLimit;
    return n < 0 ? 0 : n;
}

void KlgPrefetcher::setLimits(bool refCompatible, int maxFrames)
{
    {
        std::lock_guard<std::mutex> lk(m);
        referenceCompatible = refCompatible; frameLimit = maxFrames;
    }
    cvWork.notify_all();
}

bool KlgPrefetcher::hasMore() const { return fd >= 0 && nextDeliver < limit(); }

// One frame into a slot, as KlgLogReader::getNext decodes it (same checks, same error texts) up to the coefficient boundary.
std::string KlgPrefetcher::decode(int i, const cf_frame_slot& s, std::vector<uint8_t>& raw, int* colorKind)
{
    const Entry& e = index[(size_t)i];
    const size_t N = (size_t)width * height;
    raw.resize((size_t)e.depthSize + (size_t)e.rgbSize + 1);
    if (!preadAll(fd, raw.data(), (size_t)e.depthSize + (size_t)e.rgbSize, e.offset)) return "truncated depth block";
    if ((size_t)e.depthSize != N * 2) {
        uLongf len = (uLongf)(N * 2);
        if (uncompress(reinterpret_cast<Bytef*>(s.depth), &len, raw.data(), (uLong)e.depthSize) != Z_OK || len != N * 2)
            return "zlib: depth block does not decompress to width*height u16";
    } else {
        memcpy(s.depth, raw.data(), N * 2);
    }
    const uint8_t* c = raw.data() + e.depthSize;
    if (e.rgbSize <= 0) { *colorKind = CF_FRAME_COLOR_NONE; return ""; }
    if ((size_t)e.rgbSize == N * 3) { memcpy(s.rgb, c, N * 3); *colorKind = CF_FRAME_COLOR_RAW; return ""; }
    bool refused = false;
    std::string je = jpegFront(c, (size_t)e.rgbSize, width, height, s.header, s.coef, (size_t)s.coef_blocks, &refused);
    *colorKind = CF_FRAME_COLOR_JPEG;
    if (je.empty() && refused) {   // not a stream the device path reproduces: the whole host decoder instead
        je = decodeJpegRGB(c, (size_t)e.rgbSize, width, height, s.rgb);
        *colorKind = CF_FRAME_COLOR_DECODED;
    }
    if (!je.empty()) return "JPEG colour frame: " + je;
    return "";
}

void KlgPrefetcher::work()
{
    std::vector<uint8_t> raw;
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
        // a frame number and a slot are taken together, in log order: the frame whose turn it is always owns a slot
        cvWork.wait(lk, [&] { return stop || (!freeSlots.empty() && nextClaim < limit() && nextClaim <= (int)index.size()); });
        if (stop) return;
        const int i = nextClaim++;
        const unsigned gen = generation;
        Result r{-1, CF_FRAME_COLOR_NONE, ""};
        if (i >= (int)index.size()) {   // the frame the index ends at: delivered as an error at its position; nothing follows it
            nextClaim = 0x7fffffff;
            r.err = indexError.empty() ? "no more frames" : indexError;
        } else {
            r.slot = freeSlots.back(); freeSlots.pop_back();
            busy++;
            lk.unlock();
            r.err = decode(i, mem[(size_t)r.slot], raw, &r.colorKind);
            lk.lock();
            busy--;
            if (gen != generation || stop) {   // rewound meanwhile: rewind() takes the slot back itself
                cvReady.notify_all();
                continue;
            }
        }
        ready[i] = r;
        cvReady.notify_all();
    }
}

int KlgPrefetcher::deliver(KlgFrame* out, std::unique_lock<std::mutex>& lk, bool block)
{
    if (fd < 0) return -1;
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
        if (r.slot >= 0) { freeSlots.push_back(r.slot); cvWork.notify_all(); }
        nextDeliver = 0x7ffffff0;   // nothing is played behind a frame that failed (as the reader: its file position is lost)
        return -1;
    }
    out->index = nextDeliver; out->slot = r.slot; out->colorKind = r.colorKind; out->timestamp = index[(size_t)nextDeliver].timestamp;
    nextDeliver++;
    return 0;
}

bool KlgPrefetcher::next(KlgFrame* out)
{
    std::unique_lock<std::mutex> lk(m);
    return deliver(out, lk, true) == 0;
}

int KlgPrefetcher::tryNext(KlgFrame* out)
{
    std::unique_lock<std::mutex> lk(m);
    return deliver(out, lk, false);
}

void KlgPrefetcher::release(int slot)
{
    if (slot < 0 || slot >= (int)mem.size()) return;
    {
        std::lock_guard<std::mutex> lk(m);
        for (int s : freeSlots) if (s == slot) return;
        freeSlots.push_back(slot);
    }
    cvWork.notify_all();
}

void KlgPrefetcher::rewind()
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

}  // namespace cofusion
