// ExportWriter.cpp -- the ring of encoder slots and the writer threads of the asynchronous exports (ExportWriter.h).
#include <cerrno>
#include <cstring>
#include <stdexcept>

#include <fcntl.h>
#include <unistd.h>

#include "ExportWriter.h"

namespace cofusion {

namespace {

std::string writeFile(const std::string& path, const std::vector<uint8_t>& bytes)
{
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) return "cannot open " + path + ": " + strerror(errno);
    size_t done = 0;
    while (done < bytes.size()) {
        const ssize_t n = ::write(fd, bytes.data() + done, bytes.size() - done);
        if (n < 0) {
            if (errno == EINTR) continue;
            const std::string why = "cannot write " + path + ": " + strerror(errno);
            ::close(fd);
            return why;
        }
        done += (size_t)n;
    }
    if (::close(fd) != 0) return "cannot close " + path + ": " + strerror(errno);
    return "";
}

}  // namespace

ExportWriter::ExportWriter(cf_ctx* c, int maxWidth, int maxHeight, int workers, int nslots, int rowsPerBand) : ctx(c), slots(nslots)
{
    if (workers < 1 || workers > 8 || nslots < 2 || nslots > 16) throw std::runtime_error("asynchronous exports: 1..8 writer threads and 2..16 slots");
    if (cf_png_encoder_create(ctx, maxWidth, maxHeight, nslots, rowsPerBand, &enc) != CF_OK)
        throw std::runtime_error(std::string("cf_png_encoder_create failed: ") + cf_last_error(ctx));
    for (int s = nslots - 1; s >= 0; s--) freeSlots.push_back(s);
    for (int w = 0; w < workers; w++) threads.emplace_back([this] { work(); });
}

ExportWriter::~ExportWriter()
{
    {
        std::unique_lock<std::mutex> lk(m);
        slotFree.wait(lk, [this] { return busy == 0; });
        stop = true;
    }
    jobReady.notify_all();
    for (auto& t : threads) t.join();
    cf_png_encoder_destroy(enc);
}

void ExportWriter::submit(const std::string& path, const void* src_dev, int width, int height, int channels, int flags)
{
    int slot;
    {
        std::unique_lock<std::mutex> lk(m);
        if (freeSlots.empty()) {
            st.stalls++;
            slotFree.wait(lk, [this] { return !freeSlots.empty(); });
        }
        slot = freeSlots.back();
        freeSlots.pop_back();
        busy++;
    }
    if (cf_png_encoder_submit(enc, slot, src_dev, width, height, channels, flags) != CF_OK) {
        const std::string why = cf_last_error(ctx);
        {
            std::lock_guard<std::mutex> lk(m);
            freeSlots.push_back(slot);
            busy--;
        }
        slotFree.notify_all();
        throw std::runtime_error("cf_png_encoder_submit failed: " + why);
    }
    {
        std::lock_guard<std::mutex> lk(m);
        jobs.push_back(Job{slot, path});
    }
    jobReady.notify_one();
}

void ExportWriter::work()
{
    std::vector<uint8_t> file;
    for (;;) {
        Job job;
        {
            std::unique_lock<std::mutex> lk(m);
            jobReady.wait(lk, [this] { return stop || !jobs.empty(); });
            if (jobs.empty()) return;
            job = std::move(jobs.front());
            jobs.pop_front();
        }
        std::string why;
        cf_png_stream stream{};
        if (cf_png_encoder_acquire(enc, job.slot, &stream) != CF_OK) why = std::string("cf_png_encoder_acquire failed: ") + cf_last_error(ctx);
        else if (!(why = assemblePng(stream, &file)).empty()) why = job.path + ": " + why;
        else why = writeFile(job.path, file);
        {
            std::lock_guard<std::mutex> lk(m);
            if (why.empty()) { st.images++; st.bytes += file.size(); }
            else if (failure.empty()) failure = why;
            freeSlots.push_back(job.slot);
            busy--;
        }
        slotFree.notify_all();
    }
}

void ExportWriter::check()
{
    std::string why;
    {
        std::lock_guard<std::mutex> lk(m);
        why.swap(failure);
    }
    if (!why.empty()) throw std::runtime_error("asynchronous export: " + why);
}

void ExportWriter::flush()
{
    {
        std::unique_lock<std::mutex> lk(m);
        slotFree.wait(lk, [this] { return busy == 0; });
    }
    check();
}

ExportWriter::Stats ExportWriter::stats(bool timing)
{
    double ms = 0; uint64_t n = 0;
    {   // the encoder's events are read here: no slot may be in flight between its submit and its acquire meanwhile
        std::unique_lock<std::mutex> lk(m);
        slotFree.wait(lk, [this] { return busy == 0; });
    }
    if (cf_png_encoder_timing(enc, timing ? 1 : 0, &ms, &n) != CF_OK) throw std::runtime_error(std::string("cf_png_encoder_timing failed: ") + cf_last_error(ctx));
    std::lock_guard<std::mutex> lk(m);
    Stats out = st;
    out.deviceMs = ms; out.deviceImages = n;
    return out;
}

}  // namespace cofusion
