// klg_prefetch_check.cpp -- the log player's prefetcher (host/KlgPrefetch.cpp) against the serial reader (host/KlgIO.cpp), as a
// program of its own for the thread and address sanitizers: tests/test_cpu_klg_player.py compiles it with KlgPrefetch.cpp, KlgIO.cpp
// and Jpeg.cpp (no HIP, no Python) and runs it on a log of mixed frame kinds.
//   klg_prefetch_check <log> <width> <height> <workers>
// Plays the log twice through the prefetcher (the second time after a rewind with frames in flight), compares every frame with the
// reader's -- timestamp, depth, and colour finished by the host back end -- and destroys the prefetcher mid-way.  Exit 0 and
// "<n> frames ok" when everything matched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../co_fusion_amd/host/KlgIO.h"
#include "../../co_fusion_amd/host/KlgPlayer.h"

namespace cofusion {
void jpegFinishHost(const cf_jpeg_header* hdr, const int16_t* coef, uint8_t* rgb);
}
using namespace cofusion;

struct Slots {
    std::vector<std::vector<uint8_t>> store;
    std::vector<cf_frame_slot> mem;
    Slots(int n, int W, int H)
    {
        const size_t N = (size_t)W * H, blocks = (size_t)CF_JPEG_MAX_BLOCKS(W, H);
        const size_t offDepth = 512 + blocks * 128, offRgb = offDepth + ((N * 2 + 15) & ~(size_t)15);
        for (int s = 0; s < n; s++) {
            store.emplace_back(offRgb + N * 3);
            uint8_t* b = store.back().data();
            mem.push_back(cf_frame_slot{reinterpret_cast<cf_jpeg_header*>(b), reinterpret_cast<int16_t*>(b + 512), blocks,
                                        reinterpret_cast<uint16_t*>(b + offDepth), b + offRgb});
        }
    }
};

static const cf_frame_slot* g_slots = nullptr;   // the slot table handed to the prefetcher

static int fail(const char* what, int frame)
{
    fprintf(stderr, "frame %d: %s\n", frame, what);
    return 1;
}

// one pass over the log: `frames` frames (-1: all) against a fresh serial reader
static int play(KlgPrefetcher& p, const std::string& log, int W, int H, int frames, int* played)
{
    KlgLogReader r(log, W, H, false);
    if (!r.ok()) return fail("the reader cannot open the log", -1);
    const size_t N = (size_t)W * H;
    std::vector<uint8_t> rgb(N * 3);
    int held = -1, n = 0;
    while (p.hasMore() && (frames < 0 || n < frames)) {
        KlgFrame f;
        if (!p.next(&f)) { fprintf(stderr, "%s\n", p.error().c_str()); return 1; }
        if (held >= 0) p.release(held);
        held = f.slot;
        if (!r.getNext()) return fail("the reader has no such frame", n);
        if (f.index != n || f.timestamp != r.timestamp) return fail("timestamp / order", n);
        *played = ++n;
        const cf_frame_slot& m = g_slots[f.slot];
        for (size_t i = 0; i < N; i++)
            if ((float)m.depth[i] * 0.001f != r.depth[i]) return fail("depth", n - 1);
        bool reversed = true;   // a decoded JPEG is stored reversed by the reader (flip_colors off)
        if (f.colorKind == CF_FRAME_COLOR_JPEG) jpegFinishHost(m.header, m.coef, rgb.data());
        else if (f.colorKind == CF_FRAME_COLOR_NONE) memset(rgb.data(), 0, N * 3);
        else { memcpy(rgb.data(), m.rgb, N * 3); reversed = f.colorKind == CF_FRAME_COLOR_DECODED; }
        for (size_t i = 0; i < N; i++)
            for (int c = 0; c < 3; c++)
                if (rgb[i * 3 + (reversed ? 2 - c : c)] != r.rgb[i * 3 + c]) return fail("colour", n - 1);
    }
    if (held >= 0) p.release(held);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: klg_prefetch_check <log> <width> <height> <workers>\n"); return 2; }
    const std::string log = argv[1];
    const int W = atoi(argv[2]), H = atoi(argv[3]), workers = atoi(argv[4]);
    Slots slots(workers + 2, W, H);
    g_slots = slots.mem.data();
    int played = 0, total = 0;
    {
        KlgPrefetcher p(log, W, H, slots.mem, workers);
        if (!p.ok()) { fprintf(stderr, "%s\n", p.error().c_str()); return 1; }
        if (play(p, log, W, H, -1, &played)) return 1;
        total = played;
        if (total != p.getNumFrames()) return fail("not every frame was played", total);
        p.rewind();
        if (play(p, log, W, H, 3, &played)) return 1;   // three frames, the workers are ahead ...
        p.rewind();                                     // ... rewind with frames in flight
        if (play(p, log, W, H, -1, &played) || played != total) return fail("the replay differs", played);
        p.rewind();
        if (play(p, log, W, H, 1, &played)) return 1;
    }   // destroyed with the workers mid-frame
    printf("%d frames ok\n", total);
    return 0;
}
