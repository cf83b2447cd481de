// export_check_main.cpp -- a stand-alone checker of assemblePng (host/PngAssemble.cpp) for a sanitizer build: `make export_check`
// compiles it with -fsanitize=address,undefined.  Synthetic band tables -- stored bands, a band in the fixed code, one band, a band of
// 65535 bytes, a partial last band -- go through assemblePng and the file is read back with the project's own pngDecode; tables that
// do not describe their image or point outside their slot (no band, a band too many, a truncated slot, a wrong size, no table) must be
// refused.  The band area is an exactly-sized heap block, so that a read past it is seen.  Host only: no GPU, no Python.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <zlib.h>

#include "ExportWriter.h"
#include "ImageIO.h"

namespace cofusion {   // ImageIO.cpp's serial reader refers to the JPEG decoder; this program reads no JPEG
std::string decodeJpegRGB(const uint8_t*, size_t, int, int, uint8_t*) { return "no JPEG decoder in this program"; }
}

using namespace cofusion;
using namespace cofusion::imageio;

namespace {

int failures = 0, accepted = 0, refused = 0;

void fail(const char* what, const std::string& why)
{
    fprintf(stderr, "FAILED %s: %s\n", what, why.c_str());
    failures++;
}

struct Synthetic {
    cf_png_stream st{};
    std::vector<cf_png_band> table;
    std::vector<uint8_t> data;      // exactly the bands
    std::vector<uint8_t> pixels;
};

uint8_t pixel(int i) { return (uint8_t)((i * 37 + (i >> 3)) & 255); }

// every band as a stored block of its scanlines, filter type 0
Synthetic storedImage(int w, int h, int channels, int rowsPerBand)
{
    Synthetic s;
    const int rb = w * channels;
    s.pixels.resize((size_t)rb * h);
    for (size_t i = 0; i < s.pixels.size(); i++) s.pixels[i] = pixel((int)i);
    for (int y0 = 0; y0 < h; y0 += rowsPerBand) {
        const int rows = h - y0 < rowsPerBand ? h - y0 : rowsPerBand;
        std::vector<uint8_t> S;
        for (int y = y0; y < y0 + rows; y++) {
            S.push_back(0);
            S.insert(S.end(), s.pixels.begin() + (size_t)y * rb, s.pixels.begin() + (size_t)(y + 1) * rb);
        }
        cf_png_band e;
        e.offset = (uint32_t)s.data.size(); e.bytes = (uint32_t)S.size() + 5; e.stream_bytes = (uint32_t)S.size();
        e.adler = (uint32_t)adler32(adler32(0L, Z_NULL, 0), S.data(), (uInt)S.size());
        const uint32_t n = (uint32_t)S.size();
        const uint8_t head[5] = {0, (uint8_t)(n & 255), (uint8_t)(n >> 8), (uint8_t)(~n & 255), (uint8_t)((~n >> 8) & 255)};
        s.data.insert(s.data.end(), head, head + 5);
        s.data.insert(s.data.end(), S.begin(), S.end());
        s.table.push_back(e);
    }
    s.st.width = w; s.st.height = h; s.st.channels = channels; s.st.rows_per_band = rowsPerBand;
    return s;
}

void bind(Synthetic& s)
{
    s.st.bands = (int)s.table.size();
    s.st.table = s.table.data(); s.st.data = s.data.data(); s.st.data_bytes = s.data.size();
}

// five zero bytes (a 4 x 1 grey image of zeros) in the fixed code: literal 0, a match of 4 at distance 1, end of block, then the
// empty stored block
Synthetic fixedBand()
{
    Synthetic s;
    std::vector<int> bits;
    auto lsb = [&](unsigned v, int n) { for (int i = 0; i < n; i++) bits.push_back((v >> i) & 1); };
    auto msb = [&](unsigned v, int n) { for (int i = n - 1; i >= 0; i--) bits.push_back((v >> i) & 1); };
    lsb(0, 1); lsb(1, 2);
    msb(0x30, 8);             // literal 0
    msb(258 - 256, 7);        // length 4
    msb(0, 5);                // distance 1
    msb(0, 7);                // end of block
    lsb(0, 3);                // BFINAL = 0, BTYPE = 00
    while (bits.size() % 8) bits.push_back(0);
    for (size_t i = 0; i < bits.size(); i += 8) {
        unsigned b = 0;
        for (int k = 0; k < 8; k++) b |= (unsigned)bits[i + k] << k;
        s.data.push_back((uint8_t)b);
    }
    const uint8_t tail[4] = {0, 0, 0xff, 0xff};
    s.data.insert(s.data.end(), tail, tail + 4);
    const uint8_t S[5] = {0, 0, 0, 0, 0};
    cf_png_band e;
    e.offset = 0; e.bytes = (uint32_t)s.data.size(); e.stream_bytes = 5;
    e.adler = (uint32_t)adler32(adler32(0L, Z_NULL, 0), S, 5);
    s.table.push_back(e);
    s.pixels.assign(4, 0);
    s.st.width = 4; s.st.height = 1; s.st.channels = 1; s.st.rows_per_band = 8;
    return s;
}

void mustDecode(const char* what, Synthetic& s)
{
    bind(s);
    std::vector<uint8_t> file;
    const std::string why = assemblePng(s.st, &file);
    if (!why.empty()) return fail(what, "refused: " + why);
    const int bpp = s.st.channels;
    std::vector<uint8_t> exact(file), scan(pngScanBytes(s.st.width, s.st.height, bpp)), palette(768);
    PngInfo info;
    const std::string e = pngDecode(exact.data(), exact.size(), bpp == 4 ? ROLE_COLOR : ROLE_MASK, &info, scan.data(), scan.size(), palette.data());
    if (!e.empty()) return fail(what, "pngDecode: " + e);
    if (info.width != s.st.width || info.height != s.st.height || info.bitDepth != 8 || info.colorType != (bpp == 4 ? 6 : 0) || info.bpp != bpp)
        return fail(what, "another header than was written");
    const size_t rb = (size_t)bpp * s.st.width;
    for (int y = 0; y < s.st.height; y++)
        if (memcmp(&scan[(size_t)y * (rb + 1) + 1], &s.pixels[(size_t)y * rb], rb) != 0) return fail(what, "other pixels than were written");
    accepted++;
}

void mustRefuse(const char* what, Synthetic& s, bool rebind = true)
{
    if (rebind) bind(s);
    std::vector<uint8_t> file;
    if (assemblePng(s.st, &file).empty()) return fail(what, "accepted");
    if (!file.empty()) return fail(what, "refused, but left bytes behind");
    refused++;
}

}  // namespace

int main()
{
    { Synthetic s = storedImage(7, 3, 1, 4); mustDecode("one band", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); mustDecode("four bands, the last one partial", s); }
    { Synthetic s = storedImage(1, 1, 1, 1); mustDecode("1 x 1", s); }
    { Synthetic s = storedImage(256, 255, 1, 255); mustDecode("a stored band of 65535 bytes", s); }
    { Synthetic s = storedImage(256, 300, 1, 255); mustDecode("a band of 65535 bytes and a partial one", s); }
    { Synthetic s = fixedBand(); mustDecode("a band in the fixed code", s); }
    { Synthetic s = storedImage(1280, 16, 4, 8); mustDecode("the widest row", s); }

    { Synthetic s = storedImage(7, 3, 1, 4); s.table.clear(); s.data.clear(); mustRefuse("no band", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.table.pop_back(); mustRefuse("a band short", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.table.push_back(s.table.back()); mustRefuse("a band too many", s); }
    for (int cut = 1; cut <= 40; cut += 13) {
        Synthetic s = storedImage(5, 7, 4, 2);
        s.data.resize(s.data.size() - (size_t)cut);   // a truncated slot: the last band (and with 40, the one before) reaches past it
        std::vector<uint8_t> exact(s.data); s.data.swap(exact);
        mustRefuse("a truncated slot", s);
    }
    { Synthetic s = storedImage(5, 7, 4, 2); s.table[1].offset = 0xfffffff0u; mustRefuse("an offset that wraps", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.table[2].stream_bytes++; mustRefuse("a band of another size", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.table[3].stream_bytes = s.table[0].stream_bytes; mustRefuse("a partial band that claims to be whole", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.table[0].bytes = 4; mustRefuse("a band too short to be one", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.st.channels = 3; mustRefuse("three channels", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.st.height = 0; mustRefuse("no rows", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); s.st.rows_per_band = 0; mustRefuse("no rows per band", s); }
    { Synthetic s = storedImage(256, 300, 1, 255); s.st.rows_per_band = 256; mustRefuse("a band beyond one stored block", s); }
    { Synthetic s = storedImage(5, 7, 4, 2); bind(s); s.st.table = nullptr; mustRefuse("no table", s, false); }
    { Synthetic s = storedImage(5, 7, 4, 2); bind(s); s.st.data = nullptr; mustRefuse("no band area", s, false); }

    printf("export_check: %d accepted, %d refused, %d failed\n", accepted, refused, failures);
    return failures ? 1 : 0;
}
