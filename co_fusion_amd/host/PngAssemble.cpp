// PngAssemble.cpp -- assemblePng (ExportWriter.h): the file around the bands the device encoded.  Host only, no GPU calls: it is also
// what the sanitizer build drives (export_check_main.cpp, `make export_check`).
#include <cstring>

#include <zlib.h>

#include "ExportWriter.h"

namespace cofusion {

namespace {

void be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// closes the chunk that starts at `at` (length field, type, body up to the vector's end): fills in the length, appends the CRC
void closeChunk(std::vector<uint8_t>& f, size_t at)
{
    const size_t body = f.size() - at - 8;
    be32(&f[at], (uint32_t)body);
    const uLong c = crc32(crc32(0L, Z_NULL, 0), &f[at + 4], (uInt)(body + 4));
    uint8_t tail[4]; be32(tail, (uint32_t)c);
    f.insert(f.end(), tail, tail + 4);
}

size_t openChunk(std::vector<uint8_t>& f, const char* type)
{
    const size_t at = f.size();
    f.resize(at + 8);
    memcpy(&f[at + 4], type, 4);
    return at;
}

}  // namespace

std::string assemblePng(const cf_png_stream& s, std::vector<uint8_t>* out)
{
    out->clear();
    if (s.width < 1 || s.height < 1 || (s.channels != 1 && s.channels != 4) || s.rows_per_band < 1) return "not an 8-bit grey or RGBA image";
    const int64_t row = 1 + (int64_t)s.channels * s.width;
    if (row * s.rows_per_band > 65535) return "a band larger than one stored block";
    const int64_t bands = ((int64_t)s.height + s.rows_per_band - 1) / s.rows_per_band;
    if (s.bands != bands) return "the band table does not cover the image";
    if (!s.table || !s.data) return "no band table";
    uint64_t body = 2 + 2 + 4;
    for (int b = 0; b < s.bands; b++) {
        const cf_png_band& e = s.table[b];
        const int64_t rows = b + 1 < s.bands ? s.rows_per_band : s.height - (int64_t)b * s.rows_per_band;
        if (e.stream_bytes != (uint64_t)(row * rows)) return "a band of another size than its rows";
        // the shortest band there is: a stored block of its bytes or, in the fixed code, one literal, the end of the block and the
        // empty stored block
        if (e.bytes < 5 || (uint64_t)e.offset + e.bytes > s.data_bytes) return "a band outside the slot";
        body += e.bytes;
    }
    if (body > 0x7fffffffu) return "an IDAT chunk beyond 2^31 - 1 bytes";
    std::vector<uint8_t>& f = *out;
    f.reserve((size_t)body + 8 + 25 + 12 + 12);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    f.insert(f.end(), sig, sig + 8);
    size_t at = openChunk(f, "IHDR");
    uint8_t ihdr[13];
    be32(ihdr, (uint32_t)s.width); be32(ihdr + 4, (uint32_t)s.height);
    ihdr[8] = 8; ihdr[9] = s.channels == 4 ? 6 : 0; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    f.insert(f.end(), ihdr, ihdr + 13);
    closeChunk(f, at);
    at = openChunk(f, "IDAT");
    f.push_back(0x78); f.push_back(0x01);
    uLong adler = adler32(0L, Z_NULL, 0);
    for (int b = 0; b < s.bands; b++) {
        const cf_png_band& e = s.table[b];
        f.insert(f.end(), s.data + e.offset, s.data + e.offset + e.bytes);
        adler = adler32_combine(adler, e.adler, (z_off_t)e.stream_bytes);
    }
    f.push_back(0x03); f.push_back(0x00);   // the final block: fixed code, end-of-block at once
    uint8_t sum[4]; be32(sum, (uint32_t)adler);
    f.insert(f.end(), sum, sum + 4);
    closeChunk(f, at);
    at = openChunk(f, "IEND");
    closeChunk(f, at);
    return "";
}

}  // namespace cofusion
