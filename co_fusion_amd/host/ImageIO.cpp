// ImageIO.cpp -- see ImageIO.h.  Formats: PNG (ISO/IEC 15948: chunks, CRC-32, zlib stream, the five scanline filters), OpenEXR
// (the "OpenEXR File Layout" document: magic, version flags, attribute list, offset table, scanline blocks; ZIP = zlib + byte
// predictor + half-split interleave), PNM (netpbm's ppm/pgm pages).  Directory rules: GUI/Tools/ImageLogReader.cpp of the reference.
#include "ImageIO.h"

#include <dirent.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace cofusion {

std::string decodeJpegRGB(const uint8_t* data, size_t size, int width, int height, uint8_t* rgb);  // Jpeg.cpp

namespace imageio {

namespace {

constexpr int kMaxSide = 16384;

double now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
uint32_t le32(const uint8_t* p) { return (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0]; }
uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p + 4) << 32 | le32(p); }

// a zlib stream fed in pieces; the output must come to exactly `want` bytes and the stream must end (Adler-32 checked by inflate)
struct Inflater {
    z_stream z;
    bool live = false;
    double seconds = 0;   // spent inside inflate()
    Inflater() { memset(&z, 0, sizeof(z)); }
    ~Inflater() { if (live) inflateEnd(&z); }
    bool begin(uint8_t* out, size_t want)
    {
        if (inflateInit(&z) != Z_OK) return false;
        live = true;
        z.next_out = out; z.avail_out = (uInt)want;
        return true;
    }
    // 0: wants more input; 1: stream ended; -1: error
    int feed(const uint8_t* in, size_t n, std::string* why)
    {
        z.next_in = const_cast<Bytef*>(in); z.avail_in = (uInt)n;
        const double t0 = now();
        const int rc = inflate(&z, Z_SYNC_FLUSH);
        seconds += now() - t0;
        if (rc == Z_STREAM_END) return 1;
        if (rc == Z_OK || rc == Z_BUF_ERROR) {
            if (z.avail_in > 0) { *why = "the compressed stream holds more pixels than the header announces"; return -1; }
            return 0;
        }
        const std::string msg = z.msg ? z.msg : "";
        *why = msg == "incorrect data check" ? "zlib Adler-32 mismatch" : "corrupt zlib stream (" + (msg.empty() ? std::to_string(rc) : msg) + ")";
        return -1;
    }
};

int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

std::string pnmHeader(const uint8_t* data, size_t n, const char* magic, const char* what, int* width, int* height, size_t* pos_out)
{
    size_t pos = 0;
    std::string tok[4];
    auto space = [](uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; };
    for (int t = 0; t < 4; t++) {
        while (pos < n && (space(data[pos]) || data[pos] == '#')) {
            if (data[pos] == '#') { while (pos < n && data[pos] != '\n' && data[pos] != '\r') pos++; }
            else pos++;
        }
        const size_t start = pos;
        while (pos < n && !space(data[pos]) && data[pos] != '#') pos++;
        if (start == pos) return std::string(what) + ": truncated header";
        tok[t].assign(reinterpret_cast<const char*>(data + start), pos - start);
    }
    if (tok[0] != magic) return std::string(what) + ": magic '" + tok[0] + "', only binary " + what + " (" + magic + ") is supported";
    long v[3];
    for (int t = 0; t < 3; t++) {
        const std::string& s = tok[t + 1];
        if (s.empty() || s.size() > 9 || s.find_first_not_of("0123456789") != std::string::npos)
            return std::string(what) + ": width, height and maxval must be decimal numbers";
        v[t] = atol(s.c_str());
    }
    if (v[0] <= 0 || v[1] <= 0 || v[0] > kMaxSide || v[1] > kMaxSide) return std::string(what) + ": image size outside 1..16384";
    if (v[2] <= 0 || v[2] > 255) return std::string(what) + ": maxval " + std::to_string(v[2]) + ": samples are 8 bits (maxval <= 255)";
    if (pos >= n || !space(data[pos])) return std::string(what) + ": no whitespace after maxval";
    pos++;
    *width = (int)v[0]; *height = (int)v[1]; *pos_out = pos;
    return "";
}

}  // namespace

float halfToFloat(uint16_t h)
{
    const uint32_t s = (uint32_t)(h >> 15) << 31;
    uint32_t e = (h >> 10) & 31, m = h & 1023, bits;
    if (e == 0) {
        if (m == 0) bits = s;
        else {
            int sh = 0;
            while (!(m & 1024)) { m <<= 1; sh++; }
            bits = s | (uint32_t)(113 - sh) << 23 | (m & 1023) << 13;
        }
    } else if (e == 31) bits = s | 0x7f800000u | m << 13;
    else bits = s | (e + 112) << 23 | m << 13;
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

std::string pngDecode(const uint8_t* data, size_t n, Role role, PngInfo* info, uint8_t* scan, size_t cap, uint8_t* palette, DecodeTimes* times)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (n < 8 || memcmp(data, sig, 8) != 0) return "not a PNG file (signature)";
    size_t pos = 8;
    bool haveHeader = false, havePalette = false, ended = false, streamEnd = false, sawData = false;
    PngInfo pi;
    Inflater inf;
    size_t want = 0;
    const double t0 = now();
    while (!ended) {
        if (n - pos < 12) return "truncated: the file ends inside a chunk header";
        const uint32_t len = be32(data + pos);
        const uint8_t* type = data + pos + 4;
        std::string name(type, type + 4);
        for (char& c : name) if (c < 0x20 || c > 0x7e) c = '?';   // a damaged type field must not put raw bytes into a message
        if (len > 0x7fffffffu || (size_t)len > n - pos - 12) return "truncated: chunk '" + name + "' runs past the end of the file";
        const uint8_t* body = data + pos + 8;
        const bool critical = !(type[0] & 0x20);
        if (critical && (uint32_t)crc32(crc32(0, nullptr, 0), type, 4 + len) != be32(body + len)) return "CRC mismatch in chunk '" + name + "'";
        pos += 12 + (size_t)len;
        if (!haveHeader && name != "IHDR") return "the first chunk is '" + name + "', not IHDR";
        if (name == "IHDR") {
            if (haveHeader || len != 13) return "malformed IHDR";
            haveHeader = true;
            const uint32_t w = be32(body), h = be32(body + 4);
            if (w < 1 || h < 1 || w > (uint32_t)kMaxSide || h > (uint32_t)kMaxSide) return "image size outside 1..16384";
            pi.width = (int)w; pi.height = (int)h; pi.bitDepth = body[8]; pi.colorType = body[9];
            if (body[10] != 0 || body[11] != 0) return "unknown compression or filter method";
            if (body[12] == 1) return "Adam7 interlacing is not supported";
            if (body[12] != 0) return "unknown interlace method";
            const int ct = pi.colorType, bd = pi.bitDepth;
            const bool legal = (ct == 0 && (bd == 1 || bd == 2 || bd == 4 || bd == 8 || bd == 16)) || (ct == 3 && (bd == 1 || bd == 2 || bd == 4 || bd == 8)) ||
                               ((ct == 2 || ct == 4 || ct == 6) && (bd == 8 || bd == 16));
            if (!legal) return "illegal colour type / bit depth pair";
            if (bd < 8) return "sub-byte bit depth " + std::to_string(bd) + " is not supported";
            if (role == ROLE_COLOR) {
                if (bd == 16) return "16-bit colour is not supported";
                if (ct == 4) return "grey + alpha colour images are not supported";
            } else if (role == ROLE_DEPTH) {
                if (ct != 0 || bd != 16) return "a depth PNG must be 16-bit grey (colour type " + std::to_string(ct) + ", " + std::to_string(bd) + " bits)";
            } else {
                if (ct != 0) return "colour masks are not supported: a mask PNG must be 8-bit grey";
                if (bd != 8) return "a mask PNG must be 8-bit grey (" + std::to_string(bd) + " bits)";
            }
            const int channels = ct == 2 ? 3 : (ct == 6 ? 4 : 1);
            pi.bpp = channels * bd / 8;
            want = pngScanBytes(pi.width, pi.height, pi.bpp);
            if (want > cap) return "the image (" + std::to_string(pi.width) + " x " + std::to_string(pi.height) + ") does not fit the buffer";
            if (!inf.begin(scan, want)) return "zlib: inflateInit failed";
        } else if (name == "PLTE") {
            if (havePalette || sawData) return "misplaced PLTE";
            if (len == 0 || len % 3 != 0 || len > 768) return "malformed PLTE";
            havePalette = true;
            pi.paletteEntries = (int)(len / 3);
            if (pi.colorType == 3) {
                if (!palette) return "no room for a palette";
                memset(palette, 0, 768);
                memcpy(palette, body, len);
            }
        } else if (name == "IDAT") {
            if (pi.colorType == 3 && !havePalette) return "palette image without PLTE";
            sawData = true;
            if (len == 0) continue;
            if (streamEnd) return "data after the end of the zlib stream";
            std::string why;
            const int rc = inf.feed(body, len, &why);
            if (rc < 0) return why;
            if (rc == 1) {
                streamEnd = true;
                if (inf.z.avail_in > 0) return "data after the end of the zlib stream";
            }
        } else if (name == "IEND") {
            ended = true;
        } else if (critical) {
            return "unknown critical chunk '" + name + "'";
        }
    }
    if (!sawData) return "no IDAT chunk";
    if (!streamEnd) return "truncated: the zlib stream does not end";
    if (inf.z.total_out != want) return "the zlib stream holds " + std::to_string(inf.z.total_out) + " bytes, " + std::to_string(want) + " expected";
    const double t1 = now();
    // unfilter in place, row by row: left = bpp bytes back, up = the row above (zeros above the first)
    const size_t rb = (size_t)pi.bpp * pi.width, stride = rb + 1;
    const int bpp = pi.bpp;
    for (int y = 0; y < pi.height; y++) {
        uint8_t* cur = scan + (size_t)y * stride + 1;
        const uint8_t* up = y ? cur - stride : nullptr;
        const int f = cur[-1];
        switch (f) {
        case 0: break;
        case 1: for (size_t i = bpp; i < rb; i++) cur[i] = (uint8_t)(cur[i] + cur[i - bpp]); break;
        case 2: if (up) for (size_t i = 0; i < rb; i++) cur[i] = (uint8_t)(cur[i] + up[i]); break;
        case 3:
            for (size_t i = 0; i < rb; i++) {
                const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0;
                cur[i] = (uint8_t)(cur[i] + ((a + b) >> 1));
            }
            break;
        case 4:
            for (size_t i = 0; i < rb; i++) {
                const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= (size_t)bpp) ? up[i - bpp] : 0;
                cur[i] = (uint8_t)(cur[i] + paeth(a, b, c));
            }
            break;
        default: return "row " + std::to_string(y) + " has unknown filter type " + std::to_string(f);
        }
    }
    const double tu = now();
    if (pi.colorType == 3) {   // an index beyond the palette is an error of the file (the device would read past the entries)
        for (int y = 0; y < pi.height; y++) {
            const uint8_t* cur = scan + (size_t)y * stride + 1;
            for (int x = 0; x < pi.width; x++)
                if (cur[x] >= pi.paletteEntries) return "palette index " + std::to_string(cur[x]) + " beyond the " + std::to_string(pi.paletteEntries) + " entries of PLTE";
        }
    }
    if (times) {
        const double t2 = now();
        times->inflate += inf.seconds; times->unfilter += tu - t1; times->parse += (t1 - t0 - inf.seconds) + (t2 - tu);
    }
    *info = pi;
    return "";
}

std::string exrDecode(const uint8_t* data, size_t n, ExrInfo* info, uint8_t* raw, size_t cap, cf_exr_block* blocks, size_t maxBlocks, DecodeTimes* times)
{
    if (n < 8 || le32(data) != 20000630u) return "not an OpenEXR file (magic)";
    const uint32_t version = le32(data + 4);
    if ((version & 0xff) != 2) return "OpenEXR version " + std::to_string(version & 0xff) + " is not supported";
    if (version & 0x200) return "tiled OpenEXR files are not supported";
    if (version & 0x800) return "deep OpenEXR files are not supported";
    if (version & 0x1000) return "multipart OpenEXR files are not supported";
    if (version & ~(uint32_t)0x4ff) return "unknown OpenEXR version flags";
    size_t pos = 8;
    auto cstr = [&](std::string* s) {
        const size_t start = pos;
        while (pos < n && data[pos] != 0) pos++;
        if (pos >= n || pos - start > 255) return false;
        s->assign(reinterpret_cast<const char*>(data + start), pos - start);
        pos++;
        return true;
    };
    struct Chan { std::string name; int type; };
    std::vector<Chan> chans;
    int compression = -1, lineOrder = -1;
    int32_t dw[4] = {0, 0, -1, -1}, disp[4] = {0, 0, -1, -1};
    bool haveDw = false, haveDisp = false, haveCh = false;
    for (;;) {
        std::string name, type;
        if (!cstr(&name)) return "truncated header";
        if (name.empty()) break;
        if (!cstr(&type) || n - pos < 4) return "truncated header";
        const uint32_t size = le32(data + pos);
        pos += 4;
        if (size > n - pos) return "truncated header: attribute '" + name + "' runs past the end of the file";
        const uint8_t* v = data + pos;
        const size_t end = pos + size;
        if (name == "channels") {
            if (type != "chlist") return "attribute 'channels' is not a chlist";
            haveCh = true;
            size_t p = pos;
            for (;;) {
                if (p >= end) return "malformed channel list";
                if (data[p] == 0) break;
                const size_t s0 = p;
                while (p < end && data[p] != 0) p++;
                if (p >= end || end - (p + 1) < 16) return "malformed channel list";
                Chan c;
                c.name.assign(reinterpret_cast<const char*>(data + s0), p - s0);
                p++;
                c.type = (int)le32(data + p);
                const uint32_t xs = le32(data + p + 8), ys = le32(data + p + 12);
                p += 16;
                if (c.type == 0) return "channel '" + c.name + "' is UINT: only HALF and FLOAT are supported";
                if (c.type != 1 && c.type != 2) return "channel '" + c.name + "' has an unknown pixel type";
                if (xs != 1 || ys != 1) return "channel '" + c.name + "' is subsampled";
                chans.push_back(c);
                if (chans.size() > 4) return "more than four channels";
            }
        } else if (name == "compression") {
            if (size != 1) return "malformed attribute 'compression'";
            compression = v[0];
        } else if (name == "lineOrder") {
            if (size != 1) return "malformed attribute 'lineOrder'";
            lineOrder = v[0];
        } else if (name == "dataWindow" || name == "displayWindow") {
            if (size != 16) return "malformed attribute '" + name + "'";
            int32_t* b = name == "dataWindow" ? dw : disp;
            for (int k = 0; k < 4; k++) b[k] = (int32_t)le32(v + 4 * k);
            (name == "dataWindow" ? haveDw : haveDisp) = true;
        } else if (name == "tiles") {
            return "tiled OpenEXR files are not supported";
        }
        pos = end;
    }
    if (!haveCh || chans.empty() || compression < 0 || lineOrder < 0 || !haveDw || !haveDisp) return "a required header attribute is missing";
    static const char* cnames[] = {"NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};
    if (compression != 0 && compression != 2 && compression != 3)
        return std::string("compression ") + (compression < 10 ? cnames[compression] : std::to_string(compression).c_str()) + " is not supported (NONE, ZIPS, ZIP)";
    if (lineOrder != 0) return "line order " + std::to_string(lineOrder) + " is not supported (INCREASING_Y)";
    if (memcmp(dw, disp, sizeof(dw)) != 0) return "the dataWindow differs from the frame (displayWindow)";
    const int64_t w64 = (int64_t)dw[2] - dw[0] + 1, h64 = (int64_t)dw[3] - dw[1] + 1;
    if (w64 < 1 || h64 < 1 || w64 > kMaxSide || h64 > kMaxSide) return "image size outside 1..16384";
    ExrInfo ei;
    ei.width = (int)w64; ei.height = (int)h64; ei.compression = compression;
    ei.linesPerBlock = compression == 3 ? 16 : 1;
    ei.blocks = (ei.height + ei.linesPerBlock - 1) / ei.linesPerBlock;
    // the depth channel: the only one, or B of a file that has B, G and R (OpenCV hands the reference B first)
    int pick = -1;
    if (chans.size() == 1) pick = 0;
    else {
        bool b = false, g = false, r = false;
        for (size_t c = 0; c < chans.size(); c++) {
            b |= chans[c].name == "B"; g |= chans[c].name == "G"; r |= chans[c].name == "R";
            if (chans[c].name == "B") pick = (int)c;
        }
        if (!(b && g && r)) {
            std::string names;
            for (auto& c : chans) names += (names.empty() ? "" : ", ") + c.name;
            return "no depth channel can be chosen among the channels " + names;
        }
    }
    int off = 0;
    for (size_t c = 0; c < chans.size(); c++) {
        if ((int)c == pick) ei.chanOffset = off;
        off += ei.width * (chans[c].type == 1 ? 2 : 4);
    }
    ei.lineBytes = off;
    ei.chanHalf = chans[pick].type == 1;
    ei.channel = chans[pick].name;
    if ((size_t)ei.lineBytes * ei.height > cap || (size_t)ei.blocks > maxBlocks) return "the image (" + std::to_string(ei.width) + " x " + std::to_string(ei.height) + ") does not fit the buffer";
    if (n - pos < (size_t)ei.blocks * 8) return "truncated: the offset table runs past the end of the file";
    const uint8_t* table = data + pos;
    const double t0 = now();
    double inflating = 0;
    for (int i = 0; i < ei.blocks; i++) {
        const uint64_t o = le64(table + 8 * (size_t)i);
        if (o > n || n - o < 8) return "offset table entry " + std::to_string(i) + " points outside the file";
        const int32_t y = (int32_t)le32(data + o);
        const uint32_t size = le32(data + o + 4);
        if (size > n - o - 8) return "truncated: block " + std::to_string(i) + " runs past the end of the file";
        const int first = i * ei.linesPerBlock, lines = std::min(ei.linesPerBlock, ei.height - first);
        if ((int64_t)y != (int64_t)dw[1] + first) return "block " + std::to_string(i) + " starts at line " + std::to_string(y) + ", not where INCREASING_Y puts it";
        const size_t bytes = (size_t)lines * ei.lineBytes;
        uint8_t* dst = raw + (size_t)first * ei.lineBytes;
        cf_exr_block b;
        b.offset = (uint32_t)((size_t)first * ei.lineBytes); b.bytes = (uint32_t)bytes; b.first_line = (uint32_t)first;
        if (size == bytes) {   // NONE, or a block deflate did not shrink: the pixels as they are
            memcpy(dst, data + o + 8, bytes);
            b.stored_raw = 1;
        } else if (compression == 0 || size > bytes) {
            return "block " + std::to_string(i) + " holds " + std::to_string(size) + " bytes, " + std::to_string(bytes) + " expected";
        } else {
            Inflater inf;
            if (!inf.begin(dst, bytes)) return "zlib: inflateInit failed";
            std::string why;
            const int rc = inf.feed(data + o + 8, size, &why);
            if (rc < 0) return "block " + std::to_string(i) + ": " + why;
            inflating += inf.seconds;
            if (rc != 1 || inf.z.total_out != bytes) return "block " + std::to_string(i) + ": the zlib stream does not fill the block";
            b.stored_raw = 0;
        }
        blocks[i] = b;
    }
    if (times) { times->inflate += inflating; times->parse += now() - t0 - inflating; }
    *info = ei;
    return "";
}

std::string ppmDecode(const uint8_t* data, size_t n, int* width, int* height, const uint8_t** pixels)
{
    size_t pos = 0;
    const std::string e = pnmHeader(data, n, "P6", "PPM", width, height, &pos);
    if (!e.empty()) return e;
    const size_t want = (size_t)*width * *height * 3;
    if (n - pos < want) return "PPM: " + std::to_string(n - pos) + " bytes of pixels, " + std::to_string(want) + " expected";
    *pixels = data + pos;
    return "";
}

std::string pgmDecode(const uint8_t* data, size_t n, int* width, int* height, const uint8_t** pixels)
{
    size_t pos = 0;
    const std::string e = pnmHeader(data, n, "P5", "PGM", width, height, &pos);
    if (!e.empty()) return e;
    const size_t want = (size_t)*width * *height;
    if (n - pos < want) return "PGM: " + std::to_string(n - pos) + " bytes of pixels, " + std::to_string(want) + " expected";
    *pixels = data + pos;
    return "";
}

void pngColorFinishHost(const PngInfo& info, const uint8_t* scan, const uint8_t* palette, bool flip, uint8_t* rgba)
{
    const size_t stride = (size_t)info.bpp * info.width + 1;
    for (int y = 0; y < info.height; y++) {
        const uint8_t* row = scan + (size_t)y * stride + 1;
        uint8_t* out = rgba + (size_t)y * info.width * 4;
        for (int x = 0; x < info.width; x++) {
            uint8_t r, g, b;
            switch (info.colorType) {
            case 0: r = g = b = row[x]; break;
            case 3: { const uint8_t* p = palette + 3 * (size_t)row[x]; r = p[0]; g = p[1]; b = p[2]; break; }
            default: { const uint8_t* p = row + (size_t)x * info.bpp; r = p[0]; g = p[1]; b = p[2]; break; }
            }
            out[4 * x + 0] = flip ? b : r; out[4 * x + 1] = g; out[4 * x + 2] = flip ? r : b; out[4 * x + 3] = 255;
        }
    }
}

void pngDepthFinishHost(const PngInfo& info, const uint8_t* scan, float depthScale, float* depth)
{
    const size_t stride = (size_t)2 * info.width + 1;
    for (int y = 0; y < info.height; y++) {
        const uint8_t* row = scan + (size_t)y * stride + 1;
        for (int x = 0; x < info.width; x++) depth[(size_t)y * info.width + x] = (float)(row[2 * x] << 8 | row[2 * x + 1]) * depthScale;
    }
}

void pngMaskFinishHost(const PngInfo& info, const uint8_t* scan, uint8_t* mask)
{
    const size_t stride = (size_t)info.width + 1;
    for (int y = 0; y < info.height; y++) memcpy(mask + (size_t)y * info.width, scan + (size_t)y * stride + 1, info.width);
}

void exrFinishHost(const ExrInfo& info, const uint8_t* raw, const cf_exr_block* blocks, float* depth)
{
    std::vector<uint8_t> tmp, pix;
    for (int i = 0; i < info.blocks; i++) {
        const cf_exr_block& b = blocks[i];
        const uint8_t* src = raw + b.offset;
        if (!b.stored_raw) {
            tmp.assign(src, src + b.bytes);
            for (size_t k = 1; k < tmp.size(); k++) tmp[k] = (uint8_t)(tmp[k - 1] + tmp[k] - 128);
            pix.resize(b.bytes);
            const size_t half = ((size_t)b.bytes + 1) / 2;
            for (size_t k = 0; k < b.bytes; k++) pix[k] = (k & 1) ? tmp[half + k / 2] : tmp[k / 2];
            src = pix.data();
        }
        const int lines = (int)(b.bytes / (uint32_t)info.lineBytes);
        for (int l = 0; l < lines; l++) {
            const uint8_t* run = src + (size_t)l * info.lineBytes + info.chanOffset;
            float* out = depth + ((size_t)b.first_line + l) * info.width;
            for (int x = 0; x < info.width; x++) {
                if (info.chanHalf) out[x] = halfToFloat((uint16_t)(run[2 * x] | run[2 * x + 1] << 8));
                else { const uint32_t u = le32(run + 4 * (size_t)x); memcpy(&out[x], &u, 4); }
            }
        }
    }
}

std::string readFile(const std::string& path, std::vector<uint8_t>* out)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return "cannot open the file";
    std::string e;
    if (fseek(f, 0, SEEK_END) != 0) e = "cannot seek";
    const long size = e.empty() ? ftell(f) : -1;
    if (e.empty() && (size < 0 || size > (1l << 30))) e = "file size outside 0..1 GiB";
    if (e.empty()) {
        rewind(f);
        out->resize((size_t)size);
        if (size > 0 && fread(out->data(), 1, (size_t)size, f) != (size_t)size) e = "short read";
    }
    fclose(f);
    return e;
}

// ---- directory logic ----
namespace {

std::string withSlash(const std::string& d) { return (d.empty() || d.back() == '/') ? d : d + "/"; }

bool isFile(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

// regular files whose stem starts with the prefix and whose lower-cased extension is one of `exts`; they must share one extension
std::string countFiles(const std::string& dir, const std::string& prefix, const std::vector<std::string>& exts, int* count, std::string* ext)
{
    *count = 0;
    ext->clear();
    DIR* d = opendir(dir.c_str());
    if (!d) return "cannot open the directory " + dir;
    std::string e;
    while (struct dirent* de = readdir(d)) {
        const std::string name = de->d_name;
        if (!isFile(dir + name)) continue;
        const size_t dot = name.rfind('.');
        if (dot == std::string::npos || dot == 0) continue;
        const std::string stem = name.substr(0, dot);
        std::string x = name.substr(dot);
        std::transform(x.begin(), x.end(), x.begin(), [](unsigned char c) { return (char)tolower(c); });
        if (stem.compare(0, prefix.size(), prefix) != 0 || std::find(exts.begin(), exts.end(), x) == exts.end()) continue;
        if (ext->empty()) *ext = x;
        else if (*ext != x) { e = "the files of the dataset (" + dir + ", " + prefix + ") must have the same extension"; break; }
        (*count)++;
    }
    closedir(d);
    return e;
}

bool jpegSize(const uint8_t* p, size_t n, int* w, int* h)
{
    size_t pos = 2;
    if (n < 4 || p[0] != 0xff || p[1] != 0xd8) return false;
    while (pos + 4 <= n) {
        if (p[pos] != 0xff) return false;
        const int m = p[pos + 1];
        if (m == 0xff) { pos++; continue; }
        const size_t len = (size_t)p[pos + 2] << 8 | p[pos + 3];
        if (m >= 0xc0 && m <= 0xc2) {
            if (pos + 9 > n) return false;
            *h = p[pos + 5] << 8 | p[pos + 6]; *w = p[pos + 7] << 8 | p[pos + 8];
            return *w > 0 && *h > 0;
        }
        if (len < 2) return false;
        pos += 2 + len;
    }
    return false;
}

}  // namespace

std::string SequenceLayout::path(Role role, int frame) const
{
    char num[32];
    snprintf(num, sizeof(num), "%0*d", opt.indexWidth, frame + startIndex);
    if (role == ROLE_COLOR) return opt.colorDir + opt.colorPrefix + num + colorExt;
    if (role == ROLE_DEPTH) return opt.depthDir + opt.depthPrefix + num + depthExt;
    return opt.maskDir + opt.maskPrefix + num + maskExt;
}

int64_t SequenceLayout::timestamp(int frame) const
{
    const float t = (float)(size_t)frame * 1000.0f / opt.rateHz;   // ImageLogReader.cpp:275, in f32
    return (int64_t)t;
}

std::string scanSequence(const SequenceOptions& in, SequenceLayout* out)
{
    SequenceLayout L;
    L.opt = in;
    SequenceOptions& o = L.opt;
    if (o.colorDir.empty()) return "no colour directory";
    if (o.indexWidth < 1 || o.indexWidth > 12) return "index width outside 1..12";
    if (!(o.rateHz > 0)) return "the frame rate must be positive";
    o.colorDir = withSlash(o.colorDir);
    o.depthDir = o.depthDir.empty() ? o.colorDir : withSlash(o.depthDir);
    o.maskDir = o.maskDir.empty() ? o.colorDir : withSlash(o.maskDir);
    // overlapping directories without distinct prefixes: the default prefixes
    if ((o.depthDir == o.colorDir || o.maskDir == o.colorDir || o.maskDir == o.depthDir) &&
        (o.depthPrefix == o.colorPrefix && o.maskPrefix == o.colorPrefix)) {
        o.colorPrefix = "Color"; o.depthPrefix = "Depth"; o.maskPrefix = "Mask";
    }
    int nc = 0, nd = 0, nm = 0;
    std::string e;
    if (!(e = countFiles(o.colorDir, o.colorPrefix, {".jpg", ".png", ".ppm"}, &nc, &L.colorExt)).empty()) return e;
    if (!(e = countFiles(o.depthDir, o.depthPrefix, {".exr", ".png"}, &nd, &L.depthExt)).empty()) return e;
    if (!(e = countFiles(o.maskDir, o.maskPrefix, {".png", ".pgm"}, &nm, &L.maskExt)).empty()) return e;
    if (nc == 0) return "no colour frames (" + o.colorPrefix + "*.jpg/.png/.ppm) in " + o.colorDir;
    if (nm > 0) { L.hasMasks = true; L.maxMasks = (o.maxMasks > 0 && o.maxMasks < nm) ? o.maxMasks : nm; }
    if (nc != nd) return "number of colour frames (" + std::to_string(nc) + ") != depth frames (" + std::to_string(nd) + ")";
    if (L.hasMasks && nc != nm) return "number of colour frames (" + std::to_string(nc) + ") != mask frames (" + std::to_string(nm) + ")";
    L.numFrames = nc;
    if (o.startIndex >= 0) L.startIndex = o.startIndex;
    else {
        int index = 0;
        for (; index < 2; index++) {
            L.startIndex = index;
            if (isFile(L.path(ROLE_COLOR, 0))) break;
        }
        if (index == 2) return "could not find the start index (no " + o.colorPrefix + "<0 or 1>" + L.colorExt + " in " + o.colorDir + ")";
    }
    *out = L;
    return "";
}

ImageSequenceReader::ImageSequenceReader(const SequenceOptions& opt)
{
    err = scanSequence(opt, &lay);
    if (!err.empty()) return;
    // the frame size is the first colour frame's
    const std::string p = lay.path(ROLE_COLOR, 0);
    std::string e = readFile(p, &file);
    if (e.empty()) {
        if (lay.colorExt == ".png") {
            if (file.size() >= 24 && be32(file.data() + 12) == 0x49484452u) { w = (int)be32(file.data() + 16); h = (int)be32(file.data() + 20); }
            else e = "not a PNG file";
        } else if (lay.colorExt == ".ppm") {
            const uint8_t* px;
            e = ppmDecode(file.data(), file.size(), &w, &h, &px);
        } else if (!jpegSize(file.data(), file.size(), &w, &h)) e = "no frame header in the JPEG stream";
        if (e.empty() && (w < 1 || h < 1 || w > kMaxSide || h > kMaxSide)) e = "image size outside 1..16384";
    }
    if (!e.empty()) { err = p + ": " + e; return; }
    scan.resize((size_t)16 * w * h + h + 16);
    rgba.resize((size_t)4 * w * h);
    blocks.resize(h);
}

bool ImageSequenceReader::next(int64_t* timestamp, float* depth, uint8_t* rgb, uint8_t* mask, int* hasMask)
{
    if (w == 0) return false;   // the constructor failed: error() says why
    if (current >= lay.numFrames) { err = "no more frames"; return false; }
    const int i = current;
    const size_t N = (size_t)w * h;
    auto fail = [&](const std::string& p, const std::string& why) { err = p + ": " + why; return false; };
    auto load = [&](const std::string& p) {
        const double t0 = now();
        const std::string e = readFile(p, &file);
        times.read += now() - t0;
        return e;
    };
    std::string e;
    // colour
    std::string p = lay.path(ROLE_COLOR, i);
    if (!(e = load(p)).empty()) return fail(p, e);
    if (lay.colorExt == ".png") {
        PngInfo pi;
        uint8_t pal[768];
        if (!(e = pngDecode(file.data(), file.size(), ROLE_COLOR, &pi, scan.data(), scan.size(), pal, &times)).empty()) return fail(p, e);
        if (pi.width != w || pi.height != h) return fail(p, "the frame is not " + std::to_string(w) + " x " + std::to_string(h));
        pngColorFinishHost(pi, scan.data(), pal, lay.opt.flipColors, rgba.data());
        for (size_t k = 0; k < N; k++) { rgb[3 * k] = rgba[4 * k]; rgb[3 * k + 1] = rgba[4 * k + 1]; rgb[3 * k + 2] = rgba[4 * k + 2]; }
    } else {
        if (lay.colorExt == ".ppm") {
            int pw, ph;
            const uint8_t* px;
            if (!(e = ppmDecode(file.data(), file.size(), &pw, &ph, &px)).empty()) return fail(p, e);
            if (pw != w || ph != h) return fail(p, "the frame is not " + std::to_string(w) + " x " + std::to_string(h));
            memcpy(rgb, px, N * 3);
        } else if (!(e = decodeJpegRGB(file.data(), file.size(), w, h, rgb)).empty()) return fail(p, e);
        if (lay.opt.flipColors) for (size_t k = 0; k < N; k++) std::swap(rgb[3 * k], rgb[3 * k + 2]);
    }
    // depth
    p = lay.path(ROLE_DEPTH, i);
    if (!(e = load(p)).empty()) return fail(p, e);
    if (lay.depthExt == ".png") {
        PngInfo pi;
        if (!(e = pngDecode(file.data(), file.size(), ROLE_DEPTH, &pi, scan.data(), scan.size(), nullptr, &times)).empty()) return fail(p, e);
        if (pi.width != w || pi.height != h) return fail(p, "the frame is not " + std::to_string(w) + " x " + std::to_string(h));
        pngDepthFinishHost(pi, scan.data(), lay.opt.depthScale, depth);
    } else {
        ExrInfo ei;
        if (!(e = exrDecode(file.data(), file.size(), &ei, scan.data(), (size_t)16 * w * h, blocks.data(), blocks.size(), &times)).empty()) return fail(p, e);
        if (ei.width != w || ei.height != h) return fail(p, "the frame is not " + std::to_string(w) + " x " + std::to_string(h));
        exrFinishHost(ei, scan.data(), blocks.data(), depth);
    }
    // mask
    int got = 0;
    if (lay.hasMasks && i < lay.maxMasks) {
        p = lay.path(ROLE_MASK, i);
        if (!(e = load(p)).empty()) return fail(p, e);
        if (lay.maskExt == ".png") {
            PngInfo pi;
            if (!(e = pngDecode(file.data(), file.size(), ROLE_MASK, &pi, scan.data(), scan.size(), nullptr, &times)).empty()) return fail(p, e);
            if (pi.width != w || pi.height != h) return fail(p, "the mask is not " + std::to_string(w) + " x " + std::to_string(h));
            if (mask) pngMaskFinishHost(pi, scan.data(), mask);
        } else {
            int pw, ph;
            const uint8_t* px;
            if (!(e = pgmDecode(file.data(), file.size(), &pw, &ph, &px)).empty()) return fail(p, e);
            if (pw != w || ph != h) return fail(p, "the mask is not " + std::to_string(w) + " x " + std::to_string(h));
            if (mask) memcpy(mask, px, N);
        }
        got = 1;
    }
    if (hasMask) *hasMask = got;
    if (timestamp) *timestamp = lay.timestamp(i);
    err.clear();
    current++;
    return true;
}

}  // namespace imageio
}  // namespace cofusion
