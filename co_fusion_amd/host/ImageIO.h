// ImageIO.h -- image-sequence datasets: the files the reference's GUI/Tools/ImageLogReader.cpp reads through
// OpenCV (colour .jpg/.png/.ppm, depth .exr/.png, masks .png/.pgm), parsed here with zlib alone.
//   pngDecode   non-interlaced PNG -> UNFILTERED SCANLINES IN FILE LAYOUT (row stride 1 + bpp * width: the filter byte stays, 16-bit
//               samples stay big-endian) in memory the caller hands in; CRC of the critical chunks and the zlib Adler are checked
//   exrDecode   single-part scanline OpenEXR (NONE / ZIPS / ZIP, HALF / FLOAT) -> the inflated blocks at their place in the frame plus
//               a table (cf_exr_block); predictor and interleave are NOT undone here (a block stored raw has neither)
//   ppmDecode / pgmDecode   binary P6 / P5, maxval <= 255
// The conversion to RGBA8 / f32 depth / u8 mask is the device's (csrc/image_decode.hip); pngFinishHost / exrFinishHost state the same
// on the host for the serial reader (ImageSequenceReader), the yardstick of the device path.  Every refusal is a std::string that
// says why; callers put the file's name in front.  No GPU calls in this file.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cofusion_hip.h"

namespace cofusion {
namespace imageio {

enum Role { ROLE_COLOR = 0, ROLE_DEPTH = 1, ROLE_MASK = 2 };

struct PngInfo {
    int width = 0, height = 0, bitDepth = 0, colorType = 0;
    int bpp = 0;              // bytes per pixel: the row stride is 1 + bpp * width
    int paletteEntries = 0;   // colour type 3
};
// seconds, accumulated.  inflate: the calls of zlib's inflate() alone; unfilter: the PNG filter loop; parse: what is left of a decode
// (chunk walk, CRC-32 of the chunks, header parsing, copies of EXR blocks stored raw, the palette index check)
struct DecodeTimes { double read = 0, inflate = 0, unfilter = 0, parse = 0; };

inline size_t pngScanBytes(int width, int height, int bpp) { return ((size_t)1 + (size_t)bpp * width) * height; }

// "" or the reason.  palette: 768 bytes (colour type 3), may be null for the other roles.
std::string pngDecode(const uint8_t* data, size_t n, Role role, PngInfo* info, uint8_t* scan, size_t cap, uint8_t* palette,
                      DecodeTimes* times = nullptr);

struct ExrInfo {
    int width = 0, height = 0, compression = 0, linesPerBlock = 1, blocks = 0;
    int lineBytes = 0;      // all channels of one scanline
    int chanOffset = 0;     // where the chosen channel's run of `width` samples starts inside a scanline
    int chanHalf = 0;       // 1: HALF, 0: FLOAT
    std::string channel;    // its name
};
// blocks: room for `height` entries (ZIPS has one block per line); raw: room for lineBytes * height
std::string exrDecode(const uint8_t* data, size_t n, ExrInfo* info, uint8_t* raw, size_t cap, cf_exr_block* blocks, size_t maxBlocks,
                      DecodeTimes* times = nullptr);

std::string ppmDecode(const uint8_t* data, size_t n, int* width, int* height, const uint8_t** pixels);   // P6: 3 B/px inside `data`
std::string pgmDecode(const uint8_t* data, size_t n, int* width, int* height, const uint8_t** pixels);   // P5: 1 B/px inside `data`

// ---- the device's kernels restated on the host ----
void pngColorFinishHost(const PngInfo& info, const uint8_t* scan, const uint8_t* palette, bool flip, uint8_t* rgba);
void pngDepthFinishHost(const PngInfo& info, const uint8_t* scan, float depthScale, float* depth);
void pngMaskFinishHost(const PngInfo& info, const uint8_t* scan, uint8_t* mask);
void exrFinishHost(const ExrInfo& info, const uint8_t* raw, const cf_exr_block* blocks, float* depth);
float halfToFloat(uint16_t h);

std::string readFile(const std::string& path, std::vector<uint8_t>* out);

// ---- the dataset's layout on disk (ImageLogReader's constructor) ----
struct SequenceOptions {
    std::string colorDir, depthDir, maskDir;       // depthDir / maskDir empty: the colour directory
    std::string colorPrefix, depthPrefix, maskPrefix;
    int indexWidth = 4;
    int startIndex = -1;          // -1: the first of 0, 1 for which a colour file exists (the reference's rule)
    bool flipColors = false;      // the reference's reader hands on the file's R, G, B whatever its flag says; true reverses them
    float depthScale = 0.0006f;   // 16-bit PNG depth: metres = f32(u16) * depthScale, one f32 product
    float rateHz = 24.0f;
    int maxMasks = 0;             // > 0: masks are read for the first so many frames only (0: for as many frames as there are masks)
};
struct SequenceLayout {
    SequenceOptions opt;
    std::string colorExt, depthExt, maskExt;
    int numFrames = 0, startIndex = 0;
    bool hasMasks = false;
    int maxMasks = 0;             // masks are read for frames < maxMasks
    std::string path(Role role, int frame) const;
    int64_t timestamp(int frame) const;   // int64(f32(frame) * 1000.0f / rateHz)
};
std::string scanSequence(const SequenceOptions& opt, SequenceLayout* out);

// The serial reader: everything on the calling thread, host buffers shaped like the reference's FrameData.
class ImageSequenceReader {
  public:
    explicit ImageSequenceReader(const SequenceOptions& opt);
    bool ok() const { return err.empty(); }
    const std::string& error() const { return err; }
    const SequenceLayout& layout() const { return lay; }
    int getNumFrames() const { return lay.numFrames; }
    int width() const { return w; }
    int height() const { return h; }
    bool hasMore() const { return current < lay.numFrames; }
    void rewind() { current = 0; }
    // depth f32 [h*w], rgb u8 [h*w*3], mask u8 [h*w] (may be null); *hasMask 0 where the frame has none.  false: error() says why
    // and names the file; the reader stays at that frame.
    bool next(int64_t* timestamp, float* depth, uint8_t* rgb, uint8_t* mask, int* hasMask);
    DecodeTimes times;

  private:
    SequenceLayout lay;
    std::string err;
    int w = 0, h = 0, current = 0;
    std::vector<uint8_t> file, scan, rgba;
    std::vector<cf_exr_block> blocks;
};

}  // namespace imageio
}  // namespace cofusion
