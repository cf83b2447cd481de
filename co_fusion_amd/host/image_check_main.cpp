// image_check_main.cpp -- a stand-alone checker of the image parsers (host/ImageIO.cpp) for a sanitizer build: `make image_check`
// compiles it with -fsanitize=address,undefined.  It runs pngDecode (all three roles) / exrDecode / ppmDecode / pgmDecode and, where
// they accept, the *FinishHost routines over every .png / .exr / .ppm / .pgm file of the directories given, over prefix truncations
// of each file (EVERY prefix, whatever the file's size) and over a fixed table of byte corruptions.  A parser
// may accept or refuse; it must never read or write outside its buffers.  Exit status 0 and a line of counts when all ran through.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ImageIO.h"

namespace cofusion {   // ImageIO.cpp's serial reader refers to the JPEG decoder; this program reads no JPEG
std::string decodeJpegRGB(const uint8_t*, size_t, int, int, uint8_t*) { return "no JPEG decoder in this program"; }
}

using namespace cofusion::imageio;

namespace {

long accepted = 0, refused = 0;

// exactly-sized heap blocks, so that the sanitizer sees an access one byte past what a parser was promised
void parse(const std::string& ext, const uint8_t* p, size_t n)
{
    std::vector<uint8_t> data(p, p + n);   // a copy of exactly n bytes
    if (ext == ".png") {
        int w = 1, h = 1;
        if (n >= 24) {
            const uint32_t W = (uint32_t)p[16] << 24 | p[17] << 16 | p[18] << 8 | p[19], H = (uint32_t)p[20] << 24 | p[21] << 16 | p[22] << 8 | p[23];
            if (W >= 1 && W <= 256 && H >= 1 && H <= 256) { w = (int)W; h = (int)H; }
        }
        for (int role = 0; role < 3; role++) {
            const int bpp = role == ROLE_COLOR ? 4 : (role == ROLE_DEPTH ? 2 : 1);
            std::vector<uint8_t> scan(pngScanBytes(w, h, bpp)), palette(768);
            PngInfo info;
            const std::string e = pngDecode(data.data(), n, (Role)role, &info, scan.data(), scan.size(), palette.data());
            if (!e.empty()) { refused++; continue; }
            accepted++;
            const size_t N = (size_t)info.width * info.height;
            if (role == ROLE_COLOR) { std::vector<uint8_t> out(N * 4); pngColorFinishHost(info, scan.data(), palette.data(), true, out.data()); }
            else if (role == ROLE_DEPTH) { std::vector<float> out(N); pngDepthFinishHost(info, scan.data(), 0.001f, out.data()); }
            else { std::vector<uint8_t> out(N); pngMaskFinishHost(info, scan.data(), out.data()); }
        }
    } else if (ext == ".exr") {
        const size_t cap = 1 << 16, maxBlocks = 64;   // the fixtures' frames fit; a corrupted header that asks for more is refused
        std::vector<uint8_t> raw(cap);
        std::vector<cf_exr_block> blocks(maxBlocks);
        ExrInfo info;
        const std::string e = exrDecode(data.data(), n, &info, raw.data(), cap, blocks.data(), maxBlocks);
        if (!e.empty()) { refused++; return; }
        accepted++;
        std::vector<float> out((size_t)info.width * info.height);
        exrFinishHost(info, raw.data(), blocks.data(), out.data());
    } else {
        int w, h;
        const uint8_t* px;
        const std::string e = ext == ".ppm" ? ppmDecode(data.data(), n, &w, &h, &px) : pgmDecode(data.data(), n, &w, &h, &px);
        if (!e.empty()) { refused++; return; }
        accepted++;
        volatile uint8_t last = px[(size_t)w * h * (ext == ".ppm" ? 3 : 1) - 1];   // the last pixel lies inside the file
        (void)last;
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: image_check DIRECTORY...\n"); return 2; }
    static const uint8_t masks[] = {0x01, 0x80, 0xff};
    long files = 0;
    for (int a = 1; a < argc; a++) {
        const std::string dir = std::string(argv[a]) + "/";
        DIR* d = opendir(dir.c_str());
        if (!d) { fprintf(stderr, "cannot open %s\n", dir.c_str()); return 2; }
        std::vector<std::string> names;
        while (struct dirent* de = readdir(d)) names.push_back(de->d_name);
        closedir(d);
        std::sort(names.begin(), names.end());
        for (const std::string& name : names) {
            const size_t dot = name.rfind('.');
            const std::string ext = dot == std::string::npos ? "" : name.substr(dot);
            if (ext != ".png" && ext != ".exr" && ext != ".ppm" && ext != ".pgm") continue;
            std::vector<uint8_t> file;
            if (!readFile(dir + name, &file).empty()) { fprintf(stderr, "cannot read %s\n", name.c_str()); return 2; }
            const size_t n = file.size();
            files++;
            const long before = accepted;
            parse(ext, file.data(), n);
            if (accepted == before) { fprintf(stderr, "%s: the intact file was refused\n", name.c_str()); return 1; }
            for (size_t cut = 0; cut < n; cut++) parse(ext, file.data(), cut);
            // corruptions: every byte of the first 64 (signatures, headers, the first chunk), then 61 places spread over the file
            std::vector<size_t> places;
            for (size_t i = 0; i < 64 && i < n; i++) places.push_back(i);
            for (size_t k = 1; k <= 61; k++) places.push_back((n - 1) * k / 61);
            for (size_t at : places)
                for (uint8_t m : masks) {
                    file[at] ^= m;
                    parse(ext, file.data(), n);
                    file[at] ^= m;
                }
        }
    }
    if (files == 0) { fprintf(stderr, "no image files found\n"); return 2; }
    printf("image_check: %ld files, %ld parses accepted, %ld refused\n", files, accepted, refused);
    return 0;
}
