// mesh_check_main.cpp -- a stand-alone checker of the mesh export's PLY writer (MeshPly.cpp) for AddressSanitizer + UBSan runs: synthetic
// meshes (none, one triangle, 10 000 random records with every byte value) are written, read back by a parser of this file and compared
// field by field; arrays that are missing and a path that cannot be written are refused.  Its own main, no Python, no GPU.
//   make mesh_check && ../lib/mesh_check [directory]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cofusion_hip.h"

namespace cofusion {
bool writeMeshPly(const std::string& path, const cf_mesh_vertex* vertices, uint32_t nVertices, const uint32_t* triangles, uint32_t nTriangles);
}

static bool readBack(const std::string& path, std::vector<cf_mesh_vertex>& v, std::vector<uint32_t>& t)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<uint8_t> raw;
    uint8_t buf[4096]; size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + n);
    fclose(f);
    const std::string text(raw.begin(), raw.end());
    const size_t end = text.find("end_header\n");
    if (end == std::string::npos) return false;
    unsigned nv = 0, nt = 0;
    const size_t pv = text.find("element vertex "), pf = text.find("element face ");
    if (pv == std::string::npos || pf == std::string::npos || pv > end || pf > end) return false;
    if (sscanf(text.c_str() + pv, "element vertex %u", &nv) != 1 || sscanf(text.c_str() + pf, "element face %u", &nt) != 1) return false;
    const size_t body = end + 11;
    if (raw.size() != body + (size_t)nv * 27 + (size_t)nt * 13) return false;
    v.resize(nv); t.resize((size_t)nt * 3);
    for (unsigned i = 0; i < nv; i++) {
        const uint8_t* p = &raw[body + (size_t)i * 27];
        memcpy(&v[i].x, p, 24);
        v[i].r = p[24]; v[i].g = p[25]; v[i].b = p[26]; v[i].a = 255;
    }
    for (unsigned i = 0; i < nt; i++) {
        const uint8_t* p = &raw[body + (size_t)nv * 27 + (size_t)i * 13];
        if (p[0] != 3) return false;
        memcpy(&t[(size_t)i * 3], p + 1, 12);
    }
    return true;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? std::string(argv[1]) + "/" : std::string("/tmp/");
    int accepted = 0, refused = 0, failed = 0;
    uint32_t seed = 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed; };
    const uint32_t sizes[3][2] = {{0, 0}, {3, 1}, {10000, 19996}};
    for (int k = 0; k < 3; k++) {
        const uint32_t nv = sizes[k][0], nt = sizes[k][1];
        std::vector<cf_mesh_vertex> v(nv);
        std::vector<uint32_t> t((size_t)nt * 3);
        for (auto& p : v) {
            float* f = &p.x;
            for (int j = 0; j < 6; j++) f[j] = (float)(int)(rnd() >> 8) / 65536.0f - 64.0f;
            p.r = (uint8_t)rnd(); p.g = (uint8_t)(rnd() >> 8); p.b = (uint8_t)(rnd() >> 16); p.a = 255;
        }
        for (auto& i : t) i = nv ? rnd() % nv : 0;
        const std::string path = dir + "mesh_check_" + std::to_string(k) + ".ply";
        std::vector<cf_mesh_vertex> v2; std::vector<uint32_t> t2;
        bool ok = cofusion::writeMeshPly(path, v.data(), nv, t.data(), nt) && readBack(path, v2, t2) && v2.size() == nv && t2 == t;
        for (uint32_t i = 0; ok && i < nv; i++)
            ok = !memcmp(&v[i].x, &v2[i].x, 24) && v[i].r == v2[i].r && v[i].g == v2[i].g && v[i].b == v2[i].b;
        remove(path.c_str());
        if (ok) accepted++; else { failed++; printf("mesh %d: written and read back differ\n", k); }
    }
    cf_mesh_vertex one{}; uint32_t tri[3] = {0, 0, 0};
    const std::string path = dir + "mesh_check_refused.ply";
    if (!cofusion::writeMeshPly(path, nullptr, 1, tri, 1)) refused++; else { failed++; printf("vertices missing: not refused\n"); }
    if (!cofusion::writeMeshPly(path, &one, 1, nullptr, 1)) refused++; else { failed++; printf("triangles missing: not refused\n"); }
    if (!cofusion::writeMeshPly(dir + "no_such_directory/mesh.ply", &one, 1, tri, 1)) refused++; else { failed++; printf("unwritable path: not refused\n"); }
    remove(path.c_str());
    printf("%d accepted, %d refused, %d failed\n", accepted, refused, failed);
    return failed ? 1 : 0;
}
