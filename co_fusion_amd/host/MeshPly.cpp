// MeshPly.cpp -- the PLY writer of the mesh export (CoFusion::saveMesh, Mesh.cpp): binary little-endian, vertices x y z nx ny nz (f32)
// red green blue (u8), faces list uchar int vertex_indices.  No device code and nothing of the facade: mesh_check_main.cpp runs it under
// AddressSanitizer + UBSan (`make mesh_check`).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cofusion_hip.h"

namespace cofusion {

bool writeMeshPly(const std::string& path, const cf_mesh_vertex* vertices, uint32_t nVertices, const uint32_t* triangles, uint32_t nTriangles)
{
    if ((nVertices && !vertices) || (nTriangles && !triangles)) return false;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
               "element face %u\nproperty list uchar int vertex_indices\nend_header\n", nVertices, nTriangles);
    // records are packed by hand: 27 bytes per vertex, 13 per face (the in-memory records carry padding / no count byte)
    std::vector<uint8_t> buf;
    buf.resize((size_t)nVertices * 27);
    for (uint32_t i = 0; i < nVertices; i++) {
        uint8_t* o = &buf[(size_t)i * 27];
        memcpy(o, &vertices[i].x, 24);
        o[24] = vertices[i].r; o[25] = vertices[i].g; o[26] = vertices[i].b;
    }
    bool ok = buf.empty() || fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    buf.resize((size_t)nTriangles * 13);
    for (uint32_t i = 0; i < nTriangles; i++) {
        uint8_t* o = &buf[(size_t)i * 13];
        o[0] = 3;
        memcpy(o + 1, &triangles[(size_t)i * 3], 12);
    }
    ok = ok && (buf.empty() || fwrite(buf.data(), 1, buf.size(), f) == buf.size());
    return fclose(f) == 0 && ok;
}

}  // namespace cofusion
