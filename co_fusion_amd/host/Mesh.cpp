// Mesh.cpp -- CoFusion's mesh export: one triangle mesh per model through cf_mesh_* (csrc/mesh.hip), written as
// <prefix>mesh-<id>.ply by writeMeshPly (MeshPly.cpp).
//   mesh-<id>.ply : binary little-endian; vertices  x y z nx ny nz (f32)  red green blue (u8);  faces  list uchar int vertex_indices.
//                   Positions mapped by Tp = globalPose * modelPose^-1 (savePly's), normals by Tp's rotation block -- which is savePly's
//                   (Tp^-1)^T for a rigid Tp -- and NOT negated: the mesher's normals point outside already.
// The mesher object (64 bytes per voxel of meshMaxVoxels) is created by the first call and kept; nothing of the frame loop changes.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "CoFusion.h"

namespace cofusion {

static void mcheck(cf_ctx* ctx, int rc, const char* what)
{
    if (rc != CF_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + (ctx ? cf_last_error(ctx) : ""));
}

void CoFusion::releaseMesher()
{
    if (mesher) cf_mesh_destroy(mesher);
    mesher = nullptr; meshKept = false;
}

void CoFusion::setMeshMaxVoxels(uint64_t n)
{
    if (n < 1 || n > CF_MESH_MAX_VOXELS) throw std::runtime_error("setMeshMaxVoxels: 1 .. 2^28");
    if (n != meshMaxVoxels) releaseMesher();
    meshMaxVoxels = n;
}

// index >= 0: the active models in list order (0 = background); index < 0: the kept inactive model number -1 - index
Model* CoFusion::meshModel(int index)
{
    ModelList& l = index >= 0 ? models : inactiveModels;
    const size_t k = index >= 0 ? (size_t)index : (size_t)(-1 - index);
    if (k >= l.size()) return nullptr;
    auto it = l.begin();
    std::advance(it, k);
    return it->get();
}

Mat4f CoFusion::meshTransform(Model& model) const
{
    if (!globalModel || &model == globalModel.get()) return Mat4f::identity();
    return globalModel->getPose() * model.getPose().inverse();   // (Export.cpp's Tp)
}

void CoFusion::extractMesh(int index, float voxel, uint32_t* nVertices, uint32_t* nTriangles)
{
    Model* model = meshModel(index);
    if (!model) throw std::runtime_error("mesh: model index out of range");
    *nVertices = 0; *nTriangles = 0;
    meshKept = false;
    if (!model->isOwned()) return;   // model-parallel mode: the owner rank meshes
    if (!mesher) mcheck(ctx, cf_mesh_create(ctx, meshMaxVoxels, &mesher), "cf_mesh_create");
    const float thr = model->getConfidenceThreshold();
    cf_mesh_grid grid;
    mcheck(ctx, cf_mesh_default_grid(mesher, model->handle(), thr, voxel, &grid), "cf_mesh_default_grid");
    mcheck(ctx, cf_mesh_accumulate(mesher, model->handle(), nullptr, 0, thr, &grid, nullptr), "cf_mesh_accumulate");
    mcheck(ctx, cf_mesh_extract(mesher, 1.0f, nVertices, nTriangles), "cf_mesh_extract");
    meshKept = true; meshIndex = index; meshVoxel = voxel; meshTick = tick; meshVertices = *nVertices; meshTriangles = *nTriangles;
}

bool CoFusion::keptMesh(int index, float voxel, uint32_t* nVertices, uint32_t* nTriangles) const
{
    if (!meshKept || meshIndex != index || memcmp(&meshVoxel, &voxel, 4) || meshTick != tick) return false;
    *nVertices = meshVertices; *nTriangles = meshTriangles;
    return true;
}

void CoFusion::downloadMesh(cf_mesh_vertex* vertices, uint32_t* triangles)
{
    if (!meshKept) throw std::runtime_error("mesh: nothing extracted");
    mcheck(ctx, cf_mesh_download(mesher, vertices, triangles), "cf_mesh_download");
}

int CoFusion::saveMesh(const std::string& exportDir, float voxel)
{
    int written = 0, index = 0;
    std::vector<cf_mesh_vertex> v;
    std::vector<uint32_t> t;
    for (auto& model : models) {
        const int i = index++;
        if (!model->isOwned()) continue;   // model-parallel mode: the owner rank writes the mesh
        uint32_t nv = 0, nt = 0;
        extractMesh(i, voxel, &nv, &nt);
        v.resize(nv); t.resize((size_t)nt * 3);
        downloadMesh(v.data(), t.data());
        const Mat4f Tp = meshTransform(*model);
        for (auto& p : v) {
            const float x = p.x, y = p.y, z = p.z, a = p.nx, b = p.ny, c = p.nz;
            p.x = Tp.m[0] * x + Tp.m[1] * y + Tp.m[2] * z + Tp.m[3];
            p.y = Tp.m[4] * x + Tp.m[5] * y + Tp.m[6] * z + Tp.m[7];
            p.z = Tp.m[8] * x + Tp.m[9] * y + Tp.m[10] * z + Tp.m[11];
            p.nx = Tp.m[0] * a + Tp.m[1] * b + Tp.m[2] * c;
            p.ny = Tp.m[4] * a + Tp.m[5] * b + Tp.m[6] * c;
            p.nz = Tp.m[8] * a + Tp.m[9] * b + Tp.m[10] * c;
        }
        if (!writeMeshPly(exportDir + "mesh-" + std::to_string(model->getID()) + ".ply", v.data(), nv, t.data(), nt)) return -1;
        written++;
    }
    return written;
}

}  // namespace cofusion
