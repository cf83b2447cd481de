// cf_mesh.h -- constants and tables of the mesh export (mesh.hip; tests/mesh_ref.py holds the same in numpy).
#pragma once

#include <stdint.h>

namespace cf {
namespace mesh {

constexpr float kWScale = 4096.0f;     // weights: 12 fraction bits
constexpr float kDScale = 32768.0f;    // distance / tau: 15 fraction bits
constexpr float kRScale = 65536.0f;    // radii of the default grid's mean: 16 fraction bits
constexpr float kRadiusLimit = 1024.0f;
constexpr float kDefaultTrunc = 3.0f, kDefaultSupport = 4.0f, kDefaultConfCap = 100.0f;
constexpr float kVoxelGrowth = 1.25f;  // the default grid's voxel grows by this factor until the grid fits
constexpr int kGrowthSteps = 256;
constexpr int kPlanes = 5;             // sum wq dq | sum wq | sum wq r | sum wq g | sum wq b
constexpr int kKinds = 7;              // edge kinds of a sample: far end at offset code = kind + 1 = dx | dy << 1 | dz << 2

// Kuhn's triangulation: per permutation of the axes (lexicographic) the path 000 -> +p0 -> +p0+p1 -> 111, corners as offset codes;
// the permutation's sign is the orientation of (v0, v1, v2, v3)
#define CF_MESH_TET_CORNERS {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}}
#define CF_MESH_TET_NEGATIVE {0, 1, 1, 0, 0, 1}
// local edges of a tetrahedron: 0 (0,1)  1 (0,2)  2 (0,3)  3 (1,2)  4 (1,3)  5 (2,3)
#define CF_MESH_EDGE_ENDS {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}}
// the 16 cases of a POSITIVE tetrahedron (bit i: local vertex i is inside): triangle count, then its local edges, wound so that the
// geometric normal points outside; a negative tetrahedron swaps the last two vertices of each triangle.
//   one inside vertex a:   (ab, ac, ad) for an even permutation (a, b, c, d), b < c < d the outside ones
//   one outside vertex a:  the reverse
//   a < b inside, c < d outside:  the quad ac, ad, bd, bc as (ac, ad, bd), (ac, bd, bc)
#define CF_MESH_CASES {                                                                           \
    {0, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 2, 0, 0, 0}, {1, 0, 4, 3, 0, 0, 0}, {2, 1, 2, 4, 1, 4, 3},   \
    {1, 1, 3, 5, 0, 0, 0}, {2, 0, 5, 2, 0, 3, 5}, {2, 0, 4, 5, 0, 5, 1}, {1, 2, 4, 5, 0, 0, 0},   \
    {1, 2, 5, 4, 0, 0, 0}, {2, 0, 1, 5, 0, 5, 4}, {2, 0, 5, 3, 0, 2, 5}, {1, 1, 5, 3, 0, 0, 0},   \
    {2, 1, 3, 4, 1, 4, 2}, {1, 0, 3, 4, 0, 0, 0}, {1, 0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}}

}  // namespace mesh
}  // namespace cf
