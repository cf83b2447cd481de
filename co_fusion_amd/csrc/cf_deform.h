// cf_deform.h -- launchers of the deformation-graph kernels (deform.hip) for the C-ABI (cabi_deform.hip).  DESIGN.md 4.14.
#pragma once

#include "cf_kernels.h"

namespace cf {

constexpr int kDeformMaxNodes = 1024;   // Deformation.cpp:26
constexpr int kDeformMaxCons = 128;     // constraints, pins included, of cf_deform_create (the fern path makes at most 50 + 50)
constexpr int kDeformMaxConsSized = 1536;   // ... the most cf_deform_create_sized takes (a local closure: 768 + 768 at 640x480)
constexpr int kDeformAllEnabled = -2147483647 - 1;   // last_deform_time of the global mode: every node time is above it
constexpr int kDeformK = 4;             // neighbours of a node, nodes of a weight set
constexpr int kDeformVars = 12;         // unknowns per node: 3x3 column-major, translation
constexpr int kDeformBand = 240;        // band entries per row of A, diagonal included: nodes couple at most 19 apart
constexpr int kDeformMinNodes = kDeformK + 1;

struct DeformMeta { int count, monotone; };
// what one residual pass / one solve leaves for the host (pinned read-back of 32 bytes)
struct DeformOut { float error, mean_cons_error; double delta_norm; int failed, enabled, pad[2]; };   // enabled: nodes with time > last_deform_time

struct DeformGraph {          // device pointers of a cf_deform object
    float4* nodes;            // [kDeformMaxNodes] x y z init_time
    float* params;            // [kDeformMaxNodes][12]
    int* edges;               // [kDeformMaxNodes][4]
    float4 *cons_src, *cons_dst;   // [the object's capacity] x y z time
    int4* ids; float4* w;     // [the object's capacity] weight sets, ids ascending; a NaN weight: the point does not move
    double *AB, *b, *r;       // band of A [12 n][kDeformBand], right-hand side / delta [12 n], residual rows
    DeformOut* out;
};

struct DeformReactivate {
    float t_inv[16]; cf_cam cam; int cols, rows; float max_depth; const float* depth; float threshold; float tick;
};

void launch_deform_sample(hipStream_t s, const float* map, unsigned count, unsigned stride, const DeformGraph& g, DeformMeta* meta);
void launch_deform_init_graph(hipStream_t s, const DeformGraph& g, int n, bool identity);
void launch_deform_weights(hipStream_t s, const DeformGraph& g, int n, int n_cons);
// last_deform_time: node i is enabled iff int(time_i) > last_deform_time (DeformationGraph.cpp:401-410); kDeformAllEnabled: the global mode
void launch_deform_residual(hipStream_t s, const DeformGraph& g, int n, int n_cons, int last_deform_time);
void launch_deform_assemble(hipStream_t s, const DeformGraph& g, int n, int n_cons, int last_deform_time);
void launch_deform_solve(hipStream_t s, const DeformGraph& g, int n);
// last_deform_time >= 0: surfels none of whose four nodes is enabled (node time > last_deform_time) are not moved; < 0: every surfel is
void launch_deform_apply(hipStream_t s, const DeformGraph& g, int n, float* map, unsigned count, const DeformReactivate* re, int last_deform_time);
void launch_deform_poses(hipStream_t s, const DeformGraph& g, int n, float* poses, const int* times, int n_poses);

}  // namespace cf
