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

// relative constraints (cf_deform_enable_relative): the ring of pairs a local closure leaves, and what a global step with them needs
constexpr int kDeformRelMax = 128;     // pairs of the ring at most
constexpr int kDeformRelMin = 8;       // ... at least (one pick appends up to 5)
constexpr int kDeformRelSlots = 8;     // node blocks of a relative row: the source set, then the target set's other nodes
constexpr int kDeformRelLd = 400;      // leading dimension of C: 3 * 128 relative rows and the row of Y^T y, rounded up to 16
struct DeformRel {
    float4 *src, *dst;        // the ring [capacity]: moved source x y z srcTime, target x y z dstTime
    int4* ids; float4* w;     // [2 capacity] weight sets: of the sources, then (from capacity) of the targets
    int* uid; double* uval;   // U in compact form: [capacity][8] node ids (-1: unused), [capacity][8][4] the entries of a block
    double* Y;                // [3 capacity][12 kDeformMaxNodes]: L^-1 U^T, one column of it per row here
    double *C, *Lc;           // [kDeformRelLd][kDeformRelLd] lower: I + Y^T Y with Y^T y in row m; its factor with t in row m
    int capacity;
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
// n_rel pairs of the ring (slot order) as relative rows behind the absolute ones; the global mode only.  A step with them is
//   residual_rel, assemble, rel_rhs, solve_factor, rel_y, rel_gram, rel_c, rel_correct, solve_finish, residual_rel
// each stage a launch: the stages meet at kernel boundaries.
void launch_deform_rel_weights(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel);   // weight sets and U
void launch_deform_residual_rel(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_cons, int n_rel);
void launch_deform_rel_rhs(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_cons, int n_rel);   // b -= U^T r_rel
void launch_deform_solve_factor(hipStream_t s, const DeformGraph& g, int n);    // B = L L^T in place, b <- L^-1 b; failed = 0 or 1
void launch_deform_rel_y(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel);
void launch_deform_rel_gram(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel);
void launch_deform_rel_c(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n_rel);
void launch_deform_rel_correct(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel);   // b <- b - Y t
void launch_deform_solve_finish(hipStream_t s, const DeformGraph& g, int n);    // b <- L^-T b, the update, |delta|; nothing after a failure
// the picks 0, s, 2s, .. < n_cons (s = max(1, n_cons / 3)) of the constraint rows (row = row_stride * index), the sources moved by the
// graph `from` (its map rule, local_time as cf_deform_apply has it), into the ring from slot `head` on
void launch_deform_rel_pick(hipStream_t s, const DeformGraph& from, int n_nodes, int local_time, const float* src, const float* dst, const float* time,
                            const float* dst_time, int n_cons, int row_stride, const DeformRel& rel, int head);
// last_deform_time >= 0: surfels none of whose four nodes is enabled (node time > last_deform_time) are not moved; < 0: every surfel is
void launch_deform_apply(hipStream_t s, const DeformGraph& g, int n, float* map, unsigned count, const DeformReactivate* re, int last_deform_time);
void launch_deform_poses(hipStream_t s, const DeformGraph& g, int n, float* poses, const int* times, int n_poses);

}  // namespace cf
