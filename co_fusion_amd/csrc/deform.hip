// deform.hip -- loop closure: ElasticFusion's deformation graph (Core/Model/Deformation.*, Core/Utils/DeformationGraph.*, the node branch of
// Core/Shaders/copy_unstable.vert:155-335), device resident.  DESIGN.md 4.14 states the arithmetic; tests/deform_ref.py restates it in numpy.
//
//   deform_sample_kernel     every stride-th surfel becomes a node (x, y, z, init_time); count, monotone flag, identity parameters, edges
//   deform_weights_kernel    one lane per constraint point: the window rule -> four node ids (ascending) and weights
//   deform_residual_kernel   residual rows (E_rot, E_reg, E_con) in f32, widened; error = sum r^2 and the mean constraint error
//   deform_assemble_kernel   A = J^T J in band storage and b = -J^T r: one workgroup per 12x12 block, every entry summed by ONE thread in
//                            row order (the same bits on every run; no atomics)
//                            (both take last_deform_time, the graph's local mode: the nodes not younger than it leave the system)
//   deform_solve_kernel      band Cholesky by block columns in one workgroup (panel in LDS, trailing window in L2), forward substitution
//                            fused into the factorisation, backward substitution, the parameter update and |delta|
//                            (<1> / <2>: its two halves, for the step with relative rows)
//   deform_rel_*_kernel      relative constraints ("relative constraints" below): U in compact form, b -= U^T r, Y = L^-1 U^T by columns,
//                            C = I + Y^T Y and Y^T y, C's Cholesky and t, y - Y t; the pick of an accepted local closure into the ring
//   deform_apply_kernel      the map pass: node positions and times in LDS for the search and the 20 distances, the four chosen nodes'
//                            parameters from L2, whole 16 B records; the reactivation stamp when asked
//   deform_poses_kernel      one lane per keyframe pose: translation by the map rule, 3x3 -> polar factor (Newton in f64)
//
// All per-point arithmetic is f32 in the stated order (the library is built with -ffp-contract=off: no FMA), so weights and moved
// surfels are equal to the statement bit for bit; the normal equations and their solution are f64.
#include "cf_surfel_device.h"
#include "cf_deform.h"

namespace cf {

static constexpr int kDB = 256;       // threads per workgroup of the per-point kernels
static constexpr int kSolveT = 1024;  // threads of the one-workgroup kernels
static constexpr int kLook = 20, kBack = 10;

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// connectGraphSeq (DeformationGraph.cpp:218-245): neighbour k of node i among n >= 5
__device__ __forceinline__ int edge_of(int i, int k, int n)
{
    if (i < kDeformK / 2) return k < i ? k : k + 1;                       // 0..4 without i
    if (i >= n - kDeformK / 2) { const int base = n - (kDeformK + 1), li = i - base; return base + (k < li ? k : k + 1); }
    return (k & 1) ? i + (k >> 1) + 1 : i - (k >> 1) - 1;                   // i-1, i+1, i-2, i+2
}

struct NodeParams { float R[3][3]; f3 t; };
__device__ __forceinline__ NodeParams load_params(const float* __restrict__ params, int id)
{
    const float4* p = reinterpret_cast<const float4*>(params + (size_t)id * kDeformVars);
    const float4 a = p[0], b = p[1], c = p[2];
    NodeParams q;
    q.R[0][0] = a.x; q.R[1][0] = a.y; q.R[2][0] = a.z; q.R[0][1] = a.w; q.R[1][1] = b.x; q.R[2][1] = b.y;
    q.R[0][2] = b.z; q.R[1][2] = b.w; q.R[2][2] = c.x; q.t = f3{c.y, c.z, c.w};
    return q;
}

// The window rule (copy_unstable.vert:168-283 with the stated ties): the four nearest of up to 20 nodes around the node whose time is
// nearest to t.  nodes may be in LDS or global memory; n >= 5.  False (and nothing to apply) when a weight is not finite.
__device__ __forceinline__ bool window_weights(const float4* nodes, int n, f3 p, int t, int (&ids)[4], float (&w)[4])
{
    int imin = 0, imax = n - 1, imid = (imin + imax) / 2;
    while (imax >= imin) {
        imid = (imin + imax) / 2;
        const int nt = (int)nodes[imid].w;
        if (nt < t) imin = imid + 1;
        else if (nt > t) imax = imid - 1;
        else break;
    }
    imin = imin < n - 1 ? imin : n - 1;
    imax = imax > 0 ? imax : 0;
    const int a = abs((int)nodes[imin].w - t), b = abs((int)nodes[imid].w - t), c = abs((int)nodes[imax].w - t);
    const int found = (a <= b && a <= c) ? imin : (b <= a && b <= c) ? imid : imax;
    // the five smallest distances in candidate order (a later candidate never overtakes an equal earlier one)
    float bd[5]; int bi[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { bd[k] = __int_as_float(0x7f800000); bi[k] = 0; }
    const int lo = found - (kBack - 1) > 0 ? found - (kBack - 1) : 0;
    const int hi = (found + (kLook - (found - lo + 1)) < n - 1) ? found + (kLook - (found - lo + 1)) : n - 1;
    for (int s = 0; s < hi - lo + 1; s++) {
        const int j = s <= found - lo ? found - s : s + lo;   // found, found-1, .., lo, found+1, .., hi
        const float4 g = nodes[j];
        const float dx = p.x - g.x, dy = p.y - g.y, dz = p.z - g.z;
        float d = sqrtf((dx * dx + dy * dy) + dz * dz);
        int id = j;
        bool ins = false;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            ins = ins || d < bd[k];
            if (ins) { const float td = bd[k]; const int ti = bi[k]; bd[k] = d; bi[k] = id; d = td; id = ti; }
        }
    }
    const float dmax = bd[4];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) { const float q = 1.0f - bd[k] / dmax; w[k] = q * q; ids[k] = bi[k]; s = k ? s + w[k] : w[k]; }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) { w[k] = w[k] / s; ok = ok && finite_f(w[k]); }
    // VertexWeightMap::sort: by node id ascending
#define CF_CSWAP(i, j) if (ids[j] < ids[i]) { const int ti = ids[i]; ids[i] = ids[j]; ids[j] = ti; const float tw = w[i]; w[i] = w[j]; w[j] = tw; }
    CF_CSWAP(0, 1) CF_CSWAP(2, 3) CF_CSWAP(0, 2) CF_CSWAP(1, 3) CF_CSWAP(1, 2)
#undef CF_CSWAP
    return ok;
}

// sum over the weight set of w (R (p - g) + g + t), in id order
__device__ __forceinline__ f3 move_point(const float4* nodes, const float* __restrict__ params, f3 p, const int (&ids)[4], const float (&w)[4])
{
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float4 g4 = nodes[ids[k]];
        const NodeParams q = load_params(params, ids[k]);
        const float g[3] = {g4.x, g4.y, g4.z}, t[3] = {q.t.x, q.t.y, q.t.z};
        const float dx = p.x - g4.x, dy = p.y - g4.y, dz = p.z - g4.z;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            float v = (q.R[r][0] * dx + q.R[r][1] * dy) + q.R[r][2] * dz;
            v = v + g[r];
            v = v + t[r];
            acc[r] = acc[r] + w[k] * v;
        }
    }
    return f3{acc[0], acc[1], acc[2]};
}

// normalise(sum w R^-T n), R^-T by cofactors over the determinant
__device__ __forceinline__ f3 move_normal(const float* __restrict__ params, f3 nrm, const int (&ids)[4], const float (&w)[4])
{
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const NodeParams q = load_params(params, ids[k]);
        float C[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                C[r][c] = q.R[r1][c1] * q.R[r2][c2] - q.R[r1][c2] * q.R[r2][c1];
            }
        const float det = (q.R[0][0] * C[0][0] + q.R[0][1] * C[0][1]) + q.R[0][2] * C[0][2];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float m = ((C[r][0] / det) * nrm.x + (C[r][1] / det) * nrm.y) + (C[r][2] / det) * nrm.z;
            acc[r] = acc[r] + w[k] * m;
        }
    }
    const float len = sqrtf((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
    return f3{acc[0] / len, acc[1] / len, acc[2] / len};
}

// ------------------------------------------------------------------------------------------------ graph
__device__ __forceinline__ void init_node(const DeformGraph& g, int i, int n, bool identity)
{
    if (identity) {
        float4* p = reinterpret_cast<float4*>(g.params + (size_t)i * kDeformVars);
        p[0] = make_float4(1.f, 0.f, 0.f, 0.f); p[1] = make_float4(1.f, 0.f, 0.f, 0.f); p[2] = make_float4(1.f, 0.f, 0.f, 0.f);
    }
    int4 e = make_int4(0, 0, 0, 0);
    if (n >= kDeformMinNodes) e = make_int4(edge_of(i, 0, n), edge_of(i, 1, n), edge_of(i, 2, n), edge_of(i, 3, n));
    reinterpret_cast<int4*>(g.edges)[i] = e;
}

// one workgroup of kDeformMaxNodes threads; n = ceil(count / stride) <= kDeformMaxNodes (the host chose the stride so)
__global__ void __launch_bounds__(kDeformMaxNodes) deform_sample_kernel(const float4* __restrict__ map, unsigned count, unsigned stride, DeformGraph g,
                                                                        DeformMeta* __restrict__ meta)
{
    const int i = (int)threadIdx.x;
    const int n = (int)((count + stride - 1) / stride);
    int bad = 0;
    if (i < n) {
        const size_t at = (size_t)i * stride * 3;
        const float4 pc = map[at], ct = map[at + 1];
        g.nodes[i] = make_float4(pc.x, pc.y, pc.z, ct.z);
        init_node(g, i, n, true);
        if (i + 1 < n) bad = map[(size_t)(i + 1) * stride * 3 + 1].z < ct.z ? 1 : 0;
    }
    const int any_bad = __syncthreads_or(bad);
    if (i == 0) { meta->count = n; meta->monotone = any_bad ? 0 : 1; }
}

__global__ void __launch_bounds__(kDeformMaxNodes) deform_init_graph_kernel(DeformGraph g, int n, int identity)
{
    const int i = (int)threadIdx.x;
    if (i < n) init_node(g, i, n, identity != 0);
}

__global__ void __launch_bounds__(kDeformMaxCons) deform_weights_kernel(DeformGraph g, int n, int n_cons)
{
    const int l = (int)(blockIdx.x * kDeformMaxCons + threadIdx.x);
    if (l >= n_cons) return;
    const float4 s = g.cons_src[l];
    int ids[4]; float w[4];
    const bool ok = window_weights(g.nodes, n, f3{s.x, s.y, s.z}, (int)s.w, ids, w);
    g.ids[l] = make_int4(ids[0], ids[1], ids[2], ids[3]);
    const float bad = qnan();
    g.w[l] = ok ? make_float4(w[0], w[1], w[2], w[3]) : make_float4(bad, bad, bad, bad);
}

// ------------------------------------------------------------------------------------------------ energy
__device__ __forceinline__ float sqrt_reg() { return sqrtf(10.0f); }
constexpr float kSqrtCon = 10.0f;

// row layout of J: 6 n rotation rows, then 3 rows per directed edge (node, edge, component), then 3 per constraint
__device__ __forceinline__ int rot_row(int j, int q) { return 6 * j + q; }
__device__ __forceinline__ int edge_row(int n, int a, int k, int c) { return 6 * n + 3 * (kDeformK * a + k) + c; }
__device__ __forceinline__ int cons_row(int n, int l, int c) { return 18 * n + 3 * l + c; }

// J(rotation row q of a node, its unknown u)
__device__ __forceinline__ float jval_rot(const float* __restrict__ P, int q, int u)
{
    if (u >= 9) return 0.f;
    const int cu = u / 3, ru = u - 3 * cu;
    if (q >= 3) return cu == q - 3 ? 2.0f * P[3 * cu + ru] : 0.f;
    const int a = q == 2 ? 1 : 0, b = q == 0 ? 1 : 2;
    return cu == a ? P[3 * b + ru] : cu == b ? P[3 * a + ru] : 0.f;
}
// J(edge row a -> nb, component c; unknown u of node x) for x == a (own) or x == nb
__device__ __forceinline__ float jval_edge(f3 d, int c, bool own, int u)
{
    const float sr = sqrt_reg();
    if (!own) return u == 9 + c ? -sr : 0.f;
    if (u == 9 + c) return sr;
    if (u >= 9 || u % 3 != c) return 0.f;
    const int m = u / 3;
    return (m == 0 ? d.x : m == 1 ? d.y : d.z) * sr;
}
// J(constraint row, component c; unknown u of a node of its weight set with weight w, dw = (src - g) * w)
__device__ __forceinline__ float jval_cons(f3 dw, float w, int c, int u)
{
    if (u == 9 + c) return w * kSqrtCon;
    if (u >= 9 || u % 3 != c) return 0.f;
    const int m = u / 3;
    return (m == 0 ? dw.x : m == 1 ? dw.y : dw.z) * kSqrtCon;
}
__device__ __forceinline__ f3 node_pos(const DeformGraph& g, int i) { const float4 v = g.nodes[i]; return f3{v.x, v.y, v.z}; }
__device__ __forceinline__ bool node_on(const DeformGraph& g, int i, int ldt) { return (int)g.nodes[i].w > ldt; }
__device__ __forceinline__ int id_of(int4 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ float w_of(float4 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// fixed-order sum of one double per thread over the workgroup (kSolveT threads); the result in every thread
__device__ __forceinline__ double block_sum(double v, double* red)
{
    const int t = (int)threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int o = kSolveT / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = red[t] + red[t + o];
        __syncthreads();
    }
    return red[0];
}

// residual rows -> g.r; error, mean constraint error and the number of enabled nodes -> g.out.  One workgroup of kSolveT threads.
// A dropped row (the rotation rows of a disabled node, an edge between two disabled nodes, a constraint none of whose four nodes is
// enabled) is written as 0: it adds nothing to the error, and no enabled column of J meets it.  The mean constraint error is over
// ALL constraints (nonRelativeConstraintError does not look at `enabled`).
// kRel: the n_rel pairs of the ring follow the absolute constraints as rows f32(phi(src) - phi(tgt)) * 10 (the global mode only: ldt
// enables every node); they count in the error and in the DENOMINATOR of the mean constraint error (nonRelativeConstraintError).
template <bool kRel>
__global__ void __launch_bounds__(kSolveT) deform_residual_kernel(DeformGraph g, int n, int n_cons, int ldt, DeformRel rel, int n_rel)
{
    __shared__ double red[kSolveT];
    __shared__ float norms[kDeformMaxConsSized];
    const int t = (int)threadIdx.x;
    const float sr = sqrt_reg();
    for (int l = t; l < n_cons; l += kSolveT) {
        const float4 s = g.cons_src[l], q = g.cons_dst[l], w4 = g.w[l];
        const int4 i4 = g.ids[l];
        const int ids[4] = {i4.x, i4.y, i4.z, i4.w};
        const float w[4] = {w4.x, w4.y, w4.z, w4.w};
        f3 m = f3{s.x, s.y, s.z};
        if (finite_f(w4.x)) m = move_point(g.nodes, g.params, m, ids, w);
        const float dx = m.x - q.x, dy = m.y - q.y, dz = m.z - q.z;
        const bool keep = node_on(g, ids[0], ldt) || node_on(g, ids[1], ldt) || node_on(g, ids[2], ldt) || node_on(g, ids[3], ldt);
        g.r[cons_row(n, l, 0)] = keep ? (double)dx * (double)kSqrtCon : 0.0;
        g.r[cons_row(n, l, 1)] = keep ? (double)dy * (double)kSqrtCon : 0.0;
        g.r[cons_row(n, l, 2)] = keep ? (double)dz * (double)kSqrtCon : 0.0;
        norms[l] = sqrtf((dx * dx + dy * dy) + dz * dz);
    }
    if (kRel) {
        for (int p = t; p < n_rel; p += kSolveT) {
            f3 m[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const float4 s = e ? rel.dst[p] : rel.src[p], w4 = rel.w[e * rel.capacity + p];
                const int4 i4 = rel.ids[e * rel.capacity + p];
                const int ids[4] = {i4.x, i4.y, i4.z, i4.w};
                const float w[4] = {w4.x, w4.y, w4.z, w4.w};
                m[e] = f3{s.x, s.y, s.z};
                if (finite_f(w4.x)) m[e] = move_point(g.nodes, g.params, m[e], ids, w);
            }
            const float dx = m[0].x - m[1].x, dy = m[0].y - m[1].y, dz = m[0].z - m[1].z;
            g.r[cons_row(n, n_cons + p, 0)] = (double)dx * (double)kSqrtCon;
            g.r[cons_row(n, n_cons + p, 1)] = (double)dy * (double)kSqrtCon;
            g.r[cons_row(n, n_cons + p, 2)] = (double)dz * (double)kSqrtCon;
        }
    }
    int on_count = 0;
    for (int j = t; j < n; j += kSolveT) {
        const bool on = node_on(g, j, ldt);
        on_count += on ? 1 : 0;
        const float* P = g.params + (size_t)j * kDeformVars;
        float Pj[12];
#pragma unroll
        for (int k = 0; k < 12; k++) Pj[k] = P[k];
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const int a = q >= 3 ? q - 3 : (q == 2 ? 1 : 0), b = q >= 3 ? q - 3 : (q == 0 ? 1 : 2);
            const float dot = (Pj[3 * a] * Pj[3 * b] + Pj[3 * a + 1] * Pj[3 * b + 1]) + Pj[3 * a + 2] * Pj[3 * b + 2];
            g.r[rot_row(j, q)] = !on ? 0.0 : q >= 3 ? (double)dot - 1.0 : (double)dot;
        }
        const f3 gj = node_pos(g, j);
        const float gv[3] = {gj.x, gj.y, gj.z};
        for (int k = 0; k < kDeformK; k++) {
            const int nb = g.edges[j * kDeformK + k];
            const f3 gn = node_pos(g, nb);
            const float gnv[3] = {gn.x, gn.y, gn.z};
            const float* Pn = g.params + (size_t)nb * kDeformVars;
            const float dx = gn.x - gj.x, dy = gn.y - gj.y, dz = gn.z - gj.z;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float v = (Pj[c] * dx + Pj[3 + c] * dy) + Pj[6 + c] * dz;
                v = v + gv[c];
                v = v + Pj[9 + c];
                v = v - (gnv[c] + Pn[9 + c]);
                g.r[edge_row(n, j, k, c)] = on || node_on(g, nb, ldt) ? (double)v * (double)sr : 0.0;
            }
        }
    }
    const int enabled = __syncthreads_count(on_count);   // (n <= kSolveT: one node per thread)
    const int rows = 18 * n + 3 * n_cons + (kRel ? 3 * n_rel : 0);
    double s = 0.0;
    for (int i = t; i < rows; i += kSolveT) { const double v = g.r[i]; s = s + v * v; }
    const double e = block_sum(s, red);
    if (t == 0) {
        float m = 0.f;
        for (int l = 0; l < n_cons; l++) m = m + norms[l];
        g.out->error = (float)e;
        g.out->mean_cons_error = m / (float)(kRel ? n_cons + n_rel : n_cons);
        g.out->enabled = enabled;
    }
}

// workgroup (I, dj): the 12x12 block of A at block row I, block column J = I - dj, entry (r, c) by thread 12 r + c; the workgroups of
// dj == 0 also sum b (threads 144..155).  Every sum runs over the rows of J in row order.
// A disabled node's columns leave the system: its blocks of A are zero, its diagonal block the identity, its part of b zero.  A block
// between two enabled nodes sums exactly the rows it summed before (every row that meets an enabled column is kept).
__global__ void __launch_bounds__(192) deform_assemble_kernel(DeformGraph g, int n, int n_cons, int ldt)
{
    const int I = (int)blockIdx.x / (kDeformBand / kDeformVars), dj = (int)blockIdx.x % (kDeformBand / kDeformVars), J = I - dj;
    const int t = (int)threadIdx.x;
    if (J < 0 || t >= 156 || (t >= 144 && dj != 0)) return;
    const bool rhs = t >= 144;
    const int r = rhs ? t - 144 : t / 12, c = rhs ? 0 : t % 12;
    if (!node_on(g, I, ldt) || !node_on(g, J, ldt)) {
        const int i = kDeformVars * I + r, j = kDeformVars * J + c;
        if (rhs) g.b[i] = 0.0;
        else if (j <= i) g.AB[(size_t)i * kDeformBand + (i - j)] = i == j ? 1.0 : 0.0;
        return;
    }
    double s = 0.0;
    if (I == J) {
        const float* P = g.params + (size_t)I * kDeformVars;
        for (int q = 0; q < 6; q++) {
            const double a = (double)jval_rot(P, q, r);
            s = s + a * (rhs ? g.r[rot_row(I, q)] : (double)jval_rot(P, q, c));
        }
    }
    if (dj <= 2 * kDeformK) {   // an edge row touches nodes at most 4 apart
        const int a0 = I - kDeformK > 0 ? I - kDeformK : 0, a1 = I + kDeformK < n - 1 ? I + kDeformK : n - 1;
        for (int a = a0; a <= a1; a++) {
            const f3 ga = node_pos(g, a);
            for (int k = 0; k < kDeformK; k++) {
                const int nb = g.edges[a * kDeformK + k];
                if (!((a == I || nb == I) && (a == J || nb == J))) continue;
                const f3 gn = node_pos(g, nb);
                const f3 d = f3{gn.x - ga.x, gn.y - ga.y, gn.z - ga.z};
                for (int cc = 0; cc < 3; cc++) {
                    const double vi = (double)jval_edge(d, cc, a == I, r);
                    s = s + vi * (rhs ? g.r[edge_row(n, a, k, cc)] : (double)jval_edge(d, cc, a == J, c));
                }
            }
        }
    }
    for (int l = 0; l < n_cons; l++) {
        const int4 ids = g.ids[l];
        int ki = -1, kj = -1;
        for (int k = 0; k < 4; k++) { if (id_of(ids, k) == I) ki = k; if (id_of(ids, k) == J) kj = k; }
        if (ki < 0 || kj < 0) continue;
        const float4 w4 = g.w[l];
        if (!finite_f(w4.x)) continue;
        const float4 sp = g.cons_src[l];
        const f3 gi = node_pos(g, I), gj = node_pos(g, J);
        const float wi = w_of(w4, ki), wj = w_of(w4, kj);
        const f3 di = f3{(sp.x - gi.x) * wi, (sp.y - gi.y) * wi, (sp.z - gi.z) * wi};
        const f3 dq = f3{(sp.x - gj.x) * wj, (sp.y - gj.y) * wj, (sp.z - gj.z) * wj};
        for (int cc = 0; cc < 3; cc++) {
            const double vi = (double)jval_cons(di, wi, cc, r);
            s = s + vi * (rhs ? g.r[cons_row(n, l, cc)] : (double)jval_cons(dq, wj, cc, c));
        }
    }
    const int i = kDeformVars * I + r;
    if (rhs) { g.b[i] = -s; return; }
    const int j = kDeformVars * J + c;
    if (j <= i) g.AB[(size_t)i * kDeformBand + (i - j)] = s;
}

// A = L L^T in place (band storage, AB[i][d] = A[i][i - d]), L y = b, L^T x = y, params += x.  One workgroup of kSolveT threads.
// kPart 0: the whole step.  The step with relative rows works on y between the two halves: kPart 1 ends behind the forward substitution
// (L in AB, y in b, failed = 0 or 1), kPart 2 starts at the backward substitution and does nothing after a failure.
template <int kPart>
__global__ void __launch_bounds__(kSolveT) deform_solve_kernel(DeformGraph g, int n)
{
    constexpr int V = kDeformVars, BW = kDeformBand;
    __shared__ double P[BW][V + 1];   // the panel: rows c0 .. c0 + 239 of block column c0 .. c0 + 11
    __shared__ double y[V];
    __shared__ double red[kSolveT];
    const int t = (int)threadIdx.x;
    const int nv = V * n;
    double* AB = g.AB; double* b = g.b;   // (workgroup-shared through the barriers: not restrict)
    if (kPart == 2 && g.out->failed) {   // (the same value in every thread)
        if (t == 0) g.out->delta_norm = 0.0;
        return;
    }
    for (int c0 = 0; kPart != 2 && c0 < nv; c0 += V) {
        const int rows = nv - c0 < BW ? nv - c0 : BW;
        for (int e = t; e < rows * V; e += kSolveT) {
            const int ri = e / V, c = e - ri * V;
            P[ri][c] = ri >= c ? AB[(size_t)(c0 + ri) * BW + (ri - c)] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < V; c++) {
            const double piv = P[c][c];
            if (!(piv > 0.0)) {   // (the same value in every thread: the whole workgroup leaves)
                if (t == 0) { g.out->failed = 1; g.out->delta_norm = 0.0; }
                return;
            }
            const double l = sqrt(piv);
            __syncthreads();
            for (int ri = c + t; ri < rows; ri += kSolveT) P[ri][c] = ri == c ? l : P[ri][c] / l;
            __syncthreads();
            const int w = V - 1 - c;   // columns c+1 .. 11
            for (int e = t; e < (rows - c - 1) * w; e += kSolveT) {
                const int ri = c + 1 + e / w, cc = c + 1 + e % w;
                if (ri >= cc) P[ri][cc] = P[ri][cc] - P[ri][c] * P[cc][c];
            }
            __syncthreads();
        }
        for (int e = t; e < rows * V; e += kSolveT) {
            const int ri = e / V, c = e - ri * V;
            if (ri >= c) AB[(size_t)(c0 + ri) * BW + (ri - c)] = P[ri][c];
        }
        if (t == 0) {
            for (int c = 0; c < V; c++) {
                double v = b[c0 + c];
                for (int k = 0; k < c; k++) v = v - P[c][k] * y[k];
                y[c] = v / P[c][c];
                b[c0 + c] = y[c];
            }
        }
        __syncthreads();
        for (int ri = V + t; ri < rows; ri += kSolveT) {
            double v = b[c0 + ri];
            for (int c = 0; c < V; c++) v = v - P[ri][c] * y[c];
            b[c0 + ri] = v;
        }
        const int m = rows - V;   // the trailing window: rows and columns c0 + 12 .. c0 + rows - 1
        for (int e = t; e < m * m; e += kSolveT) {
            const int i = V + e / m, j = V + e % m;
            if (j > i) continue;
            const size_t at = (size_t)(c0 + i) * BW + (i - j);
            double v = AB[at];
            for (int c = 0; c < V; c++) v = v - P[i][c] * P[j][c];
            AB[at] = v;
        }
        __syncthreads();
    }
    if (kPart == 1) {
        if (t == 0) g.out->failed = 0;
        return;
    }
    // L^T x = y, last block column first
    for (int c0 = nv - V; c0 >= 0; c0 -= V) {
        const int rows = nv - c0 < BW ? nv - c0 : BW;
        for (int e = t; e < rows * V; e += kSolveT) {
            const int ri = e / V, c = e - ri * V;
            P[ri][c] = ri >= c ? AB[(size_t)(c0 + ri) * BW + (ri - c)] : 0.0;
        }
        __syncthreads();
        const int wave = t >> 6, lane = t & 63;
        if (wave < V) {   // wave c: sum over the rows below the diagonal block of L[ri][c] x[ri]
            double s = 0.0;
            for (int ri = V + lane; ri < rows; ri += 64) s = s + P[ri][wave] * b[c0 + ri];
            for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
            if (lane == 0) y[wave] = s;
        }
        __syncthreads();
        if (t == 0) {
            for (int c = V - 1; c >= 0; c--) {
                double v = b[c0 + c] - y[c];
                for (int k = c + 1; k < V; k++) v = v - P[k][c] * b[c0 + k];
                b[c0 + c] = v / P[c][c];
            }
        }
        __syncthreads();
    }
    // applyDeltaSparse: f32(f64(param) + delta); |delta|
    double s = 0.0;
    for (int i = t; i < nv; i += kSolveT) {
        const double d = b[i];
        g.params[i] = (float)((double)g.params[i] + d);
        s = s + d * d;
    }
    const double dn = block_sum(s, red);
    if (t == 0) { g.out->delta_norm = sqrt(dn); g.out->failed = 0; }
}

// ------------------------------------------------------------------------------------------------ map and poses
template <bool kStamp>
__global__ void __launch_bounds__(kDB) deform_apply_kernel(DeformGraph g, int n, float4* __restrict__ map, unsigned count, DeformReactivate re,
                                                           int last_deform_time)
{
    __shared__ float4 nodes[kDeformMaxNodes];
    for (int i = (int)threadIdx.x; i < n; i += kDB) nodes[i] = g.nodes[i];
    __syncthreads();
    Mat4 T;
    if (kStamp) {
#pragma unroll
        for (int k = 0; k < 16; k++) T.m[k] = re.t_inv[k];
    }
    for (size_t i = (size_t)blockIdx.x * kDB + threadIdx.x; i < count; i += (size_t)gridDim.x * kDB) {
        float4 pc = map[i * 3], ct = map[i * 3 + 1];
        int ids[4]; float w[4];
        // (the local mode: a surfel none of whose four nodes is enabled keeps its bits -- the identity of disabled nodes would still round
        // (p - g) + g; with last_deform_time < 0, the global mode, every node time passes)
        if (window_weights(nodes, n, f3{pc.x, pc.y, pc.z}, (int)ct.z, ids, w) &&
            ((int)nodes[ids[0]].w > last_deform_time || (int)nodes[ids[1]].w > last_deform_time || (int)nodes[ids[2]].w > last_deform_time ||
             (int)nodes[ids[3]].w > last_deform_time)) {
            float4 nr = map[i * 3 + 2];
            const f3 p = move_point(nodes, g.params, f3{pc.x, pc.y, pc.z}, ids, w);
            const f3 m = move_normal(g.params, f3{nr.x, nr.y, nr.z}, ids, w);
            pc.x = p.x; pc.y = p.y; pc.z = p.z;
            nr.x = m.x; nr.y = m.y; nr.z = m.z;
            map[i * 3] = pc; map[i * 3 + 2] = nr;
        }
        if (kStamp && pc.w > re.threshold) {
            const f3 l = xform_point(T, f3{pc.x, pc.y, pc.z});
            const float x = ((re.cam.fx * l.x) / l.z) + re.cam.cx, y = ((re.cam.fy * l.y) / l.z) + re.cam.cy;
            if (l.z > 0.f && l.z < re.max_depth && x > 0.f && y > 0.f && x < (float)re.cols && y < (float)re.rows) {
                const float d = re.depth[(size_t)((int)floorf(y)) * re.cols + (int)floorf(x)];
                if (d > 0.f && l.z < d + 0.1f) { ct.w = re.tick; map[i * 3 + 1] = ct; }
            }
        }
    }
}

__device__ __forceinline__ void inv_t_33(const double (&X)[3][3], double (&Y)[3][3])
{
    double C[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            C[r][c] = X[r1][c1] * X[r2][c2] - X[r1][c2] * X[r2][c1];
        }
    const double det = (X[0][0] * C[0][0] + X[0][1] * C[0][1]) + X[0][2] * C[0][2];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Y[r][c] = C[r][c] / det;
}

// applyGraphToPoses: poses row-major 4x4 [n_poses], times [n_poses]
__global__ void __launch_bounds__(kDB) deform_poses_kernel(DeformGraph g, int n, float* __restrict__ poses, const int* __restrict__ times, int n_poses)
{
    const int i = (int)(blockIdx.x * kDB + threadIdx.x);
    if (i >= n_poses) return;
    float* M = poses + (size_t)i * 16;
    const f3 p = f3{M[3], M[7], M[11]};
    int ids[4]; float w[4];
    if (!window_weights(g.nodes, n, p, times[i], ids, w)) return;
    const f3 q = move_point(g.nodes, g.params, p, ids, w);
    float B[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const NodeParams np = load_params(g.params, ids[k]);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) B[r][c] = B[r][c] + w[k] * np.R[r][c];
    }
    double X[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) X[r][c] = (double)((B[r][0] * M[c] + B[r][1] * M[4 + c]) + B[r][2] * M[8 + c]);
    for (int it = 0; it < 20; it++) {   // the orthogonal polar factor: X <- (X + X^-T) / 2
        double Y[3][3];
        inv_t_33(X, Y);
        bool same = true;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) { const double v = 0.5 * (X[r][c] + Y[r][c]); same = same && v == X[r][c]; X[r][c] = v; }
        if (same) break;
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) M[4 * r + c] = (float)X[r][c];
    }
    M[3] = q.x; M[7] = q.y; M[11] = q.z;
}

// ------------------------------------------------------------------------------------------------ relative constraints
// A = B + U^T U with B the band system and U the 3 n_rel relative rows, solved on the band factor ("Relative rows"):
//   L L^T = B, y = L^-1 b, Y = L^-1 U^T, C = I + Y^T Y, t = C^-1 (Y^T y), delta = L^-T (y - Y t)
// Every sum has one fixed order and no stage uses atomics: the same bytes on every run.  The stages meet at kernel boundaries.

// U in compact form, one thread per pair: the entries of a row do not depend on its component c -- node block o = 12 id holds
// e.x, e.y, e.z at o + c, o + 3 + c, o + 6 + c and w * 10 at o + 9 + c with e = ((p - g) * w) * 10 in f32 -- so a pair keeps eight node
// slots of four values: the source set, then the target set negated, a node of both in one slot (f64 sum, source first).
__global__ void __launch_bounds__(kDeformRelMax) deform_rel_rows_kernel(DeformGraph g, DeformRel rel, int n_rel)
{
    const int p = (int)threadIdx.x;
    if (p >= n_rel) return;
    int* uid = rel.uid + (size_t)p * kDeformRelSlots;
    double* uval = rel.uval + (size_t)p * kDeformRelSlots * 4;
    for (int s = 0; s < kDeformRelSlots; s++) {
        uid[s] = -1;
        for (int q = 0; q < 4; q++) uval[4 * s + q] = 0.0;
    }
    if (!finite_f(rel.w[p].x) || !finite_f(rel.w[rel.capacity + p].x)) return;   // a NaN set: the rows stay empty
    int used = 0;
    for (int e = 0; e < 2; e++) {
        const float4 pt = e ? rel.dst[p] : rel.src[p], w4 = rel.w[e * rel.capacity + p];
        const int4 i4 = rel.ids[e * rel.capacity + p];
        for (int k = 0; k < kDeformK; k++) {
            const int id = id_of(i4, k);
            const float w = w_of(w4, k);
            const f3 gp = node_pos(g, id);
            const float v[4] = {((pt.x - gp.x) * w) * kSqrtCon, ((pt.y - gp.y) * w) * kSqrtCon, ((pt.z - gp.z) * w) * kSqrtCon, w * kSqrtCon};
            int at = used;
            for (int s = 0; s < used; s++) at = uid[s] == id ? s : at;
            if (at == used) { uid[at] = id; used++; }
            for (int q = 0; q < 4; q++) uval[4 * at + q] = uval[4 * at + q] + (e ? -(double)v[q] : (double)v[q]);
        }
    }
}

// unknown u of a node -> (component c of the rows that meet it, which of the block's four values)
__device__ __forceinline__ int rel_comp(int u) { return u < 9 ? u % 3 : u - 9; }
__device__ __forceinline__ int rel_quad(int u) { return u < 9 ? u / 3 : 3; }

// b <- b - U^T r_rel, one thread per unknown, the sum over the rows in row order from 0
__global__ void __launch_bounds__(kDB) deform_rel_rhs_kernel(DeformGraph g, DeformRel rel, int n, int n_cons, int n_rel)
{
    const int i = (int)(blockIdx.x * kDB + threadIdx.x);
    if (i >= kDeformVars * n) return;
    const int I = i / kDeformVars, u = i - kDeformVars * I, c = rel_comp(u), q = rel_quad(u);
    double s = 0.0;
    for (int p = 0; p < n_rel; p++)
        for (int k = 0; k < kDeformRelSlots; k++)
            if (rel.uid[p * kDeformRelSlots + k] == I) s = s + rel.uval[(size_t)(p * kDeformRelSlots + k) * 4 + q] * g.r[cons_row(n, n_cons + p, c)];
    g.b[i] = g.b[i] - s;
}

// Y = L^-1 U^T: workgroup j (one wave) substitutes row j of U forward through the band factor, block row by block row, from the first
// node block the row touches (everything above it is zero).  The last 239 entries are all a row needs: they live in an LDS ring.
// Per block row the 64 lanes share the 12 dot products with the earlier entries (lane l takes d = r + 1 + l, + 64, ...; xor tree), then
// every lane solves the 12 x 12 triangle (staged in LDS) for itself.
__global__ void __launch_bounds__(64) deform_rel_y_kernel(DeformGraph g, DeformRel rel, int n)
{
    constexpr int V = kDeformVars, BW = kDeformBand, kRing = 256;
    __shared__ double win[kRing];
    __shared__ double tri[V][V + 1];
    if (g.out->failed) return;   // (the same value in every thread)
    const int col = (int)blockIdx.x, p = col / 3, c = col - 3 * p, lane = (int)threadIdx.x;
    double* __restrict__ Y = rel.Y + (size_t)col * (V * kDeformMaxNodes);
    const double* __restrict__ AB = g.AB;
    const int* uid = rel.uid + (size_t)p * kDeformRelSlots;
    const double* uval = rel.uval + (size_t)p * kDeformRelSlots * 4;
    int first = n;
    for (int s = 0; s < kDeformRelSlots; s++) { const int id = uid[s]; first = id >= 0 && id < first ? id : first; }
    for (int i = lane; i < V * first; i += 64) Y[i] = 0.0;
    for (int i = lane; i < kRing; i += 64) win[i] = 0.0;
    __syncthreads();
    for (int I = first; I < n; I++) {
        const int c0 = V * I;
        int slot = -1;
        for (int s = 0; s < kDeformRelSlots; s++) slot = uid[s] == I ? s : slot;
        // every load of the block row is issued before the first use: the row is bound by memory latency, not by arithmetic
        double tl[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {   // the diagonal block of L, entry (r, k <= r) by lane 12 r + k - 64 q
            const int e = lane + 64 * q, r = e / V, k = e - V * r;
            tl[q] = e < V * V && k <= r ? AB[(size_t)(c0 + r) * BW + (r - k)] : 0.0;
        }
        double lv[V][4];
#pragma unroll
        for (int r = 0; r < V; r++) {
            const int i = c0 + r;
            const int dmax = min(i - V * first, r + (BW - V));   // the block band: row r of a block holds L back to offset r + 228
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int d = r + 1 + lane + 64 * q;
                lv[r][q] = d <= dmax ? AB[(size_t)i * BW + d] : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int e = lane + 64 * q;
            if (e < V * V) tri[e / V][e % V] = tl[q];
        }
        double acc[V];
#pragma unroll
        for (int r = 0; r < V; r++) {
            const int i = c0 + r;
            const int dmax = min(i - V * first, r + (BW - V));   // the block band: row r of a block holds L back to offset r + 228
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {   // (d ascending, as a loop over d = r + 1 + lane, + 64, .. <= dmax sums)
                const int d = r + 1 + lane + 64 * q;
                if (d <= dmax) s = s + lv[r][q] * win[(i - d) & (kRing - 1)];
            }
            for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
            acc[r] = s;
        }
        __syncthreads();   // (the diagonal block is in LDS)
        double y[V];
#pragma unroll
        for (int r = 0; r < V; r++) {
            double v = slot >= 0 && rel_comp(r) == c ? uval[4 * slot + rel_quad(r)] : 0.0;
            v = v - acc[r];
#pragma unroll
            for (int k = 0; k < r; k++) v = v - tri[r][k] * y[k];
            y[r] = v / tri[r][r];
        }
        __syncthreads();   // (every lane has read the ring and the diagonal block for this block row)
#pragma unroll
        for (int r = 0; r < V; r++)
            if (lane == r) { win[(c0 + r) & (kRing - 1)] = y[r]; Y[c0 + r] = y[r]; }
        __syncthreads();
    }
}

// G[a][b] = v_a . v_b for b <= a over the vectors v_0 .. v_{m-1} = the rows of Y and v_m = y (g.b): C = I + G in rows 0 .. m-1, Y^T y in
// row m.  One workgroup per 16 x 16 tile of the lower triangle, 64 entries of the 32 vectors staged in LDS at a time; every entry is
// summed by ONE thread over i ascending.  The sum is compensated -- each product with its rounding error (fma), each addition with
// its own (two-sum), the errors summed beside it and added once at the end: where B alone is soft along the pairs (a loop whose old
// end hangs on regularisation edges only) Y^T Y reaches 1e3 .. 1e7 and y - Y t cancels that many digits of whatever error C and Y^T y
// carry; a plain f64 sum here cost five times the error of the whole step.
__global__ void __launch_bounds__(256) deform_rel_gram_kernel(DeformGraph g, DeformRel rel, int n, int m)
{
    constexpr int T = 16, CH = 64;
    __shared__ double A[T][CH + 1], B[T][CH + 1];
    if (g.out->failed) return;
    const int bi = (int)blockIdx.y, bj = (int)blockIdx.x;
    if (bj > bi) return;
    const int t = (int)threadIdx.x, ty = t / T, tx = t % T, nv = kDeformVars * n;
    const size_t ldy = (size_t)kDeformVars * kDeformMaxNodes;
    double acc = 0.0, low = 0.0;
    for (int i0 = 0; i0 < nv; i0 += CH) {
        for (int e = t; e < T * CH; e += 256) {
            const int row = e / CH, ii = e - row * CH, i = i0 + ii, a = T * bi + row, b = T * bj + row;
            A[row][ii] = i < nv && a <= m ? (a == m ? g.b[i] : rel.Y[a * ldy + i]) : 0.0;
            B[row][ii] = i < nv && b < m ? rel.Y[b * ldy + i] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int ii = 0; ii < CH; ii++) {
            const double x = A[ty][ii], y = B[tx][ii];
            const double p = x * y, pe = fma(x, y, -p);
            const double s = acc + p, v = s - acc;
            low = low + (((acc - (s - v)) + (p - v)) + pe);
            acc = s;
        }
        __syncthreads();
    }
    const int a = T * bi + ty, b = T * bj + tx;
    if (a == b) {   // the identity joins the sum the same way
        const double s = acc + 1.0, v = s - acc;
        low = low + ((acc - (s - v)) + (1.0 - v));
        acc = s;
    }
    if (a <= m && b < m && b <= a) rel.C[(size_t)a * kDeformRelLd + b] = acc + low;
}

// C = Lc Lc^T by panels of 16 columns (the panel in LDS, the trailing matrix through L2: 384^2 doubles do not fit in LDS), then
// Lc w = Y^T y and Lc^T t = w by columns; t replaces row m.  C itself is kept (cf_deform_download_relative); the work is done on a copy.
// One workgroup of kSolveT threads.  A pivot <= 0 fails the step.
__global__ void __launch_bounds__(kSolveT) deform_rel_c_kernel(DeformGraph g, DeformRel rel, int m)
{
    constexpr int W = 16, LD = kDeformRelLd;
    __shared__ double P[3 * kDeformRelMax][W + 1];
    __shared__ double tv[3 * kDeformRelMax];
    if (g.out->failed) return;
    const int t = (int)threadIdx.x;
    double* L = rel.Lc;   // (workgroup-shared through the barriers: not restrict)
    for (int e = t; e < (m + 1) * m; e += kSolveT) {
        const int i = e / m, j = e - i * m;
        if (j <= i) L[(size_t)i * LD + j] = rel.C[(size_t)i * LD + j];
    }
    __syncthreads();
    for (int c0 = 0; c0 < m; c0 += W) {
        const int rows = m - c0, w = rows < W ? rows : W;
        for (int e = t; e < rows * W; e += kSolveT) {
            const int ri = e / W, c = e - ri * W;
            P[ri][c] = c < w && ri >= c ? L[(size_t)(c0 + ri) * LD + c0 + c] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < w; c++) {
            const double piv = P[c][c];
            if (!(piv > 0.0)) {   // (the same value in every thread: the whole workgroup leaves)
                if (t == 0) { g.out->failed = 1; g.out->delta_norm = 0.0; }
                return;
            }
            const double l = sqrt(piv);
            __syncthreads();
            for (int ri = c + t; ri < rows; ri += kSolveT) P[ri][c] = ri == c ? l : P[ri][c] / l;
            __syncthreads();
            const int wr = w - 1 - c;   // columns c+1 .. w-1
            for (int e = t; e < (rows - c - 1) * wr; e += kSolveT) {
                const int ri = c + 1 + e / wr, cc = c + 1 + e % wr;
                if (ri >= cc) P[ri][cc] = P[ri][cc] - P[ri][c] * P[cc][c];
            }
            __syncthreads();
        }
        for (int e = t; e < rows * W; e += kSolveT) {
            const int ri = e / W, c = e - ri * W;
            if (c < w && ri >= c) L[(size_t)(c0 + ri) * LD + c0 + c] = P[ri][c];
        }
        const int mr = rows - w;   // the trailing matrix: rows and columns c0 + w .. m - 1
        for (int e = t; e < mr * mr; e += kSolveT) {
            const int i = w + e / mr, j = w + e % mr;
            if (j > i) continue;
            const size_t at = (size_t)(c0 + i) * LD + c0 + j;
            double v = L[at];
            for (int c = 0; c < w; c++) v = v - P[i][c] * P[j][c];
            L[at] = v;
        }
        __syncthreads();
    }
    for (int i = t; i < m; i += kSolveT) tv[i] = L[(size_t)m * LD + i];
    __syncthreads();
    for (int j = 0; j < m; j++) {
        if (t == 0) tv[j] = tv[j] / L[(size_t)j * LD + j];
        __syncthreads();
        for (int i = j + 1 + t; i < m; i += kSolveT) tv[i] = tv[i] - L[(size_t)i * LD + j] * tv[j];
        __syncthreads();
    }
    for (int j = m - 1; j >= 0; j--) {
        if (t == 0) tv[j] = tv[j] / L[(size_t)j * LD + j];
        __syncthreads();
        for (int i = t; i < j; i += kSolveT) tv[i] = tv[i] - L[(size_t)j * LD + i] * tv[j];
        __syncthreads();
    }
    for (int i = t; i < m; i += kSolveT) L[(size_t)m * LD + i] = tv[i];
}

// b <- y - Y t, one thread per unknown, the sum over the rows of U ascending
__global__ void __launch_bounds__(kDB) deform_rel_correct_kernel(DeformGraph g, DeformRel rel, int n, int m)
{
    if (g.out->failed) return;
    const int i = (int)(blockIdx.x * kDB + threadIdx.x);
    if (i >= kDeformVars * n) return;
    const size_t ldy = (size_t)kDeformVars * kDeformMaxNodes;
    const double* __restrict__ tv = rel.Lc + (size_t)m * kDeformRelLd;
    double s = 0.0;
    for (int j = 0; j < m; j++) s = s + rel.Y[j * ldy + i] * tv[j];
    g.b[i] = g.b[i] - s;
}

// what an accepted local closure leaves (CoFusion.cpp:445-458): lane k takes constraint k s of n, s = max(1, n / 3) (the reference's
// i += n / 3 never ends for n < 3), moves its source by the closure's graph as the map pass would and writes the pair into the ring
__global__ void __launch_bounds__(64) deform_rel_pick_kernel(DeformGraph from, int n_nodes, int local_time, const float* __restrict__ src,
                                                             const float* __restrict__ dst, const float* __restrict__ time,
                                                             const float* __restrict__ dst_time, int n, int row_stride, DeformRel rel, int head)
{
    const int k = (int)threadIdx.x, step = n / 3 > 1 ? n / 3 : 1;
    if ((long long)k * step >= n) return;
    const int idx = k * step;
    const size_t row = (size_t)idx * row_stride;
    f3 p = f3{src[3 * row], src[3 * row + 1], src[3 * row + 2]};
    const float tm = time[row];
    int ids[4]; float w[4];
    if (window_weights(from.nodes, n_nodes, p, (int)tm, ids, w) &&
        ((int)from.nodes[ids[0]].w > local_time || (int)from.nodes[ids[1]].w > local_time || (int)from.nodes[ids[2]].w > local_time ||
         (int)from.nodes[ids[3]].w > local_time))
        p = move_point(from.nodes, from.params, p, ids, w);
    const int slot = (head + k) % rel.capacity;
    rel.src[slot] = make_float4(p.x, p.y, p.z, tm);
    rel.dst[slot] = make_float4(dst[3 * row], dst[3 * row + 1], dst[3 * row + 2], dst_time[idx]);
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_deform_rel_weights(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel)
{
    if (n_rel <= 0) return;
    DeformGraph a = g, b = g;   // the window rule over the ring: the sources at srcTime, the targets at dstTime
    a.cons_src = rel.src; a.ids = rel.ids; a.w = rel.w;
    b.cons_src = rel.dst; b.ids = rel.ids + rel.capacity; b.w = rel.w + rel.capacity;
    launch_deform_weights(s, a, n, n_rel);
    launch_deform_weights(s, b, n, n_rel);
    hipLaunchKernelGGL(deform_rel_rows_kernel, dim3(1), dim3(kDeformRelMax), 0, s, g, rel, n_rel);
}
void launch_deform_residual_rel(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_cons, int n_rel)
{
    hipLaunchKernelGGL(deform_residual_kernel<true>, dim3(1), dim3(kSolveT), 0, s, g, n, n_cons, kDeformAllEnabled, rel, n_rel);
}
void launch_deform_rel_rhs(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_cons, int n_rel)
{
    hipLaunchKernelGGL(deform_rel_rhs_kernel, dim3((kDeformVars * n + kDB - 1) / kDB), dim3(kDB), 0, s, g, rel, n, n_cons, n_rel);
}
void launch_deform_solve_factor(hipStream_t s, const DeformGraph& g, int n)
{
    hipLaunchKernelGGL(deform_solve_kernel<1>, dim3(1), dim3(kSolveT), 0, s, g, n);
}
void launch_deform_rel_y(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel)
{
    hipLaunchKernelGGL(deform_rel_y_kernel, dim3(3 * n_rel), dim3(64), 0, s, g, rel, n);
}
void launch_deform_rel_gram(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel)
{
    const int tiles = (3 * n_rel + 1 + 15) / 16;
    hipLaunchKernelGGL(deform_rel_gram_kernel, dim3(tiles, tiles), dim3(256), 0, s, g, rel, n, 3 * n_rel);
}
void launch_deform_rel_c(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n_rel)
{
    hipLaunchKernelGGL(deform_rel_c_kernel, dim3(1), dim3(kSolveT), 0, s, g, rel, 3 * n_rel);
}
void launch_deform_rel_correct(hipStream_t s, const DeformGraph& g, const DeformRel& rel, int n, int n_rel)
{
    hipLaunchKernelGGL(deform_rel_correct_kernel, dim3((kDeformVars * n + kDB - 1) / kDB), dim3(kDB), 0, s, g, rel, n, 3 * n_rel);
}
void launch_deform_solve_finish(hipStream_t s, const DeformGraph& g, int n)
{
    hipLaunchKernelGGL(deform_solve_kernel<2>, dim3(1), dim3(kSolveT), 0, s, g, n);
}
void launch_deform_rel_pick(hipStream_t s, const DeformGraph& from, int n_nodes, int local_time, const float* src, const float* dst, const float* time,
                            const float* dst_time, int n_cons, int row_stride, const DeformRel& rel, int head)
{
    if (n_cons > 0) hipLaunchKernelGGL(deform_rel_pick_kernel, dim3(1), dim3(64), 0, s, from, n_nodes, local_time, src, dst, time, dst_time, n_cons, row_stride, rel, head);
}
void launch_deform_sample(hipStream_t s, const float* map, unsigned count, unsigned stride, const DeformGraph& g, DeformMeta* meta)
{
    hipLaunchKernelGGL(deform_sample_kernel, dim3(1), dim3(kDeformMaxNodes), 0, s, reinterpret_cast<const float4*>(map), count, stride, g, meta);
}
void launch_deform_init_graph(hipStream_t s, const DeformGraph& g, int n, bool identity)
{
    hipLaunchKernelGGL(deform_init_graph_kernel, dim3(1), dim3(kDeformMaxNodes), 0, s, g, n, identity ? 1 : 0);
}
void launch_deform_weights(hipStream_t s, const DeformGraph& g, int n, int n_cons)
{
    if (n_cons > 0) hipLaunchKernelGGL(deform_weights_kernel, dim3((n_cons + kDeformMaxCons - 1) / kDeformMaxCons), dim3(kDeformMaxCons), 0, s, g, n, n_cons);
}
void launch_deform_residual(hipStream_t s, const DeformGraph& g, int n, int n_cons, int last_deform_time)
{
    hipLaunchKernelGGL(deform_residual_kernel<false>, dim3(1), dim3(kSolveT), 0, s, g, n, n_cons, last_deform_time, DeformRel{}, 0);
}
void launch_deform_assemble(hipStream_t s, const DeformGraph& g, int n, int n_cons, int last_deform_time)
{
    hipLaunchKernelGGL(deform_assemble_kernel, dim3(n * (kDeformBand / kDeformVars)), dim3(192), 0, s, g, n, n_cons, last_deform_time);
}
void launch_deform_solve(hipStream_t s, const DeformGraph& g, int n)
{
    hipLaunchKernelGGL(deform_solve_kernel<0>, dim3(1), dim3(kSolveT), 0, s, g, n);
}
void launch_deform_apply(hipStream_t s, const DeformGraph& g, int n, float* map, unsigned count, const DeformReactivate* re, int last_deform_time)
{
    if (!count) return;
    unsigned blocks = (count + kDB - 1) / kDB;
    blocks = blocks > 1024 ? 1024 : blocks;   // every workgroup stages the nodes (16 KB) once
    if (re) hipLaunchKernelGGL(deform_apply_kernel<true>, dim3(blocks), dim3(kDB), 0, s, g, n, reinterpret_cast<float4*>(map), count, *re, last_deform_time);
    else hipLaunchKernelGGL(deform_apply_kernel<false>, dim3(blocks), dim3(kDB), 0, s, g, n, reinterpret_cast<float4*>(map), count, DeformReactivate{}, last_deform_time);
}
void launch_deform_poses(hipStream_t s, const DeformGraph& g, int n, float* poses, const int* times, int n_poses)
{
    if (n_poses > 0) hipLaunchKernelGGL(deform_poses_kernel, dim3((n_poses + kDB - 1) / kDB), dim3(kDB), 0, s, g, n, poses, times, n_poses);
}

}  // namespace cf
