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
__global__ void __launch_bounds__(kSolveT) deform_residual_kernel(DeformGraph g, int n, int n_cons, int ldt)
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
    const int rows = 18 * n + 3 * n_cons;
    double s = 0.0;
    for (int i = t; i < rows; i += kSolveT) { const double v = g.r[i]; s = s + v * v; }
    const double e = block_sum(s, red);
    if (t == 0) {
        float m = 0.f;
        for (int l = 0; l < n_cons; l++) m = m + norms[l];
        g.out->error = (float)e;
        g.out->mean_cons_error = m / (float)n_cons;
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
__global__ void __launch_bounds__(kSolveT) deform_solve_kernel(DeformGraph g, int n)
{
    constexpr int V = kDeformVars, BW = kDeformBand;
    __shared__ double P[BW][V + 1];   // the panel: rows c0 .. c0 + 239 of block column c0 .. c0 + 11
    __shared__ double y[V];
    __shared__ double red[kSolveT];
    const int t = (int)threadIdx.x;
    const int nv = V * n;
    double* AB = g.AB; double* b = g.b;   // (workgroup-shared through the barriers: not restrict)
    for (int c0 = 0; c0 < nv; c0 += V) {
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

// ------------------------------------------------------------------------------------------------ launchers
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
    hipLaunchKernelGGL(deform_residual_kernel, dim3(1), dim3(kSolveT), 0, s, g, n, n_cons, last_deform_time);
}
void launch_deform_assemble(hipStream_t s, const DeformGraph& g, int n, int n_cons, int last_deform_time)
{
    hipLaunchKernelGGL(deform_assemble_kernel, dim3(n * (kDeformBand / kDeformVars)), dim3(192), 0, s, g, n, n_cons, last_deform_time);
}
void launch_deform_solve(hipStream_t s, const DeformGraph& g, int n)
{
    hipLaunchKernelGGL(deform_solve_kernel, dim3(1), dim3(kSolveT), 0, s, g, n);
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
