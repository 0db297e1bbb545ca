// csr_cheb: one step of a Chebyshev three-term recurrence on a block of columns, in one pass over a square CSR:
//     S_i       = sum over row i's entries e of y[col[e], :]
//     out[i, :] = fma(a, S_i, fma(b, y[i, :], g * x[i, :]))          x given
//     out[i, :] = fma(a, S_i, b * y[i, :])                            x == NULL
// The A.X product behind ops.eigen_top (the top eigenvectors of a symmetric graph: the reference's `eigen_decomposition` initializer,
// model.py:163-180, a dense LA.eig there).  A run spends 100-300 such products on a block of 100-130 columns; the composed form --
// sage_csr_sum, which plans on every call and gives a row a whole wave, plus two or three element-wise passes over [N, dim] -- is
// what this file replaces.
//
// ORDER OF A ROW'S SUM: the bits of sage_csr_sum.  Column c of S_i is 0 + t_0 + t_1 + ... over the row's entries in stored order
// for a row of at most SAGE_CSR_MEAN_CHUNK entries; a longer row is cut into chunks of that many by the shared planner
// (sage_csr_common.h: csr_chunk_plan), p_c = 0 + the chunk's terms in stored order, S_i = 0 + p_0 + p_1 + ... in chunk order.  The rule
// is chunked_row_sum's (the one copy of it); the terms are walked by sum_edges where a row has a whole wave and by group_terms below
// -- sum_edges' loop on a part of a wave -- where it has less.  A column's additions are sequential, so which lane holds a column,
// how many lanes a row has and how many rows are in flight change no bit.  out[i, :] depends on row i's entries, y, x[i, :] and
// the three scalars alone.
//
// LANES PER ROW.  A lane holds VEC = 4 consecutive columns (16-byte accesses; VEC = 1 when dim, a leading dimension or a pointer
// does not allow them).  A row belongs to a GROUP of 16, 32 or 64 lanes, the smallest that holds ceil(dim / VEC) lanes: at dim = 100
// 25 of 32 lanes work where a wave per row keeps 25 of 64 busy, and a wave holds 4, 2 or 1 rows.  More than 64 lanes' worth of
// columns (256 on the vector path) loop over column blocks.  A trip of a group reads up to G ids (one per lane), hands them round
// by shuffles inside the group and keeps 8 gathered rows in flight before the first add; the adds follow in stored order.
//
// PLAN.  sage_csr_cheb_plan runs the planner's count, carry, expand ONCE per graph; every step reads off[] / item_row[] from the
// workspace (as sage_pagerank_step does), sums the long rows' chunks into the planned partials and then walks all rows.  A
// workspace that no plan filled for this rowptr gives wrong numbers, never an access out of range: chunk_item refuses an item
// that names no row, a first item outside [0, cap] counts as "no room" (the row is then summed in place), every id from col is
// clamped into [0, N) and every row pointer into [0, rowptr[N]].
// No float atomics; every element of out is stored once, with a plain vector store.  out may be x (a lane reads its own elements
// of x before it stores them); out overlapping y is refused.
#include "sage_csr_common.h"

namespace {

constexpr int kChebThreads = 256;
constexpr int kChebInFlight = 8;                       // gathered rows of a trip in flight before the first add; never changes a bit
constexpr int32_t kChebMaxDim = 1 << 20;

struct ChebLayout {
    ChunkWs c;
    size_t total;
};

bool cheb_layout(int64_t num_nodes, int64_t num_edges, int32_t dim, ChebLayout* L) {
    if (num_nodes < 1 || num_nodes >= (1ll << 31) || num_edges < 0 || dim < 1 || dim > kChebMaxDim) return false;
    WsCursor cur;
    if (!chunk_ws(num_nodes, num_edges, dim, cur, &L->c)) return false;
    L->total = cur.off;
    return true;
}

// acc += rows y[col[b..e)] in stored order, for a GROUP of G < 64 lanes (gl = the lane's place in it; b, e the same in the
// group's lanes): sum_edges' loop with the ids handed round by shuffles inside the group instead of readlane over the wave.
template <int VEC, int G>
__device__ inline void group_terms(const int32_t* __restrict__ col, int64_t b, int64_t e, const float* __restrict__ y, int64_t ld,
                                   int last_row, int c0, bool ok, int gl, typename VecT<VEC>::type& acc) {
    using V = typename VecT<VEC>::type;
    for (int64_t base = b; base < e; base += G) {
        const int m = (int)min((int64_t)G, e - base);
        const int raw = gl < m ? col[base + gl] : 0;
        const int myid = min(max(raw, 0), last_row);        // never read outside y
        for (int j0 = 0; j0 < m; j0 += kChebInFlight) {
            V t[kChebInFlight];
#pragma unroll
            for (int u = 0; u < kChebInFlight; ++u) {
                const int id = __shfl(myid, min(j0 + u, m - 1), G);
                if (ok) t[u] = *reinterpret_cast<const V*>(y + (int64_t)id * ld + c0);
                else vfill(t[u], 0.f);
            }
#pragma unroll
            for (int u = 0; u < kChebInFlight; ++u)
                if (j0 + u < m) vadd(acc, t[u]);
        }
    }
}

// The terms of entries [b, e): the shared walker where the row has the whole wave, the group's otherwise.
template <int VEC, int G>
__device__ inline void cheb_terms(const int32_t* __restrict__ col, int64_t b, int64_t e, const float* __restrict__ y, int64_t ld,
                                  int last_row, int c0, bool ok, int gl, typename VecT<VEC>::type& acc) {
    if constexpr (G == kWave) {
        bool unused = false;
        sum_edges<VEC, false, false>(col, b, e, y, ld, last_row, c0, ok, -1, acc, unused, nullptr, 0);
    } else {
        group_terms<VEC, G>(col, b, e, y, ld, last_row, c0, ok, gl, acc);
    }
}

__device__ inline float4 cheb_out(float a, const float4& s, float b, const float4& y, float g, const float4& x, bool hasx) {
    float4 r;
    r.x = __builtin_fmaf(a, s.x, hasx ? __builtin_fmaf(b, y.x, g * x.x) : b * y.x);
    r.y = __builtin_fmaf(a, s.y, hasx ? __builtin_fmaf(b, y.y, g * x.y) : b * y.y);
    r.z = __builtin_fmaf(a, s.z, hasx ? __builtin_fmaf(b, y.z, g * x.z) : b * y.z);
    r.w = __builtin_fmaf(a, s.w, hasx ? __builtin_fmaf(b, y.w, g * x.w) : b * y.w);
    return r;
}
__device__ inline float cheb_out(float a, const float& s, float b, const float& y, float g, const float& x, bool hasx) {
    return __builtin_fmaf(a, s, hasx ? __builtin_fmaf(b, y, g * x) : b * y);
}

// One group per item (row, chunk): partials[item] := 0 + the chunk's terms
template <int VEC, int G>
__global__ __launch_bounds__(kChebThreads) void cheb_chunk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                   int64_t num_nodes, const float* __restrict__ y, int64_t ldy, int dim,
                                                                   const int64_t* __restrict__ off, const int64_t* __restrict__ carry, int nb,
                                                                   int64_t cap, const int32_t* __restrict__ item_row,
                                                                   float* __restrict__ partials) {
    using V = typename VecT<VEC>::type;
    constexpr bool kUniform = G == kWave;
    const int gl = threadIdx.x % G;
    const int64_t group = ((int64_t)blockIdx.x * kChebThreads + threadIdx.x) / G;
    const int64_t ngroups = (int64_t)gridDim.x * (kChebThreads / G);
    const int n = (int)num_nodes;
    const int64_t items = min(carry[nb], cap);
    const int64_t total = rowptr[num_nodes];
    for (int64_t i = group; i < items; i += ngroups) {
        int32_t v;
        int64_t cb, ce;
        if (!chunk_item<kUniform>(i, item_row, rowptr, num_nodes, nullptr, n, total, off, cap, v, cb, ce)) continue;
        for (int cbk = 0; cbk < dim; cbk += G * VEC) {
            const int c0 = cbk + gl * VEC;
            const bool ok = c0 < dim;
            V acc;
            vfill(acc, 0.f);
            cheb_terms<VEC, G>(col, cb, ce, y, ldy, n - 1, c0, ok, gl, acc);
            if (ok) *reinterpret_cast<V*>(partials + i * dim + c0) = acc;
        }
    }
}

// One group per row.  x and out carry no __restrict__: they may be one array.
template <int VEC, int G, bool HASX>
__global__ __launch_bounds__(kChebThreads) void cheb_row_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 int64_t num_nodes, const float* __restrict__ y, int64_t ldy, const float* x,
                                                                 int64_t ldx, int dim, float a, float b, float g, float* out, int64_t ldo,
                                                                 const int64_t* __restrict__ off, int64_t cap,
                                                                 const float* __restrict__ partials) {
    using V = typename VecT<VEC>::type;
    constexpr bool kUniform = G == kWave;
    const int gl = threadIdx.x % G;
    const int64_t group = ((int64_t)blockIdx.x * kChebThreads + threadIdx.x) / G;
    const int64_t ngroups = (int64_t)gridDim.x * (kChebThreads / G);
    const int n = (int)num_nodes;
    const int64_t total = rowptr[num_nodes];
    for (int64_t r = group; r < n; r += ngroups) {
        int32_t v;
        int64_t rb, re;
        row_span<kUniform>(rowptr, num_nodes, nullptr, (int)r, total, v, rb, re);
        const int64_t k = long_chunks(re - rb);
        int64_t o = first_item<kUniform>(off, r, k);
        if (o < 0 || o > cap) o = cap;                       // no plan for this rowptr in the workspace: sum in place
        for (int cbk = 0; cbk < dim; cbk += G * VEC) {
            const int c0 = cbk + gl * VEC;
            const bool ok = c0 < dim;
            V yi, xi;
            vfill(yi, 0.f);
            vfill(xi, 0.f);
            if (ok) {
                yi = *reinterpret_cast<const V*>(y + r * ldy + c0);
                if constexpr (HASX) xi = *reinterpret_cast<const V*>(x + r * ldx + c0);
            }
            const V s = chunked_row_sum<V>(k, o, cap, partials, dim, c0, ok, rb, re, [&](int64_t tb, int64_t te, V& acc) {
                cheb_terms<VEC, G>(col, tb, te, y, ldy, n - 1, c0, ok, gl, acc);
            });
            if (ok) *reinterpret_cast<V*>(out + r * ldo + c0) = cheb_out(a, s, b, yi, g, xi, HASX);
        }
    }
}

struct ChebArgs {
    const int64_t* rowptr;
    const int32_t* col;
    int64_t num_nodes;
    const float* y;
    int64_t ldy;
    const float* x;
    int64_t ldx;
    int dim;
    float a, b, g;
    float* out;
    int64_t ldo;
    ChunkPlan P;
};

template <int VEC, int G>
int cheb_launch(const ChebArgs& A, hipStream_t st) {
    constexpr int kGroups = kChebThreads / G;
    if (A.P.cap > 0) {
        const int blocks = (int)std::min<int64_t>((A.P.cap + kGroups - 1) / kGroups, kNumCU * 8);
        hipLaunchKernelGGL((cheb_chunk_kernel<VEC, G>), dim3(blocks), dim3(kChebThreads), 0, st, A.rowptr, A.col, A.num_nodes, A.y, A.ldy, A.dim,
                           (const int64_t*)A.P.off, (const int64_t*)A.P.carry, A.P.nb, A.P.cap, (const int32_t*)A.P.item_row, A.P.partials);
        SAGE_CHECK_LAUNCH("cheb_chunk_kernel");
    }
    const int blocks = (int)std::min<int64_t>((A.num_nodes + kGroups - 1) / kGroups, kNumCU * 8);
    if (A.x)
        hipLaunchKernelGGL((cheb_row_kernel<VEC, G, true>), dim3(blocks), dim3(kChebThreads), 0, st, A.rowptr, A.col, A.num_nodes, A.y, A.ldy, A.x,
                           A.ldx, A.dim, A.a, A.b, A.g, A.out, A.ldo, (const int64_t*)A.P.off, A.P.cap, (const float*)A.P.partials);
    else
        hipLaunchKernelGGL((cheb_row_kernel<VEC, G, false>), dim3(blocks), dim3(kChebThreads), 0, st, A.rowptr, A.col, A.num_nodes, A.y, A.ldy, A.x,
                           A.ldx, A.dim, A.a, A.b, A.g, A.out, A.ldo, (const int64_t*)A.P.off, A.P.cap, (const float*)A.P.partials);
    SAGE_CHECK_LAUNCH("cheb_row_kernel");
    return SAGE_OK;
}

template <int VEC>
int cheb_launch_width(const ChebArgs& A, hipStream_t st) {
    const int lanes = (A.dim + VEC - 1) / VEC;             // the smallest group that holds the row's lanes
    if (lanes <= 16) return cheb_launch<VEC, 16>(A, st);
    if (lanes <= 32) return cheb_launch<VEC, 32>(A, st);
    return cheb_launch<VEC, 64>(A, st);
}

// Do [p, p + the bytes of rows x ld with dim used columns) and the same of q share a byte?
bool cheb_overlap(const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t rows, int32_t dim) {
    const uintptr_t pb = (uintptr_t)p, pe = pb + ((uintptr_t)(rows - 1) * (uintptr_t)ldp + (uintptr_t)dim) * sizeof(float);
    const uintptr_t qb = (uintptr_t)q, qe = qb + ((uintptr_t)(rows - 1) * (uintptr_t)ldq + (uintptr_t)dim) * sizeof(float);
    return pb < qe && qb < pe;
}

}  // namespace

extern "C" size_t sage_csr_cheb_workspace_bytes(int64_t num_nodes, int64_t num_edges, int32_t dim) {
    ChebLayout L;
    return cheb_layout(num_nodes, num_edges, dim, &L) ? L.total : 0;
}

extern "C" int sage_csr_cheb_plan(const int64_t* rowptr, int64_t num_nodes, int64_t num_edges, int32_t dim, void* workspace,
                                  size_t workspace_bytes, sage_stream_t stream) {
    SAGE_REQUIRE(num_nodes >= 1 && num_nodes < (1ll << 31), "csr_cheb_plan: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(num_edges >= 0, "csr_cheb_plan: num_edges = %lld", (long long)num_edges);
    SAGE_REQUIRE(dim >= 1 && dim <= kChebMaxDim, "csr_cheb_plan: dim = %d", dim);
    ChebLayout L;
    SAGE_REQUIRE(cheb_layout(num_nodes, num_edges, dim, &L), "csr_cheb_plan: num_nodes = %lld, num_edges = %lld, dim = %d out of range",
                 (long long)num_nodes, (long long)num_edges, dim);
    SAGE_REQUIRE(rowptr, "csr_cheb_plan: NULL array");
    if (const int rc = csr_workspace_check("csr_cheb_plan", workspace, workspace_bytes, L.total)) return rc;
    ChunkPlan P;
    return csr_chunk_plan(rowptr, num_nodes, nullptr, (int)num_nodes, workspace, L.c, (hipStream_t)stream, &P);
}

extern "C" int sage_csr_cheb_step(const int64_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t num_edges, const float* y, int64_t ldy,
                                  const float* x, int64_t ldx, int32_t dim, float a, float b, float g, float* out, int64_t ldo, void* workspace,
                                  size_t workspace_bytes, sage_stream_t stream) {
    // shapes first, then pointers, then the workspace: a bad shape is reported as such whatever the pointers are
    SAGE_REQUIRE(num_nodes >= 1 && num_nodes < (1ll << 31), "csr_cheb_step: num_nodes = %lld", (long long)num_nodes);
    SAGE_REQUIRE(num_edges >= 0, "csr_cheb_step: num_edges = %lld", (long long)num_edges);
    SAGE_REQUIRE(dim >= 1 && dim <= kChebMaxDim && ldy >= dim && ldo >= dim && (!x || ldx >= dim),
                 "csr_cheb_step: dim = %d, ldy = %lld, ldx = %lld, ldo = %lld", dim, (long long)ldy, (long long)ldx, (long long)ldo);
    ChebLayout L;
    SAGE_REQUIRE(cheb_layout(num_nodes, num_edges, dim, &L), "csr_cheb_step: num_nodes = %lld, num_edges = %lld, dim = %d out of range",
                 (long long)num_nodes, (long long)num_edges, dim);
    SAGE_REQUIRE(rowptr && col && y && out, "csr_cheb_step: NULL array");
    SAGE_REQUIRE(!cheb_overlap(out, ldo, y, ldy, num_nodes, dim), "csr_cheb_step: out overlaps y (every row gathers other rows of y)");
    SAGE_REQUIRE(!x || x == out || !cheb_overlap(out, ldo, x, ldx, num_nodes, dim),
                 "csr_cheb_step: out overlaps x without being x (out == x with ldo == ldx is the in-place form)");
    SAGE_REQUIRE(!x || x != out || ldx == ldo, "csr_cheb_step: out == x needs ldo == ldx, got %lld and %lld", (long long)ldo, (long long)ldx);
    if (const int rc = csr_workspace_check("csr_cheb_step", workspace, workspace_bytes, L.total)) return rc;
    char* ws = (char*)workspace;
    const ChebArgs A{rowptr, col, num_nodes, y, ldy, x, ldx, (int)dim, a, b, g, out, ldo,
                     ChunkPlan{(int64_t*)(ws + L.c.off), (int64_t*)(ws + L.c.carry), (int32_t*)(ws + L.c.item_row), (float*)(ws + L.c.partials), L.c.cap,
                               (int)L.c.nblocks}};
    const bool vec4 = (dim % 4 == 0) && (ldy % 4 == 0) && (ldo % 4 == 0) && (!x || ldx % 4 == 0) && sage_aligned(y, 16) && sage_aligned(out, 16) &&
                      (!x || sage_aligned(x, 16));
    return vec4 ? cheb_launch_width<4>(A, (hipStream_t)stream) : cheb_launch_width<1>(A, (hipStream_t)stream);
}
