// frontier_kernels.hip -- ranked frontier rows for the host-checked planner (device side).
//
// For every node row a of every graph: the live cells P[a, b] of the row, sorted by score descending, ties by source id
// ascending (include/gnnmp.h: gnnmp_frontier_rank).  The host loop (planner.greedy_expand_ranked) then only touches the cells
// it actually tries.  Three launches behind one memset, all on the caller's stream:
//
//   fr_stage       one 1024-thread workgroup per graph: target histogram (LDS up to kFrLdsRows nodes, global atomics beyond),
//                  block scan -> row_beg (the by-target CSR position), scatter of (source, score, column) into the staging arrays
//                  by arrival rank.  The arrival order inside a row differs from run to run; nothing below depends on it.
//   fr_rank_wave   one wave per row of at most kFrWaveCells cells, the row in LDS: every cell decides "dead" (score 0, self loop,
//                  collided end -- folded into a zero score by fr_stage -- or a later column names the same source), then counts
//                  the live cells that precede it and is written at row_beg + rank.
//   fr_rank_block  longer rows (listed by fr_stage): a 1024-thread workgroup streams the row through LDS tiles of
//                  kFrTileCells cells, once to find the duplicates and once to rank.
//
// The rank of a live cell is a function of the row's SET of cells only, so the output is bit-identical from run to run.
// A NaN score compares false with everything: ranks may then collide inside the row's own range (never outside it), nothing loops.
#include <hip/hip_runtime.h>

#include <climits>

#include "kernels.hpp"

namespace gnnmp {
namespace {

constexpr int kFrThreads = 1024;
constexpr int kFrLdsRows = 8192;                      // nodes per graph whose histogram fits the 32 KB LDS table
constexpr int kFrWavePer = kFrWaveCells / 64;         // cells per lane on the wave path
constexpr int kFrErrIndex = -8;                       // GNNMP_ERR_INDEX

// exclusive scan of one int per thread over the 1024-thread block; `wsum` is 16 ints of LDS
__device__ __forceinline__ int fr_block_scan(int x, int* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < w; ++i) base += wsum[i];
    __syncthreads();
    return base + inc - x;
}

template <bool kLds>
__device__ __forceinline__ int fr_ld(const int* p) {
    if (kLds) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // counters that atomics wrote: read them at L2
}
template <bool kLds>
__device__ __forceinline__ void fr_st(int* p, int x) {
    if (kLds) *p = x;
    else __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one graph: nodes [n0, n0 + N), columns [e0, e0 + E); cnt = N counters, zero on entry (global) or zeroed here (LDS)
template <bool kLds>
__device__ __forceinline__ void fr_stage_graph(const FrontierParams& p, int g, int n0, int N, int e0, int E, int* cnt, int* wsum,
                                               int* bad) {
    const int tid = threadIdx.x;
    if (kLds)
        for (int i = tid; i < N; i += kFrThreads) cnt[i] = 0;
    __syncthreads();
    const long long* src = p.edge_index + e0;
    const long long* dst = p.edge_index + (long long)p.total_edges + e0;
    bool mybad = false;
    for (int e = tid; e < E; e += kFrThreads) {
        const unsigned long long a = (unsigned long long)dst[e], b = (unsigned long long)src[e];
        if (a >= (unsigned long long)N || b >= (unsigned long long)N) mybad = true;      // dropped: never an address
        else atomicAdd(&cnt[(int)a], 1);
    }
    if (mybad) *bad = 1;
    __syncthreads();
    // rows of this thread: a contiguous chunk, so the scan is one value per thread
    const int chunk = (N + kFrThreads - 1) / kFrThreads;
    const long long lo = (long long)tid * chunk;
    const int i0 = lo < N ? (int)lo : N, i1 = (lo + chunk) < N ? (int)(lo + chunk) : N;
    int s = 0;
    for (int i = i0; i < i1; ++i) s += fr_ld<kLds>(&cnt[i]);
    int run = e0 + fr_block_scan(s, wsum);
    for (int i = i0; i < i1; ++i) {
        const int d = fr_ld<kLds>(&cnt[i]);
        fr_st<kLds>(&cnt[i], run);                   // from here on the row's write cursor
        p.row_beg[n0 + i] = run;
        p.deg[n0 + i] = d;
        if (d > kFrWaveCells) p.long_list[atomicAdd(p.long_cnt, 1)] = n0 + i;      // (list order is free: rows are independent)
        run += d;
    }
    __syncthreads();
    const int nf = p.n_free[g];
    for (int e = tid; e < E; e += kFrThreads) {
        const unsigned long long a = (unsigned long long)dst[e], b = (unsigned long long)src[e];
        if (a >= (unsigned long long)N || b >= (unsigned long long)N) continue;
        const int pos = atomicAdd(&cnt[(int)a], 1);                                 // inside [e0, e0 + E): same predicate as the count
        // what the cell's own value decides is folded into a zero score: self loop, collided end
        const bool off = a == b || (long long)a >= nf || (long long)b >= nf;
        p.st_b[pos] = (int)b;
        p.st_v[pos] = off ? 0.0f : p.scores[e0 + e];
        p.st_e[pos] = e;
    }
    __syncthreads();
    if (tid == 0) p.status[g] = *bad ? kFrErrIndex : 0;                             // one owner, no atomics
}

__global__ __launch_bounds__(kFrThreads) void fr_stage(FrontierParams p) {
    __shared__ int lds_cnt[kFrLdsRows];
    __shared__ int wsum[16];
    __shared__ int bad;
    const int g = blockIdx.x;
    // prefix arrays are clamped into the batch: a wrong one can flag its graph, never address outside the buffers
    long long n0 = p.node_ptr ? p.node_ptr[g] : 0, n1 = p.node_ptr ? p.node_ptr[g + 1] : p.total_nodes;
    long long e0 = p.edge_ptr ? p.edge_ptr[g] : 0, e1 = p.edge_ptr ? p.edge_ptr[g + 1] : p.total_edges;
    const bool ok = n0 >= 0 && n0 <= n1 && n1 <= p.total_nodes && e0 >= 0 && e0 <= e1 && e1 <= p.total_edges;
    if (threadIdx.x == 0) bad = ok ? 0 : 1;
    if (!ok) n0 = n1 = e0 = e1 = 0;
    const int N = (int)(n1 - n0), E = (int)(e1 - e0);
    if (N <= kFrLdsRows) fr_stage_graph<true>(p, g, (int)n0, N, (int)e0, E, lds_cnt, wsum, &bad);
    else fr_stage_graph<false>(p, g, (int)n0, N, (int)e0, E, p.cnt + n0, wsum, &bad);
}

// j precedes c in the ranked row
__device__ __forceinline__ bool fr_before(float vj, int bj, float vc, int bc) { return vj > vc || (vj == vc && bj < bc); }

__global__ __launch_bounds__(64) void fr_rank_wave(FrontierParams p) {
    __shared__ int sb[kFrWaveCells];
    __shared__ float sv[kFrWaveCells];
    __shared__ int se[kFrWaveCells];
    const int node = blockIdx.x, lane = threadIdx.x;
    const int L = p.deg[node];
    if (L > kFrWaveCells) return;                    // fr_rank_block's
    if (L == 0) {
        if (lane == 0) p.row_len[node] = 0;
        return;
    }
    const int beg = p.row_beg[node];
    int mb[kFrWavePer], me[kFrWavePer];
    float mv[kFrWavePer];
    bool dead[kFrWavePer];
#pragma unroll
    for (int k = 0; k < kFrWavePer; ++k) {
        const int c = lane + 64 * k;
        mb[k] = INT_MAX; me[k] = INT_MAX; mv[k] = 0.0f;
        if (c < L) {
            mb[k] = p.st_b[beg + c]; mv[k] = p.st_v[beg + c]; me[k] = p.st_e[beg + c];
            sb[c] = mb[k]; se[c] = me[k];
        }
        dead[k] = mv[k] == 0.0f;                     // +0 and -0; slots beyond the row are dead too
    }
    __syncthreads();
    for (int j = 0; j < L; ++j) {                    // the highest column naming a source decides it
        const int bj = sb[j], ej = se[j];
#pragma unroll
        for (int k = 0; k < kFrWavePer; ++k) dead[k] = dead[k] || (bj == mb[k] && ej > me[k]);
    }
    __syncthreads();
    int n_live = 0;
#pragma unroll
    for (int k = 0; k < kFrWavePer; ++k) {
        const int c = lane + 64 * k;
        if (c < L) {                                 // a dead cell precedes nothing
            sv[c] = dead[k] ? -__builtin_huge_valf() : mv[k];
            if (dead[k]) sb[c] = INT_MAX;
        }
        n_live += __popcll(__ballot(!dead[k]));
    }
    __syncthreads();
    int rank[kFrWavePer];
#pragma unroll
    for (int k = 0; k < kFrWavePer; ++k) rank[k] = 0;
    for (int j = 0; j < L; ++j) {
        const float vj = sv[j];
        const int bj = sb[j];
#pragma unroll
        for (int k = 0; k < kFrWavePer; ++k) rank[k] += fr_before(vj, bj, mv[k], mb[k]) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < kFrWavePer; ++k)
        if (!dead[k]) {                              // rank < number of live cells <= L
            p.cols[beg + rank[k]] = mb[k];
            p.vals[beg + rank[k]] = mv[k];
        }
    if (lane == 0) p.row_len[node] = n_live;
}

__global__ __launch_bounds__(kFrThreads) void fr_rank_block(FrontierParams p) {
    __shared__ int tb[kFrTileCells];
    __shared__ int te[kFrTileCells];                 // pass 1: columns; pass 2: the scores' bits
    __shared__ int wsum[16];
    const int tid = threadIdx.x;
    const int n_long = *p.long_cnt;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int node = p.long_list[r];
        const int L = p.deg[node], beg = p.row_beg[node];
        // pass 1: a cell that a later column overrides gets a zero score in the staging array (each thread writes its own
        // cells; this pass reads sources and columns only)
        for (int c0 = 0; c0 < L; c0 += kFrThreads) {
            const int c = c0 + tid;
            const bool act = c < L;
            const int mb = act ? p.st_b[beg + c] : INT_MAX, me = act ? p.st_e[beg + c] : INT_MAX;
            bool over = false;
            for (int t0 = 0; t0 < L; t0 += kFrTileCells) {
                const int n = L - t0 < kFrTileCells ? L - t0 : kFrTileCells;
                __syncthreads();
                for (int j = tid; j < n; j += kFrThreads) { tb[j] = p.st_b[beg + t0 + j]; te[j] = p.st_e[beg + t0 + j]; }
                __syncthreads();
                for (int j = 0; j < n; ++j) over = over || (tb[j] == mb && te[j] > me);
            }
            if (act && over) p.st_v[beg + c] = 0.0f;
        }
        __threadfence_block();
        __syncthreads();
        // pass 2: rank among the live cells
        int n_live = 0;
        for (int c0 = 0; c0 < L; c0 += kFrThreads) {
            const int c = c0 + tid;
            const bool act = c < L;
            const int mb = act ? p.st_b[beg + c] : INT_MAX;
            const float mv = act ? p.st_v[beg + c] : 0.0f;
            const bool live = mv != 0.0f;
            int rank = 0;
            for (int t0 = 0; t0 < L; t0 += kFrTileCells) {
                const int n = L - t0 < kFrTileCells ? L - t0 : kFrTileCells;
                __syncthreads();
                for (int j = tid; j < n; j += kFrThreads) {
                    const float vj = p.st_v[beg + t0 + j];
                    const bool lj = vj != 0.0f;          // a dead cell precedes nothing
                    tb[j] = lj ? p.st_b[beg + t0 + j] : INT_MAX;
                    te[j] = __float_as_int(lj ? vj : -__builtin_huge_valf());
                }
                __syncthreads();
                for (int j = 0; j < n; ++j) rank += fr_before(__int_as_float(te[j]), tb[j], mv, mb) ? 1 : 0;
            }
            if (live) {                              // rank < number of live cells <= L
                p.cols[beg + rank] = mb;
                p.vals[beg + rank] = mv;
                ++n_live;
            }
        }
        const int before = fr_block_scan(n_live, wsum);
        if (tid == kFrThreads - 1) p.row_len[node] = before + n_live;
    }
}

}  // namespace

hipError_t launch_frontier_rank(const FrontierParams& p, hipStream_t st) {
    hipLaunchKernelGGL(fr_stage, dim3(p.G), dim3(kFrThreads), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.total_nodes == 0) return e;
    hipLaunchKernelGGL(fr_rank_wave, dim3(p.total_nodes), dim3(64), 0, st, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // rows beyond the wave path are rare in a kNN graph (mean in-degree ~2 k1): a fixed grid walks fr_stage's list
    const long long cap = (long long)p.total_edges / (kFrWaveCells + 1);          // how many such rows there can be
    if (cap > 0) {
        hipLaunchKernelGGL(fr_rank_block, dim3((unsigned)(cap < 128 ? cap : 128)), dim3(kFrThreads), 0, st, p);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace gnnmp
