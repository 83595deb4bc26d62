// lazysp_kernels.hip -- the LazySP baseline planner (algorithm/lazy_sp.py:147-196 over algorithm/dijkstra.py:34-76) for
// batches of maze problems, every problem on its own sample stream.  The host loops over rounds only:
//   lsp_sample_kernel   informed_sample (lazy_sp.py:78-103): `batch` more free draws appended to a float64 pool per problem,
//                       every draw through MazeEnv._state_fp with its collision checks counted;
//   lsp_gather_kernel   the round's float32 node rows, node_ptr, n_free (= N: every LazySP node is free) and k1 in the
//                       layout gnnmp_graph_build reads;
//   lsp_round_kernel    the round itself: carried pairs marked in the new graph, edge costs, then Dijkstra / walk the path /
//                       check its unknown edges / invalidate the first blocked one, until the path is valid or the start is
//                       unreachable.  One wave per problem; no wave ever waits on another workgroup.
// Node 0 is the GOAL and node 1 the START (lazy_sp.py:61).  All decisions are float64, one rounded operation at a time.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "maze_f64.hpp"

// numpy rounds every float64 operation on its own; the one fused chain is the dot product of np.linalg.norm (mz_cost)
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

// the counted float64 checker (mz_maze, mz_point, mz_segment, mz_edge2, mz_stick, mz_stick_edge_wave): maze_f64.hpp

// np.linalg.norm(t - s) with its fused dot product (mz_cost): maze_f64.hpp too; wave_sync, the wave reductions and
// lower_bound: wave64.hpp

// slot of edge (a -> b) in a's out-block, -1 when the graph has no such edge
__device__ __forceinline__ int lsp_slot(const long long* dst, const int* rb, int a, int b) {
    const int q = lower_bound(dst, rb[a], rb[a + 1], (long long)b);
    return q < rb[a + 1] && dst[q] == b ? q : -1;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// informed_sample: one wave per problem classifies its own draws [att_ptr[b], att_ptr[b + 1]) 64 at a time.  Pass 1 finds the
// n-th free draw and the checks of the draws up to it (a block that ends first leaves everything untouched: status 1);
// pass 2 classifies the consumed draws again and stores the free ones behind the pool's rows in draw order.
// ---------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(64) void lsp_sample_kernel(LspSampleParams p) {
    __shared__ unsigned char occ[kMzLdsCells];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (p.active && !p.active[b]) return;
    const long long a0 = p.att_ptr[b], Mb = p.att_ptr[b + 1] - a0;
    const int N0 = p.n_nodes[b];
    const int base = N0 == 0 ? 2 : N0;                           // round 1: goal and start come first
    if (N0 < 0 || N0 == 1 || (long long)base + p.n > (long long)p.cap + 2 || a0 < 0 || a0 + (Mb > 0 ? Mb : 0) > p.M) {
        if (lane == 0) { p.status[b] = 2; p.used[b] = 0; p.checks_out[b] = 0; }
        return;
    }
    const MzMaze m = mz_maze(p.maps + (size_t)b * p.w * p.w, p.w, occ, lane);
    const double* att = p.attempts + (size_t)a0 * DIM;
    auto classify = [&](long long idx, int& cnt) {
        if (DIM == 2) return mz_point(m, att[2 * idx], att[2 * idx + 1], cnt);
        return mz_stick(m, att[3 * idx], att[3 * idx + 1], att[3 * idx + 2], cnt);
    };
    int free_before = 0;
    long long checks = 0, used = -1;
    for (long long off = 0; off < Mb; off += 64) {
        const long long idx = off + lane;
        int cnt = 0;
        const bool isfree = idx < Mb ? classify(idx, cnt) : false;
        unsigned long long bal = __builtin_amdgcn_ballot_w64(isfree);
        const int F = __builtin_popcountll(bal);
        if (free_before + F >= p.n) {                            // the n-th free draw of this call is in this step
            for (int skip = p.n - free_before - 1; skip > 0; --skip) bal &= bal - 1;
            const int t = __builtin_ctzll(bal);
            checks += wave_sum(lane <= t ? cnt : 0);
            used = off + t + 1;
            break;
        }
        free_before += F;
        checks += wave_sum(cnt);
    }
    if (used < 0) {                                              // the block ended first: nothing is touched
        if (lane == 0) { p.status[b] = 1; p.used[b] = 0; p.checks_out[b] = 0; }
        return;
    }
    double* pool = p.pool + (size_t)b * (p.cap + 2) * DIM;
    int fb = 0;
    for (long long off = 0; off < used; off += 64) {
        const long long idx = off + lane;
        int cnt = 0;
        const bool isfree = idx < used ? classify(idx, cnt) : false;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(isfree);
        if (isfree) {
            const int incl = __builtin_popcountll(bal & (~0ull >> (63 - lane)));
            double* row = pool + (size_t)(base + fb + incl - 1) * DIM;
#pragma unroll
            for (int c = 0; c < DIM; ++c) row[c] = att[DIM * idx + c];
        }
        fb += __builtin_popcountll(bal);
    }
    if (lane == 0) {
        if (N0 == 0) {
            const double* is = p.init_states + DIM * (size_t)b;
            const double* gs = p.goal_states + DIM * (size_t)b;
#pragma unroll
            for (int c = 0; c < DIM; ++c) { pool[c] = gs[c]; pool[DIM + c] = is[c]; }
        }
        p.n_nodes[b] = base + p.n;
        p.checks[b] += checks;
        p.used[b] = (int)used;
        p.checks_out[b] = checks;
        p.status[b] = 0;
    }
}

hipError_t launch_lsp_sample(const LspSampleParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    if (p.dim == 3) hipLaunchKernelGGL(lsp_sample_kernel<3>, dim3(p.B), dim3(64), 0, st, p);
    else hipLaunchKernelGGL(lsp_sample_kernel<2>, dim3(p.B), dim3(64), 0, st, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The node rows of a round: workgroup j serves slot slot_of[j]; its row offset is the sum of the node counts of the slots
// before it in slot_of, added up here (the counts live on the device).  k1 comes from the caller's table by node count (the
// host's ceil(k ln(q) / ln(100)), so no device logarithm decides an integer).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void lsp_gather_kernel(LspGatherParams p) {
    const int j = blockIdx.x, lane = threadIdx.x;
    auto count = [&](int i) {
        const int s = p.slot_of[i];
        if (s < 0 || s >= p.B) return 0;
        const int n = p.n_nodes[s];
        return n < 0 || n > p.cap + 2 ? 0 : n;
    };
    int before = 0;
    for (int i = lane; i < j; i += 64) before += count(i);
    before = wave_sum(before);
    const int N = count(j);
    if (lane == 0) {
        p.node_ptr[j] = before;
        if (j == p.A - 1) p.node_ptr[p.A] = before + N;
        p.n_free_out[j] = N;
        p.k1_out[j] = p.k1_table[N];
    }
    if (N == 0 || (long long)before + N > p.v_rows) return;
    const double* pool = p.pool + (size_t)p.slot_of[j] * (p.cap + 2) * p.dim;
    float* v = p.v + (size_t)before * p.dim;
    for (int i = lane; i < N * p.dim; i += 64) v[i] = (float)pool[i];
}

hipError_t launch_lsp_gather(const LspGatherParams& p, hipStream_t st) {
    if (p.A <= 0) return hipSuccess;
    hipLaunchKernelGGL(lsp_gather_kernel, dim3(p.A), dim3(64), 0, st, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// One round of one problem per wave.
//   Graph: the coalesced block of problem j (columns sorted by (source, target), symmetric): node a's out-edges are one
//   contiguous block sorted by target.  dijkstra() relaxes, for the extracted u, every v with an edge (v -> u) at cost
//   norm(p[u] - p[v]); the set is symmetric and the norm is too (the differences only change sign), so u's OUT-block serves.
//   Per edge slot (workspace): its float64 cost and a flag, 0 = unknown, 1 = known valid, 2 = invalidated (dead: out of both
//   neighbour lists).  Carried pairs are found in the new graph by binary search; one that is no longer an edge marks nothing.
//   Per node (LDS up to kLspLdsNodes nodes, workspace beyond): dist, prev, out-block starts.  A visited node keeps its
//   distance with the sign bit set: the scan skips it, and `alt < dist[v]` is false for it as it is in the reference (see
//   below), so no separate flag is read.
//   Dijkstra: each lane owns nodes lane, lane + 64, ...; an extraction is one scan of the owned nodes, a wave minimum of
//   (distance bits, id) -- the reference's min_dist order: least distance, lowest id among equals -- and the relaxation of u's
//   block, one lane per edge, strict `alt < dist[v]`.
//   Early exit: the run stops when node 1 is extracted (or at the first infinite minimum: dist[1] is infinite then and the
//   round ends).  Extraction keys never decrease -- costs are >= 0 and float64 addition is monotone, so every later alt is >=
//   the key it was built from -- hence a node extracted earlier can never be improved (alt >= du >= dist[v], not strictly
//   below), and neither dist[1] nor prev along node 1's chain, all extracted before it, can change in the rest of the run.
//   Path edges: the reference checks them one by one and stops at the first blocked one.  Point robot: the path's edges go to
//   the lanes 64 a pass; only the edges up to and including the first blocked one in path order are kept -- marked, appended
//   to the pair list in path order, their checks counted -- later ones stay unknown and uncounted (per-edge counts are
//   independent, so the total is exact).  Stick robot: one edge at a time, its interpolated sticks over the lanes.
//   Bounds: a run kills one unordered edge or ends the round, so a round has at most E / 2 + 1 runs; a run extracts at most N
//   nodes; a walk has at most N nodes.  Exceeding one sets status bit 1 and ends the problem.  Pair list full: status bit 0,
//   nothing of that pass is written.  Ids outside the graph: status bit 2.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kLspLdsNodes = 1024;
constexpr unsigned long long kLspInfBits = 0x7ff0000000000000ull;
constexpr unsigned long long kLspSign = 0x8000000000000000ull;

template <bool LDS, int DIM>
__device__ __forceinline__ void lsp_round_body(const LspRoundParams& p, int slot, unsigned long long* s_dist, int* s_prev, int* s_rb,
                                               unsigned char* occ) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int N = p.n_nodes[slot];
    const int e0 = p.edge_ptr[j], E = p.edge_ptr[j + 1] - e0;
    const size_t stride = (size_t)p.cap + 3;
    unsigned long long* dist = LDS ? s_dist : p.ws_dist + (size_t)j * stride;
    int* prev = LDS ? s_prev : p.ws_prev + (size_t)j * stride;
    int* rb = LDS ? s_rb : p.ws_rb + (size_t)j * stride;
    const long long* src = p.edge_index + e0;
    const long long* dst = p.edge_index + p.total_edges + e0;
    double* cost = p.ws_cost + e0;
    unsigned char* flag = p.ws_flag + e0;
    const double* pts = p.pool + (size_t)slot * (p.cap + 2) * DIM;
    int* pairs = p.pairs + (size_t)slot * p.pair_cap * 2;
    unsigned char* pstate = p.pair_state + (size_t)slot * p.pair_cap;
    int* path = p.path + (size_t)slot * (p.cap + 2);
    int n_pairs = p.n_pairs[slot];
    int status = 0, solved = 0, path_len = 0, runs = 0;
    long long checks = 0;

    const MzMaze m = mz_maze(p.maps + (size_t)slot * p.w * p.w, p.w, occ, lane);
    // ---- out-block starts, costs, flags
    for (int u = lane; u <= N; u += 64) rb[u] = lower_bound(src, 0, E, (long long)u);
    bool ok = n_pairs >= 0 && n_pairs <= p.pair_cap;
    for (int e = lane; e < E; e += 64) {
        const long long s = src[e], t = dst[e];
        if (s < 0 || s >= N || t < 0 || t >= N) { ok = false; continue; }
        cost[e] = mz_cost<DIM>(pts + s * DIM, pts + t * DIM);
        flag[e] = 0;
    }
    if (!__all(ok)) {
        if (lane == 0) p.status[slot] |= 4;
        return;
    }
    wave_sync();
    // ---- carried pairs: both directions of an invalid pair are dead, of a valid pair known
    for (int i = lane; i < n_pairs; i += 64) {
        const int a = pairs[2 * i], c = pairs[2 * i + 1];
        if (a < 0 || a >= N || c < 0 || c >= N) continue;
        const int q = lsp_slot(dst, rb, a, c), r = lsp_slot(dst, rb, c, a);
        if (q >= 0 && r >= 0) flag[q] = flag[r] = pstate[i];
    }
    wave_sync();
    const int max_runs = (E >> 1) + 1;
    while (true) {
        if (runs >= max_runs) { status |= 2; break; }
        // ---- one Dijkstra run from node 0
        for (int i = lane; i < N; i += 64) { dist[i] = kLspInfBits; prev[i] = -1; }
        wave_sync();
        if (lane == 0) { dist[0] = 0ull; prev[0] = 0; }
        wave_sync();
        ++runs;
        bool reached = false;
        int it = 0;
        for (; it < N; ++it) {
            unsigned long long best = ~0ull;
            int bi = 0x7fffffff;
            for (int i = lane; i < N; i += 64) {
                const unsigned long long k = dist[i];            // dist >= 0: bit order = value order; visited: sign bit
                if (k < best) { best = k; bi = i; }              // ascending ids: the first strict minimum
            }
            const unsigned long long w = wave_min_u64(best);
            if (w >= kLspInfBits) break;                         // +inf, or everything visited
            const int u = (int)wave_min_u64(best == w ? (unsigned long long)(unsigned)bi : ~0ull);
            if (u == 1) { reached = true; break; }
            const double du = __longlong_as_double((long long)w);
            for (int q = rb[u] + lane; q < rb[u + 1]; q += 64) {
                if (flag[q] == 2) continue;
                const int v = (int)dst[q];
                const double alt = du + cost[q];
                const unsigned long long dv = dist[v];
                if (!(dv & kLspSign) && alt < __longlong_as_double((long long)dv)) {
                    dist[v] = (unsigned long long)__double_as_longlong(alt);
                    prev[v] = u;
                }
            }
            if (lane == 0) dist[u] = w | kLspSign;
            wave_sync();
        }
        if (!reached) {
            if (it >= N) status |= 2;                            // N extractions without meeting node 1 or infinity
            break;                                               // dist[1] is infinite: the round ends
        }
        // ---- the path from node 1 along prev (every lane walks it; lane 0 writes)
        int L = 0, cur = 1;
        bool walk_ok = true;
        if (lane == 0) path[0] = 1;
        while (cur != 0) {
            cur = prev[cur];
            if (cur < 0 || cur >= N || L + 1 >= N) { walk_ok = false; break; }
            ++L;
            if (lane == 0) path[L] = cur;
        }
        if (!walk_ok) { status |= 2; break; }
        wave_sync();
        // ---- its unknown edges
        bool feasible = true, full = false;
        if (DIM == 2) {
            for (int base = 0; base < L && feasible; base += 64) {
                const int i = base + lane;
                bool unknown = false, blocked = false;
                int cnt = 0, n1 = 0, n2 = 0, q = -1;
                if (i < L) {
                    n1 = path[i]; n2 = path[i + 1];
                    q = lsp_slot(dst, rb, n1, n2);
                    if (q >= 0 && flag[q] == 0) {
                        unknown = true;
                        const double* a = pts + (size_t)n1 * 2;
                        const double* c = pts + (size_t)n2 * 2;
                        blocked = !mz_edge2(m, a[0], a[1], c[0], c[1], cnt);
                    }
                }
                const unsigned long long bad = __builtin_amdgcn_ballot_w64(blocked);
                const int first = bad ? __builtin_ctzll(bad) : 63;
                const bool keep = unknown && lane <= first;
                const unsigned long long kb = __builtin_amdgcn_ballot_w64(keep);
                const int n_new = __builtin_popcountll(kb);
                if (n_pairs + n_new > p.pair_cap) { full = true; break; }
                if (keep) {
                    const int pos = n_pairs + __builtin_popcountll(kb & ((1ull << lane) - 1ull));
                    const unsigned char st = blocked ? 2 : 1;
                    pairs[2 * pos] = n1; pairs[2 * pos + 1] = n2; pstate[pos] = st;
                    flag[q] = st;
                    const int r = lsp_slot(dst, rb, n2, n1);
                    if (r >= 0) flag[r] = st;
                }
                checks += wave_sum(keep ? cnt : 0);
                n_pairs += n_new;
                wave_sync();
                if (bad) feasible = false;
            }
        } else {
            for (int i = 0; i < L; ++i) {
                const int n1 = path[i], n2 = path[i + 1];
                const int q = lsp_slot(dst, rb, n1, n2);
                if (q < 0 || flag[q] != 0) continue;             // known valid (a dead edge is never on a path)
                if (n_pairs + 1 > p.pair_cap) { full = true; break; }
                const bool fr = mz_stick_edge_wave(m, lane, pts + (size_t)n1 * 3, pts + (size_t)n2 * 3, checks);
                const unsigned char st = fr ? 1 : 2;
                if (lane == 0) {
                    pairs[2 * n_pairs] = n1; pairs[2 * n_pairs + 1] = n2; pstate[n_pairs] = st;
                    flag[q] = st;
                    const int r = lsp_slot(dst, rb, n2, n1);
                    if (r >= 0) flag[r] = st;
                }
                ++n_pairs;
                wave_sync();
                if (!fr) { feasible = false; break; }
            }
        }
        if (full) { status |= 1; break; }
        if (feasible) { solved = 1; path_len = L + 1; break; }
    }
    if (lane == 0) {
        p.n_pairs[slot] = n_pairs;
        p.checks[slot] += checks;
        p.dijkstra_runs[slot] += runs;
        p.status[slot] |= status;
        p.solved[slot] = solved;
        p.path_len[slot] = path_len;
    }
}

template <int DIM>
__global__ __launch_bounds__(64) void lsp_round_kernel(LspRoundParams p) {
    __shared__ unsigned long long s_dist[kLspLdsNodes];
    __shared__ int s_prev[kLspLdsNodes];
    __shared__ int s_rb[kLspLdsNodes + 1];
    __shared__ unsigned char occ[kMzLdsCells];
    const int slot = p.slot_of ? p.slot_of[blockIdx.x] : (int)blockIdx.x;
    if (slot < 0 || slot >= p.B) return;
    if (p.solved[slot] || p.status[slot]) return;                // finished problems are left as they are
    const int N = p.n_nodes[slot];
    const int E = p.edge_ptr[blockIdx.x + 1] - p.edge_ptr[blockIdx.x];
    if (N < 2 || N > p.cap + 2 || E < 0 || p.edge_ptr[blockIdx.x] < 0 || (long long)p.edge_ptr[blockIdx.x + 1] > p.total_edges) {
        if (threadIdx.x == 0) p.status[slot] |= 4;
        return;
    }
    if (N <= kLspLdsNodes) lsp_round_body<true, DIM>(p, slot, s_dist, s_prev, s_rb, occ);
    else lsp_round_body<false, DIM>(p, slot, s_dist, s_prev, s_rb, occ);
}

hipError_t launch_lsp_round(const LspRoundParams& p, hipStream_t st) {
    if (p.A <= 0) return hipSuccess;
    if (p.dim == 3) hipLaunchKernelGGL(lsp_round_kernel<3>, dim3(p.A), dim3(64), 0, st, p);
    else hipLaunchKernelGGL(lsp_round_kernel<2>, dim3(p.A), dim3(64), 0, st, p);
    return hipGetLastError();
}

int lsp_lds_nodes() { return kLspLdsNodes; }

}  // namespace gnnmp
