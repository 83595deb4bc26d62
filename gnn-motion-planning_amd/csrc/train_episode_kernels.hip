// train_episode_kernels.hip -- the supervision of the explorer's training step on the device: the stages of one sample of
// train_explorer.py:124-176 for a batch of problems, so that an optimizer step needs no host round trip between the
// forward and the loss.
//   (a) ep_label_kernel:  edge_free / edge_cost of construct_graph (algorithm/dijkstra.py:15-31) for maze problems: MazeEnv._edge_fp
//       (environment/maze_env.py:266-347) on the float64 node rows, cost = np.linalg.norm(p[target] - p[source]).
//   (b) ep_paths_kernel:  dijkstra(nodes, neighbors, edge_cost, goal) (dijkstra.py:49-76): dist / prev to the goal.
//   (c) ep_episode_kernel: explore() (train_explorer.py:42-63) and policy_data() (:66-93) on the detached scores.
// Everything is the reference's arithmetic and decision order, exactly (see each kernel).  Edge sets are the symmetric,
// coalesced kNN sets of construct_graph (edge (s -> t) present iff (t -> s) present, columns sorted by (source, target)):
// node a's out-edges are one contiguous block, sorted by target, and the reverse of edge (a -> c) is found by a binary
// search in c's block.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "maze_f64.hpp"

// numpy rounds every float64 operation on its own; the one fused operation is the one numpy's BLAS dot uses (mz_cost)
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kEpLdsNodes = 1024;       // problems up to this many nodes keep their per-node state in LDS

__device__ __forceinline__ unsigned ep_ord(float x) {          // order-preserving float -> unsigned, never 0 for a non-NaN
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// all lanes: out-block starts of the problem's nodes (row_beg [N + 1], problem-local slots) and, when rev != nullptr, the
// reverse of every edge (problem-local id, -1 when the edge set is not symmetric).  Returns (wave-uniform) whether every
// edge has its reverse.
__device__ bool ep_blocks(const long long* src, const long long* dst, int N, int E, int* row_beg, int* rev, int lane) {
    for (int u = lane; u <= N; u += 64) row_beg[u] = lower_bound(src, 0, E, (long long)u);
    wave_sync();
    bool ok = true;
    if (rev) {
        for (int e = lane; e < E; e += 64) {
            const long long s = src[e], t = dst[e];
            int r = -1;
            if (t >= 0 && t < N) {
                const int q = lower_bound(dst, row_beg[t], row_beg[t + 1], s);
                if (q < row_beg[t + 1] && dst[q] == s) r = q;
            }
            rev[e] = r;
            ok = ok && r >= 0;
        }
        wave_sync();
    }
    return __all(ok);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// (a) edge labels.  Grid (kEpLabelBlocks, B), 64 lanes: the blocks of problem b stride over its edges, one lane per edge.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kEpLabelBlocks = 8;

__global__ __launch_bounds__(64) void ep_label_kernel(EpLabelParams p) {
    __shared__ unsigned char occ[kMzLdsCells];
    const int b = blockIdx.y, lane = threadIdx.x;
    const int n0 = p.node_ptr[b], e0 = p.edge_ptr[b], E = p.edge_ptr[b + 1] - e0;
    const MzMaze m = mz_maze(p.maps + (size_t)b * p.w * p.w, p.w, occ, lane);
    const long long* src = p.edge_index + e0;
    const long long* dst = p.edge_index + p.total_edges + e0;
    for (int e = blockIdx.x * 64 + lane; e < E; e += kEpLabelBlocks * 64) {
        const double* s = p.points + (size_t)(n0 + src[e]) * p.dim;
        const double* t = p.points + (size_t)(n0 + dst[e]) * p.dim;
        int cnt = 0;                                                         // (the labels carry no check count)
        const bool fr = p.dim == 2 ? mz_edge2(m, s[0], s[1], t[0], t[1], cnt) : mz_stick_edge(m, s, t, cnt);
        double cost = INFINITY;
        if (fr) cost = p.dim == 2 ? mz_cost<2>(s, t) : mz_cost<3>(s, t);
        p.edge_free[e0 + e] = fr ? 1 : 0;
        p.edge_cost[e0 + e] = cost;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) shortest paths to the goal, one wave per problem.  dijkstra() takes, every round, the unvisited node of least
// distance, the lowest id among equals (min_dist walks the int set in id order and keeps the first strict minimum), and
// relaxes every v with an edge (v -> u): alt = dist[u] + cost(v -> u), taken only when strictly smaller.  Nodes of infinite
// distance relax nothing (inf + c is never < anything), so the loop ends at the first infinite minimum.  Each lane owns
// nodes lane, lane + 64, ...; a round is one scan of the owned nodes, a wave minimum of (distance bits, id) and the
// relaxation of u's block, one lane per edge.
// ---------------------------------------------------------------------------------------------------------------------
template <bool LDS>
__device__ __forceinline__ void ep_paths_body(const EpPathsParams& p, double* s_dist, unsigned char* s_done, int* s_rb) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n0 = p.node_ptr[b], N = p.node_ptr[b + 1] - n0;
    const int e0 = p.edge_ptr[b], E = p.edge_ptr[b + 1] - e0;
    const long long* src = p.edge_index + e0;
    const long long* dst = p.edge_index + p.total_edges + e0;
    const double* cost = p.edge_cost + e0;
    double* dist = LDS ? s_dist : p.dist + n0;
    unsigned char* done = LDS ? s_done : p.done + n0;
    int* rb = LDS ? s_rb : p.row_beg + n0 + b;
    int* prev = p.prev + n0;
    const int goal = p.goal_index[b];
    for (int i = lane; i < N; i += 64) { dist[i] = INFINITY; done[i] = 0; prev[i] = -1; }
    const bool sym = ep_blocks(src, dst, N, E, rb, nullptr, lane);
    wave_sync();
    if (goal < 0 || goal >= N) {                                            // nothing to do: every node unreachable
        if (LDS) for (int i = lane; i < N; i += 64) p.dist[n0 + i] = INFINITY;
        if (lane == 0) p.n_valid[b] = 0;
        return;
    }
    if (lane == 0) { dist[goal] = 0.0; prev[goal] = goal; }
    wave_sync();
    bool sym_ok = sym;
    while (true) {
        unsigned long long best = ~0ull;
        int bi = 0x7fffffff;
        for (int i = lane; i < N; i += 64) {
            if (done[i]) continue;
            const unsigned long long k = (unsigned long long)__double_as_longlong(dist[i]);    // dist >= 0: bits order = value order
            if (k < best) { best = k; bi = i; }                              // ascending ids: the first strict minimum
        }
        const unsigned long long w = wave_min_u64(best);
        if (w >= 0x7ff0000000000000ull) break;                               // +inf (or nothing left)
        const unsigned long long cand = best == w ? (unsigned long long)(unsigned)bi : ~0ull;
        const int u = (int)wave_min_u64(cand);
        const double du = __longlong_as_double((long long)w);
        if (lane == 0) done[u] = 1;
        for (int q = rb[u] + lane; q < rb[u + 1]; q += 64) {                 // v = dst[q]; cost(v -> u) is the reverse edge's
            const int v = (int)dst[q];
            const int r = lower_bound(dst, rb[v], rb[v + 1], (long long)u);
            if (r >= rb[v + 1] || dst[r] != u) { sym_ok = false; continue; }
            const double alt = du + cost[r];
            if (alt < dist[v]) { dist[v] = alt; prev[v] = u; }
        }
        wave_sync();
    }
    int cnt = 0;
    for (int i = lane; i < N; i += 64) {
        const double d = dist[i];
        cnt += d != INFINITY ? 1 : 0;
        if (LDS) p.dist[n0 + i] = d;
    }
    cnt = wave_sum(cnt);
    sym_ok = __all(sym_ok);
    if (lane == 0) p.n_valid[b] = sym_ok ? cnt : -1;
}

__global__ __launch_bounds__(64) void ep_paths_kernel(EpPathsParams p) {
    __shared__ double s_dist[kEpLdsNodes];
    __shared__ unsigned char s_done[kEpLdsNodes];
    __shared__ int s_rb[kEpLdsNodes + 1];
    const int N = p.node_ptr[blockIdx.x + 1] - p.node_ptr[blockIdx.x];
    if (N <= kEpLdsNodes) ep_paths_body<true>(p, s_dist, s_done, s_rb);
    else ep_paths_body<false>(p, s_dist, s_done, s_rb);
}

// ---------------------------------------------------------------------------------------------------------------------
// (c) explore() / policy_data() on the detached scores, one wave per problem.  The dense clone P[a][c] = score of edge
// (c -> a) lives here as: the out-block of a (cells (a, c), sorted by c), the reverse-edge ids (cell (a, c) holds the score of
// edge rev[(a -> c)]), a dead flag per cell (blocked edges kill (a, c) and (c, a): the edges (a -> c) and (c -> a)) and a
// killed flag per column (an explored node's column).  The diagonal is zero except P[goal][goal] = 1; a cell is present iff
// its value != 0 and it is not killed.  The explored list may hold the start twice (its column is never killed until it is
// explored again), its row then twice.  Every explored position caches its row's best present cell (first maximum in column
// order), so a step looks at one key per position and rescans only the rows whose best cell died.
//   explore mode: at most max_steps steps; step[b] = the step at which the goal was taken, else max_steps - 1; status 2 when
//   the frontier empties (the reference's exception), 1 when only the goal is reachable (n_valid == 1).
//   replay mode: exactly step[b] steps (stopping at the goal), then the frontier as edge ids in (explored position, column)
//   order with P[goal][goal] = 1 restored, and the label: first argmin over the frontier of the float32 norm of
//   (row, column) - (next_node, prev[next_node]), next_node = first argmin of dist over the explored list.
// ---------------------------------------------------------------------------------------------------------------------
struct EpShared { int *rb, *explored, *key_col, *key_slot; unsigned* key; unsigned char* colkill; };

template <bool LDS>
__device__ __forceinline__ void ep_episode_body(const EpEpisodeParams& p, const EpShared& sh) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n0 = p.node_ptr[b], N = p.node_ptr[b + 1] - n0;
    const int e0 = p.edge_ptr[b], E = p.edge_ptr[b + 1] - e0;
    const long long* src = p.edge_index + e0;
    const long long* dst = p.edge_index + p.total_edges + e0;
    const float* sc = p.scores + e0;
    const unsigned char* efree = p.edge_free + e0;
    const int goal = p.goal_index[b], start = p.start_index[b];
    const int slots = N + 2;                                                 // explored list: every node once, the start twice
    int* rb = LDS ? sh.rb : p.row_beg + n0 + b;
    int* explored = LDS ? sh.explored : p.explored + n0 + 2 * b;
    unsigned* key = LDS ? sh.key : p.key + n0 + 2 * b;
    int* key_col = LDS ? sh.key_col : p.key_col + n0 + 2 * b;
    int* key_slot = LDS ? sh.key_slot : p.key_slot + n0 + 2 * b;
    unsigned char* colkill = LDS ? sh.colkill : p.colkill + n0;
    int* rev = p.rev + e0;
    unsigned char* dead = p.dead + e0;
    const bool replay = p.replay != 0;
    int* fr_out = replay ? p.frontier + 2 * (size_t)e0 + b : nullptr;

    // skip rules (train_explorer.py:133, 166-169) and bad inputs
    int status = 0;
    const int nv = p.n_valid[b];
    if (nv < 0) status = 3;
    else if (nv == 1) status = 1;
    else if (goal < 0 || goal >= N || start < 0 || start >= N) status = 3;
    const int steps_in = replay ? p.step[b] : p.max_steps;
    if (replay && (p.status[b] != 0 || steps_in < 0)) status = p.status[b] != 0 ? p.status[b] : 3;
    if (status == 0) {
        for (int i = lane; i < N; i += 64) colkill[i] = 0;
        for (int e = lane; e < E; e += 64) dead[e] = 0;
        if (!ep_blocks(src, dst, N, E, rb, rev, lane)) status = 3;
    }
    if (status != 0) {
        if (lane == 0) {
            if (replay) { p.frontier_len[b] = 0; p.label[b] = -1; }
            else { p.status[b] = status; p.step[b] = -1; }
        }
        return;
    }

    // value of cell (a, c) held by out-edge slot q = (a -> c): the clone after the diagonal reset
    auto value = [&](int a, int c, int q) -> float {
        if (a == c) return a == goal ? 1.0f : 0.0f;
        const int r = rev[q];
        return r >= 0 ? sc[r] : 0.0f;
    };
    auto rescan = [&](int i) {
        const int a = explored[i];
        unsigned long long best = 0;
        int bq = -1;
        for (int q = rb[a] + lane; q < rb[a + 1]; q += 64) {
            const int c = (int)dst[q];
            const float x = value(a, c, q);
            if (x != 0.0f && !dead[q] && !colkill[c]) {
                const unsigned long long k = ((unsigned long long)ep_ord(x) << 32) | (0xffffffffu - (unsigned)c);
                if (k > best) { best = k; bq = q; }                          // value desc, column asc
            }
        }
        const unsigned long long w = wave_max_u64(best);
        int wq = -1;
        if (w) wq = __builtin_amdgcn_readlane(bq, __builtin_ctzll(__ballot(best == w)));
        if (lane == 0) {
            key[i] = (unsigned)(w >> 32);
            key_col[i] = w ? (int)(0xffffffffu - (unsigned)w) : -1;
            key_slot[i] = wq;
        }
    };

    if (lane == 0) explored[0] = start;
    wave_sync();
    rescan(0);
    wave_sync();
    int n_expl = 1, step_i = -1;
    bool emptied = false;
    for (int it = 0; it < steps_in; ++it) {
        step_i = it;
        unsigned long long best = 0;
        for (int i = lane; i < n_expl; i += 64) {
            const unsigned k = key[i];
            const unsigned long long kk = ((unsigned long long)k << 32) | (0xffffffffu - (unsigned)i);
            if (k && kk > best) best = kk;                                   // value desc, position asc
        }
        const unsigned long long w = wave_max_u64(best);
        if (!w) { emptied = true; break; }                                   // argmax of an empty tensor raises
        const int bp = (int)(0xffffffffu - (unsigned)w);
        const int a = explored[bp], c = key_col[bp], q = key_slot[bp];
        const int r = rev[q];
        const bool fr = efree[r] != 0;                                       // edge_cost[a, c] = cost of edge (c -> a)
        if (fr) {
            if (lane == 0) { explored[n_expl] = c; colkill[c] = 1; }
            ++n_expl;
            if (c == goal) break;
        } else if (lane == 0) {
            dead[q] = 1; dead[r] = 1;                                        // cells (a, c) and (c, a)
        }
        wave_sync();
        // rows whose cached best cell died: column c (free) or the cells (a, c) / (c, a) (blocked); then the new row
        const int old_n = fr ? n_expl - 1 : n_expl;
        for (int base = 0; base < old_n; base += 64) {
            const int i = base + lane;
            bool st = false;
            if (i < old_n && key[i] != 0) {
                const int kc = key_col[i], ar = explored[i];
                st = fr ? kc == c : ((ar == a && kc == c) || (ar == c && kc == a));
            }
            unsigned long long stale = __ballot(st);
            while (stale) {
                rescan(base + __builtin_ctzll(stale));
                stale &= stale - 1;
            }
        }
        if (fr) rescan(n_expl - 1);
        wave_sync();
    }

    if (!replay) {
        if (lane == 0) {
            const bool fail = emptied || steps_in <= 0;
            p.status[b] = fail ? 2 : 0;
            p.step[b] = fail ? -1 : step_i;
        }
        return;
    }

    // ---- policy_data's tail: next node, frontier (P[goal][goal] = 1 again), label
    const double* dist = p.dist + n0;
    unsigned long long bd = ~0ull;
    for (int i = lane; i < n_expl; i += 64) {
        const unsigned long long k = (unsigned long long)__double_as_longlong(dist[explored[i]]);
        if (k < bd) bd = k;                                                  // first minimum per lane (positions ascend)
    }
    const unsigned long long wd = wave_min_u64(bd);
    unsigned long long cpos = ~0ull;
    for (int i = lane; i < n_expl; i += 64)
        if ((unsigned long long)__double_as_longlong(dist[explored[i]]) == wd) { cpos = (unsigned long long)i; break; }
    const int npos = (int)wave_min_u64(cpos);
    const int nn = explored[npos];
    const int pn = p.prev[n0 + nn];
    const float fr0 = (float)nn, fr1 = pn >= 0 ? (float)pn : INFINITY;
    int len = 0;
    unsigned long long lbest = ~0ull;                                        // (norm bits, frontier position) minimum
    for (int i = 0; i < n_expl; ++i) {
        const int a = explored[i];
        for (int base = rb[a]; base < rb[a + 1]; base += 64) {
            const int q = base + lane;
            bool pres = false;
            int c = 0;
            if (q < rb[a + 1]) {
                c = (int)dst[q];
                if (a == c) pres = a == goal;
                else pres = value(a, c, q) != 0.0f && !dead[q] && !colkill[c];
            }
            const unsigned long long bal = __ballot(pres);
            if (pres) {
                const int at = len + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
                fr_out[at] = e0 + rev[q];
                // torch (CPU): FloatTensor(frontier) - FloatTensor(next_edge), then norm over dim 0 as its reduction does it
                // for two rows: acc = fmaf(dc, dc, dr * dr) in float32, sqrt in double, rounded to float32 (measured against
                // torch for differences up to 20000, where dr * dr and the sum round in float32)
                const float dr = (float)a - fr0, dc = (float)c - fr1;
                const float acc = __builtin_fmaf(dc, dc, dr * dr);
                const float nrm = (float)sqrt((double)acc);
                const unsigned long long k = ((unsigned long long)__float_as_uint(nrm) << 32) | (unsigned)at;
                if (k < lbest) lbest = k;
            }
            len += __builtin_popcountll(bal);
        }
    }
    const unsigned long long wl = wave_min_u64(lbest);
    if (lane == 0) {
        p.frontier_len[b] = len;
        p.label[b] = len ? (pn >= 0 ? (int)(unsigned)wl : 0) : -1;          // an infinite prev: every norm is inf, argmin 0
    }
}

__global__ __launch_bounds__(64) void ep_episode_kernel(EpEpisodeParams p) {
    __shared__ int s_rb[kEpLdsNodes + 1], s_explored[kEpLdsNodes + 2], s_key_col[kEpLdsNodes + 2], s_key_slot[kEpLdsNodes + 2];
    __shared__ unsigned s_key[kEpLdsNodes + 2];
    __shared__ unsigned char s_colkill[kEpLdsNodes];
    const EpShared sh{s_rb, s_explored, s_key_col, s_key_slot, s_key, s_colkill};
    const int N = p.node_ptr[blockIdx.x + 1] - p.node_ptr[blockIdx.x];
    if (N <= kEpLdsNodes) ep_episode_body<true>(p, sh);
    else ep_episode_body<false>(p, sh);
}

hipError_t launch_ep_label(const EpLabelParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(ep_label_kernel, dim3(kEpLabelBlocks, p.B), dim3(64), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_ep_paths(const EpPathsParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(ep_paths_kernel, dim3(p.B), dim3(64), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_ep_episode(const EpEpisodeParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(ep_episode_kernel, dim3(p.B), dim3(64), 0, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
