// smoother_replay_kernels.hip -- the replay of the smoother's training loop on the device (train_smoother.py:20-61, 91-99): the
// store of (path, path_smooth, free, collided) samples, the gnnmp_smooth_batch of one optimizer step gathered out of it, and the
// loss train() differentiates with its gradient with respect to the network's output.  Each entry point is ONE launch.
//
//   smooth_replay_append_kernel   one workgroup (256 threads) per source sample; workgroups of samples that are not taken leave
//       at once, except workgroup 0, which keeps the books.  Wave 0 of every workgroup runs the SAME exclusive scan over all B
//       sources: pass 1 sums the samples and the path / free / collided rows the call would add and validates the taken sources,
//       pass 2 hands the taken samples, in ascending position, consecutive slots and row offsets behind the counts.  The counts
//       are read from bank (epoch & 1) and written, by workgroup 0 alone, to the other bank, so no workgroup reads a word another
//       one writes in the same launch.  When the call does not fit (status bit 1) or a source is malformed (bit 2) NOTHING is
//       written but status, pending[] and the new bank, which repeats the old counts.  Otherwise workgroup 0 writes the prefix
//       entries and problem[] of every new slot, and each taken sample's workgroup copies its own rows: P path rows, P target
//       rows, min(n_free, 500) free rows, min(n_coll, 500) collided rows.
//   smooth_replay_gather_kernel   one workgroup per group entry.  Wave 0 scans the G entries' sizes the same way (every workgroup
//       the same numbers); the workgroup copies its sample's rows to the offsets of its position in the group, writes its
//       3 P - 2 edges in chain_edge_index's order (i + 1 -> i, i -> i + 1, self loops; path-local ids, int64) and entry g + 1 of
//       the four prefix arrays (workgroup 0 also entry 0).
//   smooth_path_loss_kernel   ONE workgroup of 8 waves, wave w takes the paths w, w + 8, ...: the squared differences of the
//       interior rows' P - 2 times C elements, which lie side by side in memory, are summed as ONE ascending chain in double
//       (64 elements a chunk, one per lane, added in lane order out of the lanes' registers); terms[g] = sum / ((P - 2) C);
//       d_pred = 2 (pred - target) / ((P - 2) C divisor) in double, rounded once; end rows exactly 0.  After the barrier thread
//       0 adds the terms in ascending g and stores (float)(sum / divisor).
//
// Integers only in the scans; no floating-point atomics, no scratch, vector stores only; every launch is on the caller's stream
// and nothing is allocated or waited for.  Two runs give the same bits.
//
// Bounds (every guard of these kernels):
//   * append, empty side with filler: a taken sample with n_free == 0 (n_coll == 0) gets ONE free (collided) row of zeros; no
//     source row is read for it.
//   * append, truncation at 500: rows 500 and beyond of either side are neither read nor stored.
//   * append, P <= 2: a taken sample with fewer than three path rows is a malformed source (bit 2), like path rows outside
//     [0, total_path], node rows outside [0, total_nodes], n_free outside [0, node rows], more taken samples than take_upper and
//     counts outside [0, cap].  Sources that are not taken are not looked at beyond their flag.  The sums are 64-bit; the fit
//     test is counts + new <= cap for the samples and the three kinds of rows, so every destination row lies inside its array.
//   * gather, repeated index: entries are independent, a sample that occurs twice is copied twice.  An index outside
//     [0, n_samples), n_samples beyond cap_samples, prefix entries that do not ascend inside the capacities, or totals that differ
//     from the caller's: status bit 4 and nothing is written, so every destination row lies inside the caller's arrays.
//   * path loss, P <= 2: the path's term is 0 and its rows of d_pred are 0; a path whose rows are not inside [0, total_rows]
//     gets the term 0 and touches no row.  Lanes beyond the last element of a chunk compute on zeros and store nothing.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "wave64.hpp"

// the restatement on the host rounds every float64 operation on its own
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kSmFull = 1, kSmBadSource = 2, kSmBadGather = 4;
constexpr int kSmSide = 500;              // obs_data: free[:500], collided[:500]
constexpr int kSmThreads = 256;
constexpr int kSmLossWaves = 8;

__device__ __forceinline__ long long sm_wave_sum(long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ int sm_wave_incl(int x, int lane) {     // inclusive prefix sum over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(x, off, 64);
        if (lane >= off) x += o;
    }
    return x;
}
// lane i's value of x in every lane (i the same in every lane)
__device__ __forceinline__ double sm_lane_value(double x, int i) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), i);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

struct SmLen { int take, P, F, Co; };

// what source sample i adds (all zero when it is not taken), `bad` raised for a malformed taken source
__device__ __forceinline__ SmLen smooth_src_len(const SmoothReplaySrc& s, int i, bool& bad) {
    SmLen r = {0, 0, 0, 0};
    if (s.take[i] == 0) return r;
    const long long a = s.path_ptr[i], e = s.path_ptr[i + 1], na = s.node_ptr[i], ne = s.node_ptr[i + 1], nf = s.n_free[i];
    if (a < 0 || e > s.total_path || e - a <= 2 || na < 0 || ne > s.total_nodes || ne < na || nf < 0 || nf > ne - na) {
        bad = true;
        return r;
    }
    const long long nc = ne - na - nf;
    r.take = 1;
    r.P = (int)(e - a);
    r.F = nf == 0 ? 1 : (int)(nf < kSmSide ? nf : kSmSide);
    r.Co = nc == 0 ? 1 : (int)(nc < kSmSide ? nc : kSmSide);
    return r;
}

__global__ __launch_bounds__(kSmThreads) void smooth_replay_append_kernel(SmoothReplayStore st, SmoothReplaySrc s) {
    __shared__ int sh[4];                                        // fits, and this sample's path / free / collided row offset
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool mine = s.take[b] != 0;
    if (b != 0 && !mine) return;
    if (tid < 64) {
        const int lane = tid;
        const int* cur = st.counts + 4 * (st.epoch & 1);
        int* nxt = st.counts + 4 * ((st.epoch + 1) & 1);
        const int n0 = cur[0], p0 = cur[1], f0 = cur[2], c0 = cur[3];
        bool bad = n0 < 0 || n0 > st.cap_samples || p0 < 0 || p0 > st.cap_path || f0 < 0 || f0 > st.cap_free || c0 < 0 ||
                   c0 > st.cap_coll;
        long long tn = 0, tp = 0, tf = 0, tc = 0;
        for (int base = 0; base < s.B; base += 64) {
            const int i = base + lane;
            SmLen r = {0, 0, 0, 0};
            if (i < s.B) r = smooth_src_len(s, i, bad);
            tn += r.take; tp += r.P; tf += r.F; tc += r.Co;
        }
        tn = sm_wave_sum(tn); tp = sm_wave_sum(tp); tf = sm_wave_sum(tf); tc = sm_wave_sum(tc);
        bad = __ballot(bad) != 0ull || tn > s.take_upper;
        const bool fit = !bad && n0 + tn <= st.cap_samples && p0 + tp <= st.cap_path && f0 + tf <= st.cap_free &&
                         c0 + tc <= st.cap_coll;
        if (lane == 0) sh[0] = fit ? 1 : 0;
        if (fit) {
            int run_n = n0, run_p = p0, run_f = f0, run_c = c0;
            for (int base = 0; base < s.B; base += 64) {
                const int i = base + lane;
                bool unused = false;
                SmLen r = {0, 0, 0, 0};
                if (i < s.B) r = smooth_src_len(s, i, unused);
                const int in_n = sm_wave_incl(r.take, lane), in_p = sm_wave_incl(r.P, lane);
                const int in_f = sm_wave_incl(r.F, lane), in_c = sm_wave_incl(r.Co, lane);
                if (r.take) {
                    const int slot = run_n + in_n - 1;
                    if (b == 0) {
                        st.path_ptr[slot + 1] = run_p + in_p;
                        st.free_ptr[slot + 1] = run_f + in_f;
                        st.coll_ptr[slot + 1] = run_c + in_c;
                        st.problem[slot] = s.problem_ids[i];
                    }
                    if (i == b) { sh[1] = run_p + in_p - r.P; sh[2] = run_f + in_f - r.F; sh[3] = run_c + in_c - r.Co; }
                }
                run_n += __shfl(in_n, 63, 64); run_p += __shfl(in_p, 63, 64);
                run_f += __shfl(in_f, 63, 64); run_c += __shfl(in_c, 63, 64);
            }
        }
        if (b == 0 && lane == 0) {
            if (!fit) st.status[0] = st.status[0] | (bad ? kSmBadSource : kSmFull);
            const int an = fit ? (int)tn : 0, ap = fit ? (int)tp : 0, af = fit ? (int)tf : 0, ac = fit ? (int)tc : 0;
            st.pending[0] = n0; st.pending[1] = p0; st.pending[2] = f0; st.pending[3] = c0;
            st.pending[4] = an; st.pending[5] = ap; st.pending[6] = af; st.pending[7] = ac;
            if (an > 0) { st.path_ptr[n0] = p0; st.free_ptr[n0] = f0; st.coll_ptr[n0] = c0; }
            nxt[0] = n0 + an; nxt[1] = p0 + ap; nxt[2] = f0 + af; nxt[3] = c0 + ac;
        }
    }
    __syncthreads();
    if (sh[0] == 0 || !mine) return;
    // this sample's rows (validated by the scan: every row read lies inside the source, every row written inside the store)
    const int C = st.C;
    const long long a = s.path_ptr[b], na = s.node_ptr[b];
    const int P = s.path_ptr[b + 1] - s.path_ptr[b];
    const int nf = s.n_free[b], nc = (s.node_ptr[b + 1] - s.node_ptr[b]) - nf;
    const int F = nf == 0 ? 1 : (nf < kSmSide ? nf : kSmSide), Co = nc == 0 ? 1 : (nc < kSmSide ? nc : kSmSide);
    const long long dp = (long long)sh[1] * C, df = (long long)sh[2] * C, dc = (long long)sh[3] * C;
    // element counts in 64 bits: the ABI takes any row count below 2^31, times C up to 14
    for (long long e = tid; e < (long long)P * C; e += kSmThreads) {
        st.path[dp + e] = s.path[a * C + e];
        st.target[dp + e] = s.target[a * C + e];
    }
    for (long long e = tid; e < (long long)F * C; e += kSmThreads) st.free_pts[df + e] = nf == 0 ? 0.0f : s.v[na * C + e];
    for (long long e = tid; e < (long long)Co * C; e += kSmThreads) st.coll[dc + e] = nc == 0 ? 0.0f : s.v[(na + nf) * C + e];
}

struct SmSizes { int a, f, c, P, F, Co; };

// the rows of stored sample idx[j] (zeros and `bad` for an index or prefix entries outside the store)
__device__ __forceinline__ SmSizes smooth_stored(const SmoothReplayStore& st, const SmoothGatherParams& p, int j, bool& bad) {
    SmSizes r = {0, 0, 0, 0, 0, 0};
    const int i = p.idx[j];
    if (i < 0 || i >= p.n_samples) { bad = true; return r; }
    const int a = st.path_ptr[i], ae = st.path_ptr[i + 1], f = st.free_ptr[i], fe = st.free_ptr[i + 1];
    const int c = st.coll_ptr[i], ce = st.coll_ptr[i + 1];
    if (a < 0 || ae <= a || ae > st.cap_path || f < 0 || fe < f || fe > st.cap_free || c < 0 || ce < c || ce > st.cap_coll) {
        bad = true;
        return r;
    }
    r.a = a; r.f = f; r.c = c; r.P = ae - a; r.F = fe - f; r.Co = ce - c;
    return r;
}

__global__ __launch_bounds__(kSmThreads) void smooth_replay_gather_kernel(SmoothReplayStore st, SmoothGatherParams p) {
    __shared__ int sh[10];            // ok; source rows a, f, c; sizes P, F, Co; destination rows of path, free, collided
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid < 64) {
        const int lane = tid;
        bool bad = p.n_samples > st.cap_samples;
        long long tp = 0, tf = 0, tc = 0;
        if (!bad) {
            for (int base = 0; base < p.G; base += 64) {
                const int j = base + lane;
                SmSizes r = {0, 0, 0, 0, 0, 0};
                if (j < p.G) r = smooth_stored(st, p, j, bad);
                tp += r.P; tf += r.F; tc += r.Co;
            }
        }
        tp = sm_wave_sum(tp); tf = sm_wave_sum(tf); tc = sm_wave_sum(tc);
        bad = __ballot(bad) != 0ull;
        const bool ok = !bad && tp == p.total_path && tf == p.total_free && tc == p.total_coll &&
                        3 * tp - 2 * (long long)p.G == p.total_edges;
        if (lane == 0) sh[0] = ok ? 1 : 0;
        if (ok) {
            int run_p = 0, run_f = 0, run_c = 0;
            for (int base = 0; base < p.G; base += 64) {
                const int j = base + lane;
                bool unused = false;
                SmSizes r = {0, 0, 0, 0, 0, 0};
                if (j < p.G) r = smooth_stored(st, p, j, unused);
                const int in_p = sm_wave_incl(r.P, lane), in_f = sm_wave_incl(r.F, lane), in_c = sm_wave_incl(r.Co, lane);
                if (j == g) {
                    sh[1] = r.a; sh[2] = r.f; sh[3] = r.c; sh[4] = r.P; sh[5] = r.F; sh[6] = r.Co;
                    sh[7] = run_p + in_p - r.P; sh[8] = run_f + in_f - r.F; sh[9] = run_c + in_c - r.Co;
                }
                run_p += __shfl(in_p, 63, 64); run_f += __shfl(in_f, 63, 64); run_c += __shfl(in_c, 63, 64);
            }
        } else if (g == 0 && lane == 0) {
            st.status[0] = st.status[0] | kSmBadGather;
        }
    }
    __syncthreads();
    if (sh[0] == 0) return;
    const int C = st.C, P = sh[4], F = sh[5], Co = sh[6];
    const int op = sh[7], of = sh[8], oc = sh[9];
    const long long oe = 3ll * sh[7] - 2ll * g;                   // edges before this entry (<= total_edges, an int)
    const long long sa = (long long)sh[1] * C, sf = (long long)sh[2] * C, sc = (long long)sh[3] * C;
    const long long dp = (long long)op * C, df = (long long)of * C, dc = (long long)oc * C;
    for (long long e = tid; e < (long long)P * C; e += kSmThreads) {
        p.path[dp + e] = st.path[sa + e];
        p.target[dp + e] = st.target[sa + e];
    }
    for (long long e = tid; e < (long long)F * C; e += kSmThreads) p.free_pts[df + e] = st.free_pts[sf + e];
    for (long long e = tid; e < (long long)Co * C; e += kSmThreads) p.coll[dc + e] = st.coll[sc + e];
    for (long long e = tid; e < 3ll * P - 2; e += kSmThreads) {   // planner.chain_edge_index(P)
        long long r0, r1;
        if (e < P - 1) { r0 = e + 1; r1 = e; }
        else if (e < 2ll * P - 2) { r0 = e - (P - 1); r1 = r0 + 1; }
        else { r0 = e - (2ll * P - 2); r1 = r0; }
        p.edge_index[oe + e] = r0;
        p.edge_index[(long long)p.total_edges + oe + e] = r1;
    }
    if (tid == 0) {
        if (g == 0) { p.path_ptr[0] = 0; p.free_ptr[0] = 0; p.coll_ptr[0] = 0; p.edge_ptr[0] = 0; }
        p.path_ptr[g + 1] = op + P; p.free_ptr[g + 1] = of + F; p.coll_ptr[g + 1] = oc + Co;
        p.edge_ptr[g + 1] = (int)(oe + 3ll * P - 2);
    }
}

__global__ __launch_bounds__(64 * kSmLossWaves) void smooth_path_loss_kernel(SmoothPathLossParams p) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int C = p.C;
    for (int g = w; g < p.G; g += kSmLossWaves) {
        const long long a = p.path_ptr[g], b = p.path_ptr[g + 1];
        const long long P = b - a;
        double term = 0.0;
        if (a >= 0 && b <= p.total_rows && P > 2) {
            const long long M = (P - 2) * C;                     // interior elements, side by side behind row a + 1
            const long long o0 = (a + 1) * C;
            const double den_g = (double)(P - 2) * (double)C * (double)p.divisor;
            double sum = 0.0;
            for (long long base = 0; base < M; base += 64) {
                const long long k = base + lane;
                double sq = 0.0;
                if (k < M) {
                    const double d = (double)p.pred[o0 + k] - (double)p.target[o0 + k];
                    sq = d * d;
                    p.d_pred[o0 + k] = (float)(2.0 * d / den_g);
                }
                const int cnt = M - base < 64 ? (int)(M - base) : 64;
                for (int i = 0; i < cnt; ++i) sum = sum + sm_lane_value(sq, i);
            }
            if (lane < C) {
                p.d_pred[a * C + lane] = 0.0f;
                p.d_pred[(b - 1) * C + lane] = 0.0f;
            }
            term = sum / (double)M;
        } else if (a >= 0 && b <= p.total_rows && P > 0) {       // no interior row: the path's rows are zero
            for (long long e = lane; e < P * C; e += 64) p.d_pred[a * C + e] = 0.0f;
        }
        if (lane == 0) p.terms[g] = term;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int g = 0; g < p.G; ++g) total = total + p.terms[g];
        p.loss[0] = (float)(total / (double)p.divisor);
    }
}

}  // namespace

hipError_t launch_smooth_replay_append(const SmoothReplayStore& st, const SmoothReplaySrc& s, hipStream_t stream) {
    if (s.B <= 0 || s.take_upper <= 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_replay_append_kernel, dim3(s.B), dim3(kSmThreads), 0, stream, st, s);
    return hipGetLastError();
}

hipError_t launch_smooth_replay_gather(const SmoothReplayStore& st, const SmoothGatherParams& p, hipStream_t stream) {
    if (p.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_replay_gather_kernel, dim3(p.G), dim3(kSmThreads), 0, stream, st, p);
    return hipGetLastError();
}

hipError_t launch_smooth_path_loss(const SmoothPathLossParams& p, hipStream_t stream) {
    if (p.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_path_loss_kernel, dim3(1), dim3(64 * kSmLossWaves), 0, stream, p);
    return hipGetLastError();
}

}  // namespace gnnmp
