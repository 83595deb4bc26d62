// oracle_smooth_kernels.hip -- the smoother's training targets on the device: joint_smoother_ratio / joint_smoother
// (smoother.py:129-151) for a batch of maze paths -- 2-D (the point robot) or 3-D (the stick robot, MazeEnv(dim=3)) --
// one wave per path, the whole outer loop (iters x [random_path_smoother -> prune_path -> re-spacing]) in one launch.
// The kernel is one template over the dimension; the 2-D instantiation evaluates exactly the expressions it always did.
//
// Everything is the reference's arithmetic and decision order, exactly:
//   * a waypoint is float32 (an untouched input row) or float64 (perturbed / re-spaced); numpy's promotion decides the
//     precision of every expression, so every value carries a flag f ("is float32") next to its double (a float32 upcasts
//     exactly).  An expression is evaluated in float32 when all its array operands are float32, in float64 otherwise;
//   * MazeEnv._edge_fp (maze_env.py:316-326) keeps its short-circuit order inside one call, which fixes its contribution to
//     collision_check_count: both endpoint checks, then the bisection in preorder (mid, left half, right half) up to the
//     first blocked midpoint;
//   * np.linalg.norm of a 2-vector is sqrt(dot): float64 dot = fma(d1, d1, d0 * d0) (as ep_label_kernel has it), float32
//     dot = d0 * d0 + d1 * d1 with both operations rounded; sqrt and the float32 division go through double, whose 53 bits
//     make the second rounding to 24 bits harmless.
// The stick robot (maze_env.py:245-347), D = 3, waypoints (x, y, z, is32):
//   * _valid_state compares against LIMITS = (1, 1, 0.4) in float64 (a float32 z upcasts exactly); nothing wraps or clips;
//   * _stick_in_free_space does not depend on the waypoint's dtype: theta = z / 0.4 * pi and the stick ends are float64,
//     each in-bounds end is one check, then the float64 bisection of the end-to-end segment;
//   * _edge_fp of size 3: both validity tests, both stick checks, then K = int(distance / 0.015) interpolated sticks
//     c = state + k * 1. / K * disp (disp[2] wrapped by 0.8), each the 2-D _edge_fp of its ends, up to the first blocked
//     one.  Two float32 ends take the float32 flow of maze_kernels.hip's stick_edge_fp, anything else the float64 flow of
//     maze_f64.hpp's mz_stick_edge on exactly upcast values;
//   * np.linalg.norm of a 3-vector (no wrap) is sqrt(dot): float64 dot = fma(d2, d2, fma(d1, d1, d0 * d0)); float32 dot =
//     the three float32-rounded squares summed left to right in double and rounded once to float32.
// Parallel across lanes: the critical-index test and the all-pairs edge checks of create_graph (one ordered pair per lane),
// dijkstra's scan and relaxation, the duplicate test, the re-spacing.  Sequential: the perturbation trials (lanes 0 / 1 check
// the trial's two edges), dijkstra's rounds, the walk back.  Throughput comes from the batch: one 64-lane block per path.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "wave64.hpp"

// numpy rounds every operation on its own; the one fused operation is the float64 dot's (below)
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kOsCap = kOracleSmoothCap;        // waypoints per path
constexpr int kOsStack = 8;                     // pending right halves per lane (L1 length <= 4, RRT_EPS = 0.05: depth <= 7)
constexpr int kOsOccWords = kOracleSmoothMaxWidth * kOracleSmoothMaxWidth / 32;

enum : int { kStDuplicate = 1, kStCap = 2, kStUnreachable = 4, kStOrder = 8, kStStack = 16, kStNodeIdx = 32, kStTie = 64,
             kStBadPtr = 128 };

struct OsPt { double x, y, z; bool f; };        // f: the waypoint is a float32 array; z: the stick's orientation (D = 3)

struct OsMaze {
    const unsigned* occ;                        // LDS bit map, bit (cx * w + cy) set = obstacle
    int w;
    double* stk;                                // [2][kOsStack][64] pending right ends, entry (k, sp) of lane l at (k * kOsStack + sp) * 64 + l
    int* status;                                // LDS
    int lane;
};

__device__ __forceinline__ int os_cell(double x, bool f, int w) {        // ((x + 1.0) * w / 2.0).astype(int), clipped at w - 1
    int c;
    if (f) c = (int)((((float)x + 1.0f) * (float)w) / 2.0f);
    else c = (int)(((x + 1.0) * (double)w) / 2.0);
    return c > w - 1 ? w - 1 : c;
}
__device__ __forceinline__ bool os_valid(const OsPt& p) { return p.x >= -1.0 && p.x <= 1.0 && p.y >= -1.0 && p.y <= 1.0; }
__device__ __forceinline__ bool os_state(const OsMaze& m, const OsPt& p, int& cnt) {           // _point_in_free_space
    if (!os_valid(p)) return false;
    ++cnt;
    const int idx = os_cell(p.x, p.f, m.w) * m.w + os_cell(p.y, p.f, m.w);
    return ((m.occ[idx >> 5] >> (idx & 31)) & 1u) == 0u;
}
// _iterative_check_segment in preorder.  The current segment lives in registers; only the right ends of the pending right
// halves are stacked: when a subtree is done, its last leaf's right end is the pending half's left end.
__device__ bool os_segment(const OsMaze& m, OsPt l, OsPt r, int& cnt) {
    double* s = m.stk + m.lane;
    unsigned flags = 0;
    int sp = 0;
    while (true) {
        const int dc = abs(os_cell(l.x, l.f, m.w) - os_cell(r.x, r.f, m.w)) + abs(os_cell(l.y, l.f, m.w) - os_cell(r.y, r.f, m.w));
        const bool f = l.f && r.f;
        bool far;                                                            // np.sum(np.abs(left - right)) > RRT_EPS
        if (f) far = fabsf((float)l.x - (float)r.x) + fabsf((float)l.y - (float)r.y) > 0.05f;
        else far = fabs(l.x - r.x) + fabs(l.y - r.y) > 0.05;
        if (dc > 1 && far) {
            OsPt mid;
            mid.z = 0.0;
            mid.f = f;
            if (f) { mid.x = (double)(((float)l.x + (float)r.x) / 2.0f); mid.y = (double)(((float)l.y + (float)r.y) / 2.0f); }
            else { mid.x = (l.x + r.x) / 2.0; mid.y = (l.y + r.y) / 2.0; }
            if (!os_state(m, mid, cnt)) return false;
            if (sp >= kOsStack) { atomicOr(m.status, kStStack); return false; }          // cannot happen, never writes past the stack
            s[sp * 64] = r.x; s[(kOsStack + sp) * 64] = r.y;
            flags = (flags & ~(1u << sp)) | ((r.f ? 1u : 0u) << sp);
            ++sp;
            r = mid;
        } else {
            if (sp == 0) return true;
            --sp;
            l = r;
            r.x = s[sp * 64]; r.y = s[(kOsStack + sp) * 64]; r.f = ((flags >> sp) & 1u) != 0u;
        }
    }
}
__device__ bool os_edge(const OsMaze& m, const OsPt& a, const OsPt& b, int& cnt) {              // _edge_fp, size 2
    if (!os_valid(a) || !os_valid(b)) return false;
    if (!os_state(m, a, cnt)) return false;
    if (!os_state(m, b, cnt)) return false;
    return os_segment(m, a, b, cnt);
}
// ---- the stick robot.  _valid_state against LIMITS = (1, 1, 0.4)
__device__ __forceinline__ bool os_valid3(const OsPt& p) { return os_valid(p) && p.z >= -0.4 && p.z <= 0.4; }
// _end_points: theta = z / LIMITS[2] * pi, ends = center -+ (STICK_LENGTH / 2.) * (cos, sin), float64 whatever the state is
__device__ __forceinline__ void os_ends(double x, double y, double z, OsPt& a, OsPt& b) {
    const double theta = z / 0.4 * 3.141592653589793;
    const double ox = 0.1 * cos(theta), oy = 0.1 * sin(theta);
    a = OsPt{x - ox, y - oy, 0.0, false};
    b = OsPt{x + ox, y + oy, 0.0, false};
}
__device__ bool os_stick(const OsMaze& m, const OsPt& p, int& cnt) {                           // _stick_in_free_space
    if (!os_valid3(p)) return false;
    OsPt a, b;
    os_ends(p.x, p.y, p.z, a, b);
    if (!os_state(m, a, cnt)) return false;
    if (!os_state(m, b, cnt)) return false;
    return os_segment(m, a, b, cnt);
}
__device__ bool os_edge3(const OsMaze& m, const OsPt& s, const OsPt& t, int& cnt) {            // _edge_fp, size 3
    if (!os_valid3(s) || !os_valid3(t)) return false;
    if (!os_stick(m, s, cnt)) return false;
    if (!os_stick(m, t, cnt)) return false;
    OsPt a, b;
    if (s.f && t.f) {                                                        // float32 rows: stick_edge_fp's flow
        const float s0 = (float)s.x, s1 = (float)s.y, s2 = (float)s.z, t0 = (float)t.x, t1 = (float)t.y, t2 = (float)t.z;
        const float d0 = t0 - s0, d1 = t1 - s1;
        float d2 = t2 - s2;
        if (fabs((double)d2) > 0.4) d2 = (float)(d2 > 0.f ? (double)d2 - 0.8 : (double)d2 + 0.8);
        // distance(): |diff| in float32, third coordinate wrapped through float64, sqrt of the float32 sum of squares
        const float a0 = fabsf(d0), a1 = fabsf(d1), a2r = fabsf(t2 - s2);
        const double w2 = fabs((double)a2r - 0.8);
        const float a2 = (float)((double)a2r < w2 ? (double)a2r : w2);
        const float q0 = a0 * a0, q1 = a1 * a1, q2 = a2 * a2;
        const float q01 = q0 + q1;
        const float q = q01 + q2;
        const float dist = (float)sqrt((double)q);
        const int K = (int)(float)((double)dist / (double)0.015f);
        for (int k = 1; k < K; ++k) {
            const float r = (float)((double)k * 1.0 / (double)K);
            const float m0 = r * d0, m1 = r * d1, m2 = r * d2;
            const float cx = s0 + m0, cy = s1 + m1, cz = s2 + m2;
            os_ends((double)cx, (double)cy, (double)cz, a, b);
            if (!os_edge(m, a, b, cnt)) return false;
        }
        return true;
    }
    const double d0 = t.x - s.x, d1 = t.y - s.y;                             // float64, or mixed: exactly upcast values
    double d2 = t.z - s.z;
    if (fabs(d2) > 0.4) d2 = d2 > 0.0 ? d2 - 0.8 : d2 + 0.8;
    const double a0 = fabs(t.x - s.x), a1 = fabs(t.y - s.y);
    double a2 = fabs(t.z - s.z);
    const double w2 = fabs(a2 - 0.8);
    a2 = w2 < a2 ? w2 : a2;
    const double q0 = a0 * a0, q1 = a1 * a1, q2 = a2 * a2;
    const double d = sqrt((q0 + q1) + q2);
    const int K = (int)(d / 0.015);
    for (int k = 1; k < K; ++k) {
        const double r = (double)k / (double)K;                              // k * 1. / K
        const double m0 = r * d0, m1 = r * d1, m2 = r * d2;
        os_ends(s.x + m0, s.y + m1, s.z + m2, a, b);
        if (!os_edge(m, a, b, cnt)) return false;
    }
    return true;
}
template <int D> __device__ __forceinline__ bool os_state_d(const OsMaze& m, const OsPt& p, int& cnt) {    // _state_fp
    return D == 3 ? os_stick(m, p, cnt) : os_state(m, p, cnt);
}
template <int D> __device__ __forceinline__ bool os_edge_d(const OsMaze& m, const OsPt& a, const OsPt& b, int& cnt) {
    return D == 3 ? os_edge3(m, a, b, cnt) : os_edge(m, a, b, cnt);
}
// np.linalg.norm(a - b) of 3-vectors, no wrap
__device__ __forceinline__ double os_norm3(const OsPt& a, const OsPt& b, bool& f) {
    f = a.f && b.f;
    if (f) {
        const float d0 = (float)a.x - (float)b.x, d1 = (float)a.y - (float)b.y, d2 = (float)a.z - (float)b.z;
        const float p0 = d0 * d0, p1 = d1 * d1, p2 = d2 * d2;
        double acc = (double)p0 + (double)p1;
        acc = acc + (double)p2;
        return (double)(float)sqrt((double)(float)acc);
    }
    const double d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z;
    double acc = d0 * d0;
    acc = __builtin_fma(d1, d1, acc);
    acc = __builtin_fma(d2, d2, acc);
    return sqrt(acc);
}
// np.linalg.norm(a - b): the value as a double, f = it is a np.float32
__device__ __forceinline__ double os_norm(const OsPt& a, const OsPt& b, bool& f) {
    f = a.f && b.f;
    if (f) {
        const float d0 = (float)a.x - (float)b.x, d1 = (float)a.y - (float)b.y;
        const float p0 = d0 * d0, p1 = d1 * d1;
        const float sq = p0 + p1;
        return (double)(float)sqrt((double)sq);
    }
    const double d0 = a.x - b.x, d1 = a.y - b.y;
    double acc = d0 * d0;
    acc = __builtin_fma(d1, d1, acc);
    return sqrt(acc);
}
template <int D> __device__ __forceinline__ double os_norm_d(const OsPt& a, const OsPt& b, bool& f) {
    return D == 3 ? os_norm3(a, b, f) : os_norm(a, b, f);
}
// x + y of two numpy scalars with flags
__device__ __forceinline__ double os_add(double x, bool fx, double y, bool fy, bool& f) {
    f = fx && fy;
    return f ? (double)((float)x + (float)y) : x + y;
}
// (B - A) * i / n + A, one coordinate (smoother.py:148)
__device__ __forceinline__ double os_lerp(double A, double B, bool f, int i, int n) {
    if (f) {
        float d = (float)B - (float)A;
        d = d * (float)i;
        d = (float)((double)d / (double)n);
        return (double)(d + (float)A);
    }
    double d = B - A;
    d = d * (double)i;
    d = d / (double)n;
    return d + A;
}

template <int D> struct OsPath {                // one path in LDS
    double x[kOsCap], y[kOsCap], z[D == 3 ? kOsCap : 1];
    unsigned char f[kOsCap], src[kOsCap];
    __device__ __forceinline__ OsPt at(int i) const { return OsPt{x[i], y[i], D == 3 ? z[i] : 0.0, f[i] != 0}; }
    __device__ __forceinline__ void set(int i, const OsPt& p, int s) {
        x[i] = p.x; y[i] = p.y; f[i] = p.f ? 1 : 0; src[i] = (unsigned char)s;
        if (D == 3) z[i] = p.z;
    }
};

template <int D> struct OsShared {
    OsPath<D> R, P, N;                              // after the random stage; the prune's working path; the round's new path
    double dist[kOsCap];
    unsigned char dist_f[kOsCap], done[kOsCap], crit[kOsCap];
    short prev[kOsCap];
    unsigned adj[kOsCap][kOsCap / 32];
    unsigned occ[kOsOccWords];
    double stk[2 * kOsStack * 64];
    int status;
};

// two waypoints with identical coordinates among the first n of q (wave-uniform)
template <int D> __device__ bool os_duplicates(const OsPath<D>& q, int n, int lane) {
    bool dup = false;
    for (int i = lane; i < n; i += 64)
        for (int j = i + 1; j < n; ++j) dup = dup || (q.x[i] == q.x[j] && q.y[i] == q.y[j] && (D != 3 || q.z[i] == q.z[j]));
    return __any(dup);
}

}  // namespace

template <int D> __global__ __launch_bounds__(64) void oracle_smooth_kernel(OracleSmoothParams p) {
    __shared__ OsShared<D> sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int lo = p.path_ptr[b], hi = p.path_ptr[b + 1];
    if (lo < 0 || hi < lo || hi > p.total_points) {                          // nothing of this path can be addressed
        if (lane == 0) { p.status[b] = kStBadPtr; p.checks[b] = 0; p.out_len[b] = 0; }
        return;
    }
    int n = hi - lo;
    const double* in = p.paths + D * (size_t)lo;
    double* out = p.out + D * (size_t)lo;
    unsigned char* out_f = p.out_is32 + lo;
    if (n > kOsCap) {                                                        // beyond the cap: handed through, flagged
        for (int i = lane; i < n; i += 64) {
            for (int k = 0; k < D; ++k) out[D * i + k] = in[D * i + k];
            out_f[i] = p.in_is32 ? p.in_is32[lo + i] : 1;
        }
        if (lane == 0) { p.status[b] = kStCap; p.checks[b] = 0; p.out_len[b] = n; }
        return;
    }
    for (int i = lane; i < kOsOccWords; i += 64) sh.occ[i] = 0u;
    if (lane == 0) sh.status = 0;
    for (int i = lane; i < n; i += 64) {
        const bool f = p.in_is32 ? p.in_is32[lo + i] != 0 : true;
        sh.R.set(i, OsPt{in[D * i], in[D * i + 1], D == 3 ? in[D * i + 2] : 0.0, f}, i);
    }
    __syncthreads();
    const unsigned char* map = p.maps + (size_t)b * p.w * p.w;
    for (int i = lane; i < p.w * p.w; i += 64)
        if (map[i] != 0) atomicOr(&sh.occ[i >> 5], 1u << (i & 31));
    __syncthreads();
    const OsMaze m{sh.occ, p.w, sh.stk, &sh.status, lane};
    long long cnt = 0;                                                       // this lane's share of collision_check_count
    int status = 0;                                                          // wave-uniform bits
    const size_t draw0 = (size_t)b * p.iters * p.random_iter;

    if (os_duplicates(sh.R, n, lane)) status = kStDuplicate;

    for (int it = 0; it < p.iters && !(status & (kStDuplicate | kStOrder)); ++it) {
        const bool last = it == p.iters - 1;
        // ---- random_path_smoother (smoother.py:67-82): both draws of every trial are consumed whatever its outcome
        if (n > 2) {
            for (int t = 0; t < p.random_iter; ++t) {
                const size_t d = draw0 + (size_t)it * p.random_iter + t;
                int idx;
                if (p.node_idx) idx = p.node_idx[d];
                else {
                    const int k = (int)floor(p.u[d] * (double)(n - 2));
                    idx = 1 + (k < n - 3 ? (k < 0 ? 0 : k) : n - 3);
                }
                if (idx < 1 || idx > n - 2) { status |= kStNodeIdx; continue; }
                const OsPt old = sh.R.at(idx), pv = sh.R.at(idx - 1), nx = sh.R.at(idx + 1);
                const OsPt nw{old.x + p.action[D * d], old.y + p.action[D * d + 1], D == 3 ? old.z + p.action[D * d + 2] : 0.0,
                              false};                                        // tuple + float64 array
                int c0 = 0;
                bool ok = os_state_d<D>(m, nw, c0);                          // every lane: the same answer
                if (ok) {
                    int ce = 0;
                    bool e = false;
                    if (lane < 2) e = os_edge_d<D>(m, nw, lane == 0 ? pv : nx, ce);
                    const bool e1 = __shfl((int)e, 0, 64) != 0, e2 = __shfl((int)e, 1, 64) != 0;
                    if (lane == 0) cnt += c0 + ce;
                    if (lane == 1 && e1) cnt += ce;                          // the second edge is only checked after a free first
                    ok = e1 && e2;
                } else if (lane == 0) {
                    cnt += c0;
                }
                if (ok) {
                    bool f1, f2, f3, f4, fs;
                    const double a1 = os_norm_d<D>(nx, nw, f1), a2 = os_norm_d<D>(pv, nw, f2);
                    const double lhs = os_add(a1, f1, a2, f2, fs);
                    const double b1 = os_norm_d<D>(nx, old, f3), b2 = os_norm_d<D>(pv, old, f4);
                    const double rhs = os_add(b1, f3, b2, f4, fs);
                    if (lhs < rhs) {
                        __syncthreads();
                        if (lane == 0) sh.R.set(idx, nw, idx);
                        __syncthreads();
                    }
                }
            }
        }
        if (last && p.stop == 1) break;
        if (os_duplicates(sh.R, n, lane)) { status |= kStDuplicate; break; }

        // ---- prune_path (smoother.py:97-126) on a working copy P; src = index in R
        for (int i = lane; i < n; i += 64) sh.P.set(i, sh.R.at(i), i);
        __syncthreads();
        int len = n;
        for (int round = 0; round < p.prune_iter; ++round) {
            const int n0 = len;
            for (int i = lane; i < n0; i += 64) {                            // critical indices
                bool cr = i == 0 || i == n0 - 1;
                if (!cr) { int c = 0; cr = !os_edge_d<D>(m, sh.P.at(i - 1), sh.P.at(i + 1), c); cnt += c; }
                sh.crit[i] = cr ? 1 : 0;
            }
            if (lane == 0) sh.N.set(0, sh.P.at(0), sh.P.src[0]);
            __syncthreads();
            int new_len = 1, a = 0;
            bool failed = false;
            for (int e = 1; e < n0 && !failed; ++e) {
                if (!sh.crit[e]) continue;
                const int mm = e - a + 1;                                    // waypoints a .. e: create_graph, all ordered pairs
                for (int i = lane; i < mm * (kOsCap / 32); i += 64) sh.adj[i / (kOsCap / 32)][i % (kOsCap / 32)] = 0u;
                for (int v = lane; v < mm; v += 64) { sh.dist[v] = INFINITY; sh.dist_f[v] = 1; sh.done[v] = 0; sh.prev[v] = -1; }
                __syncthreads();
                for (int q = lane; q < mm * mm; q += 64) {
                    const int i = q / mm, j = q - i * mm;
                    int c = 0;
                    if (os_edge_d<D>(m, sh.P.at(a + i), sh.P.at(a + j), c)) atomicOr(&sh.adj[i][j >> 5], 1u << (j & 31));
                    cnt += c;
                }
                if (lane == 0) { sh.dist[0] = 0.0; sh.prev[0] = 0; }         // dist[source] = 0: a Python int, the cost's dtype wins
                __syncthreads();
                // dijkstra (dijkstra.py:49-76): the unvisited waypoint of least distance (lowest index among equals), strict
                // relaxation of its neighbours; entries of infinite distance relax nothing
                while (true) {
                    unsigned long long best = ~0ull;
                    int ties = 0;
                    for (int v = lane; v < mm; v += 64) {
                        if (sh.done[v]) continue;
                        const unsigned long long k = (unsigned long long)__double_as_longlong(sh.dist[v]);   // dist >= 0
                        if (k < best) best = k;
                    }
                    const unsigned long long w = wave_min_u64(best);
                    if (w >= 0x7ff0000000000000ull) break;
                    unsigned long long cand = ~0ull;
                    for (int v = lane; v < mm; v += 64) {
                        if (sh.done[v] || (unsigned long long)__double_as_longlong(sh.dist[v]) != w) continue;
                        if (cand == ~0ull) cand = (unsigned long long)v;
                        ++ties;
                    }
                    const int u = (int)wave_min_u64(cand);
                    ties += __shfl_xor(ties, 32, 64); ties += __shfl_xor(ties, 16, 64); ties += __shfl_xor(ties, 8, 64);
                    ties += __shfl_xor(ties, 4, 64); ties += __shfl_xor(ties, 2, 64); ties += __shfl_xor(ties, 1, 64);
                    if (ties > 1) status |= kStTie;
                    const double du = __longlong_as_double((long long)w);
                    const bool du_f = sh.dist_f[u] != 0;
                    const OsPt pu = sh.P.at(a + u);
                    __syncthreads();
                    if (lane == 0) sh.done[u] = 1;
                    for (int v = lane; v < mm; v += 64) {
                        if (!((sh.adj[u][v >> 5] >> (v & 31)) & 1u)) continue;
                        bool cf, af;
                        const double c = os_norm_d<D>(pu, sh.P.at(a + v), cf);
                        const double alt = os_add(du, du_f, c, cf, af);
                        if (alt < sh.dist[v]) { sh.dist[v] = alt; sh.dist_f[v] = af ? 1 : 0; sh.prev[v] = (short)u; }
                    }
                    __syncthreads();
                }
                // walk back from path[next]; an unreached waypoint is the reference's KeyError inside its try
                int steps = 0;
                for (int cur = mm - 1; cur != 0; cur = sh.prev[cur]) {
                    if (sh.prev[cur] < 0 || steps >= mm) { failed = true; break; }
                    ++steps;
                }
                if (failed || new_len + steps > kOsCap) { failed = true; break; }
                if (lane == 0) {
                    int k = new_len + steps - 1;
                    for (int cur = mm - 1; cur != 0; cur = sh.prev[cur], --k) sh.N.set(k, sh.P.at(a + cur), sh.P.src[a + cur]);
                }
                new_len += steps;
                a = e;
                __syncthreads();
            }
            if (failed) { status |= kStUnreachable; break; }                 // the path as it stood before this round
            __syncthreads();
            for (int i = lane; i < new_len; i += 64) sh.P.set(i, sh.N.at(i), sh.N.src[i]);
            len = new_len;
            __syncthreads();
            if (len == n0) break;
        }

        if ((last && p.stop == 2) || !p.ratio) {                             // joint_smoother: the pruned path goes on
            for (int i = lane; i < len; i += 64) sh.R.set(i, sh.P.at(i), i);
            n = len;
            __syncthreads();
            continue;
        }
        // ---- re-spacing (smoother.py:140-150): the reference finds the kept waypoints again by value, scanning forwards
        bool ordered = true;
        for (int k = lane; k + 1 < len; k += 64) ordered = ordered && sh.P.src[k + 1] > sh.P.src[k];
        if (!__all(ordered)) { status |= kStOrder; break; }
        for (int k = 0; k + 1 < len; ++k) {
            const int sa = sh.P.src[k], sb = sh.P.src[k + 1];
            const OsPt A = sh.R.at(sa), B = sh.R.at(sb);
            const bool f = A.f && B.f;
            for (int i = sa + 1 + lane; i < sb; i += 64)
                sh.R.set(i, OsPt{os_lerp(A.x, B.x, f, i - sa, sb - sa), os_lerp(A.y, B.y, f, i - sa, sb - sa),
                                 D == 3 ? os_lerp(A.z, B.z, f, i - sa, sb - sa) : 0.0, f}, i);
        }
        __syncthreads();
    }

    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        out[D * i] = sh.R.x[i]; out[D * i + 1] = sh.R.y[i];
        if (D == 3) out[D * i + 2] = sh.R.z[i];
        out_f[i] = sh.R.f[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) { p.status[b] = status | sh.status; p.checks[b] = cnt; p.out_len[b] = n; }
}

hipError_t launch_oracle_smooth(const OracleSmoothParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    if (p.dim == 3) hipLaunchKernelGGL(oracle_smooth_kernel<3>, dim3(p.B), dim3(64), 0, st, p);
    else hipLaunchKernelGGL(oracle_smooth_kernel<2>, dim3(p.B), dim3(64), 0, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
