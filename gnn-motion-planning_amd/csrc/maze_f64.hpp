// maze_f64.hpp -- MazeEnv's collision checker on float64 states for the classical baseline planners (lazysp_kernels.hip,
// rrtstar_kernels.hip): the point robot's counted _state_fp / _edge_fp with the stackless bisection walk, the stick robot's
// _stick_in_free_space and its _edge_fp spread over the 64 lanes of a wave (environment/maze_env.py:236-347).  Every helper
// lives in an unnamed namespace: each kernel file compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// numpy rounds every float64 operation on its own
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kLspLdsCells = 4096;       // maps up to 64 x 64 are staged into LDS as bytes
constexpr int kLspMaxLevel = 30;         // bisection levels the walk can address (a segment of L1 length <= 4 splits 7 times)

struct LspMaze {
    const unsigned char* occ;            // LDS copy (1 = obstacle) or nullptr
    const double* map;                   // [w, w] row-major map[x][y]
    int w;
};

__device__ __forceinline__ void lsp_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int lsp_wave_sum(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ unsigned long long lsp_wave_min_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o < k ? o : k;
    }
    return k;
}
// all lanes: stage the map (64 lanes)
__device__ __forceinline__ LspMaze lsp_maze(const double* map, int w, unsigned char* occ, int lane) {
    LspMaze m{nullptr, map, w};
    if (w * w <= kLspLdsCells) {
        for (int i = lane; i < w * w; i += 64) occ[i] = map[i] == 0.0 ? 0 : 1;
        m.occ = occ;
    }
    lsp_sync();
    return m;
}

// np.linalg.norm(t - s) = sqrt(dot(d, d)); numpy's BLAS dot accumulates left to right with fused multiply-adds
template <int DIM>
__device__ __forceinline__ double lsp_cost(const double* s, const double* t) {
    const double d0 = t[0] - s[0], d1 = t[1] - s[1];
    double acc = d0 * d0;
    acc = __builtin_fma(d1, d1, acc);
    if (DIM == 3) { const double d2 = t[2] - s[2]; acc = __builtin_fma(d2, d2, acc); }
    return sqrt(acc);
}

// ---- MazeEnv's checker on float64 states, every in-bounds point query counted (environment/maze_env.py:236-347)
__device__ __forceinline__ int lsp_cell(double x, int w) {      // ((x + 1.0) * w / 2.0).astype(int), clipped at w - 1
    const int c = (int)((x + 1.0) * (double)w / 2.0);
    return c > w - 1 ? w - 1 : c;
}
__device__ __forceinline__ bool lsp_valid2(double x, double y) { return x >= -1.0 && x <= 1.0 && y >= -1.0 && y <= 1.0; }
__device__ __forceinline__ bool lsp_point(const LspMaze& m, double x, double y, int& cnt) {      // _point_in_free_space
    if (!lsp_valid2(x, y)) return false;
    cnt += 1;
    const int idx = lsp_cell(x, m.w) * m.w + lsp_cell(y, m.w);
    return m.occ ? m.occ[idx] == 0 : m.map[idx] == 0.0;
}
// _iterative_check_segment without a stack: the recursion's tree is walked in its own order (a node's midpoint, its left half,
// its right half; nothing after the first blocked midpoint) by (level, index), and a node's end points are recomputed from
// the root -- index bit d from the top: 0 = left half -- with the very (l + r) / 2.0 the recursion applies, so every midpoint
// is the recursion's, bit for bit.  No LDS, no scratch; a node costs `level` halvings (level <= 7 for these mazes).
__device__ __forceinline__ bool lsp_segment(const LspMaze& m, double ax, double ay, double bx, double by, int& cnt) {
    int level = 0;
    unsigned idx = 0;
    while (true) {
        double lx = ax, ly = ay, rx = bx, ry = by;
        for (int d = level - 1; d >= 0; --d) {
            const double hx = (lx + rx) / 2.0, hy = (ly + ry) / 2.0;
            if ((idx >> d) & 1u) { lx = hx; ly = hy; } else { rx = hx; ry = hy; }
        }
        const int dc = abs(lsp_cell(lx, m.w) - lsp_cell(rx, m.w)) + abs(lsp_cell(ly, m.w) - lsp_cell(ry, m.w));
        const double l1 = fabs(lx - rx) + fabs(ly - ry);
        if (dc > 1 && l1 > 0.05 && level < kLspMaxLevel) {
            if (!lsp_point(m, (lx + rx) / 2.0, (ly + ry) / 2.0, cnt)) return false;
            ++level;
            idx <<= 1;                                           // the left half comes first
            continue;
        }
        while (level > 0 && (idx & 1u)) { idx >>= 1; --level; }  // a right half is done: so is its parent
        if (level == 0) return true;
        idx |= 1u;                                               // the right half of the same parent
    }
}
__device__ __forceinline__ bool lsp_edge2(const LspMaze& m, double ax, double ay, double bx, double by, int& cnt) {      // _edge_fp, size 2
    if (!lsp_valid2(ax, ay) || !lsp_valid2(bx, by)) return false;
    if (!lsp_point(m, ax, ay, cnt) || !lsp_point(m, bx, by, cnt)) return false;
    return lsp_segment(m, ax, ay, bx, by, cnt);
}
// stick robot: theta = z / LIMITS[2] * pi, ends = centre -+ (STICK_LENGTH / 2.) * (cos, sin)
__device__ __forceinline__ bool lsp_valid3(double x, double y, double z) { return lsp_valid2(x, y) && z >= -0.4 && z <= 0.4; }
__device__ __forceinline__ void lsp_ends(double x, double y, double z, double& ax, double& ay, double& bx, double& by) {
    const double theta = z / 0.4 * 3.141592653589793;
    const double ox = 0.1 * cos(theta), oy = 0.1 * sin(theta);
    ax = x - ox; ay = y - oy;
    bx = x + ox; by = y + oy;
}
__device__ __forceinline__ bool lsp_stick(const LspMaze& m, double x, double y, double z, int& cnt) {                    // _stick_in_free_space
    if (!lsp_valid3(x, y, z)) return false;
    double ax, ay, bx, by;
    lsp_ends(x, y, z, ax, ay, bx, by);
    if (!lsp_point(m, ax, ay, cnt) || !lsp_point(m, bx, by, cnt)) return false;
    return lsp_segment(m, ax, ay, bx, by, cnt);
}
// _edge_fp(s, t), size 3, by all 64 lanes; s and t are the same in every lane, and so are the result and `checks`.  The two
// end configurations are checked by every lane alike; the interior configurations k = 1 .. K - 1 go to the lanes, 64 a pass.
// Every lane counts its own checks and stops at its own first blocked query; the first failing k decides the edge, and the
// count is what the sequential loop spends: all of the k below it plus the failing k's own.  No pass follows a failing one.
__device__ __forceinline__ bool lsp_stick_edge_wave(const LspMaze& m, int lane, const double* s, const double* t, long long& checks) {
    if (!lsp_valid3(s[0], s[1], s[2]) || !lsp_valid3(t[0], t[1], t[2])) return false;
    int c_ends = 0;
    const bool ends_ok = lsp_stick(m, s[0], s[1], s[2], c_ends) && lsp_stick(m, t[0], t[1], t[2], c_ends);
    checks += c_ends;
    if (!ends_ok) return false;
    const double d0 = t[0] - s[0], d1 = t[1] - s[1];
    double d2 = t[2] - s[2];
    if (fabs(d2) > 0.4) d2 = d2 > 0.0 ? d2 - 0.8 : d2 + 0.8;
    // distance(): |t - s|, third coordinate min(|d|, ||d| - 0.8|), sqrt of the left-to-right sum of squares
    const double a0 = fabs(t[0] - s[0]), a1 = fabs(t[1] - s[1]);
    double a2 = fabs(t[2] - s[2]);
    const double w2 = fabs(a2 - 0.8);
    a2 = w2 < a2 ? w2 : a2;
    const double d = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
    const int K = (int)(d / 0.015);
    for (int base = 1; base < K; base += 64) {
        const int k = base + lane;
        int cnt = 0;
        bool good = true;
        if (k < K) {
            const double r = (double)k / (double)K;              // k * 1. / K
            double ax, ay, bx, by;
            lsp_ends(s[0] + r * d0, s[1] + r * d1, s[2] + r * d2, ax, ay, bx, by);
            good = lsp_edge2(m, ax, ay, bx, by, cnt);
        }
        const unsigned long long bad = __builtin_amdgcn_ballot_w64(!good);
        const int first = bad ? __builtin_ctzll(bad) : 63;
        checks += lsp_wave_sum(lane <= first ? cnt : 0);
        if (bad) return false;
    }
    return true;
}

}  // namespace

}  // namespace gnnmp
