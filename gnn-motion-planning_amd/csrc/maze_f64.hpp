// maze_f64.hpp -- MazeEnv's collision checker on float64 states (environment/maze_env.py:236-347), the one copy every device
// kernel uses: the baseline planners (lazysp, rrtstar, bitstar, rrt_tree.hpp, next_plan), the edge labels of the training
// episodes (train_episode_kernels.hip) and the stick robot's float64 queries in maze_kernels.hip.  It holds the point robot's
// _state_fp / _edge_fp with the stackless bisection walk, the stick robot's _stick_in_free_space and its _edge_fp, one lane
// walking the interpolated sticks in order (mz_stick_edge) or the 64 lanes of a wave sharing them (mz_stick_edge_wave), and
// np.linalg.norm's edge cost.  Every in-bounds point query adds one to the caller's count; a caller that reports no count
// passes a variable it discards.  Every helper lives in an unnamed namespace: each kernel file compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "wave64.hpp"

// numpy rounds every float64 operation on its own
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kMzLdsCells = 4096;        // maps up to 64 x 64 are staged into LDS as bytes
constexpr int kMzMaxLevel = 30;          // bisection levels the walk can address (a segment of L1 length <= 4 splits 7 times)

struct MzMaze {
    const unsigned char* occ;            // LDS copy (1 = obstacle) or nullptr
    const double* map;                   // [w, w] row-major map[x][y]
    int w;
};

// all `threads` threads of a block: a map of at most kMzLdsCells cells as bytes in occ (the caller synchronises before the
// first query)
__device__ __forceinline__ void mz_stage(const double* map, int w, unsigned char* occ, int tid, int threads) {
    for (int i = tid; i < w * w; i += threads) occ[i] = map[i] == 0.0 ? 0 : 1;
}
// all lanes: stage the map (64 lanes)
__device__ __forceinline__ MzMaze mz_maze(const double* map, int w, unsigned char* occ, int lane) {
    MzMaze m{nullptr, map, w};
    if (w * w <= kMzLdsCells) {
        mz_stage(map, w, occ, lane, 64);
        m.occ = occ;
    }
    wave_sync();
    return m;
}

// np.linalg.norm(t - s) = sqrt(dot(d, d)); numpy's BLAS dot accumulates left to right with fused multiply-adds
template <int DIM>
__device__ __forceinline__ double mz_cost(const double* s, const double* t) {
    const double d0 = t[0] - s[0], d1 = t[1] - s[1];
    double acc = d0 * d0;
    acc = __builtin_fma(d1, d1, acc);
    if (DIM == 3) { const double d2 = t[2] - s[2]; acc = __builtin_fma(d2, d2, acc); }
    return sqrt(acc);
}

// ---- MazeEnv's checker on float64 states, every in-bounds point query counted (environment/maze_env.py:236-347)
__device__ __forceinline__ int mz_cell(double x, int w) {      // ((x + 1.0) * w / 2.0).astype(int), clipped at w - 1
    const int c = (int)((x + 1.0) * (double)w / 2.0);
    return c > w - 1 ? w - 1 : c;
}
__device__ __forceinline__ bool mz_valid2(double x, double y) { return x >= -1.0 && x <= 1.0 && y >= -1.0 && y <= 1.0; }
__device__ __forceinline__ bool mz_point(const MzMaze& m, double x, double y, int& cnt) {      // _point_in_free_space
    if (!mz_valid2(x, y)) return false;
    cnt += 1;
    const int idx = mz_cell(x, m.w) * m.w + mz_cell(y, m.w);
    return m.occ ? m.occ[idx] == 0 : m.map[idx] == 0.0;
}
// _iterative_check_segment without a stack: the recursion's tree is walked in its own order (a node's midpoint, its left half,
// its right half; nothing after the first blocked midpoint) by (level, index), and a node's end points are recomputed from
// the root -- index bit d from the top: 0 = left half -- with the very (l + r) / 2.0 the recursion applies, so every midpoint
// is the recursion's, bit for bit.  No LDS, no scratch; a node costs `level` halvings (level <= 7 for these mazes).
__device__ __forceinline__ bool mz_segment(const MzMaze& m, double ax, double ay, double bx, double by, int& cnt) {
    int level = 0;
    unsigned idx = 0;
    while (true) {
        double lx = ax, ly = ay, rx = bx, ry = by;
        for (int d = level - 1; d >= 0; --d) {
            const double hx = (lx + rx) / 2.0, hy = (ly + ry) / 2.0;
            if ((idx >> d) & 1u) { lx = hx; ly = hy; } else { rx = hx; ry = hy; }
        }
        const int dc = abs(mz_cell(lx, m.w) - mz_cell(rx, m.w)) + abs(mz_cell(ly, m.w) - mz_cell(ry, m.w));
        const double l1 = fabs(lx - rx) + fabs(ly - ry);
        if (dc > 1 && l1 > 0.05 && level < kMzMaxLevel) {
            if (!mz_point(m, (lx + rx) / 2.0, (ly + ry) / 2.0, cnt)) return false;
            ++level;
            idx <<= 1;                                           // the left half comes first
            continue;
        }
        while (level > 0 && (idx & 1u)) { idx >>= 1; --level; }  // a right half is done: so is its parent
        if (level == 0) return true;
        idx |= 1u;                                               // the right half of the same parent
    }
}
__device__ __forceinline__ bool mz_edge2(const MzMaze& m, double ax, double ay, double bx, double by, int& cnt) {      // _edge_fp, size 2
    if (!mz_valid2(ax, ay) || !mz_valid2(bx, by)) return false;
    if (!mz_point(m, ax, ay, cnt) || !mz_point(m, bx, by, cnt)) return false;
    return mz_segment(m, ax, ay, bx, by, cnt);
}
// stick robot: theta = z / LIMITS[2] * pi, ends = centre -+ (STICK_LENGTH / 2.) * (cos, sin)
__device__ __forceinline__ bool mz_valid3(double x, double y, double z) { return mz_valid2(x, y) && z >= -0.4 && z <= 0.4; }
__device__ __forceinline__ void mz_ends(double x, double y, double z, double& ax, double& ay, double& bx, double& by) {
    const double theta = z / 0.4 * 3.141592653589793;
    const double ox = 0.1 * cos(theta), oy = 0.1 * sin(theta);
    ax = x - ox; ay = y - oy;
    bx = x + ox; by = y + oy;
}
__device__ __forceinline__ bool mz_stick(const MzMaze& m, double x, double y, double z, int& cnt) {                    // _stick_in_free_space
    if (!mz_valid3(x, y, z)) return false;
    double ax, ay, bx, by;
    mz_ends(x, y, z, ax, ay, bx, by);
    if (!mz_point(m, ax, ay, cnt) || !mz_point(m, bx, by, cnt)) return false;
    return mz_segment(m, ax, ay, bx, by, cnt);
}
// The interior of _edge_fp(s, t), size 3: the configurations s + k * 1. / K * disp, k = 1 .. K - 1, with disp = t - s
// (disp[2] wrapped by one period) and K = int(distance(s, t) / 0.015); each is the 2-D _edge_fp of its stick's ends.
struct MzStickSteps { double d0, d1, d2; int K; };
__device__ __forceinline__ MzStickSteps mz_stick_steps(const double* s, const double* t) {
    const double d0 = t[0] - s[0], d1 = t[1] - s[1];
    double d2 = t[2] - s[2];
    if (fabs(d2) > 0.4) d2 = d2 > 0.0 ? d2 - 0.8 : d2 + 0.8;
    // distance(): |t - s|, third coordinate min(|d|, ||d| - 0.8|), sqrt of the left-to-right sum of squares
    const double a0 = fabs(t[0] - s[0]), a1 = fabs(t[1] - s[1]);
    double a2 = fabs(t[2] - s[2]);
    const double w2 = fabs(a2 - 0.8);
    a2 = w2 < a2 ? w2 : a2;
    const double d = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
    return {d0, d1, d2, (int)(d / 0.015)};
}
__device__ __forceinline__ bool mz_stick_step(const MzMaze& m, const double* s, const MzStickSteps& e, int k, int& cnt) {
    const double r = (double)k / (double)e.K;                    // k * 1. / K
    double ax, ay, bx, by;
    mz_ends(s[0] + r * e.d0, s[1] + r * e.d1, s[2] + r * e.d2, ax, ay, bx, by);
    return mz_edge2(m, ax, ay, bx, by, cnt);
}
// _edge_fp(s, t), size 3, by one lane: both end sticks, then the interior configurations in order up to the first blocked one
__device__ __forceinline__ bool mz_stick_edge(const MzMaze& m, const double* s, const double* t, int& cnt) {
    if (!mz_valid3(s[0], s[1], s[2]) || !mz_valid3(t[0], t[1], t[2])) return false;
    if (!mz_stick(m, s[0], s[1], s[2], cnt) || !mz_stick(m, t[0], t[1], t[2], cnt)) return false;
    const MzStickSteps e = mz_stick_steps(s, t);
    for (int k = 1; k < e.K; ++k)
        if (!mz_stick_step(m, s, e, k, cnt)) return false;
    return true;
}
// The same by all 64 lanes; s and t are the same in every lane, and so are the result and `checks`.  The two end
// configurations are checked by every lane alike; the interior configurations go to the lanes, 64 a pass.  Every lane counts
// its own checks and stops at its own first blocked query; the first failing k decides the edge, and the count is what the
// sequential loop spends: all of the k below it plus the failing k's own.  No pass follows a failing one.
__device__ __forceinline__ bool mz_stick_edge_wave(const MzMaze& m, int lane, const double* s, const double* t, long long& checks) {
    if (!mz_valid3(s[0], s[1], s[2]) || !mz_valid3(t[0], t[1], t[2])) return false;
    int c_ends = 0;
    const bool ends_ok = mz_stick(m, s[0], s[1], s[2], c_ends) && mz_stick(m, t[0], t[1], t[2], c_ends);
    checks += c_ends;
    if (!ends_ok) return false;
    const MzStickSteps e = mz_stick_steps(s, t);
    for (int base = 1; base < e.K; base += 64) {
        const int k = base + lane;
        int cnt = 0;
        const bool good = k < e.K ? mz_stick_step(m, s, e, k, cnt) : true;
        const unsigned long long bad = __builtin_amdgcn_ballot_w64(!good);
        const int first = bad ? __builtin_ctzll(bad) : 63;
        checks += wave_sum(lane <= first ? cnt : 0);
        if (bad) return false;
    }
    return true;
}

}  // namespace

}  // namespace gnnmp
