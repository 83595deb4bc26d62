// next3d_pb.hpp -- the 3-D NEXT planning network (the arm families) for one workgroup: the layout of the packed weights, the
// attention, the tile helpers (conv27, store_rows) and the bodies of the problem-side kernels as templates.  next3d_kernels.hip
// instantiates them without saving (the inference kernels: same arithmetic in the same order, same registers and LDS as before
// the bodies moved here); next3d_train_kernels.hip instantiates SAVE = true, where round r reads h and c of slot r and writes
// slot r + 1 and the conv output of the round is kept too, and shares conv27 for the transposed convolutions of the backward.
// Every helper lives in an unnamed namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"

namespace gnnmp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kW = 15, kV = kW * kW * kW, kLat = 64;
constexpr int kRows = kV + 1, kZeroRow = kV;     // rows of a workspace buffer; the last one stays zero
constexpr int kXC = 16;                          // channels of an x9 row (9 used)
constexpr int kMT = 2, kWaves = 4, kThreads = 64 * kWaves, kTileV = 16 * kMT * kWaves, kTiles = (kV + kTileV - 1) / kTileV;
constexpr int kLS = 68;                          // LDS row stride in floats: 16-byte aligned, rows 4 banks apart
constexpr int kAtThreads = 512;                 // attention and read-out: 8 waves, seven voxels a thread
constexpr int kIn1 = 12, kMIn = 16, kPOut = 16;    // padded widths: first attention layer's inputs (point_dim + 3 <= 9), the
                                                 // a3 MLP's inputs (dim <= 15), the policy's outputs (dim + 1 <= 16)
constexpr int kF64Rounds = 1;                    // LSTM rounds that accumulate in double (see next3d_round_kernel)

// workspace of one problem, in floats
constexpr size_t wsX9 = 0, wsHL = wsX9 + (size_t)kRows * kXC, wsHA = wsHL + (size_t)kRows * kLat, wsHB = wsHA + (size_t)kRows * kLat,
                 wsC = wsHB + (size_t)kRows * kLat, kWsFloats = wsC + (size_t)kRows * kLat;

// packed weights (floats), one layout for every (dim, point_dim); gnnmp.next_model3d.pack_weights writes this order
constexpr int oW1 = 0, oB1 = oW1 + 16 * kIn1, oW2 = oB1 + 16, oB2 = oW2 + 256, oW3 = oB2 + 16, oB3 = oW3 + 512, oW4 = oB3 + 32,
              oB4 = oW4 + 1024, oW5 = oB4 + 32, oB5 = oW5 + 2048, oW6 = oB5 + 64, oB6 = oW6 + 64, oM1 = oB6 + 4,
              oMB1 = oM1 + 64 * kMIn, oM2 = oMB1 + 64, oMB2 = oM2 + 512, oP1 = oMB2 + 8, oPB1 = oP1 + 1024, oP2 = oPB1 + 128,
              oPB2 = oP2 + 8192, oP3 = oPB2 + 64, oPB3 = oP3 + kPOut * 64, oHidW = oPB3 + kPOut, oHidB = oHidW + 27 * 1024,
              oH0W = oHidB + 64, oH0B = oH0W + 108 * 1024, oC0W = oH0B + 64, oC0B = oC0W + 108 * 1024, oCvW = oC0B + 64,
              oCvB = oCvW + 108 * 1024, oLsW = oCvB + 64, oLsB = oLsW + 8 * 16 * 256, kWeightFloats = oLsB + 256;
static_assert(oHidW % 4 == 0 && oH0W % 4 == 0 && oC0W % 4 == 0 && oCvW % 4 == 0 && oLsW % 4 == 0, "16-byte weight loads");
static_assert(wsHL % 4 == 0 && wsHA % 4 == 0 && wsHB % 4 == 0 && wsC % 4 == 0 && kWsFloats % 4 == 0, "16-byte row loads");

__device__ __forceinline__ double relu(double v) { return v > 0. ? v : 0.; }
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the shared MLP of the attention behind its first layer, for one voxel: `a` = the first layer's 16 outputs (after ReLU) -> the
// logit.  In double, as in the 2-D network: the logits reach tens and the recurrent rounds amplify an error in exp().
__device__ __forceinline__ double attn_tail(const float* __restrict__ W, const double (&a)[16]) {
    double b[16], c[32], d[32];
#pragma unroll
    for (int o = 0; o < 16; ++o) {
        double v = W[oB2 + o];
#pragma unroll
        for (int i = 0; i < 16; ++i) v = fma((double)W[oW2 + o * 16 + i], a[i], v);
        b[o] = relu(v);
    }
#pragma unroll
    for (int o = 0; o < 32; ++o) {
        double v = W[oB3 + o];
#pragma unroll
        for (int i = 0; i < 16; ++i) v = fma((double)W[oW3 + o * 16 + i], b[i], v);
        c[o] = relu(v);
    }
#pragma unroll
    for (int o = 0; o < 32; ++o) {
        double v = W[oB4 + o];
#pragma unroll
        for (int i = 0; i < 32; ++i) v = fma((double)W[oW4 + o * 32 + i], c[i], v);
        d[o] = relu(v);
    }
    double logit = W[oB6];
#pragma unroll 2
    for (int o = 0; o < 64; ++o) {             // layer 5 output o goes straight into the last layer's dot product
        double v = W[oB5 + o];
#pragma unroll
        for (int i = 0; i < 32; ++i) v = fma((double)W[oW5 + o * 32 + i], d[i], v);
        logit = fma((double)W[oW6 + o], relu(v), logit);
    }
    return logit;
}

// LDS scratch of one attention, in doubles
struct AttnScratch {
    double base[16];                           // first layer: bias + the point's part, the same for every voxel
    double red[kAtThreads / 64], sum[kAtThreads / 64];
    double z[64], o[8], a3[8];
};

// The attention of one input row [point (pd), state (dim)] for a workgroup of NT threads (kAtThreads; 256 in the training
// backward), in double: a123 of every voxel in a123[] (LDS; thread tid owns voxels tid + q NT and may read those back without a
// barrier), a3[8] in s.a3, the dim-64-8 MLP's hidden layer in s.z, the first shared layer's point part in s.base.  Voxel
// v = (i 15 + j) 15 + k enters as [point, j, i, k].  The voxel loop stays rolled and keeps its logits in LDS, not in registers.
template <int NT = kAtThreads>
__device__ __forceinline__ void attention3d(const float* __restrict__ W, const float* inp, int dim, int pd, int tid, AttnScratch& s,
                                            double* a123) {
    constexpr int NWV = NT / 64;
    if (tid < 16) {
        double v = W[oB1 + tid];
        for (int q = 0; q < pd; ++q) v = fma((double)W[oW1 + tid * kIn1 + q], (double)inp[q], v);
        s.base[tid] = v;
    }
    if (tid >= 64 && tid < 128) {
        const int o = tid - 64;
        double v = W[oMB1 + o];
        for (int q = 0; q < dim; ++q) v = fma((double)W[oM1 + o * kMIn + q], (double)inp[pd + q], v);
        s.z[o] = relu(v);
    }
    __syncthreads();
    if (tid < 8) {
        double v = W[oMB2 + tid];
        for (int i = 0; i < 64; ++i) v = fma((double)W[oM2 + tid * 64 + i], s.z[i], v);
        s.o[tid] = v;
    }
    double mx = -INFINITY;
#pragma unroll 1
    for (int v = tid; v < kV; v += NT) {
        const int i = v / (kW * kW), j = (v / kW) % kW, k = v % kW;
        // the weights are re-read (scalar loads, cached) for every voxel: were the pointer visibly loop-invariant, the compiler
        // would hoist all 4 k converted weights out of the loop and spill them
        const float* Wv = W;
        asm volatile("" : "+s"(Wv));
        double l1[16];
#pragma unroll
        for (int o = 0; o < 16; ++o)
            l1[o] = relu(fma((double)Wv[oW1 + o * kIn1 + pd + 2], (double)k, fma((double)Wv[oW1 + o * kIn1 + pd + 1], (double)i,
                         fma((double)Wv[oW1 + o * kIn1 + pd], (double)j, s.base[o]))));
        const double logit = attn_tail(Wv, l1);
        a123[v] = logit;
        mx = fmax(mx, logit);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) s.red[tid >> 6] = mx;
    __syncthreads();
    mx = s.red[0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) mx = fmax(mx, s.red[w]);
    double e = 0.;
    for (int v = tid; v < kV; v += NT) {
        const double ev = exp(a123[v] - mx);
        a123[v] = ev;
        e += ev;
    }
    e = wave_sum(e);
    if ((tid & 63) == 0) s.sum[tid >> 6] = e;
    if (tid < 8) {
        double m8 = s.o[0];
        for (int i = 1; i < 8; ++i) m8 = fmax(m8, s.o[i]);
        double den = 0.;
        for (int i = 0; i < 8; ++i) den += exp(s.o[i] - m8);
        s.a3[tid] = exp(s.o[tid] - m8) / den;
    }
    __syncthreads();
    double tot = 0.;
#pragma unroll
    for (int w = 0; w < NWV; ++w) tot += s.sum[w];
    for (int v = tid; v < kV; v += NT) a123[v] = a123[v] / tot;
}

// this lane's voxel in row tile m of the wave as (i << 8 | j << 4 | k), -1 behind the last voxel
__device__ __forceinline__ int lane_cell(int tile, int wave, int m, int lane) {
    const int v = tile * kTileV + (wave * kMT + m) * 16 + (lane & 15);
    return v < kV ? ((v / (kW * kW)) << 8 | ((v / kW) % kW) << 4 | (v % kW)) : -1;
}

// row of the voxel that tap (di, dj, dk) = (tap / 9, tap / 3 % 3, tap % 3) of a cell reads: the neighbour, or the zero row
__device__ __forceinline__ int nbr_row(int cell, int tap) {
    const int di = tap / 9, dj = (tap / 3) % 3, dk = tap % 3;
    const int i = (cell >> 8) + di - 1, j = ((cell >> 4) & 15) + dj - 1, k = (cell & 15) + dk - 1;
    const bool in = cell >= 0 && i >= 0 && i < kW && j >= 0 && j < kW && k >= 0 && k < kW;
    return in ? (i * kW + j) * kW + k : kZeroRow;
}

typedef double f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f64x4 mfma4(float a, float b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64((double)a, (double)b, c, 0, 0, 0);
}
template <typename ACC> struct elem_of;
template <> struct elem_of<f32x4> { typedef float type; };
template <> struct elem_of<f64x4> { typedef double type; };
// row of a 16 x 16 result tile that register r of lane l holds (the column is l & 15): the two instructions differ
template <typename ACC> __device__ __forceinline__ int acc_row(int lane, int r);
template <> __device__ __forceinline__ int acc_row<f32x4>(int lane, int r) { return 4 * (lane >> 4) + r; }
template <> __device__ __forceinline__ int acc_row<f64x4>(int lane, int r) { return 4 * r + (lane >> 4); }

// ---- 3 x 3 x 3 convolution of the wave's two row tiles: acc[m][nt] = bias + sum over 27 taps x CG channel groups of 16; src rows
// of STRIDE floats in global memory.  ACC = f32x4: exact fp32 MFMA, as a two-level sum -- the three taps of one (di, dj) go into
// a fresh accumulator which then joins the total: nine chains of 192 and a sum of nine.  ACC = f64x4: the same operands through
// v_mfma_f64_16x16x4_f64 (same lane layout, half the rate), one chain: for the stretches whose sums are large (|h0| reaches 258:
// one fp32 chain over K = 1728 was 3.6e-4 off there, the two-level sum 4e-5, the reference's own fp32 run 9e-5).
template <int CG, int STRIDE, typename ACC>
__device__ __forceinline__ void conv27(const float* __restrict__ src, const float* __restrict__ wk, const float* __restrict__ bias,
                                       const int (&cell)[kMT], int lane, ACC (&acc)[kMT][4]) {
    typedef typename elem_of<ACC>::type T;
    constexpr bool two_level = sizeof(T) == 4;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const T bv = bias[nt * 16 + (lane & 15)];
#pragma unroll
        for (int m = 0; m < kMT; ++m) acc[m][nt] = ACC{bv, bv, bv, bv};
    }
    const f32x4* wv = reinterpret_cast<const f32x4*>(wk) + lane;
    const int koff = 4 * (lane >> 4);
#pragma unroll 1
    for (int grp = 0; grp < 9; ++grp) {
        ACC part[kMT][4];
#pragma unroll
        for (int m = 0; m < kMT; ++m)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) part[m][nt] = two_level ? ACC{0, 0, 0, 0} : acc[m][nt];
#pragma unroll 1
        for (int dk = 0; dk < 3; ++dk) {         // rolled: one tap's operands in flight
            const int tap = grp * 3 + dk;
            const float* row[kMT];
#pragma unroll
            for (int m = 0; m < kMT; ++m) row[m] = src + (size_t)nbr_row(cell[m], tap) * STRIDE + koff;
#pragma unroll
            for (int cg = 0; cg < CG; ++cg) {
                f32x4 a[kMT], bw[4];
#pragma unroll
                for (int m = 0; m < kMT; ++m) a[m] = *reinterpret_cast<const f32x4*>(row[m] + cg * 16);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) bw[nt] = wv[((tap * CG + cg) * 4 + nt) * 64];
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int m = 0; m < kMT; ++m) part[m][nt] = mfma4(a[m][s], bw[nt][s], part[m][nt]);
            }
        }
#pragma unroll
        for (int m = 0; m < kMT; ++m)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[m][nt] = two_level ? acc[m][nt] + part[m][nt] : part[m][nt];
    }
}

// accumulator tiles -> channel-last rows in global memory: lane l, register r of column tile nt is (row acc_row(l, r), column
// 16 nt + (l & 15)); rows behind the last voxel are not written
template <typename ACC>
__device__ __forceinline__ void store_rows(float* dst, const ACC (&acc)[kMT][4], int tile, int wave, int lane) {
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = tile * kTileV + (wave * kMT + m) * 16 + acc_row<ACC>(lane, r);
            if (v < kV) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) dst[(size_t)v * kLat + nt * 16 + (lane & 15)] = (float)acc[m][nt][r];
            }
        }
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

constexpr int kRoundLdsFloats = kWaves * kMT * 16 * kLS;

// ---- the bodies --------------------------------------------------------------------------------------------------------------
// the goal attention of problem b -> its x9 rows [voxel][16] = [map, a3[cap] a123[voxel], 0 x 7] and x9's zero row
__device__ __forceinline__ void next3d_x9_body(const Next3dPbParams& p, int b, float* x9, AttnScratch& sc, double* a123, int tid) {
    attention3d(p.weights, p.goals + (size_t)b * (p.pd + p.dim), p.dim, p.pd, tid, sc, a123);
    for (int v = tid; v < kV; v += kAtThreads) {
        const double a = a123[v];
        float* row = x9 + (size_t)v * kXC;
        f32x4 r0, r1, r2 = f32x4{0.f, 0.f, 0.f, 0.f};
        r0[0] = p.maps[(size_t)b * kV + v];
        r0[1] = (float)(sc.a3[0] * a); r0[2] = (float)(sc.a3[1] * a); r0[3] = (float)(sc.a3[2] * a);
        r1[0] = (float)(sc.a3[3] * a); r1[1] = (float)(sc.a3[4] * a); r1[2] = (float)(sc.a3[5] * a);
        r1[3] = (float)(sc.a3[6] * a);
        r2[0] = (float)(sc.a3[7] * a);
        reinterpret_cast<f32x4*>(row)[0] = r0;
        reinterpret_cast<f32x4*>(row)[1] = r1;
        reinterpret_cast<f32x4*>(row)[2] = r2;
        reinterpret_cast<f32x4*>(row)[3] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // the zero row: what a voxel outside the map reads
    if (tid < kXC) x9[(size_t)kZeroRow * kXC + tid] = 0.f;
}

__device__ __forceinline__ void next3d_hidden_body(const float* __restrict__ W, const float* x9, float* hl, int tile, int lane, int wave) {
    int cell[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) cell[m] = lane_cell(tile, wave, m, lane);
    f64x4 acc[kMT][4];
    conv27<1, kXC>(x9, W + oHidW, W + oHidB, cell, lane, acc);
    store_rows(hl, acc, tile, wave, lane);
}

__device__ __forceinline__ void next3d_h0c0_body(const float* __restrict__ W, const float* hl, float* h, float* c, int tile, int lane,
                                                 int wave) {
    int cell[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) cell[m] = lane_cell(tile, wave, m, lane);
    f64x4 acc[kMT][4];
    conv27<4, kLat>(hl, W + oC0W, W + oC0B, cell, lane, acc);
    store_rows(c, acc, tile, wave, lane);
    conv27<4, kLat>(hl, W + oH0W, W + oH0B, cell, lane, acc);
    store_rows(h, acc, tile, wave, lane);
}

// one round of a tile for the training forward: h_in -> h_out, c_in -> c_out, four different buffers; the text of
// next3d_round_kernel (next3d_kernels.hip) with the buffers as arguments.  The inference kernel keeps its own copy: behind a
// function boundary its LDS stores were no longer paired and it took one more VGPR, and its resource figures are pinned
// (profiles/next3d_resources.txt).  The arithmetic and its order are the same, so the bits are.  ACC = f64x4 for the first kF64Rounds rounds, whose h is still h0-sized (all-fp32
// missed the bar at 1 and 2 rounds: profiles/next3d_parity.txt); behind them |h| <= 1 and exact fp32 MFMA holds it.  The gates
// are rounded to fp32 before the transcendentals either way.  The conv output (the floats the gates read) is stored too.
template <typename ACC>
__device__ __forceinline__ void next3d_round_body(const float* W, const float* hin, float* hout,
                                                  const float* cin, float* cout, float* xsave, float* X, int tile, int lane, int wave) {
    typedef typename elem_of<ACC>::type T;
    int cell[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) cell[m] = lane_cell(tile, wave, m, lane);
    float* xw = X + wave * (kMT * 16 * kLS);                    // the wave's own 32 rows
    {
        ACC acc[kMT][4];
        conv27<4, kLat>(hin, W + oCvW, W + oCvB, cell, lane, acc);
#pragma unroll
        for (int m = 0; m < kMT; ++m)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) xw[(m * 16 + acc_row<ACC>(lane, r)) * kLS + nt * 16 + (lane & 15)] = (float)acc[m][nt][r];
        store_rows(xsave, acc, tile, wave, lane);
    }
    __syncthreads();                                            // the wave's x rows are in LDS in the A-operand order
    const f32x4* lw = reinterpret_cast<const f32x4*>(W + oLsW) + lane;
    const int koff = 4 * (lane >> 4);
    const float* hrow[kMT];                                     // the lane's own voxel: the A rows of the h half
#pragma unroll
    for (int m = 0; m < kMT; ++m) {
        const int v = tile * kTileV + (wave * kMT + m) * 16 + (lane & 15);
        hrow[m] = hin + (size_t)(v < kV ? v : kZeroRow) * kLat + koff;
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {                      // hidden units 32 half .. 32 half + 31: column tiles 2 half + t of each gate
        ACC g[kMT][4][2];
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const T bv = W[oLsB + gate * 64 + (2 * half + t) * 16 + (lane & 15)];
#pragma unroll
                for (int m = 0; m < kMT; ++m) g[m][gate][t] = ACC{bv, bv, bv, bv};
            }
#pragma unroll 1
        for (int kg = 0; kg < 8; ++kg) {
            f32x4 a[kMT];
#pragma unroll
            for (int m = 0; m < kMT; ++m)
                a[m] = kg < 4 ? *reinterpret_cast<const f32x4*>(xw + (m * 16 + (lane & 15)) * kLS + kg * 16 + koff)
                              : *reinterpret_cast<const f32x4*>(hrow[m] + (kg & 3) * 16);
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const f32x4 bw = lw[(kg * 16 + gate * 4 + 2 * half + t) * 64];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int m = 0; m < kMT; ++m)
                            g[m][gate][t] = mfma4(a[m][s], bw[s], g[m][gate][t]);
                }
        }
#pragma unroll
        for (int m = 0; m < kMT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = tile * kTileV + (wave * kMT + m) * 16 + acc_row<ACC>(lane, r);
                if (v < kV) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const size_t at = (size_t)v * kLat + (2 * half + t) * 16 + (lane & 15);
                        const float gi = sigmoidf((float)g[m][0][t][r]), gf = sigmoidf((float)g[m][1][t][r]),
                                    gg = tanhf((float)g[m][2][t][r]), go = sigmoidf((float)g[m][3][t][r]);
                        const float c = fmaf(gf, cin[at], gi * gg);
                        cout[at] = c;
                        hout[at] = go * tanhf(c);
                    }
                }
            }
    }
}

struct StateScratch {
    AttnScratch at;
    double a123[kV + 1];
    double T[kLat], x[8], h1[128], h2[64];
};

// the read-out of one input row for a workgroup of kAtThreads threads: the state attention (s.a123, s.at.a3), T[c] = sum_voxel
// a123[voxel] pb[c, voxel], x[g] = sum_cap a3[cap] T[8 g + cap] and the policy MLP's two hidden layers h1, h2, all in double
__device__ __forceinline__ void next3d_state_readout(const float* __restrict__ W, const float* inp, int dim, int pd,
                                                     const float* __restrict__ pb, StateScratch& s, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    attention3d(W, inp, dim, pd, tid, s.at, s.a123);
    __syncthreads();
    for (int c = wave; c < kLat; c += kAtThreads / 64) {        // T[c]: a wave per channel, voxels over the lanes
        double t = 0.;
        for (int q = lane; q < kV; q += 64) t = fma(s.a123[q], (double)pb[(size_t)c * kV + q], t);
        t = wave_sum(t);
        if (lane == 0) s.T[c] = t;
    }
    __syncthreads();
    if (tid < 8) {
        double x = 0.;
        for (int cap = 0; cap < 8; ++cap) x = fma(s.at.a3[cap], s.T[tid * 8 + cap], x);
        s.x[tid] = x;
    }
    __syncthreads();
    if (tid < 128) {
        double v = (double)W[oPB1 + tid];
        for (int i = 0; i < 8; ++i) v = fma((double)W[oP1 + tid * 8 + i], s.x[i], v);
        s.h1[tid] = v > 0. ? v : 0.;
    }
    __syncthreads();
    if (tid < 256) {
        const int j = tid >> 2, part = tid & 3;                 // 64 outputs, four threads each
        double v = 0.;
        for (int i = part; i < 128; i += 4) v = fma((double)W[oP2 + j * 128 + i], s.h1[i], v);
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += (double)W[oPB2 + j];
        if (part == 0) s.h2[j] = v > 0. ? v : 0.;
    }
    __syncthreads();
}

}  // namespace
}  // namespace gnnmp
