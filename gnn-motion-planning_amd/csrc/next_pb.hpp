// next_pb.hpp -- the problem half of the NEXT planning network for one workgroup: the tile helpers (conv3, store_tiles) and
// the body of next_pb_kernel as a template.  next_kernels.hip instantiates it without saving (the inference kernel, same
// arithmetic in the same order as before the body moved here); next_train_kernels.hip instantiates SAVE = true, which also
// stores what the backward needs -- x9, the hidden layer, every round's h and c going in and the conv output -- as [cell][channel]
// rows, and shares conv3 for the transposed convolutions of the backward.  Every helper lives in an unnamed namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "next_net.hpp"

namespace gnnmp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLS = 68;                        // LDS row stride in floats: 16-byte aligned, rows 4 banks apart
constexpr int kZeroRow = 256;                  // a row of zeros behind the 16 row tiles
constexpr int kBufFloats = (kZeroRow + 1) * kLS;
constexpr int kPbThreads = 512, kMT = 2;       // 8 waves, two row tiles each

static_assert(kBufFloats % 2 == 0, "the doubles behind the two buffers");
static_assert(oHidW % 4 == 0 && oH0W % 4 == 0 && oC0W % 4 == 0 && oCvW % 4 == 0 && oLsW % 4 == 0, "16-byte weight loads");

// LDS float offset of the row that tap (ky, kx) = (tap / 3, tap % 3) of a cell reads: the neighbour cell, or the zero row
__device__ __forceinline__ int nbr_row(int cell, int tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int rr = (cell >> 8) + ky - 1, cc = (cell & 255) + kx - 1;
    const bool in = cell >= 0 && rr >= 0 && rr < kW && cc >= 0 && cc < kW;
    return (in ? rr * kW + cc : kZeroRow) * kLS;
}

// ---- 3 x 3 convolution of the wave's two row tiles: acc[m][nt] = bias + sum over 9 taps x CG channel groups of 16 ---------------
template <int CG>
__device__ __forceinline__ void conv3(const float* src, const float* __restrict__ wk, const float* __restrict__ bias,
                                      const int (&cell)[kMT], int lane, f32x4 (&acc)[kMT][4]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const float bv = bias[nt * 16 + (lane & 15)];
#pragma unroll
        for (int m = 0; m < kMT; ++m) acc[m][nt] = f32x4{bv, bv, bv, bv};
    }
    const f32x4* wv = reinterpret_cast<const f32x4*>(wk) + lane;
    const int koff = 4 * (lane >> 4);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {          // rolled: one tap's operands in flight, not the whole convolution's
        int row[kMT];
#pragma unroll
        for (int m = 0; m < kMT; ++m) row[m] = nbr_row(cell[m], tap);
#pragma unroll
        for (int cg = 0; cg < CG; ++cg) {
            f32x4 a[kMT], bw[4];
#pragma unroll
            for (int m = 0; m < kMT; ++m) a[m] = *reinterpret_cast<const f32x4*>(src + row[m] + cg * 16 + koff);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) bw[nt] = wv[((tap * CG + cg) * 4 + nt) * 64];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int m = 0; m < kMT; ++m)
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], bw[nt][s], acc[m][nt], 0, 0, 0);
        }
    }
}

// accumulator tiles -> LDS rows: lane l, register r of column tile nt is (row 4 (l >> 4) + r, column 16 nt + (l & 15))
__device__ __forceinline__ void store_tiles(float* dst, const f32x4 (&acc)[kMT][4], int wave, int lane) {
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                dst[((wave * kMT + m) * 16 + 4 * (lane >> 4) + r) * kLS + nt * 16 + (lane & 15)] = acc[m][nt][r];
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// accumulator tiles -> the saved [cell][64] rows of one problem; the padding cells (rows 225..255) are not stored.  The rounds of
// next_pb_body run at the register limit: addresses hoisted out of the round loop would spill
__device__ __forceinline__ void save_tiles(float* dst, const f32x4 (&acc)[kMT][4], int wave, int lane) {
    asm volatile("" : "+v"(lane), "+v"(wave));                // opaque: the addresses are formed here, not kept across a round
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (wave * kMT + m) * 16 + 4 * (lane >> 4) + r;
                if (row < kCells) dst[row * kLat + nt * 16 + (lane & 15)] = acc[m][nt][r];
            }
}

// the 225 real rows of an LDS buffer -> the saved [cell][64] rows, 16 bytes a lane, by the whole workgroup
__device__ __forceinline__ void save_rows(float* dst, const float* src, int tid) {
    asm volatile("" : "+v"(tid));
#pragma unroll 1
    for (int i = tid; i < kCells * 16; i += kPbThreads)
        *reinterpret_cast<f32x4*>(dst + (i >> 4) * kLat + (i & 15) * 4) = *reinterpret_cast<const f32x4*>(src + (i >> 4) * kLS + (i & 15) * 4);
}

// this problem's saved rows (SAVE only): x9 [225][16], hl [225][64], H [iters + 1][225][64], C and X [iters][225][64]
struct NextPbSave {
    float *x9, *hl, *H, *C, *X;
};

template <bool SAVE>
__device__ __forceinline__ void next_pb_body(const NextPbParams& p, const NextPbSave& sv, float* lds) {
    float* H = lds;
    float* X = lds + kBufFloats;
    double* s_red = reinterpret_cast<double*>(X + kBufFloats);      // 16 + 64 + 8 doubles (2 kBufFloats is even: 8-aligned)
    double* s_a3 = s_red + 88;                                      // 8 doubles
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ W = p.weights;

    for (int i = tid; i < 2 * kBufFloats; i += kPbThreads) lds[i] = 0.f;
    __syncthreads();

    // x9 = [map, goal attention], channels 9..15 stay zero
    const double a12 = attention<kPbThreads>(W, p.goals + (size_t)b * p.dim, p.dim, tid, s_red, s_a3);
    if (tid < kCells) {
        X[tid * kLS] = p.maps[(size_t)b * kCells + tid];
#pragma unroll
        for (int c = 0; c < 8; ++c) X[tid * kLS + 1 + c] = (float)(s_a3[c] * a12);
        if constexpr (SAVE) {
#pragma unroll
            for (int c = 0; c < 16; ++c) sv.x9[tid * 16 + c] = X[tid * kLS + c];
        }
    }
    // this lane's cell in each of the wave's row tiles as (row << 8 | column), -1 for the padding cells
    int nbr[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) {
        const int cellid = (wave * kMT + m) * 16 + (lane & 15);
        nbr[m] = cellid < kCells ? ((cellid / kW) << 8 | (cellid % kW)) : -1;
    }
    __syncthreads();

    f32x4 acc[kMT][4], cst[kMT][4];
    conv3<1>(X, W + oHidW, W + oHidB, nbr, lane, acc);          // hidden
    store_tiles(H, acc, wave, lane);
    if constexpr (SAVE) save_tiles(sv.hl, acc, wave, lane);
    __syncthreads();
    conv3<4>(H, W + oC0W, W + oC0B, nbr, lane, cst);            // c0: stays in registers
    conv3<4>(H, W + oH0W, W + oH0B, nbr, lane, acc);            // h0
    __syncthreads();                                            // every wave has read the hidden layer
    store_tiles(H, acc, wave, lane);
    __syncthreads();

    const f32x4* lw = reinterpret_cast<const f32x4*>(W + oLsW) + lane;
    const int koff = 4 * (lane >> 4);
    for (int it = 0; it < p.iters; ++it) {
        if constexpr (SAVE) {                                   // h (from LDS, complete since the last barrier) and c going into the round
            save_rows(sv.H + (size_t)it * (kCells * kLat), H, tid);
            save_tiles(sv.C + (size_t)it * (kCells * kLat), cst, wave, lane);
        }
        conv3<4>(H, W + oCvW, W + oCvB, nbr, lane, acc);
        store_tiles(X, acc, wave, lane);                        // own rows: the A operand of the LSTM product
        __syncthreads();                                        // and every wave has read h
        if constexpr (SAVE) save_rows(sv.X + (size_t)it * (kCells * kLat), X, tid);
        f32x4 hn[kMT][4];
#pragma unroll
        for (int half = 0; half < 2; ++half) {                  // hidden units 32 half .. 32 half + 31: column tiles 2 half + t of each gate
            f32x4 g[kMT][4][2];
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float bv = W[oLsB + gate * 64 + (2 * half + t) * 16 + (lane & 15)];
#pragma unroll
                    for (int m = 0; m < kMT; ++m) g[m][gate][t] = f32x4{bv, bv, bv, bv};
                }
#pragma unroll 1
            for (int kg = 0; kg < 8; ++kg) {
                const float* src = kg < 4 ? X : H;
                f32x4 a[kMT];
#pragma unroll
                for (int m = 0; m < kMT; ++m)
                    a[m] = *reinterpret_cast<const f32x4*>(src + ((wave * kMT + m) * 16 + (lane & 15)) * kLS + (kg & 3) * 16 + koff);
#pragma unroll
                for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const f32x4 bw = lw[(kg * 16 + gate * 4 + 2 * half + t) * 64];
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int m = 0; m < kMT; ++m)
                                g[m][gate][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], bw[s], g[m][gate][t], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int m = 0; m < kMT; ++m)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float gi = sigmoidf(g[m][0][t][r]), gf = sigmoidf(g[m][1][t][r]), gg = tanhf(g[m][2][t][r]),
                                    go = sigmoidf(g[m][3][t][r]);
                        const float c = fmaf(gf, cst[m][2 * half + t][r], gi * gg);
                        cst[m][2 * half + t][r] = c;
                        hn[m][2 * half + t][r] = go * tanhf(c);
                    }
        }
        store_tiles(H, hn, wave, lane);                         // own rows, after both halves have read them
        __syncthreads();
    }

    if constexpr (SAVE) save_rows(sv.H + (size_t)p.iters * (kCells * kLat), H, tid);
    float* out = p.pb_rep + (size_t)b * (kLat * kCells);
    for (int i = tid; i < kLat * kCells; i += kPbThreads) out[i] = H[(i % kCells) * kLS + i / kCells];
}

}  // namespace
}  // namespace gnnmp
