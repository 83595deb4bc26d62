// next_kernels.hip -- the NEXT planning network (the PPN of next_model/model2D.py:84-210) for batches of maze problems:
// env_width 15, cap = g = 8, latent 64, dim 2 (point robot) or 3 (stick robot).
//
//   next_pb_kernel     one workgroup (8 waves) per problem computes pb_rep [64, 15, 15]: the goal attention (one thread per
//                      cell runs the 4-16-16-32-32-64-1 MLP, block softmax, times softmax(dim-64-8 MLP), all in double: see
//                      attn_logit), hidden (3 x 3, 9 -> 64),
//                      h0 / c0 (3 x 3, 64 -> 64) and `iters` rounds of { conv 3 x 3 64 -> 64 on h; LSTMCell(64, 64) per cell }.
//                      Every convolution and the LSTM's two products (one K = 128 product over [x | h]) are
//                      v_mfma_f32_16x16x4_f32 in exact fp32.  The 225 cells pad to 16 row tiles of 16; a wave owns two row tiles
//                      and all their columns: 8 independent accumulator chains in a convolution, 16 in an LSTM half.  h and the
//                      conv output live in LDS as [cell][channel] rows of 68 floats (a ds_read_b128 per lane feeds four MFMA
//                      steps: the k order inside a group of 16 is permuted, the packed weights follow it), c stays in
//                      registers in the accumulator layout for the whole run.  A convolution reads its neighbour cells row by
//                      row, one tap at a time (the tap loop stays rolled so that only one tap's operands are in flight: fully
//                      unrolled it spilled); cells outside the map read a row of zeros.  The weights (278 KB a round)
//                      stream from L2 in the packed order, one coalesced 16-byte load per lane per tile.  The LSTM of a cell
//                      needs only that cell's rows, which the wave itself produced, so a round has two barriers: after the
//                      convolution (every wave has read h) and after the new h is written.
//   next_state_kernel  one workgroup (4 waves) per queried state: the state attention (thread per cell), the read-out
//                      T[c] = sum_cell a12[cell] pb_rep[c, cell] and x[g] = sum_cap a3[cap] T[8 g + cap] and the policy MLP
//                      8-128-64-(dim + 1), both accumulated in double.  A problem index outside [0, B) is counted in the status
//                      words, its row of y is NaN and pb_rep is not read for it.
// The attention (attn_logit, attention<NT>) and the read-out with the policy MLP (next_state_readout) live in next_net.hpp,
// which next_plan_kernels.hip shares: a value has the same bits from either kernel.
// Transcendentals are the accurate expf / tanhf (exp in the attention).  Summation orders are fixed: no floating-point atomics, two runs are
// bit-identical.  Bounds: LDS rows 0..256 (256 = the zero row) of both buffers are inside the allocation; row tiles 14 and 15
// hold cells 224..255 of which only 224 is real, rows 225..255 are computed (finite, bias-only neighbours) and never read by a
// real cell nor written out.
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

__global__ __launch_bounds__(kPbThreads) void next_pb_kernel(NextPbParams p) {
    extern __shared__ float lds[];
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
    __syncthreads();
    conv3<4>(H, W + oC0W, W + oC0B, nbr, lane, cst);            // c0: stays in registers
    conv3<4>(H, W + oH0W, W + oH0B, nbr, lane, acc);            // h0
    __syncthreads();                                            // every wave has read the hidden layer
    store_tiles(H, acc, wave, lane);
    __syncthreads();

    const f32x4* lw = reinterpret_cast<const f32x4*>(W + oLsW) + lane;
    const int koff = 4 * (lane >> 4);
    for (int it = 0; it < p.iters; ++it) {
        conv3<4>(H, W + oCvW, W + oCvB, nbr, lane, acc);
        store_tiles(X, acc, wave, lane);                        // own rows: the A operand of the LSTM product
        __syncthreads();                                        // and every wave has read h
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

    float* out = p.pb_rep + (size_t)b * (kLat * kCells);
    for (int i = tid; i < kLat * kCells; i += kPbThreads) out[i] = H[(i % kCells) * kLS + i / kCells];
}

__global__ __launch_bounds__(kStThreads) void next_state_kernel(NextStateParams p) {
    __shared__ NextStateScratch sc;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nout = p.dim + 1;
    const int pr = p.problem_of_state[s];
    if (pr < 0 || pr >= p.B) {                                  // uniform over the workgroup: reported, not read, not clamped
        if (tid == 0) {
            atomicAdd(p.status, 1);
            atomicMax(p.status + 1, s + 1);
        }
        if (tid < nout) p.y[(size_t)s * nout + tid] = __int_as_float(0x7fc00000);
        return;
    }
    next_state_readout(p.weights, p.states + (size_t)s * p.dim, p.dim, tid, p.pb_rep + (size_t)pr * (kLat * kCells), sc,
                       p.y + (size_t)s * nout);
}

}  // namespace

size_t next_weights_floats() { return kWeightFloats; }

hipError_t launch_next_pb_forward(const NextPbParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    const size_t lds = (size_t)2 * kBufFloats * sizeof(float) + 96 * sizeof(double);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(next_pb_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(next_pb_kernel, dim3(p.B), dim3(kPbThreads), lds, st, p);
    return hipGetLastError();
}

hipError_t launch_next_state_forward(const NextStateParams& p, hipStream_t st) {
    if (p.S <= 0) return hipSuccess;
    hipLaunchKernelGGL(next_state_kernel, dim3(p.S), dim3(kStThreads), 0, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
