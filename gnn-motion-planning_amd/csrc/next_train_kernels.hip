// next_train_kernels.hip -- training the NEXT planning network on maze problems (dim 2 / 3, width 15): the forward that keeps its
// activations and the backward, in the packed weight layout of next_kernels.hip.
//
//   next_pb_train_kernel    next_pb_body<SAVE = true> (next_pb.hpp): the inference arithmetic in the inference order, plus the
//                           stores of x9, the hidden layer, every round's h and c going in and the conv output.  The gate
//                           activations are recomputed in the backward.  y comes from next_state_kernel itself.
//   next_state_bwd_kernel   one workgroup per state: next_state_readout again (a12, a3, T, x, h1, h2 in double), the policy MLP
//                           backwards, this state's policy-weight gradient into its row of part_state, and a12 / dT / da12 /
//                           da3 into its row of st_d.
//   next_attn_bwd_kernel    one workgroup per state (mode 0) or per goal (mode 1): the attention again, both softmaxes and the
//                           dim-64-8 MLP backwards, then the shared 4-16-16-32-32-64-1 MLP layer by layer: a thread per cell
//                           back-propagates its delta (double arithmetic, activations and deltas parked in LDS as float), then
//                           a thread per weight sums delta x activation over the 225 cells in ascending order in double.
//   next_dpb_reduce_kernel  dpb_rep[b] = sum over the states of problem b, ascending state index, of a12 (x) dT, in double.
//   next_reduce_state_kernel  sum over the states, ascending, of part_state -> attn_acc (double) and dweights[0, oHidW).
//   next_pb_bwd_kernel      one workgroup (8 waves) per problem: back-propagation through the rounds.  A round recomputes the
//                           gates (the forward's MFMA product, operands from the saved rows), forms the gate gradients dG
//                           (a [256][256] float image per problem in the workspace, the cell-state gradient beside it), then dx = dG Wih^T and dG Whh^T
//                           (v_mfma_f32_16x16x4_f32 on the transposed LSTM packing), dh = conv^T(dx) + dG Whh^T (conv3 with
//                           flipped taps and the transposed channel matrix) and the weight gradients of the round:
//                           sum over cells of h[neighbour] (x) dx and of [x | h] (x) dG on v_mfma_f64_16x16x4_f64, added to
//                           this problem's double partial sums (part_pb) by the lane that owns the element, rounds descending.
//                           Then h0 / c0 / hidden the same way and the gradient of x9's attention channels (goal_d).
//   next_reduce_pb_kernel   sum over the problems, ascending, of part_pb -> dweights[oHidW, end) and of part_goal, added to
//                           attn_acc -> dweights[0, oP1) (the shared attention: states first, then goals).
// No floating-point atomics; every sum has one fixed order; two runs give the same bits.
//
// Bounds.  (a) Padding cells: the row tiles cover cells 0..255, 225 are real.  save_tiles and every load of a saved row are
// guarded by row < 225 (the saved arrays have 225 rows); the LDS buffers have rows 0..256; the dG image has 256 rows, the rows
// 225..255 receive exact zeros (their dh and dc are zero), and the weight-gradient loops stop at cell 227 < 256.  (b) Padded tap
// neighbours: nbr_row gives the zero row of an LDS buffer, wgrad_conv reads no global row for a neighbour outside the map.
// (c) A problem with no states: next_dpb_reduce_kernel writes zeros, nothing indexes by a state.  (d) A state whose
// problem_of_state is outside [0, B): the state and attention kernels return before reading or writing anything for it and the
// reductions skip its rows.  (e) Every launcher returns before any HIP call when its grid would be empty.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "next_net.hpp"
#include "next_pb.hpp"

namespace gnnmp {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kPerState = oHidW;                       // attention + policy: the per-state range of the packed weights
constexpr int kAttn = oP1;                             // the shared attention MLP and the dim-64-8 MLP
constexpr int kPbPart = kWeightFloats - oHidW;         // hidden, h0, c0, conv, lstm
constexpr int kRow = kCells * kLat;                    // floats of one saved [225][64] array
constexpr int tCv = 0, tH0 = 36 * 1024, tC0 = 2 * tH0, tLs = 3 * tH0, tZero = tLs + 16 * 8 * 256, kWeightTFloats = tZero + 64;
constexpr int kStD = 528, sA12 = 0, sDT = 225, sDA12 = 289, sDA3 = 514;
constexpr int kAS = 97, kDS = 65;                      // LDS strides of the activations and the deltas of a cell
constexpr int kAttnDoubles = 80 + 8 + 226 + 226 + 8 + 8 + 8;
constexpr size_t kAttnLds = kAttnDoubles * sizeof(double) + (size_t)kCells * (kAS + kDS) * sizeof(float);
constexpr size_t kPbLds = (size_t)2 * kBufFloats * sizeof(float) + 96 * sizeof(double);
constexpr size_t kPbBwdLds = (size_t)2 * kBufFloats * sizeof(float);
static_assert(kAttnLds <= 160 * 1024 && kPbLds <= 160 * 1024, "LDS of a workgroup");
static_assert(sDA3 + 8 <= kStD, "a state's row of st_d");

__device__ __forceinline__ NextPbSave save_of(char* ws, const NextTrainCarve& c, int b, int iters) {
    float* base = reinterpret_cast<float*>(ws + c.saved) + (size_t)b * c.saved_floats;
    NextPbSave sv;
    sv.x9 = base;
    sv.hl = sv.x9 + kCells * 16;
    sv.H = sv.hl + kRow;
    sv.C = sv.H + (size_t)(iters + 1) * kRow;
    sv.X = sv.C + (size_t)iters * kRow;
    return sv;
}

__global__ __launch_bounds__(kPbThreads) void next_pb_train_kernel(NextPbParams p, char* ws, NextTrainCarve c) {
    extern __shared__ float lds[];
    next_pb_body<true>(p, save_of(ws, c, blockIdx.x, p.iters), lds);
}

// ------------------------------------------------------------------------------------------------------------------------
// the state side
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kStThreads) void next_state_bwd_kernel(NextTrainBwdParams p) {
    __shared__ NextStateScratch sc;
    __shared__ double s_dy[4], s_dh2[64], s_dh1[128], s_dx[8];
    __shared__ float s_y[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nout = p.dim + 1;
    const int pr = p.problem_of_state[s];
    if (pr < 0 || pr >= p.B) return;                            // uniform: counted by the forward, nothing read or written here
    const float* __restrict__ W = p.weights;
    const float* pb = p.pb_rep + (size_t)pr * (kLat * kCells);
    double* out = reinterpret_cast<double*>(p.ws + p.c.part_state) + (size_t)s * kPerState;
    double* sd = reinterpret_cast<double*>(p.ws + p.c.st_d) + (size_t)s * kStD;
    next_state_readout(W, p.states + (size_t)s * p.dim, p.dim, tid, pb, sc, s_y);
    if (tid < 4) s_dy[tid] = tid < nout ? (double)p.dy[(size_t)s * nout + tid] : 0.;
    __syncthreads();
    out[oP3 + tid] = s_dy[tid >> 6] * sc.h2[tid & 63];          // 4 x 64: the rows beyond dim + 1 get zero
    if (tid < 4) out[oPB3 + tid] = s_dy[tid];
    if (tid < 64) {
        double v = 0.;
        for (int o = 0; o < nout; ++o) v = fma((double)W[oP3 + o * 64 + tid], s_dy[o], v);
        v = sc.h2[tid] > 0. ? v : 0.;
        s_dh2[tid] = v;
        out[oPB2 + tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < 64 * 128; i += kStThreads) out[oP2 + i] = s_dh2[i >> 7] * sc.h1[i & 127];
    if (tid < 128) {
        double v = 0.;
        for (int j = 0; j < 64; ++j) v = fma((double)W[oP2 + j * 128 + tid], s_dh2[j], v);
        v = sc.h1[tid] > 0. ? v : 0.;
        s_dh1[tid] = v;
        out[oPB1 + tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < 128 * 8; i += kStThreads) out[oP1 + i] = s_dh1[i >> 3] * sc.x[i & 7];
    if (tid < 8) {
        double v = 0.;
        for (int i = 0; i < 128; ++i) v = fma((double)W[oP1 + i * 8 + tid], s_dh1[i], v);
        s_dx[tid] = v;
    }
    __syncthreads();
    if (tid < 64) sc.h2[tid] = sc.a3[tid & 7] * s_dx[tid >> 3];           // dT, in the place of h2 (no longer needed)
    if (tid < 8) {
        double v = 0.;
        for (int g = 0; g < 8; ++g) v = fma(s_dx[g], sc.T[g * 8 + tid], v);
        sd[sDA3 + tid] = v;
    }
    __syncthreads();
    if (tid < 64) sd[sDT + tid] = sc.h2[tid];
    if (tid < kCells) {
        double v = 0.;
        for (int c = 0; c < kLat; ++c) v = fma(sc.h2[c], (double)pb[c * kCells + tid], v);
        sd[sDA12 + tid] = v;
        sd[sA12 + tid] = sc.a12[tid];
    }
}

// dW[o][i] = sum over the cells, ascending, of delta[cell][o] act[cell][i]; db[o] = sum of delta[cell][o]
__device__ __forceinline__ void attn_wsum(double* outW, double* outB, int NO, int NI, const float* DEL, const float* ACT, int tid) {
    for (int idx = tid; idx < NO * NI; idx += kStThreads) {
        const int o = idx / NI, i = idx - o * NI;
        double v = 0.;
        for (int cell = 0; cell < kCells; ++cell) v = fma((double)DEL[cell * kDS + o], (double)ACT[cell * kAS + i], v);
        outW[idx] = v;
    }
    for (int o = tid; o < NO; o += kStThreads) {
        double v = 0.;
        for (int cell = 0; cell < kCells; ++cell) v += (double)DEL[cell * kDS + o];
        outB[o] = v;
    }
}

// layer 5 output o of a cell before its ReLU, as attn_logit computes it
__device__ __forceinline__ double attn_e(const float* __restrict__ W, int o, const double (&d)[32]) {
    double v = W[oB5 + o];
#pragma unroll
    for (int i = 0; i < 32; ++i) v = fma((double)W[oW5 + o * 32 + i], d[i], v);
    return v;
}

__global__ __launch_bounds__(kStThreads) void next_attn_bwd_kernel(NextTrainBwdParams p, int mode) {
    extern __shared__ double ldsd[];
    double* s_red = ldsd;                      // attention<>'s scratch: 8 + 64 (the dim-64-8 MLP's hidden layer) + 8
    double* s_a3 = s_red + 80;
    double* s_a12 = s_a3 + 8;
    double* s_dl = s_a12 + 226;
    double* s_da3 = s_dl + 226;
    double* s_do = s_da3 + 8;
    double* s_w = s_do + 8;
    float* ACT = reinterpret_cast<float*>(ldsd + kAttnDoubles);
    float* DEL = ACT + kCells * kAS;
    const int q = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ W = p.weights;
    const float* state;
    double* out;
    const double* in;
    if (mode == 0) {
        const int pr = p.problem_of_state[q];
        if (pr < 0 || pr >= p.B) return;                        // uniform
        state = p.states + (size_t)q * p.dim;
        out = reinterpret_cast<double*>(p.ws + p.c.part_state) + (size_t)q * kPerState;
        in = reinterpret_cast<const double*>(p.ws + p.c.st_d) + (size_t)q * kStD;
    } else {
        state = p.goals + (size_t)q * p.dim;
        out = reinterpret_cast<double*>(p.ws + p.c.part_goal) + (size_t)q * kAttn;
        in = reinterpret_cast<const double*>(p.ws + p.c.goal_d) + (size_t)q * (kCells * 8);
    }
    float f0 = state[0], f1 = state[1], f2 = p.dim == 3 ? state[2] : 0.f;
    if (p.dim == 3) f2 = f2 / 0.4f; else f1 = f1 / 0.4f;        // as attention<>
    const double s0 = f0, s1 = f1, s2 = f2;
    const double a12 = attention<kStThreads>(W, state, p.dim, tid, s_red, s_a3);
    const double* s_z = s_red + 2 * (kStThreads / 64);
    const bool cell = tid < kCells;

    double da12 = 0.;
    if (mode == 0) {
        if (cell) da12 = in[sDA12 + tid];
        if (tid < 8) s_da3[tid] = in[sDA3 + tid];
    } else {
        if (cell) {
            s_a12[tid] = a12;
            for (int c = 0; c < 8; ++c) da12 = fma(in[tid * 8 + c], s_a3[c], da12);
        }
        __syncthreads();
        if (tid < 8) {
            double v = 0.;
            for (int c = 0; c < kCells; ++c) v = fma(in[c * 8 + tid], s_a12[c], v);
            s_da3[tid] = v;
        }
    }
    const double ws = wave_sum(a12 * da12);
    if ((tid & 63) == 0) s_w[tid >> 6] = ws;
    __syncthreads();
    const double dot = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    const double dl = a12 * (da12 - dot);                       // the gradient of this cell's logit
    if (cell) s_dl[tid] = dl;
    if (tid < 8) {
        double t = 0.;
        for (int c = 0; c < 8; ++c) t = fma(s_a3[c], s_da3[c], t);
        const double v = s_a3[tid] * (s_da3[tid] - t);
        s_do[tid] = v;
        out[oMB2 + tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < 8 * 64; i += kStThreads) out[oM2 + i] = s_do[i >> 6] * s_z[i & 63];
    if (tid < 64) {
        double v = 0.;
        for (int c = 0; c < 8; ++c) v = fma((double)W[oM2 + c * 64 + tid], s_do[c], v);
        v = s_z[tid] > 0. ? v : 0.;
        out[oM1 + tid * 3] = v * s0;
        out[oM1 + tid * 3 + 1] = v * s1;
        out[oM1 + tid * 3 + 2] = v * s2;                        // dim 2: s2 = 0, the padding column gets zero
        out[oMB1 + tid] = v;
    }

    // ---- the shared MLP: forward of this thread's cell, activations parked as float
    float* act = ACT + (cell ? tid : 0) * kAS;
    float* del = DEL + (cell ? tid : 0) * kDS;
    const double col = (double)(tid % kW), row = (double)(tid / kW);
    double d[32];
    if (cell) {
        double a[16], b[16], c[32];
#pragma unroll
        for (int o = 0; o < 16; ++o)
            a[o] = relu(fma((double)W[oW1 + o * 4 + 3], row, fma((double)W[oW1 + o * 4 + 2], col,
                        fma((double)W[oW1 + o * 4 + 1], s1, fma((double)W[oW1 + o * 4], s0, (double)W[oB1 + o])))));
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
#pragma unroll
        for (int i = 0; i < 16; ++i) act[i] = (float)a[i], act[16 + i] = (float)b[i];
#pragma unroll
        for (int i = 0; i < 32; ++i) act[32 + i] = (float)c[i], act[64 + i] = (float)d[i];
#pragma unroll 2
        for (int o = 0; o < 64; ++o) del[o] = (float)(dl * relu(attn_e(W, o, d)));
    }
    __syncthreads();
    if (tid < 64) {                                             // the last layer: dW6[o] = sum dl relu(e[o])
        double v = 0.;
        for (int c = 0; c < kCells; ++c) v += (double)DEL[c * kDS + tid];
        out[oW6 + tid] = v;
    } else if (tid == 64) {
        double v = 0.;
        for (int c = 0; c < kCells; ++c) v += s_dl[c];
        out[oB6] = v;
    } else if (tid < 68) {
        out[oB6 + tid - 64] = 0.;                               // the bias's padding lanes
    }
    __syncthreads();
    {                                                           // layer 5 (32 -> 64)
        double dd[32];
        if (cell) {
#pragma unroll
            for (int i = 0; i < 32; ++i) dd[i] = 0.;
#pragma unroll 2
            for (int o = 0; o < 64; ++o) {
                const double de = attn_e(W, o, d) > 0. ? dl * (double)W[oW6 + o] : 0.;
                del[o] = (float)de;
#pragma unroll
                for (int i = 0; i < 32; ++i) dd[i] = fma((double)W[oW5 + o * 32 + i], de, dd[i]);
            }
        }
        __syncthreads();
        attn_wsum(out + oW5, out + oB5, 64, 32, DEL, ACT + 64, tid);
        __syncthreads();
        if (cell) {
#pragma unroll
            for (int i = 0; i < 32; ++i) del[i] = (float)(d[i] > 0. ? dd[i] : 0.);
        }
    }
    __syncthreads();
    attn_wsum(out + oW4, out + oB4, 32, 32, DEL, ACT + 32, tid);             // layer 4 (32 -> 32)
    {
        double dc[32];
        if (cell) {
#pragma unroll
            for (int i = 0; i < 32; ++i) dc[i] = 0.;
#pragma unroll 2
            for (int o = 0; o < 32; ++o) {
                const double de = del[o];
#pragma unroll
                for (int i = 0; i < 32; ++i) dc[i] = fma((double)W[oW4 + o * 32 + i], de, dc[i]);
            }
        }
        __syncthreads();
        if (cell) {
#pragma unroll
            for (int i = 0; i < 32; ++i) del[i] = (float)(act[32 + i] > 0.f ? dc[i] : 0.);
        }
    }
    __syncthreads();
    attn_wsum(out + oW3, out + oB3, 32, 16, DEL, ACT + 16, tid);             // layer 3 (16 -> 32)
    {
        double db[16];
        if (cell) {
#pragma unroll
            for (int i = 0; i < 16; ++i) db[i] = 0.;
#pragma unroll 2
            for (int o = 0; o < 32; ++o) {
                const double de = del[o];
#pragma unroll
                for (int i = 0; i < 16; ++i) db[i] = fma((double)W[oW3 + o * 16 + i], de, db[i]);
            }
        }
        __syncthreads();
        if (cell) {
#pragma unroll
            for (int i = 0; i < 16; ++i) del[i] = (float)(act[16 + i] > 0.f ? db[i] : 0.);
        }
    }
    __syncthreads();
    attn_wsum(out + oW2, out + oB2, 16, 16, DEL, ACT, tid);                  // layer 2 (16 -> 16)
    {
        double da[16];
        if (cell) {
#pragma unroll
            for (int i = 0; i < 16; ++i) da[i] = 0.;
#pragma unroll 2
            for (int o = 0; o < 16; ++o) {
                const double de = del[o];
#pragma unroll
                for (int i = 0; i < 16; ++i) da[i] = fma((double)W[oW2 + o * 16 + i], de, da[i]);
            }
        }
        __syncthreads();
        if (cell) {
#pragma unroll
            for (int i = 0; i < 16; ++i) del[i] = (float)(act[i] > 0.f ? da[i] : 0.);
            act[0] = (float)s0, act[1] = (float)s1, act[2] = (float)col, act[3] = (float)row;   // layer 1's input (exact in float)
        }
    }
    __syncthreads();
    attn_wsum(out + oW1, out + oB1, 16, 4, DEL, ACT, tid);                   // layer 1 (4 -> 16)
}

constexpr int kDpbChunks = 8, kDpbChunk = kLat * kCells / kDpbChunks, kDpbPer = (kDpbChunk + 255) / 256;
static_assert(kDpbChunk * kDpbChunks == kLat * kCells, "whole chunks");

__global__ __launch_bounds__(256) void next_dpb_reduce_kernel(NextTrainBwdParams p) {
    const int b = blockIdx.x, tid = threadIdx.x, base = blockIdx.y * kDpbChunk;
    double acc[kDpbPer];
#pragma unroll
    for (int k = 0; k < kDpbPer; ++k) acc[k] = 0.;
    const double* sdb = reinterpret_cast<const double*>(p.ws + p.c.st_d);
#pragma unroll 1
    for (int s = 0; s < p.S; ++s) {
        if (p.problem_of_state[s] != b) continue;               // uniform
        const double* sd = sdb + (size_t)s * kStD;
#pragma unroll
        for (int k = 0; k < kDpbPer; ++k) {
            const int j = tid + 256 * k, i = base + j;
            if (j < kDpbChunk) acc[k] = fma(sd[sA12 + i % kCells], sd[sDT + i / kCells], acc[k]);
        }
    }
    float* out = p.dpb_rep + (size_t)b * (kLat * kCells);
#pragma unroll
    for (int k = 0; k < kDpbPer; ++k) {
        const int j = tid + 256 * k;
        if (j < kDpbChunk) out[base + j] = (float)acc[k];
    }
}

__global__ __launch_bounds__(256) void next_reduce_state_kernel(NextTrainBwdParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kPerState) return;
    const double* part = reinterpret_cast<const double*>(p.ws + p.c.part_state);
    double v = 0.;
    for (int s = 0; s < p.S; ++s) {
        const int pr = p.problem_of_state[s];
        if (pr >= 0 && pr < p.B) v += part[(size_t)s * kPerState + i];
    }
    reinterpret_cast<double*>(p.ws + p.c.attn_acc)[i] = v;
    p.dweights[i] = (float)v;
}

__global__ __launch_bounds__(256) void next_reduce_pb_kernel(NextTrainBwdParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kWeightFloats) return;
    if (i < kAttn) {
        const double* part = reinterpret_cast<const double*>(p.ws + p.c.part_goal);
        double v = p.S > 0 ? reinterpret_cast<const double*>(p.ws + p.c.attn_acc)[i] : 0.;
        for (int b = 0; b < p.B; ++b) v += part[(size_t)b * kAttn + i];
        p.dweights[i] = (float)v;
    } else if (i < oHidW) {
        if (p.S == 0) p.dweights[i] = 0.f;                      // no state backward ran: the policy's gradient is zero
    } else {
        const double* part = reinterpret_cast<const double*>(p.ws + p.c.part_pb);
        double v = 0.;
        for (int b = 0; b < p.B; ++b) v += part[(size_t)b * kPbPart + (i - oHidW)];
        p.dweights[i] = (float)v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// the problem side
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f64x4 mfma64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// The weight gradient of a 3 x 3 convolution, added to its packed positions: for tap and input-channel tile u = (tap, cit) and the
// four output tiles, sum over the cells of src[neighbour(cell, tap)][ci] D[cell][co].  src: saved global rows [225][SS]; D: an
// LDS buffer (rows 225..255 zero).  The f64 result tile has row (lane >> 4) + 4 r, column lane & 15.
template <int CG, int SS>
__device__ __forceinline__ void wgrad_conv(const float* __restrict__ src, const float* D, double* part, int wave, int lane) {
    const int kq = lane >> 4, c16 = lane & 15;
#pragma unroll 1
    for (int u = wave; u < 9 * CG; u += 8) {
        const int tap = u / CG, cit = u - tap * CG;
        const int ky = tap / 3, kx = tap - 3 * ky;
        f64x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = f64x4{0., 0., 0., 0.};
        int rr = ky - 1, cc = kq + kx - 1;                      // the neighbour of cell kq, stepped with the cell: a division per
        asm volatile("" : "+v"(rr), "+v"(cc));                  // step, hoisted out of the round loop for all 57 steps, spilled
        const float* dp = D + kq * kLS + c16;
#pragma unroll 2
        for (int ks = 0; ks < 57; ++ks) {                       // cells 0..227: three padding cells, zero on both sides
            const int cell = 4 * ks + kq;
            const bool in = cell < kCells && rr >= 0 && rr < kW && cc >= 0 && cc < kW;
            double a = 0.;
            if (in) a = (double)src[(rr * kW + cc) * SS + cit * 16 + c16];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = mfma64(a, (double)dp[nt * 16], acc[nt]);
            dp += 4 * kLS;
            cc += 4;
            if (cc - kx + 1 >= kW) cc -= kW, ++rr;
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[((u * 4 + nt) * 64 + r * 16 + c16) * 4 + kq] += acc[nt][r];
    }
}

// dG [256][256] (global image) times the transposed LSTM packing: columns 64 pass .. 64 pass + 63 of d[x | h] for the wave's rows
__device__ __forceinline__ void gate_t_product(const float* __restrict__ dG, const f32x4* lwT, int pass, int wave, int lane, f32x4 (&o)[kMT][4]) {
    const int koff = 4 * (lane >> 4);
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) o[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kg = 0; kg < 16; ++kg) {
        f32x4 a[kMT];
#pragma unroll
        for (int m = 0; m < kMT; ++m)
            a[m] = *reinterpret_cast<const f32x4*>(dG + ((wave * kMT + m) * 16 + (lane & 15)) * 256 + kg * 16 + koff);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const f32x4 bw = lwT[(kg * 8 + pass * 4 + nt) * 64];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int m = 0; m < kMT; ++m) o[m][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], bw[s], o[m][nt], 0, 0, 0);
        }
    }
}

__global__ __launch_bounds__(kPbThreads) void next_pb_bwd_kernel(NextTrainBwdParams p) {
    extern __shared__ float lds[];
    float* DH = lds;
    float* DX = lds + kBufFloats;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ W = p.weights;
    const float* __restrict__ WT = p.weights_t;
    const NextPbSave sv = save_of(p.ws, p.c, b, p.iters);
    float* dG = reinterpret_cast<float*>(p.ws + p.c.dg) + (size_t)b * (256 * (256 + kLat));
    float* dC = dG + 256 * 256;                                 // [256][64]: the gradient of the cell state, between the rounds
    double* part = reinterpret_cast<double*>(p.ws + p.c.part_pb) + (size_t)b * kPbPart;
    constexpr int pHid = 0, pHidB = oHidB - oHidW, pH0 = oH0W - oHidW, pH0B = oH0B - oHidW, pC0 = oC0W - oHidW, pC0B = oC0B - oHidW,
                  pCv = oCvW - oHidW, pCvB = oCvB - oHidW, pLs = oLsW - oHidW, pLsB = oLsB - oHidW;

    for (int i = tid; i < 2 * kBufFloats; i += kPbThreads) lds[i] = 0.f;
    for (int i = tid; i < kPbPart; i += kPbThreads) part[i] = 0.;
    __syncthreads();
    const float* dpb = p.dpb_rep + (size_t)b * (kLat * kCells);
    for (int i = tid; i < kLat * kCells; i += kPbThreads) DH[(i % kCells) * kLS + i / kCells] = dpb[i];
    int nbr[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) {
        const int cellid = (wave * kMT + m) * 16 + (lane & 15);
        nbr[m] = cellid < kCells ? ((cellid / kW) << 8 | (cellid % kW)) : -1;
    }
    f32x4 acc[kMT][4], dhh[kMT][4];
    for (int i = tid; i < 256 * kLat; i += kPbThreads) dC[i] = 0.f;
    __syncthreads();

    const f32x4* lw = reinterpret_cast<const f32x4*>(W + oLsW) + lane;
    const f32x4* lwT = reinterpret_cast<const f32x4*>(WT + tLs) + lane;
    const int koff = 4 * (lane >> 4);
    for (int it = p.iters - 1; it >= 0; --it) {
        const float* __restrict__ Xg = sv.X + (size_t)it * kRow;
        const float* __restrict__ Hg = sv.H + (size_t)it * kRow;
        const float* __restrict__ Cg = sv.C + (size_t)it * kRow;
        // the gates again, then their gradients into the dG image; one row tile and 32 hidden units at a time (rolled: the
        // unrolled form spilled), the cell-state gradient parked in its own image between the rounds
#pragma unroll 1
        for (int mh = 0; mh < 2 * kMT; ++mh) {
            const int m = mh >> 1, half = mh & 1;
            const int tile = wave * kMT + m;
            f32x4 g[4][2];
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float bv = W[oLsB + gate * 64 + (2 * half + t) * 16 + (lane & 15)];
                    g[gate][t] = f32x4{bv, bv, bv, bv};
                }
            const int arow = tile * 16 + (lane & 15);
#pragma unroll 1
            for (int kg = 0; kg < 8; ++kg) {
                const float* src = kg < 4 ? Xg : Hg;
                f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
                if (arow < kCells) a = *reinterpret_cast<const f32x4*>(src + arow * kLat + (kg & 3) * 16 + koff);
#pragma unroll
                for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const f32x4 bw = lw[(kg * 16 + gate * 4 + 2 * half + t) * 64];
#pragma unroll
                        for (int s = 0; s < 4; ++s) g[gate][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bw[s], g[gate][t], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tile * 16 + 4 * (lane >> 4) + r, u = (2 * half + t) * 16 + (lane & 15);
                    const float gi = sigmoidf(g[0][t][r]), gf = sigmoidf(g[1][t][r]), gg = tanhf(g[2][t][r]), go = sigmoidf(g[3][t][r]);
                    const float cin = row < kCells ? Cg[row * kLat + u] : 0.f;
                    const float tc = tanhf(fmaf(gf, cin, gi * gg));
                    const float dh = DH[row * kLS + u];                      // rows 225..255 hold zeros
                    float* dcp = dC + row * kLat + u;                        // row < 256: inside the image; this lane's own element
                    const float dcn = fmaf(dh * go, 1.f - tc * tc, dcp[0]);
                    dcp[0] = dcn * gf;
                    float* o = dG + row * 256 + u;                           // row < 256: inside the image
                    o[0] = dcn * gg * gi * (1.f - gi);
                    o[64] = dcn * cin * gf * (1.f - gf);
                    o[128] = dcn * gi * (1.f - gg * gg);
                    o[192] = dh * tc * go * (1.f - go);
                }
        }
        __syncthreads();                                        // dG is complete; every wave has read dh
        gate_t_product(dG, lwT, 0, wave, lane, acc);            // dx = dG Wih^T
        store_tiles(DX, acc, wave, lane);
        gate_t_product(dG, lwT, 1, wave, lane, dhh);            // dG Whh^T
        __syncthreads();
        conv3<4>(DX, WT + tCv, WT + tZero, nbr, lane, acc);     // conv^T(dx): flipped taps, transposed channel matrix, no bias
#pragma unroll
        for (int m = 0; m < kMT; ++m)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[m][nt] += dhh[m][nt];
        store_tiles(DH, acc, wave, lane);                       // the gradient of the h going into this round
        // this round's weight gradients
        wgrad_conv<4, kLat>(Hg, DX, part + pCv, wave, lane);
        {                                                       // lstm: rows k of [x | h] = 16 wave .. 16 wave + 15, all 256 gate columns
            const int kq = lane >> 4, c16 = lane & 15;
            const float* __restrict__ src = (wave < 4 ? Xg : Hg) + (wave & 3) * 16 + c16;
#pragma unroll 1
            for (int pass = 0; pass < 4; ++pass) {
                f64x4 w4[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) w4[nt] = f64x4{0., 0., 0., 0.};
                const float* ap = src + kq * kLat;              // stepped with the cell and opaque: 57 hoisted addresses spilled
                const float* bp = dG + kq * 256 + pass * 64 + c16;
                asm volatile("" : "+v"(ap), "+v"(bp));
#pragma unroll 2
                for (int ks = 0; ks < 57; ++ks) {
                    double a = 0.;
                    if (4 * ks + kq < kCells) a = (double)ap[0];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) w4[nt] = mfma64(a, (double)bp[nt * 16], w4[nt]);
                    ap += 4 * kLat;
                    bp += 4 * 256;
                }
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) part[pLs + ((wave * 16 + pass * 4 + nt) * 64 + r * 16 + c16) * 4 + kq] += w4[nt][r];
            }
        }
        if (tid < 256) {
            double v = 0.;
#pragma unroll 4
            for (int c = 0; c < kCells; ++c) v += (double)dG[c * 256 + tid];
            part[pLsB + tid] += v;
        } else if (tid < 320) {
            double v = 0.;
#pragma unroll 4
            for (int c = 0; c < kCells; ++c) v += (double)DX[c * kLS + tid - 256];
            part[pCvB + tid - 256] += v;
        }
        __syncthreads();
    }

    // h0 and c0: DH holds the gradient of h0's output, dC that of c0's
    for (int i = tid; i < 256 * kLat; i += kPbThreads) DX[(i >> 6) * kLS + (i & 63)] = dC[i];
    __syncthreads();
    wgrad_conv<4, kLat>(sv.hl, DH, part + pH0, wave, lane);
    wgrad_conv<4, kLat>(sv.hl, DX, part + pC0, wave, lane);
    if (tid < 128) {
        const float* D = tid < 64 ? DH : DX;
        double v = 0.;
#pragma unroll 4
        for (int c = 0; c < kCells; ++c) v += (double)D[c * kLS + (tid & 63)];
        part[(tid < 64 ? pH0B : pC0B) + (tid & 63)] += v;
    }
    conv3<4>(DH, WT + tH0, WT + tZero, nbr, lane, acc);
    conv3<4>(DX, WT + tC0, WT + tZero, nbr, lane, dhh);
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] += dhh[m][nt];
    __syncthreads();
    store_tiles(DH, acc, wave, lane);                           // the gradient of the hidden layer
    __syncthreads();
    wgrad_conv<1, 16>(sv.x9, DH, part + pHid, wave, lane);
    if (tid < 64) {
        double v = 0.;
#pragma unroll 4
        for (int c = 0; c < kCells; ++c) v += (double)DH[c * kLS + tid];
        part[pHidB + tid] += v;
    }
    // the gradient of x9's attention channels 1..8: the hidden convolution transposed, in double
    double* gd = reinterpret_cast<double*>(p.ws + p.c.goal_d) + (size_t)b * (kCells * 8);
    for (int i = tid; i < kCells * 8; i += kPbThreads) {
        const int q = i >> 3, c = 1 + (i & 7);
        const int enc = (q / kW) << 8 | (q % kW);
        double v = 0.;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const float* drow = DH + nbr_row(enc, 8 - tap);
#pragma unroll 4
            for (int co = 0; co < kLat; ++co)
                v = fma((double)drow[co], (double)W[oHidW + ((tap * 4 + (co >> 4)) * 64 + (c >> 2) * 16 + (co & 15)) * 4 + (c & 3)], v);
        }
        gd[i] = v;
    }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

size_t next_weights_t_floats() { return kWeightTFloats; }

void next_train_carve(int B, int iters, int S, NextTrainCarve& c) {
    const size_t b = (size_t)B, s = (size_t)S;
    c.saved_floats = (size_t)kCells * 16 + (size_t)kRow * (2 + 3 * (size_t)iters);
    size_t o = 0;
    c.saved = o; o += up256(b * c.saved_floats * sizeof(float));
    c.dg = o; o += up256(b * 256 * (256 + kLat) * sizeof(float));
    c.part_pb = o; o += up256(b * kPbPart * sizeof(double));
    c.part_goal = o; o += up256(b * kAttn * sizeof(double));
    c.goal_d = o; o += up256(b * kCells * 8 * sizeof(double));
    c.part_state = o; o += up256(s * kPerState * sizeof(double));
    c.st_d = o; o += up256(s * kStD * sizeof(double));
    c.attn_acc = o; o += up256((size_t)kPerState * sizeof(double));
    c.total = o;
}

hipError_t launch_next_train_forward(const NextPbParams& pb, const NextStateParams& st, char* ws, const NextTrainCarve& c, hipStream_t s) {
    if (pb.B <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(next_pb_train_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPbLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(next_pb_train_kernel, dim3(pb.B), dim3(kPbThreads), kPbLds, s, pb, ws, c);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_next_state_forward(st, s);
}

hipError_t launch_next_state_backward(const NextTrainBwdParams& p, hipStream_t st) {
    if (p.B <= 0 || p.S <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(next_attn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(next_state_bwd_kernel, dim3(p.S), dim3(kStThreads), 0, st, p);
    hipLaunchKernelGGL(next_attn_bwd_kernel, dim3(p.S), dim3(kStThreads), kAttnLds, st, p, 0);
    hipLaunchKernelGGL(next_dpb_reduce_kernel, dim3(p.B, kDpbChunks), dim3(256), 0, st, p);
    hipLaunchKernelGGL(next_reduce_state_kernel, dim3((kPerState + 255) / 256), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_next_pb_backward(const NextTrainBwdParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(next_pb_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPbBwdLds);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(next_attn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(next_pb_bwd_kernel, dim3(p.B), dim3(kPbThreads), kPbBwdLds, st, p);
    hipLaunchKernelGGL(next_attn_bwd_kernel, dim3(p.B), dim3(kStThreads), kAttnLds, st, p, 1);
    hipLaunchKernelGGL(next_reduce_pb_kernel, dim3((kWeightFloats + 255) / 256), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
