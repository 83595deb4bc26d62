// next3d_train_kernels.hip -- training the 3-D NEXT planning network of the arm families (dim 1 .. 15, point_dim 3 / 6, width 15,
// 3375 voxels): the forward that keeps its activations and the backward, in the packed weight layout of next3d_kernels.hip.
// Everything is a stream-ordered launch over (problem, tile of 128 voxels) or (problem, unit of work); no workgroup waits for
// another one.
//
// Forward (the bodies of next3d_pb.hpp, the inference arithmetic in the inference order):
//   next3d_attn_train_kernel    x9 of a problem, and the zero row of every saved slot.
//   next3d_hidden_train_kernel, next3d_h0c0_train_kernel    the hidden layer; h and c of slot 0.
//   next3d_round_train_kernel   round r reads h and c of slot r, writes slot r + 1 and keeps the conv output x of the round (saved,
//                               not recomputed: 0.86 MB a round and problem against a second K = 1728 product per voxel).  The
//                               gate activations are recomputed in the backward.
//   next3d_out_train_kernel     h of slot iters -> pb_rep.  y comes from next3d_state_kernel itself.
// State side (one workgroup per input row: 8 waves for the read-out, 4 for the attention backward):
//   next3d_state_bwd_kernel     next3d_state_readout again (a123, a3, T, x, h1, h2 in double), the policy MLP backwards, this
//                               row's policy-weight gradient into its row of part_state, a123 / da123 / dT / da3 into st_d.
//   next3d_attn_bwd_kernel      per row (mode 0) or per goal (mode 1): the attention again, both softmaxes and the dim-64-8 MLP
//                               backwards, then the shared MLP in chunks of 128 voxels: a thread per voxel back-propagates its
//                               delta (double arithmetic, activations and deltas parked in LDS as float), then a thread per weight
//                               continues its one running double sum of delta x activation over the chunk's voxels in ascending
//                               order (the running value waits in this row's slice of the workspace between chunks).
//   next3d_dpb_reduce_kernel    dpb_rep[b] = sum over the rows of problem b, ascending row index, of a123 (x) dT, in double.
//   next3d_reduce_state_kernel  sum over the rows, ascending, of part_state -> attn_acc (double) and dweights[0, oHidW).
// Problem side, per round from the last to the first:
//   next3d_gates_bwd_kernel     a tile: the gates again (the forward's MFMA product in the forward's accumulator type, operands
//                               from the saved rows), the gate gradients dG into a [3456][256] image of the problem and dc in
//                               place; then dx = dG Wih^T into its own buffer and dG Whh^T into the dh buffer, both
//                               v_mfma_f32_16x16x4_f32 over the transposed LSTM packing, from the wave's own rows of dG.
//   next3d_dh_kernel            dh += conv^T(dx): conv27 over the flipped, transposed packing.  It reads dx of neighbouring tiles,
//                               hence the launch boundary.
//   next3d_wgrad_kernel         one wave per unit: (tap, input-channel tile) of a convolution, (k tile, gate) of the LSTM, or 64
//                               bias columns: sum over ALL 3375 voxels in ascending order on v_mfma_f64_16x16x4_f64 (biases: plain
//                               double adds), added to this problem's double sums (part_pb) by the lane that owns the element.
//   then h0 / c0 / hidden the same way (next3d_dhl_kernel: the hidden layer's gradient), next3d_goal_d_kernel (the gradient of
//   x9's attention channels, the hidden convolution transposed in double), next3d_attn_bwd_kernel mode 1 and
//   next3d_reduce_pb_kernel: the sum over the problems, ascending, of part_pb -> dweights[oHidW, end) and of part_goal, added to
//   attn_acc -> dweights[0, oP1) (the shared attention: rows first, then goals), rounded to float once.
// No floating-point atomics; every sum has one fixed order; two runs give the same bits.
//
// Bounds.  (a) Padding rows: the 27 tiles cover rows 0 .. 3455, 3375 are real.  Every store of a row -- store_rows, the gate
// gradients, dx, dh -- is predicated on row < 3375; a load for a padding row reads the slot's zero row or is replaced by zero
// (the dG image has 3456 rows and no zero row: its padding rows are never read as data).  (b) Every saved slot (hl, h, c, x of
// every round) and the dh / dc / dx buffers have 3376 rows; row 3375 is written as zero by next3d_attn_train_kernel /
// next3d_bwd_init_kernel, one launch before any tap reads it, and never written again.  (c) Tap neighbours outside the map:
// nbr_row gives the zero row.  (d) A problem with no rows: next3d_dpb_reduce_kernel writes zeros, nothing indexes by a row.
// (e) A row whose problem_of_state is outside [0, B): counted by the forward (next3d_state_kernel), its y is NaN; the state and
// attention kernels return before reading or writing anything for it and the reductions skip its rows; nothing is clamped.
// (f) Every launcher returns before any HIP call when its grid would be empty.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "next3d_pb.hpp"

namespace gnnmp {
namespace {

constexpr int kPerState = oHidW;                       // attention + policy: the per-row range of the packed weights
constexpr int kAttn = oP1;                             // the shared attention MLP and the dim-64-8 MLP
constexpr int kPbPart = kWeightFloats - oHidW;         // hidden, h0, c0, conv, lstm
constexpr size_t kSlot = (size_t)kRows * kLat;         // floats of one saved [3376][64] array
constexpr int kDgRows = kTiles * kTileV;               // 3456
constexpr int tCv = 0, tH0 = 108 * 1024, tC0 = 2 * tH0, tLs = 3 * tH0, tZero = tLs + 16 * 8 * 256, kWeightTFloats = tZero + 64;
constexpr int sA = 0, sDA = kRows, sDT = 2 * kRows, sDA3 = sDT + 64, kStD = sDA3 + 8;
constexpr int kCh = 128, kAS = 97, kDS = 65;           // voxels of a chunk; LDS strides of the activations and the deltas of a voxel
constexpr int kAttnDoubles = 2 * kRows + 24;
constexpr size_t kAttnLds = kAttnDoubles * sizeof(double) + (size_t)kCh * (kAS + kDS) * sizeof(float);
constexpr int kSteps = (kV + 3) / 4;                   // 844 MFMA steps of four voxels
static_assert(kAttnLds + sizeof(AttnScratch) <= 160 * 1024, "LDS of a workgroup");
static_assert(tH0 % 4 == 0 && tLs % 4 == 0 && kSlot % 4 == 0, "16-byte loads");

struct Next3dSave { float *x9, *hl, *H, *C, *X; };

__device__ __forceinline__ Next3dSave save_of(char* ws, const Next3dTrainCarve& c, int b, int iters) {
    float* base = reinterpret_cast<float*>(ws + c.saved) + (size_t)b * c.saved_floats;
    Next3dSave sv;
    sv.x9 = base;
    sv.hl = sv.x9 + (size_t)kRows * kXC;
    sv.H = sv.hl + kSlot;
    sv.C = sv.H + (size_t)(iters + 1) * kSlot;
    sv.X = sv.C + (size_t)(iters + 1) * kSlot;
    return sv;
}

// ------------------------------------------------------------------------------------------------------------------------
// the forward
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAtThreads) void next3d_attn_train_kernel(Next3dPbParams p, char* ws, Next3dTrainCarve c) {
    __shared__ AttnScratch sc;
    __shared__ double a123[kV + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const Next3dSave sv = save_of(ws, c, b, p.iters);
    next3d_x9_body(p, b, sv.x9, sc, a123, tid);
    const int slots = 3 * p.iters + 3;                          // hl, h and c of iters + 1 slots, x of iters: contiguous from hl
    for (int i = tid; i < slots * kLat; i += kAtThreads) sv.hl[(size_t)(i / kLat) * kSlot + (size_t)kZeroRow * kLat + (i % kLat)] = 0.f;
}

__global__ __launch_bounds__(kThreads) void next3d_hidden_train_kernel(Next3dPbParams p, char* ws, Next3dTrainCarve c) {
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Next3dSave sv = save_of(ws, c, b, p.iters);
    next3d_hidden_body(p.weights, sv.x9, sv.hl, tile, lane, wave);
}

__global__ __launch_bounds__(kThreads) void next3d_h0c0_train_kernel(Next3dPbParams p, char* ws, Next3dTrainCarve c) {
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Next3dSave sv = save_of(ws, c, b, p.iters);
    next3d_h0c0_body(p.weights, sv.hl, sv.H, sv.C, tile, lane, wave);
}

template <typename ACC>
__global__ __launch_bounds__(kThreads) void next3d_round_train_kernel(Next3dPbParams p, char* ws, Next3dTrainCarve c, int round) {
    __shared__ float X[kRoundLdsFloats];
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Next3dSave sv = save_of(ws, c, b, p.iters);
    next3d_round_body<ACC>(p.weights, sv.H + (size_t)round * kSlot, sv.H + (size_t)(round + 1) * kSlot, sv.C + (size_t)round * kSlot,
                           sv.C + (size_t)(round + 1) * kSlot, sv.X + (size_t)round * kSlot, X, tile, lane, wave);
}

__global__ __launch_bounds__(256) void next3d_out_train_kernel(Next3dPbParams p, char* ws, Next3dTrainCarve c) {
    const int b = blockIdx.y;
    const float* __restrict__ h = save_of(ws, c, b, p.iters).H + (size_t)p.iters * kSlot;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < kLat * kV) p.pb_rep[(size_t)b * (kLat * kV) + i] = h[(size_t)(i % kV) * kLat + i / kV];
}

// ------------------------------------------------------------------------------------------------------------------------
// the state side
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAtThreads) void next3d_state_bwd_kernel(Next3dTrainBwdParams p) {
    __shared__ StateScratch sc;
    __shared__ double s_dy[kPOut], s_dh2[64], s_dh1[128], s_dx[8], s_dT[64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nout = p.dim + 1;
    const int pr = p.problem_of_state[s];
    if (pr < 0 || pr >= p.B) return;                            // uniform: counted by the forward, nothing read or written here
    const float* __restrict__ W = p.weights;
    const float* __restrict__ pb = p.pb_rep + (size_t)pr * (kLat * kV);
    double* out = reinterpret_cast<double*>(p.ws + p.c.part_state) + (size_t)s * kPerState;
    double* sd = reinterpret_cast<double*>(p.ws + p.c.st_d) + (size_t)s * kStD;
    next3d_state_readout(W, p.inputs + (size_t)s * (p.pd + p.dim), p.dim, p.pd, pb, sc, tid);
    if (tid < kPOut) s_dy[tid] = tid < nout ? (double)p.dy[(size_t)s * nout + tid] : 0.;
    __syncthreads();
    for (int i = tid; i < kPOut * 64; i += kAtThreads) out[oP3 + i] = s_dy[i >> 6] * sc.h2[i & 63];   // rows beyond dim + 1: zero
    if (tid < kPOut) out[oPB3 + tid] = s_dy[tid];
    if (tid < 64) {
        double v = 0.;
        for (int o = 0; o < nout; ++o) v = fma((double)W[oP3 + o * 64 + tid], s_dy[o], v);
        v = sc.h2[tid] > 0. ? v : 0.;
        s_dh2[tid] = v;
        out[oPB2 + tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < 64 * 128; i += kAtThreads) out[oP2 + i] = s_dh2[i >> 7] * sc.h1[i & 127];
    if (tid < 128) {
        double v = 0.;
        for (int j = 0; j < 64; ++j) v = fma((double)W[oP2 + j * 128 + tid], s_dh2[j], v);
        v = sc.h1[tid] > 0. ? v : 0.;
        s_dh1[tid] = v;
        out[oPB1 + tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < 128 * 8; i += kAtThreads) out[oP1 + i] = s_dh1[i >> 3] * sc.x[i & 7];
    if (tid < 8) {
        double v = 0.;
        for (int i = 0; i < 128; ++i) v = fma((double)W[oP1 + i * 8 + tid], s_dh1[i], v);
        s_dx[tid] = v;
    }
    __syncthreads();
    if (tid < 64) {
        const double v = sc.at.a3[tid & 7] * s_dx[tid >> 3];    // dT of channel 8 g + cap
        s_dT[tid] = v;
        sd[sDT + tid] = v;
    }
    if (tid >= 64 && tid < 72) {
        const int cap = tid - 64;
        double v = 0.;
        for (int g = 0; g < 8; ++g) v = fma(s_dx[g], sc.T[g * 8 + cap], v);
        sd[sDA3 + cap] = v;
    }
    __syncthreads();
    for (int v = tid; v < kV; v += kAtThreads) {
        double t = 0.;
        for (int c = 0; c < kLat; ++c) t = fma(s_dT[c], (double)pb[(size_t)c * kV + v], t);
        sd[sDA + v] = t;
        sd[sA + v] = sc.a123[v];
    }
}

constexpr int kBwThreads = 256;                       // the attention backward: four waves, so a wave may hold 512 registers

// dW[o][i] continues its sum over the voxels, ascending, with the n voxels of this chunk: delta[voxel][o] act[voxel][i]; db[o]
// likewise with delta[voxel][o].  The running value is the thread's own element of `out` (zero before the first chunk).
__device__ __forceinline__ void attn_wsum(double* outW, double* outB, int NO, int NI, const float* DEL, const float* ACT, int tid, int n,
                                          bool first) {
    for (int idx = tid; idx < NO * NI; idx += kBwThreads) {
        const int o = idx / NI, i = idx - o * NI;
        double v = first ? 0. : outW[idx];
        for (int q = 0; q < n; ++q) v = fma((double)DEL[q * kDS + o], (double)ACT[q * kAS + i], v);
        outW[idx] = v;
    }
    for (int o = tid; o < NO; o += kBwThreads) {
        double v = first ? 0. : outB[o];
        for (int q = 0; q < n; ++q) v += (double)DEL[q * kDS + o];
        outB[o] = v;
    }
}

// layer 5 output o of a voxel before its ReLU, as attn_tail computes it
__device__ __forceinline__ double attn_e(const float* __restrict__ W, int o, const double (&d)[32]) {
    double v = W[oB5 + o];
#pragma unroll
    for (int i = 0; i < 32; ++i) v = fma((double)W[oW5 + o * 32 + i], d[i], v);
    return v;
}

__global__ __launch_bounds__(kBwThreads) void next3d_attn_bwd_kernel(Next3dTrainBwdParams p, int mode) {
    extern __shared__ double ldsd[];
    __shared__ AttnScratch sc;
    double* a123 = ldsd;
    double* s_dl = a123 + kRows;
    double* s_da3 = s_dl + kRows;
    double* s_do = s_da3 + 8;
    double* s_w = s_do + 8;
    float* ACT = reinterpret_cast<float*>(ldsd + kAttnDoubles);
    float* DEL = ACT + kCh * kAS;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pd = p.pd, dim = p.dim;
    const float* __restrict__ W = p.weights;
    const float* inp;
    double* out;
    const double* in;
    if (mode == 0) {
        const int pr = p.problem_of_state[q];
        if (pr < 0 || pr >= p.B) return;                        // uniform
        inp = p.inputs + (size_t)q * (pd + dim);
        out = reinterpret_cast<double*>(p.ws + p.c.part_state) + (size_t)q * kPerState;
        in = reinterpret_cast<const double*>(p.ws + p.c.st_d) + (size_t)q * kStD;
    } else {
        inp = p.goals + (size_t)q * (pd + dim);
        out = reinterpret_cast<double*>(p.ws + p.c.part_goal) + (size_t)q * kAttn;
        in = reinterpret_cast<const double*>(p.ws + p.c.goal_d) + (size_t)q * (kV * 8);
    }
    attention3d<kBwThreads>(W, inp, dim, pd, tid, sc, a123);
    __syncthreads();

    // da123 of this thread's voxels into s_dl; da3
    if (mode == 0) {
        for (int v = tid; v < kV; v += kBwThreads) s_dl[v] = in[sDA + v];
        if (tid < 8) s_da3[tid] = in[sDA3 + tid];
    } else {
        for (int v = tid; v < kV; v += kBwThreads) {
            double t = 0.;
            for (int c = 0; c < 8; ++c) t = fma(in[(size_t)v * 8 + c], sc.a3[c], t);
            s_dl[v] = t;
        }
        for (int c = wave; c < 8; c += kBwThreads / 64) {       // a wave per c: da3[c] = sum_voxel d[voxel][c] a123[voxel]
            double t = 0.;
            for (int v = lane; v < kV; v += 64) t = fma(in[(size_t)v * 8 + c], a123[v], t);
            t = wave_sum(t);
            if (lane == 0) s_da3[c] = t;
        }
    }
    double part = 0.;
    for (int v = tid; v < kV; v += kBwThreads) part = fma(a123[v], s_dl[v], part);
    part = wave_sum(part);
    if (lane == 0) s_w[wave] = part;
    __syncthreads();
    double dot = s_w[0];
#pragma unroll
    for (int w = 1; w < kBwThreads / 64; ++w) dot += s_w[w];
    for (int v = tid; v < kV; v += kBwThreads) s_dl[v] = a123[v] * (s_dl[v] - dot);       // the gradient of the voxel's logit
    if (tid < 8) {
        double t = 0.;
        for (int c = 0; c < 8; ++c) t = fma(sc.a3[c], s_da3[c], t);
        const double v = sc.a3[tid] * (s_da3[tid] - t);
        s_do[tid] = v;
        out[oMB2 + tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < 8 * 64; i += kBwThreads) out[oM2 + i] = s_do[i >> 6] * sc.z[i & 63];
    if (tid < 64) {
        double v = 0.;
        for (int c = 0; c < 8; ++c) v = fma((double)W[oM2 + c * 64 + tid], s_do[c], v);
        v = sc.z[tid] > 0. ? v : 0.;
        for (int i = 0; i < kMIn; ++i) out[oM1 + tid * kMIn + i] = i < dim ? v * (double)inp[pd + i] : 0.;   // padding columns: zero
        out[oMB1 + tid] = v;
    }

    // ---- the shared MLP, 128 voxels at a time
    float* act = ACT + (tid & (kCh - 1)) * kAS;
    float* del = DEL + (tid & (kCh - 1)) * kDS;
#pragma unroll 1
    for (int base = 0; base < kV; base += kCh) {
        const int n = kV - base < kCh ? kV - base : kCh;
        const bool first = base == 0;
        // the weights are re-read (scalar loads, cached) in every chunk: were the pointer visibly loop-invariant, the compiler
        // would hoist the converted weights out of the loop and spill them (as in attention3d)
        const float* Wv = W;
        asm volatile("" : "+s"(Wv));
        const bool cell = tid < n;
        const int vx = base + tid;
        const double ci = (double)(vx / (kW * kW)), cj = (double)((vx / kW) % kW), ck = (double)(vx % kW);
        const double dl = cell ? s_dl[vx] : 0.;
        double d[32];
        __syncthreads();                                        // the previous chunk's sums have read ACT and DEL
        if (cell) {
            double a[16], b[16], c[32];
#pragma unroll
            for (int o = 0; o < 16; ++o)
                a[o] = relu(fma((double)Wv[oW1 + o * kIn1 + pd + 2], ck, fma((double)Wv[oW1 + o * kIn1 + pd + 1], ci,
                            fma((double)Wv[oW1 + o * kIn1 + pd], cj, sc.base[o]))));
#pragma unroll
            for (int o = 0; o < 16; ++o) {
                double v = Wv[oB2 + o];
#pragma unroll
                for (int i = 0; i < 16; ++i) v = fma((double)Wv[oW2 + o * 16 + i], a[i], v);
                b[o] = relu(v);
            }
#pragma unroll
            for (int o = 0; o < 32; ++o) {
                double v = Wv[oB3 + o];
#pragma unroll
                for (int i = 0; i < 16; ++i) v = fma((double)Wv[oW3 + o * 16 + i], b[i], v);
                c[o] = relu(v);
            }
#pragma unroll
            for (int o = 0; o < 32; ++o) {
                double v = Wv[oB4 + o];
#pragma unroll
                for (int i = 0; i < 32; ++i) v = fma((double)Wv[oW4 + o * 32 + i], c[i], v);
                d[o] = relu(v);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) act[i] = (float)a[i], act[16 + i] = (float)b[i];
#pragma unroll
            for (int i = 0; i < 32; ++i) act[32 + i] = (float)c[i], act[64 + i] = (float)d[i];
#pragma unroll 2
            for (int o = 0; o < 64; ++o) del[o] = (float)(dl * relu(attn_e(Wv, o, d)));
        }
        __syncthreads();
        if (tid < 64) {                                         // the last layer: dW6[o] = sum dl relu(e[o])
            double v = first ? 0. : out[oW6 + tid];
            for (int c = 0; c < n; ++c) v += (double)DEL[c * kDS + tid];
            out[oW6 + tid] = v;
        } else if (tid == 64) {
            double v = first ? 0. : out[oB6];
            for (int c = 0; c < n; ++c) v += s_dl[base + c];
            out[oB6] = v;
        } else if (tid < 68) {
            out[oB6 + tid - 64] = 0.;                           // the bias's padding lanes
        }
        __syncthreads();
        {                                                       // layer 5 (32 -> 64)
            double dd[32];
            if (cell) {
#pragma unroll
                for (int i = 0; i < 32; ++i) dd[i] = 0.;
#pragma unroll 2
                for (int o = 0; o < 64; ++o) {
                    const double de = attn_e(Wv, o, d) > 0. ? dl * (double)Wv[oW6 + o] : 0.;
                    del[o] = (float)de;
#pragma unroll
                    for (int i = 0; i < 32; ++i) dd[i] = fma((double)Wv[oW5 + o * 32 + i], de, dd[i]);
                }
            }
            __syncthreads();
            attn_wsum(out + oW5, out + oB5, 64, 32, DEL, ACT + 64, tid, n, first);
            __syncthreads();
            if (cell) {
#pragma unroll
                for (int i = 0; i < 32; ++i) del[i] = (float)(d[i] > 0. ? dd[i] : 0.);
            }
        }
        __syncthreads();
        attn_wsum(out + oW4, out + oB4, 32, 32, DEL, ACT + 32, tid, n, first);          // layer 4 (32 -> 32)
        {
            double dc[32];
            if (cell) {
#pragma unroll
                for (int i = 0; i < 32; ++i) dc[i] = 0.;
#pragma unroll 2
                for (int o = 0; o < 32; ++o) {
                    const double de = del[o];
#pragma unroll
                    for (int i = 0; i < 32; ++i) dc[i] = fma((double)Wv[oW4 + o * 32 + i], de, dc[i]);
                }
            }
            __syncthreads();
            if (cell) {
#pragma unroll
                for (int i = 0; i < 32; ++i) del[i] = (float)(act[32 + i] > 0.f ? dc[i] : 0.);
            }
        }
        __syncthreads();
        attn_wsum(out + oW3, out + oB3, 32, 16, DEL, ACT + 16, tid, n, first);          // layer 3 (16 -> 32)
        {
            double db[16];
            if (cell) {
#pragma unroll
                for (int i = 0; i < 16; ++i) db[i] = 0.;
#pragma unroll 2
                for (int o = 0; o < 32; ++o) {
                    const double de = del[o];
#pragma unroll
                    for (int i = 0; i < 16; ++i) db[i] = fma((double)Wv[oW3 + o * 16 + i], de, db[i]);
                }
            }
            __syncthreads();
            if (cell) {
#pragma unroll
                for (int i = 0; i < 16; ++i) del[i] = (float)(act[16 + i] > 0.f ? db[i] : 0.);
            }
        }
        __syncthreads();
        attn_wsum(out + oW2, out + oB2, 16, 16, DEL, ACT, tid, n, first);               // layer 2 (16 -> 16)
        {
            double da[16];
            if (cell) {
#pragma unroll
                for (int i = 0; i < 16; ++i) da[i] = 0.;
#pragma unroll 2
                for (int o = 0; o < 16; ++o) {
                    const double de = del[o];
#pragma unroll
                    for (int i = 0; i < 16; ++i) da[i] = fma((double)Wv[oW2 + o * 16 + i], de, da[i]);
                }
            }
            __syncthreads();
            if (cell) {
#pragma unroll
                for (int i = 0; i < 16; ++i) del[i] = (float)(act[i] > 0.f ? da[i] : 0.);
                // layer 1's input [point, j, i, k, 0 ...] (exact in float), in the place of its output
                for (int i = 0; i < kIn1; ++i) act[i] = i < pd ? inp[i] : 0.f;
                act[pd] = (float)cj, act[pd + 1] = (float)ci, act[pd + 2] = (float)ck;
            }
        }
        __syncthreads();
        attn_wsum(out + oW1, out + oB1, 16, kIn1, DEL, ACT, tid, n, first);             // layer 1 (point_dim + 3 -> 16; padding columns: zero)
    }
}

__global__ __launch_bounds__(256) void next3d_dpb_reduce_kernel(Next3dTrainBwdParams p) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kLat * kV) return;
    const int c = i / kV, v = i - c * kV;
    const double* sdb = reinterpret_cast<const double*>(p.ws + p.c.st_d);
    double acc = 0.;
#pragma unroll 1
    for (int s = 0; s < p.S; ++s) {
        if (p.problem_of_state[s] != b) continue;               // uniform; a row outside [0, B) matches no problem
        const double* sd = sdb + (size_t)s * kStD;
        acc = fma(sd[sA + v], sd[sDT + c], acc);
    }
    p.dpb_rep[(size_t)b * (kLat * kV) + i] = (float)acc;
}

__global__ __launch_bounds__(256) void next3d_reduce_state_kernel(Next3dTrainBwdParams p) {
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

__global__ __launch_bounds__(256) void next3d_reduce_pb_kernel(Next3dTrainBwdParams p) {
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
constexpr int pHid = 0, pHidB = oHidB - oHidW, pH0 = oH0W - oHidW, pH0B = oH0B - oHidW, pC0 = oC0W - oHidW, pC0B = oC0B - oHidW,
              pCv = oCvW - oHidW, pCvB = oCvB - oHidW, pLs = oLsW - oHidW, pLsB = oLsB - oHidW;

struct BwdBufs { float *DH, *DC, *DX, *dG; double* part; };

__device__ __forceinline__ BwdBufs bufs_of(const Next3dTrainBwdParams& p, int b) {
    BwdBufs q;
    q.DH = reinterpret_cast<float*>(p.ws + p.c.bwd) + (size_t)b * (3 * kSlot);
    q.DC = q.DH + kSlot;
    q.DX = q.DC + kSlot;
    q.dG = reinterpret_cast<float*>(p.ws + p.c.dg) + (size_t)b * ((size_t)kDgRows * 256);
    q.part = reinterpret_cast<double*>(p.ws + p.c.part_pb) + (size_t)b * kPbPart;
    return q;
}

// zero the problem's double sums and dc, dh = dpb_rep as channel-last rows, and the zero rows of dh, dc, dx
__global__ __launch_bounds__(256) void next3d_bwd_init_kernel(Next3dTrainBwdParams p) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const BwdBufs q = bufs_of(p, b);
    if (i < kPbPart) q.part[i] = 0.;
    if ((size_t)i < kSlot) q.DC[i] = 0.f;                       // the zero row included
    if (i < kLat * kV) q.DH[(size_t)(i % kV) * kLat + i / kV] = p.dpb_rep[(size_t)b * (kLat * kV) + i];
    if (i < kLat) {
        q.DH[(size_t)kZeroRow * kLat + i] = 0.f;
        q.DX[(size_t)kZeroRow * kLat + i] = 0.f;
    }
}

// rows of dG (the wave's own) times the transposed LSTM packing: columns 64 pass .. 64 pass + 63 of d[x | h]
__device__ __forceinline__ void gate_t_product(const float* __restrict__ dG, const f32x4* lwT, int pass, int rowbase, int lane,
                                               f32x4 (&o)[kMT][4]) {
    const int koff = 4 * (lane >> 4);
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) o[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kg = 0; kg < 16; ++kg) {
        f32x4 a[kMT];
#pragma unroll
        for (int m = 0; m < kMT; ++m) {
            const int row = rowbase + m * 16 + (lane & 15);
            a[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < kV) a[m] = *reinterpret_cast<const f32x4*>(dG + (size_t)row * 256 + kg * 16 + koff);
        }
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

// fp32 accumulator tiles (row 4 (lane >> 4) + r) -> rows of dst, rows behind the last voxel not written
__device__ __forceinline__ void store_rows_f32(float* dst, const f32x4 (&acc)[kMT][4], int rowbase, int lane) {
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = rowbase + m * 16 + 4 * (lane >> 4) + r;
            if (v < kV) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) dst[(size_t)v * kLat + nt * 16 + (lane & 15)] = acc[m][nt][r];
            }
        }
}

template <typename ACC>
__global__ __launch_bounds__(kThreads) void next3d_gates_bwd_kernel(Next3dTrainBwdParams p, int it) {
    typedef typename elem_of<ACC>::type T;
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ W = p.weights;
    const Next3dSave sv = save_of(p.ws, p.c, b, p.iters);
    const BwdBufs q = bufs_of(p, b);
    const float* __restrict__ Xg = sv.X + (size_t)it * kSlot;
    const float* __restrict__ Hg = sv.H + (size_t)it * kSlot;
    const float* __restrict__ Cg = sv.C + (size_t)it * kSlot;
    const f32x4* lw = reinterpret_cast<const f32x4*>(W + oLsW) + lane;
    const f32x4* lwT = reinterpret_cast<const f32x4*>(p.weights_t + tLs) + lane;
    const int koff = 4 * (lane >> 4);
    const int wbase = tile * kTileV + wave * (kMT * 16);        // the wave's 32 rows
    // the gates again, then their gradients into the dG image; one row tile and 32 hidden units at a time (rolled)
#pragma unroll 1
    for (int mh = 0; mh < 2 * kMT; ++mh) {
        const int m = mh >> 1, half = mh & 1;
        const int rowbase = wbase + m * 16;
        ACC g[4][2];
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const T bv = W[oLsB + gate * 64 + (2 * half + t) * 16 + (lane & 15)];
                g[gate][t] = ACC{bv, bv, bv, bv};
            }
        const int arow = rowbase + (lane & 15);
        const size_t aoff = (size_t)(arow < kV ? arow : kZeroRow) * kLat + koff;
#pragma unroll 1
        for (int kg = 0; kg < 8; ++kg) {
            const f32x4 a = *reinterpret_cast<const f32x4*>((kg < 4 ? Xg : Hg) + aoff + (kg & 3) * 16);
#pragma unroll
            for (int gate = 0; gate < 4; ++gate)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const f32x4 bw = lw[(kg * 16 + gate * 4 + 2 * half + t) * 64];
#pragma unroll
                    for (int s = 0; s < 4; ++s) g[gate][t] = mfma4(a[s], bw[s], g[gate][t]);
                }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rowbase + acc_row<ACC>(lane, r), u = (2 * half + t) * 16 + (lane & 15);
                if (row < kV) {
                    const float gi = sigmoidf((float)g[0][t][r]), gf = sigmoidf((float)g[1][t][r]), gg = tanhf((float)g[2][t][r]),
                                go = sigmoidf((float)g[3][t][r]);
                    const size_t at = (size_t)row * kLat + u;
                    const float cin = Cg[at];
                    const float tc = tanhf(fmaf(gf, cin, gi * gg));
                    const float dh = q.DH[at];
                    const float dcn = fmaf(dh * go, 1.f - tc * tc, q.DC[at]);       // this lane's own element of dc
                    q.DC[at] = dcn * gf;
                    float* o = q.dG + (size_t)row * 256 + u;
                    o[0] = dcn * gg * gi * (1.f - gi);
                    o[64] = dcn * cin * gf * (1.f - gf);
                    o[128] = dcn * gi * (1.f - gg * gg);
                    o[192] = dh * tc * go * (1.f - go);
                }
            }
    }
    __threadfence_block();
    __syncthreads();                                            // the wave's rows of dG are complete; it has read its rows of dh
    f32x4 o4[kMT][4];
    gate_t_product(q.dG, lwT, 0, wbase, lane, o4);              // dx = dG Wih^T
    store_rows_f32(q.DX, o4, wbase, lane);
    gate_t_product(q.dG, lwT, 1, wbase, lane, o4);              // dG Whh^T, into dh (next3d_dh_kernel adds conv^T(dx))
    store_rows_f32(q.DH, o4, wbase, lane);
}

// dh += conv^T(dx): flipped taps, transposed channel matrix, no bias
__global__ __launch_bounds__(kThreads) void next3d_dh_kernel(Next3dTrainBwdParams p) {
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BwdBufs q = bufs_of(p, b);
    int cell[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) cell[m] = lane_cell(tile, wave, m, lane);
    f32x4 acc[kMT][4];
    conv27<4, kLat>(q.DX, p.weights_t + tCv, p.weights_t + tZero, cell, lane, acc);
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = tile * kTileV + (wave * kMT + m) * 16 + acc_row<f32x4>(lane, r);
            if (v < kV) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) q.DH[(size_t)v * kLat + nt * 16 + (lane & 15)] += acc[m][nt][r];
            }
        }
}

// the gradient of the hidden layer: conv^T_h0(dh) + conv^T_c0(dc) -> the dx buffer
__global__ __launch_bounds__(kThreads) void next3d_dhl_kernel(Next3dTrainBwdParams p) {
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const BwdBufs q = bufs_of(p, b);
    int cell[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) cell[m] = lane_cell(tile, wave, m, lane);
    f32x4 acc[kMT][4], acc2[kMT][4];
    conv27<4, kLat>(q.DH, p.weights_t + tH0, p.weights_t + tZero, cell, lane, acc);
    conv27<4, kLat>(q.DC, p.weights_t + tC0, p.weights_t + tZero, cell, lane, acc2);
#pragma unroll
    for (int m = 0; m < kMT; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] += acc2[m][nt];
    store_rows(q.DX, acc, tile, wave, lane);
}

__device__ __forceinline__ f64x4 mfma64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int cell_of(int v) { return v < kV ? ((v / (kW * kW)) << 8 | ((v / kW) % kW) << 4 | (v % kW)) : -1; }

// The weight gradient of a 3 x 3 x 3 convolution, one wave per (tap, input-channel tile) u, added to its packed positions: for the
// four output tiles, sum over all voxels, ascending, of src[neighbour(voxel, tap)][ci] D[voxel][co].  src: saved rows with a zero
// row (stride SS); D: rows [3376][64] with a zero row.  The f64 result tile has row (lane >> 4) + 4 r, column lane & 15.
template <int CG, int SS>
__device__ __forceinline__ void wgrad_conv(const float* __restrict__ src, const float* __restrict__ D, double* part, int u, int lane) {
    const int kq = lane >> 4, c16 = lane & 15;
    const int tap = u / CG, cit = u - tap * CG;
    f64x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = f64x4{0., 0., 0., 0.};
#pragma unroll 2
    for (int ks = 0; ks < kSteps; ++ks) {
        const int v = 4 * ks + kq;                              // v <= 3375: the one padding voxel reads zero rows on both sides
        const double a = (double)src[(size_t)nbr_row(cell_of(v), tap) * SS + cit * 16 + c16];
        const float* dp = D + (size_t)(v < kV ? v : kZeroRow) * kLat + c16;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = mfma64(a, (double)dp[nt * 16], acc[nt]);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((u * 4 + nt) * 64 + r * 16 + c16) * 4 + kq] += acc[nt][r];
}

// column `col` of rows [.][stride], summed over the voxels in ascending order
__device__ __forceinline__ double col_sum(const float* __restrict__ D, int stride, int col) {
    double v = 0.;
#pragma unroll 4
    for (int q = 0; q < kV; ++q) v += (double)D[(size_t)q * stride + col];
    return v;
}

// mode 0: round `it` -- units 0 .. 107 conv, 108 .. 139 lstm (k tile, gate), 140 .. 144 the biases (256 lstm + 64 conv columns)
// mode 1: units 0 .. 107 h0, 108 .. 215 c0, 216 / 217 their biases;  mode 2: units 0 .. 26 hidden, 27 its bias
constexpr int kUnits0 = 145, kUnits1 = 218, kUnits2 = 28;
__global__ __launch_bounds__(64) void next3d_wgrad_kernel(Next3dTrainBwdParams p, int mode, int it) {
    const int b = blockIdx.y, u = blockIdx.x, lane = threadIdx.x;
    const Next3dSave sv = save_of(p.ws, p.c, b, p.iters);
    const BwdBufs q = bufs_of(p, b);
    if (mode == 0) {
        const float* __restrict__ Xg = sv.X + (size_t)it * kSlot;
        const float* __restrict__ Hg = sv.H + (size_t)it * kSlot;
        if (u < 108) {
            wgrad_conv<4, kLat>(Hg, q.DX, q.part + pCv, u, lane);
        } else if (u < 140) {                                   // lstm: rows k of [x | h] = 16 kt .. 16 kt + 15, gate columns 64 pass ..
            const int kt = (u - 108) >> 2, pass = (u - 108) & 3;
            const int kq = lane >> 4, c16 = lane & 15;
            const float* __restrict__ src = (kt < 4 ? Xg : Hg) + (kt & 3) * 16 + c16;
            f64x4 w4[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) w4[nt] = f64x4{0., 0., 0., 0.};
#pragma unroll 2
            for (int ks = 0; ks < kSteps; ++ks) {
                const int v = 4 * ks + kq;
                const bool in = v < kV;
                const double a = (double)src[(size_t)(in ? v : kZeroRow) * kLat];
                const float* bp = q.dG + (size_t)(in ? v : 0) * 256 + pass * 64 + c16;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) w4[nt] = mfma64(a, in ? (double)bp[nt * 16] : 0., w4[nt]);
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) q.part[pLs + ((kt * 16 + pass * 4 + nt) * 64 + r * 16 + c16) * 4 + kq] += w4[nt][r];
        } else {
            const int col = (u - 140) * 64 + lane;
            if (col < 256) q.part[pLsB + col] += col_sum(q.dG, 256, col);
            else q.part[pCvB + col - 256] += col_sum(q.DX, kLat, col - 256);
        }
    } else if (mode == 1) {
        if (u < 108) wgrad_conv<4, kLat>(sv.hl, q.DH, q.part + pH0, u, lane);
        else if (u < 216) wgrad_conv<4, kLat>(sv.hl, q.DC, q.part + pC0, u - 108, lane);
        else if (u == 216) q.part[pH0B + lane] += col_sum(q.DH, kLat, lane);
        else q.part[pC0B + lane] += col_sum(q.DC, kLat, lane);
    } else {
        if (u < 27) wgrad_conv<1, kXC>(sv.x9, q.DX, q.part + pHid, u, lane);
        else q.part[pHidB + lane] += col_sum(q.DX, kLat, lane);
    }
}

// the gradient of x9's attention channels 1 .. 8: the hidden convolution transposed, in double; dHL is in the dx buffer
__global__ __launch_bounds__(256) void next3d_goal_d_kernel(Next3dTrainBwdParams p) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kV * 8) return;
    const float* __restrict__ W = p.weights;
    const BwdBufs q = bufs_of(p, b);
    const int vx = i >> 3, c = 1 + (i & 7);
    const int enc = cell_of(vx);
    double v = 0.;
#pragma unroll 1
    for (int tap = 0; tap < 27; ++tap) {
        const float* drow = q.DX + (size_t)nbr_row(enc, 26 - tap) * kLat;
#pragma unroll 4
        for (int co = 0; co < kLat; ++co)
            v = fma((double)drow[co], (double)W[oHidW + ((tap * 4 + (co >> 4)) * 64 + (c >> 2) * 16 + (co & 15)) * 4 + (c & 3)], v);
    }
    reinterpret_cast<double*>(p.ws + p.c.goal_d)[(size_t)b * (kV * 8) + i] = v;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

size_t next3d_weights_t_floats() { return kWeightTFloats; }

void next3d_train_carve(int B, int iters, int S, Next3dTrainCarve& c) {
    const size_t b = (size_t)B, s = (size_t)S;
    c.saved_floats = (size_t)kRows * kXC + kSlot * (3 + 3 * (size_t)iters);
    size_t o = 0;
    c.saved = o; o += up256(b * c.saved_floats * sizeof(float));
    c.bwd = o; o += up256(b * 3 * kSlot * sizeof(float));
    c.dg = o; o += up256(b * (size_t)kDgRows * 256 * sizeof(float));
    c.part_pb = o; o += up256(b * kPbPart * sizeof(double));
    c.part_goal = o; o += up256(b * kAttn * sizeof(double));
    c.goal_d = o; o += up256(b * kV * 8 * sizeof(double));
    c.part_state = o; o += up256(s * kPerState * sizeof(double));
    c.st_d = o; o += up256(s * kStD * sizeof(double));
    c.attn_acc = o; o += up256((size_t)kPerState * sizeof(double));
    c.total = o;
}

#define GNNMP_LAUNCH_CHECK()                                  \
    do {                                                      \
        const hipError_t e_ = hipGetLastError();              \
        if (e_ != hipSuccess) return e_;                      \
    } while (0)

hipError_t launch_next3d_train_forward(const Next3dPbParams& pb, const Next3dStateParams& st, char* ws, const Next3dTrainCarve& c,
                                       hipStream_t s) {
    if (pb.B <= 0) return hipSuccess;
    const dim3 grid(pb.B * kTiles);
    hipLaunchKernelGGL(next3d_attn_train_kernel, dim3(pb.B), dim3(kAtThreads), 0, s, pb, ws, c);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_hidden_train_kernel, grid, dim3(kThreads), 0, s, pb, ws, c);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_h0c0_train_kernel, grid, dim3(kThreads), 0, s, pb, ws, c);
    GNNMP_LAUNCH_CHECK();
    for (int it = 0; it < pb.iters; ++it) {
        if (it < kF64Rounds) hipLaunchKernelGGL(next3d_round_train_kernel<f64x4>, grid, dim3(kThreads), 0, s, pb, ws, c, it);
        else hipLaunchKernelGGL(next3d_round_train_kernel<f32x4>, grid, dim3(kThreads), 0, s, pb, ws, c, it);
        GNNMP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(next3d_out_train_kernel, dim3((kLat * kV + 255) / 256, pb.B), dim3(256), 0, s, pb, ws, c);
    GNNMP_LAUNCH_CHECK();
    return launch_next3d_state_forward(st, s);
}

hipError_t launch_next3d_state_backward(const Next3dTrainBwdParams& p, hipStream_t st) {
    if (p.B <= 0 || p.S <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(next3d_attn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kAttnLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(next3d_state_bwd_kernel, dim3(p.S), dim3(kAtThreads), 0, st, p);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_attn_bwd_kernel, dim3(p.S), dim3(kBwThreads), kAttnLds, st, p, 0);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_dpb_reduce_kernel, dim3((kLat * kV + 255) / 256, p.B), dim3(256), 0, st, p);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_reduce_state_kernel, dim3((kPerState + 255) / 256), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_next3d_pb_backward(const Next3dTrainBwdParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(next3d_attn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kAttnLds);
    if (e != hipSuccess) return e;
    const dim3 grid(p.B * kTiles);
    hipLaunchKernelGGL(next3d_bwd_init_kernel, dim3((kPbPart + 255) / 256, p.B), dim3(256), 0, st, p);
    GNNMP_LAUNCH_CHECK();
    for (int it = p.iters - 1; it >= 0; --it) {
        if (it < kF64Rounds) hipLaunchKernelGGL(next3d_gates_bwd_kernel<f64x4>, grid, dim3(kThreads), 0, st, p, it);
        else hipLaunchKernelGGL(next3d_gates_bwd_kernel<f32x4>, grid, dim3(kThreads), 0, st, p, it);
        GNNMP_LAUNCH_CHECK();
        hipLaunchKernelGGL(next3d_dh_kernel, grid, dim3(kThreads), 0, st, p);
        GNNMP_LAUNCH_CHECK();
        hipLaunchKernelGGL(next3d_wgrad_kernel, dim3(kUnits0, p.B), dim3(64), 0, st, p, 0, it);
        GNNMP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(next3d_wgrad_kernel, dim3(kUnits1, p.B), dim3(64), 0, st, p, 1, 0);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_dhl_kernel, grid, dim3(kThreads), 0, st, p);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_wgrad_kernel, dim3(kUnits2, p.B), dim3(64), 0, st, p, 2, 0);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_goal_d_kernel, dim3((kV * 8 + 255) / 256, p.B), dim3(256), 0, st, p);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_attn_bwd_kernel, dim3(p.B), dim3(kBwThreads), kAttnLds, st, p, 1);
    GNNMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(next3d_reduce_pb_kernel, dim3((kWeightFloats + 255) / 256), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
