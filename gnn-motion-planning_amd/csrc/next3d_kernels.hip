// next3d_kernels.hip -- the NEXT planning network of the arm families (the PPN of next_model/model3D.py:87-213) for batches of
// problems: env_width 15 (3375 voxels), cap = g = 8, latent 64, a network input row [point (3 or 6), state (dim <= 15)].
//
// h is 3375 x 64 floats (864 KB) a problem, so nothing of the 2-D kernel's "h lives in LDS" carries over: h, c and the hidden
// layer live in a caller-owned workspace as channel-last rows [voxel][64] (L2 / Infinity-Cache resident at small B), every stage
// is its own launch over (problem, tile of 128 voxels) and the stream orders them -- no workgroup ever waits for another one.
//
//   next3d_attn_kernel    one workgroup (8 waves) per problem: the goal attention (thread per voxel, seven voxels a thread, the
//                         1 x 1 x 1-conv MLP (point_dim + 3)-16-16-32-32-64-1, block softmax over the 3375 voxels, times
//                         softmax(dim-64-8 MLP), all in double) -> x9 rows [voxel][16] = [map, a3[cap] a123[voxel], 0 x 7];
//                         it also zeroes the one row behind every buffer that voxels outside the map read.
//   next3d_hidden_kernel  hidden (3 x 3 x 3, 9 -> 64) of a tile: K = 27 taps x 16 channels.
//   next3d_h0c0_kernel    h0 and c0 (3 x 3 x 3, 64 -> 64) of a tile from the hidden layer.
//   next3d_round_kernel   one LSTM round of a tile: x = conv(h) (K = 27 x 64 = 1728) into the wave's own LDS rows, the gates as
//                         one K = 128 product over [x | h], c updated in place, the new h into the OTHER h buffer (the
//                         neighbours of other tiles still read the old one: h is double-buffered, the launch boundary is the
//                         only synchronisation).
//   next3d_out_kernel     the final h, channel-last, -> the public pb_rep [B, 64, 15, 15, 15], channel-first.
//   next3d_state_kernel   one workgroup (8 waves) per queried state: the state attention, T[c] = sum_voxel a123[voxel] pb[c, voxel],
//                         x[g] = sum_cap a3[cap] T[8 g + cap] and the policy MLP 8-128-64-(dim + 1), accumulated in double.  A
//                         problem index outside [0, B) is counted in the status words, its row of y is NaN, pb_rep is not read.
//
// The convolution and the LSTM product of rounds 1 .. iters - 1 are v_mfma_f32_16x16x4_f32 in exact fp32, the convolution as a
// two-level sum; hidden, h0, c0 and round 0 -- whose operands are h0-sized, |h0| reaches 258 -- run the same operands through
// v_mfma_f64_16x16x4_f64 and store fp32 (see conv27 and kF64Rounds).  A wave owns two row tiles of 16 voxels and
// all 64 (256 for the gates) columns; it reads its A operands straight from the channel-last rows (one 16-byte load per lane feeds
// four MFMA steps; a voxel outside the map reads the zero row) and streams the packed weights from L2, one coalesced 16-byte load
// per lane per tile -- 442 KB a convolution, which no LDS holds.  The tap loop stays rolled so that one tap's operands are in
// flight.  Summation orders are fixed and a problem touches only its own slice of the workspace: no floating-point atomics, two
// runs are bit-identical, and pb_rep of a problem does not depend on its batch.
// Bounds: a buffer has 3376 rows (3375 = the zero row); the last tile's rows 3375 .. 3455 are computed from the zero row (finite)
// and every store is predicated on row < 3375.  LDS of the round kernel: 4 waves x 32 rows x 68 floats.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "next3d_pb.hpp"

namespace gnnmp {
namespace {

__global__ __launch_bounds__(kAtThreads) void next3d_attn_kernel(Next3dPbParams p) {
    __shared__ AttnScratch sc;
    __shared__ double a123[kV + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    float* ws = p.workspace + (size_t)b * kWsFloats;
    next3d_x9_body(p, b, ws + wsX9, sc, a123, tid);
    if (tid < kLat) {                                           // the zero rows of the other buffers
        ws[wsHL + (size_t)kZeroRow * kLat + tid] = 0.f;
        ws[wsHA + (size_t)kZeroRow * kLat + tid] = 0.f;
        ws[wsHB + (size_t)kZeroRow * kLat + tid] = 0.f;
        ws[wsC + (size_t)kZeroRow * kLat + tid] = 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void next3d_hidden_kernel(Next3dPbParams p) {
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* ws = p.workspace + (size_t)b * kWsFloats;
    next3d_hidden_body(p.weights, ws + wsX9, ws + wsHL, tile, lane, wave);
}

__global__ __launch_bounds__(kThreads) void next3d_h0c0_kernel(Next3dPbParams p) {
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* ws = p.workspace + (size_t)b * kWsFloats;
    next3d_h0c0_body(p.weights, ws + wsHL, ws + wsHA, ws + wsC, tile, lane, wave);
}

// one round: h_in -> h_out (two different buffers), c in place.  ACC = f64x4 for the first kF64Rounds rounds, whose h is still
// h0-sized (all-fp32 missed the bar at 1 and 2 rounds: profiles/next3d_parity.txt); behind them |h| <= 1 and exact fp32 MFMA holds
// it.  The gates are rounded to fp32 before the transcendentals either way.
template <typename ACC>
__global__ __launch_bounds__(kThreads) void next3d_round_kernel(Next3dPbParams p, int round) {
    typedef typename elem_of<ACC>::type T;
    __shared__ float X[kWaves * kMT * 16 * kLS];
    const int b = blockIdx.x / kTiles, tile = blockIdx.x % kTiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* ws = p.workspace + (size_t)b * kWsFloats;
    const float* __restrict__ hin = ws + ((round & 1) ? wsHB : wsHA);
    float* hout = ws + ((round & 1) ? wsHA : wsHB);
    float* cbuf = ws + wsC;
    const float* __restrict__ W = p.weights;
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
                        const float c = fmaf(gf, cbuf[at], gi * gg);
                        cbuf[at] = c;
                        hout[at] = go * tanhf(c);
                    }
                }
            }
    }
}

// channel-last rows -> pb_rep [B, 64, 3375]
__global__ __launch_bounds__(256) void next3d_out_kernel(Next3dPbParams p) {
    const int b = blockIdx.y;
    const float* __restrict__ h = p.workspace + (size_t)b * kWsFloats + ((p.iters & 1) ? wsHB : wsHA);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < kLat * kV) p.pb_rep[(size_t)b * (kLat * kV) + i] = h[(size_t)(i % kV) * kLat + i / kV];
}

__global__ __launch_bounds__(kAtThreads) void next3d_state_kernel(Next3dStateParams p) {
    __shared__ StateScratch s;
    const int st = blockIdx.x, tid = threadIdx.x;
    const int nout = p.dim + 1;
    const int pr = p.problem_of_state[st];
    if (pr < 0 || pr >= p.B) {                                  // uniform over the workgroup: reported, not read, not clamped
        if (tid == 0) {
            atomicAdd(p.status, 1);
            atomicMax(p.status + 1, st + 1);
        }
        if (tid < nout) p.y[(size_t)st * nout + tid] = __int_as_float(0x7fc00000);
        return;
    }
    const float* __restrict__ W = p.weights;
    next3d_state_readout(W, p.inputs + (size_t)st * (p.pd + p.dim), p.dim, p.pd, p.pb_rep + (size_t)pr * (kLat * kV), s, tid);
    if (tid < nout) {
        double v = (double)W[oPB3 + tid];
        for (int i = 0; i < 64; ++i) v = fma((double)W[oP3 + tid * 64 + i], s.h2[i], v);
        p.y[(size_t)st * nout + tid] = (float)v;
    }
}

}  // namespace

size_t next3d_weights_floats() { return kWeightFloats; }
size_t next3d_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * kWsFloats * sizeof(float); }

hipError_t launch_next3d_pb_forward(const Next3dPbParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    hipError_t e;
    hipLaunchKernelGGL(next3d_attn_kernel, dim3(p.B), dim3(kAtThreads), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid(p.B * kTiles);
    hipLaunchKernelGGL(next3d_hidden_kernel, grid, dim3(kThreads), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(next3d_h0c0_kernel, grid, dim3(kThreads), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (int it = 0; it < p.iters; ++it) {
        if (it < kF64Rounds) hipLaunchKernelGGL(next3d_round_kernel<f64x4>, grid, dim3(kThreads), 0, st, p, it);
        else hipLaunchKernelGGL(next3d_round_kernel<f32x4>, grid, dim3(kThreads), 0, st, p, it);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(next3d_out_kernel, dim3((kLat * kV + 255) / 256, p.B), dim3(256), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_next3d_state_forward(const Next3dStateParams& p, hipStream_t st) {
    if (p.S <= 0) return hipSuccess;
    hipLaunchKernelGGL(next3d_state_kernel, dim3(p.S), dim3(kAtThreads), 0, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
