// next_net.hpp -- the per-state half of the NEXT planning network, shared by next_kernels.hip (next_pb_kernel's goal attention,
// next_state_kernel) and next_plan_kernels.hip (the guided tree loop): the packed-weight offsets, the attention of one state for
// a whole workgroup and the read-out plus policy MLP.  A value or an action mean has the same bits whichever kernel computes
// it: one body, explicit fused multiply-adds, fixed summation orders.  Every helper lives in an unnamed namespace: each
// kernel file compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace gnnmp {
namespace {

constexpr int kW = 15, kCells = 225, kLat = 64;
constexpr int kStThreads = 256;                // workgroup of a state read-out

// packed weights (floats); gnnmp.next_model.pack_weights writes this order
constexpr int oW1 = 0, oB1 = oW1 + 64, oW2 = oB1 + 16, oB2 = oW2 + 256, oW3 = oB2 + 16, oB3 = oW3 + 512, oW4 = oB3 + 32,
              oB4 = oW4 + 1024, oW5 = oB4 + 32, oB5 = oW5 + 2048, oW6 = oB5 + 64, oB6 = oW6 + 64, oM1 = oB6 + 4, oMB1 = oM1 + 192,
              oM2 = oMB1 + 64, oMB2 = oM2 + 512, oP1 = oMB2 + 8, oPB1 = oP1 + 1024, oP2 = oPB1 + 128, oPB2 = oP2 + 8192,
              oP3 = oPB2 + 64, oPB3 = oP3 + 256, oHidW = oPB3 + 4, oHidB = oHidW + 9 * 1024, oH0W = oHidB + 64,
              oH0B = oH0W + 36 * 1024, oC0W = oH0B + 64, oC0B = oC0W + 36 * 1024, oCvW = oC0B + 64, oCvB = oCvW + 36 * 1024,
              oLsW = oCvB + 64, oLsB = oLsW + 8 * 16 * 256, kWeightFloats = oLsB + 256;

__device__ __forceinline__ double relu(double v) { return v > 0. ? v : 0.; }

// The ReLU of the policy MLP: a NaN stays a NaN, as in torch and numpy.  `v > 0 ? v : 0` alone turns it into 0, and a pb_rep
// that is not finite then reads out as an ordinary value (the last layer's bias) that no status word reports.  Decided and
// selected on the bits: the build does not honour NaNs in comparisons.  Every other input gives the bits of relu().
__device__ __forceinline__ double relu_keep_nan(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const bool nan = (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
    return __longlong_as_double((long long)((v > 0. || nan) ? b : 0ull));
}

// the shared 1 x 1-conv MLP of the attention for one cell: input [s0, s1, column, row] -> the logit.  In double: the logits
// reach tens, so a float32 logit carries an absolute error of 1e-6 and more into exp(), which the 20 recurrent rounds amplify;
// the MLP is 4 k multiply-adds a cell, nothing next to the convolutions.
__device__ __forceinline__ double attn_logit(const float* __restrict__ W, double s0, double s1, double col, double row) {
    double a[16], b[16], c[32], d[32];
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

__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The attention of one state / goal for the whole workgroup (NT threads, NT >= 225), in double: returns this thread's cell
// weight a12 (0 for tid >= 225) and leaves a3[8] in s_a3.  s_red: 2 NT / 64 + 64 + 8 doubles of LDS scratch.
template <int NT>
__device__ double attention(const float* __restrict__ W, const float* state, int dim, int tid, double* s_red, double* s_a3) {
    constexpr int NWV = NT / 64;
    float f0 = state[0], f1 = state[1], f2 = dim == 3 ? state[2] : 0.f;
    if (dim == 3) f2 = f2 / 0.4f; else f1 = f1 / 0.4f;          // the LAST coordinate over LIMITS[2], in float32 as the reference
    const double s0 = f0, s1 = f1, s2 = f2;
    double* s_sum = s_red + NWV;
    double* s_z = s_sum + NWV;
    double* s_o = s_z + 64;
    if (tid < 64)
        s_z[tid] = relu(fma((double)W[oM1 + tid * 3 + 2], s2, fma((double)W[oM1 + tid * 3 + 1], s1, fma((double)W[oM1 + tid * 3], s0, (double)W[oMB1 + tid]))));
    const bool cell = tid < kCells;
    double logit = -INFINITY;
    if (cell) logit = attn_logit(W, s0, s1, (double)(tid % kW), (double)(tid / kW));
    const double wm = wave_max(logit);
    if ((tid & 63) == 0) s_red[tid >> 6] = wm;
    __syncthreads();
    if (tid < 8) {
        double v = W[oMB2 + tid];
        for (int i = 0; i < 64; ++i) v = fma((double)W[oM2 + tid * 64 + i], s_z[i], v);
        s_o[tid] = v;
    }
    double mx = s_red[0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) mx = fmax(mx, s_red[w]);
    const double e = cell ? exp(logit - mx) : 0.;
    const double ws = wave_sum(e);
    if ((tid & 63) == 0) s_sum[tid >> 6] = ws;
    __syncthreads();
    double tot = 0.;
#pragma unroll
    for (int w = 0; w < NWV; ++w) tot += s_sum[w];
    if (tid < 8) {
        double m8 = s_o[0];
        for (int i = 1; i < 8; ++i) m8 = fmax(m8, s_o[i]);
        double den = 0.;
        for (int i = 0; i < 8; ++i) den += exp(s_o[i] - m8);
        s_a3[tid] = exp(s_o[tid] - m8) / den;
    }
    __syncthreads();
    return e / tot;
}

// LDS scratch of one state read-out, in doubles
struct NextStateScratch {
    double a12[kCells + 1];
    double red[8 + 64 + 8];
    double a3[8];
    double T[kLat], x[8], h1[128], h2[64];
};

// y[0 .. dim] = [action mean, value] of one state for a workgroup of kStThreads threads: the state attention (thread per
// cell), the read-out T[c] = sum_cell a12[cell] pb[c, cell] and x[g] = sum_cap a3[cap] T[8 g + cap] and the policy MLP
// 8-128-64-(dim + 1), accumulated in double.  `state` (dim floats), `pb` ([64, 225] floats) and `y` may lie in global memory or
// in LDS.  Threads tid <= dim write y; the caller puts a barrier before anybody else reads it, and before `state` changes.
__device__ __forceinline__ void next_state_readout(const float* __restrict__ W, const float* state, int dim, int tid, const float* pb,
                                                   NextStateScratch& s, float* y) {
    const int lane = tid & 63, wave = tid >> 6;
    const int nout = dim + 1;
    const double a12 = attention<kStThreads>(W, state, dim, tid, s.red, s.a3);
    if (tid < kCells) s.a12[tid] = a12;
    __syncthreads();
    for (int c = wave; c < kLat; c += 4) {                      // T[c]: a wave per channel, cells over the lanes
        double t = 0.;
        for (int q = lane; q < kCells; q += 64) t = fma(s.a12[q], (double)pb[c * kCells + q], t);
        t = wave_sum(t);
        if (lane == 0) s.T[c] = t;
    }
    __syncthreads();
    if (tid < 8) {
        double x = 0.;
        for (int cap = 0; cap < 8; ++cap) x = fma(s.a3[cap], s.T[tid * 8 + cap], x);
        s.x[tid] = x;
    }
    __syncthreads();
    if (tid < 128) {
        double v = (double)W[oPB1 + tid];
        for (int i = 0; i < 8; ++i) v = fma((double)W[oP1 + tid * 8 + i], s.x[i], v);
        s.h1[tid] = relu_keep_nan(v);
    }
    __syncthreads();
    {
        const int j = tid >> 2, part = tid & 3;                 // 64 outputs, four threads each
        double v = 0.;
        for (int i = part; i < 128; i += 4) v = fma((double)W[oP2 + j * 128 + i], s.h1[i], v);
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += (double)W[oPB2 + j];
        if (part == 0) s.h2[j] = relu_keep_nan(v);
    }
    __syncthreads();
    if (tid < nout) {
        double v = (double)W[oPB3 + tid];
        for (int i = 0; i < 64; ++i) v = fma((double)W[oP3 + tid * 64 + i], s.h2[i], v);
        y[tid] = (float)v;
    }
}

}  // namespace
}  // namespace gnnmp
