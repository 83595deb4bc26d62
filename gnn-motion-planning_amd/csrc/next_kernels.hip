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
// The body of next_pb_kernel and its tile helpers (conv3, store_tiles) live in next_pb.hpp: next_train_kernels.hip instantiates the
// same body with the stores a backward needs.
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
#include "next_pb.hpp"

namespace gnnmp {
namespace {

__global__ __launch_bounds__(kPbThreads) void next_pb_kernel(NextPbParams p) {
    extern __shared__ float lds[];
    next_pb_body<false>(p, NextPbSave{}, lds);
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
