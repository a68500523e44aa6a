// Paired launches of the software-pipelined 64x64 fp32 tile (gemm_pipe.h): two mode-5 per-tap
// problems of equal M and N as one grid, one kernel per pair of tap counts.
#include "gemm_pipe.h"

namespace a2m {
template <int NT0>
static void launch_pipe_pair_nt(const GemmArgs& a0, const GemmArgs& a1, int nt1, dim3 grid, hipStream_t st) {
  if (nt1 == 1) hipLaunchKernelGGL((gemm_pipe_kernel_pair<NT0, 1>), grid, dim3(256), 0, st, a0, a1);
  else if (nt1 == 2) hipLaunchKernelGGL((gemm_pipe_kernel_pair<NT0, 2>), grid, dim3(256), 0, st, a0, a1);
  else hipLaunchKernelGGL((gemm_pipe_kernel_pair<NT0, 3>), grid, dim3(256), 0, st, a0, a1);
}

// a0 runs at grid z = 0 (dispatched first), a1 at z = 1; the routes' per-tap variants of nt0 and
// nt1 taps, 1-3 each (checked by gemm_pair)
void launch_pipe_pair(const GemmArgs& a0, const GemmArgs& a1, int nt0, int nt1, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(a0.N, 64), (unsigned)cdiv(a0.M, 64), 2u);
  if (nt0 == 1) launch_pipe_pair_nt<1>(a0, a1, nt1, grid, st);
  else if (nt0 == 2) launch_pipe_pair_nt<2>(a0, a1, nt1, grid, st);
  else launch_pipe_pair_nt<3>(a0, a1, nt1, grid, st);
}
}  // namespace a2m
