// Launches of the software-pipelined 64x64 bf16-operand tile (gemm_pipe_bf16.h), one kernel per
// B operand mode.
#include "gemm_pipe_bf16.h"

namespace a2m {
bool launch_pipe_bf16(const GemmArgs& a, int mb, int nt, int ma, int batch, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(a.N, 64), (unsigned)cdiv(a.M, 64), (unsigned)(batch * a.splits));
#define A2M_PIPE_LAUNCH(MB, NT, MA)                                                      \
  if (mb == MB && nt == NT && ma == MA) {                                                \
    hipLaunchKernelGGL((gemm_pipe_bf16_kernel<MB, NT, MA>), grid, dim3(256), 0, st, a);  \
    return true;                                                                         \
  }
  A2M_PIPE_VARIANTS(A2M_PIPE_LAUNCH)
#undef A2M_PIPE_LAUNCH
  return false;
}
}  // namespace a2m
