// One batch of the HBM-resident PATS loader (a2m/data.py PatsLoader) in one launch: for every
// modality, the strided windows of dataUtils.py:646-665 for the clips order[b0 .. b0+n) of the
// epoch's permutation, read from the arena that holds every interval of every split, with the
// poses already neck-subtracted and normalised (version5_model_train.py:296-319) and the audio
// standardised.  order and the start tables are read on the device: nothing comes back to the
// host, so the launch captures into a HIP graph and a replay follows an overwritten order.
// Bandwidth-trivial element work (about 3.4 MB written for 64 clips); one thread per float4.
#include "a2m_internal.h"

namespace a2m {

constexpr int BPF = 104, BPJ = 52;  // planar pose [2][52]: x of joint k at k, y at 52 + k

struct BatchMods {
  const float* arena[A2M_BATCH_MAX_MOD];
  const int64_t* start[A2M_BATCH_MAX_MOD];
  const float* mean[A2M_BATCH_MAX_MOD];
  const float* std_[A2M_BATCH_MAX_MOD];
  float* out[A2M_BATCH_MAX_MOD];
  int64_t end[A2M_BATCH_MAX_MOD];  // running total of float4 items up to and including modality m
  int c4[A2M_BATCH_MAX_MOD], nj[A2M_BATCH_MAX_MOD], interval[A2M_BATCH_MAX_MOD], mode[A2M_BATCH_MAX_MOD];
  int n_mod;
};

// Item i of modality m is float4 q of output row (b, j): i = (b * nj + j) * c4 + q.  52 is a
// multiple of 4, so a float4 of a pose row lies on one side of the neck boundary.
__global__ void batch_gather_kernel(BatchMods M, const int64_t* __restrict__ order, int64_t b0) {
  const int64_t total = M.end[M.n_mod - 1];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int m = 0;
    while (i >= M.end[m]) ++m;
    const int64_t r = i - (m ? M.end[m - 1] : 0);
    const int c4 = M.c4[m], nj = M.nj[m];
    const int q = (int)(r % c4);
    const int64_t bj = r / c4;
    const int j = (int)(bj % nj);
    const int64_t b = bj / nj;
    const int64_t row = M.start[m][order[b0 + b]] + (int64_t)j * M.interval[m];
    const float* src = M.arena[m] + row * (4 * (int64_t)c4);
    float4 v = reinterpret_cast<const float4*>(src)[q];
    if (M.mode[m] != A2M_BATCH_RAW) {
      const float* mean = M.mean[m] + 4 * q;
      const float* sd = M.std_[m] + 4 * q;
      float x[4] = {v.x, v.y, v.z, v.w};
      if (M.mode[m] == A2M_BATCH_NECKSUB) {
        // pose_normalize_kernel's arithmetic: no guard on std, every step rounded once
        const float neck = src[4 * q < BPJ ? 0 : BPJ];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          x[k] = __fdiv_rn(__fsub_rn(__fsub_rn(x[k], neck), mean[k]), sd[k]);
      } else {
        // window_gather_kernel's
#pragma unroll
        for (int k = 0; k < 4; ++k)
          x[k] = __fdiv_rn(__fsub_rn(x[k], mean[k]), sd[k] < 1e-7f ? 1.f : sd[k]);
      }
      v = make_float4(x[0], x[1], x[2], x[3]);
    }
    reinterpret_cast<float4*>(M.out[m])[r] = v;
  }
}

}  // namespace a2m

using namespace a2m;

extern "C" int a2m_batch_gather_f32(int32_t n_mod, const float* const* arena,
                                    const int64_t* const* start, const int32_t* C,
                                    const int32_t* window, const int32_t* interval,
                                    const int32_t* mode, const float* const* mean,
                                    const float* const* std_, float* const* out,
                                    const int64_t* order, int64_t b0, int32_t n, void* stream) {
  A2M_CHECK_ARG(n_mod >= 1 && n_mod <= A2M_BATCH_MAX_MOD, "batch_gather: n_mod %d outside 1..%d",
                n_mod, A2M_BATCH_MAX_MOD);
  A2M_CHECK_ARG(n >= 0 && b0 >= 0, "batch_gather: n %d or b0 %lld negative", n, (long long)b0);
  if (n == 0) return A2M_OK;
  A2M_CHECK_ARG(arena && start && C && window && interval && mode && mean && std_ && out && order,
                "batch_gather: null argument with n > 0");
  BatchMods M{};
  M.n_mod = n_mod;
  int64_t total = 0;
  for (int m = 0; m < n_mod; ++m) {
    A2M_CHECK_ARG(arena[m] && start[m] && out[m], "batch_gather: modality %d: null arena, start or out", m);
    A2M_CHECK_ARG(C[m] > 0 && C[m] % 4 == 0, "batch_gather: modality %d: C %d is not a positive multiple of 4",
                  m, C[m]);
    A2M_CHECK_ARG(window[m] > 0 && interval[m] > 0, "batch_gather: modality %d: window %d, interval %d",
                  m, window[m], interval[m]);
    A2M_CHECK_ARG(mode[m] >= A2M_BATCH_RAW && mode[m] <= A2M_BATCH_NECKSUB,
                  "batch_gather: modality %d: unknown mode %d", m, mode[m]);
    if (mode[m] == A2M_BATCH_RAW)
      A2M_CHECK_ARG(!mean[m] && !std_[m], "batch_gather: modality %d: mean / std given for the raw mode", m);
    else
      A2M_CHECK_ARG(mean[m] && std_[m], "batch_gather: modality %d: mode %d needs mean and std", m, mode[m]);
    A2M_CHECK_ARG(mode[m] != A2M_BATCH_NECKSUB || C[m] == BPF,
                  "batch_gather: modality %d: the neck-sub mode needs C = 104, got %d", m, C[m]);
    A2M_CHECK_ARG(((uintptr_t)arena[m] | (uintptr_t)out[m]) % 16 == 0,
                  "batch_gather: modality %d: arena and out must be 16-byte aligned", m);
    M.arena[m] = arena[m];
    M.start[m] = start[m];
    M.mean[m] = mean[m];
    M.std_[m] = std_[m];
    M.out[m] = out[m];
    M.c4[m] = C[m] / 4;
    M.nj[m] = (window[m] + interval[m] - 1) / interval[m];
    M.interval[m] = interval[m];
    M.mode[m] = mode[m];
    total += (int64_t)n * M.nj[m] * M.c4[m];
    M.end[m] = total;
  }
  const int blocks = (int)std::min<int64_t>(cdiv(total, 256), 4096);
  hipLaunchKernelGGL(batch_gather_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), M, order, b0);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}
