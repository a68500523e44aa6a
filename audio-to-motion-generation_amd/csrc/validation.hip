// The per-batch kernels of the validation pass (version5_model_train.py:438-480).
//   val_motion   pos_to_motion of the generated and the real pose (:452-453) into one stacked
//                [2B][T-1][Fd] buffer for a single discriminator forward, and per clip the sums
//                behind the motion L1 (:467), the smoothness (:216-230) and the jerk (:233-248)
//   val_finish   those sums over the clips, the three MSE terms of :469-476 on D's logits and the
//                generator's bone / angle scalars, added to an fp64 accumulator the host reads
//                once per epoch
#include <algorithm>

#include "a2m_internal.h"

namespace a2m {
namespace {

constexpr int kValThreads = 256;
constexpr int kValFinishThreads = 64;   // the finish kernel is one wave
constexpr int kValTile = 64;            // time steps per trip: one quad of lanes each
constexpr int kValHalo = 3;             // a jerk at t reads pose rows t .. t + 3
constexpr size_t kValLds = 60 << 10;    // dynamic LDS of one workgroup (the static part rides on top)

// sum over the workgroup in a fixed order (wave butterflies, then the waves ascending)
__device__ __forceinline__ double val_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  __syncthreads();
  return s;
}

// One workgroup per clip.  The clip's pose rows pass through two LDS rings of R = tt + 3 rows
// (pose row t in slot t % R): every trip brings in the rows it is the first to need with
// coalesced loads, so each pose element leaves global memory once, and serves
//   - the motion rows t0 .. t0 + nr - 1 of both poses and their L1 difference, one element per
//     thread in memory order (coalesced stores), and
//   - the acceleration and jerk norms of those time steps, four lanes per time step (a DPP
//     quad), each summing every fourth feature, as motion_terms_kernel (train_loss.hip) does.
// A trip's new rows land in the slots of rows older than t0, which no later trip reads.
// The partial sums stay in fp64 registers across the trips; no per-time array, so no bound on T.
__global__ __launch_bounds__(kValThreads) void val_motion_kernel(const float* __restrict__ fake,
                                                                 const float* __restrict__ real, int B, int T,
                                                                 int Fd, int tt, float* __restrict__ motion,
                                                                 double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float val_ring[];
  __shared__ double red[kValThreads / 64];
  const int R = tt + kValHalo;
  float* fk = val_ring;
  float* rl = val_ring + R * Fd;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* fp = fake + (int64_t)b * T * Fd;
  const float* rp = real + (int64_t)b * T * Fd;
  float* mf_out = motion + (int64_t)b * (T - 1) * Fd;
  float* mr_out = motion + ((int64_t)B + b) * (T - 1) * Fd;
  double l1 = 0.0, sa = 0.0, sj = 0.0;
  int loaded = 0;  // pose rows [0, loaded) have been brought in
  for (int t0 = 0; t0 < T - 1; t0 += tt) {
    const int nr = min(tt, T - 1 - t0);              // motion rows of this trip
    const int hi = min(t0 + nr + kValHalo, T);       // it reads pose rows [t0, hi)
    for (int i = loaded * Fd + tid; i < hi * Fd; i += kValThreads) {
      const int t = i / Fd, f = i - t * Fd;
      const int s = (t % R) * Fd + f;
      fk[s] = fp[i];
      rl[s] = rp[i];
    }
    loaded = hi;
    __syncthreads();
    for (int i = tid; i < nr * Fd; i += kValThreads) {
      const int tl = i / Fd, f = i - tl * Fd, t = t0 + tl;
      const int s0 = (t % R) * Fd + f, s1 = ((t + 1) % R) * Fd + f;
      const float mf = fk[s1] - fk[s0], mr = rl[s1] - rl[s0];
      mf_out[t0 * Fd + i] = mf;
      mr_out[t0 * Fd + i] = mr;
      l1 += fabsf(mr - mf);
    }
    const int tl = tid >> 2, q = tid & 3, t = t0 + tl;
    const bool ha = tl < nr && t < T - 2, hj = tl < nr && t < T - 3;  // uniform over a quad
    float a2 = 0.f, j2 = 0.f;
    if (ha) {
      const float* r0 = fk + (t % R) * Fd;
      const float* r1 = fk + ((t + 1) % R) * Fd;
      const float* r2 = fk + ((t + 2) % R) * Fd;
      const float* r3 = fk + ((t + 3) % R) * Fd;   // read only where the jerk exists (t + 3 < T)
      for (int f = q; f < Fd; f += 4) {
        const float m0 = r1[f] - r0[f], m1 = r2[f] - r1[f];
        const float a = m1 - m0;
        a2 += a * a;
        if (hj) {
          const float m2 = r3[f] - r2[f];
          const float j = (m2 - m1) - (m1 - m0);
          j2 += j * j;
        }
      }
    }
    a2 = quad_sum(a2);
    j2 = quad_sum(j2);
    if (q == 0) {
      if (ha) sa += sqrtf(a2);
      if (hj) sj += sqrtf(j2);
    }
    __syncthreads();  // the next trip's rows overwrite slots this one has read
  }
  l1 = val_block_sum(l1, red);
  sa = val_block_sum(sa, red);
  sj = val_block_sum(sj, red);
  if (tid == 0) {
    part[3 * b] = l1;
    part[3 * b + 1] = sa;
    part[3 * b + 2] = sj;
  }
}

// One workgroup of one wave (the work is B * (3 + 2 L) values): the clips' partials and the logits,
// each lane a strided share in ascending order, then val_block_sum -- the same order every run.
__global__ __launch_bounds__(kValFinishThreads) void val_finish_kernel(const double* __restrict__ part, int B, int T,
                                                                 int Fd, const float* __restrict__ logits, int L,
                                                                 const float* __restrict__ bone,
                                                                 const float* __restrict__ angle, float lambda_gan,
                                                                 float lambda_d, double* __restrict__ acc) {
  __shared__ double red[kValFinishThreads / 64];
  const int tid = threadIdx.x;
  double l1 = 0.0, sa = 0.0, sj = 0.0;
  for (int b = tid; b < B; b += kValFinishThreads) {
    l1 += part[3 * b];
    sa += part[3 * b + 1];
    sj += part[3 * b + 2];
  }
  const int64_t n = (int64_t)B * L;   // logits of the fake rows, then of the real rows
  double f1 = 0.0, f0 = 0.0, r1 = 0.0;
  for (int64_t i = tid; i < n; i += kValFinishThreads) {
    const double f = (double)logits[i], r = (double)logits[n + i];
    f1 += (f - 1.0) * (f - 1.0);
    f0 += f * f;
    r1 += (r - 1.0) * (r - 1.0);
  }
  l1 = val_block_sum(l1, red);
  sa = val_block_sum(sa, red);
  sj = val_block_sum(sj, red);
  f1 = val_block_sum(f1, red);
  f0 = val_block_sum(f0, red);
  r1 = val_block_sum(r1, red);
  if (tid != 0) return;
  const double motion_l1 = l1 / ((double)B * (T - 1) * Fd);
  const double smooth = T > 2 ? sa / ((double)B * (T - 2)) : 0.0;
  const double jerk = T > 3 ? sj / ((double)B * (T - 3)) : 0.0;
  acc[0] += motion_l1 + (double)lambda_gan * (f1 / (double)n);
  acc[1] += r1 / (double)n + (double)lambda_d * (f0 / (double)n);
  acc[2] += (double)bone[0];
  acc[3] += (double)angle[0];
  acc[4] += smooth;
  acc[5] += jerk;
  acc[6] += motion_l1;
  acc[7] += 1.0;
}

}  // namespace
}  // namespace a2m

using namespace a2m;

extern "C" {

int a2m_val_motion_f32(const float* fake_pose, const float* real_pose, int32_t B, int32_t T, int32_t Fd,
                       float* motion, double* part, void* stream) {
  A2M_CHECK_ARG(fake_pose && real_pose && motion && part && B > 0 && T >= 2 && Fd > 0,
                "val_motion: bad args");
  // both rings hold tt + 3 rows of Fd floats; the kernel indexes one clip with 32-bit ints
  const int64_t rows = (int64_t)(kValLds / (2 * sizeof(float))) / Fd;
  A2M_CHECK_ARG(rows > kValHalo && (int64_t)T * Fd <= INT32_MAX,
                "val_motion: Fd = %d, T = %d beyond the kernel's limits (Fd <= 1920, T * Fd < 2^31)", Fd, T);
  const int tt = (int)std::min<int64_t>(kValTile, rows - kValHalo);
  const size_t lds = 2 * sizeof(float) * (size_t)(tt + kValHalo) * Fd;
  hipLaunchKernelGGL(val_motion_kernel, dim3(B), dim3(kValThreads), lds, as_stream(stream), fake_pose,
                     real_pose, B, T, Fd, tt, motion, part);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_val_finish_f32(const double* part, int32_t B, int32_t T, int32_t Fd, const float* logits, int32_t L,
                       const float* bone, const float* angle, float lambda_gan, float lambda_d, double* acc,
                       void* stream) {
  A2M_CHECK_ARG(part && logits && bone && angle && acc && B > 0 && T >= 2 && Fd > 0 && L > 0,
                "val_finish: bad args");
  hipLaunchKernelGGL(val_finish_kernel, dim3(1), dim3(kValFinishThreads), 0, as_stream(stream), part, B, T, Fd,
                     logits, L, bone, angle, lambda_gan, lambda_d, acc);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

}  // extern "C"
