// Train-time augmentation inside the loader's gather (a2m/data.py Augment, PatsLoader.pairs(...,
// augment=)): a draw kernel that fills a [n][8] parameter table for the clips order[b0 .. b0+n)
// from a counter-based generator, and batch_gather_kernel's (data.hip) batch with tempo, mirror,
// scale, gain and masks applied while it is formed.  Nothing is copied, nothing comes back to the
// host: both launches capture into a HIP graph, and a replay follows an overwritten order and pass
// number.  Every float step is one correctly rounded fp32 operation and no product is contracted
// with a sum (mul_rn below), so tests/augment_ref.py restates both kernels exactly.
// batch_gather_kernel itself is untouched.
#include "a2m_internal.h"

namespace a2m {

constexpr int APF = 104, APJ = 52;  // planar pose [2][52], as data.hip
constexpr int NPAR = A2M_AUGMENT_NPARAM;

struct AugDraw {
  uint32_t key0, key1;
  float p_mirror, r_speed, r_scale, r_gain;
  int max_fw, C, max_tw, T;
};

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1) bumped by the Weyl constants
// between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// A rounded product that stays one: the build (-ffp-contract=fast) fuses a product and a following
// sum into one multiply-add in the back end, through __fmul_rn / __fadd_rn alike (see
// pose_denormalize_kernel, evaluation.hip); a value that passes an empty asm cannot be fused.
__device__ __forceinline__ float mul_rn(float a, float b) {
  float t = a * b;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ float unit24(uint32_t x) { return (float)(x >> 8) * 0x1p-24f; }  // [0, 1), exact

// r * (2u - 1): 2u and 2u - 1 are exact, the product is the one rounding
__device__ __forceinline__ float spread(float r, float u) {
  return mul_rn(r, __fsub_rn(mul_rn(2.f, u), 1.f));
}

// One thread a clip.  Counter (pos_lo, pos_hi, pass, call): the parameters of a clip are a function
// of (seed, pass, pos) alone.
__global__ void augment_params_kernel(AugDraw D, const int64_t* __restrict__ order, int64_t b0, int n,
                                      const int64_t* __restrict__ pass, float* __restrict__ params) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const uint64_t pos = (uint64_t)order[b0 + b];
  const uint32_t pw = (uint32_t)pass[0];
  uint32_t c[4] = {(uint32_t)pos, (uint32_t)(pos >> 32), pw, 0u};
  philox4x32_10(c, D.key0, D.key1);
  float* P = params + (int64_t)b * NPAR;
  P[0] = unit24(c[0]) < D.p_mirror ? 1.f : 0.f;
  P[1] = __fadd_rn(1.f, spread(D.r_speed, unit24(c[1])));
  P[2] = __fadd_rn(1.f, spread(D.r_scale, unit24(c[2])));
  P[3] = spread(D.r_gain, unit24(c[3]));
  uint32_t d[4] = {(uint32_t)pos, (uint32_t)(pos >> 32), pw, 1u};
  philox4x32_10(d, D.key0, D.key1);
  // u <= 1 - 2^-24 and k < 2^24, so fl(u * k) < k: a width never exceeds its maximum
  const float fw = floorf(mul_rn(unit24(d[0]), (float)(D.max_fw + 1)));
  const float f0 = floorf(mul_rn(unit24(d[1]), (float)(D.C - (int)fw + 1)));
  const float tw = floorf(mul_rn(unit24(d[2]), (float)(D.max_tw + 1)));
  const float t0 = floorf(mul_rn(unit24(d[3]), (float)(D.T - (int)tw + 1)));
  P[4] = f0;
  P[5] = fw;
  P[6] = t0;
  P[7] = tw;
}

struct AugMods {
  const float* arena[A2M_BATCH_MAX_MOD];
  const int64_t* start[A2M_BATCH_MAX_MOD];
  const int64_t* last[A2M_BATCH_MAX_MOD];
  const float* mean[A2M_BATCH_MAX_MOD];
  const float* std_[A2M_BATCH_MAX_MOD];
  float* out[A2M_BATCH_MAX_MOD];
  int64_t end[A2M_BATCH_MAX_MOD];  // running total of float4 items up to and including modality m
  int c4[A2M_BATCH_MAX_MOD], nj[A2M_BATCH_MAX_MOD], interval[A2M_BATCH_MAX_MOD], mode[A2M_BATCH_MAX_MOD],
      role[A2M_BATCH_MAX_MOD];
  int n_mod;
};

// a + f (b - a), three roundings
__device__ __forceinline__ float lerp_rn(float a, float b, float f) {
  return __fadd_rn(a, mul_rn(f, __fsub_rn(b, a)));
}

// The item layout of batch_gather_kernel: item i of modality m is float4 q of output row (b, j).
// Row position p = fl(float(j * interval) * s) from the sample's start; rows a = floor(p) and a + 1,
// both clamped at the interval's last row; with a zero fraction row a + 1 is not read.
__global__ void batch_gather_aug_kernel(AugMods M, const int64_t* __restrict__ order, int64_t b0,
                                        const float* __restrict__ params, const int32_t* __restrict__ perm,
                                        float mask_fill) {
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
    const float* P = params + b * NPAR;
    const int64_t pos = order[b0 + b];
    const int64_t start = M.start[m][pos], last = M.last[m][pos];
    // the clamps change nothing for a drawn s in [0.5, 1.5]; they keep a caller's table (a negative,
    // huge or NaN speed) from addressing rows before the sample or converting a non-number
    const float p = fminf(fmaxf(mul_rn((float)(j * M.interval[m]), P[1]), 0.f), 16777216.f);
    const float fl = floorf(p);
    const float f = __fsub_rn(p, fl);
    const bool two = f != 0.f;
    const int64_t r0 = start + (int64_t)fl;
    const int64_t ra = r0 < last ? r0 : last, rb = r0 + 1 < last ? r0 + 1 : last;
    const float* A = M.arena[m] + ra * (4 * (int64_t)c4);
    const float* B = M.arena[m] + rb * (4 * (int64_t)c4);
    const int role = M.role[m], mode = M.mode[m];
    float x[4];
    if (mode == A2M_BATCH_NECKSUB) {
      const float* mean = M.mean[m] + 4 * q;
      const float* sd = M.std_[m] + 4 * q;
      const bool aug = role == A2M_AUGMENT_POSE;
      const bool mir = aug && P[0] != 0.f;
      const int plane = 4 * q < APJ ? 0 : APJ;
      float neck = A[plane];
      if (two) neck = lerp_rn(neck, B[plane], f);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int jt = 4 * q + k - plane;
        int sj = jt;
        if (mir) {
          const int pk = perm[jt];
          sj = (unsigned)pk < (unsigned)APJ ? pk : jt;
        }
        float v = A[plane + sj];
        if (two) v = lerp_rn(v, B[plane + sj], f);
        float d = __fsub_rn(v, neck);
        if (mir && plane == 0) d = -d;
        if (aug) d = mul_rn(d, P[2]);
        x[k] = __fdiv_rn(__fsub_rn(d, mean[k]), sd[k]);  // batch_gather_kernel's: no guard on std
      }
    } else {
      const float4 va = reinterpret_cast<const float4*>(A)[q];
      x[0] = va.x, x[1] = va.y, x[2] = va.z, x[3] = va.w;
      if (two) {
        const float4 vb = reinterpret_cast<const float4*>(B)[q];
        const float y[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = lerp_rn(x[k], y[k], f);
      }
      const bool audio = role == A2M_AUGMENT_AUDIO;
      // a zero gain is not added: x + 0 would turn a -0 into +0, and Augment() is the identity
      if (audio && P[3] != 0.f) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = __fadd_rn(x[k], P[3]);
      }
      if (mode == A2M_BATCH_STANDARDISE) {
        const float* mean = M.mean[m] + 4 * q;
        const float* sd = M.std_[m] + 4 * q;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          x[k] = __fdiv_rn(__fsub_rn(x[k], mean[k]), sd[k] < 1e-7f ? 1.f : sd[k]);
      }
      if (audio) {
        const int f0 = (int)P[4], fw = (int)P[5], t0 = (int)P[6], tw = (int)P[7];
        const bool trun = j >= t0 && j < t0 + tw;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = 4 * q + k;
          if (trun || (c >= f0 && c < f0 + fw)) x[k] = mask_fill;
        }
      }
    }
    reinterpret_cast<float4*>(M.out[m])[r] = make_float4(x[0], x[1], x[2], x[3]);
  }
}

}  // namespace a2m

using namespace a2m;

extern "C" int a2m_augment_params_f32(const int64_t* order, int64_t b0, int32_t n, const int64_t* pass,
                                      uint64_t seed, float p_mirror, float r_speed, float r_scale,
                                      float r_gain, int32_t max_fw, int32_t C, int32_t max_tw, int32_t T,
                                      float* params, void* stream) {
  A2M_CHECK_ARG(n >= 0 && b0 >= 0, "augment_params: n %d or b0 %lld negative", n, (long long)b0);
  A2M_CHECK_ARG(p_mirror >= 0.f && p_mirror <= 1.f, "augment_params: p_mirror %g outside [0, 1]", p_mirror);
  A2M_CHECK_ARG(r_speed >= 0.f && r_speed <= 0.5f, "augment_params: r_speed %g outside [0, 0.5]", r_speed);
  A2M_CHECK_ARG(r_scale >= 0.f && r_scale < 1.f, "augment_params: r_scale %g outside [0, 1)", r_scale);
  A2M_CHECK_ARG(r_gain >= 0.f && r_gain <= 3.0e38f, "augment_params: r_gain %g negative or not finite", r_gain);
  A2M_CHECK_ARG(C > 0 && T > 0 && C < (1 << 24) && T < (1 << 24), "augment_params: C %d or T %d outside 1..2^24-1", C, T);
  A2M_CHECK_ARG(max_fw >= 0 && max_fw <= C, "augment_params: max_fw %d outside [0, C = %d]", max_fw, C);
  A2M_CHECK_ARG(max_tw >= 0 && max_tw <= T, "augment_params: max_tw %d outside [0, T = %d]", max_tw, T);
  if (n == 0) return A2M_OK;
  A2M_CHECK_ARG(order && pass && params, "augment_params: null order, pass or params with n > 0");
  AugDraw D{(uint32_t)seed, (uint32_t)(seed >> 32), p_mirror, r_speed, r_scale, r_gain, max_fw, C, max_tw, T};
  hipLaunchKernelGGL(augment_params_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, as_stream(stream), D,
                     order, b0, n, pass, params);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

extern "C" int a2m_batch_gather_aug_f32(int32_t n_mod, const float* const* arena,
                                        const int64_t* const* start, const int64_t* const* last,
                                        const int32_t* C, const int32_t* window, const int32_t* interval,
                                        const int32_t* mode, const int32_t* role, const float* const* mean,
                                        const float* const* std_, float* const* out, const int64_t* order,
                                        int64_t b0, int32_t n, const float* params, const int32_t* perm,
                                        float mask_fill, void* stream) {
  A2M_CHECK_ARG(n_mod >= 1 && n_mod <= A2M_BATCH_MAX_MOD, "batch_gather_aug: n_mod %d outside 1..%d",
                n_mod, A2M_BATCH_MAX_MOD);
  A2M_CHECK_ARG(n >= 0 && b0 >= 0, "batch_gather_aug: n %d or b0 %lld negative", n, (long long)b0);
  if (n == 0) return A2M_OK;
  A2M_CHECK_ARG(arena && start && last && C && window && interval && mode && role && mean && std_ && out &&
                    order && params && perm,
                "batch_gather_aug: null argument with n > 0");
  AugMods M{};
  M.n_mod = n_mod;
  int64_t total = 0;
  for (int m = 0; m < n_mod; ++m) {
    A2M_CHECK_ARG(arena[m] && start[m] && last[m] && out[m],
                  "batch_gather_aug: modality %d: null arena, start, last or out", m);
    A2M_CHECK_ARG(C[m] > 0 && C[m] % 4 == 0, "batch_gather_aug: modality %d: C %d is not a positive multiple of 4",
                  m, C[m]);
    A2M_CHECK_ARG(window[m] > 0 && interval[m] > 0, "batch_gather_aug: modality %d: window %d, interval %d",
                  m, window[m], interval[m]);
    A2M_CHECK_ARG(mode[m] >= A2M_BATCH_RAW && mode[m] <= A2M_BATCH_NECKSUB,
                  "batch_gather_aug: modality %d: unknown mode %d", m, mode[m]);
    if (mode[m] == A2M_BATCH_RAW)
      A2M_CHECK_ARG(!mean[m] && !std_[m], "batch_gather_aug: modality %d: mean / std given for the raw mode", m);
    else
      A2M_CHECK_ARG(mean[m] && std_[m], "batch_gather_aug: modality %d: mode %d needs mean and std", m, mode[m]);
    A2M_CHECK_ARG(mode[m] != A2M_BATCH_NECKSUB || C[m] == APF,
                  "batch_gather_aug: modality %d: the neck-sub mode needs C = 104, got %d", m, C[m]);
    A2M_CHECK_ARG(role[m] >= A2M_AUGMENT_NONE && role[m] <= A2M_AUGMENT_AUDIO,
                  "batch_gather_aug: modality %d: unknown role %d", m, role[m]);
    A2M_CHECK_ARG(role[m] != A2M_AUGMENT_POSE || mode[m] == A2M_BATCH_NECKSUB,
                  "batch_gather_aug: modality %d: the pose role needs the neck-sub mode, got mode %d", m, mode[m]);
    A2M_CHECK_ARG(role[m] != A2M_AUGMENT_AUDIO || mode[m] != A2M_BATCH_NECKSUB,
                  "batch_gather_aug: modality %d: the audio role does not go with the neck-sub mode", m);
    A2M_CHECK_ARG((int64_t)window[m] < (1 << 24), "batch_gather_aug: modality %d: window %d is 2^24 or more", m,
                  window[m]);
    A2M_CHECK_ARG(((uintptr_t)arena[m] | (uintptr_t)out[m]) % 16 == 0,
                  "batch_gather_aug: modality %d: arena and out must be 16-byte aligned", m);
    M.arena[m] = arena[m];
    M.start[m] = start[m];
    M.last[m] = last[m];
    M.mean[m] = mean[m];
    M.std_[m] = std_[m];
    M.out[m] = out[m];
    M.c4[m] = C[m] / 4;
    M.nj[m] = (window[m] + interval[m] - 1) / interval[m];
    M.interval[m] = interval[m];
    M.mode[m] = mode[m];
    M.role[m] = role[m];
    total += (int64_t)n * M.nj[m] * M.c4[m];
    M.end[m] = total;
  }
  const int blocks = (int)std::min<int64_t>(cdiv(total, 256), 4096);
  hipLaunchKernelGGL(batch_gather_aug_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), M, order, b0,
                     params, perm, mask_fill);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}
