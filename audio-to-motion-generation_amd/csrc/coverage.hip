// The sample-level set metrics of the device test epoch (a2m.evaluation.CoverageEvaluator; DESIGN.md
// 7.12): precision / recall, density / coverage and diversity are functions of pairwise distances
// between whole clips and of k-th-nearest-neighbour radii.  Four kernels:
//
// coverage_store_kernel: one batch's clips as feature rows of two [capacity][D] buffers, the
// generated clip as the generator gave it, the real one normalised by the loader's formula (every
// step rounded once); feature 'motion' stores the frame differences, one fp32 subtraction each.
//
// pair_dist2_kernel: d2(i,j) = max((|a_i|^2 + |b_j|^2) - 2 a_i.b_j, 0) for two row lists into
// feature buffers.  The tile of nn_search_kernel (baselines.hip) restated for a slab
// output: a workgroup of four waves owns 64 x 64 distances, each wave one 32x32 accumulator of
// mfma_f32_32x32x2f32 (exact fp32: a k-ordered fma chain per output element, the same k order for
// every element), D streamed through LDS in 64-float chunks, register-staged one chunk ahead with
// unconditional loads at clamped addresses, issued together after the barrier; a float4 past D is
// the last float4 times 0.  The norms are summed by the staging threads (an fma chain over each
// thread's float4 column, then a 16-lane tree).  Every value is a function of the two vectors
// alone, so equal vectors give bitwise-equal distances wherever they sit.  Row numbers are clamped
// into the buffers: no list can make the kernel read outside them.
//
// row_kth_kernel: one wave per slab row.  The k-th smallest of the row by k rounds of "the smallest
// key above the last one" on key = bits << 32 | column (the values are >= +0 or +inf, which order
// as their bit patterns; the column makes every key distinct, so ties are ordered by column); and
// the row's sum of sqrt((double) d2) over its finite entries, every lane its strided share in
// ascending order, then a butterfly.
//
// row_cover_kernel: one wave per slab row: the number of columns with d2 <= r2[column] and the
// row's minimum.  Integer adds and minima only.
//
// No atomics, no workspace shared between workgroups, no dependence on scheduling.
#include "a2m_internal.h"

namespace a2m {

constexpr int CV_T = 64;          // tile edge
constexpr int CV_BK = 64;         // floats of D per LDS chunk
constexpr int CV_LD = CV_BK + 4;  // LDS row stride (floats): rows stay 16-byte aligned
constexpr int CV_MAX_K = 32;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ------------------------------------------------------------------------------------ store
struct StoreArgs {
  const float* fake;
  const float* real;
  const int32_t* style;
  const float* mean;
  const float* std_;
  float* feat_fake;
  float* feat_real;
  int32_t* styles;
  int64_t row0, n4;  // n4: float4s of the batch's feature rows
  int n, T, Fd, d4, f4, motion;
};

__device__ __forceinline__ float4 norm4(float4 v, float4 m, float4 s) {
  return make_float4(__fdiv_rn(__fsub_rn(v.x, m.x), s.x < 1e-7f ? 1.f : s.x),
                     __fdiv_rn(__fsub_rn(v.y, m.y), s.y < 1e-7f ? 1.f : s.y),
                     __fdiv_rn(__fsub_rn(v.z, m.z), s.z < 1e-7f ? 1.f : s.z),
                     __fdiv_rn(__fsub_rn(v.w, m.w), s.w < 1e-7f ? 1.f : s.w));
}

__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  return make_float4(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w));
}

__global__ void __launch_bounds__(256) coverage_store_kernel(StoreArgs A) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < A.n) A.styles[A.row0 + i] = A.style[i];
  if (i >= A.n4) return;
  const int64_t b = i / A.d4;
  const int q = (int)(i - b * A.d4);  // float4 of the feature row
  const int t = q / A.f4, c4 = q - t * A.f4;
  const int64_t src = ((b * A.T + t) * A.Fd) / 4 + c4;  // float4 index of frame t
  const float4 m = reinterpret_cast<const float4*>(A.mean)[c4];
  const float4 s = reinterpret_cast<const float4*>(A.std_)[c4];
  const float4* fk = reinterpret_cast<const float4*>(A.fake);
  const float4* rl = reinterpret_cast<const float4*>(A.real);
  float4 f = fk[src], r = norm4(rl[src], m, s);
  if (A.motion) {  // x[t+1] - x[t]
    f = sub4(fk[src + A.f4], f);
    r = sub4(norm4(rl[src + A.f4], m, s), r);
  }
  const int64_t dst = (A.row0 + b) * A.d4 + q;
  reinterpret_cast<float4*>(A.feat_fake)[dst] = f;
  reinterpret_cast<float4*>(A.feat_real)[dst] = r;
}

// ------------------------------------------------------------------------------------ distances
struct PairArgs {
  const float* fa;
  const float* fb;
  const int32_t* rows_a;
  const int32_t* rows_b;
  float* out;  // [nA][nB]
  int64_t cap_a, cap_b;
  int nA, nB, D, exclude_self, diag0;
};

struct PairStage {
  float4 a[4], b[4];
};

__device__ __forceinline__ float cv_sq4(float4 v, float s) {
  return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, s))));
}

__device__ __forceinline__ float4 cv_scale4(float4 v, float s) {
  return make_float4(__fmul_rn(v.x, s), __fmul_rn(v.y, s), __fmul_rn(v.z, s), __fmul_rn(v.w, s));
}

// Chunk `chunk` of D for this thread's four rows of either side.  Every load is unconditional, at
// an address clamped into range: a row past the end of a list is a copy of the last one (its
// results are never stored); a float4 past D is the last float4, and pair_dist2_kernel multiplies
// it by 0.
__device__ __forceinline__ void pair_load(const PairArgs& A, int chunk, int sq, const int64_t* aoff,
                                          const int64_t* boff, PairStage& st) {
  const int kq = min(chunk * (CV_BK / 4) + sq, A.D / 4 - 1);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    st.a[it] = *reinterpret_cast<const float4*>(A.fa + aoff[it] + 4 * (int64_t)kq);
    st.b[it] = *reinterpret_cast<const float4*>(A.fb + boff[it] + 4 * (int64_t)kq);
  }
}

__global__ void __launch_bounds__(256) pair_dist2_kernel(PairArgs A) {
  __shared__ __attribute__((aligned(16))) float As[CV_T * CV_LD];
  __shared__ __attribute__((aligned(16))) float Bs[CV_T * CV_LD];
  __shared__ float aas[CV_T], bbs[CV_T];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ah = wave >> 1, bh = wave & 1;  // the wave's 32 x 32 of the tile
  const int li = lane & 31, lh = lane >> 5;
  const int sq = tid & 15, srow = tid >> 4;  // staging: float4 column of the chunk, first of 4 rows
  const int a0 = blockIdx.y * CV_T, b0 = blockIdx.x * CV_T;
  const int nk = (A.D + CV_BK - 1) / CV_BK;

  int64_t aoff[4], boff[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t ra = A.rows_a[min(a0 + srow + 16 * it, A.nA - 1)];
    const int64_t rb = A.rows_b[min(b0 + srow + 16 * it, A.nB - 1)];
    aoff[it] = min(max(ra, (int64_t)0), A.cap_a - 1) * A.D;
    boff[it] = min(max(rb, (int64_t)0), A.cap_b - 1) * A.D;
  }
  float apart[4] = {0.f, 0.f, 0.f, 0.f}, bpart[4] = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  PairStage st;
  pair_load(A, 0, sq, aoff, boff, st);
  for (int c = 0; c < nk; ++c) {
    // times 1, or times 0 for a float4 past D (a product, not a select: finite values give +-0,
    // which adds nothing to an fma chain that starts at +0)
    const float live = 4 * (int64_t)(c * (CV_BK / 4) + sq) < A.D ? 1.f : 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      st.a[it] = cv_scale4(st.a[it], live);
      st.b[it] = cv_scale4(st.b[it], live);
    }
    __syncthreads();  // the previous chunk's fragments are read
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = srow + 16 * it;
      *reinterpret_cast<float4*>(As + row * CV_LD + 4 * sq) = st.a[it];
      *reinterpret_cast<float4*>(Bs + row * CV_LD + 4 * sq) = st.b[it];
      apart[it] = cv_sq4(st.a[it], apart[it]);
      bpart[it] = cv_sq4(st.b[it], bpart[it]);
    }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);       // the stage is consumed: its registers take the next loads
    pair_load(A, c + 1, sq, aoff, boff, st);  // past the last chunk: clamped, never stored
    __builtin_amdgcn_sched_barrier(0);       // the loads are issued ahead of the MFMAs they overlap
    // MFMA step: lane half h supplies k = 32 h + s of the chunk, s = 0..31, for A and B alike
    const float* pa = As + (ah * 32 + li) * CV_LD + lh * 32;
    const float* pb = Bs + (bh * 32 + li) * CV_LD + lh * 32;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float4 a = *reinterpret_cast<const float4*>(pa + 4 * t);
      const float4 b = *reinterpret_cast<const float4*>(pb + 4 * t);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
  }
  // the norms: the 16 staging threads of a row are one 16-lane DPP row
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const float aa = row16_sum(apart[it]), bb = row16_sum(bpart[it]);
    if (sq == 0) {
      aas[srow + 16 * it] = aa;
      bbs[srow + 16 * it] = bb;
    }
  }
  __syncthreads();
  const int j = b0 + bh * 32 + li;  // this lane's column of the slab: the accumulator's column
  if (j < A.nB) {
    const float bb = bbs[bh * 32 + li];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ah * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int i = a0 + row;
      if (i < A.nA) {
        float d = __fsub_rn(__fadd_rn(aas[row], bb), __fmul_rn(2.f, acc[r]));
        d = d > 0.f ? d : 0.f;
        if (A.exclude_self && j == i + A.diag0) d = __builtin_inff();
        A.out[(int64_t)i * A.nB + j] = d;
      }
    }
  }
}

// ------------------------------------------------------------------------------------ row passes
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long o = __shfl_xor(k, m);
    k = o < k ? o : k;
  }
  return k;
}

__global__ void __launch_bounds__(256) row_kth_kernel(const float* __restrict__ slab, int nA, int nB, int k,
                                                      float* __restrict__ kth, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nA) return;  // whole waves leave: the shuffles below stay among a wave's 64 lanes
  const unsigned* x = reinterpret_cast<const unsigned*>(slab) + (int64_t)row * nB;
  unsigned long long prev = 0;
  for (int round = 0; round < k; ++round) {
    unsigned long long best = ~0ull;
    for (int j = lane; j < nB; j += 64) {
      const unsigned long long key = ((unsigned long long)x[j] << 32) | (unsigned)j;
      // round 0 takes every key (key 0 itself: +0 in column 0, is above nothing yet)
      best = ((round == 0 || key > prev) && key < best) ? key : best;
    }
    prev = wave_min_u64(best);
  }
  double s = 0.0;
  for (int j = lane; j < nB; j += 64) {
    const float v = __uint_as_float(x[j]);
    if (v < __builtin_inff()) s += __dsqrt_rn((double)v);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0) {
    kth[row] = __uint_as_float((unsigned)(prev >> 32));
    sums[row] = s;
  }
}

__global__ void __launch_bounds__(256) row_cover_kernel(const float* __restrict__ slab, int nA, int nB,
                                                        const float* __restrict__ r2, int32_t* __restrict__ count,
                                                        float* __restrict__ rowmin) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nA) return;
  const float* x = slab + (int64_t)row * nB;
  int n = 0;
  unsigned lo = 0x7f800000u;  // +inf: the values are >= +0 or +inf and order as their bits
  for (int j = lane; j < nB; j += 64) {
    const float v = x[j];
    n += v <= r2[j] ? 1 : 0;
    lo = min(lo, __float_as_uint(v));
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    n += __shfl_xor(n, m);
    lo = min(lo, (unsigned)__shfl_xor((int)lo, m));
  }
  if (lane == 0) {
    count[row] = n;
    rowmin[row] = __uint_as_float(lo);
  }
}

constexpr int64_t CV_MAX_N = 65535 * (int64_t)CV_T;  // rows of a slab: the tile grid's y extent

}  // namespace a2m

using namespace a2m;

extern "C" int a2m_coverage_store_f32(const float* fake_norm, const float* real_px, const int32_t* style,
                                      const float* mean, const float* std_, int32_t n, int32_t T, int32_t Fd,
                                      int32_t feature, int64_t row0, int64_t capacity, float* feat_fake,
                                      float* feat_real, int32_t* styles, void* stream) {
  A2M_CHECK_ARG(fake_norm && real_px && style && mean && std_ && feat_fake && feat_real && styles,
                "coverage_store: null argument");
  A2M_CHECK_ARG(feature == A2M_COVERAGE_POSE || feature == A2M_COVERAGE_MOTION, "coverage_store: unknown feature %d",
                feature);
  A2M_CHECK_ARG(n > 0 && T > feature, "coverage_store: n %d, T %d (motion needs T >= 2)", n, T);
  A2M_CHECK_ARG(Fd > 0 && Fd % 4 == 0, "coverage_store: Fd %d is not a positive multiple of 4", Fd);
  A2M_CHECK_ARG(row0 >= 0 && capacity > 0 && row0 <= capacity - n, "coverage_store: rows [%lld, %lld) outside capacity %lld",
                (long long)row0, (long long)row0 + n, (long long)capacity);
  A2M_CHECK_ARG(((uintptr_t)fake_norm | (uintptr_t)real_px | (uintptr_t)mean | (uintptr_t)std_ | (uintptr_t)feat_fake |
                 (uintptr_t)feat_real) % 16 == 0,
                "coverage_store: the poses, mean, std and the feature buffers must be 16-byte aligned");
  A2M_CHECK_ARG(((uintptr_t)style | (uintptr_t)styles) % 4 == 0, "coverage_store: style ids must be 4-byte aligned");
  const int64_t D = (int64_t)(T - feature) * Fd;
  A2M_CHECK_ARG(D <= ((int64_t)1 << 30), "coverage_store: D = %lld exceeds 2^30", (long long)D);
  A2M_CHECK_ARG((int64_t)n * (D / 4) < ((int64_t)1 << 38), "coverage_store: n*D = %d * %lld reaches 2^40", n, (long long)D);
  StoreArgs A{};
  A.fake = fake_norm; A.real = real_px; A.style = style; A.mean = mean; A.std_ = std_;
  A.feat_fake = feat_fake; A.feat_real = feat_real; A.styles = styles;
  A.row0 = row0; A.n = n; A.T = T; A.Fd = Fd; A.d4 = (int)(D / 4); A.f4 = Fd / 4; A.motion = feature;
  A.n4 = (int64_t)n * A.d4;
  hipLaunchKernelGGL(coverage_store_kernel, dim3((unsigned)cdiv(A.n4, 256)), dim3(256), 0, as_stream(stream), A);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

extern "C" size_t a2m_pair_dist2_ws_bytes(int64_t nA, int64_t nB) {
  if (nA <= 0 || nB <= 0 || nA > CV_MAX_N || nB > (int64_t)0x7fff0000) return 0;
  return (size_t)nA * (size_t)nB * sizeof(float);
}

extern "C" int a2m_pair_dist2_f32(const float* feat_a, int64_t cap_a, const int32_t* rows_a, int64_t nA,
                                  const float* feat_b, int64_t cap_b, const int32_t* rows_b, int64_t nB, int64_t D,
                                  int32_t exclude_self, int64_t diag0, float* slab, size_t slab_bytes,
                                  void* stream) {
  A2M_CHECK_ARG(feat_a && feat_b && rows_a && rows_b && slab, "pair_dist2: null argument");
  A2M_CHECK_ARG(nA > 0 && nB > 0 && cap_a > 0 && cap_b > 0, "pair_dist2: nA %lld, nB %lld, capacities %lld, %lld",
                (long long)nA, (long long)nB, (long long)cap_a, (long long)cap_b);
  A2M_CHECK_ARG(D > 0 && D % 4 == 0, "pair_dist2: D %lld is not a positive multiple of 4", (long long)D);
  A2M_CHECK_ARG(D <= ((int64_t)1 << 30), "pair_dist2: D %lld exceeds 2^30", (long long)D);
  A2M_CHECK_ARG(nA <= CV_MAX_N, "pair_dist2: nA %lld exceeds %lld", (long long)nA, (long long)CV_MAX_N);
  A2M_CHECK_ARG(nB <= (int64_t)0x7fff0000, "pair_dist2: nB %lld exceeds 2^31 - 2^16", (long long)nB);
  A2M_CHECK_ARG(cap_a <= (int64_t)0x7fffffff && cap_b <= (int64_t)0x7fffffff,
                "pair_dist2: a capacity beyond 2^31 - 1 rows (32-bit row numbers)");
  A2M_CHECK_ARG(exclude_self == 0 || exclude_self == 1, "pair_dist2: exclude_self %d", exclude_self);
  A2M_CHECK_ARG(diag0 >= 0 && (exclude_self ? diag0 + nA <= nB : diag0 == 0),
                "pair_dist2: diag0 %lld (with exclude_self the diagonal (i, diag0 + i) must lie inside the slab)",
                (long long)diag0);
  A2M_CHECK_ARG(((uintptr_t)feat_a | (uintptr_t)feat_b) % 16 == 0, "pair_dist2: the feature buffers must be 16-byte aligned");
  A2M_CHECK_ARG(((uintptr_t)rows_a | (uintptr_t)rows_b | (uintptr_t)slab) % 4 == 0,
                "pair_dist2: the row lists and the slab must be 4-byte aligned");
  A2M_CHECK_ARG(slab_bytes >= a2m_pair_dist2_ws_bytes(nA, nB), "pair_dist2: slab_bytes %zu < %zu", slab_bytes,
                a2m_pair_dist2_ws_bytes(nA, nB));
  PairArgs A{};
  A.fa = feat_a; A.fb = feat_b; A.rows_a = rows_a; A.rows_b = rows_b; A.out = slab;
  A.cap_a = cap_a; A.cap_b = cap_b; A.nA = (int)nA; A.nB = (int)nB; A.D = (int)D;
  A.exclude_self = exclude_self; A.diag0 = (int)diag0;
  hipLaunchKernelGGL(pair_dist2_kernel, dim3((unsigned)cdiv(nB, CV_T), (unsigned)cdiv(nA, CV_T)), dim3(256), 0,
                     as_stream(stream), A);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

static int check_slab(const char* who, const float* slab, int64_t nA, int64_t nB) {
  A2M_CHECK_ARG(slab, "%s: null argument", who);
  A2M_CHECK_ARG(nA > 0 && nB > 0, "%s: nA %lld or nB %lld is not positive", who, (long long)nA, (long long)nB);
  A2M_CHECK_ARG(nA <= (int64_t)0x7fff0000 && nB <= (int64_t)0x7fff0000, "%s: nA %lld or nB %lld exceeds 2^31 - 2^16", who,
                (long long)nA, (long long)nB);
  A2M_CHECK_ARG((uintptr_t)slab % 4 == 0, "%s: the slab must be 4-byte aligned", who);
  return A2M_OK;
}

extern "C" int a2m_row_kth_f32(const float* slab, int64_t nA, int64_t nB, int32_t k, int32_t exclude_self, float* kth,
                               double* sums, void* stream) {
  if (int rc = check_slab("row_kth", slab, nA, nB)) return rc;
  A2M_CHECK_ARG(kth && sums, "row_kth: null argument");
  A2M_CHECK_ARG(k >= 1 && k <= CV_MAX_K, "row_kth: k %d outside 1..%d", k, CV_MAX_K);
  A2M_CHECK_ARG(exclude_self == 0 || exclude_self == 1, "row_kth: exclude_self %d", exclude_self);
  A2M_CHECK_ARG(k <= nB - exclude_self, "row_kth: k %d needs %d columns%s, the slab has %lld", k, k + exclude_self,
                exclude_self ? " (one is the row's own)" : "", (long long)nB);
  A2M_CHECK_ARG((uintptr_t)kth % 4 == 0 && (uintptr_t)sums % 8 == 0, "row_kth: kth must be 4-byte and sums 8-byte aligned");
  hipLaunchKernelGGL(row_kth_kernel, dim3((unsigned)cdiv(nA, 4)), dim3(256), 0, as_stream(stream), slab, (int)nA,
                     (int)nB, k, kth, sums);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

extern "C" int a2m_row_cover_f32(const float* slab, int64_t nA, int64_t nB, const float* r2, int32_t* count,
                                 float* rowmin, void* stream) {
  if (int rc = check_slab("row_cover", slab, nA, nB)) return rc;
  A2M_CHECK_ARG(r2 && count && rowmin, "row_cover: null argument");
  A2M_CHECK_ARG(((uintptr_t)r2 | (uintptr_t)count | (uintptr_t)rowmin) % 4 == 0,
                "row_cover: r2, count and rowmin must be 4-byte aligned");
  hipLaunchKernelGGL(row_cover_kernel, dim3((unsigned)cdiv(nA, 4)), dim3(256), 0, as_stream(stream), slab, (int)nA,
                     (int)nB, r2, count, rowmin);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}
