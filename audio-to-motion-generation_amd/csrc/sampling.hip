// The device half of PatsLoader.train_sampler (a2m/sampling.py): the mean joint speed of every
// clip of a split, exact order statistics of those speeds, and the binning of the clips.
//
// clip_velocity_kernel: a clip is addressed as batch_gather_kernel (data.hip) addresses it, rows
// arena[start[i] + t*interval], t < T, read in place.  One wave owns a clip.  The (T-1)*(K-1) terms
// (frame pair t, non-neck joint j) are dealt to the lanes in item order, item = t*(K-1) + (j-1),
// lane l taking items l, l + 64, ...: neighbouring lanes read neighbouring joints of one row, and
// every load of the loop is independent of the arithmetic, so the unrolled loop keeps several rows
// in flight.  A row is read twice (as frame t and as frame t-1 of the next pair), the second time
// from the CU's L1.  Each lane adds its terms in double in item order, the 64 partial sums meet in a
// fixed xor tree, lane 0 divides and rounds once: no atomics on the sum, and the value depends on
// the clip's rows alone.  Four clips a workgroup; clips at window_hop > 0 overlap, so the block id
// is remapped to give each XCD (blocks b and b + 8 share one) a contiguous run of clips, whose
// shared rows then meet in one L2.
//
// select: a radix select on the bit pattern (non-negative floats order as unsigned integers), 8
// bits a pass from the top, as window_median (baselines.hip) does per channel.  select_hist_kernel
// counts, for every rank, the byte of each value whose higher bytes match the rank's prefix (LDS
// histograms, integer atomics, flushed to HBM); select_choose_kernel walks the 256 counts to the
// bucket holding the rank.  After four passes the prefix is the element.  The smallest and the
// largest value ride along as ranks 0 and n-1.
//
// classify_kernel: one thread per value, the thresholds in LDS as doubles, the class counts in LDS
// integers flushed with one 64-bit integer add per class and block.
#include "a2m_internal.h"

#include <cmath>

namespace a2m {

constexpr int VEL_WAVES = 4;  // clips of a workgroup
constexpr int SEL_R = A2M_SELECT_MAX_RANKS + 2;  // the caller's ranks, then the minimum and the maximum
constexpr int SEL_MAX_BLOCKS = 1024;
constexpr int CLS_MAX_BLOCKS = 1024;

__global__ void __launch_bounds__(64 * VEL_WAVES)
    clip_velocity_kernel(const float* __restrict__ arena, const int64_t* __restrict__ start, int64_t lo,
                         int64_t n, int C, int K, int T, int interval, int blocks_per_xcd,
                         float* __restrict__ out, int* __restrict__ n_nonfinite) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)(blockIdx.x & 7) * blocks_per_xcd + (blockIdx.x >> 3);
  const int64_t clip = blk * VEL_WAVES + wave;
  if (clip >= n) return;  // the whole wave
  const float* base = arena + start[lo + clip] * C;
  const int64_t rs = (int64_t)interval * C;  // floats from a frame to the next
  const int J = K - 1, items = (T - 1) * J;
  const int dt = 64 / J, dj = 64 % J;
  int t = lane / J, j = lane % J;  // item lane: frames (t, t + 1), joint j + 1
  double acc = 0.;
#pragma unroll 4
  for (int i = lane; i < items; i += 64) {
    const float* p = base + t * rs + (j + 1);
    const float x0 = p[0], y0 = p[K], x1 = p[rs], y1 = p[rs + K];
    const float dx = x1 - x0, dy = y1 - y0;
    acc += (double)__fsqrt_rn(dx * dx + dy * dy);
    t += dt;
    j += dj;
    if (j >= J) {
      j -= J;
      ++t;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) {
    const float v = (float)(acc / (double)items);
    out[clip] = v;
    if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) atomicAdd(n_nonfinite, 1);
  }
}

// ------------------------------------------------------------------------------------ select
struct SelRanks {
  unsigned rank[SEL_R];
  int k;   // the caller's ranks; entries k and k + 1 are 0 and n - 1
};

// ws: state [SEL_R][2] (prefix, remaining rank), then hist [4 passes][SEL_R][256]
__host__ __device__ inline size_t sel_hist_off() { return (size_t)SEL_R * 2; }

__global__ void __launch_bounds__(256) select_hist_kernel(const unsigned* __restrict__ x, int64_t n, int nr,
                                                          int pass, unsigned* __restrict__ ws) {
  __shared__ unsigned hist[SEL_R * 256];
  __shared__ unsigned prefix[SEL_R];
  const int tid = threadIdx.x;
  for (int i = tid; i < SEL_R * 256; i += 256) hist[i] = 0;
  if (tid < SEL_R) prefix[tid] = (pass > 0 && tid < nr) ? ws[2 * tid] : 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned key = x[i];
    const unsigned bin = (key >> shift) & 255u;
    const unsigned high = pass == 0 ? 0u : key >> ((shift + 8) & 31);  // prefix[] is 0 in pass 0
    for (int w = 0; w < nr; ++w)
      if (high == prefix[w]) atomicAdd(&hist[w * 256 + bin], 1u);
  }
  __syncthreads();
  unsigned* ghist = ws + sel_hist_off() + (size_t)pass * SEL_R * 256;
  for (int i = tid; i < nr * 256; i += 256)
    if (hist[i]) atomicAdd(&ghist[i], hist[i]);
}

// One thread per rank: the bucket of this pass that holds the rank.  The last pass completes the
// key, which is the element's bit pattern.
__global__ void select_choose_kernel(unsigned* __restrict__ ws, SelRanks R, int pass, float* __restrict__ out,
                                     float* __restrict__ minmax) {
  const int w = threadIdx.x;
  if (w >= R.k + 2) return;
  unsigned* state = ws + 2 * w;
  const unsigned* h = ws + sel_hist_off() + ((size_t)pass * SEL_R + w) * 256;
  unsigned rank = pass == 0 ? R.rank[w] : state[1];
  const unsigned pre = pass == 0 ? 0u : state[0];
  unsigned b = 0;
  for (; b < 255; ++b) {
    const unsigned c = h[b];
    if (rank < c) break;
    rank -= c;
  }
  const unsigned key = (pre << 8) | b;
  state[0] = key;
  state[1] = rank;
  if (pass < 3) return;
  if (w < R.k)
    out[w] = __uint_as_float(key);
  else
    minmax[w - R.k] = __uint_as_float(key);
}

// ------------------------------------------------------------------------------------ classify
struct ClsThr {
  double thr[A2M_CLASSIFY_MAX_THR];
  int n_thr, kind;
};

__global__ void __launch_bounds__(256) classify_kernel(const float* __restrict__ x, int64_t n, ClsThr P,
                                                       int* __restrict__ cls,
                                                       unsigned long long* __restrict__ counts) {
  __shared__ double thr[A2M_CLASSIFY_MAX_THR];
  __shared__ unsigned cnt[A2M_CLASSIFY_MAX_THR - 1];
  const int tid = threadIdx.x;
  const int n_cls = P.kind == A2M_CLASSIFY_BINS ? P.n_thr - 1 : 1;
  for (int i = tid; i < P.n_thr; i += 256) thr[i] = P.thr[i];
  for (int i = tid; i < n_cls; i += 256) cnt[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
    const double v = (double)x[i];
    int c = -1;
    if (P.kind == A2M_CLASSIFY_ABOVE) {
      c = v > thr[0] ? 0 : -1;
    } else if (P.kind == A2M_CLASSIFY_TAIL) {
      c = (v > thr[1] || v < thr[0]) ? 0 : -1;
    } else {
      for (int j = 0; j < n_cls; ++j)
        if (thr[j] <= v && v <= thr[j + 1]) {
          c = j;
          break;
        }
    }
    cls[i] = c;
    if (c >= 0) atomicAdd(&cnt[c], 1u);
  }
  __syncthreads();
  for (int i = tid; i < n_cls; i += 256)
    if (cnt[i]) atomicAdd(&counts[i], (unsigned long long)cnt[i]);
}

}  // namespace a2m

using namespace a2m;

extern "C" int a2m_clip_velocity_f32(const float* arena, const int64_t* start, int64_t lo, int64_t n, int32_t C,
                                     int32_t window, int32_t interval, float* out, int32_t* n_nonfinite,
                                     void* stream) {
  A2M_CHECK_ARG(n >= 0 && lo >= 0, "clip_velocity: n %lld or lo %lld negative", (long long)n, (long long)lo);
  if (n == 0) return A2M_OK;
  A2M_CHECK_ARG(arena && start && out && n_nonfinite, "clip_velocity: null argument with n > 0");
  A2M_CHECK_ARG(C >= 4 && C % 2 == 0, "clip_velocity: C %d is not an even number >= 4 (x and y of two joints)", C);
  A2M_CHECK_ARG(window > 0 && interval > 0, "clip_velocity: window %d, interval %d", window, interval);
  const int64_t T = cdiv(window, interval), K = C / 2;
  A2M_CHECK_ARG(T >= 2, "clip_velocity: window %d at interval %d is one frame: no velocity", window, interval);
  A2M_CHECK_ARG((T - 1) * (K - 1) < ((int64_t)1 << 31), "clip_velocity: (T-1)*(K-1) = %lld reaches 2^31",
                (long long)((T - 1) * (K - 1)));
  A2M_CHECK_ARG(n < ((int64_t)1 << 31), "clip_velocity: n %lld reaches 2^31", (long long)n);
  hipStream_t st = as_stream(stream);
  A2M_CHECK_HIP(hipMemsetAsync(n_nonfinite, 0, sizeof(int32_t), st));
  const int blocks_per_xcd = (int)cdiv(cdiv(n, VEL_WAVES), 8);
  hipLaunchKernelGGL(clip_velocity_kernel, dim3(8 * (unsigned)blocks_per_xcd), dim3(64 * VEL_WAVES), 0, st, arena,
                     start, lo, n, C, (int)K, (int)T, interval, blocks_per_xcd, out, n_nonfinite);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

extern "C" size_t a2m_select_f32_ws_bytes(int64_t n) {
  if (n < 0 || n >= ((int64_t)1 << 32)) return 0;
  return (sel_hist_off() + (size_t)4 * SEL_R * 256) * sizeof(unsigned);
}

extern "C" int a2m_select_f32(const float* x, int64_t n, const int64_t* ranks, int32_t k, float* out,
                              float* minmax, void* ws, size_t ws_bytes, void* stream) {
  A2M_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 32), "select: n %lld outside [0, 2^32)", (long long)n);
  if (n == 0) return A2M_OK;
  A2M_CHECK_ARG(x && ranks && out && minmax && ws, "select: null argument with n > 0");
  A2M_CHECK_ARG(k >= 1 && k <= A2M_SELECT_MAX_RANKS, "select: k %d outside 1..%d", k, A2M_SELECT_MAX_RANKS);
  SelRanks R{};
  R.k = k;
  for (int w = 0; w < k; ++w) {
    A2M_CHECK_ARG(ranks[w] >= 0 && ranks[w] < n, "select: rank %lld (entry %d) outside [0, %lld)",
                  (long long)ranks[w], w, (long long)n);
    R.rank[w] = (unsigned)ranks[w];
  }
  R.rank[k] = 0;
  R.rank[k + 1] = (unsigned)(n - 1);
  A2M_CHECK_ARG((uintptr_t)ws % 4 == 0, "select: ws must be 4-byte aligned");
  A2M_CHECK_ARG(ws_bytes >= a2m_select_f32_ws_bytes(n), "select: ws_bytes %zu < %zu", ws_bytes,
                a2m_select_f32_ws_bytes(n));
  hipStream_t st = as_stream(stream);
  unsigned* w = static_cast<unsigned*>(ws);
  A2M_CHECK_HIP(hipMemsetAsync(w, 0, a2m_select_f32_ws_bytes(n), st));
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, 256), SEL_MAX_BLOCKS);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const unsigned*>(x), n,
                       k + 2, pass, w);
    A2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(select_choose_kernel, dim3(1), dim3(64), 0, st, w, R, pass, out, minmax);
    A2M_LAUNCH_CHECK();
  }
  return A2M_OK;
}

extern "C" int a2m_classify_f32(const float* x, int64_t n, int32_t kind, const double* thr, int32_t n_thr,
                                int32_t* cls, int64_t* counts, void* stream) {
  A2M_CHECK_ARG(n >= 0, "classify: n %lld negative", (long long)n);
  A2M_CHECK_ARG(kind == A2M_CLASSIFY_ABOVE || kind == A2M_CLASSIFY_TAIL || kind == A2M_CLASSIFY_BINS,
                "classify: unknown kind %d", kind);
  if (n == 0) return A2M_OK;
  A2M_CHECK_ARG(x && thr && cls && counts, "classify: null argument with n > 0");
  if (kind == A2M_CLASSIFY_ABOVE)
    A2M_CHECK_ARG(n_thr == 1, "classify: the above kind takes 1 threshold, got %d", n_thr);
  else if (kind == A2M_CLASSIFY_TAIL)
    A2M_CHECK_ARG(n_thr == 2, "classify: the tail kind takes 2 thresholds, got %d", n_thr);
  else
    A2M_CHECK_ARG(n_thr >= 2 && n_thr <= A2M_CLASSIFY_MAX_THR, "classify: the bins kind takes 2..%d edges, got %d",
                  A2M_CLASSIFY_MAX_THR, n_thr);
  ClsThr P{};
  P.n_thr = n_thr;
  P.kind = kind;
  for (int j = 0; j < n_thr; ++j) {
    A2M_CHECK_ARG(!std::isnan(thr[j]), "classify: threshold %d is NaN", j);
    if (kind == A2M_CLASSIFY_BINS && j)
      A2M_CHECK_ARG(thr[j - 1] <= thr[j], "classify: edge %d = %g descends from %g", j, thr[j], thr[j - 1]);
    P.thr[j] = thr[j];
  }
  const int n_cls = kind == A2M_CLASSIFY_BINS ? n_thr - 1 : 1;
  hipStream_t st = as_stream(stream);
  A2M_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n_cls * sizeof(int64_t), st));
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, 256), CLS_MAX_BLOCKS);
  hipLaunchKernelGGL(classify_kernel, dim3(blocks), dim3(256), 0, st, x, n, P, cls,
                     reinterpret_cast<unsigned long long*>(counts));
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}
