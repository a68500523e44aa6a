// The per-batch kernels of the test-split evaluation (a2m.evaluation.PoseEvaluator):
//   eval_clip    de-normalises the generated pose, and per clip counts the PCK hits, sums the L1
//                difference and the speeds of both poses, and bins every speed and acceleration
//                into the clip's style's histograms
//   eval_gram    per style, for the real and for the generated frames: sum x and sum x x^T in
//                fp64 (v_mfma_f64_16x16x4_f64), the inputs of the Frechet distance
//   eval_finish  the clips' partials into the per-style accumulators
// Every floating-point sum runs in a fixed order with no atomics; the histogram counters are
// integers (atomicAdd, whose result does not depend on the order).  Nothing is read back: the
// host reads the accumulators once, at the end of the pass.
#include <algorithm>

#include "a2m_internal.h"

namespace a2m {
namespace {

constexpr int kEvalThreads = 256;
constexpr int kEvalFinishThreads = 64;  // the finish kernel is one wave
constexpr int kEvalTile = 64;           // frames per trip: one quad of lanes each
constexpr int kEvalHalo = 2;            // an acceleration at t reads pose rows t .. t + 2
constexpr size_t kEvalLds = 60 << 10;   // dynamic LDS of one workgroup (the static part rides on top)
constexpr int kEvalLoads = 8;           // loads of each pose a thread keeps in flight while a trip's rows come in
constexpr int kGramSteps = 16;          // MFMA steps (of 4 frames) per chunk of the Gram walk
constexpr int kGramDepth = 4;           // chunks whose loads are in flight ahead of the MFMAs

typedef double double4_t __attribute__((ext_vector_type(4)));

// sum over the workgroup in a fixed order (wave butterflies, then the waves ascending)
__device__ __forceinline__ double eval_block_sum(double v, double* red) {
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

__device__ __forceinline__ double eval_quad_sum(double v) {
  v += __shfl_xor(v, 1);
  return v + __shfl_xor(v, 2);
}

// bin of a value >= 0: min(floor(v / width), n_bins - 1); a NaN lands in the last bin too
__device__ __forceinline__ int eval_bin(double v, double width, int n_bins) {
  const double x = floor(v / width);
  return x < (double)(n_bins - 1) ? (int)x : n_bins - 1;
}

// One count into hist[bin] for every active lane, as one atomicAdd per distinct bin of the wave:
// the frames of a clip crowd into a few bins, and atomics on one address are served one at a time.
__device__ __forceinline__ void eval_hist_add(unsigned long long* hist, int bin) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(1);   // the active lanes
  while (todo) {                           // uniform over the wave; the leader's own bin always matches
    const int leader = __ffsll(todo) - 1;
    const int b0 = __shfl(bin, leader);
    const unsigned long long same = __ballot(bin == b0) & todo;
    if (lane == leader) atomicAdd(hist + b0, (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

// mean over the joints 1 .. K-1 of |a - b| (first difference, c = null) or |a - 2b + c|, fp64 on the
// fp32 rows [x row | y row]; lane q of a quad takes every fourth joint, the quad's sum in a fixed order
__device__ __forceinline__ double eval_motion_norm(const float* a, const float* b, const float* c, int K,
                                                   int q) {
  double s = 0.0;
  for (int k = q == 0 ? 4 : q; k < K; k += 4) {
    double dx = (double)a[k] - (double)b[k], dy = (double)a[K + k] - (double)b[K + k];
    if (c) {
      dx = (double)a[k] - 2.0 * (double)b[k] + (double)c[k];
      dy = (double)a[K + k] - 2.0 * (double)b[K + k] + (double)c[K + k];
    }
    s += sqrt(dx * dx + dy * dy);
  }
  return eval_quad_sum(s) / (double)(K - 1);
}

// One workgroup per clip, shaped like val_motion_kernel (validation.hip).  The clip's rows pass
// through two LDS rings of R = tt + 2 rows (row t in slot t % R); a trip brings in the rows it is
// the first to need -- the generated ones de-normalised on the way and written out -- and adds
// their L1 difference, one element per thread in memory order.  Then four lanes (a DPP quad) take
// each frame t of the trip: the real frame's extent and the PCK hits, the speed from rows t, t + 1
// and the acceleration from rows t .. t + 2 of both poses, binned by the quad's first lane.
// The sums stay in fp64 registers across the trips; no per-time array, so no bound on T.
__global__ __launch_bounds__(kEvalThreads) void eval_clip_kernel(
    const float* __restrict__ fake_norm, const float* __restrict__ real, const int32_t* __restrict__ style,
    const float* __restrict__ mean, const float* __restrict__ std_, int T, int K, int tt, int n_styles,
    double alpha, int n_bins, double speed_width, double accel_width, float* __restrict__ fake_px,
    double* __restrict__ part, int32_t* __restrict__ hits_out, unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) float eval_ring[];
  __shared__ double red[kEvalThreads / 64];
  const int F = 2 * K, R = tt + kEvalHalo;
  float* fk = eval_ring;
  float* rl = eval_ring + R * F;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* fp = fake_norm + (int64_t)b * T * F;
  const float* rp = real + (int64_t)b * T * F;
  float* fo = fake_px + (int64_t)b * T * F;
  const int st = style[b];
  const bool counted = st >= 0 && st < n_styles;   // uniform over the workgroup
  unsigned long long* h = hist + (int64_t)(counted ? st : 0) * 4 * n_bins;
  double l1 = 0.0, sr = 0.0, sf = 0.0, hits = 0.0;
  int loaded = 0;  // pose rows [0, loaded) have been brought in
  for (int t0 = 0; t0 < T; t0 += tt) {
    const int nr = min(tt, T - t0);                  // frames of this trip
    const int hi = min(t0 + nr + kEvalHalo, T);      // it reads pose rows [t0, hi)
    for (int i0 = loaded * F + tid; i0 < hi * F; i0 += kEvalLoads * kEvalThreads) {
      // kEvalLoads elements of each pose and their statistics in flight before any is used
      float fv[kEvalLoads], rv[kEvalLoads], sv[kEvalLoads], mv[kEvalLoads];
      int slot[kEvalLoads];
#pragma unroll
      for (int u = 0; u < kEvalLoads; ++u) {
        const int i = min(i0 + u * kEvalThreads, hi * F - 1);   // past the end: the last element again, unused
        const int t = i / F, f = i - t * F;
        slot[u] = (t % R) * F + f;
        fv[u] = fp[i];
        rv[u] = rp[i];
        sv[u] = std_[f];
        mv[u] = mean[f];
      }
#pragma unroll
      for (int u = 0; u < kEvalLoads; ++u) {
        const int i = i0 + u * kEvalThreads;
        if (i >= hi * F) break;
        const int s = slot[u];
        // two roundings, as pose_denormalize_kernel (evaluation.hip): a value that passes an empty
        // asm cannot be fused into a multiply-add
        float scaled = fv[u] * sv[u];
        asm volatile("" : "+v"(scaled));
        const float px = scaled + mv[u];
        fo[i] = px;
        fk[s] = px;
        rl[s] = rv[u];
        l1 += fabs((double)px - (double)rv[u]);
      }
    }
    loaded = hi;
    __syncthreads();
    const int tl = tid >> 2, q = tid & 3, t = t0 + tl;
    if (counted && tl < nr) {                        // uniform over a quad
      const float* r0 = rl + (t % R) * F;
      const float* f0 = fk + (t % R) * F;
      float xmax = -INFINITY, xmin = INFINITY, ymax = -INFINITY, ymin = INFINITY;
      for (int k = q; k < K; k += 4) {
        xmax = fmaxf(xmax, r0[k]); xmin = fminf(xmin, r0[k]);
        ymax = fmaxf(ymax, r0[K + k]); ymin = fminf(ymin, r0[K + k]);
      }
      xmax = quad_max(xmax); xmin = -quad_max(-xmin);
      ymax = quad_max(ymax); ymin = -quad_max(-ymin);
      // as pck_kernel (evaluation.hip)
      const double ext = fmax(fabs((double)xmax - (double)xmin), fabs((double)ymax - (double)ymin));
      const double radius = ext * alpha;
      for (int k = q; k < K; k += 4) {
        const double dx = (double)r0[k] - (double)f0[k], dy = (double)r0[K + k] - (double)f0[K + k];
        hits += sqrt(dx * dx + dy * dy) <= radius ? 1.0 : 0.0;
      }
      if (t + 1 < T) {
        const float* r1 = rl + ((t + 1) % R) * F;
        const float* f1 = fk + ((t + 1) % R) * F;
        const double vr = eval_motion_norm(r1, r0, nullptr, K, q);
        const double vf = eval_motion_norm(f1, f0, nullptr, K, q);
        if (q == 0) {
          sr += vr;
          sf += vf;
          eval_hist_add(h, eval_bin(vr, speed_width, n_bins));
          eval_hist_add(h + n_bins, eval_bin(vf, speed_width, n_bins));
        }
        if (t + 2 < T) {
          const float* r2 = rl + ((t + 2) % R) * F;
          const float* f2 = fk + ((t + 2) % R) * F;
          const double ar = eval_motion_norm(r2, r1, r0, K, q);
          const double af = eval_motion_norm(f2, f1, f0, K, q);
          if (q == 0) {
            eval_hist_add(h + 2 * n_bins, eval_bin(ar, accel_width, n_bins));
            eval_hist_add(h + 3 * n_bins, eval_bin(af, accel_width, n_bins));
          }
        }
      }
    }
    __syncthreads();  // the next trip's rows overwrite slots this one has read
  }
  l1 = eval_block_sum(l1, red);
  sr = eval_block_sum(sr, red);
  sf = eval_block_sum(sf, red);
  hits = eval_block_sum(hits, red);   // a sum of ones below 2^31: exact in fp64 in any order
  if (tid == 0) {
    part[3 * b] = l1;
    part[3 * b + 1] = sr;
    part[3 * b + 2] = sf;
    hits_out[b] = (int32_t)hits;
  }
}

// One wave per (16 x 16 tile of the upper triangle, real | generated, style): the tile's only
// owner.  It walks the batch's clips in ascending order, skips those of other styles, and takes a
// clip's frames in ascending steps of 4 through v_mfma_f64_16x16x4_f64 with A = X^T, B = X: lane l
// holds A[i = l & 15][k = l >> 4] = x[t0 + (l >> 4)][16 ti + (l & 15)] and B[k][j] likewise from
// tile column tj, zero beyond F and beyond T.  The result sits at col = l & 15, row = (l >> 4) + 4 reg
// (the f64 map, not the f32 one) and is added to the global accumulator with plain loads and stores.
// The diagonal tiles' owners also sum their 16 features (sum x): per lane over the steps, then
// over the four frame lanes of a feature in a fixed order.
__global__ __launch_bounds__(64) void eval_gram_kernel(const float* __restrict__ fake_px,
                                                       const float* __restrict__ real_px,
                                                       const int32_t* __restrict__ style, int B, int T, int F,
                                                       double* __restrict__ sx, double* __restrict__ gram) {
  const int which = blockIdx.y, st = blockIdx.z, lane = threadIdx.x;
  const int nt = (F + 15) >> 4;
  int ti = 0, rest = blockIdx.x;       // tile blockIdx.x of the upper triangle, row by row
  while (rest >= nt - ti) { rest -= nt - ti; ++ti; }
  const int tj = ti + rest;
  const int k = lane >> 4, fa = 16 * ti + (lane & 15), fb = 16 * tj + (lane & 15);
  const bool ina = fa < F, inb = fb < F;
  const int fac = min(fa, F - 1), fbc = min(fb, F - 1);
  const unsigned ka = ina ? ~0u : 0u, kb = inb ? ~0u : 0u;
  const float* x = which ? fake_px : real_px;
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  double s = 0.0;
  // The walk is one chain of dependent MFMAs fed by loads, so what it costs is latency: a chunk
  // (kGramSteps steps of one clip) is loaded whole, and the loads of the next kGramDepth - 1 chunks
  // are in flight before this chunk's MFMAs.  The wave finds its clips 64 at a time with a ballot
  // over their styles.
  int bg = -64, cb = -1, ct0 = 0;      // the clip group being scanned, the current chunk's clip and first frame
  unsigned long long own = 0;          // clips of this style still to come in the group
  auto advance = [&]() -> bool {
    if (cb >= 0 && ct0 + 4 * kGramSteps < T) {
      ct0 += 4 * kGramSteps;
      return true;
    }
    while (!own) {
      bg += 64;
      if (bg >= B) return false;
      const int sb = bg + lane < B ? style[bg + lane] : -1;   // st >= 0: -1 is nobody's
      own = __ballot(sb == st);
    }
    cb = bg + __ffsll(own) - 1;
    own &= own - 1;
    ct0 = 0;
    return true;
  };
  auto load = [&](float (&a)[kGramSteps], float (&bb)[kGramSteps]) {
    const float* xc = x + (int64_t)cb * T * F;
#pragma unroll
    for (int u = 0; u < kGramSteps; ++u) {   // a step beyond T adds zeros
      // every lane loads from a clamped, valid address, and the bits are masked only where the
      // MFMA takes them: a load under a branch, or masked at once, is waited for before the next
      // is issued
      const int row = min(ct0 + 4 * u + k, T - 1) * F;
      a[u] = xc[row + fac];
      bb[u] = xc[row + fbc];
    }
  };
  // a ring of kGramDepth chunks, filled in ascending order and consumed in the same order
  float ra[kGramDepth][kGramSteps], rb[kGramDepth][kGramSteps];
  bool have[kGramDepth];
  int rt0[kGramDepth];                 // each chunk's first frame
#pragma unroll
  for (int d = 0; d < kGramDepth; ++d) {
    have[d] = advance();
    rt0[d] = ct0;
    if (have[d]) load(ra[d], rb[d]);
  }
  const bool any = have[0];
  for (bool more = any; more;) {
#pragma unroll
    for (int d = 0; d < kGramDepth; ++d) {
      if (!have[d]) {                  // the chunks are handed out in order: none after this one either
        more = false;
        break;
      }
#pragma unroll
      for (int u = 0; u < kGramSteps; ++u) {
        const unsigned keep = rt0[d] + 4 * u + k < T ? ~0u : 0u;
        const double a = (double)__uint_as_float(__float_as_uint(ra[d][u]) & (keep & ka));
        const double bb = (double)__uint_as_float(__float_as_uint(rb[d][u]) & (keep & kb));
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc, 0, 0, 0);
        s += a;
      }
      have[d] = advance();
      rt0[d] = ct0;
      if (have[d]) load(ra[d], rb[d]);
    }
  }
  if (!any) return;                    // no clip of this style in the batch: nothing to add
  double* g = gram + ((int64_t)st * 2 + which) * F * F;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * ti + k + 4 * r;
    if (row < F && inb) g[(int64_t)row * F + fb] += acc[r];
  }
  if (ti == tj) {
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (lane < 16 && ina) sx[((int64_t)st * 2 + which) * F + fa] += s;
  }
}

// One workgroup of one wave, as val_finish_kernel: per style, each lane a strided share of the
// clips in ascending order, then the butterfly -- the same order every run.
__global__ __launch_bounds__(kEvalFinishThreads) void eval_finish_kernel(
    const double* __restrict__ part, const int32_t* __restrict__ hits, const int32_t* __restrict__ style, int B,
    int T, int n_styles, long long* __restrict__ counts, double* __restrict__ sums) {
  const int tid = threadIdx.x;
  long long dropped = 0;
  for (int b = tid; b < B; b += kEvalFinishThreads) dropped += style[b] < 0 || style[b] >= n_styles;
  for (int o = 32; o > 0; o >>= 1) dropped += __shfl_xor(dropped, o);
  if (tid == 0) counts[3 * n_styles] += dropped;
  for (int st = 0; st < n_styles; ++st) {
    double l1 = 0.0, sr = 0.0, sf = 0.0;
    long long nc = 0, nh = 0;
    for (int b = tid; b < B; b += kEvalFinishThreads) {
      if (style[b] != st) continue;
      l1 += part[3 * b];
      sr += part[3 * b + 1];
      sf += part[3 * b + 2];
      nc += 1;
      nh += hits[b];
    }
    for (int o = 32; o > 0; o >>= 1) {
      l1 += __shfl_xor(l1, o);
      sr += __shfl_xor(sr, o);
      sf += __shfl_xor(sf, o);
      nc += __shfl_xor(nc, o);
      nh += __shfl_xor(nh, o);
    }
    if (tid == 0 && nc) {
      counts[3 * st] += nc;
      counts[3 * st + 1] += nc * T;
      counts[3 * st + 2] += nh;
      sums[3 * st] += l1;
      sums[3 * st + 1] += sr;
      sums[3 * st + 2] += sf;
    }
  }
}

}  // namespace
}  // namespace a2m

using namespace a2m;

extern "C" {

int a2m_eval_clip_f32(const float* fake_norm, const float* real_px, const int32_t* style, const float* mean,
                      const float* std_, int32_t B, int32_t T, int32_t F, int32_t n_styles, double alpha,
                      int32_t n_bins, double speed_width, double accel_width, float* fake_px, double* part,
                      int32_t* hits, int64_t* hist, void* stream) {
  A2M_CHECK_ARG(fake_norm && real_px && style && mean && std_ && fake_px && part && hits && hist && B > 0 &&
                    T >= 1 && F >= 4 && F % 2 == 0 && n_styles > 0 && n_bins > 0 && speed_width > 0.0 &&
                    accel_width > 0.0,
                "eval_clip: bad args");
  // both rings hold tt + 2 rows of F floats; the kernel indexes one clip with 32-bit ints
  const int64_t rows = (int64_t)(kEvalLds / (2 * sizeof(float))) / F;
  A2M_CHECK_ARG(rows > kEvalHalo && (int64_t)T * F <= INT32_MAX - kEvalLoads * kEvalThreads,
                "eval_clip: F = %d, T = %d beyond the kernel's limits (F <= 2560, T * F < 2^31)", F, T);
  const int tt = (int)std::min<int64_t>(kEvalTile, rows - kEvalHalo);
  const size_t lds = 2 * sizeof(float) * (size_t)(tt + kEvalHalo) * F;
  hipLaunchKernelGGL(eval_clip_kernel, dim3(B), dim3(kEvalThreads), lds, as_stream(stream), fake_norm, real_px,
                     style, mean, std_, T, F / 2, tt, n_styles, alpha, n_bins, speed_width, accel_width, fake_px,
                     part, hits, reinterpret_cast<unsigned long long*>(hist));
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_eval_gram_f64(const float* fake_px, const float* real_px, const int32_t* style, int32_t B, int32_t T,
                      int32_t F, int32_t n_styles, double* sx, double* gram, void* stream) {
  A2M_CHECK_ARG(fake_px && real_px && style && sx && gram && B > 0 && T >= 1 && F > 0 && n_styles > 0,
                "eval_gram: bad args");
  const int64_t nt = cdiv(F, 16);
  // the kernel indexes one clip with 32-bit ints and looks up to a chunk past T before masking
  A2M_CHECK_ARG(((int64_t)T + 4 * kGramSteps) * F <= INT32_MAX && nt * (nt + 1) / 2 <= INT32_MAX && n_styles <= 65535,
                "eval_gram: T = %d, F = %d, n_styles = %d beyond the kernel's limits ((T + 64) * F < 2^31, "
                "n_styles < 65536)",
                T, F, n_styles);
  hipLaunchKernelGGL(eval_gram_kernel, dim3((unsigned)(nt * (nt + 1) / 2), 2, (unsigned)n_styles), dim3(64), 0,
                     as_stream(stream), fake_px, real_px, style, B, T, F, sx, gram);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_eval_finish_f64(const double* part, const int32_t* hits, const int32_t* style, int32_t B, int32_t T,
                        int32_t n_styles, int64_t* counts, double* sums, void* stream) {
  A2M_CHECK_ARG(part && hits && style && counts && sums && B > 0 && T >= 1 && n_styles > 0,
                "eval_finish: bad args");
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(kEvalFinishThreads), 0, as_stream(stream), part, hits,
                     style, B, T, n_styles, reinterpret_cast<long long*>(counts), sums);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

}  // extern "C"
