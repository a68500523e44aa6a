// The per-batch kernels of the test-split evaluation (a2m.evaluation.PoseEvaluator):
//   eval_clip    de-normalises the generated pose, and per clip counts the PCK hits, sums the L1
//                difference and the speeds of both poses, and bins every speed and acceleration
//                into the clip's style's histograms
//   eval_gram    per style, for the real and for the generated frames: sum x and sum x x^T in
//                fp64 (v_mfma_f64_16x16x4_f64), the inputs of the Frechet distance
//   eval_finish  the clips' partials into the per-style accumulators
// and the two of the opt-in audio-motion synchrony metrics (a2m.evaluation.AudioSyncEvaluator):
//   eval_sync         per clip the onset strength of the audio and the speeds of both poses, their
//                     beats, the beat distance histograms and the lagged sums of (onset, speed)
//   eval_sync_finish  the clips' lagged sums into the per-style accumulators
// Every floating-point sum runs in a fixed order with no atomics; the histogram counters are
// integers (atomicAdd, whose result does not depend on the order).  Nothing is read back: the
// host reads the accumulators once, at the end of the pass.
#include <algorithm>
#include <cfloat>

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

constexpr int kSyncThreads = 256;
constexpr int kSyncCols = 4;            // audio columns a lane carries in registers: C <= 256 is read once
// 25 B of dynamic LDS a frame (onset and two speeds as doubles, a flag byte): 51,200 B at 2048, on top of
// 32 B static, under the 64 KB a workgroup gets without asking for more
constexpr int kSyncMaxT = 2048;
constexpr int kSyncMaxLags = 16;
constexpr int kSyncFinishLoads = 8;     // clips whose partials the finish kernel keeps in flight

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

__device__ __forceinline__ double eval_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// distance from frame t to the nearest frame whose flags hold `bit`, n_dist - 1 (the catch-all bin)
// where there is none closer
__device__ __forceinline__ int sync_nearest(const unsigned char* flags, int t, int T, int bit, int n_dist) {
  for (int d = 0; d < n_dist - 1; ++d) {
    const int lo = t - d, hi = t + d;
    if ((lo >= 0 && (flags[lo] & bit)) || (hi < T && (flags[hi] & bit))) return d;
  }
  return n_dist - 1;
}

// One workgroup per clip.  Its three series sit in LDS as doubles: the onset strength o (each wave
// a contiguous run of frames, lanes over the audio columns, the previous row carried in registers,
// the column sum a butterfly) and the speeds of both poses (a quad per frame, eval_clip's
// eval_motion_norm).  Then a thread per frame: the beat flags (bit 0 audio, 1 real motion, 2
// generated motion), and from every beat an outward scan for the nearest beat of the other kind.
// The lagged sums take a wave per lag, lanes striding t ascending, then the butterfly.  Every
// floating-point sum has a fixed order; the histogram and beat counters are integers.
__global__ __launch_bounds__(kSyncThreads) void eval_sync_kernel(
    const float* __restrict__ audio, const float* __restrict__ fake_px, const float* __restrict__ real_px,
    const int32_t* __restrict__ style, const float* __restrict__ audio_std, int T, int C, int K, int n_styles,
    int n_lags, int n_dist, double onset_delta, unsigned long long* __restrict__ beat_dist,
    unsigned long long* __restrict__ beat_counts, double* __restrict__ part, double* __restrict__ onset_out,
    double* __restrict__ speed_out) {
  extern __shared__ __attribute__((aligned(16))) double sync_lds[];
  __shared__ double red[kSyncThreads / 64];
  double* o = sync_lds;
  double* sr = o + T;
  double* sf = sr + T;
  unsigned char* flags = reinterpret_cast<unsigned char*>(sf + T);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, F = 2 * K;
  const float* ap = audio + (int64_t)b * T * C;
  const float* rp = real_px + (int64_t)b * T * F;
  const float* fp = fake_px + (int64_t)b * T * F;
  {
    const int per = (T - 1 + kSyncThreads / 64 - 1) / (kSyncThreads / 64);
    const int lo = 1 + w * per, hi = min(lo + per, T);    // this wave's frames [lo, hi)
    int col[kSyncCols];
    double sg[kSyncCols];                                 // 0 beyond C: that column adds nothing
    float prev[kSyncCols], cur[kSyncCols], next[kSyncCols];
#pragma unroll
    for (int j = 0; j < kSyncCols; ++j) {
      col[j] = min(lane + 64 * j, C - 1);
      sg[j] = lane + 64 * j < C ? (audio_std ? (double)audio_std[col[j]] : 1.0) : 0.0;
      prev[j] = lo < hi ? ap[(lo - 1) * C + col[j]] : 0.f;
      cur[j] = lo < hi ? ap[lo * C + col[j]] : 0.f;
    }
    for (int t = lo; t < hi; ++t) {
      double p = 0.0;
#pragma unroll
      for (int j = 0; j < kSyncCols; ++j) {   // the next row is in flight while this one is summed
        next[j] = ap[min(t + 1, hi - 1) * C + col[j]];
        p += fmax(0.0, ((double)cur[j] - (double)prev[j]) * sg[j]);
        prev[j] = cur[j];
        cur[j] = next[j];
      }
      for (int c = lane + 64 * kSyncCols; c < C; c += 64)   // wider than the registers: both rows from memory
        p += fmax(0.0, ((double)ap[t * C + c] - (double)ap[(t - 1) * C + c]) * (audio_std ? (double)audio_std[c] : 1.0));
      p = eval_wave_sum(p);
      if (lane == 0) o[t] = p / (double)C;
    }
  }
  if (tid == 0) o[0] = sr[0] = sf[0] = 0.0;
  for (int t = 1 + (tid >> 2); t < T; t += kSyncThreads / 4) {   // uniform over a quad
    const double vr = eval_motion_norm(rp + t * F, rp + (t - 1) * F, nullptr, K, tid & 3);
    const double vf = eval_motion_norm(fp + t * F, fp + (t - 1) * F, nullptr, K, tid & 3);
    if ((tid & 3) == 0) {
      sr[t] = vr;
      sf[t] = vf;
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += kSyncThreads) {
    if (onset_out) onset_out[(int64_t)b * T + t] = o[t];
    if (speed_out) {
      speed_out[(int64_t)(2 * b) * T + t] = sr[t];
      speed_out[(int64_t)(2 * b + 1) * T + t] = sf[t];
    }
  }
  const int st = style[b];
  if (st < 0 || st >= n_styles) return;                   // uniform over the workgroup
  double m = 0.0;
  for (int t = 1 + tid; t < T; t += kSyncThreads) m += o[t];
  m = eval_block_sum(m, red);
  const double thr = T > 1 ? onset_delta * (m / (double)(T - 1)) : 0.0;
  int na = 0, nr = 0, nf = 0;                             // this wave's beats
  for (int t0 = 0; t0 < T; t0 += kSyncThreads) {          // whole trips: the ballots want every lane
    const int t = t0 + tid;
    int bits = 0;
    if (t >= 2 && t <= T - 2) {
      bits = (o[t] > o[t - 1] && o[t] >= o[t + 1] && o[t] > thr ? 1 : 0) |
             (sr[t] < sr[t - 1] && sr[t] <= sr[t + 1] ? 2 : 0) | (sf[t] < sf[t - 1] && sf[t] <= sf[t + 1] ? 4 : 0);
    }
    if (t < T) flags[t] = (unsigned char)bits;
    na += __popcll(__ballot(bits & 1));
    nr += __popcll(__ballot(bits & 2));
    nf += __popcll(__ballot(bits & 4));
  }
  if (lane == 0) {
    if (na) atomicAdd(beat_counts + 3 * st, (unsigned long long)na);
    if (nr) atomicAdd(beat_counts + 3 * st + 1, (unsigned long long)nr);
    if (nf) atomicAdd(beat_counts + 3 * st + 2, (unsigned long long)nf);
  }
  __syncthreads();
  unsigned long long* h = beat_dist + (int64_t)st * 4 * n_dist;   // [real | generated][motion->audio | audio->motion]
  for (int t = 2 + tid; t <= T - 2; t += kSyncThreads) {
    const int bits = flags[t];
    if (bits & 2) eval_hist_add(h, sync_nearest(flags, t, T, 1, n_dist));
    if (bits & 1) eval_hist_add(h + n_dist, sync_nearest(flags, t, T, 2, n_dist));
    if (bits & 4) eval_hist_add(h + 2 * n_dist, sync_nearest(flags, t, T, 1, n_dist));
    if (bits & 1) eval_hist_add(h + 3 * n_dist, sync_nearest(flags, t, T, 4, n_dist));
  }
  const int L = 2 * n_lags + 1;
  for (int li = w; li < L; li += kSyncThreads / 64) {     // a wave owns a lag: no workgroup barrier per sum
    const int l = li - n_lags;
    const int hi = min(T - 1, T - 1 - l);                 // the pairs (o[t], s[t + l]), max(1, 1 - l) <= t <= hi
    double so = 0.0, soo = 0.0, s1 = 0.0, s11 = 0.0, so1 = 0.0, s2 = 0.0, s22 = 0.0, so2 = 0.0;
    for (int t = max(1, 1 - l) + lane; t <= hi; t += 64) {
      const double x = o[t], yr = sr[t + l], yf = sf[t + l];
      so += x;
      soo += x * x;
      s1 += yr;
      s11 += yr * yr;
      so1 += x * yr;
      s2 += yf;
      s22 += yf * yf;
      so2 += x * yf;
    }
    so = eval_wave_sum(so);
    soo = eval_wave_sum(soo);
    s1 = eval_wave_sum(s1);
    s11 = eval_wave_sum(s11);
    so1 = eval_wave_sum(so1);
    s2 = eval_wave_sum(s2);
    s22 = eval_wave_sum(s22);
    so2 = eval_wave_sum(so2);
    if (lane == 0) {
      double* p = part + ((int64_t)b * L + li) * 8;
      p[0] = so;
      p[1] = soo;
      p[2] = s1;
      p[3] = s11;
      p[4] = so1;
      p[5] = s2;
      p[6] = s22;
      p[7] = so2;
    }
  }
}

// One wave, as eval_finish_kernel.  Per style a lane owns an element of [2 n_lags + 1][8] and adds
// the clips' partials to it in ascending clip order; lag_n gets the pair count of each lag by its
// formula.  Every clip's row of part is loaded, so that the loads do not wait for the style test, and
// a clip of another style adds 0 by a select.  That reads, on purpose, the rows of dropped clips,
// which eval_sync_kernel never wrote: whatever bits they hold (a NaN too) are discarded unused.
__global__ __launch_bounds__(kEvalFinishThreads) void eval_sync_finish_kernel(
    const double* __restrict__ part, const int32_t* __restrict__ style, int B, int T, int n_styles, int n_lags,
    double* __restrict__ lag_sums, long long* __restrict__ lag_n) {
  const int lane = threadIdx.x, L = 2 * n_lags + 1, E = 8 * L;
  for (int st = 0; st < n_styles; ++st) {
    long long nc = 0;
    for (int b = lane; b < B; b += kEvalFinishThreads) nc += style[b] == st;
    for (int o = 32; o > 0; o >>= 1) nc += __shfl_xor(nc, o);
    if (!nc) continue;                                    // uniform: no clip of this style in the batch
    for (int e0 = 0; e0 < E; e0 += kEvalFinishThreads) {
      const int e = min(e0 + lane, E - 1);
      double acc = 0.0;
      for (int b0 = 0; b0 < B; b0 += kSyncFinishLoads) {
        double v[kSyncFinishLoads];
#pragma unroll
        for (int u = 0; u < kSyncFinishLoads; ++u) v[u] = part[(int64_t)min(b0 + u, B - 1) * E + e];
#pragma unroll
        for (int u = 0; u < kSyncFinishLoads; ++u) acc += b0 + u < B && style[b0 + u] == st ? v[u] : 0.0;
      }
      if (e0 + lane < E) lag_sums[(int64_t)st * E + e] += acc;
    }
    if (lane < L) lag_n[(int64_t)st * L + lane] += nc * max(T - 1 - abs(lane - n_lags), 0);
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

int a2m_eval_sync_f64(const float* audio, const float* fake_px, const float* real_px, const int32_t* style,
                      const float* audio_std, int32_t B, int32_t T, int32_t C, int32_t F, int32_t n_styles,
                      int32_t n_lags, int32_t n_dist, double onset_delta, int64_t* beat_dist, int64_t* beat_counts,
                      double* part, double* onset_out, double* speed_out, void* stream) {
  A2M_CHECK_ARG(audio && fake_px && real_px && style && beat_dist && beat_counts && part && B > 0 && T >= 1 &&
                    C > 0 && F >= 4 && F % 2 == 0 && n_styles > 0 && n_dist >= 2 && n_lags >= 0 &&
                    n_lags <= kSyncMaxLags && onset_delta >= 0.0 && onset_delta <= DBL_MAX,
                "eval_sync: bad args");
  // the three series of a clip sit in LDS; the kernel indexes one clip with 32-bit ints
  A2M_CHECK_ARG(T <= kSyncMaxT && (int64_t)T * C <= INT32_MAX && (int64_t)T * F <= INT32_MAX,
                "eval_sync: T = %d, C = %d, F = %d beyond the kernel's limits (T <= 2048, T * C and T * F < 2^31)", T, C,
                F);
  const size_t lds = (3 * sizeof(double) + 1) * (size_t)T;
  hipLaunchKernelGGL(eval_sync_kernel, dim3(B), dim3(kSyncThreads), lds, as_stream(stream), audio, fake_px, real_px,
                     style, audio_std, T, C, F / 2, n_styles, n_lags, n_dist, onset_delta,
                     reinterpret_cast<unsigned long long*>(beat_dist),
                     reinterpret_cast<unsigned long long*>(beat_counts), part, onset_out, speed_out);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_eval_sync_finish_f64(const double* part, const int32_t* style, int32_t B, int32_t T, int32_t n_styles,
                             int32_t n_lags, double* lag_sums, int64_t* lag_n, void* stream) {
  A2M_CHECK_ARG(part && style && lag_sums && lag_n && B > 0 && T >= 1 && n_styles > 0 && n_lags >= 0 &&
                    n_lags <= kSyncMaxLags,
                "eval_sync_finish: bad args");
  hipLaunchKernelGGL(eval_sync_finish_kernel, dim3(1), dim3(kEvalFinishThreads), 0, as_stream(stream), part, style,
                     B, T, n_styles, n_lags, lag_sums, reinterpret_cast<long long*>(lag_n));
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

}  // extern "C"
