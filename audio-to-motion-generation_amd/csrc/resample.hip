// Waveform resampling: band-limited interpolation with a Kaiser-windowed sinc (what
// librosa.core.resample did through resampy at pats/data_loading/audio.py:88, with resampy's
// published filter parameters; the continuous filter is evaluated exactly, not through
// resampy's 512-per-crossing table).
//
//   g = gcd(sr_in, sr_out), P = sr_in / g, Q = sr_out / g, M = max(P, Q), s = Q / M, L = ceil(Z M / Q)
//   output t sits at input position t P / Q:  n_t = (t P) div Q,  p_t = (t P) mod Q   (int64)
//   y[t]   = sum_{k = -L+1 .. L} h_{p_t}[k] x[n_t + k]            x = 0 outside [0, n)
//   h_p[k] = s rho sinc(s rho tau) w(s tau / Z),  tau = (p - k Q) / Q
//   w(u)   = I0(beta sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0
//
// Plan: the taps, built on the host in float64 and stored as float32, TAP-major and indexed by
// t mod Q: bankT[j][r] = h_{(r P) mod Q}[j - L + 1].  Consecutive outputs use phases that step by
// P mod Q, so a phase-major bank would scatter a wave's tap loads over rows; in this layout the
// lanes of a wave (consecutive t, so consecutive r, wrapping at Q) read one contiguous run per tap.
//
// Kernel: a 256-thread workgroup owns RS_TILE consecutive outputs of one clip.  It stages the
// tile's input span (tile P / Q + 2 L samples, zero-filled outside the clip) into LDS with
// coalesced loads, then each thread accumulates RS_OPT outputs (t, t + 256, ...) in fp32: per tap
// one coalesced tap load (the bank is small and stays cache-resident) and one LDS read per output.
// A ratio so steep that the span does not fit LDS takes the unstaged form of the same loop: one
// output per thread, samples read from global memory under the same bounds test.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "a2m_internal.h"

namespace a2m {

constexpr int RS_THREADS = 256;
constexpr int RS_OPT = 4;                      // outputs per thread of the staged kernel
constexpr int RS_TILE = RS_THREADS * RS_OPT;   // outputs per workgroup
constexpr int64_t RS_MAX_SPAN = 16384;         // floats of LDS (64 KB) a staged tile may take
constexpr int64_t RS_MAX_BANK = 1 << 21;       // floats: a larger bank is refused at plan time

struct ResampleHeader {
  int32_t sr_in, sr_out, num_zeros, P, Q, L;
  int32_t off_bank;  // byte offset of bankT[2L][Q]
  int32_t pad;
  double beta, rolloff;
};

static size_t rs_align16(size_t x) { return (x + 15) & ~size_t(15); }

struct Ratio {
  int64_t P, Q, M, L;
};

static int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

static int resample_ratio(int32_t sr_in, int32_t sr_out, int32_t num_zeros, Ratio* r) {
  A2M_CHECK_ARG(sr_in >= 1 && sr_out >= 1, "resample: rates %d -> %d must be positive", sr_in, sr_out);
  A2M_CHECK_ARG(num_zeros >= 1, "resample: num_zeros %d must be at least 1", num_zeros);
  const int64_t g = gcd64(sr_in, sr_out);
  r->P = sr_in / g;
  r->Q = sr_out / g;
  r->M = std::max(r->P, r->Q);
  r->L = ((int64_t)num_zeros * r->M + r->Q - 1) / r->Q;  // ceil(Z / s), < 2^62
  A2M_CHECK_ARG(2 * r->L <= RS_MAX_BANK / r->Q,
                "resample: %d -> %d reduces to P/Q = %lld/%lld, a bank of %lld phases x %lld taps: more "
                "than %lld floats",
                sr_in, sr_out, (long long)r->P, (long long)r->Q, (long long)r->Q, (long long)(2 * r->L),
                (long long)RS_MAX_BANK);
  return A2M_OK;
}

// I0 by its power series sum_k ((x/2)^k / k!)^2: all terms positive, so no cancellation
static double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// h_p[k] from the integer numerator num = p - k Q of tau: the arguments reduce to
// s rho tau = rho num / M and s tau / Z = num / (Z M), and |u| < 1 to |num| < Z M exactly
static double tap(int64_t num, const Ratio& r, int num_zeros, double beta, double rolloff, double i0_beta) {
  const int64_t zm = (int64_t)num_zeros * r.M;
  if (num <= -zm || num >= zm) return 0.0;
  const double pi = 3.14159265358979323846;
  const double u = (double)num / (double)zm;
  const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0_beta;
  const double v = rolloff * (double)num / (double)r.M;
  const double sinc = v == 0.0 ? 1.0 : std::sin(pi * v) / (pi * v);
  return ((double)r.Q / (double)r.M) * rolloff * sinc * w;
}

static int resample_plan(int32_t sr_in, int32_t sr_out, int32_t num_zeros, double beta, double rolloff,
                         void* host, size_t bytes, size_t* need) {
  Ratio r;
  const int rc = resample_ratio(sr_in, sr_out, num_zeros, &r);
  if (rc) return rc;
  A2M_CHECK_ARG(rolloff > 0.0 && rolloff <= 1.0, "resample: rolloff %g must be in (0, 1]", rolloff);
  A2M_CHECK_ARG(beta >= 0.0, "resample: beta %g must not be negative", beta);  // false for NaN too
  ResampleHeader h{};
  h.sr_in = sr_in; h.sr_out = sr_out; h.num_zeros = num_zeros;
  h.P = (int32_t)r.P; h.Q = (int32_t)r.Q; h.L = (int32_t)r.L;
  h.off_bank = (int32_t)rs_align16(sizeof(ResampleHeader));
  h.beta = beta; h.rolloff = rolloff;
  const size_t taps = (size_t)(2 * r.L * r.Q);
  *need = h.off_bank + sizeof(float) * taps;
  if (host == nullptr) return A2M_OK;
  if (bytes < *need) { set_error("resample plan buffer too small (%zu < %zu)", bytes, *need); return A2M_EWS; }
  unsigned char* p = static_cast<unsigned char*>(host);
  std::memset(p, 0, h.off_bank);
  std::memcpy(p, &h, sizeof(h));
  float* bankT = reinterpret_cast<float*>(p + h.off_bank);
  const double i0_beta = bessel_i0(beta);
  for (int64_t rr = 0; rr < r.Q; ++rr) {
    const int64_t phase = rr * r.P % r.Q;
    for (int64_t j = 0; j < 2 * r.L; ++j) {
      const int64_t k = j - r.L + 1;
      bankT[j * r.Q + rr] = (float)tap(phase - k * r.Q, r, num_zeros, beta, rolloff, i0_beta);
    }
  }
  return A2M_OK;
}

// ------------------------------------------------------------------------------ device
// Where a sample comes from.  Both fetches return x[g] for the global sample index g of one
// signal and 0 where the signal is defined to be zero; everything downstream of the fetch (the
// staging, the tap loop, the fmaf chain) is resample_tile, shared by the offline and the
// streaming kernel, so the two agree bit for bit.
struct ClipFetch {   // a whole clip: x = 0 outside [0, n)
  const float* __restrict__ clip;
  int64_t n;
  __device__ __forceinline__ float operator()(int64_t g) const { return g >= 0 && g < n ? clip[g] : 0.f; }
};
struct SlideFetch {  // a sliding buffer holding [base, base + len): x = 0 outside [lo, hi), which the
  const float* __restrict__ buf;  // host has clipped to the buffer (a2m_resample_stream_f32)
  int64_t base, lo, hi;
  __device__ __forceinline__ float operator()(int64_t g) const { return g >= lo && g < hi ? buf[g - base] : 0.f; }
};

// Outputs [t0, min(t0 + OPT * RS_THREADS, t_end)) of one signal, written to dst[t - t_org].
// STAGED: xs holds samples [lo, lo + count) of the signal, count <= span_cap (the host sizes
// span_cap from the same arithmetic, so the clamp never bites; it keeps LDS writes in bounds
// whatever the caller passed).
template <int OPT, bool STAGED, class Fetch>
__device__ __forceinline__ void resample_tile(const Fetch& fetch, const float* __restrict__ bankT, int P,
                                              int Q, int L, float* __restrict__ dst, int64_t t0,
                                              int64_t t_end, int64_t t_org, int span_cap, float* xs) {
  int64_t lo = 0;
  if (STAGED) {
    const int64_t t_last = (t0 + OPT * RS_THREADS < t_end ? t0 + OPT * RS_THREADS : t_end) - 1;
    lo = t0 * P / Q - L + 1;
    const int64_t span = t_last * P / Q + L - lo + 1;
    const int count = (int)(span < span_cap ? span : span_cap);
#pragma unroll 4
    for (int i = threadIdx.x; i < count; i += RS_THREADS) xs[i] = fetch(lo + i);
    __syncthreads();
  }
  float acc[OPT];
  int64_t first[OPT];  // signal index of the output's tap 0 (k = -L + 1)
  int off[OPT], row[OPT];
  bool live[OPT];
#pragma unroll
  for (int i = 0; i < OPT; ++i) {
    const int64_t t = t0 + threadIdx.x + i * RS_THREADS;
    live[i] = t < t_end;
    const int64_t tt = live[i] ? t : t0;  // a thread past the end repeats the tile's first output
    first[i] = tt * P / Q - L + 1;
    off[i] = (int)(first[i] - lo);
    row[i] = (int)(tt % Q);
    acc[i] = 0.f;
  }
  const int taps = 2 * L;
#pragma unroll 4
  for (int j = 0; j < taps; ++j) {
    const float* hj = bankT + j * Q;  // 2 L Q <= RS_MAX_BANK
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
      const float x = STAGED ? xs[off[i] + j] : fetch(first[i] + j);
      acc[i] = fmaf(hj[row[i]], x, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < OPT; ++i)
    if (live[i]) dst[t0 + threadIdx.x + i * RS_THREADS - t_org] = acc[i];
}

// Tile `blockIdx.x % tiles` of clip `blockIdx.x / tiles`.
template <int OPT, bool STAGED>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const float* __restrict__ wave, int64_t clip_stride, int64_t n_samples,
    const float* __restrict__ bankT, int P, int Q, int L, float* __restrict__ out, int64_t out_stride,
    int64_t n_out, int tiles, int span_cap) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const int64_t clip_id = blockIdx.x / (unsigned)tiles;
  const int64_t t0 = (int64_t)(blockIdx.x % (unsigned)tiles) * (OPT * RS_THREADS);
  const ClipFetch fetch{wave + clip_id * clip_stride, n_samples};
  resample_tile<OPT, STAGED>(fetch, bankT, P, Q, L, out + clip_id * out_stride, t0, n_out, 0, span_cap, xs);
}

// Tile blockIdx.x of the outputs [t_begin, t_end) of one unbounded signal, out[t - t_begin].
template <int OPT, bool STAGED>
__global__ __launch_bounds__(RS_THREADS) void resample_stream_kernel(
    SlideFetch fetch, const float* __restrict__ bankT, int P, int Q, int L, float* __restrict__ out,
    int64_t t_begin, int64_t t_end, int span_cap) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const int64_t t0 = t_begin + (int64_t)blockIdx.x * (OPT * RS_THREADS);
  resample_tile<OPT, STAGED>(fetch, bankT, P, Q, L, out, t0, t_end, t_begin, span_cap, xs);
}

}  // namespace a2m

using namespace a2m;

extern "C" {

int64_t a2m_resample_num_samples(int64_t n_samples, int32_t sr_in, int32_t sr_out) {
  if (n_samples <= 0 || sr_in <= 0 || sr_out <= 0) return 0;
  const __int128 n = ((__int128)n_samples * sr_out + sr_in - 1) / sr_in;
  return n > (__int128)INT64_MAX ? 0 : (int64_t)n;
}

size_t a2m_resample_plan_bytes(int32_t sr_in, int32_t sr_out, int32_t num_zeros, double beta,
                               double rolloff) {
  size_t need = 0;
  if (resample_plan(sr_in, sr_out, num_zeros, beta, rolloff, nullptr, 0, &need)) return 0;
  return need;
}

int a2m_resample_plan_build(int32_t sr_in, int32_t sr_out, int32_t num_zeros, double beta,
                            double rolloff, void* host_plan, size_t plan_bytes) {
  size_t need = 0;
  A2M_CHECK_ARG(host_plan, "resample: null plan buffer");
  return resample_plan(sr_in, sr_out, num_zeros, beta, rolloff, host_plan, plan_bytes, &need);
}

int a2m_resample_plan_bank(const void* host_plan, size_t plan_bytes, int32_t* P, int32_t* Q, int32_t* L,
                           float* bank) {
  A2M_CHECK_ARG(host_plan && plan_bytes >= sizeof(ResampleHeader), "resample: bad plan");
  const unsigned char* p = static_cast<const unsigned char*>(host_plan);
  ResampleHeader h;
  std::memcpy(&h, p, sizeof(h));
  A2M_CHECK_ARG(h.P >= 1 && h.Q >= 1 && h.L >= 1 && 2 * (int64_t)h.L <= RS_MAX_BANK / h.Q &&
                    h.off_bank >= (int32_t)sizeof(ResampleHeader) &&
                    (size_t)h.off_bank + sizeof(float) * 2 * (size_t)h.L * h.Q <= plan_bytes,
                "resample: bad plan");
  if (P) *P = h.P;
  if (Q) *Q = h.Q;
  if (L) *L = h.L;
  if (bank == nullptr) return A2M_OK;
  const float* bankT = reinterpret_cast<const float*>(p + h.off_bank);
  const int64_t taps = 2 * (int64_t)h.L;
  for (int64_t r = 0; r < h.Q; ++r) {
    const int64_t phase = r * h.P % h.Q;
    for (int64_t j = 0; j < taps; ++j) bank[phase * taps + j] = bankT[j * h.Q + r];
  }
  return A2M_OK;
}

int a2m_resample_f32(const float* wave, int64_t n_clips, int64_t clip_stride, int64_t n_samples,
                     int32_t sr_in, int32_t sr_out, int32_t num_zeros, const void* dev_plan, float* out,
                     int64_t out_stride, int64_t n_out, void* stream) {
  A2M_CHECK_ARG(n_clips >= 0 && n_samples >= 0 && n_out >= 0, "resample: negative size");
  Ratio r;
  const int rc = resample_ratio(sr_in, sr_out, num_zeros, &r);
  if (rc) return rc;
  A2M_CHECK_ARG(n_samples <= ((int64_t)1 << 62) / r.Q, "resample: %lld samples x Q = %lld does not fit 62 bits",
                (long long)n_samples, (long long)r.Q);
  const int64_t want = a2m_resample_num_samples(n_samples, sr_in, sr_out);
  A2M_CHECK_ARG(n_out == want, "resample: n_out %lld != ceil(n_samples * sr_out / sr_in) = %lld",
                (long long)n_out, (long long)want);
  if (n_out == 0 || n_clips == 0) return A2M_OK;
  A2M_CHECK_ARG(wave && out && dev_plan, "resample: null pointer");
  const float* bankT = reinterpret_cast<const float*>(static_cast<const unsigned char*>(dev_plan) +
                                                      rs_align16(sizeof(ResampleHeader)));
  // span of a full tile: n_{t0 + TILE - 1} - n_{t0} <= ceil((TILE - 1) P / Q), plus the 2 L taps
  const int64_t span = ((RS_TILE - 1) * r.P + r.Q - 1) / r.Q + 2 * r.L;
  const bool staged = span <= RS_MAX_SPAN;
  const int64_t tiles = cdiv(n_out, staged ? RS_TILE : RS_THREADS);
  A2M_CHECK_ARG(tiles < (1LL << 31) / n_clips, "resample: too many output tiles");
  const dim3 grid((unsigned)(tiles * n_clips));
  if (staged) {
    hipLaunchKernelGGL((resample_kernel<RS_OPT, true>), grid, dim3(RS_THREADS), sizeof(float) * (size_t)span,
                       as_stream(stream), wave, clip_stride, n_samples, bankT, (int)r.P, (int)r.Q, (int)r.L,
                       out, out_stride, n_out, (int)tiles, (int)span);
  } else {
    hipLaunchKernelGGL((resample_kernel<1, false>), grid, dim3(RS_THREADS), 0, as_stream(stream), wave,
                       clip_stride, n_samples, bankT, (int)r.P, (int)r.Q, (int)r.L, out, out_stride, n_out,
                       (int)tiles, 0);
  }
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_resample_stream_f32(const float* buf, int64_t base, int64_t len, int64_t n_total, int32_t sr_in,
                            int32_t sr_out, int32_t num_zeros, const void* dev_plan, int64_t t_begin,
                            int64_t n_out, float* out, void* stream) {
  A2M_CHECK_ARG(base >= 0 && len >= 0 && t_begin >= 0 && n_out >= 0,
                "resample_stream: negative size (base %lld len %lld t_begin %lld n_out %lld)",
                (long long)base, (long long)len, (long long)t_begin, (long long)n_out);
  Ratio r;
  const int rc = resample_ratio(sr_in, sr_out, num_zeros, &r);
  if (rc) return rc;
  const int64_t lim = ((int64_t)1 << 62) / std::max(r.P, r.Q);
  A2M_CHECK_ARG(base <= lim - len && t_begin <= lim - n_out && n_total <= lim,
                "resample_stream: sample or output indices times P or Q do not fit 62 bits");
  if (n_out == 0) return A2M_OK;
  A2M_CHECK_ARG(buf && out && dev_plan, "resample_stream: null pointer");
  // samples the outputs [t_begin, t_begin + n_out) read: [need_lo, need_hi]; what of it is not a
  // defined zero (g < 0, or g >= n_total once the end is known) must lie in the buffer
  const int64_t t_end = t_begin + n_out;
  const int64_t need_lo = std::max<int64_t>(t_begin * r.P / r.Q - r.L + 1, 0);
  int64_t need_hi = (t_end - 1) * r.P / r.Q + r.L;
  if (n_total >= 0) need_hi = std::min(need_hi, n_total - 1);
  A2M_CHECK_ARG(need_lo > need_hi || (need_lo >= base && need_hi < base + len),
                "resample_stream: outputs [%lld, %lld) read samples [%lld, %lld], the buffer holds "
                "[%lld, %lld)",
                (long long)t_begin, (long long)t_end, (long long)need_lo, (long long)need_hi,
                (long long)base, (long long)(base + len));
  SlideFetch fetch;
  fetch.buf = buf;
  fetch.base = base;
  fetch.lo = base;  // base >= 0
  fetch.hi = n_total >= 0 ? std::min(base + len, n_total) : base + len;
  const float* bankT = reinterpret_cast<const float*>(static_cast<const unsigned char*>(dev_plan) +
                                                      rs_align16(sizeof(ResampleHeader)));
  const int64_t span = ((RS_TILE - 1) * r.P + r.Q - 1) / r.Q + 2 * r.L;  // as a2m_resample_f32
  const bool staged = span <= RS_MAX_SPAN;
  const int64_t tiles = cdiv(n_out, staged ? RS_TILE : RS_THREADS);
  A2M_CHECK_ARG(tiles < (1LL << 31), "resample_stream: too many output tiles");
  const dim3 grid((unsigned)tiles);
  if (staged) {
    hipLaunchKernelGGL((resample_stream_kernel<RS_OPT, true>), grid, dim3(RS_THREADS),
                       sizeof(float) * (size_t)span, as_stream(stream), fetch, bankT, (int)r.P, (int)r.Q,
                       (int)r.L, out, t_begin, t_end, (int)span);
  } else {
    hipLaunchKernelGGL((resample_stream_kernel<1, false>), grid, dim3(RS_THREADS), 0, as_stream(stream),
                       fetch, bankT, (int)r.P, (int)r.Q, (int)r.L, out, t_begin, t_end, 0);
  }
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

}  // extern "C"
