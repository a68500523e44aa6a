// Implicit-GEMM engine: per-launch timing records and named wall-clock marks (measurement only).
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "gemm_kernel.h"

namespace a2m {

// Optional per-launch timing of the engine (bench.py's live roofline).  While enabled, every
// launch gets a record of four span stamps in a device buffer (GemmArgs::ts): the tile kernel's
// earliest block start / latest wave end and the split-K reduce's, on the GPU's constant-rate
// wall clock (span_begin / span_end, gemm_kernel.h).  The stamps are written by the kernels
// themselves, so they time the same launches eagerly and in every replay of a graph captured
// while timing was on (bench.py's in-step roofline: the step captured once more, replayed, read
// after each replay).  HIP event records were tried first: inside a graph they become
// separate nodes whose timestamps include each kernel's dispatch (+3.5 us a launch against the
// rocprof kernel trace, r04_v1), and hipExtLaunchKernel's kernel-timestamp events are not
// updated under capture (tools/micro/ext_events.hip).  Off by default, no cost when off.
struct GemmTiming {
  double flops;
  bool reduce;
  char desc[96];   // shape/plan, printed per launch by a2m_gemm_timing_read under A2M_GEMM_LOG=2
};
constexpr int kTimingRecs = 1024;   // launches per timing window
static std::mutex g_timing_mu;
static bool g_timing = false;
static bool g_timing_overflow = false;
static std::vector<GemmTiming> g_timing_recs;
// tile spans + reduce spans + the launch's ready mark (and a pad slot; A2M_GEMM_TIMING_READY=1):
// the wall clock at which a one-thread mark kernel, enqueued right before the tile kernel on its
// stream, ran -- i.e.
// when the stream reached the launch (its previous kernel done), so last end - ready counts the
// launch's dispatch and any wait for free CUs behind the other decoder branch, as a kernel
// trace's duration does
constexpr int kRecSlots = 2 * kSpanSlots + 2;
constexpr int kReadySlot = 2 * kSpanSlots;
static unsigned long long* g_ts = nullptr;   // [kTimingRecs][kRecSlots] + [A2M_TIMING_MARKS] mark slots
static double g_wall_mhz = 0.0;

// (re)arm the stamps: start slots at the maximum, end slots at 0
static int timing_reset_stamps() {
  std::vector<unsigned long long> init((size_t)kTimingRecs * kRecSlots, 0ull);
  for (size_t i = 0; i < init.size(); i += 2) init[i] = ~0ull;
  return hipMemcpy(g_ts, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) ==
         hipSuccess ? A2M_OK : A2M_EHIP;
}

__global__ void timing_mark_kernel(unsigned long long* p) {
  if (threadIdx.x == 0) *p = (unsigned long long)wall_clock64();
}

static int timing_alloc() {
  if (g_ts) return A2M_OK;
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0 ||
      hipMalloc(&g_ts, ((size_t)kTimingRecs * kRecSlots + A2M_TIMING_MARKS) * sizeof(unsigned long long)) != hipSuccess) {
    set_error("gemm timing: device stamp buffer / wall clock rate unavailable");
    g_ts = nullptr;
    return A2M_EHIP;
  }
  g_wall_mhz = khz / 1e3;
  return hipMemset(g_ts, 0, ((size_t)kTimingRecs * kRecSlots + A2M_TIMING_MARKS) * sizeof(unsigned long long)) ==
         hipSuccess ? A2M_OK : A2M_EHIP;
}

bool timing_enabled() { return g_timing; }

// Opens the next record of the window: null when timing is off or the window is full.
unsigned long long* timing_open(double flops, const char* desc, bool reduce, hipStream_t stream) {
  std::lock_guard<std::mutex> lk(g_timing_mu);
  if (!g_timing || !g_ts) return nullptr;
  if ((int)g_timing_recs.size() >= kTimingRecs) {
    g_timing_overflow = true;
    return nullptr;
  }
  GemmTiming t{};
  t.flops = flops;
  t.reduce = reduce;
  std::snprintf(t.desc, sizeof(t.desc), "%s", desc);
  g_timing_recs.push_back(t);
  unsigned long long* ts = g_ts + kRecSlots * (g_timing_recs.size() - 1);
  // A2M_GEMM_TIMING_READY=1 (diagnostic): the ready mark.  Off by default: the extra kernel
  // per launch shifts how the two decoder branches share the CUs (tools/stamp_vs_trace.py)
  static const int ready = env_int("A2M_GEMM_TIMING_READY", 0);
  if (ready) hipLaunchKernelGGL(timing_mark_kernel, dim3(1), dim3(64), 0, stream, ts + kReadySlot);
  return ts;
}

}  // namespace a2m

extern "C" {

int a2m_gemm_timing_begin(void) {
  std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
  int rc = a2m::timing_alloc();
  if (rc == A2M_OK) rc = a2m::timing_reset_stamps();
  if (rc != A2M_OK) return rc;
  a2m::g_timing_recs.clear();
  a2m::g_timing_overflow = false;
  a2m::g_timing = true;
  return A2M_OK;
}

int a2m_gemm_timing_stop(void) {
  std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
  a2m::g_timing = false;
  return A2M_OK;
}

int a2m_gemm_timing_read(int64_t* launches, double* flops, double* ms_tile, double* ms_reduce,
                         int64_t* reduces) {
  return a2m_gemm_timing_read_ex(launches, flops, ms_tile, ms_reduce, reduces, nullptr);
}

int a2m_gemm_timing_read_ex(int64_t* launches, double* flops, double* ms_tile, double* ms_reduce,
                            int64_t* reduces, double* ms_queued) {
  std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
  A2M_CHECK_ARG(a2m::g_ts != nullptr, "gemm_timing_read: timing was never begun");
  A2M_CHECK_ARG(!a2m::g_timing_overflow, "gemm_timing_read: more than %d launches in the window",
                a2m::kTimingRecs);
  const size_t nrec = a2m::g_timing_recs.size();
  const int R = a2m::kRecSlots, S = a2m::kSpanSlots;
  std::vector<unsigned long long> st(nrec * R + 1);
  if (hipDeviceSynchronize() != hipSuccess ||
      (nrec && hipMemcpy(st.data(), a2m::g_ts, nrec * R * sizeof(unsigned long long), hipMemcpyDeviceToHost) !=
                   hipSuccess)) {
    a2m::set_error("gemm timing: stamp read failed");
    return A2M_EHIP;
  }
  // a kernel's duration: last block end - first block start over all XCDs (s_memrealtime is the
  // chip's one constant-rate clock, so stamps from different XCDs are comparable: the same
  // assumption as ms_queued and a2m_timing_mark_to_launch_end); -1: nothing stamped since the
  // last reset.  *global is that interval, the return value too (kept for the log line).
  auto span = [](const unsigned long long* s, double* global) {
    double best = -1.0;
    unsigned long long glo = ~0ull, ghi = 0;
    for (int x = 0; x < 8; ++x) {
      unsigned long long lo = ~0ull, hi = 0;
      for (int l = 0; l < a2m::kSpanLanes; ++l) {
        const unsigned long long* q = s + 2 * (x * a2m::kSpanLanes + l);
        if (q[0] == ~0ull || q[1] < q[0]) continue;
        lo = std::min(lo, q[0]);
        hi = std::max(hi, q[1]);
      }
      if (lo == ~0ull) continue;
      best = std::max(best, (double)(hi - lo));
      glo = std::min(glo, lo);
      ghi = std::max(ghi, hi);
    }
    *global = ghi >= glo ? (double)(ghi - glo) : -1.0;
    return best < 0 ? -1.0 : *global;
  };
  int64_t n = 0, nr = 0;
  double f = 0, mt = 0, mr = 0, mq = 0;
  int rc = A2M_OK;
  const double tick_ms = 1.0 / (a2m::g_wall_mhz * 1e3);
  for (size_t i = 0; i < nrec; ++i) {
    const a2m::GemmTiming& t = a2m::g_timing_recs[i];
    double ga = 0, gb = 0;
    const double sa = span(&st[i * R], &ga), sb = t.reduce ? span(&st[i * R + S], &gb) : 0.0;
    if (sa < 0 || sb < 0) {
      a2m::set_error("gemm timing: launch %zu (%s) has no stamps", i, t.desc);
      rc = A2M_EHIP;
      continue;
    }
    const double a = sa * tick_ms, b = sb * tick_ms;
    // ready mark .. last block end over all XCDs (the constant-rate clock is common to them)
    const unsigned long long rdy = st[i * R + a2m::kReadySlot];
    if (ms_queued && rdy != ~0ull && ga >= 0) {
      unsigned long long hi = 0;
      for (int q = 1; q < S; q += 2)
        if (st[i * R + q - 1] != ~0ull && st[i * R + q] >= st[i * R + q - 1]) hi = std::max(hi, st[i * R + q]);
      mq += hi > rdy ? (double)(hi - rdy) * tick_ms : a;
    }
    ++n;
    f += t.flops;
    static const int log_launches = a2m::env_int("A2M_GEMM_LOG", 0);
    if (log_launches >= 2)
      std::fprintf(stderr, "a2m gemm-time %s tile %.1f us (all-XCD span %.1f) reduce %.1f us %.1f TF\n", t.desc,
                   1e3 * a, 1e3 * ga * tick_ms, 1e3 * b, a > 0 ? t.flops / (1e9 * a) : 0.0);
    mt += a;
    if (t.reduce) { mr += b; ++nr; }
  }
  if (launches) *launches = n;
  if (flops) *flops = f;
  if (ms_tile) *ms_tile = mt;
  if (ms_reduce) *ms_reduce = mr;
  if (reduces) *reduces = nr;
  if (ms_queued) *ms_queued = mq;
  // re-arm for the next replay of a graph that carries these launches
  if (a2m::timing_reset_stamps() != A2M_OK) {
    a2m::set_error("gemm timing: stamp reset failed");
    return A2M_EHIP;
  }
  return rc;
}

int a2m_gemm_timing_read_spans(int64_t cap, double* start_us, double* end_us, int64_t* n) {
  return a2m_gemm_timing_read_spans_ex(cap, nullptr, start_us, end_us, n);
}

int a2m_gemm_timing_read_spans_ex(int64_t cap, double* ready_us, double* start_us, double* end_us,
                                  int64_t* n) {
  std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
  A2M_CHECK_ARG(a2m::g_ts != nullptr && start_us && end_us && n && cap >= 0,
                "gemm_timing_read_spans: bad arguments (or timing never begun)");
  const size_t nrec = std::min<size_t>(a2m::g_timing_recs.size(), (size_t)cap);
  const int R = a2m::kRecSlots;
  std::vector<unsigned long long> st(nrec * R + 1);
  if (hipDeviceSynchronize() != hipSuccess ||
      (nrec && hipMemcpy(st.data(), a2m::g_ts, nrec * R * sizeof(unsigned long long), hipMemcpyDeviceToHost) !=
                   hipSuccess)) {
    a2m::set_error("gemm timing: stamp read failed");
    return A2M_EHIP;
  }
  for (size_t i = 0; i < nrec; ++i) {
    unsigned long long lo = ~0ull, hi = 0;
    for (int s = 0; s < a2m::kSpanSlots; s += 2) {
      const unsigned long long* q = &st[i * R + s];
      if (q[0] == ~0ull || q[1] < q[0]) continue;
      lo = std::min(lo, q[0]);
      hi = std::max(hi, q[1]);
    }
    start_us[i] = lo == ~0ull ? -1.0 : (double)lo / a2m::g_wall_mhz;
    end_us[i] = lo == ~0ull ? -1.0 : (double)hi / a2m::g_wall_mhz;
    if (ready_us) {
      const unsigned long long r = st[i * R + a2m::kReadySlot];
      ready_us[i] = r == ~0ull ? -1.0 : (double)r / a2m::g_wall_mhz;
    }
  }
  *n = (int64_t)nrec;
  return a2m::timing_reset_stamps() == A2M_OK ? A2M_OK : A2M_EHIP;
}

int a2m_gemm_timing_end(int64_t* launches, double* flops, double* ms_tile, double* ms_reduce,
                        int64_t* reduces) {
  a2m_gemm_timing_stop();
  const int rc = a2m_gemm_timing_read(launches, flops, ms_tile, ms_reduce, reduces);
  std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
  a2m::g_timing_recs.clear();
  return rc;
}

int a2m_gemm_timing_clear(void) {
  std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
  a2m::g_timing = false;
  a2m::g_timing_recs.clear();
  return A2M_OK;
}

// Named wall-clock marks (bench.py's in-step phase split: step start, log-mel done, encoder
// done): a one-thread kernel stores the clock into the mark's slot, so a mark captured into a
// graph re-stamps on every replay.  Its own dispatch is ~1-2 us of the interval it opens.
int a2m_timing_mark(int32_t slot, void* stream) {
  A2M_CHECK_ARG(slot >= 0 && slot < A2M_TIMING_MARKS, "timing_mark: slot %d", slot);
  if (!a2m::g_ts) {   // allocate the stamp buffer here unless the stream is being captured
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    A2M_CHECK_ARG(hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cs) == hipSuccess &&
                      cs == hipStreamCaptureStatusNone,
                  "timing_mark: first mark inside a stream capture (call a2m_gemm_timing_begin first)");
    std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
    const int rc = a2m::timing_alloc();
    if (rc != A2M_OK) return rc;
  }
  hipLaunchKernelGGL(a2m::timing_mark_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     a2m::g_ts + (size_t)a2m::kTimingRecs * a2m::kRecSlots + slot);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_timing_mark_elapsed(int32_t a, int32_t b, float* ms) {
  A2M_CHECK_ARG(a >= 0 && a < A2M_TIMING_MARKS && b >= 0 && b < A2M_TIMING_MARKS && a2m::g_ts && ms,
                "timing_mark_elapsed: slots %d, %d", a, b);
  unsigned long long m[A2M_TIMING_MARKS];
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(m, a2m::g_ts + (size_t)a2m::kTimingRecs * a2m::kRecSlots, sizeof(m), hipMemcpyDeviceToHost) != hipSuccess) {
    a2m::set_error("timing_mark_elapsed: stamp read failed");
    return A2M_EHIP;
  }
  *ms = (float)((double)((long long)(m[b] - m[a])) / (a2m::g_wall_mhz * 1e3));
  return A2M_OK;
}

int a2m_timing_mark_to_launch_end(int32_t slot, int64_t rec, float* ms) {
  std::lock_guard<std::mutex> lk(a2m::g_timing_mu);
  A2M_CHECK_ARG(slot >= 0 && slot < A2M_TIMING_MARKS && a2m::g_ts && ms && rec >= 0 &&
                    rec < (int64_t)a2m::g_timing_recs.size(),
                "timing_mark_to_launch_end: slot %d, record %lld", slot, (long long)rec);
  const int R = a2m::kRecSlots;
  std::vector<unsigned long long> st(R);
  unsigned long long m[A2M_TIMING_MARKS];
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(st.data(), a2m::g_ts + (size_t)rec * R, R * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(m, a2m::g_ts + (size_t)a2m::kTimingRecs * R, sizeof(m), hipMemcpyDeviceToHost) != hipSuccess) {
    a2m::set_error("timing_mark_to_launch_end: stamp read failed");
    return A2M_EHIP;
  }
  unsigned long long hi = 0;
  for (int q = 0; q < 2 * a2m::kSpanSlots; q += 2)   // tile and reduce slots
    if (st[q] != ~0ull && st[q + 1] >= st[q]) hi = std::max(hi, st[q + 1]);
  A2M_CHECK_ARG(hi > 0, "timing_mark_to_launch_end: record %lld has no stamps", (long long)rec);
  *ms = (float)((double)((long long)(hi - m[slot])) / (a2m::g_wall_mhz * 1e3));
  return A2M_OK;
}

}  // extern "C"
