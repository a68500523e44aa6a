// Implicit-GEMM engine: host side (split-K reduce, launch of the route that gemm_route.cpp
// decides).  The kernels and their description are in gemm_kernel.h, timing in gemm_timing.hip.
#include <algorithm>
#include <atomic>

#include "gemm_kernel.h"
#include "gemm_pipe_bf16.h"
#include "gemm_route.h"

namespace a2m {

// Fixed-order (s = 0, 1, ...) sum of the split-K slabs + epilogue.  Slabs are [M][N], or
// [N][M] for m-contiguous outputs (args.mcontig), so the inner slab index is also the output's
// contiguous one.  Four consecutive inner elements per thread (float4) when the inner extent
// is a multiple of 4, and the slab loads of four splits are issued before their adds, so the
// pass is bandwidth- rather than latency-bound.
__device__ __forceinline__ void reduce_store(const GemmArgs& args, int z, float v, int o, int in) {
  const int m = args.mcontig ? in : o, n = args.mcontig ? o : in;
  epi_store(args.E, z, v, m, epi_addr(args.E, m, n));
}

// Four consecutive inner elements (in .. in+3) of output row / column o: the epilogue
// constants and the column decomposition are computed once per float4 (mcontig: one column n,
// rows in..in+3; otherwise one row m, columns in..in+3).
__device__ __forceinline__ void reduce_store4(const GemmArgs& args, int z, const float4& v, int o, int in) {
  const Epilogue& E = args.E;
  const float vv[4] = {v.x, v.y, v.z, v.w};
  if (args.mcontig) {
    EpiCol c;
    c.set(E, o);
    const int64_t an = c.addr(E);
    const int64_t off = (int64_t)z * E.bstride + an + in;
    const int mp = in + z * E.pstride;
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (E.som == 1 && !E.res1 && !E.res2 && !E.gamma && al16(E.out + off) && (!E.bias || al16(E.bias + mp)) &&
        (!E.bn_w || (al16(E.bn_w + mp) && al16(E.bn_b + mp) && al16(E.bn_rm + mp) && al16(E.bn_rv + mp)))) {
      // four consecutive channels of one output position: vector parameter loads and store
      float4 bi = make_float4(0.f, 0.f, 0.f, 0.f), w = bi, b = bi, rm = bi, rv = bi;
      if (E.bias) bi = *reinterpret_cast<const float4*>(E.bias + mp);
      if (E.bn_w) {
        w = *reinterpret_cast<const float4*>(E.bn_w + mp);
        b = *reinterpret_cast<const float4*>(E.bn_b + mp);
        rm = *reinterpret_cast<const float4*>(E.bn_rm + mp);
        rv = *reinterpret_cast<const float4*>(E.bn_rv + mp);
      }
      const float bia[4] = {bi.x, bi.y, bi.z, bi.w}, wa[4] = {w.x, w.y, w.z, w.w};
      const float ba[4] = {b.x, b.y, b.z, b.w}, rma[4] = {rm.x, rm.y, rm.z, rm.w};
      const float rva[4] = {rv.x, rv.y, rv.z, rv.w};
      float o4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const EpiRow r{bia[j], rma[j], E.bn_w ? wa[j] / sqrtf(rva[j] + E.bn_eps) : 1.f, ba[j]};
        o4[j] = epi_value_p(E, vv[j], r);
      }
      float4 out4 = make_float4(o4[0], o4[1], o4[2], o4[3]);
      if (E.accumulate) {
        const float4 q = *reinterpret_cast<const float4*>(E.out + off);
        out4.x += q.x; out4.y += q.y; out4.z += q.z; out4.w += q.w;
      }
      *reinterpret_cast<float4*>(E.out + off) = out4;
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = in + j;
      epi_store_p(E, z, vv[j], epi_row(E, m + z * E.pstride), an + (int64_t)m * E.som);
    }
  } else {
    const EpiRow r = epi_row(E, o + z * E.pstride);
    const int64_t am = (int64_t)o * E.som;
    EpiCol c;
    c.set(E, in);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j) c.advance(E, 1);
      epi_store_p(E, z, vv[j], r, c.addr(E) + am);
    }
  }
}

template <typename I>
__device__ __forceinline__ void splitk_reduce4(const GemmArgs& args, int batch) {
  const I MN = (I)args.M * args.N;
  const int S = args.splits;
  const I inner = args.mcontig ? args.M : args.N;
  const I total4 = MN * batch / 4;
  for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total4; i += (I)gridDim.x * blockDim.x) {
    const I e = i * 4;
    const int z = (int)(e / MN);
    const I mn = e - (I)z * MN;
    const int o = (int)(mn / inner), in = (int)(mn - (I)o * inner);
    const float* p = args.partial + (int64_t)z * S * MN + mn;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = 0;
    for (; s + 4 <= S; s += 4) {
      const float4 a0 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 0) * MN);
      const float4 a1 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 1) * MN);
      const float4 a2 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 2) * MN);
      const float4 a3 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 3) * MN);
      v.x += a0.x; v.y += a0.y; v.z += a0.z; v.w += a0.w;
      v.x += a1.x; v.y += a1.y; v.z += a1.z; v.w += a1.w;
      v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w;
      v.x += a3.x; v.y += a3.y; v.z += a3.z; v.w += a3.w;
    }
    for (; s < S; ++s) {
      const float4 a = *reinterpret_cast<const float4*>(p + (int64_t)s * MN);
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    reduce_store4(args, z, v, o, in);
  }
}

__device__ __forceinline__ void splitk_reduce(const GemmArgs& args, int batch) {
  const int64_t MN = (int64_t)args.M * args.N;
  const int S = args.splits;
  const int inner = args.mcontig ? args.M : args.N;
  if ((inner & 3) == 0) {
    // 32-bit index arithmetic whenever the slab set fits (the 64-bit divisions cost more than
    // the float4 loads they address)
    if (MN * batch < (int64_t)1 << 31) splitk_reduce4<int>(args, batch);
    else splitk_reduce4<int64_t>(args, batch);
    return;
  }
  const int64_t total = MN * batch;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int z = (int)(i / MN);
    const int64_t mn = i - (int64_t)z * MN;
    const int o = (int)(mn / inner), in = (int)(mn - (int64_t)o * inner);
    const float* p = args.partial + (int64_t)z * S * MN + mn;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += p[s * MN];
    reduce_store(args, z, v, o, in);
  }
}

// the reduce's span stamps follow the tile kernel's in the launch's record
__device__ __forceinline__ unsigned long long* reduce_span(const GemmArgs& args) {
  return args.ts ? args.ts + kSpanSlots : nullptr;
}

__global__ void splitk_reduce_kernel(GemmArgs args, int batch) {
  span_begin(reduce_span(args));
  splitk_reduce(args, batch);
  span_end(reduce_span(args));
}

// Many splits over few outputs (graph-layer weight gradients: 64 x 64 outputs, K up to 172,032
// nodes, 128-256 splits): the per-thread serial sum above would be latency-bound on a handful of
// blocks, so here 16 lanes of a block share one float4 of outputs, each summing the splits
// s = lane, lane + 16, ... in order, and the 16 lane sums are added in lane order (a fixed order:
// still bitwise reproducible).  Inner extent a multiple of 4.
constexpr int RW_LANES = 16, RW_COLS = 16;
__device__ __forceinline__ void splitk_reduce_wide(const GemmArgs& args, int batch) {
  __shared__ float4 red[RW_LANES][RW_COLS];
  const int64_t MN = (int64_t)args.M * args.N;
  const int S = args.splits;
  const int inner = args.mcontig ? args.M : args.N;
  const int col = threadIdx.x % RW_COLS, lane = threadIdx.x / RW_COLS;
  const int64_t i = (int64_t)blockIdx.x * RW_COLS + col;
  const int64_t total4 = MN * batch / 4;
  const int64_t e = i * 4;
  const int z = (int)(e / MN);
  const int64_t mn = e - (int64_t)z * MN;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < total4) {
    const float* p = args.partial + (int64_t)z * S * MN + mn;
    int s = lane;
    for (; s + 3 * RW_LANES < S; s += 4 * RW_LANES) {
      const float4 a0 = *reinterpret_cast<const float4*>(p + (int64_t)s * MN);
      const float4 a1 = *reinterpret_cast<const float4*>(p + (int64_t)(s + RW_LANES) * MN);
      const float4 a2 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 2 * RW_LANES) * MN);
      const float4 a3 = *reinterpret_cast<const float4*>(p + (int64_t)(s + 3 * RW_LANES) * MN);
      v.x += a0.x; v.y += a0.y; v.z += a0.z; v.w += a0.w;
      v.x += a1.x; v.y += a1.y; v.z += a1.z; v.w += a1.w;
      v.x += a2.x; v.y += a2.y; v.z += a2.z; v.w += a2.w;
      v.x += a3.x; v.y += a3.y; v.z += a3.z; v.w += a3.w;
    }
    for (; s < S; s += RW_LANES) {
      const float4 a = *reinterpret_cast<const float4*>(p + (int64_t)s * MN);
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
  }
  red[lane][col] = v;
  __syncthreads();
  if (lane != 0 || i >= total4) return;
  for (int l = 1; l < RW_LANES; ++l) {
    const float4 a = red[l][col];
    v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
  }
  const int o = (int)(mn / inner), in = (int)(mn - (int64_t)o * inner);
  reduce_store4(args, z, v, o, in);
}

__global__ __launch_bounds__(RW_LANES * RW_COLS) void splitk_reduce_wide_kernel(GemmArgs args,
                                                                               int batch) {
  span_begin(reduce_span(args));
  splitk_reduce_wide(args, batch);
  span_end(reduce_span(args));
}

// The AudioEncoder's last conv (one live output column, model_layers.py:272) with the
// bilinear time resample (model_layers.py:277-279) fused into its split-K reduce: phase 1 sums
// the slabs of RB whole (m, b) rows of H values in fixed order s = 0, 1, ... (the order of
// splitk_reduce_kernel, or splitk_reduce_wide_kernel's where the unfused path would use that
// kernel) and applies the epilogue into LDS; phase 2 writes those rows' T
// outputs y[b][m][t] from the LDS rows with exactly interp_time_at's operations (ops.hip), so
// the result is the unfused conv + interp_time_kernel's bit for bit, without the [B][Co][H][W]
// round trip and the second launch.  Slabs are [M][N], n = b * H + h (rows (m, b) contiguous).
__global__ __launch_bounds__(256) void splitk_reduce_interp_kernel(GemmArgs args, int nb, int RB, int wide) {
  span_begin(reduce_span(args));
  extern __shared__ float sv[];   // [RB][H]
  const Epilogue& E = args.E;
  const int H = E.interp_H, T = E.interp_T, M = args.M, S = args.splits;
  const int64_t MN = (int64_t)M * args.N;
  const int rows = M * nb;
  const int r0 = blockIdx.x * RB;
  const int nr = min(RB, rows - r0);
  for (int e = threadIdx.x; e < nr * H; e += blockDim.x) {
    const float* p = args.partial + (int64_t)r0 * H + e;   // row r0 + e / H, h = e % H
    float v = 0.f;
    if (wide) {
      // the order of splitk_reduce_wide_kernel (which the unfused path uses at these sizes):
      // RW_LANES strided partial sums, then added in lane order
      for (int l = 0; l < RW_LANES; ++l) {
        float vl = 0.f;
        for (int s = l; s < S; s += RW_LANES) vl += p[s * MN];
        if (l == 0) v = vl;
        else v += vl;
      }
    } else {
      int s = 0;
      for (; s + 4 <= S; s += 4) {
        const float a0 = p[(s + 0) * MN], a1 = p[(s + 1) * MN], a2 = p[(s + 2) * MN], a3 = p[(s + 3) * MN];
        v += a0; v += a1; v += a2; v += a3;
      }
      for (; s < S; ++s) v += p[s * MN];
    }
    const int m = (r0 + e / H) / nb;
    sv[e] = epi_value_p(E, v, epi_row(E, m));
  }
  __syncthreads();
  const float sh = (float)H / (float)T, lw0 = E.interp_lw0;
  for (int o = threadIdx.x; o < nr * T; o += blockDim.x) {
    const int rl = o / T, t = o - rl * T;
    const int r = r0 + rl, m = r / nb, b = r - m * nb;
    float src = sh * ((float)t + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    const int h0 = (int)src;
    const int h1 = h0 + (h0 < H - 1 ? 1 : 0);
    const float lh1 = src - (float)h0, lh0 = 1.f - lh1;
    float v = lh0 * (lw0 * sv[rl * H + h0]);
    if (lh1 != 0.f) v += lh1 * (lw0 * sv[rl * H + h1]);
    E.out[((int64_t)b * M + m) * T + t] = v;
  }
  span_end(reduce_span(args));
}

// XCD-aware block order: groups of 8 M-tiles share an XCD's L2 (40 MB a launch instead of ~64 MB
// at a 0.5 % step cost; identity order and groups of 2 / 4 measured within noise)
static int gemm_xcd_group() { return 8; }

// the process-wide switches of the route (RouteConfig, gemm_route.h)
static int g_gemm_prec = 0;
static int g_override_tile = 0, g_override_split = 0;   // a2m_gemm_plan_override (tuning)
static int g_pipe_override = -1;   // a2m_gemm_pipe_override: -1 default (pipelined), 0 gemm_tile, 1 pipelined
static int g_pair_override = -1;   // a2m_convt_pair_override: -1 default (gemm_pair's fill rule), 0 never, 1 whenever eligible

RouteConfig route_config() {
  // A2M_GEMM_HALO=0: mode 5 re-stores the window shifted for every tap (the round-3 loader)
  static const int halo_on = env_int("A2M_GEMM_HALO", 1);
  return {g_gemm_prec, g_pipe_override, g_pair_override, g_override_tile, g_override_split, halo_on, XFORM_NONE};
}

int gemm_k_tile() { return gemm_bk(g_gemm_prec); }
size_t gemm_ws_bytes(int M, int N, int K, int batch) { return gemm_ws_bytes(M, N, K, batch, route_config()); }

// launches per A2M_GEMM_KIND_* since the last reset (a2m_gemm_kernel_counts), counted where the
// launch is issued
static std::atomic<int64_t> g_kind_counts[4];

static void fill_args(GemmArgs& a, const Gather& A, const Gather& B, const Epilogue& E, int M, int N, int K,
                      const GemmRoute& r) {
  a.A = A; a.B = B; a.E = E; a.M = M; a.N = N; a.K = K;
  a.B.halo = r.halo;
  a.splits = r.splits;
  a.kchunk = r.kchunk;
  a.partial = nullptr;
  a.xcd_group = gemm_xcd_group();
  a.mcontig = r.mcontig;
  a.vec4 = r.vec4;
  a.ts = nullptr;
}

// the tile kernel the route names; false: the library carries no such kernel
static bool launch_route(const GemmArgs& a, const GemmRoute& r, int prec, int batch, hipStream_t stream) {
  if (r.kind == A2M_GEMM_KIND_PIPE && r.xform != XFORM_NONE) {
    if (r.xform == XFORM_WINO) launch_pipe_wino(a, batch, stream);
    else launch_pipe_down(a, batch, stream);
    return true;
  }
  if (r.kind == A2M_GEMM_KIND_PIPE)
    return prec == 1 ? launch_pipe_bf16(a, r.pipe_mb, r.pipe_nt, r.pipe_ma, batch, stream)
                     : prec == 0 && launch_pipe(a, r.pipe_mb, r.pipe_nt, r.pipe_ma, batch, stream);
  if (r.kind != A2M_GEMM_KIND_TILE && r.kind != A2M_GEMM_KIND_TILE_KS2) return false;
  if (r.ks == 2) {
    launch_tile<64, 64, 32, 0, 2>(a, r.ma, r.mb, batch, stream);
  } else if (prec == 1) {
    if (r.tile == 128) launch_tile<128, 128, 64, 1>(a, r.ma, r.mb, batch, stream);
    else launch_tile<64, 64, 64, 1>(a, r.ma, r.mb, batch, stream);
#ifdef A2M_WITH_X6
  } else if (prec == 2) {
    if (r.tile == 128) launch_tile<128, 128, 32, 2>(a, r.ma, r.mb, batch, stream);
    else launch_tile<64, 64, 32, 2>(a, r.ma, r.mb, batch, stream);
#endif
  } else {
    if (r.tile == 128) launch_tile<128, 128, 32, 0>(a, r.ma, r.mb, batch, stream);
    else launch_tile<64, 64, 32, 0>(a, r.ma, r.mb, batch, stream);
  }
  return true;
}

// per Xform: the tile's name in a refusal, its A2M_GEMM_LOG suffix and its timing-description suffix
static const char* const kXformTile[] = {"", "Winograd", "down-sampling"};
static const char* const kXformLog[] = {" (pipe)", " (pipe) (wino)", " (pipe) (down)"};
static const char* const kXformDesc[] = {"", " wino", " down"};

int gemm(const Gather& A, const Gather& B, const Epilogue& E, int M, int N, int K, int batch,
         void* ws, size_t ws_bytes, hipStream_t stream, int force_split, Xform xform) {
  A2M_CHECK_ARG(M > 0 && N > 0 && K >= 0 && batch > 0, "gemm: bad sizes M=%d N=%d K=%d batch=%d",
                M, N, K, batch);
  A2M_CHECK_ARG(E.interp_T <= 0 || (batch == 1 && E.interp_H > 0 && N % E.interp_H == 0 &&
                                    (size_t)E.interp_H * sizeof(float) <= 32768),
                "gemm: fused resample needs batch 1, N a multiple of H = %d <= 8192", E.interp_H);
  RouteConfig cfg = route_config();
  cfg.xform = xform;
  const GemmRoute r = gemm_route(A, B, E, M, N, K, batch, force_split, cfg);
  // A holds the tile's packed weights: no other kernel can take them (a route names a tile on request only)
  A2M_CHECK_ARG(r.xform == xform, "gemm: the route refuses the %s tile for M=%d N=%d K=%d batch=%d", kXformTile[xform], M,
                N, K, batch);
  GemmArgs a;
  fill_args(a, A, B, E, M, N, K, r);
  if (r.reduce) {
    const size_t need = split_ws_bytes(r, M, N, batch);
    if (ws == nullptr || ws_bytes < need) {
      set_error("gemm: workspace too small (%zu < %zu bytes)", ws_bytes, need);
      return A2M_EWS;
    }
    a.partial = static_cast<float*>(ws);
  }
  static const int log_launches = env_int("A2M_GEMM_LOG", 0);
  if (log_launches)
    std::fprintf(stderr, "a2m gemm M=%d N=%d K=%d batch=%d tile=%d bk=%d splits=%d%s modes=%d,%d som=%d so=%d,%d,%d N12=%d,%d\n",
                 M, N, K, batch, r.tile, r.bk, r.splits, r.kind == A2M_GEMM_KIND_PIPE ? kXformLog[r.xform] : "", r.ma, r.mb, E.som,
                 E.so0, E.so1, E.so2, E.N1, E.N2);
  if (timing_enabled()) {
    char desc[96];
    std::snprintf(desc, sizeof(desc), "M=%d N=%d K=%d b=%d tile=%d split=%d modes=%d,%d%s", M, N, K,
                  batch, r.tile, r.splits, r.ma, r.mb, kXformDesc[r.xform]);
    a.ts = timing_open(2.0 * M * N * (double)K * batch, desc, r.reduce, stream);
  }
  if (!launch_route(a, r, cfg.prec, batch, stream)) {
    set_error("gemm: no kernel for kind %d tile %d precision %d (pipe <%d, %d, %d>)", r.kind, r.tile, cfg.prec,
              r.pipe_mb, r.pipe_nt, r.pipe_ma);
    return A2M_EINVAL;
  }
  ++g_kind_counts[r.kind];
  A2M_LAUNCH_CHECK();
  if (r.interp) {
    const int H = E.interp_H, nb = N / H;
    // whole (m, b) rows per block: ~2,048 outputs, the rows' H values staged in LDS
    const int RB = std::max(1, std::min(2048 / std::max(E.interp_T, 1), 8192 / H));
    const int wide = (N & 3) == 0 && r.splits >= 2 * RW_LANES && (int64_t)M * N / 4 <= 65536;
    hipLaunchKernelGGL(splitk_reduce_interp_kernel, dim3((unsigned)cdiv((int64_t)M * nb, RB)), dim3(256),
                       (size_t)RB * H * sizeof(float), stream, a, nb, RB, wide);
    A2M_LAUNCH_CHECK();
  } else if (r.splits > 1) {
    const int inner = a.mcontig ? M : N;
    const int64_t total = (int64_t)M * N * batch / ((inner & 3) == 0 ? 4 : 1);
    if ((inner & 3) == 0 && r.splits >= 2 * RW_LANES && total <= 65536) {
      hipLaunchKernelGGL(splitk_reduce_wide_kernel, dim3((unsigned)cdiv(total, RW_COLS)),
                         dim3(RW_LANES * RW_COLS), 0, stream, a, batch);
    } else {
      const int blocks = (int)std::min<int64_t>(cdiv(total, 256), 8192);
      hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, a, batch);
    }
    A2M_LAUNCH_CHECK();
  }
  return A2M_OK;
}

// The two output phases of a stride-2 ConvTranspose1d as one launch of the fp32 pipelined tile
// (gemm_pipe_kernel_pair): two mode-5 per-tap problems of equal M and N, each at one split, the one
// with more k-steps at grid z = 0 so that the long tiles are dispatched first.  Taken only where
// gemm() held to one split would launch the fp32 pipelined tile's per-tap kernel for both (each
// phase's route says so: fp32, dense packed weights, 1-3 taps over clips that tile the 64 rows,
// offsets below 2^29, 64x64 tile) and neither epilogue is a fused resample; a split count forced
// by a2m_gemm_plan_override / A2M_GEMM_PLAN_RULES other than 1 keeps the sequential path.  By default (a2m_convt_pair_override(-1)) also only where the pair
// puts at least one block on every CU (2 tiles(M, N) >= 256): below that, split-K is how the
// planner fills the chip, which one split per problem would undo.  Each problem's results are
// bitwise those of its own gemm() launch at one split.  Returns kGemmPairNotTaken (the caller
// issues the two gemm() calls) or gemm()'s status.
int gemm_pair(const Gather& A0, const Gather& B0, const Epilogue& E0, int K0, const Gather& A1,
              const Gather& B1, const Epilogue& E1, int K1, int M, int N, hipStream_t stream) {
  A2M_CHECK_ARG(M > 0 && N > 0 && K0 > 0 && K1 > 0, "gemm_pair: bad sizes M=%d N=%d K=%d,%d", M, N, K0, K1);
  RouteConfig cfg = route_config();
  cfg.halo_on = 0;   // the per-tap layout (the halo layout's results are bitwise the same)
  if (cfg.pair_override == 0 || cfg.prec != 0 || cfg.override_split > 1) return kGemmPairNotTaken;
  if (cfg.pair_override < 0 && 2 * cdiv(M, 64) * cdiv(N, 64) < 256) return kGemmPairNotTaken;
  const Gather* As[2] = {&A0, &A1};
  const Gather* Bs[2] = {&B0, &B1};
  const Epilogue* Es[2] = {&E0, &E1};
  const int Ks[2] = {K0, K1};
  GemmRoute r[2];
  GemmArgs a[2];
  for (int i = 0; i < 2; ++i) {
    r[i] = gemm_route(*As[i], *Bs[i], *Es[i], M, N, Ks[i], 1, 1, cfg);
    if (r[i].kind != A2M_GEMM_KIND_PIPE || r[i].pipe_mb != 5 || r[i].pipe_nt < 1 || r[i].pipe_nt > 3 ||
        r[i].interp || plan_rule_splits(M, N, Ks[i]))
      return kGemmPairNotTaken;
    fill_args(a[i], *As[i], *Bs[i], *Es[i], M, N, Ks[i], r[i]);
  }
  const int first = K1 > K0 ? 1 : 0;   // grid z = 0: the problem with more k-steps
  static const int log_launches = env_int("A2M_GEMM_LOG", 0);
  if (log_launches)
    std::fprintf(stderr, "a2m gemm pair M=%d N=%d K=%d+%d tile=64 bk=32 splits=1 (pipe) taps=%d+%d\n", M, N,
                 Ks[first], Ks[first ^ 1], a[first].B.tapconv, a[first ^ 1].B.tapconv);
  if (timing_enabled()) {   // one record for the pair: both problems' blocks stamp the same span slots
    char desc[96];
    std::snprintf(desc, sizeof(desc), "pair M=%d N=%d K=%d+%d b=1 tile=64 split=1 modes=0,5", M, N,
                  Ks[first], Ks[first ^ 1]);
    a[0].ts = a[1].ts = timing_open(2.0 * M * N * ((double)K0 + K1), desc, false, stream);
  }
  launch_pipe_pair(a[first], a[first ^ 1], r[first].pipe_nt, r[first ^ 1].pipe_nt, stream);
  ++g_kind_counts[A2M_GEMM_KIND_PIPE_PAIR];
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

}  // namespace a2m

extern "C" {

int a2m_convt_pair_override(int32_t mode) {
  A2M_CHECK_ARG(mode >= -1 && mode <= 1, "convt_pair_override: %d (-1 default, 0 off, 1 on)", mode);
  a2m::g_pair_override = mode;
  return A2M_OK;
}

int a2m_gemm_plan_override(int32_t tile, int32_t splits) {
  A2M_CHECK_ARG((tile == 0 || tile == 64 || tile == 128) && splits >= 0 && splits <= 256,
                "gemm_plan_override: tile %d splits %d", tile, splits);
  a2m::g_override_tile = tile;
  a2m::g_override_split = splits;
  return A2M_OK;
}

int a2m_gemm_pipe_override(int32_t mode) {
  A2M_CHECK_ARG(mode >= -1 && mode <= 1, "gemm_pipe_override: %d (-1 env, 0 off, 1 on)", mode);
  a2m::g_pipe_override = mode;
  return A2M_OK;
}

int a2m_set_gemm_precision(int32_t prec) {
#ifdef A2M_WITH_X6
  A2M_CHECK_ARG(prec >= 0 && prec <= 2, "set_gemm_precision: %d (0 = fp32, 1 = bf16, 2 = bf16x6)", prec);
#else
  // bf16x6 (2) is a build-time option (make EXTRA=-DA2M_WITH_X6): an experiment that measured
  // slower than fp32 end to end, so the shipped library carries fp32 and bf16 only
  A2M_CHECK_ARG(prec >= 0 && prec <= 1, "set_gemm_precision: %d (0 = fp32, 1 = bf16)", prec);
#endif
  a2m::g_gemm_prec = prec;
  return A2M_OK;
}

int32_t a2m_get_gemm_precision(void) { return a2m::g_gemm_prec; }

int a2m_gemm_kernel_counts(int64_t counts[4], int32_t reset) {
  A2M_CHECK_ARG(counts != nullptr, "gemm_kernel_counts: null counts");
  for (int k = 0; k < 4; ++k) counts[k] = reset ? a2m::g_kind_counts[k].exchange(0) : a2m::g_kind_counts[k].load();
  return A2M_OK;
}

}  // extern "C"
