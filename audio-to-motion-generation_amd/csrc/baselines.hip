// The evaluation baselines' two kernels (a2m/baselines.py): a nearest-neighbour search and an
// exact per-channel median over the windows of the PATS loader's arena.  Both read the arena
// through the start table in place, exactly as batch_gather_kernel (data.hip) addresses it: the
// window at table position p is the rows arena[start[p] + j*interval], j < T.
//
// nn_search_kernel: d(b,p) = (|q_b|^2 + |w_p|^2) - 2 q_b.w_p.  A workgroup of four waves owns a
// 64-query x 64-candidate tile, each wave one 32x32 accumulator of mfma_f32_32x32x2f32 (exact fp32:
// a k-ordered fma chain per output element, the same k order for every element, so the computed
// value is a function of the two vectors alone).  K = T*C is streamed through LDS in 64-float
// chunks, register-staged one chunk ahead with unconditional loads at clamped addresses; the norms
// are summed by the staging threads (an fma chain over each thread's float4 column, then a 16-lane
// tree).  Every lane keeps the running
// (distance bits, candidate) minimum of its 16 accumulator rows over the chunk's tiles; the
// chunk's minimum per query goes to its own slot of the workspace and nn_finish_kernel takes the
// minimum over the chunks: no atomics, no dependence on scheduling.
//
// window_median: a radix select on key(x) = bits ^ (sign ? ~0 : 1 << 31), 8 bits a pass from the
// top.  median_hist_kernel counts, per channel and for both ranks, the byte of every value whose
// higher bytes match the rank's prefix (LDS histograms, integer atomics, flushed to HBM);
// median_choose_kernel walks the 256 counts to the bucket holding the rank.  After four passes
// the prefix is the element itself.
#include "a2m_internal.h"

namespace a2m {

constexpr int NN_T = 64;        // tile edge: queries and candidates per workgroup step
constexpr int NN_BK = 64;       // floats of K per LDS chunk
constexpr int NN_LD = NN_BK + 4;  // LDS row stride (floats): rows stay 16-byte aligned
constexpr int NN_MAX_CHUNKS = 2048;
constexpr int NECK_F = 104, NECK_J = 52;

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct NnArgs {
  const float* arena;
  const int64_t* start;
  const float* mean;
  const float* std_;
  const float* query;
  unsigned long long* part;  // [n_chunks][B]
  int64_t lo;
  int n_cand, C, c4, interval, K, B, standardise, tiles_per_chunk, n_tiles;
};

struct NnStage {
  float4 q[4], w[4], m, s;
};

__device__ __forceinline__ float sq4(float4 v, float s) {
  return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, s))));
}

__device__ __forceinline__ float4 scale4(float4 v, float s) {
  return make_float4(__fmul_rn(v.x, s), __fmul_rn(v.y, s), __fmul_rn(v.z, s), __fmul_rn(v.w, s));
}

// Chunk `chunk` of K for this thread's four rows of the query and of the candidate tile.  Every
// load is unconditional, at an address clamped into range: a load behind a branch makes the
// compiler wait for each in turn instead of keeping them all in flight under the MFMAs.  A query
// or candidate row past the end is a copy of the last one (its results are never used); a float4
// past K is the last float4, and nn_finish_stage multiplies it by 0.
template <bool STD>
__device__ __forceinline__ void nn_load(const NnArgs& A, int chunk, int sq, const int64_t* qoff,
                                        const int64_t* wbase, NnStage& st) {
  const int kq = min(chunk * (NN_BK / 4) + sq, A.K / 4 - 1);  // float4 index into K
  const int j = kq / A.c4;
  const int cq = kq - j * A.c4;
  if (STD) {
    st.m = reinterpret_cast<const float4*>(A.mean)[cq];
    st.s = reinterpret_cast<const float4*>(A.std_)[cq];
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    st.q[it] = *reinterpret_cast<const float4*>(A.query + qoff[it] + 4 * (int64_t)kq);
    st.w[it] = *reinterpret_cast<const float4*>(A.arena + (wbase[it] + (int64_t)j * A.interval) * A.C + 4 * cq);
  }
}

// The staged chunk's values as they enter LDS: the candidate standardised by the gather's formula
// (every step rounded once), and everything times 1, or times 0 for a float4 past K (a product, not
// a select: finite values give +-0, which adds nothing to an fma chain that starts at +0).
template <bool STD>
__device__ __forceinline__ void nn_finish_stage(const NnArgs& A, int chunk, int sq, NnStage& st) {
  const float live = 4 * (int64_t)(chunk * (NN_BK / 4) + sq) < A.K ? 1.f : 0.f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    float4 v = st.w[it];
    if (STD) {
      v.x = __fdiv_rn(__fsub_rn(v.x, st.m.x), st.s.x < 1e-7f ? 1.f : st.s.x);
      v.y = __fdiv_rn(__fsub_rn(v.y, st.m.y), st.s.y < 1e-7f ? 1.f : st.s.y);
      v.z = __fdiv_rn(__fsub_rn(v.z, st.m.z), st.s.z < 1e-7f ? 1.f : st.s.z);
      v.w = __fdiv_rn(__fsub_rn(v.w, st.m.w), st.s.w < 1e-7f ? 1.f : st.s.w);
    }
    st.w[it] = scale4(v, live);
    st.q[it] = scale4(st.q[it], live);
  }
}

template <bool STD>
__global__ void __launch_bounds__(256) nn_search_kernel(NnArgs A) {
  __shared__ __attribute__((aligned(16))) float Qs[NN_T * NN_LD];
  __shared__ __attribute__((aligned(16))) float Ws[NN_T * NN_LD];
  __shared__ float qqs[NN_T], wws[NN_T];
  __shared__ unsigned long long red[2][NN_T];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qh = wave >> 1, ch = wave & 1;  // the wave's 32 queries x 32 candidates of the tile
  const int li = lane & 31, lh = lane >> 5;
  const int sq = tid & 15, srow = tid >> 4;  // staging: float4 column of the chunk, first of 4 rows
  const int qb = blockIdx.y * NN_T;
  const int nk = (A.K + NN_BK - 1) / NN_BK;
  const int tile0 = blockIdx.x * A.tiles_per_chunk;
  const int tile1 = min(tile0 + A.tiles_per_chunk, A.n_tiles);

  unsigned long long kmin[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) kmin[r] = ~0ull;

  int64_t qoff[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) qoff[it] = (int64_t)min(qb + srow + 16 * it, A.B - 1) * A.K;

  for (int tile = tile0; tile < tile1; ++tile) {
    int64_t wbase[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) wbase[it] = A.start[A.lo + min(tile * NN_T + srow + 16 * it, A.n_cand - 1)];
    float qpart[4] = {0.f, 0.f, 0.f, 0.f}, wpart[4] = {0.f, 0.f, 0.f, 0.f};
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    NnStage st;
    nn_load<STD>(A, 0, sq, qoff, wbase, st);
    for (int c = 0; c < nk; ++c) {
      nn_finish_stage<STD>(A, c, sq, st);
      __syncthreads();  // the previous chunk's fragments (and the previous tile's norms) are read
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = srow + 16 * it;
        *reinterpret_cast<float4*>(Qs + row * NN_LD + 4 * sq) = st.q[it];
        *reinterpret_cast<float4*>(Ws + row * NN_LD + 4 * sq) = st.w[it];
        qpart[it] = sq4(st.q[it], qpart[it]);
        wpart[it] = sq4(st.w[it], wpart[it]);
      }
      __syncthreads();
      __builtin_amdgcn_sched_barrier(0);            // the stage is consumed: its registers take the next loads
      nn_load<STD>(A, c + 1, sq, qoff, wbase, st);  // past the last chunk: clamped, never stored
      __builtin_amdgcn_sched_barrier(0);            // the loads are issued ahead of the MFMAs they overlap
      // MFMA step: lane half h supplies k = 32 h + s of the chunk, s = 0..31, for A and B alike
      const float* qa = Qs + (qh * 32 + li) * NN_LD + lh * 32;
      const float* wb = Ws + (ch * 32 + li) * NN_LD + lh * 32;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float4 a = *reinterpret_cast<const float4*>(qa + 4 * t);
        const float4 b = *reinterpret_cast<const float4*>(wb + 4 * t);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
      }
    }
    // the norms: the 16 staging threads of a row are one 16-lane DPP row
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const float qq = row16_sum(qpart[it]), ww = row16_sum(wpart[it]);
      if (sq == 0) {
        qqs[srow + 16 * it] = qq;
        wws[srow + 16 * it] = ww;
      }
    }
    __syncthreads();
    const int rel = tile * NN_T + ch * 32 + li;  // this lane's candidate: the accumulator's column
    if (rel < A.n_cand) {
      const float ww = wws[ch * 32 + li];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = qh * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float d = __fsub_rn(__fadd_rn(qqs[row], ww), __fmul_rn(2.f, acc[r]));
        d = d > 0.f ? d : 0.f;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)rel;
        kmin[r] = key < kmin[r] ? key : kmin[r];
      }
    }
  }

  // minimum over the 32 candidate lanes of each wave half, then over the two candidate waves
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    unsigned long long k = kmin[r];
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
      const unsigned long long o = __shfl_xor(k, m);
      k = o < k ? o : k;
    }
    if (li == 0) red[ch][qh * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = k;
  }
  __syncthreads();
  if (tid < NN_T && qb + tid < A.B) {
    const unsigned long long a = red[0][tid], b = red[1][tid];
    A.part[(int64_t)blockIdx.x * A.B + qb + tid] = a < b ? a : b;
  }
}

__global__ void nn_finish_kernel(const unsigned long long* __restrict__ part, int n_chunks, int B,
                                 int64_t lo, int64_t* __restrict__ best, float* __restrict__ best_dist) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  unsigned long long k = part[b];
  for (int c = 1; c < n_chunks; ++c) {
    const unsigned long long o = part[(int64_t)c * B + b];
    k = o < k ? o : k;
  }
  best[b] = lo + (int64_t)(k & 0xffffffffull);
  best_dist[b] = __uint_as_float((unsigned)(k >> 32));
}

static void nn_plan(int64_t n_cand, int& n_tiles, int& tiles_per_chunk, int& n_chunks) {
  n_tiles = (int)cdiv(n_cand, NN_T);
  tiles_per_chunk = (int)cdiv(n_tiles, NN_MAX_CHUNKS);
  n_chunks = (int)cdiv(n_tiles, tiles_per_chunk);
}

// ------------------------------------------------------------------------------------ median
constexpr int MED_CG = 16;     // channels of a workgroup (4 float4 columns)
constexpr int MED_ROWS = 64;   // window rows of a workgroup step
constexpr int MED_MAX_BLOCKS = 1024;

// ws: state [C][4] (prefix of rank 0, 1; remaining rank 0, 1), then hist [4 passes][C][2][256]
__host__ __device__ inline size_t med_hist_off(int C) { return (size_t)C * 4; }

__device__ __forceinline__ unsigned med_key(float x) {
  const unsigned u = __float_as_uint(x);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__global__ void __launch_bounds__(256) median_hist_kernel(const float* __restrict__ arena,
                                                          const int64_t* __restrict__ start, int64_t lo,
                                                          int64_t M, int T, int C, int interval, int necksub,
                                                          int pass, unsigned* __restrict__ ws) {
  __shared__ unsigned hist[MED_CG * 2 * 256];
  __shared__ unsigned prefix[MED_CG * 2];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * MED_CG;
  for (int i = tid; i < MED_CG * 2 * 256; i += 256) hist[i] = 0;
  if (tid < MED_CG * 2) {
    const int c = c0 + (tid >> 1);
    prefix[tid] = (pass > 0 && c < C) ? ws[(size_t)c * 4 + (tid & 1)] : 0;
  }
  __syncthreads();
  const int quad = tid & 3, slot = tid >> 2;
  const int cq = c0 + 4 * quad;  // first of this thread's four channels
  const int shift = 24 - 8 * pass;
  if (cq < C) {
    for (int64_t m = (int64_t)blockIdx.x * MED_ROWS + slot; m < M; m += (int64_t)gridDim.x * MED_ROWS) {
      const int64_t p = m / T;
      const int j = (int)(m - p * T);
      const float* src = arena + (start[lo + p] + (int64_t)j * interval) * C;
      const float4 v = *reinterpret_cast<const float4*>(src + cq);
      float x[4] = {v.x, v.y, v.z, v.w};
      if (necksub) {
        const float neck = src[cq < NECK_J ? 0 : NECK_J];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = __fsub_rn(x[k], neck);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned key = med_key(x[k]);
        const unsigned bin = (key >> shift) & 255u;
        const unsigned high = pass == 0 ? 0u : key >> ((shift + 8) & 31);  // prefix[] is 0 in pass 0
        const int lc = 4 * quad + k;
#pragma unroll
        for (int w = 0; w < 2; ++w)
          if (high == prefix[2 * lc + w]) atomicAdd(&hist[(2 * lc + w) * 256 + bin], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* ghist = ws + med_hist_off(C) + (size_t)pass * C * 512;
  for (int i = tid; i < MED_CG * 512; i += 256) {
    const int c = c0 + (i >> 9);
    if (c < C && hist[i]) atomicAdd(&ghist[(size_t)c * 512 + (i & 511)], hist[i]);
  }
}

// One thread per (channel, rank): the bucket of this pass that holds the rank.  The last pass
// completes the key and the thread of rank 0 writes the median.
__global__ void median_choose_kernel(unsigned* __restrict__ ws, int C, int pass, unsigned rank0, unsigned rank1,
                                     float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = i >> 1, w = i & 1;
  unsigned key = 0;
  if (c < C) {
    unsigned* state = ws + (size_t)c * 4;
    const unsigned* h = ws + med_hist_off(C) + ((size_t)pass * C + c) * 512 + w * 256;
    unsigned rank = pass == 0 ? (w ? rank1 : rank0) : state[2 + w];
    const unsigned pre = pass == 0 ? 0u : state[w];
    unsigned b = 0;
    for (; b < 255; ++b) {
      const unsigned n = h[b];
      if (rank < n) break;
      rank -= n;
    }
    key = (pre << 8) | b;
    state[w] = key;
    state[2 + w] = rank;
  }
  if (pass < 3) return;
  // the two rank threads of a channel are neighbouring lanes of one wave
  const unsigned other = __shfl_xor(key, 1);
  if (c < C && w == 0) {
    const unsigned u0 = key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu);
    const unsigned u1 = other ^ ((other >> 31) ? 0x80000000u : 0xffffffffu);
    const float a = __uint_as_float(u0), b = __uint_as_float(u1);
    out[c] = rank0 == rank1 ? a : (float)(((double)a + (double)b) * 0.5);
  }
}

}  // namespace a2m

using namespace a2m;

extern "C" size_t a2m_nn_search_ws_bytes(int32_t B, int64_t n_cand) {
  if (B <= 0 || n_cand <= 0 || n_cand > (int64_t)0x7fff0000) return 0;
  int n_tiles, tpc, n_chunks;
  nn_plan(n_cand, n_tiles, tpc, n_chunks);
  return (size_t)n_chunks * (size_t)B * sizeof(unsigned long long);
}

extern "C" int a2m_nn_search_f32(const float* arena, const int64_t* start, int64_t lo, int64_t n_cand, int32_t C,
                                 int32_t window, int32_t interval, int32_t mode, const float* mean,
                                 const float* std_, const float* query, int32_t B, int64_t* best,
                                 float* best_dist, void* ws, size_t ws_bytes, void* stream) {
  A2M_CHECK_ARG(arena && start && query && best && best_dist && ws, "nn_search: null argument");
  A2M_CHECK_ARG(B > 0 && n_cand > 0, "nn_search: B %d or n_cand %lld is not positive", B, (long long)n_cand);
  A2M_CHECK_ARG(window > 0 && interval > 0, "nn_search: window %d, interval %d", window, interval);
  A2M_CHECK_ARG(C > 0 && C % 4 == 0, "nn_search: C %d is not a positive multiple of 4", C);
  A2M_CHECK_ARG(lo >= 0, "nn_search: lo %lld is negative", (long long)lo);
  A2M_CHECK_ARG(mode == A2M_BATCH_RAW || mode == A2M_BATCH_STANDARDISE, "nn_search: unknown mode %d", mode);
  if (mode == A2M_BATCH_RAW)
    A2M_CHECK_ARG(!mean && !std_, "nn_search: mean / std given for the raw mode");
  else
    A2M_CHECK_ARG(mean && std_, "nn_search: the standardise mode needs mean and std");
  A2M_CHECK_ARG(((uintptr_t)arena | (uintptr_t)query | (uintptr_t)mean | (uintptr_t)std_) % 16 == 0,
                "nn_search: arena, query, mean and std must be 16-byte aligned");
  A2M_CHECK_ARG((uintptr_t)ws % 8 == 0, "nn_search: ws must be 8-byte aligned");
  A2M_CHECK_ARG(n_cand <= (int64_t)0x7fff0000, "nn_search: n_cand %lld exceeds 2^31 - 2^16", (long long)n_cand);
  const int64_t T = cdiv(window, interval), K = T * C;
  A2M_CHECK_ARG(K <= ((int64_t)1 << 30), "nn_search: T*C = %lld exceeds 2^30", (long long)K);
  A2M_CHECK_ARG(ws_bytes >= a2m_nn_search_ws_bytes(B, n_cand), "nn_search: ws_bytes %zu < %zu", ws_bytes,
                a2m_nn_search_ws_bytes(B, n_cand));
  NnArgs A{};
  A.arena = arena; A.start = start; A.mean = mean; A.std_ = std_; A.query = query;
  A.part = static_cast<unsigned long long*>(ws);
  A.lo = lo; A.n_cand = (int)n_cand; A.C = C; A.c4 = C / 4; A.interval = interval; A.K = (int)K; A.B = B;
  A.standardise = mode == A2M_BATCH_STANDARDISE;
  int n_chunks;
  nn_plan(n_cand, A.n_tiles, A.tiles_per_chunk, n_chunks);
  const int q_tiles = (int)cdiv(B, NN_T);
  A2M_CHECK_ARG(q_tiles <= 65535, "nn_search: B %d exceeds %d", B, 65535 * NN_T);
  if (A.standardise)
    hipLaunchKernelGGL(nn_search_kernel<true>, dim3(n_chunks, q_tiles), dim3(256), 0, as_stream(stream), A);
  else
    hipLaunchKernelGGL(nn_search_kernel<false>, dim3(n_chunks, q_tiles), dim3(256), 0, as_stream(stream), A);
  A2M_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_finish_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, as_stream(stream), A.part,
                     n_chunks, B, lo, best, best_dist);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

extern "C" size_t a2m_window_median_ws_bytes(int32_t C) {
  if (C <= 0 || C > (1 << 20)) return 0;
  return (med_hist_off(C) + (size_t)4 * C * 512) * sizeof(unsigned);
}

extern "C" int a2m_window_median_f32(const float* arena, const int64_t* start, int64_t lo, int64_t n, int32_t C,
                                     int32_t window, int32_t interval, int32_t mode, float* out, void* ws,
                                     size_t ws_bytes, void* stream) {
  A2M_CHECK_ARG(arena && start && out && ws, "window_median: null argument");
  A2M_CHECK_ARG(n > 0, "window_median: n %lld is not positive", (long long)n);
  A2M_CHECK_ARG(window > 0 && interval > 0, "window_median: window %d, interval %d", window, interval);
  A2M_CHECK_ARG(C > 0 && C % 4 == 0 && C <= (1 << 20), "window_median: C %d is not a multiple of 4 in [4, 2^20]", C);
  A2M_CHECK_ARG(lo >= 0, "window_median: lo %lld is negative", (long long)lo);
  A2M_CHECK_ARG(mode == A2M_BATCH_RAW || mode == A2M_BATCH_NECKSUB, "window_median: unknown mode %d", mode);
  A2M_CHECK_ARG(mode != A2M_BATCH_NECKSUB || C == NECK_F, "window_median: the neck-sub mode needs C = 104, got %d", C);
  A2M_CHECK_ARG((uintptr_t)arena % 16 == 0 && (uintptr_t)ws % 4 == 0,
                "window_median: arena must be 16-byte and ws 4-byte aligned");
  const int64_t T = cdiv(window, interval);
  A2M_CHECK_ARG(n < ((int64_t)1 << 32) && n * T < ((int64_t)1 << 32), "window_median: n*T = %lld * %lld reaches 2^32",
                (long long)n, (long long)T);
  A2M_CHECK_ARG(ws_bytes >= a2m_window_median_ws_bytes(C), "window_median: ws_bytes %zu < %zu", ws_bytes,
                a2m_window_median_ws_bytes(C));
  const int64_t M = n * T;
  const unsigned rank0 = (unsigned)((M - 1) / 2), rank1 = (unsigned)(M / 2);
  hipStream_t st = as_stream(stream);
  unsigned* w = static_cast<unsigned*>(ws);
  A2M_CHECK_HIP(hipMemsetAsync(w, 0, a2m_window_median_ws_bytes(C), st));
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(M, MED_ROWS), MED_MAX_BLOCKS), (unsigned)cdiv(C, MED_CG));
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(median_hist_kernel, grid, dim3(256), 0, st, arena, start, lo, M, (int)T, C, interval,
                       mode == A2M_BATCH_NECKSUB ? 1 : 0, pass, w);
    A2M_LAUNCH_CHECK();
    hipLaunchKernelGGL(median_choose_kernel, dim3((unsigned)cdiv(2 * (int64_t)C, 256)), dim3(256), 0, st, w, C, pass,
                       rank0, rank1, out);
    A2M_LAUNCH_CHECK();
  }
  return A2M_OK;
}
