// Scaffold of the transform tiles of the software-pipelined 64x64 fp32 tile (gemm_pipe.h): the
// Winograd F(2,3) tile (gemm_f32_pipe_wino.hip) and the Toom-Cook F(2,2) down-sampling tile
// (gemm_f32_pipe_down.hip).  Such a tile computes a 64x64 y tile as 64 rows x 32 pairs of outputs
// (y[2i], y[2i + 1]) from a few GEMMs M_p = U_p V_p of 64 x 32 pairs each: A is the packed U (dense
// rows of whole 32-k units), B the x window transformed in registers into V units [pair][36].
// Shared here: the A loader, the pair-row permutation of the V units, the epilogue that turns the
// waves' two accumulators back into one MFMA-layout accumulator of the y tile, and the launcher.
// A tile's own file keeps what makes it that tile: the x-window loader with its transform, the LDS
// sizes and the step schedule.
#pragma once
#include "gemm_pipe.h"

namespace a2m {

constexpr int kXformTA = 2 * 64 * kPipeLDK;   // an A stage: two units x 64 rows
constexpr int kXformUnit = 32 * kPipeLDK;     // a V unit: 32 pairs

// V unit row of pair i (bits 1 and 2 swapped, an involution): a thread's pairs 2G, 2G + 1
// (G = tid / 16) land 4 rows from those of G + 1, i.e. 16 banks on, which keeps the 32 lanes of a
// ds_write_b32 on distinct banks; lane li of a fragment read takes row li, so it computes pair
// xform_pair_row(li)
__device__ __forceinline__ int xform_pair_row(int i) { return (i & ~6) | ((i & 2) << 1) | ((i & 4) >> 1); }

// A: dense rows of KU floats (the packed U: 4 Ci or 6 Ci); a step's tile is 64 rows x 64 k (the
// step's first unit, then its second), four float4 per thread: q = 2 * unit + row half
struct XformRows {
  __amdgpu_buffer_rsrc_t rs;
  uint32_t off[2];
  int kq, lrow, knext, KU;
  __device__ __forceinline__ void init(const Gather& g, int z, int row0, int R, int KKU, int tid, int kbeg) {
    rs = pipe_rsrc(g.base + (int64_t)z * g.bstride);
    kq = (tid & 7) * 4;
    lrow = tid >> 3;
    KU = KKU;
    knext = kbeg;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = row0 + lrow + 32 * p;
      off[p] = row < R ? (uint32_t)(row * g.sr0 + kbeg + kq) * 4u : kPipeOOB;
    }
  }
  template <int Q>
  __device__ __forceinline__ void load(float4 (&r)[4]) {
    r[Q] = pipe_load(rs, knext < KU ? off[Q & 1] + 4u * 32 * (Q >> 1) : kPipeOOB);
    if (Q == 3) {
      off[0] += 4u * 64;
      off[1] += 4u * 64;
      knext += 64;
    }
  }
  template <int Q>
  __device__ __forceinline__ void store(float* st, const float4 (&r)[4]) const {
    *reinterpret_cast<float4*>(st + ((Q >> 1) * 64 + lrow + 32 * (Q & 1)) * kPipeLDK + kq) = r[Q];
  }
};

// After the k loop: wave (wm, wn) holds rows wm * 32 .. + 31 x all 32 pairs of M plane `plane0` in
// acc0 and of `plane1` in acc1.  The four planes go to LDS as [plane][row][pair] (pitch 32: a
// ds_write_b32's 32 lanes are one row's 32 pairs; the planes reuse the stages, at least 4 * 64 * 32
// floats), every lane rebuilds column n = wn * 32 + li of the y tile in the accumulator layout of a
// wave that owns rows wm * 32 .. and columns wn * 32 .. as combine(M1, M2, Me, odd) -- M1 / M2:
// planes 1 / 2 of pair n / 2, Me: plane 3 for the pair's odd output, plane 0 for its even one --
// and the tile's existing epilogues run unchanged (vec4 / scalar / m-contiguous / split-K slab: the
// transforms are linear, so slabs hold transformed outputs and splitk_reduce_kernel serves).
template <class Combine>
__device__ __forceinline__ void xform_epilogue(const GemmArgs& args, float* lds, EpiRow* epr, const floatx16& acc0,
                                               int plane0, const floatx16& acc1, int plane1, Combine combine, int zz,
                                               int batch, int m0, int n0, int tid, int wm, int wn, int li, int lh) {
  __syncthreads();   // the M planes reuse the stages
  const int pair = xform_pair_row(li);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
    lds[(plane0 * 64 + row) * 32 + pair] = acc0[q];
    lds[(plane1 * 64 + row) * 32 + pair] = acc1[q];
  }
  __syncthreads();
  floatx16 acc;
  {
    const int n = wn * 32 + li;
    const bool odd = n & 1;
    const float* const pm = lds + (n >> 1);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh;
      const float M1 = pm[(64 + row) * 32], M2 = pm[(128 + row) * 32];
      const float Me = pm[((odd ? 192 : 0) + row) * 32];
      acc[q] = combine(M1, M2, Me, odd);
    }
  }
  __syncthreads();   // the epilogues stage the tile through the same LDS
  floatx16 accs[1][1];
  accs[0][0] = acc;
  if (args.vec4) pipe_epilogue_vec4(args, acc, lds, epr, args.partial != nullptr, zz, batch, m0, n0, tid, wm, wn, li, lh);
  else tile_epilogue<64, 64, 1, 1>(args, accs, lds, epr, args.partial != nullptr, zz, batch, m0, n0, tid, wm, wn, li, lh);
}

template <void (*Kernel)(GemmArgs)>
void launch_xform(const GemmArgs& a, int batch, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(a.N, 64), (unsigned)cdiv(a.M, 64), (unsigned)(batch * a.splits));
  hipLaunchKernelGGL(Kernel, grid, dim3(256), 0, st, a);
}

}  // namespace a2m
