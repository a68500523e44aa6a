// Winograd F(2,3) variant of the software-pipelined 64x64 fp32 tile (gemm_pipe.h) for the 3-tap,
// pad-1, stride-1 conv1d of the halo layout's problem class (clips of T >= 16 that tile the 64
// rows, Ci % 32 == 0).  Two outputs of a clip, y[2i] and y[2i + 1], take 4 multiplies per input
// channel instead of 6:
//   d = x[2i - 1 .. 2i + 2] (zero outside the clip)
//   V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3            (input transform, here)
//   U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2 (a2m_conv1d_wino_pack_f32)
//   M_p = sum_c U_p[co][c] V_p[c][i]                                   (4 GEMMs of 64 x 32 pairs)
//   y[2i] = M0 + M1 + M2, y[2i + 1] = M1 - M2 - M3                     (output transform, epilogue)
// A 64x64 output tile is 64 rows x 32 pairs x 4 points.  Wave (wm, wn) owns rows wm * 32 .. + 31,
// all 32 pairs and the points wn and wn + 2: two accumulators, 32 MFMAs per 32-channel chunk (48
// in the direct tile).  A chunk is two of gemm_pipe.h's k-steps (pipe_step): step 0 multiplies
// points 0 / 1 into the waves' first accumulators, step 1 points 2 / 3 into their second.
//   A: the packed U, [Co][Ci / 32][4][32], read as dense rows of 4 Ci (XformRows); a step's tile is
//      two points' 64 x 32 (stages by step parity, [point][row][36]).
//   B: the chunk's x window is loaded once per thread as in the halo layout (4 consecutive t =
//      two pairs of channels kq and kq + 16) plus x[t0 - 1] and x[t0 + 4], transformed in registers
//      and stored as V[point][pair][36] (stages by chunk parity).  Pair i is stored at row
//      xform_pair_row(i) (gemm_pipe_xform.h), which keeps the 32 lanes of a ds_write_b32 on distinct
//      banks; lane li of a fragment read takes row li, so it computes pair xform_pair_row(li) (an
//      involution).
// The operand work sits in the MFMA shadows in pipe_step's slices.  The epilogue writes the four
// M planes to LDS, every lane rebuilds its accumulator of the 64x64 y tile in the MFMA C layout
// and the tile's existing epilogues run unchanged (vec4 / scalar / m-contiguous / split-K slab:
// the transform is linear, so slabs hold transformed outputs and splitk_reduce_kernel serves).
// LDS: 2 x 18 KB A stages + 2 x 18 KB V stages = 72 KB a block (two blocks a CU).
#include "gemm_pipe_xform.h"

namespace a2m {

constexpr int kWinoTA = kXformTA;        // an A stage: two points x 64 rows (XformRows)
constexpr int kWinoPlane = kXformUnit;   // one point of a V stage: 32 pairs
constexpr int kWinoTV = 4 * kWinoPlane;
constexpr int kWinoLds = 2 * kWinoTA + 2 * kWinoTV;
static_assert(4 * 64 * 32 <= kWinoLds, "the M planes reuse the stages");

// B: per chunk and channel half p the thread's x[t0 - 1], x[t0 .. t0 + 3], x[t0 + 4] of channel
// kq + 16 p (t0 = the first of its 4 rows within the clip; the two outer elements read 0 at the
// clip's edges), transformed into the 4 points of its two pairs
struct WinoX {
  __amdgpu_buffer_rsrc_t rs;
  uint32_t off, offm, offp;   // byte offsets of x[b][next chunk * 32 + kq][t0], [t0 - 1], [t0 + 4] (kPipeOOB: 0)
  int kq, ch, Ci, sk0, v0;
  __device__ __forceinline__ void init(const Gather& g, int z, int row0, int R, int CCi, int tid, int c0) {
    rs = pipe_rsrc(g.base + (int64_t)z * g.bstride);
    const int lrow = (tid >> 4) * 4;
    kq = tid & 15;
    const int T = g.R2;
    const int n = row0 + lrow;
    const int b = n / T, tt = n - b * T;
    Ci = CCi;
    sk0 = g.sk0;
    ch = c0 + kq;
    const bool valid = n < R;
    off = valid ? (uint32_t)(b * g.sr0 + tt + ch * sk0) * 4u : kPipeOOB;
    offm = valid && tt > 0 ? off - 4u : kPipeOOB;
    offp = valid && tt + 4 < T ? off + 16u : kPipeOOB;
    v0 = xform_pair_row(lrow >> 1) * kPipeLDK + kq;
  }
  template <int P>
  __device__ __forceinline__ void load(float (&r)[2][6]) {
    const bool inb = ch + 16 * P < Ci;
    const uint32_t d = 4u * 16 * sk0 * P;
    const float4 v = pipe_load(rs, inb ? off + d : kPipeOOB);
    r[P][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, inb ? offm + d : kPipeOOB, 0, 0));
    r[P][5] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, inb ? offp + d : kPipeOOB, 0, 0));
    r[P][1] = v.x; r[P][2] = v.y; r[P][3] = v.z; r[P][4] = v.w;
    if (P == 1) {
      ch += 32;
      off += 4u * 32 * sk0;
      offm += 4u * 32 * sk0;
      offp += 4u * 32 * sk0;
    }
  }
  template <int P>
  __device__ __forceinline__ void xform_store(float* st, const float (&r)[2][6]) const {
    const float xm = r[P][0], x0 = r[P][1], x1 = r[P][2], x2 = r[P][3], x3 = r[P][4], xp = r[P][5];
    float* const q = st + v0 + 16 * P;   // the thread's first pair; its second is the next row
    q[0 * kWinoPlane] = xm - x1;
    q[0 * kWinoPlane + kPipeLDK] = x1 - x3;
    q[1 * kWinoPlane] = x0 + x1;
    q[1 * kWinoPlane + kPipeLDK] = x2 + x3;
    q[2 * kWinoPlane] = x1 - x0;
    q[2 * kWinoPlane + kPipeLDK] = x3 - x2;
    q[3 * kWinoPlane] = x0 - x2;
    q[3 * kWinoPlane + kPipeLDK] = x2 - xp;
  }
};

__global__ __launch_bounds__(256) void gemm_pipe_kernel_wino(GemmArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[kWinoLds];
  __shared__ EpiRow epr[64];
  span_begin(args.ts);
  constexpr int BM = 64, BN = 64, LDK = kPipeLDK, TA = kWinoTA, TV = kWinoTV;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  int bx, by, bz;
  pipe_block<false>(args, bx, by, bz);
  const int zz = bz;
  const int batch = zz / args.splits, split = zz % args.splits;
  const int m0 = by * BM, n0 = bx * BN;
  // args.K and the split bounds are the direct conv's (3 Ci, whole 96-k chunks of 32 channels)
  const int Ci = args.K / 3;
  const int kbeg = split * args.kchunk;
  const int kend = min(args.K, kbeg + args.kchunk);
  const int c0 = kbeg / 96;
  const int nch = __builtin_amdgcn_readfirstlane(kbeg < kend ? (kend - kbeg) / 96 : 0);

  XformRows la;
  la.init(args.A, batch, m0, args.M, 4 * Ci, tid, c0 * 128);
  WinoX lx;
  lx.init(args.B, batch, n0, args.N, Ci, tid, c0 * 32);

  float* const As = lds;
  float* const Vs = lds + 2 * TA;
  const int arow = (wn * 64 + wm * 32 + li) * LDK + lh * 8;   // the wave's point of a step's A tile
  const int brow0 = (wn * 32 + li) * LDK + lh * 8;            // point wn (step 0)
  const int brow1 = brow0 + 2 * kWinoPlane;                   // point wn + 2 (step 1)
  floatx16 acc0, acc1;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc0[q] = acc1[q] = 0.f;
  float fa0[8], fb0[8];
  // A tile t is loaded two steps before it is stored (register set t & 1, as in gemm_pipe_body);
  // the x window of chunk c is loaded at step 1 of chunk c - 2 and stored at step 1 of chunk c - 1
  float4 ra[2][4];
  float rx[2][6];

  la.load<0>(ra[0]); la.load<1>(ra[0]); la.load<2>(ra[0]); la.load<3>(ra[0]);
  lx.load<0>(rx); lx.load<1>(rx);
  if (!args.partial && tid < BM && m0 + tid < args.M) epr[tid] = epi_row(args.E, m0 + tid + batch * args.E.pstride);
  la.load<0>(ra[1]); la.load<1>(ra[1]); la.load<2>(ra[1]); la.load<3>(ra[1]);
  la.store<0>(As, ra[0]); la.store<1>(As, ra[0]); la.store<2>(As, ra[0]); la.store<3>(As, ra[0]);
  lx.xform_store<0>(Vs, rx); lx.xform_store<1>(Vs, rx);
  la.load<0>(ra[0]); la.load<1>(ra[0]); la.load<2>(ra[0]); la.load<3>(ra[0]);   // tile 2
  lx.load<0>(rx); lx.load<1>(rx);                                                // chunk 1
  __syncthreads();
  pipe_frag(As + arow, fa0);
  pipe_frag(Vs + brow0, fb0);

  for (int cc = 0; cc < nch; ++cc) {
    float* const vc = Vs + (cc & 1) * TV;          // this chunk's V stage
    float* const vn = Vs + ((cc & 1) ^ 1) * TV;    // the next chunk's
    // step 0 (tile 2 cc, A stage 0): stores tile 2 cc + 1 from set 1, loads tile 2 cc + 3 into it
    pipe_step(acc0, fa0, fb0, As + arow, vc + brow0, As + TA + arow, vc + brow1, [&](int s) {
      switch (s) {
        case 0: la.store<0>(As + TA, ra[1]); break;
        case 1: la.store<1>(As + TA, ra[1]); break;
        case 2: la.store<2>(As + TA, ra[1]); break;
        case 3: la.store<3>(As + TA, ra[1]); break;
        case 4: la.load<0>(ra[1]); break;
        case 5: la.load<1>(ra[1]); break;
        case 6: la.load<2>(ra[1]); break;
        default: la.load<3>(ra[1]); break;
      }
    });
    // step 1 (tile 2 cc + 1, A stage 1): stores tile 2 cc + 2 from set 0 and the V of chunk cc + 1,
    // loads tile 2 cc + 4 into set 0 and the x window of chunk cc + 2
    pipe_step(acc1, fa0, fb0, As + TA + arow, vc + brow1, As + arow, vn + brow0, [&](int s) {
      switch (s) {
        case 0: la.store<0>(As, ra[0]); la.store<1>(As, ra[0]); break;
        case 1: la.store<2>(As, ra[0]); la.store<3>(As, ra[0]); break;
        case 2: lx.xform_store<0>(vn, rx); break;
        case 3: lx.xform_store<1>(vn, rx); break;
        case 4: la.load<0>(ra[0]); la.load<1>(ra[0]); break;
        case 5: la.load<2>(ra[0]); la.load<3>(ra[0]); break;
        case 6: lx.load<0>(rx); break;
        default: lx.load<1>(rx); break;
      }
    });
  }

  // M planes [point][row][pair]: y[2i] = M0 + M1 + M2, y[2i + 1] = M1 - M2 - M3 (Me: M3 odd, M0 even)
  xform_epilogue(args, lds, epr, acc0, wn, acc1, wn + 2,
                 [](float M1, float M2, float Me, bool odd) { return odd ? (M1 - M2) - Me : (Me + M1) + M2; },
                 zz, batch, m0, n0, tid, wm, wn, li, lh);
  span_end(args.ts);
}

void launch_pipe_wino(const GemmArgs& a, int batch, hipStream_t st) { launch_xform<gemm_pipe_kernel_wino>(a, batch, st); }

}  // namespace a2m
