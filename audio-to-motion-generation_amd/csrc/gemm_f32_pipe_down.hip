// Toom-Cook F(2,2) variant of the software-pipelined 64x64 fp32 tile (gemm_pipe.h) for the 4-tap,
// stride-2, pad-1 conv1d (the UNet's down-sampling convs): no im2col matrix, and two outputs of a
// clip, y[2i] and y[2i + 1], take 6 multiplies per input channel instead of 8.  The conv is two
// 2-tap stride-1 convs, one over the odd input samples and one over the even ones:
//   odd phase:  d = (x[4i - 1], x[4i + 1], x[4i + 3]), taps (g0, g1) = (w0, w2)
//   even phase: d = (x[4i],     x[4i + 2], x[4i + 4]), taps (g0, g1) = (w1, w3)   (x: 0 outside the clip)
//   V0 = d0 - d1, V1 = d1, V2 = d2 - d1                        (input transform, here)
//   U0 = g0, U1 = g0 + g1, U2 = g1                             (a2m_conv1d_down_pack_f32)
//   M_p = sum over both phases and the channels of U_p V_p     (3 GEMMs of 64 x 32 pairs, K = 2 Ci)
//   y[2i] = M0 + M1, y[2i + 1] = M1 + M2                       (output transform, epilogue)
// A 64x64 output tile is 64 rows x 32 pairs = 128 input samples (whole clips: 128 % Tin == 0,
// Tin >= 16).  A 32-channel chunk is six units (plane, phase) of 64 x 32 x 32 and three of
// gemm_pipe.h's k-steps; wave (wm, wn) owns rows wm * 32 .. + 31 and all 32 pairs:
//   step 0: wn = 0 (plane 0, odd)  -> acc0      wn = 1 (plane 2, odd)  -> acc0
//   step 1: wn = 0 (plane 0, even) -> acc0      wn = 1 (plane 2, even) -> acc0
//   step 2: wn = 0 (plane 1, odd)  -> acc1      wn = 1 (plane 1, even) -> acc1
// 48 MFMAs a wave and chunk (64 in the direct tile), two accumulators.
//   A: the packed U, [Co][Ci / 32][6][32] in the order (step, wn) above, read as dense rows of
//      6 Ci (XformRows); a step's tile is its two units' 64 x 32 (stages by k-step parity).
//   B: a thread loads 8 consecutive t (two pairs) of channels kq and kq + 16 plus x[t0 - 1] and
//      x[t0 + 8], transforms them in registers and stores V[unit][pair][36] (pair rows permuted
//      by xform_pair_row).  The plane-0 / plane-2 units are single-buffered: the next
//      chunk's are stored during step 2, which reads plane 1 only; the plane-1 units are stored
//      with them into the stage of the other chunk parity.  The x window of chunk c + 1 is loaded
//      at step 2 of chunk c - 1 and stored at step 2 of chunk c.
// The epilogue writes the planes to LDS (M1 as its two phase halves), every lane rebuilds its
// accumulator of the 64x64 y tile in the MFMA C layout and the tile's existing epilogues run
// unchanged (vec4 / scalar / split-K slab: the transform is linear, so slabs hold outputs and
// splitk_reduce_kernel serves).
// LDS: 2 x 18 KB A stages + 8 x 4.5 KB V units = 72 KB a block (two blocks a CU).
#include "gemm_pipe_xform.h"

namespace a2m {

constexpr int kDownTA = kXformTA;       // an A stage: two units x 64 rows (XformRows)
constexpr int kDownUnit = kXformUnit;   // a V unit: 32 pairs
constexpr int kDownLds = 2 * kDownTA + 8 * kDownUnit;
static_assert(4 * 64 * 32 <= kDownLds, "the M planes reuse the stages");

// B: per chunk and channel half p the thread's x[t0 - 1], x[t0 .. t0 + 7], x[t0 + 8] of channel
// kq + 16 p (t0 = 8 (tid / 16) within the tile's 128 input samples; the two outer elements read 0
// at the clip's edges), transformed into the six units of its two pairs
struct DownX {
  __amdgpu_buffer_rsrc_t rs;
  uint32_t off, offm, offp;   // byte offsets of x[b][next chunk * 32 + kq][t0], [t0 - 1], [t0 + 8] (kPipeOOB: 0)
  int kq, ch, Ci, sk0, v0;
  // row0 / R: the tile's first output column and the output columns (input sample = 2 x column)
  __device__ __forceinline__ void init(const Gather& g, int z, int row0, int R, int CCi, int tid, int c0) {
    rs = pipe_rsrc(g.base + (int64_t)z * g.bstride);
    const int grp = tid >> 4;
    kq = tid & 15;
    const int T = g.Lw;                 // input clip length
    const int n = 2 * row0 + 8 * grp;   // first of the thread's 8 input samples
    const int b = n / T, tt = n - b * T;
    Ci = CCi;
    sk0 = g.sk0;
    ch = c0 + kq;
    const bool valid = n < 2 * R;
    off = valid ? (uint32_t)(b * g.sr0 + tt + ch * sk0) * 4u : kPipeOOB;
    offm = valid && tt > 0 ? off - 4u : kPipeOOB;
    offp = valid && tt + 8 < T ? off + 32u : kPipeOOB;
    v0 = xform_pair_row(2 * grp) * kPipeLDK + kq;
  }
  template <int P>
  __device__ __forceinline__ void load(float (&r)[2][10]) {
    const bool inb = ch + 16 * P < Ci;
    const uint32_t d = 4u * 16 * sk0 * P;
    const float4 lo = pipe_load(rs, inb ? off + d : kPipeOOB);
    const float4 hi = pipe_load(rs, inb ? off + d + 16u : kPipeOOB);
    r[P][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, inb ? offm + d : kPipeOOB, 0, 0));
    r[P][9] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, inb ? offp + d : kPipeOOB, 0, 0));
    r[P][1] = lo.x; r[P][2] = lo.y; r[P][3] = lo.z; r[P][4] = lo.w;
    r[P][5] = hi.x; r[P][6] = hi.y; r[P][7] = hi.z; r[P][8] = hi.w;
    if (P == 1) {
      ch += 32;
      off += 4u * 32 * sk0;
      offm += 4u * 32 * sk0;
      offp += 4u * 32 * sk0;
    }
  }
  // pair J (0 / 1) of half P: units 0 (plane 0, odd), 1 (plane 2, odd), 2 (plane 0, even),
  // 3 (plane 2, even) of `st`, plane 1 odd / even at st1
  template <int P, int J>
  __device__ __forceinline__ void xform_store(float* st, float* st1, const float (&r)[2][10]) const {
    // the pair's x[4i - 1 .. 4i + 4]
    const float xm = r[P][4 * J], x0 = r[P][4 * J + 1], x1 = r[P][4 * J + 2], x2 = r[P][4 * J + 3],
                x3 = r[P][4 * J + 4], xp = r[P][4 * J + 5];
    const int o = v0 + 16 * P + J * kPipeLDK;   // the thread's second pair is the next row
    st[0 * kDownUnit + o] = xm - x1;
    st[1 * kDownUnit + o] = x3 - x1;
    st[2 * kDownUnit + o] = x0 - x2;
    st[3 * kDownUnit + o] = xp - x2;
    st1[o] = x1;
    st1[kDownUnit + o] = x2;
  }
};

__global__ __launch_bounds__(256) void gemm_pipe_kernel_down(GemmArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[kDownLds];
  __shared__ EpiRow epr[64];
  span_begin(args.ts);
  constexpr int BM = 64, BN = 64, LDK = kPipeLDK, TA = kDownTA, U = kDownUnit;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  int bx, by, bz;
  pipe_block<false>(args, bx, by, bz);
  const int zz = bz;
  const int batch = zz / args.splits, split = zz % args.splits;
  const int m0 = by * BM, n0 = bx * BN;
  // args.K and the split bounds are the direct conv's (4 Ci, whole 128-k chunks of 32 channels)
  const int Ci = args.K / 4;
  const int kbeg = split * args.kchunk;
  const int kend = min(args.K, kbeg + args.kchunk);
  const int c0 = kbeg / 128;
  const int nch = __builtin_amdgcn_readfirstlane(kbeg < kend ? (kend - kbeg) / 128 : 0);

  XformRows la;
  la.init(args.A, batch, m0, args.M, 6 * Ci, tid, c0 * 192);
  DownX lx;
  lx.init(args.B, batch, n0, args.N, Ci, tid, c0 * 32);

  float* const As = lds;
  float* const Vs = lds + 2 * TA;        // units 0-3: planes 0 / 2; 4-7: plane 1 [chunk parity][phase]
  const int arow = (wn * 64 + wm * 32 + li) * LDK + lh * 8;   // the wave's unit of a step's A tile
  const int vrow = li * LDK + lh * 8;
  const float* const vb0 = Vs + wn * U + vrow;          // step 0: plane 0 / 2, odd
  const float* const vb1 = Vs + (2 + wn) * U + vrow;    // step 1: plane 0 / 2, even
  floatx16 acc0, acc1;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc0[q] = acc1[q] = 0.f;
  float fa0[8], fb0[8];
  // A tile t is loaded two steps before it is stored (register set t & 1, as in gemm_pipe_body)
  float4 ra[2][4];
  float rx[2][10];
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;

  la.load<0>(ra[0]); la.load<1>(ra[0]); la.load<2>(ra[0]); la.load<3>(ra[0]);
  lx.load<0>(rx); lx.load<1>(rx);
  if (!args.partial && tid < BM && m0 + tid < args.M) epr[tid] = epi_row(args.E, m0 + tid + batch * args.E.pstride);
  la.load<0>(ra[1]); la.load<1>(ra[1]); la.load<2>(ra[1]); la.load<3>(ra[1]);
  la.store<0>(As, ra[0]); la.store<1>(As, ra[0]); la.store<2>(As, ra[0]); la.store<3>(As, ra[0]);
  lx.xform_store<0, 0>(Vs, Vs + 4 * U, rx); lx.xform_store<0, 1>(Vs, Vs + 4 * U, rx);
  lx.xform_store<1, 0>(Vs, Vs + 4 * U, rx); lx.xform_store<1, 1>(Vs, Vs + 4 * U, rx);
  la.load<0>(ra[0]); la.load<1>(ra[0]); la.load<2>(ra[0]); la.load<3>(ra[0]);   // tile 2
  lx.load<0>(rx); lx.load<1>(rx);                                                // chunk 1
  __syncthreads();
  pipe_frag(As + arow, fa0);
  pipe_frag(vb0, fb0);

  // chunk cc (parity P = cc & 1, so tile 3 cc + j has parity (P + j) & 1): step j stores
  // A(3 cc + j + 1) from set (P + j + 1) & 1 and loads A(3 cc + j + 3) into it
  auto chunk = [&](auto par, int cc) {
    constexpr int P = decltype(par)::value;
    constexpr int Q0 = (P + 1) & 1, Q1 = P, Q2 = (P + 1) & 1;
    float* const a0 = As + P * TA;          // stage of tiles 3 cc and 3 cc + 2
    float* const a1 = As + (P ^ 1) * TA;    // stage of tiles 3 cc + 1 and 3 cc + 3
    float* const v1c = Vs + (4 + 2 * P) * U;          // this chunk's plane-1 units
    float* const v1n = Vs + (4 + 2 * (P ^ 1)) * U;    // the next chunk's
    // step 0
    pipe_step(acc0, fa0, fb0, a0 + arow, vb0, a1 + arow, vb1, [&](int s) {
      switch (s) {
        case 0: la.store<0>(a1, ra[Q0]); break;
        case 1: la.store<1>(a1, ra[Q0]); break;
        case 2: la.store<2>(a1, ra[Q0]); break;
        case 3: la.store<3>(a1, ra[Q0]); break;
        case 4: la.load<0>(ra[Q0]); break;
        case 5: la.load<1>(ra[Q0]); break;
        case 6: la.load<2>(ra[Q0]); break;
        default: la.load<3>(ra[Q0]); break;
      }
    });
    // step 1
    pipe_step(acc0, fa0, fb0, a1 + arow, vb1, a0 + arow, v1c + wn * U + vrow, [&](int s) {
      switch (s) {
        case 0: la.store<0>(a0, ra[Q1]); break;
        case 1: la.store<1>(a0, ra[Q1]); break;
        case 2: la.store<2>(a0, ra[Q1]); break;
        case 3: la.store<3>(a0, ra[Q1]); break;
        case 4: la.load<0>(ra[Q1]); break;
        case 5: la.load<1>(ra[Q1]); break;
        case 6: la.load<2>(ra[Q1]); break;
        default: la.load<3>(ra[Q1]); break;
      }
    });
    // step 2 (+ the next chunk's V stores: planes 0 / 2 in place, plane 1 into the other parity;
    // then the x window loads of the chunk after it, three k-steps before their stores)
    pipe_step(acc1, fa0, fb0, a0 + arow, v1c + wn * U + vrow, a1 + arow, vb0, [&](int s) {
      switch (s) {
        case 0: la.store<0>(a1, ra[Q2]); la.store<1>(a1, ra[Q2]); break;
        case 1: la.store<2>(a1, ra[Q2]); la.store<3>(a1, ra[Q2]); break;
        case 2: lx.xform_store<0, 0>(Vs, v1n, rx); la.load<0>(ra[Q2]); break;
        case 3: lx.xform_store<0, 1>(Vs, v1n, rx); la.load<1>(ra[Q2]); break;
        case 4: lx.xform_store<1, 0>(Vs, v1n, rx); la.load<2>(ra[Q2]); break;
        case 5: lx.xform_store<1, 1>(Vs, v1n, rx); la.load<3>(ra[Q2]); break;
        case 6: lx.load<0>(rx); break;
        default: lx.load<1>(rx); break;
      }
    });
  };
  int cc = 0;
  for (; cc + 1 < nch; cc += 2) {
    chunk(P0(), cc);
    chunk(P1(), cc + 1);
  }
  if (cc < nch) chunk(P0(), cc);

  // M planes [plane][row][pair]: 0 = M0, 1 = M1's odd-phase half, 2 = M1's even-phase half, 3 = M2;
  // y[2i] = M0 + M1, y[2i + 1] = M2 + M1 (Me: M2 odd, M0 even)
  xform_epilogue(args, lds, epr, acc0, 3 * wn, acc1, 1 + wn,
                 [](float M1o, float M1e, float Me, bool) { return Me + (M1o + M1e); },
                 zz, batch, m0, n0, tid, wm, wn, li, lh);
  span_end(args.ts);
}

void launch_pipe_down(const GemmArgs& a, int batch, hipStream_t st) { launch_xform<gemm_pipe_kernel_down>(a, batch, st); }

}  // namespace a2m
