// Implicit-GEMM engine: the launch decision (operand modes, planner, kernel selection) as a pure
// function of the operands and the process-wide switches.  gemm.hip launches what it returns.
#include "gemm_route.h"

#include <algorithm>
#include <cassert>
#include <cstdlib>
#include <vector>

namespace a2m {

static int operand_mode(const Gather& g, int K) {
  if (g.tapconv > 0) return 5;
  if (g.nhwc > 0) return 6;
  if (!g.kcontig) {
    // rows 4-at-a-time contiguous: plain [K][R] (rows via r0, unit stride), or stride-1 im2col
    // rows along w (R2 % 4 == 0) or along h (R2 == 1, R1 % 4 == 0), unit element stride
    const bool plain = g.R1 == 1 && g.R2 == 1 && g.sr0 == 1;
    const bool along_w = g.R2 > 1 && g.R2 % 4 == 0 && (g.ar2 == 1 || g.ar2 == 2) && g.sw == 1 &&
                         g.divw == 1;
    const bool along_h = g.R2 == 1 && g.R1 > 1 && g.R1 % 4 == 0 && (g.ar1 == 1 || g.ar1 == 2) &&
                         g.sh == 1 && g.divh == 1;
    return plain || along_w || along_h ? 3 : 2;
  }
  const bool dense = g.K1 == 1 && g.K2 == 1 && g.sk0 == 1 && g.Lh == 1 && g.Lw == 1 &&
                     g.sh == 0 && g.sw == 0 && g.ch == 0 && g.cw == 0 && g.divh == 1 && g.divw == 1;
  const bool aligned = (reinterpret_cast<uintptr_t>(g.base) % 16 == 0) && (g.sr0 % 4 == 0) &&
                       (g.bstride % 4 == 0) && (K % 4 == 0);
  if (dense && aligned) return 0;
  const bool runs = g.K2 % 4 == 0 && g.bk2 == 1 && g.sw == 1 && g.divw == 1;
  return runs ? 4 : 1;
}

struct Plan {
  int bm, bk, splits, kchunk;
};

// fixed cost of a split-K reduce launch in the planner's model (us)
#ifndef A2M_RED_FIXED_US
#define A2M_RED_FIXED_US 3.0
#endif
#ifndef A2M_RED_FIXED_US_BF16
#define A2M_RED_FIXED_US_BF16 6.0
#endif

// Tile / split-K choice by a cost model fitted to measured sweeps of the engine on MI355X
// (tools/gemm_tune.py; DESIGN.md "GEMM planner").  For each candidate (tile, splits):
//   blocks = tiles * splits, per_cu = ceil(blocks / 256) (the busiest CU), c = min(per_cu,
//   resident blocks per CU: 4 at 64x64, 2 at 128x128 -- LDS-bound),
//   t = per_cu * block_flops / thr(tile, c) + ceil(per_cu / occ) * t_fixed(tile) + t_launch
//       + (splits > 1 ? (splits + 1) * M * N * 4 B / 3.5 TB/s + 3 us : 0)   (the slab reduce)
// thr is the per-CU fp32 MFMA throughput measured at c co-resident blocks; a row-gathered
// operand (modes 2/3: transposed LDS staging) costs the 64x64 tile ~16 % of throughput and
// the 128x128 tile ~6 us more per round of blocks.  The model is
// deterministic in (M, N, K, batch, gathered), so a shape always gets the same plan and the
// same (bitwise-reproducible) split order.  a2m_gemm_plan_override and A2M_GEMM_PLAN_RULES
// (per-shape "M,N,K:tile:splits;...") override it (experiments).
// Operand precision of the engine: 0 = fp32 (v_mfma_f32_32x32x2_f32, BK 32; the default and
// the parity configuration), 1 = bf16 (operands rounded to bf16 in LDS, fp32 accumulation,
// BK 64; a2m_set_gemm_precision, configs[4]), 2 = bf16x6 (fp32 operands split exactly into
// three bf16 planes in LDS, the six products of order >= 2^-16 on v_mfma_f32_32x32x16_bf16 with
// fp32 accumulation: fp32-class accuracy at 16/6 of the f32 MFMA rate; BK 32).
// (BK = 16 measured slower end to end.)
// (fp32 at BK = 64 -- fewer barriers per MFMA -- measured 10-20 % slower on every G shape:
// the k-loop's non-MFMA cost scales with the staged bytes, not with the barrier count;
// profiles/r02_gemm_ablation.txt)
int gemm_bk(int prec) { return prec == 1 ? 64 : 32; }

struct PlanRule {
  int M, N, K, tile, splits;
};
static const PlanRule* plan_rule(int M, int N, int K) {
  static const std::vector<PlanRule> rules = [] {
    std::vector<PlanRule> v;
    const char* e = std::getenv("A2M_GEMM_PLAN_RULES");
    while (e && *e) {
      PlanRule r{};
      int used = 0;
      if (std::sscanf(e, "%d,%d,%d:%d:%d%n", &r.M, &r.N, &r.K, &r.tile, &r.splits, &used) != 5) break;
      if ((r.tile == 0 || r.tile == 64 || r.tile == 128) && r.splits >= 0 && r.splits <= 256) v.push_back(r);
      else std::fprintf(stderr, "a2m: A2M_GEMM_PLAN_RULES entry %d,%d,%d:%d:%d ignored (tile 0/64/128, splits 0..256)\n",
                        r.M, r.N, r.K, r.tile, r.splits);
      e += used;
      while (*e == ';' || *e == ' ') ++e;
    }
    return v;
  }();
  for (const PlanRule& r : rules)
    if (r.M == M && r.N == N && r.K == K) return &r;
  return nullptr;
}

bool plan_rule_splits(int M, int N, int K) {
  const PlanRule* r = plan_rule(M, N, K);
  return r && r->splits > 1;
}

// (Rounds 4-5 kept a table of seven fp32 plans tuned in the replayed bench step -- 64x64 tiles
// with 2 splits on the UNet's large tap convs, 1 split on the hand stack's proj_out.  With the
// round-6 kernels the planner's own choices measured faster: 2.245 vs 2.228 ms and 2.473 vs
// 2.448 ms, three interleaved rounds on each of two boxes, training neutral
// (profiles/r06_r_tuned_plans_ab.txt); the table is gone.)

// bf16 (prec 1) throughput per CU by resident blocks, flop / us: staging- and latency-bound
// rather than MFMA-bound (16x the f32 MFMA rate), so it grows with the blocks a CU holds far more
// than the f32 tile's (kflop / us per CU by resident blocks: 64x64 at 1..4, 128x128 at 1 / 2)
static double bf16_thr(int tile, int c) {
  // fitted in the replayed bf16 bench step (r05 sweeps, two interleaved rounds each: 1.658 ms
  // against 1.831 ms with round 4's 4 x the f32 table, {1360, 1712, 1740, 1760, 1856, 2000}e3,
  // at {530, 750, 900, 1060, 1500, 2000}e3; refitted with the bf16 pipelined tile, whose 64x64
  // launches run faster: 1.416-1.422 ms against 1.447-1.449)
  static constexpr double t[6] = {600e3, 850e3, 1000e3, 1150e3, 1500e3, 2000e3};
  return tile == 128 ? t[4 + (c > 1)] : t[std::min(std::max(c, 1), 4) - 1];
}

static double plan_cost_us(int M, int N, int K, int batch, bool gathered, int tile, int kchunk,
                           int splits, int prec, bool conv_rows = false) {
  static const double thr64[4] = {340e3, 428e3, 435e3, 440e3};   // flop / us per CU
  static const double thr128[2] = {464e3, 500e3};
  // bf16x6 (fitted to a plan sweep of the G forward's shapes, tools/sweep_summary.py): three
  // bf16 planes per operand halve the resident blocks (LDS: 61 KB at 64x64, 120 KB at
  // 128x128) and the 128x128 tile gains most from the faster MFMA
  static const double x6_thr64[2] = {272e3, 342e3};
  static const double x6_thr128[1] = {557e3};
  const int occ = prec == 2 ? (tile == 128 ? 1 : 2) : (tile == 128 ? 2 : 4);
  const int64_t tiles = cdiv(M, tile) * cdiv(N, tile) * (int64_t)batch;
  const int64_t per_cu = cdiv(tiles * splits, 256);
  const int c = (int)std::min<int64_t>(per_cu, occ);
  double thr = prec == 2 ? (tile == 128 ? x6_thr128[c - 1] : x6_thr64[c - 1])
                         : (tile == 128 ? thr128[c - 1] : thr64[c - 1]);
#ifndef A2M_THR64_SCALE
#define A2M_THR64_SCALE 1.0   // diagnostic: the 64x64 tile's fitted throughput scaled
#endif
#ifndef A2M_GATHER_F
#define A2M_GATHER_F 0.84
#endif
  if (prec == 0 && tile == 64) thr *= A2M_THR64_SCALE;
  if (gathered && tile == 64) thr *= A2M_GATHER_F;
  // (channels-last conv rows, mode 6, run at the dense fit on the one-group 64x64 tile: a 0.87
  // factor measured slower, encoder 303.2 vs 300.0 us, tools/enc_plan_ab.py, round 3)
#ifndef A2M_BF16_THR128_SCALE
#define A2M_BF16_THR128_SCALE 1.0   // diagnostic: the bf16 128x128 tile's fitted throughput scaled
#endif
  if (prec == 1) thr = bf16_thr(tile, c) * (gathered && tile == 64 ? 0.84 : 1.0) * (tile == 128 ? A2M_BF16_THR128_SCALE : 1.0);
  const double block_flops = 2.0 * tile * tile * (double)kchunk;
  const double fixed = prec == 2 ? (tile == 128 ? 15.0 : 2.0)
                                 : (tile == 128 ? (gathered ? 16.0 : 10.0) : 3.0);
  double t = per_cu * block_flops / thr + cdiv(per_cu, occ) * fixed + 4.0;
  // (the reduce term scaled by 0.6 / 1.5 / 2 measured slower in-step, round 2: it is right as fitted)
  constexpr double red_scale = 1.0;
  // channels-last conv rows (the encoder): the reduce priced at A2M_GEMM_SPLIT_COST_ROWS
  // (default 200 %), so its launches take fewer splits (conv2: 3 instead of 4).  With every
  // launch's reduce at 200 % the encoder measured 0.2906-0.2937 vs 0.2951-0.2971 ms but the step
  // neutral to slightly slower (three rounds); on the encoder's launches only: in-step
  // path_frac 0.480-0.484 vs 0.473-0.476, step 2.718-2.727 vs 2.721-2.737 ms (four rounds, r04s)
#ifndef A2M_RED_SCALE_ROWS
#define A2M_RED_SCALE_ROWS 2.0
#endif
  constexpr double red_scale_rows = A2M_RED_SCALE_ROWS;
  if (splits > 1)
    t += (conv_rows ? red_scale_rows : red_scale) *
         ((splits + 1.0) * M * N * (double)batch * 4.0 / 3.5e6 + (prec == 1 ? A2M_RED_FIXED_US_BF16 : A2M_RED_FIXED_US));
  return t;
}

// force_tile / force_split: a2m_gemm_plan_override (tuning sweeps)
static Plan plan_for(int M, int N, int K, int batch, bool gathered, int prec, int kquant, bool conv_rows,
                     bool pipe64, int force_tile, int force_split) {
  const int BK = gemm_bk(prec);
  const int KQ = BK * kquant;   // split boundaries on whole k-tile groups (mode 5: all taps of a chunk)
  static const int cand_splits[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256};
  Plan p{64, BK, 1, (int)(cdiv(std::max(K, 1), KQ) * KQ)};
  double best = 1e300;
  for (int tile : {64, 128}) {
    if (force_tile && tile != force_tile) continue;
    // operands the fp32 pipelined 64x64 tile takes: the cost table is gemm_tile's, which the
    // pipelined tile outruns -- kept to 64 (training iteration 66.0 -> 64.5 ms, r05_n)
    if (!force_tile && pipe64 && tile != 64) continue;
    for (int s : cand_splits) {
      if (force_split && s != force_split) continue;
      const int kchunk = (int)(cdiv(cdiv(std::max(K, 1), s), KQ) * KQ);
      const int se = (int)cdiv(std::max(K, 1), kchunk);
      if (!force_split && se > 1 && kchunk < 128) continue;
      if (se != s && s > 1 && !force_split) continue;   // the same plan at a smaller s
      const double t = plan_cost_us(M, N, K, batch, gathered, tile, kchunk, se, prec, conv_rows);
      if (t < best) {
        best = t;
        p.bm = tile;
        p.kchunk = kchunk;
        p.splits = se;
      }
    }
  }
  if (force_split && best == 1e300) {   // a forced split outside the candidate list
    p.bm = force_tile ? force_tile : 64;
    p.kchunk = (int)(cdiv(cdiv(std::max(K, 1), force_split), KQ) * KQ);
    p.splits = (int)cdiv(std::max(K, 1), p.kchunk);
  }
  return p;
}

// the plan gemm() launches: the planner's, unless an A2M_GEMM_PLAN_RULES rule fixes the tile /
// split count for the shape.  kchunk is always a whole number of k-tile groups (bk * kquant).
static Plan launch_plan(int M, int N, int K, int batch, bool gathered, int prec, int kquant, bool rows6,
                        int force_split, bool pipe64, const RouteConfig& cfg) {
  Plan p = plan_for(M, N, K, batch, gathered, prec, kquant, rows6, pipe64, cfg.override_tile, cfg.override_split);
  if (force_split > 0) {
    p.kchunk = (int)(cdiv(cdiv(K, force_split), p.bk * kquant) * p.bk * kquant);
    p.splits = (int)cdiv(K, p.kchunk);
  }
  if (const PlanRule* r = plan_rule(M, N, K)) {
    if (r->tile) p.bm = r->tile;
    if (r->splits > 0) {
      p.kchunk = (int)(cdiv(cdiv(K, r->splits), p.bk * kquant) * p.bk * kquant);
      p.splits = (int)cdiv(K, p.kchunk);
    }
  }
  if (K == 0) { p.splits = 1; p.kchunk = p.bk; }
  return p;
}

void route_out(const GemmRoute& r, int32_t out[8]) {
  const int32_t o[8] = {r.kind, r.tile, r.bk, r.splits, r.kchunk, r.ma, r.mb,
                        (r.vec4 ? 1 : 0) | (r.mcontig ? 2 : 0) | (r.halo ? 4 : 0) | (r.reduce ? 8 : 0) |
                            (r.xform == XFORM_WINO ? 16 : 0) | (r.xform == XFORM_DOWN ? 32 : 0)};
  for (int i = 0; i < 8; ++i) out[i] = o[i];
}

size_t split_ws_bytes(const GemmRoute& r, int M, int N, int batch) {
  return (size_t)r.splits * batch * M * (size_t)N * sizeof(float);
}

size_t gemm_ws_bytes(int M, int N, int K, int batch, const RouteConfig& cfg) {
  // every plan gemm() may launch for the shape: either operand orientation (the plan depends on
  // whether an operand is row-gathered), either precision, conv rows or not, the tap-chunk
  // quantum of a tap-chunked conv (1-3 taps), and the tuned / rule overrides
  size_t need = 0;
  for (bool gathered : {false, true})
    for (int prec : {0, 1, 2})
      for (bool rows6 : {false, true})
        for (int kq : {1, 2, 3})
          for (bool p64 : {false, true}) {
            const Plan p = launch_plan(M, N, K, batch, gathered, prec, kq, rows6, 0, p64, cfg);
            if (p.splits > 1) need = std::max(need, (size_t)p.splits * batch * M * (size_t)N * sizeof(float));
          }
  return need;
}

// raw buffer loads of the pipelined tiles: every element offset below 2^29 floats
static bool pipe_below(int64_t v) { return v >= 0 && v < ((int64_t)1 << 29); }

// mode 5 as the fp32 pipelined tile takes it (at a 64-row tile): 1-3 taps over clips that tile the 64 rows
static bool pipe_tap5(const Gather& B, int mb) {
  return mb == 5 && B.tapconv >= 1 && B.tapconv <= 3 && B.R2 % 4 == 0 && 64 % B.R2 == 0;
}

// float4 output rows (pipelined tile): n contiguous within 4-aligned groups of one n2 run, every
// other stride and base 16-byte aligned; split-K slabs ([M][N]) whenever N % 4 == 0
static bool epi_vec4(const Epilogue& E, int N, bool mcontig, bool slab_out) {
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  // the innermost index that varies with n: n2 (N2 > 1), else n1 (N1 > 1), else n0
  const int in_lvl = E.N2 > 1 ? 2 : (E.N1 > 1 ? 1 : 0);
  const int in_stride = in_lvl == 2 ? E.so2 : (in_lvl == 1 ? E.so1 : E.so0);
  const int in_len = in_lvl == 2 ? E.N2 : (in_lvl == 1 ? E.N1 : 4);
  const bool outer4 = (in_lvl == 0 || E.so0 % 4 == 0) && (in_lvl != 2 || E.N1 == 1 || E.so1 % 4 == 0) &&
                      E.som % 4 == 0 && E.bstride % 4 == 0;
  return !mcontig && N % 4 == 0 &&
         (slab_out || (in_stride == 1 && in_len % 4 == 0 && outer4 && al16(E.out) &&
                       (!E.res1 || al16(E.res1)) && (!E.res2 || al16(E.res2))));
}

// The pipelined 64x64 tiles' (gemm_pipe.h, gemm_pipe_bf16.h) template arguments <MB, NT, MA> for
// the operand modes they take at a 64-row tile; taken = false for every other pair of operands.
// NT (the per-tap layout's tap count, mode 5) is filled in once the halo layout is decided.
struct PipeOperands {
  bool taken;
  bool training;   // mode-4 / plain mode-3 A (the weight gradients)
  int mb, ma;
};

// software-pipelined one-wave-per-SIMD tile (gemm_pipe.h; a2m_gemm_pipe_override(0) restores
// gemm_tile): 64x64, dense weights x dense rows / channels-last rows / tap conv, every
// element offset below 2^29 floats (raw buffer loads)
static PipeOperands pipe_operands(const Gather& A, const Gather& B, int ma, int mb, int M, int N, int K) {
  auto below = pipe_below;
  bool pipe_ext = below((int64_t)(M - 1) * A.sr0 + K);
  if (mb == 0) pipe_ext = pipe_ext && below((int64_t)(N - 1) * B.sr0 + K);
  else if (mb == 6) pipe_ext = pipe_ext && below((int64_t)((N - 1) / (B.R1 * B.R2)) * B.sr0 + (int64_t)B.Lh * B.Lw * B.nhwc);
  else if (mb == 5) pipe_ext = pipe_ext && below((int64_t)((N - 1) / B.R2) * B.sr0 + B.R2 + (int64_t)(K / B.tapconv) * B.sk0);
  else if (mb == 3) pipe_ext = pipe_ext && below((int64_t)((N - 1) / B.R2) * B.sr0 + B.R2 + (int64_t)K * B.sk0);
  // mode 3 in its plain form only: k = channel, rows (b, t) at unit stride in groups of 4
  const bool rows3 = mb == 3 && B.K1 == 1 && B.K2 == 1 && B.R1 == 1 && B.ch == 0 && B.cw == 0 &&
                     B.divh == 1 && B.divw == 1 && N % 4 == 0 &&
                     ((B.R2 == 1 && B.sr0 == 1) || (B.R2 % 4 == 0 && B.ar2 == 1 && B.sw == 1 && B.Lw >= B.R2));
  // mode 4 on both sides (the 1-D conv weight gradients): one k digit (K1 = 1) in runs of a
  // multiple of 4, every split a whole number of k-tiles, offsets below 2^29
  auto runs4 = [&](const Gather& g, int R) {
    const int64_t rmax = (int64_t)((R - 1) / (g.R1 * g.R2)) * g.sr0 +
                         (int64_t)std::max(0, g.Lh - 1) * std::abs(g.sh) + g.Lw + (int64_t)(K / g.K2) * g.sk0;
    return g.K1 == 1 && g.K2 % 4 == 0 && g.bk2 == 1 && g.sw == 1 && g.divh == 1 && g.divw == 1 &&
           g.sr0 >= 0 && g.sk0 >= 0 && below(rmax);
  };
  // ... and B as stride-2 runs (a stride-2 conv's input: gemm_tile gathers it, mode 1); the
  // pipelined kernels load them as their B mode 7
  const bool runs_s2 = mb == 1 && B.K1 == 1 && B.K2 % 4 == 0 && B.bk2 == 2 && B.sw == 1 && B.divh == 1 &&
                       B.divw == 1 && B.sr0 >= 0 && B.sk0 >= 0 &&
                       below((int64_t)((N - 1) / (B.R1 * B.R2)) * B.sr0 + (int64_t)std::max(0, B.Lh - 1) * std::abs(B.sh) +
                             B.Lw + (int64_t)(K / B.K2) * B.sk0);
  const bool m4_ok = ma == 4 && runs4(A, M) && ((mb == 4 && runs4(B, N)) || runs_s2);
  if (m4_ok) return {true, true, runs_s2 ? 7 : 4, 4};
  // A as a plain [K][M] operand (mode 3: rows at unit stride, loaded 4 at a time) with B dense or
  // plain mode 3 (the weight gradients of the linears / graph layers)
  const bool plainA3 = ma == 3 && A.K1 == 1 && A.K2 == 1 && A.R1 == 1 && A.R2 == 1 && A.sr0 == 1 && A.ch == 0 &&
                       A.cw == 0 && A.divh == 1 && A.divw == 1 && M % 4 == 0 && A.sk0 >= 0 &&
                       below((int64_t)(M - 1) + (int64_t)K * A.sk0);
  const bool pipe_a3 = plainA3 &&
                       ((mb == 0 && below((int64_t)(N - 1) * B.sr0 + K)) ||
                        (rows3 && below((int64_t)((N - 1) / B.R2) * B.sr0 + B.R2 + (int64_t)K * B.sk0)));
  if (pipe_a3) return {true, true, mb, 3};
  // dense A with the inference operands
  if (ma == 0 && (mb == 0 || mb == 6 || rows3 || pipe_tap5(B, mb)) && pipe_ext) return {true, false, mb, 0};
  return {false, false, 0, 0};
}

// Shape classes of requested, eligible launches that stay on the route without the request because
// it measured faster there: blocks = 64x64 tiles x batch of the launch (before split-K), K the
// direct conv's.  A launch outside every class of its tile's table takes the tile.
struct DirectRule {
  int64_t min_blocks, max_blocks;
  int min_k, max_k;
};
// Winograd (K = 3 Ci) against the direct tap tile.  The table is empty: all six shapes of the bench
// step measured faster on the Winograd tile, alone and in the step's kernel trace -- the UNet's
// five (512-1024 blocks, K 768-6144) by 9-19 %, the decoders' one-block-per-CU launch (256 blocks,
// K 768) by 5 % alone and 11 % in the trace (profiles/wino_conv.txt).
static const std::vector<DirectRule> kWinoDirect = {};
// down-sampling (K = 4 Ci) against the im2col route (im2col1d_kernel and the dense tile).  The
// table is empty: both shapes of the bench step measured faster on the down-sampling tile, alone
// and in the step's kernel trace (profiles/down_conv.txt).
static const std::vector<DirectRule> kDownDirect = {};
bool xform_rule(Xform xform, int M, int N, int K, int batch) {
  const int64_t blocks = cdiv(M, 64) * cdiv(N, 64) * (int64_t)batch;
  // experiments: Winograd launches of fewer blocks stay on the direct tile (read once, like A2M_GEMM_PLAN_RULES)
  static const int wino_min_blocks = env_int("A2M_WINO_MIN_BLOCKS", 0);
  if (xform == XFORM_WINO && blocks < wino_min_blocks) return false;
  for (const DirectRule& d : xform == XFORM_WINO ? kWinoDirect : kDownDirect)
    if (blocks >= d.min_blocks && blocks <= d.max_blocks && K >= d.min_k && K <= d.max_k) return false;
  return true;
}

// the Toom-Cook F(2,2) down-sampling tile (gemm_f32_pipe_down.hip) takes: fp32, dense packed
// weights of 6 Ci floats a row, B the plain gather of a 4-tap stride-2 pad-1 conv1d over
// t-contiguous, 16-byte aligned x [B][Ci][Tin] with whole 32-channel chunks and clips of Tin >= 16
// that tile the 128 input samples of a 64-column tile, every offset below 2^29 floats
static bool down_operands(const Gather& A, const Gather& B, const Epilogue& E, int ma, int M, int N, int K) {
  if (K <= 0 || K % 128 != 0) return false;
  const int Ci = K / 4, Tin = B.Lw;
  const bool conv = B.tapconv == 0 && B.nhwc == 0 && !B.kcontig && B.R1 == 1 && B.K1 == 1 && B.K2 == 4 &&
                    B.ar2 == 2 && B.bk2 == 1 && B.cw == -1 && B.ch == 0 && B.sw == 1 && B.divh == 1 &&
                    B.divw == 1 && B.Lh == 1 && Tin == 2 * B.R2;
  const bool clips = Tin >= 16 && Tin % 4 == 0 && 128 % Tin == 0;
  const bool aligned = reinterpret_cast<uintptr_t>(B.base) % 16 == 0 && B.sr0 % 4 == 0 && B.sk0 % 4 == 0 &&
                       B.bstride % 4 == 0 && B.sr0 >= 0 && B.sk0 >= 0;
  return conv && clips && aligned && ma == 0 && A.sr0 == 6 * Ci && E.interp_T <= 0 &&
         pipe_below((int64_t)(M - 1) * A.sr0 + 6 * Ci) &&
         pipe_below((int64_t)((N - 1) / B.R2) * B.sr0 + Tin + (int64_t)Ci * B.sk0);
}

GemmRoute gemm_route(const Gather& A, const Gather& B, const Epilogue& E, int M, int N, int K, int batch,
                     int force_split, const RouteConfig& cfg) {
  GemmRoute r{};
  const int ma = r.ma = operand_mode(A, K), mb = r.mb = operand_mode(B, K);
  const int prec = cfg.prec;
  // the down-sampling tile, on request only: the plan (tile, splits, kchunk in whole 128-k chunks
  // of 32 channels) is the planner's for the direct conv's M x N x 4 Ci on the pipelined 64x64
  // tile.  Refused: the caller's operands are those of no other kernel (A is the packed U), so
  // a2m_conv1d_down_* take a2m_conv1d_fwd_f32's route with its operands instead.
  if (cfg.xform == XFORM_DOWN && prec == 0 && cfg.pipe_override != 0 &&
      down_operands(A, B, E, ma, M, N, K) && xform_rule(XFORM_DOWN, M, N, K, batch)) {
    // The planner's table is the direct tile's, which splits K to put two blocks on a CU.  This
    // tile issues three quarters of the MFMAs, and a launch that already has a block for every CU
    // measured as fast or faster at one split, without slabs or a reduce launch (512x2048x2048:
    // 38.2 us against 40.9 at the planner's 2 splits; 1024x1024x4096: 67.4 against 71.7 at its 4
    // and 66.3 at 2; profiles/down_conv.txt).  Smaller launches keep the planner's splits.
    const bool fills = cdiv(M, 64) * cdiv(N, 64) * (int64_t)batch >= 256;
    const int fs = force_split == 0 && cfg.override_split == 0 && fills ? 1 : force_split;
    const Plan p = launch_plan(M, N, K, batch, true, prec, 4, false, fs, true, cfg);
    if (p.bm == 64) {
      r.tile = p.bm; r.bk = p.bk; r.splits = p.splits; r.kchunk = p.kchunk;
      assert(p.kchunk > 0 && p.kchunk % 128 == 0);
      r.reduce = p.splits > 1;
      r.mcontig = E.som == 1 && M > 1;
      r.vec4 = epi_vec4(E, N, r.mcontig, r.reduce);
      r.ks = 1;
      r.kind = A2M_GEMM_KIND_PIPE;
      r.pipe_mb = mb; r.pipe_ma = 0; r.pipe_nt = 0;
      r.xform = XFORM_DOWN;
      return r;
    }
  }
  const int kquant = mb == 5 ? B.tapconv : 1;
  const bool pipe_on = cfg.pipe_override >= 0 ? cfg.pipe_override != 0 : true;
  const PipeOperands po = pipe_operands(A, B, ma, mb, M, N, K);
  // gathered: row-vector staging (modes 2 / 3) or gathers; k-contiguous conv rows (mode 6) load
  // like dense rows
  // launches the pipelined tile takes are planned on 64x64 tiles: fp32 every such launch, bf16 its
  // training modes (mode-4 / plain mode-3 A: bf16 B=32 training kernel time 43.0 -> 41.7 ms a step,
  // r05_p; the bf16 planner table was refitted on the inference launches with its pipelined tile)
  const Plan p = launch_plan(M, N, K, batch, ma == 2 || ma == 3 || mb == 2 || (mb >= 3 && mb != 6), prec,
                             kquant, mb == 6, force_split,
                             pipe_on && po.taken && (prec == 0 || (prec == 1 && po.training)), cfg);
  r.tile = p.bm; r.bk = p.bk; r.splits = p.splits; r.kchunk = p.kchunk;
  // every split a whole number of k-tiles (the mode-4 loaders rely on it)
  assert(p.kchunk > 0 && p.kchunk % (p.bk * kquant) == 0);
  // the pipelined tile runs the launches planned at its 64x64 tile, fp32 or bf16; the bf16 tile
  // stages 64-channel k-tiles (mode 6: Ci % 64 == 0)
  const bool pipe = pipe_on && po.taken && p.bm == 64 &&
                    (prec == 0 || (prec == 1 && (mb != 6 || B.nhwc % 64 == 0)));
  // the halo layout of the 3-tap pad-1 convs over clips of T >= 16 (the window stored once per
  // chunk instead of once per tap): fp32 on the 64x64 one-group tile, gemm_tile's or the pipelined
  // one; bf16 on the pipelined tile only (gemm_tile's bf16 tile takes the per-tap stores)
  r.halo = cfg.halo_on && mb == 5 && p.bm == 64 && B.tapconv == 3 && B.cw == -1 && B.R2 >= 16 &&
           64 % B.R2 == 0 && (prec == 0 || (prec == 1 && pipe));
  // fused resample (E.interp_T): the tile always writes raw slabs (also at one split) and the
  // reduce kernel runs epilogue + resample
  r.interp = E.interp_T > 0;
  r.reduce = p.splits > 1 || r.interp;
  r.mcontig = E.som == 1 && M > 1 && !r.interp;
  r.vec4 = epi_vec4(E, N, r.mcontig, r.reduce);
  r.ks = 1;
  // the Winograd F(2,3) tile (gemm_f32_pipe_wino.hip), on request only: the fp32 pipelined tile's
  // halo-layout launches (3 taps, pad 1, clips of T >= 16) with whole 32-channel chunks and dense
  // packed weights of 4 Ci floats a row, where the rule table keeps the shape on it.  The plan
  // (tile, splits, kchunk) is the direct conv's.  Refused: exactly the route without the request.
  if (cfg.xform == XFORM_WINO && pipe && prec == 0 && r.halo && po.ma == 0 && K % 96 == 0 && !r.interp &&
      A.sr0 == 4 * (K / 3) && pipe_below((int64_t)(M - 1) * A.sr0 + 4 * (K / 3)) &&
      xform_rule(XFORM_WINO, M, N, K, batch))
    r.xform = XFORM_WINO;
  if (pipe) {
    r.kind = A2M_GEMM_KIND_PIPE;
    r.pipe_mb = po.mb; r.pipe_ma = po.ma;
    r.pipe_nt = mb == 5 && !r.halo ? B.tapconv : 0;
  } else if (prec == 0 && p.bm == 64 && ma == 0 && mb == 0) {
    // two wave groups per 64x64 tile pay off for dense operands (measured -9 % on the decoder
    // convs after im2col); with gathered operands (modes 1-4) they measured slower end to end
    // (also for channels-last conv rows, mode 6, the encoder measured 305.8 us against 303.2
    // without, tools/enc_plan_ab.py, four interleaved rounds)
    r.kind = A2M_GEMM_KIND_TILE_KS2;
    r.ks = 2;
  } else {
    r.kind = A2M_GEMM_KIND_TILE;
  }
  return r;
}

}  // namespace a2m
