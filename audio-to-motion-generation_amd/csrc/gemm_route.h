// The GEMM engine's launch decision as a value (gemm_route.cpp): operand modes, plan, kernel and
// output layout of one launch, computed from the operands alone.  gemm() and gemm_pair() (gemm.hip)
// launch what the route names; a new kernel family registers here and nowhere else.
#pragma once
#include "a2m_internal.h"

namespace a2m {

// the process-wide switches a route depends on (gemm.hip keeps them; route_config())
struct RouteConfig {
  int prec;             // a2m_set_gemm_precision
  int pipe_override;    // a2m_gemm_pipe_override: -1 default (pipelined), 0 gemm_tile, 1 pipelined
  int pair_override;    // a2m_convt_pair_override: -1 default (gemm_pair's fill rule), 0 never, 1 whenever eligible
  int override_tile, override_split;   // a2m_gemm_plan_override (tuning)
  int halo_on;          // A2M_GEMM_HALO
  int wino;             // this launch asks for the Winograd F(2,3) tile (a2m_conv1d_wino_*; not process-wide)
  int down;             // this launch asks for the Toom-Cook F(2,2) down-sampling tile (a2m_conv1d_down_*; not process-wide)
};

struct GemmRoute {
  int ma, mb;                 // operand modes
  int tile, bk, splits, kchunk;
  int kind;                   // A2M_GEMM_KIND_*
  int pipe_mb, pipe_nt, pipe_ma;   // template arguments of the pipelined kernel (kind PIPE)
  int ks;                     // gemm_tile wave groups (1 or 2)
  bool halo, vec4, mcontig, reduce, interp;
  bool wino;                  // kind PIPE as gemm_pipe_kernel_wino: A is the Winograd-packed weights
  bool down;                  // kind PIPE as gemm_pipe_kernel_down: A is the weights packed by a2m_conv1d_down_pack_f32
};

// Pure: no HIP call, no allocation, no mutable file-scope state (A2M_GEMM_PLAN_RULES is parsed
// once).  Pointers are inspected for alignment only.
GemmRoute gemm_route(const Gather& A, const Gather& B, const Epilogue& E, int M, int N, int K, int batch,
                     int force_split, const RouteConfig& cfg);

RouteConfig route_config();   // the current switches (gemm.hip)

int gemm_bk(int prec);
// slab workspace of a split route: [splits][batch][M][N] for the reduce kernel
size_t split_ws_bytes(const GemmRoute& r, int M, int N, int batch);
// the largest slab workspace of any route gemm() may take for the shape
size_t gemm_ws_bytes(int M, int N, int K, int batch, const RouteConfig& cfg);
// whether A2M_GEMM_PLAN_RULES fixes more than one split for the shape
bool plan_rule_splits(int M, int N, int K);
// whether the per-shape rule table keeps a requested, eligible launch on the Winograd tile (false:
// the direct tile measured faster for the shape class)
bool wino_rule(int M, int N, int K, int batch);
// the same for the down-sampling tile (false: the im2col route measured faster)
bool down_rule(int M, int N, int K, int batch);

}  // namespace a2m
