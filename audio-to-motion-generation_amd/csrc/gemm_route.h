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
  Xform xform;          // this launch asks for a transform tile (a2m_conv1d_wino_*, a2m_conv1d_down_*; not process-wide)
};

struct GemmRoute {
  int ma, mb;                 // operand modes
  int tile, bk, splits, kchunk;
  int kind;                   // A2M_GEMM_KIND_*
  int pipe_mb, pipe_nt, pipe_ma;   // template arguments of the pipelined kernel (kind PIPE)
  int ks;                     // gemm_tile wave groups (1 or 2)
  bool halo, vec4, mcontig, reduce, interp;
  Xform xform;                // kind PIPE as gemm_pipe_kernel_wino / gemm_pipe_kernel_down: A is that tile's packed weights
};

// Pure: no HIP call, no allocation, no mutable file-scope state (A2M_GEMM_PLAN_RULES is parsed
// once).  Pointers are inspected for alignment only.
GemmRoute gemm_route(const Gather& A, const Gather& B, const Epilogue& E, int M, int N, int K, int batch,
                     int force_split, const RouteConfig& cfg);

RouteConfig route_config();   // the current switches (gemm.hip)
// a route as the a2m_*_route queries report it: {kind, tile, bk, splits, kchunk, ma, mb, flags} with flags
// 1 vec4, 2 m-contiguous, 4 halo, 8 reduce, 16 the Winograd tile, 32 the down-sampling tile
void route_out(const GemmRoute& r, int32_t out[8]);

int gemm_bk(int prec);
// slab workspace of a split route: [splits][batch][M][N] for the reduce kernel
size_t split_ws_bytes(const GemmRoute& r, int M, int N, int batch);
// the largest slab workspace of any route gemm() may take for the shape
size_t gemm_ws_bytes(int M, int N, int K, int batch, const RouteConfig& cfg);
// whether A2M_GEMM_PLAN_RULES fixes more than one split for the shape
bool plan_rule_splits(int M, int N, int K);
// whether the tile's per-shape rule table keeps a requested, eligible launch on it (false: the
// route without the request measured faster for the shape class)
bool xform_rule(Xform xform, int M, int N, int K, int batch);

}  // namespace a2m
