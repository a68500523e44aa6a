// Pose tracks to video frames, and generated windows to one track:
//   render_poses  generate_motion_video.py:66-164 (plot_*_keypoints, draw_pose,
//                 draw_side_by_side_poses): polylines over keypoints, drawn into planar uint8 frames
//   track_blend   generate_motion_video.py:247-260 run over a whole recording: overlapping
//                 generator windows cross-faded into one track, de-normalised in the same pass
//
// The pixel function (the spec; tests/render_ref.py restates it in float64).  The centre of pixel
// (i, j) is (i + 0.5, j + 0.5).  For one polyline of one pose, d is the smallest distance from the
// centre to any of its segments in pixel space (a zero-length segment is a point; a segment with a
// non-finite endpoint is skipped), and its coverage is c = clamp(half_width + 0.5 - d, 0, 1): the
// union of round-capped segments, one coverage per polyline, so joints carry no darker fringe.
// Per channel v starts at bg, and for pose p = 0..P-1, polyline l = 0..L-1: v = v (1 - c) + rgb c;
// the byte stored is (uint8)(v + 0.5f).
//
// Distance to a segment a-b from q, with e = b - a and r = q - a: r.e <= 0 gives |q - a|,
// r.e >= e.e gives |q - b|, otherwise |r x e| / |e|.  The cross product keeps the error of an
// interior distance relative to the distance itself, not to the segment's length.
#include "a2m_internal.h"

#include <cmath>

namespace a2m {

constexpr int RENDER_MAX_L = A2M_RENDER_MAX_POLYLINES, RENDER_MAX_IDX = A2M_RENDER_MAX_INDICES,
              RENDER_MAX_PTS = A2M_RENDER_MAX_POINTS;
constexpr int TILE_W = 64, TILE_H = 16, WAVE_ROWS = 4;  // 256 threads x 4 pixels of one row
constexpr int RENDER_MAX_CHUNKS = A2M_RENDER_MAX_CHUNKS;

// The polyline tables travel by value in the kernel arguments (a captured graph needs no device
// copy of them); the kernel copies idx and line into LDS, where lanes index them, and reads rgb
// with wave-uniform indices.
struct RenderTopo {
  uint16_t idx[RENDER_MAX_IDX];
  uint8_t line[RENDER_MAX_IDX];  // the polyline of idx[t]; 255 where idx[t] ends its polyline
  uint8_t rgb[RENDER_MAX_L * 3];
};

__device__ __forceinline__ bool finite2(float2 a) { return isfinite(a.x) && isfinite(a.y); }

// v = v (1 - c) + rgb c for the four pixels of a lane, c from the polyline's squared distances
__device__ __forceinline__ void blend4(float (&v)[4][3], float (&d2)[4], float reach,
                                       float r, float g, float b) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float c = fminf(fmaxf(reach - sqrtf(d2[q]), 0.f), 1.f);
    const float k1 = 1.f - c;
    v[q][0] = v[q][0] * k1 + r * c;
    v[q][1] = v[q][1] * k1 + g * c;
    v[q][2] = v[q][2] * k1 + b * c;
    d2[q] = INFINITY;
  }
}

// does segment a-b meet the box [x0, x1] x [y0, y1]?  (conservative by `eps` in the parameter)
__device__ __forceinline__ bool segment_meets_box(float2 a, float2 b, float x0, float x1, float y0,
                                                  float y1) {
  float t0 = 0.f, t1 = 1.f;
  bool ok = true;
  const float ex = b.x - a.x, ey = b.y - a.y;
  if (ex == 0.f) {
    ok = a.x >= x0 && a.x <= x1;
  } else {
    const float inv = 1.f / ex, ta = (x0 - a.x) * inv, tb = (x1 - a.x) * inv;
    t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
  }
  if (ey == 0.f) {
    ok = ok && a.y >= y0 && a.y <= y1;
  } else {
    const float inv = 1.f / ey, ta = (y0 - a.y) * inv, tb = (y1 - a.y) * inv;
    t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
  }
  return ok && t0 <= t1 + 1e-5f;
}

// One workgroup per (frame, 64 x 16 pixel tile); wave w owns rows 4w .. 4w+3, lane = (row, 16
// groups of 4 pixels).  The frame's P*K keypoints are transformed into LDS once, next to a copy
// of the polyline tables.  Culling is never done per lane and pixel.  First the workgroup tests
// every segment once, one per lane, against the tile's rectangle grown by the line's reach (a
// slab clip of the segment) and keeps the ballots in LDS; most tiles end there with background.
// Then each wave retests the tile's survivors against its own 64 x 4 rectangle, and that ballot
// is the compact list: a scalar loop walks its set bits in ascending order, which is draw order
// with the segments of one polyline adjacent, so the lanes keep the smallest squared distance of
// the current polyline and blend when the polyline changes.  A culled segment is farther than
// the reach from every pixel of the wave, so leaving it out of the minimum changes no coverage.
__global__ __launch_bounds__(256) void render_poses_kernel(
    const float* __restrict__ kp, int P, int K, const RenderTopo topo, int n_idx,
    const float* __restrict__ xform, float reach, float bg0, float bg1, float bg2, int W, int H,
    int tiles_x, int tiles_per_frame, int dword_rows, uint8_t* __restrict__ out) {
  extern __shared__ unsigned long long s_mask[];                      // [P * cpp] tile-level survivors
  const int cpp = (n_idx + 63) >> 6;                                  // 64-segment chunks per pose
  float2* pts = reinterpret_cast<float2*>(s_mask + P * cpp);          // [P*K]
  uint16_t* s_idx = reinterpret_cast<uint16_t*>(pts + P * K);         // [n_idx]
  uint8_t* s_line = reinterpret_cast<uint8_t*>(s_idx + n_idx);        // [n_idx]
  const int tid = threadIdx.x;
  const int n = blockIdx.x / tiles_per_frame, tile = blockIdx.x - n * tiles_per_frame;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const float* fr = kp + (int64_t)n * P * 2 * K;
  for (int i = tid; i < P * K; i += 256) {
    const int p = i / K, k = i - p * K;
    const float* xf = xform + 4 * p;
    pts[i] = make_float2(xf[0] * fr[(int64_t)(2 * p) * K + k] + xf[1],
                         xf[2] * fr[(int64_t)(2 * p + 1) * K + k] + xf[3]);
  }
  for (int i = tid; i < n_idx; i += 256) { s_idx[i] = topo.idx[i]; s_line[i] = topo.line[i]; }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int wx0 = tx * TILE_W, x = wx0 + (lane & 15) * 4;
  // a pixel is touched only when d < reach; the slack covers the rounding of d and of the clip
  const float grow = reach + 0.01f + 1e-5f * reach;
  const float bx0 = wx0 + 0.5f - grow, bx1 = min(wx0 + TILE_W, W) - 0.5f + grow;

  // the tile's survivors: chunk m = (pose, 64 segment slots), one chunk per wave at a time; slot
  // t of a pose is the segment idx[t] - idx[t+1]
  {
    const float ty0 = ty * TILE_H + 0.5f - grow, ty1 = min((ty + 1) * TILE_H, H) - 0.5f + grow;
    for (int m = wave; m < P * cpp; m += 4) {
      const int p = m / cpp, t = (m - p * cpp) * 64 + lane;
      bool hit = false;
      if (t < n_idx && s_line[t] != 255) {
        const float2 a = pts[p * K + s_idx[t]], b = pts[p * K + s_idx[t + 1]];
        hit = finite2(a) && finite2(b) && segment_meets_box(a, b, bx0, bx1, ty0, ty1);
      }
      const unsigned long long mask = __ballot(hit);
      if (lane == 0) s_mask[m] = mask;
    }
  }
  __syncthreads();

  const int wy0 = ty * TILE_H + wave * WAVE_ROWS, y = wy0 + (lane >> 4);
  if (wy0 >= H) return;        // wave-uniform (every lane votes in the ballots); no barrier follows
  const float by0 = wy0 + 0.5f - grow, by1 = min(wy0 + WAVE_ROWS, H) - 0.5f + grow;
  const float qy = y + 0.5f;
  float v[4][3];
  float d2[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
#pragma unroll
  for (int q = 0; q < 4; ++q) { v[q][0] = bg0; v[q][1] = bg1; v[q][2] = bg2; }
  int cur_p = -1, cur_l = 0;   // the polyline whose segments d2 holds

  for (int p = 0; p < P; ++p) {
    const float2* pp = pts + p * K;
    for (int c = 0; c < cpp; ++c) {
      const unsigned long long tile_mask = s_mask[p * cpp + c];
      if (tile_mask == 0) continue;                                  // wave-uniform
      const int t0 = c * 64;
      bool hit = false;
      if ((tile_mask >> lane) & 1) {
        const float2 a = pp[s_idx[t0 + lane]], b = pp[s_idx[t0 + lane + 1]];
        hit = segment_meets_box(a, b, bx0, bx1, by0, by1);
      }
      unsigned long long mask = __ballot(hit);
      while (mask) {
        const int t = t0 + __builtin_ctzll(mask);
        mask &= mask - 1;
        const int l = s_line[t];
        if (p != cur_p || l != cur_l) {
          if (cur_p >= 0)
            blend4(v, d2, reach, topo.rgb[3 * cur_l], topo.rgb[3 * cur_l + 1], topo.rgb[3 * cur_l + 2]);
          cur_p = p; cur_l = l;
        }
        const float2 a = pp[s_idx[t]], b = pp[s_idx[t + 1]];
        const float ex = b.x - a.x, ey = b.y - a.y;
        const float len2 = ex * ex + ey * ey;
        const float inv = len2 > 0.f ? 1.f / len2 : 0.f;
        const float ry = qy - a.y, sy = qy - b.y;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float qx = (x + q) + 0.5f;
          const float rx = qx - a.x, sx = qx - b.x;
          const float dot = rx * ex + ry * ey;
          const float cr = rx * ey - ry * ex;
          const float da = rx * rx + ry * ry, db = sx * sx + sy * sy;
          const float dm = cr * cr * inv;
          const float d = dot <= 0.f ? da : (dot >= len2 ? db : dm);
          d2[q] = fminf(d2[q], d);
        }
      }
    }
  }
  if (cur_p >= 0) blend4(v, d2, reach, topo.rgb[3 * cur_l], topo.rgb[3 * cur_l + 1], topo.rgb[3 * cur_l + 2]);

  if (y >= H || x >= W) return;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    uint32_t b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = (uint32_t)(v[q][ch] + 0.5f);
    uint8_t* row = out + (((int64_t)n * 3 + ch) * H + y) * (int64_t)W + x;
    // dword_rows: W % 4 == 0 and an aligned base, so every group of four is whole and aligned
    if (dword_rows || (x + 3 < W && (reinterpret_cast<uintptr_t>(row) & 3) == 0)) {
      *reinterpret_cast<uint32_t*>(row) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (x + q < W) row[q] = (uint8_t)b[q];
    }
  }
}

// One element of the stitched track, shared by the offline and the streaming kernel: `val` is
// channel c of frame j of its window, *prev (null outside an overlap) the same channel of frame
// j + h of the window before.  The cross-fade is two rounded products and one rounded sum, written
// out so that no context contracts it into an fma.
__device__ __forceinline__ float track_blend_value(float val, const float* __restrict__ prev, int j,
                                                   int overlap, int c, const float* __restrict__ mean,
                                                   const float* __restrict__ std_) {
  if (prev) {
    const float w1 = __fdiv_rn(j + 0.5f, (float)overlap);
    const float w0 = __fdiv_rn(overlap - j - 0.5f, (float)overlap);
    val = __fadd_rn(__fmul_rn(w0, *prev), __fmul_rn(w1, val));
  }
  if (mean) {
    // the two roundings of a2m_pose_denormalize_f32 (see pose_denormalize_kernel)
    float scaled = val * std_[c];
    asm volatile("" : "+v"(scaled));
    val = scaled + mean[c];
  }
  return val;
}

// out frame f of the stitched track reads window k = min(f / h, n - 1) at j = f - k h, and, when
// k > 0 and j < overlap, also window k - 1 at j + h; h = T - overlap.
__global__ void track_blend_kernel(const float* __restrict__ win, int n, int T, int Fd, int overlap,
                                   const float* __restrict__ mean, const float* __restrict__ std_,
                                   int64_t total, float* __restrict__ out) {
  const int h = T - overlap;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / Fd;
    const int c = (int)(i - f * Fd);
    const int k = (int)min(f / h, (int64_t)n - 1);
    const int j = (int)(f - (int64_t)k * h);
    const float val = win[((int64_t)k * T + j) * Fd + c];
    const float* prev = k > 0 && j < overlap ? win + ((int64_t)(k - 1) * T + j + h) * Fd + c : nullptr;
    out[i] = track_blend_value(val, prev, j, overlap, c, mean, std_);
  }
}

// The same track, m windows at a time.  `tail` [overlap][Fd] carries frames [h, T) of the last
// window seen (normalised, as the generator gave them); has_prev says whether it holds one.  The
// launch writes the m h frames that the new windows make final: frame f reads window k = f / h at
// j = f - k h, and inside an overlap the window before, which for k = 0 is the tail.  Element
// (j, c) of the tail is read and then rewritten by the one thread that owns output (j, c) of
// window 0 (overlap <= h, so those outputs all belong to window 0): no ordering between threads
// is needed.  With `flush`, the overlap frames after them are the (new) tail, unblended.
__global__ void track_blend_stream_kernel(const float* __restrict__ win, int m, int T, int Fd, int overlap,
                                          float* __restrict__ tail, int has_prev, int flush,
                                          const float* __restrict__ mean, const float* __restrict__ std_,
                                          int64_t total, float* __restrict__ out) {
  const int h = T - overlap;
  const int64_t body = (int64_t)m * h * Fd;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / Fd;
    const int c = (int)(i - f * Fd);
    if (i >= body) {  // flush: frame h + j of the last window
      const int j = (int)(f - (int64_t)m * h);
      const float val = m > 0 ? win[((int64_t)(m - 1) * T + h + j) * Fd + c] : tail[(int64_t)j * Fd + c];
      out[i] = track_blend_value(val, nullptr, h + j, overlap, c, mean, std_);
      continue;
    }
    const int k = (int)(f / h);
    const int j = (int)(f - (int64_t)k * h);
    const float val = win[((int64_t)k * T + j) * Fd + c];
    const float* prev = nullptr;
    float carried = 0.f;
    if (j < overlap) {
      if (k > 0) {
        prev = win + ((int64_t)(k - 1) * T + j + h) * Fd + c;
      } else {
        float* slot = tail + (int64_t)j * Fd + c;
        carried = *slot;
        if (has_prev) prev = &carried;
        *slot = win[((int64_t)(m - 1) * T + h + j) * Fd + c];
      }
    }
    out[i] = track_blend_value(val, prev, j, overlap, c, mean, std_);
  }
}

}  // namespace a2m

using namespace a2m;

extern "C" {

int a2m_render_poses_u8(const float* kp, int32_t N, int32_t P, int32_t K, const int32_t* poly_idx,
                        const int32_t* poly_off, const uint8_t* poly_rgb, int32_t L,
                        const float* xform, float half_width_px, const uint8_t bg[3], int32_t W,
                        int32_t H, uint8_t* out, void* stream) {
  A2M_CHECK_ARG(N >= 0 && P >= 1 && K >= 1 && L >= 0 && W >= 1 && H >= 1,
                "render_poses: need N >= 0, P, K, W, H >= 1 and L >= 0 (N %d P %d K %d L %d W %d H %d)",
                N, P, K, L, W, H);
  A2M_CHECK_ARG(std::isfinite(half_width_px) && half_width_px >= 0.f,
                "render_poses: half_width_px must be finite and >= 0");
  if (N == 0) return A2M_OK;
  A2M_CHECK_ARG(kp && poly_idx && poly_off && poly_rgb && xform && bg && out,
                "render_poses: null pointer");
  A2M_CHECK_ARG(L <= RENDER_MAX_L && (int64_t)P * K <= RENDER_MAX_PTS,
                "render_poses: at most %d polylines and %d keypoints per frame (L %d, P*K %lld)",
                RENDER_MAX_L, RENDER_MAX_PTS, L, (long long)P * K);
  A2M_CHECK_ARG(poly_off[0] == 0, "render_poses: poly_off[0] must be 0");
  RenderTopo topo{};
  for (int l = 0; l < L; ++l) {
    const int64_t len = (int64_t)poly_off[l + 1] - poly_off[l];
    A2M_CHECK_ARG(len >= 2, "render_poses: polyline %d has %lld indices, needs at least 2", l,
                  (long long)len);
    A2M_CHECK_ARG(poly_off[l + 1] <= RENDER_MAX_IDX, "render_poses: more than %d polyline indices",
                  RENDER_MAX_IDX);
    for (int t = poly_off[l]; t < poly_off[l + 1]; ++t) topo.line[t] = t + 1 < poly_off[l + 1] ? l : 255;
    for (int c = 0; c < 3; ++c) topo.rgb[3 * l + c] = poly_rgb[3 * l + c];
  }
  for (int s = 0; s < poly_off[L]; ++s) {
    A2M_CHECK_ARG(poly_idx[s] >= 0 && poly_idx[s] < K, "render_poses: poly_idx[%d] = %d outside [0, %d)",
                  s, poly_idx[s], K);
    topo.idx[s] = (uint16_t)poly_idx[s];
  }
  const int tiles_x = (int)cdiv(W, TILE_W), tiles_y = (int)cdiv(H, TILE_H);
  const int64_t blocks = (int64_t)N * tiles_x * tiles_y;
  A2M_CHECK_ARG(blocks <= INT32_MAX, "render_poses: %lld tiles exceed one launch", (long long)blocks);
  const int dword_rows = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  const int n_idx = poly_off[L];
  const int64_t chunks = (int64_t)P * cdiv(n_idx, 64);
  A2M_CHECK_ARG(chunks <= RENDER_MAX_CHUNKS, "render_poses: P * ceil(indices / 64) = %lld exceeds %d",
                (long long)chunks, RENDER_MAX_CHUNKS);
  const size_t lds = (size_t)chunks * sizeof(unsigned long long) + (size_t)P * K * sizeof(float2) +
                     (size_t)n_idx * (sizeof(uint16_t) + sizeof(uint8_t));
  hipLaunchKernelGGL(render_poses_kernel, dim3((unsigned)blocks), dim3(256), lds, as_stream(stream),
                     kp, P, K, topo, n_idx, xform,
                     half_width_px + 0.5f, (float)bg[0], (float)bg[1], (float)bg[2], W, H, tiles_x,
                     tiles_x * tiles_y, dword_rows, out);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_track_blend_f32(const float* win, int32_t n, int32_t T, int32_t Fd, int32_t overlap,
                        const float* mean, const float* std_, float* out, void* stream) {
  A2M_CHECK_ARG(n >= 0 && T >= 1 && Fd >= 1, "track_blend: need n >= 0, T >= 1, Fd >= 1 (n %d T %d Fd %d)",
                n, T, Fd);
  A2M_CHECK_ARG(overlap >= 0 && overlap <= T / 2, "track_blend: overlap %d outside [0, T/2 = %d]",
                overlap, T / 2);
  A2M_CHECK_ARG((mean == nullptr) == (std_ == nullptr), "track_blend: mean and std come together");
  if (n == 0) return A2M_OK;
  A2M_CHECK_ARG(win && out, "track_blend: null pointer");
  const int64_t total = ((int64_t)(n - 1) * (T - overlap) + T) * Fd;
  const int blocks = (int)std::min<int64_t>(cdiv(total, 256), 4096);
  hipLaunchKernelGGL(track_blend_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), win, n, T, Fd,
                     overlap, mean, std_, total, out);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

int a2m_track_blend_stream_f32(const float* win, int32_t m, int32_t T, int32_t Fd, int32_t overlap,
                               float* tail, int32_t has_prev, int32_t flush, const float* mean,
                               const float* std_, float* out, void* stream) {
  A2M_CHECK_ARG(m >= 0 && T >= 1 && Fd >= 1,
                "track_blend_stream: need m >= 0, T >= 1, Fd >= 1 (m %d T %d Fd %d)", m, T, Fd);
  A2M_CHECK_ARG(overlap >= 0 && overlap <= T / 2, "track_blend_stream: overlap %d outside [0, T/2 = %d]",
                overlap, T / 2);
  A2M_CHECK_ARG((mean == nullptr) == (std_ == nullptr), "track_blend_stream: mean and std come together");
  A2M_CHECK_ARG(!flush || m > 0 || has_prev, "track_blend_stream: a flush with no window before it");
  const int64_t total = ((int64_t)m * (T - overlap) + (flush ? overlap : 0)) * Fd;
  if (m > 0 || flush) A2M_CHECK_ARG(tail || overlap == 0, "track_blend_stream: null tail");
  if (total == 0) return A2M_OK;  // nothing final: no window, or a flush at overlap 0
  A2M_CHECK_ARG((win || m == 0) && out, "track_blend_stream: null pointer");
  const int blocks = (int)std::min<int64_t>(cdiv(total, 256), 4096);
  hipLaunchKernelGGL(track_blend_stream_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), win, m, T,
                     Fd, overlap, tail, has_prev != 0, flush != 0, mean, std_, total, out);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

}  // extern "C"
