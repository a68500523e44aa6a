// Baseline JPEG on the device (include/a2m.h states the byte stream; tests/jpeg_ref.py restates it):
// planar full-range YCbCr frames -> the entropy-coded scans of 4:4:4 baseline files whose restart
// interval is one MCU row, compacted back to back.  Six launches, no atomics whose order matters:
//
//   dct_quant      one wave per 8x8 block: level shift, integer DCT (two passes through LDS),
//                  quantisation; int16 coefficients in zig-zag order
//   interval_bits  one workgroup per restart interval: each wave sizes blocks (lane k = zig-zag
//                  coefficient k, one ballot = the run-length structure), then the workgroup scans
//                  the block sizes into bit positions and zeroes the words the interval will use
//   pack           one wave per block: the same codes again, a wave prefix sum of their lengths,
//                  bit-OR into the interval's zeroed words (OR into zeroes is order-free)
//   pad_count      per interval: 1-bits up to the byte boundary, count of 0xFF bytes -> stuffed size
//   place          one workgroup: scan of interval sizes -> interval positions and offsets[N + 1]
//   emit           per interval: bytes to their final position, 0x00 after every 0xFF, RSTn after
//                  every interval but a frame's last; nothing is written at or past the capacity
//
// The unstuffed bits of an interval live in the workspace: at most 208 bytes a block (22 bits of
// DC, 63 x 26 bits of AC), which for a 188-MCU row is 117 KB and would not fit in LDS.
#include "a2m_internal.h"

namespace a2m {

constexpr int JPEG_BLOCK_BYTES = A2M_JPEG_MAX_BLOCK_BYTES;

// round(2^13 * c(u)/2 * cos((2x + 1) u pi / 16)), c(0) = 1/sqrt(2), c(u > 0) = 1
struct DctTab { int16_t m[64]; };
constexpr int16_t kC[8] = {A2M_JPEG_C0, A2M_JPEG_C1, A2M_JPEG_C2, A2M_JPEG_C3,
                           A2M_JPEG_C4, A2M_JPEG_C5, A2M_JPEG_C6, A2M_JPEG_C7};
constexpr DctTab make_dct() {
  DctTab t{};
  for (int u = 0; u < 8; ++u)
    for (int x = 0; x < 8; ++x) {
      // cos(k pi / 16) for k = (2x + 1) u, folded into the first quadrant
      int k = ((2 * x + 1) * u) % 32;
      int sign = 1;
      if (k > 16) k = 32 - k;
      if (k > 8) { k = 16 - k; sign = -1; }
      t.m[u * 8 + x] = u == 0 ? kC[0] : (int16_t)(sign * (k == 8 ? 0 : kC[k]));
    }
  return t;
}

// ITU-T T.81 Annex K.3-K.6 (BITS, HUFFVAL), the tables a2m.jpeg.jpeg_header writes into DHT
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
     0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
     0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
     0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
     0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
     0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
     0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
     0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
     0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa}};

// symbol -> (code << 5) | length, by the code assignment of T.81 Annex C; [t]: 0 luma, 1 chroma
struct HuffTab {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};
constexpr HuffTab make_huff() {
  HuffTab h{};
  for (int t = 0; t < 2; ++t) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len, code <<= 1)
      for (int i = 0; i < kDcBits[t][len - 1]; ++i, ++k, ++code) h.dc[t][k] = (code << 5) | len;
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len, code <<= 1)
      for (int i = 0; i < kAcBits[t][len - 1]; ++i, ++k, ++code)
        h.ac[t][kAcVals[t][k]] = (code << 5) | len;
  }
  return h;
}

__constant__ const DctTab d_dct = make_dct();
__constant__ const HuffTab d_huff = make_huff();
__constant__ const uint8_t d_zigzag_of[64] = {   // natural index -> zig-zag position
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct QuantTab { uint16_t q[2][64]; };   // natural order; by value in the kernel arguments

// the frame's geometry, shared by every kernel
struct JpegGeom {
  int N, W, H, MW, MH;      // MW x MH MCUs (8 x 8 pixels, three blocks each)
  int nblk;                 // blocks of one restart interval = 3 MW
  int64_t slot_words;       // 32-bit words of one interval's unstuffed bits in the workspace
};

// ------------------------------------------------------------------------------ wave helpers
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive scan of v over the 256 threads of the workgroup; *total = the sum.  s_part: 4 ints.
__device__ __forceinline__ int block_excl_scan(int v, int* s_part, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v, lane);
  __syncthreads();                       // s_part may still be read from the previous call
  if (lane == 63) s_part[wave] = incl;
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int p = s_part[w];
    if (w < wave) before += p;
    sum += p;
  }
  *total = sum;
  return before + incl - v;
}

// The bits lane k contributes to its block (k = zig-zag position; c = the quantised coefficient,
// the DC difference on lane 0), most significant first in the low `len` bits of *bits; returns
// len <= 63.  A lane with a nonzero coefficient emits the ZRLs of the zero run before it, its
// (run, size) code and its value bits; the last such lane (lane 0 when every AC is zero) appends
// EOB unless it is lane 63.
__device__ __forceinline__ int lane_code(int c, int k, int t, uint64_t* bits) {
  const unsigned long long mask = __ballot(c != 0) | 1ull;
  uint64_t b = 0;
  int len = 0;
  if (k == 0 || c != 0) {
    const int a = c < 0 ? -c : c;
    const int sz = a ? 32 - __builtin_clz(a) : 0;
    const uint32_t val = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << sz) - 1u);
    uint32_t e;
    if (k == 0) {
      e = d_huff.dc[t][sz];
    } else {
      const unsigned long long below = mask & ((1ull << k) - 1ull);
      const int run = k - 1 - (63 - __builtin_clzll(below));
      const uint32_t zrl = d_huff.ac[t][0xF0];
      for (int z = run >> 4; z > 0; --z) {
        b = (b << (zrl & 31)) | (zrl >> 5);
        len += zrl & 31;
      }
      e = d_huff.ac[t][((run & 15) << 4) | sz];
    }
    b = (b << (e & 31)) | (e >> 5);
    b = (b << sz) | val;
    len += (e & 31) + sz;
    if (k < 63 && (mask >> k) == 1ull) {
      const uint32_t eob = d_huff.ac[t][0x00];
      b = (b << (eob & 31)) | (eob >> 5);
      len += eob & 31;
    }
  }
  *bits = b;
  return len;
}

// coefficient of lane k of block `blk` (b = its index in the interval), DC as a difference to the
// same component's previous block of the interval
__device__ __forceinline__ int load_coef(const int16_t* __restrict__ coef, int64_t blk, int b, int k) {
  int c = coef[blk * 64 + k];
  if (k == 0 && b >= 3) c -= coef[(blk - 3) * 64];
  return c;
}

// ------------------------------------------------------------------------------ kernels
// Block order is scan order: blk = ((n MH + r) MW + m) 3 + comp.
__global__ __launch_bounds__(256) void jpeg_dct_quant_kernel(const uint8_t* __restrict__ frames,
                                                             const JpegGeom g, const QuantTab qt,
                                                             int64_t n_blocks,
                                                             int16_t* __restrict__ coef) {
  __shared__ int s_px[4][64];
  __shared__ int s_t[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t blk_raw = (int64_t)blockIdx.x * 4 + wave;
  const bool live = blk_raw < n_blocks;
  const int64_t blk = live ? blk_raw : n_blocks - 1;
  const int comp = (int)(blk % 3);
  const int64_t mcu = blk / 3;
  const int m = (int)(mcu % g.MW);
  const int64_t row = mcu / g.MW;           // n MH + r
  const int r = (int)(row % g.MH);
  const int64_t n = row / g.MH;
  const int i = lane >> 3, j = lane & 7;    // (y, x), then (y, u), then (v, u)
  const int y = min(r * 8 + i, g.H - 1), x = min(m * 8 + j, g.W - 1);   // edge replication
  s_px[wave][lane] = (int)frames[((n * 3 + comp) * g.H + y) * (int64_t)g.W + x] - 128;
  __syncthreads();
  int a = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) a += s_px[wave][i * 8 + q] * d_dct.m[j * 8 + q];
  s_t[wave][lane] = (a + (1 << (A2M_JPEG_PASS1_SHIFT - 1))) >> A2M_JPEG_PASS1_SHIFT;
  __syncthreads();
  int b = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) b += s_t[wave][q * 8 + j] * d_dct.m[i * 8 + q];
  const int c = (b + (1 << (A2M_JPEG_PASS2_SHIFT - 1))) >> A2M_JPEG_PASS2_SHIFT;
  const int Q = qt.q[comp != 0][lane];
  const int mag = ((c < 0 ? -c : c) * 2 + Q) / (2 * Q);      // round half away from zero
  const int lim = lane == 0 ? 1024 : 1023;                   // never reached; keeps every symbol coded
  const int v = min(mag, lim);
  if (live) coef[blk * 64 + d_zigzag_of[lane]] = (int16_t)(c < 0 ? -v : v);
}

// pos[blk]: in, nothing; out, the block's first bit within its interval.  iv_bits[iv]: the
// interval's unstuffed length in bits.
__global__ __launch_bounds__(256) void jpeg_interval_bits_kernel(const int16_t* __restrict__ coef,
                                                                 const JpegGeom g, uint32_t* pos,
                                                                 uint32_t* __restrict__ iv_bits,
                                                                 uint32_t* __restrict__ scan) {
  __shared__ int s_part[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t iv = blockIdx.x;
  const int64_t base = iv * g.nblk;
  for (int b = wave; b < g.nblk; b += 4) {
    uint64_t bits;
    const int len = lane_code(load_coef(coef, base + b, b, lane), lane, b % 3 != 0, &bits);
    const int total = wave_incl_scan(len, lane);
    if (lane == 63) pos[base + b] = (uint32_t)total;
  }
  __threadfence();
  __syncthreads();
  int carry = 0;
  for (int s = 0; s < g.nblk; s += 256) {
    const int b = s + (int)threadIdx.x;
    const int v = b < g.nblk ? (int)pos[base + b] : 0;
    int total;
    const int excl = block_excl_scan(v, s_part, &total);
    if (b < g.nblk) pos[base + b] = (uint32_t)(carry + excl);
    carry += total;
  }
  if (threadIdx.x == 0) iv_bits[iv] = (uint32_t)carry;
  // the words pack will OR into: the last code may reach two words past its first
  uint32_t* slot = scan + iv * g.slot_words;
  const int64_t words = min((int64_t)(carry >> 5) + 3, g.slot_words);
  for (int64_t w = threadIdx.x; w < words; w += 256) slot[w] = 0u;
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int16_t* __restrict__ coef,
                                                        const JpegGeom g, int64_t n_blocks,
                                                        const uint32_t* __restrict__ pos,
                                                        uint32_t* __restrict__ scan) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * 4 + wave;
  if (blk >= n_blocks) return;                       // wave-uniform
  const int64_t iv = blk / g.nblk;
  const int b = (int)(blk - iv * g.nblk);
  uint64_t bits;
  const int len = lane_code(load_coef(coef, blk, b, lane), lane, b % 3 != 0, &bits);
  const int incl = wave_incl_scan(len, lane);
  if (len == 0) return;
  const uint32_t p = pos[blk] + (uint32_t)(incl - len);
  const int64_t w = p >> 5;
  if (w + 2 >= g.slot_words) return;                 // cannot happen: the slot holds the worst case
  uint32_t* slot = scan + iv * g.slot_words + w;
  const int o = (int)(p & 31);
  const uint64_t v = bits << (64 - len);             // the code at the top of 64 bits
  const uint64_t hi = v >> o;
  const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi;
  const uint32_t w2 = o ? (uint32_t)v << (32 - o) : 0u;
  if (w0) atomicOr(slot, w0);
  if (w1) atomicOr(slot + 1, w1);
  if (w2) atomicOr(slot + 2, w2);
}

__device__ __forceinline__ uint32_t scan_byte(const uint32_t* slot, int64_t i) {
  return (slot[i >> 2] >> (24 - 8 * (int)(i & 3))) & 0xFFu;
}

// iv_size[iv]: the interval's bytes in the file, stuffing and its RSTn marker included
__global__ __launch_bounds__(256) void jpeg_pad_count_kernel(const JpegGeom g,
                                                             const uint32_t* __restrict__ iv_bits,
                                                             uint32_t* scan,
                                                             uint32_t* __restrict__ iv_size) {
  __shared__ int s_part[4];
  const int64_t iv = blockIdx.x;
  uint32_t* slot = scan + iv * g.slot_words;
  const uint32_t bits = iv_bits[iv];
  const int64_t bytes = min(((int64_t)bits + 7) >> 3, g.slot_words * 4);   // the slot holds the worst case
  if (threadIdx.x == 0 && (bits & 7)) {
    const int64_t last = bits >> 3;
    slot[last >> 2] |= ((1u << (8 - (bits & 7))) - 1u) << (24 - 8 * (int)(last & 3));
  }
  __threadfence();
  __syncthreads();
  int count = 0;
  for (int64_t i = threadIdx.x; i < bytes; i += 256) count += scan_byte(slot, i) == 0xFFu;
  int total;
  block_excl_scan(count, s_part, &total);
  const bool last_of_frame = (iv % g.MH) == g.MH - 1;
  if (threadIdx.x == 0) iv_size[iv] = (uint32_t)(bytes + total + (last_of_frame ? 0 : 2));
}

// one workgroup; thread f sums frame f's intervals, the frames are scanned 256 at a time
__global__ __launch_bounds__(256) void jpeg_place_kernel(const JpegGeom g,
                                                         const uint32_t* __restrict__ iv_size,
                                                         int64_t* __restrict__ iv_start,
                                                         int64_t* __restrict__ offsets) {
  __shared__ int64_t s_sum[256];
  __shared__ int64_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int f0 = 0; f0 < g.N; f0 += 256) {
    const int f = f0 + (int)threadIdx.x;
    int64_t size = 0;
    if (f < g.N)
      for (int r = 0; r < g.MH; ++r) size += iv_size[(int64_t)f * g.MH + r];
    s_sum[threadIdx.x] = size;
    __syncthreads();
    int64_t start = s_carry;
    for (int q = 0; q < (int)threadIdx.x; ++q) start += s_sum[q];
    __syncthreads();
    if (threadIdx.x == 255) s_carry = start + size;
    if (f < g.N) {
      offsets[f] = start;
      for (int r = 0; r < g.MH; ++r) {
        iv_start[(int64_t)f * g.MH + r] = start;
        start += iv_size[(int64_t)f * g.MH + r];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[g.N] = s_carry;
}

__global__ __launch_bounds__(256) void jpeg_emit_kernel(const JpegGeom g,
                                                        const uint32_t* __restrict__ iv_bits,
                                                        const uint32_t* __restrict__ scan,
                                                        const int64_t* __restrict__ iv_start,
                                                        uint8_t* __restrict__ out, int64_t capacity) {
  __shared__ int s_part[4];
  const int64_t iv = blockIdx.x;
  const uint32_t* slot = scan + iv * g.slot_words;
  const int64_t bytes = min(((int64_t)iv_bits[iv] + 7) >> 3, g.slot_words * 4);
  int64_t at = iv_start[iv];                          // where byte s of this pass goes
  for (int64_t s = 0; s < bytes; s += 256) {          // workgroup-uniform trip count
    const int64_t i = s + threadIdx.x;
    const uint32_t byte = i < bytes ? scan_byte(slot, i) : 0u;
    const int ff = byte == 0xFFu;
    int total;
    const int before = block_excl_scan(ff, s_part, &total);
    const int64_t o = at + threadIdx.x + before;
    if (i < bytes) {
      if (o < capacity) out[o] = (uint8_t)byte;
      if (ff && o + 1 < capacity) out[o + 1] = 0;
    }
    at += 256 + total;
  }
  const int r = (int)(iv % g.MH);
  if (threadIdx.x == 0 && r != g.MH - 1) {
    const int64_t o = at - (((bytes + 255) >> 8) << 8) + bytes;   // `at` ran to the end of the last pass
    if (o < capacity) out[o] = 0xFF;
    if (o + 1 < capacity) out[o + 1] = (uint8_t)(0xD0 + (r & 7));
  }
}

// ------------------------------------------------------------------------------ host side
struct JpegWs {
  size_t coef, pos, iv_bits, iv_size, iv_start, scan, total;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static JpegGeom jpeg_geom(int N, int W, int H) {
  JpegGeom g{};
  g.N = N; g.W = W; g.H = H;
  g.MW = (W + 7) / 8; g.MH = (H + 7) / 8;
  g.nblk = 3 * g.MW;
  g.slot_words = ((int64_t)g.nblk * JPEG_BLOCK_BYTES + 3) / 4 + 4;
  return g;
}

static JpegWs jpeg_ws(const JpegGeom& g) {
  const size_t ivs = (size_t)g.N * g.MH, blocks = ivs * g.nblk;
  JpegWs w{};
  w.coef = 0;
  w.pos = w.coef + align256(blocks * 64 * sizeof(int16_t));
  w.iv_bits = w.pos + align256(blocks * sizeof(uint32_t));
  w.iv_size = w.iv_bits + align256(ivs * sizeof(uint32_t));
  w.iv_start = w.iv_size + align256(ivs * sizeof(uint32_t));
  w.scan = w.iv_start + align256(ivs * sizeof(int64_t));
  w.total = w.scan + align256(ivs * (size_t)g.slot_words * sizeof(uint32_t));
  return w;
}

// one workgroup per interval and per four blocks: both grids must fit a launch (then every size
// below fits 64 bits with room to spare)
static bool jpeg_fits_a_launch(const JpegGeom& g) {
  const int64_t ivs = (int64_t)g.N * g.MH;
  return ivs <= INT32_MAX && cdiv(ivs * g.nblk, 4) <= INT32_MAX;
}

}  // namespace a2m

using namespace a2m;

extern "C" {

size_t a2m_jpeg_ws_bytes(int32_t N, int32_t W, int32_t H) {
  if (N < 1 || W < 1 || H < 1 || W > 65535 || H > 65535) return 0;
  const JpegGeom g = jpeg_geom(N, W, H);
  return jpeg_fits_a_launch(g) ? jpeg_ws(g).total : 0;
}

int a2m_jpeg_encode_u8(const uint8_t* frames, int32_t N, int32_t W, int32_t H,
                       const uint16_t* qluma, const uint16_t* qchroma, uint8_t* out,
                       int64_t capacity, int64_t* offsets, void* ws, size_t ws_bytes, void* stream) {
  A2M_CHECK_ARG(N >= 0 && W >= 1 && H >= 1 && W <= 65535 && H <= 65535,
                "jpeg_encode: need N >= 0 and 1 <= W, H <= 65535 (N %d W %d H %d)", N, W, H);
  A2M_CHECK_ARG(capacity >= 0, "jpeg_encode: capacity %lld is negative", (long long)capacity);
  if (N == 0) return A2M_OK;
  A2M_CHECK_ARG(frames && qluma && qchroma && offsets && ws && (out || capacity == 0),
                "jpeg_encode: null pointer");
  QuantTab qt;
  for (int i = 0; i < 64; ++i) {
    A2M_CHECK_ARG(qluma[i] >= 1 && qluma[i] <= 255 && qchroma[i] >= 1 && qchroma[i] <= 255,
                  "jpeg_encode: quantiser entry %d is (%d, %d); baseline tables hold 1..255", i,
                  (int)qluma[i], (int)qchroma[i]);
    qt.q[0][i] = qluma[i];
    qt.q[1][i] = qchroma[i];
  }
  const JpegGeom g = jpeg_geom(N, W, H);
  A2M_CHECK_ARG(jpeg_fits_a_launch(g), "jpeg_encode: %lld blocks exceed one launch",
                (long long)N * g.MH * g.nblk);
  const JpegWs w = jpeg_ws(g);
  A2M_CHECK_ARG(ws_bytes >= w.total, "jpeg_encode: workspace of %zu bytes, a2m_jpeg_ws_bytes asks for %zu",
                ws_bytes, w.total);
  const int64_t ivs = (int64_t)N * g.MH, blocks = ivs * g.nblk;
  char* base = static_cast<char*>(ws);
  int16_t* coef = reinterpret_cast<int16_t*>(base + w.coef);
  uint32_t* pos = reinterpret_cast<uint32_t*>(base + w.pos);
  uint32_t* iv_bits = reinterpret_cast<uint32_t*>(base + w.iv_bits);
  uint32_t* iv_size = reinterpret_cast<uint32_t*>(base + w.iv_size);
  int64_t* iv_start = reinterpret_cast<int64_t*>(base + w.iv_start);
  uint32_t* scan = reinterpret_cast<uint32_t*>(base + w.scan);
  hipStream_t st = as_stream(stream);
  const dim3 per_block((unsigned)cdiv(blocks, 4)), per_iv((unsigned)ivs), wg(256);
  hipLaunchKernelGGL(jpeg_dct_quant_kernel, per_block, wg, 0, st, frames, g, qt, blocks, coef);
  hipLaunchKernelGGL(jpeg_interval_bits_kernel, per_iv, wg, 0, st, coef, g, pos, iv_bits, scan);
  hipLaunchKernelGGL(jpeg_pack_kernel, per_block, wg, 0, st, coef, g, blocks, pos, scan);
  hipLaunchKernelGGL(jpeg_pad_count_kernel, per_iv, wg, 0, st, g, iv_bits, scan, iv_size);
  hipLaunchKernelGGL(jpeg_place_kernel, dim3(1), wg, 0, st, g, iv_size, iv_start, offsets);
  hipLaunchKernelGGL(jpeg_emit_kernel, per_iv, wg, 0, st, g, iv_bits, scan, iv_start, out, capacity);
  A2M_LAUNCH_CHECK();
  return A2M_OK;
}

}  // extern "C"
