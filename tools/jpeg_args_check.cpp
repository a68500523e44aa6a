// Stand-alone check of the host code of csrc/jpeg.hip (the argument checks of a2m_jpeg_encode_u8,
// the quantiser tables it copies, the workspace arithmetic of a2m_jpeg_ws_bytes) under the host
// sanitizers.  Every call returns before a launch, so it runs on a machine without a GPU:
//
//   cd audio-to-motion-generation_amd
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       ../tools/jpeg_args_check.cpp csrc/jpeg.hip csrc/capi.cpp -o build/jpeg_args_check
//   build/jpeg_args_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/a2m.h"

static int failures = 0;
#define EXPECT(call, want)                                                              \
  do {                                                                                  \
    const long long rc_ = (long long)(call);                                            \
    if (rc_ != (long long)(want)) {                                                     \
      std::printf("line %d: got %lld, want %lld (%s)\n", __LINE__, rc_, (long long)(want), a2m_last_error()); \
      ++failures;                                                                       \
    }                                                                                   \
  } while (0)

int main() {
  std::vector<uint8_t> dev(64);   // stands in for device memory: never dereferenced on the host
  uint8_t* d = dev.data();
  int64_t* off = reinterpret_cast<int64_t*>(d);
  // exactly 64 entries each: a read past either end is a sanitizer report
  std::vector<uint16_t> ql(64, 16), qc(64, 255);
  const size_t big = (size_t)1 << 40;

  EXPECT(a2m_jpeg_encode_u8(nullptr, 0, 13, 9, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr), A2M_OK);
  EXPECT(a2m_jpeg_encode_u8(d, 0, 0, 9, ql.data(), qc.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, -1, 13, 9, ql.data(), qc.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 65536, 9, ql.data(), qc.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 65536, ql.data(), qc.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, ql.data(), qc.data(), d, -1, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(nullptr, 1, 13, 9, ql.data(), qc.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, nullptr, qc.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, ql.data(), nullptr, d, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, ql.data(), qc.data(), nullptr, 8, off, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, ql.data(), qc.data(), d, 8, nullptr, d, big, nullptr), A2M_EINVAL);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, ql.data(), qc.data(), d, 8, off, nullptr, big, nullptr), A2M_EINVAL);
  for (int i : {0, 63}) {                                     // the first and the last entry are read
    for (int bad : {0, 256}) {
      std::vector<uint16_t> q(64, 16);
      q[i] = (uint16_t)bad;
      EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, q.data(), qc.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
      EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, ql.data(), q.data(), d, 8, off, d, big, nullptr), A2M_EINVAL);
    }
  }
  // the workspace: refused sizes give 0, the largest frame does not overflow, one byte short is refused
  EXPECT(a2m_jpeg_ws_bytes(0, 13, 9), 0);
  EXPECT(a2m_jpeg_ws_bytes(1, 0, 9), 0);
  EXPECT(a2m_jpeg_ws_bytes(1, 13, 65536), 0);
  EXPECT(a2m_jpeg_ws_bytes(INT32_MAX, 65535, 65535), 0);      // more blocks than one launch takes
  const size_t small = a2m_jpeg_ws_bytes(1, 13, 9), huge = a2m_jpeg_ws_bytes(42, 65535, 65535);
  EXPECT(small >= 12 * (128 + 4 + 208) && small < 12 * (128 + 4 + 208) + 4096, 1);
  EXPECT(huge > (size_t)42 * 8192 * 8192 * 3 * 340, 1);
  EXPECT(a2m_jpeg_encode_u8(d, 1, 13, 9, ql.data(), qc.data(), d, 8, off, d, small - 1, nullptr), A2M_EINVAL);
  // more blocks than one launch takes: refused before any launch, whatever the workspace
  EXPECT(a2m_jpeg_encode_u8(d, INT32_MAX, 65535, 65535, ql.data(), qc.data(), d, 8, off, d, ~(size_t)0, nullptr),
         A2M_EINVAL);

  std::printf(failures ? "%d check(s) failed\n" : "jpeg_args_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
