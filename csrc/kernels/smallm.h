// smallm.h — what the two small-M decode linear units share: smallm.hip (a wave keeps a column
// tile's weights in registers, K ≤ 4096) and smallm_stream.hip (weights streamed through a
// register ring, K split over workgroups).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nbd_common.h"

namespace nbd {
namespace smallm {

constexpr int NT = 512;
constexpr int NW = NT / kWave;  // 8 waves
constexpr int XPAD = 8;         // bf16 elements of row padding in the LDS x image (bank spread)
constexpr size_t kMaxLds = 160 * 1024;

enum Norm { NORM_NONE = 0, NORM_LN = 1, NORM_RMS = 2 };
enum Act { ACT_NONE = 0, ACT_GELU = 1, ACT_SWIGLU = 2 };

typedef float f4 __attribute__((ext_vector_type(4)));
typedef short s8v __attribute__((ext_vector_type(8)));

struct Args {
  const uint16_t* x;  // [M, K] bf16, row stride ldx
  int64_t ldx;
  const uint16_t* w;  // [N_w, K] bf16 contiguous
  const uint16_t* bias;  // [N] or nullptr
  const uint16_t* nw;    // norm γ [K] or nullptr
  const uint16_t* nb;    // LayerNorm β [K] or nullptr
  const uint16_t* res;   // [M, N] or nullptr (row stride N)
  uint16_t* out;         // [M, N]
  int M, N, K, norm, stage, ntiles, up_off;  // stage: x image in LDS; up_off: SwiGLU's first up row
  float eps;
};

__device__ __forceinline__ float gelu_tanh(float x) {
  const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
  return x * __fdividef(1.f, 1.f + __expf(-2.f * u));
}
__device__ __forceinline__ float silu(float x) { return x * __fdividef(1.f, 1.f + __expf(-x)); }

__device__ __forceinline__ void unpack8(const u32x4& w, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = __uint_as_float(w[j] << 16);
    v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// ---- the streaming kernel (smallm_stream.hip) -------------------------------------------------
constexpr int kStreamMaxK = 32768;
constexpr int kStreamMaxSlices = 16;

// K-slices the streaming kernel's plan takes for this problem; 0 = it refuses (a norm prologue
// whose x slice fits in LDS at no slice count)
int stream_plan(int M, int N, int K, int norm, int act);
// bytes of LDS the streaming kernel needs with S slices; staged: the x slice goes through LDS
size_t stream_lds_bytes(int M, int K, int S, int act, bool staged);
// launches the streaming kernel (and, with S > 1, its finishing kernel) on st; ws: fp32
// [S, (2 with SwiGLU), M, N] when S > 1.  a.stage and a.ntiles are set by the callee.
void launch_stream(Args a, int act, int S, float* ws, hipStream_t st, int device);

}  // namespace smallm
}  // namespace nbd
