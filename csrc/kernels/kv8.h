// kv8.h — the fp8 KV cache row format, shared by decode.hip and append.hip.
//
// A cache row is D bytes of OCP e4m3fn, no scales; it holds q8(r) = round-to-nearest-even(
// clamp(r, ±448)) of the bf16 row r a bf16 cache would hold (NaN stays NaN).  A thread's unit is 8
// consecutive dims: 16 B of bf16 (u32x4) or 8 B of e4m3fn (u32x2).  Every e4m3 value is exact in
// bf16, so reading a row back rounds nothing.
#pragma once
#include "nbd_common.h"

namespace nbd {

__device__ __forceinline__ void unpack8(const u32x4& w, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = __uint_as_float(w[j] << 16);
    v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
}

// a lane's 8 dims of a cache row: 16 B of bf16 or 8 B of e4m3fn; either way a row is D/8 of them
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <bool F8>
struct Row {
  using type = u32x4;
};
template <>
struct Row<true> {
  using type = u32x2;
};

__device__ __forceinline__ void unpack8(const u32x2& w, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);  // bytes 0, 1
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);   // bytes 2, 3
    v[4 * j] = lo[0];
    v[4 * j + 1] = lo[1];
    v[4 * j + 2] = hi[0];
    v[4 * j + 3] = hi[1];
  }
}

// q8 of 8 bf16 values: clamp to ±448 (±inf saturates; e4m3fn has no inf), round to nearest even.
// NaN is kept out of the clamp (fminf / fmaxf — v_min / v_max / v_med3 — return the other operand)
// and its byte is written here, 0x7f with the sign: what a cast makes of NaN is then no question.
__device__ __forceinline__ u32x2 quant8(const u32x4& w) {
  float f[8];
  unpack8(w, f);
  float c[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) c[e] = f[e] != f[e] ? 0.f : fminf(fmaxf(f[e], -448.f), 448.f);
  u32x2 r;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int x = 0;
    x = __builtin_amdgcn_cvt_pk_fp8_f32(c[4 * j], c[4 * j + 1], x, false);
    x = __builtin_amdgcn_cvt_pk_fp8_f32(c[4 * j + 2], c[4 * j + 3], x, true);
    r[j] = (uint32_t)x;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (f[e] != f[e]) r[e >> 2] |= (0x7fu | (__float_as_uint(f[e]) >> 31 << 7)) << (8 * (e & 3));
  return r;
}

// 8 e4m3 bytes -> the 8 bf16 values they stand for, element order kept.  v_cvt_pk_f32_fp8 makes two
// fp32 values of two bytes; their high halves are the bf16 values (nothing is rounded: an e4m3
// significand has 3 bits), and one v_perm_b32 per pair puts the two halves into a dword.
__device__ __forceinline__ u32x4 widen8(const u32x2& w) {
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);  // bytes 0, 1
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);   // bytes 2, 3
    // selector: result bytes 0, 1 = bytes 2, 3 of the second operand; bytes 2, 3 = those of the first
    r[2 * j] = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
    r[2 * j + 1] = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
  }
  return r;
}

}  // namespace nbd
