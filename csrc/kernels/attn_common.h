// attn_common.h — device helpers shared by the MFMA attention units (attn.hip: flash forward /
// backward; append.hip: a block of new tokens over a KV cache): the v_mfma_f32_32x32x16_bf16
// operand and accumulator helpers, the fused RoPE rotation and the K/V tile staging.  The
// operand maps are documented in attn.hip's header.
#pragma once
#include <stdint.h>

#include "nbd_common.h"

namespace nbd {
namespace attn {

typedef short s8v __attribute__((ext_vector_type(8)));
typedef short s4v __attribute__((ext_vector_type(4)));
typedef float f16x __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) s4v lds_s4v;

constexpr int D = 64;
constexpr int NT = 256;     // threads per workgroup (4 waves)
constexpr int BLK = 128;    // rows owned by a workgroup (queries in fwd/dq, keys in dkdv)
constexpr int TILE = 64;    // rows per swept tile
constexpr int RS = 72;      // LDS row stride (elements) of row-read images: 144 B
constexpr int RSV = 96;     // LDS row stride of transpose-only images: 192 B (tr reads conflict-free)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kDeferLog2 = 4.f;  // forward: skip the O rescale while the max grows by <= 2^4

struct View {
  const uint16_t* p;
  int64_t sb, sh, st;  // element strides of batch, head, row; d is contiguous
  __device__ __forceinline__ const uint16_t* row(int b, int h, int t) const { return p + b * sb + h * sh + t * st; }
};
struct MView {
  uint16_t* p;
  int64_t sb, sh, st;
  __device__ __forceinline__ uint16_t* row(int b, int h, int t) const { return p + b * sb + h * sh + t * st; }
};

__device__ __forceinline__ f16x mfma(s8v a, s8v b, f16x c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ s8v ld16(const uint16_t* p) { return *reinterpret_cast<const s8v*>(p); }
__device__ __forceinline__ void st16(uint16_t* p, s8v v) { *reinterpret_cast<s8v*>(p) = v; }
__device__ __forceinline__ s4v tr4(const uint16_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(p));
}
__device__ __forceinline__ s8v cat(s4v a, s4v b) {
  s8v r;
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3];
  r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
  return r;
}
__device__ __forceinline__ uint16_t bf(float x) { return f32_to_bf16(x); }
// registers 8s .. 8s+7 of a C tile -> bf16 B/A fragment of k-step s (k order as §3)
__device__ __forceinline__ s8v pack_half(const f16x& c, int s) {
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = pack2_bf16(c[8 * s + 2 * j], c[8 * s + 2 * j + 1]);
  return __builtin_bit_cast(s8v, w);
}
__device__ __forceinline__ int crow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
__device__ __forceinline__ f16x zero16() {
  f16x z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// store a 32x32 C tile whose rows are d (= db*32 + row) and columns a row index of `out`
// (lane&31): 4 consecutive d per 8-byte store
__device__ __forceinline__ void store_dT(uint16_t* rowp, const f16x& c, int db, int h, float mul) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const uint32_t lo = pack2_bf16(c[4 * g] * mul, c[4 * g + 1] * mul);
    const uint32_t hi = pack2_bf16(c[4 * g + 2] * mul, c[4 * g + 3] * mul);
    const int d = db * 32 + 8 * g + 4 * h;
    *reinterpret_cast<uint2*>(rowp + d) = make_uint2(lo, hi);
  }
}

// rotary embedding fused into the loads (HF rotate_half convention): dims d and d+32 of a row
// rotate by the angle of (row position, d); cos/sin = [T_max, 32] fp32 tables, nullptr = no RoPE
struct Rope {
  const float* cos;
  const float* sin;
};

// rotate 8 consecutive dims [d0, d0+8) of x (with their partners d+32 in y) for position t
__device__ __forceinline__ void rope8(s8v& x, s8v& y, const Rope& rp, int t, int d0) {
  const float4* c4 = reinterpret_cast<const float4*>(rp.cos + (int64_t)t * 32 + d0);
  const float4* s4 = reinterpret_cast<const float4*>(rp.sin + (int64_t)t * 32 + d0);
  const float4 ca = c4[0], cb = c4[1], sa = s4[0], sb = s4[1];
  const float c[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
  const float sn[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = bf16_to_f32((uint16_t)x[j]), b = bf16_to_f32((uint16_t)y[j]);
    x[j] = (short)bf(a * c[j] - b * sn[j]);
    y[j] = (short)bf(b * c[j] + a * sn[j]);
  }
}

// Q or K fragments of one row held in registers (element s covers dims 16s + 8h + [0, 8)):
// pairs (f[0], f[2]) and (f[1], f[3])
__device__ __forceinline__ void rope_frag(s8v (&f)[4], const Rope& rp, int t, int h) {
  rope8(f[0], f[2], rp, t, 8 * h);
  rope8(f[1], f[3], rp, t, 16 + 8 * h);
}

// dQ/dK tiles: acc0 holds dims [0, 32), acc1 dims [32, 64) — a d/d+32 pair shares register i of
// one lane, so the transpose rotation (gradient of the forward rotation) is applied right here
__device__ __forceinline__ void store_dT_rope(uint16_t* rowp, const f16x& a0, const f16x& a1, int h, float mul,
                                              const Rope& rp, int t) {
  const float* cr = rp.cos + (int64_t)t * 32;
  const float* sr = rp.sin + (int64_t)t * 32;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint16_t lo[4], hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int d = 8 * g + 4 * h + e;
      const float x = a0[4 * g + e] * mul, y = a1[4 * g + e] * mul;
      lo[e] = bf(x * cr[d] + y * sr[d]);
      hi[e] = bf(y * cr[d] - x * sr[d]);
    }
    const int d = 8 * g + 4 * h;
    *reinterpret_cast<uint2*>(rowp + d) =
        make_uint2((uint32_t)lo[0] | ((uint32_t)lo[1] << 16), (uint32_t)lo[2] | ((uint32_t)lo[3] << 16));
    *reinterpret_cast<uint2*>(rowp + 32 + d) =
        make_uint2((uint32_t)hi[0] | ((uint32_t)hi[1] << 16), (uint32_t)hi[2] | ((uint32_t)hi[3] << 16));
  }
}

// tile staging with the two halves of a row in one thread (row = tid/4, chunks q and q+4), so
// the rotation can be applied between the global load and the LDS store
struct StagePair {
  s8v a, b;
  __device__ __forceinline__ void load(const uint16_t* base, int64_t st, int tid) {
    const uint16_t* p = base + (tid >> 2) * st + (tid & 3) * 8;
    a = ld16(p);
    b = ld16(p + 32);
  }
  __device__ __forceinline__ void rope(const Rope& rp, int t0, int tid) {
    if (rp.cos != nullptr) rope8(a, b, rp, t0 + (tid >> 2), (tid & 3) * 8);
  }
  __device__ __forceinline__ void store(uint16_t* lds, int stride, int tid) const {
    uint16_t* p = lds + (tid >> 2) * stride + (tid & 3) * 8;
    st16(p, a);
    st16(p + 32, b);
  }
};

// cooperative tile staging: 64 rows x 64 d, 512 16-B chunks, 2 per thread
struct Stage2 {
  s8v a[2];
  __device__ __forceinline__ void load(const uint16_t* base, int64_t st, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + i * NT;
      a[i] = ld16(base + (c >> 3) * st + (c & 7) * 8);
    }
  }
  __device__ __forceinline__ void store(uint16_t* lds, int stride, int tid) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + i * NT;
      st16(lds + (c >> 3) * stride + (c & 7) * 8, a[i]);
    }
  }
};

// ---------------------------------------------------------------------------------------------
// head-dim-generic forms, used by append.hip only (D = 64 | 128).  At D = 64 each expands to the
// fixed-width helper above it is named after; attn.hip keeps the fixed ones.

// rope8 with the tables' row stride (= D/2, the distance to the rotation partner) as a parameter:
// x holds dims [d0, d0+8), y their partners [d0 + HALF, d0 + HALF + 8); cos/sin = [T_max, HALF]
template <int HALF>
__device__ __forceinline__ void rope8_hd(s8v& x, s8v& y, const Rope& rp, int t, int d0) {
  const float4* c4 = reinterpret_cast<const float4*>(rp.cos + (int64_t)t * HALF + d0);
  const float4* s4 = reinterpret_cast<const float4*>(rp.sin + (int64_t)t * HALF + d0);
  const float4 ca = c4[0], cb = c4[1], sa = s4[0], sb = s4[1];
  const float c[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
  const float sn[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = bf16_to_f32((uint16_t)x[j]), b = bf16_to_f32((uint16_t)y[j]);
    x[j] = (short)bf(a * c[j] - b * sn[j]);
    y[j] = (short)bf(b * c[j] + a * sn[j]);
  }
}

// rope_frag over D/16 fragments (element s covers dims 16s + 8h + [0, 8)): the partner of
// fragment s is fragment s + D/32 — (f[0], f[2]), (f[1], f[3]) at 64; (f[s], f[s + 4]) at 128
template <int D>
__device__ __forceinline__ void rope_frag_hd(s8v (&f)[D / 16], const Rope& rp, int t, int h) {
#pragma unroll
  for (int s = 0; s < D / 32; ++s) rope8_hd<D / 2>(f[s], f[s + D / 32], rp, t, 16 * s + 8 * h);
}

// Stage2 for 64 rows x D dims: 8·D 16-B chunks, D/32 per thread, D/8 consecutive threads per row
// (a wave's load covers whole rows; 8 consecutive lanes of a ds_write_b128 cover 128 contiguous
// bytes = all 32 banks once)
template <int D>
struct StageRows {
  s8v a[D / 32];
  __device__ __forceinline__ void store(uint16_t* lds, int stride, int tid) const {
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const int c = tid + i * NT;
      st16(lds + (c >> (D == 64 ? 3 : 4)) * stride + (c & (D / 8 - 1)) * 8, a[i]);
    }
  }
};

}  // namespace attn
}  // namespace nbd
