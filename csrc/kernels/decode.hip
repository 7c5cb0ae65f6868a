// decode.hip — single-token (decode) attention over a KV cache for generation, gfx950.
//
// One new token per sequence: its packed projection row qkv[b] = [q (H·D) | k (Hkv·D) | v (Hkv·D)]
// attends to cache rows 0..pos[b] of its key/value heads, where row pos[b] IS the new token: the
// kernel writes its (RoPE-rotated) k and v into the cache and uses the register copies for that
// key, so append + attention are one launch.  The work is pure streaming (each cached key is 256 B
// of bf16 K+V read once for G = H/Hkv query heads: G FLOP/B), so the design is about keeping HBM
// busy, not MFMA:
//
//   * grid = B · Hkv · nchunks workgroups; a workgroup owns one key/value head of one sequence and
//     one chunk of keys (flash-decoding split): the host sizes chunks so a short batch still puts
//     ≥ 2 workgroups on each of the 256 CUs;
//   * 256 threads = 32 groups of 8 lanes; a group walks keys grp, grp+32, …  with each lane
//     holding 8 of the 64 dims, so one wave-instruction loads 8 consecutive 128-B rows (1 KiB,
//     coalesced); 4 keys per group are in flight per iteration (8 × 16-B loads per lane);
//   * q·k is an 8-lane sum over DPP (quad_perm xor 1, xor 2, then row_half_mirror) — no LDS;
//   * online softmax in the exp2 domain per group; groups merge across a wave by lane shuffles
//     and across the 4 waves through 4 KiB·G of LDS;
//   * with more than one chunk, each writes its partial (o/l in fp32, log2-sum-exp) and a second
//     small kernel merges them.  (Merging in the last-arriving chunk instead needs an agent-scope
//     release/acquire, which on gfx950 is an L2 writeback + invalidate per workgroup — the XCDs'
//     L2s are not coherent with each other — and measured 3-10x slower than the extra launch.)
//     The grid shapes depend only on the host's key bound, so a decode step captures into a HIP
//     graph with the positions living on the device.
//
// fp8 caches (`decode_kernel<G, true>`): a cache row is 64 B of OCP e4m3fn, no scales; it holds
// q8(r) = round-to-nearest-even(clamp(r, ±448)) of the bf16 row r a bf16 cache would hold (NaN
// stays NaN), so the rotated k is rounded twice, fp32 -> bf16 -> e4m3, like a prefilled row.  Only
// the loads and the one store differ: a lane holds its 8 dims as 8 B, a lane group covers one 64-B
// row, one wave instruction reads 512 contiguous bytes; v_cvt_pk_f32_fp8 unpacks into the same fp32
// lanes.  The new token's register copy is the stored bytes, so it attends to its own key and
// value as every later step will read them.
//
// A shared prefix (`decode_kernel<G, F8, true>`, op `decode_attn_shared`): several samples of one
// prompt.  Sequence s of S = B·group belongs to prompt s / group; its logical key j is row j of that
// prompt's prefix cache [B, Hkv, Tp, 64] for j < plen[s / group] and row j - plen of its own cache
// [S, Hkv, Ts, 64] from there on, so the prompt is held once and the `group` workgroups of a prompt
// read the same prefix rows.  Only the address of a key differs (base pointer and row index, chosen
// per key inside `load`); chunking, lane assignment, partials and the merge run over the logical
// index as before.  The prefix is never written: plen is clamped to [0, Tp] and pos to
// [plen, plen + Ts - 1] before anything is addressed, so the new row lands in the own cache.
// Not done here: one workgroup serving all `group` sequences of a prompt, so that a prefix row is
// loaded once for group·G queries — it needs another register layout (group·G accumulators per
// lane) and has no measurement behind it; today the sharing of loads is left to L2 and the MALL.
//
// Head dim D = 64 | 128 (`decode_kernel<D, G, F8, SHARED>`, taken from the caches' last dim; the
// text above describes 64).  A lane holds 8 dims at either width, so the per-lane registers are
// the same; at 128 a lane group is 16 lanes — one DPP row — and a workgroup has 16 of them: a row
// is 256 B of bf16 or 128 B of e4m3fn, one wave instruction reads 4 consecutive rows (the same
// 1 KiB / 512 B), q·k takes one more DPP step (row_mirror) after the 8-lane sum, the RoPE partner
// dims (±64) sit in lane d8 ^ 8 and the tables are [T, 64], a wave merges 4 groups, and the
// cross-wave merge and `merge_kernel` run on two waves (thread = dim).  `plan()` is shared: its
// chunk widths are multiples of 32 groups, hence of 16.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>

#include "nbd_common.h"

namespace nbd {
namespace decode {

constexpr int NT = 256;
constexpr int NW = NT / kWave;  // 4 waves
constexpr int NG = NT / 8;      // 32 lane groups at head dim 64 (16 at 128): the unit of plan()'s chunk widths
constexpr float kLog2e = 1.4426950408889634f;

struct Params {
  const uint16_t* qkv;  // [B, W] bf16 rows (row stride qkv_ld elements)
  int64_t qkv_ld;
  void* kc;  // [B, Hkv, Tmax, D] bf16, or e4m3fn (decode_kernel<D, G, true>)
  void* vc;
  const int64_t* pos;  // [B]
  const float* cos;    // [>= Tmax, D/2] or nullptr
  const float* sin;
  uint16_t* out;  // [B, H·D] bf16
  float* part_o;  // [B, H, nchunks, D]
  float* part_l;  // [B, H, nchunks]
  int H, Hkv, Tmax, nchunks, chunk;
  float scale2;  // softmax scale · log2(e)
  // decode_kernel<D, G, F8, true> only (kc / vc are then the own caches [S, Hkv, Tmax = Ts, D])
  const void* kpre;  // [S / group, Hkv, Tp, D], read only
  const void* vpre;
  const int64_t* plen;  // [S / group] valid prefix rows
  int Tp, group;
};

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// sum over the 8 lanes of a group; every lane gets the total
__device__ __forceinline__ float sum8(float v) {
  v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]: xor 1
  v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]: xor 2
  v += dpp<0x141>(v);  // row_half_mirror: lane i <- 7-i, i.e. the other quad of the 8
  return v;
}

// sum over the LG = 8 | 16 lanes of a group (16: one DPP row); every lane gets the total
template <int LG>
__device__ __forceinline__ float sum_group(float v) {
  v = sum8(v);
  if constexpr (LG == 16) v += dpp<0x140>(v);  // row_mirror: lane i <- 15-i, i.e. the other 8 of the 16
  return v;
}

__device__ __forceinline__ void unpack8(const u32x4& w, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = __uint_as_float(w[j] << 16);
    v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
}

__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
  u32x4 w;
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = pack2_bf16(v[2 * j], v[2 * j + 1]);
  return w;
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

// HF rotate_half RoPE on this lane's 8 dims [8·d8, 8·d8+8); the partner dims (±D/2) sit in lane
// d8 ^ D/16 (64: d8^4, 128: d8^8); table rows are D/2 floats
template <int D>
__device__ __forceinline__ void rope_lane(float (&x)[8], const float* cos, const float* sin, int64_t t, int d8) {
  constexpr int HL = D / 16;  // lanes per half row
  const float4* c4 = reinterpret_cast<const float4*>(cos + t * (D / 2) + (d8 & (HL - 1)) * 8);
  const float4* s4 = reinterpret_cast<const float4*>(sin + t * (D / 2) + (d8 & (HL - 1)) * 8);
  const float4 ca = c4[0], cb = c4[1], sa = s4[0], sb = s4[1];
  const float c[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
  const float s[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
  const float sg = d8 < HL ? -1.f : 1.f;  // x1·c − x2·s  |  x2·c + x1·s
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float y = __shfl_xor(x[e], HL, kWave);
    x[e] = x[e] * c[e] + sg * y * s[e];
  }
}

template <int D, int G, bool F8, bool SHARED>
__global__ __launch_bounds__(NT) void decode_kernel(Params p) {
  static_assert(D == 64 || D == 128, "head dim 64 or 128");
  constexpr int LG = D / 8;    // lanes per group: a lane holds 8 dims, a group one row
  constexpr int NGR = NT / LG;  // groups per workgroup: 32 | 16
  // keys in flight per group.  The same on an fp8 cache, though a load is half the bytes: twice
  // the keys measured equal at G = 1, 4-30 % slower at G = 3, 4 and 8 (G = 4, 8: over 256 VGPRs)
  // and 3 % faster in the one G = 6 shape tried (docs/FINDINGS.md).  The same with SHARED: the two
  // base pointers and plen cost 0-10 VGPRs, no instantiation spills and none loses a wave
  constexpr int U = G <= 4 ? 4 : 2;
  using row_t = typename Row<F8>::type;
  __shared__ float sm_m[NW][G], sm_l[NW][G];
  __shared__ float sm_o[NW][G][D];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = tid >> (LG == 8 ? 3 : 4), d8 = tid & (LG - 1);
  const int c = blockIdx.x % p.nchunks;
  const int bh = blockIdx.x / p.nchunks;
  const int b = bh / p.Hkv, kvh = bh % p.Hkv;
  // SHARED: keys [0, plen) are prefix rows of prompt b / group, key j >= plen is own row j - plen
  int plen = 0, pb = 0;
  if constexpr (SHARED) {
    pb = b / p.group;
    plen = (int)min<int64_t>(max<int64_t>(p.plen[pb], 0), p.Tp);
  }
  const int pos = (int)min<int64_t>(max<int64_t>(p.pos[b], plen), plen + p.Tmax - 1);
  const int len = pos + 1;
  const int c0 = c * p.chunk;
  const int c1 = min(c0 + p.chunk, len);

  // queries of the G heads sharing this kv head (scaled into the exp2 domain), and the new k / v
  const uint16_t* row = p.qkv + (int64_t)b * p.qkv_ld;
  float q[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    load8<bf16_t>(reinterpret_cast<const bf16_t*>(row + (kvh * G + g) * D + d8 * 8), q[g]);
    if (p.cos != nullptr) rope_lane<D>(q[g], p.cos, p.sin, pos, d8);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[g][e] *= p.scale2;
  }
  const int64_t head_base = ((int64_t)b * p.Hkv + kvh) * p.Tmax * D;
  // the new row as stored: on an fp8 cache the bf16 row is quantised here and the register copy
  // is those bytes, so the token attends to its own key and value as later steps will read them
  row_t knew, vnew;
  {
    float kf[8];
    load8<bf16_t>(reinterpret_cast<const bf16_t*>(row + (p.H + kvh) * D + d8 * 8), kf);
    if (p.cos != nullptr) rope_lane<D>(kf, p.cos, p.sin, pos, d8);
    const u32x4 kw = pack8(kf);
    const u32x4 vw = *reinterpret_cast<const u32x4*>(row + (p.H + p.Hkv + kvh) * D + d8 * 8);
    if constexpr (F8) {
      knew = quant8(kw);
      vnew = quant8(vw);
    } else {
      knew = kw;
      vnew = vw;
    }
  }
  // a row is LG row_t (one per lane of a group) in either format
  row_t* const kbase = static_cast<row_t*>(p.kc) + head_base / 8 + d8;
  row_t* const vbase = static_cast<row_t*>(p.vc) + head_base / 8 + d8;
  if (c0 <= pos && pos < c0 + p.chunk && grp == 0) {  // this chunk owns the new row
    kbase[(int64_t)(pos - plen) * LG] = knew;
    vbase[(int64_t)(pos - plen) * LG] = vnew;
  }
  const row_t* kpre = nullptr;
  const row_t* vpre = nullptr;
  if constexpr (SHARED) {
    const int64_t pre_base = ((int64_t)pb * p.Hkv + kvh) * p.Tp * D;
    kpre = static_cast<const row_t*>(p.kpre) + pre_base / 8 + d8;
    vpre = static_cast<const row_t*>(p.vpre) + pre_base / 8 + d8;
  }

  float m[G], l[G], o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
  }

  if (c0 < c1) {
    const row_t* kb = kbase;
    const row_t* vb = vbase;
    const int iters = (c1 - c0 + NGR * U - 1) / (NGR * U);
    // two register buffers: the keys / values of iteration it+1 are in flight while iteration it
    // is computed (a chunk is only a few iterations long, so each exposed round trip shows)
    auto load = [&](int it, int (&j)[U], row_t (&kr)[U], row_t (&vr)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        j[u] = c0 + grp + NGR * (it * U + u);
        const int jj = j[u] < c1 ? j[u] : c0;  // in-bounds address for a masked key
        if constexpr (SHARED) {  // jj <= pos: a prefix row below plen <= Tp, else own row jj - plen < Ts
          const bool pre = jj < plen;
          const int64_t r = (int64_t)(pre ? jj : jj - plen) * LG;
          kr[u] = (pre ? kpre : kb)[r];
          vr[u] = (pre ? vpre : vb)[r];
        } else {
          kr[u] = kb[(int64_t)jj * LG];
          vr[u] = vb[(int64_t)jj * LG];
        }
      }
    };
    auto compute = [&](const int (&j)[U], row_t (&kr)[U], row_t (&vr)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        // the new token: its row in memory may predate this launch's write.  A masked key
        // (j > pos) takes the register copy too: with c0 == pos its load above fetched that same
        // stale row, and 0 · v is NaN when the free row holds NaN or ±inf
        if (j[u] >= pos) {
          kr[u] = knew;
          vr[u] = vnew;
        }
      float s[U][G];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float kf[8];
        unpack8(kr[u], kf);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float acc = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc += q[g][e] * kf[e];
          acc = sum_group<LG>(acc);
          s[u][g] = j[u] < c1 ? acc : -INFINITY;
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float mx = m[g];
#pragma unroll
        for (int u = 0; u < U; ++u) mx = fmaxf(mx, s[u][g]);
        const float ms = mx == -INFINITY ? 0.f : mx;
        const float corr = exp2f(m[g] - ms);
        l[g] *= corr;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] *= corr;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float pu = exp2f(s[u][g] - ms);
          l[g] += pu;
          float vf[8];
          unpack8(vr[u], vf);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[g][e] += pu * vf[e];
        }
        m[g] = mx;
      }
    };
    int ja[U], jb[U];
    row_t ka[U], va[U], kbuf[U], vbuf[U];
    load(0, ja, ka, va);
    for (int it = 0; it < iters; it += 2) {
      if (it + 1 < iters) load(it + 1, jb, kbuf, vbuf);
      compute(ja, ka, va);
      if (it + 1 < iters) {
        if (it + 2 < iters) load(it + 2, ja, ka, va);
        compute(jb, kbuf, vbuf);
      }
    }
  }

  // merge the 64 / LG groups of this wave (lanes d8, d8+LG, …): 8 groups, or 4 (no xor-8 step)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float mx = m[g];
    if constexpr (LG == 8) mx = fmaxf(mx, __shfl_xor(mx, 8, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    const float w = mx == -INFINITY ? 0.f : exp2f(m[g] - mx);
    float lg = l[g] * w;
    if constexpr (LG == 8) lg += __shfl_xor(lg, 8, kWave);
    lg += __shfl_xor(lg, 16, kWave);
    lg += __shfl_xor(lg, 32, kWave);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = o[g][e] * w;
      if constexpr (LG == 8) x += __shfl_xor(x, 8, kWave);
      x += __shfl_xor(x, 16, kWave);
      x += __shfl_xor(x, 32, kWave);
      o[g][e] = x;
    }
    if (lane < LG) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm_o[wave][g][lane * 8 + e] = o[g][e];
      if (lane == 0) {
        sm_m[wave][g] = mx;
        sm_l[wave][g] = lg;
      }
    }
  }
  __syncthreads();

  // merge the 4 waves: thread = dim (wave 0; at head dim 128 waves 0 and 1)
  const int H = p.H;
  if (D == kWave ? wave == 0 : wave < D / kWave) {
    const int dim = D == kWave ? lane : tid;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mx = -INFINITY;
#pragma unroll
      for (int w = 0; w < NW; ++w) mx = fmaxf(mx, sm_m[w][g]);
      float L = 0.f, O = 0.f;
      if (mx != -INFINITY) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const float sc = exp2f(sm_m[w][g] - mx);
          L += sm_l[w][g] * sc;
          O += sm_o[w][g][dim] * sc;
        }
      }
      const int h = kvh * G + g;
      if (p.nchunks == 1) {
        p.out[(int64_t)b * H * D + h * D + dim] = f32_to_bf16(O / L);
      } else {
        const int64_t r = ((int64_t)b * H + h) * p.nchunks + c;
        p.part_o[r * D + dim] = L > 0.f ? O / L : 0.f;
        if (dim == 0) p.part_l[r] = L > 0.f ? mx + __log2f(L) : -INFINITY;
      }
    }
  }
}

// merge the chunk partials of one (b, head) row: D threads (one wave, or two at 128), thread = dim
template <int D>
__global__ __launch_bounds__(D) void merge_kernel(Params p) {
  const int r = blockIdx.x, lane = threadIdx.x;  // r = b·H + h
  const int64_t r0 = (int64_t)r * p.nchunks;
  float mx = -INFINITY;
  for (int k = 0; k < p.nchunks; ++k) mx = fmaxf(mx, p.part_l[r0 + k]);
  float L = 0.f, O = 0.f;
  for (int k = 0; k < p.nchunks; ++k) {
    const float lk = p.part_l[r0 + k];
    if (lk == -INFINITY) continue;
    const float w = exp2f(lk - mx);
    L += w;
    O += w * p.part_o[(r0 + k) * D + lane];
  }
  p.out[(int64_t)r * D + lane] = f32_to_bf16(O / L);
}

// chunking: enough workgroups for the chip (≥ 512 when the batch allows) with ≥ 256 keys per chunk;
// no split at all up to 512 keys, where the merge kernel's node would cost more than it saves
static void plan(int64_t BHkv, int64_t kv_len, int& nchunks, int& chunk) {
  int64_t nc = 1;
  if (kv_len > 512) {
    nc = std::max<int64_t>(1, (512 + BHkv - 1) / BHkv);
    nc = std::min<int64_t>(nc, (kv_len + 255) / 256);
    nc = std::min<int64_t>(nc, 64);
  }
  int64_t ch = (kv_len + nc - 1) / nc;
  ch = (ch + NG - 1) / NG * NG;
  nchunks = (int)((kv_len + ch - 1) / ch);
  chunk = (int)ch;
}

// the operands of decode_attn_shared that decode_attn has not
struct Shared {
  const at::Tensor& k_prefix;
  const at::Tensor& v_prefix;
  const at::Tensor& plen;
  int64_t group;
};

// both ops: `sh` == nullptr is decode_attn (k_cache / v_cache hold every row), else they are the
// sequences' own rows behind the prompts' prefixes
static at::Tensor decode_run(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                             const at::Tensor& pos, int64_t n_head, double scale, int64_t kv_len_max,
                             const c10::optional<at::Tensor>& rope_cos, const c10::optional<at::Tensor>& rope_sin,
                             const at::Tensor& partials, const Shared* sh) {
  const char* op = sh ? "decode_attn_shared" : "decode_attn";
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.dim() == 2 && qkv.stride(1) == 1 &&
                  qkv.stride(0) % 8 == 0 && ((uintptr_t)qkv.data_ptr() & 15) == 0,
              op, ": qkv must be a bf16 [B, (H + 2·Hkv)·D] GPU view, unit last stride, 16-B aligned rows");
  const bool f8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  // the head dim is the caches' last dim: k, v, and with a prefix those too, all alike
  TORCH_CHECK(k_cache.dim() == 4, op, ": caches must be [B, Hkv, Tmax, D], got ", k_cache.dim(), " dims");
  const int64_t D = k_cache.size(3);
  TORCH_CHECK(D == 64 || D == 128, op, ": head dim (the caches' last dim) must be 64 or 128, got ", D);
  auto check_caches = [&](const at::Tensor& k, const at::Tensor& v) {
    if (f8) {
      TORCH_CHECK(k.is_cuda() && k.is_contiguous() && k.dim() == 4 && k.size(3) == D && v.sizes() == k.sizes() &&
                      k.scalar_type() == at::kFloat8_e4m3fn && v.scalar_type() == at::kFloat8_e4m3fn &&
                      v.is_contiguous() && ((uintptr_t)k.data_ptr() & 7) == 0 && ((uintptr_t)v.data_ptr() & 7) == 0,
                  op, ": fp8 caches must be contiguous float8_e4m3fn [B, Hkv, Tmax, ", D, "], 8-B aligned rows");
    } else {
      TORCH_CHECK(k.is_cuda() && k.scalar_type() == at::kBFloat16 && k.is_contiguous() && k.dim() == 4 &&
                      k.size(3) == D && v.sizes() == k.sizes() && v.scalar_type() == at::kBFloat16 &&
                      v.is_contiguous() && ((uintptr_t)k.data_ptr() & 15) == 0 && ((uintptr_t)v.data_ptr() & 15) == 0,
                  op, ": caches must be contiguous bf16 [B, Hkv, Tmax, ", D, "]");
    }
  };
  check_caches(k_cache, v_cache);
  const int64_t B = qkv.size(0), Hkv = k_cache.size(1), Tmax = k_cache.size(2), H = n_head;
  TORCH_CHECK(k_cache.size(0) == B, op, ": cache batch ", k_cache.size(0), " != ", B);
  TORCH_CHECK(H > 0 && Hkv > 0 && H % Hkv == 0 && H / Hkv <= 8, op, ": need H % Hkv == 0 and H / Hkv <= 8");
  TORCH_CHECK(qkv.size(1) == (H + 2 * Hkv) * D, op, ": qkv width ", qkv.size(1), " != (H + 2·Hkv)·", D,
              " (H ", H, ", Hkv ", Hkv, ")");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kLong && pos.is_contiguous() && pos.numel() == B,
              op, ": pos must be a contiguous int64 [B] GPU tensor");
  int64_t Tp = 0;  // logical keys: Tp prefix rows (decode_attn: none), then the Tmax rows of k_cache
  if (sh) {
    TORCH_CHECK(sh->k_prefix.scalar_type() == k_cache.scalar_type() && sh->v_prefix.scalar_type() == k_cache.scalar_type(),
                op, ": prefix and own caches must have the same dtype (bf16 or float8_e4m3fn)");
    TORCH_CHECK(sh->k_prefix.dim() == 4 && sh->k_prefix.size(3) == D, op, ": prefix caches of head dim ",
                sh->k_prefix.dim() == 4 ? sh->k_prefix.size(3) : -1, " with own caches of head dim ", D);
    check_caches(sh->k_prefix, sh->v_prefix);
    Tp = sh->k_prefix.size(2);
    TORCH_CHECK(Tmax >= 1, op, ": the own caches need at least one row");
    TORCH_CHECK(sh->group >= 1 && B % sh->group == 0 && sh->k_prefix.size(0) == B / sh->group &&
                    sh->k_prefix.size(1) == Hkv,
                op, ": prefix caches must be [B / group, Hkv, Tp, ", D, "] for qkv [B, ...] (B ", B, ", group ", sh->group,
                ", prefix batch ", sh->k_prefix.size(0), ")");
    TORCH_CHECK(sh->plen.is_cuda() && sh->plen.scalar_type() == at::kLong && sh->plen.is_contiguous() &&
                    sh->plen.numel() == B / sh->group,
                op, ": plen must be a contiguous int64 [B / group] GPU tensor");
    TORCH_CHECK(sh->k_prefix.get_device() == qkv.get_device() && sh->v_prefix.get_device() == qkv.get_device() &&
                    sh->plen.get_device() == qkv.get_device() && k_cache.get_device() == qkv.get_device() &&
                    v_cache.get_device() == qkv.get_device() && pos.get_device() == qkv.get_device(),
                op, ": every operand must be on qkv's device");
    TORCH_CHECK(Tp + Tmax < (1LL << 31), op, ": too many rows");
    TORCH_CHECK(kv_len_max >= 1 && kv_len_max <= Tp + Tmax, op, ": kv_len_max must be in [1, Tp + Ts]");
  } else {
    TORCH_CHECK(kv_len_max >= 1 && kv_len_max <= Tmax, op, ": kv_len_max must be in [1, Tmax]");
  }
  const bool hc = rope_cos.has_value() && rope_cos->defined(), hs = rope_sin.has_value() && rope_sin->defined();
  TORCH_CHECK(hc == hs, op, ": rope_cos and rope_sin go together");
  if (hc)
    TORCH_CHECK(rope_cos->is_cuda() && rope_cos->scalar_type() == at::kFloat && rope_cos->is_contiguous() &&
                    rope_cos->dim() == 2 && rope_cos->size(1) == D / 2 && rope_cos->size(0) >= Tp + Tmax &&
                    rope_sin->sizes() == rope_cos->sizes() && rope_sin->is_contiguous() &&
                    rope_sin->scalar_type() == at::kFloat,
                op, ": rope tables must be contiguous float32 [>= ", sh ? "Tp + Ts" : "Tmax", ", ", D / 2,
                "] at head dim ", D);
  int nchunks, chunk;
  plan(B * Hkv, kv_len_max, nchunks, chunk);
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat && partials.is_contiguous() &&
                  partials.numel() >= B * H * nchunks * (D + 1),
              op, ": partials too small: need ", B * H * nchunks * (D + 1), " floats at head dim ", D);
  TORCH_CHECK(B * Hkv * nchunks < (1LL << 31) && Tmax * D * B * Hkv < (1LL << 62) && Tp * D * B * Hkv < (1LL << 62),
              op, ": grid too large");
  at::Tensor out = at::empty({B, H * D}, qkv.options().memory_format(at::MemoryFormat::Contiguous));
  Params p;
  p.qkv = static_cast<const uint16_t*>(qkv.data_ptr());
  p.qkv_ld = qkv.stride(0);
  p.kc = k_cache.data_ptr();
  p.vc = v_cache.data_ptr();
  p.pos = pos.data_ptr<int64_t>();
  p.cos = hc ? rope_cos->data_ptr<float>() : nullptr;
  p.sin = hc ? rope_sin->data_ptr<float>() : nullptr;
  p.out = static_cast<uint16_t*>(out.data_ptr());
  p.part_o = partials.data_ptr<float>();
  p.part_l = p.part_o + B * H * nchunks * D;
  p.H = (int)H;
  p.Hkv = (int)Hkv;
  p.Tmax = (int)Tmax;
  p.nchunks = nchunks;
  p.chunk = chunk;
  p.scale2 = (float)scale * kLog2e;
  p.kpre = sh ? sh->k_prefix.data_ptr() : nullptr;
  p.vpre = sh ? sh->v_prefix.data_ptr() : nullptr;
  p.plen = sh ? sh->plen.data_ptr<int64_t>() : nullptr;
  p.Tp = (int)Tp;
  p.group = sh ? (int)sh->group : 1;
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const dim3 grid((unsigned)(B * Hkv * nchunks));
  const bool wide = D == 128;
  switch (H / Hkv) {
#define NBD_DECODE_GFS(g, f, s)                                                         \
  if (wide)                                                                             \
    hipLaunchKernelGGL((decode_kernel<128, g, f, s>), grid, dim3(NT), 0, st, p);        \
  else                                                                                  \
    hipLaunchKernelGGL((decode_kernel<64, g, f, s>), grid, dim3(NT), 0, st, p)
#define NBD_DECODE_G(g)                    \
  case g:                                  \
    if (sh) {                              \
      if (f8) {                            \
        NBD_DECODE_GFS(g, true, true);     \
      } else {                             \
        NBD_DECODE_GFS(g, false, true);    \
      }                                    \
    } else if (f8) {                       \
      NBD_DECODE_GFS(g, true, false);      \
    } else {                               \
      NBD_DECODE_GFS(g, false, false);     \
    }                                      \
    break;
    NBD_DECODE_G(1)
    NBD_DECODE_G(2)
    NBD_DECODE_G(3)
    NBD_DECODE_G(4)
    NBD_DECODE_G(5)
    NBD_DECODE_G(6)
    NBD_DECODE_G(7)
    NBD_DECODE_G(8)
#undef NBD_DECODE_G
#undef NBD_DECODE_GFS
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  if (nchunks > 1) {
    if (wide)
      hipLaunchKernelGGL(merge_kernel<128>, dim3((unsigned)(B * H)), dim3(128), 0, st, p);
    else
      hipLaunchKernelGGL(merge_kernel<64>, dim3((unsigned)(B * H)), dim3(64), 0, st, p);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return out;
}

at::Tensor decode_attn_hip(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                           const at::Tensor& pos, int64_t n_head, double scale, int64_t kv_len_max,
                           const c10::optional<at::Tensor>& rope_cos, const c10::optional<at::Tensor>& rope_sin,
                           const at::Tensor& partials) {
  return decode_run(qkv, k_cache, v_cache, pos, n_head, scale, kv_len_max, rope_cos, rope_sin, partials, nullptr);
}

// sequence s of qkv [S = B·group, ...] reads k_prefix / v_prefix [B, Hkv, Tp, D] rows [0, plen[s / group]) and
// its own rows k_own / v_own [S, Hkv, Ts, D]; pos [S] are absolute positions, kv_len_max <= Tp + Ts
at::Tensor decode_attn_shared_hip(const at::Tensor& qkv, const at::Tensor& k_prefix, const at::Tensor& v_prefix,
                                  const at::Tensor& plen, const at::Tensor& k_own, const at::Tensor& v_own,
                                  const at::Tensor& pos, int64_t group, int64_t n_head, double scale,
                                  int64_t kv_len_max, const c10::optional<at::Tensor>& rope_cos,
                                  const c10::optional<at::Tensor>& rope_sin, const at::Tensor& partials) {
  const Shared sh{k_prefix, v_prefix, plen, group};
  return decode_run(qkv, k_own, v_own, pos, n_head, scale, kv_len_max, rope_cos, rope_sin, partials, &sh);
}

// ============================================================================ greedy advance
// The end of a greedy decode step in one launch: per sequence b, tok[b] = argmax(logits[b])
// (first index among equal maxima, like torch.argmax); finished rows keep emitting eos (done[b]
// sticks once eos appears); pos[b] += 1; out[b, pos[b]] = tok[b].  One 1024-thread workgroup per
// row, 16-B loads (8 logits per lane per step), wave then LDS arg-max reduction.  Replaces torch's
// arg-max reduction (≈19 µs on a 50k vocabulary row) plus three bookkeeping kernels.
constexpr int GT = 1024;

__device__ __forceinline__ void argmax_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__global__ __launch_bounds__(GT) void greedy_kernel(const uint16_t* __restrict__ logits, int64_t ld, int V,
                                                    int64_t* __restrict__ tok, int64_t* __restrict__ pos,
                                                    int64_t* __restrict__ out, int64_t out_ld, int out_T,
                                                    bool* __restrict__ done, int64_t eos) {
  __shared__ float sv[GT / kWave];
  __shared__ int si[GT / kWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint16_t* row = logits + (int64_t)b * ld;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  const int V8 = (((uintptr_t)row & 15) == 0) ? V / 8 * 8 : 0;
  for (int v = tid * 8; v < V8; v += GT * 8) {
    float f[8];
    load8<bf16_t>(reinterpret_cast<const bf16_t*>(row + v), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) argmax_merge(best, bi, f[e], v + e);
  }
  for (int v = V8 + tid; v < V; v += GT) argmax_merge(best, bi, bf16_to_f32(row[v]), v);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float v2 = __shfl_xor(best, off, kWave);
    const int i2 = __shfl_xor(bi, off, kWave);
    argmax_merge(best, bi, v2, i2);
  }
  if ((tid & 63) == 0) {
    sv[tid >> 6] = best;
    si[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < GT / kWave; ++w) argmax_merge(best, bi, sv[w], si[w]);
    int64_t t = bi == 0x7fffffff ? 0 : bi;  // an all-NaN row picks token 0
    if (done != nullptr) {
      if (done[b]) t = eos;
      if (t == eos) done[b] = true;
    }
    tok[b] = t;
    const int64_t p = pos[b] + 1;
    pos[b] = p;
    if (p >= 0 && p < out_T) out[(int64_t)b * out_ld + p] = t;
  }
}

void greedy_advance_hip(const at::Tensor& logits, const at::Tensor& tok, const at::Tensor& pos, const at::Tensor& out,
                        const c10::optional<at::Tensor>& done, int64_t eos) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 && logits.dim() == 2 && logits.stride(1) == 1,
              "greedy_advance: logits must be a bf16 [B, V] GPU view with unit last stride");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (1LL << 31) && B >= 1 && B < (1LL << 31), "greedy_advance: bad shape");
  auto chk = [&](const at::Tensor& t, at::ScalarType ty, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() && t.dim() == 1 && t.size(0) == B,
                "greedy_advance: ", name, " must be a contiguous [B] GPU tensor of ", ty);
  };
  chk(tok, at::kLong, "tok");
  chk(pos, at::kLong, "pos");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.dim() == 2 && out.size(0) == B && out.stride(1) == 1,
              "greedy_advance: out must be an int64 [B, T] GPU view with unit last stride");
  const bool hd = done.has_value() && done->defined();
  if (hd) chk(*done, at::kBool, "done");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  hipLaunchKernelGGL(greedy_kernel, dim3((unsigned)B), dim3(GT), 0, st, static_cast<const uint16_t*>(logits.data_ptr()),
                     logits.stride(0), (int)V, tok.data_ptr<int64_t>(), pos.data_ptr<int64_t>(), out.data_ptr<int64_t>(),
                     out.stride(0), (int)out.size(1), hd ? done->data_ptr<bool>() : nullptr, eos);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace decode
}  // namespace nbd

TORCH_LIBRARY_IMPL(nbd, CUDA, m) {
  m.impl("decode_attn", &nbd::decode::decode_attn_hip);
  m.impl("decode_attn_shared", &nbd::decode::decode_attn_shared_hip);
  m.impl("greedy_advance", &nbd::decode::greedy_advance_hip);
}
