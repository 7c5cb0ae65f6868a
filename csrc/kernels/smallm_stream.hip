// smallm_stream.hip — the small-M decode linear past what smallm.hip's register-resident weights
// take (K > 4096, or 2048 with SwiGLU): the MLP products of the 1 B – 8 B models, gfx950.
//
//     out[m, n] = epilogue( prologue(x)[m, :] · W[n, :] ),   M ≤ 64, K % 32 == 0, K ≤ 32768
//
// with smallm.hip's prologues (none | LayerNorm | RMSNorm), epilogues (bias, GELU | SwiGLU,
// residual) and MFMA mapping: 512 threads, v_mfma_f32_16x16x32_bf16 with A = 16 weight rows (16
// gate + 16 up rows with SwiGLU) and B = xᵀ, lane group l/16 walking its own contiguous quarter of
// the k range so that a lane streams 16-B pieces of one weight row in address order, the 8 waves'
// partial tiles summed through LDS.  What differs:
//
//   work split   grid = (column tiles of 16) × (S K-slices).  Slice s owns the MFMA steps
//                [s·steps/S, (s+1)·steps/S) of steps = K/32 (uneven where S does not divide them),
//                and inside a slice wave w owns [w·n/8, (w+1)·n/8) of its n steps, as in smallm.hip.
//                A workgroup computes all ⌈M/16⌉ m-tiles of its column tile: smallm.hip falls back
//                to one m-tile per workgroup and a grid dimension over row groups when the column
//                tiles leave CUs idle or the x image is too large, and re-reads the weights per
//                row group.  Here the K-slices fill the chip and shrink the x image instead, and
//                every weight byte is read exactly once whatever M is (the accumulators cost
//                4·MT registers per weight matrix).
//   plan         stream_plan(): S = 1 when the column tiles alone give every CU a workgroup, else
//                the fewest slices that do, never below 1024 k per slice (32 steps: 4 per wave);
//                from there the first S at which the x slice [M, K/S] fits in LDS.
//   weights      never through LDS (each byte is used once): a ring of R = 3 chunks of 4 16-B loads
//                per lane (C = 4 k-steps, or 2 with SwiGLU's two matrices) in registers.  The loads
//                of chunks c+1 and c+2 are in flight under the MFMAs of chunk c: 8 KiB per wave,
//                64 KiB per workgroup.  K is bounded by indexing only.
//   x            the workgroup's slice [M, slice] staged in LDS (M rows, not MT·16; rows ≥ M read
//                as zeros).  Where even the plan's slice does not fit and there is no norm, the
//                fragments come straight from global memory (L2), as in smallm.hip's stage == 0.
//   norm         row statistics need the whole row: every workgroup computes mean and rstd over
//                all of K from global memory (two passes, fp32, smallm.hip's formula) and
//                normalises its own slice into LDS with the same bf16 rounding.
//   finishing    S == 1: the epilogue and the bf16 store happen here, one node.  S > 1: the
//                workgroup stores its fp32 partial tile to ws[S, (2 with SwiGLU), M, N] and
//                stream_finish_kernel sums the slices in slice order and applies the epilogue.
//                No atomics and no workgroup waits for another; results are deterministic.
//
// Register budget: no scratch, and at most 128 VGPRs up to 48 rows, so that two workgroups fit a
// CU when their LDS does (4 waves per SIMD).  The ring is 12 × 4 = 48 VGPRs, the accumulators
// 4·MT (8·MT with SwiGLU), the x fragments of a step 4·MT.  With 49 – 64 rows (MT = 4) the kernel
// takes 129 (131) VGPRs, one workgroup per CU — which the x image of that many rows allows
// anyway.  The compiler's report (-Rpass-analysis=kernel-resource-usage) is kept at the kernel.
#include <mutex>
#include <set>
#include <c10/hip/HIPException.h>

#include <algorithm>

#include "smallm.h"

namespace nbd {
namespace smallm {

constexpr int kCUs = 256;        // MI355X
constexpr int R = 3;             // chunks in the weight ring
constexpr int kChunkLoads = 4;   // 16-B weight loads per lane and chunk
constexpr int kMinSliceSteps = 32;  // 1024 k: a wave keeps at least one chunk

// bias → GELU → SwiGLU → residual, the order and the fp32 formulas of smallm.hip's epilogue
template <int ACT>
__device__ __forceinline__ uint16_t finish(const Args& a, float v0, float v1, float b, float r) {
  float y = v0;
  if (a.bias != nullptr) y += b;
  if (ACT == ACT_GELU) y = gelu_tanh(y);
  if (ACT == ACT_SWIGLU) y = silu(y) * v1;
  if (a.res != nullptr) y += r;
  return f32_to_bf16(y);
}

// rows [0, M) of x[:, k0 : k0 + sk] into xs[M][sk + XPAD].  Without a norm a plain copy; with one,
// wave w takes rows w, w+8, …: their statistics over the whole row from global memory (the rows of
// a wave interleaved, so their loads and cross-lane sums overlap), then its slice normalised
template <int MT>
__device__ __forceinline__ void stage_x(const Args& a, int k0, int sk, uint16_t* xs, int tid) {
  const int ld = sk + XPAD, M = a.M;
  if (a.norm == NORM_NONE) {
    const int total = M * sk;
#pragma unroll 4
    for (int idx = tid * 8; idx < total; idx += NT * 8) {
      const int r = idx / sk, c = idx - r * sk;
      *reinterpret_cast<u32x4*>(xs + r * ld + c) = *reinterpret_cast<const u32x4*>(a.x + (int64_t)r * a.ldx + k0 + c);
    }
    return;
  }
  constexpr int RPW = MT * 16 / NW;  // rows per wave
  const int lane = tid & 63, wave = tid >> 6;
  float s[RPW], q[RPW], mean[RPW], rstd[RPW];
#pragma unroll
  for (int j = 0; j < RPW; ++j) s[j] = q[j] = 0.f;
  if (a.norm == NORM_LN) {
    for (int c = lane * 8; c < a.K; c += kWave * 8) {
#pragma unroll
      for (int j = 0; j < RPW; ++j) {
        const int r = wave + NW * j;
        if (r < M) {
          float f[8];
          unpack8(*reinterpret_cast<const u32x4*>(a.x + (int64_t)r * a.ldx + c), f);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[j] += f[e];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RPW; ++j) mean[j] = a.norm == NORM_LN ? wave_sum(s[j]) / (float)a.K : 0.f;
  for (int c = lane * 8; c < a.K; c += kWave * 8) {  // two passes, like the standalone kernels
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int r = wave + NW * j;
      if (r < M) {
        float f[8];
        unpack8(*reinterpret_cast<const u32x4*>(a.x + (int64_t)r * a.ldx + c), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = f[e] - mean[j];
          q[j] = fmaf(d, d, q[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RPW; ++j) rstd[j] = rsqrtf(wave_sum(q[j]) / (float)a.K + a.eps);
  for (int c = lane * 8; c < sk; c += kWave * 8) {
    float g[8], b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unpack8(*reinterpret_cast<const u32x4*>(a.nw + k0 + c), g);
    if (a.norm == NORM_LN) unpack8(*reinterpret_cast<const u32x4*>(a.nb + k0 + c), b);
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int r = wave + NW * j;
      if (r < M) {
        float f[8], o[8];
        unpack8(*reinterpret_cast<const u32x4*>(a.x + (int64_t)r * a.ldx + k0 + c), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf((f[e] - mean[j]) * rstd[j], g[e], b[e]);
        store8<bf16_t>(reinterpret_cast<bf16_t*>(xs + r * ld + c), o);
      }
    }
  }
}

// Compiler's report (gfx950, -O3), VGPRs of <MT, none | GELU | SwiGLU, STAGED>, each with 0 AGPRs
// and 0 B of scratch: MT 1: 92 | 92 | 94, MT 2: 104 | 104 | 106, MT 3: 116 | 116 | 118, MT 4: 129 |
// 129 | 131; unstaged 69 | 69 | 79, 75 | 75 | 89, 85 | 85 | 99, 93 | 93 | 111.
// stream_finish_kernel: 13 VGPRs, no LDS.
// STAGED: the x slice is in LDS.  The steady loop has no branch in it: a step past the wave's
// last one loads that last step's (in-bounds) weights again and multiplies them by a zero x
// fragment, and rows >= M read row M - 1 and are zeroed the same way — so the compiler counts the
// loads in flight (s_waitcnt vmcnt(n > 0)) where a guarded load would make it wait for all of them.
template <int MT, int ACT, bool STAGED>
__global__ __launch_bounds__(NT) void linear_stream_kernel(Args a, float* __restrict__ ws, int S) {
  constexpr int NACC = ACT == ACT_SWIGLU ? 2 : 1;
  constexpr int C = kChunkLoads / NACC;  // k-steps per chunk
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int M = a.M;
  uint16_t* xs = reinterpret_cast<uint16_t*>(smem);
  float* red = reinterpret_cast<float*>(smem);  // reuses the x image once the MFMA loop is over

  // this workgroup's slice of K, and this wave's steps of it
  const int tile = blockIdx.x, sl = blockIdx.y;
  const int steps = a.K >> 5;
  const int t0 = sl * steps / S, nst = (sl + 1) * steps / S - t0;
  const int k0 = t0 * 32, sk = nst * 32;
  const int s0 = wave * nst / NW, ns = (wave + 1) * nst / NW - s0;
  const int kg = g * (sk >> 2) + s0 * 8;  // lane group g walks its own contiguous quarter of the slice
  const int ldx_s = sk + XPAD;

  const int nr = min(tile * 16 + li, a.N - 1);  // clamped for a ragged last tile
  const uint16_t* w0 = a.w + (int64_t)nr * a.K + k0 + kg;
  const uint16_t* w1 = a.w + (int64_t)(a.up_off + nr) * a.K + k0 + kg;
  const uint16_t* xg = a.x + k0 + kg;
  const int last = max(ns - 1, 0);  // (a wave that owns nothing still loads in bounds: s0 < nst)

  s8v ring[R][C][NACC];
  auto load_chunk = [&](int slot, int c) {
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int st = min(c * C + i, last);
      ring[slot][i][0] = __builtin_nontemporal_load(reinterpret_cast<const s8v*>(w0 + st * 8));
      if (ACT == ACT_SWIGLU)
        ring[slot][i][NACC - 1] = __builtin_nontemporal_load(reinterpret_cast<const s8v*>(w1 + st * 8));
    }
  };
  f4 acc[NACC][MT];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = f4{0.f, 0.f, 0.f, 0.f};
  auto mma_chunk = [&](int slot, int c) {
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int st = min(c * C + i, last);
      const bool live = c * C + i < ns;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int m = t * 16 + li, mr = min(m, M - 1);
        s8v xf = STAGED ? *reinterpret_cast<const s8v*>(xs + mr * ldx_s + kg + st * 8)
                        : *reinterpret_cast<const s8v*>(xg + (int64_t)mr * a.ldx + st * 8);
        if (!(live && m < M)) xf = s8v{0, 0, 0, 0, 0, 0, 0, 0};
        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[slot][i][0], xf, acc[0][t], 0, 0, 0);
        if (ACT == ACT_SWIGLU)
          acc[NACC - 1][t] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[slot][i][NACC - 1], xf, acc[NACC - 1][t], 0, 0, 0);
      }
    }
  };

  // the first R - 1 chunks are in flight before anything else: the x staging overlaps them
#pragma unroll
  for (int r = 0; r < R - 1; ++r) load_chunk(r, r);
  // one slice: the epilogue's operands (bias, residual) are fetched now, not after the reduction
  constexpr int QPT = (MT * 256 + NT - 1) / NT;
  float pre_b[QPT], pre_r[QPT];
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const int q = tid + u * NT, t = q >> 8, p = q & 255;
    const int ml = t * 16 + (p >> 4), n = tile * 16 + (p & 15);
    const bool ok = S == 1 && q < MT * 256 && ml < M && n < a.N;
    pre_b[u] = ok && a.bias != nullptr ? bf16_to_f32(a.bias[n]) : 0.f;
    pre_r[u] = ok && a.res != nullptr ? bf16_to_f32(a.res[(int64_t)ml * a.N + n]) : 0.f;
  }
  if (STAGED) {
    stage_x<MT>(a, k0, sk, xs, tid);
    __syncthreads();
  }

  // chunk c's MFMAs run from slot c % R while chunk c + R - 1 loads into the slot chunk c - 1 left
  const int nch = (ns + C - 1) / C;
  for (int c0 = 0; c0 < nch; c0 += R) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      load_chunk((r + R - 1) % R, c0 + r + R - 1);
      mma_chunk(r, c0 + r);
    }
  }

  __syncthreads();  // every wave is done with the x image: red takes its place
  // partial tiles of the 8 waves -> LDS: red[wave][j][t][m_local][n_local]
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t)
      *reinterpret_cast<f4*>(red + (((wave * NACC + j) * MT + t) * 256) + li * 16 + 4 * g) = acc[j][t];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const int q = tid + u * NT;
    if (q >= MT * 256) break;
    const int t = q >> 8, p = q & 255;
    const int ml = t * 16 + (p >> 4), n = tile * 16 + (p & 15);
    float v0 = 0.f, v1 = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      v0 += red[((w * NACC + 0) * MT + t) * 256 + p];
      if (ACT == ACT_SWIGLU) v1 += red[((w * NACC + 1) * MT + t) * 256 + p];
    }
    if (ml < M && n < a.N) {
      const int64_t o = (int64_t)ml * a.N + n;
      if (S == 1) {
        a.out[o] = finish<ACT>(a, v0, v1, pre_b[u], pre_r[u]);
      } else {
        const int64_t mn = (int64_t)M * a.N;
        ws[(int64_t)sl * NACC * mn + o] = v0;
        if (ACT == ACT_SWIGLU) ws[((int64_t)sl * NACC + 1) * mn + o] = v1;
      }
    }
  }
}

// out = epilogue(Σ_s ws[s]) with the slices summed in slice order; one thread per output element
template <int ACT>
__global__ __launch_bounds__(256) void stream_finish_kernel(Args a, const float* __restrict__ ws, int S) {
  constexpr int NACC = ACT == ACT_SWIGLU ? 2 : 1;
  const int64_t mn = (int64_t)a.M * a.N;
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= mn) return;
  const int n = (int)(o % a.N);
  float v0 = 0.f, v1 = 0.f;
  for (int s = 0; s < S; ++s) {
    v0 += ws[(int64_t)s * NACC * mn + o];
    if (ACT == ACT_SWIGLU) v1 += ws[((int64_t)s * NACC + 1) * mn + o];
  }
  const float b = a.bias != nullptr ? bf16_to_f32(a.bias[n]) : 0.f;
  const float r = a.res != nullptr ? bf16_to_f32(a.res[o]) : 0.f;
  a.out[o] = finish<ACT>(a, v0, v1, b, r);
}

size_t stream_lds_bytes(int M, int K, int S, int act, bool staged) {
  const int MT = (M + 15) / 16, steps = K / 32;
  const size_t red = (size_t)NW * (act == ACT_SWIGLU ? 2 : 1) * MT * 256 * 4;
  const size_t xs = staged ? (size_t)M * ((steps + S - 1) / S * 32 + XPAD) * 2 : 0;  // the largest slice
  return std::max(red, xs);
}

int stream_plan(int M, int N, int K, int norm, int act) {
  const int ntiles = (N + 15) / 16, steps = K / 32;
  const int smax = std::min(kStreamMaxSlices, std::max(1, steps / kMinSliceSteps));
  int S = 1;
  while (ntiles * S < kCUs && S < smax) ++S;
  for (int s = S; s <= smax; ++s)
    if (stream_lds_bytes(M, K, s, act, true) <= kMaxLds) return s;
  if (norm == NORM_NONE) return S;  // x fragments from global memory
  // a norm needs the image in LDS: thinner slices than 1024 k, or none
  for (int s = smax + 1; s <= std::min(kStreamMaxSlices, steps); ++s)
    if (stream_lds_bytes(M, K, s, act, true) <= kMaxLds) return s;
  return 0;
}

void launch_stream(Args a, int act, int S, float* ws, hipStream_t st, int device) {
  const int MT = (a.M + 15) / 16;
  a.ntiles = (a.N + 15) / 16;
  // the x slice goes to LDS whenever it fits (a norm prologue requires it: the caller checked)
  a.stage = a.norm != NORM_NONE || stream_lds_bytes(a.M, a.K, S, act, true) <= kMaxLds;
  const size_t lds = stream_lds_bytes(a.M, a.K, S, act, a.stage != 0);
  auto launch = [&](auto kern) {
    // keyed by (device, kernel pointer), as in smallm.hip
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    const void* fp = reinterpret_cast<const void*>(kern);
    {
      std::lock_guard<std::mutex> lk(mu);
      if (done.insert({device, fp}).second)
        C10_HIP_CHECK(hipFuncSetAttribute(fp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)a.ntiles, (unsigned)S), dim3(NT), lds, st, a, ws, S);
  };
  const bool staged = a.stage != 0;
#define NBD_SMALLM_STREAM_ACT(mt, act_)                                    \
  if (staged) launch(linear_stream_kernel<mt, act_, true>);                \
  else launch(linear_stream_kernel<mt, act_, false>);
#define NBD_SMALLM_STREAM(mt)                                              \
  case mt:                                                                 \
    if (act == ACT_NONE) { NBD_SMALLM_STREAM_ACT(mt, ACT_NONE) }           \
    else if (act == ACT_GELU) { NBD_SMALLM_STREAM_ACT(mt, ACT_GELU) }      \
    else { NBD_SMALLM_STREAM_ACT(mt, ACT_SWIGLU) }                         \
    break;
  switch (MT) {
    NBD_SMALLM_STREAM(1)
    NBD_SMALLM_STREAM(2)
    NBD_SMALLM_STREAM(3)
    NBD_SMALLM_STREAM(4)
  }
#undef NBD_SMALLM_STREAM
#undef NBD_SMALLM_STREAM_ACT
  if (S == 1) return;
  const unsigned blocks = (unsigned)(((int64_t)a.M * a.N + 255) / 256);
  if (act == ACT_NONE) hipLaunchKernelGGL(stream_finish_kernel<ACT_NONE>, dim3(blocks), dim3(256), 0, st, a, ws, S);
  else if (act == ACT_GELU) hipLaunchKernelGGL(stream_finish_kernel<ACT_GELU>, dim3(blocks), dim3(256), 0, st, a, ws, S);
  else hipLaunchKernelGGL(stream_finish_kernel<ACT_SWIGLU>, dim3(blocks), dim3(256), 0, st, a, ws, S);
}

}  // namespace smallm
}  // namespace nbd
