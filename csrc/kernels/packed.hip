// packed.hip — document bounds of packed rows for the SEG attention kernels (attn.hip).
//
// A packed row holds several documents back to back; ``position_ids`` restarts at 0 where a
// document starts (transformers' DataCollatorWithFlattening).  A document starts at t == 0 or
// wherever position_ids[b, t] == 0.  One launch, one wave per row (as mask.hip), turns that into
// the two arrays the kernels read:
//
//   kstart[b, i] = start of query i's document           (the query-on-lane kernels: forward, dQ)
//   qend[b, j]   = one past the end of key j's document  (the key-on-lane kernel: dK/dV)
//
// Query i sees key j iff kstart[i] <= j <= i, equivalently j <= i < qend[j].  Both arrays are
// non-decreasing along the row; the attention kernels rely on that (wave / workgroup bounds are
// read at the first and last row they own), which holds because only this op produces them.
//
//   bad |= 1 if a row is not consecutive inside a document: pos[t] != pos[t-1] + 1 and pos[t] != 0
//
// `bad` is read lazily by the caller (models/llama.py _MaskCheck: pinned copy + event, no sync).
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPException.h>
#include <torch/library.h>

#include <climits>

#include "nbd_common.h"

namespace nbd {
namespace packed {

constexpr int kThreads = 256;  // 4 waves = 4 rows per workgroup; one wave per row

// One wave per row, 64 positions per step.  kstart is an inclusive running maximum of the start
// marks (t where a document starts, else -1) swept forward, qend an exclusive running minimum of
// the same marks (else T) swept backward: in-wave scans by shuffles, the carry between steps in a
// wave-uniform register — no LDS, no barrier.
__global__ __launch_bounds__(kThreads) void packed_bounds_kernel(const int64_t* __restrict__ pos, int64_t B, int T,
                                                                 int32_t* __restrict__ kstart,
                                                                 int32_t* __restrict__ qend,
                                                                 int32_t* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (b >= B) return;  // (wave-uniform)
  const int64_t* row = pos + b * T;
  int32_t* ks = kstart + b * T;
  int32_t* qe = qend + b * T;
  int carry = 0, flag = 0;
  for (int c = 0; c < T; c += 64) {
    const int t = c + lane;
    int v = -1;
    if (t < T) {
      const int64_t p = row[t];
      if (t == 0 || p == 0) v = t;
      else if (p != row[t - 1] + 1) flag = 1;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v = max(v, u);
    }
    v = max(v, carry);
    if (t < T) ks[t] = v;
    carry = __shfl(v, 63, 64);
  }
  carry = T;
  for (int c = ((T - 1) / 64) * 64; c >= 0; c -= 64) {
    const int t = c + lane;
    int v = INT_MAX;
    if (t < T && t != 0 && row[t] == 0) v = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_down(v, o, 64);
      if (lane + o < 64) v = min(v, u);
    }
    v = min(v, carry);  // the first start at or after t
    const int nxt = __shfl_down(v, 1, 64);
    if (t < T) qe[t] = lane == 63 ? carry : nxt;  // the first start after t
    carry = __shfl(v, 0, 64);
  }
  flag |= __shfl_xor(flag, 32, 64);
  flag |= __shfl_xor(flag, 16, 64);
  flag |= __shfl_xor(flag, 8, 64);
  flag |= __shfl_xor(flag, 4, 64);
  flag |= __shfl_xor(flag, 2, 64);
  flag |= __shfl_xor(flag, 1, 64);
  if (lane == 0 && flag) atomicOr(bad, 1);
}

// (kstart [B, T] int32, qend [B, T] int32); ORs 1 into bad[0] for a row that is not consecutive
// inside a document
std::tuple<at::Tensor, at::Tensor> packed_bounds_hip(const at::Tensor& pos, at::Tensor bad) {
  TORCH_CHECK(pos.is_cuda() && pos.dim() == 2 && pos.scalar_type() == at::kLong && pos.is_contiguous(),
              "packed_bounds: position_ids must be a contiguous int64 [B, T] GPU tensor");
  TORCH_CHECK(bad.is_cuda() && bad.scalar_type() == at::kInt && bad.numel() >= 1, "packed_bounds: bad must be int32");
  const int64_t B = pos.size(0), T = pos.size(1);
  TORCH_CHECK(T < (1LL << 30), "packed_bounds: row too long");
  auto kstart = at::empty({B, T}, pos.options().dtype(at::kInt));
  auto qend = at::empty({B, T}, pos.options().dtype(at::kInt));
  if (B == 0 || T == 0) return {kstart, qend};
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(pos.device());
  const hipStream_t st = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const dim3 grid((unsigned)((B + kThreads / 64 - 1) / (kThreads / 64))), block(kThreads);
  hipLaunchKernelGGL(packed_bounds_kernel, grid, block, 0, st, pos.data_ptr<int64_t>(), B, (int)T,
                     kstart.data_ptr<int32_t>(), qend.data_ptr<int32_t>(), bad.data_ptr<int32_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {kstart, qend};
}

}  // namespace packed
}  // namespace nbd

TORCH_LIBRARY_IMPL(nbd, CUDA, m) { m.impl("packed_bounds", &nbd::packed::packed_bounds_hip); }
