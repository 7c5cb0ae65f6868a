// append.hip — attention of a block of new tokens over a KV cache (multi-turn append), gfx950.
//
// The middle between attn.hip (square causal T x T, no cache) and decode.hip (one query per
// sequence): sequence b brings nnew[b] <= Tn new tokens (rows of a packed projection
// qkv[b, i] = [q (H·64) | k (Hkv·64) | v (Hkv·64)], rows i >= nnew[b] are padding) that continue a
// cache holding start[b] valid rows.  New token i sits at position start[b] + i: its k (rotated at
// that position when RoPE tables are given) and v become cache row start[b] + i, and its query
// (rotated at the same position) attends cache rows 0 .. start[b] + i.  start / nnew live on the
// device, nothing synchronises, and both grids depend on host values only — the op captures into
// a HIP graph.
//
// Choices:
//   * two launches.  append_kv_kernel (elementwise, 4 threads per (b, i, kv head) row) rotates
//     and writes k | v into the cache; append_attn_kernel then reads every key, the new ones
//     included, from the cache — stream order makes them visible.  No workgroup reads a row that
//     another workgroup of the same launch writes (what that costs across XCDs: decode.hip).
//   * the attention kernel is fwd_kernel's body (attn.hip; the device helpers are shared through
//     attn_common.h): one workgroup = 4 waves = 128 new tokens of one (batch, head), a wave owns
//     32 queries on v_mfma_f32_32x32x16_bf16 with the query on the lane; 64-key K/V tiles staged
//     through LDS from the cache — one more strided view — with the next tile's loads in flight
//     under the current tile's math; online softmax in the exp2 domain with the deferred rescale.
//     K comes rotated from the cache and is not rotated again.
//   * the diagonal is key = start[b] + i, and start is not tile aligned: a lane carries its last
//     visible key `lim`, a wave the first / last lane's (lim0 / lim31, wave-uniform).  Tiles past
//     lim31 are skipped, compares run only in the 32x32 blocks that hold a key > lim0.
//   * padding queries (i >= nnew[b]) take the last valid query's limit, so no lane ever sees an
//     empty row (every sweep starts at tile 0 and key 0 <= every lim: the running maximum is
//     finite after the first tile, and exp2(-inf - (-inf)) is never reached with m = -inf as the
//     start); their result is dropped and exact zeros are stored.  A wave or workgroup whose
//     queries are all padding runs no MFMA but meets every barrier.
//   * the sweep of a workgroup ends at the tile of its last valid query — a device value, uniform
//     in the workgroup.  Cache rows >= start[b] + nnew[b] (never written here, possibly stale or
//     NaN) are replaced by zeros as a tile is staged: a masked key's p is exactly 0, and 0 · NaN
//     must not reach O.
//   * start / nnew are clamped before they address anything: 0 <= start <= L - 1 and
//     0 <= nnew <= min(Tn, L - start) with L = min(Tmax, kv_len_max); row indices of staged
//     tiles and of padding queries are clamped into their tensors on top of that.
//   * no split over keys: the grid is B · H · ceil(Tn / 128) workgroups (heaviest query block
//     first) and each sweeps its keys sequentially.  docs/FINDINGS.md has what that costs for
//     batch 1 over a long history.
// Tn needs no padding: the kernel clamps its query loads and bounds its stores at Tn.
//
// Head dim: both kernels take it as a template parameter, D = 64 | 128 (the host reads it from the
// caches' last dim); "64" above stands for D.  The algorithm is the same; what follows D:
//   * a lane holds D/16 query fragments, S takes D/16 MFMA k-steps per 32-key block, O is D/32
//     accumulator tiles per wave (64 fp32 registers per lane at 128); the RoPE partner of dim d is
//     d ± D/2 — fragment s with fragment s + D/32 — and the tables are [>= Tmax, D/2].
//   * append_kv_kernel keeps one (16-B chunk, partner chunk) pair of k and of v per thread, so a
//     row takes D/16 threads: 8 at 128, not 4 threads with two pairs each — a thread's loads in
//     flight and its registers stay what they are at 64, the kernel is elementwise (more threads
//     are only more parallelism), and 8 consecutive lanes read a contiguous 128-B half row.
//   * LDS images.  K rows are D + 8 elements (row reads with ds_read_b128: at 128 a row is 68
//     dwords, so row r starts at bank 4·(r mod 16) and the 16 lanes that ds_read_b128 serves at
//     once — 16 distinct r mod 16 — cover the 64 banks once, as the 36-dword rows do at 64).
//     V rows are RSV = 96 elements at 64 and 160 at 128.  A 32-lane half of ds_read_b64_tr_b16
//     reads 4 rows q x 16 dwords (two 16-lane groups x four 8-byte pieces); the rows must land
//     on different quarters of the 64 banks: row stride / 4 B = 48 (96 el) or 80 (160 el), both
//     = ±16 mod 64, put rows 0..3 at banks {0, 48, 32, 16} and {0, 16, 32, 48} — conflict-free; 128 + 8
//     or 192 elements do not.  160 is the smallest such stride >= 128.  At 128 the images are
//     64·136·2 + 64·160·2 = 17 408 + 20 480 = 37 888 B per workgroup (64: 21 504 B).
//   * K and V tiles at 128 are staged by StageRows (16 consecutive threads per 256-B row).  The 64
//     tile keeps StagePair (K) and Stage2 (V) — StagePair is the layout the flash forward needs
//     for its rotation, which this kernel inherited; nothing here rotates a staged tile, so 128
//     does not pay its two-way ds_write bank conflict (8 lanes = two 64-B pieces 4 banks apart).
//   * the 64 instantiations are, instruction for instruction, the kernels they were before the
//     head dim became a parameter; two places are written out for that (`if constexpr (D == 64)`
//     in load_tile and around the output stores).
//   * registers (docs/FINDINGS.md §46 has the compiler's report): the 128 instantiation holds
//     32 more O, 16 more Q and 16 more staged-tile registers per lane than the 64 one.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "attn_common.h"
#include "nbd_common.h"

namespace nbd {
namespace attn {

struct AppendParams {
  const uint16_t* qkv;  // [B, Tn, (H + 2·Hkv)·D] bf16, element strides sb / st, unit last stride
  int64_t sb, st;
  uint16_t* kc;  // [B, Hkv, Tmax, D] bf16, contiguous
  uint16_t* vc;
  const int64_t* start;  // [B]
  const int64_t* nnew;   // [B]
  uint16_t* out;         // [B, Tn, H·D] bf16, contiguous
  Rope rp;
  int H, Hkv, Tn, Tmax, L, nqb;  // L = min(Tmax, kv_len_max): the clamp of start + nnew
  float sc2;                     // softmax scale · log2(e)
};

// the clamped (start, nnew) of sequence b: s0 + n <= L <= Tmax, n <= Tn
struct Span {
  int s0, n;
};
__device__ __forceinline__ Span span_of(const AppendParams& p, int b) {
  Span s;
  s.s0 = (int)min<int64_t>(max<int64_t>(p.start[b], 0), p.L - 1);
  s.n = (int)min<int64_t>(max<int64_t>(p.nnew[b], 0), min(p.Tn, p.L - s.s0));
  return s;
}

__device__ __forceinline__ s8v zero8() {
  s8v z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = 0;
  return z;
}

// ============================================================================ cache append
// thread = (b, i, kv head, c), c < D/16: dims [8c, 8c + 8) and their rotation partners
// [D/2 + 8c, D/2 + 8c + 8) of k, the same two 16-B chunks of v
template <int D>
__global__ __launch_bounds__(NT) void append_kv_kernel(AppendParams p, int64_t total) {
  static_assert(D == 64 || D == 128, "head dim 64 or 128");
  constexpr int HALF = D / 2;
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const int c = (int)(g & (D / 16 - 1));
  const int64_t rowi = g >> (D == 64 ? 2 : 3);
  const int kvh = (int)(rowi % p.Hkv);
  const int i = (int)(rowi / p.Hkv % p.Tn);
  const int b = (int)(rowi / p.Hkv / p.Tn);
  const Span sp = span_of(p, b);
  if (i >= sp.n) return;  // padding: nothing lands in the cache
  const int t = sp.s0 + i;
  const uint16_t* row = p.qkv + b * p.sb + i * p.st;
  const uint16_t* ks = row + (p.H + kvh) * D + c * 8;
  const uint16_t* vs = row + (p.H + p.Hkv + kvh) * D + c * 8;
  s8v ka = ld16(ks), kb = ld16(ks + HALF);
  if (p.rp.cos != nullptr) rope8_hd<HALF>(ka, kb, p.rp, t, c * 8);
  const int64_t dst = (((int64_t)b * p.Hkv + kvh) * p.Tmax + t) * D + c * 8;
  st16(p.kc + dst, ka);
  st16(p.kc + dst + HALF, kb);
  st16(p.vc + dst, ld16(vs));
  st16(p.vc + dst + HALF, ld16(vs + HALF));
}

// ============================================================================ attention
// occupancy: the 64 instantiation fits two waves per SIMD (171 VGPRs).  Under the same bound the
// 128 one needs 256 VGPRs and 44 B of scratch per lane (the compiler's resource report), so it is
// built for one wave per SIMD, where it spills nothing.
template <int D>
__global__ __launch_bounds__(NT, D == 64 ? 2 : 1) void append_attn_kernel(AppendParams p) {
  static_assert(D == 64 || D == 128, "head dim 64 or 128");
  constexpr int RS = D + 8;                // K image row stride (elements): row reads
  constexpr int RSV = D == 64 ? 96 : 160;  // V image row stride: transposed reads (header: banks)
  constexpr int NS = D / 16;               // MFMA k-steps of q·k = query fragments per lane
  constexpr int NDB = D / 32;              // 32-dim blocks of O
  __shared__ __attribute__((aligned(16))) uint16_t Ks[TILE * RS];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[TILE * RSV];
  const int BH = gridDim.x / p.nqb;
  const int bh = blockIdx.x % BH;
  const int qb = p.nqb - 1 - blockIdx.x / BH;  // the last query block sweeps the most keys: first
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Span sp = span_of(p, b);
  const int s0 = sp.s0, n = sp.n;
  const int nl = max(n - 1, 0);        // the last valid query
  const int kend = s0 + n;             // cache rows >= kend hold nothing of this sequence
  const int q0 = qb * BLK + w * 32;    // this wave's first query
  const int qi = q0 + r;               // this lane's query
  const bool live = q0 < n;            // wave-uniform: some query of the wave is real
  const int lim = s0 + min(qi, nl);    // this lane's last visible key (= its position)
  const int lim0 = s0 + min(q0, nl);   // the wave's smallest / largest
  const int lim31 = s0 + min(q0 + 31, nl);
  const int kh = hh / (p.H / p.Hkv);   // GQA: the key/value head of this query head
  // the workgroup's sweep: up to the tile of its last valid query (none: all padding)
  const int ntiles = qb * BLK < n ? (s0 + min(qb * BLK + BLK - 1, nl)) / TILE + 1 : 0;

  s8v qf[NS];
  {
    const uint16_t* qrow = p.qkv + b * p.sb + (int64_t)min(qi, p.Tn - 1) * p.st + hh * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = ld16(qrow + 16 * s + 8 * h);
  }
  if (p.rp.cos != nullptr) rope_frag_hd<D>(qf, p.rp, lim, h);
  f16x acc_o[NDB] = {};
  float m = -INFINITY, l = 0.f;

  const uint16_t* kbase = p.kc + ((int64_t)b * p.Hkv + kh) * p.Tmax * D;
  const uint16_t* vbase = p.vc + ((int64_t)b * p.Hkv + kh) * p.Tmax * D;
  // the 64 tile keeps the fixed staging structs, so that instantiation stays the kernel it was
  std::conditional_t<D == 64, StagePair, StageRows<D>> sk;
  std::conditional_t<D == 64, Stage2, StageRows<D>> sv;
  // a tile's rows from the cache (row index clamped into it); rows >= kend become zeros
  auto load_rows = [&](StageRows<D>& sr, const uint16_t* base, int k0) {  // (128)
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const int c = tid + i * NT;
      const int vr = k0 + (c >> (D == 64 ? 3 : 4));
      sr.a[i] = ld16(base + (int64_t)min(vr, p.Tmax - 1) * D + (c & (D / 8 - 1)) * 8);
      if (vr >= kend) sr.a[i] = zero8();
    }
  };
  auto load_tile = [&](int k0) {
    if constexpr (D == 64) {
      const int kr = k0 + (tid >> 2);
      const uint16_t* pk = kbase + (int64_t)min(kr, p.Tmax - 1) * D + (tid & 3) * 8;
      sk.a = ld16(pk);
      sk.b = ld16(pk + 32);
      if (kr >= kend) sk.a = sk.b = zero8();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = tid + i * NT;
        const int vr = k0 + (c >> 3);
        sv.a[i] = ld16(vbase + (int64_t)min(vr, p.Tmax - 1) * D + (c & 7) * 8);
        if (vr >= kend) sv.a[i] = zero8();
      }
    } else {
      load_rows(sk, kbase, k0);
      load_rows(sv, vbase, k0);
    }
  };
  load_tile(0);
  sk.store(Ks, RS, tid);
  sv.store(Vs, RSV, tid);
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) load_tile((t + 1) * TILE);  // issue the next tile's loads now, write them after this tile
    const int k0 = t * TILE;
    // one tile; DIAG = some key of it lies past the wave's first limit (only those pay for compares)
    auto tile_body = [&](auto diag_c) {
      constexpr bool DIAG = decltype(diag_c)::value;
      // DIAG: the second 32-key block lies wholly past this wave's limits when lim31 falls in the
      // first (skip1: no S / P·V MFMAs, P = 0); a block wholly at or before lim0 needs no mask
      const bool skip1 = DIAG && k0 + 32 > lim31;
      f16x sacc[2] = {zero16(), zero16()};
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && skip1) break;
#pragma unroll
        for (int s = 0; s < NS; ++s) sacc[kb] = mfma(ld16(Ks + (kb * 32 + r) * RS + 16 * s + 8 * h), qf[s], sacc[kb]);
      }
      float mt = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if constexpr (DIAG) {
          if (kb == 1 && skip1) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[1][i] = -INFINITY;
            continue;
          }
          if (k0 + kb * 32 + 31 > lim0) {  // the diagonal key = start + i crosses this block
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (k0 + kb * 32 + crow(i, h) > lim) sacc[kb][i] = -INFINITY;
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) mt = fmaxf(mt, sacc[kb][i]);
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      // deferred rescale, as fwd_kernel: m moves only when some query's maximum grew by > 2^kDeferLog2
      const float mn = fmaxf(m, mt * p.sc2);
      if (__any(mn > m + kDeferLog2)) {
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        l *= alpha;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc_o[db][i] *= alpha;
        m = mn;
      }
      const float nmn = -m;
      float rs0 = 0.f, rs1 = 0.f;  // two chains; scalar adds (no v_pk_add_f32: -fno-slp-vectorize)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], p.sc2, nmn));
          const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i + 1], p.sc2, nmn));
          sacc[kb][i] = p0;
          sacc[kb][i + 1] = p1;
          rs0 += p0;
          rs1 += p1;
        }
      float rs = rs0 + rs1;
      rs += __shfl_xor(rs, 32, 64);
      l += rs;
      // O^T[d][q] += V^T[d][key] . P[key][q]
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        if (kb == 1 && skip1) break;  // P = 0 there
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const s8v pb = pack_half(sacc[kb], s);
          const int key = kb * 32 + 16 * s + 4 * h + (lane & 15) / 4;
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const uint16_t* base = Vs + key * RSV + db * 32 + (lane & 16) + 4 * (lane & 3);
            acc_o[db] = mfma(cat(tr4(base), tr4(base + 8 * RSV)), pb, acc_o[db]);
          }
        }
      }
    };
    if (live && k0 <= lim31) {
      if (k0 + TILE - 1 > lim0)
        tile_body(std::true_type{});
      else
        tile_body(std::false_type{});
    }
    __syncthreads();
    if (t + 1 < ntiles) {
      sk.store(Ks, RS, tid);
      sv.store(Vs, RSV, tid);
      __syncthreads();
    }
  }
  if (qi < p.Tn) {
    uint16_t* orow = p.out + (((int64_t)b * p.Tn + qi) * p.H + hh) * D;
    if (qi < n) {
      const float inv = 1.f / l;
      if constexpr (D == 64) {  // written out: as a loop the 64 kernel gets another schedule (same instructions)
        store_dT(orow, acc_o[0], 0, h, inv);
        store_dT(orow, acc_o[1], 1, h, inv);
      } else {
#pragma unroll
        for (int db = 0; db < NDB; ++db) store_dT(orow, acc_o[db], db, h, inv);
      }
    } else {  // a padding row: exact zeros
#pragma unroll
      for (int g = 0; g < D / 8; ++g) *reinterpret_cast<uint2*>(orow + 8 * g + 4 * h) = make_uint2(0u, 0u);
    }
  }
}

// ============================================================================ host
at::Tensor append_attn_hip(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                           const at::Tensor& start, const at::Tensor& nnew, int64_t n_head, double scale,
                           int64_t kv_len_max, const c10::optional<at::Tensor>& rope_cos,
                           const c10::optional<at::Tensor>& rope_sin) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.dim() == 3 && qkv.stride(2) == 1 &&
                  qkv.stride(0) % 8 == 0 && qkv.stride(1) % 8 == 0 && ((uintptr_t)qkv.data_ptr() & 15) == 0,
              "append_attn: qkv must be a bf16 [B, Tn, (H + 2·Hkv)·D] GPU view, unit last stride, strides multiples "
              "of 8 elements, 16-B aligned");
  TORCH_CHECK(k_cache.is_cuda() && k_cache.scalar_type() == at::kBFloat16 && k_cache.is_contiguous() &&
                  k_cache.dim() == 4 && v_cache.dim() == 4 && v_cache.is_cuda() &&
                  v_cache.scalar_type() == at::kBFloat16 && v_cache.is_contiguous() &&
                  ((uintptr_t)k_cache.data_ptr() & 15) == 0 && ((uintptr_t)v_cache.data_ptr() & 15) == 0,
              "append_attn: caches must be contiguous bf16 [B, Hkv, Tmax, D]");
  const int64_t D = k_cache.size(3);  // (hides attn::D: the head dim of this call)
  TORCH_CHECK(D == 64 || D == 128, "append_attn: head dim must be 64 or 128, got ", D, " (the caches' last dim)");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), "append_attn: k_cache ", k_cache.sizes(), " and v_cache ",
              v_cache.sizes(), " must have the same shape (head dim ", D, ")");
  const int64_t B = qkv.size(0), Tn = qkv.size(1), Hkv = k_cache.size(1), Tmax = k_cache.size(2), H = n_head;
  TORCH_CHECK(B >= 1 && Tn >= 1 && Tmax >= 1, "append_attn: empty input");
  TORCH_CHECK(k_cache.size(0) == B, "append_attn: cache batch ", k_cache.size(0), " != ", B);
  TORCH_CHECK(H > 0 && Hkv > 0 && H % Hkv == 0, "append_attn: need H % Hkv == 0");
  TORCH_CHECK(qkv.size(2) == (H + 2 * Hkv) * D, "append_attn: qkv width ", qkv.size(2), " != (H + 2·Hkv)·", D,
              " = ", (H + 2 * Hkv) * D, " at head dim ", D);
  auto chk = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.get_device() == qkv.get_device() && t.scalar_type() == at::kLong &&
                    t.is_contiguous() && t.numel() == B,
                "append_attn: ", name, " must be a contiguous int64 [B] tensor on qkv's device");
  };
  chk(start, "start");
  chk(nnew, "nnew");
  TORCH_CHECK(k_cache.get_device() == qkv.get_device() && v_cache.get_device() == qkv.get_device(),
              "append_attn: caches must be on qkv's device");
  TORCH_CHECK(kv_len_max >= 1 && kv_len_max <= Tmax, "append_attn: kv_len_max must be in [1, Tmax]");
  TORCH_CHECK(scale > 0, "append_attn: scale must be positive");
  const Rope rp = [&] {
    const bool hc = rope_cos.has_value() && rope_cos->defined(), hs = rope_sin.has_value() && rope_sin->defined();
    TORCH_CHECK(hc == hs, "append_attn: rope_cos and rope_sin go together");
    if (!hc) return Rope{nullptr, nullptr};
    TORCH_CHECK(rope_cos->is_cuda() && rope_sin->is_cuda() && rope_cos->get_device() == qkv.get_device() &&
                    rope_sin->get_device() == qkv.get_device() && rope_cos->scalar_type() == at::kFloat &&
                    rope_sin->scalar_type() == at::kFloat && rope_cos->is_contiguous() && rope_sin->is_contiguous() &&
                    rope_cos->dim() == 2 && rope_cos->size(1) == D / 2 && rope_cos->size(0) >= Tmax &&
                    rope_sin->sizes() == rope_cos->sizes(),
                "append_attn: rope tables must be contiguous float32 [>= Tmax, ", D / 2, "] on qkv's device at head dim ",
                D);
    return Rope{rope_cos->data_ptr<float>(), rope_sin->data_ptr<float>()};
  }();
  const int64_t nqb = (Tn + BLK - 1) / BLK;
  const int64_t total = B * Tn * Hkv * (D / 16);  // append_kv threads
  TORCH_CHECK(B * H * nqb < (1LL << 31) && (total + NT - 1) / NT < (1LL << 31) && Tmax < (1LL << 30) &&
                  Tn < (1LL << 30) && B * H * Tn < (1LL << 40),
              "append_attn: grid too large");
  at::Tensor out = at::empty({B, Tn, H * D}, qkv.options().memory_format(at::MemoryFormat::Contiguous));
  AppendParams p;
  p.qkv = static_cast<const uint16_t*>(qkv.data_ptr());
  p.sb = qkv.stride(0);
  p.st = qkv.stride(1);
  p.kc = static_cast<uint16_t*>(k_cache.data_ptr());
  p.vc = static_cast<uint16_t*>(v_cache.data_ptr());
  p.start = start.data_ptr<int64_t>();
  p.nnew = nnew.data_ptr<int64_t>();
  p.out = static_cast<uint16_t*>(out.data_ptr());
  p.rp = rp;
  p.H = (int)H;
  p.Hkv = (int)Hkv;
  p.Tn = (int)Tn;
  p.Tmax = (int)Tmax;
  p.L = (int)std::min(Tmax, kv_len_max);
  p.nqb = (int)nqb;
  p.sc2 = (float)scale * kLog2e;
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto launch = [&](auto d_c) {
    constexpr int HD = decltype(d_c)::value;
    hipLaunchKernelGGL(append_kv_kernel<HD>, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, p, total);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(append_attn_kernel<HD>, dim3((unsigned)(B * H * nqb)), dim3(NT), 0, st, p);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  };
  if (D == 64)
    launch(std::integral_constant<int, 64>{});
  else
    launch(std::integral_constant<int, 128>{});
  return out;
}

}  // namespace attn
}  // namespace nbd

TORCH_LIBRARY_IMPL(nbd, CUDA, m) { m.impl("append_attn", &nbd::attn::append_attn_hip); }
