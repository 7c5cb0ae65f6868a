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
//     empty row (every unsplit sweep starts at tile 0 and key 0 <= every lim: the running maximum is
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
//   * the unsplit grid is B · H · ceil(Tn / 128) workgroups (heaviest query block first), each
//     sweeping its keys sequentially: append_attn_kernel<D, false>.
// Tn needs no padding: the kernel clamps its query loads and bounds its stores at Tn.
//
// Key split (append_attn_kernel<D, true> + append_merge_kernel<D>; flash-decoding partials as in
// decode.hip).  Few sequences over a long history leave the unsplit grid on a fraction of the
// 256 CUs, and one workgroup's sweep is the time.  The host's plan() then cuts the sweep:
//   * grid B · H · nqb · nsplit, (query block, chunk) slowest — the last query block first, its
//     chunks from key 0 up (the low chunks are the ones every block has).  A workgroup owns
//     (batch · head, query block, chunk c) and sweeps the 64-key tiles [c · chunk_tiles,
//     (c + 1) · chunk_tiles) cut at the block's last tile; chunk edges are tile edges, the body
//     is the unsplit one.  A chunk that starts past the block's last tile (short history, early
//     query block) returns before it stages anything — uniform in the workgroup, no barrier met.
//   * partials, fp32: per (batch · head, query block, chunk, wave) one tile O^T[D][32] of the
//     chunk's normalised output followed by lse[32] = m + log2(l).  Dim-major with the 32
//     queries contiguous is the accumulator as the wave holds it (dim in the register, query on
//     the lane): every store instruction writes two whole 128-B lines, nothing is transposed,
//     and the merge reads the lines back the same way.
//   * empty rows: with c > 0 a lane, or a whole wave, of a live workgroup may see no key of its
//     chunk (the diagonal start + i crosses the chunk edge inside the block).  Its registers
//     hold nothing (or NaN, exp2(-inf + inf)); MFMA columns are per query, so nothing leaks into
//     a neighbour.  Such a lane stores nothing, and the merge never reads its slot: it derives
//     from start / nnew that query i has the chunks 0 .. (start + i) / (64 · chunk_tiles) and
//     reads exactly those — each written by this call (the chunk's first tile held a visible
//     key: m finite, l > 0).  No -inf markers, no workspace read that this call did not write.
//   * append_merge_kernel: a second small launch (why not the last-arriving workgroup:
//     decode.hip).  Per query: max of the lse values, then the exp2-weighted sum, chunks in index
//     order — bit-reproducible.  It writes the bf16 row and the zeros of the padding rows.
//   * both grids and the workspace size (at::empty inside the op, like `out`) follow host values
//     only: B, H, Tn, kv_len_max, D.  The op still captures into a HIP graph.
//   * the <D, false> instantiations are the kernels they were, instruction for instruction (one
//     kernarg displacement aside: the grid size sits behind the new fields).  Compiler's report,
//     VGPR / AGPR / scratch / waves per SIMD / LDS: <64, false> 171 / 0 / 0 / 2 / 21 504,
//     <64, true> 171 / 0 / 0 / 2 / 21 504, <128, false> 256 / 131 / 0 / 1 / 37 888, <128, true>
//     256 / 133 / 0 / 1 / 37 888; merge 52 (64) and 90 (128) VGPR, no LDS.
//
// fp8 caches (append_kv_kernel<D, true>, append_attn_kernel<D, SPLIT, true>; the row format is
// kv8.h's, decode.hip's contract: D bytes of OCP e4m3fn per row, no scales, q8 of the bf16 row):
//   * append_kv_kernel rotates k in fp32 and packs it to bf16 as before, then quantises each 8-dim
//     chunk (quant8: clamp to ±448, round to nearest even, NaN kept) and stores 8 B; v is quantised
//     from the bf16 row of qkv.  The rotated k is rounded fp32 -> bf16 -> e4m3, like a prefilled row.
//   * append_attn_kernel dequantises while it stages, not at the MFMA: a tile's rows are loaded as
//     8-B pieces, one per ld16 of the bf16 kernel, with the same thread-to-element mapping
//     (StagePair8, StageRows8<D>); a tile is one contiguous 4 KiB / 8 KiB run per (batch, kv head).
//     The pieces stay e4m3 in registers while the loads are in flight under the current tile's
//     math — half the staging registers — and become bf16 only at the ds_write (widen8:
//     v_cvt_pk_f32_fp8, then the high halves of the two fp32 values in one v_perm_b32; every e4m3
//     value is exact in bf16).  Rows >= kend become zero bytes on the row index, before the
//     conversion.  LDS images, reads, MFMA body, softmax, diagonal, partials and sweep bounds are
//     the bf16 kernel's: the output is bit for bit what <D, SPLIT, false> gives on a bf16 cache
//     holding the dequantised rows (tests/test_gpu_append_kv8.py), split and unsplit.
//   * not built: an fp8 MFMA path (q and P are bf16; quantising them changes the result) and e4m3
//     LDS images converted at every wave's read (four times the conversions, a second transposed
//     read layout).
//   * the <.., false> instantiations and both merge kernels are, instruction for instruction, what
//     they were (compared in the ISA).  The new ones, VGPR / AGPR / scratch / waves per SIMD / LDS:
//     attn <64, false, true> 163 / 0 / 0 / 3 / 21 504, <64, true, true> 165 / 0 / 0 / 3 / 21 504,
//     <128, false, true> 243 / 128 / 0 / 1 / 37 888, <128, true, true> 245 / 128 / 0 / 1 / 37 888
//     (the launch bounds are the bf16 kernels'); append_kv <64 | 128, true> 50 VGPR (bf16: 49).
//     No packed fp32 instruction in the unit, with -fno-slp-vectorize as it is built.
//
// Shared prefix (append_kv_kernel<D, F8, true>, append_attn_kernel<D, SPLIT, F8, true>,
// append_merge_kernel<D, true>; op append_attn_shared; the cache of several samples per prompt,
// decode.hip's decode_kernel<.., SHARED>): sequence s of S = B · group continues prompt p = s / group.
// Position j of it lives in prefix[p, kvh, j] for j < plen[p] and in own[s, kvh, j - plen[p]] from
// there on; plen is int64 [B] on the device, start stays an absolute position, nothing synchronises,
// and grids and workspace follow host values only (S, H, Tn, kv_len_max, D) as above.
//   * clamps, before anything is addressed: plen into [0, Tp], start - plen into [0, To - 1], nnew
//     into [0, min(Tn, To - (start - plen), L - start)] (span_of's second form; the merge kernel
//     takes the same one, so it reads the slots the attention kernel wrote under it).
//   * append_kv_kernel: the block's row at position start + i, rotated there, becomes own row
//     start + i - plen.  The prefix is never written.
//   * append_attn_kernel: only where a staged row comes from changes.  The own base of the
//     (sequence, kv head) is set back by plen rows, so the absolute key index addresses prefix and
//     own rows alike and the row clamp is one bound, plen + To - 1.  A 64-key tile is then one of
//     three cases, decided by scalar compares of the tile index with plen (uniform in the
//     workgroup): wholly prefix or wholly own — one base pointer, the unshared loads (RowsOne) —
//     or the one tile per sequence that holds key plen when plen is no multiple of 64, which
//     selects the base per row (RowsTwo: a compare and two v_cndmask per base; the row index is
//     the same either way).  load_tile branches between the two forms; both leave their loads in
//     flight, so the next tile streams under the current tile's math across the prefix-to-own
//     boundary as anywhere else.  Zeros on the row index come after the select: prefix rows
//     >= plen are never addressed (own rows stand there), own rows >= start - plen + nnew are keys
//     >= kend.  LDS images, transposed reads, MFMA body, softmax, diagonal, sweep bounds, chunk
//     edges and partials are the unshared kernel's: the output equals, bit for bit, the unshared
//     kernel's on the materialised cache (tests/test_gpu_append_shared.py), bf16 and fp8, split
//     and unsplit.
//   * grid order is the unshared one — batch · head fastest within a (query block, chunk) — so the
//     workgroups of the `group` samples of a prompt are neighbours in the grid and their prefix
//     tiles can meet in L2 / MALL instead of streaming `group` copies from HBM.  A design intent:
//     the residency was not measured (docs/FINDINGS.md §50 has the times).
//   * the parameters are a type of their own (SharedAppendParams, AppendParams plus five fields), so
//     the unshared kernels keep their kernarg segment.  Their ISA against the previous build: the
//     128 unsplit attention kernels, append_kv and merge are instruction for instruction what they
//     were; the 128 split kernels differ in the operand order of one v_add_f32; the 64 attention
//     kernels hold the same instructions, with the v_cndmask that zero a staged tile (and their
//     registers) in another order.  The compiler's choice — the loads moved into a lambda over the
//     row source — and not a change of work.
//   * the new instantiations, VGPR / AGPR / scratch / waves per SIMD / LDS (<D, SPLIT, F8, true>):
//     <64, false, false> 171 / 0 / 0 / 2 / 21 504, <64, true, false> 173 / 0 / 0 / 2 / 21 504,
//     <64, false, true> 163 / 0 / 0 / 3 / 21 504, <64, true, true> 171 / 0 / 0 / 2 / 21 504,
//     <128, false, false> 256 / 135 / 0 / 1 / 37 888, <128, true, false> 256 / 135 / 0 / 1 / 37 888,
//     <128, false, true> 256 / 129 / 0 / 1 / 37 888, <128, true, true> 253 / 128 / 0 / 1 / 37 888:
//     no scratch anywhere, the launch bounds are the unshared kernels'.  The four bases and plen
//     are scalar registers.
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
#include "kv8.h"
#include "nbd_common.h"

namespace nbd {
namespace attn {

struct AppendParams {
  const uint16_t* qkv;  // [B, Tn, (H + 2·Hkv)·D] bf16, element strides sb / st, unit last stride
  int64_t sb, st;
  uint16_t* kc;  // [B, Hkv, Tmax, D] contiguous: bf16, or e4m3fn bytes (the <.., F8 = true> kernels)
  uint16_t* vc;
  const int64_t* start;  // [B]
  const int64_t* nnew;   // [B]
  uint16_t* out;         // [B, Tn, H·D] bf16, contiguous
  Rope rp;
  int H, Hkv, Tn, Tmax, L, nqb;  // L = min(Tmax, kv_len_max): the clamp of start + nnew
  float sc2;                     // softmax scale · log2(e)
  // the key split (append_attn_kernel<D, true> and append_merge_kernel; unread otherwise)
  float* ws;                // chunk partials: [B·H, nqb, nsplit, 4 waves] tiles of (D + 1) x 32 fp32
  int nsplit, chunk_tiles;  // chunk c of a query block = its 64-key tiles [c·chunk_tiles, (c + 1)·chunk_tiles)
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

// the <.., SHARED = true> kernels (header: shared prefix): kc / vc are the sequences' own rows
// [B, Hkv, To, D], sequence b reads rows [0, plen[b / group]) of prompt b / group's prefix before
// them; Tmax = Tp + To and L count absolute positions.  A type of its own, so the unshared kernels'
// kernarg segment is what it was.
struct SharedAppendParams : AppendParams {
  const uint16_t* kp;   // [B / group, Hkv, Tp, D] contiguous, the dtype of kc / vc; never written
  const uint16_t* vp;
  const int64_t* plen;  // [B / group]
  int group, Tp, To;
};
template <bool SHARED>
using ParamsOf = std::conditional_t<SHARED, SharedAppendParams, AppendParams>;

// the same behind a prefix: plen into [0, Tp], start - plen into [0, To - 1] (the block never lands
// in the prefix), nnew into [0, min(Tn, To - (start - plen), L - start)].  s0 stays absolute; the
// rows of the block are own rows s0 - pl .. s0 - pl + n - 1 <= To - 1.
__device__ __forceinline__ Span span_of(const SharedAppendParams& p, int b, int& pl) {
  pl = (int)min<int64_t>(max<int64_t>(p.plen[b / p.group], 0), p.Tp);
  const int o0 = (int)min<int64_t>(max<int64_t>(p.start[b] - pl, 0), p.To - 1);
  Span s;
  s.s0 = pl + o0;
  s.n = (int)max<int64_t>(min<int64_t>(max<int64_t>(p.nnew[b], 0), min(min(p.Tn, p.To - o0), p.L - s.s0)), 0);
  return s;
}

__device__ __forceinline__ s8v zero8() {
  s8v z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = 0;
  return z;
}

// ---- fp8 caches: a thread's 8 dims of a row are 8 B (kv8.h)
__device__ __forceinline__ u32x2 ld8(const uint8_t* p) { return *reinterpret_cast<const u32x2*>(p); }
__device__ __forceinline__ void st8(uint8_t* p, u32x2 v) { *reinterpret_cast<u32x2*>(p) = v; }
__device__ __forceinline__ u32x2 quant8(s8v v) { return nbd::quant8(__builtin_bit_cast(u32x4, v)); }
__device__ __forceinline__ s8v widen8s(u32x2 v) { return __builtin_bit_cast(s8v, widen8(v)); }

// StagePair and StageRows<D> (attn_common.h; StageRows<64> is Stage2's mapping) over e4m3 pieces:
// the same thread-to-element mapping, half the registers while the loads are in flight, expanded
// to bf16 (widen8: exact) at the ds_write — the LDS images are the bf16 kernel's, byte for byte
struct StagePair8 {
  u32x2 a, b;
  __device__ __forceinline__ void store(uint16_t* lds, int stride, int tid) const {
    uint16_t* p = lds + (tid >> 2) * stride + (tid & 3) * 8;
    st16(p, widen8s(a));
    st16(p + 32, widen8s(b));
  }
};
template <int D>
struct StageRows8 {
  u32x2 a[D / 32];
  __device__ __forceinline__ void store(uint16_t* lds, int stride, int tid) const {
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const int c = tid + i * NT;
      st16(lds + (c >> (D == 64 ? 3 : 4)) * stride + (c & (D / 8 - 1)) * 8, widen8s(a[i]));
    }
  }
};

// where the rows of a staged tile come from: at<0>(r) / at<1>(r) is the k / v base that key row r
// is addressed from, rows the row indices that may be addressed (clamped to rows - 1).  RowsOne: one run of rows — an
// unshared cache, or a tile of a shared one that lies wholly in the prefix or wholly in own rows.
// RowsTwo: the tile that straddles plen selects per row (two v_cndmask per base).
struct RowsOne {
  const uint16_t* base[2];
  int rows;
  template <int V>
  __device__ __forceinline__ const uint16_t* at(int) const {
    return base[V];
  }
};
struct RowsTwo {
  const uint16_t* pre[2];
  const uint16_t* own[2];  // set back by plen rows: indexed by the absolute key row
  int pl, rows;
  template <int V>
  __device__ __forceinline__ const uint16_t* at(int r) const {
    return r < pl ? pre[V] : own[V];
  }
};

// ============================================================================ cache append
// thread = (b, i, kv head, c), c < D/16: dims [8c, 8c + 8) and their rotation partners
// [D/2 + 8c, D/2 + 8c + 8) of k, the same two 16-B chunks of v.  F8: each chunk is stored as its 8
// e4m3 bytes, q8 of the bf16 chunk — the rotated k is rounded fp32 -> bf16 -> e4m3, like a
// prefilled row and like decode.hip's.  SHARED: position t is own row t - plen; the prefix is not
// written
template <int D, bool F8, bool SHARED>
__global__ __launch_bounds__(NT) void append_kv_kernel(ParamsOf<SHARED> p, int64_t total) {
  static_assert(D == 64 || D == 128, "head dim 64 or 128");
  constexpr int HALF = D / 2;
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= total) return;
  const int c = (int)(g & (D / 16 - 1));
  const int64_t rowi = g >> (D == 64 ? 2 : 3);
  const int kvh = (int)(rowi % p.Hkv);
  const int i = (int)(rowi / p.Hkv % p.Tn);
  const int b = (int)(rowi / p.Hkv / p.Tn);
  Span sp;
  int tmax = p.Tmax, off = 0;  // rows per (sequence, kv head) of kc / vc; the position of their row 0
  if constexpr (SHARED) {
    sp = span_of(p, b, off);
    tmax = p.To;
  } else {
    sp = span_of(p, b);
  }
  if (i >= sp.n) return;  // padding: nothing lands in the cache
  const int t = sp.s0 + i;
  const uint16_t* row = p.qkv + b * p.sb + i * p.st;
  const uint16_t* ks = row + (p.H + kvh) * D + c * 8;
  const uint16_t* vs = row + (p.H + p.Hkv + kvh) * D + c * 8;
  s8v ka = ld16(ks), kb = ld16(ks + HALF);
  if (p.rp.cos != nullptr) rope8_hd<HALF>(ka, kb, p.rp, t, c * 8);
  const int64_t dst = (((int64_t)b * p.Hkv + kvh) * tmax + (t - off)) * D + c * 8;
  if constexpr (F8) {  // dst counts elements: bytes here
    uint8_t* const k8 = reinterpret_cast<uint8_t*>(p.kc) + dst;
    uint8_t* const v8 = reinterpret_cast<uint8_t*>(p.vc) + dst;
    st8(k8, quant8(ka));
    st8(k8 + HALF, quant8(kb));
    st8(v8, quant8(ld16(vs)));
    st8(v8 + HALF, quant8(ld16(vs + HALF)));
  } else {
    st16(p.kc + dst, ka);
    st16(p.kc + dst + HALF, kb);
    st16(p.vc + dst, ld16(vs));
    st16(p.vc + dst + HALF, ld16(vs + HALF));
  }
}

// ============================================================================ attention
// occupancy: the 64 instantiation fits two waves per SIMD (171 VGPRs).  Under the same bound the
// 128 one needs 256 VGPRs and 44 B of scratch per lane (the compiler's resource report), so it is
// built for one wave per SIMD, where it spills nothing.
// SPLIT: a workgroup sweeps one chunk of its query block's tiles and stores fp32 partials (header)
// F8: the caches hold e4m3 bytes; only load_tile and the staging structs differ (header)
// SHARED: keys below plen come from the prompt's prefix, the rest from own rows; only where
// load_tile takes a row from differs (header)
template <int D, bool SPLIT, bool F8, bool SHARED>
__global__ __launch_bounds__(NT, D == 64 ? 2 : 1) void append_attn_kernel(ParamsOf<SHARED> p) {
  static_assert(D == 64 || D == 128, "head dim 64 or 128");
  constexpr int RS = D + 8;                // K image row stride (elements): row reads
  constexpr int RSV = D == 64 ? 96 : 160;  // V image row stride: transposed reads (header: banks)
  constexpr int NS = D / 16;               // MFMA k-steps of q·k = query fragments per lane
  constexpr int NDB = D / 32;              // 32-dim blocks of O
  __shared__ __attribute__((aligned(16))) uint16_t Ks[TILE * RS];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[TILE * RSV];
  int BH, bh, qb, ck = 0;
  if constexpr (SPLIT) {  // (query block, chunk) slowest: the last block first, its chunks from key 0 up
    BH = gridDim.x / (p.nqb * p.nsplit);
    bh = blockIdx.x % BH;
    const int rest = blockIdx.x / BH;
    ck = rest % p.nsplit;
    qb = p.nqb - 1 - rest / p.nsplit;
  } else {
    BH = gridDim.x / p.nqb;
    bh = blockIdx.x % BH;
    qb = p.nqb - 1 - blockIdx.x / BH;  // the last query block sweeps the most keys: first
  }
  const int b = bh / p.H, hh = bh % p.H;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  Span sp;
  int pl = 0;  // SHARED: the prompt's prefix rows, uniform in the workgroup
  if constexpr (SHARED)
    sp = span_of(p, b, pl);
  else
    sp = span_of(p, b);
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
  // this workgroup's tiles [t0, t1): all of them, or chunk ck cut at the block's last tile
  int t0 = 0, t1 = ntiles;
  if constexpr (SPLIT) {
    t0 = ck * p.chunk_tiles;
    t1 = min(ntiles, t0 + p.chunk_tiles);
    if (t0 >= ntiles) return;  // uniform in the workgroup, before any barrier: no key of this chunk is visible
  }

  s8v qf[NS];
  {
    const uint16_t* qrow = p.qkv + b * p.sb + (int64_t)min(qi, p.Tn - 1) * p.st + hh * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = ld16(qrow + 16 * s + 8 * h);
  }
  if (p.rp.cos != nullptr) rope_frag_hd<D>(qf, p.rp, lim, h);
  f16x acc_o[NDB] = {};
  float m = -INFINITY, l = 0.f;

  // (F8: a row is D bytes, so the head's first row sits at half this element offset)
  constexpr int RE = F8 ? D / 2 : D;  // a cache row in elements of the base pointers
  int crows = p.Tmax;  // rows per (sequence, kv head) of kc / vc
  if constexpr (SHARED) crows = p.To;
  const int64_t hoff = ((int64_t)b * p.Hkv + kh) * crows * RE;
  const uint16_t* kbase = p.kc + hoff;
  const uint16_t* vbase = p.vc + hoff;
  // the 64 tile keeps the fixed staging structs, so that instantiation stays the kernel it was
  std::conditional_t<F8, std::conditional_t<D == 64, StagePair8, StageRows8<D>>,
                     std::conditional_t<D == 64, StagePair, StageRows<D>>> sk;
  std::conditional_t<F8, StageRows8<D>, std::conditional_t<D == 64, Stage2, StageRows<D>>> sv;
  // a tile's rows from `src` (RowsOne | RowsTwo: the base of key row r and the count of rows that
  // may be addressed; the row index clamped below it); rows >= kend become zeros
  auto load_rows = [&](StageRows<D>& sr, auto v_c, const auto& src, int k0) {  // (128)
    constexpr int V = decltype(v_c)::value;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const int c = tid + i * NT;
      const int vr = k0 + (c >> (D == 64 ? 3 : 4));
      sr.a[i] = ld16(src.template at<V>(vr) + (int64_t)min(vr, src.rows - 1) * D + (c & (D / 8 - 1)) * 8);
      if (vr >= kend) sr.a[i] = zero8();
    }
  };
  // F8: the same rows as 8-B pieces, one per ld16 of the bf16 tile; the row index decides on the
  // zeros before anything is converted, so a NaN byte of a free row never reaches LDS
  auto load_rows8 = [&](StageRows8<D>& sr, auto v_c, const auto& src, int k0) {
    constexpr int V = decltype(v_c)::value;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const int c = tid + i * NT;
      const int vr = k0 + (c >> (D == 64 ? 3 : 4));
      const uint8_t* const base8 = reinterpret_cast<const uint8_t*>(src.template at<V>(vr));
      sr.a[i] = ld8(base8 + (int64_t)min(vr, src.rows - 1) * D + (c & (D / 8 - 1)) * 8);
      if (vr >= kend) sr.a[i] = u32x2{0u, 0u};
    }
  };
  constexpr std::integral_constant<int, 0> K_{};
  constexpr std::integral_constant<int, 1> V_{};
  auto load_from = [&](int k0, const auto& src) {
    if constexpr (F8) {
      if constexpr (D == 64) {  // StagePair's mapping: row tid / 4, pieces q and q + 4
        const int kr = k0 + (tid >> 2);
        const uint8_t* pk = reinterpret_cast<const uint8_t*>(src.template at<0>(kr)) + (int64_t)min(kr, src.rows - 1) * D +
                            (tid & 3) * 8;
        sk.a = ld8(pk);
        sk.b = ld8(pk + 32);
        if (kr >= kend) sk.a = sk.b = u32x2{0u, 0u};
      } else {
        load_rows8(sk, K_, src, k0);
      }
      load_rows8(sv, V_, src, k0);
    } else if constexpr (D == 64) {
      const int kr = k0 + (tid >> 2);
      const uint16_t* pk = src.template at<0>(kr) + (int64_t)min(kr, src.rows - 1) * D + (tid & 3) * 8;
      sk.a = ld16(pk);
      sk.b = ld16(pk + 32);
      if (kr >= kend) sk.a = sk.b = zero8();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = tid + i * NT;
        const int vr = k0 + (c >> 3);
        sv.a[i] = ld16(src.template at<1>(vr) + (int64_t)min(vr, src.rows - 1) * D + (c & 7) * 8);
        if (vr >= kend) sv.a[i] = zero8();
      }
    } else {
      load_rows(sk, K_, src, k0);
      load_rows(sv, V_, src, k0);
    }
  };
  // SHARED: the prefix of this (prompt, kv head), and the own rows set back by plen rows, so that
  // the absolute key index addresses both; own rows end at key plen + To - 1
  const uint16_t *kpre = nullptr, *vpre = nullptr, *kown = nullptr, *vown = nullptr;
  if constexpr (SHARED) {
    const int64_t poff = ((int64_t)(b / p.group) * p.Hkv + kh) * p.Tp * RE;
    kpre = p.kp + poff;
    vpre = p.vp + poff;
    kown = kbase - (int64_t)pl * RE;
    vown = vbase - (int64_t)pl * RE;
  }
  // a tile lies wholly in the prefix or wholly in own rows: one base, chosen by a scalar compare
  // (uniform in the workgroup).  Only the tile that holds key plen, when plen is no multiple of
  // 64, picks its base per row.
  auto load_tile = [&](int k0) {
    if constexpr (SHARED) {
      const int rows = pl + p.To;
      if (k0 < pl && k0 + TILE > pl) {
        load_from(k0, RowsTwo{{kpre, vpre}, {kown, vown}, pl, rows});
      } else {
        const bool pre = k0 < pl;
        load_from(k0, RowsOne{{pre ? kpre : kown, pre ? vpre : vown}, rows});
      }
    } else {
      load_from(k0, RowsOne{{kbase, vbase}, p.Tmax});
    }
  };
  load_tile(t0 * TILE);
  sk.store(Ks, RS, tid);
  sv.store(Vs, RSV, tid);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    if (t + 1 < t1) load_tile((t + 1) * TILE);  // issue the next tile's loads now, write them after this tile
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
    if (t + 1 < t1) {
      sk.store(Ks, RS, tid);
      sv.store(Vs, RSV, tid);
      __syncthreads();
    }
  }
  if constexpr (SPLIT) {
    // the chunk's partial of a real query that sees a key of this chunk (t0·64 <= lim: its first
    // tile ran, m is finite and l > 0).  Other lanes hold nothing (or NaN: an empty row's
    // exp2(-inf + inf)) and store nothing; append_merge_kernel never reads their slots.
    if (qi < n && lim >= t0 * TILE) {
      float* wt = p.ws + ((((int64_t)bh * p.nqb + qb) * p.nsplit + ck) * 4 + w) * ((D + 1) * 32);
      const float inv = 1.f / l;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) wt[(db * 32 + crow(i, h)) * 32 + r] = acc_o[db][i] * inv;
      if (h == 0) wt[D * 32 + r] = m + __log2f(l);
    }
  } else if (qi < p.Tn) {
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

// ============================================================================ merge of the key split
// workgroup = the 32 queries of one wave tile of one (batch, head); thread = (query r = tid & 31,
// dim group g = tid >> 5): dims 4·(g + 8j) + [0, 4), j < D/32 — a wave instruction reads two whole
// 128-B lines of a partial tile, a thread's four dims of a piece become one 8-B store of the row.
// A query reads the chunks that hold one of its keys, chunk 0 .. lim / (64·chunk_tiles), and no
// other: those slots were written by this call's append_attn_kernel<D, true> (header).  Fixed
// order, fp32: bit-reproducible.
// SHARED changes the clamp of (start, nnew) only: the one the attention kernel wrote the slots under.
template <int D, bool SHARED>
__global__ __launch_bounds__(NT) void append_merge_kernel(ParamsOf<SHARED> p) {
  constexpr int NP = D / 32;  // 8-B pieces of the row per thread
  const int BH = gridDim.x / ((p.Tn + 31) / 32);
  const int bh = blockIdx.x % BH, qt = blockIdx.x / BH;
  const int b = bh / p.H, hh = bh % p.H;
  const int r = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int qi = qt * 32 + r;
  if (qi >= p.Tn) return;
  Span sp;
  if constexpr (SHARED) {
    int pl;
    sp = span_of(p, b, pl);
  } else {
    sp = span_of(p, b);
  }
  uint16_t* orow = p.out + (((int64_t)b * p.Tn + qi) * p.H + hh) * D;
  if (qi >= sp.n) {  // a padding row: exact zeros
#pragma unroll
    for (int j = 0; j < NP; ++j) *reinterpret_cast<uint2*>(orow + 4 * (g + 8 * j)) = make_uint2(0u, 0u);
    return;
  }
  const int nc = min((sp.s0 + qi) / (TILE * p.chunk_tiles) + 1, p.nsplit);
  constexpr int TS = (D + 1) * 32;  // floats of a wave tile: O^T[D][32], then lse[32]
  const float* wt = p.ws + ((((int64_t)bh * p.nqb + (qt >> 2)) * p.nsplit) * 4 + (qt & 3)) * TS;
  float mx = -INFINITY;
  for (int k = 0; k < nc; ++k) mx = fmaxf(mx, wt[(int64_t)k * 4 * TS + D * 32 + r]);
  float L = 0.f, O[NP][4] = {};
  for (int k = 0; k < nc; ++k) {
    const float* t = wt + (int64_t)k * 4 * TS;
    const float wgt = exp2f(t[D * 32 + r] - mx);
    L += wgt;
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) O[j][e] += wgt * t[(4 * (g + 8 * j) + e) * 32 + r];
  }
  const float inv = 1.f / L;
#pragma unroll
  for (int j = 0; j < NP; ++j)
    *reinterpret_cast<uint2*>(orow + 4 * (g + 8 * j)) =
        make_uint2(pack2_bf16(O[j][0] * inv, O[j][1] * inv), pack2_bf16(O[j][2] * inv, O[j][3] * inv));
}

// ============================================================================ host
// the key split of a call: nsplit chunks of chunk_tiles 64-key tiles each (nsplit = 1: the unsplit
// kernel).  key_splits = 1: never; n > 1: n chunks asked for, whatever the thresholds (tests, A/B
// runs); 0: the plan —
//   * as many chunks as keep B · H · nqb · nsplit within the workgroups the chip holds at once,
//     256 CUs x 2 at head dim 64 and x 1 at 128 (the launch bounds above): one more round of
//     workgroups costs what the split saved (measured at 128, batch 8: 0.76 - 0.93 x);
//   * at least kMinTiles tiles (256 keys, decode.hip's figure) per chunk, at most kMaxSplit chunks;
//   * none unless that gives kMinChunks chunks, i.e. from 12 tiles (> 704 keys) on: with two chunks
//     of a 512-key history the kernels gain 1 us and an eager turn pays 3 us per layer for the
//     second launch and the workspace.
// docs/FINDINGS.md §48 has the runs behind these.  fp8 caches take the same plan: the thresholds
// were measured on bf16 bytes, and how the fp8 kernel's time divides between the streamed bytes
// (half) and the MFMA / conversion work (more) is not known well enough to move them — a change
// here wants an interleaved A/B of its own.
constexpr int64_t kMinTiles = 4, kMinChunks = 3, kMaxSplit = 64;
struct SplitPlan {
  int nsplit, chunk_tiles;
};
static SplitPlan plan(int64_t BHq, int64_t L, int64_t head_dim, int64_t key_splits) {
  const int64_t tiles = (L + TILE - 1) / TILE;
  const int64_t slots = head_dim == 64 ? 512 : 256;
  int64_t nc = 1;
  if (key_splits > 1) {
    nc = std::min(key_splits, tiles);
  } else if (key_splits == 0 && 2 * BHq <= slots && tiles >= kMinChunks * kMinTiles) {
    nc = std::min({slots / BHq, tiles / kMinTiles, kMaxSplit});
  }
  const int64_t ct = (tiles + nc - 1) / nc;
  return SplitPlan{(int)((tiles + ct - 1) / ct), (int)ct};
}

int64_t append_attn_plan(int64_t batch, int64_t n_head, int64_t Tn, int64_t kv_len_max, int64_t head_dim) {
  TORCH_CHECK(batch >= 1 && n_head >= 1 && Tn >= 1 && kv_len_max >= 1, "append_attn_plan: empty problem");
  TORCH_CHECK(head_dim == 64 || head_dim == 128, "append_attn_plan: head dim must be 64 or 128, got ", head_dim);
  return plan(batch * n_head * ((Tn + BLK - 1) / BLK), kv_len_max, head_dim, 0).nsplit;
}

// the operands of append_attn_shared that append_attn has not
struct Shared {
  const at::Tensor& k_prefix;
  const at::Tensor& v_prefix;
  const at::Tensor& plen;
  int64_t group;
};

// both ops: `sh` == nullptr is append_attn (k_cache / v_cache hold every row), else they are the
// sequences' own rows behind the prompts' prefixes (B counts sequences: prompts · group)
static at::Tensor append_run(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                             const at::Tensor& start, const at::Tensor& nnew, int64_t n_head, double scale,
                             int64_t kv_len_max, const c10::optional<at::Tensor>& rope_cos,
                             const c10::optional<at::Tensor>& rope_sin, int64_t key_splits, const Shared* sh) {
  const char* op = sh ? "append_attn_shared" : "append_attn";
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.dim() == 3 && qkv.stride(2) == 1 &&
                  qkv.stride(0) % 8 == 0 && qkv.stride(1) % 8 == 0 && ((uintptr_t)qkv.data_ptr() & 15) == 0,
              op, ": qkv must be a bf16 [B, Tn, (H + 2·Hkv)·D] GPU view, unit last stride, strides multiples "
              "of 8 elements, 16-B aligned");
  const bool f8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(), op, ": k_cache (", k_cache.scalar_type(),
              ") and v_cache (", v_cache.scalar_type(), ") must have the same dtype, bf16 or float8_e4m3fn");
  auto check_caches = [&](const at::Tensor& k, const at::Tensor& v) {
    if (f8) {
      TORCH_CHECK(k.is_cuda() && k.is_contiguous() && k.dim() == 4 && v.dim() == 4 && v.is_cuda() &&
                      v.is_contiguous() && k.scalar_type() == at::kFloat8_e4m3fn &&
                      v.scalar_type() == at::kFloat8_e4m3fn && ((uintptr_t)k.data_ptr() & 7) == 0 &&
                      ((uintptr_t)v.data_ptr() & 7) == 0,
                  op, ": fp8 caches must be contiguous float8_e4m3fn [B, Hkv, Tmax, D], 8-B aligned rows");
    } else {
      TORCH_CHECK(k.is_cuda() && k.scalar_type() == at::kBFloat16 && k.is_contiguous() && k.dim() == 4 &&
                      v.dim() == 4 && v.is_cuda() && v.scalar_type() == at::kBFloat16 && v.is_contiguous() &&
                      ((uintptr_t)k.data_ptr() & 15) == 0 && ((uintptr_t)v.data_ptr() & 15) == 0,
                  op, ": caches must be contiguous bf16 [B, Hkv, Tmax, D]");
    }
  };
  check_caches(k_cache, v_cache);
  const int64_t D = k_cache.size(3);  // (hides attn::D: the head dim of this call)
  TORCH_CHECK(D == 64 || D == 128, op, ": head dim must be 64 or 128, got ", D, " (the caches' last dim)");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), op, ": k_cache ", k_cache.sizes(), " and v_cache ",
              v_cache.sizes(), " must have the same shape (head dim ", D, ")");
  // To = the rows of k_cache; absolute positions run to Tmax = Tp + To behind a prefix of Tp rows
  const int64_t B = qkv.size(0), Tn = qkv.size(1), Hkv = k_cache.size(1), To = k_cache.size(2), H = n_head;
  int64_t Tp = 0;
  TORCH_CHECK(B >= 1 && Tn >= 1 && To >= 1, op, ": empty input");
  TORCH_CHECK(k_cache.size(0) == B, op, ": cache batch ", k_cache.size(0), " != ", B);
  TORCH_CHECK(H > 0 && Hkv > 0 && H % Hkv == 0, op, ": need H % Hkv == 0");
  TORCH_CHECK(qkv.size(2) == (H + 2 * Hkv) * D, op, ": qkv width ", qkv.size(2), " != (H + 2·Hkv)·", D, " = ",
              (H + 2 * Hkv) * D, " at head dim ", D);
  if (sh) {
    TORCH_CHECK(sh->k_prefix.scalar_type() == k_cache.scalar_type() && sh->v_prefix.scalar_type() == k_cache.scalar_type(),
                op, ": prefix and own caches must have the same dtype (bf16 or float8_e4m3fn)");
    TORCH_CHECK(sh->k_prefix.dim() == 4 && sh->k_prefix.size(3) == D, op, ": prefix caches of head dim ",
                sh->k_prefix.dim() == 4 ? sh->k_prefix.size(3) : -1, " with own caches of head dim ", D);
    check_caches(sh->k_prefix, sh->v_prefix);
    TORCH_CHECK(sh->v_prefix.sizes() == sh->k_prefix.sizes(), op, ": k_prefix ", sh->k_prefix.sizes(), " and v_prefix ",
                sh->v_prefix.sizes(), " must have the same shape");
    Tp = sh->k_prefix.size(2);
    TORCH_CHECK(sh->group >= 1 && B % sh->group == 0 && sh->k_prefix.size(0) == B / sh->group &&
                    sh->k_prefix.size(1) == Hkv,
                op, ": prefix caches must be [B / group, Hkv, Tp, ", D, "] for qkv [B, ...] (B ", B, ", group ", sh->group,
                ", prefix batch ", sh->k_prefix.size(0), ")");
    TORCH_CHECK(sh->plen.is_cuda() && sh->plen.get_device() == qkv.get_device() && sh->plen.scalar_type() == at::kLong &&
                    sh->plen.is_contiguous() && sh->plen.numel() == B / sh->group,
                op, ": plen must be a contiguous int64 [B / group] tensor on qkv's device");
    TORCH_CHECK(sh->k_prefix.get_device() == qkv.get_device() && sh->v_prefix.get_device() == qkv.get_device(),
                op, ": caches must be on qkv's device");
  }
  const int64_t Tmax = Tp + To;
  auto chk = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.get_device() == qkv.get_device() && t.scalar_type() == at::kLong &&
                    t.is_contiguous() && t.numel() == B,
                op, ": ", name, " must be a contiguous int64 [B] tensor on qkv's device");
  };
  chk(start, "start");
  chk(nnew, "nnew");
  TORCH_CHECK(k_cache.get_device() == qkv.get_device() && v_cache.get_device() == qkv.get_device(),
              op, ": caches must be on qkv's device");
  TORCH_CHECK(kv_len_max >= 1 && kv_len_max <= Tmax, op, ": kv_len_max must be in [1, ", sh ? "Tp + To" : "Tmax", "]");
  TORCH_CHECK(scale > 0, op, ": scale must be positive");
  TORCH_CHECK(key_splits >= 0, op, ": key_splits must be 0 (the plan), 1 (never) or a chunk count, got ", key_splits);
  const Rope rp = [&] {
    const bool hc = rope_cos.has_value() && rope_cos->defined(), hs = rope_sin.has_value() && rope_sin->defined();
    TORCH_CHECK(hc == hs, op, ": rope_cos and rope_sin go together");
    if (!hc) return Rope{nullptr, nullptr};
    TORCH_CHECK(rope_cos->is_cuda() && rope_sin->is_cuda() && rope_cos->get_device() == qkv.get_device() &&
                    rope_sin->get_device() == qkv.get_device() && rope_cos->scalar_type() == at::kFloat &&
                    rope_sin->scalar_type() == at::kFloat && rope_cos->is_contiguous() && rope_sin->is_contiguous() &&
                    rope_cos->dim() == 2 && rope_cos->size(1) == D / 2 && rope_cos->size(0) >= Tmax &&
                    rope_sin->sizes() == rope_cos->sizes(),
                op, ": rope tables must be contiguous float32 [>= ", sh ? "Tp + To" : "Tmax", ", ", D / 2,
                "] on qkv's device at head dim ", D);
    return Rope{rope_cos->data_ptr<float>(), rope_sin->data_ptr<float>()};
  }();
  const int64_t nqb = (Tn + BLK - 1) / BLK;
  const int64_t total = B * Tn * Hkv * (D / 16);  // append_kv threads
  TORCH_CHECK(B * H * nqb < (1LL << 31) && (total + NT - 1) / NT < (1LL << 31) && Tmax < (1LL << 30) &&
                  Tn < (1LL << 30) && B * H * Tn < (1LL << 40),
              op, ": grid too large");
  at::Tensor out = at::empty({B, Tn, H * D}, qkv.options().memory_format(at::MemoryFormat::Contiguous));
  SharedAppendParams p;  // launched whole, or as its AppendParams base (the unshared kernels)
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
  p.kp = sh ? static_cast<const uint16_t*>(sh->k_prefix.data_ptr()) : nullptr;
  p.vp = sh ? static_cast<const uint16_t*>(sh->v_prefix.data_ptr()) : nullptr;
  p.plen = sh ? sh->plen.data_ptr<int64_t>() : nullptr;
  p.group = sh ? (int)sh->group : 1;
  p.Tp = (int)Tp;
  p.To = (int)To;
  // host values only (B, H, Tn, kv_len_max, D): the grids and the workspace are the same on every replay of a graph
  const SplitPlan sp = plan(B * H * nqb, p.L, D, key_splits);
  p.nsplit = sp.nsplit;
  p.chunk_tiles = sp.chunk_tiles;
  p.ws = nullptr;
  const int64_t nwg = B * H * nqb * sp.nsplit, nmerge = B * H * ((Tn + 31) / 32);
  TORCH_CHECK(nwg < (1LL << 31) && nmerge < (1LL << 31), op, ": grid too large");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  at::Tensor ws;  // allocated like `out`; every slot the merge reads is written by this call first
  if (sp.nsplit > 1) {
    ws = at::empty({nwg * 4 * (D + 1) * 32}, qkv.options().dtype(at::kFloat));
    p.ws = ws.data_ptr<float>();
  }
  hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto launch = [&](auto d_c, auto f8_c, auto sh_c) {
    constexpr int HD = decltype(d_c)::value;
    constexpr bool F8 = decltype(f8_c)::value;
    constexpr bool SH = decltype(sh_c)::value;
    const ParamsOf<SH> q = p;
    hipLaunchKernelGGL((append_kv_kernel<HD, F8, SH>), dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, q, total);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    if (sp.nsplit == 1) {
      hipLaunchKernelGGL((append_attn_kernel<HD, false, F8, SH>), dim3((unsigned)nwg), dim3(NT), 0, st, q);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      hipLaunchKernelGGL((append_attn_kernel<HD, true, F8, SH>), dim3((unsigned)nwg), dim3(NT), 0, st, q);
      C10_HIP_KERNEL_LAUNCH_CHECK();
      hipLaunchKernelGGL((append_merge_kernel<HD, SH>), dim3((unsigned)nmerge), dim3(NT), 0, st, q);  // fp32 partials only
      C10_HIP_KERNEL_LAUNCH_CHECK();
    }
  };
  auto launch_d = [&](auto f8_c, auto sh_c) {
    if (D == 64)
      launch(std::integral_constant<int, 64>{}, f8_c, sh_c);
    else
      launch(std::integral_constant<int, 128>{}, f8_c, sh_c);
  };
  if (sh) {
    if (f8)
      launch_d(std::true_type{}, std::true_type{});
    else
      launch_d(std::false_type{}, std::true_type{});
  } else {
    if (f8)
      launch_d(std::true_type{}, std::false_type{});
    else
      launch_d(std::false_type{}, std::false_type{});
  }
  return out;
}

at::Tensor append_attn_hip(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                           const at::Tensor& start, const at::Tensor& nnew, int64_t n_head, double scale,
                           int64_t kv_len_max, const c10::optional<at::Tensor>& rope_cos,
                           const c10::optional<at::Tensor>& rope_sin, int64_t key_splits) {
  return append_run(qkv, k_cache, v_cache, start, nnew, n_head, scale, kv_len_max, rope_cos, rope_sin, key_splits,
                    nullptr);
}

// sequence s of qkv [S = B·group, Tn, ...] continues prompt s / group: keys [0, plen[s / group]) are rows of
// k_prefix / v_prefix [B, Hkv, Tp, D] (read only), the rest its own rows k_own / v_own [S, Hkv, To, D];
// start [S] counts absolute positions, kv_len_max <= Tp + To
at::Tensor append_attn_shared_hip(const at::Tensor& qkv, const at::Tensor& k_prefix, const at::Tensor& v_prefix,
                                  const at::Tensor& plen, const at::Tensor& k_own, const at::Tensor& v_own,
                                  const at::Tensor& start, const at::Tensor& nnew, int64_t group, int64_t n_head,
                                  double scale, const c10::optional<at::Tensor>& rope_cos,
                                  const c10::optional<at::Tensor>& rope_sin, int64_t kv_len_max, int64_t key_splits) {
  const Shared sh{k_prefix, v_prefix, plen, group};
  return append_run(qkv, k_own, v_own, start, nnew, n_head, scale, kv_len_max, rope_cos, rope_sin, key_splits, &sh);
}

}  // namespace attn
}  // namespace nbd

TORCH_LIBRARY_IMPL(nbd, CUDA, m) {
  m.impl("append_attn", &nbd::attn::append_attn_hip);
  m.impl("append_attn_shared", &nbd::attn::append_attn_shared_hip);
}
TORCH_LIBRARY_IMPL(nbd, CompositeExplicitAutograd, m) { m.impl("append_attn_plan", &nbd::attn::append_attn_plan); }

