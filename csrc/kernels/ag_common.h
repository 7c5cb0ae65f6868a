// ag_common.h — shared by the autograd units: autograd.hip (the per-op nodes; defines every helper
// declared here), llama_block.hip (the fused decoder block, its HIP graphs) and cast_group.hip.
#pragma once
#include <ATen/ATen.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <functional>

#include "gemm_common.h"
#include "graddst.h"
#include "host_api.h"

namespace nbd {
namespace ag {
using at::Tensor;
using c10::optional;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;
using namespace nbd::gemm;

// ---- host-time breakdown of the block nodes (NBD_HOST_TIMING=1; torch.ops.nbd.host_timing) --
namespace ht {
enum Id { FWD, BWD, UNPACK, RMS_NEXT, SWIGLU, RMS_POST, LIN_O, ATTN, LIN_QKV, GEMM_CALL, PAIR_CALL, ATTN_CALL,
          CLAIM, ALLOC, kN };
inline std::atomic<int64_t> g_ns[kN], g_cnt[kN];
inline bool on() {
  static const bool e = [] {
    const char* v = std::getenv("NBD_HOST_TIMING");
    return v != nullptr && v[0] == '1';
  }();
  return e;
}
struct Scope {
  int id;
  bool active;
  std::chrono::steady_clock::time_point t0;
  explicit Scope(int i) : id(i), active(on()) {
    if (active) t0 = std::chrono::steady_clock::now();
  }
  ~Scope() {
    if (!active) return;
    g_ns[id] += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    ++g_cnt[id];
  }
};
}  // namespace ht

// ---- plans.  Which kernel (tile, split-K, or the hipBLASLt library GEMM) runs each product is
// decided in Python once per shape (ops/gemm.py `native_plan`) and passed down as an int list, so
// the native and the Python nodes pick identical kernels.  Wire layout: the products, 3 ints each
// (library?, tile, splits), then the grouped-launch split counts (-1 = products one by one):
//   linear_ag     int[10]  [fwd, dgrad, wgrad]                                        + [pair]
//   mlp_gelu_ag   int[20]  [fc, proj, proj dgrad, proj wgrad, fc dgrad, fc wgrad]     + [pair proj, pair fc]
//   mlp_swiglu_ag int[20]  [gate_up, down, down dgrad, down wgrad, gu dgrad, gu wgrad] + [pair down, pair gu]
struct Prod {
  bool lib;
  int64_t tile, splits;
  static Prod at(c10::IntArrayRef p, int i) { return {p[3 * i] != 0, p[3 * i + 1], p[3 * i + 2]}; }
};
struct LinearPlan {
  Prod fwd, dgrad, wgrad;
  int64_t pair;
  static LinearPlan parse(c10::IntArrayRef p) {
    TORCH_CHECK(p.size() == 10, "nbd autograd: a Linear plan is int[10], got ", p.size());
    return {Prod::at(p, 0), Prod::at(p, 1), Prod::at(p, 2), p[9]};
  }
};
struct MLPPlan {  // "up" = fc / gate_up, "down" = proj / down
  Prod up, down, down_dgrad, down_wgrad, up_dgrad, up_wgrad;
  int64_t pair_down, pair_up;
  static MLPPlan parse(c10::IntArrayRef p) {
    TORCH_CHECK(p.size() == 20, "nbd autograd: an MLP plan is int[20], got ", p.size());
    return {Prod::at(p, 0), Prod::at(p, 1), Prod::at(p, 2), Prod::at(p, 3), Prod::at(p, 4), Prod::at(p, 5), p[18], p[19]};
  }
};

inline bool aligned(const Tensor& t, int bytes = 16) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0; }
inline Tensor bf16c(const Tensor& t) {
  Tensor r = t.scalar_type() == at::kBFloat16 ? t : t.to(at::kBFloat16);
  return r.is_contiguous() ? r : r.contiguous();
}
inline optional<Tensor> opt(const Tensor& t) { return t.defined() ? optional<Tensor>(t.contiguous()) : c10::nullopt; }
inline std::vector<int64_t> out_shape(const Tensor& x, int64_t n) {
  std::vector<int64_t> s(x.sizes().begin(), x.sizes().end());
  s.back() = n;
  return s;
}
// A CPU scalar for a node's saved list: `f` runs when the backward releases the saved tensors
// (or the node dies) — how static memory learns that the pass which used it is over.
inline Tensor release_token(std::function<void()> f) {
  static int64_t dummy = 0;
  return at::from_blob(&dummy, {1}, [f](void*) { f(); }, at::TensorOptions().dtype(at::kLong));
}
// packed [B, T, (H + 2·Hkv)·D] -> q [B, H, T, D], k, v [B, Hkv, T, D] (views)
std::tuple<Tensor, Tensor, Tensor> split_qkv(const Tensor& qkv, int64_t H, int64_t Hkv);

// ---- GEMM calls (autograd.hip)
std::pair<Tensor, Tensor> run(const Tensor& a, const Tensor& b, bool a_km, bool b_kn, const Prod& p, int epi = EPI_NONE,
                              const optional<Tensor>& bias = c10::nullopt, const optional<Tensor>& aux = c10::nullopt,
                              const Tensor& c_out = Tensor(), const Tensor& rs_out = Tensor(), int accum = 0);
// A gradient output: the parameter's registered destination (graddst.h) or a fresh tensor.
struct GradOut {
  Tensor t;
  Tensor param;
  bool claimed = false, acc = false;
  int bit(int b) const { return acc ? b : 0; }
  Tensor done() const { return claimed ? graddst::hand_back(param, t, acc) : t; }
};
GradOut grad_out(const Tensor& param, bool want, at::IntArrayRef shape, const at::TensorOptions& opt);
std::tuple<Tensor, Tensor, Tensor> pair(const Tensor& dy, const Tensor& w, const Tensor& x, int epi1,
                                        const optional<Tensor>& aux1, bool bias_grad, int64_t splits,
                                        const Tensor& bparam = Tensor(), const Tensor& delta = Tensor(),
                                        int64_t delta_T = 0);
std::pair<Tensor, Tensor> wgrad(const Tensor& dy, const Tensor& x2, const Tensor& w, const Tensor& bparam, bool nb,
                                const Prod& p);
inline Tensor linear_forward(const Tensor& x2, const Tensor& w, const optional<Tensor>& b, const LinearPlan& plan) {
  return run(x2, w, false, false, plan.fwd, EPI_NONE, b).first;
}

// ---- the backward of each op, once: the per-op nodes and the fused decoder block both call
// these, which keeps the two bit-identical (same kernels, same order).
// (dx, dW, db) of y = x2·Wᵀ (+b); `delta` defined: also the flash backward's δ (autograd.hip adelta)
std::tuple<Tensor, Tensor, Tensor> linear_bwd_core(const Tensor& dy, const Tensor& x2, const Tensor& w, const Tensor& b,
                                                   const LinearPlan& plan, bool nx, bool nw, bool nb,
                                                   const Tensor& delta = Tensor());
// y = act·W_downᵀ (+b_down), act = gelu(pre) or silu(g)·u of pre = x2·W_upᵀ (+b_up): depi =
// EPI_DGELU / EPI_DSWIGLU (no biases)
struct MLPGrads { Tensor dx, dw_up, db_up, dw_down, db_down; };
MLPGrads mlp_bwd_core(int depi, const Tensor& dy, const Tensor& x2, const Tensor& w_up, const Tensor& w_down,
                      const Tensor& pre, const Tensor& act, const MLPPlan& plan, bool nx, const Tensor& b_up = Tensor(),
                      bool nb_up = false, const Tensor& b_down = Tensor(), bool nb_down = false);
// (d sum, dγ [, dβ]) of (s = x + δ, y = norm(s)) for dy and the sum's own gradient ds (may be
// undefined); dγ / dβ into their bucket slices when DDP registered them (graddst.h)
std::pair<Tensor, Tensor> rms_bwd_core(const Tensor& s, const Tensor& dy, const Tensor& ds, const Tensor& w,
                                       const Tensor& rstd);
std::tuple<Tensor, Tensor, Tensor> ln_bwd_core(const Tensor& s, const Tensor& dy, const Tensor& ds, const Tensor& w,
                                               const Tensor& bparam, const Tensor& mean, const Tensor& rstd);
// the packed dqkv of attention from packed q|k|v, for da [B, T, H·D]
Tensor attn_bwd_core(const Tensor& da, const Tensor& qkv, const Tensor& o, const Tensor& lse, int64_t H, int64_t Hkv,
                     bool causal, double scale, const optional<Tensor>& cos, const optional<Tensor>& sin,
                     const Tensor& delta = Tensor());

// ---- the links between the block graphs (llama_block.hip) and the kept casts (cast_group.hip)
namespace castbuf {
bool kept(const Tensor& t);  // t lives in a kept cast buffer (its address is stable across steps)
// minus kept cast buffers: the cache keeps those alive; a graph holding them would make them look in use
std::vector<Tensor> drop_kept(std::vector<Tensor> refs);
}  // namespace castbuf
namespace bg {
// Casts into kept buffers (CastGroupFn) since process start.  A stack graph replays every member
// at the head's call, so a cast between two member calls would be read one step late: serving
// checks that none ran since the head's replay.
extern std::atomic<uint64_t> g_cast_epoch;
}  // namespace bg

}  // namespace ag
}  // namespace nbd
