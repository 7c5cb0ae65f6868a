// autograd.hip — the per-op autograd nodes of the model paths in C++.
//
// An eager training step of a small model is host-bound: SmolLM2-135M at 16x128 tokens spends
// ≈11 ms issuing what the GPU runs in 7 ms (graph replay), and a Python torch.autograd.Function
// costs ≈20-25 µs per call before its kernels (ctx object, saved tensors, Python wrappers around
// every GEMM) — forward and again backward (benchmarks/host_profile.py --cprofile).  These nodes
// run the same kernels (gemm.hip: fused bias / GELU / SwiGLU epilogues, the grouped dgrad + wgrad
// backward launch) with no Python between the dispatcher and the launches; the kernel of each
// product comes down from Python as a plan (ag_common.h).
// Here: Linear and the two MLPs (Python reference: ops/gemm.py _Linear / _MLPGelu / _MLPSwiGLU —
// same math, same kernels), the (add +) RMSNorm / LayerNorm nodes (ops/llama.py _RMSNorm /
// _AddRMSNorm, ops/norm.py _LayerNorm / _AddLayerNorm), the embedding + norm nodes, attention
// from a packed q|k|v projection (ops/attention.py _FlashAttentionQKV) — and the helpers and
// per-op backward cores of ag_common.h, which llama_block.hip's fused decoder block shares.
#include <mutex>
#include <unordered_map>

#include "ag_common.h"

namespace nbd {
namespace ag {

// c = A·B (layouts as gemm.hip), `epi` with its operands; returns (c, aux_out).  The library path
// (hipBLASLt through at::mm / addmm) serves plain products the plan routes there, and any plain
// product whose operands are not 16-byte aligned (as ops.gemm.matmul does).  `c_out` / `rs_out`:
// write the product / row sums there (gradient destinations, graddst.h), adding to their contents
// when `accum` bit 0 / bit 1 is set.
std::pair<Tensor, Tensor> run(const Tensor& a, const Tensor& b, bool a_km, bool b_kn, const Prod& p, int epi,
                              const optional<Tensor>& bias, const optional<Tensor>& aux, const Tensor& c_out,
                              const Tensor& rs_out, int accum) {
  const int64_t M = a_km ? a.size(1) : a.size(0), N = b_kn ? b.size(1) : b.size(0);
  const bool bias_ok = !bias || (bias->is_contiguous() && aligned(*bias, 8) && bias->scalar_type() == at::kBFloat16);
  const bool out_ok = !c_out.defined() || aligned(c_out);
  if (epi == EPI_NONE && (p.lib || !aligned(a) || !aligned(b) || !bias_ok || !out_ok)) {
    const Tensor A = a_km ? a.t() : a, B = b_kn ? b : b.t();
    if (c_out.defined()) {
      TORCH_CHECK(!bias, "nbd autograd: bias with a destination");
      if (accum & 1) c_out.view({M, N}).addmm_(A, B);
      else {
        Tensor o = c_out.view({M, N});
        at::mm_out(o, A, B);
      }
      return {c_out, Tensor()};
    }
    return {bias ? at::addmm(*bias, A, B) : at::mm(A, B), Tensor()};
  }
  const int64_t cN = epi == EPI_SWIGLU ? N / 2 : epi == EPI_DSWIGLU ? 2 * N : N;
  // the 256x256 kernel has no accumulating epilogue: product into a temporary, then add
  const bool tmp_acc = accum != 0 && (p.tile / 1000 % 1000) == 256;
  Tensor c = c_out.defined() && !(tmp_acc && (accum & 1)) ? c_out.view({M, cN}) : at::empty({M, cN}, a.options());
  Tensor out;
  if (epi == EPI_GELU) out = at::empty_like(c);
  if (epi == EPI_ROWSUM) out = rs_out.defined() && !(tmp_acc && (accum & 2)) ? rs_out.view({M}) : at::empty({M}, a.options());
  if (epi == EPI_SWIGLU) out = at::empty({M, N}, a.options());
  // a deferred split-K reduce only when it writes the destinations themselves (not a temporary
  // that is read right after)
  const defer::Scope ds(defer::want() && !tmp_acc && c_out.defined() && (epi != EPI_ROWSUM || rs_out.defined()));
  {
    const ht::Scope hs(ht::GEMM_CALL);
    gemm_hip(a, b, c, a_km, b_kn, bias, epi, aux, out.defined() ? optional<Tensor>(out) : c10::nullopt, p.splits,
             p.tile, tmp_acc ? 0 : accum);
  }
  if (tmp_acc) {
    if (accum & 1) { c_out.view({M, cN}).add_(c); c = c_out.view({M, cN}); }
    if (accum & 2) { rs_out.view({M}).add_(out); out = rs_out.view({M}); }
  }
  return {c, out};
}

GradOut grad_out(const Tensor& param, bool want, at::IntArrayRef shape, const at::TensorOptions& opt) {
  const ht::Scope hs(ht::CLAIM);
  GradOut g;
  if (!want) return g;
  if (param.defined()) {
    g.t = graddst::claim(param, g.acc);
    g.claimed = g.t.defined();
    if (g.claimed) {
      g.param = param;
      if (!aligned(g.t) || g.t.scalar_type() != opt.dtype().toScalarType()) {  // unusable: normal path
        g = GradOut();
      }
    }
  }
  if (!g.claimed) g.t = at::empty(shape, opt);
  return g;
}

// dx = dy·W [· act′(aux)], dW = dyᵀ·x [, db = Σ dy] in one grouped launch (gemm_pair_hip)
std::tuple<Tensor, Tensor, Tensor> pair(const Tensor& dy, const Tensor& w, const Tensor& x, int epi1,
                                        const optional<Tensor>& aux1, bool bias_grad, int64_t splits,
                                        const Tensor& bparam, const Tensor& delta, int64_t delta_T) {
  const int64_t M = dy.size(0), N = dy.size(1), K = w.size(1);
  Tensor dx = at::empty({M, epi1 == EPI_DSWIGLU ? 2 * K : K}, dy.options());
  const GradOut dw = grad_out(w, true, {N, K}, dy.options());
  const GradOut db = grad_out(bparam, bias_grad, {N}, dy.options());
  // every output of the split-K reduce is a bucket slice: it may be deferred (graddst.h)
  const defer::Scope ds(dw.claimed && (!bias_grad || db.claimed));
  {
    const ht::Scope hs(ht::PAIR_CALL);
    gemm_pair_hip(dy, w, dx, epi1, aux1, dy, x, dw.t.view({N, K}), bias_grad ? EPI_ROWSUM : EPI_NONE,
                  bias_grad ? optional<Tensor>(db.t.view({N})) : c10::nullopt, splits, dw.bit(1) | db.bit(2),
                  delta.defined() ? optional<Tensor>(delta) : c10::nullopt, delta_T);
  }
  return {dx, dw.done(), bias_grad ? db.done() : Tensor()};
}

// dW = dyᵀ·x [, db = Σ dy] as a separate product `p`, into the gradient destinations
std::pair<Tensor, Tensor> wgrad(const Tensor& dy, const Tensor& x2, const Tensor& w, const Tensor& bparam, bool nb,
                                const Prod& p) {
  const int64_t N = dy.size(1), K = x2.size(1);
  const GradOut dw = grad_out(w, true, {N, K}, dy.options());
  const GradOut db = grad_out(bparam, nb, {N}, dy.options());
  const defer::Scope ds(dw.claimed && (!nb || db.claimed));
  run(dy, x2, true, true, p, nb ? EPI_ROWSUM : EPI_NONE, c10::nullopt, c10::nullopt, dw.t,
      nb ? db.t : Tensor(), dw.bit(1) | db.bit(2));
  return {dw.done(), nb ? db.done() : Tensor()};
}

// ---- the backward of each op (ag_common.h)
std::tuple<Tensor, Tensor, Tensor> linear_bwd_core(const Tensor& dy, const Tensor& x2, const Tensor& w, const Tensor& b,
                                                   const LinearPlan& plan, bool nx, bool nw, bool nb,
                                                   const Tensor& delta) {
  Tensor dx, dw, db;
  if (nx && nw && plan.pair >= 0) {
    const bool d = delta.defined();
    std::tie(dx, dw, db) = pair(dy, w, x2, d ? EPI_ADELTA : EPI_NONE, d ? optional<Tensor>(x2) : c10::nullopt, nb,
                                plan.pair, b, delta, d ? delta.size(2) : 0);
  } else {
    if (nx) dx = run(dy, w, false, true, plan.dgrad).first;
    if (nw) std::tie(dw, db) = wgrad(dy, x2, w, b, nb, plan.wgrad);
    else if (nb) db = dy.sum(0, false, at::kFloat).to(dy.scalar_type());
  }
  return {dx, dw, db};
}

MLPGrads mlp_bwd_core(int depi, const Tensor& dy, const Tensor& x2, const Tensor& w_up, const Tensor& w_down,
                      const Tensor& pre, const Tensor& act, const MLPPlan& plan, bool nx, const Tensor& b_up, bool nb_up,
                      const Tensor& b_down, bool nb_down) {
  MLPGrads g;
  Tensor dpre;
  if (plan.pair_down >= 0) {
    std::tie(dpre, g.dw_down, g.db_down) = pair(dy, w_down, act, depi, pre, nb_down, plan.pair_down, b_down);
  } else {
    dpre = run(dy, w_down, false, true, plan.down_dgrad, depi, c10::nullopt, pre).first;
    std::tie(g.dw_down, g.db_down) = wgrad(dy, act, w_down, b_down, nb_down, plan.down_wgrad);
  }
  if (nx && plan.pair_up >= 0) {
    std::tie(g.dx, g.dw_up, g.db_up) = pair(dpre, w_up, x2, EPI_NONE, c10::nullopt, nb_up, plan.pair_up, b_up);
  } else {
    if (nx) g.dx = run(dpre, w_up, false, true, plan.up_dgrad).first;
    std::tie(g.dw_up, g.db_up) = wgrad(dpre, x2, w_up, b_up, nb_up, plan.up_wgrad);
  }
  return g;
}

std::pair<Tensor, Tensor> rms_bwd_core(const Tensor& s, const Tensor& dy, const Tensor& ds, const Tensor& w,
                                       const Tensor& rstd) {
  const GradOut gw = grad_out(w, w.requires_grad(), w.sizes(), w.options());
  const defer::Scope dsc(gw.claimed);  // the column sum may be deferred
  auto [dx, dw] = norm::rms_bwd_into(s, dy.contiguous(), opt(ds), w, rstd, gw.t, gw.bit(1));
  return {dx, gw.t.defined() ? gw.done() : dw};
}

std::tuple<Tensor, Tensor, Tensor> ln_bwd_core(const Tensor& s, const Tensor& dy, const Tensor& ds, const Tensor& w,
                                               const Tensor& bparam, const Tensor& mean, const Tensor& rstd) {
  const GradOut gw = grad_out(w, w.requires_grad(), w.sizes(), w.options());
  const GradOut gb = grad_out(bparam, true, w.sizes(), w.options());
  const defer::Scope dsc(gw.claimed && gb.claimed);
  auto [dx, dw, db] = norm::ln_bwd_into(s, dy.contiguous(), opt(ds), w, mean, rstd, gw.t, gb.t, gw.bit(1) | gb.bit(2));
  return {dx, gw.t.defined() ? gw.done() : dw, gb.t.defined() ? gb.done() : db};
}

std::tuple<Tensor, Tensor, Tensor> split_qkv(const Tensor& qkv, int64_t H, int64_t Hkv) {
  const int64_t B = qkv.size(0), T = qkv.size(1), D = qkv.size(2) / (H + 2 * Hkv);
  return {qkv.narrow(2, 0, H * D).view({B, T, H, D}).transpose(1, 2),
          qkv.narrow(2, H * D, Hkv * D).view({B, T, Hkv, D}).transpose(1, 2),
          qkv.narrow(2, (H + Hkv) * D, Hkv * D).view({B, T, Hkv, D}).transpose(1, 2)};
}

Tensor attn_bwd_core(const Tensor& da, const Tensor& qkv, const Tensor& o, const Tensor& lse, int64_t H, int64_t Hkv,
                     bool causal, double scale, const optional<Tensor>& cos, const optional<Tensor>& sin,
                     const Tensor& delta) {
  const int64_t B = qkv.size(0), T = qkv.size(1), D = qkv.size(2) / (H + 2 * Hkv);
  auto [q, k, v] = split_qkv(qkv, H, Hkv);
  Tensor dqkv = at::empty_like(qkv, at::MemoryFormat::Contiguous);
  auto [dq, dk, dv] = split_qkv(dqkv, H, Hkv);
  const Tensor dout = da.contiguous().view({B, T, H, D}).transpose(1, 2);
  const ht::Scope hs(ht::ATTN_CALL);
  attn::attn_bwd_hip(dout, q, k, v, o, lse, causal, scale, dq, dk, dv, cos, sin,
                     delta.defined() ? optional<Tensor>(delta) : c10::nullopt);
  return dqkv;
}

// ---- the flash backward's δ from the output projection (GPT-2: attention -> c_proj) ----------
// δ = Σ_d dO·O per (query, head) is the attention backward's pre-pass; dO is the input gradient
// of the Linear that consumes the attention output O, so that Linear's grouped backward launch
// can produce δ in its epilogue (gemm.hip EPI_ADELTA) and the pre-pass launch goes away.  The
// attention node registers its output here at forward time; the Linear's backward, finding its
// input registered, fills δ; the attention's backward takes it only if its dout IS that Linear's
// input gradient (a second consumer of O would have summed gradients into another tensor).
namespace adelta {
struct Req {
  int64_t T = 0, H = 0;
  Tensor delta;             // filled by the Linear's backward
  const void* dx = nullptr;  // ... for this input gradient
};
std::mutex mu;
std::unordered_map<const void*, Req> reqs;

static bool enabled() {
  static const bool on = [] {
    const char* e = std::getenv("NBD_ATTN_DELTA_EPI");  // 0: the pre-pass kernel (A/B)
    return e == nullptr || e[0] != '0';
  }();
  return on;
}
static void want(const Tensor& o, int64_t T, int64_t H) {
  std::lock_guard<std::mutex> lk(mu);
  reqs[o.data_ptr()] = Req{T, H, Tensor(), nullptr};  // (a new forward resets a stale entry)
}
// the δ tensor to fill for the Linear input x2 [B·T, H·64], or undefined
static Tensor request(const Tensor& x2) {
  std::lock_guard<std::mutex> lk(mu);
  auto it = reqs.find(x2.data_ptr());
  if (it == reqs.end()) return Tensor();
  Req& r = it->second;
  if (x2.dim() != 2 || x2.size(1) != r.H * 64 || r.T <= 0 || x2.size(0) % r.T != 0) return Tensor();
  r.delta = at::empty({x2.size(0) / r.T, r.H, r.T}, x2.options().dtype(at::kFloat));
  r.dx = nullptr;
  return r.delta;
}
static void produced(const Tensor& x2, const Tensor& dx) {
  std::lock_guard<std::mutex> lk(mu);
  auto it = reqs.find(x2.data_ptr());
  if (it != reqs.end()) it->second.dx = dx.data_ptr();
}
// δ for the attention output o whose incoming gradient is dout (and forget the entry)
static Tensor take(const Tensor& o, const Tensor& dout) {
  std::lock_guard<std::mutex> lk(mu);
  auto it = reqs.find(o.data_ptr());
  if (it == reqs.end()) return Tensor();
  Tensor d = (it->second.delta.defined() && it->second.dx == dout.data_ptr()) ? it->second.delta : Tensor();
  reqs.erase(it);
  return d;
}
}  // namespace adelta

// ------------------------------------------------------------------------------------- Linear
// fp32 / fp16 weights (a user's nn.Linear under nbd DDP, parallel/ddp.py): the library GEMMs, with
// the weight / bias gradients written into their DDP bucket slices like the bf16 path
static bool lib_dtype(const Tensor& w) { return w.scalar_type() != at::kBFloat16; }

struct LinearFn : public torch::autograd::Function<LinearFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& w, const optional<Tensor>& b,
                        at::IntArrayRef plan_ints) {
    at::AutoDispatchBelowADInplaceOrView guard;
    const LinearPlan plan = LinearPlan::parse(plan_ints);
    const bool lib = lib_dtype(w);
    const Tensor x2 = lib ? x.reshape({-1, x.size(-1)}).contiguous() : bf16c(x).view({-1, x.size(-1)});
    ctx->save_for_backward({x2, w, b ? *b : Tensor()});
    ctx->saved_data["plan"] = plan_ints.vec();
    ctx->saved_data["need"] = std::vector<bool>{x.requires_grad(), w.requires_grad(), b && b->requires_grad()};
    ctx->saved_data["xshape"] = x.sizes().vec();
    if (lib) {
      const Tensor y = b ? at::addmm(*b, x2, w.t()) : at::mm(x2, w.t());
      return y.view(out_shape(x, w.size(0)));
    }
    return linear_forward(x2, w, b, plan).view(out_shape(x, w.size(0)));
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &x2 = saved[0], &w = saved[1], &b = saved[2];
    const LinearPlan plan = LinearPlan::parse(ctx->saved_data["plan"].toIntVector());
    const auto need = ctx->saved_data["need"].toBoolList();
    const auto xshape = ctx->saved_data["xshape"].toIntVector();
    const bool nx = need[0], nw = need[1], nb = need[2];
    Tensor dx, dw, db;
    if (lib_dtype(w)) {
      const Tensor dy = grads[0].reshape({-1, w.size(0)}).contiguous();
      if (nx) dx = at::mm(dy, w);
      if (nw) {
        const GradOut g = grad_out(w, true, w.sizes(), dy.options());
        if (g.acc) g.t.addmm_(dy.t(), x2);
        else {
          Tensor o = g.t;
          at::mm_out(o, dy.t(), x2);
        }
        dw = g.done();
      }
      if (nb) {
        const GradOut g = grad_out(b, true, {w.size(0)}, dy.options());
        if (g.acc) g.t.add_(dy.sum(0));
        else {
          Tensor o = g.t;
          at::sum_out(o, dy, {0});
        }
        db = g.done();
      }
      return {dx.defined() ? dx.view(xshape) : dx, dw, db, Tensor()};
    }
    const Tensor dy = bf16c(grads[0]).view({-1, w.size(0)});
    // an attention output as this Linear's input: the flash backward's δ from the grouped launch
    const Tensor delta = nx && nw && plan.pair >= 0 && adelta::enabled() ? adelta::request(x2) : Tensor();
    std::tie(dx, dw, db) = linear_bwd_core(dy, x2, w, b, plan, nx, nw, nb, delta);
    if (delta.defined()) adelta::produced(x2, dx);
    return {dx.defined() ? dx.view(xshape) : dx, dw, db, Tensor()};
  }
};

Tensor linear_ag(const Tensor& x, const Tensor& w, const optional<Tensor>& b, at::IntArrayRef plan) {
  return LinearFn::apply(x, w, b, plan);
}

Tensor linear_noag(const Tensor& x, const Tensor& w, const optional<Tensor>& b, at::IntArrayRef plan) {
  if (lib_dtype(w)) {
    const Tensor x2 = x.reshape({-1, x.size(-1)});
    return (b ? at::addmm(*b, x2, w.t()) : at::mm(x2, w.t())).view(out_shape(x, w.size(0)));
  }
  return linear_forward(bf16c(x).view({-1, x.size(-1)}), w, b, LinearPlan::parse(plan)).view(out_shape(x, w.size(0)));
}

// ------------------------------------------------------------------------------ GPT-2 MLP (GELU)
struct MLPGeluFn : public torch::autograd::Function<MLPGeluFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& w1, const optional<Tensor>& b1,
                        const Tensor& w2, const optional<Tensor>& b2, at::IntArrayRef plan_ints) {
    at::AutoDispatchBelowADInplaceOrView guard;
    const MLPPlan plan = MLPPlan::parse(plan_ints);
    const Tensor x2 = bf16c(x).view({-1, x.size(-1)});
    auto [g, pre] = run(x2, w1, false, false, plan.up, EPI_GELU, b1);
    const Tensor y = run(g, w2, false, false, plan.down, EPI_NONE, b2).first;
    ctx->save_for_backward({x2, w1, w2, pre, g, b1 ? *b1 : Tensor(), b2 ? *b2 : Tensor()});
    ctx->saved_data["plan"] = plan_ints.vec();
    ctx->saved_data["need"] = std::vector<bool>{x.requires_grad(), b1.has_value(), b2.has_value()};
    ctx->saved_data["xshape"] = x.sizes().vec();
    return y.view(out_shape(x, w2.size(0)));
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    const Tensor &x2 = s[0], &w1 = s[1], &w2 = s[2], &pre = s[3], &g = s[4], &b1 = s[5], &b2 = s[6];
    const MLPPlan plan = MLPPlan::parse(ctx->saved_data["plan"].toIntVector());
    const auto need = ctx->saved_data["need"].toBoolList();  // [x wants a gradient, has b1, has b2]
    const auto xshape = ctx->saved_data["xshape"].toIntVector();
    const Tensor dy = bf16c(grads[0]).view({-1, w2.size(0)});
    const MLPGrads r = mlp_bwd_core(EPI_DGELU, dy, x2, w1, w2, pre, g, plan, need[0], b1, need[1], b2, need[2]);
    return {r.dx.defined() ? r.dx.view(xshape) : r.dx, r.dw_up, r.db_up, r.dw_down, r.db_down, Tensor()};
  }
};

Tensor mlp_gelu_ag(const Tensor& x, const Tensor& w1, const optional<Tensor>& b1, const Tensor& w2,
                   const optional<Tensor>& b2, at::IntArrayRef plan) {
  return MLPGeluFn::apply(x, w1, b1, w2, b2, plan);
}

Tensor mlp_gelu_noag(const Tensor& x, const Tensor& w1, const optional<Tensor>& b1, const Tensor& w2,
                     const optional<Tensor>& b2, at::IntArrayRef plan_ints) {
  const MLPPlan plan = MLPPlan::parse(plan_ints);
  const Tensor x2 = bf16c(x).view({-1, x.size(-1)});
  const Tensor g = run(x2, w1, false, false, plan.up, EPI_GELU, b1).first;
  return run(g, w2, false, false, plan.down, EPI_NONE, b2).first.view(out_shape(x, w2.size(0)));
}

// ----------------------------------------------------------------------------- Llama MLP (SwiGLU)
struct MLPSwiGLUFn : public torch::autograd::Function<MLPSwiGLUFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& w_gu, const Tensor& w_down,
                        at::IntArrayRef plan_ints) {
    at::AutoDispatchBelowADInplaceOrView guard;
    const MLPPlan plan = MLPPlan::parse(plan_ints);
    const Tensor x2 = bf16c(x).view({-1, x.size(-1)});
    auto [act, pre] = run(x2, w_gu, false, false, plan.up, EPI_SWIGLU);
    const Tensor y = run(act, w_down, false, false, plan.down).first;
    ctx->save_for_backward({x2, w_gu, w_down, pre, act});
    ctx->saved_data["plan"] = plan_ints.vec();
    ctx->saved_data["nx"] = x.requires_grad();
    ctx->saved_data["xshape"] = x.sizes().vec();
    return y.view(out_shape(x, w_down.size(0)));
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    const Tensor &x2 = s[0], &w_gu = s[1], &w_down = s[2], &pre = s[3], &act = s[4];
    const MLPPlan plan = MLPPlan::parse(ctx->saved_data["plan"].toIntVector());
    const bool nx = ctx->saved_data["nx"].toBool();
    const auto xshape = ctx->saved_data["xshape"].toIntVector();
    const Tensor dy = bf16c(grads[0]).view({-1, w_down.size(0)});
    const MLPGrads r = mlp_bwd_core(EPI_DSWIGLU, dy, x2, w_gu, w_down, pre, act, plan, nx);
    return {r.dx.defined() ? r.dx.view(xshape) : r.dx, r.dw_up, r.dw_down, Tensor()};
  }
};

Tensor mlp_swiglu_ag(const Tensor& x, const Tensor& w_gu, const Tensor& w_down, at::IntArrayRef plan) {
  return MLPSwiGLUFn::apply(x, w_gu, w_down, plan);
}

Tensor mlp_swiglu_noag(const Tensor& x, const Tensor& w_gu, const Tensor& w_down, at::IntArrayRef plan_ints) {
  const MLPPlan plan = MLPPlan::parse(plan_ints);
  const Tensor x2 = bf16c(x).view({-1, x.size(-1)});
  const Tensor act = run(x2, w_gu, false, false, plan.up, EPI_SWIGLU).first;
  return run(act, w_down, false, false, plan.down).first.view(out_shape(x, w_down.size(0)));
}

// ------------------------------------------------------------ (add +) RMSNorm / LayerNorm nodes
// The residual add and the norm in one pass forward (s = x + delta, y = norm(s)), their
// backward in one pass too (dx = ds + norm′(dy)).  ``delta`` absent: the plain norm (one output).
struct RMSFn : public torch::autograd::Function<RMSFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const optional<Tensor>& delta, const Tensor& w,
                               double eps) {
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->set_materialize_grads(false);
    auto [y, sum, rstd] = norm::rms_fwd_hip(x, delta, w, eps);
    const bool add = delta.has_value();
    ctx->save_for_backward({add ? sum : x, w, rstd});
    ctx->saved_data["add"] = add;
    if (add) return {sum, y};
    return {y};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const bool add = ctx->saved_data["add"].toBool();
    const Tensor ds = add ? grads[0] : Tensor(), dy = add ? grads[1] : grads[0];
    if (!dy.defined()) return {ds, ds, Tensor(), Tensor()};
    auto [dx, dw] = rms_bwd_core(saved[0], dy, ds, saved[1], saved[2]);
    return {dx, add ? dx : Tensor(), dw, Tensor()};
  }
};

struct LNFn : public torch::autograd::Function<LNFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const optional<Tensor>& delta, const Tensor& w,
                               const Tensor& b, double eps) {
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->set_materialize_grads(false);
    auto [y, sum, mean, rstd] = norm::ln_fwd_hip(x, delta, w, b, eps);
    const bool add = delta.has_value();
    ctx->save_for_backward({add ? sum : x, w, mean, rstd});
    ctx->saved_data["add"] = add;
    if (b.requires_grad()) ctx->saved_data["b"] = b;  // (identity only: its gradient's bucket slice)
    if (add) return {sum, y};
    return {y};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const bool add = ctx->saved_data["add"].toBool();
    const Tensor ds = add ? grads[0] : Tensor(), dy = add ? grads[1] : grads[0];
    if (!dy.defined()) return {ds, ds, Tensor(), Tensor(), Tensor()};
    // (the bias is not saved as a tensor: only its identity, for its gradient's slice)
    const Tensor b = ctx->saved_data.count("b") ? ctx->saved_data["b"].toTensor() : Tensor();
    auto [dx, dw, db] = ln_bwd_core(saved[0], dy, ds, saved[1], b, saved[2], saved[3]);
    return {dx, add ? dx : Tensor(), dw, db, Tensor()};
  }
};

// The gradient of an embedding table from the gradient at its gathered rows (ids < V; rows of the
// table past V are padding and get zeros): into the table's DDP bucket slice when it has one — or,
// when a tied LM head already wrote this pass's gradient there, added into it (nothing returned)
static Tensor table_grad(const Tensor& table, const Tensor& dx, const Tensor& ids, int64_t V) {
  const int64_t C = table.size(1);
  const Tensor d2 = dx.reshape({-1, C}).contiguous(), id1 = ids.reshape({-1});
  const Tensor j = graddst::grad_dest_join(table);
  if (j.numel() > 0 && j.scalar_type() == d2.scalar_type()) {
    embed::embedding_bwd_hip(d2, id1, V, j.view(table.sizes()), true);
    return Tensor();
  }
  const GradOut gt = grad_out(table, true, table.sizes(), table.options());
  embed::embedding_bwd_hip(d2, id1, V, gt.t, gt.acc);
  return gt.done();
}

// Token embedding + the first RMSNorm (Llama): one forward launch (norm.hip embed_rms_kernel)
// returning the residual stream x0 and h0 = RMSNorm(x0); in backward the two incoming gradients
// meet here, so the norm's backward adds the residual stream's gradient in its own pass (no
// separate add), and the table's gradient goes straight into its DDP bucket slice (graddst.h).
struct EmbedRMSFn : public torch::autograd::Function<EmbedRMSFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& ids, const Tensor& table, const Tensor& w,
                               double eps, const optional<Tensor>& err) {
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->set_materialize_grads(false);
    auto [x0, y, rstd] = norm::embed_rms_fwd_hip(ids, table, w, eps, err);
    ctx->save_for_backward({ids, x0, w, rstd});
    ctx->saved_data["table"] = table;  // (its bucket slice; the values are not read)
    return {x0, y};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &ids = saved[0], &x0 = saved[1], &w = saved[2];
    const Tensor table = ctx->saved_data["table"].toTensor();
    const Tensor ds = grads[0], dy = grads[1];
    Tensor dx = ds, dw_ret;
    if (dy.defined()) std::tie(dx, dw_ret) = rms_bwd_core(x0, dy, ds, w, saved[3]);
    const Tensor dtable = dx.defined() && table.requires_grad() ? table_grad(table, dx, ids, table.size(0)) : Tensor();
    return {Tensor(), dtable, dw_ret, Tensor(), Tensor()};
  }
};

// GPT-2's token + position embedding + the first LayerNorm: one forward launch (norm.hip
// tokpos_ln_kernel); in backward the norm's pass adds the residual stream's gradient, then the
// token table's gradient (bucket slice / tied head: table_grad) and the position table's
// (the batch summed per position, into its slice: embedding_pos_bwd).
struct TokPosLNFn : public torch::autograd::Function<TokPosLNFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& idx, const Tensor& wte, const Tensor& pos,
                               const Tensor& wpe, const Tensor& w, const Tensor& b, int64_t vocab, double eps,
                               const optional<Tensor>& err) {
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->set_materialize_grads(false);
    auto [x0, y, mean, rstd] = norm::tokpos_ln_fwd_hip(idx, wte, pos, wpe, vocab, w, b, eps, err);
    ctx->save_for_backward({idx, pos, x0, w, mean, rstd});
    ctx->saved_data["wte"] = wte;  // (identities only: their gradients' bucket slices)
    ctx->saved_data["wpe"] = wpe;
    if (b.requires_grad()) ctx->saved_data["b"] = b;
    ctx->saved_data["V"] = vocab > 0 ? std::min<int64_t>(vocab, wte.size(0)) : wte.size(0);
    return {x0, y};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &idx = saved[0], &pos = saved[1], &x0 = saved[2], &w = saved[3];
    const Tensor wte = ctx->saved_data["wte"].toTensor(), wpe = ctx->saved_data["wpe"].toTensor();
    const Tensor ds = grads[0], dy = grads[1];
    Tensor dx = ds, dw_ret, db_ret;
    if (dy.defined()) {
      const Tensor b = ctx->saved_data.count("b") ? ctx->saved_data["b"].toTensor() : Tensor();
      std::tie(dx, dw_ret, db_ret) = ln_bwd_core(x0, dy, ds, w, b, saved[4], saved[5]);
    }
    Tensor dwte, dwpe;
    if (dx.defined()) {
      if (wte.requires_grad()) dwte = table_grad(wte, dx, idx, ctx->saved_data["V"].toInt());
      if (wpe.requires_grad()) {
        const int64_t C = wpe.size(1), P = wpe.size(0);
        const Tensor d2 = dx.reshape({-1, C}).contiguous();
        const GradOut gp = grad_out(wpe, true, wpe.sizes(), wpe.options());
        embed::embedding_pos_bwd_hip(d2, pos, P, gp.t, gp.acc);
        dwpe = gp.done();
      }
    }
    return {Tensor(), dwte, Tensor(), dwpe, dw_ret, db_ret, Tensor(), Tensor(), Tensor()};
  }
};

std::tuple<Tensor, Tensor> tokpos_layer_norm_ag(const Tensor& idx, const Tensor& wte, const Tensor& pos,
                                                const Tensor& wpe, const Tensor& w, const Tensor& b, int64_t vocab,
                                                double eps, const optional<Tensor>& err) {
  auto r = TokPosLNFn::apply(idx, wte, pos, wpe, w, b, vocab, eps, err);
  return {r[0], r[1]};
}
std::tuple<Tensor, Tensor> tokpos_layer_norm_noag(const Tensor& idx, const Tensor& wte, const Tensor& pos,
                                                  const Tensor& wpe, const Tensor& w, const Tensor& b, int64_t vocab,
                                                  double eps, const optional<Tensor>& err) {
  auto r = norm::tokpos_ln_fwd_hip(idx, wte, pos, wpe, vocab, w, b, eps, err);
  return {std::get<0>(r), std::get<1>(r)};
}

std::tuple<Tensor, Tensor> embed_rms_norm_ag(const Tensor& ids, const Tensor& table, const Tensor& w, double eps,
                                             const optional<Tensor>& err) {
  auto r = EmbedRMSFn::apply(ids, table, w, eps, err);
  return {r[0], r[1]};
}
std::tuple<Tensor, Tensor> embed_rms_norm_noag(const Tensor& ids, const Tensor& table, const Tensor& w, double eps,
                                               const optional<Tensor>& err) {
  auto r = norm::embed_rms_fwd_hip(ids, table, w, eps, err);
  return {std::get<0>(r), std::get<1>(r)};
}

Tensor rms_norm_ag(const Tensor& x, const Tensor& w, double eps) { return RMSFn::apply(x, c10::nullopt, w, eps)[0]; }
std::tuple<Tensor, Tensor> add_rms_norm_ag(const Tensor& x, const Tensor& delta, const Tensor& w, double eps) {
  auto r = RMSFn::apply(x, optional<Tensor>(delta), w, eps);
  return {r[0], r[1]};
}
Tensor layer_norm_ag(const Tensor& x, const Tensor& w, const Tensor& b, double eps) {
  return LNFn::apply(x, c10::nullopt, w, b, eps)[0];
}
std::tuple<Tensor, Tensor> add_layer_norm_ag(const Tensor& x, const Tensor& delta, const Tensor& w, const Tensor& b,
                                             double eps) {
  auto r = LNFn::apply(x, optional<Tensor>(delta), w, b, eps);
  return {r[0], r[1]};
}
Tensor rms_norm_noag(const Tensor& x, const Tensor& w, double eps) {
  return std::get<0>(norm::rms_fwd_hip(x, c10::nullopt, w, eps));
}
std::tuple<Tensor, Tensor> add_rms_norm_noag(const Tensor& x, const Tensor& delta, const Tensor& w, double eps) {
  auto r = norm::rms_fwd_hip(x, delta, w, eps);
  return {std::get<1>(r), std::get<0>(r)};
}
Tensor layer_norm_noag(const Tensor& x, const Tensor& w, const Tensor& b, double eps) {
  return std::get<0>(norm::ln_fwd_hip(x, c10::nullopt, w, b, eps));
}
std::tuple<Tensor, Tensor> add_layer_norm_noag(const Tensor& x, const Tensor& delta, const Tensor& w, const Tensor& b,
                                               double eps) {
  auto r = norm::ln_fwd_hip(x, delta, w, b, eps);
  return {std::get<1>(r), std::get<0>(r)};
}

// ------------------------------------------------------------------ attention from packed q|k|v
// [B, T, (H + 2·Hkv)·D] in, [B, T, H·D] out; the backward writes the packed gradient directly.
// Python reference: ops/attention.py _FlashAttentionQKV.
struct AttnQKVFn : public torch::autograd::Function<AttnQKVFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& qkv, int64_t H, int64_t Hkv, bool causal, double scale,
                        const optional<Tensor>& cos, const optional<Tensor>& sin) {
    at::AutoDispatchBelowADInplaceOrView guard;
    auto [q, k, v] = split_qkv(qkv, H, Hkv);
    auto [o, lse] = attn::attn_fwd_hip(q, k, v, causal, scale, cos, sin);
    const bool rope = cos.has_value();
    // sequences past two 128-query blocks get the pre-pass (attn.hip: fd off): offer δ to the
    // consumer of the output (adelta above)
    if (adelta::enabled() && q.size(3) == 64 && qkv.size(1) / 128 > 2 && qkv.size(1) % 128 == 0)
      adelta::want(o, qkv.size(1), H);
    if (rope) ctx->save_for_backward({qkv, o, lse, *cos, *sin});
    else ctx->save_for_backward({qkv, o, lse});
    ctx->saved_data["H"] = H;
    ctx->saved_data["Hkv"] = Hkv;
    ctx->saved_data["causal"] = causal;
    ctx->saved_data["scale"] = scale;
    return o.transpose(1, 2).reshape({qkv.size(0), qkv.size(1), -1});  // o is stored [B, T, H, D]: a view
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const Tensor &qkv = saved[0], &o = saved[1], &lse = saved[2];
    const bool rope = saved.size() > 3;
    const Tensor delta = adelta::enabled() ? adelta::take(o, grads[0]) : Tensor();
    const Tensor dqkv = attn_bwd_core(grads[0], qkv, o, lse, ctx->saved_data["H"].toInt(), ctx->saved_data["Hkv"].toInt(),
                                      ctx->saved_data["causal"].toBool(), ctx->saved_data["scale"].toDouble(),
                                      rope ? optional<Tensor>(saved[3]) : c10::nullopt,
                                      rope ? optional<Tensor>(saved[4]) : c10::nullopt, delta);
    return {dqkv, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

Tensor attn_qkv_ag(const Tensor& qkv, int64_t H, int64_t Hkv, bool causal, double scale, const optional<Tensor>& cos,
                   const optional<Tensor>& sin) {
  return AttnQKVFn::apply(qkv, H, Hkv, causal, scale, cos, sin);
}

Tensor attn_qkv_noag(const Tensor& qkv, int64_t H, int64_t Hkv, bool causal, double scale, const optional<Tensor>& cos,
                     const optional<Tensor>& sin) {
  auto [q, k, v] = split_qkv(qkv, H, Hkv);
  auto [o, lse] = attn::attn_fwd_hip(q, k, v, causal, scale, cos, sin);
  return o.transpose(1, 2).reshape({qkv.size(0), qkv.size(1), -1});
}

}  // namespace ag
}  // namespace nbd

// Autograd key: the nodes above.  CUDA key (reached under torch.inference_mode / no autograd):
// the forward alone.
TORCH_LIBRARY_IMPL(nbd, Autograd, m) {
  m.impl("linear_ag", &nbd::ag::linear_ag);
  m.impl("mlp_gelu_ag", &nbd::ag::mlp_gelu_ag);
  m.impl("mlp_swiglu_ag", &nbd::ag::mlp_swiglu_ag);
  m.impl("rms_norm_ag", &nbd::ag::rms_norm_ag);
  m.impl("add_rms_norm_ag", &nbd::ag::add_rms_norm_ag);
  m.impl("layer_norm_ag", &nbd::ag::layer_norm_ag);
  m.impl("add_layer_norm_ag", &nbd::ag::add_layer_norm_ag);
  m.impl("embed_rms_norm_ag", &nbd::ag::embed_rms_norm_ag);
  m.impl("tokpos_layer_norm_ag", &nbd::ag::tokpos_layer_norm_ag);
  m.impl("attn_qkv_ag", &nbd::ag::attn_qkv_ag);
}

TORCH_LIBRARY_IMPL(nbd, CUDA, m) {
  m.impl("rms_norm_ag", &nbd::ag::rms_norm_noag);
  m.impl("add_rms_norm_ag", &nbd::ag::add_rms_norm_noag);
  m.impl("layer_norm_ag", &nbd::ag::layer_norm_noag);
  m.impl("add_layer_norm_ag", &nbd::ag::add_layer_norm_noag);
  m.impl("embed_rms_norm_ag", &nbd::ag::embed_rms_norm_noag);
  m.impl("tokpos_layer_norm_ag", &nbd::ag::tokpos_layer_norm_noag);
  m.impl("attn_qkv_ag", &nbd::ag::attn_qkv_noag);
  m.impl("linear_ag", &nbd::ag::linear_noag);
  m.impl("mlp_gelu_ag", &nbd::ag::mlp_gelu_noag);
  m.impl("mlp_swiglu_ag", &nbd::ag::mlp_swiglu_noag);
}
