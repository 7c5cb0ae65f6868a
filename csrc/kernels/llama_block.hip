// llama_block.hip — the fused Llama decoder block node and its per-block / stack HIP graphs.
//
// One autograd node for a whole pre-norm decoder block of the Llama family:
//   qkv = h·W_qkvᵀ (+b) → causal GQA attention with RoPE → y = a·W_oᵀ (+b)
//   x1 = x + y, h1 = rms(x1)·γ_post → m = down(silu(g)·u), [g|u] = h1·W_guᵀ
//   x2 = x1 + m, h2 = rms(x2)·γ_next                                  → returns (x2, h2)
// The same kernels, in the same order, as the per-op nodes of autograd.hip (Linear, attention,
// add+RMSNorm, SwiGLU MLP: bit-identical results — the backward IS theirs, ag_common.h *_bwd_core),
// but one Python call and one autograd node per block instead of six and five — an eager SmolLM2
// step is host-bound (docs/FINDINGS.md §15, §27).  Weight gradients go to their bucket slices
// (graddst) exactly as in the per-op nodes.
#include <ATen/hip/HIPGraph.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/GradMode.h>

#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <sstream>
#include <unordered_map>
#include <unordered_set>

#include "ag_common.h"

namespace nbd {
namespace ag {

// what the forward saves for the backward, in save_for_backward order
enum Sv { SV_H2, SV_W_QKV, SV_B_QKV, SV_QKV, SV_O, SV_LSE, SV_W_O, SV_B_O, SV_X1, SV_W_POST, SV_RSTD1, SV_H1F, SV_W_GU,
          SV_W_DOWN, SV_PRE, SV_ACT, SV_X_OUT, SV_W_NEXT, SV_RSTD2, SV_COS, SV_SIN, SV_N };
// the slots holding the call's weights / RoPE tables; the first 8 are the node's gradient
// targets, returned as node outputs 2..9 in this order
constexpr int kBlockWeightSlots[] = {SV_W_QKV, SV_B_QKV, SV_W_O,    SV_B_O, SV_W_POST,
                                     SV_W_GU,  SV_W_DOWN, SV_W_NEXT, SV_COS, SV_SIN};

// One call of the block: tensors by reference, the plans in wire form (ag_common.h), the scalars.
// Members in the order of the op's arguments (nbd_ops.cpp llama_block_ag).
struct BlockCall {
  const Tensor &x, &h, &w_qkv;
  const optional<Tensor>& b_qkv;
  const Tensor& w_o;
  const optional<Tensor>& b_o;
  const Tensor &w_post, &w_gu, &w_down, &w_next;
  at::IntArrayRef plan_qkv, plan_o, plan_mlp;
  int64_t H, Hkv;
  double scale, eps;
  const optional<Tensor>&cos, &sin;
  // the weights / RoPE tables in kBlockWeightSlots order (nullptr: absent)
  std::array<const Tensor*, 10> weights() const {
    auto p = [](const optional<Tensor>& t) { return t ? &*t : nullptr; };
    return {&w_qkv, p(b_qkv), &w_o, p(b_o), &w_post, &w_gu, &w_down, &w_next, p(cos), p(sin)};
  }
  BlockCall with_inputs(const Tensor& x_, const Tensor& h_) const {
    return {x_, h_, w_qkv, b_qkv, w_o, b_o, w_post, w_gu, w_down, w_next, plan_qkv, plan_o, plan_mlp, H, Hkv, scale, eps,
            cos, sin};
  }
  void put_weights(std::vector<Tensor>& saved) const {
    const auto ws = weights();
    for (size_t i = 0; i < ws.size(); ++i) saved[kBlockWeightSlots[i]] = ws[i] != nullptr ? *ws[i] : Tensor();
  }
};

// forward of the block; `save` (autograd) receives what the backward needs
static std::tuple<Tensor, Tensor> llama_block_fwd(const BlockCall& c, std::vector<Tensor>* save) {
  const LinearPlan plan_qkv = LinearPlan::parse(c.plan_qkv), plan_o = LinearPlan::parse(c.plan_o);
  const MLPPlan plan_mlp = MLPPlan::parse(c.plan_mlp);
  const int64_t B = c.h.size(0), T = c.h.size(1), C = c.h.size(2);
  const Tensor h2 = bf16c(c.h).view({-1, C});
  const Tensor qkv = linear_forward(h2, c.w_qkv, c.b_qkv, plan_qkv).view({B, T, -1});
  auto [q, k, v] = split_qkv(qkv, c.H, c.Hkv);
  auto [o, lse] = attn::attn_fwd_hip(q, k, v, true, c.scale, c.cos, c.sin);
  const Tensor a2 = o.transpose(1, 2).reshape({B * T, -1});  // o is stored [B, T, H, D]: a view
  const Tensor y = linear_forward(a2, c.w_o, c.b_o, plan_o).view({B, T, C});
  auto [h1, x1, rstd1] = norm::rms_fwd_hip(bf16c(c.x), y, c.w_post, c.eps);
  const Tensor h1f = h1.view({-1, C});
  auto [act, pre] = run(h1f, c.w_gu, false, false, plan_mlp.up, EPI_SWIGLU);
  const Tensor m = run(act, c.w_down, false, false, plan_mlp.down).first.view({B, T, C});
  auto [h_out, x_out, rstd2] = norm::rms_fwd_hip(x1, m, c.w_next, c.eps);
  if (save != nullptr) {
    std::vector<Tensor>& s = *save;
    s.assign(SV_N, Tensor());
    c.put_weights(s);
    s[SV_H2] = h2, s[SV_QKV] = qkv, s[SV_O] = o, s[SV_LSE] = lse, s[SV_X1] = x1, s[SV_RSTD1] = rstd1;
    s[SV_H1F] = h1f, s[SV_PRE] = pre, s[SV_ACT] = act, s[SV_X_OUT] = x_out, s[SV_RSTD2] = rstd2;
  }
  return {x_out, h_out};
}

// ---- one HIP graph per decoder block for the EAGER step (opt-in: NBD_BLOCK_GRAPHS=1 or
// torch.ops.nbd.llama_block_graphs(1)).  The block's forward — seven kernels plus allocations,
// ≈70 µs of issuing-thread time on SmolLM2 (docs/FINDINGS.md §27) — is captured once per
// (block, shape) after two eager calls and then replayed: one graph launch instead of seven
// kernel launches.  The graph writes its activations into static memory (its private pool), so:
//  * the block's inputs are copied into static buffers, except when they ARE another block
//    graph's outputs (the residual stream between consecutive graphed blocks needs no copy);
//  * the static memory may be replayed into only once the previous pass's autograd node has let
//    go of it: a token among the node's saved tensors clears `armed` when backward releases the
//    saved tensors (or the node dies).  A forward while the block is armed (a second forward
//    before backward, retain_graph) runs eagerly, as does any call whose weights, RoPE tables or
//    aliased input moved, or that comes inside another capture (graphs.GraphedStep);
//  * the returned tensors alias that memory: they hold this pass's values until the block's next
//    replay (a caller keeping block outputs across steps must clone them);
//  * each (block, shape) keeps its activations allocated between steps: at most 4 shapes per block
//    are graphed, further sequence lengths run eagerly.
// The backward of a graph-forwarded block is captured too (its first graphed backward) when every
// weight gradient goes to a DDP bucket slice (graddst.h): the claims made during the capture are
// recorded, and a replay first checks that each parameter's destination (and whether it
// accumulates, no_sync) is still the captured one — peek(), no side effects — then claims them
// (the pass bookkeeping) and hands the slices back as the weight gradients.  One backward graph per
// accumulate pattern; the deferred reductions of the capture are recorded and queued after each
// replay, so they join the backward's single flush.  Without bucket slices
// (plain training) the backward stays eager: a graph's weight gradients would be static memory
// that AccumulateGrad keeps as .grad.
// Same kernels, same order: bit-identical to the eager block (tests/test_gpu_block_graphs.py).
namespace bg {
using Key = std::tuple<const void*, int64_t, int64_t, int64_t>;  // (W_qkv, B, T, device)

// What a captured forward is valid for: the slot key, the addresses of the weights / RoPE tables,
// and their shapes with the block's scalars and plans.
struct Ident {
  Key key{};
  std::vector<const void*> ptrs;
  std::vector<int64_t> sig;
  Ident() = default;
  explicit Ident(const BlockCall& c)
      : key{c.w_qkv.data_ptr(), c.h.size(0), c.h.size(1), c.h.get_device()},
        sig{c.H, c.Hkv, (int64_t)(c.scale * 1e9), (int64_t)(c.eps * 1e12), (int64_t)c.x.scalar_type()} {
    for (const Tensor* t : c.weights()) {
      ptrs.push_back(t != nullptr ? t->data_ptr() : nullptr);
      if (t != nullptr) sig.insert(sig.end(), t->sizes().begin(), t->sizes().end());
      sig.push_back(-1);
    }
    for (at::IntArrayRef p : {c.plan_qkv, c.plan_o, c.plan_mlp}) sig.insert(sig.end(), p.begin(), p.end());
  }
  bool operator==(const Ident& o) const { return key == o.key && ptrs == o.ptrs && sig == o.sig; }
  bool operator!=(const Ident& o) const { return !(*this == o); }
};
// One captured block forward: a graph of its own (Graph) or a member of a stack graph (Stack)
struct Captured {
  Ident ident;
  std::vector<Tensor> saved;  // llama_block_fwd's saved list (static; weight slots empty)
  Tensor x_out, h_out;
};

struct Bwd {
  std::unique_ptr<at::cuda::CUDAGraph> g;
  Tensor dx_in, dh_in;                    // static inputs (the incoming gradients)
  bool dx_alias = false, dh_alias = false;  // ...that are another block graph's outputs
  Tensor g1, dh;                          // static outputs: the gradients of x and h
  std::vector<graddst::ClaimRecord> claims;  // in capture order
  std::vector<int> pidx;                  // the saved parameter each claim was made for (by position:
                                          // native()'s cast weights are new tensors every step)
  std::vector<int> slot;                  // the node output each claim's slice is returned as
  std::vector<Tensor> warm_refs;
  std::shared_ptr<void> deferred;          // its deferred reductions (defer::record_begin)
};
struct Graph : Captured {
  std::unique_ptr<at::cuda::CUDAGraph> g;
  Tensor x_in, h_in;                   // static inputs
  bool x_alias = false, h_alias = false;  // ...that are another block graph's outputs
  std::vector<Tensor> warm_refs;       // storages the captured GEMM warm-ups read
  std::atomic<bool> armed{false};
  int64_t id = 0;
  std::map<int, std::shared_ptr<Bwd>> bwd;  // key: accumulate mask | need bits
  int bwd_captures = 0;
  bool bwd_off = false;
  // the static output at `p` (forward or backward), or nullptr
  const Tensor* output_at(const void* p) const {
    if (x_out.defined() && x_out.data_ptr() == p) return &x_out;
    if (h_out.defined() && h_out.data_ptr() == p) return &h_out;
    for (const auto& kv : bwd) {
      if (kv.second->g1.defined() && kv.second->g1.data_ptr() == p) return &kv.second->g1;
      if (kv.second->dh.defined() && kv.second->dh.data_ptr() == p) return &kv.second->dh;
    }
    return nullptr;
  }
};
// A block call's arguments (BlockCall's owning copy), kept so that a stack capture can re-run it.
// variable_data(): the data only — a registry holding a cast weight's autograd history would
// keep that pass's AccumulateGrad nodes alive (the stream hazard of x_in below)
struct Args {
  static optional<Tensor> vd(const optional<Tensor>& t) { return t ? optional<Tensor>(t->variable_data()) : c10::nullopt; }
  Tensor w_qkv, w_o, w_post, w_gu, w_down, w_next;
  optional<Tensor> b_qkv, b_o, cos, sin;
  std::vector<int64_t> plan_qkv, plan_o, plan_mlp;
  int64_t H, Hkv;
  double scale, eps;
  explicit Args(const BlockCall& c)
      : w_qkv(c.w_qkv.variable_data()), w_o(c.w_o.variable_data()), w_post(c.w_post.variable_data()),
        w_gu(c.w_gu.variable_data()), w_down(c.w_down.variable_data()), w_next(c.w_next.variable_data()),
        b_qkv(vd(c.b_qkv)), b_o(vd(c.b_o)), cos(vd(c.cos)), sin(vd(c.sin)), plan_qkv(c.plan_qkv.vec()),
        plan_o(c.plan_o.vec()), plan_mlp(c.plan_mlp.vec()), H(c.H), Hkv(c.Hkv), scale(c.scale), eps(c.eps) {}
  BlockCall call(const Tensor& x, const Tensor& h) const {
    return {x, h, w_qkv, b_qkv, w_o, b_o, w_post, w_gu, w_down, w_next, plan_qkv, plan_o, plan_mlp, H, Hkv, scale, eps,
            cos, sin};
  }
};

// Stack graphs (mode 1): every graph launch costs the GPU ≈8.5 µs of its own
// (benchmarks/graph_chunks.py), so once a run of consecutive graphed blocks has replayed
// steadily — each block's input the previous block's static output — the whole run is captured
// as ONE graph, replayed at its first block's call; the following blocks' calls, arriving in the
// recorded order with the recorded weights and the stack's outputs as inputs, are served from it
// without a launch.  Any deviation drops the stack (back to per-block graphs).
std::atomic<uint64_t> g_cast_epoch{0};  // (ag_common.h)

struct Stack {
  std::unique_ptr<at::cuda::CUDAGraph> g;
  Tensor x_in, h_in;
  uint64_t cast_epoch = 0;     // g_cast_epoch at the head's replay
  std::vector<Captured> m;
  std::vector<Tensor> warm_refs;
  size_t next = 0;             // members served in the current pass
  std::atomic<int> held{0};    // served members whose autograd nodes still hold the memory
  Key head{};
  int64_t owner = 0;           // the head slot's owner (per-model reset)
};

struct Slot {
  int64_t owner = 0;  // the model that made the calls (LlamaModel's id; per-model reset)
  int eager = 0, captures = 0, misses = 0;
  bool off = false;
  std::shared_ptr<Graph> g;
  std::shared_ptr<Args> args;  // (stack capture)
  Key next_key{};              // the block that consumed this block's outputs last pass
  bool has_next = false;
  int steady = 0;              // consecutive per-block replays
  std::shared_ptr<Stack> stack;  // a stack headed by this block
  int stack_fail = 0;
};
std::mutex g_mu;
std::map<Key, Slot> g_slots;
std::unordered_map<const void*, std::weak_ptr<Graph>> g_outs;  // a graph's output address -> graph
std::unordered_map<int64_t, std::weak_ptr<Graph>> g_by_id;      // for the backward
int64_t g_next_id = 1;
std::atomic<int> g_mode{-1};                                    // -1: not read from the env yet
std::atomic<bool> g_suspended{false};                           // overrides per-model modes too
// forward captures, replays, eager calls; backward captures, replays, eager calls
std::atomic<int64_t> g_stat[10];  // + stack captures, stack replays, stack-served blocks, stacks dropped
std::weak_ptr<Stack> g_active;    // the stack serving the current pass
std::atomic<int> g_fail_bwd{0};   // fault injection (tests): fail this many backward captures

// 0 off, 1 forward graphs, 2 forward and backward graphs (NBD_BLOCK_GRAPHS)
int mode() {
  int m = g_mode.load(std::memory_order_relaxed);
  if (m < 0) {
    const char* e = std::getenv("NBD_BLOCK_GRAPHS");
    m = e != nullptr && (e[0] == '1' || e[0] == '2') ? e[0] - '0' : 0;
    g_mode.store(m, std::memory_order_relaxed);
  }
  return m;
}
bool enabled() { return mode() >= 1; }
bool stacks_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("NBD_BLOCK_STACKS");
    return e == nullptr || e[0] != '0';
  }();
  return on;
}
bool bwd_enabled() { return mode() >= 2; }

bool stream_capturing() {
  hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(), &s) != hipSuccess) return true;
  return s != hipStreamCaptureStatusNone;
}

// x is an output of a live block graph (so it stays put while that graph lives); under g_mu
bool is_graph_output(const Tensor& x) {
  if (!x.is_contiguous()) return false;
  auto it = g_outs.find(x.data_ptr());
  if (it == g_outs.end()) return false;
  auto gr = it->second.lock();
  if (!gr) return false;
  const Tensor* o = gr->output_at(x.data_ptr());
  return o != nullptr && o->numel() == x.numel() && o->scalar_type() == x.scalar_type();
}

// Capture `body` into `g` on a side stream ordered after the caller's stream, which then waits
// for it.  Returns the error ("" = captured).
// A stream of our own per device for the captures: a pool stream could be the one a process
// group's collectives run on (ProcessGroupNCCL takes its streams from the same pool).
c10::hip::HIPStreamMasqueradingAsCUDA capture_stream(c10::DeviceIndex dev) {
  static std::mutex mu;
  static std::unordered_map<int, hipStream_t> streams;
  std::lock_guard<std::mutex> lk(mu);
  hipStream_t& st = streams[dev];
  if (st == nullptr) {
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(c10::Device(c10::DeviceType::CUDA, dev));
    C10_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  }
  return c10::hip::getStreamFromExternalMasqueradingAsCUDA(st, dev);
}

std::string capture(at::cuda::CUDAGraph& g, const std::function<void()>& body) {
  auto cur = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  auto side = capture_stream(cur.device_index());
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  C10_HIP_CHECK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
  C10_HIP_CHECK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
  C10_HIP_CHECK(hipEventRecord(ev_in, cur.stream()));
  C10_HIP_CHECK(hipStreamWaitEvent(side.stream(), ev_in, 0));
  std::string err;
  {
    const c10::hip::HIPStreamGuardMasqueradingAsCUDA sg(side);
    g.capture_begin(at::cuda::graph_pool_handle(), hipStreamCaptureModeThreadLocal);
    try {
      body();
    } catch (const std::exception& e) {
      err = e.what();
    }
    try {
      g.capture_end();
    } catch (const std::exception& e) {
      if (err.empty()) err = e.what();
    }
  }
  C10_HIP_CHECK(hipEventRecord(ev_out, side.stream()));
  C10_HIP_CHECK(hipStreamWaitEvent(cur.stream(), ev_out, 0));
  C10_HIP_CHECK(hipEventDestroy(ev_in));
  C10_HIP_CHECK(hipEventDestroy(ev_out));
  return err;
}

Tensor token(const std::shared_ptr<Graph>& gr) {  // its release disarms the graph
  return release_token([w = std::weak_ptr<Graph>(gr)] {
    if (auto g = w.lock()) g->armed.store(false, std::memory_order_release);
  });
}
std::vector<std::shared_ptr<Stack>> g_dropped;  // dropped stacks: a replay may still be in flight

// under g_mu: the block whose static output `x` is now feeds block `key`
void link_pred(const Tensor& x, const Key& key) {
  auto it = g_outs.find(x.data_ptr());
  if (it == g_outs.end()) return;
  auto pg = it->second.lock();
  if (!pg) return;
  auto ps = g_slots.find(pg->ident.key);
  if (ps == g_slots.end()) return;
  ps->second.next_key = key;
  ps->second.has_next = true;
}

// under g_mu: stop serving `st` (its head slot captures no new stack after two failures)
void drop_stack(const std::shared_ptr<Stack>& st, const Key& head) {
  auto it = g_slots.find(head);
  if (it != g_slots.end() && it->second.stack == st) {
    it->second.stack.reset();
    ++it->second.stack_fail;
  }
  if (g_active.lock() == st) g_active.reset();
  g_dropped.push_back(st);
  if (g_dropped.size() > 8) g_dropped.erase(g_dropped.begin());
  ++g_stat[9];
}

Tensor stack_token(const std::shared_ptr<Stack>& st) {
  return release_token([w = std::weak_ptr<Stack>(st)] {
    if (auto s = w.lock()) s->held.fetch_sub(1, std::memory_order_acq_rel);
  });
}
}  // namespace bg

// Replay (or capture, then replay) the block's graph for this call; nullptr = run it eagerly.
static std::shared_ptr<bg::Graph> block_graph(const BlockCall& c, int64_t owner) {
  using namespace bg;
  if (stream_capturing()) return nullptr;  // inside a whole-step capture: the outer graph takes it
  const Tensor &x = c.x, &h = c.h;
  const Ident ident(c);
  const Key& key = ident.key;
  auto make_args = [&c] { return std::make_shared<Args>(c); };
  std::shared_ptr<Graph> gr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    Slot& s = g_slots[key];
    s.owner = owner;
    if (s.off) return nullptr;
    if (s.g && s.g->ident != ident) s.g.reset(), s.eager = 0, s.args.reset(), s.steady = 0;
    if (s.g) {
      Graph& G = *s.g;
      const bool inputs_ok = (!G.x_alias || x.data_ptr() == G.x_in.data_ptr()) &&
                             (!G.h_alias || h.data_ptr() == G.h_in.data_ptr());
      if (!inputs_ok) {  // the block before ran eagerly this time; twice in a row: capture anew
        if (++s.misses >= 2) s.g.reset(), s.eager = 0, s.misses = 0;
        ++g_stat[2];
        return nullptr;
      }
      if (G.armed.exchange(true, std::memory_order_acq_rel)) {  // last pass still holds the memory
        ++g_stat[2];
        return nullptr;
      }
      s.misses = 0;
      ++s.steady;
      if (!s.args) s.args = make_args();
      if (G.x_alias) link_pred(x, key);
      gr = s.g;
    } else if (++s.eager < 3) {
      ++g_stat[2];
      return nullptr;
    } else if (++s.captures > 4) {
      s.off = true;
      return nullptr;
    } else {
      // each (block, shape) keeps its activations: a model fed many sequence lengths (dynamic
      // padding) would grow without bound — at most kMaxShapes graphs per block, the rest eager
      // (and at most kMaxLive graphs in all: weights that move every step — per-forward casts
      // landing at new addresses — must not capture without bound either)
      constexpr int kMaxShapes = 4, kMaxLive = 512;
      int shapes = 0, live = 0;
      for (const auto& kv : g_slots) {
        live += kv.second.g != nullptr;
        shapes += std::get<0>(kv.first) == std::get<0>(key) && std::get<3>(kv.first) == std::get<3>(key) &&
                  kv.second.g != nullptr;
      }
      if (shapes >= kMaxShapes || live >= kMaxLive) {
        s.off = true;
        ++g_stat[2];
        return nullptr;
      }
    }
  }
  if (gr) {
    if (!gr->x_alias && x.data_ptr() != gr->x_in.data_ptr()) gr->x_in.copy_(x);
    if (!gr->h_alias && h.data_ptr() != gr->h_in.data_ptr()) gr->h_in.copy_(h);
    gr->g->replay();
    ++g_stat[1];
    return gr;
  }
  // capture on a side stream, then replay once on the caller's stream (capturing runs nothing)
  auto G = std::make_shared<Graph>();
  G->ident = ident;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    G->x_alias = is_graph_output(x);
    G->h_alias = is_graph_output(h);
  }
  // (variable_data: the graph must not hold the caller's autograd history — an aliased input is
  // the previous block's output, whose node would keep this pass's AccumulateGrad nodes alive)
  G->x_in = G->x_alias ? x.variable_data() : at::empty_like(x, at::MemoryFormat::Contiguous).copy_(x);
  G->h_in = G->h_alias ? h.variable_data() : at::empty_like(h, at::MemoryFormat::Contiguous).copy_(h);
  std::vector<Tensor> save;
  G->g = std::make_unique<at::cuda::CUDAGraph>();
  const std::string err = capture(*G->g, [&] {
    std::tie(G->x_out, G->h_out) = llama_block_fwd(c.with_inputs(G->x_in, G->h_in), &save);
  });
  G->warm_refs = castbuf::drop_kept(gemm::gemm_warm_take_refs());
  if (!err.empty()) {
    TORCH_WARN_ONCE("nbd: a decoder block's HIP graph capture failed (", err, "); the block runs eagerly");
    std::lock_guard<std::mutex> lk(g_mu);
    g_slots[key].off = true;
    return nullptr;
  }
  for (int i : kBlockWeightSlots) save[i] = Tensor();
  G->saved = std::move(save);
  G->armed.store(true, std::memory_order_release);
  G->g->replay();
  ++g_stat[0];
  ++g_stat[1];
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto it = g_outs.begin(); it != g_outs.end();) it = it->second.expired() ? g_outs.erase(it) : std::next(it);
  for (auto it = g_by_id.begin(); it != g_by_id.end();) it = it->second.expired() ? g_by_id.erase(it) : std::next(it);
  g_outs[G->x_out.data_ptr()] = G;
  g_outs[G->h_out.data_ptr()] = G;
  G->id = g_next_id++;
  g_by_id[G->id] = G;
  Slot& s = g_slots[key];
  s.g = G;
  s.misses = 0;
  s.steady = 0;
  s.args = make_args();
  if (G->x_alias) link_pred(x, key);
  return G;
}

// A stack graph for this call (see bg::Stack): the head's call replays it, the following blocks'
// calls are served from it.  {nullptr, 0} = not served (per-block path).
static std::pair<std::shared_ptr<bg::Stack>, size_t> stack_serve(const BlockCall& c) {
  using namespace bg;
  if (stream_capturing()) return {nullptr, 0};
  const Tensor &x = c.x, &h = c.h;
  const Ident ident(c);
  const Key& key = ident.key;
  std::lock_guard<std::mutex> lk(g_mu);
  // 1. the next member of the stack serving this pass
  if (auto st = g_active.lock()) {
    if (st->next > 0 && st->next < st->m.size()) {
      const Captured& prev = st->m[st->next - 1];
      if (st->m[st->next].ident == ident && x.data_ptr() == prev.x_out.data_ptr() &&
          h.data_ptr() == prev.h_out.data_ptr()) {
        // the replay already ran this member on the weights as they were at the head's call
        TORCH_CHECK(g_cast_epoch.load(std::memory_order_acquire) == st->cast_epoch,
                    "nbd: a decoder block's weights were cast after its stack graph had replayed (the block would "
                    "read the previous values): cast every layer before the first block (models/llama.py "
                    "_forward_cast), or turn block graphs off (NBD_BLOCK_GRAPHS=0)");
        st->held.fetch_add(1, std::memory_order_acq_rel);
        ++g_stat[8];
        return {st, st->next++};
      }
      drop_stack(st, st->head);  // the pass left the recorded order
    }
  }
  // 2. the head of a stack
  auto it = g_slots.find(key);
  if (it == g_slots.end()) return {nullptr, 0};
  Slot& s = it->second;
  if (!s.stack) {
    // 3. capture one: a steadily replaying chain of >= 2 graphed blocks starting here
    if (!s.g || s.g->x_alias || s.g->ident != ident) return {nullptr, 0};
    if (s.stack_fail >= 2 || s.steady < 3 || !s.args) return {nullptr, 0};
    std::vector<Key> chain{key};
    for (Key k = key; chain.size() < 256;) {
      const Slot& cs = g_slots[k];
      if (!cs.has_next) break;
      auto nit = g_slots.find(cs.next_key);
      if (nit == g_slots.end() || !nit->second.g || !nit->second.args || nit->second.steady < 3 ||
          !nit->second.g->x_alias || std::find(chain.begin(), chain.end(), cs.next_key) != chain.end())
        break;
      chain.push_back(cs.next_key);
      k = cs.next_key;
    }
    if (chain.size() < 2) return {nullptr, 0};
    auto st = std::make_shared<Stack>();
    st->head = key;
    st->owner = s.owner;
    st->x_in = at::empty_like(x, at::MemoryFormat::Contiguous);
    st->h_in = at::empty_like(h, at::MemoryFormat::Contiguous);
    st->m.resize(chain.size());
    std::vector<std::shared_ptr<Args>> args;
    for (size_t i = 0; i < chain.size(); ++i) {
      const Slot& cs = g_slots[chain[i]];
      st->m[i].ident = cs.g->ident;
      args.push_back(cs.args);
    }
    st->g = std::make_unique<at::cuda::CUDAGraph>();
    const std::string err = capture(*st->g, [&] {
      Tensor cx = st->x_in, ch = st->h_in;
      for (size_t i = 0; i < args.size(); ++i) {
        std::vector<Tensor> save;
        std::tie(st->m[i].x_out, st->m[i].h_out) = llama_block_fwd(args[i]->call(cx, ch), &save);
        for (int j : kBlockWeightSlots) save[j] = Tensor();
        st->m[i].saved = std::move(save);
        cx = st->m[i].x_out;
        ch = st->m[i].h_out;
      }
    });
    st->warm_refs = castbuf::drop_kept(gemm::gemm_warm_take_refs());
    if (!err.empty()) {
      ++s.stack_fail;
      TORCH_WARN_ONCE("nbd: a stack of decoder-block graphs failed to capture (", err, "); per-block graphs stay");
      return {nullptr, 0};
    }
    ++g_stat[6];
    s.stack = st;
    // the members' own graphs are not replayed while the stack serves: free their static memory
    // (a block the stack stops serving captures its own graph again after two eager calls)
    for (const Key& k : chain) {
      Slot& ms = g_slots[k];
      ms.g.reset();
      ms.eager = 0;
      ms.steady = 0;
    }
  }
  Stack& st = *s.stack;
  if (st.m[0].ident != ident) {
    drop_stack(s.stack, key);
    return {nullptr, 0};
  }
  if (st.held.load(std::memory_order_acquire) != 0) return {nullptr, 0};  // the last pass still holds it
  if (st.x_in.data_ptr() != x.data_ptr()) st.x_in.copy_(x);
  if (st.h_in.data_ptr() != h.data_ptr()) st.h_in.copy_(h);
  st.g->replay();
  st.next = 1;
  st.cast_epoch = g_cast_epoch.load(std::memory_order_acquire);
  st.held.store(1, std::memory_order_release);
  g_active = s.stack;
  ++g_stat[7];
  return {s.stack, 0};
}

// What the backward needs beside the saved tensors (LlamaBlockFn::forward's "m" and "s").
struct BlockBwdArgs {
  LinearPlan plan_qkv, plan_o;
  MLPPlan plan_mlp;
  int64_t H, Hkv;
  double scale;
  std::vector<int64_t> shape;  // [B, T, C]
  bool need_x, need_h;
};

// The block's backward into `out` (the node's 20 outputs).
static void block_bwd(const std::vector<Tensor>& sv, const BlockBwdArgs& a, const Tensor& dx_out, const Tensor& dh_out,
                      variable_list& out) {
  const Tensor &h2 = sv[SV_H2], &w_qkv = sv[SV_W_QKV], &b_qkv = sv[SV_B_QKV], &qkv = sv[SV_QKV], &o = sv[SV_O],
               &lse = sv[SV_LSE], &w_o = sv[SV_W_O], &b_o = sv[SV_B_O], &x1 = sv[SV_X1], &w_post = sv[SV_W_POST],
               &rstd1 = sv[SV_RSTD1], &h1f = sv[SV_H1F], &w_gu = sv[SV_W_GU], &w_down = sv[SV_W_DOWN],
               &pre = sv[SV_PRE], &act = sv[SV_ACT], &x_out = sv[SV_X_OUT], &w_next = sv[SV_W_NEXT],
               &rstd2 = sv[SV_RSTD2];
  auto table = [&](int i) { return sv[i].defined() ? optional<Tensor>(sv[i]) : c10::nullopt; };
  const std::vector<int64_t>& shape = a.shape;
  const int64_t C = shape[2];
  // x2 = x1 + m, h2 = rms(x2)·γ_next
  Tensor g2, dw_next;
  {
    const ht::Scope hs(ht::RMS_NEXT);
    if (dh_out.defined()) std::tie(g2, dw_next) = rms_bwd_core(x_out, dh_out, dx_out, w_next, rstd2);
    else g2 = dx_out;
  }
  if (!g2.defined()) return;  // neither output reached the loss
  // m = down(swiglu(h1·W_guᵀ))
  Tensor dh1, dw_gu, dw_down;
  {
    const ht::Scope hs(ht::SWIGLU);
    const MLPGrads g = mlp_bwd_core(EPI_DSWIGLU, bf16c(g2).view({-1, C}), h1f, w_gu, w_down, pre, act, a.plan_mlp, true);
    dh1 = g.dx, dw_gu = g.dw_up, dw_down = g.dw_down;
  }
  // x1 = x + y, h1 = rms(x1)·γ_post
  Tensor g1, dw_post;
  {
    const ht::Scope hs(ht::RMS_POST);
    std::tie(g1, dw_post) = rms_bwd_core(x1, dh1.view(shape), g2, w_post, rstd1);
  }
  // y = a·W_oᵀ (+b)
  Tensor da, dw_o, db_o;
  {
    const ht::Scope hs(ht::LIN_O);
    const Tensor a2 = o.transpose(1, 2).reshape({h2.size(0), -1});
    std::tie(da, dw_o, db_o) = linear_bwd_core(bf16c(g1).view({-1, C}), a2, w_o, b_o, a.plan_o, true,
                                               w_o.requires_grad(), b_o.defined() && b_o.requires_grad());
  }
  Tensor dqkv;
  {
    const ht::Scope hs(ht::ATTN);
    dqkv = attn_bwd_core(da, qkv, o, lse, a.H, a.Hkv, true, a.scale, table(SV_COS), table(SV_SIN));
  }
  Tensor dh, dw_qkv, db_qkv;
  {
    const ht::Scope hs(ht::LIN_QKV);
    std::tie(dh, dw_qkv, db_qkv) = linear_bwd_core(dqkv.view({h2.size(0), -1}), h2, w_qkv, b_qkv, a.plan_qkv, a.need_h,
                                                   w_qkv.requires_grad(), b_qkv.defined() && b_qkv.requires_grad());
  }
  out[0] = a.need_x ? g1 : Tensor();
  out[1] = dh.defined() ? dh.view(shape) : dh;
  out[2] = dw_qkv, out[3] = db_qkv, out[4] = dw_o, out[5] = db_o;  // (kBlockWeightSlots order)
  out[6] = dw_post, out[7] = dw_gu, out[8] = dw_down, out[9] = dw_next;
}

// The block's backward as a HIP graph (see namespace bg); false = run it eagerly.
static bool block_bwd_graph(bg::Graph& G, const std::vector<Tensor>& sv, const BlockBwdArgs& a, const Tensor& dx_out,
                            const Tensor& dh_out, variable_list& out) {
  using namespace bg;
  const std::vector<int64_t>& shape = a.shape;
  const bool need_x = a.need_x, need_h = a.need_h;
  if (G.bwd_off || !dh_out.defined() || bg::stream_capturing()) return false;
  for (const Tensor* t : {&dx_out, &dh_out})
    if (t->defined() && (!t->is_contiguous() || t->scalar_type() != at::kBFloat16 ||
                         t->numel() != shape[0] * shape[1] * shape[2]))
      return false;
  const bool has_dx = dx_out.defined();  // (the last block's residual output reaches no loss)
  // the parameters whose gradients this node returns: every one needs a bucket slice
  constexpr int kSlot[] = {2, 3, 4, 5, 6, 7, 8, 9};  // node outputs of the first 8 kBlockWeightSlots
  const Tensor* ps[8];
  for (int i = 0; i < 8; ++i) ps[i] = &sv[kBlockWeightSlots[i]];
  Tensor dst[8];
  bool acc[8] = {};
  int mask = 0, wants = 0;
  for (int i = 0; i < 8; ++i) {
    if (!ps[i]->defined() || !ps[i]->requires_grad()) continue;
    dst[i] = graddst::peek(*ps[i], acc[i]);
    if (!dst[i].defined()) return false;
    mask |= (int)acc[i] << i;
    wants |= 1 << i;
  }
  // one graph per (accumulate pattern, which parameters want gradients, which inputs do)
  const int key = mask | (int)need_x << 8 | (int)need_h << 9 | (int)has_dx << 10 | wants << 11;
  auto param_index = [&](const c10::TensorImpl* impl) {
    for (int i = 0; i < 8; ++i)
      if (ps[i]->defined() && ps[i]->unsafeGetTensorImpl() == impl) return i;
    return -1;
  };
  std::shared_ptr<Bwd> found;  // (G.bwd under g_mu: is_graph_output reads it from the forward)
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = G.bwd.find(key);
    if (it != G.bwd.end()) found = it->second;
  }
  if (found) {
    Bwd& B = *found;
    bool ok = (!has_dx || !B.dx_alias || dx_out.data_ptr() == B.dx_in.data_ptr()) &&
              (!B.dh_alias || dh_out.data_ptr() == B.dh_in.data_ptr());
    for (size_t k = 0; k < B.claims.size(); ++k) {
      const auto& c = B.claims[k];
      const int i = B.pidx[k];
      ok = ok && i >= 0 && dst[i].defined() && dst[i].data_ptr() == c.dst && acc[i] == c.acc;
    }
    if (!ok) {
      std::lock_guard<std::mutex> lk(g_mu);
      G.bwd.erase(key);  // destinations moved: capture anew next time
      return false;
    }
    if (has_dx && !B.dx_alias && dx_out.data_ptr() != B.dx_in.data_ptr()) B.dx_in.copy_(dx_out);
    if (!B.dh_alias && dh_out.data_ptr() != B.dh_in.data_ptr()) B.dh_in.copy_(dh_out);
    for (size_t k = 0; k < B.claims.size(); ++k) {  // the pass bookkeeping of the captured claims
      const auto& c = B.claims[k];
      const int i = B.pidx[k];
      bool a = false;
      const Tensor d = graddst::claim(*ps[i], a);
      TORCH_CHECK(d.defined() && d.data_ptr() == c.dst && a == c.acc, "nbd: block graph claim changed");
    }
    B.g->replay();
    defer::replay(B.deferred, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream());
    out[0] = need_x ? at::alias(B.g1) : Tensor();
    out[1] = need_h ? at::alias(B.dh) : Tensor();
    for (size_t k = 0; k < B.claims.size(); ++k) {
      const int i = B.pidx[k];
      if (B.slot[k] >= 0) out[B.slot[k]] = graddst::hand_back(*ps[i], dst[i], B.claims[k].acc);
    }
    return true;
  }
  if (G.bwd_captures >= 4) {
    G.bwd_off = true;
    return false;
  }
  ++G.bwd_captures;
  defer::flush();  // reductions queued by eager nodes before this one stay out of the graph
  auto B = std::make_shared<Bwd>();
  {
    std::lock_guard<std::mutex> lk(g_mu);
    B->dx_alias = has_dx && is_graph_output(dx_out);
    B->dh_alias = is_graph_output(dh_out);
  }
  if (has_dx)
    B->dx_in = B->dx_alias ? dx_out.variable_data() : at::empty_like(dx_out, at::MemoryFormat::Contiguous).copy_(dx_out);
  B->dh_in = B->dh_alias ? dh_out.variable_data() : at::empty_like(dh_out, at::MemoryFormat::Contiguous).copy_(dh_out);
  B->g = std::make_unique<at::cuda::CUDAGraph>();
  variable_list o(20);
  std::string err;
  {
    // (RAII: an exception must not leave this thread recording claims or deferred reductions)
    struct Recording {
      explicit Recording(std::vector<graddst::ClaimRecord>* log) {
        graddst::record_claims(log);
        defer::record_begin();  // this node's deferred reductions: queued after each replay
      }
      ~Recording() {
        if (!ended) defer::record_end();
        graddst::record_claims(nullptr);
      }
      std::shared_ptr<void> end() {
        ended = true;
        return defer::record_end();
      }
      bool ended = false;
    } rec(&B->claims);
    err = capture(*B->g, [&] {
      block_bwd(sv, a, B->dx_in, B->dh_in, o);
      int f = g_fail_bwd.load();
      while (f > 0 && !g_fail_bwd.compare_exchange_weak(f, f - 1)) {
      }
      if (f > 0) throw std::runtime_error("injected backward capture failure");
    });
    B->deferred = rec.end();
  }
  B->warm_refs = castbuf::drop_kept(gemm::gemm_warm_take_refs());
  if (!err.empty()) {
    // nothing captured ran: undo the pass bookkeeping of the claims made while capturing, so the
    // eager backward the caller runs next claims the same bucket slices (a training step must not
    // be lost to a performance feature)
    G.bwd_off = true;
    graddst::release(B->claims);
    TORCH_WARN_ONCE("nbd: a decoder block's backward graph capture failed (", err, "); the block's backward runs eagerly");
    return false;
  }
  // every weight gradient must be its claimed slice (else it would be static graph memory)
  B->pidx.resize(B->claims.size());
  for (size_t k = 0; k < B->claims.size(); ++k) B->pidx[k] = param_index(B->claims[k].param);
  B->slot.assign(B->claims.size(), -1);
  bool valid = true;
  for (int i = 0; i < 8; ++i) {
    const Tensor& g = o[kSlot[i]];
    if (!g.defined()) continue;
    int found = -1;
    for (size_t k = 0; k < B->claims.size(); ++k)
      if (B->claims[k].dst == g.data_ptr() && B->claims[k].param == ps[i]->unsafeGetTensorImpl()) found = (int)k;
    if (found < 0) valid = false;
    else B->slot[found] = kSlot[i];
  }
  B->g->replay();
  defer::replay(B->deferred, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream());
  ++g_stat[3];
  if (!valid) {  // this call: private copies of the non-slice gradients; later calls: eager
    G.bwd_off = true;
    for (int i = 0; i < 8; ++i) {
      Tensor& g = o[kSlot[i]];
      bool claimed = false;
      for (const auto& c : B->claims) claimed = claimed || (g.defined() && c.dst == g.data_ptr());
      if (g.defined() && !claimed) g = g.clone();
    }
    out = o;
    for (int k : {0, 1})
      if (out[k].defined()) out[k] = out[k].clone();
    return true;
  }
  B->g1 = o[0].defined() ? o[0].view(shape) : Tensor();
  B->dh = o[1].defined() ? o[1].view(shape) : Tensor();
  out = o;
  out[0] = B->g1.defined() ? at::alias(B->g1) : Tensor();
  out[1] = B->dh.defined() ? at::alias(B->dh) : Tensor();
  std::lock_guard<std::mutex> lk(g_mu);
  G.bwd[key] = B;
  auto self = g_by_id.count(G.id) ? g_by_id[G.id] : std::weak_ptr<Graph>();
  if (B->g1.defined()) g_outs[B->g1.data_ptr()] = self;
  if (B->dh.defined()) g_outs[B->dh.data_ptr()] = self;
  return true;
}

struct LlamaBlockFn : public torch::autograd::Function<LlamaBlockFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const Tensor& h, const Tensor& w_qkv,
                               const optional<Tensor>& b_qkv, const Tensor& w_o, const optional<Tensor>& b_o,
                               const Tensor& w_post, const Tensor& w_gu, const Tensor& w_down, const Tensor& w_next,
                               at::IntArrayRef plan_qkv, at::IntArrayRef plan_o, at::IntArrayRef plan_mlp, int64_t H,
                               int64_t Hkv, double scale, double eps, const optional<Tensor>& cos,
                               const optional<Tensor>& sin, int64_t graph_mode) {
    const ht::Scope hs(ht::FWD);
    at::AutoDispatchBelowADInplaceOrView guard;
    ctx->set_materialize_grads(false);
    const int64_t owner = graph_mode >> 8;  // (llama_block_ag packs the model id above the mode)
    graph_mode &= 0xff;
    const BlockCall c{x, h, w_qkv, b_qkv, w_o, b_o, w_post, w_gu, w_down, w_next, plan_qkv, plan_o, plan_mlp, H, Hkv,
                      scale, eps, cos, sin};
    TORCH_CHECK(plan_qkv.size() == 10 && plan_o.size() == 10 && plan_mlp.size() == 20,
                "nbd llama_block: plans are int[10], int[10], int[20]");  // (a replayed graph parses none)
    std::vector<Tensor> save;
    Tensor x_out, h_out;
    std::shared_ptr<bg::Graph> gr;
    std::pair<std::shared_ptr<bg::Stack>, size_t> sh{nullptr, 0};
    if (graph_mode == 1 && bg::stacks_enabled()) sh = stack_serve(c);
    if (!sh.first && graph_mode >= 1) gr = block_graph(c, owner);
    if (sh.first || gr) {  // served from a graph: its static saved list with this call's weights
      const bg::Captured& cap = sh.first ? sh.first->m[sh.second] : *gr;
      save = cap.saved;
      c.put_weights(save);
      save.push_back(sh.first ? bg::stack_token(sh.first) : bg::token(gr));
      x_out = at::alias(cap.x_out);
      h_out = at::alias(cap.h_out);
      if (gr && graph_mode >= 2) ctx->saved_data["bg"] = gr->id;
    } else {
      std::tie(x_out, h_out) = llama_block_fwd(c, &save);
    }
    ctx->save_for_backward(save);
    // [H, Hkv, need x, need h, B, T, C, plan_qkv (10), plan_o (10), plan_mlp (20)] (one IValue)
    std::vector<int64_t> meta{H, Hkv, x.requires_grad(), h.requires_grad(), h.size(0), h.size(1), h.size(2)};
    meta.reserve(meta.size() + plan_qkv.size() + plan_o.size() + plan_mlp.size());
    for (at::IntArrayRef p : {plan_qkv, plan_o, plan_mlp}) meta.insert(meta.end(), p.begin(), p.end());
    ctx->saved_data["m"] = std::move(meta);
    ctx->saved_data["s"] = scale;
    return {x_out, h_out};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const ht::Scope hs_total(ht::BWD);
    std::optional<ht::Scope> hs_unpack(std::in_place, ht::UNPACK);
    const auto sv = ctx->get_saved_variables();
    const std::vector<int64_t> m = ctx->saved_data["m"].toIntVector();
    const at::IntArrayRef plans(m.data() + 7, 40);
    const BlockBwdArgs a{LinearPlan::parse(plans.slice(0, 10)), LinearPlan::parse(plans.slice(10, 10)),
                         MLPPlan::parse(plans.slice(20, 20)), m[0], m[1], ctx->saved_data["s"].toDouble(),
                         {m[4], m[5], m[6]}, m[2] != 0, m[3] != 0};
    hs_unpack.reset();
    variable_list out(20);
    if (ctx->saved_data.count("bg")) {  // graph-forwarded: the backward may be a graph too
      std::shared_ptr<bg::Graph> gr;
      {
        std::lock_guard<std::mutex> lk(bg::g_mu);
        auto it = bg::g_by_id.find(ctx->saved_data["bg"].toInt());
        if (it != bg::g_by_id.end()) gr = it->second.lock();
      }
      if (gr && block_bwd_graph(*gr, sv, a, grads[0], grads[1], out)) {
        ++bg::g_stat[4];
        return out;
      }
      ++bg::g_stat[5];
    }
    block_bwd(sv, a, grads[0], grads[1], out);
    return out;
  }
};


std::tuple<Tensor, Tensor> llama_block_ag(const Tensor& x, const Tensor& h, const Tensor& w_qkv,
                                          const optional<Tensor>& b_qkv, const Tensor& w_o, const optional<Tensor>& b_o,
                                          const Tensor& w_post, const Tensor& w_gu, const Tensor& w_down,
                                          const Tensor& w_next, at::IntArrayRef plan_qkv, at::IntArrayRef plan_o,
                                          at::IntArrayRef plan_mlp, int64_t H, int64_t Hkv, double scale, double eps,
                                          const optional<Tensor>& cos, const optional<Tensor>& sin, int64_t graphs,
                                          int64_t owner) {
  // graphs: the caller's per-model mode (LlamaModel.block_graphs), -1 = the process setting;
  // only parameters, or weights cast into a kept buffer (models.native(): stable addresses)
  int64_t mode = graphs < 0 ? bg::mode() : std::min<int64_t>(graphs, 2);
  if (bg::g_suspended.load(std::memory_order_relaxed)) mode = 0;  // (graphs.GraphedStep)
  if (!(c10::GradMode::is_enabled() && x.is_cuda() && (w_qkv.is_leaf() || castbuf::kept(w_qkv)))) mode = 0;
  // owner: the model's id (LlamaModel), recorded with its block graphs for a per-model reset
  auto r = LlamaBlockFn::apply(x, h, w_qkv, b_qkv, w_o, b_o, w_post, w_gu, w_down, w_next, plan_qkv, plan_o, plan_mlp,
                               H, Hkv, scale, eps, cos, sin, mode | (std::max<int64_t>(owner, 0) << 8));
  return {r[0], r[1]};
}

std::tuple<Tensor, Tensor> llama_block_noag(const Tensor& x, const Tensor& h, const Tensor& w_qkv,
                                            const optional<Tensor>& b_qkv, const Tensor& w_o,
                                            const optional<Tensor>& b_o, const Tensor& w_post, const Tensor& w_gu,
                                            const Tensor& w_down, const Tensor& w_next, at::IntArrayRef plan_qkv,
                                            at::IntArrayRef plan_o, at::IntArrayRef plan_mlp, int64_t H, int64_t Hkv,
                                            double scale, double eps, const optional<Tensor>& cos,
                                            const optional<Tensor>& sin, int64_t /*graphs*/, int64_t /*owner*/) {
  return llama_block_fwd({x, h, w_qkv, b_qkv, w_o, b_o, w_post, w_gu, w_down, w_next, plan_qkv, plan_o, plan_mlp, H, Hkv,
                          scale, eps, cos, sin},
                         nullptr);
}

// The NBD_HOST_TIMING breakdown: per section calls and mean µs; `reset` clears the counters.
std::string host_timing(bool reset) {
  static const char* const kNames[ht::kN] = {
      "block fwd (node)", "block bwd (node)", "  bwd: saved unpack", "  bwd: rms next", "  bwd: swiglu",
      "  bwd: rms post", "  bwd: linear o", "  bwd: attention", "  bwd: linear qkv", "gemm_hip call",
      "gemm_pair_hip call", "attn_bwd_hip call", "grad_out (claim+alloc)", "unused"};
  std::ostringstream os;
  for (int i = 0; i < ht::kN - 1; ++i) {
    const int64_t n = ht::g_cnt[i].load(), ns = ht::g_ns[i].load();
    if (n == 0) continue;
    os << kNames[i] << ": " << n << " calls, " << (double)ns / n / 1e3 << " us/call\n";
  }
  if (reset)
    for (int i = 0; i < ht::kN; ++i) ht::g_ns[i] = 0, ht::g_cnt[i] = 0;
  return os.str();
}

// Per-block graphs: mode 0 off, 1 forward, 2 forward and backward, -1 query; returns the previous mode.
int64_t llama_block_graphs(int64_t mode) {
  const int64_t prev = bg::mode();
  if (mode >= 0) bg::g_mode.store((int)std::min<int64_t>(mode, 2), std::memory_order_relaxed);
  return prev;
}

// Suspend every block graph, per-model modes included (graphs.GraphedStep's warm-up and
// capture); returns the previous state.
bool llama_block_graphs_suspend(bool on) { return bg::g_suspended.exchange(on); }

// Drop every captured block graph (their static memory goes once no autograd node holds it).
void llama_block_graphs_reset() {
  std::map<bg::Key, bg::Slot> slots;
  std::vector<std::shared_ptr<bg::Stack>> dropped;
  std::lock_guard<std::mutex> lk(bg::g_mu);
  slots.swap(bg::g_slots);
  dropped.swap(bg::g_dropped);
  bg::g_active.reset();
  bg::g_outs.clear();
}

// Drop the block graphs made by one model (LlamaModel's finalizer): the other models' graphs stay.
void llama_block_graphs_reset_owner(int64_t owner) {
  std::vector<bg::Slot> drop;  // (destroyed after the lock is released)
  std::vector<std::shared_ptr<bg::Stack>> stacks;  // dropped stacks of this model go too
  std::lock_guard<std::mutex> lk(bg::g_mu);
  auto active = bg::g_active.lock();
  for (auto it = bg::g_slots.begin(); it != bg::g_slots.end();) {
    if (it->second.owner != owner) {
      ++it;
      continue;
    }
    if (active && it->second.stack == active) bg::g_active.reset();
    drop.push_back(std::move(it->second));
    it = bg::g_slots.erase(it);
  }
  for (auto it = bg::g_dropped.begin(); it != bg::g_dropped.end();) {
    if ((*it)->owner == owner) {
      stacks.push_back(*it);
      it = bg::g_dropped.erase(it);
    } else {
      ++it;
    }
  }
  std::unordered_set<const bg::Graph*> gone;
  for (const auto& s : drop)
    if (s.g) gone.insert(s.g.get());
  for (auto it = bg::g_outs.begin(); it != bg::g_outs.end();) {
    auto g = it->second.lock();
    it = (!g || gone.count(g.get())) ? bg::g_outs.erase(it) : std::next(it);
  }
}

// The private memory pools of every live block / stack graph, as [id0, id1, ...] pairs: the
// caching allocator's segments in those pools are the memory block graphs hold (%dist_status).
std::vector<int64_t> llama_block_graphs_pools() {
  std::vector<int64_t> out;
  auto add = [&](const std::unique_ptr<at::cuda::CUDAGraph>& g) {
    if (!g) return;
    const auto id = g->pool();
    out.push_back((int64_t)id.first);
    out.push_back((int64_t)id.second);
  };
  std::lock_guard<std::mutex> lk(bg::g_mu);
  for (const auto& kv : bg::g_slots) {
    if (kv.second.g) {
      add(kv.second.g->g);
      for (const auto& b : kv.second.g->bwd) add(b.second->g);
    }
    if (kv.second.stack) add(kv.second.stack->g);
  }
  for (const auto& st : bg::g_dropped) add(st->g);
  return out;
}

// Tests: make the next `n` backward block-graph captures fail (the eager fallback must run).
void llama_block_graphs_fault(int64_t n) { bg::g_fail_bwd.store((int)n); }

// [captures, replays, eager calls, live graphs, backward captures, replays, eager calls]
std::vector<int64_t> llama_block_graphs_stats() {
  std::lock_guard<std::mutex> lk(bg::g_mu);
  int64_t live = 0;
  for (const auto& kv : bg::g_slots) live += kv.second.g != nullptr;
  return {bg::g_stat[0].load(), bg::g_stat[1].load(), bg::g_stat[2].load(), live,
          bg::g_stat[3].load(), bg::g_stat[4].load(), bg::g_stat[5].load(),
          bg::g_stat[6].load(), bg::g_stat[7].load(), bg::g_stat[8].load(), bg::g_stat[9].load()};
}

}  // namespace ag
}  // namespace nbd

// Autograd key: the node.  CUDA key (torch.inference_mode / no autograd): the forward alone.
TORCH_LIBRARY_IMPL(nbd, Autograd, m) { m.impl("llama_block_ag", &nbd::ag::llama_block_ag); }
TORCH_LIBRARY_IMPL(nbd, CUDA, m) { m.impl("llama_block_ag", &nbd::ag::llama_block_noag); }

// bookkeeping only (no device work): catch-all kernels
TORCH_LIBRARY_FRAGMENT(nbd, m) {
  m.def("llama_block_graphs(int mode) -> int", &nbd::ag::llama_block_graphs);
  m.def("llama_block_graphs_reset() -> ()", &nbd::ag::llama_block_graphs_reset);
  m.def("llama_block_graphs_reset_owner(int owner) -> ()", &nbd::ag::llama_block_graphs_reset_owner);
  m.def("llama_block_graphs_pools() -> int[]", &nbd::ag::llama_block_graphs_pools);
  m.def("llama_block_graphs_fault(int n) -> ()", &nbd::ag::llama_block_graphs_fault);
  m.def("llama_block_graphs_stats() -> int[]", &nbd::ag::llama_block_graphs_stats);
  m.def("host_timing(bool reset) -> str", &nbd::ag::host_timing);
  m.def("llama_block_graphs_suspend(bool on) -> bool", &nbd::ag::llama_block_graphs_suspend);
}
