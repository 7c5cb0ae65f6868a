// cast_group.hip — fp32 master weights, bf16 compute: the cast node of `models.native()`.
//
// One decoder layer's parameters cast into one flat compute-dtype buffer by one bucket_flatten
// pass, and their gradients cast back into one flat fp32 buffer by another (models/llama.py
// _CastGroup, the Python form of the same node): `models.native()` runs one per layer per
// forward, and the Python autograd.Function around it was ≈20-30 µs of host time per call and
// direction on a host-bound loop (docs/FINDINGS.md §30).
#include <c10/core/GradMode.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <unordered_map>

#include "ag_common.h"

namespace nbd {
namespace ag {

static std::pair<std::vector<int64_t>, int64_t> flat_offsets(const std::vector<Tensor>& ts) {
  std::vector<int64_t> offs;
  offs.reserve(ts.size());
  int64_t pos = 0;
  for (const Tensor& t : ts) {
    offs.push_back(pos);
    pos += (t.numel() + 63) / 64 * 64;  // 64-element starts: every slice on the 16-B vector path
  }
  return {offs, pos};
}

static std::vector<Tensor> slices(const Tensor& buf, const std::vector<int64_t>& offs,
                                  const std::vector<std::vector<int64_t>>& shapes) {
  std::vector<Tensor> out;
  out.reserve(offs.size());
  for (size_t i = 0; i < offs.size(); ++i) {
    int64_t n = 1;
    for (int64_t d : shapes[i]) n *= d;
    out.push_back(buf.narrow(0, offs[i], n).view(shapes[i]));
  }
  return out;
}

// The cast buffer of a parameter group is kept and rewritten by the next forward when nothing
// else holds it any more (the previous pass's autograd graph has released its saved weights):
// the compute-dtype weights then stay at the same addresses from step to step, which is what lets
// the per-block graphs (namespace bg) run on the fp32-master path too.  Still held (a second
// forward before backward): a fresh buffer, as before.
namespace castbuf {
struct Entry {
  c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl> first;  // the group's first parameter (validates the key)
  Tensor buf;
  std::shared_ptr<std::atomic<bool>> busy;  // a cast node of an earlier pass still owns it
  Tensor gbuf;  // the kept cast's gradient buffer (same layout): its slices are the cast weights'
                // registered gradient destinations (graddst::set), allocated on first use
};
std::mutex g_mu;
std::unordered_map<const c10::TensorImpl*, Entry> g_bufs;
std::unordered_map<const void*, int> g_addrs;  // data pointers of the kept buffers
std::vector<Tensor> g_old;                      // replaced buffers (see get)

// The buffer for this group's cast and, when it is the kept one, the flag its node releases
// (a token among the node's saved tensors: freed by that node's backward — which runs after every
// node that saved the cast weights — or with the node).  Storage use counts cannot tell: the
// block graphs keep references to the weights they were captured with.
std::pair<Tensor, std::shared_ptr<std::atomic<bool>>> get(const Tensor& first, int64_t total,
                                                          const at::TensorOptions& opt) {
  std::lock_guard<std::mutex> lk(g_mu);
  // forget the groups of dead parameters (a re-run `model = native(...)` cell must not keep the
  // old model's cast and gradient buffers); the map holds a few groups per live model
  for (auto it = g_bufs.begin(); it != g_bufs.end();) {
    if (it->second.first.expired()) {
      g_addrs.erase(it->second.buf.data_ptr());
      it = g_bufs.erase(it);
    } else {
      ++it;
    }
  }
  auto it = g_bufs.find(first.unsafeGetTensorImpl());
  if (it != g_bufs.end() && !it->second.first.expired() && it->second.buf.numel() == total &&
      it->second.buf.scalar_type() == opt.dtype().toScalarType() && it->second.buf.device() == opt.device()) {
    if (!it->second.busy->exchange(true)) return {it->second.buf, it->second.busy};
    return {at::empty({total}, opt), nullptr};  // still owned (a second forward before backward): a temporary
  }
  Tensor buf = at::empty({total}, opt);
  auto busy = std::make_shared<std::atomic<bool>>(true);
  if (it != g_bufs.end()) {  // (the group changed shape: the old buffer may still be read by a
    g_old.push_back(it->second.buf);  // captured warm-up — keep it, bounded)
    if (g_old.size() > 64) g_old.erase(g_old.begin());
    g_addrs.erase(it->second.buf.data_ptr());
  }
  g_bufs.insert_or_assign(first.unsafeGetTensorImpl(),
                          Entry{c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>(
                                    first.getIntrusivePtr()),
                                buf, busy});
  g_addrs[buf.data_ptr()] = 1;
  return {buf, busy};
}

// The gradient buffer of the group whose kept cast buffer is `buf` (allocated on first use).
Tensor grad_buf(const Tensor& first, const Tensor& buf) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_bufs.find(first.unsafeGetTensorImpl());
  if (it == g_bufs.end() || !it->second.buf.is_same(buf)) return Tensor();
  if (!it->second.gbuf.defined()) it->second.gbuf = at::empty_like(buf);
  return it->second.gbuf;
}

// [live groups, cast-buffer bytes, gradient-buffer bytes] held for models.native()'s kept casts
// (bytes of every held group: a dead model's stay until the next cast purges them; %dist_status)
std::vector<int64_t> memory() {
  std::lock_guard<std::mutex> lk(g_mu);
  int64_t n = 0, cb = 0, gb = 0;
  for (const auto& kv : g_bufs) {
    n += !kv.second.first.expired();
    cb += kv.second.buf.nbytes();
    if (kv.second.gbuf.defined()) gb += kv.second.gbuf.nbytes();
  }
  return {n, cb, gb};
}

// t lives in a kept cast buffer (its address is stable across steps)
bool kept(const Tensor& t) {
  if (!t.has_storage()) return false;
  std::lock_guard<std::mutex> lk(g_mu);
  return g_addrs.count(t.storage().data()) != 0;
}

std::vector<Tensor> drop_kept(std::vector<Tensor> refs) {
  std::lock_guard<std::mutex> lk(g_mu);
  refs.erase(std::remove_if(refs.begin(), refs.end(),
                            [](const Tensor& t) { return t.has_storage() && g_addrs.count(t.storage().data()) != 0; }),
             refs.end());
  return refs;
}
}  // namespace castbuf

// Gradient destinations for the cast weights (NBD_CAST_GRAD_DEST=0: off).  A kept cast (stable
// addresses) gets a kept gradient buffer of the same layout; cast_group_ag registers each returned
// weight's slice of it (graddst::set), so the decoder block's backward writes the weight gradients
// there — static addresses, which is what lets the block's backward run as a HIP graph (bg, mode 2)
// on the fp32-master path — and the cast node's backward reads them from one place.
static bool cast_grad_dest_on() {
  static const bool on = [] {
    const char* e = std::getenv("NBD_CAST_GRAD_DEST");
    return e == nullptr || std::atoi(e) != 0;
  }();
  return on;
}
thread_local Tensor t_cast_gbuf;  // forward -> cast_group_ag: the gradient buffer to register

struct CastGroupFn : public torch::autograd::Function<CastGroupFn> {
  // (ps as a TensorList: only that form counts its elements as the node's inputs)
  static variable_list forward(AutogradContext* ctx, at::TensorList ps, int64_t dtype) {
    at::AutoDispatchBelowADInplaceOrView guard;
    TORCH_CHECK(!ps.empty(), "cast_group: no tensors");
    auto [offs, total] = flat_offsets(ps.vec());
    std::vector<std::vector<int64_t>> shapes;
    for (const Tensor& p : ps) {
      TORCH_CHECK(p.is_cuda() && p.device() == ps[0].device() && p.scalar_type() == ps[0].scalar_type(),
                  "cast_group: one device and dtype");
      shapes.push_back(p.sizes().vec());
    }
    auto [buf, busy] = castbuf::get(ps[0], total, ps[0].options().dtype((at::ScalarType)dtype));
    bg::g_cast_epoch.fetch_add(1, std::memory_order_acq_rel);
    if (busy) ctx->save_for_backward({release_token([busy = busy] { busy->store(false, std::memory_order_release); })});
    t_cast_gbuf = busy && cast_grad_dest_on() ? castbuf::grad_buf(ps[0], buf) : Tensor();
    std::vector<Tensor> src;
    src.reserve(ps.size());
    for (const Tensor& p : ps) src.push_back(p.contiguous());
    bucket_flatten_hip(src, buf, offs, 1.0, false);
    std::vector<int64_t> flat_shapes;
    for (const auto& sh : shapes) {
      flat_shapes.push_back((int64_t)sh.size());
      flat_shapes.insert(flat_shapes.end(), sh.begin(), sh.end());
    }
    ctx->saved_data["offs"] = offs;
    ctx->saved_data["shapes"] = flat_shapes;
    ctx->saved_data["meta"] = std::vector<int64_t>{total, (int64_t)ps[0].scalar_type()};
    return slices(buf, offs, shapes);
  }

  static variable_list backward(AutogradContext* ctx, variable_list gs) {
    const auto offs = ctx->saved_data["offs"].toIntVector();
    const auto flat = ctx->saved_data["shapes"].toIntVector();
    const auto meta = ctx->saved_data["meta"].toIntVector();
    std::vector<std::vector<int64_t>> shapes;
    for (size_t i = 0; i < flat.size();) {
      const int64_t r = flat[i];
      shapes.emplace_back(flat.begin() + (int64_t)i + 1, flat.begin() + (int64_t)i + 1 + r);
      i += (size_t)r + 1;
    }
    variable_list out(gs.size() + 1);  // (the dtype argument: none)
    // weight gradients written into the registered slices may still have reductions queued
    // (defer.hip: nothing else flushes them on this path)
    if (defer::pending() > 0) defer::flush();
    std::vector<Tensor> have;
    std::vector<int64_t> have_offs;
    for (size_t i = 0; i < gs.size(); ++i)
      if (gs[i].defined()) {
        have.push_back(gs[i].contiguous());
        have_offs.push_back(offs[i]);
      }
    if (have.empty()) return out;
    const Tensor buf = at::empty({meta[0]}, have[0].options().dtype((at::ScalarType)meta[1]));
    bucket_flatten_hip(have, buf, have_offs, 1.0, false);
    const auto views = slices(buf, offs, shapes);
    for (size_t i = 0; i < gs.size(); ++i)
      if (gs[i].defined()) out[i] = views[i];
    return out;
  }
};

std::vector<Tensor> cast_group_ag(at::TensorList ps, int64_t dtype) {
  t_cast_gbuf = Tensor();
  std::vector<Tensor> out = CastGroupFn::apply(ps, dtype);
  const Tensor gbuf = std::move(t_cast_gbuf);
  t_cast_gbuf = Tensor();
  if (gbuf.defined() && c10::GradMode::is_enabled()) {
    auto [offs, total] = flat_offsets(ps.vec());
    for (size_t i = 0; i < out.size(); ++i)
      if (out[i].requires_grad()) graddst::set(out[i], gbuf.narrow(0, offs[i], out[i].numel()).view(out[i].sizes()));
  }
  return out;
}

std::vector<Tensor> cast_group_noag(at::TensorList ps, int64_t dtype) {
  const std::vector<Tensor> v = ps.vec();
  auto [offs, total] = flat_offsets(v);
  std::vector<std::vector<int64_t>> shapes;
  std::vector<Tensor> src;
  for (const Tensor& p : v) {
    shapes.push_back(p.sizes().vec());
    src.push_back(p.contiguous());
  }
  const Tensor buf = at::empty({total}, v[0].options().dtype((at::ScalarType)dtype));
  bucket_flatten_hip(src, buf, offs, 1.0, false);
  return slices(buf, offs, shapes);
}

}  // namespace ag
}  // namespace nbd

// Autograd key: the node.  CUDA key (torch.inference_mode / no autograd): the forward alone.
TORCH_LIBRARY_IMPL(nbd, Autograd, m) { m.impl("cast_group_ag", &nbd::ag::cast_group_ag); }
TORCH_LIBRARY_IMPL(nbd, CUDA, m) { m.impl("cast_group_ag", &nbd::ag::cast_group_noag); }
TORCH_LIBRARY_FRAGMENT(nbd, m) { m.def("cast_buffers_memory() -> int[]", &nbd::ag::castbuf::memory); }
