// host_api.h — the host entry points that one translation unit defines and another calls.
// Included by the defining file too, so a changed signature is seen by the compiler on both sides;
// default arguments live here only.  ATen only: no device code.
#pragma once
#include <ATen/ATen.h>

#include <tuple>
#include <vector>

namespace nbd {
namespace gemm {  // gemm.hip
void gemm_hip(const at::Tensor& a, const at::Tensor& b, const at::Tensor& c, bool a_km, bool b_kn,
              const c10::optional<at::Tensor>& bias, int64_t epi, const c10::optional<at::Tensor>& aux_in,
              const c10::optional<at::Tensor>& aux_out, int64_t splits, int64_t tile_hint, int64_t accum);
void gemm_pair_hip(const at::Tensor& a1, const at::Tensor& b1, const at::Tensor& c1, int64_t epi1,
                   const c10::optional<at::Tensor>& aux_in1, const at::Tensor& a2, const at::Tensor& b2,
                   const at::Tensor& c2, int64_t epi2, const c10::optional<at::Tensor>& aux_out2, int64_t splits2,
                   int64_t accum2, const c10::optional<at::Tensor>& delta1 = c10::nullopt, int64_t delta_T = 0);
std::vector<at::Tensor> gemm_warm_take_refs();
}  // namespace gemm
namespace norm {  // norm.hip
using T3 = std::tuple<at::Tensor, at::Tensor, at::Tensor>;
using T4 = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
T4 ln_fwd_hip(const at::Tensor& x, const c10::optional<at::Tensor>& delta, const at::Tensor& weight,
              const at::Tensor& bias, double eps);
T3 ln_bwd_hip(const at::Tensor& x, const at::Tensor& dy, const c10::optional<at::Tensor>& dres, const at::Tensor& weight,
              const at::Tensor& mean, const at::Tensor& rstd);
T3 rms_fwd_hip(const at::Tensor& x, const c10::optional<at::Tensor>& delta, const at::Tensor& weight, double eps);
std::tuple<at::Tensor, at::Tensor> rms_bwd_hip(const at::Tensor& x, const at::Tensor& dy,
                                               const c10::optional<at::Tensor>& dres, const at::Tensor& weight,
                                               const at::Tensor& rstd);
T3 ln_bwd_into(const at::Tensor& x, const at::Tensor& dy, const c10::optional<at::Tensor>& dres, const at::Tensor& weight,
               const at::Tensor& mean, const at::Tensor& rstd, const at::Tensor& dw_dst, const at::Tensor& db_dst,
               int accum);
std::tuple<at::Tensor, at::Tensor> rms_bwd_into(const at::Tensor& x, const at::Tensor& dy,
                                                const c10::optional<at::Tensor>& dres, const at::Tensor& weight,
                                                const at::Tensor& rstd, const at::Tensor& dw_dst, int accum);
T3 embed_rms_fwd_hip(const at::Tensor& ids, const at::Tensor& table, const at::Tensor& weight, double eps,
                     const c10::optional<at::Tensor>& err);
T4 tokpos_ln_fwd_hip(const at::Tensor& idx, const at::Tensor& wte, const at::Tensor& pos, const at::Tensor& wpe,
                     int64_t vocab, const at::Tensor& weight, const at::Tensor& bias, double eps,
                     const c10::optional<at::Tensor>& err);
}  // namespace norm
namespace embed {  // embed.hip
at::Tensor embedding_bwd_hip(const at::Tensor& dy, const at::Tensor& idx, int64_t V,
                             const c10::optional<at::Tensor>& grad_out, bool accumulate);
at::Tensor embedding_pos_bwd_hip(const at::Tensor& dy, const at::Tensor& pos, int64_t P,
                                 const c10::optional<at::Tensor>& out_opt, bool accumulate);
}  // namespace embed
namespace attn {  // attn.hip
std::tuple<at::Tensor, at::Tensor> attn_fwd_hip(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                                bool causal, double scale, const c10::optional<at::Tensor>& rope_cos,
                                                const c10::optional<at::Tensor>& rope_sin);
void attn_bwd_hip(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                  const at::Tensor& out, const at::Tensor& lse, bool causal, double scale, const at::Tensor& dq,
                  const at::Tensor& dk, const at::Tensor& dv, const c10::optional<at::Tensor>& rope_cos,
                  const c10::optional<at::Tensor>& rope_sin, const c10::optional<at::Tensor>& delta = c10::nullopt);
}  // namespace attn
// bucket.hip
void bucket_flatten_hip(at::TensorList tensors, const at::Tensor& bucket, at::IntArrayRef offsets, double scale,
                        bool accumulate);
}  // namespace nbd
