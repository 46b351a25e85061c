// Entry points of attention_head_dims.hip: fused attention for bf16 head dims
// with D % 8 == 0, D <= 128 that are not multiples of 32.  The public entries
// (attention_fwd, attn_bwd_preprocess, attention_bwd, attention_bwd_dbias)
// validate shapes and dtypes and hand such calls to these.
#pragma once

#include <torch/extension.h>

std::vector<at::Tensor> attention_fwd_head_dims(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const c10::optional<at::Tensor>& mask, double scale);

std::vector<at::Tensor> attn_bwd_preprocess_head_dims(const at::Tensor& dout, const at::Tensor& o);

void attention_bwd_head_dims(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& dov, const at::Tensor& lse, const at::Tensor& delta,
    const c10::optional<at::Tensor>& mask,
    at::Tensor& dq, at::Tensor& dk, at::Tensor& dv, double scale);

// Writes chunk z of the reduction into slab z of `out` ([nsplit,mB,Hm,Nq,Nk]);
// the caller sums the slabs.
void attention_bwd_dbias_head_dims(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& dov, const at::Tensor& lse, const at::Tensor& delta,
    const at::Tensor& mask, float* out, double scale, int n_red, int chunk, int nsplit);
