// Fused rotary position embedding for q and k (gfx950), forward and backward.
//
// Replaces the eager chain in EvaAttention / AttentionRope (prefix slice,
// rot(x) via strided slices + stack, two multiplies, add, cat, cast) with one
// launch that rotates q and k together, so every [sin | cos] chunk is loaded
// once and applied to both tensors.
//
//   q, k  : [B, H, N, D], arbitrary b/h/n strides, contiguous last dim
//   rope  : [Br, Hr, N - npt, 2D], Br in {1,B}, Hr in {1,H} (stride 0 when
//           broadcast), last dim = [sin | cos], fp32 or bf16
//   out   : [B, N, H, D] storage returned as [B, H, N, D] views
//
// Rows n < npt (prefix tokens) are copied through; row n >= npt uses table row
// n - npt.  sin/cos are indexed per element: nothing assumes s[2i] == s[2i+1]
// (mixed / learned tables do not guarantee it).
//
//   interleaved fwd: y[2i]   = x[2i]  c[2i]   - x[2i+1] s[2i]
//                    y[2i+1] = x[2i+1]c[2i+1] + x[2i]   s[2i+1]
//               bwd: dx[2i]   = dy[2i]  c[2i]   + dy[2i+1] s[2i+1]
//                    dx[2i+1] = dy[2i+1]c[2i+1] - dy[2i]   s[2i]
//   half (h = D/2) fwd: y[j]   = x[j]  c[j]   - x[j+h] s[j]
//                       y[j+h] = x[j+h]c[j+h] + x[j]   s[j+h]
//                  bwd: dx[j]   = dy[j]  c[j]   + dy[j+h] s[j+h]
//                       dx[j+h] = dy[j+h]c[j+h] - dy[j]   s[j]
//
// HBM-bound: 16B accesses per lane (short8 / f32x4), fp32 math, one rounding
// at the store (guide Appendix B, elementwise).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8 blocks, grid-stride the rest
constexpr int kChunk = 8;         // elements per work item and tensor

// 8 consecutive elements <-> fp32 registers, 16B per access.
__device__ __forceinline__ void load8(const float* p, float (&v)[kChunk]) {
  f32x4 a = *reinterpret_cast<const f32x4*>(p);
  f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[j + 4] = b[j]; }
}
__device__ __forceinline__ void load8(const __hip_bfloat16* p, float (&v)[kChunk]) {
  short8 a = *reinterpret_cast<const short8*>(p);
#pragma unroll
  for (int j = 0; j < kChunk; ++j) v[j] = bf16s_to_f32(a[j]);
}
__device__ __forceinline__ void store8(float* p, const float (&v)[kChunk]) {
  f32x4 a, b;
#pragma unroll
  for (int j = 0; j < 4; ++j) { a[j] = v[j]; b[j] = v[j + 4]; }
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}
__device__ __forceinline__ void store8(__hip_bfloat16* p, const float (&v)[kChunk]) {
  short8 a;
#pragma unroll
  for (int j = 0; j < kChunk; ++j) {
    __hip_bfloat16 r = __float2bfloat16(v[j]);
    a[j] = *reinterpret_cast<const short*>(&r);
  }
  *reinterpret_cast<short8*>(p) = a;
}

struct RopeParams {
  const void* q; const void* k; const void* rope;
  void* oq; void* ok;
  long q_sb, q_sh, q_sn;     // element strides
  long k_sb, k_sh, k_sn;
  long r_sb, r_sh, r_sn;     // 0 on broadcast dims
  long o_sb, o_sh, o_sn;     // both outputs share one layout
  unsigned total;            // B*H*N*cpr work items
  unsigned H, N, cpr;        // cpr: work items per [D] row
  int npt, D;
};

// interleaved: one chunk of 4 (even, odd) pairs
template <bool BWD>
__device__ __forceinline__ void rotate_pairs(
    const float (&x)[kChunk], const float (&s)[kChunk], const float (&c)[kChunk],
    float (&y)[kChunk]) {
#pragma unroll
  for (int i = 0; i < kChunk; i += 2) {
    if (BWD) {
      y[i]     = x[i] * c[i] + x[i + 1] * s[i + 1];
      y[i + 1] = x[i + 1] * c[i + 1] - x[i] * s[i];
    } else {
      y[i]     = x[i] * c[i] - x[i + 1] * s[i];
      y[i + 1] = x[i + 1] * c[i + 1] + x[i] * s[i + 1];
    }
  }
}

// half: chunk j (lo) and chunk j + D/2 (hi)
template <bool BWD>
__device__ __forceinline__ void rotate_halves(
    const float (&xl)[kChunk], const float (&xh)[kChunk],
    const float (&sl)[kChunk], const float (&sh)[kChunk],
    const float (&cl)[kChunk], const float (&ch)[kChunk],
    float (&yl)[kChunk], float (&yh)[kChunk]) {
#pragma unroll
  for (int j = 0; j < kChunk; ++j) {
    if (BWD) {
      yl[j] = xl[j] * cl[j] + xh[j] * sh[j];
      yh[j] = xh[j] * ch[j] - xl[j] * sl[j];
    } else {
      yl[j] = xl[j] * cl[j] - xh[j] * sl[j];
      yh[j] = xh[j] * ch[j] + xl[j] * sh[j];
    }
  }
}

template <typename TIn, typename TOut, typename TTab, bool HALF, bool BWD>
__global__ __launch_bounds__(kBlock)
void rope_qk_kernel(RopeParams p) {
  const TIn* __restrict__ q = static_cast<const TIn*>(p.q);
  const TIn* __restrict__ k = static_cast<const TIn*>(p.k);
  const TTab* __restrict__ tab = static_cast<const TTab*>(p.rope);
  TOut* __restrict__ oq = static_cast<TOut*>(p.oq);
  TOut* __restrict__ ok = static_cast<TOut*>(p.ok);
  const int half_d = p.D / 2;

  const unsigned step = gridDim.x * kBlock;
  // 64-bit loop counter: u + step may pass 2^32 on the last trip
  for (unsigned long u = (unsigned long)blockIdx.x * kBlock + threadIdx.x; u < p.total; u += step) {
    // chunk fastest, then head, then token: matches the [B,N,H,D] output
    // storage and the packed [B,N,3,H,D] projection the inputs usually view
    unsigned t = (unsigned)u;
    const unsigned c = t % p.cpr; t /= p.cpr;
    const unsigned h = t % p.H;   t /= p.H;
    const unsigned n = t % p.N;
    const unsigned b = t / p.N;
    const int col = (int)c * kChunk;

    const long qo = (long)b * p.q_sb + (long)h * p.q_sh + (long)n * p.q_sn + col;
    const long ko = (long)b * p.k_sb + (long)h * p.k_sh + (long)n * p.k_sn + col;
    const long oo = (long)b * p.o_sb + (long)h * p.o_sh + (long)n * p.o_sn + col;

    float xq[kChunk], xk[kChunk], yq[kChunk], yk[kChunk];
    load8(q + qo, xq);
    load8(k + ko, xk);

    if ((int)n < p.npt) {
      // prefix token: copy through (cast only)
      store8(oq + oo, xq);
      store8(ok + oo, xk);
      if (HALF) {
        load8(q + qo + half_d, xq);
        load8(k + ko + half_d, xk);
        store8(oq + oo + half_d, xq);
        store8(ok + oo + half_d, xk);
      }
      continue;
    }

    const long ro = (long)b * p.r_sb + (long)h * p.r_sh + (long)((int)n - p.npt) * p.r_sn + col;
    float s[kChunk], cs[kChunk];
    load8(tab + ro, s);
    load8(tab + ro + p.D, cs);

    if (HALF) {
      float xq_hi[kChunk], xk_hi[kChunk], yq_hi[kChunk], yk_hi[kChunk];
      float s_hi[kChunk], c_hi[kChunk];
      load8(q + qo + half_d, xq_hi);
      load8(k + ko + half_d, xk_hi);
      load8(tab + ro + half_d, s_hi);
      load8(tab + ro + p.D + half_d, c_hi);
      rotate_halves<BWD>(xq, xq_hi, s, s_hi, cs, c_hi, yq, yq_hi);
      rotate_halves<BWD>(xk, xk_hi, s, s_hi, cs, c_hi, yk, yk_hi);
      store8(oq + oo + half_d, yq_hi);
      store8(ok + oo + half_d, yk_hi);
    } else {
      rotate_pairs<BWD>(xq, s, cs, yq);
      rotate_pairs<BWD>(xk, s, cs, yk);
    }
    store8(oq + oo, yq);
    store8(ok + oo, yk);
  }
}

template <typename TIn, typename TOut, typename TTab>
void launch_rope(const RopeParams& p, bool half, bool bwd, int blocks, hipStream_t stream) {
  auto go = [&](auto htag, auto btag) {
    hipLaunchKernelGGL(
        (rope_qk_kernel<TIn, TOut, TTab, decltype(htag)::value, decltype(btag)::value>),
        dim3(blocks), dim3(kBlock), 0, stream, p);
  };
  if (half && bwd) go(std::true_type{}, std::true_type{});
  else if (half) go(std::true_type{}, std::false_type{});
  else if (bwd) go(std::false_type{}, std::true_type{});
  else go(std::false_type{}, std::false_type{});
}

template <typename TIn, typename TOut>
void launch_rope_tab(const RopeParams& p, at::ScalarType tab, bool half, bool bwd, int blocks,
                     hipStream_t stream) {
  if (tab == at::kFloat) launch_rope<TIn, TOut, float>(p, half, bwd, blocks, stream);
  else launch_rope<TIn, TOut, __hip_bfloat16>(p, half, bwd, blocks, stream);
}

bool aligned16(const at::Tensor& t) {
  const long es = t.element_size();
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 != 0) return false;
  for (int d = 0; d < 3; ++d) {
    if (t.size(d) > 1 && (t.stride(d) * es) % 16 != 0) return false;
  }
  return true;
}

}  // namespace

// Rotates q and k in one launch.  bwd=false: inputs are q/k, output dtype
// `out_dtype`.  bwd=true: inputs are the output grads, `out_dtype` is the
// dtype of the forward inputs.
std::vector<at::Tensor> rope_qk(at::Tensor q, at::Tensor k, at::Tensor rope,
                                long npt, bool half, bool bwd, at::ScalarType out_dtype) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && rope.is_cuda(), "rope_qk: tensors must be on the GPU");
  TORCH_CHECK(q.device() == k.device() && q.device() == rope.device(),
              "rope_qk: q, k and rope must share a device");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && rope.dim() == 4,
              "rope_qk: q, k and rope must be 4-D");
  TORCH_CHECK(q.sizes() == k.sizes(), "rope_qk: q and k must have the same shape");
  TORCH_CHECK(q.scalar_type() == k.scalar_type(), "rope_qk: q and k must share a dtype");
  const long B = q.size(0), H = q.size(1), N = q.size(2), D = q.size(3);
  TORCH_CHECK(D % (half ? 2 * kChunk : kChunk) == 0,
              "rope_qk: head dim ", D, " must be a multiple of ", half ? 2 * kChunk : kChunk);
  TORCH_CHECK(npt >= 0 && npt <= N, "rope_qk: num_prefix_tokens ", npt, " outside [0, ", N, "]");
  TORCH_CHECK(rope.size(3) == 2 * D, "rope_qk: rope last dim must be 2*D = ", 2 * D);
  TORCH_CHECK(rope.size(2) == N - npt, "rope_qk: rope has ", rope.size(2), " rows, expected ", N - npt);
  TORCH_CHECK(rope.size(0) == 1 || rope.size(0) == B, "rope_qk: rope batch dim must be 1 or B");
  TORCH_CHECK(rope.size(1) == 1 || rope.size(1) == H, "rope_qk: rope head dim must be 1 or H");

  const auto in_t = q.scalar_type();
  const auto tab_t = rope.scalar_type();
  TORCH_CHECK(tab_t == at::kFloat || tab_t == at::kBFloat16, "rope_qk: rope must be fp32 or bf16");
  const bool bb = in_t == at::kBFloat16 && out_dtype == at::kBFloat16;
  const bool ff = in_t == at::kFloat && out_dtype == at::kFloat;
  // fwd casts fp32 -> bf16 (qk-norm output under autocast), its bwd bf16 -> fp32
  const bool mixed = bwd ? (in_t == at::kBFloat16 && out_dtype == at::kFloat)
                         : (in_t == at::kFloat && out_dtype == at::kBFloat16);
  TORCH_CHECK(bb || ff || mixed, "rope_qk: unsupported dtype combination ", in_t, " -> ", out_dtype);

  auto oq = at::empty({B, N, H, D}, q.options().dtype(out_dtype)).permute({0, 2, 1, 3});
  auto ok = at::empty({B, N, H, D}, q.options().dtype(out_dtype)).permute({0, 2, 1, 3});
  const long cpr = D / (half ? 2 * kChunk : kChunk);
  const long total = B * H * N * cpr;
  if (total == 0) return {oq, ok};
  TORCH_CHECK(total < (1L << 31), "rope_qk: too many elements for one launch");

  TORCH_CHECK(q.stride(3) == 1 && k.stride(3) == 1 && rope.stride(3) == 1,
              "rope_qk: last dim must be contiguous");
  TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(rope),
              "rope_qk: data pointers and b/h/n strides must be 16-byte aligned");

  RopeParams p;
  p.q = q.data_ptr(); p.k = k.data_ptr(); p.rope = rope.data_ptr();
  p.oq = oq.data_ptr(); p.ok = ok.data_ptr();
  p.q_sb = q.stride(0); p.q_sh = q.stride(1); p.q_sn = q.stride(2);
  p.k_sb = k.stride(0); p.k_sh = k.stride(1); p.k_sn = k.stride(2);
  p.r_sb = rope.size(0) == 1 ? 0 : rope.stride(0);
  p.r_sh = rope.size(1) == 1 ? 0 : rope.stride(1);
  p.r_sn = rope.stride(2);
  p.o_sb = oq.stride(0); p.o_sh = oq.stride(1); p.o_sn = oq.stride(2);
  p.total = (unsigned)total;
  p.H = (unsigned)H; p.N = (unsigned)N; p.cpr = (unsigned)cpr;
  p.npt = (int)npt; p.D = (int)D;

  const int blocks = (int)std::min((long)kMaxBlocks, (total + kBlock - 1) / kBlock);
  auto stream = at::hip::getCurrentHIPStream();
  if (bb) launch_rope_tab<__hip_bfloat16, __hip_bfloat16>(p, tab_t, half, bwd, blocks, stream);
  else if (ff) launch_rope_tab<float, float>(p, tab_t, half, bwd, blocks, stream);
  else if (bwd) launch_rope_tab<__hip_bfloat16, float>(p, tab_t, half, bwd, blocks, stream);
  else launch_rope_tab<float, __hip_bfloat16>(p, tab_t, half, bwd, blocks, stream);
  HIP_CHECK_LAST();
  return {oq, ok};
}
