// Cross-covariance attention (XCiT's XCA), forward and backward: bf16,
// head_dim 32 / 48 / 64, any number of tokens N >= 1, gfx950.
//
// Per (batch, head), with Q, K, V the [N, d] slices of the packed qkv Linear
// output [B, N, 3, H, d] (token rows, channel contiguous):
//
//   nq_i = max(|Q[:, i]|, 1e-12), nk_j likewise   (norms over the tokens)
//   G = Q^T K                                     (d x d, reduction over tokens)
//   C = G / (nq nk^T),  A = softmax_rows(tau C),  O[n, :] = A V[n, :]
//
// and, given dO:
//
//   dV[n, :] = A^T dO[n, :],  dA = dO^T V,  dS = A o (dA - rowsum(A o dA)),
//   dtau = sum(dS o C),  dC = tau dS,  W = dC / (nq nk^T),
//   rq_i = sum_j dC_ij C_ij,  rk_j = sum_i dC_ij C_ij,
//   dQ[n, :] = W K[n, :] - (rq / nq^2) o Q[n, :],
//   dK[n, :] = W^T Q[n, :] - (rk / nk^2) o K[n, :].
//
// The token axis is the reduction axis of the first GEMM and the softmax runs
// over channels, so neither q^, k^, a [.., d, N] copy of qkv nor any gradient
// of a normalised tensor ever exists.  O is written as [B, N, H*d] and dqkv as
// one [B, N, 3, H, d] buffer.
//
// Split of the work.  One workgroup of four waves owns a (batch, head) pair
// and makes two passes over the tokens.
//
//  Pass 1 (token_gram): d x d = X^T Y with the token as the MFMA reduction
//  dimension (X, Y = Q, K in the forward; dO, V in the backward).  All 256
//  threads stage 128 token rows of both tensors as [128][d] bf16 LDS images
//  (rows padded by 16 bytes, so the 16 rows x 32 bytes of one transposed read
//  fall on different banks); both MFMA operands are transposed LDS reads
//  (ds_read_b64_tr_b16, the V^T path of the window kernels).  The waves split
//  the TOKENS, not the output tiles: wave w owns the 32-token MFMA step w of
//  every round and accumulates all (d/16)^2 output tiles.  Reasons: d = 32 has
//  four tiles and d = 48 nine, which four waves cannot share evenly, while
//  tokens split evenly at every d; and a wave that owns all tiles reads d/16
//  + d/16 operand fragments for (d/16)^2 MFMA, the best reuse available.  The
//  price is one reduction of four partials through LDS, done once per
//  workgroup in the fixed order (w0 + w2) + (w1 + w3).  The next round's rows
//  are fetched into registers while the MFMA of the current round run.
//  A thread stages the same eight channels in every round, so the sums of
//  squares for the norms are eight fp32 accumulators per tensor fed by the
//  staging loads themselves; they are reduced over the thread groups in group
//  order.  Rows past N are staged as zeros.
//
//  d x d stage: four threads per row, row reductions by two shuffles.  G (or
//  dA), C, A, dS, dC and the sums dtau, rq, rk are fp32 in registers / LDS.
//  The forward saves C [B, H, d, d] and the inverse norms [B, H, 2, d] (fp32),
//  so the backward's pass 1 reads dO and V only and recomputes A from C with
//  the forward's own code.  rk is a column sum: dC o C goes through LDS once
//  and is summed in row order.  dtau: lanes by shuffle, waves in wave order,
//  one partial per workgroup in a [B, H] buffer that the caller sums over B.
//  No atomics: the same bits on every run.
//
//  Pass 2: the channel is the reduction dimension.  A, A^T, W and W^T are
//  rounded to bf16 once and held in registers as MFMA A operands for the whole
//  loop; the waves take 16-token blocks round-robin and load token rows of V
//  (dO, K, Q) from global memory straight into B-operand registers (lane =
//  token, 8 or 4 consecutive channels).  The accumulator then holds four
//  consecutive channels of the lane's token: one 8-byte store.  d = 48 is one
//  16x16x32 step plus one 16x16x16 step.  The diag(.) terms of dQ / dK are
//  applied in fp32 to an 8-byte load of the raw Q / K quad.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef short short4_t __attribute__((ext_vector_type(4)));
typedef short short8_t __attribute__((ext_vector_type(8)));

constexpr float kNormEps = 1e-12f;  // F.normalize
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * WAVE_SIZE;
constexpr int kRound = kWaves * 32;  // tokens staged per round: one 32-token MFMA step per wave

constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int D>
struct Cfg {
  static constexpr int NT = D / 16;            // 16-channel tiles
  static constexpr int KF = D / 32;            // 16x16x32 steps over the channels
  static constexpr bool kTail = D % 32 == 16;  // plus one 16x16x16 step
  static constexpr int CH = D / 8;             // 16-byte chunks of a token row
  static constexpr int GRP = kThreads / CH;    // token rows staged per iteration
  static constexpr int NIT = (kRound + GRP - 1) / GRP;
  static constexpr int STRIDE = 2 * D + 16;    // bytes of an image row
  static constexpr int IMG = kRound * STRIDE;
  static constexpr int LD = D + 4;             // row length of a d x d fp32 matrix in LDS
  static constexpr int MAT = D * LD;
  // the images, the two d x d matrices and the sum-of-squares partials share one buffer
  static constexpr int SMEM = cmax(2 * IMG, cmax(2 * MAT * 4, 2 * GRP * D * 4));
};

__device__ __forceinline__ bf16x8_t load_row(const __bf16* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}

// Two ds_read_b64_tr_b16 -> one 16x16x32 operand fragment.  Every lane of the
// wave must be active.
__device__ __forceinline__ bf16x8_t tr_pair(const char* lds, int off0, int off1) {
  typedef __attribute__((address_space(3))) short4_t* lds_ptr;
  short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(lds + off0));
  short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(lds + off1));
  short8_t r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8_t, r);
}

// acc[it][jt] += X^T Y over this wave's tokens: X = pa, Y = pb, token rows of
// D channels with row strides ra / rb (elements).  With NORMS the staging
// threads also accumulate the sums of squares of their eight channels.
// Ends with a barrier: the images are free afterwards.
template <int D, bool NORMS>
__device__ __forceinline__ void token_gram(
    const __bf16* __restrict__ pa, long ra, const __bf16* __restrict__ pb, long rb, int N,
    char* img_a, char* img_b, f32x4 (&acc)[Cfg<D>::NT][Cfg<D>::NT], float (&ssa)[8], float (&ssb)[8]) {
  using C = Cfg<D>;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int g4 = lane >> 4;
  const int tq = (lane & 15) >> 2;
  const int tp = lane & 3;
  const bool stager = tid < C::GRP * C::CH;
  const int grp = tid / C::CH;
  const int ch = tid % C::CH;

  bf16x8_t xa[C::NIT], xb[C::NIT];
  auto fetch = [&](int base) {
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int t = it * C::GRP + grp;
      const int n = base + t;
      xa[it] = bf16x8_t{};
      xb[it] = bf16x8_t{};
      if (stager && t < kRound && n < N) {
        xa[it] = load_row(pa + (long)n * ra + ch * 8);
        xb[it] = load_row(pb + (long)n * rb + ch * 8);
      }
    }
  };
  fetch(0);
  for (int base = 0; base < N; base += kRound) {
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int t = it * C::GRP + grp;
      if (stager && t < kRound) {
        *reinterpret_cast<bf16x8_t*>(img_a + t * C::STRIDE + ch * 16) = xa[it];
        *reinterpret_cast<bf16x8_t*>(img_b + t * C::STRIDE + ch * 16) = xb[it];
        if (NORMS) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            ssa[e] += (float)xa[it][e] * (float)xa[it][e];
            ssb[e] += (float)xb[it][e] * (float)xb[it][e];
          }
        }
      }
    }
    __syncthreads();
    if (base + kRound < N) fetch(base + kRound);
    if (base + wave * 32 < N) {  // wave-uniform; rows past N are zeros
      const int row = wave * 32 + g4 * 4 + tq;
      bf16x8_t fa[C::NT], fb[C::NT];
#pragma unroll
      for (int t = 0; t < C::NT; ++t) {
        const int off = row * C::STRIDE + t * 32 + tp * 8;
        fa[t] = tr_pair(img_a, off, off + 16 * C::STRIDE);
        fb[t] = tr_pair(img_b, off, off + 16 * C::STRIDE);
      }
#pragma unroll
      for (int it = 0; it < C::NT; ++it) {
#pragma unroll
        for (int jt = 0; jt < C::NT; ++jt) {
          acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[it], fb[jt], acc[it][jt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
}

// Sum of the four waves' partial tiles, (w0 + w2) + (w1 + w3), left in slot0
// as a [D][LD] matrix.  Ends with a barrier.
template <int D>
__device__ __forceinline__ void reduce_partials(
    f32x4 (&acc)[Cfg<D>::NT][Cfg<D>::NT], float* slot0, float* slot1) {
  using C = Cfg<D>;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE_SIZE);
  const int l16 = threadIdx.x & 15;
  const int g4 = (threadIdx.x % WAVE_SIZE) >> 4;
  auto put = [&](float* s) {
#pragma unroll
    for (int it = 0; it < C::NT; ++it)
#pragma unroll
      for (int jt = 0; jt < C::NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[(it * 16 + g4 * 4 + r) * C::LD + jt * 16 + l16] = acc[it][jt][r];
  };
  auto add = [&](const float* s) {
#pragma unroll
    for (int it = 0; it < C::NT; ++it)
#pragma unroll
      for (int jt = 0; jt < C::NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[it][jt][r] += s[(it * 16 + g4 * 4 + r) * C::LD + jt * 16 + l16];
  };
  if (wave == 2) put(slot0);
  if (wave == 3) put(slot1);
  __syncthreads();
  if (wave == 0) add(slot0);
  if (wave == 1) add(slot1);
  __syncthreads();
  if (wave == 1) put(slot0);
  __syncthreads();
  if (wave == 0) {  // every lane reads and writes its own positions
    add(slot0);
    put(slot0);
  }
  __syncthreads();
}

// a = softmax(tau * c) of one row spread over four lanes (lane bits 0 and 1)
template <int D>
__device__ __forceinline__ void softmax_row(const float (&c)[D / 4], float tau, float (&a)[D / 4]) {
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < D / 4; ++e) m = fmaxf(m, tau * c[e]);
  m = fmaxf(m, __shfl_xor(m, 1, WAVE_SIZE));
  m = fmaxf(m, __shfl_xor(m, 2, WAVE_SIZE));
  float l = 0.f;
#pragma unroll
  for (int e = 0; e < D / 4; ++e) {
    a[e] = __expf(tau * c[e] - m);
    l += a[e];
  }
  l += __shfl_xor(l, 1, WAVE_SIZE);
  l += __shfl_xor(l, 2, WAVE_SIZE);
  const float inv_l = 1.f / l;
#pragma unroll
  for (int e = 0; e < D / 4; ++e) a[e] *= inv_l;
}

// A d x d matrix as MFMA A operands, one set per 16-row output tile, bf16.
template <int D>
struct MatFrags {
  bf16x8_t full[Cfg<D>::NT][Cfg<D>::KF];
  short4_t tail[Cfg<D>::NT];
};

// Rows of M (TRANS: of M^T) from the fp32 [D][LD] matrix m: lane l16 holds row
// t*16 + l16, reduction indices s*32 + g4*8.. (tail: KF*32 + g4*4..).
template <int D, bool TRANS>
__device__ __forceinline__ void load_mat_frags(const float* m, int l16, int g4, MatFrags<D>& f) {
  using C = Cfg<D>;
#pragma unroll
  for (int t = 0; t < C::NT; ++t) {
    const int r = t * 16 + l16;
#pragma unroll
    for (int s = 0; s < C::KF; ++s) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = s * 32 + g4 * 8 + e;
        f.full[t][s][e] = (__bf16)(TRANS ? m[k * C::LD + r] : m[r * C::LD + k]);
      }
    }
    if (C::kTail) {
      bf16x4_t v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = C::KF * 32 + g4 * 4 + e;
        v[e] = (__bf16)(TRANS ? m[k * C::LD + r] : m[r * C::LD + k]);
      }
      f.tail[t] = __builtin_bit_cast(short4_t, v);
    }
  }
}

// One token row (D channels at p) as MFMA B operands; zeros when !valid.
template <int D>
struct RowFrags {
  bf16x8_t full[Cfg<D>::KF];
  short4_t tail;
};

template <int D>
__device__ __forceinline__ void load_row_frags(const __bf16* p, bool valid, int g4, RowFrags<D>& f) {
  using C = Cfg<D>;
#pragma unroll
  for (int s = 0; s < C::KF; ++s) {
    f.full[s] = bf16x8_t{};
    if (valid) f.full[s] = load_row(p + s * 32 + g4 * 8);
  }
  f.tail = short4_t{};
  if (C::kTail && valid) f.tail = *reinterpret_cast<const short4_t*>(p + C::KF * 32 + g4 * 4);
}

// [rows t*16 + g4*4 + r of M][token l16] = M x.  The 16-wide tail step has an
// accumulator of its own and is added on the VALU, so that no MFMA takes the
// result of an MFMA of another shape as its SrcC: see the note at contract_d
// in attention_head_dims.hip.
template <int D>
__device__ __forceinline__ f32x4 mat_row(const MatFrags<D>& a, int t, const RowFrags<D>& b) {
  using C = Cfg<D>;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < C::KF; ++s) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.full[t][s], b.full[s], acc, 0, 0, 0);
  }
  if (C::kTail) {
    acc += __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
        a.tail[t], b.tail, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
  return acc;
}

__device__ __forceinline__ void store_quad(__bf16* p, const f32x4& v) {
  bf16x4_t o4;
#pragma unroll
  for (int r = 0; r < 4; ++r) o4[r] = (__bf16)v[r];
  *reinterpret_cast<bf16x4_t*>(p) = o4;
}

template <int D>
__global__ __launch_bounds__(kThreads)
void xca_fwd_kernel(
    const __bf16* __restrict__ qkv,          // [B,N,3,H,D]
    const float* __restrict__ temperature,   // [H]
    __bf16* __restrict__ o,                  // [B,N,H,D]
    float* __restrict__ c_save,              // [B,H,D,D]
    float* __restrict__ inv_save,            // [B,H,2,D]
    int N, int H) {
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) char smem[C::SMEM];
  __shared__ float inv_s[2 * D];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const long HD = (long)H * D;
  const long rs = 3 * HD;
  const __bf16* qbase = qkv + (long)b * N * rs + h * D;
  const float tau = temperature[h];

  // ---- pass 1: G = Q^T K and the sums of squares ----
  f32x4 acc[C::NT][C::NT];
#pragma unroll
  for (int it = 0; it < C::NT; ++it)
#pragma unroll
    for (int jt = 0; jt < C::NT; ++jt) acc[it][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ssq[8] = {}, ssk[8] = {};
  token_gram<D, true>(qbase, rs, qbase + HD, rs, N, smem, smem + C::IMG, acc, ssq, ssk);

  // ---- norms: thread groups summed in group order ----
  float* ssbuf = reinterpret_cast<float*>(smem);  // [2][GRP][D]
  if (tid < C::GRP * C::CH) {
    const int grp = tid / C::CH, ch = tid % C::CH;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ssbuf[grp * D + ch * 8 + e] = ssq[e];
      ssbuf[(C::GRP + grp) * D + ch * 8 + e] = ssk[e];
    }
  }
  __syncthreads();
  if (tid < 2 * D) {
    const int which = tid / D, c = tid - which * D;
    float s = 0.f;
    for (int g = 0; g < C::GRP; ++g) s += ssbuf[(which * C::GRP + g) * D + c];
    const float inv = 1.f / fmaxf(sqrtf(s), kNormEps);
    inv_s[tid] = inv;
    inv_save[(long)bh * 2 * D + tid] = inv;
  }
  __syncthreads();

  float* slot0 = reinterpret_cast<float*>(smem);
  float* slot1 = slot0 + C::MAT;
  reduce_partials<D>(acc, slot0, slot1);

  // ---- d x d stage: C = G / (nq nk^T), A = softmax(tau C); four threads per row ----
  const int row = tid >> 2, sub = tid & 3;
  if (row < D) {  // whole waves
    float c[D / 4], a[D / 4];
    const float invq = inv_s[row];
#pragma unroll
    for (int e = 0; e < D / 4; ++e) {
      const int j = sub + 4 * e;
      c[e] = slot0[row * C::LD + j] * invq * inv_s[D + j];
      c_save[((long)bh * D + row) * D + j] = c[e];
    }
    softmax_row<D>(c, tau, a);
#pragma unroll
    for (int e = 0; e < D / 4; ++e) slot0[row * C::LD + sub + 4 * e] = a[e];
  }
  __syncthreads();

  // ---- pass 2: O[n, :] = A V[n, :], 16-token blocks round-robin ----
  MatFrags<D> fa;
  load_mat_frags<D, false>(slot0, l16, g4, fa);
  const int nblk = (N + 15) >> 4;
  for (int blk = wave; blk < nblk; blk += kWaves) {
    const int n = blk * 16 + l16;
    const bool valid = n < N;
    RowFrags<D> fv;
    load_row_frags<D>(qbase + (long)n * rs + 2 * HD, valid, g4, fv);
    __bf16* op = o + ((long)b * N + n) * HD + h * D + g4 * 4;
#pragma unroll
    for (int it = 0; it < C::NT; ++it) {
      const f32x4 r = mat_row<D>(fa, it, fv);
      if (valid) store_quad(op + it * 16, r);
    }
  }
}

template <int D>
__global__ __launch_bounds__(kThreads)
void xca_bwd_kernel(
    const __bf16* __restrict__ qkv,          // [B,N,3,H,D]
    const __bf16* __restrict__ dout,         // [B,N,H,D]
    const float* __restrict__ temperature,   // [H]
    const float* __restrict__ c_save,        // [B,H,D,D]
    const float* __restrict__ inv_save,      // [B,H,2,D]
    __bf16* __restrict__ dqkv,               // [B,N,3,H,D]
    float* __restrict__ dtau_part,           // [B,H]
    int N, int H) {
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) char smem[C::SMEM];
  __shared__ float inv_s[2 * D];
  __shared__ __attribute__((aligned(16))) float cq_s[D];  // rq / nq^2
  __shared__ __attribute__((aligned(16))) float ck_s[D];  // rk / nk^2
  __shared__ float wsum[kWaves];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh - b * H;
  const long HD = (long)H * D;
  const long rs = 3 * HD;
  const __bf16* qbase = qkv + (long)b * N * rs + h * D;
  const __bf16* dobase = dout + (long)b * N * HD + h * D;
  const float tau = temperature[h];

  // ---- pass 1: dA = dO^T V ----
  f32x4 acc[C::NT][C::NT];
#pragma unroll
  for (int it = 0; it < C::NT; ++it)
#pragma unroll
    for (int jt = 0; jt < C::NT; ++jt) acc[it][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float unused_a[8], unused_b[8];
  token_gram<D, false>(dobase, HD, qbase + 2 * HD, rs, N, smem, smem + C::IMG, acc, unused_a, unused_b);
  if (tid < 2 * D) inv_s[tid] = inv_save[(long)bh * 2 * D + tid];

  float* slot0 = reinterpret_cast<float*>(smem);
  float* slot1 = slot0 + C::MAT;
  reduce_partials<D>(acc, slot0, slot1);  // its barriers publish inv_s

  // ---- d x d stage; four threads per row ----
  const int row = tid >> 2, sub = tid & 3;
  float a[D / 4], w[D / 4];
  float dtau = 0.f;
  if (row < D) {  // whole waves
    float c[D / 4];
    const float invq = inv_s[row];
#pragma unroll
    for (int e = 0; e < D / 4; ++e) c[e] = c_save[((long)bh * D + row) * D + sub + 4 * e];
    softmax_row<D>(c, tau, a);
    float da[D / 4];
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < D / 4; ++e) {
      da[e] = slot0[row * C::LD + sub + 4 * e];
      dot += a[e] * da[e];
    }
    dot += __shfl_xor(dot, 1, WAVE_SIZE);
    dot += __shfl_xor(dot, 2, WAVE_SIZE);
    float rq = 0.f;
#pragma unroll
    for (int e = 0; e < D / 4; ++e) {
      const int j = sub + 4 * e;
      const float ds = a[e] * (da[e] - dot);
      dtau += ds * c[e];
      const float dc = tau * ds;
      const float dcc = dc * c[e];
      rq += dcc;
      w[e] = dc * invq * inv_s[D + j];
      slot0[row * C::LD + j] = dcc;  // this thread's own element of dA
    }
    rq += __shfl_xor(rq, 1, WAVE_SIZE);
    rq += __shfl_xor(rq, 2, WAVE_SIZE);
    if (sub == 0) cq_s[row] = rq * invq * invq;
  }
  dtau = wave_reduce_sum(dtau);
  if (lane == 0) wsum[wave] = dtau;
  __syncthreads();
  if (tid < D) {  // rk: column sums in row order
    float rk = 0.f;
    for (int i = 0; i < D; ++i) rk += slot0[i * C::LD + tid];
    const float invk = inv_s[D + tid];
    ck_s[tid] = rk * invk * invk;
  }
  if (tid == 0) dtau_part[bh] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  __syncthreads();
  if (row < D) {
#pragma unroll
    for (int e = 0; e < D / 4; ++e) {
      slot0[row * C::LD + sub + 4 * e] = a[e];
      slot1[row * C::LD + sub + 4 * e] = w[e];
    }
  }
  __syncthreads();

  // ---- pass 2: dV = A^T dO, dQ = W K - cq o Q, dK = W^T Q - ck o K ----
  MatFrags<D> fat, fw, fwt;
  load_mat_frags<D, true>(slot0, l16, g4, fat);
  load_mat_frags<D, false>(slot1, l16, g4, fw);
  load_mat_frags<D, true>(slot1, l16, g4, fwt);
  const int nblk = (N + 15) >> 4;
  for (int blk = wave; blk < nblk; blk += kWaves) {
    const int n = blk * 16 + l16;
    const bool valid = n < N;
    const __bf16* qp = qbase + (long)n * rs;
    RowFrags<D> fq, fk, fdo;
    load_row_frags<D>(qp, valid, g4, fq);
    load_row_frags<D>(qp + HD, valid, g4, fk);
    load_row_frags<D>(dobase + (long)n * HD, valid, g4, fdo);
    __bf16* dp = dqkv + ((long)b * N + n) * rs + h * D + g4 * 4;
#pragma unroll
    for (int t = 0; t < C::NT; ++t) {
      const int c0 = t * 16 + g4 * 4;
      const f32x4 dv = mat_row<D>(fat, t, fdo);
      f32x4 dq = mat_row<D>(fw, t, fk);
      f32x4 dk = mat_row<D>(fwt, t, fq);
      if (valid) {
        const bf16x4_t q4 = *reinterpret_cast<const bf16x4_t*>(qp + c0);
        const bf16x4_t k4 = *reinterpret_cast<const bf16x4_t*>(qp + HD + c0);
        const f32x4 cq = *reinterpret_cast<const f32x4*>(&cq_s[c0]);
        const f32x4 ck = *reinterpret_cast<const f32x4*>(&ck_s[c0]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dq[r] -= cq[r] * (float)q4[r];
          dk[r] -= ck[r] * (float)k4[r];
        }
        store_quad(dp + t * 16, dq);
        store_quad(dp + HD + t * 16, dk);
        store_quad(dp + 2 * HD + t * 16, dv);
      }
    }
  }
}

struct XcaShape {
  int64_t B, N, H, D;
};

XcaShape xca_shape(const at::Tensor& qkv, const at::Tensor& temperature, int64_t heads) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dim() == 3 && qkv.scalar_type() == at::kBFloat16 &&
              qkv.is_contiguous() && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "xca_attention: qkv must be a contiguous, 16-byte-aligned bf16 [B,N,3*heads*head_dim]");
  TORCH_CHECK(heads >= 1 && qkv.size(2) % (3 * heads) == 0, "xca_attention: qkv channels must be 3*heads*head_dim");
  XcaShape s{qkv.size(0), qkv.size(1), heads, qkv.size(2) / (3 * heads)};
  TORCH_CHECK(s.D == 32 || s.D == 48 || s.D == 64, "xca_attention: head_dim must be 32, 48 or 64");
  TORCH_CHECK(s.N >= 1, "xca_attention: needs at least one token");
  TORCH_CHECK(s.B * s.H < (1L << 31) && s.N < (1L << 31) - kRound, "xca_attention: shape too large");
  TORCH_CHECK(temperature.is_cuda() && temperature.is_contiguous() &&
              temperature.scalar_type() == at::kFloat && temperature.numel() == heads,
              "xca_attention: temperature must be contiguous fp32 with `heads` elements");
  return s;
}

}  // namespace

// qkv [B,N,3*H*D] bf16 -> O [B,N,H*D], the cosines C [B,H,D,D] fp32 and the
// inverse norms of q and k [B,H,2,D] fp32 (both saved for the backward).
std::vector<at::Tensor> xca_attention_fwd(at::Tensor qkv, at::Tensor temperature, int64_t heads) {
  const XcaShape s = xca_shape(qkv, temperature, heads);
  const auto f32 = qkv.options().dtype(at::kFloat);
  at::Tensor o = at::empty({s.B, s.N, s.H * s.D}, qkv.options());
  at::Tensor c = at::empty({s.B, s.H, s.D, s.D}, f32);
  at::Tensor inv = at::empty({s.B, s.H, 2, s.D}, f32);
  if (s.B == 0) return {o, c, inv};
  auto stream = at::hip::getCurrentHIPStream();
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)(s.B * s.H)), dim3(kThreads), 0, stream,
        (const __bf16*)qkv.data_ptr(), temperature.data_ptr<float>(), (__bf16*)o.data_ptr(),
        c.data_ptr<float>(), inv.data_ptr<float>(), (int)s.N, (int)s.H);
  };
  switch (s.D) {
    case 32: run(xca_fwd_kernel<32>); break;
    case 48: run(xca_fwd_kernel<48>); break;
    default: run(xca_fwd_kernel<64>); break;
  }
  HIP_CHECK_LAST();
  return {o, c, inv};
}

// Returns dqkv (qkv's shape) and the d temperature partials [B,H]; the caller
// sums dim 0.
std::vector<at::Tensor> xca_attention_bwd(
    at::Tensor qkv, at::Tensor dout, at::Tensor temperature, at::Tensor c, at::Tensor inv,
    int64_t heads) {
  const XcaShape s = xca_shape(qkv, temperature, heads);
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == at::kBFloat16 && dout.is_contiguous() &&
              dout.dim() == 3 && dout.size(0) == s.B && dout.size(1) == s.N &&
              dout.size(2) == s.H * s.D && reinterpret_cast<uintptr_t>(dout.data_ptr()) % 16 == 0,
              "xca_attention_bwd: dO must be a contiguous, 16-byte-aligned bf16 [B,N,heads*head_dim]");
  TORCH_CHECK(c.is_cuda() && c.is_contiguous() && c.scalar_type() == at::kFloat &&
              c.numel() == s.B * s.H * s.D * s.D,
              "xca_attention_bwd: C must be contiguous fp32 [B,heads,head_dim,head_dim]");
  TORCH_CHECK(inv.is_cuda() && inv.is_contiguous() && inv.scalar_type() == at::kFloat &&
              inv.numel() == s.B * s.H * 2 * s.D,
              "xca_attention_bwd: the inverse norms must be contiguous fp32 [B,heads,2,head_dim]");
  at::Tensor dqkv = at::empty_like(qkv);
  at::Tensor dtau = at::empty({s.B, s.H}, c.options());
  if (s.B == 0) return {dqkv, dtau};
  auto stream = at::hip::getCurrentHIPStream();
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)(s.B * s.H)), dim3(kThreads), 0, stream,
        (const __bf16*)qkv.data_ptr(), (const __bf16*)dout.data_ptr(), temperature.data_ptr<float>(),
        c.data_ptr<float>(), inv.data_ptr<float>(), (__bf16*)dqkv.data_ptr(),
        dtau.data_ptr<float>(), (int)s.N, (int)s.H);
  };
  switch (s.D) {
    case 32: run(xca_bwd_kernel<32>); break;
    case 48: run(xca_bwd_kernel<48>); break;
    default: run(xca_bwd_kernel<64>); break;
  }
  HIP_CHECK_LAST();
  return {dqkv, dtau};
}
