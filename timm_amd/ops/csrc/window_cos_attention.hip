// Cosine windowed attention (SwinV2 W-MSA / SW-MSA) on the un-partitioned
// feature map, forward and backward: bf16, head_dim 32, window area N <= 256,
// gfx950.
//
//   S = logit_scale[h] * q^ k^T + bias[h] + shift_mask,  O = softmax(S) V,
//   q^ = q / max(|q|, 1e-12), k^ likewise (F.normalize).
//
// qkv is the qkv Linear's output on the map, [B, Hf, Wf, 3, heads, 32];
// addressing, window order and the shift-mask labels are those of
// window_attention.hip (token n = i*ww + j of window w sits at the map
// coordinate ((wy*wh + i + sh) mod Hf, (wx*ww + j + sw) mod Wf)), so roll,
// partition, reverse, the two normalisations and the [nW, heads, N, N] mask
// tensor never exist.  The norms are fp32, q^ / k^ are rounded to bf16 once,
// and logit_scale multiplies the fp32 accumulator.
//
// Split of the work.  A window of up to 256 tokens no longer fits one wave
// (64 fp32 logits per lane for a single 16-query block), so one workgroup of
// four waves owns a (window, head) pair:
//  * all 256 threads stage the pair's rows once, four lanes per token (16
//    bytes each; the sum of squares of a row is two shuffles), as swizzled
//    [rows][32] bf16 LDS images, plus the token's map position and mask label;
//  * after ONE barrier the images are read-only.  The waves then take 16-row
//    blocks round-robin and never exchange anything again, so a wave with
//    fewer blocks (N = 144: 9 blocks over 4 waves) or none simply arrives at
//    the end earlier.
//
// Forward (window_cos_fwd_kernel<KP>, KP = 32-key steps compiled in): images
// of K^ and V.  Per 16-query block: Q rows from global memory into operand
// registers, normalised there; S^T = K^ Q^^T with the query on the lane and
// the keys kt*16 + g4*4 + r in 2*KP accumulators; scale, bias (global memory,
// shared by all windows, cache-resident), mask; direct softmax (logits are
// bounded, no running max); P packed to bf16 is the B operand of
// O^T = V^T P^T, V^T by transposed LDS reads.  LSE is written [B*nW, heads, N].
//
// Backward (window_cos_bwd_kernel): images of Q^, dO and K^ (48 KB at
// N = 256; V is only ever read by rows, so it stays in global memory and the
// kernel keeps below 64 KB of LDS), delta = rowsum(dO o O) from the staging
// loads, inverse norms recomputed.  Two read-only phases per wave:
//  A. key tiles round-robin, key on the lane: S = Q^ K^^T, dP = dO V^T,
//     P = exp(S - LSE), dS = P o (dP - delta); dV^T += dO^T P and
//     dK^^T += Q^^T dS with the 16 accumulators of the tile in registers;
//  B. query blocks round-robin, query on the lane: S^T and dP^T again, and
//     dQ^^T = K^^T dS^T straight from the accumulators (the forward's P V
//     pattern), plus the block's share of d logit_scale = sum dS o C.
//  dS is computed twice (7 instead of 5 MFMA per 16x16 block) so that it never
//  crosses LDS and no wave waits for another: no dS image, no barrier inside a
//  pair, no atomics.  Both phases end with the normalisation's backward,
//  dx = (dx^ - x^ (x^ . dx^)) / max(|x|, eps), a 32-dim row dot = two shuffles.
//  Each workgroup writes one d logit_scale partial [B*nW, heads]; the caller
//  sums them (fixed order).
//
// dBias (window_cos_dbias_kernel<KP>): [heads, N, N] fp32 is 64 K values per
// head at N = 256, so it has a kernel of its own: one wave per (head,
// 16-query block, chunk of windows) keeps its 16 x N slice of dS in 2*KP
// accumulators, loops over the windows of its chunk recomputing S^T and dP^T
// from global memory (operand registers, no LDS images), and writes one slab;
// the slabs are summed in slab order.  Same bits every run.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef short short4_t __attribute__((ext_vector_type(4)));
typedef short short8_t __attribute__((ext_vector_type(8)));
typedef int int4_t __attribute__((ext_vector_type(4)));

constexpr float kNegInf = -1e30f;
constexpr float kShiftMask = -100.0f;  // SwinTransformerV2Block.get_attn_mask
constexpr float kNormEps = 1e-12f;     // F.normalize
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * WAVE_SIZE;
constexpr int kD = 32;
constexpr int kMaxRows = 256;
constexpr int kImgBytes = kMaxRows * 64;  // [256 tokens][32 dims] bf16

struct CosGeom {
  int Hf, Wf, wh, ww, sh, sw;
  int nWx, nW;  // windows per map row, per image
  int heads, N;
};

// [rows][32] bf16 image, 64-byte rows of two 32-byte halves; the half is
// flipped on every other 4-row block (layout of window_attention.hip).
__device__ __forceinline__ int img_off(int row, int chunk) {
  return row * 64 + (((chunk >> 1) ^ ((row >> 2) & 1)) << 5) + ((chunk & 1) << 4);
}
// 8-byte piece tp of the 16 dims dt*16.. of a row (transposed reads)
__device__ __forceinline__ int img_tr_off(int row, int dt, int tp) {
  return row * 64 + ((dt ^ ((row >> 2) & 1)) << 5) + (tp << 3);
}
// the four dims dt*16 + g4*4.. of a row: where a C-layout accumulator quad lives
__device__ __forceinline__ int img_quad_off(int row, int dt, int g4) {
  return img_off(row, dt * 2 + (g4 >> 1)) + ((g4 & 1) << 3);
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

__device__ __forceinline__ bf16x8_t lds_b128(const char* lds, int off) {
  return *reinterpret_cast<const bf16x8_t*>(lds + off);
}

__device__ __forceinline__ bf16x8_t load_row(const __bf16* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int shift_region(int c, int size, int win, int shift) {
  if (shift == 0) return 0;
  return c < size - win ? 0 : (c < size - shift ? 1 : 2);
}

// Map position (token index into [B*Hf*Wf], -1 beyond the window area) and
// mask label of token n of global window wg.
__device__ __forceinline__ void token_of(const CosGeom& g, int wg, int n, int& pos, int& label) {
  const int b = wg / g.nW;
  const int w = wg - b * g.nW;
  const int wy = w / g.nWx;
  const int wx = w - wy * g.nWx;
  const int ti = n / g.ww;
  const int tj = n - ti * g.ww;
  const int yp = wy * g.wh + ti;
  const int xp = wx * g.ww + tj;
  int y = yp + g.sh;
  if (y >= g.Hf) y -= g.Hf;
  int x = xp + g.sw;
  if (x >= g.Wf) x -= g.Wf;
  pos = n < g.N ? (b * g.Hf + y) * g.Wf + x : -1;
  label = n < g.N ? 3 * shift_region(yp, g.Hf, g.wh, g.sh) + shift_region(xp, g.Wf, g.ww, g.sw) : 0;
}

// x / max(|x|, eps) of a 32-dim row held as 8 dims in each of four lanes that
// differ in the lane bits kA and kB.  fp32 norm, one rounding to bf16.
template <int kA, int kB>
__device__ __forceinline__ bf16x8_t normalise_row(bf16x8_t x, float& inv) {
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss += (float)x[j] * (float)x[j];
  ss += __shfl_xor(ss, kA, WAVE_SIZE);
  ss += __shfl_xor(ss, kB, WAVE_SIZE);
  inv = 1.f / fmaxf(sqrtf(ss), kNormEps);
  bf16x8_t r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)((float)x[j] * inv);
  return r;
}

// bias[q][key0 .. key0+3] of one head (key0 a multiple of 4), zero outside N
__device__ __forceinline__ f32x4 bias4(const float* __restrict__ bias_h, int q, int key0, int N) {
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (bias_h == nullptr || q >= N || key0 >= N) return b;
  const float* p = bias_h + (long)q * N + key0;
  if ((N & 3) == 0) {
    b = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (key0 + r < N) b[r] = p[r];
    }
  }
  return b;
}

// dx = (dx^ - x^ (x^ . dx^)) * inv for the row on lane l16: acc holds
// dx^[d = dt*16 + g4*4 + r], the x^ image supplies the same dims.
__device__ __forceinline__ void normalise_bwd(const char* img, int row, int g4, float inv,
                                              const f32x4 (&acc)[2], bf16x4_t (&out)[2]) {
  bf16x4_t xh[2];
  float dot = 0.f;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    xh[dt] = *reinterpret_cast<const bf16x4_t*>(img + img_quad_off(row, dt, g4));
#pragma unroll
    for (int r = 0; r < 4; ++r) dot += (float)xh[dt][r] * acc[dt][r];
  }
  dot += __shfl_xor(dot, 16, WAVE_SIZE);
  dot += __shfl_xor(dot, 32, WAVE_SIZE);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[dt][r] = (__bf16)((acc[dt][r] - (float)xh[dt][r] * dot) * inv);
  }
}

template <int KP>
__global__ __launch_bounds__(kThreads)
void window_cos_fwd_kernel(
    const __bf16* __restrict__ qkv,          // [B,Hf,Wf,3,heads,32]
    const float* __restrict__ bias,          // [heads,N,N] or null
    const float* __restrict__ logit_scale,   // [heads]
    __bf16* __restrict__ o,                  // [B,Hf,Wf,heads,32]
    float* __restrict__ lse,                 // [B*nW,heads,N]
    CosGeom g) {
  __shared__ __attribute__((aligned(16))) char k_img[kImgBytes];
  __shared__ __attribute__((aligned(16))) char v_img[kImgBytes];
  __shared__ __attribute__((aligned(16))) int lab_s[kMaxRows];
  __shared__ __attribute__((aligned(16))) int pos_s[kMaxRows];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int tq = l16 >> 2;
  const int tp = l16 & 3;
  const int head = blockIdx.x % g.heads;
  const int wg = blockIdx.x / g.heads;
  const int N = g.N;
  const long HD = (long)g.heads * kD;
  const float* bias_h = bias != nullptr ? bias + (long)head * N * N : nullptr;
  const float ls = logit_scale[head];

  // ---- stage K^ and V: token base + tid/4, dims (tid%4)*8.. ----
  for (int base = 0; base < KP * 32; base += 64) {
    const int n = base + (tid >> 2), c = tid & 3;
    int pos, label;
    token_of(g, wg, n, pos, label);
    bf16x8_t kf = {}, vf = {};
    if (pos >= 0) {
      const __bf16* p = qkv + (long)pos * 3 * HD + HD + head * kD + c * 8;
      kf = load_row(p);
      vf = load_row(p + HD);
    }
    float inv;
    kf = normalise_row<1, 2>(kf, inv);
    *reinterpret_cast<bf16x8_t*>(k_img + img_off(n, c)) = kf;
    *reinterpret_cast<bf16x8_t*>(v_img + img_off(n, c)) = vf;
    if (c == 0) {
      lab_s[n] = label;
      pos_s[n] = pos;
    }
  }
  __syncthreads();

  const int nblk = (N + 15) >> 4;
  for (int qb = wave; qb < nblk; qb += kWaves) {
    const int nq = qb * 16 + l16;
    const int tokq = pos_s[nq];
    const int labq = lab_s[nq];
    bf16x8_t qf = {};
    if (tokq >= 0) qf = load_row(qkv + (long)tokq * 3 * HD + head * kD + g4 * 8);
    float invq;
    qf = normalise_row<16, 32>(qf, invq);

    f32x4 s[2 * KP];
    float m = kNegInf;
#pragma unroll
    for (int kt = 0; kt < 2 * KP; ++kt) {
      const int key0 = kt * 16 + g4 * 4;
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          lds_b128(k_img, img_off(kt * 16 + l16, g4)), qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      const f32x4 b4 = bias4(bias_h, nq, key0, N);
      const int4_t lab4 = *reinterpret_cast<const int4_t*>(&lab_s[key0]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float val = s[kt][r] * ls + b4[r];
        if (lab4[r] != labq) val += kShiftMask;
        if (key0 + r >= N) val = kNegInf;
        s[kt][r] = val;
        m = fmaxf(m, val);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, WAVE_SIZE));
    m = fmaxf(m, __shfl_xor(m, 32, WAVE_SIZE));
    float l = 0.f;
    bf16x8_t pf[KP];
#pragma unroll
    for (int kt = 0; kt < 2 * KP; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (kt * 16 + g4 * 4 + r < N) ? __expf(s[kt][r] - m) : 0.f;
        l += p;
        pf[kt >> 1][(kt & 1) * 4 + r] = (__bf16)p;
      }
    }
    l += __shfl_xor(l, 16, WAVE_SIZE);
    l += __shfl_xor(l, 32, WAVE_SIZE);
    const float inv_l = 1.f / l;
    // O^T = V^T P^T; V^T fragments: dims dt*16 + l16, keys {32j + 4g.., 32j + 16 + 4g..}
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        const int row = j * 32 + g4 * 4 + tq;
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            tr_pair(v_img, img_tr_off(row, dt, tp), img_tr_off(row + 16, dt, tp)), pf[j], acc, 0, 0, 0);
      }
      bf16x4_t o4;
#pragma unroll
      for (int r = 0; r < 4; ++r) o4[r] = (__bf16)(acc[r] * inv_l);
      if (tokq >= 0) {
        *reinterpret_cast<bf16x4_t*>(o + (long)tokq * HD + head * kD + dt * 16 + g4 * 4) = o4;
      }
    }
    if (g4 == 0 && nq < N) lse[((long)wg * g.heads + head) * N + nq] = m + __logf(l);
  }
}

__global__ __launch_bounds__(kThreads)
void window_cos_bwd_kernel(
    const __bf16* __restrict__ qkv,          // [B,Hf,Wf,3,heads,32]
    const __bf16* __restrict__ o,            // [B,Hf,Wf,heads,32]
    const __bf16* __restrict__ dov,          // [B,Hf,Wf,heads,32]
    const float* __restrict__ lse,           // [B*nW,heads,N]
    const float* __restrict__ bias,          // [heads,N,N] or null
    const float* __restrict__ logit_scale,   // [heads]
    __bf16* __restrict__ dqkv,               // [B,Hf,Wf,3,heads,32]
    float* __restrict__ dscale_part,         // [B*nW,heads]
    CosGeom g) {
  __shared__ __attribute__((aligned(16))) char q_img[kImgBytes];
  __shared__ __attribute__((aligned(16))) char do_img[kImgBytes];
  __shared__ __attribute__((aligned(16))) char k_img[kImgBytes];
  __shared__ __attribute__((aligned(16))) float lse_s[kMaxRows];
  __shared__ __attribute__((aligned(16))) float delta_s[kMaxRows];
  __shared__ __attribute__((aligned(16))) float invq_s[kMaxRows];
  __shared__ __attribute__((aligned(16))) float invk_s[kMaxRows];
  __shared__ __attribute__((aligned(16))) int lab_s[kMaxRows];
  __shared__ __attribute__((aligned(16))) int pos_s[kMaxRows];
  __shared__ float wsum[kWaves];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int tq = l16 >> 2;
  const int tp = l16 & 3;
  const int head = blockIdx.x % g.heads;
  const int wg = blockIdx.x / g.heads;
  const int N = g.N;
  const long HD = (long)g.heads * kD;
  const float* bias_h = bias != nullptr ? bias + (long)head * N * N : nullptr;
  const float ls = logit_scale[head];
  const int nt = (N + 15) >> 4;   // 16-row tiles
  const int nsl = (N + 31) >> 5;  // 32-row slices

  // ---- stage Q^, dO, K^, delta, LSE: token base + tid/4, dims (tid%4)*8.. ----
  for (int base = 0; base < nsl * 32; base += 64) {
    const int n = base + (tid >> 2), c = tid & 3;
    int pos, label;
    token_of(g, wg, n, pos, label);
    bf16x8_t qf = {}, kf = {}, dof = {}, of = {};
    if (pos >= 0) {
      const __bf16* p = qkv + (long)pos * 3 * HD + head * kD + c * 8;
      const long po = (long)pos * HD + head * kD + c * 8;
      qf = load_row(p);
      kf = load_row(p + HD);
      dof = load_row(dov + po);
      of = load_row(o + po);
    }
    float invq, invk;
    qf = normalise_row<1, 2>(qf, invq);
    kf = normalise_row<1, 2>(kf, invk);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) d += (float)dof[j] * (float)of[j];
    d += __shfl_xor(d, 1, WAVE_SIZE);
    d += __shfl_xor(d, 2, WAVE_SIZE);
    const int off = img_off(n, c);
    *reinterpret_cast<bf16x8_t*>(q_img + off) = qf;
    *reinterpret_cast<bf16x8_t*>(k_img + off) = kf;
    *reinterpret_cast<bf16x8_t*>(do_img + off) = dof;
    if (c == 0) {
      lab_s[n] = label;
      pos_s[n] = pos;
      delta_s[n] = d;
      invq_s[n] = invq;
      invk_s[n] = invk;
      lse_s[n] = n < N ? lse[((long)wg * g.heads + head) * N + n] : 0.f;
    }
  }
  __syncthreads();

  // ---- phase A: dK, dV of the key tiles kt = wave, wave + 4, .. (key on the lane) ----
  for (int kt = wave; kt < nt; kt += kWaves) {
    const int key = kt * 16 + l16;
    const int tokk = pos_s[key];
    const int labk = lab_s[key];
    const bf16x8_t kf = lds_b128(k_img, img_off(key, g4));
    bf16x8_t vf = {};
    if (tokk >= 0) vf = load_row(qkv + (long)tokk * 3 * HD + 2 * HD + head * kD + g4 * 8);
    f32x4 acc_dk[2], acc_dv[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      acc_dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc_dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int sl = 0; sl < nsl; ++sl) {  // 32 query rows at a time
      bf16x8_t p_frag, ds_frag;
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2) {
        const int q0 = (sl * 2 + q2) * 16 + g4 * 4;
        const int off = img_off((sl * 2 + q2) * 16 + l16, g4);
        const f32x4 acc_s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            lds_b128(q_img, off), kf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const f32x4 acc_dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            lds_b128(do_img, off), vf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        // C layout: q row = q0 + r, key on the lane
        const f32x4 lse_r = *reinterpret_cast<const f32x4*>(&lse_s[q0]);
        const f32x4 delta_r = *reinterpret_cast<const f32x4*>(&delta_s[q0]);
        const int4_t labq = *reinterpret_cast<const int4_t*>(&lab_s[q0]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = key < N && q0 + r < N;
          float s = acc_s[r] * ls;
          if (bias_h != nullptr && valid) s += bias_h[(long)(q0 + r) * N + key];
          if (labq[r] != labk) s += kShiftMask;
          const float p = valid ? __expf(s - lse_r[r]) : 0.f;
          const float ds = p * (acc_dp[r] - delta_r[r]);
          p_frag[q2 * 4 + r] = (__bf16)p;
          ds_frag[q2 * 4 + r] = (__bf16)(ds * ls);
        }
      }
      // dV^T[d][key] += dO^T[d][q] P[q][key], dK^^T[d][key] += Q^^T[d][q] dS[q][key]
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int row = sl * 32 + g4 * 4 + tq;
        const int off0 = img_tr_off(row, dt, tp);
        const int off1 = img_tr_off(row + 16, dt, tp);
        acc_dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            tr_pair(do_img, off0, off1), p_frag, acc_dv[dt], 0, 0, 0);
        acc_dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            tr_pair(q_img, off0, off1), ds_frag, acc_dk[dt], 0, 0, 0);
      }
    }
    // C layout holds [d = dt*16 + g4*4 + r][key]
    bf16x4_t k4[2];
    normalise_bwd(k_img, key, g4, invk_s[key], acc_dk, k4);
    if (tokk >= 0) {
      __bf16* p = dqkv + (long)tokk * 3 * HD + HD + head * kD + g4 * 4;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        bf16x4_t v4;
#pragma unroll
        for (int r = 0; r < 4; ++r) v4[r] = (__bf16)acc_dv[dt][r];
        *reinterpret_cast<bf16x4_t*>(p + dt * 16) = k4[dt];
        *reinterpret_cast<bf16x4_t*>(p + HD + dt * 16) = v4;
      }
    }
  }

  // ---- phase B: dQ of the query blocks qb = wave, wave + 4, .. (query on the lane) ----
  float dsc = 0.f;
  for (int qb = wave; qb < nt; qb += kWaves) {
    const int nq = qb * 16 + l16;
    const int tokq = pos_s[nq];
    const int labq = lab_s[nq];
    const float lse_q = lse_s[nq];
    const float delta_q = delta_s[nq];
    const bf16x8_t qf = lds_b128(q_img, img_off(nq, g4));
    const bf16x8_t dof = lds_b128(do_img, img_off(nq, g4));
    f32x4 acc_dq[2];
    acc_dq[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_dq[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nsl; ++j) {  // 32 keys at a time
      bf16x8_t ds_frag;
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int krow = (j * 2 + h2) * 16 + l16;
        const int key0 = (j * 2 + h2) * 16 + g4 * 4;
        const int tokv = pos_s[krow];
        bf16x8_t vf = {};
        if (tokv >= 0) vf = load_row(qkv + (long)tokv * 3 * HD + 2 * HD + head * kD + g4 * 8);
        const f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            lds_b128(k_img, img_off(krow, g4)), qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            vf, dof, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        // C layout: key = key0 + r, query on the lane
        const f32x4 b4 = bias4(bias_h, nq, key0, N);
        const int4_t lab4 = *reinterpret_cast<const int4_t*>(&lab_s[key0]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = key0 + r < N && nq < N;
          float s = c[r] * ls + b4[r];
          if (lab4[r] != labq) s += kShiftMask;
          const float p = valid ? __expf(s - lse_q) : 0.f;
          const float ds = p * (dp[r] - delta_q);
          dsc += ds * c[r];
          ds_frag[h2 * 4 + r] = (__bf16)(ds * ls);
        }
      }
      // dQ^^T[d][q] += K^^T[d][key] dS^T[key][q]
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int row = j * 32 + g4 * 4 + tq;
        acc_dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            tr_pair(k_img, img_tr_off(row, dt, tp), img_tr_off(row + 16, dt, tp)),
            ds_frag, acc_dq[dt], 0, 0, 0);
      }
    }
    bf16x4_t q4[2];
    normalise_bwd(q_img, nq, g4, invq_s[nq], acc_dq, q4);
    if (tokq >= 0) {
      __bf16* p = dqkv + (long)tokq * 3 * HD + head * kD + g4 * 4;
      *reinterpret_cast<bf16x4_t*>(p) = q4[0];
      *reinterpret_cast<bf16x4_t*>(p + 16) = q4[1];
    }
  }
  // d logit_scale: lanes by shuffle, waves in wave order
  dsc = wave_reduce_sum(dsc);
  if (lane == 0) wsum[wave] = dsc;
  __syncthreads();
  if (tid == 0) {
    dscale_part[(long)wg * g.heads + head] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  }
}

// One wave per (head, 16-query block, chunk of windows): dS of its rows summed
// over the chunk's windows, written as slab [split][head][N][N].
template <int KP>
__global__ __launch_bounds__(WAVE_SIZE)
void window_cos_dbias_kernel(
    const __bf16* __restrict__ qkv, const __bf16* __restrict__ o, const __bf16* __restrict__ dov,
    const float* __restrict__ lse, const float* __restrict__ bias,
    const float* __restrict__ logit_scale,
    float* __restrict__ slabs,               // [nsplit,heads,N,N]
    CosGeom g, int n_win, int chunk) {
  __shared__ __attribute__((aligned(16))) int lab_s[kMaxRows];
  __shared__ __attribute__((aligned(16))) int pos_s[kMaxRows];

  const int lane = threadIdx.x;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int N = g.N;
  const int nt = (N + 15) >> 4;
  const int head = blockIdx.x % g.heads;
  const int qb = (blockIdx.x / g.heads) % nt;
  const int split = blockIdx.x / (g.heads * nt);
  const long HD = (long)g.heads * kD;
  const float* bias_h = bias + (long)head * N * N;
  const float ls = logit_scale[head];
  const int nq = qb * 16 + l16;

  f32x4 acc[2 * KP];
#pragma unroll
  for (int kt = 0; kt < 2 * KP; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int w_end = min((split + 1) * chunk, n_win);
  for (int wg = split * chunk; wg < w_end; ++wg) {
    for (int n = lane; n < KP * 32; n += WAVE_SIZE) {
      int pos, label;
      token_of(g, wg, n, pos, label);
      pos_s[n] = pos;
      lab_s[n] = label;
    }
    wave_lds_sync();
    const int tokq = pos_s[nq];
    const int labq = lab_s[nq];
    bf16x8_t qf = {}, dof = {}, of = {};
    float lse_q = 0.f;
    if (tokq >= 0) {
      const long po = (long)tokq * HD + head * kD + g4 * 8;
      qf = load_row(qkv + (long)tokq * 3 * HD + head * kD + g4 * 8);
      dof = load_row(dov + po);
      of = load_row(o + po);
      lse_q = lse[((long)wg * g.heads + head) * N + nq];
    }
    float invq;
    qf = normalise_row<16, 32>(qf, invq);
    float delta_q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) delta_q += (float)dof[j] * (float)of[j];
    delta_q += __shfl_xor(delta_q, 16, WAVE_SIZE);
    delta_q += __shfl_xor(delta_q, 32, WAVE_SIZE);

#pragma unroll
    for (int kt = 0; kt < 2 * KP; ++kt) {
      if (kt * 16 < N) {  // wave-uniform
        const int key0 = kt * 16 + g4 * 4;
        const int tokk = pos_s[kt * 16 + l16];
        bf16x8_t kf = {}, vf = {};
        if (tokk >= 0) {
          const __bf16* p = qkv + (long)tokk * 3 * HD + HD + head * kD + g4 * 8;
          kf = load_row(p);
          vf = load_row(p + HD);
        }
        float invk;
        kf = normalise_row<16, 32>(kf, invk);
        const f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            vf, dof, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const f32x4 b4 = bias4(bias_h, nq, key0, N);
        const int4_t lab4 = *reinterpret_cast<const int4_t*>(&lab_s[key0]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = key0 + r < N && nq < N;
          float s = c[r] * ls + b4[r];
          if (lab4[r] != labq) s += kShiftMask;
          const float p = valid ? __expf(s - lse_q) : 0.f;
          acc[kt][r] += p * (dp[r] - delta_q);
        }
      }
    }
    wave_lds_sync();  // positions and labels are rewritten by the next window
  }

  if (nq < N) {
    float* row = slabs + (((long)split * g.heads + head) * N + nq) * N;
#pragma unroll
    for (int kt = 0; kt < 2 * KP; ++kt) {
      const int key0 = kt * 16 + g4 * 4;
      if ((N & 3) == 0) {
        if (key0 < N) *reinterpret_cast<f32x4*>(row + key0) = acc[kt];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (key0 + r < N) row[key0 + r] = acc[kt][r];
        }
      }
    }
  }
}

// Sum the slabs in slab order (fixed order -> same bits every run).
__global__ __launch_bounds__(kThreads)
void window_cos_dbias_reduce_kernel(
    const float* __restrict__ slabs, float* __restrict__ out, long n, int nsplit) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int z = 0; z < nsplit; ++z) acc += slabs[(long)z * n + i];
  out[i] = acc;
}

CosGeom cos_geom(const at::Tensor& qkv, int64_t heads, int64_t wh, int64_t ww,
                 int64_t sh, int64_t sw) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dim() == 4 && qkv.scalar_type() == at::kBFloat16 &&
              qkv.is_contiguous() && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "window_cos_attention: qkv must be a contiguous, 16-byte-aligned bf16 [B,Hf,Wf,3*heads*32]");
  const int64_t B = qkv.size(0), Hf = qkv.size(1), Wf = qkv.size(2);
  TORCH_CHECK(heads >= 1 && qkv.size(3) == 3 * heads * kD, "window_cos_attention: head_dim must be 32");
  TORCH_CHECK(wh >= 1 && ww >= 1 && wh * ww <= kMaxRows,
              "window_cos_attention: window area must be <= 256");
  TORCH_CHECK(Hf % wh == 0 && Wf % ww == 0, "window_cos_attention: the map must need no padding");
  TORCH_CHECK(sh >= 0 && sh < wh && sw >= 0 && sw < ww, "window_cos_attention: 0 <= shift < window");
  TORCH_CHECK(B * Hf * Wf < (1L << 31) / 4, "window_cos_attention: map too large");
  CosGeom g;
  g.Hf = (int)Hf; g.Wf = (int)Wf; g.wh = (int)wh; g.ww = (int)ww; g.sh = (int)sh; g.sw = (int)sw;
  g.nWx = (int)(Wf / ww);
  g.nW = (int)((Hf / wh) * (Wf / ww));
  g.heads = (int)heads;
  g.N = (int)(wh * ww);
  return g;
}

const float* cos_bias_ptr(const c10::optional<at::Tensor>& bias, const CosGeom& g) {
  if (!bias.has_value()) return nullptr;
  TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() && bias->scalar_type() == at::kFloat &&
              bias->dim() == 3 && bias->size(0) == g.heads && bias->size(1) == g.N &&
              bias->size(2) == g.N && reinterpret_cast<uintptr_t>(bias->data_ptr()) % 16 == 0,
              "window_cos_attention: bias must be contiguous, 16-byte-aligned fp32 [heads,N,N]");
  return bias->data_ptr<float>();
}

const float* cos_scale_ptr(const at::Tensor& logit_scale, const CosGeom& g) {
  TORCH_CHECK(logit_scale.is_cuda() && logit_scale.is_contiguous() &&
              logit_scale.scalar_type() == at::kFloat && logit_scale.numel() == g.heads,
              "window_cos_attention: logit_scale must be contiguous fp32 with `heads` elements");
  return logit_scale.data_ptr<float>();
}

// 32-key steps compiled into the forward and dBias kernels: 2, 3, 5 or 8
// (N <= 64, 96, 160, 256)
int key_steps(int N) {
  const int need = (N + 31) / 32;
  return need <= 2 ? 2 : need <= 3 ? 3 : need <= 5 ? 5 : 8;
}

}  // namespace

// qkv [B,Hf,Wf,3*heads*32] bf16 -> O [B,Hf,Wf,heads*32] in map layout and
// LSE [B*nW,heads,N] fp32.
std::vector<at::Tensor> window_cos_attention_fwd(
    at::Tensor qkv, c10::optional<at::Tensor> bias, at::Tensor logit_scale, int64_t heads,
    int64_t wh, int64_t ww, int64_t sh, int64_t sw) {
  const CosGeom g = cos_geom(qkv, heads, wh, ww, sh, sw);
  const float* bias_p = cos_bias_ptr(bias, g);
  const float* scale_p = cos_scale_ptr(logit_scale, g);
  const int64_t B = qkv.size(0);
  const int64_t n_win = B * g.nW;
  at::Tensor o = at::empty({B, g.Hf, g.Wf, heads * kD}, qkv.options());
  at::Tensor lse = at::empty({n_win, heads, (int64_t)g.N}, qkv.options().dtype(at::kFloat));
  if (n_win == 0) return {o, lse};
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)(n_win * heads));
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, stream,
        (const __bf16*)qkv.data_ptr(), bias_p, scale_p, (__bf16*)o.data_ptr(),
        lse.data_ptr<float>(), g);
  };
  switch (key_steps(g.N)) {
    case 2: run(window_cos_fwd_kernel<2>); break;
    case 3: run(window_cos_fwd_kernel<3>); break;
    case 5: run(window_cos_fwd_kernel<5>); break;
    default: run(window_cos_fwd_kernel<8>); break;
  }
  HIP_CHECK_LAST();
  return {o, lse};
}

// Returns dqkv (qkv's shape), the d logit_scale partials [B*nW,heads] (the
// caller sums dim 0) and, when `need_dbias`, the fp32 bias gradient
// [heads,N,N].  `nsplit` cuts the B*nW windows into that many chunks for the
// dBias kernel, one slab each.
std::tuple<at::Tensor, at::Tensor, c10::optional<at::Tensor>> window_cos_attention_bwd(
    at::Tensor qkv, at::Tensor o, at::Tensor lse, at::Tensor dout,
    c10::optional<at::Tensor> bias, at::Tensor logit_scale, int64_t heads,
    int64_t wh, int64_t ww, int64_t sh, int64_t sw, bool need_dbias, int64_t nsplit) {
  const CosGeom g = cos_geom(qkv, heads, wh, ww, sh, sw);
  const float* bias_p = cos_bias_ptr(bias, g);
  const float* scale_p = cos_scale_ptr(logit_scale, g);
  const int64_t B = qkv.size(0);
  const int n_win = (int)(B * g.nW);
  auto map_ok = [&](const at::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() &&
           t.dim() == 4 && t.size(0) == B && t.size(1) == g.Hf && t.size(2) == g.Wf &&
           t.size(3) == heads * kD && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  TORCH_CHECK(map_ok(o) && map_ok(dout),
              "window_cos_attention_bwd: O and dO must be contiguous bf16 [B,Hf,Wf,heads*32]");
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() && lse.scalar_type() == at::kFloat &&
              lse.numel() == (int64_t)n_win * heads * g.N,
              "window_cos_attention_bwd: lse must be contiguous fp32 [B*nW,heads,N]");
  TORCH_CHECK(!need_dbias || bias_p != nullptr, "window_cos_attention_bwd: need_dbias without a bias");
  at::Tensor dqkv = at::empty_like(qkv);
  at::Tensor dscale = at::empty({(int64_t)n_win, heads}, lse.options());
  c10::optional<at::Tensor> dbias;
  if (need_dbias) dbias = at::empty_like(*bias);
  if (n_win == 0) {
    if (need_dbias) dbias->zero_();
    return {dqkv, dscale, dbias};
  }
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(window_cos_bwd_kernel, dim3((unsigned)(n_win * heads)), dim3(kThreads), 0, stream,
      (const __bf16*)qkv.data_ptr(), (const __bf16*)o.data_ptr(), (const __bf16*)dout.data_ptr(),
      lse.data_ptr<float>(), bias_p, scale_p, (__bf16*)dqkv.data_ptr(), dscale.data_ptr<float>(), g);
  HIP_CHECK_LAST();
  if (!need_dbias) return {dqkv, dscale, dbias};

  int ns = (int)std::min<int64_t>(std::max<int64_t>(nsplit, 1), n_win);
  const int chunk = cdiv(n_win, ns);
  ns = cdiv(n_win, chunk);  // no empty chunks
  at::Tensor slabs;
  float* slab_p = dbias->data_ptr<float>();
  if (ns > 1) {
    slabs = at::empty({(int64_t)ns * dbias->numel()}, dbias->options());
    slab_p = slabs.data_ptr<float>();
  }
  const dim3 grid((unsigned)(ns * cdiv(g.N, 16) * g.heads));
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(WAVE_SIZE), 0, stream,
        (const __bf16*)qkv.data_ptr(), (const __bf16*)o.data_ptr(), (const __bf16*)dout.data_ptr(),
        lse.data_ptr<float>(), bias_p, scale_p, slab_p, g, n_win, chunk);
  };
  switch (key_steps(g.N)) {
    case 2: run(window_cos_dbias_kernel<2>); break;
    case 3: run(window_cos_dbias_kernel<3>); break;
    case 5: run(window_cos_dbias_kernel<5>); break;
    default: run(window_cos_dbias_kernel<8>); break;
  }
  HIP_CHECK_LAST();
  if (ns > 1) {
    const long n = dbias->numel();
    hipLaunchKernelGGL(window_cos_dbias_reduce_kernel,
        dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
        slabs.data_ptr<float>(), dbias->data_ptr<float>(), n, ns);
    HIP_CHECK_LAST();
  }
  return {dqkv, dscale, dbias};
}
