// Windowed (Swin W-MSA / SW-MSA) attention, forward and backward, that reads
// the feature map in place: bf16, head_dim 32, window area N <= 64, gfx950.
//
// qkv is the qkv Linear's output on the un-rolled, un-partitioned map,
// [B, Hf, Wf, 3, heads, 32].  Window w = wy * (Wf/ww) + wx, token n = i*ww + j
// sits at the shifted coordinate (y', x') = (wy*wh + i, wx*ww + j) and at the
// map coordinate (y, x) = ((y' + sh) mod Hf, (x' + sw) mod Wf).  Each lane
// works out the map position and the shift-mask label 3*r_h(y') + r_w(x') of
// ONE token per window (token = lane) and the others fetch them by shuffle:
// roll, partition, reverse and the [nW, heads, N, N] mask tensor never exist.
// O, dQ, dK and dV are written back at (y, x), i.e. already reversed and
// un-shifted.
//
// Split of the work.  A (window, head) pair is one 64x64 tile with a single
// 32-deep MFMA step per 16x16 block: 32 MFMAs forward, 80 backward.  That is
// too little to spread over a workgroup, so ONE WAVE owns a pair from its
// loads to its stores and never waits for another wave.  A workgroup is four
// such waves on the same head, and every wave loops over several windows:
//  * the forward stages the head's bias once per workgroup as a zero-padded
//    [64][68] fp32 LDS image (pitch 68: 16-byte reads by rows without bank
//    conflicts), behind the only barrier of that kernel;
//  * the backward keeps the unscaled dS of all its windows in 64 fp32
//    registers per lane (its LDS is taken by the images below, so it reads
//    the bias, 9.6 KB per head and cache-resident, from global memory with
//    the key on the lane).  After the loop the four waves add their sums in
//    wave order through the then idle images - five barriers per KERNEL -
//    and the workgroup writes one slab [split][head][N][N].  A small kernel
//    sums the slabs in slab order.  No float atomics: same bits every run.
// Per pair there is no workgroup barrier at all.  The LDS images are private
// to a wave, the LDS unit serves one wave's requests in order, and
// wave_lds_sync() only keeps the compiler from reordering around them.
// Registers: the forward and the backward without dBias run at 4 and 2
// waves per SIMD; the 64 dBias accumulators push the dBias variants past 256
// registers, so these are built for 1 wave per SIMD (accumulators in AGPRs,
// no scratch) - see profiles/window_attention/.
//
// Forward (window_attn_fwd_kernel), per pair:
//  * Q, K rows go from global memory straight into MFMA operand registers
//    (16 bytes per lane: token t*16 + l16, dims g4*8..g4*8+7; the row base is
//    the shuffled token position).  V takes the same loads but is written to
//    a swizzled [64][32] LDS image, because P V needs it by columns.
//  * S^T = K Q^T: query on the lane, keys g4*4 + r of four key tiles in the
//    accumulators.  One query's 64 logits are 16 registers of 4 lanes, so
//    max and sum are in-lane loops plus two shuffles: direct softmax, no
//    running max / rescale.  Keys >= N get p = 0.
//  * packed to bf16, the S^T accumulators of two key tiles already are the B
//    operand of O^T = V^T P^T in the key order {4g..4g+3, 16+4g..16+4g+3},
//    which the transposed reads (ds_read_b64_tr_b16) of the V image follow:
//    P never touches LDS.  O^T has the query on the lane and four
//    consecutive dims in a register quad: 8-byte stores at the token's row.
//  * LSE (natural log) is written [B*nW, heads, N].
//
// Backward (window_attn_bwd_kernel), per pair:
//  * K, V row fragments live in registers (B operands of S = Q K^T and
//    dP = dO V^T, key on the lane).  Q, dO and K also go to LDS images:
//    Q / dO are read by rows for S / dP and by columns for dK^T / dV^T; K is
//    read once by columns into K^T fragments (registers), after which its
//    image is reused for dS.
//  * delta = rowsum(dO o O) comes from the same 16-byte loads (8 products per
//    lane, two shuffles): no preprocess launch, no contiguous dO copy.
//  * the 16-key tile is the outer loop, so only that tile's dK^T / dV^T
//    accumulators (16 registers) are live, and they are stored when the tile
//    is done.  Per tile and 32-query slice: S, dP, P = exp(S - LSE),
//    dS = P o (dP - delta), each once.  The C-layout accumulators of two
//    query tiles, packed, are the B operand of dV^T += dO^T P and
//    dK^T += Q^T dS.
//  * dS crosses LDS once, as two [64 keys][32 q] slice images, and comes back
//    by transposed reads as the B operand of dQ^T = K^T dS^T, so dQ too has
//    the query on the lane and leaves in 8-byte stores.
//  * dQ, dK, dV go into one packed dqkv buffer of qkv's shape; without
//    padding every element is written exactly once.
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
constexpr float kShiftMask = -100.0f;  // SwinTransformerBlock.get_attn_mask
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * WAVE_SIZE;
constexpr int kD = 32;
constexpr int kBiasPitch = 68;      // fp32 elements per row of the bias image
constexpr int kFwdWindows = 16;     // windows per forward workgroup (4 per wave)
constexpr int kImgBytes = 64 * 64;  // [64 tokens][32 dims] bf16

struct WinGeom {
  int Hf, Wf, wh, ww, sh, sw;
  int nWx, nW;  // windows per map row, per image
  int heads, N;
};

// [64][32] bf16 image, 64-byte rows of two 32-byte halves.  The half is
// flipped on every other 4-row block, so that the 16 rows a transposed read
// takes for one half cover all banks twice instead of half of them four
// times.
__device__ __forceinline__ int img_off(int row, int chunk) {
  return row * 64 + (((chunk >> 1) ^ ((row >> 2) & 1)) << 5) + ((chunk & 1) << 4);
}
// 8-byte piece tp of the 16 dims dt*16.. of a row (transposed reads)
__device__ __forceinline__ int img_tr_off(int row, int dt, int tp) {
  return row * 64 + ((dt ^ ((row >> 2) & 1)) << 5) + (tp << 3);
}
// [64 keys][32 q] bf16 image of dS^T in 8-byte pieces (4 q rows); layout of
// attention_bwd_single_pass.hip.
__device__ __forceinline__ int ds_off(int key, int piece) {
  return key * 64 + ((piece ^ (((key >> 3) & 1) << 2)) << 3);
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

// Orders one wave's LDS writes before its later LDS reads (and the reverse).
// The hardware already serves a wave's LDS requests in order.
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
// mask label of token (ti, tj) of global window wg.
__device__ __forceinline__ void token_of(const WinGeom& g, int wg, int ti, int tj, bool valid,
                                         int& pos, int& label) {
  const int b = wg / g.nW;
  const int w = wg - b * g.nW;
  const int wy = w / g.nWx;
  const int wx = w - wy * g.nWx;
  const int yp = wy * g.wh + ti;
  const int xp = wx * g.ww + tj;
  int y = yp + g.sh;
  if (y >= g.Hf) y -= g.Hf;
  int x = xp + g.sw;
  if (x >= g.Wf) x -= g.Wf;
  pos = valid ? (b * g.Hf + y) * g.Wf + x : -1;
  label = 3 * shift_region(yp, g.Hf, g.wh, g.sh) + shift_region(xp, g.Wf, g.ww, g.sw);
}

// Zero-padded [64][kBiasPitch] image of one head's bias; ends with the
// workgroup barrier that makes it visible.
__device__ __forceinline__ void stage_bias(float* bias_s, const float* __restrict__ bias,
                                           int head, int N, int tid) {
  for (int idx = tid; idx < 64 * 64; idx += kThreads) {
    const int qrow = idx >> 6, key = idx & 63;
    float val = 0.f;
    if (bias != nullptr && qrow < N && key < N) val = bias[((long)head * N + qrow) * N + key];
    bias_s[qrow * kBiasPitch + key] = val;
  }
  __syncthreads();
}

__device__ __forceinline__ bf16x8_t load_row(const __bf16* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}

template <bool kShift>
__global__ __launch_bounds__(kThreads)
void window_attn_fwd_kernel(
    const __bf16* __restrict__ qkv,   // [B,Hf,Wf,3,heads,32]
    const float* __restrict__ bias,   // [heads,N,N] or null
    __bf16* __restrict__ o,           // [B,Hf,Wf,heads,32]
    float* __restrict__ lse,          // [B*nW,heads,N]
    WinGeom g, int n_win, float scale) {
  __shared__ __attribute__((aligned(16))) float bias_s[64 * kBiasPitch];
  __shared__ __attribute__((aligned(16))) char v_imgs[kWaves][kImgBytes];
  __shared__ __attribute__((aligned(16))) int lab_all[kWaves][64];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int tq = l16 >> 2;  // transposed read: row of the 4-row block
  const int tp = l16 & 3;   // transposed read: 8-byte piece of the 16 columns
  const int head = blockIdx.x % g.heads;
  const int grp = blockIdx.x / g.heads;
  const int N = g.N;
  const long HD = (long)g.heads * kD;

  stage_bias(bias_s, bias, head, N, tid);

  char* v_img = v_imgs[wave];
  int* lab_s = lab_all[wave];
  const int ti = lane / g.ww;
  const int tj = lane - ti * g.ww;
  const int w_end = min((grp + 1) * kFwdWindows, n_win);

  for (int wg = grp * kFwdWindows + wave; wg < w_end; wg += kWaves) {
    int pos, label;
    token_of(g, wg, ti, tj, lane < N, pos, label);
    int tok[4], labq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      tok[t] = __shfl(pos, t * 16 + l16, WAVE_SIZE);
      labq[t] = kShift ? __shfl(label, t * 16 + l16, WAVE_SIZE) : 0;
    }
    if (kShift) lab_s[lane] = label;

    bf16x8_t qf[4], kf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf16x8_t vf = {};
      qf[t] = bf16x8_t{};
      kf[t] = bf16x8_t{};
      if (tok[t] >= 0) {
        const __bf16* p = qkv + (long)tok[t] * 3 * HD + head * kD + g4 * 8;
        qf[t] = load_row(p);
        kf[t] = load_row(p + HD);
        vf = load_row(p + 2 * HD);
      }
      *reinterpret_cast<bf16x8_t*>(v_img + img_off(t * 16 + l16, g4)) = vf;
    }
    wave_lds_sync();

    // V^T fragments: dims dt*16 + l16, keys {32j + 4g.., 32j + 16 + 4g..}
    bf16x8_t vt[2][2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = j * 32 + g4 * 4 + tq;
        vt[dt][j] = tr_pair(v_img, img_tr_off(row, dt, tp), img_tr_off(row + 16, dt, tp));
      }
    }

#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const int nq = qt * 16 + l16;
      f32x4 s[4];
      float m = kNegInf;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            kf[kt], qf[qt], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(
            &bias_s[nq * kBiasPitch + kt * 16 + g4 * 4]);
        int4_t lab4 = {0, 0, 0, 0};
        if (kShift) lab4 = *reinterpret_cast<const int4_t*>(&lab_s[kt * 16 + g4 * 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float val = s[kt][r] * scale + b4[r];
          if (kShift && lab4[r] != labq[qt]) val += kShiftMask;
          if (kt * 16 + g4 * 4 + r >= N) val = kNegInf;
          s[kt][r] = val;
          m = fmaxf(m, val);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16, WAVE_SIZE));
      m = fmaxf(m, __shfl_xor(m, 32, WAVE_SIZE));
      float l = 0.f;
      bf16x8_t pf[2];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
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
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vt[dt][j], pf[j], acc, 0, 0, 0);
        }
        // C layout: query on the lane, dims dt*16 + g4*4 + r
        bf16x4_t o4;
#pragma unroll
        for (int r = 0; r < 4; ++r) o4[r] = (__bf16)(acc[r] * inv_l);
        if (tok[qt] >= 0) {
          *reinterpret_cast<bf16x4_t*>(
              o + (long)tok[qt] * HD + head * kD + dt * 16 + g4 * 4) = o4;
        }
      }
      if (g4 == 0 && nq < N) {
        lse[((long)wg * g.heads + head) * N + nq] = m + __logf(l);
      }
    }
    wave_lds_sync();  // V image and labels are rewritten by the next window
  }
}

template <bool kShift, bool kDbias>
__global__ __launch_bounds__(kThreads, kDbias ? 1 : 2)
void window_attn_bwd_kernel(
    const __bf16* __restrict__ qkv,   // [B,Hf,Wf,3,heads,32]
    const __bf16* __restrict__ o,     // [B,Hf,Wf,heads,32]
    const __bf16* __restrict__ dov,   // [B,Hf,Wf,heads,32]
    const float* __restrict__ lse,    // [B*nW,heads,N]
    const float* __restrict__ bias,   // [heads,N,N] or null
    __bf16* __restrict__ dqkv,        // [B,Hf,Wf,3,heads,32]
    float* __restrict__ slabs,        // [nsplit,heads,N,N] (kDbias)
    WinGeom g, int n_win, int chunk, float scale) {
  // per wave: Q, dO, and dS^T as two [64 keys][32 q] slices; the K image lies
  // on the first dS slice
  __shared__ __attribute__((aligned(16))) char imgs[kWaves][4][kImgBytes];
  __shared__ __attribute__((aligned(16))) float lse_all[kWaves][64];
  __shared__ __attribute__((aligned(16))) float delta_all[kWaves][64];
  __shared__ __attribute__((aligned(16))) int lab_all[kWaves][64];
  static_assert(sizeof(imgs) >= 64 * kBiasPitch * sizeof(float), "dBias sum image");

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int tq = l16 >> 2;
  const int tp = l16 & 3;
  const int head = blockIdx.x % g.heads;
  const int split = blockIdx.x / g.heads;
  const int N = g.N;
  const long HD = (long)g.heads * kD;
  const float* bias_h = bias != nullptr ? bias + (long)head * N * N : nullptr;

  char* q_img = imgs[wave][0];
  char* do_img = imgs[wave][1];
  char* ds_img = imgs[wave][2];  // [2 slices][64 keys][32 q]
  float* lse_s = lse_all[wave];
  float* delta_s = delta_all[wave];
  int* lab_s = lab_all[wave];

  // unscaled dS summed over this wave's windows: [q tile][key tile], C layout
  f32x4 acc_db[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) acc_db[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int ti = lane / g.ww;
  const int tj = lane - ti * g.ww;
  const int w_end = min((split + 1) * chunk, n_win);

  for (int wg = split * chunk + wave; wg < w_end; wg += kWaves) {
    int pos, label;
    token_of(g, wg, ti, tj, lane < N, pos, label);
    int tok[4], labk[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      tok[t] = __shfl(pos, t * 16 + l16, WAVE_SIZE);
      labk[t] = kShift ? __shfl(label, t * 16 + l16, WAVE_SIZE) : 0;
    }
    if (kShift) lab_s[lane] = label;
    // byte offset of bias[g4*4][l16].  Hidden from the compiler once per
    // window, or it keeps all 64 bias addresses of a lane in registers for
    // the whole loop and spills the dBias accumulators.
    int bias_lane = (g4 * 4 * N + l16) * 4;
    __asm__ volatile("" : "+v"(bias_lane));
    lse_s[lane] = lane < N ? lse[((long)wg * g.heads + head) * N + lane] : 0.f;

    // ---- rows of token t*16 + l16, dims g4*8..g4*8+7 ----
    bf16x8_t kf[4], vf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf16x8_t qf = {}, dof = {}, of = {};
      kf[t] = bf16x8_t{};
      vf[t] = bf16x8_t{};
      if (tok[t] >= 0) {
        const __bf16* p = qkv + (long)tok[t] * 3 * HD + head * kD + g4 * 8;
        const long po = (long)tok[t] * HD + head * kD + g4 * 8;
        qf = load_row(p);
        kf[t] = load_row(p + HD);
        vf[t] = load_row(p + 2 * HD);
        dof = load_row(dov + po);
        of = load_row(o + po);
      }
      const int off = img_off(t * 16 + l16, g4);
      *reinterpret_cast<bf16x8_t*>(q_img + off) = qf;
      *reinterpret_cast<bf16x8_t*>(do_img + off) = dof;
      *reinterpret_cast<bf16x8_t*>(ds_img + off) = kf[t];
      // delta = rowsum(dO o O): 8 dims here, the other 24 in the lanes l16 + 16k
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d += (float)dof[j] * (float)of[j];
      d += __shfl_xor(d, 16, WAVE_SIZE);
      d += __shfl_xor(d, 32, WAVE_SIZE);
      if (g4 == 0) delta_s[t * 16 + l16] = d;
      // two token tiles (ten 16-byte loads) in flight at a time: all twenty
      // next to the dBias accumulators would spill
      if (t == 1) __builtin_amdgcn_sched_barrier(0);
    }
    wave_lds_sync();

    // K^T fragments: dims dt*16 + l16, keys 32s + 8g .. 32s + 8g + 7
    bf16x8_t ktr[2][2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int row = s * 32 + g4 * 8 + tq;
        ktr[dt][s] = tr_pair(ds_img, img_tr_off(row, dt, tp), img_tr_off(row + 4, dt, tp));
      }
    }
    wave_lds_sync();  // the K image becomes the first dS slice

#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int key = kt * 16 + l16;
      f32x4 acc_dk[2], acc_dv[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        acc_dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc_dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) {  // 32 query rows at a time
        bf16x8_t p_frag, ds_frag;
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
          const int qt = sl * 2 + q2;
          const int off = img_off(qt * 16 + l16, g4);
          const f32x4 acc_s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              lds_b128(q_img, off), kf[kt], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          const f32x4 acc_dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              lds_b128(do_img, off), vf[kt], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          // C layout: q row = qt*16 + g4*4 + r, key on the lane
          const f32x4 lse_r = *reinterpret_cast<const f32x4*>(&lse_s[qt * 16 + g4 * 4]);
          const f32x4 delta_r = *reinterpret_cast<const f32x4*>(&delta_s[qt * 16 + g4 * 4]);
          int4_t labq = {0, 0, 0, 0};
          if (kShift) labq = *reinterpret_cast<const int4_t*>(&lab_s[qt * 16 + g4 * 4]);
          bf16x4_t ds4;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qrow = qt * 16 + g4 * 4 + r;
            const bool valid = key < N && qrow < N;
            float s = acc_s[r] * scale;
            if (bias_h != nullptr && valid) {
              s += *reinterpret_cast<const float*>(reinterpret_cast<const char*>(bias_h) +
                  (unsigned)(bias_lane + ((qt * 16 + r) * N + kt * 16) * 4));
            }
            if (kShift && labq[r] != labk[kt]) s += kShiftMask;
            const float p = valid ? __expf(s - lse_r[r]) : 0.f;
            const float dsu = p * (acc_dp[r] - delta_r[r]);
            if (kDbias) acc_db[qt][kt][r] += dsu;
            const float dsv = dsu * scale;
            p_frag[q2 * 4 + r] = (__bf16)p;
            ds_frag[q2 * 4 + r] = (__bf16)dsv;
            ds4[r] = (__bf16)dsv;
          }
          *reinterpret_cast<bf16x4_t*>(ds_img + sl * kImgBytes + ds_off(key, q2 * 4 + g4)) = ds4;
        }
        // dV^T[d][key] += dO^T[d][q] P[q][key], dK^T[d][key] += Q^T[d][q] dS[q][key]
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
        // keep the scheduler from pulling the loads of later tiles up here:
        // with all 16 tiles in flight the dBias accumulators would spill
        __builtin_amdgcn_sched_barrier(0);
      }
      // dK, dV of the key tile: C layout holds [d = dt*16 + g4*4 + r][key]
      if (tok[kt] >= 0) {
        __bf16* p = dqkv + (long)tok[kt] * 3 * HD + HD + head * kD + g4 * 4;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          bf16x4_t k4, v4;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            k4[r] = (__bf16)acc_dk[dt][r];
            v4[r] = (__bf16)acc_dv[dt][r];
          }
          *reinterpret_cast<bf16x4_t*>(p + dt * 16) = k4;
          *reinterpret_cast<bf16x4_t*>(p + HD + dt * 16) = v4;
        }
      }
    }
    wave_lds_sync();  // dS of the pair complete

    // dQ^T[d][q] = K^T[d][key] dS^T[key][q]: query on the lane
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const char* ds_sl = ds_img + (qt >> 1) * kImgBytes;
      const int q2 = qt & 1;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int krow = s * 32 + g4 * 8 + tq;
          const bf16x8_t dst = tr_pair(
              ds_sl, ds_off(krow, q2 * 4 + tp), ds_off(krow + 4, q2 * 4 + tp));
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ktr[dt][s], dst, acc, 0, 0, 0);
        }
        bf16x4_t q4;
#pragma unroll
        for (int r = 0; r < 4; ++r) q4[r] = (__bf16)acc[r];
        if (tok[qt] >= 0) {
          *reinterpret_cast<bf16x4_t*>(
              dqkv + (long)tok[qt] * 3 * HD + head * kD + dt * 16 + g4 * 4) = q4;
        }
      }
    }
    wave_lds_sync();  // images free for the next window
  }

  if (kDbias) {
    // the four waves add their sums in wave order through LDS (the images are idle)
    float* sum_s = reinterpret_cast<float*>(&imgs[0][0][0]);
    __syncthreads();
#pragma unroll 1
    for (int w = 0; w < kWaves; ++w) {
      if (wave == w) {
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* dst = &sum_s[(qt * 16 + g4 * 4 + r) * kBiasPitch + kt * 16 + l16];
              *dst = (w == 0 ? 0.f : *dst) + acc_db[qt][kt][r];
            }
          }
        }
      }
      __syncthreads();
    }
    float* slab = slabs + ((long)split * g.heads + head) * N * N;
    for (int idx = tid; idx < 64 * 64; idx += kThreads) {
      const int qrow = idx >> 6, key = idx & 63;
      if (qrow < N && key < N) slab[qrow * N + key] = sum_s[qrow * kBiasPitch + key];
    }
  }
}

// Sum the slabs in slab order (fixed order -> same bits every run).
__global__ __launch_bounds__(kThreads)
void window_attn_dbias_reduce_kernel(
    const float* __restrict__ slabs, float* __restrict__ out, long n, int nsplit) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int z = 0; z < nsplit; ++z) acc += slabs[(long)z * n + i];
  out[i] = acc;
}

WinGeom window_geom(const at::Tensor& qkv, int64_t heads, int64_t wh, int64_t ww,
                    int64_t sh, int64_t sw) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dim() == 4 && qkv.scalar_type() == at::kBFloat16 &&
              qkv.is_contiguous() && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "window_attention: qkv must be a contiguous, 16-byte-aligned bf16 [B,Hf,Wf,3*heads*32]");
  const int64_t B = qkv.size(0), Hf = qkv.size(1), Wf = qkv.size(2);
  TORCH_CHECK(heads >= 1 && qkv.size(3) == 3 * heads * kD, "window_attention: head_dim must be 32");
  TORCH_CHECK(wh >= 1 && ww >= 1 && wh * ww <= 64, "window_attention: window area must be <= 64");
  TORCH_CHECK(Hf % wh == 0 && Wf % ww == 0, "window_attention: the map must need no padding");
  TORCH_CHECK(sh >= 0 && sh < wh && sw >= 0 && sw < ww, "window_attention: 0 <= shift < window");
  TORCH_CHECK(B * Hf * Wf < (1L << 31) / 4, "window_attention: map too large");
  WinGeom g;
  g.Hf = (int)Hf; g.Wf = (int)Wf; g.wh = (int)wh; g.ww = (int)ww; g.sh = (int)sh; g.sw = (int)sw;
  g.nWx = (int)(Wf / ww);
  g.nW = (int)((Hf / wh) * (Wf / ww));
  g.heads = (int)heads;
  g.N = (int)(wh * ww);
  return g;
}

const float* bias_ptr(const c10::optional<at::Tensor>& bias, const WinGeom& g) {
  if (!bias.has_value()) return nullptr;
  TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() && bias->scalar_type() == at::kFloat &&
              bias->dim() == 3 && bias->size(0) == g.heads && bias->size(1) == g.N &&
              bias->size(2) == g.N, "window_attention: bias must be contiguous fp32 [heads,N,N]");
  return bias->data_ptr<float>();
}

}  // namespace

// qkv [B,Hf,Wf,3*heads*32] bf16 (the qkv Linear's output on the map) ->
// O [B,Hf,Wf,heads*32] in map layout and LSE [B*nW,heads,N] fp32.
std::vector<at::Tensor> window_attention_fwd(
    at::Tensor qkv, c10::optional<at::Tensor> bias, int64_t heads,
    int64_t wh, int64_t ww, int64_t sh, int64_t sw, double scale) {
  const WinGeom g = window_geom(qkv, heads, wh, ww, sh, sw);
  const float* bias_p = bias_ptr(bias, g);
  const int64_t B = qkv.size(0);
  const int n_win = (int)(B * g.nW);
  at::Tensor o = at::empty({B, g.Hf, g.Wf, heads * kD}, qkv.options());
  at::Tensor lse = at::empty({(int64_t)n_win, heads, (int64_t)g.N},
                             qkv.options().dtype(at::kFloat));
  if (n_win == 0) return {o, lse};
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)(cdiv(n_win, kFwdWindows) * g.heads));
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, stream,
        (const __bf16*)qkv.data_ptr(), bias_p, (__bf16*)o.data_ptr(), lse.data_ptr<float>(),
        g, n_win, (float)scale);
  };
  if (sh != 0 || sw != 0) run(window_attn_fwd_kernel<true>);
  else run(window_attn_fwd_kernel<false>);
  HIP_CHECK_LAST();
  return {o, lse};
}

// Returns dqkv (qkv's shape) and, when `need_dbias`, the fp32 bias gradient
// [heads,N,N].  `nsplit` cuts the B*nW windows of a head into that many
// chunks, one workgroup and (with need_dbias) one slab each.
std::tuple<at::Tensor, c10::optional<at::Tensor>> window_attention_bwd(
    at::Tensor qkv, at::Tensor o, at::Tensor lse, at::Tensor dout,
    c10::optional<at::Tensor> bias, int64_t heads,
    int64_t wh, int64_t ww, int64_t sh, int64_t sw, double scale,
    bool need_dbias, int64_t nsplit) {
  const WinGeom g = window_geom(qkv, heads, wh, ww, sh, sw);
  const float* bias_p = bias_ptr(bias, g);
  const int64_t B = qkv.size(0);
  const int n_win = (int)(B * g.nW);
  auto map_ok = [&](const at::Tensor& t) {
    return t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() &&
           t.dim() == 4 && t.size(0) == B && t.size(1) == g.Hf && t.size(2) == g.Wf &&
           t.size(3) == heads * kD && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  TORCH_CHECK(map_ok(o) && map_ok(dout),
              "window_attention_bwd: O and dO must be contiguous bf16 [B,Hf,Wf,heads*32]");
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() && lse.scalar_type() == at::kFloat &&
              lse.numel() == (int64_t)n_win * heads * g.N,
              "window_attention_bwd: lse must be contiguous fp32 [B*nW,heads,N]");
  TORCH_CHECK(!need_dbias || bias_p != nullptr, "window_attention_bwd: need_dbias without a bias");
  at::Tensor dqkv = at::empty_like(qkv);
  c10::optional<at::Tensor> dbias;
  if (need_dbias) dbias = at::empty_like(*bias);
  if (n_win == 0) {
    if (need_dbias) dbias->zero_();
    return {dqkv, dbias};
  }
  int ns = (int)std::min<int64_t>(std::max<int64_t>(nsplit, 1), n_win);
  const int chunk = cdiv(n_win, ns);
  ns = cdiv(n_win, chunk);  // no empty chunks
  at::Tensor slabs;
  float* slab_p = nullptr;
  if (need_dbias) {
    slab_p = dbias->data_ptr<float>();
    if (ns > 1) {
      slabs = at::empty({(int64_t)ns * dbias->numel()}, dbias->options());
      slab_p = slabs.data_ptr<float>();
    }
  }
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((unsigned)(ns * g.heads));
  auto run = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, stream,
        (const __bf16*)qkv.data_ptr(), (const __bf16*)o.data_ptr(),
        (const __bf16*)dout.data_ptr(), lse.data_ptr<float>(), bias_p,
        (__bf16*)dqkv.data_ptr(), slab_p, g, n_win, chunk, (float)scale);
  };
  const bool shift = sh != 0 || sw != 0;
  if (shift) {
    if (need_dbias) run(window_attn_bwd_kernel<true, true>);
    else run(window_attn_bwd_kernel<true, false>);
  } else {
    if (need_dbias) run(window_attn_bwd_kernel<false, true>);
    else run(window_attn_bwd_kernel<false, false>);
  }
  HIP_CHECK_LAST();
  if (need_dbias && ns > 1) {
    const long n = dbias->numel();
    hipLaunchKernelGGL(window_attn_dbias_reduce_kernel,
        dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
        slabs.data_ptr<float>(), dbias->data_ptr<float>(), n, ns);
    HIP_CHECK_LAST();
  }
  return {dqkv, dbias};
}
