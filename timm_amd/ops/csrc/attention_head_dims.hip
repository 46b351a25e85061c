// Fused attention for head dims that are not multiples of 32 (gfx950, bf16):
// forward, backward preprocess, dQ, dK/dV and dBias for D % 8 == 0, D <= 128,
// D % 32 != 0 (72: so400m ViTs, 80: ViT-H, 88: ViT-g / EVA-giant, 104, 48, ...).
// The kernels in attention.hip / attention_bwd.hip keep every D % 32 == 0 call;
// their host entries hand the other head dims to the launchers at the bottom.
//
// Same math as those kernels (fp32 online softmax and saved LSE, additive fp32
// mask [mB,H|1,Nq,Nk] read as mask[b % mB] with -inf clamped, strided dq/dk/dv,
// dBias slabs summed in a fixed order), different data movement:
//
//  * Kernels are compiled per Dp = round_up(D, 16) in {16, 32, ..., 128}; D is
//    Dp or Dp - 8.  q/k/v/dO are read from HBM through their strides in
//    16-byte chunks, D/8 per row - no padded copy exists anywhere.
//  * LDS rows have pitch Dp + 8 elements.  Columns D..Dp and rows past Nq/Nk
//    are written as zeros whenever a tile is staged, so no MFMA operand ever
//    holds uninitialised LDS, and the half-valid last 16-column fragment of
//    D % 16 == 8 multiplies zeros.
//    Bank arithmetic: the pitch is 2*Dp + 16 bytes = (Dp/8 + 1) 16-byte units,
//    an odd number because Dp/8 is even.  A fragment read is 16 rows x 16 bytes
//    at one column offset (ds_read_b128); row r starts at unit r*odd mod 16,
//    which takes 16 different values for r = 0..15, so the 16 lanes cover the
//    64 four-byte banks exactly once (and any 8 consecutive lanes cover 32
//    banks once).  Dp = 80: pitch 176 B = 44 banks, rows start at banks
//    0,44,24,4,48,28,8,52,32,12,56,36,16,60,40,20.  The transposed images
//    (V^T, K^T, Q^T, dO^T: [Dp][rows + 8]) and the P / dS round-trip buffers
//    have pitches 72 or 40 elements = 9 or 5 units, odd again.  The 8-byte
//    reads of the 16-wide tail step put two 16-lane groups on adjacent 8-byte
//    halves of the same units: 32 lanes x 8 bytes cover 64 banks once.
//    The XOR swizzle of the other kernels needs a power-of-two pitch and is
//    not used here.
//  * The operand that a wave reuses over its whole loop lives in registers,
//    loaded once from HBM in MFMA A-fragment layout: Q in the forward, Q and
//    dO in the dQ and dBias passes, K and V in the dK/dV pass.  Only the
//    streamed side goes through LDS.
//  * Contraction over D (S = Q K^T, dP = dO V^T): Dp/32 steps of
//    v_mfma_f32_16x16x32_bf16 plus, when Dp % 32 == 16, one
//    v_mfma_f32_16x16x16_bf16 step (4 bf16 per lane per operand).  D = 72 and
//    80 cost 80 columns, D = 88 costs 96.
//  * D as output columns (O, dQ, dK, dV): Dp/16 accumulator fragments; every
//    global store is guarded with col < D, because in the BNHD output and in a
//    packed dqkv buffer the next 8 columns belong to another head or tensor.
//
// Work split (256 threads = 4 waves everywhere, wave w owns 16 rows):
//   forward: block = 64 q rows of one (b,h); K / V^T streamed in 64-key tiles.
//   dQ:      block = 64 q rows; K, V, K^T streamed in 32-key tiles.
//   dK/dV:   block = 64 keys; Q, dO, Q^T, dO^T streamed in 32-row tiles.
//   dBias:   block = one 64x64 bias tile, loop over the (b,h) that share it.
// LDS per block, bytes (Dp = 80 / 128; pitch 88 / 136 elements):
//   forward: K 64 x pitch, V^T Dp x 72, P 4 x 16 x 72        32,000 / 45,056
//   dQ:      K, V 32 x pitch, K^T Dp x 40, dS 4 x 16 x 40    22,784 / 32,768
//   dK/dV:   Q, dO 32 x pitch, Q^T, dO^T Dp x 40, P^T, dS^T  34,304 / 48,128
//   dBias:   K, V 64 x pitch                                  22,528 / 34,816
// Registers and workgroups per CU: profiles/attn_head_dims/README.md.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cstdint>
#include <type_traits>
#include "common.h"
#include "attention_head_dims.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kPad = 8;  // elements; makes every pitch an odd number of 16-byte units
constexpr float kNegInf = -1e30f;

// One 16-row operand's share of a lane, in MFMA A/B layout: lane (l16, g4)
// holds columns [s*32 + g4*8, +8) of row l16 for each full step s, and columns
// [Dp-16 + g4*4, +4) for the tail step.
template <int kDp>
struct RowFrags {
  static constexpr int kFull = kDp / 32;
  static constexpr bool kTail = (kDp % 32) == 16;
  bf16x8_t full[kFull > 0 ? kFull : 1];
  bf16x4 tail;
};

// Load a row's fragments from global memory; zeros for an invalid row and for
// columns >= D (D % 8 == 0, so a chunk is wholly inside or wholly outside).
template <int kDp>
__device__ __forceinline__ RowFrags<kDp> load_row_frags(
    const __bf16* row, bool valid, int D, int g4) {
  RowFrags<kDp> a;
  a.full[0] = bf16x8_t{};
#pragma unroll
  for (int s = 0; s < RowFrags<kDp>::kFull; ++s) {
    const int col = s * 32 + g4 * 8;
    a.full[s] = bf16x8_t{};
    if (valid && col < D) a.full[s] = *reinterpret_cast<const bf16x8_t*>(row + col);
  }
  a.tail = bf16x4{0, 0, 0, 0};
  if (RowFrags<kDp>::kTail) {
    const int col = kDp - 16 + g4 * 4;
    if (valid && col < D) a.tail = *reinterpret_cast<const bf16x4*>(row + col);
  }
  return a;
}

// A(row fragments in registers) . B(row `brow` of a row-major LDS tile of pitch
// kDp + kPad), contracted over the kDp columns.  The 16-wide tail step has an
// accumulator of its own and is added on the VALU: the 16x16x32 steps then
// chain through one opcode only, and no MFMA takes the result of an MFMA of
// another shape as its SrcC.  (Chained as SrcC, with the compiler's schedule
// of a few LDS reads between the two opcodes, the sums came out wrong on the
// MI355X in some launches and right in others; the tests that caught it are
// tests/test_attention_head_dims_gpu.py at D = 48, 72, 80, 104.)
template <int kDp>
__device__ __forceinline__ f32x4 contract_d(
    const RowFrags<kDp>& a, const __bf16* b_lds, int brow, int g4) {
  const __bf16* br = b_lds + brow * (kDp + kPad);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < RowFrags<kDp>::kFull; ++s) {
    const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(br + s * 32 + g4 * 8);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.full[s], b, acc, 0, 0, 0);
  }
  if (RowFrags<kDp>::kTail) {
    const bf16x4 b = *reinterpret_cast<const bf16x4*>(br + kDp - 16 + g4 * 4);
    const f32x4 t = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
        a.tail, b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    acc = RowFrags<kDp>::kFull > 0 ? acc + t : t;
  }
  return acc;
}

// Cooperative stage of global rows [base, base + kRows) x kDp columns: row-major
// into lds_r (pitch kDp + kPad) and/or transposed into lds_t ([kDp][kRows +
// kPad]).  One 16-byte global read per chunk; rows >= n_limit and columns >= D
// are written as zeros.
template <int kDp, int kRows, bool kRowMajor, bool kTransposed>
__device__ __forceinline__ void stage(
    __bf16* lds_r, __bf16* lds_t, const __bf16* src, long src_sn,
    int base, int n_limit, int D) {
  constexpr int c8 = kDp / 8;
  for (int c = threadIdx.x; c < kRows * c8; c += kThreads) {
    const int row = c / c8, col = (c % c8) * 8;
    bf16x8_t val = {};
    if (base + row < n_limit && col < D) {
      val = *reinterpret_cast<const bf16x8_t*>(src + (long)(base + row) * src_sn + col);
    }
    if (kRowMajor) {
      *reinterpret_cast<bf16x8_t*>(lds_r + row * (kDp + kPad) + col) = val;
    }
    if (kTransposed) {
#pragma unroll
      for (int j = 0; j < 8; ++j) lds_t[(col + j) * (kRows + kPad) + row] = val[j];
    }
  }
}

// Write a wave's 16 x (kN16*16) C-layout tile into its LDS buffer (pitch
// kN16*16 + kPad) and read it back as the A fragment of k-step `ks`.
template <int kN16>
__device__ __forceinline__ void c_to_lds(__bf16* buf, const float (*frag)[4], int l16, int g4) {
#pragma unroll
  for (int n16 = 0; n16 < kN16; ++n16) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      buf[(g4 * 4 + r) * (kN16 * 16 + kPad) + n16 * 16 + l16] = (__bf16)frag[n16][r];
    }
  }
  __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

template <int kN16>
__device__ __forceinline__ bf16x8_t a_from_lds(const __bf16* buf, int ks, int l16, int g4) {
  return *reinterpret_cast<const bf16x8_t*>(buf + l16 * (kN16 * 16 + kPad) + ks * 32 + g4 * 8);
}

// p of one score: scale, bounds, mask, clamp, exp against the row's lse.
template <bool kHasMask>
__device__ __forceinline__ float masked_score(
    float acc, float scale, bool in_range, const float* mask, long mask_idx) {
  float s = acc * scale;
  if (!in_range) return kNegInf;
  if (kHasMask) {
    s += mask[mask_idx];
    if (s < kNegInf) s = kNegInf;
  }
  return s;
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
template <int kDp, bool kHasMask>
__global__ __launch_bounds__(kThreads)
void attn_hd_fwd_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const float* __restrict__ mask,   // [mB,H|1,Nq,Nk] or null
    __bf16* __restrict__ o,           // [B,Nq,H,D]
    float* __restrict__ lse,          // [B,H,Nq]
    int H, int Nq, int Nk, int D, float scale,
    int mB, long m_sb, long m_sh,
    long q_sb, long q_sh, long q_sn,
    long k_sb, long k_sh, long k_sn,
    long v_sb, long v_sh, long v_sn) {
  constexpr int kKv = 64, kNF = kKv / 16, kPT = kKv + kPad;
  __shared__ __attribute__((aligned(16))) __bf16 k_lds[kKv * (kDp + kPad)];
  __shared__ __attribute__((aligned(16))) __bf16 vt_lds[kDp * kPT];
  __shared__ __attribute__((aligned(16))) __bf16 p_lds[4 * 16 * kPT];

  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int qbase = blockIdx.x * 64;
  const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15, g4 = lane >> 4;
  const __bf16* k_bh = k + (long)b * k_sb + (long)h * k_sh;
  const __bf16* v_bh = v + (long)b * v_sb + (long)h * v_sh;
  __bf16* p_w = p_lds + wave * 16 * kPT;

  const int arow = qbase + wave * 16 + l16;
  const RowFrags<kDp> qa = load_row_frags<kDp>(
      q + (long)b * q_sb + (long)h * q_sh + (long)arow * q_sn, arow < Nq, D, g4);

  float m_run[4], l_run[4];
  f32x4 acc_o[kDp / 16];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = kNegInf; l_run[r] = 0.f; }
#pragma unroll
  for (int f = 0; f < kDp / 16; ++f) acc_o[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long m_off = kHasMask ? (long)(b % mB) * m_sb + (long)h * m_sh : 0;
  for (int kv0 = 0; kv0 < Nk; kv0 += kKv) {
    __syncthreads();  // previous tile's reads done before restage
    stage<kDp, kKv, true, false>(k_lds, nullptr, k_bh, k_sn, kv0, Nk, D);
    stage<kDp, kKv, false, true>(nullptr, vt_lds, v_bh, v_sn, kv0, Nk, D);
    __syncthreads();

    float s_frag[kNF][4], m_tile[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) m_tile[r] = kNegInf;
#pragma unroll
    for (int n16 = 0; n16 < kNF; ++n16) {
      const f32x4 acc = contract_d<kDp>(qa, k_lds, n16 * 16 + l16, g4);
      const int kvcol = kv0 + n16 * 16 + l16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qbase + wave * 16 + g4 * 4 + r;
        const float s = masked_score<kHasMask>(acc[r], scale, kvcol < Nk && qrow < Nq, mask,
                                               m_off + (long)qrow * Nk + kvcol);
        s_frag[n16][r] = s;
        m_tile[r] = fmaxf(m_tile[r], s);
      }
    }

    float factor[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float m_new = fmaxf(m_run[r], group16_reduce_max(m_tile[r]));
      factor[r] = (m_run[r] == kNegInf) ? 0.f : __expf(m_run[r] - m_new);
      m_run[r] = m_new;
      float psum = 0.f;
#pragma unroll
      for (int n16 = 0; n16 < kNF; ++n16) {
        const float p = (s_frag[n16][r] <= kNegInf) ? 0.f : __expf(s_frag[n16][r] - m_new);
        s_frag[n16][r] = p;
        psum += p;
      }
      l_run[r] = l_run[r] * factor[r] + group16_reduce_sum(psum);
    }

    // O = O * factor + P V: P through the wave's LDS buffer into A layout,
    // V^T rows are the B fragments (rows D..Dp of V^T are zero).
    c_to_lds<kNF>(p_w, s_frag, l16, g4);
    const bf16x8_t pa0 = a_from_lds<kNF>(p_w, 0, l16, g4);
    const bf16x8_t pa1 = a_from_lds<kNF>(p_w, 1, l16, g4);
#pragma unroll
    for (int f = 0; f < kDp / 16; ++f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc_o[f][r] *= factor[r];
      const __bf16* vr = vt_lds + (f * 16 + l16) * kPT + g4 * 8;
      acc_o[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pa0, *reinterpret_cast<const bf16x8_t*>(vr), acc_o[f], 0, 0, 0);
      acc_o[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pa1, *reinterpret_cast<const bf16x8_t*>(vr + 32), acc_o[f], 0, 0, 0);
    }
  }

  __bf16* o_bh = o + ((long)b * Nq) * ((long)H * D) + (long)h * D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = qbase + wave * 16 + g4 * 4 + r;
    if (qrow >= Nq) continue;
    const float inv_l = (l_run[r] > 0.f) ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int f = 0; f < kDp / 16; ++f) {
      const int col = f * 16 + l16;
      if (col < D) o_bh[(long)qrow * ((long)H * D) + col] = (__bf16)(acc_o[f][r] * inv_l);
    }
    if (l16 == 0) {
      lse[(long)bh * Nq + qrow] = (l_run[r] > 0.f) ? (m_run[r] + __logf(l_run[r])) : INFINITY;
    }
  }
}

// ---------------------------------------------------------------------------
// Backward preprocess: contiguous copy of strided dO + delta = rowsum(dO o O)
// over the D columns.  lpr lanes (the power of two >= D/8, host-chosen) share
// a row, one 16-byte chunk each.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads)
void attn_hd_bwd_preprocess_kernel(
    const __bf16* __restrict__ dov, const __bf16* __restrict__ ov,  // strided [B,H,N,D]
    __bf16* __restrict__ do_c,       // contiguous [B,H,N,D]
    float* __restrict__ delta,       // [B,H,N]
    long rows, int D, int lpr,
    long do_sb, long do_sh, long do_sn,
    long o_sb, long o_sh, long o_sn, int H, int N) {
  const int rows_per_block = kThreads / lpr;
  const int local_row = threadIdx.x / lpr;
  const int col = (threadIdx.x % lpr) * 8;
  for (long row = (long)blockIdx.x * rows_per_block + local_row; row < rows;
       row += (long)gridDim.x * rows_per_block) {
    const long n = row % N, h = (row / N) % H, b = row / ((long)H * N);
    float acc = 0.f;
    if (col < D) {
      const bf16x8_t dv = *reinterpret_cast<const bf16x8_t*>(
          dov + b * do_sb + h * do_sh + n * do_sn + col);
      const bf16x8_t oval = *reinterpret_cast<const bf16x8_t*>(
          ov + b * o_sb + h * o_sh + n * o_sn + col);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += (float)dv[j] * (float)oval[j];
      *reinterpret_cast<bf16x8_t*>(do_c + row * D + col) = dv;
    }
    for (int off = lpr / 2; off > 0; off /= 2) acc += __shfl_xor(acc, off, 64);
    if (col == 0) delta[row] = acc;
  }
}

// ---------------------------------------------------------------------------
// dQ pass: block owns 64 q rows (Q, dO fragments in registers), loops over
// 32-key tiles:  S, dP -> dS = P o (dP - delta) * scale -> dQ += dS K.
// ---------------------------------------------------------------------------
template <int kDp, bool kHasMask>
__global__ __launch_bounds__(kThreads)
void attn_hd_bwd_dq_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dov,   // contiguous [B,H,Nq,D]
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ mask,
    __bf16* __restrict__ dq,          // strided out
    int H, int Nq, int Nk, int D, float scale,
    int mB, long m_sb, long m_sh,
    long q_sb, long q_sh, long q_sn,
    long k_sb, long k_sh, long k_sn,
    long v_sb, long v_sh, long v_sn,
    long dq_sb, long dq_sh, long dq_sn) {
  constexpr int kKv = 32, kPT = kKv + kPad;
  __shared__ __attribute__((aligned(16))) __bf16 k_lds[kKv * (kDp + kPad)];
  __shared__ __attribute__((aligned(16))) __bf16 v_lds[kKv * (kDp + kPad)];
  __shared__ __attribute__((aligned(16))) __bf16 kt_lds[kDp * kPT];
  __shared__ __attribute__((aligned(16))) __bf16 ds_lds[4 * 16 * kPT];

  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int qbase = blockIdx.x * 64;
  const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15, g4 = lane >> 4;
  const __bf16* k_bh = k + (long)b * k_sb + (long)h * k_sh;
  const __bf16* v_bh = v + (long)b * v_sb + (long)h * v_sh;
  __bf16* ds_w = ds_lds + wave * 16 * kPT;

  const int arow = qbase + wave * 16 + l16;
  const RowFrags<kDp> qa = load_row_frags<kDp>(
      q + (long)b * q_sb + (long)h * q_sh + (long)arow * q_sn, arow < Nq, D, g4);
  const RowFrags<kDp> da = load_row_frags<kDp>(
      dov + ((long)bh * Nq + arow) * D, arow < Nq, D, g4);

  float lse_r[4], delta_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = qbase + wave * 16 + g4 * 4 + r;
    lse_r[r] = (qrow < Nq) ? lse[(long)bh * Nq + qrow] : INFINITY;
    delta_r[r] = (qrow < Nq) ? delta[(long)bh * Nq + qrow] : 0.f;
  }
  f32x4 acc_dq[kDp / 16];
#pragma unroll
  for (int f = 0; f < kDp / 16; ++f) acc_dq[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long m_off = kHasMask ? (long)(b % mB) * m_sb + (long)h * m_sh : 0;
  for (int kv0 = 0; kv0 < Nk; kv0 += kKv) {
    __syncthreads();
    stage<kDp, kKv, true, true>(k_lds, kt_lds, k_bh, k_sn, kv0, Nk, D);
    stage<kDp, kKv, true, false>(v_lds, nullptr, v_bh, v_sn, kv0, Nk, D);
    __syncthreads();

    float ds_frag[2][4];
#pragma unroll
    for (int n16 = 0; n16 < 2; ++n16) {
      const f32x4 acc_s = contract_d<kDp>(qa, k_lds, n16 * 16 + l16, g4);
      const f32x4 acc_dp = contract_d<kDp>(da, v_lds, n16 * 16 + l16, g4);
      const int kvcol = kv0 + n16 * 16 + l16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qbase + wave * 16 + g4 * 4 + r;
        const float s = masked_score<kHasMask>(acc_s[r], scale, kvcol < Nk && qrow < Nq, mask,
                                               m_off + (long)qrow * Nk + kvcol);
        const float p = (s <= kNegInf) ? 0.f : __expf(s - lse_r[r]);
        ds_frag[n16][r] = p * (acc_dp[r] - delta_r[r]) * scale;
      }
    }

    c_to_lds<2>(ds_w, ds_frag, l16, g4);
    const bf16x8_t dsa = a_from_lds<2>(ds_w, 0, l16, g4);
#pragma unroll
    for (int f = 0; f < kDp / 16; ++f) {
      const bf16x8_t kcol = *reinterpret_cast<const bf16x8_t*>(
          kt_lds + (f * 16 + l16) * kPT + g4 * 8);
      acc_dq[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, kcol, acc_dq[f], 0, 0, 0);
    }
  }

  __bf16* dq_bh = dq + (long)b * dq_sb + (long)h * dq_sh;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = qbase + wave * 16 + g4 * 4 + r;
    if (qrow >= Nq) continue;
#pragma unroll
    for (int f = 0; f < kDp / 16; ++f) {
      const int col = f * 16 + l16;
      if (col < D) dq_bh[(long)qrow * dq_sn + col] = (__bf16)acc_dq[f][r];
    }
  }
}

// ---------------------------------------------------------------------------
// dK/dV pass: block owns 64 keys (K, V fragments in registers), loops over
// 32-row q tiles with the transposed products
//   S^T = K Q^T, dP^T = V dO^T,  dV += P^T dO,  dK += dS^T Q.
// ---------------------------------------------------------------------------
template <int kDp, bool kHasMask>
__global__ __launch_bounds__(kThreads)
void attn_hd_bwd_dkdv_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dov,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ mask,
    __bf16* __restrict__ dk, __bf16* __restrict__ dv,
    int H, int Nq, int Nk, int D, float scale,
    int mB, long m_sb, long m_sh,
    long q_sb, long q_sh, long q_sn,
    long k_sb, long k_sh, long k_sn,
    long v_sb, long v_sh, long v_sn,
    long dk_sb, long dk_sh, long dk_sn,
    long dv_sb, long dv_sh, long dv_sn) {
  constexpr int kQ = 32, kPT = kQ + kPad;
  __shared__ __attribute__((aligned(16))) __bf16 q_lds[kQ * (kDp + kPad)];
  __shared__ __attribute__((aligned(16))) __bf16 do_lds[kQ * (kDp + kPad)];
  __shared__ __attribute__((aligned(16))) __bf16 qt_lds[kDp * kPT];
  __shared__ __attribute__((aligned(16))) __bf16 dot_lds[kDp * kPT];
  __shared__ __attribute__((aligned(16))) __bf16 pt_lds[4 * 16 * kPT];
  __shared__ __attribute__((aligned(16))) __bf16 dst_lds[4 * 16 * kPT];

  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int kvbase = blockIdx.x * 64;
  const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15, g4 = lane >> 4;
  const __bf16* q_bh = q + (long)b * q_sb + (long)h * q_sh;
  const __bf16* do_bh = dov + ((long)bh * Nq) * D;
  __bf16* pt_w = pt_lds + wave * 16 * kPT;
  __bf16* dst_w = dst_lds + wave * 16 * kPT;

  const int arow = kvbase + wave * 16 + l16;
  const RowFrags<kDp> ka = load_row_frags<kDp>(
      k + (long)b * k_sb + (long)h * k_sh + (long)arow * k_sn, arow < Nk, D, g4);
  const RowFrags<kDp> va = load_row_frags<kDp>(
      v + (long)b * v_sb + (long)h * v_sh + (long)arow * v_sn, arow < Nk, D, g4);

  f32x4 acc_dk[kDp / 16], acc_dv[kDp / 16];
#pragma unroll
  for (int f = 0; f < kDp / 16; ++f) {
    acc_dk[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_dv[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const long m_off = kHasMask ? (long)(b % mB) * m_sb + (long)h * m_sh : 0;
  for (int q0 = 0; q0 < Nq; q0 += kQ) {
    __syncthreads();
    stage<kDp, kQ, true, true>(q_lds, qt_lds, q_bh, q_sn, q0, Nq, D);
    stage<kDp, kQ, true, true>(do_lds, dot_lds, do_bh, D, q0, Nq, D);
    __syncthreads();

    float pt_frag[2][4], dst_frag[2][4];
#pragma unroll
    for (int n16 = 0; n16 < 2; ++n16) {
      const int qcol = q0 + n16 * 16 + l16;
      const float lse_c = (qcol < Nq) ? lse[(long)bh * Nq + qcol] : INFINITY;
      const float delta_c = (qcol < Nq) ? delta[(long)bh * Nq + qcol] : 0.f;
      const f32x4 acc_s = contract_d<kDp>(ka, q_lds, n16 * 16 + l16, g4);
      const f32x4 acc_dp = contract_d<kDp>(va, do_lds, n16 * 16 + l16, g4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kvrow = kvbase + wave * 16 + g4 * 4 + r;
        const float s = masked_score<kHasMask>(acc_s[r], scale, kvrow < Nk && qcol < Nq, mask,
                                               m_off + (long)qcol * Nk + kvrow);
        const float p = (s <= kNegInf) ? 0.f : __expf(s - lse_c);
        pt_frag[n16][r] = p;
        dst_frag[n16][r] = p * (acc_dp[r] - delta_c) * scale;
      }
    }

    c_to_lds<2>(pt_w, pt_frag, l16, g4);
    c_to_lds<2>(dst_w, dst_frag, l16, g4);
    const bf16x8_t pa = a_from_lds<2>(pt_w, 0, l16, g4);
    const bf16x8_t dsa = a_from_lds<2>(dst_w, 0, l16, g4);
#pragma unroll
    for (int f = 0; f < kDp / 16; ++f) {
      const int t = (f * 16 + l16) * kPT + g4 * 8;
      acc_dv[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pa, *reinterpret_cast<const bf16x8_t*>(dot_lds + t), acc_dv[f], 0, 0, 0);
      acc_dk[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          dsa, *reinterpret_cast<const bf16x8_t*>(qt_lds + t), acc_dk[f], 0, 0, 0);
    }
  }

  __bf16* dk_bh = dk + (long)b * dk_sb + (long)h * dk_sh;
  __bf16* dv_bh = dv + (long)b * dv_sb + (long)h * dv_sh;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kvrow = kvbase + wave * 16 + g4 * 4 + r;
    if (kvrow >= Nk) continue;
#pragma unroll
    for (int f = 0; f < kDp / 16; ++f) {
      const int col = f * 16 + l16;
      if (col < D) {
        dk_bh[(long)kvrow * dk_sn + col] = (__bf16)acc_dk[f][r];
        dv_bh[(long)kvrow * dv_sn + col] = (__bf16)acc_dv[f][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dBias pass: block owns one (m, h', 64 q rows, 64 keys) tile of the bias
// gradient and sums the unscaled dS = P o (dP - delta) in fp32 over chunk
// blockIdx.z of the (b, h) pairs that share it; plain stores into slab z.
// ---------------------------------------------------------------------------
template <int kDp>
__global__ __launch_bounds__(kThreads)
void attn_hd_bwd_dbias_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dov,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ mask,   // [mB,Hm,Nq,Nk] contiguous
    float* __restrict__ out,          // [nsplit,mB,Hm,Nq,Nk]
    int H, int Nq, int Nk, int D, float scale,
    int mB, int Hm, int n_kt, int n_red, int chunk,
    long q_sb, long q_sh, long q_sn,
    long k_sb, long k_sh, long k_sn,
    long v_sb, long v_sh, long v_sn) {
  constexpr int kTile = 64;
  __shared__ __attribute__((aligned(16))) __bf16 k_lds[kTile * (kDp + kPad)];
  __shared__ __attribute__((aligned(16))) __bf16 v_lds[kTile * (kDp + kPad)];

  const int tiles = gridDim.x / (mB * Hm);
  const int tile = blockIdx.x % tiles, mh = blockIdx.x / tiles;
  const int m = mh / Hm, hm = mh % Hm;
  const int qbase = (tile / n_kt) * kTile, kvbase = (tile % n_kt) * kTile;
  const int nh = (Hm == 1) ? H : 1;
  const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int arow = qbase + wave * 16 + l16;

  const long mh_off = (long)mh * Nq * Nk;
  float bias_r[4][4];
  f32x4 acc[4];
#pragma unroll
  for (int n16 = 0; n16 < 4; ++n16) {
    acc[n16] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kvcol = kvbase + n16 * 16 + l16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qbase + wave * 16 + g4 * 4 + r;
      bias_r[n16][r] = (qrow < Nq && kvcol < Nk) ? mask[mh_off + (long)qrow * Nk + kvcol] : 0.f;
    }
  }

  const int r_end = min(n_red, (int)blockIdx.z * chunk + chunk);
  for (int ri = blockIdx.z * chunk; ri < r_end; ++ri) {
    const int b = m + (ri / nh) * mB;
    const int h = (Hm == 1) ? (ri % nh) : hm;
    const long bh = (long)b * H + h;
    const RowFrags<kDp> qa = load_row_frags<kDp>(
        q + (long)b * q_sb + (long)h * q_sh + (long)arow * q_sn, arow < Nq, D, g4);
    const RowFrags<kDp> da = load_row_frags<kDp>(
        dov + (bh * Nq + arow) * D, arow < Nq, D, g4);
    float lse_r[4], delta_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qbase + wave * 16 + g4 * 4 + r;
      lse_r[r] = (qrow < Nq) ? lse[bh * Nq + qrow] : INFINITY;
      delta_r[r] = (qrow < Nq) ? delta[bh * Nq + qrow] : 0.f;
    }

    __syncthreads();
    stage<kDp, kTile, true, false>(k_lds, nullptr, k + (long)b * k_sb + (long)h * k_sh, k_sn,
                                   kvbase, Nk, D);
    stage<kDp, kTile, true, false>(v_lds, nullptr, v + (long)b * v_sb + (long)h * v_sh, v_sn,
                                   kvbase, Nk, D);
    __syncthreads();

#pragma unroll
    for (int n16 = 0; n16 < 4; ++n16) {
      const f32x4 acc_s = contract_d<kDp>(qa, k_lds, n16 * 16 + l16, g4);
      const f32x4 acc_dp = contract_d<kDp>(da, v_lds, n16 * 16 + l16, g4);
      const int kvcol = kvbase + n16 * 16 + l16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qbase + wave * 16 + g4 * 4 + r;
        float s = kNegInf;
        if (kvcol < Nk && qrow < Nq) s = fmaxf(acc_s[r] * scale + bias_r[n16][r], kNegInf);
        const float p = (s <= kNegInf) ? 0.f : __expf(s - lse_r[r]);
        acc[n16][r] += p * (acc_dp[r] - delta_r[r]);
      }
    }
  }

  float* out_t = out + ((long)blockIdx.z * mB * Hm + mh) * Nq * Nk;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = qbase + wave * 16 + g4 * 4 + r;
    if (qrow >= Nq) continue;
#pragma unroll
    for (int n16 = 0; n16 < 4; ++n16) {
      const int kvcol = kvbase + n16 * 16 + l16;
      if (kvcol < Nk) out_t[(long)qrow * Nk + kvcol] = acc[n16][r];
    }
  }
}

// ---- host side ----

// Calls f(std::integral_constant<int, Dp>) for Dp = round_up(D, 16).
template <typename F>
void dispatch_dp(int D, F&& f) {
  switch ((D + 15) / 16) {
    case 1: f(std::integral_constant<int, 16>{}); break;
    case 2: f(std::integral_constant<int, 32>{}); break;
    case 3: f(std::integral_constant<int, 48>{}); break;
    case 4: f(std::integral_constant<int, 64>{}); break;
    case 5: f(std::integral_constant<int, 80>{}); break;
    case 6: f(std::integral_constant<int, 96>{}); break;
    case 7: f(std::integral_constant<int, 112>{}); break;
    case 8: f(std::integral_constant<int, 128>{}); break;
    default: TORCH_CHECK(false, "attention: head_dim ", D, " out of range");
  }
}

// The kernels move 16-byte chunks through the tensors' own strides: the base
// must be 16-byte aligned and every stride that is stepped a multiple of 8.
void check_chunks(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1, "attention: ", name, ": head_dim stride must be 1");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "attention: ", name, " must be 16-byte aligned");
  for (int d = 0; d < 3; ++d) {
    TORCH_CHECK(t.size(d) <= 1 || t.stride(d) % 8 == 0,
                "attention: ", name, ": stride ", d, " must be a multiple of 8 elements");
  }
}

struct MaskArgs {
  const float* ptr = nullptr;
  int mB = 1;
  long sb = 0, sh = 0;
};

MaskArgs mask_args(const c10::optional<at::Tensor>& mask, int Nq, int Nk) {
  MaskArgs mi;
  if (mask.has_value()) {
    mi.ptr = mask->data_ptr<float>();
    mi.mB = (int)mask->size(0);
    mi.sb = mi.mB == 1 ? 0 : mask->size(1) * (long)Nq * Nk;
    mi.sh = mask->size(1) == 1 ? 0 : (long)Nq * Nk;
  }
  return mi;
}

}  // namespace

std::vector<at::Tensor> attention_fwd_head_dims(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const c10::optional<at::Tensor>& mask, double scale) {
  const int B = q.size(0), H = q.size(1), Nq = q.size(2), D = q.size(3), Nk = k.size(2);
  TORCH_CHECK(D % 8 == 0 && D >= 8 && D <= 128, "attention_fwd: head_dim must be a multiple of 8, <=128");
  TORCH_CHECK(k.dim() == 4 && v.dim() == 4 && k.size(0) == B && k.size(1) == H && k.size(3) == D &&
              v.size(0) == B && v.size(1) == H && v.size(2) == Nk && v.size(3) == D &&
              k.scalar_type() == at::kBFloat16 && v.scalar_type() == at::kBFloat16,
              "attention_fwd: q/k/v shapes or dtypes disagree");
  check_chunks(q, "q"); check_chunks(k, "k"); check_chunks(v, "v");
  auto o_bnhd = at::empty({B, Nq, H, D}, q.options());
  auto o = o_bnhd.permute({0, 2, 1, 3});
  auto lse = at::empty({B, H, Nq}, q.options().dtype(at::kFloat));
  if (o.numel() == 0) return {o, lse};
  const MaskArgs mi = mask_args(mask, Nq, Nk);
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_dp(D, [&](auto dp) {
    constexpr int kDp = decltype(dp)::value;
    auto run = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(cdiv(Nq, 64), B * H), dim3(kThreads), 0, stream,
          (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
          mi.ptr, (__bf16*)o_bnhd.data_ptr(), lse.data_ptr<float>(),
          H, Nq, Nk, D, (float)scale, mi.mB, mi.sb, mi.sh,
          q.stride(0), q.stride(1), q.stride(2),
          k.stride(0), k.stride(1), k.stride(2),
          v.stride(0), v.stride(1), v.stride(2));
    };
    if (mi.ptr) run(attn_hd_fwd_kernel<kDp, true>);
    else run(attn_hd_fwd_kernel<kDp, false>);
  });
  HIP_CHECK_LAST();
  return {o, lse};
}

std::vector<at::Tensor> attn_bwd_preprocess_head_dims(const at::Tensor& dout, const at::Tensor& o) {
  const int B = dout.size(0), H = dout.size(1), N = dout.size(2), D = dout.size(3);
  TORCH_CHECK(D % 8 == 0 && D >= 8 && D <= 128);
  TORCH_CHECK(o.sizes() == dout.sizes() && o.scalar_type() == at::kBFloat16);
  check_chunks(dout, "dO"); check_chunks(o, "O");
  auto do_c = at::empty({B, H, N, D}, dout.options());
  auto delta = at::empty({B, H, N}, dout.options().dtype(at::kFloat));
  const long rows = (long)B * H * N;
  if (rows == 0) return {do_c, delta};
  int lpr = 1;
  while (lpr * 8 < D) lpr *= 2;
  const int rows_per_block = kThreads / lpr;
  const int blocks = (int)std::min((rows + rows_per_block - 1) / rows_per_block, (long)8192);
  hipLaunchKernelGGL(attn_hd_bwd_preprocess_kernel, dim3(blocks), dim3(kThreads), 0,
      at::hip::getCurrentHIPStream(),
      (const __bf16*)dout.data_ptr(), (const __bf16*)o.data_ptr(),
      (__bf16*)do_c.data_ptr(), delta.data_ptr<float>(), rows, D, lpr,
      dout.stride(0), dout.stride(1), dout.stride(2),
      o.stride(0), o.stride(1), o.stride(2), H, N);
  HIP_CHECK_LAST();
  return {do_c, delta};
}

void attention_bwd_head_dims(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& dov, const at::Tensor& lse, const at::Tensor& delta,
    const c10::optional<at::Tensor>& mask,
    at::Tensor& dq, at::Tensor& dk, at::Tensor& dv, double scale) {
  const int B = q.size(0), H = q.size(1), Nq = q.size(2), D = q.size(3), Nk = k.size(2);
  TORCH_CHECK(D % 8 == 0 && D >= 8 && D <= 128, "attention_bwd: head_dim must be a multiple of 8, <=128");
  TORCH_CHECK(k.dim() == 4 && v.dim() == 4 && k.size(0) == B && k.size(1) == H && k.size(3) == D &&
              v.size(0) == B && v.size(1) == H && v.size(2) == Nk && v.size(3) == D &&
              dq.sizes() == q.sizes() && dk.sizes() == k.sizes() && dv.sizes() == v.sizes() &&
              dov.sizes() == q.sizes(), "attention_bwd: shapes disagree");
  TORCH_CHECK(k.scalar_type() == at::kBFloat16 && v.scalar_type() == at::kBFloat16 &&
              dov.scalar_type() == at::kBFloat16 && dq.scalar_type() == at::kBFloat16 &&
              dk.scalar_type() == at::kBFloat16 && dv.scalar_type() == at::kBFloat16,
              "attention_bwd: bf16 only");
  const long rows = (long)B * H * Nq;
  TORCH_CHECK(lse.is_contiguous() && lse.scalar_type() == at::kFloat && lse.numel() == rows &&
              delta.is_contiguous() && delta.scalar_type() == at::kFloat && delta.numel() == rows,
              "attention_bwd: lse/delta must be contiguous fp32 [B,H,Nq]");
  check_chunks(q, "q"); check_chunks(k, "k"); check_chunks(v, "v");
  check_chunks(dq, "dq"); check_chunks(dk, "dk"); check_chunks(dv, "dv");
  check_chunks(dov, "dO");
  if (q.numel() == 0 || k.numel() == 0) return;
  const MaskArgs mi = mask_args(mask, Nq, Nk);
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_dp(D, [&](auto dp) {
    constexpr int kDp = decltype(dp)::value;
    auto run_dq = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(cdiv(Nq, 64), B * H), dim3(kThreads), 0, stream,
          (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
          (const __bf16*)dov.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
          mi.ptr, (__bf16*)dq.data_ptr(),
          H, Nq, Nk, D, (float)scale, mi.mB, mi.sb, mi.sh,
          q.stride(0), q.stride(1), q.stride(2),
          k.stride(0), k.stride(1), k.stride(2),
          v.stride(0), v.stride(1), v.stride(2),
          dq.stride(0), dq.stride(1), dq.stride(2));
    };
    auto run_kv = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(cdiv(Nk, 64), B * H), dim3(kThreads), 0, stream,
          (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
          (const __bf16*)dov.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
          mi.ptr, (__bf16*)dk.data_ptr(), (__bf16*)dv.data_ptr(),
          H, Nq, Nk, D, (float)scale, mi.mB, mi.sb, mi.sh,
          q.stride(0), q.stride(1), q.stride(2),
          k.stride(0), k.stride(1), k.stride(2),
          v.stride(0), v.stride(1), v.stride(2),
          dk.stride(0), dk.stride(1), dk.stride(2),
          dv.stride(0), dv.stride(1), dv.stride(2));
    };
    if (mi.ptr) {
      run_dq(attn_hd_bwd_dq_kernel<kDp, true>);
      run_kv(attn_hd_bwd_dkdv_kernel<kDp, true>);
    } else {
      run_dq(attn_hd_bwd_dq_kernel<kDp, false>);
      run_kv(attn_hd_bwd_dkdv_kernel<kDp, false>);
    }
  });
  HIP_CHECK_LAST();
}

void attention_bwd_dbias_head_dims(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& dov, const at::Tensor& lse, const at::Tensor& delta,
    const at::Tensor& mask, float* out, double scale, int n_red, int chunk, int nsplit) {
  const int H = q.size(1), Nq = q.size(2), D = q.size(3), Nk = k.size(2);
  TORCH_CHECK(D % 8 == 0 && D >= 8 && D <= 128);
  check_chunks(q, "q"); check_chunks(k, "k"); check_chunks(v, "v"); check_chunks(dov, "dO");
  const MaskArgs mi = mask_args(mask, Nq, Nk);
  const int Hm = (int)mask.size(1), n_kt = cdiv(Nk, 64);
  auto stream = at::hip::getCurrentHIPStream();
  dispatch_dp(D, [&](auto dp) {
    constexpr int kDp = decltype(dp)::value;
    hipLaunchKernelGGL(attn_hd_bwd_dbias_kernel<kDp>,
        dim3(cdiv(Nq, 64) * n_kt * mi.mB * Hm, 1, nsplit), dim3(kThreads), 0, stream,
        (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
        (const __bf16*)dov.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
        mi.ptr, out,
        H, Nq, Nk, D, (float)scale, mi.mB, Hm, n_kt, n_red, chunk,
        q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2));
  });
  HIP_CHECK_LAST();
}
