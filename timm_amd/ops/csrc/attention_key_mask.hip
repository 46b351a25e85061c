// Key-padding attention for gfx950 (CDNA4): forward, dQ and dK/dV kernels that
// take a per-sample key validity vector instead of an additive [B,1,Nq,Nk] mask.
//
// Serves the NaFlex padding case (timm_amd/models/naflexvit.py): a bool
// [B,1,1,Nk] mask through ops.flash_attention / ops.flash_attention_qkv, bf16,
// head_dim 64.  The additive-mask kernels of attention.hip / attention_bwd.hip
// read 4 bytes of mask per score from HBM, per head and per pass, and run the
// MFMAs of tiles whose keys are all padding.  Here validity is N bits per
// sample and lives in scalar registers.
//
// Validity words
//   The launcher passes validity as contiguous uint8 [B,Nk].  For every 64-key
//   tile, lane i of a wave loads byte tile*64 + i (0 past Nk) and a ballot
//   turns the 64 bytes into one 64-bit word.  The forward and dQ kernels form
//   all words of their sample once at kernel start into a small LDS array
//   (kMaxTiles words, so Nk <= kMaxNk; the launcher checks) and read them back
//   as wave-uniform values (readfirstlane -> SGPR pair).  The dK/dV kernel owns
//   one key tile and keeps only that tile's word.  The Nk tail is folded into
//   the bits, so no kernel compares a column index with Nk.
//     word == 0   the tile is skipped before any K/V load: it never leaves HBM
//     word == ~0  no per-element select at all
//     otherwise   column c is live iff bit c; K/V rows of dead keys are not
//                 loaded either (zero-filled), and their P / dS are exact zeros
//
// Work split (256 threads = 4 waves, MFMA v_mfma_f32_16x16x32_bf16 throughout)
//   fwd, dQ: one workgroup per (64-query tile, batch, head); wave w owns query
//            rows [16w, 16w+16) and sweeps the live 64-key tiles.
//   dK/dV:   one workgroup per (64-key tile, batch, head); wave w owns key rows
//            [16w, 16w+16) and sweeps the queries in 32-row tiles.  A workgroup
//            whose word is 0 stores zeros to its dk/dv rows and exits.
//   No float atomics anywhere: every output element has one writer and a fixed
//   summation order, so results are bit-reproducible.
//
// Data movement
//   * The loop-invariant MFMA operand stays in registers for the whole sweep
//     and is read straight from global memory in fragment layout (lane
//     (l16, g4) takes 16 contiguous bytes of row l16), never through LDS:
//     Q in the forward, Q and dO in dQ, K and V in dK/dV.
//   * The streamed operand (K/V tiles, or Q/dO tiles in dK/dV) is prefetched:
//     while the MFMAs of the current live tile run, each thread already holds
//     the global loads of the next live tile in registers; they are stored to
//     LDS after the barrier that ends the current tile.  Skipped tiles are
//     stepped over by scanning the words, so the prefetch always targets a
//     tile that will be used.
//   * Row-major LDS tiles have 128-byte rows with the XOR swizzle of
//     attention.hip (byte ^= (row & 7) << 4) for conflict-free ds_read_b128
//     fragment reads.  Operands that an MFMA needs column-wise (V in the
//     forward, K in dQ, Q and dO in dK/dV) are also stored transposed, from
//     the same prefetch registers, so those fragments are one ds_read_b128 too.
//   * P and dS go from the C layout to the A layout through a per-wave LDS
//     patch whose rows are padded by 8 elements (144 / 80 bytes), which puts
//     the 16 rows of a fragment read on different banks.
//   LDS per workgroup: forward 25.5 KB, dQ 33.5 KB, dK/dV 26 KB.
//
// q/k/v and dq/dk/dv go through their strides (views into a packed
// [B,N,3,H,D] buffer work); O is written BNHD, lse [B,H,Nq], as attention_fwd.
// A query row of a sample with no valid key gets O = 0, lse = +inf and zero
// gradients, like the additive-mask kernels.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

constexpr int kD = 64;            // head_dim, fixed
constexpr int kThreads = 256;
constexpr int kTile = 64;         // keys per validity word
constexpr int kMaxTiles = 64;     // words kept in LDS
constexpr int kMaxNk = kMaxTiles * kTile;
constexpr int kRowBytes = kD * 2;
constexpr int kPRow = kTile + 8;  // padded row of the 16 x 64 P / dS patch
constexpr int kQB = 32;           // query rows per step of the dK/dV sweep
constexpr int kPtRow = kQB + 8;   // padded row of the 16 x 32 P^T / dS^T patch
constexpr float kNegInf = -1e30f;

__device__ __forceinline__ int swz(int row, int byte_off) {
  return byte_off ^ ((row & 7) << 4);
}
// transposed tiles: rows of 64 or 128 bytes
__device__ __forceinline__ int swz_t(int row, int byte_off) {
  return byte_off ^ ((row & 3) << 4);
}

__device__ __forceinline__ u64 tile_word(const unsigned char* valid_b, int tile, int Nk, int lane) {
  const int col = tile * kTile + lane;
  const int byte = (col < Nk) ? valid_b[col] : 0;
  return __ballot(byte != 0);
}

__device__ __forceinline__ void build_words(u64* vw, const unsigned char* valid_b,
                                            int n_tiles, int Nk, int wave, int lane) {
  for (int t = wave; t < n_tiles; t += kThreads / WAVE_SIZE) {
    const u64 w = tile_word(valid_b, t, Nk, lane);
    if (lane == 0) vw[t] = w;
  }
}

__device__ __forceinline__ u64 uniform_word(const u64* vw, int t) {
  const u64 w = vw[t];
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)w);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(w >> 32));
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ int next_live(const u64* vw, int t, int n_tiles) {
  while (t < n_tiles && uniform_word(vw, t) == 0) ++t;
  return t;
}

// is column n16*16 + l16 of the tile live
__device__ __forceinline__ bool col_live(u64 word, int n16, int l16) {
  return (((unsigned)(word >> (n16 * 16)) >> l16) & 1u) != 0;
}

// MFMA A/B fragment of one row, straight from global memory; rows that are
// not live give zeros
__device__ __forceinline__ void load_frag(bf16x8_t (&f)[2], const __bf16* row_ptr, bool live,
                                          int g4) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8_t z = {};
    f[ks] = live ? *reinterpret_cast<const bf16x8_t*>(row_ptr + ks * 32 + g4 * 8) : z;
  }
}

// Prefetch of one 64-row tile: thread t takes 16-byte chunks t and t + 256
// (row = chunk / 8).  Rows whose bit is 0 are not read.
__device__ __forceinline__ void load_tile64(bf16x8_t (&reg)[2], const __bf16* base, long sn,
                                            int row0, u64 word) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = threadIdx.x + i * kThreads;
    const int row = c >> 3, col8 = c & 7;
    bf16x8_t z = {};
    reg[i] = ((word >> row) & 1)
        ? *reinterpret_cast<const bf16x8_t*>(base + (long)(row0 + row) * sn + col8 * 8) : z;
  }
}

__device__ __forceinline__ void store_tile64(__bf16* lds, const bf16x8_t (&reg)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = threadIdx.x + i * kThreads;
    const int row = c >> 3, col8 = c & 7;
    *reinterpret_cast<bf16x8_t*>(
        reinterpret_cast<char*>(lds) + swz(row, row * kRowBytes + col8 * 16)) = reg[i];
  }
}

// transposed store T[d][row], 128-byte rows
__device__ __forceinline__ void store_tile64_t(__bf16* lds_t, const bf16x8_t (&reg)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = threadIdx.x + i * kThreads;
    const int row = c >> 3, col8 = c & 7;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = col8 * 8 + j;
      *reinterpret_cast<__bf16*>(
          reinterpret_cast<char*>(lds_t) + swz_t(d, d * (kTile * 2) + row * 2)) = reg[i][j];
    }
  }
}

__device__ __forceinline__ bf16x8_t frag_row(const __bf16* lds, int row, int ks, int g4) {
  return *reinterpret_cast<const bf16x8_t*>(
      reinterpret_cast<const char*>(lds) + swz(row, row * kRowBytes + ks * 64 + g4 * 16));
}

// fragment of a transposed tile with `cols` columns: T[drow][ks*32 + g4*8 .. +8)
__device__ __forceinline__ bf16x8_t frag_row_t(const __bf16* lds_t, int drow, int ks, int g4,
                                               int cols) {
  return *reinterpret_cast<const bf16x8_t*>(
      reinterpret_cast<const char*>(lds_t) + swz_t(drow, drow * cols * 2 + ks * 64 + g4 * 16));
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads)
void attn_key_mask_fwd_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const unsigned char* __restrict__ valid,  // [B,Nk]
    __bf16* __restrict__ o,                   // [B,Nq,H,D]
    float* __restrict__ lse,                  // [B,H,Nq]
    int H, int Nq, int Nk, float scale,
    long q_sb, long q_sh, long q_sn,
    long k_sb, long k_sh, long k_sn,
    long v_sb, long v_sh, long v_sn) {
  __shared__ __attribute__((aligned(16))) __bf16 k_lds[kTile * kD];
  __shared__ __attribute__((aligned(16))) __bf16 vt_lds[kD * kTile];
  __shared__ __attribute__((aligned(16))) __bf16 p_lds[4 * 16 * kPRow];
  __shared__ u64 vw[kMaxTiles];

  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh % H;
  const int qbase = blockIdx.x * 64;
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;

  const int n_tiles = (Nk + kTile - 1) / kTile;
  build_words(vw, valid + (long)b * Nk, n_tiles, Nk, wave, lane);

  const __bf16* k_bh = k + (long)b * k_sb + (long)h * k_sh;
  const __bf16* v_bh = v + (long)b * v_sb + (long)h * v_sh;
  bf16x8_t qa[2];
  {
    const int qrow = qbase + wave * 16 + l16;
    load_frag(qa, q + (long)b * q_sb + (long)h * q_sh + (long)qrow * q_sn, qrow < Nq, g4);
  }
  __syncthreads();  // words visible

  float m_run[4], l_run[4];
  f32x4 acc_o[kD / 16];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = kNegInf; l_run[r] = 0.f; }
#pragma unroll
  for (int f = 0; f < kD / 16; ++f) acc_o[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  __bf16* p_w = p_lds + wave * (16 * kPRow);
  bf16x8_t kreg[2], vreg[2];
  int kt = next_live(vw, 0, n_tiles);
  if (kt < n_tiles) {
    const u64 w = uniform_word(vw, kt);
    load_tile64(kreg, k_bh, k_sn, kt * kTile, w);
    load_tile64(vreg, v_bh, v_sn, kt * kTile, w);
  }
  while (kt < n_tiles) {
    const u64 word = uniform_word(vw, kt);
    store_tile64(k_lds, kreg);
    store_tile64_t(vt_lds, vreg);
    __syncthreads();
    const int nxt = next_live(vw, kt + 1, n_tiles);
    if (nxt < n_tiles) {  // in flight under the MFMAs below
      const u64 w = uniform_word(vw, nxt);
      load_tile64(kreg, k_bh, k_sn, nxt * kTile, w);
      load_tile64(vreg, v_bh, v_sn, nxt * kTile, w);
    }

    // S = scale * Q K^T; rows past Nq hold zeros and are never written
    float s_frag[4][4];
#pragma unroll
    for (int n16 = 0; n16 < 4; ++n16) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            qa[ks], frag_row(k_lds, n16 * 16 + l16, ks, g4), acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s_frag[n16][r] = acc[r] * scale;
    }
    if (word != ~0ull) {  // mixed tile
#pragma unroll
      for (int n16 = 0; n16 < 4; ++n16) {
        const bool live = col_live(word, n16, l16);
#pragma unroll
        for (int r = 0; r < 4; ++r) s_frag[n16][r] = live ? s_frag[n16][r] : kNegInf;
      }
    }

    // online softmax.  The tile has a live column, so m_new is finite and
    // exp(kNegInf - m_new) is an exact 0: dead columns and the first tile's
    // rescale need no select.
    float factor[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m_tile = fmaxf(fmaxf(s_frag[0][r], s_frag[1][r]), fmaxf(s_frag[2][r], s_frag[3][r]));
      m_tile = group16_reduce_max(m_tile);
      const float m_new = fmaxf(m_run[r], m_tile);
      factor[r] = __expf(m_run[r] - m_new);
      m_run[r] = m_new;
      float psum = 0.f;
#pragma unroll
      for (int n16 = 0; n16 < 4; ++n16) {
        const float p = __expf(s_frag[n16][r] - m_new);
        s_frag[n16][r] = p;
        psum += p;
      }
      l_run[r] = l_run[r] * factor[r] + group16_reduce_sum(psum);
    }

    // P: C layout -> A layout through this wave's LDS patch
#pragma unroll
    for (int n16 = 0; n16 < 4; ++n16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p_w[(g4 * 4 + r) * kPRow + n16 * 16 + l16] = (__bf16)s_frag[n16][r];
      }
    }
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16x8_t pa[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      pa[ks] = *reinterpret_cast<const bf16x8_t*>(p_w + l16 * kPRow + ks * 32 + g4 * 8);
    }
#pragma unroll
    for (int f = 0; f < kD / 16; ++f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc_o[f][r] *= factor[r];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        acc_o[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pa[ks], frag_row_t(vt_lds, f * 16 + l16, ks, g4, kTile), acc_o[f], 0, 0, 0);
      }
    }
    __syncthreads();  // tile consumed before the next one is stored
    kt = nxt;
  }

  __bf16* o_bh = o + ((long)b * Nq) * (H * kD) + (long)h * kD;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = qbase + wave * 16 + g4 * 4 + r;
    if (qrow >= Nq) continue;
    const float inv_l = (l_run[r] > 0.f) ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int f = 0; f < kD / 16; ++f) {
      o_bh[(long)qrow * (H * kD) + f * 16 + l16] = (__bf16)(acc_o[f][r] * inv_l);
    }
    if (l16 == 0) {
      lse[(long)bh * Nq + qrow] = (l_run[r] > 0.f) ? (m_run[r] + __logf(l_run[r])) : INFINITY;
    }
  }
}

// ---------------------------------------------------------------------------
// dQ: same split and skip loop as the forward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads)
void attn_key_mask_bwd_dq_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dov,           // [B,H,Nq,D] contiguous
    const float* __restrict__ lse, const float* __restrict__ delta,  // [B,H,Nq]
    const unsigned char* __restrict__ valid,
    __bf16* __restrict__ dq,
    int H, int Nq, int Nk, float scale,
    long q_sb, long q_sh, long q_sn,
    long k_sb, long k_sh, long k_sn,
    long v_sb, long v_sh, long v_sn,
    long dq_sb, long dq_sh, long dq_sn) {
  __shared__ __attribute__((aligned(16))) __bf16 k_lds[kTile * kD];
  __shared__ __attribute__((aligned(16))) __bf16 v_lds[kTile * kD];
  __shared__ __attribute__((aligned(16))) __bf16 kt_lds[kD * kTile];
  __shared__ __attribute__((aligned(16))) __bf16 ds_lds[4 * 16 * kPRow];
  __shared__ u64 vw[kMaxTiles];

  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh % H;
  const int qbase = blockIdx.x * 64;
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;

  const int n_tiles = (Nk + kTile - 1) / kTile;
  build_words(vw, valid + (long)b * Nk, n_tiles, Nk, wave, lane);

  const __bf16* k_bh = k + (long)b * k_sb + (long)h * k_sh;
  const __bf16* v_bh = v + (long)b * v_sb + (long)h * v_sh;
  bf16x8_t qa[2], da[2];
  {
    const int qrow = qbase + wave * 16 + l16;
    load_frag(qa, q + (long)b * q_sb + (long)h * q_sh + (long)qrow * q_sn, qrow < Nq, g4);
    load_frag(da, dov + ((long)bh * Nq + qrow) * kD, qrow < Nq, g4);
  }
  // rows past Nq: lse = +inf makes P an exact 0
  float lse_r[4], delta_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = qbase + wave * 16 + g4 * 4 + r;
    lse_r[r] = (qrow < Nq) ? lse[(long)bh * Nq + qrow] : INFINITY;
    delta_r[r] = (qrow < Nq) ? delta[(long)bh * Nq + qrow] : 0.f;
  }
  __syncthreads();  // words visible

  f32x4 acc_dq[kD / 16];
#pragma unroll
  for (int f = 0; f < kD / 16; ++f) acc_dq[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  __bf16* ds_w = ds_lds + wave * (16 * kPRow);
  bf16x8_t kreg[2], vreg[2];
  int kt = next_live(vw, 0, n_tiles);
  if (kt < n_tiles) {
    const u64 w = uniform_word(vw, kt);
    load_tile64(kreg, k_bh, k_sn, kt * kTile, w);
    load_tile64(vreg, v_bh, v_sn, kt * kTile, w);
  }
  while (kt < n_tiles) {
    const u64 word = uniform_word(vw, kt);
    store_tile64(k_lds, kreg);
    store_tile64_t(kt_lds, kreg);
    store_tile64(v_lds, vreg);
    __syncthreads();
    const int nxt = next_live(vw, kt + 1, n_tiles);
    if (nxt < n_tiles) {
      const u64 w = uniform_word(vw, nxt);
      load_tile64(kreg, k_bh, k_sn, nxt * kTile, w);
      load_tile64(vreg, v_bh, v_sn, nxt * kTile, w);
    }

    // dS = P o (dP - delta) * scale, P = exp(scale * S - lse)
    float ds_frag[4][4];
#pragma unroll
    for (int n16 = 0; n16 < 4; ++n16) {
      f32x4 acc_s = {0.f, 0.f, 0.f, 0.f};
      f32x4 acc_dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        acc_s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            qa[ks], frag_row(k_lds, n16 * 16 + l16, ks, g4), acc_s, 0, 0, 0);
        acc_dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            da[ks], frag_row(v_lds, n16 * 16 + l16, ks, g4), acc_dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(acc_s[r] * scale - lse_r[r]);
        ds_frag[n16][r] = p * (acc_dp[r] - delta_r[r]) * scale;
      }
    }
    if (word != ~0ull) {  // mixed tile
#pragma unroll
      for (int n16 = 0; n16 < 4; ++n16) {
        const bool live = col_live(word, n16, l16);
#pragma unroll
        for (int r = 0; r < 4; ++r) ds_frag[n16][r] = live ? ds_frag[n16][r] : 0.f;
      }
    }

#pragma unroll
    for (int n16 = 0; n16 < 4; ++n16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ds_w[(g4 * 4 + r) * kPRow + n16 * 16 + l16] = (__bf16)ds_frag[n16][r];
      }
    }
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16x8_t dsa[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      dsa[ks] = *reinterpret_cast<const bf16x8_t*>(ds_w + l16 * kPRow + ks * 32 + g4 * 8);
    }
    // dQ += dS K
#pragma unroll
    for (int f = 0; f < kD / 16; ++f) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        acc_dq[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            dsa[ks], frag_row_t(kt_lds, f * 16 + l16, ks, g4, kTile), acc_dq[f], 0, 0, 0);
      }
    }
    __syncthreads();
    kt = nxt;
  }

  __bf16* dq_bh = dq + (long)b * dq_sb + (long)h * dq_sh;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = qbase + wave * 16 + g4 * 4 + r;
    if (qrow >= Nq) continue;
#pragma unroll
    for (int f = 0; f < kD / 16; ++f) {
      dq_bh[(long)qrow * dq_sn + f * 16 + l16] = (__bf16)acc_dq[f][r];
    }
  }
}

// ---------------------------------------------------------------------------
// dK/dV: workgroup owns 64 keys, sweeps the queries in 32-row tiles
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads)
void attn_key_mask_bwd_dkdv_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dov,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const unsigned char* __restrict__ valid,
    __bf16* __restrict__ dk, __bf16* __restrict__ dv,
    int H, int Nq, int Nk, float scale,
    long q_sb, long q_sh, long q_sn,
    long k_sb, long k_sh, long k_sn,
    long v_sb, long v_sh, long v_sn,
    long dk_sb, long dk_sh, long dk_sn,
    long dv_sb, long dv_sh, long dv_sn) {
  __shared__ __attribute__((aligned(16))) __bf16 q_lds[kQB * kD];
  __shared__ __attribute__((aligned(16))) __bf16 do_lds[kQB * kD];
  __shared__ __attribute__((aligned(16))) __bf16 qt_lds[kD * kQB];
  __shared__ __attribute__((aligned(16))) __bf16 dot_lds[kD * kQB];
  __shared__ __attribute__((aligned(16))) __bf16 pt_lds[4 * 16 * kPtRow];
  __shared__ __attribute__((aligned(16))) __bf16 dst_lds[4 * 16 * kPtRow];

  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh % H;
  const int kvbase = blockIdx.x * kTile;
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;

  __bf16* dk_bh = dk + (long)b * dk_sb + (long)h * dk_sh;
  __bf16* dv_bh = dv + (long)b * dv_sb + (long)h * dv_sh;

  // every wave forms the word of this key tile itself: no LDS, no barrier
  const u64 word = tile_word(valid + (long)b * Nk, blockIdx.x, Nk, lane);
  if (word == 0) {
    // all padding: the rows below Nk get zeros (the buffers are uninitialised)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = threadIdx.x + i * kThreads;
      const int row = kvbase + (c >> 3), col8 = c & 7;
      if (row < Nk) {
        bf16x8_t z = {};
        *reinterpret_cast<bf16x8_t*>(dk_bh + (long)row * dk_sn + col8 * 8) = z;
        *reinterpret_cast<bf16x8_t*>(dv_bh + (long)row * dv_sn + col8 * 8) = z;
      }
    }
    return;
  }

  // K and V rows of this wave, loop-invariant A operands
  bf16x8_t ka[2], va[2];
  {
    const int row = wave * 16 + l16;
    const bool live = ((word >> row) & 1) != 0;
    load_frag(ka, k + (long)b * k_sb + (long)h * k_sh + (long)(kvbase + row) * k_sn, live, g4);
    load_frag(va, v + (long)b * v_sb + (long)h * v_sh + (long)(kvbase + row) * v_sn, live, g4);
  }
  // liveness of the 4 key rows this lane holds in the C layout
  bool row_live[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) row_live[r] = ((word >> (wave * 16 + g4 * 4 + r)) & 1) != 0;

  f32x4 acc_dk[kD / 16], acc_dv[kD / 16];
#pragma unroll
  for (int f = 0; f < kD / 16; ++f) {
    acc_dk[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc_dv[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const __bf16* q_bh = q + (long)b * q_sb + (long)h * q_sh;
  const __bf16* do_bh = dov + ((long)bh * Nq) * kD;
  __bf16* pt_w = pt_lds + wave * (16 * kPtRow);
  __bf16* dst_w = dst_lds + wave * (16 * kPtRow);

  // prefetch of a 32-row Q / dO tile: one 16-byte chunk of each per thread
  const int st_row = threadIdx.x >> 3, st_col8 = threadIdx.x & 7;
  bf16x8_t qreg, doreg;
  auto load_q = [&](int q0) {
    bf16x8_t z = {};
    const int row = q0 + st_row;
    qreg = (row < Nq) ? *reinterpret_cast<const bf16x8_t*>(q_bh + (long)row * q_sn + st_col8 * 8) : z;
    doreg = (row < Nq) ? *reinterpret_cast<const bf16x8_t*>(do_bh + (long)row * kD + st_col8 * 8) : z;
  };
  auto store_q = [&](__bf16* lds, __bf16* lds_t, const bf16x8_t& reg) {
    *reinterpret_cast<bf16x8_t*>(
        reinterpret_cast<char*>(lds) + swz(st_row, st_row * kRowBytes + st_col8 * 16)) = reg;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = st_col8 * 8 + j;
      *reinterpret_cast<__bf16*>(
          reinterpret_cast<char*>(lds_t) + swz_t(d, d * (kQB * 2) + st_row * 2)) = reg[j];
    }
  };

  const int n_qt = (Nq + kQB - 1) / kQB;
  load_q(0);
  for (int qt = 0; qt < n_qt; ++qt) {
    const int q0 = qt * kQB;
    __syncthreads();  // previous tile consumed
    store_q(q_lds, qt_lds, qreg);
    store_q(do_lds, dot_lds, doreg);
    __syncthreads();
    if (qt + 1 < n_qt) load_q(q0 + kQB);

    // S^T = K Q^T, dP^T = V dO^T: rows = keys (wave*16 + g4*4 + r), cols = queries
    float pt_frag[2][4], dst_frag[2][4];
#pragma unroll
    for (int n16 = 0; n16 < 2; ++n16) {
      const int qcol = q0 + n16 * 16 + l16;
      // columns past Nq: lse = +inf makes P an exact 0
      const float lse_c = (qcol < Nq) ? lse[(long)bh * Nq + qcol] : INFINITY;
      const float delta_c = (qcol < Nq) ? delta[(long)bh * Nq + qcol] : 0.f;
      f32x4 acc_s = {0.f, 0.f, 0.f, 0.f};
      f32x4 acc_dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        acc_s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ka[ks], frag_row(q_lds, n16 * 16 + l16, ks, g4), acc_s, 0, 0, 0);
        acc_dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            va[ks], frag_row(do_lds, n16 * 16 + l16, ks, g4), acc_dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(acc_s[r] * scale - lse_c);
        pt_frag[n16][r] = p;
        dst_frag[n16][r] = p * (acc_dp[r] - delta_c) * scale;
      }
    }
    if (word != ~0ull) {  // mixed tile: rows of dead keys are exact zeros
#pragma unroll
      for (int n16 = 0; n16 < 2; ++n16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pt_frag[n16][r] = row_live[r] ? pt_frag[n16][r] : 0.f;
          dst_frag[n16][r] = row_live[r] ? dst_frag[n16][r] : 0.f;
        }
      }
    }

#pragma unroll
    for (int n16 = 0; n16 < 2; ++n16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pt_w[(g4 * 4 + r) * kPtRow + n16 * 16 + l16] = (__bf16)pt_frag[n16][r];
        dst_w[(g4 * 4 + r) * kPtRow + n16 * 16 + l16] = (__bf16)dst_frag[n16][r];
      }
    }
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const bf16x8_t pa = *reinterpret_cast<const bf16x8_t*>(pt_w + l16 * kPtRow + g4 * 8);
    const bf16x8_t dsa = *reinterpret_cast<const bf16x8_t*>(dst_w + l16 * kPtRow + g4 * 8);
    // dV += P^T dO, dK += dS^T Q
#pragma unroll
    for (int f = 0; f < kD / 16; ++f) {
      acc_dv[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pa, frag_row_t(dot_lds, f * 16 + l16, 0, g4, kQB), acc_dv[f], 0, 0, 0);
      acc_dk[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          dsa, frag_row_t(qt_lds, f * 16 + l16, 0, g4, kQB), acc_dk[f], 0, 0, 0);
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kvrow = kvbase + wave * 16 + g4 * 4 + r;
    if (kvrow >= Nk) continue;
#pragma unroll
    for (int f = 0; f < kD / 16; ++f) {
      dk_bh[(long)kvrow * dk_sn + f * 16 + l16] = (__bf16)acc_dk[f][r];
      dv_bh[(long)kvrow * dv_sn + f * 16 + l16] = (__bf16)acc_dv[f][r];
    }
  }
}

// 16-byte chunks through the tensor's own strides
bool aligned16(const at::Tensor& t) {
  return t.dim() == 4 && t.stride(3) == 1 &&
         reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 &&
         t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 && t.stride(2) % 8 == 0;
}

void check_qkv(const char* who, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
               const at::Tensor& valid) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda() && valid.is_cuda(), who, ": GPU tensors");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 && k.scalar_type() == at::kBFloat16 &&
              v.scalar_type() == at::kBFloat16, who, ": bf16 only");
  TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(v),
              who, ": q/k/v must be 4-D with 16-byte aligned rows");
  const int64_t B = q.size(0), H = q.size(1), Nk = k.size(2);
  TORCH_CHECK(q.size(3) == kD && k.size(3) == kD && v.size(3) == kD, who, ": head_dim 64 only");
  TORCH_CHECK(k.size(0) == B && k.size(1) == H && v.size(0) == B && v.size(1) == H &&
              v.size(2) == Nk, who, ": q/k/v shapes disagree");
  TORCH_CHECK(Nk >= 1 && Nk <= kMaxNk, who, ": Nk must be in [1, ", kMaxNk, "]");
  TORCH_CHECK(B * H <= 65535, who, ": B * H must fit the grid");
  TORCH_CHECK(valid.scalar_type() == at::kByte && valid.is_contiguous() && valid.dim() == 2 &&
              valid.size(0) == B && valid.size(1) == Nk,
              who, ": valid must be contiguous uint8 [B,Nk]");
}

}  // namespace

// q/k/v strided [B,H,N,64] bf16, valid uint8 [B,Nk] (non-zero = the key takes
// part).  Returns O as a [B,H,Nq,D] view of BNHD storage and lse [B,H,Nq].
std::vector<at::Tensor> attention_key_mask_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                               at::Tensor valid, double scale) {
  check_qkv("attention_key_mask_fwd", q, k, v, valid);
  const int B = q.size(0), H = q.size(1), Nq = q.size(2), Nk = k.size(2);
  auto o_bnhd = at::empty({B, Nq, H, kD}, q.options());
  auto o = o_bnhd.permute({0, 2, 1, 3});
  auto lse = at::empty({B, H, Nq}, q.options().dtype(at::kFloat));
  if (o.numel() == 0) return {o, lse};
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(attn_key_mask_fwd_kernel, dim3(cdiv(Nq, 64), B * H), dim3(kThreads), 0,
      stream,
      (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
      valid.data_ptr<uint8_t>(), (__bf16*)o_bnhd.data_ptr(), lse.data_ptr<float>(),
      H, Nq, Nk, (float)scale,
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2));
  HIP_CHECK_LAST();
  return {o, lse};
}

// dov contiguous [B,H,Nq,64], lse/delta fp32 [B,H,Nq] (attn_bwd_preprocess);
// dq/dk/dv preallocated, possibly views into a packed dqkv buffer.
void attention_key_mask_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                            at::Tensor dov, at::Tensor lse, at::Tensor delta,
                            at::Tensor valid,
                            at::Tensor dq, at::Tensor dk, at::Tensor dv, double scale) {
  check_qkv("attention_key_mask_bwd", q, k, v, valid);
  const int B = q.size(0), H = q.size(1), Nq = q.size(2), Nk = k.size(2);
  TORCH_CHECK(dov.is_cuda() && dov.scalar_type() == at::kBFloat16 && dov.is_contiguous() &&
              dov.sizes() == q.sizes(), "attention_key_mask_bwd: dO must be contiguous [B,H,Nq,D]");
  const int64_t rows = (int64_t)B * H * Nq;
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() && lse.scalar_type() == at::kFloat &&
              lse.numel() == rows && delta.is_cuda() && delta.is_contiguous() &&
              delta.scalar_type() == at::kFloat && delta.numel() == rows,
              "attention_key_mask_bwd: lse/delta must be contiguous fp32 [B,H,Nq]");
  for (const at::Tensor* t : {&dq, &dk, &dv}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && aligned16(*t),
                "attention_key_mask_bwd: dq/dk/dv must be bf16 with 16-byte aligned rows");
  }
  TORCH_CHECK(dq.sizes() == q.sizes() && dk.sizes() == k.sizes() && dv.sizes() == v.sizes(),
              "attention_key_mask_bwd: gradient shapes disagree");
  if (q.numel() == 0) {
    dk.zero_();
    dv.zero_();
    return;
  }
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(attn_key_mask_bwd_dq_kernel, dim3(cdiv(Nq, 64), B * H), dim3(kThreads), 0,
      stream,
      (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
      (const __bf16*)dov.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
      valid.data_ptr<uint8_t>(), (__bf16*)dq.data_ptr(),
      H, Nq, Nk, (float)scale,
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2),
      dq.stride(0), dq.stride(1), dq.stride(2));
  hipLaunchKernelGGL(attn_key_mask_bwd_dkdv_kernel, dim3(cdiv(Nk, kTile), B * H), dim3(kThreads),
      0, stream,
      (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
      (const __bf16*)dov.data_ptr(), lse.data_ptr<float>(), delta.data_ptr<float>(),
      valid.data_ptr<uint8_t>(), (__bf16*)dk.data_ptr(), (__bf16*)dv.data_ptr(),
      H, Nq, Nk, (float)scale,
      q.stride(0), q.stride(1), q.stride(2),
      k.stride(0), k.stride(1), k.stride(2),
      v.stride(0), v.stride(1), v.stride(2),
      dk.stride(0), dk.stride(1), dk.stride(2),
      dv.stride(0), dv.stride(1), dv.stride(2));
  HIP_CHECK_LAST();
}
