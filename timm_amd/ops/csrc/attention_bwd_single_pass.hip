// Single-pass fused attention BACKWARD for short key sequences (Nk <= 256),
// head_dim 64, bf16, gfx950 (CDNA4).
//
// One workgroup owns every key of one (batch, head) pair and sweeps the query
// rows in 32-row slices, so S = QK^T, dP = dO V^T, P and dS are computed once
// per (slice, 16-key tile) - five MFMA products per tile instead of the seven
// of the two-pass kernels in attention_bwd.hip - and no sum crosses
// workgroups: no float atomics, no second kernel, bit-reproducible.
//
//  * Wave w owns keys [32w, 32w+32) (two 16-key tiles).  K and V row fragments
//    of those keys live in registers for the whole kernel, and so do the fp32
//    accumulators of dK^T and dV^T ([d][key], 2 x 4 tiles each), which are
//    stored once at the end.  16-key tiles wholly beyond Nk are skipped with a
//    wave-uniform branch.
//  * S and dP are computed with the key on the MFMA lane (A = Q / dO rows,
//    B = K / V rows), so the C-layout accumulators of two 16-row q tiles
//    are, packed to bf16, already the B operand of dV^T += dO^T P and
//    dK^T += Q^T dS (k index = query row, in the permuted order
//    {4g..4g+3, 16+4g..16+4g+3} that the transposed reads of Q / dO follow).
//  * Q and dO of a slice are staged once into one swizzled LDS image each and
//    read by rows (ds_read_b128) for S / dP and by columns
//    (ds_read_b64_tr_b16) for dK^T / dV^T: no second, transposed copy.
//  * dS crosses LDS once, as a [key][q] image written 8 bytes per lane from
//    the C layout.  After one barrier every wave takes 16x16 sub-tiles of the
//    slice's dQ over ALL keys (A = dS by transposed read, B = K^T fragments
//    held in registers) and stores them through the dq strides.
//  * The global loads of slice i+1 (Q, dO, O, LSE) are issued before slice i
//    computes and written to LDS after its dS barrier (issue-early /
//    write-late): one LDS buffer, two barriers per slice (dS hand-over and
//    staged-slice visibility).
//  * delta = rowsum(dO o O) is formed while the slice is staged when the
//    caller passes O instead of a precomputed delta, reading dO and O through
//    their strides - attn_bwd_preprocess and its contiguous dO copy are then
//    not needed.
//
// Mask semantics are those of the two-pass kernels: optional additive fp32
// mask [mB, H|1, Nq, Nk] read as mask[b % mB]; -inf gives p = 0 without NaN;
// LSE is the forward's natural-log value; rows / columns beyond Nq / Nk
// contribute nothing and are never stored.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef short short4_t __attribute__((ext_vector_type(4)));
typedef short short8_t __attribute__((ext_vector_type(8)));
typedef int int2_t __attribute__((ext_vector_type(2)));

constexpr float kNegInf = -1e30f;
constexpr int kSlice = 32;   // query rows per slice

// [rows][64] bf16 image, 128-byte rows.  The 16-byte chunk index is XORed
// with an even function of the row so that the row reads (ds_read_b128) and
// the transposed reads (8-byte pieces, pairs stay together) of 8 consecutive
// rows are bank-conflict-free.
__device__ __forceinline__ int img_off(int row, int chunk) {
  return row * 128 + ((chunk ^ (((row >> 1) & 3) << 1)) << 4);
}

// [keys][32 q] bf16 image of dS^T, 64-byte rows, in 8-byte pieces (4 q rows).
// Rows 8..15 of every 16 swap the two 32-byte halves: the transposed read
// takes rows {n..n+3, n+8..n+11} in one 32-lane group.
__device__ __forceinline__ int ds_off(int key, int piece) {
  return key * 64 + ((piece ^ (((key >> 3) & 1) << 2)) << 3);
}

// Two ds_read_b64_tr_b16 -> one 16x16x32 operand fragment.  Every lane of the
// wave must be active (wave-uniform control flow only around this).
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

struct Strides3 { long sb, sh, sn; };

template <int kWaves, bool kHasMask>
// 4 and 8 waves: <= 256 registers, two waves per SIMD.  The 2-wave variant
// stages four chunks per thread and would spill under that cap.
__global__ __launch_bounds__(kWaves * 64, kWaves >= 4 ? 2 : 1)
void attn_bwd_single_pass_kernel(
    const __bf16* __restrict__ q,        // [B,H,Nq,64] strided
    const __bf16* __restrict__ k,        // [B,H,Nk,64] strided
    const __bf16* __restrict__ v,        // [B,H,Nk,64] strided
    const __bf16* __restrict__ dov,      // [B,H,Nq,64] strided
    const __bf16* __restrict__ ov,       // [B,H,Nq,64] strided, or null with delta_in
    const float* __restrict__ lse,       // [B,H,Nq]
    const float* __restrict__ delta_in,  // [B,H,Nq] or null: computed from dO, O
    const float* __restrict__ mask,      // [mB,H|1,Nq,Nk] or null
    __bf16* __restrict__ dq, __bf16* __restrict__ dk, __bf16* __restrict__ dv,
    int H, int Nq, int Nk, float scale,
    int mB, long m_sb, long m_sh,
    Strides3 qs, Strides3 ks, Strides3 vs, Strides3 dos, Strides3 os,
    Strides3 dqs, Strides3 dks, Strides3 dvs) {
  constexpr int kT = kWaves * 64;
  constexpr int kKeys = kWaves * 32;
  constexpr int kStageIt = (2 * kSlice * 8) / kT;  // 16-byte chunks of Q + dO per thread
  constexpr int kDqTiles = 8 / kWaves;             // 16x16 dQ tiles per wave and slice
  static_assert(kWaves == 2 || kWaves == 4 || kWaves == 8, "2, 4 or 8 waves");

  __shared__ __attribute__((aligned(16))) char k_img[kKeys * 128];
  __shared__ __attribute__((aligned(16))) char qdo_img[2][kSlice * 128];  // Q, dO
  __shared__ __attribute__((aligned(16))) char ds_img[kKeys * 64];
  __shared__ __attribute__((aligned(16))) float lse_s[kSlice];
  __shared__ __attribute__((aligned(16))) float delta_s[kSlice];

  const int bh = blockIdx.x;
  const int b = bh / H;
  const int h = bh % H;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);  // scalar: uniform branches
  const int lane = tid % WAVE_SIZE;
  const int l16 = lane & 15;
  const int g4 = lane >> 4;
  const int tq = l16 >> 2;  // transposed read: row of the 4-row block
  const int tp = l16 & 3;   // transposed read: 8-byte piece of the 16 columns

  const __bf16* q_bh = q + b * qs.sb + h * qs.sh;
  const __bf16* k_bh = k + b * ks.sb + h * ks.sh;
  const __bf16* v_bh = v + b * vs.sb + h * vs.sh;
  const __bf16* do_bh = dov + b * dos.sb + h * dos.sh;
  const __bf16* o_bh = delta_in ? nullptr : ov + b * os.sb + h * os.sh;
  const float* lse_bh = lse + (long)bh * Nq;
  const float* delta_bh = delta_in ? delta_in + (long)bh * Nq : nullptr;
  const float* mask_bh = kHasMask ? mask + (long)(b % mB) * m_sb + (long)h * m_sh : nullptr;

  const int n_tiles = (Nk + 15) / 16;     // 16-key tiles with a valid key
  const int n_ksteps = (n_tiles + 1) / 2;  // 32-key steps of the dQ product
  const int n_slices = (Nq + kSlice - 1) / kSlice;

  // ---- slice staging: issue-early (registers) / write-late (LDS) ----
  bf16x8_t pre_a[kStageIt], pre_o[kStageIt];
  float pre_lse = 0.f, pre_delta = 0.f;
  auto issue_slice = [&](int q0) {
#pragma unroll
    for (int it = 0; it < kStageIt; ++it) {
      const int c = it * kT + tid;
      const int which = (it * kT + wave * WAVE_SIZE) >> 8;  // 0: Q, 1: dO (scalar)
      const int qrow = q0 + ((c & 255) >> 3);
      const int c8 = c & 7;
      pre_a[it] = bf16x8_t{};
      pre_o[it] = bf16x8_t{};
      // one load instruction for both tensors (scalar select of base and
      // pitch): two loads into the same registers would make the compiler
      // wait between them
      const __bf16* src = which == 0 ? q_bh : do_bh;
      const long src_sn = which == 0 ? qs.sn : dos.sn;
      if (qrow < Nq) {
        pre_a[it] = *reinterpret_cast<const bf16x8_t*>(src + qrow * src_sn + c8 * 8);
        if (which == 1 && !delta_in) {
          pre_o[it] = *reinterpret_cast<const bf16x8_t*>(o_bh + qrow * os.sn + c8 * 8);
        }
      }
    }
    if (tid < kSlice) {
      const int qrow = q0 + tid;
      pre_lse = (qrow < Nq) ? lse_bh[qrow] : 0.f;
      pre_delta = (delta_in && qrow < Nq) ? delta_bh[qrow] : 0.f;
    }
  };
  auto commit_slice = [&]() {
#pragma unroll
    for (int it = 0; it < kStageIt; ++it) {
      const int c = it * kT + tid;
      const int which = (it * kT + wave * WAVE_SIZE) >> 8;
      const int row = (c & 255) >> 3;
      const int c8 = c & 7;
      *reinterpret_cast<bf16x8_t*>(qdo_img[which] + img_off(row, c8)) = pre_a[it];
      if (which == 1 && !delta_in) {
        // delta = rowsum(dO o O): 8 lanes per row, as attn_bwd_preprocess
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += (float)pre_a[it][j] * (float)pre_o[it][j];
        acc += __shfl_xor(acc, 4, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 1, 64);
        if (c8 == 0) delta_s[row] = acc;
      }
    }
    if (tid < kSlice) {
      lse_s[tid] = pre_lse;
      if (delta_in) delta_s[tid] = pre_delta;
    }
  };

  // ---- prologue: K image, dS image zero-fill, V fragments, slice 0 ----
  issue_slice(0);
#pragma unroll
  for (int it = 0; it < (kKeys * 8) / kT; ++it) {
    const int c = it * kT + tid;
    const int row = c >> 3, c8 = c & 7;
    bf16x8_t val = {};
    if (row < Nk) val = *reinterpret_cast<const bf16x8_t*>(k_bh + row * ks.sn + c8 * 8);
    *reinterpret_cast<bf16x8_t*>(k_img + img_off(row, c8)) = val;
  }
  // tiles beyond Nk are never written again: their dS stays zero for the
  // 32-key step they share with a valid tile
#pragma unroll
  for (int it = 0; it < (kKeys * 64) / (kT * 16); ++it) {
    *reinterpret_cast<bf16x8_t*>(ds_img + (it * kT + tid) * 16) = bf16x8_t{};
  }
  bf16x8_t v_reg[2][2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = wave * 32 + kt * 16 + l16;
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
      v_reg[kt][ds] = bf16x8_t{};
      if (key < Nk) {
        v_reg[kt][ds] = *reinterpret_cast<const bf16x8_t*>(
            v_bh + key * vs.sn + ds * 32 + g4 * 8);
      }
    }
  }
  commit_slice();
  __syncthreads();

  // K row fragments of this wave's keys (B operand of S = Q K^T)
  bf16x8_t k_reg[2][2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
      k_reg[kt][ds] = lds_b128(k_img, img_off(wave * 32 + kt * 16 + l16, ds * 4 + g4));
    }
  }
  // K^T fragments of this wave's dQ tiles over all keys (B operand of dS K)
  bf16x8_t kt_reg[kDqTiles][kWaves];
#pragma unroll
  for (int t = 0; t < kDqTiles; ++t) {
    const int dt = (wave * kDqTiles + t) & 3;
#pragma unroll
    for (int s = 0; s < kWaves; ++s) {
      const int row = s * 32 + g4 * 8 + tq;
      kt_reg[t][s] = tr_pair(k_img,
          img_off(row, dt * 2 + (tp >> 1)) + 8 * (tp & 1),
          img_off(row + 4, dt * 2 + (tp >> 1)) + 8 * (tp & 1));
    }
  }

  f32x4 acc_dk[2][4], acc_dv[2][4];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      acc_dk[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc_dv[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  const char* q_img = qdo_img[0];
  const char* do_img = qdo_img[1];

  // dQ of a slice is held as bf16 and stored at the top of the NEXT slice,
  // ahead of that slice's prefetch loads: a wait for the stores (the compiler
  // adds one before it reuses their data registers) then never covers the
  // younger loads, and the stores drain under the S / dP products.
  bf16x4_t dq_hold[kDqTiles] = {};
  __bf16* dq_bh = dq + b * dqs.sb + h * dqs.sh;
  auto store_dq = [&](int q0) {
#pragma unroll
    for (int t = 0; t < kDqTiles; ++t) {
      const int id = wave * kDqTiles + t;
      const int qt = id >> 2, dt = id & 3;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + qt * 16 + g4 * 4 + r;
        if (qrow < Nq) dq_bh[qrow * dqs.sn + dt * 16 + l16] = dq_hold[t][r];
      }
    }
  };

  // V fragments have landed before the loop: no wait for them inside it,
  // where it would also wait for the prefetch just issued
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), as an instruction the compiler tracks

  for (int sl = 0; sl < n_slices; ++sl) {
    const int q0 = sl * kSlice;
    const bool has_next = sl + 1 < n_slices;
    if (sl > 0) store_dq(q0 - kSlice);
    if (has_next) issue_slice(q0 + kSlice);

    // ---- S, dP, P, dS once per (slice, key tile); dV^T, dK^T ----
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if (wave * 2 + kt >= n_tiles) continue;  // wave-uniform
      const int key = wave * 32 + kt * 16 + l16;
      bf16x8_t p_frag, ds_frag;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        f32x4 acc_s = {0.f, 0.f, 0.f, 0.f};
        f32x4 acc_dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ds = 0; ds < 2; ++ds) {
          const int off = img_off(qt * 16 + l16, ds * 4 + g4);
          acc_s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              lds_b128(q_img, off), k_reg[kt][ds], acc_s, 0, 0, 0);
          acc_dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              lds_b128(do_img, off), v_reg[kt][ds], acc_dp, 0, 0, 0);
        }
        // C layout: q row = qt*16 + g4*4 + r, key on the lane
        const f32x4 lse_r = *reinterpret_cast<const f32x4*>(&lse_s[qt * 16 + g4 * 4]);
        const f32x4 delta_r = *reinterpret_cast<const f32x4*>(&delta_s[qt * 16 + g4 * 4]);
        bf16x4_t ds4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow = q0 + qt * 16 + g4 * 4 + r;
          float s = acc_s[r] * scale;
          if (key >= Nk || qrow >= Nq) {
            s = kNegInf;
          } else if (kHasMask) {
            s += mask_bh[(long)qrow * Nk + key];
            if (s < kNegInf) s = kNegInf;
          }
          const float p = (s <= kNegInf) ? 0.f : __expf(s - lse_r[r]);
          const float dsv = p * (acc_dp[r] - delta_r[r]) * scale;
          p_frag[qt * 4 + r] = (__bf16)p;
          ds_frag[qt * 4 + r] = (__bf16)dsv;
          ds4[r] = (__bf16)dsv;
        }
        *reinterpret_cast<bf16x4_t*>(ds_img + ds_off(key, qt * 4 + g4)) = ds4;
      }
      // dV^T[d][key] += dO^T[d][q] P[q][key], dK^T[d][key] += Q^T[d][q] dS[q][key]
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int off0 = img_off(g4 * 4 + tq, dt * 2 + (tp >> 1)) + 8 * (tp & 1);
        const int off1 = img_off(16 + g4 * 4 + tq, dt * 2 + (tp >> 1)) + 8 * (tp & 1);
        acc_dv[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            tr_pair(do_img, off0, off1), p_frag, acc_dv[kt][dt], 0, 0, 0);
        acc_dk[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            tr_pair(q_img, off0, off1), ds_frag, acc_dk[kt][dt], 0, 0, 0);
      }
    }
    __syncthreads();  // dS of the slice complete; Q / dO image no longer read

    // Next slice to LDS first: its loads were issued before S / dP.  The dQ
    // registers stored at the top of this slice stay pinned until this wait
    // has passed, so that reusing them needs no earlier wait of its own.
    // (the wait is unconditional so that no load counts as pending at the
    // top of the next slice, where a wait would cover the fresh dQ stores)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    if (has_next) commit_slice();
#pragma unroll
    for (int t = 0; t < kDqTiles; ++t) {
      const int2_t pin = __builtin_bit_cast(int2_t, dq_hold[t]);
      __asm__ volatile("" :: "v"(pin.x), "v"(pin.y));
    }

    // ---- dQ: each wave takes 16x16 tiles over all keys ----
#pragma unroll
    for (int t = 0; t < kDqTiles; ++t) {
      const int qt = (wave * kDqTiles + t) >> 2;
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int s = 0; s < kWaves; ++s) {
        if (s >= n_ksteps) break;  // wave-uniform
        const int krow = s * 32 + g4 * 8 + tq;
        const bf16x8_t a = tr_pair(ds_img, ds_off(krow, qt * 4 + tp), ds_off(krow + 4, qt * 4 + tp));
        acc[s & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, kt_reg[t][s], acc[s & 1], 0, 0, 0);
      }
      const f32x4 sum = acc[0] + acc[1];
#pragma unroll
      for (int r = 0; r < 4; ++r) dq_hold[t][r] = (__bf16)sum[r];
    }

    __syncthreads();  // next slice staged; dS image free
  }
  store_dq((n_slices - 1) * kSlice);

  // ---- dK, dV: C layout holds [d = dt*16 + g4*4 + r][key = lane] ----
  __bf16* dk_bh = dk + b * dks.sb + h * dks.sh;
  __bf16* dv_bh = dv + b * dvs.sb + h * dvs.sh;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const int key = wave * 32 + kt * 16 + l16;
    if (key >= Nk) continue;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x4_t k4, v4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        k4[r] = (__bf16)acc_dk[kt][dt][r];
        v4[r] = (__bf16)acc_dv[kt][dt][r];
      }
      *reinterpret_cast<bf16x4_t*>(dk_bh + key * dks.sn + dt * 16 + g4 * 4) = k4;
      *reinterpret_cast<bf16x4_t*>(dv_bh + key * dvs.sn + dt * 16 + g4 * 4) = v4;
    }
  }
}

Strides3 strides3(const at::Tensor& t) { return {t.stride(0), t.stride(1), t.stride(2)}; }

bool aligned16(const at::Tensor& t) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 != 0 || t.stride(3) != 1) return false;
  for (int i = 0; i < 3; ++i) {
    if (t.stride(i) % 8 != 0) return false;
  }
  return true;
}

}  // namespace

// Single-pass fused backward for Nk <= 256, head_dim 64.  q/k/v/dO/O strided
// [B,H,N,64] with head_dim contiguous and 16-byte-aligned rows; lse fp32
// [B,H,Nq] contiguous.  Pass either `o` (delta is formed in the kernel) or a
// precomputed contiguous fp32 `delta` [B,H,Nq].  dq/dk/dv are preallocated by
// the caller (possibly views into a packed [B,N,3,H,D] dqkv buffer).
void attention_bwd_single_pass(at::Tensor q, at::Tensor k, at::Tensor v,
                               at::Tensor dov, c10::optional<at::Tensor> o,
                               at::Tensor lse, c10::optional<at::Tensor> delta,
                               c10::optional<at::Tensor> mask,
                               at::Tensor dq, at::Tensor dk, at::Tensor dv,
                               double scale) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.scalar_type() == at::kBFloat16);
  TORCH_CHECK(k.is_cuda() && k.dim() == 4 && k.scalar_type() == at::kBFloat16 &&
              v.is_cuda() && v.dim() == 4 && v.scalar_type() == at::kBFloat16 &&
              dov.is_cuda() && dov.dim() == 4 && dov.scalar_type() == at::kBFloat16 &&
              dq.is_cuda() && dq.scalar_type() == at::kBFloat16 &&
              dk.is_cuda() && dk.scalar_type() == at::kBFloat16 &&
              dv.is_cuda() && dv.scalar_type() == at::kBFloat16);
  const int B = q.size(0), H = q.size(1), Nq = q.size(2), D = q.size(3);
  const int Nk = k.size(2);
  TORCH_CHECK(D == 64, "attention_bwd_single_pass: head_dim must be 64");
  TORCH_CHECK(Nk >= 1 && Nk <= 256, "attention_bwd_single_pass: 1 <= Nk <= 256");
  TORCH_CHECK(k.size(0) == B && k.size(1) == H && k.size(3) == D &&
              v.sizes() == k.sizes() && dov.sizes() == q.sizes() &&
              dq.sizes() == q.sizes() && dk.sizes() == k.sizes() && dv.sizes() == k.sizes(),
              "attention_bwd_single_pass: shapes disagree");
  TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(dov) &&
              aligned16(dq) && aligned16(dk) && aligned16(dv),
              "attention_bwd_single_pass: head_dim contiguous, 16-byte-aligned rows");
  const long rows = (long)B * H * Nq;
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() && lse.scalar_type() == at::kFloat &&
              lse.numel() == rows, "attention_bwd_single_pass: lse fp32 [B,H,Nq]");
  TORCH_CHECK(o.has_value() != delta.has_value(),
              "attention_bwd_single_pass: pass exactly one of o and delta");
  if (o.has_value()) {
    TORCH_CHECK(o->is_cuda() && o->scalar_type() == at::kBFloat16 &&
                o->sizes() == q.sizes() && aligned16(*o));
  } else {
    TORCH_CHECK(delta->is_cuda() && delta->is_contiguous() &&
                delta->scalar_type() == at::kFloat && delta->numel() == rows);
  }
  int mB = 1;
  long m_sb = 0, m_sh = 0;
  if (mask.has_value()) {
    TORCH_CHECK(mask->is_cuda() && mask->dim() == 4 && mask->is_contiguous() &&
                mask->scalar_type() == at::kFloat);
    TORCH_CHECK(mask->size(0) >= 1 && B % mask->size(0) == 0 &&
                (mask->size(1) == H || mask->size(1) == 1) &&
                mask->size(2) == Nq && mask->size(3) == Nk);
    mB = (int)mask->size(0);
    m_sb = mB == 1 ? 0 : mask->size(1) * (long)Nq * Nk;
    m_sh = mask->size(1) == 1 ? 0 : (long)Nq * Nk;
  }
  if (rows == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  const at::Tensor& o_or_do = o.has_value() ? *o : dov;

  auto run = [&](auto kern, int waves) {
    hipLaunchKernelGGL(kern, dim3(B * H), dim3(waves * 64), 0, stream,
        (const __bf16*)q.data_ptr(), (const __bf16*)k.data_ptr(), (const __bf16*)v.data_ptr(),
        (const __bf16*)dov.data_ptr(),
        o.has_value() ? (const __bf16*)o->data_ptr() : (const __bf16*)nullptr,
        lse.data_ptr<float>(),
        delta.has_value() ? delta->data_ptr<float>() : (const float*)nullptr,
        mask.has_value() ? mask->data_ptr<float>() : (const float*)nullptr,
        (__bf16*)dq.data_ptr(), (__bf16*)dk.data_ptr(), (__bf16*)dv.data_ptr(),
        H, Nq, Nk, (float)scale, mB, m_sb, m_sh,
        strides3(q), strides3(k), strides3(v), strides3(dov), strides3(o_or_do),
        strides3(dq), strides3(dk), strides3(dv));
  };
  const bool has_mask = mask.has_value();
  // 32 keys per wave: the smallest workgroup that holds every key
  if (Nk <= 64) {
    if (has_mask) run(attn_bwd_single_pass_kernel<2, true>, 2);
    else run(attn_bwd_single_pass_kernel<2, false>, 2);
  } else if (Nk <= 128) {
    if (has_mask) run(attn_bwd_single_pass_kernel<4, true>, 4);
    else run(attn_bwd_single_pass_kernel<4, false>, 4);
  } else {
    if (has_mask) run(attn_bwd_single_pass_kernel<8, true>, 8);
    else run(attn_bwd_single_pass_kernel<8, false>, 8);
  }
  HIP_CHECK_LAST();
}
