// TinyECG declarations shared by the training step (kernels/tiny_ecg_step.hip), the close of a cohort round
// (kernels/tiny_ecg_close.hip) and the evaluation kernel (kernels/tiny_ecg_eval.hip): the flat parameter layout, the
// prepared-fragment image, the cohort stride, the Philox rounds and the small device helpers they use.
#pragma once
#include "ecg_common.h"

namespace ecg {
namespace tiny {

constexpr int C = 16;   // hidden channels
constexpr int K1 = 7;   // conv1 taps (padding 3)
constexpr int K2 = 5;   // conv2 taps (padding 2)
constexpr int MAX_CLASSES = 16;

struct Layout {
  int w1, b1, w2, b2, wh, bh, P;
};

__host__ __device__ inline Layout make_layout(int nc) {
  Layout l;
  l.w1 = 0;
  l.b1 = C * K1;             // 112
  l.w2 = l.b1 + C;           // 128
  l.b2 = l.w2 + C * C * K2;  // 1408
  l.wh = l.b2 + C;           // 1424
  l.bh = l.wh + nc * C;
  l.P = l.bh + nc;
  return l;
}

// A raw buffer resource over exactly ``bytes`` bytes at ``p``: accesses at or past its end are dropped / read 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// Plain (cached) bounded load: a byte offset at or past the resource's size reads 0.  Callers keep every offset
// non-negative and below 2^31 so no sum of offsets wraps.
__device__ __forceinline__ float ld_bounded(__amdgpu_buffer_rsrc_t r, int byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

// ---- prepared fragments (PF, bf16 path): the conv operands of the flat fp32 parameters in MFMA lane order,
// kept in a small global image instead of being rebuilt in every workgroup's LDS every step.
//   WP_FRAGF  bf16 [3][64][8]  conv2 forward operand   (element (r, co), r = 16k + ci, as put_param's fragF)
//   WP_FRAGD  bf16 [3][64][8]  conv2 dgrad operand     (element (r, ci), r = 16k + co)
//   WP_AW1    bf16 [16][8]     conv1 A operand row c: {w1[c][0..6], b1[c]}
//   WP_B2     fp32 [16]        conv2 bias (byte offset WP_B2_BYTE)
// tiny_prep_kernel writes the whole image from the flat parameters (ecg_tiny_prep and the gradient-only / forward
// entry points), and slab_reduce_sgd_kernel's SGD epilogue rewrites each updated parameter's slots.  A round has
// no prep launch: a FedAvg all-reduce / broadcast / checkpoint load may have rewritten the weights since the last
// one, so its first step builds its operands in LDS and that step's SGD epilogue rewrites the whole image.  From
// then on the image equals what put_param would have built from ``params`` - bitwise the same MFMA operands - and
// every step workgroup loads its operands straight into VGPRs (7 x 16 B per lane, L2-hot: all 32 workgroups of
// an XCD read the same 6.4 KB): no per-step scatter into LDS (1,280 x 2 two-byte stores + conversions per
// sample) and no LDS round trip for the fragments in conv1 / conv2 / dgrad.
constexpr int WP_FRAGF = 0;
constexpr int WP_FRAGD = 3 * 64 * 8;
constexpr int WP_AW1 = 2 * 3 * 64 * 8;
constexpr int WP_B2_BYTE = (WP_AW1 + C * 8) * 2;  // 6400
constexpr int WP_BYTES = WP_B2_BYTE + C * 4;     // 6464
constexpr int kParamsW2End = C * K1 + C + C * C * K2;  // == make_layout(nc).b2 for every nc (1408)

// conv2's bias rides in the MFMA: reduction row r = 80 (tap 5 = K padding, ci 0) of the forward operand holds
// bf16(b2[co]) and the matching B-operand row is a constant 1 (autocast semantics: the bias of a bf16 conv is bf16
// too), so the epilogue adds nothing.  Element (r = 80, co) of fragF: fragment s = 2, lane 32 + co, slot j = 0.
__host__ __device__ constexpr int frag_bias_elem(int co) { return (2 * 64 + 32 + co) * 8; }

// Broadcast lane ``src``'s value to the whole wave (v_readlane_b32: the result is an SGPR; src wave-uniform).
__device__ __forceinline__ float lane_bcast(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// Sum over the 16 lanes of a DPP row (inclusive row_shr scan 1, 2, 4, 8; out-of-row sources read 0):
// lane 15 of each row ends with the row's total.
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
  return v;
}

// Floats between two clients' weights (and momenta) in a cohort's ``params`` / ``mom``: >= P, a multiple of 64.
__host__ __device__ constexpr int cohort_pstride(int P) { return (P + 63) / 64 * 64; }

// Philox4x32-10 (Salmon et al., SC'11): the counter-based generator behind both DP noise streams (dp_normal in
// kernels/tiny_ecg_step.hip, cohort_dp_normal in kernels/tiny_ecg_close.hip; utils/philox.py is the host twin).
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

}  // namespace tiny
}  // namespace ecg

// Build the prepared-fragment image of ``params`` (defined in kernels/tiny_ecg_step.hip).
ECG_API int ecg_tiny_prep(const float* params, void* wprep, hipStream_t stream);
