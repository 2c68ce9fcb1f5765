// Fused TinyECG training step for gfx950 (MI355X, CDNA4).
//
// One workgroup owns one ECG window and runs the WHOLE per-sample training computation out of LDS:
//   gather x[idx[b]]  ->  conv1(1->16,k7,p3)+bias+ReLU (bf16: MFMA, each wave builds its im2col operand in
//   registers straight from the global window row, no LDS copy of the window; fp32: VALU over the window staged in
//   LDS)  ->  conv2(16->16,k5,p2)+bias+ReLU
//   (MFMA bf16 16x16x32, implicit GEMM M=t, N=c_out, K=(tap,c_in)=80->96)  ->  mean-pool  ->
//   Linear(16->C)  ->  softmax-CE  ->  head grads  ->  dconv2 wgrad (MFMA, dh2 kept in the MFMA
//   accumulator layout and used directly as the A operand; h1 read as the B operand with the gfx950
//   transposing LDS read ds_read_b64_tr_b16)  ->  dconv2 dgrad (MFMA)  ->  ReLU mask  ->  dconv1 wgrad.
// The sample's parameter gradient (1,458 floats for C=2) plus its loss form one row.  The rows of a step are
// summed and SGD+momentum is applied to the flat fp32 master weights by a second launch
// (``slab_reduce_sgd_kernel``); a local round's launches are captured into one hipGraph and replayed.
// The reduce launch of step s also gathers step s + 1's windows (GatherArgs: otherwise idle CUs), both as fp32 rows
// (xg) and as packed bf16 rows with the conv padding written out as zeros (xbg, kPackLead); a round's steps s > 0 run
// the PK variant of the step kernel, whose conv1 operand is one 16-byte load of such a row and a one-element shift -
// conversion, edge shifts and bounds handling are done once per element by the gather, not 7 times per step here.
// The dataset itself does not change while a trainer lives, so it can be packed once (tiny_pack_rows_kernel, xpk): the
// gather blocks then only copy packed rows (kPrepackGather), or there is no gather at all and the PK kernel loads
// idx[b] and reads its row from the packed dataset (MODE 4, kPrepackDirect - the default of FusedTinyTrainer: 9.45-9.52
// against 9.76-9.81 us/step with the per-step gather, 9.58-9.64 with the copying gather; profiles/r15/tiny_prepacked.txt).
// (One launch per step with an in-kernel last-arriver reduction tree and one persistent launch per round were
// measured slower - 13.23 and 16.33 vs 10.62 us/step, profiles/r4/tiny_phase_diag.txt - and were removed in round 5.)
//
// Reference semantics being reproduced (per step): Module_3/TRUE_FL_M3/part3_fedavg_overlap_mpi_gpu.py:103-132
// (train_step_G0/G1: fwd, cross_entropy(mean), backward, SGD(lr=1e-2, momentum=0.9).step()) on the
// TinyECG of Module_3/tiny_ecg_model.py:8-29, with batches drawn as in Module_3/shard_dataset.py:118-136.
// Precision: bf16 MFMA operands, fp32 accumulation, fp32 master weights/optimizer state (native bf16 AMP).
#include "../include/ecg_common.h"
#include "../include/tiny_ecg.h"
#include "../include/tiny_ecg_close.h"

#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

// Layout / make_layout, the WP_* image offsets, frag_bias_elem, the class / tap constants and the bounded-load and
// lane helpers: include/tiny_ecg.h (shared with the evaluation kernel)
using namespace ecg::tiny;

constexpr int MAX_PAIRS_PER_WAVE = 4;  // mask bits: 4 pairs x 2 tiles x 4 rows = 32 bits

// LDS carve (bytes), all offsets multiples of 16.  fp32: the window xs, then the activations; bf16 has no xs (conv1
// reads the window from global memory) and starts with the conv1 im2col rows xcol, kept for the conv1 wgrad.
struct Smem {
  int Lp;  // L rounded up to 32 (tile pairs)
  int xs_off, xcol_off, h1_off, dh2_off, ps_off, frag_off, red_off, bytes;
};

// red region (floats): per-wave partials are written with plain stores and summed after a barrier
// (deterministic; no LDS float atomics).
constexpr int RED_G = 0;       // [16] dL/dh2 scale per channel (dpooled / L), written by the head
constexpr int RED_POOLED = 16; // [16] pooled features
constexpr int RED_POOL = 48;   // [WAVES][16] pooled partials

// Per-launch options of the step kernel.
struct FusedOpt {
  int slab_wt;  // store the gradient rows write-through (sc1): they leave the XCD L2s while the step runs
};
// conv2 wgrad work split: 5 taps x msplit(WAVES) pair ranges, one (tap, range) per wave 1.. (wave 0 runs the head)
__host__ __device__ constexpr int msplit(int waves) { return (waves - 1) / 5 < 1 ? 1 : (waves - 1) / 5; }
__host__ __device__ constexpr int red_cnt(int waves) { return RED_POOL + waves * 16; }      // relu'(h2) counts: [msplit][16] (bf16), [WAVES][16] (fp32)
__host__ __device__ constexpr int red_m(int waves) { return red_cnt(waves) + waves * 16; }  // [msplit][16*16*5] M partials
__host__ __device__ constexpr int red_dw1(int waves) { return red_m(waves) + msplit(waves) * 1280; }  // [WAVES][16][8]
__host__ __device__ constexpr int red_head(int waves) { return red_dw1(waves) + waves * 128; }  // dWh, dbh, loss
__host__ __device__ constexpr int red_floats(int waves) { return red_head(waves) + 288; }

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Write-through (sc1) global accesses for data handed between workgroups inside one launch: the
// stores need no release fence and the sc1 loads need no acquire fence (MI355X guide, Guideline 16 R1).
__device__ __forceinline__ void st_wt(__amdgpu_buffer_rsrc_t r, int idx, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, idx * 4, 0, 16);
}
__device__ __forceinline__ void st_wt4(__amdgpu_buffer_rsrc_t r, int idx, f32x4 v) {  // idx: float index, 16-B aligned
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), r, idx * 4, 0, 16);
}
__device__ __forceinline__ void st_wt_b128(__amdgpu_buffer_rsrc_t r, int byte_off, u32x4 v) {  // 16-byte aligned
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), r, byte_off, 0, 16);
}
__device__ __forceinline__ void st_wt_b64(__amdgpu_buffer_rsrc_t r, int byte_off, u32x2 v) {  // 8-byte aligned
  __builtin_amdgcn_raw_buffer_store_b64(v, r, byte_off, 0, 16);
}
__device__ __forceinline__ void st_wt_b16(__amdgpu_buffer_rsrc_t r, int byte_off, unsigned short v) {
  __builtin_amdgcn_raw_buffer_store_b16(v, r, byte_off, 0, 16);
}
__device__ __forceinline__ float ld_wt(__amdgpu_buffer_rsrc_t r, int idx) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, idx * 4, 0, 16));
}
constexpr int kOobByte = 0x40000000;  // past every window row (L <= 1024 floats), far from wrapping with + 4j

// Packed bf16 window rows (``xbg``, written by the gather blocks of the reduce launches, read by the PK step kernel):
//   [kPackLead zeros][bf16(x[0 .. L-1])][zeros up to ldb],  ldb = Lp + 8 (Lp = L rounded up to 32).
// Step t's conv1 window x[t-3 .. t+3] is elements t + kPackLead - 3 .. t + kPackLead + 3: the zeros on both sides are
// the conv padding, and the 8-element load of any step t < Lp, which starts at most one element lower, ends at element
// Lp + kPackLead + 3 < ldb at the latest.  Rows are 16-byte multiples, and a lead of 4 puts x[4j] on an 8-byte
// boundary (the gather's 4-float form stores 4 bf16 at once).
constexpr int kPackLead = 4;
__host__ __device__ constexpr int pack_ldb(int L) { return (L + 31) / 32 * 32 + 8; }

// fp32 path: v_mfma_f32_16x16x4_f32 (exact f32 products, K = 80 = 20 k-steps of 4, no padding)
constexpr int F32_KSTEPS = C * K2 / 4;

// the K-padding elements (r in [80, 96)) of a fragment set that stay zero: all of them except the bias row
__host__ __device__ constexpr bool frag_pad_is_bias(int which, int l, int j) { return which == 0 && j == 0 && l < 48; }

// Write flat parameter i's slots of the image (parameters past b2 - the head - have none).
__device__ __forceinline__ void wprep_put(unsigned char* wp, int i, float v) {
  __bf16* wb = reinterpret_cast<__bf16*>(wp);
  if (i < C * K1) {
    wb[WP_AW1 + (i / K1) * 8 + i % K1] = ecg::to_bf16(v);
  } else if (i < C * K1 + C) {
    wb[WP_AW1 + (i - C * K1) * 8 + 7] = ecg::to_bf16(v);
  } else if (i < kParamsW2End) {
    const int e = i - (C * K1 + C);
    const int co = e / (C * K2), ci = (e / K2) % C, k = e % K2;
    const int rf = 16 * k + ci, rd = 16 * k + co;
    const __bf16 bv = ecg::to_bf16(v);
    wb[WP_FRAGF + ((rf >> 5) * 64 + 16 * ((rf & 31) >> 3) + co) * 8 + (rf & 7)] = bv;
    wb[WP_FRAGD + ((rd >> 5) * 64 + 16 * ((rd & 31) >> 3) + ci) * 8 + (rd & 7)] = bv;
  } else if (i < kParamsW2End + C) {
    reinterpret_cast<float*>(wp + WP_B2_BYTE)[i - kParamsW2End] = v;
    wb[WP_FRAGF + frag_bias_elem(i - kParamsW2End)] = ecg::to_bf16(v);
  }
}

// One block: the whole prepared-fragment image from ``params`` (K padding rows r in [80, 96) zero).
__global__ __launch_bounds__(256) void tiny_prep_kernel(const float* __restrict__ params,
                                                        unsigned char* __restrict__ wp) {
  const int tid = threadIdx.x;
  for (int i = tid; i < kParamsW2End + C; i += 256) wprep_put(wp, i, params[i]);
  __bf16* wb = reinterpret_cast<__bf16*>(wp);
  for (int e = tid; e < 2 * 32 * 8; e += 256) {
    const int which = e >> 8, l = 32 + ((e >> 3) & 31), j = e & 7;
    if (!frag_pad_is_bias(which, l, j)) wb[(which ? WP_FRAGD : WP_FRAGF) + (2 * 64 + l) * 8 + j] = ecg::to_bf16(0.f);
  }
}

__host__ __device__ inline Smem make_smem(int L, int waves, int nc = MAX_CLASSES, bool f32 = false) {
  Smem s;
  s.Lp = (L + 31) / 32 * 32;
  s.xs_off = 0;
  // fp32: window xs[Lp + 16]; bf16: the conv1 im2col rows xcol[Lp + 1][8] (row Lp = zeros) and no xs
  s.xcol_off = s.xs_off + (f32 ? ((s.Lp + 16) * 4 + 15) / 16 * 16 : 0);
  s.h1_off = s.xcol_off + (f32 ? 0 : (s.Lp + 1) * 16);
  const int act_bytes = (s.Lp + 8) * C * (f32 ? 4 : 2);  // [Lp+8][16] in the activation type
  s.dh2_off = s.h1_off + act_bytes;
  s.ps_off = s.dh2_off + act_bytes;
  const int ps_bytes = ((make_layout(nc).P) * 4 + 15) / 16 * 16;
  // conv2 MFMA B fragments in lane order, fwd + dgrad: bf16 [2][3][64][8] or fp32 [2][20][64]
  s.frag_off = s.ps_off + ps_bytes;
  s.red_off = s.frag_off + (f32 ? 2 * F32_KSTEPS * 64 * 4 : 2 * 3 * 64 * 16);
  s.bytes = s.red_off + (red_floats(waves) * 4 + 15) / 16 * 16;
  return s;
}

__device__ __forceinline__ bf16x8 cat44(s16x4 a, s16x4 b) {
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 r;
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3];
  r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
  return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ s16x4 lds_tr16(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// ------------------------------------------------------------------------------------------------------------
// The per-sample computation (phases 0-5) of the per-step kernel.
//
// Backward algebra used (h2 = relu(conv2(h1)), pooled = mean_t h2, g[co] = dL/dpooled[co] / L):
//   dh2[t][co]       = g[co] * m[t][co]          with m = relu'(h2) in {0, 1} (exact in bf16)
//   dW2[co][ci][k]   = g[co] * M[co][ci][k],     M = sum_t m[t][co] h1[t+k-2][ci]   (needs no g)
//   db2[co]          = g[co] * sum_t m[t][co]
//   dh1[t][ci]       = sum_{co,k} m[t-k+2][co] * (g[co] w2[co][ci][k])   (g folded into the B operand)
// so the M MFMAs of waves 1.. run concurrently with the head on wave 0, and every MFMA operand that
// carries activation gradients is the exact 0/1 mask.
//
// bf16 path (AMP): every conv runs on MFMA with the TIME axis as the N dimension, so a lane's accumulator holds
// 4 consecutive channels of one time step and every epilogue is one 8-byte LDS access:
//   conv1       out^T[co][t] = W1ext[co][kk] x xcol[t][kk]   (kk < 7: taps, kk = 7: bias x "t < L", K padded to 32)
//   conv2       out^T[co][t] = W2[co][(k,ci)] x h1col[(k,ci)][t]
//   conv2 dgrad dh1^T[ci][t] = (g W2)[ci][(k,co)] x m[(k,co)][t], times relu'(h1), written over h1
//   conv1 wgrad dW1ext[ci][kk] = dh1^T[ci][t] x xcol[t][kk]   (both operands by transposing reads; kk = 7 -> db1)
// The fp32 path keeps conv1 / conv1-wgrad on VALU (exact f32) and the time-major MFMA orientation.
// LEAN (the MODE 4 kernels only): the same values by fewer vector instructions - conv1_operand_packed, the head wave's
// g broadcast and row_store; every other instantiation keeps its code (profiles/r19/step_isa_account.txt).
template <int WAVES, bool F32, bool PF = false, bool PK = false, bool LEAN = false>
struct TinySample {
  static_assert(!(PF && F32), "prepared fragments are bf16 operands");
  static_assert(!PK || PF, "packed window rows feed the prepared-fragment kernel only");
  static_assert(!LEAN || PK, "the lean forms are written for the packed-row kernel");
  using AT = std::conditional_t<F32, float, __bf16>;  // activation / MFMA operand type
  static constexpr int NT = WAVES * 64;
  Smem sm;
  Layout lay;
  int L, Lp, NP, nc;
  int tid, lane, w, h, c;  // h: lane quarter, c: channel owned by this lane in C-layout phases
  float* xs;               // fp32 path: [Lp + 16]: xs[i] = x[i - 3] (conv1 halo)
  __bf16* xcol;            // bf16 path: [Lp + 1][8]: {x[t-3..t+3], t < L} (0 for t >= L), row Lp = zeros;
                           // written by conv1 (a copy of its register operand), read by the conv1 wgrad
  AT* h1s;                 // row (t+2): h1[t][ci]
  AT* ms;                  // row (t+4): m[t][co] = relu'(h2) in {0,1}
  float* ps;               // fp32 copy of the flat params
  __bf16* fragF;           // [3][64][8] conv2 fwd B operand
  __bf16* fragD;           // [3][64][8] conv2 dgrad B operand
  float* fragF32;          // fp32 path: [20][64] fwd B operand
  float* fragD32;          // fp32 path: [20][64] dgrad B operand
  float* red;
  uint32_t mask1 = 0u;     // relu'(h1) bits of this lane's conv1 outputs (phase 1 -> phase 4)
  // PF: this lane's conv operands in registers, loaded from the global image (phase 0 / end of phase 2).
  // pf_aw (conv1's A operand) is register-resident in the LDS-built bf16 kernel too (load_aw).
  bf16x8 pf_aw, pf_wf[3], pf_wd[3];

  // LDS-built bf16 kernel: conv1's A operand row {w1[c][0..6], b1[c]} straight from the flat parameters (the same
  // bf16 values as the image's WP_AW1 row), so conv1 reads nothing that another thread staged.
  __device__ __forceinline__ void load_aw(const float* __restrict__ params) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = j < K1 ? params[lay.w1 + c * K1 + j] : params[lay.b1 + c];
      pf_aw[j] = ecg::to_bf16(h == 0 ? v : 0.f);
    }
  }

  __device__ __forceinline__ void pf_load_fwd(const unsigned char* __restrict__ wp) {
    const __bf16* wb = reinterpret_cast<const __bf16*>(wp);
    if (h == 0) {
      pf_aw = *reinterpret_cast<const bf16x8*>(wb + WP_AW1 + c * 8);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) pf_aw[j] = ecg::to_bf16(0.f);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) pf_wf[s] = *reinterpret_cast<const bf16x8*>(wb + WP_FRAGF + (s * 64 + lane) * 8);
  }
  __device__ __forceinline__ void pf_load_dgrad(const unsigned char* __restrict__ wp) {
    // only the head wave scales the dgrad fragments (head_and_M, right after g): wave 0 loads all three sets
    const __bf16* wb = reinterpret_cast<const __bf16*>(wp);
    if (w == 0) {
#pragma unroll
      for (int s = 0; s < 3; ++s) pf_wd[s] = *reinterpret_cast<const bf16x8*>(wb + WP_FRAGD + (s * 64 + lane) * 8);
    }
  }

  __device__ __forceinline__ TinySample(unsigned char* smem, int L_, int nc_)
      : sm(make_smem(L_, WAVES, nc_, F32)), lay(make_layout(nc_)), L(L_), nc(nc_) {
    Lp = sm.Lp;
    NP = Lp / 32;
    xs = reinterpret_cast<float*>(smem + sm.xs_off);
    xcol = reinterpret_cast<__bf16*>(smem + sm.xcol_off);
    h1s = reinterpret_cast<AT*>(smem + sm.h1_off);
    ms = reinterpret_cast<AT*>(smem + sm.dh2_off);
    ps = reinterpret_cast<float*>(smem + sm.ps_off);
    fragF = reinterpret_cast<__bf16*>(smem + sm.frag_off);
    fragD = fragF + 3 * 64 * 8;
    fragF32 = reinterpret_cast<float*>(smem + sm.frag_off);
    fragD32 = fragF32 + F32_KSTEPS * 64;
    red = reinterpret_cast<float*>(smem + sm.red_off);
    tid = threadIdx.x;
    lane = tid & 63;
    w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: w-derived bounds, taps and loops stay scalar
    h = lane >> 4;
    c = lane & 15;
  }

  // ---- phase 0: window, parameters, constant pads
  // fp32: the window goes global -> registers (load_x) -> LDS (put_x): xs elements i = tid + k*NT, one coalesced
  // load each.  bf16 stages no window: conv1_load below.
  static constexpr int XK = (32 * MAX_PAIRS_PER_WAVE * WAVES + 16 + NT - 1) / NT;
  struct XRegs {
    float v[XK];
  };
  __device__ __forceinline__ void load_x(const float* __restrict__ xrow, XRegs& r) const {
#pragma unroll
    for (int k = 0; k < XK; ++k) {
      const int i = tid + k * NT, t = i - 3;
      if (k * NT < Lp + 16) {  // wave-uniform; the load itself is clamped, never branched
        const float v = xrow[min(max(t, 0), L - 1)];
        r.v[k] = (i < Lp + 16 && t >= 0 && t < L) ? v : 0.f;
      }
    }
  }
  __device__ __forceinline__ void put_x(const XRegs& r) {
#pragma unroll
    for (int k = 0; k < XK; ++k) {
      const int i = tid + k * NT;
      if (i < Lp + 16) xs[i] = r.v[k];
    }
  }
  __device__ __forceinline__ void stage_x(const float* __restrict__ xrow) {
    XRegs r;
    load_x(xrow, r);
    put_x(r);
  }

  // bf16: the conv1 B operand of tile pair (pi, pi + 1) of this wave, fetched by the lanes that use it.  Lane n of
  // quarter 0 loads the 7 window floats x[t-3 .. t+3] of its time step t = 16*tile + n through ``xr``, a buffer
  // resource over exactly the row's L floats: elements past the row's end read 0 (the conv padding) without a
  // branch, and quarters 1..3 and steps t >= L (whose operand is all zero) load from an out-of-range offset.
  // Offsets never go negative: the three steps t < 3, whose window starts before the row, load x[0 .. 6] and
  // conv1_operand shifts their values into place (tile 0 only: every other wave skips that branch).
  // PK: the row is a packed bf16 row written by the gather blocks (gather_block, kPackLead) and ``xr`` covers all of it.
  struct X1f {
    float v[2][K1];
  };
  struct X1p {
    u32x4 p[2];  // the 8 packed bf16 of each tile's load
  };
  using X1 = std::conditional_t<PK, X1p, X1f>;
  __device__ __forceinline__ int conv1_t(int pi, int u) const {  // (clamped: the pair's second tile may not exist)
    return 16 * min(w + (pi + u) * WAVES, Lp / 16 - 1) + (lane & 15);
  }
  __device__ __forceinline__ void conv1_load(__amdgpu_buffer_rsrc_t xr, int pi, X1& r) const {
    if constexpr (PK) {
      // Packed row: step t's window x[t-3 .. t+3] is elements t + 1 .. t + 7 of the row.  One 16-byte
      // load of the 8 elements from the even element at or below t + 1 (a dword-aligned byte offset, which is all a
      // raw buffer load of any width needs - the unpacked kernel's x4 + x3 loads start at any float too); the row's
      // zero pads stand in for the conv padding on both sides, so no offset is clamped and nothing reads past the row.
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = conv1_t(pi, u);
        const int off = (h == 0 && t < L) ? 2 * ((t + kPackLead - 3) & ~1) : kOobByte;
        r.p[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
      }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = conv1_t(pi, u);
        const int base = (h == 0 && t < L) ? 4 * max(t - 3, 0) : kOobByte;
#pragma unroll
        for (int j = 0; j < K1; ++j) r.v[u][j] = ld_bounded(xr, base + 4 * j);
      }
    }
  }
  // The loaded values as the MFMA operand {bf16(x[t-3 .. t+3]), "t < L"} (all zero in quarters 1..3 and for t >= L).
  // PK: the same operand from the 8 packed bf16 ``d``: the window starts at element 0 or 1 of the load by the
  // parity of t (the lane's parity: tiles are 16 steps apart), so three funnel shifts move it down and one byte
  // permute puts the window's last element under the flag.  An out-of-range load is all zero and has no flag.
  __device__ __forceinline__ bf16x8 conv1_operand_packed(u32x4 d, int t) const {
    static_assert(kPackLead % 2 == 0, "the shift below assumes an even lead: window start t + kPackLead - 3");
    const unsigned flag = (h == 0 && t < L) ? 0x3f80u : 0u;  // bf16 1.0
    u32x4 o;
    if constexpr (LEAN) {
      // The shift count and the permute selector as lane-constant registers, computed by arithmetic: written as
      // selects (below), hipcc turns every funnel shift into a byte permute plus a select on the parity - two
      // instructions per dword where one v_alignbit_b32 with its count in a register does it.
      const unsigned sh = ((lane & 1u) ^ 1u) << 4;  // 16: t even, the window starts at element 1 of the load
#pragma unroll
      for (int i = 0; i < 3; ++i) o[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], sh);
      o[3] = __builtin_amdgcn_perm(flag, d[3], 0x05040100u + (sh >> 3) * 0x0101u);  // 0x05040302 when sh = 16
      return __builtin_bit_cast(bf16x8, o);
    }
    const bool odd = !(lane & 1);  // t even: t + kPackLead - 3 is odd, the window starts at element 1
    const unsigned sh = odd ? 16u : 0u;
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], sh);
    // bytes {flag.b1, flag.b0, d3 high or low half}
    o[3] = __builtin_amdgcn_perm(flag, d[3], odd ? 0x05040302u : 0x05040100u);
    return __builtin_bit_cast(bf16x8, o);
  }
  __device__ __forceinline__ bf16x8 conv1_operand(const float (&ld)[K1], int t) const {
    float v[K1];
#pragma unroll
    for (int j = 0; j < K1; ++j) v[j] = ld[j];
    if (h == 0 && t < 3) {  // v[j] = x[j] so far; wanted x[t + j - 3], 0 before the row: shift up by 3 - t
      const int s = 3 - t;
#pragma unroll
      for (int j = K1 - 1; j >= 0; --j) v[j] = (s & 1) ? (j >= 1 ? v[j - 1] : 0.f) : v[j];
#pragma unroll
      for (int j = K1 - 1; j >= 0; --j) v[j] = (s & 2) ? (j >= 2 ? v[j - 2] : 0.f) : v[j];
    }
    bf16x8 Bx;
#pragma unroll
    for (int j = 0; j < K1; ++j) Bx[j] = ecg::to_bf16(v[j]);
    Bx[7] = ecg::to_bf16(h == 0 && t < L ? 1.f : 0.f);
    return Bx;
  }

  // One flat parameter -> its fp32 LDS copy and, for conv2 weights w2[co][ci][k], the MFMA B fragments in
  // lane order (read back with one ds_read_b128 per fragment).  bf16: fwd B[r][co], r = 16k + ci; dgrad
  // B[r][ci], r = 16k + co; element (r, col) lives at frag[s = r>>5][lane = 16*((r&31)>>3) + col][j = r&7].
  // fp32 (16x16x4): element (r, col) at frag[s = r>>2][lane = 16*(r&3) + col].
  __device__ __forceinline__ void put_param(int i, float v) {
    ps[i] = v;
    if constexpr (!F32) {
      if (i >= lay.b2 && i < lay.b2 + C) fragF[frag_bias_elem(i - lay.b2)] = ecg::to_bf16(v);
    }
    const int e = i - lay.w2;
    if (e >= 0 && e < C * C * K2) {
      const int co = e / (C * K2), ci = (e / K2) % C, k = e % K2;
      const int rf = 16 * k + ci, rd = 16 * k + co;
      if constexpr (F32) {
        fragF32[(rf >> 2) * 64 + 16 * (rf & 3) + co] = v;
        fragD32[(rd >> 2) * 64 + 16 * (rd & 3) + ci] = v;
      } else {
        const __bf16 bv = ecg::to_bf16(v);
        fragF[((rf >> 5) * 64 + 16 * ((rf & 31) >> 3) + co) * 8 + (rf & 7)] = bv;
        fragD[((rd >> 5) * 64 + 16 * ((rd & 31) >> 3) + ci) * 8 + (rd & 7)] = bv;
      }
    }
  }

  // bf16: r in [80, 96) (the 6th, padding tap) of both fragment sets and the im2col row Lp are zero; h1 halo
  // rows 0,1 (t=-2,-1) and [Lp+2, Lp+8), mask halo rows [0,4) and [Lp+4, Lp+8) are zero.  No phase writes
  // them, so once per launch.
  __device__ __forceinline__ void zero_pads() {
    if constexpr (!F32) {
      for (int e = PF ? 2 * 32 * 8 : tid; e < 2 * 32 * 8; e += NT) {  // (PF: the image holds its own pads)
        const int which = e >> 8, l = 32 + ((e >> 3) & 31), j = e & 7;
        if (!frag_pad_is_bias(which, l, j)) (which ? fragD : fragF)[(2 * 64 + l) * 8 + j] = ecg::to_bf16(0.f);
      }
      if (tid < 4) reinterpret_cast<uint32_t*>(xcol + Lp * 8)[tid] = 0u;  // im2col zero row
    }
    constexpr int DW = C * (int)sizeof(AT) / 4;  // dwords per activation row
    uint32_t* h1w = reinterpret_cast<uint32_t*>(h1s);
    uint32_t* mw = reinterpret_cast<uint32_t*>(ms);
    for (int i = tid; i < 8 * DW; i += NT) {  // 8 rows
      const int r = i / DW, d = i % DW;
      const int hr = r < 2 ? r : Lp + 2 + (r - 2);
      h1w[hr * DW + d] = 0u;
      const int dr = r < 4 ? r : Lp + 4 + (r - 4);
      mw[dr * DW + d] = 0u;
    }
  }

  // ---- phase 1: conv1 + bias + ReLU into h1s (bf16: MFMA, conv1_mfma; fp32: VALU, conv1)
  // bf16.  A = W1ext[co][kk] (pf_aw): quarter 0 holds kk 0..7 (taps, then the bias), quarters 1..3 the zero K
  // padding.  B = xcol[t][kk], K = 32: quarter 0 holds {bf16(x[t-3 .. t+3]), "t < L"} built in registers from its
  // own loads (conv1_load / conv1_operand), quarters 1..3 hold zeros.  Quarter 0 also stores its operand as the
  // im2col row t (one 16-byte LDS store) for phase 4's conv1 wgrad; nothing reads xcol before the phase-1 barrier.
  __device__ __forceinline__ void conv1_pair(int pi, const X1& x) {
    const bool has2 = w + (pi + 1) * WAVES < Lp / 16;
    bf16x8 Bx[2];
    int t[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      t[u] = conv1_t(pi, u);
      if constexpr (PK)
        Bx[u] = conv1_operand_packed(x.p[u], t[u]);
      else
        Bx[u] = conv1_operand(x.v[u], t[u]);
      // (a clamped duplicate tile rewrites the same values)
      if (h == 0) *reinterpret_cast<bf16x8*>(xcol + t[u] * 8) = Bx[u];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !has2) break;
      const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf_aw, Bx[u], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      // acc[i] = conv1(x)[t][co = 4h + i] + bias (exactly 0 for t >= L)
      bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (AT)fmaxf(acc[i], 0.f);
      *reinterpret_cast<bf16x4*>(h1s + (t[u] + 2) * C + 4 * h) = o;
    }
  }
  // ``x0``: the wave's first pair, whose loads phase 0 issued.  Further pairs (8 waves or windows past 512 steps)
  // load their own.
  __device__ __forceinline__ void conv1_mfma(__amdgpu_buffer_rsrc_t xr, const X1& x0) {
    const int ntiles = Lp / 16;
    if (w < ntiles) conv1_pair(0, x0);  // wave-uniform
#pragma unroll 1
    for (int pi = 2; pi < 2 * MAX_PAIRS_PER_WAVE; pi += 2) {
      if (w + pi * WAVES >= ntiles) break;  // wave-uniform
      X1 x;
      conv1_load(xr, pi, x);
      conv1_pair(pi, x);
    }
  }

  __device__ __forceinline__ void conv1() {
    static_assert(F32, "bf16 kernels run conv1_mfma");
    mask1 = 0u;
    float w1r[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) w1r[k] = ps[lay.w1 + c * K1 + k];
    const float b1r = ps[lay.b1 + c];
#pragma unroll
    for (int pi = 0; pi < MAX_PAIRS_PER_WAVE; ++pi) {
      const int pair = w + pi * WAVES;
      if (pair < NP) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int t0 = 32 * pair + 16 * half + 4 * h;
          float xw[12];
#pragma unroll
          for (int q4 = 0; q4 < 3; ++q4) {
            const float4 v = reinterpret_cast<const float4*>(xs + t0)[q4];
            xw[4 * q4] = v.x; xw[4 * q4 + 1] = v.y; xw[4 * q4 + 2] = v.z; xw[4 * q4 + 3] = v.w;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int t = t0 + i;
            float v = b1r;
#pragma unroll
            for (int k = 0; k < K1; ++k) v = fmaf(w1r[k], xw[i + k], v);
            v = (t < L) ? fmaxf(v, 0.f) : 0.f;
            const AT vb = (AT)v;
            h1s[(t + 2) * C + c] = vb;
            mask1 |= ((float)vb > 0.f ? 1u : 0u) << (pi * 8 + half * 4 + i);
          }
        }
      }
    }
  }

  // ---- phase 2: conv2 (MFMA) + bias + ReLU -> pool partials, mask m -> LDS
  __device__ __forceinline__ void conv2() {
    if constexpr (!F32) {
      // out^T[co][t]: A = W2[co][(k,ci)] (the fragments are lane-order symmetric: the same registers serve as
      // B[(k,ci)][co] or A[co][(k,ci)]), B = h1col[(k,ci)][t] read straight from the [t][ci] rows.  The K padding
      // (tap 5) carries the bias: B rows r = 80..95 are the constant {1, 0, ...} (quarter 2) / 0 (quarter 3).
      bf16x8 Wf[3];
      float pool[4];
      if constexpr (PF) {
#pragma unroll
        for (int s = 0; s < 3; ++s) Wf[s] = pf_wf[s];
      } else {
#pragma unroll
        for (int s = 0; s < 3; ++s) Wf[s] = *reinterpret_cast<const bf16x8*>(fragF + (s * 64 + lane) * 8);
      }
      bf16x8 Bone;
#pragma unroll
      for (int j = 0; j < 8; ++j) Bone[j] = ecg::to_bf16(0.f);
      if (h == 2) Bone[0] = ecg::to_bf16(1.f);
#pragma unroll
      for (int i = 0; i < 4; ++i) pool[i] = 0.f;
#pragma unroll
      for (int pi = 0; pi < MAX_PAIRS_PER_WAVE; ++pi) {
        const int pair = w + pi * WAVES;
        if (pair < NP) {
          // all six B fragments of the pair first (one LDS round trip), then two independent MFMA chains
          bf16x8 Bh[2][3];
#pragma unroll
          for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int s = 0; s < 3; ++s) {
              const int r = 32 * pair + 16 * half + (lane & 15) + 2 * s + (h >> 1) - 2;  // h1 time index
              if (s == 2 && h >= 2)
                Bh[half][s] = Bone;  // tap 5: the bias row
              else
                Bh[half][s] = *reinterpret_cast<const bf16x8*>(h1s + (r + 2) * C + 8 * (h & 1));
            }
          f32x4 accs[2];
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            accs[half] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 3; ++s)
              accs[half] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Wf[s], Bh[half][s], accs[half], 0, 0, 0);
          }
          // acc[i] = conv2(h1)[t = t0 + (lane&15)][co = 4h + i] + b2[co]; the window mask t < L only matters in
          // the pair that straddles L (wave-uniform branch: every other pair runs the mask-free epilogue)
          auto epilogue = [&](auto masked) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
              const int t = 32 * pair + 16 * half + (lane & 15);
              const bool tv = !decltype(masked)::value || t < L;
              bf16x4 mk;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float a = tv ? accs[half][i] : 0.f;  // t >= L: h2 = 0, relu'(h2) = 0
                pool[i] += fmaxf(a, 0.f);
                // relu'(h2) = (acc > 0) as clamp(acc * 2^126, 0, 1): ONE v_mul_f32 with the clamp modifier instead of
                // a compare + select.  Exactly 1 for every acc >= 2^-126; a bf16 x bf16 MFMA sum plus a bf16 bias is
                // a multiple of products of bf16 ulps, so a non-zero acc below 2^-126 needs |weights x inputs|
                // below ~2^-63 (not reachable by a trained or initialised TinyECG).  Divergences from the reference's
                // (h2 > 0), by construction: a subnormal positive acc gives a fractional mask (its h2 contribution is
                // itself subnormal), and a NaN acc gives whatever v_med3 returns for NaN under this file's
                // -fno-honor-nans build (the reference's mask is 0 there) - with a NaN pre-activation the pooled
                // features, the loss and every gradient of the sample are NaN in both implementations anyway.
                mk[i] = ecg::to_bf16(__builtin_amdgcn_fmed3f(a * 0x1p126f, 0.f, 1.f));
              }
              *reinterpret_cast<bf16x4*>(ms + (t + 4) * C + 4 * h) = mk;
            }
          };
          if (32 * pair + 32 <= L)
            epilogue(std::false_type{});
          else
            epilogue(std::true_type{});
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) pool[i] = row16_sum(pool[i]);
      // (the relu'(h2) counts behind db2 come from the M phase's MFMAs: head_and_M)
      if ((lane & 15) == 15) {
#pragma unroll
        for (int i = 0; i < 4; ++i) red[RED_POOL + w * 16 + 4 * h + i] = pool[i];
      }
      return;
    }
    // fp32 from here on (the bf16 path returned above)
    float Wf[F32_KSTEPS];
#pragma unroll
    for (int s = 0; s < F32_KSTEPS; ++s) Wf[s] = fragF32[s * 64 + lane];
    const float b2r = ps[lay.b2 + c];
    float pool = 0.f, cnt = 0.f;
#pragma unroll
    for (int pi = 0; pi < MAX_PAIRS_PER_WAVE; ++pi) {
      const int pair = w + pi * WAVES;
      if (pair < NP) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int t0 = 32 * pair + 16 * half;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          // 16x16x4 f32: lane holds A[t0 + (l&15)][r = 4s + h], r = 16*tap + ci
#pragma unroll
          for (int s = 0; s < F32_KSTEPS; ++s) {
            const int r = 4 * s + h, tap = r >> 4, ci = r & 15;
            const float a = h1s[(t0 + (lane & 15) + tap - 2 + 2) * C + ci];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Wf[s], acc, 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int t = t0 + 4 * h + i;
            float v = fmaxf(acc[i] + b2r, 0.f);
            if (t >= L) v = 0.f;
            pool += v;
            const bool on = v > 0.f;
            cnt += on ? 1.f : 0.f;
            ms[(t + 4) * C + c] = (AT)(on ? 1.f : 0.f);
          }
        }
      }
    }
    pool = ecg::quarter_sum(pool);
    cnt = ecg::quarter_sum(cnt);
    if (lane < 16) {
      red[RED_POOL + w * 16 + lane] = pool;
      red[red_cnt(WAVES) + w * 16 + lane] = cnt;
    }
  }

  // ---- phase 3: wave 0 = head (TRAIN: softmax-CE + head grads; else logits -> out[b]);
  //               waves 1.. = M (mask-weighted conv2 wgrad, MFMA), training only
  template <bool TRAIN>
  __device__ __forceinline__ void head_and_M(int ylab, float inv_B, float* out, int out_stride, int b) {
    if (w == 0) {
      // Wave 0 runs the head with cross-lane traffic through v_readlane (SGPR broadcasts), not LDS shuffles.
      // pooled[c] (every quarter computes all 16 channels; only the broadcasts of lanes 0..15 are used)
      float pp[WAVES];
#pragma unroll
      for (int ww = 0; ww < WAVES; ++ww) pp[ww] = red[RED_POOL + ww * 16 + c];
      float pooled = 0.f;
#pragma unroll
      for (int ww = 0; ww < WAVES; ++ww) pooled += pp[ww];
      pooled *= 1.0f / (float)L;
      float pv[C];
#pragma unroll
      for (int co = 0; co < C; ++co) pv[co] = lane_bcast(pooled, co);
      // logit n = c (< nc) on every quarter
      const int n = c;
      float logit = -INFINITY;
      if (n < nc) {
        const float4* whr = reinterpret_cast<const float4*>(ps + lay.wh + n * C);
        logit = ps[lay.bh + n];
#pragma unroll
        for (int q4 = 0; q4 < C / 4; ++q4) {
          const float4 wv4 = whr[q4];
          logit = fmaf(wv4.x, pv[4 * q4], logit);
          logit = fmaf(wv4.y, pv[4 * q4 + 1], logit);
          logit = fmaf(wv4.z, pv[4 * q4 + 2], logit);
          logit = fmaf(wv4.w, pv[4 * q4 + 3], logit);
        }
      }
      if constexpr (!TRAIN) {
        if (lane < nc) out[(long)b * out_stride + n] = logit;
      } else {
        // softmax-CE over the nc logits of lanes 0..nc-1 (wave-uniform scalar loop)
        float m = -INFINITY;
        for (int nn = 0; nn < nc; ++nn) m = fmaxf(m, lane_bcast(logit, nn));
        const float e = (n < nc) ? __expf(logit - m) : 0.f;
        float ssum = 0.f;
        for (int nn = 0; nn < nc; ++nn) ssum += lane_bcast(e, nn);
        const int y = __builtin_amdgcn_readfirstlane(ylab);
        const float loss = m + __logf(ssum) - lane_bcast(logit, y);
        const float dlogit = (n < nc) ? (e / ssum - (n == y ? 1.f : 0.f)) * inv_B : 0.f;
        float* hg = red + red_head(WAVES);  // [wh, P] of this sample's row, stored with the rest in phase 5
        if (lane < nc) {
          float4* hr = reinterpret_cast<float4*>(hg + n * C);
#pragma unroll
          for (int q4 = 0; q4 < C / 4; ++q4)
            hr[q4] = make_float4(dlogit * pv[4 * q4], dlogit * pv[4 * q4 + 1], dlogit * pv[4 * q4 + 2],
                                 dlogit * pv[4 * q4 + 3]);
          hg[nc * C + n] = dlogit;
        }
        if (lane == 0) hg[nc * C + nc] = loss;
        // dpooled[co] = sum_n dlogit[n] * Wh[n][co]; lane co (< 16)
        float dp = 0.f;
        for (int nn = 0; nn < nc; ++nn) dp = fmaf(lane_bcast(dlogit, nn), ps[lay.wh + nn * C + c], dp);
        const float gl = dp * (1.0f / (float)L);
        if (lane < 16) red[RED_G + c] = gl;
        if constexpr (PF) {
          // The g-scaled conv2 dgrad fragments (phase 4's A operand; the same in every wave), built here by the head
          // wave as soon as g exists - it finishes ~270 cycles before the last M wave - into the LDS fragD slots, so
          // phase 4 needs no barrier of its own.  B[r][ci] = g[co] * w2[co][ci][k], co = 8(h&1) + j: the same
          // products and rounding as the per-wave scaling of the LDS-built kernel (bitwise equal operands).
          float gq[8];
          if constexpr (LEAN) {
            // Every 16-lane row of this wave holds g[0 .. 15] in lane order (each quarter computes all 16 channels
            // from the same broadcasts), so gq[j] = g[8(h&1) + j] is a move inside the row: odd quarters rotate
            // their row by 8 lanes, then lane j of each row is broadcast over the row - 10 DPP moves and selects
            // instead of 16 v_readlane, 16 moves out of the SGPRs and 8 selects.
            const int gi = __builtin_bit_cast(int, gl);
            const int gr = (h & 1) ? __builtin_amdgcn_update_dpp(0, gi, 0x128, 0xf, 0xf, false) : gi;  // row_ror:8
#define ECG_ROW_BCAST(j) gq[j] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, gr, 0x150 + (j), 0xf, 0xf, false));
            ECG_ROW_BCAST(0) ECG_ROW_BCAST(1) ECG_ROW_BCAST(2) ECG_ROW_BCAST(3)
            ECG_ROW_BCAST(4) ECG_ROW_BCAST(5) ECG_ROW_BCAST(6) ECG_ROW_BCAST(7)  // row_newbcast:j
#undef ECG_ROW_BCAST
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float lo = lane_bcast(gl, j), hi = lane_bcast(gl, 8 + j);
              gq[j] = (h & 1) ? hi : lo;
            }
          }
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            bf16x8 sc;
#pragma unroll
            for (int j = 0; j < 8; ++j) sc[j] = ecg::to_bf16(ecg::from_bf16(pf_wd[s][j]) * gq[j]);
            *reinterpret_cast<bf16x8*>(fragD + (s * 64 + lane) * 8) = sc;
          }
        }
      }
    } else if (TRAIN && w <= 5 * msplit(WAVES)) {
      // work item (tap k, pair range part): M_k[co][ci] = sum_t m[t][co] * h1[t+k-2][ci]
      constexpr int S = msplit(WAVES);
      const int item = w - 1, k = item / S, part = item % S;
      const int per = (NP + S - 1) / S;
      const int p0 = part * per, p1 = p0 + per < NP ? p0 + per : NP;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if constexpr (F32) {
        // 16x16x4 f32: lane holds A[co = l&15][t = 4s + h] and B[t][ci = l&15]
        for (int pair = p0; pair < p1; ++pair) {
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const int t = 32 * pair + 4 * s + h;
            const float a = ms[(t + 4) * C + (lane & 15)];
            const float bb = h1s[(t + k - 2 + 2) * C + (lane & 15)];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc, 0, 0, 0);
          }
        }
      } else {
        const int q = (lane & 15) >> 2, p4 = (lane & 3) * 4;
        // The centre-tap waves (k == 2) also count relu'(h2) per channel for db2: the same A (mask) fragment times
        // an all-ones B gives sum_t m[t][co] in every column (exact small integers in fp32) - one MFMA per pair
        // instead of a compare, an add and a 16-lane DPP reduction per value in every wave's conv2 epilogue.
        bf16x8 ones;
#pragma unroll
        for (int j = 0; j < 8; ++j) ones[j] = ecg::to_bf16(1.f);
        f32x4 cnt1 = {0.f, 0.f, 0.f, 0.f}, cnt2 = {0.f, 0.f, 0.f, 0.f};
        auto mfma_pair = [&](int pair, f32x4 a, f32x4& cn) {
          // Reduction slot (h, j) holds time 32*pair + 4h + j (j < 4) or 32*pair + 16 + 4h + (j - 4): the two
          // lane quarters of one 32-lane LDS cycle read 8 consecutive 32-B rows (256 B, conflict-free); with
          // 8h + j their rows were 256 B apart (2-way conflicts on every transposing read of this phase).
          const int ta = 32 * pair + 4 * h + q;
          // A[co][t]: transposing reads of the [t][co] mask image
          const bf16x8 A = cat44(lds_tr16(ms + (ta + 4) * C + p4), lds_tr16(ms + (ta + 16 + 4) * C + p4));
          // B[t][ci] = h1[t + k - 2][ci]
          const bf16x8 Bm =
              cat44(lds_tr16(h1s + (ta + k - 2 + 2) * C + p4), lds_tr16(h1s + (ta + 16 + k - 2 + 2) * C + p4));
          if (k == 2) cn = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, ones, cn, 0, 0, 0);  // wave-uniform
          return __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, Bm, a, 0, 0, 0);
        };
        // two independent accumulation chains so the next pair's transposing reads overlap this pair's MFMA
        f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
        int pair = p0;
        for (; pair + 1 < p1; pair += 2) {
          acc = mfma_pair(pair, acc, cnt1);
          acc2 = mfma_pair(pair + 1, acc2, cnt2);
        }
        if (pair < p1) acc = mfma_pair(pair, acc, cnt1);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += acc2[i];
        if (k == 2 && (lane & 15) == 0) {  // cnt[co = 4h + i] of this part's pairs (every column holds it)
#pragma unroll
          for (int i = 0; i < 4; ++i) red[red_cnt(WAVES) + part * 16 + 4 * h + i] = cnt1[i] + cnt2[i];
        }
      }
      // acc[i] = M_k[co = 4h+i][ci = c]
      float* pm = red + red_m(WAVES) + part * 1280;
#pragma unroll
      for (int i = 0; i < 4; ++i) pm[(4 * h + i) * (C * K2) + c * K2 + k] = acc[i];
    }
  }

  // ---- phase 4: conv2 dgrad (MFMA, A = mask, B = g-scaled w2) * relu'(h1), conv1 wgrad
  __device__ __forceinline__ void dgrad() {
    if constexpr (!F32) {
      // B[r][ci] = g[co] * w2[co][ci][k], r = 32s + 8h + j -> k = r>>4, co = r&15 = 8(h&1) + j
      float gq[8];
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2) {
        const float4 v = reinterpret_cast<const float4*>(red + RED_G + 8 * (h & 1))[q2];
        gq[4 * q2] = v.x; gq[4 * q2 + 1] = v.y; gq[4 * q2 + 2] = v.z; gq[4 * q2 + 3] = v.w;
      }
      bf16x8 Bd[3];
      // (g W2) fragments, used as A[ci][(k,co)]
      if constexpr (PF) {
        // The scaled fragments are the same in every wave: the head wave built them into the LDS fragD slots in
        // phase 3 (unused by the prepared-fragment kernels otherwise: their operands come from the global image),
        // published by the phase-3 barrier; every wave reads its three back (16 waves x 48 scaling VALU become one
        // wave's 48; the round-5 form, waves 0..2 scaling one set each behind an extra barrier, cost that barrier).
        // Same products, same rounding: bitwise the same operands.
#pragma unroll
        for (int s = 0; s < 3; ++s) Bd[s] = *reinterpret_cast<const bf16x8*>(fragD + (s * 64 + lane) * 8);
      } else {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const bf16x8 raw = *reinterpret_cast<const bf16x8*>(fragD + (s * 64 + lane) * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) Bd[s][j] = ecg::to_bf16(ecg::from_bf16(raw[j]) * gq[j]);
        }
      }
      const int q = (lane & 15) >> 2, p4 = (lane & 3) * 4;
      const __bf16* xzero = xcol + Lp * 8;
      f32x4 wacc = {0.f, 0.f, 0.f, 0.f};  // dW1ext[ci = 4h + i][kk = lane & 15] over this wave's pairs
#pragma unroll
      for (int pi = 0; pi < MAX_PAIRS_PER_WAVE; ++pi) {
        const int pair = w + pi * WAVES;
        if (pair < NP) {
          // both halves' mask fragments and h1 values first (one LDS round trip), then the two MFMA chains
          bf16x8 Am[2][3];
          bf16x4 hv[2];
          // mask time index r = t0 + (lane&15) - (2s + (h>>1)) + 2: one lane base (s = 2, half 0) and the six
          // fragments at non-negative constant row offsets 16*half + 4 - 2s, so every read is base + immediate
          const __bf16* mbase = ms + (32 * pair + (lane & 15) - (h >> 1) + 2) * C + 8 * (h & 1);
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int t0 = 32 * pair + 16 * half;
#pragma unroll
            for (int s = 0; s < 3; ++s)
              Am[half][s] = *reinterpret_cast<const bf16x8*>(mbase + (16 * half + 4 - 2 * s) * C);
            hv[half] = *reinterpret_cast<const bf16x4*>(h1s + (t0 + (lane & 15) + 2) * C + 4 * h);
          }
          f32x4 accs[2];
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            accs[half] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 3; ++s)
              accs[half] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Bd[s], Am[half][s], accs[half], 0, 0, 0);
          }
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            // acc[i] = dh1[t = t0 + (lane&15)][ci = 4h + i]; times relu'(h1), written over h1 (this wave's rows)
            const int t0 = 32 * pair + 16 * half;
            // dv = bf16(acc) where h1 > 0, else +0: h1 >= 0 (a ReLU output, possibly -0), so "h1 > 0" is "the 15
            // magnitude bits are non-zero"; (bits & 0x7fff) + 0x7fff carries into bit 15 exactly then, and an
            // arithmetic 16-bit shift by 15 widens that bit to the whole half - two packed halves per dword
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 hb = __builtin_bit_cast(u32x2, hv[half]);
            u32x2 db;
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2) {
              const unsigned nz = (hb[q2] & 0x7fff7fffu) + 0x7fff7fffu;
              typedef short s16x2 __attribute__((ext_vector_type(2)));
              const s16x2 m = __builtin_bit_cast(s16x2, nz) >> (short)15;
              bf16x2 pr;
              pr[0] = ecg::to_bf16(accs[half][2 * q2]);
              pr[1] = ecg::to_bf16(accs[half][2 * q2 + 1]);
              db[q2] = __builtin_bit_cast(unsigned, pr) & __builtin_bit_cast(unsigned, m);
            }
            *reinterpret_cast<u32x2*>(h1s + (t0 + (lane & 15) + 2) * C + 4 * h) = db;
          }
          // conv1 wgrad over the pair's 32 steps: A[ci][t] = dh1 (transposing reads of the rows just written by
          // this wave), B[t][kk] = xcol (columns 8..15 come from the zero row); reduction slots as in phase 3
          const int ta = 32 * pair + 4 * h + q;
          const bf16x8 Ad = cat44(lds_tr16(h1s + (ta + 2) * C + p4), lds_tr16(h1s + (ta + 16 + 2) * C + p4));
          const __bf16* xa = p4 < 8 ? xcol + ta * 8 + p4 : xzero;
          const __bf16* xb = p4 < 8 ? xcol + (ta + 16) * 8 + p4 : xzero;
          wacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ad, cat44(lds_tr16(xa), lds_tr16(xb)), wacc, 0, 0, 0);
        }
      }
      if ((lane & 15) < 8) {  // kk < 7: dW1[ci][kk]; kk = 7: db1[ci]
#pragma unroll
        for (int i = 0; i < 4; ++i) red[red_dw1(WAVES) + w * 128 + (4 * h + i) * 8 + (lane & 15)] = wacc[i];
      }
      return;
    }
    // fp32 from here on (the bf16 path returned above).  16x16x4 f32: B[r][ci], r = 4s + h = 16k + co
    float Wd[F32_KSTEPS];
#pragma unroll
    for (int s = 0; s < F32_KSTEPS; ++s) Wd[s] = fragD32[s * 64 + lane] * red[RED_G + ((4 * s + h) & 15)];
    float dw1[K1 + 1];
#pragma unroll
    for (int k = 0; k <= K1; ++k) dw1[k] = 0.f;
#pragma unroll
    for (int pi = 0; pi < MAX_PAIRS_PER_WAVE; ++pi) {
      const int pair = w + pi * WAVES;
      if (pair < NP) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int t0 = 32 * pair + 16 * half;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < F32_KSTEPS; ++s) {
            const int r = 4 * s + h, k = r >> 4, co = r & 15;
            const float a = ms[(t0 + (lane & 15) - k + 2 + 4) * C + co];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Wd[s], acc, 0, 0, 0);
          }
          const int tb = t0 + 4 * h;
          float xw[12];
#pragma unroll
          for (int q4 = 0; q4 < 3; ++q4) {
            const float4 v = reinterpret_cast<const float4*>(xs + tb)[q4];
            xw[4 * q4] = v.x; xw[4 * q4 + 1] = v.y; xw[4 * q4 + 2] = v.z; xw[4 * q4 + 3] = v.w;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool on = (mask1 >> (pi * 8 + half * 4 + i)) & 1u;
            const float d = on ? acc[i] : 0.f;
            dw1[K1] += d;
#pragma unroll
            for (int k = 0; k < K1; ++k) dw1[k] = fmaf(d, xw[i + k], dw1[k]);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k <= K1; ++k) {
      const float v = ecg::quarter_sum(dw1[k]);
      if (lane < 16) red[red_dw1(WAVES) + w * 128 + c * 8 + k] = v;
    }
  }

  // ---- phase 5: element i (0..P; P = loss) of this sample's gradient row, from the phase partials
  __device__ __forceinline__ float row_value(int i) const {
    float v = 0.f;
    if (i >= lay.wh) {
      v = red[red_head(WAVES) + (i - lay.wh)];
    } else if (i < lay.b1) {
      const int o = red_dw1(WAVES) + (i / K1) * 8 + (i % K1);
#pragma unroll
      for (int ww = 0; ww < WAVES; ++ww) v += red[o + ww * 128];
    } else if (i < lay.w2) {
      const int o = red_dw1(WAVES) + (i - lay.b1) * 8 + K1;
#pragma unroll
      for (int ww = 0; ww < WAVES; ++ww) v += red[o + ww * 128];
    } else if (i < lay.b2) {
      const int e = i - lay.w2;
#pragma unroll
      for (int part = 0; part < msplit(WAVES); ++part) v += red[red_m(WAVES) + part * 1280 + e];
      v *= red[RED_G + e / (C * K2)];
    } else {
      const int co = i - lay.b2;
      // relu'(h2) counts: bf16 path - one partial per M part (head_and_M), fp32 path - one per wave (conv2)
      constexpr int NCP = F32 ? WAVES : msplit(WAVES);
#pragma unroll
      for (int pp = 0; pp < NCP; ++pp) v += red[red_cnt(WAVES) + pp * 16 + co];
      v *= red[RED_G + co];
    }
    return v;
  }

  // Phase 5 with one job per thread and no loop: threads [0, 320) each write 4 consecutive conv2-weight
  // gradients (one 16-B LDS read per partial, one 16-B write-through store), threads [320, 448) the 128 conv1
  // weight/bias elements, threads [448, ...) conv2 bias, head and loss (row_value's sums, same order).
  __device__ __forceinline__ void row_store(__amdgpu_buffer_rsrc_t r, int rowbase) const {
    constexpr int NQ = C * C * K2 / 4;  // 320 quads of conv2 weights
    static_assert(NQ + 128 + C <= NT || WAVES < 16, "one job per thread at 16 waves");
    if constexpr (LEAN) {
      // The three thread ranges are whole waves (320 = 5 x 64, 448 = 7 x 64): scalar branches on the wave index, and
      // each range reads its own partials directly - row_value's sums in row_value's order, without its chain of
      // range tests and without the division by K1 (the conv1 range takes the partials' own [ci][8] order).
      static_assert(NQ % 64 == 0 && (NQ + 128) % 64 == 0, "thread ranges are whole waves");
      if (w >= NQ / 64) {
        if (w < (NQ + 128) / 64) {
          const int j = tid - NQ, ci = j >> 3, kk = j & 7;  // kk < 7: dW1[ci][kk]; kk = 7: db1[ci]
          float v = 0.f;
#pragma unroll
          for (int ww = 0; ww < WAVES; ++ww) v += red[red_dw1(WAVES) + ww * 128 + j];
          st_wt(r, rowbase + (kk < K1 ? lay.w1 + ci * K1 + kk : lay.b1 + ci), v);
        } else {
          const int co = tid - NQ - 128, i = lay.b2 + co;  // conv2 bias, then head and loss
          if (i <= lay.P) {
            float v;
            if (i >= lay.wh) {
              v = red[red_head(WAVES) + (i - lay.wh)];
            } else {
              v = 0.f;
#pragma unroll
              for (int pp = 0; pp < msplit(WAVES); ++pp) v += red[red_cnt(WAVES) + pp * 16 + co];
              v *= red[RED_G + co];
            }
            st_wt(r, rowbase + i, v);
          }
        }
        return;
      }
    }
    if (tid < NQ) {
      const int e0 = 4 * tid;
      f32x4 v = *reinterpret_cast<const f32x4*>(red + red_m(WAVES) + e0);
#pragma unroll
      for (int part = 1; part < msplit(WAVES); ++part) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(red + red_m(WAVES) + part * 1280 + e0);
        v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
      }
      const float g = red[RED_G + e0 / (C * K2)];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] *= g;
      st_wt4(r, rowbase + lay.w2 + e0, v);
    } else {
      const int i = tid < NQ + 128 ? tid - NQ : lay.b2 + (tid - NQ - 128);
      if (i <= lay.P) st_wt(r, rowbase + i, row_value(i));
    }
  }
};

// MODE 0: full training step (grads -> slab row).  MODE 1: forward only (logits -> out [B, nc]).
// MODE 2: diagnostic - every workgroup computes its training step twice; the second pass runs with warm
//         instruction / scalar / data caches (phase stamps of both passes: scripts/diag_step_phases.py).
// PK (MODE 0, PF): X holds packed bf16 window rows (kPackLead comment) instead of floats, row b at X + b * ldx
// (ldx = ldb / 2: the row pitch in 4-byte units, as for float rows).
//
// Argument order.  This file is built with kernarg preload (csrc/build.py): the hardware places the first 14 dwords of
// the kernel arguments in SGPRs when the wave starts (16 user SGPRs less the two of the kernarg pointer), and
// everything behind them is fetched by scalar loads whose wait the compiler puts in front of the first use.  So the
// arguments come in the order in which the kernel's first instructions need them - the stamps pointer (its null test
// is the first instruction), then what the addresses of phase 0's loads are made of: the window rows and their
// pitch, the image, the labels, L, nc and the head parameters - and fill the 14 dwords exactly: X 0-1, ldx 2-3,
// wprep 4-5, Y 6-7, stamps 8-9, L 10, nc 11, params 12-13.  The slab / logits pointer, its stride and 1/B are first
// read in phase 3 or later; ``idx`` is first in the kernels that gather for themselves, which run once per round
// (the PK kernel never reads it).  A pointer or long that straddles dword 14 would not be preloaded at all: keep the
// 8-byte arguments on even dwords when this list changes.  The code is also correct where the firmware does not
// preload: the compiler's prologue then loads the same dwords.
// MODE 4: MODE 0 of the PK kernel on the dataset packed once (tiny_pack_rows_kernel) instead of gathered rows: workgroup
//         b reads packed row idx[b] of X and label Y[idx[b]] itself.  The pitch of packed rows follows from L
//         (pack_ldb), so the ``ldx`` argument is free and carries the address of this step's ``idx`` row: it lies
//         inside the preloaded dwords, and the chain in front of the window loads is one scalar round trip (idx[b]),
//         not two (the idx pointer from the kernarg segment, then idx[b]).  A new instantiation: MODE 0's code is
//         untouched.
// MODE 3: MODE 0 for a cohort of M virtual clients of B windows each in one launch, grid (B, M).  Workgroup (x, c)
//         works on row c * B + x of the M * B rows (``idx``, the gathered rows and the slab hold the clients' rows back
//         to back) with client c's weights and image, which lie at the fixed strides cohort_pstride /
//         kCohortWprepStride from ``params`` / ``wprep``.  Both strides follow from ``nc``, so the argument list is
//         unchanged, and c is a workgroup id, not a division.  ``inv_B`` is 1 / B of one client.
constexpr int kCohortWprepStride = (WP_BYTES + 127) / 128 * 128;                          // bytes between images

template <int WAVES, int MODE, bool F32, bool PF, bool PK = false>
__global__ __launch_bounds__(WAVES * 64) void tiny_ecg_step_kernel(
    const float* __restrict__ X, long ldx,               // dataset windows [N, ldx]; MODE 4: ldx carries ``idx``
    const unsigned char* __restrict__ wprep,             // PF image of ``params`` (PF only)
    const int* __restrict__ Y,                           // [N] int32 labels (unused in MODE 1)
    unsigned long long* __restrict__ stamps,             // diagnostic phase clock (nullptr = off)
    int L, int nc,                                       // window length, classes
    const float* __restrict__ params,                    // flat fp32 params          -- preloaded up to here
    float* __restrict__ out, int out_stride,             // MODE0/2: slab [B][out_stride]; MODE1: logits
    float inv_B,
    const int* __restrict__ idx,                         // [B] rows of X for this step (nullptr: b; PK: unused)
    int slab_wt) {                                       // FusedOpt::slab_wt
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Sample = TinySample<WAVES, F32, PF, PK, MODE == 4>;  // LEAN: the MODE 4 kernels only
  Sample S(smem, L, nc);
  constexpr bool TRAIN = MODE != 1;
  constexpr bool COHORT = MODE == 3;
  constexpr bool PKI = MODE == 4;
  static_assert(!PKI || PK, "MODE 4 reads packed rows");
  const int tid = threadIdx.x;
  const int b = COHORT ? blockIdx.y * gridDim.x + blockIdx.x : blockIdx.x;
  const long rows = COHORT ? (long)gridDim.x * gridDim.y : (long)gridDim.x;
  if constexpr (COHORT) {
    params += (long)blockIdx.y * cohort_pstride(S.lay.P);
    if constexpr (PF) wprep += (long)blockIdx.y * kCohortWprepStride;
  }
  const __amdgpu_buffer_rsrc_t slab_r = make_rsrc(out, rows * out_stride * 4);
  const int rowbase = b * out_stride;
  if (stamps && tid == 0) stamps[(long)b * 16 + 15] = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
  for (int rep = 0; rep < (MODE == 2 ? 2 : 1); ++rep) {
#define ECG_STAMP(k) \
  if (stamps && tid == 0) stamps[(long)b * 16 + 7 * rep + (k)] = __builtin_amdgcn_s_memtime();
    ECG_STAMP(0)
    // phase 0: stage params (fp32: + x) into LDS, zero pads.  (Measured: pre-gathering a round's windows into
    // contiguous buffers inside the round graph, to drop the dependent idx -> row load, costs more than it saves:
    // 12.98 vs 12.52 us/step, profiles/r1_round_kernel/ab_pregather.log.)
    // The parameter loads are issued first, into registers, so their round trip overlaps the dependent
    // idx -> window chain.  bf16: the window never goes to LDS - each wave issues the loads of its first conv1
    // operand pair here (conv1_load) and phase 1 starts without a barrier: conv1 reads only its own registers, and
    // the pads and head parameters written here are first read after the phase-1 barrier.  Stamp 1 then marks
    // "inputs issued, pads written", not a barrier; the wait for the window is counted in phase 1.
    int ylab = 0;
    long row = b;  // PK: gathered rows, read in place (launch_step rejects an idx), so ``idx`` is never waited for
    long pitch = ldx;
    if constexpr (PKI) {
      // one scalar load, its address made of preloaded dwords only; the constant address space keeps it scalar
      typedef const __attribute__((address_space(4))) int* IdxPtr;
      row = ((IdxPtr)ldx)[b];
      pitch = pack_ldb(L) / 2;
    } else if constexpr (!PK) {
      row = idx ? (long)idx[b] : (long)b;
    }
    const float* xrow = X + row * pitch;
    // exactly the row (bf16); PK: the whole packed row, pads included
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t xr = make_rsrc(xrow, PK ? pitch * 4 : (long)L * 4);
    [[maybe_unused]] typename Sample::X1 x0;
    [[maybe_unused]] float hv_pk = 0.f;
    if constexpr (PK) {
      // Every address here is made of preloaded arguments and the workgroup / lane ids, so the loads go out in
      // latency order with no wait between them: the packed window row and the label, which the previous reduce
      // launch's gather blocks wrote through and which come from beyond the L2, then the image (L2-hot: every
      // workgroup of an XCD reads the same 6.4 KB), then this thread's head parameter.  (The label is a scalar load:
      // hipcc places it behind the pad stores below, still ahead of the first wait.)  The head parameter is the
      // last to arrive and nothing reads its LDS copy before phase 3: it is stored after conv1 (below), so that
      // conv1 waits for the window and the image only and the pad stores of phase 0 wait for nothing.
      S.conv1_load(xr, 0, x0);
      ylab = Y[row];
      S.pf_load_fwd(wprep);
      const int i = S.lay.wh + tid;
      hv_pk = i < S.lay.P ? params[i] : 0.f;
    } else if constexpr (PF) {
      // conv operands: global image -> VGPRs; only the head's parameters go to LDS (plain fp32 copy)
      S.pf_load_fwd(wprep);
      const int i = S.lay.wh + tid;
      const float hv = i < S.lay.P ? params[i] : 0.f;
      if (TRAIN) ylab = Y[row];
      S.conv1_load(xr, 0, x0);
      if (i < S.lay.P) S.ps[i] = hv;
      static_assert(MAX_CLASSES * C + MAX_CLASSES <= 8 * 64, "head parameters: one per thread");
    } else {
      constexpr int PR = 4;  // parameters per thread held in registers (P <= PR * NT for nc <= 40 at 8 waves)
      float pv[PR];
#pragma unroll
      for (int j = 0; j < PR; ++j) {
        const int i = tid + j * S.NT;
        pv[j] = i < S.lay.P ? params[i] : 0.f;
      }
      if constexpr (!F32) S.load_aw(params);
      if (TRAIN) ylab = Y[row];  // label prefetched with the window (used by the head)
      if constexpr (F32) {
        S.stage_x(xrow);
      } else {
        S.conv1_load(xr, 0, x0);
      }
#pragma unroll
      for (int j = 0; j < PR; ++j) {
        const int i = tid + j * S.NT;
        if (i < S.lay.P) S.put_param(i, pv[j]);
      }
      for (int i = tid + PR * S.NT; i < S.lay.P; i += S.NT) S.put_param(i, params[i]);
    }
    S.zero_pads();
    if constexpr (F32) {
      __syncthreads();
      ECG_STAMP(1)
      S.conv1();
    } else {
      ECG_STAMP(1)
      S.conv1_mfma(xr, x0);
      if constexpr (PK) {
        const int i = S.lay.wh + tid;
        if (i < S.lay.P) S.ps[i] = hv_pk;
      }
    }
    __syncthreads();
    ECG_STAMP(2)
    S.conv2();
    if constexpr (PF && TRAIN) S.pf_load_dgrad(wprep);  // lands under the barrier and the head phase
    __syncthreads();
    ECG_STAMP(3)
    S.template head_and_M<TRAIN>(ylab, inv_B, out, out_stride, b);
    if (!TRAIN) return;
    if ((MODE == 0 || PKI) && stamps && (tid & 63) == 0 && (S.w <= 1 || S.w == WAVES - 1))  // diagnostic: head / M wave ends
      stamps[(long)b * 16 + 8 + (S.w == 0 ? 0 : S.w == 1 ? 1 : 2)] = __builtin_amdgcn_s_memtime();
    __syncthreads();
    ECG_STAMP(4)
    S.dgrad();
    __syncthreads();
    ECG_STAMP(5)
    // phase 5: combine partials, scale by g, write this sample's gradient row (published by the kernel boundary).
    if (WAVES == 16 && slab_wt && S.lay.P - S.lay.b2 + 1 <= S.NT - 448) {
      S.row_store(slab_r, rowbase);
    } else if (slab_wt) {
      for (int i = tid; i <= S.lay.P; i += S.NT) st_wt(slab_r, rowbase + i, S.row_value(i));
    } else {
      for (int i = tid; i <= S.lay.P; i += S.NT) out[rowbase + i] = S.row_value(i);
    }
    ECG_STAMP(6)
#undef ECG_STAMP
    if (MODE == 2) __syncthreads();  // the second pass reuses the LDS
  }
  if (stamps && tid == 0) stamps[(long)b * 16 + 14] = __builtin_amdgcn_s_memrealtime();
}

// Sum the per-sample gradient rows and apply SGD (+momentum, weight decay, nesterov) in place.
// grid = ceil((P+1)/32) blocks of 512 threads: 32 columns x 16 row groups per block, each thread keeps 16
// independent row loads in flight.  The slab was just written by CUs on every XCD, so this is a
// latency/fabric-bound read of ~1.5 MB.  Measured (bench.py, us/step, two-launch graph round, TinyECG
// B=256): 4 cols 13.7, 8 cols 12.5, 16 cols 11.8, 32 cols 11.5, 64 cols 11.7 - 128-byte row segments per
// wave instruction over 46 CUs beat narrower segments over more CUs (profiles/r1_final/ab_red_cols.txt).
// Column P carries the per-sample loss (accumulated into loss_acc, never SGD-updated).
// RED_COLS (columns per block) only changes how columns are grouped into blocks, never a column's summation
// order (fixed by RED_ROWG and the chunking below), so every width gives bitwise-identical results.
// Argument order (kernarg preload, see tiny_ecg_step_kernel): the 14 preloaded dwords are what stands between the
// wave's start and its loads - slab 0-1, params 2-3, mom 4-5, then nred (the reduce / gather branch is the first
// instruction), G, stride, P, the apply / nesterov flags (one dword) and momentum (dwords 6-11) - and the two scalars
// of the update, lr and wd (12-13), so that the epilogue behind the barrier starts no scalar load of its own.  The
// image, loss and gradient-copy pointers are fetched under the slab loads; the gather blocks' GatherArgs, about 80
// bytes by value, comes last - nothing waits for those blocks.  The DP and cohort kernels keep this order.
constexpr int kRedColsDefault = 32;
constexpr int kRedApply = 1, kRedNesterov = 2;
inline int red_flags(int apply, int nesterov) { return (apply ? kRedApply : 0) | (nesterov ? kRedNesterov : 0); }
constexpr int RED_ROWG = 16;

// Next-step gather riding on the reduce launch: blocks >= nred copy the windows and labels of
// the NEXT step's batch (idx) into a contiguous buffer xg [B][ldg] / yg [B], so that step's kernel stages row b
// directly - its phase 0 loses the dependent idx -> window round trip.  The reduce blocks are latency-bound
// (46 blocks on 256 CUs), so the copy runs beside them on otherwise idle CUs instead of as a launch of its own
// (a separate pre-gather node was measured slower in round 1: profiles/r1_round_kernel/ab_pregather.log).
struct GatherArgs {
  const float* X;
  long ldx;
  const int* idx;  // [B] dataset rows of the next step
  const int* Y;
  float* xg;       // [B][ldg] written write-through
  int* yg;         // [B]
  int L, ldg, B, vec;  // vec: 16-byte rows (L % 4 == 0, ldx % 4 == 0, X 16-byte aligned)
  __bf16* xbg;         // [B][ldb] packed bf16 rows (kPackLead comment), written write-through; nullptr: none
  int ldb;
  const __bf16* xpk;   // [N][ldb] the whole dataset as packed rows (tiny_pack_rows_kernel); nullptr: none.  With it
                       // the blocks copy packed rows xpk[idx[b]] -> xbg[b] and the labels: X and xg are not touched
};
// Threads that share one row - one per element, per 4 floats (vec) or, for packed source rows, per 16 bytes - and
// the rows a block of ``nt`` threads takes.
__host__ __device__ inline int gather_per_row(const GatherArgs& ga) {
  return ga.xpk ? ga.ldb / 8 : ga.vec ? ga.L / 4 : ga.L;
}
__host__ __device__ inline int gather_rows_per_block(int per_row, int nt) {
  return per_row >= nt ? 1 : nt / per_row;
}

// A gather block (blockIdx.x >= nred) of NT threads: ``gather_rows_per_block`` rows of the next step's batch, one
// element (vec: 4 elements) per thread and pass.  With ``xbg`` each thread also stores the bf16 of what it loaded -
// the same cast as the step kernel's ecg::to_bf16 - and the row's threads share out its zero pads: the whole packed
// row is written every time, and X is read once.
// With ``xpk`` (the dataset packed once, tiny_pack_rows_kernel) a row is ldb / 8 threads that each move 16 bytes of
// the packed row xpk[idx[b]], pads included, to xbg[b]: no fp32 is read, nothing is converted and xg is not written.
template <int NT>
__device__ __forceinline__ void gather_block(const GatherArgs& ga, int nred) {
  const int per_row = gather_per_row(ga);
  const int rpb = gather_rows_per_block(per_row, NT);
  const int r0 = ((int)blockIdx.x - nred) * rpb;
  const __amdgpu_buffer_rsrc_t br = make_rsrc(ga.xbg, ga.xbg ? (long)ga.B * ga.ldb * 2 : 0);
  if (ga.xpk) {  // (launch-uniform)
    for (int e = threadIdx.x; e < rpb * per_row; e += NT) {
      const int lr_ = e / per_row, j = e - lr_ * per_row, b = r0 + lr_;
      if (b >= ga.B) break;
      const long row = ga.idx[b];
      const u32x4 v = *reinterpret_cast<const u32x4*>(ga.xpk + row * ga.ldb + 8 * j);
      st_wt_b128(br, (b * ga.ldb + 8 * j) * 2, v);
      if (j == 0) ga.yg[b] = ga.Y[row];
    }
    return;
  }
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(ga.xg, (long)ga.B * ga.ldg * 4);
  const int npad = ga.ldb - ga.L;  // pad elements of a packed row: kPackLead in front, the rest behind the data
  for (int e = threadIdx.x; e < rpb * per_row; e += NT) {
    const int lr_ = e / per_row, j = e - lr_ * per_row, b = r0 + lr_;
    if (b >= ga.B) break;  // e only grows, so every later e is past the batch too
    const long row = ga.idx[b];
    if (ga.vec) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(ga.X + row * ga.ldx + 4 * j);
      st_wt4(xr, b * ga.ldg + 4 * j, v);
      if (ga.xbg) {  // 8-byte units: 4 | L, kPackLead and ldb, so the pads are npad / 4 whole units
        bf16x4 p;
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = ecg::to_bf16(v[q]);
        st_wt_b64(br, (b * ga.ldb + kPackLead + 4 * j) * 2, __builtin_bit_cast(u32x2, p));
        for (int u = j; u < npad / 4; u += per_row)
          st_wt_b64(br, (b * ga.ldb + (u == 0 ? 0 : ga.L + 4 * u)) * 2, u32x2{0u, 0u});
      }
    } else {
      const float v = ga.X[row * ga.ldx + j];
      st_wt(xr, b * ga.ldg + j, v);
      if (ga.xbg) {
        st_wt_b16(br, (b * ga.ldb + kPackLead + j) * 2, __builtin_bit_cast(unsigned short, ecg::to_bf16(v)));
        for (int u = j; u < npad; u += per_row)
          st_wt_b16(br, (b * ga.ldb + (u < kPackLead ? u : ga.L + u)) * 2, (unsigned short)0);
      }
    }
    if (j == 0) ga.yg[b] = ga.Y[row];
  }
}
static_assert(kPackLead == 4, "gather_block's 4-float form writes the lead as one 8-byte unit");

// DP-SGD noise is counter-based so that a graph replay, an enqueued round and the torch backend (utils/philox.py) draw
// the same z: philox4x32_10 with counter (i, t lo, t hi, 0) and key (seed lo, seed hi), i the parameter index and t the
// 64-bit DP step counter; u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (w1 >> 8) * 2^-24 in [0, 1),
// z = sqrt(-2 ln u1) * cos(2 pi u2) with the accurate logf / sqrtf / cosf (|z| <= 5.77).
// ``stream`` is the counter's last word: 0 single-client DP-SGD, 1 client-level DP (tiny_ecg_close.hip), 2 + c the
// record-level DP-SGD of cohort slot c (c < 65535), so the M clients of one cohort step draw independent vectors.
__device__ inline float dp_normal(int i, unsigned long long seed, unsigned long long t, uint32_t stream = 0u) {
  uint32_t c[4] = {(uint32_t)i, (uint32_t)t, (uint32_t)(t >> 32), stream};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u1 = (float)((c[0] >> 8) + 1u) * 0x1p-24f, u2 = (float)(c[1] >> 8) * 0x1p-24f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// The one body of the reduce kernels.  DP: every loaded gradient value is multiplied by its row's clip factor
// ``scale[row]`` and ``noise_scale`` * z_col is added to the column sum before the epilogue (the loss column is neither
// scaled nor noised; noise_scale == 0: no noise is drawn).  COHORT: block c * nblk + j (nblk = the single-client block
// count) is block j on client c's G slab rows, weights, momentum, image and loss word; the update is always applied.
// Column-to-block map, row chunking, summation order and epilogue are these lines for every form, so DP with every
// scale[b] == 1 and no noise, a cohort of one, and PROX with mu == 0 give the plain kernel's bits.  The pointers carry no __restrict__
// here: the kernels' own parameters do, and a second set of alias scopes from the inlined body changes the gather
// branch's code (profiles/r12/tiny_reduce_merge.txt).
// PROX (FedProx, Li et al. 2020): the gradient that enters the epilogue gains mu * (p - anchor[col]), the gradient of
// mu/2 * |w - anchor|^2: d = gsum + wd * p + mu * (p - a), which then passes through momentum and nesterov like any
// other gradient (torch.optim.SGD with mu * (p - a) added to p.grad).  ``anchor`` [P] is shared by all clients of a cohort
// (never offset by the client stride); the updating thread loads it beside p0 / m0, before the slab reads.
// STEPS (COHORT only; clients with unequal local work): a block of client c returns at once when ``step`` >=
// client_steps[c] ([M] int32 on the device: a cohort is drawn per round, and kernel arguments are baked into a captured
// graph) - before any parameter, momentum, anchor or slab load and before the barrier; the condition is block-uniform.
// A client that has finished its local steps is thereby frozen: its weights, momentum, image and loss word are not
// written, while the step kernel still fills its slab rows and the gather blocks, which leave above, still run.
// DP && COHORT (record-level DP-SGD inside a cohort): ``scale`` holds M * G clip factors, client c's at scale + c * G
// (dp_row_scale_cohort_kernel), and client c draws its noise from Philox stream 2 + c of the one step word - after
// the STEPS return, so a frozen client draws nothing.
template <int RED_COLS, bool DP, bool COHORT, bool PROX = false, bool STEPS = false>
__device__ __forceinline__ void slab_reduce_body(
    const float* slab, float* params, float* mom, int nred, int G, int stride, int P, int flags, float momentum,
    float lr, float wd, unsigned char* wprep, float* loss_acc, float* grad_out, const float* scale, float noise_scale,
    unsigned long long seed, const unsigned long long* dp_step, const GatherArgs& ga, const float* anchor = nullptr,
    float mu = 0.f, const int* client_steps = nullptr, int step = 0) {
  static_assert(!STEPS || COHORT, "per-client step counts exist in the cohort form only");
  constexpr int NT = RED_COLS * RED_ROWG;
  const int apply = COHORT ? 1 : flags & kRedApply, nesterov = flags & kRedNesterov;
  if ((int)blockIdx.x >= nred) {  // block-uniform: gather blocks never reach the barrier below
    gather_block<NT>(ga, nred);
    return;
  }
  int blk = blockIdx.x, client = 0;
  if constexpr (COHORT) {
    const int nblk = (P + RED_COLS) / RED_COLS;  // blocks per client: columns 0 .. P
    client = blk / nblk;
    if constexpr (STEPS)
      if (step >= client_steps[client]) return;  // block-uniform, before the barrier: a frozen client
    const int pstride = cohort_pstride(P);
    slab += (long)client * G * stride;
    if constexpr (DP) scale += (long)client * G;
    params += (long)client * pstride;
    mom += (long)client * pstride;  // (only dereferenced when momentum != 0, which needs a momentum buffer)
    if (wprep) wprep += (long)client * kCohortWprepStride;
    blk -= client * nblk;
  }
  __shared__ float part[RED_ROWG][RED_COLS + 1];
  const int cl = threadIdx.x % RED_COLS, rg = threadIdx.x / RED_COLS;
  const int col = blk * RED_COLS + cl;
  // the updating threads fetch their parameter / momentum before the slab reads: one round trip, not two
  const bool upd = rg == 0 && col < P && apply;
  const float p0 = upd ? params[col] : 0.f;
  const float m0 = (upd && momentum != 0.f) ? mom[col] : 0.f;
  float a0 = 0.f;
  if constexpr (PROX) a0 = upd ? anchor[col] : 0.f;
  float noise = 0.f;  // drawn before the slab reads, under their latency
  if constexpr (DP && COHORT) {
    if (rg == 0 && col < P && noise_scale != 0.f)
      noise = noise_scale * dp_normal(col, seed, dp_step[0] - 1ull, 2u + (uint32_t)client);
  } else if constexpr (DP) {
    if (rg == 0 && col < P && noise_scale != 0.f) noise = noise_scale * dp_normal(col, seed, dp_step[0] - 1ull);
  }
  float s = 0.f;
  if (col <= P) {
    const float* base = slab + col;
    const bool grad_col = col < P;  // DP: the loss column is summed as it is
    auto load = [&](int rr) {
      const float v = base[(long)rr * stride];
      if constexpr (DP) return v * (grad_col ? scale[rr] : 1.f);
      else return v;
    };
    int r = rg;
    for (; r + RED_ROWG * 15 < G; r += RED_ROWG * 16) {
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = load(r + RED_ROWG * j);
#pragma unroll
      for (int j = 0; j < 16; j += 2) s += v[j] + v[j + 1];
    }
    for (; r < G; r += RED_ROWG) s += load(r);
  }
  part[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && col <= P) {
    float gsum = 0.f;
#pragma unroll
    for (int j = 0; j < RED_ROWG; ++j) gsum += part[j][cl];
    if (col == P) {
      if (loss_acc) loss_acc[client] += gsum;
    } else {
      if constexpr (DP)
        if (noise_scale != 0.f) gsum += noise;
      if (grad_out) grad_out[col] = gsum;
      if (apply) {
        const float p = p0;
        float d = gsum + wd * p;
        if constexpr (PROX) d += mu * (p - a0);
        if (momentum != 0.f) {
          const float bm = momentum * m0 + d;
          mom[col] = bm;
          d = nesterov ? d + momentum * bm : bm;
        }
        const float pn = p - lr * d;
        params[col] = pn;
        if (wprep) wprep_put(wprep, col, pn);
      }
    }
  }
}

template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom,
    int nred,   // blocks below this index reduce, the rest gather; INT_MAX = no gather
    int G, int stride, int P,
    int flags,  // kRedApply | kRedNesterov
    float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep,   // PF image kept current with the updated parameters (nullable)
    float* __restrict__ loss_acc, float* __restrict__ grad_out, GatherArgs ga) {
  slab_reduce_body<RED_COLS, false, false>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd, wprep,
                                           loss_acc, grad_out, nullptr, 0.f, 0ull, nullptr, ga);
}

// ---------------------------------------------------------------------------- DP-SGD (per-sample clip + noise)
// The slab already holds one gradient row per sample, so DP-SGD only changes the reduce side: a row-norm launch
// writes the clip factors c_b = min(1, C / n_b) and ``slab_reduce_dp_sgd_kernel`` sums c_b * row_b, adds
// sigma * C / B * z_i (dp_normal, above the body) and runs the same SGD / wprep / gather epilogue.  The step kernel is
// not involved.

// Diagnostic: z[i] for i < P of step t (the values the DP reduce adds, without the sigma * C / B factor).
template <int NT>
__global__ __launch_bounds__(NT) void dp_noise_kernel(float* __restrict__ z, int P, unsigned long long seed,
                                                      unsigned long long t) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < P) z[i] = dp_normal(i, seed, t);
}

// Clip factors of one step's slab: one wave per row, scale[b] = min(1, clip / n_b) with n_b = B * |row_b[0:P]|_2 (the
// step kernel stores rows pre-scaled by 1/B; the loss column P is not part of the norm; n_b == 0 -> 1).  Fixed
// summation order (per lane in column order, then a butterfly over the wave), no atomics.  vec: 16-byte loads
// (rows 16-byte aligned, stride % 4 == 0 so the last row's padding is readable).  Thread 0 of block 0 advances the DP
// step counter: it is the counter's only writer, and its only reader is the DP reduce launched next, which
// therefore draws step ``dp_step[0] - 1``.  Kernel arguments are baked into a captured graph; a device word is not.
constexpr int DP_ROWS_PER_BLOCK = 4;
template <int ROWS>
__global__ __launch_bounds__(ROWS * 64) void dp_row_scale_kernel(
    const float* __restrict__ slab, int G, int stride, int P, float clip, float* __restrict__ scale,
    unsigned long long* __restrict__ dp_step, int vec) {
  if (blockIdx.x == 0 && threadIdx.x == 0) dp_step[0] = dp_step[0] + 1ull;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS + (threadIdx.x >> 6);
  if (b >= G) return;  // wave-uniform
  const float* row = slab + (long)b * stride;
  float ss = 0.f;
  if (vec) {
    for (int c0 = 4 * lane; c0 < P; c0 += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) ss += (c0 + j < P) ? v[j] * v[j] : 0.f;
    }
  } else {
    for (int c0 = lane; c0 < P; c0 += 64) {
      const float v = row[c0];
      ss += v * v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) {
    const float n = (float)G * sqrtf(ss);
    scale[b] = n > 0.f ? fminf(1.f, clip / n) : 1.f;
  }
}

// The clip factors of one cohort step, all M clients in one launch: ``rows`` = M * B slab rows, scale[c * B + b] =
// min(1, clip / (B * |row|_2)) - the un-scaling is the client's batch size, not the row count.  One advance of the
// step word per launch, i.e. per cohort step, whichever clients are frozen.  dp_row_scale_kernel's lines with ``rows``
// as the bound and ``B`` as the factor; a kernel of its own because a shared body changed that kernel's code (two
// commuted adds), and its machine code is kept as it was.
template <int ROWS>
__global__ __launch_bounds__(ROWS * 64) void dp_row_scale_cohort_kernel(
    const float* __restrict__ slab, int rows, int B, int stride, int P, float clip, float* __restrict__ scale,
    unsigned long long* __restrict__ dp_step, int vec) {
  if (blockIdx.x == 0 && threadIdx.x == 0) dp_step[0] = dp_step[0] + 1ull;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS + (threadIdx.x >> 6);
  if (b >= rows) return;  // wave-uniform
  const float* row = slab + (long)b * stride;
  float ss = 0.f;
  if (vec) {
    for (int c0 = 4 * lane; c0 < P; c0 += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) ss += (c0 + j < P) ? v[j] * v[j] : 0.f;
    }
  } else {
    for (int c0 = lane; c0 < P; c0 += 64) {
      const float v = row[c0];
      ss += v * v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) {
    const float n = (float)B * sqrtf(ss);
    scale[b] = n > 0.f ? fminf(1.f, clip / n) : 1.f;
  }
}

// slab_reduce_body's DP form: ``scale`` [G] from dp_row_scale_kernel, noise_scale = sigma * C / B.  The plain
// kernel's argument order with the DP arguments in front of ``ga``.
template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_dp_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, float* __restrict__ grad_out,
    const float* __restrict__ scale, float noise_scale, unsigned long long seed,
    const unsigned long long* __restrict__ dp_step, GatherArgs ga) {
  slab_reduce_body<RED_COLS, true, false>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd, wprep,
                                          loss_acc, grad_out, scale, noise_scale, seed, dp_step, ga);
}

// ---------------------------------------------------------------------------- cohorts of virtual clients
// A cohort round trains M stateless virtual clients of B windows each side by side: one step launch of M * B
// workgroups and one reduce launch of M x the plain reduce's blocks per step, between a fan-out of the global weights
// and the mean of the clients' weights.  Client c's weights / momentum are at ``params`` / ``mom`` + c * pstride
// floats (cohort_pstride), its image at ``wprep`` + c * kCohortWprepStride bytes, its loss word at loss_acc[c] and its
// slab rows at [c * B, (c + 1) * B).  The step kernel is tiny_ecg_step_kernel's MODE 3.
// slab_reduce_body's COHORT form, M clients in one launch: blocks >= nred = M * nblk gather the next step's M * G rows
// (ga.B).  The plain kernel's argument order without ``grad_out``; the apply flag is not read.
template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_cohort_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, GatherArgs ga) {
  slab_reduce_body<RED_COLS, false, true>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd, wprep,
                                          loss_acc, nullptr, nullptr, 0.f, 0ull, nullptr, ga);
}

// ---------------------------------------------------------------------------- FedProx (proximal local steps)
// slab_reduce_body's PROX form in the plain and the cohort kernel, and the snapshot a single client's round starts
// with.  The step kernel is not involved: the proximal term only enters the SGD epilogue, as one more load per updating
// thread (under the slab reads) and a subtract and a multiply-add.
// The plain kernel's argument order with ``anchor``, ``mu`` in front of ``ga``.
template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_prox_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, float* __restrict__ grad_out,
    const float* __restrict__ anchor, float mu, GatherArgs ga) {
  slab_reduce_body<RED_COLS, false, false, true>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd, wprep,
                                                 loss_acc, grad_out, nullptr, 0.f, 0ull, nullptr, ga, anchor, mu);
}

// The cohort kernel's argument order with ``anchor`` [P] - one vector for all M clients - and ``mu`` in front of ``ga``.
template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_cohort_prox_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, const float* __restrict__ anchor, float mu,
    GatherArgs ga) {
  slab_reduce_body<RED_COLS, false, true, true>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd, wprep,
                                                loss_acc, nullptr, nullptr, 0.f, 0ull, nullptr, ga, anchor, mu);
}

// ---------------------------------------------------------------------------- per-client local steps
// slab_reduce_body's STEPS form of the two cohort kernels: their argument lists with ``client_steps`` [M], ``step`` in
// front of ``ga``.  With every client_steps[c] > step they leave the bits of the kernels above.
template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_cohort_steps_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, const int* __restrict__ client_steps, int step,
    GatherArgs ga) {
  slab_reduce_body<RED_COLS, false, true, false, true>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd,
                                                       wprep, loss_acc, nullptr, nullptr, 0.f, 0ull, nullptr, ga,
                                                       nullptr, 0.f, client_steps, step);
}

template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_cohort_steps_prox_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, const float* __restrict__ anchor, float mu,
    const int* __restrict__ client_steps, int step, GatherArgs ga) {
  slab_reduce_body<RED_COLS, false, true, true, true>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd,
                                                      wprep, loss_acc, nullptr, nullptr, 0.f, 0ull, nullptr, ga, anchor,
                                                      mu, client_steps, step);
}

// ---------------------------------------------------------------------------- record-level DP-SGD in a cohort
// slab_reduce_body's DP && COHORT forms: the cohort kernels' argument lists with ``scale`` [M * G], ``noise_scale`` =
// sigma * C / G, ``seed`` and ``dp_step`` in front of ``ga`` (and of ``client_steps``, ``step``).  With every factor 1
// and no noise they leave the bits of the cohort kernels above; a cohort of one without noise those of
// slab_reduce_dp_sgd_kernel.
template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_cohort_dp_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, const float* __restrict__ scale,
    float noise_scale, unsigned long long seed, const unsigned long long* __restrict__ dp_step, GatherArgs ga) {
  slab_reduce_body<RED_COLS, true, true>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd, wprep,
                                         loss_acc, nullptr, scale, noise_scale, seed, dp_step, ga);
}

template <int RED_COLS>
__global__ __launch_bounds__(RED_COLS * RED_ROWG) void slab_reduce_cohort_dp_steps_sgd_kernel(
    const float* __restrict__ slab, float* __restrict__ params, float* __restrict__ mom, int nred, int G, int stride,
    int P, int flags, float momentum, float lr, float wd,  // -- preloaded up to here
    unsigned char* __restrict__ wprep, float* __restrict__ loss_acc, const float* __restrict__ scale,
    float noise_scale, unsigned long long seed, const unsigned long long* __restrict__ dp_step,
    const int* __restrict__ client_steps, int step, GatherArgs ga) {
  slab_reduce_body<RED_COLS, true, true, false, true>(slab, params, mom, nred, G, stride, P, flags, momentum, lr, wd,
                                                      wprep, loss_acc, nullptr, scale, noise_scale, seed, dp_step, ga,
                                                      nullptr, 0.f, client_steps, step);
}

// Diagnostic: dp_noise_kernel with the stream word (2 + c: what client slot c of a cohort DP reduce draws).
template <int NT>
__global__ __launch_bounds__(NT) void dp_noise_stream_kernel(float* __restrict__ z, int P, unsigned long long seed,
                                                             unsigned long long t, uint32_t stream) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < P) z[i] = dp_normal(i, seed, t, stream);
}

// anchor[0:P] = params[0:P]: the first launch of a single client's FedProx round.
template <int NT>
__global__ __launch_bounds__(NT) void prox_snapshot_kernel(const float* __restrict__ params, float* __restrict__ anchor,
                                                           int P) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < P) anchor[i] = params[i];
}

// ---------------------------------------------------------------------------- the dataset packed once
// The whole dataset as packed rows, once: out[n] = [kPackLead zeros][bf16(X[n][0 .. L-1])][zeros up to ldb] for every
// row n < N - the layout and the cast (ecg::to_bf16) of gather_block's xbg rows, so a step that reads out[idx[b]]
// sees the bits it would have seen in the gathered row.  One block per row (rows beyond the grid: grid stride); every
// element of a row, pads included, is written on every call.  VEC (4 | L, 4 | ldx, X 16-byte aligned): a thread takes
// 4 packed elements - which lie wholly in the data or wholly in a pad, 4 dividing L, kPackLead and ldb - with one
// 16-byte load and one 8-byte store; otherwise one element per thread and pass.
template <bool VEC>
__global__ __launch_bounds__(128) void tiny_pack_rows_kernel(const float* __restrict__ X, long ldx, long N, int L,
                                                             __bf16* __restrict__ out) {
  const int ldb = pack_ldb(L);
  for (long n = blockIdx.x; n < N; n += gridDim.x) {
    const float* x = X + n * ldx;
    __bf16* o = out + n * ldb;
    if constexpr (VEC) {
      for (int u = threadIdx.x; u < ldb / 4; u += blockDim.x) {
        const int j = 4 * u - kPackLead;  // first source element of the unit
        bf16x4 p;
        if (j >= 0 && j < L) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(x + j);
#pragma unroll
          for (int q = 0; q < 4; ++q) p[q] = ecg::to_bf16(v[q]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) p[q] = ecg::to_bf16(0.f);
        }
        *reinterpret_cast<bf16x4*>(o + 4 * u) = p;
      }
    } else {
      for (int e = threadIdx.x; e < ldb; e += blockDim.x) {
        const int j = e - kPackLead;
        const bool in = j >= 0 && j < L;  // the pad is chosen as bits: this file is built without signed zeros
        const unsigned short v = __builtin_bit_cast(unsigned short, ecg::to_bf16(x[in ? j : 0]));
        reinterpret_cast<unsigned short*>(o)[e] = in ? v : (unsigned short)0;
      }
    }
  }
}

// ---------------------------------------------------------------------------- cohort fan-out and mean
// Start of a cohort round: every client's weights = the global weights, every momentum = 0 (virtual clients keep no
// state between rounds).  grid (ceil(P / NT), M); the pstride - P padding floats of a client are not written.
template <int NT>
__global__ __launch_bounds__(NT) void cohort_fanout_kernel(const float* __restrict__ global_params,
                                                           float* __restrict__ params, float* __restrict__ mom, int P) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= P) return;
  const long o = (long)blockIdx.y * cohort_pstride(P) + i;
  params[o] = global_params[i];
  if (mom) mom[o] = 0.f;
}

// End of a cohort round: global[i] = (((p_0[i] + p_1[i]) + ...) + p_{M-1}[i]) * inv_M in fp32, clients in ascending
// order (inv_M = 1.0f / M, rounded once on the host): one fixed order, so the mean is reproducible.  Every other close
// of a round is ecg::tiny::cohort_close (kernels/tiny_ecg_close.hip).
template <int NT>
__global__ __launch_bounds__(NT) void cohort_mean_kernel(const float* __restrict__ params,
                                                         float* __restrict__ global_params, int P, int M, float inv_M) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= P) return;
  const int pstride = cohort_pstride(P);
  float s = params[i];
  for (int c = 1; c < M; ++c) s += params[(long)c * pstride + i];
  global_params[i] = s * inv_M;
}

// ---------------------------------------------------------------------------- host launchers
unsigned long long* g_stamps = nullptr;  // diagnostic phase stamps (ecg_tiny_set_stamps)

FusedOpt no_fuse() {
  FusedOpt o{};
  // Write-through gradient rows: the rows leave the XCD L2s while the step runs instead of in the boundary's
  // write-back, and the reduce kernel finds them beyond L2: 11.1 vs 11.4 us/step with plain stores (bench, A/B x2,
  // profiles/r2/bench_slab_wt.txt).
  o.slab_wt = 1;
  return o;
}

// One launch of the step kernel: B workgroups, workgroup b on window X[idx ? idx[b] : b].
struct StepArgs {
  const float* X;  // windows [N][ldx], window length L
  int L;
  long ldx;
  const int* idx;  // [B] rows of X (nullptr: row b)
  const int* Y;    // [N] labels (unused by MODE 1)
  const float* params;
  int nc;
  float* out;  // MODE 0/2: slab [B][out_stride]; MODE 1: logits
  int out_stride, B;
  float inv_B;
  const unsigned char* wprep;  // PF image of ``params`` (bf16 only); nullptr: operands built in LDS from ``params``
  bool packed = false;  // X holds packed bf16 rows (PK kernel: MODE 0, bf16, wprep): gathered rows (idx == nullptr) or,
                        // with an idx, the dataset packed once at pitch pack_ldb(L) (MODE 4; ldx is not read)
};

// MODE 3 (cohort): grid (a.B, M), ``a.params`` / ``a.wprep`` client 0's, ``a.out`` the M * a.B-row slab.
template <int WAVES, int MODE, bool F32, bool PF, bool PK = false>
int launch_step(const StepArgs& a, hipStream_t stream, int M = 1) {
  const Smem sm = make_smem(a.L, WAVES, a.nc, F32);
  auto kern = tiny_ecg_step_kernel<WAVES, MODE, F32, PF, PK>;
  if (sm.bytes > 64 * 1024)
    ECG_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, sm.bytes));
  if (PK && (MODE == 4) != (a.idx != nullptr)) return ecg::kBadArg;  // MODE 0 reads row b, MODE 4 row idx[b]
  const long ldx = MODE == 4 ? (long)reinterpret_cast<uintptr_t>(a.idx) : a.ldx;  // (MODE 4 comment at the kernel)
  hipLaunchKernelGGL(kern, dim3(a.B, M), dim3(WAVES * 64), sm.bytes, stream, a.X, ldx, PF ? a.wprep : nullptr, a.Y,
                     g_stamps, a.L, a.nc, a.params, a.out, a.out_stride, a.inv_B, a.idx, no_fuse().slab_wt);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// The prepared-fragment image of ``params``, one launch.
int launch_prep(const float* params, unsigned char* wprep, hipStream_t stream) {
  if (!params || !wprep) return ecg::kBadArg;
  hipLaunchKernelGGL(tiny_prep_kernel, dim3(1), dim3(256), 0, stream, params, wprep);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

constexpr int kMaxLds = 160 * 1024;

// 16 waves (one tile pair each at L=500) when the per-wave partial slots fit in LDS, else 8.
// ecg_tiny_force_waves overrides it (tests); the choice never changes results beyond fp32 summation order.
// Both precisions take 16 waves once there are >= 16 time tiles: bf16 12.57 vs 12.73 us/step at L=500 with the
// MFMA conv1 (profiles/r1_round_kernel/ab_waves.log; 8 waves had been faster before conv1 moved to MFMA), fp32
// has 4x more MFMA instructions per tile on v_mfma_f32_16x16x4_f32.
int g_forced_waves = 0;  // ecg_tiny_force_waves (tests)
int pick_waves(int L, bool f32) {
  const int Lp = (L + 31) / 32 * 32;
  const int forced = g_forced_waves;
  const bool fit16 = Lp <= 32 * 4 * 16 && make_smem(L, 16, MAX_CLASSES, f32).bytes <= kMaxLds;
  if (forced == 16 && fit16) return 16;
  if (forced == 8) return 8;
  return (fit16 && Lp / 32 >= 16) ? 16 : 8;
}

int check_step_args(int L, int nc, int B, int out_stride, int mode, bool f32 = false) {
  if (L < 8 || B <= 0 || nc < 1 || nc > MAX_CLASSES) return ecg::kBadArg;
  const int Lp = (L + 31) / 32 * 32;
  if (Lp > 32 * 4 * 8 || make_smem(L, 8, MAX_CLASSES, f32).bytes > kMaxLds) return ecg::kTooLarge;  // op-by-op path
  const Layout lay = make_layout(nc);
  if (mode != 1 && out_stride < lay.P + 1) return ecg::kBadArg;
  if (mode == 1 && out_stride < nc) return ecg::kBadArg;
  return ecg::kOk;
}

template <bool F32, bool PF>
int dispatch_cfg(int mode, int waves, const StepArgs& a, hipStream_t stream) {
  if (mode == 2)  // diagnostic (8 waves: the 16-wave two-pass variant spills registers; the production kernel's own
                 // phase stamps come from MODE 0 with ecg_tiny_set_stamps, scripts/diag_step_phases.py)
    return launch_step<8, 2, F32, PF>(a, stream);
  if (mode == 0) return waves == 8 ? launch_step<8, 0, F32, PF>(a, stream) : launch_step<16, 0, F32, PF>(a, stream);
  return waves == 8 ? launch_step<8, 1, F32, PF>(a, stream) : launch_step<16, 1, F32, PF>(a, stream);
}

// prec: 0 = bf16 MFMA operands (AMP), 1 = fp32 (exact f32 MFMA).  ``a.wprep`` (bf16 only): the kernel reads its
// conv operands from that prepared-fragment image, which the caller keeps equal to ``params`` (launch_prep /
// slab_reduce_sgd_kernel); nullptr: the in-LDS build from ``params``.
int step_dispatch(int mode, int prec, const StepArgs& a, hipStream_t stream) {
  if (prec != 0 && prec != 1) return ecg::kBadArg;
  int st = check_step_args(a.L, a.nc, a.B, a.out_stride, mode, prec == 1);
  if (st) return st;
  if (a.wprep && prec == 1) return ecg::kBadArg;
  const int waves = pick_waves(a.L, prec == 1);
  if (a.packed) {
    if (mode != 0 || prec != 0 || !a.wprep) return ecg::kBadArg;
    if (!a.idx)
      return waves == 8 ? launch_step<8, 0, false, true, true>(a, stream)
                        : launch_step<16, 0, false, true, true>(a, stream);
    return waves == 8 ? launch_step<8, 4, false, true, true>(a, stream)
                      : launch_step<16, 4, false, true, true>(a, stream);
  }
  if (prec == 1) return dispatch_cfg<true, false>(mode, waves, a, stream);
  if (a.wprep) return dispatch_cfg<false, true>(mode, waves, a, stream);
  return dispatch_cfg<false, false>(mode, waves, a, stream);
}

// ---------------------------------------------------------------------------- the reduce of one step, host side
// DP-SGD settings of a reduce: clip > 0 (sigma >= 0), the clip-factor vector (one float per slab row) and the device
// step counter.
struct DpArgs {
  float clip, sigma;
  unsigned long long seed;
  float* scale;
  unsigned long long* step;
};

// One step's reduce + SGD, as check_reduce and launch_reduce take it.  Every reduce has the fields down to ``nesterov``
// (callers list them); the ones below it are zero unless a caller names them.
struct Reduce {
  // the slab: M clients' G rows each (back to back) of ``stride`` floats, P gradient columns and the loss column
  const float* slab;
  int G, M, stride, P;
  // state: client c's weights / momentum at the cohort parameter stride, its image at the cohort image stride and its
  // loss word loss_acc[c] (a single client: the plain buffers).  mom may be null when momentum == 0; loss_acc and wprep
  // are nullable
  float* params;
  float* mom;
  float* loss_acc;
  unsigned char* wprep;
  // update
  float lr, momentum, wd;
  int nesterov;
  // a single client's reduce only: apply == 0 just sums - into grad_out [P] (nullable, a copy of the summed gradient)
  // and loss_acc - and then there is no image to keep current
  int apply;
  float* grad_out;
  // the cohort kernel - a cohort of one is still the cohort kernel: the update is always applied (apply is not read),
  // and there is no grad_out
  bool cohort;
  // (nullable) the next step's batch, gathered by this launch's blocks past the reduce blocks
  const GatherArgs* gather;
  // FedProx: mu != 0, or ``prox`` (the stand-alone prox entry points: the prox kernel at mu == 0 too), puts
  // mu * (p - anchor[col]) into the gradient, one anchor [P] for all clients; otherwise the anchor is not looked at
  const float* anchor;
  float mu;
  bool prox;
  // (nullable; cohort only) [M] int32 on the device: the STEPS kernel, which leaves client c as it is when
  // step >= client_steps[c]
  const int* client_steps;
  int step;
  // (nullable) DP-SGD: a clip-factor launch in front, then the DP form of the kernel; there is no PROX x DP kernel
  const DpArgs* dp;
};

// kOk, or the status of a reduce that launch_reduce must not be given - the forms without a kernel among them.
int check_reduce(const Reduce& r) {
  const bool prox = r.prox || r.mu != 0.f;
  if (r.G <= 0 || r.P <= 0 || r.stride < r.P + 1) return ecg::kBadArg;
  if (r.cohort ? (r.M < 1 || r.M > 65535 || r.grad_out) : (r.M != 1 || r.client_steps)) return ecg::kBadArg;
  if ((r.cohort || r.apply) && (!r.params || (r.momentum != 0.f && !r.mom))) return ecg::kBadArg;
  if (r.wprep && !r.cohort && !r.apply) return ecg::kBadArg;
  if ((r.cohort || r.dp) && !r.slab) return ecg::kBadArg;  // (the plain entry points never looked at theirs)
  if (prox && (!r.anchor || r.mu < 0.f || r.dp)) return ecg::kBadArg;
  if (r.client_steps && r.step < 0) return ecg::kBadArg;
  if (r.dp && (r.dp->clip <= 0.f || r.dp->sigma < 0.f || !r.dp->scale || !r.dp->step)) return ecg::kBadArg;
  if (r.dp && (long)r.M * r.G > INT_MAX) return ecg::kTooLarge;  // (a round's rows are bounded by check_cohort_round)
  return ecg::kOk;
}

// The clip factors of all M * G rows (and the advance of the step word) in front of a DP reduce: the two kernels'
// launches differ in ``rows`` and the un-scaling divisor, one client's G, only.
int launch_dp_row_scale(const Reduce& r, hipStream_t stream) {
  const int rows = r.M * r.G;
  const int vec = (r.stride % 4 == 0 && reinterpret_cast<uintptr_t>(r.slab) % 16 == 0) ? 1 : 0;
  const dim3 grid((rows + DP_ROWS_PER_BLOCK - 1) / DP_ROWS_PER_BLOCK), block(DP_ROWS_PER_BLOCK * 64);
  if (r.cohort)
    hipLaunchKernelGGL(dp_row_scale_cohort_kernel<DP_ROWS_PER_BLOCK>, grid, block, 0, stream, r.slab, rows, r.G,
                       r.stride, r.P, r.dp->clip, r.dp->scale, r.dp->step, vec);
  else
    hipLaunchKernelGGL(dp_row_scale_kernel<DP_ROWS_PER_BLOCK>, grid, block, 0, stream, r.slab, r.G, r.stride, r.P,
                       r.dp->clip, r.dp->scale, r.dp->step, vec);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// Check ``r`` and launch it: with DP the clip factors, then exactly one reduce kernel, chosen by (DP, COHORT, PROX,
// STEPS).  Geometry: (P + 1 columns) / kRedColsDefault reduce blocks per client (A/B: profiles/r1_final/ab_red_cols.txt),
// then the gather blocks; ``nred`` is the first gather block - M * blocks, or INT_MAX when a single client's reduce
// has none.
int launch_reduce(const Reduce& r, hipStream_t stream) {
  int st = check_reduce(r);
  if (!st && r.dp) st = launch_dp_row_scale(r, stream);
  if (st) return st;
  constexpr int RC = kRedColsDefault, NT = RC * RED_ROWG;
  int grid = r.M * ((r.P + RC) / RC);
  const int nred = (r.gather || r.cohort) ? grid : INT_MAX;
  GatherArgs ga{};
  if (r.gather) {
    ga = *r.gather;
    const int rpb = gather_rows_per_block(gather_per_row(ga), NT);
    grid += (ga.B + rpb - 1) / rpb;
  }
  const int flags = red_flags(r.cohort ? 1 : r.apply, r.nesterov);
  // every kernel's argument list starts alike (the preloaded dwords and the three pointers behind them); ``tail`` is
  // what its form adds - grad_out first, where the kernel has one - and ends in ``ga``
  auto launch = [&](auto kern, auto... tail) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), 0, stream, r.slab, r.params, r.mom, nred, r.G, r.stride, r.P, flags,
                       r.momentum, r.lr, r.wd, r.wprep, r.loss_acc, tail...);
  };
  const bool prox = r.prox || r.mu != 0.f;
  const int* cs = r.client_steps;
  if (const DpArgs* d = r.dp) {
    const float noise_scale = d->sigma * d->clip / (float)r.G;
    if (!r.cohort) launch(slab_reduce_dp_sgd_kernel<RC>, r.grad_out, d->scale, noise_scale, d->seed, d->step, ga);
    else if (cs) launch(slab_reduce_cohort_dp_steps_sgd_kernel<RC>, d->scale, noise_scale, d->seed, d->step, cs, r.step, ga);
    else launch(slab_reduce_cohort_dp_sgd_kernel<RC>, d->scale, noise_scale, d->seed, d->step, ga);
  } else if (!r.cohort) {
    if (prox) launch(slab_reduce_prox_sgd_kernel<RC>, r.grad_out, r.anchor, r.mu, ga);
    else launch(slab_reduce_sgd_kernel<RC>, r.grad_out, ga);
  } else if (prox) {
    if (cs) launch(slab_reduce_cohort_steps_prox_sgd_kernel<RC>, r.anchor, r.mu, cs, r.step, ga);
    else launch(slab_reduce_cohort_prox_sgd_kernel<RC>, r.anchor, r.mu, ga);
  } else {
    if (cs) launch(slab_reduce_cohort_steps_sgd_kernel<RC>, cs, r.step, ga);
    else launch(slab_reduce_cohort_sgd_kernel<RC>, ga);
  }
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// anchor[0:P] = params[0:P], the first launch of a single client's FedProx round with a snapshot.
int prox_snapshot_launch(const float* params, float* anchor, int P, hipStream_t stream) {
  hipLaunchKernelGGL(prox_snapshot_kernel<256>, dim3((P + 255) / 256), dim3(256), 0, stream, params, anchor, P);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// The cohort forms of the three kernels a production round launches: fp32; bf16 building its operands in LDS (a
// round's first step: ``a.wprep`` null); bf16 on packed rows and the images (``a.packed``).  Arguments are checked
// by check_cohort_round.
int cohort_step_dispatch(int prec, const StepArgs& a, int M, hipStream_t stream) {
  const bool w8 = pick_waves(a.L, prec == 1) == 8;
  if (prec == 1)
    return w8 ? launch_step<8, 3, true, false>(a, stream, M) : launch_step<16, 3, true, false>(a, stream, M);
  if (a.packed)
    return w8 ? launch_step<8, 3, false, true, true>(a, stream, M) : launch_step<16, 3, false, true, true>(a, stream, M);
  if (a.wprep) return ecg::kBadArg;  // the unpacked prepared-fragment kernel has no cohort form
  return w8 ? launch_step<8, 3, false, false>(a, stream, M) : launch_step<16, 3, false, false>(a, stream, M);
}

struct RoundGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int steps = 0;
};

}  // namespace

// ---------------------------------------------------------------------------- C ABI
ECG_API int ecg_tiny_param_count(int nc) { return make_layout(nc).P; }

// Diagnostic: when set, every fused-step workgroup b writes s_memtime at each phase boundary to
// stamps[b*16 + k] (k = 0..6; MODE 2's second pass: 7..13) and
// s_memrealtime at entry/exit to [b*16+15] / [b*16+14].
ECG_API int ecg_tiny_set_stamps(unsigned long long* stamps) {
  g_stamps = stamps;
  return ecg::kOk;
}

// Force the per-step kernel's wave count (8 or 16; 0 = automatic); returns the previous setting.  Tests use it
// to compare paths at the same per-sample summation order.  Graphs captured before a change keep their kernel.
ECG_API int ecg_tiny_force_waves(int waves) {
  const int prev = g_forced_waves;
  g_forced_waves = (waves == 8 || waves == 16) ? waves : 0;
  return prev;
}

ECG_API int ecg_tiny_smem_bytes(int L, int prec) {
  return make_smem(L, pick_waves(L, prec == 1), MAX_CLASSES, prec == 1).bytes;
}

// Bytes of the prepared-fragment image (``wprep`` below; 16-byte aligned device memory).
ECG_API int ecg_tiny_wprep_bytes(void) { return WP_BYTES; }

// Build the prepared-fragment image of ``params`` (bf16 conv operands in MFMA lane order).
ECG_API int ecg_tiny_prep(const float* params, void* wprep, hipStream_t stream) {
  return launch_prep(params, static_cast<unsigned char*>(wprep), stream);
}

// The three entry points below take an optional ``wprep`` (bf16 only): when given, the image is first rebuilt from
// ``params`` (one small launch) and the step kernel reads its conv operands from it (PF path); nullptr builds
// them in every workgroup's LDS.  Both give bitwise-identical results.
static int prep_then(int mode, int prec, const StepArgs& a, hipStream_t stream) {
  if (a.wprep) {
    if (prec != 0) return ecg::kBadArg;
    const int st = launch_prep(a.params, const_cast<unsigned char*>(a.wprep), stream);
    if (st) return st;
  }
  return step_dispatch(mode, prec, a, stream);
}

// One fused training step's gradient pass: writes slab[B][slab_stride] (grads + loss at column P).
ECG_API int ecg_tiny_step_grads(const float* X, int L, long ldx, const int* idx, const int* Y,
                                const float* params, int nc, float* slab, int slab_stride, int B, float inv_B,
                                int prec, void* wprep, hipStream_t stream) {
  return prep_then(0, prec, {X, L, ldx, idx, Y, params, nc, slab, slab_stride, B, inv_B,
                             static_cast<const unsigned char*>(wprep)}, stream);
}

// Diagnostic twin of ecg_tiny_step_grads: every workgroup computes its sample twice (cold, then warm caches).
ECG_API int ecg_tiny_step_grads_twice(const float* X, int L, long ldx, const int* idx, const int* Y,
                                      const float* params, int nc, float* slab, int slab_stride, int B, float inv_B,
                                      int prec, void* wprep, hipStream_t stream) {
  return prep_then(2, prec, {X, L, ldx, idx, Y, params, nc, slab, slab_stride, B, inv_B,
                             static_cast<const unsigned char*>(wprep)}, stream);
}

// Inference: logits[B][nc] for windows X[idx[b]].
ECG_API int ecg_tiny_forward(const float* X, int L, long ldx, const int* idx, const float* params, int nc,
                             float* logits, int B, int prec, void* wprep, hipStream_t stream) {
  return prep_then(1, prec, {X, L, ldx, idx, nullptr, params, nc, logits, nc, B, 0.f,
                             static_cast<const unsigned char*>(wprep)}, stream);
}

ECG_API int ecg_slab_reduce_sgd(const float* slab, int G, int stride, int P, float* params, float* mom,
                                float* grad_out, float* loss_acc, float lr, float momentum, float wd, int nesterov,
                                int apply, void* wprep, hipStream_t stream) {
  Reduce r{slab, G, 1, stride, P, params, mom, loss_acc, static_cast<unsigned char*>(wprep), lr, momentum, wd, nesterov};
  r.apply = apply, r.grad_out = grad_out;
  return launch_reduce(r, stream);
}

// DP-SGD twin of ecg_slab_reduce_sgd (two launches): clip factors of the slab's rows into ``dp_scale`` [G] and
// ``dp_step[0]`` += 1, then the sum of dp_scale[b] * row_b plus dp_sigma * dp_clip / G * z(dp_seed, step, column),
// where ``step`` is the value ``dp_step[0]`` held before the call, through the same SGD epilogue.
ECG_API int ecg_slab_reduce_dp_sgd(const float* slab, int G, int stride, int P, float* params, float* mom,
                                   float* grad_out, float* loss_acc, float lr, float momentum, float wd, int nesterov,
                                   int apply, void* wprep, float dp_clip, float dp_sigma, unsigned long long dp_seed,
                                   float* dp_scale, unsigned long long* dp_step, hipStream_t stream) {
  const DpArgs dp{dp_clip, dp_sigma, dp_seed, dp_scale, dp_step};
  Reduce r{slab, G, 1, stride, P, params, mom, loss_acc, static_cast<unsigned char*>(wprep), lr, momentum, wd, nesterov};
  r.apply = apply, r.grad_out = grad_out, r.dp = &dp;
  return launch_reduce(r, stream);
}

// Diagnostic: z[0:P], the standard normals the DP reduce draws for (seed, step t).
ECG_API int ecg_dp_noise(float* z, int P, unsigned long long seed, unsigned long long t, hipStream_t stream) {
  if (!z || P <= 0) return ecg::kBadArg;
  hipLaunchKernelGGL(dp_noise_kernel<256>, dim3((P + 255) / 256), dim3(256), 0, stream, z, P, seed, t);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// ecg_slab_reduce_sgd with the proximal term mu * (p - anchor[col]) in the gradient (``anchor`` [P], mu >= 0).  It
// always launches the prox kernel: mu == 0 gives ecg_slab_reduce_sgd's bits.
ECG_API int ecg_slab_reduce_prox_sgd(const float* slab, int G, int stride, int P, float* params, float* mom,
                                     float* grad_out, float* loss_acc, float lr, float momentum, float wd, int nesterov,
                                     int apply, void* wprep, const float* anchor, float mu, hipStream_t stream) {
  Reduce r{slab, G, 1, stride, P, params, mom, loss_acc, static_cast<unsigned char*>(wprep), lr, momentum, wd, nesterov};
  r.apply = apply, r.grad_out = grad_out;
  r.anchor = anchor, r.mu = mu, r.prox = true;
  return launch_reduce(r, stream);
}

// The cohort twin on caller-supplied buffers: M clients' G slab rows each, weights / momenta at the cohort parameter
// stride, images at the cohort image stride (nullable), loss words loss_acc[M] (nullable), one ``anchor`` [P] for all.
ECG_API int ecg_slab_reduce_cohort_prox_sgd(const float* slab, int G, int M, int stride, int P, float* params,
                                            float* mom, float* loss_acc, float lr, float momentum, float wd,
                                            int nesterov, void* wprep, const float* anchor, float mu,
                                            hipStream_t stream) {
  Reduce r{slab, G, M, stride, P, params, mom, loss_acc, static_cast<unsigned char*>(wprep), lr, momentum, wd, nesterov};
  r.cohort = true;
  r.anchor = anchor, r.mu = mu, r.prox = true;
  return launch_reduce(r, stream);
}

// ecg_slab_reduce_cohort_prox_sgd's twin with per-client step counts: the reduce of local step ``step`` (>= 0), which
// leaves every client c with ``step`` >= client_steps[c] ([M] int32, device) as it is.  ``mu`` may be 0 (the plain
// STEPS kernel; ``anchor`` is then not looked at).
ECG_API int ecg_slab_reduce_cohort_steps_sgd(const float* slab, int G, int M, int stride, int P, float* params,
                                             float* mom, float* loss_acc, float lr, float momentum, float wd,
                                             int nesterov, void* wprep, const float* anchor, float mu,
                                             const int* client_steps, int step, hipStream_t stream) {
  if (!client_steps) return ecg::kBadArg;
  Reduce r{slab, G, M, stride, P, params, mom, loss_acc, static_cast<unsigned char*>(wprep), lr, momentum, wd, nesterov};
  r.cohort = true;
  r.anchor = anchor, r.mu = mu;
  r.client_steps = client_steps, r.step = step;
  return launch_reduce(r, stream);
}

// The record-level DP-SGD twin of ecg_slab_reduce_cohort_steps_sgd (two launches, no FedProx): the clip factors of all
// M * G rows into ``dp_scale`` [M * G] (un-scaling G) and ``dp_step[0]`` += 1, then per client c the sum of its
// clipped rows plus dp_sigma * dp_clip / G * z(dp_seed, step, column, stream 2 + c), ``step`` the value ``dp_step[0]``
// held before the call.  ``client_steps`` is nullable here: null runs every client.  The argument list is
// ecg_slab_reduce_cohort_steps_sgd's with the DP fields behind ``step``; there is no PROX x DP kernel, so ``mu`` must
// be 0 and ``anchor`` is not looked at.
ECG_API int ecg_slab_reduce_cohort_dp_sgd(const float* slab, int G, int M, int stride, int P, float* params, float* mom,
                                          float* loss_acc, float lr, float momentum, float wd, int nesterov,
                                          void* wprep, const float* anchor, float mu, const int* client_steps,
                                          int step, float dp_clip, float dp_sigma, unsigned long long dp_seed,
                                          float* dp_scale, unsigned long long* dp_step, hipStream_t stream) {
  (void)anchor;
  if (mu != 0.f) return ecg::kBadArg;
  const DpArgs dp{dp_clip, dp_sigma, dp_seed, dp_scale, dp_step};
  Reduce r{slab, G, M, stride, P, params, mom, loss_acc, static_cast<unsigned char*>(wprep), lr, momentum, wd, nesterov};
  r.cohort = true;
  r.client_steps = client_steps, r.step = step;
  r.dp = &dp;
  return launch_reduce(r, stream);
}

// Diagnostic: ecg_dp_noise with the Philox stream word (0: ecg_dp_noise itself; 2 + c: cohort slot c's record-level
// draw).
ECG_API int ecg_dp_noise_stream(float* z, int P, unsigned long long seed, unsigned long long t, unsigned stream_word,
                                hipStream_t stream) {
  if (!z || P <= 0) return ecg::kBadArg;
  hipLaunchKernelGGL(dp_noise_stream_kernel<256>, dim3((P + 255) / 256), dim3(256), 0, stream, z, P, seed, t,
                     (uint32_t)stream_word);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// A local round: ``steps`` times "step kernel, then reduce + SGD kernel" (DP-SGD: step kernel, clip factors, clipped
// and noised reduce + SGD).  ops/_lib.py mirrors this struct field for field and compares its size with
// ecg_tiny_round_sizeof() when it binds the library.
struct EcgTinyRound {
  const float* X;  // dataset windows [N][ldx], window length L
  long ldx;
  const int* idx;  // [steps][B] batch rows, read in place; nullptr: every step reads rows 0..B-1
  const int* Y;    // [N] int32 labels
  float* params;   // flat fp32 weights [P], updated in place
  float* mom;      // [P] (may be null when momentum == 0)
  float* slab;     // [B][slab_stride] gradient rows (scratch)
  float* loss_acc;  // [1] += the summed sample losses of every step (nullable)
  void* wprep;  // PF image (bf16 only, nullable).  The first step builds its operands in LDS - the weights may have
                // been rewritten since the last round - and its SGD epilogue rewrites the image; later steps read it.
  float* xg;    // [2][B][ldg] / yg [2][B] (both or neither; need wprep and idx): the reduce launch of step s
  int* yg;      // gathers step s + 1's windows and labels into buffer (s + 1) & 1, which that step reads by row
  int L, nc, slab_stride, B, steps;
  float lr, momentum, wd;
  int nesterov, prec;
  // DP-SGD (dp_clip > 0): per-sample clip norm C, noise multiplier sigma, the Philox key, the [B] clip factors
  // (scratch) and the 64-bit step counter (device word, advanced by every step).  dp_clip == 0: today's launches.
  float dp_clip, dp_sigma;
  unsigned long long dp_seed;
  float* dp_scale;
  unsigned long long* dp_step;
  void* xbg;  // bf16 [2][B][ldb] (ecg_tiny_gather_halfs; nullable, needs xg): the gather also writes each window as
              // a packed bf16 row into buffer (s + 1) & 1, and step s + 1 runs the kernel that reads those (PK)
  // The dataset packed once (ecg_tiny_pack_dataset; bf16 [N][pack_ldb(L)], nullable) and what a round does with it:
  //   kPrepackGather  the gather blocks copy packed rows xpk[idx[b]] -> xbg[b] (16 bytes per thread) and the labels;
  //                   X is read by the round's first step only.  Needs wprep, idx, yg and xbg; takes no xg.
  //   kPrepackDirect  no gather: steps s > 0 run the PK kernel on xpk itself (MODE 4: row idx[b], label Y[idx[b]]).
  //                   Needs wprep and idx; takes no xg, yg or xbg.
  // Without xpk, ``prepack`` is kPrepackNone.  Every form computes the same bits.
  const void* xpk;
  int prepack;
  // FedProx (prox_mu > 0; not with DP-SGD): every step's gradient gains prox_mu * (w - prox_anchor), prox_anchor [P]
  // a buffer of its own (never ``params``).  With prox_snapshot the round's first launch copies params -> prox_anchor
  // (prox_snapshot_kernel, enqueued and captured alike: a replayed graph re-anchors every round); without it the
  // anchor is read as the caller left it.  prox_mu == 0: the other two are not read, today's launches.
  float prox_mu;
  float* prox_anchor;
  int prox_snapshot;
};
enum { kPrepackNone = 0, kPrepackGather = 1, kPrepackDirect = 2 };

ECG_API int ecg_tiny_round_sizeof(void) { return (int)sizeof(EcgTinyRound); }

static int check_round(const EcgTinyRound* r) {
  if (!r || r->steps < 1 || !r->X || !r->Y || !r->params || !r->slab) return ecg::kBadArg;
  if (r->prec != 0 && r->prec != 1) return ecg::kBadArg;
  if (r->wprep && r->prec != 0) return ecg::kBadArg;
  if (r->prepack == kPrepackNone) {
    if (r->xpk) return ecg::kBadArg;
    if ((!r->xg) != (!r->yg) || (r->xg && (!r->wprep || !r->idx))) return ecg::kBadArg;
    if (r->xbg && !r->xg) return ecg::kBadArg;
  } else {
    if (r->prepack != kPrepackGather && r->prepack != kPrepackDirect) return ecg::kBadArg;
    if (!r->xpk || !r->wprep || !r->idx || r->xg) return ecg::kBadArg;
    const bool bufs = r->prepack == kPrepackGather;  // the packed ping-pong and its labels: both or neither
    if ((r->yg != nullptr) != bufs || (r->xbg != nullptr) != bufs) return ecg::kBadArg;
    if (reinterpret_cast<uintptr_t>(r->xpk) % 16 != 0) return ecg::kBadArg;
  }
  if (r->dp_clip < 0.f || r->dp_sigma < 0.f || (r->dp_sigma > 0.f && r->dp_clip == 0.f)) return ecg::kBadArg;
  if (r->dp_clip > 0.f && (!r->dp_scale || !r->dp_step)) return ecg::kBadArg;
  if (r->prox_mu < 0.f) return ecg::kBadArg;
  if (r->prox_mu > 0.f && (!r->prox_anchor || r->prox_anchor == r->params || r->dp_clip > 0.f)) return ecg::kBadArg;
  return check_step_args(r->L, r->nc, r->B, r->slab_stride, 0, r->prec == 1);
}

// The gather ping-pong of a round whose steps take ``rows`` windows each: xg [2][rows][ldg], yg [2][rows] and
// (nullable) the packed bf16 rows xbg [2][rows][ldb].  Step s > 0 reads buffer s & 1, which the reduce launch of step
// s - 1 filled (stream order: that buffer's previous reader, step s - 2's kernel, finished before that reduce
// started).  With xbg the step reads the packed rows instead of xg (xg is still written: it is the unpacked kernel's
// input).  With ``xpk``, the dataset packed once, there is no xg at all: the gather copies packed rows into xbg.
struct GatherBufs {
  float* xg;
  int* yg;
  __bf16* xbg;
  const __bf16* xpk = nullptr;
};
// What every gather launch of the round shares; gather_fill sets the rest.
static GatherArgs gather_args(const float* X, long ldx, const int* Y, int L, int rows) {
  const int vec = (L % 4 == 0 && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0) ? 1 : 0;
  return {X, ldx, nullptr, Y, nullptr, nullptr, L, (L + 3) / 4 * 4, rows, vec, nullptr, pack_ldb(L), nullptr};
}
// The reduce launch of step s gathers step s + 1's batch ``idx_next`` into buffer (s + 1) & 1.
static void gather_fill(GatherArgs& ga, const GatherBufs& g, int s, const int* idx_next) {
  const long buf = (long)((s + 1) & 1) * ga.B;
  ga.idx = idx_next;
  ga.xg = g.xg ? g.xg + buf * ga.ldg : nullptr;
  ga.yg = g.yg + buf;
  ga.xbg = g.xbg ? g.xbg + buf * ga.ldb : nullptr;
  ga.xpk = g.xpk;
}
// Step s reads buffer s & 1 by row.
static void gather_read(StepArgs& a, const GatherArgs& ga, const GatherBufs& g, int s) {
  const long buf = (long)(s & 1) * ga.B;
  a.X = g.xg ? g.xg + buf * ga.ldg : nullptr;  // (null with xpk: the packed rows below)
  a.ldx = ga.ldg;
  a.idx = nullptr;
  a.Y = g.yg + buf;
  if (g.xbg) {
    a.X = reinterpret_cast<const float*>(g.xbg + buf * ga.ldb);
    a.ldx = ga.ldb / 2;
    a.packed = true;
  }
}

// Enqueue a checked round on ``stream`` (a capturing stream included): two launches per step, three with DP-SGD;
// FedProx with a snapshot adds one launch per round in front.
// (Warm-up loads of the next step's windows in the step kernel's tail measured neutral - 11.11 vs 11.08 us/step,
// the windows already sit in the Infinity Cache; profiles/r2/bench_prefetch.txt - and were removed.)
static int enqueue_round(const EcgTinyRound& r, hipStream_t stream) {
  const int P = make_layout(r.nc).P;
  if (r.prox_mu > 0.f && r.prox_snapshot) {
    const int st = prox_snapshot_launch(r.params, r.prox_anchor, P, stream);
    if (st) return st;
  }
  unsigned char* wprep = static_cast<unsigned char*>(r.wprep);
  const __bf16* xpk = static_cast<const __bf16*>(r.xpk);
  const bool gathers = r.xg || r.prepack == kPrepackGather;
  const GatherBufs bufs{r.xg, r.yg, static_cast<__bf16*>(r.xbg), r.prepack == kPrepackGather ? xpk : nullptr};
  GatherArgs ga = gather_args(r.X, r.ldx, r.Y, r.L, r.B);
  const DpArgs dp{r.dp_clip, r.dp_sigma, r.dp_seed, r.dp_scale, r.dp_step};
  Reduce red{r.slab, r.B, 1, r.slab_stride, P, r.params, r.mom, r.loss_acc, wprep, r.lr, r.momentum, r.wd, r.nesterov};
  red.apply = 1;
  red.anchor = r.prox_anchor, red.mu = r.prox_mu;  // (check_round: not with DP-SGD)
  if (r.dp_clip > 0.f) red.dp = &dp;
  for (int s = 0; s < r.steps; ++s) {
    const int* idx = r.idx ? r.idx + (long)s * r.B : nullptr;
    const bool gather_next = gathers && s + 1 < r.steps;
    if (gather_next) gather_fill(ga, bufs, s, idx + r.B);
    StepArgs a{r.X, r.L, r.ldx, idx, r.Y, r.params, r.nc, r.slab, r.slab_stride, r.B, 1.0f / (float)r.B,
               s == 0 ? nullptr : wprep};
    if (gathers && s > 0) gather_read(a, ga, bufs, s);
    if (r.prepack == kPrepackDirect && s > 0) {  // the PK kernel on the packed dataset itself, row idx[b]
      a.X = reinterpret_cast<const float*>(xpk);
      a.packed = true;
    }
    int st = step_dispatch(0, r.prec, a, stream);
    if (st) return st;
    red.gather = gather_next ? &ga : nullptr;
    st = launch_reduce(red, stream);
    if (st) return st;
  }
  return ecg::kOk;
}

// ``enqueue(stream)``'s launches captured into one instantiated hipGraph (the handle of ecg_round_graph_*).
template <class Enqueue>
static int capture_round(void** handle, int steps, Enqueue enqueue) {
  hipStream_t cap;
  ECG_HIP_CHECK(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
  RoundGraph* rg = new RoundGraph();
  rg->steps = steps;
  hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    delete rg;
    (void)hipStreamDestroy(cap);
    return ecg::kHipError;
  }
  const int st = enqueue(cap);
  e = hipStreamEndCapture(cap, &rg->graph);
  (void)hipStreamDestroy(cap);
  if (st != 0 || e != hipSuccess) {
    if (rg->graph) (void)hipGraphDestroy(rg->graph);
    delete rg;
    return st ? st : ecg::kHipError;
  }
  e = hipGraphInstantiate(&rg->exec, rg->graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(rg->graph);
    delete rg;
    return ecg::kHipError;
  }
  *handle = rg;
  return ecg::kOk;
}

// The round's kernels enqueued on ``stream``, without a graph.
ECG_API int ecg_tiny_round_enqueue(const EcgTinyRound* round, hipStream_t stream) {
  const int st = check_round(round);
  return st ? st : enqueue_round(*round, stream);
}

// The same launches captured into one hipGraph (replayed by ecg_round_graph_launch).  All pointers are baked
// into the graph: callers keep the buffers alive and refill ``idx`` in place.
ECG_API int ecg_tiny_round_capture(void** handle, const EcgTinyRound* round) {
  if (!handle) return ecg::kBadArg;
  const int st = check_round(round);
  if (st) return st;
  return capture_round(handle, round->steps, [&](hipStream_t cap) { return enqueue_round(*round, cap); });
}

// Floats of the gather buffer ``xg`` of a round (its ``yg`` holds 2 * B int32).
ECG_API long ecg_tiny_gather_floats(int L, int B) { return 2L * B * ((L + 3) / 4 * 4); }

// bf16 elements of the packed gather buffer ``xbg`` of a round.
ECG_API long ecg_tiny_gather_halfs(int L, int B) { return 2L * B * pack_ldb(L); }

// bf16 elements of the dataset packed once (``EcgTinyRound::xpk``): N rows of pack_ldb(L).
ECG_API long ecg_tiny_pack_halfs(int L, long N) { return N * pack_ldb(L); }

// Pack the dataset X [N][ldx] (window length L) into ``out`` [N][pack_ldb(L)], 16-byte aligned: every row, pads
// included, is written (tiny_pack_rows_kernel).  Callers repeat it after they rewrite X.
ECG_API int ecg_tiny_pack_dataset(const float* X, long ldx, long N, int L, void* out, hipStream_t stream) {
  if (!X || !out || N <= 0 || L < 1 || ldx < L || reinterpret_cast<uintptr_t>(out) % 16 != 0) return ecg::kBadArg;
  const bool vec = L % 4 == 0 && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0;
  const unsigned grid = (unsigned)(N < (1L << 20) ? N : (1L << 20));  // rows beyond it: the kernel's grid stride
  __bf16* o = static_cast<__bf16*>(out);
  if (vec)
    hipLaunchKernelGGL(tiny_pack_rows_kernel<true>, dim3(grid), dim3(128), 0, stream, X, ldx, N, L, o);
  else
    hipLaunchKernelGGL(tiny_pack_rows_kernel<false>, dim3(grid), dim3(128), 0, stream, X, ldx, N, L, o);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

ECG_API int ecg_round_graph_launch(void* handle, hipStream_t stream) {
  if (!handle) return ecg::kBadArg;
  RoundGraph* rg = static_cast<RoundGraph*>(handle);
  ECG_HIP_CHECK(hipGraphLaunch(rg->exec, stream));
  return ecg::kOk;
}

// Upload a round graph's executable to the device ahead of its first replay (keeps that one-time cost out of a
// timed region; the replay itself is unchanged).
ECG_API int ecg_round_graph_upload(void* handle, hipStream_t stream) {
  if (!handle) return ecg::kBadArg;
  RoundGraph* rg = static_cast<RoundGraph*>(handle);
  ECG_HIP_CHECK(hipGraphUpload(rg->exec, stream));
  return ecg::kOk;
}

ECG_API int ecg_round_graph_destroy(void* handle) {
  if (!handle) return ecg::kOk;
  RoundGraph* rg = static_cast<RoundGraph*>(handle);
  if (rg->exec) (void)hipGraphExecDestroy(rg->exec);
  if (rg->graph) (void)hipGraphDestroy(rg->graph);
  delete rg;
  return ecg::kOk;
}

// ---------------------------------------------------------------------------- cohort rounds
// Floats between two clients' weights (and momenta) in a cohort's ``params`` / ``mom``: >= P, a multiple of 64.
ECG_API int ecg_tiny_cohort_param_stride(int nc) { return cohort_pstride(make_layout(nc).P); }

// Bytes between two clients' prepared-fragment images in a cohort's ``wprep``: >= ecg_tiny_wprep_bytes(), 16 | it.
ECG_API int ecg_tiny_cohort_wprep_stride(void) { return kCohortWprepStride; }

// A cohort round: M virtual clients of B windows each start from ``global_params`` (fanout), run ``steps`` local SGD
// steps side by side - one step launch and one reduce launch per step for the whole cohort - and their weights' mean
// (ascending client order, cohort_mean_kernel) becomes ``global_params``.  Client c: weights / momentum at
// ``params`` / ``mom`` + c * ecg_tiny_cohort_param_stride(nc) floats, image at ``wprep`` + c *
// ecg_tiny_cohort_wprep_stride() bytes (zero-initialised by the caller, like a single client's), loss word
// loss_acc[c], slab rows [c * B, (c + 1) * B), columns [c * B, (c + 1) * B) of every ``idx`` row.  bf16 rounds run
// like a packed EcgTinyRound - the first step builds its operands in LDS, later steps read the images and the packed
// rows gathered by the previous reduce - and need wprep, xg, yg and xbg, sized for M * B rows
// (ecg_tiny_gather_floats / _halfs(L, M * B)); fp32 rounds take none of them.  Record-level DP-SGD: the dp_* fields.
// The close: with the cdp_* fields, server_lr, server_opt and server_delta all zero (server_lr 1 counts as zero) it is
// cohort_mean_kernel; anything else - client_weight and robust_trim among it - is ecg::tiny::cohort_close (include/tiny_ecg_close.h), which picks its kernel by
// server_delta, then server_opt.
// ops/_lib.py mirrors this struct (TinyCohortRound) and checks its size against ecg_tiny_cohort_round_sizeof().
struct EcgTinyCohortRound {
  const float* X;
  long ldx;
  const int* idx;  // [steps][M * B] batch rows, read in place
  const int* Y;
  float* params;         // [M][pstride] client weights (scratch between rounds unless fanout == 0)
  float* mom;            // [M][pstride] (may be null when momentum == 0)
  float* slab;           // [M * B][slab_stride]
  float* loss_acc;       // [M] += each client's summed sample losses (nullable)
  void* wprep;           // [M] images at the wprep stride (bf16)
  float* xg;             // [2][M * B][ldg] (bf16)
  int* yg;               // [2][M * B] (bf16)
  void* xbg;             // bf16 [2][M * B][ldb] (bf16)
  float* global_params;  // [P]: read by the fan-out, written by the mean
  int L, nc, slab_stride, B, steps, M;
  int fanout;  // 0: the clients start from what ``params`` / ``mom`` hold (tests: distinct weights per client)
  float lr, momentum, wd;
  int nesterov, prec;
  // Client-level DP: clip norm C of a client's round delta (0: no clipping, every factor is 1), the noise multiplier
  // of this rank's share (noise std = cdp_sigma * cdp_clip / M per parameter; a driver of W ranks that averages their
  // weights passes sigma / sqrt(W)), the server step size eta (0 means 1), the Philox key, the [M] clip factors and
  // delta norms of the last round, and the 64-bit round counter (device word, advanced by every round's close).
  float cdp_clip, cdp_sigma, server_lr;
  unsigned long long cdp_seed;
  float* cdp_scale;
  float* cdp_norm;
  unsigned long long* cdp_round;
  // Server optimizer on the averaged (clipped, noised) client delta: 0 none (the plain server step), 1 sgdm (FedAvgM),
  // 2 adagrad, 3 adam, 4 yogi (cohort_server_opt_kernel states the rules); beta1, beta2 in [0, 1), tau > 0 (2..4), and
  // the server state m / v [P] (fp32, read and written by every round's close; v may be null for sgdm).  With
  // server_opt == 0 the other five fields are not read.
  int server_opt;
  float server_beta1, server_beta2, server_tau;
  float* server_m;
  float* server_v;
  // The split close (nullable): [P], receives this round's averaged, clipped, noised delta - the value the closes above
  // form, bit for bit - in place of any server step.  ``global_params`` then still holds the round's starting weights
  // when the round ends, and server_opt, server_m and server_v are not read; it needs cdp_scale, cdp_norm and
  // cdp_round.  Null: the round issues the launches it issues without this field.
  float* server_delta;
  // FedProx (prox_mu > 0): every client's local steps add prox_mu * (w - global_params) to the gradient.  The anchor is
  // ``global_params`` itself - the fan-out leaves the round's starting weights there and nothing writes them before
  // the close, whichever close it is, nor with fanout == 0.  prox_mu == 0: the launches of before.
  float prox_mu;
  // Unequal local work (nullable): [M] int32 on the device, client c runs the first client_steps[c] of the round's
  // ``steps`` local steps and is frozen for the rest (slab_reduce_body's STEPS form, with step = s in every step's
  // reduce; the step launches and the gather do not change, so the ``idx`` rows of a frozen client's steps are still
  // read and must be valid dataset rows).  The caller guarantees 1 <= client_steps[c] <= steps - device values cannot
  // be range-checked here, and a bf16 round's first reduce is what writes a client's whole image.  Read when a
  // round runs, not when it is captured: one graph serves every round's values.
  const int* client_steps;
  // A weighted close (nullable): [M] fp32 on the device, Delta = sum_c client_weight[c] * d_c in ascending order - the
  // close is always ecg::tiny::cohort_close with these weights (CohortClose::weight), never cohort_mean_kernel.  It
  // needs cdp_scale, cdp_norm and cdp_round and cdp_clip == 0.  Read when a round runs, like client_steps.
  const float* client_weight;
  // A robust close (robust_trim k != 0): the coordinate-wise trimmed mean of the clients' deltas, k dropped at each end
  // (CohortClose::trim; the median at k = (M - 1) / 2), through ecg::tiny::cohort_close.  It needs 1 <= k, 2 k < M <=
  // 64, cdp_scale, cdp_norm and cdp_round, no clip, noise or client_weight, and ``robust_scratch`` [P] unless
  // server_delta is set.  A scalar baked into a captured graph: a trainer's M and k are fixed.  Both zero: the
  // launches of before.
  int robust_trim;
  float* robust_scratch;
  // Record-level DP-SGD inside the cohort (dp_clip > 0; not with FedProx): every client's every local step clips its B
  // per-sample gradients to l2 norm C and adds noise of standard deviation dp_sigma * dp_clip / B per parameter, drawn
  // from Philox stream 2 + c of (dp_seed, the step word) for cohort slot c - three launches per step (step, clip
  // factors, DP cohort reduce; launch_reduce).  dp_scale: [M * B] clip factors (scratch); dp_step: the
  // 64-bit step word (device), advanced once per cohort step whichever clients are frozen.  Independent of the close.
  // All zero / null: the launches of before.
  float dp_clip, dp_sigma;
  unsigned long long dp_seed;
  float* dp_scale;
  unsigned long long* dp_step;
};

ECG_API int ecg_tiny_cohort_round_sizeof(void) { return (int)sizeof(EcgTinyCohortRound); }

// A close with a server step runs in place of the mean: with a clip norm, with a server step size other than 1 (0
// means 1), or with a server optimizer.
static bool cohort_dp_on(const EcgTinyCohortRound& r) {
  return r.cdp_clip > 0.f || (r.server_lr != 0.f && r.server_lr != 1.f) || r.server_opt != 0;
}

// The round ends on ecg::tiny::cohort_close, not on cohort_mean_kernel.
static bool cohort_close_on(const EcgTinyCohortRound& r) {
  return cohort_dp_on(r) || r.server_delta || r.client_weight || r.robust_trim != 0;
}

// The round's close as ecg::tiny::cohort_close takes it.
static CohortClose cohort_close_args(const EcgTinyCohortRound& r) {
  return {r.params,   r.global_params, make_layout(r.nc).P, r.M,           r.cdp_clip,    r.cdp_sigma,
          r.server_lr, r.cdp_seed,     r.cdp_round,         r.cdp_scale,   r.cdp_norm,    r.server_opt,
          r.server_beta1, r.server_beta2, r.server_tau,     r.server_m,    r.server_v,    r.server_delta,
          r.client_weight, r.robust_trim, r.robust_scratch};
}

static int check_cohort_round(const EcgTinyCohortRound* r) {
  if (!r || r->steps < 1 || r->M < 1 || r->M > 65535) return ecg::kBadArg;  // (M is the grid's y extent)
  if (!r->X || !r->Y || !r->idx || !r->params || !r->slab || !r->global_params) return ecg::kBadArg;
  if (r->momentum != 0.f && !r->mom) return ecg::kBadArg;
  if (r->prec != 0 && r->prec != 1) return ecg::kBadArg;
  const bool gath = r->wprep && r->xg && r->yg && r->xbg, none = !r->wprep && !r->xg && !r->yg && !r->xbg;
  if (r->prec == 0 ? !gath : !none) return ecg::kBadArg;
  const int st = check_step_args(r->L, r->nc, r->B, r->slab_stride, 0, r->prec == 1);
  if (st) return st;
  // the slab and gather buffer resources hold byte sizes in 32 bits, and their row offsets are ints
  const long rows = (long)r->M * r->B;
  if (rows * r->slab_stride * 4 > INT_MAX || rows * (pack_ldb(r->L) + 8) * 4 > INT_MAX) return ecg::kTooLarge;
  if (r->prox_mu < 0.f) return ecg::kBadArg;
  if (r->dp_clip < 0.f || r->dp_sigma < 0.f || (r->dp_sigma > 0.f && r->dp_clip == 0.f)) return ecg::kBadArg;
  if (r->dp_clip > 0.f && (!r->dp_scale || !r->dp_step || r->prox_mu > 0.f)) return ecg::kBadArg;
  if (cohort_close_on(*r)) return check_cohort_close(cohort_close_args(*r));
  // the plain mean reads none of the close's fields; a negative clip norm, or noise without a clip norm, is an error
  return (r->cdp_clip < 0.f || r->cdp_sigma != 0.f) ? ecg::kBadArg : ecg::kOk;
}

static int enqueue_cohort_round(const EcgTinyCohortRound& r, hipStream_t stream) {
  const int P = make_layout(r.nc).P, rows = r.M * r.B;
  unsigned char* wprep = static_cast<unsigned char*>(r.wprep);
  const GatherBufs bufs{r.xg, r.yg, static_cast<__bf16*>(r.xbg)};  // M * B rows each (bf16: all three, fp32: none)
  const bool bf16 = r.prec == 0;
  if (r.fanout) {
    hipLaunchKernelGGL(cohort_fanout_kernel<256>, dim3((P + 255) / 256, r.M), dim3(256), 0, stream, r.global_params,
                       r.params, r.mom, P);
    ECG_HIP_CHECK(hipGetLastError());
  }
  GatherArgs ga = gather_args(r.X, r.ldx, r.Y, r.L, rows);
  const DpArgs dp{r.dp_clip, r.dp_sigma, r.dp_seed, r.dp_scale, r.dp_step};
  Reduce red{r.slab, r.B, r.M, r.slab_stride, P, r.params, r.mom, r.loss_acc, wprep, r.lr, r.momentum, r.wd, r.nesterov};
  red.cohort = true;
  red.anchor = r.global_params, red.mu = r.prox_mu;  // (check_cohort_round: not with DP-SGD)
  red.client_steps = r.client_steps;
  if (r.dp_clip > 0.f) red.dp = &dp;
  for (int s = 0; s < r.steps; ++s) {
    const int* idx = r.idx + (long)s * rows;
    const bool gather_next = bf16 && s + 1 < r.steps;
    if (gather_next) gather_fill(ga, bufs, s, idx + rows);
    StepArgs a{r.X, r.L, r.ldx, idx, r.Y, r.params, r.nc, r.slab, r.slab_stride, r.B, 1.0f / (float)r.B, nullptr};
    if (bf16 && s > 0) {
      gather_read(a, ga, bufs, s);
      a.wprep = wprep;
    }
    int st = cohort_step_dispatch(r.prec, a, r.M, stream);
    if (st) return st;
    red.gather = gather_next ? &ga : nullptr, red.step = s;
    st = launch_reduce(red, stream);
    if (st) return st;
  }
  if (cohort_close_on(r)) return cohort_close(cohort_close_args(r), stream);
  hipLaunchKernelGGL(cohort_mean_kernel<256>, dim3((P + 255) / 256), dim3(256), 0, stream, r.params, r.global_params,
                     P, r.M, 1.0f / (float)r.M);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

ECG_API int ecg_tiny_cohort_round_enqueue(const EcgTinyCohortRound* round, hipStream_t stream) {
  const int st = check_cohort_round(round);
  return st ? st : enqueue_cohort_round(*round, stream);
}

// The cohort round as one hipGraph; the handle is the one ecg_round_graph_launch / _upload / _destroy take.
ECG_API int ecg_tiny_cohort_round_capture(void** handle, const EcgTinyCohortRound* round) {
  if (!handle) return ecg::kBadArg;
  const int st = check_cohort_round(round);
  if (st) return st;
  return capture_round(handle, round->steps, [&](hipStream_t cap) { return enqueue_cohort_round(*round, cap); });
}
