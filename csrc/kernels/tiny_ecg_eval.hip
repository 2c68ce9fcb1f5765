// TinyECG evaluation for gfx950 (MI355X, CDNA4): a persistent, forward-only kernel that reduces the metrics of a
// set of windows inside the launch.
//
// The forward of the training step (tiny_ecg_step.hip, MODE 1) spends one 16-wave workgroup, the full training LDS
// carve and three workgroup barriers on every window, and leaves an [N, C] logits tensor for torch to reduce.  A
// forward pass keeps nothing for a backward pass, so here ONE WAVE owns a window from its first load to its loss:
//   window row -> registers (16-byte bounded loads, or 4-byte ones for rows that are not 16-byte aligned; the NEXT
//   window's loads are in flight while this one computes) -> the wave's own LDS copy xs
//   -> conv1 (1->16, k7) + bias + ReLU on MFMA (operand {x[t-3..t+3], 1} built from xs, bias = 8th reduction column)
//   -> h1 through a per-wave LDS RING: one tile pair (32 time steps) plus 4 halo rows, 36 rows x 32 B
//   -> conv2 (16->16, k5) + bias + ReLU on MFMA (bf16 bias riding in the K padding), pooled in registers
//   -> head (16 -> C <= 16), argmax (ties to the lowest index), softmax cross-entropy in fp32.
// The operand numerics are those of the training forward (same prepared-fragment image WP_FRAGF / WP_AW1, same
// bf16 roundings, fp32 accumulation); only fp32 summation order of the pooling differs.
//
// h1 ring, not the whole window: the ring costs 1,152 B per wave against (L + 8) x 32 B (16.6 KB at L = 500) for a
// whole-window h1, so LDS (3.3 KB per wave at L = 500 including xs) never limits occupancy - registers do.  Ring
// row r of pair p holds h1 at time 32p - 2 + r: conv1 of pair p computes times [32p + 2, 32p + 34) into rows 4..35
// and rows 0..3 are carried over from rows 32..35 of the previous pair (a prologue tile provides times -2..1).
//
// No workgroup-wide barrier anywhere: a workgroup is just 4 independent waves with disjoint LDS slices.  A wave's
// LDS accesses execute in program order, so the cross-lane hand-offs through xs / the ring need only a compiler
// fence.  The grid is persistent (CUs x resident workgroups, capped by the work) and wave g of G evaluates windows
// g, g + G, g + 2G, ...: a static stride, no work queue, and nothing depends on where a workgroup runs.
//
// Reduction (deterministic): every wave keeps its loss partial in fp64 and its counts (windows, correct, the
// confusion matrix: 4 entries per lane) in integer registers.  At its end it stores the loss partial write-through
// to scratch[g] and adds its non-zero counts to the output record with 64-bit INTEGER atomics (exact in any
// order); a second one-block launch sums the G loss partials in a fixed order.  No float atomics.
#include "../include/ecg_common.h"
#include "../include/tiny_ecg.h"

#include <cstdint>

namespace {

using namespace ecg::tiny;

constexpr int EW = 4;                  // waves per workgroup (one per SIMD); they never synchronise
constexpr int RING_ROWS = 36;          // h1 ring: a tile pair + 4 halo rows
constexpr int kMaxEvalWaves = 16384;   // bound of the loss-partial scratch (grid <= kMaxEvalWaves / EW workgroups)
constexpr int FIN_NT = 256;            // threads of the finalize block

__host__ __device__ inline int round_lp(int L) { return (L + 31) / 32 * 32; }
// per-wave LDS: xs [Lp + 24] fp32 (xs[t + 8] = x[t], zero outside the row), then the h1 ring [36][16] bf16
constexpr int XS_HALO = 8;
__host__ __device__ inline int xs_floats(int Lp) { return Lp + XS_HALO + 16; }
__host__ __device__ inline int wave_lds_bytes(int Lp) { return xs_floats(Lp) * 4 + RING_ROWS * C * 2; }

// Order this wave's LDS accesses for the compiler (the hardware runs one wave's LDS instructions in order).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A window row in registers: VEC - float4 q = lane + 64k in v[4k .. 4k+3]; else element lane + 64k in v[k].
struct XRegs {
  float v[16];
};

template <bool VEC>
__device__ __forceinline__ void load_x(const float* xrow, int L, int Lp, int lane, XRegs& r) {
  // exactly the row: a load at or past its end reads 0 (the conv padding up to Lp) and never touches memory
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(xrow, (long)L * 4);
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (256 * k < Lp) {  // wave-uniform
        const f32x4 q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, (lane + 64 * k) * 16, 0, 0));
#pragma unroll
        for (int j = 0; j < 4; ++j) r.v[4 * k + j] = q[j];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (64 * k < Lp) r.v[k] = ld_bounded(xr, (lane + 64 * k) * 4);
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void put_x(float* xs, int Lp, int lane, const XRegs& r) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * (lane + 64 * k);
      if (256 * k < Lp && e < Lp)
        *reinterpret_cast<f32x4*>(xs + XS_HALO + e) = f32x4{r.v[4 * k], r.v[4 * k + 1], r.v[4 * k + 2], r.v[4 * k + 3]};
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int e = lane + 64 * k;
      if (64 * k < Lp && e < Lp) xs[XS_HALO + e] = r.v[k];
    }
  }
}

// out: {double loss_sum, u64 count, u64 correct, u64 conf[nc][nc]} (zeroed by a memset node before this launch).
template <bool VEC>
__global__ __launch_bounds__(EW * 64) void tiny_ecg_eval_kernel(
    const float* __restrict__ X, int L, long ldx,  // windows [.., ldx], window length L
    const int* __restrict__ idx,                   // [N] rows of X (nullptr: row i)
    const int* __restrict__ Y,                     // labels by row of X (nullptr: inference only)
    int N, const float* __restrict__ params, int nc,
    const unsigned char* __restrict__ wprep,       // prepared-fragment image of ``params``
    double* __restrict__ partials,                 // [gridDim.x * EW] loss partials
    unsigned long long* __restrict__ out, int* __restrict__ pred, float* __restrict__ logits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int h = lane >> 4, c = lane & 15;
  const int Lp = round_lp(L), NP = Lp / 32;
  unsigned char* mine = smem + w * wave_lds_bytes(Lp);
  float* xs = reinterpret_cast<float*>(mine);
  __bf16* ring = reinterpret_cast<__bf16*>(mine + xs_floats(Lp) * 4);
  const int gw = (int)blockIdx.x * EW + w, G = (int)gridDim.x * EW;
  const Layout lay = make_layout(nc);

  // conv operands: image -> VGPRs, once per wave (conv1's A operand lives in quarter 0, the rest is K padding)
  const __bf16* wb = reinterpret_cast<const __bf16*>(wprep);
  bf16x8 aw, Wf[3], Bone;
#pragma unroll
  for (int j = 0; j < 8; ++j) aw[j] = Bone[j] = ecg::to_bf16(0.f);
  if (h == 0) aw = *reinterpret_cast<const bf16x8*>(wb + WP_AW1 + c * 8);
  if (h == 2) Bone[0] = ecg::to_bf16(1.f);  // conv2's bias row: B rows r = 80..95 are {1, 0, ...}
#pragma unroll
  for (int s = 0; s < 3; ++s) Wf[s] = *reinterpret_cast<const bf16x8*>(wb + WP_FRAGF + (s * 64 + lane) * 8);
  // head: lane n (< nc, every quarter) holds row n of Wh and bh[n] in fp32
  float wh[C], bh = 0.f;
#pragma unroll
  for (int j = 0; j < C; ++j) wh[j] = c < nc ? params[lay.wh + c * C + j] : 0.f;
  if (c < nc) bh = params[lay.bh + c];

  // xs halo: x[-8 .. -1] and x[Lp .. Lp + 15] are zero and never rewritten (put_x writes x[0 .. Lp - 1]); the front
  // halo doubles as the all-zero operand of the lanes that have no time step
  if (lane < XS_HALO) xs[lane] = 0.f;
  if (lane < 16) xs[Lp + XS_HALO + lane] = 0.f;

  double loss_acc = 0.0;
  unsigned cnt = 0u, corr = 0u, conf[4] = {0u, 0u, 0u, 0u};  // conf: entries 4*lane .. 4*lane + 3 of [nc][nc]

  auto row_of = [&](int i) { return __builtin_amdgcn_readfirstlane(idx ? idx[i] : i); };
  // conv1 + bias + ReLU of times t0 .. t0 + 15 into ring rows row0 .. row0 + 15 (exactly 0 outside [0, L))
  auto conv1_tile = [&](int t0, int row0) {
    const int t = t0 + c;
    const bool valid = h == 0 && t >= 0 && t < L;
    const int a = valid ? t + XS_HALO - 3 : 0;  // x[t - 3 + j] = xs[a + j]; no time step: xs[0 .. 6] = 0
    bf16x8 Bx;
#pragma unroll
    for (int j = 0; j < K1; ++j) Bx[j] = ecg::to_bf16(xs[a + j]);
    Bx[7] = ecg::to_bf16(valid ? 1.f : 0.f);
    const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, Bx, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    bf16x4 o;  // acc[i] = conv1(x)[t][co = 4h + i] + bias
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = ecg::to_bf16(fmaxf(acc[i], 0.f));
    *reinterpret_cast<bf16x4*>(ring + (row0 + c) * C + 4 * h) = o;
  };

  int i = gw, row = 0, ylab = 0;
  XRegs xr;
  if (i < N) {
    row = row_of(i);
    load_x<VEC>(X + (long)row * ldx, L, Lp, lane, xr);
    if (Y) ylab = Y[row];
  }
  while (i < N) {
    wave_lds_sync();  // the previous window's reads of xs come first
    put_x<VEC>(xs, Lp, lane, xr);
    const int y = __builtin_amdgcn_readfirstlane(ylab);
    const int inext = i + G;
    if (inext < N) {  // the next window's loads fly while this one computes
      row = row_of(inext);
      load_x<VEC>(X + (long)row * ldx, L, Lp, lane, xr);
      if (Y) ylab = Y[row];
    }
    wave_lds_sync();

    float pool[4] = {0.f, 0.f, 0.f, 0.f};
    conv1_tile(-2, 0);  // prologue: ring rows 0..3 = times -2..1 (rows 4..15 are rewritten by pair 0)
#pragma unroll 1
    for (int p = 0; p < NP; ++p) {
      wave_lds_sync();
      conv1_tile(32 * p + 2, 4);
      conv1_tile(32 * p + 18, 20);
      wave_lds_sync();
      // conv2: out^T[co][t] = W2[co][(k,ci)] x h1col[(k,ci)][t]; lane (n, h) of fragment s holds tap 2s + (h >> 1),
      // channels 8(h & 1) .. +7 of time t + tap - 2 = ring row 16u + n + tap; tap 5 is the bias row
      f32x4 accs[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        bf16x8 Bh[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int r = 16 * u + c + 2 * s + (h >> 1);
          if (s == 2 && h >= 2)
            Bh[s] = Bone;
          else
            Bh[s] = *reinterpret_cast<const bf16x8*>(ring + r * C + 8 * (h & 1));
        }
        accs[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 3; ++s) accs[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Wf[s], Bh[s], accs[u], 0, 0, 0);
      }
      // accs[u][i] = conv2(h1)[t = 32p + 16u + n][co = 4h + i] + b2[co]; only the pair that straddles L masks
      if (32 * p + 32 <= L) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) pool[q] += fmaxf(accs[u][q], 0.f);
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool tv = 32 * p + 16 * u + c < L;
#pragma unroll
          for (int q = 0; q < 4; ++q) pool[q] += tv ? fmaxf(accs[u][q], 0.f) : 0.f;
        }
      }
      wave_lds_sync();
      if (lane < 8) {  // carry rows 32..35 (times 32p + 30 .. 32p + 33) to rows 0..3 of the next pair
        const int o = (lane >> 1) * C + 8 * (lane & 1);
        *reinterpret_cast<bf16x8*>(ring + o) = *reinterpret_cast<const bf16x8*>(ring + 32 * C + o);
      }
    }

    // head: pooled[co = 4h' + q] sits in lane 16h' + 15 after the row sums
#pragma unroll
    for (int q = 0; q < 4; ++q) pool[q] = row16_sum(pool[q]);
    const float inv_L = 1.0f / (float)L;
    float logit = bh;
#pragma unroll
    for (int hh = 0; hh < 4; ++hh)
#pragma unroll
      for (int q = 0; q < 4; ++q) logit = fmaf(wh[4 * hh + q], lane_bcast(pool[q], 16 * hh + 15) * inv_L, logit);
    // argmax (ties to the lowest index) and the row maximum in one scalar pass
    float m = lane_bcast(logit, 0);
    int best = 0;
    for (int n = 1; n < nc; ++n) {
      const float v = lane_bcast(logit, n);
      if (v > m) {
        m = v;
        best = n;
      }
    }
    if (logits && lane < nc) logits[(long)i * nc + lane] = logit;
    if (pred && lane == 0) pred[i] = best;
    if (Y) {
      const float e = c < nc ? expf(logit - m) : 0.f;
      float ssum = 0.f;
      for (int n = 0; n < nc; ++n) ssum += lane_bcast(e, n);
      const int yc = min(max(y, 0), nc - 1);  // (labels are validated by the caller; keeps the lane read in range)
      const float loss = logf(ssum) - (lane_bcast(logit, yc) - m);
      loss_acc += (double)loss;
      cnt += 1u;
      corr += best == y ? 1u : 0u;
      const int ce = y * nc + best;
#pragma unroll
      for (int j = 0; j < 4; ++j) conf[j] += (lane == (ce >> 2) && j == (ce & 3)) ? 1u : 0u;
    }
    i = inext;
  }

  if (Y) {
    if (lane == 0) {
      // write-through (sc1) store; the finalize launch reads it after the kernel boundary
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(partials + gw),
                         __builtin_bit_cast(unsigned long long, loss_acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cnt) atomicAdd(out + 1, (unsigned long long)cnt);
      if (corr) atomicAdd(out + 2, (unsigned long long)corr);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ce = 4 * lane + j;
      if (ce < nc * nc && conf[j]) atomicAdd(out + 3 + ce, (unsigned long long)conf[j]);
    }
  }
}

// One block: loss_sum = the G wave partials summed in a fixed order (thread t: t, t + 256, ...; then thread 0 over
// the 256 thread sums), independent of how the evaluation launch was scheduled.
__global__ __launch_bounds__(FIN_NT) void tiny_eval_finalize_kernel(const double* __restrict__ partials, int G,
                                                                    double* __restrict__ loss_sum) {
  __shared__ double part[FIN_NT];
  double s = 0.0;
  for (int g = threadIdx.x; g < G; g += FIN_NT) s += partials[g];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int j = 0; j < FIN_NT; ++j) t += part[j];
    *loss_sum = t;
  }
}

int out_bytes(int nc) { return 8 * (3 + nc * nc); }

int check_eval_args(int L, long ldx, int N, int nc) {
  if (L < 8 || N <= 0 || nc < 1 || nc > MAX_CLASSES || ldx < L) return ecg::kBadArg;
  if (round_lp(L) > 32 * 4 * 8) return ecg::kTooLarge;  // the training step's limit (check_step_args)
  return ecg::kOk;
}

template <bool VEC>
int launch_eval(const float* X, int L, long ldx, const int* idx, const int* Y, int N, const float* params, int nc,
                const unsigned char* wprep, double* partials, unsigned long long* out, int* pred, float* logits,
                int max_workgroups, int* waves_out, hipStream_t stream) {
  auto kern = tiny_ecg_eval_kernel<VEC>;
  const int lds = EW * wave_lds_bytes(round_lp(L));  // <= 21 KB
  int dev = 0, cus = 0, resident = 0;
  ECG_HIP_CHECK(hipGetDevice(&dev));
  ECG_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  ECG_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kern, EW * 64, lds));
  // persistent grid: what the device holds at once, never more workgroups than windows / EW or partial slots;
  // no workgroup waits for another, so a grid the device cannot hold at once is only slower, never wrong
  long grid = (long)(cus > 0 ? cus : 1) * (resident > 0 ? resident : 1);
  if (grid > (N + EW - 1) / EW) grid = (N + EW - 1) / EW;
  if (grid > kMaxEvalWaves / EW) grid = kMaxEvalWaves / EW;
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(EW * 64), lds, stream, X, L, ldx, idx, Y, N, params, nc, wprep,
                     partials, out, pred, logits);
  ECG_HIP_CHECK(hipGetLastError());
  *waves_out = (int)grid * EW;
  return ecg::kOk;
}

}  // namespace

// ---------------------------------------------------------------------------- C ABI
// Bytes of the loss-partial scratch and of the output record of ecg_tiny_eval.
ECG_API int ecg_tiny_eval_scratch_bytes(int nc) {
  (void)nc;
  return kMaxEvalWaves * (int)sizeof(double);
}
ECG_API int ecg_tiny_eval_out_bytes(int nc) { return (nc < 1 || nc > MAX_CLASSES) ? 0 : out_bytes(nc); }

// Evaluate TinyECG (bf16 MFMA operands, fp32 accumulation) on the N windows X[idx[i]] (X[i] when idx is null).
//   Y      int32 labels by row of X; null: inference only (``out`` / ``scratch`` are not touched)
//   wprep  ecg_tiny_wprep_bytes() of 16-byte aligned device memory owned by the caller: the prepared-fragment
//          image, rebuilt here from ``params`` on every call
//   out    ecg_tiny_eval_out_bytes(nc): {double loss_sum; int64 count, correct, conf[true][pred]}, overwritten
//   pred   [N] int32 argmax (ties to the lowest class) / logits [N][nc] fp32: optional, null skips them
//   max_workgroups  <= 0: the grid is sized from the device (CUs x resident workgroups); > 0 caps it.  A test knob
//          (like ecg_tiny_force_waves): counts and predictions never depend on it, loss_sum only in its fp64
//          summation order.
// Enqueues a prep launch, a memset of ``out``, the evaluation and a one-block finalize launch on ``stream``;
// never synchronises, so it can be stream-captured.
ECG_API int ecg_tiny_eval(const float* X, int L, long ldx, const int* idx, const int* Y, int N,
                          const float* params, int nc, void* wprep, void* scratch, void* out, int* pred,
                          float* logits, int max_workgroups, hipStream_t stream) {
  if (!X || !params || !wprep || reinterpret_cast<uintptr_t>(wprep) % 16) return ecg::kBadArg;
  int st = check_eval_args(L, ldx, N, nc);
  if (st) return st;
  if (Y ? (!scratch || !out) : (!pred && !logits)) return ecg::kBadArg;
  st = ecg_tiny_prep(params, wprep, stream);
  if (st) return st;
  if (Y) ECG_HIP_CHECK(hipMemsetAsync(out, 0, out_bytes(nc), stream));
  // 16-byte rows: the predicate of the training round's gather (GatherArgs::vec)
  const bool vec = L % 4 == 0 && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0;
  const unsigned char* wp = static_cast<const unsigned char*>(wprep);
  double* partials = static_cast<double*>(scratch);
  unsigned long long* o = static_cast<unsigned long long*>(out);
  int waves = 0;
  st = vec ? launch_eval<true>(X, L, ldx, idx, Y, N, params, nc, wp, partials, o, pred, logits, max_workgroups,
                               &waves, stream)
           : launch_eval<false>(X, L, ldx, idx, Y, N, params, nc, wp, partials, o, pred, logits, max_workgroups,
                                &waves, stream);
  if (st) return st;
  if (Y) {
    hipLaunchKernelGGL(tiny_eval_finalize_kernel, dim3(1), dim3(FIN_NT), 0, stream, partials, waves,
                       static_cast<double*>(out));
    ECG_HIP_CHECK(hipGetLastError());
  }
  return ecg::kOk;
}
