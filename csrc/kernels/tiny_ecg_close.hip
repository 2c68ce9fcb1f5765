// The close of a TinyECG cohort round with a server step, and the server step on its own, for gfx950.
//
// A cohort round (kernels/tiny_ecg_step.hip) ends on the plain mean of its clients' weights or on one of the closes
// here, which work on the clients' round deltas: with g the round's starting weights (what the fan-out read:
// ``global_params`` is untouched until the close), d_c = p_c - g, n_c = |d_c|_2 and s_c = min(1, C / n_c) (n_c == 0 -> 1),
//   Delta_i = (((s_0 d_0[i] + s_1 d_1[i]) + ...) + s_{M-1} d_{M-1}[i]) * inv_M + nu * z_i,
// clients in ascending order in fp32, every multiply-add fused, nu = sigma * C / M rounded once on the host (nu == 0:
// nothing is drawn).  A close is two launches - cohort_delta_scale_kernel (the clip factors, which need every client's
// whole delta before any parameter can be written: one launch would need a grid-wide barrier for nothing), then one of
//   cohort_dp_mean_kernel      g_new = g + eta * Delta                              (client-level DP, DP-FedAvg)
//   cohort_server_opt_kernel   a server optimizer's step on Delta                   (FedAvgM, FedAdagrad, FedAdam, FedYogi)
//   cohort_delta_kernel        delta = Delta, g left alone                          (the split close)
// - chosen by cohort_close.  All three form Delta_i with cohort_noise and cohort_delta below, so their bits agree.
//
// A robust close (CohortClose::trim k > 0: the coordinate-wise trimmed mean, the median at k = (M - 1) / 2; Yin et al.,
// "Byzantine-Robust Distributed Learning") is not a linear combination of the deltas and takes three launches:
// cohort_delta_scale_kernel without a clip (the norms and the round word keep their meaning), then
//   cohort_robust_delta_kernel  delta = the mean of the M - 2k middle values of d_c[i]  (into the split close's buffer
//                                                                                        or a [P] scratch)
// and, unless the close is split, server_step_kernel on (g, scratch) - the kernel the split close's second half runs,
// so the two ways end on the same bits by construction.
//
// The split close exists because a driver of several ranks that wants ONE server optimizer over all their clients must
// average the deltas first (the adaptive rules are nonlinear in Delta): cohort_delta_kernel ends the round with Delta
// in a buffer of its own, the caller all-reduces that buffer, and server_step_kernel (ecg_server_opt_step) takes the
// step every rank then takes alike.  Run back to back on one rank the pair leaves the bits of the fused close.
#include "../include/ecg_common.h"
#include "../include/tiny_ecg.h"
#include "../include/tiny_ecg_close.h"

#include <cfloat>
#include <climits>
#include <cstdint>

namespace {

using namespace ecg::tiny;

// z_i: dp_normal's generator (kernels/tiny_ecg_step.hip) on its own stream - the last counter word is 1 where
// dp_normal has 0, so the counters of the two noise streams never coincide, whatever the seeds and step / round
// numbers.  r is the 64-bit round counter.
__device__ inline float cohort_dp_normal(int i, unsigned long long seed, unsigned long long r) {
  uint32_t c[4] = {(uint32_t)i, (uint32_t)r, (uint32_t)(r >> 32), 1u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u1 = (float)((c[0] >> 8) + 1u) * 0x1p-24f, u2 = (float)(c[1] >> 8) * 0x1p-24f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// Diagnostic: z[i] for i < P of round r (the values the closes add, without the nu factor).
template <int NT>
__global__ __launch_bounds__(NT) void cohort_dp_noise_kernel(float* __restrict__ z, int P, unsigned long long seed,
                                                             unsigned long long r) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i < P) z[i] = cohort_dp_normal(i, seed, r);
}

// Clip factors of a cohort: one wave per client, scale[c] = s_c and norm[c] = n_c (reported, not read by the close).
// Fixed summation order (per lane in column order, then a butterfly over the wave), no atomics.  Exactly P floats of a
// client are read: the pstride - P padding floats are never written.  Thread 0 of block 0 advances the round counter
// (dp_row_scale_kernel's pattern: its only writer; its only reader is the kernel launched next, which therefore draws
// round ``round_word[0] - 1``), so a replayed graph draws fresh noise.
constexpr int CDP_CLIENTS_PER_BLOCK = 4;
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void cohort_delta_scale_kernel(
    const float* __restrict__ params, const float* __restrict__ global_params, int P, int M, float clip,
    float* __restrict__ scale, float* __restrict__ norm, unsigned long long* __restrict__ round_word) {
  if (blockIdx.x == 0 && threadIdx.x == 0) round_word[0] = round_word[0] + 1ull;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (c >= M) return;  // wave-uniform
  const float* p = params + (long)c * cohort_pstride(P);
  float ss = 0.f;
  for (int i = lane; i < P; i += 64) {
    const float d = p[i] - global_params[i];
    ss += d * d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) {
    const float n = sqrtf(ss);
    norm[c] = n;
    scale[c] = n > 0.f ? fminf(1.f, clip / n) : 1.f;
  }
}

// cohort_delta_scale_kernel's sibling for a weighted close: norms, clip factor and the advance of the round word are
// its lines; the one difference is scale[c] = s_c * weight[c] (``weight`` [M] fp32 on the device: a cohort's weights
// change per round, and kernel arguments are baked into a captured graph).  The kernels below then form
// Delta_i = sum_c (s_c w_c) d_c[i] with inv_M = 1.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void cohort_delta_wscale_kernel(
    const float* __restrict__ params, const float* __restrict__ global_params, int P, int M, float clip,
    float* __restrict__ scale, float* __restrict__ norm, unsigned long long* __restrict__ round_word,
    const float* __restrict__ weight) {
  if (blockIdx.x == 0 && threadIdx.x == 0) round_word[0] = round_word[0] + 1ull;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (c >= M) return;  // wave-uniform
  const float* p = params + (long)c * cohort_pstride(P);
  float ss = 0.f;
  for (int i = lane; i < P; i += 64) {
    const float d = p[i] - global_params[i];
    ss += d * d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) {
    const float n = sqrtf(ss);
    norm[c] = n;
    scale[c] = (n > 0.f ? fminf(1.f, clip / n) : 1.f) * weight[c];
  }
}

// Delta_i in two parts, shared by the three kernels below (one thread per parameter): the noise nu * z_i, drawn first,
// under the latency of the loads that follow, and the clipped mean plus that noise.  Each kernel loads g - and its
// server state - between the two: that order is the kernels' schedule.
__device__ __forceinline__ float cohort_noise(int i, float noise_scale, unsigned long long seed,
                                              const unsigned long long* round_word) {
  float noise = 0.f;
  if (noise_scale != 0.f) noise = noise_scale * cohort_dp_normal(i, seed, round_word[0] - 1ull);
  return noise;
}
__device__ __forceinline__ float cohort_delta(const float* params, const float* scale, int i, int P, int M, float inv_M,
                                              float g, float noise) {
  const int pstride = cohort_pstride(P);
  float s = scale[0] * (params[i] - g);
  for (int c = 1; c < M; ++c) s = __builtin_fmaf(scale[c], params[(long)c * pstride + i] - g, s);
  return __builtin_fmaf(s, inv_M, noise);
}

template <int NT>
__global__ __launch_bounds__(NT) void cohort_dp_mean_kernel(
    const float* __restrict__ params, float* __restrict__ global_params, int P, int M, float inv_M,
    const float* __restrict__ scale, float server_lr, float noise_scale, unsigned long long seed,
    const unsigned long long* __restrict__ round_word) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= P) return;
  const float noise = cohort_noise(i, noise_scale, seed, round_word);
  const float g = global_params[i];
  global_params[i] = __builtin_fmaf(server_lr, cohort_delta(params, scale, i, P, M, inv_M, g, noise), g);
}

// A server optimizer (Reddi et al., "Adaptive Federated Optimization") on Delta, with the server state m, v [P] (fp32,
// kept across rounds; no bias correction, as in the paper) and one_minus = 1 - beta in fp32:
//   OPT 1 sgdm (FedAvgM):  m = b1 m + Delta;               g += eta m
//   OPT 2 adagrad:         m = b1 m + (1 - b1) Delta;      v = v + Delta^2
//   OPT 3 adam:            m as adagrad;                   v = b2 v + (1 - b2) Delta^2
//   OPT 4 yogi:            m as adagrad;                   v = v - (1 - b2) Delta^2 sign(v - Delta^2), sign(0) = 0
//   OPT 2..4:              g += eta m / (sqrt(v) + tau)    (the new m and v; division and sqrt correctly rounded)
// One thread per parameter reads g[i], m[i], v[i] and the M client values and writes g[i], m[i] and (OPT 2..4) v[i]:
// no atomics, a fixed order.  sgdm takes v == nullptr.  With b1 == 0 and m == 0 sgdm is cohort_dp_mean_kernel's result
// bit for bit (m = Delta, g + eta * Delta): sgdm's two multiply-adds are written out fused, because left to the
// compiler b1 * m0 and s * inv_M pair up in one packed multiply, which rounds Delta once more.
constexpr int SOPT_SGDM = 1, SOPT_ADAGRAD = 2, SOPT_ADAM = 3, SOPT_YOGI = 4;

template <int NT, int OPT>
__global__ __launch_bounds__(NT) void cohort_server_opt_kernel(
    const float* __restrict__ params, float* __restrict__ global_params, int P, int M, float inv_M,
    const float* __restrict__ scale, float server_lr, float noise_scale, unsigned long long seed,
    const unsigned long long* __restrict__ round_word, float b1, float b2, float tau, float* __restrict__ m,
    float* __restrict__ v) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= P) return;
  const float noise = cohort_noise(i, noise_scale, seed, round_word);
  const float g = global_params[i];
  const float m0 = m[i];
  float v1 = 0.f;
  if (OPT != SOPT_SGDM) v1 = v[i];
  const float delta = cohort_delta(params, scale, i, P, M, inv_M, g, noise);
  float m1;
  if (OPT == SOPT_SGDM) {
    m1 = __builtin_fmaf(b1, m0, delta);
    global_params[i] = __builtin_fmaf(server_lr, m1, g);
  } else {
    m1 = b1 * m0 + (1.f - b1) * delta;
    const float d2 = delta * delta;
    if (OPT == SOPT_ADAGRAD) {
      v1 = v1 + d2;
    } else if (OPT == SOPT_ADAM) {
      v1 = b2 * v1 + (1.f - b2) * d2;
    } else {
      const float e = v1 - d2;
      const float sg = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
      v1 = v1 - (1.f - b2) * d2 * sg;
    }
    v[i] = v1;
    global_params[i] = g + (server_lr * m1) / (sqrtf(v1) + tau);
  }
  m[i] = m1;
}

// delta[i] = Delta_i; nothing else is written, and exactly P floats of a client are read.
template <int NT>
__global__ __launch_bounds__(NT) void cohort_delta_kernel(
    const float* __restrict__ params, const float* __restrict__ global_params, int P, int M, float inv_M,
    const float* __restrict__ scale, float noise_scale, unsigned long long seed,
    const unsigned long long* __restrict__ round_word, float* __restrict__ delta) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= P) return;
  const float noise = cohort_noise(i, noise_scale, seed, round_word);
  const float g = global_params[i];
  delta[i] = cohort_delta(params, scale, i, P, M, inv_M, g, noise);
}

// One server step on a flat vector of n floats: OPT 0 the plain step g = fma(eta, delta, g) (m and v not touched), OPT
// 1..4 cohort_server_opt_kernel's rules from Delta on.  Every rounding is pinned - contraction is off in the body and
// the fused multiply-adds are written out - to what cohort_dp_mean_kernel and cohort_server_opt_kernel compile to, so
// that the split close ends on their bits: sgdm's two fused multiply-adds, adagrad's v = fma(Delta, Delta, v), yogi's
// sign taken of fma(-Delta, Delta, v), every other product and sum rounded on its own.  Division and sqrtf are
// correctly rounded; one thread per element, no atomics.
template <int NT, int OPT>
__global__ __launch_bounds__(NT) void server_step_kernel(float* __restrict__ g, const float* __restrict__ delta, long n,
                                                         float eta, float b1, float b2, float tau,
                                                         float* __restrict__ m, float* __restrict__ v) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float d = delta[i], g0 = g[i];
  if (OPT == 0) {
    g[i] = __builtin_fmaf(eta, d, g0);
    return;
  }
  const float m0 = m[i];
  float m1;
  if (OPT == SOPT_SGDM) {
    m1 = __builtin_fmaf(b1, m0, d);
    g[i] = __builtin_fmaf(eta, m1, g0);
  } else {
    float v1 = v[i];
    m1 = b1 * m0 + (1.f - b1) * d;
    if (OPT == SOPT_ADAGRAD) {
      v1 = __builtin_fmaf(d, d, v1);
    } else if (OPT == SOPT_ADAM) {
      v1 = b2 * v1 + (1.f - b2) * (d * d);
    } else {
      const float e = __builtin_fmaf(-d, d, v1);
      const float sg = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
      v1 = v1 - ((1.f - b2) * (d * d)) * sg;
    }
    v[i] = v1;
    g[i] = g0 + (eta * m1) / (sqrtf(v1) + tau);
  }
  m[i] = m1;
}

// The coordinate-wise trimmed mean of the clients' deltas: with x_c = p_c[i] - g[i] in fp32 (no factor, no weight, no
// noise), the M values of parameter i are ordered by a 32-bit key - NaN of either sign 0xFFFFFFFF, else the bit
// pattern with the sign bit flipped (non-negative) or all bits flipped (negative): -inf < ... < -0 < +0 < ... < +inf <
// NaN - ties by client index, so rank_c = #{j : key_j < key_c or (key_j == key_c and j < c)} is a permutation; client c
// is kept when trim <= rank_c < M - trim, and
//   delta[i] = (((x_c1 + x_c2) + ...) + x_cn) * inv_n,    n = M - 2 trim, inv_n = fp32(1 / n),
// the kept clients in ascending client order, every sum and the product rounded on its own.  The sum starts from -0,
// the one value with -0 + x == x bit for bit for every x, and takes its terms by a select: no mask is multiplied in.
//
// Lanes of a wave are cut into segments of W = 1 << logw >= M lanes (W <= 64); lane (q, c) of a segment holds client
// c's value of parameter i0 + q, so a wave serves 64 >> logw parameters.  The rank is a loop over j < M that reads lane
// base + j's key (ds_bpermute); which lanes are kept goes round in one ballot, and the sum is a second loop over j < M
// that every lane of the segment takes alike, which fixes the order without a reduction tree.  Lanes with c >= M and
// segments with i >= P load nothing and are read by no live lane (they run the loops, since a cross-lane read needs
// its source lanes active); lane c == 0 stores.  No LDS, no barrier, no atomics; exactly P floats of a client are read.
// This file is compiled with -fno-honor-nans -fno-signed-zeros, and here both matter (a NaN client has to sort last, a
// kept -0 has to stay -0): the body runs under float_control(precise), the NaN test is an integer compare, and a
// client that is not kept enters the sum as -0 chosen by an integer select - nothing is left for those flags to fold.
template <int NT>
__global__ __launch_bounds__(NT) void cohort_robust_delta_kernel(
    const float* __restrict__ params, const float* __restrict__ global_params, int P, int M, int logw, int trim,
    float inv_n, float* __restrict__ delta) {
#pragma float_control(precise, on)
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const int i0 = wave << (6 - logw);
  if (i0 >= P) return;  // wave-uniform
  const int c = lane & ((1 << logw) - 1), base = lane - c;
  const int i = i0 + (lane >> logw);
  const bool live = c < M && i < P;
  float x = 0.f;
  uint32_t key = 0u;
  if (live) {
    x = params[(long)c * cohort_pstride(P) + i] - global_params[i];
    const uint32_t b = __float_as_uint(x);
    key = (b & 0x7FFFFFFFu) > 0x7F800000u ? 0xFFFFFFFFu : ((b & 0x80000000u) ? ~b : (b ^ 0x80000000u));
  }
  int rank = 0;
  for (int j = 0; j < M; ++j) {
    const uint32_t kj = (uint32_t)__shfl((int)key, base + j, 64);
    rank += (kj < key || (kj == key && j < c)) ? 1 : 0;
  }
  const unsigned long long kept = __ballot(live && rank >= trim && rank < M - trim);
  float s = -0.f;
  for (int j = 0; j < M; ++j) {
    const uint32_t xj = (uint32_t)__shfl((int)__float_as_uint(x), base + j, 64);
    s = s + __uint_as_float(((kept >> (base + j)) & 1ull) ? xj : 0x80000000u);
  }
  if (live && c == 0) delta[i] = s * inv_n;
}

// server_step_kernel<256, opt> on ``n`` floats (opt 0..4, checked by the caller; ``step`` is the step size itself).
void launch_server_step(float* g, const float* delta, long n, int opt, float step, float b1, float b2, float tau,
                        float* m, float* v, hipStream_t stream) {
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define ECG_SERVER_STEP_LAUNCH(OPT) \
  hipLaunchKernelGGL((server_step_kernel<256, OPT>), grid, block, 0, stream, g, delta, n, step, b1, b2, tau, m, v)
  switch (opt) {
    case 0: ECG_SERVER_STEP_LAUNCH(0); break;
    case SOPT_SGDM: ECG_SERVER_STEP_LAUNCH(SOPT_SGDM); break;
    case SOPT_ADAGRAD: ECG_SERVER_STEP_LAUNCH(SOPT_ADAGRAD); break;
    case SOPT_ADAM: ECG_SERVER_STEP_LAUNCH(SOPT_ADAM); break;
    default: ECG_SERVER_STEP_LAUNCH(SOPT_YOGI); break;
  }
#undef ECG_SERVER_STEP_LAUNCH
}

int check_server_opt(int opt, float b1, float b2, float tau, const float* m, const float* v) {
  if (opt < SOPT_SGDM || opt > SOPT_YOGI || !m) return ecg::kBadArg;
  if (!(b1 >= 0.f && b1 < 1.f) || !(b2 >= 0.f && b2 < 1.f)) return ecg::kBadArg;
  if (opt != SOPT_SGDM && (!v || !(tau > 0.f))) return ecg::kBadArg;
  return ecg::kOk;
}

}  // namespace

int ecg::tiny::check_cohort_close(const CohortClose& c) {
  if (!c.params || !c.global || !c.round_word || !c.scale || !c.norm) return ecg::kBadArg;
  if (c.P < 1 || c.M < 1 || c.M > 65535) return ecg::kBadArg;  // a cohort's range (M is a grid extent of its rounds)
  if (c.clip < 0.f || c.sigma < 0.f || c.server_lr < 0.f || (c.sigma > 0.f && c.clip == 0.f)) return ecg::kBadArg;
  // the sensitivity of a weighted, clipped mean is not C / M, and no accountant here covers it
  if (c.weight && c.clip > 0.f) return ecg::kBadArg;
  // a robust close: 1 <= trim and 2 trim < M, a cohort that fits a wave, nothing that scales or perturbs a delta (the
  // sensitivity of a trimmed mean is not C / M), and somewhere to put Delta
  if (c.trim != 0 && (c.trim < 0 || 2 * c.trim >= c.M || c.M > 64 || c.clip > 0.f || c.sigma > 0.f || c.weight ||
                      (!c.robust_scratch && !c.delta)))
    return ecg::kBadArg;
  if (c.delta) return ecg::kOk;  // the split close reads neither the optimizer nor its state
  return c.opt != 0 ? check_server_opt(c.opt, c.beta1, c.beta2, c.tau, c.m, c.v) : ecg::kOk;
}

// clip == 0: no clipping (every factor is 1; the norms are still reported); server_lr == 0 means 1.  nu = sigma *
// clip / M is computed in double and rounded to fp32 here; ``sigma`` arrives as an fp32 value (the caller's sigma /
// sqrt(W), already rounded), so nu can differ by one ulp from the value a caller rounds once from doubles
// (train/cohort.py does): 2^-24 of the noise, far below the Box-Muller difference between device and host.
int ecg::tiny::cohort_close(const CohortClose& c, hipStream_t stream) {
  const float nu = (float)((double)c.sigma * (double)c.clip / (double)c.M);
  const float eta = c.server_lr == 0.f ? 1.f : c.server_lr, inv_M = c.weight ? 1.0f : 1.0f / (float)c.M;
  const float* scale = c.scale;
  const unsigned long long* word = c.round_word;
  const dim3 sgrid((c.M + CDP_CLIENTS_PER_BLOCK - 1) / CDP_CLIENTS_PER_BLOCK), sblock(CDP_CLIENTS_PER_BLOCK * 64);
  if (c.weight)  // the weights are folded into scale[]: the second kernel is the one of an unweighted close
    hipLaunchKernelGGL(cohort_delta_wscale_kernel<CDP_CLIENTS_PER_BLOCK>, sgrid, sblock, 0, stream, c.params,
                       (const float*)c.global, c.P, c.M, c.clip > 0.f ? c.clip : FLT_MAX, c.scale, c.norm, c.round_word,
                       c.weight);
  else
    hipLaunchKernelGGL(cohort_delta_scale_kernel<CDP_CLIENTS_PER_BLOCK>, sgrid, sblock, 0, stream, c.params,
                       (const float*)c.global, c.P, c.M, c.clip > 0.f ? c.clip : FLT_MAX, c.scale, c.norm,
                       c.round_word);
  ECG_HIP_CHECK(hipGetLastError());
  if (c.trim != 0) {  // the robust close: the selection, then (not split) the split close's own second half
    int logw = 0;
    while ((1 << logw) < c.M) ++logw;
    const int per_block = 4 * (64 >> logw);
    float* out = c.delta ? c.delta : c.robust_scratch;
    hipLaunchKernelGGL(cohort_robust_delta_kernel<256>, dim3((c.P + per_block - 1) / per_block), dim3(256), 0, stream,
                       c.params, (const float*)c.global, c.P, c.M, logw, c.trim, 1.0f / (float)(c.M - 2 * c.trim), out);
    ECG_HIP_CHECK(hipGetLastError());
    if (!c.delta) {
      launch_server_step(c.global, out, (long)c.P, c.opt, eta, c.beta1, c.beta2, c.tau, c.m, c.v, stream);
      ECG_HIP_CHECK(hipGetLastError());
    }
    return ecg::kOk;
  }
  const dim3 grid((c.P + 255) / 256), block(256);
#define ECG_SERVER_OPT_LAUNCH(OPT)                                                                                 \
  hipLaunchKernelGGL((cohort_server_opt_kernel<256, OPT>), grid, block, 0, stream, c.params, c.global, c.P, c.M, inv_M, \
                     scale, eta, nu, c.seed, word, c.beta1, c.beta2, c.tau, c.m, c.v)
  if (c.delta) {
    hipLaunchKernelGGL(cohort_delta_kernel<256>, grid, block, 0, stream, c.params, (const float*)c.global, c.P, c.M,
                       inv_M, scale, nu, c.seed, word, c.delta);
  } else {
    switch (c.opt) {
      case 0:
        hipLaunchKernelGGL(cohort_dp_mean_kernel<256>, grid, block, 0, stream, c.params, c.global, c.P, c.M, inv_M,
                           scale, eta, nu, c.seed, word);
        break;
      case SOPT_SGDM: ECG_SERVER_OPT_LAUNCH(SOPT_SGDM); break;
      case SOPT_ADAGRAD: ECG_SERVER_OPT_LAUNCH(SOPT_ADAGRAD); break;
      case SOPT_ADAM: ECG_SERVER_OPT_LAUNCH(SOPT_ADAM); break;
      default: ECG_SERVER_OPT_LAUNCH(SOPT_YOGI); break;
    }
  }
#undef ECG_SERVER_OPT_LAUNCH
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// ---------------------------------------------------------------------------- C ABI
// The three entry points below run only the close of a cohort round, on caller-supplied buffers: ``params`` holds M
// clients' weights at the cohort stride (ecg_tiny_cohort_param_stride(nc)), ``global`` [P] the round's starting weights
// and, afterwards, the new ones; ``scale`` / ``norm`` [M] receive the clip factors and delta norms; the noise is that
// of round ``round_word[0]`` as found, and the word is advanced by one.  ``sigma`` is the noise multiplier of this
// rank's share, as EcgTinyCohortRound's cdp_sigma.
static int close_entry(int nc, CohortClose c, hipStream_t stream) {
  if (nc < 1 || nc > MAX_CLASSES) return ecg::kBadArg;
  c.P = make_layout(nc).P;
  const int st = check_cohort_close(c);
  return st ? st : cohort_close(c, stream);
}

ECG_API int ecg_cohort_dp_close(const float* params, float* global, int nc, int M, float clip, float sigma,
                                float server_lr, unsigned long long seed, unsigned long long* round_word, float* scale,
                                float* norm, hipStream_t stream) {
  return close_entry(nc, {params, global, 0, M, clip, sigma, server_lr, seed, round_word, scale, norm, 0, 0.f, 0.f, 0.f,
                          nullptr, nullptr, nullptr}, stream);
}

// Diagnostic: z[0:P], the standard normals the closes draw for (seed, round r).
ECG_API int ecg_cohort_dp_noise(float* z, int P, unsigned long long seed, unsigned long long r, hipStream_t stream) {
  if (!z || P <= 0) return ecg::kBadArg;
  hipLaunchKernelGGL(cohort_dp_noise_kernel<256>, dim3((P + 255) / 256), dim3(256), 0, stream, z, P, seed, r);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}

// ecg_cohort_dp_close's twin with a server optimizer: ``opt`` (1 sgdm, 2 adagrad, 3 adam, 4 yogi), beta1, beta2 in
// [0, 1), tau > 0 (opt 2..4) and the server state ``m`` / ``v`` [P], read and written (``v`` may be null for sgdm).
ECG_API int ecg_cohort_server_close(const float* params, float* global, int nc, int M, float clip, float sigma,
                                    float server_lr, unsigned long long seed, unsigned long long* round_word,
                                    float* scale, float* norm, int opt, float b1, float b2, float tau, float* m,
                                    float* v, hipStream_t stream) {
  if (opt == 0) return ecg::kBadArg;  // (that is ecg_cohort_dp_close)
  return close_entry(nc, {params, global, 0, M, clip, sigma, server_lr, seed, round_word, scale, norm, opt, b1, b2, tau,
                          m, v, nullptr}, stream);
}

// ecg_cohort_dp_close's twin that stops at the delta: ``global`` [P] is only read, ``delta`` [P] receives the averaged,
// clipped, noised delta.
ECG_API int ecg_cohort_delta_close(const float* params, const float* global, int nc, int M, float clip, float sigma,
                                   unsigned long long seed, unsigned long long* round_word, float* scale, float* norm,
                                   float* delta, hipStream_t stream) {
  if (!delta) return ecg::kBadArg;
  return close_entry(nc, {params, const_cast<float*>(global), 0, M, clip, sigma, 0.f, seed, round_word, scale, norm, 0,
                          0.f, 0.f, 0.f, nullptr, nullptr, delta}, stream);
}

// The weighted close on caller-supplied buffers: Delta = sum_c weight[c] * (p_c - g) in ascending order (``weight`` [M]
// fp32, device; no clip, no noise), then the plain step (``opt`` 0), a server optimizer (1..4, as
// ecg_cohort_server_close) or, with ``delta`` non-null, the split close (``global`` is only read; opt, m, v are not).
// ``scale`` receives the weights as the second kernel reads them, ``norm`` the delta norms.
ECG_API int ecg_cohort_weighted_close(const float* params, float* global, int nc, int M, const float* weight,
                                      float server_lr, unsigned long long* round_word, float* scale, float* norm,
                                      int opt, float b1, float b2, float tau, float* m, float* v, float* delta,
                                      hipStream_t stream) {
  if (!weight) return ecg::kBadArg;
  return close_entry(nc, {params, global, 0, M, 0.f, 0.f, server_lr, 0ull, round_word, scale, norm, opt, b1, b2, tau, m,
                          v, delta, weight}, stream);
}

// ecg_cohort_weighted_close's twin for the robust close: ``trim`` k (1 <= k, 2 k < M <= 64) clients are dropped at each
// end of every parameter's order and the rest averaged (cohort_robust_delta_kernel; no clip, no weight, no noise), then
// the plain step (``opt`` 0), a server optimizer (1..4) on ``scratch`` [P], or, with ``delta`` non-null, the split
// close (``global`` is only read and ``scratch`` may be null).  ``scale`` receives ones, ``norm`` the delta norms.
ECG_API int ecg_cohort_robust_close(const float* params, float* global, int nc, int M, int trim, float server_lr,
                                    unsigned long long* round_word, float* scale, float* norm, int opt, float b1,
                                    float b2, float tau, float* m, float* v, float* delta, float* scratch,
                                    hipStream_t stream) {
  if (trim < 1) return ecg::kBadArg;  // (that is ecg_cohort_dp_close and its twins)
  return close_entry(nc, {params, global, 0, M, 0.f, 0.f, server_lr, 0ull, round_word, scale, norm, opt, b1, b2, tau, m,
                          v, delta, nullptr, trim, scratch}, stream);
}

// One server step on ``g`` [n] from ``delta`` [n] (the second half of the split close, after the caller averaged the
// ranks' deltas): ``opt`` 0 the plain step g += eta delta (m and v are not read and may be null), 1 sgdm, 2 adagrad, 3
// adam, 4 yogi with the server state ``m`` / ``v`` [n], read and written (``v`` may be null for sgdm); eta == 0 means
// 1; beta1, beta2 in [0, 1) and tau > 0 as in check_server_opt.
ECG_API int ecg_server_opt_step(float* g, const float* delta, long n, int opt, float eta, float b1, float b2, float tau,
                                float* m, float* v, hipStream_t stream) {
  if (!g || !delta || n < 1 || eta < 0.f) return ecg::kBadArg;
  if (opt != 0) {
    const int st = check_server_opt(opt, b1, b2, tau, m, v);
    if (st) return st;
  }
  if ((n + 255) / 256 > (long)INT_MAX) return ecg::kTooLarge;
  launch_server_step(g, delta, n, opt, eta == 0.f ? 1.f : eta, b1, b2, tau, m, v, stream);
  ECG_HIP_CHECK(hipGetLastError());
  return ecg::kOk;
}
