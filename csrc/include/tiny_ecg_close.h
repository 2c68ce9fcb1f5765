// The close of a cohort round with a server step, as kernels/tiny_ecg_step.hip's round calls it and
// kernels/tiny_ecg_close.hip defines it.
#pragma once
#include "ecg_common.h"

namespace ecg {
namespace tiny {

// One close: M clients' weights ``params`` at the cohort stride, the round's starting weights ``global`` [P], the clip
// norm (0: none), the noise multiplier of this rank's share, the server step size (0 means 1), the Philox key and the
// device round word, the [M] clip factors and delta norms it reports, and the server optimizer (0 none, 1 sgdm, 2
// adagrad, 3 adam, 4 yogi) with its state m / v [P].  ``delta`` (nullable) [P]: the split close - the averaged, clipped,
// noised delta goes there, ``global`` is only read, and opt, m and v are not read at all.
struct CohortClose {
  const float* params;
  float* global;
  int P, M;
  float clip, sigma, server_lr;
  unsigned long long seed;
  unsigned long long* round_word;
  float* scale;
  float* norm;
  int opt;
  float beta1, beta2, tau;
  float* m;
  float* v;
  float* delta;
  // (nullable) [M] fp32 on the device: Delta = sum_c weight[c] * d_c in place of the mean (cohort_delta_wscale_kernel
  // folds it into scale[], and inv_M is 1); not with a clip norm
  const float* weight;
  // A robust close (0: none): the coordinate-wise mean of the M - 2 trim middle values of the clients' deltas, 1 <= trim,
  // 2 trim < M <= 64, with no clip, noise or weight.  Delta goes to ``delta`` or, when the close is not split, to
  // ``robust_scratch`` [P], from which server_step_kernel takes the step.
  int trim;
  float* robust_scratch;
};

// kOk, or kBadArg for a close that cohort_close must not be given.
int check_cohort_close(const CohortClose& c);

// The two launches of a checked close: cohort_delta_scale_kernel (``weight`` set: cohort_delta_wscale_kernel), then cohort_delta_kernel (``delta`` set),
// cohort_server_opt_kernel<opt> (opt != 0) or cohort_dp_mean_kernel.  With ``trim`` set there are three: the first as
// above, cohort_robust_delta_kernel and, unless ``delta`` is set, server_step_kernel<opt>.
int cohort_close(const CohortClose& c, hipStream_t stream);

}  // namespace tiny
}  // namespace ecg
