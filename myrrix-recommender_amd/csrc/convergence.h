// convergence.h -- AlternatingLeastSquares.iterateXFromY's outer loop (ALS:196-256), stated once for one handle
// (mals_factorize, mals_api.hip) and for a group (mals_group_factorize, mals_group.cpp): the estimate table of the convergence
// sample, DoubleWeightedMean, the iteration report and the three stop rules.  Host code only;
// tests/cpp/test_group_host.cpp drives the loop with a scripted driver and no device.
#pragma once
#include "../../include/myrrix_als.h"

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace mals {

// DoubleWeightedMean.increment (common/src/net/myrrix/common/stats/DoubleWeightedMean.java:73-81)
inline void dwm_increment(double& total_weight, double& mean, double datum, double weight) {
  const double old = total_weight;
  total_weight += weight;
  if (old <= 0) {
    mean = datum;
  } else {
    mean = mean * old / total_weight + datum * weight / total_weight;
  }
}

// ALS:231-238: the table takes the fresh estimates; returns the mean of |fresh - previous| weighted by max(fresh, 0), in
// table order (the mean depends on it).  NaN for an empty sample.
inline double update_estimates(std::vector<double>& est, const std::vector<double>& fresh) {
  double tw = 0.0, mean = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < est.size(); ++i) {
    const double nv = fresh[i], ov = est[i];
    est[i] = nv;
    dwm_increment(tw, mean, std::fabs(nv - ov), nv > 0.0 ? nv : 0.0);
  }
  return mean;
}

inline bool should_stop(int iteration, double mean, double convergence_threshold, int max_iterations, bool random_y) {
  if (max_iterations > 0 && iteration >= max_iterations) return true;       // ALS:242-245
  if (!std::isfinite(mean)) return true;                                    // ALS:248-251
  return !(random_y && iteration == 1) && mean < convergence_threshold;     // ALS:253-256
}

// The loop over what differs between one handle and a group.  Driver:
//   int fail(int code, const char* msg)          the failure text goes where the caller's last_error reads it
//   void clear_cancel()
//   int cancelled()                              MALS_OK or the status that ends the run (a group agrees on it over its ranks)
//   int half_iteration(int side)
//   int sample_dots(users, n_users, items, n_items, double* out)      out: n_users x n_items, from complete factors
//   mals_iteration_fn callback(void** user)      read ONCE per iteration: one installed while an iteration runs starts with
//                                                the next one
//   void count(int point)                        the report's counters are read: 0 = the iteration starts, 1 = X is solved
//   void report(mals_iteration_info* info)       x_rows, y_rows, entries_gathered, algorithmic_bytes, devices of this iteration
template <class Driver>
int factorize_loop(Driver& d, double convergence_threshold, int32_t max_iterations, int32_t random_y, int32_t iterate,
                   const int64_t* test_users, int32_t n_test_users, const int64_t* test_items, int32_t n_test_items,
                   int32_t* iterations_out, double* convergence_out) {
  if (iterations_out) *iterations_out = 0;
  if (convergence_out) *convergence_out = std::numeric_limits<double>::quiet_NaN();
  if (!(convergence_threshold > 0.0 && convergence_threshold < 1.0)) return d.fail(MALS_INVALID_ARG, "threshold must be in (0,1)");  // ALS:140-141
  if (n_test_users < 0 || n_test_items < 0 || (n_test_users > 0 && !test_users) || (n_test_items > 0 && !test_items))
    return d.fail(MALS_INVALID_ARG, "bad convergence sample");
  d.clear_cancel();
  if (!iterate) return d.half_iteration(MALS_SIDE_X);  // ALS:196-204
  std::vector<double> est((size_t)n_test_users * (size_t)n_test_items, 0.0);  // ALS:215: X empty => 0
  std::vector<double> fresh(est.size());
  for (int it = 1;; ++it) {
    const auto t_it = std::chrono::steady_clock::now();
    void* iter_user = nullptr;
    const mals_iteration_fn iter_fn = d.callback(&iter_user);
    if (iter_fn) d.count(0);
    if (int rc = d.cancelled()) return rc;
    if (int rc = d.half_iteration(MALS_SIDE_X)) return rc;  // ALS:228
    if (iter_fn) d.count(1);
    if (int rc = d.cancelled()) return rc;
    if (int rc = d.half_iteration(MALS_SIDE_Y)) return rc;  // ALS:229
    // the sample dots on the device (ALS:234), the order-dependent running mean on the host (ALS:237)
    if (int rc = d.sample_dots(test_users, n_test_users, test_items, n_test_items, fresh.data())) return rc;
    const double mean = update_estimates(est, fresh);
    if (iterations_out) *iterations_out = it;
    if (convergence_out) *convergence_out = mean;
    if (iter_fn) {   // what the reference logs per iteration (ALS:241-246, 351-358)
      mals_iteration_info info;
      std::memset(&info, 0, sizeof(info));
      info.struct_size = (int32_t)sizeof(info);
      info.iteration = it;
      info.avg_abs_difference = mean;
      info.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_it).count();
      d.report(&info);
      iter_fn(iter_user, &info);
    }
    if (should_stop(it, mean, convergence_threshold, max_iterations, random_y != 0)) return MALS_OK;
  }
}

}  // namespace mals
