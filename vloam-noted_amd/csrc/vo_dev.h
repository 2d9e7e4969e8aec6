// vo_dev.h — the visual-odometry solve on records that are already in device memory (vo.hip).
#pragma once
#include "common.h"

namespace loam {

constexpr int VO_MAX_ITERATIONS = 255;  // the kernel's pass budget less the first evaluation

// k_vo_solve on stream st: problem p (one workgroup) = records d_off[p * off_stride] ..
// d_off[p * off_stride + 1] of d_records (10 doubles each, loam_vo_solve's layout); d_x:
// n_problems x 6 in/out; d_stats: n_problems.  Enqueues only, never waits.
int32_t vo_solve_launch(const double* d_records, const int* d_off, int off_stride, double* d_x, int max_iterations,
                        loam_lm_stats* d_stats, int n_problems, hipStream_t st);

}  // namespace loam
