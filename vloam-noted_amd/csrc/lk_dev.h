// lk_dev.h — pyramidal Lucas-Kanade tracking on images that are already in device memory (lk.hip).
#pragma once
#include "common.h"

namespace loam {

constexpr int LK_MAX_LEVELS = 8;  // max_level <= 7
constexpr int LK_MAX_WIN = 31;

// one frame pair of a launch
struct LkPair {
  int active;  // 0: the pair is skipped
  int w, h;    // level 0
  int levels;  // lk_levels(w, h, ...)
  int n;       // points
};

// the pyramids of a handle: [pair][image 0 prev / 1 curr][level], every level dense (row stride =
// its own width) at a fixed offset that the largest image decides; plus the tracker's constants
struct LkPlan {
  int win, max_level, max_count;
  int max_w, max_h;
  double eps2;     // epsilon clamped to [0, 10], squared in double
  double min_eig;  // compared with (double)minEig
  size_t lvl_off[LK_MAX_LEVELS];
  size_t image_bytes;  // one pyramid
};

// levels a w x h image gets: buildOpticalFlowPyramid stops before a level that is no larger than
// the window
inline int lk_levels(int w, int h, int win, int max_level) {
  int n = 1;
  while (n <= max_level) {
    w = (w + 1) / 2;
    h = (h + 1) / 2;
    if (w <= win || h <= win) break;
    ++n;
  }
  return n;
}

// checks the parameters (LOAM_ERR_ARG) and lays the pyramids out
int32_t lk_plan(const loam_lk_params* p, LkPlan* out);

// pyramids of every active pair (level 0 of both images is in place), then the tracks of its n
// points: d_kp0 -> d_kp1, d_status, d_err ([pair][K]).  Enqueues only, never waits.
int32_t lk_launch(const LkPlan& plan, const LkPair* d_pairs, const LkPair* pairs, int n_pairs, uint8_t* d_pyr,
                  const float2* d_kp0, float2* d_kp1, uint8_t* d_status, float* d_err, int K, hipStream_t st);

}  // namespace loam
