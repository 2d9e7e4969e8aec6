// vo_detect_check.cpp — one frame pair from its two images alone through
// loam_amd::VisualOdometryFrames (loam_core.hpp: enableImages / enableDetection / inputImagePair /
// tracks), compiled with plain g++ as a node would.
// Without an argument it prints the library version (the compile-and-link check).  With a file
// written by tests/test_gpu_gftt.py it runs the depth association and the VO frame and prints the
// detected corners, their tracks and the results with every bit (%a), for the test to compare with the Python binding's.
//
// File: int32 n_points, width, height, row_stride, detect_on; float cam_T_velo[16], rect0_T_cam[16],
// P_rect0[12]; double x0[6]; float xyz[n_points * 3]; uint8 prev[height * row_stride],
// curr[height * row_stride].
#include <cstdio>
#include <cstring>
#include <vector>

#include "loam_core.hpp"

namespace {

template <typename T>
bool read(std::FILE* f, T* dst, size_t n) {
  return n == 0 || std::fread(dst, sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  std::printf("version %d\n", loam_version());
  if (argc < 2) return 0;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[5];
  loam_depth_params dp;
  loam_depth_params_default(&dp);
  loam_vo_frames_params vp = loam_amd::default_vo_frames_params();
  double x0[6];
  bool ok = read(f, hdr, 5) && read(f, dp.cam_T_velo, 16) && read(f, dp.rect0_T_cam, 16) && read(f, dp.P_rect0, 12) &&
            read(f, x0, 6);
  if (!ok || hdr[0] < 0 || hdr[1] <= 0 || hdr[2] <= 0 || hdr[3] < hdr[1] || hdr[4] < 0 || hdr[4] > 1) return 3;
  const int32_t n_pts = hdr[0], width = hdr[1], height = hdr[2], stride = hdr[3], detect_on = hdr[4];
  std::vector<float> xyz(static_cast<size_t>(n_pts) * 3);
  std::vector<uint8_t> prev(static_cast<size_t>(height) * stride), curr(prev.size());
  ok = read(f, xyz.data(), xyz.size()) && read(f, prev.data(), prev.size()) && read(f, curr.data(), curr.size());
  std::fclose(f);
  if (!ok) return 3;
  std::memcpy(vp.P_rect0, dp.P_rect0, sizeof(vp.P_rect0));
  try {
    loam_depth* depth = nullptr;
    loam_amd::check(loam_depth_create(&dp, 0, 1, &depth));
    loam_amd::check(loam_depth_input(depth, 0, xyz.data(), n_pts, 3));
    loam_amd::check(loam_depth_process(depth));
    {
      loam_amd::VisualOdometryFrames vo(vp, depth);
      vo.enableImages(loam_amd::default_lk_params(width, height));
      vo.enableDetection();
      vo.inputImagePair(0, prev.data(), curr.data(), width, height, stride, detect_on, 0);
      vo.setInitial(0, x0);
      vo.solveNlsAll();
      double x[6];
      loam_vo_frame_stats st;
      const loam_lm_stats lm = vo.result(0, x, &st);
      std::printf("x %a %a %a %a %a %a\n", x[0], x[1], x[2], x[3], x[4], x[5]);
      std::printf("lm %d %d %d %d %a %a\n", lm.iterations, lm.successful, lm.invalid, lm.termination, lm.initial_cost,
                  lm.final_cost);
      std::printf("stats %d %d %d %d %d\n", st.n_knn, st.n_matches, st.n_gated, st.counter32, st.counter22);
      const loam_amd::VisualOdometryFrames::Tracks t = vo.tracks(0);
      for (size_t i = 0; i < t.status.size(); ++i)
        std::printf("t %a %a %a %a %d %a\n", t.prev_xy[2 * i], t.prev_xy[2 * i + 1], t.curr_xy[2 * i],
                    t.curr_xy[2 * i + 1], static_cast<int>(t.status[i]), t.err[i]);
    }
    loam_depth_destroy(depth);
  } catch (const loam_amd::Error& e) {
    std::printf("error %d %s\n", e.code(), e.what());
    return 1;
  }
  return 0;
}
