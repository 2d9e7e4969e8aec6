// vo_frames_check.cpp — one frame pair through loam_amd::VisualOdometryFrames (loam_core.hpp),
// compiled with plain g++ as a node would.  Without an argument it prints the library version
// (the compile-and-link check).  With a file written by tests/vo_frames_util.py (run_shim) and the
// pair's input mode it runs the depth association and the VO frame and prints the results with
// every bit (%a), for the test to compare with the Python binding's:
//   descriptors  inputDescriptors; prints the matches (m)
//   images       enableImages / inputImages; prints the tracks (t)
//   detect       enableImages / enableDetection / inputImagePair; prints the corners' tracks (t)
//
// File: int32 n_points and the mode's header (below); float cam_T_velo[16], rect0_T_cam[16],
// P_rect0[12]; double x0[6]; float xyz[n_points * 3]; then the mode's arrays:
//   descriptors  n0, n1, desc_bytes; float kp0[n0 * 2]; uint8 desc0[n0 * desc_bytes];
//                float kp1[n1 * 2]; uint8 desc1[n1 * desc_bytes]
//   images       width, height, row_stride, n; uint8 prev[height * row_stride],
//                curr[height * row_stride]; float pts[n * 2]
//   detect       width, height, row_stride, detect_on; uint8 prev[height * row_stride],
//                curr[height * row_stride]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "loam_core.hpp"

namespace {

template <typename T>
bool read(std::FILE* f, T* dst, size_t n) {
  return n == 0 || std::fread(dst, sizeof(T), n, f) == n;
}

template <typename T>
bool read(std::FILE* f, std::vector<T>* dst, size_t n) {
  dst->resize(n);
  return read(f, dst->data(), n);
}

}  // namespace

int main(int argc, char** argv) {
  std::printf("version %d\n", loam_version());
  if (argc < 2) return 0;
  const std::string mode = argc > 2 ? argv[2] : "";
  const bool desc = mode == "descriptors", detect = mode == "detect";
  if (!desc && !detect && mode != "images") return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[5] = {0, 0, 0, 0, 0};
  loam_depth_params dp;
  loam_depth_params_default(&dp);
  loam_vo_frames_params vp = loam_amd::default_vo_frames_params();
  double x0[6];
  std::vector<float> xyz, kp0, kp1;  // images: kp0 holds the points
  std::vector<uint8_t> a, b;         // descriptors of, or the images, previous / current
  bool ok = read(f, hdr, desc ? 4 : 5) && read(f, dp.cam_T_velo, 16) && read(f, dp.rect0_T_cam, 16) &&
            read(f, dp.P_rect0, 12) && read(f, x0, 6) && hdr[0] >= 0 &&
            read(f, &xyz, static_cast<size_t>(hdr[0]) * 3);
  const int32_t n_pts = hdr[0], h1 = hdr[1], h2 = hdr[2], h3 = hdr[3], h4 = hdr[4];
  if (desc) {  // n0, n1, desc_bytes
    ok = ok && h1 >= 0 && h2 >= 0 && h3 > 0 && read(f, &kp0, static_cast<size_t>(h1) * 2) &&
         read(f, &a, static_cast<size_t>(h1) * h3) && read(f, &kp1, static_cast<size_t>(h2) * 2) &&
         read(f, &b, static_cast<size_t>(h2) * h3);
    vp.desc_bytes = h3;
  } else {  // width, height, row_stride, n or detect_on
    ok = ok && h1 > 0 && h2 > 0 && h3 >= h1 && h4 >= 0 && (!detect || h4 <= 1) &&
         read(f, &a, static_cast<size_t>(h2) * h3) && read(f, &b, static_cast<size_t>(h2) * h3) &&
         (detect || read(f, &kp0, static_cast<size_t>(h4) * 2));
  }
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
      if (desc) {
        vo.inputDescriptors(0, kp0.data(), a.data(), h1, kp1.data(), b.data(), h2, 0);
      } else {
        vo.enableImages(loam_amd::default_lk_params(h1, h2));
        if (detect) {
          vo.enableDetection();
          vo.inputImagePair(0, a.data(), b.data(), h1, h2, h3, h4, 0);
        } else {
          vo.inputImages(0, a.data(), b.data(), h1, h2, h3, kp0.data(), h4, 0);
        }
      }
      vo.setInitial(0, x0);
      vo.solveNlsAll();
      double x[6];
      loam_vo_frame_stats st;
      const loam_lm_stats lm = vo.result(0, x, &st);
      std::printf("x %a %a %a %a %a %a\n", x[0], x[1], x[2], x[3], x[4], x[5]);
      std::printf("lm %d %d %d %d %a %a\n", lm.iterations, lm.successful, lm.invalid, lm.termination, lm.initial_cost,
                  lm.final_cost);
      std::printf("stats %d %d %d %d %d\n", st.n_knn, st.n_matches, st.n_gated, st.counter32, st.counter22);
      if (desc) {
        for (const auto& m : vo.matches(0)) std::printf("m %d %d %d\n", m.queryIdx, m.trainIdx, m.distance);
      } else {
        const loam_amd::VisualOdometryFrames::Tracks t = vo.tracks(0);
        for (size_t i = 0; i < t.status.size(); ++i)
          std::printf("t %a %a %a %a %d %a\n", t.prev_xy[2 * i], t.prev_xy[2 * i + 1], t.curr_xy[2 * i],
                      t.curr_xy[2 * i + 1], static_cast<int>(t.status[i]), t.err[i]);
      }
    }
    loam_depth_destroy(depth);
  } catch (const loam_amd::Error& e) {
    std::printf("error %d %s\n", e.code(), e.what());
    return 1;
  }
  return 0;
}
