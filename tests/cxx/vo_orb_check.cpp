// vo_orb_check.cpp — one frame pair of the reference's default configuration (optical_flow_match =
// false) through loam_amd::VisualOdometryFrames (loam_core.hpp), compiled with plain g++ as a node
// would.  Without an argument it prints the library version (the compile-and-link check).  With a
// file written by tests/test_gpu_orb.py it runs the depth association and the VO frame from the two
// images alone (enableImages / enableDetection / enableDescription / inputImagePairMatch) and
// prints the results with every bit (%a), for the test to compare with the Python binding's: the
// pose (x), the solver's and the frame's counts (lm, stats), the matches (m), and per image the
// kept keypoints with their descriptors in hex (k0 / k1).
//
// File: int32 n_points, width, height, row_stride; float cam_T_velo[16], rect0_T_cam[16],
// P_rect0[12]; double x0[6]; float xyz[n_points * 3]; uint8 prev[height * row_stride],
// curr[height * row_stride]
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
  int32_t hdr[4] = {0, 0, 0, 0};
  loam_depth_params dp;
  loam_depth_params_default(&dp);
  loam_vo_frames_params vp = loam_amd::default_vo_frames_params();
  double x0[6];
  std::vector<float> xyz;
  std::vector<uint8_t> a, b;
  bool ok = read(f, hdr, 4) && read(f, dp.cam_T_velo, 16) && read(f, dp.rect0_T_cam, 16) && read(f, dp.P_rect0, 12) &&
            read(f, x0, 6) && hdr[0] >= 0 && hdr[1] > 0 && hdr[2] > 0 && hdr[3] >= hdr[1];
  const int32_t n_pts = hdr[0], w = hdr[1], h = hdr[2], stride = hdr[3];
  if (ok) {
    xyz.resize(static_cast<size_t>(n_pts) * 3);
    a.resize(static_cast<size_t>(h) * stride);
    b.resize(a.size());
    ok = read(f, xyz.data(), xyz.size()) && read(f, a.data(), a.size()) && read(f, b.data(), b.size());
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
      vo.enableImages(loam_amd::default_lk_params(w, h));
      vo.enableDetection();
      vo.enableDescription();
      vo.inputImagePairMatch(0, a.data(), b.data(), w, h, stride, 0);
      vo.setInitial(0, x0);
      vo.solveNlsAll();
      double x[6];
      loam_vo_frame_stats st;
      const loam_lm_stats lm = vo.result(0, x, &st);
      std::printf("x %a %a %a %a %a %a\n", x[0], x[1], x[2], x[3], x[4], x[5]);
      std::printf("lm %d %d %d %d %a %a\n", lm.iterations, lm.successful, lm.invalid, lm.termination, lm.initial_cost,
                  lm.final_cost);
      std::printf("stats %d %d %d %d %d\n", st.n_knn, st.n_matches, st.n_gated, st.counter32, st.counter22);
      for (const auto& m : vo.matches(0)) std::printf("m %d %d %d\n", m.queryIdx, m.trainIdx, m.distance);
      for (int image = 0; image < 2; ++image) {
        const loam_amd::VisualOdometryFrames::Described d = vo.descriptors(0, image);
        for (size_t i = 0; i < d.kp_xy.size() / 2; ++i) {
          std::printf("k%d %a %a ", image, d.kp_xy[2 * i], d.kp_xy[2 * i + 1]);
          for (int k = 0; k < 32; ++k) std::printf("%02x", static_cast<unsigned>(d.desc[32 * i + k]));
          std::printf("\n");
        }
      }
    }
    loam_depth_destroy(depth);
  } catch (const loam_amd::Error& e) {
    std::printf("error %d %s\n", e.code(), e.what());
    return 1;
  }
  return 0;
}
