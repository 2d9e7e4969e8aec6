// orb_dev.h — ORB descriptors (cv::ORB::create()->compute on given keypoints) on images that are
// already in device memory (orb.hip).
#pragma once
#include "common.h"
#include "vo_frames_dev.h"

namespace loam {

constexpr int ORB_TESTS = 256;       // point pairs of the pattern (orb_pattern.h)
constexpr int ORB_REACH = 19;        // no rotated, rounded point lies further from the centre on either axis
constexpr int ORB_MIN_EDGE = 22;     // the pattern's reach (19) + the blur's (3)
constexpr int ORB_MAX_EDGE = 32767;
constexpr int ORB_DESC_DWORDS = 8;   // 256 bits

// one frame pair of a launch
struct OrbPair {
  int active;     // 0: the pair is skipped
  int w, h;       // level 0 of both images
  int rot0, rot1; // 1: the image's keypoints carry their own (cos, sin) in d_rot0 / d_rot1
};

struct OrbPlan {
  int edge;             // edge_threshold
  size_t plane_stride;  // bytes per blurred plane = max_w * max_h
};

struct OrbBuffers {
  OrbPair* orb;     // [pair]
  uint8_t* blur;    // [pair][2][plane_stride]
  float2* rot0;     // [pair][K] (cos, sin) of the previous image's keypoints, where rot0 is set
  float2* rot1;     // [pair][K]
  char2* uniform;   // [512] the pattern rotated by the angle of keypoints without one (-1 degree), rounded
};

// the pattern rotated by angle_deg and rounded as computeOrbDescriptors does (float products, one
// float add or subtract, cvRound): 512 (x, y) pairs
void orb_rotated_pattern(float angle_deg, int8_t* xy);
// (cos, sin) of a keypoint angle in degrees, as computeOrbDescriptors forms them
void orb_cos_sin(float angle_deg, float* cs);

// every active pair, both images: the blurred planes of level 0 of the pair's pyramid slot; the
// border filter as a stable compaction of d_kp0 / d_kp1 (and d_rot0 / d_rot1) in place, the kept
// counts into d_pairs[pair].n0 / n1; the descriptors of the kept keypoints into d_desc0 / d_desc1
// ([pair][K][8 dwords]).  kb: no pair has more keypoints per image than this.  Enqueues only.
int32_t orb_launch(const OrbPlan& plan, const OrbBuffers& B, const OrbPair* pairs, int n_pairs, const uint8_t* d_pyr,
                   size_t image_bytes, float2* d_kp0, float2* d_kp1, uint32_t* d_desc0, uint32_t* d_desc1, int K,
                   int kb, VfPair* d_pairs, hipStream_t st);

}  // namespace loam
