// vo_frames_dev.h — the pair table of the frame kernels (vo_frames.hip).  gftt.hip's selection
// kernel writes the corner count into it, orb.hip's border filter the kept keypoints'.
#pragma once

namespace loam {

enum { VF_NONE = 0, VF_DESC = 1, VF_TRACKS = 2, VF_IMAGES = 3, VF_DETECT = 4, VF_DESCRIBE = 5, VF_MATCH = 6 };

// one frame pair as the frame kernels see it (VF_IMAGES / VF_DETECT are the host's: the kernels are
// handed such a pair as VF_TRACKS; so are VF_DESCRIBE / VF_MATCH, the two images with given or
// detected keypoints to describe: the kernels are handed such a pair as VF_DESC)
struct VfPair {
  int mode;    // VF_*: what the pair's pending input is
  int n0, n1;  // descriptors of image 0 / 1 (tracks: n0 = n1 = n)
  int stream;  // depth stream of the previous frame
};

}  // namespace loam
