// vo_frames.hip — the visual-odometry frame between the descriptors and the pose, on MI355X.
//
// Reference: VisualOdometry::solveNlsAll (src/visual_odometry/src/visual_odometry.cpp:304-509)
// with the matcher it is handed, ImageUtil::matchDescriptors (image_util.cpp:347-438: ORB,
// BFMatcher(NORM_HAMMING), knnMatch k = 2, ratio 0.8).  One handle = n_pairs independent frame
// pairs; one launch sequence per loam_vo_frames_solve for all of them, nothing read back between:
//   k_vo_match     Hamming brute force: one query descriptor per lane (in VGPRs), the train
//                  descriptors staged through LDS in tiles every lane reads at the same address
//                  (a broadcast), the train set cut into S slices over grid.y so that one pair
//                  still fills the chip; grid.z = the pair.  Writes (best, its index, second
//                  best) per (slice, query).
//   k_vo_merge     one workgroup per pair: merges the slices exactly (the second best is the
//                  smallest of every slice's second best and every losing slice's best), applies
//                  the ratio test in double as the reference does, and compacts the accepted
//                  matches stably in query order (ballots).  An accepted match has a strictly
//                  unique best (match_ratio <= 1), so no index tie ever decides one.  Tracks
//                  (optical_flow_match): the points with status 1, as (j, j, 0).
//   k_vo_assemble  one workgroup per pair, one thread per match: integer pixel coordinates and
//                  the outlier gate (:344-368), queryDepth of the previous point (dp_query_one,
//                  the body loam_depth_query runs), the CostFunctor32 / 22 record (:400-474),
//                  stable compaction: the record order is the solve's summation order.  Writes the
//                  pair's record range for the solve.
//   k_vo_solve     (vo.hip) one workgroup per pair on those records.
// A pair given its two images instead (loam_vo_frames_input_images) first runs lk.hip's pyramid and
// tracking kernels on the same stream; they leave kp0 / kp1 / status as loam_vo_frames_input_tracks
// would have, and the kernels here see a tracks pair.  A pair given the images alone
// (loam_vo_frames_input_image_pair) runs gftt.hip's corner detection in front of that: it leaves kp0
// and, on the device, the point count in the pair tables the tracker and the kernels here read.
// A pair given its two images and the keypoints of both (loam_vo_frames_input_images_keypoints), or
// the images alone in the reference's default configuration (loam_vo_frames_input_image_pair_match:
// gftt.hip on both images, one after the other through the same scratch), runs orb.hip's blur,
// border filter and descriptors on the same stream: they leave kp0 / kp1 / desc0 / desc1 and the
// kept counts as loam_vo_frames_input_descriptors would have, and the kernels here see a
// descriptors pair.
// No workgroup waits on another: the merge is a launch of its own.
// Host: one VfHost per pair.  loam_vo_frames_solve plans (the stages to run and the kernels' tables,
// from the pending inputs), enqueues (one launch sequence) and collects (the read-back; the pending
// inputs become last solves).
//
// Records: the right-hand sides are formed in float as the reference does, the 3 x 3 solve with
// K = P_rect0.leftCols(3) runs in fp64 (an LU with partial pivoting, factored once on the host),
// the solution is rounded to fp32 (point_3d_rect0_* are Vector3f) and the quotients are fp64:
// vo.vo_factors' definition (the reference's float colPivHouseholderQr is not pinned).
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "depth_dev.h"
#include "device_res.h"
#include "gftt_dev.h"
#include "lk_dev.h"
#include "orb_dev.h"
#include "vo_dev.h"
#include "vo_frames_dev.h"

namespace loam {

constexpr int VM_THREADS = 256;   // k_vo_match: queries per workgroup
constexpr int VM_TILE = 256;      // train descriptors per LDS tile
constexpr int VM_INF = 1 << 20;   // "no neighbour yet" (a distance is <= 512)
constexpr int VM_MAX_SLICES = 16;
constexpr int VA_THREADS = 1024;  // k_vo_merge / k_vo_assemble: one workgroup per pair
constexpr int VF_MAX_KEYPOINTS = 1 << 16;

constexpr size_t VF_MAX_PYRAMID_BYTES = (size_t)2 << 30;
constexpr size_t VF_MAX_DETECT_BYTES = (size_t)2 << 30;  // eigenvalue planes + candidate keys + cell grids
constexpr size_t VF_MAX_BLUR_BYTES = (size_t)2 << 30;
constexpr int VF_MAX_IMAGE_PAIRS = 32767;  // grid.z of the pyramid kernel = 2 * pairs

struct VfCount {
  int n_knn, n_matches, n_gated, counter32, counter22;
};

struct VfCam {
  double lu[9];  // P K = L U (unit L below the diagonal, U on and above), row-major
  int perm[3];
};

// exclusive rank of the threads with keep set, in thread order, and their number (every thread
// of the workgroup calls it)
__device__ inline int vf_block_rank(bool keep, int* ws, int* total) {
  const int tid = threadIdx.x, wid = tid >> 6;
  const uint64_t bal = __ballot(keep);
  if ((tid & 63) == 0) ws[wid] = __popcll(bal);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < (int)blockDim.x / 64; ++w) {
    const int v = ws[w];
    if (w < wid) off += v;
    tot += v;
  }
  __syncthreads();
  *total = tot;
  return off + __popcll(bal & lanemask_lt());
}

// WP: dwords per stored descriptor (8 or 16; shorter ones are zero-padded, which adds no bits)
template <int WP>
__global__ void __launch_bounds__(VM_THREADS) k_vo_match(const VfPair* pairs, const uint32_t* desc0,
                                                         const uint32_t* desc1, int K, int S, int3* part) {
  __shared__ uint4 tile[VM_TILE * WP / 4];
  const int p = blockIdx.z, s = blockIdx.y, tid = threadIdx.x;
  const VfPair P = pairs[p];
  const int q0 = blockIdx.x * VM_THREADS;
  if (P.mode != VF_DESC || P.n1 < 2 || q0 >= P.n0) return;  // the whole workgroup
  const int q = q0 + tid;
  const bool live = q < P.n0;
  const int ntiles = (P.n1 + VM_TILE - 1) / VM_TILE, tps = (ntiles + S - 1) / S;
  const int t_begin = min(P.n1, s * tps * VM_TILE), t_end = min(P.n1, (s + 1) * tps * VM_TILE);
  uint32_t qd[WP];
  {
    const uint4* src = reinterpret_cast<const uint4*>(desc0 + ((size_t)p * K + (live ? q : q0)) * WP);
#pragma unroll
    for (int k = 0; k < WP / 4; ++k) {
      const uint4 v = src[k];
      qd[4 * k] = v.x;
      qd[4 * k + 1] = v.y;
      qd[4 * k + 2] = v.z;
      qd[4 * k + 3] = v.w;
    }
  }
  int d0 = VM_INF, i0 = -1, d1 = VM_INF;
  for (int t0 = t_begin; t0 < t_end; t0 += VM_TILE) {
    const int nt = min(VM_TILE, t_end - t0);
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(desc1 + ((size_t)p * K + t0) * WP);
    for (int i = tid; i < nt * (WP / 4); i += VM_THREADS) tile[i] = src[i];
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
      int d = 0;
#pragma unroll
      for (int k = 0; k < WP / 4; ++k) {
        const uint4 v = tile[j * (WP / 4) + k];  // the same address in every lane
        d += __popc(qd[4 * k] ^ v.x) + __popc(qd[4 * k + 1] ^ v.y) + __popc(qd[4 * k + 2] ^ v.z) +
             __popc(qd[4 * k + 3] ^ v.w);
      }
      if (d < d1) {
        if (d < d0) {  // strict: the first of equal bests keeps the index, the other is the second
          d1 = d0;
          d0 = d;
          i0 = t0 + j;
        } else {
          d1 = d;
        }
      }
    }
  }
  if (live) part[((size_t)p * S + s) * K + q] = make_int3(d0, i0, d1);
}

__global__ void __launch_bounds__(VA_THREADS) k_vo_merge(const VfPair* pairs, const int3* part, int S, int K,
                                                         double ratio, const uint8_t* status, int3* matches,
                                                         VfCount* cnt) {
  __shared__ int ws[VA_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const VfPair P = pairs[p];
  if (P.mode == VF_NONE) return;
  const bool knn = P.mode == VF_DESC && P.n1 >= 2;  // knn_match[1] exists
  int base = 0;
  for (int c0 = 0; c0 < P.n0; c0 += VA_THREADS) {
    const int q = c0 + tid;
    bool keep = false;
    int3 m = make_int3(q, q, 0);
    if (q < P.n0) {
      if (P.mode == VF_TRACKS) {
        keep = status[(size_t)p * K + q] == 1;
      } else if (knn) {
        int d0 = VM_INF, i0 = -1, d1 = VM_INF;
        for (int s = 0; s < S; ++s) {
          const int3 e = part[((size_t)p * S + s) * K + q];
          if (e.x < d0) {
            d1 = min(d0, e.z);
            d0 = e.x;
            i0 = e.y;
          } else {
            d1 = min(d1, e.x);
          }
        }
        // image_util.cpp:417: float < 0.8 * float, evaluated in double
        keep = (double)d0 < ratio * (double)d1;
        m = make_int3(q, i0, d0);
      }
    }
    int tot;
    const int pos = vf_block_rank(keep, ws, &tot);
    if (keep) matches[(size_t)p * K + base + pos] = m;
    base += tot;
  }
  if (tid == 0) {
    cnt[p].n_knn = (P.mode == VF_TRACKS || knn) ? P.n0 : 0;
    cnt[p].n_matches = base;
  }
}

// x = K^-1 b through the host's LU
__device__ inline void vf_solve3(const VfCam& C, const double* b, double* x) {
  const double y0 = b[C.perm[0]];
  const double y1 = b[C.perm[1]] - C.lu[3] * y0;
  const double y2 = (b[C.perm[2]] - C.lu[6] * y0) - C.lu[7] * y1;
  x[2] = y2 / C.lu[8];
  x[1] = (y1 - C.lu[5] * x[2]) / C.lu[4];
  x[0] = ((y0 - C.lu[1] * x[1]) - C.lu[2] * x[2]) / C.lu[0];
}

// the float image-frame vector (a, b, c) -> point_3d_rect0 (Vector3f)
__device__ inline void vf_unproject(const VfCam& C, float a, float b, float c, float* out) {
  const double rhs[3] = {(double)a, (double)b, (double)c};
  double x[3];
  vf_solve3(C, rhs, x);
  for (int i = 0; i < 3; ++i) out[i] = (float)x[i];
}

__global__ void __launch_bounds__(VA_THREADS) k_vo_assemble(const VfPair* pairs, const int3* matches, VfCount* cnt,
                                                            const float2* kp0, const float2* kp1, int K, DepthDev D,
                                                            VfCam cam, int gate, int radius, double* records,
                                                            float* depth0, int* off) {
  __shared__ int ws[VA_THREADS / 64];
  __shared__ int n32;
  const int p = blockIdx.x, tid = threadIdx.x;
  const VfPair P = pairs[p];
  if (tid == 0) {  // an idle pair solves an empty problem
    off[2 * p] = p * K;
    off[2 * p + 1] = p * K;
    n32 = 0;
  }
  if (P.mode == VF_NONE) return;
  __syncthreads();
  const int nm = cnt[p].n_matches;
  int base = 0;
  for (int c0 = 0; c0 < nm; c0 += VA_THREADS) {
    const int i = c0 + tid;
    bool keep = false;
    float d = -1.0f;
    double rec[10];
    for (int k = 0; k < 10; ++k) rec[k] = 0.0;
    if (i < nm) {
      const int3 m = matches[(size_t)p * K + i];
      const float2 a = kp0[(size_t)p * K + m.x], b = kp1[(size_t)p * K + m.y];
      // :344-356: the pixel coordinates are stored in ints
      const int px = static_cast<int>(a.x), py = static_cast<int>(a.y);
      const int cx = static_cast<int>(b.x), cy = static_cast<int>(b.y);
      keep = true;
      if (gate > 0) {  // :363-368
        const long long dx = (long long)px - cx, dy = (long long)py - cy;
        keep = !(dx * dx + dy * dy > (long long)gate * gate);
      }
      if (keep) {
        const float fx = (float)px, fy = (float)py;
        d = dp_query_one(D, P.stream, fx, fy, radius);  // :371
        float p1[3];
        vf_unproject(cam, (float)cx, (float)cy, 1.0f, p1);
        const double x1 = (double)p1[0] / (double)p1[2], y1 = (double)p1[1] / (double)p1[2];
        if (d > 0) {  // CostFunctor32, :400-427
          float X0[3];
          vf_unproject(cam, fx * d, fy * d, d, X0);
          rec[0] = 4.0;
          rec[1] = (double)X0[0];
          rec[2] = (double)X0[1];
          rec[3] = (double)X0[2];
          rec[4] = x1;
          rec[5] = y1;
        } else {  // CostFunctor22, :452-474
          float p0[3];
          vf_unproject(cam, fx, fy, 1.0f, p0);
          rec[0] = 5.0;
          rec[4] = (double)p0[0] / (double)p0[2];
          rec[5] = (double)p0[1] / (double)p0[2];
          rec[7] = x1;
          rec[8] = y1;
        }
      }
    }
    int tot;
    const int pos = vf_block_rank(keep, ws, &tot);
    if (keep) {
      const size_t r = (size_t)p * K + base + pos;
      for (int k = 0; k < 10; ++k) records[r * 10 + k] = rec[k];
      depth0[r] = d;
    }
    const uint64_t has = __ballot(keep && d > 0);
    if ((tid & 63) == 0 && has) atomicAdd(&n32, __popcll(has));
    base += tot;
  }
  __syncthreads();
  if (tid == 0) {
    off[2 * p + 1] = p * K + base;
    cnt[p].n_gated = base;
    cnt[p].counter32 = n32;
    cnt[p].counter22 = base - n32;
  }
}

}  // namespace loam

using namespace loam;

// One pair on the host.  in: the input that waits for the next solve (mode VF_NONE: none; VF_DETECT:
// the counts are the device's).  done: what the last solve left (mode VF_NONE: never solved).
struct VfImage {
  int w, h, levels;  // level 0 of both images, the levels of their pyramids (VF_IMAGES / VF_DETECT)
};
struct VfInput {
  VfPair pair;
  VfImage img;
  int detect_on;
  int rot[2];  // VF_DESCRIBE: the image's keypoints came with angles
};
struct VfDone {
  int mode;
  int n_tracks;   // points in d_kp0 / d_kp1 / d_status (0 unless VF_TRACKS / VF_IMAGES / VF_DETECT)
  int n_kept[2];  // keypoints the border filter kept (VF_DESCRIBE / VF_MATCH)
  VfImage img;
  GfState gf[2];  // VF_DETECT: [0] the detection; VF_MATCH: the previous / current image's; else zero
  bool replaced;  // a later input has overwritten the keypoints, pyramids, planes and descriptors
};
struct VfHost {
  VfInput in;
  VfDone done;
};

struct loam_vo_frames {
  DevStream st;  // first: destroyed after everything below
  int dev = 0;
  int P = 0, K = 0;       // pairs, keypoints per image
  int W = 0, WP = 0;      // descriptor dwords given / stored
  int S_cap = 1;          // slices the partial buffer holds
  loam_vo_frames_params prm{};
  loam_depth* depth = nullptr;
  VfCam cam{};
  std::vector<VfHost> rec;      // [P]
  std::vector<double> x0, x;    // [P][6] initial values / results
  std::vector<loam_lm_stats> lm;
  std::vector<VfCount> cnt;
  std::vector<VfPair> up;       // a solve's tables, from rec[].in; they outlive the asynchronous uploads
  std::vector<LkPair> lk_up;
  std::vector<GfPair> gf_up;    // [2][P]: the first and the second detection of a solve
  std::vector<OrbPair> orb_up;
  DevPool pool;
  VfPair* d_pairs = nullptr;
  uint32_t *d_desc0 = nullptr, *d_desc1 = nullptr;  // [P][K][WP]
  float2 *d_kp0 = nullptr, *d_kp1 = nullptr;        // [P][K]
  uint8_t* d_status = nullptr;                      // [P][K]
  int3* d_part = nullptr;                           // [P][S_cap][K]
  int3* d_matches = nullptr;                        // [P][K]
  double* d_records = nullptr;                      // [P][K][10]
  float* d_depth0 = nullptr;                        // [P][K]
  int* d_off = nullptr;                             // [P][2]
  double* d_x = nullptr;                            // [P][6]
  loam_lm_stats* d_lm = nullptr;
  VfCount* d_cnt = nullptr;
  // images mode (loam_vo_frames_enable_images)
  bool lk_on = false;
  LkPlan lk{};
  uint8_t* d_pyr = nullptr;      // [P][2][lk.image_bytes]
  LkPair* d_lk = nullptr;        // [P]
  float* d_err = nullptr;        // [P][K]
  // detect mode (loam_vo_frames_enable_detection)
  bool gf_on = false;
  GfPlan gf{};
  GfBuffers gfb{};
  GfPair* d_gf2 = nullptr;       // [P] the image table and the states of a solve's second detection (a match
  GfState* d_state2 = nullptr;   // pair's current image): allocated once detection and description are enabled
  // description (loam_vo_frames_enable_description)
  bool orb_on = false;
  OrbPlan orb{};
  OrbBuffers orbb{};
  DevEvent ev[2];
  float ms = 0.f;
  ~loam_vo_frames() { (void)hipStreamSynchronize(st); }
};

namespace {

// P K = L U with partial pivoting; false when K is singular to working precision
bool vf_factor(const float* P_rect0, VfCam* C) {
  double a[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a[3 * i + j] = (double)P_rect0[4 * i + j];
  double scale = 0.0;
  for (double v : a) scale = std::max(scale, std::fabs(v));
  if (!(scale > 0.0) || !std::isfinite(scale)) return false;
  int perm[3] = {0, 1, 2};
  for (int c = 0; c < 3; ++c) {
    int piv = c;
    for (int r = c + 1; r < 3; ++r)
      if (std::fabs(a[3 * r + c]) > std::fabs(a[3 * piv + c])) piv = r;
    if (!(std::fabs(a[3 * piv + c]) > 1e-12 * scale)) return false;
    if (piv != c) {
      for (int j = 0; j < 3; ++j) std::swap(a[3 * c + j], a[3 * piv + j]);
      std::swap(perm[c], perm[piv]);
    }
    for (int r = c + 1; r < 3; ++r) {
      a[3 * r + c] /= a[3 * c + c];
      for (int j = c + 1; j < 3; ++j) a[3 * r + j] -= a[3 * r + c] * a[3 * c + j];
    }
  }
  for (int i = 0; i < 9; ++i) C->lu[i] = a[i];
  for (int i = 0; i < 3; ++i) C->perm[i] = perm[i];
  return true;
}

int32_t vf_check(loam_vo_frames* h, int32_t pair, const char* who) {
  if (!h || pair < 0 || pair >= h->P) {
    set_error(std::string(who) + ": bad handle or pair");
    return LOAM_ERR_ARG;
  }
  return LOAM_OK;
}

int32_t vf_check_input(loam_vo_frames* h, int32_t pair, int32_t n0, int32_t n1, int32_t stream, const char* who) {
  TRY(vf_check(h, pair, who));
  DepthDev D;
  int dev;
  TRY(depth_device_view(h->depth, &D, &dev));
  if (n0 < 0 || n1 < 0 || stream < 0 || stream >= D.B) {
    set_error(std::string(who) + ": bad sizes or depth stream");
    return LOAM_ERR_ARG;
  }
  if (n0 > h->K || n1 > h->K) {
    set_error(std::string(who) + ": more keypoints than max_keypoints");
    return LOAM_ERR_CAPACITY;
  }
  return LOAM_OK;
}

// an accepted input: it has overwritten what the copies read of the pair's last solve
void vf_replace(loam_vo_frames* h, int32_t pair, const VfInput& in) {
  h->rec[pair].done.replaced = true;
  h->rec[pair].in = in;
}

constexpr int vf_bit(int mode) { return 1 << mode; }
constexpr int VF_ANY = ~vf_bit(VF_NONE);
constexpr int VF_HAS_TRACKS = vf_bit(VF_TRACKS) | vf_bit(VF_IMAGES) | vf_bit(VF_DETECT);
constexpr int VF_HAS_PYRAMIDS = vf_bit(VF_IMAGES) | vf_bit(VF_DETECT);
constexpr int VF_HAS_EIG = vf_bit(VF_DETECT) | vf_bit(VF_MATCH);
constexpr int VF_HAS_ORB = vf_bit(VF_DESCRIBE) | vf_bit(VF_MATCH);

// the accessors' preamble: the pair's last solve, if it ran in one of `modes` (what every mode
// leaves, the matches and the records, only a solve writes; the rest lies where a later input has
// written)
int32_t vf_last(loam_vo_frames* h, int32_t pair, const char* who, int modes, const char* what,
                const VfDone** out) {
  TRY(vf_check(h, pair, who));
  *out = &h->rec[pair].done;
  if (!(vf_bit((*out)->mode) & modes) || (modes != VF_ANY && (*out)->replaced)) {
    set_error(std::string(who) + ": " + what);
    return LOAM_ERR_STATE;
  }
  return LOAM_OK;
}

// the checks and the copies input_images and input_image_pair share: both images into level 0 of
// the pair's pyramid slot
int32_t vf_put_images(loam_vo_frames* h, int32_t pair, const uint8_t* img_prev, const uint8_t* img_curr,
                      int32_t width, int32_t height, int32_t row_stride, const char* who, VfImage* img) {
  if (!img_prev || !img_curr || width <= 0 || height <= 0 || row_stride < width) {
    set_error(std::string(who) + ": null input or bad image size");
    return LOAM_ERR_ARG;
  }
  if (width > h->lk.max_w || height > h->lk.max_h) {
    set_error(std::string(who) + ": the image is larger than max_width x max_height");
    return LOAM_ERR_CAPACITY;
  }
  LOAM_HIP(hipSetDevice(h->dev));
  // from here on the pair's device data is being overwritten: what the last solve left there is gone,
  // and so is a pending input, whether or not every copy below and in the caller succeeds
  h->rec[pair].done.replaced = true;
  h->rec[pair].in = VfInput{};
  uint8_t* lvl0 = h->d_pyr + (size_t)pair * 2 * h->lk.image_bytes;  // level 0: dense rows
  LOAM_HIP(hipMemcpy2DAsync(lvl0, width, img_prev, row_stride, width, height, hipMemcpyHostToDevice, h->st));
  LOAM_HIP(hipMemcpy2DAsync(lvl0 + h->lk.image_bytes, width, img_curr, row_stride, width, height,
                            hipMemcpyHostToDevice, h->st));
  *img = VfImage{width, height, lk_levels(width, height, h->lk.win, h->lk.max_level)};
  return LOAM_OK;
}

// a match pair is detected on twice in a solve: the second image table and states, once the handle
// both detects and describes (a handle that only detects allocates what it always did)
int32_t vf_alloc_second_detection(loam_vo_frames* h) {
  if (!h->gf_on || !h->orb_on || h->d_gf2) return LOAM_OK;
  TRY(h->pool.alloc(&h->d_gf2, (size_t)h->P, h->st));
  TRY(h->pool.alloc(&h->d_state2, (size_t)h->P, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  return LOAM_OK;
}

struct VfStages {  // what a solve runs
  bool match, images, detect, detect2, orb;
  int qb, S;  // the matcher's query blocks and slices of the train set
  int kb;     // no pair to describe has more keypoints per image
};

// the stages and the kernels' tables, from the pending inputs
int32_t vf_plan(loam_vo_frames* h, VfStages* out) {
  int active = 0, max_n0 = 0, max_n1 = 0;
  VfStages g{};
  for (int p = 0; p < h->P; ++p) {
    const VfInput& in = h->rec[p].in;
    const VfPair& q = in.pair;
    const bool images = q.mode == VF_IMAGES || q.mode == VF_DETECT, detect = q.mode == VF_DETECT;
    const bool twice = q.mode == VF_MATCH, orb = twice || q.mode == VF_DESCRIBE;
    // an images / detect pair is a tracks pair once its points are tracked; a detect pair's n is the
    // width of the tracker's grid until the detection writes the pair's own count over it.  A pair to
    // describe is a descriptors pair once the border filter has written the kept counts over n0 / n1
    // (a match pair's: over the two detections' counts)
    h->up[p] = VfPair{images ? VF_TRACKS : orb ? VF_DESC : q.mode, q.n0, q.n1, q.stream};
    h->lk_up[p] = LkPair{images, in.img.w, in.img.h, in.img.levels, detect ? h->gf.max_corners : q.n0};
    h->gf_up[p] = GfPair{detect || twice, in.img.w, in.img.h, (short)(twice ? 0 : in.detect_on),
                         (short)(twice ? GF_TO_KP0 : GF_TO_TRACKS)};
    h->gf_up[h->P + p] = GfPair{twice, in.img.w, in.img.h, 1, GF_TO_KP1};
    h->orb_up[p] = OrbPair{orb, in.img.w, in.img.h, in.rot[0], in.rot[1]};
    if (q.mode == VF_NONE) continue;
    ++active;
    if (!depth_stream_processed(h->depth, q.stream)) {
      set_error("loam_vo_frames_solve: depth stream " + std::to_string(q.stream) + " was never processed");
      return LOAM_ERR_STATE;
    }
    g.images |= images;
    g.detect |= detect || twice;
    g.detect2 |= twice;
    g.orb |= orb;
    // the matcher's grid: a pair to describe has at most these keypoints (the counts are the device's)
    const int b0 = twice ? h->gf.max_corners : q.n0, b1 = twice ? h->gf.max_corners : q.n1;
    if (orb) g.kb = std::max({g.kb, b0, b1});
    if ((q.mode == VF_DESC || orb) && b0 > 0 && b1 >= 2) {
      g.match = true;
      max_n0 = std::max(max_n0, b0);
      max_n1 = std::max(max_n1, b1);
    }
  }
  if (!active) {
    set_error("loam_vo_frames_solve: no pair has an input");
    return LOAM_ERR_STATE;
  }
  // slices of the train set: enough workgroups for two per CU, no slice thinner than a tile
  const int qb = (max_n0 + VM_THREADS - 1) / VM_THREADS, tiles = (max_n1 + VM_TILE - 1) / VM_TILE;
  int S = 1;
  if (g.match) S = std::max(1, std::min({h->S_cap, tiles, (512 + qb * active - 1) / (qb * active)}));
  *out = VfStages{g.match, g.images, g.detect, g.detect2, g.orb, qb, S, g.kb};
  return LOAM_OK;
}

// the uploads and the launch sequence, between the handle's two events
int32_t vf_enqueue(loam_vo_frames* h, const VfStages& g, const DepthDev& D) {
  hipStream_t st = h->st;
  const int P = h->P, K = h->K, S = g.S;
  LOAM_HIP(hipMemcpyAsync(h->d_pairs, h->up.data(), sizeof(VfPair) * P, hipMemcpyHostToDevice, st));
  LOAM_HIP(hipMemcpyAsync(h->d_x, h->x0.data(), sizeof(double) * 6 * P, hipMemcpyHostToDevice, st));
  if (g.images) LOAM_HIP(hipMemcpyAsync(h->d_lk, h->lk_up.data(), sizeof(LkPair) * P, hipMemcpyHostToDevice, st));
  if (g.detect)
    LOAM_HIP(hipMemcpyAsync(h->gfb.gf, h->gf_up.data(), sizeof(GfPair) * P, hipMemcpyHostToDevice, st));
  if (g.detect2)
    LOAM_HIP(hipMemcpyAsync(h->d_gf2, h->gf_up.data() + P, sizeof(GfPair) * P, hipMemcpyHostToDevice, st));
  if (g.orb) LOAM_HIP(hipMemcpyAsync(h->orbb.orb, h->orb_up.data(), sizeof(OrbPair) * P, hipMemcpyHostToDevice, st));
  LOAM_HIP(hipEventRecord(h->ev[0], st));
  if (g.detect)  // after the tables' upload: it writes the corner counts into them
    TRY(gftt_launch(h->gf, h->gfb, h->gf_up.data(), P, h->d_pyr, h->lk.image_bytes, h->d_kp0, h->d_kp1, K, h->d_pairs,
                    h->d_lk, st));
  if (g.detect2) {  // the match pairs' current images, through the same scratch: the stream orders the two
    GfBuffers second = h->gfb;
    second.gf = h->d_gf2;
    second.state = h->d_state2;
    TRY(gftt_launch(h->gf, second, h->gf_up.data() + P, P, h->d_pyr, h->lk.image_bytes, h->d_kp0, h->d_kp1, K,
                    h->d_pairs, h->d_lk, st));
  }
  if (g.images)
    TRY(lk_launch(h->lk, h->d_lk, h->lk_up.data(), P, h->d_pyr, h->d_kp0, h->d_kp1, h->d_status, h->d_err, K, st));
  if (g.orb)
    TRY(orb_launch(h->orb, h->orbb, h->orb_up.data(), P, h->d_pyr, h->lk.image_bytes, h->d_kp0, h->d_kp1, h->d_desc0,
                   h->d_desc1, K, g.kb, h->d_pairs, st));
  if (g.match) {
    const dim3 grid(g.qb, S, P);
    if (h->WP == 8)
      k_vo_match<8><<<grid, VM_THREADS, 0, st>>>(h->d_pairs, h->d_desc0, h->d_desc1, K, S, h->d_part);
    else
      k_vo_match<16><<<grid, VM_THREADS, 0, st>>>(h->d_pairs, h->d_desc0, h->d_desc1, K, S, h->d_part);
  }
  k_vo_merge<<<P, VA_THREADS, 0, st>>>(h->d_pairs, h->d_part, S, K, h->prm.match_ratio, h->d_status, h->d_matches,
                                       h->d_cnt);
  k_vo_assemble<<<P, VA_THREADS, 0, st>>>(h->d_pairs, h->d_matches, h->d_cnt, h->d_kp0, h->d_kp1, K, D, h->cam,
                                          h->prm.remove_vo_outlier, h->prm.depth_radius, h->d_records, h->d_depth0,
                                          h->d_off);
  LOAM_HIP(hipGetLastError());
  TRY(vo_solve_launch(h->d_records, h->d_off, 2, h->d_x, h->prm.max_iterations, h->d_lm, P, st));
  LOAM_HIP(hipEventRecord(h->ev[1], st));
  return LOAM_OK;
}

// the read-back; every pending input becomes the pair's last solve
int32_t vf_collect(loam_vo_frames* h, const VfStages& g) {
  hipStream_t st = h->st;
  const int P = h->P;
  std::vector<double> x(6 * (size_t)P);
  std::vector<loam_lm_stats> lm(P);
  std::vector<VfCount> cnt(P);
  LOAM_HIP(hipMemcpyAsync(x.data(), h->d_x, sizeof(double) * 6 * P, hipMemcpyDeviceToHost, st));
  LOAM_HIP(hipMemcpyAsync(lm.data(), h->d_lm, sizeof(loam_lm_stats) * P, hipMemcpyDeviceToHost, st));
  LOAM_HIP(hipMemcpyAsync(cnt.data(), h->d_cnt, sizeof(VfCount) * P, hipMemcpyDeviceToHost, st));
  std::vector<GfState> gfs(g.detect ? 2 * (size_t)P : 0);
  if (g.detect) LOAM_HIP(hipMemcpyAsync(gfs.data(), h->gfb.state, sizeof(GfState) * P, hipMemcpyDeviceToHost, st));
  if (g.detect2)
    LOAM_HIP(hipMemcpyAsync(gfs.data() + P, h->d_state2, sizeof(GfState) * P, hipMemcpyDeviceToHost, st));
  std::vector<VfPair> kept(g.orb ? P : 0);  // the pair tables as the border filter left them
  if (g.orb) LOAM_HIP(hipMemcpyAsync(kept.data(), h->d_pairs, sizeof(VfPair) * P, hipMemcpyDeviceToHost, st));
  LOAM_HIP(hipStreamSynchronize(st));
  LOAM_HIP(hipEventElapsedTime(&h->ms, h->ev[0], h->ev[1]));
  for (int p = 0; p < P; ++p) {
    VfInput& in = h->rec[p].in;
    const int mode = in.pair.mode;
    if (mode == VF_NONE) continue;  // an idle pair keeps its earlier results
    for (int i = 0; i < 6; ++i) h->x[6 * (size_t)p + i] = x[6 * (size_t)p + i];
    h->lm[p] = lm[p];
    h->cnt[p] = cnt[p];
    VfDone d{};
    d.mode = mode;
    d.img = in.img;
    if (mode == VF_DETECT || mode == VF_MATCH) d.gf[0] = gfs[p];
    if (mode == VF_MATCH) d.gf[1] = gfs[(size_t)P + p];
    if (mode == VF_TRACKS || mode == VF_IMAGES) d.n_tracks = in.pair.n0;
    if (mode == VF_DETECT) d.n_tracks = d.gf[0].n_corners;
    if (mode == VF_DESCRIBE || mode == VF_MATCH) {
      d.n_kept[0] = kept[p].n0;
      d.n_kept[1] = kept[p].n1;
    }
    h->rec[p].done = d;
    in = VfInput{};
  }
  return LOAM_OK;
}

}  // namespace

extern "C" {

void loam_vo_frames_params_default(loam_vo_frames_params* p) {
  if (!p) return;
  *p = loam_vo_frames_params{};
  p->remove_vo_outlier = 100;
  p->match_ratio = 0.8;
  p->desc_bytes = 32;
  p->depth_radius = 2;
  p->max_iterations = 100;
  p->max_keypoints = 8192;
}

int32_t loam_vo_frames_create(const loam_vo_frames_params* p, loam_depth* depth, int32_t n_pairs,
                              loam_vo_frames** out) {
  if (!out || !p || !depth || n_pairs <= 0 || p->desc_bytes < 4 || p->desc_bytes > 64 || p->desc_bytes % 4 != 0 ||
      !(p->match_ratio > 0.0 && p->match_ratio <= 1.0) || p->depth_radius < 0 || p->max_iterations < 0 ||
      p->max_iterations > VO_MAX_ITERATIONS || p->max_keypoints <= 0 || p->max_keypoints > VF_MAX_KEYPOINTS ||
      (int64_t)n_pairs * p->max_keypoints > (int64_t)1 << 28) {
    set_error("loam_vo_frames_create: bad arguments");
    return LOAM_ERR_ARG;
  }
  *out = nullptr;
  VfCam cam;
  if (!vf_factor(p->P_rect0, &cam)) {
    set_error("loam_vo_frames_create: P_rect0.leftCols(3) is singular");
    return LOAM_ERR_ARG;
  }
  DepthDev D;
  int dev = 0;
  TRY(depth_device_view(depth, &D, &dev));
  LOAM_HIP(hipSetDevice(dev));
  std::unique_ptr<loam_vo_frames> h(new loam_vo_frames);
  h->dev = dev;
  h->depth = depth;
  h->prm = *p;
  h->cam = cam;
  h->P = n_pairs;
  h->K = p->max_keypoints;
  h->W = p->desc_bytes / 4;
  h->WP = h->W <= 8 ? 8 : 16;
  h->S_cap = std::max(1, std::min(VM_MAX_SLICES, 256 / n_pairs));
  TRY(h->st.create());
  for (auto& e : h->ev) TRY(e.create());
  const size_t P = n_pairs, K = h->K;
  auto alloc = [&](auto& ptr, size_t n) { return h->pool.alloc(&ptr, n, h->st); };
  TRY(alloc(h->d_pairs, P));
  TRY(alloc(h->d_desc0, P * K * h->WP));
  TRY(alloc(h->d_desc1, P * K * h->WP));
  TRY(alloc(h->d_kp0, P * K));
  TRY(alloc(h->d_kp1, P * K));
  TRY(alloc(h->d_status, P * K));
  TRY(alloc(h->d_part, P * h->S_cap * K));
  TRY(alloc(h->d_matches, P * K));
  TRY(alloc(h->d_records, P * K * 10));
  TRY(alloc(h->d_depth0, P * K));
  TRY(alloc(h->d_off, P * 2));
  TRY(alloc(h->d_x, P * 6));
  TRY(alloc(h->d_lm, P));
  TRY(alloc(h->d_cnt, P));
  h->rec.assign(P, VfHost{});
  h->x0.assign(P * 6, 0.0);
  h->x.assign(P * 6, 0.0);
  h->lm.assign(P, loam_lm_stats{});
  h->cnt.assign(P, VfCount{});
  h->up.assign(P, VfPair{});
  h->lk_up.assign(P, LkPair{});
  h->gf_up.assign(2 * P, GfPair{});
  h->orb_up.assign(P, OrbPair{});
  LOAM_HIP(hipStreamSynchronize(h->st));
  *out = h.release();
  return LOAM_OK;
}

int32_t loam_vo_frames_destroy(loam_vo_frames* h) {
  if (!h) return LOAM_ERR_ARG;
  (void)hipSetDevice(h->dev);
  delete h;
  return LOAM_OK;
}

int32_t loam_vo_frames_input_descriptors(loam_vo_frames* h, int32_t pair, const float* kp0_xy,
                                         const uint8_t* desc0, int32_t n0, const float* kp1_xy,
                                         const uint8_t* desc1, int32_t n1, int32_t depth_stream_prev) {
  const char* who = "loam_vo_frames_input_descriptors";
  TRY(vf_check_input(h, pair, n0, n1, depth_stream_prev, who));
  if ((n0 > 0 && (!kp0_xy || !desc0)) || (n1 > 0 && (!kp1_xy || !desc1))) {
    set_error(std::string(who) + ": null input");
    return LOAM_ERR_ARG;
  }
  LOAM_HIP(hipSetDevice(h->dev));
  const size_t o = (size_t)pair * h->K, row = sizeof(uint32_t) * h->W, pitch = sizeof(uint32_t) * h->WP;
  // rows are stored WP dwords apart; the padding stays zero from create
  if (n0) {
    LOAM_HIP(hipMemcpy2DAsync(h->d_desc0 + o * h->WP, pitch, desc0, row, row, n0, hipMemcpyHostToDevice, h->st));
    LOAM_HIP(hipMemcpyAsync(h->d_kp0 + o, kp0_xy, sizeof(float2) * n0, hipMemcpyHostToDevice, h->st));
  }
  if (n1) {
    LOAM_HIP(hipMemcpy2DAsync(h->d_desc1 + o * h->WP, pitch, desc1, row, row, n1, hipMemcpyHostToDevice, h->st));
    LOAM_HIP(hipMemcpyAsync(h->d_kp1 + o, kp1_xy, sizeof(float2) * n1, hipMemcpyHostToDevice, h->st));
  }
  LOAM_HIP(hipStreamSynchronize(h->st));  // the caller's buffers are free after return
  vf_replace(h, pair, VfInput{{VF_DESC, n0, n1, depth_stream_prev}, {}, 0});
  return LOAM_OK;
}

int32_t loam_vo_frames_input_tracks(loam_vo_frames* h, int32_t pair, const float* prev_xy, const float* curr_xy,
                                    const uint8_t* status, int32_t n, int32_t depth_stream_prev) {
  const char* who = "loam_vo_frames_input_tracks";
  TRY(vf_check_input(h, pair, n, n, depth_stream_prev, who));
  if (n > 0 && (!prev_xy || !curr_xy || !status)) {
    set_error(std::string(who) + ": null input");
    return LOAM_ERR_ARG;
  }
  LOAM_HIP(hipSetDevice(h->dev));
  const size_t o = (size_t)pair * h->K;
  if (n) {
    LOAM_HIP(hipMemcpyAsync(h->d_kp0 + o, prev_xy, sizeof(float2) * n, hipMemcpyHostToDevice, h->st));
    LOAM_HIP(hipMemcpyAsync(h->d_kp1 + o, curr_xy, sizeof(float2) * n, hipMemcpyHostToDevice, h->st));
    LOAM_HIP(hipMemcpyAsync(h->d_status + o, status, (size_t)n, hipMemcpyHostToDevice, h->st));
  }
  LOAM_HIP(hipStreamSynchronize(h->st));
  vf_replace(h, pair, VfInput{{VF_TRACKS, n, n, depth_stream_prev}, {}, 0});
  return LOAM_OK;
}

int32_t loam_vo_frames_enable_images(loam_vo_frames* h, const loam_lk_params* p) {
  if (!h || !p) {
    set_error("loam_vo_frames_enable_images: null handle or parameters");
    return LOAM_ERR_ARG;
  }
  LkPlan plan;
  TRY(lk_plan(p, &plan));
  if (h->lk_on) {
    set_error("loam_vo_frames_enable_images: the handle already has its pyramids");
    return LOAM_ERR_STATE;
  }
  if (h->P > VF_MAX_IMAGE_PAIRS || plan.image_bytes > VF_MAX_PYRAMID_BYTES / 2 / (size_t)h->P) {
    set_error("loam_vo_frames_enable_images: more than 2 GiB of pyramids or more than 32767 pairs");
    return LOAM_ERR_CAPACITY;
  }
  LOAM_HIP(hipSetDevice(h->dev));
  TRY(h->pool.alloc(&h->d_pyr, (size_t)h->P * 2 * plan.image_bytes, h->st));
  TRY(h->pool.alloc(&h->d_lk, (size_t)h->P, h->st));
  TRY(h->pool.alloc(&h->d_err, (size_t)h->P * h->K, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  h->lk = plan;
  h->lk_on = true;
  return LOAM_OK;
}

int32_t loam_vo_frames_input_images(loam_vo_frames* h, int32_t pair, const uint8_t* img_prev,
                                    const uint8_t* img_curr, int32_t width, int32_t height, int32_t row_stride,
                                    const float* pts_xy, int32_t n, int32_t depth_stream_prev) {
  const char* who = "loam_vo_frames_input_images";
  TRY(vf_check(h, pair, who));
  if (!h->lk_on) {
    set_error(std::string(who) + ": call loam_vo_frames_enable_images first");
    return LOAM_ERR_STATE;
  }
  TRY(vf_check_input(h, pair, n, n, depth_stream_prev, who));
  if (n > 0 && !pts_xy) {
    set_error(std::string(who) + ": null input or bad image size");
    return LOAM_ERR_ARG;
  }
  VfImage img;
  TRY(vf_put_images(h, pair, img_prev, img_curr, width, height, row_stride, who, &img));
  if (n)
    LOAM_HIP(hipMemcpyAsync(h->d_kp0 + (size_t)pair * h->K, pts_xy, sizeof(float2) * n, hipMemcpyHostToDevice, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  vf_replace(h, pair, VfInput{{VF_IMAGES, n, n, depth_stream_prev}, img, 0});
  return LOAM_OK;
}

int32_t loam_vo_frames_enable_detection(loam_vo_frames* h, const loam_gftt_params* p) {
  const char* who = "loam_vo_frames_enable_detection";
  if (!h || !p) {
    set_error(std::string(who) + ": null handle or parameters");
    return LOAM_ERR_ARG;
  }
  if (!h->lk_on) {
    set_error(std::string(who) + ": call loam_vo_frames_enable_images first");
    return LOAM_ERR_STATE;
  }
  if (h->gf_on) {
    set_error(std::string(who) + ": the handle already detects");
    return LOAM_ERR_STATE;
  }
  GfPlan plan;
  TRY(gftt_plan(p, h->K, h->lk.max_w, h->lk.max_h, &plan));
  const size_t per_image = sizeof(float) * plan.eig_stride + sizeof(uint64_t) * plan.cand_pad +
                           (sizeof(uint32_t) * plan.cell_cap + sizeof(int)) * plan.cell_stride;
  if (per_image > VF_MAX_DETECT_BYTES / (size_t)h->P) {
    set_error(std::string(who) + ": more than 2 GiB of eigenvalue planes, candidate keys and cell grids");
    return LOAM_ERR_CAPACITY;
  }
  LOAM_HIP(hipSetDevice(h->dev));
  const size_t P = h->P;
  GfBuffers B{};
  TRY(h->pool.alloc(&B.gf, P, h->st));
  TRY(h->pool.alloc(&B.state, P, h->st));
  TRY(h->pool.alloc(&B.eig, P * plan.eig_stride, h->st));
  TRY(h->pool.alloc(&B.keys, P * plan.cand_pad, h->st));
  TRY(h->pool.alloc(&B.cells, P * plan.cell_stride * plan.cell_cap, h->st));
  TRY(h->pool.alloc(&B.cell_cnt, P * plan.cell_stride, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  h->gf = plan;
  h->gfb = B;
  h->gf_on = true;
  return vf_alloc_second_detection(h);
}

int32_t loam_vo_frames_input_image_pair(loam_vo_frames* h, int32_t pair, const uint8_t* img_prev,
                                        const uint8_t* img_curr, int32_t width, int32_t height,
                                        int32_t row_stride, int32_t detect_on, int32_t depth_stream_prev) {
  const char* who = "loam_vo_frames_input_image_pair";
  TRY(vf_check(h, pair, who));
  if (!h->gf_on) {
    set_error(std::string(who) + ": call loam_vo_frames_enable_detection first");
    return LOAM_ERR_STATE;
  }
  TRY(vf_check_input(h, pair, 0, 0, depth_stream_prev, who));
  if (detect_on < 0 || detect_on > 1) {
    set_error(std::string(who) + ": detect_on is 0 (the previous image) or 1 (the current one)");
    return LOAM_ERR_ARG;
  }
  VfImage img;
  TRY(vf_put_images(h, pair, img_prev, img_curr, width, height, row_stride, who, &img));
  LOAM_HIP(hipStreamSynchronize(h->st));
  vf_replace(h, pair, VfInput{{VF_DETECT, 0, 0, depth_stream_prev}, img, detect_on});
  return LOAM_OK;
}

int32_t loam_vo_frames_enable_description(loam_vo_frames* h, const loam_orb_params* p) {
  const char* who = "loam_vo_frames_enable_description";
  if (!h || !p) {
    set_error(std::string(who) + ": null handle or parameters");
    return LOAM_ERR_ARG;
  }
  if (h->prm.desc_bytes != 4 * ORB_DESC_DWORDS || p->edge_threshold < ORB_MIN_EDGE || p->edge_threshold > ORB_MAX_EDGE) {
    set_error(std::string(who) + ": desc_bytes is 32 for ORB, edge_threshold in 22..32767");
    return LOAM_ERR_ARG;
  }
  if (!h->lk_on) {
    set_error(std::string(who) + ": call loam_vo_frames_enable_images first");
    return LOAM_ERR_STATE;
  }
  if (h->orb_on) {
    set_error(std::string(who) + ": the handle already describes");
    return LOAM_ERR_STATE;
  }
  OrbPlan plan{p->edge_threshold, (size_t)h->lk.max_w * h->lk.max_h};
  if (plan.plane_stride > VF_MAX_BLUR_BYTES / 2 / (size_t)h->P) {
    set_error(std::string(who) + ": more than 2 GiB of blurred planes");
    return LOAM_ERR_CAPACITY;
  }
  LOAM_HIP(hipSetDevice(h->dev));
  const size_t P = h->P, K = h->K;
  OrbBuffers B{};
  TRY(h->pool.alloc(&B.orb, P, h->st));
  TRY(h->pool.alloc(&B.blur, P * 2 * plan.plane_stride, h->st));
  TRY(h->pool.alloc(&B.rot0, P * K, h->st));
  TRY(h->pool.alloc(&B.rot1, P * K, h->st));
  TRY(h->pool.alloc(&B.uniform, (size_t)ORB_TESTS * 2, h->st));
  int8_t xy[ORB_TESTS * 4];
  orb_rotated_pattern(-1.f, xy);  // cv::KeyPoint's default angle
  LOAM_HIP(hipMemcpyAsync(B.uniform, xy, sizeof(xy), hipMemcpyHostToDevice, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  h->orb = plan;
  h->orbb = B;
  h->orb_on = true;
  return vf_alloc_second_detection(h);
}

int32_t loam_vo_frames_input_images_keypoints(loam_vo_frames* h, int32_t pair, const uint8_t* img_prev,
                                              const uint8_t* img_curr, int32_t width, int32_t height,
                                              int32_t row_stride, const float* kp0_xy, const float* angle0_deg,
                                              int32_t n0, const float* kp1_xy, const float* angle1_deg, int32_t n1,
                                              int32_t depth_stream_prev) {
  const char* who = "loam_vo_frames_input_images_keypoints";
  TRY(vf_check(h, pair, who));
  if (!h->orb_on) {
    set_error(std::string(who) + ": call loam_vo_frames_enable_description first");
    return LOAM_ERR_STATE;
  }
  TRY(vf_check_input(h, pair, n0, n1, depth_stream_prev, who));
  if ((n0 > 0 && !kp0_xy) || (n1 > 0 && !kp1_xy)) {
    set_error(std::string(who) + ": null input or bad image size");
    return LOAM_ERR_ARG;
  }
  const size_t o = (size_t)pair * h->K;
  // (cos, sin) of the keypoints that come with an angle: the host's cosf / sinf, as OpenCV's
  std::vector<float> cs[2];
  const float* angles[2] = {n0 > 0 ? angle0_deg : nullptr, n1 > 0 ? angle1_deg : nullptr};
  const float* kps[2] = {kp0_xy, kp1_xy};
  float2* d_kp[2] = {h->d_kp0, h->d_kp1};
  float2* d_rot[2] = {h->orbb.rot0, h->orbb.rot1};
  const int n[2] = {n0, n1};
  for (int s = 0; s < 2; ++s) {
    if (!angles[s]) continue;
    cs[s].resize(2 * (size_t)n[s]);
    for (int i = 0; i < n[s]; ++i) orb_cos_sin(angles[s][i], &cs[s][2 * (size_t)i]);
  }
  VfImage img;
  auto copies = [&]() -> int32_t {
    TRY(vf_put_images(h, pair, img_prev, img_curr, width, height, row_stride, who, &img));
    for (int s = 0; s < 2; ++s) {
      if (n[s]) LOAM_HIP(hipMemcpyAsync(d_kp[s] + o, kps[s], sizeof(float2) * n[s], hipMemcpyHostToDevice, h->st));
      if (angles[s])
        LOAM_HIP(hipMemcpyAsync(d_rot[s] + o, cs[s].data(), sizeof(float2) * n[s], hipMemcpyHostToDevice, h->st));
    }
    return LOAM_OK;
  };
  const int32_t rc = copies();
  const hipError_t drained = hipStreamSynchronize(h->st);  // also after a failure: cs and the caller's buffers are free
  TRY(rc);
  LOAM_HIP(drained);
  img.levels = 1;  // no pyramid is built
  vf_replace(h, pair, VfInput{{VF_DESCRIBE, n0, n1, depth_stream_prev}, img, 0, {angles[0] != nullptr, angles[1] != nullptr}});
  return LOAM_OK;
}

int32_t loam_vo_frames_input_image_pair_match(loam_vo_frames* h, int32_t pair, const uint8_t* img_prev,
                                              const uint8_t* img_curr, int32_t width, int32_t height,
                                              int32_t row_stride, int32_t depth_stream_prev) {
  const char* who = "loam_vo_frames_input_image_pair_match";
  TRY(vf_check(h, pair, who));
  if (!h->gf_on || !h->orb_on) {
    set_error(std::string(who) + ": call loam_vo_frames_enable_detection and loam_vo_frames_enable_description first");
    return LOAM_ERR_STATE;
  }
  TRY(vf_check_input(h, pair, 0, 0, depth_stream_prev, who));
  VfImage img;
  TRY(vf_put_images(h, pair, img_prev, img_curr, width, height, row_stride, who, &img));
  img.levels = 1;  // no pyramid is built
  LOAM_HIP(hipStreamSynchronize(h->st));
  vf_replace(h, pair, VfInput{{VF_MATCH, 0, 0, depth_stream_prev}, img, 0, {0, 0}});
  return LOAM_OK;
}

int32_t loam_vo_frames_descriptors_copy(loam_vo_frames* h, int32_t pair, int32_t image, float* kp_xy, uint8_t* desc,
                                        int32_t cap) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_descriptors_copy", VF_HAS_ORB,
              "the pair has no solved description (or a later input replaced it)", &d));
  if (image < 0 || image > 1) {
    set_error("loam_vo_frames_descriptors_copy: image is 0 or 1");
    return LOAM_ERR_ARG;
  }
  const int n = d->n_kept[image];
  if (n > cap || n == 0) return n;  // the count only
  LOAM_HIP(hipSetDevice(h->dev));
  const size_t o = (size_t)pair * h->K;
  if (kp_xy) LOAM_HIP(hipMemcpy(kp_xy, (image ? h->d_kp1 : h->d_kp0) + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
  if (desc)
    LOAM_HIP(hipMemcpy(desc, (image ? h->d_desc1 : h->d_desc0) + o * h->WP, sizeof(uint32_t) * h->WP * n,
                       hipMemcpyDeviceToHost));
  return n;
}

int32_t loam_vo_frames_blur_copy(loam_vo_frames* h, int32_t pair, int32_t image, uint8_t* out, int32_t cap,
                                 int32_t* wh) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_blur_copy", VF_HAS_ORB,
              "the pair has no solved description (or a later input replaced it)", &d));
  if (image < 0 || image > 1) {
    set_error("loam_vo_frames_blur_copy: image is 0 or 1");
    return LOAM_ERR_ARG;
  }
  if (wh) {
    wh[0] = d->img.w;
    wh[1] = d->img.h;
  }
  const int n = d->img.w * d->img.h;
  if (n > cap || !out) return n;  // the size only
  LOAM_HIP(hipSetDevice(h->dev));
  LOAM_HIP(hipMemcpy(out, h->orbb.blur + ((size_t)pair * 2 + image) * h->orb.plane_stride, (size_t)n,
                     hipMemcpyDeviceToHost));
  return n;
}

int32_t loam_vo_frames_set_initial(loam_vo_frames* h, int32_t pair, const double* x6) {
  TRY(vf_check(h, pair, "loam_vo_frames_set_initial"));
  for (int i = 0; i < 6; ++i) h->x0[(size_t)pair * 6 + i] = x6 ? x6[i] : 0.0;
  return LOAM_OK;
}

int32_t loam_vo_frames_solve(loam_vo_frames* h) {
  if (!h) return LOAM_ERR_ARG;
  VfStages g;
  TRY(vf_plan(h, &g));
  DepthDev D;
  int dev;
  TRY(depth_device_view(h->depth, &D, &dev));
  LOAM_HIP(hipSetDevice(h->dev));
  TRY(vf_enqueue(h, g, D));
  return vf_collect(h, g);
}

int32_t loam_vo_frames_result(loam_vo_frames* h, int32_t pair, double* x6, loam_lm_stats* lm,
                              loam_vo_frame_stats* st) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_result", VF_ANY, "the pair was never solved", &d));
  for (const GfState& g : d->gf) {  // zero where the pair had no detection
    if (g.n_cand > h->gf.max_cand) {
      set_error("loam_vo_frames_result: the image has " + std::to_string(g.n_cand) +
                " corner candidates, more than max_candidates = " + std::to_string(h->gf.max_cand));
      return LOAM_ERR_CAPACITY;
    }
    if (g.err) {
      set_error("loam_vo_frames_result: a cell of the corner grid was full");
      return LOAM_ERR_CAPACITY;
    }
  }
  if (x6)
    for (int i = 0; i < 6; ++i) x6[i] = h->x[(size_t)pair * 6 + i];
  if (lm) *lm = h->lm[pair];
  if (st) {
    const VfCount& c = h->cnt[pair];
    st->n_knn = c.n_knn;
    st->n_matches = c.n_matches;
    st->n_gated = c.n_gated;
    st->counter32 = c.counter32;
    st->counter22 = c.counter22;
    st->ms = (double)h->ms;
  }
  return LOAM_OK;
}

int32_t loam_vo_frames_matches_copy(loam_vo_frames* h, int32_t pair, int32_t* out, int32_t cap) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_matches_copy", VF_ANY, "the pair has no solved frame", &d));
  const int n = h->cnt[pair].n_matches;
  if (n > cap || n == 0 || !out) return n;  // the count only
  LOAM_HIP(hipSetDevice(h->dev));
  LOAM_HIP(hipMemcpy(out, h->d_matches + (size_t)pair * h->K, sizeof(int3) * n, hipMemcpyDeviceToHost));
  return n;
}

int32_t loam_vo_frames_records_copy(loam_vo_frames* h, int32_t pair, double* records, float* depth0,
                                    int32_t cap) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_records_copy", VF_ANY, "the pair has no solved frame", &d));
  const int n = h->cnt[pair].n_gated;
  if (n > cap || n == 0) return n;  // the count only
  LOAM_HIP(hipSetDevice(h->dev));
  const size_t o = (size_t)pair * h->K;
  if (records) LOAM_HIP(hipMemcpy(records, h->d_records + o * 10, sizeof(double) * 10 * n, hipMemcpyDeviceToHost));
  if (depth0) LOAM_HIP(hipMemcpy(depth0, h->d_depth0 + o, sizeof(float) * n, hipMemcpyDeviceToHost));
  return n;
}

int32_t loam_vo_frames_tracks_copy(loam_vo_frames* h, int32_t pair, float* prev_xy, float* curr_xy,
                                   uint8_t* status, float* err, int32_t cap) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_tracks_copy", VF_HAS_TRACKS,
              "the pair has no solved tracks (never solved, solved from descriptors, or replaced by a later input)",
              &d));
  const int n = d->n_tracks;
  if (n > cap || n == 0) return n;  // the count only
  LOAM_HIP(hipSetDevice(h->dev));
  const size_t o = (size_t)pair * h->K;
  if (prev_xy) LOAM_HIP(hipMemcpy(prev_xy, h->d_kp0 + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
  if (curr_xy) LOAM_HIP(hipMemcpy(curr_xy, h->d_kp1 + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
  if (status) LOAM_HIP(hipMemcpy(status, h->d_status + o, (size_t)n, hipMemcpyDeviceToHost));
  if (err) {
    if (d->mode == VF_IMAGES || d->mode == VF_DETECT)
      LOAM_HIP(hipMemcpy(err, h->d_err + o, sizeof(float) * n, hipMemcpyDeviceToHost));
    else
      std::fill(err, err + n, 0.f);
  }
  return n;
}

int32_t loam_vo_frames_pyramid_copy(loam_vo_frames* h, int32_t pair, int32_t image, int32_t level, uint8_t* out,
                                    int32_t cap, int32_t* wh) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_pyramid_copy", VF_HAS_PYRAMIDS,
              "the pair has no solved images (or a later input replaced them)", &d));
  const VfImage& L = d->img;
  if (image < 0 || image > 1 || level < 0 || level >= L.levels) {
    set_error("loam_vo_frames_pyramid_copy: image is 0 or 1, level below the pair's level count");
    return LOAM_ERR_ARG;
  }
  int w = L.w, ht = L.h;
  for (int l = 0; l < level; ++l) {
    w = (w + 1) / 2;
    ht = (ht + 1) / 2;
  }
  if (wh) {
    wh[0] = w;
    wh[1] = ht;
  }
  const int n = w * ht;
  if (n > cap || !out) return n;  // the size only
  LOAM_HIP(hipSetDevice(h->dev));
  LOAM_HIP(hipMemcpy(out, h->d_pyr + ((size_t)pair * 2 + image) * h->lk.image_bytes + h->lk.lvl_off[level], (size_t)n,
                     hipMemcpyDeviceToHost));
  return n;
}

int32_t loam_vo_frames_eig_copy(loam_vo_frames* h, int32_t pair, float* out, int32_t cap, int32_t* wh) {
  const VfDone* d;
  TRY(vf_last(h, pair, "loam_vo_frames_eig_copy", VF_HAS_EIG,
              "the pair has no solved detection (or a later input replaced it)", &d));
  const VfImage& G = d->img;
  if (wh) {
    wh[0] = G.w;
    wh[1] = G.h;
  }
  const int n = G.w * G.h;
  if (n > cap || !out) return n;  // the size only
  LOAM_HIP(hipSetDevice(h->dev));
  LOAM_HIP(hipMemcpy(out, h->gfb.eig + (size_t)pair * h->gf.eig_stride, sizeof(float) * n, hipMemcpyDeviceToHost));
  return n;
}

}  // extern "C"
