// orb.hip — cv::ORB::create()->compute on given keypoints (OpenCV 4.2: patchSize 31, edgeThreshold 31,
// WTA_K 2, 32 bytes, one pyramid level at scale 1, no orientation: the keypoints keep the angle they
// come with) on MI355X: the call ImageUtil::descKeypoints makes (image_util.cpp:280-339), for both
// images of many pairs at once, on level 0 of the pyramid slots lk.hip tracks in.
//
//   k_orb_blur      grid.z = pair * 2 + image.  A workgroup takes a 64 x 16 tile: the pixels with a
//                   halo of 3 go to LDS (REFLECT_101 coordinates), the horizontal pass of the 7-tap
//                   fixed-point Gaussian (18 34 49 55 49 34 18, sum 257: cvRound(256 g) of the float
//                   kernel of sigma 2) is kept there as u16 (257 * 255 fits), the vertical pass runs
//                   from it: saturate_u8((sum + 32768) >> 16).  Exact integers.
//   k_orb_filter    one workgroup per (pair, image): KeyPointsFilter::runByImageBorder as a stable
//                   compaction of the keypoints (and their (cos, sin)) in place, a chunk of 1024 at
//                   a time (ballots; a chunk is read before any of it is written, and is written at
//                   or below where it was read).  The kept count replaces n0 / n1 of the pair table:
//                   the describing and the matching kernels read it there.
//   k_orb_describe  one wavefront per kept keypoint.  Lane l evaluates tests l, l + 64, l + 128,
//                   l + 192; the four ballots are the descriptor's four little-endian 64-bit words
//                   (bit t % 8 of byte t / 8 is test t), which lane 0 writes where k_vo_match
//                   reads them.  Keypoints without an angle of their own read the pattern the host
//                   rotated once (LDS); the others rotate the constant table by their (cos, sin):
//                   two float products and one float add or subtract per coordinate, each rounded on
//                   its own, then half to even.
//
// The filter is what keeps every sample inside the plane: edge_threshold >= 22 leaves 19 pixels of
// pattern reach around every kept centre.  The describing kernel clamps all the same.
#include <algorithm>
#include <cmath>

#include "orb_dev.h"
#include "orb_pattern.h"

namespace loam {

namespace {

constexpr int OB_TX = 64, OB_TY = 16, OB_THREADS = 256, OB_R = 3;
constexpr int OB_PW = OB_TX + 2 * OB_R, OB_PH = OB_TY + 2 * OB_R;
constexpr int OF_THREADS = 1024;
constexpr int OD_THREADS = 256, OD_WAVES = OD_THREADS / 64;

__constant__ int8_t c_orb_pattern[ORB_TESTS * 4] = {LOAM_ORB_PATTERN_VALUES};

__device__ inline int ob_reflect(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

// the 7 taps on values `step` apart
template <typename T>
__device__ inline int ob_taps(const T* c, int step) {
  return 18 * ((int)c[0] + (int)c[6 * step]) + 34 * ((int)c[step] + (int)c[5 * step]) +
         49 * ((int)c[2 * step] + (int)c[4 * step]) + 55 * (int)c[3 * step];
}

__global__ void __launch_bounds__(OB_THREADS) k_orb_blur(const OrbPair* orb, const uint8_t* pyr, size_t image_bytes,
                                                         uint8_t* blur, size_t plane_stride) {
  __shared__ uint8_t s_pix[OB_PW * OB_PH];
  __shared__ uint16_t s_row[OB_TX * OB_PH];
  const int p = blockIdx.z >> 1, side = blockIdx.z & 1, tid = threadIdx.x;
  const OrbPair O = orb[p];
  const int x0 = blockIdx.x * OB_TX, y0 = blockIdx.y * OB_TY;
  if (!O.active || x0 >= O.w || y0 >= O.h) return;  // the whole workgroup
  const int w = O.w, h = O.h;
  const uint8_t* img = pyr + ((size_t)p * 2 + side) * image_bytes;
  // pixel tile: position (i, j) is the coordinate (x0 - 3 + i, y0 - 3 + j), reflected
  for (int q = tid; q < OB_PW * OB_PH; q += OB_THREADS) {
    const int j = q / OB_PW, i = q - j * OB_PW;
    s_pix[q] = img[(size_t)ob_reflect(y0 - OB_R + j, h) * w + ob_reflect(x0 - OB_R + i, w)];
  }
  __syncthreads();
  for (int q = tid; q < OB_TX * OB_PH; q += OB_THREADS) {
    const int j = q / OB_TX, i = q - j * OB_TX;
    s_row[q] = (uint16_t)ob_taps(s_pix + j * OB_PW + i, 1);  // <= 257 * 255
  }
  __syncthreads();
  const int lx = tid & 63, ly = tid >> 6, x = x0 + lx;
  uint8_t* out = blur + ((size_t)p * 2 + side) * plane_stride;
#pragma unroll
  for (int m = 0; m < OB_TY / 4; ++m) {
    const int ty = ly + 4 * m, y = y0 + ty;
    if (x >= w || y >= h) continue;
    const int v = (ob_taps(s_row + ty * OB_TX + lx, OB_TX) + 32768) >> 16;
    out[(size_t)y * w + x] = (uint8_t)min(v, 255);
  }
}

// exclusive rank of the threads with keep set, in thread order, and their number (every thread of
// the workgroup calls it)
__device__ inline int of_block_rank(bool keep, int* ws, int* total) {
  const int tid = threadIdx.x, wid = tid >> 6;
  const uint64_t bal = __ballot(keep);
  if ((tid & 63) == 0) ws[wid] = __popcll(bal);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < OF_THREADS / 64; ++w) {
    const int v = ws[w];
    if (w < wid) off += v;
    tot += v;
  }
  __syncthreads();
  *total = tot;
  return off + __popcll(bal & lanemask_lt());
}

__global__ void __launch_bounds__(OF_THREADS) k_orb_filter(const OrbPair* orb, VfPair* pairs, float2* kp0, float2* kp1,
                                                           float2* rot0, float2* rot1, int K, int edge) {
  __shared__ int ws[OF_THREADS / 64];
  const int side = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const OrbPair O = orb[p];
  if (!O.active) return;
  int* count = side ? &pairs[p].n1 : &pairs[p].n0;
  const int n = min(max(*count, 0), K);
  __syncthreads();  // every thread has read the count thread 0 replaces
  float2* kp = (side ? kp1 : kp0) + (size_t)p * K;
  float2* rot = (side ? O.rot1 : O.rot0) ? (side ? rot1 : rot0) + (size_t)p * K : nullptr;
  const bool small = O.w <= 2 * edge || O.h <= 2 * edge;  // runByImageBorder removes every keypoint
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += OF_THREADS) {
    const int i = c0 + tid;
    bool keep = false;
    float2 v = make_float2(0.f, 0.f), r = v;
    if (i < n) {
      v = kp[i];
      if (rot) r = rot[i];
      if (!small && isfinite(v.x) && isfinite(v.y)) {
        const int cx = __float2int_rn(v.x), cy = __float2int_rn(v.y);  // cvRound; saturates
        keep = cx >= edge && cx < O.w - edge && cy >= edge && cy < O.h - edge;
      }
    }
    int tot;
    const int pos = of_block_rank(keep, ws, &tot);  // (its barriers: the chunk is read before it is written)
    if (keep) {
      kp[base + pos] = v;
      if (rot) rot[base + pos] = r;
    }
    base += tot;
  }
  if (tid == 0) *count = base;
}

__global__ void __launch_bounds__(OD_THREADS) k_orb_describe(const OrbPair* orb, const VfPair* pairs, const float2* kp0,
                                                             const float2* kp1, const float2* rot0, const float2* rot1,
                                                             const char2* uniform, const uint8_t* blur,
                                                             size_t plane_stride, uint32_t* desc0, uint32_t* desc1,
                                                             int K) {
  __shared__ char2 s_pat[ORB_TESTS * 2];
  const int side = blockIdx.y, p = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
  const OrbPair O = orb[p];
  if (!O.active) return;
  const int n = min(max(side ? pairs[p].n1 : pairs[p].n0, 0), K);
  const int q = blockIdx.x * OD_WAVES + (tid >> 6);
  if ((int)blockIdx.x * OD_WAVES >= n) return;  // the whole workgroup
  const bool own = side ? O.rot1 : O.rot0;
  if (!own)
    for (int i = tid; i < ORB_TESTS * 2; i += OD_THREADS) s_pat[i] = uniform[i];
  __syncthreads();
  if (q >= n) return;  // the whole wavefront
  const size_t o = (size_t)p * K + q;
  const float2 c = (side ? kp1 : kp0)[o];
  const int w = O.w, cx = __float2int_rn(c.x), cy = __float2int_rn(c.y);
  uint4* dst = reinterpret_cast<uint4*>((side ? desc1 : desc0) + o * ORB_DESC_DWORDS);
  if (cx < ORB_REACH || cx >= w - ORB_REACH || cy < ORB_REACH || cy >= O.h - ORB_REACH) {
    // never: the filter kept this keypoint
    if (lane == 0) dst[0] = dst[1] = make_uint4(0, 0, 0, 0);
    return;
  }
  const uint8_t* centre = blur + ((size_t)p * 2 + side) * plane_stride + (size_t)cy * w + cx;
  const float2 cs = own ? (side ? rot1 : rot0)[o] : make_float2(1.f, 0.f);
  uint64_t word[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = lane + 64 * k;
    int off[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      int ix, iy;
      if (own) {
        const float px = (float)c_orb_pattern[4 * t + 2 * e], py = (float)c_orb_pattern[4 * t + 2 * e + 1];
        ix = __float2int_rn(__fsub_rn(__fmul_rn(px, cs.x), __fmul_rn(py, cs.y)));
        iy = __float2int_rn(__fadd_rn(__fmul_rn(px, cs.y), __fmul_rn(py, cs.x)));
        ix = min(max(ix, -ORB_REACH), ORB_REACH);  // (a (cos, sin) that is none: stay in the plane)
        iy = min(max(iy, -ORB_REACH), ORB_REACH);
      } else {
        const char2 v = s_pat[2 * t + e];
        ix = v.x;
        iy = v.y;
      }
      off[e] = iy * w + ix;
    }
    word[k] = __ballot(centre[off[0]] < centre[off[1]]);
  }
  if (lane == 0) {
    dst[0] = make_uint4((uint32_t)word[0], (uint32_t)(word[0] >> 32), (uint32_t)word[1], (uint32_t)(word[1] >> 32));
    dst[1] = make_uint4((uint32_t)word[2], (uint32_t)(word[2] >> 32), (uint32_t)word[3], (uint32_t)(word[3] >> 32));
  }
}

}  // namespace

void orb_cos_sin(float angle_deg, float* cs) {
  const float angle = angle_deg * (float)(3.1415926535897932384626433832795 / 180.f);
  cs[0] = cosf(angle);
  cs[1] = sinf(angle);
}

void orb_rotated_pattern(float angle_deg, int8_t* xy) {
  float cs[2];
  orb_cos_sin(angle_deg, cs);
  for (int i = 0; i < ORB_TESTS * 2; ++i) {
    const float px = (float)ORB_PATTERN[2 * i], py = (float)ORB_PATTERN[2 * i + 1];
    const float ax = px * cs[0], bx = py * cs[1], ay = px * cs[1], by = py * cs[0];
    const float fx = ax - bx, fy = ay + by;
    xy[2 * i] = (int8_t)std::min(std::max((int)lrintf(fx), -ORB_REACH), ORB_REACH);  // cvRound: half to even
    xy[2 * i + 1] = (int8_t)std::min(std::max((int)lrintf(fy), -ORB_REACH), ORB_REACH);
  }
}

int32_t orb_launch(const OrbPlan& plan, const OrbBuffers& B, const OrbPair* pairs, int n_pairs, const uint8_t* d_pyr,
                   size_t image_bytes, float2* d_kp0, float2* d_kp1, uint32_t* d_desc0, uint32_t* d_desc1, int K,
                   int kb, VfPair* d_pairs, hipStream_t st) {
  int w = 0, h = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (!pairs[p].active) continue;
    w = std::max(w, pairs[p].w);
    h = std::max(h, pairs[p].h);
  }
  if (!w) return LOAM_OK;
  k_orb_blur<<<dim3((w + OB_TX - 1) / OB_TX, (h + OB_TY - 1) / OB_TY, 2 * n_pairs), OB_THREADS, 0, st>>>(
      B.orb, d_pyr, image_bytes, B.blur, plan.plane_stride);
  k_orb_filter<<<dim3(2, n_pairs), OF_THREADS, 0, st>>>(B.orb, d_pairs, d_kp0, d_kp1, B.rot0, B.rot1, K, plan.edge);
  if (kb > 0)
    k_orb_describe<<<dim3((kb + OD_WAVES - 1) / OD_WAVES, 2, n_pairs), OD_THREADS, 0, st>>>(
        B.orb, d_pairs, d_kp0, d_kp1, B.rot0, B.rot1, B.uniform, B.blur, plan.plane_stride, d_desc0, d_desc1, K);
  LOAM_HIP(hipGetLastError());
  return LOAM_OK;
}

}  // namespace loam

extern "C" void loam_orb_params_default(loam_orb_params* p) {
  if (!p) return;
  *p = loam_orb_params{};
  p->edge_threshold = 31;
}
