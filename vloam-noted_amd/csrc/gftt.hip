// gftt.hip — cv::goodFeaturesToTrack (OpenCV 4, 8-bit single channel, no mask, gradientSize 3,
// useHarrisDetector false) on MI355X: the call ImageUtil::detKeypoints makes (image_util.cpp:8-71),
// for many images at once, on level 0 of the pyramid slots lk.hip tracks in.
//
//   k_gftt_eig         grid.z = image.  A workgroup takes a 64 x 16 tile: the pixels with a halo of
//                      1 + block / 2 go to LDS (reflected coordinates), the 3 x 3 Sobel pair of the
//                      positions the boxes cover is formed from them there (int16; a position outside
//                      the image takes the derivative AT its reflected position, as boxFilter's
//                      REFLECT_101 on the derivative planes gives, which is not the derivative of the
//                      reflected pixels), then the three box sums in int32 and the smaller
//                      eigenvalue in float.  Writes the dense plane and folds the tile's maximum into
//                      the image's with an atomicMax on an order-preserving int.
//   k_gftt_candidates  threshold (THRESH_TOZERO), 3 x 3 maximum of the thresholded values, one-pixel
//                      border; appends (ordered value bits << 32 | linear index) keys, one atomic per
//                      wave.  The keys are unique: the append order does not matter.
//   k_gftt_sort        one workgroup per image: bitonic, descending = value descending, then index
//                      descending (greaterThanPtr).  Strides below 4096 keys run in LDS, the others
//                      over global memory.
//   k_gftt_select      one wavefront per image: the sequential greedy of minDistance, 64 candidates
//                      at a time.  Each lane tests its candidate against the kept corners in the
//                      3 x 3 cells around it (cell cvRound(minDistance), in device memory); the chunk
//                      is then resolved in order with ballots: the lowest pending lane is kept and
//                      knocks out the later lanes within the distance.  A decision depends only on
//                      earlier kept corners, so this is the sequential result.  Writes the corners
//                      and, on the device, the count the tracker and the frame kernels read, where
//                      the image's dst says (the previous image's keypoints for the tracker, or
//                      either image's for the descriptors of orb.hip).
//
// The box sums are exact integers (OpenCV adds float products in an order its SIMD / IPP dispatch
// decides); every float operation is a single one in calcMinEigenVal's order (-ffp-contract=off,
// a correctly rounded sqrt).
#include <algorithm>
#include <climits>
#include <cmath>

#include "gftt_dev.h"

namespace loam {

namespace {

constexpr int GF_TX = 64, GF_TY = 16, GF_THREADS = 256;
constexpr int GF_DW = GF_TX + GF_MAX_BLOCK - 1, GF_DH = GF_TY + GF_MAX_BLOCK - 1;  // derivative tile
constexpr int GF_PW = GF_DW + 2, GF_PH = GF_DH + 2;                                // pixel tile
constexpr int GF_SORT_THREADS = 1024, GF_SORT_TILE = 4096;

__device__ inline int gf_reflect(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

// float bits -> an int that orders as the float does (and back: the map is its own inverse)
__device__ inline int gf_enc(float v) {
  const int b = __float_as_int(v);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ inline float gf_dec(int e) { return __int_as_float(e >= 0 ? e : e ^ 0x7fffffff); }

// float bits -> an unsigned that orders as the float does
__device__ inline uint32_t gf_ordered(float v) {
  const uint32_t b = (uint32_t)__float_as_int(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline int gf_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void k_gftt_reset(const GfPair* gf, GfState* state, int n) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n && gf[p].active) state[p] = GfState{INT_MIN, 0, 0, 0};
}

__global__ void __launch_bounds__(GF_THREADS) k_gftt_eig(const GfPair* gf, GfState* state, const uint8_t* pyr,
                                                         size_t image_bytes, int block, float k, float* eig,
                                                         size_t eig_stride) {
  __shared__ uint8_t s_pix[GF_PW * GF_PH];
  __shared__ short s_dx[GF_DW * GF_DH], s_dy[GF_DW * GF_DH];
  const int p = blockIdx.z, tid = threadIdx.x;
  const GfPair G = gf[p];
  const int x0 = blockIdx.x * GF_TX, y0 = blockIdx.y * GF_TY;
  if (!G.active || x0 >= G.w || y0 >= G.h) return;  // the whole workgroup
  const int w = G.w, h = G.h, lo = block / 2;
  const int dw = GF_TX + block - 1, dh = GF_TY + block - 1, pw = dw + 2, ph = dh + 2;
  const uint8_t* img = pyr + ((size_t)p * 2 + G.side) * image_bytes;
  // pixel tile: position (i, j) is the coordinate (x0 - lo - 1 + i, y0 - lo - 1 + j), reflected
  for (int q = tid; q < pw * ph; q += GF_THREADS) {
    const int j = q / pw, i = q - j * pw;
    s_pix[q] = img[(size_t)gf_reflect(y0 - lo - 1 + j, h) * w + gf_reflect(x0 - lo - 1 + i, w)];
  }
  __syncthreads();
  // derivative tile: position (i, j) is the coordinate (x0 - lo + i, y0 - lo + j); its value is the
  // Sobel pair at the reflected coordinate, whose 3 x 3 pixels sit around that coordinate's own
  // place in the pixel tile for every position a box of an in-image pixel covers;
  // the others are never summed into a pixel that is written and get 0
  for (int q = tid; q < dw * dh; q += GF_THREADS) {
    const int j = q / dw, i = q - j * dw;
    const int li = gf_reflect(x0 - lo + i, w) - (x0 - lo - 1), lj = gf_reflect(y0 - lo + j, h) - (y0 - lo - 1);
    int dx = 0, dy = 0;
    if (li >= 1 && li <= pw - 2 && lj >= 1 && lj <= ph - 2) {
      const uint8_t* c = s_pix + lj * pw + li;
      const int a00 = c[-pw - 1], a01 = c[-pw], a02 = c[-pw + 1], a10 = c[-1], a12 = c[1], a20 = c[pw - 1],
                a21 = c[pw], a22 = c[pw + 1];
      dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
      dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
    }
    s_dx[q] = (short)dx;
    s_dy[q] = (short)dy;
  }
  __syncthreads();
  const int lx = tid & 63, ly = tid >> 6, x = x0 + lx;
  int best = INT_MIN;
#pragma unroll
  for (int m = 0; m < GF_TY / 4; ++m) {
    const int ty = ly + 4 * m, y = y0 + ty;
    if (x >= w || y >= h) continue;
    int sxx = 0, sxy = 0, syy = 0;
    for (int r = 0; r < block; ++r) {
      const short* ddx = s_dx + (ty + r) * dw + lx;
      const short* ddy = s_dy + (ty + r) * dw + lx;
      for (int c = 0; c < block; ++c) {
        const int gx = ddx[c], gy = ddy[c];
        sxx += gx * gx;
        sxy += gx * gy;
        syy += gy * gy;
      }
    }
    const float a = ((float)sxx * k) * 0.5f, b = (float)sxy * k, c = ((float)syy * k) * 0.5f;
    const float e = (a + c) - sqrtf((a - c) * (a - c) + b * b);
    eig[(size_t)p * eig_stride + (size_t)y * w + x] = e;
    best = max(best, gf_enc(e));
  }
  best = gf_wave_max(best);
  if ((tid & 63) == 0 && best != INT_MIN) atomicMax(&state[p].max_enc, best);
}

__global__ void __launch_bounds__(GF_THREADS) k_gftt_candidates(const GfPair* gf, GfState* state, const float* eig,
                                                                size_t eig_stride, double quality, uint64_t* keys,
                                                                int cand_pad, int max_cand) {
  const int p = blockIdx.z;
  const GfPair G = gf[p];
  if (!G.active) return;
  const int w = G.w, h = G.h;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  bool cand = false;
  float v = 0.f;
  if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
    const float thr = (float)((double)gf_dec(state[p].max_enc) * quality);
    const float* e = eig + (size_t)p * eig_stride + (size_t)y * w + x;
    v = e[0];
    if (v > thr && v != 0.f) {
      cand = true;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const float u = e[dy * w + dx];
          if ((u > thr ? u : 0.f) > v) cand = false;  // the 3 x 3 maximum of the thresholded values
        }
    }
  }
  const uint64_t bal = __ballot(cand);
  if (!bal) return;
  int base = 0;
  if ((threadIdx.x & 63) == (__ffsll((unsigned long long)bal) - 1)) base = atomicAdd(&state[p].n_cand, __popcll(bal));
  base = __shfl(base, __ffsll((unsigned long long)bal) - 1, 64);
  const int pos = base + __popcll(bal & lanemask_lt());
  if (cand && pos < max_cand)
    keys[(size_t)p * cand_pad + pos] = ((uint64_t)gf_ordered(v) << 32) | (uint32_t)(y * w + x);
}

// one compare-exchange step of the descending bitonic network on a[0 .. n) (n a power of two) whose
// element 0 has the global position g0
__device__ inline void gf_bitonic_step(uint64_t* a, int n, int g0, int k, int j, int tid) {
  for (int t = tid; t < n / 2; t += GF_SORT_THREADS) {
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const uint64_t u = a[i], v = a[l];
    const bool desc = ((g0 + i) & k) == 0;
    if (desc ? u < v : u > v) {
      a[i] = v;
      a[l] = u;
    }
  }
}

// the steps with a stride below T of the merges k_first .. k_last, tile by tile in LDS
__device__ inline void gf_sort_tiles(uint64_t* K, uint64_t* s, int N, int T, int k_first, int k_last, int tid) {
  for (int b = 0; b < N; b += T) {
    for (int i = tid; i < T; i += GF_SORT_THREADS) s[i] = K[b + i];
    __syncthreads();
    for (int k = k_first; k <= k_last; k <<= 1)
      for (int j = min(k, T) >> 1; j > 0; j >>= 1) {
        gf_bitonic_step(s, T, b, k, j, tid);
        __syncthreads();
      }
    for (int i = tid; i < T; i += GF_SORT_THREADS) K[b + i] = s[i];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(GF_SORT_THREADS) k_gftt_sort(const GfPair* gf, const GfState* state, uint64_t* keys,
                                                               int cand_pad, int max_cand) {
  __shared__ uint64_t s[GF_SORT_TILE];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (!gf[p].active) return;
  const int n = state[p].n_cand;
  if (n < 2 || n > max_cand) return;  // the whole workgroup; an overflowing list is never selected from
  int N = 2;
  while (N < n) N <<= 1;  // <= cand_pad
  uint64_t* K = keys + (size_t)p * cand_pad;
  for (int i = n + tid; i < N; i += GF_SORT_THREADS) K[i] = 0;  // below every key
  __syncthreads();
  const int T = min(N, GF_SORT_TILE);
  gf_sort_tiles(K, s, N, T, 2, T, tid);  // every tile sorted, in the direction its position asks for
  for (int k = 2 * T; k <= N; k <<= 1) {
    for (int j = k >> 1; j >= T; j >>= 1) {
      gf_bitonic_step(K, N, 0, k, j, tid);
      __syncthreads();
    }
    gf_sort_tiles(K, s, N, T, k, k, tid);
  }
}

__global__ void __launch_bounds__(64) k_gftt_select(const GfPair* gf, GfState* state, const uint64_t* keys,
                                                    int cand_pad, int max_cand, int max_corners, double min_dist2,
                                                    int cell, int cell_cap, uint32_t* cells, int* cell_cnt,
                                                    size_t cell_stride, float2* kp0, float2* kp1, int K,
                                                    VfPair* pairs, LkPair* lk) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const GfPair G = gf[p];
  if (!G.active) return;
  const int w = G.w;
  float2* kp = G.dst == GF_TO_KP1 ? kp1 : kp0;
  int n = state[p].n_cand;
  if (n > max_cand) n = 0;
  const uint64_t* Kp = keys + (size_t)p * cand_pad;
  uint32_t* C = cells + (size_t)p * cell_stride * cell_cap;
  int* CC = cell_cnt + (size_t)p * cell_stride;
  const int gw = cell ? (w + cell - 1) / cell : 0, gh = cell ? (G.h + cell - 1) / cell : 0;
  if (cell && n > 0) {
    for (int i = lane; i < gw * gh; i += 64) CC[i] = 0;
    __threadfence();
    __syncthreads();
  }
  int total = 0;
  bool full = false;
  for (int c0 = 0; c0 < n && total < max_corners; c0 += 64) {
    const int i = c0 + lane;
    const bool live = i < n;
    const uint32_t idx = live ? (uint32_t)Kp[i] : 0u;
    const int x = (int)(idx % (uint32_t)w), y = (int)(idx / (uint32_t)w);
    const int cx = cell ? x / cell : 0, cy = cell ? y / cell : 0;
    bool pass = live;
    if (cell && live) {
      for (int yy = max(0, cy - 1); yy <= min(gh - 1, cy + 1); ++yy)
        for (int xx = max(0, cx - 1); xx <= min(gw - 1, cx + 1); ++xx) {
          const int c = yy * gw + xx;
          const int m = min(__hip_atomic_load(&CC[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), cell_cap);
          for (int s = 0; s < m; ++s) {
            const uint32_t q = __hip_atomic_load(&C[(size_t)c * cell_cap + s], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            const long long dx = x - (int)(q & 0xffffu), dy = y - (int)(q >> 16);
            if ((double)(dx * dx + dy * dy) < min_dist2) pass = false;
          }
        }
    }
    uint64_t pend = __ballot(pass), kept = 0;
    if (cell) {
      while (pend) {  // uniform: the lowest pending lane is kept, the later ones near it are not
        const int l = __ffsll((unsigned long long)pend) - 1;
        const long long dx = x - __shfl(x, l, 64), dy = y - __shfl(y, l, 64);
        kept |= 1ull << l;
        pend &= ~(1ull << l);
        pend &= ~__ballot((double)(dx * dx + dy * dy) < min_dist2);
      }
    } else {
      kept = pend;
    }
    const int rank = total + __popcll(kept & lanemask_lt());
    if (((kept >> lane) & 1) && rank < max_corners) {
      kp[(size_t)p * K + rank] = make_float2((float)x, (float)y);
      if (cell) {
        const int c = cy * gw + cx;
        const int s = atomicAdd(&CC[c], 1);
        if (s < cell_cap)
          __hip_atomic_store(&C[(size_t)c * cell_cap + s], (uint32_t)x | ((uint32_t)y << 16), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        else
          full = true;
      }
    }
    total = min(max_corners, total + __popcll(kept));
    if (cell) {
      __threadfence();
      __syncthreads();
    }
  }
  if (__ballot(full)) total = 0;
  if (lane == 0) {
    state[p].n_corners = total;
    state[p].err = __ballot(full) ? 1 : 0;
    if (G.dst != GF_TO_KP1) pairs[p].n0 = total;
    if (G.dst != GF_TO_KP0) pairs[p].n1 = total;
    if (G.dst == GF_TO_TRACKS) lk[p].n = total;
  }
}

}  // namespace

int32_t gftt_plan(const loam_gftt_params* p, int max_keypoints, int max_w, int max_h, GfPlan* out) {
  if (!p || !out || p->max_corners < 1 || p->max_corners > max_keypoints || !(p->quality_level > 0.0) ||
      !std::isfinite(p->quality_level) || !(p->min_distance >= 0.0) || !std::isfinite(p->min_distance) ||
      p->block_size < 2 || p->block_size > GF_MAX_BLOCK || p->max_candidates < 1 ||
      p->max_candidates > GF_MAX_CANDIDATES) {
    set_error("loam_gftt_params: max_corners in 1..max_keypoints, quality_level > 0, min_distance >= 0 and finite, "
              "block_size in 2..15, max_candidates in 1..4194304");
    return LOAM_ERR_ARG;
  }
  if (max_w > GF_MAX_DIM || max_h > GF_MAX_DIM) {
    set_error("loam_vo_frames_enable_detection: images wider or higher than 65535");
    return LOAM_ERR_CAPACITY;
  }
  GfPlan G{};
  G.max_corners = p->max_corners;
  G.block = p->block_size;
  G.max_cand = p->max_candidates;
  G.cand_pad = 2;
  while (G.cand_pad < G.max_cand) G.cand_pad <<= 1;
  G.quality = p->quality_level;
  G.min_dist2 = p->min_distance * p->min_distance;
  const double scale = 1.0 / (4.0 * p->block_size * 255.0);
  G.k = (float)(scale * scale);
  G.max_w = max_w;
  G.max_h = max_h;
  G.eig_stride = (size_t)max_w * max_h;
  if (p->min_distance >= 1.0) {
    // cvRound (half to even); a cell wider than any image is one cell whatever its width
    G.cell = (int)std::nearbyint(std::min(p->min_distance, (double)GF_MAX_DIM + 1.0));
    // Kept corners are pairwise >= min_distance apart and those of one cell lie in a square of side
    // s = cell - 1 <= min_distance - 0.5: two need the diagonal, and no four points of a square are
    // pairwise further apart than its side
    const double s = (double)(G.cell - 1);
    G.cell_cap = 2.0 * s * s < G.min_dist2 ? 1 : 4;
    G.cell_stride = (size_t)((max_w + G.cell - 1) / G.cell) * ((max_h + G.cell - 1) / G.cell);
  } else {
    G.cell = 0;
    G.cell_cap = 1;
    G.cell_stride = 1;
  }
  *out = G;
  return LOAM_OK;
}

int32_t gftt_launch(const GfPlan& plan, const GfBuffers& B, const GfPair* pairs, int n_pairs, const uint8_t* d_pyr,
                    size_t image_bytes, float2* d_kp0, float2* d_kp1, int K, VfPair* d_pairs, LkPair* d_lk,
                    hipStream_t st) {
  int w = 0, h = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (!pairs[p].active) continue;
    w = std::max(w, pairs[p].w);
    h = std::max(h, pairs[p].h);
  }
  if (!w) return LOAM_OK;
  k_gftt_reset<<<(n_pairs + 255) / 256, 256, 0, st>>>(B.gf, B.state, n_pairs);
  k_gftt_eig<<<dim3((w + GF_TX - 1) / GF_TX, (h + GF_TY - 1) / GF_TY, n_pairs), GF_THREADS, 0, st>>>(
      B.gf, B.state, d_pyr, image_bytes, plan.block, plan.k, B.eig, plan.eig_stride);
  k_gftt_candidates<<<dim3((w + 63) / 64, (h + 3) / 4, n_pairs), GF_THREADS, 0, st>>>(
      B.gf, B.state, B.eig, plan.eig_stride, plan.quality, B.keys, plan.cand_pad, plan.max_cand);
  k_gftt_sort<<<n_pairs, GF_SORT_THREADS, 0, st>>>(B.gf, B.state, B.keys, plan.cand_pad, plan.max_cand);
  k_gftt_select<<<n_pairs, 64, 0, st>>>(B.gf, B.state, B.keys, plan.cand_pad, plan.max_cand, plan.max_corners,
                                        plan.min_dist2, plan.cell, plan.cell_cap, B.cells, B.cell_cnt,
                                        plan.cell_stride, d_kp0, d_kp1, K, d_pairs, d_lk);
  LOAM_HIP(hipGetLastError());
  return LOAM_OK;
}

}  // namespace loam

extern "C" void loam_gftt_params_default(loam_gftt_params* p) {
  if (!p) return;
  *p = loam_gftt_params{};
  p->max_corners = 1024;
  p->quality_level = 0.03;
  p->min_distance = 7.5;
  p->block_size = 5;
  p->max_candidates = 65536;
}
