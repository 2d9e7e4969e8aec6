// lk.hip — cv::calcOpticalFlowPyrLK (OpenCV 4.2, 8-bit single channel, flags 0) on MI355X: the
// call ImageUtil::calculateOpticalFlow makes (image_util.cpp:503-570), for many frame pairs at once.
//
//   k_lk_pyr_down  one launch per level for every pair and both images: [1 4 6 4 1]^2 on the even
//                  samples, REFLECT_101, (sum + 128) >> 8 (cv::pyrDown on CV_8U).
//   k_lk_track     one wavefront (= one workgroup) per point, walking the levels from the top:
//                    - the (win + 3)^2 patch of the previous image around the window goes to LDS
//                      (reflected coordinates), the Scharr derivatives of the (win + 1)^2 positions
//                      the window interpolates between are formed from it there (0 outside the
//                      image, as calcSharrDeriv + the constant border give); nothing of the
//                      derivative images ever exists in device memory;
//                    - lanes take the win^2 window pixels 64 at a time; I, Ix, Iy of a lane's
//                      pixels stay in its registers for the iterations;
//                    - every iteration stages the (win + 1)^2 patch of the current image, the
//                      lanes form diff * Ix / diff * Iy partials in int32, a butterfly leaves the
//                      exact int64 totals in every lane, and every lane takes the same 2 x 2
//                      float step: the loop control is uniform without a broadcast.
//                  One wavefront per workgroup makes __syncthreads() the LDS hand-off between the
//                  stages although points finish after different numbers of iterations.
//
// The five sums are exact integers (OpenCV adds floats in an order its SIMD width decides); all
// float arithmetic is single operations in OpenCV's order (the library is built with
// -ffp-contract=off; sqrt and the divisions are correctly rounded).
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "lk_dev.h"

namespace loam {

namespace {

constexpr int LK_W_BITS = 14;

struct LkDev {
  int win, max_count;
  double eps2, min_eig;
  size_t lvl_off[LK_MAX_LEVELS];
  size_t image_bytes;
};

// cv::borderInterpolate(i, n, BORDER_REFLECT_101), any i
__host__ __device__ inline int lk_reflect(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

__host__ __device__ inline void lk_level_size(int w, int h, int level, int* lw, int* lh) {
  for (int i = 0; i < level; ++i) {
    w = (w + 1) / 2;
    h = (h + 1) / 2;
  }
  *lw = w;
  *lh = h;
}

// cvFloor; a value no int holds (or a NaN) becomes INT_MIN as cvtss2si makes it, which fails
// every bounds check
__device__ inline int lk_floor(float v) {
  if (!(v > -1.0e9f && v < 1.0e9f)) return INT_MIN;
  const int i = (int)v;
  return i - (i > v);
}

__device__ inline bool lk_outside(int x, int y, int w, int h, int win) {
  return x < -win || x >= w || y < -win || y >= h;
}

struct LkWeights {
  int w00, w01, w10, w11;
};

// the fixed-point bilinear weights of p - floor(p) (cvRound: half to even)
__device__ inline LkWeights lk_weights(float px, float py, int ix, int iy) {
  const float a = px - (float)ix, b = py - (float)iy;
  LkWeights W;
  W.w00 = (int)rintf((1.f - a) * (1.f - b) * (float)(1 << LK_W_BITS));
  W.w01 = (int)rintf(a * (1.f - b) * (float)(1 << LK_W_BITS));
  W.w10 = (int)rintf((1.f - a) * b * (float)(1 << LK_W_BITS));
  W.w11 = (1 << LK_W_BITS) - W.w00 - W.w01 - W.w10;
  return W;
}

__device__ inline int lk_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

__device__ inline long long lk_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (float)S * 2^-20 of an exact integer sum (|S| < 2^53: the double is exact, one rounding)
__device__ inline float lk_scaled(long long s) { return (float)(double)s * (1.f / (float)(1 << 20)); }

__global__ void __launch_bounds__(256) k_lk_pyr_down(const LkPair* pairs, uint8_t* pyr, LkDev L, int level) {
  const int pi = blockIdx.z >> 1;
  const LkPair P = pairs[pi];
  if (!P.active || level >= P.levels) return;
  int sw, sh, dw, dh;
  lk_level_size(P.w, P.h, level - 1, &sw, &sh);
  lk_level_size(P.w, P.h, level, &dw, &dh);
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  uint8_t* base = pyr + (size_t)blockIdx.z * L.image_bytes;
  const uint8_t* src = base + L.lvl_off[level - 1];
  int xs[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) xs[k] = lk_reflect(2 * x + k - 2, sw);
  const int wt[5] = {1, 4, 6, 4, 1};
  int sum = 0;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const uint8_t* row = src + (size_t)lk_reflect(2 * y + r - 2, sh) * sw;
    sum += wt[r] * (row[xs[0]] + 4 * row[xs[1]] + 6 * row[xs[2]] + 4 * row[xs[3]] + row[xs[4]]);
  }
  base[L.lvl_off[level] + (size_t)y * dw + x] = (uint8_t)((sum + 128) >> 8);
}

// PASSES * 64 >= win^2
template <int PASSES>
__global__ void __launch_bounds__(64) k_lk_track(const LkPair* pairs, const uint8_t* pyr, LkDev L, const float2* kp0,
                                                 float2* kp1, uint8_t* status, float* err, int K) {
  constexpr int PW_MAX = LK_MAX_WIN + 3, DW_MAX = LK_MAX_WIN + 1;
  __shared__ uint8_t s_img[PW_MAX * PW_MAX];  // the previous image's patch, then the current one's
  __shared__ short s_dx[DW_MAX * DW_MAX], s_dy[DW_MAX * DW_MAX];
  const int pi = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  const LkPair P = pairs[pi];
  if (!P.active || i >= P.n) return;
  const int win = L.win, nwin = win * win, pw = win + 3, dw = win + 1;
  const float half = (float)(win - 1) * 0.5f;
  const float2 pt = kp0[(size_t)pi * K + i];
  const uint8_t* prev = pyr + (size_t)pi * 2 * L.image_bytes;
  const uint8_t* curr = prev + L.image_bytes;
  float nx = 0.f, ny = 0.f, e = 0.f;
  int st = 1;

  // the current image's (win + 1)^2 patch from (ix, iy) into s_img, rows dw apart
  auto stage_curr = [&](const uint8_t* J, int w, int h, int ix, int iy) {
    __syncthreads();  // the readers of what s_img held are done
    for (int k = lane; k < dw * dw; k += 64) {
      const int r = k / dw, c = k - r * dw;
      s_img[k] = J[(size_t)lk_reflect(iy + r, h) * w + lk_reflect(ix + c, w)];
    }
    __syncthreads();
  };
  auto sample_curr = [&](int idx, const LkWeights& W) {
    const int r = idx / win, c = idx - r * win;
    const uint8_t* q = s_img + r * dw + c;
    return lk_descale(q[0] * W.w00 + q[1] * W.w01 + q[dw] * W.w10 + q[dw + 1] * W.w11, LK_W_BITS - 5);
  };

  for (int lv = P.levels - 1; lv >= 0; --lv) {
    int w, h;
    lk_level_size(P.w, P.h, lv, &w, &h);
    const float scale = 1.f / (float)(1 << lv);
    float px = pt.x * scale, py = pt.y * scale;
    if (lv == P.levels - 1) {
      nx = px;
      ny = py;
    } else {
      nx = nx * 2.f;
      ny = ny * 2.f;
    }
    px -= half;
    py -= half;
    const int ipx = lk_floor(px), ipy = lk_floor(py);
    if (lk_outside(ipx, ipy, w, h, win)) {
      if (lv == 0) {
        st = 0;
        e = 0.f;
      }
      continue;
    }
    const LkWeights W = lk_weights(px, py, ipx, ipy);
    const uint8_t* I = prev + L.lvl_off[lv];
    const uint8_t* J = curr + L.lvl_off[lv];

    __syncthreads();
    for (int k = lane; k < pw * pw; k += 64) {  // coordinates ip - 1 .. ip + win + 1
      const int r = k / pw, c = k - r * pw;
      s_img[k] = I[(size_t)lk_reflect(ipy - 1 + r, h) * w + lk_reflect(ipx - 1 + c, w)];
    }
    __syncthreads();
    for (int k = lane; k < dw * dw; k += 64) {  // Scharr at ip .. ip + win
      const int r = k / dw, c = k - r * dw, x = ipx + c, y = ipy + r;
      int dx = 0, dy = 0;
      if (x >= 0 && x < w && y >= 0 && y < h) {
        const uint8_t* q = s_img + (r + 1) * pw + (c + 1);
        const int a00 = q[-pw - 1], a01 = q[-pw], a02 = q[-pw + 1], a10 = q[-1], a12 = q[1], a20 = q[pw - 1],
                  a21 = q[pw], a22 = q[pw + 1];
        dx = 3 * (a02 + a22 - a00 - a20) + 10 * (a12 - a10);
        dy = 3 * (a20 + a22 - a00 - a02) + 10 * (a21 - a01);
      }
      s_dx[k] = (short)dx;
      s_dy[k] = (short)dy;
    }
    __syncthreads();

    int Iv[PASSES], Ixv[PASSES], Iyv[PASSES];
    int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
      const int idx = lane + 64 * k;
      Iv[k] = Ixv[k] = Iyv[k] = 0;
      if (idx < nwin) {
        const int r = idx / win, c = idx - r * win;
        const uint8_t* q = s_img + (r + 1) * pw + (c + 1);
        const int d = r * dw + c;
        Iv[k] = lk_descale(q[0] * W.w00 + q[1] * W.w01 + q[pw] * W.w10 + q[pw + 1] * W.w11, LK_W_BITS - 5);
        Ixv[k] = lk_descale(s_dx[d] * W.w00 + s_dx[d + 1] * W.w01 + s_dx[d + dw] * W.w10 + s_dx[d + dw + 1] * W.w11,
                            LK_W_BITS);
        Iyv[k] = lk_descale(s_dy[d] * W.w00 + s_dy[d + 1] * W.w01 + s_dy[d + dw] * W.w10 + s_dy[d + dw + 1] * W.w11,
                            LK_W_BITS);
        s11 += Ixv[k] * Ixv[k];
        s12 += Ixv[k] * Iyv[k];
        s22 += Iyv[k] * Iyv[k];
      }
    }
    const float A11 = lk_scaled(lk_wave_sum(s11)), A12 = lk_scaled(lk_wave_sum(s12)),
                A22 = lk_scaled(lk_wave_sum(s22));
    float D = A11 * A22 - A12 * A12;
    const float min_eig =
        (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
    if ((double)min_eig < L.min_eig || D < FLT_EPSILON) {
      if (lv == 0) st = 0;
      continue;
    }
    D = 1.f / D;

    float qx = nx - half, qy = ny - half, pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < L.max_count; ++j) {
      const int iqx = lk_floor(qx), iqy = lk_floor(qy);
      if (lk_outside(iqx, iqy, w, h, win)) {
        if (lv == 0) st = 0;
        break;
      }
      const LkWeights Wq = lk_weights(qx, qy, iqx, iqy);
      stage_curr(J, w, h, iqx, iqy);
      int b1 = 0, b2 = 0;
#pragma unroll
      for (int k = 0; k < PASSES; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nwin) {
          const int diff = sample_curr(idx, Wq) - Iv[k];
          b1 += diff * Ixv[k];
          b2 += diff * Iyv[k];
        }
      }
      const float B1 = lk_scaled(lk_wave_sum(b1)), B2 = lk_scaled(lk_wave_sum(b2));
      const float dx = (A12 * B2 - A22 * B1) * D, dy = (A12 * B1 - A11 * B2) * D;
      qx += dx;
      qy += dy;
      nx = qx + half;
      ny = qy + half;
      if ((double)dx * (double)dx + (double)dy * (double)dy <= L.eps2) break;
      if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
        nx -= dx * 0.5f;
        ny -= dy * 0.5f;
        break;
      }
      pdx = dx;
      pdy = dy;
    }

    if (lv == 0 && st) {
      const float ex = nx - half, ey = ny - half;
      const int iex = lk_floor(ex), iey = lk_floor(ey);
      if (lk_outside(iex, iey, w, h, win)) {
        st = 0;
      } else {
        const LkWeights We = lk_weights(ex, ey, iex, iey);
        stage_curr(J, w, h, iex, iey);
        int sad = 0;
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
          const int idx = lane + 64 * k;
          if (idx < nwin) sad += abs(sample_curr(idx, We) - Iv[k]);
        }
        e = (float)lk_wave_sum(sad) / (float)(32 * win * win);
      }
    }
  }
  if (lane == 0) {
    const size_t o = (size_t)pi * K + i;
    kp1[o] = make_float2(nx, ny);
    status[o] = (uint8_t)st;
    err[o] = e;
  }
}

}  // namespace

int32_t lk_plan(const loam_lk_params* p, LkPlan* out) {
  if (!p || !out || p->max_width <= 0 || p->max_height <= 0 || p->win < 3 || p->win > LK_MAX_WIN ||
      p->win % 2 == 0 || p->max_level < 0 || p->max_level >= LK_MAX_LEVELS || !(p->epsilon == p->epsilon) ||
      !(p->min_eig_threshold == p->min_eig_threshold)) {
    set_error("loam_lk_params: sizes must be positive, win odd in 3..31, max_level in 0..7");
    return LOAM_ERR_ARG;
  }
  LkPlan L{};
  L.win = p->win;
  L.max_level = p->max_level;
  L.max_count = std::min(std::max(p->max_count, 0), 100);
  L.max_w = p->max_width;
  L.max_h = p->max_height;
  const double eps = std::min(std::max(p->epsilon, 0.0), 10.0);
  L.eps2 = eps * eps;
  L.min_eig = p->min_eig_threshold;
  size_t off = 0;
  for (int l = 0; l < LK_MAX_LEVELS; ++l) {
    int w, h;
    lk_level_size(L.max_w, L.max_h, l, &w, &h);
    L.lvl_off[l] = off;
    if (l <= L.max_level) off += ((size_t)w * h + 15) & ~(size_t)15;
  }
  L.image_bytes = off;
  *out = L;
  return LOAM_OK;
}

int32_t lk_launch(const LkPlan& plan, const LkPair* d_pairs, const LkPair* pairs, int n_pairs, uint8_t* d_pyr,
                  const float2* d_kp0, float2* d_kp1, uint8_t* d_status, float* d_err, int K, hipStream_t st) {
  LkDev L{};
  L.win = plan.win;
  L.max_count = plan.max_count;
  L.eps2 = plan.eps2;
  L.min_eig = plan.min_eig;
  for (int l = 0; l < LK_MAX_LEVELS; ++l) L.lvl_off[l] = plan.lvl_off[l];
  L.image_bytes = plan.image_bytes;
  int max_n = 0, levels = 0, w = 0, h = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (!pairs[p].active) continue;
    max_n = std::max(max_n, pairs[p].n);
    levels = std::max(levels, pairs[p].levels);
    w = std::max(w, pairs[p].w);
    h = std::max(h, pairs[p].h);
  }
  for (int l = 1; l < levels; ++l) {
    int lw, lh;
    lk_level_size(w, h, l, &lw, &lh);  // the level size grows with the image: this covers every pair
    const dim3 grid((lw + 63) / 64, (lh + 3) / 4, 2 * n_pairs);
    k_lk_pyr_down<<<grid, 256, 0, st>>>(d_pairs, d_pyr, L, l);
  }
  if (max_n > 0) {
    const dim3 grid(max_n, n_pairs);
    if (plan.win * plan.win <= 4 * 64)
      k_lk_track<4><<<grid, 64, 0, st>>>(d_pairs, d_pyr, L, d_kp0, d_kp1, d_status, d_err, K);
    else
      k_lk_track<16><<<grid, 64, 0, st>>>(d_pairs, d_pyr, L, d_kp0, d_kp1, d_status, d_err, K);
  }
  LOAM_HIP(hipGetLastError());
  return LOAM_OK;
}

}  // namespace loam

extern "C" void loam_lk_params_default(loam_lk_params* p) {
  if (!p) return;
  *p = loam_lk_params{};
  p->win = 15;
  p->max_level = 2;
  p->max_count = 10;
  p->epsilon = 0.03;
  p->min_eig_threshold = 1e-4;
}
