// depth_dev.h — the device view of a loam_depth handle and queryDepth as a device function,
// shared by depth.hip (k_dp_query) and vo_frames.hip (k_vo_assemble): both translation units
// compile the same body with -ffp-contract=off, so a depth is the same bits from either.
#pragma once
#include <cmath>

#include "common.h"

namespace loam {

struct DepthFrame {
  const float* xyz;  // input points (stride floats each)
  int n, stride;
  int active;
  int n_front, n_dnsp;
  int err;
};

struct DepthDev {
  int B, cap, W, H, nchunk;  // nchunk: chunks per stream (cap / DP_CHUNK)
  float grid;
  float A[16], Bm[16], C[12];  // cam_T_velo, rect0_T_cam, P_rect0 (row-major)
  DepthFrame* fr;
  float4* tmp;       // [B][cap] (u, v, depth, bucket as float bits or -1)
  int* chunk_cnt;    // [B][nchunk] front points per chunk -> offsets
  float4* p2d;       // [B][cap] point_cloud_2d (u, v, depth)
  int* bcnt;         // [B][W*H] bucket_count
  int* bstart;       // [B][W*H + 1] member list starts
  int* bfill;        // [B][W*H]
  int* bslot;        // [B][W*H] dnsp slot (occupied buckets)
  int* members;      // [B][cap] front rank of each bucketed point, grouped by bucket
  float* bx;         // [B][W*H]
  float* by;
  float* bd;
  float4* dnsp;      // [B][W*H]
};

// queryDepth (point_cloud_util.cpp:381-487) of image point (x, y) in stream s (0 <= s < D.B)
__device__ inline float dp_query_one(const DepthDev& D, int s, float x, float y, int radius) {
  const int WH = D.W * D.H;
  const int* bc = D.bcnt + (size_t)s * WH;
  const float *bx = D.bx + (size_t)s * WH, *by = D.by + (size_t)s * WH, *bd = D.bd + (size_t)s * WH;
  const int ix = static_cast<int>(x / D.grid), iy = static_cast<int>(y / D.grid);
  // the 3 nearest in gather order (a stable sort's first three), and the count
  float nd[3] = {INFINITY, INFINITY, INFINITY}, nz[3] = {0.f, 0.f, 0.f};
  int cnt = 0;
  for (int i = ix - radius; i <= ix + radius; ++i)
    for (int j = iy - radius; j <= iy + radius; ++j) {
      if (!(i >= 0 && i < D.W && j >= 0 && j < D.H)) continue;
      const int b = i * D.H + j;
      if (bc[b] <= 0) continue;
      ++cnt;
      // std::pow(float, int) promotes to double (:407)
      const double dx = (double)(x - bx[b]), dy = (double)(y - by[b]);
      const float dist = (float)sqrt(dx * dx + dy * dy);
      const float z = bd[b];
      if (dist < nd[2]) {
        if (dist < nd[1]) {
          nd[2] = nd[1];
          nz[2] = nz[1];
          if (dist < nd[0]) {
            nd[1] = nd[0];
            nz[1] = nz[0];
            nd[0] = dist;
            nz[0] = z;
          } else {
            nd[1] = dist;
            nz[1] = z;
          }
        } else {
          nd[2] = dist;
          nz[2] = z;
        }
      }
    }
  if (cnt < 10) return -1.0f;
  return (nz[0] * nd[1] * nd[2] + nz[1] * nd[0] * nd[2] + nz[2] * nd[0] * nd[1]) /
         (0.0001f + nd[1] * nd[2] + nd[0] * nd[2] + nd[0] * nd[1]);
}

// internal accessors of a loam_depth handle (depth.hip): its device arrays and device, and
// whether stream s holds the buckets of a loam_depth_process
int32_t depth_device_view(loam_depth* h, DepthDev* D, int* device);
bool depth_stream_processed(loam_depth* h, int s);

}  // namespace loam
