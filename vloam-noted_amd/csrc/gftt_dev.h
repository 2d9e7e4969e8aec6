// gftt_dev.h — Shi-Tomasi corner detection on an image that is already in device memory (gftt.hip).
#pragma once
#include "common.h"
#include "lk_dev.h"
#include "vo_frames_dev.h"

namespace loam {

constexpr int GF_MAX_BLOCK = 15;
constexpr int GF_MAX_DIM = 65535;          // a kept corner is packed as x | y << 16
constexpr int GF_MAX_CANDIDATES = 1 << 22;

// one image of a launch
struct GfPair {
  int active;  // 0: the pair is skipped
  int w, h;
  short side;  // 0: the previous image of the pair's pyramid slot, 1: the current one
  short dst;   // GF_TO_*: where the corners and their count go
};

// corners -> d_kp0, count -> n0, n1 and the tracker's n (a detect pair: its corners are tracked);
// corners -> d_kp0, count -> n0; corners -> d_kp1, count -> n1 (a match pair's two images)
enum { GF_TO_TRACKS = 0, GF_TO_KP0 = 1, GF_TO_KP1 = 2 };

// what the kernels leave per image
struct GfState {
  int max_enc;    // the largest eigenvalue, as an ordered int (gf_enc)
  int n_cand;     // candidates found (may exceed max_candidates: then none is selected)
  int n_corners;  // corners written
  int err;        // 1: a grid cell was full (impossible by the geometry; fails closed with 0 corners)
};

struct GfPlan {
  int max_corners, block, max_cand;
  int cand_pad;  // keys per image: max_cand rounded up to a power of two
  double quality, min_dist2;
  float k;       // (float)(scale * scale), scale = 1 / (4 * block * 255)
  int cell;      // cvRound(min_distance), 0: no suppression (min_distance < 1)
  int cell_cap;  // kept corners a cell can hold
  int max_w, max_h;
  size_t eig_stride;   // floats per image
  size_t cell_stride;  // cells per image
};

// checks the parameters (LOAM_ERR_ARG) and sizes the buffers for images up to max_w x max_h
int32_t gftt_plan(const loam_gftt_params* p, int max_keypoints, int max_w, int max_h, GfPlan* out);

struct GfBuffers {
  GfPair* gf;          // [pair] of this launch
  GfState* state;      // [pair] of this launch
  float* eig;          // [pair][eig_stride]
  uint64_t* keys;      // [pair][cand_pad]
  uint32_t* cells;     // [pair][cell_stride][cell_cap]
  int* cell_cnt;       // [pair][cell_stride]
};

// corners of every active image: level 0 of the pair's pyramid slot (d_pyr, image_bytes per
// pyramid) -> d_kp0 or d_kp1 ([pair][K], selection order), the count into d_pairs[pair].n0 / n1 and
// d_lk[pair].n, as the image's dst says.  Launches on one stream may share B's scratch (eig, keys,
// cells); each needs its own gf and state.  Enqueues only, never waits.
int32_t gftt_launch(const GfPlan& plan, const GfBuffers& B, const GfPair* pairs, int n_pairs, const uint8_t* d_pyr,
                    size_t image_bytes, float2* d_kp0, float2* d_kp1, int K, VfPair* d_pairs, LkPair* d_lk,
                    hipStream_t st);

}  // namespace loam
