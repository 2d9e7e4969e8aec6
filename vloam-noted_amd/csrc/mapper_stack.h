// mapper_stack.h — the stack VoxelGrids (laser_mapping.cpp:492-500): k_stack_ds / _part / _cat / _done / _counts.
// Part of the mapper.hip translation unit: included there only, in the order the phases run.
#pragma once

namespace loam {

// PCL-order VoxelGrid (voxel_pcl.h) in a VX_THREADS workgroup owning the whole LDS: the sort's
// level lists in LDS (inputs up to ~115k points); the elements E and the stop lists A / B in LDS
// too for inputs up to MP_LDS_N points (the sort's dependent accesses are LDS latency, not L2),
// else at offset `so` of the (stream, map) sort scratch, where the sorted copy S always goes.
// Returns false (MAP_ERR_SORT) when the input is too large for the lists.
constexpr int MP_LDS_N = 8192;                                    // E 64 KiB + A, B 32 KiB each
constexpr int MP_LEV_W = 40;  // SsLevels words
static_assert(sizeof(SsLevels) <= 4 * MP_LEV_W, "SsLevels area");
constexpr int MP_SEG_LDS = (VX_LDS_WORDS - VX_TAIL_WORDS - 2 * MP_LEV_W - 4 * MP_LDS_N) / 6;  // level lists beside them
static_assert(MP_SEG_LDS >= MP_LDS_N / (SS_THRESHOLD + 1) + 2, "level lists of an LDS-resident sort");
static_assert(VX_THREADS / 64 * SS_LOC_WORDS + VX_TAIL_WORDS + 2 * MP_LEV_W <= VX_LDS_WORDS, "wave-local sort buffers");
// global-memory sorts: segments of at most MP_LDS_N elements are sorted whole in LDS
// (ss_sort_deferred: E, A, B and the level lists of one segment at a time)
constexpr int MP_DEF_SEG = MP_LDS_N / (SS_THRESHOLD + 1) + 2;
static_assert(4 * MP_LDS_N + 6 * MP_DEF_SEG + VX_TAIL_WORDS + 2 * MP_LEV_W <= VX_LDS_WORDS, "deferred segment sort in LDS");
// sort scratch of a (stream, map), mp_scratch elements: the cubes' blocks of n + MP_SLACK from 0
// (the frame's hot_tail), below the stack's (its own region: it may run beside the previous
// frame's re-filter) at mp_stack_offset
constexpr uint32_t MP_SLACK = 64;
__host__ __device__ inline size_t mp_cube_scratch(const MapperDev& D) { return (size_t)D.scratch_cap + MP_SLACK * (INS_SLOTS + 1); }
__host__ __device__ inline uint32_t mp_stack_offset(const MapperDev& D) { return (uint32_t)mp_cube_scratch(D); }
__host__ __device__ inline size_t mp_scratch(const MapperDev& D) { return mp_cube_scratch(D) + (size_t)D.max_in + MP_SLACK; }
// D.pseg (a global-memory sort's level and deferred lists): the ints before element offset off of
// the sort scratch, 9 per 16 elements; a (stream, map) has mp_pseg(ps) + 9
template <typename T>
__host__ __device__ inline T mp_pseg(T off) { return 9 * (off / 16); }
template <typename PF>
__device__ inline bool map_voxel_pcl(const MapperDev& D, size_t sm, uint32_t so, const PF& P, int n, float leaf,
                                     const VxPclOut& O, uint32_t* lds, int* err) {
  const size_t ps = mp_scratch(D);
  const bool stk = so == mp_stack_offset(D);
  const size_t lim = stk ? ps : mp_cube_scratch(D);  // cubes stay below the stack
  if ((size_t)so + (uint32_t)n + MP_SLACK > lim) {
    if (threadIdx.x == 0) atomicOr(err, MAP_ERR_SORT);
    return false;
  }
  VxMisc& M = vx_misc(lds);
  uint32_t* ws = vx_ws(lds);
  SsLevels* lev = reinterpret_cast<SsLevels*>(lds + VX_LDS_WORDS - VX_TAIL_WORDS - MP_LEV_W);
  const size_t b = sm * ps + so;
  // the counters of the stack's or the cubes' sorts
  auto slot = [&](int stack, int cube) { return D.pdbg ? (stk ? D.pdbg + stack : D.pdbg + cube) : nullptr; };
  unsigned long long *prof = slot(MD_STACK_SEG, MD_CUBE_SEG), *heap = slot(MD_STACK_HEAP, MD_CUBE_HEAP),
                     *glob = slot(MD_STACK_GLOB, MD_CUBE_GLOB);
  if (n <= MP_LDS_N) {
    uint64_t* E = reinterpret_cast<uint64_t*>(lds);
    uint32_t* A = lds + 2 * MP_LDS_N;
    uint32_t* B = A + MP_LDS_N;
    int* seg0 = reinterpret_cast<int*>(B + MP_LDS_N);
    const VxPclScratch X{E, A, B, D.ps + b, lev, {seg0, seg0 + 3 * MP_SEG_LDS}, MP_SEG_LDS, nullptr, prof, heap, glob};
    voxel_grid_pcl<VX_THREADS>(P, n, leaf, O, X, M, ws, err);
  } else {  // level lists in global memory; segments that fit the LDS are sorted there whole
    const int cap = (int)((n + MP_SLACK) / 16);
    int* seg0 = D.pseg + sm * (mp_pseg(ps) + 9) + mp_pseg(so);
    int* dseg = reinterpret_cast<int*>(lds + 4 * MP_LDS_N);
    const VxPclDefer dfr{MP_LDS_N, seg0 + 6 * cap, cap, reinterpret_cast<uint64_t*>(lds), lds + 2 * MP_LDS_N,
                         lds + 3 * MP_LDS_N, dseg, dseg + 3 * MP_DEF_SEG, MP_DEF_SEG,
                         reinterpret_cast<SsLevels*>(lds + VX_LDS_WORDS - VX_TAIL_WORDS - 2 * MP_LEV_W)};
    const VxPclScratch X{D.pe + b, D.pa + b, D.pb + b, D.ps + b, lev, {seg0, seg0 + 3 * cap}, cap, lds, prof, heap, glob};
    voxel_grid_pcl<VX_THREADS, true>(P, n, leaf, O, X, M, ws, err, &dfr);
  }
  return true;
}

// exact order (voxel_hot.h): the hot records of a filter of n points in the (stream, map) sort
// scratch at offset so (a block of n + MP_SLACK): rk in pa, fpos in pb, the member lists and the
// per-voxel records in pe (2 (n + MP_SLACK) words)
__device__ inline VxHot map_hot(const MapperDev& D, size_t sm, uint32_t so, uint32_t n) {
  const size_t b = sm * mp_scratch(D) + so;
  uint32_t* hl = reinterpret_cast<uint32_t*>(D.pe + b);
  return VxHot{D.pa + b, hl, hl + n, D.pb + b, n / 3 + 1, D.ps + b};  // (w: sorts of VH_MAX_N .. VH_BIG_N points)
}

__device__ inline VxPclOut map_pcl_out(const VoxSeg& S, uint32_t reuse_off, uint32_t reuse_cnt) {
  return VxPclOut{S.out, S.tail, S.cap, S.res_off, S.res_cnt, S.stable_out, reuse_off, reuse_cnt};
}
// The exact-order ladder of the filter S (S.src1 used whole; S.hot = map_hot of its sort-scratch
// block at offset so) of a (stream, map): up to VH_BIG_N points vx_filter_exact (the merge when
// `fixed`; merged: it ran); above, or when vh_fixup cannot split the sort for the LDS (he < 0), the
// whole std::sort in global memory on the points P.  entry: a cube's table entry (the stack: null).
template <typename PF>
__device__ __attribute__((always_inline)) inline void map_filter_exact(
    const MapperDev& D, size_t sm, uint32_t so, const VoxSeg& S, const PF& P, uint32_t* lds,
    const uint2* entry = nullptr, bool fixed = false, bool* merged = nullptr) {
  const uint32_t n = (uint32_t)(S.n0 + S.n1);
  bool global = n > (uint32_t)VH_BIG_N;
  uint32_t reuse_off = 0xFFFFFFFFu, reuse_cnt = 0;
  if (!global) {
    if (entry && (size_t)so + n + MP_SLACK > mp_cube_scratch(D)) {
      if (threadIdx.x == 0) atomicOr(S.err, MAP_ERR_SORT);  // (only cubes: the stack's block holds max_in)
    } else {
      auto slot = [&](int stack, int cube) { return D.pdbg ? D.pdbg + (entry ? cube : stack) : nullptr; };
      const VhDiag C{slot(MD_STACK_HOT, MD_CUBE_HOT), slot(MD_STACK_SORT, MD_CUBE_SORT),
                     entry && D.pdbg ? D.pdbg + MD_CUBE_WAVES : nullptr};
      int he;
      if constexpr (std::is_same<PF, VxSrc>::value) he = vx_filter_exact<VX_THREADS>(S, P, (int)n, lds, S.stable_out, S.err, C, fixed, merged);
      else he = vx_filter_exact<VX_THREADS>(S, VxSrc{S.src0, S.n0, S.src1}, (int)n, lds, S.stable_out, S.err, C, fixed, merged);
      global = he < 0;
      __syncthreads();
      // the global sort writes a cube again, into the block the filter allocated (the entry, written before
      // the barrier).  Also after VX_ERR_OUTPUT, when the entry is the old content's: that fix is a change of its own
      if (global && entry) reuse_off = entry->x, reuse_cnt = entry->y;
    }
  }
  if (global) map_voxel_pcl(D, sm, so, P, (int)n, S.leaf, map_pcl_out(S, reuse_off, reuse_cnt), lds, S.err);
}

// ---------------------------------------------------------------------------------------
// VoxelGrid of the incoming feature clouds -> CornerStack / SurfStack (:492-500)
// ---------------------------------------------------------------------------------------
// one 1024-thread workgroup per (stream, map): grid B * 2
template <bool PCL>
__global__ void __launch_bounds__(VX_THREADS) k_stack_ds(MapperDev D) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[VX_LDS_WORDS];
  const int s = D.s0 + (blockIdx.x >> 1), m = blockIdx.x & 1;
  const StackIn& I = D.sin[s];
  if (!I.active) return;
  const size_t sm = sm_index(s, m);
  int* err = &D.stk_err[s];
  VoxSeg S{};  // (no secondary source, tail or offset word)
  S.leaf = D.leaf[m];
  S.err = err;
  S.prof_seg = D.pdbg ? D.pdbg + MD_STACK_SEG : nullptr;  // stack VoxelGrid phases
  S.src0 = I.p[m];
  S.n0 = I.n[m];
  S.out = D.stack[m] + (size_t)s * D.max_in;
  S.cap = D.max_in;
  S.res_cnt = reinterpret_cast<uint32_t*>(&D.stk_n[2 * s + m]);
  S.scratch_pts = D.stk_pts + sm * D.max_in;
  S.scratch_idx = D.stk_idx + sm * D.max_in;
  S.scratch_cap = D.max_in;
  if (PCL) S.hot = map_hot(D, sm, mp_stack_offset(D), (uint32_t)I.n[m]);  // PCL's summation order
  if (PCL) map_filter_exact(D, sm, mp_stack_offset(D), S, VxPtrSrc{I.p[m]}, lds);
  else voxel_segment(S, lds);
}

// Few streams: the input-order stack VoxelGrid of a (stream, map) over stack_k workgroups.
// Every workgroup computes the same geometry and idx histogram (VX_NB buckets) from all the
// points, cuts the idx range into stack_k ranges of about equal point counts, and filters its
// own range (vx_group: hash, sorted unique voxels, member lists in input order, centroids) into
// the (stream, map) staging area at the point-count prefix of its range.  k_stack_cat then
// concatenates the ranges in idx order.  Same voxels, same member order, same sums: the bits of
// the one-workgroup filter.
constexpr int STACK_K_MAX = 16;
__global__ void __launch_bounds__(VX_THREADS) k_stack_part(MapperDev D) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[VX_LDS_WORDS];
  const int K = D.stack_k;
  const int j = blockIdx.x % K, pm = blockIdx.x / K;
  const int s = D.s0 + (pm >> 1), m = pm & 1;
  const StackIn& I = D.sin[s];
  if (!I.active) return;
  const size_t sm = sm_index(s, m);
  uint2* part = D.stk_part + sm * STACK_K_MAX;
  const uint32_t N = (uint32_t)I.n[m];
  const VxSrc P{I.p[m], (int)N, nullptr};
  float4* stage = D.stk_pts + sm * D.max_in;
  uint32_t* ws = vx_ws(lds);
  VxMisc& M = vx_misc(lds);
  const int tid = threadIdx.x;
  if (N == 0) {
    if (tid == 0) part[j] = make_uint2(0, 0);
    return;
  }
  unsigned long long tp = __builtin_readcyclecounter();  // phase counters (diagnostics)
  vx_geometry(P, N, D.leaf[m], M);
  vx_phase(D.pdbg ? D.pdbg + MD_STACK_SEG : nullptr, 0, &tp);  // bounding box (summed over the K parts)
  const VxGeom g = M.g;
  if (g.overflow) {  // PCL: "Leaf size is too small" -> output = input (range 0 copies it)
    if (j == 0)
      for (uint32_t i = tid; i < N; i += VX_THREADS) stage[i] = P(i);
    if (tid == 0) part[j] = make_uint2(0, j == 0 ? N : 0u);
    return;
  }
  // idx histogram -> the ranges' bucket cuts by cumulative point count
  uint32_t* hist = lds + VX_HIST_WORD;
  // bucket(k) = floor(k mulc / 2^32) with mulc = floor(2^32 VX_NB / V): monotone in k and below
  // VX_NB for k < V, and a multiply instead of a 64-bit division per point (the histogram pass
  // spent most of its cycles in the division); blo(b) = ceil(b 2^32 / mulc) is its exact inverse
  // (the first key of bucket b), so the parts still cut the idx range at key boundaries
  const unsigned long long V = g.nvox;
  const unsigned long long mulc = (((unsigned long long)VX_NB) << 32) / V;
  auto bucket = [&](uint32_t k) { return (uint32_t)(((unsigned long long)k * mulc) >> 32); };
  auto blo = [&](uint32_t b) { return (uint32_t)((((unsigned long long)b << 32) + mulc - 1) / mulc); };
  for (int b = tid; b < VX_NB; b += VX_THREADS) hist[b] = 0;
  __syncthreads();
  // loads in flight together; the scan's points come in ring order, so a wave's lanes (consecutive
  // points) mostly fall in one bucket: each run of equal buckets adds its length with one LDS
  // atomic by its first lane (same-address atomics of a wave serialise).  Wave-uniform loop.
  {
    const int lane = tid & 63;
    const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    for (uint32_t ib = (uint32_t)(tid & ~63); ib < N; ib += VX_UNROLL * VX_THREADS) {
      uint32_t kk4[VX_UNROLL];
      vx_keys4(g, P, N, ib + lane, kk4);
#pragma unroll
      for (int u = 0; u < VX_UNROLL; ++u) {
        const uint32_t bk = kk4[u] != VX_EMPTY ? bucket(kk4[u]) : 0xFFFFFFFFu;
        const uint32_t prev = (uint32_t)__shfl_up((int)bk, 1, 64);
        const uint64_t starts = __ballot(lane == 0 || prev != bk);
        if (bk != 0xFFFFFFFFu && ((starts >> lane) & 1ull)) {
          const uint64_t after = starts & ~le;
          atomicAdd(&hist[bk], (uint32_t)((after ? __ffsll((long long)after) - 1 : 64) - lane));
        }
      }
    }
  }
  __syncthreads();
  // range r starts at the first bucket whose points-before count reaches r N / K: a block scan
  // of the histogram (two buckets per thread) and a test at every bucket
  static_assert(VX_NB == 2 * VX_THREADS, "two buckets per thread");
  const uint32_t h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
  uint32_t tot;
  const uint32_t a0 = vx_block_scan(h0 + h1, ws, &tot), a1 = a0 + h0;  // points before buckets 2t, 2t+1
  const uint64_t thr0 = (uint64_t)j * N / K, thr1 = (uint64_t)(j + 1) * N / K;
  if (tid == 0) {
    M.sbase[0] = j == 0 ? 0u : (uint32_t)VX_NB;
    M.sbase[1] = j == K - 1 ? (uint32_t)VX_NB : (uint32_t)VX_NB;
    M.sfail = j == 0 ? 0 : (int)N;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const uint32_t bb = 2 * tid + u, acc = u ? a1 : a0, prev = u ? a0 : a0 - (tid ? hist[2 * tid - 1] : 0u);
    const bool first = bb == 0;
    if (j > 0 && acc >= thr0 && (first || prev < thr0)) {
      M.sbase[0] = bb;
      M.sfail = (int)acc;
    }
    if (j < K - 1 && acc >= thr1 && (first || prev < thr1)) M.sbase[1] = bb;
  }
  __syncthreads();
  const uint32_t b0 = M.sbase[0], b1 = max(M.sbase[0], M.sbase[1]), base = (uint32_t)M.sfail;
  __syncthreads();  // vx_group reuses M
  vx_phase(D.pdbg ? D.pdbg + MD_STACK_CUTS : nullptr, 0, &tp);  // histogram + range cuts
  if (b0 >= b1) {  // empty range
    if (tid == 0) part[j] = make_uint2(base, 0);
    return;
  }
  VoxSeg S{};  // (no secondary source, tail or result words)
  S.src0 = I.p[m];
  S.n0 = (int)N;
  S.leaf = D.leaf[m];
  S.out = stage;
  S.cap = (uint32_t)D.max_in;
  S.scratch_idx = D.stk_idx + sm * D.max_in;
  S.scratch_cap = (uint32_t)D.max_in;
  S.err = &D.stk_err[s];
  S.prof_seg = D.pdbg ? D.pdbg + MD_STACK_SEG : nullptr;  // hash, sort + scan, members + centroids
  int moved = 0;
  const uint32_t klo = blo(b0), khi = b1 >= (uint32_t)VX_NB ? 0xFFFFFFFFu : blo(b1);
  const uint32_t U = vx_group(S, g, P, N, D.stk_idx + sm * D.max_in + base, klo, khi, base,
                              VX_LDS_WORDS - VX_TAIL_WORDS, lds, ws, M, &moved);
  if (tid == 0) {
    if (U == VX_OVERFLOW) atomicOr(&D.stk_err[s], MAP_ERR_STACK);
    part[j] = make_uint2(base, U == VX_OVERFLOW ? 0u : U);
  }
}

// the ranges of k_stack_part in idx order -> the stack and its count
__global__ void __launch_bounds__(VX_THREADS) k_stack_cat(MapperDev D) {
  const int s = D.s0 + (blockIdx.x >> 1), m = blockIdx.x & 1;
  if (!D.sin[s].active) return;
  const size_t sm = sm_index(s, m);
  const uint2* part = D.stk_part + sm * STACK_K_MAX;
  const float4* stage = D.stk_pts + sm * D.max_in;
  float4* out = D.stack[m] + (size_t)s * D.max_in;
  uint32_t o = 0;
  for (int j = 0; j < D.stack_k; ++j) {
    const uint2 pj = part[j];
    for (uint32_t i = threadIdx.x; i < pj.y; i += VX_THREADS) out[o + i] = stage[pj.x + i];
    o += pj.y;
  }
  if (threadIdx.x == 0) D.stk_n[2 * s + m] = (int)o;
}

// LaserMapping::input's initial guess (laser_mapping.cpp:206-207): pose = wmap (x) wodom
__host__ __device__ inline void pose_initial_guess(const double* wmap, const double* wodom, double* pose) {
  const dq qm{wmap[0], wmap[1], wmap[2], wmap[3]};
  const dq qo{wodom[0], wodom[1], wodom[2], wodom[3]};
  const dq q = qmul(qm, qo);
  const d3 r = qrot(qm, d3{wodom[4], wodom[5], wodom[6]});
  pose[0] = q.x; pose[1] = q.y; pose[2] = q.z; pose[3] = q.w;
  pose[4] = r.x + wmap[4];
  pose[5] = r.y + wmap[5];
  pose[6] = r.z + wmap[6];
}

// LaserMapping::transformUpdate (laser_mapping.cpp:147-151): wmap = pose (x) wodom^-1
__host__ __device__ inline void pose_transform_update(const double* pose, const double* wodom, double* wmap) {
  const dq qw{pose[0], pose[1], pose[2], pose[3]};
  const dq qo{wodom[0], wodom[1], wodom[2], wodom[3]};
  const dq qm = qmul(qw, qinv(qo));
  const d3 r = qrot(qm, d3{wodom[4], wodom[5], wodom[6]});
  wmap[0] = qm.x; wmap[1] = qm.y; wmap[2] = qm.z; wmap[3] = qm.w;
  wmap[4] = pose[4] - r.x;
  wmap[5] = pose[5] - r.y;
  wmap[6] = pose[6] - r.z;
}

// centerCube and the recentering count (laser_mapping.cpp:228-251): the window centre of a pose
// and how far the grid must shift (cen follows the shift); true if it shifts
__host__ __device__ inline bool frame_center(const double* pose, int* cen, int* center, int* shift) {
  const int dims[3] = {CW, CH, CD};
  bool any = false;
  for (int a = 0; a < 3; ++a) {
    int c = cube_of(pose[4 + a], cen[a]);
    shift[a] = 0;
    while (c < 3) { c++; cen[a]++; shift[a]++; }
    while (c >= dims[a] - 3) { c--; cen[a]--; shift[a]--; }
    center[a] = c;
    any |= shift[a] != 0;
  }
  return any;
}

// the window cubes (laserCloudValidInd, :455-472) and the cell-hash origin of F.center / F.cen
__host__ __device__ inline void frame_window(StreamFrame& F) {
  const int* c3 = F.center;
  int vn = 0;
  for (int i = c3[0] - 2; i <= c3[0] + 2; i++)
    for (int j = c3[1] - 2; j <= c3[1] + 2; j++)
      for (int k = c3[2] - 1; k <= c3[2] + 1; k++)
        if (i >= 0 && i < CW && j >= 0 && j < CH && k >= 0 && k < CD) F.window[vn++] = i + CW * j + CW * CH * k;
  F.valid_num = vn;
  // hash cell origin: world metres of the window's low corner, minus a 2-cell margin
  F.origin[0] = (c3[0] - 2 - F.cen[0]) * 50 - 25 - 2;
  F.origin[1] = (c3[1] - 2 - F.cen[1]) * 50 - 25 - 2;
  F.origin[2] = (c3[2] - 1 - F.cen[2]) * 50 - 25 - 2;
}

// per-frame resets of a stream record (the host's, or k_frame_prep's for a queued frame)
__host__ __device__ inline void frame_reset(StreamFrame& F) {
  F.shift[0] = F.shift[1] = F.shift[2] = 0;
  F.err = 0;
  F.nc_stack = F.ns_stack = 0;
  F.corner_num[0] = F.corner_num[1] = F.surf_num[0] = F.surf_num[1] = 0;
  F.sub_n[0] = F.sub_n[1] = 0;
  F.optimize = 0;
  F.cand[0] = F.cand[1] = 0;
}

// the frame's stack sizes and stack-filter errors into its stream records (after the stack
// kernels, which may have run while the previous frame was in flight)
// (agent-scope atomic loads: k_frame_prep reads them while other stacks of the same frame may
// still be running, and the words of all streams share lines that another stream's block of this
// XCD may have pulled into the L2 before this stack was written; an acquire fence instead would
// invalidate the XCD's whole L2 and cost the frame's later kernels their cached cubes)
__device__ inline void stack_counts(const MapperDev& D, int s, StreamFrame& F) {
  F.nc_stack = __hip_atomic_load(&D.stk_n[2 * s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  F.ns_stack = __hip_atomic_load(&D.stk_n[2 * s + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int e = __hip_atomic_load(&D.stk_err[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (e) {
    F.err |= e;
    __hip_atomic_store(&D.stk_err[s], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// after a stack launch on the stack stream: its number (agent scope); k_frame_prep
// waits for it on the device (a cross-stream event wait between two graph launches, pending when
// enqueued, costs ~5 us of the device's time, tools/mb_flush.hip)
__global__ void k_stack_done(unsigned long long* w, unsigned long long v) {
  // (the stack kernels before it on this stream ended with their own release: a relaxed store,
  // no L2 write-back here)
  if (threadIdx.x == 0) __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_stack_counts(MapperDev D) {
  const int s = D.s0 + blockIdx.x;
  StreamFrame& F = D.fr[s];
  if (threadIdx.x != 0 || !F.active) return;
  stack_counts(D, s, F);
}

}  // namespace loam
