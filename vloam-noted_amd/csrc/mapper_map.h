// mapper_map.h — the map: insertion, re-VoxelGrid, cube cell index, compaction, publish kernels.
// Part of the mapper.hip translation unit: included there only, in the order the phases run.
#pragma once

namespace loam {

// which cube (if any) slot `slot` of (s, m) re-filters this frame; false: nothing to do.  A
// window cube that received nothing and whose content is a VoxelGrid fixed point keeps it:
// re-filtering it (laser_mapping.cpp:795-808) would reproduce it bit for bit.
__device__ inline bool revox_target(const MapperDev& D, int s, int m, int slot, int* cube_out, int* append_out) {
  const StreamFrame& F = D.fr[s];
  if (!F.active) return false;
  int cube, append;
  if (slot < F.valid_num) {
    cube = F.window[slot];
    append = 0;
  } else if (slot >= WIN_VALID_MAX && slot - WIN_VALID_MAX < min(F.extra_n[m], EXTRA_CAP)) {
    cube = F.extra_list[m][slot - WIN_VALID_MAX];
    append = 1;
  } else {
    return false;
  }
  const uint32_t* ioff = D.ins_off + sm_index(s, m) * (INS_SLOTS + 1);
  const uint32_t n_new = ioff[slot + 1] - ioff[slot];
  const uint2 cv = D.cube_tab[sm_index(s, m) * NCUBE + cube];
  if (!append && n_new == 0 && (cv.y == 0 || D.stable_tok[sm_index(s, m) * NCUBE + cube] == cv.x + 1))
    return false;
  *cube_out = cube;
  *append_out = append;
  return true;
}

// ---------------------------------------------------------------------------------------
// insertion of the stacks into the cube grid with the final pose (laser_mapping.cpp:741-788),
// then the inserted points grouped by target cube (stable counting sort); one workgroup per
// (stream, map): each re-VoxelGrid workgroup then reads one contiguous run, in input order
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VX_THREADS) k_insert_bucket(MapperDev D) {
  __shared__ int cslot[NCUBE];
  __shared__ uint32_t base[INS_SLOTS];
  __shared__ uint32_t wcnt[VX_WAVES][INS_SLOTS];
  const int sm = 2 * D.s0 + blockIdx.x, s = sm >> 1, m = sm & 1;
  StreamFrame& F = D.fr[s];
  if (!F.active) return;
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int n = m == 0 ? F.nc_stack : F.ns_stack;
  {
    // insertion of the stack into the cube grid with the final pose (laser_mapping.cpp:741-788):
    // the map-frame point and its cube; cubes outside the window that receive points are listed
    double X[7];
    for (int i = 0; i < 7; ++i) X[i] = F.pose[i];
    // transformUpdate (:147-151) for a frame queued behind this one (k_frame_prep); the host
    // computes the same at the end of the frame
    if (m == 0 && tid == 0) pose_transform_update(X, F.wodom, F.wmap);
    const int c0 = F.center[0], c1 = F.center[1], c2 = F.center[2];
    const int e0 = F.cen[0], e1 = F.cen[1], e2 = F.cen[2];
    const uint32_t epoch = F.epoch;
    // the stack points INS_LOADS at a time from a clamped index, all in flight before the first is
    // transformed (a load per loop trip is one memory latency per trip)
    constexpr int INS_LOADS = 4;
    const float4* stk = D.stack[m] + (size_t)s * D.max_in;
    for (int i0 = tid; i0 < n; i0 += INS_LOADS * VX_THREADS) {
      float4 q[INS_LOADS];
#pragma unroll
      for (int u = 0; u < INS_LOADS; ++u) q[u] = stk[min(i0 + u * VX_THREADS, n - 1)];
#pragma unroll
      for (int u = 0; u < INS_LOADS; ++u) {
        const int i = i0 + u * VX_THREADS;
        if (i >= n) break;
        const float4 sel = to_map(X, q[u]);
        const int ci = cube_of(sel.x, e0), cj = cube_of(sel.y, e1), ck = cube_of(sel.z, e2);
        int tag = -1;
        // sharded: only the owner of the point's 4 m block stores it (comm.h)
        const bool mine = !D.sharded || shard_owner(sel.x, sel.y, sel.z, 1.0f / D.leaf[m], D.blk_v[m], D.nrank) == D.rank;
        if (mine && ci >= 0 && ci < CW && cj >= 0 && cj < CH && ck >= 0 && ck < CD) {
          tag = ci + CW * cj + CW * CH * ck;
          const bool in_window = ci >= c0 - 2 && ci <= c0 + 2 && cj >= c1 - 2 && cj <= c1 + 2 && ck >= c2 - 1 && ck <= c2 + 1;
          if (!in_window) {
            uint32_t* fl = D.extra_flag + sm_index(s, m) * NCUBE + tag;
            if (atomicExch(fl, epoch) != epoch) {
              int e = atomicAdd(&F.extra_n[m], 1);
              if (e < EXTRA_CAP) F.extra_list[m][e] = tag;
              else atomicOr(&F.err, MAP_ERR_EXTRA);
            }
          }
        }
        const size_t o = sm_index(s, m) * D.max_in + i;
        D.ins_pts[o] = sel;
        D.ins_tag[o] = tag;
      }
    }
    __syncthreads();  // the points, tags and the out-of-window list, for the grouping below
  }
  // group the inserted points by target cube (stable counting sort): each re-VoxelGrid
  // workgroup then reads one contiguous run, in input order
  const int* tag = D.ins_tag + sm_index(s, m) * D.max_in;
  const float4* pts = D.ins_pts + sm_index(s, m) * D.max_in;
  float4* out = D.ins_sorted + sm_index(s, m) * D.max_in;
  uint32_t* off = D.ins_off + sm_index(s, m) * (INS_SLOTS + 1);
  for (int c = tid; c < NCUBE; c += VX_THREADS) cslot[c] = -1;
  for (int k = tid; k < INS_SLOTS; k += VX_THREADS) base[k] = 0;
  __syncthreads();
  const int vn = F.valid_num, ne = min(F.extra_n[m], EXTRA_CAP);
  if (tid < vn) cslot[F.window[tid]] = tid;
  if (tid < ne) cslot[F.extra_list[m][tid]] = WIN_VALID_MAX + tid;
  // this thread's slot (tid < INS_SLOTS) for the re-VoxelGrid list below: its cube's table entry and
  // token are loaded now, their latency hidden behind the grouping (the revox_target test)
  int my_cube = -1;
  if (tid < vn) my_cube = F.window[tid];
  else if (tid >= WIN_VALID_MAX && tid < WIN_VALID_MAX + ne) my_cube = F.extra_list[m][tid - WIN_VALID_MAX];
  uint2 my_cv = make_uint2(0u, 0u);
  uint32_t my_tok = 0u;
  if (my_cube >= 0) {
    my_cv = D.cube_tab[sm_index(s, m) * NCUBE + my_cube];
    my_tok = D.stable_tok[sm_index(s, m) * NCUBE + my_cube];
  }
  __syncthreads();
  for (int i = tid; i < n; i += VX_THREADS) {
    const int t = tag[i];
    const int sl = t >= 0 ? cslot[t] : -1;
    if (sl >= 0) atomicAdd(&base[sl], 1u);
  }
  __syncthreads();
  const uint32_t my_new = tid < INS_SLOTS ? base[tid] : 0u;  // points inserted into this slot's cube
  __syncthreads();  // (every count read before the scan below rewrites base)
  if (wid == 0) {  // exclusive scan of the slot counts by one wave: lane l owns slots l*PL ..
    constexpr int PL = (INS_SLOTS + 63) / 64;
    uint32_t c[PL], sum = 0;
#pragma unroll
    for (int u = 0; u < PL; ++u) {
      const int k = lane * PL + u;
      c[u] = k < INS_SLOTS ? base[k] : 0u;
      sum += c[u];
    }
    uint32_t x = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    uint32_t acc = x - sum;
#pragma unroll
    for (int u = 0; u < PL; ++u) {
      const int k = lane * PL + u;
      if (k < INS_SLOTS) {
        base[k] = acc;
        off[k] = acc;
      }
      acc += c[u];
    }
    if (lane == 63) off[INS_SLOTS] = x;
  }
  __syncthreads();
  // software pipeline: the next chunk's tag and point are loaded while this chunk is grouped
  int t_next = tid < n ? tag[tid] : -1;
  float4 p_next = tid < n ? pts[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = 0; c0 < n; c0 += VX_THREADS) {
    const int i = c0 + tid;
    const int t = t_next;
    const float4 p_cur = p_next;
    t_next = -1;  // (past the end: no point)
    if (i + VX_THREADS < n) {
      t_next = tag[i + VX_THREADS];
      p_next = pts[i + VX_THREADS];
    }
    const int sl = t >= 0 ? cslot[t] : -1;
    for (int k = tid; k < VX_WAVES * INS_SLOTS; k += VX_THREADS) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    // rank among the lanes of this wave with the same slot (peel one slot value per pass)
    uint32_t rank = 0;
    bool pending = sl >= 0;
    while (true) {
      const uint64_t live = __ballot(pending);
      if (!live) break;
      const int leader = __ffsll((unsigned long long)live) - 1;
      const int lsl = __shfl(sl, leader, 64);
      const bool mine = pending && sl == lsl;
      const uint64_t mk = __ballot(mine);
      if (mine) {
        rank = __popcll(mk & lanemask_lt());
        pending = false;
      }
      if (lane == 0) wcnt[wid][lsl] = __popcll(mk);
    }
    __syncthreads();
    if (tid < INS_SLOTS) {  // wave prefix per slot, advance the slot base
      uint32_t acc = base[tid];
      for (int w = 0; w < VX_WAVES; ++w) {
        const uint32_t c = wcnt[w][tid];
        wcnt[w][tid] = acc;
        acc += c;
      }
      base[tid] = acc;
    }
    __syncthreads();
    if (sl >= 0) out[wcnt[wid][sl] + rank] = p_cur;
    __syncthreads();
  }
  // this (stream, map)'s re-VoxelGrid items, listed by size class (k_revox takes the largest
  // first); the test is revox_target's: a window cube that received nothing and holds fixed-point
  // (or no) content is skipped
  static_assert(INS_SLOTS <= VX_THREADS, "one thread per slot");
  if (my_cube >= 0) {
    const bool append = tid >= WIN_VALID_MAX;
    if (append || my_new != 0 || (my_cv.y != 0 && my_tok != my_cv.x + 1)) {
      const uint32_t nt = my_cv.y + my_new;
      const int c = nt < 1024u ? 0 : min(RQ_CLASSES - 1, 32 - __clz(nt >> 10));
      const uint32_t k = atomicAdd(&D.rq_ctl[c], 1u);
      D.rq[(size_t)c * D.rq_cap + k] = (uint32_t)(sm * INS_SLOTS + tid);
    }
  }
}

// ---------------------------------------------------------------------------------------
// re-VoxelGrid of every window cube (old content ++ inserted points, :795-808); cubes outside
// the window that received points get them appended raw (:762).  One workgroup per cube:
// the merge path (a fixed-point cube plus a few new points, voxel.h vx_merge_fixed_point) or
// the full filter in a VX_THREADS workgroup with the whole LDS, then the cube's cell index.
// ---------------------------------------------------------------------------------------
#ifndef REVOX_PROF_MIN_N
#define REVOX_PROF_MIN_N 0  // diagnostics builds: phase counters of the items of at least this many points only
#endif
template <bool PCL>
__device__ inline void revox_item(MapperDev& D, int s, int m, int slot, int cube, int append, uint32_t* lds) {
  StreamFrame& F = D.fr[s];
  const uint32_t* ioff = D.ins_off + sm_index(s, m) * (INS_SLOTS + 1);
  const uint32_t i0 = ioff[slot], n_new = ioff[slot + 1] - i0;
  uint32_t* tok = D.stable_tok + sm_index(s, m) * NCUBE + cube;
  uint2* tab = D.cube_tab + sm_index(s, m) * NCUBE;
  const uint2 cv = tab[cube];
  // the cube's occupancy block, loaded here so that the index build below does not wait for it
  const uint32_t occ0 = D.occ_blocks ? D.cube_occ[sm_index(s, m) * NCUBE + cube] : 0u;
  if (cv.y + n_new < (uint32_t)REVOX_PROF_MIN_N) D.pdbg = nullptr;
  float4* ar = arena_base(D, s, m, F.arena_active[m]);
  VoxSeg S;
  S.src0 = ar + cv.x;
  S.n0 = (int)cv.y;
  S.src1 = D.ins_sorted + sm_index(s, m) * D.max_in + i0;
  S.tag1 = nullptr;
  S.n1 = (int)n_new;
  S.tag = cube;
  S.leaf = D.leaf[m];
  S.append_only = append;
  S.out = ar;
  S.tail = &F.arena_tail[m];
  S.cap = D.map_cap;
  S.res_off = &tab[cube].x;
  S.res_cnt = &tab[cube].y;
  S.stable_out = tok;
  S.scratch_pts = D.vx_pts + sm_index(s, m) * D.scratch_cap;
  S.scratch_idx = D.vx_idx + sm_index(s, m) * D.scratch_cap;
  S.scratch_tail = &F.scratch_tail[m];
  S.scratch_cap = D.scratch_cap;
  S.err = &F.err;
  S.prof = D.pdbg ? D.pdbg + MD_CUBE_SEG : nullptr;  // merge phases
  S.anchored = 1;  // a merge keys the voxels from the cube's corner (VoxSeg::anchored)
  cube_corner(cube, F.cen, S.anchor);
  bool merged = false;
  const unsigned long long t0 = __builtin_readcyclecounter();
  const bool fixed = n_new > 0 && n_new <= VX_MERGE_CAP && cv.y > 0 && *tok == cv.x + 1;
  if (PCL && !append) {
    // PCL's summation order (exact_voxel_order): also a window cube that received nothing but is not a
    // VoxelGrid fixed point (raw appended or API-set content; the reference re-filters every window
    // cube, :795-808).  Its block of the sort scratch first
    uint32_t* sb = vx_park_block(lds);
    if (threadIdx.x == 0) *sb = atomicAdd(&F.hot_tail[m], cv.y + n_new + MP_SLACK);
    __syncthreads();
    const uint32_t so = *sb;
    __syncthreads();
    S.hot = map_hot(D, sm_index(s, m), so, cv.y + n_new);
    map_filter_exact(D, sm_index(s, m), so, S, VxSrc{S.src0, S.n0, S.src1}, lds, &tab[cube], fixed, &merged);
    __syncthreads();
  } else {
    if (!append && fixed) {
      merged = vx_merge_fixed_point(S, lds);
      __syncthreads();  // false: grid overflow, full filter below
    }
    if (!merged) voxel_segment(S, lds);
    __syncthreads();
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  // the cube's new content -> its cell index (cubeindex.h)
  uint32_t* res = vx_park_result(lds);
  uint32_t* occ_id = vx_park_block(lds);  // (the sort scratch block is done with)
  if (threadIdx.x == 0) {
    const uint2 v = tab[cube];  // written by this thread inside the filter
    res[0] = v.x;
    res[1] = v.y;
    *occ_id = (occ0 && v.y) ? occ0 : occ_acquire(D, sm_index(s, m), cube, v.y);
  }
  __syncthreads();
  const uint32_t off = res[0], n = res[1], oid = *occ_id;
  __syncthreads();  // res may lie in the index build's LDS
  int corner[3];
  cube_corner(cube, F.cen, corner);
  if (!cube_index_build<VX_THREADS, CI_LDS_MAX_T>(ar + off, n, corner, carena_base(D, s, m, F.arena_active[m]) + off,
                                  ctab_base(D, s, m, F.arena_active[m]) + 4 * (size_t)off, lds, D.pdbg ? D.pdbg + MD_INDEX_HASH_CYC : nullptr,
                                  oid ? occ_block(D, sm_index(s, m), oid & ~OCC_FRESH) : nullptr, (oid & OCC_FRESH) != 0) &&
      threadIdx.x == 0)
    atomicOr(&F.err, MAP_ERR_INDEX);
  // read old content + new points, write the filtered cube, then its index (read it, write
  // the cell-sorted copy and the table)
  if (threadIdx.x == 0)
    atomicAdd(&F.vx_bytes, 16ull * (cv.y + n_new) + 16ull * 3 * n + (n ? 8ull * ci_table_size(n) : 0ull));
  if (threadIdx.x == 0 && D.pdbg) {
    const unsigned long long t2 = __builtin_readcyclecounter();
    const int k = merged ? 0 : (append ? 2 : 1);
    atomicAdd(&D.dbg[MD_REVOX_CYC + k], t1 - t0);  // filter cycles: merge / full / append
    atomicAdd(&D.dbg[MD_REVOX_ITEMS + k], 1ull);
    atomicAdd(&D.dbg[MD_INDEX_CYC], t2 - t1);
    atomicAdd(&D.dbg[MD_INDEX_PTS], (unsigned long long)n);
    atomicAdd(&D.dbg[MD_OLD_PTS], (unsigned long long)cv.y);
    int hb = 0;
    while (hb < 7 && n >= (1024u << hb)) ++hb;
    atomicAdd(&D.dbg[MD_REVOX_SIZE_ITEMS + hb], 1ull);
    atomicAdd(&D.dbg[MD_REVOX_SIZE_CYC + hb], t2 - t0);
    if (merged) {
      atomicAdd(&D.dbg[MD_MERGE_NEW_PTS], (unsigned long long)n_new);
      atomicAdd(&D.dbg[MD_MERGES], 1ull);
    }
  }
}

// One workgroup per item (no loop over items: a loop around revox_item spills hundreds of
// registers): workgroup b takes the b-th item of the frame's list (k_insert_bucket), largest size
// class first, so the longest items are dispatched first; workgroups past the list's end leave
// after one load.  PCL: exact_voxel_order (its own instantiation, so that the sort's registers do
// not weigh on the input-order kernel)
static_assert(CI_LDS_MAX_T + CI_OCC_LDS_AT + CI_OCC_LDS <= VX_LDS_WORDS - VX_TAIL_WORDS, "index build LDS");
template <bool PCL>
__global__ void __launch_bounds__(VX_THREADS) k_revox(MapperDev D) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[VX_LDS_WORDS];
  uint32_t b = blockIdx.x;
  int item = -1;
  for (int c = RQ_CLASSES - 1; c >= 0; --c) {
    const uint32_t nc = D.rq_ctl[c];
    if (b < nc) {
      item = (int)D.rq[(size_t)c * D.rq_cap + b];
      break;
    }
    b -= nc;
  }
  if (item < 0) return;
  const int slot = item % INS_SLOTS, sm = item / INS_SLOTS;
  int cube = 0, append = 0;
  if (!revox_target(D, sm >> 1, sm & 1, slot, &cube, &append)) return;
  revox_item<PCL>(D, sm >> 1, sm & 1, slot, cube, append, lds);
}

// cell index of one cube whose content was set through the API (cen: the host's grid centre)
__global__ void __launch_bounds__(VX_THREADS) k_cube_index(MapperDev D, int s, int m, int c0, int c1,
                                                           int3 cen) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[CI_LDS_MAX_T + CI_OCC_LDS_AT + CI_OCC_LDS];
  __shared__ uint32_t occ_id;
  const int cube = c0 + blockIdx.x;
  if (cube >= c1) return;
  StreamFrame& F = D.fr[s];
  const uint2 cv = D.cube_tab[sm_index(s, m) * NCUBE + cube];
  if (threadIdx.x == 0) occ_id = occ_acquire(D, sm_index(s, m), cube, cv.y);  // (an emptied cube's block goes back)
  __syncthreads();
  if (cv.y == 0) return;
  const int cenv[3] = {cen.x, cen.y, cen.z};
  int corner[3];
  cube_corner(cube, cenv, corner);
  const int active = F.arena_active[m];
  if (!cube_index_build<VX_THREADS>(arena_base(D, s, m, active) + cv.x, cv.y, corner,
                                    carena_base(D, s, m, active) + cv.x,
                                    ctab_base(D, s, m, active) + 4 * (size_t)cv.x, lds, nullptr,
                                    occ_id ? occ_block(D, sm_index(s, m), occ_id & ~OCC_FRESH) : nullptr, (occ_id & OCC_FRESH) != 0) &&
      threadIdx.x == 0)
    atomicOr(&F.err, MAP_ERR_INDEX);
}

// ---------------------------------------------------------------------------------------
// arena compaction: live cubes copied, in cube order, into the other arena
// ---------------------------------------------------------------------------------------
// Launched over every (stream, map) pair sm = 2 s0 + b of the handle; a pair whose tail is at
// or below compact_at exits at once (the decision is taken on the device, from the records)
__device__ inline bool compact_due(const MapperDev& D, int sm) {
  return D.fr[sm >> 1].arena_tail[sm & 1] > D.compact_due_at;
}

__global__ void k_compact_scan(MapperDev D, uint32_t* new_off) {
  // one workgroup (1024 threads) per pair
  __shared__ uint32_t ws[VX_WAVES + 1];
  const int sm = 2 * D.s0 + blockIdx.x;
  if (!compact_due(D, sm)) return;
  const uint2* tab = D.cube_tab + (size_t)sm * NCUBE;
  uint32_t* no = new_off + (size_t)blockIdx.x * (NCUBE + 1);
  constexpr int PER = (NCUBE + VX_THREADS - 1) / VX_THREADS;  // 5
  uint32_t v[PER];
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    int c = threadIdx.x * PER + k;
    v[k] = c < NCUBE ? tab[c].y : 0u;
    sum += v[k];
  }
  uint32_t total;
  uint32_t pre = vx_block_scan(sum, ws, &total);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    int c = threadIdx.x * PER + k;
    if (c < NCUBE) no[c] = pre;
    pre += v[k];
  }
  if (threadIdx.x == 0) no[NCUBE] = total;
}

__global__ void k_compact_copy(MapperDev D, const uint32_t* new_off) {
  const int p = blockIdx.y, sm = 2 * D.s0 + p;
  if (!compact_due(D, sm)) return;
  const int s = sm >> 1, m = sm & 1;
  StreamFrame& F = D.fr[s];
  uint2* tab = D.cube_tab + (size_t)sm * NCUBE;
  const uint32_t* no = new_off + (size_t)p * (NCUBE + 1);
  const float4* src = arena_base(D, s, m, F.arena_active[m]);
  float4* dst = arena_base(D, s, m, 1 - F.arena_active[m]);
  const float4* csrc = carena_base(D, s, m, F.arena_active[m]);
  float4* cdst = carena_base(D, s, m, 1 - F.arena_active[m]);
  const uint2* tsrc = ctab_base(D, s, m, F.arena_active[m]);
  uint2* tdst = ctab_base(D, s, m, 1 - F.arena_active[m]);
  for (int c = blockIdx.x; c < NCUBE; c += gridDim.x) {
    const uint2 cv = tab[c];
    for (uint32_t i = threadIdx.x; i < cv.y; i += blockDim.x) {
      dst[no[c] + i] = src[cv.x + i];
      cdst[no[c] + i] = csrc[cv.x + i];  // the cell index moves verbatim (offsets are local)
    }
    if (cv.y) {
      const uint32_t T = ci_table_size(cv.y);
      for (uint32_t h = threadIdx.x; h < T; h += blockDim.x) tdst[4 * (size_t)no[c] + h] = tsrc[4 * (size_t)cv.x + h];
    }
  }
}

__global__ void k_compact_commit(MapperDev D, const uint32_t* new_off) {
  __shared__ int due;
  const int p = blockIdx.x, sm = 2 * D.s0 + p;
  if (threadIdx.x == 0) due = compact_due(D, sm);
  __syncthreads();  // thread 0 moves the tail below
  if (!due) return;
  const int s = sm >> 1, m = sm & 1;
  StreamFrame& F = D.fr[s];
  uint2* tab = D.cube_tab + (size_t)sm * NCUBE;
  const uint32_t* no = new_off + (size_t)p * (NCUBE + 1);
  uint32_t* tok = D.stable_tok + (size_t)sm * NCUBE;
  for (int c = threadIdx.x; c < NCUBE; c += blockDim.x) {
    const bool stable = tok[c] != 0 && tok[c] == tab[c].x + 1;  // content moves verbatim
    tab[c].x = no[c];
    tok[c] = stable ? no[c] + 1 : 0u;
  }
  if (threadIdx.x == 0) {
    F.arena_tail[m] = no[NCUBE];
    F.arena_active[m] = 1 - F.arena_active[m];
    if (no[NCUBE] > D.compact_at) atomicOr(&F.err, MAP_ERR_LIVE);  // the live map itself
    atomicAdd(&D.dbg[MD_COMPACTIONS], 1ull);
    atomicAdd(&D.dbg[MD_COMPACTIONS_MAP + m], 1ull);
  }
}

// ---------------------------------------------------------------------------------------
// publish-side outputs (laser_mapping.cpp:884-911)
// ---------------------------------------------------------------------------------------
// laserCloudMap = corner cube 0, surf cube 0, corner cube 1, ... (:886-891): offsets of every
// (cube, map) run, one workgroup
__global__ void __launch_bounds__(VX_THREADS) k_map_scan(MapperDev D, int s, uint32_t* off) {
  __shared__ uint32_t ws[VX_WAVES + 1];
  const uint2* tc = D.cube_tab + sm_index(s, 0) * NCUBE;
  const uint2* ts = D.cube_tab + sm_index(s, 1) * NCUBE;
  constexpr int PER = (NCUBE + VX_THREADS - 1) / VX_THREADS;
  uint32_t v[2 * PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = threadIdx.x * PER + k;
    v[2 * k] = c < NCUBE ? tc[c].y : 0u;
    v[2 * k + 1] = c < NCUBE ? ts[c].y : 0u;
    sum += v[2 * k] + v[2 * k + 1];
  }
  uint32_t total;
  uint32_t pre = vx_block_scan(sum, ws, &total);
#pragma unroll
  for (int k = 0; k < 2 * PER; ++k) {
    const int c = threadIdx.x * PER + k / 2;
    if (c < NCUBE) off[2 * c + (k & 1)] = pre;
    pre += v[k];
  }
  if (threadIdx.x == 0) off[2 * NCUBE] = total;
}

__global__ void k_map_gather(MapperDev D, int s, const uint32_t* off, float4* out) {
  const StreamFrame& F = D.fr[s];
  for (int e = blockIdx.x; e < 2 * NCUBE; e += gridDim.x) {
    const int c = e >> 1, m = e & 1;
    const uint2 cv = D.cube_tab[sm_index(s, m) * NCUBE + c];
    const float4* src = arena_base(D, s, m, F.arena_active[m]) + cv.x;
    for (uint32_t i = threadIdx.x; i < cv.y; i += blockDim.x) out[off[e] + i] = src[i];
  }
}

// laserCloudFullRes registered with the mapped pose: pointAssociateToMap (:154-164, :901-905)
__global__ void k_register(const float4* in, float4* out, int n, MapPose P) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = to_map(P.x, in[i]);
}

}  // namespace loam
