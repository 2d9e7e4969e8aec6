// mapper_frame.h — a frame's records: k_frame_prep, k_submap_prep / _count, k_frame_out.
// Part of the mapper.hip translation unit: included there only, in the order the phases run.
#pragma once

namespace loam {

// a queued frame's stream record, prepared on the device from what the frames before left (what
// the host does in enqueue_frame): the initial guess (:206-207) with the transform of the
// stream's last solve, the window (:228-251, :455-472).  A frame that needs a recentering or an
// arena compaction, or follows a deferred one, is deferred: the stream stays inactive and the
// host runs it again on its own path (the device state is left as the frames before left it).
// All threads of the block: thread 0 decides from registers (one round of loads of the record),
// the window list is built one slot per thread (i, j, k order: :455-472).
__device__ inline void frame_prep_device(const MapperDev& D, StreamFrame& F, const FrameIn& I) {
  __shared__ int ok, c3s[3], cens[3];
  __shared__ uint64_t vmask[2];
  const int tid = threadIdx.x;
  if (tid == 0) {
    const int prev_deferred = F.deferred;
    double wmap[7];
    for (int i = 0; i < 7; ++i) wmap[i] = F.wmap[i];
    int cen[3] = {F.cen[0], F.cen[1], F.cen[2]};
    const uint32_t t0 = F.arena_tail[0], t1 = F.arena_tail[1];
    F.active = 0;
    ok = 0;
    if (I.active) {
      double pose[7];
      pose_initial_guess(wmap, I.wodom, pose);
      int center[3], shift[3];
      const bool shifted = frame_center(pose, cen, center, shift);
      const bool compact = t0 > D.compact_at || t1 > D.compact_at;
      const bool forced = D.defer_every > 0 && I.epoch % (uint32_t)D.defer_every == 0;
      for (int i = 0; i < 7; ++i) F.wodom[i] = I.wodom[i];
      if (prev_deferred || shifted || compact || forced) {
        F.deferred = 1;
      } else {
        frame_reset(F);
        F.active = 1;
        for (int i = 0; i < 7; ++i) F.pose[i] = pose[i];
        for (int a = 0; a < 3; ++a) {
          F.center[a] = c3s[a] = center[a];
          cens[a] = cen[a];
        }
        F.origin[0] = (center[0] - 2 - cen[0]) * 50 - 25 - 2;  // as frame_window
        F.origin[1] = (center[1] - 2 - cen[1]) * 50 - 25 - 2;
        F.origin[2] = (center[2] - 1 - cen[2]) * 50 - 25 - 2;
        F.epoch = I.epoch;
        F.in_ptr[0] = I.in_ptr[0];
        F.in_ptr[1] = I.in_ptr[1];
        F.nc_in = I.n[0];
        F.ns_in = I.n[1];
        ok = 1;
      }
    }
  }
  __syncthreads();
  if (!ok) return;
  // window slot t = (i * 5 + j) * 3 + k of the 5 x 5 x 3 cubes around the centre, kept if inside
  // the grid, in that order (frame_window)
  const int t = tid;
  const int i = c3s[0] - 2 + t / 15, j = c3s[1] - 2 + (t / 3) % 5, k = c3s[2] - 1 + t % 3;
  const bool in = t < 75 && i >= 0 && i < CW && j >= 0 && j < CH && k >= 0 && k < CD;
  const uint64_t b = __ballot(in);
  const int w = tid >> 6, lane = tid & 63;
  if (lane == 0 && w < 2) vmask[w] = b;
  __syncthreads();
  const int pos = (w == 1 ? __popcll(vmask[0]) : 0) + __popcll(b & ((1ull << lane) - 1));
  if (in) F.window[pos] = i + CW * j + CW * CH * k;
  if (tid == 0) F.valid_num = __popcll(vmask[0]) + __popcll(vmask[1]);
  __syncthreads();
}

// the graph path's last kernel: every stream record to page-locked host memory (write-through
// stores), then the frame's number (FrameIn.epoch) to the host's done word: the host waits on
// that word instead of an event record and a D2H copy between frames
__global__ void __launch_bounds__(256) k_frame_out(MapperDev D, StreamFrame* out, unsigned long long* done) {
  constexpr int W = (int)(sizeof(StreamFrame) / 8);
  static_assert(sizeof(StreamFrame) % 8 == 0, "record copy granularity");
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(D.fr + D.s0);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(out);
  for (int w = threadIdx.x; w < D.B * W; w += blockDim.x)
    __hip_atomic_store(dst + w, src[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // every lane's write-through stores complete before the done word (no fence: a system-scope
  // release writes back the whole L2, dirty with the frame's map; ~5 us, tools/mb_flush.hip)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long e = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(&D.fin[0].epoch),
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) & 0xFFFFFFFFull;
    __hip_atomic_store(done, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}


// FrameIn from page-locked host memory into LDS: one system-scope load per lane, all in flight
// together (the host wrote it before the launch; each read crosses the host link)
constexpr int FRAME_IN_WORDS = (int)(sizeof(FrameIn) / 8);
static_assert(sizeof(FrameIn) % 8 == 0 && FRAME_IN_WORDS <= 64, "FrameIn copy granularity");
__device__ inline void load_frame_in(const FrameIn* p, FrameIn* lds) {
  const int w = threadIdx.x;
  if (w < FRAME_IN_WORDS)
    reinterpret_cast<unsigned long long*>(lds)[w] =
        __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p) + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------
// submap: offsets of the window cubes (laserCloudCornerFromMap concatenation order)
// ---------------------------------------------------------------------------------------
__device__ inline void submap_prep(const MapperDev& D, int s, StreamFrame& F) {
  // one wave per map; window slots 2*lane, 2*lane+1 (valid_num <= 75 <= 128)
  const int m = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint2* tab = D.cube_tab + sm_index(s, m) * NCUBE;
  const int vn = F.valid_num;
  const int w0 = 2 * lane, w1 = 2 * lane + 1;
  const uint32_t* wc = D.wcnt + sm_index(s, m) * WIN_MAX;  // sharded: summed over the ranks
  const uint32_t c0 = w0 < vn ? (D.sharded ? wc[w0] : tab[F.window[w0]].y) : 0u;
  const uint32_t c1 = w1 < vn ? (D.sharded ? wc[w1] : tab[F.window[w1]].y) : 0u;
  const uint32_t inc = wave_incl_scan_u(c0 + c1);
  uint32_t total = __shfl(inc, 63, 64);
  const bool over = total > (uint32_t)D.sub_cap;
  const uint32_t ex = over ? 0u : inc - (c0 + c1);
  if (w0 < vn) F.sub_off[m][w0] = ex;
  if (w1 < vn) F.sub_off[m][w1] = over ? 0u : ex + c0;
  if (lane == 0) {
    if (over) {
      atomicOr(&F.err, MAP_ERR_SUBMAP);
      total = 0;
    }
    F.sub_off[m][vn] = total;
    F.sub_n[m] = total;
    F.scratch_tail[m] = 0;  // re-VoxelGrid scratch (bounded by max_submap_points + stacks)
    F.hot_tail[m] = 0;
    F.extra_n[m] = 0;
    if (m == 0) F.vx_bytes = 0;
  }
  __syncthreads();
  // laser_mapping.cpp:514
  if (threadIdx.x == 0) F.optimize = (F.sub_n[0] > 10 && F.sub_n[1] > 50) ? 1 : 0;
}

__global__ void __launch_bounds__(128) k_submap_prep(MapperDev D) {
  const int s = D.s0 + blockIdx.x;
  StreamFrame& F = D.fr[s];
  if (blockIdx.x == 0 && threadIdx.x < RQ_CLASSES) D.rq_ctl[threadIdx.x] = 0u;  // this frame's k_revox list
  if (!F.active) return;
  submap_prep(D, s, F);
}

// the graph path's first kernel: a queued frame's records (frame_prep_device), the stack sizes
// (k_stack_counts) and the submap offsets (k_submap_prep) in one launch
__global__ void __launch_bounds__(128) k_frame_prep(MapperDev D) {
  const int s = D.s0 + blockIdx.x;
  StreamFrame& F = D.fr[s];
  if (blockIdx.x == 0 && threadIdx.x < RQ_CLASSES) D.rq_ctl[threadIdx.x] = 0u;  // this frame's k_revox list
  __shared__ int go;
  __shared__ FrameIn I;
  const unsigned long long t0 = __builtin_readcyclecounter();
  load_frame_in(D.fin + s, &I);
  __syncthreads();
  if (threadIdx.x == 0 && I.active && I.stack_seq) {  // the stream's stacks (launched on the stack stream)
    uint32_t spins = 0;
    while (__hip_atomic_load(D.stk_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < I.stack_seq) {
      if (++spins > (1u << 24)) {
        atomicOr(&F.err, MAP_ERR_STACK_WAIT);
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
    // the stack sizes are read with agent-scope loads (stack_counts); the stack points only by
    // later kernels, which start after every stack of the frame has ended
  }
  __syncthreads();
  const unsigned long long t1 = __builtin_readcyclecounter();
  if (I.mode == 1) frame_prep_device(D, F, I);  // (block-uniform branch)
  const unsigned long long t2 = __builtin_readcyclecounter();
  if (threadIdx.x == 0) {
    if (F.active) stack_counts(D, s, F);
    go = F.active;
  }
  __syncthreads();
  if (!go) return;
  const unsigned long long t3 = __builtin_readcyclecounter();
  submap_prep(D, s, F);
  if (D.pdbg && threadIdx.x == 0) {  // cycles: FrameIn load, device prep, stack counts, submap
    const unsigned long long t4 = __builtin_readcyclecounter();
    atomicAdd(&D.pdbg[MD_PREP_CYC], t1 - t0);
    atomicAdd(&D.pdbg[MD_PREP_CYC + 1], t2 - t1);
    atomicAdd(&D.pdbg[MD_PREP_CYC + 2], t3 - t2);
    atomicAdd(&D.pdbg[MD_PREP_CYC + 3], t4 - t3);
    atomicAdd(&D.pdbg[MD_PREP_LAUNCHES], 1ull);
    if (I.mode == 1) atomicAdd(&D.pdbg[MD_PREP_ON_DEVICE], 1ull);
  }
}

// sharded: this rank's point count of every window cube, all-reduced before k_submap_prep so
// that every rank sees the whole submap's sizes and concatenation offsets (:475-489, :514)
__global__ void __launch_bounds__(256) k_submap_count(MapperDev D) {
  const int s = D.s0 + blockIdx.x;
  const StreamFrame& F = D.fr[s];
  for (int t = threadIdx.x; t < 2 * WIN_MAX; t += blockDim.x) {
    const int m = t / WIN_MAX, w = t % WIN_MAX;
    uint32_t c = 0;
    if (F.active && w < F.valid_num) c = D.cube_tab[sm_index(s, m) * NCUBE + F.window[w]].y;
    D.wcnt[sm_index(s, m) * WIN_MAX + w] = c;
  }
}

}  // namespace loam
