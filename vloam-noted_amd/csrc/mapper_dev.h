// mapper_dev.h — constants, error flags, the stream / frame records, MapperDev, arena accessors, k_shift_cubes.
// Part of the mapper.hip translation unit: included there only, in the order the phases run.
#pragma once

namespace loam {

constexpr int CW = 21, CH = 21, CD = 11, NCUBE = CW * CH * CD;
constexpr int WIN_MAX = 125;
constexpr int WIN_VALID_MAX = 75;
constexpr int EXTRA_CAP = 64;
// correspondence workgroups: 128 threads x 128 per stream (grid-stride) beat 256 x 64 by 3-5% at
// B = 128 and at one stream (finer scheduling of the latency-bound kNN)
constexpr int CORR_THREADS = 128;  // >= WIN_VALID_MAX (k_knn fills the window tables per thread)
constexpr int CORR_BLK = 128;
static_assert(CORR_THREADS >= WIN_VALID_MAX, "k_knn window tables");
constexpr int LM_THREADS = 256;
constexpr int LM_EBLK = 32;     // LM evaluation workgroups per stream (grid-stride)
constexpr int INS_SLOTS = WIN_VALID_MAX + EXTRA_CAP;
constexpr int RQ_CLASSES = 8;  // re-VoxelGrid items by size: < 1k points, < 2k, .. < 64k, more
constexpr int MAP_ERR_SUBMAP = 4, MAP_ERR_EXTRA = 8, MAP_ERR_HASH = 16, MAP_ERR_LM_SYNC = 32,
              MAP_ERR_INDEX = 64, MAP_ERR_LIVE = 128, MAP_ERR_SORT = 256,
              MAP_ERR_STACK = 512, MAP_ERR_STACK_WAIT = 2048;

// Slots of MapperDev::dbg / pdbg (include/loam_core.h).  Bases of relative slots: _SEG VoxSeg::prof
// (VXM_*, cubes) / prof_seg (VXS_*) and VxPclScratch::prof (VXP_*); _HEAP, _GLOB VxPclScratch's; _HOT, _SORT,
// _WAVES voxel_hot.h's VHF_*, VHS_*, VHD_*; MD_LM lm.h's LmJob::prof ([-2]: the step alone).
enum MapDbg {
  MD_REVOX_CYC = 0 /* [3]: merge, full, append */, MD_MERGE_NEW_PTS = 3, MD_REVOX_ITEMS = 4 /* [3] */, MD_MERGES = 7,
  MD_INDEX_CYC = 8, MD_INDEX_PTS = 9, MD_OLD_PTS = 10, MD_CUBE_SEG = 11 /* [4] */, MD_INDEX_HASH_CYC = 16,
  MD_LM = 17 /* [7] */, MD_REVOX_SIZE_ITEMS = 24 /* [8]: by output size */, MD_REVOX_SIZE_CYC = 32 /* [8] */,
  MD_POSE_DIFF = 40, MD_COMPACTIONS = 41, MD_STACK_SEG = 42 /* [6] */, MD_COMPACTIONS_MAP = 48 /* [2] */,
  MD_CUBE_HOT = 50, MD_STACK_HOT = 54, MD_PREP_CYC = 58 /* [4]: FrameIn load, preparation, stack sizes, submap */,
  MD_PREP_LAUNCHES = 62, MD_PREP_ON_DEVICE = 63, MD_CUBE_GLOB = 64, MD_STACK_GLOB = 65, MD_CUBE_HEAP = 66 /* [2] */,
  MD_STACK_HEAP = 68 /* [2] */, MD_CUBE_SORT = 72, MD_STACK_SORT = 77, MD_CUBE_WAVES = 82, MD_STACK_CUTS = 91,
  MD_OCC_IN_USE = 92 /* filled by the host from occ_used */, MD_OCC_ALLOC_FAIL = 93,
  MD_DBG_END = 94
};
// occupancy blocks (cubeindex.h) of a (stream, map): the window's cubes plus a margin for cubes
// outside the window that hold content; one bit per block in occ_used
constexpr int OCC_POOL = 160, OCC_USED_WORDS = OCC_POOL / 32;
static_assert(OCC_POOL >= WIN_MAX && OCC_POOL % 32 == 0, "occupancy pool");
// k_knn's window view of cube_occ: the cube is not in the submap or empty / has no block
constexpr uint32_t OCC_ABSENT = 0xFFFFFFFFu, OCC_NONE = 0u;
static_assert(MD_POSE_DIFF == 40 && MD_COMPACTIONS == 41 && MD_COMPACTIONS_MAP + 1 == 49, "slots the tests read by number");
static_assert(MD_CUBE_HOT + VHF_SLOTS <= MD_STACK_HOT && MD_STACK_HOT + VHF_SLOTS <= MD_PREP_CYC &&
                  MD_CUBE_SORT + VHS_SLOTS == MD_STACK_SORT && MD_STACK_SORT + VHS_SLOTS == MD_CUBE_WAVES &&
                  MD_CUBE_WAVES + VHD_SLOTS == MD_STACK_CUTS && MD_CUBE_SEG + VXM_SLOTS <= MD_INDEX_HASH_CYC &&
                  MD_STACK_SEG + VXS_SLOTS == MD_COMPACTIONS_MAP && MD_DBG_END <= LOAM_DEBUG_COUNTERS,
              "counter slots");

struct StreamFrame {
  double pose[7];  // in: initial guess (transformAssociateToMap); out: optimised pose
  int active;
  uint32_t epoch;  // frame counter of the handle (marks the cubes outside the window touched this frame)
  int nc_in, ns_in;
  int nc_stack, ns_stack;
  int sub_n[2];
  int optimize;
  int corner_num[2], surf_num[2];
  int valid_num;
  int window[WIN_MAX];
  int sub_off[2][WIN_MAX + 1];
  int center[3];
  int cen[3];
  int shift[3];
  int origin[3];
  uint32_t arena_tail[2];
  int arena_active[2];
  uint32_t scratch_tail[2];
  uint32_t hot_tail[2];   // exact order: the cubes' blocks of the sort scratch (pe / pa / pb / ps)
  int extra_n[2];
  int extra_list[2][EXTRA_CAP];
  int err;
  const float4* in_ptr[2];        // input clouds (mapper staging buffer or caller's HBM)
  unsigned long long cand[2];     // map points in the queries' 27-cell neighbourhoods, per round
  unsigned long long vx_bytes;    // algorithmic bytes of this frame's re-VoxelGrid + cell index
  double wodom[7];  // the frame's odometry pose q_wodom (xyzw), t_wodom
  // q_wmap_wodom, t_wmap_wodom: the frame's initial guess (:206-207) is taken with it, and k_insert_bucket
  // advances it by the frame's transformUpdate (:147-151) as the host does after the frame
  double wmap[7];
  int deferred;     // a queued frame found a recentering or compaction due: left to the host
  LmState lm[2];
  double knn_pose[7];  // the pose the newest k_knn transformed its queries with (loam_mapper_corr_copy)
};

// per-stream input of a frame in the graph path (k_frame_prep), read from page-locked host
// memory: mode 0, the host uploaded the stream records; mode 1, a frame queued behind the one
// in flight (loam_mapper_solve_async) whose records the device prepares from the frame before
struct FrameIn {
  double wodom[7];
  const float4* in_ptr[2];
  int n[2];
  int active;
  int mode;
  uint32_t epoch;
  int pad;
  unsigned long long stack_seq;  // the stack launch (launch_stacks) whose stacks the stream takes
};

// the stack VoxelGrid inputs of a stream (laser_mapping.cpp:492-500): set when its stack is
// launched (loam_mapper_prefetch or the solve), double-buffered by stack parity so that the next
// frame's stack can run beside a frame in flight
struct StackIn {
  const float4* p[2];
  int n[2];
  int active;
  int pad;
};

struct MapPose {  // by-value kernel argument: q (xyzw) + t
  double x[7];
};

struct MapperDev {
  int B;       // streams of this launch (a group of the handle's streams)
  int s0 = 0;  // first stream of the launch
  int max_in, map_cap, sub_cap, scratch_cap, max_chunks;
  float leaf[2];
  uint32_t epoch;
  StreamFrame* fr;
  float4* in_pts[2];
  float4* stack[2];
  float4* arena;  // [B][2 maps][2 arenas][map_cap]
  float4* carena; // same shape: each cube's points sorted by 1 m cell (cubeindex.h)
  uint2* ctab;    // [B][2 maps][2 arenas][4 * map_cap]: each cube's cell table
  uint2* cube_tab;  // [B][2 maps][NCUBE] (off, cnt) — current parity
  uint32_t* extra_flag;  // [B][2][NCUBE]
  // cell occupancy (k_knn skips empty cells): a cube's block id + 1 in its (stream, map)'s pool, 0: none
  // (pool exhausted: every cell "maybe occupied").  Indexed by cube, not by arena offset: a compaction
  // leaves it alone, a window shift moves the id (k_shift_cubes).
  uint32_t* cube_occ;   // [B][2][NCUBE]
  uint32_t* occ_used;   // [B][2][OCC_USED_WORDS] blocks taken
  uint64_t* occ_pool;   // [B][2][occ_blocks][CI_OCC_WORDS]
  int occ_blocks = 0;   // blocks per (stream, map); 0: off (LOAM_KNN_OCC=0), k_knn probes every cell
  int* knn_id;     // [5][B][2*max_in] neighbour ids (submap index) per query, -1: none
  size_t knn_stride;
  // factor records (SoA) [B][2*max_in]
  int* r_type;
  float* r_px;
  float* r_py;
  float* r_pz;
  double* r_a[3];
  double* r_b[3];
  float4* ins_pts;  // [B][2][max_in]
  int* ins_tag;
  float4* ins_sorted;    // [B][2][max_in] inserted points grouped by target cube (input order kept)
  uint32_t* ins_off;     // [B][2][INS_SLOTS + 1] group offsets: window slots, then extra cubes
  unsigned long long* dbg;  // [LOAM_DEBUG_COUNTERS] counters (loam_mapper_debug_counters)
  unsigned long long* pdbg;  // dbg when the phase cycle counters are on (LOAM_PHASE_COUNTERS=1), else null
  uint32_t* stable_tok;  // [B][2][NCUBE] arena offset + 1 of content known to be a VoxelGrid
                         // fixed point (re-filtering it is the identity), else 0
  float4* vx_pts;  // [B][2][scratch_cap]
  int* vx_idx;
  double* partials;  // [B][max_chunks][LM_NACC]
  uint32_t* lm_sync;   // [B][2 rounds][LM_SYNC_WORDS] (lm.h)
  double* lm_xpub;     // [B][2 rounds][8]: eval point published to the workers
  uint32_t* tickets;  // [B]
  uint32_t* lm_tick;  // [B] k_lm_eval's workgroups done (sharded: the last one reduces)
  uint32_t* rq;       // [RQ_CLASSES][rq_cap] re-VoxelGrid items ((2 s + m) INS_SLOTS + slot) by size class
  uint32_t* rq_ctl;   // [RQ_CLASSES] items per class (zeroed by the frame's first kernel)
  int rq_cap = 0;
  // sharded mode (loam_mapper_create_sharded): this rank of nrank; map points are stored by
  // the rank owning their 4 m block (comm.h, shard_owner); blk_v: voxels per block edge
  uint32_t compact_at = 0;  // an arena whose tail passed this is compacted
  uint32_t compact_due_at = 0;  // the compaction kernels' test (compact_at, or earlier: enqueue_frame)
  // exact_voxel_order: the stack and cube VoxelGrids in PCL's summation order (voxel_pcl.h);
  // sort scratch [B][2][scratch_cap] (the stack at offset 0, the cubes from scratch_tail)
  int pcl_order = 0;
  uint64_t* pe;
  uint32_t* pa;
  uint32_t* pb;
  uint64_t* ps;
  int* pseg;  // level lists of global-memory sorts
  int rank = 0, nrank = 1, sharded = 0;
  int blk_v[2] = {1, 1};
  uint32_t* wcnt;        // [B][2][WIN_MAX] window cube counts (all-reduced over the ranks)
  struct NnRec* nn_send; // [queries of all streams] this rank's 5 nearest candidates per query
  const struct NnRec* nn_recv;  // [nrank][same]: every rank's candidates (all-gather)
  const int* q_off;      // [B] first query of stream s in nn_send
  float4* nn_xyz;        // [5][B][2*max_in] merged neighbours (k_geom input in sharded mode)
  double* pose_x;        // [nrank][B][8] every rank's optimised pose (agreement check)
  double* lm_red;        // [B][LM_NACC] this rank's normal-equation sums, then the all-reduced
  // in-process ranks (loam_comm_create_local): the persistent LM's cross-rank slots, shared by the
  // ranks (comm_peer_buffer): [2 frame parities][B][2 rounds][nrank][LM_MAX_PASSES][LM_NACC] and
  // the flags [B][2 rounds][nrank] (lm.h LmJob)
  double* lm_peer = nullptr;
  uint32_t* lm_peer_flag = nullptr;
  // ranks in separate processes (RCCL / callback comms): every rank's LM peer buffer as this
  // process maps it (ipc_peer_setup): [r] slot base, [nrank + r] flag base; each buffer holds
  // [2 frame parities][ipc_B][2 rounds][LM_MAX_PASSES][LM_NACC] f64, then flags [ipc_B][2 rounds]
  const unsigned long long* ipc_tab = nullptr;
  int ipc_B = 0;
  // few streams: the stack VoxelGrid of a (stream, map) split over stack_k workgroups by voxel
  // idx range (k_stack_part + k_stack_cat), else one workgroup (k_stack_ds)
  int stack_k = 0;
  uint2* stk_part;       // [B][2][STACK_K_MAX] (staging offset, centroids) of each range
  // the stack kernels' inputs, outputs and scratch (one stack parity: the frame's, or the next
  // frame's while this one is in flight; D.stack[m] is that parity's stack)
  const StackIn* sin;    // [B]
  int* stk_n;            // [B][2] stack sizes (copied into the frame records by k_stack_counts)
  int* stk_err;          // [B] error flags of the stack kernels (merged by k_stack_counts)
  float4* stk_pts;       // [B][2][max_in] scratch of the input-order stack filter
  int* stk_idx;          // [B][2][max_in]
  int knn_blk = CORR_BLK;  // k_knn workgroups per stream of the cell-split variant
  const FrameIn* fin = nullptr;  // [B] (page-locked host memory) the graph path's frame inputs
  unsigned long long* stk_ready = nullptr;  // the last stack launch done into this parity (k_stack_done)
  int defer_every = 0;    // tests: queued frames with epoch % defer_every == 0 are deferred
};

// one query's 5 nearest candidates on one rank (d: FLANN L2_Simple float distance, id: global
// tie-break key, xyz: the point) — the all-gathered record of the sharded kNN
struct NnRec {
  float d[5];
  int id[5];
  float x[5], y[5], z[5];
};

__device__ inline size_t sm_index(int s, int m) { return (size_t)s * 2 + m; }

__device__ inline float4* arena_base(const MapperDev& D, int s, int m, int active) {
  return D.arena + ((sm_index(s, m) * 2 + active) * (size_t)D.map_cap);
}
__device__ inline float4* carena_base(const MapperDev& D, int s, int m, int active) {
  return D.carena + ((sm_index(s, m) * 2 + active) * (size_t)D.map_cap);
}
__device__ inline uint2* ctab_base(const MapperDev& D, int s, int m, int active) {
  return D.ctab + ((sm_index(s, m) * 2 + active) * (size_t)D.map_cap * 4);
}
// lower corner of cube c (grid index) given the grid centre
__device__ inline void cube_corner(int c, const int* cen, int corner[3]) {
  corner[0] = ci_corner(c % CW, cen[0]);
  corner[1] = ci_corner((c / CW) % CH, cen[1]);
  corner[2] = ci_corner(c / (CW * CH), cen[2]);
}

// occupancy block `id` (1-based) of pair sm
__device__ inline uint64_t* occ_block(const MapperDev& D, size_t sm, uint32_t id) {
  return D.occ_pool + (sm * D.occ_blocks + (id - 1)) * (size_t)CI_OCC_WORDS;
}
__device__ inline void occ_release(const MapperDev& D, size_t sm, uint32_t id) {
  atomicAnd(&D.occ_used[sm * OCC_USED_WORDS + (id - 1) / 32], ~(1u << ((id - 1) & 31)));
}
// a free block of pair sm (any thread; takers and releasers may run side by side); 0: none left
__device__ inline uint32_t occ_alloc(const MapperDev& D, size_t sm) {
  uint32_t* used = D.occ_used + sm * OCC_USED_WORDS;
  for (int w = 0; 32 * w < D.occ_blocks; ++w) {
    const int nb = D.occ_blocks - 32 * w;
    const uint32_t valid = nb >= 32 ? 0xFFFFFFFFu : (1u << nb) - 1u;
    uint32_t cur = atomicOr(&used[w], 0u);
    while (~cur & valid) {
      const int b = __ffs((int)(~cur & valid)) - 1;
      cur = atomicOr(&used[w], 1u << b);
      if (!((cur >> b) & 1u)) return (uint32_t)(32 * w + b + 1);  // the bit was clear: taken
    }
  }
  return 0;
}
// The block the index build of (sm, cube) with n points writes (one thread per cube): the cube's own, else
// a free one (OCC_FRESH set: its old content is another cube's); an empty cube gives its block back.  0: none.
constexpr uint32_t OCC_FRESH = 0x80000000u;
__device__ inline uint32_t occ_acquire(const MapperDev& D, size_t sm, int cube, uint32_t n) {
  if (!D.occ_blocks) return 0;
  uint32_t* slot = D.cube_occ + sm * NCUBE + cube;
  uint32_t id = *slot;
  if (n == 0) {
    if (id) {
      occ_release(D, sm, id);
      *slot = 0;
    }
    return 0;
  }
  if (id) return id;
  id = occ_alloc(D, sm);
  if (id) *slot = id;
  else atomicAdd(&D.dbg[MD_OCC_ALLOC_FAIL], 1ull);
  return id ? id | OCC_FRESH : 0u;
}

// ---------------------------------------------------------------------------------------
// ring-buffer recentering (laser_mapping.cpp:252-444): content moves by shift[axis] cube
// indices, the slabs that wrap around are cleared.
// ---------------------------------------------------------------------------------------
// The fixed-point tokens move with their cubes (into tok_tmp, copied back on the same stream):
// a token left at the old index would send every moved cube through a full re-filter.  So do the
// occupancy block ids (occ_tmp); a cube that leaves the grid gives its block back.
__global__ void k_shift_cubes(MapperDev D, const uint2* __restrict__ old_tab, uint2* new_tab, uint32_t* tok_tmp,
                              uint32_t* occ_tmp) {
  int s = D.s0 + blockIdx.y;
  const StreamFrame& F = D.fr[s];
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < 2 * NCUBE; t += gridDim.x * blockDim.x) {
    int m = t / NCUBE, c = t % NCUBE;
    int i = c % CW, j = (c / CW) % CH, k = c / (CW * CH);
    int oi = i - F.shift[0], oj = j - F.shift[1], ok = k - F.shift[2];
    uint2 v = make_uint2(0, 0);
    uint32_t tok = 0, occ = 0;
    if (oi >= 0 && oi < CW && oj >= 0 && oj < CH && ok >= 0 && ok < CD) {
      const size_t o = sm_index(s, m) * NCUBE + oi + CW * oj + CW * CH * ok;
      v = old_tab[o];
      tok = D.stable_tok[o];
      occ = D.cube_occ[o];
    }
    new_tab[sm_index(s, m) * NCUBE + c] = v;
    tok_tmp[sm_index(s, m) * NCUBE + c] = tok;
    occ_tmp[sm_index(s, m) * NCUBE + c] = occ;
    // cube c of the old grid: where it goes
    const int ni = i + F.shift[0], nj = j + F.shift[1], nk = k + F.shift[2];
    const uint32_t mine = D.cube_occ[sm_index(s, m) * NCUBE + c];
    if (mine && (ni < 0 || ni >= CW || nj < 0 || nj >= CH || nk < 0 || nk >= CD)) occ_release(D, sm_index(s, m), mine);
  }
}

}  // namespace loam
