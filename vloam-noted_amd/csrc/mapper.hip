// mapper.hip — LaserMapping::solveMapping (laser_mapping.cpp:212-814) on MI355X.
//
// One handle = B independent mapping streams; every launch below covers all of them.
// Per frame (all device resident):
//   k_stack_part/_cat  VoxelGrid of laserCloudCornerLast (0.4 m) / SurfLast (0.8 m) (:492-500),
//                      on a second stream, ahead of the frame (loam_mapper_prefetch / the
//                      solve), double-buffered by frame parity; k_stack_ds at many streams
//   k_shift_cubes      ring-buffer recentering of the 21x21x11 cube grid (:252-444), rare
//   k_frame_prep       (graph path) a queued frame's records from the frame before (initial
//                      guess :206-207, window :228-251), stack sizes, submap offsets (:448-489);
//                      no per-frame index build: every cube keeps a persistent 1 m cell
//                      index (cubeindex.h, replaces the KD-tree build :519-520), rebuilt
//                      only when its content changes (k_revox); exact 5-NN because accepted
//                      matches need all 5 neighbours within 1 m (:557, :642)
//   2 x { k_knn         exact 5-NN of every query in the cell index (:554, :633)
//         k_geom        PCA line / QR plane fit of the neighbours -> factor records (:557-699)
//         k_lm_round    all <= 5 Ceres TR-LM passes, G workgroups per stream (lm.h) }
//   k_insert_bucket    transform stacks with the final pose, assign cubes (:741-788), group
//                      the points by target cube
//   k_revox            re-VoxelGrid every changed window cube (:795-808) into the map arena,
//                      and its cell index
//   k_frame_out        (graph path) the records to the host and the frame's done word
//                      (a last-workgroup hand-off inside k_revox measured 1.5x slower: every
//                      workgroup's agent-scope release writes back L2)
//
// Map storage: per (stream, map) an append-only arena of float4 points + a cube table
// (offset, count) for the 4851 cubes; window cubes are rewritten at the arena tail every
// frame, the host compacts an arena when its tail passes half the capacity.
//
// The device code lives in headers included below in this order (one translation unit); this
// file is the host side: the handle, the two-frames-in-flight queue and the C-ABI.
//   mapper_dev.h    constants, error flags, StreamFrame / FrameIn / StackIn / MapperDev, k_shift_cubes
//   mapper_stack.h  k_stack_ds / _part / _cat / _done / _counts
//   mapper_frame.h  k_frame_prep, k_submap_prep / _count, k_frame_out
//   mapper_corr.h   k_knn, k_nn_merge, k_geom
//   mapper_lm.h     k_lm_eval / _step / _round / _group, k_pose_publish / _adopt
//   mapper_map.h    k_insert_bucket, k_revox, k_cube_index, k_compact_*, k_map_scan / _gather, k_register
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <array>
#include <cstring>
#include <deque>
#include <memory>
#include <vector>

#include "common.h"
#include "device_math.h"
#include "cellhash.h"
#include "comm.h"
#include "cubeindex.h"
#include "device_res.h"
#include "lm.h"
#include "voxel.h"
#include "voxel_hot.h"
#include "voxel_pcl.h"
#include "mapper_dev.h"
#include "mapper_stack.h"
#include "mapper_frame.h"
#include "mapper_corr.h"
#include "mapper_lm.h"
#include "mapper_map.h"

namespace loam {

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct HostStream {
  double q_wmap_wodom[4] = {0, 0, 0, 1}, t_wmap_wodom[3] = {0, 0, 0};
  double q_wodom[4] = {0, 0, 0, 1}, t_wodom[3] = {0, 0, 0};
  double pose[7] = {0, 0, 0, 1, 0, 0, 0};
  double q_hf[4] = {0, 0, 0, 1}, t_hf[3] = {0, 0, 0};
  bool skip = false;
  bool solved_last = false;  // solved by the last loam_mapper_solve (loam_mapper_total_iterations)
  // the input of the next solve (LaserMapping::input, laser_mapping.cpp:178-209), kept apart from
  // the frame in flight (loam_mapper_solve_async) until that solve takes it
  bool in_ready = false;
  bool stk_launched = false;  // its stack VoxelGrid already queued (loam_mapper_prefetch)
  unsigned long long stk_seq = 0;  // that stack launch (k_stack_done)
  const float4* in_p[2] = {nullptr, nullptr};
  int in_n[2] = {0, 0};
  double in_q[4] = {0, 0, 0, 1}, in_t[3] = {0, 0, 0};
  int frame = 0;
  int cen[3] = {10, 10, 5};  // laserCloudCen* after the stream's last finished frame
  loam_map_stats st{};
};

// device error flags of a stream -> message (VX_ERR_* of voxel.h, MAP_ERR_* above)
inline std::string map_err_text(int e) {
  std::string m;
  auto add = [&](int bit, const char* what) {
    if (e & bit) m += (m.empty() ? "" : ", ") + std::string(what);
  };
  add(VX_ERR_CAPACITY, "VoxelGrid scratch full");
  add(VX_ERR_OUTPUT, "map arena full (max_map_points)");
  add(MAP_ERR_SUBMAP, "submap larger than max_submap_points");
  add(MAP_ERR_EXTRA, "too many out-of-window insertions");
  add(MAP_ERR_HASH, "cell table full");
  add(MAP_ERR_LM_SYNC, "LM workgroup hand-off timed out");
  add(MAP_ERR_INDEX, "cube cell index capacity");
  add(MAP_ERR_LIVE, "live map larger than the arena's compaction bound");
  add(MAP_ERR_SORT, "PCL-order VoxelGrid input larger than its sort lists / scratch");
  add(MAP_ERR_STACK, "split stack VoxelGrid: a range has more voxels than its LDS groups");
  add(MAP_ERR_STACK_WAIT, "the frame's stack VoxelGrid did not finish in time (device wait)");
  add(VH_ERR_ROOTS | VH_ERR_LIST, "PCL-order VoxelGrid sort lists full");
  add(VH_ERR_SPIN, "PCL-order VoxelGrid sort: a wave's wait for a listed subtree ran out");
  return m + " (flags " + std::to_string(e) + ")";
}

}  // namespace loam

using namespace loam;

enum : int { FAM_STACK = 0, FAM_HASH, FAM_CORR, FAM_LM, FAM_INSERT, FAM_REVOX, FAM_OTHER, NFAM };

// a frame in flight (loam_mapper_solve_async): what its streams were given, where its records
// come back (the D2H buffer of its stack parity), and whether it was queued behind another
// frame with its records prepared on the device (chained)
struct FrameRec {
  bool chained = false, graph = false;
  bool has_deferred = false;  // known (its records are back) to have deferred streams
  bool pending = false;       // not enqueued yet: inputs and stack taken, run on the host path later
  bool behind = false;        // solve_async was called with another frame in the queue
  bool early_seen = false;    // its poses and stats were taken from the early records (loam_mapper_solve_pose)
  uint32_t epoch = 0;         // its frame number (the done word frame_out writes)
  int fpar = 0;
  uint64_t seq = 0;  // enqueue order (0: not enqueued)
  std::vector<int> active;
  std::vector<std::array<double, 7>> wodom;
  std::vector<std::array<const float4*, 2>> in_p;
  std::vector<std::array<int, 2>> in_n;
  std::vector<unsigned long long> stk_seq;
  FrameRec() = default;
  FrameRec(int B, int par)  // no stream active yet
      : fpar(par), active(B, 0), wodom(B, std::array<double, 7>{0, 0, 0, 1, 0, 0, 0}),
        in_p(B, std::array<const float4*, 2>{nullptr, nullptr}), in_n(B, std::array<int, 2>{0, 0}), stk_seq(B, 0ull) {}
  bool any_active() const { return std::find(active.begin(), active.end(), 1) != active.end(); }
  // stream s of the frame takes what stream s of `from` was given
  void take(int s, const FrameRec& from) {
    active[s] = 1;
    wodom[s] = from.wodom[s];
    in_p[s] = from.in_p[s];
    in_n[s] = from.in_n[s];
    stk_seq[s] = from.stk_seq[s];
  }
};

// what is double-buffered by stack parity (a frame's fpar): the next frame's stack VoxelGrid runs
// beside the frame in flight, and each of the two frames in the queue has its own record buffers
struct ParitySlot {
  PinnedArray<StreamFrame> hfo;  // the records after that parity's frame
  StreamFrame* hfo_dev = nullptr;
  // loam_mapper_solve_pose: graph-path frames also write their records after the second LM round
  // (before the insertion and re-VoxelGrid) with their own done word
  PinnedArray<StreamFrame> hfo_early;
  StreamFrame* hfo_early_dev = nullptr;
  PinnedArray<FrameIn> fin;  // the graph path's frame inputs (k_frame_prep)
  const FrameIn* fin_dev = nullptr;
  DevEvent ev_fr[2];  // frame start / records back (timed)
  DevEvent ev_sin;    // the last reads of hsin done
  float4* stack_buf[2] = {nullptr, nullptr};  // [map]
  int* stk_n_buf = nullptr;
  int* stk_err_buf = nullptr;
  StackIn* sin_buf = nullptr;
  PinnedArray<StackIn> hsin;
};

struct loam_mapper {
  DevStream st;   // the streams first: destroyed after everything below
  DevStream st2;  // stack VoxelGrid, concurrent with the submap / hash build
  // the status of a frame loam_mapper_solve_async finished to make room (LOAM_ERR_CAPACITY /
  // _SYNC), held for the next loam_mapper_wait / loam_mapper_solve (as LOAM_ERR_EARLIER): the
  // solve_async that finished it returns OK, since it did enqueue its own frame
  int32_t held_rc = 0;
  std::string held_msg;
  loam_params P;
  bool prof = false;
  std::vector<DevEvent> ev_pool;
  std::vector<int> ev_fam;  // family of each recorded (start, stop) pair
  double fam_ms[NFAM] = {0}, fam_bytes[NFAM] = {0};
  long long fam_launches[NFAM] = {0};
  int dev = 0, B = 1;
  DevEvent ev_opt_begin, ev_opt_end;  // around the optimisation block (host path)
  MapperDev D{};
  PinnedArray<StreamFrame> hf;  // pinned: the per-frame H2D / D2H of the stream records
  std::vector<HostStream> hs;
  uint2* cube_tab[2] = {nullptr, nullptr};
  int parity = 0;
  uint32_t* tok_tmp = nullptr;  // [B][2][NCUBE] the shifted fixed-point tokens
  uint32_t* occ_tmp = nullptr;  // [B][2][NCUBE] the shifted occupancy block ids
  uint32_t* d_new_off = nullptr;
  DevPool pool;
  uint32_t frame_counter = 0;
  int n_cu = 256;  // compute units (grid of the worklist kernels)
  // compact an arena once its tail passes this: one frame writes at most the window content
  // (<= max_submap_points) plus the stack (<= max_input_points) plus the few cubes outside
  // the window that receive points; a write past the capacity is reported (err flags)
  uint32_t compact_at = 0;
  int lm_G = 0;  // workgroups per stream of k_lm_round (0: two-kernel path k_lm_eval / k_lm_step)
  bool want_ipc = false;            // cross-process ranks: set up the IPC peer buffers at create
  DevBuf<char> ipc_own;             // this rank's LM peer buffer (ipc_peer_setup)
  std::vector<void*> ipc_open;      // the other ranks' buffers, mapped from their IPC handles
  int knn_cs = 0;     // k_knn: 8 lanes per query splitting the cells (handles of <= 4 streams), else 0
                      // (one lane per query)
  loam_comm* comm = nullptr;  // sharded mode (loam_mapper_create_sharded)
  PinnedArray<int> q_off;     // [B + 1] query offsets of the sharded kNN exchange
  int* d_q_off = nullptr;
  // hipGraph of the whole per-frame sequence (handles of <= 4 streams): one per cube-table
  // parity, used for frames without recentering, compaction, profiling or sharding
  int use_graph = 0;
  hipGraphExec_t gexec[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [cube parity][stack parity]
  // stack VoxelGrids ahead of their frame (loam_mapper_prefetch / loam_mapper_solve_async):
  // stacks, their inputs and counts double-buffered by stack parity; spar: the next frame's
  int spar = 0, last_spar = 0;
  ParitySlot slot[2];
  // frames in flight, oldest first: at most two, the second queued behind the first on the
  // device (loam_mapper_solve_async on a graph-path handle, its records from k_frame_prep)
  std::deque<FrameRec> q;
  uint64_t seq = 0, mirror_seq = 0;  // hf mirrors the device records as of frame mirror_seq
  unsigned long long stack_seq = 0;
  unsigned long long* d_stk_ready = nullptr;  // [2 parities]
  PinnedArray<unsigned long long> done;  // [2 parities]
  unsigned long long* done_dev = nullptr;
  bool early = false;  // loam_mapper_solve_pose was called: frames write their early records
  PinnedArray<unsigned long long> done_early;  // [2 parities]
  unsigned long long* done_early_dev = nullptr;
  uint32_t grow_max = 0;     // largest arena growth of one frame seen (compaction foresight)
  std::vector<std::array<uint32_t, 2>> last_tail;
  DevEvent ev_stack;               // after the last stack launch (on st2)
  // publish-side buffers (grown on demand)
  uint32_t* d_map_off = nullptr;  // [2 * NCUBE + 1]
  DevBuf<float4> d_pub;
  // what is not a plain resource goes here; the members release themselves after it
  ~loam_mapper() {
    (void)hipStreamSynchronize(st);
    (void)hipStreamSynchronize(st2);
    if (D.lm_peer && comm) comm_peer_release(comm);  // the group's LM peer buffer
    for (void* p : ipc_open) (void)hipIpcCloseMemHandle(p);
    for (auto& gp : gexec)
      for (auto& g : gp)
        if (g) (void)hipGraphExecDestroy(g);
  }
};

namespace {

uint32_t next_pow2(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

void host_initial_guess(HostStream& H, double* pose) {
  // LaserMapping::input (laser_mapping.cpp:206-207)
  dq qm{H.q_wmap_wodom[0], H.q_wmap_wodom[1], H.q_wmap_wodom[2], H.q_wmap_wodom[3]};
  dq qo{H.q_wodom[0], H.q_wodom[1], H.q_wodom[2], H.q_wodom[3]};
  dq q = qmul(qm, qo);
  d3 r = qrot(qm, d3{H.t_wodom[0], H.t_wodom[1], H.t_wodom[2]});
  pose[0] = q.x; pose[1] = q.y; pose[2] = q.z; pose[3] = q.w;
  pose[4] = r.x + H.t_wmap_wodom[0];
  pose[5] = r.y + H.t_wmap_wodom[1];
  pose[6] = r.z + H.t_wmap_wodom[2];
}

void host_transform_update(HostStream& H) {
  // LaserMapping::transformUpdate (laser_mapping.cpp:147-151)
  dq qw{H.pose[0], H.pose[1], H.pose[2], H.pose[3]};
  dq qo{H.q_wodom[0], H.q_wodom[1], H.q_wodom[2], H.q_wodom[3]};
  dq qm = qmul(qw, qinv(qo));
  d3 r = qrot(qm, d3{H.t_wodom[0], H.t_wodom[1], H.t_wodom[2]});
  H.q_wmap_wodom[0] = qm.x; H.q_wmap_wodom[1] = qm.y; H.q_wmap_wodom[2] = qm.z; H.q_wmap_wodom[3] = qm.w;
  H.t_wmap_wodom[0] = H.pose[4] - r.x;
  H.t_wmap_wodom[1] = H.pose[5] - r.y;
  H.t_wmap_wodom[2] = H.pose[6] - r.z;
}

// the record of a stream before its first frame: centred cube grid, identity poses
StreamFrame fresh_record() {
  StreamFrame F{};
  F.cen[0] = 10; F.cen[1] = 10; F.cen[2] = 5;
  F.pose[3] = F.wodom[3] = F.wmap[3] = 1.0;
  return F;
}

// q (xyzw) + t <-> one pose array of 7
void pack7(const double* q, const double* t, double* x) {
  std::copy(q, q + 4, x);
  std::copy(t, t + 3, x + 4);
}
void unpack7(const double* x, double* q, double* t) {
  std::copy(x, x + 4, q);
  std::copy(x + 4, x + 7, t);
}

int32_t check_stream(loam_mapper* h, int32_t s) {
  if (!h) {
    set_error("null mapper handle");
    return LOAM_ERR_ARG;
  }
  if (s < 0 || s >= h->B) {
    set_error("stream index out of range");
    return LOAM_ERR_ARG;
  }
  return LOAM_OK;
}

// the stack buffers, inputs and counts of stack parity `par` for the kernels launched with D
void bind_stack_parity(const loam_mapper* h, MapperDev& D, int par) {
  const ParitySlot& S = h->slot[par];
  D.sin = S.sin_buf;
  D.stk_n = S.stk_n_buf;
  D.stk_err = S.stk_err_buf;
  for (int m = 0; m < 2; ++m) D.stack[m] = S.stack_buf[m];
}

}  // namespace

extern "C" {

// The persistent LM across processes (the peer one-shot reduce instead of an RCCL
// all-reduce per LM iteration): every rank allocates its LM peer buffer, exports it as an IPC handle,
// the handles travel through the comm's own all-gather, and every rank maps the others'.  All ranks
// take the same decision (each one's outcome is all-gathered): on any failure every rank keeps the
// two-kernel path.  Returns LOAM_OK with D.ipc_tab set, or LOAM_OK without it (fall back), or the
// comm's error.
static int32_t ipc_peer_setup(loam_mapper* h) {
  loam_comm* c = h->comm;
  MapperDev& D = h->D;
  const int R = c->size, me = c->rank;
  const size_t B = h->B, nslot = 2 * B * 2 * LM_MAX_PASSES * LM_NACC;
  const size_t bytes = nslot * sizeof(double) + B * 2 * sizeof(uint32_t);
  struct Msg {
    hipIpcMemHandle_t hdl;
    int32_t ok, pad;
  };
  static_assert(sizeof(Msg) % 8 == 0, "exchange record");
  Msg mine{};
  void* buf = nullptr;
  DevBuf<char> own;
  // uncached device memory where the runtime offers it (its accesses bypass the caches of every
  // agent, as RCCL's flags); else ordinary device memory (the accesses are system-scope atomics)
  if (hipExtMallocWithFlags(&buf, bytes, hipDeviceMallocUncached) != hipSuccess) {
    (void)hipGetLastError();
    buf = nullptr;
    if (hipMalloc(&buf, bytes) != hipSuccess) {
      (void)hipGetLastError();
      buf = nullptr;
    }
  }
  own.adopt(static_cast<char*>(buf), bytes);
  mine.ok = buf && hipMemset(buf, 0, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
            hipIpcGetMemHandle(&mine.hdl, buf) == hipSuccess;
  if (!mine.ok) (void)hipGetLastError();
  DevBuf<Msg> dsend, drecv;
  std::vector<Msg> all(R);
  TRY(dsend.reserve(1));
  TRY(drecv.reserve(R));
  auto exchange = [&]() -> int32_t {  // mine -> all (every rank's, in rank order)
    if (hipMemcpy(dsend, &mine, sizeof(Msg), hipMemcpyHostToDevice) != hipSuccess) return LOAM_ERR_HIP;
    TRY(comm_allgather(c, dsend, drecv, (int64_t)sizeof(Msg), h->st));
    if (hipStreamSynchronize(h->st) != hipSuccess ||
        hipMemcpy(all.data(), drecv, sizeof(Msg) * R, hipMemcpyDeviceToHost) != hipSuccess)
      return LOAM_ERR_HIP;
    return LOAM_OK;
  };
  int32_t rc = exchange();
  bool ok = rc == LOAM_OK;
  for (int r = 0; r < R && ok; ++r) ok = all[r].ok != 0;
  std::vector<unsigned long long> tab(2 * (size_t)R, 0ull);
  if (ok) {  // map the others' buffers; then agree that every rank mapped every buffer
    for (int r = 0; r < R; ++r) {
      void* p = buf;
      if (r != me) {
        p = nullptr;
        if (hipIpcOpenMemHandle(&p, all[r].hdl, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
          (void)hipGetLastError();
          p = nullptr;
        } else {
          h->ipc_open.push_back(p);
        }
      }
      tab[r] = reinterpret_cast<unsigned long long>(p);
      tab[R + r] = p ? reinterpret_cast<unsigned long long>(static_cast<char*>(p) + nslot * sizeof(double)) : 0ull;
      if (!p) ok = false;
    }
    const hipIpcMemHandle_t keep = mine.hdl;
    mine = Msg{};
    mine.hdl = keep;
    mine.ok = ok ? 1 : 0;
    if (rc == LOAM_OK) rc = exchange();
    ok = rc == LOAM_OK;
    for (int r = 0; r < R && ok; ++r) ok = all[r].ok != 0;
  }
  dsend.release();
  drecv.release();
  if (!ok) {  // every rank arrives here alike: the two-kernel path (own frees the buffer)
    for (void* p : h->ipc_open) (void)hipIpcCloseMemHandle(p);
    h->ipc_open.clear();
    return rc;
  }
  h->ipc_own = std::move(own);
  unsigned long long* dtab = nullptr;
  TRY(h->pool.alloc(&dtab, tab.size(), h->st));
  // on the handle's stream, behind the pool's zero fill there (a null-stream copy is not ordered
  // after it: the fill could land last and leave null peer pointers)
  LOAM_HIP(hipMemcpyAsync(dtab, tab.data(), sizeof(unsigned long long) * tab.size(), hipMemcpyHostToDevice, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  D.ipc_tab = dtab;
  D.ipc_B = (int)B;
  return LOAM_OK;
}

static int32_t mapper_create(const loam_params* p, int32_t device, int32_t n_streams, loam_comm* comm,
                             loam_mapper** out) {
  if (!out || n_streams <= 0) {
    set_error("loam_mapper_create: bad arguments");
    return LOAM_ERR_ARG;
  }
  *out = nullptr;
  if (p) {
    // the VoxelGrid leaves as the kernels see them (float): finite and positive.  Small positive
    // leaves are PCL's business (its "leaf size is too small" rule, voxel.h)
    for (const double leaf : {p->mapping_line_resolution, p->mapping_plane_resolution})
      if (!std::isfinite(leaf) || !(leaf < 3.0e38) || !((float)leaf > 0.f)) {
        set_error("loam_mapper_create: mapping_line_resolution / mapping_plane_resolution must be finite and > 0");
        return LOAM_ERR_ARG;
      }
  }
  TRY(ensure_device(device));
  LOAM_HIP(hipSetDevice(device));
  vh_spin_limit_from_env(device);
  lm_peer_spin_limit_from_env(device);
  std::unique_ptr<loam_mapper> hold(new loam_mapper);
  loam_mapper* const h = hold.get();
  if (p) h->P = *p; else loam_params_default(&h->P);
  h->dev = device;
  h->B = n_streams;
  h->comm = comm;
  MapperDev& D = h->D;
  D.B = n_streams;
  if (comm) {
    D.sharded = 1;
    D.rank = comm->rank;
    D.nrank = comm->size;
  }
  D.max_in = h->P.max_input_points;
  D.map_cap = h->P.max_map_points;
  D.sub_cap = h->P.max_submap_points;
  D.scratch_cap = D.sub_cap + D.max_in;
  {
    const uint64_t cap = (uint64_t)D.map_cap, margin = (uint64_t)D.sub_cap + 2ull * D.max_in;
    h->compact_at = (uint32_t)std::max<uint64_t>(cap / 2, cap > margin ? cap - margin : 0);
    D.compact_at = h->compact_at;
    D.compact_due_at = h->compact_at;
  }
  D.max_chunks = LM_EBLK;
  {
    // k_lm_round: G workgroups per stream, B * G <= CUs x blocks/CU so that one launch fits the
    // GPU (speed only: the shares are claimed by whichever workgroups run, lm.h, so handles
    // sharing the GPU cannot deadlock).  LOAM_LM_PERSISTENT=0 selects the two-kernel path
    // (tests cover both).
    int occ = 0, cus = 0;
    const char* env = std::getenv("LOAM_LM_PERSISTENT");
    const bool allow = !(env && env[0] == '0');
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      h->n_cu = cus;
    // sharded over several ranks: ranks of one process (loam_comm_create_local) meet inside the
    // persistent round (peer slots, lm.h); other transports all-reduce between two kernels per
    // pass.  At one rank every collective is the identity and the round stays one launch.
    const bool peer = comm && comm->size > 1 && comm->kind == 2;
    // ranks in separate processes: the same persistent round, meeting in IPC-mapped peer buffers
    // (ipc_peer_setup, below, once the stream exists; LOAM_PEER_LM=0 keeps the two-kernel path)
    const char* ienv = std::getenv("LOAM_PEER_LM");
    const bool ipc = comm && comm->size > 1 && comm->kind != 2 && !(ienv && ienv[0] == '0');
    h->want_ipc = false;
    if (allow && (!comm || comm->size == 1 || peer || ipc) &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_lm_round, LM_THREADS, 0) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) {
      // 256 threads x 256 VGPRs: exactly one block per CU; the API can over-report by one
      // block per CU at some SGPR counts (MI355X_MICROARCH.md, correctness boundaries)
      occ = std::min(occ, 1);
      const int cap = occ * cus;
      // 16 at one stream: LM pass 26.5k -> 24.9k cycles once the leader loads the share partials
      // 8 at a time (4 / 8 / 12 / 16: 30.8k / 26.5k / 25.6k / 24.9k, tools/dbg_lm.py)
      // (with peer ranks on this device every rank's round must fit at once: a leader waits for
      // the other ranks' leaders)
      h->lm_G = std::min(LM_EBLK, std::min(16, cap / (peer ? lm_padded(n_streams) * comm->size : n_streams)));
      const char* genv = std::getenv("LOAM_LM_G");  // measurement override
      if (genv && std::atoi(genv) > 0) h->lm_G = std::min(LM_EBLK, std::atoi(genv));
      // cross-process ranks: every rank's leaders wait for each other; they fit even if every rank
      // shared this device (the test's two processes on one GPU); the members are claimed (lm.h)
      if (ipc && h->lm_G > 0) {
        if (lm_padded(n_streams) * comm->size <= cap) h->want_ipc = true;
        else h->lm_G = 0;
      }
      if (peer && h->lm_G > 0) {
        const size_t nd = (size_t)2 * n_streams * 2 * comm->size * LM_MAX_PASSES * LM_NACC;
        void* pb = nullptr;
        // the leaders (R x Bp) reserved against the device's LM capacity with every other group of
        // this process: all of them must fit at once (comm.hip); else the two-kernel path
        if (comm_peer_buffer(comm, nd * sizeof(double) + (size_t)n_streams * 2 * comm->size * sizeof(uint32_t),
                             lm_padded(n_streams) * comm->size, cap, &pb) == LOAM_OK) {
          D.lm_peer = static_cast<double*>(pb);
          D.lm_peer_flag = reinterpret_cast<uint32_t*>(D.lm_peer + nd);
        } else {
          h->lm_G = 0;  // the two-kernel path
        }
      }
    }
  }
  D.pcl_order = h->P.exact_voxel_order ? 1 : 0;
  // few streams: the input-order stack VoxelGrid over 8 workgroups per (stream, map)
  // (k_stack_part; 4 / 6 / 12 ranges measured slower)
  D.stack_k = (n_streams <= 4 && !D.pcl_order) ? 8 : 0;
  if (const char* kenv = std::getenv("LOAM_STACK_K"))  // measurement override (parts per stack)
    if (D.stack_k) D.stack_k = std::max(1, std::min(STACK_K_MAX, std::atoi(kenv)));
  D.leaf[0] = (float)h->P.mapping_line_resolution;
  D.leaf[1] = (float)h->P.mapping_plane_resolution;
  const size_t B = n_streams;
  auto alloc = [&](auto& ptr, size_t n) { return h->pool.alloc(&ptr, n, h->st); };
  TRY(h->st.create());
  TRY(h->st2.create());
  TRY(h->ev_opt_begin.create());
  TRY(h->ev_opt_end.create());
  TRY(h->ev_stack.create(hipEventDisableTiming));
  for (ParitySlot& S : h->slot) {
    TRY(S.ev_sin.create(hipEventDisableTiming));
    TRY(S.ev_fr[0].create());
    TRY(S.ev_fr[1].create());
  }
  {
    const char* denv = std::getenv("LOAM_DEFER_EVERY");  // tests: force the deferral path
    D.defer_every = denv ? std::max(0, std::atoi(denv)) : 0;
  }
  // graphs pay off where launch gaps are the cost (B = 1: 0.750 -> 0.733 ms per frame); with
  // two handles of 64 streams, graph launches measured 20% slower (375k vs 470k iterations/s)
  h->use_graph = n_streams <= 4 ? 1 : 0;
  // cell split at few streams: B = 1 correspondence search 67.8 -> 35.6 us per round (8 lanes;
  // 4 lanes 43.4, 16 lanes 41.3, 2 lanes per query splitting the points 0.19 ms per frame); at
  // B = 128 it costs 1.2x (more lanes idle on pruned cells): one lane per query there
  h->knn_cs = n_streams <= 4 ? 8 : 0;
  D.knn_blk = n_streams <= 4 ? 4 * CORR_BLK : CORR_BLK;
  if (const char* benv = std::getenv("LOAM_KNN_BLK"))  // measurement override (cell-split workgroups per stream)
    if (h->knn_cs) D.knn_blk = std::max(1, std::min(64 * CORR_BLK, std::atoi(benv)));
  TRY(alloc(D.fr, B));
  for (int m = 0; m < 2; ++m) {
    TRY(alloc(D.in_pts[m], B * D.max_in));
    for (ParitySlot& S : h->slot) TRY(alloc(S.stack_buf[m], B * D.max_in));
  }
  TRY(alloc(D.arena, B * 2 * 2 * (size_t)D.map_cap));
  TRY(alloc(D.carena, B * 2 * 2 * (size_t)D.map_cap));
  TRY(alloc(D.ctab, B * 2 * 2 * 4 * (size_t)D.map_cap));
  TRY(alloc(h->cube_tab[0], B * 2 * NCUBE));
  TRY(alloc(h->cube_tab[1], B * 2 * NCUBE));
  TRY(alloc(D.extra_flag, B * 2 * NCUBE));
  D.knn_stride = B * 2 * (size_t)D.max_in;
  TRY(alloc(D.knn_id, 5 * D.knn_stride));
  TRY(alloc(D.r_type, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.r_px, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.r_py, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.r_pz, B * 2 * (size_t)D.max_in));
  for (int k = 0; k < 3; ++k) {
    TRY(alloc(D.r_a[k], B * 2 * (size_t)D.max_in));
    TRY(alloc(D.r_b[k], B * 2 * (size_t)D.max_in));
  }
  TRY(alloc(D.ins_pts, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.ins_tag, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.ins_sorted, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.ins_off, B * 2 * (size_t)(INS_SLOTS + 1)));
  TRY(alloc(D.stable_tok, B * 2 * (size_t)NCUBE));
  TRY(alloc(h->tok_tmp, B * 2 * (size_t)NCUBE));
  {
    // cell occupancy blocks: a pool of OCC_POOL per (stream, map) (sized from the window).  LOAM_KNN_OCC=0:
    // no cube has a block, k_knn probes every cell (A/B runs, tests); LOAM_KNN_OCC_BLOCKS: a smaller
    // pool (tests of the exhausted pool)
    const char* oenv = std::getenv("LOAM_KNN_OCC");
    const char* benv = std::getenv("LOAM_KNN_OCC_BLOCKS");
    // handles of few streams search with the cell-split kernel, which does not read the blocks: none built
    D.occ_blocks = (h->knn_cs || (oenv && oenv[0] == '0')) ? 0 : OCC_POOL;
    if (D.occ_blocks && benv) D.occ_blocks = std::max(1, std::min(OCC_POOL, std::atoi(benv)));
    TRY(alloc(D.cube_occ, B * 2 * (size_t)NCUBE));
    TRY(alloc(h->occ_tmp, B * 2 * (size_t)NCUBE));
    TRY(alloc(D.occ_used, B * 2 * (size_t)OCC_USED_WORDS));
    TRY(alloc(D.occ_pool, B * 2 * (size_t)D.occ_blocks * CI_OCC_WORDS));
  }
  TRY(alloc(D.dbg, LOAM_DEBUG_COUNTERS));
  {  // phase cycle counters (readcyclecounter + device-scope atomics in the kernels): diagnostics only
    const char* penv = std::getenv("LOAM_PHASE_COUNTERS");
    D.pdbg = (penv && std::atoi(penv) > 0) ? D.dbg : nullptr;
  }
  TRY(alloc(D.vx_pts, B * 2 * (size_t)D.scratch_cap));
  if (D.pcl_order) {
    const size_t ps = mp_scratch(D);
    TRY(alloc(D.pe, B * 2 * ps));
    TRY(alloc(D.pa, B * 2 * ps));
    TRY(alloc(D.pb, B * 2 * ps));
    TRY(alloc(D.ps, B * 2 * ps));
    TRY(alloc(D.pseg, B * 2 * (mp_pseg(ps) + 9)));
  }
  TRY(alloc(D.vx_idx, B * 2 * (size_t)D.scratch_cap));
  TRY(alloc(D.stk_part, B * 2 * (size_t)STACK_K_MAX));
  for (ParitySlot& S : h->slot) {
    TRY(alloc(S.stk_n_buf, B * 2));
    TRY(alloc(S.stk_err_buf, B));
    // few streams: the stack inputs in page-locked host memory the stack kernels read in place
    // (mapped), no H2D copy ahead of the stack VoxelGrid, which heads the blocking frame's critical
    // path; many streams: a device copy (256 workgroups reading host memory cost the stack family
    // ~0.05 ms per step at B = 128, profiles/r6_member_chunks_ab.txt)
    if (B <= 4) {
      TRY(S.hsin.assign_mapped(B, StackIn{}, &S.sin_buf));
    } else {
      TRY(alloc(S.sin_buf, B));
      TRY(S.hsin.assign(B, StackIn{}));
    }
  }
  bind_stack_parity(h, D, 0);
  TRY(alloc(h->d_stk_ready, 2));
  TRY(alloc(D.stk_pts, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.stk_idx, B * 2 * (size_t)D.max_in));
  TRY(alloc(D.partials, B * (size_t)D.max_chunks * LM_NACC));
  TRY(alloc(D.lm_sync, B * 2 * LM_SYNC_WORDS));
  TRY(alloc(D.lm_xpub, B * 2 * 8));
  TRY(alloc(D.tickets, B));
  TRY(alloc(D.lm_tick, B));
  D.rq_cap = B * 2 * INS_SLOTS;
  TRY(alloc(D.rq, (size_t)RQ_CLASSES * D.rq_cap));
  TRY(alloc(D.rq_ctl, RQ_CLASSES));
  TRY(alloc(h->d_map_off, 2 * NCUBE + 1));
  TRY(alloc(h->d_new_off, B * 2 * (NCUBE + 1)));
  if (D.sharded) {
    for (int m = 0; m < 2; ++m) D.blk_v[m] = shard_block_voxels(D.leaf[m]);
    const size_t nq = B * 2 * (size_t)D.max_in;
    NnRec* recv = nullptr;
    TRY(alloc(D.wcnt, B * 2 * (size_t)WIN_MAX));
    TRY(alloc(D.nn_send, nq));
    if (D.nrank > 1) {
      TRY(alloc(recv, nq * D.nrank));
      D.nn_recv = recv;
    } else {
      D.nn_recv = D.nn_send;  // one rank: the all-gather is the identity
    }
    TRY(alloc(D.nn_xyz, 5 * nq));
    TRY(alloc(D.lm_red, B * (size_t)LM_NACC));
    TRY(alloc(D.pose_x, (size_t)D.nrank * B * 8));
    TRY(alloc(h->d_q_off, B + 1));
    D.q_off = h->d_q_off;
    TRY(h->q_off.assign(2 * (B + 1), 0));  // [parity][B + 1]
    if (D.nrank == 1) {  // fixed query slots: no per-frame host read of the stack sizes
      for (size_t s = 0; s <= B; ++s) h->q_off[s] = (int)(s * 2 * (size_t)D.max_in);
      LOAM_HIP(hipMemcpyAsync(h->d_q_off, h->q_off.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice, h->st));
    }
  }
  D.cube_tab = h->cube_tab[0];
  TRY(h->hf.assign(B, StreamFrame{}));
  for (ParitySlot& S : h->slot) {
    TRY(S.hfo.assign_mapped(B, StreamFrame{}, &S.hfo_dev));
    TRY(S.fin.assign_mapped(B, FrameIn{}, &S.fin_dev));
    TRY(S.hfo_early.assign_mapped(B, StreamFrame{}, &S.hfo_early_dev));
  }
  TRY(h->done.assign_mapped(2, 0ull, &h->done_dev));
  TRY(h->done_early.assign_mapped(2, 0ull, &h->done_early_dev));
  h->hs.assign(B, HostStream{});
  h->last_tail.assign(B, std::array<uint32_t, 2>{0u, 0u});
  for (size_t s = 0; s < B; ++s) h->hf[s] = fresh_record();
  LOAM_HIP(hipStreamSynchronize(h->st));  // zero-fills done
  if (h->want_ipc) {  // collective: every rank of the comm creates its mapper
    TRY(ipc_peer_setup(h));
    if (!D.ipc_tab) h->lm_G = 0;  // some rank could not map the buffers: the two-kernel path
  }
  *out = hold.release();
  return LOAM_OK;
}

int32_t loam_mapper_create(const loam_params* p, int32_t device, int32_t n_streams, loam_mapper** out) {
  return mapper_create(p, device, n_streams, nullptr, out);
}

int32_t loam_mapper_create_sharded(const loam_params* p, int32_t device, int32_t n_streams, loam_comm* comm,
                                   loam_mapper** out) {
  if (!comm) {
    set_error("loam_mapper_create_sharded: null comm");
    return LOAM_ERR_ARG;
  }
  return mapper_create(p, device, n_streams, comm, out);
}

int32_t loam_shard_owner(const float* xyz, float leaf, int32_t nrank) {
  if (!xyz || !(leaf > 0.f) || nrank < 1) return LOAM_ERR_ARG;
  return shard_owner(xyz[0], xyz[1], xyz[2], 1.0f / leaf, shard_block_voxels(leaf), nrank);
}

static int32_t finish_oldest(loam_mapper* h);
static int32_t settle_all(loam_mapper* h);
static bool chain_capable(const loam_mapper* h);
// every frame in flight is finished before anything reads or changes the handle's state
#define SETTLE(h)                                \
  do {                                           \
    if ((h) && !(h)->q.empty()) {                \
      LOAM_HIP(hipSetDevice((h)->dev));          \
      TRY(settle_all(h));                        \
    }                                            \
  } while (0)
// the result calls (pose, stats, state, iterations) report the newest finished frame: they finish
// the oldest frame in the queue unless it was given behind another (whose results they report)
#define SETTLE_RESULTS(h)                                                                   \
  do {                                                                                      \
    if ((h) && !(h)->q.empty() && !(h)->q.front().behind && !(h)->q.front().early_seen) { \
      LOAM_HIP(hipSetDevice((h)->dev));                                                     \
      TRY(finish_oldest(h));                                                                \
    }                                                                                       \
  } while (0)

int32_t loam_mapper_destroy(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  (void)hipSetDevice(h->dev);
  while (!h->q.empty()) (void)finish_oldest(h);
  delete h;
  return LOAM_OK;
}

int32_t loam_mapper_reset(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  SETTLE(h);
  LOAM_HIP(hipSetDevice(h->dev));
  LOAM_HIP(hipStreamSynchronize(h->st2));  // stacks queued ahead are dropped with their inputs
  for (int p = 0; p < 2; ++p)
    LOAM_HIP(hipMemsetAsync(h->cube_tab[p], 0, sizeof(uint2) * h->B * 2 * NCUBE, h->st));
  LOAM_HIP(hipMemsetAsync(h->D.stable_tok, 0, sizeof(uint32_t) * h->B * 2 * NCUBE, h->st));
  LOAM_HIP(hipMemsetAsync(h->D.cube_occ, 0, sizeof(uint32_t) * h->B * 2 * NCUBE, h->st));
  LOAM_HIP(hipMemsetAsync(h->D.occ_used, 0, sizeof(uint32_t) * h->B * 2 * OCC_USED_WORDS, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  for (int s = 0; s < h->B; ++s) {
    h->hf[s] = fresh_record();
    h->last_tail[s] = {0u, 0u};
    h->hs[s] = HostStream{};
  }
  return LOAM_OK;
}

// LaserMapping::input (laser_mapping.cpp:178-209): the clouds and odometry pose of the next
// solve.  Kept apart from a frame in flight (loam_mapper_solve_async): the solve that takes it
// computes the initial guess (:206-207) once the previous frame's transformUpdate is known.
static int32_t mapper_input_common(loam_mapper* h, int32_t s, const float* corner, int32_t nc,
                                   const float* surf, int32_t ns, const double* q_wodom,
                                   const double* t_wodom, int32_t skip, hipMemcpyKind kind) {
  TRY(check_stream(h, s));
  if (!q_wodom || !t_wodom || nc < 0 || ns < 0 || (nc > 0 && !corner) || (ns > 0 && !surf)) {
    set_error("loam_mapper_input: bad arguments");
    return LOAM_ERR_ARG;
  }
  if (nc > h->D.max_in || ns > h->D.max_in) {
    set_error("loam_mapper_input: cloud larger than max_input_points");
    return LOAM_ERR_CAPACITY;
  }
  LOAM_HIP(hipSetDevice(h->dev));
  HostStream& H = h->hs[s];
  if (skip) {  // laser_mapping.cpp:197-201: high-frequency pose only (needs the last transformUpdate)
    SETTLE(h);
    for (int i = 0; i < 4; ++i) H.q_wodom[i] = q_wodom[i];
    for (int i = 0; i < 3; ++i) H.t_wodom[i] = t_wodom[i];
    H.skip = true;
    double pose[7];
    host_initial_guess(H, pose);
    unpack7(pose, H.q_hf, H.t_hf);
    H.in_ready = false;
    H.stk_launched = false;
    return LOAM_OK;
  }
  if (kind == hipMemcpyHostToDevice) {
    // LaserMapping::input deep-copies the clouds (:188-190); on the stack stream, after any
    // stack still reading the staging buffer
    H.in_p[0] = h->D.in_pts[0] + (size_t)s * h->D.max_in;
    H.in_p[1] = h->D.in_pts[1] + (size_t)s * h->D.max_in;
    if (nc) LOAM_HIP(hipMemcpyAsync((void*)H.in_p[0], corner, sizeof(float4) * nc, kind, h->st2));
    if (ns) LOAM_HIP(hipMemcpyAsync((void*)H.in_p[1], surf, sizeof(float4) * ns, kind, h->st2));
  } else {
    // HBM-resident clouds are read in place: they must stay valid until the stack VoxelGrid has
    // read them (loam_mapper_solve returns, or the wait after loam_mapper_solve_async)
    H.in_p[0] = reinterpret_cast<const float4*>(corner);
    H.in_p[1] = reinterpret_cast<const float4*>(surf);
  }
  H.in_n[0] = nc;
  H.in_n[1] = ns;
  for (int i = 0; i < 4; ++i) H.in_q[i] = q_wodom[i];
  for (int i = 0; i < 3; ++i) H.in_t[i] = t_wodom[i];
  H.skip = false;
  H.in_ready = true;
  H.stk_launched = false;
  return LOAM_OK;
}

int32_t loam_mapper_input(loam_mapper* h, int32_t s, const float* corner, int32_t nc, const float* surf,
                          int32_t ns, const double* q_wodom, const double* t_wodom, int32_t skip) {
  return mapper_input_common(h, s, corner, nc, surf, ns, q_wodom, t_wodom, skip, hipMemcpyHostToDevice);
}

int32_t loam_mapper_input_device(loam_mapper* h, int32_t s, const float* corner, int32_t nc,
                                 const float* surf, int32_t ns, const double* q_wodom,
                                 const double* t_wodom, int32_t skip) {
  return mapper_input_common(h, s, corner, nc, surf, ns, q_wodom, t_wodom, skip, hipMemcpyDeviceToDevice);
}

// HIP events around each launch when profiling is on (accumulated per kernel family)
static int32_t prof_begin(loam_mapper* h, int fam, hipEvent_t* stop, hipStream_t st) {
  *stop = nullptr;
  if (!h->prof) return LOAM_OK;
  size_t k = h->ev_fam.size() * 2;
  while (h->ev_pool.size() < k + 2) {
    DevEvent e;
    TRY(e.create());
    h->ev_pool.push_back(std::move(e));
  }
  h->ev_fam.push_back(fam);
  *stop = h->ev_pool[k + 1];
  LOAM_HIP(hipEventRecord(h->ev_pool[k], st));
  return LOAM_OK;
}
// the stop event of a timed launch: recorded by end(), or, when the launch body returns early (a
// TRY inside it), by the destructor, so no listed (start, stop) pair is left without its stop
struct ProfStop {
  hipEvent_t ev = nullptr;
  hipStream_t st = nullptr;
  hipError_t end() {
    const hipError_t e = ev ? hipEventRecord(ev, st) : hipSuccess;
    ev = nullptr;
    return e;
  }
  ~ProfStop() { (void)end(); }
};
#define LAUNCH_ON(stream, fam, ...)                     \
  do {                                                  \
    ProfStop stop_;                                     \
    stop_.st = (stream);                                \
    TRY(prof_begin(h, (fam), &stop_.ev, (stream)));      \
    __VA_ARGS__;                                        \
    LOAM_HIP(stop_.end());                              \
  } while (0)
#define LAUNCH(fam, ...) LAUNCH_ON(h->st, fam, __VA_ARGS__)

int32_t loam_mapper_input_device_batch(loam_mapper* h, int32_t n, const int32_t* streams,
                                       const uint64_t* d_corner, const int32_t* n_corner,
                                       const uint64_t* d_surf, const int32_t* n_surf,
                                       const double* q_wodom, const double* t_wodom) {
  if (!h || n < 0 || (n > 0 && (!streams || !d_corner || !n_corner || !d_surf || !n_surf || !q_wodom || !t_wodom))) {
    set_error("loam_mapper_input_device_batch: bad arguments");
    return LOAM_ERR_ARG;
  }
  for (int i = 0; i < n; ++i) {
    int32_t rc = mapper_input_common(h, streams[i], reinterpret_cast<const float*>(d_corner[i]), n_corner[i],
                                     reinterpret_cast<const float*>(d_surf[i]), n_surf[i], q_wodom + 4 * i,
                                     t_wodom + 3 * i, 0, hipMemcpyDeviceToDevice);
    if (rc != LOAM_OK) return rc;
  }
  return LOAM_OK;
}

int32_t loam_mapper_lm_path(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  if (h->lm_G <= 0) return 0;
  if (h->D.lm_peer) return 2;
  if (h->D.ipc_tab) return 3;
  return 1;
}

int64_t loam_mapper_total_iterations(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  SETTLE_RESULTS(h);
  int64_t it = 0;
  for (int s = 0; s < h->B; ++s)
    if (h->hs[s].solved_last) it += h->hs[s].st.lm[0].iterations + h->hs[s].st.lm[1].iterations;
  return it;
}

int32_t loam_mapper_stats_all(loam_mapper* h, loam_map_stats* out, int32_t n) {
  SETTLE_RESULTS(h);
  if (!h || !out || n < 0 || n > h->B) return LOAM_ERR_ARG;
  for (int s = 0; s < n; ++s) out[s] = h->hs[s].st;
  return LOAM_OK;
}

// The stack VoxelGrids (laser_mapping.cpp:492-500) of every stream whose input has none queued
// yet, in one launch on the stack stream, into the stack buffers of the next frame's parity.
// They read only the frame's body-frame input, so they may run beside a frame in flight.
static int32_t launch_stacks(loam_mapper* h) {
  const int par = h->spar, B = h->B;
  for (const FrameRec& R : h->q)  // that parity's stack buffers still belong to a frame in flight
    if (R.fpar == par) return LOAM_OK;
  bool any = false;
  ParitySlot& S = h->slot[par];
  LOAM_HIP(hipEventSynchronize(S.ev_sin));  // the last reads of its hsin are done
  StackIn* in = S.hsin.data();
  for (int s = 0; s < B; ++s) {
    HostStream& H = h->hs[s];
    const bool go = H.in_ready && !H.stk_launched;
    in[s].active = go ? 1 : 0;
    if (!go) continue;
    any = true;
    H.stk_launched = true;
    H.stk_seq = h->stack_seq + 1;
    for (int m = 0; m < 2; ++m) {
      in[s].p[m] = H.in_p[m];
      in[s].n[m] = H.in_n[m];
    }
  }
  if (!any) return LOAM_OK;
  const unsigned long long seq = ++h->stack_seq;
  MapperDev D = h->D;
  bind_stack_parity(h, D, par);
  hipStream_t s2 = h->st2;
  if (h->B > 4) LOAM_HIP(hipMemcpyAsync(S.sin_buf, in, sizeof(StackIn) * B, hipMemcpyHostToDevice, s2));
  if (D.stack_k) {
    LAUNCH_ON(s2, FAM_STACK, k_stack_part<<<B * 2 * D.stack_k, VX_THREADS, 0, s2>>>(D));
    LAUNCH_ON(s2, FAM_STACK, k_stack_cat<<<B * 2, VX_THREADS, 0, s2>>>(D));
  } else {
    if (D.pcl_order) LAUNCH_ON(s2, FAM_STACK, k_stack_ds<true><<<B * 2, VX_THREADS, 0, s2>>>(D));
    else LAUNCH_ON(s2, FAM_STACK, k_stack_ds<false><<<B * 2, VX_THREADS, 0, s2>>>(D));
  }
  k_stack_done<<<1, 64, 0, s2>>>(h->d_stk_ready + par, seq);
  LOAM_HIP(hipGetLastError());
  LOAM_HIP(hipEventRecord(S.ev_sin, s2));  // (hsin is read, in place or by the copy, until here)
  LOAM_HIP(hipEventRecord(h->ev_stack, s2));
  return LOAM_OK;
}

int32_t loam_mapper_prefetch(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  return launch_stacks(h);
}

// k_revox workgroups: one per possible item
static int revox_grid(const loam_mapper* h) { return h->B * 2 * INS_SLOTS; }
// the frame's re-VoxelGrid
static void launch_revox(const loam_mapper* h, const MapperDev& D, hipStream_t st) {
  if (D.pcl_order) k_revox<true><<<revox_grid(h), VX_THREADS, 0, st>>>(D);
  else k_revox<false><<<revox_grid(h), VX_THREADS, 0, st>>>(D);
}
// the exact 5-NN of one round: 8 lanes per query splitting the cells, or one lane per query
static void launch_knn(const loam_mapper* h, const MapperDev& D, int round, hipStream_t st) {
  if (h->knn_cs) k_knn<8, true><<<h->B * D.knn_blk, CORR_THREADS, 0, st>>>(D, round);
  else k_knn<1><<<h->B * CORR_BLK, CORR_THREADS, 0, st>>>(D, round);
}
// compaction of the arenas whose tail is past due_at (each workgroup checks its own pair's), queued
// ahead of a frame so that the host never waits on it
static int32_t launch_compaction(const loam_mapper* h, const MapperDev& D, uint32_t due_at, hipStream_t st) {
  const int B = h->B;
  MapperDev Dc = D;
  Dc.compact_due_at = due_at;
  k_compact_scan<<<B * 2, VX_THREADS, 0, st>>>(Dc, h->d_new_off);
  k_compact_copy<<<dim3(128, B * 2), 256, 0, st>>>(Dc, h->d_new_off);
  k_compact_commit<<<B * 2, 256, 0, st>>>(Dc, h->d_new_off);
  LOAM_HIP(hipGetLastError());
  return LOAM_OK;
}

// the frame's kernel sequence for the hipGraph path: k_frame_prep (records of a queued frame,
// stack sizes, submap offsets), 2 x (kNN, geometry, LM round), insertion, re-VoxelGrid, and the
// records back to the D2H buffer of the frame's stack parity.  Every kernel argument is fixed per
// (cube-table parity, stack parity): the frame's values travel in the records and FrameIn.
static void capture_frame(loam_mapper* h, const MapperDev& D, int fpar, hipStream_t st) {
  const int B = h->B;
  k_frame_prep<<<B, 128, 0, st>>>(D);
  for (int round = 0; round < 2; ++round) {
    launch_knn(h, D, round, st);
    k_geom<<<B * CORR_BLK, CORR_THREADS, 0, st>>>(D, round);
    k_lm_round<<<lm_padded(B) * h->lm_G, LM_THREADS, 0, st>>>(D, round, h->lm_G);
  }
  // (loam_mapper_solve_pose) the final poses and the frame's stats are in the records now
  if (h->early) k_frame_out<<<1, 256, 0, st>>>(D, h->slot[fpar].hfo_early_dev, h->done_early_dev + fpar);
  k_insert_bucket<<<B * 2, VX_THREADS, 0, st>>>(D);
  launch_revox(h, D, st);
  k_frame_out<<<1, 256, 0, st>>>(D, h->slot[fpar].hfo_dev, h->done_dev + fpar);
}

// The pending inputs become the frame R, of the next stack parity (h->spar): every stream with an
// input, whose stack VoxelGrid launch_stacks has queued into that parity's buffers.
static int32_t take_inputs(loam_mapper* h, FrameRec& R) {
  R = FrameRec(h->B, h->spar);
  for (int s = 0; s < h->B; ++s) {
    HostStream& H = h->hs[s];
    if (!H.in_ready) continue;
    if (!H.stk_launched) {
      set_error("loam_mapper: stack buffers of the frame's parity still in use");
      return LOAM_ERR_ARG;
    }
    R.active[s] = 1;
    pack7(H.in_q, H.in_t, R.wodom[s].data());
    R.in_p[s] = {H.in_p[0], H.in_p[1]};
    R.in_n[s] = {H.in_n[0], H.in_n[1]};
    R.stk_seq[s] = H.stk_seq;
    H.in_ready = false;
    H.stk_launched = false;
  }
  return LOAM_OK;
}

// Enqueue one solveMapping of the streams active in R, which holds what they were given and the
// stack parity of their stacks (the work of loam_mapper_solve up to the host bookkeeping, which
// mapper_finish_rec does).  chained: queued behind the frame in flight, whose results the host
// does not have yet: the device prepares the stream records (k_frame_prep) from what that frame
// left, and only the graph path runs.
static int32_t enqueue_frame(loam_mapper* h, bool chained, FrameRec& R) {
  MapperDev& D = h->D;
  const int B = h->B;
  const int fpar = R.fpar;
  ParitySlot& S = h->slot[fpar];
  bind_stack_parity(h, D, fpar);
  D.fin = S.fin_dev;
  D.stk_ready = h->d_stk_ready + fpar;
  R.chained = chained;
  R.pending = false;
  R.seq = ++h->seq;
  h->frame_counter++;
  R.epoch = D.epoch = h->frame_counter;
  D.cube_tab = h->cube_tab[h->parity];
  hipStream_t st = h->st;
  FrameIn* fin = S.fin.data();
  for (int s = 0; s < B; ++s) {  // mode 0: the records as uploaded; mode 1: prepared on the device
    FrameIn& I = fin[s];
    I = FrameIn{};
    I.epoch = h->frame_counter;
    I.active = R.active[s];
    I.stack_seq = R.stk_seq[s];
    if (!chained) continue;
    I.mode = 1;
    for (int i = 0; i < 7; ++i) I.wodom[i] = R.wodom[s][i];
    for (int m = 0; m < 2; ++m) {
      I.in_ptr[m] = R.in_p[s][m];
      I.n[m] = R.in_n[s][m];
    }
  }
  if (!chained) {
    // the host prepares the records: initial guess (:206-207), centerCube + recentering
    // (:228-444), window (:455-472)
    for (int s = 0; s < B; ++s) {
      StreamFrame& F = h->hf[s];
      const HostStream& H = h->hs[s];
      frame_reset(F);
      F.active = R.active[s];
      if (!F.active) continue;  // (a stream deferred in a frame still in flight stays deferred)
      F.deferred = 0;
      pack7(H.q_wmap_wodom, H.t_wmap_wodom, F.wmap);
      for (int i = 0; i < 7; ++i) F.wodom[i] = R.wodom[s][i];
      pose_initial_guess(F.wmap, F.wodom, F.pose);
      frame_center(F.pose, F.cen, F.center, F.shift);
      frame_window(F);
      F.epoch = h->frame_counter;
      F.in_ptr[0] = R.in_p[s][0];
      F.in_ptr[1] = R.in_p[s][1];
      F.nc_in = R.in_n[s][0];
      F.ns_in = R.in_n[s][1];
    }
  }
  bool any_shift = false;
  for (int s = 0; s < B && !chained; ++s)
    any_shift |= h->hf[s].active && (h->hf[s].shift[0] || h->hf[s].shift[1] || h->hf[s].shift[2]);
  // arenas past the compaction threshold are compacted ahead of this frame.  With frames queued
  // behind each other, a little early (the threshold less three frames' growth) so that queued
  // frames rarely meet a due compaction (they would be deferred); the moves are verbatim, the
  // results do not depend on when they happen.
  uint32_t due_at = h->compact_at;
  if (chain_capable(h)) {
    const uint64_t ahead = 3ull * h->grow_max + 4096ull;
    due_at = (uint32_t)std::max<uint64_t>(h->compact_at / 2, h->compact_at > ahead ? h->compact_at - ahead : 0);
  }
  // (a queued frame: the tails known now are those before the frame in flight, which may add
  // one frame's growth; the kernels test the tails as they are when they run)
  bool compact_due = false;
  const uint64_t unknown = chained ? (uint64_t)h->grow_max : 0ull;
  for (int s = 0; s < B && !compact_due; ++s)
    compact_due = h->hf[s].arena_tail[0] + unknown > due_at || h->hf[s].arena_tail[1] + unknown > due_at;
  const bool graph = chained || (h->use_graph && !h->prof && !any_shift && !D.sharded && h->lm_G > 0);
  R.graph = graph;
  if (graph) {
    hipGraphExec_t& ge = h->gexec[h->parity][fpar];
    // a frame queued behind the one in flight is launched kernel by kernel: a graph launch costs
    // 14 against 6 us between two frames at one stream (rocprofv3 trace); the others as the graph
    const bool direct = chained;
    if (!ge && !direct) {
      hipGraph_t gr = nullptr;
      LOAM_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      capture_frame(h, D, fpar, st);
      LOAM_HIP(hipStreamEndCapture(st, &gr));
      const hipError_t ie = hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0);
      (void)hipGraphDestroy(gr);
      LOAM_HIP(ie);
    }
    if (!chained) LOAM_HIP(hipMemcpyAsync(D.fr, h->hf.data(), sizeof(StreamFrame) * B, hipMemcpyHostToDevice, st));
    // compactions ahead of the graph (a queued frame's k_frame_prep defers if still due)
    if (compact_due) TRY(launch_compaction(h, D, due_at, st));
    // the frame's stacks: waited for by k_frame_prep on the device (stack_seq)
    // a queued frame is not timed: its start is its predecessor's end, and the timing markers
    // between two graph launches would cost the device time
    if (!chained) LOAM_HIP(hipEventRecord(S.ev_fr[0], st));
    if (direct) {
      capture_frame(h, D, fpar, st);
      LOAM_HIP(hipGetLastError());
    } else {
      LOAM_HIP(hipGraphLaunch(ge, st));
    }
    if (!chained) LOAM_HIP(hipEventRecord(S.ev_fr[1], st));
    return LOAM_OK;
  }
  LOAM_HIP(hipMemcpyAsync(D.fr, h->hf.data(), sizeof(StreamFrame) * B, hipMemcpyHostToDevice, st));
  LOAM_HIP(hipEventRecord(S.ev_fr[0], st));
  if (compact_due) TRY(launch_compaction(h, D, due_at, st));
  // the stack VoxelGrids run on the second stream (launch_stacks: at prefetch, or at the start
  // of this solve), overlapping the cube shift and submap preparation; joined before the
  // correspondences
  if (any_shift) {
    LAUNCH(FAM_OTHER, k_shift_cubes<<<dim3(16, B), 256, 0, st>>>(D, h->cube_tab[h->parity],
                                                                 h->cube_tab[1 - h->parity], h->tok_tmp, h->occ_tmp));
    LOAM_HIP(hipMemcpyAsync(D.stable_tok, h->tok_tmp, sizeof(uint32_t) * B * 2 * NCUBE, hipMemcpyDeviceToDevice, st));
    LOAM_HIP(hipMemcpyAsync(D.cube_occ, h->occ_tmp, sizeof(uint32_t) * B * 2 * NCUBE, hipMemcpyDeviceToDevice, st));
    h->parity ^= 1;
    D.cube_tab = h->cube_tab[h->parity];
  }
  const bool multi = D.sharded && D.nrank > 1;  // collectives that are not the identity
  if (D.sharded) {  // the submap sizes over all ranks
    LAUNCH(FAM_OTHER, k_submap_count<<<B, 256, 0, st>>>(D));
    if (multi) TRY(comm_allreduce(h->comm, D.wcnt, (int64_t)B * 2 * WIN_MAX, LOAM_DT_I32, st));
  }
  LAUNCH(FAM_OTHER, k_submap_prep<<<B, 128, 0, st>>>(D));
  LOAM_HIP(hipEventRecord(h->ev_opt_begin, st));
  LOAM_HIP(hipStreamWaitEvent(st, h->ev_stack, 0));
  LAUNCH(FAM_OTHER, k_stack_counts<<<B, 64, 0, st>>>(D));
  size_t q_tot = 0;
  if (multi) {
    // each stream's queries in the exchange: slots sized by the frame's input counts, which the
    // host has without waiting (a VoxelGrid never outputs more points than it reads, :492-500),
    // identical on every rank.  The host array is double-buffered by the frame parity: its copy
    // may still be queued when the next frame is enqueued.
    int* qo = h->q_off.data() + (size_t)fpar * (B + 1);
    for (int s = 0; s < B; ++s) {
      const StreamFrame& F = h->hf[s];
      qo[s] = (int)q_tot;
      if (F.active) q_tot += (size_t)F.nc_in + F.ns_in;
    }
    qo[B] = (int)q_tot;
    LOAM_HIP(hipMemcpyAsync(h->d_q_off, qo, sizeof(int) * (B + 1), hipMemcpyHostToDevice, st));
  }
  for (int round = 0; round < 2; ++round) {
    LAUNCH(FAM_CORR, launch_knn(h, D, round, st));
    if (D.sharded) {  // every rank's candidates -> the exact 5-NN on every rank
      if (multi)
        TRY(comm_allgather(h->comm, D.nn_send, const_cast<NnRec*>(D.nn_recv), (int64_t)(q_tot * sizeof(NnRec)), st));
      LAUNCH(FAM_CORR, k_nn_merge<<<B * CORR_BLK, CORR_THREADS, 0, st>>>(D));
    }
    LAUNCH(FAM_CORR, k_geom<<<B * CORR_BLK, CORR_THREADS, 0, st>>>(D, round));
    if (h->lm_G > 0) {
      if (D.lm_peer) {  // in-process ranks: one launch for every rank's round (k_lm_group)
        LmRankArgs a{D.fr, D.r_type, D.r_px, D.r_py, D.r_pz, {D.r_a[0], D.r_a[1], D.r_a[2]},
                     {D.r_b[0], D.r_b[1], D.r_b[2]}, D.partials, D.lm_sync, D.lm_xpub, D.pdbg,
                     D.max_in, D.max_chunks, B, D.s0};
        LmGroupCtx ctx{round, h->lm_G, D.lm_peer, D.lm_peer_flag};
        LAUNCH(FAM_LM, TRY(comm_group_launch(h->comm, &a, st, lm_group_launch, &ctx)));
      } else {
        LAUNCH(FAM_LM, k_lm_round<<<lm_padded(B) * h->lm_G, LM_THREADS, 0, st>>>(D, round, h->lm_G));
      }
    } else {
      for (int it = 0; it < 5; ++it) {  // iteration 0 + max_num_iterations = 4 candidates
        // sharded: evaluation + this rank's sums (last workgroup), then per Ceres iteration the
        // all-reduce of the 6x6 normal equations
        LAUNCH(FAM_LM, k_lm_eval<<<B * LM_EBLK, LM_THREADS, 0, st>>>(D, round, D.sharded ? 1 : 0));
        if (D.sharded) TRY(comm_allreduce(h->comm, D.lm_red, (int64_t)B * LM_NACC, LOAM_DT_F64, st));
        LAUNCH(FAM_LM, k_lm_step<<<B, 64, 0, st>>>(D, round));
      }
    }
  }
  // pose agreement across ranks before anything is stored (k_pose_adopt); the group LM round
  // (in-process ranks) leaves every rank with the same bits by construction: every rank steps on
  // the same peer slots summed in the same order
  if (D.sharded && !(multi && D.lm_peer && h->lm_G > 0)) {
    LAUNCH(FAM_OTHER, k_pose_publish<<<B, 64, 0, st>>>(D));
    if (multi)
      TRY(comm_allgather(h->comm, D.pose_x + (size_t)D.rank * B * 8, D.pose_x, (int64_t)B * 8 * sizeof(double), st));
    LAUNCH(FAM_OTHER, k_pose_adopt<<<B, 64, 0, st>>>(D));
  }
  LOAM_HIP(hipEventRecord(h->ev_opt_end, st));
  LAUNCH(FAM_INSERT, k_insert_bucket<<<B * 2, VX_THREADS, 0, st>>>(D));
  LAUNCH(FAM_REVOX, launch_revox(h, D, st));
  LOAM_HIP(hipGetLastError());
  LOAM_HIP(hipMemcpyAsync(S.hfo.data(), D.fr, sizeof(StreamFrame) * B, hipMemcpyDeviceToHost, st));
  LOAM_HIP(hipEventRecord(S.ev_fr[1], st));
  return LOAM_OK;
}

static int32_t mapper_replay(loam_mapper* h, const FrameRec& R, const std::vector<int>& redo);

// a queued frame is done when frame_out has written its number to the done word of its parity
// (the words only grow: a later frame of the same parity is not enqueued before this one is
// finished).  The stream is polled for errors while waiting.
static int32_t wait_word(loam_mapper* h, const unsigned long long* word, uint32_t epoch) {
  const volatile unsigned long long* w = word;
  for (uint64_t spins = 0;; ++spins) {
    if (__atomic_load_n(const_cast<const unsigned long long*>(w), __ATOMIC_ACQUIRE) >= epoch) return LOAM_OK;
    if ((spins & 1023) == 1023) {
      const hipError_t e = hipStreamQuery(h->st);
      if (e == hipSuccess) {  // the stream drained: the word must be there now
        if (__atomic_load_n(const_cast<const unsigned long long*>(w), __ATOMIC_ACQUIRE) >= epoch) return LOAM_OK;
        set_error("loam_mapper: frame finished without its done word");
        return LOAM_ERR_HIP;
      }
      if (e != hipErrorNotReady) LOAM_HIP(e);
    }
  }
}
static int32_t wait_done(loam_mapper* h, const FrameRec& R) { return wait_word(h, h->done.data() + R.fpar, R.epoch); }

// a finished frame's stream record -> the stream's stats and cube-grid centre (what
// loam_mapper_stats / _get_state report)
static void frame_stats(const StreamFrame& F, HostStream& H) {
  loam_map_stats& S = H.st;
  S.optimized = F.optimize;
  S.corner_stack = F.nc_stack;
  S.surf_stack = F.ns_stack;
  S.corner_map = F.sub_n[0];
  S.surf_map = F.sub_n[1];
  for (int r = 0; r < 2; ++r) {
    S.corner_num[r] = F.corner_num[r];
    S.surf_num[r] = F.surf_num[r];
    const LmState& L = F.lm[r];
    S.lm[r].iterations = F.optimize ? L.iteration : 0;
    S.lm[r].successful = L.successful;
    S.lm[r].invalid = L.invalid;
    S.lm[r].termination = L.term;
    S.lm[r].initial_cost = L.initial_cost;
    S.lm[r].final_cost = L.min_cost;
  }
  for (int a = 0; a < 3; ++a) {
    S.center[a] = F.center[a];
    H.cen[a] = F.cen[a];
  }
  S.valid_num = F.valid_num;
}

// stream s of frame R has finished with the record F: its pose, the transformUpdate (:147-151)
// and its stats (ms_total, ms_opt, queued and rerun are the caller's)
static void commit_stream(loam_mapper* h, int s, const FrameRec& R, const StreamFrame& F) {
  HostStream& H = h->hs[s];
  for (int i = 0; i < 7; ++i) H.pose[i] = F.pose[i];
  unpack7(R.wodom[s].data(), H.q_wodom, H.t_wodom);
  host_transform_update(H);
  frame_stats(F, H);
}

// the host side of one finished frame: transformUpdate (:147-151), stats, errors, timing.
// replay: a deferred frame run again for some streams (the others keep what their frame gave).
static int32_t mapper_finish_rec(loam_mapper* h, const FrameRec& R, bool replay) {
  const int B = h->B;
  float ms_total = 0, ms_opt = 0;  // (0 for a queued frame: not timed)
  if (R.chained) {
    TRY(wait_done(h, R));
  } else {
    const ParitySlot& S = h->slot[R.fpar];
    LOAM_HIP(hipEventSynchronize(S.ev_fr[1]));
    LOAM_HIP(hipEventElapsedTime(&ms_total, S.ev_fr[0], S.ev_fr[1]));
    if (R.graph) ms_opt = ms_total;  // no event inside the graph (the optimisation block is most of it)
    else LOAM_HIP(hipEventElapsedTime(&ms_opt, h->ev_opt_begin, h->ev_opt_end));
  }
  const StreamFrame* FO = h->slot[R.fpar].hfo.data();
  if (R.seq > h->mirror_seq) {  // the newest records the host has seen
    std::memcpy(h->hf.data(), FO, sizeof(StreamFrame) * B);
    h->mirror_seq = R.seq;
  }
  if (h->prof) {
    // the launches timed so far whose stop event has passed: this frame's, and perhaps a queued
    // frame's stack VoxelGrid (launched beside this one); the others stay listed for a later frame
    size_t kept = 0;
    for (size_t k = 0; k < h->ev_fam.size(); ++k) {
      const hipError_t q = hipEventQuery(h->ev_pool[2 * k + 1]);
      if (q == hipErrorNotReady) {
        std::swap(h->ev_pool[2 * kept], h->ev_pool[2 * k]);
        std::swap(h->ev_pool[2 * kept + 1], h->ev_pool[2 * k + 1]);
        h->ev_fam[kept++] = h->ev_fam[k];
        continue;
      }
      // a pair that cannot be timed (a launch whose enqueue failed between its events) is
      // dropped from the list, not an error of this frame
      float ms = 0;
      if (q != hipSuccess || hipEventElapsedTime(&ms, h->ev_pool[2 * k], h->ev_pool[2 * k + 1]) != hipSuccess) {
        (void)hipGetLastError();
        continue;
      }
      h->fam_ms[h->ev_fam[k]] += ms;
      h->fam_launches[h->ev_fam[k]]++;
    }
    h->ev_fam.resize(kept);
    // algorithmic bytes (DESIGN.md "Kernels"): what each family must read / write
    for (int s = 0; s < B; ++s) {
      const StreamFrame& F = FO[s];
      if (!F.active) continue;
      const double nst = (double)F.nc_stack + F.ns_stack;
      h->fam_bytes[FAM_STACK] += 16.0 * ((double)F.nc_in + F.ns_in + nst);
      h->fam_bytes[FAM_INSERT] += 36.0 * nst;
      if (F.optimize) {
        for (int r = 0; r < 2; ++r) {
          const double ne = F.corner_num[r], npl = F.surf_num[r], ninv = nst - ne - npl;
          const double rec = 60.0 * ne + 44.0 * npl + 4.0 * ninv;
          h->fam_bytes[FAM_CORR] += 16.0 * nst + 16.0 * (double)F.cand[r] + rec;
          h->fam_bytes[FAM_LM] += (double)F.lm[r].passes * rec;
        }
      }
    }
  }
  h->last_spar = R.fpar;
  // host bookkeeping
  int32_t status = LOAM_OK;
  std::vector<int> redo;
  for (int s = 0; s < B; ++s) {
    const StreamFrame& F = FO[s];
    HostStream& H = h->hs[s];
    if (R.active[s] && F.deferred) {  // left to the host (k_frame_prep): run again below
      redo.push_back(s);
      continue;
    }
    if (!replay || R.active[s]) H.solved_last = R.active[s] && F.active;
    if (!R.active[s] || !F.active) continue;
    commit_stream(h, s, R, F);
    H.frame++;
    for (int m = 0; m < 2; ++m) {  // arena growth of one frame (compaction foresight)
      if (F.arena_tail[m] >= h->last_tail[s][m]) h->grow_max = std::max(h->grow_max, F.arena_tail[m] - h->last_tail[s][m]);
      h->last_tail[s][m] = F.arena_tail[m];
    }
    loam_map_stats& S = H.st;
    S.ms_total = ms_total;
    S.ms_opt = ms_opt;
    S.queued = R.chained ? 1 : 0;
    S.rerun = replay ? 1 : 0;
    if (h->prof) h->fam_bytes[FAM_REVOX] += (double)F.vx_bytes;  // counted by k_revox
    if (F.err) {
      // the frame is committed as computed (pose, insertion, re-VoxelGrid ran on the device);
      // the status says it is not trustworthy: the caller resets the stream (include/loam_core.h)
      set_error("loam_mapper_solve: stream " + std::to_string(s) + ": " + map_err_text(F.err));
      const int32_t st = (F.err & (MAP_ERR_LM_SYNC | MAP_ERR_STACK_WAIT | VH_ERR_SPIN)) ? LOAM_ERR_SYNC : LOAM_ERR_CAPACITY;
      if (status == LOAM_OK || st == LOAM_ERR_SYNC) status = st;
    }
  }
  if (!redo.empty()) {
    const int32_t rc = mapper_replay(h, R, redo);
    if (rc != LOAM_OK && (status == LOAM_OK || rc == LOAM_ERR_SYNC)) status = rc;
  }
  return status;
}

// Enqueue, on the host-prepared path, the streams `run` of a frame whose inputs and stack were
// taken earlier (R: a pending frame, or a deferred one to run again): the stack buffers of its
// parity still hold them (no stack is launched into a parity a frame in the queue holds).
static int32_t enqueue_saved(loam_mapper* h, const FrameRec& R, const std::vector<int>& run, FrameRec& out) {
  out = FrameRec(h->B, R.fpar);
  for (int s : run) out.take(s, R);
  return run.empty() ? LOAM_OK : enqueue_frame(h, false, out);
}

// A deferred frame (k_frame_prep found a recentering or compaction due, or followed a deferred
// frame) runs again for its deferred streams on the host-prepared path, with the inputs and the
// stack it was given.  The device work queued after it, if any, left those streams alone (they
// were inactive).
static int32_t mapper_replay(loam_mapper* h, const FrameRec& R, const std::vector<int>& redo) {
  const int B = h->B;
  LOAM_HIP(hipStreamSynchronize(h->st));
  for (FrameRec& Q : h->q) {  // every frame in flight has finished on the device
    if (Q.pending) continue;
    if (Q.seq > h->mirror_seq) {  // the newest records
      std::memcpy(h->hf.data(), h->slot[Q.fpar].hfo.data(), sizeof(StreamFrame) * B);
      h->mirror_seq = Q.seq;
    }
    // frames queued behind this one defer the same streams (k_frame_prep): no frame is queued
    // behind them until they have run again (chain_ok), so the device's deferral flags, which the
    // runs again clear, are never read meanwhile
    for (int s = 0; s < B; ++s) Q.has_deferred |= Q.active[s] && h->slot[Q.fpar].hfo[s].deferred;
  }
  FrameRec R2;
  int32_t rc = enqueue_saved(h, R, redo, R2);
  if (rc == LOAM_OK && R2.seq) rc = mapper_finish_rec(h, R2, true);
  return rc;
}

// a failed frame finished by loam_mapper_solve_async (see loam_mapper::held_rc); a hand-off
// error outranks a capacity one, the first of equal rank is kept
static void hold_status(loam_mapper* h, int32_t rc) {
  if (rc == LOAM_OK) return;
  if (h->held_rc == LOAM_OK || (rc == LOAM_ERR_SYNC && h->held_rc != LOAM_ERR_SYNC)) {
    h->held_rc = rc;
    h->held_msg = loam_last_error();
  }
}
static int32_t take_held(loam_mapper* h) {
  if (h->held_rc == LOAM_OK) return LOAM_OK;
  set_error("an earlier frame, finished by loam_mapper_solve_async, failed (" +
            std::string(h->held_rc == LOAM_ERR_SYNC ? "LOAM_ERR_SYNC" : "LOAM_ERR_CAPACITY") + "): " + h->held_msg);
  h->held_rc = LOAM_OK;
  h->held_msg.clear();
  return LOAM_ERR_EARLIER;
}

// a pending frame at the front of the queue is enqueued (its predecessor has been waited for)
static int32_t launch_front(loam_mapper* h) {
  if (h->q.empty() || !h->q.front().pending) return LOAM_OK;
  FrameRec P = std::move(h->q.front());
  h->q.pop_front();
  std::vector<int> run;
  for (int s = 0; s < h->B; ++s)
    if (P.active[s]) run.push_back(s);
  FrameRec R;
  const int32_t rc = enqueue_saved(h, P, run, R);
  if (rc != LOAM_OK) {  // the pending frame is dropped, not run: say so
    set_error("a queued frame was dropped, not run: " + std::string(loam_last_error()));
    return rc;
  }
  R.behind = P.behind;
  if (R.seq) h->q.push_front(std::move(R));
  return LOAM_OK;
}

static int32_t finish_oldest(loam_mapper* h) {
  TRY(launch_front(h));
  if (h->q.empty()) return LOAM_OK;
  FrameRec R = std::move(h->q.front());
  h->q.pop_front();
  return mapper_finish_rec(h, R, false);
}

// the oldest frame finished to make room: its own failure (a capacity or hand-off error, committed
// as computed) is held for the next loam_mapper_wait / _solve; a HIP / argument / state error returns
static int32_t finish_oldest_held(loam_mapper* h) {
  const int32_t older = finish_oldest(h);
  if (older == LOAM_ERR_HIP || older == LOAM_ERR_ARG || older == LOAM_ERR_STATE) return older;
  hold_status(h, older);
  return LOAM_OK;
}

static int32_t settle_all(loam_mapper* h) {
  int32_t status = LOAM_OK;
  while (!h->q.empty()) {
    const int32_t rc = finish_oldest(h);
    if (rc != LOAM_OK && (status == LOAM_OK || rc == LOAM_ERR_SYNC)) status = rc;
  }
  return status;
}

// can the next frame be queued behind the one in flight?  Not when the host foresees a
// recentering for it: the initial guess from the transform known now, with a 2 m margin for the
// correction of the frame in flight.  (k_frame_prep checks exactly and defers the frame when the
// foresight was wrong.)  Compactions are queued ahead of it instead (enqueue_frame).
static bool chain_capable(const loam_mapper* h) {
  return h->use_graph && !h->prof && !h->D.sharded && h->lm_G > 0;
}

static bool chain_ok(const loam_mapper* h) {
  if (!chain_capable(h)) return false;
  for (const FrameRec& Q : h->q)
    if (Q.has_deferred || Q.pending) return false;
  const int dims[3] = {CW, CH, CD};
  const double R = 2.0;
  for (int s = 0; s < h->B; ++s) {
    const HostStream& H = h->hs[s];
    if (!H.in_ready) continue;
    const StreamFrame& F = h->hf[s];
    double wmap[7], wodom[7], pose[7];
    pack7(H.q_wmap_wodom, H.t_wmap_wodom, wmap);
    pack7(H.in_q, H.in_t, wodom);
    pose_initial_guess(wmap, wodom, pose);
    for (int a = 0; a < 3; ++a)
      for (double d : {-R, R}) {
        const int c = cube_of(pose[4 + a] + d, F.cen[a]);
        if (c < 3 || c >= dims[a] - 3) return false;
      }
  }
  return true;
}

// Frames in the queue, oldest first, at most two: a frame in flight may have one more behind
// it, queued on the device (chained) or, when the host cannot queue it there (chain_ok), kept
// pending with its inputs and stack taken, and enqueued once its predecessor has been waited for.
// loam_mapper_wait always finishes the oldest frame, so frame f + 1 can be given before frame f
// is waited for, whichever way it runs.
static int32_t solve_async_impl(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  // a third frame first finishes the oldest.  A non-OK return means the new frame was NOT
  // enqueued (a HIP / argument / state error here, or one of its own enqueue); the oldest
  // frame's own failure (a capacity or hand-off error, committed as computed) is held for the
  // next loam_mapper_wait / _solve, which return it as LOAM_ERR_EARLIER.
  if (h->q.size() >= 2) TRY(finish_oldest_held(h));
  TRY(launch_front(h));
  // behind a frame in flight: queued on the device (chained) where the host can, else pending:
  // its stack now, beside the frame in flight; the rest once that frame has been waited for
  const bool behind = !h->q.empty(), chained = behind && chain_ok(h);
  TRY(launch_stacks(h));  // inputs not prefetched
  FrameRec R;
  TRY(take_inputs(h, R));
  if (!R.any_active()) return LOAM_OK;
  R.behind = behind;
  if (behind && !chained) {
    R.pending = true;
    R.seq = 1;  // (a real sequence number when it is enqueued)
  } else {
    TRY(enqueue_frame(h, chained, R));
  }
  h->spar ^= 1;  // the next frame's stacks go to the other buffers
  h->q.push_back(std::move(R));
  return LOAM_OK;
}

int32_t loam_mapper_solve_async(loam_mapper* h) {
  const int32_t rc = solve_async_impl(h);
  // a sharded rank whose HIP runtime fails here may never reach the frame's collectives: the
  // others then fail theirs at once (in-process groups) instead of waiting out the transport's
  // timeout.  (Argument, state and capacity errors are the same on every rank: identical inputs.)
  if (rc == LOAM_ERR_HIP && h && h->comm) comm_abort(h->comm);
  return rc;
}

int32_t loam_mapper_wait(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  if (h->q.empty()) return take_held(h);
  LOAM_HIP(hipSetDevice(h->dev));
  TRY(finish_oldest(h));  // (a pending oldest frame is enqueued first)
  // a frame waiting behind the finished one (its stack VoxelGrid already queued) is enqueued now,
  // so the device works on it while the host returns and gives the next input
  TRY(launch_front(h));
  return take_held(h);
}

int32_t loam_mapper_solve(loam_mapper* h) {
  TRY(loam_mapper_solve_async(h));
  SETTLE(h);
  return take_held(h);
}

// the newest frame's poses and stats from its early records (written after the second LM round):
// false when they cannot stand for the frame (a deferred stream, or an error flag already set),
// then the caller finishes the frame whole
static bool take_early(loam_mapper* h, FrameRec& R) {
  const StreamFrame* FE = h->slot[R.fpar].hfo_early.data();
  for (int s = 0; s < h->B; ++s)
    if (R.active[s] && (FE[s].deferred || FE[s].err)) return false;
  for (int s = 0; s < h->B; ++s) {
    const StreamFrame& F = FE[s];
    HostStream& H = h->hs[s];
    H.solved_last = R.active[s] && F.active;
    if (!H.solved_last) continue;
    commit_stream(h, s, R, F);  // (the full finish repeats it on the same values)
    loam_map_stats& S = H.st;
    S.ms_total = 0;
    S.ms_opt = 0;
    S.queued = R.chained ? 1 : 0;
    S.rerun = 0;
  }
  R.early_seen = true;
  return true;
}

int32_t loam_mapper_solve_pose(loam_mapper* h) {
  if (!h) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  if (!h->early) {  // the frames' sequences gain the early records: recapture the graphs
    SETTLE(h);
    for (auto& gp : h->gexec)
      for (auto& g : gp)
        if (g) {
          (void)hipGraphExecDestroy(g);
          g = nullptr;
        }
    h->early = true;
  }
  TRY(loam_mapper_solve_async(h));  // queued behind the previous frame, as the pipelined solves
  while (h->q.size() > 1) TRY(finish_oldest_held(h));  // the previous frame: its insertion and re-VoxelGrid ran meanwhile
  TRY(launch_front(h));  // (a frame kept pending behind it is enqueued now)
  if (h->q.empty()) return take_held(h);
  FrameRec& R = h->q.front();
  bool early = R.graph && !R.pending;
  if (early) TRY(wait_word(h, h->done_early.data() + R.fpar, R.epoch));
  if (!early || !take_early(h, R)) {  // the frame whole: its status now
    const int32_t rc = finish_oldest(h);
    if (rc != LOAM_OK) return rc;
  }
  return take_held(h);
}

int32_t loam_mapper_debug_counters(loam_mapper* h, uint64_t* out, int32_t n, int32_t reset) {
  SETTLE(h);
  if (!h || !out || n < 0 || n > LOAM_DEBUG_COUNTERS) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  LOAM_HIP(hipStreamSynchronize(h->st));
  LOAM_HIP(hipMemcpy(out, h->D.dbg, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
  if (n > MD_OCC_IN_USE) {  // occupancy blocks taken now, over the handle's (stream, map) pools
    std::vector<uint32_t> used((size_t)h->B * 2 * OCC_USED_WORDS);
    LOAM_HIP(hipMemcpy(used.data(), h->D.occ_used, sizeof(uint32_t) * used.size(), hipMemcpyDeviceToHost));
    out[MD_OCC_IN_USE] = 0;
    for (uint32_t w : used) out[MD_OCC_IN_USE] += (uint64_t)__builtin_popcount(w);
  }
  if (reset) LOAM_HIP(hipMemset(h->D.dbg, 0, sizeof(uint64_t) * LOAM_DEBUG_COUNTERS));
  return LOAM_OK;
}

int32_t loam_mapper_set_profiling(loam_mapper* h, int32_t enable) {
  SETTLE(h);
  if (!h) return LOAM_ERR_ARG;
  h->prof = enable != 0;
  h->ev_fam.clear();  // (settled: every timed launch has been read)
  return LOAM_OK;
}

int32_t loam_mapper_kernel_times(loam_mapper* h, loam_kernel_times* out) {
  SETTLE(h);
  if (!h || !out) return LOAM_ERR_ARG;
  for (int f = 0; f < LOAM_KFAM_COUNT; ++f) {
    out->ms[f] = f < NFAM ? h->fam_ms[f] : 0.0;
    out->launches[f] = f < NFAM ? h->fam_launches[f] : 0;
    out->bytes[f] = f < NFAM ? h->fam_bytes[f] : 0.0;
  }
  return LOAM_OK;
}

int32_t loam_mapper_reset_kernel_times(loam_mapper* h) {
  SETTLE(h);
  if (!h) return LOAM_ERR_ARG;
  for (int f = 0; f < NFAM; ++f) {
    h->fam_ms[f] = h->fam_bytes[f] = 0.0;
    h->fam_launches[f] = 0;
  }
  return LOAM_OK;
}

int32_t loam_mapper_pose(loam_mapper* h, int32_t s, double* q_w, double* t_w) {
  SETTLE_RESULTS(h);
  TRY(check_stream(h, s));
  if (!q_w || !t_w) return LOAM_ERR_ARG;
  const HostStream& H = h->hs[s];
  if (H.skip) {
    std::copy(H.q_hf, H.q_hf + 4, q_w);
    std::copy(H.t_hf, H.t_hf + 3, t_w);
  } else {
    unpack7(H.pose, q_w, t_w);
  }
  return LOAM_OK;
}

int32_t loam_mapper_stats(loam_mapper* h, int32_t s, loam_map_stats* st) {
  SETTLE_RESULTS(h);
  TRY(check_stream(h, s));
  if (!st) return LOAM_ERR_ARG;
  *st = h->hs[s].st;
  return LOAM_OK;
}

int32_t loam_mapper_get_state(loam_mapper* h, int32_t s, int32_t* cen, double* q, double* t) {
  SETTLE_RESULTS(h);
  TRY(check_stream(h, s));
  if (!cen || !q || !t) return LOAM_ERR_ARG;
  for (int a = 0; a < 3; ++a) cen[a] = h->hs[s].cen[a];
  for (int i = 0; i < 4; ++i) q[i] = h->hs[s].q_wmap_wodom[i];
  for (int i = 0; i < 3; ++i) t[i] = h->hs[s].t_wmap_wodom[i];
  return LOAM_OK;
}

// cell index of cubes [c0, c1) of (stream, map) after host-side changes
static int32_t build_cube_index(loam_mapper* h, int32_t s, int32_t m, int32_t c0, int32_t c1) {
  LOAM_HIP(hipSetDevice(h->dev));
  // the device copy of the stream record supplies arena_active: refresh it first
  LOAM_HIP(hipMemcpyAsync(h->D.fr + s, &h->hf[s], sizeof(StreamFrame), hipMemcpyHostToDevice, h->st));
  MapperDev D = h->D;
  D.cube_tab = h->cube_tab[h->parity];
  const int3 cen = make_int3(h->hf[s].cen[0], h->hf[s].cen[1], h->hf[s].cen[2]);
  k_cube_index<<<c1 - c0, VX_THREADS, 0, h->st>>>(D, s, m, c0, c1, cen);
  LOAM_HIP(hipGetLastError());
  LOAM_HIP(hipStreamSynchronize(h->st));
  return LOAM_OK;
}

int32_t loam_mapper_set_state(loam_mapper* h, int32_t s, const int32_t* cen, const double* q, const double* t) {
  SETTLE(h);
  TRY(check_stream(h, s));
  if (!cen || !q || !t) return LOAM_ERR_ARG;
  bool moved = false;
  for (int a = 0; a < 3; ++a) {
    moved |= h->hf[s].cen[a] != cen[a];
    h->hf[s].cen[a] = h->hs[s].cen[a] = cen[a];
  }
  for (int i = 0; i < 4; ++i) h->hs[s].q_wmap_wodom[i] = h->hf[s].wmap[i] = q[i];
  for (int i = 0; i < 3; ++i) h->hs[s].t_wmap_wodom[i] = h->hf[s].wmap[4 + i] = t[i];
  if (moved)  // cube world positions changed: rebuild every cube's cell index
    for (int m = 0; m < 2; ++m) TRY(build_cube_index(h, s, m, 0, NCUBE));
  return LOAM_OK;
}

int32_t loam_mapper_cube_count(loam_mapper* h, int32_t s, int32_t which, int32_t cube) {
  SETTLE(h);
  TRY(check_stream(h, s));
  if (which < 0 || which > 1 || cube < 0 || cube >= NCUBE) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  uint2 v;
  LOAM_HIP(hipMemcpy(&v, h->cube_tab[h->parity] + ((size_t)s * 2 + which) * NCUBE + cube, sizeof(uint2), hipMemcpyDeviceToHost));
  return (int32_t)v.y;
}

int32_t loam_mapper_cube_copy(loam_mapper* h, int32_t s, int32_t which, int32_t cube, float* out) {
  SETTLE(h);
  TRY(check_stream(h, s));
  if (which < 0 || which > 1 || cube < 0 || cube >= NCUBE || !out) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  uint2 v;
  LOAM_HIP(hipMemcpy(&v, h->cube_tab[h->parity] + ((size_t)s * 2 + which) * NCUBE + cube, sizeof(uint2), hipMemcpyDeviceToHost));
  const float4* base = h->D.arena + (((size_t)s * 2 + which) * 2 + h->hf[s].arena_active[which]) * (size_t)h->D.map_cap;
  if (v.y) LOAM_HIP(hipMemcpy(out, base + v.x, sizeof(float4) * v.y, hipMemcpyDeviceToHost));
  return (int32_t)v.y;
}

int32_t loam_mapper_stack_copy(loam_mapper* h, int32_t s, int32_t which, float* out, int32_t cap) {
  SETTLE(h);
  TRY(check_stream(h, s));
  if (which < 0 || which > 1 || (cap > 0 && !out)) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  const int32_t n = which == 0 ? h->hf[s].nc_stack : h->hf[s].ns_stack;
  if (n > cap) return n;  // the count only
  if (n) {
    LOAM_HIP(hipMemcpy(out, h->slot[h->last_spar].stack_buf[which] + (size_t)s * h->D.max_in, sizeof(float4) * n,
                       hipMemcpyDeviceToHost));
  }
  return n;
}

int32_t loam_mapper_corr_copy(loam_mapper* h, int32_t s, double* x0, int32_t* type, double* records, float* nbr_xyz,
                              int32_t cap) {
  SETTLE(h);
  TRY(check_stream(h, s));
  if (cap < 0 || (cap > 0 && (!type || !records || !nbr_xyz))) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  const StreamFrame& F = h->hf[s];
  const int32_t n = F.nc_stack + F.ns_stack;
  if (x0) std::copy(F.knn_pose, F.knn_pose + 7, x0);
  if (n > cap || n == 0) return n;  // the count only
  DevBuf<int> dt;
  DevBuf<double> dr;
  DevBuf<float> dn;
  TRY(dt.reserve(n));
  TRY(dr.reserve((size_t)n * 10));
  TRY(dn.reserve((size_t)n * 15));
  k_corr_gather<<<std::min(256, (n + 255) / 256), 256, 0, h->st>>>(h->D, s, F.nc_stack, n, F.optimize, F.arena_active[0],
                                                                  F.arena_active[1], dt, dr, dn);
  LOAM_HIP(hipGetLastError());
  LOAM_HIP(hipMemcpyAsync(type, dt, sizeof(int) * n, hipMemcpyDeviceToHost, h->st));
  LOAM_HIP(hipMemcpyAsync(records, dr, sizeof(double) * n * 10, hipMemcpyDeviceToHost, h->st));
  LOAM_HIP(hipMemcpyAsync(nbr_xyz, dn, sizeof(float) * n * 15, hipMemcpyDeviceToHost, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  return n;
}

int32_t loam_mapper_cube_set(loam_mapper* h, int32_t s, int32_t which, int32_t cube, const float* pts, int32_t n) {
  SETTLE(h);
  TRY(check_stream(h, s));
  if (which < 0 || which > 1 || cube < 0 || cube >= NCUBE || n < 0 || (n > 0 && !pts)) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  std::vector<float> mine;
  if (h->D.sharded) {  // a sharded handle stores the points of the blocks its rank owns
    for (int i = 0; i < n; ++i)
      if (loam_shard_owner(pts + 4 * (size_t)i, h->D.leaf[which], h->D.nrank) == h->D.rank) mine.insert(mine.end(), pts + 4 * (size_t)i, pts + 4 * (size_t)i + 4);
    pts = mine.data();
    n = (int32_t)(mine.size() / 4);
  }
  StreamFrame& F = h->hf[s];
  uint32_t& tail = F.arena_tail[which];
  if (tail + (uint32_t)n > (uint32_t)h->D.map_cap) {
    set_error("loam_mapper_cube_set: arena full");
    return LOAM_ERR_CAPACITY;
  }
  float4* base = h->D.arena + (((size_t)s * 2 + which) * 2 + F.arena_active[which]) * (size_t)h->D.map_cap;
  if (n) LOAM_HIP(hipMemcpy(base + tail, pts, sizeof(float4) * n, hipMemcpyHostToDevice));
  uint2 v = make_uint2(tail, (uint32_t)n);
  tail += n;
  LOAM_HIP(hipMemcpy(h->cube_tab[h->parity] + ((size_t)s * 2 + which) * NCUBE + cube, &v, sizeof(uint2), hipMemcpyHostToDevice));
  const uint32_t zero = 0;  // caller content: not known to be a VoxelGrid fixed point
  LOAM_HIP(hipMemcpy(h->D.stable_tok + ((size_t)s * 2 + which) * NCUBE + cube, &zero, sizeof(zero), hipMemcpyHostToDevice));
  return build_cube_index(h, s, which, cube, cube + 1);
}

int32_t loam_mapper_map_copy(loam_mapper* h, int32_t s, float* out, int64_t cap) {
  SETTLE(h);
  TRY(check_stream(h, s));
  if (cap < 0 || (cap > 0 && !out)) return LOAM_ERR_ARG;
  LOAM_HIP(hipSetDevice(h->dev));
  MapperDev D = h->D;
  D.cube_tab = h->cube_tab[h->parity];
  // the device stream record supplies arena_active (current after every solve / set)
  LOAM_HIP(hipMemcpyAsync(h->D.fr + s, &h->hf[s], sizeof(StreamFrame), hipMemcpyHostToDevice, h->st));
  k_map_scan<<<1, VX_THREADS, 0, h->st>>>(D, s, h->d_map_off);
  uint32_t total = 0;
  LOAM_HIP(hipMemcpyAsync(&total, h->d_map_off + 2 * NCUBE, sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  if ((int64_t)total > cap) return (int32_t)total;  // the count only
  if (total) {
    TRY(h->d_pub.reserve(total));
    k_map_gather<<<512, 256, 0, h->st>>>(D, s, h->d_map_off, h->d_pub);
    LOAM_HIP(hipGetLastError());
    LOAM_HIP(hipMemcpyAsync(out, h->d_pub, sizeof(float4) * total, hipMemcpyDeviceToHost, h->st));
    LOAM_HIP(hipStreamSynchronize(h->st));
  }
  return (int32_t)total;
}

static int32_t register_common(loam_mapper* h, int32_t s, const float* in, int32_t n, float* out, bool device) {
  TRY(check_stream(h, s));
  if (n < 0 || (n > 0 && (!in || !out))) return LOAM_ERR_ARG;
  if (n == 0) return 0;
  LOAM_HIP(hipSetDevice(h->dev));
  MapPose P;
  TRY(loam_mapper_pose(h, s, P.x, P.x + 4));
  const float4* src = reinterpret_cast<const float4*>(in);
  float4* dst = reinterpret_cast<float4*>(out);
  if (!device) {
    TRY(h->d_pub.reserve(n));
    LOAM_HIP(hipMemcpyAsync(h->d_pub, in, sizeof(float4) * n, hipMemcpyHostToDevice, h->st));
    src = dst = h->d_pub;
  }
  k_register<<<std::min(1024, (n + 255) / 256), 256, 0, h->st>>>(src, dst, n, P);
  LOAM_HIP(hipGetLastError());
  if (!device) LOAM_HIP(hipMemcpyAsync(out, h->d_pub, sizeof(float4) * n, hipMemcpyDeviceToHost, h->st));
  LOAM_HIP(hipStreamSynchronize(h->st));
  return n;
}

int32_t loam_mapper_register_cloud(loam_mapper* h, int32_t s, const float* in, int32_t n, float* out) {
  SETTLE(h);
  return register_common(h, s, in, n, out, false);
}

int32_t loam_mapper_register_cloud_device(loam_mapper* h, int32_t s, const float* d_in, int32_t n, float* d_out) {
  SETTLE(h);
  return register_common(h, s, d_in, n, d_out, true);
}

}  // extern "C"
