// mapper_lm.h — the LM rounds (lm.h): k_lm_eval / _step / _round / _group, pose agreement across ranks.
// Part of the mapper.hip translation unit: included there only, in the order the phases run.
#pragma once

namespace loam {

// LM evaluation pass at the state's evaluation point (lm.h)
// reduce: sharded over several ranks, the stream's last workgroup to finish also sums the
// stream's partials in a fixed order into lm_red[s] (then all-reduced over the ranks): plain
// partial stores + agent-scope release + a ticket; the last acquires before it reads
__global__ void __launch_bounds__(LM_THREADS) k_lm_eval(MapperDev D, int round, int reduce) {
  const int s = D.s0 + blockIdx.x / LM_EBLK, blk = blockIdx.x % LM_EBLK;
  const StreamFrame& F = D.fr[s];
  if (!F.active) return;
  const size_t rb = (size_t)s * 2 * D.max_in;
  const LmRecView R{D.r_type + rb, D.r_px + rb, D.r_py + rb, D.r_pz + rb, D.r_a[0] + rb,
                    D.r_a[1] + rb, D.r_a[2] + rb, D.r_b[0] + rb, D.r_b[1] + rb, D.r_b[2] + rb};
  // sharded: this rank's workgroups are blocks rank * LM_EBLK + blk of nrank * LM_EBLK
  lm_eval_block<LM_THREADS>(R, F.nc_stack + F.ns_stack, F.lm[round], D.rank * LM_EBLK + blk, D.nrank * LM_EBLK,
                            D.partials + ((size_t)s * LM_EBLK + blk) * LM_NACC);
  if (!reduce || F.lm[round].status == LM_DONE) return;  // (uniform over the stream's workgroups)
  __shared__ int last;
  __syncthreads();  // this workgroup's partial stored
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const uint32_t t = __hip_atomic_fetch_add(&D.lm_tick[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = t == (uint32_t)LM_EBLK - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(&D.lm_tick[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x < 64) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (every reading wave)
  if (threadIdx.x < LM_NACC) {
    const double* p = D.partials + (size_t)s * LM_EBLK * LM_NACC;
    double v = 0.0;
    for (int c = 0; c < LM_EBLK; ++c) v += p[(size_t)c * LM_NACC + threadIdx.x];
    D.lm_red[(size_t)s * LM_NACC + threadIdx.x] = v;
  }
}

// LM step: one wave per stream; on termination the best point becomes the stream pose
// (Ceres writes it back into the parameter blocks, laser_mapping.cpp:535-536)
__global__ void __launch_bounds__(64) k_lm_step(MapperDev D, int round) {
  const int s = D.s0 + blockIdx.x;
  StreamFrame& F = D.fr[s];
  if (!F.active) return;
  LmState& S = F.lm[round];
  if (D.sharded)  // the all-reduced sums: every rank takes the identical step
    lm_step_wave(D.lm_red + (size_t)s * LM_NACC, 1, S, F.pose);
  else
    lm_step_wave(D.partials + (size_t)s * LM_EBLK * LM_NACC, LM_EBLK, S, F.pose);  // pose = best when done
}

// ---------------------------------------------------------------------------------------
// One launch per outer round: all <= 5 LM passes of every stream.  G workgroups per stream
// evaluate a share of the records each; the stream's leader (g = 0) keeps the trust-region
// state in its LDS, reduces the workers' partials and runs the step.  Hand-offs follow the
// agent-scope release/acquire recipe (cdna_hip_programming.md §6 Guideline 16): partials are
// plain stores + drain + release fence + relaxed ticket; the eval point is published with sc1
// (atomic) stores + drain + a relaxed flag; every consumer polls relaxed and acquires once.
// Shares are claimed per pass by whichever workgroups run (no residency needed), and every spin is
// bounded (MAP_ERR_LM_SYNC, the stream's LM then stops).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LM_THREADS) k_lm_round(MapperDev D, int round, int G) {
  // block b -> stream b % Bp, member b / Bp with B padded to a multiple of 8 (the padding
  // blocks leave at once): all of a stream's blocks share an XCD (b % 8), so its hand-offs
  // stay in one L2 (placement is speed only)
  const int Bp = lm_padded(D.B), sl = blockIdx.x % Bp, g = blockIdx.x / Bp;
  if (sl >= D.B) return;
  const int s = D.s0 + sl;
  StreamFrame& F = D.fr[s];
  if (!F.active) return;
  const size_t rb = (size_t)s * 2 * D.max_in;
  LmJob J;
  J.S = &F.lm[round];
  J.R = LmRecView{D.r_type + rb, D.r_px + rb, D.r_py + rb, D.r_pz + rb, D.r_a[0] + rb, D.r_a[1] + rb,
                  D.r_a[2] + rb, D.r_b[0] + rb, D.r_b[1] + rb, D.r_b[2] + rb};
  J.nrec = F.nc_stack + F.ns_stack;
  J.part = D.partials + (size_t)s * D.max_chunks * LM_NACC;
  J.sync = D.lm_sync + ((size_t)s * 2 + round) * LM_SYNC_WORDS;
  J.xpub = D.lm_xpub + ((size_t)s * 2 + round) * 8;
  J.best_out = F.pose;
  J.err = &F.err;
  J.err_code = MAP_ERR_LM_SYNC;
  J.prof = D.pdbg ? D.pdbg + MD_LM : nullptr;
  if (D.ipc_tab) {  // ranks in other processes: the per-pass sums meet in their mapped buffers
    J.rank = D.rank;
    J.nrank = D.nrank;
    J.ipc = D.ipc_tab;
    J.ipc_slot_off = (((size_t)(F.epoch & 1u) * D.ipc_B + s) * 2 + round) * LM_MAX_PASSES * LM_NACC;
    J.ipc_flag_off = (size_t)s * 2 + round;
    J.flag_base = F.epoch * (uint32_t)LM_MAX_PASSES;
  }
  lm_round_device<LM_THREADS>(J, g, G);
}

// The LM round of every rank of an in-process sharded group in ONE launch (comm_group_launch):
// the ranks' leaders wait for each other's per-pass sums (peer slots, lm.h), which separate
// launches could not do safely (two streams' kernels may share a hardware queue, one behind the
// other).  What k_lm_round reads of each rank's MapperDev:
struct LmRankArgs {
  StreamFrame* fr;
  const int* r_type;
  const float *r_px, *r_py, *r_pz;
  const double* r_a[3];
  const double* r_b[3];
  double* partials;
  uint32_t* lm_sync;
  double* lm_xpub;
  unsigned long long* pdbg;
  int max_in, max_chunks, B, s0;
};
struct LmGroupArgs {
  LmRankArgs r[LOAM_LOCAL_MAX_RANKS];
  double* peer;        // MapperDev::lm_peer (the group's)
  uint32_t* peer_flag;
  int nrank;
};
// blocks: the R x Bp leaders first (rank-major, so every leader is dispatched before any member),
// then each rank's members; a stream's blocks are congruent mod 8 (one XCD) as in k_lm_round
__global__ void __launch_bounds__(LM_THREADS) k_lm_group(LmGroupArgs A, int round, int G) {
  const int R = A.nrank, Bp = lm_padded(A.r[0].B);
  int b = blockIdx.x, rank, sl, g;
  if (b < R * Bp) {
    rank = b / Bp;
    sl = b % Bp;
    g = 0;
  } else {
    b -= R * Bp;
    const int per = Bp * (G - 1);
    rank = b / per;
    sl = (b % per) % Bp;
    g = 1 + (b % per) / Bp;
  }
  const LmRankArgs& a = A.r[rank];
  if (sl >= a.B) return;
  const int s = a.s0 + sl;
  StreamFrame& F = a.fr[s];
  if (!F.active) return;
  const size_t rb = (size_t)s * 2 * a.max_in;
  LmJob J;
  J.S = &F.lm[round];
  J.R = LmRecView{a.r_type + rb, a.r_px + rb, a.r_py + rb, a.r_pz + rb, a.r_a[0] + rb, a.r_a[1] + rb,
                  a.r_a[2] + rb, a.r_b[0] + rb, a.r_b[1] + rb, a.r_b[2] + rb};
  J.nrec = F.nc_stack + F.ns_stack;
  J.part = a.partials + (size_t)s * a.max_chunks * LM_NACC;
  J.sync = a.lm_sync + ((size_t)s * 2 + round) * LM_SYNC_WORDS;
  J.xpub = a.lm_xpub + ((size_t)s * 2 + round) * 8;
  J.best_out = F.pose;
  J.err = &F.err;
  J.err_code = MAP_ERR_LM_SYNC;
  J.prof = a.pdbg ? a.pdbg + MD_LM : nullptr;
  J.rank = rank;
  J.nrank = R;
  const size_t sr = (size_t)s * 2 + round;
  J.peer = A.peer + (((size_t)(F.epoch & 1u) * a.B * 2 + sr) * R) * LM_MAX_PASSES * LM_NACC;
  J.peer_flag = A.peer_flag + sr * R;
  J.flag_base = F.epoch * (uint32_t)LM_MAX_PASSES;
  lm_round_device<LM_THREADS>(J, g, G);
}

struct LmGroupCtx {
  int round, G;
  double* peer;
  uint32_t* peer_flag;
};
static void lm_group_launch(const void* const* blobs, int nrank, hipStream_t st, void* user) {
  const LmGroupCtx& C = *static_cast<const LmGroupCtx*>(user);
  LmGroupArgs A{};
  for (int r = 0; r < nrank; ++r) A.r[r] = *static_cast<const LmRankArgs*>(blobs[r]);
  A.peer = C.peer;
  A.peer_flag = C.peer_flag;
  A.nrank = nrank;
  k_lm_group<<<nrank * lm_padded(A.r[0].B) * C.G, LM_THREADS, 0, st>>>(A, C.round, C.G);
}

// sharded: every rank stores points with the same pose, so after the LM every rank adopts
// rank 0's (they are equal when the all-reduce is bit-identical on every rank, as RCCL's and
// the Python transports are); a rank that differed counts it in debug counter 40
__global__ void k_pose_publish(MapperDev D) {
  const int s = D.s0 + blockIdx.x, i = threadIdx.x;
  if (i < 7) D.pose_x[((size_t)D.rank * D.B + s) * 8 + i] = D.fr[s].pose[i];
}
__global__ void k_pose_adopt(MapperDev D) {
  const int s = D.s0 + blockIdx.x, i = threadIdx.x;
  StreamFrame& F = D.fr[s];
  if (i < 7) {
    const double v = D.pose_x[(size_t)s * 8 + i];  // rank 0's slot
    if (__double_as_longlong(v) != __double_as_longlong(F.pose[i])) atomicAdd(&D.dbg[MD_POSE_DIFF], 1ull);
    F.pose[i] = v;
  }
}

}  // namespace loam
