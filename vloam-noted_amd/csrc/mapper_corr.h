// mapper_corr.h — correspondences: exact 5-NN (k_knn, k_nn_merge) and the factor records (k_geom).
// Part of the mapper.hip translation unit: included there only, in the order the phases run.
#pragma once

namespace loam {

// ---------------------------------------------------------------------------------------
// correspondences of one outer round (laser_mapping.cpp:545-699) -> factor records
// ---------------------------------------------------------------------------------------
// pass 1: exact 5-NN of every query (laser_mapping.cpp:554, :633; accepted only if the 5th is
// within 1 m: :557, :642) over the window cubes' cell indexes (cubeindex.h).  Distances are
// FLANN's L2_Simple<float>; ties go to the lower submap index (sub_off[slot] + position in
// the cube).  Output: positions of the 5 neighbours in the cell-sorted arena, -1: none.
struct Near5 {
  float d[5];
  int id[5];   // submap index (tie-break)
  int pos[5];  // cell-sorted arena position
};
__device__ inline void near5_offer(Near5& T, float d, int id, int pos) {
  if (!(d < T.d[4] || (d == T.d[4] && id < T.id[4]))) return;
  T.d[4] = d; T.id[4] = id; T.pos[4] = pos;
#pragma unroll
  for (int k = 4; k > 0; --k) {
    if (T.d[k] < T.d[k - 1] || (T.d[k] == T.d[k - 1] && T.id[k] < T.id[k - 1])) {
      float td = T.d[k]; T.d[k] = T.d[k - 1]; T.d[k - 1] = td;
      int ti = T.id[k]; T.id[k] = T.id[k - 1]; T.id[k - 1] = ti;
      int tp = T.pos[k]; T.pos[k] = T.pos[k - 1]; T.pos[k - 1] = tp;
    }
  }
}
__device__ inline int floor_div50(int v) { return v >= 0 ? v / 50 : -((-v + 49) / 50); }

struct WinMap {  // per (stream, map) window cubes, in LDS
  uint32_t off[WIN_MAX], n[WIN_MAX], tsize[WIN_MAX];
  int sub[WIN_MAX];
};

// L lanes per query (L | 64): the lanes of a group visit the same cells and split each cell's
// points; the pruning bound is the group minimum of the lanes' 5th distances (each bounds the
// union's 5th from above, so it is safe), and a butterfly merge leaves the union's 5 nearest in
// every lane.  The result is the L = 1 result (the minimum over (d, key) of the same
// candidates); L > 1 shortens each query's chain of dependent loads.
// block -> (stream, member): stream b % B, member b / B (a stream's blocks on one XCD, b % 8,
// when B is a multiple of 8: they share that XCD's L2 copy of the stream's cell indexes)
__device__ inline void corr_block(const MapperDev& D, int* s, int* blk) {
  *s = D.s0 + blockIdx.x % D.B;
  *blk = blockIdx.x / D.B;
}

#ifndef KNN_WAVES
#define KNN_WAVES 7  // 72 VGPRs, 20 B spill outside the cell loop: 6 -> 7 waves, correspondence -8%
#endif
// CS (cell split): the L lanes of a query take different cells, lane g the cells g, g + L, ...
// of the nearest-first order, each scanning all of its cell's points, with the group minimum of
// their 5th distances as the shared pruning bound: a query's chain of dependent probes is 27 / L
// steps long instead of 27 (few streams leave the chip mostly idle: latency, not issue, bounds
// the search).  Without CS the lanes share each cell and split its points.
template <int L, bool CS = false>
__global__ void __launch_bounds__(CORR_THREADS) __attribute__((amdgpu_waves_per_eu(CS ? 4 : KNN_WAVES, 8))) k_knn(MapperDev D, int round) {
  __shared__ WinMap W[2];
  __shared__ int slot_of[75];  // 5 x 5 x 3 window position -> slot (laserCloudValidInd order)
  // window position -> the cube's occupancy block id + 1, OCC_NONE: it has none, OCC_ABSENT: no such
  // cube in the submap, or nothing in it
  __shared__ uint32_t wocc[2][75];
  int s, blk;
  corr_block(D, &s, &blk);
  StreamFrame& F = D.fr[s];
  if (!F.active) return;
  double X[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) X[i] = F.pose[i];
  if (blk == 0 && threadIdx.x < LM_SYNC_WORDS) D.lm_sync[((size_t)s * 2 + round) * LM_SYNC_WORDS + threadIdx.x] = 0;
  if (blk == 0 && threadIdx.x == 0) {
    lm_init(F.lm[round], X, 4, F.optimize != 0);
#pragma unroll
    for (int i = 0; i < 7; ++i) F.knn_pose[i] = X[i];
  }
  if (!F.optimize) return;  // k_geom types every record 0
  const int tid = threadIdx.x;
  const int c0 = F.center[0] - 2, c1 = F.center[1] - 2, c2 = F.center[2] - 1;
  if (tid < 75) slot_of[tid] = -1;
  if (L == 1 && !CS && tid < 75) wocc[0][tid] = wocc[1][tid] = OCC_ABSENT;  // (the cell-split kernel does not read it)
  __syncthreads();
  if (tid < F.valid_num) {
    const int cube = F.window[tid];
    const int ci = cube % CW, cj = (cube / CW) % CH, ck = cube / (CW * CH);
    slot_of[(ci - c0) * 15 + (cj - c1) * 3 + (ck - c2)] = tid;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const uint2 cv = D.cube_tab[sm_index(s, m) * NCUBE + cube];
      if (L == 1 && !CS && cv.y) wocc[m][(ci - c0) * 15 + (cj - c1) * 3 + (ck - c2)] = D.cube_occ[sm_index(s, m) * NCUBE + cube];
      W[m].off[tid] = cv.x;
      W[m].n[tid] = cv.y;
      W[m].tsize[tid] = cv.y ? ci_table_size(cv.y) : 0u;
      W[m].sub[tid] = F.sub_off[m][tid];
    }
  }
  __syncthreads();
  const int nc = F.nc_stack, ns = F.ns_stack;
  const size_t rb = (size_t)s * 2 * D.max_in;
  uint32_t ncand = 0;
  const int gsub = tid % L;
  const int nblk = CS ? D.knn_blk : CORR_BLK;
  for (int ridx = blk * (CORR_THREADS / L) + tid / L; ridx < nc + ns; ridx += nblk * (CORR_THREADS / L)) {
    const int m = ridx < nc ? 0 : 1;  // corners [0, nc), surfs [nc, nc + ns)
    const int qi = m == 0 ? ridx : ridx - nc;
    const float4 q = to_map(X, D.stack[m][(size_t)s * D.max_in + qi]);
    const float4* cp = carena_base(D, s, m, F.arena_active[m]);
    const uint2* ct = ctab_base(D, s, m, F.arena_active[m]);
    const WinMap& WM = W[m];
    Near5 T;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      T.d[k] = INFINITY;
      T.id[k] = 0x7FFFFFFF;
      T.pos[k] = -1;
    }
    const float fx = floorf(q.x), fy = floorf(q.y), fz = floorf(q.z);
    const int qx = (int)fx, qy = (int)fy, qz = (int)fz;
    const float lx = q.x - fx, hx = (fx + 1.0f) - q.x;
    const float ly = q.y - fy, hy = (fy + 1.0f) - q.y;
    const float lz = q.z - fz, hz = (fz + 1.0f) - q.z;
    // points of cell (x, y, z) filed in cube (bi, bj, bk) at local (ax, ay, az)
    auto scan = [&](int bi, int bj, int bk, int ax, int ay, int az) {
      const int wx = bi - c0, wy = bj - c1, wz = bk - c2;
      if (wx < 0 || wx > 4 || wy < 0 || wy > 4 || wz < 0 || wz > 2) return;  // not in the submap
      const int sl = slot_of[wx * 15 + wy * 3 + wz];
      if (sl < 0) return;
      const uint32_t n = WM.n[sl];
      if (n == 0) return;
      const uint32_t off = WM.off[sl];
      const uint2 e = ci_find(ct + 4 * (size_t)off, WM.tsize[sl],
                              (uint32_t)ax | ((uint32_t)ay << 6) | ((uint32_t)az << 12));
      ncand += e.y;
      const int sub = WM.sub[sl];
      for (uint32_t k = CS ? 0 : gsub; k < e.y; k += CS ? 1 : L) {
        const uint32_t pos = off + e.x + k;
        const float4 p = cp[pos];
        // sharded: submap position x ranks + rank keeps the key unique (and equal to the
        // unsharded key at one rank)
        const int key = (sub + __float_as_int(p.w)) * D.nrank + D.rank;
        near5_offer(T, fdist2(q.x, q.y, q.z, p.x, p.y, p.z), key, (int)pos);
      }
    };
    // cell (qx + dx, qy + dy, qz + dz): its cube and local coordinates, and the cubes below at an edge
    auto visit = [&](int dx, int dy, int dz) {
      const int x = qx + dx, y = qy + dy, z = qz + dz;
      const int bi = floor_div50(x + 25) + F.cen[0], bj = floor_div50(y + 25) + F.cen[1],
                bk = floor_div50(z + 25) + F.cen[2];
      int cx[3] = {bi, bj, bk};
      int lc[3];
      const int cv[3] = {x, y, z};
#pragma unroll
      for (int a = 0; a < 3; ++a) lc[a] = cv[a] - ci_corner(cx[a], F.cen[a]);
      scan(bi, bj, bk, lc[0], lc[1], lc[2]);
      // the reference files points at an exact negative multiple of 50 (v + 25) in the cube
      // below (laser_mapping.cpp:747-756): local coordinate 50 there
      int edge = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
        if (cv[a] + 25 < 0 && (cv[a] + 25) % 50 == 0) edge |= 1 << a;
      for (int e = edge; e; e = (e - 1) & edge) {
        int b2[3], l2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          b2[a] = (e >> a) & 1 ? cx[a] - 1 : cx[a];
          l2[a] = (e >> a) & 1 ? 50 : lc[a];
        }
        scan(b2[0], b2[1], b2[2], l2[0], l2[1], l2[2]);
      }
    };
    if constexpr (L == 1 && !CS) {
      // One lane per query: the lane's own occupied cells only.  Bit o of `cells` (nearest-first order,
      // cell_order_code) is clear where the cell is known to be empty: its cube is not in the submap,
      // holds nothing, or the cube's occupancy block (cubeindex.h) has the cell's bit clear.  A cell
      // the block does not decide keeps its bit and is probed as before: a cube without a block, a
      // cell in another cube along x than the query's, a coordinate with the edge rule below.  Empty
      // cells offer nothing and count nothing, so the result and `cand` are those of all 27 cells.
      uint32_t cells = 0x7FFFFFFu;
      if (D.occ_blocks) {
        const uint64_t* pool = D.occ_pool + sm_index(s, m) * D.occ_blocks * (size_t)CI_OCC_WORDS;
        const uint32_t* wo = wocc[m];
        const int qv[3] = {qx, qy, qz};
        int wb[3][3], lo[3][3];  // [axis][offset + 1]: window coordinate of the cube, local coordinate
        uint32_t open[3] = {0u, 0u, 0u};  // per axis, bit offset + 1: the block does not decide
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const int v = qv[a] + d - 1;
            const int bc = floor_div50(v + 25) + F.cen[a];
            wb[a][d] = bc - (a == 0 ? c0 : (a == 1 ? c1 : c2));
            lo[a][d] = v - ci_corner(bc, F.cen[a]);
            if (v + 25 < 0 && (v + 25) % 50 == 0) open[a] |= 1u << d;
          }
        }
        if (wb[0][0] != wb[0][1]) open[0] |= 1u;
        if (wb[0][2] != wb[0][1]) open[0] |= 4u;
        // the nine (y, z) rows of the query's x cube, every load issued before the first is used
        uint64_t row[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
          const int dy = r % 3, dz = r / 3;
          const int wx = wb[0][1], wy = wb[1][dy], wz = wb[2][dz];
          const bool in = wx >= 0 && wx <= 4 && wy >= 0 && wy <= 4 && wz >= 0 && wz <= 2;
          const uint32_t id = in ? wo[wx * 15 + wy * 3 + wz] : OCC_ABSENT;
          const bool has = id != OCC_ABSENT && id != OCC_NONE;
          const uint64_t w = pool[has ? (size_t)(id - 1) * CI_OCC_WORDS + (size_t)(lo[2][dz] * CI_OCC_DIM + lo[1][dy]) : 0];
          row[r] = has ? w : (id == OCC_ABSENT ? 0ull : ~0ull);
          if ((open[1] >> dy | open[2] >> dz) & 1u) row[r] = ~0ull;
        }
        // (lo[0][1] - 1 is -1 only where open[0] has bit 0, lo[0][1] + 1 is 50 only where it has bit 2)
        const int sh = lo[0][1] > 0 ? lo[0][1] - 1 : 0;
        const int up = lo[0][1] > 0 ? 0 : 1;
        cells = 0u;
#pragma unroll
        for (int o = 0; o < 27; ++o) {
          const uint32_t code = cell_order_code(o);
          const int dx = (int)(code & 3u), dy = (int)((code >> 2) & 3u), dz = (int)(code >> 4);
          const uint32_t t3 = ((uint32_t)(row[dz * 3 + dy] >> sh) << up) | open[0];
          cells |= ((t3 >> dx) & 1u) << o;
        }
      }
      // Two loops, not one `while (cells)`: the inner one is arithmetic only and skips the cells the bound
      // prunes, so that every lane that still has an admitted cell arrives at `visit` (the memory chain) in
      // the same trip of the outer loop; with the gap test and a `continue` in one loop, a lane whose cell is
      // pruned would idle through the other lanes' probe.
      while (true) {
        // the lane's next occupied cell the bound admits (the same test, in the same order, as below)
        const float bound = fminf(T.d[4], 1.0f) * 1.01f + 1e-6f;  // rounding margin
        int dx = 0, dy = 0, dz = 0;
        bool found = false;
        while (cells && !found) {
          const int o = __builtin_ctz(cells);
          cells &= cells - 1u;
          const uint32_t code = cell_order_code(o);
          dx = (int)(code & 3u) - 1, dy = (int)((code >> 2) & 3u) - 1, dz = (int)(code >> 4) - 1;
          const float gx = dx < 0 ? lx : (dx > 0 ? hx : 0.f);
          const float gy = dy < 0 ? ly : (dy > 0 ? hy : 0.f);
          const float gz = dz < 0 ? lz : (dz > 0 ? hz : 0.f);
          found = !(gx * gx + gy * gy + gz * gz > bound);
        }
        if (!found) break;
        visit(dx, dy, dz);
      }
    } else {
      // (the cell's visit is written out here, not a call of `visit`: through the lambda this instantiation
      // took 97 VGPRs instead of 95, a wave per SIMD less)
      for (int ob = 0; ob < 27; ob += CS ? L : 1) {
        const int o = CS ? ob + gsub : ob;
        const uint32_t code = cell_order_code(o < 27 ? o : 0);
        const int dx = (int)(code & 3u) - 1, dy = (int)((code >> 2) & 3u) - 1, dz = (int)(code >> 4) - 1;
        const float gx = dx < 0 ? lx : (dx > 0 ? hx : 0.f);
        const float gy = dy < 0 ? ly : (dy > 0 ? hy : 0.f);
        const float gz = dz < 0 ? lz : (dz > 0 ? hz : 0.f);
        float bound = fminf(T.d[4], 1.0f) * 1.01f + 1e-6f;  // rounding margin
#pragma unroll
        for (int o2 = 1; o2 < L; o2 <<= 1) bound = fminf(bound, __shfl_xor(bound, o2, 64));
        if (o >= 27 || gx * gx + gy * gy + gz * gz > bound) continue;
        const int x = qx + dx, y = qy + dy, z = qz + dz;
        const int bi = floor_div50(x + 25) + F.cen[0], bj = floor_div50(y + 25) + F.cen[1],
                  bk = floor_div50(z + 25) + F.cen[2];
        int cx[3] = {bi, bj, bk};
        int lc[3];
        const int cv[3] = {x, y, z};
  #pragma unroll
        for (int a = 0; a < 3; ++a) lc[a] = cv[a] - ci_corner(cx[a], F.cen[a]);
        scan(bi, bj, bk, lc[0], lc[1], lc[2]);
        // the reference files points at an exact negative multiple of 50 (v + 25) in the cube
        // below (laser_mapping.cpp:747-756): local coordinate 50 there
        int edge = 0;
  #pragma unroll
        for (int a = 0; a < 3; ++a)
          if (cv[a] + 25 < 0 && (cv[a] + 25) % 50 == 0) edge |= 1 << a;
        for (int e = edge; e; e = (e - 1) & edge) {
          int b2[3], l2[3];
  #pragma unroll
          for (int a = 0; a < 3; ++a) {
            b2[a] = (e >> a) & 1 ? cx[a] - 1 : cx[a];
            l2[a] = (e >> a) & 1 ? 50 : lc[a];
          }
          scan(b2[0], b2[1], b2[2], l2[0], l2[1], l2[2]);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < L; o <<= 1) {  // butterfly: disjoint candidate sets at every step
      float pd[5];
      int pid[5], ppos[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        pd[k] = __shfl_xor(T.d[k], o, 64);
        pid[k] = __shfl_xor(T.id[k], o, 64);
        ppos[k] = __shfl_xor(T.pos[k], o, 64);
      }
#pragma unroll
      for (int k = 0; k < 5; ++k)
        if (ppos[k] >= 0) near5_offer(T, pd[k], pid[k], ppos[k]);
    }
    if (gsub != 0) continue;
    if (D.sharded) {  // this rank's candidates; the 1 m test follows the merge (k_nn_merge)
      NnRec& o = D.nn_send[D.q_off[s] + ridx];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        o.d[k] = T.d[k];
        o.id[k] = T.id[k];
        const float4 p = T.pos[k] >= 0 ? cp[T.pos[k]] : make_float4(0.f, 0.f, 0.f, 0.f);
        o.x[k] = p.x;
        o.y[k] = p.y;
        o.z[k] = p.z;
      }
      continue;
    }
    const bool ok = T.d[4] < 1.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) D.knn_id[k * D.knn_stride + rb + ridx] = ok ? T.pos[k] : -1;
  }
  unsigned long long wc = ncand;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wc += __shfl_xor(wc, o, 64);
  if ((threadIdx.x & 63) == 0 && wc) atomicAdd(&F.cand[round], wc);
}

// sharded: merge every rank's 5 candidates into the exact 5-NN of the whole submap (each
// rank's list is exact over its own points, so the union's 5 smallest (d, key) are the
// unsharded result), then the 1 m acceptance (:557, :642).  Neighbours go to nn_xyz.
__global__ void __launch_bounds__(CORR_THREADS) k_nn_merge(MapperDev D) {
  const int s = D.s0 + blockIdx.x % D.B, blk = blockIdx.x / D.B;
  const StreamFrame& F = D.fr[s];
  if (!F.active || !F.optimize) return;
  const int nq = F.nc_stack + F.ns_stack;
  const size_t rb = (size_t)s * 2 * D.max_in;
  const size_t qtot = (size_t)D.q_off[D.s0 + D.B];  // records per rank
  for (int ridx = blk * CORR_THREADS + threadIdx.x; ridx < nq; ridx += CORR_BLK * CORR_THREADS) {
    Near5 T;
    float px[5], py[5], pz[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      T.d[k] = INFINITY;
      T.id[k] = 0x7FFFFFFF;
      T.pos[k] = -1;
      px[k] = py[k] = pz[k] = 0.f;
    }
    for (int r = 0; r < D.nrank; ++r) {
      const NnRec& c = D.nn_recv[(size_t)r * qtot + D.q_off[s] + ridx];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float d = c.d[k];
        const int id = c.id[k];
        if (!(d < T.d[4] || (d == T.d[4] && id < T.id[4]))) break;  // c is sorted
        // insert at the tail, bubble up; pos carries the candidate's slot in (px, py, pz)
        int j = 4;
        while (j > 0 && (d < T.d[j - 1] || (d == T.d[j - 1] && id < T.id[j - 1]))) {
          T.d[j] = T.d[j - 1];
          T.id[j] = T.id[j - 1];
          px[j] = px[j - 1];
          py[j] = py[j - 1];
          pz[j] = pz[j - 1];
          --j;
        }
        T.d[j] = d;
        T.id[j] = id;
        px[j] = c.x[k];
        py[j] = c.y[k];
        pz[j] = c.z[k];
      }
    }
    const bool ok = T.d[4] < 1.0f;
    D.knn_id[rb + ridx] = ok ? 0 : -1;
    if (ok) {
#pragma unroll
      for (int k = 0; k < 5; ++k) D.nn_xyz[k * D.knn_stride + rb + ridx] = make_float4(px[k], py[k], pz[k], 0.f);
    }
  }
}

// pass 2: line PCA / plane fit of the 5 neighbours -> factor records (laser_mapping.cpp:557-603,
// :642-680)
__global__ void __launch_bounds__(CORR_THREADS) k_geom(MapperDev D, int round) {
  int s, blk;
  corr_block(D, &s, &blk);
  StreamFrame& F = D.fr[s];
  if (!F.active) return;
  const int nc = F.nc_stack, ns = F.ns_stack;
  const size_t rb = (size_t)s * 2 * D.max_in;
  uint32_t n_edge = 0, n_plane = 0;  // reduced once per wave after the loop
  for (int ridx = blk * CORR_THREADS + threadIdx.x; ridx < nc + ns; ridx += CORR_BLK * CORR_THREADS) {
    if (!F.optimize) {
      D.r_type[rb + ridx] = 0;
      continue;
    }
    const int m = ridx < nc ? 0 : 1;
    const int qi = m == 0 ? ridx : ridx - nc;
    const float4 po = D.stack[m][(size_t)s * D.max_in + qi];
    int type = 0;
    double a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    if (D.knn_id[rb + ridx] >= 0) {
      const float4* lin = carena_base(D, s, m, F.arena_active[m]);
      float nb[5][3];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const float4 p = D.sharded ? D.nn_xyz[j * D.knn_stride + rb + ridx] : lin[D.knn_id[j * D.knn_stride + rb + ridx]];
        nb[j][0] = p.x;
        nb[j][1] = p.y;
        nb[j][2] = p.z;
      }
      if (m == 0) {
        d3 pa, pb;
        if (edge_from_nbrs(nb, pa, pb)) {
          type = 1;
          d3 de{pa.x - pb.x, pa.y - pb.y, pa.z - pb.z};
          double dn = sqrt(de.x * de.x + de.y * de.y + de.z * de.z);
          a[0] = pa.x; a[1] = pa.y; a[2] = pa.z;
          b[0] = de.x / dn; b[1] = de.y / dn; b[2] = de.z / dn;
          ++n_edge;
        }
      } else {
        d3 n;
        double d;
        if (plane_from_nbrs(nb, n, d)) {
          type = 3;
          a[0] = n.x; a[1] = n.y; a[2] = n.z;
          b[0] = d;
          ++n_plane;
        }
      }
    }
    D.r_type[rb + ridx] = type;
    D.r_px[rb + ridx] = po.x;
    D.r_py[rb + ridx] = po.y;
    D.r_pz[rb + ridx] = po.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      D.r_a[k][rb + ridx] = a[k];
      D.r_b[k][rb + ridx] = b[k];
    }
  }
  uint32_t we = n_edge, wp = n_plane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    we += __shfl_xor(we, o, 64);
    wp += __shfl_xor(wp, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (we) atomicAdd(&F.corner_num[round], (int)we);
    if (wp) atomicAdd(&F.surf_num[round], (int)wp);
  }
}

// loam_mapper_corr_copy: what the last round left for the nq = nc + ns queries of stream s, in stack
// order: type[nq], rec[nq][10] = (type, po, a, b) as loam_lm_solve takes them, nbr[nq][5][3] the
// accepted neighbours in kNN order (NaN where the 1 m test rejected them).  The neighbours are read
// as k_geom reads them: through knn_id in the cell-sorted arena `active`, sharded from nn_xyz.  A
// frame that was not optimised has no records: type 0, neighbours NaN.
__global__ void k_corr_gather(MapperDev D, int s, int nc, int nq, int optimize, int active0, int active1, int* type,
                              double* rec, float* nbr) {
  const size_t rb = (size_t)s * 2 * D.max_in;
  for (int ridx = blockIdx.x * blockDim.x + threadIdx.x; ridx < nq; ridx += gridDim.x * blockDim.x) {
    const int m = ridx < nc ? 0 : 1;
    double* r = rec + (size_t)ridx * 10;
    float* o = nbr + (size_t)ridx * 15;
    const int t = optimize ? D.r_type[rb + ridx] : 0;
    type[ridx] = t;
    r[0] = (double)t;
    r[1] = optimize ? (double)D.r_px[rb + ridx] : 0.0;
    r[2] = optimize ? (double)D.r_py[rb + ridx] : 0.0;
    r[3] = optimize ? (double)D.r_pz[rb + ridx] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[4 + k] = optimize ? D.r_a[k][rb + ridx] : 0.0;
      r[7 + k] = optimize ? D.r_b[k][rb + ridx] : 0.0;
    }
    const bool has = optimize && D.knn_id[rb + ridx] >= 0;
    const float4* lin = carena_base(D, s, m, m == 0 ? active0 : active1);
    for (int j = 0; j < 5; ++j) {
      float4 p = make_float4(NAN, NAN, NAN, 0.f);
      if (has) p = D.sharded ? D.nn_xyz[j * D.knn_stride + rb + ridx] : lin[D.knn_id[j * D.knn_stride + rb + ridx]];
      o[3 * j] = p.x;
      o[3 * j + 1] = p.y;
      o[3 * j + 2] = p.z;
    }
  }
}

}  // namespace loam
