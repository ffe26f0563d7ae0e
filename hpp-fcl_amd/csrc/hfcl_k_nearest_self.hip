// hfcl_k_nearest_self.hip -- the clearance of a scene per configuration on device-made pairs (hfcl_scene_nearest_self*): the sweeps that
// make the seeds and the two passes' lists of pairs, and the kernel that combines the two passes.  The narrow phase itself runs through the
// path of the lists of pairs (hfcl_k_cull.hip), the row scans are those of hfcl_k_pairs.hip.  hfcl_nearest_self.hpp has the arithmetic.
// Built without contraction (FLAGS_k_nearest_self): the bounds are the bits of nearest_bound.
//   k_nself_sweep<MODE, GROUPS>   the geometry of k_pairs_sweep: a workgroup owns PAIRS_ROWS rows of one configuration, a wave
//                         PAIRS_WAVE_ROWS of them -- box and the box's terms of the bound in registers --, and walks the column tiles j > i
//                         in ascending order.  A thread brings in one column of the tile as three 16-byte loads, computes the box's terms
//                         once and stores 8 doubles component by component (8 x PAIRS_TILE doubles of LDS: a lane's read of column j is
//                         8 bytes beside its neighbour's, no bank conflict).  With groups the workgroup-uniform skips of k_pairs_sweep_groups.
//                         MODE seed: a row's smallest L and its lowest j, one 16-byte partial per row of the whole table.
//                         MODE count / emit: the predicate of pass 1 / pass 2 (seed[c], thr[c]: uniform loads), counts and positions by
//                         ballots as k_pairs_sweep.
//   k_nself_small<MODE, GROUPS>   scenes of at most 64 objects: a wave per configuration, lane = column, row boxes by __shfl; MODE seed
//                         writes seed[c] itself.
//   k_nself_seed_combine  a wave per configuration folds its rows' partials: butterfly, on a tie the lowest (i, j)
//   k_nself_combine<R>    a lane per configuration: the smaller of the two passes' minima (tie: the lower pair), the counts, the min record
// No atomics, no scratch, no kernel waits for another workgroup; the lists are the same bytes however the call is cut into chunks.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_nearest_self.hpp"

constexpr int NSELF_SEED = 0, NSELF_COUNT = 1, NSELF_EMIT = 2;

static __device__ __forceinline__ uint64_t nself_uniform64(uint64_t m) {  // (a value the wave shares, into scalar registers)
  const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m)))), hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m >> 32))));
  return (uint64_t(hi) << 32) | lo;
}
// butterfly over the 64 lanes: the smallest L, on a tie the lowest key
static __device__ __forceinline__ void nself_seed_wave_reduce(NselfSeed& s) {
  for (int off = 32; off > 0; off >>= 1) {
    const double L = __shfl_xor(s.L, off, 64);
    const uint32_t lo = __shfl_xor(uint32_t(s.key), off, 64), hi = __shfl_xor(uint32_t(s.key >> 32), off, 64);
    nself_seed_merge(s, L, (uint64_t(hi) << 32) | lo);
  }
}

template <int MODE, bool GROUPS>
__global__ void __launch_bounds__(256) k_nself_sweep(NselfArgs na) {
  const PairsArgs& a = na.p;
  __shared__ double tile[8][PAIRS_TILE];                     // box, diagonal, largest |coordinate| (negative: not finite)
  __shared__ uint8_t tile_group[GROUPS ? PAIRS_TILE : 1u];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t n = a.n_objects;
  PairsGeometry geo;
  geo.n_objects = n;
  geo.rows_per_block = a.rows_per_block;
  geo.blocks_per_conf = a.blocks_per_conf;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(geo, a.g0 + blockIdx.x, c, i0, i1);
  const double* __restrict__ boxes = a.boxes + 6u * ((c - a.c_box0) * n);
  const uint64_t chunk_row = c * n + i0 - a.row0;  // the block's first row in the chunk's row arrays
  NselfRowSeed* __restrict__ row_seeds = static_cast<NselfRowSeed*>(na.row_seeds) + c * n;  // the configuration's rows in the table's

  // GROUPS: the block's mask from ALL its rows, the same in the four waves (what is skipped in front of the barriers is skipped by all)
  uint64_t block_mask = 0;
  if (GROUPS) {
    block_mask = pairs_block_mask(a.group, a.collides, i0, i1);
    if (block_mask == 0u) {  // no candidate in these rows
      if (threadIdx.x < i1 - i0) {
        if (MODE == NSELF_SEED) {
          NselfRowSeed none;
          none.L = __builtin_inf();
          none.j = SCENE_NONE;
          none.pad = 0u;
          row_seeds[i0 + threadIdx.x] = none;
        } else if (MODE == NSELF_COUNT) {
          a.row_counts[chunk_row + threadIdx.x] = 0u;
        }
      }
      return;
    }
  }
  // the configuration's seed and threshold: the same for the whole workgroup
  const uint64_t seed = MODE == NSELF_SEED ? NSELF_NO_PAIR : na.seed[c];
  const double thr = (MODE != NSELF_SEED && na.pass == 2) ? na.thr[c] : 0.0;

  // the wave's rows: i0 + wave * PAIRS_WAVE_ROWS + r (past i1: no row -- row index n, no column is above it)
  double row_box[PAIRS_WAVE_ROWS][6], row_diag[PAIRS_WAVE_ROWS], row_big[PAIRS_WAVE_ROWS];
  uint32_t row_i[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
  uint64_t pos[PAIRS_WAVE_ROWS];
  uint64_t row_mask[GROUPS ? PAIRS_WAVE_ROWS : 1u];
  NselfSeed best[MODE == NSELF_SEED ? PAIRS_WAVE_ROWS : 1u];  // (key: the column alone)
  for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
    const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
    const bool there = i < i1;
    row_i[r] = there ? i : n;
    count[r] = 0u;
    if (GROUPS) row_mask[r] = nself_uniform64(there ? a.collides[a.group[i] & 63u] : 0u);
    for (int k = 0; k < 6; ++k) row_box[r][k] = boxes[6u * size_t(there ? i : i0) + k];
    const NearestBoxTerms t = nearest_box_terms(row_box[r]);
    row_diag[r] = t.diagonal;
    row_big[r] = nself_pack_largest(t);
    pos[r] = MODE == NSELF_EMIT && there ? a.row_offsets[chunk_row + wave * PAIRS_WAVE_ROWS + r] : 0u;
    if (MODE == NSELF_SEED) nself_seed_init(best[r]);
  }

  const double2* __restrict__ vec = reinterpret_cast<const double2*>(boxes);  // (a box: 48 B, three vectors; the table is 16-byte aligned)
  for (uint32_t base = pairs_first_tile(i0); base < n; base += PAIRS_TILE) {
    if (GROUPS && pairs_tile_skipped(a.tile_groups[base / PAIRS_TILE], block_mask)) continue;  // (workgroup-uniform: no loads, no barrier)
    __syncthreads();  // (the tile before has been read)
    for (uint32_t col = threadIdx.x; col < PAIRS_TILE; col += 256u) {
      if (base + col < n) {
        const double2 x = vec[3u * size_t(base + col)], y = vec[3u * size_t(base + col) + 1u], z = vec[3u * size_t(base + col) + 2u];
        const double box[6] = {x.x, x.y, y.x, y.y, z.x, z.y};
        const NearestBoxTerms t = nearest_box_terms(box);  // (once per box and tile, not once per test)
        for (int k = 0; k < 6; ++k) tile[k][col] = box[k];
        tile[6][col] = t.diagonal;
        tile[7][col] = nself_pack_largest(t);
        if (GROUPS) tile_group[col] = a.group[base + col];
      }
    }
    __syncthreads();
    for (uint32_t step = 0; step < PAIRS_TILE; step += 64u) {
      const uint32_t j = base + step + lane;
      double col_box[6];
      for (int k = 0; k < 6; ++k) col_box[k] = tile[k][step + lane];  // (columns past n: stale values, refused by j < n)
      const NearestBoxTerms col_terms = nself_unpack(tile[6][step + lane], tile[7][step + lane]);
      const uint32_t col_group = GROUPS ? tile_group[step + lane] : 0u;
      for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
        const bool candidate = j > row_i[r] && j < n && (!GROUPS || pairs_allowed(row_mask[r], col_group));
        const double L = nearest_bound_terms(row_box[r], nself_unpack(row_diag[r], row_big[r]), col_box, col_terms, na.r);
        if (MODE == NSELF_SEED) {
          if (candidate && L < best[r].L) {  // (a lane's columns ascend: the first of equal values is the lowest)
            best[r].L = L;
            best[r].key = j;
          }
        } else {
          const bool keep = candidate && nself_in_pass(na.pass, L, nself_key(row_i[r], j), seed, na.upper, thr);
          const uint64_t ballot = __ballot(keep);
          if (MODE == NSELF_EMIT && ballot != 0u) {
            const uint64_t p = pos[r] + count[r] + cull_rank(ballot, lane);
            if (keep && p < a.capacity) reinterpret_cast<uint2*>(a.pairs)[p] = make_uint2(row_i[r], j);
          }
          count[r] += cull_popcount(ballot);
        }
      }
    }
  }
  if (MODE == NSELF_SEED) {
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
      nself_seed_wave_reduce(best[r]);
      if (lane == 0u && row_i[r] < n) {
        NselfRowSeed out;
        out.L = best[r].L;
        out.j = best[r].key == NSELF_NO_PAIR ? SCENE_NONE : uint32_t(best[r].key);
        out.pad = 0u;
        row_seeds[row_i[r]] = out;
      }
    }
  } else if (MODE == NSELF_COUNT && lane == 0u) {
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r)
      if (row_i[r] < n) a.row_counts[chunk_row + wave * PAIRS_WAVE_ROWS + r] = count[r];
  }
}

// a wave per configuration (a row block is the configuration: rows_per_block = n_objects <= 64, blocks_per_conf = 1)
template <int MODE, bool GROUPS>
__global__ void __launch_bounds__(256) k_nself_small(NselfArgs na) {
  const PairsArgs& a = na.p;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (b >= a.n_blocks) return;
  const uint32_t n = a.n_objects;
  const uint64_t c = a.g0 + b;
  const double* __restrict__ boxes = a.boxes + 6u * ((c - a.c_box0) * n);
  const uint64_t chunk_row = c * n - a.row0;
  double col_box[6];
  for (int k = 0; k < 6; ++k) col_box[k] = boxes[6u * size_t(lane < n ? lane : 0u) + k];
  const NearestBoxTerms col_terms = nearest_box_terms(col_box);
  const double col_big = nself_pack_largest(col_terms);
  const uint32_t col_group = GROUPS ? a.group[lane < n ? lane : 0u] : 0u;
  const uint64_t seed = MODE == NSELF_SEED ? NSELF_NO_PAIR : na.seed[c];
  const double thr = (MODE != NSELF_SEED && na.pass == 2) ? na.thr[c] : 0.0;
  NselfSeed best;
  nself_seed_init(best);
  for (uint32_t i = 0; i < n; ++i) {
    double row_box[6];
    for (int k = 0; k < 6; ++k) row_box[k] = __shfl(col_box[k], int(i), 64);
    const NearestBoxTerms row_terms = nself_unpack(__shfl(col_terms.diagonal, int(i), 64), __shfl(col_big, int(i), 64));
    const bool candidate = lane > i && lane < n && (!GROUPS || pairs_allowed(a.collides[a.group[i] & 63u], col_group));
    const double L = nearest_bound_terms(row_box, row_terms, col_box, col_terms, na.r);
    if (MODE == NSELF_SEED) {
      if (candidate && L < best.L) {  // (the rows ascend: the first of equal values has the lowest i of this column)
        best.L = L;
        best.key = nself_key(i, lane);
      }
    } else {
      const bool keep = candidate && nself_in_pass(na.pass, L, nself_key(i, lane), seed, na.upper, thr);
      const uint64_t ballot = __ballot(keep);
      if (MODE == NSELF_EMIT) {
        const uint64_t p = a.row_offsets[chunk_row + i] + cull_rank(ballot, lane);
        if (keep && p < a.capacity) reinterpret_cast<uint2*>(a.pairs)[p] = make_uint2(i, lane);
      } else if (lane == 0u) {
        a.row_counts[chunk_row + i] = cull_popcount(ballot);
      }
    }
  }
  if (MODE == NSELF_SEED) {
    nself_seed_wave_reduce(best);
    if (lane == 0u) na.seed[c] = best.key;
  }
}

__global__ void __launch_bounds__(256) k_nself_seed_combine(NselfArgs na) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n = na.p.n_objects;
  const NselfRowSeed* __restrict__ rows = static_cast<const NselfRowSeed*>(na.row_seeds);
  for (uint64_t c = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); c < na.p.n_conf; c += uint64_t(gridDim.x) * 4u) {
    NselfSeed s;
    nself_seed_init(s);
    for (uint32_t i = lane; i < n; i += 64u) {
      const NselfRowSeed o = rows[c * n + i];
      if (o.j != SCENE_NONE) nself_seed_merge(s, o.L, nself_key(i, o.j));
    }
    nself_seed_wave_reduce(s);
    if (lane == 0u) na.seed[c] = s.key;
  }
}

template <typename R>
__global__ void __launch_bounds__(256) k_nself_combine(NselfCombineArgs a) {
  const uint64_t c = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (c >= a.n_conf) return;
  const R* rec[2] = {static_cast<const R*>(a.rec[0]), static_cast<const R*>(a.rec[1])};
  hfcl_scene_clearance out;
  nself_combine<R>(c, a.summary, a.pairs, a.conf_begin, rec, out, a.min_out ? static_cast<R*>(a.min_out) + c : nullptr);
  a.out[c] = out;
}

void launch_nself_seed(hipStream_t st, const NselfArgs& a) {
  const bool groups = a.p.group != nullptr;
  const dim3 grid(a.p.small ? (a.p.n_blocks + 3u) / 4u : a.p.n_blocks);
  void (*const k)(NselfArgs) = a.p.small ? (groups ? k_nself_small<NSELF_SEED, true> : k_nself_small<NSELF_SEED, false>)
                                         : (groups ? k_nself_sweep<NSELF_SEED, true> : k_nself_sweep<NSELF_SEED, false>);
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, a);
}
void launch_nself_seed_combine(hipStream_t st, const NselfArgs& a, int max_blocks) {
  if (!a.p.n_conf) return;
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((a.p.n_conf + 3u) / 4u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_nself_seed_combine, dim3(grid), dim3(256), 0, st, a);
}
void launch_nself_chunk(hipStream_t st, const NselfArgs& a) {
  const bool groups = a.p.group != nullptr;
  const dim3 grid(a.p.small ? (a.p.n_blocks + 3u) / 4u : a.p.n_blocks);
  void (*const count)(NselfArgs) = a.p.small ? (groups ? k_nself_small<NSELF_COUNT, true> : k_nself_small<NSELF_COUNT, false>)
                                             : (groups ? k_nself_sweep<NSELF_COUNT, true> : k_nself_sweep<NSELF_COUNT, false>);
  void (*const emit)(NselfArgs) = a.p.small ? (groups ? k_nself_small<NSELF_EMIT, true> : k_nself_small<NSELF_EMIT, false>)
                                            : (groups ? k_nself_sweep<NSELF_EMIT, true> : k_nself_sweep<NSELF_EMIT, false>);
  hipLaunchKernelGGL(count, grid, dim3(256), 0, st, a);
  launch_pairs_scan(st, a.p);
  if (!a.p.pairs || !a.p.capacity) return;  // count only
  hipLaunchKernelGGL(emit, grid, dim3(256), 0, st, a);
}
void launch_nself_combine(hipStream_t st, const NselfCombineArgs& a, bool f32) {
  if (!a.n_conf) return;
  const uint32_t grid = uint32_t((a.n_conf + 255u) / 256u);
  if (f32)
    hipLaunchKernelGGL(k_nself_combine<hfcl_result_f32>, dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_nself_combine<hfcl_result>, dim3(grid), dim3(256), 0, st, a);
}
