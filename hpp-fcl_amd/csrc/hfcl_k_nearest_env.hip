// hfcl_k_nearest_env.hip -- the clearance of the moving objects of a scene among an environment kept on the device
// (include/hppfcl_amd_nearest_env.h: hfcl_scene_nearest_env*): the set-time tables of the bound's terms, and the sweeps that make the seeds
// and the two passes' lists of pairs.  The narrow phase runs through the path of the env lists (hfcl_k_env.hip), the scans are those of
// hfcl_k_pairs.hip, thresholds and the combination of the two passes those of hfcl_k_nearest.hip / hfcl_k_nearest_self.hip.
// hfcl_nearest_env.hpp has the arithmetic.  Built without contraction (FLAGS_k_nearest_env): the bounds are the bits of nearest_bound.
//   k_nenv_terms          set time: a thread per environment box writes its two terms, then (a second launch) a thread per tile folds its
//                         members' in member order
//   k_nenv_sweep<MODE, GROUPS>   the cells of k_env_sweep: a workgroup owns PAIRS_ROWS moving rows of one configuration -- box and the
//                         box's terms in registers -- times a span of column tiles, the moving columns j > i first, the environment's tiles
//                         behind them.  A tile is staged as 8 doubles a column, as in k_nself_sweep: a moving column's terms are computed
//                         when it is loaded, an environment column's are loaded (no square root at sweep time).  A tile is skipped -- in
//                         front of the barriers, by a value the whole workgroup shares -- when none of its groups may pair with any row of
//                         the block, or, an environment tile in pass 1 / pass 2, by nenv_tile_dropped on nenv_tile_bound of the block and
//                         the tile: it holds no pair of the pass.
//                         MODE seed: a row's smallest L in the span and its lowest j, one 16-byte partial per (row, span).
//                         MODE count / emit: the predicate of pass 1 / pass 2 (seed[c], thr[c]: uniform loads), a uint32 per (row, span),
//                         row-major; the scan is launch_pairs_scan with rows x spans as its rows; positions by ballots.
//   k_nenv_seed_combine   a wave per configuration folds its n_moving * n_spans partials: butterfly, on a tie the lowest (i, j)
// No atomics, no scratch, no kernel waits for another workgroup; the lists are the same bytes however the call is cut into chunks and
// spans and whether or not cells are dropped by distance.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_nearest_env.hpp"

constexpr int NENV_SEED = 0, NENV_COUNT = 1, NENV_EMIT = 2;

__global__ void __launch_bounds__(256) k_nenv_terms(const double* __restrict__ env_boxes, uint32_t n_env, double* __restrict__ env_terms) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n_env) return;
  nenv_box_terms(env_boxes + 6u * size_t(e), env_terms + 2u * size_t(e));
}
__global__ void __launch_bounds__(256) k_nenv_tile_terms(const double* __restrict__ env_terms, uint32_t n_env, double* __restrict__ tile_terms) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= env_tiles(n_env)) return;
  nenv_tile_terms(env_terms, n_env, t, tile_terms + 2u * size_t(t));
}
void launch_nenv_terms(hipStream_t st, const double* env_boxes, uint32_t n_env, double* env_terms, double* tile_terms) {
  if (!n_env) return;
  hipLaunchKernelGGL(k_nenv_terms, dim3((n_env + 255u) / 256u), dim3(256), 0, st, env_boxes, n_env, env_terms);
  hipLaunchKernelGGL(k_nenv_tile_terms, dim3((env_tiles(n_env) + 255u) / 256u), dim3(256), 0, st, env_terms, n_env, tile_terms);
}

// a decision every lane took from the same values, as a scalar: what it guards lies in front of a workgroup barrier
static __device__ __forceinline__ bool nenv_uniform(bool x) { return __builtin_amdgcn_readfirstlane(int(x)) != 0; }
static __device__ __forceinline__ uint64_t nenv_uniform64(uint64_t m) {
  const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m)))), hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m >> 32))));
  return (uint64_t(hi) << 32) | lo;
}
// butterfly over the 64 lanes: the smallest L, on a tie the lowest key
static __device__ __forceinline__ void nenv_seed_wave_reduce(NselfSeed& s) {
  for (int off = 32; off > 0; off >>= 1) {
    const double L = __shfl_xor(s.L, off, 64);
    const uint32_t lo = __shfl_xor(uint32_t(s.key), off, 64), hi = __shfl_xor(uint32_t(s.key >> 32), off, 64);
    nself_seed_merge(s, L, (uint64_t(hi) << 32) | lo);
  }
}

template <int MODE, bool GROUPS>
__global__ void __launch_bounds__(256) k_nenv_sweep(NenvArgs na) {
  const EnvArgs& a = na.e;
  __shared__ double tile[8][PAIRS_TILE];  // box, diagonal, largest |coordinate| (negative: not finite)
  __shared__ uint8_t tile_group[GROUPS ? PAIRS_TILE : 1u];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t nm = a.n_moving, n = nm + a.n_env;
  const uint32_t blk = blockIdx.x / a.n_spans, span = blockIdx.x - blk * a.n_spans;
  PairsGeometry geo;
  geo.n_objects = nm;
  geo.rows_per_block = PAIRS_ROWS;
  geo.blocks_per_conf = a.blocks_per_conf;
  EnvGeometry eg;
  eg.n_moving = nm;
  eg.n_env = a.n_env;
  eg.tiles_moving = a.tiles_moving;
  eg.tiles = a.tiles;
  eg.span_len = a.span_len;
  eg.n_spans = a.n_spans;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(geo, a.p.g0 + blk, c, i0, i1);
  const double* __restrict__ boxes = a.p.boxes + 6u * ((c - a.p.c_box0) * nm);  // the configuration's moving boxes
  const uint64_t chunk_row = c * nm + i0 - a.row0;                              // the block's first row in the chunk
  NselfRowSeed* __restrict__ row_seeds = static_cast<NselfRowSeed*>(na.row_seeds);  // (row, span) partials of the WHOLE table

  // what the whole workgroup shares: the groups any row of the block may pair with, the block as one box, the configuration's seed and threshold
  uint64_t block_mask = ~uint64_t(0);
  if (GROUPS) block_mask = pairs_block_mask(a.p.group, a.p.collides, i0, i1);
  const bool prune = MODE != NENV_SEED && na.prune != 0;
  __shared__ double block_part[4][8];
  const int mode = MODE == NENV_SEED ? 0 : na.pass;
  const uint64_t seed = MODE == NENV_SEED ? NSELF_NO_PAIR : na.seed[c];
  const double thr = (MODE != NENV_SEED && na.pass == 2) ? na.thr[c] : 0.0;

  double row_box[PAIRS_WAVE_ROWS][6], row_diag[PAIRS_WAVE_ROWS], row_big[PAIRS_WAVE_ROWS];
  uint32_t row_i[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
  uint64_t pos[PAIRS_WAVE_ROWS];
  uint64_t row_mask[GROUPS ? PAIRS_WAVE_ROWS : 1u];
  NselfSeed best[MODE == NENV_SEED ? PAIRS_WAVE_ROWS : 1u];  // (key: the column alone)
  for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
    const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
    const bool there = i < i1;
    row_i[r] = there ? i : n;  // (no row: its tests fail on j > i)
    count[r] = 0u;
    if (GROUPS) row_mask[r] = nenv_uniform64(there ? a.p.collides[a.p.group[i] & 63u] : 0u);
    for (int k = 0; k < 6; ++k) row_box[r][k] = boxes[6u * size_t(there ? i : i0) + k];
    const NearestBoxTerms t = nearest_box_terms(row_box[r]);
    row_diag[r] = t.diagonal;
    row_big[r] = nself_pack_largest(t);
    pos[r] = MODE == NENV_EMIT && there ? a.p.row_offsets[(chunk_row + wave * PAIRS_WAVE_ROWS + r) * a.n_spans + span] : 0u;
    if (MODE == NENV_SEED) nself_seed_init(best[r]);
  }
  // the block as one box, from the rows the waves hold (a row that is not there holds row i0 once more, which changes nothing): every
  // wave folds its own, the four parts meet in LDS -- no load, no square root beyond the rows' own
  NenvBlock block;
  nenv_block_init(block);
  if (prune) {  // (a kernel argument: the whole workgroup takes the barrier or none of it does)
    NenvBlock mine;
    nenv_block_init(mine);
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) nenv_block_add(mine, row_box[r], row_diag[r], row_big[r]);
    double w[8];
    nenv_block_pack(mine, w);
    if (lane == 0u)
      for (int k = 0; k < 8; ++k) block_part[wave][k] = w[k];
    __syncthreads();
    for (uint32_t v = 0; v < 4u; ++v) {
      double part[8];
      for (int k = 0; k < 8; ++k) part[k] = block_part[v][k];
      nenv_block_merge(block, part);
    }
  }

  uint32_t u0 = span * a.span_len;
  const uint32_t u1 = a.tiles - u0 > a.span_len ? u0 + a.span_len : a.tiles;
  const uint32_t first = env_first_tile(i0, a.tiles_moving);
  if (u0 < first) u0 = first;
  if (GROUPS && block_mask == 0u) u0 = u1;  // (a block that may pair with nothing: no candidate)
  for (uint32_t u = u0; u < u1; ++u) {
    bool env;
    uint32_t base, j0, j_end;
    env_tile_columns(eg, u, env, base, j0, j_end);
    if (GROUPS && pairs_tile_skipped(a.col_tile_groups[u], block_mask)) continue;  // (workgroup-uniform: no loads, no barrier)
    const uint32_t cols = j_end - j0 < PAIRS_TILE ? j_end - j0 : PAIRS_TILE;  // columns of the tile
    if (prune && env) {  // (the same: every lane computes the cell's bound from the same values)
      const uint32_t t = base / PAIRS_TILE;
      const double Lt = nenv_tile_bound(block, a.env_tile_boxes + 6u * size_t(t), na.env_tile_terms + 2u * size_t(t), na.r);
      if (nenv_uniform(nenv_tile_dropped(mode, Lt, seed, i0, i1, j0, cols, thr))) continue;
    }
    const double2* __restrict__ vec = reinterpret_cast<const double2*>(env ? a.env_boxes : boxes) + 3u * size_t(base);  // (48 B a box, 16-byte aligned tables)
    const double2* __restrict__ terms = reinterpret_cast<const double2*>(na.env_terms) + base;
    __syncthreads();  // (the tile before has been read)
    for (uint32_t col = threadIdx.x; col < cols; col += 256u) {
      const double2 x = vec[3u * col], y = vec[3u * col + 1u], z = vec[3u * col + 2u];
      const double box[6] = {x.x, x.y, y.x, y.y, z.x, z.y};
      for (int k = 0; k < 6; ++k) tile[k][col] = box[k];
      if (env) {  // (workgroup-uniform)
        const double2 t = terms[col];
        tile[6][col] = t.x;
        tile[7][col] = t.y;
      } else {
        const NearestBoxTerms t = nearest_box_terms(box);  // (once per box and tile, not once per test)
        tile[6][col] = t.diagonal;
        tile[7][col] = nself_pack_largest(t);
      }
      if (GROUPS) tile_group[col] = a.p.group[j0 + col];
    }
    __syncthreads();
    for (uint32_t step = 0; step < PAIRS_TILE; step += 64u) {
      const uint32_t j = j0 + step + lane;
      double col_box[6];
      for (int k = 0; k < 6; ++k) col_box[k] = tile[k][step + lane];  // (columns past the tile's: stale values, refused by j < j_end)
      const NearestBoxTerms col_terms = nself_unpack(tile[6][step + lane], tile[7][step + lane]);
      const uint32_t col_group = GROUPS ? tile_group[step + lane] : 0u;
      for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
        const bool candidate = j > row_i[r] && j < j_end && step + lane < cols && (!GROUPS || pairs_allowed(row_mask[r], col_group));
        const double L = nearest_bound_terms(row_box[r], nself_unpack(row_diag[r], row_big[r]), col_box, col_terms, na.r);
        if (MODE == NENV_SEED) {
          if (candidate && L < best[r].L) {  // (a lane's columns ascend: the first of equal values is the lowest)
            best[r].L = L;
            best[r].key = j;
          }
        } else {
          const bool keep = candidate && nself_in_pass(na.pass, L, nself_key(row_i[r], j), seed, na.upper, thr);
          const uint64_t ballot = __ballot(keep);
          if (MODE == NENV_EMIT && ballot != 0u) {
            const uint64_t p = pos[r] + count[r] + cull_rank(ballot, lane);
            if (keep && p < a.p.capacity) reinterpret_cast<uint2*>(a.p.pairs)[p] = make_uint2(row_i[r], j);
          }
          count[r] += cull_popcount(ballot);
        }
      }
    }
  }
  if (MODE == NENV_SEED) {
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
      nenv_seed_wave_reduce(best[r]);
      if (lane == 0u && row_i[r] < n) {
        NselfRowSeed out;
        out.L = best[r].L;
        out.j = best[r].key == NSELF_NO_PAIR ? SCENE_NONE : uint32_t(best[r].key);
        out.pad = 0u;
        row_seeds[(c * nm + row_i[r]) * a.n_spans + span] = out;
      }
    }
  } else if (MODE == NENV_COUNT && lane == 0u) {
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r)
      if (row_i[r] < n) a.p.row_counts[(chunk_row + wave * PAIRS_WAVE_ROWS + r) * a.n_spans + span] = count[r];
  }
}

__global__ void __launch_bounds__(256) k_nenv_seed_combine(NenvArgs na) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t per_conf = uint64_t(na.e.n_moving) * na.e.n_spans;
  const NselfRowSeed* __restrict__ rows = static_cast<const NselfRowSeed*>(na.row_seeds);
  for (uint64_t c = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); c < na.e.p.n_conf; c += uint64_t(gridDim.x) * 4u) {
    NselfSeed s;
    nself_seed_init(s);
    for (uint64_t x = lane; x < per_conf; x += 64u) nenv_seed_fold(s, rows + c * per_conf, na.e.n_spans, x);
    nenv_seed_wave_reduce(s);
    if (lane == 0u) na.seed[c] = s.key;
  }
}

void launch_nenv_seed(hipStream_t st, const NenvArgs& a) {
  const dim3 grid(a.e.p.n_blocks * a.e.n_spans);
  void (*const k)(NenvArgs) = a.e.p.group ? k_nenv_sweep<NENV_SEED, true> : k_nenv_sweep<NENV_SEED, false>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, a);
}
void launch_nenv_seed_combine(hipStream_t st, const NenvArgs& a, int max_blocks) {
  if (!a.e.p.n_conf) return;
  const uint32_t grid = uint32_t(std::max<uint64_t>(1u, std::min<uint64_t>((a.e.p.n_conf + 3u) / 4u, uint64_t(max_blocks))));
  hipLaunchKernelGGL(k_nenv_seed_combine, dim3(grid), dim3(256), 0, st, a);
}
void launch_nenv_chunk(hipStream_t st, const NenvArgs& a) {
  const bool groups = a.e.p.group != nullptr;
  const dim3 grid(a.e.p.n_blocks * a.e.n_spans);
  void (*const count)(NenvArgs) = groups ? k_nenv_sweep<NENV_COUNT, true> : k_nenv_sweep<NENV_COUNT, false>;
  void (*const emit)(NenvArgs) = groups ? k_nenv_sweep<NENV_EMIT, true> : k_nenv_sweep<NENV_EMIT, false>;
  hipLaunchKernelGGL(count, grid, dim3(256), 0, st, a);
  launch_pairs_scan(st, a.e.p);
  if (!a.e.p.pairs || !a.e.p.capacity) return;  // count only
  hipLaunchKernelGGL(emit, grid, dim3(256), 0, st, a);
}
