// hfcl_k_pairs.hip -- the self-collision pairs of a scene per configuration on the device (hfcl_scene_self_pairs*): a tiled all-pairs test of
// the world boxes k_cull_aabbs computes (hfcl_k_cull.hip), compacted by count / scan / emit.  hfcl_pairs.hpp has the arithmetic and the
// geometry of rows, row blocks and chunks.  Built without contraction (FLAGS_k_pairs): the grown boxes are the bits of cull_keep.
//   k_pairs_sweep<EMIT>   large scenes.  A workgroup owns a block of PAIRS_ROWS consecutive rows i of one configuration, a wave
//                         PAIRS_WAVE_ROWS of them, their grown boxes in registers.  The workgroup walks the column tiles j > i in ascending
//                         order: a tile's PAIRS_TILE boxes come in as 16-byte loads (three a box), are grown and stored component by component
//                         (6 x PAIRS_TILE doubles: a lane's ds_read_b64 of column j is 8 bytes beside its neighbour's, no bank conflict); per 64
//                         columns a lane reads its column once and tests it against the wave's rows, a ballot per row.  Count: the popcounts
//                         add up to a uint32 per row.  Emit: the same walk; a surviving column's position is the row's offset + the row's
//                         count so far + the ballot's bits below the lane -- ascending by construction --, written below the capacity.
//   k_pairs_small<EMIT>   scenes of at most 64 objects: a wave per configuration, lane = column j with its grown box in registers, a loop over
//                         the rows i whose box comes from lane i (readlane); the same counts, the same positions.
//   k_pairs_sweep_groups<EMIT> / k_pairs_small_groups<EMIT>   the same two forms for a scene with object groups (hppfcl_amd_groups.h):
//                         a pair is kept iff its boxes touch and bit group[j] of collides[group[i]] is set.  The tiled form -- the second
//                         instantiation of the body k_pairs_sweep shares with it -- stages a tile's
//                         group bytes next to its boxes (256 B of LDS), keeps a row's mask wave-uniform, and skips -- in front of the
//                         barriers, by a decision the whole workgroup shares (pairs_block_mask) -- every column tile none of whose groups
//                         (tile_groups, built on the host) may pair with any row of the block; a block that may pair with nothing writes
//                         its rows' zero counts and leaves.  The emit pass takes the same decisions.
//   k_pairs_scan_sums     a workgroup per PAIRS_SCAN_BLOCK rows of the chunk: their entries
//   k_pairs_scan_top      one workgroup (the structure of k_cull_scan): exclusive scan of those sums on top of the chunks before
//   k_pairs_scan_rows     a workgroup per PAIRS_SCAN_BLOCK rows: the rows' offsets, conf_begin of the configurations whose first row is in the
//                         chunk, and with the table's last row conf_begin[n_conf] and the count
// No atomics, no scratch, no kernel waits for another workgroup; the list is the same bytes however the call is cut into chunks.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_pairs.hpp"

static __device__ __forceinline__ PairsGeometry pairs_geometry_of(const PairsArgs& a) {
  PairsGeometry g;
  g.n_objects = a.n_objects;
  g.rows_per_block = a.rows_per_block;
  g.blocks_per_conf = a.blocks_per_conf;
  return g;
}

// the body of k_pairs_sweep<EMIT> (GROUPS = false: the code of the kernel as it was) and of k_pairs_sweep_groups<EMIT>
template <bool EMIT, bool GROUPS>
static __device__ __forceinline__ void pairs_sweep_body(PairsArgs a) {
  __shared__ double tile[6][PAIRS_TILE];
  __shared__ uint8_t tile_group[GROUPS ? PAIRS_TILE : 1u];  // (GROUPS: the tile's groups next to its boxes)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t n = a.n_objects;
  uint64_t c;
  uint32_t i0, i1;
  pairs_block(pairs_geometry_of(a), a.g0 + blockIdx.x, c, i0, i1);
  const double* __restrict__ boxes = a.boxes + 6u * ((c - a.c_box0) * n);
  const uint64_t chunk_row = c * n + i0 - a.row0;  // the block's first row in the chunk's row arrays

  // GROUPS: the block's mask, from ALL rows of the block -- the same value in the four waves, so that what is skipped in front of the
  // barriers below is skipped by the whole workgroup.  A block that may pair with nothing leaves; the scan still reads its rows' counts
  uint64_t block_mask = 0;
  if (GROUPS) {
    block_mask = pairs_block_mask(a.group, a.collides, i0, i1);
    if (block_mask == 0u) {
      if (!EMIT && threadIdx.x < i1 - i0) a.row_counts[chunk_row + threadIdx.x] = 0u;
      return;
    }
  }

  // the wave's rows: i0 + wave * PAIRS_WAVE_ROWS + r (past i1: no row -- its tests fail on j < n with a row index of n)
  double row_box[PAIRS_WAVE_ROWS][6];
  uint32_t row_i[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
  uint64_t pos[PAIRS_WAVE_ROWS];
  uint64_t row_mask[GROUPS ? PAIRS_WAVE_ROWS : 1u];  // collides[group of the row]: wave-uniform; 0 for a row past i1
  for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
    const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
    const bool there = i < i1;
    row_i[r] = there ? i : n;
    count[r] = 0u;
    if (GROUPS) {  // (uniform in the wave, which the compiler cannot see of threadIdx.x >> 6: held in scalar registers, 22 VGPRs fewer)
      const uint64_t m = there ? a.collides[a.group[i] & 63u] : 0u;
      const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m)))), hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(m >> 32))));
      row_mask[r] = (uint64_t(hi) << 32) | lo;  // (the builtin returns an int: widened as it is, a low word with its top bit set would fill the high one)
    }
    double raw[6];
    for (int k = 0; k < 6; ++k) raw[k] = boxes[6u * size_t(there ? i : i0) + k];
    pairs_grow(raw, a.inflate, row_box[r]);
    pos[r] = EMIT && there ? a.row_offsets[chunk_row + wave * PAIRS_WAVE_ROWS + r] : 0u;
  }

  const double2* __restrict__ vec = reinterpret_cast<const double2*>(boxes);  // (a box: 48 B, three vectors; the table is 16-byte aligned)
  for (uint32_t base = pairs_first_tile(i0); base < n; base += PAIRS_TILE) {
    if (GROUPS && pairs_tile_skipped(a.tile_groups[base / PAIRS_TILE], block_mask)) continue;  // (workgroup-uniform: no loads, no barrier)
    __syncthreads();  // (the tile before has been read)
    for (uint32_t v = threadIdx.x; v < 3u * PAIRS_TILE; v += 256u) {
      const uint32_t col = v / 3u, part = v - 3u * col;
      if (base + col < n) {
        const double2 x = vec[3u * size_t(base) + v];
        // components 2 part, 2 part + 1 of the box: min below 3, max from 3 on
        tile[2u * part][col] = part < 2u ? x.x - a.inflate : x.x + a.inflate;
        tile[2u * part + 1u][col] = part < 1u ? x.y - a.inflate : x.y + a.inflate;
      }
    }
    if (GROUPS)
      for (uint32_t col = threadIdx.x; col < PAIRS_TILE; col += 256u)
        if (base + col < n) tile_group[col] = a.group[base + col];
    __syncthreads();
    for (uint32_t step = 0; step < PAIRS_TILE; step += 64u) {
      const uint32_t j = base + step + lane;
      double col_box[6];
      for (int k = 0; k < 6; ++k) col_box[k] = tile[k][step + lane];  // (columns past n: stale values, refused by j < n)
      const uint32_t col_group = GROUPS ? tile_group[step + lane] : 0u;  // (consecutive lanes, consecutive bytes: no bank conflict)
      for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
        const bool keep = pairs_keep(row_i[r], j, n, row_box[r], col_box) && (!GROUPS || pairs_allowed(row_mask[r], col_group));
        const uint64_t ballot = __ballot(keep);
        if (EMIT && ballot != 0u) {  // (most steps list nothing: cfg5's scene keeps one test in 4 700)
          const uint64_t p = pos[r] + count[r] + cull_rank(ballot, lane);
          if (keep && p < a.capacity) reinterpret_cast<uint2*>(a.pairs)[p] = make_uint2(row_i[r], j);
        }
        count[r] += cull_popcount(ballot);
      }
    }
  }
  if (!EMIT && lane == 0u)
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r)
      if (row_i[r] < n) a.row_counts[chunk_row + wave * PAIRS_WAVE_ROWS + r] = count[r];
}
template <bool EMIT>
__global__ void __launch_bounds__(256) k_pairs_sweep(PairsArgs a) {
  pairs_sweep_body<EMIT, false>(a);
}
template <bool EMIT>
__global__ void __launch_bounds__(256) k_pairs_sweep_groups(PairsArgs a) {
  pairs_sweep_body<EMIT, true>(a);
}

// a wave per configuration (a row block is the configuration: rows_per_block = n_objects <= 64, blocks_per_conf = 1)
template <bool EMIT>
__global__ void __launch_bounds__(256) k_pairs_small(PairsArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (b >= a.n_blocks) return;
  const uint32_t n = a.n_objects;
  const uint64_t c = a.g0 + b;
  const double* __restrict__ boxes = a.boxes + 6u * ((c - a.c_box0) * n);
  const uint64_t chunk_row = c * n - a.row0;
  double raw[6], col_box[6];
  for (int k = 0; k < 6; ++k) raw[k] = boxes[6u * size_t(lane < n ? lane : 0u) + k];
  pairs_grow(raw, a.inflate, col_box);
  for (uint32_t i = 0; i < n; ++i) {
    double row_box[6];
    for (int k = 0; k < 6; ++k) row_box[k] = __shfl(col_box[k], int(i), 64);
    const bool keep = pairs_keep(i, lane, n, row_box, col_box);
    const uint64_t ballot = __ballot(keep);
    if (EMIT) {
      const uint64_t p = a.row_offsets[chunk_row + i] + cull_rank(ballot, lane);
      if (keep && p < a.capacity) reinterpret_cast<uint2*>(a.pairs)[p] = make_uint2(i, lane);
    } else if (lane == 0u) {
      a.row_counts[chunk_row + i] = cull_popcount(ballot);
    }
  }
}
// ... with object groups: the lane keeps its column's group, the row's mask is the one of lane i's group (wave-uniform); no tiles.
// (A kernel of its own, not a second instantiation of a shared body as the tiled form is: with its body moved into an inlined function
// k_pairs_small<true> allocates 36 registers instead of 34 -- the compiler's handling of the argument block, not the code -- and the
// kernels without groups are to stay the kernels they were.)
template <bool EMIT>
__global__ void __launch_bounds__(256) k_pairs_small_groups(PairsArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (b >= a.n_blocks) return;
  const uint32_t n = a.n_objects;
  const uint64_t c = a.g0 + b;
  const double* __restrict__ boxes = a.boxes + 6u * ((c - a.c_box0) * n);
  const uint64_t chunk_row = c * n - a.row0;
  double raw[6], col_box[6];
  for (int k = 0; k < 6; ++k) raw[k] = boxes[6u * size_t(lane < n ? lane : 0u) + k];
  pairs_grow(raw, a.inflate, col_box);
  const uint32_t col_group = a.group[lane < n ? lane : 0u];
  for (uint32_t i = 0; i < n; ++i) {
    double row_box[6];
    for (int k = 0; k < 6; ++k) row_box[k] = __shfl(col_box[k], int(i), 64);
    const bool keep = pairs_keep(i, lane, n, row_box, col_box) && pairs_allowed(a.collides[a.group[i] & 63u], col_group);
    const uint64_t ballot = __ballot(keep);
    if (EMIT) {
      const uint64_t p = a.row_offsets[chunk_row + i] + cull_rank(ballot, lane);
      if (keep && p < a.capacity) reinterpret_cast<uint2*>(a.pairs)[p] = make_uint2(i, lane);
    } else if (lane == 0u) {
      a.row_counts[chunk_row + i] = cull_popcount(ballot);
    }
  }
}

// ---- the scan of a chunk's row counts ---------------------------------------------------------------------------------------------
// the four consecutive rows of a thread of a scan workgroup: rows [4 t, 4 t + 4) of the workgroup's PAIRS_SCAN_BLOCK
static __device__ __forceinline__ uint32_t scan_rows_of(const PairsArgs& a, uint32_t* cnt) {
  const uint32_t r0 = blockIdx.x * PAIRS_SCAN_BLOCK + 4u * threadIdx.x;
  uint32_t sum = 0;
  for (uint32_t k = 0; k < 4u; ++k) {
    cnt[k] = r0 + k < a.n_rows ? a.row_counts[r0 + k] : 0u;
    sum += cnt[k];
  }
  return sum;
}
// inclusive scan of `mine` over the workgroup's 256 threads (wave_sum: four words of LDS); total: the workgroup's sum
static __device__ __forceinline__ uint32_t scan_block_inclusive(uint32_t mine, uint32_t* wave_sum, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off, 64);
    if (lane >= uint32_t(off)) incl += up;
  }
  if (lane == 63u) wave_sum[wave] = incl;
  __syncthreads();
  total = 0;
  for (uint32_t w = 0; w < 4u; ++w) {
    if (w < wave) incl += wave_sum[w];
    total += wave_sum[w];
  }
  return incl;
}

// (32-bit sums: a row has fewer than n_objects entries and the host refuses scenes of more than 2^32 / PAIRS_SCAN_BLOCK objects)
__global__ void __launch_bounds__(256) k_pairs_scan_sums(PairsArgs a) {
  __shared__ uint32_t wave_sum[4];
  uint32_t cnt[4], total;
  scan_block_inclusive(scan_rows_of(a, cnt), wave_sum, total);
  if (threadIdx.x == 0u) a.sums[blockIdx.x] = total;
}

// One workgroup.  Thread t owns the sums [t * share, (t + 1) * share): their sum, a scan of the 256 sums, then the offsets (k_cull_scan).
__global__ void __launch_bounds__(256) k_pairs_scan_top(PairsArgs a, uint32_t n_sums) {
  __shared__ uint64_t wave_sum[4];
  const uint32_t share = (n_sums + 255u) / 256u;
  const uint32_t lo = threadIdx.x * share < n_sums ? threadIdx.x * share : n_sums;
  const uint32_t hi = lo + share < n_sums ? lo + share : n_sums;
  const uint64_t before = a.first ? 0u : *a.running;
  uint64_t mine = 0;
  for (uint32_t b = lo; b < hi; ++b) mine += a.sums[b];
  uint64_t incl = mine;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t up = __shfl_up(incl, off, 64);
    if (lane >= uint32_t(off)) incl += up;
  }
  if (lane == 63u) wave_sum[wave] = incl;
  __syncthreads();  // (every thread has read *running by now)
  uint64_t run = before + incl - mine;
  for (uint32_t w = 0; w < wave; ++w) run += wave_sum[w];
  for (uint32_t b = lo; b < hi; ++b) {
    a.sum_offsets[b] = run;
    run += a.sums[b];
  }
  if (threadIdx.x == 255u) *a.running = run;
}

__global__ void __launch_bounds__(256) k_pairs_scan_rows(PairsArgs a) {
  __shared__ uint32_t wave_sum[4];
  uint32_t cnt[4], total;
  const uint32_t mine = scan_rows_of(a, cnt);
  const uint32_t incl = scan_block_inclusive(mine, wave_sum, total);
  uint64_t off = a.sum_offsets[blockIdx.x] + (incl - mine);
  const uint32_t r0 = blockIdx.x * PAIRS_SCAN_BLOCK + 4u * threadIdx.x;
  for (uint32_t k = 0; k < 4u && r0 + k < a.n_rows; ++k) {
    a.row_offsets[r0 + k] = off;
    pairs_row_marks(a.row0 + r0 + k, off, cnt[k], a.n_objects, a.total_rows, a.n_conf, a.conf_begin, a.n_listed);
    off += cnt[k];
  }
}

// the scan of a chunk's row counts (also behind the counts of hfcl_k_nearest_self.hip)
void launch_pairs_scan(hipStream_t st, const PairsArgs& a) {
  const uint32_t n_sums = (a.n_rows + PAIRS_SCAN_BLOCK - 1u) / PAIRS_SCAN_BLOCK;
  hipLaunchKernelGGL(k_pairs_scan_sums, dim3(n_sums), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_pairs_scan_top, dim3(1), dim3(256), 0, st, a, n_sums);
  hipLaunchKernelGGL(k_pairs_scan_rows, dim3(n_sums), dim3(256), 0, st, a);
}

void launch_pairs_chunk(hipStream_t st, const PairsArgs& a) {
  const uint32_t small_grid = (a.n_blocks + 3u) / 4u;
  // with object groups (hfcl_scene_set_groups: the three tables come together) the kernels that read them
  const bool groups = a.group != nullptr;
  void (*const count)(PairsArgs) = a.small ? (groups ? k_pairs_small_groups<false> : k_pairs_small<false>)
                                           : (groups ? k_pairs_sweep_groups<false> : k_pairs_sweep<false>);
  void (*const emit)(PairsArgs) = a.small ? (groups ? k_pairs_small_groups<true> : k_pairs_small<true>)
                                          : (groups ? k_pairs_sweep_groups<true> : k_pairs_sweep<true>);
  const dim3 grid(a.small ? small_grid : a.n_blocks);
  hipLaunchKernelGGL(count, grid, dim3(256), 0, st, a);
  launch_pairs_scan(st, a);
  if (!a.pairs || !a.capacity) return;  // count only
  hipLaunchKernelGGL(emit, grid, dim3(256), 0, st, a);
}
