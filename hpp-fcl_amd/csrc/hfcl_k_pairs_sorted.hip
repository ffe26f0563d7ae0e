// hfcl_k_pairs_sorted.hip -- the self-collision pairs of a scene per configuration by sort and sweep along one axis (option
// scene_pairs_sorted): the list of hfcl_k_pairs.hip, byte for byte, for scenes whose all-pairs test is too much work.
// hfcl_pairs_sorted.hpp has the arithmetic and the argument why no touching pair is skipped.  Built without contraction
// (FLAGS_k_pairs_sorted): the grown boxes are the bits of cull_keep.  A chunk is a number of WHOLE configurations:
//   k_psort_spread / k_psort_axis   automatic axis: per configuration the axis on which the boxes' centres spread widest (min / max per
//                         workgroup of PSORT_SPREAD_BLOCK objects, then a wave per configuration)
//   k_psort_keys          a lane per (configuration, object): the word (configuration in the chunk, key of the grown min), the object
//   rocprim::radix_sort_pairs   device-wide, stable, over the bits in use
//   k_psort_gather        a lane per sorted position: the grown box, the group, and the window's end by binary search in the
//                         configuration's keys
//   k_psort_sweep<EMIT>   the hot path, shaped as k_pairs_sweep: a workgroup owns PAIRS_ROWS consecutive sorted positions of one
//                         configuration, a wave PAIRS_WAVE_ROWS of them, their boxes in registers.  The workgroup walks the column tiles
//                         of the positions' JOINT window [first position + 1, the largest end) -- PAIRS_TILE sorted boxes through LDS,
//                         component by component --, a wave skips the 64-column steps outside its own rows' windows.  Count: a uint32
//                         per position.  Emit: position's offset + count so far + ballot bits below the lane -> the word (configuration,
//                         min(i, j), max(i, j)).  An unbounded box (a tilted Plane) has the configuration as its window: its
//                         workgroup walks all tiles with all its lanes, as a row block of the all-pairs form does.
//   launch_pairs_scan     the scan of hfcl_k_pairs.hip over the sorted positions: their offsets, conf_begin, the count
//   rocprim::radix_sort_keys   the emitted words: c, then i, then j ascending
//   k_psort_write         (i, j) of the sorted words into the caller's list, below the capacity
// No atomics of our own, no scratch; the list does not depend on the axis or on the chunks.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_pairs_sorted.hpp"

// ---- the axis -----------------------------------------------------------------------------------------------------------------------
// workgroup c * spread_blocks + b: min / max of the finite centres of PSORT_SPREAD_BLOCK objects of configuration c
__global__ void __launch_bounds__(256) k_psort_spread(PairsSortedArgs a) {
  __shared__ double part[4][6];
  const uint32_t n = a.p.n_objects, c = blockIdx.x / a.spread_blocks;
  const uint32_t start = (blockIdx.x - c * a.spread_blocks) * PSORT_SPREAD_BLOCK;
  const uint32_t stop = n - start > PSORT_SPREAD_BLOCK ? start + PSORT_SPREAD_BLOCK : n;
  const double* __restrict__ boxes = a.p.boxes + 6u * (uint64_t(c) * n);
  const double inf = __builtin_inf();
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t i = start + threadIdx.x; i < stop; i += 256u) {
    double box[6];
    for (int k = 0; k < 6; ++k) box[k] = boxes[6u * size_t(i) + k];
    for (int k = 0; k < 3; ++k) {
      double centre;
      if (psort_centre(box, k, centre)) {
        lo[k] = centre < lo[k] ? centre : lo[k];
        hi[k] = centre > hi[k] ? centre : hi[k];
      }
    }
  }
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      const double l = __shfl_xor(lo[k], off, 64), h = __shfl_xor(hi[k], off, 64);
      lo[k] = l < lo[k] ? l : lo[k];
      hi[k] = h > hi[k] ? h : hi[k];
    }
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (lane == 0u)
    for (int k = 0; k < 3; ++k) {
      part[wave][k] = lo[k];
      part[wave][3 + k] = hi[k];
    }
  __syncthreads();
  if (threadIdx.x < 6u) {
    double v = part[0][threadIdx.x];
    for (uint32_t w = 1; w < 4u; ++w) {
      const double x = part[w][threadIdx.x];
      v = threadIdx.x < 3u ? (x < v ? x : v) : (x > v ? x : v);
    }
    a.spread[uint64_t(blockIdx.x) * 6u + threadIdx.x] = v;
  }
}
// a wave per configuration: the min / max over its workgroups, the axis
__global__ void __launch_bounds__(256) k_psort_axis(PairsSortedArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (c >= a.n_conf_chunk) return;
  const double inf = __builtin_inf();
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t b = lane; b < a.spread_blocks; b += 64u) {
    const double* s = a.spread + (uint64_t(c) * a.spread_blocks + b) * 6u;
    for (int k = 0; k < 3; ++k) {
      lo[k] = s[k] < lo[k] ? s[k] : lo[k];
      hi[k] = s[3 + k] > hi[k] ? s[3 + k] : hi[k];
    }
  }
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      const double l = __shfl_xor(lo[k], off, 64), h = __shfl_xor(hi[k], off, 64);
      lo[k] = l < lo[k] ? l : lo[k];
      hi[k] = h > hi[k] ? h : hi[k];
    }
  if (lane == 0u) a.conf_axis[c] = psort_pick_axis(lo, hi);
}

// ---- keys, gather, windows ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_psort_keys(PairsSortedArgs a) {
  const uint32_t n = a.p.n_objects;
  for (uint64_t r = uint64_t(blockIdx.x) * 256u + threadIdx.x; r < a.p.n_rows; r += uint64_t(gridDim.x) * 256u) {
    const uint32_t c = uint32_t(r / n);
    const uint32_t axis = a.axis < 3u ? a.axis : a.conf_axis[c];
    const double lo = a.p.boxes[6u * r + axis] - a.p.inflate;  // (pairs_grow's subtraction)
    a.keys[0][r] = psort_word(c, psort_key(lo));
    a.vals[0][r] = uint32_t(r - uint64_t(c) * n);
  }
}
__global__ void __launch_bounds__(256) k_psort_gather(PairsSortedArgs a) {
  const uint32_t n = a.p.n_objects;
  for (uint64_t p = uint64_t(blockIdx.x) * 256u + threadIdx.x; p < a.p.n_rows; p += uint64_t(gridDim.x) * 256u) {
    const uint32_t c = uint32_t(p / n);  // (every configuration has n keys: position p is one of configuration p / n)
    const uint32_t i = a.vals[1][p];
    const uint32_t axis = a.axis < 3u ? a.axis : a.conf_axis[c];
    double raw[6], grown[6];
    for (int k = 0; k < 6; ++k) raw[k] = a.p.boxes[6u * (uint64_t(c) * n + i) + k];
    pairs_grow(raw, a.p.inflate, grown);
    for (int k = 0; k < 6; ++k) a.sorted_boxes[6u * p + k] = grown[k];
    if (a.p.group) a.sorted_group[p] = a.p.group[i];
    a.ends[p] = psort_upper_bound(a.keys[1] + uint64_t(c) * n, n, psort_end(grown[3u + axis]));
  }
}

// ---- the sweep over the windows ---------------------------------------------------------------------------------------------------------
template <bool EMIT, bool GROUPS>
__global__ void __launch_bounds__(256) k_psort_sweep(PairsSortedArgs a) {
  __shared__ double tile[6][PAIRS_TILE];
  __shared__ uint32_t tile_id[PAIRS_TILE];
  __shared__ uint8_t tile_group[GROUPS ? PAIRS_TILE : 1u];
  __shared__ uint64_t collides[GROUPS ? PAIRS_MAX_GROUPS : 1u];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t n = a.p.n_objects;
  const uint32_t c = blockIdx.x / a.blocks_per_conf;
  const uint32_t i0 = (blockIdx.x - c * a.blocks_per_conf) * PAIRS_ROWS;
  const uint32_t i1 = n - i0 > PAIRS_ROWS ? i0 + PAIRS_ROWS : n;
  const uint64_t first = uint64_t(c) * n;  // the configuration's first position in the chunk
  const double* __restrict__ boxes = a.sorted_boxes + 6u * first;
  const uint32_t* __restrict__ ids = a.vals[1] + first;
  const uint32_t* __restrict__ ends = a.ends + first;

  // the joint window's end: one value for the workgroup -- it decides how many tiles go through the barriers below
  uint32_t block_end = 0;
  for (uint32_t i = i0; i < i1; ++i) block_end = ends[i] > block_end ? ends[i] : block_end;
  block_end = uint32_t(__builtin_amdgcn_readfirstlane(int(block_end)));
  if (GROUPS) {
    if (threadIdx.x < PAIRS_MAX_GROUPS) collides[threadIdx.x] = a.p.collides[threadIdx.x];
    __syncthreads();
  }

  // the wave's rows: sorted positions i0 + wave * PAIRS_WAVE_ROWS + r (past i1: no row -- a window end of 0 refuses every column)
  double row_box[PAIRS_WAVE_ROWS][6];
  uint32_t row_i[PAIRS_WAVE_ROWS], row_end[PAIRS_WAVE_ROWS], row_id[PAIRS_WAVE_ROWS], row_group[PAIRS_WAVE_ROWS], count[PAIRS_WAVE_ROWS];
  uint64_t pos[PAIRS_WAVE_ROWS];
  uint32_t wave_end = 0;
  for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
    const uint32_t i = i0 + wave * PAIRS_WAVE_ROWS + r;
    const bool there = i < i1;
    const uint32_t at = there ? i : i0;
    row_i[r] = there ? i : n;
    row_end[r] = there ? ends[at] : 0u;
    row_id[r] = ids[at];
    row_group[r] = GROUPS ? a.sorted_group[first + at] : 0u;
    count[r] = 0u;
    for (int k = 0; k < 6; ++k) row_box[r][k] = boxes[6u * size_t(at) + k];
    pos[r] = EMIT && there ? a.p.row_offsets[first + at] - a.emit_base : 0u;
    wave_end = row_end[r] > wave_end ? row_end[r] : wave_end;
  }
  const uint32_t wave_first = i0 + wave * PAIRS_WAVE_ROWS + 1u;  // the first column any of the wave's rows looks at

  const double2* __restrict__ vec = reinterpret_cast<const double2*>(boxes);  // (a box: 48 B, three vectors; 48 * first is a multiple of 16)
  for (uint32_t base = pairs_first_tile(i0); base < block_end; base += PAIRS_TILE) {
    __syncthreads();  // (the tile before has been read)
    for (uint32_t v = threadIdx.x; v < 3u * PAIRS_TILE; v += 256u) {
      const uint32_t col = v / 3u, part = v - 3u * col;
      if (base + col < n) {
        const double2 x = vec[3u * size_t(base) + v];
        tile[2u * part][col] = x.x;
        tile[2u * part + 1u][col] = x.y;
      }
    }
    for (uint32_t col = threadIdx.x; col < PAIRS_TILE; col += 256u)
      if (base + col < n) {
        tile_id[col] = ids[base + col];
        if (GROUPS) tile_group[col] = a.sorted_group[first + base + col];
      }
    __syncthreads();
    for (uint32_t step = 0; step < PAIRS_TILE; step += 64u) {
      if (base + step >= wave_end || base + step + 64u <= wave_first) continue;  // (the same in the whole wave; no barrier in here)
      const uint32_t j = base + step + lane;
      double col_box[6];
      for (int k = 0; k < 6; ++k) col_box[k] = tile[k][step + lane];  // (columns past n: stale values, refused by j < row_end <= n)
      const uint32_t col_id = tile_id[step + lane];
      const uint32_t col_group = GROUPS ? tile_group[step + lane] : 0u;
      for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r) {
        const bool keep = j > row_i[r] && j < row_end[r] && cull_boxes_touch(row_box[r], col_box) &&
                          (!GROUPS || psort_allowed(row_id[r], row_group[r], col_id, col_group, collides));
        const uint64_t ballot = __ballot(keep);
        if (EMIT && ballot != 0u) {
          const uint64_t e = pos[r] + count[r] + cull_rank(ballot, lane);
          if (keep && e < a.n_emit) a.emit[0][e] = psort_pair_word(c, row_id[r], col_id, a.obj_bits);
        }
        count[r] += cull_popcount(ballot);
      }
    }
  }
  if (!EMIT && lane == 0u)
    for (uint32_t r = 0; r < PAIRS_WAVE_ROWS; ++r)
      if (row_i[r] < n) a.p.row_counts[first + row_i[r]] = count[r];
}

// the sorted words of a chunk into the caller's list
__global__ void __launch_bounds__(256) k_psort_write(PairsSortedArgs a) {
  for (uint64_t e = uint64_t(blockIdx.x) * 256u + threadIdx.x; e < a.n_emit; e += uint64_t(gridDim.x) * 256u) {
    const uint64_t at = a.emit_base + e;
    if (at >= a.p.capacity) continue;
    uint32_t i, j;
    psort_pair_of(a.emit[1][e], a.obj_bits, i, j);
    reinterpret_cast<uint2*>(a.p.pairs)[at] = make_uint2(i, j);
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------
static uint32_t psort_grid(uint64_t work) { return uint32_t(std::min<uint64_t>((work + 255u) / 256u, 65536u)); }

hipError_t pairs_sorted_temp_bytes(const PairsSortedArgs& a, bool emit, size_t& bytes) {
  bytes = 0;
  uint64_t* k = nullptr;
  uint32_t* v = nullptr;
  if (emit) return rocprim::radix_sort_keys(nullptr, bytes, k, k, size_t(a.n_emit), 0u, a.conf_bits + 2u * a.obj_bits);
  return rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, size_t(a.p.n_rows), 0u, 32u + a.conf_bits);
}

hipError_t launch_pairs_sorted_count(hipStream_t st, const PairsSortedArgs& a) {
  if (a.axis >= 3u) {
    hipLaunchKernelGGL(k_psort_spread, dim3(a.spread_blocks * a.n_conf_chunk), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_psort_axis, dim3((a.n_conf_chunk + 3u) / 4u), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_psort_keys, dim3(psort_grid(a.p.n_rows)), dim3(256), 0, st, a);
  size_t bytes = a.temp_bytes;
  const hipError_t e = rocprim::radix_sort_pairs(a.temp, bytes, a.keys[0], a.keys[1], a.vals[0], a.vals[1], size_t(a.p.n_rows), 0u, 32u + a.conf_bits, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_psort_gather, dim3(psort_grid(a.p.n_rows)), dim3(256), 0, st, a);
  const dim3 grid(a.n_conf_chunk * a.blocks_per_conf);
  if (a.p.group)
    hipLaunchKernelGGL((k_psort_sweep<false, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_psort_sweep<false, false>), grid, dim3(256), 0, st, a);
  launch_pairs_scan(st, a.p);
  return hipSuccess;
}

hipError_t launch_pairs_sorted_emit(hipStream_t st, const PairsSortedArgs& a) {
  const dim3 grid(a.n_conf_chunk * a.blocks_per_conf);
  if (a.p.group)
    hipLaunchKernelGGL((k_psort_sweep<true, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_psort_sweep<true, false>), grid, dim3(256), 0, st, a);
  size_t bytes = a.temp_bytes;
  const hipError_t e = rocprim::radix_sort_keys(a.temp, bytes, a.emit[0], a.emit[1], size_t(a.n_emit), 0u, a.conf_bits + 2u * a.obj_bits, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_psort_write, dim3(psort_grid(a.n_emit)), dim3(256), 0, st, a);
  return hipSuccess;
}
