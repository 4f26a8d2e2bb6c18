// egm_route.hip — cluster routes on the device (egm_route.h): the forward
// pass of emqx_broker:do_route/2's third arm (apps/emqx/src/emqx_broker.erl:
// 242-247, 262-280) over the route-node table, and cleanup_routes/1's node
// drop (emqx_router_helper.erl:137-146).  gfx950, wave64.
//
// The forward pass turns a match CSR into one list of (row, filter) pairs per
// remote node.  A wave owns a tile of 64 consecutive match rows, whose entries
// are the contiguous range [row[t0], row[t0 + 64]):
//   k_fwd_count  per (node, tile) the forwards, node-major; per entry its remote
//                nodes (bit 31: a local route); per row its forwards
//   scan         one exclusive scan of the tile counts: every (node, tile) base
//   k_fwd_fill   the same tiling again: per 64 entries and per node present in
//                them, one contiguous run of pairs at base + running count + rank
// The lane n of a wave keeps node n's count (running base) in a register, so
// no counter is indexed dynamically; an entry's row comes from a 6-step search
// over the tile's 65 row values in LDS (k_fan_fill's method).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "egm_kernels.h"
#include "egm_route.h"

namespace egm {

// the scan of egm_kernels.hip (counts u32[n] -> row_ptr u64[n + 1], exclusive)
__global__ void k_scan_reduce(const uint32_t* __restrict__ cnt, uint32_t n, uint64_t* __restrict__ tile_sums);
__global__ void k_scan_top(uint64_t* __restrict__ tile_sums, uint32_t ntiles);
__global__ void k_scan_apply(const uint32_t* __restrict__ cnt, uint32_t n, const uint64_t* __restrict__ tile_sums,
                             uint32_t ntiles, uint64_t* __restrict__ row_ptr, uint64_t* __restrict__ copy);
__global__ void k_scan_small(const uint32_t* __restrict__ cnt, uint32_t n, uint64_t* __restrict__ row_ptr,
                             uint64_t* __restrict__ copy);
constexpr uint32_t FWD_SCAN_SMALL = 65536;   // one launch up to here (k_scan_small takes any n)

constexpr int FWD_WAVES = 4;     // waves (tiles) per block
constexpr int FWD_UNROLL = 4;    // mask reads per lane in flight

struct FwdTile {
  uint64_t e0, e1;   // the tile's entries
  uint32_t t0, nr;   // first row, rows (0: no tile for this wave)
};

// rowv[0 .. nr] = the tile's row values clamped to nids, the rest padding that
// no entry reaches.  Every wave of the block comes here (one barrier).
__device__ __forceinline__ FwdTile fwd_tile(const uint64_t* __restrict__ row, uint32_t n, uint64_t nids, uint64_t tile,
                                            uint64_t n_tiles, uint64_t* rowv, uint32_t lane) {
  FwdTile T{0, 0, 0, 0};
  if (tile < n_tiles) {
    T.t0 = (uint32_t)(tile * FWD_TILE);
    T.nr = n - T.t0 < FWD_TILE ? n - T.t0 : FWD_TILE;
  }
  uint64_t v = ~0ull;
  if (T.nr && lane <= T.nr) {
    v = row[(uint64_t)T.t0 + lane];
    if (v > nids) v = nids;
  }
  rowv[lane] = v;
  if (lane == 0) {
    uint64_t last = ~0ull;
    if (T.nr == FWD_TILE) {
      last = row[(uint64_t)T.t0 + FWD_TILE];
      if (last > nids) last = nids;
    }
    rowv[FWD_TILE] = last;
  }
  __syncthreads();
  if (T.nr) {
    T.e0 = rowv[0];
    T.e1 = rowv[T.nr];
    if (T.e1 < T.e0) T.e1 = T.e0;
  }
  return T;
}

// The row of entry e inside the tile: the last r with rowv[r] <= e (empty rows
// share a value; the padding past the tile's end is never <= e).  r + step
// stays below 64.
__device__ __forceinline__ uint32_t fwd_row_of(const uint64_t* rowv, uint64_t e) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t step = 32; step >= 1; step >>= 1)
    if (rowv[r + step] <= e) r += step;
  return r;
}

// The OR of v over the wave, as a scalar (the loops over its bits are wave-uniform).
__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ uint64_t fwd_remote(const RouteTable& rt, uint64_t m) {
  const uint64_t nodes = rt.n_nodes >= 64 ? ~0ull : (1ull << rt.n_nodes) - 1;
  return m & nodes & ~(1ull << rt.self_node);
}

__global__ __launch_bounds__(64 * FWD_WAVES) void k_fwd_count(RouteTable rt, const uint64_t* __restrict__ row,
                                                              const uint32_t* __restrict__ ids, uint32_t n,
                                                              uint64_t nids, uint64_t n_tiles,
                                                              uint32_t* __restrict__ tile_cnt,
                                                              uint32_t* __restrict__ entry_fwd,
                                                              uint32_t* __restrict__ topic_fwd) {
  __shared__ uint64_t rowv_s[FWD_WAVES][FWD_TILE + 1];
  __shared__ uint32_t cnt_s[FWD_WAVES][FWD_TILE];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t tile = (uint64_t)blockIdx.x * FWD_WAVES + wv;
  uint64_t* rowv = rowv_s[wv];
  uint32_t* cnt = cnt_s[wv];
  cnt[lane] = 0;
  const FwdTile T = fwd_tile(row, n, nids, tile, n_tiles, rowv, lane);
  uint32_t mine = 0;   // lane k: the tile's forwards to node k
  for (uint64_t b = T.e0; b < T.e1; b += 64 * FWD_UNROLL) {   // wave-uniform trip count
    uint32_t fid[FWD_UNROLL];
    uint64_t m[FWD_UNROLL];
#pragma unroll
    for (int k = 0; k < FWD_UNROLL; ++k) {
      const uint64_t e = b + 64 * k + lane;
      fid[k] = e < T.e1 ? ids[e] : NONE;
    }
#pragma unroll
    for (int k = 0; k < FWD_UNROLL; ++k) m[k] = fid[k] < rt.n_fid_slots ? rt.masks[fid[k]] : 0ull;
#pragma unroll
    for (int k = 0; k < FWD_UNROLL; ++k) {
      const uint64_t e = b + 64 * k + lane;
      const uint64_t remote = fwd_remote(rt, m[k]);
      const uint32_t c = (uint32_t)__popcll(remote);
      if (e < T.e1) {
        if (entry_fwd) entry_fwd[e] = c | ((m[k] >> rt.self_node) & 1ull ? 0x80000000u : 0u);
        if (topic_fwd && c) atomicAdd(&cnt[fwd_row_of(rowv, e)], c);
      }
      if (!__ballot(c != 0)) continue;
      uint64_t any = wave_or(remote);
      while (any) {
        const uint32_t node = (uint32_t)__builtin_ctzll(any);
        any &= any - 1;
        const uint32_t k_node = (uint32_t)__popcll(__ballot((remote >> node) & 1ull));
        if (lane == node) mine += k_node;
      }
    }
  }
  if (T.nr && lane < rt.n_nodes) tile_cnt[(uint64_t)lane * n_tiles + tile] = mine;
  __syncthreads();
  if (topic_fwd && lane < T.nr) topic_fwd[(uint64_t)T.t0 + lane] = cnt[lane];
}

// node_row[k] = the first forward of node k (nodes past the table's: the
// total); state = {total, total > cap}.
__global__ __launch_bounds__(128) void k_fwd_rows(const uint64_t* __restrict__ tile_base, uint32_t n_nodes,
                                                  uint64_t n_tiles, uint64_t cap, uint64_t* __restrict__ node_row,
                                                  uint64_t* __restrict__ state) {
  const uint32_t k = threadIdx.x;
  const uint64_t total = tile_base[(uint64_t)n_nodes * n_tiles];
  if (k <= ROUTE_MAX_NODES) node_row[k] = k < n_nodes ? tile_base[(uint64_t)k * n_tiles] : total;
  if (k == 0) {
    state[0] = total;
    state[1] = total > cap ? 1 : 0;
  }
}

__global__ __launch_bounds__(64 * FWD_WAVES) void k_fwd_fill(RouteTable rt, const uint64_t* __restrict__ row,
                                                             const uint32_t* __restrict__ ids, uint32_t n,
                                                             uint64_t nids, uint64_t n_tiles,
                                                             const uint64_t* __restrict__ tile_base,
                                                             const uint64_t* __restrict__ state,
                                                             uint32_t* __restrict__ fwd_topic,
                                                             uint32_t* __restrict__ fwd_fid) {
  __shared__ uint64_t rowv_s[FWD_WAVES][FWD_TILE + 1];
  if (state[1]) return;   // the lists are too small: nothing is written (the whole grid returns)
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t tile = (uint64_t)blockIdx.x * FWD_WAVES + wv;
  uint64_t* rowv = rowv_s[wv];
  const FwdTile T = fwd_tile(row, n, nids, tile, n_tiles, rowv, lane);
  // lane k: where node k's next pair of this tile goes
  uint64_t run = (T.nr && lane < rt.n_nodes) ? tile_base[(uint64_t)lane * n_tiles + tile] : 0;
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t b = T.e0; b < T.e1; b += 64 * FWD_UNROLL) {   // wave-uniform trip count
    uint32_t fid[FWD_UNROLL];
    uint64_t m[FWD_UNROLL];
#pragma unroll
    for (int k = 0; k < FWD_UNROLL; ++k) {
      const uint64_t e = b + 64 * k + lane;
      fid[k] = e < T.e1 ? ids[e] : NONE;
    }
#pragma unroll
    for (int k = 0; k < FWD_UNROLL; ++k) m[k] = fid[k] < rt.n_fid_slots ? rt.masks[fid[k]] : 0ull;
#pragma unroll
    for (int k = 0; k < FWD_UNROLL; ++k) {
      const uint64_t remote = fwd_remote(rt, m[k]);
      if (!__ballot(remote != 0)) continue;
      const uint32_t topic = T.t0 + (remote ? fwd_row_of(rowv, b + 64 * k + lane) : 0u);
      uint64_t any = wave_or(remote);
      while (any) {
        const uint32_t node = (uint32_t)__builtin_ctzll(any);
        any &= any - 1;
        const bool on = (remote >> node) & 1ull;
        const uint64_t bal = __ballot(on);
        const uint64_t at = __shfl(run, (int)node, 64);
        if (on) {   // one contiguous run of pairs per node
          const uint64_t dst = at + (uint32_t)__popcll(bal & below);
          fwd_topic[dst] = topic;
          fwd_fid[dst] = fid[k];
        }
        if (lane == node) run += (uint32_t)__popcll(bal);
      }
    }
  }
}

// cleanup_routes/1 (emqx_router_helper.erl:137-146, 175-179), atom dests: one
// streaming pass clears the node's bit; the filter ids whose mask went from
// non-zero to zero are appended wave-aggregated (as k_rs_expire appends its
// ranks).
__global__ __launch_bounds__(256) void k_route_drop(uint64_t* __restrict__ masks, uint32_t n_slots, uint64_t bit,
                                                    uint32_t* __restrict__ out, uint32_t out_cap,
                                                    uint32_t* __restrict__ n_out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t n_iter = (n_slots + stride - 1) / stride;   // uniform trip count: the wave ballots
  for (uint64_t it = 0; it < n_iter; ++it) {
    const uint64_t f = it * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool on = false;
    if (f < n_slots) {
      const uint64_t m = masks[f];
      if (m & bit) {
        masks[f] = m & ~bit;
        on = out && (m & ~bit) == 0;
      }
    }
    const uint64_t b = __ballot(on);
    if (!b) continue;
    const uint32_t leader = (uint32_t)__builtin_ctzll(b);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(n_out, (uint32_t)__popcll(b));
    base = __shfl(base, (int)leader, 64);
    if (on) {
      const uint32_t at = base + (uint32_t)__popcll(b & ((1ull << lane) - 1));
      if (at < out_cap) out[at] = (uint32_t)f;
    }
  }
}

static void fwd_scan(const uint32_t* cnt, uint32_t n, uint64_t* tile_sums, uint64_t* out, hipStream_t s) {
  if (n <= FWD_SCAN_SMALL) {
    hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, s, cnt, n, out, (uint64_t*)nullptr);
    return;
  }
  const uint32_t ntiles = (uint32_t)scan_tiles(n);
  hipLaunchKernelGGL(k_scan_reduce, dim3(ntiles), dim3(256), 0, s, cnt, n, tile_sums);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, s, tile_sums, ntiles);
  hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(256), 0, s, cnt, n, (const uint64_t*)tile_sums, ntiles, out,
                     (uint64_t*)nullptr);
}

hipError_t launch_forward(const RouteTable& rt, const uint64_t* match_row, const uint32_t* match_ids, uint32_t n,
                          uint64_t nids, uint64_t* node_row, uint32_t* fwd_topic, uint32_t* fwd_fid, uint64_t fwd_cap,
                          uint32_t* entry_fwd, uint32_t* topic_fwd, uint32_t* tile_cnt, uint64_t* tile_base,
                          uint64_t* tile_sums, uint64_t* state, hipStream_t s, hipEvent_t* ev) {
  const uint64_t n_tiles = fwd_tiles(n);
  const uint32_t blocks = (uint32_t)((n_tiles + FWD_WAVES - 1) / FWD_WAVES);
  if (ev) hipEventRecord(ev[0], s);
  if (blocks)
    hipLaunchKernelGGL(k_fwd_count, dim3(blocks), dim3(64 * FWD_WAVES), 0, s, rt, match_row, match_ids, n, nids,
                       n_tiles, tile_cnt, entry_fwd, topic_fwd);
  fwd_scan(tile_cnt, (uint32_t)(rt.n_nodes * n_tiles), tile_sums, tile_base, s);
  hipLaunchKernelGGL(k_fwd_rows, dim3(1), dim3(128), 0, s, (const uint64_t*)tile_base, rt.n_nodes, n_tiles, fwd_cap,
                     node_row, state);
  if (blocks && rt.n_nodes)
    hipLaunchKernelGGL(k_fwd_fill, dim3(blocks), dim3(64 * FWD_WAVES), 0, s, rt, match_row, match_ids, n, nids,
                       n_tiles, (const uint64_t*)tile_base, (const uint64_t*)state, fwd_topic, fwd_fid);
  if (ev) hipEventRecord(ev[1], s);
  return hipGetLastError();
}

hipError_t launch_route_drop(uint64_t* masks, uint32_t n_fid_slots, uint32_t node, uint32_t* out, uint32_t out_cap,
                             uint32_t* n_out, hipStream_t s) {
  if (!n_fid_slots) return hipSuccess;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_fid_slots + 255) / 256, 8192);
  hipLaunchKernelGGL(k_route_drop, dim3(blocks), dim3(256), 0, s, masks, n_fid_slots, 1ull << node, out, out_cap,
                     n_out);
  return hipGetLastError();
}

}  // namespace egm
