// egm_route.h — host-callable launchers for the kernels of egm_route.hip: the
// forward pass over the route-node table and the node drop.  Device pointers
// unless stated.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace egm {

constexpr uint32_t ROUTE_MAX_NODES = 64;   // EGM_ROUTE_MAX_NODES: one bit of a filter's mask per node
constexpr uint32_t FWD_TILE = 64;          // match rows per wave

struct RouteTable {
  const uint64_t* masks;   // [n_fid_slots] bit n: a route {filter, node n}
  uint32_t n_fid_slots;    // a filter id at or past it has mask 0
  uint32_t self_node;
  uint32_t n_nodes;        // largest node id ever set + 1
};

inline uint64_t fwd_tiles(uint32_t n_topics) { return ((uint64_t)n_topics + FWD_TILE - 1) / FWD_TILE; }

// The forward pass (k_fwd_count, the scan of its node-major tile counts,
// k_fwd_fill).  Scratch: tile_cnt u32[n_nodes * tiles + 1], tile_base
// u64[n_nodes * tiles + 1], tile_sums u64[scan_tiles(n_nodes * tiles) + 2],
// state u64[2] = {total, overflow}.  node_row receives ROUTE_MAX_NODES + 1
// entries.  ev (optional) brackets the pass.
hipError_t launch_forward(const RouteTable& rt, const uint64_t* match_row, const uint32_t* match_ids, uint32_t n,
                          uint64_t nids, uint64_t* node_row, uint32_t* fwd_topic, uint32_t* fwd_fid, uint64_t fwd_cap,
                          uint32_t* entry_fwd, uint32_t* topic_fwd, uint32_t* tile_cnt, uint64_t* tile_base,
                          uint64_t* tile_sums, uint64_t* state, hipStream_t s, hipEvent_t* ev);

// cleanup_routes/1 over one copy of the masks: clears bit `node` everywhere;
// a filter id whose mask went from non-zero to zero is appended to out
// (out_cap entries; null: not collected), *n_out = how many.
hipError_t launch_route_drop(uint64_t* masks, uint32_t n_fid_slots, uint32_t node, uint32_t* out, uint32_t out_cap,
                             uint32_t* n_out, hipStream_t s);

}  // namespace egm
