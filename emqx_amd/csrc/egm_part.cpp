// egm_part.cpp — tables split over several GPUs, and the host-only image:
// the merge of per-shard results (egm_shard_merge), the filter and topic
// assignment of the shard and prefix partitions (egm_shard_assign,
// egm_prefix_*), and egm_image_* (a HostTable without a device).
#include "egm_ctx.h"

using namespace egm;

static constexpr uint32_t PREFIX_RANKS_MAX = 16;   // ranks of one prefix partition (kernel limit)

extern "C" {

int egm_shard_merge(egm_ctx* c, uint32_t n_shards, uint32_t n, const uint32_t* d_counts,
                    const uint32_t* const* d_shard_ids, uint64_t total_ids, void* hip_stream, uint64_t* d_row,
                    uint32_t* d_ids, uint64_t ids_cap) {
  if (!c || n_shards == 0 || n_shards > MAX_SHARDS || !d_counts || !d_shard_ids || !d_row) return EGM_E_INVAL;
  if (total_ids > ids_cap || (total_ids && !d_ids)) return EGM_E_OVERFLOW;
  for (uint32_t g = 0; g < n_shards; ++g)
    if (!d_shard_ids[g] && total_ids) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = (hipStream_t)hip_stream;   // NULL: the HIP default (null) stream, as the caller's own work
  hipError_t e;
  const uint64_t nn = (uint64_t)n + 1;
  if ((e = c->part.m_srow.ensure(nn * n_shards * 8)) != hipSuccess) return c->hip_fail(e, "merge srow");
  if ((e = c->part.m_tiles.ensure((scan_tiles(n) + 2) * 8)) != hipSuccess) return c->hip_fail(e, "merge tiles");
  if ((e = c->part.m_tot.ensure(nn * 4)) != hipSuccess) return c->hip_fail(e, "merge tot");
  ShardIds src{};
  for (uint32_t k = 0; k < n_shards; ++k) src.ids[k] = d_shard_ids[k];
  c->work_begin(s);
  e = launch_shard_merge(d_counts, n_shards, n, src, c->part.m_srow.as<uint64_t>(),
                         c->part.m_tiles.as<uint64_t>(), c->part.m_tot.as<uint32_t>(), d_row, d_ids, ids_cap, s);
  c->work_end(s);
  if (e != hipSuccess) return c->hip_fail(e, "launch_shard_merge");
  return EGM_OK;
}

// ---------------------------------------------------- host-only image API --
struct egm_image {
  HostTable t;
  DirtyLog d;   // the log egm_image_take_dirty last handed out
};

egm_image* egm_image_new(void) { return new (std::nothrow) egm_image(); }
void egm_image_free(egm_image* im) { delete im; }
int egm_image_insert(egm_image* im, const uint8_t* f, uint32_t len, uint32_t id) {
  if (!im || (!f && len)) return EGM_E_INVAL;
  return im->t.insert(f, len, id, nullptr);
}
int egm_image_remove(egm_image* im, const uint8_t* f, uint32_t len) {
  if (!im || (!f && len)) return EGM_E_INVAL;
  return im->t.remove(f, len);
}
void egm_image_relayout(egm_image* im) {
  if (im) im->t.relayout();
}
int egm_image_build(egm_image* im, const uint8_t* blob, const uint32_t* off, uint32_t n, const uint32_t* ids,
                    uint32_t threads) {
  if (!im || (n && (!blob || !valid_offsets(off, n)))) return EGM_E_INVAL;
  std::string why;
  if (!validate_inserts(im->t, blob, off, n, ids, true, &why)) return EGM_E_INVAL;
  if (ids)
    for (uint32_t i = 0; i < n; ++i)
      if (ids[i] == NONE) return EGM_E_INVAL;
  return im->t.bulk_build(blob, off, n, ids, threads) < 0 ? EGM_E_INVAL : EGM_OK;
}
int egm_image_take_dirty(egm_image* im, egm_dirty_view* v) {
  if (!im || !v) return EGM_E_INVAL;
  im->d = im->t.take_dirty();
  sort_unique(im->d.nodes, im->t.nodes.size());
  sort_unique(im->d.edges, im->t.edges.size());
  sort_unique(im->d.dict, im->t.dict.size());
  v->nodes = im->d.nodes.data();
  v->n_nodes = im->d.nodes.size();
  v->edges = im->d.edges.data();
  v->n_edges = im->d.edges.size();
  v->dict = im->d.dict.data();
  v->n_dict = im->d.dict.size();
  v->nodes_full = im->d.nodes_full;
  v->edges_full = im->d.edges_full;
  v->dict_full = im->d.dict_full;
  v->words_full = im->d.words_full;
  return EGM_OK;
}
int egm_image_get_view(egm_image* im, egm_image_view* v) {
  if (!im || !v) return EGM_E_INVAL;
  const HostTable& t = im->t;
  v->nodes = t.nodes.data();
  v->n_nodes = t.nodes.size();
  v->hash_child = t.hash_child.data();
  v->edges = t.edges.data();
  v->n_edge_slots = t.edges.size();
  v->edge_mask = t.edge_mask();
  v->dict = t.dict.data();
  v->n_dict_slots = t.dict.size();
  v->dict_mask = t.dict_mask();
  v->dict_blob = t.dict_blob.data();
  v->dict_off = t.dict_off.data();
  v->n_words = t.n_words();
  v->n_filters = t.n_filters();
  v->n_live_nodes = t.n_nodes_live();
  v->n_edges = t.n_edges();
  return EGM_OK;
}
int egm_shard_assign(const uint8_t* blob, const uint32_t* off, uint32_t n, uint32_t g, uint32_t* out) {
  if (!off || !out || g == 0 || (n && !blob)) return EGM_E_INVAL;
  for (uint32_t i = 0; i < n; ++i) out[i] = filter_shard(blob + off[i], off[i + 1] - off[i], g);
  return EGM_OK;
}
// ---- prefix partition ----
int egm_prefix_assign(const uint8_t* blob, const uint32_t* off, uint32_t n, uint32_t n_vparts, uint32_t n_ranks,
                      uint8_t* vpart_rank, uint32_t* filter_rank) {
  if (!off || !vpart_rank || !filter_rank || n_vparts == 0 || n_ranks == 0 || n_ranks > PREFIX_RANKS_MAX ||
      (n && !blob))
    return EGM_E_INVAL;
  std::vector<uint64_t> load(n_vparts, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* p = blob + off[i];
    const uint32_t len = off[i + 1] - off[i];
    if (prefix_replicated(p, len)) {
      filter_rank[i] = EGM_PREFIX_ALL;
    } else {
      const uint32_t v = prefix_vpart(p, len, n_vparts);
      filter_rank[i] = v;   // the vpart for now, its rank below
      load[v] += 1;
    }
  }
  // greedy: the heaviest virtual partitions first, each to the least loaded
  // rank (ties: the lower vpart, the lower rank) — deterministic on every rank
  std::vector<uint32_t> order(n_vparts);
  for (uint32_t v = 0; v < n_vparts; ++v) order[v] = v;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return load[a] > load[b]; });
  std::vector<uint64_t> rl(n_ranks, 0);
  for (uint32_t v : order) {
    uint32_t best = 0;
    for (uint32_t k = 1; k < n_ranks; ++k)
      if (rl[k] < rl[best]) best = k;
    vpart_rank[v] = (uint8_t)best;
    rl[best] += load[v];
  }
  for (uint32_t i = 0; i < n; ++i)
    if (filter_rank[i] != EGM_PREFIX_ALL) filter_rank[i] = vpart_rank[filter_rank[i]];
  return EGM_OK;
}

uint64_t egm_prefix_slot_bytes(uint32_t n_ranks, uint32_t cap_topics, uint64_t cap_bytes) {
  const PrefixSlots ps{n_ranks, cap_topics, cap_bytes};
  return ps.slot_bytes();
}

int egm_prefix_route(egm_ctx* c, const uint8_t* d_blob, const uint32_t* d_off, uint32_t n, const uint8_t* d_vpart_rank,
                     uint32_t n_vparts, uint32_t n_ranks, uint32_t cap_topics, uint64_t cap_bytes, void* hip_stream,
                     uint8_t* d_send) {
  if (!c || !d_vpart_rank || !d_send || n_vparts == 0 || n_ranks == 0 || n_ranks > PREFIX_RANKS_MAX ||
      (n && (!d_blob || !d_off)) || cap_bytes >= (1ull << 32) || n >= PFX_TOPICS_MAX || cap_topics >= PFX_TOPICS_MAX)
    return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = (hipStream_t)hip_stream;   // NULL: the HIP default (null) stream, as the caller's own work
  hipError_t e;
  if ((e = c->part.p_ctr.ensure(2 * 8 * PREFIX_RANKS_MAX)) != hipSuccess) return c->hip_fail(e, "prefix counters");
  if ((e = c->part.p_dst.ensure(8ull * std::max<uint32_t>(n, 1))) != hipSuccess) return c->hip_fail(e, "prefix routes");
  c->work_begin(s);
  const PrefixSlots ps{n_ranks, cap_topics, cap_bytes};
  e = launch_prefix_route(d_blob, d_off, n, d_vpart_rank, n_vparts, ps, d_send, c->part.p_ctr.as<unsigned long long>(),
                          c->part.p_dst.as<uint64_t>(), s);
  c->work_end(s);
  return e == hipSuccess ? EGM_OK : c->hip_fail(e, "launch_prefix_route");
}

}  // extern "C"
