// egm_route.cpp — cluster routes on the device: the route-node table
// (egm_routes_*: the host mirror and the two device copies a commit
// alternates between) and the forward pass over a match CSR
// (egm_forward_*, egm_last_forward; kernels in egm_route.hip).
#include <unordered_set>

#include "egm_ctx.h"

using namespace egm;

// New filter ids a delta may introduce past the table's slots and the match
// table's own id range (egm_subs_apply_delta's bound, with the match table in).
static constexpr uint64_t ROUTE_FID_GROWTH = 1ull << 22;

static uint32_t mask_nodes(uint64_t m) { return m ? 64u - (uint32_t)__builtin_clzll(m) : 0u; }

// The whole mirror into both copies: egm_routes_build, and a commit whose new
// filter id lies past the slots.  Slots: the largest filter id with a route (or
// `least`) + a quarter + 4096 spare.
static int routes_upload(egm_ctx* c, uint64_t least) {
  RouteState& R = c->route;
  R.uses[0].drain();
  R.uses[1].drain();
  uint64_t hi = 0;
  for (uint64_t f = R.mask.size(); f > 0; --f)
    if (R.mask[f - 1]) {
      hi = f;
      break;
    }
  hi = std::max(hi, least);
  const uint32_t slots = (uint32_t)std::min<uint64_t>(WID_MAX, hi + hi / 4 + 4096);
  R.mask.resize(slots, 0ull);   // (what is cut off is zero)
  hipError_t e;
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "routes: stream");
  for (int k = 0; k < 2; ++k)
    if ((e = R.copy[k].ensure((size_t)slots * 8)) != hipSuccess) return c->hip_fail(e, "route masks");
  if ((e = hipMemcpy(R.copy[0].p, R.mask.data(), (size_t)slots * 8, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(R.copy[1].p, R.copy[0].p, (size_t)slots * 8, hipMemcpyDeviceToDevice)) != hipSuccess ||
      (e = hipDeviceSynchronize()) != hipSuccess)
    return c->hip_fail(e, "H2D route masks");
  R.n_fid_slots = slots;
  R.pending.clear();
  for (int k = 0; k < 2; ++k) {
    R.stale[k].clear();
    R.drops[k].clear();
  }
  R.cur = 0;
  R.built = true;
  R.epoch += 1;
  return EGM_OK;
}

static int routes_apply_delta(egm_ctx* c, const egm_route_pair* add, uint64_t n_add, const egm_route_pair* del,
                              uint64_t n_del) {
  RouteState& R = c->route;
  if (!R.built) return c->fail(EGM_E_STATE, "route table: egm_routes_build first");
  const uint64_t fid_limit =
      std::max<uint64_t>({R.n_fid_slots, R.mask.size(), c->table.next_fid()}) + ROUTE_FID_GROWTH;
  for (uint64_t i = 0; i < n_add; ++i) {
    if (add[i].node >= ROUTE_MAX_NODES) return c->fail(EGM_E_INVAL, "route delta: node id past EGM_ROUTE_MAX_NODES");
    if (add[i].fid >= WID_MAX || add[i].fid >= fid_limit)
      return c->fail(EGM_E_INVAL, "route delta: filter id out of range");
  }
  for (uint64_t i = 0; i < n_del; ++i)
    if (del[i].node >= ROUTE_MAX_NODES) return c->fail(EGM_E_INVAL, "route delta: node id past EGM_ROUTE_MAX_NODES");
  // net changes (egm_subs_apply_delta's contract): a pair in both lists is refused before anything is applied
  if (n_add && n_del) {
    std::unordered_set<uint64_t> adds;
    adds.reserve(n_add * 2);
    for (uint64_t i = 0; i < n_add; ++i) adds.insert((uint64_t)add[i].fid << 32 | add[i].node);
    for (uint64_t i = 0; i < n_del; ++i)
      if (adds.count((uint64_t)del[i].fid << 32 | del[i].node))
        return c->fail(EGM_E_INVAL, "route delta: a (filter, node) pair is both added and removed");
  }
  uint64_t hi = 0;
  for (uint64_t i = 0; i < n_add; ++i) hi = std::max<uint64_t>(hi, (uint64_t)add[i].fid + 1);
  if (hi > R.mask.size()) R.mask.resize(hi, 0ull);
  for (uint64_t i = 0; i < n_add; ++i) {   // do_add_route/2: a route is in the bag once (emqx_router.erl:114-125)
    const uint64_t bit = 1ull << add[i].node;
    if (R.mask[add[i].fid] & bit) continue;
    R.mask[add[i].fid] |= bit;
    R.n_nodes = std::max(R.n_nodes, add[i].node + 1);
    R.pending.push_back(add[i].fid);
  }
  for (uint64_t i = 0; i < n_del; ++i) {   // do_delete_route/2 (:164-170, 230-248)
    const uint64_t bit = 1ull << del[i].node;
    if (del[i].fid >= R.mask.size() || !(R.mask[del[i].fid] & bit)) continue;
    R.mask[del[i].fid] &= ~bit;
    R.pending.push_back(del[i].fid);
  }
  return EGM_OK;
}

// The commit; with drop >= 0 also cleanup_routes/1 of that node, whose emptied
// filter ids (sorted) go to *emptied.
static int routes_commit(egm_ctx* c, uint64_t* epoch, int drop, std::vector<uint32_t>* emptied) {
  RouteState& R = c->route;
  if (!R.built) return c->fail(EGM_E_STATE, "route table: egm_routes_build first");
  R.last_patched = 0;
  R.last_rebuilt = false;
  std::vector<uint32_t> P = R.pending;
  sort_unique(P);
  // a full upload instead of a patch: a filter id past the slots got a route
  bool rebuild = false;
  while (!P.empty() && P.back() >= R.n_fid_slots) {
    if (R.mask[P.back()]) rebuild = true;
    P.pop_back();   // (without a route it has mask 0 on the device as it is)
  }
  if (rebuild) {
    const int r = routes_upload(c, 0);
    if (r != EGM_OK) return r;
    R.last_rebuilt = true;
    P.clear();
    if (drop < 0) {
      if (epoch) *epoch = R.epoch;
      return EGM_OK;
    }
  }
  // the copy no reader uses: its last readers first, then the node drops and every mask it lacks
  const int x = 1 - R.cur;
  R.uses[x].drain();
  uint64_t* dst = R.copy[x].as<uint64_t>();
  std::vector<uint32_t> need = R.stale[x];
  need.insert(need.end(), P.begin(), P.end());
  sort_unique(need);
  hipError_t e;
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "routes commit: stream");
  for (uint32_t node : R.drops[x])
    if ((e = launch_route_drop(dst, R.n_fid_slots, node, nullptr, 0, nullptr, c->stream)) != hipSuccess)
      return c->hip_fail(e, "routes commit: node drop");
  if (!need.empty()) {
    const size_t o_val = (need.size() * 4 + 15) & ~(size_t)15, total = o_val + need.size() * 8;
    uint8_t* h = patch_stage(c, total);
    if (!h) return c->fail(EGM_E_NOMEM, "routes commit: pinned staging");
    memcpy(h, need.data(), need.size() * 4);
    for (size_t i = 0; i < need.size(); ++i) memcpy(h + o_val + 8 * i, &R.mask[need[i]], 8);
    if ((e = c->patch_dev.ensure(total)) != hipSuccess) return c->hip_fail(e, "routes commit: patch buffer");
    uint8_t* dp = (uint8_t*)c->patch_dev.p;
    if ((e = hipMemcpyAsync(dp, h, total, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = launch_patch(dst, 8, (const uint32_t*)dp, dp + o_val, need.size(), c->stream)) != hipSuccess)
      return c->hip_fail(e, "routes commit: patch");
  }
  if (drop >= 0) {
    // the host mirror in a plain loop; it says how many filters the device pass will report
    const uint64_t bit = 1ull << drop;
    uint64_t n_emp = 0;
    for (uint64_t& m : R.mask) {
      if (m == bit) ++n_emp;
      m &= ~bit;
    }
    unsigned int got = 0;
    emptied->assign(n_emp, 0u);
    if ((e = R.drop_out.ensure((n_emp + 1) * 4)) != hipSuccess || (e = R.drop_n.ensure(16)) != hipSuccess)
      return c->hip_fail(e, "routes drop: buffers");
    if ((e = hipMemsetAsync(R.drop_n.p, 0, 4, c->stream)) != hipSuccess ||
        (e = launch_route_drop(dst, R.n_fid_slots, (uint32_t)drop, R.drop_out.as<uint32_t>(), (uint32_t)n_emp,
                               R.drop_n.as<uint32_t>(), c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(&got, R.drop_n.p, 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (n_emp && (e = hipMemcpyAsync(emptied->data(), R.drop_out.p, n_emp * 4, hipMemcpyDeviceToHost, c->stream)) !=
                      hipSuccess) ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
      return c->hip_fail(e, "routes drop");
    if (got != n_emp) return c->fail(EGM_E_DEVICE, "routes drop: the device copy and the host mirror disagree (a bug)");
    std::sort(emptied->begin(), emptied->end());
  } else if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) {
    return c->hip_fail(e, "routes commit: sync");
  }
  R.stale[x].clear();
  R.drops[x].clear();
  R.stale[R.cur].insert(R.stale[R.cur].end(), P.begin(), P.end());   // the old copy now lacks this commit
  if (drop >= 0) R.drops[R.cur].push_back((uint32_t)drop);
  R.cur = x;
  R.pending.clear();
  R.epoch += 1;
  R.last_patched = need.size();
  if (epoch) *epoch = R.epoch;
  return EGM_OK;
}

// The forward pass of a device match CSR.
static int run_forward(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len, uint32_t n,
                       hipStream_t s, uint64_t* d_nrow, uint32_t* d_topic, uint32_t* d_fid, uint64_t cap,
                       uint32_t* d_efwd, uint32_t* d_tfwd, uint64_t* total) {
  RouteState& R = c->route;
  uint64_t nids = 0;
  hipError_t e = hipMemcpyAsync(&nids, d_mrow + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return c->hip_fail(e, "match_row readback");
  if (nids >= 0xFFFFFFF0ull) return c->fail(EGM_E_INVAL, "too many matched ids for one forward batch");
  if (nids > mids_len) return c->fail(EGM_E_OVERFLOW, "match row total exceeds the id buffer (overflowed match batch)");
  const uint64_t cells = (uint64_t)R.n_nodes * fwd_tiles(n);
  if (cells >= 0xFFFFFFF0ull) return c->fail(EGM_E_INVAL, "too many topics for one forward batch");
  if ((e = R.tile_cnt.ensure((cells + 1) * 4)) != hipSuccess) return c->hip_fail(e, "r_tile_cnt");
  if ((e = R.tile_base.ensure((cells + 1) * 8)) != hipSuccess) return c->hip_fail(e, "r_tile_base");
  if ((e = R.tile_sums.ensure((scan_tiles((uint32_t)cells) + 2) * 8)) != hipSuccess) return c->hip_fail(e, "r_tiles");
  if ((e = R.state.ensure(16)) != hipSuccess) return c->hip_fail(e, "r_state");
  const int k = R.cur;   // the current copy; a commit patches the other one
  const RouteTable rt{R.copy[k].as<uint64_t>(), R.n_fid_slots, R.self_node, R.n_nodes};
  hipEvent_t evs[2] = {nullptr, nullptr};
  hipEvent_t* evp = c->timing.take_pair(evs);
  c->work_begin(s);
  e = launch_forward(rt, d_mrow, d_mids, n, nids, d_nrow, d_topic, d_fid, cap, d_efwd, d_tfwd,
                     R.tile_cnt.as<uint32_t>(), R.tile_base.as<uint64_t>(), R.tile_sums.as<uint64_t>(),
                     R.state.as<uint64_t>(), s, evp);
  R.uses[k].note(s);   // a later commit must not patch this copy before the pass has read it
  c->timing.push_pair(c->timing.fwd, evp);
  c->work_end(s);
  R.last_stream = s;
  R.launched = true;
  if (e != hipSuccess) return c->hip_fail(e, "launch_forward");
  if (total) {
    uint64_t st[2] = {0, 0};
    if ((e = hipMemcpyAsync(st, R.state.p, 16, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
      return c->hip_fail(e, "forward readback");
    *total = st[0];
    if (st[1]) return EGM_E_OVERFLOW;
  }
  return EGM_OK;
}

extern "C" {

int egm_routes_build(egm_ctx* c, const uint64_t* masks, uint32_t n_fid_slots, uint32_t self_node) {
  if (!c || (n_fid_slots && !masks)) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (self_node >= ROUTE_MAX_NODES) return c->fail(EGM_E_INVAL, "route table: node id past EGM_ROUTE_MAX_NODES");
  if (n_fid_slots >= WID_MAX) return c->fail(EGM_E_INVAL, "route table: filter id out of range");
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "route build: host allocation", [&] {
    RouteState& R = c->route;
    R.mask.assign(masks, masks + n_fid_slots);
    R.self_node = self_node;
    R.n_nodes = 0;
    for (uint64_t m : R.mask) R.n_nodes = std::max(R.n_nodes, mask_nodes(m));
    return routes_upload(c, n_fid_slots);
  });
}

int egm_routes_apply_delta(egm_ctx* c, const egm_route_pair* add, uint64_t n_add, const egm_route_pair* del,
                           uint64_t n_del) {
  if (!c || (n_add && !add) || (n_del && !del)) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  return no_throw(c, "route delta: host allocation", [&] { return routes_apply_delta(c, add, n_add, del, n_del); });
}

int egm_routes_commit(egm_ctx* c, uint64_t* epoch) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "route commit: host allocation", [&] { return routes_commit(c, epoch, -1, nullptr); });
}

int egm_routes_last_commit(egm_ctx* c, uint64_t* patched, int* rebuilt) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (patched) *patched = c->route.last_patched;
  if (rebuilt) *rebuilt = c->route.last_rebuilt ? 1 : 0;
  return EGM_OK;
}

int egm_routes_drop_node(egm_ctx* c, uint32_t node, uint32_t** emptied_fids, uint64_t* n) {
  if (!c || !emptied_fids || !n) return EGM_E_INVAL;
  *emptied_fids = nullptr;
  *n = 0;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (node >= ROUTE_MAX_NODES) return c->fail(EGM_E_INVAL, "routes drop: node id past EGM_ROUTE_MAX_NODES");
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "routes drop: host allocation", [&] {
    std::vector<uint32_t> emptied;
    const int r = routes_commit(c, nullptr, (int)node, &emptied);
    if (r != EGM_OK || emptied.empty()) return r;
    uint32_t* out = (uint32_t*)result_alloc(emptied.size() * 4);
    if (!out) return c->fail(EGM_E_NOMEM, "routes drop: result");
    memcpy(out, emptied.data(), emptied.size() * 4);
    *emptied_fids = out;
    *n = emptied.size();
    return (int)EGM_OK;
  });
}

int egm_forward_device(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len, uint32_t n,
                       void* hip_stream, uint64_t* d_node_row, uint32_t* d_fwd_topic, uint32_t* d_fwd_fid,
                       uint64_t fwd_cap, uint32_t* d_entry_fwd, uint32_t* d_topic_fwd) {
  if (!c || !d_mrow || !d_node_row || !d_fwd_topic || !d_fwd_fid) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!c->route.built) return c->fail(EGM_E_STATE, "forward: egm_routes_build first");
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = (hipStream_t)hip_stream;   // NULL: the HIP default (null) stream, as the caller's own work
  return run_forward(c, d_mrow, d_mids, mids_len, n, s, d_node_row, d_fwd_topic, d_fwd_fid, fwd_cap, d_entry_fwd,
                     d_topic_fwd, nullptr);
}

int egm_forward_batch(egm_ctx* c, const egm_result* m, egm_forward** out) {
  if (!c || !m || !out) return EGM_E_INVAL;
  *out = nullptr;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!m->row_ptr || (m->n_ids && !m->ids))   // a packed result (EGM_RESULT_PACKED) is not taken here
    return c->fail(EGM_E_INVAL, "egm_forward_batch takes the plain result form (match without EGM_RESULT_PACKED)");
  if (!c->route.built) return c->fail(EGM_E_STATE, "forward: egm_routes_build first");
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = c->stream;
  RouteState& R = c->route;
  const uint32_t n = m->n_topics;
  const uint64_t nids = m->row_ptr[n];
  hipError_t e;
  if ((e = R.mrow.ensure(((uint64_t)n + 1) * 8)) != hipSuccess) return c->hip_fail(e, "r_mrow");
  if ((e = R.mids.ensure(nids * 4 + 16)) != hipSuccess) return c->hip_fail(e, "r_mids");
  if ((e = R.nrow.ensure((ROUTE_MAX_NODES + 1) * 8)) != hipSuccess) return c->hip_fail(e, "r_nrow");
  if ((e = R.efwd.ensure(nids * 4 + 16)) != hipSuccess) return c->hip_fail(e, "r_efwd");
  if ((e = R.tfwd.ensure((uint64_t)n * 4 + 16)) != hipSuccess) return c->hip_fail(e, "r_tfwd");
  if ((e = hipMemcpyAsync(R.mrow.p, m->row_ptr, ((uint64_t)n + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c->hip_fail(e, "H2D match rows");
  if (nids && (e = hipMemcpyAsync(R.mids.p, m->ids, nids * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c->hip_fail(e, "H2D match ids");
  uint64_t cap = nids + 1024, total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((e = R.ftopic.ensure(cap * 4)) != hipSuccess) return c->hip_fail(e, "r_ftopic");
    if ((e = R.ffid.ensure(cap * 4)) != hipSuccess) return c->hip_fail(e, "r_ffid");
    const int r = run_forward(c, R.mrow.as<uint64_t>(), R.mids.as<uint32_t>(), nids, n, s, R.nrow.as<uint64_t>(),
                              R.ftopic.as<uint32_t>(), R.ffid.as<uint32_t>(), cap, R.efwd.as<uint32_t>(),
                              R.tfwd.as<uint32_t>(), &total);
    if (r == EGM_OK) break;
    if (r != EGM_E_OVERFLOW || attempt == 1) return r;
    cap = total + 1024;
  }
  auto al8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
  size_t sz = al8(sizeof(egm_forward));
  const size_t o_row = sz;
  sz += (ROUTE_MAX_NODES + 1) * 8;
  const size_t o_topic = sz;
  sz += al8(total * 4);
  const size_t o_fid = sz;
  sz += al8(total * 4);
  const size_t o_ef = sz;
  sz += al8(nids * 4);
  const size_t o_tf = sz;
  sz += al8((size_t)n * 4);
  uint8_t* mem = (uint8_t*)result_alloc(sz);
  if (!mem) return c->fail(EGM_E_NOMEM, "forward result");
  egm_forward* f = (egm_forward*)mem;
  f->n_topics = n;
  f->n_nodes = ROUTE_MAX_NODES;
  f->n_entries = nids;
  f->n_forwards = total;
  f->node_row = (uint64_t*)(mem + o_row);
  f->topic = (uint32_t*)(mem + o_topic);
  f->fid = (uint32_t*)(mem + o_fid);
  f->entry_fwd = (uint32_t*)(mem + o_ef);
  f->topic_fwd = (uint32_t*)(mem + o_tf);
  if ((e = hipMemcpy(f->node_row, R.nrow.p, (ROUTE_MAX_NODES + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (total && (e = hipMemcpy(f->topic, R.ftopic.p, total * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
      (total && (e = hipMemcpy(f->fid, R.ffid.p, total * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
      (nids && (e = hipMemcpy(f->entry_fwd, R.efwd.p, nids * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
      (n && (e = hipMemcpy(f->topic_fwd, R.tfwd.p, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess)) {
    result_discard(mem);
    return c->hip_fail(e, "D2H forwards");
  }
  *out = f;
  return EGM_OK;
}

int egm_last_forward(egm_ctx* c, uint64_t* n_forwards, uint32_t* overflow) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!c->route.launched) return c->fail(EGM_E_STATE, "no forward pass launched");
  if (set_device(c)) return EGM_E_DEVICE;
  uint64_t st[2] = {0, 0};
  hipError_t e;
  if ((e = hipStreamSynchronize(c->route.last_stream)) != hipSuccess ||
      (e = hipMemcpy(st, c->route.state.p, 16, hipMemcpyDeviceToHost)) != hipSuccess)
    return c->hip_fail(e, "forward readback");
  if (n_forwards) *n_forwards = st[0];
  if (overflow) *overflow = (uint32_t)st[1];
  return EGM_OK;
}

int egm_get_forward_timing(egm_ctx* c, double* ms, uint64_t* launches) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->timing.drain();
  if (ms) *ms = c->timing.fwd.ms;
  if (launches) *launches = c->timing.fwd.n;
  return EGM_OK;
}

}  // extern "C"
