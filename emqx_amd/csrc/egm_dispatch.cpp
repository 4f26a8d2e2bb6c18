// egm_dispatch.cpp — dispatch on the device: the liveness bitmap
// (egm_subs_set_dead), the $share member table (egm_share_*: host lists and
// the two device copies a commit alternates between) and the dispatch itself
// (egm_dispatch_*, egm_last_dispatch): the compact fan-out followed by the
// resolve pass (k_disp_resolve, egm_kernels.hip).
#include <set>
#include <utility>

#include "egm_ctx.h"

using namespace egm;

static constexpr uint32_t GROUP_MASK = 0x7FFFFFFFu;

static inline uint64_t share_key(const egm_share_member& r) { return (uint64_t)r.fid << 32 | (r.group & GROUP_MASK); }

static int share_validate(egm_ctx* c, const egm_share_member* rows, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if ((rows[i].member & ~GROUP_MASK) || rows[i].fid == SUB_NONE)
      return c->fail(EGM_E_INVAL, "share table: a member id has bit 31 clear, a filter id is not 0xFFFFFFFF");
  return EGM_OK;
}

static void share_add(DispState& D, const egm_share_member& r) {
  auto it = D.keys.find(share_key(r));
  if (it == D.keys.end()) {
    it = D.keys.emplace(share_key(r), ShareKey{}).first;
    it->second.slot = D.next_slot++;   // a key seen for the first time (or again, after its last member left)
  }
  std::vector<uint32_t>& M = it->second.members;
  if (std::find(M.begin(), M.end(), r.member) == M.end()) M.push_back(r.member);
}

// rr / sticky hold `need` slots: grown by allocate + device-to-device copy, new
// cursors 0 and new sticky members none.
static int share_grow_slots(egm_ctx* c, uint32_t need) {
  DispState& D = c->disp;
  if (need <= D.slot_cap) return EGM_OK;
  D.uses[0].drain();   // dispatches in flight advance the old arrays
  D.uses[1].drain();
  const uint32_t cap = std::max<uint32_t>(need + need / 2, 1024);
  DevBuf rr, sticky;
  hipError_t e;
  if ((e = rr.ensure((size_t)cap * 4)) != hipSuccess || (e = sticky.ensure((size_t)cap * 4)) != hipSuccess)
    return c->hip_fail(e, "share slots");
  if ((e = hipMemsetAsync(rr.p, 0, (size_t)cap * 4, c->stream)) != hipSuccess ||
      (e = hipMemsetAsync(sticky.p, 0xFF, (size_t)cap * 4, c->stream)) != hipSuccess)
    return c->hip_fail(e, "share slots: fill");
  if (D.slot_cap &&
      ((e = hipMemcpyAsync(rr.p, D.rr.p, (size_t)D.slot_cap * 4, hipMemcpyDeviceToDevice, c->stream)) != hipSuccess ||
       (e = hipMemcpyAsync(sticky.p, D.sticky.p, (size_t)D.slot_cap * 4, hipMemcpyDeviceToDevice, c->stream)) !=
           hipSuccess))
    return c->hip_fail(e, "share slots: copy");
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "share slots: sync");
  std::swap(D.rr.p, rr.p);
  std::swap(D.rr.cap, rr.cap);
  std::swap(D.sticky.p, sticky.p);
  std::swap(D.sticky.cap, sticky.cap);
  D.slot_cap = cap;
  return EGM_OK;
}

// The whole table, rebuilt on the host into the copy no dispatch in flight reads.
static int share_commit(egm_ctx* c, uint64_t* epoch) {
  DispState& D = c->disp;
  const int x = 1 - D.cur;
  D.uses[x].drain();
  std::vector<std::pair<uint32_t, uint64_t>> order;   // (slot, key): a layout that does not depend on the map's order
  order.reserve(D.keys.size());
  uint64_t n_mem = 0;
  for (const auto& kv : D.keys) {
    order.push_back({kv.second.slot, kv.first});
    n_mem += kv.second.members.size();
  }
  if (n_mem >= 0xFFFFFFFFull || order.size() >= (1ull << 29))
    return c->fail(EGM_E_INVAL, "share table: at most 2^32 members and 2^29 keys");
  std::sort(order.begin(), order.end());
  uint32_t nb = 0;   // buckets: a power of two, at most half full
  if (!order.empty()) {
    nb = 1;
    while ((uint64_t)nb * SHARE_BUCKET < order.size() * 2) nb <<= 1;
  }
  const uint64_t n_rec = (uint64_t)nb * SHARE_BUCKET;
  std::vector<uint4> hash(n_rec, make_uint4(SUB_NONE, SUB_NONE, 0, 0));
  std::vector<uint32_t> cnt(n_rec, 0), mem;
  mem.reserve(n_mem);
  for (const auto& sk : order) {
    const ShareKey& K = D.keys[sk.second];
    const uint32_t fid = (uint32_t)(sk.second >> 32), group = (uint32_t)sk.second;
    uint32_t b = share_bucket(fid, group, nb);
    uint64_t at = n_rec;
    for (uint32_t step = 0; step < nb && at == n_rec; ++step, b = (b + 1) & (nb - 1))
      for (uint32_t k = 0; k < SHARE_BUCKET; ++k)
        if (hash[(uint64_t)b * SHARE_BUCKET + k].x == SUB_NONE) {
          at = (uint64_t)b * SHARE_BUCKET + k;
          break;
        }
    if (at == n_rec) return c->fail(EGM_E_DEVICE, "share table: no free record (a bug)");
    hash[at] = make_uint4(fid, group, (uint32_t)mem.size(), K.slot);
    cnt[at] = (uint32_t)K.members.size();
    mem.insert(mem.end(), K.members.begin(), K.members.end());
  }
  int r = share_grow_slots(c, D.next_slot);
  if (r != EGM_OK) return r;
  ShareCopy& S = D.copy[x];
  hipError_t e;
  if (nb) {
    if ((e = S.hash.ensure(n_rec * 16)) != hipSuccess || (e = S.cnt.ensure(n_rec * 4)) != hipSuccess ||
        (e = S.members.ensure(mem.size() * 4 + 16)) != hipSuccess)
      return c->hip_fail(e, "share table");
    if ((e = hipMemcpy(S.hash.p, hash.data(), n_rec * 16, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(S.cnt.p, cnt.data(), n_rec * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(S.members.p, mem.data(), mem.size() * 4, hipMemcpyHostToDevice)) != hipSuccess)
      return c->hip_fail(e, "H2D share table");
  }
  S.n_buckets = nb;
  D.cur = x;
  D.epoch += 1;
  if (epoch) *epoch = D.epoch;
  return EGM_OK;
}

static int subs_set_dead(egm_ctx* c, const uint32_t* subs, uint64_t n, int dead) {
  DispState& D = c->disp;
  uint32_t hi = 0;
  for (uint64_t i = 0; i < n; ++i) hi = std::max(hi, subs[i]);
  // an id past the bitmap is alive already: only a dead one grows it
  if (dead && (uint64_t)(hi >> 5) + 1 > D.dead_host.size()) D.dead_host.resize((size_t)(hi >> 5) + 1, 0u);
  std::vector<uint32_t> idx;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t w = subs[i] >> 5, bit = 1u << (subs[i] & 31u);
    if (w >= D.dead_host.size()) continue;
    const uint32_t old = D.dead_host[w];
    D.dead_host[w] = dead ? (old | bit) : (old & ~bit);
    if (D.dead_host[w] != old) idx.push_back(w);
  }
  if (idx.empty()) return EGM_OK;
  if (set_device(c)) return EGM_E_DEVICE;
  hipError_t e;
  const uint64_t words = D.dead_host.size();
  if (words > D.dead_words) {   // grown: the whole bitmap again
    if (words * 4 > D.dead.cap) {
      D.uses[0].drain();   // dispatches in flight read the old allocation
      D.uses[1].drain();
      if ((e = D.dead.ensure((size_t)std::max<uint64_t>(words * 4 * 2, 4096))) != hipSuccess)
        return c->hip_fail(e, "dead bitmap");
    }
    if ((e = hipMemcpy(D.dead.p, D.dead_host.data(), words * 4, hipMemcpyHostToDevice)) != hipSuccess)
      return c->hip_fail(e, "H2D dead bitmap");
    D.dead_words = words;
    return EGM_OK;
  }
  // the changed words, merged on the host, written whole (a dispatch in flight sees a word's old or new state)
  sort_unique(idx);
  const size_t o_val = (idx.size() * 4 + 15) & ~(size_t)15, total = o_val + idx.size() * 4;
  uint8_t* h = patch_stage(c, total);
  if (!h) return c->fail(EGM_E_NOMEM, "dead bitmap: pinned staging");
  memcpy(h, idx.data(), idx.size() * 4);
  for (size_t i = 0; i < idx.size(); ++i) memcpy(h + o_val + 4 * i, &D.dead_host[idx[i]], 4);
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "dead bitmap: stream");
  if ((e = c->patch_dev.ensure(total)) != hipSuccess) return c->hip_fail(e, "dead bitmap: patch buffer");
  uint8_t* dp = (uint8_t*)c->patch_dev.p;
  if ((e = hipMemcpyAsync(dp, h, total, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
      (e = launch_patch(D.dead.p, 4, (const uint32_t*)dp, dp + o_val, idx.size(), c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return c->hip_fail(e, "dead bitmap: patch");
  return EGM_OK;
}

static bool pick_hashed(int strategy) { return strategy >= PICK_HASH; }

static int run_dispatch(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len, uint32_t n,
                        const uint32_t* d_key, int strategy, uint64_t seed, hipStream_t s, uint64_t* d_drow,
                        uint64_t* d_epos, uint32_t* d_sub, uint64_t cap, uint32_t* d_live, uint32_t* d_shared,
                        uint64_t* total) {
  DispState& D = c->disp;
  hipError_t e;
  if (!D.stats.p && ((e = D.stats.ensure(4 * sizeof(unsigned long long))) != hipSuccess ||
                     (e = hipMemset(D.stats.p, 0, 4 * sizeof(unsigned long long))) != hipSuccess))
    return c->hip_fail(e, "dispatch stats");
  const ShareCopy& S = D.copy[D.cur];
  DispArgs da;
  da.t = DispTable{D.dead.as<uint32_t>(), (uint32_t)D.dead_words, S.hash.as<uint4>(), S.n_buckets,
                   S.members.as<uint32_t>(), S.cnt.as<uint32_t>(), D.rr.as<uint32_t>(), D.sticky.as<uint32_t>()};
  da.msg_key = d_key;
  da.strategy = strategy;
  da.seed = seed;
  da.seq = D.seq++;
  da.entry_live = d_live;
  da.entry_shared = d_shared;
  da.stats = D.stats.as<unsigned long long>();
  D.last_stream = s;
  D.launched = true;
  return run_fanout(c, d_mrow, d_mids, mids_len, n, s, d_drow, nullptr, d_sub, cap, total, d_epos, &da);
}

extern "C" {

int egm_subs_set_dead(egm_ctx* c, const uint32_t* subs, uint64_t n, int dead) {
  if (!c || (n && !subs)) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  for (uint64_t i = 0; i < n; ++i)
    if (subs[i] & ~GROUP_MASK) return c->fail(EGM_E_INVAL, "egm_subs_set_dead: a subscriber id has bit 31 clear");
  if (!n) return EGM_OK;
  return no_throw(c, "dead bitmap: host allocation", [&] { return subs_set_dead(c, subs, n, dead); });
}

int egm_share_build(egm_ctx* c, const egm_share_member* rows, uint64_t n) {
  if (!c || (n && !rows)) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (share_validate(c, rows, n)) return EGM_E_INVAL;
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "share build: host allocation", [&] {
    c->disp.keys.clear();   // (their slots are not reused)
    for (uint64_t i = 0; i < n; ++i) share_add(c->disp, rows[i]);
    return share_commit(c, nullptr);
  });
}

int egm_share_apply_delta(egm_ctx* c, const egm_share_member* add, uint64_t n_add, const egm_share_member* del,
                          uint64_t n_del) {
  if (!c || (n_add && !add) || (n_del && !del)) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (share_validate(c, add, n_add)) return EGM_E_INVAL;
  return no_throw(c, "share delta: host allocation", [&] {
    DispState& D = c->disp;
    // net changes (egm_subs_apply_delta's contract): a triple in both lists is refused before anything is applied
    if (n_add && n_del) {
      std::set<std::pair<uint64_t, uint32_t>> adds;
      for (uint64_t i = 0; i < n_add; ++i) adds.insert({share_key(add[i]), add[i].member});
      for (uint64_t i = 0; i < n_del; ++i)
        if (adds.count({share_key(del[i]), del[i].member}))
          return c->fail(EGM_E_INVAL, "share delta: a (filter, group, member) triple is both added and removed");
    }
    for (uint64_t i = 0; i < n_add; ++i) share_add(D, add[i]);
    for (uint64_t i = 0; i < n_del; ++i) {
      auto it = D.keys.find(share_key(del[i]));
      if (it == D.keys.end()) continue;
      std::vector<uint32_t>& M = it->second.members;
      auto m = std::find(M.begin(), M.end(), del[i].member);
      if (m != M.end()) M.erase(m);
      if (M.empty()) D.keys.erase(it);   // the key is gone: added again it is a new key
    }
    return (int)EGM_OK;
  });
}

int egm_share_commit(egm_ctx* c, uint64_t* epoch) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "share commit: host allocation", [&] { return share_commit(c, epoch); });
}

int egm_dispatch_device(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len, uint32_t n,
                        const uint32_t* d_msg_key, int strategy, uint64_t seed, void* hip_stream, uint64_t* d_drow,
                        uint64_t* d_entry_pos, uint32_t* d_sub, uint64_t cap, uint32_t* d_entry_live,
                        uint32_t* d_entry_shared) {
  if (!c || !d_mrow || !d_drow || !d_entry_pos || !d_entry_live || !d_entry_shared) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (strategy < PICK_RANDOM || strategy > PICK_HASH_TOPIC) return c->fail(EGM_E_INVAL, "dispatch: unknown strategy");
  if (pick_hashed(strategy) && !d_msg_key) return c->fail(EGM_E_INVAL, "dispatch: a hash strategy needs d_msg_key");
  if (!c->fan.subs.built) return c->fail(EGM_E_STATE, "dispatch: egm_subs_build first");
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = (hipStream_t)hip_stream;   // NULL: the HIP default (null) stream, as the caller's own work
  return run_dispatch(c, d_mrow, d_mids, mids_len, n, d_msg_key, strategy, seed, s, d_drow, d_entry_pos, d_sub, cap,
                      d_entry_live, d_entry_shared, nullptr);
}

int egm_dispatch_batch(egm_ctx* c, const egm_result* m, const uint32_t* msg_key, int strategy, uint64_t seed,
                       egm_dispatch** out) {
  if (!c || !m || !out) return EGM_E_INVAL;
  *out = nullptr;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!m->row_ptr || (m->n_ids && !m->ids))   // a packed result (EGM_RESULT_PACKED) is not taken here
    return c->fail(EGM_E_INVAL, "egm_dispatch_batch takes the plain result form (match without EGM_RESULT_PACKED)");
  if (strategy < PICK_RANDOM || strategy > PICK_HASH_TOPIC) return c->fail(EGM_E_INVAL, "dispatch: unknown strategy");
  if (pick_hashed(strategy) && !msg_key) return c->fail(EGM_E_INVAL, "dispatch: a hash strategy needs msg_key");
  if (!c->fan.subs.built) return c->fail(EGM_E_STATE, "dispatch: egm_subs_build first");
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = c->stream;
  DispState& D = c->disp;
  const uint32_t n = m->n_topics;
  const uint64_t nids = m->row_ptr[n];
  hipError_t e;
  if ((e = c->fan.mrow.ensure(((uint64_t)n + 1) * 8)) != hipSuccess) return c->hip_fail(e, "f_mrow");
  if ((e = c->fan.mids.ensure(nids * 4 + 16)) != hipSuccess) return c->hip_fail(e, "f_mids");
  if ((e = c->fan.drow.ensure(((uint64_t)n + 1) * 8)) != hipSuccess) return c->hip_fail(e, "f_drow");
  if ((e = D.mkey.ensure((uint64_t)n * 4 + 16)) != hipSuccess) return c->hip_fail(e, "d_mkey");
  if ((e = D.epos.ensure((nids + 2) * 8)) != hipSuccess) return c->hip_fail(e, "d_epos");
  if ((e = D.elive.ensure(nids * 4 + 16)) != hipSuccess) return c->hip_fail(e, "d_elive");
  if ((e = D.eshared.ensure(nids * 4 + 16)) != hipSuccess) return c->hip_fail(e, "d_eshared");
  if ((e = hipMemcpyAsync(c->fan.mrow.p, m->row_ptr, ((uint64_t)n + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c->hip_fail(e, "H2D match rows");
  if (nids && (e = hipMemcpyAsync(c->fan.mids.p, m->ids, nids * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c->hip_fail(e, "H2D match ids");
  if (msg_key && n && (e = hipMemcpyAsync(D.mkey.p, msg_key, (uint64_t)n * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c->hip_fail(e, "H2D message keys");
  uint64_t cap = nids * 2 + 1024, total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((e = c->fan.dsub.ensure(cap * 4)) != hipSuccess) return c->hip_fail(e, "f_dsub");
    int r = run_dispatch(c, c->fan.mrow.as<uint64_t>(), c->fan.mids.as<uint32_t>(), nids, n,
                         msg_key ? D.mkey.as<uint32_t>() : nullptr, strategy, seed, s, c->fan.drow.as<uint64_t>(),
                         D.epos.as<uint64_t>(), c->fan.dsub.as<uint32_t>(), cap, D.elive.as<uint32_t>(),
                         D.eshared.as<uint32_t>(), &total);
    if (r == EGM_OK) break;
    if (r != EGM_E_OVERFLOW || attempt == 1) return r;
    cap = total + 1024;
  }
  auto al8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
  size_t sz = al8(sizeof(egm_dispatch));
  const size_t o_row = sz;
  sz += ((uint64_t)n + 1) * 8;
  const size_t o_pos = sz;
  sz += (nids + 1) * 8;
  const size_t o_sub = sz;
  sz += al8(total * 4);
  const size_t o_live = sz;
  sz += al8(nids * 4);
  const size_t o_sh = sz;
  sz += al8(nids * 4);
  uint8_t* mem = (uint8_t*)result_alloc(sz);
  if (!mem) return c->fail(EGM_E_NOMEM, "dispatch result");
  egm_dispatch* d = (egm_dispatch*)mem;
  d->n_topics = n;
  d->n_entries = nids;
  d->n_deliveries = total;
  d->row_ptr = (uint64_t*)(mem + o_row);
  d->entry_pos = (uint64_t*)(mem + o_pos);
  d->sub = (uint32_t*)(mem + o_sub);
  d->entry_live = (uint32_t*)(mem + o_live);
  d->entry_shared = (uint32_t*)(mem + o_sh);
  if ((e = hipMemcpy(d->row_ptr, c->fan.drow.p, ((uint64_t)n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(d->entry_pos, D.epos.p, (nids + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (total && (e = hipMemcpy(d->sub, c->fan.dsub.p, total * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
      (nids && (e = hipMemcpy(d->entry_live, D.elive.p, nids * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
      (nids && (e = hipMemcpy(d->entry_shared, D.eshared.p, nids * 4, hipMemcpyDeviceToHost)) != hipSuccess)) {
    result_discard(mem);
    return c->hip_fail(e, "D2H dispatch");
  }
  *out = d;
  return EGM_OK;
}

int egm_last_dispatch(egm_ctx* c, uint64_t* dead_dropped, uint64_t* groups_resolved, uint64_t* groups_empty,
                      uint64_t* missing_groups) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!c->disp.launched) return c->fail(EGM_E_STATE, "no dispatch launched");
  if (set_device(c)) return EGM_E_DEVICE;
  unsigned long long st[4] = {0, 0, 0, 0};
  hipError_t e;
  if ((e = hipStreamSynchronize(c->disp.last_stream)) != hipSuccess ||
      (e = hipMemcpy(st, c->disp.stats.p, sizeof(st), hipMemcpyDeviceToHost)) != hipSuccess)
    return c->hip_fail(e, "dispatch readback");
  if (dead_dropped) *dead_dropped = st[0];
  if (groups_resolved) *groups_resolved = st[1];
  if (groups_empty) *groups_empty = st[2];
  if (missing_groups) *missing_groups = st[3];
  return EGM_OK;
}

int egm_get_dispatch_timing(egm_ctx* c, double* resolve_ms, uint64_t* launches) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->timing.drain();
  if (resolve_ms) *resolve_ms = c->timing.disp.ms;
  if (launches) *launches = c->timing.disp.n;
  return EGM_OK;
}

}  // extern "C"
