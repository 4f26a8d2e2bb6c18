// egm_fanout.cpp — the subscriber table (egm_subs_*: host lists, the device
// entries and the two record copies a commit alternates between) and the
// fan-out of matched filter ids to deliveries (egm_fanout_*, egm_last_fanout).
#include <unordered_set>

#include "egm_ctx.h"

using namespace egm;

// The record of filter f with subscribers L whose row (if stored) starts at
// `start` — k_sub_pairs' layout (egm_kernels.hip): x = the third subscriber
// of a row of at most FAN_INLINE_ALL (3), else the row start's low 32 bits;
// y = start bits 32-39 | count (24 bits, saturated) << 8; z, w = the first two.
static uint4 sub_record(const uint32_t* L, uint64_t cnt, uint64_t start) {
  const uint32_t cs = (uint32_t)std::min<uint64_t>(cnt, (1u << 24) - 1);
  const uint32_t x = cnt <= 3 ? (cnt > 2 ? L[2] : 0u) : (uint32_t)start;
  const uint32_t y = (cnt <= 3 ? 0u : ((uint32_t)(start >> 32) & 0xFFu)) | (cs << 8);
  return make_uint4(x, y, cnt > 0 ? L[0] : 0u, cnt > 1 ? L[1] : 0u);
}

// Full build from the host lists (egm_subs_build, and a commit that cannot patch).
static int subs_upload(egm_ctx* c, const uint64_t* row, uint32_t n_slots, const uint32_t* subs) {
  const uint64_t ns = row[n_slots];
  hipError_t e;
  c->fan.subs.uses[0].drain();
  c->fan.subs.uses[1].drain();
  if ((e = hipDeviceSynchronize()) != hipSuccess) return c->hip_fail(e, "subs: device sync");
  if ((e = c->fan.sub_row.ensure(((uint64_t)n_slots + 1) * 8)) != hipSuccess) return c->hip_fail(e, "sub_row");
  // room for appended rows: a quarter of the table + 64K entries before the next full build
  if ((e = c->fan.sub_ids.ensure((ns + ns / 4 + 65536) * 4 + 16)) != hipSuccess) return c->hip_fail(e, "sub_ids");
  if ((e = hipMemcpy(c->fan.sub_row.p, row, ((uint64_t)n_slots + 1) * 8, hipMemcpyHostToDevice)) != hipSuccess)
    return c->hip_fail(e, "H2D sub_row");
  if (ns && (e = hipMemcpy(c->fan.sub_ids.p, subs, ns * 4, hipMemcpyHostToDevice)) != hipSuccess)
    return c->hip_fail(e, "H2D subs");
  for (int k = 0; k < 2; ++k)
    if ((e = c->fan.sub_rec(k).ensure(((uint64_t)n_slots + 1) * 16)) != hipSuccess) return c->hip_fail(e, "sub_rp");
  if ((e = launch_sub_pairs(c->fan.sub_row.as<uint64_t>(), c->fan.sub_ids.as<uint32_t>(), n_slots, c->fan.sub_rp.as<uint4>(),
                            c->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(c->fan.sub_rp2.p, c->fan.sub_rp.p, (uint64_t)n_slots * 16, hipMemcpyDeviceToDevice, c->stream)) !=
          hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return c->hip_fail(e, "sub pairs");
  c->fan.n_fid_slots = n_slots;
  SubsState& S = c->fan.subs;
  S.lists.clear();
  S.recs.clear();
  S.pending.clear();
  S.stale[0].clear();
  S.stale[1].clear();
  S.tail = ns;
  S.garbage = 0;
  S.cur = 0;
  S.built = true;
  S.epoch += 1;
  return EGM_OK;
}

extern "C" {

int egm_subs_build(egm_ctx* c, const uint64_t* row, uint32_t n_slots, const uint32_t* subs) {
  if (!c || !row) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  for (uint32_t i = 0; i < n_slots; ++i)
    if (row[i + 1] < row[i]) return EGM_E_INVAL;
  const uint64_t ns = row[n_slots];
  if (ns && !subs) return EGM_E_INVAL;
  if (ns >= (1ull << 40)) return c->fail(EGM_E_INVAL, "subscriber table: at most 2^40 entries (40-bit row starts)");
  return no_throw(c, "subscriber build: host allocation", [&] {
  // the host keeps the lists: the base of later incremental changes (egm_subs_apply_delta)
  SubsState& S = c->fan.subs;
  // record slots beyond the given filter ids (empty rows): new filters subscribed
  // later are patched in, not rebuilt
  const uint32_t cap_slots = (uint32_t)std::min<uint64_t>(WID_MAX, (uint64_t)n_slots + n_slots / 4 + 4096);
  S.row.assign(row, row + (uint64_t)n_slots + 1);
  S.row.resize((uint64_t)cap_slots + 1, row[n_slots]);
  if (subs)
    S.subs.assign(subs, subs + ns);
  else
    S.subs.clear();
  return subs_upload(c, S.row.data(), cap_slots, S.subs.data());
  });
}

// The current subscriber list of filter f (host).
static std::vector<uint32_t>* subs_list(SubsState& S, uint32_t f, bool create) {
  auto it = S.lists.find(f);
  if (it != S.lists.end()) return &it->second;
  if (!create) return nullptr;
  std::vector<uint32_t>& L = S.lists[f];
  if ((uint64_t)f + 1 < S.row.size()) L.assign(S.subs.begin() + S.row[f], S.subs.begin() + S.row[f + 1]);
  return &L;
}

// New filter ids a delta may introduce past the table's current slots.  Filter
// ids are dense (the table builder assigns them in insertion order), so one
// delta never legitimately reaches millions of ids past the table; a larger id
// is a stale or garbage id from the caller, refused before it can size a
// rebuild (one id near WID_MAX asked for a ~34 GB row vector).
static constexpr uint64_t SUBS_FID_GROWTH = 1ull << 22;

static int subs_apply_delta(egm_ctx* c, const egm_sub_pair* add, uint64_t n_add, const egm_sub_pair* del,
                            uint64_t n_del) {
  SubsState& S = c->fan.subs;
  if (!S.built) return c->fail(EGM_E_STATE, "subscriber table: egm_subs_build first");
  const uint64_t fid_limit = std::max<uint64_t>(c->fan.n_fid_slots, S.row.size() - 1) + SUBS_FID_GROWTH;
  for (uint64_t i = 0; i < n_add; ++i)
    if (add[i].fid >= WID_MAX || add[i].fid >= fid_limit)
      return c->fail(EGM_E_INVAL, "subscriber delta: filter id out of range");
  // The two lists are NET effects since the caller's last delta, so a pair
  // may not be in both: adds are applied before removes, and "unsubscribe X,
  // subscribe X" passed as Adds=[X], Dels=[X] would silently drop X.  Refused
  // before anything is applied.
  if (n_add && n_del) {
    std::unordered_set<uint64_t> adds;
    adds.reserve(n_add * 2);
    for (uint64_t i = 0; i < n_add; ++i) adds.insert((uint64_t)add[i].fid << 32 | add[i].sub);
    for (uint64_t i = 0; i < n_del; ++i)
      if (adds.count((uint64_t)del[i].fid << 32 | del[i].sub))
        return c->fail(EGM_E_INVAL, "subscriber delta: a (filter, subscriber) pair is both added and removed");
  }
  // subscribe: a subscriber is in a filter's bag at most once (an ets bag keeps
  // one copy of an identical object, emqx_broker.erl:144-157)
  for (uint64_t i = 0; i < n_add; ++i) {
    std::vector<uint32_t>& L = *subs_list(S, add[i].fid, true);
    if (std::find(L.begin(), L.end(), add[i].sub) == L.end()) L.push_back(add[i].sub);
    S.pending.push_back(add[i].fid);
  }
  // unsubscribe / subscriber_down: removed wherever present, order kept (:178-190, 331-345)
  for (uint64_t i = 0; i < n_del; ++i) {
    if (del[i].fid >= WID_MAX) continue;
    std::vector<uint32_t>* L = subs_list(S, del[i].fid, (uint64_t)del[i].fid + 1 < S.row.size());
    if (!L) continue;
    auto it = std::find(L->begin(), L->end(), del[i].sub);
    if (it != L->end()) {
      L->erase(it);
      S.pending.push_back(del[i].fid);
    }
  }
  return EGM_OK;
}

int egm_subs_apply_delta(egm_ctx* c, const egm_sub_pair* add, uint64_t n_add, const egm_sub_pair* del,
                         uint64_t n_del) {
  if (!c || (n_add && !add) || (n_del && !del)) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  return no_throw(c, "subscriber delta: host allocation", [&] { return subs_apply_delta(c, add, n_add, del, n_del); });
}

static int subs_commit(egm_ctx* c, uint64_t* epoch);

int egm_subs_commit(egm_ctx* c, uint64_t* epoch) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "subscriber commit: host allocation", [&] { return subs_commit(c, epoch); });
}

static int subs_commit(egm_ctx* c, uint64_t* epoch) {
  SubsState& S = c->fan.subs;
  if (!S.built) return c->fail(EGM_E_STATE, "subscriber table: egm_subs_build first");
  S.last_appended = S.last_patched = 0;
  S.last_rebuilt = false;
  std::vector<uint32_t> P = S.pending;
  sort_unique(P);
  // a full build instead of a patch: a new filter id past the table's slots, a
  // row too long for the record's 24-bit count, no room left for appended rows,
  // or more superseded entries than live ones
  bool rebuild = false;
  uint64_t append = 0;
  for (uint32_t f : P) {
    const std::vector<uint32_t>& L = *subs_list(S, f, true);
    if (f >= c->fan.n_fid_slots) rebuild = true;
    if (L.size() >= (1u << 24) - 1) rebuild = true;
    if (L.size() > 3) append += L.size();
  }
  const uint64_t cap_ids = c->fan.sub_ids.cap / 4;
  if (S.tail + append + 16 > cap_ids || S.garbage + append > S.tail / 2 + 65536) rebuild = true;
  if (rebuild) {
    // flatten: the build's lists with every changed list in place (and new
    // empty slots).  Sized from the largest LIVE filter id — a non-empty base
    // row or changed list, or a new id — not from the padded slot count, so
    // repeated rebuilds under churn do not grow the table.
    uint64_t hi = 0;
    for (uint64_t f = S.row.size() - 1; f > 0; --f)
      if (S.row[f] > S.row[f - 1]) {
        hi = f;
        break;
      }
    for (const auto& kv : S.lists)
      if (!kv.second.empty()) hi = std::max<uint64_t>(hi, (uint64_t)kv.first + 1);
    for (uint32_t f : P)
      if (f >= c->fan.n_fid_slots) hi = std::max<uint64_t>(hi, (uint64_t)f + 1);
    const uint32_t n = (uint32_t)std::min<uint64_t>(WID_MAX, hi + hi / 4 + 4096);
    std::vector<uint64_t> row((uint64_t)n + 1, 0);
    for (uint32_t f = 0; f < n; ++f) {
      auto it = S.lists.find(f);
      const uint64_t k = it != S.lists.end() ? it->second.size()
                         : ((uint64_t)f + 1 < S.row.size() ? S.row[f + 1] - S.row[f] : 0);
      row[f + 1] = row[f] + k;
    }
    std::vector<uint32_t> flat(row[n]);
    for (uint32_t f = 0; f < n; ++f) {
      auto it = S.lists.find(f);
      if (it != S.lists.end())
        std::copy(it->second.begin(), it->second.end(), flat.begin() + row[f]);
      else if ((uint64_t)f + 1 < S.row.size())
        std::copy(S.subs.begin() + S.row[f], S.subs.begin() + S.row[f + 1], flat.begin() + row[f]);
    }
    if (row[n] >= (1ull << 40)) return c->fail(EGM_E_INVAL, "subscriber table: at most 2^40 entries");
    S.row.swap(row);
    S.subs.swap(flat);
    const int r = subs_upload(c, S.row.data(), n, S.subs.data());
    if (r == EGM_OK) S.last_rebuilt = true;
    if (epoch) *epoch = S.epoch;
    return r;
  }
  // appended rows and the new records of the changed filters
  std::vector<uint32_t> app;
  app.reserve(append);
  const uint64_t base = S.tail;
  for (uint32_t f : P) {
    const std::vector<uint32_t>& L = *subs_list(S, f, true);
    const uint64_t start = L.size() > 3 ? base + app.size() : 0;
    if (L.size() > 3) app.insert(app.end(), L.begin(), L.end());
    auto old = S.recs.find(f);
    const uint64_t old_cnt = old != S.recs.end() ? (old->second.y >> 8)
                             : ((uint64_t)f + 1 < S.row.size() ? S.row[f + 1] - S.row[f] : 0);
    if (old_cnt > 3) S.garbage += old_cnt;
    S.recs[f] = sub_record(L.data(), L.size(), start);
  }
  // the copy no reader uses: its last readers first, then every record it lacks
  const int x = 1 - S.cur;
  S.uses[x].drain();
  std::vector<uint32_t> need = S.stale[x];
  need.insert(need.end(), P.begin(), P.end());
  sort_unique(need);
  hipError_t e;
  const size_t o_app = 0, o_idx = (app.size() * 4 + 15) & ~(size_t)15, o_rec = (o_idx + need.size() * 4 + 15) & ~(size_t)15;
  const size_t total = o_rec + need.size() * 16;
  if (total) {
    uint8_t* h = patch_stage(c, total);
    if (!h) return c->fail(EGM_E_NOMEM, "subs commit: pinned staging");
    memcpy(h + o_app, app.data(), app.size() * 4);
    memcpy(h + o_idx, need.data(), need.size() * 4);
    for (size_t i = 0; i < need.size(); ++i) memcpy(h + o_rec + 16 * i, &S.recs[need[i]], 16);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "subs commit: stream");
    if ((e = c->patch_dev.ensure(total)) != hipSuccess) return c->hip_fail(e, "subs commit: patch buffer");
    if ((e = hipMemcpyAsync(c->patch_dev.p, h, total, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
      return c->hip_fail(e, "subs commit: upload");
    uint8_t* dp = (uint8_t*)c->patch_dev.p;
    // appended rows lie past every entry a reader of either copy can reach
    if (!app.empty() &&
        (e = hipMemcpyAsync(c->fan.sub_ids.as<uint32_t>() + base, dp + o_app, app.size() * 4, hipMemcpyDeviceToDevice,
                            c->stream)) != hipSuccess)
      return c->hip_fail(e, "subs commit: rows");
    if ((e = launch_patch(c->fan.sub_rec(x).p, 16, (const uint32_t*)(dp + o_idx), dp + o_rec, need.size(), c->stream)) !=
        hipSuccess)
      return c->hip_fail(e, "subs commit: patch");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "subs commit: sync");
  }
  S.tail = base + app.size();
  S.stale[x].clear();
  S.stale[S.cur].insert(S.stale[S.cur].end(), P.begin(), P.end());   // the old copy now lacks this commit
  S.cur = x;
  S.pending.clear();
  S.epoch += 1;
  S.last_appended = app.size();
  S.last_patched = need.size();
  if (epoch) *epoch = S.epoch;
  return EGM_OK;
}

int egm_subs_slots(egm_ctx* c, uint32_t* n_fid_slots) {
  if (!c || !n_fid_slots) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  *n_fid_slots = c->fan.n_fid_slots;
  return EGM_OK;
}

int egm_subs_last_commit(egm_ctx* c, uint64_t* appended, uint64_t* patched, int* rebuilt, uint64_t* entries) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (appended) *appended = c->fan.subs.last_appended;
  if (patched) *patched = c->fan.subs.last_patched;
  if (rebuilt) *rebuilt = c->fan.subs.last_rebuilt ? 1 : 0;
  if (entries) *entries = c->fan.subs.tail;
  return EGM_OK;
}

}  // extern "C"

int egm::run_fanout(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len, uint32_t n,
                    hipStream_t s, uint64_t* d_drow, uint32_t* d_fid, uint32_t* d_sub, uint64_t cap, uint64_t* total,
                    uint64_t* d_entry_pos, const DispArgs* da) {
  uint64_t nids = 0;
  hipError_t e = hipMemcpyAsync(&nids, d_mrow + n, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return c->hip_fail(e, "match_row readback");
  if (nids >= 0xFFFFFFF0ull) return c->fail(EGM_E_INVAL, "too many matched ids for one fan-out batch");
  if (nids > mids_len) return c->fail(EGM_E_OVERFLOW, "match row total exceeds the id buffer (overflowed match batch)");
  const uint64_t nwin = (nids + 63) / 64;
  if ((e = c->fan.dc.ensure((nwin + 1) * 4)) != hipSuccess) return c->hip_fail(e, "f_dc");   // window totals
  const bool ord = c->last_walk.order && c->last_walk.row == d_mrow && c->last_walk.n == n;
  if (fan_uses_ds0(ord) && (e = c->fan.ds0.ensure((nids + 1) * 16)) != hipSuccess)
    return c->hip_fail(e, "f_ds0");   // entry records (the two-pass form)
  if ((e = c->fan.wbase.ensure((nwin + 2) * 8)) != hipSuccess) return c->hip_fail(e, "f_wbase");
  if (!d_entry_pos && (e = c->fan.dpos.ensure((nids + 2) * 8)) != hipSuccess) return c->hip_fail(e, "f_dpos");
  uint64_t* dpos = d_entry_pos ? d_entry_pos : c->fan.dpos.as<uint64_t>();   // the caller's, in the compact form
  if ((e = c->fan.tiles.ensure((scan_tiles((uint32_t)nwin) + 2) * 8)) != hipSuccess) return c->hip_fail(e, "f_tiles");
  if ((e = c->fan.ovf.ensure(16)) != hipSuccess) return c->hip_fail(e, "f_ovf");
  const int rk = c->fan.subs.cur;   // the current record copy; a commit patches the other one
  SubTable st{c->fan.sub_row.as<uint64_t>(), c->fan.sub_ids.as<uint32_t>(), c->fan.n_fid_slots, c->fan.sub_rec(rk).as<uint4>()};
  hipEvent_t evs[2] = {nullptr, nullptr};
  hipEvent_t* evp = c->timing.take_pair(evs);
  c->work_begin(s);
  // these rows are the last match's: count in its walk order (the workspace
  // holding it is then protected until this fan-out has read it)
  MatchWs* OW = ord ? &c->ws[c->last_walk.ws] : nullptr;
  if (OW && OW->used && OW->stream != s && OW->ev) hipStreamWaitEvent(s, OW->ev, 0);   // (stream 0 is a stream too)
  hipEvent_t evd[2] = {nullptr, nullptr};
  hipEvent_t* evdp = da ? c->timing.take_pair(evd) : nullptr;
  if (da)   // the dispatch: the compact fan-out, then the resolve pass over its deliveries
    e = launch_dispatch(st, d_mrow, d_mids, n, nids, d_drow, d_sub, cap, c->fan.dc.as<uint32_t>(),
                        c->fan.ds0.as<uint4>(), dpos, c->fan.wbase.as<uint64_t>(), c->fan.tiles.as<uint64_t>(),
                        c->fan.ovf.as<unsigned int>(), s, evp, ord ? c->last_walk.order : nullptr, *da, evdp);
  else
    e = launch_fanout(st, d_mrow, d_mids, n, nids, d_drow, d_fid, d_sub, cap, c->fan.dc.as<uint32_t>(),
                      c->fan.ds0.as<uint4>(), dpos, c->fan.wbase.as<uint64_t>(), c->fan.tiles.as<uint64_t>(),
                      c->fan.ovf.as<unsigned int>(), s, evp, ord ? c->last_walk.order : nullptr);
  if (OW) ws_done(*OW, s);
  c->fan.subs.uses[rk].note(s);   // a later subscriber commit must not patch this copy before the fan-out has read it
  c->timing.push_pair(c->timing.fan, evp);
  if (da) {
    c->disp.uses[c->disp.cur].note(s);   // ... nor a share commit, a bitmap growth or a cursor growth free what it reads
    c->timing.push_pair(c->timing.disp, evdp);
  }
  c->work_end(s);
  c->fan.last_drow = d_drow;
  c->fan.last_topics = n;
  c->fan.last_stream = s;
  if (e != hipSuccess) return c->hip_fail(e, "launch_fanout");
  if (total) {
    unsigned int ovf = 0;
    if ((e = hipMemcpyAsync(total, d_drow + n, 8, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipMemcpyAsync(&ovf, c->fan.ovf.p, 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
      return c->hip_fail(e, "fanout readback");
    if (ovf) return EGM_E_OVERFLOW;
  }
  return EGM_OK;
}

extern "C" {

int egm_fanout_device(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len, uint32_t n,
                      void* hip_stream,
                      uint64_t* d_drow, uint32_t* d_fid, uint32_t* d_sub, uint64_t cap) {
  if (!c || !d_mrow || !d_drow) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = (hipStream_t)hip_stream;   // NULL: the HIP default (null) stream, as the caller's own work
  return run_fanout(c, d_mrow, d_mids, mids_len, n, s, d_drow, d_fid, d_sub, cap, nullptr);
}

int egm_fanout_device_compact(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len,
                              uint32_t n, void* hip_stream, uint64_t* d_drow, uint64_t* d_entry_pos, uint32_t* d_sub,
                              uint64_t cap) {
  if (!c || !d_mrow || !d_drow || !d_entry_pos) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = (hipStream_t)hip_stream;   // NULL: the HIP default (null) stream, as the caller's own work
  return run_fanout(c, d_mrow, d_mids, mids_len, n, s, d_drow, nullptr, d_sub, cap, nullptr, d_entry_pos);
}

int egm_fanout_batch(egm_ctx* c, const egm_result* m, egm_delivery** out) {
  if (!c || !m || !out) return EGM_E_INVAL;
  *out = nullptr;
  if (!m->row_ptr || (m->n_ids && !m->ids))   // a packed result (EGM_RESULT_PACKED) is not taken here
    return c->fail(EGM_E_INVAL, "egm_fanout_batch takes the plain result form (match without EGM_RESULT_PACKED)");
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = c->stream;
  const uint32_t n = m->n_topics;
  const uint64_t nids = m->row_ptr[n];
  hipError_t e;
  if ((e = c->fan.mrow.ensure(((uint64_t)n + 1) * 8)) != hipSuccess) return c->hip_fail(e, "f_mrow");
  if ((e = c->fan.mids.ensure(nids * 4 + 16)) != hipSuccess) return c->hip_fail(e, "f_mids");
  if ((e = hipMemcpyAsync(c->fan.mrow.p, m->row_ptr, ((uint64_t)n + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c->hip_fail(e, "H2D match rows");
  if (nids && (e = hipMemcpyAsync(c->fan.mids.p, m->ids, nids * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return c->hip_fail(e, "H2D match ids");
  uint64_t cap = nids * 2 + 1024, total = 0;
  if ((e = c->fan.drow.ensure(((uint64_t)n + 1) * 8)) != hipSuccess) return c->hip_fail(e, "f_drow");
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((e = c->fan.dfid.ensure(cap * 4)) != hipSuccess) return c->hip_fail(e, "f_dfid");
    if ((e = c->fan.dsub.ensure(cap * 4)) != hipSuccess) return c->hip_fail(e, "f_dsub");
    int r = run_fanout(c, c->fan.mrow.as<uint64_t>(), c->fan.mids.as<uint32_t>(), nids, n, s, c->fan.drow.as<uint64_t>(),
                       c->fan.dfid.as<uint32_t>(), c->fan.dsub.as<uint32_t>(), cap, &total);
    if (r == EGM_OK) break;
    if (r != EGM_E_OVERFLOW || attempt == 1) return r;
    cap = total + 1024;
  }
  size_t sz = sizeof(egm_delivery);
  size_t o_row = sz;
  sz += ((uint64_t)n + 1) * 8;
  size_t o_fid = sz;
  sz += (total * 4 + 7) & ~7ull;
  size_t o_sub = sz;
  sz += (total * 4 + 7) & ~7ull;
  uint8_t* mem = (uint8_t*)result_alloc(sz);
  if (!mem) return c->fail(EGM_E_NOMEM, "delivery");
  egm_delivery* d = (egm_delivery*)mem;
  d->n_topics = n;
  d->n_deliveries = total;
  d->row_ptr = (uint64_t*)(mem + o_row);
  d->fid = (uint32_t*)(mem + o_fid);
  d->sub = (uint32_t*)(mem + o_sub);
  if ((e = hipMemcpy(d->row_ptr, c->fan.drow.p, ((uint64_t)n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (total && (e = hipMemcpy(d->fid, c->fan.dfid.p, total * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
      (total && (e = hipMemcpy(d->sub, c->fan.dsub.p, total * 4, hipMemcpyDeviceToHost)) != hipSuccess)) {
    result_discard(mem);
    return c->hip_fail(e, "D2H deliveries");
  }
  *out = d;
  return EGM_OK;
}

int egm_last_fanout(egm_ctx* c, uint64_t* n_deliveries, uint32_t* overflow) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (!c->fan.last_drow) return c->fail(EGM_E_STATE, "no fan-out launched");
  if (set_device(c)) return EGM_E_DEVICE;
  uint64_t tot = 0;
  unsigned int ovf = 0;
  hipError_t e;
  if ((e = hipStreamSynchronize(c->fan.last_stream)) != hipSuccess ||
      (e = hipMemcpy(&tot, c->fan.last_drow + c->fan.last_topics, 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(&ovf, c->fan.ovf.p, 4, hipMemcpyDeviceToHost)) != hipSuccess)
    return c->hip_fail(e, "fan-out readback");
  if (n_deliveries) *n_deliveries = tot;
  if (overflow) *overflow = ovf;
  return EGM_OK;
}

}  // extern "C"
