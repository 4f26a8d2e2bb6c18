// egm_capi.cpp — the C-ABI of libemqx_gpu_match.so (include/emqx_gpu_match.h).
//
// Owns: one HIP stream per context, the staged host table (egm_table.cpp),
// the committed device epochs (double-buffered through shared_ptr so a batch
// in flight keeps the epoch it started with — the race-free analogue of the
// reference's mnesia transactions around emqx_trie:insert/delete,
// apps/emqx/src/emqx_router.erl:252-303).  This file: open/close, the table
// entries and the commit, the plain getters and setters.  The match entries
// are in egm_match.cpp, the host pipeline in egm_pipe.cpp, the fan-out in
// egm_fanout.cpp, merge/partition/image in egm_part.cpp (state: egm_ctx.h).
#include <stdlib.h>

#include <chrono>
#include <unordered_set>

#include "egm_ctx.h"

using namespace egm;

// Sorted, unique indices.  Large logs go through a bitmap over the array
// (O(n + size/64)) rather than a sort.
void egm::sort_unique(std::vector<uint32_t>& v, uint64_t size) {
  if (v.size() < 8192 || size == 0 || size > (1ull << 32)) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return;
  }
  std::vector<uint64_t> bits((size + 63) / 64, 0);
  for (uint32_t i : v)
    if (i < size) bits[i >> 6] |= 1ull << (i & 63);
  v.clear();
  for (uint64_t w = 0; w < bits.size(); ++w)
    for (uint64_t b = bits[w]; b; b &= b - 1) v.push_back((uint32_t)(w * 64 + __builtin_ctzll(b)));
}

// out[i] = rec[idx[i]] for records of R bytes; the records are random reads
// of a multi-GB host image, so large patches use several threads.
template <size_t R>
static void gather(uint8_t* out, const void* rec, const std::vector<uint32_t>& idx) {
  const uint8_t* base = (const uint8_t*)rec;
  auto work = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) memcpy(out + i * R, base + (size_t)idx[i] * R, R);
  };
  const size_t n = idx.size();
  unsigned nt = std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  if (n < 65536 || nt == 1) {
    work(0, n);
    return;
  }
  std::vector<std::thread> th;
  const size_t per = (n + nt - 1) / nt;
  for (unsigned k = 0; k < nt; ++k) {
    size_t lo = k * per, hi = std::min(n, lo + per);
    if (lo < hi) th.emplace_back(work, lo, hi);
  }
  for (auto& x : th) x.join();
}

// Bring one array of slot `dst` to the host image.  Preference order:
//  1. patch in place: the slot holds the image minus `need` (its pending log
//     plus this commit's), and it is big enough;
//  2. device copy from the current slot (which lacks only this commit's
//     changes `d`) followed by a patch of `d` — the slot was stale or too
//     small, the changes were not a rebuild;
//  3. whole upload from the host (rebuild: relayout, rehash, clear).
// Returns the indices still to patch in *idx (sorted, unique).
template <class T>
static int sync_array(egm_ctx* c, DevBuf& dst, uint64_t& held, const DevBuf* src, uint64_t src_held,
                      const std::vector<T>& host, bool need_full, bool d_full, const std::vector<uint32_t>& need,
                      const std::vector<uint32_t>& d, uint64_t headroom, std::vector<uint32_t>* idx,
                      const char* what) {
  const uint64_t n = host.size(), sz = sizeof(T);
  hipStream_t s = c->stream;
  hipError_t e;
  idx->clear();
  if (!need_full && held <= n && n * sz <= dst.cap && dst.p) {
    *idx = need;
  } else if (!d_full && src && src->p && src_held <= n) {
    if ((e = dst.ensure((n + headroom) * sz)) != hipSuccess) return c->hip_fail(e, what);
    if (src_held && (e = hipMemcpyAsync(dst.p, src->p, src_held * sz, hipMemcpyDeviceToDevice, s)) != hipSuccess)
      return c->hip_fail(e, what);
    c->last_commit.d2d += src_held * sz;
    *idx = d;
    for (uint64_t i = src_held; i < n; ++i) idx->push_back((uint32_t)i);   // appended beyond the copy
  } else {
    if ((e = dst.ensure((n + headroom) * sz + 16)) != hipSuccess) return c->hip_fail(e, what);
    if (n && (e = hipMemcpyAsync(dst.p, host.data(), n * sz, hipMemcpyHostToDevice, s)) != hipSuccess)
      return c->hip_fail(e, what);
    c->last_commit.h2d += n * sz;
  }
  sort_unique(*idx, n);
  while (!idx->empty() && idx->back() >= n) idx->pop_back();
  held = n;
  return EGM_OK;
}

// Append-only arrays (dictionary words and their offsets): upload the tail.
template <class T>
static int sync_tail(egm_ctx* c, DevBuf& dst, uint64_t& held, const DevBuf* src, uint64_t src_held,
                     const std::vector<T>& host, bool need_full, bool d_full, const char* what) {
  const uint64_t n = host.size(), sz = sizeof(T);
  hipStream_t s = c->stream;
  hipError_t e;
  uint64_t from;
  if (!need_full && held <= n && n * sz <= dst.cap && dst.p) {
    from = held;
  } else if (!d_full && src && src->p && src_held <= n) {
    if ((e = dst.ensure(n * sz + n * sz / 4 + 4096)) != hipSuccess) return c->hip_fail(e, what);
    if (src_held && (e = hipMemcpyAsync(dst.p, src->p, src_held * sz, hipMemcpyDeviceToDevice, s)) != hipSuccess)
      return c->hip_fail(e, what);
    c->last_commit.d2d += src_held * sz;
    from = src_held;
  } else {
    if ((e = dst.ensure(n * sz + n * sz / 4 + 4096)) != hipSuccess) return c->hip_fail(e, what);
    from = 0;
  }
  if (n > from) {
    if ((e = hipMemcpyAsync((uint8_t*)dst.p + from * sz, host.data() + from, (n - from) * sz,
                            hipMemcpyHostToDevice, s)) != hipSuccess)
      return c->hip_fail(e, what);
    c->last_commit.h2d += (n - from) * sz;
  }
  held = n;
  return EGM_OK;
}

// Pinned staging for `bytes` (> 0) of patch records, or null.
uint8_t* egm::patch_stage(egm_ctx* c, size_t bytes) {
  return c->patch_host.ensure(bytes, bytes + bytes / 2 + 65536) == hipSuccess ? (uint8_t*)c->patch_host.p : nullptr;
}

// Publish the host table as a new epoch (egm_table_commit).
static int commit_locked(egm_ctx* c, uint64_t* epoch) {
  auto t0 = std::chrono::steady_clock::now();
  c->last_commit = CommitStats{};
  const HostTable& t = c->table;
  DirtyLog d = c->table.take_dirty();
  // on any failure below, the changes go back into the table's log, so the
  // next commit publishes them (the half-written slot stays invalid)
  struct Restore {
    egm_ctx* c;
    const DirtyLog& d;
    bool armed = true;
    ~Restore() {
      if (armed) c->table.restore_dirty(d);
    }
  } restore{c, d};
  if (c->debug & EGM_DEBUG_FAIL_COMMIT) {   // test hook: a commit that fails after taking the log (one shot)
    c->debug &= ~EGM_DEBUG_FAIL_COMMIT;
    return c->fail(EGM_E_DEVICE, "commit: injected failure");
  }
  const int x = c->cur_slot < 0 ? 0 : 1 - c->cur_slot;
  Slot& S = c->slots[x];
  Slot* C = c->cur_slot < 0 ? nullptr : &c->slots[c->cur_slot];
  S.uses.drain();   // every queued launch that reads slot x: it is about to be written
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return c->hip_fail(e, "commit: stream");
  DirtyLog need = S.pending;
  need.merge(d);
  if (!S.valid) need.nodes_full = need.edges_full = need.dict_full = need.words_full = true;
  // a failure below leaves S half-written: it stays invalid (full copy next time)
  S.valid = false;
  const uint64_t nn = t.nodes.size();
  std::vector<uint32_t> in, ih, ie, id;
  int r;
  if ((r = sync_array(c, S.nodes, S.n_nodes, C ? &C->nodes : nullptr, C ? C->n_nodes : 0, t.nodes,
                      need.nodes_full, d.nodes_full, need.nodes, d.nodes, nn / 8 + 4096, &in, "nodes")) ||
      (r = sync_array(c, S.hash_child, S.n_hc, C ? &C->hash_child : nullptr, C ? C->n_hc : 0, t.hash_child,
                      need.nodes_full, d.nodes_full, need.nodes, d.nodes, nn / 8 + 4096, &ih, "hash_child")) ||
      (r = sync_array(c, S.edges, S.n_edges, C ? &C->edges : nullptr, C ? C->n_edges : 0, t.edges,
                      need.edges_full, d.edges_full, need.edges, d.edges, 0, &ie, "edges")) ||
      (r = sync_array(c, S.dict, S.n_dict, C ? &C->dict : nullptr, C ? C->n_dict : 0, t.dict, need.dict_full,
                      d.dict_full, need.dict, d.dict, 0, &id, "dict")) ||
      (r = sync_tail(c, S.dict_blob, S.n_blob, C ? &C->dict_blob : nullptr, C ? C->n_blob : 0, t.dict_blob,
                     need.words_full, d.words_full, "dict_blob")) ||
      (r = sync_tail(c, S.dict_off, S.n_off, C ? &C->dict_off : nullptr, C ? C->n_off : 0, t.dict_off,
                     need.words_full, d.words_full, "dict_off")))
    return r;
  // pack {indices, records} of all four patched arrays into one pinned buffer
  const size_t o_in = 0, o_rn = al16(o_in + in.size() * 4), o_ih = o_rn + in.size() * 16,
               o_rh = al16(o_ih + ih.size() * 4), o_ie = al16(o_rh + ih.size() * 4),
               o_re = al16(o_ie + ie.size() * 4), o_id = o_re + ie.size() * 32, o_rd = al16(o_id + id.size() * 4),
               total = o_rd + id.size() * 32;
  const uint64_t np = in.size() + ih.size() + ie.size() + id.size();
  if (np) {
    uint8_t* h = patch_stage(c, total);
    if (!h) return c->fail(EGM_E_NOMEM, "commit: pinned staging");
    memcpy(h + o_in, in.data(), in.size() * 4);
    memcpy(h + o_ih, ih.data(), ih.size() * 4);
    memcpy(h + o_ie, ie.data(), ie.size() * 4);
    memcpy(h + o_id, id.data(), id.size() * 4);
    gather<16>(h + o_rn, t.nodes.data(), in);
    gather<4>(h + o_rh, t.hash_child.data(), ih);
    gather<32>(h + o_re, t.edges.data(), ie);
    gather<32>(h + o_rd, t.dict.data(), id);
    if ((e = c->patch_dev.ensure(total)) != hipSuccess) return c->hip_fail(e, "commit: patch buffer");
    if ((e = hipMemcpyAsync(c->patch_dev.p, h, total, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
      return c->hip_fail(e, "commit: patch upload");
    c->last_commit.h2d += total;
    uint8_t* dp = (uint8_t*)c->patch_dev.p;
    if ((e = launch_patch(S.nodes.p, 16, (const uint32_t*)(dp + o_in), dp + o_rn, in.size(), c->stream)) ||
        (e = launch_patch(S.hash_child.p, 4, (const uint32_t*)(dp + o_ih), dp + o_rh, ih.size(), c->stream)) ||
        (e = launch_patch(S.edges.p, 32, (const uint32_t*)(dp + o_ie), dp + o_re, ie.size(), c->stream)) ||
        (e = launch_patch(S.dict.p, 32, (const uint32_t*)(dp + o_id), dp + o_rd, id.size(), c->stream)))
      return c->hip_fail(e, "commit: patch");
    c->last_commit.patched = np;
  }
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "commit: sync");
  restore.armed = false;
  S.valid = true;
  S.pending.clear();
  if (C) C->pending.merge(d);   // the previous epoch's slot now lacks this commit's changes

  auto ep = std::make_shared<Epoch>();
  ep->slot = x;
  ep->view.nodes = S.nodes.as<NodeRec>();
  ep->view.hash_child = S.hash_child.as<uint32_t>();
  ep->view.edges = S.edges.as<EdgeSlot>();
  ep->view.edge_mask = t.edge_mask();
  ep->view.dict = S.dict.as<DictSlot>();
  ep->view.dict_mask = t.dict_mask();
  ep->view.dict_blob = S.dict_blob.as<uint8_t>();
  ep->view.dict_off = S.dict_off.as<uint64_t>();
  ep->view.sig_packed = t.n_words() <= (1u << 27) ? 1u : 0u;
  ep->n_filters = t.n_filters();
  ep->n_nodes = t.n_nodes_live();
  ep->n_edges = t.n_edges();
  ep->n_words = t.n_words();
  ep->fid_end = t.next_fid();
  ep->bytes = S.bytes();
  ep->id = c->next_epoch++;
  c->cur = ep;
  c->cur_slot = x;
  if (epoch) *epoch = ep->id;
  c->last_commit.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return EGM_OK;
}

// Check a batch of inserts against the table before changing anything (the
// reference applies route changes in all-or-nothing mnesia transactions,
// emqx_router.erl:252-303): every new filter's id must be < WID_MAX, unused by
// a live filter (deletes of the same delta apply after the inserts) and not
// claimed twice in the batch.  Filters already present (or repeated in the
// batch) are idempotent no-ops (emqx_trie.erl:84-86).
bool egm::validate_inserts(const HostTable& t, const uint8_t* blob, const uint32_t* off, uint32_t n,
                           const uint32_t* ids, bool from_empty, std::string* why) {
  if (!ids) return true;   // ids assigned by the table
  std::unordered_set<std::string> seen_bytes;
  std::unordered_set<uint32_t> seen_ids;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* p = blob + off[i];
    const uint32_t len = off[i + 1] - off[i];
    std::string key((const char*)p, len);
    if (!from_empty && t.lookup(p, len) != NONE) continue;
    if (!seen_bytes.insert(key).second) continue;
    const uint32_t id = ids[i];
    if (id == NONE) continue;
    if (id >= WID_MAX || (!from_empty && t.id_in_use(id)) || !seen_ids.insert(id).second) {
      *why = "bad or duplicate filter id at index " + std::to_string(i);
      return false;
    }
  }
  return true;
}

// egm_table_build uses the parallel bulk build from EGM_BULK_MIN filters on
// (default 65 536; 0 = always), unless an id asks to be assigned (NONE).
static bool use_bulk_build(uint32_t n, const uint32_t* ids) {
  const char* e = getenv("EGM_BULK_MIN");
  const uint64_t lim = (e && *e) ? strtoull(e, nullptr, 10) : 65536;
  if (n < lim) return false;
  if (ids)
    for (uint32_t i = 0; i < n; ++i)
      if (ids[i] == NONE) return false;
  return true;
}

extern "C" {

const char* egm_version(void) { return "emqx_gpu_match 0.1 (gfx950)"; }

int egm_open(const egm_config* cfg, egm_ctx** out) {
  if (!out) return EGM_E_INVAL;
  *out = nullptr;
  egm_ctx* c = new (std::nothrow) egm_ctx();
  if (!c) return EGM_E_NOMEM;
  c->device = cfg ? cfg->device : 0;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= c->device || c->device < 0) {
    delete c;
    return EGM_E_DEVICE;
  }
  if (set_device(c) != 0 || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return EGM_E_DEVICE;
  }
  if (commit_locked(c, nullptr) != EGM_OK) {  // empty epoch
    hipStreamDestroy(c->stream);
    delete c;
    return EGM_E_DEVICE;
  }
  if (cfg && cfg->max_batch)
    ensure_work(c, c->ws[0], cfg->max_batch, (uint64_t)cfg->max_batch * 64, (uint64_t)cfg->max_batch * 4, 1024);
  *out = c;
  return EGM_OK;
}

void egm_close(egm_ctx* c) {
  if (!c) return;
  {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    set_device(c);
    hipStreamSynchronize(c->stream);
    c->timing.drain();
    for (hipEvent_t e : c->timing.ev_free) hipEventDestroy(e);
    c->cur.reset();
    c->slots[0].uses.drain();
    c->slots[1].uses.drain();
    c->patch_host.release();
    c->fan.subs.uses[0].drain();
    c->fan.subs.uses[1].drain();
    if (c->work_ev) hipEventDestroy(c->work_ev);
    c->work_ev = nullptr;
    if (c->pipe.copy_stream) hipStreamSynchronize(c->pipe.copy_stream);
  }
  auto& P = c->pipe;
  if (P.copier.joinable()) {   // outside the context lock: the copier never takes it
    {
      std::lock_guard<std::mutex> q(P.cq_mu);
      P.cq_stop = true;
    }
    P.cq_cv.notify_all();
    P.copier.join();
  }
  {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    set_device(c);
    if (P.d2h_stream) hipStreamSynchronize(P.d2h_stream);
    if (P.d2h_stream2) hipStreamSynchronize(P.d2h_stream2);
    for (auto& ss : P.small_streams)
      if (ss) {
        hipStreamSynchronize(ss);
        hipStreamDestroy(ss);
        ss = nullptr;
      }
    P.slots.clear();
    if (P.copy_stream) hipStreamDestroy(P.copy_stream);
    if (P.d2h_stream) hipStreamDestroy(P.d2h_stream);
    if (P.d2h_stream2) hipStreamDestroy(P.d2h_stream2);
    P.copy_stream = P.d2h_stream = P.d2h_stream2 = nullptr;
  }
  hipStreamDestroy(c->stream);
  delete c;
}

const char* egm_last_error(egm_ctx* c) { return c ? c->err.c_str() : "null context"; }

int egm_table_build(egm_ctx* c, const uint8_t* blob, const uint32_t* off, uint32_t n, const uint32_t* ids) {
  if (!c || (n && (!blob || !valid_offsets(off, n)))) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "table build: host allocation", [&] {
  std::string why;
  if (!validate_inserts(c->table, blob, off, n, ids, true, &why)) return c->fail(EGM_E_INVAL, why);
  if (use_bulk_build(n, ids)) {   // parallel: the same image as the insert loop below (egm_bulk.cpp)
    if (c->table.bulk_build(blob, off, n, ids, 0) < 0) {
      c->table.clear();
      return c->fail(EGM_E_INVAL, "table too large (node ids exhausted)");
    }
    return commit_locked(c, nullptr);
  }
  c->table.clear();
  for (uint32_t i = 0; i < n; ++i) {
    int r = c->table.insert(blob + off[i], off[i + 1] - off[i], ids ? ids[i] : i, nullptr);
    if (r < 0) return c->fail(EGM_E_INVAL, "bad or duplicate filter id at index " + std::to_string(i));
  }
  c->table.relayout();
  return commit_locked(c, nullptr);
  });
}

int egm_table_apply_delta(egm_ctx* c, const egm_delta* ins, const egm_delta* del) {
  if (!c) return EGM_E_INVAL;
  if (ins && ins->n && (!ins->blob || !valid_offsets(ins->offsets, ins->n))) return EGM_E_INVAL;
  if (del && del->n && (!del->blob || !valid_offsets(del->offsets, del->n))) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  return no_throw(c, "table delta: host allocation", [&] {
  std::string why;
  if (ins && !validate_inserts(c->table, ins->blob, ins->offsets, ins->n, ins->ids, false, &why))
    return c->fail(EGM_E_INVAL, why);   // nothing staged
  if (ins)
    for (uint32_t i = 0; i < ins->n; ++i) {
      int r = c->table.insert(ins->blob + ins->offsets[i], ins->offsets[i + 1] - ins->offsets[i],
                              ins->ids ? ins->ids[i] : NONE, nullptr);
      if (r < 0) return c->fail(EGM_E_INVAL, "bad or duplicate filter id at insert " + std::to_string(i));
    }
  if (del)
    for (uint32_t i = 0; i < del->n; ++i)
      c->table.remove(del->blob + del->offsets[i], del->offsets[i + 1] - del->offsets[i]);
  return EGM_OK;
  });
}

int egm_table_commit(egm_ctx* c, uint64_t* epoch) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  return no_throw(c, "table commit: host allocation", [&] { return commit_locked(c, epoch); });
}

int egm_table_epoch(egm_ctx* c, uint64_t* epoch) {
  if (!c || !epoch) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  *epoch = c->cur ? c->cur->id : 0;
  return EGM_OK;
}

int egm_table_empty(egm_ctx* c) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  return c->cur->n_filters == 0 ? 1 : 0;
}

int egm_table_stats(egm_ctx* c, uint64_t* nf, uint64_t* nn, uint64_t* ne, uint64_t* nw, uint64_t* bytes) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (nf) *nf = c->cur->n_filters;
  if (nn) *nn = c->cur->n_nodes;
  if (ne) *ne = c->cur->n_edges;
  if (nw) *nw = c->cur->n_words;
  if (bytes) *bytes = c->cur->bytes;
  return EGM_OK;
}

int egm_filter_id(egm_ctx* c, const uint8_t* f, uint32_t len, uint32_t* id) {
  if (!c || (!f && len) || !id) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  uint32_t r = c->table.lookup(f, len);
  if (r == NONE) return EGM_E_NOTFOUND;
  *id = r;
  return EGM_OK;
}

int egm_filter_bytes(egm_ctx* c, uint32_t id, const uint8_t** bytes, uint32_t* len) {
  if (!c || !bytes || !len) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  const uint8_t* p = c->table.filter_bytes(id, len);
  if (!p) return EGM_E_NOTFOUND;
  *bytes = p;
  return EGM_OK;
}

int egm_last_commit_stats(egm_ctx* c, uint64_t* h2d_bytes, uint64_t* d2d_bytes, uint64_t* patched,
                          double* ms) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (h2d_bytes) *h2d_bytes = c->last_commit.h2d;
  if (d2d_bytes) *d2d_bytes = c->last_commit.d2d;
  if (patched) *patched = c->last_commit.patched;
  if (ms) *ms = c->last_commit.ms;
  return EGM_OK;
}

int egm_set_debug(egm_ctx* c, uint32_t flags) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->debug = flags;
  return EGM_OK;
}

int egm_set_timing(egm_ctx* c, int enable) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  Timing& T = c->timing;
  T.drain();
  T.on = enable != 0;
  T.walk.ms = T.fan.ms = T.disp.ms = 0;
  T.walk.n = T.fan.n = T.disp.n = 0;
  return EGM_OK;
}

int egm_get_timing(egm_ctx* c, double* walk_ms, uint64_t* walk_n, double* fan_ms, uint64_t* fan_n) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  c->timing.drain();
  if (walk_ms) *walk_ms = c->timing.walk.ms;
  if (walk_n) *walk_n = c->timing.walk.n;
  if (fan_ms) *fan_ms = c->timing.fan.ms;
  if (fan_n) *fan_n = c->timing.fan.n;
  return EGM_OK;
}

uint64_t egm_word_hash(const uint8_t* p, uint32_t len) { return word_hash(p, len); }
uint32_t egm_edge_bucket(uint32_t parent, uint32_t w, uint32_t mask) { return edge_bucket(parent, w, mask); }

}  // extern "C"
