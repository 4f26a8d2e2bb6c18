// egm_ctx.h — the context behind the C-ABI (include/emqx_gpu_match.h) and what
// its translation units share.  One egm_ctx holds the state of every
// subsystem, grouped by owner:
//   egm_capi.cpp    open/close, the staged host table, the two-slot commit
//   egm_match.cpp   match workspaces, the device match entries, egm_last_*
//   egm_pipe.cpp    the host pipeline (egm_match_submit / _wait / _batch)
//   egm_fanout.cpp  the subscriber table and the fan-out
//   egm_dispatch.cpp the dead bitmap, the share table and the dispatch
//   egm_route.cpp   the route-node table and the forward pass
//   egm_part.cpp    shard merge, prefix partition, the host-only image API
// Everything here is internal to the library (hidden visibility).
#pragma once
#include <hip/hip_runtime_api.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/emqx_gpu_match.h"
#include "egm_alloc.h"
#include "egm_buf.h"
#include "egm_kernels.h"
#include "egm_route.h"
#include "egm_table.h"

#pragma GCC visibility push(hidden)
namespace egm {

// The last reading launch per stream of device memory that a commit rewrites:
// note() after each reading launch, drain() before the memory is written.
struct StreamUses {
  std::vector<std::pair<hipStream_t, hipEvent_t>> v;
  void note(hipStream_t s) {
    for (auto& p : v)
      if (p.first == s) {
        hipEventRecord(p.second, s);
        return;
      }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return;
    hipEventRecord(e, s);
    v.push_back({s, e});
  }
  void drain() {
    for (auto& p : v) {
      hipEventSynchronize(p.second);
      hipEventDestroy(p.second);
    }
    v.clear();
  }
};

// One batch of the host pipeline (egm_match_submit / egm_match_wait): its
// pinned input copy, device input and output, and the pinned result the
// caller reads until egm_result_free.
struct PipeSlot {
  bool busy = false;       // submitted, not yet waited for
  bool waiting = false;    // a thread is in egm_match_wait for it
  bool held = false;       // its result is with the caller
  bool sync = false;       // taken by egm_match_batch (not a ticket of egm_match_submit)
  bool abandoned = false;  // egm_match_cancel: reclaimed once its batch has finished
  uint32_t gen = 0;        // bumped at every submit: part of the ticket, so a stale ticket is refused
  uint32_t n = 0;
  int mode = 0;
  bool want_packed = false;   // submitted with EGM_RESULT_PACKED
  bool packed = false;        // this launch's result is packed (egm_pack.h): row32 + 3-byte ids
  uint64_t bytes = 0, maxlen = 0, cap = 0;
  uint64_t o_off = 0;      // the offsets' place after the blob in h_in and d_in (one H2D copy)
  PinBuf h_in, h_out, h_stats;
  DevBuf d_in, d_row, d_ids, d_flags, d_row32, d_pk;
  // ev_in: staged input copied in; ev_match: matched (stream s); ev_done: the
  // CSR in h_out (the copier's D2H copies, or the copy-out kernel)
  hipEvent_t ev_in = nullptr, ev_match = nullptr, ev_done = nullptr;
  uint64_t epoch = 0;
  // launches of this slot / of them, how many the copier has enqueued the
  // D2H of (ev_done is recorded for launch k once copied_gen == k; guarded by
  // egm_ctx::pipe.cq_mu)
  uint64_t launch_gen = 0, copied_gen = 0;
  bool copy_failed = false;   // the copier's DMA reported an error (guarded by cq_mu)
  ~PipeSlot() {
    if (ev_in) hipEventDestroy(ev_in);
    if (ev_match) hipEventDestroy(ev_match);
    if (ev_done) hipEventDestroy(ev_done);
  }
};

// Layout of a pipeline result in the slot's pinned buffer (h_out): header,
// egm_result, then row_ptr, ids (room for `cap`), flags, counts — each 16-B
// aligned, as the copy-out kernel writes them.
struct OutLayout {
  size_t o_res, o_row, o_ids, o_fl, o_cnt, total;
};
inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
inline OutLayout out_layout(uint64_t n, uint64_t cap) {
  OutLayout o;
  o.o_res = sizeof(ResultHdr);
  o.o_row = al16(o.o_res + sizeof(egm_result));
  o.o_ids = al16(o.o_row + (n + 1) * 8);
  o.o_fl = al16(o.o_ids + cap * 4);
  o.o_cnt = al16(o.o_fl + n);
  o.total = o.o_cnt + n * 4 + 16;
  return o;
}

// One match workspace: the per-batch scratch of launch_match.
struct MatchWs {
  DevBuf wid, lv, tfl, cnt, ids_tmp, pieces, deferred, heavy_stack, tile_sums, stats;
  DevBuf skey, skey_out, sval, order, wfix, sort_tmp;   // walk-order sort
  DevBuf rec, chunks, dir;                               // flush records, per-chunk chains and directories
  uint64_t pieces_cap = 0, ids_tmp_cap = 0, rec_cap = 0;
  uint32_t rec_grain = REC_GRAIN, flush_lim = 0;
  uint32_t heavy_cap = 0;        // stack items per heavy wave
  uint64_t blob_bytes = 0;       // topic bytes of the batch it was last sized for (k_tokenise's LDS shape)
  hipEvent_t ev = nullptr;       // recorded after its last batch
  hipStream_t stream = nullptr;  // stream of its last batch
  uint64_t used = 0;             // LRU clock
  ~MatchWs() {
    if (ev) hipEventDestroy(ev);
  }
};
constexpr uint32_t MATCH_WORKSPACES = 2;

// One device copy of the table image.  Two slots alternate: a commit writes
// the slot that is NOT current, so batches still reading the current epoch are
// never disturbed, and it brings that slot up to date with the records the
// host changed since the slot was last written (its pending log + this
// commit's) instead of re-uploading the whole image.
struct Slot {
  DevBuf nodes, hash_child, edges, dict, dict_blob, dict_off;
  uint64_t n_nodes = 0, n_hc = 0, n_edges = 0, n_dict = 0, n_blob = 0, n_off = 0;   // elements held
  bool valid = false;
  DirtyLog pending;   // host changes not yet applied here
  StreamUses uses;    // the queued launches that read it
  uint64_t bytes() const {
    return nodes.cap + hash_child.cap + edges.cap + dict.cap + dict_blob.cap + dict_off.cap;
  }
};

// The subscriber table of the fan-out (emqx_subscriber, emqx_broker.erl:144-197,
// 331-345), kept incrementally: the authoritative lists on the host (the CSR
// of the last full build + the lists changed since), and on the device the
// entries (sub_ids: the build's rows, then every changed row appended) and
// two copies of the per-filter records the fan-out reads (k_sub_pairs'
// layout).  A commit appends the changed rows past the entries any reader
// can reach, patches them into the record copy no reader uses (after its
// last readers finished) and makes it current — the table's two-slot epoch
// scheme (egm_table_commit) for the subscriber side.
struct SubsState {
  bool built = false;
  std::vector<uint64_t> row;                                  // the last full build's CSR
  std::vector<uint32_t> subs;
  std::unordered_map<uint32_t, std::vector<uint32_t>> lists;  // filters changed since that build
  std::unordered_map<uint32_t, uint4> recs;                   // their current records
  std::vector<uint32_t> pending;                              // changed since the last commit
  std::vector<uint32_t> stale[2];                             // records a copy lacks (changed since it was written)
  uint64_t tail = 0, garbage = 0;                             // device entries in use / superseded
  int cur = 0;                                                // the record copy the fan-out reads
  StreamUses uses[2];                                         // the queued fan-outs that read each copy
  uint64_t epoch = 0;
  uint64_t last_appended = 0, last_patched = 0;
  bool last_rebuilt = false;
};

struct Epoch {
  DevTable view{};
  int slot = 0;
  uint64_t id = 0;
  uint64_t n_filters = 0, n_nodes = 0, n_edges = 0, n_words = 0, bytes = 0;
  uint64_t fid_end = 0;   // every filter id of the epoch is below this (packed results: < 2^24)
};

struct CommitStats {
  uint64_t h2d = 0, d2d = 0, patched = 0;
  double ms = 0;
};

// Kernel times of the walk and the fan-out (egm_set_timing): each timed launch
// records a pair of events; the pairs are read and recycled at the next drain.
struct Timing {
  struct Series {
    std::vector<hipEvent_t> ev;   // pairs
    double ms = 0;
    uint64_t n = 0;
  };
  bool on = false;
  Series walk, fan, disp, fwd;   // disp: the dispatch's resolve pass alone; fwd: the forward pass
  std::vector<hipEvent_t> ev_free;
  hipEvent_t take_event() {
    if (!ev_free.empty()) {
      hipEvent_t e = ev_free.back();
      ev_free.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
  }
  // The pair for one launch, or null when timing is off; push it after the launch.
  hipEvent_t* take_pair(hipEvent_t (&evp)[2]) {
    if (!on) return nullptr;
    evp[0] = take_event();
    evp[1] = take_event();
    return evp;
  }
  void push_pair(Series& s, const hipEvent_t* evp) {
    if (!evp) return;
    s.ev.push_back(evp[0]);
    s.ev.push_back(evp[1]);
  }
  void drain(Series& s) {
    for (size_t i = 0; i + 1 < s.ev.size(); i += 2) {
      float ms = 0;
      hipEventSynchronize(s.ev[i + 1]);
      hipEventElapsedTime(&ms, s.ev[i], s.ev[i + 1]);
      s.ms += ms;
      ++s.n;
      ev_free.push_back(s.ev[i]);
      ev_free.push_back(s.ev[i + 1]);
    }
    s.ev.clear();
  }
  void drain() {
    drain(walk);
    drain(fan);
    drain(disp);
    drain(fwd);
  }
};

// Shard merge and prefix partition routing (egm_part.cpp).
struct PartState {
  DevBuf m_srow, m_tiles, m_tot;   // merge
  DevBuf p_ctr, p_dst;             // prefix routes
};

// Dispatch on the device (egm_dispatch.cpp): the liveness bitmap
// (is_process_alive, emqx_broker.erl:297-302) and the $share member table
// (emqx_shared_sub's ?TAB).  The host keeps both authoritative; a share commit
// rebuilds the device table into the copy no dispatch in flight reads (the
// subscriber commit's two-copy scheme).  rr / sticky are indexed by a key's
// slot, assigned once per key and never reused, and survive commits.
struct ShareKey {
  uint32_t slot = 0;
  std::vector<uint32_t> members;   // in the order given
};
struct ShareCopy {
  DevBuf hash, members, cnt;
  uint32_t n_buckets = 0;
};
struct DispState {
  // dead bitmap
  std::vector<uint32_t> dead_host;   // the words, as on the device
  DevBuf dead;
  uint64_t dead_words = 0;           // words valid on the device
  // share table
  std::unordered_map<uint64_t, ShareKey> keys;   // fid << 32 | group
  uint32_t next_slot = 0;
  ShareCopy copy[2];
  int cur = 0;
  StreamUses uses[2];                // the queued dispatches that read each copy (and the bitmap, rr, sticky)
  DevBuf rr, sticky;
  uint32_t slot_cap = 0;             // entries of rr / sticky
  uint64_t epoch = 0;
  // the last dispatch (egm_last_dispatch)
  DevBuf stats, mkey, epos, elive, eshared;
  uint64_t seq = 0;                  // dispatches launched: the random pick's sequence number
  hipStream_t last_stream = nullptr;
  bool launched = false;
};

// Cluster routes (egm_route.cpp): the route-node table — the emqx_route bag
// restricted to atom dests (emqx_router.erl:114-125), one 64-bit node mask per
// filter id — and the forward pass's workspaces.  The host mirror is
// authoritative; a commit patches the changed masks into the device copy no
// forward pass in flight reads and makes it current (the subscriber commit's
// two-copy scheme).  A node drop rewrites one copy in a streaming pass; the
// other copy gets the same pass when it next becomes the commit's target.
struct RouteState {
  bool built = false;
  uint32_t self_node = 0;
  uint32_t n_nodes = 0;                 // largest node id ever set + 1
  uint32_t n_fid_slots = 0;             // masks of each device copy
  std::vector<uint64_t> mask;           // host mirror (longer than the device copies until a commit uploads it)
  std::vector<uint32_t> pending;        // filter ids changed since the last commit
  std::vector<uint32_t> stale[2];       // masks a copy lacks (changed since it was written)
  std::vector<uint32_t> drops[2];       // node drops a copy lacks
  DevBuf copy[2];
  int cur = 0;                          // the copy the forward pass reads
  StreamUses uses[2];                   // the queued forward passes that read each copy
  uint64_t epoch = 0, last_patched = 0;
  bool last_rebuilt = false;
  DevBuf drop_out, drop_n;              // egm_routes_drop_node's emptied list
  // the forward pass
  DevBuf tile_cnt, tile_base, tile_sums, state;
  DevBuf mrow, mids, nrow, ftopic, ffid, efwd, tfwd;   // egm_forward_batch
  hipStream_t last_stream = nullptr;
  bool launched = false;
};

// Subscriber table and fan-out (egm_fanout.cpp).
struct FanState {
  DevBuf sub_row, sub_rp, sub_rp2, sub_ids, dc, ds0, dpos, wbase, tiles, ovf, mrow, mids, drow, dfid, dsub;
  uint32_t n_fid_slots = 0;
  SubsState subs;
  DevBuf& sub_rec(int k) { return k ? sub_rp2 : sub_rp; }
  // the last fan-out (egm_last_fanout)
  const uint64_t* last_drow = nullptr;
  uint32_t last_topics = 0;
  hipStream_t last_stream = nullptr;
};

// Host pipeline (egm_pipe.cpp).
struct PipeState {
  std::vector<std::unique_ptr<PipeSlot>> slots;
  std::condition_variable_any cv;    // a slot was freed (wait done, result freed, ticket cancelled)
  std::mutex cancel_mu;              // guards cancel_q only (never held across another lock)
  std::vector<uint64_t> cancel_q;    // cancels that found the context busy (egm_match_cancel)
  hipStream_t copy_stream = nullptr;   // host->device copies
  hipStream_t d2h_stream = nullptr;    // device->host copies (PCIe is full duplex)
  hipStream_t d2h_stream2 = nullptr;   // ... the second half of the ids
  hipStream_t small_streams[MATCH_WORKSPACES] = {};   // small batches, round robin: they run side by side
  uint32_t small_rr = 0;
  // The copier thread (round 4): it waits for each launched batch's match
  // (ev_match; the stats, copied before it in stream order, hold the exact id
  // total) and enqueues the result's D2H as DMA copies of exactly that size.
  // A copy-out kernel storing to pinned memory instead (EGM_PIPE_COPY=kernel)
  // stalls the next batch's memory-bound kernels behind the PCIe writes
  // (k_tokenise 0.1 -> 1-2 ms beside it, profiles/r4_host_trace.json).
  std::thread copier;
  std::mutex cq_mu;                    // guards cq, cq_stop and every slot's launch/copied gens
  std::condition_variable cq_cv;       // work for the copier
  std::condition_variable copied_cv;   // a slot's D2H was enqueued
  std::vector<std::pair<PipeSlot*, uint64_t>> cq;
  bool cq_stop = false;
  uint64_t cap_hint = 0;   // ids room a batch needed (overflow reruns): new slots start there
};

}  // namespace egm

// egm_ctx itself keeps the default visibility of its declaration in the public
// header (a hidden type in their signatures would hide the entry points), so
// GCC notes that its fields' types are more hidden than it is: intended, the
// struct is opaque to callers.
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wattributes"
struct egm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::recursive_mutex mu;
  std::string err;
  uint32_t debug = 0;

  // ---- the table and its commit (egm_capi.cpp)
  egm::HostTable table;
  std::shared_ptr<egm::Epoch> cur;
  uint64_t next_epoch = 1;
  egm::Slot slots[2];
  int cur_slot = -1;
  egm::PinBuf patch_host;   // pinned staging of patch records (the subscriber commit's too)
  egm::DevBuf patch_dev;
  egm::CommitStats last_commit;

  // ---- match (egm_match.cpp)
  // per-batch match workspaces: batches on different streams get different
  // ones, so consecutive batches overlap (one's compaction with the next one's
  // walk); a workspace reused from another stream waits for its last batch
  egm::MatchWs ws[egm::MATCH_WORKSPACES];
  uint32_t cur_ws = 0;           // workspace of the last batch (egm_last_stats)
  uint64_t ws_clock = 0;
  uint32_t heavy_waves = 64;     // waves of the heavy kernel (rare path; each owns an HBM stack)
  egm::MatchStats last{};
  bool last_pending = false;
  hipStream_t last_stream = nullptr;
  // the last match launch's walk order, for a fan-out of the same rows (k_fan_count_ord)
  struct {
    const uint64_t* order = nullptr;   // null: that batch was walked in input order
    const uint64_t* row = nullptr;
    uint32_t n = 0, ws = 0;
  } last_walk;

  egm::PartState part;   // shard merge and prefix partition routing (egm_part.cpp)
  egm::FanState fan;     // subscriber table and fan-out (egm_fanout.cpp)
  egm::DispState disp;   // dead bitmap, share table and dispatch (egm_dispatch.cpp)
  egm::RouteState route; // route-node table and forward pass (egm_route.cpp)
  egm::Timing timing;

  // The per-context workspaces (fan-out, merge, routes) are shared by every
  // launch, whatever stream the caller gives: a launch on a new stream first
  // waits for the last launch that used them (one event, recorded after each).
  hipEvent_t work_ev = nullptr;
  hipStream_t work_stream = nullptr;
  bool work_used = false;   // (the null stream is a stream: work_stream may be 0 after a launch)
  void work_begin(hipStream_t s) {
    if (work_used && work_stream != s && work_ev) hipStreamWaitEvent(s, work_ev, 0);
  }
  void work_end(hipStream_t s) {
    if (!work_ev && hipEventCreateWithFlags(&work_ev, hipEventDisableTiming) != hipSuccess) work_ev = nullptr;
    if (work_ev) hipEventRecord(work_ev, s);
    work_stream = s;
    work_used = true;
  }

  egm::PipeState pipe;   // host pipeline (egm_pipe.cpp)

  // (hidden like the types above: an outlined constructor is no dynamic symbol)
  __attribute__((visibility("hidden"))) egm_ctx() = default;
  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
  int hip_fail(hipError_t e, const char* where) {
    err = std::string(where) + ": " + hipGetErrorString(e);
    return EGM_E_DEVICE;
  }
};
#pragma GCC diagnostic pop

namespace egm {

inline int set_device(egm_ctx* c) {
  hipError_t e = hipSetDevice(c->device);
  return e == hipSuccess ? 0 : c->hip_fail(e, "hipSetDevice");
}

inline bool valid_offsets(const uint32_t* off, uint32_t n) {
  if (!off) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

// A host allocation failure inside an entry point is reported, never thrown
// across the C ABI (a std::bad_alloc escaping an extern "C" function would
// terminate the embedding BEAM node).
template <class F>
inline int no_throw(egm_ctx* c, const char* what, F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return c->fail(EGM_E_NOMEM, what);
  } catch (const std::exception& ex) {
    return c->fail(EGM_E_DEVICE, ex.what());
  }
}

// fn(lo, hi) over [0, n) on up to 8 threads, `grain` items or more each
// (the host side of a 1M-topic batch: one core stages ~10 GB/s into pinned
// memory, the PCIe link takes ~50; round 3 copied a 39 MB batch on one core).
// (static, par_copy too: the std::thread instantiations over their lambdas
// then stay internal to each unit instead of becoming dynamic symbols)
template <class F>
static void par_for(size_t n, size_t grain, F fn) {
  const unsigned nt = (unsigned)std::min<size_t>(8, std::max<size_t>(1, n / std::max<size_t>(grain, 1)));
  if (nt <= 1) {
    fn((size_t)0, n);
    return;
  }
  std::vector<std::thread> th;
  const size_t per = (n + nt - 1) / nt;
  for (unsigned k = 1; k < nt; ++k) {
    const size_t lo = k * per, hi = std::min(n, lo + per);
    if (lo < hi) th.emplace_back([=] { fn(lo, hi); });
  }
  fn((size_t)0, std::min(n, per));
  for (auto& x : th) x.join();
}

static inline void par_copy(void* dst, const void* src, size_t bytes) {
  par_for(bytes, 4u << 20, [=](size_t lo, size_t hi) { memcpy((uint8_t*)dst + lo, (const uint8_t*)src + lo, hi - lo); });
}

// ---- what crosses the units
// egm_capi.cpp
void sort_unique(std::vector<uint32_t>& v, uint64_t size = 0);
bool validate_inserts(const HostTable& t, const uint8_t* blob, const uint32_t* off, uint32_t n, const uint32_t* ids,
                      bool from_empty, std::string* why);
uint8_t* patch_stage(egm_ctx* c, size_t bytes);
// egm_match.cpp
MatchWs& pick_ws(egm_ctx* c, hipStream_t s);
int ensure_work(egm_ctx* c, MatchWs& W, uint32_t n, uint64_t blob_bytes, uint64_t ids_cap, uint64_t max_levels);
int run_match(egm_ctx* c, MatchWs& W, const Epoch& ep, const uint8_t* d_blob, const uint32_t* d_off, uint32_t n,
              int mode, hipStream_t s, uint64_t* d_row, uint32_t* d_ids, uint64_t ids_cap,
              const uint32_t* d_n_live = nullptr, uint32_t* d_topic = nullptr);
void ws_done(MatchWs& W, hipStream_t s);
// egm_fanout.cpp: the fan-out of a device match CSR; with `da` the compact form followed by the dispatch's resolve pass
int run_fanout(egm_ctx* c, const uint64_t* d_mrow, const uint32_t* d_mids, uint64_t mids_len, uint32_t n, hipStream_t s,
               uint64_t* d_drow, uint32_t* d_fid, uint32_t* d_sub, uint64_t cap, uint64_t* total,
               uint64_t* d_entry_pos = nullptr, const DispArgs* da = nullptr);

}  // namespace egm
#pragma GCC visibility pop
