// egm_pipe.cpp — the host pipeline of the C-ABI: egm_match_submit stages a
// batch in a slot's pinned memory and enqueues its copy-in and match;
// egm_match_wait hands out the result in place (egm_result_free releases it);
// egm_match_batch is the two in one call.  Locks: the context lock (c->mu),
// then pipe.cq_mu (the copier thread's queue; the copier never takes c->mu);
// pipe.cancel_mu is held across no other lock.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>

#include "egm_ctx.h"
#include "egm_dma.h"
#include "egm_pack.h"

using namespace egm;

namespace {

constexpr size_t PIPE_MAX_SLOTS = 8;    // tickets of egm_match_submit busy or held at once
constexpr size_t PIPE_HARD_SLOTS = 16;   // all slots, egm_match_batch's included (then it waits); each
                                         // keeps buffers for the largest batch it saw (~ dirty schedulers)
constexpr int PIPE_BATCH_WAIT_MS = 30000;   // egm_match_batch's longest wait for a slot

// ticket = generation << 16 | (slot index + 1)
inline uint64_t make_ticket(size_t k, uint32_t gen) { return ((uint64_t)gen << 16) | (uint64_t)(k + 1); }
inline size_t ticket_slot(uint64_t t) { return (size_t)(t & 0xFFFFu) - 1; }
inline uint32_t ticket_gen(uint64_t t) { return (uint32_t)(t >> 16); }

}  // namespace

// How a pipeline result reaches pinned memory (EGM_PIPE_COPY, A/B):
//   dma (default) — the copier thread, SDMA engines through the HSA runtime
//   hip           — the copier thread, hipMemcpyAsync (a blit kernel here)
//   kernel        — a copy-out kernel on the d2h stream, sized on the device
enum { PIPE_DMA = 0, PIPE_HIP = 1, PIPE_KERNEL = 2 };
static int pipe_copy_mode() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("EGM_PIPE_COPY");
    v = (e && strcmp(e, "kernel") == 0) ? PIPE_KERNEL : (e && strcmp(e, "hip") == 0) ? PIPE_HIP : PIPE_DMA;
  }
  return v;
}
static bool pipe_copy_kernel() { return pipe_copy_mode() == PIPE_KERNEL; }
// EGM_PIPE_COPY set explicitly: every batch takes that copy (A/B), small ones too
static bool pipe_copy_forced() {
  static const bool v = getenv("EGM_PIPE_COPY") != nullptr;
  return v;
}
// Batches up to this many topics take the small-batch result path (pipe_launch).
constexpr uint64_t PIPE_SMALL_TOPICS = 16384;   // (65536 measured: the copy-out on the match's
                                                 // stream then costs more than the SDMA path's overlap)

// EGM_PIPE_TRACE=1: one stderr line per pipeline event with a ms clock
// (diagnostics of the host pipeline's bubbles).
static void ptrace(const char* what, const void* slot, uint64_t gen) {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("EGM_PIPE_TRACE");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  if (v != 1) return;
  static const auto t0 = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fprintf(stderr, "[pipe] %10.3f %-14s %p %llu\n", ms, what, slot, (unsigned long long)gen);
}

extern "C" {

// Enqueue one staged batch of slot S: H2D on the copy stream, the match on
// the context stream once the input is in, then the batch's flags and
// counters copied out in stream order (the next batch reuses the workspace).
static int pipe_launch(egm_ctx* c, PipeSlot& S) {
  hipError_t e;
  hipStream_t s = c->stream;
  const uint64_t n = S.n;
  const bool small = n <= PIPE_SMALL_TOPICS && !pipe_copy_forced();
  if (small) {
    // a small batch fills a fraction of the GPU: consecutive ones run side by
    // side, each on its own stream and workspace (pick_ws orders a workspace
    // last used on another stream after that use)
    hipStream_t& ss = c->pipe.small_streams[c->pipe.small_rr++ % MATCH_WORKSPACES];
    if (!ss && (e = hipStreamCreateWithFlags(&ss, hipStreamNonBlocking)) != hipSuccess)
      return c->hip_fail(e, "small-batch stream");
    s = ss;
  }
  std::shared_ptr<Epoch> ep = c->cur;
  S.epoch = ep->id;
  MatchWs& W = pick_ws(c, s);
  int r = ensure_work(c, W, S.n, S.bytes, S.cap, S.maxlen + 1);
  if (r) return r;
  if ((e = S.d_row.ensure((n + 1) * 8)) != hipSuccess) return c->hip_fail(e, "pipe row");
  if ((e = S.d_ids.ensure((S.cap + 4) * 4)) != hipSuccess) return c->hip_fail(e, "pipe ids");   // (+4: the packer reads groups of 4)
  if ((e = S.d_flags.ensure(n + 8)) != hipSuccess) return c->hip_fail(e, "pipe flags");
  if ((e = S.h_stats.ensure(sizeof(MatchStats))) != hipSuccess) return c->hip_fail(e, "pipe stats");
  const OutLayout ol = out_layout(n, S.cap);
  if ((e = S.h_out.ensure(ol.total)) != hipSuccess) return c->hip_fail(e, "pipe pinned result");
  if ((e = hipStreamWaitEvent(s, S.ev_in, 0)) != hipSuccess) return c->hip_fail(e, "pipe wait input");
  r = run_match(c, W, *ep, S.d_in.as<uint8_t>(), (const uint32_t*)(S.d_in.as<uint8_t>() + S.o_off), S.n, S.mode, s,
                S.d_row.as<uint64_t>(), S.d_ids.as<uint32_t>(), S.cap);
  if (r) {
    ws_done(W, s);
    return r;
  }
  c->last_pending = false;   // this batch's counters travel with the slot
  // the packed form (EGM_RESULT_PACKED, egm_pack.h): large batches on the copier's path whose
  // epoch's filter ids fit 24 bits; the packer runs on the match's stream, before ev_match
  S.packed = S.want_packed && !small && !pipe_copy_kernel() && ep->fid_end <= (1ull << 24) && S.cap < (1ull << 31);
  if (S.packed) {
    if ((e = S.d_row32.ensure((n + 1) * 4)) != hipSuccess || (e = S.d_pk.ensure(S.cap * 3 + 16)) != hipSuccess ||
        (e = launch_pack_result(S.d_row.as<uint64_t>(), (uint32_t)n, S.d_ids.as<uint32_t>(), S.cap,
                                S.d_row32.as<uint32_t>(), S.d_pk.as<uint8_t>(), s)) != hipSuccess) {
      ws_done(W, s);
      return c->hip_fail(e, "pipe pack");
    }
  }
  if (small) {
    // A small batch (the Erlang batcher's: 4096 by default) is latency-bound,
    // not bandwidth-bound: its result goes to pinned memory by a copy-out
    // kernel on the match's own stream — flags read from the workspace, the
    // counters too — so no D2D copy, no copier-thread hand-off and no SDMA
    // round trips (round 6: ~330 us -> see DESIGN §6 "small batches").
    uint8_t* h = (uint8_t*)S.h_out.p;
    if ((e = launch_copy_out(S.d_row.as<uint64_t>(), (uint32_t)n, S.d_ids.as<uint32_t>(), S.cap, W.tfl.as<uint8_t>(),
                             h + ol.o_row, h + ol.o_ids, h + ol.o_fl, s, W.stats.as<MatchStats>(),
                             (MatchStats*)S.h_stats.p)) != hipSuccess ||
        (e = hipEventRecord(S.ev_match, s)) != hipSuccess || (e = hipEventRecord(S.ev_done, s)) != hipSuccess) {
      ws_done(W, s);
      return c->hip_fail(e, "pipe copy-out (small batch)");
    }
    ws_done(W, s);
    std::lock_guard<std::mutex> q(c->pipe.cq_mu);
    S.copied_gen = ++S.launch_gen;
    return EGM_OK;
  }
  if ((n && (e = hipMemcpyAsync(S.d_flags.p, W.tfl.p, n, hipMemcpyDeviceToDevice, s)) != hipSuccess) ||
      (e = hipMemcpyAsync(S.h_stats.p, W.stats.p, sizeof(MatchStats), hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipEventRecord(S.ev_match, s)) != hipSuccess) {
    ws_done(W, s);
    return c->hip_fail(e, "pipe epilogue");
  }
  ws_done(W, s);
  if (pipe_copy_kernel()) {
    // the CSR straight into pinned memory by a kernel, sized on the device
    uint8_t* h = (uint8_t*)S.h_out.p;
    if ((e = hipStreamWaitEvent(c->pipe.d2h_stream, S.ev_match, 0)) != hipSuccess ||
        (e = launch_copy_out(S.d_row.as<uint64_t>(), (uint32_t)n, S.d_ids.as<uint32_t>(), S.cap,
                             S.d_flags.as<uint8_t>(), h + ol.o_row, h + ol.o_ids, h + ol.o_fl, c->pipe.d2h_stream)) !=
            hipSuccess ||
        (e = hipEventRecord(S.ev_done, c->pipe.d2h_stream)) != hipSuccess)
      return c->hip_fail(e, "pipe copy-out");
    std::lock_guard<std::mutex> q(c->pipe.cq_mu);
    S.copied_gen = ++S.launch_gen;
    return EGM_OK;
  }
  {   // the copier enqueues the D2H once the match is done
    std::lock_guard<std::mutex> q(c->pipe.cq_mu);
    c->pipe.cq.emplace_back(&S, ++S.launch_gen);
  }
  c->pipe.cq_cv.notify_one();
  return EGM_OK;
}

// The copier thread's loop (egm_ctx::copier): in launch order, wait for a
// batch's match, then enqueue its result's D2H — row_ptr and flags and the
// first half of the ids on one DMA stream, the second half on another (one
// stream alone measured 17-57 GB/s, two 56) — and record ev_done.  It never
// takes the context lock; a slot it holds is not reused before copied_gen
// reaches its launch (the waiter and the cancel path check it).
static void copier_main(egm_ctx* c) {
  hipSetDevice(c->device);
  hipEvent_t join = nullptr;
  hipEventCreateWithFlags(&join, hipEventDisableTiming);
  Dma* dma = pipe_copy_mode() == PIPE_DMA ? dma_open(c->device) : nullptr;   // null: hipMemcpyAsync
  for (;;) {
    std::pair<PipeSlot*, uint64_t> it;
    {
      std::unique_lock<std::mutex> q(c->pipe.cq_mu);
      c->pipe.cq_cv.wait(q, [&] { return c->pipe.cq_stop || !c->pipe.cq.empty(); });
      if (c->pipe.cq.empty()) break;   // stopping, nothing left
      it = c->pipe.cq.front();
      c->pipe.cq.erase(c->pipe.cq.begin());
    }
    PipeSlot& S = *it.first;
    ptrace("copier-take", &S, it.second);
    hipError_t e = hipEventSynchronize(S.ev_match);   // (a host-synchronised event: device writes released)
    ptrace("match-done", &S, it.second);
    const MatchStats st = *(const MatchStats*)S.h_stats.p;   // copied before ev_match, in stream order
    bool failed = e != hipSuccess;   // the match itself failed: nothing is copied, the waiter reports EGM_E_DEVICE
    if (e == hipSuccess && !st.overflow && !st.guard) {
      const uint64_t n = S.n, nids = std::min<uint64_t>(st.total_ids, S.cap);
      // the ids in two halves (two SDMA queues), then row starts and flags; packed: 3 bytes per id, u32 rows
      const uint64_t ib = nids * (S.packed ? 3 : 4), h1 = std::min<uint64_t>((ib / 2 + 15) & ~15ull, ib);
      const OutLayout ol = out_layout(n, S.cap);
      uint8_t* h = (uint8_t*)S.h_out.p;
      const uint8_t* di = S.packed ? S.d_pk.as<uint8_t>() : S.d_ids.as<uint8_t>();
      const void* dr = S.packed ? S.d_row32.p : S.d_row.p;
      const uint64_t rb = (n + 1) * (S.packed ? 4 : 8);
      if (dma) {
        const DmaPart parts[4] = {{h + ol.o_ids, di, h1},
                                  {h + ol.o_ids + h1, di + h1, ib - h1},
                                  {h + ol.o_row, dr, rb},
                                  {h + ol.o_fl, S.d_flags.p, n}};
        failed = !dma_copy_d2h(dma, parts, 4);
      } else {
        hipMemcpyAsync(h + ol.o_row, dr, rb, hipMemcpyDeviceToHost, c->pipe.d2h_stream);
        if (n) hipMemcpyAsync(h + ol.o_fl, S.d_flags.p, n, hipMemcpyDeviceToHost, c->pipe.d2h_stream);
        if (h1) hipMemcpyAsync(h + ol.o_ids, di, h1, hipMemcpyDeviceToHost, c->pipe.d2h_stream);
        if (ib > h1) {
          hipMemcpyAsync(h + ol.o_ids + h1, di + h1, ib - h1, hipMemcpyDeviceToHost, c->pipe.d2h_stream2);
          hipEventRecord(join, c->pipe.d2h_stream2);
          hipStreamWaitEvent(c->pipe.d2h_stream, join, 0);
        }
      }
    }
    // an overflowed or guarded batch copies nothing: the waiter reads the stats
    ptrace("copied", &S, it.second);
    hipEventRecord(S.ev_done, c->pipe.d2h_stream);
    {
      std::lock_guard<std::mutex> q(c->pipe.cq_mu);
      S.copied_gen = it.second;
      S.copy_failed = failed;
    }
    c->pipe.copied_cv.notify_all();
  }
  if (join) hipEventDestroy(join);
  dma_close(dma);
}

// Whether the slot's last launch has its D2H enqueued (ev_done recorded).
static bool slot_copied(egm_ctx* c, PipeSlot& S) {
  std::lock_guard<std::mutex> q(c->pipe.cq_mu);
  return S.copied_gen == S.launch_gen;
}

// A free pipeline slot for a batch (index into c->pipe), or -1.  Slots whose
// ticket was cancelled are reclaimed here once their batch has finished.
static PipeSlot* ticket_slot_of(egm_ctx* c, uint64_t ticket);

// Apply the cancels queued while the context was busy (context lock held).
static void drain_cancels(egm_ctx* c) {
  std::vector<uint64_t> q;
  {
    std::lock_guard<std::mutex> g(c->pipe.cancel_mu);
    q.swap(c->pipe.cancel_q);
  }
  for (uint64_t t : q)
    if (PipeSlot* sp = ticket_slot_of(c, t)) sp->abandoned = true;   // a stale ticket: dropped
  if (!q.empty()) c->pipe.cv.notify_all();
}

static long pipe_free_slot(egm_ctx* c) {
  drain_cancels(c);
  for (size_t k = 0; k < c->pipe.slots.size(); ++k) {
    PipeSlot& S = *c->pipe.slots[k];
    if (S.busy && S.abandoned && !S.waiting && slot_copied(c, S) && hipEventQuery(S.ev_done) == hipSuccess) {
      S.busy = S.abandoned = false;   // a cancelled ticket whose batch is done
    }
    if (!S.busy && !S.held) return (long)k;
  }
  return -1;
}

static int pipe_new_slot(egm_ctx* c, long* k) {
  c->pipe.slots.emplace_back(new PipeSlot());
  PipeSlot& N = *c->pipe.slots.back();
  if (hipEventCreateWithFlags(&N.ev_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&N.ev_match, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&N.ev_done, hipEventDisableTiming) != hipSuccess) {
    c->pipe.slots.pop_back();
    return c->fail(EGM_E_DEVICE, "pipe events");
  }
  *k = (long)c->pipe.slots.size() - 1;
  return EGM_OK;
}

// Submit with the context lock held once by the caller (g).  A ticket of
// egm_match_submit (sync = false) is refused when PIPE_MAX_SLOTS tickets are
// busy or unreleased; egm_match_batch (sync = true) takes any free slot, adds
// slots up to PIPE_HARD_SLOTS and beyond that waits for one to be freed, so
// concurrent synchronous callers queue instead of failing.
static int submit_locked(egm_ctx* c, std::unique_lock<std::recursive_mutex>& g, const uint8_t* blob,
                         const uint32_t* off, uint32_t n, int mode, bool sync, uint64_t* ticket) {
  if (set_device(c)) return EGM_E_DEVICE;
  hipError_t e;
  if (!c->pipe.copy_stream && (e = hipStreamCreateWithFlags(&c->pipe.copy_stream, hipStreamNonBlocking)) != hipSuccess)
    return c->hip_fail(e, "copy stream");
  if (!c->pipe.d2h_stream && (e = hipStreamCreateWithFlags(&c->pipe.d2h_stream, hipStreamNonBlocking)) != hipSuccess)
    return c->hip_fail(e, "d2h stream");
  if (!c->pipe.d2h_stream2 && (e = hipStreamCreateWithFlags(&c->pipe.d2h_stream2, hipStreamNonBlocking)) != hipSuccess)
    return c->hip_fail(e, "d2h stream");
  if (!c->pipe.copier.joinable()) c->pipe.copier = std::thread(copier_main, c);
  if (!sync) {
    size_t tickets = 0;
    for (auto& p : c->pipe.slots)   // a cancelled ticket no longer counts (its slot comes back when its batch is done)
      tickets += (!p->sync && !p->abandoned && (p->busy || p->held)) ? 1u : 0u;
    if (tickets >= PIPE_MAX_SLOTS) return c->fail(EGM_E_STATE, "pipeline full: wait for a ticket or free its result");
  }
  long k = pipe_free_slot(c);
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(PIPE_BATCH_WAIT_MS);
  while (k < 0) {
    if (c->pipe.slots.size() < PIPE_HARD_SLOTS) {
      const int r = pipe_new_slot(c, &k);
      if (r) return r;
      break;
    }
    if (!sync) return c->fail(EGM_E_STATE, "pipeline full: wait for a ticket or free its result");
    // every slot busy: wait for a release (polling too, for cancelled tickets)
    if (std::chrono::steady_clock::now() > deadline)
      return c->fail(EGM_E_STATE, "no pipeline slot freed within 30 s (results not released?)");
    c->pipe.cv.wait_for(g, std::chrono::milliseconds(2));
    k = pipe_free_slot(c);
  }
  PipeSlot& S = *c->pipe.slots[(size_t)k];
  // stage the caller's (borrowed) batch in pinned memory, offsets rebased to 0
  const uint32_t base0 = n ? off[0] : 0;
  const uint64_t bytes = n ? (uint64_t)off[n] - base0 : 0;
  const uint64_t o_off = (bytes + 15) & ~15ull, in_sz = o_off + ((uint64_t)n + 1) * 4;
  // the previous use of this slot's staging must be finished (its H2D)
  if ((e = hipEventSynchronize(S.ev_in)) != hipSuccess) return c->hip_fail(e, "pipe input reuse");
  if ((e = S.h_in.ensure(in_sz)) != hipSuccess) return c->hip_fail(e, "pipe pinned input");
  uint8_t* hin = (uint8_t*)S.h_in.p;
  if (bytes) par_copy(hin, blob + base0, bytes);
  uint32_t* hoff = (uint32_t*)(hin + o_off);
  std::atomic<uint64_t> maxlen{0};
  hoff[0] = 0;
  par_for(n, 1u << 18, [&](size_t lo, size_t hi) {   // offsets rebased to 0, and the longest topic
    uint64_t m = 0;
    for (size_t i = lo; i < hi; ++i) {
      hoff[i + 1] = off[i + 1] - base0;
      m = std::max<uint64_t>(m, (uint64_t)off[i + 1] - off[i]);
    }
    uint64_t cur = maxlen.load();
    while (m > cur && !maxlen.compare_exchange_weak(cur, m)) {
    }
  });
  S.n = n;
  S.mode = mode & ~EGM_RESULT_PACKED;
  S.want_packed = (mode & EGM_RESULT_PACKED) != 0;
  S.bytes = bytes;
  S.maxlen = maxlen.load();
  S.cap = std::max<uint64_t>(std::max<uint64_t>((uint64_t)n * 4 + 1024, S.cap), c->pipe.cap_hint);
  // blob and offsets in one copy (the staging already holds them back to back)
  S.o_off = o_off;
  if ((e = S.d_in.ensure(in_sz + 16)) != hipSuccess) return c->hip_fail(e, "pipe input");
  if ((e = hipMemcpyAsync(S.d_in.p, hin, in_sz, hipMemcpyHostToDevice, c->pipe.copy_stream)) != hipSuccess ||
      (e = hipEventRecord(S.ev_in, c->pipe.copy_stream)) != hipSuccess)
    return c->hip_fail(e, "pipe H2D");
  int r = pipe_launch(c, S);
  if (r) return r;
  S.busy = true;
  S.sync = sync;
  S.abandoned = false;
  S.gen = (S.gen + 1) & 0x7FFFFFFFu;
  if (S.gen == 0) S.gen = 1;
  *ticket = make_ticket((size_t)k, S.gen);
  return EGM_OK;
}

static bool pipe_mode_ok(int mode) {   // EGM_MODE_TRIE / EGM_MODE_ROUTES, optionally | EGM_RESULT_PACKED
  const int m = mode & ~EGM_RESULT_PACKED;
  return m == EGM_MODE_TRIE || m == EGM_MODE_ROUTES;
}

int egm_match_submit(egm_ctx* c, const uint8_t* blob, const uint32_t* off, uint32_t n, int mode, uint64_t* ticket) {
  if (!c || !ticket || !pipe_mode_ok(mode)) return EGM_E_INVAL;
  if (n && (!off || !valid_offsets(off, n) || (!blob && off[n] > off[0]))) return EGM_E_INVAL;
  ptrace("submit-enter", nullptr, n);
  std::unique_lock<std::recursive_mutex> g(c->mu);
  const int r = submit_locked(c, g, blob, off, n, mode, false, ticket);
  ptrace("submit-exit", nullptr, *ticket);
  return r;
}

// The slot of a live ticket (submitted, not yet waited for or cancelled), or null.
static PipeSlot* ticket_slot_of(egm_ctx* c, uint64_t ticket) {
  const size_t k = ticket_slot(ticket);
  if (ticket == 0 || k >= c->pipe.slots.size()) return nullptr;
  PipeSlot& S = *c->pipe.slots[k];
  if (!S.busy || S.waiting || S.abandoned || S.gen != ticket_gen(ticket)) return nullptr;
  return &S;
}

// The device syncs happen without the context lock, so another thread can
// submit (stage + enqueue) the next batch while this one waits.
int egm_match_wait(egm_ctx* c, uint64_t ticket, egm_result** out) {
  if (!c || !out || ticket == 0) return EGM_E_INVAL;
  *out = nullptr;
  std::unique_lock<std::recursive_mutex> g(c->mu);
  drain_cancels(c);
  PipeSlot* sp = ticket_slot_of(c, ticket);
  if (!sp) return c->fail(EGM_E_STATE, "unknown, stale or already waited ticket");
  if (set_device(c)) return EGM_E_DEVICE;
  PipeSlot& S = *sp;
  S.waiting = true;
  auto done = [&](int rc) {   // the slot is free again (its result, if any, held by the caller)
    if (!g.owns_lock()) g.lock();
    S.busy = S.waiting = false;
    c->pipe.cv.notify_all();
    return rc;
  };
  hipError_t e;
  MatchStats st{};
  ptrace("wait-enter", &S, ticket);
  for (int attempt = 0;; ++attempt) {
    g.unlock();
    bool copy_failed = false;
    {   // the copier has copied this launch's result (DMA) or enqueued its D2H (ev_done recorded)
      std::unique_lock<std::mutex> q(c->pipe.cq_mu);
      c->pipe.copied_cv.wait(q, [&] { return S.copied_gen == S.launch_gen; });
      copy_failed = S.copy_failed;
    }
    e = hipEventSynchronize(S.ev_done);
    g.lock();
    if (e != hipSuccess) return done(c->hip_fail(e, "pipe wait"));
    if (copy_failed) return done(c->fail(EGM_E_DEVICE, "pipe result copy (SDMA) failed"));
    st = *(const MatchStats*)S.h_stats.p;
    if (st.guard) {   // a kernel invariant failed: a bug, never a capacity problem (no retry)
      c->last = st;
      return done(c->fail(EGM_E_DEVICE, "walk guard tripped (bits " + std::to_string(st.guard) +
                                             "): kernel invariant failed, batch not matched"));
    }
    if (!st.overflow) break;
    if (attempt == 2) return done(c->fail(EGM_E_NOMEM, "ids capacity"));
    // the exact total is known even on overflow: rerun the staged batch once with room for it
    S.cap = st.total_ids + st.total_ids / 8 + 1024;
    c->pipe.cap_hint = std::max(c->pipe.cap_hint, S.cap);
    const int r = pipe_launch(c, S);
    if (r) return done(r);
  }
  c->last = st;   // egm_last_stats reports the waited batch
  const uint64_t n = S.n, nids = st.total_ids;
  // the copy-out kernel wrote row_ptr, ids and flags into h_out (ev_done)
  const OutLayout ol = out_layout(n, S.cap);
  uint8_t* h = (uint8_t*)S.h_out.p;
  ResultHdr* hdr = (ResultHdr*)h;
  egm_result* res = (egm_result*)(h + ol.o_res);
  memset(res, 0, sizeof(*res));
  res->n_topics = S.n;
  res->n_ids = nids;
  res->counts = (uint32_t*)(h + ol.o_cnt);
  if (S.packed) {   // row starts as u32, ids as 3 bytes (egm_result_row / egm_result_id)
    res->id_bytes = 3;
    res->row32 = (const uint32_t*)(h + ol.o_row);
    res->ids24 = h + ol.o_ids;
  } else {
    res->id_bytes = 4;
    res->row_ptr = (uint64_t*)(h + ol.o_row);
    res->ids = (uint32_t*)(h + ol.o_ids);
  }
  res->flags = (uint8_t*)(h + ol.o_fl);
  res->epoch = S.epoch;
  res->visited = st.visited;
  res->n_error = st.errors;
  g.unlock();
  // host work outside the lock, on up to 8 threads: counts (not copied over
  // PCIe: row_ptr has them) and the heavy-topic total
  std::atomic<uint32_t> heavy_n{0};
  {
    const uint64_t* rp = res->row_ptr;
    const uint32_t* r32 = res->row32;
    uint32_t* cn = res->counts;
    const uint8_t* fl = res->flags;
    par_for(n, 1u << 17, [&](size_t lo, size_t hi) {
      uint32_t h = 0;
      for (size_t i = lo; i < hi; ++i) {
        cn[i] = r32 ? r32[i + 1] - r32[i] : (uint32_t)(rp[i + 1] - rp[i]);
        h += (fl[i] & TF_HEAVY) ? 1u : 0u;
      }
      heavy_n += h;
    });
  }
  const uint32_t heavy = heavy_n.load();
  g.lock();
  if (egm_result_row(res, (uint32_t)n) != nids) return done(c->fail(EGM_E_DEVICE, "row_ptr total mismatch"));
  res->n_heavy = heavy;
  hdr->magic = RES_PIPE;
  hdr->owner = c;
  hdr->slot = ticket_slot(ticket);
  S.held = true;
  done(EGM_OK);
  ptrace("wait-exit", &S, ticket);
  *out = res;
  if (res->n_error) {
    c->err = "some topics could not be walked (flag EGM_TF_ERROR)";
    return EGM_E_OVERFLOW;
  }
  return EGM_OK;
}

// Give up a ticket without its result: the slot is reclaimed as soon as its
// batch has finished (no wait here).  For a waiter that will never call
// egm_match_wait (e.g. the NIF ticket resource collected unwaited).
int egm_match_cancel(egm_ctx* c, uint64_t ticket) {
  if (!c || ticket == 0) return EGM_E_INVAL;
  std::unique_lock<std::recursive_mutex> g(c->mu, std::try_to_lock);
  if (!g.owns_lock()) {   // busy (a build or commit can hold the context for seconds): queue it
    std::lock_guard<std::mutex> q(c->pipe.cancel_mu);
    c->pipe.cancel_q.push_back(ticket);
    return EGM_OK;
  }
  drain_cancels(c);
  PipeSlot* sp = ticket_slot_of(c, ticket);
  if (!sp) return c->fail(EGM_E_STATE, "unknown, stale or already waited ticket");
  sp->abandoned = true;
  c->pipe.cv.notify_all();
  return EGM_OK;
}

// One synchronous batch: submit + wait on a pipeline slot of its own.  Host
// buffers are staged in pinned memory and the result is read in place from
// pinned memory (released by egm_result_free).  Concurrent callers never get
// "pipeline full": they take extra slots, then wait for one to be released.
int egm_match_batch(egm_ctx* c, const uint8_t* blob, const uint32_t* off, uint32_t n, int mode,
                    egm_result** out) {
  if (!c || !out || !pipe_mode_ok(mode)) return EGM_E_INVAL;
  *out = nullptr;
  if (n && (!off || !valid_offsets(off, n) || (!blob && off[n] > off[0]))) return EGM_E_INVAL;
  uint64_t t = 0;
  {
    std::unique_lock<std::recursive_mutex> g(c->mu);
    const int r = submit_locked(c, g, blob, off, n, mode, true, &t);
    if (r) return r;
  }
  return egm_match_wait(c, t, out);
}

// egm_result_free for a pipeline result: the slot's pinned memory is free again.
static void pipe_release(egm_ctx* c, uint64_t slot) {
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (slot < c->pipe.slots.size()) c->pipe.slots[slot]->held = false;
  c->pipe.cv.notify_all();
}

void egm_result_free(void* r) {
  if (!r) return;
  ResultHdr* h = (ResultHdr*)r - 1;
  if (h->magic == RES_PIPE) pipe_release((egm_ctx*)h->owner, h->slot);
  else result_discard(r);
}

}  // extern "C"
