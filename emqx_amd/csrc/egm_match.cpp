// egm_match.cpp — the device match path of the C-ABI: the per-batch
// workspaces, run_match (every match launch goes through it, the host
// pipeline's too), the egm_match_device* entries, the egm_last_* counters of
// the last batch, and the walk sort's test entry.
#include <stdlib.h>

#include "egm_ctx.h"

using namespace egm;

// Walk order: the sort key's bits per level as hex nibbles,
// level 0 in the lowest; 0 walks in input order.  EGM_WALK_KEY is a tuning
// knob for A/B runs (read at every batch); the default is the measured best:
// 4/6/7/7 bits over four levels — 24 bits, three sort passes (round 5, one
// process: 11.63 ms per C2 step against 11.75-11.78 for round 4's 6/8/10/8,
// whose fourth sort pass bought no walk time with the flush records; the
// walk 8.57 vs 8.58-8.61 ms; profiles/r5_walk_key_ab.jsonl).
constexpr uint32_t WALK_KEY_DEFAULT = 0x7764u;
static uint32_t walk_key_shape() {
  const char* v = getenv("EGM_WALK_KEY");
  const uint32_t shape = (v && *v) ? (uint32_t)strtoul(v, nullptr, 16) & 0xFFFFu : WALK_KEY_DEFAULT;   // KEY_LEVELS nibbles
  return walk_key_bits(shape) <= 32 ? shape : WALK_KEY_DEFAULT;
}

// EGM_WALK_SORT_MIN_BYTES: tables smaller than this are walked in input order.
// Sorting pays when the table is far larger than the caches (C2: 2.85 GB,
// 13.3 -> 12.7 ms per step); at C1 (357 MB, mostly MALL-resident) the walk
// gains 0.16 ms and the sort costs 0.4.
static uint64_t walk_sort_min_bytes() {
  const char* v = getenv("EGM_WALK_SORT_MIN_BYTES");
  return (v && *v) ? strtoull(v, nullptr, 10) : (1ull << 30);
}

// Test and A/B knobs of the flush records: EGM_FLUSH_AT — staged emits that
// trigger a flush (1..WALK_STAGE, default WALK_STAGE: small values make many
// short records per chunk); EGM_REC_SEG — u32 per record segment (default
// REC_GRAIN; small values make chunks' record chains jump between segments).
static uint32_t env_u32(const char* name, uint32_t dflt, uint32_t lo, uint32_t hi) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  const long long k = atoll(v);
  return (uint32_t)std::min<long long>(std::max<long long>(k, lo), hi);
}
static uint32_t flush_lim() { return env_u32("EGM_FLUSH_AT", walk_stage(), 1, walk_stage()); }
static uint32_t rec_grain() { return env_u32("EGM_REC_SEG", REC_GRAIN, 64, 1u << 24) & ~(uint32_t)(EGM_REC_ALIGN - 1); }

// The workspace for a batch on stream s: the one that last ran on s (stream
// order protects it), else the least recently used one, ordered after its
// last batch on the other stream.
MatchWs& egm::pick_ws(egm_ctx* c, hipStream_t s) {
  uint32_t k = 0;
  for (uint32_t i = 0; i < MATCH_WORKSPACES; ++i) {
    if (c->ws[i].stream == s && c->ws[i].used) {
      k = i;
      break;
    }
    if (c->ws[i].used < c->ws[k].used) k = i;
  }
  MatchWs& W = c->ws[k];
  if (W.used && W.stream != s && W.ev) hipStreamWaitEvent(s, W.ev, 0);   // (stream 0 is a stream too)
  c->cur_ws = k;
  W.used = ++c->ws_clock;
  return W;
}

// max_levels: an upper bound on the levels of any topic of the batch (the
// heavy kernel's stack must hold the deepest one's DFS, egm_kernels.hip).
int egm::ensure_work(egm_ctx* c, MatchWs& W, uint32_t n, uint64_t blob_bytes, uint64_t ids_cap,
                     uint64_t max_levels) {
  hipError_t e;
  const uint64_t nn = (uint64_t)n + 1;
  W.blob_bytes = blob_bytes;
  if ((e = W.wid.ensure((blob_bytes + nn) * 4)) != hipSuccess) return c->hip_fail(e, "wid");
  if ((e = W.lv.ensure(nn * 4)) != hipSuccess) return c->hip_fail(e, "lv");
  if ((e = W.tfl.ensure(nn)) != hipSuccess) return c->hip_fail(e, "tfl");
  if ((e = W.cnt.ensure(nn * 4)) != hipSuccess) return c->hip_fail(e, "cnt");
  // flush records: sized for the worst case of the batch's id capacity
  W.flush_lim = flush_lim();
  W.rec_grain = rec_grain();
  const uint64_t rcap = rec_capacity(ids_cap, n, W.flush_lim, W.rec_grain);
  if ((e = W.rec.ensure(rcap * 4)) != hipSuccess) return c->hip_fail(e, "flush records");
  W.rec_cap = W.rec.cap / 4;
  if (W.rec_cap >= (1ull << 34)) return c->fail(EGM_E_INVAL, "batch too large: > 16G u32 of flush records (split it)");
  if ((e = W.chunks.ensure(walk_chunk_cap(n) * 16)) != hipSuccess) return c->hip_fail(e, "chunk records");
  if ((e = W.dir.ensure(walk_chunk_cap(n) * REC_DIR * 4)) != hipSuccess)
    return c->hip_fail(e, "chunk directories");
  // heavy topics: their ids (count then fill, one piece per topic)
  const uint64_t tcap = ids_cap + 4096;
  if (tcap >= 0xFFFFFFF0ull) return c->fail(EGM_E_INVAL, "batch too large: > 4G matched ids (split it)");
  if ((e = W.ids_tmp.ensure(tcap * 4)) != hipSuccess) return c->hip_fail(e, "ids_tmp");
  W.ids_tmp_cap = W.ids_tmp.cap / 4;
  if ((e = W.pieces.ensure(((uint64_t)n + 4096) * 16)) != hipSuccess) return c->hip_fail(e, "pieces");
  W.pieces_cap = std::min<uint64_t>(W.pieces.cap / 16, 0xFFFFFFF0ull);
  if ((e = W.deferred.ensure(walk_chunk_cap(n) * 4 * 2)) != hipSuccess) return c->hip_fail(e, "deferred");
  const uint32_t hcap = heavy_stack_items(max_levels);
  if ((e = W.heavy_stack.ensure((uint64_t)c->heavy_waves * hcap * 16)) != hipSuccess)
    return c->hip_fail(e, "heavy stack");
  W.heavy_cap = (uint32_t)std::min<uint64_t>(W.heavy_stack.cap / 16 / c->heavy_waves, 0xFFFFFFFFull);
  if ((e = W.tile_sums.ensure((scan_tiles(n) + 2) * 8)) != hipSuccess) return c->hip_fail(e, "tile_sums");
  if ((e = W.stats.ensure(sizeof(MatchStats))) != hipSuccess) return c->hip_fail(e, "stats");
  const uint32_t shape = walk_key_shape();
  if (shape) {
    if ((e = W.skey.ensure(nn * 4)) != hipSuccess) return c->hip_fail(e, "sort keys");
    if ((e = W.skey_out.ensure(nn * 4)) != hipSuccess) return c->hip_fail(e, "sort keys");
    if ((e = W.sval.ensure(nn * 8)) != hipSuccess) return c->hip_fail(e, "sort values");
    if ((e = W.order.ensure(nn * 8)) != hipSuccess) return c->hip_fail(e, "walk order");
    if ((e = W.wfix.ensure(nn * 4 * FIX_WORDS)) != hipSuccess) return c->hip_fail(e, "fixed-stride words");

    if ((e = W.sort_tmp.ensure(walk_sort_temp_bytes(n, shape))) != hipSuccess) return c->hip_fail(e, "sort scratch");
  }
  if (!W.ev && (e = hipEventCreateWithFlags(&W.ev, hipEventDisableTiming)) != hipSuccess)
    return c->hip_fail(e, "workspace event");
  return EGM_OK;
}

static MatchWork work_view(egm_ctx* c, MatchWs& W) {
  MatchWork w{};
  w.wid = W.wid.as<uint32_t>();
  w.lv = W.lv.as<uint32_t>();
  w.tfl = W.tfl.as<uint8_t>();
  w.cnt = W.cnt.as<uint32_t>();
  w.rec = W.rec.as<uint32_t>();
  w.rec_cap = W.rec_cap;
  w.rec_grain = W.rec_grain;
  w.flush_lim = W.flush_lim;
  w.blob_bytes = W.blob_bytes;
  w.chunks = W.chunks.as<uint4>();
  w.dir = W.dir.as<uint32_t>();
  w.ids_tmp = W.ids_tmp.as<uint32_t>();
  w.ids_cap = W.ids_tmp_cap;   // ids_tmp entries (the output capacity is MatchOut's)
  w.pieces = W.pieces.as<uint4>();
  w.pieces_cap = W.pieces_cap;
  w.deferred = W.deferred.as<uint32_t>();
  w.deep = w.deferred + W.deferred.cap / 8;   // the second half: the walk's deep-pass list
  w.heavy_stack = W.heavy_stack.as<uint4>();
  w.heavy_waves = c->heavy_waves;
  w.heavy_cap = W.heavy_cap;
  w.tile_sums = W.tile_sums.as<uint64_t>();
  w.stats = W.stats.as<MatchStats>();
  w.debug = c->debug;
  w.key_shape = walk_key_shape();
  if (w.key_shape && W.order.p) {
    w.skey = W.skey.as<uint32_t>();
    w.skey_out = W.skey_out.as<uint32_t>();
    w.sval = W.sval.as<uint64_t>();
    w.order = W.order.as<uint64_t>();
    w.wfix = W.wfix.as<uint32_t>();

    w.sort_tmp = W.sort_tmp.p;
    w.sort_tmp_bytes = W.sort_tmp.cap;
  } else {
    w.key_shape = 0;
  }

  return w;
}

int egm::run_match(egm_ctx* c, MatchWs& W, const Epoch& ep, const uint8_t* d_blob, const uint32_t* d_off, uint32_t n,
                   int mode, hipStream_t s, uint64_t* d_row, uint32_t* d_ids, uint64_t ids_cap,
                   const uint32_t* d_n_live, uint32_t* d_topic) {
  MatchWork w = work_view(c, W);
  w.n_live = d_n_live;
  if (ep.bytes < walk_sort_min_bytes()) w.key_shape = 0;   // the table fits the caches: the order buys nothing
  MatchOut o{d_row, d_ids, ids_cap, d_topic};
  hipEvent_t evs[2] = {nullptr, nullptr};
  hipEvent_t* evp = c->timing.take_pair(evs);
  bool walk_sorted = false;
  hipError_t e = launch_match(ep.view, d_blob, d_off, n, mode, w, o, s, evp, &walk_sorted);
  c->last_walk.order = (walk_sorted && !d_topic) ? w.order : nullptr;   // (walk-order rows: already in that order)
  c->last_walk.row = d_row;
  c->last_walk.n = n;
  c->last_walk.ws = (uint32_t)(&W - c->ws);
  c->slots[ep.slot].uses.note(s);   // a later commit must not overwrite this slot before the walk is done
  c->timing.push_pair(c->timing.walk, evp);
  if (e != hipSuccess) return c->hip_fail(e, "launch_match");
  c->last_pending = true;
  c->last_stream = s;
  return EGM_OK;
}

// After the batch's last use of W on s (a flags/counts copy included).
void egm::ws_done(MatchWs& W, hipStream_t s) {
  hipEventRecord(W.ev, s);
  W.stream = s;
}

static int sync_last(egm_ctx* c) {
  if (!c->last_pending) return EGM_OK;
  hipError_t e = hipStreamSynchronize(c->last_stream);
  if (e != hipSuccess) return c->hip_fail(e, "hipStreamSynchronize");
  e = hipMemcpy(&c->last, c->ws[c->cur_ws].stats.p, sizeof(MatchStats), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return c->hip_fail(e, "stats readback");
  c->last_pending = false;
  return EGM_OK;
}

// What the egm_match_device* entries share once their arguments are checked:
// one batch of n topics (*d_n of them live, when given) on the caller's
// stream; d_topic: rows in walk order; d_flags: the per-topic flags copied out.
static int match_device_common(egm_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint32_t* d_off,
                               uint32_t n, const uint32_t* d_n, int mode, void* hip_stream, uint64_t* d_row,
                               uint32_t* d_topic, uint32_t* d_ids, uint64_t ids_cap, uint8_t* d_flags) {
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  hipStream_t s = (hipStream_t)hip_stream;   // NULL: the HIP default (null) stream, as the caller's own work
  // a topic has at most (its bytes + 1) levels, and a legal one at most 65 536
  // (emqx_topic.erl:45, 99-100): bound the device batch's depth by its blob
  MatchWs& W = pick_ws(c, s);
  int r = ensure_work(c, W, n, blob_bytes, ids_cap, std::min<uint64_t>(blob_bytes, 65535) + 1);
  if (r) return r;
  std::shared_ptr<Epoch> ep = c->cur;
  r = run_match(c, W, *ep, d_blob, d_off, n, mode, s, d_row, d_ids, ids_cap, d_n, d_topic);
  if (r == EGM_OK && d_flags && n) {
    hipError_t e = hipMemcpyAsync(d_flags, W.tfl.p, n, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) r = c->hip_fail(e, "flags copy");
  }
  ws_done(W, s);
  return r;
}

extern "C" {

int egm_match_device(egm_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint32_t* d_off, uint32_t n,
                     int mode, void* hip_stream, uint64_t* d_row, uint32_t* d_ids, uint64_t ids_cap,
                     uint8_t* d_flags) {
  if (!c || (mode != EGM_MODE_TRIE && mode != EGM_MODE_ROUTES) || !d_row) return EGM_E_INVAL;
  if (n && (!d_blob || !d_off || ((uintptr_t)d_blob & 3))) return EGM_E_INVAL;
  return match_device_common(c, d_blob, blob_bytes, d_off, n, nullptr, mode, hip_stream, d_row, nullptr, d_ids, ids_cap,
                             d_flags);
}

int egm_match_device_ordered(egm_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint32_t* d_off,
                             uint32_t n, int mode, void* hip_stream, uint64_t* d_row, uint32_t* d_topic,
                             uint32_t* d_ids, uint64_t ids_cap) {
  if (!c || (mode != EGM_MODE_TRIE && mode != EGM_MODE_ROUTES) || !d_row || (n && !d_topic)) return EGM_E_INVAL;
  if (n && (!d_blob || !d_off || ((uintptr_t)d_blob & 3))) return EGM_E_INVAL;
  return match_device_common(c, d_blob, blob_bytes, d_off, n, nullptr, mode, hip_stream, d_row, d_topic, d_ids, ids_cap,
                             nullptr);
}

int egm_match_device_counted(egm_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint32_t* d_off,
                             uint32_t n_max, const uint32_t* d_n, int mode, void* hip_stream, uint64_t* d_row,
                             uint32_t* d_ids, uint64_t ids_cap) {
  return egm_match_device_counted_ordered(c, d_blob, blob_bytes, d_off, n_max, d_n, mode, hip_stream, d_row, nullptr,
                                          d_ids, ids_cap);
}

int egm_match_device_counted_ordered(egm_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint32_t* d_off,
                                     uint32_t n_max, const uint32_t* d_n, int mode, void* hip_stream, uint64_t* d_row,
                                     uint32_t* d_topic, uint32_t* d_ids, uint64_t ids_cap) {
  if (!c || (mode != EGM_MODE_TRIE && mode != EGM_MODE_ROUTES) || !d_row || !d_n) return EGM_E_INVAL;
  if (n_max && (!d_blob || !d_off || ((uintptr_t)d_blob & 3))) return EGM_E_INVAL;
  return match_device_common(c, d_blob, blob_bytes, d_off, n_max, d_n, mode, hip_stream, d_row, d_topic, d_ids,
                             ids_cap, nullptr);
}

int egm_last_walk_counters(egm_ctx* c, uint64_t* iters, uint64_t* popped, uint64_t* bounded, uint64_t* lit_probes,
                           uint64_t* plus_reads) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  int r = sync_last(c);
  if (r) return r;
  if (iters) *iters = c->last.iters;
  if (popped) *popped = c->last.popped;
  if (bounded) *bounded = c->last.bounded;
  if (lit_probes) *lit_probes = c->last.lit_probes;
  if (plus_reads) *plus_reads = c->last.plus_reads;
  return EGM_OK;
}

int egm_last_walk_probes(egm_ctx* c, uint64_t* slow_lanes, uint64_t* slow_iters) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  int r = sync_last(c);
  if (r) return r;
  if (slow_lanes) *slow_lanes = c->last.slow_lanes;
  if (slow_iters) *slow_iters = c->last.slow_iters;
  return EGM_OK;
}

int egm_last_stats(egm_ctx* c, uint64_t* n_ids, uint64_t* visited, uint32_t* n_def, uint32_t* overflow,
                   uint32_t* n_error) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  int r = sync_last(c);
  if (r) return r;
  if (n_ids) *n_ids = c->last.total_ids;
  if (visited) *visited = c->last.visited;
  if (n_def) *n_def = c->last.n_deferred;
  if (overflow) *overflow = c->last.overflow;
  if (n_error) *n_error = c->last.errors;
  if (c->last.guard)   // a kernel invariant failed: the batch's rows are not valid (never a capacity problem)
    return c->fail(EGM_E_DEVICE, "walk guard tripped (bits " + std::to_string(c->last.guard) +
                                     "): kernel invariant failed, batch not matched");
  return EGM_OK;
}

int egm_last_walk_chunks(egm_ctx* c, uint32_t* deep, uint32_t* deferred) {
  if (!c) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  int r = sync_last(c);
  if (r) return r;
  if (deep) *deep = c->last.n_deep;
  if (deferred) *deferred = c->last.n_deferred;
  return EGM_OK;
}

int egm_last_guard(egm_ctx* c, uint32_t* guard) {
  if (!c || !guard) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  int r = sync_last(c);
  if (r) return r;
  *guard = c->last.guard;
  return EGM_OK;
}

int egm_debug_walk_sort(egm_ctx* c, const uint32_t* d_keys, const uint64_t* d_vals, uint32_t n, uint32_t kbits,
                        uint64_t* d_out) {
  if (!c || !d_keys || !d_vals || !d_out || !n || n >= (1u << 29) || !kbits || kbits > 32) return EGM_E_INVAL;
  std::lock_guard<std::recursive_mutex> g(c->mu);
  if (set_device(c)) return EGM_E_DEVICE;
  DevBuf k1, k2, v1, tmp, st;
  // a shape whose levels sum to kbits (the scratch size depends only on the bits)
  const uint32_t shape = kbits <= 15 ? kbits : (kbits <= 30 ? (15u | ((kbits - 15) << 4)) : (15u | (15u << 4) | ((kbits - 30) << 8)));
  hipError_t e;
  if ((e = k1.ensure((size_t)n * 4)) != hipSuccess || (e = k2.ensure((size_t)n * 4)) != hipSuccess ||
      (e = v1.ensure((size_t)n * 8)) != hipSuccess || (e = tmp.ensure(walk_sort_temp_bytes(n, shape))) != hipSuccess ||
      (e = st.ensure(sizeof(MatchStats))) != hipSuccess)
    return c->hip_fail(e, "debug sort: scratch");
  if ((e = hipMemcpyAsync(k1.p, d_keys, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(v1.p, d_vals, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream)) != hipSuccess ||
      (e = hipMemsetAsync(st.p, 0, sizeof(MatchStats), c->stream)) != hipSuccess ||
      (e = launch_walk_sort(k1.as<uint32_t>(), k2.as<uint32_t>(), v1.as<uint64_t>(), d_out, tmp.p, st.as<MatchStats>(),
                            n, kbits, c->stream)) != hipSuccess)
    return c->hip_fail(e, "debug sort: launch");
  MatchStats hs{};
  if ((e = hipMemcpyAsync(&hs, st.p, sizeof hs, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return c->hip_fail(e, "debug sort: sync");
  if (hs.guard) return c->fail(EGM_E_DEVICE, "debug sort: look-back guard tripped");
  return EGM_OK;
}

}  // extern "C"
