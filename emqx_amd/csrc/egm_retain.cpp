// egm_retain.cpp — retained-message store and its reverse match on the GPU
// (C-ABI in include/emqx_gpu_match.h, egm_rstore_*).
//
// Mirrors apps/emqx_retainer/src/emqx_retainer_mnesia.erl:
//   store_retained/2 :73-101  -> egm_rstore_put     (a topic keeps one record;
//                                is_table_full/0 :230-240 as egm_rstore_set_max_retained)
//   delete_message/2 :114-129 -> egm_rstore_delete  (plain topic) and, with
//                                match_delete_messages/1 :206-212,
//                                egm_rstore_delete_matching (filters)
//   clean/1          :148-150 -> egm_rstore_clean
//   clear_expired/1  :103-112 -> egm_rstore_clear_expired
//   match_messages/1 :200-204 -> egm_rstore_match   (condition/1 :215-220,
//                                make_match_spec/1 :222-228)
//   read_messages/1  :187-198 -> egm_rstore_match, EGM_RMODE_DISPATCH
//
// Device image (egm_kernels.h RetainView): the topics' word trie, nodes
// numbered breadth-first (children contiguous), topics ranked depth-first so
// the topics under a node are one rank range; a (node, word) -> child hash
// table; the dictionary in the layout k_tokenise reads; rank -> message id and
// expiry.
//
// Commits are incremental: a put on a topic of the image patches
// msg[rank] and expiry[rank] in place, a delete makes the rank a tombstone
// (msg[rank] = RS_TOMB), and a topic the image does not hold goes into the
// overlay, a small device list that the match compares byte by byte
// (RetainOverlay).  The image is rebuilt from the records only when
// rs_commit_locked says so.
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/emqx_gpu_match.h"
#include "egm_alloc.h"
#include "egm_buf.h"
#include "egm_kernels.h"

using namespace egm;

namespace {

template <class T>
hipError_t put_vec(DevBuf& b, const std::vector<T>& v) {
  hipError_t e = b.ensure(v.size() * sizeof(T) + 16);
  if (e == hipSuccess && !v.empty()) e = hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

// One record per topic.  A topic is in the image (rank != NONE) or in the
// overlay (ov != NONE), never both.  A deleted image topic stays in the map,
// marked dead, until the next rebuild: its rank is a tombstone on the device
// and a later put of the topic revives that rank.
struct Rec {
  uint32_t msg = 0;
  uint64_t expiry = 0;
  uint32_t rank = NONE;    // image rank
  uint32_t ov = NONE;      // index in egm_rstore::ov_ents
  bool dead = false;       // image topic, deleted
  bool dev_dead = false;   // the device holds a tombstone at the rank
  bool dirty = false;      // the rank is queued in egm_rstore::touched
};
using RecMap = std::unordered_map<std::string, Rec>;
using Ent = RecMap::value_type;   // node-based map: an entry's address is stable until it is erased

// The host image (built at a rebuild).
struct Image {
  std::vector<uint4> nodes;           // RetainView::nodes
  std::vector<uint4> edges;           // 16 B slots, 4 per bucket
  uint32_t edge_mask = 0;
  std::vector<DictSlot> dict;
  std::vector<uint8_t> dict_blob;
  std::vector<uint64_t> dict_off;
  std::vector<uint32_t> msg;
  std::vector<uint64_t> expiry;
};

bool split_words(const std::string& t, std::vector<std::pair<uint32_t, uint32_t>>* out) {
  out->clear();
  uint32_t ws = 0;
  for (uint32_t i = 0; i <= t.size(); ++i) {
    if (i < t.size() && t[i] != '/') continue;
    out->push_back({ws, i - ws});
    ws = i + 1;
  }
  return true;
}

// ents: the live records; on return they carry their ranks and by_rank lists them in rank order
void build_image(const std::vector<Ent*>& ents, Image* im, std::vector<Ent*>* by_rank) {
  // dictionary: every distinct topic word, in the k_tokenise probe layout
  std::unordered_map<std::string, uint32_t> wmap;
  std::vector<const std::string*> topics;
  topics.reserve(ents.size());
  for (const Ent* e : ents) topics.push_back(&e->first);
  std::vector<uint64_t> woff(1, 0);   // per topic: first word in flat
  std::vector<uint32_t> flat;
  std::vector<std::pair<uint32_t, uint32_t>> ws;
  im->dict_blob.clear();
  im->dict_off.assign(1, 0);
  for (const std::string* t : topics) {
    split_words(*t, &ws);
    for (auto [s, l] : ws) {
      std::string w = t->substr(s, l);
      auto it = wmap.find(w);
      uint32_t id;
      if (it == wmap.end()) {
        id = (uint32_t)wmap.size();
        wmap.emplace(w, id);
        im->dict_blob.insert(im->dict_blob.end(), w.begin(), w.end());
        im->dict_off.push_back(im->dict_blob.size());
      } else {
        id = it->second;
      }
      flat.push_back(id);
    }
    woff.push_back(flat.size());
  }
  size_t dcap = 64;
  while (dcap < wmap.size() * 2) dcap <<= 1;
  im->dict.assign(dcap, DictSlot{0, NONE, 0, {0}});
  for (uint32_t w = 0; w + 1 < im->dict_off.size(); ++w) {
    const uint8_t* p = im->dict_blob.data() + im->dict_off[w];
    const uint32_t len = (uint32_t)(im->dict_off[w + 1] - im->dict_off[w]);
    const uint64_t h = word_hash(p, len);
    uint32_t i = (uint32_t)(h & (dcap - 1));
    while (im->dict[i].wid != NONE) i = (i + 1) & (uint32_t)(dcap - 1);
    DictSlot s{h, w, len, {0}};
    memcpy(s.inl, p, len < 16 ? len : 16);
    im->dict[i] = s;
  }

  // depth-first ranks: topics sorted by their word-id sequences (a prefix
  // sorts before its extensions)
  const uint32_t M = (uint32_t)topics.size();
  std::vector<uint32_t> order(M);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return std::lexicographical_compare(flat.begin() + woff[a], flat.begin() + woff[a + 1], flat.begin() + woff[b],
                                        flat.begin() + woff[b + 1]);
  });
  // trie in depth-first order: node = (parent, word, lo, hi, term)
  struct DNode {
    uint32_t parent, word, lo, hi;
    bool term;
  };
  std::vector<DNode> dn;
  dn.push_back({NONE, NONE, 0, M, false});   // root: no word consumed
  std::vector<uint32_t> path(1, 0);            // path[d] = node after d words
  im->msg.resize(M);
  im->expiry.resize(M);
  by_rank->resize(M);
  for (uint32_t r = 0; r < M; ++r) {
    const uint32_t t = order[r];
    const uint64_t a = woff[t], b = woff[t + 1];
    const uint32_t D = (uint32_t)(b - a);
    // common prefix with the current path
    uint32_t c = 0;
    while (c + 1 < path.size() && c < D && dn[path[c + 1]].word == flat[a + c]) ++c;
    for (size_t d = path.size() - 1; d > c; --d) dn[path[d]].hi = r;   // close the rest
    path.resize(c + 1);
    for (uint32_t d = c; d < D; ++d) {
      dn.push_back({path[d], flat[a + d], r, M, false});
      path.push_back((uint32_t)dn.size() - 1);
    }
    dn[path[D]].term = true;   // D >= 1: words/1 of any topic has >= 1 word
    Rec& rec = ents[t]->second;
    im->msg[r] = rec.msg;
    im->expiry[r] = rec.expiry;
    rec.rank = r;
    rec.ov = NONE;
    rec.dev_dead = rec.dirty = false;
    (*by_rank)[r] = ents[t];
  }
  // breadth-first numbering: the children of a node are contiguous
  const uint32_t N = (uint32_t)dn.size();
  std::vector<uint32_t> kstart(N + 1, 0), kids;
  for (uint32_t i = 1; i < N; ++i) ++kstart[dn[i].parent + 1];
  for (uint32_t i = 0; i < N; ++i) kstart[i + 1] += kstart[i];
  kids.resize(kstart[N]);
  {
    std::vector<uint32_t> pos(kstart.begin(), kstart.end() - 1);
    for (uint32_t i = 1; i < N; ++i) kids[pos[dn[i].parent]++] = i;   // depth-first = word order
  }
  std::vector<uint32_t> bfs;
  bfs.reserve(N);
  std::vector<uint32_t> nid(N, NONE);
  bfs.push_back(0);
  nid[0] = 0;
  for (size_t q = 0; q < bfs.size(); ++q)
    for (uint32_t k = kstart[bfs[q]]; k < kstart[bfs[q] + 1]; ++k) {
      nid[kids[k]] = (uint32_t)bfs.size();
      bfs.push_back(kids[k]);
    }
  im->nodes.assign(N, uint4{0, 0, 0, 0});
  for (uint32_t o = 0; o < N; ++o) {
    const uint32_t i = nid[o];
    const uint32_t nk = kstart[o + 1] - kstart[o];
    const uint32_t first = nk ? nid[kids[kstart[o]]] : 0u;
    im->nodes[i] = uint4{first, nk | (dn[o].term ? RN_TERM : 0u), dn[o].lo, dn[o].hi};
  }
  // (node, word) -> child, 25-50 % slot load
  size_t nb = 16;
  while (nb * 4 < (size_t)(N - 1) * 2) nb <<= 1;
  im->edges.assign(nb * 4, uint4{NONE, 0, 0, 0});
  im->edge_mask = (uint32_t)(nb - 1);
  for (uint32_t o = 1; o < N; ++o) {
    const uint32_t par = nid[dn[o].parent], w = dn[o].word;
    uint32_t bkt = edge_bucket(par, w, im->edge_mask);
    for (;;) {
      uint4* sl = &im->edges[(size_t)bkt * 4];
      int k = 0;
      while (k < 4 && sl[k].x != NONE) ++k;
      if (k < 4) {
        sl[k] = uint4{par, w, nid[o], 0};
        break;
      }
      bkt = (bkt + 1) & im->edge_mask;
    }
  }
}

}  // namespace

// (-Wattributes: the opaque egm_rstore is less hidden than DevBuf, as egm_ctx is; see egm_ctx.h)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wattributes"
struct egm_rstore {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::string err;
  // host records and what changed since the last commit
  RecMap recs;                   // live records, and the dead topics of the image
  uint64_t n_live = 0;
  std::vector<Ent*> by_rank;     // image rank -> record
  std::vector<Ent*> ov_ents;     // the overlay, in its device order
  std::vector<uint32_t> touched; // image ranks to patch
  uint64_t dead_ranks = 0;       // tombstones on the device
  uint32_t ov_cap = 4096;
  uint64_t max_retained = 0;     // max_retained_messages (:230-240); 0: no limit
  bool reset = true;             // the image is to be dropped (a new store, clean)
  bool ov_dirty = false;         // the device overlay is out of date
  struct {
    int rebuilt = 0;
    uint64_t patched = 0, tombstoned = 0, overlay = 0, dead = 0, h2d = 0;
  } last;
  // committed image
  DevBuf nodes, edges, dict, dict_blob, dict_off, msg, expiry;
  RetainView view{};
  DevTable dtab{};
  uint64_t n_nodes = 0;
  // overlay and patch staging
  DevBuf ovbuf, pbuf, xout, xn;
  RetainOverlay ov{};
  // per-batch workspace
  DevBuf in_blob, in_off, wid, lv, tfl, pf[2], pn[2], pc, paux, poff, tiles, rf, rlo, rhi, nr, alive, apre, fcnt, roff,
      row, ids, ovmask, ovbase;

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
  int hip_fail(hipError_t e, const char* where) {
    err = std::string(where) + ": " + hipGetErrorString(e);
    return EGM_E_DEVICE;
  }
  void touch(Rec& x) {
    if (!x.dirty) touched.push_back(x.rank);
    x.dirty = true;
  }
  void ov_remove(Rec& x) {
    Ent* last = ov_ents.back();
    ov_ents[x.ov] = last;
    last->second.ov = x.ov;
    ov_ents.pop_back();
    ov_dirty = true;
  }
};
#pragma GCC diagnostic pop

// A full image from `ents` (the live records); the overlay and the tombstones are gone afterwards.
static int rs_upload_image(egm_rstore* r, const std::vector<Ent*>& ents, uint64_t* h2d) {
  Image im;
  build_image(ents, &im, &r->by_rank);
  hipError_t e;
  hipStreamSynchronize(r->stream);
  if ((e = put_vec(r->nodes, im.nodes)) || (e = put_vec(r->edges, im.edges)) || (e = put_vec(r->dict, im.dict)) ||
      (e = put_vec(r->dict_blob, im.dict_blob)) || (e = put_vec(r->dict_off, im.dict_off)) ||
      (e = put_vec(r->msg, im.msg)) || (e = put_vec(r->expiry, im.expiry)))
    return r->hip_fail(e, "retained image upload");
  *h2d += im.nodes.size() * 16 + im.edges.size() * 16 + im.dict.size() * sizeof(DictSlot) + im.dict_blob.size() +
          im.dict_off.size() * 8 + im.msg.size() * 12;
  r->view.nodes = r->nodes.as<uint4>();
  r->view.edges = r->edges.as<uint4>();
  r->view.edge_mask = im.edge_mask;
  r->view.msg = r->msg.as<uint32_t>();
  r->view.expiry = r->expiry.as<uint64_t>();
  r->view.n_topics = (uint32_t)im.msg.size();
  r->dtab = DevTable{};
  r->dtab.dict = r->dict.as<DictSlot>();
  r->dtab.dict_mask = (uint32_t)(im.dict.size() - 1);
  r->dtab.dict_blob = r->dict_blob.as<uint8_t>();
  r->dtab.dict_off = r->dict_off.as<uint64_t>();
  r->n_nodes = im.nodes.size();
  r->dead_ranks = 0;
  r->touched.clear();
  r->reset = false;
  return EGM_OK;
}

// The overlay as one device block: expiry[P] | off[P + 1] | levels[P] | msg[P] | topic bytes.
static int rs_upload_overlay(egm_rstore* r, uint64_t* h2d) {
  const size_t P = r->ov_ents.size();
  uint64_t bytes = 0;
  for (const Ent* e : r->ov_ents) bytes += e->first.size();
  if (bytes > 0xFFFFFFF0ull) return r->fail(EGM_E_NOMEM, "overlay topics exceed 4 GiB (lower the overlay cap)");
  const size_t o_off = P * 8, o_lv = o_off + (P + 1) * 4, o_msg = o_lv + P * 4, o_blob = o_msg + P * 4;
  std::vector<uint8_t> h(o_blob + bytes);
  uint64_t* ex = (uint64_t*)h.data();
  uint32_t* off = (uint32_t*)(h.data() + o_off);
  uint32_t* lv = (uint32_t*)(h.data() + o_lv);
  uint32_t* msg = (uint32_t*)(h.data() + o_msg);
  uint32_t at = 0;
  for (size_t p = 0; p < P; ++p) {
    const std::string& t = r->ov_ents[p]->first;
    const Rec& x = r->ov_ents[p]->second;
    ex[p] = x.expiry;
    off[p] = at;
    lv[p] = 1 + (uint32_t)std::count(t.begin(), t.end(), '/');
    msg[p] = x.msg;
    if (!t.empty()) memcpy(h.data() + o_blob + at, t.data(), t.size());
    at += (uint32_t)t.size();
  }
  off[P] = at;
  hipError_t e;
  if ((e = r->ovbuf.ensure(h.size() + 16)) ||
      (e = hipMemcpyAsync(r->ovbuf.p, h.data(), h.size(), hipMemcpyHostToDevice, r->stream)) ||
      (e = hipStreamSynchronize(r->stream)))   // h is pageable and goes out of scope
    return r->hip_fail(e, "overlay upload");
  *h2d += h.size();
  uint8_t* d = r->ovbuf.as<uint8_t>();
  r->ov.expiry = (const uint64_t*)d;
  r->ov.off = (const uint32_t*)(d + o_off);
  r->ov.levels = (const uint32_t*)(d + o_lv);
  r->ov.msg = (const uint32_t*)(d + o_msg);
  r->ov.blob = d + o_blob;
  r->ov.n = (uint32_t)P;
  r->ov_dirty = false;
  return EGM_OK;
}

// Bring the device up to the host records: patches and tombstones in place,
// new topics through the overlay.  A rebuild only when asked for, when the
// overlay outgrew its cap (cap 0: at every change), or when the tombstones
// outnumber the image's live ranks (the rule of egm_subs_commit).  No match
// is in flight: the store is one mutex, and a match ends synchronised.
static int rs_commit_locked(egm_rstore* r, bool force = false) {
  const bool changed = r->reset || r->ov_dirty || !r->touched.empty();
  uint64_t dead = r->dead_ranks;
  for (uint32_t rank : r->touched) {
    const Rec& x = r->by_rank[rank]->second;
    dead += (uint64_t)x.dead - (uint64_t)x.dev_dead;
  }
  const bool rebuild = force || (changed && r->ov_cap == 0) || r->ov_ents.size() > r->ov_cap ||
                       dead > r->by_rank.size() - dead;
  if (!changed && !rebuild) return EGM_OK;
  uint64_t h2d = 0, patched = 0, tombstoned = 0;
  int rc;
  if (rebuild) {
    std::vector<Ent*> ents;
    ents.reserve(r->n_live);
    for (auto it = r->recs.begin(); it != r->recs.end();) {
      if (it->second.dead) {
        it = r->recs.erase(it);
      } else {
        ents.push_back(&*it);
        ++it;
      }
    }
    r->ov_ents.clear();
    if ((rc = rs_upload_image(r, ents, &h2d))) return rc;
    r->ov.n = 0;
    r->ov_dirty = false;
  } else {
    if (r->reset && (rc = rs_upload_image(r, {}, &h2d))) return rc;   // the empty image: no record is read
    const size_t k = r->touched.size();
    if (k) {   // expiry[k] | rank[k] | msg[k], scattered by k_patch on the store's stream
      std::vector<uint8_t> h(k * 16);
      uint64_t* ex = (uint64_t*)h.data();
      uint32_t* idx = (uint32_t*)(h.data() + k * 8);
      uint32_t* msg = idx + k;
      for (size_t i = 0; i < k; ++i) {
        Rec& x = r->by_rank[r->touched[i]]->second;
        idx[i] = x.rank;
        ex[i] = x.expiry;
        msg[i] = x.dead ? RS_TOMB : x.msg;
        if (!x.dead) ++patched;
        else if (!x.dev_dead) ++tombstoned;
        x.dev_dead = x.dead;
        x.dirty = false;
      }
      r->dead_ranks = dead;
      r->touched.clear();
      hipError_t e;
      if ((e = r->pbuf.ensure(h.size()))) return r->hip_fail(e, "retained patch");
      const uint8_t* d = r->pbuf.as<uint8_t>();
      const uint32_t* d_idx = (const uint32_t*)(d + k * 8);
      if ((e = hipMemcpyAsync(r->pbuf.p, h.data(), h.size(), hipMemcpyHostToDevice, r->stream)) ||
          (e = launch_patch(r->expiry.p, 8, d_idx, d, k, r->stream)) ||
          (e = launch_patch(r->msg.p, 4, d_idx, d + k * 12, k, r->stream)) ||
          (e = hipStreamSynchronize(r->stream)))   // h is pageable and goes out of scope
        return r->hip_fail(e, "retained patch");
      h2d += h.size();
    }
    if (r->ov_dirty && (rc = rs_upload_overlay(r, &h2d))) return rc;
  }
  r->last.rebuilt = rebuild ? 1 : 0;
  r->last.patched = patched;
  r->last.tombstoned = tombstoned;
  r->last.overlay = r->ov_ents.size();
  r->last.dead = r->dead_ranks;
  r->last.h2d = h2d;
  return EGM_OK;
}

static bool has_wildcard_word(const uint8_t* p, uint32_t len) {
  uint32_t ws = 0;
  for (uint32_t i = 0; i <= len; ++i) {
    if (i < len && p[i] != '/') continue;
    if (i - ws == 1 && (p[ws] == '+' || p[ws] == '#')) return true;
    ws = i + 1;
  }
  return false;
}

// a batch of filters as blob + offsets[n + 1], the argument form of the match and of the delete
static bool rs_filters_ok(const uint8_t* blob, const uint32_t* off, uint32_t n) {
  if (n && !off) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return !(n && !blob && off[n] > off[0]);
}

// The frontier walk of a batch of filters over the committed image, shared by
// egm_rstore_match and egm_rstore_delete_matching: the filters go to the
// device (in_blob, in_off) and are tokenised, then k_rs_init and one k_rs_step /
// scan / k_rs_fill round per level; a range list that overflows is walked again
// with room.  On return *w describes the batch, w->rf/rlo/rhi hold *n_ranges
// ranges, w->fcnt[n + 1] is allocated and the stream is synchronised.
// with_alive: also the alive flags at `now` and their scan (w->alive, w->apre),
// which the match's rows count from.
static int rs_walk(egm_rstore* r, const uint8_t* blob, const uint32_t* off, uint32_t n, uint64_t now, bool ge_plain,
                   bool with_alive, RetainWork* wp, uint32_t* n_ranges_out) {
  RetainWork& w = *wp;
  hipStream_t s = r->stream;
  hipError_t e;
  const uint32_t base0 = n ? off[0] : 0;
  const uint64_t bytes = n ? (uint64_t)off[n] - base0 : 0;
  std::vector<uint32_t> loff(n + 1);
  for (uint32_t i = 0; i <= n; ++i) loff[i] = n ? off[i] - base0 : 0;
  const uint32_t M = r->view.n_topics;
  const size_t nn = (size_t)n + 1;
  if ((e = r->in_blob.ensure(bytes + 16)) || (e = r->in_off.ensure(nn * 4)) ||
      (e = r->wid.ensure((bytes + nn) * 4)) || (e = r->lv.ensure(nn * 4)) || (e = r->tfl.ensure(nn)) ||
      (with_alive && ((e = r->alive.ensure(((size_t)M + 1) * 4)) || (e = r->apre.ensure(((size_t)M + 2) * 8)))) ||
      (e = r->fcnt.ensure(nn * 4)) || (e = r->nr.ensure(16)))
    return r->hip_fail(e, "retained workspace");
  if (bytes && (e = hipMemcpyAsync(r->in_blob.p, blob + base0, bytes, hipMemcpyHostToDevice, s)))
    return r->hip_fail(e, "H2D filters");
  if ((e = hipMemcpyAsync(r->in_off.p, loff.data(), nn * 4, hipMemcpyHostToDevice, s)))
    return r->hip_fail(e, "H2D offsets");

  w.off = r->in_off.as<uint32_t>();
  w.wid = r->wid.as<uint32_t>();
  w.lv = r->lv.as<uint32_t>();
  w.tfl = r->tfl.as<uint8_t>();
  w.alive = with_alive ? r->alive.as<uint32_t>() : nullptr;
  w.apre = with_alive ? r->apre.as<uint64_t>() : nullptr;
  w.fcnt = r->fcnt.as<uint32_t>();
  w.n_ranges = r->nr.as<uint32_t>();
  w.now = now;
  w.ge_plain = ge_plain;
  auto tiles_for = [&](uint64_t m) { return (scan_tiles((uint32_t)std::min<uint64_t>(m, 0xFFFFFFFFull)) + 2) * 8; };
  size_t tiles_need = std::max(tiles_for(with_alive ? M : 0), tiles_for(n));
  if ((e = r->tiles.ensure(tiles_need))) return r->hip_fail(e, "tiles");
  w.tiles = r->tiles.as<uint64_t>();

  if ((e = launch_tokenise(r->dtab, r->in_blob.as<uint8_t>(), bytes, w.off, n, r->wid.as<uint32_t>(), r->lv.as<uint32_t>(),
                           r->tfl.as<uint8_t>(), s)) ||
      (with_alive && (e = launch_rs_alive(r->view, w, s))))
    return r->hip_fail(e, "tokenise/alive");

  // frontier walk, level by level; ranges may overflow -> rerun with room
  uint64_t range_cap = std::max<uint64_t>(4 * (uint64_t)n + 1024, r->rf.cap / 4);
  uint32_t n_ranges = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (range_cap > 0xFFFFFFF0ull) return r->fail(EGM_E_NOMEM, "too many result ranges in one batch");
    if ((e = r->rf.ensure(range_cap * 4)) || (e = r->rlo.ensure(range_cap * 4)) || (e = r->rhi.ensure(range_cap * 4)) ||
        (e = r->roff.ensure(range_cap * 4)))
      return r->hip_fail(e, "ranges");
    w.rf = r->rf.as<uint32_t>();
    w.rlo = r->rlo.as<uint32_t>();
    w.rhi = r->rhi.as<uint32_t>();
    w.roff = r->roff.as<uint32_t>();
    w.range_cap = (uint32_t)range_cap;
    if ((e = hipMemsetAsync(w.n_ranges, 0, 4, s))) return r->hip_fail(e, "memset");
    uint64_t np = n;
    int cur = 0;
    if ((e = r->pf[0].ensure(nn * 4)) || (e = r->pn[0].ensure(nn * 4))) return r->hip_fail(e, "frontier");
    if ((e = launch_rs_init(n, r->pf[0].as<uint32_t>(), r->pn[0].as<uint32_t>(), s)))
      return r->hip_fail(e, "init");
    for (uint32_t level = 0; np; ++level) {
      if (np > 0xFFFFFFF0ull) return r->fail(EGM_E_NOMEM, "frontier too large (split the batch)");
      if ((e = r->pc.ensure((np + 1) * 4)) || (e = r->paux.ensure((np + 1) * 4)) ||
          (e = r->poff.ensure((np + 2) * 8)) || (e = r->tiles.ensure(std::max(tiles_need, tiles_for(np)))))
        return r->hip_fail(e, "level workspace");
      w.pc = r->pc.as<uint32_t>();
      w.paux = r->paux.as<uint32_t>();
      w.poff = r->poff.as<uint64_t>();
      w.tiles = r->tiles.as<uint64_t>();
      if ((e = launch_rs_level(r->view, w, level, (uint32_t)np, r->pf[cur].as<uint32_t>(), r->pn[cur].as<uint32_t>(),
                               s)))
        return r->hip_fail(e, "level");
      uint64_t nnext = 0;
      if ((e = hipMemcpyAsync(&nnext, w.poff + np, 8, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
        return r->hip_fail(e, "level readback");
      if (nnext) {
        if ((e = r->pf[cur ^ 1].ensure(nnext * 4 + 16)) || (e = r->pn[cur ^ 1].ensure(nnext * 4 + 16)))
          return r->hip_fail(e, "frontier");
        if ((e = launch_rs_fill(w, (uint32_t)np, nnext, r->pf[cur].as<uint32_t>(), r->pf[cur ^ 1].as<uint32_t>(),
                                r->pn[cur ^ 1].as<uint32_t>(), s)))
          return r->hip_fail(e, "fill");
        // the next level may grow (reallocate) the buffers this fill reads
        if ((e = hipStreamSynchronize(s))) return r->hip_fail(e, "fill sync");
      }
      cur ^= 1;
      np = nnext;
    }
    if ((e = hipMemcpyAsync(&n_ranges, w.n_ranges, 4, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
      return r->hip_fail(e, "ranges readback");
    if (n_ranges <= range_cap) break;
    range_cap = (uint64_t)n_ranges + n_ranges / 4 + 1024;
    if (attempt == 1) return r->fail(EGM_E_NOMEM, "ranges capacity");
  }
  *n_ranges_out = n_ranges;
  return EGM_OK;
}

extern "C" {

int egm_rstore_open(int device, egm_rstore** out) {
  if (!out) return EGM_E_INVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return EGM_E_DEVICE;
  egm_rstore* r = new (std::nothrow) egm_rstore();
  if (!r) return EGM_E_NOMEM;
  r->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) {
    delete r;
    return EGM_E_DEVICE;
  }
  if (rs_commit_locked(r) != EGM_OK) {
    hipStreamDestroy(r->stream);
    delete r;
    return EGM_E_DEVICE;
  }
  *out = r;
  return EGM_OK;
}

void egm_rstore_close(egm_rstore* r) {
  if (!r) return;
  hipSetDevice(r->device);
  hipStreamSynchronize(r->stream);
  hipStreamDestroy(r->stream);
  delete r;
}

const char* egm_rstore_last_error(egm_rstore* r) { return r ? r->err.c_str() : "null store"; }

int egm_rstore_put(egm_rstore* r, const uint8_t* topic, uint32_t len, uint32_t msg_id, uint64_t expiry_ms) {
  if (!r || (!topic && len)) return EGM_E_INVAL;
  if (msg_id == RS_TOMB) return EGM_E_INVAL;               // the image's tombstone mark
  if (has_wildcard_word(topic, len)) return EGM_E_INVAL;   // publish topics carry no wildcard
  std::lock_guard<std::mutex> g(r->mu);
  std::string key((const char*)topic, len);
  if (r->max_retained && r->n_live >= r->max_retained) {   // is_table_full/0: only a held topic is written (:82-98)
    auto held = r->recs.find(key);
    if (held == r->recs.end() || held->second.dead) return r->fail(EGM_E_FULL, "the retained table is full");
  }
  auto [it, fresh] = r->recs.try_emplace(std::move(key));
  Rec& x = it->second;
  if (fresh) {                       // not in the image: the overlay
    x.ov = (uint32_t)r->ov_ents.size();
    r->ov_ents.push_back(&*it);
    ++r->n_live;
  } else if (x.rank != NONE) {       // patch the rank; a tombstoned one comes back
    if (x.dead) ++r->n_live;
    x.dead = false;
    r->touch(x);
  }
  if (x.rank == NONE) r->ov_dirty = true;
  x.msg = msg_id;
  x.expiry = expiry_ms;
  return EGM_OK;
}

int egm_rstore_delete(egm_rstore* r, const uint8_t* topic, uint32_t len) {
  if (!r || (!topic && len)) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  auto it = r->recs.find(std::string((const char*)topic, len));
  if (it == r->recs.end() || it->second.dead) return EGM_OK;
  Rec& x = it->second;
  --r->n_live;
  if (x.rank != NONE) {
    x.dead = true;
    r->touch(x);
  } else {
    r->ov_remove(x);
    r->recs.erase(it);
  }
  return EGM_OK;
}

int egm_rstore_clean(egm_rstore* r) {
  if (!r) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  r->recs.clear();
  r->by_rank.clear();
  r->ov_ents.clear();
  r->touched.clear();
  r->n_live = r->dead_ranks = 0;
  r->reset = r->ov_dirty = true;
  return EGM_OK;
}

int egm_rstore_size(egm_rstore* r, uint64_t* n) {
  if (!r || !n) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  *n = r->n_live;
  return EGM_OK;
}

int egm_rstore_commit(egm_rstore* r) {
  if (!r) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  if (hipSetDevice(r->device) != hipSuccess) return EGM_E_DEVICE;
  return rs_commit_locked(r);
}

int egm_rstore_rebuild(egm_rstore* r) {
  if (!r) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  if (hipSetDevice(r->device) != hipSuccess) return EGM_E_DEVICE;
  return rs_commit_locked(r, true);
}

int egm_rstore_set_overlay_cap(egm_rstore* r, uint32_t max_topics) {
  if (!r) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  r->ov_cap = max_topics;
  return EGM_OK;
}

int egm_rstore_set_max_retained(egm_rstore* r, uint64_t max) {
  if (!r) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  r->max_retained = max;
  return EGM_OK;
}

int egm_rstore_last_commit(egm_rstore* r, int* rebuilt, uint64_t* patched, uint64_t* tombstoned,
                           uint64_t* overlay_topics, uint64_t* dead_ranks, uint64_t* h2d_bytes) {
  if (!r || !rebuilt || !patched || !tombstoned || !overlay_topics || !dead_ranks || !h2d_bytes) return EGM_E_INVAL;
  std::lock_guard<std::mutex> g(r->mu);
  *rebuilt = r->last.rebuilt;
  *patched = r->last.patched;
  *tombstoned = r->last.tombstoned;
  *overlay_topics = r->last.overlay;
  *dead_ranks = r->last.dead;
  *h2d_bytes = r->last.h2d;
  return EGM_OK;
}

int egm_rstore_clear_expired(egm_rstore* r, uint64_t now_ms, uint32_t** msg_ids, uint64_t* n) {
  if (!r || !msg_ids || !n) return EGM_E_INVAL;
  *msg_ids = nullptr;
  *n = 0;
  std::lock_guard<std::mutex> g(r->mu);
  if (hipSetDevice(r->device) != hipSuccess) return EGM_E_DEVICE;
  int rc = rs_commit_locked(r);   // the device's expiry[] and tombstones are the records'
  if (rc) return rc;
  hipStream_t s = r->stream;
  hipError_t e;
  const uint32_t M = r->view.n_topics;
  uint32_t k = 0;
  std::vector<uint32_t> ranks;
  if ((e = r->xout.ensure((size_t)M * 4 + 16)) || (e = r->xn.ensure(16)) ||
      (e = launch_rs_expire(r->expiry.as<uint64_t>(), r->msg.as<uint32_t>(), M, now_ms, r->xout.as<uint32_t>(),
                            r->xn.as<uint32_t>(), s)) ||
      (e = hipMemcpyAsync(&k, r->xn.p, 4, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
    return r->hip_fail(e, "expire");
  ranks.resize(k);
  if (k && ((e = hipMemcpyAsync(ranks.data(), r->xout.p, (size_t)k * 4, hipMemcpyDeviceToHost, s)) ||
            (e = hipStreamSynchronize(s))))
    return r->hip_fail(e, "expire readback");
  std::vector<uint32_t> gone;
  gone.reserve(k);
  for (uint32_t rank : ranks) {      // the kernel made these ranks tombstones
    Rec& x = r->by_rank[rank]->second;
    gone.push_back(x.msg);
    x.dead = x.dev_dead = true;
  }
  r->dead_ranks += k;
  for (size_t p = r->ov_ents.size(); p-- > 0;) {   // the overlay, on the host
    Ent* en = r->ov_ents[p];
    if (en->second.expiry == 0 || en->second.expiry >= now_ms) continue;
    gone.push_back(en->second.msg);
    r->ov_remove(en->second);
    r->recs.erase(r->recs.find(en->first));
  }
  r->n_live -= gone.size();
  if (gone.empty()) return EGM_OK;
  uint32_t* mem = (uint32_t*)result_alloc(gone.size() * 4);
  if (!mem) return r->fail(EGM_E_NOMEM, "result");
  memcpy(mem, gone.data(), gone.size() * 4);
  *msg_ids = mem;
  *n = gone.size();
  return EGM_OK;
}

int egm_rstore_delete_matching(egm_rstore* r, const uint8_t* blob, const uint32_t* off, uint32_t n, uint32_t** msg_ids,
                               uint64_t* n_ids) {
  if (!r || !msg_ids || !n_ids) return EGM_E_INVAL;
  if (!rs_filters_ok(blob, off, n)) return EGM_E_INVAL;
  *msg_ids = nullptr;
  *n_ids = 0;
  std::lock_guard<std::mutex> g(r->mu);
  if (hipSetDevice(r->device) != hipSuccess) return EGM_E_DEVICE;
  int rc = rs_commit_locked(r);   // the device's image, tombstones and overlay are the records'
  if (rc) return rc;
  if (!n || !r->n_live) return EGM_OK;
  hipStream_t s = r->stream;
  hipError_t e;
  // now = 0: rs_alive holds for every expiry, so the walk emits every rank a
  // filter matches, expired or not (:209-211); no alive scan is needed
  RetainWork w{};
  uint32_t nr = 0;
  if ((rc = rs_walk(r, blob, off, n, 0, false, false, &w, &nr))) return rc;

  // the image: one exchange per covered rank
  const uint32_t M = r->view.n_topics;
  uint32_t k = 0;
  std::vector<uint2> killed;
  if (nr) {
    uint64_t total = 0;
    if ((e = r->pc.ensure(((size_t)nr + 1) * 4)) || (e = r->poff.ensure(((size_t)nr + 2) * 8)) ||
        (e = r->tiles.ensure((scan_tiles(nr) + 2) * 8)) || (e = r->xout.ensure((size_t)M * 8 + 16)) ||
        (e = r->xn.ensure(16)))
      return r->hip_fail(e, "kill workspace");
    w.tiles = r->tiles.as<uint64_t>();
    uint64_t* koff = r->poff.as<uint64_t>();
    if ((e = launch_rs_kill_scan(w, nr, r->pc.as<uint32_t>(), koff, s)) ||
        (e = hipMemcpyAsync(&total, koff + nr, 8, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
      return r->hip_fail(e, "kill scan");
    if ((e = launch_rs_kill(w, nr, koff, total, M, r->msg.as<uint32_t>(), r->xout.as<uint2>(), r->xn.as<uint32_t>(),
                            s)) ||
        (e = hipMemcpyAsync(&k, r->xn.p, 4, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
      return r->hip_fail(e, "kill");
    killed.resize(k);
    if (k && ((e = hipMemcpyAsync(killed.data(), r->xout.p, (size_t)k * 8, hipMemcpyDeviceToHost, s)) ||
              (e = hipStreamSynchronize(s))))
      return r->hip_fail(e, "kill readback");
  }
  std::vector<uint32_t> gone;
  gone.reserve(k);
  for (const uint2& kr : killed) {   // {rank, the id it held}: the kernel made these ranks tombstones
    Rec& x = r->by_rank[kr.x]->second;
    gone.push_back(kr.y);
    x.dead = x.dev_dead = true;
  }
  r->dead_ranks += k;

  // the overlay: the byte match's masks, OR-ed per tile over the batch
  RetainOverlay ov = r->ov;
  const uint32_t ov_tiles = (ov.n + 63) / 64;
  if (ov_tiles) {
    const uint64_t ov_pairs = (uint64_t)n * ov_tiles;
    if ((e = r->ovmask.ensure(ov_pairs * 8 + 16)) || (e = r->ovbase.ensure(ov_pairs * 4 + 16)))
      return r->hip_fail(e, "overlay workspace");
    ov.mask = r->ovmask.as<uint64_t>();
    ov.base = r->ovbase.as<uint32_t>();
    std::vector<uint64_t> masks(ov_pairs), hit(ov_tiles, 0);
    if ((e = launch_rs_ov_masks(w, ov, r->in_blob.as<uint8_t>(), n, s)) ||
        (e = hipMemcpyAsync(masks.data(), ov.mask, ov_pairs * 8, hipMemcpyDeviceToHost, s)) ||
        (e = hipStreamSynchronize(s)))
      return r->hip_fail(e, "overlay masks");
    for (uint64_t q = 0; q < ov_pairs; ++q) hit[q % ov_tiles] |= masks[q];
    for (size_t p = r->ov_ents.size(); p-- > 0;) {   // downwards: ov_remove moves the last entry into the hole
      if (!((hit[p >> 6] >> (p & 63)) & 1)) continue;
      Ent* en = r->ov_ents[p];
      gone.push_back(en->second.msg);
      r->ov_remove(en->second);
      r->recs.erase(r->recs.find(en->first));
    }
  }
  r->n_live -= gone.size();
  if (gone.empty()) return EGM_OK;
  uint32_t* mem = (uint32_t*)result_alloc(gone.size() * 4);
  if (!mem) return r->fail(EGM_E_NOMEM, "result");
  memcpy(mem, gone.data(), gone.size() * 4);
  *msg_ids = mem;
  *n_ids = gone.size();
  return EGM_OK;
}

int egm_rstore_match(egm_rstore* r, const uint8_t* blob, const uint32_t* off, uint32_t n, uint64_t now_ms, int mode,
                     egm_result** out) {
  if (!r || !out || (mode != EGM_RMODE_MATCH && mode != EGM_RMODE_DISPATCH)) return EGM_E_INVAL;
  if (!rs_filters_ok(blob, off, n)) return EGM_E_INVAL;
  *out = nullptr;
  std::lock_guard<std::mutex> g(r->mu);
  if (hipSetDevice(r->device) != hipSuccess) return EGM_E_DEVICE;
  int rc = rs_commit_locked(r);   // queries see every put/delete made before them
  if (rc) return rc;
  hipStream_t s = r->stream;
  hipError_t e;
  const size_t nn = (size_t)n + 1;
  if ((e = r->row.ensure(nn * 8))) return r->hip_fail(e, "retained workspace");
  RetainWork w{};
  uint32_t n_ranges = 0;
  if ((rc = rs_walk(r, blob, off, n, now_ms, mode == EGM_RMODE_DISPATCH, true, &w, &n_ranges))) return rc;
  uint64_t* d_row = r->row.as<uint64_t>();
  RetainOverlay ov = r->ov;   // one mask and base per (filter, tile of 64 overlay topics)
  const uint64_t ov_pairs = (uint64_t)n * ((ov.n + 63) / 64);
  if ((e = r->ovmask.ensure(ov_pairs * 8 + 16)) || (e = r->ovbase.ensure(ov_pairs * 4 + 16)))
    return r->hip_fail(e, "overlay workspace");
  ov.mask = r->ovmask.as<uint64_t>();
  ov.base = r->ovbase.as<uint32_t>();
  if ((e = launch_rs_rows(w, ov, r->in_blob.as<uint8_t>(), n_ranges, n, d_row, s))) return r->hip_fail(e, "rows");
  uint64_t total = 0;
  if ((e = hipMemcpyAsync(&total, d_row + n, 8, hipMemcpyDeviceToHost, s)) || (e = hipStreamSynchronize(s)))
    return r->hip_fail(e, "rows readback");
  if ((e = r->ids.ensure(total * 4 + 16))) return r->hip_fail(e, "ids");
  if ((e = launch_rs_expand(r->view, w, n_ranges, d_row, r->ids.as<uint32_t>(), s)) ||
      (e = launch_rs_ov_fill(ov, n, d_row, r->ids.as<uint32_t>(), s)))
    return r->hip_fail(e, "expand");

  size_t sz = sizeof(egm_result);
  const size_t o_counts = sz;
  sz += ((uint64_t)n * 4 + 7) & ~7ull;
  const size_t o_row = sz;
  sz += nn * 8;
  const size_t o_ids = sz;
  sz += (total * 4 + 7) & ~7ull;
  const size_t o_flags = sz;
  sz += n + 8;
  uint8_t* mem = (uint8_t*)result_alloc(sz);
  if (!mem) return r->fail(EGM_E_NOMEM, "result");
  egm_result* res = (egm_result*)mem;
  memset(res, 0, sizeof(*res));
  res->n_topics = n;
  res->n_ids = total;
  res->counts = (uint32_t*)(mem + o_counts);
  res->row_ptr = (uint64_t*)(mem + o_row);
  res->ids = (uint32_t*)(mem + o_ids);
  res->flags = (uint8_t*)(mem + o_flags);
  if ((e = hipMemcpyAsync(res->row_ptr, d_row, nn * 8, hipMemcpyDeviceToHost, s)) ||
      (total && (e = hipMemcpyAsync(res->ids, r->ids.p, total * 4, hipMemcpyDeviceToHost, s))) ||
      (n && (e = hipMemcpyAsync(res->flags, r->tfl.p, n, hipMemcpyDeviceToHost, s))) ||
      (e = hipStreamSynchronize(s))) {
    result_discard(mem);
    return r->hip_fail(e, "D2H result");
  }
  for (uint32_t i = 0; i < n; ++i) res->counts[i] = (uint32_t)(res->row_ptr[i + 1] - res->row_ptr[i]);
  res->visited = n_ranges;
  *out = res;
  return EGM_OK;
}

}  // extern "C"
