/*
 * emqx_gpu_match_nif.c — Erlang NIF shim over libemqx_gpu_match.so.
 *
 * Binds the C-ABI in include/emqx_gpu_match.h to the Erlang module
 * erl/emqx_gpu_match.erl.  Written against the documented erl_nif API; it
 * compiles only where an ERTS include directory exists (there is none in the
 * build container: see INTEGRATION.md for the command line).
 *
 * Mapping to the reference (EMQ X 5.0-alpha.3):
 *   open/1          -> egm_open            (one context per node, device ordinal)
 *   build/2         -> egm_table_build     (bulk load of the route filters)
 *   apply_delta/3   -> egm_table_apply_delta + egm_table_commit
 *                      (emqx_trie:insert/1, delete/1 — apps/emqx/src/emqx_trie.erl:82-96)
 *   match_batch/3   -> egm_match_batch     (emqx_trie:match/1 and the filter set of
 *                      emqx_router:match_routes/1 — emqx_router.erl:129-141 — for a
 *                      list of publish topics; returns [[FilterId]])
 *   submit/3, wait/2 -> egm_match_submit / egm_match_wait (the batcher's pipeline:
 *                      submit returns a ticket at once, wait blocks for its rows).
 *                      The ticket is a resource: collected unwaited (its waiter
 *                      died), its destructor calls egm_match_cancel, so a dead
 *                      waiter never keeps a pipeline slot busy.
 *   cancel/2        -> egm_match_cancel
 *   subs_delta/3    -> egm_subs_apply_delta + egm_subs_commit (subscriber changes)
 *   subs_build/2    -> egm_subs_build      (filter id -> subscriber ids: the
 *                      emqx_subscriber bag flattened, emqx_broker.erl:116-162)
 *   publish_batch/2 -> egm_match_batch (routes mode) + egm_fanout_batch: the
 *                      match_routes/1 + dispatch/2 expansion of emqx_broker:publish/1
 *                      (emqx_broker.erl:200-209, 283-308) for a list of topics;
 *                      returns [{[FilterId], [{FilterId, Sub}]}]
 *   subs_set_dead/3 -> egm_subs_set_dead   (is_process_alive/1 of dispatch/3,
 *                      emqx_broker.erl:297-302, as a device bitmap)
 *   share_build/2, share_delta/3 -> egm_share_build / egm_share_apply_delta +
 *                      egm_share_commit (emqx_shared_sub's member table,
 *                      emqx_shared_sub.erl:108-118, 292-300)
 *   dispatch_batch/5 -> egm_match_batch (routes mode) + egm_dispatch_batch:
 *                      publish_batch/2 with the last step of dispatch/2 and
 *                      emqx_shared_sub:dispatch/3 done on the device (dead
 *                      subscribers dropped, one live member picked per group,
 *                      emqx_shared_sub.erl:239-290; live counts per filter,
 *                      emqx_broker.erl:283-295)
 *
 * The retained store (apps/emqx_retainer/src/emqx_retainer_mnesia.erl), a
 * resource of its own beside the route context:
 *   rs_open/1            -> egm_rstore_open
 *   rs_put/4             -> egm_rstore_put           (store_retained/2 :73-101;
 *                           {error, full} is is_table_full/0's refusal :92-97)
 *   rs_delete/2          -> egm_rstore_delete        (delete_message/2, plain topic :117-127)
 *   rs_delete_matching/2 -> egm_rstore_delete_matching (delete_message/2 with
 *                           wildcard filters :114-116, 206-212; returns the dropped ids)
 *   rs_set_max_retained/2 -> egm_rstore_set_max_retained (max_retained_messages :230-240)
 *   rs_clean/1           -> egm_rstore_clean         (clean/1 :148-150)
 *   rs_size/1            -> egm_rstore_size          (table_size/0 :238-240)
 *   rs_commit/1          -> egm_rstore_commit
 *   rs_clear_expired/2   -> egm_rstore_clear_expired (clear_expired/1 :103-112; NowMs is passed in)
 *   rs_match/4           -> egm_rstore_match         (match_messages/1 :200-204, or, Mode 1,
 *                           read_messages/1 :187-198 for plain topics; returns [[MsgId]])
 * Messages stay in Erlang: the store maps a topic to the caller's message id.
 *
 * Threading: match_batch and apply_delta run on dirty CPU schedulers
 * (ERL_NIF_DIRTY_JOB_CPU_BOUND) — a batch takes well over 1 ms.  The library
 * serialises calls per context.  Inputs (Erlang binaries) are borrowed only
 * for the duration of the call: they are packed into one contiguous buffer
 * here and the library copies them to device memory before returning.
 * Errors: bad arguments -> enif_make_badarg (the reference's function_clause);
 * library / device failures -> {error, Reason} so the caller can fall back to
 * emqx_trie:match/1.
 */
#include <erl_nif.h>
#include <stdlib.h>
#include <string.h>

#include "../include/emqx_gpu_match.h"

typedef struct {
  egm_ctx* ctx;
} egm_res_t;

static ErlNifResourceType* EGM_RES;
static ErlNifResourceType* EGM_TICKET;
static ErlNifResourceType* EGM_RSTORE;

typedef struct {
  egm_rstore* rs;
} egm_rs_t;

/* A submitted batch: keeps its context alive until it is waited or cancelled. */
typedef struct {
  egm_res_t* owner;   /* enif_keep_resource'd */
  uint64_t ticket;
  int live;           /* not yet waited or cancelled */
} egm_ticket_t;
static ERL_NIF_TERM ATOM_OK, ATOM_ERROR, ATOM_FULL;

static void egm_res_dtor(ErlNifEnv* env, void* obj) {
  (void)env;
  egm_res_t* r = (egm_res_t*)obj;
  if (r->ctx) egm_close(r->ctx);
  r->ctx = NULL;
}

static void egm_ticket_dtor(ErlNifEnv* env, void* obj) {
  (void)env;
  egm_ticket_t* t = (egm_ticket_t*)obj;
  if (t->live && t->owner && t->owner->ctx) egm_match_cancel(t->owner->ctx, t->ticket);
  t->live = 0;
  if (t->owner) enif_release_resource(t->owner);
  t->owner = NULL;
}

static void egm_rs_dtor(ErlNifEnv* env, void* obj) {
  (void)env;
  egm_rs_t* r = (egm_rs_t*)obj;
  if (r->rs) egm_rstore_close(r->rs);
  r->rs = NULL;
}

static int load(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)priv;
  (void)info;
  EGM_RES = enif_open_resource_type(env, NULL, "emqx_gpu_match_ctx", egm_res_dtor,
                                    ERL_NIF_RT_CREATE | ERL_NIF_RT_TAKEOVER, NULL);
  EGM_TICKET = enif_open_resource_type(env, NULL, "emqx_gpu_match_ticket", egm_ticket_dtor,
                                       ERL_NIF_RT_CREATE | ERL_NIF_RT_TAKEOVER, NULL);
  EGM_RSTORE = enif_open_resource_type(env, NULL, "emqx_gpu_match_rstore", egm_rs_dtor,
                                       ERL_NIF_RT_CREATE | ERL_NIF_RT_TAKEOVER, NULL);
  ATOM_OK = enif_make_atom(env, "ok");
  ATOM_ERROR = enif_make_atom(env, "error");
  ATOM_FULL = enif_make_atom(env, "full");
  return (EGM_RES && EGM_TICKET && EGM_RSTORE) ? 0 : -1;
}

static ERL_NIF_TERM error_tuple(ErlNifEnv* env, egm_ctx* ctx, int rc) {
  const char* msg = ctx ? egm_last_error(ctx) : "egm error";
  return enif_make_tuple2(env, ATOM_ERROR,
                          enif_make_tuple2(env, enif_make_int(env, rc), enif_make_string(env, msg, ERL_NIF_LATIN1)));
}

/* Pack a proper list of binaries into blob + offsets (caller frees). */
static int pack_list(ErlNifEnv* env, ERL_NIF_TERM list, uint8_t** blob, uint32_t** off, uint32_t* n) {
  unsigned len;
  if (!enif_get_list_length(env, list, &len)) return 0;
  uint32_t* o = (uint32_t*)malloc(((size_t)len + 1) * sizeof(uint32_t));
  if (!o) return 0;
  size_t total = 0;
  ERL_NIF_TERM head, tail = list;
  ErlNifBinary bin;
  o[0] = 0;
  for (unsigned i = 0; i < len; ++i) {
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_inspect_binary(env, head, &bin) ||
        total + bin.size > 0xFFFFFFFFu) {
      free(o);
      return 0;
    }
    total += bin.size;
    o[i + 1] = (uint32_t)total;
  }
  uint8_t* b = (uint8_t*)malloc(total + 16);
  if (!b) {
    free(o);
    return 0;
  }
  tail = list;
  for (unsigned i = 0; i < len; ++i) {
    enif_get_list_cell(env, tail, &head, &tail);
    enif_inspect_binary(env, head, &bin);
    memcpy(b + o[i], bin.data, bin.size);
  }
  *blob = b;
  *off = o;
  *n = len;
  return 1;
}

static int get_ctx(ErlNifEnv* env, ERL_NIF_TERM t, egm_res_t** r) {
  return enif_get_resource(env, t, EGM_RES, (void**)r) && (*r)->ctx;
}

/* open(Device :: non_neg_integer()) -> {ok, Ctx} | {error, _} */
static ERL_NIF_TERM nif_open(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  int dev;
  if (argc != 1 || !enif_get_int(env, argv[0], &dev) || dev < 0) return enif_make_badarg(env);
  egm_config cfg = {dev, 1, 0, 1000};
  egm_ctx* ctx = NULL;
  int rc = egm_open(&cfg, &ctx);
  if (rc) return error_tuple(env, NULL, rc);
  egm_res_t* r = (egm_res_t*)enif_alloc_resource(EGM_RES, sizeof(egm_res_t));
  r->ctx = ctx;
  ERL_NIF_TERM term = enif_make_resource(env, r);
  enif_release_resource(r);
  return enif_make_tuple2(env, ATOM_OK, term);
}

/* build(Ctx, [Filter :: binary()]) -> ok | {error, _}   (ids = list positions) */
static ERL_NIF_TERM nif_build(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  uint8_t* blob;
  uint32_t *off, n;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !pack_list(env, argv[1], &blob, &off, &n))
    return enif_make_badarg(env);
  int rc = egm_table_build(r->ctx, blob, off, n, NULL);
  free(blob);
  free(off);
  return rc ? error_tuple(env, r->ctx, rc) : ATOM_OK;
}

/* apply_delta(Ctx, [{Filter, Id}] inserts, [Filter] deletes) -> {ok, Epoch} | {error, _} */
static ERL_NIF_TERM nif_apply_delta(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  if (argc != 3 || !get_ctx(env, argv[0], &r)) return enif_make_badarg(env);
  unsigned ni;
  if (!enif_get_list_length(env, argv[1], &ni)) return enif_make_badarg(env);
  ERL_NIF_TERM filters = enif_make_list(env, 0), head, tail = argv[1];
  uint32_t* ids = (uint32_t*)malloc(((size_t)ni + 1) * sizeof(uint32_t));
  for (unsigned i = 0; i < ni; ++i) {
    const ERL_NIF_TERM* tup;
    int arity;
    unsigned id;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_tuple(env, head, &arity, &tup) || arity != 2 ||
        !enif_get_uint(env, tup[1], &id)) {
      free(ids);
      return enif_make_badarg(env);
    }
    ids[i] = id;
    filters = enif_make_list_cell(env, tup[0], filters);
  }
  ERL_NIF_TERM rev;
  enif_make_reverse_list(env, filters, &rev);
  uint8_t *ib = NULL, *db = NULL;
  uint32_t *io = NULL, *dof = NULL, nin = 0, nd = 0;
  if (!pack_list(env, rev, &ib, &io, &nin) || !pack_list(env, argv[2], &db, &dof, &nd)) {
    free(ids);
    free(ib);
    free(io);
    return enif_make_badarg(env);
  }
  egm_delta ins = {ib, io, nin, ids}, del = {db, dof, nd, NULL};
  uint64_t epoch = 0;
  int rc = egm_table_apply_delta(r->ctx, &ins, &del);
  if (!rc) rc = egm_table_commit(r->ctx, &epoch);
  free(ids);
  free(ib);
  free(io);
  free(db);
  free(dof);
  if (rc) return error_tuple(env, r->ctx, rc);
  return enif_make_tuple2(env, ATOM_OK, enif_make_uint64(env, epoch));
}

/* Rows of a CSR as [[Id]] (shared by match_batch and wait); either result
   form — wait/2's batches are submitted packed (EGM_RESULT_PACKED). */
static ERL_NIF_TERM rows_term(ErlNifEnv* env, const egm_result* res) {
  ERL_NIF_TERM rows = enif_make_list(env, 0);
  for (uint32_t i = res->n_topics; i-- > 0;) {
    ERL_NIF_TERM row = enif_make_list(env, 0);
    for (uint64_t k = egm_result_row(res, i + 1); k-- > egm_result_row(res, i);)
      row = enif_make_list_cell(env, enif_make_uint(env, egm_result_id(res, k)), row);
    rows = enif_make_list_cell(env, row, rows);
  }
  return rows;
}

/* match_batch(Ctx, [Topic :: binary()], Mode :: 0 | 1) -> {ok, [[Id]]} | {error, _} */
static ERL_NIF_TERM nif_match_batch(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  int mode;
  uint8_t* blob;
  uint32_t *off, n;
  if (argc != 3 || !get_ctx(env, argv[0], &r) || !enif_get_int(env, argv[2], &mode) ||
      (mode != EGM_MODE_TRIE && mode != EGM_MODE_ROUTES) || !pack_list(env, argv[1], &blob, &off, &n))
    return enif_make_badarg(env);
  egm_result* res = NULL;
  int rc = egm_match_batch(r->ctx, blob, off, n, mode, &res);
  free(blob);
  free(off);
  if (rc && !res) return error_tuple(env, r->ctx, rc);
  if (rc) {
    egm_result_free(res);
    return error_tuple(env, r->ctx, rc);
  }
  ERL_NIF_TERM rows = rows_term(env, res);
  egm_result_free(res);
  return enif_make_tuple2(env, ATOM_OK, rows);
}

/* submit(Ctx, [Topic], Mode) -> {ok, Ticket} | {error, _}: the topics are
   staged in pinned memory before it returns; Ticket is a resource. */
static ERL_NIF_TERM nif_submit(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  int mode;
  uint8_t* blob;
  uint32_t *off, n;
  if (argc != 3 || !get_ctx(env, argv[0], &r) || !enif_get_int(env, argv[2], &mode) ||
      (mode != EGM_MODE_TRIE && mode != EGM_MODE_ROUTES) || !pack_list(env, argv[1], &blob, &off, &n))
    return enif_make_badarg(env);
  uint64_t ticket = 0;
  int rc = egm_match_submit(r->ctx, blob, off, n, mode | EGM_RESULT_PACKED, &ticket);
  free(blob);
  free(off);
  if (rc) return error_tuple(env, r->ctx, rc);
  egm_ticket_t* t = (egm_ticket_t*)enif_alloc_resource(EGM_TICKET, sizeof(egm_ticket_t));
  enif_keep_resource(r);
  t->owner = r;
  t->ticket = ticket;
  t->live = 1;
  ERL_NIF_TERM term = enif_make_resource(env, t);
  enif_release_resource(t);
  return enif_make_tuple2(env, ATOM_OK, term);
}

static int get_ticket(ErlNifEnv* env, ERL_NIF_TERM term, egm_res_t* r, egm_ticket_t** t) {
  return enif_get_resource(env, term, EGM_TICKET, (void**)t) && (*t)->live && (*t)->owner == r;
}

/* wait(Ctx, Ticket) -> {ok, [[Id]]} | {error, _} (a ticket is waited once) */
static ERL_NIF_TERM nif_wait(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  egm_ticket_t* t;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !get_ticket(env, argv[1], r, &t)) return enif_make_badarg(env);
  t->live = 0;   /* from here the library owns the outcome: no cancel in the destructor */
  egm_result* res = NULL;
  int rc = egm_match_wait(r->ctx, t->ticket, &res);
  if (rc) {
    if (res) egm_result_free(res);
    return error_tuple(env, r->ctx, rc);
  }
  ERL_NIF_TERM rows = rows_term(env, res);
  egm_result_free(res);
  return enif_make_tuple2(env, ATOM_OK, rows);
}

/* cancel(Ctx, Ticket) -> ok | {error, _}: give the batch up without its rows.
   A normal (not dirty) NIF: egm_match_cancel never blocks — while a build or
   commit holds the context it queues the cancel — so this call and the ticket
   destructor (run on whatever scheduler collects the ticket) return at once.
   Always ok for a ticket of this context: egm_match_cancel answers EGM_OK for
   a queued (unvalidated) cancel and EGM_E_STATE for a stale ticket only when
   the context happened to be free, so that difference is lock contention,
   not a result (include/emqx_gpu_match.h). */
static ERL_NIF_TERM nif_cancel(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  egm_ticket_t* t;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !get_ticket(env, argv[1], r, &t)) return enif_make_badarg(env);
  t->live = 0;
  int rc = egm_match_cancel(r->ctx, t->ticket);
  return (rc == EGM_OK || rc == EGM_E_STATE) ? ATOM_OK : error_tuple(env, r->ctx, rc);
}

/* subs_build(Ctx, [[Sub]]) -> ok | {error, _}: list position = filter id; a
   shared group is the integer GroupId bor 16#80000000. */
static ERL_NIF_TERM nif_subs_build(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  unsigned nf;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !enif_get_list_length(env, argv[1], &nf))
    return enif_make_badarg(env);
  uint64_t* row = (uint64_t*)malloc(((size_t)nf + 1) * sizeof(uint64_t));
  if (!row) return enif_make_badarg(env);
  ERL_NIF_TERM head, tail = argv[1];
  row[0] = 0;
  for (unsigned i = 0; i < nf; ++i) {
    unsigned len;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_list_length(env, head, &len)) {
      free(row);
      return enif_make_badarg(env);
    }
    row[i + 1] = row[i] + len;
  }
  uint32_t* subs = (uint32_t*)malloc((size_t)(row[nf] ? row[nf] : 1) * sizeof(uint32_t));
  if (!subs) {
    free(row);
    return enif_make_badarg(env);
  }
  tail = argv[1];
  for (unsigned i = 0; i < nf; ++i) {
    ERL_NIF_TERM h2, t2;
    enif_get_list_cell(env, tail, &head, &tail);
    t2 = head;
    for (uint64_t k = row[i]; k < row[i + 1]; ++k) {
      unsigned v;
      if (!enif_get_list_cell(env, t2, &h2, &t2) || !enif_get_uint(env, h2, &v)) {
        free(row);
        free(subs);
        return enif_make_badarg(env);
      }
      subs[k] = v;
    }
  }
  int rc = egm_subs_build(r->ctx, row, nf, subs);
  free(row);
  free(subs);
  return rc ? error_tuple(env, r->ctx, rc) : ATOM_OK;
}

/* [{FilterId, Sub}] -> egm_sub_pair[] (malloc'd; *n pairs); 0 on a bad term */
static int get_pairs(ErlNifEnv* env, ERL_NIF_TERM list, egm_sub_pair** out, unsigned* n) {
  ERL_NIF_TERM head, tail = list;
  if (!enif_get_list_length(env, list, n)) return 0;
  *out = (egm_sub_pair*)malloc(sizeof(egm_sub_pair) * (*n ? *n : 1));
  if (!*out) return 0;
  for (unsigned i = 0; i < *n; ++i) {
    const ERL_NIF_TERM* el;
    int arity;
    unsigned f, sub;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_tuple(env, head, &arity, &el) || arity != 2 ||
        !enif_get_uint(env, el[0], &f) || !enif_get_uint(env, el[1], &sub)) {
      free(*out);
      *out = NULL;
      return 0;
    }
    (*out)[i].fid = f;
    (*out)[i].sub = sub;
  }
  return 1;
}

/* subs_delta(Ctx, Adds, Dels) -> {ok, Epoch} | {error, _}: the subscriber
   changes since the last call ({FilterId, Sub} pairs; a $share group as
   GroupId bor 16#80000000) in one epoch of the fan-out's table —
   emqx_broker:subscribe/3, unsubscribe/1 and subscriber_down/1
   (emqx_broker.erl:144-197, 331-345).  Adds and Dels are NET effects: a pair
   in both lists is refused ({error, einval}, nothing applied); an
   unsubscribe-then-resubscribe since the last call is the add alone. */
static ERL_NIF_TERM nif_subs_delta(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  egm_sub_pair *add = NULL, *del = NULL;
  unsigned na = 0, nd = 0;
  if (argc != 3 || !get_ctx(env, argv[0], &r)) return enif_make_badarg(env);
  if (!get_pairs(env, argv[1], &add, &na)) return enif_make_badarg(env);
  if (!get_pairs(env, argv[2], &del, &nd)) {
    free(add);
    return enif_make_badarg(env);
  }
  uint64_t epoch = 0;
  int rc = egm_subs_apply_delta(r->ctx, add, na, del, nd);
  if (!rc) rc = egm_subs_commit(r->ctx, &epoch);
  free(add);
  free(del);
  return rc ? error_tuple(env, r->ctx, rc) : enif_make_tuple2(env, ATOM_OK, enif_make_uint64(env, epoch));
}

/* publish_batch(Ctx, [Topic]) -> {ok, [{[FilterId], [{FilterId, Sub}]}]} | {error, _} */
static ERL_NIF_TERM nif_publish_batch(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  uint8_t* blob;
  uint32_t *off, n;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !pack_list(env, argv[1], &blob, &off, &n))
    return enif_make_badarg(env);
  egm_result* res = NULL;
  egm_delivery* dl = NULL;
  int rc = egm_match_batch(r->ctx, blob, off, n, EGM_MODE_ROUTES, &res);
  free(blob);
  free(off);
  if (!rc) rc = egm_fanout_batch(r->ctx, res, &dl);
  if (rc) {
    if (res) egm_result_free(res);
    if (dl) egm_result_free(dl);
    return error_tuple(env, r->ctx, rc);
  }
  ERL_NIF_TERM out = enif_make_list(env, 0);
  for (uint32_t i = n; i-- > 0;) {
    ERL_NIF_TERM ids = enif_make_list(env, 0), dv = enif_make_list(env, 0);
    for (uint64_t k = res->row_ptr[i + 1]; k-- > res->row_ptr[i];)
      ids = enif_make_list_cell(env, enif_make_uint(env, res->ids[k]), ids);
    for (uint64_t k = dl->row_ptr[i + 1]; k-- > dl->row_ptr[i];)
      dv = enif_make_list_cell(
          env, enif_make_tuple2(env, enif_make_uint(env, dl->fid[k]), enif_make_uint(env, dl->sub[k])), dv);
    out = enif_make_list_cell(env, enif_make_tuple2(env, ids, dv), out);
  }
  egm_result_free(res);
  egm_result_free(dl);
  return enif_make_tuple2(env, ATOM_OK, out);
}

/* [uint32] -> malloc'd array (*n values); 0 on a bad term */
static int get_u32_list(ErlNifEnv* env, ERL_NIF_TERM list, uint32_t** out, unsigned* n) {
  ERL_NIF_TERM head, tail = list;
  if (!enif_get_list_length(env, list, n)) return 0;
  *out = (uint32_t*)malloc(sizeof(uint32_t) * (*n ? *n : 1));
  if (!*out) return 0;
  for (unsigned i = 0; i < *n; ++i) {
    unsigned v;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_uint(env, head, &v)) {
      free(*out);
      *out = NULL;
      return 0;
    }
    (*out)[i] = v;
  }
  return 1;
}

/* subs_set_dead(Ctx, [Sub], Dead :: 0 | 1) -> ok | {error, _}: the subscribers
   whose process is gone (1) or back (0); a Sub with bit 31 set is refused. */
static ERL_NIF_TERM nif_subs_set_dead(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  uint32_t* subs = NULL;
  unsigned n = 0;
  int dead;
  if (argc != 3 || !get_ctx(env, argv[0], &r) || !enif_get_int(env, argv[2], &dead) || (dead != 0 && dead != 1) ||
      !get_u32_list(env, argv[1], &subs, &n))
    return enif_make_badarg(env);
  int rc = egm_subs_set_dead(r->ctx, subs, n, dead);
  free(subs);
  return rc ? error_tuple(env, r->ctx, rc) : ATOM_OK;
}

/* [{FilterId, GroupId, Member}] -> egm_share_member[] (malloc'd; *n rows); 0 on a bad term */
static int get_triples(ErlNifEnv* env, ERL_NIF_TERM list, egm_share_member** out, unsigned* n) {
  ERL_NIF_TERM head, tail = list;
  if (!enif_get_list_length(env, list, n)) return 0;
  *out = (egm_share_member*)malloc(sizeof(egm_share_member) * (*n ? *n : 1));
  if (!*out) return 0;
  for (unsigned i = 0; i < *n; ++i) {
    const ERL_NIF_TERM* el;
    int arity;
    unsigned f, g, m;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_tuple(env, head, &arity, &el) || arity != 3 ||
        !enif_get_uint(env, el[0], &f) || !enif_get_uint(env, el[1], &g) || !enif_get_uint(env, el[2], &m)) {
      free(*out);
      *out = NULL;
      return 0;
    }
    (*out)[i].fid = f;
    (*out)[i].group = g;
    (*out)[i].member = m;
  }
  return 1;
}

/* share_build(Ctx, [{FilterId, GroupId, Member}]) -> ok | {error, _}: the
   $share groups' members, a group's in the order given. */
static ERL_NIF_TERM nif_share_build(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  egm_share_member* rows = NULL;
  unsigned n = 0;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !get_triples(env, argv[1], &rows, &n)) return enif_make_badarg(env);
  int rc = egm_share_build(r->ctx, rows, n);
  free(rows);
  return rc ? error_tuple(env, r->ctx, rc) : ATOM_OK;
}

/* share_delta(Ctx, Adds, Dels) -> {ok, Epoch} | {error, _}: the member
   changes since the last call in one epoch (NET effects, as subs_delta/3: a
   triple in both lists is refused and nothing is applied). */
static ERL_NIF_TERM nif_share_delta(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  egm_share_member *add = NULL, *del = NULL;
  unsigned na = 0, nd = 0;
  if (argc != 3 || !get_ctx(env, argv[0], &r)) return enif_make_badarg(env);
  if (!get_triples(env, argv[1], &add, &na)) return enif_make_badarg(env);
  if (!get_triples(env, argv[2], &del, &nd)) {
    free(add);
    return enif_make_badarg(env);
  }
  uint64_t epoch = 0;
  int rc = egm_share_apply_delta(r->ctx, add, na, del, nd);
  if (!rc) rc = egm_share_commit(r->ctx, &epoch);
  free(add);
  free(del);
  return rc ? error_tuple(env, r->ctx, rc) : enif_make_tuple2(env, ATOM_OK, enif_make_uint64(env, epoch));
}

/* dispatch_batch(Ctx, [Topic], Keys, Strategy, Seed)
     -> {ok, [{{[FilterId], [{FilterId, Sub}]}, [{Live, SharedOk}]}]} | {error, _}
   publish_batch/2's rows with the dead subscribers and the groups without a
   live member already removed and each group entry replaced by its picked
   member, and per matched filter (in [FilterId]'s order) its live subscribers
   and its groups that got a member.  Strategy is EGM_PICK_* (0 random,
   1 round_robin, 2 sticky, 3 hash, 4 hash_clientid, 5 hash_topic); Keys is one
   hash per topic (of the client id or the source topic) for the hash
   strategies, [] otherwise. */
static ERL_NIF_TERM nif_dispatch_batch(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  uint8_t* blob;
  uint32_t *off, n, *keys = NULL;
  unsigned nk = 0;
  int strategy;
  ErlNifUInt64 seed;
  if (argc != 5 || !get_ctx(env, argv[0], &r) || !enif_get_int(env, argv[3], &strategy) ||
      strategy < EGM_PICK_RANDOM || strategy > EGM_PICK_HASH_TOPIC || !enif_get_uint64(env, argv[4], &seed) ||
      !get_u32_list(env, argv[2], &keys, &nk))
    return enif_make_badarg(env);
  if (!pack_list(env, argv[1], &blob, &off, &n) || (nk != 0 && nk != n) ||
      (strategy >= EGM_PICK_HASH && nk != n)) {
    free(keys);
    return enif_make_badarg(env);
  }
  egm_result* res = NULL;
  egm_dispatch* dl = NULL;
  int rc = egm_match_batch(r->ctx, blob, off, n, EGM_MODE_ROUTES, &res);
  free(blob);
  free(off);
  if (!rc) rc = egm_dispatch_batch(r->ctx, res, nk ? keys : NULL, strategy, seed, &dl);
  free(keys);
  if (rc) {
    if (res) egm_result_free(res);
    if (dl) egm_result_free(dl);
    return error_tuple(env, r->ctx, rc);
  }
  ERL_NIF_TERM out = enif_make_list(env, 0);
  for (uint32_t i = n; i-- > 0;) {
    ERL_NIF_TERM ids = enif_make_list(env, 0), dv = enif_make_list(env, 0), cn = enif_make_list(env, 0);
    for (uint64_t k = res->row_ptr[i + 1]; k-- > res->row_ptr[i];) {
      ids = enif_make_list_cell(env, enif_make_uint(env, res->ids[k]), ids);
      cn = enif_make_list_cell(
          env, enif_make_tuple2(env, enif_make_uint(env, dl->entry_live[k]), enif_make_uint(env, dl->entry_shared[k])),
          cn);
      for (uint64_t j = dl->entry_pos[k + 1]; j-- > dl->entry_pos[k];)
        if (dl->sub[j] != EGM_SUB_NONE)
          dv = enif_make_list_cell(
              env, enif_make_tuple2(env, enif_make_uint(env, res->ids[k]), enif_make_uint(env, dl->sub[j])), dv);
    }
    out = enif_make_list_cell(env, enif_make_tuple2(env, enif_make_tuple2(env, ids, dv), cn), out);
  }
  egm_result_free(res);
  egm_result_free(dl);
  return enif_make_tuple2(env, ATOM_OK, out);
}

/* ---- cluster routes ---- */
_Static_assert(sizeof(egm_route_pair) == sizeof(egm_sub_pair), "get_pairs fills either pair");
/* erl_nif.h's own declaration, repeated (a compatible redeclaration): forward/2 is the one entry that builds a binary */
extern unsigned char* enif_make_new_binary(ErlNifEnv* env, size_t size, ERL_NIF_TERM* termp);

/* routes_build(Ctx, [Mask], SelfNode) -> ok | {error, _}: the route-node table,
   one 64-bit node mask per filter id (bit N: a route {Filter, node N}). */
static ERL_NIF_TERM nif_routes_build(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  unsigned n, self;
  if (argc != 3 || !get_ctx(env, argv[0], &r) || !enif_get_list_length(env, argv[1], &n) ||
      !enif_get_uint(env, argv[2], &self))
    return enif_make_badarg(env);
  uint64_t* masks = (uint64_t*)malloc(sizeof(uint64_t) * (n ? n : 1));
  if (!masks) return enif_make_badarg(env);
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; i < n; ++i) {
    ErlNifUInt64 m;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_uint64(env, head, &m)) {
      free(masks);
      return enif_make_badarg(env);
    }
    masks[i] = m;
  }
  int rc = egm_routes_build(r->ctx, masks, n, self);
  free(masks);
  return rc ? error_tuple(env, r->ctx, rc) : ATOM_OK;
}

/* routes_delta(Ctx, Adds, Dels) -> {ok, Epoch} | {error, _}: the {FilterId,
   NodeId} routes added and deleted since the last call (emqx_router:
   do_add_route/2, do_delete_route/2) in one epoch; NET effects, as
   subs_delta/3. */
static ERL_NIF_TERM nif_routes_delta(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  egm_sub_pair *add = NULL, *del = NULL;
  unsigned na = 0, nd = 0;
  if (argc != 3 || !get_ctx(env, argv[0], &r)) return enif_make_badarg(env);
  if (!get_pairs(env, argv[1], &add, &na)) return enif_make_badarg(env);
  if (!get_pairs(env, argv[2], &del, &nd)) {
    free(add);
    return enif_make_badarg(env);
  }
  uint64_t epoch = 0;
  int rc = egm_routes_apply_delta(r->ctx, (const egm_route_pair*)add, na, (const egm_route_pair*)del, nd);
  if (!rc) rc = egm_routes_commit(r->ctx, &epoch);
  free(add);
  free(del);
  return rc ? error_tuple(env, r->ctx, rc) : enif_make_tuple2(env, ATOM_OK, enif_make_uint64(env, epoch));
}

/* routes_drop_node(Ctx, NodeId) -> {ok, [FilterId]} | {error, _}:
   emqx_router_helper:cleanup_routes/1 for a node's atom dests; the filters
   left without any route, ascending (the caller deletes them). */
static ERL_NIF_TERM nif_routes_drop_node(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  unsigned node;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !enif_get_uint(env, argv[1], &node)) return enif_make_badarg(env);
  uint32_t* ids = NULL;
  uint64_t n = 0;
  int rc = egm_routes_drop_node(r->ctx, node, &ids, &n);
  if (rc) return error_tuple(env, r->ctx, rc);
  ERL_NIF_TERM out = enif_make_list(env, 0);
  for (uint64_t k = n; k-- > 0;) out = enif_make_list_cell(env, enif_make_uint(env, ids[k]), out);
  if (ids) egm_result_free(ids);
  return enif_make_tuple2(env, ATOM_OK, out);
}

/* forward(Ctx, [Topic]) -> {ok, [{NodeId, Pairs :: binary()}]} | {error, _}:
   per remote node with any forward, its <<TopicIndex:32/native,
   FilterId:32/native>> pairs in (topic, match order) — the payload of one
   batched rpc to that node (emqx_broker:forward/4). */
static ERL_NIF_TERM nif_forward(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_res_t* r;
  uint8_t* blob;
  uint32_t *off, n;
  if (argc != 2 || !get_ctx(env, argv[0], &r) || !pack_list(env, argv[1], &blob, &off, &n))
    return enif_make_badarg(env);
  egm_result* res = NULL;
  egm_forward* fw = NULL;
  int rc = egm_match_batch(r->ctx, blob, off, n, EGM_MODE_ROUTES, &res);
  free(blob);
  free(off);
  if (!rc) rc = egm_forward_batch(r->ctx, res, &fw);
  if (res) egm_result_free(res);
  if (rc) {
    if (fw) egm_result_free(fw);
    return error_tuple(env, r->ctx, rc);
  }
  ERL_NIF_TERM out = enif_make_list(env, 0);
  for (uint32_t k = fw->n_nodes; k-- > 0;) {
    const uint64_t lo = fw->node_row[k], hi = fw->node_row[k + 1];
    if (hi == lo) continue;
    ERL_NIF_TERM bin;
    uint32_t* p = (uint32_t*)enif_make_new_binary(env, (size_t)(hi - lo) * 8, &bin);
    if (!p) {
      egm_result_free(fw);
      return enif_make_badarg(env);
    }
    for (uint64_t j = lo; j < hi; ++j) {
      p[2 * (j - lo)] = fw->topic[j];
      p[2 * (j - lo) + 1] = fw->fid[j];
    }
    out = enif_make_list_cell(env, enif_make_tuple2(env, enif_make_uint(env, k), bin), out);
  }
  egm_result_free(fw);
  return enif_make_tuple2(env, ATOM_OK, out);
}

/* ---- retained store ---- */
static ERL_NIF_TERM rs_error(ErlNifEnv* env, egm_rstore* rs, int rc) {
  const char* msg = rs ? egm_rstore_last_error(rs) : "egm error";
  return enif_make_tuple2(env, ATOM_ERROR,
                          enif_make_tuple2(env, enif_make_int(env, rc), enif_make_string(env, msg, ERL_NIF_LATIN1)));
}

static int get_rs(ErlNifEnv* env, ERL_NIF_TERM t, egm_rs_t** r) {
  return enif_get_resource(env, t, EGM_RSTORE, (void**)r) && (*r)->rs;
}

/* [MsgId] from ids[n] */
static ERL_NIF_TERM ids_term(ErlNifEnv* env, const uint32_t* ids, uint64_t n) {
  ERL_NIF_TERM list = enif_make_list(env, 0);
  for (uint64_t k = n; k-- > 0;) list = enif_make_list_cell(env, enif_make_uint(env, ids[k]), list);
  return list;
}

/* rs_open(Device :: non_neg_integer()) -> {ok, Store} | {error, _} */
static ERL_NIF_TERM nif_rs_open(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  int dev;
  if (argc != 1 || !enif_get_int(env, argv[0], &dev) || dev < 0) return enif_make_badarg(env);
  egm_rstore* rs = NULL;
  int rc = egm_rstore_open(dev, &rs);
  if (rc) return rs_error(env, NULL, rc);
  egm_rs_t* r = (egm_rs_t*)enif_alloc_resource(EGM_RSTORE, sizeof(egm_rs_t));
  r->rs = rs;
  ERL_NIF_TERM term = enif_make_resource(env, r);
  enif_release_resource(r);
  return enif_make_tuple2(env, ATOM_OK, term);
}

/* rs_put(Store, Topic :: binary(), MsgId, ExpiryMs) -> ok | {error, full} | {error, _}
   (0 =< MsgId < 16#FFFFFFFF; ExpiryMs 0 = never) */
static ERL_NIF_TERM nif_rs_put(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  ErlNifBinary topic;
  unsigned id;
  ErlNifUInt64 expiry;
  if (argc != 4 || !get_rs(env, argv[0], &r) || !enif_inspect_binary(env, argv[1], &topic) ||
      topic.size > 0xFFFFFFFFu || !enif_get_uint(env, argv[2], &id) || !enif_get_uint64(env, argv[3], &expiry))
    return enif_make_badarg(env);
  int rc = egm_rstore_put(r->rs, topic.data, (uint32_t)topic.size, id, expiry);
  if (rc == EGM_E_FULL) return enif_make_tuple2(env, ATOM_ERROR, ATOM_FULL);
  return rc ? rs_error(env, r->rs, rc) : ATOM_OK;
}

/* rs_delete(Store, Topic :: binary()) -> ok | {error, _}: the topic itself, no wildcard */
static ERL_NIF_TERM nif_rs_delete(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  ErlNifBinary topic;
  if (argc != 2 || !get_rs(env, argv[0], &r) || !enif_inspect_binary(env, argv[1], &topic) ||
      topic.size > 0xFFFFFFFFu)
    return enif_make_badarg(env);
  int rc = egm_rstore_delete(r->rs, topic.data, (uint32_t)topic.size);
  return rc ? rs_error(env, r->rs, rc) : ATOM_OK;
}

/* rs_delete_matching(Store, [Filter :: binary()]) -> {ok, [MsgId]} | {error, _} */
static ERL_NIF_TERM nif_rs_delete_matching(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  uint8_t* blob;
  uint32_t *off, n;
  if (argc != 2 || !get_rs(env, argv[0], &r) || !pack_list(env, argv[1], &blob, &off, &n))
    return enif_make_badarg(env);
  uint32_t* ids = NULL;
  uint64_t n_ids = 0;
  int rc = egm_rstore_delete_matching(r->rs, blob, off, n, &ids, &n_ids);
  free(blob);
  free(off);
  if (rc) return rs_error(env, r->rs, rc);
  ERL_NIF_TERM list = ids_term(env, ids, n_ids);
  egm_result_free(ids);
  return enif_make_tuple2(env, ATOM_OK, list);
}

/* rs_set_max_retained(Store, Max) -> ok | {error, _}: max_retained_messages; 0 = no limit */
static ERL_NIF_TERM nif_rs_set_max_retained(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  ErlNifUInt64 max;
  if (argc != 2 || !get_rs(env, argv[0], &r) || !enif_get_uint64(env, argv[1], &max)) return enif_make_badarg(env);
  int rc = egm_rstore_set_max_retained(r->rs, max);
  return rc ? rs_error(env, r->rs, rc) : ATOM_OK;
}

/* rs_clean(Store) -> ok | {error, _} */
static ERL_NIF_TERM nif_rs_clean(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  if (argc != 1 || !get_rs(env, argv[0], &r)) return enif_make_badarg(env);
  int rc = egm_rstore_clean(r->rs);
  return rc ? rs_error(env, r->rs, rc) : ATOM_OK;
}

/* rs_size(Store) -> {ok, non_neg_integer()} | {error, _} */
static ERL_NIF_TERM nif_rs_size(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  if (argc != 1 || !get_rs(env, argv[0], &r)) return enif_make_badarg(env);
  uint64_t n = 0;
  int rc = egm_rstore_size(r->rs, &n);
  return rc ? rs_error(env, r->rs, rc) : enif_make_tuple2(env, ATOM_OK, enif_make_uint64(env, n));
}

/* rs_commit(Store) -> ok | {error, _}: apply the puts and deletes now (the next lookup would) */
static ERL_NIF_TERM nif_rs_commit(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  if (argc != 1 || !get_rs(env, argv[0], &r)) return enif_make_badarg(env);
  int rc = egm_rstore_commit(r->rs);
  return rc ? rs_error(env, r->rs, rc) : ATOM_OK;
}

/* rs_clear_expired(Store, NowMs) -> {ok, [MsgId]} | {error, _} */
static ERL_NIF_TERM nif_rs_clear_expired(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  ErlNifUInt64 now;
  if (argc != 2 || !get_rs(env, argv[0], &r) || !enif_get_uint64(env, argv[1], &now)) return enif_make_badarg(env);
  uint32_t* ids = NULL;
  uint64_t n_ids = 0;
  int rc = egm_rstore_clear_expired(r->rs, now, &ids, &n_ids);
  if (rc) return rs_error(env, r->rs, rc);
  ERL_NIF_TERM list = ids_term(env, ids, n_ids);
  egm_result_free(ids);
  return enif_make_tuple2(env, ATOM_OK, list);
}

/* rs_match(Store, [Filter :: binary()], NowMs, Mode :: 0 | 1) -> {ok, [[MsgId]]} | {error, _} */
static ERL_NIF_TERM nif_rs_match(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  egm_rs_t* r;
  ErlNifUInt64 now;
  int mode;
  uint8_t* blob;
  uint32_t *off, n;
  if (argc != 4 || !get_rs(env, argv[0], &r) || !enif_get_uint64(env, argv[2], &now) ||
      !enif_get_int(env, argv[3], &mode) || (mode != EGM_RMODE_MATCH && mode != EGM_RMODE_DISPATCH) ||
      !pack_list(env, argv[1], &blob, &off, &n))
    return enif_make_badarg(env);
  egm_result* res = NULL;
  int rc = egm_rstore_match(r->rs, blob, off, n, now, mode, &res);
  free(blob);
  free(off);
  if (rc) {
    if (res) egm_result_free(res);
    return rs_error(env, r->rs, rc);
  }
  ERL_NIF_TERM rows = rows_term(env, res);
  egm_result_free(res);
  return enif_make_tuple2(env, ATOM_OK, rows);
}

static ErlNifFunc nif_funcs[] = {
    {"open", 1, nif_open, 0},
    {"build", 2, nif_build, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"apply_delta", 3, nif_apply_delta, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"match_batch", 3, nif_match_batch, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"submit", 3, nif_submit, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"wait", 2, nif_wait, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"cancel", 2, nif_cancel, 0},
    {"subs_build", 2, nif_subs_build, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"subs_delta", 3, nif_subs_delta, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"publish_batch", 2, nif_publish_batch, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"subs_set_dead", 3, nif_subs_set_dead, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"share_build", 2, nif_share_build, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"share_delta", 3, nif_share_delta, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"dispatch_batch", 5, nif_dispatch_batch, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"routes_build", 3, nif_routes_build, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"routes_delta", 3, nif_routes_delta, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"routes_drop_node", 2, nif_routes_drop_node, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"forward", 2, nif_forward, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    /* the retained store: every call takes the store's lock, which a match or a
       delete holds across its device work, so none runs on a normal scheduler */
    {"rs_open", 1, nif_rs_open, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_put", 4, nif_rs_put, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_delete", 2, nif_rs_delete, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_delete_matching", 2, nif_rs_delete_matching, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_set_max_retained", 2, nif_rs_set_max_retained, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_clean", 1, nif_rs_clean, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_size", 1, nif_rs_size, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_commit", 1, nif_rs_commit, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_clear_expired", 2, nif_rs_clear_expired, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"rs_match", 4, nif_rs_match, ERL_NIF_DIRTY_JOB_CPU_BOUND},
};

ERL_NIF_INIT(emqx_gpu_match, nif_funcs, load, NULL, NULL, NULL)
