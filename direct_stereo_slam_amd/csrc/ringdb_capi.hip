// ringdb_capi.hip -- C ABI of the ring-key database: replaces the flann::Index created at
// LoopHandler.cpp:35-39 and the function-static delay queue of search_ringkey
// (search_place.h:41-56).  Host code keeps the queue and the ordinal bookkeeping; the scan runs
// in ringkey_kernels.hip.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "call_arena.hpp"
#include <string>

#include "ringdb_internal.hpp"

using namespace dsm;

static int rdb_reserve(dsm_ringdb *db, int64_t need_local) {
  if (need_local <= db->cap) return DSM_OK;
  int64_t ncap = db->cap > 0 ? db->cap : 1024;
  while (ncap < need_local) ncap *= 2;
  // the scans with four keys per thread (DSM_RINGKEY_FORM_FEWQ4_*, MANY4) load 16 bytes per plane at slots that are multiples of four
  if (ncap & 3) return invalid("ring-key index: the capacity must be a multiple of four");
  float *nk = nullptr;
  DSM_HIP(hipMalloc(&nk, sizeof(float) * (size_t)ncap * db->dim));
  hipError_t e = hipSuccess;
  if (db->d_keysT && db->n_local > 0)
    for (int j = 0; j < db->dim && e == hipSuccess; j++)
      e = hipMemcpyAsync(nk + (size_t)j * ncap, db->d_keysT + (size_t)j * db->cap, sizeof(float) * db->n_local,
                         hipMemcpyDeviceToDevice, db->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(db->ctx->stream);
  if (e != hipSuccess) { // the old planes stay valid; give the new allocation back
    hipFree(nk);
    DSM_HIP(e);
  }
  if (db->d_keysT) DSM_HIP(hipFree(db->d_keysT));
  db->d_keysT = nk;
  db->cap = ncap;
  return DSM_OK;
}

static int rdb_stage(dsm_ringdb *db, size_t floats) {
  if (floats <= db->q_floats) return DSM_OK;
  if (db->d_q) DSM_HIP(hipFree(db->d_q));
  db->d_q = nullptr;
  DSM_HIP(hipMalloc(&db->d_q, floats * sizeof(float)));
  db->q_floats = floats;
  return DSM_OK;
}

// append n keys with global ordinals size_global .. size_global+n-1; keep those of this shard
static int rdb_append(dsm_ringdb *db, const float *keys, int64_t n) {
  // candidates are packed (float_bits(d^2) << 32) | global index, and dsm_ringdb_query_then_enqueue hands indices out
  // as int (search_place.h:36): the global index must stay below 2^31
  if (db->size_global + n > (int64_t)INT32_MAX) return invalid("ring-key index full: global ordinals are limited to 2^31 - 1");
  std::vector<float> mine;
  mine.reserve((size_t)(n / db->shard_count + 1) * db->dim);
  for (int64_t i = 0; i < n; i++) {
    const int64_t g = db->size_global + i;
    if (g % db->shard_count == db->shard_rank) mine.insert(mine.end(), keys + i * db->dim, keys + (i + 1) * db->dim);
  }
  const int64_t m = (int64_t)mine.size() / db->dim;
  if (m > 0) {
    int rc = rdb_reserve(db, db->n_local + m);
    if (rc) return rc;
    // upload in bounded pieces through the staging buffer
    const int64_t piece = 1 << 16;
    rc = rdb_stage(db, (size_t)(m < piece ? m : piece) * db->dim);
    if (rc) return rc;
    for (int64_t o = 0; o < m; o += piece) {
      const int64_t c = m - o < piece ? m - o : piece;
      DSM_HIP(hipMemcpyAsync(db->d_q, mine.data() + o * db->dim, sizeof(float) * c * db->dim, hipMemcpyHostToDevice,
                             db->ctx->stream));
      launch_ringkey_insert(db->ctx->stream, db->d_keysT, db->cap, db->n_local + o, db->dim, db->d_q, (int)c);
      DSM_HIP(hipStreamSynchronize(db->ctx->stream));
    }
    db->n_local += m;
  }
  db->size_global += n;
  return DSM_OK;
}

static int rdb_knn_dev(dsm_ringdb *db, const float *d_queries, int nq, unsigned long long *d_out) {
  const int n_slices = ringkey_num_slices(db->n_local, nq, db->dim);
  const size_t need = (size_t)n_slices * nq * db->k;
  if (need > db->scratch_words) {
    if (db->d_scratch) DSM_HIP(hipFree(db->d_scratch));
    db->d_scratch = nullptr;
    DSM_HIP(hipMalloc(&db->d_scratch, need * sizeof(unsigned long long)));
    db->scratch_words = need;
  }
  launch_ringkey_knn(db->ctx->stream, db->d_keysT, db->cap, db->n_local, db->dim, db->k, db->thres, db->shard_rank,
                     db->shard_count, d_queries, nq, db->d_scratch, n_slices, d_out);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

namespace dsm {
int ringdb_knn_device(dsm_ringdb *db, const float *d_queries, int nq, unsigned long long *d_out) { return rdb_knn_dev(db, d_queries, nq, d_out); }

int ringdb_finish_query(const dsm_ringdb *db, const float *key, const unsigned long long *dev, const float *matured, long long n_matured,
                        long long base, int *cand_out) {
  const int k = db->k;
  unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  int nb = 0;
  if (base + n_matured > k) { // `ringkeys->size() > FLANN_NN`, search_place.h:29, with the index as this query sees it
    if (dev)
      for (int i = 0; i < k; i++)
        if (dev[i] != (unsigned long long)DSM_RINGDB_NO_CANDIDATE) best[nb++] = dev[i];
    for (long long m = 0; m < n_matured; m++) { // flann::L2, as the kernels: groups of four, then the tail
      const float *kp = matured + m * db->dim;
      float result = 0.f;
      int d = 0;
      for (; d + 3 < db->dim; d += 4) {
        const float d0 = key[d] - kp[d], d1 = key[d + 1] - kp[d + 1], d2 = key[d + 2] - kp[d + 2], d3 = key[d + 3] - kp[d + 3];
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      }
      for (; d < db->dim; d++) {
        const float d0 = key[d] - kp[d];
        result += d0 * d0;
      }
      if (!(result < db->thres)) continue;
      unsigned bits;
      memcpy(&bits, &result, 4);
      const unsigned long long c = ((unsigned long long)bits << 32) | (unsigned long long)(base + m);
      // insert into the ascending list of at most k
      int pos = nb < k ? nb : k;
      for (int i = 0; i < nb && i < k; i++)
        if (c < best[i]) {
          pos = i;
          break;
        }
      if (pos < k) {
        for (int i = (nb < k ? nb : k - 1); i > pos; i--) best[i] = best[i - 1];
        best[pos] = c;
        if (nb < k) nb++;
      }
    }
  }
  int nc = 0;
  for (int i = 0; i < nb && i < k; i++) {
    const int idx = (int)(best[i] & 0xFFFFFFFFull);
    if (idx > 0) cand_out[nc++] = idx - 1; // :34-38
  }
  return nc;
}

void ringdb_queue_push(dsm_ringdb *db, const float *key, std::vector<float> *matured) {
  float *slot = db->queue.data() + (size_t)(db->queue_idx % db->margin) * db->dim;
  if (db->queue_idx >= db->margin && matured) matured->insert(matured->end(), slot, slot + db->dim);
  memcpy(slot, key, sizeof(float) * db->dim);
  db->queue_idx++;
}

int ringdb_many_prepare(dsm_context *ctx, int n, dsm_ringdb *const *dbs, int dim, const char *who, RingManyPlan &P) {
  const std::string w(who);
  if (n < 1 || !dbs) return invalid((w + ": bad argument").c_str());
  for (int j = 0; j < n; j++)
    if (!dbs[j]) return invalid((w + ": null index").c_str());
  if (!ctx) ctx = dbs[0]->ctx;
  if (dim < 0) dim = dbs[0]->dim;
  const int k = dbs[0]->k;
  for (int j = 0; j < n; j++) {
    const dsm_ringdb *db = dbs[j];
    if (db->ctx != ctx) return invalid((w + ": every index must belong to the call's context").c_str());
    if (db->shard_count != 1) return invalid((w + ": unsharded indexes only (a sharded one searches through dsm_ringdb_query_then_enqueue)").c_str());
    if (db->dim != dim) return invalid((w + ": every index must have the same key dimension (num_r in the loop form)").c_str());
    if (db->k != k) return invalid((w + ": every index must have the same k").c_str());
  }
  P.n = n, P.dim = dim, P.k = k;
  // the distinct indexes, in order of first appearance (many_slot is -1 between calls)
  P.uniq.clear();
  P.slot_of.resize(n);
  for (int j = 0; j < n; j++) {
    if (dbs[j]->many_slot < 0) {
      dbs[j]->many_slot = (int)P.uniq.size();
      P.uniq.push_back(dbs[j]);
    }
    P.slot_of[j] = dbs[j]->many_slot;
  }
  for (dsm_ringdb *db : P.uniq) db->many_slot = -1;
  const int nu = (int)P.uniq.size();
  std::vector<int> jobs(nu, 0);
  P.mat_count.assign(nu, 0);
  for (int j = 0; j < n; j++) {
    const int u = P.slot_of[j];
    if (P.uniq[u]->queue_idx + jobs[u] >= P.uniq[u]->margin) P.mat_count[u]++; // this enqueue moves a key out of the delay queue
    jobs[u]++;
  }
  for (int u = 0; u < nu; u++) {
    const dsm_ringdb *db = P.uniq[u];
    if (jobs[u] > db->margin) return invalid((w + ": at most `margin` jobs per index and call").c_str());
    if (db->size_global + P.mat_count[u] > (int64_t)INT32_MAX) return invalid((w + ": ring-key index full: global ordinals are limited to 2^31 - 1").c_str());
  }
  // every index that the matured keys outgrow grows now, before anything is enqueued (a failure leaves every index as it was)
  DSM_HIP(hipSetDevice(ctx->device));
  for (int u = 0; u < nu; u++) {
    const int rc = rdb_reserve(P.uniq[u], P.uniq[u]->n_local + P.mat_count[u]);
    if (rc) return rc;
  }
  P.mat_off.assign(nu, 0);
  P.base.assign(nu, 0);
  P.n_matured = 0;
  for (int u = 0; u < nu; u++) {
    P.mat_off[u] = P.n_matured;
    P.n_matured += P.mat_count[u];
    P.base[u] = P.uniq[u]->size_global;
  }
  P.matured.resize((size_t)P.n_matured * dim);
  P.ins.resize(P.n_matured);
  P.scan.resize(n);
  std::fill(jobs.begin(), jobs.end(), 0);
  std::vector<int> filled(nu, 0);
  P.n_slices = 1;
  P.four = true;
  for (int j = 0; j < n; j++) {
    const int u = P.slot_of[j];
    dsm_ringdb *db = P.uniq[u];
    const int64_t qi = db->queue_idx + jobs[u]++;
    if (qi >= db->margin) { // the slot this enqueue overwrites holds the key of its start-of-call state (each slot is overwritten once)
      const int row = P.mat_off[u] + filled[u];
      memcpy(P.matured.data() + (size_t)row * dim, db->queue.data() + (size_t)(qi % db->margin) * dim, sizeof(float) * dim);
      P.ins[row] = RingKeyInsertDesc{db->d_keysT, (long long)db->cap, (long long)(db->n_local + filled[u])};
      filled[u]++;
    }
    RingKeyScanDesc &D = P.scan[j];
    D.keysT = db->d_keysT, D.cap = db->cap, D.n_local = db->n_local, D.thres = db->thres, D.n_slices = ringkey_many_slices(db->n_local);
    if (D.n_slices > P.n_slices) P.n_slices = D.n_slices;
    if (db->cap % 4) P.four = false; // rdb_reserve keeps capacities at 1024 * 2^m: checked, not assumed
  }
  CallArena::Region staged;
  staged.take(sizeof(RingKeyScanDesc) * (size_t)n);
  P.off_ins = staged.take(sizeof(RingKeyInsertDesc) * (size_t)P.n_matured);
  P.off_keys = staged.used;
  P.staged_bytes = P.off_keys + sizeof(float) * P.matured.size();
  return DSM_OK;
}

void ringdb_many_stage(const RingManyPlan &P, unsigned char *h_staged) {
  memcpy(h_staged, P.scan.data(), sizeof(RingKeyScanDesc) * P.scan.size());
  if (P.n_matured) {
    memcpy(h_staged + P.off_ins, P.ins.data(), sizeof(RingKeyInsertDesc) * P.ins.size());
    memcpy(h_staged + P.off_keys, P.matured.data(), sizeof(float) * P.matured.size());
  }
}

size_t ringdb_many_scratch_words(const RingManyPlan &P) { return (size_t)P.n_slices * P.n * P.k; }

int ringdb_many_launch(hipStream_t s, const RingManyPlan &P, const unsigned char *d_staged, const float *d_queries,
                       unsigned long long *d_scratch, unsigned long long *d_packed) {
  launch_ringkey_knn_many(s, (const RingKeyScanDesc *)d_staged, P.dim, P.k, P.four, d_queries, P.n, P.n_slices, d_scratch, d_packed);
  if (P.n_matured) // behind the scan on the same stream: the scan sees every index as it stood at the start of the call
    launch_ringkey_insert_many(s, (const RingKeyInsertDesc *)(d_staged + P.off_ins), P.dim, (const float *)(d_staged + P.off_keys), P.n_matured);
  DSM_HIP(hipGetLastError());
  return DSM_OK;
}

void ringdb_many_finish(const RingManyPlan &P, dsm_ringdb *const *dbs, const float *const *keys, const unsigned long long *h_packed,
                        int *cand_out, int *ncand_out) {
  std::vector<int> seen(P.uniq.size(), 0); // matured keys of each index so far
  for (int j = 0; j < P.n; j++) {
    const int u = P.slot_of[j];
    dsm_ringdb *db = dbs[j];
    ncand_out[j] = ringdb_finish_query(db, keys[j], h_packed + (size_t)j * P.k, P.matured.data() + (size_t)P.mat_off[u] * P.dim, seen[u],
                                       P.base[u], cand_out + (size_t)j * P.k);
    if (db->queue_idx >= db->margin) seen[u]++;
    ringdb_queue_push(db, keys[j], nullptr);
  }
  for (size_t u = 0; u < P.uniq.size(); u++) { // their planes were written by the insert launch
    P.uniq[u]->n_local += P.mat_count[u];
    P.uniq[u]->size_global += P.mat_count[u];
  }
}
} // namespace dsm
extern "C" {
int dsm_ringdb_destroy(dsm_ringdb *db);

int dsm_ringdb_create(dsm_context *ctx, int dim, int margin, int k, float thres, const float *dummy_key,
                      int64_t capacity, int shard_rank, int shard_count, dsm_ringdb **out) {
  if (!ctx || !out) return invalid("dsm_ringdb_create: null argument");
  if (dim < 1 || dim > 32) return invalid("dsm_ringdb_create: dim must be in [1,32]");
  if (k < 1 || k > 4) return invalid("dsm_ringdb_create: k must be in [1,4]");
  if (margin < 1) return invalid("dsm_ringdb_create: margin must be >= 1");
  if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return invalid("dsm_ringdb_create: bad shard");
  DSM_HIP(hipSetDevice(ctx->device));
  dsm_ringdb *db = new dsm_ringdb();
  db->ctx = ctx;
  db->dim = dim;
  db->margin = margin;
  db->k = k;
  db->thres = thres;
  db->shard_rank = shard_rank;
  db->shard_count = shard_count;
  db->queue.assign((size_t)margin * dim, 0.f);
  int rc = rdb_reserve(db, capacity > 16 ? capacity : 16);
  if (rc) {
    dsm_ringdb_destroy(db);
    return rc;
  }
  // index slot 0: the reference's dummy entry (LoopHandler.cpp:35-39, quirk Q8)
  std::vector<float> dummy(dim, 0.f);
  if (dummy_key) memcpy(dummy.data(), dummy_key, sizeof(float) * dim);
  rc = rdb_append(db, dummy.data(), 1);
  if (rc) {
    dsm_ringdb_destroy(db);
    return rc;
  }
  *out = db;
  return DSM_OK;
}

int dsm_ringdb_destroy(dsm_ringdb *db) {
  if (!db) return DSM_OK;
  hipSetDevice(db->ctx->device);
  hipStreamSynchronize(db->ctx->stream);
  hipFree(db->d_keysT);
  hipFree(db->d_q);
  hipFree(db->d_scratch);
  hipFree(db->d_out);
  hipFree(db->d_merge);
  hipFree(db->d_agree);
  dsm::ringdb_forget_comm(db);
  delete db;
  return DSM_OK;
}

int64_t dsm_ringdb_size(dsm_ringdb *db) { return db ? db->size_global : -1; }

int dsm_ringdb_add_points(dsm_ringdb *db, const float *keys, int64_t n_keys) {
  if (!db || !keys || n_keys < 0) return invalid("dsm_ringdb_add_points: bad argument");
  DSM_HIP(hipSetDevice(db->ctx->device));
  return rdb_append(db, keys, n_keys);
}

int dsm_ringdb_enqueue(dsm_ringdb *db, const float *key) { // search_place.h:41-56
  if (!db || !key) return invalid("dsm_ringdb_enqueue: bad argument");
  DSM_HIP(hipSetDevice(db->ctx->device));
  float *slot = db->queue.data() + (size_t)(db->queue_idx % db->margin) * db->dim;
  if (db->queue_idx >= db->margin) {
    int rc = rdb_append(db, slot, 1);
    if (rc) return rc;
  }
  memcpy(slot, key, sizeof(float) * db->dim);
  db->queue_idx++;
  return DSM_OK;
}

int dsm_ringdb_knn_packed_dev(dsm_ringdb *db, const void *d_queries, int nq, void *d_packed_out) {
  if (!db || !d_queries || !d_packed_out || nq < 1) return invalid("dsm_ringdb_knn_packed_dev: bad argument");
  DSM_HIP(hipSetDevice(db->ctx->device));
  return rdb_knn_dev(db, (const float *)d_queries, nq, (unsigned long long *)d_packed_out);
}

int dsm_ringdb_knn_packed(dsm_ringdb *db, const float *queries, int nq, void *d_packed_out) {
  if (!db || !queries || !d_packed_out || nq < 1) return invalid("dsm_ringdb_knn_packed: bad argument");
  DSM_HIP(hipSetDevice(db->ctx->device));
  int rc = rdb_stage(db, (size_t)nq * db->dim);
  if (rc) return rc;
  DSM_HIP(hipMemcpyAsync(db->d_q, queries, sizeof(float) * (size_t)nq * db->dim, hipMemcpyHostToDevice, db->ctx->stream));
  rc = rdb_knn_dev(db, db->d_q, nq, (unsigned long long *)d_packed_out);
  if (rc) return rc;
  DSM_HIP(hipStreamSynchronize(db->ctx->stream));
  return DSM_OK;
}

int dsm_ringdb_knn_packed_host(dsm_ringdb *db, const float *queries, int nq, int64_t *packed_out) {
  if (!db || !queries || !packed_out || nq < 1) return invalid("dsm_ringdb_knn_packed_host: bad argument");
  DSM_HIP(hipSetDevice(db->ctx->device));
  const size_t words = (size_t)nq * db->k;
  if (words > db->out_words) {
    if (db->d_out) DSM_HIP(hipFree(db->d_out));
    db->d_out = nullptr;
    DSM_HIP(hipMalloc(&db->d_out, words * sizeof(unsigned long long)));
    db->out_words = words;
  }
  int rc = dsm_ringdb_knn_packed(db, queries, nq, db->d_out);
  if (rc) return rc;
  DSM_HIP(hipMemcpy(packed_out, db->d_out, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return DSM_OK;
}

int dsm_ringdb_scan_plan(dsm_ringdb *db, int nq, int many, int *form_out, int *n_slices_out, long long *keys_per_slice_out) {
  if (!db || !form_out || !n_slices_out || !keys_per_slice_out || (!many && nq < 1)) return invalid("dsm_ringdb_scan_plan: bad argument");
  const int form = many ? ringkey_many_form(db->dim, db->cap % 4 == 0) : ringkey_scan_form(db->dim, nq);
  const int n_slices = many ? ringkey_many_slices(db->n_local) : ringkey_num_slices(db->n_local, nq, db->dim);
  *form_out = form;
  *n_slices_out = n_slices;
  *keys_per_slice_out = ringkey_slice_keys(db->n_local, n_slices, form);
  return DSM_OK;
}

int dsm_ringdb_query_then_enqueue(dsm_ringdb *db, const float *key, int *cand_out, int *ncand_out) {
  if (!db || !key || !cand_out || !ncand_out) return invalid("dsm_ringdb_query_then_enqueue: bad argument");
  // Sharded handle: a COLLECTIVE call -- every rank passes the same key, scans its shard, the candidates are merged
  // through the attached communicator (RCCL all-reduce(min)), and every rank returns the same candidate list and
  // enqueues the key (each shard keeps the ordinals that are its own).
  if (db->shard_count != 1 && !db->comm && !db->tr_allreduce) {
    set_error("dsm_ringdb_query_then_enqueue on a sharded DB needs a communicator (dsm_ringdb_attach_comm); "
              "without one use knn_packed + your own merge + enqueue");
    return DSM_ERR_STATE;
  }
  int nc = 0;
  const bool search = db->size_global > db->k; // `ringkeys->size() > FLANN_NN`, search_place.h:29
  int64_t packed[4] = {DSM_RINGDB_NO_CANDIDATE, DSM_RINGDB_NO_CANDIDATE, DSM_RINGDB_NO_CANDIDATE, DSM_RINGDB_NO_CANDIDATE};
  if (db->shard_count == 1) {
    if (search) {
      const int rc = dsm_ringdb_knn_packed_host(db, key, 1, packed);
      if (rc) return rc;
    }
  } else {
    DSM_HIP(hipSetDevice(db->ctx->device));
    // Local part first; whatever goes wrong here is agreed upon by ALL ranks (round 0, also when the index is still too small
    // to be searched: the ranks must agree on that as well) before any of them enters the merge rounds -- a rank that
    // returned early on its own would leave the others waiting in an all-reduce.
    auto local_scan = [&]() -> int {
      if ((size_t)db->k > db->out_words) {
        if (db->d_out) DSM_HIP(hipFree(db->d_out));
        db->d_out = nullptr;
        db->out_words = 0;
        DSM_HIP(hipMalloc(&db->d_out, 4 * sizeof(unsigned long long)));
        db->out_words = 4;
      }
      const int r = rdb_stage(db, (size_t)db->dim);
      if (r) return r;
      DSM_HIP(hipMemcpyAsync(db->d_q, key, sizeof(float) * db->dim, hipMemcpyHostToDevice, db->ctx->stream));
      return rdb_knn_dev(db, db->d_q, 1, db->d_out);
    };
    const int rc_local = search ? local_scan() : DSM_OK;
    const std::string why = rc_local ? dsm_last_error() : "";
    int rc = ringdb_agree(db, rc_local == DSM_OK, why.c_str());
    if (rc) return rc_local ? rc_local : rc;
    if (search) {
      rc = ringdb_merge_attached(db, db->d_out, 1);
      if (rc) return rc;
      DSM_HIP(hipMemcpyAsync(packed, db->d_out, sizeof(unsigned long long) * db->k, hipMemcpyDeviceToHost, db->ctx->stream));
      DSM_HIP(hipStreamSynchronize(db->ctx->stream));
    }
  }
  for (int i = 0; search && i < db->k; i++) {
    if (packed[i] == DSM_RINGDB_NO_CANDIDATE) continue; // dist >= RINGKEY_THRES was filtered on the device
    const int idx = (int)(packed[i] & 0xFFFFFFFFll);
    if (idx > 0) cand_out[nc++] = idx - 1; // :34-38
  }
  *ncand_out = nc;
  return dsm_ringdb_enqueue(db, key);
}

/* search_ringkey of n sequences in one call, each against its own index: one upload, one scan launch over all indexes, one merge, one
 * insert of the keys that mature during the call, one read-back and one synchronisation */
int dsm_ringdb_query_then_enqueue_many(int n, dsm_ringdb *const *dbs, const float *keys, int *cand_out, int *ncand_out) {
  if (!keys || !cand_out || !ncand_out) return invalid("dsm_ringdb_query_then_enqueue_many: bad argument");
  RingManyPlan P;
  int rc = ringdb_many_prepare(nullptr, n, dbs, -1, "dsm_ringdb_query_then_enqueue_many", P);
  if (rc) return rc;
  dsm_context *ctx = P.uniq[0]->ctx;
  // device [queries | staged | scratch | candidates], page-locked mirror [queries | staged | candidates]
  CallArena A;
  const size_t o_q = A.in.take(sizeof(float) * (size_t)n * P.dim), o_staged = A.in.take(P.staged_bytes);
  const size_t o_scratch = A.work.take(sizeof(unsigned long long) * ringdb_many_scratch_words(P));
  const size_t pk_bytes = sizeof(unsigned long long) * (size_t)n * P.k, o_packed = A.out.take(pk_bytes);
  if ((rc = A.bind(ctx))) return rc;
  memcpy(A.host_in<float>(o_q), keys, sizeof(float) * (size_t)n * P.dim);
  ringdb_many_stage(P, A.host_in<unsigned char>(o_staged));
  if ((rc = A.upload())) return rc;
  rc = ringdb_many_launch(ctx->stream, P, A.dev_in<unsigned char>(o_staged), A.dev_in<float>(o_q), A.dev_work<unsigned long long>(o_scratch),
                          A.dev_out<unsigned long long>(o_packed));
  if (rc) return rc;
  if ((rc = A.fetch(pk_bytes))) return rc;
  std::vector<const float *> kp(n);
  for (int j = 0; j < n; j++) kp[j] = keys + (size_t)j * P.dim;
  ringdb_many_finish(P, dbs, kp.data(), A.host_out<unsigned long long>(o_packed), cand_out, ncand_out);
  return DSM_OK;
}

} // extern "C"
