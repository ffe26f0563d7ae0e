// hfcl_host_listed.hpp -- host side of the listed-leaf pipeline (the kernels: hfcl_listed.hpp), written once for its kinds: the chunk
// driver of the device form (count, scan, list, solve, fold), the bodies of the *_collide_batch_device / *_collide_batch entry points,
// and the chunked copy / compute / copy of a host form.  Behind them the same three pieces for the octrees' distance() calls (one launch
// per chunk, no workspace of their own, nothing read back).  Included by hfcl_host_hfield.hip and hfcl_host_octree.hip, each of which
// defines its kinds: structs of static functions and strings.  Both kinds of kind have --
//   Args, ws(lib), n_containers(lib)     the kernels' parameter block, the library's workspace of the kind, its registered containers
//   upload(lib), fill(lib, a)            the kind's tables on the device; its part of the block
//   chunk(lib)                           queries per chunk
//   supported(type)                      a shape the kind has an evaluator for
//   check(who, lib, shape, n)            what it refuses of a batch beyond that (listed_no_check: nothing); shape: null in a device form
//   noun, a_noun                         "octree", "an octree"
// a collide kind --
//   ids(a, p), item_cap(lib), limit_who  its array of container ids; its items option; its name in the driver's limit message
//   request(who, req, q, skip_all)       what every form checks of a request before any work
//   count(st, a), solve(st, a, ...)      the kind's launches
// a distance kind (its ws(lib) is a collide kind's: the host form borrows the staging buffers and the count buffer) --
//   ptrs(a, ids, tf_c, tf_2)             the chunk's container ids and the two pose arrays, by their names in the block
//   request(who, req, q), launch(st, a)  the request checks, "null request" included; the one launch of a chunk
//   timer                                its entry of last_kernel_breakdown()
#pragma once
#include "hfcl_host.hpp"

constexpr size_t LISTED_AUTO_CHUNK = 65536;          // queries per chunk when the kind's chunk option is 0
constexpr uint64_t LISTED_ITEM_SOFT_CAP = 1u << 20;  // a chunk is cut down (to one query at the least) while it lists more items than this (the kind's items option)
// (LISTED_ITEM_HARD_CAP, hfcl_host.hpp: ... and a single query that lists more is refused)

// The call on device pointers: queries [0, n) in chunks; pair0: the index of query 0 in the caller's batch; first: this is the first
// part of that batch (the running contact count starts at 0)
template <class K>
int listed_run(hfcl_lib* lib, const uint32_t* d_id, const uint32_t* d_shape, const double* d_tfc, const double* d_tfs, size_t n,
               const uint8_t* d_swapped, const hfcl_collision_request* req, const QParams<double>& q, bool skip_all, hfcl_result* d_out, double* d_dlb,
               hfcl_contact* d_contacts, size_t contacts_cap, bool want_contacts, uint32_t pair0, bool first, hipStream_t st) {
  auto& w = K::ws(lib);
  const int rc = K::upload(lib);
  if (rc) return rc;
  if (!w.h_words) HIP_TRY(w.h_words.alloc(2));
  HIP_TRY(w.d_running.grow(1));
  if (first) HIP_TRY(hipMemsetAsync(w.d_running, 0, sizeof(uint64_t), st));
  const size_t chunk = std::min(K::chunk(lib), n);
  HIP_TRY(w.d_counts.grow(chunk));
  HIP_TRY(w.d_ccounts.grow(chunk));
  HIP_TRY(w.d_offsets.grow(chunk + 1));
  HIP_TRY(w.d_coffsets.grow(chunk + 1));
  HIP_TRY(w.d_box_total.grow(chunk));
  for (auto& t : lib->timers) t.used = false;
  const bool timed = lib->kernel_timing;
  hipEvent_t e0[LISTED_TIMED_KERNELS], e1[LISTED_TIMED_KERNELS];
  const char* names[LISTED_TIMED_KERNELS];
  if (timed)
    for (int k = 0; k < LISTED_TIMED_KERNELS; ++k) {
      KernelTime* t = timer_slot(lib, size_t(k), "");
      e0[k] = t->e0;
      e1[k] = t->e1;
    }
  typename K::Args a;
  a.shapes = lib->d_shapes64;
  a.verts = lib->d_verts64;
  a.n_shapes = uint32_t(lib->n_shapes);
  K::fill(lib, a);
  a.q = q;
  a.bd2 = req->break_distance * req->break_distance;
  a.num_max_contacts = req->num_max_contacts;
  a.skip_all = skip_all ? 1 : 0;
  a.counts = w.d_counts;
  a.offsets = w.d_offsets;
  a.box_total = w.d_box_total;
  a.ccounts = w.d_ccounts;
  a.coffsets = w.d_coffsets;
  a.running = w.d_running;
  a.contacts = d_contacts;
  a.contacts_cap = d_contacts ? contacts_cap : 0;
  // A chunk that was cut leaves the counts of the queries behind the cut in place: `left` of them from w.d_counts + at on.  The next
  // chunk is those queries and scans their counts again instead of walking them (and every query still to come) once more
  size_t left = 0, at = 0;
  for (size_t q0 = 0; q0 < n;) {  // (every pass takes at least one query)
    size_t m = left ? left : std::min(chunk, n - q0);
    K::ids(a, d_id + q0);
    a.shape = d_shape + q0;
    a.tf_c = d_tfc + 12 * q0;
    a.tf_s = d_tfs + 12 * q0;
    a.swapped = d_swapped ? d_swapped + q0 : nullptr;
    a.out = d_out + q0;
    a.dlb = d_dlb ? d_dlb + q0 : nullptr;
    a.pair0 = pair0 + uint32_t(q0);
    a.m = uint32_t(m);
    a.items = w.d_items;
    a.leaves = w.d_leaves;
    a.n_items = 0;
    if (left) {
      a.counts = w.d_counts.get() + at;
      launch_hf_scan(st, a.counts, a.offsets, a.m, nullptr);
    } else {
      a.counts = w.d_counts;
      at = 0;
      K::count(st, a);
    }
    const size_t counted = m;
    // the one read-back of a chunk: its item count (the item workspace is sized by it); a chunk that lists too much is cut at a query
    uint64_t total = 0;
    for (;;) {  // (m at least halves per pass)
      HIP_TRY(hipMemcpyAsync(w.h_words, w.d_offsets.get() + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      total = w.h_words[0];
      if (total <= K::item_cap(lib) || m == 1) break;
      m = m / 2;
    }
    if (total > LISTED_ITEM_HARD_CAP) {
      set_error(std::string(K::limit_who) + ": one query lists " + std::to_string(total) + " leaves (limit 2^26)");
      return HFCL_ERR_LIMIT;
    }
    if (total > w.d_items.capacity()) {
      const size_t want = size_t(total + total / 4 + 1024);
      HIP_TRY(w.d_items.grow(want));
      HIP_TRY(w.d_leaves.grow(want));
    }
    a.m = uint32_t(m);
    a.items = w.d_items;
    a.leaves = w.d_leaves;
    a.n_items = total;
    K::solve(st, a, lib->n_cus * 16, want_contacts, names, timed ? e0 : nullptr, timed ? e1 : nullptr);
    if (timed)
      for (int k = 0; k < LISTED_TIMED_KERNELS; ++k) lib->timers[size_t(k)].name = names[k];
    q0 += m;
    left = counted - m;
    at += m;
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

// What the entry points on arrays refuse after their request checks, in this order: null arrays, a batch too large
inline int listed_check_arrays(const char* who, const void* id, const void* shape, const void* tf_c, const void* tf_s, const void* out, size_t n) {
  if (!id || !shape || !tf_c || !tf_s || !out) {
    set_error(std::string(who) + ": null buffer");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  return HFCL_OK;
}

// A kind's check() that refuses nothing
inline int listed_no_check(const char*, hfcl_lib*, const uint32_t*, size_t) { return HFCL_OK; }

// What a host form refuses of its queries: an id outside the library, a solid without an evaluator ("<verb> function between <a_noun> and ...")
inline int listed_check_queries(const char* who, const hfcl_lib* lib, const uint32_t* id, size_t n_containers, const uint32_t* shape, size_t n,
                                const char* noun, const char* a_noun, const char* verb, int (*supported)(int32_t)) {
  for (size_t i = 0; i < n; ++i) {
    if (id[i] >= n_containers || shape[i] >= lib->n_shapes) {
      set_error(std::string(who) + ": " + noun + " / shape id outside the library at query " + std::to_string(i));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    if (!supported(lib->h_shapes[shape[i]].type)) {
      set_error(std::string(verb) + " function between " + a_noun + " and node type " + std::to_string(lib->h_shapes[shape[i]].type) + " is not yet supported.");
      return HFCL_ERR_UNSUPPORTED_PAIR;
    }
  }
  return HFCL_OK;
}

// The chunks of a host form on the workspace's stream: a chunk's arrays to the staging buffers, run(q0, m) on them, then its records
// -- and, where `second` is given, m elements of d_second -- to the host; the stream is waited for after every chunk (the staging
// buffers are the next chunk's).  The caller has grown what d_second points into
template <class Ws, class T2, class Run>
int listed_staged(const char* who, Ws& w, size_t chunk, const uint32_t* id, const uint32_t* shape, const double* tf_c, const double* tf_s, size_t n,
                  const uint8_t* swapped, hfcl_result* out, T2* second, const T2* d_second, Run run) {
  hipStream_t st = w.st;
  HIP_TRY(w.s_id.grow(chunk));
  HIP_TRY(w.s_shape.grow(chunk));
  HIP_TRY(w.s_tf_a.grow(12 * chunk));
  HIP_TRY(w.s_tf_s.grow(12 * chunk));
  HIP_TRY(w.s_swapped.grow(chunk));
  HIP_TRY(w.s_out.grow(chunk));
  for (size_t q0 = 0; q0 < n; q0 += chunk) {
    const size_t m = std::min(chunk, n - q0);
    bool ok = hipMemcpyAsync(w.s_id, id + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(w.s_shape, shape + q0, m * sizeof(uint32_t), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(w.s_tf_a, tf_c + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(w.s_tf_s, tf_s + 12 * q0, m * 12 * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && (!swapped || hipMemcpyAsync(w.s_swapped, swapped + q0, m, hipMemcpyHostToDevice, st) == hipSuccess);
    if (ok) {
      if (const int rc = run(q0, m)) return rc;
      ok = hipMemcpyAsync(out + q0, w.s_out, m * sizeof(hfcl_result), hipMemcpyDeviceToHost, st) == hipSuccess;
      ok = ok && (!second || hipMemcpyAsync(second + q0, d_second, m * sizeof(T2), hipMemcpyDeviceToHost, st) == hipSuccess);
      ok = ok && hipStreamSynchronize(st) == hipSuccess;
    }
    if (!ok) {
      set_error(std::string(who) + ": HIP copy failed");
      return HFCL_ERR_HIP;
    }
  }
  return HFCL_OK;
}

// The body of a kind's *_collide_batch_device
template <class K>
int listed_collide_device(const char* who, hfcl_lib* lib, const uint32_t* d_id, const uint32_t* d_shape, const double* d_tf_c, const double* d_tf_s,
                          size_t n, const uint8_t* d_swapped, const hfcl_collision_request* req, hfcl_result* d_out, double* d_dlb,
                          hfcl_contact* d_contacts, size_t max_contacts_total, size_t* n_contacts_out, hipStream_t st) {
  if (int rc = no_device()) return rc;
  if (!lib || !req) {
    set_error(std::string(who) + ": null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  bool skip_all = false;
  if (int rc = K::request(who, req, q, skip_all)) return rc;
  if (n)  // (before the count is zeroed, as a refusal of the request)
    if (int rc = K::check(who, lib, nullptr, n)) return rc;
  if (n_contacts_out) *n_contacts_out = 0;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays(who, d_id, d_shape, d_tf_c, d_tf_s, d_out, n)) return rc;
  HIP_TRY(hipSetDevice(lib->device));
  const bool want_contacts = d_contacts || n_contacts_out;
  const int rc = listed_run<K>(lib, d_id, d_shape, d_tf_c, d_tf_s, n, d_swapped, req, q, skip_all, d_out, d_dlb, d_contacts, max_contacts_total,
                               want_contacts, 0u, true, st);
  if (rc) return rc;
  if (n_contacts_out) HIP_TRY(listed_contacts_back(K::ws(lib), st, n_contacts_out));
  return HFCL_OK;
}

// The body of a kind's *_collide_batch: a chunked copy / compute / copy around listed_run on the workspace's stream
template <class K>
int listed_collide_host(const char* who, hfcl_lib* lib, const uint32_t* id, const uint32_t* shape, const double* tf_c, const double* tf_s, size_t n,
                        const uint8_t* swapped, const hfcl_collision_request* req, hfcl_result* out, double* distance_lower_bound,
                        hfcl_contact* contacts, size_t max_contacts_total, size_t* n_contacts_out) {
  if (int rc = no_device()) return rc;
  if (!lib || !req) {
    set_error(std::string(who) + ": null library / request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<double> q;
  bool skip_all = false;
  if (int rc = K::request(who, req, q, skip_all)) return rc;
  if (n && shape)  // (no shape array: refused below as a null buffer)
    if (int rc = K::check(who, lib, shape, n)) return rc;
  if (n_contacts_out) *n_contacts_out = 0;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays(who, id, shape, tf_c, tf_s, out, n)) return rc;
  if (int rc = listed_check_queries(who, lib, id, K::n_containers(lib), shape, n, K::noun, K::a_noun, "Collision", K::supported)) return rc;
  HIP_TRY(hipSetDevice(lib->device));
  auto& w = K::ws(lib);
  if (!w.st) HIP_TRY(w.st.create());
  hipStream_t st = w.st;
  const size_t chunk = std::min(K::chunk(lib), n);
  const bool want_contacts = contacts || n_contacts_out;
  const size_t ccap = listed_contact_cap(contacts, max_contacts_total, n, req);
  HIP_TRY(w.s_dlb.grow(chunk));
  if (ccap) HIP_TRY(w.s_contacts.grow(ccap));
  int rc = listed_staged(who, w, chunk, id, shape, tf_c, tf_s, n, swapped, out, distance_lower_bound, w.s_dlb.get(), [&](size_t q0, size_t m) {
    return listed_run<K>(lib, w.s_id, w.s_shape, w.s_tf_a, w.s_tf_s, m, swapped ? w.s_swapped.get() : nullptr, req, q, skip_all, w.s_out,
                         distance_lower_bound ? w.s_dlb.get() : nullptr, ccap ? w.s_contacts.get() : nullptr, ccap, want_contacts, uint32_t(q0),
                         q0 == 0, st);
  });
  if (!rc && want_contacts && listed_contacts_back(w, st, n_contacts_out, contacts, ccap) != hipSuccess) {
    set_error(std::string(who) + ": HIP copy failed");
    rc = HFCL_ERR_HIP;
  }
  hipStreamSynchronize(st);
  return rc;
}

// ---- distance(): one launch per chunk ---------------------------------------------------------------------------------------------
// one entry of last_kernel_breakdown() around the launches of a call (a name of its own: hfcl_host_batch.hip has a Timed)
struct ListedTimed {
  hfcl_lib* lib = nullptr;
  hipStream_t st;
  ListedTimed(hfcl_lib* l, const char* name, hipStream_t s) : st(s) {
    for (auto& t : l->timers) t.used = false;
    if (!l->kernel_timing) return;
    lib = l;
    (void)hipEventRecord(timer_slot(lib, 0, name)->e0, st);
  }
  ~ListedTimed() {
    if (lib) (void)hipEventRecord(lib->timers[0].e1, st);
  }
  ListedTimed(const ListedTimed&) = delete;
};

// The call on device pointers: queries [0, n) in chunks, one launch each; nothing is read back
template <class D>
int listed_distance_run(hfcl_lib* lib, const uint32_t* d_id, const uint32_t* d_shape, const double* d_tfc, const double* d_tf2, size_t n,
                        const uint8_t* d_swapped, const QParams<double>& q, hfcl_result* d_out, uint32_t* d_visited, hipStream_t st) {
  if (int rc = D::upload(lib)) return rc;
  typename D::Args a;
  a.shapes = lib->d_shapes64;
  a.n_shapes = uint32_t(lib->n_shapes);
  D::fill(lib, a);
  a.q = q;
  const size_t chunk = std::min(D::chunk(lib), n);
  ListedTimed t(lib, D::timer, st);
  for (size_t q0 = 0; q0 < n; q0 += chunk) {
    D::ptrs(a, d_id + q0, d_tfc + 12 * q0, d_tf2 + 12 * q0);
    a.shape = d_shape + q0;
    a.swapped = d_swapped ? d_swapped + q0 : nullptr;
    a.out = d_out + q0;
    a.n_visited = d_visited ? d_visited + q0 : nullptr;
    a.m = uint32_t(std::min(chunk, n - q0));
    D::launch(st, a);
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

// What both distance bodies refuse first: no device, a null library, the request
template <class D>
int listed_distance_checks(const char* who, hfcl_lib* lib, const hfcl_distance_request* req, QParams<double>& q) {
  if (int rc = no_device()) return rc;
  if (!lib) {
    set_error(std::string(who) + ": null library");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return D::request(who, req, q);
}

// The body of a kind's *_distance_batch_device
template <class D>
int listed_distance_device(const char* who, hfcl_lib* lib, const uint32_t* d_id, const uint32_t* d_shape, const double* d_tf_c, const double* d_tf_2,
                           size_t n, const uint8_t* d_swapped, const hfcl_distance_request* req, hfcl_result* d_out, uint32_t* d_visited, hipStream_t st) {
  QParams<double> q;
  if (int rc = listed_distance_checks<D>(who, lib, req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays(who, d_id, d_shape, d_tf_c, d_tf_2, d_out, n)) return rc;
  if (int rc = D::check(who, lib, nullptr, n)) return rc;
  HIP_TRY(hipSetDevice(lib->device));
  return listed_distance_run<D>(lib, d_id, d_shape, d_tf_c, d_tf_2, n, d_swapped, q, d_out, d_visited, st);
}

// The body of a kind's *_distance_batch: staged in pieces of the chunk option -- the staging buffers are the collide call's of the kind's
// workspace, the visited counts go through its count buffer
template <class D>
int listed_distance_host(const char* who, hfcl_lib* lib, const uint32_t* id, const uint32_t* shape, const double* tf_c, const double* tf_2, size_t n,
                         const uint8_t* swapped, const hfcl_distance_request* req, hfcl_result* out, uint32_t* n_visited) {
  QParams<double> q;
  if (int rc = listed_distance_checks<D>(who, lib, req, q)) return rc;
  if (n == 0) return HFCL_OK;
  if (int rc = listed_check_arrays(who, id, shape, tf_c, tf_2, out, n)) return rc;
  if (int rc = D::check(who, lib, shape, n)) return rc;
  if (int rc = listed_check_queries(who, lib, id, D::n_containers(lib), shape, n, D::noun, D::a_noun, "Distance", D::supported)) return rc;
  HIP_TRY(hipSetDevice(lib->device));
  auto& w = D::ws(lib);
  if (!w.st) HIP_TRY(w.st.create());
  const size_t chunk = std::min(D::chunk(lib), n);
  HIP_TRY(w.d_counts.grow(chunk));
  const int rc = listed_staged(who, w, chunk, id, shape, tf_c, tf_2, n, swapped, out, n_visited, w.d_counts.get(), [&](size_t, size_t m) {
    return listed_distance_run<D>(lib, w.s_id, w.s_shape, w.s_tf_a, w.s_tf_s, m, swapped ? w.s_swapped.get() : nullptr, q, w.s_out,
                                  n_visited ? w.d_counts.get() : nullptr, w.st);
  });
  hipStreamSynchronize(w.st);
  return rc;
}
