// mals_group.cpp -- the multi-GPU half-iteration of include/myrrix_als.h, built
// entirely on the per-GPU C-ABI of mals_api.hip and mals_serving.hip plus streams, events and the exchange.
//
// The reference runs one process with N worker threads, every output row written by exactly one of
// them (ALS:391-410, ALS:497-499); here the workers are GPUs, a row belongs to the rank whose slice
// holds it, and the only communication per half-iteration is (1) the k x k fp64 sum of the partial
// Gramians and (2) the freshly solved rows of every slice into every replica -- an all-gather with
// per-rank counts, issued chunk by chunk behind the solve.
//
// RCCL is resolved with dlopen at group creation (no link-time dependency for single-GPU users; inside
// a process that already loaded PyTorch's copy the same library is reused).  Collectives of several
// local members are always enclosed in ncclGroupStart/End (one thread drives all devices), and every RCCL call
// of a rank is issued on that rank's comm stream -- a communicator is never used from two streams at once.
#include "../../include/myrrix_als.h"
#include "mals_internal.h"
#include "hip_buffer.h"
#include "factor_digest.h"
#include "group_plan.h"
#include "generation_group_plan.h"
#include "convergence.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <thread>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

namespace {

struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommCuDevice)(const ncclComm_t, int*) = nullptr;
  std::string forced;  // mals_group_use_transport: this library and no other

  bool load(std::string& err) {
    if (lib) return true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    // No environment variable selects the library: what gets loaded as "RCCL" into a server process is decided by the
    // process itself (mals_group_use_transport: a particular RCCL build, or the tests' stand-in transport).
    if (!forced.empty()) {
      lib = dlopen(forced.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (!lib) {
        const char* e = dlerror();  // once: dlerror() clears its state
        err = "transport library " + forced + " could not be loaded: " + (e ? e : "");
        return false;
      }
    }
    for (const char* n : names) {
      if (lib) break;
      lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);  // a copy the process already mapped (e.g. PyTorch's) first
    }
    std::string first_error;
    for (const char* n : names) {
      if (lib) break;
      lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (!lib && first_error.empty()) {  // right behind the failing dlopen: later attempts overwrite the message
        const char* e = dlerror();
        first_error = e ? e : "";
      }
    }
    if (!lib) {
      err = "librccl.so.1 could not be loaded: " + first_error;
      return false;
    }
#define MALS_SYM(field, name)                                                  \
  field = reinterpret_cast<decltype(field)>(dlsym(lib, name));                 \
  if (!field) {                                                                \
    err = std::string("RCCL symbol missing: ") + name;                         \
    dlclose(lib);                                                              \
    lib = nullptr;                                                             \
    return false;                                                              \
  }
    MALS_SYM(GetUniqueId, "ncclGetUniqueId")
    MALS_SYM(CommInitRank, "ncclCommInitRank")
    MALS_SYM(CommInitAll, "ncclCommInitAll")
    MALS_SYM(CommDestroy, "ncclCommDestroy")
    MALS_SYM(AllReduce, "ncclAllReduce")
    MALS_SYM(Send, "ncclSend")
    MALS_SYM(Recv, "ncclRecv")
    MALS_SYM(GroupStart, "ncclGroupStart")
    MALS_SYM(GroupEnd, "ncclGroupEnd")
    MALS_SYM(GetErrorString, "ncclGetErrorString")
    MALS_SYM(CommCount, "ncclCommCount")
    MALS_SYM(CommUserRank, "ncclCommUserRank")
    MALS_SYM(CommCuDevice, "ncclCommCuDevice")
#undef MALS_SYM
    return true;
  }
};

Rccl g_rccl;

struct Member {
  mals_handle h = nullptr;
  int device = 0;
  int rank = 0;
  mals::Stream compute, comm;
  mals::Stream compute2;   // odd chunks of a half-iteration (alternate_streams)
  mals::Event ev_solved, ev_exchanged;
  mals::Event ev_half, ev_join;
  ncclComm_t nccl = nullptr;
  mals::DeviceBuffer<double> d_gp;    // k*k: partial Gramian / all-reduce buffer
  mals::DeviceBuffer<double> d_stat;  // 4 doubles: value statistics, status
  mals::DeviceBuffer<float> d_ymax;   // max |element| of the rows of this member's partial Gramian (bit pattern = non-negative float)
  float* F[2] = {nullptr, nullptr};
  mals::DeviceBuffer<int64_t> d_row_ptr[2];  // rebased row pointers of borrowed device matrices
  // mals_ingest_install_group: the member's slices when the ingest lives on ANOTHER device (peer copies), and its slice of
  // knownItemIDs (rebased offsets always; the indices only when copied)
  mals::DeviceBuffer<int32_t> own_col[2];
  mals::DeviceBuffer<float> own_val[2];
  mals::DeviceBuffer<int64_t> own_known_ptr;
  mals::DeviceBuffer<int32_t> own_known_idx;
  mals::DeviceBuffer<int64_t> own_tag_idx;
  // chunked upload
  int64_t up_rows = 0;
};

}  // namespace

struct mals_group_s {
  mals_config cfg;
  int world = 1;
  int backend = MALS_GROUP_RCCL;
  bool single_process = true;
  std::vector<Member> m;
  int64_t n_total[2] = {0, 0};
  int64_t n_rows[2] = {0, 0};
  std::vector<int64_t> bounds[2];
  std::vector<int64_t> up_row_ptr[2];  // chunked upload: the full row_ptr
  int64_t up_next_row[2] = {0, 0};
  int exchange_chunks = 4;        // what the NEXT matrix upload of a side is cut into
  int side_chunks[2] = {4, 4};    // what each side's CURRENT matrix was cut into (plan_side): the members' work lists are
                                  // built for this count, so the solve loop, the exchange ranges and the members agree
  // Consecutive chunks of a half-iteration on two alternating compute streams: every chunk boundary otherwise drains the
  // persistent kernels (rows, long rows, dual classes each have a tail) -- +3.7 % at 4 chunks on C4 (round 3).  A chunk's
  // completion event goes to the exchange stream as before; the streams are joined before anything that assumes one.
  bool alternate_streams = true;
  std::atomic<int> cancelled{0};
  mals_iteration_fn iter_fn = nullptr;   // mals_group_set_iteration_callback
  void* iter_user = nullptr;
  // the online write path (mals_group_set_preferences ...): two writes reach every member's serving front in the same
  // order (updates that share a row do not commute); the reads take no lock and rotate over the local members
  std::mutex write_mu;
  std::mutex err_mu;                   // the failure text of a read: request threads share the group's string
  std::atomic<uint32_t> next_reader{0};
  std::atomic<int64_t> users_end{0};   // rows of the X replicas: users past the installed matrix belong to the last rank
  // mals_group_load_generation changes bounds[X] and every member's slice while request threads route by them: odd while a load
  // runs; a routed read that began under another value is repeated (route_by_owner)
  std::atomic<uint64_t> generation_seq{0};
  std::string err;
};

namespace {

int gfail(mals_group g, int code, const std::string& msg) {
  if (g) g->err = msg;
  return code;
}

#define GHIP(g, call)                                                                                   \
  do {                                                                                                  \
    hipError_t _e = (call);                                                                             \
    if (_e != hipSuccess) return gfail(g, _e == hipErrorOutOfMemory ? MALS_OOM : MALS_HIP_ERROR,        \
                                       std::string(#call) + ": " + hipGetErrorString(_e));              \
  } while (0)

#define GNCCL(g, call)                                                                                  \
  do {                                                                                                  \
    ncclResult_t _r = (call);                                                                           \
    if (_r != ncclSuccess) return gfail(g, MALS_COMM_ERROR, std::string(#call) + ": " + g_rccl.GetErrorString(_r)); \
  } while (0)

// a member call failed: keep its message
int mfail(mals_group g, const Member& mb, int rc) {
  return gfail(g, rc, std::string("rank ") + std::to_string(mb.rank) + ": " + mals_last_error(mb.h));
}

#define GSIDE(g, side)                                                                    \
  do {                                                                                    \
    if (!(g)) return MALS_INVALID_ARG;                                                    \
    if ((side) != MALS_SIDE_X && (side) != MALS_SIDE_Y) return gfail(g, MALS_INVALID_ARG, "side must be MALS_SIDE_X or _Y"); \
  } while (0)

int64_t chunk_rows_of(const mals_group g, int side, int rank) {
  return mals::chunk_rows_of(g->bounds[side][(size_t)rank], g->bounds[side][(size_t)rank + 1], g->side_chunks[side]);
}

// rows [lo, hi) (global) of chunk c of rank's slice
void chunk_range(const mals_group g, int side, int rank, int c, int64_t* lo, int64_t* hi) {
  mals::chunk_range(g->bounds[side][(size_t)rank], g->bounds[side][(size_t)rank + 1], g->side_chunks[side], c, lo, hi);
}

// Every local member in turn with its device current (one thread drives all devices: the set-device before a member's HIP
// calls is part of their correctness).  body(member) or body(member, i) -> status; the first failure ends the loop.
template <class Body>
int for_members(mals_group g, Body&& body) {
  for (size_t i = 0; i < g->m.size(); ++i) {
    Member& mb = g->m[i];
    GHIP(g, hipSetDevice(mb.device));
    int rc;
    if constexpr (std::is_invocable_v<Body, Member&, size_t>) rc = body(mb, i); else rc = body(mb);
    if (rc) return rc;
  }
  return MALS_OK;
}

// `to` goes on behind everything `from` holds now
int hand_off(mals_group g, hipStream_t from, hipEvent_t ev, hipStream_t to) {
  GHIP(g, hipEventRecord(ev, from));
  GHIP(g, hipStreamWaitEvent(to, ev, 0));
  return MALS_OK;
}

int sync_comm(mals_group g) {
  return for_members(g, [&](Member& mb) -> int {
    GHIP(g, hipStreamSynchronize(mb.comm));
    return MALS_OK;
  });
}

int init_member(mals_group g, Member& mb, const mals_config& cfg, int device, int rank) {
  mb.device = -1;   // until the handle exists: destroy_member must not select a device that may not be there
  mb.rank = rank;
  mals_config c = cfg;
  c.device = device;
  if (int rc = mals_create(&c, &mb.h)) {
    char why[512];
    (void)mals_create_error(why, sizeof(why));
    return gfail(g, rc, std::string(why[0] ? why : "mals_create failed") + " (group member " + std::to_string(rank) + ", device " + std::to_string(device) + ")");
  }
  malsi_mark_group_member(mb.h);
  mb.device = device;
  GHIP(g, hipSetDevice(device));
  GHIP(g, mb.compute.ensure());
  GHIP(g, mb.comm.ensure());
  GHIP(g, mb.compute2.ensure());
  GHIP(g, mb.ev_half.ensure(hipEventDisableTiming));
  GHIP(g, mb.ev_join.ensure(hipEventDisableTiming));
  GHIP(g, mb.ev_solved.ensure(hipEventDisableTiming));
  GHIP(g, mb.ev_exchanged.ensure(hipEventDisableTiming));
  GHIP(g, hipEventRecord(mb.ev_exchanged, mb.comm));
  const size_t kk = (size_t)cfg.features * cfg.features;
  GHIP(g, mb.d_gp.alloc(kk));
  GHIP(g, mb.d_stat.alloc(4));
  GHIP(g, mb.d_ymax.alloc((size_t)malsi_ymax_slots()));
  if (int rc = mals_set_stream(mb.h, mb.compute)) return mfail(g, mb, rc);
  return MALS_OK;
}

void destroy_member(Member& mb) {
  if (mb.device >= 0) (void)hipSetDevice(mb.device);
  if (mb.compute) (void)hipStreamSynchronize(mb.compute);
  if (mb.compute2) (void)hipStreamSynchronize(mb.compute2);
  if (mb.comm) (void)hipStreamSynchronize(mb.comm);
  if (mb.nccl && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(mb.nccl);
  if (mb.h) (void)mals_destroy(mb.h);   // before `compute`, which it borrows
  mb = Member();   // the member's streams, events and buffers, with its device current
}

// ---- the collectives: each stated once, with both transports (RCCL, peer copy) inside ----

// One ncclGroupStart/End around the RCCL calls of every local member (one thread drives all devices).  call(member, i) issues
// local member i's calls on ITS comm stream -- a communicator is never used from two streams at once -- and returns the first
// result that is not ncclSuccess: the group is then ended, that result ignored, and the failure is "<label>: <RCCL's text>".
template <class Call>
int rccl_group(mals_group g, const char* label, Call&& call) {
  GNCCL(g, g_rccl.GroupStart());
  for (size_t i = 0; i < g->m.size(); ++i) {
    const ncclResult_t r = call(g->m[i], i);
    if (r != ncclSuccess) {
      (void)g_rccl.GroupEnd();
      return gfail(g, MALS_COMM_ERROR, std::string(label) + ": " + g_rccl.GetErrorString(r));
    }
  }
  GNCCL(g, g_rccl.GroupEnd());
  return MALS_OK;
}

// one all-reduce in place: dev[i] = local member i's n elements of ncclDouble or ncclInt64 (ncclSum, ncclMax) or ncclFloat (ncclMax
// of non-negative values)
struct Reduce {
  void* const* dev;
  size_t n;
  ncclDataType_t type;
  ncclRedOp_t op;
  size_t bytes() const { return n * (type == ncclFloat ? sizeof(float) : sizeof(double)); }
};

void reduce_identity(const Reduce& r, void* acc) {
  if (r.type == ncclDouble) std::fill_n(static_cast<double*>(acc), r.n, r.op == ncclMax ? -std::numeric_limits<double>::infinity() : 0.0);
  else if (r.type == ncclInt64) std::fill_n(static_cast<int64_t*>(acc), r.n, r.op == ncclMax ? std::numeric_limits<int64_t>::min() : 0);
  else std::fill_n(static_cast<float*>(acc), r.n, 0.f);
}

template <class T>
void reduce_fold(T* acc, const T* v, size_t n, ncclRedOp_t op) {
  for (size_t i = 0; i < n; ++i) acc[i] = op == ncclMax ? std::max(acc[i], v[i]) : acc[i] + v[i];
}

void reduce_fold(const Reduce& r, void* acc, const void* v) {
  if (r.type == ncclDouble) return reduce_fold(static_cast<double*>(acc), static_cast<const double*>(v), r.n, r.op);
  if (r.type == ncclInt64) return reduce_fold(static_cast<int64_t*>(acc), static_cast<const int64_t*>(v), r.n, r.op);
  float* a = static_cast<float*>(acc);
  const float* f = static_cast<const float*>(v);
  for (size_t i = 0; i < r.n; ++i)
    if (!(f[i] <= a[i])) a[i] = f[i];   // an inf pattern wins and makes the consumer fall back
}

// when an all-reduce over RCCL counts as done: the host waits for the comm streams (status words, value statistics, the
// ingest's counters), or -- no host wait -- the comm streams start behind the compute streams and the compute streams go on
// behind the comm streams (the Gramian: partial Gramian -> all-reduce behind whatever exchange is still queued -> solve)
enum class Done { HOST_WAITS, COMPUTE_FOLLOWS };

// The all-reduces `parts` over every rank, the results in every member's buffers.  Nothing to do for a one-rank group without
// a communicator.  RCCL: all parts of all local members in ONE group, on the comm streams.  Peer copy: staged through the
// host on the compute streams and folded in member order 0, 1, ... -- that fixed order makes this backend deterministic --
// and complete when it returns, whatever `done` says.
int all_reduce(mals_group g, std::initializer_list<Reduce> parts, Done done) {
  if (g->world == 1 && !g->m[0].nccl) return MALS_OK;
  if (g->backend == MALS_GROUP_PEER_COPY) {
    std::vector<std::vector<double>> acc, tmp;   // 8-byte words under elements of any of the three types
    for (const Reduce& r : parts) {
      acc.emplace_back((r.bytes() + 7) / 8);
      tmp.emplace_back((r.bytes() + 7) / 8);
      reduce_identity(r, acc.back().data());
    }
    for (size_t i = 0; i < g->m.size(); ++i) {
      Member& mb = g->m[i];
      GHIP(g, hipSetDevice(mb.device));
      size_t p = 0;
      for (const Reduce& r : parts) GHIP(g, hipMemcpyAsync(tmp[p++].data(), r.dev[i], r.bytes(), hipMemcpyDeviceToHost, mb.compute));
      GHIP(g, hipStreamSynchronize(mb.compute));
      p = 0;
      for (const Reduce& r : parts) reduce_fold(r, acc[p].data(), tmp[p].data()), ++p;
    }
    for (size_t i = 0; i < g->m.size(); ++i) {
      Member& mb = g->m[i];
      GHIP(g, hipSetDevice(mb.device));
      size_t p = 0;
      for (const Reduce& r : parts) GHIP(g, hipMemcpyAsync(r.dev[i], acc[p++].data(), r.bytes(), hipMemcpyHostToDevice, mb.compute));
      GHIP(g, hipStreamSynchronize(mb.compute));
    }
    return MALS_OK;
  }
  if (done == Done::COMPUTE_FOLLOWS)
    if (int rc = for_members(g, [&](Member& mb) { return hand_off(g, mb.compute, mb.ev_solved, mb.comm); })) return rc;
  const int rc = rccl_group(g, "ncclAllReduce", [&](Member& mb, size_t i) {
    ncclResult_t r = ncclSuccess;
    for (const Reduce& p : parts)
      if (r == ncclSuccess) r = g_rccl.AllReduce(p.dev[i], p.dev[i], p.n, p.type, p.op, mb.nccl, mb.comm);
    return r;
  });
  if (rc != MALS_OK) return rc;
  if (done == Done::HOST_WAITS) return sync_comm(g);
  return for_members(g, [&](Member& mb) { return hand_off(g, mb.comm, mb.ev_exchanged, mb.compute); });
}

// the d_stat words of every local member
std::vector<void*> stat_words(mals_group g) {
  std::vector<void*> dev;
  for (Member& mb : g->m) dev.push_back(mb.d_stat.get());
  return dev;
}

// every member's d_stat[0..n) <- host values (one per member), then all-reduce (op: 0 = sum, 1 = max), then read back (member 0)
int allreduce_host(mals_group g, const std::vector<std::vector<double>>& per_member, int n, int op, double* out) {
  for (size_t i = 0; i < g->m.size(); ++i) {
    Member& mb = g->m[i];
    GHIP(g, hipSetDevice(mb.device));
    GHIP(g, hipMemcpyAsync(mb.d_stat.get(), per_member[i].data(), sizeof(double) * n, hipMemcpyHostToDevice, mb.compute));
    GHIP(g, hipStreamSynchronize(mb.compute));  // the source is a pageable temporary
  }
  const std::vector<void*> dev = stat_words(g);
  if (int rc = all_reduce(g, {Reduce{dev.data(), (size_t)n, ncclDouble, op ? ncclMax : ncclSum}}, Done::HOST_WAITS)) return rc;
  Member& m0 = g->m[0];
  GHIP(g, hipSetDevice(m0.device));
  GHIP(g, hipMemcpyAsync(out, m0.d_stat.get(), sizeof(double) * n, hipMemcpyDeviceToHost, m0.compute));
  GHIP(g, hipStreamSynchronize(m0.compute));
  return MALS_OK;
}

// A status every rank agrees on: the largest code any rank saw (collective in multi-process groups).
int agree_status(mals_group g, int local_rc, const std::string& local_msg) {
  if (g->single_process) {
    if (local_rc != MALS_OK) g->err = local_msg;
    return local_rc;
  }
  std::vector<std::vector<double>> v(g->m.size(), std::vector<double>(1, (double)local_rc));
  double worst = 0.0;
  if (int rc = allreduce_host(g, v, 1, 1, &worst)) return rc;
  const int agreed = (int)worst;
  if (agreed != MALS_OK) g->err = local_rc != MALS_OK ? local_msg : "another rank reported status " + std::to_string(agreed);
  return agreed;
}

int sync_value_stats(mals_group g, int side) {
  std::vector<std::vector<double>> mx(g->m.size(), std::vector<double>(1, 0.0)), sm(g->m.size(), std::vector<double>(2, 0.0));
  for (size_t i = 0; i < g->m.size(); ++i) {
    float m = 0.f;
    double s = 0.0;
    int64_t n = 0;
    if (int rc = mals_get_value_stats(g->m[i].h, side, &m, &s, &n)) return mfail(g, g->m[i], rc);
    mx[i][0] = (double)m;
    sm[i][0] = s;
    sm[i][1] = (double)n;
  }
  double vmax = 0.0, vs[2] = {0.0, 0.0};
  if (int rc = allreduce_host(g, mx, 1, 1, &vmax)) return rc;
  if (int rc = allreduce_host(g, sm, 2, 0, vs)) return rc;
  for (Member& mb : g->m)
    if (int rc = mals_set_value_stats(mb.h, side, (float)vmax, vs[1] > 0.0 ? vs[0] / vs[1] : 0.0)) return mfail(g, mb, rc);
  return MALS_OK;
}

int refresh_replica_ptrs(mals_group g, int side) {
  for (Member& mb : g->m) {
    void* p = nullptr;
    int64_t n = 0;
    if (int rc = mals_factor_device_ptr(mb.h, side, &p, &n)) return mfail(g, mb, rc);
    mb.F[side] = static_cast<float*>(p);
  }
  return MALS_OK;
}

// slices at given bounds: every member told its chunking
int set_side_bounds(mals_group g, int side, const std::vector<int64_t>& bounds) {
  g->n_rows[side] = bounds.back();
  g->side_chunks[side] = g->exchange_chunks;
  g->bounds[side] = bounds;
  for (Member& mb : g->m)
    if (int rc = mals_set_chunk_rows(mb.h, side, chunk_rows_of(g, side, mb.rank))) return mfail(g, mb, rc);
  return MALS_OK;
}

// slices planned from the full row_ptr on the host, then set
int plan_side(mals_group g, int side, const int64_t* row_ptr, int64_t n_rows) {
  std::vector<int64_t> bounds((size_t)g->world + 1, 0);
  if (int rc = mals_plan_shards(row_ptr, n_rows, g->world, -1.0, g->cfg.features, bounds.data())) return gfail(g, rc, "mals_plan_shards failed");
  return set_side_bounds(g, side, bounds);
}

// The compute streams behind the previous exchange: a half-iteration's gather reads every row of the opposite replica.
int await_exchange(mals_group g) {
  if (int rc = for_members(g, [&](Member& mb) -> int {
        GHIP(g, hipStreamWaitEvent(mb.compute, mb.ev_exchanged, 0));
        return MALS_OK;
      }))
    return rc;
  if (!(g->single_process && g->backend == MALS_GROUP_PEER_COPY)) return MALS_OK;
  // peer copies INTO a replica run on the SOURCE's comm stream: every member also waits for every other member's exchange
  for (Member& mb : g->m)
    for (Member& other : g->m) {
      GHIP(g, hipSetDevice(mb.device));
      GHIP(g, hipStreamWaitEvent(mb.compute, other.ev_exchanged, 0));
    }
  return MALS_OK;
}

// ... and the event they wait for: everything the comm streams hold now (the chunks of an exchange) is in
int mark_exchanged(mals_group g) {
  return for_members(g, [&](Member& mb) -> int {
    GHIP(g, hipEventRecord(mb.ev_exchanged, mb.comm));
    return MALS_OK;
  });
}

// The freshly solved rows of chunk c of every slice into every replica (comm streams).
int exchange_chunk(mals_group g, int side, int c) {
  const int k = g->cfg.features;
  if (g->world == 1) return MALS_OK;
  if (g->backend == MALS_GROUP_PEER_COPY)
    return for_members(g, [&](Member& src) -> int {
      int64_t lo, hi;
      chunk_range(g, side, src.rank, c, &lo, &hi);
      for (Member& dst : g->m)
        if (dst.rank != src.rank && hi > lo)
          GHIP(g, hipMemcpyPeerAsync(dst.F[side] + lo * k, dst.device, src.F[side] + lo * k, src.device, sizeof(float) * (size_t)(hi - lo) * k,
                                     src.comm));
      return MALS_OK;
    });
  return rccl_group(g, "ncclSend/ncclRecv", [&](Member& mb, size_t) {
    int64_t lo, hi;
    chunk_range(g, side, mb.rank, c, &lo, &hi);
    ncclResult_t r = ncclSuccess;
    for (int q = 0; q < g->world && r == ncclSuccess; ++q) {
      if (q == mb.rank) continue;
      if (hi > lo) r = g_rccl.Send(mb.F[side] + lo * k, (size_t)(hi - lo) * k, ncclFloat, q, mb.nccl, mb.comm);
      int64_t qlo, qhi;
      chunk_range(g, side, q, c, &qlo, &qhi);
      if (r == ncclSuccess && qhi > qlo) r = g_rccl.Recv(mb.F[side] + qlo * k, (size_t)(qhi - qlo) * k, ncclFloat, q, mb.nccl, mb.comm);
    }
    return r;
  });
}

// The first LOCAL failure of a half-iteration (MALS_OOM, MALS_INVALID_ARG ... of one member) and its text.  Such a failure
// never leaves a rank between two collectives: the member contributes zeros or skips its solves, every rank's calls stay
// matched, and the status is agreed at the end of the half-iteration.
struct LocalFailure {
  int rc = MALS_OK;
  std::string msg;
  void note(const Member& mb, int code) {
    if (rc != MALS_OK) return;
    rc = code;
    msg = std::string("rank ") + std::to_string(mb.rank) + ": " + mals_last_error(mb.h);
  }
};

// G = sum over ranks of the partial Gramians of `side`'s replica, installed on every member.  Every
// replica is complete when this runs (the caller has waited for the exchange), so the rows -- stale Y rows
// behind the matrix included (ALS:304-308) -- are simply cut into `world` equal ranges: the work of M^T M
// is proportional to rows, not to entries.
// A LOCAL failure of a member's partial Gramian or of installing the sum goes to `local` (the member contributes zeros); the
// return value is for failures that end the half-iteration on the spot (communication, device).
int group_gramian(mals_group g, int side, LocalFailure& local) {
  const size_t kk = (size_t)g->cfg.features * g->cfg.features, ns = (size_t)malsi_ymax_slots();
  const int64_t per = (g->n_total[side] + g->world - 1) / g->world;
  std::vector<void*> gp, ymax;
  if (int rc = for_members(g, [&](Member& mb) -> int {
        const int64_t r0 = std::min(g->n_total[side], per * mb.rank);
        const int64_t r1 = std::min(g->n_total[side], per * (mb.rank + 1));
        // the kernels that form the partial Gramian also record the largest |element| of their rows: summed Gramian + the
        // maximum over all ranks give every member the exact operand bound of the split-precision gather (instead of
        // sqrt(max_f G_ff), which at 1e8 rows is 13 binades loose)
        GHIP(g, hipMemsetAsync(mb.d_ymax.get(), 0, sizeof(float) * ns, mb.compute));
        int prc = MALS_OK;
        if (r1 > r0) {
          prc = malsi_gramian_partial(mb.h, side, r0, r1 - r0, mb.d_gp.get(), reinterpret_cast<unsigned*>(mb.d_ymax.get()));
          if (prc == MALS_HIP_ERROR) return mfail(g, mb, prc);
          if (prc != MALS_OK) local.note(mb, prc);
        }
        if (r1 <= r0 || prc != MALS_OK) GHIP(g, hipMemsetAsync(mb.d_gp.get(), 0, sizeof(double) * kk, mb.compute));
        gp.push_back(mb.d_gp.get());
        ymax.push_back(mb.d_ymax.get());
        return MALS_OK;
      }))
    return rc;
  if (int rc = all_reduce(g, {Reduce{gp.data(), kk, ncclDouble, ncclSum}, Reduce{ymax.data(), ns, ncclFloat, ncclMax}}, Done::COMPUTE_FOLLOWS))
    return rc;
  return for_members(g, [&](Member& mb) -> int {
    if (int rc = malsi_set_gramian(mb.h, side, mb.d_gp.get(), MALS_MEM_DEVICE, reinterpret_cast<const unsigned*>(mb.d_ymax.get()))) {
      if (rc == MALS_HIP_ERROR) return mfail(g, mb, rc);
      local.note(mb, rc);
    }
    return MALS_OK;
  });
}

// "This member's n elements at src on device src_dev": src itself when it lives on the member's device and no copy is forced,
// else a copy in `own`, enqueued on the member's compute stream (*copied: the caller waits for that stream before the use).
template <class T>
int member_slice(mals_group g, Member& mb, const T* src, int src_dev, bool force_copy, int64_t n, mals::DeviceBuffer<T>& own, const T** out,
                 bool* copied) {
  *out = src;
  if (n <= 0 || (mb.device == src_dev && !force_copy)) return MALS_OK;
  GHIP(g, own.alloc((size_t)n));
  GHIP(g, hipMemcpyPeerAsync(own.get(), mb.device, src, src_dev, sizeof(T) * (size_t)n, mb.compute));
  *out = own.get();
  *copied = true;
  return MALS_OK;
}

// a slice's rebased row pointers on the member's device
int upload_row_ptr(mals_group g, mals::DeviceBuffer<int64_t>& dst, const std::vector<int64_t>& local) {
  GHIP(g, dst.alloc(local.size()));
  GHIP(g, hipMemcpy(dst.get(), local.data(), sizeof(int64_t) * local.size(), hipMemcpyHostToDevice));
  return MALS_OK;
}

// what both create calls do when one of their steps failed
int create_failed(mals_group g, const char* call, int rc) {
  std::fprintf(stderr, "%s: %s\n", call, g->err.c_str());
  malsi_set_create_error((std::string(call) + ": " + g->err).c_str());
  for (Member& mb : g->m) destroy_member(mb);
  delete g;
  (void)hipGetLastError();   // a failed create leaves no sticky error behind for the next group of this process
  return rc;
}

}  // namespace

// =================================================================================================
extern "C" {

int mals_plan_shards(const int64_t* row_ptr, int64_t n_rows, int32_t world, double row_cost, int32_t features, int64_t* bounds_out) {
  return mals::plan_shards(row_ptr, n_rows, world, row_cost, features, bounds_out) ? MALS_OK : MALS_INVALID_ARG;
}

int mals_group_create(const mals_config* cfg, const int32_t* devices, int32_t n_devices, int32_t backend, mals_group* out) {
  if (!cfg || !devices || !out || n_devices <= 0) {
    malsi_set_create_error("mals_group_create: null argument or empty device list");
    return MALS_INVALID_ARG;
  }
  *out = nullptr;
  if (backend != MALS_GROUP_RCCL && backend != MALS_GROUP_PEER_COPY) {
    malsi_set_create_error("mals_group_create: backend must be MALS_GROUP_RCCL or MALS_GROUP_PEER_COPY");
    return MALS_INVALID_ARG;
  }
  mals_group g = new (std::nothrow) mals_group_s();
  if (!g) {
    malsi_set_create_error("mals_group_create: out of host memory");
    return MALS_OOM;
  }
  g->cfg = *cfg;
  g->world = n_devices;
  g->backend = backend;
  g->single_process = true;
  g->m.resize((size_t)n_devices);
  int rc = MALS_OK;
  for (int i = 0; i < n_devices && rc == MALS_OK; ++i) rc = init_member(g, g->m[(size_t)i], *cfg, devices[i], i);
  if (rc == MALS_OK && backend == MALS_GROUP_RCCL && n_devices > 1) {
    std::string e;
    if (!g_rccl.load(e)) {
      rc = gfail(g, MALS_COMM_ERROR, e);
    } else {
      std::vector<ncclComm_t> comms((size_t)n_devices);
      std::vector<int> devs(devices, devices + n_devices);
      const ncclResult_t r = g_rccl.CommInitAll(comms.data(), n_devices, devs.data());
      if (r != ncclSuccess) {
        rc = gfail(g, MALS_COMM_ERROR, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r));
      } else {
        for (int i = 0; i < n_devices; ++i) g->m[(size_t)i].nccl = comms[(size_t)i];
      }
    }
  }
  if (rc == MALS_OK && backend == MALS_GROUP_PEER_COPY) {
    for (Member& a : g->m)
      for (Member& b : g->m) {
        if (a.device == b.device) continue;
        (void)hipSetDevice(a.device);
        const hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();  // copies then stage through the host
      }
  }
  if (rc != MALS_OK) return create_failed(g, "mals_group_create", rc);
  malsi_set_create_error("");
  *out = g;
  return MALS_OK;
}

int mals_group_unique_id(void* id_out_128_bytes) {
  if (!id_out_128_bytes) return MALS_INVALID_ARG;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  std::string e;
  if (!g_rccl.load(e)) {
    malsi_set_create_error(("mals_group_unique_id: " + e).c_str());
    return MALS_COMM_ERROR;
  }
  ncclUniqueId id;
  if (g_rccl.GetUniqueId(&id) != ncclSuccess) {
    malsi_set_create_error("mals_group_unique_id: ncclGetUniqueId failed");
    return MALS_COMM_ERROR;
  }
  std::memcpy(id_out_128_bytes, &id, sizeof(id));
  return MALS_OK;
}

int mals_group_create_rank(const mals_config* cfg, int32_t world, int32_t rank, const void* id_128_bytes, mals_group* out) {
  if (!cfg || !out || world <= 0 || rank < 0 || rank >= world || (world > 1 && !id_128_bytes)) {
    malsi_set_create_error("mals_group_create_rank: null argument, rank outside 0..world-1, or no unique id for world > 1");
    return MALS_INVALID_ARG;
  }
  *out = nullptr;
  mals_group g = new (std::nothrow) mals_group_s();
  if (!g) {
    malsi_set_create_error("mals_group_create_rank: out of host memory");
    return MALS_OOM;
  }
  g->cfg = *cfg;
  g->world = world;
  g->backend = MALS_GROUP_RCCL;
  g->single_process = world == 1;
  g->m.resize(1);
  int rc = init_member(g, g->m[0], *cfg, cfg->device, rank);
  if (rc == MALS_OK && id_128_bytes) {  // also for world = 1 when an id is given: a real one-rank communicator
    std::string e;
    if (!g_rccl.load(e)) {
      rc = gfail(g, MALS_COMM_ERROR, e);
    } else {
      ncclUniqueId id;
      std::memcpy(&id, id_128_bytes, sizeof(id));
      (void)hipSetDevice(cfg->device);
      const ncclResult_t r = g_rccl.CommInitRank(&g->m[0].nccl, world, id, rank);
      if (r != ncclSuccess) rc = gfail(g, MALS_COMM_ERROR, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
    }
  }
  if (rc != MALS_OK) return create_failed(g, "mals_group_create_rank", rc);
  malsi_set_create_error("");
  *out = g;
  return MALS_OK;
}

int mals_group_destroy(mals_group g) {
  if (!g) return MALS_INVALID_ARG;
  for (Member& mb : g->m) destroy_member(mb);
  delete g;
  return MALS_OK;
}

int mals_group_set_alternate_streams(mals_group g, int32_t on) {
  if (!g) return MALS_INVALID_ARG;
  g->alternate_streams = on != 0;
  return MALS_OK;
}

int mals_group_set_iteration_callback(mals_group g, mals_iteration_fn fn, void* user) {
  if (!g) return MALS_INVALID_ARG;
  g->iter_fn = fn;
  g->iter_user = user;
  return MALS_OK;
}

const char* mals_group_last_error(mals_group g) { return g ? g->err.c_str() : "null group"; }

int mals_group_world(mals_group g) { return g ? g->world : 0; }

int mals_group_features(mals_group g) { return g ? g->cfg.features : 0; }

int mals_group_pending_entries(mals_group g, int side, int64_t n_rows, int64_t* n_entries_out) {
  GSIDE(g, side);
  const std::vector<int64_t>& rp = g->up_row_ptr[side];
  if (rp.empty() || !n_entries_out) return gfail(g, MALS_INVALID_ARG, "no chunked upload in progress");
  const int64_t a = g->up_next_row[side], b = a + n_rows;
  if (n_rows < 0 || b > g->n_rows[side]) return gfail(g, MALS_INVALID_ARG, "piece exceeds the declared matrix");
  *n_entries_out = rp[(size_t)b] - rp[(size_t)a];
  return MALS_OK;
}

int mals_group_local(mals_group g, int32_t i, mals_handle* handle_out, int32_t* rank_out) {
  if (!g) return MALS_INVALID_ARG;
  if (i < 0 || (size_t)i >= g->m.size()) return gfail(g, MALS_INVALID_ARG, "no such local member");
  if (handle_out) *handle_out = g->m[(size_t)i].h;
  if (rank_out) *rank_out = g->m[(size_t)i].rank;
  return MALS_OK;
}

int mals_group_set_exchange_chunks(mals_group g, int32_t n_chunks) {
  if (!g || n_chunks <= 0) return MALS_INVALID_ARG;
  // takes effect with the next matrix upload of each side: a side that already holds a matrix keeps the count its
  // members' work lists were built for (side_chunks), so a later call can never leave part of a slice unsolved
  g->exchange_chunks = n_chunks;
  return MALS_OK;
}

int mals_group_use_transport(const char* library_path) {
  if (g_rccl.lib) return MALS_INVALID_ARG;  // already loaded: the choice is made once per process, before the first group
  g_rccl.forced = library_path ? library_path : "";
  return MALS_OK;
}

int mals_group_comm_info(mals_group g, int32_t local_member, int32_t* comm_size, int32_t* comm_rank, int32_t* hip_device,
                         char* pci_bus_id, int32_t pci_len) {
  if (!g) return MALS_INVALID_ARG;
  if (local_member < 0 || (size_t)local_member >= g->m.size()) return gfail(g, MALS_INVALID_ARG, "no such local member");
  const Member& mb = g->m[(size_t)local_member];
  int n = 0, r = -1, dev = mb.device;
  if (mb.nccl) {  // read back from the communicator itself, not from what this library was told
    GNCCL(g, g_rccl.CommCount(mb.nccl, &n));
    GNCCL(g, g_rccl.CommUserRank(mb.nccl, &r));
    GNCCL(g, g_rccl.CommCuDevice(mb.nccl, &dev));
  }
  if (comm_size) *comm_size = n;
  if (comm_rank) *comm_rank = r;
  if (hip_device) *hip_device = dev;
  if (pci_bus_id && pci_len > 0) {
    pci_bus_id[0] = 0;
    if (hipDeviceGetPCIBusId(pci_bus_id, pci_len, mb.device) != hipSuccess) {
      (void)hipGetLastError();
      pci_bus_id[0] = 0;
    }
  }
  return MALS_OK;
}

int mals_group_set_refine_limit(mals_group g, double limit) {
  if (!g) return MALS_INVALID_ARG;
  for (Member& mb : g->m)
    if (int rc = mals_set_refine_limit(mb.h, limit)) return mfail(g, mb, rc);
  return MALS_OK;
}

int mals_group_set_factor_rows(mals_group g, int side, int64_t n_rows_total) {
  GSIDE(g, side);
  for (Member& mb : g->m)
    if (int rc = mals_set_factor_rows(mb.h, side, n_rows_total)) return mfail(g, mb, rc);
  g->n_total[side] = n_rows_total;
  if (side == MALS_SIDE_X) g->users_end.store(n_rows_total, std::memory_order_release);
  return refresh_replica_ptrs(g, side);
}

int mals_group_set_factors(mals_group g, int side, int64_t row_begin, int64_t n_rows, const float* host_rows) {
  GSIDE(g, side);
  for (Member& mb : g->m)
    if (int rc = mals_set_factors(mb.h, side, row_begin, n_rows, host_rows)) return mfail(g, mb, rc);
  return MALS_OK;
}

int mals_group_get_factors(mals_group g, int side, int64_t row_begin, int64_t n_rows, float* host_out) {
  GSIDE(g, side);
  if (int rc = mals_group_synchronize(g)) return rc;  // rows other ranks solved arrive on the comm streams
  Member& mb = g->m[0];
  if (int rc = mals_get_factors(mb.h, side, row_begin, n_rows, host_out)) return mfail(g, mb, rc);
  return MALS_OK;
}

int mals_group_get_rows(mals_group g, int side, const int64_t* row_idx, int32_t n, float* host_out) {
  GSIDE(g, side);
  if (int rc = mals_group_synchronize(g)) return rc;
  Member& mb = g->m[0];
  if (int rc = mals_get_rows(mb.h, side, row_idx, n, host_out)) return mfail(g, mb, rc);
  return MALS_OK;
}

int mals_group_set_matrix(mals_group g, int side, int64_t n_rows, int64_t nnz, const int64_t* row_ptr, const int32_t* col_idx,
                          const float* val, int mem_kind) {
  GSIDE(g, side);
  if (n_rows < 0 || nnz < 0 || !row_ptr || (nnz > 0 && (!col_idx || !val))) return gfail(g, MALS_INVALID_ARG, "bad matrix arguments");
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return gfail(g, MALS_INVALID_ARG, "mem_kind must be MALS_MEM_HOST or MALS_MEM_DEVICE");
  std::vector<int64_t> rp_host;
  const int64_t* rp = row_ptr;
  if (mem_kind == MALS_MEM_DEVICE) {
    rp_host.resize((size_t)n_rows + 1);
    GHIP(g, hipMemcpy(rp_host.data(), row_ptr, sizeof(int64_t) * (size_t)(n_rows + 1), hipMemcpyDeviceToHost));
    rp = rp_host.data();
  }
  if (rp[0] != 0 || rp[n_rows] != nnz) return gfail(g, MALS_INVALID_ARG, "row_ptr must start at 0 and end at nnz");
  if (int rc = plan_side(g, side, rp, n_rows)) return rc;
  if (int rc = for_members(g, [&](Member& mb) -> int {
        const mals::CsrSlice s = mals::csr_slice(rp, g->bounds[side][(size_t)mb.rank], g->bounds[side][(size_t)mb.rank + 1]);
        const int64_t* local = s.local.data();
        if (mem_kind == MALS_MEM_DEVICE) {
          if (int rc = upload_row_ptr(g, mb.d_row_ptr[side], s.local)) return rc;
          local = mb.d_row_ptr[side].get();
        }
        if (int rc = mals_set_matrix(mb.h, side, s.r0, s.rows(), s.entries(), local, col_idx + s.e0, val + s.e0, mem_kind)) return mfail(g, mb, rc);
        // (slices an earlier mals_ingest_install_group copied for this member are not this matrix: they go now that the handle
        // has taken the new arrays -- mals_set_matrix synchronises the member's stream before it drops the old ones)
        mb.own_col[side].reset();
        mb.own_val[side].reset();
        return MALS_OK;
      }))
    return rc;
  return sync_value_stats(g, side);
}

// InputFilesReader.readInputFiles -> DelegateGenerationManager.java:406-410, for a group: see include/myrrix_als.h
int mals_ingest_install_group(mals_ingest in, mals_group g, int32_t flags) {
  if (!g) return MALS_INVALID_ARG;
  if (!in) return gfail(g, MALS_INVALID_ARG, "null ingest handle");
  if (malsi_ingest_spent(in)) return gfail(g, MALS_INVALID_ARG, "the ingest holds one member's slices (mals_group_ingest_finish), not the whole input");
  int64_t n_rows[2] = {0, 0}, nnz = 0;
  if (int rc = mals_ingest_counts(in, nullptr, &n_rows[0], &n_rows[1], &nnz)) return gfail(g, rc, mals_ingest_last_error(in));
  int32_t in_dev = 0;
  if (int rc = mals_ingest_device(in, &in_dev)) return gfail(g, rc, "mals_ingest_device failed");
  if (flags & ~MALS_INSTALL_COPY) return gfail(g, MALS_INVALID_ARG, "unknown install flag");
  const bool force_copy = (flags & MALS_INSTALL_COPY) != 0;   // members on the ingest's own device copy too: the ingest may go
  // replicas first: validate_columns of the matrix upload checks the column indices against the opposite replica
  for (int sd = 0; sd < 2; ++sd)
    if (g->n_total[sd] < n_rows[sd])
      if (int rc = mals_group_set_factor_rows(g, sd, n_rows[sd])) return rc;
  for (int sd = 0; sd < 2; ++sd) {
    const int64_t* d_ptr = nullptr;
    const int32_t* d_col = nullptr;
    const float* d_val = nullptr;
    if (int rc = mals_ingest_device_csr(in, sd, &d_ptr, &d_col, &d_val)) return gfail(g, rc, mals_ingest_last_error(in));
    // the row pointers cross to the host once (8 bytes per row): the plan is made there, like for every other upload
    std::vector<int64_t> rp((size_t)n_rows[sd] + 1);
    GHIP(g, hipSetDevice(in_dev));
    GHIP(g, hipMemcpy(rp.data(), d_ptr, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost));
    if (rp[0] != 0 || rp[(size_t)n_rows[sd]] != nnz) return gfail(g, MALS_INVALID_ARG, "the ingest's row pointers do not match its entry count");
    if (int rc = plan_side(g, sd, rp.data(), n_rows[sd])) return rc;
    if (int rc = for_members(g, [&](Member& mb) -> int {
          const mals::CsrSlice s = mals::csr_slice(rp.data(), g->bounds[sd][(size_t)mb.rank], g->bounds[sd][(size_t)mb.rank + 1]);
          mb.own_col[sd].reset();
          mb.own_val[sd].reset();
          if (int rc = upload_row_ptr(g, mb.d_row_ptr[sd], s.local)) return rc;
          const int32_t* col = nullptr;
          const float* val = nullptr;
          bool copied = false;
          if (int rc = member_slice(g, mb, d_col + s.e0, in_dev, force_copy, s.entries(), mb.own_col[sd], &col, &copied)) return rc;
          if (int rc = member_slice(g, mb, d_val + s.e0, in_dev, force_copy, s.entries(), mb.own_val[sd], &val, &copied)) return rc;
          if (copied) GHIP(g, hipStreamSynchronize(mb.compute));
          if (int rc = mals_set_matrix(mb.h, sd, s.r0, s.rows(), s.entries(), mb.d_row_ptr[sd].get(), col, val, MALS_MEM_DEVICE)) return mfail(g, mb, rc);
          return MALS_OK;
        }))
      return rc;
    if (int rc = sync_value_stats(g, sd)) return rc;
  }
  // knownItemIDs: every member the rows of its own users (mals_recommend by user index is answered by the member that
  // holds the user's row); userTagIDs: every member the whole mask
  const int64_t *k_ptr = nullptr, *t_idx = nullptr;
  const int32_t* k_idx = nullptr;
  int64_t n_known = 0, n_tags = 0;
  (void)mals_ingest_device_known_items(in, &k_ptr, &k_idx, &n_known);   // fails when the ingest did not build them: k_ptr stays null
  if (int rc = mals_ingest_device_tag_items(in, &t_idx, &n_tags)) return gfail(g, rc, mals_ingest_last_error(in));
  std::vector<int64_t> kp;
  if (k_ptr) {
    kp.resize((size_t)n_rows[0] + 1);
    GHIP(g, hipSetDevice(in_dev));
    GHIP(g, hipMemcpy(kp.data(), k_ptr, sizeof(int64_t) * kp.size(), hipMemcpyDeviceToHost));
  }
  return for_members(g, [&](Member& mb) -> int {
    mb.own_known_ptr.reset();
    mb.own_known_idx.reset();
    mb.own_tag_idx.reset();
    if (k_ptr) {
      const mals::CsrSlice s = mals::csr_slice(kp.data(), g->bounds[0][(size_t)mb.rank], g->bounds[0][(size_t)mb.rank + 1]);
      if (int rc = upload_row_ptr(g, mb.own_known_ptr, s.local)) return rc;
      const int32_t* idx = nullptr;
      bool copied = false;
      if (int rc = member_slice(g, mb, k_idx + s.e0, in_dev, force_copy, s.entries(), mb.own_known_idx, &idx, &copied)) return rc;
      if (copied) GHIP(g, hipStreamSynchronize(mb.compute));
      if (int rc = mals_set_known_items(mb.h, s.rows(), mb.own_known_ptr.get(), idx, MALS_MEM_DEVICE)) return mfail(g, mb, rc);
    }
    const int64_t* tags = nullptr;
    bool copied = false;
    if (int rc = member_slice(g, mb, t_idx, in_dev, force_copy, n_tags, mb.own_tag_idx, &tags, &copied)) return rc;
    if (copied) GHIP(g, hipStreamSynchronize(mb.compute));
    if (int rc = mals_set_tag_items(mb.h, n_tags, tags, MALS_MEM_DEVICE)) return mfail(g, mb, rc);
    return MALS_OK;
  });
}

}  // extern "C"

// ---- mals_group_ingest_finish: the group's transport for the ingest side (ingest_group_host.h) ----
namespace {

const char* shard_ops_error(void* ctx) { return static_cast<mals_group>(ctx)->err.c_str(); }

int shard_ops_allreduce(void* ctx, int64_t* const* dev, int64_t n, int op_max) {
  const std::vector<void*> d(dev, dev + static_cast<mals_group>(ctx)->m.size());
  return all_reduce(static_cast<mals_group>(ctx), {Reduce{d.data(), (size_t)n, ncclInt64, op_max ? ncclMax : ncclSum}}, Done::HOST_WAITS);
}

// every member's run for rank q (send_off row of the member) into q's receive buffer at q's offset for the sender
int shard_ops_exchange(void* ctx, const uint8_t* const* send, const int64_t* send_off, uint8_t* const* recv, const int64_t* recv_off) {
  mals_group g = static_cast<mals_group>(ctx);
  const int W = g->world;
  const size_t nl = g->m.size();
  if (g->backend == MALS_GROUP_PEER_COPY || (W == 1 && !g->m[0].nccl)) {
    for (size_t i = 0; i < nl; ++i) {
      const Member& src = g->m[i];
      GHIP(g, hipSetDevice(src.device));
      for (size_t j = 0; j < nl; ++j) {
        const Member& dst = g->m[j];
        const int64_t b = send_off[i * (W + 1) + dst.rank], e = send_off[i * (W + 1) + dst.rank + 1];
        if (e > b)
          GHIP(g, hipMemcpyPeerAsync(recv[j] + recv_off[j * (W + 1) + src.rank], dst.device, send[i] + b, src.device, (size_t)(e - b), src.comm));
      }
    }
    return sync_comm(g);
  }
  const int rc = rccl_group(g, "ncclSend/ncclRecv", [&](Member& mb, size_t i) {
    ncclResult_t r = ncclSuccess;
    for (int q = 0; q < W && r == ncclSuccess; ++q) {
      const int64_t sb = send_off[i * (W + 1) + q], se = send_off[i * (W + 1) + q + 1];
      const int64_t rb = recv_off[i * (W + 1) + q], re = recv_off[i * (W + 1) + q + 1];
      if (q == mb.rank) {
        if (se > sb && hipSetDevice(mb.device) == hipSuccess &&
            hipMemcpyAsync(recv[i] + rb, send[i] + sb, (size_t)(se - sb), hipMemcpyDeviceToDevice, mb.comm) != hipSuccess)
          r = ncclUnhandledCudaError;
      } else {
        if (se > sb) r = g_rccl.Send(send[i] + sb, (size_t)(se - sb), ncclUint8, q, mb.nccl, mb.comm);
        if (r == ncclSuccess && re > rb) r = g_rccl.Recv(recv[i] + rb, (size_t)(re - rb), ncclUint8, q, mb.nccl, mb.comm);
      }
    }
    return r;
  });
  return rc != MALS_OK ? rc : sync_comm(g);
}

int shard_ops_agree(void* ctx, const int* local_rc) {
  mals_group g = static_cast<mals_group>(ctx);
  int worst = MALS_OK;
  for (size_t i = 0; i < g->m.size(); ++i) worst = std::max(worst, local_rc[i]);
  if (g->single_process) return worst;
  // multi-process: the group's status words (allocated with the group), max over every rank
  std::vector<std::vector<double>> v(g->m.size(), std::vector<double>(1, 0.0));
  for (size_t i = 0; i < g->m.size(); ++i) v[i][0] = (double)local_rc[i];
  double agreed = 0.0;
  if (int rc = allreduce_host(g, v, 1, 1, &agreed)) return rc == MALS_COMM_ERROR ? MALS_COMM_ERROR : -1;
  return (int)agreed;
}

}  // namespace

extern "C" {

int mals_group_ingest_finish(mals_group g, mals_ingest* ingests, int32_t n_local, int32_t flags) {
  if (!g) return MALS_INVALID_ARG;
  if (!ingests || n_local != (int32_t)g->m.size()) return gfail(g, MALS_INVALID_ARG, "one ingest per local member");
  if (flags != 0) return gfail(g, MALS_INVALID_ARG, "flags: reserved, must be 0");
  for (int32_t i = 0; i < n_local; ++i) {
    int32_t dev = -1;
    if (!ingests[i] || mals_ingest_device(ingests[i], &dev) != MALS_OK) return gfail(g, MALS_INVALID_ARG, "null ingest handle");
    if (dev != g->m[(size_t)i].device) return gfail(g, MALS_INVALID_ARG, "ingest " + std::to_string(i) + " is not on its member's device");
  }
  std::vector<int32_t> ranks((size_t)n_local);
  for (int32_t i = 0; i < n_local; ++i) ranks[(size_t)i] = g->m[(size_t)i].rank;
  malsi_group_ops ops{g, g->world, n_local, g->cfg.features, ranks.data(), shard_ops_allreduce, shard_ops_exchange, shard_ops_agree, shard_ops_error};
  std::vector<int64_t> bounds[2] = {std::vector<int64_t>((size_t)g->world + 1, 0), std::vector<int64_t>((size_t)g->world + 1, 0)};
  if (int rc = malsi_ingest_shard_finish(ingests, &ops, bounds[0].data(), bounds[1].data())) return gfail(g, rc, mals_ingest_last_error(ingests[0]));
  // the ingests hold their slices only: records, workspace and exchange buffers are gone before the replicas are declared
  int64_t n_rows[2] = {0, 0};
  if (int rc = mals_ingest_counts(ingests[0], nullptr, &n_rows[0], &n_rows[1], nullptr)) return gfail(g, rc, mals_ingest_last_error(ingests[0]));
  for (int32_t i = 0; i < n_local; ++i) malsi_ingest_note_replicas(ingests[i]);
  for (int sd = 0; sd < 2; ++sd)
    if (g->n_total[sd] < n_rows[sd])
      if (int rc = mals_group_set_factor_rows(g, sd, n_rows[sd])) return rc;
  for (int sd = 0; sd < 2; ++sd) {
    if (int rc = set_side_bounds(g, sd, bounds[sd])) return rc;
    for (int32_t i = 0; i < n_local; ++i) {
      Member& mb = g->m[(size_t)i];
      const int64_t *d_ptr = nullptr;
      const int32_t* d_col = nullptr;
      const float* d_val = nullptr;
      if (int rc = mals_ingest_device_csr(ingests[i], sd, &d_ptr, &d_col, &d_val)) return gfail(g, rc, mals_ingest_last_error(ingests[i]));
      const int64_t r0 = bounds[sd][(size_t)mb.rank], r1 = bounds[sd][(size_t)mb.rank + 1];
      int64_t nnz = 0;
      GHIP(g, hipSetDevice(mb.device));
      GHIP(g, hipMemcpy(&nnz, d_ptr + (r1 - r0), sizeof(int64_t), hipMemcpyDeviceToHost));
      mb.own_col[sd].reset();
      mb.own_val[sd].reset();
      if (int rc = mals_set_matrix(mb.h, sd, r0, r1 - r0, nnz, d_ptr, d_col, d_val, MALS_MEM_DEVICE)) return mfail(g, mb, rc);
    }
    if (int rc = sync_value_stats(g, sd)) return rc;
  }
  for (int32_t i = 0; i < n_local; ++i) {
    Member& mb = g->m[(size_t)i];
    GHIP(g, hipSetDevice(mb.device));
    mb.own_known_ptr.reset();
    mb.own_known_idx.reset();
    mb.own_tag_idx.reset();
    const int64_t *k_ptr = nullptr, *t_idx = nullptr;
    const int32_t* k_idx = nullptr;
    int64_t n_known = 0, n_tags = 0;
    (void)mals_ingest_device_known_items(ingests[i], &k_ptr, &k_idx, &n_known);
    if (k_ptr)
      if (int rc = mals_set_known_items(mb.h, bounds[0][(size_t)mb.rank + 1] - bounds[0][(size_t)mb.rank], k_ptr, k_idx, MALS_MEM_DEVICE)) return mfail(g, mb, rc);
    if (int rc = mals_ingest_device_tag_items(ingests[i], &t_idx, &n_tags)) return gfail(g, rc, mals_ingest_last_error(ingests[i]));
    if (int rc = mals_set_tag_items(mb.h, n_tags, t_idx, MALS_MEM_DEVICE)) return mfail(g, mb, rc);
  }
  return MALS_OK;
}

}  // extern "C"

namespace {

// mals_group_factorize's side of the loop in convergence.h: a cancellation is local knowledge and agreed on before a collective
// is entered; the report counts what THIS process's members solved and gathered, from their stats before, between and after
// the halves
struct GroupFactorize {
  mals_group g;
  int64_t rows[2] = {0, 0}, entries0 = 0;   // rows solved up to: the iteration's start, the end of its X half
  void totals(int64_t* rows_out, int64_t* entries_out) {
    *rows_out = *entries_out = 0;
    for (Member& mb : g->m) {
      mals_stats st;
      (void)mals_get_stats(mb.h, &st);
      *rows_out += st.rows_solved;
      *entries_out += st.nnz_gathered;
    }
  }
  int fail(int code, const char* msg) { return gfail(g, code, msg); }
  void clear_cancel() { g->cancelled.store(0); }
  int cancelled() { return agree_status(g, g->cancelled.load() ? MALS_CANCELLED : MALS_OK, "cancelled"); }
  int half_iteration(int side) { return mals_group_half_iteration(g, side); }
  // from one complete replica: every replica holds the same factors once the exchange is in
  int sample_dots(const int64_t* users, int32_t n_users, const int64_t* items, int32_t n_items, double* out) {
    if (int rc = mals_group_synchronize(g)) return rc;
    if (int rc = mals_sample_dots(g->m[0].h, users, n_users, items, n_items, out)) return mfail(g, g->m[0], rc);
    return MALS_OK;
  }
  mals_iteration_fn callback(void** user) {
    *user = g->iter_user;
    return g->iter_fn;
  }
  void count(int point) {
    int64_t e = 0;
    totals(&rows[point], point == 0 ? &entries0 : &e);
  }
  void report(mals_iteration_info* info) {
    int64_t rows_now = 0, entries_now = 0;
    totals(&rows_now, &entries_now);
    info->entries_gathered = entries_now - entries0;
    info->x_rows = rows[1] - rows[0];
    info->y_rows = rows_now - rows[0] - info->x_rows;
    info->algorithmic_bytes = (double)(info->entries_gathered + rows_now - rows[0]) * (4.0 * g->cfg.features + 8.0);
    info->devices = (int32_t)g->m.size();
  }
};

// Every member holds full replicas of X and Y but only its own users' rows of R / knownItemIDs, so a user is answered by the
// member whose slice holds its row: runs of consecutive queries with one owner go to that member in one call,
// call(handle, q0, n).  any_member: the replicas alone answer, so a run whose owner is another process's rank goes to member 0.
// (No message on a refusal: request threads share the group's error string.)
template <class Call>
int route_by_owner(mals_group g, const int64_t* user_idx, int32_t n_queries, bool any_member, Call&& call) {
  for (;;) {
    // a load of a new generation (mals_group_load_generation) moves users between members: what was routed by the old bounds
    // and answered after the swap is asked again
    const uint64_t seq = g->generation_seq.load(std::memory_order_acquire);
    if (seq & 1) {
      std::this_thread::yield();
      continue;
    }
    int rc = MALS_OK;
    const std::vector<int64_t>& b = g->bounds[MALS_SIDE_X];
    if (b.empty()) rc = MALS_INVALID_ARG;
    for (int32_t q0 = 0, q1 = 0; rc == MALS_OK && q0 < n_queries; q0 = q1) {
      int owner = 0;
      if (!mals::owner_run(b, g->users_end.load(std::memory_order_acquire), user_idx, n_queries, q0, &q1, &owner)) {
        rc = MALS_INVALID_ARG;
        break;
      }
      const Member* mb = any_member ? &g->m[0] : nullptr;
      for (const Member& m : g->m)
        if (m.rank == owner) mb = &m;
      if (!mb) rc = MALS_INVALID_ARG;   // the owner is another process's rank
      else rc = call(mb->h, q0, q1 - q0);
    }
    if (g->generation_seq.load(std::memory_order_acquire) == seq) return rc;
  }
}

}  // namespace

extern "C" {

// ServerRecommender.recommend(userID, ...) on a group.  consider_known_items: any member can answer (the replicas are
// complete); else only the owner knows the user's items
int mals_group_recommend(mals_group g, const int64_t* user_idx, int32_t n_queries, int32_t how_many, int32_t consider_known_items,
                         int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (!g) return MALS_INVALID_ARG;
  if (n_queries < 0 || how_many <= 0 || (n_queries > 0 && (!user_idx || !item_idx_out || !score_out))) return MALS_INVALID_ARG;
  return route_by_owner(g, user_idx, n_queries, consider_known_items != 0, [&](mals_handle h, int32_t q0, int32_t n) {
    return mals_recommend(h, user_idx + q0, n, how_many, consider_known_items, item_idx_out + (size_t)q0 * how_many,
                          score_out + (size_t)q0 * how_many, n_out ? n_out + q0 : nullptr);
  });
}

// mostSimilarItems / similarityToItem on a group: the Y replicas are complete on every member, any local member answers
int mals_group_most_similar_items(mals_group g, const int64_t* item_idx, const int64_t* item_ptr, int32_t n_queries, int32_t how_many,
                                  int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (!g || g->m.empty()) return MALS_INVALID_ARG;
  return mals_most_similar_items(g->m[0].h, item_idx, item_ptr, n_queries, how_many, item_idx_out, score_out, n_out);
}

int mals_group_similarity_to_item(mals_group g, int64_t to_item, const int64_t* item_idx, int32_t n, float* out) {
  if (!g || g->m.empty()) return MALS_INVALID_ARG;
  return mals_similarity_to_item(g->m[0].h, to_item, item_idx, n, out);
}

// recommendedBecause on a group: the user's known items live on the member whose slice holds its row
int mals_group_recommended_because(mals_group g, const int64_t* user_idx, const int64_t* item_idx, int32_t n_queries, int32_t how_many,
                                   int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (!g) return MALS_INVALID_ARG;
  if (n_queries < 0 || how_many <= 0 || (n_queries > 0 && (!user_idx || !item_idx || !item_idx_out || !score_out))) return MALS_INVALID_ARG;
  return route_by_owner(g, user_idx, n_queries, false, [&](mals_handle h, int32_t q0, int32_t n) {
    return mals_recommended_because(h, user_idx + q0, item_idx + q0, n, how_many, item_idx_out + (size_t)q0 * how_many,
                                    score_out + (size_t)q0 * how_many, n_out ? n_out + q0 : nullptr);
  });
}

int mals_group_begin_matrix(mals_group g, int side, int64_t n_rows, const int64_t* row_ptr) {
  GSIDE(g, side);
  if (n_rows < 0 || !row_ptr || row_ptr[0] != 0) return gfail(g, MALS_INVALID_ARG, "bad matrix arguments");
  g->up_row_ptr[side].assign(row_ptr, row_ptr + n_rows + 1);
  g->up_next_row[side] = 0;
  if (int rc = plan_side(g, side, row_ptr, n_rows)) return rc;
  for (Member& mb : g->m) {
    const int64_t r0 = g->bounds[side][(size_t)mb.rank], r1 = g->bounds[side][(size_t)mb.rank + 1];
    if (int rc = mals_begin_matrix(mb.h, side, r0, r1 - r0, row_ptr[r1] - row_ptr[r0])) return mfail(g, mb, rc);
    mb.up_rows = 0;
  }
  return MALS_OK;
}

int mals_group_append_rows(mals_group g, int side, int64_t n_rows, const int32_t* col_idx, const float* val) {
  GSIDE(g, side);
  const std::vector<int64_t>& rp = g->up_row_ptr[side];
  if (rp.empty()) return gfail(g, MALS_INVALID_ARG, "mals_group_append_rows without mals_group_begin_matrix");
  const int64_t a = g->up_next_row[side], b = a + n_rows;
  if (n_rows < 0 || b > g->n_rows[side]) return gfail(g, MALS_INVALID_ARG, "piece exceeds the declared matrix");
  const int64_t base = rp[(size_t)a];
  if (rp[(size_t)b] > base && (!col_idx || !val)) return gfail(g, MALS_INVALID_ARG, "null entry arrays");
  for (Member& mb : g->m) {  // the part of [a, b) inside this member's slice
    const int64_t r0 = std::max(a, g->bounds[side][(size_t)mb.rank]), r1 = std::min(b, g->bounds[side][(size_t)mb.rank + 1]);
    if (r1 <= r0) continue;
    const mals::CsrSlice s = mals::csr_slice(rp.data(), r0, r1);
    const int64_t off = s.e0 - base;
    if (int rc = mals_append_rows(mb.h, side, s.rows(), s.local.data(), col_idx ? col_idx + off : nullptr, val ? val + off : nullptr))
      return mfail(g, mb, rc);
  }
  g->up_next_row[side] = b;
  return MALS_OK;
}

int mals_group_end_matrix(mals_group g, int side) {
  GSIDE(g, side);
  if (g->up_row_ptr[side].empty()) return gfail(g, MALS_INVALID_ARG, "mals_group_end_matrix without mals_group_begin_matrix");
  const bool complete = g->up_next_row[side] == g->n_rows[side];
  g->up_row_ptr[side].clear();
  g->up_row_ptr[side].shrink_to_fit();
  if (!complete) return gfail(g, MALS_INVALID_ARG, "appended rows do not match the declared matrix size");
  for (Member& mb : g->m)
    if (int rc = mals_end_matrix(mb.h, side)) return mfail(g, mb, rc);
  return sync_value_stats(g, side);
}

int mals_group_bounds(mals_group g, int side, int64_t* bounds_out) {
  GSIDE(g, side);
  if (!bounds_out || g->bounds[side].empty()) return gfail(g, MALS_INVALID_ARG, "matrix of this side not set");
  std::memcpy(bounds_out, g->bounds[side].data(), sizeof(int64_t) * g->bounds[side].size());
  return MALS_OK;
}

int mals_group_half_iteration(mals_group g, int side) {
  GSIDE(g, side);
  if (g->bounds[side].empty()) return gfail(g, MALS_INVALID_ARG, "matrix of this side not set");
  if (!g->m[0].F[side] || !g->m[0].F[1 - side]) return gfail(g, MALS_INVALID_ARG, "factor replicas not allocated");
  // A failure of the local solve (MALS_OOM, MALS_INVALID_ARG ...) must not leave the peers alone in a collective:
  // the remaining exchanges of the half-iteration are still issued (only the solves are skipped), so that every rank
  // arrives at the agreed status with matching calls behind it.  Only a communication / device failure ends it here.
  LocalFailure local;
  auto run = [&]() -> int {
    if (int rc = await_exchange(g)) return rc;
    if (int rc = group_gramian(g, 1 - side, local)) return rc;  // ALS:342 / ALS:369
    const bool alternate = g->alternate_streams && g->side_chunks[side] > 1;
    if (alternate)   // the second stream starts behind everything the first has seen so far
      if (int rc = for_members(g, [&](Member& mb) { return hand_off(g, mb.compute, mb.ev_half, mb.compute2); })) return rc;
    for (int c = 0; c < g->side_chunks[side]; ++c) {
      const bool odd = alternate && (c & 1);
      if (alternate)
        if (int rc = for_members(g, [&](Member& mb) -> int {
              if (int rc = mals_set_stream(mb.h, odd ? mb.compute2 : mb.compute)) return mfail(g, mb, rc);
              // ... and behind what the half-iteration sets up once, in its first chunk (operand scale, images, rotated copy)
              if (c == 1) GHIP(g, hipStreamWaitEvent(mb.compute2, (hipEvent_t)malsi_ready_event(mb.h), 0));
              return MALS_OK;
            }))
          return rc;
      // Like the reference's pool, where every worker is started before any result is awaited (ALS:186-191,391-410):
      // the direct kernels of EVERY member are enqueued before any host work; the k x k eigendecomposition of the
      // dual path (the same G on every member after the all-reduce) is then computed once, under those kernels, and
      // handed to the others; only then the members' dual kernels follow.
      std::vector<char> has(g->m.size(), 0);
      if (int rc = for_members(g, [&](Member& mb, size_t i) -> int {
            int32_t mine = 0;
            if (int rc = mals_num_chunks(mb.h, side, &mine)) return mfail(g, mb, rc);
            has[i] = c < mine && local.rc == MALS_OK;
            if (has[i])
              if (int rc = malsi_solve_chunk_begin(mb.h, side, c)) {  // ALS:344 / ALS:371
                local.note(mb, rc);
                has[i] = 0;
              }
            return MALS_OK;
          }))
        return rc;
      Member* decomposed = nullptr;
      for (size_t i = 0; i < g->m.size(); ++i) {
        Member& mb = g->m[i];
        if (!has[i] || !malsi_dual_pending(mb.h)) continue;
        GHIP(g, hipSetDevice(mb.device));
        if (int rc = malsi_dual_host(mb.h, side, decomposed ? decomposed->h : nullptr)) {
          local.note(mb, rc);
          has[i] = 0;
          continue;
        }
        if (!decomposed) decomposed = &mb;
      }
      if (int rc = for_members(g, [&](Member& mb, size_t i) -> int {
            if (has[i])
              if (int rc = malsi_solve_chunk_end(mb.h, side, c)) local.note(mb, rc);
            return hand_off(g, odd ? mb.compute2 : mb.compute, mb.ev_solved, mb.comm);
          }))
        return rc;
      if (int rc = exchange_chunk(g, side, c)) return rc;
    }
    if (alternate)   // join: everything after this half-iteration assumes the one compute stream
      if (int rc = for_members(g, [&](Member& mb) -> int {
            if (int rc = hand_off(g, mb.compute2, mb.ev_join, mb.compute)) return rc;
            if (int rc = mals_set_stream(mb.h, mb.compute)) return mfail(g, mb, rc);
            return MALS_OK;
          }))
        return rc;
    if (int rc = mark_exchanged(g)) return rc;
    if (local.rc != MALS_OK) return gfail(g, local.rc, local.msg);
    return for_members(g, [&](Member& mb) -> int {  // ALS:346-361: f.get() of every worker
      if (int rc = mals_check(mb.h)) return mfail(g, mb, rc);
      return MALS_OK;
    });
  };
  const int local_rc = run();
  const std::string local_msg = g->err;
  for (Member& mb : g->m) (void)mals_set_stream(mb.h, mb.compute);   // (also after a failure in the middle of the chunk loop)
  // a communication failure cannot be agreed upon over the same communicator
  if (local_rc == MALS_COMM_ERROR || local_rc == MALS_HIP_ERROR) return local_rc;
  return agree_status(g, local_rc, local_msg);
}

int mals_group_singular_info(mals_group g, int32_t* side, int64_t* row, int32_t* apparent_rank) {
  if (!g) return MALS_INVALID_ARG;
  if (side) *side = -1;
  if (row) *row = -1;
  if (apparent_rank) *apparent_rank = 0;
  for (Member& mb : g->m) {  // the local member that reported it (multi-process groups: each process knows its own)
    int32_t sd = -1, rk = 0;
    int64_t rw = -1;
    if (mals_singular_info(mb.h, &sd, &rw, &rk) == MALS_OK && sd >= 0) {
      if (side) *side = sd;
      if (row) *row = rw;
      if (apparent_rank) *apparent_rank = rk;
      return MALS_OK;
    }
  }
  return MALS_OK;
}

int mals_group_exchange_only(mals_group g, int side) {
  GSIDE(g, side);
  if (g->bounds[side].empty()) return gfail(g, MALS_INVALID_ARG, "matrix of this side not set");
  if (int rc = for_members(g, [&](Member& mb) { return hand_off(g, mb.compute, mb.ev_solved, mb.comm); })) return rc;
  for (int c = 0; c < g->side_chunks[side]; ++c)
    if (int rc = exchange_chunk(g, side, c)) return rc;
  return mark_exchanged(g);
}

int mals_group_cancel(mals_group g) {
  if (!g) return MALS_INVALID_ARG;
  g->cancelled.store(1);
  return MALS_OK;
}

int mals_group_synchronize(mals_group g) {
  if (!g) return MALS_INVALID_ARG;
  return for_members(g, [&](Member& mb) -> int {
    GHIP(g, hipStreamSynchronize(mb.compute));
    GHIP(g, hipStreamSynchronize(mb.comm));
    return MALS_OK;
  });
}

int mals_group_factorize(mals_group g, double convergence_threshold, int32_t max_iterations, int32_t random_y, int32_t iterate,
                         const int64_t* test_users, int32_t n_test_users, const int64_t* test_items, int32_t n_test_items,
                         int32_t* iterations_out, double* convergence_out) {
  if (!g) return MALS_INVALID_ARG;
  GroupFactorize d{g};
  return mals::factorize_loop(d, convergence_threshold, max_iterations, random_y, iterate, test_users, n_test_users, test_items, n_test_items,
                              iterations_out, convergence_out);
}

}  // extern "C"

// ---- the online write path and the fold-in reads on a group (include/myrrix_als.h; the members' side: mals_serving.hip) ----
namespace {

// what every twin checks first: a group all of whose ranks live in this process
int foldin_group_ready(mals_group g, const char* call) {
  if (!g) return MALS_INVALID_ARG;
  if (!g->single_process)
    return gfail(g, MALS_INVALID_ARG, std::string(call) + ": not for a group of several processes (a process cannot reach another process's members)");
  return MALS_OK;
}

std::vector<mals_handle> member_handles(mals_group g) {
  std::vector<mals_handle> hs;
  for (Member& mb : g->m) hs.push_back(mb.h);
  return hs;
}

// member m keeps the known items of the users own[m] <= u < own[m + 1] (the members are the ranks, in order)
int owned_users(mals_group g, const char* call, std::vector<int64_t>& own) {
  const std::vector<int64_t>& b = g->bounds[MALS_SIDE_X];
  if (b.size() != g->m.size() + 1) return gfail(g, MALS_INVALID_ARG, std::string(call) + ": the user-side matrix is not set (it says who owns a user)");
  own = b;
  own.back() = std::numeric_limits<int64_t>::max();   // grown users: the last rank's
  return MALS_OK;
}

int write_failed(mals_group g, int rc, const char* call, const std::string& msg) {
  return rc == MALS_OK ? rc : gfail(g, rc, std::string(call) + ": " + msg);
}

mals_handle next_reader(mals_group g) { return g->m[g->next_reader.fetch_add(1, std::memory_order_relaxed) % g->m.size()].h; }

// a read's failure text is the answering member's (the last failing read wins; no read waits for a write here)
int read_failed(mals_group g, mals_handle h, int rc) {
  if (rc != MALS_OK) {
    std::lock_guard<std::mutex> lk(g->err_mu);
    g->err = mals_last_error(h);
  }
  return rc;
}

}  // namespace

extern "C" {

int mals_group_set_foldin_solver(mals_group g, int side, mals_solver s) {
  if (int rc = foldin_group_ready(g, "mals_group_set_foldin_solver")) return rc;
  GSIDE(g, side);
  std::vector<mals_handle> hs = member_handles(g);
  std::lock_guard<std::mutex> lk(g->write_mu);
  std::string msg;
  return write_failed(g, malsi_group_set_foldin_solver(hs.data(), (int)hs.size(), side, s, &msg), "mals_group_set_foldin_solver", msg);
}

int mals_group_set_foldin_learn_rate(mals_group g, double rate) {
  if (int rc = foldin_group_ready(g, "mals_group_set_foldin_learn_rate")) return rc;
  if (!std::isfinite(rate)) return gfail(g, MALS_INVALID_ARG, "mals_group_set_foldin_learn_rate: the fold-in learning rate must be finite");
  std::vector<mals_handle> hs = member_handles(g);
  std::lock_guard<std::mutex> lk(g->write_mu);
  std::string msg;
  return write_failed(g, malsi_group_set_foldin_learn_rate(hs.data(), (int)hs.size(), rate, &msg), "mals_group_set_foldin_learn_rate", msg);
}

int mals_group_foldin_stats(mals_group g, int64_t* out6) {
  if (int rc = foldin_group_ready(g, "mals_group_foldin_stats")) return rc;
  if (!out6) return MALS_INVALID_ARG;
  // every member counted the group's writes once: the counters are member 0's, the device times the slowest member's
  for (size_t i = 0; i < g->m.size(); ++i) {
    int64_t o[6];
    if (int rc = mals_foldin_stats(g->m[i].h, o)) return rc;
    for (int j = 0; j < 6; ++j)
      if (i == 0 || (j >= 4 && o[j] > out6[j])) out6[j] = o[j];
  }
  return MALS_OK;
}

// the group twins of setPreference, setUserTag and setItemTag: one batch of one kind
static int group_set_impl(mals_group g, const char* call, int kind, int64_t n, const int64_t* user_row, const int64_t* item_row, const float* value,
                   int32_t* status_out) {
  if (int rc = foldin_group_ready(g, call)) return rc;
  if (n < 0 || (n > 0 && (!user_row || !item_row || !value))) return gfail(g, MALS_INVALID_ARG, std::string(call) + ": bad arguments");
  if (n > (int64_t)1 << 30) return gfail(g, MALS_INVALID_ARG, std::string(call) + ": at most 2^30 updates per call");
  if (n == 0) return MALS_OK;
  std::vector<mals_handle> hs = member_handles(g);
  std::lock_guard<std::mutex> lk(g->write_mu);
  std::vector<int64_t> own;
  if (int rc = owned_users(g, call, own)) return rc;
  std::string msg;
  return write_failed(g, malsi_group_set_preferences(hs.data(), (int)hs.size(), own.data(), n, user_row, item_row, value, kind, status_out, &msg), call,
                      msg);
}

int mals_group_set_preferences(mals_group g, int64_t n, const int64_t* user_row, const int64_t* item_row, const float* value, int32_t* status_out) {
  return group_set_impl(g, "mals_group_set_preferences", 0, n, user_row, item_row, value, status_out);
}

int mals_group_set_user_tags(mals_group g, int64_t n, const int64_t* user_row, const int64_t* tag_item_row, const float* value, int32_t* status_out) {
  return group_set_impl(g, "mals_group_set_user_tags", 2, n, user_row, tag_item_row, value, status_out);
}

int mals_group_set_item_tags(mals_group g, int64_t n, const int64_t* tag_user_row, const int64_t* item_row, const float* value, int32_t* status_out) {
  return group_set_impl(g, "mals_group_set_item_tags", 1, n, tag_user_row, item_row, value, status_out);
}

int mals_group_remove_preferences(mals_group g, int64_t n, const int64_t* user_row, const int64_t* item_row, int64_t* removed_users_out,
                                  int64_t* n_removed_out) {
  if (n_removed_out) *n_removed_out = 0;
  if (int rc = foldin_group_ready(g, "mals_group_remove_preferences")) return rc;
  if (n < 0 || (n > 0 && (!user_row || !item_row))) return gfail(g, MALS_INVALID_ARG, "mals_group_remove_preferences: bad arguments");
  if (n == 0) return MALS_OK;
  std::vector<mals_handle> hs = member_handles(g);
  std::lock_guard<std::mutex> lk(g->write_mu);
  std::vector<int64_t> own;
  if (int rc = owned_users(g, "mals_group_remove_preferences", own)) return rc;
  std::string msg;
  return write_failed(g, malsi_group_remove_preferences(hs.data(), (int)hs.size(), own.data(), n, user_row, item_row, removed_users_out,
                                                        n_removed_out, &msg),
                      "mals_group_remove_preferences", msg);
}

int mals_group_grow_factor_rows(mals_group g, int side, int64_t n_rows_total) {
  if (int rc = foldin_group_ready(g, "mals_group_grow_factor_rows")) return rc;
  GSIDE(g, side);
  std::vector<mals_handle> hs = member_handles(g);
  std::lock_guard<std::mutex> lk(g->write_mu);
  std::string msg;
  // (single process: local member i is rank i, the last one owns the users past the installed matrix)
  if (int rc = malsi_group_grow_factor_rows(hs.data(), (int)hs.size(), side, n_rows_total, (int)hs.size() - 1, &msg))
    return write_failed(g, rc, "mals_group_grow_factor_rows", msg);
  g->n_total[side] = n_rows_total;
  if (side == MALS_SIDE_X) g->users_end.store(n_rows_total, std::memory_order_release);
  return refresh_replica_ptrs(g, side);   // (a capacity doubling moved the replicas)
}

int mals_group_estimate_preferences(mals_group g, int64_t n, const int64_t* user_row, const int64_t* item_row, float* out) {
  if (int rc = foldin_group_ready(g, "mals_group_estimate_preferences")) return rc;
  mals_handle h = next_reader(g);
  return read_failed(g, h, malsi_member_estimate_preferences(h, n, user_row, item_row, out));
}

int mals_group_anonymous_features(mals_group g, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values, float* out,
                                  int32_t* status_out) {
  if (int rc = foldin_group_ready(g, "mals_group_anonymous_features")) return rc;
  mals_handle h = next_reader(g);
  return read_failed(g, h, malsi_member_anonymous_features(h, n_queries, item_ptr, item_row, values, out, status_out));
}

int mals_group_recommend_to_anonymous(mals_group g, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values,
                                      int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out, int32_t* status_out) {
  if (int rc = foldin_group_ready(g, "mals_group_recommend_to_anonymous")) return rc;
  mals_handle h = next_reader(g);
  return read_failed(g, h, malsi_member_recommend_to_anonymous(h, n_queries, item_ptr, item_row, values, how_many, item_idx_out, score_out, n_out,
                                                               status_out));
}

int mals_group_estimate_for_anonymous(mals_group g, int32_t n_queries, const int64_t* to_item, const int64_t* item_ptr, const int64_t* item_row,
                                      const float* values, float* out, int32_t* status_out) {
  if (int rc = foldin_group_ready(g, "mals_group_estimate_for_anonymous")) return rc;
  mals_handle h = next_reader(g);
  return read_failed(g, h, malsi_member_estimate_for_anonymous(h, n_queries, to_item, item_ptr, item_row, values, out, status_out));
}

int mals_group_set_tag_users(mals_group g, int64_t n, const int64_t* user_idx) {
  if (int rc = foldin_group_ready(g, "mals_group_set_tag_users")) return rc;
  if (n < 0 || (n > 0 && !user_idx)) return gfail(g, MALS_INVALID_ARG, "mals_group_set_tag_users: bad tag user list");
  std::vector<mals_handle> hs = member_handles(g);
  std::lock_guard<std::mutex> lk(g->write_mu);
  std::string msg;
  return write_failed(g, malsi_group_set_tag_users(hs.data(), (int)hs.size(), n, user_idx, &msg), "mals_group_set_tag_users", msg);
}

int mals_group_most_popular_items(mals_group g, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  if (int rc = foldin_group_ready(g, "mals_group_most_popular_items")) return rc;
  if (how_many <= 0 || how_many > 4096 || !item_idx_out || !score_out) {
    std::lock_guard<std::mutex> lk(g->err_mu);
    return gfail(g, MALS_INVALID_ARG, "mals_group_most_popular_items: bad arguments (how_many in 1..4096)");
  }
  std::vector<mals_handle> hs = member_handles(g);
  std::string msg;
  const int rc = malsi_group_most_popular_items(hs.data(), (int)hs.size(), how_many, item_idx_out, score_out, n_out, &msg);
  if (rc != MALS_OK) {
    std::lock_guard<std::mutex> lk(g->err_mu);
    return write_failed(g, rc, "mals_group_most_popular_items", msg);
  }
  return MALS_OK;
}

int mals_group_replica_digest(mals_group g, int side, int64_t row_begin, int64_t n_rows, uint64_t* out_per_local_member, int32_t* all_equal_out) {
  if (int rc = foldin_group_ready(g, "mals_group_replica_digest")) return rc;
  GSIDE(g, side);
  if (!out_per_local_member) return gfail(g, MALS_INVALID_ARG, "mals_group_replica_digest: out_per_local_member is NULL");
  std::vector<mals_handle> hs = member_handles(g);
  std::string msg;
  const int rc = malsi_group_factor_digest(hs.data(), (int)hs.size(), side, row_begin, n_rows, out_per_local_member, &msg);
  if (rc != MALS_OK) {
    std::lock_guard<std::mutex> lk(g->err_mu);
    return write_failed(g, rc, "mals_group_replica_digest", msg);
  }
  if (all_equal_out) {
    *all_equal_out = 1;
    for (size_t i = 1; i < hs.size(); ++i)
      if (out_per_local_member[i] != out_per_local_member[0]) *all_equal_out = 0;
  }
  return MALS_OK;
}

int mals_factor_digest_host(const float* rows, int32_t features, int64_t row_begin, int64_t n_rows, uint64_t* out) {
  if (!out || features <= 0 || row_begin < 0 || n_rows < 0 || (n_rows > 0 && !rows)) return MALS_INVALID_ARG;
  uint64_t sum = 0;
  const uint64_t j0 = (uint64_t)row_begin * (uint64_t)features;
  const uint64_t n = (uint64_t)n_rows * (uint64_t)features;
  for (uint64_t e = 0; e < n; ++e) {
    uint32_t bits;
    std::memcpy(&bits, rows + e, sizeof(bits));
    sum += mals::factor_digest_term(j0 + e, bits);
  }
  *out = sum;
  return MALS_OK;
}

}  // extern "C"

// ---- loading a new generation into a group (include/myrrix_als.h; the members' side: generation_group_host.h) -----------------
namespace {

// the arrays of a load that live on `src_dev`, as a member on another device reads them: peer copies on its compute stream
struct LoadCopies {
  mals::DeviceBuffer<int64_t> i64[7];
  mals::DeviceBuffer<float> f32[2];
  mals::DeviceBuffer<int32_t> i32;
};

template <class T>
int load_copy(mals_group g, Member& mb, int src_dev, const T** field, int64_t n, mals::DeviceBuffer<T>& own) {
  if (!*field || n <= 0) return MALS_OK;
  bool copied = false;
  return member_slice(g, mb, *field, src_dev, false, n, own, field, &copied);
}

}  // namespace

extern "C" {

int mals_group_load_generation(mals_group g, const mals_generation_load* load, mals_generation_result* result_out) {
  if (!g) return MALS_INVALID_ARG;
  if (!load || load->struct_size != (int32_t)sizeof(mals_generation_load) || (result_out && result_out->struct_size != (int32_t)sizeof(mals_generation_result)))
    return gfail(g, MALS_INVALID_ARG, "mals_group_load_generation: null argument or struct_size mismatch");
  if (int rc = foldin_group_ready(g, "mals_group_load_generation")) return rc;
  const mals_generation_load& L = *load;
  bool ok = (L.cur_mem_kind == MALS_MEM_HOST || L.cur_mem_kind == MALS_MEM_DEVICE) && (L.new_mem_kind == MALS_MEM_HOST || L.new_mem_kind == MALS_MEM_DEVICE);
  for (int sd = 0; sd < 2 && ok; ++sd)
    ok = L.n_cur[sd] >= 0 && L.n_new[sd] >= 0 && (L.n_cur[sd] == 0 || L.cur_ids[sd]) && (L.n_new[sd] == 0 || (L.new_ids[sd] && L.new_rows[sd])) &&
         L.n_cur[sd] < ((int64_t)1 << 31) && L.n_new[sd] < ((int64_t)1 << 31);
  ok = ok && L.n_item_tag_ids >= 0 && L.n_user_tag_ids >= 0 && (L.n_item_tag_ids == 0 || L.item_tag_ids) && (L.n_user_tag_ids == 0 || L.user_tag_ids);
  if (!ok) return gfail(g, MALS_INVALID_ARG, "mals_group_load_generation: bad arguments (mem kinds, counts in [0, 2^31), null arrays)");
  std::vector<mals_handle> hs = member_handles(g);
  const size_t n = hs.size();
  std::lock_guard<std::mutex> lk(g->write_mu);
  // device arrays live on the first member's device: a member elsewhere reads its own copies
  const int src_dev = g->m[0].device;
  std::vector<mals_generation_load> loads(n, L);
  std::vector<LoadCopies> copies(n);
  const int k = g->cfg.features;
  if (int rc = for_members(g, [&](Member& mb, size_t i) -> int {
        if (mb.device == src_dev) return MALS_OK;
        mals_generation_load& M = loads[i];
        LoadCopies& c = copies[i];
        if (L.cur_mem_kind == MALS_MEM_DEVICE)
          for (int sd = 0; sd < 2; ++sd)
            if (int rc = load_copy(g, mb, src_dev, &M.cur_ids[sd], L.n_cur[sd], c.i64[sd])) return rc;
        if (L.new_mem_kind == MALS_MEM_DEVICE) {
          for (int sd = 0; sd < 2; ++sd) {
            if (int rc = load_copy(g, mb, src_dev, &M.new_ids[sd], L.n_new[sd], c.i64[2 + sd])) return rc;
            if (int rc = load_copy(g, mb, src_dev, &M.new_rows[sd], L.n_new[sd] * k, c.f32[sd])) return rc;
          }
          if (L.new_known_ptr) {
            int64_t nnz = 0;
            if (L.n_new[MALS_SIDE_X] > 0)
              GHIP(g, hipMemcpy(&nnz, L.new_known_ptr + L.n_new[MALS_SIDE_X], sizeof(int64_t), hipMemcpyDeviceToHost));
            if (nnz < 0) return gfail(g, MALS_INVALID_ARG, "mals_group_load_generation: bad known-item arrays of the new model");
            if (int rc = load_copy(g, mb, src_dev, &M.new_known_ptr, L.n_new[MALS_SIDE_X] + 1, c.i64[4])) return rc;
            if (int rc = load_copy(g, mb, src_dev, &M.new_known_idx, nnz, c.i32)) return rc;
          }
          if (int rc = load_copy(g, mb, src_dev, &M.item_tag_ids, L.n_item_tag_ids, c.i64[5])) return rc;
          if (int rc = load_copy(g, mb, src_dev, &M.user_tag_ids, L.n_user_tag_ids, c.i64[6])) return rc;
        }
        GHIP(g, hipStreamSynchronize(mb.compute));
        return MALS_OK;
      }))
    return rc;
  const bool had_bounds = g->bounds[MALS_SIDE_X].size() == n + 1;
  std::vector<int64_t> bx(n + 1, 0), by(n + 1, 0);
  std::string msg;
  g->generation_seq.fetch_add(1, std::memory_order_acq_rel);   // odd: routed reads wait, and repeat what they began before
  const int rc = malsi_group_load_generation(hs.data(), (int)n, loads.data(), result_out, had_bounds ? g->bounds[MALS_SIDE_X].data() : nullptr, bx.data(),
                                             by.data(), &msg);
  int rc2 = MALS_OK;
  if (rc == MALS_OK) {
    const int64_t n_users = bx.back(), n_items = by.back();
    for (int sd = 0; sd < 2; ++sd) {
      const std::vector<int64_t>& nb = sd == MALS_SIDE_X ? bx : by;
      if (g->bounds[sd].size() == nb.size()) std::copy(nb.begin(), nb.end(), g->bounds[sd].begin());   // (in place: readers hold no stale block)
      else g->bounds[sd] = nb;
      g->n_rows[sd] = g->n_total[sd] = sd == MALS_SIDE_X ? n_users : n_items;
    }
    g->users_end.store(n_users, std::memory_order_release);
    // the members' matrices and installed slices named live rows: the handles dropped them, the group's copies go too
    for (Member& mb : g->m) {
      (void)hipSetDevice(mb.device);
      for (int sd = 0; sd < 2; ++sd) {
        mb.d_row_ptr[sd].reset();
        mb.own_col[sd].reset();
        mb.own_val[sd].reset();
      }
      mb.own_known_ptr.reset();
      mb.own_known_idx.reset();
      mb.own_tag_idx.reset();
    }
    for (int sd = 0; sd < 2 && rc2 == MALS_OK; ++sd) rc2 = refresh_replica_ptrs(g, sd);
  }
  g->generation_seq.fetch_add(1, std::memory_order_acq_rel);
  for (size_t i = 0; i < n; ++i) {   // a member's copies go with its device current
    (void)hipSetDevice(g->m[i].device);
    copies[i] = LoadCopies();
  }
  if (rc != MALS_OK) return write_failed(g, rc, "mals_group_load_generation", msg);
  return rc2;
}

static int group_generation_get(mals_group g, int side, bool ids, int64_t* out, const char* call) {
  if (int rc = foldin_group_ready(g, call)) return rc;
  GSIDE(g, side);
  Member& mb = g->m[0];   // (every member holds the same ids and maps)
  const int rc = ids ? mals_generation_get_ids(mb.h, side, out) : mals_generation_get_map(mb.h, side, out);
  return rc == MALS_OK ? rc : mfail(g, mb, rc);
}
int mals_group_generation_get_ids(mals_group g, int side, int64_t* ids_out) { return group_generation_get(g, side, true, ids_out, "mals_group_generation_get_ids"); }
int mals_group_generation_get_map(mals_group g, int side, int64_t* map_out) { return group_generation_get(g, side, false, map_out, "mals_group_generation_get_map"); }

// the group's recent rows are its first member's record, in global rows
int mals_group_mark_recent(mals_group g, int side, int64_t n, const int64_t* rows) {
  if (int rc = foldin_group_ready(g, "mals_group_mark_recent")) return rc;
  GSIDE(g, side);
  std::lock_guard<std::mutex> lk(g->write_mu);
  Member& mb = g->m[0];
  const int rc = mals_mark_recent(mb.h, side, n, rows);
  return rc == MALS_OK ? rc : mfail(g, mb, rc);
}

int mals_group_get_recent(mals_group g, int side, int64_t* rows_out, int64_t* n_out) {
  if (int rc = foldin_group_ready(g, "mals_group_get_recent")) return rc;
  GSIDE(g, side);
  std::lock_guard<std::mutex> lk(g->write_mu);
  Member& mb = g->m[0];
  const int rc = mals_get_recent(mb.h, side, rows_out, n_out);
  return rc == MALS_OK ? rc : mfail(g, mb, rc);
}

int mals_group_generation_plan_host(int32_t world, int32_t features, int64_t n_new, const int64_t* new_known_ptr, int64_t n_kept,
                                    const int64_t* kept_sizes, const int64_t* kept_rows, const int64_t* old_bounds, int64_t* bounds_out,
                                    int64_t* moves_out) {
  if (!bounds_out) return MALS_INVALID_ARG;
  mals::GenGroupPlan p;
  if (!mals::generation_group_plan(world, features, n_new, new_known_ptr, n_kept, kept_sizes, kept_rows, old_bounds, p)) return MALS_INVALID_ARG;
  std::copy(p.bounds.begin(), p.bounds.end(), bounds_out);
  if (moves_out) std::copy(p.move.begin(), p.move.end(), moves_out);
  return MALS_OK;
}

}  // extern "C"
