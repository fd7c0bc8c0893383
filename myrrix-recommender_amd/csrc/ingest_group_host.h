// ingest_group_host.h -- the ingest half of mals_group_ingest_finish (include/myrrix_als.h): every rank of a group has
// ingested one SHARE of the input stream (shares in stream order); the finish gives every rank the users of one id range and
// the items of one bound range, without any rank ever holding the whole input.  Host code of ingest_api.hip.
// Expects before it: ingest_host.h (the ingest object, setup_workspace, transpose_by_item), split_kernels.h,
// ingest_big_kernels.h (the 64-bit scan) and mals_internal.h (malsi_group_ops).
//
//   a. status and text counters of every share in one all-reduce; the header candidate of a share and the "line after the
//      101st bad line" rule are decided on the combined counters, identically on every rank
//   b. user-id splitters from a weighted sample of every rank's records: rank r owns the users with ids in [s_r, s_r+1)
//   c. records split by owner (split_kernels.h), a world x world count matrix, one exchange; runs arrive in share order
//   d. the existing finish on the received records (replay, removeSmall, knownItemIDs, tags): rows of this rank's users
//   e. the ranks' ascending item / user / tag tables all-gathered and merged; columns renumbered to global item indices
//   f. item bounds from mals_plan_shards on the all-reduced entry counts; entries split by item owner, exchanged; a stable
//      sort by item of runs that arrive in ascending user order gives R^T's rows of this rank's items
//   g. records, workspace and exchange buffers are released before the caller declares the factor replicas
#pragma once

namespace {

constexpr int SHARD_SAMPLE = 1024;   // user ids per rank for the splitters
constexpr int SHARD_BADPOS = 101;
// per-rank slot of the first all-reduce
enum { SC_RC, SC_LINES, SC_BAD, SC_HEADER, SC_SKIPPED, SC_SLOW, SC_BYTES, SC_FATAL, SC_NPOS, SC_POS, SC_N = SC_POS + SHARD_BADPOS };

__global__ void shard_sample_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t m, int64_t* __restrict__ out) {
  MALS_GRID_STRIDE(j, m) out[j] = ids[(j * n) / m];
}
// entries of a CSR slice as (global row, column, value)
__global__ void shard_expand_rows_kernel(const int64_t* __restrict__ ptr, int64_t n_rows, int64_t row_base, int64_t* __restrict__ row_out) {
  MALS_GRID_STRIDE(r, n_rows)
    for (int64_t e = ptr[r]; e < ptr[r + 1]; ++e) row_out[e] = row_base + r;
}
__global__ void shard_widen_kernel(const int32_t* __restrict__ in, int64_t n, int64_t* __restrict__ out) {
  MALS_GRID_STRIDE(i, n) out[i] = in[i];
}
__global__ void shard_remap_kernel(int32_t* __restrict__ col, int64_t n, const int32_t* __restrict__ map) {
  MALS_GRID_STRIDE(i, n) col[i] = map[col[i]];
}
// (item - item_lo) << 32 | user, value bits: the sort keys of R^T's rows
__global__ void shard_transpose_keys_kernel(const int64_t* __restrict__ user, const int64_t* __restrict__ item, const float* __restrict__ val, int64_t n,
                                            int64_t item_lo, uint64_t* __restrict__ keys, unsigned* __restrict__ pay) {
  MALS_GRID_STRIDE(i, n) {
    keys[i] = ((uint64_t)(uint32_t)(item[i] - item_lo) << 32) | (uint32_t)user[i];
    pay[i] = __float_as_uint(val[i]);
  }
}

struct ShardCtx {
  mals_ingest* g;
  const malsi_group_ops* ops;
  int world, nl;
  std::string comm_msg;
};

// A rank never leaves between two collectives on a local failure (real RCCL would hang the others in the next one): local
// failures are recorded, and every rank agrees on the worst status before the next collective that depends on them.

// a HIP call's status as a library status, with the message kept on the ingest
int hip_status(mals_ingest g, hipError_t e, const char* what) {
  if (e == hipSuccess) return MALS_OK;
  return fail(g, e == hipErrorOutOfMemory ? MALS_OOM : MALS_HIP_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}

// every rank's worst local status (max over the ranks; the codes are positive).  The group's own status words carry it: no
// allocation on the way.
int shard_agree(ShardCtx& c, const std::vector<int>& rc) {
  const int agreed = c.ops->agree(c.ops->ctx, rc.data());
  if (agreed == MALS_COMM_ERROR || agreed < 0) {
    c.comm_msg = c.ops->last_error(c.ops->ctx);
    return MALS_COMM_ERROR;
  }
  return agreed;
}
int shard_agree1(ShardCtx& c, int member, int rc) {
  std::vector<int> v((size_t)c.nl, MALS_OK);
  v[(size_t)member] = rc;
  return shard_agree(c, v);
}

// an all-reduce of one host vector per local member; the (identical) result in out.  Every rank returns the same status.
int shard_allreduce(ShardCtx& c, const std::vector<std::vector<int64_t>>& per, int op_max, std::vector<int64_t>* out) {
  const int64_t n = (int64_t)per[0].size();
  std::vector<DeviceBuffer<int64_t>> buf((size_t)c.nl);
  std::vector<int64_t*> dev((size_t)c.nl);
  std::vector<int> rcs((size_t)c.nl, MALS_OK);
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    int rc = hip_status(g, hipSetDevice(g->device), "hipSetDevice");
    if (!rc) rc = hip_status(g, buf[(size_t)i].alloc((size_t)std::max<int64_t>(n, 1)), "all-reduce buffer");
    if (!rc && n) rc = hip_status(g, hipMemcpy(buf[(size_t)i].get(), per[(size_t)i].data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice), "hipMemcpy");
    rcs[(size_t)i] = rc;
    dev[(size_t)i] = buf[(size_t)i].get();
  }
  if (int rc = shard_agree(c, rcs)) return rc;
  if (n) {
    if (int rc = c.ops->allreduce_i64(c.ops->ctx, dev.data(), n, op_max)) {
      c.comm_msg = c.ops->last_error(c.ops->ctx);
      return rc;
    }
  }
  out->assign((size_t)n, 0);
  int rc0 = hip_status(c.g[0], hipSetDevice(c.g[0]->device), "hipSetDevice");
  if (!rc0 && n) rc0 = hip_status(c.g[0], hipMemcpy(out->data(), dev[0], sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost), "hipMemcpy");
  return shard_agree1(c, 0, rc0);
}

// all-gather: member i contributes rows of `len[rank]` int64 at device pointer src[i]; out = the concatenation in rank order on
// every member (device), of sum(len) elements
int shard_allgather(ShardCtx& c, const std::vector<int64_t>& len, const std::vector<const int64_t*>& src, std::vector<DeviceBuffer<int64_t>>* out) {
  std::vector<int64_t> off((size_t)c.world + 1, 0);
  for (int r = 0; r < c.world; ++r) off[(size_t)r + 1] = off[(size_t)r] + len[(size_t)r];
  const int64_t n = off.back();
  out->clear();
  out->resize((size_t)c.nl);
  std::vector<int64_t*> dev((size_t)c.nl);
  std::vector<int> rcs((size_t)c.nl, MALS_OK);
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    const int r = c.ops->ranks[i];
    int rc = hip_status(g, hipSetDevice(g->device), "hipSetDevice");
    if (!rc) rc = hip_status(g, (*out)[(size_t)i].alloc((size_t)std::max<int64_t>(n, 1)), "all-gather buffer");
    dev[(size_t)i] = (*out)[(size_t)i].get();
    if (!rc && n) rc = hip_status(g, hipMemsetAsync(dev[(size_t)i], 0, sizeof(int64_t) * (size_t)n, g->stream), "hipMemsetAsync");
    if (!rc && len[(size_t)r])
      rc = hip_status(g, hipMemcpyAsync(dev[(size_t)i] + off[(size_t)r], src[(size_t)i], sizeof(int64_t) * (size_t)len[(size_t)r], hipMemcpyDeviceToDevice, g->stream),
                      "hipMemcpyAsync");
    if (!rc) rc = hip_status(g, hipStreamSynchronize(g->stream), "hipStreamSynchronize");
    rcs[(size_t)i] = rc;
  }
  if (int rc = shard_agree(c, rcs)) return rc;
  if (n == 0) return MALS_OK;
  if (int rc = c.ops->allreduce_i64(c.ops->ctx, dev.data(), n, 0)) {
    c.comm_msg = c.ops->last_error(c.ops->ctx);
    return rc;
  }
  return MALS_OK;
}

// Records (a, b, c) of one member split by `key` (a or b) at the splitters into world runs: *out_* in bucket order, counts[q]
int shard_split(mals_ingest g, const int64_t* key, const std::vector<int64_t>& splitters, const int64_t* a, const int64_t* b, const float* v, int64_t n,
                DeviceBuffer<int64_t>& oa, DeviceBuffer<int64_t>& ob, DeviceBuffer<float>& ov, std::vector<int64_t>* counts) {
  const int nb = (int)splitters.size() + 1;
  counts->assign((size_t)nb, 0);
  ICHK(g, oa.alloc((size_t)std::max<int64_t>(n, 1)));
  ICHK(g, ob.alloc((size_t)std::max<int64_t>(n, 1)));
  ICHK(g, ov.alloc((size_t)std::max<int64_t>(n, 1)));
  if (n == 0) return MALS_OK;
  const int64_t n_tiles = (n + SPLIT_TILE - 1) / SPLIT_TILE;
  const int64_t n_counts = (int64_t)nb * n_tiles;
  const int64_t scan_tiles = (n_counts + SC_TILE - 1) / SC_TILE;
  DeviceBuffer<int64_t> spl, offs;
  DeviceBuffer<uint8_t> dest;
  DeviceBuffer<unsigned> counts_d;
  DeviceBuffer<unsigned long long> sums;
  ICHK(g, spl.alloc(std::max<size_t>(splitters.size(), 1)));
  ICHK(g, dest.alloc((size_t)n));
  ICHK(g, counts_d.alloc((size_t)n_counts));
  ICHK(g, offs.alloc((size_t)n_counts + 1));
  ICHK(g, sums.alloc((size_t)scan_tiles + 1));
  if (!splitters.empty()) ICHK(g, hipMemcpy(spl.get(), splitters.data(), sizeof(int64_t) * splitters.size(), hipMemcpyHostToDevice));
  EventPair ev;
  ICHK(g, ev.ensure());
  ICHK(g, hipEventRecord(ev.begin, g->stream));
  ITRY(launch_grid(g, {(unsigned)n_tiles}, split_count_kernel, key, n, spl.get(), nb - 1, n_tiles, dest.get(), counts_d.get()));
  ITRY(launch_grid(g, {(unsigned)scan_tiles}, big_scan64_reduce_kernel, counts_d.get(), n_counts, sums.get()));
  ITRY(launch_grid(g, {1, 64}, big_scan64_sums_kernel, sums.get(), scan_tiles, sums.get() + scan_tiles));
  ITRY(launch_grid(g, {(unsigned)scan_tiles}, big_scan64_apply_kernel, counts_d.get(), n_counts, sums.get(), sums.get() + scan_tiles, offs.get()));
  ITRY(launch_grid(g, {(unsigned)n_tiles}, split_scatter_kernel, dest.get(), n, nb, n_tiles, offs.get(), a, b, v, oa.get(), ob.get(), ov.get()));
  ICHK(g, hipEventRecord(ev.end, g->stream));
  ICHK(g, hipEventSynchronize(ev.end));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ev.begin, ev.end);
  g->split_ms += ms;
  // the traffic of the two split kernels: count pass 8 B key read + 1 B destination written, scatter 1 B destination + 20 B
  // record read and 20 B written (the scan over tiles x buckets, 12 B per tile and bucket, is below 1 % at world <= 8)
  g->split_bytes += 50.0 * (double)n;
  std::vector<int64_t> starts((size_t)nb + 1);
  for (int q = 0; q < nb; ++q) ICHK(g, hipMemcpy(&starts[(size_t)q], offs.get() + (int64_t)q * n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost));
  starts[(size_t)nb] = n;
  for (int q = 0; q < nb; ++q) (*counts)[(size_t)q] = starts[(size_t)q + 1] - starts[(size_t)q];
  return MALS_OK;
}

// Every member's records (three arrays, runs per destination rank given by `cnt` rows of the world x world matrix) to their
// owners; the receivers get the runs in source-rank order
int shard_exchange(ShardCtx& c, const std::vector<int64_t>& mat, std::vector<DeviceBuffer<int64_t>>& sa, std::vector<DeviceBuffer<int64_t>>& sb,
                   std::vector<DeviceBuffer<float>>& sv, std::vector<DeviceBuffer<int64_t>>& ra, std::vector<DeviceBuffer<int64_t>>& rb,
                   std::vector<DeviceBuffer<float>>& rv, std::vector<int64_t>* n_recv) {
  const int W = c.world;
  n_recv->assign((size_t)c.nl, 0);
  std::vector<int64_t> soff((size_t)c.nl * (W + 1)), roff((size_t)c.nl * (W + 1));
  for (int i = 0; i < c.nl; ++i) {
    const int me = c.ops->ranks[i];
    int64_t s = 0, r = 0;
    for (int q = 0; q <= W; ++q) {
      soff[(size_t)i * (W + 1) + q] = s;
      roff[(size_t)i * (W + 1) + q] = r;
      if (q < W) {
        s += mat[(size_t)me * W + q];
        r += mat[(size_t)q * W + me];
      }
    }
    (*n_recv)[(size_t)i] = r;
  }
  ra.clear(); rb.clear(); rv.clear();
  ra.resize((size_t)c.nl); rb.resize((size_t)c.nl); rv.resize((size_t)c.nl);
  int local_rc = MALS_OK;
  for (int i = 0; i < c.nl && !local_rc; ++i) {
    mals_ingest g = c.g[i];
    const size_t m = (size_t)std::max<int64_t>((*n_recv)[(size_t)i], 1);
    if (hipSetDevice(g->device) != hipSuccess || ra[(size_t)i].alloc(m) != hipSuccess || rb[(size_t)i].alloc(m) != hipSuccess || rv[(size_t)i].alloc(m) != hipSuccess)
      local_rc = fail(g, MALS_OOM, "sharded ingest: receive buffers: out of device memory");
  }
  std::vector<int> rcs((size_t)c.nl, local_rc);
  if (int agreed = shard_agree(c, rcs)) return agreed;
  for (int arr = 0; arr < 3; ++arr) {
    const int64_t es = arr == 2 ? 4 : 8;
    std::vector<const uint8_t*> snd((size_t)c.nl);
    std::vector<uint8_t*> rcv((size_t)c.nl);
    std::vector<int64_t> so(soff.size()), ro(roff.size());
    for (size_t k = 0; k < so.size(); ++k) {
      so[k] = soff[k] * es;
      ro[k] = roff[k] * es;
    }
    for (int i = 0; i < c.nl; ++i) {
      snd[(size_t)i] = arr == 0 ? (const uint8_t*)sa[(size_t)i].get() : arr == 1 ? (const uint8_t*)sb[(size_t)i].get() : (const uint8_t*)sv[(size_t)i].get();
      rcv[(size_t)i] = arr == 0 ? (uint8_t*)ra[(size_t)i].get() : arr == 1 ? (uint8_t*)rb[(size_t)i].get() : (uint8_t*)rv[(size_t)i].get();
    }
    if (int rc = c.ops->exchange(c.ops->ctx, snd.data(), so.data(), rcv.data(), ro.data())) {
      c.comm_msg = c.ops->last_error(c.ops->ctx);
      return rc;
    }
  }
  return MALS_OK;
}

// a: status + counters of every share decided on the combined counters
int shard_decide_text(ShardCtx& c, const std::vector<int64_t>& all, std::string* why) {
  int64_t B = 0, lines = 0, bad = 0, hdr = 0, skip = 0, slow = 0, bytes = 0;
  bool any_before = false;
  int abort_share = -1;
  int64_t abort_after = 0;
  for (int s = 0; s < c.world; ++s) {
    const int64_t* sc = &all[(size_t)s * SC_N];
    const int64_t L = sc[SC_LINES];
    const bool hc = sc[SC_HEADER] > 0 && any_before;   // a header candidate that is not line 1 of the whole input: a bad line
    const int64_t bad_s = sc[SC_BAD] + (hc ? 1 : 0);
    if (abort_share < 0) {
      if (B > 100 && L > 0) {
        abort_share = s;
        abort_after = 0;
      } else if (B + bad_s > 100) {
        std::vector<int64_t> P;
        if (hc) P.push_back(1);
        for (int64_t k = 0; k < sc[SC_NPOS]; ++k) P.push_back(sc[SC_POS + k]);
        const int64_t k = 101 - B;   // the 101st bad line of the stream is the k-th of this share
        const int64_t pos = k - 1 < (int64_t)P.size() ? P[(size_t)(k - 1)] : L;
        if (L > pos) {
          abort_share = s;
          abort_after = pos;
        }
      }
    }
    B += bad_s;
    lines += L;
    bad += bad_s;
    hdr += sc[SC_HEADER] - (hc ? 1 : 0);
    skip += sc[SC_SKIPPED];
    slow += sc[SC_SLOW];
    bytes += sc[SC_BYTES];
    any_before = any_before || L > 0;
  }
  int fail_share = -1;
  for (int s = 0; s < c.world && fail_share < 0; ++s)
    if (all[(size_t)s * SC_N + SC_RC] != 0) fail_share = s;
  int code = MALS_OK;
  if (abort_share >= 0 &&
      (fail_share < 0 || abort_share < fail_share ||
       (abort_share == fail_share && all[(size_t)fail_share * SC_N + SC_FATAL] > abort_after))) {
    code = MALS_IO_ERROR;
    *why = "Too many bad lines; aborting";
  } else if (fail_share >= 0) {
    code = (int)all[(size_t)fail_share * SC_N + SC_RC];
    *why = "share " + std::to_string(fail_share) + " failed with status " + std::to_string(code);
  }
  if (code == MALS_OK) {
    for (int i = 0; i < c.nl; ++i) {
      mals_ingest g = c.g[i];
      g->lines = lines;
      g->bad_lines = bad;
      g->header_lines = hdr;
      g->skipped_lines = skip;
      g->slow_lines = slow;
      g->text_bytes = bytes;
    }
  }
  return code;
}

// b: world - 1 user-id splitters from the weighted samples, the same on every rank
std::vector<int64_t> shard_splitters(int world, const std::vector<int64_t>& all) {
  const int S = SHARD_SAMPLE + 2;
  std::vector<std::pair<int64_t, double>> smp;
  double W = 0.0;
  for (int r = 0; r < world; ++r) {
    const int64_t n = all[(size_t)r * S], m = all[(size_t)r * S + 1];
    for (int64_t j = 0; j < m; ++j) smp.push_back({all[(size_t)r * S + 2 + j], (double)n / (double)m});
    W += (double)n;
  }
  std::sort(smp.begin(), smp.end());
  std::vector<int64_t> spl((size_t)world - 1, std::numeric_limits<int64_t>::max());
  double acc = 0.0;
  size_t q = 0;
  for (int j = 1; j < world; ++j) {
    const double target = W * j / world;
    while (q < smp.size() && acc + smp[q].second <= target) acc += smp[q++].second;
    if (q < smp.size()) spl[(size_t)j - 1] = smp[q].first;
  }
  return spl;
}

// ---- the steps of the group finish, in the order shard_finish_impl runs them.  A step that talks to the other ranks returns
// the same status on every rank; its collective calls are part of its contract (ranks in other processes meet them call for call).

// one int64 vector of `len` per local member, for an all-reduce in which every rank fills its own slots
std::vector<std::vector<int64_t>> shard_slots(const ShardCtx& c, int64_t len) {
  return std::vector<std::vector<int64_t>>((size_t)c.nl, std::vector<int64_t>((size_t)len, 0));
}

// a. the text status: status and counters of every share in one all-reduce, decided on the combined counters
int shard_agree_text(ShardCtx& c) {
  std::vector<std::vector<int64_t>> per = shard_slots(c, (int64_t)c.world * SC_N);
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    const int r = c.ops->ranks[i];
    int64_t* sc = &per[(size_t)i][(size_t)r * SC_N];
    int rc = g->text_failed ? g->text_fail_code : g->carry_len ? MALS_INVALID_ARG : MALS_OK;
    if (!rc && g->share != r) rc = fail(g, MALS_INVALID_ARG, "the share of local member " + std::to_string(i) + " is not its rank");
    sc[SC_RC] = rc;
    sc[SC_LINES] = g->lines;
    sc[SC_BAD] = g->bad_lines;
    sc[SC_HEADER] = g->header_lines;
    sc[SC_SKIPPED] = g->skipped_lines;
    sc[SC_SLOW] = g->slow_lines;
    sc[SC_BYTES] = g->text_bytes;
    sc[SC_FATAL] = g->fatal_line;
    sc[SC_NPOS] = (int64_t)std::min<size_t>(g->bad_pos.size(), SHARD_BADPOS);
    for (int64_t k = 0; k < sc[SC_NPOS]; ++k) sc[SC_POS + k] = g->bad_pos[(size_t)k];
  }
  std::vector<int64_t> all;
  ITRY(shard_allreduce(c, per, 0, &all));
  std::string why;
  const int rc = shard_decide_text(c, all, &why);
  for (int i = 0; i < c.nl && rc; ++i) {
    mals_ingest g = c.g[i];
    if (!g->text_failed || g->text_fail_code != rc) g->err = why;
    else g->err = g->text_fail_msg;
  }
  return rc;
}

// b. the user splitters: a sample of every member's user ids, all-reduced; the same splitters on every rank
int shard_user_splitters(ShardCtx& c, std::vector<int64_t>* spl) {
  const int S = SHARD_SAMPLE + 2;
  std::vector<std::vector<int64_t>> per = shard_slots(c, (int64_t)c.world * S);
  std::vector<int> rcs((size_t)c.nl, MALS_OK);
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    const int r = c.ops->ranks[i];
    const int64_t m = std::min<int64_t>(g->n, SHARD_SAMPLE);
    per[(size_t)i][(size_t)r * S] = g->n;
    per[(size_t)i][(size_t)r * S + 1] = m;
    if (m == 0) continue;
    DeviceBuffer<int64_t> d;
    if (hipSetDevice(g->device) != hipSuccess || d.alloc((size_t)m) != hipSuccess) {
      rcs[(size_t)i] = fail(g, MALS_OOM, "sharded ingest: sample: out of device memory");
      continue;
    }
    if (launch(g, m, shard_sample_kernel, g->d_user.get(), g->n, m, d.get()) != MALS_OK ||
        hipMemcpyAsync(&per[(size_t)i][(size_t)r * S + 2], d.get(), sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
        hipStreamSynchronize(g->stream) != hipSuccess)
      rcs[(size_t)i] = fail(g, MALS_HIP_ERROR, "sharded ingest: sample failed");
  }
  ITRY(shard_agree(c, rcs));
  std::vector<int64_t> all;
  ITRY(shard_allreduce(c, per, 0, &all));
  *spl = shard_splitters(c.world, all);
  return MALS_OK;
}

// c / f. One redistribution of rows (two ids and a value) among the ranks.  split(i, &cnt) splits member i's rows by owner
// into the send buffers (shard_split) and counts the runs; the world x world count matrix is all-reduced and every run goes
// to its owner in one exchange.  The receivers hold the runs in source-rank order; the caller adopts them.
struct ShardRuns {
  std::vector<DeviceBuffer<int64_t>> sa, sb, ra, rb;
  std::vector<DeviceBuffer<float>> sv, rv;
  std::vector<int64_t> n_recv;
  explicit ShardRuns(int nl) : sa((size_t)nl), sb((size_t)nl), sv((size_t)nl) {}
  void release_sent(int i) { sa[(size_t)i].reset(); sb[(size_t)i].reset(); sv[(size_t)i].reset(); }
  void release_received(int i) { ra[(size_t)i].reset(); rb[(size_t)i].reset(); rv[(size_t)i].reset(); }
};
template <typename Split>
int shard_redistribute(ShardCtx& c, ShardRuns& R, bool records_are_source, Split&& split) {
  const int W = c.world;
  std::vector<std::vector<int64_t>> per = shard_slots(c, (int64_t)W * W);
  std::vector<int> rcs((size_t)c.nl, MALS_OK);
  for (int i = 0; i < c.nl; ++i) {
    std::vector<int64_t> cnt;
    rcs[(size_t)i] = split(i, &cnt);
    if (!rcs[(size_t)i])
      for (int q = 0; q < W; ++q) per[(size_t)i][(size_t)c.ops->ranks[i] * W + q] = cnt[(size_t)q];
  }
  ITRY(shard_agree(c, rcs));
  std::vector<int64_t> mat;
  ITRY(shard_allreduce(c, per, 0, &mat));
  for (int i = 0; i < c.nl && records_are_source; ++i) {   // the split copies hold the records now
    (void)hipSetDevice(c.g[i]->device);
    c.g[i]->d_user.reset(); c.g[i]->d_item.reset(); c.g[i]->d_value.reset(); c.g[i]->d_kind.reset();
  }
  return shard_exchange(c, mat, R.sa, R.sb, R.sv, R.ra, R.rb, R.rv, &R.n_recv);
}

// c. records to the owners of their users
int shard_redistribute_records(ShardCtx& c, const std::vector<int64_t>& spl) {
  ShardRuns R(c.nl);
  ITRY(shard_redistribute(c, R, true, [&](int i, std::vector<int64_t>* cnt) -> int {
    mals_ingest g = c.g[i];
    if (hipSetDevice(g->device) != hipSuccess) return MALS_HIP_ERROR;
    return shard_split(g, g->d_user.get(), spl, g->d_user.get(), g->d_item.get(), g->d_value.get(), g->n, R.sa[(size_t)i], R.sb[(size_t)i], R.sv[(size_t)i], cnt);
  }));
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    (void)hipSetDevice(g->device);
    R.release_sent(i);
    g->d_user = std::move(R.ra[(size_t)i]);
    g->d_item = std::move(R.rb[(size_t)i]);
    g->d_value = std::move(R.rv[(size_t)i]);
    g->n = R.n_recv[(size_t)i];
    g->shard_records = g->n;
  }
  return MALS_OK;
}

// d. the one-device finish on every member's users; records and workspace go: nothing of them is needed afterwards
int shard_finish_members(ShardCtx& c) {
  std::vector<int> rcs((size_t)c.nl, MALS_OK);
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    const double sm = g->split_ms, sbytes = g->split_bytes;
    rcs[(size_t)i] = mals_ingest_finish(g);
    g->split_ms = sm;
    g->split_bytes = sbytes;
    (void)hipSetDevice(g->device);
    g->release_work();
  }
  return shard_agree(c, rcs);
}

// e. the group's tables, as every rank knows them after the members' finishes
struct ShardTables {
  std::vector<int64_t> sizes;                        // per rank: users, items, tags0, tags1
  int64_t n_users = 0, n_items = 0;
  std::vector<int64_t> items_glob;                   // the ranks' item tables merged, ascending (host)
  std::vector<std::vector<int64_t>> local_items;     // per local member: its own item table (host)
  std::vector<DeviceBuffer<int64_t>> users_glob;     // per local member: the ranks' user tables in rank order = ascending
  std::vector<int64_t> tags_glob[2];
  std::vector<std::vector<int32_t>> maps;            // per local member: its item index -> global item index
  std::vector<int64_t> column(int world, int k) const {
    std::vector<int64_t> v((size_t)world);
    for (int r = 0; r < world; ++r) v[(size_t)r] = sizes[(size_t)r * 4 + k];
    return v;
  }
};

int shard_table_sizes(ShardCtx& c, ShardTables& T) {
  std::vector<std::vector<int64_t>> per = shard_slots(c, (int64_t)c.world * 4);
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    const int64_t mine[4] = {g->n_users, g->n_items, g->n_tag_ids[0], g->n_tag_ids[1]};
    std::copy(mine, mine + 4, &per[(size_t)i][(size_t)c.ops->ranks[i] * 4]);
  }
  return shard_allreduce(c, per, 0, &T.sizes);
}

// one table of every member (table(g): its device pointer, len[rank]: its length) all-gathered in rank order into
// *gathered (one device copy per member) and, where the host merges it, brought to the host as *cat
template <typename Table>
int shard_gather_table(ShardCtx& c, const std::vector<int64_t>& len, Table&& table, std::vector<DeviceBuffer<int64_t>>* gathered,
                       std::vector<int64_t>* cat = nullptr) {
  std::vector<const int64_t*> src((size_t)c.nl);
  for (int i = 0; i < c.nl; ++i) src[(size_t)i] = table(c.g[i]);
  ITRY(shard_allgather(c, len, src, gathered));
  if (!cat) return MALS_OK;
  int64_t tot = 0;
  for (int64_t v : len) tot += v;
  cat->assign((size_t)tot, 0);
  int rc0 = hip_status(c.g[0], hipSetDevice(c.g[0]->device), "hipSetDevice");
  if (!rc0 && tot) rc0 = hip_status(c.g[0], hipMemcpy(cat->data(), (*gathered)[0].get(), sizeof(int64_t) * (size_t)tot, hipMemcpyDeviceToHost), "hipMemcpy");
  return shard_agree1(c, 0, rc0);
}

// item tables: all-gathered, merged on the host (each is ascending: pairwise merges, no sort)
int shard_merge_item_tables(ShardCtx& c, ShardTables& T) {
  const std::vector<int64_t> n_items_r = T.column(c.world, 1);
  std::vector<int64_t> cat;
  std::vector<DeviceBuffer<int64_t>> gathered;
  ITRY(shard_gather_table(c, n_items_r, [](mals_ingest g) { return g->ids[1].get(); }, &gathered, &cat));
  T.local_items.resize((size_t)c.nl);
  int64_t off = 0;
  for (int r = 0; r < c.world; ++r) {
    const auto b = cat.begin() + off, e = b + n_items_r[(size_t)r];
    std::vector<int64_t> m;
    m.reserve(T.items_glob.size() + (size_t)n_items_r[(size_t)r]);
    std::set_union(T.items_glob.begin(), T.items_glob.end(), b, e, std::back_inserter(m));
    T.items_glob.swap(m);
    for (int i = 0; i < c.nl; ++i)
      if (c.ops->ranks[i] == r) T.local_items[(size_t)i].assign(b, e);
    off += n_items_r[(size_t)r];
  }
  T.n_items = (int64_t)T.items_glob.size();
  return MALS_OK;
}

// f. per-item entry counts of every rank, all-reduced -> the item bounds of the group (mals_plan_shards)
int shard_plan_item_bounds(ShardCtx& c, ShardTables& T, int64_t* bounds_y) {
  const int64_t n_items = T.n_items;
  T.maps.resize((size_t)c.nl);
  std::vector<std::vector<int64_t>> per = shard_slots(c, std::max<int64_t>(n_items, 1));
  std::vector<int> rcs((size_t)c.nl, MALS_OK);
  for (int i = 0; i < c.nl; ++i) {
    mals_ingest g = c.g[i];
    const std::vector<int64_t>& li = T.local_items[(size_t)i];
    std::vector<int32_t>& map = T.maps[(size_t)i];
    map.resize(li.size());
    for (size_t j = 0; j < li.size(); ++j) map[j] = (int32_t)(std::lower_bound(T.items_glob.begin(), T.items_glob.end(), li[j]) - T.items_glob.begin());
    std::vector<int64_t> cp(li.size() + 1);
    int rc = hip_status(g, hipSetDevice(g->device), "hipSetDevice");
    if (!rc) rc = hip_status(g, hipMemcpy(cp.data(), g->ptr[1].get(), sizeof(int64_t) * cp.size(), hipMemcpyDeviceToHost), "hipMemcpy");
    rcs[(size_t)i] = rc;
    if (!rc)
      for (size_t j = 0; j < li.size(); ++j) per[(size_t)i][(size_t)map[j]] = cp[j + 1] - cp[j];
  }
  ITRY(shard_agree(c, rcs));
  std::vector<int64_t> cnt;
  ITRY(shard_allreduce(c, per, 0, &cnt));
  std::vector<int64_t> rp((size_t)n_items + 1, 0);
  for (int64_t j = 0; j < n_items; ++j) rp[(size_t)j + 1] = rp[(size_t)j] + cnt[(size_t)j];
  const int rc = mals_plan_shards(rp.data(), n_items, c.world, -1.0, c.ops->features, bounds_y);
  for (int i = 0; i < c.nl && rc; ++i) fail(c.g[i], rc, "mals_plan_shards failed");
  return rc;
}

// f. member i's entries as (global user, global item, value), split by the owner of the item.  Its columns and knownItemIDs
// become global item indices on the way; its local R^T is not needed any more.
int shard_split_entries(ShardCtx& c, int i, const ShardTables& T, const std::vector<int64_t>& yspl, int64_t user_base, ShardRuns& R, std::vector<int64_t>* cnt) {
  mals_ingest g = c.g[i];
  const std::vector<int32_t>& host_map = T.maps[(size_t)i];
  ICHK(g, hipSetDevice(g->device));
  const int64_t nnz = g->nnz, nu = g->n_users;
  DeviceBuffer<int32_t> map;
  ICHK(g, map.alloc(std::max<size_t>(host_map.size(), 1)));
  if (!host_map.empty()) ICHK(g, hipMemcpy(map.get(), host_map.data(), sizeof(int32_t) * host_map.size(), hipMemcpyHostToDevice));
  if (nnz) ITRY(launch(g, nnz, shard_remap_kernel, g->col[0].get(), nnz, map.get()));
  if (g->known_ptr && g->n_known) ITRY(launch(g, g->n_known, shard_remap_kernel, g->known_idx.get(), g->n_known, map.get()));
  DeviceBuffer<int64_t> eu, ei;
  ICHK(g, eu.alloc((size_t)std::max<int64_t>(nnz, 1)));
  ICHK(g, ei.alloc((size_t)std::max<int64_t>(nnz, 1)));
  if (nnz) {
    ITRY(launch(g, nu, shard_expand_rows_kernel, g->ptr[0].get(), nu, user_base, eu.get()));
    ITRY(launch(g, nnz, shard_widen_kernel, g->col[0].get(), nnz, ei.get()));
  }
  ICHK(g, hipStreamSynchronize(g->stream));
  g->ptr[1].reset(); g->col[1].reset(); g->val[1].reset();
  return shard_split(g, ei.get(), yspl, eu.get(), ei.get(), g->val[0].get(), nnz, R.sa[(size_t)i], R.sb[(size_t)i], R.sv[(size_t)i], cnt);
}

// f. member i's rows of R^T, items [y0, y0 + ny), from the m entries it received: the runs arrive in ascending user order,
// so a stable sort on the item half of the key alone does it
int shard_build_item_slice(ShardCtx& c, int i, ShardRuns& R, int64_t y0, int64_t ny) {
  mals_ingest g = c.g[i];
  ICHK(g, hipSetDevice(g->device));
  R.release_sent(i);
  const int64_t m = R.n_recv[(size_t)i];
  ICHK(g, g->ptr[1].alloc((size_t)ny + 1));
  ICHK(g, g->col[1].alloc((size_t)std::max<int64_t>(m, 1)));
  ICHK(g, g->val[1].alloc((size_t)std::max<int64_t>(m, 1)));
  if (m > 0) {
    Scratch s;
    ITRY(setup_workspace(g, s, m, 0));
    ITRY(launch(g, m, shard_transpose_keys_kernel, R.ra[(size_t)i].get(), R.rb[(size_t)i].get(), R.rv[(size_t)i].get(), m, y0, s.keys[0], s.pay[0]));
    ITRY(transpose_by_item(g, s, m, ny, g->ptr[1].get(), g->col[1].get(), g->val[1].get()));
    ICHK(g, hipStreamSynchronize(g->stream));
    for (int b = 0; b < mals_ingest_s::N_WS; ++b) g->ws[b].reset();
  } else {
    ICHK(g, hipMemset(g->ptr[1].get(), 0, sizeof(int64_t) * ((size_t)ny + 1)));
  }
  R.release_received(i);
  g->slice_begin[1] = y0;
  g->slice_rows[1] = ny;
  g->slice_nnz[1] = m;
  return MALS_OK;
}

// the global tables on member i; from here on its counts are the group's and its matrices are slices
int shard_install_tables(ShardCtx& c, int i, ShardTables& T, int64_t user_base) {
  mals_ingest g = c.g[i];
  const int64_t n_users = T.n_users, n_items = T.n_items;
  const int64_t x_rows = g->n_users, x_nnz = g->nnz;
  ICHK(g, g->ids[0].alloc((size_t)std::max<int64_t>(n_users, 1)));
  if (n_users) ICHK(g, hipMemcpy(g->ids[0].get(), T.users_glob[(size_t)i].get(), sizeof(int64_t) * (size_t)n_users, hipMemcpyDeviceToDevice));
  T.users_glob[(size_t)i].reset();
  ICHK(g, g->ids[1].alloc((size_t)std::max<int64_t>(n_items, 1)));
  if (n_items) ICHK(g, hipMemcpy(g->ids[1].get(), T.items_glob.data(), sizeof(int64_t) * (size_t)n_items, hipMemcpyHostToDevice));
  for (int w = 0; w < 2; ++w) {
    g->tag_ids[w].reset();
    g->n_tag_ids[w] = (int64_t)T.tags_glob[w].size();
    if (!T.tags_glob[w].empty()) {
      ICHK(g, g->tag_ids[w].alloc(T.tags_glob[w].size()));
      ICHK(g, hipMemcpy(g->tag_ids[w].get(), T.tags_glob[w].data(), sizeof(int64_t) * T.tags_glob[w].size(), hipMemcpyHostToDevice));
    }
  }
  g->tag_item_idx.reset();
  if (g->n_tag_ids[1] > 0) {
    ICHK(g, g->tag_item_idx.alloc((size_t)g->n_tag_ids[1]));
    ITRY(launch(g, g->n_tag_ids[1], index_of_ids_kernel, g->tag_ids[1].get(), g->n_tag_ids[1], g->ids[1].get(), n_items, g->tag_item_idx.get()));
  }
  ICHK(g, hipStreamSynchronize(g->stream));
  g->sharded = true;
  g->slice_begin[0] = user_base;
  g->slice_rows[0] = x_rows;
  g->slice_nnz[0] = x_nnz;
  g->n_users = n_users;
  g->n_items = n_items;
  return MALS_OK;
}

// f. entries to the owners of their items; every member's item slice; the global tables in place of its own
int shard_redistribute_entries(ShardCtx& c, ShardTables& T, const int64_t* bounds_x, const int64_t* bounds_y) {
  const std::vector<int64_t> yspl(bounds_y + 1, bounds_y + c.world);
  ShardRuns R(c.nl);
  ITRY(shard_redistribute(c, R, false, [&](int i, std::vector<int64_t>* cnt) { return shard_split_entries(c, i, T, yspl, bounds_x[c.ops->ranks[i]], R, cnt); }));
  std::vector<int> rcs((size_t)c.nl, MALS_OK);
  for (int i = 0; i < c.nl; ++i) {
    const int r = c.ops->ranks[i];
    int rc = shard_build_item_slice(c, i, R, bounds_y[r], bounds_y[r + 1] - bounds_y[r]);
    if (!rc) rc = shard_install_tables(c, i, T, bounds_x[r]);
    rcs[(size_t)i] = rc;
  }
  return shard_agree(c, rcs);
}

// the global entry count on every member
int shard_total_entries(ShardCtx& c) {
  std::vector<std::vector<int64_t>> per = shard_slots(c, 1);
  for (int i = 0; i < c.nl; ++i) per[(size_t)i][0] = c.g[i]->slice_nnz[0];
  std::vector<int64_t> tot;
  ITRY(shard_allreduce(c, per, 0, &tot));
  for (int i = 0; i < c.nl; ++i) c.g[i]->nnz = tot[0];
  return MALS_OK;
}

int shard_finish_impl(ShardCtx& c, int64_t* bounds_x, int64_t* bounds_y) {
  const int W = c.world;
  ITRY(shard_agree_text(c));                                   // a
  for (int i = 0; i < c.nl; ++i) {
    c.g[i]->free_results();
    c.g[i]->split_ms = c.g[i]->split_bytes = 0.0;
    c.g[i]->work_at_replicas = -1;
  }
  std::vector<int64_t> spl;
  ITRY(shard_user_splitters(c, &spl));                         // b
  ITRY(shard_redistribute_records(c, spl));                    // c
  ITRY(shard_finish_members(c));                               // d
  ShardTables T;                                               // e
  ITRY(shard_table_sizes(c, T));
  bounds_x[0] = 0;   // users: ranks own ascending id ranges, so the concatenation of their tables is the ascending table
  for (int r = 0; r < W; ++r) bounds_x[r + 1] = bounds_x[r] + T.sizes[(size_t)r * 4];
  T.n_users = bounds_x[W];
  ITRY(shard_merge_item_tables(c, T));
  ITRY(shard_gather_table(c, T.column(W, 0), [](mals_ingest g) { return g->ids[0].get(); }, &T.users_glob));
  for (int w = 0; w < 2; ++w) {   // tags: union of every rank's sets
    std::vector<int64_t>& tags = T.tags_glob[w];
    std::vector<DeviceBuffer<int64_t>> gathered;
    ITRY(shard_gather_table(c, T.column(W, 2 + w), [w](mals_ingest g) { return g->tag_ids[w].get(); }, &gathered, &tags));
    std::sort(tags.begin(), tags.end());
    tags.erase(std::unique(tags.begin(), tags.end()), tags.end());
  }
  ITRY(shard_plan_item_bounds(c, T, bounds_y));                // f
  ITRY(shard_redistribute_entries(c, T, bounds_x, bounds_y));
  return shard_total_entries(c);
}

}  // namespace

int malsi_ingest_shard_finish(mals_ingest* ingests, const malsi_group_ops* ops, int64_t* bounds_x, int64_t* bounds_y) {
  ShardCtx c{ingests, ops, ops->world, ops->n_local, std::string()};
  const int rc = shard_finish_impl(c, bounds_x, bounds_y);
  if (rc != MALS_OK) {
    for (int i = 0; i < c.nl; ++i) {
      mals_ingest g = ingests[i];
      if (!c.comm_msg.empty()) g->err = c.comm_msg;
      else if (g->err.empty()) g->err = "another rank reported status " + std::to_string(rc);
      (void)hipSetDevice(g->device);
      g->free_results();
      g->release_work();
      g->spent = true;   // its records are gone: a new ingest starts over
    }
    return rc;
  }
  for (int i = 0; i < c.nl; ++i) {
    ingests[i]->finished = true;
    ingests[i]->spent = true;
  }
  return MALS_OK;
}

int malsi_ingest_spent(mals_ingest g) { return g && g->spent ? 1 : 0; }

void malsi_ingest_note_replicas(mals_ingest g) {
  int64_t w = 0;
  (void)mals_ingest_memory(g, &w, nullptr, nullptr, nullptr, nullptr);
  g->work_at_replicas = w;
}

extern "C" {

int mals_ingest_slice(mals_ingest g, int side, int64_t* row_begin, int64_t* n_rows) {
  if (!g) return MALS_INVALID_ARG;
  if (side != MALS_SIDE_X && side != MALS_SIDE_Y) return fail(g, MALS_INVALID_ARG, "side must be MALS_SIDE_X or _Y");
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  if (row_begin) *row_begin = g->sharded ? g->slice_begin[side] : 0;
  if (n_rows) *n_rows = g->sharded ? g->slice_rows[side] : side == MALS_SIDE_X ? g->n_users : g->n_items;
  return MALS_OK;
}

int mals_ingest_memory(mals_ingest g, int64_t* work_bytes, int64_t* result_bytes, int64_t* work_bytes_at_replicas, double* split_ms,
                       double* split_bytes) {
  if (!g) return MALS_INVALID_ARG;
  int64_t w = 0, r = 0;
  auto add = [](int64_t& acc, const auto& b) { acc += (int64_t)(b.capacity() * sizeof(*b.get())); };
  add(w, g->d_user); add(w, g->d_item); add(w, g->d_value); add(w, g->d_kind);
  for (int b = 0; b < mals_ingest_s::N_WS; ++b) add(w, g->ws[b]);
  add(w, g->d_text); add(w, g->d_carry); add(w, g->t_block_counts); add(w, g->t_tile_sums); add(w, g->t_starts); add(w, g->t_flag);
  add(w, g->t_defer); add(w, g->t_status); add(w, g->t_user); add(w, g->t_item); add(w, g->t_value); add(w, g->t_counters);
  add(w, g->d_tags[0]); add(w, g->d_tags[1]);
  for (int sd = 0; sd < 2; ++sd) {
    add(r, g->ids[sd]); add(r, g->ptr[sd]); add(r, g->col[sd]); add(r, g->val[sd]); add(r, g->tag_ids[sd]);
  }
  add(r, g->known_ptr); add(r, g->known_idx); add(r, g->tag_item_idx);
  if (work_bytes) *work_bytes = w;
  if (result_bytes) *result_bytes = r;
  if (work_bytes_at_replicas) *work_bytes_at_replicas = g->work_at_replicas;
  if (split_ms) *split_ms = g->split_ms;
  if (split_bytes) *split_bytes = g->split_bytes;
  return MALS_OK;
}

}  // extern "C"
