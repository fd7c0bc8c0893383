// topn_host.h -- host side of top-N scoring (mals_recommend*, include/myrrix_als.h; kernels and the argument for
// exactness in topn_kernels.h).  Included by mals_serving.hip inside its anonymous namespace, after ServingState.
#pragma once

constexpr int TOPN_SLOTS = 6;  // passes in flight, each on its own stream (3 -> 6: 3-4 % at 64-128 queries per pass, nothing at 240)

// Everything one pass of the filter path owns.  Passes are independent (Y, X and the known items are only read), so
// pass p runs on stream p % TOPN_SLOTS: while the streaming filter kernel of one pass has the chip, the small kernels
// either side of it (prepare / sample / threshold of the next pass, scatter / rescore / final of the previous one) run
// beside it instead of in its shadow -- serialised on one stream they and the launch gaps between them were two thirds
// of a pass.
struct TopnSlot {
  Stream stream;
  Event ev;
  // inputs of the pass: ONE device block, the image of the slot's pinned block (one copy); the pointers below are views
  // into it
  DeviceBuffer<uint8_t> d_in;
  PinnedBuffer<uint8_t> h_in;         // input block (offsets, rows, vectors, exclusion lists)
  const float* d_vecs = nullptr;      // [n_vecs][k] (caller's vectors) or X itself (model users: rows d_vrow)
  const int64_t* d_vrow = nullptr;    // vector v = row d_vrow[v] of d_vecs; NULL: row v
  const int32_t* d_vptr = nullptr;    // [nq + 1]
  const int64_t* d_rows = nullptr;    // [nq]: local row of the query's user (known items), -1 = none
  const int64_t* d_excl_ptr = nullptr;
  const int64_t* d_excl_idx = nullptr;
  DeviceBuffer<float> d_tau, d_bmax;  // thresholds; the sample's bucket maxima [queries][16 x TOPN_SAMPLE_GROUPS] ...
  DeviceBuffer<uint32_t> d_bidx;      // ... and the items that attain them
  DeviceBuffer<unsigned> d_count;
  DeviceBuffer<uint32_t> d_cand;
  DeviceBuffer<uint64_t> d_pairs;
  DeviceBuffer<bf16x8> d_img;         // the pass's queries as split bf16 MFMA operands (topn_prepare_kernel)
  DeviceBuffer<unsigned> d_wcount;    // hits per wave of the filter kernel, [n_waves] + one overflow word
  DeviceBuffer<uint2> d_whits;        // [n_waves][TOPN_WAVE_CAP] (item, query)
  DeviceBuffer<double> d_qn;          // cosine mode: the exact norms of the pass's query vectors ...
  DeviceBuffer<uint32_t> d_qflag;     // ... and per query 0 / 1 (answered empty) / 2 (dense path), topn_prepare_kernel<true>
  DeviceBuffer<uint64_t> d_vsig;      // candidate filter: the bit signatures of the pass's query vectors (lsh_sign_vectors_kernel)
  PinnedBuffer<uint8_t> h_stage;      // the pass's results (TopnStage: topn_final_kernel writes them there), decoded while later
                                      // passes run
};

struct TopnWorkspace {
  TopnSlot slot[TOPN_SLOTS];
  Event ev_begin;  // the caller's stream at the start of the call: every slot stream waits for it
  // dense path
  DeviceBuffer<float> d_scores;
  DeviceBuffer<uint32_t> d_sel;
  DeviceBuffer<TopnState> d_state;
  DeviceBuffer<unsigned> d_hist;
};

void topn_free(mals_handle h) {
  TopnWorkspace* w = h->serving->tn_ws;
  if (!w) return;
  for (TopnSlot& s : w->slot)
    if (s.stream) (void)hipStreamSynchronize(s.stream);
  delete w;   // its buffers, events and streams
  h->serving->tn_ws = nullptr;
}

struct TopnOut {
  int64_t* items;
  float* scores;
  int32_t* n;
};
// what one call asks for (host pointers)
struct TopnRequest {
  int n_queries = 0, how_many = 0;
  const int64_t* user_idx = nullptr;     // model users: query q's single vector is X[user_idx[q]] ...
  bool skip_known = false;               // ... and its user's known items are skipped
  const float* vectors = nullptr;        // or caller's vectors: [n_vectors][k],
  const int64_t* vec_ptr = nullptr;      //   query q owns vectors [vec_ptr[q], vec_ptr[q+1]) (NULL: one each)
  const int64_t* excl_ptr = nullptr;     // optional per-query exclusion lists (item indices)
  const int64_t* excl_idx = nullptr;
  int64_t* item_idx_out = nullptr;
  float* score_out = nullptr;
  int32_t* n_out = nullptr;
  // a coalesced pass of the serving front (below): queries of several callers -- every query has its own output block and
  // its own "skip the known items" flag
  const TopnOut* out_q = nullptr;
  const uint8_t* skip_known_q = nullptr;
  // mostSimilarItems (kind TOPN_KIND_SCORE, cosine): the query vectors are rows of Y, vector v = Y[item_rows[v]] (grouped by
  // vec_ptr); the caller passes the query items as the exclusion lists (MostSimilarItemIterator.java:81-85)
  const int64_t* item_rows = nullptr;
  bool cosine = false;
  int kind = 0;                          // TOPN_KIND_*
  // recommendedBecause (TOPN_KIND_BECAUSE): query q = (user because_user[q], item item_rows[q]), candidates = the user's
  // known items
  const int64_t* because_user = nullptr;
  // similarityToItem (TOPN_KIND_SIMILARITY_TO): n_queries items item_rows[], against to_item, into sim_out
  int64_t to_item = 0;
  float* sim_out = nullptr;
  // a write or fold-in read of foldin_host.h (TOPN_KIND_CALL): runs alone on the handle, in queue order
  const std::function<int()>* call = nullptr;
  // a rescored call (kind TOPN_KIND_SCORE, not cosine): the rescorer named by the caller, and what the pass reads of it (the
  // state it had when the call's turn came: a mals_rescorer_set_* is an exclusive ticket of the front)
  const mals_rescorer_s* rescorer = nullptr;
  const TopnRescore* rs = nullptr;
  // mals_most_similar_items_rescored (cosine with a rescorer): MALS_SIMILAR_* of the call, how the pair rescorer reads its filter
  int32_t flags = 0;
  // per query: 1 = its result is not finite (RecommendIterator.java:105) -- the query's caller fails, the others are answered.
  // NULL: the whole request fails
  uint8_t* bad_q = nullptr;
};
constexpr const char* TOPN_BAD_VALUE = "Bad recommendation value: a non-finite score (non-finite factors; RecommendIterator.java:105 throws IllegalStateException)";
constexpr const char* TOPN_BAD_SIMILARITY = "Bad similarity value: a non-finite rescored similarity (MostSimilarItemIterator.java:117 throws IllegalStateException)";
inline const char* topn_bad_value(const TopnRequest& rq) { return rq.cosine ? TOPN_BAD_SIMILARITY : TOPN_BAD_VALUE; }
enum { TOPN_KIND_SCORE = 0, TOPN_KIND_BECAUSE = 1, TOPN_KIND_SIMILARITY_TO = 2, TOPN_KIND_CALL = 3 };

inline TopnOut topn_out(const TopnRequest& rq, size_t qq) {
  if (rq.out_q) return rq.out_q[qq];
  return {rq.item_idx_out + qq * (size_t)rq.how_many, rq.score_out + qq * (size_t)rq.how_many, rq.n_out ? rq.n_out + qq : nullptr};
}

struct TopnPass {
  int q0 = 0, nq = 0;
  int64_t v0 = 0, n_vecs = 0;
  bool have_rows = false, have_excl = false;
};

struct TopnCand {
  uint32_t key;
  int64_t idx;
};
// false: a non-finite score among the results (the reference: Preconditions.checkState(isFinite(result)), RecommendIterator.java:105)
bool topn_emit(std::vector<TopnCand>& cand, int how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out) {
  // best score first; equal scores in ascending item index (the reference's order among ties is its hash order)
  std::sort(cand.begin(), cand.end(), [](const TopnCand& a, const TopnCand& b) { return a.key != b.key ? a.key > b.key : a.idx < b.idx; });
  const int n = (int)std::min<size_t>(cand.size(), (size_t)how_many);
  if (n_out) *n_out = n;
  for (int j = 0; j < how_many; ++j) {
    if (j < n) {
      item_idx_out[j] = cand[(size_t)j].idx;
      score_out[j] = key_score(cand[(size_t)j].key);
    } else {
      item_idx_out[j] = -1;
      score_out[j] = -std::numeric_limits<float>::infinity();
    }
  }
  // (NaN sorts above +inf in score_key: a non-finite score, if there is one, is the first result)
  return n == 0 || std::isfinite(score_out[0]);
}

// The pass's vectors, offsets, known-item rows and exclusion lists on the device: assembled in the slot's pinned input
// block and sent with ONE asynchronous copy on `stream` (the host never waits for a pass that is still running; the slot's
// previous pass has been decoded before the slot is used again).
int topn_upload_pass(mals_handle h, TopnSlot& sl, hipStream_t stream, const TopnRequest& rq, TopnPass& ps) {
  const int k = h->cfg.features;
  SideState& x = h->side[MALS_SIDE_X];
  const bool own_vectors = !rq.user_idx && !rq.item_rows;
  if (rq.user_idx || !rq.vec_ptr) {
    ps.v0 = ps.q0;
    ps.n_vecs = ps.nq;
  } else {
    ps.v0 = rq.vec_ptr[ps.q0];
    ps.n_vecs = rq.vec_ptr[ps.q0 + ps.nq] - ps.v0;
  }
  // by-user queries whose known items the writes changed (foldin_host.h): the additions as exclusion lists beside the base
  // row; users with removals (or grown rows) drop the base row (rows[q] = -1) and exclude their whole list instead
  std::vector<int64_t> ov_ptr, ov_idx;
  std::vector<uint8_t> ov_drop;
  if (rq.user_idx && (rq.skip_known || rq.skip_known_q) && foldin_has_overlay(h)) {
    ov_ptr.assign(1, 0);
    ov_drop.assign((size_t)ps.nq, 0);
    for (int q = 0; q < ps.nq; ++q) {
      if (!rq.skip_known_q || rq.skip_known_q[ps.q0 + q]) {
        const size_t b = ov_idx.size();
        ov_drop[(size_t)q] = foldin_known_view(h, rq.user_idx[ps.q0 + q] - x.row_offset, ov_idx) ? 1 : 0;
        std::sort(ov_idx.begin() + (ptrdiff_t)b, ov_idx.end());
        ov_idx.erase(std::unique(ov_idx.begin() + (ptrdiff_t)b, ov_idx.end()), ov_idx.end());
      }
      ov_ptr.push_back((int64_t)ov_idx.size());
    }
  }
  const bool overlay = !ov_ptr.empty();
  const int64_t n_ex = overlay ? (int64_t)ov_idx.size() : (rq.excl_ptr && rq.excl_idx) ? rq.excl_ptr[ps.q0 + ps.nq] - rq.excl_ptr[ps.q0] : 0;
  // layout of the block (8-byte aligned pieces)
  const size_t o_vptr = 0, o_rows = o_vptr + 8 * ((TOPN_FILTER_QUERIES + 2) / 2), o_uidx = o_rows + 8 * TOPN_FILTER_QUERIES,
               o_eptr = o_uidx + 8 * TOPN_FILTER_QUERIES, o_vecs = o_eptr + 8 * (TOPN_FILTER_QUERIES + 1),
               o_eidx = o_vecs + ((own_vectors ? sizeof(float) * (size_t)ps.n_vecs * (size_t)k
                                               : rq.item_rows ? sizeof(int64_t) * (size_t)ps.n_vecs : 0) + 15) / 16 * 16,
               total = o_eidx + 8 * (size_t)n_ex;
  if (total > sl.h_in.capacity()) HIPCHK(h, sl.h_in.reserve(total + total / 2, stream));  // an earlier copy may still be reading the old block
  HIPCHK(h, sl.d_in.reserve(total + total / 2, stream));
  uint8_t* in = sl.h_in.get();
  int32_t* vptr = reinterpret_cast<int32_t*>(in + o_vptr);
  for (int q = 0; q <= ps.nq; ++q) vptr[q] = (rq.user_idx || !rq.vec_ptr) ? q : (int32_t)(rq.vec_ptr[ps.q0 + q] - ps.v0);
  ps.have_rows = ps.have_excl = false;
  sl.d_vptr = reinterpret_cast<const int32_t*>(sl.d_in.get() + o_vptr);
  sl.d_rows = reinterpret_cast<const int64_t*>(sl.d_in.get() + o_rows);
  sl.d_excl_ptr = reinterpret_cast<const int64_t*>(sl.d_in.get() + o_eptr);
  sl.d_excl_idx = reinterpret_cast<const int64_t*>(sl.d_in.get() + o_eidx);
  if (rq.user_idx) {
    std::memcpy(in + o_uidx, rq.user_idx + ps.q0, sizeof(int64_t) * (size_t)ps.nq);
    sl.d_vecs = x.F;
    sl.d_vrow = reinterpret_cast<const int64_t*>(sl.d_in.get() + o_uidx);
    if (rq.skip_known || rq.skip_known_q) {
      int64_t* rows = reinterpret_cast<int64_t*>(in + o_rows);
      for (int q = 0; q < ps.nq; ++q)
        rows[q] = (!rq.skip_known_q || rq.skip_known_q[ps.q0 + q]) && !(overlay && ov_drop[(size_t)q]) ? rq.user_idx[ps.q0 + q] - x.row_offset : -1;
      ps.have_rows = true;
    }
  } else if (rq.item_rows) {   // rows of Y (the replica is complete on every handle)
    std::memcpy(in + o_vecs, rq.item_rows + ps.v0, sizeof(int64_t) * (size_t)ps.n_vecs);
    sl.d_vecs = h->side[MALS_SIDE_Y].F;
    sl.d_vrow = reinterpret_cast<const int64_t*>(sl.d_in.get() + o_vecs);
    if (rq.because_user) {
      int64_t* rows = reinterpret_cast<int64_t*>(in + o_rows);
      for (int q = 0; q < ps.nq; ++q) rows[q] = rq.because_user[ps.q0 + q] - x.row_offset;
      ps.have_rows = true;
    }
  } else {
    std::memcpy(in + o_vecs, rq.vectors + ps.v0 * k, sizeof(float) * (size_t)ps.n_vecs * (size_t)k);
    sl.d_vecs = reinterpret_cast<const float*>(sl.d_in.get() + o_vecs);
    sl.d_vrow = nullptr;
  }
  if (n_ex > 0 && overlay) {
    std::memcpy(in + o_eptr, ov_ptr.data(), sizeof(int64_t) * (size_t)(ps.nq + 1));
    std::memcpy(in + o_eidx, ov_idx.data(), sizeof(int64_t) * (size_t)n_ex);
    ps.have_excl = true;
  } else if (n_ex > 0) {
    int64_t* eptr = reinterpret_cast<int64_t*>(in + o_eptr);
    for (int q = 0; q <= ps.nq; ++q) eptr[q] = rq.excl_ptr[ps.q0 + q] - rq.excl_ptr[ps.q0];
    std::memcpy(in + o_eidx, rq.excl_idx + rq.excl_ptr[ps.q0], sizeof(int64_t) * (size_t)n_ex);
    ps.have_excl = true;
  }
  HIPCHK(h, hipMemcpyAsync(sl.d_in.get(), in, total, hipMemcpyHostToDevice, stream));
  return MALS_OK;
}

// ---- the scoring variant of a pass ------------------------------------------------------------------------------------
// Which instantiations of the scoring kernels run a pass: derived once from (h, rq), turned into template arguments in one
// place (topn_dispatch), and the kernel arguments that go with it derived once per pass (topn_variant_args).
struct TopnVariant {
  bool cos;   // cosine to rows of Y (mostSimilarItems, recommendedBecause)
  bool rs;    // the caller's rescorer
  bool lsh;   // the candidate filter is built and this kind of call consults it
};
TopnVariant topn_variant(mals_handle h, const TopnRequest& rq) {
  return {rq.cosine, rq.rs != nullptr, h->lsh.H > 0 && rq.kind == TOPN_KIND_SCORE && !rq.cosine};
}

// f(COS, RS, LSH) with the variant as std::bool_constants: the six combinations the library is built for
template <class F>
auto topn_dispatch(const TopnVariant& v, F&& f) {
  assert(!(v.cos && v.lsh));   // no cosine call consults the candidate filter (the reference passes none to similarity)
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (v.cos && v.rs) return f(yes, yes, no);
  if (v.cos) return f(yes, no, no);
  if (v.rs && v.lsh) return f(no, yes, yes);
  if (v.rs) return f(no, yes, no);
  if (v.lsh) return f(no, no, yes);
  return f(no, no, no);
}

struct TopnVariantArgs {
  const double* qn;         // cosine: the exact norms of the pass's query vectors, else NULL
  uint32_t* qflag;          // cosine: the per-query flags of topn_prepare_kernel<true>, else NULL
  TopnRescore rs;           // rescored: what the pass reads of the rescorer, else the identity
  TopnImgTrailer trailer;   // rescored: the items' filter data behind the query image, else none
  int pair_flags;           // rescored cosine: TOPN_PAIR_* (= the call's MALS_SIMILAR_* flags), else 0
};
// (after the pass's sl.d_qn has its size: the pointer is taken here)
TopnVariantArgs topn_variant_args(const TopnVariant& v, const TopnSlot& sl, const TopnRequest& rq) {
  TopnVariantArgs a{nullptr, nullptr, TopnRescore(), TopnImgTrailer(), 0};
  if (v.cos) {
    a.qn = sl.d_qn.get();
    a.qflag = sl.d_qflag.get();
  }
  if (v.rs) {
    a.rs = *rq.rs;
    a.trailer = TopnImgTrailer{rq.rs->fdata, rq.rs->n_fdata, rq.rs->fdef};
    if (v.cos) a.pair_flags = a.rs.pair_flags = rq.flags;
  }
  return a;
}

// mals_similar_stats: which path answered the queries of mostSimilarItems calls (plain and rescored), counted where a pass
// decides it per query.  A query the filter hands to the dense path counts there only.
enum { TOPN_SIMILAR_FILTER = 0, TOPN_SIMILAR_DENSE = 1, TOPN_SIMILAR_EMPTY = 2, TOPN_SIMILAR_RESCORED = 3 };
void topn_similar_count(mals_handle h, int which, int n, bool rescored);

// the known-items CSR of a handle: knownItemIDs if the caller installed them, else the rows of R
struct TopnKnown {
  const int64_t* ptr;
  const int32_t* idx;
};
TopnKnown topn_known(mals_handle h) {
  const SideState& x = h->side[MALS_SIDE_X];
  return h->known_ptr ? TopnKnown{h->known_ptr, h->known_idx} : TopnKnown{x.row_ptr, x.col};
}

// ---- the candidate filter (mals_lsh_build; lsh_kernels.h) ---------------------------------------------------------------
// mals_recommend* and their rescored twins consult it (ServerRecommender.java:431-436, :555); mostSimilarItems,
// similarityToItem and recommendedBecause never do (the reference passes no candidate filter there).  A build is an exclusive
// ticket of the front: no pass is in flight while the state changes, so a pass reads it as it is when it is enqueued
// (TopnVariant::lsh).

// toBitSignature (LSH:169-190) of the pass's query vectors where they already are on the device -- rows of X, the uploaded
// block -- on `st`, no host round trip; *view = what the pass's kernels read of the filter.  img: the pass's query image (the
// streaming kernels find the view behind it), NULL for the dense path.
int topn_lsh_sign_pass(mals_handle h, TopnSlot& sl, hipStream_t st, const TopnPass& ps, bf16x8* img, TopnLsh* view) {
  LshState& l = h->lsh;
  HIPCHK(h, sl.d_vsig.reserve((size_t)std::max<int64_t>(ps.n_vecs, 1), st));
  view->isig = l.d_sig.get();
  view->n_signed = l.n_signed;
  view->vsig = sl.d_vsig.get();
  view->vptr = sl.d_vptr;
  view->mb = l.mb;
  hipLaunchKernelGGL(lsh_sign_vectors_kernel, dim3((unsigned)std::max<int64_t>(ps.n_vecs, 1)), dim3(64), 0, st, sl.d_vecs, sl.d_vrow, (int)ps.n_vecs,
                     h->cfg.features, l.d_mean.get(), l.d_mask.get(), l.H, sl.d_vsig.get(),
                     img ? reinterpret_cast<TopnLsh*>(img + TOPN_IMG_LSH_AT) : nullptr, *view);
  HIPCHK(h, hipGetLastError());
  return MALS_OK;
}

// ---- dense path: exact scores of every item (on the caller's stream, with slot 0's input block; nothing else of the
// workspace is in flight when it runs) -------------------------------------------------------------------------------
int topn_select_threshold(mals_handle h, const float* d_scores, int64_t n_row, int nq, int how_many, TopnState* d_st, unsigned* d_hist,
                          unsigned* slabs_out) {
  hipLaunchKernelGGL(topn_init_kernel, dim3((unsigned)((nq * 256 + 255) / 256)), dim3(256), 0, h->stream, d_st, d_hist, nq, how_many);
  const unsigned slabs = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_row + 4095) / 4096, (int64_t)(h->n_cu * 8 + nq - 1) / nq));
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(topn_hist_kernel, dim3(slabs, (unsigned)nq), dim3(256), 0, h->stream, d_scores, n_row, pass, d_st, d_hist);
    hipLaunchKernelGGL(topn_pick_kernel, dim3((unsigned)nq), dim3(256), 0, h->stream, d_st, d_hist, pass);
  }
  HIPCHK(h, hipGetLastError());
  *slabs_out = slabs;
  return MALS_OK;
}

int topn_pass_dense(mals_handle h, TopnWorkspace* w, TopnSlot& sl, const TopnRequest& rq, const TopnPass& ps) {
  SideState& y = h->side[MALS_SIDE_Y];
  const int k = h->cfg.features, nq = ps.nq, how_many = rq.how_many;
  const int64_t n_items = y.n_total;
  const int cap_ties = 1024;
  const size_t per_q = 2 * ((size_t)how_many + cap_ties);
  HIPCHK(h, w->d_scores.reserve((size_t)TOPN_MAX_QUERIES * (size_t)n_items, h->stream));
  HIPCHK(h, w->d_sel.reserve((size_t)TOPN_MAX_QUERIES * per_q, h->stream));
  if (!w->d_state.get()) HIPCHK(h, w->d_state.alloc(TOPN_MAX_QUERIES));
  if (!w->d_hist.get()) HIPCHK(h, w->d_hist.alloc(256 * TOPN_MAX_QUERIES));
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_items + 63) / 64, (int64_t)h->n_cu * 8));
  const TopnVariant v = topn_variant(h, rq);
  if (v.cos && rq.kind == TOPN_KIND_SCORE) topn_similar_count(h, TOPN_SIMILAR_DENSE, nq, v.rs);
  if (v.cos) {
    HIPCHK(h, sl.d_qn.reserve((size_t)std::max<int64_t>(ps.n_vecs, 1), h->stream));
    hipLaunchKernelGGL(topn_qnorm_kernel, dim3((unsigned)((ps.n_vecs + 63) / 64)), dim3(64), 0, h->stream, sl.d_vecs, sl.d_vrow, (int)ps.n_vecs, k,
                       sl.d_qn.get());
  }
  const TopnVariantArgs va = topn_variant_args(v, sl, rq);
  topn_dispatch(v, [&](auto COS, auto RS, auto) {
    hipLaunchKernelGGL((topn_exact_dense_kernel<COS, RS>), dim3(grid), dim3(256), sizeof(float) * 64 * (size_t)(k + 1),
                       h->stream, y.F, n_items, k, sl.d_vecs, sl.d_vrow, sl.d_vptr, nq, w->d_scores.get(), va.qn, va.rs);
  });
  if (ps.have_rows) {
    const TopnKnown kn = topn_known(h);
    hipLaunchKernelGGL(topn_mask_kernel, dim3(64, (unsigned)nq), dim3(256), 0, h->stream, kn.ptr, kn.idx, sl.d_rows, nq, 1, n_items, w->d_scores.get());
  }
  if (ps.have_excl)
    hipLaunchKernelGGL(topn_exclude_kernel, dim3(64, (unsigned)nq), dim3(256), 0, h->stream, sl.d_excl_ptr, sl.d_excl_idx, nq, n_items, 1, n_items,
                       w->d_scores.get());
  if (h->tag_bits)
    hipLaunchKernelGGL(topn_mask_tags_kernel, dim3((unsigned)(((n_items + 31) / 32 + 255) / 256)), dim3(256), 0, h->stream, h->tag_bits.get(), nq, n_items,
                       w->d_scores.get());
  if (v.lsh) {   // the non-candidates of every query (LSH:193-216)
    TopnLsh lv;
    if (int rc = topn_lsh_sign_pass(h, sl, h->stream, ps, nullptr, &lv)) return rc;
    hipLaunchKernelGGL(lsh_mask_dense_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_items + 255) / 256, 1024)), (unsigned)nq), dim3(256), 0,
                       h->stream, lv, nq, n_items, w->d_scores.get());
    h->lsh.q_dense.fetch_add(nq);
  }
  unsigned slabs = 1;
  if (int rc = topn_select_threshold(h, w->d_scores.get(), n_items, nq, how_many, w->d_state.get(), w->d_hist.get(), &slabs)) return rc;
  hipLaunchKernelGGL(topn_collect_kernel, dim3(slabs, (unsigned)nq), dim3(256), 0, h->stream, w->d_scores.get(), n_items, w->d_state.get(), how_many, cap_ties,
                     w->d_sel.get());
  HIPCHK(h, hipGetLastError());
  std::vector<uint32_t> out((size_t)nq * per_q);
  std::vector<TopnState> st((size_t)nq);
  HIPCHK(h, hipMemcpyAsync(out.data(), w->d_sel.get(), sizeof(uint32_t) * out.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(st.data(), w->d_state.get(), sizeof(TopnState) * (size_t)nq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::vector<float> row;
  std::vector<TopnCand> cand;
  for (int q = 0; q < nq; ++q) {
    const uint32_t* o = &out[(size_t)q * per_q];
    const uint32_t above = st[(size_t)q].above, ties_total = st[(size_t)q].ties;
    const uint32_t ties_stored = std::min<uint32_t>(ties_total, (uint32_t)cap_ties);
    const uint32_t need_ties = above < (uint32_t)how_many ? (uint32_t)how_many - above : 0;
    cand.clear();
    if (above > (uint32_t)how_many || (ties_stored < ties_total && need_ties > 0)) {
      // more ties at the N-th score than the selection buffer holds (e.g. a block of identical items): which of
      // them have the lowest indices is not known from an unordered subset -- resolve this query from its score row
      row.resize((size_t)n_items);
      HIPCHK(h, hipMemcpy(row.data(), w->d_scores.get() + (size_t)q * (size_t)n_items, sizeof(float) * (size_t)n_items, hipMemcpyDeviceToHost));
      const uint32_t ninf = score_key(-std::numeric_limits<float>::infinity());
      for (int64_t i = 0; i < n_items; ++i) {
        const uint32_t kk = score_key(row[(size_t)i]);
        if (kk > ninf && kk >= st[(size_t)q].prefix) cand.push_back({kk, i});
      }
    } else {
      for (uint32_t p = 0; p < above; ++p) cand.push_back({o[2 * p + 1], (int64_t)o[2 * p]});
      for (uint32_t p = 0; p < ties_stored; ++p) cand.push_back({o[2 * (how_many + p) + 1], (int64_t)o[2 * (how_many + p)]});
    }
    const TopnOut o_q = topn_out(rq, (size_t)(ps.q0 + q));
    if (!topn_emit(cand, how_many, o_q.items, o_q.scores, o_q.n)) {
      if (!rq.bad_q) return fail(h, MALS_INVALID_ARG, topn_bad_value(rq));
      rq.bad_q[ps.q0 + q] = 1;   // this query's caller fails; the rest of the pass is answered
    }
  }
  return MALS_OK;
}

// ---- filter path ------------------------------------------------------------------------------------------------------
// query tiles per pass the LDS image of the split query operands allows (64 KB): S steps x NT tiles x 2 KB
int topn_max_tiles(int S) { return S == 1 ? 16 : S == 2 ? 15 : S == 3 ? 10 : 7; }

constexpr int TOPN_WAVE_CAP = 2048;  // hits a wave of the filter kernel can record (expected: a hundred)

// the slot's overflow word: behind its padded per-query counters
unsigned* topn_overflow_word(const TopnSlot& sl) { return sl.d_count.get() + (size_t)TOPN_FILTER_QUERIES * TOPN_COUNT_STRIDE; }

// topn_stream_kernel: QT = query tiles per wave, 4 QT per workgroup, LM = its load mode.  MODE 0: *n_out = workgroups of the
// sample (16 buckets each); MODE 1: *n_out = waves of the filter (one hit list each).
// RS: the rescored instantiations (the rescorer's per-item data: behind the query image, topn_prepare_kernel<false, true>)
template <int S, int QT, int MODE, int LM, bool COS, bool RS, bool LSH>
int topn_launch_stream_LM(mals_handle h, TopnSlot& sl, const float* Y, int64_t n_items, int k, int nq, int tile_stride, int cap, int* n_out) {
  constexpr auto kernel = topn_stream_kernel<S, QT, MODE, LM, COS, RS, LSH>;   // asked for its occupancy and launched: the same one
  const int64_t tiles = (n_items + 16 * (int64_t)tile_stride - 1) / (16 * (int64_t)tile_stride);
  const int64_t stages = (tiles + 3) / 4;
  // resident workgroups per CU: what the instantiation's registers and LDS (two buffers of 4 (S + 1) KB) allow, asked once
  static int per_cu_cached = 0;
  if (!per_cu_cached) {
    int nb = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, 0);
    per_cu_cached = (e == hipSuccess && nb > 0) ? std::min(nb, 6) : 2;
  }
  int per_cu = per_cu_cached;
  if (const char* e = std::getenv("MALS_TOPN_BLOCKS_PER_CU")) per_cu = std::max(1, std::atoi(e));
  // the filter is a persistent grid; the sample's workgroups each keep 16 buckets per query
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(stages, MODE == 0 ? TOPN_SAMPLE_GROUPS : (int64_t)h->n_cu * per_cu));
  if (MODE == 1) {
    const size_t nw = (size_t)grid * 4;
    if (nw * TOPN_WAVE_CAP > sl.d_whits.capacity() || nw + 1 > sl.d_wcount.capacity()) {
      HIPCHK(h, hipStreamSynchronize(sl.stream));
      sl.d_whits.reset();
      sl.d_wcount.reset();
      HIPCHK(h, sl.d_whits.alloc(nw * TOPN_WAVE_CAP));
      HIPCHK(h, sl.d_wcount.alloc(nw + 1));
    }
    *n_out = (int)nw;
  } else {
    *n_out = (int)grid;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, sl.stream, Y, n_items, k, sl.d_img.get(), nq, tile_stride, sl.d_bmax.get(), sl.d_bidx.get(),
                     sl.d_tau.get(), TOPN_WAVE_CAP, sl.d_wcount.get(), sl.d_whits.get(), cap, sl.d_count.get(), sl.d_cand.get(), topn_overflow_word(sl));
  HIPCHK(h, hipGetLastError());
  return MALS_OK;
}
// topn_stream_kernel's load mode: what the feature count allows
template <int S, int QT, int MODE, bool COS, bool RS, bool LSH>
int topn_launch_stream_QT(mals_handle h, TopnSlot& sl, const float* Y, int64_t n_items, int k, int nq, int tile_stride, int cap, int* n_out) {
#define MALS_TOPN_LM(LM) return topn_launch_stream_LM<S, QT, MODE, LM, COS, RS, LSH>(h, sl, Y, n_items, k, nq, tile_stride, cap, n_out)
  if (k == 32 * S) MALS_TOPN_LM(1);
  if ((k & 3) == 0) MALS_TOPN_LM(2);
  if ((k & 1) == 0) MALS_TOPN_LM(3);
  MALS_TOPN_LM(0);
#undef MALS_TOPN_LM
}
// the pass's variant, features and query tiles -> the instantiation
template <int MODE>
int topn_launch_stream(mals_handle h, TopnSlot& sl, const TopnVariant& v, int S, int nt, const float* Y, int64_t n_items, int k, int nq, int tile_stride,
                       int cap, int* n_out) {
  const int qt = (nt + 3) / 4;
  return topn_dispatch(v, [&](auto COS, auto RS, auto LSH) -> int {
#define MALS_TOPN_STREAM(SS, QQ) return topn_launch_stream_QT<SS, QQ, MODE, COS, RS, LSH>(h, sl, Y, n_items, k, nq, tile_stride, cap, n_out)
    switch (S) {
      case 1:
        if (qt <= 1) MALS_TOPN_STREAM(1, 1);
        if (qt == 2) MALS_TOPN_STREAM(1, 2);
        if (qt == 3) MALS_TOPN_STREAM(1, 3);
        MALS_TOPN_STREAM(1, 4);
      case 2:
        if (qt <= 1) MALS_TOPN_STREAM(2, 1);
        if (qt == 2) MALS_TOPN_STREAM(2, 2);
        if (qt == 3) MALS_TOPN_STREAM(2, 3);
        MALS_TOPN_STREAM(2, 4);
      case 3:  // at most 10 query tiles per pass
        if (qt <= 1) MALS_TOPN_STREAM(3, 1);
        if (qt == 2) MALS_TOPN_STREAM(3, 2);
        MALS_TOPN_STREAM(3, 3);
      default:  // at most 7
        if (qt <= 1) MALS_TOPN_STREAM(4, 1);
        MALS_TOPN_STREAM(4, 2);
    }
#undef MALS_TOPN_STREAM
  });
}

// The pinned result block of a pass, [capacity][how_many] (key, ~index) pairs | [capacity] counts | [capacity] taus | an
// overflow word: topn_final_kernel writes it (topn_launch_final), the host decodes it, and both find the pieces here.
struct TopnStage {
  uint8_t* base;
  size_t o_count, o_tau, o_overflow;
  TopnStage(uint8_t* block, int capacity, int how_many)
      : base(block), o_count(sizeof(uint64_t) * (size_t)capacity * (size_t)how_many), o_tau(o_count + sizeof(unsigned) * (size_t)capacity),
        o_overflow(o_tau + sizeof(float) * (size_t)capacity) {}
  uint64_t* pairs() const { return reinterpret_cast<uint64_t*>(base); }
  unsigned* count() const { return reinterpret_cast<unsigned*>(base + o_count); }
  float* tau() const { return reinterpret_cast<float*>(base + o_tau); }
  unsigned* overflow() const { return reinterpret_cast<unsigned*>(base + o_overflow); }
  size_t bytes() const { return o_overflow + 16; }
};
// one place of the block's pairs; false: empty (the query has fewer results than how_many)
inline bool topn_decode_pair(uint64_t pr, TopnCand* c) {
  if (pr == 0) return false;
  *c = {(uint32_t)(pr >> 32), (int64_t)(0xffffffffu - (uint32_t)pr)};
  return true;
}

struct TopnFilterPlan {
  int S, cap, cap_pad, tile_stride;
  size_t stage_bytes;
};
TopnFilterPlan topn_plan(mals_handle h, int how_many) {
  TopnFilterPlan p;
  const int64_t n_items = h->side[MALS_SIDE_Y].n_total;
  p.S = (h->cfg.features + 31) / 32;
  p.cap = 48 * how_many + 2048;
  p.cap_pad = 1;
  while (p.cap_pad < p.cap) p.cap_pad <<= 1;
  // sample items: expected candidates per query = how_many x stride, spread like a negative binomial (sigma = mean / sqrt(N)).
  // An eighth of the items: the sample kernel keeps only bucket maxima, so it costs an eighth of a filter pass whatever the
  // catalogue, and every candidate less is less hit bookkeeping in the filter, less to scatter and rescore (16384 -> 131072 at
  // a million items: 1.4x the queries per second).  A sample that does NOT grow with the catalogue lets the candidates grow
  // with it instead: at 10M items a 131072-item sample put every fourth pass of 240 queries over its candidate buffers.
  int64_t target = std::max<int64_t>(512 * (int64_t)how_many, std::max<int64_t>(16384, n_items / 8));
  if (const char* e = std::getenv("MALS_TOPN_SAMPLE_ITEMS")) target = std::max<int64_t>(1024, std::atoll(e));  // tuning override
  p.tile_stride = (int)std::max<int64_t>(1, n_items / target);
  p.stage_bytes = TopnStage(nullptr, TOPN_FILTER_QUERIES, how_many).bytes();
  return p;
}

// exact scores of the candidates in sl.d_cand into sl.d_pairs (the known items `kn` of the rows d_rows, the exclusion lists and
// the tag items dropped), and from there the N best of every query into the result block `o`
void topn_launch_rescore(mals_handle h, TopnSlot& sl, hipStream_t st, const TopnVariant& v, const TopnVariantArgs& va, int nq, int cap, const TopnKnown& kn,
                         const int64_t* d_rows, const int64_t* d_eptr, const int64_t* d_eidx) {
  const int k = h->cfg.features;
  topn_dispatch(v, [&](auto COS, auto RS, auto) {
    hipLaunchKernelGGL((topn_rescore_kernel<COS, RS>), dim3(8, (unsigned)nq), dim3(64), sizeof(float) * 64 * (size_t)(k + 1), st, h->side[MALS_SIDE_Y].F, k,
                       sl.d_vecs, sl.d_vrow, sl.d_vptr, sl.d_count.get(), cap, sl.d_cand.get(), kn.ptr, kn.idx, d_rows, d_eptr, d_eidx, h->tag_bits.get(),
                       sl.d_pairs.get(), topn_overflow_word(sl), va.qn, h->side[MALS_SIDE_Y].n_total, va.rs);
  });
}
void topn_launch_final(TopnSlot& sl, hipStream_t st, int nq, int cap, int how_many, const TopnStage& o) {
  hipLaunchKernelGGL(topn_final_kernel, dim3((unsigned)nq), dim3(256), sizeof(uint64_t) * (size_t)cap, st, sl.d_pairs.get(), sl.d_count.get(), cap, how_many,
                     o.pairs(), o.count(), sl.d_tau.get(), o.tau(), topn_overflow_word(sl), o.overflow());
}

// the kernels of one pass on the slot's stream (plain launches, or recorded into a graph while the stream is capturing)
int topn_pass_filter_launch(mals_handle h, TopnSlot& sl, const TopnRequest& rq, const TopnPass& ps, const TopnFilterPlan& p) {
  SideState& y = h->side[MALS_SIDE_Y];
  const int k = h->cfg.features, nq = ps.nq, how_many = rq.how_many;
  const int64_t n_items = y.n_total;
  const int nt = (nq + 15) / 16;
  hipStream_t st = sl.stream;
  const TopnVariant v = topn_variant(h, rq);
  const TopnVariantArgs va = topn_variant_args(v, sl, rq);
  const TopnKnown kn = topn_known(h);
  const int64_t* d_rows = ps.have_rows ? sl.d_rows : nullptr;
  const int64_t* d_eptr = ps.have_excl ? sl.d_excl_ptr : nullptr;
  const int64_t* d_eidx = ps.have_excl ? sl.d_excl_idx : nullptr;
  // 0. the queries as matrix operands (every tile an instantiation may touch: padding queries never produce a hit); in
  // cosine mode first the exact norms of the query vectors
  if (v.cos)
    hipLaunchKernelGGL(topn_qnorm_kernel, dim3((unsigned)((ps.n_vecs + 63) / 64)), dim3(64), 0, st, sl.d_vecs, sl.d_vrow, (int)ps.n_vecs, k, sl.d_qn.get());
  topn_dispatch(v, [&](auto COS, auto RS, auto) {
    hipLaunchKernelGGL((topn_prepare_kernel<COS, RS>), dim3(16), dim3(256), 0, st, sl.d_vecs, sl.d_vrow, sl.d_vptr, nq, k, p.S, sl.d_img.get(),
                       sl.d_count.get(), topn_overflow_word(sl), va.qn, va.qflag, va.trailer, va.pair_flags);
  });
  // the candidate filter: the signatures of the pass's vectors, and the pass's view of the filter behind the query image
  TopnLsh lv;
  if (v.lsh)
    if (int rc = topn_lsh_sign_pass(h, sl, st, ps, sl.d_img.get(), &lv)) return rc;
  // 1. sample: bucket maxima of the lower bounds of every tile_stride-th tile; 2. threshold (buckets won by known items dropped)
  int n_groups = 0, n_fw = 0;
  if (int rc = topn_launch_stream<0>(h, sl, v, p.S, nt, y.F, n_items, k, nq, p.tile_stride, p.cap, &n_groups)) return rc;
  if (v.lsh)   // buckets won by non-candidates of the queries of several vectors
    hipLaunchKernelGGL(lsh_drop_buckets_kernel, dim3(8, (unsigned)nq), dim3(256), 0, st, lv, 16 * (int64_t)n_groups, sl.d_bmax.get(), sl.d_bidx.get());
  hipLaunchKernelGGL(topn_threshold_kernel, dim3((unsigned)nq), dim3(1024), 0, st, sl.d_bmax.get(), sl.d_bidx.get(), n_groups, how_many, kn.ptr, kn.idx, d_rows,
                     d_eptr, d_eidx, n_items, p.tile_stride, h->tag_bits.get(), sl.d_tau.get(), va.qflag);
  // 3. filter, 4. exact scores of the hits (known items dropped), 5. the N best -- written straight into the slot's pinned
  // block (device-visible host memory: no copy kernel, no copy call)
  // (the filter's waves scatter their own hits into the per-query candidate lists: no kernel in between)
  if (int rc = topn_launch_stream<1>(h, sl, v, p.S, nt, y.F, n_items, k, nq, 1, p.cap, &n_fw)) return rc;
  topn_launch_rescore(h, sl, st, v, va, nq, p.cap, kn, d_rows, d_eptr, d_eidx);
  if (v.lsh)   // whatever the streaming tests let through
    hipLaunchKernelGGL(lsh_strike_pairs_kernel, dim3(2, (unsigned)nq), dim3(256), 0, st, lv, sl.d_count.get(), TOPN_COUNT_STRIDE, p.cap, sl.d_cand.get(),
                       sl.d_pairs.get());
  topn_launch_final(sl, st, nq, p.cap, how_many, TopnStage(sl.h_stage.get(), TOPN_FILTER_QUERIES, how_many));
  HIPCHK(h, hipGetLastError());
  return MALS_OK;
}

// enqueue one pass on its slot's stream; its results land in the slot's pinned block behind the slot's event
// the slot's fixed buffers, once
int topn_slot_alloc(mals_handle h, TopnSlot& sl) {
  if (!sl.d_bidx.get()) {   // (the last of them: all six exist)
    HIPCHK(h, sl.d_tau.alloc(TOPN_FILTER_QUERIES));
    HIPCHK(h, sl.d_count.alloc(TOPN_FILTER_QUERIES * TOPN_COUNT_STRIDE + 1));  // padded counters, then the overflow word
    HIPCHK(h, sl.d_img.alloc((size_t)TOPN_IMG_TOTAL));   // (+ the rescored filter's trailer, TopnImgTrailer, and the candidate filter's, TopnLsh)
    HIPCHK(h, sl.d_qflag.alloc(TOPN_FILTER_QUERIES));
    HIPCHK(h, sl.d_bmax.alloc(TOPN_FILTER_QUERIES * 16 * TOPN_SAMPLE_GROUPS));
    HIPCHK(h, sl.d_bidx.alloc(TOPN_FILTER_QUERIES * 16 * TOPN_SAMPLE_GROUPS));
  }
  return MALS_OK;
}

int topn_pass_filter_enqueue(mals_handle h, TopnSlot& sl, const TopnRequest& rq, const TopnPass& ps, const TopnFilterPlan& p) {
  hipStream_t st = sl.stream;
  if (int rc = topn_slot_alloc(h, sl)) return rc;
  HIPCHK(h, sl.d_pairs.reserve((size_t)TOPN_FILTER_QUERIES * (size_t)p.cap, st));
  HIPCHK(h, sl.d_cand.reserve((size_t)TOPN_FILTER_QUERIES * (size_t)p.cap, st));
  if (rq.cosine) HIPCHK(h, sl.d_qn.reserve((size_t)std::max<int64_t>(ps.n_vecs, 1), st));
  // the result block of THIS slot only: another slot may hold a finished pass that has not been decoded yet
  HIPCHK(h, sl.h_stage.reserve(p.stage_bytes, st));
  // (one graph launch per pass instead of nine kernel launches was tried: no faster -- the device, not the host's launch
  // calls, sets the pace even at 64 queries per pass)
  if (int rc = topn_pass_filter_launch(h, sl, rq, ps, p)) return rc;
  HIPCHK(h, hipEventRecord(sl.ev, st));
  return MALS_OK;
}

// decode a finished pass; failed[q] != 0: query q of the pass overflowed its candidate buffer or had a thin sample (the dense
// path answers it); all of them if a wave's hit list overflowed (whose hits are missing is not known)
int topn_pass_filter_finish(mals_handle h, TopnSlot& sl, const TopnRequest& rq, const TopnPass& ps, const TopnFilterPlan& p,
                            std::vector<uint8_t>& failed, bool* any_failed) {
  HIPCHK(h, hipEventSynchronize(sl.ev));
  const int how_many = rq.how_many;
  const TopnStage o(sl.h_stage.get(), TOPN_FILTER_QUERIES, how_many);
  const uint64_t* outp = o.pairs();
  const unsigned* count = o.count();
  const float* tau = o.tau();
  const unsigned wave_overflow = *o.overflow();
  const TopnVariant v = topn_variant(h, rq);
  const bool lsh = v.lsh;
  failed.assign((size_t)ps.nq, 0);
  *any_failed = false;
  for (int q = 0; q < ps.nq; ++q)
    if (wave_overflow != 0 || count[q] > (unsigned)p.cap || !(tau[q] > -std::numeric_limits<float>::infinity())) {
      failed[(size_t)q] = 1;
      *any_failed = true;
    }
  for (int q = 0; q < ps.nq; ++q) {
    if (failed[(size_t)q]) continue;
    const TopnOut o_q = topn_out(rq, (size_t)(ps.q0 + q));
    int n = 0;
    for (int j = 0; j < how_many; ++j) {
      TopnCand c;
      if (topn_decode_pair(outp[(size_t)q * how_many + j], &c)) {
        o_q.items[j] = c.idx;
        o_q.scores[j] = key_score(c.key);
        ++n;
      } else {
        o_q.items[j] = -1;
        o_q.scores[j] = -std::numeric_limits<float>::infinity();
      }
    }
    if (o_q.n) *o_q.n = n;
    if (lsh) h->lsh.q_filter.fetch_add(1);
    // (cosine: a query with a dead or filtered query item comes back with the threshold no candidate reaches)
    if (v.cos) topn_similar_count(h, tau[q] == TOPN_COS_DEAD_TAU ? TOPN_SIMILAR_EMPTY : TOPN_SIMILAR_FILTER, 1, v.rs);
    // (rescored mode: a result that is not finite comes back as THE NaN, ranked first -- RecommendIterator.java:105)
    if (n > 0 && !std::isfinite(o_q.scores[0])) {
      if (!rq.bad_q) return fail(h, MALS_INVALID_ARG, topn_bad_value(rq));
      rq.bad_q[ps.q0 + q] = 1;
    }
  }
  return MALS_OK;
}

bool topn_dense_only(mals_handle h, int how_many, const mals_rescorer_s* r = nullptr, bool cosine = false) {
  const int64_t n_items = h->side[MALS_SIDE_Y].n_total;
  // (a rescorer outside the filter's range -- RESCORED MODE's, or RESCORED COSINE MODE's for a cosine call: topn_kernels.h)
  return n_items < 131072 || n_items >= 0xffffffffll || how_many > TOPN_FILTER_MAX_N || n_items / 16 < 64 * (int64_t)how_many ||
         std::getenv("MALS_TOPN_FULL") || (r && !(cosine ? rescorer_cos_filter_ok(r) : rescorer_filter_ok(r)));
}

// streams, events and pinned result blocks of the slots; every slot stream ordered after the work already on the handle's
int topn_prepare_slots(mals_handle h, TopnWorkspace* w) {
  for (TopnSlot& sl : w->slot) {
    HIPCHK(h, sl.stream.ensure());
    HIPCHK(h, sl.ev.ensure(hipEventDisableTiming));
  }
  HIPCHK(h, w->ev_begin.ensure(hipEventDisableTiming));
  return MALS_OK;
}

// decode the pass in slot s; the queries the filter could not answer (rare) go through the dense path, run by run (the
// slot's input block is free again: its pass has finished)
int topn_finish_slot(mals_handle h, TopnWorkspace* w, int s, const TopnRequest& rq, const TopnPass& done, const TopnFilterPlan& p,
                     std::vector<uint8_t>& failed) {
  bool any_failed = false;
  if (int rc = topn_pass_filter_finish(h, w->slot[s], rq, done, p, failed, &any_failed)) return rc;
  if (any_failed && std::getenv("MALS_TOPN_DEBUG")) {
    int nf = 0;
    for (uint8_t f : failed) nf += f;
    std::fprintf(stderr, "[mals top-N] pass at query %d (%d queries): %d to the dense path\n", done.q0, done.nq, nf);
  }
  if (any_failed) {
    for (int q = 0; q < done.nq;) {
      if (!failed[(size_t)q]) {
        ++q;
        continue;
      }
      int e = q;
      while (e < done.nq && failed[(size_t)e] && e - q < TOPN_MAX_QUERIES) ++e;
      TopnPass ps;
      ps.q0 = done.q0 + q;
      ps.nq = e - q;
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (int rc = topn_upload_pass(h, w->slot[s], h->stream, rq, ps)) return rc;
      if (int rc = topn_pass_dense(h, w, w->slot[s], rq, ps)) return rc;
      q = e;
    }
  }
  return MALS_OK;
}

// ---- recommendedBecause: the rescore and final kernels on a given candidate list -------------------------------------
// RecommendedBecauseIterator.java:61-75 over the user's known items (ServerRecommender.java:1324-1376): no sample, no filter.
// Up to TOPN_MAX_QUERIES queries per pass, the lists in chunks of TOPN_BECAUSE_CAP candidates; the N best of every chunk
// come back, and the N best of those are the N best of the list (ties by ascending index, topn_emit).  On the caller's
// stream with slot 0's buffers (the call runs alone on the workspace).
constexpr int TOPN_BECAUSE_CAP = 4096;

int topn_because_run(mals_handle h, TopnWorkspace* w, const TopnRequest& rq_in) {
  SideState& x = h->side[MALS_SIDE_X];
  const int k = h->cfg.features, how_many = rq_in.how_many, cap = TOPN_BECAUSE_CAP;
  TopnKnown kn = topn_known(h);
  // known items changed by writes (foldin_host.h): the queries' current sets as a CSR of their own, query q = its row q
  TopnRequest rq = rq_in;
  std::vector<int64_t> own_user, own_ptr, rows;
  std::vector<int32_t> own_idx;
  std::vector<std::vector<int32_t>> sets;
  DeviceBuffer<int64_t> d_own_ptr;
  DeviceBuffer<int32_t> d_own_idx;
  if (foldin_has_overlay(h)) {
    for (int q = 0; q < rq.n_queries; ++q) rows.push_back(rq.because_user[q] - x.row_offset);
    std::string msg;
    if (int rc = foldin_known_full(h, rows, sets, msg)) return fail(h, rc, msg);
    own_ptr.assign(1, 0);
    for (int q = 0; q < rq.n_queries; ++q) {
      own_idx.insert(own_idx.end(), sets[(size_t)q].begin(), sets[(size_t)q].end());
      own_ptr.push_back((int64_t)own_idx.size());
      own_user.push_back(x.row_offset + q);
    }
    HIPCHK(h, d_own_ptr.alloc(own_ptr.size()));
    HIPCHK(h, d_own_idx.alloc(std::max<size_t>(own_idx.size(), 1)));
    HIPCHK(h, hipMemcpyAsync(d_own_ptr.get(), own_ptr.data(), sizeof(int64_t) * own_ptr.size(), hipMemcpyHostToDevice, h->stream));
    if (!own_idx.empty())
      HIPCHK(h, hipMemcpyAsync(d_own_idx.get(), own_idx.data(), sizeof(int32_t) * own_idx.size(), hipMemcpyHostToDevice, h->stream));
    kn = {d_own_ptr.get(), d_own_idx.get()};
    rq.because_user = own_user.data();
  }
  TopnSlot& sl = w->slot[0];
  if (int rc = topn_slot_alloc(h, sl)) return rc;
  HIPCHK(h, sl.d_pairs.reserve((size_t)TOPN_MAX_QUERIES * (size_t)cap, h->stream));
  HIPCHK(h, sl.d_cand.reserve((size_t)TOPN_MAX_QUERIES * (size_t)cap, h->stream));
  HIPCHK(h, sl.d_qn.reserve((size_t)TOPN_MAX_QUERIES, h->stream));
  HIPCHK(h, sl.h_stage.reserve(TopnStage(nullptr, TOPN_MAX_QUERIES, how_many).bytes(), h->stream));
  const TopnStage o(sl.h_stage.get(), TOPN_MAX_QUERIES, how_many);
  const TopnVariant v = topn_variant(h, rq);   // cosine
  const TopnVariantArgs va = topn_variant_args(v, sl, rq);
  std::vector<std::vector<TopnCand>> cand;
  for (int q0 = 0; q0 < rq.n_queries; q0 += TOPN_MAX_QUERIES) {
    TopnPass ps;
    ps.q0 = q0;
    ps.nq = std::min(TOPN_MAX_QUERIES, rq.n_queries - q0);
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (the input block is reused pass by pass)
    if (int rc = topn_upload_pass(h, sl, h->stream, rq, ps)) return rc;
    hipLaunchKernelGGL(topn_qnorm_kernel, dim3(1), dim3(64), 0, h->stream, sl.d_vecs, sl.d_vrow, ps.nq, k, sl.d_qn.get());
    cand.assign((size_t)ps.nq, {});
    for (int64_t off = 0;; off += cap) {
      hipLaunchKernelGGL(topn_known_cand_kernel, dim3((unsigned)ps.nq), dim3(256), 0, h->stream, kn.ptr, kn.idx, sl.d_rows, off, cap, sl.d_cand.get(),
                         sl.d_count.get());
      // (the candidates ARE the known items: nothing to drop but the tag items)
      topn_launch_rescore(h, sl, h->stream, v, va, ps.nq, cap, TopnKnown{nullptr, nullptr}, nullptr, nullptr, nullptr);
      topn_launch_final(sl, h->stream, ps.nq, cap, how_many, o);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipStreamSynchronize(h->stream));
      bool more = false;
      for (int q = 0; q < ps.nq; ++q) {
        for (int j = 0; j < how_many; ++j) {
          TopnCand c;
          if (topn_decode_pair(o.pairs()[(size_t)q * how_many + j], &c)) cand[(size_t)q].push_back(c);
        }
        more = more || o.count()[q] > (unsigned)cap;
      }
      if (!more) break;
    }
    for (int q = 0; q < ps.nq; ++q) {
      const TopnOut o_q = topn_out(rq, (size_t)(ps.q0 + q));
      (void)topn_emit(cand[(size_t)q], how_many, o_q.items, o_q.scores, o_q.n);   // (finite scores only: the rescore struck the rest)
    }
  }
  return MALS_OK;
}

// similarityToItem: one small kernel on the caller's stream
int topn_similarity_to_run(mals_handle h, const TopnRequest& rq) {
  const int n = rq.n_queries;
  DeviceBuffer<int64_t> d_idx;
  DeviceBuffer<float> d_out;
  HIPCHK(h, d_idx.alloc((size_t)n));
  HIPCHK(h, d_out.alloc((size_t)n));
  HIPCHK(h, hipMemcpyAsync(d_idx.get(), rq.item_rows, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(topn_similarity_to_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->side[MALS_SIDE_Y].F, h->cfg.features,
                     rq.to_item, d_idx.get(), n, d_out.get());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(rq.sim_out, d_out.get(), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MALS_OK;
}

int topn_run(mals_handle h, const TopnRequest& rq) {
  if (!h->serving->tn_ws) h->serving->tn_ws = new TopnWorkspace();
  TopnWorkspace* w = h->serving->tn_ws;
  if (rq.kind == TOPN_KIND_BECAUSE) return topn_because_run(h, w, rq);
  if (rq.kind == TOPN_KIND_SIMILARITY_TO) return topn_similarity_to_run(h, rq);
  if (rq.kind == TOPN_KIND_CALL) return (*rq.call)();
  if (topn_dense_only(h, rq.how_many, rq.rescorer, rq.cosine)) {
    for (int q0 = 0; q0 < rq.n_queries; q0 += TOPN_MAX_QUERIES) {
      TopnPass ps;
      ps.q0 = q0;
      ps.nq = std::min(TOPN_MAX_QUERIES, rq.n_queries - q0);
      if (int rc = topn_upload_pass(h, w->slot[0], h->stream, rq, ps)) return rc;
      if (int rc = topn_pass_dense(h, w, w->slot[0], rq, ps)) return rc;
    }
    return MALS_OK;
  }
  const TopnFilterPlan p = topn_plan(h, rq.how_many);
  if (int rc = topn_prepare_slots(h, w)) return rc;
  // whatever the caller's stream still has to do (an iteration, a factor upload) comes first
  HIPCHK(h, hipEventRecord(w->ev_begin, h->stream));
  for (TopnSlot& sl : w->slot) HIPCHK(h, hipStreamWaitEvent(sl.stream, w->ev_begin, 0));
  int per_pass = 16 * topn_max_tiles(p.S);
  if (const char* e = std::getenv("MALS_TOPN_QUERIES_PER_PASS")) per_pass = std::max(16, std::min(per_pass, std::atoi(e) / 16 * 16));  // tuning override
  int n_slots = TOPN_SLOTS;
  if (const char* e = std::getenv("MALS_TOPN_SLOTS")) n_slots = std::max(1, std::min(TOPN_SLOTS, std::atoi(e)));  // tuning override
  // Passes go round the slots; pass i is decoded after pass i + n_slots - 1 has been enqueued, right before its slot is
  // needed again: the device never waits for the host between passes.
  TopnPass inflight[TOPN_SLOTS];
  bool busy[TOPN_SLOTS] = {};
  std::vector<uint8_t> failed;
  auto finish = [&](int s) -> int {
    if (!busy[s]) return MALS_OK;
    busy[s] = false;
    return topn_finish_slot(h, w, s, rq, inflight[s], p, failed);
  };
  int s = 0;
  int rc_all = MALS_OK;
  for (int q0 = 0; q0 < rq.n_queries && rc_all == MALS_OK; q0 += per_pass) {
    if ((rc_all = finish(s))) break;
    TopnPass ps;
    ps.q0 = q0;
    ps.nq = std::min(per_pass, rq.n_queries - q0);
    if ((rc_all = topn_upload_pass(h, w->slot[s], w->slot[s].stream, rq, ps))) break;
    if ((rc_all = topn_pass_filter_enqueue(h, w->slot[s], rq, ps, p))) break;
    inflight[s] = ps;
    busy[s] = true;
    s = (s + 1) % n_slots;
  }
  // drain in enqueue order (also on an error: nothing of this call may still be running when it returns)
  for (int i = 0; i < n_slots; ++i) {
    const int t = (s + i) % n_slots;
    if (rc_all != MALS_OK) {
      if (w->slot[t].stream) (void)hipStreamSynchronize(w->slot[t].stream);
      busy[t] = false;
    } else {
      rc_all = finish(t);
    }
  }
  return rc_all;
}

// ---- the serving front: many request threads, one handle ---------------------------------------------------------------
// The reference's top-N is entered by every request thread of the servlet container at once (ServerRecommender.java:359-441
// -> multithreadedTopN :443-508), one user per call.  Here a call is cheap only as part of a PASS (one read of Y answers up
// to 240 queries), so concurrent calls are folded into passes: a call becomes a ticket in the handle's queue; the first
// thread that finds no leader becomes the leader, packs whatever is queued into the next pass, enqueues it on a slot,
// decodes finished passes and wakes their callers.  When its own ticket is answered it hands leadership to a caller that is
// still waiting.  While a pass is on the device the tickets of the calls that arrive pile up and form the next one (group
// commit); `depth` passes are in flight at most (2: one streaming Y, one being prepared behind it; more would only split the
// same callers over more reads of Y).  Calls that are passes of their own already (>= TOPN_FRONT_BULK queries, caller's
// vectors, how_many the filter does not take) run exclusively, in queue order, through topn_run.
constexpr int TOPN_FRONT_BULK = 64;

struct TopnTicket {
  TopnRequest rq;      // what the call asks for, as its entry point built it
  bool fold = false;   // small enough to share a pass with other callers' calls (the entry point's size tests); false: the
                       // call is passes of its own, or no top-N at all, and runs alone in queue order
  int rc = MALS_OK;
  std::string err;
  bool done = false;          // under the front's mutex
  bool is_leader = false;
  // How a waiting caller hears from the leader: `sig` (TOPN_SIG_DONE: the answer is in the caller's arrays; TOPN_SIG_LEAD:
  // take over as leader).  A caller first polls it (an answer takes 100-200 us: most arrive while it polls, and then the
  // leader's "wake-up" is one store, not a futex call per caller -- 33 of those per pass were half of a pass's host time at
  // 128 callers), then blocks on its own condition variable.  Everything the leader touches of a ticket it touches under
  // the ticket's mutex, and a caller takes that mutex once before it returns: the ticket lives on the caller's stack.
  std::atomic<int> sig{0};
  std::atomic<bool> blocked{false};
  std::mutex mu;
  std::condition_variable cv;
  // Waking the callers of a finished pass is a futex call each (they block): 28 of them were 110 us of the leader's time
  // per pass at 128 callers, more than the pass takes on the device.  The leader wakes ONE caller of the pass and leaves it
  // the list of the others (to_wake); that caller wakes them on its way out.  A ticket on such a list has visit_pending set
  // until its waker has let go of it, and does not return before.
  std::vector<TopnTicket*> to_wake;
  std::atomic<bool> visit_pending{false};
};
enum { TOPN_SIG_DONE = 1, TOPN_SIG_LEAD = 2 };

void topn_signal(TopnTicket* t, int bits) {
  std::lock_guard<std::mutex> lk(t->mu);
  t->sig.fetch_or(bits, std::memory_order_seq_cst);
  if (t->blocked.load(std::memory_order_seq_cst)) t->cv.notify_one();
}

// returns the signal bits seen (never 0)
int topn_wait_signal(TopnTicket* t, int spin_us) {
  const auto t0 = std::chrono::steady_clock::now();
  for (int it = 0;; ++it) {
    const int sg = t->sig.load(std::memory_order_acquire);
    if (sg) return sg;
    if ((it & 15) == 15) {
      if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > (double)spin_us) break;
      std::this_thread::yield();
    } else {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
      __builtin_ia32_pause();
#endif
    }
  }
  std::unique_lock<std::mutex> lk(t->mu);
  t->blocked.store(true, std::memory_order_seq_cst);
  while (!t->sig.load(std::memory_order_seq_cst)) t->cv.wait(lk);
  t->blocked.store(false, std::memory_order_seq_cst);
  return t->sig.load(std::memory_order_seq_cst);
}

struct TopnFrontPass {
  std::vector<TopnTicket*> tickets;
  std::vector<int64_t> users;
  std::vector<uint8_t> skip;
  std::vector<TopnOut> outs;
  // a pass of by-vector calls: the callers' vectors and exclusion lists back to back (of mostSimilarItems calls: their items)
  std::vector<int64_t> items;
  std::vector<float> vecs;
  std::vector<int64_t> vptr, eptr, eidx;
  TopnRequest rq;
  TopnPass ps;
  TopnFilterPlan plan;
  // the pass's rescorer as it was when the pass was formed (kept alive until the pass is decoded), and the failed queries
  std::shared_ptr<const RescorerState> rs_keep;
  TopnRescore rs_args;
  std::vector<uint8_t> bad;
};

struct TopnFront {
  std::atomic<int64_t> similar[4] = {};   // mals_similar_stats (TOPN_SIMILAR_*), read without a ticket
  std::mutex mu;
  std::deque<TopnTicket*> queue;
  bool leader = false;
  TopnFrontPass inflight[TOPN_SLOTS];
  bool busy[TOPN_SLOTS] = {};
  int n_busy = 0, next_slot = 0, oldest = 0;
  int depth = 2;
  int spin_us = 0;     // how long a waiting caller polls before it blocks (mals_recommend_set_spin_us; MALS_TOPN_FRONT_SPIN_US at
                       // mals_create).  0: block at once -- polling callers compete with the HIP runtime's own threads for cores
  std::vector<uint8_t> failed;
  // counters (mals_recommend_front_stats)
  uint64_t calls = 0, queries = 0, passes = 0, bulk_calls = 0;
  // mals_load_generation replaces the rows a request's indices were checked against (generation_host.h): odd while a swap
  // writes the handle, two more after every swap.  A request carries the value its entry point read BEFORE its argument
  // checks (topn_generation_guard); one that reaches the queue with another value, or waits in it across a swap, is handed
  // back with TOPN_RETRY and its entry point checks it again against the new generation.
  std::atomic<uint64_t> gen_seq{0};
  TopnFrontPass stale;   // the requests a swap hands back (topn_generation_swap_end)
};
constexpr int TOPN_RETRY = -1000;   // internal: never leaves the library

TopnFront* topn_front(mals_handle h) { return h->serving->tn_front; }
void topn_similar_count(mals_handle h, int which, int n, bool rescored) {
  TopnFront* f = topn_front(h);
  f->similar[which].fetch_add(n, std::memory_order_relaxed);
  if (rescored) f->similar[TOPN_SIMILAR_RESCORED].fetch_add(n, std::memory_order_relaxed);
}

struct TopnGenStamp {
  mals_handle h = nullptr;
  uint64_t seq = 0;
};
thread_local TopnGenStamp t_gen_stamp;

// an entry point of the readers: `call` = its argument checks and its topn_front_submit
template <class F>
int topn_generation_guard(mals_handle h, F&& call) {
  if (!h) return call();
  TopnFront* f = topn_front(h);
  for (;;) {
    const uint64_t seq = f->gen_seq.load(std::memory_order_acquire);
    if (seq & 1) {   // a swap is writing the handle
      std::this_thread::yield();
      continue;
    }
    t_gen_stamp = {h, seq};
    const int rc = call();
    t_gen_stamp = {nullptr, 0};
    if (rc == TOPN_RETRY) continue;
    if (rc != MALS_OK && f->gen_seq.load(std::memory_order_acquire) != seq) continue;   // (the checks may have read a handle in mid-swap)
    return rc;
  }
}

// THE CHECKS AND THE SWAP.  The argument checks read plain fields of the handle (SideState::F, n_total, n_local, known_ptr,
// known_rows, tag_bits_items ...) on the caller's thread while a swap may be writing them: a sequence lock over data that is
// not atomic, which the language calls a data race.  What makes it sound here: the fields are aligned words, read once each
// and only compared (no pointer among them is followed before the ticket runs), a check that saw a mixture can only come
// out wrong in a call whose sequence number no longer matches, and every such call is checked again -- a request is never
// RUN on the strength of a check that overlapped a swap.  mals_grow_factor_rows has always changed n_total under the same
// readers.
// mals_load_generation, leader only, mutex NOT held.  Before the swap, and fallible: room for the list of the requests that
// topn_generation_swap_end hands back (they are in the queue by now: one that arrives later is refused at the door) ...
void topn_generation_swap_reserve(mals_handle h) {
  TopnFront* f = topn_front(h);
  std::lock_guard<std::mutex> lk(f->mu);
  f->stale.tickets.reserve(f->queue.size());
}
// ... before the first write of the swap ...
void topn_generation_swap_begin(mals_handle h) { topn_front(h)->gen_seq.fetch_add(1, std::memory_order_acq_rel); }

// leader only, mutex NOT held: the pass in `fp` (already filled) onto slot s
int topn_front_enqueue(mals_handle h, TopnWorkspace* w, int s, TopnFrontPass& fp) {
  if (int rc = topn_prepare_slots(h, w)) return rc;
  HIPCHK(h, hipEventRecord(w->ev_begin, h->stream));
  HIPCHK(h, hipStreamWaitEvent(w->slot[s].stream, w->ev_begin, 0));
  if (int rc = topn_upload_pass(h, w->slot[s], w->slot[s].stream, fp.rq, fp.ps)) return rc;
  return topn_pass_filter_enqueue(h, w->slot[s], fp.rq, fp.ps, fp.plan);
}

void topn_front_complete(TopnFrontPass& fp, int rc, const std::string& err) {  // mutex held
  TopnTicket* waker = nullptr;
  size_t waiting = 0;
  size_t q0 = 0;   // a coalesced pass: the tickets' queries back to back; a query that is not finite fails its own ticket only
  for (TopnTicket* t : fp.tickets) {
    int trc = rc;
    if (rc == MALS_OK && !fp.bad.empty())
      for (size_t q = q0; q < q0 + (size_t)t->rq.n_queries && q < fp.bad.size(); ++q)
        if (fp.bad[q]) trc = MALS_INVALID_ARG;
    q0 += (size_t)t->rq.n_queries;
    t->rc = trc;
    if (trc != MALS_OK) t->err = rc != MALS_OK ? err : std::string(topn_bad_value(t->rq));
    t->done = true;
    if (!t->is_leader) ++waiting;
  }
  fp.bad.clear();
  fp.rs_keep.reset();
  if (waiting >= 16) {
    // groups of 8: the leader wakes the first caller of every group and leaves it the other seven (measured at 128 callers,
    // ~37 per pass: 2.4e5 -> 4.3e5 queries/s, p50 510 -> 260 us; below 16 per pass the leader's own wake-ups cost less than the
    // extra hop adds to the tail, so small passes are woken directly)
    size_t in_group = 0;
    std::vector<TopnTicket*> wakers;
    for (TopnTicket* t : fp.tickets) {
      if (t->is_leader) continue;
      if (in_group == 0) {
        waker = t;
        waker->to_wake.reserve(7);
        wakers.push_back(waker);
      } else {
        t->visit_pending.store(true, std::memory_order_seq_cst);   // before the answer becomes visible
        waker->to_wake.push_back(t);
        t->sig.fetch_or(TOPN_SIG_DONE, std::memory_order_seq_cst);  // (a caller that is polling sees it at once; one that blocks is woken by its group's first)
      }
      in_group = (in_group + 1) % 8;
    }
    for (TopnTicket* w : wakers) topn_signal(w, TOPN_SIG_DONE);
  } else {
    for (TopnTicket* t : fp.tickets)
      if (!t->is_leader) topn_signal(t, TOPN_SIG_DONE);   // (after this the ticket may be gone)
  }
  fp.tickets.clear();
}

// ... and after its last: the requests that waited in the queue across the swap were checked against the old generation --
// each goes back to its entry point (the calls of foldin_host.h check their arguments inside their own ticket and stay)
void topn_generation_swap_end(mals_handle h) {
  TopnFront* f = topn_front(h);
  std::lock_guard<std::mutex> lk(f->mu);
  f->gen_seq.fetch_add(1, std::memory_order_acq_rel);
  TopnFrontPass& stale = f->stale;
  stale.tickets.clear();
  // (requests that came while the swap ran were refused by topn_front_submit: these all fit what _reserve made room for)
  auto first_stale = std::stable_partition(f->queue.begin(), f->queue.end(), [](const TopnTicket* t) { return t->rq.kind == TOPN_KIND_CALL; });
  for (auto it = first_stale; it != f->queue.end(); ++it) {
    stale.tickets.push_back(*it);
    --f->calls;   // its entry point submits it again: one call, counted once
    f->queries -= (uint64_t)(*it)->rq.n_queries;
  }
  f->queue.erase(first_stale, f->queue.end());
  if (!stale.tickets.empty()) topn_front_complete(stale, TOPN_RETRY, "");
}

// a caller on its way out: the pass-mates the leader left to it, then its own ticket's last visitors
void topn_ticket_leave(TopnTicket& me) {
  for (TopnTicket* m : me.to_wake) {
    {
      std::lock_guard<std::mutex> lk(m->mu);
      if (m->blocked.load(std::memory_order_seq_cst)) m->cv.notify_one();
    }
    m->visit_pending.store(false, std::memory_order_release);   // the last touch of m
  }
  me.to_wake.clear();
  while (me.visit_pending.load(std::memory_order_acquire)) std::this_thread::yield();
  { std::lock_guard<std::mutex> own(me.mu); }   // the leader has let go of the ticket
}

// The calling thread leads until its own ticket is answered.
void topn_front_lead(mals_handle h, TopnFront* f, std::unique_lock<std::mutex>& lk, TopnTicket* me) {
  if (!h->serving->tn_ws) h->serving->tn_ws = new TopnWorkspace();
  TopnWorkspace* w = h->serving->tn_ws;
  const int k_tiles = topn_max_tiles((h->cfg.features + 31) / 32);
  auto finish_oldest = [&]() {
    const int s = f->oldest;
    TopnFrontPass& fp = f->inflight[s];
    lk.unlock();
    const int rc = topn_finish_slot(h, w, s, fp.rq, fp.ps, fp.plan, f->failed);
    const std::string err = rc != MALS_OK ? h->err : std::string();
    lk.lock();
    f->busy[s] = false;
    --f->n_busy;
    f->oldest = (s + 1) % f->depth;
    topn_front_complete(fp, rc, err);
  };
  while (!me->done) {
    TopnTicket* head = f->queue.empty() ? nullptr : f->queue.front();
    if (head && (!head->fold || topn_dense_only(h, head->rq.how_many, head->rq.rescorer, head->rq.cosine))) {
      // a request that is passes of its own (or a catalogue the dense path answers): alone on the workspace, as it is
      while (f->n_busy > 0) finish_oldest();
      if (me->done && head != me) break;   // (own answer arrived while draining: let the successor run it)
      f->queue.pop_front();
      TopnFrontPass one;
      one.tickets.push_back(head);
      one.rq = head->rq;
      if (!head->fold && one.rq.kind != TOPN_KIND_CALL) ++f->bulk_calls;   // (the writes of foldin_host.h are no recommend calls)
      if (one.rq.rescorer) {
        rescorer_bind(one.rq.rescorer, one.rs_keep, one.rs_args);
        one.rq.rs = &one.rs_args;
      }
      lk.unlock();
      const int rc = topn_run(h, one.rq);
      const std::string err = rc != MALS_OK ? h->err : std::string();
      lk.lock();
      topn_front_complete(one, rc, err);
      continue;
    }
    if (head && f->n_busy < f->depth) {
      // the next pass: whole tickets, one how_many, up to the pass's query capacity
      const int s = f->next_slot;
      TopnFrontPass& fp = f->inflight[s];
      const int cap = 16 * k_tiles;
      const int kf = h->cfg.features;
      fp.tickets.clear(); fp.users.clear(); fp.skip.clear(); fp.outs.clear();
      fp.items.clear(); fp.vecs.clear(); fp.vptr.assign(1, 0); fp.eptr.assign(1, 0); fp.eidx.clear();
      const int how_many = head->rq.how_many;
      // a pass holds by-user calls, by-vector calls or mostSimilarItems calls, never two kinds (where its query vectors come
      // from -- X on the device, an uploaded block, rows of Y -- and how they score is per pass)
      auto kind_of = [](const TopnTicket* t) { return t->rq.vectors ? 1 : t->rq.item_rows ? 2 : 0; };
      const int kind = kind_of(head);
      const bool by_vector = kind == 1;
      bool any_excl = false;
      while (!f->queue.empty()) {
        TopnTicket* t = f->queue.front();
        const TopnRequest& r = t->rq;
        if (!t->fold || r.how_many != how_many || kind_of(t) != kind || r.rescorer != head->rq.rescorer || r.flags != head->rq.flags || (int)fp.outs.size() + r.n_queries > cap) break;
        f->queue.pop_front();
        fp.tickets.push_back(t);
        for (int q = 0; q < r.n_queries; ++q) {
          if (kind == 2) {   // (vec_ptr is never NULL here; the query's items are also its exclusions)
            const int64_t v0 = r.vec_ptr[q], v1 = r.vec_ptr[q + 1];
            fp.items.insert(fp.items.end(), r.item_rows + v0, r.item_rows + v1);
            fp.vptr.push_back(fp.vptr.back() + (v1 - v0));
            fp.eptr.push_back(fp.vptr.back());
          } else if (by_vector) {
            const int64_t v0 = r.vec_ptr ? r.vec_ptr[q] : q, v1 = r.vec_ptr ? r.vec_ptr[q + 1] : q + 1;
            fp.vecs.insert(fp.vecs.end(), r.vectors + v0 * kf, r.vectors + v1 * kf);
            fp.vptr.push_back(fp.vptr.back() + (v1 - v0));
            if (r.excl_ptr && r.excl_idx) {
              fp.eidx.insert(fp.eidx.end(), r.excl_idx + r.excl_ptr[q], r.excl_idx + r.excl_ptr[q + 1]);
              any_excl = any_excl || r.excl_ptr[q + 1] > r.excl_ptr[q];
            }
            fp.eptr.push_back((int64_t)fp.eidx.size());
          } else {
            fp.users.push_back(r.user_idx[q]);
            fp.skip.push_back(r.skip_known ? 1 : 0);
          }
          fp.outs.push_back(topn_out(r, (size_t)q));
        }
      }
      fp.rq = TopnRequest();
      fp.rq.n_queries = (int)fp.outs.size();
      fp.rq.how_many = how_many;
      if (kind == 2) {
        fp.rq.item_rows = fp.items.data();
        fp.rq.vec_ptr = fp.vptr.data();
        fp.rq.excl_ptr = fp.eptr.data();
        fp.rq.excl_idx = fp.items.data();
        fp.rq.cosine = true;
      } else if (by_vector) {
        fp.rq.vectors = fp.vecs.data();
        fp.rq.vec_ptr = fp.vptr.data();
        if (any_excl) {
          fp.rq.excl_ptr = fp.eptr.data();
          fp.rq.excl_idx = fp.eidx.data();
        }
      } else {
        fp.rq.user_idx = fp.users.data();
        fp.rq.skip_known_q = fp.skip.data();
      }
      fp.rq.out_q = fp.outs.data();
      if (head->rq.rescorer) {
        fp.rq.rescorer = head->rq.rescorer;
        fp.rq.flags = head->rq.flags;
        rescorer_bind(head->rq.rescorer, fp.rs_keep, fp.rs_args);
        fp.rq.rs = &fp.rs_args;
      }
      fp.bad.assign((size_t)fp.rq.n_queries, 0);
      fp.rq.bad_q = fp.bad.data();
      fp.ps = TopnPass();
      fp.ps.q0 = 0;
      fp.ps.nq = fp.rq.n_queries;
      fp.plan = topn_plan(h, how_many);
      f->busy[s] = true;
      ++f->n_busy;
      f->next_slot = (s + 1) % f->depth;
      ++f->passes;
      lk.unlock();
      const int rc = topn_front_enqueue(h, w, s, fp);
      const std::string err = rc != MALS_OK ? h->err : std::string();
      lk.lock();
      if (rc != MALS_OK) {  // nothing of the pass may still run when its callers return
        lk.unlock();
        if (w->slot[s].stream) (void)hipStreamSynchronize(w->slot[s].stream);
        lk.lock();
        f->busy[s] = false;
        --f->n_busy;
        // (slots complete in order: an enqueue failure of the newest pass leaves `oldest` where it was unless it was alone)
        if (f->n_busy == 0) f->oldest = f->next_slot;
        else f->next_slot = s;
        topn_front_complete(fp, rc, err);
      }
      continue;
    }
    if (f->n_busy > 0) {
      finish_oldest();
      continue;
    }
    break;  // (not reached: a leader's own ticket is queued, in flight or done)
  }
}

// every mals_recommend* call ends here: `rq` as a ticket in the handle's queue; fold: it may share a pass with other callers'
int topn_front_submit(mals_handle h, const TopnRequest& rq, bool fold) {
  TopnTicket me;
  me.rq = rq;
  me.fold = fold;
  TopnFront* f = topn_front(h);
  std::unique_lock<std::mutex> lk(f->mu);
  if (rq.kind != TOPN_KIND_CALL && t_gen_stamp.h == h && t_gen_stamp.seq != f->gen_seq.load(std::memory_order_acquire)) return TOPN_RETRY;
  ++f->calls;
  f->queries += (uint64_t)rq.n_queries;
  f->queue.push_back(&me);
  for (;;) {
    if (me.done) break;
    if (!f->leader) {
      f->leader = true;
      me.is_leader = true;
      topn_front_lead(h, f, lk, &me);
      me.is_leader = false;
      f->leader = false;
      // successor: a caller whose answer is still out -- in the oldest pass in flight, else at the head of the queue
      TopnTicket* next = nullptr;
      if (f->n_busy > 0) {
        for (TopnTicket* t : f->inflight[f->oldest].tickets)
          if (!t->done) { next = t; break; }
      }
      if (!next && !f->queue.empty()) next = f->queue.front();
      if (next) topn_signal(next, TOPN_SIG_LEAD);
      continue;
    }
    // somebody leads: wait for the answer, or for the call to lead
    const int spin_us = f->spin_us;
    lk.unlock();
    const int sg = topn_wait_signal(&me, spin_us);
    if (sg & TOPN_SIG_LEAD) me.sig.fetch_and(~TOPN_SIG_LEAD, std::memory_order_seq_cst);
    lk.lock();
  }
  const int rc = me.rc;
  if (rc != MALS_OK && rc != TOPN_RETRY) h->err = me.err;   // (a request handed back is no failure: it is submitted again)
  lk.unlock();
  topn_ticket_leave(me);
  return rc;
}
