/*
 * myrrix_als.h -- C-ABI of the MI355X-native ALS matrix-factorization core (libmyrrix_als.so).
 *
 * This is the drop-in boundary behind myrrix-recommender's
 *   net.myrrix.online.factorizer.MatrixFactorizer            (online/src/.../MatrixFactorizer.java:31-77)
 *   net.myrrix.online.factorizer.als.AlternatingLeastSquares (online/src/.../als/AlternatingLeastSquares.java:66)
 * Plain pointers and sizes only; no C++/torch types.  The reference has no FFI for this path (it is
 * pure Java); the JNI stub a maintainer would add to bind these entry points is shown in
 * INTEGRATION.md, next to the Java adapter that keeps the 5-argument constructor of
 * AlternatingLeastSquares.java:132-136.  Abbreviations below: ALS = that file, MU =
 * common/src/net/myrrix/common/math/MatrixUtils.java, CMLSS =
 * common/src/net/myrrix/common/math/CommonsMathLinearSystemSolver.java.
 *
 * Data model.  The Java side keeps FastByIDMap<FastByIDFloatMap> RbyRow / RbyColumn and
 * FastByIDMap<float[]> X / Y; the adapter maps 64-bit ids to dense row indices and hands the native
 * side CSR arrays: "side X" = rows of R (users; its factor matrix is X, solved from Y), "side Y" =
 * rows of R^T (items; factor matrix Y, solved from X).  Factor matrices are row-major fp32,
 * n_rows_total x features, resident in HBM.  n_rows_total may exceed the number of matrix rows: Y may
 * carry stale rows that are never re-solved but still count in Y^T Y (ALS:304-308,342), and a
 * multi-GPU shard layout may pad each rank's slice.  One handle drives ONE GPU and holds the
 * matrix rows [row_offset, row_offset+n_rows_local) of each side plus FULL replicas of X and Y;
 * the caller exchanges freshly solved slices between handles (all-gather) -- see
 * mals_factor_device_ptr / mals_bind_factors.
 *
 * Every function returns a status code and never throws across the ABI.
 */
#ifndef MYRRIX_ALS_H
#define MYRRIX_ALS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MALS_ABI_VERSION 5

typedef struct mals_handle_s* mals_handle;

/* Status codes.  Java adapter mapping (ALS:349, CMLSS:46-54, MatrixFactorizer.java:41-47):
 * SINGULAR -> ExecutionException(SingularMatrixSolverException(apparentRank)),
 * CANCELLED -> InterruptedException, everything else -> ExecutionException(IllegalStateException). */
enum {
  MALS_OK = 0,
  MALS_SINGULAR = 1,
  MALS_INVALID_ARG = 2,
  MALS_HIP_ERROR = 3,
  MALS_COMM_ERROR = 4,
  MALS_CANCELLED = 5,
  MALS_OOM = 6,
  MALS_ILL_CONDITIONED = 7, /* IllConditionedSolverException (Generation.java:150-153) */
  MALS_IO_ERROR = 8         /* java.io.IOException (unreadable / corrupt / truncated model file) */
};

enum { MALS_SIDE_X = 0, MALS_SIDE_Y = 1 };

/* ALS:85-91: model.reconstructRMatrix / model.lossIgnoresUnspecified (static finals there). */
enum { MALS_FLAG_RECONSTRUCT_R = 1, MALS_FLAG_LOSS_IGNORES_UNSPECIFIED = 2 };

enum { MALS_MEM_HOST = 0, MALS_MEM_DEVICE = 1 };

enum { MALS_GRAMIAN_AUTO = 0, MALS_GRAMIAN_FP32 = 1, MALS_GRAMIAN_SPLIT_F16 = 2, MALS_GRAMIAN_SPLIT3_F16 = 3 };

enum { MALS_SOLVE_AUTO = 0, MALS_SOLVE_DIRECT = 1, MALS_SOLVE_DUAL = 2 };

typedef struct mals_config {
  int32_t struct_size;          /* sizeof(mals_config), for ABI evolution                      */
  int32_t features;             /* k; ALS:134 "features must be positive"; 1..128 supported    */
  double alpha;                 /* model.als.alpha,  default 1.0 (ALS:71,506-509)              */
  double lambda;                /* model.als.lambda, default 0.1 (ALS:73,511-514); the ridge
                                   applied per row is lambda*alpha*n_u (ALS:435,488)           */
  double singularity_threshold; /* common.matrix.singularityThreshold, default 1e-5
                                   (LinearSystemSolver.java:33-34)                             */
  int32_t flags;                /* MALS_FLAG_*                                                 */
  int32_t device;               /* HIP device ordinal                                          */
  int32_t segment_nnz;          /* rows longer than this are split across waves; 0 = default.
                                   Long dense rows with ascending columns are cut by band of the
                                   gather table instead of by count        */
  int32_t chunk_rows;           /* >0: the shard's rows are cut into contiguous ranges of this many
                                   rows that can be solved one by one (mals_solve_chunk), so that
                                   the caller can exchange a finished range while the next one is
                                   being solved; 0 = one chunk                                  */
  int32_t gramian_mode;         /* arithmetic of the per-row Gramian sum (c-1) y y^T (ALS:471-477):
                                   MALS_GRAMIAN_FP32: fp32 products, fp32 accumulate;
                                   MALS_GRAMIAN_SPLIT_F16: operands split into two f16 halves (22
                                   significand bits), exact products, fp32 accumulate (the rank-16
                                   updates of the factorization use the same operands) -- 2.5x less
                                   matrix-pipe time, rounding error on a par with FP32 (measured
                                   2-4e-7 vs the fp64 reference for both);
                                   MALS_GRAMIAN_SPLIT3_F16 (features 49..64 only; a measured alternative,
                                   DESIGN.md section 6): THREE f16 terms per operand -- every fp32 operand
                                   exactly -- and the six products at or above 2^-24 of the leading one:
                                   fp32-operand arithmetic on the f16 pipe, twice SPLIT_F16's matrix time;
                                   MALS_GRAMIAN_AUTO (default): FP32 for features <= 16 (where the
                                   products are not the bottleneck), SPLIT_F16 above            */
  int32_t solve_mode;           /* how a row with FEWER ENTRIES THAN FEATURES is solved (ALS:447-494 is the
                                   same k x k system either way):
                                   MALS_SOLVE_DIRECT: the k x k system W x = b, whatever the row length;
                                   MALS_SOLVE_DUAL: rows with n_u <= 16*floor(ceil(k/16)/2) entries through
                                   the n_u x n_u system of the push-through identity in the eigenbasis of
                                   the shared Gramian (csrc/dual_kernels.h: same x, 8x fewer factorization
                                   flops at n_u <= k/2), the others directly; needs the reference's default
                                   mode (flags = 0), alpha > 0 and min eig(G) + lambda*alpha >= 1e-4 and
                                   otherwise falls back to DIRECT for that half-iteration;
                                   MALS_SOLVE_AUTO (default): DUAL for features > 32, DIRECT below    */
} mals_config;

typedef struct mals_stats {
  int32_t struct_size;
  int32_t reserved;
  /* Accumulated since mals_reset_stats.  Times are HIP-event milliseconds measured on the handle's
   * stream around each kernel launch, only while timing is enabled (mals_enable_timing); bytes are
   * the ALGORITHMIC bytes of SURVEY.md section 8(d) attributed to that kernel's launches:
   * entries*(4k+4+4) gathered + rows*(4k+8) written.                                            */
  double rows_ms;           /* als_rows_kernel: fused gather+Gramian+Cholesky, rows <= segment_nnz */
  double segments_ms;       /* als_segments_kernel: gather+Gramian partials of long rows           */
  double finish_ms;         /* als_finish_kernel: partial sums + Cholesky of long rows             */
  double gramian_ms;        /* gramian_partial_kernel + gramian_finalize_kernel (K1)               */
  int64_t rows_launches;
  int64_t segments_launches;
  int64_t finish_launches;
  int64_t gramian_launches;
  double rows_bytes;
  double segments_bytes;
  double finish_bytes;
  double gramian_bytes;     /* rows*4k read                                                        */
  int64_t rows_solved;
  int64_t nnz_gathered;
  /* appended in ABI version 2 */
  double dual_ms;           /* als_dual_kernel: short rows through the n_u x n_u system               */
  double rotate_ms;         /* rotate_rows_kernel: M Q before, x = Q x' after the dual kernels        */
  int64_t dual_launches;
  int64_t rotate_launches;
  double dual_bytes;        /* entries*(4k+8) + rows*(4k+8), like rows_bytes                          */
  double rotate_bytes;      /* rows*(4k + 64*ceil(k/16)) forward, rows*8k in place                    */
  int64_t rows_dual;        /* rows solved by the dual kernels (included in rows_solved)              */
  double eigen_host_ms;     /* host time of the k x k eigendecompositions (overlapped with kernels)   */
  int64_t rows_refined;     /* rows re-solved with fp64 residuals (mals_set_refine_limit)             */
} mals_stats;

int mals_abi_version(void);

/* Fill cfg with the reference's defaults (k=30, alpha=1, lambda=0.1, threshold 1e-5;
 * MatrixFactorizer.java:34, ALS:71-75). */
int mals_default_config(mals_config* cfg);

/* Create a handle on cfg->device.  Replaces `new AlternatingLeastSquares(...)` (ALS:132-147). */
int mals_create(const mals_config* cfg, mals_handle* out);
int mals_destroy(mals_handle h);

/* Why the last mals_create / mals_group_create / mals_group_create_rank / mals_group_unique_id ON THIS THREAD failed --
 * there is no handle to ask then ("no HIP device", "device ordinal 3 outside 0..0", "librccl.so.1: cannot open ...",
 * "ncclCommInitAll: ...").  Copies at most cap - 1 characters + NUL into buf, returns the full length ("" / 0 after a
 * success).  mals_group_create_error is the same call under the group's name.  What the JVM adapter puts into the
 * ExecutionException instead of a bare "create failed" (jni/myrrix_als_jni.c nativeCreateError). */
int mals_create_error(char* buf, size_t cap);
int mals_group_create_error(char* buf, size_t cap);

/* cfg.features of the handle (0 for a null handle): lets a binding size-check factor and query-vector arrays. */
int mals_features(mals_handle h);

/* Human-readable message for the last non-OK status on this handle ("" if none). */
const char* mals_last_error(mals_handle h);

/* Use an existing hipStream_t (e.g. the caller's current stream) for all work; NULL = default. */
int mals_set_stream(mals_handle h, void* hip_stream);

/* Declare the number of rows of a side's factor replica and (re)allocate it zero-filled, unless
 * the caller binds its own device buffer with mals_bind_factors. */
int mals_set_factor_rows(mals_handle h, int side, int64_t n_rows_total);

/* Use caller-owned device memory (row-major n_rows_total x features fp32) as the factor replica
 * of `side`.  The caller keeps it alive until mals_destroy or the next bind. */
int mals_bind_factors(mals_handle h, int side, float* device_ptr, int64_t n_rows_total);

/* Device pointer of the factor replica of `side` (for the caller's collective). */
int mals_factor_device_ptr(mals_handle h, int side, void** out_device_ptr, int64_t* out_n_rows_total);

/* Upload the local matrix rows of a side: rows [row_offset, row_offset+n_rows_local) of R (side X)
 * or R^T (side Y) in CSR with local row_ptr (n_rows_local+1 entries, row_ptr[0]=0), col_idx indexing
 * rows of the OPPOSITE side's factor replica.  This is what iterating RbyRow / RbyColumn delivers
 * (ALS:399,455).  mem_kind = MALS_MEM_DEVICE borrows the caller's device arrays (no copy; keep
 * them alive); MALS_MEM_HOST copies.  n_u of a row = its entry count (ALS:488 ru.size()). */
int mals_set_matrix(mals_handle h, int side, int64_t row_offset, int64_t n_rows_local, int64_t nnz,
                    const int64_t* row_ptr, const int32_t* col_idx, const float* val, int mem_kind);

/* Chunked variant for callers that cannot hold one array per matrix (Java arrays are < 2^31):
 * begin, then append consecutive row chunks (host memory; row_ptr_chunk has n_rows+1 entries
 * starting at 0), then end. */
int mals_begin_matrix(mals_handle h, int side, int64_t row_offset, int64_t n_rows_local, int64_t nnz);
int mals_append_rows(mals_handle h, int side, int64_t n_rows, const int64_t* row_ptr_chunk,
                     const int32_t* col_idx, const float* val);
int mals_end_matrix(mals_handle h, int side);

/* Largest |value| of the local matrix rows of `side` (computed at upload), and an override for it.
 * The split-precision Gramian takes its operand scale from this bound; a multi-GPU caller installs
 * the maximum over all shards so that every rank uses the same scale and the factors do not depend
 * on how the rows are sharded.  The override must be >= the local maximum. */
int mals_get_value_bound(mals_handle h, int side, float* max_abs_value);
int mals_set_value_bound(mals_handle h, int side, float max_abs_value);
/* The same with the second statistic the split-precision gather looks at: sum of |value| and number of
 * entries of the local rows (their ratio is the "typical" weight of the operand-range check that decides
 * per launch between the split-precision and the fp32 gather).  A multi-GPU caller adds the sums and
 * counts of all shards and installs max and mean everywhere. */
int mals_get_value_stats(mals_handle h, int side, float* max_abs_value, double* sum_abs_value, int64_t* n_values);
int mals_set_value_stats(mals_handle h, int side, float max_abs_value, double mean_abs_value);

/* Host <-> device factor rows.  setPreviousY (ALS:172-174) = mals_set_factors(MALS_SIDE_Y, ...);
 * getX()/getY() (ALS:149-157) = mals_get_factors. */
int mals_set_factors(mals_handle h, int side, int64_t row_begin, int64_t n_rows, const float* host_rows);
int mals_get_factors(mals_handle h, int side, int64_t row_begin, int64_t n_rows, float* host_out);
int mals_get_rows(mals_handle h, int side, const int64_t* row_idx, int32_t n, float* host_out);

/* K1.  G = M^T M over ALL rows of `side`'s factor replica (MU:219-239 as called at ALS:342,369),
 * fp64, left on the device for the next mals_solve_side of the OTHER side; optionally copied to
 * host_G (features*features doubles, row-major) when host_G != NULL. */
int mals_gramian(mals_handle h, int side, double* host_G);

/* Multi-GPU variant: partial Gramian of rows [row_begin,row_begin+n_rows) of `side`'s replica into
 * device_out (features*features doubles); the caller all-reduces and installs the sum. */
int mals_gramian_partial(mals_handle h, int side, int64_t row_begin, int64_t n_rows, double* device_out);
int mals_set_gramian(mals_handle h, int side, const double* G, int mem_kind);

/* K2+K3.  Solve the local rows of `side` from the opposite side's factors and Gramian
 * (ALS:391-410 addWorkers + ALS:432-504 Worker.call): per row W = G + sum (c-1) y y^T +
 * lambda*alpha*n_u I, b = sum_{r>0} c y, x = W^-1 b, written into rows
 * [row_offset, row_offset+n_rows_local) of `side`'s factor replica.  Asynchronous on the handle's
 * stream; errors (singular rows) are reported by the next mals_check. */
int mals_solve_side(mals_handle h, int side);

/* The same for one chunk: local rows [chunk*cfg.chunk_rows, (chunk+1)*cfg.chunk_rows) of the shard
 * (all chunks, in any order, = mals_solve_side).  mals_num_chunks = ceil(n_rows_local/chunk_rows). */
int mals_solve_chunk(mals_handle h, int side, int32_t chunk);
int mals_num_chunks(mals_handle h, int side, int32_t* n_chunks);
/* cfg.chunk_rows for one side only (the two sides of a shard usually differ in size); takes effect at the
 * next matrix upload of that side.  0 = one chunk. */
int mals_set_chunk_rows(mals_handle h, int side, int64_t chunk_rows);

/* Synchronise the stream and report MALS_SINGULAR if any row solved since the last check had a
 * non-positive-definite system (the reference throws SingularMatrixSolverException, CMLSS:46-54). */
int mals_check(mals_handle h);
/* Details of the last MALS_SINGULAR: the side, the (global) row -- -1 when it was a model Gramian
 * (mals_recompute_solver) -- and the apparent rank the reference would report (CMLSS:47,
 * RRQRDecomposition.getRank(0.01)), which DelegateGenerationManager.java:345-354 uses to lower
 * model.features and retry.  For a row, the rank is recomputed on the host in fp64 from the row's
 * entries and the CURRENT opposite factors / Gramian, i.e. it is exact when the check directly
 * follows the solve (mals_half_iteration, mals_factorize); 0 = could not be determined. */
int mals_singular_info(mals_handle h, int32_t* side, int64_t* row, int32_t* apparent_rank);

/* iterateXFromY (ALS:340-362) for side X, iterateYFromX (ALS:367-389) for side Y:
 * mals_gramian(opposite) + mals_solve_side(side) + mals_check. Single-GPU convenience. */
int mals_half_iteration(mals_handle h, int side);

/* call() (ALS:176-262) on one GPU: alternate half-iterations until the convergence rule fires.
 * test_users / test_items: dense indices of the convergence sample (the adapter draws them with the
 * reference's own RandomUtils.chooseAboutNFromStream, ALS:206-215).  random_y: Y was random
 * (ALS:181,253).  iterate = 0: model.als.iterate=false (ALS:196-204).  max_iterations <= 0: no cap. */
int mals_factorize(mals_handle h, double convergence_threshold, int32_t max_iterations,
                   int32_t random_y, int32_t iterate, const int64_t* test_users, int32_t n_test_users,
                   const int64_t* test_items, int32_t n_test_items, int32_t* iterations_out,
                   double* convergence_out);

/* The convergence sample on the device (ALS:230-238): host_out[i*n_test_items+j] =
 * SimpleVectorMath.dot(X[test_users[i]], Y[test_items[j]]) (float product, double sum, features in order --
 * bit-identical to the Java loop) from the resident factors; 8 bytes per pair cross PCIe instead of the
 * sampled rows.  mals_factorize / mals_group_factorize use it every iteration and keep only the
 * order-dependent DoubleWeightedMean on the host. */
int mals_sample_dots(mals_handle h, const int64_t* test_users, int32_t n_test_users, const int64_t* test_items,
                     int32_t n_test_items, double* host_out);

/* The host eigensolver of the dual path (csrc/host_eigen.h; no GPU needed): A = V diag(evals) V^T for a symmetric
 * row-major n x n matrix (Householder tridiagonalisation + implicit QR; evals in no particular order, column j of
 * the row-major V is the unit eigenvector of evals[j]).  MALS_INVALID_ARG for a non-finite input or no convergence. */
int mals_symmetric_eigen(const double* A, int32_t n, double* evals_out, double* V_out);

/* Cooperative cancellation (InterruptedException path, MatrixFactorizer.java:43-44): checked
 * between half-iterations of mals_factorize. */
int mals_cancel(mals_handle h);

/* ---- the model-load consumer of K1 --------------------------------
 * Generation.recomputeSolver (online/src/net/myrrix/online/generation/Generation.java:142-158):
 * M^T M of `side`'s factors (K1 on the device), its max-abs-column-sum norm (getNorm(), :149), and
 * MatrixUtils.getSolver(M^T M) (MU:137, CMLSS:37-55).  The k x k factorization is host fp64.
 *   MALS_OK, *out = NULL        the side has no factor rows ("M == null || M.isEmpty()", :145)
 *   MALS_ILL_CONDITIONED        norm < 1.0 (:150-153); *inf_norm_out holds the norm
 *   MALS_SINGULAR               getSolver threw; rank via mals_singular_info (row = -1)
 * The Gramian stays installed on the device like after mals_gramian. */
typedef struct mals_solver_s* mals_solver;
int mals_recompute_solver(mals_handle h, int side, mals_solver* out, double* inf_norm_out);

/* MatrixUtils.getSolver(A) for a caller-supplied row-major n x n matrix (host only, no device
 * needed).  MALS_SINGULAR: *apparent_rank_out = getRank(0.01) and *out = NULL. */
int mals_solver_create(const double* A, int32_t n, double singularity_threshold, mals_solver* out,
                       int32_t* apparent_rank_out);
int mals_solver_dim(mals_solver s);
/* Solver.solveDToF / solveFToD (Solver.java:35-41, CommonsMathSolver.java:37-59). */
int mals_solver_solve_dtof(mals_solver s, const double* b, float* x);
int mals_solver_solve_ftod(mals_solver s, const float* b, double* x);
int mals_solver_destroy(mals_solver s);

/* ---- reconstruction metric on the device -------------------------------
 * ReconstructionEvaluator.evaluate (online/src/net/myrrix/online/eval/ReconstructionEvaluator.java:
 * 91-102): over every stored entry (u,i) of the local rows of side X, err = max(0, 1 - dot(X_u, Y_i))
 * with SimpleVectorMath.dot (fp32 products, fp64 sum).  Returns the sum and the number of entries; the
 * evaluator's result is sum/count (a multi-GPU caller adds the ranks' sums and counts first).
 * (The convergence statistic of call() already crosses PCIe as 200 sampled rows only, mals_factorize.) */
int mals_reconstruction_error(mals_handle h, double* sum_out, int64_t* count_out);

/* ---- top-N scoring -------------------------------------------------------
 * ServerRecommender.recommend(userID, howMany, considerKnownItems, null) (online/src/net/myrrix/online/
 * ServerRecommender.java:382-441) -> multithreadedTopN (:443-508) -> RecommendIterator (RecommendIterator.
 * java:62-109) -> TopN (common/src/net/myrrix/common/TopN.java:49-128), for a batch of model users given by
 * their dense indices.  The score of item i IS the reference's: (float)(sum_j dot(Y_i, f_j) / n) over the
 * query's n vectors with SimpleVectorMath.dot (every product rounded to fp32, fp64 sum in feature order,
 * RecommendIterator.java:93-104) -- bit-identical; the user's known items (the entries of its row of R on this
 * handle) are skipped unless consider_known_items; the how_many best come back best first, equal scores in
 * ascending item index (the reference leaves ties in hash order).  item_idx_out / score_out: n_queries x
 * how_many, padded with -1 / -inf; n_out (may be NULL): results per query.  Rescorers (mals_rescorer_*), the
 * candidate filter (mals_lsh_*) and tag items (mals_set_tag_items) run on the device too.  On large item sets a bf16 MFMA pass with a
 * proven error margin only narrows the items down to a few hundred candidates per query, whose scores are then
 * computed exactly (csrc/topn_kernels.h); Y is streamed once per up to 240 queries, the passes of a call overlap
 * on six internal streams (ordered after the work already on the handle's stream; the call returns when all have
 * finished). */
int mals_recommend(mals_handle h, const int64_t* user_idx, int32_t n_queries, int32_t how_many, int32_t consider_known_items,
                   int64_t* item_idx_out, float* score_out, int32_t* n_out);
/* THREADS.  The reference's top-N is entered by every request thread at once, one user per call (ServerRecommender.java:
 * 359-441 -> multithreadedTopN :443-508).  mals_recommend, mals_recommend_vectors and mals_recommend_to_many may be
 * called on ONE handle from any number of threads concurrently (with each other -- not with calls that change the
 * handle's matrices, factors, known or tag items).  A call is cheap only as part of a pass (one read of Y answers up to 240
 * queries), so concurrent calls are folded into passes behind the ABI: every call becomes a ticket in the handle's queue;
 * the first thread that finds no leader leads -- it packs the queued calls of fewer than 64 queries into the next pass
 * (by-user calls together, calls with their own vectors -- an anonymous user, recommendToMany -- together), enqueues it,
 * decodes finished passes, wakes their callers -- and hands leadership on when its own answer is there.
 * At most `passes_in_flight` passes (default 2, environment MALS_TOPN_FRONT_DEPTH at mals_create) are on the device at a
 * time; what arrives meanwhile forms the next one.  Larger calls run exclusively, in queue order.  Every result is what the
 * call alone would have returned (bit-identical).  mals_recommend_front_stats:
 * out4 = {calls, queries, coalesced passes, exclusive calls} since mals_create. */
int mals_recommend_front_stats(mals_handle h, int64_t* out4);
int mals_recommend_set_depth(mals_handle h, int32_t passes_in_flight);   /* 1..6; not while calls are in flight */
/* How long a caller whose call is in somebody else's pass polls for its answer before it blocks on a condition variable
 * (default 0: block at once; a process with cores to spare trades them for wake-up latency). */
int mals_recommend_set_spin_us(mals_handle h, int32_t spin_us);
/* userTagIDs (RecommendIterator.java:72 -- "if (userTagIDs.contains(itemID)) return null"; likewise MostSimilarItemIterator
 * .java:77): rows of Y that stand for tags of users (InputFilesReader.java:159-165) are never recommended, to anybody, by
 * any mals_recommend* call.  item_idx: n dense item indices (host or device; entries outside [0, rows of Y) are ignored:
 * a tag whose entries were all removed owns no row).  n = 0 clears.  Needs the item factor rows declared
 * (mals_set_factor_rows).  mals_ingest_install / mals_ingest_install_group hand the ingest's userTagIDs over. */
int mals_set_tag_items(mals_handle h, int64_t n, const int64_t* item_idx, int mem_kind);
int mals_get_tag_item_count(mals_handle h, int64_t* n_out);   /* distinct rows of Y currently struck */
/* The same for caller-supplied query vectors (n_queries x features, host) -- anonymous users / fold-in
 * (SR:561-606) -- with optional per-query lists of item indices to skip (CSR: exclude_ptr has
 * n_queries+1 entries; both NULL = none). */
int mals_recommend_vectors(mals_handle h, const float* query_vectors, int32_t n_queries, int32_t how_many,
                           const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out, float* score_out,
                           int32_t* n_out);
/* knownItemIDs for mals_recommend (ServerRecommender.java:394-425 takes them from generation.getKnownItemIDs(), which
 * differ from the rows of R by the entries InputFilesReader.removeSmall pruned): a CSR over the handle's local user rows
 * (n_rows = the local rows of side X) of dense item indices.  MALS_MEM_DEVICE arrays are borrowed, host arrays copied.
 * row_ptr NULL: back to the rows of R.  mals_ingest_install hands them over when the ingest built them. */
int mals_set_known_items(mals_handle h, int64_t n_rows, const int64_t* row_ptr, const int32_t* item_idx, int mem_kind);
/* ... and for queries of SEVERAL vectors each -- recommendToMany (ServerRecommender.java:366-441: the feature
 * vectors of all the users asked for; the caller passes the intersection of their known items, :398-425, as the
 * exclusion list): query q owns vectors[vector_ptr[q] .. vector_ptr[q+1]) (rows of `vectors`, features floats
 * each; at least one: RecommendIterator.java:52), its score is the mean of the dots, divided last
 * (RecommendIterator.java:93-104).  vector_ptr NULL = one vector per query. */
int mals_recommend_to_many(mals_handle h, const float* vectors, const int64_t* vector_ptr, int32_t n_queries, int32_t how_many,
                           const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out, float* score_out,
                           int32_t* n_out);

/* ---- rescorers: RecommendIterator's IDRescorer on the device ----------------------------------------------------
 * RecommendIterator.next (online/src/net/myrrix/online/RecommendIterator.java:62-109) with an IDRescorer of the shape the
 * reference's own FilterHalfRescorerProvider has -- a filter set and an affine rescore -- as a native object:
 *     isFiltered(i) = i is in the filter set;   rescore(i, sum) = fl(fl(scale_i * sum) + offset_i)   (fp64, no contraction)
 * Per candidate item, in the reference's order: userTagIDs, known / excluded items and filtered items are skipped; sum = the
 * fp64 sum of the dots over the query's n vectors (unchanged); r = rescore(i, sum) -- on the SUM, before the division; an
 * r that is not finite skips the item (never an error); the score is (float)(r / n), and a score that is not finite fails
 * THAT CALL with MALS_INVALID_ARG, "Bad recommendation value" (checkState, :105) -- the other calls folded into the same
 * pass are answered as if alone.  Scores and indices are bit-identical to the reference running a Java IDRescorer that
 * computes the same formula (java/.../NativeIDRescorer.java); ties in ascending item index.
 * A rescorer is bound to one handle; it starts as the identity (nothing filtered, scale 1, offset 0).
 *   mals_rescorer_set_filter(r, n, item_idx, mem_kind): the filter set, n dense item indices in [0, rows of Y) (host or
 *     device); n = 0 clears it.
 *   mals_rescorer_set_weights(r, scale, offset, n_rows, mem_kind): per-item fp64 weights of rows [0, n_rows) (host or
 *     device); either array may be NULL (scale 1 / offset 0).  Every scale must be finite and > 0, every offset finite
 *     (an item a Java rescorer scores NaN belongs in the filter set): else MALS_INVALID_ARG and nothing changes.  Replaces
 *     the uniform weights (back to 1, 0).
 *   mals_rescorer_set_uniform(r, scale, offset): the same weights for every item, no arrays; replaces the per-item weights.
 * Rows of Y the arrays do not cover (rows added by mals_grow_factor_rows among them) are unfiltered, with scale 1 and
 * offset 0 -- or the uniform weights.  Every set_* is an exclusive ticket of the serving front (as the fold-in writes): a
 * call sees the rescorer as it was when the call was queued.  mals_rescorer_destroy: not while a call that names it is in
 * flight; before the handle is destroyed.
 * The rescored twins of mals_recommend, mals_recommend_to_many (which covers mals_recommend_vectors: vector_ptr NULL) and
 * mals_recommend_to_anonymous take the rescorer as their second argument (NULL: exactly the plain call).  Calls with the
 * same rescorer (or none), kind and how_many are folded into one pass; different rescorers never share one.  The filter
 * path runs on rescorers whose unfiltered weights lie in scale [2^-20, 2^20], |offset| <= 2^64 (csrc/topn_kernels.h,
 * RESCORED MODE: the bound); the calls of any other rescorer are answered exactly by the dense path, one call at a time. */
typedef struct mals_rescorer_s* mals_rescorer;
int mals_rescorer_create(mals_handle h, mals_rescorer* out);
int mals_rescorer_destroy(mals_rescorer r);
int mals_rescorer_set_filter(mals_rescorer r, int64_t n, const int64_t* item_idx, int mem_kind);
int mals_rescorer_set_weights(mals_rescorer r, const double* scale, const double* offset, int64_t n_rows, int mem_kind);
int mals_rescorer_set_uniform(mals_rescorer r, double scale, double offset);
int mals_recommend_rescored(mals_handle h, mals_rescorer r, const int64_t* user_idx, int32_t n_queries, int32_t how_many,
                            int32_t consider_known_items, int64_t* item_idx_out, float* score_out, int32_t* n_out);
int mals_recommend_to_many_rescored(mals_handle h, mals_rescorer r, const float* vectors, const int64_t* vector_ptr, int32_t n_queries,
                                    int32_t how_many, const int64_t* exclude_ptr, const int64_t* exclude_idx, int64_t* item_idx_out,
                                    float* score_out, int32_t* n_out);
int mals_recommend_to_anonymous_rescored(mals_handle h, mals_rescorer r, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row,
                                         const float* values, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out,
                                         int32_t* status_out);

/* ---- the candidate filter: LocationSensitiveHash on the device ------------------------------------------------
 * When model.lsh.sampleRatio < 1 the reference's Generation builds a LocationSensitiveHash over Y (online/src/net/myrrix/
 * online/candidate/LocationSensitiveHash.java:89-152, chosen by CandidateFilterFactory.java:50-71) and multithreadedTopN
 * (ServerRecommender.java:443-508) only sees the items it returns for the query's vectors.  Built on a handle, every
 * mals_recommend, mals_recommend_vectors, mals_recommend_to_many, mals_recommend_to_anonymous call and their rescored twins
 * behave the same way:
 *   item i is a candidate of a query iff bitCount(sig_i ^ sig(f_j)) <= max_bits_differing for ANY of the query's vectors f_j
 *   (LSH:193-216), or i is a new item: a row of Y added by mals_grow_factor_rows after the build (addItem, LSH:219-225).
 * sig = toBitSignature (LSH:169-190): per hash, in order, the fp64 sum over the features, in order, of +-((double)v[f] -
 * mean[f]); the bit is sum > 0.0; hash 0 is the most significant of the num_hashes bits -- bit-identical to the reference
 * given the same mean and random vectors.  Signatures are a snapshot: a fold-in write that moves a row of Y does not change
 * its signature (the reference buckets once per generation).  Everything after candidacy is unchanged (tag, known, excluded
 * and rescorer-filtered items, the score arithmetic, ties in ascending item index); a query with fewer candidates than
 * how_many returns fewer results.  mals_most_similar_items, mals_similarity_to_item, mals_recommended_because and
 * mals_estimate_* never consult the filter (the reference passes none there).
 *   mals_lsh_max_bits_differing: LSH:98-108 on the host, no device, no handle: sample_ratio in (0, 1], num_hashes in 1..64;
 *     the result may be -1 (no bucket matches: only new items are candidates).
 *   mals_lsh_build: random_vectors = [num_hashes][features] bytes 0 / 1 (host), hash-major as the reference draws them
 *     (LSH:113-119); mean = features doubles (host), or NULL: computed on the device from the rows of Y (the fp64 sum of
 *     the rows in a fixed order / rows -- the same bits on every run; the reference's own order is its hash map's).  Signs
 *     every row of Y present now; replaces an earlier build.  An exclusive ticket of the serving front, like
 *     mals_rescorer_set_*: calls queued before it see the old filter, calls after it the new one.
 *   mals_lsh_clear: back to every item a candidate.  Declaring Y's rows anew (mals_set_factor_rows / mals_bind_factors on
 *     side Y) clears the filter too.  Those two calls are no tickets of the serving front: like every call that changes the
 *     handle's matrices or factors (THREADS, above) they must not run while mals_recommend* or mals_lsh_* calls are in flight.
 *   mals_lsh_info: out6 = {num_hashes (0: none), max_bits_differing, rows signed at build, rows of Y now, queries answered
 *     with the filter on by the bf16 filter path, ... by the dense path}.
 *   mals_lsh_get: the mean (features doubles; may be NULL) and the signatures of rows [row_begin, row_begin + n_rows) of the
 *     rows signed at build.
 *   mals_lsh_signatures: toBitSignature of n caller vectors (n x features, host) with the built mean and random vectors.
 * Not for members of a group: the mals_group_* twins are out of scope. */
int mals_lsh_max_bits_differing(double sample_ratio, int32_t num_hashes, int32_t* out);
int mals_lsh_build(mals_handle h, int32_t num_hashes, int32_t max_bits_differing, const uint8_t* random_vectors, const double* mean);
int mals_lsh_clear(mals_handle h);
int mals_lsh_info(mals_handle h, int64_t* out6);
int mals_lsh_get(mals_handle h, double* mean_out, int64_t row_begin, int64_t n_rows, uint64_t* signatures_out);
int mals_lsh_signatures(mals_handle h, const float* vectors, int32_t n, uint64_t* out);

/* ---- item-to-item similarity on the device ------------------------------------------------------------
 * ServerRecommender.mostSimilarItems (online/src/net/myrrix/online/ServerRecommender.java:1171-1266, scored by
 * MostSimilarItemIterator.java:73-120): for query q of items i_1..i_n (dense item indices; item_ptr NULL: one item per
 * query, else query q owns item_idx[item_ptr[q] .. item_ptr[q+1]), at least one) the score of item i is
 * (float)((s_1 + ... + s_n) / n), s_j = dot(Y_i, Y_ij) / (norm(Y_i) * norm(Y_ij)) in fp64 (SimpleVectorMath.dot and .norm:
 * fp32 products / squares, fp64 sums in feature order; the product of the norms first, then the division) -- bit-identical;
 * n counts duplicates.  Skipped: tag items (:77), the query's own items (:81-85), items with a non-finite s_j (:104: a
 * zero or NaN row, or a query item of zero norm, gives fewer results, never an error).  The how_many best come back best
 * first, ties in ascending item index; padding -1 / -inf; n_out (may be NULL): results per query.  Mapping IDs to indices
 * stays with the caller; a Rescorer<LongPair> is mals_most_similar_items_rescored, below.  An index outside [0, rows of Y) is MALS_INVALID_ARG; how_many in 1..4096.  The same
 * filter as mals_recommend (a bf16 MFMA pass with a proven cosine margin, then the exact rescore; csrc/topn_kernels.h)
 * over the resident Y.  Threads: as mals_recommend* (any number of request threads, together with recommend calls); calls
 * of fewer than 64 queries are folded into passes of their own kind, larger ones run exclusively. */
int mals_most_similar_items(mals_handle h, const int64_t* item_idx, const int64_t* item_ptr, int32_t n_queries, int32_t how_many,
                            int64_t* item_idx_out, float* score_out, int32_t* n_out);
/* mostSimilarItems(long[] itemIDs, int howMany, Rescorer<LongPair> rescorer) (ServerRecommender.java:1180-1265, scored by
 * MostSimilarItemIterator.java:87-117) with a mals_rescorer (above) as the pair rescorer.  For the pair (candidate c, query
 * item q_j):
 *     isFiltered(pair) = c is in the filter set F; with MALS_SIMILAR_FILTER_QUERY_ITEMS in `flags` also q_j in F -- "either
 *         end of the pair", the shape of FilterHalfRescorerProvider.getMostSimilarItemsRescorer.  A query with a filtered query
 *         item then comes back empty (n_out = 0), which is no error;
 *     rescore(pair, s) = fl(fl(scale_c * s) + offset_c)   (fp64, no contraction)
 * Per candidate, in the order of MostSimilarItemIterator.next(): 1. tag items are struck (:77); 2. the query's own items are
 * struck (:81-85); 3. for each query item j in order: a filtered pair skips the candidate; s_j = the cosine of
 * mals_most_similar_items, not finite skips the candidate; r_j = rescore(pair, s_j), not finite skips the candidate (:109),
 * never an error; total += r_j; 4. the result is (float)(total / n).  A result that is not finite fails THAT CALL with
 * MALS_INVALID_ARG, "Bad similarity value" (checkState, :117); the other calls folded into the same pass are answered as if
 * alone.  The rescore is PER TERM -- unlike mals_recommend_rescored, where it acts on the sum before the division: with n >= 2
 * query items the offset is added n times and divided once, so the mean is scale_c * mean(s_j) + offset_c up to rounding, with
 * no 1 / n on the offset.  Ties in ascending item index, padding -1 / -inf, how_many in 1..4096, as mals_most_similar_items.
 * r = NULL is exactly mals_most_similar_items (same kernels, same bits); a rescorer bound to another handle is
 * MALS_INVALID_ARG.  Threads: a ticket of the serving front like the other rescored calls; calls with the same rescorer, flags
 * and how_many and fewer than 64 queries fold into passes of their own, different rescorers never share a pass, and
 * mals_rescorer_set_* stays an exclusive ticket: a call sees the rescorer as it was when queued.  The filter path runs for
 * rescorers whose unfiltered weights lie in scale [2^-20, 2^20], |offset| <= 2^6 * scale (csrc/topn_kernels.h, RESCORED COSINE
 * MODE: the bound), up to four items outside that range allowed (candidates of every query; the exact rescore decides); any
 * other rescorer is answered exactly by the dense path, one call at a time.  Not for members of a group.
 * mals_similar_stats: out4 = {mostSimilarItems queries answered by the filter path, ... by the dense path (the fallbacks of a
 * filter pass included), ... answered empty by a filter pass before scoring (a dead or a filtered query item), the rescored
 * queries among all of these} since mals_create; plain and rescored calls both count; read without a ticket. */
enum { MALS_SIMILAR_FILTER_QUERY_ITEMS = 1 };
int mals_most_similar_items_rescored(mals_handle h, mals_rescorer r, int32_t flags, const int64_t* item_idx, const int64_t* item_ptr,
                                     int32_t n_queries, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out);
int mals_similar_stats(mals_handle h, int64_t* out4);
/* ServerRecommender.similarityToItem (ServerRecommender.java:1268-1304): out[j] = (float)(dot(Y_ij, Y_to) / (norm(Y_ij) *
 * norm(Y_to))) for the n items item_idx[j]; NaN is returned as NaN (no skip, no exclusion). */
int mals_similarity_to_item(mals_handle h, int64_t to_item, const int64_t* item_idx, int32_t n, float* out);
/* ServerRecommender.recommendedBecause (ServerRecommender.java:1324-1376, scored by RecommendedBecauseIterator.java:61-75):
 * for query q the candidates are the known items of user user_idx[q] (global row of X in this handle's local shard):
 * mals_set_known_items if installed, else the user's row of R -- the lists mals_recommend skips.  Score (float)(dot(Y_c,
 * Y_item) / (norm(Y_c) * norm(Y_item))) with item = item_idx[q]; tag items and non-finite scores skipped; item itself is
 * NOT excluded.  Outputs and order as mals_most_similar_items; exact for lists of any length. */
int mals_recommended_because(mals_handle h, const int64_t* user_idx, const int64_t* item_idx, int32_t n_queries, int32_t how_many,
                             int64_t* item_idx_out, float* score_out, int32_t* n_out);

/* ---- the online write path: setPreference / removePreference and the fold-in reads -------------------------------
 * ServerRecommender (online/src/net/myrrix/online/ServerRecommender.java) changes the model on every write between two
 * generations; these calls do it to the X, Y and known items resident on the device, in the reference's arithmetic (every
 * result bit-identical to the CPU restatement tests/foldin_oracle.py).  For handles OUTSIDE a group: a member's handle is
 * refused (MALS_INVALID_ARG); a group is written and read through the mals_group_* twins further down, which route every
 * user's known items to their owner.  Rows are dense indices (user = row of X,
 * item = row of Y); ids become rows through the id directory (mals_ids_* below), a tag's id is mals_tag_id_host of the tag
 * (setUserTag / setItemTag: mals_set_user_tags / mals_set_item_tags); the candidate filter, clustering and
 * generationManager.append stay with the caller.
 * THREADS: every call below may be made from any thread while mals_recommend* / similarity calls run on the same handle.
 * Each (but mals_foldin_stats) is an exclusive ticket in the serving front's queue -- mals_recommend_to_anonymous is two,
 * see there: passes formed before it see the old model, passes formed after it the new one; concurrent writes are
 * applied one after another in queue order.
 *
 * The generation's solvers (Generation.getXTXSolver / getYTYSolver) on the device: s from mals_recompute_solver or
 * mals_solver_create (its factors are copied; s stays the caller's).  side X = the solver of X^T X, side Y = of Y^T Y;
 * s = NULL clears that side.  The writes never recompute them (the reference keeps them until the next generation). */
int mals_set_foldin_solver(mals_handle h, int side, mals_solver s);
/* FOLDIN_LEARN_RATE (ServerRecommender.java:98-99), default 1.0. */
int mals_set_foldin_learn_rate(mals_handle h, double rate);
/* out6 = {updates applied, updates failed, "fold in vector is large" warnings the reference would have logged (norm of
 * userFoldIn > BIG_FOLDIN_THRESHOLD = 1e4, counted once per branch that reads it, :889 and :899), levels run, device
 * nanoseconds of the level kernels (HIP events around them) over all calls, the same for the last call} of
 * mals_set_preferences since mals_create.  Read without a ticket: it never waits for a pass. */
int mals_foldin_stats(mals_handle h, int64_t* out6);
/* Solver.solveFToD on the device (the solve every write uses): x_out[q] = A^-1 (double) b[q] for n_rhs vectors of
 * features floats, with the solver of `side` -- bit-identical to mals_solver_solve_ftod. */
int mals_foldin_solve(mals_handle h, int side, const float* b, int32_t n_rhs, double* x_out);
/* setPreference (:770-836, updateFeatures :865-912) for n updates: the result is exactly what n calls in array order
 * leave.  Update t, from the rows as they stand after the earlier updates:
 *   estimate = dot(x_u, y_i) (fp32 products, fp64 sum); not finite: the update fails before anything changes (:982);
 *   w = foldInWeight(estimate, value) (:981-994); w == 0: only the known items change (:870-872);
 *   itemFoldIn = solveFToD_XTX(x_u), userFoldIn = solveFToD_YTY(y_i), both from the rows before the update;
 *   y_i[f] += (float)(w * itemFoldIn[f]) (XTX solver set), then x_u[f] += (float)(w * userFoldIn[f]) (YTY solver set);
 *   a non-finite delta stops that update at that element (:893 / :903): the elements before it keep their new values;
 *   in the item loop x_u is not touched; the known items do not change;
 *   the user's known items gain i.
 * Solvers: no XTX solver: only x_u moves.  An XTX solver WITHOUT a YTY solver: the reference's item branch reads
 * norm(userFoldIn) of a null vector and throws before anything changes -- every update with w != 0 fails so, and adds no
 * known item.  status_out (n, nullable): MALS_OK or the code of each update; the other updates of the batch go on.
 * Returns the code of the first failed update (array order), else MALS_OK.  Every row must be inside the replicas
 * (new users / items: mals_grow_factor_rows first) and every user inside this handle's local shard.  Every write makes
 * the next half-iteration recompute its Gramian.  Updates that touch disjoint rows run side by side on the device; an
 * update waits for the last earlier update of its user and of its item (a hot item updated m times is m levels). */
int mals_set_preferences(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, const float* value, int32_t* status_out);
/* setUserTag (:1076-1120) and setItemTag (:1122-1165) for n updates, in array order like mals_set_preferences and with
 * its status words, return code and row rules (dense rows: mals_ids_resolve / mals_grow_factor_rows first; a tag id is
 * mals_tag_id_host of the tag, and owns a row like any other id -- one that collides with a numeric id is the same row).
 *   mals_set_user_tags: the tag's row is a row of Y.  It joins the userTagIDs (the mask of mals_set_tag_items: the row is
 *     never recommended, similar or popular from then on; a handle without a mask gets one), then
 *     updateFeatures(x_user, y_tag, value) runs -- the update of mals_set_preferences, bit for bit.
 *   mals_set_item_tags: the tag's row is a row of X.  It joins the itemTagIDs (the tag users of mals_set_tag_users: the
 *     row is not counted by mals_most_popular_items), then updateFeatures(x_tag, y_item, value) runs.
 * Neither adds a known item.  The mark is made before the update and whatever becomes of it: a failed update (estimate not
 * finite, an X^T X solver without a Y^T Y solver) and a value of NaN (weight 0) leave it.  Each call is one exclusive
 * ticket; the rows are marked recent, so mals_load_generation carries them. */
int mals_set_user_tags(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* tag_item_row, const float* value, int32_t* status_out);
int mals_set_item_tags(mals_handle h, int64_t n, const int64_t* tag_user_row, const int64_t* item_row, const float* value, int32_t* status_out);
/* The tag sets as they stand (a ticket): side Y = userTagIDs as rows of Y, side X = itemTagIDs as user rows of this handle,
 * ascending.  *n_out = the set's size; rows_out (capacity cap, nullable when cap is 0) takes the first min(cap, size).  A
 * member of a group answers for itself: the mask every member holds, the tag users it owns (global rows). */
int mals_get_tag_rows(mals_handle h, int side, int64_t* rows_out, int64_t cap, int64_t* n_out);
/* tagHasher.toLongID(tag) (OneWayMigrator: the first 8 bytes of the MD5 of the tag's UTF-8 form, big-endian) of the tag whose
 * UTF-8 bytes are given: what the text parser makes of the token "<bytes>".  Host only, no handle. */
int mals_tag_id_host(const void* utf8, int64_t n_bytes, int64_t* id_out);
/* removePreference (:1001-1074) for n pairs in order: a user without known items, or an item the user does not know, is
 * ignored; otherwise the item leaves the user's known items, and when that empties them the user is removed: its row of
 * X is zeroed (a later setPreference recreates it from zeros, getFeatures :838-863) and reported in removed_users_out
 * (capacity n; *n_removed_out of them) -- the caller drops the id (NoSuchUserException from then on). */
int mals_remove_preferences(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, int64_t* removed_users_out,
                            int64_t* n_removed_out);
/* getFeatures (:838-863) for unseen users / items: grow a replica the library owns to n_rows_total rows (content kept, new
 * rows zero; capacity doubles, so a stream of new rows does not copy the replica each time).  A bound replica
 * (mals_bind_factors) is MALS_INVALID_ARG.  Side Y extends the userTagIDs with zeros; new users (side X) have no known
 * items and are valid users of mals_recommend / mals_recommended_because on this handle.  Iterations afterwards run on
 * the grown shapes.  The known-item changes of the writes (kept beside the installed known items / the rows of R, which
 * are never written) are dropped by mals_set_known_items, mals_set_matrix of side X and mals_ingest_install*. */
int mals_grow_factor_rows(mals_handle h, int side, int64_t n_rows_total);
/* estimatePreferences (:690-727): out[t] = (float)dot(x_u, y_i); a row of -1 (unknown user or item) gives 0.0f.  A
 * non-finite estimate is MALS_INVALID_ARG (checkState, :718); out still holds every value (the bad ones not finite). */
int mals_estimate_preferences(mals_handle h, int64_t n, const int64_t* user_row, const int64_t* item_row, float* out);
/* buildAnonymousUserFeatures (:561-609): query q owns the items item_row[item_ptr[q] .. item_ptr[q+1]) with values (NULL:
 * 1.0 each); rows -1 are skipped; out[q] = sum over the items in order of (float)(foldInWeight(0, value) *
 * solveFToD_YTY(y_item)[f]), accumulated in fp32 (n_queries x features).  A query without an item that has a row, or a
 * handle without a YTY solver, fails (status_out[q], nullable; the first failure's code is returned). */
int mals_anonymous_features(mals_handle h, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values,
                            float* out, int32_t* status_out);
/* recommendToAnonymous (:511-559): the vectors of mals_anonymous_features through mals_recommend_to_many, each query's
 * items excluded (and userTagIDs struck as always).  Failed queries (status_out) come back empty (-1 / -inf, n_out 0).
 * TWO tickets, the vectors and then the top-N: a write may land between them (the reference holds no lock across the
 * two steps either). */
int mals_recommend_to_anonymous(mals_handle h, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values,
                                int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out, int32_t* status_out);
/* estimateForAnonymous (:734-759): out[q] = (float)dot(anonymous features of query q, y_to_item[q]). */
int mals_estimate_for_anonymous(mals_handle h, int32_t n_queries, const int64_t* to_item, const int64_t* item_ptr, const int64_t* item_row,
                                const float* values, float* out, int32_t* status_out);

/* ---- the id directory: 64-bit ids <-> dense rows, resident on the handle -------------------------------------------
 * Per side the handle can hold row -> id (a dense device array) and id -> row (an open-addressing table on the device:
 * the slots and hash of mals_load_generation's join, at most half full, every 64-bit pattern a legal id), so that a
 * caller needs no dictionary of its own and no trip through the host per batch.  For handles OUTSIDE a group (a member
 * is MALS_INVALID_ARG, as on the write path).  Every call is an exclusive ticket of the serving front: a lookup sees
 * every resolve queued before it.
 * COVER: a side's directory must hold exactly one id per row of its replica.  Only mals_ids_resolve grows both together.
 * A side that was never set, or whose replica was grown by mals_grow_factor_rows directly, is refused by every call
 * below (MALS_INVALID_ARG; the message says which rows have no id) until mals_ids_set installs the ids of the rows as
 * they are.  Whatever renumbers or replaces a side's rows DROPS its directory: mals_load_generation (install the merged
 * ids it hands back: mals_generation_get_ids), mals_set_factor_rows, mals_bind_factors.
 * A user that mals_remove_preferences empties keeps its id and its zeroed row: a later set of that id finds the row,
 * which is exactly the vector getFeatures (:838-863) creates for a returning user.
 *
 * mals_ids_set: the ids of rows [0, n); n must be the rows of the side's replica; ids in host or device memory
 * (mem_kind), e.g. what mals_ingest_get_ids returned.  An id that appears twice is MALS_INVALID_ARG -- the message names
 * the smallest row that repeats an earlier row's id -- and nothing changes.  n = 0 with ids = NULL clears the side. */
int mals_ids_set(mals_handle h, int side, int64_t n, const int64_t* ids, int mem_kind);
/* rows_out[t] = the row of ids[t], or -1 if the directory does not know it (host arrays).  Changes nothing. */
int mals_ids_lookup(mals_handle h, int side, int64_t n, const int64_t* ids, int64_t* rows_out);
/* The same, except that an unknown id gets a new row: rows, rows + 1, ... in ORDER OF FIRST APPEARANCE in the batch,
 * every later occurrence of the id the same row -- the result of a dictionary that reads the batch front to back,
 * whatever the device's scheduling.  The replica grows as by mals_grow_factor_rows (new rows zero, userTagIDs extended,
 * new users own no known items, capacity doubling; a bound replica is MALS_INVALID_ARG and nothing changes); the table
 * is rebuilt at twice the slots -- as often as the batch needs -- before it would pass half full.  *n_new_out
 * (nullable): the rows added.  n <= 2^30. */
int mals_ids_resolve(mals_handle h, int side, int64_t n, const int64_t* ids, int64_t* rows_out, int64_t* n_new_out);
/* ids_out[j] = the id of row row_begin + j, j < n (host); *n_out = the rows that have an id. */
int mals_ids_get(mals_handle h, int side, int64_t row_begin, int64_t n, int64_t* ids_out);
int mals_ids_count(mals_handle h, int side, int64_t* n_out);

/* ---- mostPopularItems on the device -----------------------------------------------------------------------------
 * ServerRecommender.mostPopularItems(howMany, rescorer) (online/src/net/myrrix/online/ServerRecommender.java:611-673,
 * scored by MostPopularItemsIterator.java:51-67) over the known items resident on the handle, in the reference's order:
 *  1. Counted users: every user row this handle holds known items for -- the local shard and, on a handle outside a group,
 *     the rows mals_grow_factor_rows added -- except the rows named by mals_set_tag_users: the itemTagIDs, "users" that
 *     are really tags of items (:631-638).  mals_set_tag_users takes n GLOBAL user rows (host or device); rows outside the
 *     handle's users are ignored; n = 0 clears the set; nothing else reads it.  Like mals_set_tag_items it must not run
 *     while calls are in flight.  mals_set_matrix / mals_begin_matrix of side X drop the set (it named the old rows).
 *     mals_ingest_install hands the ingest's itemTagIDs over as user rows; mals_ingest_install_group and
 *     mals_group_ingest_finish do NOT: their callers use mals_group_set_tag_users.
 *  2. A user's set is its CURRENT known items: the replaced set after a removal, else the base row (the installed known
 *     items, or the user's row of R if none were installed) plus the items this generation's writes added.  It is a set:
 *     an item repeated in a caller-supplied row, or added again by a write, counts once; base rows need not be sorted.  A
 *     handle with neither a side-X matrix, nor known items, nor written known items is MALS_INVALID_ARG (the reference
 *     throws UnsupportedOperationException, :622).
 *  3. count(i) = the number of counted users whose set holds i.  Items with count 0 are no candidates whatever a
 *     rescorer's offset (they are not in itemCounts), nor are the rows of Y struck by mals_set_tag_items (userTagIDs,
 *     :657-667).
 *  4. value(i) = the float that count(i) increments by 1.0f reach (FastByIDFloatMap.increment, :644): (float)min(count(i),
 *     16777216) -- in fp32 2^24 + 1.0f rounds back to 2^24 (halfway, to even), so the reference's sum stays there.
 *  5. With a rescorer (r non-NULL, bound to this handle; MostPopularItemsIterator.java:56-63): a filtered item is skipped;
 *     value = (float) fl(fl(scale_i * (double)value) + offset_i), fp64 without contraction (the formula of
 *     mals_recommend_rescored); a value that is not finite after the cast to float skips the item -- never an error
 *     (this iterator has no checkState).  Always exact: the weight range of the bf16 filter does not apply.
 *  6. The how_many (1..4096) best come back best first, equal values in ascending item index (the library's rule; the
 *     reference leaves ties in hash order): ONE block of how_many entries in item_idx_out / score_out, padded with -1 /
 *     -inf; n_out (may be NULL): the results.  Counts are small integers, ties at the cut are the rule: the selection is a
 *     radix select over 64-bit (value, index) keys on the device, exact for any number of ties (csrc/popular_kernels.h);
 *     only the result block crosses to the host.  Needs the item factor rows declared (they say how many items there are).
 *  7. THREADS: an exclusive ticket of the serving front, like the fold-in reads: callable from any request thread while
 *     mals_recommend* calls are in flight; it sees the known items, the writes and the rescorer as they are when its turn
 *     comes.  Not for a member of a group (mals_group_most_popular_items).
 *  8. The per-item counts stay on the device after a call and are recomputed only when something they depend on changed
 *     since: mals_set_known_items, mals_set_matrix / mals_begin_matrix of side X, mals_set_factor_rows / mals_bind_factors
 *     of side X, any mals_set_preferences / mals_remove_preferences / mals_grow_factor_rows batch, mals_set_tag_users, or
 *     another item count.  Rescorer changes and mals_set_tag_items act after the count and never force a recount.
 *     mals_most_popular_stats: out4 = {calls, recounts, user rows whose set the last recount took from the writes' overlay
 *     (not their base row), (user, item) pairs counted in the last recount}; read without a ticket. */
int mals_set_tag_users(mals_handle h, int64_t n, const int64_t* user_idx, int mem_kind);
int mals_get_tag_user_count(mals_handle h, int64_t* n_out);   /* distinct user rows of this handle currently not counted */
int mals_most_popular_items(mals_handle h, mals_rescorer r, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out);
int mals_most_popular_stats(mals_handle h, int64_t* out4);

/* ---- ingest -> CSR ------------------------------------------------------
 * What InputFilesReader.readInputFiles (online-local/src/net/myrrix/online/generation/
 * InputFilesReader.java:64-211) does to the parsed records of the input files, on the device: the
 * caller appends (user id, item id, value) records IN FILE ORDER -- value NaN = the line had an empty
 * value token = "remove this entry" (IFR:137,165-167) -- and mals_ingest_finish leaves in HBM exactly
 * the matrices the reference ends up with in RbyRow / RbyColumn:
 *   per (user,item) pair the records are replayed in order: NaN removes the entry (MU:102-125), a
 *   value starts it or is added to it with one fp32 add per record (MU:64-92, FastByIDFloatMap.java:
 *   129-138); a user / item exists iff it still owns an entry at the end of the stream (MU:117-125);
 *   then entries with |value| < zero_threshold (model.decay.zeroThreshold, IFR:58-59) are dropped,
 *   which may leave existing rows empty (IFR:200-211 removes entries, not rows).
 * Dense indices are assigned in ascending id order; CSR columns ascend within a row.  Side X = R by
 * user, side Y = R^T by item.  Records come from the caller (mals_ingest_append) or from the text of the
 * input files (mals_ingest_append_text / _read_file / _read_dir, below).  Up to 2^31 - 256 records go through one sort
 * pipeline; more (C5: 5e9 lines) are finished user-id range by user-id range (MALS_INGEST_OPT_PARTITION_RECORDS), bounded
 * by device memory: 24 bytes per record held + 8 per entry and matrix + the workspace of one range.  Dense indices are
 * 32-bit: at most 2^31 - 256 distinct users and items. */
typedef struct mals_ingest_s* mals_ingest;
int mals_ingest_create(int32_t device, float zero_threshold, mals_ingest* out);
int mals_ingest_destroy(mals_ingest g);
const char* mals_ingest_last_error(mals_ingest g);
int mals_ingest_append(mals_ingest g, int64_t n, const int64_t* user_ids, const int64_t* item_ids,
                       const float* values, int mem_kind);
int mals_ingest_finish(mals_ingest g);
int mals_ingest_counts(mals_ingest g, int64_t* n_records, int64_t* n_users, int64_t* n_items, int64_t* nnz);
/* dense index -> 64-bit id (n_users / n_items entries) */
int mals_ingest_get_ids(mals_ingest g, int side, int64_t* host_ids_out);
/* host copies of one CSR (any pointer may be NULL) / the device arrays themselves */
int mals_ingest_get_csr(mals_ingest g, int side, int64_t* host_row_ptr, int32_t* host_col_idx, float* host_val);
int mals_ingest_device_csr(mals_ingest g, int side, const int64_t** row_ptr, const int32_t** col_idx, const float** val);
/* mals_set_matrix(MALS_MEM_DEVICE) of both sides into a factorizer handle on the same device; the
 * handle borrows the arrays, so the ingest object must outlive their use. */
int mals_ingest_install(mals_ingest g, mals_handle h);

/* ---- ServerRecommender.ingest(Reader): input lines applied to the live model ---------------------------------------
 * (ServerRecommender.java:204-309.)  g holds the records appended since its creation or its last mals_ingest_apply --
 * through mals_ingest_append_text, mals_ingest_read_file or mals_ingest_append -- and is on h's device; h is a handle
 * outside a group with both id directories in place (above), and, if the stream removes anything, with known items.
 *  1. A record whose value is NaN (an empty third token) is a remove, any other a set.
 *  2. The ids of the sets go through mals_ids_resolve, users and items, in record order: new ids get rows and the
 *     replicas grow.  The ids of the removes are then looked up: a remove whose user or item has no row is dropped
 *     (:1033-1042) and never creates one; a remove that stands before the set that creates its user finds a user
 *     without known items, which mals_remove_preferences ignores as the reference does.
 *  3. The stream is cut into maximal runs of sets and of removes (a dropped remove cuts nothing), and the runs go, in
 *     order, through mals_set_preferences and mals_remove_preferences: every row's arithmetic is theirs.  The whole call
 *     is one ticket of the serving front.
 *  4. stats_out8 (nullable) = {records, sets, removes passed on, removes dropped for an unknown id, sets failed, new
 *     users, new items, write calls made}.  removed_user_ids_out (capacity removed_cap; *n_removed_out of them): the IDS
 *     of the users the removes emptied, in order.  removed_cap smaller than the number of remove records is
 *     MALS_INVALID_ARG before anything changes.  Returns the code of the first failed update in stream order; the other
 *     updates go on.
 *  5. Afterwards the applied records are released from g; its line, bad-line and header counters and a carried partial
 *     line stay, so append_text(end_of_file = 0) -> apply -> append_text -> apply streams a file of any length, and
 *     "header" still means line 1 of the stream.
 *  6. TAG LINES, with MALS_INGEST_OPT_LIVE_TAGS = 1 (:281-293): a line with a tag in the user column is a setItemTag, one
 *     with a tag in the item column a setUserTag (mals_set_item_tags / mals_set_user_tags), unless its value is empty: a
 *     tag remove is ignored altogether -- no row, no mark, no cut of a run.  Tag sets are sets of step 1: their ids are
 *     resolved with the others' in record order (the user column on side X, the item column on side Y), they ride in the
 *     same runs and stats_out8 counts them among sets, new users and new items.  A line that SETS the empty tag (a tag token
 *     of two chars: "", but also "a -- substring(1, length - 1) is empty) throws out of the reference's ingest; here the
 *     text fails when it is appended, like the lone quote.  mals_ingest_apply_tag_stats has the tag lines' own counts.
 * REFUSED WHOLE (MALS_INVALID_ARG, nothing changed, the records stay in g): an ingest whose text has failed (more than
 * 100 bad lines, a lone-quote token, with live tags a set of the empty tag); without MALS_INGEST_OPT_LIVE_TAGS an ingest
 * that has seen a tag in either column; a finished, sharded or spent ingest; g on
 * another device; a member of a group; a directory that does not cover its side.  THE ONE DIFFERENCE from the reference:
 * it would have applied the lines in front of the fatal one; the caller can feed those lines again in a new ingest.
 * The failure's text is mals_ingest_last_error(g). */
int mals_ingest_apply(mals_ingest g, mals_handle h, int64_t* stats_out8, int64_t* removed_user_ids_out, int64_t removed_cap,
                      int64_t* n_removed_out);
/* Where the last mals_ingest_apply on h that ran to its end spent its time, in ms: out4 = {the ids on the device -- gather,
 * resolve, lookup and the copy of the rows to the host, HIP events on the handle's stream (the host's waits between the
 * kernels are inside); classification, cut and batches on the host; the write drivers (their level kernels alone:
 * mals_foldin_stats); the whole ticket}.  The parse has its own times (mals_ingest_text_info). */
int mals_ingest_apply_times(mals_handle h, double* out4);
/* Of the last mals_ingest_apply on h: out4 = {setItemTag records, setUserTag records, tag removes ignored, rows newly marked
 * (new members of the userTagIDs and of the itemTagIDs)}. */
int mals_ingest_apply_tag_stats(mals_handle h, int64_t* out4);

/* The device the ingest lives on, and its userTagIDs as rows of R^T: device_idx_out = a device array owned by the ingest
 * (valid until the next finish / destroy) holding, per userTagID in ascending id order (mals_ingest_get_tag_ids), its dense
 * item index, or -1 for a tag that owns no row at the end of the stream; n_out = the number of userTagIDs.  What
 * mals_ingest_install passes to mals_set_tag_items. */
int mals_ingest_device(mals_ingest g, int32_t* device_out);
int mals_ingest_device_tag_items(mals_ingest g, const int64_t** device_idx_out, int64_t* n_out);
int mals_ingest_get_tag_items(mals_ingest g, int64_t* host_idx_out);   /* the same array, copied to the host */
/* last finish: HIP-event milliseconds of the pipeline, host milliseconds spent (re)allocating its
 * workspace (52 bytes per record, kept for later finishes; hipMalloc of tens of GB is slow), algorithmic
 * bytes read+written by all passes, radix passes run */
int mals_ingest_stats(mals_ingest g, double* finish_ms, double* workspace_ms, double* bytes_moved, int32_t* radix_passes);
/* last finish: user-id ranges and item ranges it was cut into (0, 0: one pipeline) */
int mals_ingest_partitions(mals_ingest g, int32_t* user_ranges, int32_t* item_ranges);

/* ---- the TEXT half of the same row: bytes of the input files -> records, on the device -----------------
 * Replaces the line loop of InputFilesReader.readInputFiles (IFR = online-local/src/net/myrrix/online/generation/
 * InputFilesReader.java:88-192) over FileLineIterable (common/src/net/myrrix/common/iterator/FileLineIterator.java):
 *   lines      java.io.BufferedReader.readLine: '\n', '\r' or "\r\n" ends a line; bytes after the last terminator
 *              of a file are its last line
 *   IFR:92-98  one line counter and one bad-line counter over all files; the line FOLLOWING the 101st bad line
 *              fails the whole read with "Too many bad lines; aborting" (MALS_IO_ERROR, like the IOException)
 *   IFR:101    empty lines and lines starting with '#' are skipped
 *   IFR:51,105 Splitter.on(',').trimResults(): only the first three tokens are looked at; guava whitespace
 *              (ASCII and non-ASCII) is trimmed from each
 *   IFR:114-130 user and item tokens: Long.parseLong, or -- token starting with '"' -- a tag:
 *              OneWayMigrator.toLongID(token.substring(1, token.length()-1)) = first 8 bytes of the MD5 of the
 *              UTF-8 bytes, big-endian; a token that is a lone '"' makes the reference throw an unchecked
 *              StringIndexOutOfBoundsException out of readInputFiles: MALS_INVALID_ARG here
 *   IFR:132-137 value token: absent -> 1.0f; empty -> NaN = "remove this entry"; else LangUtils.parseFloat
 *              (Float.parseFloat's grammar, correctly rounded; NaN / infinite / overflowing values rejected)
 *   IFR:139-157 fewer than two tokens, or two tags -> bad line; an unparseable token -> bad line, except on line 1
 *              of the whole input, which is taken for a header and ignored
 *   IFR:159-165 tag in the user column -> its id joins itemTagIDs; in the item column -> userTagIDs
 *   IFR:173-191 knownItemIDs (MALS_INGEST_OPT_KNOWN_ITEMS): per user the items whose last line was not a remove
 * The parsed records join those of mals_ingest_append in stream order and go through the same mals_ingest_finish.
 * Everything after the bytes reach HBM runs on the device (csrc/ingest_text_kernels.h, csrc/text_parse.h); the
 * host lists and inflates files (zlib) and keeps the two sequential counters.  Behaviour of the JDK / guava /
 * mahout pieces this restates is listed, with what is pinned and what is not, at the top of csrc/text_parse.h.
 *
 * mals_ingest_append_text: `bytes` continue the current file (any split, also inside a line or between '\r' and
 * '\n'); end_of_file != 0 closes the file: its unterminated last line, if any, is a line.  MALS_MEM_DEVICE: the
 * bytes are already in HBM. */
/* KNOWN_ITEMS: also build knownItemIDs (off by default); TEXT_BLOCK_BYTES: bytes handed to the device at a time
 * (default 256 MiB); RESERVE_RECORDS: allocate the record arrays for this many records now (they grow by copying
 * otherwise) */
/* PARTITION_RECORDS: most records ONE sort pipeline is given (52 bytes of workspace each); an ingest with more is finished
 * user-id range by user-id range (csrc/ingest_big_host.h: same result, bit for bit).  0 = the default: one pipeline up to
 * 2^31 - 256 records; beyond, ranges as large as 70 % of the device's free memory hold at 76 bytes per record (at least
 * 2^26) -- which is how C5's 5e9 lines fit one 288 GB device next to their 120 GB of records.  (Tests set a few hundred
 * to run the oracle suites through the partitioned path.) */
/* SHARE (set before the first append): which piece of a stream ingested by a group this ingest holds (0 = default = the
 * stream's start; mals_group_ingest_finish).  A share > 0 takes an unparseable first line as a header CANDIDATE: the group
 * finish counts it as the header when every earlier share is empty, as a bad line otherwise. */
enum { MALS_INGEST_OPT_KNOWN_ITEMS = 1, MALS_INGEST_OPT_TEXT_BLOCK_BYTES = 2, MALS_INGEST_OPT_RESERVE_RECORDS = 3, MALS_INGEST_OPT_PARTITION_RECORDS = 4,
       MALS_INGEST_OPT_SHARE = 5,
       /* ServerRecommender.ingest(Reader) splits a line at commas AND tabs (DELIMITER, ServerRecommender.java:95), where the
        * input-file reader splits at commas alone (COMMA, InputFilesReader.java:51) and trims a tab as white space.  Value 1:
        * every tab of the text appended from then on is read as a comma -- both are then delimiters, which is exactly the
        * former splitter (quotes protect nothing in either).  Set it before the first text of a stream that goes to
        * mals_ingest_apply; default 0, the input-file reader's lines. */
       MALS_INGEST_OPT_TAB_DELIMITER = 6,
       /* 1: the tag lines of the text are writes of mals_ingest_apply (setUserTag / setItemTag; see there): every record keeps
        * its kind, one byte.  Set before the first append; default 0 (mals_ingest_apply refuses a text with tag lines).
        * mals_ingest_finish reads the records as before either way. */
       MALS_INGEST_OPT_LIVE_TAGS = 7 };
enum { MALS_ITEM_TAG_IDS = 0, MALS_USER_TAG_IDS = 1 };
int mals_ingest_set_option(mals_ingest g, int32_t option, int64_t value);
int mals_ingest_append_text(mals_ingest g, const void* bytes, int64_t n_bytes, int mem_kind, int32_t end_of_file);
/* One input file, by name like FileLineIterator.getFileInputStream (FLI:92-102): "*.gz" is inflated (all members, like
 * GZIPInputStream); "*.zip" yields NO lines -- the reference wraps it in a ZipInputStream on which getNextEntry()
 * is never called, and such a stream reads as empty; anything else is read as it is. */
int mals_ingest_read_file(mals_ingest g, const char* path);
/* IFR:71-86: the files of input_dir matching .+\.csv(\.(zip|gz))? in ascending last-modified order (equal
 * timestamps: by name; the reference leaves that order to File.listFiles()).  A missing directory reads nothing. */
int mals_ingest_read_dir(mals_ingest g, const char* input_dir, int32_t* n_files_read);
/* Share `share` of n_shares (<= 256) of the stream mals_ingest_read_dir reads (same files, same order), cut into pieces of
 * about equal on-disk bytes: the shares concatenated in index order are that stream.  A cut moves forward to the next line
 * start of a plain file (byte 0, after '\n', after a '\r' no '\n' follows); a .gz / .zip file goes whole to the share in
 * which its first byte falls.  A share may be empty.  Sets MALS_INGEST_OPT_SHARE. */
int mals_ingest_read_dir_share(mals_ingest g, const char* input_dir, int32_t share, int32_t n_shares, int32_t* n_files_read);
typedef struct mals_ingest_text_info_t {
  int32_t struct_size; /* sizeof(mals_ingest_text_info_t) */
  int32_t reserved;
  int64_t lines;             /* IFR:99 `lines` */
  int64_t bad_lines;         /* IFR:93 `badLines` */
  int64_t header_lines;      /* 0 or 1 */
  int64_t skipped_lines;     /* empty or comment */
  int64_t full_parser_lines; /* lines the fast (ASCII, numeric) parser handed to the full one */
  int64_t text_bytes;
  int64_t records;           /* records held (text and mals_ingest_append) */
  double parse_ms;           /* HIP-event milliseconds of the text kernels so far */
  double stage_ms;           /* ... of bringing the blocks in front of them: host-to-device copies (PCIe) for
                                MALS_MEM_HOST bytes, a device-to-device copy for MALS_MEM_DEVICE */
  int64_t n_item_tag_ids;    /* after mals_ingest_finish; -1 before */
  int64_t n_user_tag_ids;
  int64_t n_known_items;     /* entries of knownItemIDs; -1 if not requested / not finished */
} mals_ingest_text_info_t;
int mals_ingest_text_info(mals_ingest g, mals_ingest_text_info_t* out);
/* after mals_ingest_finish: ascending ids of itemTagIDs / userTagIDs */
int mals_ingest_get_tag_ids(mals_ingest g, int32_t which, int64_t* host_ids_out);
/* after mals_ingest_finish with MALS_INGEST_OPT_KNOWN_ITEMS: knownItemIDs as a CSR over the dense user indices
 * (n_users + 1 offsets) holding dense item indices, ascending within a user.  Its users are exactly the rows of
 * side X and its items rows of side Y; it differs from R's pattern by the entries removeSmall pruned (IFR:194-211). */
int mals_ingest_get_known_items(mals_ingest g, int64_t* host_ptr, int32_t* host_item_idx);
int mals_ingest_device_known_items(mals_ingest g, const int64_t** ptr, const int32_t** item_idx, int64_t* n_known);

/* ---- model.bin.gz, the file through which the factors leave and re-enter
 * the unmodified Java server.  Replaces GenerationSerializer.writeGeneration / readGeneration
 * (online-local/src/net/myrrix/online/generation/GenerationSerializer.java:84-95; body :96-262) and
 * IOUtils.writeObjectToFile / readObjectFromFile (common/src/net/myrrix/common/io/IOUtils.java:259-283):
 * a gzip member holding a Java Object Serialization stream (protocol version 2) with ONE object of
 * class net.myrrix.online.generation.GenerationSerializer (serialVersionUID 1, GS:51) whose custom
 * writeObject data (GS:96-105) is, big-endian, in 1024-byte block-data records:
 *   knownItemIDs  int count | -1 for null, then per user: long id, int n, n x long      GS:129-165
 *   X, Y          int count, then per row: long id, int length, length x float          GS:167-201
 *   itemTagIDs, userTagIDs   int count, count x long                                    GS:203-222
 *   userClusters, itemClusters  int count, per cluster: int n, n x long members,
 *                               int length, length x float centroid                     GS:224-262
 * Host only (no GPU, no handle).  Rows are written in the order given (the reference's order is the
 * hash order of its maps, which its reader does not depend on).  A non-finite factor is rejected on
 * both sides like Preconditions.checkState(LangUtils.isFinite(f)) (GS:167-201): MALS_INVALID_ARG.
 * Rows of X and Y must share one length ("features"); a file with ragged rows is MALS_INVALID_ARG.
 * Parity note: no JVM exists in the build image, so interoperability is pinned to the published
 * stream grammar (Java Object Serialization Specification, section 6.4) and to an independent
 * restatement in oracle/model_oracle.py -- not to a file written by the reference itself. */
typedef struct mals_model_view {
  int32_t struct_size; /* sizeof(mals_model_view) */
  int32_t features;
  int64_t n_users;
  const int64_t* user_ids;
  const float* X; /* n_users x features, row-major */
  int64_t n_items;
  const int64_t* item_ids;
  const float* Y;
  int64_t n_known; /* users with a known-item set; -1 = knownItemIDs is null (GS:131-133,148-149) */
  const int64_t* known_user_ids;
  const int64_t* known_ptr; /* n_known + 1 offsets into known_item_ids */
  const int64_t* known_item_ids;
  int64_t n_item_tags;
  const int64_t* item_tag_ids;
  int64_t n_user_tags;
  const int64_t* user_tag_ids;
  /* clusters: members of cluster c = members[member_ptr[c] .. member_ptr[c+1]), its centroid =
   * centroids[centroid_ptr[c] .. centroid_ptr[c+1]) */
  int64_t n_user_clusters;
  const int64_t* user_cluster_member_ptr;
  const int64_t* user_cluster_members;
  const int64_t* user_cluster_centroid_ptr;
  const float* user_cluster_centroids;
  int64_t n_item_clusters;
  const int64_t* item_cluster_member_ptr;
  const int64_t* item_cluster_members;
  const int64_t* item_cluster_centroid_ptr;
  const float* item_cluster_centroids;
} mals_model_view;
typedef struct mals_model_s* mals_model;
/* path must end in ".gz" (IOUtils.java:276) */
int mals_model_write(const char* path, const mals_model_view* model);
int mals_model_read(const char* path, mals_model* out);
/* the arrays of a model that was read; the pointers stay valid until mals_model_destroy */
int mals_model_get(mals_model m, mals_model_view* out);
int mals_model_destroy(mals_model m);
/* message of the last failed mals_model_* call of this thread */
const char* mals_model_last_error(void);

/* ---- the multi-GPU half-iteration below the C-ABI ------------------------------
 * Rows within a half-iteration are independent given the full opposite factor matrix and its Gramian --
 * how the reference threads it (ALS:391-410, one writer per output row ALS:497-499).  A GROUP is `world`
 * ranks, one GPU each, every rank holding the CSR rows of its slice of users and of items plus FULL
 * replicas of X and Y.  Per half-iteration: partial Gramian of the rank's own slice + k x k fp64 all-reduce;
 * solve the slice in `exchange_chunks` row chunks; as soon as a chunk is solved its rows go to every other
 * replica (in place, on a second stream, while the next chunk is being solved).  Slices are contiguous row
 * ranges balanced by COST (entries + row_cost per row, mals_plan_shards), not by row count, so the
 * exchange is an all-gather with per-rank counts: one grouped ncclSend/ncclRecv per peer pair (RCCL; on a
 * fully connected xGMI node every pair has its own link).
 * Two ways to form a group, same calls afterwards:
 *   mals_group_create         ONE process drives all GPUs (the JVM deployment): ncclCommInitAll;
 *   mals_group_create_rank    one process per GPU (torchrun / MPI style): rank 0 calls mals_group_unique_id,
 *                             ships the 128 bytes to the others by its own means, every rank calls
 *                             create_rank; all later mals_group_* calls are collective (every rank, same
 *                             order, same arguments apart from host buffers).
 * backend: MALS_GROUP_RCCL (RCCL, dlopen'ed: librccl.so.1 must be loadable) or MALS_GROUP_PEER_COPY
 * (single-process groups only: hipMemcpyPeerAsync between the replicas -- the SDMA engines move the
 * slices, no CU is taken from the solve -- and the k x k sum through the host).
 * Errors: MALS_COMM_ERROR for a failed RCCL call; a per-row error (MALS_SINGULAR ...) found by any rank is
 * returned by every rank. */
typedef struct mals_group_s* mals_group;
enum { MALS_GROUP_RCCL = 0, MALS_GROUP_PEER_COPY = 1 };

/* Contiguous row slices of equal cost: row r costs (row_ptr[r+1]-row_ptr[r]) + row_cost (row_cost < 0: a
 * default for `features`: the factorization of a row in entry-gathers, ~ features^2 / 200).
 * bounds_out[world+1]: slice j = rows [bounds_out[j], bounds_out[j+1]).  Host only. */
int mals_plan_shards(const int64_t* row_ptr, int64_t n_rows, int32_t world, double row_cost, int32_t features,
                     int64_t* bounds_out);

int mals_group_create(const mals_config* cfg, const int32_t* devices, int32_t n_devices, int32_t backend, mals_group* out);
int mals_group_unique_id(void* id_out_128_bytes);
int mals_group_create_rank(const mals_config* cfg, int32_t world, int32_t rank, const void* id_128_bytes, mals_group* out);
int mals_group_destroy(mals_group g);
const char* mals_group_last_error(mals_group g);
int mals_group_world(mals_group g);
int mals_group_features(mals_group g);   /* cfg.features (0 for a null group): lets a binding size-check factor arrays */
/* the handle of local member i (0 .. n_local-1; n_local = world for mals_group_create, 1 for create_rank)
 * and its rank -- for per-GPU calls such as mals_get_stats, mals_recommend, mals_reconstruction_error */
int mals_group_local(mals_group g, int32_t i, mals_handle* handle_out, int32_t* rank_out);
/* Row chunks per slice (default 4).  Takes effect with the NEXT matrix upload of each side: a side that already
 * holds a matrix keeps the count its work lists were built for. */
int mals_group_set_exchange_chunks(mals_group g, int32_t n_chunks);
/* Consecutive chunks of a half-iteration are solved on two alternating compute streams (default on): a chunk's tail -- the
 * last waves of its persistent kernels -- then overlaps the next chunk's head instead of draining the GPU at every chunk
 * boundary; each chunk's completion event is handed to the exchange stream as before and the streams are joined at the end
 * of the half-iteration.  0 = one stream (A/B; the factors are bitwise the same either way). */
int mals_group_set_alternate_streams(mals_group g, int32_t on);
/* Which shared library is loaded as RCCL: by default librccl.so.1 (a copy the process already mapped first).  A
 * process that wants a particular build -- or the tests' stand-in transport, tests/cpp/libmock_rccl.so -- says so
 * HERE, once, before its first group or unique id (MALS_INVALID_ARG afterwards); NULL = the default.  Deliberately
 * not an environment variable: what runs as "RCCL" inside a server process is the process's own decision. */
int mals_group_use_transport(const char* library_path);
/* What the communicator itself reports for local member i (ncclCommCount / ncclCommUserRank / ncclCommCuDevice;
 * 0 / -1 when the group has no communicator: world 1 or the peer-copy backend), the HIP device ordinal of the member
 * and its PCI bus id ("0000:c1:00.0"; pci_bus_id may be NULL) -- so that a benchmark line can prove how many ranks
 * RCCL saw and on which devices. */
int mals_group_comm_info(mals_group g, int32_t local_member, int32_t* comm_size, int32_t* comm_rank, int32_t* hip_device,
                         char* pci_bus_id, int32_t pci_len);
int mals_group_set_refine_limit(mals_group g, double limit);        /* mals_set_refine_limit on every local member */

/* Replicas: n_rows_total rows per side on every rank (>= the matrix rows: stale Y rows, ALS:304-308). */
int mals_group_set_factor_rows(mals_group g, int side, int64_t n_rows_total);
/* host rows -> every local replica / rows of local member 0's replica -> host */
int mals_group_set_factors(mals_group g, int side, int64_t row_begin, int64_t n_rows, const float* host_rows);
int mals_group_get_factors(mals_group g, int side, int64_t row_begin, int64_t n_rows, float* host_out);
int mals_group_get_rows(mals_group g, int side, const int64_t* row_idx, int32_t n, float* host_out);

/* The FULL matrix of a side (CSR, n_rows rows, global row_ptr; host or device arrays of the calling
 * process): slices are planned from row_ptr (mals_plan_shards with row_cost < 0) and every local member
 * uploads its own.  Device arrays are borrowed (col_idx / val) like mals_set_matrix(MALS_MEM_DEVICE). */
int mals_group_set_matrix(mals_group g, int side, int64_t n_rows, int64_t nnz, const int64_t* row_ptr,
                          const int32_t* col_idx, const float* val, int mem_kind);
/* The same for callers that cannot hold one array per matrix (Java arrays are < 2^31 entries): the full
 * row_ptr first (n_rows+1 longs always fit), then the entries of consecutive rows in any number of
 * pieces (each piece = whole rows), then end. */
int mals_group_begin_matrix(mals_group g, int side, int64_t n_rows, const int64_t* row_ptr);
int mals_group_append_rows(mals_group g, int side, int64_t n_rows, const int32_t* col_idx, const float* val);
int mals_group_end_matrix(mals_group g, int side);
/* How many entries the next n_rows rows of the chunked upload in progress hold (from the row_ptr given to begin): what a
 * binding checks its arrays against BEFORE mals_group_append_rows reads them. */
int mals_group_pending_entries(mals_group g, int side, int64_t n_rows, int64_t* n_entries_out);
/* InputFilesReader.readInputFiles -> the GROUP, without the detour through the host: after mals_ingest_finish both CSRs
 * are cut at the group's cost-balanced bounds (mals_plan_shards on the ingest's row pointers) and every local member takes
 * its slice of R and of R^T device to device -- borrowed in place when the member sits on the ingest's device, copied with
 * hipMemcpyPeerAsync into arrays the group owns otherwise -- together with its slice of knownItemIDs (when the ingest built
 * them) and the userTagIDs item mask.  Factor rows of both sides are declared from the ingest's counts (n_users, n_items)
 * unless already declared at least that large.  In a one-process-per-GPU group every rank calls this with its OWN ingest of
 * the same input (collective like mals_group_set_matrix); mals_group_ingest_finish is the other way, in which every rank
 * ingests only its share of the input.  flags = 0: the ingest must outlive the group's use of the
 * borrowed slices; MALS_INSTALL_COPY: members on the ingest's device copy their slices too (8 bytes per entry and side more
 * on that device) and the ingest -- its records and its 52 bytes per record of workspace -- can be destroyed right away. */
enum { MALS_INSTALL_COPY = 1 };
int mals_ingest_install_group(mals_ingest g, mals_group grp, int32_t flags);
/* The sharded ingest, the path that never holds the whole input on one device: ingests[i] holds share `rank of local member
 * i` of the stream (MALS_INGEST_OPT_SHARE / mals_ingest_read_dir_share) on that member's device; n_local = the group's local
 * members.  Collective (RCCL: all-reduces and grouped send/recv only; or MALS_GROUP_PEER_COPY), every rank returns the same
 * status: the text counters are combined in share order (header, bad lines, the abort after the 101st bad line, the
 * lone-quote error), the records go to the rank that owns their user (user-id ranges from a sample of every share), every rank
 * finishes its users like mals_ingest_finish would, the item and id tables are merged, and R^T's rows go to the rank that owns
 * their item (mals_plan_shards on the global entry counts).  The X bounds of the group are the user ranges, the Y bounds the
 * item ranges.  Records and workspace are released before the factor replicas are declared; each ingest then holds its
 * member's slices of R, R^T (global column indices) and knownItemIDs, the userTagIDs mask and both full id tables, which the
 * members borrow (the ingests must outlive their use).  Afterwards mals_ingest_counts reports the global counts (n_records:
 * the records this rank finished), mals_ingest_get_ids / mals_ingest_text_info the global tables and counters, and
 * mals_ingest_get_csr / _device_csr / _get_known_items this member's slice (mals_ingest_slice).  flags: reserved, 0. */
int mals_group_ingest_finish(mals_group grp, mals_ingest* ingests, int32_t n_local, int32_t flags);
/* Which rows of `side` the ingest's CSR holds: [*row_begin, *row_begin + *n_rows) -- all of them after mals_ingest_finish,
 * the member's slice after mals_group_ingest_finish. */
int mals_ingest_slice(mals_ingest g, int side, int64_t* row_begin, int64_t* n_rows);
/* Device bytes the ingest holds: work (records, text buffers, workspace) and results (CSRs, tables, knownItemIDs); the work
 * bytes it still held when mals_group_ingest_finish declared the factor replicas (-1: not through a group finish); and the
 * time and memory traffic of the split kernels (count + scatter: 50 B per record moved) of the last group finish. */
int mals_ingest_memory(mals_ingest g, int64_t* work_bytes, int64_t* result_bytes, int64_t* work_bytes_at_replicas, double* split_ms,
                       double* split_bytes);
/* ServerRecommender.recommend for model users on a group (arguments as mals_recommend): every member holds complete replicas
 * of X and Y but only ITS users' rows of R / knownItemIDs, so a query is answered by the local member whose slice holds the
 * user's row (consider_known_items: by any local member).  Callable from any number of request threads like mals_recommend:
 * it only reads the group and enters the members' serving fronts.  MALS_INVALID_ARG for a user whose owner is a rank of
 * another process (a one-process-per-GPU deployment routes the request to that process). */
int mals_group_recommend(mals_group g, const int64_t* user_idx, int32_t n_queries, int32_t how_many, int32_t consider_known_items,
                         int64_t* item_idx_out, float* score_out, int32_t* n_out);
/* The similarity calls on a group (arguments as mals_most_similar_items / mals_similarity_to_item /
 * mals_recommended_because): the Y replicas are complete on every member, so any local member answers the first two;
 * recommendedBecause goes to the local member that owns the user's row (MALS_INVALID_ARG if a rank of another process owns
 * it), as mals_group_recommend does. */
int mals_group_most_similar_items(mals_group g, const int64_t* item_idx, const int64_t* item_ptr, int32_t n_queries, int32_t how_many,
                                  int64_t* item_idx_out, float* score_out, int32_t* n_out);
int mals_group_similarity_to_item(mals_group g, int64_t to_item, const int64_t* item_idx, int32_t n, float* out);
int mals_group_recommended_because(mals_group g, const int64_t* user_idx, const int64_t* item_idx, int32_t n_queries, int32_t how_many,
                                   int64_t* item_idx_out, float* score_out, int32_t* n_out);
/* slice bounds of a side after its matrix was set: bounds_out[world+1] */
int mals_group_bounds(mals_group g, int side, int64_t* bounds_out);

/* ---- the online write path on a group: the twins of mals_set_preferences ... ---------------------------------------
 * Semantics, arguments, status_out, return codes and failure texts are the single-handle calls' (above), rows are dense
 * global indices.  For groups whose ranks all live in this process (mals_group_create with either backend, or
 * mals_group_create_rank with world 1); on a rank of a multi-process group every call below is MALS_INVALID_ARG -- like
 * mals_group_recommend, it cannot reach another process's owner.
 * WRITES (set_foldin_solver, set_foldin_learn_rate, set_preferences, set_user_tags, set_item_tags, remove_preferences,
 * grow_factor_rows) are a
 * replicated state machine: every member holds complete replicas of X and Y, the update kernels are deterministic, so
 * every local member applies the same batch in the same order to its own replicas and nothing is exchanged.  Afterwards
 * every member's X and Y are bit for bit what ONE handle holding the whole model would hold after the same call.  A
 * write holds the serving fronts of all members at once (the single-handle call's exclusive ticket, on each), enqueues
 * every member's kernels and only then waits for each: the devices work side by side.  The group orders its writes with a
 * lock of its own -- two writes from two threads reach every member in the same order (updates that share a row do not
 * commute).  Reads take no group-wide lock; a read racing a write sees, per member, the model before it or after it.
 * KNOWN ITEMS stay with their owner: user u belongs to the member whose slice of X holds its row (mals_group_bounds),
 * users past the installed matrix (rows of mals_group_grow_factor_rows) to the last rank.  Only the owner records the
 * items a write adds, only the owner decides whether a removal applies and whether it empties the user; every member
 * zeroes the rows of the emptied users.  mals_group_recommend and mals_group_recommended_because route grown users to the
 * last rank's member.  A new generation drops these overlays on every member: mals_group_set_matrix of side X,
 * mals_ingest_install_group, mals_group_ingest_finish (and mals_group_set_factor_rows of side X forgets the grown users).
 * ITERATIONS afterwards: a half-iteration of a side solves the rows of that side's installed matrix; rows past it (grown
 * rows) keep the values the writes gave them, on every member alike, and count in the Gramian of the opposite side's
 * half-iteration like every other row of the replica.  The replicas stay bitwise equal either way.
 * mals_group_foldin_stats: out6 as mals_foldin_stats; the counters count each update of a group write once (not once per
 * member), the two device times are the maximum over the members.
 * READS (estimate_preferences, anonymous_features, recommend_to_anonymous, estimate_for_anonymous): any member answers
 * (replicas and solvers are complete everywhere); successive calls rotate over the local members, so W devices serve W
 * callers.  Every answer is bit-identical to the single handle's.  Rescorers and the candidate filter on groups stay out
 * of scope. */
int mals_group_set_foldin_solver(mals_group g, int side, mals_solver s);
int mals_group_set_foldin_learn_rate(mals_group g, double rate);
int mals_group_foldin_stats(mals_group g, int64_t* out6);
/* setUserTag / setItemTag on a group (mals_set_user_tags / mals_set_item_tags): writes like mals_group_set_preferences.  Every
 * member marks the tag's row of Y in its own mask; the member that owns a tag's row of X (grown rows: the last rank's) keeps it
 * among its tag users, as mals_group_set_tag_users splits them. */
int mals_group_set_user_tags(mals_group g, int64_t n, const int64_t* user_row, const int64_t* tag_item_row, const float* value, int32_t* status_out);
int mals_group_set_item_tags(mals_group g, int64_t n, const int64_t* tag_user_row, const int64_t* item_row, const float* value, int32_t* status_out);
int mals_group_set_preferences(mals_group g, int64_t n, const int64_t* user_row, const int64_t* item_row, const float* value,
                               int32_t* status_out);
int mals_group_remove_preferences(mals_group g, int64_t n, const int64_t* user_row, const int64_t* item_row, int64_t* removed_users_out,
                                  int64_t* n_removed_out);
int mals_group_grow_factor_rows(mals_group g, int side, int64_t n_rows_total);
int mals_group_estimate_preferences(mals_group g, int64_t n, const int64_t* user_row, const int64_t* item_row, float* out);
int mals_group_anonymous_features(mals_group g, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values,
                                  float* out, int32_t* status_out);
int mals_group_recommend_to_anonymous(mals_group g, int32_t n_queries, const int64_t* item_ptr, const int64_t* item_row, const float* values,
                                      int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out, int32_t* status_out);
int mals_group_estimate_for_anonymous(mals_group g, int32_t n_queries, const int64_t* to_item, const int64_t* item_ptr,
                                      const int64_t* item_row, const float* values, float* out, int32_t* status_out);
/* mostPopularItems on a group whose ranks all live in this process (else MALS_INVALID_ARG, like the twins above).  The
 * known items are sharded by owner, so no member can answer alone: every local member counts the users it owns, side by
 * side on its own device; the partial count arrays are added on one member (peer copies, whichever backend the group was
 * made with); saturation at 2^24, the tag items and the selection happen after the sum.  The answer is bit for bit what
 * ONE handle holding the whole model returns from mals_most_popular_items (arguments as there; no rescorer: rescorers on
 * groups stay out of scope).  It holds every member's serving front while it runs, like a group write, but takes no
 * group-wide lock.  Each member keeps its own counts and recounts only after a change (point 8 there).
 * mals_group_set_tag_users: n GLOBAL user rows (host); each member keeps those it owns; n = 0 clears.  The calls that
 * start a new generation on a group (mals_group_set_matrix / mals_group_begin_matrix of side X, mals_ingest_install_group,
 * mals_group_ingest_finish) drop the set on every member, as they drop the overlays -- and none of them hands the ingest's
 * itemTagIDs over: call mals_group_set_tag_users afterwards. */
int mals_group_set_tag_users(mals_group g, int64_t n, const int64_t* user_idx);
int mals_group_most_popular_items(mals_group g, int32_t how_many, int64_t* item_idx_out, float* score_out, int32_t* n_out);

/* ---- a digest of a factor replica, on the device -------------------------------------------------------------------
 * The proof that replicas agree without copying them to the host.  The digest of rows [row_begin, row_begin + n_rows) of a
 * replica with k = features columns is the sum modulo 2^64, over the elements of the range, of term(j, bits): j = the
 * element's global flat index row * k + f, bits = the 32 bits of the float, and in uint64 arithmetic
 *     z = j * 0x9E3779B97F4A7C15 + bits;   z ^= z >> 32;   z *= 0xD6E8FEB86659FD93;   z ^= z >> 32;   term = z.
 * A sum, so any reduction order gives the same number and the digests of adjacent ranges add up (mod 2^64) to the digest
 * of their union -- a caller checks only the bands it touched.  It sees a value in the wrong row (j enters the mix),
 * tells -0.0 from 0.0 and one NaN payload from another (the bits enter, not the value); a range of 0 rows has digest 0.
 * It is a checksum against divergence, not a cryptographic hash.
 *   mals_factor_digest: one streaming pass on the device (16-byte loads; csrc/factor_digest.h), a ticket of the serving
 *     front: it sees the model between two writes, never the middle of one.  Members of a group are allowed.
 *   mals_group_replica_digest: the same range on every local member, taken with all members' fronts held at once, i.e.
 *     between the same two group writes; out_per_local_member[i] for local member i; *all_equal_out (nullable) = 1 iff
 *     they are all the same number.  Single-process groups only, like the write path.
 *   mals_factor_digest_host: the same arithmetic on the host over rows[n_rows][features] (the rows of the range, not the
 *     whole replica), no device -- what another runtime compares its own copy with. */
int mals_factor_digest(mals_handle h, int side, int64_t row_begin, int64_t n_rows, uint64_t* out);
int mals_group_replica_digest(mals_group g, int side, int64_t row_begin, int64_t n_rows, uint64_t* out_per_local_member,
                              int32_t* all_equal_out);
int mals_factor_digest_host(const float* rows, int32_t features, int64_t row_begin, int64_t n_rows, uint64_t* out);

/* ---- loading a new generation into a live handle -------------------------------------------------------------------
 * GenerationLoader.loadModel (online-local/src/net/myrrix/online/generation/GenerationLoader.java:49-106), which
 * DelegateGenerationManager calls after every rebuild (DelegateGenerationManager.java:359): the new X, Y, knownItemIDs and
 * tag sets are merged into the generation being served BY ID, and what the new model no longer has survives only if it
 * was written since the last load.  On the device the model is dense rows, so the merge is an id join, a compaction and a
 * row gather (csrc/generation_kernels.h), run as ONE exclusive ticket of the serving front on the handle's stream: a
 * concurrent mals_recommend* sees the old generation or the new one, never a mixture.  For handles outside a group
 * (a member is MALS_INVALID_ARG, like the writes; a group loads through mals_group_load_generation below).
 *
 * RECENT ROWS (recentlyActiveUsers / recentlyActiveItems, DelegateGenerationManager.java:179-186): the handle records,
 * per side, the user row and the item row of every datum given to mals_set_preferences and mals_remove_preferences whose
 * batch passed its argument checks, as doAppend does -- a host bit per written row, set inside the write's ticket; no
 * other call sees it.  mals_mark_recent adds n rows of `side` (host; rows inside the replica) for writes made elsewhere
 * (tag writes, an append on the JVM side); mals_get_recent returns them ascending (rows_out: capacity = the replica's
 * rows, may be NULL to ask for *n_out alone).  A successful load clears both sides (:97-98).
 *
 * THE MERGE, per side, with cur_ids[r] = the id of live row r (n_cur = the replica's rows) and new_ids[j] = the id of row
 * j of the new model:
 *   - merged rows 0 .. n_new-1 are the new model's rows in its order; behind them come, in live order, the live rows whose
 *     id is not among new_ids and which are recent -- the KEPT rows, with their live values, fold-in updates included.
 *     Every other live row is pruned (removeNotUpdated, :137-152).  A live row whose id is among new_ids takes the new
 *     model's vector even if it was written recently (updateMap is a put, :117-126).
 *     MALS_GENERATION_KEEP_NOT_UPDATED (model.removeNotUpdatedData=false, :72): every live row not among new_ids is kept.
 *   - the new rows are a prefix of the merged rows, so the new model's known-item CSR and its dense item indices hold for
 *     the merged model unchanged.
 *   - known items: a user of the new model gets the new model's set, whole (a put).  A kept user keeps its effective live
 *     set -- base row plus the writes' additions, or the set left by removals -- with every item re-indexed to its merged
 *     row.  DEVIATION: an item of such a set that has no merged row (it was pruned) is dropped and counted in
 *     n_known_dropped; the reference keeps the bare id there, where only mostPopularItems could still see it.
 *   - tag sets (updateTagIDs :108-115, removeNotUpdated :88-95): final set = updated set + the live tags whose row is
 *     recent (with KEEP_NOT_UPDATED: + every live tag).  item_tag_ids (itemTagIDs) are user-side ids and become the set of
 *     mals_set_tag_users over merged user rows; user_tag_ids (userTagIDs) are item-side ids and become the mask of
 *     mals_set_tag_items over merged item rows.  Ids without a merged row are ignored and counted
 *     (n_tag_ids_without_row).
 *   - state derived from the model (Generation.recomputeState, :101-102): both Gramians and the padded / rotated copies of
 *     the replicas are invalidated, the counts of mals_most_popular_items are recounted on the next call, and the
 *     candidate filter is DROPPED -- its signatures were a snapshot of the live Y: call mals_lsh_build again.  With
 *     MALS_GENERATION_RECOMPUTE_SOLVERS the solvers of X^T X and Y^T Y are recomputed from the merged replicas and set as
 *     mals_recompute_solver + mals_set_foldin_solver do, still inside the ticket; solver_status = the first code that was
 *     not MALS_OK (MALS_ILL_CONDITIONED, MALS_SINGULAR: the load itself stands, the solvers of the old generation stay).
 *     Rescorers name item rows of the generation they were made for: the caller makes them again.
 *   - the handle's matrices (mals_set_matrix) named live rows and are released: a handle that serves loaded generations
 *     is not iterated; a builder handle does that beside it ("rebuild beside a serving handle").
 * The merged replicas are the library's own blocks with room to grow (mals_grow_factor_rows), whatever the live ones were;
 * the new known items are copied (the new model's arrays stay the caller's and may go once the call returns).
 *
 * ALL OR NOTHING: everything is built aside and swapped in last.  Any failure -- MALS_OOM, an id twice within cur_ids or
 * within new_ids (MALS_INVALID_ARG), features != the handle's, n_cur != the replica's rows, missing known items on a
 * handle that holds some, a group member -- leaves the handle answering exactly as before.
 *
 * THE JOIN is an open-addressing table of the new ids with linear probing: slots = the smallest power of two >= max(64,
 * 2 n_new), home slot = mals_generation_hash_host(id) & (slots - 1), with in uint64 arithmetic
 *     z = id * 0x9E3779B97F4A7C15;   z ^= z >> 32;   z *= 0xD6E8FEB86659FD93;   z ^= z >> 32;   hash = z.
 * Every 64-bit value is a legal id (Long.MIN_VALUE, -1 and 0 included): a slot is claimed through its value word.
 * mals_generation_join_host is the same join on the host, no device: recent_rows = n_recent live rows (any order, repeats
 * allowed), flags as above; map_out[n_cur] = live row -> merged row, -1 = pruned; counts_out[4] (nullable) = {n_merged,
 * n_updated, n_kept, n_pruned}.  MALS_INVALID_ARG for a duplicate id on either side or a recent row outside [0, n_cur). */
enum { MALS_GENERATION_KEEP_NOT_UPDATED = 1, MALS_GENERATION_RECOMPUTE_SOLVERS = 2 };
typedef struct mals_generation_load {
  int32_t struct_size;
  int32_t flags;                  /* MALS_GENERATION_* */
  int32_t features;               /* of new_rows: must be the handle's */
  int32_t cur_mem_kind;           /* of cur_ids */
  int32_t new_mem_kind;           /* of every array of the new model below (device: what a builder handle and an ingest hold) */
  int32_t reserved;
  const int64_t* cur_ids[2];      /* [side]: the id of every live row */
  int64_t n_cur[2];               /* = the replica's rows (0 for a side without a replica) */
  const int64_t* new_ids[2];
  int64_t n_new[2];
  const float* new_rows[2];       /* n_new x features, dense */
  const int64_t* new_known_ptr;   /* CSR over the new users: n_new[X] + 1 offsets; NULL only if the handle holds no known items */
  const int32_t* new_known_idx;   /* dense item rows of the new model */
  const int64_t* item_tag_ids;    /* updatedItemTagIDs: user-side ids */
  int64_t n_item_tag_ids;
  const int64_t* user_tag_ids;    /* updatedUserTagIDs: item-side ids */
  int64_t n_user_tag_ids;
} mals_generation_load;
typedef struct mals_generation_result {
  int32_t struct_size;
  int32_t solver_status;          /* MALS_GENERATION_RECOMPUTE_SOLVERS: MALS_OK or the first failure */
  int64_t n_merged[2], n_updated[2], n_kept[2], n_pruned[2];   /* [side]; n_updated: live rows whose id the new model has */
  int64_t n_known_dropped, n_tag_ids_without_row;
  double join_ms[2], scan_ms[2], gather_ms[2];   /* device times (HIP events): tables + probe; scan + map; head copy + tail gather */
  double sides_ms, known_ms, tags_ms, total_ms;  /* host wall time: both sides (waits included), known items, tag sets, the ticket */
} mals_generation_result;
int mals_load_generation(mals_handle h, const mals_generation_load* load, mals_generation_result* result_out);
/* Of the last successful load, valid until the next: the merged ids in row order (n_merged of them), and live row ->
 * merged row for the n_cur rows the handle had before it (-1 = pruned) -- what the caller re-keys its id map with. */
int mals_generation_get_ids(mals_handle h, int side, int64_t* ids_out);
int mals_generation_get_map(mals_handle h, int side, int64_t* map_out);
int mals_mark_recent(mals_handle h, int side, int64_t n, const int64_t* rows);
int mals_get_recent(mals_handle h, int side, int64_t* rows_out, int64_t* n_out);
uint64_t mals_generation_hash_host(int64_t id);
int mals_generation_join_host(const int64_t* cur_ids, int64_t n_cur, const int64_t* new_ids, int64_t n_new, const int64_t* recent_rows,
                              int64_t n_recent, int32_t flags, int64_t* map_out, int64_t* counts_out);

/* ---- loading a new generation into a group ---------------------------------------------------------------------------
 * mals_group_load_generation: mals_load_generation for a group all of whose ranks live in this process (mals_group_create,
 * or mals_group_create_rank with world 1; a rank of a multi-process group is MALS_INVALID_ARG, like the write twins).  The
 * structs are mals_load_generation's, unchanged.  What differs:
 *   - the new model is given WHOLE -- ids, rows, the known-item CSR over all new users, the two tag-id sets -- not sliced;
 *     MALS_MEM_DEVICE arrays live on the device of the group's first local member (the others read peer copies).
 *   - n_cur = the rows of the replicas, which every member holds whole.  Every member runs the join, the compaction and the
 *     row gather on its own replicas and its own stream (the replicated state machine of the write path); afterwards every
 *     member's X and Y, the merged ids and the maps are bit for bit what ONE handle holding the whole live model would hold
 *     after mals_load_generation with the same arguments and the same history of writes and mark_recent calls, and so are
 *     the result's counts and every answer of the group's readers.  n_known_dropped and n_tag_ids_without_row are counted
 *     once per group; the device times are the slowest member's.
 *   - RECENT ROWS: mals_group_set_preferences and mals_group_remove_preferences record the user row and the item row of
 *     every datum of a batch that passed its argument checks, once per group and in global rows; mals_group_mark_recent /
 *     mals_group_get_recent are the twins of mals_mark_recent / mals_get_recent.  A successful load clears both sides.
 *   - OWNERSHIP: known items stay with a user's owner, and the owners are planned anew.  bounds[X] over the n_merged users
 *     = mals_plan_shards (default row cost, the group's features) over the row pointer "new_known_ptr, then the running
 *     sum of the kept users' set sizes" (all zeros without known items: the plan cuts by rows alone); bounds[Y] = the same
 *     over n_merged items without entries.  mals_group_bounds returns them; users grown later go to the last rank as
 *     before.  A kept user whose set is its base row moves as a row of its owner's CSR, re-indexed on the device in
 *     base-row order (csrc/generation_group_kernels.h); one with additions, a replaced set or a grown row is installed on
 *     its new owner as a whole set.  itemTagIDs are split by the new owners as mals_group_set_tag_users does.
 *   - the members' matrices are released: a loaded group serves and is not iterated until mals_group_set_matrix starts a
 *     new generation.  With MALS_GENERATION_RECOMPUTE_SOLVERS the solvers are computed once and installed on every member.
 *   - ALL OR NOTHING ACROSS MEMBERS: the call holds every member's serving front and the group's write lock; every member
 *     builds aside, and only when all are ready do they swap and the bounds change.  Any failure leaves every member, the
 *     bounds and the recent rows as they were.  A read racing the load is answered from the old generation or the new one.
 * mals_group_generation_get_ids / _get_map: of the last successful load, as mals_generation_get_ids / _get_map.
 * mals_group_generation_plan_host: the ownership plan alone, no device.  kept_rows = the kept users' live rows (n_kept,
 * strictly ascending: their old owners follow from old_bounds, world + 1 bounds or NULL = all on the last rank);
 * kept_sizes = their set sizes; new_known_ptr = n_new + 1 offsets (host) or NULL.  bounds_out: world + 1.  moves_out
 * (nullable): world x world x 2, [old][new] = the run [begin, end) of the OLD member's own kept list that the new member
 * gets -- contiguous, and in new-member order, because kept users are a tail of the merged order in old-owner order. */
int mals_group_load_generation(mals_group g, const mals_generation_load* load, mals_generation_result* result_out);
int mals_group_generation_get_ids(mals_group g, int side, int64_t* ids_out);
int mals_group_generation_get_map(mals_group g, int side, int64_t* map_out);
int mals_group_mark_recent(mals_group g, int side, int64_t n, const int64_t* rows);
int mals_group_get_recent(mals_group g, int side, int64_t* rows_out, int64_t* n_out);
int mals_group_generation_plan_host(int32_t world, int32_t features, int64_t n_new, const int64_t* new_known_ptr, int64_t n_kept,
                                    const int64_t* kept_sizes, const int64_t* kept_rows, const int64_t* old_bounds, int64_t* bounds_out,
                                    int64_t* moves_out);

/* iterateXFromY / iterateYFromX (ALS:340-389) and call() (ALS:176-262) on the group; arguments as for
 * mals_half_iteration / mals_factorize. */
int mals_group_half_iteration(mals_group g, int side);
int mals_group_factorize(mals_group g, double convergence_threshold, int32_t max_iterations, int32_t random_y,
                         int32_t iterate, const int64_t* test_users, int32_t n_test_users, const int64_t* test_items,
                         int32_t n_test_items, int32_t* iterations_out, double* convergence_out);
/* details of the last MALS_SINGULAR as mals_singular_info reports them, from whichever local member hit it
 * (side = -1: none of the local members did) */
int mals_group_singular_info(mals_group g, int32_t* side, int64_t* row, int32_t* apparent_rank);
/* diagnostic: the exchange of a side on its own (the current slices into every replica again), to price the
 * wire separately from the solve it normally hides behind */
int mals_group_exchange_only(mals_group g, int side);
int mals_group_cancel(mals_group g);
/* wait for everything enqueued on the local members' streams (timing brackets) */
int mals_group_synchronize(mals_group g);

/* Accuracy on ill-conditioned rows.  The reference solves every row's k x k system in fp64 (ALS:494 ->
 * CMLSS:37-55); the kernels here accumulate and factor it in fp32, which costs about cond(W) 6e-8 of x -- inside the
 * 1e-4 bar up to cond(W) ~ 1e3, not beyond (confidence weights alpha|r| in the thousands against a small lambda).
 * Every solving kernel therefore estimates cond(W) from below -- max(largest entry of the row's own sum w y y^T,
 * a quarter of the largest entry of W) / (smallest pivot) -- and a row above `limit` is solved again
 * (als_refine_kernel): the same fp32 factor as preconditioner, conjugate gradients on the exact system with every
 * product in fp64 straight from the entries, the factor rows and the fp64 Gramian, until a step is below 1e-6 |x|.
 * Default 64 (environment MALS_REFINE_LIMIT overrides it at mals_create; a sixteenth of it applies under
 * MALS_FLAG_LOSS_IGNORES_UNSPECIFIED); 0 = never.  Independently of the limit, a row whose fp32 factorization
 * breaks down (pivot <= singularity_threshold) is re-done in fp64 with the reference's own roundings
 * (als_exact_kernel) before it is called singular.  mals_stats.rows_refined counts both. */
int mals_set_refine_limit(mals_handle h, double limit);

/* The operand scale of the split-precision gather as the last half-iteration computed it on the device (diagnostic):
 * out4 = {S, 1/S^2, range flag (1 = split-precision kernels ran, 0 = their fp32 twins), the bound on |y| that was
 * used}.  The bound is the exact max |element| of the gathered factor matrix whenever this library formed its Gramian
 * (mals_gramian, mals_half_iteration, mals_factorize, the group calls: the Gramian kernels record it, a group all-reduces
 * it), and sqrt(max_f G_ff) -- loose by up to sqrt(rows) -- after mals_set_gramian. */
int mals_get_gather_scale(mals_handle h, float* out4);

/* Host-side timeline of the current / last half-iteration on this handle (diagnostic), microseconds of one
 * process-wide steady clock: out4[0] = its first kernel was enqueued, out4[1] / out4[2] = begin / end of the host half
 * of the dual preparation (the k x k eigendecomposition, computed here or received from the group member that
 * computed it; 0 = none in this half-iteration), out4[3] reserved.  tests/test_gpu_group.py uses it to check that a
 * single-process group enqueues every member's kernels before any member's host work. */
int mals_get_timeline(mals_handle h, double* out4);

/* What call() logs per iteration in the reference -- "Finished iteration {}", "Avg absolute difference in estimate vs prior
 * iteration: {}" (ALS:241-246), "{} X/tag rows computed" (ALS:351-358) -- needs values out of the library WHILE
 * mals_factorize / mals_group_factorize run: the callback is called on the calling thread after every iteration's
 * convergence statistic, before the stop rules (ALS:242-256) are applied.  seconds = host wall time of the iteration;
 * rows / entries / algorithmic bytes of the iteration are what THIS process's members solved (a
 * one-process group: everything).  fn = NULL removes it. */
typedef struct mals_iteration_info {
  int32_t struct_size;
  int32_t iteration;             /* 1-based */
  double avg_abs_difference;     /* DoubleWeightedMean of |new - old| over the convergence sample (ALS:230-238) */
  double seconds;
  int64_t x_rows, y_rows;        /* rows solved by the two half-iterations */
  int64_t entries_gathered;
  double algorithmic_bytes;
  int32_t devices;               /* GPUs of this process taking part */
  int32_t reserved;
} mals_iteration_info;
typedef void (*mals_iteration_fn)(void* user, const mals_iteration_info* info);
int mals_set_iteration_callback(mals_handle h, mals_iteration_fn fn, void* user);
int mals_group_set_iteration_callback(mals_group g, mals_iteration_fn fn, void* user);

int mals_enable_timing(mals_handle h, int32_t on);
int mals_reset_stats(mals_handle h);
int mals_get_stats(mals_handle h, mals_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* MYRRIX_ALS_H */
