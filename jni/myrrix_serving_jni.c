/*
 * myrrix_serving_jni.c -- JNI shim for the rows of SURVEY.md section 8(f) either side of the factorization:
 *   * input files -> matrices (InputFilesReader.readInputFiles, online-local/src/net/myrrix/online/generation/
 *     InputFilesReader.java:64-211)          -> mals_ingest_* (read_dir / finish / counts / ids / CSR / tags / known items)
 *   * top-N scoring (ServerRecommender.recommend / recommendToMany / recommendToAnonymous,
 *     online/src/net/myrrix/online/ServerRecommender.java:366-508,561-606) -> mals_recommend, _to_many, _set_known_items,
 *     with the candidate filter of model.lsh.sampleRatio < 1 (LocationSensitiveHash.java) -> mals_lsh_build / _clear
 * bound by net.myrrix.online.generation.NativeGeneration (java/net/myrrix/online/generation/NativeGeneration.java).  The
 * reference has no FFI on these paths either; this is the binding a maintainer adds.
 *
 * NOT BUILT IN THIS REPOSITORY'S IMAGE (no JDK); compiled with -fsyntax-only -Wall -Wextra -Werror against
 * tools/jni_stub/jni.h by tests/test_jni_compiles.py.  Build where a JDK exists:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude \
 *       -o libmyrrix_serving_jni.so jni/myrrix_serving_jni.c -Lmyrrix-recommender_amd/csrc -lmyrrix_als
 *
 * Arrays are pinned or copied for the duration of one call only (no GetPrimitiveArrayCritical: serving threads must not
 * stall one another); results go back with Set<Type>ArrayRegion.  Status codes only, no exception crosses.
 */
#include <jni.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "myrrix_als.h"

#define JNI_FN(name) Java_net_myrrix_online_generation_NativeGeneration_##name

static mals_handle as_handle(jlong h) { return (mals_handle)(intptr_t)h; }
static mals_ingest as_ingest(jlong g) { return (mals_ingest)(intptr_t)g; }

/* ---- input files (InputFilesReader.java:64-211) ------------------------------------------------------------------ */

/* new ingest object on `device`; zeroThreshold = model.decay.zeroThreshold (IFR:194-211); wantKnownItems = !model.noKnownItems.
 * 0 on failure. */
JNIEXPORT jlong JNICALL JNI_FN(nativeIngestCreate)(JNIEnv* env, jclass cls, jint device, jfloat zero_threshold, jboolean want_known_items) {
  (void)env; (void)cls;
  mals_ingest g = NULL;
  if (mals_ingest_create((int32_t)device, (float)zero_threshold, &g) != MALS_OK) return 0;
  if (mals_ingest_set_option(g, MALS_INGEST_OPT_KNOWN_ITEMS, want_known_items ? 1 : 0) != MALS_OK) {
    (void)mals_ingest_destroy(g);
    return 0;
  }
  return (jlong)(intptr_t)g;
}

JNIEXPORT void JNICALL JNI_FN(nativeIngestDestroy)(JNIEnv* env, jclass cls, jlong g) {
  (void)env; (void)cls;
  if (g) (void)mals_ingest_destroy(as_ingest(g));
}

JNIEXPORT jstring JNICALL JNI_FN(nativeIngestLastError)(JNIEnv* env, jclass cls, jlong g) {
  (void)cls;
  const char* e = g ? mals_ingest_last_error(as_ingest(g)) : "no ingest object";
  return (*env)->NewStringUTF(env, e ? e : "");
}

/* readInputFiles(inputDir): every *.csv / *.csv.gz / *.csv.zip of the directory in last-modified order, then the finish.
 * `dir` arrives as modified-UTF-8 bytes + terminating 0 in a byte-sized int array-free form: the Java side passes
 * File.getAbsolutePath().getBytes(UTF_8) widened to longs (paths are short; this keeps the stub's surface at the array
 * accessors the other shims already use).  info (long[8]): lines, badLines, headerLines, skippedLines, records, users, items, nnz. */
JNIEXPORT jint JNICALL JNI_FN(nativeReadInputDir)(JNIEnv* env, jclass cls, jlong g, jlongArray dir_bytes, jlongArray info) {
  (void)cls;
  const jsize n = (*env)->GetArrayLength(env, dir_bytes);
  if (n <= 0 || n > 4096 || (*env)->GetArrayLength(env, info) < 8) return MALS_INVALID_ARG;
  char* path = (char*)malloc((size_t)n + 1);
  if (!path) return MALS_OOM;
  jlong* b = (*env)->GetLongArrayElements(env, dir_bytes, NULL);
  if (!b) {
    free(path);
    return MALS_OOM;
  }
  for (jsize i = 0; i < n; ++i) path[i] = (char)b[i];
  path[n] = 0;
  (*env)->ReleaseLongArrayElements(env, dir_bytes, b, JNI_ABORT);
  int32_t n_files = 0;
  int rc = mals_ingest_read_dir(as_ingest(g), path, &n_files);   /* "Too many bad lines" (IFR:96-98) comes back as a status + text */
  free(path);
  if (rc == MALS_OK) rc = mals_ingest_finish(as_ingest(g));
  if (rc != MALS_OK) return rc;
  mals_ingest_text_info_t ti;
  ti.struct_size = (int32_t)sizeof ti;
  rc = mals_ingest_text_info(as_ingest(g), &ti);
  if (rc != MALS_OK) return rc;
  int64_t n_records = 0, n_users = 0, n_items = 0, nnz = 0;
  rc = mals_ingest_counts(as_ingest(g), &n_records, &n_users, &n_items, &nnz);
  if (rc != MALS_OK) return rc;
  const jlong out[8] = {(jlong)ti.lines, (jlong)ti.bad_lines, (jlong)ti.header_lines, (jlong)ti.skipped_lines,
                        (jlong)n_records, (jlong)n_users, (jlong)n_items, (jlong)nnz};
  (*env)->SetLongArrayRegion(env, info, 0, 8, out);
  return MALS_OK;
}

/* dense index -> id of one side (side 0 = users / X, 1 = items / Y): ids must hold the side's count */
JNIEXPORT jint JNICALL JNI_FN(nativeIngestIds)(JNIEnv* env, jclass cls, jlong g, jint side, jlongArray ids) {
  (void)cls;
  /* the native side writes the side's count of ids: the array must hold them (a short one would corrupt the Java heap) */
  int64_t n_users = 0, n_items = 0;
  const int rc0 = mals_ingest_counts(as_ingest(g), NULL, &n_users, &n_items, NULL);
  if (rc0 != MALS_OK) return rc0;
  if (!ids || (side != 0 && side != 1) || (int64_t)(*env)->GetArrayLength(env, ids) < (side == 0 ? n_users : n_items)) return MALS_INVALID_ARG;
  jlong* p = (*env)->GetLongArrayElements(env, ids, NULL);
  if (!p) return MALS_OOM;
  const int rc = mals_ingest_get_ids(as_ingest(g), (int)side, (int64_t*)p);
  (*env)->ReleaseLongArrayElements(env, ids, p, rc == MALS_OK ? 0 : JNI_ABORT);
  return rc;
}

/* itemTagIDs (which = 0) / userTagIDs (1), IFR:152-165: pass an array of n_item_tag_ids / n_user_tag_ids longs */
JNIEXPORT jint JNICALL JNI_FN(nativeIngestTagIds)(JNIEnv* env, jclass cls, jlong g, jint which, jlongArray ids) {
  (void)cls;
  mals_ingest_text_info_t ti;
  ti.struct_size = (int32_t)sizeof ti;
  const int rc0 = mals_ingest_text_info(as_ingest(g), &ti);
  if (rc0 != MALS_OK) return rc0;
  const int64_t need = which == 0 ? ti.n_item_tag_ids : ti.n_user_tag_ids;
  if (!ids || (which != 0 && which != 1) || need < 0 || (int64_t)(*env)->GetArrayLength(env, ids) < need) return MALS_INVALID_ARG;
  jlong* p = (*env)->GetLongArrayElements(env, ids, NULL);
  if (!p) return MALS_OOM;
  const int rc = mals_ingest_get_tag_ids(as_ingest(g), (int32_t)which, (int64_t*)p);
  (*env)->ReleaseLongArrayElements(env, ids, p, rc == MALS_OK ? 0 : JNI_ABORT);
  return rc;
}

/* tag id counts and the size of knownItemIDs after the finish: out (long[3]) = itemTagIDs, userTagIDs, known entries (-1: none) */
JNIEXPORT jint JNICALL JNI_FN(nativeIngestSetSizes)(JNIEnv* env, jclass cls, jlong g, jlongArray out) {
  (void)cls;
  if ((*env)->GetArrayLength(env, out) < 3) return MALS_INVALID_ARG;
  mals_ingest_text_info_t ti;
  ti.struct_size = (int32_t)sizeof ti;
  const int rc = mals_ingest_text_info(as_ingest(g), &ti);
  if (rc != MALS_OK) return rc;
  const jlong v[3] = {(jlong)ti.n_item_tag_ids, (jlong)ti.n_user_tag_ids, (jlong)ti.n_known_items};
  (*env)->SetLongArrayRegion(env, out, 0, 3, v);
  return MALS_OK;
}

/* R by row (side 0) or by column (side 1) as CSR over the dense indices, for the maps the Java side still wants
 * (RbyRow / RbyColumn of the Generation): rowPtr has count + 1 longs, colIdx / val have nnz entries */
JNIEXPORT jint JNICALL JNI_FN(nativeIngestCsr)(JNIEnv* env, jclass cls, jlong g, jint side, jlongArray row_ptr, jintArray col_idx,
                                              jfloatArray val) {
  (void)cls;
  int64_t n_users = 0, n_items = 0, nnz = 0;
  const int rc0 = mals_ingest_counts(as_ingest(g), NULL, &n_users, &n_items, &nnz);
  if (rc0 != MALS_OK) return rc0;
  if (!row_ptr || !col_idx || !val || (side != 0 && side != 1) ||
      (int64_t)(*env)->GetArrayLength(env, row_ptr) < (side == 0 ? n_users : n_items) + 1 ||
      (int64_t)(*env)->GetArrayLength(env, col_idx) < nnz || (int64_t)(*env)->GetArrayLength(env, val) < nnz)
    return MALS_INVALID_ARG;
  jlong* rp = (*env)->GetLongArrayElements(env, row_ptr, NULL);
  jint* ci = (*env)->GetIntArrayElements(env, col_idx, NULL);
  jfloat* v = (*env)->GetFloatArrayElements(env, val, NULL);
  int rc = MALS_OOM;
  if (rp && ci && v) rc = mals_ingest_get_csr(as_ingest(g), (int)side, (int64_t*)rp, (int32_t*)ci, (float*)v);
  const jint mode = rc == MALS_OK ? 0 : JNI_ABORT;
  if (v) (*env)->ReleaseFloatArrayElements(env, val, v, mode);
  if (ci) (*env)->ReleaseIntArrayElements(env, col_idx, ci, mode);
  if (rp) (*env)->ReleaseLongArrayElements(env, row_ptr, rp, mode);
  return rc;
}

/* knownItemIDs as CSR over the dense user indices (IFR:172-191): ptr has users + 1 longs, itemIdx the known entries */
JNIEXPORT jint JNICALL JNI_FN(nativeIngestKnownItems)(JNIEnv* env, jclass cls, jlong g, jlongArray ptr, jintArray item_idx) {
  (void)cls;
  int64_t n_users = 0;
  mals_ingest_text_info_t ti;
  ti.struct_size = (int32_t)sizeof ti;
  int rc0 = mals_ingest_counts(as_ingest(g), NULL, &n_users, NULL, NULL);
  if (rc0 == MALS_OK) rc0 = mals_ingest_text_info(as_ingest(g), &ti);
  if (rc0 != MALS_OK) return rc0;
  if (!ptr || !item_idx || ti.n_known_items < 0 || (int64_t)(*env)->GetArrayLength(env, ptr) < n_users + 1 ||
      (int64_t)(*env)->GetArrayLength(env, item_idx) < ti.n_known_items)
    return MALS_INVALID_ARG;
  jlong* p = (*env)->GetLongArrayElements(env, ptr, NULL);
  jint* ii = (*env)->GetIntArrayElements(env, item_idx, NULL);
  int rc = MALS_OOM;
  if (p && ii) rc = mals_ingest_get_known_items(as_ingest(g), (int64_t*)p, (int32_t*)ii);
  const jint mode = rc == MALS_OK ? 0 : JNI_ABORT;
  if (ii) (*env)->ReleaseIntArrayElements(env, item_idx, ii, mode);
  if (p) (*env)->ReleaseLongArrayElements(env, ptr, p, mode);
  return rc;
}

/* both matrices (and knownItemIDs, if built) handed to a factorizer handle on the same device without leaving HBM:
 * the handle borrows the arrays, keep the ingest object alive while it uses them */
JNIEXPORT jint JNICALL JNI_FN(nativeIngestInstall)(JNIEnv* env, jclass cls, jlong g, jlong handle) {
  (void)env; (void)cls;
  return mals_ingest_install(as_ingest(g), as_handle(handle));
}

/* ... or to every member of a factorizer group, cut at its bounds, device to device (mals_ingest_install_group; flags:
 * MALS_INSTALL_COPY = the members own copies and the ingest may be closed) */
JNIEXPORT jint JNICALL JNI_FN(nativeIngestInstallGroup)(JNIEnv* env, jclass cls, jlong g, jlong group, jint flags) {
  (void)env; (void)cls;
  return mals_ingest_install_group(as_ingest(g), (mals_group)(intptr_t)group, (int32_t)flags);
}

/* ---- top-N (ServerRecommender.java:366-508, RecommendIterator.java:62-109, TopN.java:49-128) ------------------------- */

/* the single-GPU handle of member `member` of a factorizer group (HipAlternatingLeastSquares keeps the group): its factors and
 * R stay resident after call(), so the generation that was just built can be served from the same memory.  0 on failure. */
JNIEXPORT jlong JNICALL JNI_FN(nativeGroupHandle)(JNIEnv* env, jclass cls, jlong group, jint member) {
  (void)env; (void)cls;
  mals_handle h = NULL;
  int32_t rank = 0;
  if (!group || mals_group_local((mals_group)(intptr_t)group, (int32_t)member, &h, &rank) != MALS_OK) return 0;
  return (jlong)(intptr_t)h;
}

/* generation.getKnownItemIDs() for the handle's users (SR:394-425): CSR over its local user rows of dense item indices;
 * rowPtr null = back to the rows of R */
JNIEXPORT jint JNICALL JNI_FN(nativeSetKnownItems)(JNIEnv* env, jclass cls, jlong handle, jlongArray row_ptr, jintArray item_idx) {
  (void)cls;
  if (!row_ptr) return mals_set_known_items(as_handle(handle), 0, NULL, NULL, MALS_MEM_HOST);
  const jsize n = (*env)->GetArrayLength(env, row_ptr);
  if (n < 1 || !item_idx) return MALS_INVALID_ARG;
  jlong* rp = (*env)->GetLongArrayElements(env, row_ptr, NULL);
  jint* ii = (*env)->GetIntArrayElements(env, item_idx, NULL);
  int rc = MALS_OOM;
  /* the offsets index item_idx: they must stay inside it */
  if (rp && ii && (rp[0] != 0 || rp[n - 1] < 0 || rp[n - 1] > (jlong)(*env)->GetArrayLength(env, item_idx))) rc = MALS_INVALID_ARG;
  else if (rp && ii) rc = mals_set_known_items(as_handle(handle), (int64_t)n - 1, (const int64_t*)rp, (const int32_t*)ii, MALS_MEM_HOST);
  if (ii) (*env)->ReleaseIntArrayElements(env, item_idx, ii, JNI_ABORT);
  if (rp) (*env)->ReleaseLongArrayElements(env, row_ptr, rp, JNI_ABORT);
  return rc;
}

/* recommend(userID, howMany, considerKnownItems, null) for a batch of model users by dense index (SR:382-441): items /
 * scores hold users x howMany results, best first, -1 / -inf padded; counts (may be null) the results per user */
JNIEXPORT jint JNICALL JNI_FN(nativeRecommend)(JNIEnv* env, jclass cls, jlong handle, jlongArray user_idx, jint how_many,
                                              jboolean consider_known_items, jlongArray items, jfloatArray scores, jintArray counts) {
  (void)cls;
  const jsize nq = (*env)->GetArrayLength(env, user_idx);
  if (how_many < 1 || (int64_t)(*env)->GetArrayLength(env, items) < (int64_t)nq * how_many ||
      (int64_t)(*env)->GetArrayLength(env, scores) < (int64_t)nq * how_many || (counts && (*env)->GetArrayLength(env, counts) < nq))
    return MALS_INVALID_ARG;
  jlong* u = (*env)->GetLongArrayElements(env, user_idx, NULL);
  jlong* it = (*env)->GetLongArrayElements(env, items, NULL);
  jfloat* sc = (*env)->GetFloatArrayElements(env, scores, NULL);
  jint* cn = counts ? (*env)->GetIntArrayElements(env, counts, NULL) : NULL;
  int rc = MALS_OOM;
  if (u && it && sc && (cn || !counts))
    rc = mals_recommend(as_handle(handle), (const int64_t*)u, (int32_t)nq, (int32_t)how_many, consider_known_items ? 1 : 0, (int64_t*)it, (float*)sc,
                        (int32_t*)cn);
  const jint mode = rc == MALS_OK ? 0 : JNI_ABORT;
  if (cn) (*env)->ReleaseIntArrayElements(env, counts, cn, mode);
  if (sc) (*env)->ReleaseFloatArrayElements(env, scores, sc, mode);
  if (it) (*env)->ReleaseLongArrayElements(env, items, it, mode);
  if (u) (*env)->ReleaseLongArrayElements(env, user_idx, u, JNI_ABORT);
  return rc;
}

/* recommendToMany (SR:366-441) and recommendToAnonymous (SR:561-606): query q owns the rows vectorPtr[q] .. vectorPtr[q+1] of
 * `vectors` (features floats each; vectorPtr null = one each), its exclusion list is excludeIdx[excludePtr[q] ..
 * excludePtr[q+1]) (dense item indices; both null = none).  Score = the reference's mean of dots (RecommendIterator.java:93-104). */
JNIEXPORT jint JNICALL JNI_FN(nativeRecommendToMany)(JNIEnv* env, jclass cls, jlong handle, jfloatArray vectors, jlongArray vector_ptr, jint n_queries,
                                                    jint how_many, jlongArray exclude_ptr, jlongArray exclude_idx, jlongArray items,
                                                    jfloatArray scores, jintArray counts) {
  (void)cls;
  if (n_queries < 0 || how_many < 1 || (vector_ptr && (*env)->GetArrayLength(env, vector_ptr) < n_queries + 1) ||
      (!exclude_ptr) != (!exclude_idx) || (exclude_ptr && (*env)->GetArrayLength(env, exclude_ptr) < n_queries + 1) ||
      (int64_t)(*env)->GetArrayLength(env, items) < (int64_t)n_queries * how_many ||
      (int64_t)(*env)->GetArrayLength(env, scores) < (int64_t)n_queries * how_many || (counts && (*env)->GetArrayLength(env, counts) < n_queries))
    return MALS_INVALID_ARG;
  jfloat* v = (*env)->GetFloatArrayElements(env, vectors, NULL);
  jlong* vp = vector_ptr ? (*env)->GetLongArrayElements(env, vector_ptr, NULL) : NULL;
  jlong* ep = exclude_ptr ? (*env)->GetLongArrayElements(env, exclude_ptr, NULL) : NULL;
  jlong* ei = exclude_idx ? (*env)->GetLongArrayElements(env, exclude_idx, NULL) : NULL;
  jlong* it = (*env)->GetLongArrayElements(env, items, NULL);
  jfloat* sc = (*env)->GetFloatArrayElements(env, scores, NULL);
  jint* cn = counts ? (*env)->GetIntArrayElements(env, counts, NULL) : NULL;
  int rc = MALS_OOM;
  if (v && it && sc && (vp || !vector_ptr) && (ep || !exclude_ptr) && (ei || !exclude_idx) && (cn || !counts)) {
    /* what the offsets promise must be inside the arrays they index */
    mals_handle hh = as_handle(handle);
    const int64_t n_vec = vp ? (int64_t)vp[n_queries] : (int64_t)n_queries;
    const int64_t features = (int64_t)mals_features(hh);
    if (n_vec < 0 || features <= 0 || (int64_t)(*env)->GetArrayLength(env, vectors) < n_vec * features ||
        (ep && (ep[n_queries] < 0 || (int64_t)(*env)->GetArrayLength(env, exclude_idx) < (int64_t)ep[n_queries])))
      rc = MALS_INVALID_ARG;
    else
    rc = mals_recommend_to_many(as_handle(handle), (const float*)v, (const int64_t*)vp, (int32_t)n_queries, (int32_t)how_many, (const int64_t*)ep,
                                (const int64_t*)ei, (int64_t*)it, (float*)sc, (int32_t*)cn);
  }
  const jint mode = rc == MALS_OK ? 0 : JNI_ABORT;
  if (cn) (*env)->ReleaseIntArrayElements(env, counts, cn, mode);
  if (sc) (*env)->ReleaseFloatArrayElements(env, scores, sc, mode);
  if (it) (*env)->ReleaseLongArrayElements(env, items, it, mode);
  if (ei) (*env)->ReleaseLongArrayElements(env, exclude_idx, ei, JNI_ABORT);
  if (ep) (*env)->ReleaseLongArrayElements(env, exclude_ptr, ep, JNI_ABORT);
  if (vp) (*env)->ReleaseLongArrayElements(env, vector_ptr, vp, JNI_ABORT);
  if (v) (*env)->ReleaseFloatArrayElements(env, vectors, v, JNI_ABORT);
  return rc;
}

/* ---- rescorers (include/myrrix_als.h): NativeIDRescorer's device side.  fp64 weights travel as their raw bits
 * (Double.doubleToRawLongBits) in long arrays and are handed to the library as they are. ---- */
static mals_rescorer as_rescorer(jlong r) { return (mals_rescorer)(intptr_t)r; }

JNIEXPORT jlong JNICALL JNI_FN(nativeRescorerCreate)(JNIEnv* env, jclass cls, jlong handle) {
  (void)env;
  (void)cls;
  mals_rescorer r = NULL;
  if (mals_rescorer_create(as_handle(handle), &r) != MALS_OK) return 0;
  return (jlong)(intptr_t)r;
}

JNIEXPORT void JNICALL JNI_FN(nativeRescorerDestroy)(JNIEnv* env, jclass cls, jlong rescorer) {
  (void)env;
  (void)cls;
  if (rescorer) mals_rescorer_destroy(as_rescorer(rescorer));
}

JNIEXPORT jint JNICALL JNI_FN(nativeRescorerSetFilter)(JNIEnv* env, jclass cls, jlong rescorer, jlongArray item_idx) {
  (void)cls;
  if (!rescorer) return MALS_INVALID_ARG;
  const jsize n = item_idx ? (*env)->GetArrayLength(env, item_idx) : 0;
  if (n == 0) return mals_rescorer_set_filter(as_rescorer(rescorer), 0, NULL, MALS_MEM_HOST);
  jlong* ii = (*env)->GetLongArrayElements(env, item_idx, NULL);
  int rc = MALS_OOM;
  if (ii) rc = mals_rescorer_set_filter(as_rescorer(rescorer), (int64_t)n, (const int64_t*)ii, MALS_MEM_HOST);
  if (ii) (*env)->ReleaseLongArrayElements(env, item_idx, ii, JNI_ABORT);
  return rc;
}

/* scale_bits / offset_bits: n_rows fp64 bit patterns each (either may be null) */
JNIEXPORT jint JNICALL JNI_FN(nativeRescorerSetWeights)(JNIEnv* env, jclass cls, jlong rescorer, jlongArray scale_bits, jlongArray offset_bits,
                                                       jlong n_rows) {
  (void)cls;
  if (!rescorer || n_rows < 0 || (scale_bits && (*env)->GetArrayLength(env, scale_bits) < n_rows) ||
      (offset_bits && (*env)->GetArrayLength(env, offset_bits) < n_rows))
    return MALS_INVALID_ARG;
  jlong* sb = scale_bits ? (*env)->GetLongArrayElements(env, scale_bits, NULL) : NULL;
  jlong* ob = offset_bits ? (*env)->GetLongArrayElements(env, offset_bits, NULL) : NULL;
  double* sc = sb ? (double*)malloc(sizeof(double) * (size_t)(n_rows > 0 ? n_rows : 1)) : NULL;
  double* of = ob ? (double*)malloc(sizeof(double) * (size_t)(n_rows > 0 ? n_rows : 1)) : NULL;
  int rc = MALS_OOM;
  if ((sb || !scale_bits) && (ob || !offset_bits) && (sc || !sb) && (of || !ob)) {
    if (sc) memcpy(sc, sb, sizeof(double) * (size_t)n_rows);
    if (of) memcpy(of, ob, sizeof(double) * (size_t)n_rows);
    rc = mals_rescorer_set_weights(as_rescorer(rescorer), sc, of, (int64_t)n_rows, MALS_MEM_HOST);
  }
  free(of);
  free(sc);
  if (ob) (*env)->ReleaseLongArrayElements(env, offset_bits, ob, JNI_ABORT);
  if (sb) (*env)->ReleaseLongArrayElements(env, scale_bits, sb, JNI_ABORT);
  return rc;
}

JNIEXPORT jint JNICALL JNI_FN(nativeRescorerSetUniform)(JNIEnv* env, jclass cls, jlong rescorer, jlong scale_bits, jlong offset_bits) {
  (void)env;
  (void)cls;
  if (!rescorer) return MALS_INVALID_ARG;
  double s, o;
  memcpy(&s, &scale_bits, sizeof(double));
  memcpy(&o, &offset_bits, sizeof(double));
  return mals_rescorer_set_uniform(as_rescorer(rescorer), s, o);
}

/* nativeRecommend with a rescorer (0: none) */
JNIEXPORT jint JNICALL JNI_FN(nativeRecommendRescored)(JNIEnv* env, jclass cls, jlong handle, jlong rescorer, jlongArray user_idx, jint how_many,
                                                      jboolean consider_known_items, jlongArray items, jfloatArray scores, jintArray counts) {
  (void)cls;
  const jsize nq = (*env)->GetArrayLength(env, user_idx);
  if (how_many < 1 || (int64_t)(*env)->GetArrayLength(env, items) < (int64_t)nq * how_many ||
      (int64_t)(*env)->GetArrayLength(env, scores) < (int64_t)nq * how_many || (counts && (*env)->GetArrayLength(env, counts) < nq))
    return MALS_INVALID_ARG;
  jlong* u = (*env)->GetLongArrayElements(env, user_idx, NULL);
  jlong* it = (*env)->GetLongArrayElements(env, items, NULL);
  jfloat* sc = (*env)->GetFloatArrayElements(env, scores, NULL);
  jint* cn = counts ? (*env)->GetIntArrayElements(env, counts, NULL) : NULL;
  int rc = MALS_OOM;
  if (u && it && sc && (cn || !counts))
    rc = mals_recommend_rescored(as_handle(handle), as_rescorer(rescorer), (const int64_t*)u, (int32_t)nq, (int32_t)how_many, consider_known_items ? 1 : 0,
                                 (int64_t*)it, (float*)sc, (int32_t*)cn);
  const jint mode = rc == MALS_OK ? 0 : JNI_ABORT;
  if (cn) (*env)->ReleaseIntArrayElements(env, counts, cn, mode);
  if (sc) (*env)->ReleaseFloatArrayElements(env, scores, sc, mode);
  if (it) (*env)->ReleaseLongArrayElements(env, items, it, mode);
  if (u) (*env)->ReleaseLongArrayElements(env, user_idx, u, JNI_ABORT);
  return rc;
}

/* nativeRecommendToMany with a rescorer (0: none).  An exclusion offset array without its index array is refused before
 * any length is read from either. */
JNIEXPORT jint JNICALL JNI_FN(nativeRecommendToManyRescored)(JNIEnv* env, jclass cls, jlong handle, jlong rescorer, jfloatArray vectors,
                                                            jlongArray vector_ptr, jint n_queries, jint how_many, jlongArray exclude_ptr,
                                                            jlongArray exclude_idx, jlongArray items, jfloatArray scores, jintArray counts) {
  (void)cls;
  if ((!exclude_ptr) != (!exclude_idx)) return MALS_INVALID_ARG;
  if (n_queries < 0 || how_many < 1 || !vectors || (vector_ptr && (*env)->GetArrayLength(env, vector_ptr) < n_queries + 1) ||
      (exclude_ptr && (*env)->GetArrayLength(env, exclude_ptr) < n_queries + 1) ||
      (int64_t)(*env)->GetArrayLength(env, items) < (int64_t)n_queries * how_many ||
      (int64_t)(*env)->GetArrayLength(env, scores) < (int64_t)n_queries * how_many || (counts && (*env)->GetArrayLength(env, counts) < n_queries))
    return MALS_INVALID_ARG;
  jfloat* v = (*env)->GetFloatArrayElements(env, vectors, NULL);
  jlong* vp = vector_ptr ? (*env)->GetLongArrayElements(env, vector_ptr, NULL) : NULL;
  jlong* ep = exclude_ptr ? (*env)->GetLongArrayElements(env, exclude_ptr, NULL) : NULL;
  jlong* ei = exclude_idx ? (*env)->GetLongArrayElements(env, exclude_idx, NULL) : NULL;
  jlong* it = (*env)->GetLongArrayElements(env, items, NULL);
  jfloat* sc = (*env)->GetFloatArrayElements(env, scores, NULL);
  jint* cn = counts ? (*env)->GetIntArrayElements(env, counts, NULL) : NULL;
  int rc = MALS_OOM;
  if (v && it && sc && (vp || !vector_ptr) && (ep || !exclude_ptr) && (ei || !exclude_idx) && (cn || !counts)) {
    /* what the offsets promise must be inside the arrays they index */
    mals_handle hh = as_handle(handle);
    const int64_t n_vec = vp ? (int64_t)vp[n_queries] : (int64_t)n_queries;
    const int64_t features = (int64_t)mals_features(hh);
    if (n_vec < 0 || features <= 0 || (int64_t)(*env)->GetArrayLength(env, vectors) < n_vec * features ||
        (ep && (ep[0] < 0 || ep[n_queries] < ep[0] || (int64_t)(*env)->GetArrayLength(env, exclude_idx) < (int64_t)ep[n_queries])))
      rc = MALS_INVALID_ARG;
    else
      rc = mals_recommend_to_many_rescored(hh, as_rescorer(rescorer), (const float*)v, (const int64_t*)vp, (int32_t)n_queries, (int32_t)how_many,
                                           (const int64_t*)ep, (const int64_t*)ei, (int64_t*)it, (float*)sc, (int32_t*)cn);
  }
  const jint mode = rc == MALS_OK ? 0 : JNI_ABORT;
  if (cn) (*env)->ReleaseIntArrayElements(env, counts, cn, mode);
  if (sc) (*env)->ReleaseFloatArrayElements(env, scores, sc, mode);
  if (it) (*env)->ReleaseLongArrayElements(env, items, it, mode);
  if (ei) (*env)->ReleaseLongArrayElements(env, exclude_idx, ei, JNI_ABORT);
  if (ep) (*env)->ReleaseLongArrayElements(env, exclude_ptr, ep, JNI_ABORT);
  if (vp) (*env)->ReleaseLongArrayElements(env, vector_ptr, vp, JNI_ABORT);
  if (v) (*env)->ReleaseFloatArrayElements(env, vectors, v, JNI_ABORT);
  return rc;
}

/* ---- the candidate filter (include/myrrix_als.h, mals_lsh_*): LocationSensitiveHash.java on the device ---- */

/* maxBitsDiffering (LocationSensitiveHash.java:98-108) for model.lsh.sampleRatio (its raw fp64 bits) and model.lsh.numHashes
 * into out[0] */
JNIEXPORT jint JNICALL JNI_FN(nativeLshMaxBitsDiffering)(JNIEnv* env, jclass cls, jlong ratio_bits, jint num_hashes, jintArray out) {
  (void)cls;
  if (!out || (*env)->GetArrayLength(env, out) < 1) return MALS_INVALID_ARG;
  double ratio;
  memcpy(&ratio, &ratio_bits, sizeof(double));
  int32_t mb = 0;
  const int rc = mals_lsh_max_bits_differing(ratio, (int32_t)num_hashes, &mb);
  if (rc != MALS_OK) return rc;
  const jint v = (jint)mb;
  (*env)->SetIntArrayRegion(env, out, 0, 1, &v);
  return MALS_OK;
}

/* random_vectors: numHashes x features entries, 0 / 1, hash-major (LocationSensitiveHash.java:113-119); mean_bits: features
 * fp64 bit patterns, or null = the mean of Y's rows, computed on the device.  The lengths are checked before an element is
 * read. */
JNIEXPORT jint JNICALL JNI_FN(nativeLshBuild)(JNIEnv* env, jclass cls, jlong handle, jint num_hashes, jint max_bits_differing,
                                             jintArray random_vectors, jlongArray mean_bits) {
  (void)cls;
  if (!handle || !random_vectors || num_hashes < 1 || num_hashes > 64) return MALS_INVALID_ARG;
  const int64_t features = (int64_t)mals_features(as_handle(handle));
  if (features <= 0 || (int64_t)(*env)->GetArrayLength(env, random_vectors) < (int64_t)num_hashes * features ||
      (mean_bits && (int64_t)(*env)->GetArrayLength(env, mean_bits) < features))
    return MALS_INVALID_ARG;
  const size_t n = (size_t)num_hashes * (size_t)features;
  jint* rv = (*env)->GetIntArrayElements(env, random_vectors, NULL);
  jlong* mb = mean_bits ? (*env)->GetLongArrayElements(env, mean_bits, NULL) : NULL;
  uint8_t* bytes = (uint8_t*)malloc(n);
  double* mean = mean_bits ? (double*)malloc(sizeof(double) * (size_t)features) : NULL;
  int rc = MALS_OOM;
  if (rv && bytes && (mb || !mean_bits) && (mean || !mean_bits)) {
    for (size_t i = 0; i < n; ++i) bytes[i] = rv[i] ? 1 : 0;
    if (mean) memcpy(mean, mb, sizeof(double) * (size_t)features);
    rc = mals_lsh_build(as_handle(handle), (int32_t)num_hashes, (int32_t)max_bits_differing, bytes, mean);
  }
  free(mean);
  free(bytes);
  if (mb) (*env)->ReleaseLongArrayElements(env, mean_bits, mb, JNI_ABORT);
  if (rv) (*env)->ReleaseIntArrayElements(env, random_vectors, rv, JNI_ABORT);
  return rc;
}

JNIEXPORT jint JNICALL JNI_FN(nativeLshClear)(JNIEnv* env, jclass cls, jlong handle) {
  (void)env;
  (void)cls;
  if (!handle) return MALS_INVALID_ARG;
  return mals_lsh_clear(as_handle(handle));
}

JNIEXPORT jstring JNICALL JNI_FN(nativeLastError)(JNIEnv* env, jclass cls, jlong handle) {
  (void)cls;
  const char* e = handle ? mals_last_error(as_handle(handle)) : "no handle";
  return (*env)->NewStringUTF(env, e ? e : "");
}

/* ---- a new generation into the serving handle (GenerationLoader.loadModel, GenerationLoader.java:49-106) -------------- */

/* mals_load_generation with every array of the new model on the host: cur*Ids = the id of every live row, new*Ids / newX /
 * newY (n x features, row-major) the rebuilt model, knownPtr / knownIdx its knownItemIDs as a CSR over the new users (both
 * null only for a handle without known items), itemTagIds / userTagIds the updated tag sets (may be empty).  flags: 1 =
 * model.removeNotUpdatedData=false, 2 = recompute the solvers.  counts (long[12]): per side merged, updated, kept, pruned
 * (users then items), known items dropped, tag ids without a row, the solvers' status, 0.  userMap / itemMap (one long per
 * live row): live row -> merged row, -1 = pruned.  The merged ids come from nativeGenerationIds. */
JNIEXPORT jint JNICALL JNI_FN(nativeLoadGeneration)(JNIEnv* env, jclass cls, jlong handle, jint flags, jint features, jlongArray cur_user_ids,
                                                    jlongArray cur_item_ids, jlongArray new_user_ids, jlongArray new_item_ids, jfloatArray new_x,
                                                    jfloatArray new_y, jlongArray known_ptr, jintArray known_idx, jlongArray item_tag_ids,
                                                    jlongArray user_tag_ids, jlongArray counts, jlongArray user_map, jlongArray item_map) {
  (void)cls;
  if (!cur_user_ids || !cur_item_ids || !new_user_ids || !new_item_ids || !new_x || !new_y || !item_tag_ids || !user_tag_ids || !counts ||
      !user_map || !item_map || features < 1 || (known_ptr == NULL) != (known_idx == NULL))
    return MALS_INVALID_ARG;
  const jsize n_cur[2] = {(*env)->GetArrayLength(env, cur_user_ids), (*env)->GetArrayLength(env, cur_item_ids)};
  const jsize n_new[2] = {(*env)->GetArrayLength(env, new_user_ids), (*env)->GetArrayLength(env, new_item_ids)};
  /* the native side reads n x features floats and n + 1 offsets, and writes one map entry per live row */
  if ((int64_t)(*env)->GetArrayLength(env, new_x) < (int64_t)n_new[0] * features || (int64_t)(*env)->GetArrayLength(env, new_y) < (int64_t)n_new[1] * features ||
      (known_ptr && (*env)->GetArrayLength(env, known_ptr) < n_new[0] + 1) || (*env)->GetArrayLength(env, counts) < 12 ||
      (*env)->GetArrayLength(env, user_map) < n_cur[0] || (*env)->GetArrayLength(env, item_map) < n_cur[1])
    return MALS_INVALID_ARG;
  jlong* cu = (*env)->GetLongArrayElements(env, cur_user_ids, NULL);
  jlong* ci = (*env)->GetLongArrayElements(env, cur_item_ids, NULL);
  jlong* nu = (*env)->GetLongArrayElements(env, new_user_ids, NULL);
  jlong* ni = (*env)->GetLongArrayElements(env, new_item_ids, NULL);
  jfloat* x = (*env)->GetFloatArrayElements(env, new_x, NULL);
  jfloat* y = (*env)->GetFloatArrayElements(env, new_y, NULL);
  jlong* kp = known_ptr ? (*env)->GetLongArrayElements(env, known_ptr, NULL) : NULL;
  jint* ki = known_idx ? (*env)->GetIntArrayElements(env, known_idx, NULL) : NULL;
  jlong* it = (*env)->GetLongArrayElements(env, item_tag_ids, NULL);
  jlong* ut = (*env)->GetLongArrayElements(env, user_tag_ids, NULL);
  int rc = MALS_OOM;
  mals_generation_result res;
  memset(&res, 0, sizeof res);
  res.struct_size = (int32_t)sizeof res;
  if (cu && ci && nu && ni && x && y && it && ut && (kp || !known_ptr) && (ki || !known_idx)) {
    if (kp && (kp[0] != 0 || kp[n_new[0]] < 0 || kp[n_new[0]] > (jlong)(*env)->GetArrayLength(env, known_idx))) {
      rc = MALS_INVALID_ARG;   /* the offsets index knownIdx: they must stay inside it */
    } else {
      mals_generation_load ld;
      memset(&ld, 0, sizeof ld);
      ld.struct_size = (int32_t)sizeof ld;
      ld.flags = (int32_t)flags;
      ld.features = (int32_t)features;
      ld.cur_mem_kind = MALS_MEM_HOST;
      ld.new_mem_kind = MALS_MEM_HOST;
      ld.cur_ids[0] = (const int64_t*)cu;
      ld.cur_ids[1] = (const int64_t*)ci;
      ld.new_ids[0] = (const int64_t*)nu;
      ld.new_ids[1] = (const int64_t*)ni;
      ld.new_rows[0] = (const float*)x;
      ld.new_rows[1] = (const float*)y;
      for (int s = 0; s < 2; ++s) {
        ld.n_cur[s] = (int64_t)n_cur[s];
        ld.n_new[s] = (int64_t)n_new[s];
      }
      ld.new_known_ptr = (const int64_t*)kp;
      ld.new_known_idx = (const int32_t*)ki;
      ld.item_tag_ids = (const int64_t*)it;
      ld.n_item_tag_ids = (int64_t)(*env)->GetArrayLength(env, item_tag_ids);
      ld.user_tag_ids = (const int64_t*)ut;
      ld.n_user_tag_ids = (int64_t)(*env)->GetArrayLength(env, user_tag_ids);
      rc = mals_load_generation(as_handle(handle), &ld, &res);
    }
  }
  if (ut) (*env)->ReleaseLongArrayElements(env, user_tag_ids, ut, JNI_ABORT);
  if (it) (*env)->ReleaseLongArrayElements(env, item_tag_ids, it, JNI_ABORT);
  if (ki) (*env)->ReleaseIntArrayElements(env, known_idx, ki, JNI_ABORT);
  if (kp) (*env)->ReleaseLongArrayElements(env, known_ptr, kp, JNI_ABORT);
  if (y) (*env)->ReleaseFloatArrayElements(env, new_y, y, JNI_ABORT);
  if (x) (*env)->ReleaseFloatArrayElements(env, new_x, x, JNI_ABORT);
  if (ni) (*env)->ReleaseLongArrayElements(env, new_item_ids, ni, JNI_ABORT);
  if (nu) (*env)->ReleaseLongArrayElements(env, new_user_ids, nu, JNI_ABORT);
  if (ci) (*env)->ReleaseLongArrayElements(env, cur_item_ids, ci, JNI_ABORT);
  if (cu) (*env)->ReleaseLongArrayElements(env, cur_user_ids, cu, JNI_ABORT);
  if (rc != MALS_OK) return rc;
  const jlong out[12] = {(jlong)res.n_merged[0], (jlong)res.n_updated[0], (jlong)res.n_kept[0], (jlong)res.n_pruned[0],
                         (jlong)res.n_merged[1], (jlong)res.n_updated[1], (jlong)res.n_kept[1], (jlong)res.n_pruned[1],
                         (jlong)res.n_known_dropped, (jlong)res.n_tag_ids_without_row, (jlong)res.solver_status, 0};
  (*env)->SetLongArrayRegion(env, counts, 0, 12, out);
  jlongArray maps[2] = {user_map, item_map};
  for (int s = 0; s < 2 && rc == MALS_OK; ++s) {
    if (n_cur[s] == 0) continue;
    jlong* m = (*env)->GetLongArrayElements(env, maps[s], NULL);
    if (!m) return MALS_OOM;
    rc = mals_generation_get_map(as_handle(handle), s, (int64_t*)m);
    (*env)->ReleaseLongArrayElements(env, maps[s], m, rc == MALS_OK ? 0 : JNI_ABORT);
  }
  return rc;
}

/* the merged ids of the last load in row order: ids must hold the side's merged rows (counts[0] / counts[4] above) */
JNIEXPORT jint JNICALL JNI_FN(nativeGenerationIds)(JNIEnv* env, jclass cls, jlong handle, jint side, jlong n_merged, jlongArray ids) {
  (void)cls;
  int64_t n_rows = 0;
  void* rows = NULL;
  if (!ids || (side != 0 && side != 1)) return MALS_INVALID_ARG;
  /* the native side writes one id per row of the replica: the array must hold them */
  const int rc0 = mals_factor_device_ptr(as_handle(handle), (int)side, &rows, &n_rows);
  if (rc0 != MALS_OK) return rc0;
  if (n_merged != (jlong)n_rows || (int64_t)(*env)->GetArrayLength(env, ids) < n_rows) return MALS_INVALID_ARG;
  jlong* p = (*env)->GetLongArrayElements(env, ids, NULL);
  if (!p) return MALS_OOM;
  const int rc = mals_generation_get_ids(as_handle(handle), (int)side, (int64_t*)p);
  (*env)->ReleaseLongArrayElements(env, ids, p, rc == MALS_OK ? 0 : JNI_ABORT);
  return rc;
}

/* recentlyActiveUsers / recentlyActiveItems for writes the library did not see (tag writes, an append on the JVM side) */
JNIEXPORT jint JNICALL JNI_FN(nativeMarkRecent)(JNIEnv* env, jclass cls, jlong handle, jint side, jlongArray rows) {
  (void)cls;
  if (!rows) return MALS_INVALID_ARG;
  const jsize n = (*env)->GetArrayLength(env, rows);
  if (n == 0) return MALS_OK;
  jlong* r = (*env)->GetLongArrayElements(env, rows, NULL);
  if (!r) return MALS_OOM;
  const int rc = mals_mark_recent(as_handle(handle), (int)side, (int64_t)n, (const int64_t*)r);
  (*env)->ReleaseLongArrayElements(env, rows, r, JNI_ABORT);
  return rc;
}
