/*
 * NativeGeneration -- the Java side of the two rows either side of the factorization that the MI355X-native library also
 * covers (SURVEY.md section 8(f) rows 2 and 4), via jni/myrrix_serving_jni.c:
 *
 *   readInputFiles(...)   same signature and effect as InputFilesReader.readInputFiles
 *                         (online-local/src/net/myrrix/online/generation/InputFilesReader.java:64-211): the files of the input
 *                         directory are read, split, parsed and merged ON THE DEVICE (mals_ingest_read_dir + _finish) and the
 *                         reference's own structures are filled from the resulting CSR -- RbyRow, RbyColumn, itemTagIDs,
 *                         userTagIDs, knownItemIDs -- so DelegateGenerationManager keeps working unchanged; a caller that goes
 *                         on to the native factorizer can skip the maps and call install(handle) instead.
 *   recommend(...) /      ServerRecommender.recommend / recommendToMany / recommendToAnonymous
 *   recommendToMany(...)  (online/src/net/myrrix/online/ServerRecommender.java:366-508,561-606) for dense user / item indices: the
 *                         scores are the reference's (RecommendIterator.java:93-104) bit for bit; with a NativeIDRescorer as the
 *                         rescorer, and -- after buildCandidateFilter(handle, features) -- with the reference's candidate filter
 *                         (LocationSensitiveHash, chosen when model.lsh.sampleRatio < 1) deciding which items a query sees.
 *
 * NOT BUILT IN THIS REPOSITORY'S IMAGE (no JDK); complete source against the reference's public classes, like
 * HipAlternatingLeastSquares.  Same package as InputFilesReader so that the call site at DelegateGenerationManager.java:336
 * switches by class name only.
 */
package net.myrrix.online.generation;

import java.io.File;
import java.io.IOException;
import java.nio.charset.Charset;

import net.myrrix.common.collection.FastByIDFloatMap;
import net.myrrix.common.collection.FastByIDMap;
import net.myrrix.common.collection.FastIDSet;
import net.myrrix.common.random.RandomManager;

import org.apache.commons.math3.random.RandomGenerator;

public final class NativeGeneration implements AutoCloseable {

  private static final float ZERO_THRESHOLD = Float.parseFloat(System.getProperty("model.decay.zeroThreshold", "0.0001"));   // IFR:58-59

  static {
    System.loadLibrary("myrrix_serving_jni");   // which loads libmyrrix_als.so
  }

  private long ingest;            // mals_ingest
  private long[] userIDs;         // dense index -> id, after readInputFiles
  private long[] itemIDs;

  private static native long nativeIngestCreate(int device, float zeroThreshold, boolean wantKnownItems);
  private static native void nativeIngestDestroy(long ingest);
  private static native String nativeIngestLastError(long ingest);
  private static native int nativeReadInputDir(long ingest, long[] dirBytes, long[] info);
  private static native int nativeIngestIds(long ingest, int side, long[] ids);
  private static native int nativeIngestTagIds(long ingest, int which, long[] ids);
  private static native int nativeIngestSetSizes(long ingest, long[] out);
  private static native int nativeIngestCsr(long ingest, int side, long[] rowPtr, int[] colIdx, float[] val);
  private static native int nativeIngestKnownItems(long ingest, long[] ptr, int[] itemIdx);
  private static native int nativeIngestInstall(long ingest, long handle);
  private static native int nativeIngestInstallGroup(long ingest, long group, int flags);
  private static native long nativeGroupHandle(long group, int member);
  private static native int nativeSetKnownItems(long handle, long[] rowPtr, int[] itemIdx);
  private static native int nativeRecommend(long handle, long[] userIdx, int howMany, boolean considerKnownItems,
                                            long[] items, float[] scores, int[] counts);
  private static native int nativeRecommendToMany(long handle, float[] vectors, long[] vectorPtr, int nQueries, int howMany,
                                                  long[] excludePtr, long[] excludeIdx, long[] items, float[] scores, int[] counts);
  private static native long nativeRescorerCreate(long handle);
  private static native void nativeRescorerDestroy(long rescorer);
  private static native int nativeRescorerSetFilter(long rescorer, long[] itemIdx);
  private static native int nativeRescorerSetWeights(long rescorer, long[] scaleBits, long[] offsetBits, long nRows);
  private static native int nativeRescorerSetUniform(long rescorer, long scaleBits, long offsetBits);
  private static native int nativeRecommendRescored(long handle, long rescorer, long[] userIdx, int howMany, boolean considerKnownItems,
                                                    long[] items, float[] scores, int[] counts);
  private static native int nativeRecommendToManyRescored(long handle, long rescorer, float[] vectors, long[] vectorPtr, int nQueries,
                                                          int howMany, long[] excludePtr, long[] excludeIdx, long[] items, float[] scores,
                                                          int[] counts);
  private static native int nativeLshMaxBitsDiffering(long ratioBits, int numHashes, int[] out);
  private static native int nativeLshBuild(long handle, int numHashes, int maxBitsDiffering, int[] randomVectors, long[] meanBits);
  private static native int nativeLshClear(long handle);
  private static native String nativeLastError(long handle);
  private static native int nativeLoadGeneration(long handle, int flags, int features, long[] curUserIds, long[] curItemIds,
                                                 long[] newUserIds, long[] newItemIds, float[] newX, float[] newY,
                                                 long[] knownPtr, int[] knownIdx, long[] itemTagIds, long[] userTagIds,
                                                 long[] counts, long[] userMap, long[] itemMap);
  private static native int nativeGenerationIds(long handle, int side, long nMerged, long[] ids);
  private static native int nativeMarkRecent(long handle, int side, long[] rows);

  /** The reference's own six arguments (InputFilesReader.java:64-69; call site DelegateGenerationManager.java:336): a switch by
   *  class name only.  The device is the first of -Dmodel.als.gpus (default 0). */
  public static NativeGeneration readInputFiles(FastByIDMap<FastIDSet> knownItemIDs,
                                                FastByIDMap<FastByIDFloatMap> rbyRow,
                                                FastByIDMap<FastByIDFloatMap> rbyColumn,
                                                FastIDSet itemTagIDs,
                                                FastIDSet userTagIDs,
                                                File inputDir) throws IOException {
    String gpus = System.getProperty("model.als.gpus", "0");
    int device = Integer.parseInt(gpus.split(",")[0].trim());
    return readInputFiles(knownItemIDs, rbyRow, rbyColumn, itemTagIDs, userTagIDs, inputDir, device);
  }

  /** InputFilesReader.readInputFiles (IFR:64-211) with the work on device `device`; the object keeps the matrices in HBM
   *  until close() so that install() can hand them to a factorizer without a round trip. */
  public static NativeGeneration readInputFiles(FastByIDMap<FastIDSet> knownItemIDs,
                                                FastByIDMap<FastByIDFloatMap> rbyRow,
                                                FastByIDMap<FastByIDFloatMap> rbyColumn,
                                                FastIDSet itemTagIDs,
                                                FastIDSet userTagIDs,
                                                File inputDir,
                                                int device) throws IOException {
    NativeGeneration g = new NativeGeneration();
    g.ingest = nativeIngestCreate(device, ZERO_THRESHOLD, knownItemIDs != null);
    if (g.ingest == 0) {
      throw new IOException("no native ingest on device " + device);
    }
    boolean ok = false;
    try {
      byte[] path = inputDir.getAbsolutePath().getBytes(Charset.forName("UTF-8"));
      long[] wide = new long[path.length];
      for (int i = 0; i < path.length; i++) {
        wide[i] = path[i];
      }
      long[] info = new long[8];   // lines, badLines, headerLines, skippedLines, records, users, items, nnz
      check(g.ingest, nativeReadInputDir(g.ingest, wide, info));   // "Too many bad lines" (IFR:96-98) arrives here
      // Java arrays end at 2^31 - 1 elements: an input with more users, items or entries than that cannot become the reference's
      // maps here (nor could the reference hold it) -- such inputs go to the factorizer with install() / installGroup() instead
      if (info[5] > Integer.MAX_VALUE || info[6] > Integer.MAX_VALUE || info[7] > Integer.MAX_VALUE) {
        throw new IOException("input too large for Java maps (" + info[5] + " users, " + info[6] + " items, " + info[7]
            + " entries): read it with NativeGeneration.readInputFiles(inputDir, device) and install() it");
      }
      int nUsers = (int) info[5];
      int nItems = (int) info[6];
      int nnz = (int) info[7];
      g.userIDs = new long[nUsers];
      g.itemIDs = new long[nItems];
      check(g.ingest, nativeIngestIds(g.ingest, 0, g.userIDs));
      check(g.ingest, nativeIngestIds(g.ingest, 1, g.itemIDs));
      fill(g, 0, nUsers, nnz, g.userIDs, g.itemIDs, rbyRow);
      fill(g, 1, nItems, nnz, g.itemIDs, g.userIDs, rbyColumn);
      long[] sizes = new long[3];
      check(g.ingest, nativeIngestSetSizes(g.ingest, sizes));
      if (sizes[0] > Integer.MAX_VALUE || sizes[1] > Integer.MAX_VALUE || sizes[2] > Integer.MAX_VALUE) {
        throw new IOException("input too large for Java sets (" + sizes[0] + " / " + sizes[1] + " tag ids, " + sizes[2] + " known items)");
      }
      addAll(g.ingest, 0, (int) sizes[0], itemTagIDs);
      addAll(g.ingest, 1, (int) sizes[1], userTagIDs);
      if (knownItemIDs != null && sizes[2] >= 0) {
        long[] ptr = new long[nUsers + 1];
        int[] idx = new int[(int) sizes[2]];
        check(g.ingest, nativeIngestKnownItems(g.ingest, ptr, idx));
        for (int u = 0; u < nUsers; u++) {
          FastIDSet known = new FastIDSet((int) (ptr[u + 1] - ptr[u]));
          for (long e = ptr[u]; e < ptr[u + 1]; e++) {
            known.add(g.itemIDs[idx[(int) e]]);
          }
          knownItemIDs.put(g.userIDs[u], known);
        }
      }
      ok = true;
      return g;
    } finally {
      if (!ok) {
        g.close();
      }
    }
  }

  private static void fill(NativeGeneration g, int side, int nRows, int nnz, long[] rowIDs, long[] colIDs,
                           FastByIDMap<FastByIDFloatMap> out) throws IOException {
    long[] rowPtr = new long[nRows + 1];
    int[] colIdx = new int[nnz];
    float[] val = new float[nnz];
    check(g.ingest, nativeIngestCsr(g.ingest, side, rowPtr, colIdx, val));
    for (int r = 0; r < nRows; r++) {
      FastByIDFloatMap row = new FastByIDFloatMap((int) (rowPtr[r + 1] - rowPtr[r]));
      for (long e = rowPtr[r]; e < rowPtr[r + 1]; e++) {
        row.put(colIDs[colIdx[(int) e]], val[(int) e]);
      }
      out.put(rowIDs[r], row);   // rows emptied by removeSmall stay, as in the reference (IFR:202-211 vs MU:117-125)
    }
  }

  private static void addAll(long ingest, int which, int n, FastIDSet into) throws IOException {
    if (n <= 0) {
      return;
    }
    long[] ids = new long[n];
    check(ingest, nativeIngestTagIds(ingest, which, ids));
    for (long id : ids) {
      into.add(id);
    }
  }

  private static void check(long ingest, int status) throws IOException {
    if (status != 0) {
      throw new IOException(nativeIngestLastError(ingest));   // e.g. "Too many bad lines; aborting" (IFR:96-98)
    }
  }

  /** Both matrices and knownItemIDs to a native factorizer handle on the same device, without leaving HBM
   *  (mals_ingest_install); the handle borrows them: keep this object open while it factorizes and serves. */
  public void install(long handle) throws IOException {
    check(ingest, nativeIngestInstall(ingest, handle));
  }

  /** The same for a multi-GPU factorizer (mals_ingest_install_group): both matrices cut at the group's cost-balanced bounds, every
   *  member its slices device to device, its users' knownItemIDs and the userTagIDs mask.  copy = true: the members own copies
   *  and this object may be closed right away; false: members on this object's device borrow, keep it open. */
  public void installGroup(long group, boolean copy) throws IOException {
    check(ingest, nativeIngestInstallGroup(ingest, group, copy ? 1 : 0));
  }

  public long[] getUserIDs() {
    return userIDs;
  }

  public long[] getItemIDs() {
    return itemIDs;
  }

  /** The single-GPU handle of a member of the factorizer's group (HipAlternatingLeastSquares): factors and R stay resident
   *  after call(), so the generation just built is served from the same memory. */
  public static long handleOf(long group, int member) {
    long handle = nativeGroupHandle(group, member);
    if (handle == 0) {
      throw new IllegalStateException("no member " + member + " in this group");
    }
    return handle;
  }

  /** generation.getKnownItemIDs() for a handle that was not fed by install(): CSR over its user rows, dense item indices. */
  public static void setKnownItems(long handle, long[] rowPtr, int[] itemIdx) {
    checkHandle(handle, nativeSetKnownItems(handle, rowPtr, itemIdx));
  }

  /** ServerRecommender.recommend(userID, howMany, considerKnownItems, null) (SR:382-441) for users by dense index:
   *  items[q * howMany + j] = dense index of the j-th best item of query q (-1 beyond counts[q]), scores likewise. */
  public static void recommend(long handle, long[] userIdx, int howMany, boolean considerKnownItems,
                               long[] items, float[] scores, int[] counts) {
    checkHandle(handle, nativeRecommend(handle, userIdx, howMany, considerKnownItems, items, scores, counts));
  }

  /** recommendToMany (SR:366-441; the caller passes the intersection of the users' known items as the exclusion list,
   *  SR:398-425) and recommendToAnonymous (SR:561-606; the query vector comes from the Solver of the generation). */
  public static void recommendToMany(long handle, float[] vectors, long[] vectorPtr, int nQueries, int howMany,
                                     long[] excludePtr, long[] excludeIdx, long[] items, float[] scores, int[] counts) {
    checkHandle(handle, nativeRecommendToMany(handle, vectors, vectorPtr, nQueries, howMany, excludePtr, excludeIdx, items, scores, counts));
  }

  /** recommend with a rescorer that the device runs (NativeIDRescorer; null = the plain call): the same answer as the Java
   *  path with the same object as its IDRescorer, bit for bit. */
  public static void recommend(long handle, long[] userIdx, int howMany, boolean considerKnownItems, NativeIDRescorer rescorer,
                               long[] items, float[] scores, int[] counts) {
    if (rescorer == null) {
      recommend(handle, userIdx, howMany, considerKnownItems, items, scores, counts);
      return;
    }
    checkHandle(handle, nativeRecommendRescored(handle, rescorer.nativeRescorer(handle), userIdx, howMany, considerKnownItems, items, scores,
                                                counts));
  }

  /** recommendToMany / recommendToAnonymous with a rescorer that the device runs (null = the plain call). */
  public static void recommendToMany(long handle, float[] vectors, long[] vectorPtr, int nQueries, int howMany, long[] excludePtr,
                                     long[] excludeIdx, NativeIDRescorer rescorer, long[] items, float[] scores, int[] counts) {
    if (rescorer == null) {
      recommendToMany(handle, vectors, vectorPtr, nQueries, howMany, excludePtr, excludeIdx, items, scores, counts);
      return;
    }
    checkHandle(handle, nativeRecommendToManyRescored(handle, rescorer.nativeRescorer(handle), vectors, vectorPtr, nQueries, howMany, excludePtr,
                                                      excludeIdx, items, scores, counts));
  }

  /** What Generation does when model.lsh.sampleRatio < 1 (CandidateFilterFactory.java:50-71 -> new LocationSensitiveHash(Y),
   *  LocationSensitiveHash.java:89-152), on the device: maxBitsDiffering from model.lsh.sampleRatio and model.lsh.numHashes
   *  (LSH:98-108), the random vectors drawn hash-major from RandomManager.getRandom().nextBoolean() as LSH:113-119 draws them,
   *  the mean of Y and one signature per row of Y computed on the device.  From then on recommend / recommendToMany on this
   *  handle only see a query's candidates (LSH:193-216).  Items that setPreference creates later are rows grown with
   *  mals_grow_factor_rows (the write path does that): they are always candidates, like the reference's newItems (LSH:219-225).
   *  With model.lsh.sampleRatio >= 1 (the default) no filter is built and an earlier one is cleared.  Returns true if one
   *  was built. */
  public static boolean buildCandidateFilter(long handle, int features) {
    double sampleRatio = Double.parseDouble(System.getProperty("model.lsh.sampleRatio", "1.0"));   // LSH:70
    int numHashes = Integer.parseInt(System.getProperty("model.lsh.numHashes", "20"));             // LSH:71
    if (!(sampleRatio > 0.0 && sampleRatio <= 1.0)) {
      throw new IllegalArgumentException("Bad LSH ratio: " + sampleRatio);                          // LSH:73-74
    }
    if (numHashes < 1 || numHashes > 64) {
      throw new IllegalArgumentException("Bad # hashes: " + numHashes);                             // LSH:75-76
    }
    if (sampleRatio >= 1.0) {
      checkHandle(handle, nativeLshClear(handle));
      return false;
    }
    if (features < 1) {
      throw new IllegalArgumentException("features must be positive");
    }
    int[] maxBits = new int[1];
    checkHandle(handle, nativeLshMaxBitsDiffering(Double.doubleToRawLongBits(sampleRatio), numHashes, maxBits));
    RandomGenerator random = RandomManager.getRandom();
    int[] randomVectors = new int[numHashes * features];
    for (int h = 0; h < numHashes; h++) {
      for (int j = 0; j < features; j++) {
        randomVectors[h * features + j] = random.nextBoolean() ? 1 : 0;
      }
    }
    checkHandle(handle, nativeLshBuild(handle, numHashes, maxBits[0], randomVectors, null));
    return true;
  }

  /** Back to every item a candidate. */
  public static void clearCandidateFilter(long handle) {
    checkHandle(handle, nativeLshClear(handle));
  }

  // NativeIDRescorer's way to its device object
  static long rescorerCreate(long handle) {
    return nativeRescorerCreate(handle);
  }

  static void rescorerDestroy(long rescorer) {
    nativeRescorerDestroy(rescorer);
  }

  static int rescorerSetFilter(long rescorer, long[] itemIdx) {
    return nativeRescorerSetFilter(rescorer, itemIdx);
  }

  static int rescorerSetWeights(long rescorer, long[] scaleBits, long[] offsetBits, long nRows) {
    return nativeRescorerSetWeights(rescorer, scaleBits, offsetBits, nRows);
  }

  static int rescorerSetUniform(long rescorer, long scaleBits, long offsetBits) {
    return nativeRescorerSetUniform(rescorer, scaleBits, offsetBits);
  }

  /** model.removeNotUpdatedData=false (GenerationLoader.java:72): every live row the new model lacks is kept. */
  public static final int KEEP_NOT_UPDATED = 1;
  /** Generation.recomputeState: the XTX / YTY solvers are recomputed from the merged model inside the load. */
  public static final int RECOMPUTE_SOLVERS = 2;

  /** What loadGeneration leaves: the merged ids in row order and, per live row, its merged row (-1 = pruned) -- what the
   *  caller re-keys its id maps with -- and the counts. */
  public static final class LoadedGeneration {
    public long[] userIDs;
    public long[] itemIDs;
    public long[] userMap;
    public long[] itemMap;
    /** per side merged, updated, kept, pruned (users, then items); known items dropped; tag ids without a row; solver status */
    public long[] counts;
  }

  /** GenerationLoader.loadModel (GenerationLoader.java:49-106) on the serving handle, by id: the rebuilt model's rows come
   *  first in its own order, then the live rows it lacks that were written since the last load (setPreference,
   *  removePreference, markRecent).  curUserIDs / curItemIDs: the id of every live row; newX / newY: n x features,
   *  row-major; knownPtr / knownIdx: the new knownItemIDs as a CSR over the new users with dense new item rows (null, null
   *  only for a handle without known items).  One exclusive step of the serving front: a concurrent recommend sees the old
   *  generation or the new one.  The candidate filter is dropped: call buildCandidateFilter again.  A kept user's known
   *  item that was pruned is dropped (counts[8]); the reference keeps the bare id. */
  public static LoadedGeneration loadGeneration(long handle, int flags, int features, long[] curUserIDs, long[] curItemIDs,
                                                long[] newUserIDs, long[] newItemIDs, float[] newX, float[] newY,
                                                long[] knownPtr, int[] knownIdx, long[] itemTagIDs, long[] userTagIDs) {
    LoadedGeneration g = new LoadedGeneration();
    g.counts = new long[12];
    g.userMap = new long[curUserIDs.length];
    g.itemMap = new long[curItemIDs.length];
    checkHandle(handle, nativeLoadGeneration(handle, flags, features, curUserIDs, curItemIDs, newUserIDs, newItemIDs, newX, newY,
                                             knownPtr, knownIdx, itemTagIDs == null ? new long[0] : itemTagIDs,
                                             userTagIDs == null ? new long[0] : userTagIDs, g.counts, g.userMap, g.itemMap));
    g.userIDs = new long[(int) g.counts[0]];
    g.itemIDs = new long[(int) g.counts[4]];
    checkHandle(handle, nativeGenerationIds(handle, 0, g.counts[0], g.userIDs));
    checkHandle(handle, nativeGenerationIds(handle, 1, g.counts[4], g.itemIDs));
    return g;
  }

  /** recentlyActiveUsers (side 0) / recentlyActiveItems (side 1) for writes made outside the library
   *  (DelegateGenerationManager.java:179-186): dense rows of the serving handle. */
  public static void markRecent(long handle, int side, long[] rows) {
    checkHandle(handle, nativeMarkRecent(handle, side, rows));
  }

  static String lastError(long handle) {
    return nativeLastError(handle);
  }

  private static void checkHandle(long handle, int status) {
    if (status != 0) {
      throw new IllegalStateException("native top-N failed with status " + status + ": " + nativeLastError(handle));
    }
  }

  @Override
  public void close() {
    if (ingest != 0) {
      nativeIngestDestroy(ingest);
      ingest = 0;
    }
  }
}
