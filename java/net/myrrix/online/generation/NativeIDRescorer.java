/*
 * NativeIDRescorer -- an IDRescorer of the one shape the device runs (include/myrrix_als.h, "rescorers"): a filter set and
 * an affine rescore,
 *     isFiltered(itemID) = itemID is in the filter set
 *     rescore(itemID, score) = scale(itemID) * score + offset(itemID)      (Java: two roundings, never fused)
 * with scale 1 and offset 0 for items the weights do not cover.  The same object answers on the Java path
 * (RecommendIterator.java:84-101 calls it) and, through NativeGeneration.recommend / recommendToMany, on the device, which
 * computes the same formula in the same fp64 operations: the two agree bit for bit.
 *
 * A RescorerProvider returns one from getRecommendRescorer / getRecommendToAnonymousRescorer (the reference's
 * FilterHalfRescorerProvider is new NativeIDRescorer(itemIDs, oddItemIndices, null, null, 10.0, 0.0)); the serving layer
 * hands it to NativeGeneration when the request has a native handle and keeps the Java path otherwise.  Weights must be
 * finite, scales > 0 (an item a rule scores NaN belongs in the filter set).
 *
 * Lifecycle (INTEGRATION.md, "Rescorers"): NOT a per-request object.  Construction builds an ID map over the catalogue and
 * the first native use uploads the weights through exclusive tickets of the handle's serving front, so a provider builds
 * one per generation and rule set, keeps it, and returns the same object to every request (thread-safe).  It is bound to
 * the first handle it is used with; for the next generation's handle build a new one, and close() the old one once no
 * request holds it and before its handle is destroyed -- close() frees the device buffers, nothing else does.
 */
package net.myrrix.online.generation;

import org.apache.mahout.cf.taste.recommender.IDRescorer;

import net.myrrix.common.collection.FastByIDMap;
import net.myrrix.common.collection.FastIDSet;

public final class NativeIDRescorer implements IDRescorer, AutoCloseable {

  private final FastByIDMap<Integer> indexOf;   // item ID -> dense item index (row of Y)
  private final FastIDSet filtered;             // item IDs
  private final long[] filteredIdx;             // dense indices
  private final double[] scale;                 // per dense index, may be null
  private final double[] offset;                // per dense index, may be null
  private final double uniformScale;
  private final double uniformOffset;
  private long handle;
  private long rescorer;

  /**
   * @param itemIDs       itemIDs[i] = the ID of dense item i (row i of Y)
   * @param filteredIdx   dense indices of the filtered items (may be null)
   * @param scale         per-item scale of rows [0, scale.length) (null: the uniform scale)
   * @param offset        per-item offset of rows [0, offset.length) (null: the uniform offset)
   * @param uniformScale  the scale of every item without a per-item weight (1 when per-item weights are given)
   * @param uniformOffset the offset of every item without a per-item weight (0 when per-item weights are given)
   */
  public NativeIDRescorer(long[] itemIDs, long[] filteredIdx, double[] scale, double[] offset, double uniformScale, double uniformOffset) {
    boolean perItem = scale != null || offset != null;
    if (perItem && (uniformScale != 1.0 || uniformOffset != 0.0)) {
      throw new IllegalArgumentException("per-item weights leave the other rows at scale 1, offset 0");
    }
    if (scale != null && offset != null && scale.length != offset.length) {
      throw new IllegalArgumentException("scale and offset cover different rows");
    }
    if (!(uniformScale > 0.0 && uniformScale < Double.POSITIVE_INFINITY) || Double.isNaN(uniformOffset) || Double.isInfinite(uniformOffset)) {
      throw new IllegalArgumentException("scale must be finite and > 0, offset finite");
    }
    indexOf = new FastByIDMap<Integer>(itemIDs.length);
    for (int i = 0; i < itemIDs.length; i++) {
      indexOf.put(itemIDs[i], i);
    }
    this.filteredIdx = filteredIdx == null ? new long[0] : filteredIdx.clone();
    filtered = new FastIDSet(this.filteredIdx.length);
    for (long i : this.filteredIdx) {
      filtered.add(itemIDs[(int) i]);
    }
    this.scale = scale == null ? null : scale.clone();
    this.offset = offset == null ? null : offset.clone();
    this.uniformScale = uniformScale;
    this.uniformOffset = uniformOffset;
  }

  @Override
  public boolean isFiltered(long itemID) {
    return filtered.contains(itemID);
  }

  @Override
  public double rescore(long itemID, double score) {
    Integer i = indexOf.get(itemID);
    int idx = i == null ? -1 : i;
    double s = scale != null && idx >= 0 && idx < scale.length ? scale[idx] : (scale == null && offset == null ? uniformScale : 1.0);
    double o = offset != null && idx >= 0 && idx < offset.length ? offset[idx] : (scale == null && offset == null ? uniformOffset : 0.0);
    double p = s * score;
    return p + o;
  }

  /** The device object on `handle`, made on first use (one handle per NativeIDRescorer). */
  synchronized long nativeRescorer(long handle) {
    if (rescorer != 0) {
      if (handle != this.handle) {
        throw new IllegalStateException("a NativeIDRescorer serves one handle");
      }
      return rescorer;
    }
    long r = NativeGeneration.rescorerCreate(handle);
    if (r == 0) {
      throw new IllegalStateException("native rescorer: " + NativeGeneration.lastError(handle));
    }
    int status = NativeGeneration.rescorerSetFilter(r, filteredIdx);
    if (status == 0) {
      if (scale != null || offset != null) {
        int n = scale != null ? scale.length : offset.length;
        status = NativeGeneration.rescorerSetWeights(r, bits(scale), bits(offset), n);
      } else {
        status = NativeGeneration.rescorerSetUniform(r, Double.doubleToRawLongBits(uniformScale), Double.doubleToRawLongBits(uniformOffset));
      }
    }
    if (status != 0) {
      String msg = NativeGeneration.lastError(handle);
      NativeGeneration.rescorerDestroy(r);
      throw new IllegalStateException("native rescorer failed with status " + status + ": " + msg);
    }
    this.handle = handle;
    rescorer = r;
    return r;
  }

  private static long[] bits(double[] v) {
    if (v == null) {
      return null;
    }
    long[] out = new long[v.length];
    for (int i = 0; i < v.length; i++) {
      out[i] = Double.doubleToRawLongBits(v[i]);
    }
    return out;
  }

  /** Releases the device object (no call that uses it may be in flight; before the handle is destroyed). */
  @Override
  public synchronized void close() {
    if (rescorer != 0) {
      NativeGeneration.rescorerDestroy(rescorer);
      rescorer = 0;
    }
  }
}
