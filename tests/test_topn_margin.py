"""The top-N filter's margin against its worst case (csrc/topn_kernels.h, header: "Error bound of the approximate score"),
on the CPU restatement of the kernels (tests/topn_filter_emulation.py, constants read from the header):
  (a) per item, both signs: rows whose bf16 roundings all point the same way, at every feature count the kernels
      instantiate differently and at power-of-two scales 2^+-40 -- |approx - exact| <= margin_i, the sample's lower bound
      is not above the exact score, and the filter's hit test passes the item at tau = its exact score (recommend, the
      mean of equal vectors of recommendToMany, and the cosine of mostSimilarItems);
  (b) whole catalogues built so that a margin under sqrt(2) * 2^-8 hides the true winners behind high-error items of
      the sample, and the randomized family of the GPU file: the filter's answer equals the oracles', and with the old
      margin (1.25 * 2^-8) most of the family's seeds answer wrongly;
  (c) the filter kernels convert their bf16 operands with v_cvt_pk_bf16_f32 (round to nearest, as the emulation
      assumes): at least one per pair of features, counted in the cross-compiled ISA."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import topn_oracle as to
from tests import similarity_oracle as so
from tests import topn_filter_emulation as fe

KS = [1, 2, 10, 16, 30, 31, 32, 33, 64, 100, 127, 128]
SCALES = [(0, 0), (40, 0), (-40, 0), (0, 40), (0, -40), (40, -40), (-40, -40), (40, 40)]


def coherent_cases(k, rng):
    """(name, x, rows): query vectors and item rows whose bf16 roundings all point the same way"""
    sign = np.where(rng.random(k) < 0.5, -1, 1).astype(np.float32)   # the same signs on both sides: every product > 0
    mant = fe.bf16(rng.uniform(1, 2, k).astype(np.float32))          # random bf16 grid values, then just off their midpoints
    half = (np.float32(2.0 ** -8) * np.exp2(np.floor(np.log2(mant)))).astype(np.float32)
    down = (mant + half - mant * np.float32(2.0 ** -20)).astype(np.float32)
    up = (mant + half + mant * np.float32(2.0 ** -20)).astype(np.float32)
    out = []
    for name, v in (("D", fe.D), ("U", fe.U)):                       # the full support, worst mantissa
        x = np.full(k, v, np.float32)
        out.append(("full-" + name, x * sign, np.stack([x, x * np.float32(2.0)]) * sign))
    out.append(("full-random-down", down * sign, down[None, :] * sign))
    out.append(("full-random-up", up * sign, up[None, :] * sign))
    if k >= 2:                                                       # D / U halves: the catalogues' B and T rows
        h = k // 2
        x = np.ones(k, np.float32)
        x[:h], x[h:2 * h] = fe.D, fe.U
        b = np.zeros(k, np.float32)
        b[h:2 * h] = fe.U
        t = np.zeros(k, np.float32)
        t[:h] = fe.D
        t[0] = fe.BUMP
        out.append(("halves", x * sign, np.stack([b, t]) * sign))
        ex = rng.random(k) < 0.3                                     # a set of bf16-exact components, the rest coherent
        x = np.where(ex, mant, down).astype(np.float32)
        out.append(("exact-mix", x * sign, np.stack([np.where(ex, mant, down), np.where(ex, 0, down)]).astype(np.float32) * sign))
    return out


def check_recommend(x_vectors, rows, tag):
    x, nrm, m0, floor = fe.prepare(x_vectors)
    approx = fe.approx_scores(rows, x)
    n0, ny = fe.item_norms(rows)
    xv = np.atleast_2d(x_vectors)
    exact = to.scores(rows, xv[0]) if len(xv) == 1 else to.scores_to_many(rows, xv)
    assert np.all(np.isfinite(exact)) and np.all(np.isfinite(approx)), tag
    err = np.abs(approx.astype(np.float64) - exact.astype(np.float64))
    m = fe.margin_i(ny, m0, floor)
    assert np.all(err <= m), (tag, err / m)
    lb = fe.lower_bound(approx, ny, n0, m0, floor)
    assert np.all(lb <= exact), (tag, lb, exact)
    for i in range(len(rows)):
        assert fe.hits(approx[i:i + 1], ny[i:i + 1], n0[i:i + 1], m0, floor, exact[i])[0], (tag, i)


def check_cosine(q, rows, tag):
    x, nrm, m0, floor = fe.prepare(q[None, :], cos=True)
    approx = fe.approx_scores(rows, x)
    n0, ny = fe.item_norms(rows)
    exact = so.cosine64(rows, q).astype(np.float32)
    assert np.all(np.isfinite(exact)), tag
    lb = fe.lower_bound(approx, ny, n0, m0, floor, cos=True)
    assert np.all(lb <= exact), (tag, lb, exact)
    # the premise of the header's term (e): tau, a bucket maximum of these lower bounds, satisfies |tau| <= 1 + 2^-5
    # (rows against -q: cosines near -1, the lower bounds below them)
    assert np.all(np.abs(lb) <= 1 + 2.0 ** -5), (tag, lb)
    for i in range(len(rows)):
        assert fe.hits(approx[i:i + 1], ny[i:i + 1], n0[i:i + 1], m0, floor, exact[i], cos=True)[0], (tag, i)


@pytest.mark.parametrize("k", KS)
def test_recommend_margin_bounds_coherent_rounding(k):
    rng = np.random.default_rng(1000 + k)
    for name, x, rows in coherent_cases(k, rng):
        for sx, sy in SCALES:
            xs = (x * np.float32(2.0 ** sx)).astype(np.float32)
            ys = (rows * np.float32(2.0 ** sy)).astype(np.float32)
            check_recommend(xs, ys, (k, name, sx, sy))
            # recommendToMany: the filter vector is the mean of the query's vectors, |x| the mean of their norms
            check_recommend(np.stack([xs, xs]), ys, (k, name, sx, sy, "x2"))
            check_recommend(np.stack([xs, xs, xs]), ys, (k, name, sx, sy, "x3"))


@pytest.mark.parametrize("k", KS)
def test_cosine_margin_bounds_coherent_rounding(k):
    rng = np.random.default_rng(2000 + k)
    if k >= 4:   # a unit query whose normalised components sit just off the midpoints (cosine_query), both directions
        xq, h, c = fe.cosine_query(k)
        qs = [("halves", xq)]
        for name, v in (("D", fe.D), ("U", fe.U)):
            q = xq.copy()
            q[:2 * h] = np.float32(c) * v
            qs.append(("full-" + name, q))
    else:
        qs = [("full-D", np.full(k, fe.D, np.float32))]
    for qname, q in qs:
        for name, _, rows in coherent_cases(k, rng):
            rows = np.abs(rows) * np.sign(q)[None, :]                # the query's signs
            rows = np.where(rows == 0, 0, rows).astype(np.float32)
            for sq, sy in ((0, 0), (40, 0), (-40, 0), (0, 40), (0, -40)):
                for sgn in (1, -1):
                    check_cosine((q * np.float32(sgn * 2.0 ** sq)).astype(np.float32), (rows * np.float32(2.0 ** sy)).astype(np.float32),
                                 (k, qname, name, sq, sy, sgn))


@pytest.mark.parametrize("k", [30, 64, 100, 128])
@pytest.mark.parametrize("how_many", [1, 10, 64])
def test_recommend_catalogue_through_the_filter_equals_the_oracle(k, how_many):
    Y, x, high, win = fe.recommend_catalogue(k, how_many)
    oidx, osc = to.recommend(Y, x, how_many)
    assert oidx[0] == win[-1] and set(oidx.tolist()) <= set(win.tolist())    # the catalogue is what it claims to be
    for vectors in (x, np.stack([x, x])):
        idx, sc, info = fe.topn(Y, vectors, how_many)
        assert not info["dense"], info
        assert np.array_equal(idx, oidx), (idx[:4], oidx[:4], info)
        assert np.array_equal(sc.view(np.uint32), osc.view(np.uint32))
    known = np.array([5, 77, 1234], np.int64)                        # an X row with known items (none of them planted)
    idx, sc, info = fe.topn(Y, x, how_many, known=known)
    oidx, osc = to.recommend(Y, x, how_many, known)
    assert np.array_equal(idx, oidx) and np.array_equal(sc.view(np.uint32), osc.view(np.uint32))


@pytest.mark.parametrize("k", [30, 64, 100, 128])
@pytest.mark.parametrize("how_many", [1, 10, 64])
def test_cosine_catalogue_through_the_filter_equals_the_oracle(k, how_many):
    Y, q, high, win = fe.cosine_catalogue(k, how_many)
    oidx, osc = so.most_similar(Y, [q], how_many)
    assert oidx[0] == win[-1] and set(oidx.tolist()) <= set(win.tolist())
    idx, sc, info = fe.topn(Y, Y[q], how_many, cos=True, exclude=[q])
    assert not info["dense"], info
    assert np.array_equal(idx, oidx), (idx[:4], oidx[:4], info)
    assert np.array_equal(sc.view(np.uint32), osc.view(np.uint32))


def family_disagreements(seeds):
    """per seed of fe.random_family: how many of its patterns the emulated filter answers differently from the oracle"""
    out = []
    for seed in seeds:
        Y, P, how_many, k = fe.random_family(seed)
        norms = fe.item_norms(Y)
        bad = 0
        for x in P:
            idx, sc, info = fe.topn(Y, x, how_many, norms=norms)
            assert not info["dense"], (seed, info)
            oidx, osc = to.recommend(Y, x, how_many)
            bad += not (np.array_equal(idx, oidx) and np.array_equal(sc.view(np.uint32), osc.view(np.uint32)))
        out.append(bad)
    return out


def test_randomized_family_agrees_with_the_oracle():
    """the family the GPU file runs on the device (tests/test_gpu_topn_adversarial.py), through the emulation"""
    assert family_disagreements(range(20)) == [0] * 20


def test_randomized_family_catches_the_old_margin(monkeypatch):
    """the family's power: with the margin of the first single-bf16 filter (1.25 * 2^-8), most seeds answer wrongly"""
    monkeypatch.setattr(fe, "TOPN_MARGIN", np.float32(1.25 * 2.0 ** -8))
    bad = family_disagreements(range(20))
    assert sum(b > 0 for b in bad) >= 15, bad


def test_emulation_follows_the_header():
    """the constants come from the header, and the plan is the one of the catalogues' 140 003 items"""
    assert 0 < fe.TOPN_MARGIN < fe.TOPN_COS_MARGIN < 2.0 ** -6 and 0 < fe.TOPN_MARGIN_FLOOR < 1e-20
    assert fe.plan(140_003, 1, 64) == (2, 2096, 8, 274)
    assert fe.plan(140_003, 64, 128) == (4, 5120, 4, 512)
    assert fe.bf16(np.float32(fe.D)) == 1.0 and fe.bf16(np.float32(fe.U)) == 1 + 2.0 ** -7
    assert fe.bf16_up(np.float32(1 + 2.0 ** -20)) == 1 + 2.0 ** -7 and fe.bf16_up(np.float32(-(1 + 2.0 ** -20))) == -1.0


# ---- (c) the rounding mode of the filter's bf16 operands on the device ------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INSTANCES = ["topn_stream_kernel<%d, %d, %d, 1, %s>" % (S, QT, mode, cos) for S, QT in ((1, 4), (2, 4), (3, 3), (4, 2))
             for mode in (0, 1) for cos in ("false", "true")] + ["topn_prepare_kernel<false>", "topn_prepare_kernel<true>"]


@pytest.fixture(scope="module")
def filter_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("topn_isa")
    src = d / "topn_only.hip"
    src.write_text('#include "%s"\nvoid* topn_instances[] = {%s};\n' % (
        fe.HEADER, ", ".join("(void*)&mals::%s" % i for i in INSTANCES)))
    out = d / "topn_only.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-S", "--cuda-device-only", "-o", str(out), str(src)],
                   check=True, capture_output=True)
    return out.read_text()


def test_filter_operands_round_to_nearest(filter_asm):
    """Every stream kernel instance holds at least one v_cvt_pk_bf16_f32 (round to nearest even, as fe.bf16) per pair of
    the 8 S item features a lane converts, and the prepare kernels' loop over the query operands holds them too.  (A
    count, not a data-flow proof: it does not exclude bit operations beside the conversions.)"""
    from tests.test_foldin_isa import bodies
    b = bodies(filter_asm)
    stream = [n for n in b if "topn_stream_kernel" in n]
    assert len(stream) == len(INSTANCES) - 2
    for n in stream:
        S = int(re.search(r"topn_stream_kernelILi(\d+)E", n).group(1))
        assert sum(1 for l in b[n] if l.startswith("v_cvt_pk_bf16_f32")) >= 4 * S, n
    prepare = [n for n in b if "topn_prepare_kernel" in n]
    assert len(prepare) == 2
    for n in prepare:
        assert sum(1 for l in b[n] if l.startswith("v_cvt_pk_bf16_f32")) >= 4, n   # 8 query features per loop step
    assert re.search(r"v_mfma_f32_16x16x32_bf16", filter_asm)
