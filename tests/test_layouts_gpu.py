"""Every lane layout the host can dispatch for the word2vec kernels, against
the oracle.  The instantiation is picked from the dimension D alone
(bfp_shape in swps_w2v_ctx.h, check_cfg's tail / NCH in swps_w2v_ingest.hip,
and SWPS_BFP_SHAPES / SWPS_NCH_DISPATCH / SWPS_TAIL_DISPATCH, the D < 512 /
D < 768 ladder, in swps_w2v_learn.hip), so the sweep is over D, one test id
per (mode, D) so that a failure names the layout:

  bfp40 / bfp32   k_forward_b / k_gather_b / k_push_b <NCH, NT>: <0,1> (D = 4,
                  64), <0,2> (68, 128), <1,0> (132, 200, 256), <1,1> (260,
                  320), <1,2> (324, 352, 384), <2,0> (388, 512) — the first
                  element of each new tail, a partial last 4-element chunk
                  (132, 200, 388), and the full 64-lane tails (64, 128, 320,
                  384) where ScaleLane falls back to a separate scale load;
  fast            the generic fp32 kernels NCH 1..4 and the tail kernels
                  k_forward_t / k_gather_t / k_push_t <1> (260, 320: fused
                  push), <2> (516, 576), <3> (772, 832);
  parity          the generic kernels with fp64 intermediates, NCH 1..4;
  f64             the fp64 table's generic kernels, NCH 1..4 (2-element chunks).

Section 1 input: 60 Zipf lines (1216 tokens, 222 words), window 5, negative 5,
no subsampling, ONE minibatch (line 1 is learned before the first pull, which
drops its gradients; lines 2-60 are the batch; the oracle pushes twice).  The
top key has 201 target records and ~1000 context records, so the single-chunk,
the multi-chunk (k_gather*) and the in-push sums all run.  Section 2 repeats
one D per BFP layout with 8-record chunks and the second level forced on (more
than kGroup = 16 chunks per hot run: k_combine_b leaders and the push's strided
leader reads); section 3 runs the config limits window 32 / negative 63 /
negative 0 (S = 2W + N + 1 up to 128 record slots) on 24 lines of 70-90 tokens;
section 4 sends all-zero and tiny (2^-100) rows through DAcc::st_bfp.

Bars, with rel = |gpu - oracle| / max(|oracle|, 1e-3) over the full array
[h | v | h2sum | v2sum] as in test_bench_shape_gpu.py:
  f64                      np.allclose(rtol=1e-9, atol=1e-12)
  parity, bfp40, bfp32     rel.max() <= 1e-5 (the single-batch fp32 bar)
  fast                     rel.max() <= FAST_TOL_BATCH, and in every column the
                           90th percentile of rel over the rows that took an
                           AdaGrad step <= 1e-5: rounding noise is independent
                           from column to column, a misplaced lane or tail hits
                           most rows of the columns it touches.
In every mode the two LCG end states equal the oracle's and every value is
finite.

The CPU emulation of each mode's rounding inside the oracle's arithmetic
(orc_set_diag_round; tests/test_layout_margins.py asserts these stay within
one fifth of the bars) gives, as maxima over the swept D / (W, N):
            section 1           section 3                    worst column p90
  fast      1.2e-5 (D = 4)      7.5e-6 (D = 300, W 1, N 63)  2.9e-7
  bfp32     2.0e-7 (D = 4)      3.2e-7 (D = 64, W 1, N 63)   n/a
  bfp40     1.2e-7              1.2e-7                       n/a
(1.2e-7 is the fp32 storage of the rows themselves.)
"""
import numpy as np
import pytest

from conftest import zipf_corpus
from test_bench_shape_gpu import FAST_TOL_BATCH, MODES, rel_err

pytestmark = pytest.mark.gpu

CFG1 = dict(window=5, negative=5, minibatch=60, sample=-1.0, alpha=0.05, lr=0.7, table=10 ** 6)
CFG3 = dict(CFG1, minibatch=24)
FP32_BAR = 1e-5  # parity / bfp: full-array max; fast: every column's p90 over the stepped rows

BFP_DIMS = [4, 64, 68, 128, 132, 200, 256, 260, 320, 324, 352, 384, 388, 512]
FAST_DIMS = [4, 64, 256, 260, 320, 324, 512, 516, 576, 580, 768, 772, 832, 836, 1024]
PARITY_DIMS = [256, 260, 512, 516, 768, 772, 1024]
F64_DIMS = [128, 130, 256, 258, 384, 386, 512]
BFP_ONE_PER_LAYOUT = [64, 128, 200, 320, 352, 512]
WN_LIMITS = [(1, 0), (32, 63), (32, 0), (1, 63)]
LIMIT_DIMS = {"bfp32": [64, 300, 512], "bfp40": [64, 300, 512], "fast": [300], "parity": [300], "f64": [16]}


def layout(mode, D):
    """The instantiation the host dispatches for (mode, D) — for the test ids only."""
    if mode.startswith("bfp"):
        nch, rem = divmod(D, 256)
        nch, nt = (nch, 0) if rem == 0 else (nch, (rem + 63) // 64) if rem <= 128 else (nch + 1, 0)
        return "b%d_%d" % (nch, nt)
    E = 2 if mode == "f64" else 4
    if mode == "fast" and D > 256 and 0 < D % 256 <= 64:
        return "tail%d" % (D // 256)
    return "nch%d" % ((D // E + 63) // 64)


def case_id(mode, D):
    return "%s-D%d-%s" % (mode, D, layout(mode, D))


def corpus1(path):
    return zipf_corpus(str(path), 60, 300, seed=101, lo=10, hi=30)


def corpus3(path):
    return zipf_corpus(str(path), 24, 300, seed=103, lo=70, hi=90)


def make_oracle(oracle_mod, path, D, f32, cfg):
    orc = oracle_mod.W2V(path, D, window=cfg["window"], negative=cfg["negative"], minibatch=cfg["minibatch"],
                         sample=cfg["sample"], alpha=cfg["alpha"], lr=cfg["lr"], table_size=cfg["table"],
                         storage_f32=f32)
    orc.init_rand(1, 2)
    return orc


def make_gpu(lib, path, D, mode, cfg, V):
    dtype, fp64i = MODES[mode]
    t = lib.Table("w2v", dim=D, capacity=V + 16, dtype=dtype, learning_rate=cfg["lr"])
    # profile=True: the gradient-sum counters (sum_stats) are only kept for a profiled context; the
    # kernels launched are the same
    w = lib.Word2Vec(t, window=cfg["window"], negative=cfg["negative"], minibatch=cfg["minibatch"],
                     sample=cfg["sample"], alpha=cfg["alpha"], unigram_size=cfg["table"], init="ref", rand_offset=2,
                     fp64_intermediates=fp64i, profile=True)
    w.load_text(path)
    w.init()
    return t, w


def stepped_column_p90(rel, want, D):
    """Per column of [h | v | h2 | v2]: the 90th percentile of rel over the rows whose half (h or v)
    took an AdaGrad step (a non-zero squared-gradient sum in the reference)."""
    out = np.zeros(4 * D)
    for half in (0, 1):
        rows = want[:, (2 + half) * D:(3 + half) * D].any(axis=1)
        assert rows.sum() >= 20, int(rows.sum())
        for base in (half * D, (2 + half) * D):
            out[base:base + D] = np.quantile(rel[rows, base:base + D], 0.9, axis=0)
    return out


def check_rows(mode, D, got, want, tag=""):
    assert got.shape == want.shape == (want.shape[0], 4 * D)
    assert np.isfinite(got).all()
    assert want[:, 2 * D:].any(axis=1).sum() >= 20  # keys with an AdaGrad step
    if mode == "f64":
        print("%s D=%d f64: max abs %.3g" % (tag, D, float(np.abs(got - want).max())))
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12), float(np.abs(got - want).max())
        return
    rel = rel_err(got, want)
    worst = np.unravel_index(np.argmax(rel), rel.shape)
    print("%s D=%d %s: max rel %.3g at (row %d, column %d), median %.3g"
          % (tag, D, mode, rel.max(), worst[0], worst[1], np.median(rel)))
    if mode == "fast":
        col = stepped_column_p90(rel, want, D)
        print("   worst column p90 %.3g (column %d)" % (col.max(), int(np.argmax(col))))
        assert rel.max() <= FAST_TOL_BATCH, float(rel.max())
        assert col.max() <= FP32_BAR, (float(col.max()), int(np.argmax(col)))
    else:
        assert rel.max() <= FP32_BAR, (float(rel.max()), worst)


def check_rng(w, orc):
    sg, so = w.stats(), orc.stats()
    assert sg["kept"] == so["kept"] > 0
    assert sg["lstate"] == so["rng"] and sg["fstate"] == so["frng"]


class OracleCache:
    """Trained oracles shared by the tests of this module (never modified after train)."""

    def __init__(self, oracle_mod, tmp):
        self.oracle_mod, self.tmp, self.cache, self.paths = oracle_mod, tmp, {}, {}

    def path(self, which):
        if which not in self.paths:
            self.paths[which] = {1: corpus1, 3: corpus3}[which](self.tmp / ("c%d.txt" % which))
        return self.paths[which]

    def get(self, which, D, f32, W=5, N=5):
        key = (which, D, f32, W, N)
        if key not in self.cache:
            cfg = dict(CFG1 if which == 1 else CFG3, window=W, negative=N)
            orc = make_oracle(self.oracle_mod, self.path(which), D, f32, cfg)
            orc.train(1)
            assert orc.stats()["pushes"] == 2
            self.cache[key] = (orc, orc.get_params())
        return self.cache[key]


@pytest.fixture(scope="module")
def oracles(oracle_mod, tmp_path_factory):
    return OracleCache(oracle_mod, tmp_path_factory.mktemp("layouts"))


def run_case(lib, oracles, which, mode, D, W=5, N=5):
    orc, want = oracles.get(which, D, mode != "f64", W, N)
    cfg = dict(CFG1 if which == 1 else CFG3, window=W, negative=N)
    t, w = make_gpu(lib, oracles.path(which), D, mode, cfg, orc.vocab_size)
    w.train(1)
    check_rng(w, orc)
    ss = w.sum_stats()
    print("sum stats", ss)
    assert ss["multi_items"] > 0  # no case passes without the multi-chunk path
    check_rows(mode, D, w.get_params(), want, "section %d W=%d N=%d" % (which, W, N))
    return ss


SWEEP = ([("bfp40", D) for D in BFP_DIMS] + [("bfp32", D) for D in BFP_DIMS] + [("fast", D) for D in FAST_DIMS]
         + [("parity", D) for D in PARITY_DIMS] + [("f64", D) for D in F64_DIMS])


# ---- 1. the dimension sweep ----
@pytest.mark.parametrize("mode,D", SWEEP, ids=[case_id(m, D) for m, D in SWEEP])
def test_layout_matches_oracle(lib, gpu, oracles, mode, D):
    run_case(lib, oracles, 1, mode, D)


@pytest.mark.parametrize("mode,D", [("bfp40", 516), ("bfp32", 516), ("fast", 1028), ("parity", 1028), ("f64", 514)])
def test_unsupported_dim_refused(lib, gpu, mode, D):
    """Past the last compiled layout the constructor refuses; nothing is launched."""
    dtype, fp64i = MODES[mode]
    t = lib.Table("w2v", dim=D, capacity=64, dtype=dtype, learning_rate=0.7)
    with pytest.raises(lib.SwpsError, match="SWPS_E_UNSUPPORTED.*dim"):
        lib.Word2Vec(t, window=5, negative=5, minibatch=60, unigram_size=10 ** 6, fp64_intermediates=fp64i)


# ---- 2. second-level sums at each BFP layout (and k_combine<..., NCH> behind the tail kernels) ----
COMBINE = ([("bfp40", D) for D in BFP_ONE_PER_LAYOUT] + [("bfp32", D) for D in BFP_ONE_PER_LAYOUT]
           + [("fast", 320), ("fast", 576), ("parity", 768)])


@pytest.mark.parametrize("mode,D", COMBINE, ids=[case_id(m, D) for m, D in COMBINE])
def test_layout_second_level_sums(lib, gpu, oracles, monkeypatch, mode, D):
    """8-record chunks and the second level forced on: every run of more than 128 records has more
    than kGroup = 16 chunks, so group leaders (k_combine_b / k_combine) sum them and the push reads
    the leaders with a stride."""
    monkeypatch.setenv("SWPS_COMBINE", "1")
    monkeypatch.setenv("SWPS_MULTI_CHUNK", "8")
    ss = run_case(lib, oracles, 1, mode, D)
    # the 8-record chunks took effect: every multi-chunk run (> 128 records) has more than 16 of them
    assert ss["multi_items"] >= ss["multi_records"] / 8 > 16


# ---- 3. window and negative limits ----
LIMITS = [(m, D, W, N) for m in ("bfp32", "bfp40", "fast", "parity", "f64") for D in LIMIT_DIMS[m] for W, N in WN_LIMITS]


@pytest.mark.parametrize("mode,D,W,N", LIMITS, ids=["%s-W%d-N%d" % (case_id(m, D), W, N) for m, D, W, N in LIMITS])
def test_window_negative_limits(lib, gpu, oracles, mode, D, W, N):
    """S = 2W + N + 1 = 3, 65, 66 and 128 record slots (the first three no multiple of the
    forward's G rows in flight);
    lines of 70-90 tokens fill all 64 context slots at window 32 (the top key has 343 target
    records: multi-chunk runs here too)."""
    run_case(lib, oracles, 3, mode, D, W, N)


@pytest.mark.parametrize("W,N", [(33, 5), (5, 64)])
def test_window_negative_past_limits_refused(lib, gpu, W, N):
    t = lib.Table("w2v", dim=16, capacity=64, dtype="f32", learning_rate=0.7)
    with pytest.raises(lib.SwpsError, match="SWPS_E_CFG: (window|negative)"):
        lib.Word2Vec(t, window=W, negative=N, minibatch=24, unigram_size=10 ** 6)


def test_s2v_negative_63_refused(lib, gpu, tmp_path):
    """sent2vec's record holds one slot more: negative stops at 62."""
    from conftest import int_corpus
    corpus = int_corpus(str(tmp_path / "c.txt"), 10, 20, seed=1)
    t = lib.Table("w2v", dim=8, capacity=64, dtype="f64")
    s = lib.Sent2Vec(t, window=2, negative=63, minibatch=3, unigram_size=10 ** 5)
    with pytest.raises(lib.SwpsError, match="SWPS_E_CFG: negative"):
        s.load_text(corpus)  # the context is created on the first load


# ---- 4. zero and tiny rows through the BFP encoder ----
@pytest.mark.parametrize("D", [64, 300, 512])
@pytest.mark.parametrize("mode", ["bfp40", "bfp32"])
def test_bfp_zero_rows_exact(lib, oracle_mod, gpu, oracles, mode, D):
    """Every h and v element 1.0 and no negatives: every dot is at least D > 6, the sigmoid
    saturates, every g is 0 and every neu1e row is all zero (DAcc::st_bfp's exponent clamp encodes
    it).  Rows stay as set, the squared-gradient sums stay 0, bit for bit as in the oracle."""
    cfg = dict(CFG1, negative=0)
    path = oracles.path(1)
    orc = make_oracle(oracle_mod, path, D, True, cfg)
    V = orc.vocab_size
    hv = np.ones((V, 2 * D))
    orc.set_params(hv)
    t, w = make_gpu(lib, path, D, mode, cfg, V)
    w.set_params(hv)
    orc.train(1)
    w.train(1)
    check_rng(w, orc)
    assert w.sum_stats()["multi_items"] > 0
    want, got = orc.get_params(), w.get_params()
    assert np.array_equal(want[:, :2 * D], hv) and not want[:, 2 * D:].any()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("D", [64, 300, 512])
@pytest.mark.parametrize("mode", ["bfp40", "bfp32"])
def test_bfp_tiny_rows_finite(lib, oracle_mod, gpu, oracles, mode, D):
    """The initial rows times 2^-100: the row exponent is clamped so that the scale stays a normal
    fp32 (u >= 2^-126), which leaves fewer mantissa bits but |error| <= u/2 per element.  AdaGrad's
    first step passes a gradient error on times lr / sqrt(fudge) = 700: rows within the fp32 bar
    relative to the rows' own scale plus 700 clamp units, and finite."""
    path = oracles.path(1)
    orc = make_oracle(oracle_mod, path, D, True, CFG1)
    V = orc.vocab_size
    hv = orc.get_params()[:, :2 * D] * 2.0 ** -100
    orc.set_params(hv)
    t, w = make_gpu(lib, path, D, mode, CFG1, V)
    w.set_params(hv)
    orc.train(1)
    w.train(1)
    check_rng(w, orc)
    want, got = orc.get_params(), w.get_params()
    assert np.isfinite(got).all()
    assert np.abs(want[:, :2 * D] - hv).max() > 2.0 ** -110  # the batch moved the rows
    err = np.abs(got - want)
    bound = 1e-5 * np.maximum(np.abs(want), 1e-3 * 2.0 ** -100) + 700 * 2.0 ** -126
    print("tiny rows D=%d %s: max err %.3g = %.3g of the bound" % (D, mode, err.max(), (err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
