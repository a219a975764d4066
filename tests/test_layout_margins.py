"""CPU guard for the bars of tests/test_layouts_gpu.py (no GPU).

The oracle emulates each GPU mode's rounding inside the reference's arithmetic
(oracle/swps_oracle.cpp orc_set_diag_round, as scripts/diag_bfp.py: 15 = fast
mode's fp32 neu1 / neu1e / chunk partials / mean, 259 = BFP32 rows, 515 = BFP40
rows).  On the corpora of the GPU module's sections 1 and 3, at every swept D
and every (window, negative), the emulated run's distance from the unrounded
oracle must stay within one fifth of the bar the GPU test asserts: a GPU
failure is then a wrong kernel, not rounding the bar never had room for — also
after someone changes the corpus."""
import numpy as np
import pytest

from test_bench_shape_gpu import FAST_TOL_BATCH, rel_err
from test_layouts_gpu import (BFP_DIMS, CFG1, CFG3, FAST_DIMS, FP32_BAR, LIMIT_DIMS, WN_LIMITS, corpus1, corpus3,
                              make_oracle, stepped_column_p90)

BITS = {"fast": 15, "bfp32": 259, "bfp40": 515}
# one fifth of the GPU bars: fast 2e-4 -> 4e-5 (columns: 1e-5 -> 2e-6), bfp 1e-5 -> 2e-6
MARGIN = {"fast": FAST_TOL_BATCH / 5, "bfp32": FP32_BAR / 5, "bfp40": FP32_BAR / 5}
COLUMN_MARGIN = FP32_BAR / 5

CASES = ([(m, 1, D, 5, 5) for m in ("bfp32", "bfp40") for D in BFP_DIMS] + [("fast", 1, D, 5, 5) for D in FAST_DIMS]
         + [(m, 3, D, W, N) for m in ("bfp32", "bfp40", "fast") for D in LIMIT_DIMS[m] for W, N in WN_LIMITS])


@pytest.fixture(scope="module")
def runs(oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("margins")
    paths = {1: corpus1(tmp / "c1.txt"), 3: corpus3(tmp / "c3.txt")}
    cache = {}

    def run(which, D, W, N, bits):
        key = (which, D, W, N, bits)
        if key not in cache:
            cfg = dict(CFG1 if which == 1 else CFG3, window=W, negative=N)
            try:
                oracle_mod.lib().orc_set_diag_round(bits)
                orc = make_oracle(oracle_mod, paths[which], D, True, cfg)
                orc.train(1)
            finally:
                oracle_mod.lib().orc_set_diag_round(0)
            assert orc.stats()["pushes"] == 2
            cache[key] = orc.get_params()
        return cache[key]
    return run


def test_corpora_as_described(oracle_mod, tmp_path):
    """Section 1's corpus: 1216 tokens over 222 words, and a top key hot enough for multi-chunk
    runs (every token is a target record with subsampling off: more than 128 in the one minibatch)."""
    orc = make_oracle(oracle_mod, corpus1(tmp_path / "c1.txt"), 4, True, CFG1)
    _, counts = orc.vocab()
    assert orc.vocab_size == 222 and orc.train_words == 1216
    assert counts.max() > 128 + 30  # even without line 1 (at most 30 tokens), which is not in the batch
    orc3 = make_oracle(oracle_mod, corpus3(tmp_path / "c3.txt"), 4, True, CFG3)
    assert orc3.train_words > 24 * 64  # lines longer than 2 * 32 tokens


@pytest.mark.parametrize("mode", ["fast", "bfp32", "parity", "f64"])
@pytest.mark.parametrize("fault", ["dropped", "neighbour"])
def test_bars_catch_one_wrong_column(oracle_mod, runs, tmp_path, mode, fault):
    """The GPU module's check on doctored rows: the last tail element of h at D = 320 left at its
    initial value (a dropped tail lane), or holding its neighbour's value (a lane map off by one) —
    one column of 1280 — fails every mode's bar, while the emulated rounding itself passes."""
    from test_layouts_gpu import check_rows
    D, col = 320, 319
    want = runs(1, D, 5, 5, 0)
    init = make_oracle(oracle_mod, corpus1(tmp_path / "c1.txt"), D, True, CFG1).get_params()
    if mode in BITS:
        check_rows(mode, D, runs(1, D, 5, 5, BITS[mode]), want)
    got = want.copy()
    got[:, col] = init[:, col] if fault == "dropped" else want[:, col - 1]
    with pytest.raises(AssertionError):
        check_rows(mode, D, got, want)


@pytest.mark.parametrize("mode,which,D,W,N", CASES,
                         ids=["%s-s%d-D%d-W%d-N%d" % c for c in CASES])
def test_emulated_rounding_within_a_fifth_of_the_bar(runs, mode, which, D, W, N):
    want = runs(which, D, W, N, 0)
    got = runs(which, D, W, N, BITS[mode])
    assert np.isfinite(got).all()
    rel = rel_err(got, want)
    msg = "%s section %d D=%d W=%d N=%d: emulated max rel %.3g" % (mode, which, D, W, N, rel.max())
    if mode == "fast":
        col = stepped_column_p90(rel, want, D)
        msg += ", worst column p90 %.3g" % col.max()
        print(msg)
        assert col.max() <= COLUMN_MARGIN, msg
    else:
        print(msg)
    assert rel.max() <= MARGIN[mode], msg
