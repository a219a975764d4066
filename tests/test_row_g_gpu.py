"""SWPS_ROW_G = 0 and 1 train to the same bits.

SWPS_ROW_G = 1 (unset: from 65536 keys per batch, which no corpus of this
size has) carries g_0..g_N of a kept position in its BFP neu1 row, in the
zero pad after the row scale, where that pad holds N + 1 floats (swps_w2v_ctx.h
bfp_row_g); the forward then writes no pg, and the gather and
the push read a record's g with the row instead of gathering it from pg.  It
changes no sum's terms, their order or the per-element arithmetic, so the
steps below leave every table row [h | v | h2sum | v2sum] byte for byte the
same under both settings.

The corpus: 300 lines of 50 tokens, minibatch 150, subsampling off, window 1;
three steps: line 1 alone (the reference learns it before its first pull,
word2vec_global.h:630-633), then the two minibatches, lines 2..150 and
151..300.
With window 1 the reduced window is always 1 (rand % 1 = 0), so a word
occurrence is a context of exactly its in-line neighbours: an interior
occurrence adds 2 v records to its word's run, one at a line end adds 1.
Planted in the first of the two minibatches (lines 11..140), on words that
occur nowhere else:
  hot    12 interior occurrences per line: 3120 v records > kGroup * 128 =
         2048 (k_gather_b's chunks and k_combine_b's group leaders);
  r128   64 interior occurrences: a v run of exactly 128 records (the longest
         single-chunk run, summed in k_push_b);
  r129   the same plus one at a line start: 129 (the shortest multi-chunk run:
         k_gather_b);
  r1     once, at a line end: a v run of 1 record.
The fillers of the two minibatches come from disjoint halves of the
vocabulary, and negatives are drawn from all of it: about half of a
minibatch's negative draws are keys with no occurrence in its lines — an
empty v half, and short h runs (whose records are the ones that carry g).
Checked from the counters: the batches pulled more keys than their lines hold
words (negative-only keys exist); multi-chunk items exist and one run has more
than kGroup chunks (multi_items > 2 * 16); the v-record model above accounts
for the records counted (kept <= records - v records <= (N + 1) * kept).

Layouts (swps_w2v_bfp.h): D = 300 (free tail lanes carry the scale and g),
256 (NT = 0: separate loads), 64 (a full tail: no free lane), 320, bfp40 at
D = 300 (pad 8 >= N + 1); D = 28 and 508 (pad 3 < N + 1) and D = 300 with
N = 20 fall back to pg, N = 15 fits.  The fit is bfp_row_g's formula, restated
in fits() below; where it does not hold the two settings run the same code."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LINES, LEN, MB = 300, 50, 150


def fits(D, rb, N):  # swps_w2v_ctx.h: bfp_ld, bfp_row_g
    s0 = D + rb * D // 4
    return s0 + 1 + N + 1 <= (s0 + 1 + 31) // 32 * 32


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    rng = np.random.default_rng(7)
    p = 1.0 / np.arange(1, 1001)
    p /= p.sum()
    toks = [["w%d" % (x + (0 if l < MB else 1000)) for x in rng.choice(1000, LEN, p=p)] for l in range(LINES)]
    for l in range(10, 140):
        for c in range(3, 48, 4):
            toks[l][c] = "hot"
    for l in range(10, 74):
        toks[l][1] = "r128"
        toks[l][5] = "r129"
    toks[80][0] = "r129"
    toks[81][LEN - 1] = "r1"
    path = str(tmp_path_factory.mktemp("rowg") / "planted.txt")
    with open(path, "w") as f:
        for t in toks:
            f.write(" ".join(t) + "\n")
    vrec = {}  # the v records of every word: its occurrences' in-line neighbours
    for t in toks:
        for c, w in enumerate(t):
            vrec[w] = vrec.get(w, 0) + (c > 0) + (c + 1 < len(t))
    assert vrec["hot"] == 3120 and vrec["r128"] == 128 and vrec["r129"] == 129 and vrec["r1"] == 1
    words = [len({w for t in toks[a:b] for w in t}) for a, b in ((0, 1), (1, MB), (MB, LINES))]
    return path, sum(vrec.values()), sum(words)


def train(lib, path, D, mode, N, row_g, monkeypatch, profile=False):
    monkeypatch.setenv("SWPS_ROW_G", row_g)
    t = lib.Table("w2v", dim=D, capacity=2100, dtype="f32", learning_rate=0.7)
    w = lib.Word2Vec(t, window=1, negative=N, minibatch=MB, sample=-1.0, alpha=0.05, unigram_size=10 ** 6,
                     init="ref", fp64_intermediates=mode, profile=profile)
    w.load_text(path)
    w.init()
    w.train_batches(3)
    w.sync()
    return w.get_params(), w.stats(), (w.sum_stats() if profile else None)


@pytest.mark.parametrize("D,mode,N", [(300, "bfp32", 5), (256, "bfp32", 5), (64, "bfp32", 5), (320, "bfp32", 5),
                                      (300, "bfp40", 5), (28, "bfp32", 5), (508, "bfp32", 5), (300, "bfp32", 15),
                                      (300, "bfp32", 20)])
def test_row_g_bit_identical(lib, gpu, planted, monkeypatch, D, mode, N):
    path, vrecs, words = planted
    assert fits(D, int(mode == "bfp40"), N) == ((D, N) not in ((28, 5), (508, 5), (300, 20)))
    ref, st, ss = train(lib, path, D, mode, N, "0", monkeypatch, profile=True)
    assert st["batches"] == 3 and st["kept"] == LINES * LEN
    assert st["pulled"] > words  # keys drawn only as negatives: empty v halves
    assert ss["multi_items"] > 2 * 16 and ss["fused"] == ss["batches"] >= 2  # r129's two chunks, hot's 25
    assert st["kept"] <= ss["records"] - vrecs <= (N + 1) * st["kept"]
    assert np.isfinite(ref).all() and np.count_nonzero(ref[:, 2 * D:].any(axis=1)) > 1000
    got = train(lib, path, D, mode, N, "1", monkeypatch)[0]
    assert got.tobytes() == ref.tobytes(), int(np.count_nonzero((got != ref).any(axis=1)))
