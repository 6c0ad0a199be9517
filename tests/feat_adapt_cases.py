"""The case table of the set-to-set prototype adaptation, shared by tests/test_feat_adapt_cpu.py and tests/test_feat_adapt_gpu.py.

Shapes are the smallest that reach each edge: N on both sides of the 16-row MFMA tile (2, 5, 16, 17) and at the limit (64); F at the
smallest width (32), off the 64-column GEMM tile and the 128-feature block (96) and at the ResNet-12 width (640: more than two
256-feature blocks of the means kernel); F = 2048 once; B = 1 and 3 (B N = 192: three 64-row GEMM tiles, two 128-row chunks of the
column sums); unequal class counts that always include a class with one row; one case with out-of-range support labels, one with a
class that has no support row.

Three input regimes:
  unit       features N(0, 1), scaled until the scores Q K^T / sqrt(F) have standard deviation 1: the attention is neither uniform nor one-hot;
  saturated  the same features, the classes at scales spread log-uniformly over a factor of 100, then all scaled until the mean gap
             between a row's two largest scores is 50: exercises the max subtraction.  The spread keeps a few rows of the attention
             soft: where every row is one-hot the gradients of Wq and Wk are of the size e^-50 and round-off is all that any fp32
             arithmetic returns for them, so a table of such rows alone would measure nothing;
  offset     post-ReLU-like features max(8 + N(0, 1), 0): a common offset of 8.  At the initialisation scale the offset alone puts
             a spread of about 8 into a row of the scores, so these cases need rows enough (B N >= 5, several shots) for some of
             them to stay soft, for the reason given above.
Weights are random at the initialisation scale (std sqrt(2 / (F + F)) for all four projections), with non-trivial bo, gamma, beta."""
import numpy as np

from feat_adapt_ref import feat_adapt_fwd_ref

# name: (B, N, F, class counts (cycled over the classes), regime, label case)
CASES = {
    "n2_f32_unit": (1, 2, 32, (1, 3), "unit", None),
    "n5_f96_unit": (3, 5, 96, (1, 2, 3, 4, 5), "unit", None),
    "n5_f32_unit": (1, 5, 32, (2, 1, 3), "unit", None),
    "n16_f640_saturated": (1, 16, 640, (1, 2, 3), "saturated", None),
    "n17_f96_offset": (3, 17, 96, (2, 1, 4), "offset", None),
    "n64_f32_saturated": (1, 64, 32, (1, 2), "saturated", None),
    "n64_f640_unit": (3, 64, 640, (1, 3, 2), "unit", None),
    "n5_f2048_offset": (1, 5, 2048, (5, 1, 4, 2, 3), "offset", None),
    "n5_f640_saturated": (3, 5, 640, (5, 1, 5, 3, 5), "saturated", None),
    "n5_f96_label_range": (3, 5, 96, (1, 2, 3, 4, 5), "unit", "label_range"),
    "n5_f96_class_missing": (3, 5, 96, (1, 2, 3, 4, 5), "unit", "class_missing"),
}
SMALLEST = ("n2_f32_unit", "n5_f32_unit", "n5_f96_unit")       # the finite-difference check runs on these
SATURATED_GAP = 50.0
SPREAD = 100.0                     # saturated: the ratio of the largest to the smallest class scale
OFFSET = 8.0
LEFT_OUT = (0, 2)                  # label_range: the episodes in which one support label is made N, and -1
MISSING = (1, 3)                   # class_missing: (episode, class) whose rows are relabelled to class 0

# the composition case: 5-way 5-shot, Qn = 15, F = 64, B = 2
COMPOSE = dict(B=2, N=5, shots=5, Qn=15, F=64)
MARGIN = 1e-5                      # predictions are compared on rows whose float64 top-two logit margin exceeds this


def make_weights(rng, F):
    """(wqkv [3F,F], wo [F,F], bo, gamma, beta [F]) float32 at the initialisation scale, bo / gamma / beta non-trivial."""
    std = np.sqrt(2.0 / (F + F))
    wqkv = rng.standard_normal((3 * F, F)) * std
    wo = rng.standard_normal((F, F)) * std
    bo = 0.1 * rng.standard_normal(F)
    gamma = 1.0 + 0.3 * rng.standard_normal(F)
    beta = 0.2 * rng.standard_normal(F)
    return tuple(t.astype(np.float32) for t in (wqkv, wo, bo, gamma, beta))


def mean_top2_gap(scores):
    top2 = np.sort(scores, axis=-1)[..., -2:]
    return float((top2[..., 1] - top2[..., 0]).mean())


def make_case(name):
    """dict(B, S, N, F, regime, label_case, feats_s [B,S,F] f32, y_s [B,S] i64, w (5 f32 arrays), dprotos [B,N,F] f32)."""
    B, N, F, counts, regime, label_case = CASES[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    per_class = [counts[n % len(counts)] for n in range(N)]
    S = sum(per_class)
    base = np.repeat(np.arange(N), per_class)
    y_s = np.stack([rng.permutation(base) for _ in range(B)]).astype(np.int64)
    w = make_weights(rng, F)
    x = rng.standard_normal((B, S, F))
    if regime == "offset":
        x = np.maximum(OFFSET + x, 0.0)
    if label_case == "label_range":      # in LEFT_OUT's episodes, the first row of a class that keeps another row: labels N and -1
        for b, bad in zip(LEFT_OUT, (N, -1)):
            s0 = next(i for i in range(S) if (y_s[b] == y_s[b, i]).sum() > 1)
            y_s[b, s0] = bad
    if label_case == "class_missing":
        y_s[MISSING[0]][y_s[MISSING[0]] == MISSING[1]] = 0
    if regime == "saturated":            # classes at scales spread over SPREAD: rows of the attention from soft to one-hot
        x = x * np.exp(np.log(SPREAD) * (rng.permutation(N) / (N - 1.0) - 0.5))[np.clip(y_s, 0, N - 1)][..., None]
    if regime != "offset":               # the scores are quadratic in the features: scale them to the regime's statistic
        sc = feat_adapt_fwd_ref(x.astype(np.float32), y_s, *w, N)["scores"]
        x = x * np.sqrt(SATURATED_GAP / mean_top2_gap(sc) if regime == "saturated" else 1.0 / sc.std())
    dprotos = rng.standard_normal((B, N, F)).astype(np.float32)
    return dict(name=name, B=B, S=S, N=N, F=F, regime=regime, label_case=label_case, feats_s=x.astype(np.float32), y_s=y_s, w=w,
                dprotos=dprotos)


def make_compose():
    """The composition case: dict(feats_s [B,S,F], y_s, feats_q [B,Qn,F], y_q, w, N), class-structured so the head has something to
    classify (class centres N(0,1), rows centre + 0.7 N(0,1))."""
    c = COMPOSE
    B, N, K, Qn, F = c["B"], c["N"], c["shots"], c["Qn"], c["F"]
    rng = np.random.default_rng(4343)
    centres = rng.standard_normal((B, N, F))
    y_s = np.stack([rng.permutation(np.repeat(np.arange(N), K)) for _ in range(B)]).astype(np.int64)
    y_q = np.stack([rng.permutation(np.repeat(np.arange(N), Qn // N)) for _ in range(B)]).astype(np.int64)
    rows = lambda y: (np.take_along_axis(centres, y[..., None], axis=1) + 0.7 * rng.standard_normal((B, y.shape[1], F)))
    return dict(feats_s=rows(y_s).astype(np.float32), y_s=y_s, feats_q=rows(y_q).astype(np.float32), y_q=y_q,
                w=make_weights(rng, F), N=N)
