"""The case table of the MetaOptNet-SVM head's tests (tests/test_svm_head_cpu.py establishes on the CPU what tests/test_svm_head_gpu.py
relies on).  A case is (name, (N, shots, Qn, F), B, T, Tb, variant, seed); S = N * shots.  Shapes, each a place where the kernels can go
wrong:
    (5,1,3,32)    one shot, fewer query rows than a tile          (5,5,15,64)   the 5-way 5-shot episode
    (3,2,17,40)   N not a power of two, a query-tile remainder    (20,5,20,64)  the MFMA form with several row tiles
    (64,2,16,48)  S = 128, N = 64: alpha outside LDS              (5,5,15,132)  a feature-block remainder
with B in {1, 3}, T in {1, 2, 37, 120} (both parities of the double buffer) and Tb in {1, 40} (40: the early exit of the conjugate
gradients on the small shapes).  Variants: "unbalanced" moves support rows between classes, "status" gives one support row a label out of
range and leaves one class without support rows, "offset" adds 8.0 to every feature.

Features are class centres plus noise, every row scaled to norm 3 (before the offset).  The seeds are chosen so that the float64 fit sets
aside at most 1 % of an episode's entries at the margin M_FIT and no query row at the margin 1e-5 (test_svm_head_cpu.py asserts both)."""
import numpy as np

C_REG, EPS, SCALE = 0.1, 1.0, 1.0              # the defaults of the flags
SCALE_TEST = 1.7                               # the parity tests run at a scale other than 1
M_FIT = 1e-5                                   # entries of the last projection closer than this to their bound are set aside
MAX_SET_ASIDE = 0.01                           # of an episode's S * N entries
MARGIN = 1e-5                                  # top-two logit margin below which a prediction is not compared

SHAPES = [(5, 1, 3, 32), (5, 5, 15, 64), (3, 2, 17, 40), (20, 5, 20, 64), (64, 2, 16, 48), (5, 5, 15, 132)]

CASES = (
    [(f"s{i}-B1-T120-Tb40", s, 1, 120, 40, None, 100 + i) for i, s in enumerate(SHAPES)]
    + [(f"s{i}-B3-T37-Tb1", s, 3, 37, 1, None, 200 + i) for i, s in enumerate(SHAPES)]
    + [("s1-B1-T1-Tb40", SHAPES[1], 1, 1, 40, None, 301), ("s4-B1-T1-Tb1", SHAPES[4], 1, 1, 1, None, 302),
       ("s3-B3-T2-Tb40", SHAPES[3], 3, 2, 40, None, 303), ("s4-B1-T2-Tb40", SHAPES[4], 1, 2, 40, None, 304),
       ("s0-B3-T2-Tb1", SHAPES[0], 3, 2, 1, None, 305),
       ("s1-B3-T120-Tb40-unbalanced", SHAPES[1], 3, 120, 40, "unbalanced", 401),
       ("s3-B1-T37-Tb40-unbalanced", SHAPES[3], 1, 37, 40, "unbalanced", 402),
       ("s2-B3-T120-Tb40-status", SHAPES[2], 3, 120, 40, "status", 403),
       ("s1-B1-T120-Tb40-offset", SHAPES[1], 1, 120, 40, "offset", 404)]
)
IDS = [c[0] for c in CASES]


def case_inputs(case):
    """(feats_s [B,S,F], y_s [B,S], feats_q [B,Qn,F], y_q [B,Qn]) float32 / int64 of one case, from its seed."""
    _, (N, shots, Qn, F), B, _, _, variant, seed = case
    rng = np.random.default_rng(seed)
    S = N * shots
    y_s = np.stack([rng.permutation(np.repeat(np.arange(N), shots)) for _ in range(B)]).astype(np.int64)
    if variant == "unbalanced":                # class 0 takes a row of class 1 (and, with more shots, one of class 2)
        for b in range(B):
            y_s[b, np.nonzero(y_s[b] == 1)[0][0]] = 0
            if shots > 2:
                y_s[b, np.nonzero(y_s[b] == 2)[0][0]] = 0
    y_q = rng.integers(0, N, size=(B, Qn)).astype(np.int64)
    centres = rng.standard_normal((B, N, F))

    def rows(y):
        x = np.take_along_axis(centres, np.clip(y, 0, N - 1)[..., None], axis=1) + 0.8 * rng.standard_normal(y.shape + (F,))
        return 3.0 * x / np.linalg.norm(x, axis=-1, keepdims=True)
    f_s, f_q = rows(y_s), rows(y_q)
    if variant == "status":                    # episode 1: row 0 out of range, class N - 1 without support rows
        y_s[1, 0] = N
        y_s[1][y_s[1] == N - 1] = 0
    if variant == "offset":
        f_s, f_q = f_s + 8.0, f_q + 8.0
    return f_s.astype(np.float32), y_s, f_q.astype(np.float32), y_q
