"""The form table of the episode chain (csrc/episode.hip: plan_episodes), shared by
tests/test_epi_forms_cpu.py, tests/test_epi_forms_gpu.py and tools/epi_forms_report.py -- TEST INFRASTRUCTURE ONLY.

One row per case: the smallest shape that reaches a form of the adapt / query / reverse kernels or of the backward X-panel pass, or
that sits on one side of one of the edges between two forms.  A row is (id, entry, B, N, K, Q, D, hidden sizes, T, options) and the
plan `fumi_hip_epi_plan` must report for it: the eight FORM entries are written out by hand, the ten derived entries (slab counts,
LDS totals, staging units) were read off `fumi_hip_epi_plan_query` once and are pinned here, so that a layout function or a staging
builder that moves shows up as a changed number on a machine without a GPU.  S = N K support rows, Qn = N Q query rows.

No row costs more than MAX_MACS = 2e8 multiply-adds, counted as B (S + Qn) (D h0 + S D + 3 (T + 1) sum_i h_i h_{i-1}).

Forms the C ABI cannot reach with the reference widths: `fused` by S = 29..32 at h = [256, 64].  The fused layout of that network
holds 28 support rows at most (29..32 rows: 40776 floats, over the 40000 cap), so such a step loses `fused_fixed` to `lds` with a
`global` adapt launch, not to `fused` (rows q_fixed_s28 / q_lds_s30); narrower networks reach `fused` at S = 29..32 (q_fused_s32).
The product ceil(S/16) ceil(h0/64) of the adapt kernel cannot step from 8 to 9 by one granule (9 = 3 x 3 only): the table holds 8
(a_lds_blocks8) and 9 (a_glob_blocks9) at layouts that both fit, so the product alone decides.

The 512-unit cap of the staging tables (stage_ok).  A copy unit moves 256 floats of a job whose rows are 16-byte aligned (vec) and 64
floats otherwise, so 512 units are at least 32768 floats of non-vec jobs and the 40000-float layout, which holds every staged
matrix, binds first unless most of the table is non-vec.  The query table gets there with h0 % 4 != 0 (A0, D and W_1 rows lose
vec): s_q511_s28 | s_qglob_s30, 511 units against a layout that still fits.  The adapt table gets there the same way:
s_a512_h126 | s_aglob_h127, 512 units against 516 at the same layout total.  The fused query table needs h0 % 4 == 0 and at most 32
support rows, and both reverse tables need h0 % 4P == 0 with every carved base aligned, so their wide jobs are always vec: over
200000 random shapes (1..3 hidden layers, widths 1..300, N 1..33, S up to 64, parameters aligned and one float off) the largest
tables that still took the LDS-resident form had 401 (fused), 215 (reverse, first) and 276 (reverse, per step) units.  For those
three the LDS cap always binds first and the table has no pair."""
import os
from collections import OrderedDict

import torch

from helpers import dropout_mask, rel_to_max
from oracle import casegen as cg, fumi_ref as R

MAX_MACS = 2e8
LOGIT_TOL, GRAD_TOL, MARGIN = 1e-4, 1e-4, 1e-5         # the project's bounds (tests/test_hip_parity.py)
WITNESS_TOL = 2e-5     # the float32 oracle against its own float64 run: a fifth of the bound, far above summation-order noise
# Form bound: a form's error against float64 may exceed the float32 oracle's on the same row by this factor (measured on every row,
# profiles/epi_forms/errors.json: the smallest power of two that is at least twice the largest ratio seen).  Errors below
# ERR_FLOOR (2^-22 of the reference's maximum: a few float32 roundings) count as ERR_FLOOR on both sides.
FORM_MARGIN = 16
ERR_FLOOR = 2.0 ** -22
DROP_SEED = 0x1234_5678_9ABC_DEF1

FORM_KEYS = ("adapt", "AP", "query", "reverse", "P", "two_part", "drop", "fixed_last")
DERIVED_KEYS = ("nsq", "nss", "ql_total", "al_total", "rl_total", "nu_adapt", "nu_query", "nu_fused", "nu_rev_init", "nu_rev_step")
PLAN_KEYS = ("adapt", "AP", "query", "reverse", "P", "two_part", "nsq", "nss", "drop", "fixed_last",
             "ql_total", "al_total", "rl_total", "nu_adapt", "nu_query", "nu_fused", "nu_rev_init", "nu_rev_step")   # = hip.EPI_PLAN_KEYS
ADAPT = {"none": 0, "lds": 1, "global": 2}
QUERY = {"fused_fixed": 0, "fused": 1, "lds": 2, "global": 3}
REVERSE = {"lds_fixed": 0, "lds": 1, "global": 2}
LDS_CAP, UNIT_CAP = 40000, 512
LDS_MAX = 40960        # floats of LDS a CU has: a cap moved there must fail a row (CAP_OUTSIDE)
REF = [256, 64]

# ---- the three layouts of csrc/episode.hip restated (adapt_layout, query_layout, reverse_layout: totals only).  The plan reports
# the total of a layout it took; these give the total of one it REJECTED, which is what places a row just outside a cap.
_r4 = lambda x: (x + 3) & ~3
_r16 = lambda x: (x + 15) & ~15
_ld = lambda c: ((c + 31) & ~31) + 4          # wg_ld
QR = 32


def adapt_total(h, S, N):
    RS = _r4(S)
    t = sum(RS * _ld(x) for x in h) + sum(RS * _ld(x) for x in h[1:]) + RS * (_ld(S) + _ld(N) + _ld(h[0]))
    t += sum(_r16(h[i]) * _ld(h[i - 1]) + _r4(h[i]) for i in range(1, len(h)))
    return t + _r16(N) * _ld(h[-1]) + _r4(h[0]) + _r4(N) + 64


def query_total(h, S, N, fused=False):
    t = sum(QR * _ld(x) for x in h) + sum(_r16(h[i]) * _ld(h[i - 1]) + _r4(h[i]) for i in range(1, len(h)))
    t += _r16(N) * _ld(h[-1]) * (2 if fused else 1)
    return t + QR * _ld(S) + _r4(S) * _ld(h[0]) + QR * _ld(N) + 3 * _r4(h[0]) + _r4(N)


def reverse_total(h, S, N, P):
    RS, h0c = _r4(S), h[0] // P
    t = 0
    for i in range(1, len(h)):
        kc = h0c if i == 1 else h[i - 1]
        t += 2 * _r16(h[i]) * _ld(kc) + _r4(h[i]) + 3 * RS * _ld(h[i])
    t += 5 * RS * _ld(h0c) + 2 * RS * _ld(max([4] + list(h[1:]))) + 2 * _r16(N) * _ld(h[-1]) + 3 * RS * _ld(N) + RS * _ld(S)
    return t + 2 * _r4(h0c) + _r4(N) + 64


def _row(entry, B, N, K, Q, D, hid, T, form, derived, **o):
    """form: 'adapt/AP query reverse/P two_part drop fixed_last' by name; derived: the ten DERIVED_KEYS."""
    a, q, r, tp, dr, fl = form.split()
    an, ap = a.split("/")
    rn, rp = r.split("/")
    plan = dict(adapt=ADAPT[an], AP=int(ap), query=QUERY[q], reverse=REVERSE[rn], P=int(rp), two_part=int(tp), drop=int(dr),
                fixed_last=int(fl))
    assert len(derived) == len(DERIVED_KEYS)
    plan.update(zip(DERIVED_KEYS, derived))
    c = dict(entry=entry, B=B, N=N, K=K, Q=Q, D=D, hid=list(hid), T=T, Dt=16, Ht=16, tanh=False, dropout=0.0, first_order=False,
             need_grad=True, off=None, plan=plan)
    c.update(o)
    return c


# id -> row.  Seeds: SEEDS below (SEED_OVERRIDE where the seed has a near-tie or a ReLU on a kink).
CASES = OrderedDict([
    # ---- query: fused_fixed, and every way of losing it
    ("q_fixed", _row("fumi", 2, 5, 5, 3, 64, REF, 1, "none/1 fused_fixed lds_fixed/4 0 0 3", (0, 0, 39736, 0, 37512, 0, 0, 113, 41, 47))),
    ("q_fixed_drop", _row("fumi", 2, 5, 5, 3, 64, REF, 1, "none/1 fused_fixed lds_fixed/4 0 1 3", (0, 0, 39736, 0, 37512, 0, 0, 113, 41, 47),
                          dropout=0.25, tanh=True)),
    ("q_fixed_s28", _row("fumi", 2, 2, 14, 3, 64, REF, 1, "none/1 fused_fixed lds_fixed/4 0 0 3", (0, 0, 39736, 0, 37512, 0, 0, 101, 31, 40))),
    ("q_lds_s30", _row("fumi", 2, 2, 15, 3, 64, REF, 1, "global/1 lds lds_fixed/4 0 0 2", (0, 0, 39684, 0, 37512, 0, 147, 0, 43, 43))),
    ("q_fixed_n8", _row("fumi", 2, 8, 2, 2, 64, REF, 1, "none/1 fused_fixed lds/2 0 0 1", (0, 0, 39736, 0, 37768, 0, 0, 93, 46, 52))),
    ("q_fused_n9", _row("fumi", 2, 9, 2, 2, 64, REF, 1, "none/1 fused lds/4 0 0 0", (0, 0, 37660, 0, 27628, 0, 0, 110, 36, 44))),
    ("q_fused_h128", _row("fumi", 2, 5, 5, 3, 64, [128, 64], 1, "none/1 fused lds/2 0 0 0", (0, 0, 23480, 0, 34216, 0, 0, 69, 41, 47))),
    ("q_fused_nograd", _row("fumi", 2, 5, 5, 3, 64, REF, 1, "none/1 fused lds/4 0 0 0", (0, 0, 39736, 0, 34216, 0, 0, 113, 41, 47),
                            need_grad=False)),
    # the run-time-shaped fused kernel on the REFERENCE layout (ql_total 39736): only the 16-byte test of one parameter fails
    ("q_fused_w1off", _row("fumi", 2, 5, 5, 3, 64, REF, 1, "none/1 fused lds_fixed/4 0 0 2", (0, 0, 39736, 0, 37512, 0, 0, 305, 41, 47), off="W1")),
    ("q_fused_b1off", _row("fumi", 2, 5, 5, 3, 64, REF, 1, "none/1 fused lds_fixed/4 0 0 2", (0, 0, 39736, 0, 37512, 0, 0, 113, 41, 47), off="b1")),
    ("q_fused_b0off", _row("fumi", 2, 5, 5, 3, 64, REF, 1, "none/1 fused lds_fixed/4 0 0 2", (0, 0, 39736, 0, 37512, 0, 0, 116, 41, 47), off="b0")),
    # ---- query: fused (run-time shape), and every way of losing it to lds
    ("q_fused_small", _row("fumi", 2, 3, 2, 2, 32, [8, 4], 1, "none/1 fused lds/1 0 0 0", (0, 0, 6656, 0, 6424, 0, 0, 10, 7, 7))),
    ("q_lds_t2", _row("fumi", 2, 3, 2, 2, 32, [8, 4], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 6080, 2960, 6424, 5, 12, 0, 7, 7), tanh=True)),
    ("q_lds_l1", _row("fumi", 2, 3, 2, 2, 32, [8], 1, "lds/1 lds global/0 0 0 0", (0, 0, 4348, 1804, 0, 3, 10, 0, 0, 0))),
    ("q_lds_l3", _row("fumi", 2, 3, 2, 2, 32, [8, 8, 4], 1, "lds/1 lds lds/1 0 0 0", (0, 0, 7816, 4120, 8448, 7, 14, 0, 9, 10))),
    ("q_fused_s32", _row("fumi", 2, 2, 16, 2, 32, [16, 8], 1, "none/1 fused lds/1 0 0 0", (0, 0, 7548, 0, 18540, 0, 0, 11, 11, 8))),
    ("q_lds_s33", _row("fumi", 2, 3, 11, 2, 32, [16, 8], 1, "lds/1 lds lds/1 0 0 0", (0, 0, 8140, 10172, 21708, 37, 43, 0, 41, 15))),
    ("q_fused_h12", _row("fumi", 2, 3, 2, 2, 32, [12, 4], 1, "none/1 fused lds/1 0 0 0", (0, 0, 6668, 0, 6432, 0, 0, 10, 7, 7))),
    ("q_lds_h10", _row("fumi", 2, 3, 2, 2, 32, [10, 4], 1, "lds/1 lds global/0 0 0 0", (0, 0, 6092, 2964, 0, 5, 20, 0, 0, 0))),
    ("q_fused_h256", _row("fumi", 2, 3, 2, 2, 32, [256, 8], 1, "none/1 fused lds/1 0 0 0", (0, 0, 19948, 0, 23052, 0, 0, 22, 19, 19))),
    ("q_lds_h260", _row("fumi", 2, 3, 2, 2, 32, [260, 8], 1, "lds/1 lds lds/1 0 0 0", (0, 0, 21176, 11408, 25364, 20, 103, 0, 34, 33))),
    # the fused layout (40776) over the cap while the plain one (39688) fits; its adapt layout does not fit either
    ("q_lds_s32n8", _row("fumi", 2, 8, 4, 2, 64, REF, 1, "global/1 lds lds_fixed/4 0 0 2", (0, 0, 39688, 0, 37512, 0, 138, 0, 33, 44))),
    # ---- query and adapt: global by layout
    ("q_glob_h512", _row("fumi", 2, 3, 2, 2, 32, [512, 64], 1, "global/1 global lds/4 0 0 0", (0, 0, 0, 0, 28612, 0, 0, 0, 40, 42))),
    # ---- adapt: lds / global by layout / global by the one-block-per-wave product (6, 8 -> 9)
    ("a_lds_blocks6", _row("fumi", 2, 2, 16, 2, 64, [192, 64], 2, "lds/1 lds lds/4 0 0 0", (0, 0, 31300, 33156, 37476, 72, 137, 0, 32, 43))),
    ("a_glob_layout", _row("fumi", 2, 2, 16, 2, 64, REF, 2, "global/1 lds lds/4 0 0 0", (0, 0, 39684, 0, 37508, 0, 137, 0, 32, 43))),
    ("a_lds_blocks8", _row("fumi", 2, 2, 25, 2, 32, [128, 16], 2, "lds/1 lds lds/2 0 0 0", (0, 0, 18660, 25780, 39732, 61, 86, 0, 71, 30))),
    ("a_glob_blocks9", _row("fumi", 2, 3, 11, 2, 32, [192, 16], 2, "global/1 lds lds/2 0 0 0", (0, 0, 22116, 0, 35444, 0, 118, 0, 62, 38))),
    # ---- reverse: P = 1 -> 2 -> 4 -> 8 -> generic, each step an inside / outside pair
    ("r_p1_h192", _row("fumi", 2, 2, 4, 2, 32, [192, 64], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 26596, 18756, 39492, 69, 110, 0, 77, 79))),
    ("r_p2_h256", _row("fumi", 2, 2, 4, 2, 32, REF, 2, "lds/1 lds lds/2 0 0 0", (0, 0, 33444, 23940, 28612, 69, 110, 0, 41, 43))),
    ("r_p8_h320", _row("fumi", 2, 2, 16, 2, 32, [320, 64], 2, "global/1 global lds/8 0 0 0", (0, 0, 0, 0, 37460, 0, 0, 0, 32, 43))),
    ("r_p8_h512", _row("fumi", 2, 2, 16, 2, 32, [512, 64], 2, "global/1 global lds/8 0 0 0", (0, 0, 0, 0, 37508, 0, 0, 0, 32, 43))),
    ("r_glob_h576", _row("fumi", 2, 2, 16, 2, 32, [576, 64], 2, "global/1 global global/0 0 0 0", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0))),
    # the same steps by S alone (N = 2, K = S / 2), every other form entry unchanged; the rejected layouts in the comments
    ("r_p1_s16", _row("fumi", 2, 2, 8, 2, 32, [192, 32], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 20324, 15716, 35044, 36, 87, 0, 53, 55))),
    ("r_p2_s18", _row("fumi", 2, 2, 9, 2, 32, [192, 32], 2, "lds/1 lds lds/2 0 0 0", (0, 0, 21108, 17860, 24324, 44, 103, 0, 38, 34))),             # P = 1: 40260
    ("r_p2_s16", _row("fumi", 2, 2, 8, 2, 32, REF, 2, "lds/1 lds lds/2 0 0 0", (0, 0, 35524, 29764, 37764, 69, 119, 0, 45, 51))),
    ("r_p4_s18", _row("fumi", 2, 2, 9, 2, 32, REF, 2, "lds/1 lds lds/4 0 0 0", (0, 0, 36564, 32676, 27620, 77, 135, 0, 34, 34))),                   # P = 2: 42340
    ("r_p4_s24", _row("fumi", 2, 2, 12, 2, 32, [320, 64], 2, "global/1 global lds/4 0 0 0", (0, 0, 0, 0, 38884, 0, 0, 0, 51, 59))),
    ("r_p8_s26", _row("fumi", 2, 2, 13, 2, 32, [320, 64], 2, "global/1 global lds/8 0 0 0", (0, 0, 0, 0, 34164, 0, 0, 0, 40, 40))),      # P = 4: 42820
    ("r_p8_s44", _row("fumi", 2, 2, 22, 2, 32, REF, 2, "global/1 global lds/8 0 0 0", (0, 0, 0, 0, 37604, 0, 0, 0, 29, 41))),
    ("r_glob_s46", _row("fumi", 2, 2, 23, 2, 32, REF, 2, "global/1 global global/0 0 0 0", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0))),       # P = 8: 40388
    # ---- the adapt layout just outside its cap (40196), by S alone
    ("a_lds_s40", _row("fumi", 2, 2, 20, 2, 32, [96, 128], 2, "lds/1 lds global/0 0 0 0", (0, 0, 30084, 37924, 0, 80, 113, 0, 0, 0))),
    ("a_glob_s42", _row("fumi", 2, 2, 21, 2, 32, [96, 128], 2, "global/1 lds global/0 0 0 0", (0, 0, 30484, 0, 0, 0, 138, 0, 0, 0))),
    # ---- the 512-unit cap of the staging tables: the query table (h0 % 4 != 0: no 16-byte rows) and the adapt table
    ("s_q511_s28", _row("fumi", 2, 2, 14, 2, 32, [254, 64], 1, "lds/1 lds global/0 0 0 0", (0, 0, 38644, 38500, 0, 264, 511, 0, 0, 0))),
    ("s_qglob_s30", _row("fumi", 2, 2, 15, 2, 32, [254, 64], 1, "global/1 global global/0 0 0 0", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0))),   # layout 39684 fits; the adapt layout (41412) does not
    ("s_a512_h126", _row("fumi", 2, 2, 2, 2, 32, [250, 126], 2, "lds/1 global global/0 0 0 0", (0, 0, 0, 39264, 0, 512, 0, 0, 0, 0))),
    ("s_aglob_h127", _row("fumi", 2, 2, 2, 2, 32, [250, 127], 2, "global/1 global global/0 0 0 0", (0, 0, 0, 0, 0, 0, 0, 0, 0, 0))),  # 516 units, same layout total
    ("r_lds_l4", _row("fumi", 2, 3, 2, 2, 32, [8, 8, 8, 4], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 9552, 5280, 10472, 9, 16, 0, 11, 13), tanh=True)),
    ("r_glob_l5", _row("fumi", 2, 3, 2, 2, 32, [8, 8, 8, 8, 4], 2, "lds/1 lds global/0 0 0 0", (0, 0, 11288, 6440, 0, 11, 18, 0, 0, 0), tanh=True)),
    ("r_lds_q256", _row("fumi", 1, 2, 1, 128, 32, [8, 4], 1, "none/1 fused lds/1 0 0 0", (0, 0, 6512, 0, 4408, 0, 0, 7, 7, 7))),
    ("r_glob_q258", _row("fumi", 1, 2, 1, 129, 32, [8, 4], 1, "none/1 fused global/0 0 0 0", (0, 0, 6512, 0, 0, 0, 0, 7, 0, 0))),
    # ---- backward X-panel pass: two launches at B Qn = 2048 (D % 128 == 0 and h0 % 256 == 0: xpanel_bwd_two_part_ok), one below, refused at D = 64
    ("b_two_2048", _row("fumi", 8, 4, 1, 64, 128, [256, 8], 2, "lds/1 lds lds/1 1 0 0", (32, 1, 18332, 7724, 16556, 12, 50, 0, 17, 17))),
    ("b_one_2016", _row("fumi", 8, 4, 1, 63, 128, [256, 8], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 18332, 7724, 16556, 12, 50, 0, 17, 17))),
    ("b_one_d64", _row("fumi", 8, 4, 1, 64, 64, [256, 8], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 18332, 7724, 16556, 12, 50, 0, 17, 17))),
    # ---- variants the kernels branch on
    ("v_t0", _row("fumi", 2, 3, 2, 2, 32, [8, 4], 0, "lds/1 lds lds/1 0 0 0", (0, 0, 6080, 2960, 6424, 5, 12, 0, 7, 7))),
    ("v_eval_t2", _row("fumi", 2, 3, 2, 2, 32, [8, 4], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 6080, 2960, 6424, 5, 12, 0, 7, 7), need_grad=False)),
    ("v_drop_t2", _row("fumi", 2, 3, 2, 2, 32, [8, 4], 2, "lds/1 lds lds/1 0 1 0", (0, 0, 6080, 2960, 6424, 5, 12, 0, 7, 7), dropout=0.25)),
    ("v_n17", _row("fumi", 2, 17, 1, 1, 32, [8, 4], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 7104, 6144, 13640, 14, 24, 0, 15, 23))),
    ("v_n1_one_row", _row("fumi", 1, 1, 1, 1, 32, [8, 4], 1, "none/1 fused lds/1 0 0 0", (0, 0, 6512, 0, 4408, 0, 0, 7, 7, 7))),
    ("v_n2_b1", _row("fumi", 1, 2, 1, 1, 32, [8, 4], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 5936, 2096, 4408, 5, 9, 0, 7, 7))),
    ("v_ragged_q33", _row("fumi", 2, 3, 2, 11, 32, [8, 4], 1, "none/1 fused lds/1 0 0 0", (0, 0, 6656, 0, 6424, 0, 0, 10, 7, 7), tanh=True)),
    ("v_b9_fixed", _row("fumi", 9, 5, 5, 3, 64, REF, 1, "none/1 fused_fixed lds_fixed/4 0 0 3", (0, 0, 39736, 0, 37512, 0, 0, 113, 41, 47))),
    ("v_b9_p2", _row("fumi", 9, 2, 4, 2, 32, REF, 2, "lds/1 lds lds/2 0 0 0", (0, 0, 33444, 23940, 28612, 69, 110, 0, 41, 43))),
    ("v_b1_p4", _row("fumi", 1, 5, 5, 3, 64, REF, 2, "lds/1 lds lds/4 0 0 0", (0, 0, 38648, 38504, 34216, 84, 143, 0, 41, 47))),
    # ---- the MAML entry: first order (no tape, no two-launch pass, no fixed shape), second order
    ("m_first_t2", _row("maml", 3, 4, 3, 3, 32, [16, 8], 2, "lds/1 lds lds/1 0 0 0", (0, 0, 6252, 3836, 8460, 5, 11, 0, 7, 7), first_order=True)),
    ("m_first_t1", _row("maml", 2, 5, 5, 3, 64, REF, 1, "none/1 fused lds/4 0 0 0", (0, 0, 39736, 0, 34216, 0, 0, 113, 41, 47), first_order=True)),
    ("m_second_t1", _row("maml", 2, 3, 2, 2, 32, [8, 4], 1, "none/1 fused lds/1 0 0 0", (0, 0, 6656, 0, 6424, 0, 0, 10, 7, 7))),
])
ALL_CASES = list(CASES)
SEED_OVERRIDE = {"v_b9_fixed": 9101}          # 9000 + index: a layer-0 ReLU on a kink in episode order (float32 oracle 5e-4 off)
# the rows at the caps and the by-S pairs came later: they draw from 9200 on, so that the earlier rows kept their seeds
_LATER = [n for n in CASES if n.startswith("s_") or n in ("r_p1_s16", "r_p2_s18", "r_p2_s16", "r_p4_s18", "r_p4_s24", "r_p8_s26", "r_p8_s44",
                                                          "r_glob_s46", "a_lds_s40", "a_glob_s42")]
SEEDS = {n: 9000 + i for i, n in enumerate(n for n in CASES if n not in _LATER)}
SEEDS.update({n: 9200 + i for i, n in enumerate(_LATER)})
SEEDS.update(SEED_OVERRIDE)

# (inside, outside, the form entries the edge is about, the row arguments that differ): the two rows' FORM entries differ in exactly
# these entries and the rows in exactly these arguments.  The derived entries follow the forms and the shapes and are pinned per row.
EDGE_PAIRS = [
    ("q_fixed_s28", "q_lds_s30", {"adapt", "query", "fixed_last"}, {"K"}),                   # S = 28 against 29..32 (REF_SQ)
    ("q_fixed_n8", "q_fused_n9", {"query", "fixed_last", "P"}, {"N"}),                       # N = 8 against 9 (REF_NP; 16 head rows: P = 2 no longer fits)
    ("q_fixed", "q_fused_h128", {"query", "reverse", "P", "fixed_last"}, {"hid"}),           # h = [256, 64] against another network
    ("q_fixed", "q_fused_nograd", {"query", "reverse", "fixed_last"}, {"need_grad"}),
    ("q_fixed", "q_fused_w1off", {"query", "fixed_last"}, {"off"}),
    ("q_fixed", "q_fused_b1off", {"query", "fixed_last"}, {"off"}),
    ("q_fixed", "q_fused_b0off", {"query", "fixed_last"}, {"off"}),
    ("q_fixed", "q_fixed_drop", {"drop"}, {"dropout", "tanh"}),
    ("q_fused_small", "q_lds_t2", {"adapt", "query"}, {"T", "tanh"}),                        # T = 1 against 2
    ("q_fused_s32", "q_lds_s33", {"adapt", "query"}, {"N", "K"}),                            # S = 32 against 33 (QR)
    ("q_fused_h12", "q_lds_h10", {"adapt", "query", "reverse", "P"}, {"hid"}),               # h0 % 4 (the reverse sweep needs h0 % 4 == 0 too)
    ("q_fused_h256", "q_lds_h260", {"adapt", "query"}, {"hid"}),                             # h0 = 256 against 260
    ("q_fixed_s28", "q_lds_s32n8", {"adapt", "query", "fixed_last"}, {"N", "K", "Q"}),       # fused layout over the cap, plain layout under it
    ("a_lds_blocks6", "a_glob_layout", {"adapt"}, {"hid"}),                                  # adapt layout over the cap (h0 = 192 against 256)
    ("a_lds_s40", "a_glob_s42", {"adapt"}, {"K"}),                                           # the same cap from just outside (40196)
    ("a_lds_blocks8", "a_glob_blocks9", {"adapt"}, {"N", "K", "hid"}),                       # ceil(S/16) ceil(h0/64) = 8 against 9
    ("r_p1_h192", "r_p2_h256", {"P"}, {"hid"}),
    ("r_p1_s16", "r_p2_s18", {"P"}, {"K"}),
    ("r_p2_s16", "r_p4_s18", {"P"}, {"K"}),
    ("r_p4_s24", "r_p8_s26", {"P"}, {"K"}),
    ("r_p8_s44", "r_glob_s46", {"reverse", "P"}, {"K"}),                                     # no P <= 8 fits (P = 8: 40388)
    ("r_p8_h512", "r_glob_h576", {"reverse", "P"}, {"hid"}),
    ("r_lds_l4", "r_glob_l5", {"reverse", "P"}, {"hid"}),                                    # L = 4 against 5
    ("q_lds_t2", "q_lds_l1", {"reverse", "P"}, {"hid", "T", "tanh"}),                        # L = 2 against 1 (both with an adapt launch)
    ("r_lds_q256", "r_glob_q258", {"reverse", "P"}, {"Q"}),                                  # 8 against 9 query tiles
    ("b_two_2048", "b_one_2016", {"two_part"}, {"Q"}),                                       # B Qn = 2048 against fewer
    ("b_two_2048", "b_one_d64", {"two_part"}, {"D"}),                                        # refused by xpanel_bwd_two_part_ok (D % 128)
    ("q_lds_t2", "v_drop_t2", {"drop"}, {"dropout", "tanh"}),
    ("s_q511_s28", "s_qglob_s30", {"adapt", "query"}, {"K"}),                                # 511 units against more than 512, layout fits
    ("s_a512_h126", "s_aglob_h127", {"adapt"}, {"hid"}),                                     # 512 units against 516, same layout
]

# (row, the argument that grows, its granule, the cap it is next to): growing the dimension by one granule flips a form entry
CAP_NEIGHBOURS = [
    ("q_fixed_s28", "K", 1, "query layout (fused)"),            # S 28 -> 30: the fused layout leaves the cap
    ("a_lds_blocks6", "h0", 64, "adapt layout"),
    ("a_lds_s40", "K", 1, "adapt layout"),
    ("r_p1_h192", "h0", 64, "reverse layout"),
    ("r_p1_s16", "K", 1, "reverse layout"),
    ("r_p8_s44", "K", 1, "reverse layout"),
    ("r_p8_h512", "h0", 64, "reverse layout"),
    ("r_lds_q256", "Q", 1, "query tiles"),
    ("s_q511_s28", "K", 1, "query table units"),
    ("s_a512_h126", "h1", 1, "adapt table units"),
]

# (row, cap, the layout the row's plan REJECTED): its total lies in (LDS_CAP, LDS_MAX], so the named cap moved to 40960 changes the
# row's plan and fails tests/test_epi_forms_cpu.py
CAP_OUTSIDE = [
    ("q_lds_s30", "QLDS_CAP", lambda c, S: query_total(c["hid"], S, c["N"], fused=True)),
    ("q_lds_s32n8", "QLDS_CAP", lambda c, S: query_total(c["hid"], S, c["N"], fused=True)),
    ("a_glob_s42", "ALDS_CAP", lambda c, S: adapt_total(c["hid"], S, c["N"])),
    ("r_p2_s18", "RLDS_CAP", lambda c, S: reverse_total(c["hid"], S, c["N"], 1)),
    ("r_glob_s46", "RLDS_CAP", lambda c, S: reverse_total(c["hid"], S, c["N"], 8)),
]
# (row, cap, the table that does not fit although the form's layout does): the other side of the 512-unit cap
UNITS_OUTSIDE = [
    ("s_qglob_s30", "query table", lambda c, S: query_total(c["hid"], S, c["N"])),
    ("s_aglob_h127", "adapt table", lambda c, S: adapt_total(c["hid"], S, c["N"])),
]

# ---- knob-only forms: one child process per setting; the rows it changes and the entries it changes them to, form and derived
# (every other entry stays the row's own)
_G = dict(adapt=2, query=3, reverse=2, P=0, ql_total=0, al_total=0, rl_total=0, nu_adapt=0, nu_query=0, nu_rev_init=0, nu_rev_step=0)
KNOB_SETTINGS = [
    ({"FUMI_EPI_FUSE": "0"}, {"q_fixed": dict(adapt=1, query=2, fixed_last=2, ql_total=38648, al_total=38504, nu_adapt=84, nu_query=143, nu_fused=0),
                              "q_fused_small": dict(adapt=1, query=2, ql_total=6080, al_total=2960, nu_adapt=5, nu_query=12, nu_fused=0)}),
    ({"FUMI_EPI_FIXED": "0"}, {"q_fixed": dict(query=1, reverse=1, fixed_last=0, rl_total=34216),
                               "q_fixed_drop": dict(query=1, reverse=1, fixed_last=0, rl_total=34216)}),
    ({"FUMI_EPI_GLOBAL": "1"}, {"q_fixed": dict(adapt=2, query=3, reverse=2, P=0, fixed_last=0, ql_total=0, rl_total=0, nu_fused=0, nu_rev_init=0,
                                                nu_rev_step=0),
                                "q_lds_t2": _G, "q_lds_l3": _G, "m_first_t2": _G}),
    ({"FUMI_EPI_OVERLAP": "0"}, {"b_two_2048": dict(two_part=0, nsq=0, nss=0)}),
    ({"FUMI_EPI_OVERLAP": "2"}, {"b_one_2016": dict(two_part=1, nsq=32, nss=1), "b_one_d64": dict(), "q_lds_t2": dict()}),
    # the adapt layout and table are those of h0 / AP columns
    ({"FUMI_ADAPT_P": "2"}, {"a_glob_layout": dict(adapt=1, AP=2, al_total=24900, nu_adapt=40), "r_p2_h256": dict(AP=2, al_total=13572, nu_adapt=37),
                             "a_lds_blocks6": dict()}),                                                   # h0 = 192: no part of 64 k columns
    ({"FUMI_ADAPT_P": "4"}, {"a_glob_layout": dict(adapt=1, AP=4, al_total=16644, nu_adapt=24), "v_b9_p2": dict(AP=4, al_total=8388, nu_adapt=21)}),
    ({"FUMI_ADAPT_P": "8"}, {"a_glob_layout": dict(adapt=1, AP=4, al_total=16644, nu_adapt=24),          # h0 = 256: 8 halves to 4
                             "q_glob_h512": dict(adapt=1, AP=8, al_total=8388, nu_adapt=22)}),
    ({"FUMI_ADAPT_P": "16"}, {"r_p2_h256": dict(AP=4, al_total=8388, nu_adapt=21),                       # capped at 8, then halved
                              "r_p8_h512": dict(adapt=1, AP=8, al_total=16644, nu_adapt=24)}),
]


def setting_id(env):
    return " ".join(f"{k}={v}" for k, v in env.items())


def dims(c):
    return c["N"] * c["K"], c["N"] * c["Q"]


def macs(c):
    S, Qn = dims(c)
    h = [c["D"]] + c["hid"]
    deep = sum(h[i] * h[i + 1] for i in range(1, len(h) - 1)) + h[-1] * c["N"]
    return c["B"] * (S + Qn) * (c["D"] * c["hid"][0] + S * c["D"] + 3 * (c["T"] + 1) * deep)


def table_plan(name, changes=None):
    """The plan the table says row ``name`` reports (``changes``: the entries a knob setting moves, form and derived)."""
    p = dict(CASES[name]["plan"])
    p.update(changes or {})
    return p


def query_plan(name, **grow):
    """fumi_hip_epi_plan_query for the row (``grow``: K / Q / h0 replaced), under this process's knobs."""
    from fumi_amd import hip
    c = dict(CASES[name])
    hid = list(c["hid"])
    for i, k in enumerate(("h0", "h1")):
        if k in grow:
            hid[i] = grow.pop(k)
    c.update(grow)
    S, Qn = dims(c)
    off = c["off"]
    return hip.epi_plan_query(c["B"], c["N"], S, Qn, c["D"], hid, c["T"], need_grad=c["need_grad"], second_order=not c["first_order"],
                              dropout=c["dropout"] > 0, w_off=(int(off[1]),) if off and off[0] == "W" else (),
                              b_off=(int(off[1]),) if off and off[0] == "b" else ())


# ---- inputs, the oracle, the step ------------------------------------------------------------------------------------------------
def _case(name):
    """A row of this table by id, or a row of another table that shares these helpers (tests/hyper_forms.py), passed as the row itself
    with its seed under 'seed'."""
    return CASES[name] if isinstance(name, str) else name


def make_inputs(name):
    c = _case(name)
    seed = SEEDS[name] if isinstance(name, str) else c["seed"]
    ep = cg.make_episodes(seed, c["B"], c["N"], c["K"], c["Q"], c["D"], c["Dt"], blocked=bool(seed & 1))
    if c["entry"] == "fumi":
        theta, phi = cg.make_fumi_params(seed, c["D"], c["hid"], c["Dt"], c["Ht"])
        return ep, theta, phi
    return ep, cg.make_maml_params(seed, c["D"], c["hid"], c["N"]), None


def names(c):
    if c["entry"] == "fumi":
        return ([f"im_net.linear{i}.{k}" for i in range(len(c["hid"])) for k in ("weight", "bias")]
                + ["hyper_net.0.weight", "hyper_net.0.bias", "hyper_net.2.weight", "hyper_net.2.bias"])
    return [f"net.lin_{i}.{k}" for i in range(len(c["hid"])) for k in ("weight", "bias")] + ["net.lin_final.weight", "net.lin_final.bias"]


def oracle(name, inputs, dtype, text_grad=False):
    """oracle.fumi_ref on the CPU in ``dtype``: dict(logits, loss_b, preds, grads or None); ``text_grad`` (FuMI rows with gradients):
    also g_text_s [B,S,Dt], the gradient of the same loss with respect to the support text rows."""
    c = _case(name)
    ep, a, b = inputs
    f = lambda t: t.to(dtype)
    leaf = lambda ts: [t.clone().to(dtype).requires_grad_(True) for t in ts]
    if c["entry"] == "fumi":
        p = c["dropout"]
        drop = (lambda bb, call, layer, rows, width: dropout_mask(DROP_SEED, p, bb, call, layer, rows, width).to(dtype)) if p > 0 else None
        text = f(ep["text_s"]).clone().requires_grad_(True) if text_grad and c["need_grad"] else f(ep["text_s"])
        r = R.fumi_meta_step(leaf(a), leaf(b), text, f(ep["x_s"]), ep["y_s"], f(ep["x_q"]), ep["y_q"], c["N"], c["T"], cg.ALPHA,
                             c["tanh"], need_grad=c["need_grad"], dropout=drop, extra=[text] if text.requires_grad else None)
        grads = (r["g_theta"] + r["g_phi"]) if c["need_grad"] else None
        if text.requires_grad:
            return dict(logits=r["logits"], loss_b=r["loss_b"], preds=r["preds"], grads=grads, g_text_s=r["g_extra"][0])
    else:
        r = R.maml_meta_step(leaf(a), f(ep["x_s"]), ep["y_s"], f(ep["x_q"]), ep["y_q"], c["T"], cg.ALPHA, c["first_order"],
                             need_grad=c["need_grad"])
        grads = r["g_params"] if c["need_grad"] else None
    return dict(logits=r["logits"], loss_b=r["loss_b"], preds=r["preds"], grads=grads)


def run_step(name, inputs, dev, ws):
    """The row through hip.fumi_step_select / hip.maml_step: dict(logits, loss_b, preds, acc_b, grads or None) on the device.  The
    tensor named by the row's ``off`` is a view one float into a larger buffer."""
    from fumi_amd import hip
    c = CASES[name]
    ep, a, b = inputs
    g = lambda t: t.to(dev).contiguous()
    params = [g(t) for t in a]
    if c["off"]:
        i = 2 * int(c["off"][1]) + (0 if c["off"][0] == "W" else 1)
        buf = torch.zeros(params[i].numel() + 4, device=dev, dtype=torch.float32)
        view = buf[1:1 + params[i].numel()].view(params[i].shape)
        view.copy_(params[i])
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        params[i] = view
    if c["entry"] == "fumi":
        out = hip.fumi_step_select(ws, c["N"], g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]), g(ep["text_s"]), params,
                                   [g(t) for t in b], c["T"], cg.ALPHA, c["tanh"], need_grad=c["need_grad"], dropout_p=c["dropout"],
                                   seed=DROP_SEED)
        grads = (out["g_theta"] + out["g_phi"]) if c["need_grad"] else None
    else:
        out = hip.maml_step(ws, g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]), params, c["T"], cg.ALPHA, c["first_order"],
                            need_grad=c["need_grad"])
        grads = out["g_params"] if c["need_grad"] else None
    return dict(logits=out["logits"], loss_b=out["loss_b"], preds=out["preds"], acc_b=out["acc_b"], grads=grads)


def grad_floor(ref_grads):
    """The floor rule of _check_grads (tests/test_hip_parity.py) without a golden file."""
    return max(0.05 * max(float(r.abs().max()) for r in ref_grads), 1e-5)


def errors(name, got, ref):
    """{quantity: error of ``got`` against ``ref`` as a fraction of the reference's maximum} -- rel_to_max, gradients with the floor."""
    e = {"logits": rel_to_max(got["logits"].cpu(), ref["logits"]), "loss_b": rel_to_max(got["loss_b"].cpu(), ref["loss_b"])}
    if ref["grads"] is not None:
        fl = grad_floor(ref["grads"])
        for n, a, r in zip(names(_case(name)), got["grads"], ref["grads"]):
            e[n] = rel_to_max(a.cpu(), r, fl)
    return e


def project_bound(q):
    return LOGIT_TOL if q in ("logits", "loss_b") else GRAD_TOL


def margin_mask(ref_logits):
    """safe_margin_mask at MARGIN; a one-class row has no second logit and no tie."""
    from helpers import safe_margin_mask
    if ref_logits.shape[-1] < 2:
        return torch.ones(ref_logits.shape[:-1], dtype=torch.bool)
    return safe_margin_mask(ref_logits, MARGIN)


def child_env(env):
    e = dict(os.environ)
    for k in ("FUMI_EPI_FUSE", "FUMI_EPI_FIXED", "FUMI_EPI_GLOBAL", "FUMI_EPI_OVERLAP", "FUMI_ADAPT_P"):
        e.pop(k, None)
    e.update(env)
    return e
