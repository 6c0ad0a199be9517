"""Float64 statement of one step of the fused optimizer launch (csrc/adam.hip: optim_kernel<RULE>, OPTIM_STEP_BODY; element
functions: csrc/common.h) and the tensor lists the edge tests run on (not a test module; no GPU).

    adam                gr = g + wd p ; m += (1 - b1)(gr - m) ; v = b2 v + (1 - b2) gr gr ; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
    adamw               p *= 1 - lr wd ; the same moments and update on the raw g
    sgd_momentum_first  gr = g + wd p ; buf = gr (written, never read) ; p -= lr buf
    sgd_momentum        gr = g + wd p ; buf = mu buf + gr ; p -= lr buf
    sgd                 gr = g + wd p ; p -= lr gr
    bc1 = 1 - b1^step, bc2 = 1 - b2^step, folded on the host as adam_coef / sgd_coef fold them.

EVERY SCALAR IS TAKEN AS THE ENTRY POINT RECEIVES IT (`abi`): rounded to the C parameter's type first -- float for lr, eps,
weight_decay, momentum and Adam's betas, double for AdamW's betas -- and only then used in float64.

Deviation from torch.optim.Adam, on record: fumi_hip_adam_step takes beta1 and beta2 as floats and adam_update1 forms 1.f - b2 in
fp32 (exact: Sterbenz), so the Adam launch uses b2 = fp32(0.999) = 0.99900001287... and 1 - b2 = 0.00099998712..., where torch, fed
the Python doubles, uses 0.999 and 0.001.  Each increment (1 - b2) gr^2 of exp_avg_sq is therefore 1.2875e-5 smaller, relatively,
than torch's (`ADAM_BETA2_DEVIATION`; tests/test_optim_edges_cpu.py measures its effect on exp_avg_sq after one step).  That is a
property of the ABI's parameter types, not of the kernel; `rule64` follows the ABI, and the AdamW entry points take doubles.

`rule32` restates the same step in np.float32, one rounded operation at a time in the order the element functions state, with the
coefficients rounded where OptCoef holds floats.  It is no second oracle: it measures the rounding a correct fp32 implementation
shows against `rule64`, recorded in `E32`; the bound the device is held to is `bound(rule, stream)` = 4 * max(E32, 2^-24)."""
import functools
import math

import numpy as np

import clip_ref

RULES = ["adam", "adamw", "sgd_momentum_first", "sgd_momentum", "sgd"]
NSTATE = {"adam": 2, "adamw": 2, "sgd_momentum_first": 1, "sgd_momentum": 1, "sgd": 0}
STREAMS = ("p", "g", "s0", "s1")
OUT_STREAMS = ("p", "s0", "s1")
MAXT = 32                              # csrc/adam.hip: tensors of one launch
MAX_FOLD = 24                          # csrc/adam.hip: tensors of a deferred step
OPT_CAP = 2048                         # csrc/adam.hip: optim_launch caps the grid at 2048 workgroups of 256 threads, one float4 each
WRAP = OPT_CAP * 1024                  # elements of one sweep of its grid-stride loop
GUARD = 64                             # sentinel words in front of and behind every stream of every tensor
SENTINEL = np.float32(-7.5e7)

HYPERS = [dict(lr=3e-3, wd=5e-4, step=3, b1=0.9, b2=0.999, eps=1e-8, momentum=0.9),
          dict(lr=1e-3, wd=0.0, step=1, b1=0.9, b2=0.999, eps=1e-8, momentum=0.9)]

_MIS = [(37,), (8, 5), (130,)]


def _one(stream):
    off = {stream: 1}
    return [(_MIS[0], off), (_MIS[1], {}), (_MIS[2], off)]


# name -> list of (shape, {stream: offset}): offset 1 = a view starting one float into a larger buffer (no 16-byte access may
# touch it); a stream the rule does not have is ignored
CASES = {
    "smallest": [((1,), {})],
    "quad_tails": [((3,), {}), ((4,), {}), ((5,), {})],
    "boundaries_in_one_workgroup": [(s, {}) for s, _ in clip_ref.CASES["boundaries_in_one_workgroup"]],
    "one_stream_misaligned_p": _one("p"),
    "one_stream_misaligned_g": _one("g"),
    "one_stream_misaligned_s0": _one("s0"),
    "one_stream_misaligned_s1": _one("s1"),
    "all_misaligned": [(s, {k: 1 for k in STREAMS}) for s in _MIS],
    "thirty_two": [((5,), {})] * MAXT,
    # the boundary search runs inside the wrapped iterations, and the last workgroup handles a scalar tail
    "grid_stride_wraps": [((WRAP + 5,), {}), ((6,), {}), ((1025,), {})],
    "wrap_then_misaligned": [((WRAP + 1,), {}), ((130,), {"p": 1})],
}
VARIANTS = ("warm", "cold")


def abi(rule, hyper):
    """The hyper-parameters as the rule's entry point receives them (Python floats holding the rounded values)."""
    f = lambda x: float(np.float32(x))
    h = dict(lr=f(hyper["lr"]), eps=f(hyper["eps"]), wd=f(hyper["wd"]), momentum=f(hyper["momentum"]), step=int(hyper["step"]))
    h["b1"], h["b2"] = (f(hyper["b1"]), f(hyper["b2"])) if rule == "adam" else (float(hyper["b1"]), float(hyper["b2"]))
    return h


ADAM_BETA2_DEVIATION = 1.0 - (1.0 - float(np.float32(0.999))) / (1.0 - 0.999)       # 1.2875e-5


def coef64(rule, hyper):
    """adam_coef / sgd_coef in float64 on the ABI's scalars."""
    h = abi(rule, hyper)
    if rule in ("adam", "adamw"):
        bc1, bc2 = 1.0 - h["b1"] ** h["step"], 1.0 - h["b2"] ** h["step"]
        return dict(lr=h["lr"] / bc1, a=1.0 / math.sqrt(bc2), b1=h["b1"], b2=h["b2"], omb1=1.0 - h["b1"], omb2=1.0 - h["b2"],
                    eps=h["eps"], wd=1.0 - h["lr"] * h["wd"] if rule == "adamw" else h["wd"])
    return dict(lr=h["lr"], a=h["momentum"], wd=h["wd"])


def _step(rule, p, g, s0, s1, c, one):
    """The element functions of common.h, operation by operation; the arrays' dtype decides where each one rounds."""
    if rule in ("adam", "adamw"):
        if rule == "adam":
            gr = g + c["wd"] * p
            omb1, omb2 = one - c["b1"], one - c["b2"]                          # formed in the kernel's precision (exact in fp32)
        else:
            p = p * c["wd"]                                                    # decay = 1 - lr wd
            gr = g
            omb1, omb2 = c["omb1"], c["omb2"]                                  # folded on the host in double
        m = s0 + omb1 * (gr - s0)
        v = c["b2"] * s1 + omb2 * gr * gr
        p = p - c["lr"] * (m / (np.sqrt(v) * c["a"] + c["eps"]))
        return p, m, v
    gr = g + c["wd"] * p
    if rule == "sgd":
        return p - c["lr"] * gr, None, None
    buf = gr if rule == "sgd_momentum_first" else c["a"] * s0 + gr
    return p - c["lr"] * buf, buf, None


def _as(x, dt):
    return None if x is None else np.asarray(x, dtype=dt)


def rule64(rule, p, g, s0, s1, hyper):
    """One step in float64 -> the new (p, s0, s1); a stream the rule does not have is None."""
    c = coef64(rule, hyper)
    f = np.float64
    return _step(rule, _as(p, f), _as(g, f), _as(s0, f) if NSTATE[rule] >= 1 else None, _as(s1, f) if NSTATE[rule] >= 2 else None, c, f(1))


def rule32(rule, p, g, s0, s1, hyper):
    """The same step as a correct fp32 implementation rounds it (see the module docstring)."""
    c = {k: np.float32(v) for k, v in coef64(rule, hyper).items()}
    f = np.float32
    return _step(rule, _as(p, f), _as(g, f), _as(s0, f) if NSTATE[rule] >= 1 else None, _as(s1, f) if NSTATE[rule] >= 2 else None, c, f(1))


def rel_to_max(a, b):
    """|a - b|_inf / |b|_inf in float64 (tests/helpers.py: rel_to_max, in numpy and without its 1e-5 floor, which would hide errors
    in the small-scale tensors here; a reference that is all zero admits only zero)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def cold_hyper(hyper, variant):
    return dict(hyper, step=1) if variant == "cold" else hyper


@functools.lru_cache(maxsize=None)
def case_inputs(name, rule, variant="warm"):
    """{stream: [float32 arrays]} of the case for `rule`: seeded per case and stream as clip_ref.case_arrays seeds, the scale cycling
    over 1e-2 .. 1e2 by tensor index; exp_avg_sq is a square.  The last element of every gradient is at least the tensor's scale in
    magnitude, so that leaving a tensor's tail alone moves every rule's outputs visibly.  cold: zero moments (the hyper-parameters'
    step becomes 1: `cold_hyper`) and one gradient element per tensor exactly 0, so 0 / (0 + eps) occurs.  Shared and read only."""
    idx = sorted(CASES).index(name)

    def draw(seed):
        rng = np.random.default_rng([seed, idx])
        return [(rng.standard_normal(shape).astype(np.float32) * np.float32(10.0 ** ((i % 5) - 2))).astype(np.float32)
                for i, (shape, _) in enumerate(CASES[name])]
    out = {"p": draw(1), "g": draw(0), "s0": None, "s1": None}
    for i, g in enumerate(out["g"]):
        scale = np.float32(10.0 ** ((i % 5) - 2))
        if abs(g.flat[-1]) < scale:
            g.flat[-1] = np.copysign(scale, g.flat[-1])
        if variant == "cold":
            g.flat[(g.size - 1) // 2] = 0.0
    if rule in ("adam", "adamw"):
        out["s0"] = [(a * np.float32(0.1)).astype(np.float32) for a in draw(2)]
        out["s1"] = [(a * a).astype(np.float32) for a in draw(3)]
    elif NSTATE[rule] == 1:
        out["s0"] = draw(2)
    if variant == "cold":
        for k in ("s0", "s1"):
            if out[k] is not None:
                out[k] = [np.zeros_like(a) for a in out[k]]
    for k in STREAMS:
        for a in out[k] or []:
            a.setflags(write=False)
    return out


def reference(name, rule, hyper, variant="warm"):
    """[(p, s0, s1) in float64 per tensor] of one step on the case's inputs."""
    x = case_inputs(name, rule, variant)
    h = cold_hyper(hyper, variant)
    n = len(x["p"])
    return [rule64(rule, x["p"][i], x["g"][i], x["s0"][i] if x["s0"] else None, x["s1"][i] if x["s1"] else None, h) for i in range(n)]


def measure_e32(rule, names=None):
    """{stream: max over cases, variants, hyper-parameter sets and tensors of rel_to_max(rule32, rule64)}."""
    worst = {k: 0.0 for k in OUT_STREAMS[:1 + NSTATE[rule]]}
    for name in names or sorted(CASES):
        for variant in VARIANTS:
            x = case_inputs(name, rule, variant)
            for hyper in HYPERS:
                h = cold_hyper(hyper, variant)
                for i in range(len(x["p"])):
                    args = (x["p"][i], x["g"][i], x["s0"][i] if x["s0"] else None, x["s1"][i] if x["s1"] else None, h)
                    for k, lo, hi in zip(OUT_STREAMS, rule32(rule, *args), rule64(rule, *args)):
                        if hi is not None:
                            worst[k] = max(worst[k], rel_to_max(lo, hi))
    return worst


# measured by tests/test_optim_edges_cpu.py (which fails when this table is below what it measures, or more than twice above it)
E32 = {
    "adam": {"p": 6.20e-07, "s0": 1.21e-07, "s1": 1.43e-07},
    "adamw": {"p": 1.28e-07, "s0": 1.04e-07, "s1": 1.25e-07},
    "sgd_momentum_first": {"p": 5.59e-08, "s0": 5.02e-08},
    "sgd_momentum": {"p": 5.72e-08, "s0": 8.68e-08},
    "sgd": {"p": 5.59e-08},
}


def bound(rule, stream):
    """What the device may differ from rule64 by, rel-to-max: 4 x the measured rounding of a correct fp32 implementation, floored at
    the rounding of the final store alone.  The 4 covers a divide or square root good to an ulp or two and one reassociation; a wrong
    coefficient (smallest on record here: 1.3e-5) has no room in it."""
    return 4.0 * max(E32[rule][stream], 2.0 ** -24)
