"""GPU suite that holds the stand-alone fused optimizer launch (csrc/adam.hip: optim_kernel<RULE>, optim_fill, step_later) to the
float64 rule of tests/optim_ref.py at the edges of the launch: quad tails, tensor boundaries inside a workgroup and inside the
wrapped iterations of the grid-stride loop, one misaligned stream among aligned ones, 32 tensors, zero moments and 0 / (0 + eps).

Every stream of every tensor lives in its own buffer between GUARD sentinel words.  The bound per output stream is
optim_ref.bound(rule, stream) = 4 x the rounding a correct fp32 implementation shows against the rule (tests/test_optim_edges_cpu.py
measures that table and shows that the comparison notices a dropped tail element, a wrong tensor and a missing weight decay).
Everything goes through the ctypes wrappers (hip.adam_step / adamw_step / sgd_step and their deferred forms), not the torch classes.
The clipped and the folded forms hang from this kernel bit for bit (test_clip_grad_gpu.py, test_folded_step_gpu.py,
test_reduce_forms_gpu.py)."""
import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ws(dev):
    """A workspace of this suite's own: no other test's pending step or publication rides on these launches."""
    from fumi_amd import hip
    return hip.Workspace.get(dev, role="optim_edges")


class Placed:
    """One stream of one tensor on the device: GUARD sentinels, `offset` more of them, the values, GUARD sentinels."""

    def __init__(self, arr, offset, dev, fill=None):
        n = arr.size
        host = np.full(R.GUARD + offset + n + R.GUARD, R.SENTINEL, dtype=np.float32)
        self.lo, self.hi = R.GUARD + offset, R.GUARD + offset + n
        host[self.lo:self.hi] = arr.reshape(-1) if fill is None else fill
        self.buf = torch.from_numpy(host).to(dev)
        self.before = host
        self.view = self.buf[self.lo:self.hi].view(arr.shape)
        assert self.view.is_contiguous() and (self.view.data_ptr() % 16 != 0) == bool(offset % 4)

    def guards_intact(self, after=None):
        after = self.buf.cpu().numpy() if after is None else after
        return bool((after[:self.lo].view(np.int32) == R.SENTINEL.view(np.int32)).all()
                    and (after[self.hi:].view(np.int32) == R.SENTINEL.view(np.int32)).all())

    def unchanged(self):
        """every word of the buffer, guards and values, bit for bit (NaN included)"""
        return bool((self.buf.cpu().numpy().view(np.int32) == self.before.view(np.int32)).all())


def _place(name, rule, variant, dev, nan_first=True):
    """{stream: [Placed]} of the case (None for a stream the rule does not have); a first step's momentum buffers hold NaN."""
    x = R.case_inputs(name, rule, variant)
    out = {}
    for s in R.STREAMS:
        if x[s] is None:
            out[s] = None
            continue
        fill = np.float32(np.nan) if (s == "s0" and rule == "sgd_momentum_first" and nan_first) else None
        out[s] = [Placed(a, off.get(s, 0), dev, fill) for a, (_, off) in zip(x[s], R.CASES[name])]
    return out


def _views(pl, s):
    return None if pl[s] is None else [t.view for t in pl[s]]


def _launch(rule, pl, hyper, dev, deferred=False, ws=None):
    from fumi_amd import hip
    ws = ws or _ws(dev)
    h = hyper
    if rule in ("adam", "adamw"):
        args = hip.AdamArgs(_views(pl, "p"), _views(pl, "g"), _views(pl, "s0"), _views(pl, "s1"))
        scal = (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"])
        if deferred:
            (hip.adam_step_deferred if rule == "adam" else hip.adamw_step_deferred)(ws, args, *scal)
        else:
            (hip.adam_step if rule == "adam" else hip.adamw_step)(ws, args, *scal, dev)
    else:
        args = hip.SgdArgs(_views(pl, "p"), _views(pl, "g"), _views(pl, "s0"))
        mom = h["momentum"] if rule != "sgd" else 0.0
        if deferred:
            hip.sgd_step_deferred(ws, args, h["lr"], mom, h["wd"], rule == "sgd_momentum_first")
        else:
            hip.sgd_step(ws, args, h["lr"], mom, h["wd"], rule == "sgd_momentum_first", dev)


def _outputs(pl):
    return [t for s in R.OUT_STREAMS if pl[s] is not None for t in pl[s]]


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("hyper", range(len(R.HYPERS)))
@pytest.mark.parametrize("rule", R.RULES)
def test_one_step_matches_the_float64_rule(rule, hyper, name, variant, dev):
    h = R.cold_hyper(R.HYPERS[hyper], variant)
    pl = _place(name, rule, variant, dev)
    _launch(rule, pl, h, dev)
    torch.cuda.synchronize()
    ref = R.reference(name, rule, R.HYPERS[hyper], variant)
    worst = {}
    failures = []
    for k, s in enumerate(R.OUT_STREAMS):
        if pl[s] is None:
            continue
        for i, t in enumerate(pl[s]):
            after = t.buf.cpu().numpy()
            if not t.guards_intact(after):
                failures.append(f"{s}[{i}]: a guard word was written")
            got = after[t.lo:t.hi].reshape(ref[i][k].shape)
            if not np.isfinite(got).all():
                failures.append(f"{s}[{i}]: not finite")
                continue
            err = R.rel_to_max(got, ref[i][k])
            worst[s] = max(worst.get(s, 0.0), err)
            if not err <= R.bound(rule, s):
                failures.append(f"{s}[{i}]: rel-to-max {err:.3e} > {R.bound(rule, s):.3e}")
    print(f"{rule} hyper {hyper} {name} {variant}: " + ", ".join(f"{s} {e:.3e} (bound {R.bound(rule, s):.3e})" for s, e in worst.items()))
    for i, t in enumerate(pl["g"]):
        if not t.unchanged():
            failures.append(f"g[{i}]: the gradient buffer was written")
    assert not failures, failures


@pytest.mark.parametrize("rule", R.RULES)
def test_equal_inputs_give_equal_bits(rule, dev):
    h = R.HYPERS[0]
    a = _place("grid_stride_wraps", rule, "warm", dev)
    b = _place("grid_stride_wraps", rule, "warm", dev)
    _launch(rule, a, h, dev)
    _launch(rule, b, h, dev)
    torch.cuda.synchronize()
    for x, y in zip(_outputs(a), _outputs(b)):
        assert torch.equal(x.buf, y.buf)


@pytest.mark.parametrize("name", ["boundaries_in_one_workgroup", "all_misaligned"])
@pytest.mark.parametrize("rule", R.RULES)
def test_deferred_then_flushed_is_the_same_launch(rule, name, dev):
    """No meta-step between the deferred call and adam_flush: the path a step takes when it cannot fold the update."""
    from fumi_amd import hip
    ws = _ws(dev)
    h = R.HYPERS[0]
    a = _place(name, rule, "warm", dev)
    b = _place(name, rule, "warm", dev)
    _launch(rule, a, h, dev, deferred=True)
    torch.cuda.synchronize()
    assert all(t.unchanged() for s in R.STREAMS if a[s] is not None for t in a[s])      # nothing ran yet
    assert hip.adam_flush(ws, dev) is True
    _launch(rule, b, h, dev)
    torch.cuda.synchronize()
    for x, y in zip(_outputs(a), _outputs(b)):
        assert torch.equal(x.buf, y.buf)
    assert all(t.unchanged() for t in a["g"])
    keep = [t.buf.clone() for t in _outputs(a)]
    assert hip.adam_flush(ws, dev) is False
    torch.cuda.synchronize()
    for x, k in zip(_outputs(a), keep):
        assert torch.equal(x.buf, k)


def _many(n, rule, dev):
    x = R.case_inputs("thirty_two", rule)
    pick = lambda s: None if x[s] is None else [Placed(x[s][i % R.MAXT], 0, dev) for i in range(n)]
    return {s: pick(s) for s in R.STREAMS}


def _untouched(pl):
    return all(t.unchanged() for s in R.STREAMS if pl[s] is not None for t in pl[s])


def test_refusals_leave_every_buffer_alone(dev):
    from fumi_amd import hip
    ws = _ws(dev)
    h = R.HYPERS[0]
    assert hip.adam_flush(ws, dev) is False

    def refused(rule, pl, hyper, deferred, code):
        with pytest.raises(hip.FumiHipError, match=code):
            _launch(rule, pl, hyper, dev, deferred=deferred)
        if deferred:
            assert hip.adam_flush(ws, dev) is False                          # a refused call leaves nothing pending
        torch.cuda.synchronize()
        assert _untouched(pl), (rule, deferred)

    for rule in ("adam", "adamw", "sgd_momentum", "sgd"):
        refused(rule, _many(R.MAXT + 1, rule, dev), h, False, r"\(-4\)")      # FUMI_ENOTSUP
        refused(rule, _many(R.MAX_FOLD + 1, rule, dev), h, True, r"\(-4\)")
    for rule in ("adam", "adamw"):
        for deferred in (False, True):
            refused(rule, _place("quad_tails", rule, "warm", dev), dict(h, step=0), deferred, r"\(-1\)")       # FUMI_EINVAL
    # a tensor of no elements with a NULL pointer (what torch gives it), in each stream in turn
    empty = torch.empty(0, dtype=torch.float32, device=dev)
    assert empty.data_ptr() == 0
    for rule in ("adam", "sgd_momentum", "sgd"):
        for s in R.STREAMS:
            for deferred in (False, True):
                pl = _place("quad_tails", rule, "warm", dev)
                if pl[s] is None:
                    continue
                full = {k: _views(pl, k) for k in R.STREAMS}
                full[s] = [full[s][0], empty, full[s][2]]
                with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):
                    if rule == "adam":
                        args = hip.AdamArgs(full["p"], full["g"], full["s0"], full["s1"])
                        args.numel[1] = 0
                        scal = (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"])
                        hip.adam_step_deferred(ws, args, *scal) if deferred else hip.adam_step(ws, args, *scal, dev)
                    else:
                        args = hip.SgdArgs(full["p"], full["g"], full["s0"])
                        args.numel[1] = 0
                        mom = h["momentum"] if rule != "sgd" else 0.0
                        (hip.sgd_step_deferred(ws, args, h["lr"], mom, h["wd"], False) if deferred
                         else hip.sgd_step(ws, args, h["lr"], mom, h["wd"], False, dev))
                assert hip.adam_flush(ws, dev) is False
                torch.cuda.synchronize()
                assert _untouched(pl), (rule, s, deferred)
    # buffers with momentum == 0, and none with momentum != 0
    pl = _place("quad_tails", "sgd_momentum", "warm", dev)
    with_buf = hip.SgdArgs(_views(pl, "p"), _views(pl, "g"), _views(pl, "s0"))
    without = hip.SgdArgs(_views(pl, "p"), _views(pl, "g"), None)
    for args, mom in ((with_buf, 0.0), (without, 0.9)):
        with pytest.raises(hip.FumiHipError):
            hip.sgd_step(ws, args, h["lr"], mom, h["wd"], False, dev)
        with pytest.raises(hip.FumiHipError):
            hip.sgd_step_deferred(ws, args, h["lr"], mom, h["wd"], False)
    assert hip.adam_flush(ws, dev) is False
    torch.cuda.synchronize()
    assert _untouched(pl)


def test_a_refused_deferred_call_leaves_a_pending_step_as_it_was(dev):
    """An accepted deferred step, then one that is refused at its second tensor (a NULL pointer): the flush launches the first step
    whole -- no tensor of the refused call -- with the bits of the immediate entry point."""
    from fumi_amd import hip
    ws = _ws(dev)
    h = R.HYPERS[0]
    a = _place("boundaries_in_one_workgroup", "adam", "warm", dev)
    b = _place("boundaries_in_one_workgroup", "adam", "warm", dev)
    other = _place("quad_tails", "adam", "warm", dev)
    _launch("adam", a, h, dev, deferred=True)
    empty = torch.empty(0, dtype=torch.float32, device=dev)
    grads = _views(other, "g")
    args = hip.AdamArgs(_views(other, "p"), [grads[0], empty, grads[2]], _views(other, "s0"), _views(other, "s1"))
    with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):
        hip.adam_step_deferred(ws, args, 0.5, h["b1"], h["b2"], h["eps"], 0.0, 7)
    assert hip.adam_flush(ws, dev) is True
    _launch("adam", b, h, dev)
    torch.cuda.synchronize()
    assert _untouched(other)
    for x, y in zip(_outputs(a), _outputs(b)):
        assert torch.equal(x.buf, y.buf)
    assert hip.adam_flush(ws, dev) is False
