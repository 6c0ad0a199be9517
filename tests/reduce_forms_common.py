"""Shared by test_reduce_forms_cpu.py and test_reduce_forms_gpu.py (not a test module): the documented order of the slab reductions
(csrc/gemm.hip: slab_sum) restated in float32 numpy, the segment cases of both suites and their seeded inputs, and the worker that
runs the optimizer rules through the folded last launch of the FuMI step (also the child process of the FUMI_ADAM_FUSE=0 run)."""
import os
import sys
import zlib

import numpy as np

SLABS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 40, 70]          # one batch, a batch edge (16 float4 / 32 scalars), several batches
COUNTS = [1, 3, 4, 5, 252, 255, 256, 257, 1024, 1028]            # below / at / above a 256-thread workgroup; multiples of 4 or not
GUARD = 64                                                       # words behind every destination that must stay untouched
SENTINEL = np.float32(-7.5e7)


def two_chains(slabs, scale):
    """slabs [ns, n] float32 -> scale * (sum of the even slabs + sum of the odd slabs), each chain in increasing slab index from
    +0.0, every operation rounded to float32."""
    a0 = np.zeros(slabs.shape[1], np.float32)
    a1 = np.zeros(slabs.shape[1], np.float32)
    for t in range(slabs.shape[0]):
        if t % 2 == 0:
            a0 = a0 + slabs[t]
        else:
            a1 = a1 + slabs[t]
    return np.float32(scale) * (a0 + a1)


def one_chain(slabs, scale):
    s = np.zeros(slabs.shape[1], np.float32)
    for t in range(slabs.shape[0]):
        s = s + slabs[t]
    return np.float32(scale) * s


class Case:
    """One segment: ns slabs of `count` floats, `stride` floats apart; src_off / dst_off: the tensors start one float off a 16-byte
    boundary (the one-float-per-thread path)."""
    def __init__(self, ns, count, stride=None, src_off=0, dst_off=0):
        self.ns, self.count, self.stride = ns, count, count if stride is None else stride
        self.src_off, self.dst_off = src_off, dst_off

    @property
    def name(self):
        return f"ns{self.ns}_n{self.count}_st{self.stride}_so{self.src_off}_do{self.dst_off}"

    @property
    def vec(self):
        """What ReduceSegs::add decides for 16-byte aligned base allocations."""
        return self.count % 4 == 0 and self.stride % 4 == 0 and self.src_off == 0 and self.dst_off == 0

    def slabs(self):
        """[ns, stride] float32 (the first `count` of every row are summed): magnitudes 1e-3 .. 1e3, both signs, seeded by name.
        With four slabs or more the draw is repeated (next seed) until the two-chain order and a single chain differ in at least
        one summed column -- a handful of columns can agree by chance.  So the guarantee that every such input can tell the orders
        apart lives HERE, in the generator; test_reduce_forms_cpu.py re-verifies it on the arrays this returns (and at the other
        scale), it does not establish it."""
        for salt in range(64):
            g = np.random.default_rng(zlib.crc32(self.name.encode()) + salt)
            mag = 10.0 ** g.uniform(-3.0, 3.0, (self.ns, self.stride))
            x = (mag * g.choice([-1.0, 1.0], (self.ns, self.stride))).astype(np.float32)
            s = x[:, :self.count]
            if self.ns < 4 or (two_chains(s, 1.0).view(np.int32) != one_chain(s, 1.0).view(np.int32)).any():
                return x
        raise AssertionError(f"{self.name}: no draw tells the two orders apart")


def grid_cases(ns):
    return [Case(ns, n) for n in COUNTS]


def odd_cases():
    """Offsets by one float, strides larger than the count."""
    out = []
    for ns in (3, 16, 33):
        out += [Case(ns, 256, src_off=1), Case(ns, 256, dst_off=1), Case(ns, 1028, src_off=1, dst_off=1), Case(ns, 5, src_off=1),
                Case(ns, 256, stride=260), Case(ns, 1024, stride=2048), Case(ns, 255, stride=259), Case(ns, 4, stride=8),
                Case(ns, 1, stride=7)]
    return out


def mixed24():
    """One launch of 24 segments mixing all of the above."""
    picks = [(1, 1), (2, 3), (3, 4), (4, 5), (5, 252), (15, 255), (16, 256), (17, 257), (31, 1024), (32, 1028), (33, 256), (40, 4),
             (70, 1028), (32, 1), (16, 1024), (70, 5)]
    out = [Case(ns, n) for ns, n in picks]
    out += [Case(16, 256, src_off=1), Case(32, 1028, dst_off=1), Case(33, 255, stride=259), Case(17, 1024, stride=2048),
            Case(32, 5, src_off=1, dst_off=1), Case(40, 256, stride=260), Case(2, 4, stride=8), Case(70, 1, stride=7)]
    assert len(out) == 24
    return out


# ---- the folded launch through the step path ----------------------------------------------------------------------------------
RULES = ["adam", "adamw", "sgd_momentum", "sgd"]


def run_rules():
    """Three training steps of FUMI.evaluate per rule at B = 2, N = 5, S = 5, Qn = 10, D = 256, h = [256, 64], T = 1 with a deferred
    optimizer step.  Returns {rule: dict(tensors=[grads, params, state...] on the CPU, stats=[(loss, acc)...], folded=[...])}."""
    from types import SimpleNamespace
    import torch
    from fumi_amd import optim
    from fumi_amd.models.fumi import FUMI
    from oracle import casegen as cg
    dev = torch.device("cuda:0")
    c = dict(B=2, N=5, K=1, Q=2, D=256, hid=[256, 64], Dt=48, Ht=64)
    out = {}
    for rule in RULES:
        torch.manual_seed(5)
        m = FUMI(n_way=c["N"], im_emb_dim=c["D"], im_hid_dim=c["hid"], text_encoder="BERT", text_emb_dim=c["Dt"], text_hid_dim=c["Ht"],
                 dropout_rate=0.0, norm_hypernet=True).to(dev)
        if rule == "adam":
            opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
        elif rule == "adamw":
            opt = optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
        elif rule == "sgd_momentum":
            opt = optim.SGD(m.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4)
        else:
            opt = optim.SGD(m.parameters(), lr=1e-2, weight_decay=5e-4)
        folded = []
        fin = opt.finish_deferred
        opt.finish_deferred = lambda device, fin=fin, folded=folded: folded.append(not fin(device))
        args = SimpleNamespace(device=dev, num_train_adapt_steps=1, num_test_adapt_steps=1, step_size=0.05, first_order=False,
                               num_ways=c["N"], batch_size=c["B"])
        stats = []
        for i in range(3):
            ep = cg.make_episodes(200 + i, c["B"], c["N"], c["K"], c["Q"], c["D"], c["Dt"])
            loss, acc, _, _ = m.evaluate(args, cg.to_batch(ep), opt, "train")
            stats.append((float(loss), float(acc)))
        torch.cuda.synchronize()
        st = opt.state_dict()["state"]
        state = [torch.as_tensor(st[i][k]).detach().cpu().clone() for i in sorted(st) for k in sorted(st[i])]
        tensors = [p.grad.detach().cpu().clone() for p in m.parameters()] + [p.detach().cpu().clone() for p in m.parameters()] + state
        out[rule] = dict(tensors=tensors, stats=stats, folded=folded)
    return out


if __name__ == "__main__":                     # the child process: python reduce_forms_common.py OUT.pt  (FUMI_ADAM_FUSE set by the parent)
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    torch.save(run_rules(), sys.argv[1])
