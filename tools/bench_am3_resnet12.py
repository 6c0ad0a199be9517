"""Times AM3 with the bf16 ResNet-12 backbone (5-way 5-shot, 32 queries per class, 3x84x84 images, channels 64/160/320/640) straight
through the C ABI: resnet12_encode (tape kept) -> am3_step_dx -> resnet12_encode_bwd, synthetic images resident in HBM.  Runs the form
the workspace budget selects, then the recompute form forced through fumi_hip_resnet12_set_budget.
python tools/bench_am3_resnet12.py [B] [steps]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fumi_amd import hip  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N, K, Q, Cin, H, W, Dt, Ht, P = 5, 5, 32, 3, 84, 84, 768, 256, 64
CH = (64, 160, 320, 640)
dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
S, Qn = N * K, N * Q
x_s = torch.randn(B, S, Cin, H, W, device=dev, generator=g)
x_q = torch.randn(B, Qn, Cin, H, W, device=dev, generator=g)
y_s = torch.arange(N, device=dev).repeat_interleave(K).repeat(B, 1)
y_q = torch.arange(N, device=dev).repeat_interleave(Q).repeat(B, 1)
text = torch.randn(B, N, Dt, device=dev, generator=g)[:, y_s[0]]
F = CH[-1]
theta, ci = [], Cin
for c in CH:
    for (cin, k) in ((ci, 3), (c, 3), (c, 3), (ci, 1)):
        theta += [(torch.rand(c, cin, k, k, device=dev, generator=g) * 2 - 1) / (cin * k * k) ** 0.5, torch.ones(c, device=dev),
                  torch.zeros(c, device=dev)]
    ci = c
u = lambda *s, fan: (torch.rand(*s, device=dev, generator=g) * 2 - 1) / fan ** 0.5
w = [u(P, F, fan=F), u(P, fan=F), u(Ht, Dt, fan=Dt), u(Ht, fan=Dt), u(P, Ht, fan=Ht), u(P, fan=Ht), u(Ht, P, fan=P), u(Ht, fan=P),
     u(1, Ht, fan=Ht), u(1, fan=Ht)]
g_w = [torch.empty_like(t) for t in w]
g_theta = [torch.empty_like(t) for t in theta]

# convolution products per image (derived from the layer shapes, not measured): forward, input gradient (none into the image),
# weight gradient
fwd = dgrad = 0
hw, ci = H * W, Cin
for i, c in enumerate(CH):
    layers = ((ci, 9), (c, 9), (c, 9), (ci, 1))
    for j, (cin, taps) in enumerate(layers):
        f = 2 * hw * taps * cin * c
        fwd += f
        dgrad += 0 if (i == 0 and j in (0, 3)) else f
    hw, ci = (H >> (i + 1)) * (W >> (i + 1)), c
step_flops = B * (S + Qn) * (2 * fwd + dgrad)


def step():
    f_s, f_q = hip.resnet12_encode(ws_enc, x_s, x_q, theta, keep_tape=True)
    out = hip.am3_step(ws, f_s, y_s, f_q, y_q, text, w, N, None, g_w=g_w, dropout_p=0.25, seed=1, want_dx=True)
    hip.resnet12_encode_bwd(ws_enc, x_s, x_q, out["dx_s"], out["dx_q"], theta, g_theta=g_theta)
    return out


def run(label):
    t0 = time.perf_counter(); out = step(); torch.cuda.synchronize()
    taped, chunk, lanes = hip.resnet12_encode_plan()
    form = "taped" if taped else "recompute"
    print(f"[{label}] first call {time.perf_counter() - t0:.2f} s, form {form} (chunk {chunk}, lanes {lanes}), workspaces "
          f"{ws.bytes() / 2**30:.1f} + {ws_enc.bytes() / 2**30:.1f} GiB, loss {float(out['loss']):.4f}", flush=True)
    step(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    extra = "" if taped else " (+1 forward recomputed, not counted)"
    print(f"[{label}] AM3 + ResNet-12, B={B}, form {form}: {ms:.2f} ms/step, {B / ms * 1e3:.2f} episodes/s, "
          f"{step_flops / ms / 1e9:.1f} TFLOP/s in the conv products ({fwd / 1e9:.2f} GFLOP forward per image){extra}", flush=True)
    return [t.clone() for t in g_theta]


g_sel = run("budget")
hip.resnet12_set_budget(48)                        # the tape does not fit 48 GB (B = 32: ~80 GB): the recompute form
try:
    g_rc = run("recompute")
finally:
    hip.resnet12_set_budget(0)
print("forms bit-identical:", all(torch.equal(a, b) for a, b in zip(g_sel, g_rc)), flush=True)
