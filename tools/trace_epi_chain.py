"""Per-phase wall-clock stamps of the per-episode chain (block 0 of the query and reverse kernels, csrc/episode.hip) at the bench
shape (BASELINE.json configs[1]: 32 episodes, 5-way 5-shot, h = [256, 64], T = 1), and which form of the two kernels ran: the
fixed-shape instances (default) or the run-time-shaped ones (FUMI_EPI_FIXED=0).
    python tools/trace_epi_chain.py            FUMI_EPI_FIXED=0 python tools/trace_epi_chain.py"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from fumi_amd import hip  # noqa: E402
from oracle import casegen as cg  # noqa: E402


def phases(t):
    n = int((t > 0).sum())
    return [(int(t[i + 1]) - int(t[i])) / 100.0 for i in range(n - 1)]      # s_memrealtime: 100 MHz


def main():
    dev = torch.device("cuda:0")
    ws = hip.Workspace.get(dev)
    B, N, K, Q, D, hid, Dt, Ht, T = 32, 5, 5, 32, 2048, [256, 64], 300, 256, 1
    ep = cg.make_episodes(1, B, N, K, Q, D, Dt)
    theta, phi = cg.make_fumi_params(1, D, hid, Dt, Ht)
    g = lambda t: t.to(dev).contiguous()
    args = (ws, N, g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]), g(ep["text_s"]), [g(t) for t in theta],
            [g(t) for t in phi], T, 0.01, False)
    for _ in range(3):
        hip.fumi_step_select(*args)
    tr = torch.zeros(256, dtype=torch.int64, device=dev)
    L = hip.lib()
    L.fumi_hip_set_trace_buffer(0, ctypes.c_void_p(tr.data_ptr()))
    hip.fumi_step_select(*args)
    torch.cuda.synchronize()
    L.fumi_hip_set_trace_buffer(0, None)
    fx = int(L.fumi_hip_epi_fixed_last())
    print("form: query", "fixed-shape" if fx & 1 else "run-time-shaped", "| reverse", "fixed-shape" if fx & 2 else "run-time-shaped",
          "(FUMI_EPI_FIXED=%s)" % os.environ.get("FUMI_EPI_FIXED", "1"))
    t = tr.cpu()
    # (192: the fixed-shape query kernel's last tile of episode 0, stamped when there is more than one tile)
    for name, lo in (("query_lds", 64), ("reverse_lds", 128), ("query_lds last tile", 192)):
        d = phases(t[lo:lo + 64])
        if not d:
            continue
        print(f"{name} phase durations (us):", [round(x, 2) for x in d], "total", round(sum(d), 1))


if __name__ == "__main__":
    main()
