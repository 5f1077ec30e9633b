"""Times the attention-pooling kernels against what they replace and against a plain copy (needs a GPU).

    python tools/pool_probe.py [--json out.json]

Per shape (n, S, H): ops.attn_pool_fwd / ops.attn_pool_bwd in microseconds and achieved GB/s (bytes of x read once), and in the same
process at the same shape  ops.gemm_nt(x, W_kv [2H, H])  — the first step of the formulation being replaced — and a device-to-device
copy of x.  Device events around `iters` back-to-back calls after a warm-up; medians over `reps` windows.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(16, 2048, 1024), (8, 1024, 512)]


def timed(fn, iters=50, reps=5, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_probe: no GPU; timings are taken on the device only")
    from bioreason_amd import _lib, ops
    lib = _lib.get_lib()
    dev = torch.device("cuda:0")
    results = []
    for n, S, H in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(n, S, H, generator=g).to(torch.bfloat16).to(dev)
        mask = torch.ones(n, S, dtype=torch.uint8, device=dev)
        qt = (torch.randn(8, H, generator=g) * (2.0 / H ** 0.5)).to(dev)
        go = torch.randn(n, 8, H, generator=g).to(dev)
        wkv = (torch.randn(2 * H, H, generator=g) * 0.02).to(torch.bfloat16).to(dev)
        pooled, lse = ops.attn_pool_fwd(x, mask, qt)
        y = torch.empty_like(x)
        xb = x.numel() * 2
        nsplit = int(lib._dll.bra_attn_pool_nsplit(n, S, 0))
        rec = {"n": n, "S": S, "H": H, "x_MB": xb / 1e6, "workgroups": n * nsplit, "chunk_rows": -(-S // nsplit)}
        for name, fn, nbytes in [
            ("pool_fwd", lambda: ops.attn_pool_fwd(x, mask, qt), xb),
            ("pool_bwd", lambda: ops.attn_pool_bwd(x, mask, qt, pooled, lse, go), xb),
            ("gemm_kv", lambda: ops.gemm_nt(x.view(n * S, H), wkv), xb),
            ("copy_d2d", lambda: y.copy_(x), 2 * xb),
        ]:
            med, lo, hi = timed(fn)
            rec[name] = {"us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "GBps": round(nbytes / med / 1e3, 1)}
        rec["fwd_faster_than_gemm"] = rec["pool_fwd"]["us"] < rec["gemm_kv"]["us"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    if not all(r["fwd_faster_than_gemm"] for r in results):
        raise SystemExit("pool_probe: the fused forward is not faster than the K/V projection GEMM it replaces")


if __name__ == "__main__":
    main()
