"""Cost of the policy entropy in the fused lm_head (HIP events, warm-up, median of N):

  kernels   lmhead_logprob vs lmhead_logprob_entropy, lmhead_dlogits without / with ecoef, at M x 151 936 x 2048 (M = B C of the step;
            the full-row policy pass feeds the lm_head the same B C kept rows).  Each pair is timed A, B, A so that the first variant's
            own run-to-run spread stands beside the delta.
  step      GRPOStepRunner at bench.py's configuration (its model, batch and config), ms per step with the switches off, with
            log_entropy, and with entropy_coef = 0.01; prints the `entropy` metric of each step (a random-init model: near ln V).

    python tools/entropy_probe.py kernels [--m 2048 4096] [--iters 20]
    python tools/entropy_probe.py step [--steps 4] [--warmup 2]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bioreason_amd import ops  # noqa: E402


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def kernels(args):
    dev = torch.device("cuda:0")
    V, K = 151936, 2048
    g = torch.Generator().manual_seed(1)
    e = (torch.randn(V, K, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    for M in args.m:
        h = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
        tgt = torch.randint(0, V, (M,), generator=g).to(torch.int32).to(dev)
        coef = torch.randn(M, generator=g).to(dev)
        ecoef = torch.randn(M, generator=g).to(dev)
        logp, lse, ent = ops.lmhead_logprob_entropy(h, e, tgt)
        fwd0 = lambda: ops.lmhead_logprob(h, e, tgt)
        fwd1 = lambda: ops.lmhead_logprob_entropy(h, e, tgt)
        bwd0 = lambda: ops.lmhead_dlogits(h, e, tgt, lse, coef)
        bwd1 = lambda: ops.lmhead_dlogits(h, e, tgt, lse, coef, ent, ecoef)
        res = {"M": M, "V": V, "K": K, "entropy_mean": round(ent.mean().item(), 4), "ln_V": round(math.log(V), 4)}
        for name, f0, f1 in (("forward", fwd0, fwd1), ("dlogits", bwd0, bwd1)):
            a1, b, a2 = _time(f0, args.iters), _time(f1, args.iters), _time(f0, args.iters)
            res[name] = {"off_us": [round(a1, 1), round(a2, 1)], "on_us": round(b, 1), "delta_us": round(b - 0.5 * (a1 + a2), 1),
                         "off_spread_us": round(abs(a1 - a2), 1)}
        print(json.dumps(res), flush=True)


def step(args):
    import bench
    from bioreason_amd import trainer
    dev = torch.device("cuda:0")
    dims = bench.Dims(False)
    ns = argparse.Namespace(no_graph=False, no_shared_decode=False)
    for label, log, coef in (("off", False, 0.0), ("log_entropy", True, 0.0), ("entropy_coef=0.01", True, 0.01), ("off again", False, 0.0)):
        model = bench.build_model(dims, dev, 0.0)
        # the two fields go in through the config bench.make_grpo_leg builds (it imports GRPOConfig from bioreason_amd.trainer when called)
        real_cfg = trainer.GRPOConfig
        trainer.GRPOConfig = lambda **kw: real_cfg(**kw, log_entropy=log, entropy_coef=coef)
        try:
            runner, do_step, _ = bench.make_grpo_leg(model, dims, 1, dims.c, 0, dev, ns, None, args.steps + args.warmup)
        finally:
            trainer.GRPOConfig = real_cfg
        assert runner.cfg.log_entropy == log and runner.cfg.entropy_coef == coef and runner.with_entropy == log
        ent = []
        for i in range(args.warmup):
            out = do_step(i)
            ent.append(out["metrics_t"][-1].item() if log else None)
        torch.cuda.synchronize()
        ts = []
        for i in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = do_step(args.warmup + i)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
            ent.append(out["metrics_t"][-1].item() if log else None)
        print(json.dumps({"switches": label, "ms_per_step_median": round(statistics.median(ts), 2), "ms_per_step": [round(t, 2) for t in ts],
                          "entropy": [None if v is None else round(v, 4) for v in ent], "ln_V": round(math.log(model.text_model.engine.V), 4)}),
              flush=True)
        del runner, model, do_step
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step"])
    ap.add_argument("--m", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    kernels(a) if a.what == "kernels" else step(a)
