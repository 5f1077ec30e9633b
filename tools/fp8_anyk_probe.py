#!/usr/bin/env python3
"""Token loop and prompt pass of an fp8 rollout at Qwen3-4B widths, BRA_FP8_ANYK=0 against =1 (NOTES.md, "fp8 weights at any K").

    python tools/fp8_anyk_probe.py [--rows 8 16 32] [--layers 36] [--prompt 2180] [--steps 128] [--reps 3] [--no-anyk] [--tree DIR] [--json out.json]

Random weights, no adapters, `rollout_fp8`, one prompt per 8 rows (17+ rows: BRA_DEC_ROWS32=1).  The token loop alone is timed by the HIP
events of generate(loop_events=...), sampling T = 0.6 / top-k 20 / top-p 0.95, bf16 prompt pass; the two configurations alternate in one
process, one warm rollout each, then `--reps` rollouts each.  The prompt pass is timed (host-synchronised, generate(profile=...)) under
BRA_FP8_ANYK=1 with BRA_FP8_PREFILL=0 and =1.  `--no-anyk` measures the =0 column alone and `--tree` imports the package from another
checkout (with its own built library): together, the parent commit on the same box."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--prompt", type=int, default=2180)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-anyk", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from bioreason_amd import configs, generation
    from bioreason_amd.modeling import Qwen3ForCausalLM
    dev = torch.device("cuda:0")
    tc = dict(vocab_size=a.vocab, hidden_size=2560, intermediate_size=9728, num_hidden_layers=a.layers, num_attention_heads=32,
              num_key_value_heads=8, head_dim=128, rope_theta=1e6, max_position_embeddings=8192)
    m = Qwen3ForCausalLM(configs.qwen3_config(**tc), device=dev)
    m.init_weights(0.02, seed=1)
    m.ensure_packed()
    m.rollout_fp8 = True
    res = {"config": vars(a), "loop_ms_per_step": {}, "prefill_ms": {}, "fp8_proj": {}}
    g = torch.Generator().manual_seed(3)
    kw = dict(max_new_tokens=a.steps + 1, do_sample=True, temperature=0.6, top_k=20, top_p=0.95, eos_token_id=None)
    configs_ = ["0"] if a.no_anyk else ["0", "1"]

    def run(emb, mask, alias, **extra):
        ev = []
        generation.generate(m, emb, mask, prompt_alias=alias, loop_events=ev, **extra, **kw)
        torch.cuda.synchronize()
        e0, e1, n = ev[-1]
        return e0.elapsed_time(e1) / n

    for rows in a.rows:
        prompts = rows // 8
        os.environ["BRA_DEC_ROWS32"] = "1" if rows > 16 else "0"
        emb = (torch.randn(prompts, a.prompt, 2560, generator=g) * 0.02).to(torch.bfloat16).to(dev).repeat_interleave(8, 0)
        mask = torch.ones(rows, a.prompt, dtype=torch.long, device=dev)
        alias = [(r // 8) * 8 for r in range(rows)]
        os.environ["BRA_FP8_PREFILL"] = "0"
        times = {c: [] for c in configs_}
        for rep in range(a.reps + 1):
            for c in configs_:
                os.environ["BRA_FP8_ANYK"] = c
                ms = run(emb, mask, alias)
                if rep:                               # (rep 0 builds the weight set of the configuration and warms it)
                    times[c].append(round(ms, 4))
                res["fp8_proj"][f"{rows} rows, ANYK={c}"] = list(generation.rollout_weights(m, rows=rows)[0].get("fp8_proj", ()))
        res["loop_ms_per_step"][str(rows)] = times
        print(f"[fp8-anyk] {rows} rows: ms per token step " + "  ".join(f"ANYK={c}: {times[c]}" for c in configs_), flush=True)
        if not a.no_anyk:
            os.environ["BRA_FP8_ANYK"] = "1"
            pf = {}
            for w8 in ("0", "1"):
                os.environ["BRA_FP8_PREFILL"] = w8
                m.ensure_packed()._rollout = None                 # (the row-major images of the prompt pass are part of the cached set)
                pf[w8] = []
                for rep in range(a.reps + 1):
                    prof = {}
                    generation.generate(m, emb, mask, prompt_alias=alias, profile=prof, **dict(kw, max_new_tokens=2))
                    if rep:
                        pf[w8].append(round(prof["prefill"], 3))
                assert (generation.prefill_fp8_weights(m, rows) is not None) == (w8 == "1")
            res["prefill_ms"][str(rows)] = {"bf16": pf["0"], "w8a8": pf["1"]}
            print(f"[fp8-anyk] {rows} rows: prompt pass ms, bf16 {pf['0']}  W8A8 {pf['1']}", flush=True)
            m.ensure_packed()._rollout = None
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
