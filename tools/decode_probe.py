"""Rollout-only probe (full-size models, B=8, P=2180): prints ms per decode step.

PROBE_PROJ=1: instead, the streaming decode projections alone at the Qwen3-1.7B widths, 16 against 32 batch rows — us per launch and
fraction of the 8.0 TB/s HBM3E specification peak (the figure `roofline.frac` uses).  Every projection is launched back to back over a
ring of packed weight copies larger than L2 + MALL, so each launch streams from HBM; timed with events over the whole ring;
bytes = the weight matrix (activations and outputs are below 1 % of it)."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bioreason_amd import configs
from bioreason_amd.dna_llm import DNALLMModel
from bioreason_amd.synth import synth_prompt_batch

dev = torch.device("cuda:0")


def projection_table():
    from bioreason_amd import ops
    BF = torch.bfloat16
    HBM_PEAK = 8.0e12
    ROLES = [("qkv", 4096, 2048, dict(norm=True)), ("o", 2048, 2048, dict(res=True)), ("gate/up", 12288, 2048, dict(norm=True, act=True)),
             ("down", 2048, 6144, dict(res=True)), ("lm_head", 151936, 2048, dict(norm=True, out_f32=True))]

    def bench(M, N, K, norm=False, res=False, act=False, out_f32=False):
        ncopy = max(2, min(24, int(1.2e9 // (N * K * 2))))
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(M, K, generator=g)).to(BF).to(dev)
        nw = torch.ones(K, dtype=BF, device=dev)
        W = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF).to(dev)
        Wp = [ops.dec_pack_weights(W, act=act, out_f32=out_f32, norm_w=nw if norm else None, rows=16) for _ in range(ncopy)]
        del W
        r = torch.zeros(M, N, dtype=BF, device=dev) if res else None
        ss = ops.row_sumsq(x, 256) if norm else None
        tm = torch.empty(M, (N + 15) // 16, dtype=torch.float32, device=dev) if out_f32 else None

        def once(w):
            ops.dec_gemm2(x, w, ss_in=ss, norm_w=nw if norm else None, res=r, act=act, out_f32=out_f32, want_ss=res, packed=3 if norm else 1,
                          tile_max=tm)
        for w in Wp:
            once(w)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 4
        e0.record()
        for _ in range(reps):
            for w in Wp:
                once(w)
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / (reps * ncopy)
        return us, N * K * 2 / (us * 1e-6) / HBM_PEAK

    print("role      rows      us   frac_of_HBM   us_per_row")
    for name, N, K, kw in ROLES:
        for M in (16, 32):
            us, frac = bench(M, N, K, **kw)
            print("%-9s %4d %7.2f %13.3f %12.3f" % (name, M, us, frac, us / M), flush=True)


if os.environ.get("PROBE_PROJ") == "1":
    projection_table()
    sys.exit(0)
C = int(os.environ.get("PROBE_C", "64"))
m = DNALLMModel(configs.qwen3_config(), configs.nt_v2_config(), device=dev)
m.text_model.init_weights(0.02, seed=1); m.dna_model.init_weights(0.02, seed=2)
if os.environ.get("PROBE_LORA", "1") == "1":
    m.text_model.apply_lora(r=32, alpha=64.0, arena=m.arena)
b = synth_prompt_batch(B=8, n_unique=1, dna_token_id=m.dna_token_id, device=dev)
kw = dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"], dna_tokenized=b["dna_tokenized"], batch_idx_map=b["batch_idx_map"],
          dna_alias=b["dna_alias"], prompt_alias=b["prompt_alias"], do_sample=True, temperature=0.6, top_k=20, top_p=0.95, eos_token_id=None)
MODES = {"sg": (True, True), "se": (True, False), "ng": (False, True), "ne": (False, False)}
for shared_dec, graph in [MODES[k] for k in os.environ.get("PROBE_MODES", "sg,se,ng,ne").split(",")]:
    kw["shared_prefix_decode"], kw["use_graph"] = shared_dec, graph
    for it in range(2):
        torch.cuda.synchronize(); t0 = time.time()
        m.generate(max_new_tokens=1, **kw); torch.cuda.synchronize(); t1 = time.time()
        m.generate(max_new_tokens=C, **kw); torch.cuda.synchronize(); t2 = time.time()
        print("shared", shared_dec, "graph", graph, "prefill+1 ms %.1f" % ((t1 - t0) * 1e3), "gen", C, "ms %.1f" % ((t2 - t1) * 1e3),
              "per decode step ms %.3f" % (((t2 - t1) - (t1 - t0)) * 1e3 / (C - 1)), flush=True)

prof = {}
kw["shared_prefix_decode"], kw["use_graph"] = True, True
torch.cuda.synchronize(); t0 = time.time()
m.generate(max_new_tokens=C, profile=prof, **kw); torch.cuda.synchronize()
print("generate total ms %.1f" % ((time.time() - t0) * 1e3), {k: round(v, 2) for k, v in prof.items()}, flush=True)

# cost of rebuilding the merged rollout weights (done once per training step, after the optimizer touched the adapters)
from bioreason_amd import generation
eng = m.text_model.engine
for it in range(2):
    eng._rollout = None
    torch.cuda.synchronize(); t0 = time.time()
    generation.rollout_weights(m.text_model); torch.cuda.synchronize()
    print("rollout_weights rebuild ms %.2f" % ((time.time() - t0) * 1e3), flush=True)
