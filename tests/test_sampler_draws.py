"""The token samplers, draw by draw against float64: topk_slices_kernel, sample_kernel, sample_merge_kernel, sample_tiles_kernel,
sample_tiles_one_kernel and sample_full_kernel (k_grpo.hip) through bra_sample, bra_sample_embed, bra_sample_tiles and
bra_sample_full.  The other sampler tests are statistical (chi-square, frequencies), compare one path with a sibling, or bound the
log-prob by the kernel's own error; a draw mapped to the neighbouring token, a log-prob from the wrong normalisation, a uniform
shared between rows or steps, a candidate lost when one list holds all k survivors pass all of them.

The draw is deterministic: uniform01(seed, step, row) is a 32-bit integer hash (`u01` restates it with Python / numpy integers; the
result (h >> 8) / 2^24 is exact), the survivor list is ordered (value desc, index asc) with +0 == -0, and bra_sample_full draws in
index order.  So a numpy float64 reference (`Small`, `Full`; no project kernel is called) names THE token of every (seed, step, row).

  Small (<= 64 survivors)   first min(k, V) entries under (value desc, index asc); a_j = l_j / T; p = softmax(a); top-p from the tail
                            (drop while cum <= 1 - top_p, entry 0 stays); min-p as the prefix p_j >= min_p p_0; q = p / sum(kept);
                            token = the j whose interval [c_(j-1), c_j) of q's CDF holds u; log-prob = log q_j
  Full (bra_sample_full)    kept_k = {l >= k-th largest} (ties kept, as HF); top-p by value groups: kept iff the mass strictly above
                            is < top_p z (equal values stay or go together); min-p exp((l - max) / T) >= min_p; draw in INDEX order

Band.  Where the fp32 kernel and float64 may legitimately decide differently the reference says "undecided": u within DELTA of a CDF
edge, a top-p cumulative within DELTA of 1 - top_p (Full: mass above / z of top_p), a min-p ratio within DELTA of min_p.  An
undecided draw must still return one of the tokens whose interval meets (u - DELTA, u + DELTA) (two neighbours, unless an interval is
narrower than the band), or a token of the larger candidate support when a threshold is the fuzzy one.  The undecided share is
asserted <= 2 % per case from the reference alone BEFORE the kernel runs: a badly chosen input fails as bad input.

  DELTA = 2^-16.  Derived error of a CDF edge c_j = (p_0 + .. + p_j) / z2, in units of 2^-24 (one fp32 rounding):
    128            the two addition chains, z over the k <= 64 survivors and z2 (= the running sum the draw compares: same operands,
                   same order) over the kept ones
    2 (0.37 n + 4) the p_j: each is off by p_j (|a_j - a_0| + c) 2^-23 — the product with log2(e) in front of v_exp_f32 scales the
                   error with the argument, x e^-x <= 0.37, so the n <= 64 of them sum to at most (0.37 n + c) 2^-23; c = 4: v_exp_f32
                   itself (1 ulp = 2 roundings, the ISA manual's figure: the kernel guides state none), the division by z, the
                   rounding of (a_j - a_0)
    2 A            A = max |l_j / T| <= 24 (asserted on the inputs): without fma contraction (the emulator's build) l_j / T is
                   rounded before a_0 is subtracted
    2              u z2 and 1 - top_p
  = 128 + 55.4 + 48 + 2 = 233.4 < 256 = DELTA / 2^-24.  bra_sample_full: the chain is its kept set plus the block sum (26), the p_j term
  is 2 (E_p|a - a_0| + 4) with the expectation under the reference's own distribution (sum_j p_j |a_j - a_0|, what the 0.37 n bounds);
  it is computed per row and asserted <= DELTA, which limits the general path's cases to about 180 survivors.

Log-prob, every row of every draw:  |out_logp - log q_ref| <= (|a_pick - a_0| + n_add + 8) 2^-23 + L,  n_add = the additions of z
and z2 (Small: k + kept; Full: kept + 2).  L = absolute error of __logf over (2^-40, 1], measured against float64 log and doubled:

      backend     __logf realised as             measured max |err|        L (2 x)
      emulator    libm logf                      9.56e-07                  1.91e-06
      MI355X      v_log_f32 x ln 2               4.10e-06 (x = 2.3e-10)    8.20e-06
  (a stand-alone program: 2^21 points log-uniform over (2^-40, 1), 2^21 uniform over (0.001, 1]; the kernel guides state no figure;
  test_logf_figure_of_the_emulator re-checks the emulator's on a subset)

Worst excess  max(|out_logp - log q_ref| - bound)  of the unmodified kernels over every row of every draw of every case of a path
(negative: inside the bound; in brackets the largest error / bound — the additions' worst case never materialises):

      path                                                     emulator              MI355X
      sample_kernel<1024>                                      -3.10e-06 (0.121)     -9.39e-06 (0.035)
      topk_slices_kernel<10> + sample_merge_kernel             -3.10e-06 (0.084)     -9.39e-06 (0.045)
      bra_sample_embed                                         -3.10e-06 (0.138)     -9.39e-06 (0.037)
      bra_sample_tiles, two launches                           -3.10e-06 (0.121)     -9.39e-06 (0.045)
      sample_tiles_one_kernel<10, *>                           -3.10e-06 (0.070)     -9.39e-06 (0.035)
      topk_slices_kernel<16> + merge (V = 163 841)             skipped               -1.17e-05 (0.045)
      bra_sample_tiles at V = 163 840 / 163 857 / 327 697      skipped               -1.17e-05 (0.045)
      sample_tiles_one_kernel<16, *> (V = 163 857)             skipped               -1.17e-05 (0.045)
      sample_full_kernel                                       -3.22e-06 (0.062)     -9.51e-06 (0.042)
  (the excess is that of the case with the smallest bound: one survivor, 11 x 2^-23 + L.  Undecided draws: none in 75 of the 81
  cases, at most 2 / 205.)

Side outputs, exactly: tokens_out[row, step] holds the token and no other column changes; a finished row emits pad_id and keeps its
flag; a draw of eos_id / eos_id2 sets it; x == E[token]; ss[:, 0] == the float64 sum of squares within (H / 64 + 8) 2^-24 of it
(H / 64 products and additions per lane, six butterfly levels), its other columns 0, rows past B untouched; pos_out == pos0 + step
and rope_rows the (cos | sin) row of that position.
"""
import math

import numpy as np
import pytest
import torch

from bioreason_amd import ops
from bioreason_amd._lib import current_stream, get_lib

DELTA = 2.0 ** -16
U23 = 2.0 ** -23
CAP = 0.02
A_MAX = 24.0
# measured max |__logf(x) - log(x)| over (2^-40, 1] per backend (docstring table); L = 2 x
LOGF_ERR = {"cpu": 9.56e-07, "cuda": 4.10e-06}
M32 = 0xFFFFFFFF


def _f32(v):
    return float(np.float32(v))


# ----------------------------------------------------------------------------- the hash
def _hash(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def hash32(seed, step, row):
    """h of uniform01(seed, step, row): numpy uint64 arithmetic masked to 32 bits (broadcasts)"""
    step = np.asarray(step, dtype=np.uint64) & M32
    row = np.asarray(row, dtype=np.uint64) & M32
    a = _hash((step * np.uint64(0x9e3779b9) + np.uint64(0x85ebca6b)) & M32)
    b = _hash((row + np.uint64(0xc2b2ae35)) & M32)
    return _hash(np.uint64(seed & M32) ^ a ^ b)


def u01(seed, step, row):
    return (hash32(seed, step, row) >> np.uint64(8)).astype(np.float64) / 2.0 ** 24


def _u01_int(seed, step, row):
    """the same with Python ints (an independent restatement: the two must agree)"""
    def h(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & M32
        x ^= x >> 15
        x = (x * 0x846ca68b) & M32
        return x ^ (x >> 16)
    return (h((seed & M32) ^ h((step * 0x9e3779b9 + 0x85ebca6b) & M32) ^ h((row + 0xc2b2ae35) & M32)) >> 8) / 2.0 ** 24


# ----------------------------------------------------------------------------- references
def _interval(c, u):
    """indices j whose CDF interval [c_(j-1), c_j) meets (u - DELTA, u + DELTA) -> (lo, hi); lo == hi: decided"""
    lo = int(np.searchsorted(c, u - DELTA, side="right"))
    hi = int(np.searchsorted(c, u + DELTA, side="left"))
    n = len(c)
    return min(lo, n - 1), min(hi, n - 1)


class Small:
    """one row of the <= 64-survivor paths"""

    def __init__(self, l, T, k, top_p, min_p):
        l = np.asarray(l, dtype=np.float64) + 0.0                       # -0 -> +0: one value
        V = l.size
        self.tok = np.lexsort((np.arange(V), -l))[:min(k, V)]           # (value desc, index asc)
        self.k = k
        a = l[self.tok] / T
        self.x = a - a[0]
        e = np.exp(self.x)
        self.p = e / e.sum()
        self.amax = float(np.abs(a[e > 0]).max()) if int((e > 0).sum()) > 1 else 0.0
        self.keep_s, self.keep_g = self._keep(top_p, min_p, -DELTA), self._keep(top_p, min_p, DELTA)
        assert self.keep_s <= self.keep_g
        self.fuzzy = self.keep_s != self.keep_g
        self.c = np.cumsum(self.p[:self.keep_s]) / self.p[:self.keep_s].sum()
        self.pos = {int(t): i for i, t in enumerate(self.tok.tolist())}

    def _keep(self, top_p, min_p, s):
        """survivors of top-p + min-p with every comparison moved by s towards keeping (s > 0) or dropping (s < 0)"""
        p, n = self.p, len(self.p)
        keep = n
        if top_p < 1.0:
            cum = 0.0
            for j in range(n - 1, 0, -1):
                cum += p[j]
                if cum <= 1.0 - top_p - s:
                    keep = j
                else:
                    break
        if min_p > 0.0:
            kk = 1
            while kk < keep and p[kk] >= (min_p - s) * p[0]:
                kk += 1
            keep = kk
        return keep

    def draw(self, u):
        """-> (decided, token or None, allowed token set, [(position, log q, bound without L)] alternatives)"""
        if self.fuzzy:
            alts = []
            for kk in range(self.keep_s, self.keep_g + 1):
                z = self.p[:kk].sum()
                alts += [(j, math.log(self.p[j] / z), (abs(self.x[j]) + self.k + kk + 8) * U23) for j in range(kk) if self.p[j] > 0]
            return False, None, set(self.tok[:self.keep_g].tolist()), alts
        lo, hi = _interval(self.c, u)
        z = self.p[:self.keep_s].sum()
        alts = [(j, math.log(self.p[j] / z), (abs(self.x[j]) + self.k + self.keep_s + 8) * U23) for j in range(lo, hi + 1) if self.p[j] > 0]
        return lo == hi, int(self.tok[lo]), set(self.tok[lo:hi + 1].tolist()), alts


class Full:
    """one row of bra_sample_full"""

    def __init__(self, l, T, top_k, top_p, min_p):
        l = np.asarray(l, dtype=np.float64) + 0.0
        V = l.size
        kept_k = np.ones(V, dtype=bool)
        if 0 < top_k < V:
            kept_k = l >= np.sort(l)[V - top_k]                         # ties of the k-th value stay (HF: `scores < kth` is removed)
        self.x = (l - l.max()) / T
        e = np.exp(self.x)
        z = e[kept_k].sum()
        vals, inv = np.unique(-l, return_inverse=True)                  # value groups, descending
        gm = np.bincount(inv, weights=np.where(kept_k, e, 0.0), minlength=len(vals))
        above = (np.cumsum(gm) - gm)[inv] / z                           # mass strictly above each element's value, / z
        ex = float(np.where(kept_k & (e > 0), e * np.abs(np.where(e > 0, self.x, 0.0)), 0.0).sum() / z)     # E_p |a - a_0| over kept_k

        def kept(s):
            m = kept_k.copy()
            if top_p < 1.0:
                m &= above < top_p + s
            if min_p > 0.0:
                m &= e >= min_p - s
            return m
        ks, kg = kept(-DELTA), kept(DELTA)
        self.fuzzy = bool((ks != kg).any())
        self.idx = np.nonzero(ks)[0]
        self.idx_g = np.nonzero(kg)[0]
        self.e = e
        self.zf = e[self.idx].sum()
        self.c = np.cumsum(e[self.idx]) / self.zf
        # the serial chain of zf over the survivors, the block sums of zk and the mass above (two strided elements, six butterfly levels,
        # sixteen partials: 26), the p_j, u zf and top_p zk
        self.derived = (len(self.idx_g) + 26 + 2.0 * (ex + 4.0) + 2.0) * 2.0 ** -24
        self.amax = 0.0                                                 # (no 2 A term here: (l - max) is formed before the product with 1 / T,
                                                                        #  so run_case's A_MAX assertion has nothing to check on this path)

    def draw(self, u):
        if self.fuzzy:
            alts = []
            for idx in (self.idx, self.idx_g):
                z = self.e[idx].sum()
                alts += [(int(j), math.log(self.e[j] / z), (abs(self.x[j]) + len(idx) + 10) * U23) for j in idx if self.e[j] > 0]
            return False, None, set(self.idx_g.tolist()), alts
        lo, hi = _interval(self.c, u)
        n = len(self.idx)
        alts = [(int(self.idx[j]), math.log(self.e[self.idx[j]] / self.zf), (abs(self.x[self.idx[j]]) + n + 10) * U23)
                for j in range(lo, hi + 1) if self.e[self.idx[j]] > 0]
        return lo == hi, int(self.idx[lo]), set(self.idx[lo:hi + 1].tolist()), alts


# ----------------------------------------------------------------------------- value sets
SETS = ["normal", "flat", "peaked", "bf16grid", "ties_k", "clu_tile", "clu_slice", "spread", "half_inf", "one_finite", "forced", "zeros"]
_ROWS = {}


def _cluster(n):
    """n values well above the rest of a row and close together (seven levels, so there are ties): every one of them, the k-th
    included, carries a share of the probability — a survivor lost at the end of a list moves every draw's log-prob"""
    return 6.0 + 0.03125 * (torch.arange(n) * 3 % 7).float()


def make_row(kind, V, k, seed):
    """one logits row (fp32, [V]) of the value set `kind`; shared between the tests that need it, never modified"""
    key = (kind, V, k, seed)
    if key in _ROWS:
        return _ROWS[key]
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + k + 31 * SETS.index(kind))
    r = torch.randn(V, generator=g) * 2.0
    perm = torch.randperm(V, generator=g)
    kk = min(k, V)
    per64, per_t = (V + 63) // 64, ((V + 15) // 16 + 7) // 8
    if kind == "flat":
        r = r * 0.1                                                     # (x 0.2 of the unit normal)
    elif kind == "peaked":
        r = r.clamp(max=6.0)
        r[int(perm[0])] += 6.0
    elif kind == "bf16grid":                                            # many exact ties, no zeros
        r = r.to(torch.bfloat16).float()
        r[r == 0] = 0.5
    elif kind == "ties_k":                                              # k - 2 distinct values on top, then five equal ones across the k-th place
        r = -r.abs() - 1.0
        top = perm[:max(kk - 2, 0)]
        r[top] = 3.0 + torch.arange(len(top), dtype=torch.float32) * 0.125
        r[perm[max(kk - 2, 0):max(kk - 2, 0) + 5]] = 2.0
    elif kind == "clu_tile":                                            # the k best in as few 16-column tiles as hold them, inside ONE vocabulary slice
        s0 = (3 * per64 + 15) // 16 * 16 if V > 4 * per64 + 80 else 0
        r = r.clamp(max=3.0)
        n = min(s0 + kk, V) - s0
        r[s0:s0 + n] = _cluster(n)
    elif kind == "clu_slice":                                           # one per tile, all in ONE slice of the tile maxima
        s0 = per_t * 16 if 2 * per_t * 16 <= V else 0
        idx = s0 + 16 * torch.arange(kk) + 3
        r = r.clamp(max=3.0)
        r[idx[idx < V]] = _cluster(int((idx < V).sum()))
    elif kind == "spread":                                              # one per vocabulary slice
        idx = per64 * torch.arange(kk) + (5 if per64 > 5 else 0)
        r = r.clamp(max=3.0)
        r[idx[idx < V]] = _cluster(int((idx < V).sum()))
    elif kind == "half_inf":
        r[perm[:V // 2]] = float("-inf")
    elif kind == "one_finite":
        keep = float(r[int(perm[0])])
        r[:] = float("-inf")
        r[int(perm[0])] = keep
    elif kind == "forced":
        r[int(perm[0])] = 1.0e30                                        # as bra_force_token writes it
    elif kind == "zeros":                                               # +0 and -0 among the survivors and at the k-th place
        r = -r.abs() - 1.0
        top = perm[:max(kk - 3, 0)]
        r[top] = 1.0 + torch.arange(len(top), dtype=torch.float32) * 0.125
        z = perm[max(kk - 3, 0):max(kk - 3, 0) + 6]
        r[z] = torch.tensor([-0.0, 0.0, -0.0, 0.0, 0.0, -0.0])[:len(z)]
    _ROWS[key] = r.contiguous()
    return _ROWS[key]


def make_rows(sets, V, k, seed):
    return torch.stack([make_row(s, V, k, seed + i) for i, s in enumerate(sets)])


# ----------------------------------------------------------------------------- running one path
def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


class Aux:
    """the optional outputs of one case: allocated once, poisoned before every launch, checked after it"""

    def __init__(self, path, R, V, dev, step0, steps, fin, extras):
        self.path, self.R, self.V, self.dev = path, R, V, dev
        self.width = step0 + steps if step0 < 4096 else 0
        self.toks = torch.zeros(R, self.width, dtype=torch.int32, device=dev) if self.width else None
        self.fin0 = torch.zeros(R, dtype=torch.uint8)
        if fin:
            self.fin0[R - 1] = 1
        self.use_fin = fin
        self.H, self.hd = (256 if V < 100000 else 64), 64
        self.embed = extras and path in ("embed", "tiles", "one")
        self.advance = extras and path in ("tiles", "one") and step0 == 0
        if self.embed:
            g = torch.Generator().manual_seed(V)
            self.E = (torch.randn(V, self.H, generator=g) * 0.5).to(torch.bfloat16).to(dev)
            self.x = torch.zeros(R, self.H, dtype=torch.bfloat16, device=dev)
            self.ss = torch.zeros(R + 2, 4, device=dev)
        if self.advance:
            g = torch.Generator().manual_seed(V + 1)
            self.cosT = torch.randn(steps + 40, self.hd // 2, generator=g).to(dev)
            self.sinT = torch.randn(steps + 40, self.hd // 2, generator=g).to(dev)
            self.pos0 = (torch.arange(R, dtype=torch.int32) * 5 % 37).to(dev)
            self.pos = torch.zeros(R, dtype=torch.int32, device=dev)
            self.rows = torch.zeros(R, self.hd, device=dev)


def launch(path, dl, tmax, ws, T, k, top_p, min_p, seed, step, as_word, out, lp, aux, pad_id, eos, eos2, fin):
    """one draw of every row through `path`: the entry point is called directly (ops.sample would add a workspace of its own)"""
    R, V = dl.shape
    dev = dl.device
    lib = get_lib()
    st = current_stream(dl)
    word = _i32([step], dev) if (as_word or path in ("scan", "merge", "embed")) else None
    toks, ldt = (aux.toks, aux.toks.stride(0)) if aux.toks is not None else (None, 0)
    if path in ("scan", "merge"):
        lib.call("bra_sample", dl, dl.stride(0), R, V, T, k, top_p, 1, seed, word, fin, pad_id, eos, eos2, out, lp, toks, ldt,
                 ws if path == "merge" else None, min_p, st)
    elif path == "embed":
        E, x, ss = (aux.E, aux.x, aux.ss) if aux.embed else (None, None, None)
        lib.call("bra_sample_embed", dl, dl.stride(0), R, V, T, k, top_p, 1, seed, word, fin, pad_id, eos, eos2, out, lp, toks, ldt, ws,
                 E, E.stride(0) if E is not None else 0, aux.H if E is not None else 0, x, x.stride(0) if x is not None else 0, ss,
                 ss.shape[1] if ss is not None else 0, min_p, st)
    elif path in ("tiles", "one"):
        E, x, ss = (aux.E, aux.x, aux.ss) if aux.embed else (None, None, None)
        adv = (aux.pos0, aux.pos, aux.cosT, aux.sinT, aux.hd, aux.rows) if aux.advance else (None, None, None, None, 0, None)
        lib.call("bra_sample_tiles", dl, dl.stride(0), tmax, tmax.stride(0), R, V, T, k, top_p, 1, seed, word, 0 if word is not None else step,
                 fin, pad_id, eos, eos2, out, lp, toks, ldt, ws, E, E.stride(0) if E is not None else 0, aux.H if E is not None else 0,
                 x, x.stride(0) if x is not None else 0, ss, ss.shape[1] if ss is not None else 0, *adv, min_p, st)
    else:
        lib.call("bra_sample_full", dl, dl.stride(0), R, V, T, k, top_p, seed, word, 0 if word is not None else step, fin, pad_id, eos, eos2,
                 out, lp, toks, ldt, min_p, st)


def run_case(dev, path, sets, V, k, warp, seed, step0, rep=1, steps=25, lseed=1, fin=True, extras=True):
    """every draw of one case against the reference; -> worst log-prob excess"""
    T, top_p, min_p = (_f32(v) for v in warp)
    if step0 < 0:
        step0 = 2 ** 31 - steps
    logits = make_rows(sets, V, k, lseed)
    B = logits.shape[0]
    R = B * rep
    full = path == "full"
    refs = [Full(logits[b].numpy(), T, k, top_p, min_p) if full else Small(logits[b].numpy(), T, k, top_p, min_p) for b in range(B)]
    for b, r in enumerate(refs):
        assert r.amax <= A_MAX, ("bad input: |l / T| beyond the band's derivation", sets[b], r.amax)
        if full:
            assert r.derived <= DELTA, ("bad input: derived band above 2^-16", sets[b], r.derived, len(r.idx_g))
    fin = fin and R > 1
    live = R - 1 if fin else R
    assert live * steps >= 200

    def no_flags(s):
        """steps launched WITHOUT the finished array (a null pointer: every row draws), one in five when there are several rows"""
        return R == 1 or s % 5 == 4
    # ---- the reference's draws and the undecided share, before any kernel runs
    st = step0 + np.arange(steps)
    us = u01(seed, st[:, None], np.arange(R)[None, :])
    assert us.shape == (steps, R) and us[1, 0] == _u01_int(seed, int(st[1]), 0) and us[-1, R - 1] == _u01_int(seed, int(st[-1]), R - 1)
    want = [[refs[r % B].draw(float(us[s, r])) for r in range(R)] for s in range(steps)]
    drawn = [(s, r) for s in range(steps) for r in range(R) if r < live or no_flags(s)]
    und = sum(1 for s, r in drawn if not want[s][r][0])
    share = und / len(drawn)
    assert share <= CAP, ("bad input: undecided share", share, [(sets[b], refs[b].fuzzy) for b in range(B)])
    # ---- eos ids: the reference's most frequent token of row 0 and another row's (never the pad id 0)
    seen = [w[1] for s in range(steps) for w in want[s][:live] if w[0] and w[1] != 0]
    eos = max(set(seen), key=seen.count) if seen else -1
    rest = [t for t in seen if t != eos]
    eos2 = max(set(rest), key=rest.count) if rest else -1
    pad_id = 0
    dl = logits.repeat(rep, 1).contiguous().to(dev)
    tmax = ops.tile_max(dl) if path in ("tiles", "one") else None
    kk = k if not full else 1
    ws = torch.empty(2 * R * 64 * max(kk, 1), dtype=torch.float32, device=dev) if path in ("merge", "embed", "tiles", "one") else None
    aux = Aux(path, R, V, dev, step0, steps, fin, extras)
    out = torch.empty(R, dtype=torch.int32, device=dev)
    lp = torch.empty(R, device=dev)
    L = 2.0 * LOGF_ERR[dev.type]
    worst, ratio = -1.0, 0.0
    for s in range(steps):
        step = int(st[s])
        out.fill_(-7)
        lp.fill_(float("nan"))
        finished = None if no_flags(s) else aux.fin0.clone().to(dev)
        if aux.toks is not None:
            aux.toks.fill_(-5)
        if aux.embed:
            aux.x.fill_(9.0)
            aux.ss.fill_(7.0)
        if aux.advance:
            aux.pos.fill_(-3)
            aux.rows.fill_(9.0)
        launch(path, dl, tmax, ws, T, k, top_p, min_p, seed, step, s % 2 == 0, out, lp, aux, pad_id, eos, eos2, finished)
        got, glp = out.cpu().tolist(), lp.cpu().double().tolist()
        tok_true = []
        for r in range(R):
            decided, tok, allowed, alts = want[s][r]
            was_fin = finished is not None and int(aux.fin0[r]) == 1
            where = f"{path} set={sets[r % B]} V={V} k={k} warp={warp} seed={seed:#x} step={step} row={r}"
            if was_fin:
                assert got[r] == pad_id, where
                cands = alts
                tok_true.append(pad_id)
            else:
                if decided:
                    assert got[r] == tok, ("wrong token", where, got[r], tok, float(us[s, r]))
                else:
                    assert got[r] in allowed, ("token outside the band's candidates", where, got[r], sorted(allowed))
                j = refs[r % B].pos[got[r]] if not full else got[r]
                cands = [a for a in alts if a[0] == j]
                assert cands, where
                tok_true.append(got[r])
            exc = min(abs(glp[r] - lq) - (bd + L) for _, lq, bd in cands)
            assert not math.isnan(exc), where
            worst = max(worst, exc)
            ratio = max(ratio, min(abs(glp[r] - lq) / (bd + L) for _, lq, bd in cands))
            assert exc <= 0.0, ("log-prob", where, glp[r], [c[1] for c in cands], exc)
        tt = torch.tensor(tok_true, dtype=torch.int64)
        if finished is not None:
            hit = torch.tensor([(t == eos and eos >= 0) or (t == eos2 and eos2 >= 0) for t in tok_true], dtype=torch.uint8)
            assert torch.equal(finished.cpu(), aux.fin0 | hit), (path, step)
        if aux.toks is not None:
            tk = aux.toks.cpu()
            assert tk[:, step].tolist() == tok_true, (path, step)
            tk[:, step] = -5
            assert bool((tk == -5).all()), ("tokens_out: another column was written", path, step)
        if aux.embed:
            assert torch.equal(aux.x.cpu(), aux.E.cpu()[tt]), (path, step)
            ss = aux.ss.cpu().double()
            ref_ss = aux.E.cpu()[tt].double().pow(2).sum(1)
            assert bool(((ss[:R, 0] - ref_ss).abs() <= (aux.H / 64 + 8) * 2.0 ** -24 * ref_ss).all()), (path, step)
            assert float(ss[:R, 1:].abs().max()) == 0.0 and float(ss[R:].min()) == 7.0 and float(ss[R:].max()) == 7.0
        if aux.advance:
            wp = aux.pos0.cpu().long() + step
            assert torch.equal(aux.pos.cpu().long(), wp)
            assert torch.equal(aux.rows.cpu(), torch.cat([aux.cosT.cpu()[wp], aux.sinT.cpu()[wp]], -1))
    print(f"{path} {'+'.join(sets) if B <= 3 else 'all-sets'} V={V} k={k} warp={warp} seed={seed:#x} step0={step0}: undecided {und}/{len(drawn)}"
          f" worst log-prob excess {worst:.3e} (error / bound at most {ratio:.3f})")
    return worst


# ----------------------------------------------------------------------------- cases
W = [(0.6, 0.95, 0.0), (1.0, 1.0, 0.0), (0.7, 0.5, 0.05), (1.3, 0.9, 0.3)]
S0 = [0, 1, 300, -1]                            # -1: the case's last step is 2^31 - 1
SEEDS = [0, 99, 0xFFFFFFFF]
ALL = SETS
TRI = [["normal", "zeros", "ties_k"], ["flat", "peaked", "bf16grid"], ["half_inf", "forced", "clu_tile"], ["spread", "clu_slice", "one_finite"]]


def _cases(vk, b17):
    """(sets, V, k, warp, seed, step0, rep, steps): B = 1 (208 steps), 3 (x 3 rows) over `vk`, and 17 rows over `b17`; every warp, seed
    and step0 comes round"""
    cs = []
    for i, (V, k, *ls) in enumerate(vk):
        w, sd, s0 = W[i % 4], SEEDS[i % 3], S0[(i + 1) % 4]
        if i % 3 == 0:
            cs.append(([SETS[(5 * i) % 12]], V, k, w, sd, s0, 1, 208, *ls))
        else:
            cs.append((TRI[i % 4], V, k, w, sd, s0, 3, 25, *ls))
    for i, (V, k) in enumerate(b17):
        cs.append((ALL + ALL[:5], V, k, W[(i + 1) % 4], SEEDS[(i + 1) % 3], S0[i % 4], 1, 25))     # (the first of them without top-p)
    return cs


def _ids(cs):
    return [f"{'B1' if len(c[0]) == 1 else 'B3' if len(c[0]) == 3 else 'B17'}-V{c[1]}-k{c[2]}-w{W.index(c[3])}-s{c[5] if c[5] >= 0 else 'max'}" for c in cs]


SCAN = _cases([(1, 1), (7, 4), (17, 20), (40, 64), (300, 21), (4095, 63), (40, 2), (300, 3), (17, 64), (4096, 20), (7, 1), (5003, 2)],
              [(300, 20), (4095, 64), (40, 21), (4097, 3)])
MERGE = _cases([(4096, 1), (4097, 2), (5003, 3), (4096, 4), (4097, 20), (5003, 21), (4096, 63), (4097, 64)],
               [(4096, 20), (4097, 21), (5003, 3)])
EMBED = _cases([(4096, 20), (5003, 64), (4097, 3), (4096, 63), (4097, 1), (5003, 2), (4096, 4), (4097, 63)], [(4096, 21), (5003, 20)])
TILES = _cases([(1, 1), (7, 2), (17, 3), (40, 4), (300, 20), (4095, 21), (4096, 63), (4097, 64), (5003, 20), (40, 64), (300, 63), (17, 21)],
               [(4096, 20), (5003, 64), (300, 21), (4097, 3)])
ONE = _cases([(300, 20), (5003, 21), (17, 4), (4096, 64), (1, 1), (7, 2), (40, 3), (4095, 2), (40, 1), (7, 3), (4095, 63)], [(4096, 20), (4097, 63)])
# (V, k, seed of the logits: chosen on the CPU so that no row's top-p / min-p threshold lies in the band — run_case asserts it)
BIG_SLICES = [(163841, 20, 1), (163841, 64, 1)]               # bra_sample: topk_slices_kernel<16>
BIG_TILES = [(163840, 20, 1), (163857, 21, 1), (327697, 20, 1), (327697, 64, 1)]      # bra_sample_tiles: topk_slices_kernel<5>, <10>, <16>
BIG_ONE = [(163857, 20, 2), (163857, 21, 1)]                  # sample_tiles_one_kernel<16, 5> and <16, 16>


@pytest.mark.parametrize("case", SCAN, ids=_ids(SCAN))
def test_sample_kernel_draws(backend, case):
    """sample_kernel<1024>: bra_sample without a workspace (and every V < 4096)"""
    run_case(backend, "scan", *case)


@pytest.mark.parametrize("case", MERGE, ids=_ids(MERGE))
def test_slices_and_merge_draws(backend, case):
    """topk_slices_kernel<10> + sample_merge_kernel: bra_sample with a workspace, V >= 4096"""
    run_case(backend, "merge", *case)


@pytest.mark.parametrize("case", EMBED, ids=_ids(EMBED))
def test_sample_embed_draws(backend, case):
    """bra_sample_embed: the merge kernel with E / x / ss"""
    run_case(backend, "embed", *case)


@pytest.mark.parametrize("case", TILES, ids=_ids(TILES))
def test_sample_tiles_draws(backend, case):
    """bra_sample_tiles in two launches: topk_slices_kernel<5> + sample_tiles_kernel<3, 5> (k <= 20) / <8, 16> (k >= 21)"""
    run_case(backend, "tiles", *case)


@pytest.mark.parametrize("case", ONE, ids=_ids(ONE))
def test_sample_tiles_one_launch_draws(debug_backend, case):
    """sample_tiles_one_kernel<10, 5> and <10, 16> (bra_sample_set_one_launch of the debug library)"""
    get_lib().call("bra_sample_set_one_launch", 1)
    try:
        run_case(debug_backend, "one", *case)
    finally:
        get_lib().call("bra_sample_set_one_launch", 0)


def _big(dev, path, V, k, i, lseed):
    if dev.type == "cpu":
        pytest.skip("emulator: a 64 x 256-fiber scan of > 160 000 logits per row and draw takes minutes; the GPU run covers it")
    sets = ["normal", "clu_tile", "zeros", "spread", "ties_k", "clu_slice", "bf16grid", "peaked", "forced"]
    run_case(dev, path, sets, V, k, W[i % 4], SEEDS[i % 3], S0[i % 4], 1, 26, extras=(i % 2 == 0), lseed=lseed)


@pytest.mark.parametrize("i,V,k,lseed", [(i, V, k, ls) for i, (V, k, ls) in enumerate(BIG_SLICES)])
def test_slices16_and_merge_draws(backend, i, V, k, lseed):
    """topk_slices_kernel<16> + merge: the smallest V with more than 2560 logits per slice"""
    _big(backend, "merge" if i else "embed", V, k, i, lseed)


@pytest.mark.parametrize("i,V,k,lseed", [(i, V, k, ls) for i, (V, k, ls) in enumerate(BIG_TILES)])
def test_sample_tiles_large_vocabulary_draws(backend, i, V, k, lseed):
    """bra_sample_tiles at the boundaries of topk_slices_kernel<5> / <10> / <16> over the tile maxima"""
    _big(backend, "tiles", V, k, i, lseed)


@pytest.mark.parametrize("i,V,k,lseed", [(i, V, k, ls) for i, (V, k, ls) in enumerate(BIG_ONE)])
def test_sample_tiles_one_launch_large_vocabulary_draws(debug_backend, i, V, k, lseed):
    """sample_tiles_one_kernel<16, 5> and <16, 16>: more than 10 240 tiles"""
    get_lib().call("bra_sample_set_one_launch", 1)
    try:
        _big(debug_backend, "one", V, k, i, lseed)
    finally:
        get_lib().call("bra_sample_set_one_launch", 0)


# bra_sample_full: (sets, V, top_k, warp, seed, step0, rep, steps); the kept sets stay below ~180 so that the derived band holds
FULL = [
    (["normal", "peaked", "bf16grid", "ties_k", "half_inf", "forced", "zeros", "clu_tile", "spread", "normal", "peaked", "bf16grid", "ties_k",
      "zeros", "forced", "half_inf", "normal"], 1500, 100, W[0], 99, 0, 1, 25),
    (["normal", "flat", "zeros"], 150, 0, W[1], 0, -1, 3, 25),
    (["normal", "peaked", "one_finite"], 1500, 0, W[2], 0xFFFFFFFF, 300, 3, 25),
    (["ties_k", "zeros", "peaked"], 300, 400, W[3], 0, 1, 3, 25),
    (["normal"], 7, 0, W[1], 99, 0, 1, 208),
    (["one_finite"], 1, 65, W[0], 0xFFFFFFFF, 1, 1, 208),
    (["zeros", "ties_k", "half_inf"], 1025, 65, W[2], 99, 300, 3, 25),
]


@pytest.mark.parametrize("case", FULL, ids=[f"V{c[1]}-k{c[2]}-w{W.index(c[3])}" for c in FULL])
def test_sample_full_draws(backend, case):
    """sample_full_kernel: top_k = 0, top_k > 64, top_k >= V; ties of the k-th value are kept, the draw runs in index order"""
    run_case(backend, "full", *case)


# ----------------------------------------------------------------------------- the tie rules, pinned
def test_tie_rules_of_the_references():
    """ties across the k-th place: the <= 64 paths keep exactly k, lower indices first; bra_sample_full (and HF) keep every tie; +0
    and -0 are one value for both"""
    l = np.array([1.0, 2.0, 0.0, 2.0, -0.0, 2.0, 5.0, 0.0], dtype=np.float64)
    s = Small(l, 1.0, 3, 1.0, 0.0)
    assert s.tok.tolist() == [6, 1, 3]
    f = Full(l, 1.0, 3, 1.0, 0.0)
    assert f.idx.tolist() == [1, 3, 5, 6]
    assert Small(l, 1.0, 6, 1.0, 0.0).tok.tolist() == [6, 1, 3, 5, 0, 2]
    assert Full(l, 1.0, 6, 1.0, 0.0).idx.tolist() == [0, 1, 2, 3, 4, 5, 6, 7]


# ----------------------------------------------------------------------------- all <= 64-survivor paths agree bit for bit
@pytest.mark.parametrize("V,k", [(4096, 20), (4097, 64), (40, 64), (40, 20)])
def test_fast_paths_agree_on_every_value_set(debug_backend, V, k):
    """on every value set, signed zeros included, sample_kernel, slices + merge, bra_sample_embed, bra_sample_tiles and its one-launch
    form return identical tokens and bit-identical log-probs (V = 40: the issue's signed-zero reproducer, round(2 randn) at seed 40)"""
    dev = debug_backend
    if V == 40:
        logits = torch.round(torch.randn(3, 40, generator=torch.Generator().manual_seed(40)) * 2)
        assert bool((logits == 0).any()) and bool(torch.signbit(logits[logits == 0]).any()) and not bool(torch.signbit(logits[logits == 0]).all())
        paths, seed, st0 = ["scan", "tiles", "one"], 11, 7
    else:
        logits = make_rows(SETS, V, k, 3)
        paths, seed, st0 = ["scan", "merge", "embed", "tiles", "one"], 99, 0
    R = logits.shape[0]
    dl = logits.to(dev)
    tmax = ops.tile_max(dl)
    ws = torch.empty(2 * R * 64 * k, dtype=torch.float32, device=dev)
    T, top_p, min_p = 1.0, 1.0, 0.0                # (no top-p cut: the zeros in the middle of a row keep their share of the draws)
    refs = [Small(logits[b].numpy(), T, k, top_p, min_p) for b in range(R)]
    for s in range(24 if V == 40 else 8):
        res = {}
        for path in paths:
            aux = Aux(path, R, V, dev, 0, 32, False, False)
            out = torch.full((R,), -7, dtype=torch.int32, device=dev)
            lp = torch.full((R,), float("nan"), device=dev)
            get_lib().call("bra_sample_set_one_launch", 1 if path == "one" else 0)
            try:
                launch(path, dl, tmax, ws, T, k, top_p, min_p, seed, st0 + s, s % 2 == 0, out, lp, aux, 0, -1, -1, None)
            finally:
                get_lib().call("bra_sample_set_one_launch", 0)
            res[path] = (out.cpu(), lp.cpu())
        for path in paths[1:]:
            assert res[path][0].tolist() == res[paths[0]][0].tolist(), (path, st0 + s, res[path][0].tolist(), res[paths[0]][0].tolist())
            assert torch.equal(res[path][1].view(torch.int32), res[paths[0]][1].view(torch.int32)), (path, st0 + s)
        for r in range(R):
            decided, tok, allowed, _ = refs[r].draw(float(u01(seed, st0 + s, r)))
            if decided:
                assert int(res["scan"][0][r]) == tok, (r, st0 + s)


# ----------------------------------------------------------------------------- the hash, on the host
def test_uniform_hash_statistics():
    """256-bin chi-square of u and the 16 x 16 chi-squares of the pairs (u[s, r], u[s + 1, r]) and (u[s, r], u[s, r + 1]) over 4096
    steps x 32 rows, under the suite's chi-square rule dof + 5 sqrt(2 dof) + 5 (= 372.9 at dof 255); fixed inputs: deterministic"""
    dof = 255
    bound = dof + 5.0 * math.sqrt(2.0 * dof) + 5.0
    assert abs(bound - 372.9) < 0.05
    s, r = np.arange(4096)[:, None], np.arange(32)[None, :]
    for seed in (0, 42, 99, 1234, 0xFFFFFFFF):
        h = hash32(seed, s, r)
        u = (h >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
        assert u[5, 3] == _u01_int(seed, 5, 3) and u[4095, 31] == _u01_int(seed, 4095, 31)
        # u is built from the TOP 24 bits: the bottom 8 of h do not enter it
        assert np.array_equal(u, ((h & np.uint64(0xFFFFFF00)) >> np.uint64(8)).astype(np.float64) / 2.0 ** 24)
        assert not np.array_equal(u, (h & np.uint64(0xFFFFFF)).astype(np.float64) / 2.0 ** 24)

        def chi2(cells, ncell):
            o = np.bincount(cells.ravel(), minlength=ncell).astype(np.float64)
            e = cells.size / ncell
            return float(((o - e) ** 2 / e).sum())
        b16 = (u * 16).astype(np.int64)
        stats = [chi2((u * 256).astype(np.int64), 256), chi2(b16[:-1] * 16 + b16[1:], 256), chi2(b16[:, :-1] * 16 + b16[:, 1:], 256)]
        for v in stats:
            assert v <= bound, (seed, stats)


def test_band_derivation():
    """the docstring's sum for the <= 64-survivor paths stays under DELTA"""
    units = 128 + 2 * (0.37 * 64 + 4) + 2 * A_MAX + 2
    assert units * 2.0 ** -24 <= DELTA, units


def test_logf_figure_of_the_emulator():
    """LOGF_ERR["cpu"] still covers the host's logf (what the emulator build calls for __logf): 2^16 points log-uniform over
    (2^-40, 1) and 2^12 next to 1, through ctypes; a libm whose error grew past the recorded figure would make L too small"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    x = np.concatenate([np.exp2(-40.0 * (np.arange(1 << 16) + 1) / (1 << 16)), 1.0 - np.arange(1 << 12) / (1 << 12) * 0.999]).astype(np.float32)
    worst = max(abs(float(libm.logf(float(v))) - math.log(float(v))) for v in x)
    print(f"host logf: max |err| {worst:.3e} over {x.size} points (recorded {LOGF_ERR['cpu']:.3e})")
    assert 0.0 < worst <= LOGF_ERR["cpu"], worst
