// k_decgemm.hip — weight-streaming projections of the single-token decode step, second generation.
// Arithmetic: y[M<=16, N] = rmsnorm(x; w, eps) W^T (+ res) | SwiGLU | fp32 logits — Qwen3DecoderLayer.forward with a
// KV cache (TF:qwen3:294-323), Qwen3RMSNorm (TF:qwen3:59-64), Qwen3MLP (TF:qwen3:81-83), tied lm_head (TF:qwen3:495).
//
// At M = 8 rows a projection is pure HBM streaming of its weight matrix (8.4 - 50 MB per launch), and a launch lasts
// only a few microseconds, so what decides its speed is how many bytes are in flight how soon after the launch:
//   * every lane requests ALL the 16-byte weight chunks it will consume (NL per lane, non-temporal) in its first
//     instructions, together with the activations, the residual and the norm statistics; nothing waits on anything
//     before the first MFMA;
//   * no RMSNorm prologue pass: the PRODUCER of x (o_proj / down_proj epilogue here, bra_row_sumsq after the embedding
//     gather) leaves per-workgroup partial sums of squares [8][nss]; every wave folds them in a fixed order
//     (deterministic) and normalises just the fragments it multiplies;
//   * N = hidden projections (o_proj, down_proj) use 8-column workgroups so that 256 workgroups exist, and fill the
//     16x16x32 MFMA by putting two K-halves on the two row halves of A and B ("diagonal" mode): the products
//     C[j][b] and C[j+8][b+8] are the two K-halves of output (b, j); all 64 lanes stream weights.
#include "bra_decgemm.h"
#include "bra_api_internal.h"
#include <array>
#include <utility>

namespace bra {

// MODE 0: 16 output columns per tile, 32 k per step.  MODE 1: 8 columns, 64 k per step (diagonal).
// A workgroup walks the tiles blockIdx.x, + gridDim.x, ..: its waves split K, keep their (normalised) activation
// fragments in registers for all tiles, request tile i+1's weights before multiplying tile i, and hand the K-reduction
// and epilogue of tile i to wave i % NW through a double-buffered LDS slab (one barrier per tile).
// WIDE: 9 .. 16 batch rows (two prompts x 8 rollouts per GPU): MODE 0 only (the diagonal tiles hold 8 rows), folded norm or none
// WIDE == 2: 17 .. 32 batch rows (three or four prompts x 8 rollouts): the weight fragment of a (tile, k-step) is requested once, as
// in the 16-row form, and feeds TWO MFMAs — against the activation fragments of rows 0 - 15 and of rows 16 - 31 — into two
// accumulators.  Per output element the K-reduction is the 16-row form's own (same k-steps per wave, same wave order in the LDS
// hand-off, same fold of the statistics), so row r of a 32-row launch is bit-identical to row r of a 16-row launch on the same
// inputs.  The two row halves of a tile are finished by two different waves (i % NW and (i + 1) % NW), each through the unchanged
// 16-row epilogue on a record whose row pointers are moved down 16 rows.
// PK: the weights are in fragment order (compile-time: with a run-time flag every weight address is built both ways and selected,
// ~100 VALU instructions between kernel entry and the first weight request of a launch that lasts 5-11 us)
// FAST (the shapes of the decode step): packed weights, K == NW * NL * KS exactly (one register round, no step is clamped or
// zeroed), every offset fits 32 bits (host-checked), no probe stamps.  With two waves per SIMD each prologue instruction costs
// ~8 cycles of the launch's critical path, so the path to the first request is kept to: kernel arguments, one 24-bit multiply
// per base, scalar base + 32-bit lane offset + immediate per request.
#define BRA_DG2_HEAD_PARAMS const bf16_t* h_x, const bf16_t* h_W, const bf16_t* h_res, const float* h_ss_in, int h_ldx, int h_ldres, int h_M, int h_N, \
                            int h_K, int h_nss_in
#define BRA_DG2_HEAD_ARGS(g) (g).x, (g).W, (g).res, (g).ss_in, (int)(g).ldx, (int)(g).ldres, (g).M, (g).N, (g).K, (g).nss_in
// F8 (round 5; FAST only): the packed weights are fp8 e4m3 with one fp32 scale per output row (bra_dec_pack_weights_fp8) — HALF the
// streamed bytes.  A 16-byte request then carries the lane's fragments of TWO consecutive k-steps (8 + 8 bytes), decoded to bf16 in
// registers (exact: v_cvt_scalef32_pk_bf16_fp8, 4 instructions per step) in front of the same bf16 MFMAs; the row scale multiplies the
// K-reduced products next to rstd.  Activations, accumulation and every epilogue are unchanged (W8A16).  With WIDE == 1 (9 .. 16 rows,
// bra_dec_pack_weights_fp8_rows(rows = 16): 16-column tiles for every projection) the accumulation order, the LDS hand-off and the
// two-pass statistics fold are the bf16 16-row form's; the 16-wave forms (K = 4096, 6144) hold one half-size weight set, one tile per
// workgroup.  With WIDE == 2 (17 .. 32 rows, the same rows = 16 image) a request still goes out once and feeds both row halves; k-steps per
// wave, hand-off, the four-wave statistics fold and the scale next to rstd are unchanged per output element, so row r is bit-identical
// to row r of the 16-row fp8 form.  No multi-round (WIDE == 3) fp8 form: fp8 images exist at single-round K only.
template <int MODE, int NORM, int ACT, int OUTF32, int NW, int NL, int WIDE = 0, int PK = 0, int FAST = 0, int F8 = 0>
__global__ __launch_bounds__(NW * 64) void dec_gemm2_kernel(BRA_DG2_HEAD_PARAMS, DecGemm2Args g0) {
    // everything between kernel entry and the first weight / activation request arrives in SGPRs with the wave (kernel-argument
    // preload, -mllvm -amdgpu-kernarg-preload-count: the leading 14 dwords); the rest of the record is fetched from the argument
    // segment while the requests are in flight (a scalar load of the arguments is one memory round trip that every wave of a
    // 5 - 10 us launch otherwise waits for before it can form its first address)
    DecGemm2Args g = g0;
    g.x = h_x; g.W = h_W; g.res = h_res; g.ss_in = h_ss_in; g.ldx = h_ldx; g.ldres = h_ldres; g.M = h_M; g.N = h_N; g.K = h_K; g.nss_in = h_nss_in;
    // WIDE == 3: the 32-row form of the multi-round loop alone (K beyond one register round) — a kernel of its own, so that neither
    // path pays for the other's registers
    constexpr bool W32 = WIDE >= 2;
    static_assert(dg2_kernel_exists({MODE, NORM, ACT, OUTF32, NW, NL, WIDE, PK, FAST, F8}), "not a form of bra_decgemm.h's list");
    // (fp8, 16 rows: the same decode in front of the 16-row form's MFMAs, statistics fold and hand-off — row r of a 16-row launch does
    //  not depend on M)
    // (fp8, 32 rows: every 16-byte request is issued once and feeds both row halves — decoded once where rows 16 .. 31 have registers of
    //  their own, a second time behind the first chain on 16 waves, where they take the registers of rows 0 .. 15)
    constexpr int NLW = F8 ? NL / 2 : NL;                               // 16-byte weight requests per lane and tile
    constexpr int NH = W32 ? 2 : 1;                               // 16-row halves of the batch (slab rows [h * NW, (h + 1) * NW))
    // (32 rows x 16 waves: one slab — 64 KiB of LDS would hold two; the single-round form of 16 waves runs one tile per workgroup,
    //  the multi-round loop pays a second barrier per tile)
    // INVARIANT (dg2_form_of: `gmax = nw == 16 ? ntiles : ..`): the single-round form of 16 waves gets one workgroup per tile — it
    // reuses x[] for rows 16 .. 31 and has one slab, both wrong for a second tile; the multi-round loop re-reads x and pays the
    // second barrier, so it may walk several tiles
    constexpr int NBUF = (W32 && NW == 16) ? 1 : 2;
    __shared__ float red[NBUF][NH * NW][64][4];
    constexpr int KS = MODE ? 64 : 32;
    constexpr int NCOL = MODE ? 8 : 16;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    if (!FAST) dg2_stamp(g, 0);
    const int nsteps = FAST ? NW * NL : g.K / KS;
    const int ntiles = (g.N + NCOL - 1) / NCOL;
    const int lrow = MODE ? (fr & 7) : fr;                            // A row = weight row, B row = batch row
    const int koff = MODE ? ((fr >> 3) * 32 + fq * 8) : fq * 8;
    const int xr = lrow < g.M ? lrow : g.M - 1;
    const bf16_t* xp = FAST ? g.x + (dg2_mul24(xr, (int)g.ldx) + (unsigned)koff) : g.x + (long)xr * g.ldx + koff;
    // rows 16 .. 31 (W32): clamped like the first half — a row past M re-reads row M - 1 and is never stored.  Everything
    // the second half needs is formed BEHIND the weight requests: the path from kernel entry to the first request stays the
    // 16-row form's
    auto x2_ptr = [&]() -> const bf16_t* {
        const int xr2 = lrow + 16 < g.M ? lrow + 16 : g.M - 1;
        return FAST ? g.x + (dg2_mul24(xr2, (int)g.ldx) + (unsigned)koff) : g.x + (long)xr2 * g.ldx + koff;
    };
    auto second_half = [&]() -> DecGemm2Args {        // the record the second half's epilogue sees: the same tile, 16 rows down
        DecGemm2Args g2 = g;
        g2.M = g.M - 16;
        if (g.res) g2.res = g.res + 16 * g.ldres;
        g2.out = OUTF32 ? (void*)((float*)g.out + 16 * g.ldo) : (void*)((bf16_t*)g.out + 16 * g.ldo);
        if (g.ss_out) g2.ss_out = g.ss_out + 16 * (long)g.nss_out;
        return g2;
    };
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const int rounds = FAST ? 1 : (nsteps + NW * NL - 1) / (NW * NL);
    int tile = (int)blockIdx.x;
    int rn = tile * NCOL + lrow; rn = rn < g.N ? rn : g.N - 1;
    const bf16_t* wp = FAST ? g.W : g.W + (long)rn * g.ldw + koff;

    // epilogue operand of the first tile requested now (all waves, clamped address: no branch around a load)
    const int em = fr < g.M ? fr : g.M - 1;
    int en = tile * NCOL + 4 * fq; en = en + 3 < g.N ? en : (g.N >= 4 ? g.N - 4 : 0);
    u32x2 resv = {0u, 0u}, resv2 = {0u, 0u};
    if (!FAST && !ACT && !OUTF32 && g.res) resv = ld8(g.res + (long)em * g.ldres + en);
    auto em2_row = [&]() -> int { return fr + 16 < g.M ? fr : g.M - 17; };      // row of the second half's record (formed where it is used)

    // NORM: lane l folds partials [per * (l & 7), per * (l & 7) + per) of row l >> 3 (per <= 32, fixed order =>
    // run-to-run identical); requested first, they are the smallest and the first thing the MFMAs need
    // NORM == 2 ("folded"): the RMSNorm weight is already multiplied into the (packed) weights and the row factor rstd is
    // applied to the K-reduced products in the epilogue — y = rstd * (x (W . nw)^T) — so no wave loads norm weights or
    // statistics up front (the per-CU load path, 64 B/clk, is what bounds these kernels: the activation-side loads of
    // NORM == 1 are 3x the weight bytes); wave 0 alone folds the statistics, behind its weight requests, into LDS.
    const int per = NORM ? g.nss_in >> 3 : 0;
    f32x4 pv[8];
    __shared__ float rs_lds[W32 ? 32 : (WIDE ? 16 : 8)];
    if (NORM == 1) {
        const float* pp = g.ss_in + (long)(lane >> 3) * g.nss_in + (lane & 7) * per;
#pragma unroll
        for (int i = 0; i < 8; ++i) pv[i] = *reinterpret_cast<const f32x4*>(pp + (4 * i < per ? 4 * i : 0));
    }
    float rstd = 1.f;

    if (WIDE != 3 && rounds == 1) {
        int st[NL];
#pragma unroll
        for (int u = 0; u < NL; ++u)      // MODE 0: a wave takes both 64-byte halves of a 128-byte line back to back;
            st[u] = PK ? wave * NL + u            // packed weights: NL consecutive KiB blocks per wave and tile
                             : (MODE ? wave + NW * u : 2 * (wave + NW * (u >> 1)) + (u & 1));
        long so[NL];
#pragma unroll
        for (int u = 0; u < NL; ++u) so[u] = FAST ? (long)(u * KS) : (long)(st[u] < nsteps ? st[u] : nsteps - 1) * KS;
        if (FAST) xp += (unsigned)(wave * (NL * KS));
        // request order = arrival order (one in-order counter per wave): statistics, activations, norm weights, then
        // the weight tile, so that the normalisation below runs while the weights are still in flight
        // (X2LATE — 32 rows on 16 waves, 128 registers per lane: the fragments of rows 16 .. 31 take the registers of rows 0 .. 15
        //  once the first half's MFMAs have read them; that form runs one tile per workgroup, so nothing is re-read)
        constexpr bool X2LATE = W32 && NW == 16;
        u32x4 w0[NLW], w1[NLW], x[NL], nv[NL], x2[(W32 && !X2LATE) ? NL : 1];
        f32x4 sc0 = {1.f, 1.f, 1.f, 1.f}, sc1 = sc0;                      // F8: scales of the four weight rows behind this lane's products
#pragma unroll
        for (int u = 0; u < NL; ++u) x[u] = ld16(xp + so[u]);
        if (NORM == 1) {
#pragma unroll
            for (int u = 0; u < NL; ++u) nv[u] = ld16(g.nw + koff + so[u]);
        }
        // packed: lane l's 16 bytes of (tile, step) sit at ((tile * nsteps + step) * 64 + l) * 8 — one contiguous KiB per
        // wave-instruction (full 128-byte lines) instead of 16 row segments of 64 bytes
        long wo[NLW];
#pragma unroll
        for (int u = 0; u < NLW; ++u) wo[u] = FAST ? (long)(u * 512) : (PK ? (long)(st[u] < nsteps ? st[u] : nsteps - 1) * 512 : so[u]);
        const unsigned wlane = (unsigned)(wave * (NLW * 512) + lane * 8);         // FAST: the lane's offset inside every tile
        // F8: the row scales of tile t, requested by every wave with the tile's weights (no branch around a load; one KiB line
        // shared by the workgroup) — lane (fr, fq) holds the products of weight rows (4 fq + r) & (NCOL - 1)
        auto scale_of = [&](int t) -> f32x4 {
            return *reinterpret_cast<const f32x4*>(g.wscale + (unsigned)(t * NCOL + ((4 * fq) & (NCOL - 1))));
        };
        auto tile_base = [&](int t) -> const bf16_t* {
            if (FAST) return g.W + (long)t * (NW * NLW * 512) + wlane;          // scalar base + 32-bit lane offset (+ immediates)
            if (PK) return g.W + (long)t * nsteps * 512 + lane * 8;
            int rnn = t * NCOL + lrow; rnn = rnn < g.N ? rnn : g.N - 1;
            return g.W + (long)rnn * g.ldw + koff;
        };
        wp = tile_base(tile);
#pragma unroll
        for (int u = 0; u < NLW; ++u) {
            w0[u] = ld16_nt(wp + wo[u]);
            // (32 rows: under the higher register pressure the scheduler otherwise forms the bases of the requests past the
            //  4 KiB immediate range first — 7 - 8 instructions in front of the first request)
            if (W32 && u == 0) sched_fence();
        }
        const bf16_t* xp2 = xp;
        if constexpr (W32) {
            sched_fence();                // the weight requests are out: now the second half's activations
            xp2 = x2_ptr();
            if (FAST) xp2 += (unsigned)(wave * (NL * KS));
            if constexpr (!X2LATE) {
#pragma unroll
                for (int u = 0; u < NL; ++u) x2[u] = ld16(xp2 + so[u]);
            }
            if (!FAST && !ACT && !OUTF32 && g.res) resv2 = ld8(g.res + (long)(em2_row() + 16) * g.ldres + en);
        }
        if (F8) {
            sched_fence();                // the weight requests go out before anything waits for the scale pointer (argument segment)
            sc0 = scale_of(tile);
        }
        if (FAST && !ACT && !OUTF32) {            // needed last (epilogue of the first tile), requested last; no branch around the load
            const bf16_t* rp = g.res ? g.res : g.x;
            const unsigned ro = g.res ? dg2_mul24(em, (int)g.ldres) + (unsigned)en : 0u;
            resv = ld8(rp + ro);
            if (W32) resv2 = ld8(rp + (g.res ? dg2_mul24(em2_row() + 16, (int)g.ldres) + (unsigned)en : 0u));
        }
        sched_fence();                    // every request above is in flight before the first dependent instruction
        if (!FAST) dg2_stamp(g, 1);
        // folded norm: wave 0 requests the statistics partials behind its weights — all of them, unconditionally (a load that
        // sits under a uniform `4 i < per` test is issued and awaited one at a time: eight serial round trips on the wave
        // that every other wave then waits for at the first barrier) — and folds them in the shadow of the first tile's MFMAs
        // (fp8 weights, 16 rows on 16 waves, 128 registers per lane: waves 0 and 1 fold eight rows each, as the 32-row form's waves
        //  0 .. 3 do — the same partials in the same order per row, so the same rstd — and nothing spills)
        constexpr bool FOLD2 = F8 && WIDE == 1 && NW == 16;
        constexpr int NPASS = (WIDE == 1 && !FOLD2) ? 2 : 1;          // (32 rows: waves 0 .. 3 fold eight rows each — 32 registers instead of 64)
        f32x4 sq[NPASS][8];
        const int swave = W32 ? 4 : (FOLD2 ? 2 : 1), sbase = (W32 || FOLD2) ? 8 * wave : 0;
        if (NORM == 2 && wave < swave) {
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass) {
                const int srow = (lane >> 3) + 8 * pass + sbase;                            // (rows past M fold row M - 1 again)
                const int sr = srow < g.M ? srow : g.M - 1;
                const float* pp = FAST ? g.ss_in + (dg2_mul24(sr, g.nss_in) + (unsigned)((lane & 7) * per))
                                       : g.ss_in + (long)sr * g.nss_in + (lane & 7) * per;
#pragma unroll
                for (int i = 0; i < 8; ++i) sq[pass][i] = *reinterpret_cast<const f32x4*>(pp + (4 * i < per ? 4 * i : 0));
            }
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass)
#pragma unroll
                for (int i = 0; i < 8; ++i) reg_fence(sq[pass][i]);
        }
        auto fold_stats = [&]() {
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass) {
                const int srow = (lane >> 3) + 8 * pass + sbase;
                const float rs = dg2_fold_rstd(sq[pass], per, g.inv_K, g.eps);
                if ((lane & 7) == 0) rs_lds[srow] = rs;       // visible after the tile barrier
            }
        };
        if (NORM == 1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) reg_fence(pv[i]);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s += 4 * i < per ? (pv[i][0] + pv[i][1]) + (pv[i][2] + pv[i][3]) : 0.f;
            s += wave_shfl_xor(s, 1); s += wave_shfl_xor(s, 2); s += wave_shfl_xor(s, 4);
            rstd = rsqrtf(wave_shfl(s, xr * 8) / (float)g.K + g.eps);
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                float xf[8], nf[8];
                unpack8(x[u], xf); unpack8(nv[u], nf);
#pragma unroll
                for (int i = 0; i < 8; ++i) xf[i] = nf[i] * round_bf(xf[i] * rstd);
                x[u] = pack8(xf);
            }
        }
#pragma unroll
        for (int u = 0; u < NL; ++u) if (!FAST && st[u] >= nsteps) x[u] = zero4;        // steps past K contribute zero
        if constexpr (W32 && !X2LATE) {
#pragma unroll
            for (int u = 0; u < NL; ++u) if (!FAST && st[u] >= nsteps) x2[u] = zero4;
        }
        // weight registers ping-pong (w0 / w1): tile i+1 is requested before tile i is multiplied.  The requests sit
        // in straight-line code (no branch around a load: the compiler would wait for them at the join), so the last
        // one or two tiles are peeled.
        const int G = (int)gridDim.x;
        const int nmine = (ntiles - tile + G - 1) / G;
        auto issue = [&](u32x4 (&wn)[NLW], f32x4& scn, int t) {
            const bf16_t* wpn = tile_base(t);
#pragma unroll
            for (int u = 0; u < NLW; ++u) wn[u] = ld16_nt(wpn + wo[u]);
            if (F8) scn = scale_of(t);
        };
        auto compute = [&](u32x4 (&wc)[NLW], const f32x4& scc, int t, int it) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
            if constexpr (F8 != 0 && W32 && !X2LATE) {
                // 32 rows: a fragment is decoded once and multiplied against both row halves; each accumulator sees the k-steps in the
                // 16-row form's order
#pragma unroll
                for (int u = 0; u < NLW; ++u) {
                    const u32x4 lo = f8x8_to_bf16x8(wc[u].x, wc[u].y), hi = f8x8_to_bf16x8(wc[u].z, wc[u].w);
                    acc = mfma_16x16x32(lo, x[2 * u], acc);
                    acc2 = mfma_16x16x32(lo, x2[2 * u], acc2);
                    acc = mfma_16x16x32(hi, x[2 * u + 1], acc);
                    acc2 = mfma_16x16x32(hi, x2[2 * u + 1], acc2);
                }
            } else if constexpr (F8 != 0) {
#pragma unroll
                for (int u = 0; u < NLW; ++u) {
                    acc = mfma_16x16x32(f8x8_to_bf16x8(wc[u].x, wc[u].y), x[2 * u], acc);
                    acc = mfma_16x16x32(f8x8_to_bf16x8(wc[u].z, wc[u].w), x[2 * u + 1], acc);
                }
            } else {
#pragma unroll
                for (int u = 0; u < NL; ++u) acc = mfma_16x16x32(wc[u], x[u], acc);
            }
            if constexpr (F8 != 0 && X2LATE) {
                // 16 waves, 128 registers per lane: rows 16 .. 31 take the registers of rows 0 .. 15 and the fragments are decoded again
                // (4 VALU instructions per k-step, behind the weight stream)
                sched_fence();
#pragma unroll
                for (int u = 0; u < NL; ++u) x[u] = ld16(xp2 + so[u]);
#pragma unroll
                for (int u = 0; u < NLW; ++u) {
                    acc2 = mfma_16x16x32(f8x8_to_bf16x8(wc[u].x, wc[u].y), x[2 * u], acc2);
                    acc2 = mfma_16x16x32(f8x8_to_bf16x8(wc[u].z, wc[u].w), x[2 * u + 1], acc2);
                }
            } else if constexpr (F8 != 0) {
                // (8 and 16 rows: one half; 32 rows: both chains above)
            } else if constexpr (X2LATE) {
                sched_fence();
#pragma unroll
                for (int u = 0; u < NL; ++u) x[u] = ld16(xp2 + so[u]);
#pragma unroll
                for (int u = 0; u < NL; ++u) if (!FAST && st[u] >= nsteps) x[u] = zero4;
#pragma unroll
                for (int u = 0; u < NL; ++u) acc2 = mfma_16x16x32(wc[u], x[u], acc2);
            } else if constexpr (W32) {
#pragma unroll
                for (int u = 0; u < NL; ++u) acc2 = mfma_16x16x32(wc[u], x2[u], acc2);
            }
            if (NORM == 2 && it == 0 && wave < swave) fold_stats();
            float (*slab)[64][4] = red[NBUF == 2 ? it & 1 : 0];
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[wave][lane][r] = acc[r];
            if constexpr (W32) {
#pragma unroll
                for (int r = 0; r < 4; ++r) slab[NW + wave][lane][r] = acc2[r];
            }
            if (!FAST && it == 0) dg2_stamp(g, 2);
            __syncthreads();
            if (!FAST && it == 0) dg2_stamp(g, 3);
            if (wave == it % NW) {
                float v[4];
                dg2_reduce<NW>(slab, lane, v);
                if (NORM == 2) {
                    const int mrow = MODE ? (fr & 7) : fr;                   // batch row of this lane's products (both K-halves of MODE 1)
                    const float rsf = rs_lds[mrow < g.M ? mrow : g.M - 1];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] *= rsf;
                }
                if (F8) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] *= scc[r];
                }
                dg2_epilogue<MODE, ACT, OUTF32, PK>(g, v, t, lane, it == 0, resv);
            }
            if constexpr (W32) {
                if (wave == (it + 1) % NW) {          // rows 16 .. 31: the same reduction and epilogue, on the next wave
                    float v[4];
                    dg2_reduce<NW>(slab + NW, lane, v);
                    if (NORM == 2) {
                        const float rsf = rs_lds[16 + em2_row()];
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] *= rsf;
                    }
                    if (F8) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] *= scc[r];
                    }
                    const DecGemm2Args g2 = second_half();
                    dg2_epilogue<MODE, ACT, OUTF32, PK>(g2, v, t, lane, it == 0, resv2);
                }
            }
            if (!FAST && it == 0) dg2_stamp(g, 4);
        };
        if (NW == 16) {                   // 16 waves x 12 chunks: no registers for a second weight set; the host launches one
            compute(w0, sc0, tile, 0);    // workgroup per tile (dg2_form_of)
            return;
        }
        int it = 0;
        for (; it + 2 < nmine; it += 2) {
            issue(w1, sc1, tile + (it + 1) * G); compute(w0, sc0, tile + it * G, it);
            issue(w0, sc0, tile + (it + 2) * G); compute(w1, sc1, tile + (it + 1) * G, it + 1);
        }
        if (nmine - it == 2) {
            issue(w1, sc1, tile + (it + 1) * G); compute(w0, sc0, tile + it * G, it);
            compute(w1, sc1, tile + (it + 1) * G, it + 1);
        } else {
            compute(w0, sc0, tile + it * G, it);
        }
        return;
    }

    if constexpr (WIDE == 2) return;      // (32 rows: the host launches the multi-round loop as its own kernel, WIDE == 3)
    // K larger than one register round (NW * NL steps): one tile per iteration, fragments re-read every round
    // (32 rows on 16 waves, 128 registers per lane: the fragments of rows 16 .. 31 take the registers of rows 0 .. 15 once the round's
    //  first-half MFMAs have read them, as in the single-round form; x is re-read every round here anyway)
    constexpr bool X2LATE_MR = W32 && NW == 16;
    for (int it = 0; tile < ntiles; ++it, tile += (int)gridDim.x) {
        rn = tile * NCOL + lrow; rn = rn < g.N ? rn : g.N - 1;
        wp = g.W + (long)rn * g.ldw + koff;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = acc;
        for (int rd = 0; rd < rounds; ++rd) {
            const int base = rd * NW * NL;
            int st[NL];
#pragma unroll
            for (int u = 0; u < NL; ++u) st[u] = base + (MODE ? wave + NW * u : 2 * (wave + NW * (u >> 1)) + (u & 1));
            u32x4 w[NL], x[NL], nv[NL], x2[(W32 && !X2LATE_MR) ? NL : 1];
            // (packed weights: chunk ((tile * nsteps + step) * 64 + lane) holds the lane's 8 elements of (tile, step) — K beyond one
            //  register round, e.g. Qwen3-4B's o / down projections, walks the same image round by round)
            const bf16_t* wpk = g.W + ((long)tile * nsteps * 64 + lane) * 8;
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                const int sc = st[u] < nsteps ? st[u] : nsteps - 1;
                w[u] = PK ? ld16_nt(wpk + (long)sc * 512) : ld16_nt(wp + (long)sc * KS);
            }
#pragma unroll
            for (int u = 0; u < NL; ++u) { const int sc = st[u] < nsteps ? st[u] : nsteps - 1; x[u] = ld16(xp + (long)sc * KS); }
            const bf16_t* xp2 = xp;
            if constexpr (W32) {
                sched_fence();            // weights and first-half activations are requested: now what the second half needs
                xp2 = x2_ptr();
                if (it == 0 && rd == 0 && !ACT && !OUTF32 && g.res) resv2 = ld8(g.res + (long)(em2_row() + 16) * g.ldres + en);
                if constexpr (!X2LATE_MR) {
#pragma unroll
                    for (int u = 0; u < NL; ++u) { const int sc = st[u] < nsteps ? st[u] : nsteps - 1; x2[u] = ld16(xp2 + (long)sc * KS); }
                }
            }
            if (NORM == 1) {
#pragma unroll
                for (int u = 0; u < NL; ++u) { const int sc = st[u] < nsteps ? st[u] : nsteps - 1; nv[u] = ld16(g.nw + koff + (long)sc * KS); }
                if (it == 0 && rd == 0) {
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) s += 4 * i < per ? (pv[i][0] + pv[i][1]) + (pv[i][2] + pv[i][3]) : 0.f;
                    s += wave_shfl_xor(s, 1); s += wave_shfl_xor(s, 2); s += wave_shfl_xor(s, 4);
                    rstd = rsqrtf(wave_shfl(s, xr * 8) / (float)g.K + g.eps);
                }
#pragma unroll
                for (int u = 0; u < NL; ++u) {
                    float xf[8], nf[8];
                    unpack8(x[u], xf); unpack8(nv[u], nf);
#pragma unroll
                    for (int i = 0; i < 8; ++i) xf[i] = nf[i] * round_bf(xf[i] * rstd);
                    x[u] = pack8(xf);
                }
            }
#pragma unroll
            for (int u = 0; u < NL; ++u) acc = mfma_16x16x32(st[u] < nsteps ? w[u] : zero4, x[u], acc);
            if constexpr (X2LATE_MR) {
                sched_fence();
#pragma unroll
                for (int u = 0; u < NL; ++u) { const int sc = st[u] < nsteps ? st[u] : nsteps - 1; x[u] = ld16(xp2 + (long)sc * KS); }
#pragma unroll
                for (int u = 0; u < NL; ++u) acc2 = mfma_16x16x32(st[u] < nsteps ? w[u] : zero4, x[u], acc2);
            } else if constexpr (W32) {
#pragma unroll
                for (int u = 0; u < NL; ++u) acc2 = mfma_16x16x32(st[u] < nsteps ? w[u] : zero4, x2[u], acc2);
            }
        }
        float (*slab)[64][4] = red[NBUF == 2 ? it & 1 : 0];
#pragma unroll
        for (int r = 0; r < 4; ++r) slab[wave][lane][r] = acc[r];
        if constexpr (W32) {
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[NW + wave][lane][r] = acc2[r];
        }
        __syncthreads();
        if (wave == it % NW) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = 0.f;
#pragma unroll
                for (int wv = 0; wv < NW; ++wv) s += slab[wv][lane][r];
                v[r] = s;
            }
            dg2_epilogue<MODE, ACT, OUTF32>(g, v, tile, lane, it == 0, resv);
        }
        if constexpr (W32) {
            if (wave == (it + 1) % NW) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = 0.f;
#pragma unroll
                    for (int wv = 0; wv < NW; ++wv) s += slab[NW + wv][lane][r];
                    v[r] = s;
                }
                const DecGemm2Args g2 = second_half();
                dg2_epilogue<MODE, ACT, OUTF32>(g2, v, tile, lane, it == 0, resv2);
            }
            if (NBUF == 1) __syncthreads();           // one slab: the next tile's partial products wait for this tile's readers
        }
    }
}

// sums of squares of the rows of x [M <= 32, K] (after the embedding gather): ss[r][0] = sum, ss[r][1 .. nss) = 0
__global__ __launch_bounds__(256) void row_sumsq_kernel(const bf16_t* x, long ldx, int K, float* ss, int nss) {
    __shared__ float part[4];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    float s = 0.f;
    for (int j = tid; j < K / 8; j += 256) {
        float f[8];
        unpack8(ld16(x + (long)r * ldx + j * 8), f);
#pragma unroll
        for (int i = 0; i < 8; ++i) s += f[i] * f[i];
    }
    s = wave_sum<64>(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    for (int j = tid; j < nss; j += 256) ss[(long)r * nss + j] = j == 0 ? (part[0] + part[1]) + (part[2] + part[3]) : 0.f;
}

// W [N, K] row-major -> fragment order of dec_gemm2_kernel<MODE>: chunk ((tile * nsteps + step) * 64 + lane) holds the 8
// elements lane (fr, fq) feeds to the MFMA of (tile, step).  One thread per 16-byte chunk, coalesced on the write side.
template <int MODE>
__global__ __launch_bounds__(256) void dec_pack_kernel(const bf16_t* W, long ldw, int N, int K, const bf16_t* nw, bf16_t* out) {
    constexpr int KS = MODE ? 64 : 32, NCOL = MODE ? 8 : 16;
    const int nsteps = K / KS;
    const long nchunk = (long)(N / NCOL) * nsteps * 64;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunk) return;
    const int lane = (int)(c & 63);
    const long ts = c >> 6;
    const int step = (int)(ts % nsteps), tile = (int)(ts / nsteps);
    const int fr = lane & 15, fq = lane >> 4;
    const int row = tile * NCOL + (MODE ? (fr & 7) : fr);
    const int col = step * KS + (MODE ? ((fr >> 3) * 32 + fq * 8) : fq * 8);
    u32x4 v = ld16(W + (long)row * ldw + col);
    if (nw) {                                 // fold the RMSNorm weight of the projection's input: W[n, k] * nw[k], one rounding
        float f[8], s[8];
        unpack8(v, f); unpack8(ld16(nw + col), s);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] *= s[i];
        v = pack8(f);
    }
    st16(out + c * 8, v);
}

// fp8 image of a projection (BASELINE config 5: "fp8 weights"): scale[n] = max_k |W[n, k] nw[k]| / 448 (the e4m3
// maximum; 1 for an all-zero row), q[n, k] = e4m3(W[n, k] nw[k] / scale[n]) rounded to nearest even.  One wave per row.
__global__ __launch_bounds__(256) void dec_rowscale_fp8_kernel(const bf16_t* W, long ldw, int N, int K, const bf16_t* nw, float* scale) {
    const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (row >= N) return;
    float mx = 0.f;
    for (int j = lane; j < K / 8; j += 64) {
        float f[8], s[8];
        unpack8(ld16(W + (long)row * ldw + j * 8), f);
        if (nw) { unpack8(ld16(nw + j * 8), s);
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] *= s[i]; }
#pragma unroll
        for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(f[i]));
    }
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, wave_shfl_xor(mx, m));
    if (lane == 0) scale[row] = mx > 0.f ? mx * (1.0f / 448.0f) : 1.0f;
}

// fragment order of dec_gemm2_kernel<.., F8 = 1>: 16-byte chunk ((tile * nsteps / 2 + s2) * 64 + lane) = the lane's 8 elements of
// k-step 2 s2 followed by its 8 elements of k-step 2 s2 + 1, one byte each.  One thread per chunk.
template <int MODE>
__global__ __launch_bounds__(256) void dec_pack_fp8_kernel(const bf16_t* W, long ldw, int N, int K, const bf16_t* nw, const float* scale,
                                                           unsigned* out) {
    constexpr int KS = MODE ? 64 : 32, NCOL = MODE ? 8 : 16;
    const int npair = K / KS / 2;
    const long nchunk = (long)(N / NCOL) * npair * 64;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunk) return;
    const int lane = (int)(c & 63);
    const long ts = c >> 6;
    const int s2 = (int)(ts % npair), tile = (int)(ts / npair);
    const int fr = lane & 15, fq = lane >> 4;
    const int row = tile * NCOL + (MODE ? (fr & 7) : fr);
    const float inv = 1.0f / scale[row];
    unsigned o[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int col = (2 * s2 + h) * KS + (MODE ? ((fr >> 3) * 32 + fq * 8) : fq * 8);
        float f[8];
        unpack8(ld16(W + (long)row * ldw + col), f);
        if (nw) { float s[8]; unpack8(ld16(nw + col), s);
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] *= s[i]; }
        unsigned b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = f32_to_e4m3(f[i] * inv);
        o[2 * h] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        o[2 * h + 1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    }
    u32x4 v = {o[0], o[1], o[2], o[3]};
    *reinterpret_cast<u32x4*>(out + c * 4) = v;
}

// One slot per value of the form's ten fields: the launcher of the kernel at slot I, or null where dg2_kernel_exists says there is none
// (nothing is instantiated there).
using Dg2Launch = int (*)(const DecGemm2Args&, int, bra_stream_t);
constexpr int DG2_SLOTS = 2 * 3 * 2 * 2 * 8 * 4 * 2 * 2 * 2;
constexpr Dg2Form dg2_form_at(int i) {
    Dg2Form f = {};
    f.f8 = i % 2; i /= 2; f.fast = i % 2; i /= 2; f.pk = i % 2; i /= 2; f.wide = i % 4; i /= 4;
    f.nw = DG2_SHAPES[i % 8][0]; f.nl = DG2_SHAPES[i % 8][1]; i /= 8;
    f.outf32 = i % 2; i /= 2; f.act = i % 2; i /= 2; f.norm = i % 3; f.mode = i / 3;
    return f;
}
constexpr int dg2_slot(const Dg2Form& f) {        // (of a form that exists)
    int s = 0;
    while (DG2_SHAPES[s][0] != f.nw || DG2_SHAPES[s][1] != f.nl) ++s;
    return (((((((f.mode * 3 + f.norm) * 2 + f.act) * 2 + f.outf32) * 8 + s) * 4 + f.wide) * 2 + f.pk) * 2 + f.fast) * 2 + f.f8;
}
template <int I>
static int dg2_launch_at(const DecGemm2Args& g, int grid, bra_stream_t st) {
    constexpr Dg2Form f = dg2_form_at(I);
    static_assert(dg2_slot(f) == I, "dg2_slot inverts dg2_form_at");
    BRA_LAUNCH((dec_gemm2_kernel<f.mode, f.norm, f.act, f.outf32, f.nw, f.nl, f.wide, f.pk, f.fast, f.f8>), dim3(grid), dim3(f.nw * 64), 0, st,
               BRA_DG2_HEAD_ARGS(g), g);
    return BRA_LAUNCH_STATUS();
}
template <int I>
constexpr Dg2Launch dg2_launcher() {
    if constexpr (dg2_kernel_exists(dg2_form_at(I))) return &dg2_launch_at<I>;
    else return nullptr;
}
template <int... I>
constexpr std::array<Dg2Launch, sizeof...(I)> dg2_launchers(std::integer_sequence<int, I...>) { return {{dg2_launcher<I>()...}}; }
static constexpr auto DG2_TABLE = dg2_launchers(std::make_integer_sequence<int, DG2_SLOTS>{});

static int launch_dg2(const Dg2Call& c, const DecGemm2Args& g, bra_stream_t st) {
    Dg2Form f;
    int grid;
    const int rc = dg2_form_of(c, f, grid);
    return rc ? rc : DG2_TABLE[dg2_slot(f)](g, grid, st);
}

}  // namespace bra

using namespace bra;

static int dec_gemm2_any(const void* x, long ldx, const float* ss_in, int nss_in, const void* norm_w, float eps,
                        const void* W, long ldw, const void* res, long ldres, void* out, long ldo, float* ss_out,
                        int nss_out, int M, int N, int K, int act, int out_f32, int packed, void* probe, void* stream,
                        const float* wscale = nullptr);

extern "C" int bra_dec_gemm2(const void* x, long ldx, const float* ss_in, int nss_in, const void* norm_w, float eps,
                             const void* W, long ldw, const void* res, long ldres, void* out, long ldo, float* ss_out,
                             int nss_out, int M, int N, int K, int act, int out_f32, void* stream) {
    return dec_gemm2_any(x, ldx, ss_in, nss_in, norm_w, eps, W, ldw, res, ldres, out, ldo, ss_out, nss_out, M, N, K, act, out_f32,
                         0, nullptr, stream);
}

extern "C" int bra_dec_gemm2_packed(const void* x, long ldx, const float* ss_in, int nss_in, const void* norm_w, float eps,
                                    const void* W, long ldw, const void* res, long ldres, void* out, long ldo, float* ss_out,
                                    int nss_out, int M, int N, int K, int act, int out_f32, int packed, void* stream) {
    return dec_gemm2_any(x, ldx, ss_in, nss_in, norm_w, eps, W, ldw, res, ldres, out, ldo, ss_out, nss_out, M, N, K, act, out_f32,
                         packed, nullptr, stream);
}

// fp8 (e4m3) weights with one fp32 scale per output row (bra_dec_pack_weights_fp8): y = rstd * scale[n] * (x Wq^T) ... — the same
// epilogues as bra_dec_gemm2_packed.  `norm_folded` != 0: ss_in / nss_in carry the statistics of x and the norm weight was folded
// into Wq before quantisation.  BRA_ERR_UNSUPPORTED outside the single-register-round shapes (the caller keeps bf16 weights there).
// `image_rows`: the row class the image was packed for (bra_dec_pack_weights_fp8_rows) — 8 streams against M <= 8, 16 (16-column tiles
// for every projection) against 9 <= M <= 16, 32 the SAME rows = 16 image against 17 <= M <= 32 (each request feeds both 16-row halves;
// where bra_dec_gemm2_fp8_rows32_ok says so); any other pairing is BRA_ERR_UNSUPPORTED.
extern "C" int bra_dec_gemm2_fp8_rows(const void* x, long ldx, const float* ss_in, int nss_in, float eps, const void* Wq, const float* wscale,
                                      const void* res, long ldres, void* out, long ldo, float* ss_out, int nss_out, int M, int N, int K,
                                      int act, int out_f32, int norm_folded, int image_rows, void* stream) {
    if (!Wq || !wscale) return BRA_ERR_ARG;
    if (M > 32 || image_rows != dg2_row_class(M)) return BRA_ERR_UNSUPPORTED;
    // (norm_w only selects the folded-norm form here: its values are never read when the weights carry it)
    return dec_gemm2_any(x, ldx, norm_folded ? ss_in : nullptr, norm_folded ? nss_in : 0, norm_folded ? Wq : nullptr, eps, Wq, K, res, ldres,
                         out, ldo, ss_out, nss_out, M, N, K, act, out_f32, norm_folded ? 3 : 1, nullptr, stream, wscale);
}

extern "C" int bra_dec_gemm2_fp8(const void* x, long ldx, const float* ss_in, int nss_in, float eps, const void* Wq, const float* wscale,
                                 const void* res, long ldres, void* out, long ldo, float* ss_out, int nss_out, int M, int N, int K,
                                 int act, int out_f32, int norm_folded, void* stream) {
    return bra_dec_gemm2_fp8_rows(x, ldx, ss_in, nss_in, eps, Wq, wscale, res, ldres, out, ldo, ss_out, nss_out, M, N, K, act, out_f32,
                                  norm_folded, 8, stream);
}

#ifdef BRA_DEBUG
extern "C" int bra_dec_gemm2_probe(const void* x, long ldx, const float* ss_in, int nss_in, const void* norm_w, float eps,
                                   const void* W, long ldw, const void* res, long ldres, void* out, long ldo, float* ss_out,
                                   int nss_out, int M, int N, int K, int act, int out_f32, int packed, void* probe, void* stream) {
    return dec_gemm2_any(x, ldx, ss_in, nss_in, norm_w, eps, W, ldw, res, ldres, out, ldo, ss_out, nss_out, M, N, K, act, out_f32,
                         packed, probe, stream);
}
#endif

static int dec_gemm2_any(const void* x, long ldx, const float* ss_in, int nss_in, const void* norm_w, float eps,
                        const void* W, long ldw, const void* res, long ldres, void* out, long ldo, float* ss_out,
                        int nss_out, int M, int N, int K, int act, int out_f32, int packed, void* probe, void* stream,
                        const float* wscale) {
    // fp8 weights: the entry point pairs the row class of the image with M; packed, norm folded or absent
    if (wscale && (!(packed & 1) || (norm_w && !(packed & 2)))) return BRA_ERR_UNSUPPORTED;
    if (M <= 0 || M > 32 || N <= 0 || K <= 0 || K % 32 || ldx % 8 || ldw % 8 || !x || !W || !out) return BRA_ERR_ARG;
    if (act && (N % 16 || out_f32 || res || ss_out)) return BRA_ERR_ARG;
    if (out_f32 && res) return BRA_ERR_ARG;            // (out_f32 with ss_out: per-tile maxima of the logits, 16-column tiles)
    if (norm_w && (!ss_in || nss_in < 32 || nss_in % 32 || nss_in > 256)) return BRA_ERR_ARG;
    if (res && ldres % 4) return BRA_ERR_ARG;
    const bool diag = dg2_diag(dg2_row_class(M), N, K, act, out_f32);
    if (ss_out && nss_out < (diag ? N / 8 : (N + 15) / 16)) return BRA_ERR_ARG;
    DecGemm2Args g = {(const bf16_t*)x, ldx, ss_in, nss_in, (const bf16_t*)norm_w, eps, (const bf16_t*)W, ldw,
                      (const bf16_t*)res, ldres, out, ldo, ss_out, nss_out, M, N, K, packed, wscale, BRA_DBG_INIT((unsigned long long*)probe) 1.f / (float)K};
    if (packed && (N % (diag ? 8 : 16) || K % (diag ? 64 : 32))) return BRA_ERR_ARG;
    if ((packed & 2) && !(packed & 1)) return BRA_ERR_ARG;
    // what is left to refuse is BRA_ERR_UNSUPPORTED: the call has no kernel (dg2_form_of)
    return launch_dg2({M, N, K, act, out_f32, norm_w != nullptr, packed, wscale != nullptr, ldx, ldres, nss_in, probe != nullptr}, g, (bra_stream_t)stream);
}

extern "C" int bra_dec_pack_weights_rows(const void* W, long ldw, int N, int K, int act, int out_f32, const void* norm_w, int rows,
                                         void* out, void* stream);
extern "C" int bra_dec_pack_weights(const void* W, long ldw, int N, int K, int act, int out_f32, const void* norm_w, void* out,
                                    void* stream) {
    return bra_dec_pack_weights_rows(W, ldw, N, K, act, out_f32, norm_w, 8, out, stream);
}

// rows = batch rows the copy will be streamed against: more than 8 selects the 16-column tile order for every projection
extern "C" int bra_dec_pack_weights_rows(const void* W, long ldw, int N, int K, int act, int out_f32, const void* norm_w, int rows,
                                         void* out, void* stream) {
    if (!W || !out || N <= 0 || K <= 0 || ldw % 8 || rows <= 0 || rows > 16) return BRA_ERR_ARG;
    const bool diag = dg2_diag(rows, N, K, act, out_f32);
    if (N % (diag ? 8 : 16) || K % (diag ? 64 : 32)) return BRA_ERR_UNSUPPORTED;
    const long nchunk = (long)N * K / 8;
    const dim3 grid((unsigned)((nchunk + 255) / 256));
    if (diag) BRA_LAUNCH((dec_pack_kernel<1>), grid, dim3(256), 0, (bra_stream_t)stream, (const bf16_t*)W, ldw, N, K, (const bf16_t*)norm_w, (bf16_t*)out);
    else BRA_LAUNCH((dec_pack_kernel<0>), grid, dim3(256), 0, (bra_stream_t)stream, (const bf16_t*)W, ldw, N, K, (const bf16_t*)norm_w, (bf16_t*)out);
    return BRA_LAUNCH_STATUS();
}

// W [N, K] bf16 (optionally with the input's RMSNorm weight folded in) -> fp8 e4m3 image in bra_dec_gemm2_fp8's fragment order
// (out_q: N * K bytes) + one fp32 scale per row (out_scale: N floats).  Same tile rule as bra_dec_pack_weights_rows: `rows` <= 8 the
// 8-row class, 9 .. 16 the 16-column tile order for every projection (same quantiser: the codes and scales of the two images are
// equal, only their order differs).  BRA_ERR_UNSUPPORTED when the shape is not a whole number of tiles and k-step pairs.
extern "C" int bra_dec_pack_weights_fp8_rows(const void* W, long ldw, int N, int K, int act, int out_f32, const void* norm_w, int rows,
                                             void* out_q, float* out_scale, void* stream) {
    if (!W || !out_q || !out_scale || N <= 0 || K <= 0 || ldw % 8 || rows <= 0 || rows > 16) return BRA_ERR_ARG;
    const bool diag = dg2_diag(rows, N, K, act, out_f32);
    if (N % (diag ? 8 : 16) || K % (diag ? 128 : 64)) return BRA_ERR_UNSUPPORTED;
    {   // only what bra_dec_gemm2_fp8_rows streams against `rows` rows
        Dg2Form f;
        int grid;
        if (dg2_form_of({rows, N, K, act, out_f32, norm_w != nullptr, norm_w ? 3 : 1, 1, K, 0, 32, 0}, f, grid)) return BRA_ERR_UNSUPPORTED;
    }
    bra_stream_t st = (bra_stream_t)stream;
    BRA_LAUNCH(dec_rowscale_fp8_kernel, dim3((N + 3) / 4), dim3(256), 0, st, (const bf16_t*)W, ldw, N, K, (const bf16_t*)norm_w, out_scale);
    int rc = BRA_LAUNCH_STATUS();
    if (rc) return rc;
    const long nchunk = (long)N * K / 16;
    const dim3 grid((unsigned)((nchunk + 255) / 256));
    if (diag) BRA_LAUNCH((dec_pack_fp8_kernel<1>), grid, dim3(256), 0, st, (const bf16_t*)W, ldw, N, K, (const bf16_t*)norm_w, out_scale, (unsigned*)out_q);
    else BRA_LAUNCH((dec_pack_fp8_kernel<0>), grid, dim3(256), 0, st, (const bf16_t*)W, ldw, N, K, (const bf16_t*)norm_w, out_scale, (unsigned*)out_q);
    return BRA_LAUNCH_STATUS();
}

extern "C" int bra_dec_pack_weights_fp8(const void* W, long ldw, int N, int K, int act, int out_f32, const void* norm_w, void* out_q,
                                        float* out_scale, void* stream) {
    return bra_dec_pack_weights_fp8_rows(W, ldw, N, K, act, out_f32, norm_w, 8, out_q, out_scale, stream);
}

// the e4m3 image of a plain projection (no norm, bf16 output) at ANY K % 64 == 0, for bra_dec_gemm2_fp8_anyk (k_decgemm8.hip): the quantiser
// and the rows = 16 order of bra_dec_pack_weights_fp8_rows without its single-round check — at a K both take, the same bytes
extern "C" int bra_dec_gemm2_fp8_anyk_ok(int N, int K);
extern "C" int bra_dec_pack_weights_fp8_anyk(const void* W, long ldw, int N, int K, void* out_q, float* out_scale, void* stream) {
    if (!W || !out_q || !out_scale || N <= 0 || K <= 0 || ldw % 8) return BRA_ERR_ARG;
    if (!bra_dec_gemm2_fp8_anyk_ok(N, K)) return BRA_ERR_UNSUPPORTED;
    bra_stream_t st = (bra_stream_t)stream;
    BRA_LAUNCH(dec_rowscale_fp8_kernel, dim3((N + 3) / 4), dim3(256), 0, st, (const bf16_t*)W, ldw, N, K, (const bf16_t*)nullptr, out_scale);
    const int rc = BRA_LAUNCH_STATUS();
    if (rc) return rc;
    const long nchunk = (long)N * K / 16;
    BRA_LAUNCH((dec_pack_fp8_kernel<0>), dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, st, (const bf16_t*)W, ldw, N, K, (const bf16_t*)nullptr,
               out_scale, (unsigned*)out_q);
    return BRA_LAUNCH_STATUS();
}

// statistics columns of a step whose hidden size is H: the workgroups of an N = H projection (one partial each), as a multiple of 32;
// 0 where that is more than the 256 a consumer folds (the step then runs the first-generation projections)
extern "C" int bra_dec_stat_cols(int H) {
    if (H <= 0) return 0;
    const int nss = ((dg2_diag_tiles(H) ? H / 8 : (H + 15) / 16) + 31) / 32 * 32;
    return nss > 256 ? 0 : nss;
}

// the form of a call (see Dg2Call; the arguments are taken as valid) without launching anything: form[10] = dec_gemm2_kernel's template
// arguments in their order, or BRA_ERR_UNSUPPORTED.  The plan queries of the 32-row class are this question at M = 32.
static int dg2_form_query(const Dg2Call& c, int* form) {
    Dg2Form f;
    int grid;
    const int rc = dg2_form_of(c, f, grid);
    if (!rc && form) { const int v[10] = {f.mode, f.norm, f.act, f.outf32, f.nw, f.nl, f.wide, f.pk, f.fast, f.f8}; for (int i = 0; i < 10; ++i) form[i] = v[i]; }
    return rc;
}
#ifdef BRA_DEBUG
extern "C" int bra_dec_gemm2_form(int M, int N, int K, int act, int out_f32, int normed, int packed, int fp8, long ldx, long ldres, int nss_in,
                                  int probed, int* form) {
    return dg2_form_query({M, N, K, act, out_f32, normed, packed, fp8, ldx, ldres, nss_in, probed}, form);
}
#endif
extern "C" int bra_dec_gemm2_rows32_ok(int K, int normed, int packed) {
    return K > 0 && K % 32 == 0 && !dg2_form_query({32, 16, K, 0, 0, normed, (packed ? 1 : 0) | (normed ? 2 : 0), 0, K, 0, 32, 0}, nullptr);
}
extern "C" int bra_dec_gemm2_fp8_rows32_ok(int K, int normed) {
    return K > 0 && K % 32 == 0 && !dg2_form_query({32, 16, K, 0, 0, normed, normed ? 3 : 1, 1, K, 0, 32, 0}, nullptr);
}

extern "C" int bra_row_sumsq(const void* x, long ldx, int M, int K, float* ss, int nss, void* stream) {
    if (M <= 0 || M > 32 || K <= 0 || K % 8 || ldx % 8 || !x || !ss || nss < 1) return BRA_ERR_ARG;
    BRA_LAUNCH(row_sumsq_kernel, dim3(M), dim3(256), 0, (bra_stream_t)stream, (const bf16_t*)x, ldx, K, ss, nss);
    return BRA_LAUNCH_STATUS();
}
