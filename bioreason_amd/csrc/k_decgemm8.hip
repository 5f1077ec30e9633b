// k_decgemm8.hip — the plain decode projection (o_proj, down_proj: no norm, no SwiGLU, bf16 output, optional residual and statistics)
// over an fp8 e4m3 image at ANY K % 64 == 0, 1 .. 32 rows.  k_decgemm.hip's e4m3 forms exist where K is exactly one register round;
// Qwen3-4B's down projection (K = 9728) and, at <= 8 rows, its o projection (K = 4096) have none and streamed bf16.  This kernel
// streams K in rounds instead.
//
// One geometry for every M: 16-column tiles, 32-deep k-steps, the rows = 16 image of bra_dec_pack_weights_fp8_rows — 16-byte chunk
// ((tile * K / 64 + pair) * 64 + lane) holds the lane's fragments of k-steps 2 pair and 2 pair + 1.  The K / 64 step pairs of a tile are
// split over the workgroup's NW waves in contiguous runs of ceil(pairs / NW); a wave walks its run in rounds of NR requests (ld16_nt),
// the next round's requests issued before the current round's MFMAs — across tile seams too: a workgroup's (tile, round) items form one
// stream.  The loads sit in straight-line code (see k_decgemm.hip's header: a load under a branch is awaited at the join), so the
// items are walked two per iteration with the tail peeled; a round that reaches past the wave's run clamps its addresses and
// multiplies zero weights.  Rows 16 .. 31 (W32) are a second accumulator fed by the same decoded fragment.  The activation fragments
// of a round travel with its weights, one round ahead of the MFMAs that read them (two register sets of each).
//
// Per output element the order of the sum is: pairs in ascending order inside a wave (k-step 2 p, then 2 p + 1), waves in ascending
// order through LDS (dg2_reduce).  Nothing in it depends on M: row r of an M = 32, an M = 16 and an M = r + 1 call are bit-identical.
#include "bra_decgemm.h"
#include "bra_api_internal.h"

namespace bra {

// waves per workgroup of a projection with `npair` step pairs, and the most workgroups it is given (one of 8 waves per CU, two of 4)
constexpr int df8_waves(int npair) { return npair >= 16 ? 8 : 4; }
constexpr int df8_grid_cap(int nw) { return nw == 4 ? 512 : 256; }
// 16-byte weight requests per lane and round: 4, or from K = 4096 on 5 where that leaves fewer empty slots in the last round of a wave's
// run (K = 9728: 19 pairs per wave, four rounds of 5 instead of five of 4) — an empty slot costs what a full one does
constexpr int df8_waste(int ppw, int nr) { return (ppw + nr - 1) / nr * nr - ppw; }
constexpr int df8_requests(int npair) {
    const int ppw = (npair + 7) / 8;
    return npair >= 64 && df8_waste(ppw, 5) < df8_waste(ppw, 4) ? 5 : 4;
}

template <int NW, int NR, int W32>
__global__ __launch_bounds__(NW * 64) void dec_f8k_kernel(DecGemm2Args g) {
    constexpr int NH = W32 ? 2 : 1;                                     // 16-row halves of the batch (slab rows [h * NW, (h + 1) * NW))
    constexpr int NBUF = NH * NW * 1024 * 2 <= 32768 ? 2 : 1;           // one slab: a second barrier per tile
    __shared__ float red[NBUF][NH * NW][64][4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int npair = g.K >> 6;
    const int ntiles = g.N >> 4;
    const int ppw = (npair + NW - 1) / NW;                              // pairs of a wave's run
    const int rounds = (ppw + NR - 1) / NR;
    const int p0 = wave * ppw;
    const int pend = p0 + ppw < npair ? p0 + ppw : npair;               // the run [p0, pend) (empty on the last waves of a short K)
    const int G = (int)gridDim.x;
    const int tile0 = (int)blockIdx.x;
    const int nmine = (ntiles - tile0 + G - 1) / G;
    const int nitems = nmine * rounds;

    // activation rows: a row past M re-reads row M - 1 and is never stored
    const int xr = fr < g.M ? fr : g.M - 1;
    const bf16_t* xp = g.x + (long)xr * g.ldx + fq * 8;
    const int xr2 = fr + 16 < g.M ? fr + 16 : g.M - 1;
    const bf16_t* xp2 = g.x + (long)xr2 * g.ldx + fq * 8;
    const unsigned char* wq = (const unsigned char*)g.W + (long)lane * 16;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // epilogue operand of the first tile, requested now (clamped address: no branch around a load)
    const int em = fr < g.M ? fr : g.M - 1;
    const int em2 = fr + 16 < g.M ? fr + 16 : g.M - 1;
    u32x2 resv = {0u, 0u}, resv2 = {0u, 0u};
    {
        const bf16_t* rp = g.res ? g.res : g.x;
        const int en = tile0 * 16 + 4 * fq;
        resv = ld8(rp + (g.res ? (long)em * g.ldres + en : 0L));
        if (W32) resv2 = ld8(rp + (g.res ? (long)em2 * g.ldres + en : 0L));
    }

    // pair of slot u in round rd of this wave (clamped to the image) and whether the slot is inside the run
    auto pair_of = [&](int rd, int u, bool& live) -> int {
        const int p = p0 + rd * NR + u;
        live = p < pend;
        return p < npair ? p : npair - 1;
    };
    auto issue = [&](u32x4 (&wn)[NR], int t, int rd) {
        const unsigned char* wt = wq + (long)t * npair * 1024;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            bool live;
            const int p = pair_of(rd, u, live);
            wn[u] = ld16_nt(wt + (long)p * 1024);
        }
    };
    auto scale_of = [&](int t) -> f32x4 { return *reinterpret_cast<const f32x4*>(g.wscale + (t * 16 + 4 * fq)); };
    auto second_half = [&]() -> DecGemm2Args {        // the record the second half's epilogue sees: the same tile, 16 rows down
        DecGemm2Args g2 = g;
        g2.M = g.M - 16;
        if (g.res) g2.res = g.res + 16 * g.ldres;
        g2.out = (void*)((bf16_t*)g.out + 16 * g.ldo);
        if (g.ss_out) g2.ss_out = g.ss_out + 16 * (long)g.nss_out;
        return g2;
    };

    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = acc;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f};
    // the activation fragments of round rd of this wave
    auto load_x = [&](u32x4 (&x)[2 * NR], u32x4 (&x2)[W32 ? 2 * NR : 1], int rd) {
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            bool live;
            const int p = pair_of(rd, u, live);
            x[2 * u] = ld16(xp + (long)p * 64);
            x[2 * u + 1] = ld16(xp + (long)p * 64 + 32);
            if constexpr (W32 != 0) {
                x2[2 * u] = ld16(xp2 + (long)p * 64);
                x2[2 * u + 1] = ld16(xp2 + (long)p * 64 + 32);
            }
        }
    };
    // item (it, rd) of this workgroup over the weights `wc` and activations `xc`; `wn` / `xn` receive the next item's requests when there is
    // one (`more`)
    auto step = [&](u32x4 (&wc)[NR], u32x4 (&xc)[2 * NR], u32x4 (&x2c)[W32 ? 2 * NR : 1], u32x4 (&wn)[NR], u32x4 (&xn)[2 * NR],
                    u32x4 (&x2n)[W32 ? 2 * NR : 1], const bool more, int it, int rd) {
        const int t = tile0 + it * G;
        bool live[NR];
#pragma unroll
        for (int u = 0; u < NR; ++u) pair_of(rd, u, live[u]);
        const f32x4 sct = scale_of(t);                                // (unconditional: no branch around a load)
        if (more) {
            const bool last = rd + 1 == rounds;
            issue(wn, last ? t + G : t, last ? 0 : rd + 1);
            load_x(xn, x2n, last ? 0 : rd + 1);
        }
        sched_fence();                    // the next round is in flight before the first dependent instruction
        if (rd == 0) { acc = {0.f, 0.f, 0.f, 0.f}; acc2 = acc; sc = sct; }
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const u32x4 w = live[u] ? wc[u] : zero4;                  // slots past the run contribute zero
            const u32x4 lo = f8x8_to_bf16x8(w.x, w.y), hi = f8x8_to_bf16x8(w.z, w.w);
            acc = mfma_16x16x32(lo, xc[2 * u], acc);
            if constexpr (W32 != 0) acc2 = mfma_16x16x32(lo, x2c[2 * u], acc2);
            acc = mfma_16x16x32(hi, xc[2 * u + 1], acc);
            if constexpr (W32 != 0) acc2 = mfma_16x16x32(hi, x2c[2 * u + 1], acc2);
        }
        if (rd + 1 != rounds) return;
        // the tile is complete: K-reduction in wave order and epilogue, by wave it % NW (rows 16 .. 31: the next wave)
        float (*slab)[64][4] = red[NBUF == 2 ? it & 1 : 0];
#pragma unroll
        for (int r = 0; r < 4; ++r) slab[wave][lane][r] = acc[r];
        if constexpr (W32 != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[NW + wave][lane][r] = acc2[r];
        }
        __syncthreads();
        if (wave == it % NW) {
            float v[4];
            dg2_reduce<NW>(slab, lane, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= sc[r];
            dg2_epilogue<0, 0, 0>(g, v, t, lane, it == 0, resv);
        }
        if constexpr (W32 != 0) {
            if (wave == (it + 1) % NW) {
                float v[4];
                dg2_reduce<NW>(slab + NW, lane, v);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] *= sc[r];
                const DecGemm2Args g2 = second_half();
                dg2_epilogue<0, 0, 0>(g2, v, t, lane, it == 0, resv2);
            }
        }
        if (NBUF == 1) __syncthreads();               // one slab: the next tile's partial products wait for this tile's readers
    };

    u32x4 w0[NR], w1[NR], x0[2 * NR], x1[2 * NR], y0[W32 ? 2 * NR : 1], y1[W32 ? 2 * NR : 1];
    issue(w0, tile0, 0);
    load_x(x0, y0, 0);
    int it = 0, rd = 0;
    auto advance = [&]() { if (++rd == rounds) { rd = 0; ++it; } };
    int j = 0;
    for (; j + 2 < nitems; j += 2) {
        step(w0, x0, y0, w1, x1, y1, true, it, rd); advance();
        step(w1, x1, y1, w0, x0, y0, true, it, rd); advance();
    }
    if (nitems - j == 2) {
        step(w0, x0, y0, w1, x1, y1, true, it, rd); advance();
        step(w1, x1, y1, w0, x0, y0, false, it, rd);
    } else {
        step(w0, x0, y0, w1, x1, y1, false, it, rd);
    }
}

template <int NW, int NR, int W32>
static int df8_launch(const DecGemm2Args& g, int grid, bra_stream_t st) {
    BRA_LAUNCH((dec_f8k_kernel<NW, NR, W32>), dim3(grid), dim3(NW * 64), 0, st, g);
    return BRA_LAUNCH_STATUS();
}

}  // namespace bra

using namespace bra;

// THE rule of the any-K form: whole 16-column tiles and whole k-step pairs.  The packer, the launcher and the host ask here.
extern "C" int bra_dec_gemm2_fp8_anyk_ok(int N, int K) { return N > 0 && K > 0 && N % 16 == 0 && K % 64 == 0; }

extern "C" int bra_dec_gemm2_fp8_anyk(const void* x, long ldx, const void* Wq, const float* wscale, const void* res, long ldres, void* out,
                                      long ldo, float* ss_out, int nss_out, int M, int N, int K, void* stream) {
    // (argument errors as dec_gemm2_any's)
    if (!Wq || !wscale) return BRA_ERR_ARG;
    if (M <= 0 || N <= 0 || K <= 0 || K % 32 || ldx % 8 || !x || !out) return BRA_ERR_ARG;
    if (M > 32) return BRA_ERR_UNSUPPORTED;
    if (res && ldres % 4) return BRA_ERR_ARG;
    if (ss_out && nss_out < (N + 15) / 16) return BRA_ERR_ARG;
    if (!bra_dec_gemm2_fp8_anyk_ok(N, K)) return BRA_ERR_UNSUPPORTED;
    DecGemm2Args g = {(const bf16_t*)x, ldx, nullptr, 0, nullptr, 0.f, (const bf16_t*)Wq, (long)K, (const bf16_t*)res, ldres, out, ldo, ss_out,
                      nss_out, M, N, K, 1, wscale, BRA_DBG_INIT((unsigned long long*)nullptr) 1.f / (float)K};
    // a pure function of (N, K): the waves that split K and the workgroups that walk the tiles
    const int nw = df8_waves(K / 64), nr = df8_requests(K / 64), ntiles = N / 16, cap = df8_grid_cap(nw);
    const int grid = ntiles < cap ? ntiles : cap;
    bra_stream_t st = (bra_stream_t)stream;
    if (M <= 16) return nr == 5 ? df8_launch<8, 5, 0>(g, grid, st) : (nw == 8 ? df8_launch<8, 4, 0>(g, grid, st) : df8_launch<4, 4, 0>(g, grid, st));
    return nr == 5 ? df8_launch<8, 5, 1>(g, grid, st) : (nw == 8 ? df8_launch<8, 4, 1>(g, grid, st) : df8_launch<4, 4, 1>(g, grid, st));
}
