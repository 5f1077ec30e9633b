// k_pool.hip — single-query multi-head attention pooling over encoder hidden states (the DNA-only classifier's
// SelfAttentionPooling, bioreason/models/dna_only.py:8-39, with the K / V projections folded away: DESIGN.md "Attention pooling").
//   forward : score[h, l] = x_l . qt_h over the valid keys, p = softmax_l(score), pooled[h, :] = sum_l p[h, l] x_l, lse[h]
//   backward: dqt_h = sum_{n, l} p[h, l] (x_l . g_h - pooled_h . g_h) x_l          (hidden states frozen: no dx)
// One workgroup (4 waves) owns a chunk of rows of one sequence and walks it in tiles of 128 rows:
//   A  every wave scores its 32 rows on MFMA: X[32 x H] . B[H x 16], the 16 columns = 8 heads x {hi, lo} bf16 halves of the fp32
//      operand (so qt / g are not rounded to one bf16); x rows go from global memory straight into the A fragments
//   S  safe softmax of the tile against the chunk's running maximum (online softmax over the tiles of a chunk)
//   B  every thread owns 8 hidden columns and accumulates sum_l w[h, l] x_l in fp32 for the 8 heads (the tile's rows are read a
//      second time, from L2 / Infinity Cache)
// Chunks are merged by a second launch in a FIXED order: no atomics, results are bit-repeatable.
#include "bra_device.h"
#include "bra_api_internal.h"

namespace bra {

constexpr int kPoolNH = 8;         // heads of the reference's pooler (SelfAttentionPooling(num_heads=8))
constexpr int kPoolTile = 128;     // rows per tile: 4 waves x 32 rows
constexpr int kPoolThreads = 256;

// fragment-ordered bf16 image of v[8][H] (fp32) as the B operand of the score product: entry ((kb * 2 + t) * 64 + lane) holds the 8
// values v[c & 7][kb * 64 + 16 g + 8 t + j] (c = lane & 15, g = lane >> 4): their bf16 roundings for c < 8, the remainders for c >= 8
__device__ __forceinline__ void pool_build_image(const float* v, int H, char* img) {
    for (int e = (int)threadIdx.x; e < 2 * H; e += kPoolThreads) {
        const int l = e & 63, t = (e >> 6) & 1, kb = e >> 7;
        const int c = l & 15, g = l >> 4;
        const float* src = v + (size_t)(c & 7) * H + kb * 64 + 16 * g + 8 * t;
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = src[j], hi = round_bf(a);
            f[j] = c < 8 ? hi : a - hi;
        }
        st16(img + (size_t)e * 16, pack8(f));
    }
}

// acc[i][u][r] += X[row0 + 16 u + 4 g + r] . image_i[column c]   (rows past S - 1 read row S - 1: the caller masks them)
template <int NB>
__device__ __forceinline__ void pool_scores(const bf16_t* xb, long x_ss, int S, int row0, int H, const char* img,
                                            f32x4 (&acc)[NB][2]) {
    const int l = lane_id(), c = l & 15, g = l >> 4;
    const int ra = row0 + c < S ? row0 + c : S - 1, rb = row0 + 16 + c < S ? row0 + 16 + c : S - 1;
    const bf16_t* pa = xb + (long)ra * x_ss + 16 * g;
    const bf16_t* pb = xb + (long)rb * x_ss + 16 * g;
    const char* ql = img + (size_t)l * 16;
    const size_t imgsz = (size_t)H * 32;
    const int nkb = H / 64;
#pragma unroll 2
    for (int kb = 0; kb < nkb; ++kb) {
        const u32x4 a0 = ld16(pa + kb * 64), a1 = ld16(pa + kb * 64 + 8);
        const u32x4 b0 = ld16(pb + kb * 64), b1 = ld16(pb + kb * 64 + 8);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const u32x4 q0 = ld16(ql + i * imgsz + (size_t)kb * 2048), q1 = ld16(ql + i * imgsz + (size_t)kb * 2048 + 1024);
            acc[i][0] = mfma_16x16x32(a0, q0, acc[i][0]);
            acc[i][0] = mfma_16x16x32(a1, q1, acc[i][0]);
            acc[i][1] = mfma_16x16x32(b0, q0, acc[i][1]);
            acc[i][1] = mfma_16x16x32(b1, q1, acc[i][1]);
        }
    }
}

// BWD = false: partial (max, sum, sum_l p x_l) of the chunk -> part_ml [n, nsplit, 8, 2], part_acc [n, nsplit, 8, H]
// BWD = true : the chunk's share of dqt -> part_acc [n, nsplit, 8, H]   (aux = g, pooled, lse of the forward)
template <bool BWD>
__global__ __launch_bounds__(kPoolThreads) void attn_pool_kernel(const bf16_t* x, long x_sb, long x_ss, const uint8_t* mask,
                                                                 const float* qt, const float* g, const float* pooled,
                                                                 const float* lse, float* part_acc, float* part_ml, int S, int H,
                                                                 int chunk) {
    constexpr int NB = BWD ? 2 : 1;
    BRA_DYN_SMEM(smem);
    char* img = smem;                                                   // NB images of 32 H bytes; at the end [8][H] fp32
    float* sc = reinterpret_cast<float*>(smem + (size_t)NB * 32 * H);   // [NB][128][8]: scores (and x . g) -> weights
    float* small = sc + NB * kPoolTile * kPoolNH;                       // [8] rescale factors | [8] delta
    uint8_t* val = reinterpret_cast<uint8_t*>(small + 16);              // [128] row is a valid key
    const int tid = (int)threadIdx.x, w = tid >> 6, l = lane_id();
    const int b = (int)blockIdx.y, ck = (int)blockIdx.x, nsplit = (int)gridDim.x;
    const int r_begin = ck * chunk, r_end = r_begin + chunk < S ? r_begin + chunk : S;
    const bf16_t* xb = x + (long)b * x_sb;
    const uint8_t* mb = mask + (long)b * S;
    const int hs = tid >> 5, sub = tid & 31;                            // softmax step: 32 lanes per head

    pool_build_image(qt, H, img);
    float lse_h = 0.f, delta_h = 0.f;
    if (BWD) {
        const float* gb = g + (size_t)b * kPoolNH * H;
        pool_build_image(gb, H, img + (size_t)32 * H);
        const float* ph = pooled + ((size_t)b * kPoolNH + hs) * H;
        // against the g the MFMA sees (hi + lo, 16 significant bits), so that x_l . g - pooled . g = (x_l - pooled) . g cancels as it
        // must where the softmax is nearly one-hot; with the unrounded g the difference carries 2^-17 |x . g| of the rounding
        for (int d = sub; d < H; d += 32) {
            const float gv = gb[(size_t)hs * H + d], hi = round_bf(gv);
            delta_h += ph[d] * (hi + round_bf(gv - hi));
        }
        delta_h = wave_sum<32>(delta_h);
        lse_h = lse[b * kPoolNH + hs];
    }
    // accumulation step: thread = (row group, 8 columns)
    const int cpr = H / 8, ngrp = kPoolThreads / cpr, grp = tid / cpr, col = tid % cpr;
    const bool active = grp < ngrp;
    float acc[kPoolNH][8];
#pragma unroll
    for (int h = 0; h < kPoolNH; ++h)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    __syncthreads();

    for (int t0 = r_begin; t0 < r_end; t0 += kPoolTile) {
        if (tid < kPoolTile) val[tid] = (t0 + tid < r_end && mb[t0 + tid]) ? 1 : 0;
        // ---- A: scores of this wave's 32 rows (skipped when none of them is a valid key)
        const int row0 = t0 + 32 * w;
        const bool mine = l < 32 && row0 + l < r_end && mb[row0 + l];
        if (wave_ballot(mine) != 0) {
            f32x4 s[NB][2];
#pragma unroll
            for (int i = 0; i < NB; ++i) { s[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; s[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            pool_scores<NB>(xb, x_ss, S, row0, H, img, s);
            const int c = l & 15, gq = l >> 4;
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = s[i][u][r] + wave_shfl_xor(s[i][u][r], 8);        // hi + lo column of the head
                        if (c < 8) sc[(i * kPoolTile + 32 * w + 16 * u + 4 * gq + r) * kPoolNH + c] = v;
                    }
        }
        __syncthreads();
        // ---- S: weights of the tile's rows, head hs
        {
            float sv[4], mt = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = sub + 32 * i;
                sv[i] = val[rl] ? sc[rl * kPoolNH + hs] : -INFINITY;
                mt = fmaxf(mt, sv[i]);
            }
            if (!BWD) {
                mt = wave_max<32>(mt);
                const float m_new = fmaxf(m_run, mt);
                const float alpha = m_new == -INFINITY ? 1.f : __expf(m_run - m_new);     // no valid key yet: nothing to rescale
                float lt = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rl = sub + 32 * i;
                    const float p = val[rl] ? __expf(sv[i] - m_new) : 0.f;
                    sc[rl * kPoolNH + hs] = p;
                    lt += p;
                }
                lt = wave_sum<32>(lt);
                l_run = l_run * alpha + lt;
                m_run = m_new;
                if (sub == 0) small[hs] = alpha;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rl = sub + 32 * i;
                    const float dp = sc[(kPoolTile + rl) * kPoolNH + hs];
                    sc[rl * kPoolNH + hs] = val[rl] ? __expf(sv[i] - lse_h) * (dp - delta_h) : 0.f;
                }
            }
        }
        __syncthreads();
        // ---- B: acc[h][:] = alpha[h] acc[h][:] + sum over the valid rows of the tile of weight[row][h] x[row][8 col ..]
        if (active) {
            if (!BWD) {
#pragma unroll
                for (int h = 0; h < kPoolNH; ++h) {
                    const float a = small[h];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[h][j] *= a;
                }
            }
            const bf16_t* xc = xb + 8 * col;
            for (int rl0 = grp; rl0 < kPoolTile; rl0 += 4 * ngrp) {
                u32x4 v[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int rl = rl0 + u * ngrp;
                    ok[u] = rl < kPoolTile && val[rl];
                    v[u] = u32x4{0u, 0u, 0u, 0u};
                    if (ok[u]) v[u] = ld16(xc + (long)(t0 + rl) * x_ss);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!ok[u]) continue;
                    const int rl = rl0 + u * ngrp;
                    float xf[8];
                    unpack8(v[u], xf);
                    const f32x4 p0 = *reinterpret_cast<const f32x4*>(sc + rl * kPoolNH);
                    const f32x4 p1 = *reinterpret_cast<const f32x4*>(sc + rl * kPoolNH + 4);
#pragma unroll
                    for (int h = 0; h < kPoolNH; ++h) {
                        const float p = h < 4 ? p0[h & 3] : p1[h & 3];
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[h][j] += p * xf[j];
                    }
                }
            }
        }
        __syncthreads();
    }

    // row groups 1 .. ngrp - 1 are added to group 0 in order (through the image's LDS), group 0 writes the chunk's partial
    float* red = reinterpret_cast<float*>(img);
    for (int g2 = 1; g2 < ngrp; ++g2) {
        if (grp == g2)
#pragma unroll
            for (int h = 0; h < kPoolNH; ++h)
#pragma unroll
                for (int j = 0; j < 8; ++j) red[h * H + 8 * col + j] = acc[h][j];
        __syncthreads();
        if (grp == 0)
#pragma unroll
            for (int h = 0; h < kPoolNH; ++h)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[h][j] += red[h * H + 8 * col + j];
        __syncthreads();
    }
    const size_t slot = (size_t)b * nsplit + ck;
    if (grp == 0) {
        float* po = part_acc + slot * kPoolNH * H + 8 * col;
#pragma unroll
        for (int h = 0; h < kPoolNH; ++h) {
            *reinterpret_cast<f32x4*>(po + (size_t)h * H) = f32x4{acc[h][0], acc[h][1], acc[h][2], acc[h][3]};
            *reinterpret_cast<f32x4*>(po + (size_t)h * H + 4) = f32x4{acc[h][4], acc[h][5], acc[h][6], acc[h][7]};
        }
    }
    if (!BWD && sub == 0) {
        part_ml[(slot * kPoolNH + hs) * 2] = m_run;
        part_ml[(slot * kPoolNH + hs) * 2 + 1] = l_run;
    }
}

// pooled[b, h, d] = sum_c w_c acc[b, c, h, d] / sum_c w_c l_c, w_c = exp(m_c - max_c m_c), chunks in index order; lse = max + log(sum).
// A sequence without a valid key (every chunk's maximum -inf) gets NaN, as softmax over an all-masked row does in the reference.
__global__ __launch_bounds__(256) void attn_pool_merge_kernel(const float* part_acc, const float* part_ml, float* pooled, float* lse,
                                                              int nsplit, int H) {
    const int d = (int)blockIdx.x * 256 + (int)threadIdx.x, h = (int)blockIdx.y, b = (int)blockIdx.z;
    const float* ml = part_ml + ((size_t)b * nsplit * kPoolNH + h) * 2;
    float M = -INFINITY;
    for (int c = 0; c < nsplit; ++c) M = fmaxf(M, ml[(size_t)c * kPoolNH * 2]);
    const bool none = M == -INFINITY;
    float L = 0.f, a = 0.f;
    for (int c = 0; c < nsplit; ++c) {
        const float mc = ml[(size_t)c * kPoolNH * 2];
        const float wgt = (none || mc == -INFINITY) ? 0.f : __expf(mc - M);
        L += wgt * ml[(size_t)c * kPoolNH * 2 + 1];
        if (d < H) a += wgt * part_acc[(((size_t)b * nsplit + c) * kPoolNH + h) * H + d];
    }
    const float nan = __builtin_nanf("");
    if (d < H) pooled[((size_t)b * kPoolNH + h) * H + d] = none ? nan : a / L;
    if (d == 0) lse[b * kPoolNH + h] = none ? nan : M + __logf(L);
}

// out[i] = sum_p part[p][i], p in index order (4 floats per thread)
__global__ __launch_bounds__(256) void attn_pool_sum_kernel(const float* part, float* out, int nparts, int n4) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n4) return;
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < nparts; ++p) a += *reinterpret_cast<const f32x4*>(part + ((size_t)p * n4 + i) * 4);
    *reinterpret_cast<f32x4*>(out + (size_t)i * 4) = a;
}

// rows per workgroup: tiles of 128, doubled while the grid would still hold two workgroups per CU (fewer, larger partials)
static int pool_chunk(int n, int S, int chunk) {
    if (chunk > 0) return (chunk + kPoolTile - 1) / kPoolTile * kPoolTile;
    int rows = kPoolTile;
    while ((long)n * ((S + 2 * rows - 1) / (2 * rows)) >= 512) rows *= 2;
    return rows;
}

static int pool_check(const void* x, long x_sb, long x_ss, const void* mask, const void* qt, int n, int S, int H, int NH) {
    if (n < 0 || S <= 0 || H <= 0 || !x || !mask || !qt || x_ss < H || (x_ss % 8) || (x_sb % 8)) return BRA_ERR_ARG;
    if (NH != kPoolNH || H % 64 || H > 2048) return BRA_ERR_UNSUPPORTED;
    return BRA_OK;
}

}  // namespace bra

using namespace bra;

extern "C" int bra_attn_pool_nsplit(int n, int S, int chunk) {
    if (n <= 0 || S <= 0) return 0;
    const int rows = pool_chunk(n, S, chunk);
    return (S + rows - 1) / rows;
}

extern "C" int bra_attn_pool_fwd(const void* x, long x_sb, long x_ss, const void* mask, const float* qt, float* pooled, float* lse,
                                 float* part_acc, float* part_ml, int n, int S, int H, int NH, int chunk, void* stream) {
    if (n == 0) return 0;
    const int rc = pool_check(x, x_sb, x_ss, mask, qt, n, S, H, NH);
    if (rc) return rc;
    if (!pooled || !lse || !part_acc || !part_ml) return BRA_ERR_ARG;
    const int rows = pool_chunk(n, S, chunk), nsplit = (S + rows - 1) / rows;
    const int smem = 32 * H + kPoolTile * kPoolNH * 4 + 64 + kPoolTile;
    BRA_ALLOW_SMEM((attn_pool_kernel<false>), smem);
    BRA_LAUNCH((attn_pool_kernel<false>), dim3(nsplit, n), dim3(kPoolThreads), smem, stream, (const bf16_t*)x, x_sb, x_ss,
               (const uint8_t*)mask, qt, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, part_acc, part_ml, S,
               H, rows);
    BRA_LAUNCH(attn_pool_merge_kernel, dim3((H + 255) / 256, kPoolNH, n), dim3(256), 0, stream, (const float*)part_acc,
               (const float*)part_ml, pooled, lse, nsplit, H);
    return BRA_LAUNCH_STATUS();
}

extern "C" int bra_attn_pool_bwd(const void* x, long x_sb, long x_ss, const void* mask, const float* qt, const float* pooled,
                                 const float* lse, const float* g, float* dqt, float* part, int n, int S, int H, int NH, int chunk,
                                 void* stream) {
    const int rc = pool_check(x, x_sb, x_ss, mask, qt, n, S, H, NH);
    if (rc) return rc;
    if (!pooled || !lse || !g || !dqt || !part || n == 0) return BRA_ERR_ARG;
    const int rows = pool_chunk(n, S, chunk), nsplit = (S + rows - 1) / rows;
    const int smem = 64 * H + 2 * kPoolTile * kPoolNH * 4 + 64 + kPoolTile;
    BRA_ALLOW_SMEM((attn_pool_kernel<true>), smem);
    BRA_LAUNCH((attn_pool_kernel<true>), dim3(nsplit, n), dim3(kPoolThreads), smem, stream, (const bf16_t*)x, x_sb, x_ss,
               (const uint8_t*)mask, qt, g, pooled, lse, part, (float*)nullptr, S, H, rows);
    const int n4 = kPoolNH * H / 4;
    BRA_LAUNCH(attn_pool_sum_kernel, dim3((n4 + 255) / 256), dim3(256), 0, stream, (const float*)part, dqt, n * nsplit, n4);
    return BRA_LAUNCH_STATUS();
}
